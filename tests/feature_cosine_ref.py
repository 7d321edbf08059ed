"""numpy restatement of the feature-matching term of the distillation cell (csrc/spv_distill.hip: spv_feature_cosine_*; reference
spectre_vit/repl/train.py:306, 343-346):

    feat = 1 - mean_r cos_r,   cos_r = s_r . t_r / (|s_r| |t_r|)
    ds_r = -go * w / rows * (t_r / |t_r| - cos_r * s_r / |s_r|) / |s_r|

with the one stated deviation: a row whose |s| or |t| is below TINY = 1e-12 has cos_r = 0 and a zero gradient row.
``forward`` / ``backward`` are the float64 statement (tests/test_feature_distill.py holds them to torch's F.normalize +
nn.CosineSimilarity + autograd).  ``forward32`` / ``backward32`` state the same in float32 with every dot product accumulated
sequentially, element by element; they serve only to size the GPU tests' bars (4 x their own gap to float64 on the same inputs)."""
import numpy as np

TINY = 1e-12


def forward(s, t):
    """float64 -> (feat, stat3 [3][rows] = |s|, |t|, cos)"""
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    ns, nt = np.sqrt((s * s).sum(1)), np.sqrt((t * t).sum(1))
    tiny = (ns < TINY) | (nt < TINY)
    with np.errstate(all="ignore"):
        cos = np.where(tiny, 0.0, (s * t).sum(1) / ns / nt)
    return 1.0 - cos.mean(), np.stack([ns, nt, cos])


def backward(s, t, stat3, go=1.0, w=1.0):
    """float64 -> ds [rows][width]"""
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    ns, nt, cos = (np.asarray(v, np.float64)[:, None] for v in stat3)
    tiny = (ns < TINY) | (nt < TINY)
    with np.errstate(all="ignore"):
        ds = -go * w / s.shape[0] * ((t / nt - cos * (s / ns)) / ns)
    return np.where(tiny, 0.0, ds)


def _dot32(a, b):
    """row-wise dot product, float32, one element after the other"""
    acc = np.zeros(a.shape[0], np.float32)
    for c in range(a.shape[1]):
        acc = (acc + a[:, c] * b[:, c]).astype(np.float32)
    return acc


def forward32(s, t):
    """the float32 sequential restatement -> (feat, stat3), float32"""
    s, t = np.asarray(s, np.float32), np.asarray(t, np.float32)
    ns, nt = np.sqrt(_dot32(s, s)), np.sqrt(_dot32(t, t))
    tiny = (ns < np.float32(TINY)) | (nt < np.float32(TINY))
    with np.errstate(all="ignore"):
        cos = np.where(tiny, np.float32(0), _dot32(s, t) / ns / nt).astype(np.float32)
    acc = np.float32(0)
    for c in cos:
        acc = np.float32(acc + c)
    return np.float32(1) - acc / np.float32(s.shape[0]), np.stack([ns, nt, cos])


def backward32(s, t, stat3, go=1.0, w=1.0):
    s, t = np.asarray(s, np.float32), np.asarray(t, np.float32)
    ns, nt, cos = (np.asarray(v, np.float32)[:, None] for v in stat3)
    tiny = (ns < np.float32(TINY)) | (nt < np.float32(TINY))
    k = np.float32(-np.float32(go) * np.float32(w) / np.float32(s.shape[0]))
    with np.errstate(all="ignore"):
        ds = (k * ((t / nt - cos * (s / ns)) / ns)).astype(np.float32)
    return np.where(tiny, np.float32(0), ds)


def rows_in_range(rng, rows, width, lo=1e-3, hi=1e3):
    """float32 [rows][width] whose row norms are log-uniform in [lo, hi]"""
    x = rng.standard_normal((rows, width))
    x /= np.sqrt((x * x).sum(1, keepdims=True))
    x *= np.exp(rng.uniform(np.log(lo * 1.01), np.log(hi / 1.01), size=(rows, 1)))
    return x.astype(np.float32)
