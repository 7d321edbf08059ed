"""The case tables of tests/test_gpu_embed_edges.py (csrc/spv_patch.hip with csrc/spv_prologue_core.h: spv_patchify, spv_patchify_u8,
spv_embed_posbias, spv_embed_cls_rows, spv_spectral_fold[_bf16], spv_spectral_fold_bwd, spv_embed_bwd, spv_dropout), their seeded
inputs, a host restatement of each dispatch rule written in that source, and what each case is judged by (tests/edge_judge.py holds the
judging function both test files share).
tests/test_embed_ref.py shows on the CPU that the tables reach every branch, that a float32 restatement of each kernel passes the
judge on exactly these inputs and that plausible mistakes do not.

Shapes are (B, C, H, W, P), K = C P P, Np = (H / P)(W / P).  expect(family, case) -> {output name: Spec}: kind "bits" holds the output
to the reference bit for bit (a copy, a cast, a single IEEE operation, the add-multiply-round of dtok); kind "bar" holds
|got - ref| elementwise within  c 2^-24 S_i (+ half a bf16 ulp of the reference for bf16 outputs), S_i the float64 sum of the absolute
values of the terms of element i; where S_i = 0 -- the CLS slot and the padding of the uint8 patch rows -- the output must be the
reference's zero, sign included.

c is four times the floor, rounded up: the floor is the worst err_i / (2^-24 S_i) of the float32 restatement of embed_ref.py against
float64 on exactly these inputs (tests/test_embed_ref.py prints it and asserts floor <= c / 4); the factor 4 leaves room for fused
multiply-adds, another fixed summation tree and the few-ulp device cospif.  Measured floors and the bars they set:

    patchify_u8   floor 1.87   c = 8
    fold          floor 4.28   c = 18      (P = 1: 0.76, P = 2: 3.32, P = 16: 4.27, P = 64: 4.02)
    fold_bwd      floor 3.34   c = 14      (dw, the scratch product, dfreq_h and dfreq_w together)
    embed_bwd     floor 2.39   c = 10      (dpos, dbias and dcls together)"""
import functools
import zlib
from collections import namedtuple

import numpy as np

import dropout_ref as D
import embed_ref as R
from attention_edge_cases import SEED
from edge_judge import EPS, F32, LIMIT_BYTES, Spec, cast, cdiv, floor_ratio, half_ulp, round8, values, verdict  # noqa: F401  (re-exported)
from embed_ref import EB_GS
from permut_edge_cases import CODE, DTYPES, ES, bits  # noqa: F401

C_BAR = dict(patchify_u8=8, fold=18, fold_bwd=14, embed_bwd=10)
P_DROP = 0.3


# ------------------------------------------------------------------------------------------------------------------ dispatch
PATCH_CAP = 4096       # patch_ew_blocks: min(cdiv(n, 256), 4096) workgroups of 256 threads
EB_HB = 8              # spv_embed_bwd: of the EB_GS = 16 samples of a workgroup's row-group, the rows in flight per thread


def patch_trips(work_items):
    """trips of the capped grid-stride loop of spv_patch.hip over `work_items` items"""
    return cdiv(work_items, 256 * min(cdiv(work_items, 256), PATCH_CAP))


def geometry(c):
    """(Np, K) of a case with fields C H W P"""
    return (c.H // c.P) * (c.W // c.P), c.C * c.P * c.P


def out_elems(c):
    Np, K = geometry(c)
    return {0: c.B * Np * c.ld, 1: K * c.ld, 2: c.B * (Np + 1) * c.ld}[c.mode]


def patchify_vec4(c):
    """spv_patchify: the four-pixel kernel serves row-major outputs of 4-aligned patches, widths and ld through 16-byte-aligned pointers"""
    return c.mode != 1 and c.P % 4 == 0 and c.W % 4 == 0 and c.ld % 4 == 0 and c.off == ""


def patchify_items(c):
    return out_elems(c) // 4 if patchify_vec4(c) else out_elems(c)


def embed_bwd_plan(c):
    """spv_embed_bwd: dict(groups, last: samples of the ragged last group, cblocks: 256-thread column blocks of 8-element vectors,
    fold: (8-batches, tail) of the group fold, bias: (8-batches, tail) of the bias loop over t >= 1)"""
    groups, TE = cdiv(c.B, EB_GS), c.T * c.E
    return dict(groups=groups, last=c.B - (groups - 1) * EB_GS, cblocks=cdiv(TE // 8, 256), fold=(groups // 8, groups % 8),
                bias=((c.T - 1) // 8, (c.T - 1) % 8))


def mask_crossings(c):
    """(a 4096-element key block ends inside a sample, a sample ends inside a key block that the next sample shares, two consecutive
    samples begin in different key blocks)"""
    TE = c.T * c.E
    inside = any(b * TE // 4096 != ((b + 1) * TE - 1) // 4096 for b in range(c.B))
    shared = any(b * TE % 4096 != 0 for b in range(1, c.B))
    differ = any((b - 1) * TE // 4096 != b * TE // 4096 for b in range(1, c.B))
    return inside, shared, differ


# ------------------------------------------------------------------------------------------------------------------ tables
PF = namedtuple("PF", "dtype B C H W P mode ld off", defaults=("",))
U8 = namedtuple("U8", "dtype B C H W P mode ld")
PB = namedtuple("PB", "Np E cls")
CR = namedtuple("CR", "dtype B T E")
SF = namedtuple("SF", "E C P")
EB = namedtuple("EB", "dtype B T E gcls p dtok")
DR = namedtuple("DR", "dtype n p")

PATCHIFY_CASES = [PF(dt, *v) for dt in DTYPES for v in (
    (3, 3, 8, 8, 4, 2, 48),                                   # the training call: token rows, ld = K, four pixels per thread
    (3, 3, 8, 8, 4, 0, 52), (3, 3, 8, 8, 4, 2, 56),           # padding columns
    (3, 3, 8, 8, 2, 2, 12),                                   # the element kernel by each refusing condition on its own: P = 2
    (2, 1, 28, 28, 7, 2, 49), (2, 1, 28, 28, 7, 0, 56),       # P = 7 with ld odd and ld a multiple of 4
    (2, 3, 9, 10, 4, 2, 48),                                  # W = 10 (and H = 9: the leftover pixels are unused)
    (3, 3, 8, 8, 4, 0, 50),                                   # ld off the four-element store
    (3, 3, 8, 8, 4, 2, 48, "out"), (3, 3, 8, 8, 4, 2, 48, "img"),       # a pointer one 8-byte step off 16-byte alignment
    (3, 3, 8, 8, 4, 1, 16),                                   # transposed, ld = round8(rows) > rows = 12
    (1, 3, 8, 8, 4, 2, 48), (1, 3, 8, 8, 4, 1, 8),            # B = 1
    (22, 3, 128, 128, 4, 1, 22528),                           # second trip: 1 081 344 elements against 4096 x 256 threads
    (22, 3, 256, 256, 4, 2, 48))]                             # second trip of the four-pixel kernel: 1 081 608 vectors

U8_CASES = [U8(dt, *v) for dt in DTYPES for v in (
    (2, 3, 16, 16, 4, 0, 52), (2, 3, 16, 16, 4, 1, 40), (2, 3, 16, 16, 4, 2, 56), (2, 1, 28, 28, 7, 0, 49), (2, 1, 28, 28, 7, 1, 32),
    (2, 1, 28, 28, 7, 2, 56), (1, 1, 16, 16, 4, 2, 16), (2, 3, 28, 28, 7, 2, 152), (2, 3, 28, 28, 7, 0, 147),
    (22, 3, 128, 128, 4, 2, 48))]                             # second trip: 1 082 400 elements

POSBIAS_CASES = [PB(n, e, cls) for n, e in ((3, 5), (4, 64), (1, 8), (2048, 513)) for cls in (1, 0)]
CLS_ROWS_CASES = [CR(dt, *v) for dt in DTYPES for v in ((3, 5, 8), (1, 1, 5), (2049, 1, 513))]

FOLD_CASES = [SF(5, 3, p) for p in (1, 2, 3, 4, 7, 8, 16)] + [SF(2, 1, p) for p in (32, 64)] + [
    SF(343, 3, 2), SF(512, 2, 2),          # E C = 1029 and 1024 against freq_weight_grad_kernel's 1024 threads
    SF(8192, 33, 2)]                       # second trip of the fold (1 081 344 elements) and of its backward (1 081 344)
FOLD_BWD_REFUSED = [SF(2, 1, 65)]

_EB_SHAPES = ((1, 1, 8), (8, 2, 8), (9, 5, 24), (16, 9, 8), (17, 10, 24), (33, 9, 24), (120, 17, 8), (130, 2, 24), (9, 9, 256), (17, 1, 256))
_EB_THIRD = (("fp32", 0, 0.0, 0), ("bf16", 0, 0.0, 0), ("fp32", 1, 0.0, 1), ("bf16", 1, 0.0, 1))
EMBED_BWD_CASES = [EB(v[0], *s, *v[1:]) for i, s in enumerate(_EB_SHAPES) for v in (
    (DTYPES[i % 2], 1, P_DROP, 1), (DTYPES[1 - i % 2], 0, P_DROP, 1), _EB_THIRD[i % 4])]
EMBED_BWD_REFUSED = [(EB("fp32", 2, 3, 12, 0, 0.0, 1), "multiple of 8"), (EB("bf16", 2, 3, 8, 0, P_DROP, 0), "dtok may be NULL only")]

DROP_BIG = 8388621         # 1 048 577 8-element vectors against 4096 x 256 threads, and a 5-element tail
DROPOUT_CASES = [DR(dt, n, p) for dt in DTYPES for p in (0.0, P_DROP) for n in (1, 7, 8, 9, 4095, 4096, 4097, 8200, DROP_BIG)]

ALL = dict(patchify=PATCHIFY_CASES, patchify_u8=U8_CASES, posbias=POSBIAS_CASES, cls_rows=CLS_ROWS_CASES, fold=FOLD_CASES, fold_bwd=FOLD_CASES,
           embed_bwd=EMBED_BWD_CASES, dropout=DROPOUT_CASES)
for _cases in ALL.values():
    assert len(set(_cases)) == len(_cases)


def case_id(c):
    return "-".join(str(v) if v != "" else "_" for v in c)


def device_bytes(family, c):
    """bytes of device buffers a case allocates (sentinels aside), by arithmetic from the table"""
    if family == "patchify":
        return 4 * c.B * c.C * c.H * c.W + out_elems(c) * ES[c.dtype]
    if family == "patchify_u8":
        return c.B * c.C * c.H * c.W + 8 * c.C + out_elems(c) * ES[c.dtype]
    if family == "posbias":
        return 4 * ((c.Np + 1) * c.E + 2 * c.E + (c.Np + 1) * c.E)
    if family == "cls_rows":
        return 4 * (c.E + c.T * c.E) + c.B * c.T * c.E * ES[c.dtype]
    if family in ("fold", "fold_bwd"):
        Pv = c.P // 2 + 1
        spectrum, full = 4 * c.E * c.C * c.P * Pv, 4 * c.E * c.C * c.P * c.P
        return spectrum + 2 * full + full // 2 if family == "fold" else full + 3 * spectrum + 8 * (c.P + Pv)
    if family == "embed_bwd":
        n = c.B * c.T * c.E
        return ES[c.dtype] * (2 * n + c.B * c.E) + 4 * (cdiv(c.B, EB_GS) * c.T * c.E + c.T * c.E + 2 * c.E)
    return 2 * c.n * ES[c.dtype]


# ------------------------------------------------------------------------------------------------------------------ inputs
def rng_of(c, tag=""):
    return np.random.default_rng(zlib.crc32(f"{type(c).__name__}/{case_id(c)}/{tag}".encode()))


def byte_image(rng, B, H, W, C):
    """uint8 [B, H, W, C] whose first image holds every byte value in every channel"""
    img = rng.integers(0, 256, (B, H, W, C), dtype=np.uint8)
    assert H * W >= 256
    for ch in range(C):
        flat = img[0, :, :, ch].reshape(-1)        # (a copy where the channel is strided)
        flat[rng.permutation(H * W)[:256]] = np.arange(256, dtype=np.uint8)
        img[0, :, :, ch] = flat.reshape(H, W)
    assert all(len(np.unique(img[0, :, :, ch])) == 256 for ch in range(C))
    img.setflags(write=False)
    return img


def pattern(shape, dtype):
    """the fixed content of a buffer a kernel must only partly write: small integers, exact in bf16"""
    return cast((np.arange(int(np.prod(shape))) % 251 - 125.0).reshape(shape), dtype)


@functools.lru_cache(maxsize=4)
def inputs(family, c):
    """{name: array of storage values (float64; the uint8 image as it is)} of a case; an absent optional input is None"""
    rng = rng_of(c)
    if family == "patchify":
        rng = rng_of(c._replace(off=""))          # a misaligned case reads the image of its aligned twin
        return dict(img=values(rng, (c.B, c.C, c.H, c.W), "fp32"))
    if family == "patchify_u8":
        return dict(img=byte_image(rng, c.B, c.H, c.W, c.C), mean=cast(rng.uniform(0.3, 0.6, c.C), "fp32"), inv_std=cast(1.0 / rng.uniform(0.2, 0.3, c.C), "fp32"))
    if family == "posbias":
        return dict(pos=values(rng, (c.Np + 1, c.E), "fp32"), bias=values(rng, (c.E,), "fp32", "finite"),
                    cls=values(rng, (c.E,), "fp32", "finite") if c.cls else None)
    if family == "cls_rows":
        return dict(cls=values(rng, (c.E,), "fp32", "finite"), pos=values(rng, (c.T, c.E), "fp32"), tokens=pattern((c.B, c.T, c.E), c.dtype))
    if family in ("fold", "fold_bwd"):
        Pv = c.P // 2 + 1
        d = dict(w=values(rng, (c.E, c.C, c.P, Pv), "fp32", ""), fh=values(rng, (c.P,), "fp32", ""), fw=values(rng, (Pv,), "fp32", ""))
        if family == "fold_bwd":
            d["dwf"] = values(rng, (c.E, c.C, c.P, c.P), "fp32", "")
        return d
    if family == "embed_bwd":
        return dict(g=values(rng, (c.B, c.T, c.E), c.dtype, "finite"), gcls=values(rng, (c.B, c.E), c.dtype, "finite") if c.gcls else None)
    return dict(x=values(rng, (c.n,), c.dtype, "finite_huge"))      # (no inf: inf times a dropped element's 0 is NaN)


def seed_of(c):
    return SEED if c.p > 0 else 0


# ------------------------------------------------------------------------------------------------------------------ the judge
def bar_of(name, ref, S, dtype):
    return C_BAR[name] * EPS * S + half_ulp(ref, dtype)


def embed_dtok_ref(c):
    """dtok by dropout_ref.keep's mask over 4096-element rows of the flat tensor: (g + gcls on row 0) * keep / (1 - p)"""
    d = inputs("embed_bwd", c)
    x = np.array(d["g"], np.float64).astype(F32)
    if c.gcls:
        x[:, 0, :] = x[:, 0, :] + np.asarray(d["gcls"], np.float64).astype(F32)
    if c.p > 0:
        keep = D.keep(seed_of(c), cdiv(x.size, 4096), 4096, c.p).reshape(-1)[:x.size].reshape(x.shape)
        x = x * np.where(keep, D.inv_keep(c.p), F32(0)).astype(F32)
    return cast(x, c.dtype)


@functools.lru_cache(maxsize=4)
def expect(family, c):
    d = inputs(family, c)
    if family == "patchify":
        return dict(out=Spec("bits", R.patchify_ref(d["img"], c.P, c.mode, c.ld, c.dtype), c.dtype))
    if family == "patchify_u8":
        out, S = R.patchify_u8_ref(d["img"], d["mean"], d["inv_std"], c.P, c.mode, c.ld)
        return dict(out=Spec("bar", out, c.dtype, bar_of("patchify_u8", out, S, c.dtype)))
    if family == "posbias":
        return dict(out=Spec("bits", R.posbias_ref(d["pos"], d["bias"], d["cls"]), "fp32"))
    if family == "cls_rows":
        return dict(tokens=Spec("bits", R.cls_rows_ref(d["tokens"], d["cls"], d["pos"], c.dtype), c.dtype))
    if family == "fold":
        wf, S = R.fold_ref(d["w"], d["fh"], d["fw"])
        return dict(wf=Spec("bar", wf, "fp32", bar_of("fold", wf, S, "fp32")))
    if family == "fold_bwd":
        ref, S = R.fold_bwd_ref(d["dwf"], d["w"], d["fh"], d["fw"])
        return {k: Spec("bar", ref[k], "fp32", bar_of("fold_bwd", ref[k], S[k], "fp32")) for k in ref}
    if family == "embed_bwd":
        dtok = embed_dtok_ref(c)
        ref, S = R.embed_bwd_ref(dtok)
        out = {k: Spec("bar", ref[k], "fp32", bar_of("embed_bwd", ref[k], S[k], "fp32")) for k in ref}
        if c.dtok:
            out["dtok"] = Spec("bits", dtok, c.dtype)
        return out
    return dict(y=Spec("bits", R.dropout_ref(d["x"], c.p, seed_of(c), c.dtype), c.dtype))


def restate(family, c, mutant=None):
    """{output name: float64 storage values} of the float32 restatement of a case"""
    d = inputs(family, c)
    if family == "patchify":
        return dict(out=R.patchify_restate(d["img"], c.P, c.mode, c.ld, c.dtype, mutant))
    if family == "patchify_u8":
        return dict(out=R.patchify_u8_restate(d["img"], d["mean"], d["inv_std"], c.P, c.mode, c.ld, c.dtype, mutant))
    if family == "posbias":
        return dict(out=R.posbias_restate(d["pos"], d["bias"], d["cls"], mutant))
    if family == "cls_rows":
        return dict(tokens=R.cls_rows_restate(d["tokens"], d["cls"], d["pos"], c.dtype))
    if family == "fold":
        return dict(wf=R.fold_restate(d["w"], d["fh"], d["fw"], mutant))
    if family == "fold_bwd":
        return R.fold_bwd_restate(d["dwf"], d["w"], d["fh"], d["fw"])
    if family == "embed_bwd":
        dtok = R.embed_dtok(d["g"], d["gcls"], c.p, seed_of(c), c.dtype, mutant)
        out = R.embed_bwd_restate(dtok, mutant)
        if c.dtok:
            out["dtok"] = dtok
        return out
    return dict(y=R.dropout_restate(d["x"], c.p, seed_of(c), c.dtype, mutant))
