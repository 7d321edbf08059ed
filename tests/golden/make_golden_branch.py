"""Generate tests/golden/model_spectre_branch.npz (and its post-AdamW half, model_spectre_branch_after.npz) by EXECUTING the reference's SpectreBranch
(spectre_vit/models/spectre_branch/spectre_branch.py).

Run in the build container only (the reference is mounted read-only and never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_branch.py

Like make_golden.py: the reference module is imported (not copied), its weights are drawn in fp32 under a fixed seed, it is
switched to float64 and run with dropout 0.  Only arrays are written.  The model has 9.6 M parameters, so the weights are NOT
stored: the tests rebuild them from the seed and the file holds per-tensor init checksums instead (sum, sum of |w|, 32 strided
values).  The post-AdamW weights go to a second file so that each stays under 1 MiB.  Gradients and post-AdamW weights are stored in full up to 16 k elements; larger tensors as row sums, column sums (over
the tensor viewed as in matrix()) and 8 full rows; all stored as fp32.
"""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("SPV_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

from spectre_vit.models.spectre_branch.spectre_branch import SpectreBranch, SpectreMix  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

SEED = 1234
CFG = dict(img_size=32, patch_size=4, in_channels=3, num_classes=100, embed_dim=768, num_encoders=4, num_heads=8, hidden_dim=256,
           dropout=0.0, activation="gelu")
BATCH = 4
FULL = 16384          # tensors up to this many elements are stored whole
ROWS = 8              # full rows kept of a larger tensor
FEAT_ROWS = 8         # sampled (sample, token) rows of each feats[k]


def npy(t):
    return t.detach().cpu().numpy()


def strided(a, n=32):
    f = a.reshape(-1)
    return f[np.linspace(0, f.size - 1, n).astype(np.int64)]


def row_index(n):
    return np.linspace(0, n - 1, ROWS).astype(np.int64)


def matrix(a):
    """the 2-D view the summaries are taken over: (shape[0], -1), or (-1, shape[-1]) when shape[0] == 1 (position embeddings)"""
    return a.reshape(-1, a.shape[-1]) if a.shape[0] == 1 else a.reshape(a.shape[0], -1)


def summary(prefix, a, d):
    """the tensor whole, or (row sums, column sums, 8 rows) of its (shape[0], -1) view"""
    a = np.asarray(a, dtype=np.float64)
    if a.size <= FULL:
        d[prefix] = a.astype(np.float32)
        return
    m = matrix(a)
    d[prefix + ".rowsum"] = m.sum(1).astype(np.float32)
    d[prefix + ".colsum"] = m.sum(0).astype(np.float32)
    d[prefix + ".rows"] = m[row_index(m.shape[0])].astype(np.float32)


def model_fixture():
    d = {}
    torch.manual_seed(SEED)
    m = SpectreBranch(**CFG)
    sd = m.state_dict()
    d["keys"] = np.array(list(sd.keys()))
    d["shapes"] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], dtype=np.int64)
    for k, v in sd.items():
        a = npy(v).astype(np.float64)
        d["init." + k] = np.concatenate([[a.sum(), np.abs(a).sum()], strided(a)])
    m = m.double()
    m.train()
    g = torch.Generator().manual_seed(SEED + 1)
    img = torch.randn(BATCH, 3, CFG["img_size"], CFG["img_size"], generator=g).double()
    labels = torch.randint(0, CFG["num_classes"], (BATCH,), generator=g)
    d["img"], d["labels"] = npy(img).astype(np.float32), npy(labels)
    img = torch.from_numpy(d["img"]).double()   # the tests feed the fp32 image
    _, feats = m.encoder_blocks.spectre_branch(img)
    n_tok = feats[0].shape[1]
    sel = np.linspace(0, BATCH * n_tok - 1, FEAT_ROWS).astype(np.int64)
    d["feat_rows"] = sel
    for k, f in enumerate(feats):
        d[f"feats.{k}"] = npy(f).reshape(BATCH * n_tok, -1)[sel].astype(np.float32)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01)
    logits, cls = m(img, return_features=True)
    loss = torch.nn.CrossEntropyLoss()(logits, labels)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    d["logits"], d["cls"], d["loss"] = npy(logits).astype(np.float32), npy(cls).astype(np.float32), np.array(loss.item())
    for k, p in m.named_parameters():
        if p.grad is None:
            d["nograd." + k] = np.array(1)
        else:
            summary("grad." + k, npy(p.grad), d)
    opt.step()
    for k, p in m.named_parameters():
        summary("after." + k, npy(p), d)
    d["cfg.batch"] = np.array(BATCH)
    d["cfg.seed"] = np.array(SEED)
    return d


def mix_fixture():
    d = {}
    torch.manual_seed(77)
    m = SpectreMix(64, 2, 5).double()
    d.update({"mix.sd." + k: npy(v).astype(np.float32) for k, v in m.state_dict().items()})
    g = torch.Generator().manual_seed(78)
    x = torch.randn(3, 5, 64, generator=g).double().requires_grad_(True)
    dy = torch.randn(3, 5, 64, generator=g).double()
    y = m(x)
    y.backward(dy)
    d["mix.x"], d["mix.dy"], d["mix.y"], d["mix.dx"] = npy(x).astype(np.float32), npy(dy).astype(np.float32), npy(y), npy(x.grad)
    d.update({"mix.grad." + k: npy(p.grad) for k, p in m.named_parameters()})
    return d


def main():
    d = model_fixture()
    d.update(mix_fixture())
    after = {k: v for k, v in d.items() if k.startswith("after.")}
    rest = {k: v for k, v in d.items() if not k.startswith("after.")}
    for name, part in (("model_spectre_branch.npz", rest), ("model_spectre_branch_after.npz", after)):
        path = os.path.join(OUT, name)
        np.savez_compressed(path, **part)
        print(path, os.path.getsize(path), "bytes,", len(part), "arrays")


if __name__ == "__main__":
    main()
