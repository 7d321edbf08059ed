"""The patch-embedding kernels of csrc/spv_patch.hip and csrc/spv_prologue_core.h (spv_patchify, spv_patchify_u8, spv_embed_posbias,
spv_embed_cls_rows, spv_spectral_fold[_bf16], spv_spectral_fold_bwd, spv_embed_bwd, spv_dropout) at their edges against
tests/embed_ref.py's float64 references: raw C-ABI calls within include/spv.h's contract, one per entry point, in eager mode, on the
current stream, then one synchronize.

Every case (tests/embed_edge_cases.py) asserts, in this order: memory -- the sentinels around every buffer are intact (workspaces have
exactly the size the header asks for), every input is bit-identical afterwards, every output element is written (outputs start as NaN),
and the token rows spv_embed_cls_rows must not touch keep their pattern; values -- patch rows, position rows, CLS rows, dtok and dropout
bit for bit (padding and the CLS slot exactly + 0), the uint8 patch rows, the spectral fold with its backward and the embedding
backward's sums within the elementwise bars derived in embed_edge_cases, the worst ratio to the bar printed.  Inputs carry +-0,
subnormals, +-inf and the largest finite value where the operation tolerates them.  tests/test_embed_ref.py shows on the CPU that a
float32 restatement of each kernel passes this judge on these inputs and that plausible mistakes do not."""
import numpy as np
import pytest
import torch

import embed_edge_cases as C
from embed_ref import cast
from test_gpu_ops import dev
from test_gpu_permut_edges import buf, raw_bits

pytestmark = pytest.mark.gpu

PAD, BYTE = 256, 0xA5


class GuardedBytes:
    """a uint8 tensor inside a larger allocation with PAD sentinel bytes either side"""

    def __init__(self, data):
        n = data.size
        self.big = torch.full((PAD + n + PAD,), BYTE, dtype=torch.uint8, device=dev())
        self.t = self.big[PAD:PAD + n].view(data.shape)
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(data)))
        self.data = data

    @property
    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.big[:PAD] == BYTE).all() and (self.big[-PAD:] == BYTE).all()) and np.array_equal(self.t.cpu().numpy(), self.data)


def _native():
    from spectre_vit import _native as n
    return n


def _st():
    from spectre_vit import hip_ops
    return hip_ops._stream()


def check_memory(ins, outs, data, scratch=()):
    for name, b in {**ins, **outs, **dict(scratch)}.items():
        assert b.intact(), f"{name}: sentinel overwritten"
    for name, b in ins.items():
        assert np.array_equal(raw_bits(b.t), C.bits(data[name], b.dtn).reshape(-1)), f"input {name} changed"


def judge(tag, family, case, outs, only=None):
    specs = C.expect(family, case)
    ok, worst = C.verdict({k: specs[k] for k in (only or specs)}, {k: b.f64() for k, b in outs.items()})
    print(f"EMBED {tag} {C.case_id(case)} worst ratio to the bar: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert ok, (tag, case, worst)


def ptr(b):
    return b.ptr if b is not None else 0


# ------------------------------------------------------------------------------------------------------------------ patch rows
def _patchify(c):
    d = C.inputs("patchify", c)
    ins = dict(img=buf((c.B, c.C, c.H, c.W), "fp32", d["img"], 2 if c.off == "img" else 0))
    outs = dict(out=buf(C.expect("patchify", c)["out"].ref.shape, c.dtype, off=8 // C.ES[c.dtype] if c.off == "out" else 0))
    assert ins["img"].ptr % 16 == (8 if c.off == "img" else 0) and outs["out"].ptr % 16 == (8 if c.off == "out" else 0)
    _native().call("spv_patchify", ins["img"].ptr, outs["out"].ptr, c.B, c.C, c.H, c.W, c.P, c.ld, c.mode, C.CODE[c.dtype], _st())
    torch.cuda.synchronize()
    check_memory(ins, outs, d)
    return outs


@pytest.mark.parametrize("case", C.PATCHIFY_CASES, ids=C.case_id)
def test_patchify_bit_for_bit(case):
    outs = _patchify(case)
    judge("patchify", "patchify", case, outs)
    if case.off:
        twin = _patchify(case._replace(off=""))
        assert np.array_equal(raw_bits(outs["out"].t), raw_bits(twin["out"].t)), "differs from the aligned call"


@pytest.mark.parametrize("case", C.U8_CASES, ids=C.case_id)
def test_patchify_u8_vs_float64(case):
    c, d = case, C.inputs("patchify_u8", case)
    img = GuardedBytes(d["img"])
    ins = dict(mean=buf((c.C,), "fp32", d["mean"]), inv_std=buf((c.C,), "fp32", d["inv_std"]))
    shape = C.expect("patchify_u8", c)["out"].ref.shape
    outs = dict(out=buf(shape, c.dtype))
    _native().call("spv_patchify_u8", img.ptr, ins["mean"].ptr, ins["inv_std"].ptr, outs["out"].ptr, c.B, c.C, c.H, c.W, c.P, c.ld, c.mode,
                   C.CODE[c.dtype], _st())
    torch.cuda.synchronize()
    assert img.intact(), "the image or its sentinels changed"
    check_memory(ins, outs, d)
    judge("patchify_u8", "patchify_u8", c, outs)


# ------------------------------------------------------------------------------------------------------------------ position / CLS rows
@pytest.mark.parametrize("case", C.POSBIAS_CASES, ids=C.case_id)
def test_posbias_bit_for_bit(case):
    c, d = case, C.inputs("posbias", case)
    ins = dict(pos=buf((c.Np + 1, c.E), "fp32", d["pos"]), bias=buf((c.E,), "fp32", d["bias"]))
    if c.cls:
        ins["cls"] = buf((c.E,), "fp32", d["cls"])
    outs = dict(out=buf((c.Np + c.cls, c.E), "fp32"))
    _native().call("spv_embed_posbias", ins["pos"].ptr, ins["bias"].ptr, ptr(ins.get("cls")), outs["out"].ptr, c.Np, c.E, _st())
    torch.cuda.synchronize()
    check_memory(ins, outs, d)
    judge("posbias", "posbias", c, outs)


@pytest.mark.parametrize("case", C.CLS_ROWS_CASES, ids=C.case_id)
def test_cls_rows_bit_for_bit_and_nothing_else_touched(case):
    c, d = case, C.inputs("cls_rows", case)
    ins = dict(cls=buf((c.E,), "fp32", d["cls"]), pos=buf((c.T, c.E), "fp32", d["pos"]))
    outs = dict(tokens=buf((c.B, c.T, c.E), c.dtype, d["tokens"]))       # a fixed pattern: only row 0 of every image may change
    _native().call("spv_embed_cls_rows", ins["cls"].ptr, ins["pos"].ptr, outs["tokens"].ptr, c.B, c.T, c.E, C.CODE[c.dtype], _st())
    torch.cuda.synchronize()
    check_memory(ins, outs, d)
    judge("cls_rows", "cls_rows", c, outs)


# ------------------------------------------------------------------------------------------------------------------ spectral fold
@pytest.mark.parametrize("case", C.FOLD_CASES, ids=C.case_id)
def test_spectral_fold_vs_float64(case):
    c, d = case, C.inputs("fold", case)
    Pv = c.P // 2 + 1
    ins = dict(w=buf((c.E, c.C, c.P, Pv), "fp32", d["w"]), fh=buf((c.P,), "fp32", d["fh"]), fw=buf((Pv,), "fp32", d["fw"]))
    full = (c.E, c.C, c.P, c.P)
    outs = dict(wf=buf(full, "fp32"), wf2=buf(full, "fp32"), wf_bf16=buf(full, "bf16"))
    _native().call("spv_spectral_fold", ins["w"].ptr, ins["fh"].ptr, ins["fw"].ptr, outs["wf"].ptr, c.E, c.C, c.P, _st())
    _native().call("spv_spectral_fold_bf16", ins["w"].ptr, ins["fh"].ptr, ins["fw"].ptr, outs["wf2"].ptr, outs["wf_bf16"].ptr, c.E, c.C, c.P, _st())
    torch.cuda.synchronize()
    check_memory(ins, outs, d)
    judge("fold", "fold", c, dict(wf=outs["wf"]))
    judge("fold_bf16", "fold", c, dict(wf=outs["wf2"]))
    # the bf16 copy is the RNE cast of the float32 output of the same call
    assert np.array_equal(raw_bits(outs["wf_bf16"].t), C.bits(cast(outs["wf2"].f64(), "bf16"), "bf16").reshape(-1)), "wf_bf16 is not the cast of wf"


@pytest.mark.parametrize("case", C.FOLD_CASES, ids=C.case_id)
def test_spectral_fold_bwd_vs_float64(case):
    c, d = case, C.inputs("fold_bwd", case)
    Pv = c.P // 2 + 1
    ins = dict(dwf=buf((c.E, c.C, c.P, c.P), "fp32", d["dwf"]), w=buf((c.E, c.C, c.P, Pv), "fp32", d["w"]), fh=buf((c.P,), "fp32", d["fh"]),
               fw=buf((Pv,), "fp32", d["fw"]))
    # gw: the scratch of include/spv.h, exactly embed chans patch (patch / 2 + 1) floats -- the products the frequency sums read
    outs = dict(dw=buf((c.E, c.C, c.P, Pv), "fp32"), gw=buf((c.E, c.C, c.P, Pv), "fp32"), dfh=buf((c.P,), "fp32"), dfw=buf((Pv,), "fp32"))
    _native().call("spv_spectral_fold_bwd", ins["dwf"].ptr, ins["w"].ptr, ins["fh"].ptr, ins["fw"].ptr, outs["dw"].ptr, outs["dfh"].ptr,
                   outs["dfw"].ptr, outs["gw"].ptr, c.E, c.C, c.P, _st())
    torch.cuda.synchronize()
    check_memory(ins, outs, d)
    judge("fold_bwd", "fold_bwd", c, outs)


@pytest.mark.parametrize("case", C.FOLD_BWD_REFUSED, ids=C.case_id)
def test_spectral_fold_bwd_refuses_a_patch_over_64(case):
    c = case
    Pv = c.P // 2 + 1
    ins = [buf(s, "fp32", np.ones(s)) for s in ((c.E, c.C, c.P, c.P), (c.E, c.C, c.P, Pv), (c.P,), (Pv,))]
    outs = [buf(s, "fp32") for s in ((c.E, c.C, c.P, Pv), (c.P,), (Pv,), (c.E, c.C, c.P, Pv))]
    with pytest.raises(RuntimeError, match="spv_spectral_fold_bwd"):
        _native().call("spv_spectral_fold_bwd", *[b.ptr for b in ins + outs], c.E, c.C, c.P, _st())
    torch.cuda.synchronize()
    assert all(b.intact() for b in ins + outs) and all(bool(torch.isnan(b.t).all()) for b in outs), "a refused call wrote"


# ------------------------------------------------------------------------------------------------------------------ embedding backward
def _embed_bwd(c, d):
    groups = _native().call("spv_embed_bwd_groups", c.B)
    assert groups == C.embed_bwd_plan(c)["groups"]
    ins = dict(g=buf((c.B, c.T, c.E), c.dtype, d["g"]))
    if c.gcls:
        ins["gcls"] = buf((c.B, c.E), c.dtype, d["gcls"])
    outs = dict(dpos=buf((c.T, c.E), "fp32"), dbias=buf((c.E,), "fp32"), dcls=buf((c.E,), "fp32"))
    if c.dtok:
        outs["dtok"] = buf((c.B, c.T, c.E), c.dtype)
    partials = buf((groups * c.T * c.E,), "fp32")        # exactly what include/spv.h asks for
    call = lambda: _native().call("spv_embed_bwd", ins["g"].ptr, ptr(ins.get("gcls")), ptr(outs.get("dtok")), partials.ptr, outs["dpos"].ptr,
                                  outs["dbias"].ptr, outs["dcls"].ptr, c.B, c.T, c.E, c.p, C.seed_of(c), C.CODE[c.dtype], _st())
    return ins, outs, partials, call


@pytest.mark.parametrize("case", C.EMBED_BWD_CASES, ids=C.case_id)
def test_embed_bwd_vs_float64(case):
    c, d = case, C.inputs("embed_bwd", case)
    ins, outs, partials, call = _embed_bwd(c, d)
    call()
    torch.cuda.synchronize()
    check_memory(ins, outs, d, dict(partials=partials))
    judge("embed_bwd", "embed_bwd", c, outs)
    assert np.array_equal(raw_bits(outs["dcls"].t), raw_bits(outs["dpos"].t[0])), "dcls is not dpos[0]"


@pytest.mark.parametrize("case,why", C.EMBED_BWD_REFUSED, ids=[C.case_id(c) for c, _ in C.EMBED_BWD_REFUSED])
def test_embed_bwd_refusals(case, why):
    c = case
    rng = np.random.default_rng(3)
    ins, outs, partials, call = _embed_bwd(c, dict(g=cast(rng.standard_normal((c.B, c.T, c.E)), c.dtype), gcls=None))
    with pytest.raises(RuntimeError, match=why):
        call()
    torch.cuda.synchronize()
    assert all(b.intact() for b in list(ins.values()) + list(outs.values()) + [partials])
    assert all(bool(torch.isnan(b.t).all()) for b in outs.values()), "a refused call wrote"


# ------------------------------------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("case", C.DROPOUT_CASES, ids=C.case_id)
def test_dropout_bit_for_bit(case):
    c, d = case, C.inputs("dropout", case)
    ins, outs = dict(x=buf((c.n,), c.dtype, d["x"])), dict(y=buf((c.n,), c.dtype))
    _native().call("spv_dropout", ins["x"].ptr, outs["y"].ptr, c.n, c.p, C.seed_of(c), C.CODE[c.dtype], _st())
    torch.cuda.synchronize()
    check_memory(ins, outs, d)
    judge("dropout", "dropout", c, outs)


@pytest.mark.parametrize("which", ["x", "y"])
def test_dropout_refuses_a_misaligned_pointer(which):
    x, y = buf((16,), "fp32", np.ones(16), 2 if which == "x" else 0), buf((16,), "fp32", off=2 if which == "y" else 0)
    with pytest.raises(RuntimeError, match="spv_dropout"):
        _native().call("spv_dropout", x.ptr, y.ptr, 16, 0.3, C.SEED, C.CODE["fp32"], _st())
    torch.cuda.synchronize()
    assert x.intact() and y.intact() and bool(torch.isnan(y.t).all()), "a refused call wrote"
