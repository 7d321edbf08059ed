"""The two token mixers that do their token-axis product on the matrix cores with compensated bf16 arithmetic, held to float64 element
by element: gfilter_fast_kernel<0/1> (spv_gfilter_fwd / _bwd on the fast path; the generic kernels too, with a c of their own) and
hadamard_mfma_kernel<0/1> (spv_hadamard_ln_fwd / _bwd).  Raw C-ABI calls on guarded buffers, in eager mode, on the current stream.

tests/test_gpu_gfilter_mixer.py and tests/test_gpu_hadamard_mixer.py judge the bf16 outputs of these kernels by the largest error over
the sample's largest reference value, within 2e-5 / 3e-5 / 6e-5 + 2^-8.  2^-8 of the largest of some 33 000 elements is about ten
times what a missing lo part does, so a kernel without its lo tables, its lo spectrum or its lo image passes there.  Here every
element has its own bar, c 2^-24 S_i (+ half a bf16 ulp of the reference for a bf16 store), S_i the sum of the absolute values of the
products that reach it: tests/mfma_mixer_ref.py, whose c come from the floors tests/test_mfma_mixer_ref.py measures on exactly these
inputs, and which shows there that a restatement of each kernel passes this judge and that each dropped lo part does not.

Every case asserts, in this order: memory -- sentinels intact, inputs bit-identical afterwards, every output written, nothing behind
the documented floats of a slab buffer; values -- edge_judge.verdict over every element of every output, the worst ratio to each bar
printed; repeat -- the same calls again into fresh buffers give the same bits.  Inputs are seeded normals with +0, -0 and the smallest
bf16 / fp32 subnormal planted, and for the filter one all-zero column of x and of dy in one sample, whose column of y / dx must come
back as zeros (of either sign: numpy.fft's is no reference)."""
import numpy as np
import pytest
import torch

import gfilter_ref as G
import hadamard_ref as H
import mfma_mixer_ref as M
from test_gpu_attention_edges import Guarded
from test_gpu_gfilter_mixer import _bits, _table
from test_gpu_spectral_edges import check_memory, scratch

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
F32 = torch.float32
WORST, UNITS = {}, {}


@pytest.fixture(autouse=True)
def stop_after_a_device_fault():
    """a sticky HIP error ends the session here: nothing more is started on a device that has faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error ({e}); no further case is started on it", returncode=3)


def _native():
    from spectre_vit import _native as n
    return n


def _st():
    from spectre_vit import hip_ops
    return hip_ops._stream()


def _record(family, tag, worst, units):
    """units: the error beyond the store's half ulp in units of 2^-24 S_i, the figure the floors and c are stated in"""
    print(f"MFMA-MIXER-GPU {family} {tag} worst ratio to the bar: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items())
          + "; units: " + " ".join(f"{k}={v:.2f}" for k, v in units.items()))
    for k, v in worst.items():
        WORST[(family, k)] = max(WORST.get((family, k), 0.0), v)
    for k, v in units.items():
        UNITS[(family, k)] = max(UNITS.get((family, k), 0.0), v)


def _same_bits(first, second, used):
    for name, b in first.items():
        n = used.get(name, b.t.numel()) * b.t.element_size()
        assert torch.equal(_bits(b.t)[:n], _bits(second[name].t)[:n]), f"{name}: the second call gave other bits"


# ------------------------------------------------------------------------------------------------------------------ A. the global filter
@pytest.mark.parametrize("case", M.FILTER_CASES, ids=G.case_id)
def test_gfilter_fwd_and_bwd_element_by_element(case):
    nat, c = _native(), case
    code, dtype, K = G.CODE[c.dtype], DT[c.dtype], G.bins(c.tokens)
    shape = (c.batch, c.tokens, c.dim)
    family = M.path_name(c)
    assert nat.call("spv_gfilter_path", code, c.tokens, c.dim, 1) == (G.FAST if family == "fast" else G.GENERIC)
    x64, dy64, w64 = M.filter_inputs(c)
    data = dict(x=x64, dy=dy64, filter=w64)
    tab = _table(c.tokens)
    ins = dict(x=Guarded(shape, dtype, x64), dy=Guarded(shape, dtype, dy64), filter=Guarded((K, c.dim, 2), F32, w64))
    before = {k: _bits(b.t).clone() for k, b in {**ins, "tables": tab}.items()}
    pn = nat.call("spv_gfilter_partial_floats", *shape)
    assert pn == G.partial_floats(*shape) and nat.call("spv_gfilter_workspace_floats", *shape) == 0
    runs = [dict(y=Guarded(shape, dtype), dx=Guarded(shape, dtype), dfilter=Guarded((K, c.dim, 2), F32), partials=scratch(pn)) for _ in range(2)]
    for o in runs:
        nat.call("spv_gfilter_fwd", ins["x"].ptr, ins["filter"].ptr, o["y"].ptr, tab.ptr, *shape, code, 0, _st())
        nat.call("spv_gfilter_bwd", ins["x"].ptr, ins["dy"].ptr, ins["filter"].ptr, o["dx"].ptr, o["dfilter"].ptr, tab.ptr, o["partials"].ptr,
                 *shape, code, 0, _st())
    torch.cuda.synchronize()
    # memory
    for n, o in enumerate(runs):
        check_memory(ins if n == 0 else {}, o, data, dict(partials=pn))
    assert tab.intact()
    for k, b in {**ins, "tables": tab}.items():
        assert torch.equal(_bits(b.t), before[k]), f"input {k} changed"
    # values: every element of y, dx and dW; the zeroed columns; the inert imaginary parts of the gradient and of every slab
    got = dict(y=runs[0]["y"].f64(), dx=runs[0]["dx"].f64(), dw=runs[0]["dfilter"].f64())
    ref = M.filter_reference(x64, dy64, w64)
    ok, worst = M.filter_verdict(c, ref, got)
    _record(f"{family} {c.dtype}", G.case_id(c), worst, {k: M.excess_units(ref, got[k], k, "fp32" if k == "dw" else c.dtype) for k in got})
    assert ok, (G.case_id(c), worst)
    for name, src in (("y", x64), ("dx", dy64)):
        dead = np.broadcast_to(~src.any(1)[:, None, :], shape)
        assert dead.any() and not got[name][dead].any(), f"{name}: a column of zeros did not come back as zeros"
    slabs = runs[0]["partials"].t[:pn].cpu().numpy().reshape(G.slabs(c.batch), K, c.dim, 2)
    for k in G.inert(c.tokens):
        assert not slabs[:, k, :, 1].any() and not np.signbit(slabs[:, k, :, 1]).any()
    # repeat
    _same_bits(runs[0], runs[1], dict(partials=pn))


# ------------------------------------------------------------------------------------------------------------------ B. the Hadamard pair
@pytest.mark.parametrize("mode", H.LN_MODES)
@pytest.mark.parametrize("case", M.HADAMARD_CASES, ids=H.case_id)
def test_hadamard_fused_pair_element_by_element(case, mode):
    """spv_hadamard_ln_fwd, then spv_hadamard_ln_bwd fed the forward's own prenorm, mean and rstd; "defer": no dgamma / dbeta pointers,
    the caller folds the slabs [batch][2][512]"""
    nat, c, bf = _native(), case, torch.bfloat16
    B, N, Dm = c.batch, c.tokens, 512
    shape, defer = (B, N, Dm), mode == "defer"
    assert nat.call("spv_hadamard_ln_supported", N, Dm, 1) == 1
    data = M.hadamard_inputs(c)
    ins = dict(x=Guarded(shape, bf, data["x"]), gamma=Guarded((Dm,), F32, data["gamma"]), beta=Guarded((Dm,), F32, data["beta"]),
               dout=Guarded(shape, bf, data["dout"]))
    before = {k: _bits(b.t).clone() for k, b in ins.items()}
    s = H.scale32(N, Dm)
    runs = []
    for _ in range(2):
        o = dict(prenorm=Guarded(shape, bf), out=Guarded(shape, bf), mean=Guarded((B, N), F32), rstd=Guarded((B, N), F32), dx=Guarded(shape, bf),
                 partials=scratch(B * 2 * Dm))
        if not defer:
            o.update(dgamma=Guarded((Dm,), F32), dbeta=Guarded((Dm,), F32))
        nat.call("spv_hadamard_ln_fwd", ins["x"].ptr, o["prenorm"].ptr, o["out"].ptr, ins["gamma"].ptr, ins["beta"].ptr, o["mean"].ptr,
                 o["rstd"].ptr, s, B, N, Dm, 1, _st())
        nat.call("spv_hadamard_ln_bwd", ins["dout"].ptr, o["prenorm"].ptr, o["mean"].ptr, o["rstd"].ptr, ins["gamma"].ptr, o["dx"].ptr,
                 0 if defer else o["dgamma"].ptr, 0 if defer else o["dbeta"].ptr, o["partials"].ptr, s, B, N, Dm, 1, _st())
        runs.append(o)
    torch.cuda.synchronize()
    # memory
    for n, o in enumerate(runs):
        check_memory(ins if n == 0 else {}, o, data, dict(partials=B * 2 * Dm))
    for k, b in ins.items():
        assert torch.equal(_bits(b.t), before[k]), f"input {k} changed"
    # values
    got = {k: b.f64() for k, b in runs[0].items()}
    got["partials"] = got["partials"][:B * 2 * Dm].reshape(B, 2, Dm)
    if defer:
        got["dgamma"], got["dbeta"] = got["partials"].sum(0)
    ok, worst = M.hadamard_verdict(data, got)
    ref = M.hadamard_reference(data, got)
    _record("hadamard", f"{mode} {H.case_id(c)}", worst,
            {k: M.excess_units(ref, got[k], k, "bf16" if k in ("prenorm", "dx") else "fp32") for k in M.HADAMARD_ELEMENTWISE})
    assert ok, (mode, H.case_id(c), worst)
    # repeat
    _same_bits(runs[0], runs[1], dict(partials=B * 2 * Dm))


def test_worst_ratio_to_each_bar_per_family():
    """what the cases above measured (empty when this test runs alone)"""
    for (family, k), v in sorted(WORST.items()):
        print(f"MFMA-MIXER-GPU-WORST {family} {k}: ratio to the bar {v:.3f}" + (f", {UNITS[(family, k)]:.2f} units of 2^-24 S_i" if (family, k) in UNITS else ""))
    assert all(v <= 1.0 for v in WORST.values())
