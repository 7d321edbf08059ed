"""Weight averaging (EMA) inside FusedAdamW's launch, on the GPU: the average does not perturb training (bit for bit), its values
against the float64 restatement of tests/ema_ref.py, the dropped step, graph replay following the warm-up, resume, the in-place
exchange with the live weights, the harness, and two data-parallel ranks.

One tensor set for the optimizer tests, all averaged tensors in ONE group (sizes 1, 5, 2048, 2049, 2051, 4096, 6000: a scalar, a
sub-vector tail, an exact chunk, chunk + 1, chunk + 3, two chunks, three chunks with a short last one) plus
  * a second 2051-element tensor, the TWIN of the first: same values, same gradients; the first one's average is a view 4 bytes off a
    16-byte boundary while its p, g, m, v are aligned (the average alone is walked element by element),
  * the 4096-element tensor excluded from averaging (a NULL entry of the launch's ema_table),
  * a second group with ema_decay=None.

Bound (ema_ref.bound): |e - e64| <= 4 k 2^-24 max(|p|, |e|) per tensor after k steps.
Measured on an MI355X: worst |e - e64| / bound 0.149 after 6 eager steps, 0.227 over a warm-up step + 5 replays."""
import copy
import json
import math
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ema_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu

SIZES = [1, 5, 2048, 2049, 2051, 4096, 6000, 2051]
I_MIS, I_TWIN, I_NULL = 4, 7, 5
OTHER = 300            # the one tensor of the group that is not averaged
DEV = "cuda:0"


def offset_view(values):
    """a contiguous tensor holding `values` whose data pointer is 4 bytes past a 16-byte boundary"""
    buf = torch.empty(values.numel() + 1, device=values.device, dtype=values.dtype)
    v = buf[1:].view(values.shape)
    v.copy_(values)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def make_params(seed):
    g = torch.Generator().manual_seed(seed)
    vals = [torch.randn(n, generator=g) for n in SIZES[:-1]]
    vals.append(vals[I_MIS].clone())
    ps = [v.to(DEV).requires_grad_(True) for v in vals]
    other = torch.randn(OTHER, generator=g).to(DEV).requires_grad_(True)
    assert all(p.data_ptr() % 16 == 0 for p in ps)
    return ps, other


def clone_params(ps, other):
    return [p.detach().clone().requires_grad_(True) for p in ps], other.detach().clone().requires_grad_(True)


def make_grads(gen, scale=1.0):
    gs = [torch.randn(n, generator=gen) * scale for n in SIZES[:-1]]
    gs.append(gs[I_MIS].clone())
    return [g.to(DEV) for g in gs], (torch.randn(OTHER, generator=gen) * scale).to(DEV)


def set_grads(ps, other, grads):
    for p, g in zip(ps + [other], grads[0] + [grads[1]]):
        p.grad = g.clone()


def make_opt(ps, other, ema_decay=0.9, misalign=True, **kw):
    """the averaging optimizer of the tests: group 0 averaged (the 4096 tensor excluded), group 1 not"""
    from spectre_vit.optim import FusedAdamW
    kw.setdefault("lr", 1e-2)
    kw.setdefault("weight_decay", 0.01)
    groups = [dict(params=ps), dict(params=[other], ema_decay=None)]
    o = FusedAdamW(groups, ema_decay=ema_decay, ema_exclude=[ps[I_NULL]], **kw)
    if misalign:   # before the first step: the state entry is taken as it is found
        o.state[ps[I_MIS]]["ema"] = offset_view(ps[I_MIS].detach())
    return o


def averaged(ps):
    return [(i, p) for i, p in enumerate(ps) if i != I_NULL]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


PATHS = {"plain": dict(capturable=False), "capturable": dict(capturable=True),
         "control": dict(capturable=True, skip_nonfinite=True, max_grad_norm=1.0)}


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the average does not perturb training
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("warmup", [False, True])
def test_average_does_not_perturb_training(path, warmup):
    from spectre_vit.optim import FusedAdamW
    a, oa_ = make_params(0)
    b, ob_ = clone_params(a, oa_)
    oa = make_opt(a, oa_, ema_decay=0.999, ema_warmup=warmup, **PATHS[path])
    ob = FusedAdamW([dict(params=b), dict(params=[ob_])], lr=1e-2, weight_decay=0.01, **PATHS[path])
    gen = torch.Generator().manual_seed(1)
    for step in range(4):
        grads = make_grads(gen, 0.1 + step)
        set_grads(a, oa_, grads)
        set_grads(b, ob_, grads)
        oa.step()
        ob.step()
    for i, (x, y) in enumerate(zip(a + [oa_], b + [ob_])):
        assert same_bits(x, y), (i, (x - y).abs().max().item())
        for k in ("exp_avg", "exp_avg_sq"):
            assert same_bits(oa.state[x][k], ob.state[y][k]), (i, k)
        assert float(oa.state[x]["step"]) == float(ob.state[y]["step"]) == 4.0
        assert "ema" not in ob.state[y]
        assert ("ema" in oa.state[x]) == (i not in (I_NULL, len(a))), i
    assert oa.state[a[I_MIS]]["ema"].data_ptr() % 16 == 4, "the misaligned view is the buffer the kernel wrote"
    assert len(oa.ema_parameters()) == len(SIZES) - 1
    sd_keys = [set(v) for v in oa.state_dict()["state"].values()]
    assert sd_keys.count({"exp_avg", "exp_avg_sq", "step", "ema"}) == len(SIZES) - 1 and sd_keys.count({"exp_avg", "exp_avg_sq", "step"}) == 2


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. values
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("decay", [0.9, 0.999])
def test_values_against_the_float64_restatement(decay, warmup, capturable):
    from spectre_vit.optim import ema_weight_at
    K = 6
    ps, other = make_params(2)
    o = make_opt(ps, other, ema_decay=decay, ema_warmup=warmup, capturable=capturable)
    es = o.ema_parameters()   # creates the averages: before the first step they are p_0 bit for bit
    assert len(es) == len(SIZES) - 1 and es[I_MIS].data_ptr() % 16 == 4
    for (i, p), e in zip(averaged(ps), es):
        assert same_bits(e, p) and e.data_ptr() != p.data_ptr(), i
    ref = {i: R.Average(p.detach().cpu().numpy()) for i, p in averaged(ps)}
    gen = torch.Generator().manual_seed(3)
    worst = 0.0
    for k in range(1, K + 1):
        set_grads(ps, other, make_grads(gen, 0.1 * k))
        o.step()
        w = R.weight(k, decay, warmup)
        assert float(w) == ema_weight_at(k, decay, warmup)
        for (i, p), e in zip(averaged(ps), o.ema_parameters()):
            pn = p.detach().cpu().numpy()
            r = R.ratio(e.cpu().numpy(), ref[i].update(pn, w), k, pn)
            worst = max(worst, r)
            assert r <= 1.0, (i, k, r)
        assert same_bits(o.state[ps[I_MIS]]["ema"], o.state[ps[I_TWIN]]["ema"]), ("the misaligned average and its aligned twin", k)
        assert same_bits(ps[I_MIS], ps[I_TWIN])
    assert [e.data_ptr() for e in o.ema_parameters()] == [e.data_ptr() for e in es], "the averages never move"
    assert not same_bits(o.state[ps[0]]["ema"], ps[0])
    print(f"decay {decay} warmup {warmup} capturable {capturable}: worst |e - e64| / bound over {K} steps = {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. a dropped step
# ---------------------------------------------------------------------------------------------------------------------------------
def test_dropped_step_leaves_the_average_and_the_next_step_uses_the_unadvanced_count():
    decay = 0.999
    ps, other = make_params(4)
    o = make_opt(ps, other, ema_decay=decay, ema_warmup=True, capturable=True, skip_nonfinite=True)
    gen = torch.Generator().manual_seed(5)
    for k in range(2):
        set_grads(ps, other, make_grads(gen))
        o.step()
    before_e = [e.clone() for e in o.ema_parameters()]
    before_p = [p.detach().clone() for p in ps]
    grads = make_grads(gen)
    grads[0][2][2047] = float("inf")
    set_grads(ps, other, grads)
    o.step()
    assert o.skipped_steps() == 1 and float(o.state[ps[0]]["step"]) == 2.0
    for i, (e, e0) in enumerate(zip(o.ema_parameters(), before_e)):
        assert same_bits(e, e0), i
    assert all(same_bits(p, q) for p, q in zip(ps, before_p))
    set_grads(ps, other, make_grads(gen))
    o.step()
    assert o.skipped_steps() == 1 and float(o.state[ps[0]]["step"]) == 3.0
    w3, w4 = R.weight(3, decay, True), R.weight(4, decay, True)
    for (i, p), e, e0 in zip(averaged(ps), o.ema_parameters(), before_e):
        pn = p.detach().cpu().numpy()
        want = R.Average(e0.cpu().numpy()).update(pn, w3)
        assert R.ratio(e.cpu().numpy(), want, 1, pn) <= 1.0, i
        if p.numel() >= 2048:   # the count of a step that had been advanced by the dropped one would show
            assert R.ratio(e.cpu().numpy(), R.Average(e0.cpu().numpy()).update(pn, w4), 1, pn) > 1.0, i


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. graph replay follows the warm-up
# ---------------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_follows_the_warmup():
    from spectre_vit.graph import GraphedDPStep, GraphedTrainStep
    from spectre_vit.models.spectre.spectre import SpectreViT
    from spectre_vit.optim import FusedAdamW
    cfg = dict(img_size=32, patch_size=4, in_channels=3, num_classes=100, embed_dim=512, num_encoders=1, num_heads=16, hidden_dim=768,
               activation="gelu", dropout=0.0, mixer="fft")
    decay = 0.999
    g = torch.Generator().manual_seed(3)
    img = torch.randn(16, 3, 32, 32, generator=g).to(DEV)
    labels = torch.randint(0, 100, (16,), generator=g).to(DEV)
    crit = torch.nn.CrossEntropyLoss()
    for cls in (GraphedTrainStep, GraphedDPStep):
        torch.manual_seed(11)
        m = SpectreViT(**cfg).to(DEV).train()
        params = list(m.parameters())
        o = FusedAdamW(params, lr=1e-3, weight_decay=0.01, capturable=True, static_grads=True, ema_decay=decay, ema_warmup=True)
        ref = [R.Average(p.detach().cpu().numpy()) for p in params]
        frozen = [R.Average(p.detach().cpu().numpy()) for p in params]   # what a kernel whose w_t froze at capture would compute
        step = cls(m, o, crit, img, labels, warmup=1)   # the warm-up step is Adam step 1
        try:
            worst = worst_frozen = 0.0
            for s in range(1, 7):
                if s > 1:
                    step(img, labels)
                assert float(o.state[params[0]]["step"]) == float(s)
                es = o.ema_parameters()
                for p, e, r, f in zip(params, es, ref, frozen):
                    pn, en = p.detach().cpu().numpy(), e.cpu().numpy()
                    worst = max(worst, R.ratio(en, r.update(pn, R.weight(s, decay, True)), s, pn))
                    # the first replay is step 2: the count a capture would have frozen
                    fr = R.ratio(en, f.update(pn, R.weight(min(s, 2), decay, True)), s, pn)
                    if s == 6:
                        worst_frozen = max(worst_frozen, fr)
                assert worst <= 1.0, (cls.__name__, s, worst)
            print(f"{cls.__name__}: worst |e - e64| / bound over warm-up + 5 replays {worst:.3f}; with w_t frozen at the first replay's "
                  f"count {worst_frozen:.1f}")
            assert worst_frozen > 1.0, "the restatement with a constant weight must miss the bound, or this test shows nothing"
            if cls is GraphedDPStep:   # graph B (the optimizer) holds the averaging launch, graph A none
                before = [e.clone() for e in o.ema_parameters()]
                step.graph.replay()
                assert all(same_bits(x, y) for x, y in zip(o.ema_parameters(), before))
                step.graph_opt.replay()
                assert any(not same_bits(x, y) for x, y in zip(o.ema_parameters(), before))
        finally:
            step.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. resume
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["plain", "control"])
def test_resume_continues_the_average_bit_for_bit(path):
    kw = dict(ema_decay=0.999, ema_warmup=True, **PATHS[path])
    a, a_other = make_params(6)
    b, b_other = clone_params(a, a_other)
    oa, ob = make_opt(a, a_other, misalign=False, **kw), make_opt(b, b_other, misalign=False, **kw)
    gen = torch.Generator().manual_seed(7)
    all_grads = [make_grads(gen) for _ in range(6)]
    for grads in all_grads:
        set_grads(a, a_other, grads)
        oa.step()
    for grads in all_grads[:3]:
        set_grads(b, b_other, grads)
        ob.step()
    sd = copy.deepcopy(ob.state_dict())
    c, c_other = clone_params(b, b_other)
    oc = make_opt(c, c_other, misalign=False, **kw)
    oc.load_state_dict(copy.deepcopy(sd))
    for grads in all_grads[3:]:
        set_grads(c, c_other, grads)
        oc.step()
    for i, (x, y) in enumerate(zip(a, c)):
        assert same_bits(x, y), i
        if i != I_NULL:
            assert same_bits(oa.state[x]["ema"], oc.state[y]["ema"]), i
    assert "ema" not in oc.state[c[I_NULL]] and "ema" not in oc.state[c_other]

    # the same state without its averages (what a torch.optim.AdamW checkpoint looks like): the average starts from the current p
    for st in sd["state"].values():
        st.pop("ema", None)
    d, d_other = clone_params(b, b_other)
    od = make_opt(d, d_other, misalign=False, **kw)
    od.load_state_dict(sd)
    assert od.ema_enabled and all("ema" not in od.state[p] for p in d)
    p3 = [p.detach().cpu().numpy().copy() for p in d]
    set_grads(d, d_other, all_grads[3])
    od.step()
    w4 = R.weight(4, 0.999, True)   # the loaded Adam step count goes on
    for i, p in averaged(d):
        pn = p.detach().cpu().numpy()
        want = R.Average(p3[i]).update(pn, w4)
        assert R.ratio(od.state[p]["ema"].cpu().numpy(), want, 1, pn) <= 1.0, i


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the exchange with the live weights
# ---------------------------------------------------------------------------------------------------------------------------------
MODEL = dict(img_size=16, patch_size=4, in_channels=3, num_classes=100, embed_dim=64, num_encoders=2, num_heads=4, hidden_dim=96,
             dropout=0.0, activation="gelu")


def trained_model(mixer="permut", steps=3, **okw):
    from spectre_vit.models.spectre.spectre import SpectreViT
    from spectre_vit.optim import FusedAdamW
    torch.manual_seed(21)
    m = SpectreViT(**MODEL, mixer=mixer).to(DEV).train()
    o = FusedAdamW(m.parameters(), lr=1e-2, capturable=True, ema_decay=0.9, **okw)
    g = torch.Generator().manual_seed(22)
    img = torch.randn(8, 3, 16, 16, generator=g).to(DEV)
    labels = torch.randint(0, 100, (8,), generator=g).to(DEV)
    for _ in range(steps):
        o.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(m(img), labels).backward()
        o.step()
    return m, o, img, labels


def eval_logits(m, img):
    m.eval()
    with torch.no_grad():
        return m(img).clone()


def test_ema_weights_exchanges_in_place_and_restores():
    from spectre_vit.models.spectre.spectre import SpectreViT
    m, o, img, labels = trained_model()
    params = list(m.parameters())
    live = [p.detach().clone() for p in params]
    ema = [e.clone() for e in o.ema_parameters()]
    mom = [(o.state[p]["exp_avg"].clone(), o.state[p]["exp_avg_sq"].clone()) for p in params]
    ptrs = [p.data_ptr() for p in params]
    assert any(not same_bits(p, e) for p, e in zip(live, ema))
    live_logits = eval_logits(m, img)
    buffers = {k: v.clone() for k, v in m.named_buffers()}

    def check_restored():
        assert [p.data_ptr() for p in params] == ptrs
        for p, p0, e, e0, (m0, v0) in zip(params, live, o.ema_parameters(), ema, mom):
            assert same_bits(p, p0) and same_bits(e, e0)
            assert same_bits(o.state[p]["exp_avg"], m0) and same_bits(o.state[p]["exp_avg_sq"], v0)

    sd = o.ema_state_dict(m)
    with o.ema_weights():
        assert [p.data_ptr() for p in params] == ptrs
        for p, e0, e, p0 in zip(params, ema, o.ema_parameters(), live):
            assert same_bits(p, e0) and same_bits(e, p0)
        inside = eval_logits(m, img)
        with pytest.raises(RuntimeError, match="ema_weights"):
            o.step()
        with pytest.raises(RuntimeError, match="nest"):
            with o.ema_weights():
                pass
    check_restored()
    assert torch.equal(eval_logits(m, img), live_logits), "the cached compute-dtype copies were invalidated on exit"
    assert not torch.equal(inside, live_logits)

    torch.manual_seed(99)
    fresh = SpectreViT(**MODEL, mixer="permut").to(DEV)
    fresh.load_state_dict(sd, strict=True)
    assert torch.equal(eval_logits(fresh, img), inside)
    names = dict(m.named_parameters())
    for k, v in sd.items():
        if k in names:
            assert same_bits(v, o.state[names[k]]["ema"]) and v.data_ptr() != o.state[names[k]]["ema"].data_ptr(), k
        else:
            assert same_bits(v, buffers[k]), k
    assert set(sd) == set(m.state_dict())

    with pytest.raises(KeyError, match="boom"):
        with o.ema_weights():
            raise KeyError("boom")
    check_restored()
    m.train()   # and training goes on
    o.zero_grad(set_to_none=True)
    torch.nn.functional.cross_entropy(m(img), labels).backward()
    o.step()
    assert any(not same_bits(p, p0) for p, p0 in zip(params, live))


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the harness
# ---------------------------------------------------------------------------------------------------------------------------------
CFG = "spectre_vit/configs/spectre_vit_mnist.py"
NEW_KEYS = {"Accuracy/ValidationEMA", "Loss/ValidationEMA"}


@pytest.mark.parametrize("mode", ["eager", "graph", "graph+graph_eval"])
def test_harness_validates_and_saves_the_average(tmp_path, mode):
    from spectre_vit.configs.parser import parse_config
    from spectre_vit.harness import build_model, train
    kw = dict(mixer="fft", epochs=2, steps_per_epoch=3, batch_size=16, n_train=64, n_val=32, log=lambda r: None,
              graph=mode != "eager", graph_eval=mode == "graph+graph_eval")
    _, h = train(CFG, out_dir=str(tmp_path / "ema"), ema_decay=0.9, **kw)
    # the same run without the average; eager: the same optimizer class, selected through skip_nonfinite
    _, h0 = train(CFG, out_dir=str(tmp_path / "ref"), **kw, **(dict(skip_nonfinite=True) if mode == "eager" else {}))
    assert len(h) == len(h0) == 2
    for rec, rec0 in zip(h, h0):
        print(mode, rec)
        assert NEW_KEYS <= set(rec) and not NEW_KEYS & set(rec0)
        assert all(math.isfinite(rec[k]) for k in NEW_KEYS)
        old = set(rec) - NEW_KEYS
        assert old == {"epoch", "Loss/Train", "Loss/Validation", "Accuracy/Train", "Accuracy/Validation", "steps", "val_samples"}
        for k in old:
            assert json.dumps(rec[k]) == json.dumps(rec0[k]), (mode, k, rec[k], rec0[k])
    lines = [json.loads(l) for l in open(tmp_path / "ema" / "scalars.jsonl")]
    assert [NEW_KEYS <= set(l) for l in lines] == [True, True, False]
    best = torch.load(tmp_path / "ema" / "model_best.pt", weights_only=True)
    ema = torch.load(tmp_path / "ema" / "model_ema_best.pt", weights_only=True)
    assert not os.path.exists(tmp_path / "ref" / "model_ema_best.pt")
    fresh = build_model(parse_config(CFG), "fft", DEV)
    fresh.load_state_dict(ema, strict=True)
    pnames = {k for k, _ in fresh.named_parameters()}
    assert set(ema) == set(best)
    assert any(not same_bits(ema[k], best[k]) for k in pnames)
    assert all(same_bits(ema[k], best[k]) for k in set(ema) - pnames)


def test_distill_harness_records_the_average(tmp_path):
    from spectre_vit.harness import train_distill
    _, h = train_distill(CFG, mixer="fft", out_dir=str(tmp_path), log=lambda r: None, epochs=1, steps_per_epoch=3, batch_size=16, n_train=64,
                         n_val=32, augment=False, ema_decay=0.9, cache_teacher=True, graph=True)
    assert len(h) == 1 and NEW_KEYS <= set(h[0]) and all(math.isfinite(h[0][k]) for k in NEW_KEYS)
    assert os.path.exists(tmp_path / "model_ema_best.pt")


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. data parallel
# ---------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, outdir):
    sys.path.insert(0, PKG)
    from spectre_vit.dp import GradReducer, broadcast_module
    from spectre_vit.models.spectre.spectre import SpectreViT
    from spectre_vit.optim import FusedAdamW
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(100 + rank)   # different init per rank: broadcast_module reconciles, and the average starts from the result
    m = SpectreViT(**MODEL, mixer="fft").to(DEV).train()
    broadcast_module(m)
    red = GradReducer(m, bucket_mb=0.05)
    o = FusedAdamW(m.parameters(), lr=1e-2, capturable=True, ema_decay=0.9, ema_warmup=True)
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(8, 3, 16, 16, generator=g), torch.randint(0, 100, (8,), generator=g)
    xs, ys = x[rank * 4:(rank + 1) * 4].to(DEV), y[rank * 4:(rank + 1) * 4].to(DEV)
    for _ in range(3):
        red.zero_grad()
        torch.nn.functional.cross_entropy(m(xs), ys).backward()
        red.finish()
        o.step()
    torch.save(dict(ema=[e.cpu() for e in o.ema_parameters()], p=[p.detach().cpu() for p in m.parameters()]),
               os.path.join(outdir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_hold_the_same_average(tmp_path):
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt") for r in range(2))
    assert len(r0["ema"]) == len(r0["p"]) > 0
    for i, (a, b) in enumerate(zip(r0["ema"], r1["ema"])):
        assert same_bits(a, b), i
    for i, (a, b) in enumerate(zip(r0["p"], r1["p"])):
        assert same_bits(a, b), i
    assert any(not same_bits(e, p) for e, p in zip(r0["ema"], r0["p"]))
