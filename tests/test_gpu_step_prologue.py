"""spv_step_prologue: one launch whose workgroup ranges are dealt to the roles seed word / weight shadows / spectral fold / patch rows /
position rows.  Every role against its separate launch, bit for bit, for the subsets seed only, shadows only and all roles; and a tiny
SpectreViT whose graph-replayed step is bit-equal with the prologue on and off, with one prologue call per step in the C-ABI call log."""
import collections
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

SEED_STEP = 0x9e3779b97f4a7c15
SEPARATE = ("spv_seed_advance", "spv_weight_shadows_multi", "spv_spectral_fold_bf16", "spv_spectral_fold", "spv_patchify", "spv_embed_posbias")


def _st():
    return torch.cuda.current_stream().cuda_stream


class _Problem:
    """the inputs of every role and two sets of outputs: one for the separate launches, one for the prologue"""

    def __init__(self):
        from spectre_vit import shadows
        g = torch.Generator().manual_seed(17)
        r = lambda *s: torch.randn(*s, generator=g).cuda()
        self.ws = [r(40, 24), r(8, 72)]   # partial 32 x 64 tiles both ways; ld = 40 and 8 (the rows padded to 8)
        self.E, self.C, self.P, self.B, self.H = 16, 3, 4, 3, 8
        self.Np = (self.H // self.P) ** 2
        self.K = self.C * self.P * self.P
        self.proj_w, self.fh, self.fw = r(self.E, self.C * self.P * (self.P // 2 + 1)), r(self.P), r(self.P // 2 + 1)
        self.img = r(self.B, self.C, self.H, self.H)
        self.pos, self.bias, self.cls = r(1, self.Np + 1, self.E), r(self.E), r(1, 1, self.E)
        self.out = [self._outputs(shadows), self._outputs(shadows)]

    def _outputs(self, shadows):
        bf = torch.bfloat16
        sh = [(torch.full((n, k), -3.0, dtype=bf, device="cuda"), torch.full((k, (n + 7) // 8 * 8), -3.0, dtype=bf, device="cuda"))
              for n, k in (tuple(w.shape) for w in self.ws)]
        return dict(seed=torch.tensor([123456789012345], dtype=torch.int64, device="cuda"), sh=sh,
                    tables=shadows._multi_table([(w, wc, wt) for w, (wc, wt) in zip(self.ws, sh)]),
                    wf=torch.full((self.E, self.K), -3.0, device="cuda"), wb=torch.full((self.E, self.K), -3.0, dtype=bf, device="cuda"),
                    patches=torch.full((self.B * (self.Np + 1), self.K), -3.0, dtype=bf, device="cuda"),
                    posbias=torch.full((self.Np + 1, self.E), -3.0, device="cuda"))

    def separate(self, roles):
        from spectre_vit import _native
        o = self.out[0]
        P = lambda t: t.data_ptr()
        if "seed" in roles:
            _native.call("spv_seed_advance", P(o["seed"]), _st())
        if "shadows" in roles:
            table, tt, tx, ty, ntiles = o["tables"]
            assert ntiles == 2 + 2
            _native.call("spv_weight_shadows_multi", P(table), P(tt), P(tx), P(ty), ntiles, 1, _st())
        if "fold" in roles:
            _native.call("spv_spectral_fold_bf16", P(self.proj_w), P(self.fh), P(self.fw), P(o["wf"]), P(o["wb"]), self.E, self.C, self.P, _st())
        if "patchify" in roles:
            _native.call("spv_patchify", P(self.img), P(o["patches"]), self.B, self.C, self.H, self.H, self.P, self.K, 2, 1, _st())
        if "posbias" in roles:
            _native.call("spv_embed_posbias", P(self.pos), P(self.bias), P(self.cls), P(o["posbias"]), self.Np, self.E, _st())

    def prologue(self, roles):
        from spectre_vit import _native
        o = self.out[1]
        P = lambda t: t.data_ptr()
        j = _native.PrologueJobs()
        if "seed" in roles:
            j.seed_word = P(o["seed"])
        if "shadows" in roles:
            table, tt, tx, ty, ntiles = o["tables"]
            j.shadow_table, j.tile_tensor, j.tile_x, j.tile_y, j.ntiles, j.shadow_dtype = P(table), P(tt), P(tx), P(ty), ntiles, 1
        if "fold" in roles:
            j.fold_w, j.fold_fh, j.fold_fw, j.fold_out, j.fold_out_bf16 = P(self.proj_w), P(self.fh), P(self.fw), P(o["wf"]), P(o["wb"])
            j.fold_embed, j.fold_chans, j.fold_patch = self.E, self.C, self.P
        if "patchify" in roles:
            j.patch_img, j.patch_out = P(self.img), P(o["patches"])
            j.patch_batch, j.patch_chans, j.patch_height, j.patch_width = self.B, self.C, self.H, self.H
            j.patch_size, j.patch_ld, j.patch_dtype = self.P, self.K, 1
        if "posbias" in roles:
            j.pos_pos, j.pos_bias, j.pos_cls, j.pos_out = P(self.pos), P(self.bias), P(self.cls), P(o["posbias"])
            j.pos_patches, j.pos_embed = self.Np, self.E
        _native.call("spv_step_prologue", ctypes.addressof(j), _st())

    def compare(self, roles):
        torch.cuda.synchronize()
        a, b = self.out
        if "seed" in roles:
            assert int(a["seed"]) == 123456789012345 + SEED_STEP - (1 << 64), "the separate launch's own constant"
        assert int(a["seed"]) == int(b["seed"])
        for (wa, ta), (wb_, tb), w in zip(a["sh"], b["sh"], self.ws):
            assert torch.equal(wa, wb_) and torch.equal(ta, tb), tuple(w.shape)
            if "shadows" in roles:   # and they are the casts (columns past the rows of W^T: zero padding)
                n = w.shape[0]
                assert torch.equal(wa, w.to(torch.bfloat16)) and torch.equal(ta[:, :n], w.t().to(torch.bfloat16))
                assert float(ta[:, n:].abs().sum()) == 0.0
            else:
                assert float(wa.float().min()) == -3.0 == float(ta.float().max())
        for key in ("wf", "wb", "patches", "posbias"):
            assert torch.equal(a[key], b[key]), key
            role = dict(wf="fold", wb="fold", patches="patchify", posbias="posbias")[key]
            touched = not bool((a[key].float() == -3.0).all())
            assert touched == (role in roles), (key, roles)


ALL = ("seed", "shadows", "fold", "patchify", "posbias")


@pytest.mark.parametrize("roles", [("seed",), ("shadows",), ALL, ("fold",), ("patchify",), ("posbias",), ("shadows", "posbias")],
                         ids=lambda r: "+".join(r))
def test_roles_against_their_separate_launches(roles):
    p = _Problem()
    p.separate(roles)
    p.prologue(roles)
    p.compare(roles)


def test_an_empty_prologue_launches_nothing_and_bad_jobs_are_refused():
    from spectre_vit import _native
    empty = _native.PrologueJobs()   # (named: the address of a temporary would outlive the struct it points into)
    _native.call("spv_step_prologue", ctypes.addressof(empty), _st())
    torch.cuda.synchronize()
    p = _Problem()
    j = _native.PrologueJobs()
    j.patch_img, j.patch_out = p.img.data_ptr(), p.out[1]["patches"].data_ptr()
    j.patch_batch, j.patch_chans, j.patch_height, j.patch_width, j.patch_size, j.patch_ld, j.patch_dtype = 3, 3, 8, 8, 4, 40, 1   # ld < K
    with pytest.raises(RuntimeError, match="ld=40 too small"):
        _native.call("spv_step_prologue", ctypes.addressof(j), _st())
    with pytest.raises(RuntimeError, match="null jobs"):
        _native.call("spv_step_prologue", 0, _st())


def test_whole_step_is_bit_equal_and_issues_one_prologue_call():
    from spectre_vit import _native, hip_ops, prologue
    from spectre_vit.graph import GraphedTrainStep
    from spectre_vit.models.spectre.spectre import SpectreViT
    from spectre_vit.optim import FusedAdamW
    cfg = dict(img_size=8, patch_size=4, in_channels=3, num_classes=10, embed_dim=64, num_encoders=2, num_heads=4, hidden_dim=96,
               dropout=0.1, activation="gelu", mixer="fft")
    g = torch.Generator().manual_seed(9)
    img = torch.randn(4, 3, 8, 8, generator=g).cuda()
    labels = torch.randint(0, 10, (4,), generator=g).cuda()
    orig = _native.call

    def run(on):
        keep = hip_ops.STEP_PROLOGUE
        hip_ops.STEP_PROLOGUE = on
        log = collections.Counter()

        def spy(name, *a):
            log[name] += 1
            return orig(name, *a)
        _native.call = spy
        try:
            torch.manual_seed(33)
            m = SpectreViT(**cfg).cuda().train()
            opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.01, capturable=True)
            step = GraphedTrainStep(m, opt, torch.nn.CrossEntropyLoss(), img, labels, autocast_dtype=torch.bfloat16, warmup=2)
            try:
                losses = [step(img, labels).detach().clone() for _ in range(3)]
                torch.cuda.synchronize()
                assert prologue.pending() == []   # every prepared result found its consumer
                return losses, step.out.detach().clone(), {k: p.detach().clone() for k, p in m.named_parameters()}, log
            finally:
                step.close()
        finally:
            _native.call = orig
            hip_ops.STEP_PROLOGUE = keep

    la, oa, pa, log_on = run(True)
    lb, ob, pb, log_off = run(False)
    steps = 3   # two warm-up steps and the capture issue launches; the replays go through no C-ABI call
    assert log_on["spv_step_prologue"] == steps and all(log_on[n] == 0 for n in SEPARATE), log_on
    assert log_off["spv_step_prologue"] == 0 and log_off["spv_seed_advance"] == steps and log_off["spv_weight_shadows_multi"] == steps, log_off
    assert log_off["spv_spectral_fold_bf16"] == log_off["spv_patchify"] == log_off["spv_embed_posbias"] == steps, log_off
    for x, y in zip(la, lb):
        assert torch.equal(x, y), (la, lb)
    assert len({float(x) for x in la}) == 3   # three different steps (dropout masks move with the seed word)
    assert torch.equal(oa, ob)
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
