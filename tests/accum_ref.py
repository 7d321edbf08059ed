"""Host restatement of on-device gradient accumulation (FusedAdamW(accumulate_steps=k); include/spv.h: spv_grad_accumulate,
spv_step_control_accum), in numpy: the accumulators as float32 sequential sums, the fp64 sum of squares of the new accumulator in the
kernels' summation order, and the 64-byte control block after every micro-step, packed with the optimizer module's own format.

The accumulators start as NaN: the first micro-step of a window ASSIGNS, so nothing of that survives.  The sum of squares is formed
with a separate multiply and add per element; the device may contract the pair into one fused multiply-add, so its sum agrees to a
few units in the last place of a double, not bit for bit -- the tests compare the norm at 1e-5 and the integer fields exactly."""
import math
import struct

import numpy as np

CHUNK = 2048
SCHEDULE, CLIP, SKIP_NONFINITE = 1, 2, 4


def chunk_sumsq(x):
    """fp64 sum of squares of one chunk (<= 2048 float32 values) in grad_sumsq_kernel's order: thread t of 256 adds the squares of
    elements 4t .. 4t+3 and 1024+4t .. 1024+4t+3 one after the other, a butterfly (xor 32, 16, .. 1) joins each wave of 64, and the
    four wave sums are added as (w0 + w1) + (w2 + w3).  Slots past the chunk's end add +0.0, which changes no sum of squares."""
    v = np.zeros(CHUNK, dtype=np.float64)
    v[:x.size] = x.astype(np.float64)
    sq = (v * v).reshape(2, 256, 4)
    s = np.zeros(256, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(2):
            for u in range(4):
                s = s + sq[h, :, u]
        lane = np.arange(256)
        for w in (32, 16, 8, 4, 2, 1):
            s = s + s[lane ^ w]
        return float((s[0] + s[64]) + (s[128] + s[192]))


def fold_partials(partials):
    """step_control_kernel's fold: thread i adds partials i, i + 256, ... in that order, then a tree over the 256 sums"""
    red = np.zeros(256, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, p in enumerate(partials):
            red[i % 256] = red[i % 256] + p
        w = 128
        while w > 0:
            red[:w] = red[:w] + red[w:2 * w]
            w >>= 1
    return float(red[0])


def cosine_ab(t, warmup, total, eta_min):
    """the schedule's (a, b) at t: lr = float32(a * base + b) (spv_step_control)"""
    if t < warmup:
        return (t + 1) / (warmup + 1), 0.0
    span = total - warmup
    k = min(t - warmup, span)
    a = 0.0 if k >= span else 0.5 * (1.0 + math.cos(math.pi * k / span))
    return a, eta_min * (1.0 - a)


class AccumRef:
    """one optimizer's accumulators and control block.  sizes: the element count of every tensor, all groups in order."""

    def __init__(self, k, sizes, schedule=None, max_grad_norm=None, skip_nonfinite=False):
        """schedule: (total_steps, warmup_steps, eta_min) or None"""
        self.k, self.sizes = int(k), [int(n) for n in sizes]
        self.schedule, self.max_grad_norm, self.skip_nonfinite = schedule, max_grad_norm, bool(skip_nonfinite)
        self.acc = [np.full(n, np.nan, dtype=np.float32) for n in self.sizes]
        self.ctl = dict(a=1.0, b=0.0, clip_coef=np.float32(1.0), apply=1, grad_norm=np.float32(0.0), sched_step=0, skipped=0, micro=0)
        self.adam_steps = 0
        self.sumsq = 0.0

    @property
    def flags(self):
        return ((SCHEDULE if self.schedule is not None else 0) | (CLIP if self.max_grad_norm is not None else 0)
                | (SKIP_NONFINITE if self.skip_nonfinite else 0))

    def micro_step(self, grads):
        """grads: one float32 array per tensor.  -> a copy of the control-block fields after this micro-step"""
        c, k = self.ctl, self.k
        partials = []
        with np.errstate(invalid="ignore", over="ignore"):
            for i, g in enumerate(grads):
                g = np.asarray(g, dtype=np.float32).reshape(-1)
                assert g.size == self.sizes[i]
                self.acc[i] = g.copy() if c["micro"] == 0 else (self.acc[i] + g).astype(np.float32)   # assignment / one fp32 add
                partials += [chunk_sumsq(self.acc[i][off:off + CHUNK]) for off in range(0, g.size, CHUNK)]
        if c["micro"] < k - 1:   # inside the window: two fields move
            c["apply"] = 0
            c["micro"] += 1
            return dict(c)
        sumsq = self.sumsq = fold_partials(partials)
        with np.errstate(invalid="ignore", over="ignore"):
            norm = np.float32(np.sqrt(np.float64(sumsq)) / np.float64(k))   # the norm of the MEAN gradient
            t = c["sched_step"]
            a, b = cosine_ab(t, self.schedule[1], self.schedule[0], self.schedule[2]) if self.schedule is not None else (1.0, 0.0)
            coef = np.float32(1.0)
            if self.max_grad_norm is not None:
                cc = np.float32(self.max_grad_norm) / (norm + np.float32(1e-6))
                coef = cc if cc < 1.0 else (cc if cc != cc else np.float32(1.0))   # clamp(max=1) that keeps a NaN
            coef = np.float32(np.float64(coef) / np.float64(k))
        apply = 0 if (self.skip_nonfinite and not math.isfinite(sumsq)) else 1
        c.update(a=a, b=b, clip_coef=coef, apply=apply, grad_norm=norm, sched_step=t + 1, micro=0)
        if apply:
            self.adam_steps += 1
        else:
            c["skipped"] += 1
        return dict(c)

    def block_bytes(self):
        from spectre_vit import optim
        c = self.ctl
        return struct.pack(optim._CTL_FMT, c["a"], c["b"], float(c["clip_coef"]), c["apply"], float(c["grad_norm"]), c["sched_step"],
                           c["skipped"], c["micro"])

    def lr(self, base_lr):
        """float32(a * base + b), product and sum each rounded to double: the optimizer launch's expression"""
        return float(np.float32(np.float64(self.ctl["a"]) * np.float64(base_lr) + np.float64(self.ctl["b"])))
