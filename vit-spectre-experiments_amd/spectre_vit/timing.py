"""Live kernel timing for bench.py's roofline block: HIP events recorded on the launch stream around EVERY C-ABI entry point that
launches (hooked in _native.call; torch.cuda.Event records on torch's current stream == the stream we launch on), and the
algorithmic work model of each entry point."""
from __future__ import annotations

import torch

from . import _native
from ._launch import BF16, F32

PEAK_TFLOPS = {BF16: 2500.0, F32: 157.3}  # dense MFMA peaks
PEAK_HBM_GBS = 8000.0


def _es(dt):
    return 2 if dt == BF16 else 4


# entry point -> f(ints) -> (label, shape, dtype code, bound, algorithmic work per call: flops (mfma) or compulsory bytes (hbm)).
# ints are the integer arguments of the C-ABI call in header order (include/spv.h).
_WORK_MODELS = {
    "spv_small_sl_fwd": lambda i: ("head_fwd", i[2:5], i[5], "mfma", 2.0 * i[2] * i[3] * i[4]),
    "spv_small_sl_bwd": lambda i: ("head_bwd", i[0:3], i[3], "mfma", 4.0 * i[0] * i[1] * i[2]),
    # the two halves of head_bwd on their own: dx = dh W (rows); dW = dh^T x (weights)
    "spv_small_sl_bwd_rows": lambda i: ("head_bwd_rows", i[0:3], i[3], "mfma", 2.0 * i[0] * i[1] * i[2]),
    "spv_small_sl_bwd_w": lambda i: ("head_bwd_w", i[0:3], F32, "mfma", 2.0 * i[0] * i[1] * i[2]),
    "spv_cross_entropy_fwd": lambda i: ("cross_entropy_fwd", i[0:2], F32, "hbm", i[0] * i[1] * 4.0),
    "spv_cross_entropy_bwd": lambda i: ("cross_entropy_bwd", i[0:2], F32, "hbm", i[0] * i[1] * 8.0),
    # student + teacher logits read (forward), read + the gradient written (backward)
    "spv_distill_loss_fwd": lambda i: ("distill_loss_fwd", i[0:2], F32, "hbm", i[0] * i[1] * 8.0),
    "spv_distill_loss_bwd": lambda i: ("distill_loss_bwd", i[0:2], F32, "hbm", i[0] * i[1] * 12.0),
    # (rows, n_cache, classes): the same traffic with the teacher's rows gathered from the cache, + the index; the store copies rows once
    "spv_distill_loss_idx_fwd": lambda i: ("distill_loss_idx_fwd", (i[0], i[2]), F32, "hbm", i[0] * (i[2] * 8.0 + 8.0)),
    "spv_distill_loss_idx_bwd": lambda i: ("distill_loss_idx_bwd", (i[0], i[2]), F32, "hbm", i[0] * (i[2] * 12.0 + 8.0)),
    # the metered forwards (rows, classes[, n_cache], k): the un-metered traffic; the meter's row and header are a few words
    "spv_cross_entropy_meter_fwd": lambda i: ("cross_entropy_meter_fwd", i[0:2], F32, "hbm", i[0] * i[1] * 4.0),
    "spv_distill_loss_meter_fwd": lambda i: ("distill_loss_meter_fwd", i[0:2], F32, "hbm", i[0] * i[1] * 8.0),
    "spv_distill_loss_idx_meter_fwd": lambda i: ("distill_loss_idx_meter_fwd", (i[0], i[2]), F32, "hbm", i[0] * (i[2] * 8.0 + 8.0)),
    # (rows, width, s_dtype, t_dtype) / (rows, n_cache, width, s_dtype): both feature matrices read once (forward), read again and the
    # student's gradient written (backward); the cache is fp32, the three per-row stats and the index are a few words a row
    "spv_feature_cosine_fwd": lambda i: ("feature_cosine_fwd", i[0:2], F32, "hbm", 1.0 * i[0] * i[1] * (_es(i[2]) + _es(i[3]))),
    "spv_feature_cosine_bwd": lambda i: ("feature_cosine_bwd", i[0:2], F32, "hbm", 1.0 * i[0] * i[1] * (2 * _es(i[2]) + _es(i[3]))),
    "spv_feature_cosine_idx_fwd": lambda i: ("feature_cosine_idx_fwd", (i[0], i[2]), F32, "hbm", 1.0 * i[0] * i[2] * (_es(i[3]) + 4)),
    "spv_feature_cosine_idx_bwd": lambda i: ("feature_cosine_idx_bwd", (i[0], i[2]), F32, "hbm", 1.0 * i[0] * i[2] * (2 * _es(i[3]) + 4)),
    "spv_logit_cache_store": lambda i: ("logit_cache_store", (i[0], i[2]), F32, "hbm", i[0] * (i[2] * 8.0 + 8.0)),
    # (batch, n_src, chans, n, resize, crop, dtype): the uint8 images read, the cropped view written once
    "spv_teacher_view_u8": lambda i: ("teacher_view", (i[0], i[2], i[3], i[5]), i[6], "hbm",
                                      1.0 * i[0] * i[2] * (i[3] * i[3] + i[5] * i[5] * _es(i[6]))),
    "spv_gemm_nt": lambda i: ("gemm_acc" if i[8] else "gemm", i[0:3], i[6], "mfma", 2.0 * i[0] * i[1] * i[2]),
    "spv_gemm_nt_grouped_rows": lambda i: ("gemm_grouped_rows", i[0:3], i[6], "mfma", 2.0 * i[0] * i[1] * i[2]),
    "spv_gemm_nt_grouped_rows_drop": lambda i: ("gemm_grouped_rows", i[0:3], i[6], "mfma", 2.0 * i[0] * i[1] * i[2]),
    # (rows, n, k, tokens per image): the same contraction on the thin-K kernel, under the same key
    "spv_token_embed_fwd": lambda i: ("gemm_grouped_rows", i[0:3], BF16, "mfma", 2.0 * i[0] * i[1] * i[2]),
    "spv_gemm_nt_pool_bwd": lambda i: ("gemm_pool_bwd", i[1:4], i[7], "mfma", 2.0 * i[1] * i[2] * i[3]),
    "spv_gemm_tn": lambda i: ("gemm_tn", i[0:3], BF16, "mfma", 2.0 * i[0] * i[1] * i[2]),
    "spv_gemm_tn_fold": lambda i: ("gemm_tn", i[0:3], BF16, "mfma", 2.0 * i[0] * i[1] * i[2]),
    # (nprob, rows, splits, nfolds, part): the batched weight gradients; the work comes as the caller's hint (sum of 2 m n rows / the
    # slabs read + the sums written)
    "spv_gemm_tn_batch_part": lambda i: (("gemm_tn_batch", i[0:3], BF16, "mfma", float(i[-1])) if i[4] == 1 else
                                         ("splitk_reduce_batch", i[0:4], F32, "hbm", float(i[-1]))),
    # token-gradient pass of the embedding: read dtok, write the masked copy (when asked for: pointer 2)
    "spv_embed_bwd": lambda i: ("embed_bwd", i[0:3], i[3], "hbm", 1.0 * i[0] * i[1] * i[2] * _es(i[3]) * (1 if (i[-2] >> 2) & 1 else 2)),
    "spv_fnet_cls_fwd": lambda i: ("fnet_cls_fwd", i[0:3], i[3], "hbm", 1.0 * i[0] * (i[1] + 1) * i[2] * _es(i[3])),
    "spv_fnet_cls_bwd": lambda i: ("fnet_cls_bwd", i[0:3], i[3], "hbm", 1.0 * i[0] * (i[1] + 1) * i[2] * _es(i[3])),
    # one gathered row (n values) + row 0 (embed values) per image, read and written
    "spv_permut_row0_fwd": lambda i: ("permut_row0_fwd", i[0:4], i[4], "hbm", 2.0 * i[0] * (i[2] + i[3]) * _es(i[4])),
    # the dense input gradient [batch, d] written once (+ the n + embed values read)
    "spv_permut_row0_bwd": lambda i: ("permut_row0_bwd", i[0:4], i[4], "hbm", 1.0 * i[0] * (i[1] + i[2] + i[3]) * _es(i[4])),
    # (B, C, H, W, patch, K, mode, dtype): read the fp32 image, write the patch / token-row matrix
    "spv_patchify": lambda i: ("patchify", i[0:5], i[7], "hbm",
                               1.0 * i[0] * i[1] * i[2] * i[3] * 4 + 1.0 * i[0] * ((i[2] // i[4]) * (i[3] // i[4]) + (i[6] == 2)) * i[5] * _es(i[7])),
    # 32 x 64 tiles: fp32 read, two bf16 copies written
    "spv_weight_shadows_multi": lambda i: ("weight_shadows_multi", i[0:1], i[1], "hbm", 2048.0 * i[0] * (4 + 2 * _es(i[1]))),
    # read h [rows,n] + x [rows,k], write out [rows,n]
    "spv_spectre_tail_fwd": lambda i: ("tail_fwd", i[0:3], i[3], "hbm", i[0] * (2.0 * i[1] + i[2]) * _es(i[3])),
    # read dout, h; write dh [rows,n] and -- unless the caller passes no dx (MHPermutMix: the pooled skip gradient is added by the data
    # gradient GEMM's epilogue instead; pointer 7 of the call is NULL then) -- dx_pool [rows,k]
    "spv_spectre_tail_bwd": lambda i: ("tail_bwd" if not (i[-2] >> 7) & 1 else "tail_bwd_nodx", i[0:3], i[3], "hbm",
                                       i[0] * (3.0 * i[1] + (0 if (i[-2] >> 7) & 1 else i[2])) * _es(i[3])),
    # + read dx_add and up_src [rows,k]
    "spv_spectre_tail_bwd_up": lambda i: ("tail_bwd_up", i[0:3], i[3], "hbm", i[0] * (3.0 * i[1] + 3.0 * i[2]) * _es(i[3])),
    # read h3, res [rows,n], x [rows,k]; write f3, out2 [rows,n]
    "spv_spectre_tail_ln_fwd": lambda i: ("tail_ln_fwd", i[0:3], i[3], "hbm", i[0] * (4.0 * i[1] + i[2]) * _es(i[3])),
    # read dout2, f3, res, h3; write ds, dh3 [rows,n]
    "spv_spectre_tail_ln_bwd": lambda i: ("tail_ln_bwd", i[0:3], i[3], "hbm", i[0] * 6.0 * i[1] * _es(i[3])),
    "spv_add_layernorm_fwd": lambda i: ("addln_fwd", i[0:2], i[3], "hbm", 3.0 * i[0] * i[1] * _es(i[3])),
    "spv_add_layernorm_bwd": lambda i: ("addln_bwd", i[0:2], i[3], "hbm", (3.0 + (i[2] == 1)) * i[0] * i[1] * _es(i[3])),
    "spv_permut_gather_fwd": lambda i: ("gather_fwd", i[1:4], i[4], "hbm", i[1] * i[3] * (1.0 + i[2]) * _es(i[4])),
    "spv_permut_gather_bwd": lambda i: ("gather_bwd", i[0:3], i[3], "hbm", i[0] * i[2] * (1.0 + i[1]) * _es(i[3])),
    "spv_fnet_mix": lambda i: ("fnet_mix", i[0:3], i[3], "hbm", 2.0 * i[0] * i[1] * i[2] * _es(i[3])),
    # mixer + LayerNorm-1 + residual: read x, write the pre-norm tensor and x1
    "spv_fnet_ln_fwd": lambda i: ("fnet_ln_fwd", i[0:3], i[3], "hbm", 3.0 * i[0] * i[1] * i[2] * _es(i[3])),
    # read dout and the pre-norm tensor, write dx
    "spv_fnet_ln_bwd": lambda i: ("fnet_ln_bwd", i[0:3], i[3], "hbm", 3.0 * i[0] * i[1] * i[2] * _es(i[3])),
    "spv_haar_ln_fwd": lambda i: ("haar_ln_fwd", i[0:2], i[2], "hbm", 2.0 * i[0] * i[1] * _es(i[2])),
    "spv_haar_ln_bwd": lambda i: ("haar_ln_bwd", i[0:2], i[2], "hbm", 3.0 * i[0] * i[1] * _es(i[2])),
    "spv_haar_dwt": lambda i: ("haar_dwt", i[0:3], i[6], "hbm", 2.0 * i[0] * i[1] * i[2] * _es(i[6])),
    # p, g, m, v read + p, m, v written, 2048 elements per workgroup (the last chunk of a tensor is short: an upper bound)
    "spv_adamw_multi": lambda i: ("adamw_multi", i[0:1], F32, "hbm", 7.0 * 4 * 2048 * i[0]),
    # ... plus the moving average read and written (every tensor averaged: an upper bound)
    "spv_adamw_multi_ema": lambda i: ("adamw_multi_ema", i[0:1], F32, "hbm", 9.0 * 4 * 2048 * i[0]),
    "spv_adamw_multi_ctl_ema": lambda i: ("adamw_multi_ctl_ema", i[0:1], F32, "hbm", 9.0 * 4 * 2048 * i[0]),
    # step control: the gradient read once (chunks as above), the per-chunk fp64 partials folded, the optimizer's seven streams
    "spv_grad_sumsq": lambda i: ("grad_sumsq", i[0:1], F32, "hbm", 4.0 * 2048 * i[0]),
    "spv_step_control": lambda i: ("step_control", i[0:2], F32, "hbm", 8.0 * i[0] + 64),
    # gradient accumulation: the gradient read, the accumulator read and written (chunks as above); the control launch as without
    "spv_grad_accumulate": lambda i: ("grad_accumulate", i[0:1], F32, "hbm", 3.0 * 4 * 2048 * i[0]),
    "spv_step_control_accum": lambda i: ("step_control_accum", i[0:2], F32, "hbm", 8.0 * i[0] + 64),
    "spv_adamw_multi_ctl": lambda i: ("adamw_multi_ctl", i[0:1], F32, "hbm", 7.0 * 4 * 2048 * i[0]),
    # one launch for the step's small opening jobs: the sum of its roles' compulsory bytes, handed over as the caller's hint
    "spv_step_prologue": lambda i: ("step_prologue", (), BF16, "hbm", float(i[-1])),
    "spv_weight_shadows": lambda i: ("weight_shadows", i[0:2], i[3], "hbm", i[0] * i[1] * (4.0 + 2 * _es(i[3]))),
    "spv_dropout": lambda i: ("dropout", i[0:1], i[1], "hbm", 2.0 * i[0] * _es(i[1])),
    "spv_axpby": lambda i: ("axpby", i[0:1], i[1], "hbm", 3.0 * i[0] * _es(i[1])),
    "spv_colsum": lambda i: ("colsum", i[0:2], i[2], "hbm", 1.0 * i[0] * i[1] * _es(i[2])),
    # (n, batch, chans, height, width, world, rank, steps, shuffle, mode, label dtype): index and labels written, the labels read, and
    # the image read as uint8 and written as fp32 (mode 1) or uint8 (mode 2)
    "spv_loader_fetch": lambda i: ("loader_fetch", i[1:5], F32, "hbm",
                                   i[1] * (16.0 + (8 if i[10] else 1) + i[2] * i[3] * i[4] * {0: 0, 1: 5, 2: 2}.get(i[9], 0))),
    # (n, batch, chans, height, width, world, rank, steps, shuffle, label dtype): index, labels and the table row written, the label
    # read, the image read as uint8 and written as fp32
    "spv_loader_fetch_augment": lambda i: ("loader_fetch_augment", i[1:5], F32, "hbm",
                                           i[1] * (16.0 + (8 if i[9] else 1) + 64.0 + i[2] * i[3] * i[4] * 5)),
    # the same integers: as above, and the image read a second time by the contrast mean's pre-pass (its partial sums are a few floats)
    "spv_loader_fetch_augment_tiled": lambda i: ("loader_fetch_augment_tiled", i[1:5], F32, "hbm",
                                                 i[1] * (16.0 + (8 if i[9] else 1) + 64.0 + i[2] * i[3] * i[4] * 6)),
    # (label dtype, n, chans, height, width, layout, classes): the payload read and -- unless dst is NULL (pointer 1) -- written once
    "spv_dataset_ingest": lambda i: ("dataset_ingest", i[1:5], F32, "hbm", 1.0 * i[1] * i[2] * i[3] * i[4] * (1 if (i[-2] >> 1) & 1 else 2)),
    "spv_cast": lambda i: ("cast", i[2:3], i[1], "hbm", 1.0 * i[2] * (_es(i[0]) + _es(i[1]))),
}


class KernelTimer:
    def __init__(self):
        self.records = []  # (name, key, start, end)
        self.empties = []  # empty pairs recorded BETWEEN the kernel brackets, i.e. with the queue as busy as it is around them
        self.overhead_s = 0.0
        self.passes = 0    # steps recorded (bench.py counts them: per-step totals = totals / passes)

    def bracket(self, name, key, launch):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        self.records.append((name, key, e0, e1))
        if len(self.records) % 8 == 0:
            z0, z1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            z0.record()
            z1.record()
            self.empties.append((z0, z1))

    def _groups(self):
        torch.cuda.synchronize()
        if self.empties:
            # what a bracket adds to the kernel's own duration: the median of the empty pairs taken inside the pass (a pair on an
            # idle stream read 5-13 us depending on the box; the in-pass median agrees with rocprofv3's durations)
            self.overhead_s = sorted(a.elapsed_time(b) for a, b in self.empties)[len(self.empties) // 2] * 1e-3
            self.empties = []
        groups = {}
        for name, key, e0, e1 in self.records:
            g = groups.setdefault((name, key), [0, 0.0])
            g[0] += 1
            # the raw bracket: NOT reduced by the empty-pair overhead (round 2 subtracted 4.5 us per bracket and read the layer GEMM at
            # 30.85 us where rocprofv3 measured 34.35; the raw bracket is the conservative figure, within a few per cent of rocprofv3)
            g[1] += max(e0.elapsed_time(e1) * 1e-3, 1e-7)
        return groups

    @staticmethod
    def _work(name, key):
        """-> (label, shape, dtype name, bound or None, algorithmic work per launch, peak per second)"""
        model = _WORK_MODELS.get(name)
        if model is not None:
            label, shape, dt, bound, work = model(key)
            peak = PEAK_TFLOPS[dt] * 1e12 if bound == "mfma" else PEAK_HBM_GBS * 1e9
            return label, list(shape), "bf16" if dt == BF16 else "f32", bound, work, peak
        if name.startswith("torch:") and key and key[0] > 0:  # bench.py's own brackets around torch ops: key = (bytes,)
            return name, [], "f32", "hbm", float(key[0]), PEAK_HBM_GBS * 1e9
        return name.replace("spv_", ""), list(key[:4]), "-", None, 0.0, 1.0

    def summary(self):
        out = []
        for (name, key), (cnt, tot) in sorted(self._groups().items(), key=lambda kv: -kv[1][1]):
            label, shape, dt, bound, work, peak = self._work(name, key)
            d = dict(kernel=label, shape=shape, dtype=dt, launches=cnt, avg_us=round(tot / cnt * 1e6, 2), total_ms=round(tot * 1e3, 3))
            if bound is not None:
                ach = work * cnt / tot
                d.update(bound=bound, achieved=round(ach / (1e12 if bound == "mfma" else 1e9), 2),
                         unit="TFLOP/s" if bound == "mfma" else "GB/s", frac=round(ach / peak, 4), algorithmic=int(work))
            out.append(d)
        return out

    def roofline(self):
        """the single modelled (kernel, shape) with the largest total time in the recorded steps"""
        s = [d for d in self.summary() if "bound" in d]
        if not s:
            return None
        d = s[0]
        peak = (PEAK_TFLOPS[BF16 if d["dtype"] == "bf16" else F32]) if d["bound"] == "mfma" else PEAK_HBM_GBS
        return dict(bound=d["bound"], achieved=d["achieved"], peak=peak, unit=d["unit"], frac=d["frac"], traffic=None,
                    kernel=d["kernel"], shape=d["shape"], avg_us=d["avg_us"], launches=d["launches"],
                    event_overhead_us=round(self.overhead_s * 1e6, 2))


def set_kernel_timer(t):
    _native.timer = t


def _timing():
    return _native.timer is not None
