"""float64 restatement of the weight average FusedAdamW keeps (include/spv.h: spv_adamw_multi_ema), written from the definition and
independent of spectre_vit.optim: timm ModelEmaV2's rule, e <- e + w_t (p' - e), fed with the device's own fp32 weights after every
step, w_t being the fp32 value the kernel uses."""
import numpy as np

U = 2.0 ** -24   # unit roundoff of fp32


def weight(step, decay, warmup):
    """w_t as fp32: float32(1 - decay) from a double difference; with warm-up max(that, float32(9) / float32(10 + step)) -- timm's
    decay_t = min(decay, (1 + step) / (10 + step)); step = the Adam step count of this step, 1 on the first applied step"""
    w = np.float32(1.0 - np.float64(decay))
    if warmup:
        w = max(w, np.float32(9.0) / np.float32(10.0 + step))
    return np.float32(w)


class Average:
    """the recurrence of one tensor in float64, started at p_0"""

    def __init__(self, p0):
        self.e = np.asarray(p0, dtype=np.float64).copy()
        self.steps = 0

    def update(self, p_new, w):
        assert np.asarray(w).dtype == np.float32
        self.e += np.float64(w) * (np.asarray(p_new, dtype=np.float64) - self.e)
        self.steps += 1
        return self.e


def bound(k, p, e):
    """|e - e64| <= 4 k 2^-24 max(|p|, |e|) over one tensor after k steps: the difference p' - e and the fused multiply-add round
    once each, at most 2 * 2^-24 * M per step together; the recurrence contracts (factor 1 - w_t <= 1), so the steps' errors add at
    most; the remaining factor 2 is margin"""
    m = max(float(np.max(np.abs(p))), float(np.max(np.abs(e))))
    return 4.0 * k * U * m


def ratio(e_dev, e64, k, p):
    """worst |e - e64| of one tensor over its bound (<= 1 passes)"""
    e_dev = np.asarray(e_dev, dtype=np.float64)
    return float(np.max(np.abs(e_dev - e64))) / bound(k, p, e_dev)
