"""float64 numpy restatement of the training meter (include/spv.h): the reference the CPU and GPU tests compare with.
Built on eval_ref.py's rules (spv_eval_head's):

    pred[r]   index of the FIRST maximum of z_r among its ordered entries: a NaN never wins, a row without an ordered maximum (every
              entry NaN or -inf) predicts class 0.  On rows without NaN this is torch.argmax / numpy.argmax.
    counted   0 <= y_r < C; any other label: not in seen / top1 / topk, and the step's loss is NaN
    top-k hit #{j : z_j > z_y} + #{j < y : z_j == z_y} < k          (k = 1: pred == y on rows without NaN)
    step loss mean_r(logsumexp(z_r) - z_r[y_r]) rounded to fp32 (the kernel's own fp32 loss is compared with this to a tolerance; the
              meter's books are defined on the fp32 value the kernel RETURNS, which is what `step` takes when given)
    meter     cursor / capacity / dropped, int totals, float64 sums of the fp32 step values (one add per step), log rows
"""
import numpy as np

import eval_ref as E


def predictions(z):
    z = np.asarray(z, np.float64)
    return E.first_argmax(np.where(np.isnan(z), -np.inf, z))


def hits(logits, labels, k):
    """-> (seen, top1, topk) of one step"""
    z = np.asarray(logits, np.float64)
    labels = np.asarray(labels, np.int64)
    rows, C = z.shape
    pred = predictions(z)
    seen = top1 = topk = 0
    for r in range(rows):
        y = int(labels[r])
        if not 0 <= y < C:
            continue
        seen += 1
        top1 += int(pred[r] == y)
        topk += int(E.topk_hit(z[r], y, k))
    return seen, top1, topk


def step_loss(logits, labels):
    """mean cross-entropy in float64, rounded once to fp32; NaN when a label is outside the classes"""
    z = np.asarray(logits, np.float64)
    labels = np.asarray(labels, np.int64)
    rows, C = z.shape
    if ((labels < 0) | (labels >= C)).any():
        return np.float32(np.nan)
    with np.errstate(invalid="ignore"):
        return np.float32(sum(E.row_loss(z[r], int(labels[r])) for r in range(rows)) / rows)


class Meter:
    """the block's books"""

    def __init__(self, capacity, k):
        assert capacity >= 1 and 1 <= k <= 8
        self.capacity, self.k = int(capacity), int(k)
        self.reset()

    def reset(self):
        self.cursor = self.dropped = self.seen = self.top1 = self.topk = 0
        self.loss_sum = self.soft_sum = self.ce_sum = np.float64(0.0)
        self.rows = []

    def step(self, logits, labels, loss=None, soft=0.0, ce=0.0):
        """one metered forward.  loss / soft / ce: the fp32 values the kernel returned (None: this module's own step_loss)"""
        loss = np.float32(step_loss(logits, labels) if loss is None else loss)
        soft, ce = np.float32(soft), np.float32(ce)
        seen, top1, topk = hits(logits, labels, self.k)
        if self.cursor < self.capacity:
            self.rows.append((float(loss), float(soft), float(ce), top1, topk))
            self.cursor += 1
        else:
            self.dropped += 1
        self.seen += seen
        self.top1 += top1
        self.topk += topk
        self.loss_sum = self.loss_sum + np.float64(loss)   # one float64 add of the fp32 value per step
        self.soft_sum = self.soft_sum + np.float64(soft)
        self.ce_sum = self.ce_sum + np.float64(ce)
        return seen, top1, topk

    def read(self):
        steps = self.cursor + self.dropped
        return {"steps": steps, "dropped": self.dropped, "seen": self.seen, "top1": self.top1, "topk": self.topk,
                "loss_sum": float(self.loss_sum), "soft_sum": float(self.soft_sum), "ce_sum": float(self.ce_sum), "rows": list(self.rows),
                "loss_mean": float(self.loss_sum) / steps if steps else 0.0,
                "accuracy": self.top1 / self.seen if self.seen else 0.0, "accuracy_topk": self.topk / self.seen if self.seen else 0.0}
