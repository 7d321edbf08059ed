"""The training meter: the loop's per-step bookkeeping (reference spectre_vit/repl/train.py:221-224, 243; distillation cell :329-332,
355-361) kept on the device by the loss kernels themselves (csrc/spv_head.hip, csrc/spv_distill.hip; include/spv.h).

    meter = TrainMeter(capacity=steps_per_epoch, topk=5, device=device)
    criterion = CrossEntropyLoss(meter=meter)            # or DistillationLoss(..., meter=meter)
    for img, label in batches:                            # eager or replayed from a graph: the criterion carries the meter
        loss = criterion(model(img), label); ...
    epoch = meter.read()                                  # ONE device-to-host copy
    meter.reset()

A metered loss forward counts top-1 / top-k hits on the row walk it already does and its joining workgroup writes the step's loss and
hit counts into log row ``cursor`` of one int64 block -- the row index is read from the device, so a captured launch logs a new row
at every replay.  The loss itself keeps the bits of the un-metered kernel.
"""
import struct

import numpy as np
import torch

# the block's words (include/spv.h)
CURSOR, CAPACITY, DROPPED, SEEN, TOP1, TOPK, LOSS_SUM, SOFT_SUM, CE_SUM = range(9)
HEADER_WORDS = 16
ROW_WORDS = 5
MAX_CAPACITY = 1 << 24


def _check_args(capacity, topk):
    if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or not 1 <= int(capacity) <= MAX_CAPACITY:
        raise ValueError(f"TrainMeter: capacity={capacity!r} must be an integer in 1..{MAX_CAPACITY} (the log rows of one epoch)")
    if isinstance(topk, bool) or not isinstance(topk, (int, np.integer)) or not 1 <= int(topk) <= 8:
        raise ValueError(f"TrainMeter: topk={topk!r} must be an integer in 1..8")
    return int(capacity), int(topk)


def decode(words):
    """The dict of ``TrainMeter.read()`` from the block's int64 words on the host (numpy int64 [HEADER_WORDS + ROW_WORDS * capacity])."""
    w = np.ascontiguousarray(words, dtype=np.int64)
    cursor, capacity, dropped = int(w[CURSOR]), int(w[CAPACITY]), int(w[DROPPED])
    sums = w[LOSS_SUM:CE_SUM + 1].view(np.float64)
    n = max(0, min(cursor, capacity))
    log = w[HEADER_WORDS:HEADER_WORDS + ROW_WORDS * n].reshape(n, ROW_WORDS)
    f32 = (log[:, :3] & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
    rows = [(float(f32[i, 0]), float(f32[i, 1]), float(f32[i, 2]), int(log[i, 3]), int(log[i, 4])) for i in range(n)]
    steps = cursor + dropped   # every step is in the totals, logged or not
    seen, top1, topk = int(w[SEEN]), int(w[TOP1]), int(w[TOPK])
    return {"steps": steps, "dropped": dropped, "seen": seen, "top1": top1, "topk": topk,
            "loss_sum": float(sums[0]), "soft_sum": float(sums[1]), "ce_sum": float(sums[2]), "rows": rows,
            "loss_mean": float(sums[0]) / steps if steps else 0.0,
            "accuracy": top1 / seen if seen else 0.0, "accuracy_topk": topk / seen if seen else 0.0}


class TrainMeter:
    """One device-resident block of the training meter: a header (cursor, capacity, dropped; seen / top1 / topk as int64; the sums of
    the steps' fp32 loss, soft and CE terms as float64) and ``capacity`` log rows, one per step.  Its address never changes, so a
    criterion that holds it can be captured into a graph.  A step past ``capacity`` writes no row (``dropped`` counts it) but still
    enters the totals.  Bad arguments raise before any device is touched."""

    def __init__(self, capacity, topk=5, device="cuda"):
        self.capacity, self.topk = _check_args(capacity, topk)
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"TrainMeter lives on the GPU the loss kernels run on, got device={str(device)!r}")
        from . import _native
        words = int(_native.call("spv_train_meter_words", self.capacity))
        if words != HEADER_WORDS + ROW_WORDS * self.capacity:
            raise RuntimeError(f"libspv_hip.so lays the meter of {self.capacity} rows out in {words} words, this module in "
                               f"{HEADER_WORDS + ROW_WORDS * self.capacity}")
        fresh = torch.zeros((words,), dtype=torch.int64)
        fresh[CAPACITY] = self.capacity
        self._fresh = fresh.to(device)    # what reset() copies: a zero header with its capacity, a zero log
        self._block = self._fresh.clone()

    def reset(self):
        """zero header (capacity kept) and log: one device-to-device copy on the current stream.  Between epochs; never captured."""
        self._block.copy_(self._fresh)

    def tensor(self):
        """the raw int64 block (a caller's all_reduce, a test's guard words)"""
        return self._block

    def read(self):
        """ONE device-to-host copy of the whole block -> {"steps", "dropped", "seen", "top1", "topk", "loss_sum", "soft_sum", "ce_sum",
        "rows": [(loss, soft, ce, top1, topk) per logged step], "loss_mean" (loss_sum / steps), "accuracy" (top1 / seen),
        "accuracy_topk"}.  steps = logged + dropped: the steps in the totals."""
        return decode(self._block.cpu().numpy())


def float_bits(x):
    """the fp32 bit pattern of a Python float that holds an fp32 value (test aid: log rows are compared bit for bit)"""
    return struct.unpack("<I", struct.pack("<f", x))[0]
