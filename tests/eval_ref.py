"""float64 numpy restatement of the inference metrics (spv_eval_head, include/spv.h): the reference the CPU and GPU tests compare with.

    pred[r]   index of the FIRST maximum of z_r (torch.argmax's documented tie rule)
    counted   r < n_valid and 0 <= y_r < C (label -1, or any label outside the classes: predicted, never counted)
    top-k hit #{j : z_j > z_y} + #{j < y : z_j == z_y} < k          (k = 1: pred == y)
    loss_r    logsumexp(z_r) - z_r[y_r], max-subtracted
    stats     seen / top1 / topk counts and the running sum of loss_r, batch after batch
"""
import numpy as np


def new_stats():
    return {"seen": 0, "top1": 0, "topk": 0, "loss_sum": 0.0}


def first_argmax(z):
    z = np.asarray(z, np.float64)
    return np.argmax(z, axis=1).astype(np.int64)   # numpy documents the first occurrence


def topk_hit(row, y, k):
    """the rule itself, on one row"""
    zy = row[y]
    return int((row > zy).sum() + (row[:y] == zy).sum()) < k


def row_loss(row, y):
    m = row.max()
    return float(m + np.log(np.exp(row - m).sum()) - row[y])


def eval_head(logits, labels, n_valid, k, stats=None):
    """-> (pred int64 [rows], stats): `stats` (new_stats() when None) with this batch added"""
    z = np.asarray(logits, np.float64)
    labels = np.asarray(labels, np.int64)
    rows, C = z.shape
    stats = dict(stats) if stats is not None else new_stats()
    pred = first_argmax(z)
    batch_loss = 0.0
    for r in range(min(int(n_valid), rows)):
        y = int(labels[r])
        if not 0 <= y < C:
            continue
        stats["seen"] += 1
        stats["top1"] += int(pred[r] == y)
        stats["topk"] += int(topk_hit(z[r], y, k))
        batch_loss += row_loss(z[r], y)
    stats["loss_sum"] += batch_loss   # the batch's sum first, then one add to the running sum
    return pred, stats
