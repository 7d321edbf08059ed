"""AdamW on one HIP launch per step -- drop-in for ``torch.optim.AdamW`` as the reference's script builds it
(spectre_vit/repl/train.py:199-201: ``optim.AdamW(model.parameters(), betas=..., lr=..., weight_decay=...)``).

Same update rule, same ``state`` layout (``step`` / ``exp_avg`` / ``exp_avg_sq`` per parameter, so ``state_dict()`` is
interchangeable with torch's), one parameter group or many.  torch's own fused kernel spends 100+ us per step on the FFT
model's 63 small tensors; ``spv_adamw_multi`` walks a chunk table in a single launch.  ``capturable=True`` keeps the step
count on the device, so the whole training step can be captured in a HIP graph (spectre_vit/graph.py).

Step control (``schedule=``, ``max_grad_norm=``, ``skip_nonfinite=``): what the reference's loop does on the host around
``optimizer.step()`` -- ``CosineAnnealingLR`` (train.py:202-203), ``GradScaler``'s dropped step on an inf / NaN gradient
(train.py:205,236-238), and the usual ``clip_grad_norm_`` -- decided on the device from the step count and the gradient, so a
replayed graph follows the schedule instead of keeping the captured rate.  Per step: ``spv_grad_sumsq`` per group, one
``spv_step_control`` that fills a 64-byte control block (include/spv.h: spv_step_ctl), ``spv_adamw_multi_ctl`` per group.

Weight averaging (``ema_decay=``): an exponential moving average of every parameter, kept as ``state[p]["ema"]`` and updated by the
optimizer launch itself from the registers that hold the new weight (``spv_adamw_multi_ema`` / ``spv_adamw_multi_ctl_ema``): no extra
launch, nothing for the host to do between two graph replays, and a dropped step leaves the average where it is.
``ema_weights()`` / ``ema_state_dict()`` take the averaged weights to validation and into a checkpoint.

Gradient accumulation (``accumulate_steps=k``): every ``step()`` is a micro-step that adds the gradients to fp32 accumulators; the
device counts the micro-steps of the open window and every k-th one applies AdamW to the mean.  The decision is the control block's
``apply`` flag, so ONE captured graph serves every micro-step.  Per micro-step: ``spv_grad_accumulate`` per group (it also forms the
accumulator's sum of squares, so ``spv_grad_sumsq`` is not launched), one ``spv_step_control_accum``, ``spv_adamw_multi_ctl[_ema]`` per
group on a table whose gradient column is the accumulator.

The update rule is the pluggable part (``_FusedOptimizer``): ``FusedAdam`` and ``FusedSGD`` are the script's two other optimizer lines
(train.py:197-198, :307: ``optim.Adam(...)``, ``optim.SGD(..., nesterov=True, momentum=0.9)``) on the same tables, control block,
accumulators and average -- ``spv_adam_multi*`` / ``spv_sgd_multi*`` where AdamW launches ``spv_adamw_multi*``.
"""
from __future__ import annotations

import contextlib
import math
import struct
import warnings

import numpy as np
import torch

from spectre_vit import _native, hip_ops
from spectre_vit.hip_ops import _stream

_CHUNK = 2048
_CTL_FMT = "<ddfifiii24x"   # include/spv.h: spv_step_ctl (a, b, clip_coef, apply, grad_norm, sched_step, skipped, micro, reserved)
_CTL_FIELDS = ("a", "b", "clip_coef", "apply", "grad_norm", "sched_step", "skipped", "micro")
_CTL_SCHEDULE, _CTL_CLIP, _CTL_SKIP = 1, 2, 4


class CosineSchedule:
    """Linear warm-up, then cosine annealing, as a function of the number t of ``step()`` calls made so far (skipped steps count, the
    way ``scheduler.step()`` sits in a user's loop).  W = warmup_steps, T = total_steps:

        t <  W:  lr = base * (t + 1) / (W + 1)                                        LinearLR(start_factor=1/(W+1), total_iters=W)
        t >= W:  lr = eta_min + (base - eta_min) * (1 + cos(pi * min(t - W, T - W) / (T - W))) / 2       CosineAnnealingLR(T - W, eta_min)

    i.e. torch's ``SequentialLR([LinearLR, CosineAnnealingLR], milestones=[W])`` for t <= T.  Past T the rate STAYS at eta_min (torch's
    closed form would rise again).  ``lr_at`` is the float64 definition; the device evaluates the same expressions in fp64 and
    rounds the rate to fp32 once."""

    def __init__(self, total_steps, warmup_steps=0, eta_min=0.0):
        total_steps, warmup_steps, eta_min = int(total_steps), int(warmup_steps), float(eta_min)
        if warmup_steps < 0:
            raise ValueError(f"CosineSchedule: warmup_steps={warmup_steps} must be >= 0")
        if total_steps <= warmup_steps:
            raise ValueError(f"CosineSchedule: total_steps={total_steps} must be larger than warmup_steps={warmup_steps}")
        if not eta_min >= 0.0:
            raise ValueError(f"CosineSchedule: eta_min={eta_min} must be >= 0")
        self.total_steps, self.warmup_steps, self.eta_min = total_steps, warmup_steps, eta_min

    def lr_at(self, t, base_lr):
        t, base_lr = int(t), float(base_lr)
        W, T = self.warmup_steps, self.total_steps
        if t < W:
            return base_lr * (t + 1) / (W + 1)
        if t >= T:
            return self.eta_min
        return self.eta_min + (base_lr - self.eta_min) * (1.0 + math.cos(math.pi * (t - W) / (T - W))) / 2.0

    def __repr__(self):
        return f"CosineSchedule(total_steps={self.total_steps}, warmup_steps={self.warmup_steps}, eta_min={self.eta_min})"


def ema_weight_at(step, decay, warmup=False):
    """The weight w_t of the new parameters in the average at Adam step count `step` (1 on the first applied step), as the kernel
    forms it: w = float32(1 - decay) from a double difference; with warm-up max(w, float32(9) / float32(10 + step)) in fp32 --
    timm ModelEmaV2's decay_t = min(decay, (1 + step) / (10 + step)).  The average moves by e' = fmaf(w_t, p' - e, e).
    Returns the fp32 value as a Python float."""
    w = np.float32(1.0 - float(decay))
    if not warmup:
        return float(w)
    return float(max(w, np.float32(9.0) / np.float32(10.0 + int(step))))


def _check_ema_decay(d, who="FusedAdamW"):
    if d is None:
        return None
    if isinstance(d, bool) or not 0.0 <= float(d) < 1.0:
        raise ValueError(f"{who}: ema_decay={d!r} must be None or a float in [0, 1)")
    return float(d)


class _FusedOptimizer(torch.optim.Optimizer):
    """What does not depend on the update rule: the pointer and chunk tables with static_grads, the gradient accumulators, the
    step-control block with its first two launches and its readers, and the weights' moving average.  A rule (FusedAdamW, FusedAdam,
    FusedSGD below) supplies three things: the state it creates per parameter (_init_rule_state), the third and fourth column of a
    table row (_rule_columns), and its launch on the plain and on the control path (_launch / _launch_ctl).  The keyword arguments
    are documented at FusedAdamW.__init__."""

    @property
    def _who(self):
        return type(self).__name__

    # -- the rule's side ----------------------------------------------------------------------------------------------------------
    def _init_rule_state(self, p, group, st):
        raise NotImplementedError

    def _rule_columns(self, p, group):
        """the state tensors behind columns three and four of p's table row (None: the rule has no such column, the pointer is 0)"""
        raise NotImplementedError

    def _launch(self, group, t, step_ptr):
        """the plain launch of one group; step_ptr = the device-side count (capturable), 0 = t["host_step"] holds this step's count"""
        raise NotImplementedError

    def _launch_ctl(self, group, t, table, st):
        raise NotImplementedError

    def __init__(self, params, defaults, capturable=False, static_grads=False, schedule=None, max_grad_norm=None, skip_nonfinite=False,
                 ema_decay=None, ema_warmup=False, ema_exclude=None, accumulate_steps=None):
        if schedule is not None and not isinstance(schedule, CosineSchedule):
            raise ValueError(f"{self._who}: schedule must be a spectre_vit.optim.CosineSchedule or None, not {schedule!r}")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"{self._who}: max_grad_norm={max_grad_norm} must be > 0")
        self.schedule = schedule
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        if accumulate_steps is not None and (isinstance(accumulate_steps, bool) or not isinstance(accumulate_steps, (int, np.integer))
                                             or accumulate_steps < 1):
            raise ValueError(f"{self._who}: accumulate_steps={accumulate_steps!r} must be None or an int >= 1")
        self.accumulate_steps = None if accumulate_steps is None else int(accumulate_steps)
        self.step_control = (schedule is not None or max_grad_norm is not None or self.skip_nonfinite
                             or self.accumulate_steps is not None)
        if self.step_control and not capturable:
            raise ValueError(f"{self._who}: schedule / max_grad_norm / skip_nonfinite / accumulate_steps need capturable=True (a skipped "
                             "step leaves the step count where it is, so the count must live on the device)")
        defaults = dict(defaults, capturable=capturable)
        params = list(params)
        # a group default like the others -- but only where averaging is asked for: without it the groups keep exactly their old keys
        if ema_decay is not None or any(isinstance(g, dict) and "ema_decay" in g for g in params):
            defaults["ema_decay"] = _check_ema_decay(ema_decay, self._who)
        super().__init__(params, defaults)
        for group in self.param_groups:
            _check_ema_decay(group.get("ema_decay"), self._who)
        self.ema_warmup = bool(ema_warmup)
        if self.ema_warmup and not self.ema_enabled:
            raise ValueError(f"{self._who}: ema_warmup=True needs ema_decay in at least one parameter group")
        self._ema_exclude = frozenset(id(p) for p in (ema_exclude or ()))
        if self._ema_exclude and not self.ema_enabled:
            raise ValueError(f"{self._who}: ema_exclude needs ema_decay in at least one parameter group")
        self._ema_swapped = False
        self.static_grads = bool(static_grads)
        self._tables = {}  # group index -> dict(key, table, chunk_tensor, chunk_off, sizes, nchunks, step_dev)
        # step control: the device block (spv_step_ctl), the per-chunk fp64 partial sums and the device array of the groups' step
        # count pointers; built on the first step() -- before any capture -- and again after load_state_dict()
        self._ctl = None
        self._ctl_ws = None
        self._ctl_counts = (0, 0)   # (schedule step, skipped steps) a freshly built block starts from
        self._ctl_raw = None        # ... or the 64 raw bytes of a saved block (load_train_state), micro-step included
        self._acc = {}  # gradient accumulation: group index -> dict(sizes, flat, views), one allocation per group, made once

    def _table(self, gi, ps):
        """device-side pointer / chunk tables of one parameter group; rebuilt only when a pointer moved (in the steady state the
        caching allocator hands the same gradient blocks back every step; with GradReducer the gradients live in fixed buckets)"""
        # (the rule's state tensors are part of the key: load_state_dict() on an optimizer that has already stepped replaces them)
        group = self.param_groups[gi]
        cols = [tuple(0 if c is None else c.data_ptr() for c in self._rule_columns(p, group)) for p in ps]
        key = tuple((p.data_ptr(), p.grad.data_ptr(), p.numel()) + c for p, c in zip(ps, cols))
        # the averages' addresses belong to the key just as the moments' do
        emas = [self.state[p].get("ema") if self._averaged(p, self.param_groups[gi]) else None for p in ps]
        if any(e is not None for e in emas):
            key += tuple(0 if e is None else e.data_ptr() for e in emas)
        accs = None
        if self.accumulate_steps is not None:   # ... and so do the accumulators'
            views = self._accumulators(gi)
            accs = [views[id(p)] for p in ps]
            key += tuple(a.data_ptr() for a in accs)
        t = self._tables.get(gi)
        if t is not None and t["key"] == key:
            return t
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{self._who}: a parameter or gradient moved while a HIP graph is being captured (its pointer table "
                               "cannot be uploaded inside a capture): give the gradients fixed addresses with "
                               "spectre_vit.dp.GradReducer(model, always=True) and run a warm-up step first")
        dev = ps[0].device
        rows, ct, co, sizes = [], [], [], []
        for i, p in enumerate(ps):
            if not p.grad.is_contiguous() or p.grad.dtype != torch.float32:
                raise RuntimeError(f"{self._who} needs contiguous fp32 gradients")
            e = emas[i]
            if e is not None and (not e.is_cuda or e.dtype != torch.float32 or not e.is_contiguous() or e.shape != p.shape):
                raise RuntimeError(f"{self._who}: state['ema'] must be a contiguous fp32 tensor on the GPU, shaped like its parameter")
            rows += [p.data_ptr(), p.grad.data_ptr(), *cols[i]]
            n = p.numel()
            sizes.append(n)
            for off in range(0, n, _CHUNK):
                ct.append(i)
                co.append(off)
        t = dict(key=key,
                 table=torch.tensor(rows, dtype=torch.int64).to(dev), chunk_tensor=torch.tensor(ct, dtype=torch.int32).to(dev),
                 chunk_off=torch.tensor(co, dtype=torch.int32).to(dev), sizes=torch.tensor(sizes, dtype=torch.int32).to(dev),
                 nchunks=len(ct))
        if any(e is not None for e in emas):   # one float* per table row, NULL = not averaged (include/spv.h: spv_adamw_multi_ema)
            t["ema_table"] = torch.tensor([0 if e is None else e.data_ptr() for e in emas], dtype=torch.int64).to(dev)
        if accs is not None:   # one float* per table row for spv_grad_accumulate, and the optimizer's table with acc where g was
            t["acc_table"] = torch.tensor([a.data_ptr() for a in accs], dtype=torch.int64).to(dev)
            acc_rows = list(rows)
            acc_rows[1::4] = [a.data_ptr() for a in accs]
            t["table_acc"] = torch.tensor(acc_rows, dtype=torch.int64).to(dev)
        prev = self._tables.get(gi)
        if prev is not None:  # the step counter outlives a table rebuild
            for k in ("step", "host_step"):
                if k in prev:
                    t[k] = prev[k]
        self._tables[gi] = t
        return t

    def _accumulators(self, gi):
        """id(p) -> the fp32 accumulator of every parameter of group gi: views, shaped like the parameters, into ONE allocation whose
        slots are rounded up to four elements (16-byte aligned: spv_grad_accumulate's float4 walk relies on it).  Made once, for every
        parameter of the group whether it has a gradient yet or not, so the addresses never move; never under a graph capture."""
        group = self.param_groups[gi]
        sizes = tuple(p.numel() for p in group["params"])
        a = self._acc.get(gi)
        if a is not None and a["sizes"] == sizes:
            return a["views"]
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{self._who}: the gradient accumulators have to be allocated while a HIP graph is being captured (their "
                               "addresses cannot enter the pointer table inside a capture): run a warm-up step() before the capture")
        cuda = [p for p in group["params"] if p.is_cuda]
        if not cuda:
            raise RuntimeError(f"{self._who}: parameters must be contiguous fp32 tensors on the GPU (no CPU fallback)")
        flat = torch.zeros(sum((n + 3) // 4 * 4 for n in sizes), dtype=torch.float32, device=cuda[0].device)
        assert flat.data_ptr() % 16 == 0
        views, off = {}, 0
        for p, n in zip(group["params"], sizes):
            views[id(p)] = flat[off:off + n].view(p.shape)
            off += (n + 3) // 4 * 4
        self._acc[gi] = dict(sizes=sizes, flat=flat, views=views)
        return views

    def accumulated_grads(self):
        """the accumulators, in parameter order (the tensors themselves, not copies): after a micro-step the fp32 sequential sum of the
        open window's gradients, after a boundary the whole window's (divide by accumulate_steps for the mean)"""
        if self.accumulate_steps is None:
            raise RuntimeError(f"{self._who}: built without accumulate_steps: there is no accumulator")
        return [self._accumulators(gi)[id(p)] for gi, group in enumerate(self.param_groups) for p in group["params"]]

    def micro_step(self):
        """micro-steps already in the open window: 0 right after a boundary (and before the first step)"""
        if self.accumulate_steps is None:
            raise RuntimeError(f"{self._who}: built without accumulate_steps: there is no micro-step count")
        return self._read_ctl()["micro"]

    def load_state_dict(self, state_dict):
        """torch's loader replaces the per-parameter state (moments, step count): drop the device tables so that the next step() reads
        the loaded step count and points at the loaded moment tensors (in-place resume / rollback of an optimizer that has stepped).
        Averaging: a group's ``ema_decay`` comes from the loaded group when it has one and stays this optimizer's otherwise; parameters
        that arrive without ``"ema"`` start their average from their current values at the next step().
        Accumulation: the accumulators are not part of a checkpoint, so the window restarts (micro = 0: the next micro-step assigns);
        a saved ``micro_step`` other than 0 means that the open window's micro-batches are lost, and warns."""
        if self._ema_swapped:
            raise RuntimeError(f"{self._who}: load_state_dict() inside ema_weights(): the parameters hold the averaged weights")
        mine = [g["ema_decay"] for g in self.param_groups] if "ema_decay" in self.defaults else None
        capturable = [g["capturable"] for g in self.param_groups]
        super().load_state_dict(state_dict)
        for i, g in enumerate(self.param_groups):
            g.setdefault("capturable", capturable[i])   # (torch.optim.SGD's groups carry no such key)
            if "ema_decay" in g:
                _check_ema_decay(g["ema_decay"], self._who)
            elif mine is not None:
                g["ema_decay"] = mine[i]
        self._tables = {}
        for st in self.state.values():
            if isinstance(st.get("step"), torch.Tensor):
                st["step"] = st["step"].float()
        if self.step_control:   # the control block is rebuilt by the next step(), from the loaded counters
            sc = state_dict.get("step_control") or {}
            self._ctl_counts = (int(sc.get("schedule_step", 0)), int(sc.get("skipped_steps", 0)))
            self._ctl = self._ctl_ws = self._ctl_raw = None
            if self.accumulate_steps is not None and int(sc.get("micro_step", 0)) != 0:
                warnings.warn(f"{self._who}.load_state_dict: the state was saved {int(sc['micro_step'])} micro-step(s) into an accumulation "
                              "window; the accumulators are not checkpointed, so the window restarts at micro-step 0", stacklevel=2)

    def state_blocks(self):
        """the optimizer's device-resident state as named tensors -- the tensors themselves, at the addresses the launches use --
        for a spectre_vit.checkpoint.StateSnapshot: every per-parameter entry as "optim/<index>/<key>" in state_dict()'s numbering
        (moments, ``ema``, the step count: one tensor per group, named once), with step control the raw 64-byte control block as
        "optim/control_block", with accumulate_steps every group's accumulators as "optim/accumulators/<group>" (the flat allocation,
        slot padding included).  Reads nothing from the device.  After the first step(): the moments, the step count and the
        control block are made there.  -> (blocks, host_state, aliases) as spectre_vit.checkpoint.optimizer_blocks"""
        from spectre_vit.checkpoint import optimizer_blocks
        blocks, host_state, aliases = optimizer_blocks(self)
        if self.step_control:
            if self._ctl is None:
                raise RuntimeError(f"{self._who}.state_blocks(): the control block is built by the first step()")
            blocks.append(("optim/control_block", self._ctl))
        if self.accumulate_steps is not None:
            for gi in range(len(self.param_groups)):
                self._accumulators(gi)
                blocks.append((f"optim/accumulators/{gi}", self._acc[gi]["flat"]))
        return blocks, host_state, aliases

    def load_train_state(self, state_dict, control_block=None, accumulators=None):
        """load_state_dict(state_dict) plus what a checkpoint of a RUNNING window needs (spectre_vit.checkpoint): control_block, the 64
        raw bytes state_blocks() saved -- the schedule count, the skipped count and the micro-step of the open window, with the last
        boundary's rate and norm -- and accumulators, one flat fp32 tensor per parameter group, copied bit for bit into this
        optimizer's.  The window then continues where it was saved: no warning, nothing lost."""
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")   # (the open window is restored below)
            self.load_state_dict(state_dict)
        if self.step_control and control_block is not None:
            raw = bytes(control_block.cpu().contiguous().view(torch.uint8).numpy().tobytes()) if isinstance(control_block, torch.Tensor) \
                else bytes(control_block)
            if len(raw) != struct.calcsize(_CTL_FMT):
                raise ValueError(f"{self._who}.load_train_state: the control block is {struct.calcsize(_CTL_FMT)} bytes, got {len(raw)}")
            c = dict(zip(_CTL_FIELDS, struct.unpack(_CTL_FMT, raw)))
            self._ctl_counts, self._ctl_raw = (c["sched_step"], c["skipped"]), raw
        if self.accumulate_steps is not None and accumulators is not None:
            if len(accumulators) != len(self.param_groups):
                raise ValueError(f"{self._who}.load_train_state: {len(accumulators)} accumulator blocks for {len(self.param_groups)} groups")
            for gi, saved in enumerate(accumulators):
                self._accumulators(gi)
                flat = self._acc[gi]["flat"]
                if saved.numel() != flat.numel() or saved.dtype != flat.dtype:
                    raise ValueError(f"{self._who}.load_train_state: group {gi}'s accumulators hold {flat.numel()} fp32 values here, "
                                     f"{saved.numel()} {saved.dtype} in the saved state")
                flat.copy_(saved.reshape(-1))

    def state_dict(self):
        """torch's layout; with step control on, one more top-level entry carries the schedule count and the skipped count, so that a
        resumed run continues the curve (a host synchronisation).  Without step control: exactly torch's dict.  The averages travel
        as ``state[...]["ema"]``; with averaging off in every group the groups carry no ``ema_decay`` key."""
        sd = super().state_dict()
        if not self.ema_enabled:
            sd["param_groups"] = [{k: v for k, v in g.items() if k != "ema_decay"} for g in sd["param_groups"]]
        if self.step_control:
            c = self._read_ctl()
            sd["step_control"] = dict(schedule_step=c["sched_step"], skipped_steps=c["skipped"])
            if self.accumulate_steps is not None:
                sd["step_control"]["micro_step"] = c["micro"]
        return sd

    # -- weight averaging ---------------------------------------------------------------------------------------------------------
    @property
    def ema_enabled(self):
        return any(g.get("ema_decay") is not None for g in self.param_groups)

    def _averaged(self, p, group):
        return group.get("ema_decay") is not None and id(p) not in self._ema_exclude

    def _init_state(self, p, group):
        """moments and (in an averaged group) the average of one parameter, created together; the average alone where a loaded state
        came without one.  Never under a graph capture: the new addresses change the table key, and _table refuses there."""
        st = self.state[p]
        self._init_rule_state(p, group, st)
        if "ema" not in st and self._averaged(p, group):
            st["ema"] = p.detach().clone(memory_format=torch.contiguous_format)   # a bit copy: e_0 = p_0

    def _ema_pairs(self):
        """(parameter, average) of every averaged parameter, in parameter order (state created where a parameter has none yet)"""
        pairs = []
        for group in self.param_groups:
            for p in group["params"]:
                if self._averaged(p, group) and p.is_cuda:
                    self._init_state(p, group)
                    pairs.append((p, self.state[p]["ema"]))
        return pairs

    def ema_parameters(self):
        """the averages, in parameter order (the tensors themselves, not copies)"""
        return [e for _, e in self._ema_pairs()]

    def ema_state_dict(self, model):
        """``model.state_dict()`` with every averaged parameter replaced by a clone of its average; buffers (the permutation tables,
        signs, indices: they are not parameters and not averaged) and parameters that are not averaged are the model's own.  Loads
        with strict=True into a fresh model.  Inside ema_weights() the two are exchanged and this returns the live weights."""
        ema = {id(p): e for p, e in self._ema_pairs()}
        sd = model.state_dict()
        for name, p in model.named_parameters(remove_duplicate=False):
            if id(p) in ema and name in sd:
                sd[name] = ema[id(p)].detach().clone()
        return sd

    def _exchange(self, ps, es):
        with torch.no_grad():
            tmp = [torch.empty_like(p) for p in ps]
            torch._foreach_copy_(tmp, ps)
            torch._foreach_copy_(ps, es)
            torch._foreach_copy_(es, tmp)
        hip_ops.invalidate_weight_shadows()

    @contextlib.contextmanager
    def ema_weights(self):
        """``with optimizer.ema_weights(): validate(model)``: the CONTENTS of every averaged parameter and its average are exchanged in
        place and exchanged back on exit (an exception included), bit for bit.  No address changes, so captured graphs, GradReducer
        buckets and the pointer tables stay valid; the cached compute-dtype weight copies are invalidated both times.  step() inside
        the context raises, and so does nesting.  Three _foreach_copy_ through a temporary: meant for once an epoch."""
        if self._ema_swapped:
            raise RuntimeError(f"{self._who}.ema_weights() does not nest: the parameters already hold the averaged weights")
        if not self.ema_enabled:
            raise RuntimeError(f"{self._who}.ema_weights(): built without ema_decay: there is no average")
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{self._who}.ema_weights() cannot run inside a graph capture")
        pairs = self._ema_pairs()
        ps, es = [p.detach() for p, _ in pairs], [e for _, e in pairs]   # (detach: p's version counter moves with the copy)
        self._exchange(ps, es)
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._exchange(ps, es)
            self._ema_swapped = False

    # -- step control -------------------------------------------------------------------------------------------------------------
    def _read_ctl(self):
        """the control block as the last step() left it (synchronises the host: meant for once an epoch)"""
        if not self.step_control:
            raise RuntimeError(f"{self._who}: built without schedule / max_grad_norm / skip_nonfinite / accumulate_steps: there is no "
                               "step-control block")
        return dict(zip(_CTL_FIELDS, struct.unpack(_CTL_FMT, self.control_block_bytes())))

    def last_lr(self, _ctl=None):
        """the rate the last step() used, one float per parameter group: float32(a * lr + b), the kernel's own expression (under
        accumulation: the last boundary's)"""
        c = _ctl or self._read_ctl()
        return [float(np.float32(np.float64(c["a"]) * np.float64(float(g["lr"])) + np.float64(c["b"]))) for g in self.param_groups]

    def last_grad_norm(self):
        """the L2 norm over all gradients that the last step() saw (before clipping); under accumulation the norm of the last
        boundary's MEAN gradient, accumulator / accumulate_steps"""
        return self._read_ctl()["grad_norm"]

    def skipped_steps(self):
        return self._read_ctl()["skipped"]

    def schedule_step(self):
        """step() calls so far, skipped ones included: the schedule's t of the next step (under accumulation: windows closed so far,
        dropped ones included -- one tick per window)"""
        return self._read_ctl()["sched_step"]

    def control_block_bytes(self):
        """the 64 raw bytes of the control block: the device's, or (before the first step) the ones it will start from"""
        if self._ctl is None:
            return self._ctl_raw or struct.pack(_CTL_FMT, 1.0, 0.0, 1.0, 1, 0.0, *self._ctl_counts, 0)
        return self._ctl.cpu().numpy().tobytes()

    def _control_workspace(self, active):
        """control block, partial-sum workspace and step-pointer array for the groups that step this call; rebuilt (never under capture)
        when a group's chunk count or step tensor changed"""
        key = tuple((t["nchunks"], t["step"].data_ptr()) for _, t in active)
        ws = self._ctl_ws
        if ws is not None and ws["key"] == key and self._ctl is not None:
            return ws
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{self._who}: the step-control workspace has to be (re)built while a HIP graph is being captured: run a "
                               "warm-up step() before the capture")
        dev = active[0][1]["step"].device
        if self._ctl is None:
            self._ctl = torch.frombuffer(bytearray(self.control_block_bytes()), dtype=torch.uint8).to(dev)
        offs, n = [], 0
        for _, t in active:
            offs.append(n)
            n += t["nchunks"]
        ws = dict(key=key, offs=offs, n=n, partials=torch.zeros(max(n, 1), dtype=torch.float64, device=dev),
                  step_ptrs=torch.tensor([t["step"].data_ptr() for _, t in active], dtype=torch.int64).to(dev))
        self._ctl_ws = ws
        return ws

    def _step_controlled(self, active):
        ws = self._control_workspace(active)
        st = _stream()
        k = self.accumulate_steps
        for (_, t), off in zip(active, ws["offs"]):
            if k is not None:   # acc (+)= g and the NEW accumulator's sum of squares in one walk
                _native.call("spv_grad_accumulate", t["table"].data_ptr(), t["acc_table"].data_ptr(), t["chunk_tensor"].data_ptr(),
                             t["chunk_off"].data_ptr(), t["sizes"].data_ptr(), t["nchunks"], self._ctl.data_ptr(),
                             ws["partials"].data_ptr() + 8 * off, st)
                continue
            _native.call("spv_grad_sumsq", t["table"].data_ptr(), t["chunk_tensor"].data_ptr(), t["chunk_off"].data_ptr(),
                         t["sizes"].data_ptr(), t["nchunks"], ws["partials"].data_ptr() + 8 * off, st)
        sch = self.schedule
        flags = ((_CTL_SCHEDULE if sch is not None else 0) | (_CTL_CLIP if self.max_grad_norm is not None else 0)
                 | (_CTL_SKIP if self.skip_nonfinite else 0))
        # (this launch also advances the groups' Adam step counts -- when the step is applied)
        ctl_args = (ws["partials"].data_ptr(), ws["n"], ws["step_ptrs"].data_ptr(), len(active), self._ctl.data_ptr(), flags,
                    sch.warmup_steps if sch else 0, sch.total_steps if sch else 0, sch.eta_min if sch else 0.0, self.max_grad_norm or 0.0)
        if k is not None:   # inside a window: apply = 0 and the count; at its boundary: the block from the mean gradient's norm
            _native.call("spv_step_control_accum", *ctl_args, k, st)
        else:
            _native.call("spv_step_control", *ctl_args, st)
        for group, t in active:
            self._launch_ctl(group, t, t["table" if k is None else "table_acc"], st)   # accumulation: the g column holds the accumulators

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._ema_swapped:
            raise RuntimeError(f"{self._who}.step() inside ema_weights(): the parameters hold the averaged weights")
        active = []   # step control: (group, table) of every group that steps, launched together below
        for gi, group in enumerate(self.param_groups):
            t = self._tables.get(gi)
            if (t is not None and t.get("static")
                    and t["grad_ptrs"] == tuple(0 if p.grad is None else p.grad.data_ptr() for p in group["params"])):
                # fixed gradient addresses (GradReducer(always=True) / a captured graph), verified: nothing to look up
                t["calls"] += 1
            else:
                ps = [p for p in group["params"] if p.grad is not None]
                if not ps:
                    continue
                for p in ps:
                    if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                        raise RuntimeError(f"{self._who}: parameters must be contiguous fp32 tensors on the GPU (no CPU fallback)")
                    self._init_state(p, group)
                had = t is not None
                old_key = t["key"] if had else None
                t = self._table(gi, ps)
                if "step" not in t:  # ONE step counter per group, shared by its parameters' state entries
                    prev = next((self.state[p]["step"] for p in ps if self.state[p].get("step") is not None), None)
                    dev = ps[0].device if group["capturable"] else "cpu"
                    t["step"] = prev.to(dev).clone() if prev is not None else torch.zeros((), dtype=torch.float32, device=dev)
                    t["host_step"] = int(float(t["step"]))
                for p in ps:
                    self.state[p]["step"] = t["step"]
                # static once the same table has served two consecutive look-ups
                t["static"] = self.static_grads and had and old_key == t["key"]
                # what the fast path compares every step: the gradient address of EVERY parameter of the group (0 = no gradient)
                t["grad_ptrs"] = tuple(0 if p.grad is None else p.grad.data_ptr() for p in group["params"])
                t["calls"] = 1
            if self.step_control:
                if not group["capturable"]:
                    raise ValueError(f"{self._who}: step control needs capturable=True in every parameter group")
                active.append((group, t))
                continue
            if group["capturable"]:
                t["step"] += 1.0
                step_ptr = t["step"].data_ptr()
            else:
                t["host_step"] += 1
                t["step"].fill_(float(t["host_step"]))
                step_ptr = 0
            self._launch(group, t, step_ptr)
        if active:
            self._step_controlled(active)
        return loss


class _AdamFamily(_FusedOptimizer):
    """torch.optim.AdamW's and torch.optim.Adam's shared side: the constructor, the state (``step`` / ``exp_avg`` / ``exp_avg_sq``) and
    the launches, which differ in the entry points' prefix only (include/spv.h: spv_adamw_multi* / spv_adam_multi*)."""
    _KERNEL = None

    def _init_rule_state(self, p, group, st):
        if "exp_avg" not in st:
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st.setdefault("step", None)

    def _rule_columns(self, p, group):
        st = self.state[p]
        return st["exp_avg"], st["exp_avg_sq"]

    def _launch(self, group, t, step_ptr):
        b1, b2 = group["betas"]
        bc1 = bc2 = 0.0
        if not step_ptr:
            bc1, bc2 = 1.0 - b1 ** t["host_step"], 1.0 - b2 ** t["host_step"]
        args = (t["table"].data_ptr(), t["chunk_tensor"].data_ptr(), t["chunk_off"].data_ptr(), t["sizes"].data_ptr(), t["nchunks"],
                float(group["lr"]), float(b1), float(b2), 1.0 - b1, 1.0 - b2, float(group["eps"]), float(group["weight_decay"]),
                bc1, bc2, step_ptr)
        if "ema_table" in t:   # (the host's count is read only without a device-side one)
            _native.call(self._KERNEL + "_ema", *args, t["ema_table"].data_ptr(), 1.0 - group["ema_decay"], int(self.ema_warmup),
                         float(t["host_step"]), _stream())
        else:
            _native.call(self._KERNEL, *args, _stream())

    def _launch_ctl(self, group, t, table, st):
        b1, b2 = group["betas"]
        args = (table.data_ptr(), t["chunk_tensor"].data_ptr(), t["chunk_off"].data_ptr(), t["sizes"].data_ptr(), t["nchunks"],
                float(group["lr"]), float(b1), float(b2), 1.0 - b1, 1.0 - b2, float(group["eps"]), float(group["weight_decay"]),
                t["step"].data_ptr(), self._ctl.data_ptr())
        if "ema_table" in t:
            _native.call(self._KERNEL + "_ctl_ema", *args, t["ema_table"].data_ptr(), 1.0 - group["ema_decay"], int(self.ema_warmup), st)
        else:
            _native.call(self._KERNEL + "_ctl", *args, st)


class FusedAdamW(_AdamFamily):
    _KERNEL = "spv_adamw_multi"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, capturable=False, static_grads=False,
                 schedule=None, max_grad_norm=None, skip_nonfinite=False, ema_decay=None, ema_warmup=False, ema_exclude=None,
                 accumulate_steps=None):
        """static_grads=True: the caller expects fixed gradient addresses (spectre_vit.dp.GradReducer(model, always=True), or a
        captured graph): after two identical look-ups a step only COMPARES the gradient addresses with the table's (one tuple of
        ``p.grad.data_ptr()`` per group, every step: a caller that swapped a ``.grad`` gets a rebuilt table, never a write through a
        stale pointer) and skips the state walk and the table build -- 0.3 ms of host time per step otherwise.

        Any of schedule / max_grad_norm / skip_nonfinite switches step() to the on-device control path (needs capturable=True):
          schedule        a CosineSchedule: a group's rate is the schedule of its ``lr`` (the base rate) at t = step() calls so far.
                          None: the group's ``lr``, read from param_groups on every eager call (a captured graph keeps the value).
          max_grad_norm   the update uses g * min(1, max_grad_norm / (norm + 1e-6)), norm = the L2 norm over every gradient of every
                          group, as torch.nn.utils.clip_grad_norm_ -- but ``p.grad`` is NOT rewritten (the scale is applied in the
                          optimizer kernel's registers); read the norm with last_grad_norm().
          skip_nonfinite  a step whose gradients hold an inf or a NaN changes no parameter, no moment and not the Adam step count
                          (GradScaler.step()'s rule); skipped_steps() counts them and the schedule count still advances.
        Without skip_nonfinite a non-finite norm under clipping acts as torch's does (NaN weights).

        ema_decay=d in [0, 1): every parameter gets an fp32 average ``state[p]["ema"]``, updated inside the optimizer launch:
        e' = fmaf(w_t, p' - e, e) with w_t = ema_weight_at(Adam step count, d, ema_warmup) -- torch's ``e.lerp_(p', 1 - d)``.  A group
        default: a parameter group's own ``ema_decay`` overrides it, None = that group is not averaged.  Works with and without
        capturable, step control and static_grads; a step dropped by skip_nonfinite does not move the average.
          ema_warmup      w_t = max(1 - d, 9 / (10 + step)) (timm ModelEmaV2's warm-up); under capturable the count is read on the
                          device, so a replayed graph follows it.
          ema_exclude     parameters that are never averaged although their group is (no ``"ema"`` state; ema_state_dict() takes the
                          live values).
        The average starts as a bit copy of p, made together with the moments at the first step() (or the first ema_parameters() /
        ema_weights() / ema_state_dict()), so e_1 = p_0 + w_1 (p_1 - p_0).  state_dict() carries ``"ema"`` with the moments and a
        resumed run continues the average bit for bit; loading a state that has no ``"ema"`` entries (a torch.optim.AdamW
        checkpoint, or one saved with averaging off) keeps this optimizer's ema_decay and starts the average from the current
        parameters at the next step().  With averaging off in every group state_dict() is exactly what it was without the feature.

        accumulate_steps=k (an int >= 1; None = off; needs capturable=True and switches the control path on): every step() call is a
        MICRO-step, a window is k consecutive micro-steps, and a device counter ``micro`` holds the micro-steps already in the open
        window.  A micro-step adds every gradient to an fp32 accumulator (micro == 0: acc = g, an assignment that does not read the old
        contents; otherwise acc = fp32(acc + g)).  Inside the window (micro < k - 1 on entry) nothing else happens: no parameter, moment,
        average, Adam step count or schedule count moves, and last_lr() / last_grad_norm() / schedule_step() keep describing the last
        boundary.  The k-th micro-step is the boundary: the norm is that of the MEAN gradient acc / k (last_grad_norm()), the schedule
        is read at t = schedule_step() and ticks once per window, clipping acts on the mean, AdamW applies acc * (clip / k), and
        skip_nonfinite drops the whole window (skipped_steps() += 1) when any of its micro-steps held an inf or a NaN.  ``p.grad`` is never
        rewritten (it holds the last micro-batch's gradient); with a per-micro-batch mean loss, acc / k is the mean over the window.
        k = 1 is bit for bit the control path without the option.  The accumulators (one fp32 allocation per parameter group, read
        with accumulated_grads()) do not travel in state_dict(): it carries ``micro_step`` beside the other counters, and
        load_state_dict() restarts the window at micro = 0, warning when the saved window was open."""
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"{self._who}: invalid hyper-parameters lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), capturable=capturable,
                         static_grads=static_grads, schedule=schedule, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite,
                         ema_decay=ema_decay, ema_warmup=ema_warmup, ema_exclude=ema_exclude, accumulate_steps=accumulate_steps)


class FusedAdam(_AdamFamily):
    """``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` (amsgrad / maximize off) -- the reference script's other Adam line
    (spectre_vit/repl/train.py:197, :307) -- on FusedAdamW's launches: the decay joins the gradient (d = g + weight_decay * p) where
    AdamW's multiplies the weight.  torch's state layout, which is FusedAdamW's; every keyword means what it means there
    (FusedAdamW.__init__).  With weight_decay=0 the two classes give the same bits."""
    _KERNEL = "spv_adam_multi"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable=False, static_grads=False,
                 schedule=None, max_grad_norm=None, skip_nonfinite=False, ema_decay=None, ema_warmup=False, ema_exclude=None,
                 accumulate_steps=None):
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"{self._who}: invalid hyper-parameters lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), capturable=capturable,
                         static_grads=static_grads, schedule=schedule, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite,
                         ema_decay=ema_decay, ema_warmup=ema_warmup, ema_exclude=ema_exclude, accumulate_steps=accumulate_steps)


class FusedSGD(_FusedOptimizer):
    """``torch.optim.SGD(params, lr, momentum, dampening, weight_decay, nesterov)`` (maximize off) -- the reference script's SGD line
    (spectre_vit/repl/train.py:198: ``momentum=0.9, nesterov=True``) -- on one launch per step, with FusedAdamW's control path, moving
    average and accumulation (the keywords of FusedAdamW.__init__, unchanged in meaning).  The kernel rounds every operation of
    torch's rule separately in fp32 (include/spv.h: spv_sgd_multi), the same on its vector and its scalar walk.

    State: ``state[p]["momentum_buffer"]`` as torch's (none with momentum=0), and the group's count of applied steps as
    ``state[p]["step"]``, which torch.optim.SGD ignores -- so state_dict() loads into torch.optim.SGD and back.  The count is what
    tells the first applied step, where torch clones the gradient into the buffer (buf = d, untouched by dampening); a step dropped
    by skip_nonfinite does not move it, so the step after a dropped first step is still the first.  It is one count per parameter
    GROUP: a parameter whose gradient first appears after its group has stepped starts from a zero buffer, which differs from torch's
    clone only with dampening != 0.  A loaded state that has momentum buffers but no ``step`` (a torch.optim.SGD checkpoint) starts
    the count at 1: the loaded buffers are used, not overwritten.  dampening is held to [0, 1)."""

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, capturable=False,
                 static_grads=False, schedule=None, max_grad_norm=None, skip_nonfinite=False, ema_decay=None, ema_warmup=False,
                 ema_exclude=None, accumulate_steps=None):
        if lr < 0.0 or weight_decay < 0.0 or not 0.0 <= momentum < 1.0 or not 0.0 <= dampening < 1.0:
            raise ValueError(f"{self._who}: invalid hyper-parameters lr={lr} momentum={momentum} dampening={dampening} "
                             f"weight_decay={weight_decay}")
        if nesterov and (momentum <= 0.0 or dampening != 0.0):
            raise ValueError(f"{self._who}: Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=bool(nesterov)),
                         capturable=capturable, static_grads=static_grads, schedule=schedule, max_grad_norm=max_grad_norm,
                         skip_nonfinite=skip_nonfinite, ema_decay=ema_decay, ema_warmup=ema_warmup, ema_exclude=ema_exclude,
                         accumulate_steps=accumulate_steps)
        for g in self.param_groups:   # a group's own values
            if not 0.0 <= g["momentum"] < 1.0 or not 0.0 <= g["dampening"] < 1.0 or g["weight_decay"] < 0.0 or g["lr"] < 0.0:
                raise ValueError(f"{self._who}: invalid hyper-parameters in a parameter group: lr={g['lr']} momentum={g['momentum']} "
                                 f"dampening={g['dampening']} weight_decay={g['weight_decay']}")
            if g["nesterov"] and (g["momentum"] <= 0.0 or g["dampening"] != 0.0):
                raise ValueError(f"{self._who}: Nesterov momentum requires a momentum and zero dampening")

    def _init_rule_state(self, p, group, st):
        if group["momentum"] != 0.0:
            if st.get("momentum_buffer") is None:
                st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            elif st.get("step") is None:   # buffers that came without a count (torch.optim.SGD's): they have been through a step
                st["step"] = torch.ones((), dtype=torch.float32)
        st.setdefault("step", None)

    def _rule_columns(self, p, group):
        return (self.state[p]["momentum_buffer"] if group["momentum"] != 0.0 else None), None

    def _rule_args(self, group):
        return (float(group["momentum"]), 1.0 - float(group["dampening"]), float(group["weight_decay"]), int(bool(group["nesterov"])))

    def _launch(self, group, t, step_ptr):
        args = (t["table"].data_ptr(), t["chunk_tensor"].data_ptr(), t["chunk_off"].data_ptr(), t["sizes"].data_ptr(), t["nchunks"],
                float(group["lr"]), *self._rule_args(group), float(t["host_step"]), step_ptr)
        if "ema_table" in t:
            _native.call("spv_sgd_multi_ema", *args, t["ema_table"].data_ptr(), 1.0 - group["ema_decay"], int(self.ema_warmup), _stream())
        else:
            _native.call("spv_sgd_multi", *args, _stream())

    def _launch_ctl(self, group, t, table, st):
        args = (table.data_ptr(), t["chunk_tensor"].data_ptr(), t["chunk_off"].data_ptr(), t["sizes"].data_ptr(), t["nchunks"],
                float(group["lr"]), *self._rule_args(group), t["step"].data_ptr(), self._ctl.data_ptr())
        if "ema_table" in t:
            _native.call("spv_sgd_multi_ctl_ema", *args, t["ema_table"].data_ptr(), 1.0 - group["ema_decay"], int(self.ema_warmup), st)
        else:
            _native.call("spv_sgd_multi_ctl", *args, st)
