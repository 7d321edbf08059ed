"""The training step replayed from HIP graphs (MI355X: ~70 kernel launches per 1.6 ms step leave an eager host behind the GPU;
a replay costs the host ~15 us).

    step = GraphedTrainStep(model, optimizer, criterion, example_img, example_labels, autocast_dtype=torch.bfloat16)
    loss = step(img, labels)        # copies the batch into the captured buffers, replays, returns the (device) loss

What is captured: zero_grad -> forward (autocast) -> loss -> backward -> optimizer.step(), i.e. reference
spectre_vit/repl/train.py:216-238 minus the host-side bookkeeping.  Requirements:
  * the optimizer must keep its step count on the device: ``spectre_vit.optim.FusedAdamW(capturable=True)`` or
    ``torch.optim.AdamW(fused=True, capturable=True)``;
  * learning-rate schedule, gradient clipping, non-finite skip: by-value kernel arguments are frozen at capture, so a rate set through
    ``param_groups`` between replays has no effect -- ``FusedAdamW(schedule=..., max_grad_norm=..., skip_nonfinite=...)`` decides all
    three on the device inside ``optimizer.step()``, which is what every step class here captures (``GraphedDPStep``: in graph B,
    behind the all-reduce, so every rank decides alike);
  * gradient accumulation: ``FusedAdamW(accumulate_steps=k)`` -- each replay is one micro-step, the device counts them and every
    k-th replay applies the optimizer; the graph is the same for all of them and nothing here changes.  The warm-up steps are real
    MICRO-steps: ``warmup`` a multiple of k keeps the first replay at the start of a window (any other value is valid too: the window
    is then open when the replays begin, ``optimizer.micro_step()`` tells where).  A ``GraphedDPStep`` rank all-reduces every
    micro-step, which is correct because the exchange is linear;
  * dropout: seeds are by-value kernel arguments frozen at capture, so every dropout kernel adds a 64-bit device word that this
    class advances once per replay (a role of ``spv_step_prologue``, the first node of the graph) -- fresh masks every step;
  * fixed shapes (one graph per batch shape).

``loader=`` (a ``spectre_vit.data.ResidentLoader`` with an image output) puts the batch inside the graph as well: the step's image and
label buffers ARE the loader's, ``loader.fetch()`` is the graph's first node -- in front of ``hip_ops.step_prologue``, whose patch-row
role reads the image buffer -- and a step is one replay with no host-issued work in front of it:

    step = GraphedTrainStep(model, optimizer, criterion, None, None, loader=loader)
    loss = step()                   # step.img / step.labels: the batch that replay trained on

The warm-up steps are real steps and each consumes one loader step; the capture consumes none (a recorded launch does not run).

``GraphedTrainStep`` is the single-process form: ONE graph.  ``GraphedDPStep`` is a data-parallel rank (the reference is single
device, train.py:41; SURVEY 8e makes the gradient exchange new work):

    graph A   seed word, zero_grad, forward, loss, backward -- with the layer weight gradients held back and computed by one batched
              launch, exactly as in the single-process graph -- every gradient written into the reducer's flat buffer
    host      ONE all-reduce over that buffer (torch.distributed: RCCL over xGMI; 13 MB for the FFT model)
    graph B   the optimizer step

so a rank's host issues two replays and one collective per step instead of ~70 launches, and the eager path's three handicaps
(host issue time above the GPU time, weight gradients one by one, no side stream) are gone.  The collective is NOT captured: RCCL
inside a graph has not run on a multi-GPU box in this project, and the exchange is one call either way.
"""
from __future__ import annotations

import contextlib
import weakref

import torch

from spectre_vit import _native, hip_ops, shadows
from spectre_vit.dp import GradReducer

_seed_owner = None   # weakref to the live step object whose seed word the library's dropout kernels read


def _claim_seed_word(obj):
    global _seed_owner
    cur = _seed_owner() if _seed_owner is not None else None
    if cur is not None and cur is not obj and not cur._closed:
        raise RuntimeError("a graph-replayed training step is already live in this process: the dropout seed word is one device "
                           "symbol of libspv_hip.so, so two live steps would share (or steal) each other's masks -- call .close() "
                           "on the old step first")
    _native.call("spv_set_seed_device_ptr", obj.seed_word.data_ptr())
    _seed_owner = weakref.ref(obj)


def _release_seed_word(obj):
    """eager kernels after this object's life must not read its seed word; only the CURRENT owner may clear the pointer (an old
    step's __del__ running after a new step registered its word must leave the new word in place)"""
    global _seed_owner
    cur = _seed_owner() if _seed_owner is not None else None
    if cur is obj or cur is None:
        if _seed_owner is not None:
            _native.call("spv_set_seed_device_ptr", 0)
        _seed_owner = None


def _check_loader(name, loader, example_img, example_labels):
    """the refusals of every loader-fed step, raised before a device is touched"""
    if loader.img is None:
        raise ValueError(f"{name}(loader=...): the loader has no image output (output='none'); fetch eagerly, "
                         "build the images from loader.index and feed the step instead")
    if example_img is not None or example_labels is not None:
        raise ValueError(f"{name}(loader=...): the batch comes from the loader, pass example_img = example_labels = None")


class GraphedTrainStep:
    _dp = False

    def __init__(self, model, optimizer, criterion, example_img, example_labels, autocast_dtype=torch.bfloat16, warmup=3,
                 return_features=False, process_group=None, force_collective=False, loader=None, seed_word=0, capture_rng_state=None):
        """seed_word: the dropout seed word's initial value (a resumed run passes the saved word, so that its warm-up step draws the
        masks the uninterrupted run's next replay draws).  capture_rng_state: torch's CPU generator state an earlier step object of
        the same run was captured under (its ``capture_rng_state`` attribute): the by-value dropout seeds are drawn from that
        generator and frozen in the graph, so a resumed run sets it in front of its warm-up step AND in front of its capture --
        both then draw the seeds the interrupted run's graph holds (exact with warmup=1, the harness's value)."""
        if loader is not None:
            _check_loader(type(self).__name__, loader, example_img, example_labels)
        elif not example_img.is_cuda:
            raise RuntimeError(f"{type(self).__name__} needs the example batch on the GPU")
        for g in optimizer.param_groups:
            if not g.get("capturable", False):
                raise ValueError(f"{type(self).__name__}: build the optimizer with capturable=True (its step count must live on the device)")
        self._closed = True   # until the seed word is claimed
        self.model, self.optimizer, self.criterion = model, optimizer, criterion
        self.autocast_dtype = autocast_dtype
        self.loader = loader
        if loader is None:
            self.img = example_img.clone()
            self.labels = example_labels.clone()
        else:   # the loader's fixed-address buffers are the step's
            self.img, self.labels = loader.img, loader.labels
        dev = self.img.device
        self.force_collective = bool(force_collective)
        # fixed gradient addresses (the graphs replay into them; the optimizer's pointer table is built once, before the capture).
        # A rank of a data-parallel job exchanges them with one call between its two graphs: no hook launches anything.
        self.reducer = GradReducer(model, always=True, process_group=process_group, overlap=not self._dp)
        if not self._dp and self.reducer.world > 1:
            raise RuntimeError("GraphedTrainStep is the single-process step; a rank of a torch.distributed job uses GraphedDPStep")
        seed_word = int(seed_word) & (2 ** 64 - 1)
        self.seed_word = torch.zeros(1, dtype=torch.int64, device=dev)
        if seed_word:   # (0: the launches of a step built without the keyword)
            self.seed_word.copy_(torch.tensor([seed_word if seed_word < 2 ** 63 else seed_word - 2 ** 64], dtype=torch.int64))
        self._resume_rng = capture_rng_state
        self.capture_rng_state = None
        _claim_seed_word(self)
        self._closed = False
        self._one = torch.ones((), dtype=torch.float32, device=dev)
        self.replays = 0
        try:
            self._build(max(1, warmup))
        except BaseException:
            self.close()
            raise

    @property
    def fetch_in_graph(self):
        """the loader's fetch is a node of the captured step (a replay is then counted as one fetch)"""
        return self.loader is not None

    # -- the two halves of a step -----------------------------------------------------------------------------------------------
    def _forward_backward(self):
        if self.fetch_in_graph:
            self.loader.fetch()   # the first node: this step's batch into self.img / self.labels, the device cursor moved on
        # ONE launch: the seed word's advance and whatever else of the forward's opening depends on nothing but the parameters and
        # the image buffer (hip_ops.step_prologue); the nodes concerned pick their results up instead of launching
        hip_ops.step_prologue(self.model, self.img, self.seed_word, self.autocast_dtype)
        self.reducer.zero_grad()
        with torch.autocast("cuda", dtype=self.autocast_dtype, enabled=self.autocast_dtype is not None):
            out = self.model(self.img)
        loss = self.criterion(out, self.labels)
        loss.backward(self._one)   # a kept 1.0 (backward() alone fills a fresh one: a launch per step)
        return loss, out

    def _eager_step(self):
        loss, out = self._forward_backward()
        self.reducer.finish()
        self.optimizer.step()
        return loss, out

    @contextlib.contextmanager
    def _hold(self):
        """while this object's backward passes run: layer weight gradients and folds may be held for the batched launch even in a
        multi-rank job (nothing is exchanged before the pass ends)"""
        prev = hip_ops.HOLD_UNDER_DP
        hip_ops.HOLD_UNDER_DP = prev or self._dp
        try:
            yield
        finally:
            hip_ops.HOLD_UNDER_DP = prev

    def _set_capture_rng(self):
        """in front of the capture (and, resumed, of the warm-up): the generator state the graph's by-value seeds are drawn under"""
        if self._resume_rng is not None:
            torch.set_rng_state(self._resume_rng)

    def _warm(self, warmup):
        # warm-up on a side stream (allocator pools, lazily built tables, optimizer state), then capture
        self._set_capture_rng()
        side = torch.cuda.Stream(device=self.img.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), self._hold():
            for _ in range(warmup):
                loss, out = self._eager_step()
        torch.cuda.current_stream().wait_stream(side)
        # the warm-up steps are REAL training steps on the example batch: a caller that feeds the example batch as its first batch
        # takes the last one's results from here instead of replaying that batch a second time
        self.warm_loss, self.warm_out = loss.detach(), out.detach()
        shadows.reset_shadow_cache()  # the weight casts must be recorded in the graph, not served from a cache
        self._set_capture_rng()
        self.capture_rng_state = torch.get_rng_state()   # what a checkpoint keeps of this capture (a host read of a host generator)

    def _build(self, warmup):
        self._warm(warmup)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), self._hold():
            self.loss, self.out = self._eager_step()

    def _replay(self):
        self.graph.replay()

    def __call__(self, img=None, labels=None):
        if self._closed:
            raise RuntimeError("this graph-replayed step was closed")
        if self.loader is not None and (img is not None or labels is not None):
            raise ValueError("this step fetches its own batch (loader=...): call it without arguments")
        if img is not None:
            self.img.copy_(img, non_blocking=True)
        if labels is not None:
            self.labels.copy_(labels, non_blocking=True)
        self._replay()
        self.replays += 1
        if self.fetch_in_graph:
            self.loader.count_replay()
        # the replay updated the weights through raw pointers: neither the parameters' version counters nor the optimizer's post-step
        # hook saw it, so the inference-time cache of bf16 weight copies (shadows._ShadowCache) must be told
        shadows.invalidate_weight_shadows()
        return self.loss

    def close(self):
        if not self._closed:
            self._closed = True
            _release_seed_word(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GraphedDPStep(GraphedTrainStep):
    """One rank of the data-parallel step: graph A (forward + loss + backward, batched weight gradients) -> one all-reduce of the flat
    gradient buffer (mean over ranks) -> graph B (optimizer).  Build it AFTER ``torch.distributed.init_process_group`` and after the
    rank-0 weights / buffers were broadcast (``spectre_vit.dp.broadcast_module``); every rank must construct it (the warm-up steps
    contain the collective).  In a single process it runs the same launch sequence with the collective skipped
    (``force_collective=True``: issued in the one-rank group, when one is initialised)."""
    _dp = True

    def _eager_step(self):
        loss, out = self._forward_backward()
        self.reducer.allreduce_flat(force=self.force_collective)
        self.optimizer.step()
        return loss, out

    def _build(self, warmup):
        self._warm(warmup)
        torch.cuda.synchronize()   # the warm-up's collectives are complete before a capture begins
        pool = torch.cuda.graph_pool_handle()
        # capture_error_mode "thread_local": only THIS thread's calls are checked against the capture.  A process group keeps a
        # watchdog thread that queries its work events at any time; under the default ("global") mode such a query from another
        # thread can invalidate an ongoing capture.  Nothing of the collective is captured here, so thread-local checking is exact.
        mode = dict(capture_error_mode="thread_local")
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, pool=pool, **mode), self._hold():
            self.loss, self.out = self._forward_backward()
        self.graph_opt = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph_opt, pool=pool, **mode):
            self.optimizer.step()

    def _replay(self):
        self.graph.replay()
        self.reducer.allreduce_flat(force=self.force_collective)   # host-issued, on the current stream's order: RCCL over xGMI
        self.graph_opt.replay()


class GraphedDistillStep(GraphedTrainStep):
    """The distillation step of reference train.py:298-361 replayed from one graph: zero_grad, student forward, the fused loss
    (``spectre_vit.distillation.DistillationLoss``), backward, optimizer.  Two forms:

    teacher logits per step -- the loss reads a fixed-address ``teacher_logits`` buffer.  The teacher is NOT captured -- a real backbone
    is arbitrary user code -- it runs eagerly under no_grad in front of the replay, on the step's stream:

        step = GraphedDistillStep(model, optimizer, DistillationLoss(), img, labels, teacher_logits, autocast_dtype=None)
        loss = step(img, labels, teacher_logits)      # step.soft / step.ce / step.out: the other captured outputs

    cached teacher -- the loss reads the resident ``TeacherLogitCache`` through a fixed-address int64 ``index`` buffer the step owns; a
    step is the index copy and the replay, no teacher and no view kernel:

        step = GraphedDistillStep(model, optimizer, DistillationLoss(), img, labels, teacher_cache=cache, example_index=sel)
        loss = step(img, labels, index=sel)

    ``loader=`` (a ``spectre_vit.data.ResidentLoader`` with an image output; pass example_img = example_labels = None and no
    example_index): the step's image and label buffers ARE the loader's.

    cached teacher -- the loss's index buffer IS ``loader.index`` and ``loader.fetch()`` is the graph's first node: a step is one replay,
    with no index copy and no host-issued work in front of it (every warm-up step consumes one loader step, the capture none):

        step = GraphedDistillStep(model, optimizer, DistillationLoss(), None, None, teacher_cache=cache, loader=loader)
        loss = step()                                 # step.img / step.labels / step.index: the batch that replay trained on

    teacher logits per step -- the teacher needs the batch's index BEFORE the replay, so the fetch is NOT captured; the caller fetches,
    runs the view and the teacher on ``loader.index`` and replays a graph that reads the loader's buffers (the first batch is fetched
    before the step is built: its warm-up trains on it):

        loader.fetch()
        step = GraphedDistillStep(model, optimizer, DistillationLoss(), None, None, teacher_logits_of(loader.index), loader=loader)
        loader.fetch(); loss = step(teacher_logits=teacher_logits_of(loader.index))

    A criterion with a non-zero ``feature_loss_weight`` (the feature-matching term): the student's forward returns its features too and
    the feature launch is captured with the rest.  Uncached, the step owns a second fixed-address buffer ``teacher_feat`` beside
    ``teacher_logits`` -- pass ``example_teacher_feat`` and, per step, ``teacher_feat=`` -- filled in front of the replay; cached, the
    term reads ``teacher_cache.features`` (a ``TeacherLogitCache(feature_dim=...)``) through the same index, so the loader-fed cached
    step stays one replay.  ``step.feat`` is the captured unweighted term.

    Single process only: a graph-replayed data-parallel distillation rank is not built."""

    def __init__(self, model, optimizer, criterion, example_img, example_labels, example_teacher_logits=None, autocast_dtype=None, warmup=3,
                 process_group=None, *, teacher_cache=None, example_index=None, loader=None, example_teacher_feat=None, seed_word=0,
                 capture_rng_state=None):
        import torch.distributed as dist
        if loader is not None:
            _check_loader("GraphedDistillStep", loader, example_img, example_labels)
            if example_index is not None:
                raise ValueError("GraphedDistillStep(loader=...): the loss reads the teacher cache through loader.index, pass no example_index")
        if (example_teacher_logits is None) == (teacher_cache is None):
            raise ValueError("GraphedDistillStep takes example_teacher_logits (the teacher runs in front of every replay) or "
                             "teacher_cache (its logits are resident), one of the two")
        if loader is None and (teacher_cache is None) != (example_index is None):
            raise ValueError("GraphedDistillStep: teacher_cache and example_index go together")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(process_group) > 1:
            raise RuntimeError("GraphedDistillStep is the single-process step: GraphedDPStep is not built for distillation "
                               "(run the ranks of a torch.distributed job with the eager step)")
        self.featured = getattr(criterion, "feature_loss_weight", 0.0) != 0.0
        if self.featured and teacher_cache is None and example_teacher_feat is None:
            raise ValueError(f"GraphedDistillStep: the criterion's feature_loss_weight={criterion.feature_loss_weight} needs "
                             "example_teacher_feat beside example_teacher_logits")
        if self.featured and teacher_cache is not None and getattr(teacher_cache, "features", None) is None:
            raise ValueError(f"GraphedDistillStep: the criterion's feature_loss_weight={criterion.feature_loss_weight} needs a teacher "
                             "cache with features (TeacherLogitCache(feature_dim=...))")
        self.teacher_feat = example_teacher_feat.detach().clone() if self.featured and teacher_cache is None else None
        self.teacher_cache = teacher_cache
        if teacher_cache is None:
            self.teacher_logits, self.index = example_teacher_logits.detach().clone(), None
        elif loader is not None:   # the loader's fixed-address index is the loss's
            self.teacher_logits, self.index = None, loader.index
        else:
            if example_index.dtype != torch.int64 or example_index.shape != example_labels.shape[:1]:
                raise ValueError(f"GraphedDistillStep: example_index is an int64 vector of the batch's {example_labels.shape[0]} rows, got "
                                 f"{example_index.dtype} {tuple(example_index.shape)}")
            self.teacher_logits, self.index = None, example_index.detach().clone()
        super().__init__(model, optimizer, criterion, example_img, example_labels, autocast_dtype=autocast_dtype, warmup=warmup,
                         process_group=process_group, loader=loader, seed_word=seed_word, capture_rng_state=capture_rng_state)

    @property
    def fetch_in_graph(self):
        """cache mode only: with a teacher in front of the replay the caller fetches eagerly (the teacher's view needs the index)"""
        return self.loader is not None and self.teacher_cache is not None

    def _forward_backward(self):
        if self.fetch_in_graph:
            self.loader.fetch()   # the first node: this step's batch into self.img / self.labels / self.index
        _native.call("spv_seed_advance", self.seed_word.data_ptr(), torch.cuda.current_stream().cuda_stream)
        self.reducer.zero_grad()
        with torch.autocast("cuda", dtype=self.autocast_dtype, enabled=self.autocast_dtype is not None):
            out = self.model(self.img, return_features=True) if self.featured else self.model(self.img)
        feats = {}
        if self.featured:
            out, student_feat = out
            feats = dict(student_feat=student_feat, teacher_feat=self.teacher_feat if self.index is None else self.teacher_cache.features)
        if self.index is None:
            loss = self.criterion(out, self.teacher_logits, self.labels, **feats)   # on the fp32 logits, outside autocast
        else:
            loss = self.criterion(out, self.teacher_cache, self.labels, index=self.index, **feats)
        loss.backward(self._one)
        return loss, out

    def _warm(self, warmup):
        super()._warm(warmup)
        self.warm_soft, self.warm_ce = self.criterion.soft, self.criterion.ce
        self.warm_feat = self.criterion.feat if self.featured else None

    def _build(self, warmup):
        super()._build(warmup)
        self.soft, self.ce = self.criterion.soft, self.criterion.ce
        self.feat = self.criterion.feat if self.featured else None

    def __call__(self, img=None, labels=None, teacher_logits=None, *, index=None, teacher_feat=None):
        if not self._closed:
            if teacher_feat is not None:
                if self.teacher_feat is None:
                    raise ValueError("this step has no teacher feature buffer: its criterion's feature_loss_weight is 0, or it reads the "
                                     "teacher cache's features through the index")
                self.teacher_feat.copy_(teacher_feat, non_blocking=True)
            if teacher_logits is not None:
                if self.teacher_logits is None:
                    raise ValueError("this step reads the teacher cache: pass index=, not teacher logits")
                self.teacher_logits.copy_(teacher_logits, non_blocking=True)
            if index is not None:
                if self.loader is not None:
                    raise ValueError("this step reads the teacher cache through the loader's index (loader=...): pass no index")
                if self.index is None:
                    raise ValueError("this step takes the teacher's logits per step: it was built without teacher_cache")
                self.index.copy_(index, non_blocking=True)
        return super().__call__(img, labels)
