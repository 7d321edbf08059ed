"""Distillation helpers -- counterpart of reference spectre_vit/distillation.py:5-43 plus the loss of
spectre_vit/repl/train.py:334-348.

``DinoClassifier`` wraps a frozen backbone exposing ``forward_features(x)["x_norm_clstoken"]`` (the DINOv3 contract);
the real teacher weights are not available offline, so ``SyntheticTeacher`` provides the same output
contract with fixed random projections for benchmarks and tests.  The teacher runs under ``no_grad`` in stock PyTorch --
it is outside the accelerated path.

The paired-view step (reference train.py:139-141, 298-361) on the HIP path (csrc/spv_distill.hip):
``TeacherView`` is the teacher's transform -- Resize(256, BICUBIC) -> CenterCrop(224) -> ToTensor -> Normalize of the raw 8-bit
sample (train.py:92-100), Pillow's integer resampling bit for bit -- read from the resident uint8 NHWC set through the batch's index;
``DistillationLoss`` is the soft-target + cross-entropy loss as one launch each way (``hip_ops.distill_loss``).
``TeacherLogitCache`` keeps the frozen teacher's logits of every sample resident on the GPU (the teacher's view has no random op and
the teacher is frozen, so they are a function of the sample index alone): filled once, read by ``DistillationLoss(..., index=...)``.
``DistillationLoss(feature_loss_weight=...)`` adds the cell's feature-matching term (train.py:306, 343-346: 1 - mean cosine of the two
models' CLS features) as one more launch each way; ``TeacherLogitCache(feature_dim=...)`` keeps the teacher's features beside its logits.
"""
import math

import numpy as np
import torch
import torch.nn as nn


class DinoClassifier(nn.Module):
    """backbone.forward_features -> CLS feature -> Linear decoder; ``forward(x, return_features)`` like the student."""

    def __init__(self, backbone, num_classes, embed_dim=384):
        super().__init__()
        self.backbone = backbone
        self.decoder = nn.Sequential(nn.Linear(embed_dim, num_classes))

    def forward(self, x, return_features=False):
        feats = self.backbone.forward_features(x)["x_norm_clstoken"]  # [B, C]
        logits = self.decoder(feats)
        return (logits, feats) if return_features else logits


class DistillationDatasetCls(torch.utils.data.Dataset):
    """Two views of one sample: {"img_teacher", "img_model", "label"} (reference distillation.py:25-43)."""

    def __init__(self, samples, teacher_tf, model_tf):
        self.samples = samples
        self.teacher_tf = teacher_tf
        self.model_tf = model_tf

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, idx):
        img, label = self.samples[idx]
        return {"img_teacher": self.teacher_tf(img), "img_model": self.model_tf(img), "label": label}


class _SyntheticBackbone(nn.Module):
    """fixed random features with the DINOv3 ``forward_features`` dictionary contract"""

    def __init__(self, in_channels, embed_dim, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.register_buffer("proj", torch.randn(in_channels * 64, embed_dim, generator=g) / 8.0)

    def forward_features(self, x):
        pooled = nn.functional.adaptive_avg_pool2d(x, 8).flatten(1)  # [B, C*64]
        return {"x_norm_clstoken": nn.functional.layer_norm(pooled @ self.proj, (self.proj.shape[1],))}


def SyntheticTeacher(num_classes=100, embed_dim=384, in_channels=3, seed=0):
    """stand-in for the frozen DINOv3-S teacher: (B, num_classes) logits and (B, embed_dim) features"""
    t = DinoClassifier(_SyntheticBackbone(in_channels, embed_dim, seed), num_classes, embed_dim)
    for p in t.parameters():
        p.requires_grad_(False)
    return t.eval()


def distillation_loss(student_logits, teacher_logits, labels, T=2.0, soft_target_loss_weight=0.25, ce_loss_weight=0.75):
    """0.25 * T^2 * sum(p_t (log p_t - log p_s)) / B + 0.75 * CE  (reference train.py:300-302, 334-348).
    Returns (loss, soft_targets_loss, ce_loss)."""
    soft_targets = nn.functional.softmax(teacher_logits / T, dim=-1)
    soft_prob = nn.functional.log_softmax(student_logits / T, dim=-1)
    soft = torch.sum(soft_targets * (soft_targets.log() - soft_prob)) / soft_prob.size(0) * (T ** 2)
    if student_logits.is_cuda and student_logits.dtype == torch.float32:
        from . import hip_ops
        ce = hip_ops.cross_entropy(student_logits, labels)  # one launch each way (csrc/spv_head.hip)
    else:
        ce = nn.functional.cross_entropy(student_logits, labels)
    return soft_target_loss_weight * soft + ce_loss_weight * ce, soft, ce


# ---------------------------------------------------------------- the teacher's view (csrc/spv_distill.hip)
PRECISION_BITS = 22   # Pillow's fixed point for 8-bit images: 32 - 8 - 2


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def teacher_view_table(n, resize=256, crop=224):
    """The coefficient table of Resize(resize, BICUBIC) -> CenterCrop(crop) along one axis of an n-pixel source, as Pillow builds it
    for 8-bit images (float64 weights normalised to sum 1, then rounded half away from zero to 22 fractional bits).  Returns
    (xmin int32 [crop], taps int32 [crop, 4]): cropped output j reads source pixels xmin[j] .. xmin[j] + 3.  Only up-scaling is
    supported (n <= resize: Pillow widens the support otherwise), and every cropped output must keep its four taps inside the image."""
    n, resize, crop = int(n), int(resize), int(crop)
    if not (2 <= n <= resize and 0 < crop <= resize):
        raise ValueError(f"teacher view: n={n}, resize={resize}, crop={crop} outside 2 <= n <= resize, 0 < crop <= resize")
    lo = (resize - crop) // 2
    scale = n / resize
    xmin = np.zeros(crop, np.int32)
    taps = np.zeros((crop, 4), np.int32)
    for j in range(crop):
        center = (lo + j + 0.5) * scale
        x0 = max(int(center - 2.0 + 0.5), 0)
        x1 = min(int(center + 2.0 + 0.5), n)
        if x1 - x0 != 4:
            raise ValueError(f"teacher view: output {lo + j} of an n={n} source at resize={resize} has {x1 - x0} taps inside the image; "
                             "the kernel takes exactly 4")
        w = [_bicubic(x + x0 - center + 0.5) for x in range(4)]
        ww = 0.0
        for v in w:
            ww += v
        w = [v / ww for v in w]
        xmin[j] = x0
        taps[j] = [int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5) for v in w]
    return xmin, taps


_tables = {}   # (n, resize, crop, device) -> int32 [5][crop_p] on the device


def _device_table(n, resize, crop, device):
    key = (n, resize, crop, str(device))
    if key not in _tables:
        xmin, taps = teacher_view_table(n, resize, crop)
        crop_p = (crop + 7) // 8 * 8
        packed = np.zeros((5, crop_p), np.int32)
        packed[0, :crop] = xmin
        packed[1:, :crop] = taps.T
        _tables[key] = torch.from_numpy(packed).to(device)
    return _tables[key]


def normalize_lut(mean, std):
    """fp32 [C][256]: ToTensor + Normalize of every 8-bit value, by torch's own fp32 operations on the host, on a (C, 256, 1) "image"
    with the statistics shaped (C, 1, 1) as torchvision shapes them: the table is built by the very expression it stands for, so
    whatever torch's kernels do with a scalar-like operand (a one-channel std is one), the table does too"""
    C = len(mean)
    v = torch.arange(256, dtype=torch.uint8).view(1, 256, 1).expand(C, 256, 1).contiguous().float().div(255)
    m = torch.tensor(mean, dtype=torch.float32).view(-1, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(-1, 1, 1)
    return ((v - m) / s).reshape(C, 256).contiguous()


class TeacherView:
    """The teacher's transform of reference train.py:92-100 on the GPU, for square uint8 sources:

        view = TeacherView(CIFAR_MEAN, CIFAR_STD)                     # resize=256, crop=224
        img_teacher = view(train_u8_nhwc, index)                      # (B, C, 224, 224), float32 or bfloat16

    No autograd: the teacher runs under no_grad."""

    def __init__(self, mean, std, resize=256, crop=224, dtype=torch.float32):
        self.mean = tuple(float(m) for m in mean)
        self.std = tuple(float(s) for s in std)
        if len(self.mean) != len(self.std) or len(self.mean) not in (1, 3):
            raise ValueError(f"mean / std name {len(self.mean)} / {len(self.std)} channels; the teacher view kernel takes 1 or 3")
        if dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"the teacher view is written as float32 or bfloat16, got {dtype}")
        self.resize, self.crop, self.dtype = int(resize), int(crop), dtype
        if not 0 < self.crop <= self.resize:
            raise ValueError(f"teacher view: crop={crop} outside 0 < crop <= resize={resize}")
        self._lut = {}   # device -> fp32 [C][256]

    def lut(self, device):
        key = str(device)
        if key not in self._lut:
            self._lut[key] = normalize_lut(self.mean, self.std).to(device)
        return self._lut[key]

    def __call__(self, images_u8_nhwc, index=None):
        """images_u8_nhwc: the resident uint8 set (N, n, n, C); index: int64 (B,) rows of it (None: all of them)."""
        from spectre_vit import _native
        from spectre_vit.hip_ops import _DT, _p, _require_gpu, _stream
        x = images_u8_nhwc
        if x.dtype != torch.uint8 or x.dim() != 4 or not x.is_contiguous():
            raise TypeError(f"the teacher view kernel takes a contiguous uint8 (N, H, W, C) set, got {x.dtype} {tuple(x.shape)}")
        N, H, W, C = x.shape
        if C != len(self.mean):
            raise ValueError(f"{C}-channel images, but mean / std name {len(self.mean)} channels")
        if index is not None:
            if index.dtype != torch.int64 or index.dim() != 1 or not index.is_contiguous():
                raise TypeError(f"index is a contiguous int64 vector, got {index.dtype} {tuple(index.shape)}")
            batch = index.numel()
        else:
            batch = N
        _require_gpu(x, index)
        if H != W or not _native.call("spv_teacher_view_supported", C, H, self.resize, self.crop):
            raise ValueError(f"a {C} x {H} x {W} source to resize {self.resize}, crop {self.crop} is outside the teacher view kernel "
                             "(square, 1 or 3 channels, n <= resize, four taps inside the image, staging within 64 KiB of LDS)")
        table = _device_table(H, self.resize, self.crop, x.device)
        out = torch.empty((batch, C, self.crop, self.crop), dtype=self.dtype, device=x.device)
        _native.call("spv_teacher_view_u8", _p(x), _p(index), _p(table), _p(self.lut(x.device)), _p(out), batch, N, C, H, self.resize,
                     self.crop, _DT[self.dtype], _stream())
        return out


class DistillationLoss(nn.Module):
    """The loss of reference train.py:300-302, 334-348 on the HIP path (GPU only, like spectre_vit.loss.CrossEntropyLoss): returns the
    weighted loss; ``.soft`` and ``.ce`` hold the unweighted soft-target and cross-entropy terms of the last call (device scalars,
    detached), the reference's "Batch Loss/Dist" and "Batch Loss/CE".
    feature_loss_weight (0.0: off, and then not one launch differs): the feature-matching term of train.py:306, 343-346,
    feat = 1 - mean_r cos(student_feat[r], teacher_feat[r]), one more launch each way (``hip_ops.feature_cosine``); the loss is then
    w_soft * soft + w_ce * ce + w_feat * feat and ``.feat`` holds the unweighted term of the last call.  The two feature matrices must
    have one width: a teacher of another width projects inside its own module (no learned projector here, as in the reference)."""

    def __init__(self, T=2.0, soft_target_loss_weight=0.25, ce_loss_weight=0.75, meter=None, feature_loss_weight=0.0):
        super().__init__()
        if not (T > 0 and math.isfinite(T)):
            raise ValueError(f"temperature T={T} must be positive and finite")
        self.T, self.soft_target_loss_weight, self.ce_loss_weight = float(T), float(soft_target_loss_weight), float(ce_loss_weight)
        self.feature_loss_weight = float(feature_loss_weight)
        if not math.isfinite(self.feature_loss_weight):
            raise ValueError(f"feature_loss_weight={feature_loss_weight!r} must be finite")
        if self.feature_loss_weight != 0.0 and meter is not None:
            raise ValueError(f"feature_loss_weight={self.feature_loss_weight} with a meter ({type(meter).__name__}): the meter's log row "
                             "holds loss, soft and CE and has no slot for a fourth term, so its logged loss would lack the feature term")
        self.soft = self.ce = self.feat = None
        if meter is not None:
            from .meter import TrainMeter
            if not isinstance(meter, TrainMeter):
                raise TypeError(f"meter is a spectre_vit.meter.TrainMeter or None, got {type(meter).__name__}")
        # a TrainMeter: the forward takes the metered launch -- the same bits, the student's hits counted and the step (loss, soft, ce)
        # logged into the meter's device block; None: the un-metered launch, exactly
        self.meter = meter

    def _features(self, student_feat, teacher_feat, teacher_logits, index):
        """the two feature matrices of a call with the term on, checked (ValueErrors name the values) -> (student, teacher)"""
        w = self.feature_loss_weight
        if teacher_feat is None and index is not None and isinstance(teacher_logits, TeacherLogitCache):
            teacher_feat = teacher_logits.features
        if isinstance(teacher_feat, TeacherLogitCache):
            teacher_feat = teacher_feat.features
        if student_feat is None or teacher_feat is None:
            raise ValueError(f"feature_loss_weight={w}: the feature term needs student_feat and teacher_feat, got student_feat="
                             f"{None if student_feat is None else tuple(student_feat.shape)}, teacher_feat="
                             f"{None if teacher_feat is None else tuple(teacher_feat.shape)} (with index=: the cache's feature matrix, "
                             "TeacherLogitCache(feature_dim=...).features)")
        if student_feat.dim() != 2 or teacher_feat.dim() != 2 or student_feat.shape[1] != teacher_feat.shape[1]:
            raise ValueError(f"feature_loss_weight={w}: student features {tuple(student_feat.shape)} and teacher features "
                             f"{tuple(teacher_feat.shape)} differ in width; project inside the teacher module (there is no learned "
                             "projector in this loss)")
        return student_feat, teacher_feat

    def forward(self, student_logits, teacher_logits, labels, index=None, student_feat=None, teacher_feat=None):
        """index (int64 [rows], on the device): ``teacher_logits`` is then the resident cache -- a TeacherLogitCache or its [n, classes]
        matrix -- and row r's teacher logits are cache[index[r]], read inside the kernel (``hip_ops.distill_loss_cached``).
        student_feat, teacher_feat ([rows, width]; with index= teacher_feat is the cache's feature matrix [n, width]): read only with a
        non-zero feature_loss_weight; with 0.0 they are allowed and ignored."""
        from . import hip_ops
        metered = {} if self.meter is None else {"meter": self.meter}
        featured = self.feature_loss_weight != 0.0
        if featured:   # refused before the logit loss launches
            student_feat, teacher_feat = self._features(student_feat, teacher_feat, teacher_logits, index)
        if index is not None:
            cache = teacher_logits.logits if isinstance(teacher_logits, TeacherLogitCache) else teacher_logits
            loss, self.soft, self.ce = hip_ops.distill_loss_cached(student_logits, cache, index, labels, self.T,
                                                                   self.soft_target_loss_weight, self.ce_loss_weight, **metered)
            if featured:
                loss, self.feat = hip_ops.feature_cosine_cached(student_feat, teacher_feat, index, self.feature_loss_weight, loss)
            return loss
        loss, self.soft, self.ce = hip_ops.distill_loss(student_logits, teacher_logits, labels, self.T, self.soft_target_loss_weight,
                                                        self.ce_loss_weight, **metered)
        if featured:
            loss, self.feat = hip_ops.feature_cosine(student_feat, teacher_feat, self.feature_loss_weight, loss)
        return loss


# ---------------------------------------------------------------- the cached teacher
def fill_plan(n, batch_size, rank=0, world=1):
    """The row blocks [start, stop) of an n-row cache that ``rank`` of ``world`` computes: the rows are cut into blocks of batch_size
    (the last one short) and block k belongs to rank k % world, so a rank's j-th block is block j * world + rank -- round j of the
    exchange.  Over all ranks every row is in exactly one block."""
    n, batch_size, rank, world = int(n), int(batch_size), int(rank), int(world)
    if n <= 0 or batch_size <= 0 or world <= 0 or not 0 <= rank < world:
        raise ValueError(f"fill_plan: n={n}, batch_size={batch_size}, rank={rank}, world={world}")
    blocks = (n + batch_size - 1) // batch_size
    return [(k * batch_size, min((k + 1) * batch_size, n)) for k in range(rank, blocks, world)]


class TeacherLogitCache:
    """The frozen teacher's logits of every sample of a resident set, fp32 [n, classes] on the device, NaN until filled (an unfilled
    row poisons the loss that reads it).  ``.logits`` is allocated once: a captured graph may read it by address.

        cache = TeacherLogitCache(n_train, num_classes, device)
        cache.fill(teacher, view, train_u8_nhwc)                  # ceil(n / 512) teacher calls, once
        loss = criterion(student_logits, cache, labels, index=sel)

    feature_dim (None: no features, and every byte of the behaviour and the file format is that of a cache without the argument): a
    second fixed-address fp32 matrix ``.features`` [n, feature_dim], NaN until filled, holds the teacher's CLS features for
    ``DistillationLoss(feature_loss_weight=...)``; ``store`` / ``fill`` / ``complete`` / ``save`` / ``load`` cover both matrices."""

    META = ("n", "classes", "resize", "crop", "tag")

    def __init__(self, n, classes, device, feature_dim=None):
        n, classes = int(n), int(classes)
        if n <= 0 or classes <= 0:
            raise ValueError(f"TeacherLogitCache: n={n}, classes={classes}")
        if feature_dim is not None and int(feature_dim) <= 0:
            raise ValueError(f"TeacherLogitCache: feature_dim={feature_dim}")
        self.n, self.classes = n, classes
        self.feature_dim = None if feature_dim is None else int(feature_dim)
        self.logits = torch.full((n, classes), float("nan"), dtype=torch.float32, device=device)
        self.features = None if feature_dim is None else torch.full((n, self.feature_dim), float("nan"), dtype=torch.float32, device=device)

    def store(self, index, logits, features=None):
        """logits fp32 [rows, classes] -> rows ``index`` (int64 [rows]; None: rows 0..rows-1) of the cache: one launch.  A row whose
        index lies outside the cache is skipped by the kernel.  features fp32 [rows, feature_dim] (a cache built with feature_dim): the
        same rows of ``.features``, by a second launch of the same kernel."""
        from spectre_vit import _native
        from spectre_vit.hip_ops import _p, _require_gpu, _stream
        if logits.dim() != 2 or logits.dtype != torch.float32 or logits.shape[1] != self.classes:
            raise ValueError(f"TeacherLogitCache.store: fp32 logits [rows, {self.classes}] expected, got {logits.dtype} {tuple(logits.shape)}")
        if index is not None and (index.dtype != torch.int64 or index.shape != logits.shape[:1]):
            raise ValueError(f"TeacherLogitCache.store: index is an int64 vector of {logits.shape[0]} rows, got {index.dtype} {tuple(index.shape)}")
        if (features is None) != (self.features is None):
            raise ValueError(f"TeacherLogitCache.store: a cache with feature_dim={self.feature_dim} "
                             f"{'takes no features' if self.features is None else 'needs features with every store'}")
        if features is not None and (features.dim() != 2 or features.dtype != torch.float32
                                     or tuple(features.shape) != (logits.shape[0], self.feature_dim)):
            raise ValueError(f"TeacherLogitCache.store: fp32 features [{logits.shape[0]}, {self.feature_dim}] expected, got "
                             f"{features.dtype} {tuple(features.shape)}")
        _require_gpu(self.logits, logits, index, features)
        logits = logits.detach().contiguous()
        index = None if index is None else index.contiguous()
        _native.call("spv_logit_cache_store", _p(self.logits), _p(index), _p(logits), logits.shape[0], self.n, self.classes, _stream())
        if features is not None:
            features = features.detach().contiguous()
            _native.call("spv_logit_cache_store", _p(self.features), _p(index), _p(features), features.shape[0], self.n, self.feature_dim,
                         _stream())

    def fill(self, teacher, view, images_u8_nhwc, batch_size=512, rank=0, world=1, process_group=None, batch_hook=None):
        """Every row of the cache: ``view(images, idx)`` -> ``teacher(img, return_features=True)[0].float()`` under no_grad -> ``store``,
        over the row blocks of ``fill_plan`` (a cache with feature_dim stores the same call's features too).  Draws from no torch
        generator.  world > 1: a rank computes its own blocks only, and round by round the ranks exchange them with an all-gather (a
        copy: every rank ends with every row, bits unchanged).
        batch_hook("teacher_fill", k, img_teacher, idx), k the block's number (test seam).  -> the teacher calls of this rank."""
        if getattr(teacher, "training", False):
            raise ValueError("TeacherLogitCache.fill: the teacher is in train mode -- its output is then not a function of the sample "
                             "(dropout, batch statistics); call teacher.eval()")
        if images_u8_nhwc.shape[0] != self.n:
            raise ValueError(f"TeacherLogitCache.fill: {images_u8_nhwc.shape[0]} images for a cache of {self.n} rows")
        dev = self.logits.device
        mine = fill_plan(self.n, batch_size, rank, world)
        rounds = ((self.n + batch_size - 1) // batch_size + world - 1) // world
        calls = 0
        for j in range(rounds):
            out = feats = None
            if j < len(mine):
                start, stop = mine[j]
                idx = torch.arange(start, stop, dtype=torch.int64, device=dev)
                with torch.no_grad():
                    img = view(images_u8_nhwc, idx)
                    if batch_hook is not None:
                        batch_hook("teacher_fill", j * world + rank, img, idx)
                    out, feats = teacher(img, return_features=True)
                    out = out.float()
                if out.shape != (stop - start, self.classes):
                    raise ValueError(f"TeacherLogitCache.fill: the teacher returned {tuple(out.shape)} for {stop - start} samples of "
                                     f"{self.classes} classes")
                if self.features is None:
                    feats = None
                    self.store(idx, out)
                else:
                    feats = feats.float()
                    if feats.shape != (stop - start, self.feature_dim):
                        raise ValueError(f"TeacherLogitCache.fill: the teacher returned features {tuple(feats.shape)} for {stop - start} "
                                         f"samples of feature_dim={self.feature_dim}; project inside the teacher module")
                    self.store(idx, out, feats)
                calls += 1
            if world > 1:
                self._exchange(j, out, feats, batch_size, rank, world, process_group)
        return calls

    def _exchange(self, j, out, feats, batch_size, rank, world, process_group):
        """round j: every rank hands in its block (padded to batch_size rows) and stores the others' at their rows"""
        import torch.distributed as dist
        dev = self.logits.device
        # gloo gathers host tensors; RCCL device tensors.  Either way the rows are copied, never summed.
        where = torch.device("cpu") if dist.get_backend(process_group) == "gloo" else dev

        def gather(block, width):
            send = torch.full((batch_size, width), float("nan"), dtype=torch.float32, device=where)
            if block is not None:
                send[:block.shape[0]].copy_(block)
            recv = [torch.empty_like(send) for _ in range(world)]
            dist.all_gather(recv, send, group=process_group)
            return recv

        recv = gather(out, self.classes)
        frecv = None if self.features is None else gather(feats, self.feature_dim)
        for r in range(world):
            start = (j * world + r) * batch_size
            stop = min(start + batch_size, self.n)
            if r != rank and start < stop:
                self.store(torch.arange(start, stop, dtype=torch.int64, device=dev), recv[r][:stop - start].to(dev),
                           None if frecv is None else frecv[r][:stop - start].to(dev))

    def complete(self):
        """no NaN left: one host read"""
        if self.features is None:
            return not bool(torch.isnan(self.logits).any().item())
        return not bool((torch.isnan(self.logits).any() | torch.isnan(self.features).any()).item())

    def save(self, path, **meta):
        """torch.save of {"logits", "meta"}; meta: resize, crop, tag (what the rows were computed from), n and classes are the cache's.
        A cache with feature_dim: {"logits", "features", "meta"}, the meta with a "feature_dim" field."""
        unknown = set(meta) - set(self.META[2:])
        if unknown:
            raise ValueError(f"TeacherLogitCache.save: unknown meta field(s) {sorted(unknown)} (resize, crop, tag)")
        m = {"n": self.n, "classes": self.classes, "resize": None, "crop": None, "tag": None}
        m.update(meta)
        blob = {"logits": self.logits.detach().cpu(), "meta": m}
        if self.features is not None:
            m["feature_dim"] = self.feature_dim
            blob["features"] = self.features.detach().cpu()
        torch.save(blob, path)

    @classmethod
    def load(cls, path, device, feature_dim=None, **expect):
        """The cache saved at ``path`` on ``device``.  Every field of ``expect`` (n, classes, resize, crop, tag) must equal the file's;
        a file with NaN rows is refused.  feature_dim: the features are asked for -- a file without them, or with another width, is
        refused; None: a file's features, if it has any, are left out."""
        blob = torch.load(path, map_location="cpu", weights_only=True)
        logits, meta = blob["logits"], blob["meta"]
        for k, v in expect.items():
            if k not in cls.META:
                raise ValueError(f"TeacherLogitCache.load: unknown meta field {k!r}")
            if meta.get(k) != v:
                raise ValueError(f"TeacherLogitCache.load: {path} was saved with {k}={meta.get(k)!r}, expected {k}={v!r}")
        if logits.dtype != torch.float32 or tuple(logits.shape) != (meta["n"], meta["classes"]):
            raise ValueError(f"TeacherLogitCache.load: {path} holds {logits.dtype} {tuple(logits.shape)}, its meta says fp32 "
                             f"[{meta['n']}, {meta['classes']}]")
        if bool(torch.isnan(logits).any()):
            raise ValueError(f"TeacherLogitCache.load: {path} is incomplete ({int(torch.isnan(logits).any(dim=1).sum())} rows hold NaN)")
        features = None
        if feature_dim is not None:
            features = blob.get("features")
            if features is None or meta.get("feature_dim") is None:
                raise ValueError(f"TeacherLogitCache.load: {path} holds no features (it was saved from a cache without feature_dim), "
                                 f"feature_dim={feature_dim} was asked for")
            if meta["feature_dim"] != int(feature_dim):
                raise ValueError(f"TeacherLogitCache.load: {path} was saved with feature_dim={meta['feature_dim']!r}, expected "
                                 f"feature_dim={int(feature_dim)!r}")
            if features.dtype != torch.float32 or tuple(features.shape) != (meta["n"], meta["feature_dim"]):
                raise ValueError(f"TeacherLogitCache.load: {path} holds features {features.dtype} {tuple(features.shape)}, its meta says "
                                 f"fp32 [{meta['n']}, {meta['feature_dim']}]")
            if bool(torch.isnan(features).any()):
                raise ValueError(f"TeacherLogitCache.load: {path} is incomplete ({int(torch.isnan(features).any(dim=1).sum())} feature "
                                 "rows hold NaN)")
        cache = cls(meta["n"], meta["classes"], device, feature_dim=feature_dim)
        cache.logits.copy_(logits)
        if features is not None:
            cache.features.copy_(features)
        return cache
