"""Training harness -- the build's counterpart of reference spectre_vit/repl/train.py.

Same loop structure (train.py:207-295 classification, :298-361 distillation): seeds, model from a parsed config,
AdamW(betas, lr, weight_decay), autocast, per-epoch eval, accuracy bookkeeping on device, best-validation
``state_dict`` checkpoint.  What differs: the data resident on the GPU -- synthetic CIFAR-shaped sets by default, or, ``data_root=`` /
``--data-root``, the dataset files the reference's ``./data`` holds, read by spectre_vit.datasets (no torchvision / network) --,
bf16 autocast (no GradScaler needed), the training transform chain of train.py:100-115 as an on-GPU kernel pair (``--augment``,
spectre_vit.augment) instead of PIL on loader workers, scalars to a JSON-lines file instead of TensorBoard, optional data parallelism
(one process per GPU, RCCL all-reduce through spectre_vit.dp.GradReducer), and a synthetic frozen teacher for the
distillation path (the DINOv3 weights are unavailable offline).  ``train(distill=True)`` is the early form of that path (the teacher
sees a 64 x 64 interpolation of the student's batch); ``train_distill`` / ``--distill-paired`` is the loop with the reference's two views
per sample, the teacher's 224 view and the KD loss on HIP kernels, and the step replayed from a graph on request.
Both entry points check their arguments, build what is their own (criterion, teacher / view / cache, step object) and call the shared
_setup and _run_epochs (the one loop; _epoch_tail is its validation, record, log and checkpoints).  A step object owes the loop
batches() -- what the host knows of each next batch -- run(batch, n) -> (loss, y_pred, img, label, *loss terms) and close().

    python -m spectre_vit.harness --config spectre_vit/configs/spectre_vit_cifar100.py --epochs 2 --steps-per-epoch 20
"""
from __future__ import annotations

import argparse
import json
import math
import os
import random
import time
from types import SimpleNamespace

import numpy as np
import torch
import torch.distributed as dist
from torch import nn, optim

from spectre_vit.augment import TrainAugment
from spectre_vit.configs.parser import parse_config
from spectre_vit.datasets import ResidentSet
from spectre_vit.distillation import DistillationLoss, SyntheticTeacher, TeacherView, distillation_loss
from spectre_vit.dp import GradReducer, broadcast_module
from spectre_vit.loss import CrossEntropyLoss
from spectre_vit.models.spectre.spectre import SpectreViT
from spectre_vit.models.spectre_branch.spectre_branch import SpectreBranch

CIFAR_MEAN = (0.5071, 0.4867, 0.4408)  # train.py:109-112
CIFAR_STD = (0.2675, 0.2565, 0.2761)


def seed_everything(seed: int):
    """train.py:31-35"""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def augment_seed(seed: int, rank: int = 0) -> int:
    """the augmentation stream's 64-bit seed: the config seed in the low word, the rank in the high one (ranks draw different tables)"""
    return (int(seed) & 0xFFFFFFFF) | ((int(rank) & 0xFFFFFFFF) << 32)


def loader_seed(seed: int) -> int:
    """the resident loader's 64-bit seed: the config seed's low word, as augment_seed(seed, 0).  NOT a function of the rank: the ranks
    take disjoint parts (idx[rank::world]) of ONE permutation, so they must draw the same one; the rank enters through the position"""
    return augment_seed(seed, 0)


def build_model(c, mixer="permut", device="cuda", model="spectre"):
    """train.py:48-59; model="spectre_branch" builds reference spectre_branch.py's SpectreBranch from the same config fields"""
    if model == "spectre_branch":
        return SpectreBranch(img_size=c.img_size, patch_size=c.patch_size, in_channels=c.in_channels, num_classes=c.num_classes,
                             embed_dim=c.embed_dim, num_encoders=c.num_encoders, num_heads=c.num_heads, hidden_dim=c.hidden_dim,
                             dropout=c.dropout, activation=c.activation).to(device)
    if model != "spectre":
        raise ValueError(f"unknown model {model!r} (spectre, spectre_branch)")
    return SpectreViT(img_size=c.img_size, patch_size=c.patch_size, in_channels=c.in_channels, num_classes=c.num_classes,
                      embed_dim=c.embed_dim, num_encoders=c.num_encoders, num_heads=c.num_heads, hidden_dim=c.hidden_dim,
                      dropout=c.dropout, activation=c.activation, mixer=mixer).to(device)


class SyntheticCifar(ResidentSet):
    """class-conditional uint8 images resident in HBM: a fixed random template per class plus noise, so a model can
    actually learn something; normalised like train.py:109-112 when a batch is drawn."""

    def __init__(self, n, c, device, seed=0):
        g = torch.Generator().manual_seed(seed)
        templates = torch.rand(c.num_classes, c.in_channels, c.img_size, c.img_size, generator=torch.Generator().manual_seed(1))
        self.labels = torch.randint(0, c.num_classes, (n,), generator=g)
        noise = torch.rand(n, c.in_channels, c.img_size, c.img_size, generator=g)
        self.images = ((0.6 * templates[self.labels] + 0.4 * noise) * 255).to(torch.uint8).to(device)
        self.labels = self.labels.to(torch.uint8 if c.num_classes <= 256 else torch.int64).to(device)  # uint8 as train.py:218
        self.mean = torch.tensor(CIFAR_MEAN[:c.in_channels], device=device).view(1, -1, 1, 1)
        self.std = torch.tensor(CIFAR_STD[:c.in_channels], device=device).view(1, -1, 1, 1)
        self.mean_values, self.std_values = CIFAR_MEAN[:c.in_channels], CIFAR_STD[:c.in_channels]


def _step_control_args(lr_schedule, warmup_steps, eta_min, clip_grad_norm, skip_nonfinite, total_steps, accumulate_steps=None):
    """the harness's step-control arguments -> FusedAdamW keywords; {} when none is on (the optimizer choice is then untouched).
    total_steps counts loader steps; with accumulate_steps=k each is a micro-step and the schedule runs over total_steps // k optimizer
    steps (warmup_steps counts optimizer steps as well)."""
    if lr_schedule not in (None, "cosine"):
        raise ValueError(f"lr_schedule={lr_schedule!r}: None or 'cosine'")
    if lr_schedule is None and (warmup_steps or eta_min):
        raise ValueError("warmup_steps / eta_min belong to lr_schedule='cosine'")
    k = accumulate_steps
    if k is not None and (isinstance(k, bool) or not isinstance(k, int) or k < 1):
        raise ValueError(f"accumulate_steps={k!r} must be None or an int >= 1")
    if lr_schedule is None and clip_grad_norm is None and not skip_nonfinite and k is None:
        return {}
    from spectre_vit.optim import CosineSchedule
    schedule = CosineSchedule(total_steps // (k or 1), warmup_steps, eta_min) if lr_schedule == "cosine" else None
    control = dict(schedule=schedule, max_grad_norm=clip_grad_norm, skip_nonfinite=skip_nonfinite)
    if k is not None:
        control["accumulate_steps"] = k
    return control


def _step_control_record(optimizer):
    """the epoch record's step-control entries: ONE read of the optimizer's control block.  Under accumulation they describe the last
    window boundary, and the record gains the window length and the optimizer steps made so far (windows closed, dropped ones included)"""
    c = optimizer._read_ctl()
    rec = {"LR": optimizer.last_lr(c)[0], "GradNorm": c["grad_norm"], "SkippedSteps": c["skipped"]}
    if optimizer.accumulate_steps is not None:
        rec["AccumulateSteps"] = optimizer.accumulate_steps
        rec["OptimizerSteps"] = c["sched_step"]
    return rec


def _optimizer_choice(optimizer, momentum, nesterov):
    """the harness's optimizer arguments -> (name, the rule's keywords).  None = "adamw" left unsaid: the same optimizer, and the epoch
    record does not name it.  "adam" / "sgd" are the reference script's two other optimizer lines (train.py:197-198, :307):
    spectre_vit.optim.FusedAdam / FusedSGD on every path (there is no torch.optim fallback for them); momentum / nesterov belong to
    "sgd", whose defaults are the script's (momentum=0.9, nesterov=True).  Raises before any device is touched."""
    if optimizer not in (None, "adamw", "adam", "sgd"):
        raise ValueError(f"optimizer={optimizer!r}: 'adamw', 'adam' or 'sgd'")
    if isinstance(momentum, bool) or not isinstance(momentum, (int, float)) or not 0.0 <= momentum < 1.0:
        raise ValueError(f"momentum={momentum!r} must be a float in [0, 1)")
    if not isinstance(nesterov, bool):
        raise ValueError(f"nesterov={nesterov!r} must be True or False")
    if optimizer != "sgd":
        if momentum != 0.9 or nesterov is not True:
            raise ValueError("momentum / nesterov belong to optimizer='sgd'")
        return optimizer, {}
    if nesterov and momentum == 0.0:
        raise ValueError("nesterov=True needs momentum > 0 (torch.optim.SGD's rule): pass nesterov=False with momentum=0")
    return optimizer, dict(momentum=float(momentum), nesterov=nesterov)


def _make_optimizer(name, rule, params, c, lr, fused):
    """the optimizer of a training loop.  fused: the keywords of the one-launch optimizer (capturable, static_grads, control, averaging)
    or None where the default AdamW may stay torch's own (the reference's eager loop shape)"""
    if name == "sgd":     # train.py:198
        from spectre_vit.optim import FusedSGD
        return FusedSGD(params, lr=lr, weight_decay=c.adam_weight_decay, **rule, **(fused or dict(capturable=True)))
    if name == "adam":    # train.py:197, :307
        from spectre_vit.optim import FusedAdam
        return FusedAdam(params, betas=c.adam_betas, lr=lr, weight_decay=c.adam_weight_decay, **(fused or dict(capturable=True)))
    if fused is not None:
        from spectre_vit.optim import FusedAdamW
        return FusedAdamW(params, betas=c.adam_betas, lr=lr, weight_decay=c.adam_weight_decay, **fused)
    return optim.AdamW(params, betas=c.adam_betas, lr=lr, weight_decay=c.adam_weight_decay)  # train.py:199-201, :307-309


def _ema_args(ema_decay, ema_warmup):
    """the harness's two averaging arguments -> FusedAdamW keywords; {} when averaging is off.  Raises before any device is touched."""
    if ema_decay is None:
        if ema_warmup:
            raise ValueError("ema_warmup=True needs ema_decay")
        return {}
    if isinstance(ema_decay, bool) or not 0.0 <= float(ema_decay) < 1.0:
        raise ValueError(f"ema_decay={ema_decay!r} must be None or a float in [0, 1)")
    return dict(ema_decay=float(ema_decay), ema_warmup=bool(ema_warmup))


def _train_meter(device_meter, epoch_steps, device):
    """the harness's device_meter argument -> the epoch's spectre_vit.meter.TrainMeter (one log row per step), or None when off"""
    if not device_meter:
        return None
    from spectre_vit.meter import TrainMeter
    return TrainMeter(max(epoch_steps, 1), topk=5, device=device)


def _check_device_meter(device_meter, distill=False):
    """raises before any device is touched"""
    if not isinstance(device_meter, bool):
        raise ValueError(f"device_meter={device_meter!r} must be True or False")
    if device_meter and distill:
        raise ValueError("device_meter=True meters the criterion's launch: the early distill=True form has no criterion on its training "
                         "path (train_distill has)")


def _loader_output(augment, uint8_input, chans, height, width):
    """the ResidentLoader output that serves a training set's shape: with augmentation the fused LDS fetch where it can stage the image,
    the fused tiled fetch for the sizes only the tiled chain takes (spv_augment_plan == 2), and index and labels alone ("none": draw and
    apply host-issued) for what is left -- the LDS border shape, whose whole-image chain the tiled kernels are not held to bit for bit"""
    from spectre_vit import _native
    if not augment:
        return "uint8" if uint8_input else "float"
    if _native.call("spv_loader_augment_supported", chans, height, width):
        return "augment"
    return "augment_tiled" if _native.call("spv_augment_plan", chans, height, width) == 2 else "none"


def _check_device_loader(device_loader, distill=False):
    """raises before any device is touched"""
    if not isinstance(device_loader, bool):
        raise ValueError(f"device_loader={device_loader!r} must be True or False")
    if device_loader and distill:
        raise ValueError("device_loader=True fetches the batches of the plain training step: the early distill=True form is not built "
                         "for it")


def _eager_validate(model, batches, criterion, amp, batch_hook, world, device, float_logits=False):
    """one eager validation pass: every sample of the rank's shard, the loss sample-weighted (the tail batch is short), the sums kept on
    the device and read once.  -> (accuracy, loss, samples)"""
    v_correct = torch.zeros((), device=device, dtype=torch.int64)
    v_loss = torch.zeros((), device=device)
    v_total, v_steps = 0, 0
    with torch.no_grad():
        for img, label in batches:
            if batch_hook is not None:
                batch_hook("val", v_steps, img, label)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                y_pred = model(img)
            v_correct += (label == torch.argmax(y_pred, dim=1)).sum()
            v_loss += criterion(y_pred.float() if float_logits else y_pred, label.long()) * label.size(0)
            v_total += label.size(0)
            v_steps += 1
    stats = torch.stack([v_correct.float(), torch.tensor(float(v_total), device=device), v_loss])
    if world > 1:
        dist.all_reduce(stats)
    return (stats[0] / stats[1].clamp(min=1)).item(), (stats[2] / stats[1].clamp(min=1)).item(), int(stats[1].item())


def _graph_validate(session, batches, batch_hook, world):
    """one validation pass through a spectre_vit.inference.InferenceSession: the model's current weights are taken (refresh), every batch
    is one graph replay that ends in the on-device metrics kernel, and the epoch costs ONE host read.  -> (accuracy, loss, samples)"""
    session.refresh()
    session.reset_stats()
    v_steps = 0
    for img, label in batches:
        if batch_hook is not None:
            batch_hook("val", v_steps, img, label)
        session.accumulate(img, label)
        v_steps += 1
    acc = session.stats_tensor()   # float64 (seen, top1, topk, loss_sum)
    if world > 1:
        dist.all_reduce(acc)
    seen, top1, _, loss_sum = acc.tolist()
    return top1 / max(seen, 1.0), loss_sum / max(seen, 1.0), int(seen)


def _eval_session(model, n_val, val_batch, rank, world, autocast_dtype, uint8):
    from spectre_vit.inference import InferenceSession, eval_buckets
    shard = len(range(rank, n_val, world))
    return InferenceSession(model, batch_sizes=eval_buckets(shard, val_batch), autocast_dtype=autocast_dtype,
                            input="uint8" if uint8 else "float")


class _Unsaid(int):
    """n_train / n_val left unsaid: the synthetic sets' sizes as ever (it IS that int), the whole split with data_root"""


_UNSAID_TRAIN, _UNSAID_VAL = _Unsaid(4096), _Unsaid(1024)


def _data_args(c, config_path, data_root, dataset, normalize, n_train, n_val):
    """the harness's data arguments -> (the two host-side FileDatasets' record or None, n_train, n_val, the fingerprint's further
    keys).  Without data_root: the synthetic sets of 4096 / 1024 samples unless a number is said, and nothing more.  With it the files
    are read and checked here, on the host: n_train / n_val left unsaid (or None) are the whole split, a number is the limit.  Raises
    before any device is touched."""
    if data_root is None:
        if dataset is not None or normalize is not None:
            raise ValueError("dataset / normalize describe the files under data_root: they need data_root")
        n_train, n_val = (4096 if n_train is None else n_train), (1024 if n_val is None else n_val)
        return None, int(n_train) if isinstance(n_train, _Unsaid) else n_train, int(n_val) if isinstance(n_val, _Unsaid) else n_val, {}
    n_train, n_val = (None if isinstance(n, _Unsaid) else n for n in (n_train, n_val))
    from spectre_vit import datasets
    if dataset is None:
        dataset = datasets.dataset_of_config(config_path)
    norm = datasets.resolve_normalize(dataset, normalize)
    sets = []
    for split, limit, what in (("train", n_train, "n_train"), ("test", n_val, "n_val")):
        if limit is not None and (isinstance(limit, bool) or not isinstance(limit, int) or limit < 1):
            raise ValueError(f"{what}={limit!r} must be None (the whole {split} split) or an int >= 1")
        try:
            ds = datasets.FileDataset(data_root, dataset, split, None, norm, limit)
        except ValueError as e:
            raise ValueError(f"{what}: {e}") if limit is not None and "is above the" in str(e) else e
        if (ds.channels, ds.height, ds.width) != (c.in_channels, c.img_size, c.img_size):
            raise ValueError(f"{ds.root} ({dataset}, {split}) holds {ds.channels} x {ds.height} x {ds.width} images, the config "
                             f"in_channels={c.in_channels}, img_size={c.img_size}")
        if ds.num_classes > c.num_classes:
            raise ValueError(f"{ds.root} ({dataset}, {split}) has {ds.num_classes} classes, the config num_classes={c.num_classes}")
        ds.num_classes = int(c.num_classes)   # the model's: the label dtype and the histogram's width (MNIST's configs keep 100)
        sets.append(ds)
    train_set, val_set = sets
    plain_norm = norm if isinstance(norm, str) else [list(norm[0]), list(norm[1])]
    data = SimpleNamespace(train=train_set, val=val_set, name=dataset, root=train_set.root, normalize=norm,
                           digest=f"{train_set.digest}-{val_set.digest}")
    return data, len(train_set), len(val_set), dict(dataset=dataset, dataset_digest=data.digest, normalize=plain_norm)


def _setup(c, mixer, model_name, epochs, steps_per_epoch, batch_size, n_train, n_val, out_dir, graph, device_meter, optimizer_name, rule,
           ema, control_args, data=None):
    """what every run has before its first batch, from a parsed config and the arguments train() and train_distill() share -> the run's
    record: rank / world / device, seed, lr, the model (built under the seed, broadcast), the two sets, batch_size, epoch_steps (the
    loader steps of one epoch), the step control / meter / optimizer / reducer, the open scalars.jsonl (rank 0), the shuffle generator,
    and the loop's state (global_step, history, the two best accuracies, the lazy evaluation session, the start time)"""
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)  # always: kernels launch on the current device's stream (also with a pre-initialised group)
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl")
    device = torch.device("cuda", local_rank)
    seed = getattr(c, "random_seed", 42)
    lr = getattr(c, "learning_rate", 1e-3)
    seed_everything(seed)
    model = build_model(c, mixer, device, model_name)
    broadcast_module(model)
    batch_size = batch_size or c.batch_size
    dataset = None
    if data is None:
        train_set = SyntheticCifar(n_train, c, device, seed=seed)
        val_set = SyntheticCifar(n_val, c, device, seed=seed + 1)
    else:   # the files were read and checked on the host (_data_args); a measured normalisation is the train split's for both
        train_set = data.train.upload(device)
        val_set = data.val.upload(device, measured_from=train_set)
        dataset = {"name": data.name, "root": data.root, "n_train": n_train, "n_val": n_val, "digest": data.digest,
                   "mean": list(train_set.mean_values), "std": list(train_set.std_values)}
        if hasattr(model, "modules"):   # uint8 input: the model's patch gather normalises with the set's values
            from spectre_vit.hip_ops import PixelNorm
            for m in model.modules():
                if hasattr(m, "pixel_norm"):
                    m.pixel_norm = PixelNorm(train_set.mean_values, train_set.std_values)
    per_pass = (n_train // world) // batch_size
    epoch_steps = min(per_pass, steps_per_epoch) if steps_per_epoch else per_pass
    control = _step_control_args(total_steps=epoch_steps * epochs, **control_args)
    meter = _train_meter(device_meter, epoch_steps, device)
    optimizer, reducer = _optimizer_and_reducer(optimizer_name, rule, model, c, lr, graph, control, ema)
    os.makedirs(out_dir, exist_ok=True)
    log_f = open(os.path.join(out_dir, "scalars.jsonl"), "a") if rank == 0 else None
    return SimpleNamespace(c=c, rank=rank, world=world, device=device, seed=seed, lr=lr, model=model, train_set=train_set, val_set=val_set,
                           n_val=n_val, batch_size=batch_size, epoch_steps=epoch_steps, control=control, ema=ema, meter=meter,
                           optimizer_name=optimizer_name, optimizer=optimizer, reducer=reducer, out_dir=out_dir, log_f=log_f,
                           gen=torch.Generator().manual_seed(seed), global_step=0, history=[], best_acc=0.0, best_ema_acc=0.0,
                           session=None, start=time.perf_counter(), start_epoch=0, elapsed=0.0, checkpoint_every=None, resume=None,
                           fingerprint=None, snapshot=None, loader=None, step_resume={}, dataset=dataset)


def _optimizer_and_reducer(name, rule, model, c, lr, graph, control, ema):
    """graph: the one-launch optimizer on fixed-address gradients and no reducer (the graphed step owns its gradient buffer); eager: the
    reference's loop shape -- torch's own AdamW unless step control, averaging or the named rule ask for a fused one -- and GradReducer"""
    if graph:
        return _make_optimizer(name, rule, model.parameters(), c, lr, dict(capturable=True, static_grads=True, **control, **ema)), None
    fused = dict(capturable=True, **control, **ema) if control or ema else None
    return _make_optimizer(name, rule, model.parameters(), c, lr, fused), GradReducer(model)


def _resident_loader(run, train_nhwc, aug, uint8_input):
    """the run's spectre_vit.data.ResidentLoader: its output picked by shape (_loader_output), this loop's steps per epoch, this rank's
    shard.  With a fused output the loader fetches and augments in ONE call (the table is keyed by the loader's cursor, which equals
    global_step); with "none" it fetches index and labels only, draw and apply host-issued as without the loader"""
    from spectre_vit.data import ResidentLoader
    H, W, C = train_nhwc.shape[1:]
    output = _loader_output(aug is not None, uint8_input, C, H, W)
    mean, std = run.train_set.mean_values, run.train_set.std_values
    return ResidentLoader(train_nhwc, run.train_set.labels, run.batch_size, mean, std, seed=loader_seed(run.seed),
                          rank=run.rank, world=run.world, steps_per_epoch=run.epoch_steps, output=output,
                          augment=aug if output.startswith("augment") else None)


def _eager_update(run, loss):
    run.reducer.zero_grad()
    loss.backward()
    run.reducer.finish()
    run.optimizer.step()


def _step(batches, run_step, gstep):
    """a step object: batches() yields what the host knows of the next batch, run(batch, n) trains on it, close() closes the graphed
    step where one was built (gstep: a one-element list, filled on the first batch)"""
    return SimpleNamespace(batches=batches, run=run_step, close=lambda: gstep[0] is not None and gstep[0].close(), gstep=gstep)


class _TrainBooks:
    """an epoch's training loss and accuracy, kept where the run keeps them: in the criterion's meter, read once; or, without a meter,
    accumulated on the device -- the loss as a running sum whose mean is taken on the device (train()), or, block=True, as one row of
    `names` per step read once, the mean taken on the host (train_distill(), which logs every step).  The two means differ in bits."""

    def __init__(self, run, names, block):
        self.run, self.names, self.block = run, names, block

    def begin(self):
        if self.run.meter is not None:
            return
        device = self.run.device
        self.correct, self.total = torch.zeros((), device=device, dtype=torch.int64), 0
        self.loss = torch.zeros((max(self.run.epoch_steps, 1), len(self.names)), device=device) if self.block else torch.zeros((), device=device)

    def add(self, k, y_pred, label, loss, *terms):
        if self.run.meter is not None:
            return
        self.correct += (label == torch.argmax(y_pred, dim=1)).sum()
        self.total += label.size(0)
        if self.block:
            torch.stack((loss.detach(), *terms), out=self.loss[k])
        else:
            self.loss += loss.detach()  # accumulated on device: no host sync per step (train.py:243 syncs every step)

    def read(self, steps):
        """the epoch's one read -> (Loss/Train, Accuracy/Train, Accuracy/TrainTop5 or None, the per-step log lines' entries)"""
        meter = self.run.meter
        if meter is not None:
            metered = meter.read()
            meter.reset()
            return metered["loss_mean"], metered["accuracy"], metered["accuracy_topk"], [dict(zip(self.names, row)) for row in metered["rows"]]
        rows = self.loss[:steps].tolist() if self.block else []
        train_loss = sum(r[0] for r in rows) / max(steps, 1) if self.block else (self.loss / max(steps, 1)).item()
        return train_loss, self.correct.item() / max(self.total, 1), None, [dict(zip(self.names, row)) for row in rows]


def _validator(run, graph_eval, amp, uint8=False, float_logits=False):
    """-> validate(hook): one pass over the validation set, every sample of the rank's shard -> (accuracy, loss, samples).  graph_eval:
    through an InferenceSession built on first use and kept in the run's record; otherwise eagerly with a meter-less criterion"""
    criterion = CrossEntropyLoss()
    val_batch = min(getattr(run.c, "val_batch_size", run.batch_size), run.n_val)

    def validate(hook):
        batches = run.val_set.batches(val_batch, False, None, run.rank, run.world, raw_uint8=uint8, drop_last=False)
        if not graph_eval:
            return _eager_validate(run.model, batches, criterion, amp, hook, run.world, run.device, float_logits)
        if run.session is None:
            run.session = _eval_session(run.model, run.n_val, val_batch, run.rank, run.world, torch.bfloat16 if amp else None, uint8)
        return _graph_validate(run.session, batches, hook, run.world)
    return validate


def _checkpoint_args(checkpoint_every, resume, out_dir, fingerprint):
    """the harness's two checkpoint arguments -> (checkpoint_every, the loaded state to resume from or None).  Raises before any device
    is touched: a bad argument, a data-parallel rank, a missing file, and whatever spectre_vit.checkpoint.load_train_state refuses --
    a damaged file by its job's name, another run's file by the first differing key of the fingerprint."""
    if checkpoint_every is not None:
        if isinstance(checkpoint_every, float):
            raise ValueError(f"checkpoint_every={checkpoint_every!r}: mid-epoch checkpoints are not built -- it counts whole epochs (an int >= 1)")
        if isinstance(checkpoint_every, bool) or not isinstance(checkpoint_every, int) or checkpoint_every < 1:
            raise ValueError(f"checkpoint_every={checkpoint_every!r} must be None or an int >= 1 (epochs)")
    if resume is not None and resume is not True and not isinstance(resume, (str, os.PathLike)):
        raise ValueError(f"resume={resume!r}: None, True (out_dir/train_state.pt) or a path")
    if checkpoint_every is None and resume is None:
        return None, None
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError("checkpoint_every / resume with world > 1 are not built: every rank's seed word and RNG states need a file of "
                         "their own")
    if resume is None:
        return checkpoint_every, None
    from spectre_vit import checkpoint
    path = os.path.join(out_dir, checkpoint.FILE_NAME) if resume is True else os.fspath(resume)
    if not os.path.exists(path):
        raise ValueError(f"resume: no such file: {path}")
    return checkpoint_every, checkpoint.load_train_state(path, fingerprint)


def _fingerprint(entry, c, **args):
    """what shapes a run's trajectory: the parsed config's fields and the arguments of train() / train_distill() that do (graph_eval,
    device_meter, log, batch_hook and out_dir do not enter).  A resume is held to it key by key."""
    fp = {"entry": entry, "world": int(os.environ.get("WORLD_SIZE", "1"))}
    fp.update({f"config/{k}": v for k, v in sorted(vars(c).items())})
    fp.update(args)
    return fp


def _state_blocks(run, step):
    """the run's device-resident state as the named tensors of ONE snapshot launch -> (blocks, the names the non-finite gate watches):
    every entry of model.state_dict() (the parameters gated), the optimizer's per-parameter state (the averages gated), control
    block and accumulators, the loader's cursor block, the graphed step's seed word"""
    from spectre_vit import checkpoint
    blocks = [("model/" + k, v) for k, v in run.model.state_dict().items()]
    gated = {"model/" + k for k, _ in run.model.named_parameters()}
    opt = run.optimizer
    optim_blocks = (opt.state_blocks() if hasattr(opt, "state_blocks") else checkpoint.optimizer_blocks(opt))[0]
    blocks += optim_blocks
    gated |= {name for name, _ in optim_blocks if name.endswith("/ema")}
    if run.loader is not None:
        blocks.append(("loader/cursor", run.loader._cursor))
    gstep = getattr(step, "gstep", [None])[0]
    if gstep is not None:
        blocks.append(("step/seed_word", gstep.seed_word))
    return blocks, gated


def _take_checkpoint(run, step, epoch):
    """after an epoch's tail: ONE launch takes the device's state in stream order (the snapshot is built at the first call, when every
    block exists), the host's part is put together here, and the file is written behind the training's back"""
    from spectre_vit import checkpoint
    if run.snapshot is None:
        def report(rec):   # a finished write, told at the next take() or at close()
            run.log_f.write(json.dumps(rec) + "\n")
            run.log_f.flush()
        blocks, gated = _state_blocks(run, step)
        run.snapshot = checkpoint.StateSnapshot(blocks, run.out_dir, gated=gated, report=report)
    opt = run.optimizer
    _, optim_host, aliases = opt.state_blocks() if hasattr(opt, "state_blocks") else checkpoint.optimizer_blocks(opt)
    gstep = getattr(step, "gstep", [None])[0]
    host = dict(fingerprint=run.fingerprint, epoch=epoch, global_step=run.global_step, history=[dict(r) for r in run.history],
                best_acc=run.best_acc, best_ema_acc=run.best_ema_acc, elapsed=run.elapsed + time.perf_counter() - run.start,
                param_groups=checkpoint.packed_param_groups(opt), optim_host=optim_host, optim_aliases=aliases,
                loader=None if run.loader is None else run.loader.state_dict(),
                capture_rng_state=None if gstep is None else gstep.capture_rng_state, rng=checkpoint.host_rng_state(run.gen))
    run.snapshot.take(host, epoch)


def _restore(run):
    """a loaded train state into the run _setup built: model, optimizer (with the open window: control block and accumulators) and
    loader; the loop's counters, history and best accuracies; the seed word and the capture's generator state for the step object the
    first batch builds; the RNG states LAST, because set-up drew from them"""
    from spectre_vit import checkpoint, shadows
    host, tensors = run.resume["host"], run.resume["tensors"]
    run.model.load_state_dict({k[len("model/"):]: v for k, v in tensors.items() if k.startswith("model/")})
    shadows.invalidate_weight_shadows()
    opt = run.optimizer
    optim_sd = checkpoint.optimizer_state_dict(tensors, host)
    if hasattr(opt, "load_train_state"):
        accs = None
        if opt.accumulate_steps is not None:
            accs = [tensors[f"optim/accumulators/{gi}"] for gi in range(len(opt.param_groups))]
        opt.load_train_state(optim_sd, tensors.get("optim/control_block"), accs)
    else:
        opt.load_state_dict(optim_sd)
    if getattr(run, "loader", None) is not None:
        cursor = int(tensors["loader/cursor"][0]) & (2 ** 64 - 1)
        if cursor != host["loader"]["step"]:
            raise ValueError(f"resume: the loader's saved cursor block is at step {cursor}, its host mirror at {host['loader']['step']}")
        run.loader.load_state_dict(host["loader"])
    if "step/seed_word" in tensors:
        run.step_resume = dict(seed_word=int(tensors["step/seed_word"][0]) & (2 ** 64 - 1), capture_rng_state=host["capture_rng_state"])
    run.global_step, run.start_epoch, run.elapsed = host["global_step"], host["epoch"], host["elapsed"]
    run.history[:] = host["history"]
    run.best_acc, run.best_ema_acc = host["best_acc"], host["best_ema_acc"]
    checkpoint.set_host_rng_state(host["rng"], getattr(run, "gen", None))


def _epoch_tail(run, epoch, steps, first_step, train, validate, batch_hook, log):
    """after an epoch's training: validation, the epoch record (with the averaged weights' second pass), rank 0's log lines -- the
    per-step ones, then the record -- and the two best checkpoints.  train: what _TrainBooks.read returned"""
    train_loss, train_acc, top5, lines = train
    val_acc, val_loss, val_samples = validate(batch_hook)
    rec = {"epoch": epoch + 1, "Loss/Train": train_loss, "Loss/Validation": val_loss, "Accuracy/Train": train_acc,
           "Accuracy/Validation": val_acc, "steps": steps, "val_samples": val_samples}
    if top5 is not None:
        rec["Accuracy/TrainTop5"] = top5
    if lines and "Batch Loss/Feat" in lines[0]:   # the feature term's epoch mean, from the rows the other losses come from
        rec["Loss/Feat"] = sum(line["Batch Loss/Feat"] for line in lines) / len(lines)
    if run.optimizer_name is not None:
        rec["Optimizer"] = run.optimizer_name
    if run.control:
        rec.update(_step_control_record(run.optimizer))
    if run.ema:   # the same pass on the averaged weights (a session keeps its own copies: leaving the context does not disturb it)
        with run.optimizer.ema_weights():
            rec["Accuracy/ValidationEMA"], rec["Loss/ValidationEMA"], _ = validate(None)
    if getattr(run, "dataset", None) is not None:   # a run from files (data_root) says which
        rec["Dataset"] = dict(run.dataset)
    run.history.append(rec)
    if run.rank != 0:
        return
    for k, line in enumerate(lines):
        run.log_f.write(json.dumps({"step": first_step + k, **line}) + "\n")
    run.log_f.write(json.dumps(rec) + "\n")
    run.log_f.flush()
    log(rec)
    if val_acc > run.best_acc or epoch == 0:  # train.py:288-290; the reference's distillation cell keeps no checkpoint
        run.best_acc = max(run.best_acc, val_acc)
        torch.save(run.model.state_dict(), os.path.join(run.out_dir, "model_best.pt"))
    if run.ema and (rec["Accuracy/ValidationEMA"] > run.best_ema_acc or epoch == 0):
        run.best_ema_acc = max(run.best_ema_acc, rec["Accuracy/ValidationEMA"])
        torch.save(run.optimizer.ema_state_dict(run.model), os.path.join(run.out_dir, "model_ema_best.pt"))


def _run_epochs(run, step, books, validate, epochs, batch_hook, hook_after, log):
    """THE training loop.  Per step: the next batch from step.batches(); batch_hook("train", ...) in front of the step when the host
    knows the batch beforehand, or (hook_after: a resident loader feeds the step) after it with the buffers the step trained on;
    global_step counted between the two; step.run(batch, n) -> (loss, y_pred, img, label, *further loss terms); the books.  Per epoch
    _epoch_tail, then (checkpoint_every) the state's snapshot; at the end -- in a finally: a run that ends in an exception releases the
    seed word and finishes a pending write too -- the step, the session, the snapshot's writer and the log are closed, the "Training
    time" line written in front of that when the loop came through.  A run with a loaded state (resume) takes it in first and starts
    at the saved epoch.  -> (model, history)"""
    every = getattr(run, "checkpoint_every", None)
    done = False
    try:
        if getattr(run, "resume", None) is not None:
            _restore(run)
        for epoch in range(getattr(run, "start_epoch", 0), epochs):
            run.model.train()
            books.begin()
            first_step, steps = run.global_step, 0
            for batch in step.batches():
                n = run.global_step
                if batch_hook is not None and not hook_after:
                    batch_hook("train", n, batch[0], batch[1])
                run.global_step += 1
                loss, y_pred, img, label, *terms = step.run(batch, n)
                books.add(steps, y_pred, label, loss, *terms)
                if batch_hook is not None and hook_after:
                    batch_hook("train", n, img, label)
                steps += 1
                if steps >= run.epoch_steps:
                    break
            train = books.read(steps)
            run.model.eval()
            _epoch_tail(run, epoch, steps, first_step, train, validate, batch_hook, log)
            if every is not None and (epoch + 1) % every == 0 and run.rank == 0:
                _take_checkpoint(run, step, epoch + 1)
        done = True
    finally:
        try:
            step.close()
            if run.session is not None:
                run.session.close()
            if getattr(run, "snapshot", None) is not None:
                run.snapshot.close()   # a pending write is finished, and logged, first
        finally:
            if run.rank == 0:
                if done:
                    elapsed = getattr(run, "elapsed", 0.0) + time.perf_counter() - run.start
                    run.log_f.write(json.dumps({"Training time": elapsed}) + "\n")
                run.log_f.close()
    return run.model, run.history


def _plain_step(run, criterion, use_amp, graph, uint8_input, aug, loader, train_nhwc):
    """train()'s step: forward, criterion, backward, optimizer -- eager, or replayed by GraphedTrainStep / GraphedDPStep (built on the
    first batch, whose training step its warm-up is), with the loader's fetch as the graph's first node where the loader yields images"""
    host_aug = aug if loader is None or loader.output == "none" else None   # the transform the host still issues per batch
    loader_in_graph = loader is not None and graph and loader.img is not None   # the step fetches its own batch
    gstep = [None]

    def batches():
        if loader is not None:
            for _ in range(loader.steps_per_epoch):
                if loader_in_graph:
                    yield None, None
                    continue
                loader.fetch()
                yield loader.img if host_aug is None else host_aug(train_nhwc, loader.index, step=run.global_step), loader.labels
            return
        if aug is None:
            yield from run.train_set.batches(run.batch_size, True, run.gen, run.rank, run.world, raw_uint8=uint8_input)
            return
        for sel in run.train_set.index_batches(run.batch_size, True, run.gen, run.rank, run.world):
            yield aug(train_nhwc, sel, step=run.global_step), run.train_set.labels[sel]

    def run_step(batch, n):
        img, label = batch
        if not graph:
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=use_amp):
                y_pred = run.model(img)
            loss = criterion(y_pred, label.long())
            _eager_update(run, loss)
            return loss, y_pred, img, label
        if gstep[0] is None:   # built on the first batch (its shape is the captured one); warm-up steps are real training steps
            from spectre_vit.graph import GraphedDPStep, GraphedTrainStep
            cls = GraphedDPStep if run.world > 1 else GraphedTrainStep
            fed = dict(loader=loader) if loader_in_graph else {}
            gstep[0] = cls(run.model, run.optimizer, criterion, img, None if loader_in_graph else label.long(),
                           autocast_dtype=torch.bfloat16 if use_amp else None, warmup=1, **fed, **run.step_resume)
            loss, y_pred = gstep[0].warm_loss, gstep[0].warm_out   # the warm-up step WAS this batch's training step
        else:
            loss = gstep[0]() if loader_in_graph else gstep[0](img, label.long())   # loader_in_graph: ONE replay, fetch to optimizer
            y_pred = gstep[0].out
        if loader_in_graph:
            img, label = loader.img, loader.labels   # what the step just trained on
        return loss, y_pred, img, label
    return _step(batches, run_step, gstep)


def _early_distill_step(run, teacher):
    """train(distill=True)'s step: the teacher sees a 64 x 64 interpolation of the student's batch; eager, fp32 (train.py:299)"""
    def batches():
        return run.train_set.batches(run.batch_size, True, run.gen, run.rank, run.world)

    def run_step(batch, n):
        img, label = batch
        student_logits, _ = run.model(img, return_features=True)
        with torch.no_grad():
            teacher_logits, _ = teacher(nn.functional.interpolate(img, size=64, mode="bicubic"), return_features=True)
        loss, _, _ = distillation_loss(student_logits, teacher_logits, label.long())
        _eager_update(run, loss)
        return loss, student_logits, img, label
    return _step(batches, run_step, [None])


def train(config_path, mixer="permut", epochs=1, steps_per_epoch=None, batch_size=None, n_train=_UNSAID_TRAIN, n_val=_UNSAID_VAL,
          use_amp=True, distill=False, out_dir="runs/spectre_vit", log=print, uint8_input=False, graph=False, model="spectre",
          augment=False, batch_hook=None, graph_eval=False, lr_schedule=None, warmup_steps=0, eta_min=0.0, clip_grad_norm=None,
          skip_nonfinite=False, ema_decay=None, ema_warmup=False, device_meter=False, device_loader=False, accumulate_steps=None,
          optimizer=None, momentum=0.9, nesterov=True, checkpoint_every=None, resume=None, data_root=None, dataset=None,
          normalize=None):
    """graph=True (not with distill): the training step -- zero_grad, forward, loss, backward, AdamW -- is replayed from HIP graphs
    (spectre_vit.graph: one graph in a single process; as a rank of a torch.distributed job two graphs around ONE all-reduce of the
    flat gradient buffer) with the one-launch optimizer (spectre_vit.optim.FusedAdamW: torch.optim.AdamW's rule and state layout).
    The default is the reference's own loop shape (train.py:216-238) with the overlapped bucket exchange under data parallelism.
    augment=True: every training batch goes through the reference's transform chain (train.py:100-115) on the GPU -- the training set
    kept once as uint8 NHWC, the shuffled batch index, the global step and augment_seed(config seed, rank) handed to
    spectre_vit.augment.TrainAugment; validation batches stay ToTensor + Normalize (eval_transform_spectre).  With graph=True its
    launches (draw and apply; above the LDS kernel's size also the contrast mean's pre-pass) run on the step's stream in front of the replay
    (with device_loader=True they are inside the replay: below).  Not with uint8_input (the chain's output is float) or distill.
    batch_hook(kind, step, img, label), kind "train" / "val": called with every batch as the model is about to see it (test seam).
    graph_eval=True: the epoch's validation runs through one spectre_vit.inference.InferenceSession -- a graph replay per batch (buckets:
    the validation batch size and the tail rounded up to a multiple of 8), accuracy and loss accumulated on the device by its metrics
    kernel, one host read per epoch; the session takes the trained weights with refresh() after the epoch's training, with graph=True
    (weights updated through raw pointers) as with graph=False.
    lr_schedule="cosine" (with warmup_steps, eta_min), clip_grad_norm, skip_nonfinite: the optimizer's on-device step control
    (spectre_vit.optim: CosineSchedule over total_steps = steps per epoch * epochs as train.py:202-203, gradient clipping, a step with
    an inf / NaN gradient dropped as GradScaler does, train.py:236-238).  With any of them the optimizer is FusedAdamW(capturable=True)
    on the eager path too, and the epoch record gains "LR" (the last step's rate), "GradNorm" (the last step's) and "SkippedSteps".
    accumulate_steps=k: on-device gradient accumulation (FusedAdamW(accumulate_steps=k), part of the step control): every loader step
    is a micro-step and every k-th applies the optimizer to the window's mean gradient -- with graph=True from the same replayed graph.
    steps_per_epoch keeps counting micro-steps, the schedule's total_steps is (epochs * steps per epoch) // k, and a window may span
    an epoch boundary.  The record gains "AccumulateSteps" and "OptimizerSteps" (windows closed by the epoch's end); "LR" and
    "GradNorm" are the last boundary's.
    ema_decay (with ema_warmup): the optimizer keeps an exponential moving average of the weights inside its own launch
    (spectre_vit.optim.FusedAdamW(ema_decay=...), capturable=True on the eager path too).  After each epoch's validation a second pass
    runs on the averaged weights (inside optimizer.ema_weights(); through the same session with graph_eval=True) and the record gains
    "Accuracy/ValidationEMA" and "Loss/ValidationEMA"; model_ema_best.pt holds optimizer.ema_state_dict(model) of the best such epoch.
    Every other entry of the record is what it is without averaging.
    optimizer="adamw" | "adam" | "sgd" (with momentum, nesterov for "sgd"): the update rule -- the script's three optimizer lines,
    train.py:197-201.  lr, the betas and weight_decay come from the config for each; "adam" is spectre_vit.optim.FusedAdam and "sgd"
    FusedSGD(momentum=0.9, nesterov=True by default, the script's values) on every path, with all of the above unchanged in meaning.
    Left unsaid it is "adamw" as ever; said, the epoch record gains "Optimizer".
    device_meter=True (not with distill): the training criterion carries a spectre_vit.meter.TrainMeter of one log row per step of the
    epoch, so its loss launch -- eager or replayed -- counts the batch's hits and logs the step on the device: the host issues no
    argmax / == / sum / accumulate per step, reads the meter ONCE per epoch and resets it.  "Loss/Train" and "Accuracy/Train" (rank
    local, as without it) come from the meter, the record gains "Accuracy/TrainTop5", and scalars.jsonl gains one
    {"step", "Batch Loss/Train"} line per step (the reference's loss.item(), train.py:243).  Validation keeps a meter-less criterion.
    device_loader=True (not with distill): the training batches come from a spectre_vit.data.ResidentLoader over the resident uint8 set
    -- the epoch's permutation is computed on the device, one launch fetches a step's batch into fixed buffers -- instead of the host's
    randperm, slices, gathers and normalisation; with or without uint8_input.  Its steps per epoch are this loop's (min(per_pass,
    steps_per_epoch)), its seed loader_seed(config seed), its shard this rank's.  With graph=True the fetch is the first node of the
    step's graph, so a step is one replay and nothing else -- with augment=True too: the loader then fetches and augments in one
    launch (ResidentLoader(output="augment"): the table is keyed by the device cursor, which equals the global step, so the batches
    are the bits TrainAugment(...)(set, loader.index, step=global_step) yields), and for the sizes only the tiled chain takes (64 x 64
    ... 224 x 224 ... 512 x 512) in two (output="augment_tiled": fetch, draw and contrast pre-pass, then the tile kernel), the same
    bits again.  Only for the LDS border shape, which neither fused kernel serves with the whole-image chain's bits, the loader fetches
    index and labels alone and TrainAugment takes loader.index, draw and apply host-issued in front of the step (their step number is
    a by-value argument).
    The host then no longer knows a batch beforehand: batch_hook("train", step, img, label) is called AFTER the step, with the step's
    buffers (the loader's, or the augmented batch) -- valid until the next step overwrites them.  Validation is untouched.  The sample
    ORDER differs from the host randperm's (same distribution, another stream): hence a flag and not the default.
    checkpoint_every=E: after every E-th epoch's tail the run's whole state -- model.state_dict(), the optimizer's moments, step count,
    averages, control block and accumulators (an accumulation window may be open across the boundary), the loader's cursor, the graphed
    step's seed word -- is taken on the device by ONE launch (spectre_vit.checkpoint.StateSnapshot) and written to
    out_dir/train_state.pt behind the training's back, with the host's part: counters, history, best accuracies, RNG states.  A finished
    write is logged as a {"Checkpoint": ...} line; a non-finite weight or average keeps the old file ({"CheckpointSkipped": ...}).
    resume=True (out_dir/train_state.pt) or a path: the run is built as ever from the SAME arguments (the file's fingerprint is held
    against them, a ValueError names the first differing key), then continues the saved one bit for bit from its saved epoch.
    Single process only; model_best.pt / model_ema_best.pt stay what they are.  Left unsaid, nothing of a run changes.
    data_root=DIR (with dataset, normalize): train on the dataset files under DIR instead of the synthetic sets
    (spectre_vit.datasets.FileDataset: the CIFAR-100 / CIFAR-10 pickles, MNIST idx files or {train,test}.npz that torchvision or the
    user left there; no download).  dataset=None follows the config's file name (*cifar100*, *mnist*; anything else is refused),
    validation is the test split, n_train / n_val left unsaid are the whole splits and a number keeps the first samples (above the
    split's size it is refused).  The files are read and checked on the host before a device is touched: the config's img_size and
    in_channels must be the files', its num_classes at least the data's.  normalize: "reference" (the reference's constants:
    cifar100, mnist), "measured" (the train split's mean and population std from the ingest kernel's integer sums; the test split
    takes them too) or a (mean, std) pair; None is "reference" where there is one, else "measured".  The set's mean / std replace the
    CIFAR constants in the loader, the augmentation, validation and the model's uint8 patch gather, its resident NHWC copy serves
    where one was formed per run, and every path above works from files.  The fingerprint gains the dataset's name, digest and
    normalisation (a synthetic run's checkpoint, or other files', is refused by the first differing key) and the epoch record
    "Dataset": {name, root, n_train, n_val, digest, mean, std}.  Without data_root n_train / n_val are 4096 / 1024 as ever."""
    _check_device_meter(device_meter, distill)
    _check_device_loader(device_loader, distill)
    if augment and (uint8_input or distill):
        raise ValueError("augment=True yields normalised float batches for the plain training step: not with uint8_input or distill")
    ema = _ema_args(ema_decay, ema_warmup)
    optimizer_name, rule = _optimizer_choice(optimizer, momentum, nesterov)
    c = parse_config(config_path)
    if model == "spectre_branch" and uint8_input:
        raise ValueError("the SpectreBranch spectrum takes fp32 images: the uint8 NHWC input path is not built for it")
    if graph and distill:
        raise ValueError("graph=True replays the plain training step; the distillation step (teacher forward + KD loss) runs eagerly")
    data, n_train, n_val, data_fp = _data_args(c, config_path, data_root, dataset, normalize, n_train, n_val)
    fingerprint = _fingerprint("train", c, mixer=mixer, model=model, batch_size=batch_size, n_train=n_train, n_val=n_val,
                               steps_per_epoch=steps_per_epoch, epochs=epochs, use_amp=use_amp, graph=graph, augment=augment,
                               uint8_input=uint8_input, device_loader=device_loader, optimizer=optimizer, momentum=momentum,
                               nesterov=nesterov, lr_schedule=lr_schedule, warmup_steps=warmup_steps, eta_min=eta_min,
                               clip_grad_norm=clip_grad_norm, skip_nonfinite=skip_nonfinite, accumulate_steps=accumulate_steps,
                               ema_decay=ema_decay, ema_warmup=ema_warmup, distill=distill, **data_fp)
    checkpoint_every, resume = _checkpoint_args(checkpoint_every, resume, out_dir, fingerprint)
    run = _setup(c, mixer, model, epochs, steps_per_epoch, batch_size, n_train, n_val, out_dir, graph, device_meter, optimizer_name, rule,
                 ema, dict(lr_schedule=lr_schedule, warmup_steps=warmup_steps, eta_min=eta_min, clip_grad_norm=clip_grad_norm,
                           skip_nonfinite=skip_nonfinite, accumulate_steps=accumulate_steps), data)
    run.checkpoint_every, run.resume, run.fingerprint = checkpoint_every, resume, fingerprint
    amp = use_amp and not distill          # distill: use_amp False, train.py:299
    uint8 = uint8_input and not distill
    if distill:
        step = _early_distill_step(run, SyntheticTeacher(c.num_classes, 384, c.in_channels).to(run.device))
    else:
        # nn.CrossEntropyLoss() of train.py:196 on the HIP path (spectre_vit/loss.py); with a meter it logs every step it computes
        criterion = CrossEntropyLoss(**({} if run.meter is None else {"meter": run.meter}))
        aug = train_nhwc = loader = None
        if augment or device_loader:
            train_nhwc = run.train_set.nhwc()
        if augment:
            aug = TrainAugment(run.train_set.mean_values, run.train_set.std_values, seed=augment_seed(run.seed, run.rank))
        if device_loader:
            run.loader = loader = _resident_loader(run, train_nhwc, aug, uint8)
        step = _plain_step(run, criterion, amp, graph, uint8, aug, loader, train_nhwc)
    return _run_epochs(run, step, _TrainBooks(run, ("Batch Loss/Train",), block=False), _validator(run, graph_eval, amp, uint8), epochs,
                       batch_hook, device_loader, log)


def _teacher_cache(teacher, view, train_nhwc, classes, device, path, resize, crop, rank, world, batch_hook, batch_size, feature_dim=None,
                   data_tag=None):
    """train_distill's cached teacher: loaded from `path` when that file exists and was saved for this set size, class count and view;
    filled otherwise (every rank its share of the rows, then exchanged) and saved by rank 0.  -> (cache, the "TeacherCache" record)"""
    from spectre_vit.distillation import TeacherLogitCache
    n = train_nhwc.shape[0]
    tag = type(teacher).__name__ if data_tag is None else f"{type(teacher).__name__}@{data_tag}"   # files: the set's name and digest
    if path is not None and os.path.exists(path):
        wanted = {} if feature_dim is None else {"feature_dim": feature_dim}   # a file without features is refused by name then
        cache = TeacherLogitCache.load(path, device, n=n, classes=int(classes), resize=int(resize), crop=int(crop), tag=tag, **wanted)
        calls, loaded = 0, True
    else:
        cache = TeacherLogitCache(n, classes, device, **({} if feature_dim is None else {"feature_dim": feature_dim}))
        calls = cache.fill(teacher, view, train_nhwc, batch_size=batch_size, rank=rank, world=world, batch_hook=batch_hook)
        loaded = False
    if not cache.complete():
        raise RuntimeError("the teacher cache holds NaN rows after its fill: the teacher returned NaN, or rows were left out")
    if path is not None and not loaded and rank == 0:
        cache.save(path, resize=int(resize), crop=int(crop), tag=tag)
    return cache, {"rows": n, "teacher_batches": calls, "seconds": 0.0, "loaded": loaded}


def _paired_distill_step(run, criterion, use_amp, graph, aug, view, teacher, cache, loader, train_nhwc, batch_hook):
    """train_distill()'s step: ONE index seen twice -- the student's view and, uncached, the teacher's view and forward (the "teacher"
    hook in front of it) -- then the fused DistillationLoss, eager or replayed by GraphedDistillStep (built on the first batch, whose
    training step its warm-up is).  A criterion with a non-zero feature_loss_weight also gets both models' features (the cache's, when
    cached).  -> (loss, y_pred, img, label, soft, ce[, feat])"""
    featured = criterion.feature_loss_weight != 0.0
    loader_step = loader is not None and graph and loader.img is not None       # the graphed step reads the loader's buffers
    loader_in_graph = loader_step and cache is not None                         # ... and fetches them itself: a step is one replay
    autocast_dtype = torch.bfloat16 if use_amp else None
    train_set = run.train_set
    gstep = [None]

    def index_batches():
        if loader is None:
            yield from train_set.index_batches(run.batch_size, True, run.gen, run.rank, run.world)
            return
        for _ in range(loader.steps_per_epoch):
            if loader_in_graph:
                yield None
                continue
            loader.fetch()
            yield loader.index

    def batches():
        for sel in index_batches():
            if loader_in_graph:
                img = label = None   # the replay fetches them
            elif loader is not None:
                label = loader.labels
                img = loader.img if loader.img is not None else aug(train_nhwc, sel, step=run.global_step)
            else:
                label = train_set.labels[sel]
                if aug is not None:
                    img = aug(train_nhwc, sel, step=run.global_step)
                else:
                    img = (train_set.images[sel].float() / 255.0 - train_set.mean) / train_set.std
            yield img, label, sel, view(train_nhwc, sel) if cache is None else None

    def run_step(batch, n):
        img, label, sel, img_teacher = batch
        if cache is None:
            if batch_hook is not None:
                batch_hook("teacher", n, img_teacher, label)
            with torch.no_grad():   # train.py:326-327
                teacher_logits, teacher_feat = teacher(img_teacher, return_features=True)
            teacher_logits = teacher_logits.float()
        if not graph:
            feats = {}
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=use_amp):
                if featured:   # train.py:325
                    y_pred, student_feat = run.model(img, return_features=True)
                    feats = dict(student_feat=student_feat, teacher_feat=teacher_feat if cache is None else cache.features)
                else:
                    y_pred = run.model(img)
            if cache is None:
                loss = criterion(y_pred.float(), teacher_logits, label.long(), **feats)
            else:
                loss = criterion(y_pred.float(), cache, label.long(), index=sel, **feats)
            terms = (criterion.soft, criterion.ce) + ((criterion.feat,) if featured else ())
            _eager_update(run, loss)
            return (loss, y_pred, img, label) + terms
        if gstep[0] is None:   # built on the first batch; its warm-up step WAS this batch's training step
            from spectre_vit.graph import GraphedDistillStep
            fed = dict(example_teacher_feat=teacher_feat) if featured and cache is None else {}
            if loader_step:   # the batch (and, cached, its index) are the loader's buffers
                teacher_args = dict(example_teacher_logits=teacher_logits, **fed) if cache is None else dict(teacher_cache=cache)
                g = GraphedDistillStep(run.model, run.optimizer, criterion, None, None, autocast_dtype=autocast_dtype, warmup=1,
                                       loader=loader, **teacher_args, **run.step_resume)
            else:
                teacher_args = dict(example_teacher_logits=teacher_logits, **fed) if cache is None else dict(teacher_cache=cache, example_index=sel)
                g = GraphedDistillStep(run.model, run.optimizer, criterion, img, label.long(), autocast_dtype=autocast_dtype, warmup=1,
                                       **teacher_args, **run.step_resume)
            gstep[0] = g
            loss, soft, ce, feat, y_pred = g.warm_loss, g.warm_soft, g.warm_ce, g.warm_feat, g.warm_out
        else:
            g = gstep[0]
            fed = dict(teacher_feat=teacher_feat) if featured and cache is None else {}
            if loader_in_graph:
                loss = g()   # ONE replay: fetch, forward, cached loss, backward, optimizer
            elif loader_step:
                loss = g(teacher_logits=teacher_logits, **fed)
            else:
                loss = g(img, label.long(), teacher_logits, **fed) if cache is None else g(img, label.long(), index=sel)
            soft, ce, feat, y_pred = g.soft, g.ce, g.feat, g.out
        if loader_in_graph:
            img, label = loader.img, loader.labels   # what the step just trained on
        return (loss, y_pred, img, label, soft, ce) + ((feat,) if featured else ())
    return _step(batches, run_step, gstep)


def train_distill(config_path, mixer="permut", epochs=1, steps_per_epoch=None, batch_size=None, n_train=_UNSAID_TRAIN, n_val=_UNSAID_VAL,
                  use_amp=False, graph=False, augment=True, teacher=None, T=2.0, soft_target_loss_weight=0.25, ce_loss_weight=0.75,
                  resize=256, crop=224, out_dir="runs/spectre_vit_distill", log=print, batch_hook=None, graph_eval=False,
                  lr_schedule=None, warmup_steps=0, eta_min=0.0, clip_grad_norm=None, skip_nonfinite=False, ema_decay=None,
                  ema_warmup=False, device_meter=False, device_loader=False, accumulate_steps=None, optimizer=None, momentum=0.9,
                  nesterov=True, feature_loss_weight=0.0, checkpoint_every=None, resume=None, data_root=None, dataset=None,
                  normalize=None, cache_teacher=False, teacher_cache_path=None):
    """The distillation loop of reference train.py:298-396 with its data contract (DistillationDatasetCls, train.py:139-141): every
    batch is ONE shuffled index into the resident uint8 set, seen twice -- the student's view through the training transform chain
    (spectre_vit.augment.TrainAugment; augment=False: ToTensor + Normalize) and the teacher's view through
    spectre_vit.distillation.TeacherView (Resize(resize, BICUBIC) -> CenterCrop(crop) -> ToTensor -> Normalize of the raw 8-bit image).
    The teacher (None: SyntheticTeacher; any module with forward(x, return_features=True)) runs under no_grad; the student's step goes
    through the fused DistillationLoss, eagerly with GradReducer (also as a rank of a torch.distributed job) or, graph=True, replayed
    by spectre_vit.graph.GraphedDistillStep with FusedAdamW (single process).  use_amp=False as the reference's distillation cell
    (train.py:299); True runs the student under bf16 autocast, the loss on its fp32 logits.  Validation: student only, CE only, every
    sample (train.py:365-383).  The three per-batch losses the reference logs (train.py:355-359) are kept on the device and written
    once per epoch as {"step", "Batch Loss/Train", "Batch Loss/Dist", "Batch Loss/CE"} lines: no host synchronisation per step.
    batch_hook(kind, step, img, label), kind "train" / "teacher" / "val" (test seam).  graph_eval, lr_schedule, warmup_steps, eta_min,
    clip_grad_norm, skip_nonfinite, ema_decay, ema_warmup, accumulate_steps, optimizer, momentum, nesterov: as in train() (the
    distillation cell's own optimizer line is the Adam one, train.py:307).
    cache_teacher=True: the teacher's view has no random op and the teacher is frozen, so its logits are a function of the sample alone;
    they are computed once before epoch 0 into a resident spectre_vit.distillation.TeacherLogitCache (sharded over the ranks; loaded from
    teacher_cache_path when that file exists and matches, saved there by rank 0 otherwise), a {"TeacherCache": ...} line is logged, and
    the epochs call neither the view nor the teacher: the loss reads the cache through the batch's index (no "teacher" hook then; the
    fill calls batch_hook("teacher_fill", block, img_teacher, index)).  Eager, as a data-parallel rank, and graph=True.
    device_meter=True: as in train() -- the DistillationLoss carries a TrainMeter, the host issues no per-step stack / argmax / == / sum
    / accumulate, and the epoch's "Loss/Train", "Accuracy/Train", "Accuracy/TrainTop5" and the three per-batch loss lines come from
    ONE read of the meter (its log rows hold each step's loss, soft and CE terms).
    device_loader=True: as in train() -- the batches come from a spectre_vit.data.ResidentLoader (seed loader_seed(config seed), this
    rank's shard, this loop's steps per epoch) whose output is picked by shape: "augment" / "augment_tiled" fetch and augment in one
    call, "float" with augment=False; the one LDS border shape fetches index and labels alone and TrainAugment takes loader.index.
    The loader's index serves the teacher's view and the cached loss directly.  With graph=True and cache_teacher=True the step is
    GraphedDistillStep(loader=..., teacher_cache=...): the fetch is the graph's first node, the loss reads the cache through
    loader.index, and a step is ONE replay with nothing host-issued in front of it.  Uncached, the teacher needs the index first: the
    host fetches, runs the view and the teacher, and replays a graph that reads the loader's buffers.  The global step, the
    augmentation's step and the loader's cursor stay equal.  batch_hook("train", step, img, label) is called AFTER the step with the
    step's buffers (valid until the next fetch); the "teacher" hook keeps its place in front of the teacher.  The sample order is the
    loader's, not the host randperm's.
    feature_loss_weight=W (0.0: off, and the record and the launches are those of a run without the argument): the feature-matching
    term of train.py:306, 343-346 -- W * (1 - mean cos(student CLS features, teacher CLS features)) -- joins the loss
    (DistillationLoss(feature_loss_weight=W): one more launch each way).  Both models are asked for their features (train.py:325-327);
    teacher=None builds the SyntheticTeacher with the student's embed_dim as its feature width, a teacher of another width is refused
    before the first step (project inside the teacher module).  With cache_teacher=True the cache keeps the teacher's features too
    (TeacherLogitCache(feature_dim=...)) and the term reads them through the batch's index, so the graphed, cached, loader-fed step
    stays one replay.  The epoch record gains "Loss/Feat" and the per-step lines "Batch Loss/Feat", from the same per-epoch device
    buffer as the other three.  Not with device_meter=True (the meter's log row has no slot for a fourth term).  Eager, graph=True,
    cache_teacher, device_loader, and as an eager data-parallel rank.
    checkpoint_every, resume: as in train().  The teacher, its view and its cache are no part of the state: a resumed run builds (or
    loads) them as ever, before the saved state is taken in.
    data_root, dataset, normalize: as in train().  The teacher's view takes the set's resident NHWC copy and its mean / std, and the
    teacher cache's meta tag carries the dataset's name and digest: a cache filled from other data is refused by name."""
    from spectre_vit import _native
    _check_device_meter(device_meter)
    _check_device_loader(device_loader)
    ema = _ema_args(ema_decay, ema_warmup)
    optimizer_name, rule = _optimizer_choice(optimizer, momentum, nesterov)
    c = parse_config(config_path)
    if teacher_cache_path is not None and not cache_teacher:
        raise ValueError("teacher_cache_path names the file of the cached teacher's logits: it needs cache_teacher=True")
    if graph and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError("graph=True replays the single-process distillation step (GraphedDistillStep); a data-parallel rank runs it eagerly")
    if not _native.call("spv_teacher_view_supported", int(c.in_channels), int(c.img_size), int(resize), int(crop)):
        raise ValueError(f"the teacher view kernel does not take {c.in_channels} x {c.img_size} x {c.img_size} images at resize={resize}, "
                         f"crop={crop} (1 or 3 channels, img_size <= resize, 0 < crop <= resize, four taps inside the image)")
    if not (T > 0):
        raise ValueError(f"temperature T={T} must be positive")
    if isinstance(feature_loss_weight, bool) or not isinstance(feature_loss_weight, (int, float)) \
            or not math.isfinite(feature_loss_weight) or feature_loss_weight < 0:
        raise ValueError(f"feature_loss_weight={feature_loss_weight!r} must be a finite number >= 0")
    featured = feature_loss_weight != 0
    if featured and device_meter:
        raise ValueError(f"feature_loss_weight={feature_loss_weight} with device_meter=True: the meter's log row holds loss, soft and CE "
                         "and has no slot for the feature term")
    data, n_train, n_val, data_fp = _data_args(c, config_path, data_root, dataset, normalize, n_train, n_val)
    fingerprint = _fingerprint("train_distill", c, mixer=mixer, batch_size=batch_size, n_train=n_train, n_val=n_val,
                               steps_per_epoch=steps_per_epoch, epochs=epochs, use_amp=use_amp, graph=graph, augment=augment,
                               device_loader=device_loader, optimizer=optimizer, momentum=momentum, nesterov=nesterov,
                               lr_schedule=lr_schedule, warmup_steps=warmup_steps, eta_min=eta_min, clip_grad_norm=clip_grad_norm,
                               skip_nonfinite=skip_nonfinite, accumulate_steps=accumulate_steps, ema_decay=ema_decay,
                               ema_warmup=ema_warmup, teacher=None if teacher is None else type(teacher).__name__, T=T,
                               soft_target_loss_weight=soft_target_loss_weight, ce_loss_weight=ce_loss_weight, resize=resize, crop=crop,
                               feature_loss_weight=feature_loss_weight, cache_teacher=cache_teacher, **data_fp)
    checkpoint_every, resume = _checkpoint_args(checkpoint_every, resume, out_dir, fingerprint)
    run = _setup(c, mixer, "spectre", epochs, steps_per_epoch, batch_size, n_train, n_val, out_dir, graph, device_meter, optimizer_name, rule,
                 ema, dict(lr_schedule=lr_schedule, warmup_steps=warmup_steps, eta_min=eta_min, clip_grad_norm=clip_grad_norm,
                           skip_nonfinite=skip_nonfinite, accumulate_steps=accumulate_steps), data)
    run.checkpoint_every, run.resume, run.fingerprint = checkpoint_every, resume, fingerprint
    train_nhwc = run.train_set.nhwc()
    mean, std = run.train_set.mean_values, run.train_set.std_values
    aug = TrainAugment(mean, std, seed=augment_seed(run.seed, run.rank)) if augment else None
    view = TeacherView(mean, std, resize=resize, crop=crop)
    if teacher is None:   # with the feature term the stand-in's features have the student's width
        teacher = SyntheticTeacher(c.num_classes, int(c.embed_dim) if featured else 384, c.in_channels).to(run.device)
    teacher.eval()
    criterion = DistillationLoss(T, soft_target_loss_weight, ce_loss_weight, **({} if run.meter is None else {"meter": run.meter}),
                                 **({"feature_loss_weight": float(feature_loss_weight)} if featured else {}))
    if featured:   # a teacher of another feature width is refused here, before the first step and before the cache's fill
        with torch.no_grad():
            probe = teacher(view(train_nhwc, torch.zeros(1, dtype=torch.int64, device=run.device)), return_features=True)[1]
        if probe.dim() != 2 or probe.shape[1] != int(c.embed_dim):
            raise ValueError(f"feature_loss_weight={feature_loss_weight}: the teacher's features {tuple(probe.shape)} and the student's "
                             f"(width embed_dim={c.embed_dim}) differ in width; project inside the teacher module (there is no learned "
                             "projector in this loss)")
    cache = None
    if cache_teacher:
        # filled in blocks of the training batch: the teacher then sees the batch shape it would see inside the epochs
        cache, cache_rec = _teacher_cache(teacher, view, train_nhwc, c.num_classes, run.device, teacher_cache_path, resize, crop, run.rank,
                                          run.world, batch_hook, run.batch_size, int(c.embed_dim) if featured else None,
                                          None if data is None else f"{data.name}:{data.train.digest}")
        cache_rec["seconds"] = time.perf_counter() - run.start
        if run.rank == 0:
            run.log_f.write(json.dumps({"TeacherCache": cache_rec}) + "\n")
            run.log_f.flush()
    run.loader = loader = _resident_loader(run, train_nhwc, aug, False) if device_loader else None
    step = _paired_distill_step(run, criterion, use_amp, graph, aug, view, teacher, cache, loader, train_nhwc, batch_hook)
    names = ("Batch Loss/Train", "Batch Loss/Dist", "Batch Loss/CE") + (("Batch Loss/Feat",) if featured else ())
    return _run_epochs(run, step, _TrainBooks(run, names, block=True),
                       _validator(run, graph_eval, use_amp, float_logits=True), epochs, batch_hook, device_loader, log)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="spectre_vit/configs/spectre_vit_cifar100.py")
    ap.add_argument("--mixer", default="permut")
    ap.add_argument("--model", default="spectre", choices=("spectre", "spectre_branch"),
                    help="spectre: SpectreViT (with --mixer); spectre_branch: SpectreBranch (spectre_branch.py)")
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--steps-per-epoch", type=int, default=None)
    ap.add_argument("--batch-size", type=int, default=None)
    ap.add_argument("--distill", action="store_true")
    ap.add_argument("--graph", action="store_true", help="replay the training step from HIP graphs (spectre_vit.graph)")
    ap.add_argument("--augment", action="store_true",
                    help="the reference's training transform chain (train.py:100-115) on the GPU (spectre_vit.augment)")
    ap.add_argument("--distill-paired", action="store_true",
                    help="the reference's distillation loop with its two views per sample (train_distill): the student's augmented view "
                         "and the teacher's Resize(256) -> CenterCrop(224) view, fused KD loss; with --graph, --no-augment")
    ap.add_argument("--no-augment", action="store_true", help="--distill-paired: the student's view is ToTensor + Normalize only")
    ap.add_argument("--cache-teacher", action="store_true",
                    help="--distill-paired: compute the frozen teacher's logits of every sample once, keep them on the GPU and read them "
                         "by index (no teacher view and no teacher forward inside the epochs)")
    ap.add_argument("--teacher-cache", default=None, metavar="PATH",
                    help="--cache-teacher: load the logits from PATH when it exists and matches, save them there otherwise")
    ap.add_argument("--feature-loss-weight", type=float, default=0.0, metavar="W",
                    help="--distill-paired: add W * (1 - mean cosine of the student's and the teacher's CLS features), the reference's "
                         "feature-matching term (train.py:343-346); with --cache-teacher the features are cached too; not with "
                         "--device-meter")
    ap.add_argument("--graph-eval", action="store_true",
                    help="validate through a graph-replayed InferenceSession with on-device metrics (spectre_vit.inference)")
    ap.add_argument("--lr-schedule", default=None, choices=("cosine",),
                    help="cosine annealing over steps-per-epoch * epochs steps (train.py:202-203), evaluated on the device every step")
    ap.add_argument("--warmup-steps", type=int, default=0, help="--lr-schedule cosine: linear warm-up steps in front of the cosine")
    ap.add_argument("--eta-min", type=float, default=0.0, help="--lr-schedule cosine: the rate the schedule ends at")
    ap.add_argument("--clip-grad-norm", type=float, default=None, help="clip the global gradient norm (on the device, inside the optimizer step)")
    ap.add_argument("--skip-nonfinite", action="store_true", help="drop a step whose gradients hold an inf or a NaN (GradScaler's rule)")
    ap.add_argument("--accumulate-steps", type=int, default=None, metavar="K",
                    help="accumulate the gradients of K steps on the device and apply the optimizer to their mean on every K-th; "
                         "--steps-per-epoch keeps counting micro-steps and the schedule runs over (epochs * steps) // K optimizer steps")
    ap.add_argument("--optimizer", default=None, choices=("adamw", "adam", "sgd"),
                    help="the update rule: the script's three optimizer lines (train.py:197-201); lr, betas and weight decay from the config")
    ap.add_argument("--momentum", type=float, default=0.9, help="--optimizer sgd: the momentum (the script's 0.9)")
    ap.add_argument("--no-nesterov", action="store_true", help="--optimizer sgd: plain momentum where the script's line has nesterov=True")
    ap.add_argument("--ema-decay", type=float, default=None,
                    help="keep an exponential moving average of the weights inside the optimizer launch, validate it after every epoch "
                         "and save model_ema_best.pt")
    ap.add_argument("--ema-warmup", action="store_true", help="--ema-decay: the decay warms up as min(decay, (1 + step) / (10 + step))")
    ap.add_argument("--device-meter", action="store_true",
                    help="keep the training loss / accuracy books on the device inside the loss launch (spectre_vit.meter.TrainMeter): "
                         "no host-issued argmax / == / sum / accumulate per step, one read per epoch, per-step loss lines")
    ap.add_argument("--device-loader", action="store_true",
                    help="fetch the shuffled training batches on the GPU (spectre_vit.data.ResidentLoader), with --augment augmented in "
                         "the same call (LDS sizes: one launch; 64 x 64 .. 512 x 512: two): with --graph a step is one replay with no "
                         "host-issued work in front of it; also with --distill-paired (there one replay with --graph --cache-teacher; "
                         "uncached the teacher runs between the fetch and the replay); the sample order differs from the host "
                         "randperm's")
    ap.add_argument("--checkpoint-every", type=int, default=None, metavar="E",
                    help="after every E-th epoch take the run's whole state on the GPU in one launch and write OUT/train_state.pt behind "
                         "the training's back (spectre_vit.checkpoint); single process")
    ap.add_argument("--resume", nargs="?", const=True, default=None, metavar="PATH",
                    help="continue the run saved in PATH (left out: OUT/train_state.pt) bit for bit; every other argument as in the "
                         "saved run")
    ap.add_argument("--data-root", default=None, metavar="DIR",
                    help="train on the dataset files under DIR (what torchvision leaves in ./data: cifar-100-python/, "
                         "cifar-10-batches-py/, MNIST/raw/, or {train,test}.npz) instead of the synthetic set; validation is the test split")
    ap.add_argument("--dataset", default=None, choices=("cifar100", "cifar10", "mnist", "npz"),
                    help="--data-root: the files' format; left out it follows the config's file name (*cifar100*, *mnist*)")
    ap.add_argument("--normalize", default=None, choices=("reference", "measured"),
                    help="--data-root: the reference's constants (cifar100, mnist) or the train split's measured mean and std")
    ap.add_argument("--out", default="runs/spectre_vit")
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    common = dict(mixer=a.mixer, epochs=a.epochs, steps_per_epoch=a.steps_per_epoch, batch_size=a.batch_size, out_dir=a.out, graph=a.graph,
                  graph_eval=a.graph_eval, device_meter=a.device_meter, device_loader=a.device_loader, lr_schedule=a.lr_schedule,
                  warmup_steps=a.warmup_steps, eta_min=a.eta_min, clip_grad_norm=a.clip_grad_norm, skip_nonfinite=a.skip_nonfinite,
                  ema_decay=a.ema_decay, ema_warmup=a.ema_warmup, accumulate_steps=a.accumulate_steps, optimizer=a.optimizer,
                  momentum=a.momentum, nesterov=not a.no_nesterov, checkpoint_every=a.checkpoint_every, resume=a.resume,
                  data_root=a.data_root, dataset=a.dataset, normalize=a.normalize)
    if a.distill_paired:
        train_distill(a.config, augment=not a.no_augment, cache_teacher=a.cache_teacher, teacher_cache_path=a.teacher_cache,
                      feature_loss_weight=a.feature_loss_weight, **common)
        return
    train(a.config, distill=a.distill, model=a.model, augment=a.augment, **common)


if __name__ == "__main__":
    main()
