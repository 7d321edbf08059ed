"""harness.train(mixer="filter") end to end: a graphed two-epoch run on the resident loader with a checkpoint after every epoch,
interrupted at the first step of epoch 2 and resumed, ends on the uninterrupted run's bits in every state_dict entry -- the filters
included, which the optimizer, the checkpoint and the resume all reach through named_parameters alone.  The configuration is the
smallest one of tests/test_gpu_resume.py."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = "spectre_vit/configs/spectre_vit_mnist.py"
EPOCHS, STEPS, N_TRAIN, BATCH = 2, 4, 64, 16


class Preempted(Exception):
    pass


def _train(out, hook=None, **more):
    from spectre_vit import harness
    model, history = harness.train(CFG, mixer="filter", n_train=N_TRAIN, n_val=40, batch_size=BATCH, steps_per_epoch=STEPS, epochs=EPOCHS,
                                   out_dir=out, log=lambda r: None, batch_hook=hook, graph=True, device_loader=True, checkpoint_every=1, **more)
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in model.state_dict().items()}, history


def test_filter_run_resumes_on_the_uninterrupted_runs_bits(tmp_path):
    whole, whole_history = _train(str(tmp_path / "whole"))
    filters = [k for k in whole if k.endswith("mix_layer.complex_weight")]
    assert filters and all(whole[k].dtype == torch.float32 and bool(torch.isfinite(whole[k]).all()) for k in filters)

    def cut(kind, step, img, label):
        if kind == "train" and step == STEPS:
            raise Preempted
    with pytest.raises(Preempted):
        _train(str(tmp_path / "cut"), cut)
    from spectre_vit.checkpoint import FILE_NAME, load_train_state
    saved = load_train_state(os.path.join(str(tmp_path / "cut"), FILE_NAME))
    assert saved["host"]["epoch"] == 1 and {"model/" + k for k in filters} <= set(saved["tensors"])
    # training moved the filters before the cut, and moves them again after it
    assert any(not torch.equal(saved["tensors"]["model/" + k].cpu(), whole[k].cpu()) for k in filters)
    resumed, resumed_history = _train(str(tmp_path / "cut"), resume=True)
    assert sorted(resumed) == sorted(whole) and resumed_history == whole_history
    for k in whole:
        a, b = whole[k].cpu().contiguous().reshape(-1), resumed[k].cpu().contiguous().reshape(-1)
        assert a.dtype == b.dtype and a.view(torch.uint8).equal(b.view(torch.uint8)), k
