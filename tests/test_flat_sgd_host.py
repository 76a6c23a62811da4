"""CPU checks of the flat-buffer SGD state every trainer shares (flat_sgd.FlatSGD), built on
CPU models: the two stage-1 parameter groups against the reference optimizer's, the aliasing
of the Parameters and their gradients, the gradient buffer's tail slots, and the train-mode
engine cache of STDClassifier."""
import pytest
import torch

from tcam_wsol_video_amd import cl_training as CT
from tcam_wsol_video_amd.checkpoints import reference_param_groups
from tcam_wsol_video_amd.flat_sgd import FlatSGD
from tcam_wsol_video_amd.models import build_r50_stdcl, build_stdcl
from tcam_wsol_video_amd.vgg_training import VGG16ClassifierTrainer

BUILD = {"resnet50": lambda: build_r50_stdcl(seed=0), "vgg16": lambda: build_stdcl("vgg16", seed=0)}


@pytest.fixture(scope="module", params=sorted(BUILD))
def built(request):
    """(encoder name, CPU model, its trainer class's group boundary), built once: a test
    that re-points the Parameters into a flat buffer of its own leaves the model usable for
    the next one (the values move along)."""
    model = BUILD[request.param]()
    return request.param, model, CT.classifier_trainer_class(request.param).param_split(model)


def test_group_boundary_is_the_reference_optimizers(built):
    name, model, split = built
    g0, g1 = reference_param_groups(model)
    numel = {n: p.numel() for n, p in model.named_parameters()}
    assert list(numel) == g0 + g1                  # group 1 is the tail of the flat order
    assert split == sum(numel[n] for n in g0)
    assert sum(numel.values()) - split == sum(numel[n] for n in g1)
    assert g0 and g1
    if name == "vgg16":
        assert [len(g0), len(g1)] == [26, 4]


@pytest.mark.parametrize("amp", [False, True])
def test_flat_state_aliasing_and_tail_slots(built, amp):
    _, model, split = built
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    fs = FlatSGD(list(model.parameters()), [split], amp=amp, init_scale=2.0 ** 10)
    n = sum(p.numel() for p in model.parameters())
    assert fs.flat.numel() == fs.mom.numel() == fs.grad.numel() == n and fs.bounds == [split]
    off = 0
    for p in fs.params:
        assert p.data_ptr() == fs.flat.data_ptr() + 4 * off
        g = fs.g(p)
        assert g.shape == p.shape and g.data_ptr() == fs.grad.data_ptr() + 4 * off
        off += p.numel()
    assert off == n
    for k, v in model.state_dict().items():        # the copy into the flat buffer is exact
        assert torch.equal(v, sd[k]), k
    # the gradient buffer's tail: the loss gate, then AMP's found_inf
    assert fs.grad.data_ptr() == fs._gbuf.data_ptr()
    assert fs.loss_gate.data_ptr() == fs._gbuf.data_ptr() + 4 * n and fs.loss_gate.numel() == 1
    if amp:
        assert fs._gbuf.numel() == n + 2
        assert fs.found_inf.data_ptr() == fs._gbuf.data_ptr() + 4 * (n + 1)
        assert fs.found_inf.numel() == 1
    else:
        assert fs._gbuf.numel() == n + 1 and fs.found_inf is None
    fs.loss_gate.fill_(3.0)
    assert fs._gbuf[n].item() == 3.0 and not fs.grad.any()
    # the tail group carries the real scaler state and counters, the first one shadows
    assert len(fs._group_state) == 2
    sc, tr, cnt = fs._group_state[1]
    assert sc is fs.scale and tr is fs.growth_tracker and cnt is fs.step_counts
    assert fs._group_state[0][0].item() == fs.scale.item() == 2.0 ** 10
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(*fs._group_state))
    assert fs.applied_steps == 0 and fs.skipped_steps == 0 and fs.steps == 0
    assert not fs.bns and fs.bn_flat.numel() == 0      # no BatchNorm handed over
    # a Parameter whose .data was replaced breaks the aliasing
    assert fs.views_intact()
    v0 = fs.param_version()
    p = fs.params[3]
    p.data = p.data.clone()
    assert not fs.views_intact()
    assert fs.param_version() == v0


def test_one_group_and_bad_boundaries():
    ps = [torch.nn.Parameter(torch.arange(6.).view(2, 3)), torch.nn.Parameter(torch.ones(4))]
    fs = FlatSGD(ps)
    assert fs.bounds == [] and len(fs._group_state) == 1
    assert fs._group_state[0] == (fs.scale, fs.growth_tracker, fs.step_counts)
    assert fs.flat.tolist() == [0., 1., 2., 3., 4., 5., 1., 1., 1., 1.]
    with pytest.raises(ValueError, match="boundaries"):
        FlatSGD(ps, [11])


def test_engine_cached_for_one_encoder_is_not_reused_for_the_other(built):
    """train_forward rebuilds the engine when the cached one is not the model's own trainer
    class: on a CPU model the rebuild is refused ("HIP path") before a device is touched,
    where reusing the foreign engine would have run its forward."""
    name, model, _ = built
    eng = object.__new__({"vgg16": CT.ClassifierTrainer, "resnet50": VGG16ClassifierTrainer}[name])
    assert not isinstance(eng, CT.classifier_trainer_class(model.encoder_name))
    model.__dict__["_train_engine"] = eng
    try:
        with pytest.raises(RuntimeError, match="HIP path"):
            CT.train_forward(model, torch.zeros(1, 3, 32, 32))
        assert model.__dict__["_train_engine"] is eng     # nothing was built
    finally:
        del model.__dict__["_train_engine"]


def test_no_trainer_borrows_another_classes_methods():
    """A method two trainers share is inherited from a common base, never assigned across
    (``name = OtherClass.name`` in a class body)."""
    from tcam_wsol_video_amd.training import DecoderTrainer
    classes = (CT.ClassifierTrainer, VGG16ClassifierTrainer, CT.Stage1Trainer, DecoderTrainer,
               FlatSGD)
    for cls in classes:
        for k, v in vars(cls).items():
            if callable(v) or isinstance(v, property):
                owners = [o.__name__ for o in classes if vars(o).get(k) is v]
                assert owners == [cls.__name__], (k, owners)
