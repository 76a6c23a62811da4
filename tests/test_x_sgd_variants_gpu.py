"""tcam_sgd_step, tcam_sgd_step_gated and tcam_sgd_step_amp against each other, through the C
ABI: the three entries apply one update, so from the same start an applied step leaves the same
bits in p and buf whichever entry ran it, and a skipped step leaves every bit where it was.
tests/test_grad_chain_gpu.py holds each entry against the fp64 step; nothing there ties the
three to each other.

n = 1 one thread; 255 / 256 / 257 either side of one 256-thread block; 1000 a ragged last
block.  The points cover momentum 0 / 0.9, nesterov, weight decay, dampening (without nesterov,
as torch.optim.SGD requires) and grad_scale 1 / 0.5."""
import pytest
import torch

from tcam_wsol_video_amd import _lib
from test_gpu_enc_train import _st

pytestmark = pytest.mark.gpu

NS = [1, 255, 256, 257, 1000]
LR = 0.05
# (momentum, dampening, weight_decay, nesterov, grad_scale)
POINTS = [(0.0, 0.0, 0.0, 0, 1.0), (0.0, 0.0, 1e-4, 0, 0.5), (0.9, 0.0, 0.0, 0, 1.0),
          (0.9, 0.0, 1e-4, 1, 1.0), (0.9, 0.1, 0.0, 0, 0.5), (0.9, 0.1, 1e-4, 0, 1.0),
          (0.9, 0.0, 0.0, 1, 0.5), (0.9, 0.0, 1e-4, 0, 0.5)]
INF, NAN = float("inf"), float("nan")


def _bits(t):
    return t.view(torch.int32)


def _i32(cuda, v):
    return torch.tensor([v], dtype=torch.int32, device=cuda)


def _start(cuda, n, seed, buf_fill):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g).to(cuda)
    buf = torch.full((n,), buf_fill, device=cuda)   # stale: the first step must not read it
    grads = [(torch.randn(n, generator=g) * s).to(cuda) for s in (1.0, 1e-3)]
    return p, buf, grads


class _Run:
    """One entry's own copy of the state and its counters."""

    def __init__(self, cuda, kind, p, buf, steps=0):
        self.kind, self.p, self.buf = kind, p.clone(), buf.clone()
        self.n = p.numel()
        self.steps, self.skipped = _i32(cuda, steps), _i32(cuda, 0)
        self.scale = torch.tensor([1024.0], device=cuda)
        self.tracker = _i32(cuda, 1)

    def step(self, g, cfg, gate=None, first=0, scaler=(2.0, 0.5, 1000)):
        lib = _lib.load()
        m, damp, wd, nest, gs = cfg
        head = (self.p.data_ptr(), g.data_ptr(), self.buf.data_ptr(), self.n, LR, m, damp, wd,
                nest)
        if self.kind == "plain":
            rc = lib.tcam_sgd_step(*head, first, gs, _st())
        elif self.kind == "gated":
            rc = lib.tcam_sgd_step_gated(*head, gs, gate.data_ptr(), self.steps.data_ptr(),
                                         self.skipped.data_ptr(), _st())
        else:
            rc = lib.tcam_sgd_step_amp(*head, gs, gate.data_ptr(), self.steps.data_ptr(),
                                       self.skipped.data_ptr(), self.scale.data_ptr(),
                                       self.tracker.data_ptr(), *scaler, _st())
        assert rc == 0


@pytest.mark.parametrize("cfg", POINTS, ids=lambda c: "-".join(f"{v:g}" for v in c))
@pytest.mark.parametrize("n", NS)
def test_three_entries_apply_the_same_step(cuda, n, cfg):
    """Two consecutive applied steps from the same start: p and buf bit-equal between
    tcam_sgd_step(first = [step == 0]), tcam_sgd_step_gated (finite gate) and tcam_sgd_step_amp
    (gate = (finite, 0)) after each; steps counts 1, then 2."""
    p, buf, grads = _start(cuda, n, n, 7.0)
    plain, gated, amp = (_Run(cuda, k, p, buf) for k in ("plain", "gated", "amp"))
    g1 = torch.tensor([0.7], device=cuda)
    g2 = torch.tensor([0.7, 0.0], device=cuda)
    for step, g in enumerate(grads):
        plain.step(g, cfg, first=int(step == 0))
        gated.step(g, cfg, gate=g1)
        amp.step(g, cfg, gate=g2)
        for other in (gated, amp):
            assert torch.equal(_bits(other.p), _bits(plain.p)), (other.kind, step)
            assert torch.equal(_bits(other.buf), _bits(plain.buf)), (other.kind, step)
            assert int(other.steps) == step + 1 and int(other.skipped) == 0
    assert not torch.equal(_bits(plain.p), _bits(p))     # the steps did move p
    if cfg[0] == 0.0:
        assert torch.equal(_bits(plain.buf), _bits(buf))   # no momentum: buf never written


@pytest.mark.parametrize("cfg", [POINTS[1], POINTS[3]], ids=["nomomentum", "nesterov"])
@pytest.mark.parametrize("n", NS)
def test_skipped_steps_touch_nothing(cuda, n, cfg):
    """gated with gate = inf / NaN and amp with gate = (inf, 0) / (1, 1): p and buf keep their
    bits (buf all NaN without momentum: not even read into p), steps stays, skipped goes up by
    one; (1, 1) backs the scale off and resets the tracker, (inf, 0) leaves both."""
    p, buf, grads = _start(cuda, n, n + 1, NAN if cfg[0] == 0.0 else 7.0)
    for kind, gv in (("gated", [INF]), ("gated", [NAN]), ("amp", [INF, 0.0]),
                     ("amp", [1.0, 1.0])):
        r = _Run(cuda, kind, p, buf, steps=3)
        r.step(grads[0], cfg, gate=torch.tensor(gv, device=cuda))
        assert torch.equal(_bits(r.p), _bits(p)), (kind, gv)
        assert torch.equal(_bits(r.buf), _bits(buf)), (kind, gv)
        assert int(r.steps) == 3 and int(r.skipped) == 1, (kind, gv)
        if gv == [1.0, 1.0]:
            assert float(r.scale) == 1024.0 * 0.5 and int(r.tracker) == 0
        else:
            assert float(r.scale) == 1024.0 and int(r.tracker) == 1


def test_amp_scale_grows_after_interval_clean_steps(cuda):
    """growth_interval = 2: two clean amp steps multiply the scale by growth once and reset the
    tracker."""
    p, buf, grads = _start(cuda, 257, 5, 7.0)
    r = _Run(cuda, "amp", p, buf)
    r.tracker.zero_()
    gate = torch.tensor([0.3, 0.0], device=cuda)
    r.step(grads[0], POINTS[3], gate=gate, scaler=(2.0, 0.5, 2))
    assert float(r.scale) == 1024.0 and int(r.tracker) == 1 and int(r.steps) == 1
    r.step(grads[1], POINTS[3], gate=gate, scaler=(2.0, 0.5, 2))
    assert float(r.scale) == 2048.0 and int(r.tracker) == 0 and int(r.steps) == 2
    assert int(r.skipped) == 0
