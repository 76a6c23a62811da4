"""torch.optim.SGD's step restated in fp64 on the fp32 hyper-parameters the device kernels
receive: the reference of the SGD kernel checks (tests/test_grad_chain_gpu.py), itself pinned
to torch.optim.SGD by tests/test_train_oracle.py."""
import numpy as np
import torch

# (momentum, dampening, weight_decay, nesterov, grad_scale)
SGD_CFGS = [(0.0, 0.0, 0.0, 0, 1.0), (0.0, 0.0, 1e-4, 0, 0.5), (0.9, 0.0, 1e-4, 1, 1.0),
            (0.9, 0.1, 0.0, 0, 0.5), (0.9, 0.0, 0.0, 0, 1.0)]
LR = 0.05


def f32(v):
    return float(np.float32(v))


def ulp(m):
    """One fp32 ulp at magnitude m (fp64 tensor)."""
    _, e = torch.frexp(m.clamp(min=2.0 ** -126))
    return torch.ldexp(torch.ones_like(m), e - 24)


def sgd_ref(p, g, buf, first, cfg):
    """torch.optim.SGD's step in fp64 on the fp32 hyper-parameters the kernel receives; returns
    (p, buf, bound p, bound buf): 4 fp32 ulps of |p| + lr (|g| + wd |p| + m |buf|)(1 + m), and of
    the buffer's own magnitude sum."""
    m, damp, wd, nest, gs = cfg
    lr, m, damp, wd, gs = f32(LR), f32(m), f32(damp), f32(wd), f32(gs)
    d = g * gs + wd * p
    dm = g.abs() * gs + wd * p.abs()
    nb, bmag = buf, buf.abs()
    if m != 0:
        nb = d.clone() if first else m * buf + (1 - damp) * d
        bmag = dm if first else m * buf.abs() + (1 - damp) * dm
        d = d + m * nb if nest else nb
    mag = p.abs() + lr * (g.abs() + wd * p.abs() + m * buf.abs()) * (1 + m)
    return p - lr * d, nb, 4 * ulp(mag), 4 * ulp(bmag)
