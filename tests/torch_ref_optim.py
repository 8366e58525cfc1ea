"""numpy float32 restatement of the fused Adam step's declared arithmetic (include/sgr_optim.h): one IEEE single
operation at a time, no contraction, correctly rounded division and square root, denormals kept -- the op order of
torch/optim/adam.py: _multi_tensor_adam, with the host scalars computed in double as torch's Python computes them."""
import numpy as np

f32 = np.float32


def host_scalars(lr, step, betas=(0.9, 0.999)):
    """(step_size, bc2_sqrt) as f32: bc1 = 1 - beta1 ** step, bc2_sqrt = (1 - beta2 ** step) ** 0.5 in double,
    step_size = -(lr / bc1), then rounded."""
    beta1, beta2 = betas
    bc1 = 1 - beta1 ** float(step)
    bc2 = 1 - beta2 ** float(step)
    return f32(-(lr / bc1)), f32(bc2 ** 0.5)


def adam_step(p, g, m, v, lr, step, betas=(0.9, 0.999), eps=1e-15):
    """One step of one chunk (float32 arrays, not modified); ``step`` is the count after this step's increment.
    Returns new (p, m, v)."""
    p, g, m, v = (np.asarray(a, dtype=f32) for a in (p, g, m, v))
    c1, b2, c2 = f32(1 - betas[0]), f32(betas[1]), f32(1 - betas[1])
    ss, bc2s = host_scalars(lr, step, betas)
    e = f32(eps)
    with np.errstate(all="ignore"):
        m = m + c1 * (g - m)
        v = v * b2
        v = v + c2 * (g * g)
        d = np.sqrt(v) / bc2s + e
        p = p + ss * (m / d)
    return p.astype(f32), m.astype(f32), v.astype(f32)
