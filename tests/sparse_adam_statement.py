"""The rule of optim.SparseAdam written down in float64 numpy -- nothing shared with the kernel or its host code.

One parameter tensor [P, ...], a visibility mask vis[P] and the tensor's own 1-based step count t:
  * a row with vis == 0 keeps param, exp_avg and exp_avg_sq;
  * a row with vis != 0 gets
        m <- m + (g - m) (1 - beta1)
        v <- v beta2 + (1 - beta2) g^2
        p <- p - step_size m / (sqrt(v) inv_bc2_sqrt + eps)
    with step_size = lr / (1 - beta1^t), inv_bc2_sqrt = 1 / sqrt(1 - beta2^t) under bias_correction, and step_size = lr, inv_bc2_sqrt = 1
    without it;
  * t advances on every call in which the tensor has a gradient, whatever the mask says.
vis = None is the dense step (every row visible, always bias-corrected: what optim.Adam does and what SparseAdam does to its dense groups)."""
import numpy as np


class Tensor:
    def __init__(self, value):
        self.p = np.array(value, dtype=np.float64)
        self.m = np.zeros_like(self.p)
        self.v = np.zeros_like(self.p)
        self.t = 0

    def load(self, exp_avg, exp_avg_sq, step):
        self.m, self.v, self.t = np.array(exp_avg, dtype=np.float64), np.array(exp_avg_sq, dtype=np.float64), int(step)
        return self


def step(tensor, grad, lr, vis=None, beta1=0.9, beta2=0.999, eps=1e-15, bias_correction=True):
    """One call of the optimizer for one tensor; grad None = the tensor has no gradient this call (nothing happens, t stays)."""
    if grad is None:
        return
    tensor.t += 1
    t = tensor.t
    g = np.asarray(grad, dtype=np.float64)
    if vis is None:
        rows = np.ones(tensor.p.shape[0], dtype=bool)
        bias_correction = True
    else:
        rows = np.asarray(vis) != 0
        assert rows.shape == (tensor.p.shape[0],)
    if bias_correction:
        step_size, inv_bc2_sqrt = lr / (1.0 - beta1 ** t), 1.0 / np.sqrt(1.0 - beta2 ** t)
    else:
        step_size, inv_bc2_sqrt = lr, 1.0
    r = rows                                                              # boolean row index: the other rows are not touched
    m = tensor.m[r] + (g[r] - tensor.m[r]) * (1.0 - beta1)
    v = tensor.v[r] * beta2 + (1.0 - beta2) * g[r] * g[r]
    tensor.m[r], tensor.v[r] = m, v
    tensor.p[r] = tensor.p[r] - step_size * m / (np.sqrt(v) * inv_bc2_sqrt + eps)
