"""float64 reference for nemo_amd/csrc/norm.hip: LayerNorm forward / backward, log-softmax forward / backward, column sums.

Closed forms in plain torch on the CPU, no autograd.  Operands arrive in their storage dtype and are up-cast, so a bf16
operand is the bf16-rounded value (the convention of tests/test_kernels_gpu.py): a kernel is then judged on its own
arithmetic only.  tests/test_norm_host.py pins these closed forms to torch.autograd in float64.
"""
import torch

F64 = torch.float64


def _f64(t):
    return t.detach().to("cpu").to(F64)


def layernorm_fwd(x, gamma, beta, eps=1e-5):
    """y [M,d], mean [M], rstd [M] -- biased variance, as torch.nn.LayerNorm"""
    x, gamma, beta = _f64(x), _f64(gamma), _f64(beta)
    mean = x.mean(-1)
    xc = x - mean[:, None]
    rstd = (xc.square().mean(-1) + eps).rsqrt()
    return xc * rstd[:, None] * gamma + beta, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd):
    """dx [M,d], dgamma [d], dbeta [d], and the conditioning of the two column sums: sum_m |dy * xhat| and sum_m |dy|.
    `mean` / `rstd` are inputs (what the kernel is given), not recomputed from x."""
    dy, x, gamma, mean, rstd = _f64(dy), _f64(x), _f64(gamma), _f64(mean), _f64(rstd)
    xhat = (x - mean[:, None]) * rstd[:, None]
    gd = dy * gamma
    s1 = gd.mean(-1, keepdim=True)
    s2 = (gd * xhat).mean(-1, keepdim=True)
    dx = rstd[:, None] * (gd - s1 - xhat * s2)
    t = dy * xhat
    return dx, t.sum(0), dy.sum(0), t.abs().sum(0), dy.abs().sum(0)


def log_softmax_fwd(x):
    """rows may hold -inf entries (never a whole row): those stay -inf"""
    x = _f64(x)
    mx = x.max(-1, keepdim=True).values
    return x - (mx + (x - mx).exp().sum(-1, keepdim=True).log())


def log_softmax_bwd(dy, y, scale=1.0):
    """dx = scale * (dy - exp(y) * sum_j dy): `y` is the saved forward output"""
    dy, y = _f64(dy), _f64(y)
    return scale * (dy - y.exp() * dy.sum(-1, keepdim=True))


def colsum(x, alpha=1.0):
    """alpha * sum_m x[m, :] and its conditioning |alpha| * sum_m |x[m, :]|"""
    x = _f64(x)
    return alpha * x.sum(0), abs(alpha) * x.abs().sum(0)
