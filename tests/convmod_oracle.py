"""float64 reference for nemo_amd/csrc/convmod.hip: depthwise Conv1d along time on [B,T,d], BatchNorm1d statistics, BN + Swish,
the GLU / Swish + pad mask in front of the convolution, and their gradients.

Plain torch on the CPU.  Operands arrive in their storage dtype and are up-cast, so a bf16 operand is the bf16-rounded value: a
kernel is then judged on its own arithmetic only.  The forward functions are differentiable (float64 operands that require grad
keep their graph); the convolution's and the masks' gradients come from autograd, BatchNorm + Swish backward is a closed form in
the kernels' own terms (mean / rstd / sums are INPUTS there).  tests/test_convmod_host.py pins all of it to torch.nn.
"""
import torch

F64 = torch.float64


def _f64(t):
    return t.to("cpu").to(F64)


def _wk(w):
    w = _f64(w)
    return w.reshape(w.shape[0], w.shape[-1])   # [d, 1, k] or [d, k]


def _shifted(x, k, pad_left):
    """k views xs[j][b, t, c] = x[b, t + j - pad_left, c], zero outside [0, T)"""
    T = x.shape[1]
    xp = torch.nn.functional.pad(x, (0, 0, pad_left, k - 1 - pad_left))
    return [xp[:, j:j + T] for j in range(k)]


def dwconv(x, w, bias, pad_left):
    """y[b,t,c] = bias[c] + sum_k w[c,k] * x[b, t+k-pad_left, c], zero outside [0, T).  x [B,T,d], w [d,k] or [d,1,k]"""
    x, w = _f64(x), _wk(w)
    k = w.shape[1]
    assert 0 <= pad_left < k
    y = torch.zeros_like(x) if bias is None else _f64(bias).expand_as(x).clone()
    for j, xs in enumerate(_shifted(x, k, pad_left)):
        y = y + w[:, j] * xs
    return y


def dwconv_cond(x, w, bias, pad_left):
    """|bias| + sum_k |w * x| per output: what the rounding errors of the tap chain scale with"""
    return dwconv(_f64(x).detach().abs(), _wk(w).detach().abs(), None if bias is None else _f64(bias).detach().abs(), pad_left)


def dwconv_grads(dy, x, w, pad_left):
    """(dx, dw [d,k], dbias) by autograd, then their conditioning (sum_k |w * dy|, sum_{b,t} |dy * x|, sum_{b,t} |dy|): the
    same gradients at |dy|, |x|, |w|, where no term cancels"""
    out = []
    for f in (lambda t: t, torch.abs):
        xx = f(_f64(x).detach()).requires_grad_(True)
        ww = f(_wk(w).detach()).requires_grad_(True)
        bb = torch.zeros(ww.shape[0], dtype=F64, requires_grad=True)
        dwconv(xx, ww, bb, pad_left).backward(f(_f64(dy).detach()))
        out += [xx.grad, ww.grad, bb.grad]
    return tuple(out)


def dwconv_dw_terms(dy, x, k, pad_left):
    """the terms of the weight gradient, tap by tap: yields [B*T, d] = dy[b,t,c] * x[b, t+j-pad_left, c] for j = 0 .. k-1"""
    dy, x = _f64(dy), _f64(x)
    for xs in _shifted(x, k, pad_left):
        yield (dy * xs).reshape(-1, x.shape[-1])


def colsum(terms):
    """(sum, sum of magnitudes) over the rows of [M, d]: a reduced column and its conditioning"""
    t = _f64(terms).reshape(-1, terms.shape[-1])
    return t.sum(0), t.abs().sum(0)


# ------------------------------------------------------------------------------------------------ BatchNorm + Swish
def bn_stats(c):
    """[2, d]: sum and sum of squares per channel over every position of c [..., d]"""
    c = _f64(c).reshape(-1, c.shape[-1])
    return torch.stack([c.sum(0), c.square().sum(0)])


def bn_finalize(stats, count, running_mean=None, running_var=None, momentum=0.1, eps=1e-5):
    """(mean, rstd, new running_mean, new running_var): biased variance for rstd, unbiased for the running variance (torch.nn.
    BatchNorm1d); count = 1 has no unbiased variance and the running variance then takes the biased one (0), as the kernels do"""
    stats = _f64(stats)
    mean = stats[0] / count
    var = (stats[1] / count - mean * mean).clamp_min(0.0)
    rstd = (var + eps).rsqrt()
    unb = var * count / (count - 1) if count > 1 else var
    rm = None if running_mean is None else (1 - momentum) * _f64(running_mean) + momentum * mean
    rv = None if running_var is None else (1 - momentum) * _f64(running_var) + momentum * unb
    return mean, rstd, rm, rv


def bn_eval_stats(running_mean, running_var, eps=1e-5):
    return _f64(running_mean), (_f64(running_var) + eps).rsqrt()


def swish(z):
    return z * torch.sigmoid(z)


def bn_swish(c, mean, rstd, gamma, beta):
    """swish(gamma * (c - mean) * rstd + beta)"""
    return swish(_f64(gamma) * (_f64(c) - _f64(mean)) * _f64(rstd) + _f64(beta))


def bn_swish_bwd_terms(dy, c, mean, rstd, gamma, beta):
    """(dz, dz * xhat, xhat) per element: dz = dy * swish'(gamma * xhat + beta); their column sums are dbeta and dgamma"""
    xh = (_f64(c) - _f64(mean)) * _f64(rstd)
    z = _f64(gamma) * xh + _f64(beta)
    s = torch.sigmoid(z)
    dz = _f64(dy) * (s * (1 + z * (1 - s)))
    return dz, dz * xh, xh


def bn_swish_bwd_sums(dy, c, mean, rstd, gamma, beta):
    """sums [2, d] = (sum dz, sum dz * xhat) and their conditioning [2, d]"""
    dz, dzx, _ = bn_swish_bwd_terms(dy, c, mean, rstd, gamma, beta)
    d = dz.shape[-1]
    dz, dzx = dz.reshape(-1, d), dzx.reshape(-1, d)
    return torch.stack([dz.sum(0), dzx.sum(0)]), torch.stack([dz.abs().sum(0), dzx.abs().sum(0)])


def bn_swish_bwd_apply(dy, c, mean, rstd, gamma, beta, sums, count, training):
    """d(loss)/dc = gamma * rstd * (dz - sums[0] / count - xhat * sums[1] / count); eval mode (training false) drops the two mean
    terms (the statistics are constants there) and does not look at `sums`"""
    dz, _, xh = bn_swish_bwd_terms(dy, c, mean, rstd, gamma, beta)
    if training:
        sums = _f64(sums)
        dz = dz - sums[0] / count - xh * (sums[1] / count)
    return _f64(gamma) * _f64(rstd) * dz


# ------------------------------------------------------------------------------------------------ GLU / Swish + pad mask
def _grid(p, lens, T, cu):
    """rows of p on the padded [B, T, width] grid (packed rows: utterance b's frames are p[cu[b] : cu[b] + len[b]]), and the mask"""
    p = _f64(p)
    B = len(lens)
    valid = torch.arange(T)[None] < torch.as_tensor(lens)[:, None].clamp_max(T)
    if cu is None:
        return p.reshape(B, T, -1), valid
    g = torch.zeros(B, T, p.shape[-1], dtype=F64)
    idx = valid.nonzero()
    rows = torch.as_tensor(cu)[idx[:, 0]] + idx[:, 1]
    g = g.index_put((idx[:, 0], idx[:, 1]), p[rows])
    return g, valid


def glu_mask(p, lens, T, cu=None):
    """[B,T,d] = a * sigmoid(b) * (t < len[b]),  a | b = the halves of p [rows, 2d]; rows = B*T, or packed rows with cu [B+1]"""
    g, valid = _grid(p, lens, T, cu)
    d = g.shape[-1] // 2
    return torch.where(valid[:, :, None], g[..., :d] * torch.sigmoid(g[..., d:]), torch.zeros((), dtype=F64))


def swish_mask(p, lens, T, cu=None):
    """[B,T,d] = swish(p) * (t < len[b]),  p [rows, d]"""
    g, valid = _grid(p, lens, T, cu)
    return torch.where(valid[:, :, None], swish(g), torch.zeros((), dtype=F64))


def mask_bwd(fn, p, dout, lens, T, cu=None):
    """gradient of glu_mask / swish_mask w.r.t. p, in p's own layout (padded grid: zero rows beyond len[b])"""
    pp = _f64(p).detach().requires_grad_(True)
    fn(pp, lens, T, cu).backward(_f64(dout).detach())
    return pp.grad
