"""float64 reference for nemo_amd/csrc/subsample.hip and nemo_amd/csrc/dwconv2d.hip: the 3x3 stride-2 stages of the convolutional
sub-sampling (dense 1 -> C on the mel spectrogram, im2col / col2im around the conv2 GEMM, depthwise C -> C), their gradients, and
the second stage of the weight-gradient reductions (tap_reduce_kernel, common.h).

Plain torch on the CPU, no project imports and no conv2d: every operation is written on a zero-padded tensor and its nine strided
slices, `pad` (1 or 2) zeros in front of each axis and one behind it.  Operands arrive in their storage dtype and are up-cast, so a
bf16 operand is the bf16-rounded value and a kernel is judged on its own arithmetic only.  Next to every sum the functions return
the sum of the magnitudes of its terms (`cond`): what its rounding errors scale with.  tests/test_subsample_host.py pins all of
it to torch.nn.functional in float64.

Layouts (the kernels'): mel [B,F,T]; activations channels-last [B,T1,F1,C]; weights [C,1,3,3] or [C,3,3], tap k = kh*3 + kw
(kh along time, kw along frequency); col [B*T2*F2, 9C] with column k*C + ci.
"""
import torch

F64 = torch.float64


def _f64(t):
    return torch.as_tensor(t).detach().to("cpu").to(F64)


def _w9(w):
    w = _f64(w)
    return w.reshape(w.shape[0], 9)   # [C,1,3,3] or [C,3,3] -> [C, 9]


def half_len(n, pad):
    """extent after one stage: kernel 3, stride 2, `pad` zeros in front and one behind"""
    return (n + pad - 2) // 2 + 1


def _padded(x, pad):
    """x [B, T, F, ...] -> [B, T + pad + 1, F + pad + 1, ...], zeros around"""
    B, T, F_ = x.shape[:3]
    xp = torch.zeros((B, T + pad + 1, F_ + pad + 1) + tuple(x.shape[3:]), dtype=x.dtype)
    xp[:, pad:pad + T, pad:pad + F_] = x
    return xp


def _slices(n_t, n_f):
    """the nine index pairs: tap k = kh*3 + kw of output (t2, f2) reads the padded grid at (2 t2 + kh, 2 f2 + kw)"""
    return [(slice(kh, kh + 2 * n_t - 1, 2), slice(kw, kw + 2 * n_f - 1, 2)) for kh in range(3) for kw in range(3)]


def _taps(x, pad):
    """nine views xs[k][b, t2, f2, ...] = x[b, 2 t2 + kh - pad, 2 f2 + kw - pad, ...], zero outside the grid"""
    T2, F2 = half_len(x.shape[1], pad), half_len(x.shape[2], pad)
    xp = _padded(x, pad)
    return [xp[:, st, sf] for st, sf in _slices(T2, F2)]


def _scatter(terms, T1, F1, pad):
    """the transpose of _taps: terms[k] [B,T2,F2,...] are added at the places tap k read; returns [B,T1,F1,...]"""
    B, T2, F2 = terms[0].shape[:3]
    acc = torch.zeros((B, T1 + pad + 1, F1 + pad + 1) + tuple(terms[0].shape[3:]), dtype=F64)
    for (st, sf), t in zip(_slices(T2, F2), terms):
        acc[:, st, sf] += t
    return acc[:, pad:pad + T1, pad:pad + F1]


def _masked_mel(mel, len0):
    """mel [B,F,T] -> [B,T,F] with the frames t >= min(T, len0[b]) set to zero"""
    x = _f64(mel).transpose(1, 2)
    T = x.shape[1]
    lim = torch.as_tensor(len0).to("cpu").to(torch.int64).clamp(max=T)
    return x * (torch.arange(T)[None, :] < lim[:, None])[:, :, None]


# ------------------------------------------------------------------------------------------------ conv1 (dense, 1 -> C)
def conv1_fwd(mel, w, b, len0, len1, pad):
    """(pre [B,T1,F1,C] = b + sum_k w[c,k] * x_k, cond = |b| + sum_k |w * x|, out = (t1 < min(T1, len1)) * relu(pre))"""
    xs = _taps(_masked_mel(mel, len0), pad)
    w, b = _w9(w), _f64(b)
    pre = b.expand(xs[0].shape + (w.shape[0],)).clone()
    cond = pre.abs()
    for k, x in enumerate(xs):
        t = x[..., None] * w[:, k]
        pre += t
        cond += t.abs()
    T1 = pre.shape[1]
    lim = torch.as_tensor(len1).to("cpu").to(torch.int64).clamp(max=T1)
    live = (torch.arange(T1)[None, :] < lim[:, None])[:, :, None, None]
    return pre, cond, pre.clamp_min(0.0) * live


def conv1_bwd_terms(dout, mel, len0, pad):
    """the terms of the ten reduced columns per channel: yields [B*T1*F1, C] for the nine taps, then for the bias.  dout is taken
    as it is (the kernel's contract: already gated by the ReLU and the length mask); only the mel is masked"""
    dout = _f64(dout)
    C = dout.shape[-1]
    for x in _taps(_masked_mel(mel, len0), pad):
        yield (dout * x[..., None]).reshape(-1, C)
    yield dout.reshape(-1, C)


def _reduce(terms):
    """(sums [C, 9], bias sum [C], sums of magnitudes [C, 9], [C]) of ten term matrices"""
    s, a = zip(*((t.sum(0), t.abs().sum(0)) for t in terms))
    return torch.stack(s[:9], 1), s[9], torch.stack(a[:9], 1), a[9]


def conv1_bwd(dout, mel, len0, pad):
    """(dw [C,3,3], db [C], sum |term| of dw, of db)"""
    dw, db, adw, adb = _reduce(conv1_bwd_terms(dout, mel, len0, pad))
    return dw.reshape(-1, 3, 3), db, adw.reshape(-1, 3, 3), adb


# ------------------------------------------------------------------------------------------------ im2col / col2im
def im2col(x, pad):
    """x [B,T1,F1,C] -> [B*T2*F2, 9C], column (kh*3 + kw)*C + ci; taps outside the grid are zero"""
    C = x.shape[-1]
    return torch.stack(_taps(_f64(x), pad), 3).reshape(-1, 9 * C)


def col2im_relu(dcol, act, pad):
    """(din [B,T1,F1,C] = (act > 0) * sum of the dcol entries that im2col filled from (b,t1,f1,c), sum of their magnitudes)"""
    act = _f64(act)
    B, T1, F1, C = act.shape
    T2, F2 = half_len(T1, pad), half_len(F1, pad)
    d = _f64(dcol).reshape(B, T2, F2, 9, C)
    gate = act > 0
    out = []
    for f in (lambda t: t, torch.abs):
        out.append(_scatter([f(d[:, :, :, k]) for k in range(9)], T1, F1, pad) * gate)
    return tuple(out)


# ------------------------------------------------------------------------------------------------ depthwise (C -> C)
def dwconv2d_fwd(x, w, b, pad):
    """(out [B,T2,F2,C] = b + sum_k w[c,k] * x_k[..., c], cond = |b| + sum_k |w * x|)"""
    w, b = _w9(w), _f64(b)
    xs = _taps(_f64(x), pad)
    out = b.expand(xs[0].shape).clone()
    cond = out.abs()
    for k, xk in enumerate(xs):
        t = xk * w[:, k]
        out += t
        cond += t.abs()
    return out, cond


def dwconv2d_dw_terms(dout, x, pad):
    """yields [B*T2*F2, C]: dout * x_k for the nine taps, then dout for the bias"""
    dout = _f64(dout)
    C = dout.shape[-1]
    for xk in _taps(_f64(x), pad):
        yield (dout * xk).reshape(-1, C)
    yield dout.reshape(-1, C)


def dwconv2d_bwd(dout, x, w, pad):
    """(din = (x > 0) * sum_k w[c,k] * dout at the outputs that read x, its cond, dw [C,3,3], dbias, sum |term| of dw, of dbias)"""
    dout, x, w = _f64(dout), _f64(x), _w9(w)
    T1, F1 = x.shape[1:3]
    gate = x > 0
    terms = [dout * w[:, k] for k in range(9)]
    din = _scatter(terms, T1, F1, pad) * gate
    cdin = _scatter([t.abs() for t in terms], T1, F1, pad) * gate
    dw, db, adw, adb = _reduce(dwconv2d_dw_terms(dout, x, pad))
    return din, cdin, dw.reshape(-1, 3, 3), db, adw.reshape(-1, 3, 3), adb


# ------------------------------------------------------------------------------------------------ second-stage reduction
def tap_reduce(partial):
    """partial [P, KS+1, d] -> (sums [KS+1, d], sums of magnitudes): row k < KS is tap k of every channel, row KS the bias"""
    p = _f64(partial)
    return p.sum(0), p.abs().sum(0)
