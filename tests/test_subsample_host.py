"""The convolutional sub-sampling without a GPU: the float64 reference of tests/subsample_oracle.py (written on nine strided slices
of a zero-padded tensor, no conv2d) against torch.nn.functional in float64 -- F.conv2d on F.pad(x, (pad, 1, pad, 1)) with
groups = 1 and groups = C, autograd for the gradients, F.unfold / F.fold for im2col / col2im -- which is what makes it a reference
for tests/test_subsample_kernels_gpu.py.  Also the extent formulas of the package against the oracle's, and the CPU measurement
of the float32 column-sum error that the GPU file derives its column bound from."""
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subsample_oracle as SO  # noqa: E402

F64 = torch.float64
TOL = 1e-12
# (T, F) of the input grid: odd and even extents on both axes, the 1x1 and 2x2 grids, one axis of length 1 or 2
GRIDS = [(1, 1), (2, 2), (1, 4), (5, 2), (3, 3), (6, 7), (7, 6), (8, 10), (11, 9)]
PADS = (1, 2)


def _rel(a, b):
    a, b = a.detach(), b.detach()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def _gen(*seed):
    return torch.Generator().manual_seed(sum(s * 131 ** i for i, s in enumerate(seed)) + 7)


def _bounds(cond, val):
    return bool(torch.all(cond >= val.abs() * (1 - 1e-12)))


def _padded_nchw(x, pad):
    """channels-last [B,T,F,C] -> F.pad(NCHW, (pad, 1, pad, 1)): `pad` zeros in front of and one behind both axes"""
    return F.pad(x.permute(0, 3, 1, 2), (pad, 1, pad, 1))


# ------------------------------------------------------------------------------------------------ conv1
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("T,F_", GRIDS)
def test_conv1_equals_conv2d_and_its_autograd(T, F_, pad):
    B, C = 3, 5
    g = _gen(T, F_, pad)
    mel = torch.randn(B, F_, T, generator=g, dtype=F64)
    w = torch.randn(C, 1, 3, 3, generator=g, dtype=F64).requires_grad_(True)
    b = torch.randn(C, generator=g, dtype=F64).requires_grad_(True)
    len0 = torch.tensor([T + 5, (2 * T) // 3, 0])     # clamped to T; inside; empty
    T1, F1 = SO.half_len(T, pad), SO.half_len(F_, pad)
    len1 = torch.tensor([T1, max(T1 - 1, 0), T1 + 3])
    x = mel.transpose(1, 2) * (torch.arange(T)[None, :, None] < len0.clamp(max=T)[:, None, None])
    ref = F.conv2d(_padded_nchw(x[..., None], pad), w, b, stride=2).permute(0, 2, 3, 1)
    assert tuple(ref.shape) == (B, T1, F1, C)
    pre, cond, out = SO.conv1_fwd(mel, w, b, len0, len1, pad)
    assert _rel(pre, ref) < TOL
    live = (torch.arange(T1)[None, :, None, None] < len1.clamp(max=T1)[:, None, None, None])
    assert _rel(out, torch.relu(ref) * live) < TOL
    assert _bounds(cond, pre)
    assert _rel(cond, F.conv2d(_padded_nchw(x[..., None].abs(), pad), w.abs(), b.abs(), stride=2).permute(0, 2, 3, 1)) < TOL
    # gradients: dout is NOT masked by the reference (the kernel's contract is "already gated"), the mel is
    dout = torch.randn(B, T1, F1, C, generator=g, dtype=F64)
    ref.backward(dout)
    dw, db, adw, adb = SO.conv1_bwd(dout, mel, len0, pad)
    assert _rel(dw, w.grad[:, 0]) < TOL and _rel(db, b.grad) < TOL
    assert _bounds(adw, dw) and _bounds(adb, db)
    assert _rel(adb, dout.abs().sum((0, 1, 2))) < TOL
    assert _rel(adw, SO.conv1_bwd(dout.abs(), mel.abs(), len0, pad)[0]) < TOL
    terms = list(SO.conv1_bwd_terms(dout, mel, len0, pad))
    assert len(terms) == 10 and all(tuple(t.shape) == (B * T1 * F1, C) for t in terms)


def test_conv1_upcasts_its_operands():
    g = _gen(1)
    mel, w, b = torch.randn(2, 6, 7, generator=g), torch.randn(4, 1, 3, 3, generator=g), torch.randn(4, generator=g)
    pre, _, _ = SO.conv1_fwd(mel, w, b, [7, 7], [4, 4], 1)
    assert pre.dtype == F64
    assert torch.equal(pre, SO.conv1_fwd(mel.double(), w.double(), b.double(), [7, 7], [4, 4], 1)[0])
    d16 = torch.randn(2, 4, 3, 4, generator=g).bfloat16()
    assert torch.equal(SO.conv1_bwd(d16, mel, [7, 7], 1)[0], SO.conv1_bwd(d16.double(), mel, [7, 7], 1)[0])


# ------------------------------------------------------------------------------------------------ im2col / col2im
def _unfold(x, pad):
    """[B,T1,F1,C] -> [B*T2*F2, 9C] through F.unfold (whose rows are c*9 + k)"""
    B, T1, F1, C = x.shape
    nchw = x.permute(0, 3, 1, 2)
    u = F.unfold(nchw, 3, padding=1, stride=2) if pad == 1 else F.unfold(F.pad(nchw, (2, 1, 2, 1)), 3, stride=2)
    return u.view(B, C, 9, -1).permute(0, 3, 2, 1).reshape(-1, 9 * C)


def _fold(dcol, B, T1, F1, C, pad):
    """the transpose of _unfold through F.fold"""
    d = dcol.view(B, -1, 9, C).permute(0, 3, 2, 1).reshape(B, C * 9, -1)
    if pad == 1:
        y = F.fold(d, (T1, F1), 3, padding=1, stride=2)
    else:
        y = F.fold(d, (T1 + 3, F1 + 3), 3, stride=2)[:, :, 2:2 + T1, 2:2 + F1]
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("T1,F1", GRIDS)
def test_im2col_and_col2im_equal_unfold_and_fold(T1, F1, pad):
    B, C = 2, 3
    g = _gen(T1, F1, pad, 2)
    x = torch.randn(B, T1, F1, C, generator=g, dtype=F64)
    col = SO.im2col(x, pad)
    T2, F2 = SO.half_len(T1, pad), SO.half_len(F1, pad)
    assert tuple(col.shape) == (B * T2 * F2, 9 * C)
    assert torch.equal(col, _unfold(x, pad))                       # a gather: exact
    # the element the kernels' index arithmetic names: (b, t2, f2), (kh, kw, ci) <- x[b, 2 t2 + kh - pad, 2 f2 + kw - pad, ci]
    c5 = col.view(B, T2, F2, 9, C)
    for kh in range(3):
        for kw in range(3):
            t1, f1 = 2 * (T2 - 1) + kh - pad, 2 * (F2 - 1) + kw - pad
            want = x[1, t1, f1] if 0 <= t1 < T1 and 0 <= f1 < F1 else torch.zeros(C, dtype=F64)
            assert torch.equal(c5[1, T2 - 1, F2 - 1, kh * 3 + kw], want)
    act = torch.relu(torch.randn(B, T1, F1, C, generator=g, dtype=F64))
    act[0, 0, 0, 0] = -0.0
    dcol = torch.randn(B * T2 * F2, 9 * C, generator=g, dtype=F64)
    din, cdin = SO.col2im_relu(dcol, act, pad)
    ref = _fold(dcol, B, T1, F1, C, pad) * (act > 0)
    assert _rel(din, ref) < TOL
    assert _rel(cdin, _fold(dcol.abs(), B, T1, F1, C, pad) * (act > 0)) < TOL
    assert _bounds(cdin, din) and not din[act <= 0].any()
    # col2im is the transpose of im2col
    y = torch.randn(B, T1, F1, C, generator=g, dtype=F64)
    ones = torch.ones_like(act)
    assert abs(((SO.im2col(y, pad) * dcol).sum() - (y * SO.col2im_relu(dcol, ones, pad)[0]).sum()).item()) < 1e-10


def test_im2col_keeps_the_bits_of_a_bf16_operand():
    x = torch.tensor([1.0, -0.0, 3.140625, -2.5]).bfloat16().view(1, 1, 1, 4)
    col = SO.im2col(x, 1)
    assert col.dtype == F64 and tuple(col.shape) == (1, 36)
    back = col.to(torch.bfloat16).view(torch.int16)
    assert torch.equal(back[0, 16:20], x.view(torch.int16).flatten()) and not back[0, :16].any() and not back[0, 20:].any()


# ------------------------------------------------------------------------------------------------ depthwise
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("T1,F1", GRIDS)
def test_dwconv2d_equals_grouped_conv2d_and_its_autograd(T1, F1, pad):
    B, C = 2, 5
    g = _gen(T1, F1, pad, 3)
    x = torch.relu(torch.randn(B, T1, F1, C, generator=g, dtype=F64))
    x[0, 0, 0, 1] = -0.0
    xr = x.clone().requires_grad_(True)
    w = torch.randn(C, 1, 3, 3, generator=g, dtype=F64).requires_grad_(True)
    b = torch.randn(C, generator=g, dtype=F64).requires_grad_(True)
    ref = F.conv2d(_padded_nchw(xr, pad), w, b, stride=2, groups=C).permute(0, 2, 3, 1)
    T2, F2 = SO.half_len(T1, pad), SO.half_len(F1, pad)
    assert tuple(ref.shape) == (B, T2, F2, C)
    out, cond = SO.dwconv2d_fwd(x, w, b, pad)
    assert _rel(out, ref) < TOL and _bounds(cond, out)
    assert _rel(cond, F.conv2d(_padded_nchw(x.abs(), pad), w.abs(), b.abs(), stride=2, groups=C).permute(0, 2, 3, 1)) < TOL
    dout = torch.randn(B, T2, F2, C, generator=g, dtype=F64)
    ref.backward(dout)
    din, cdin, dw, db, adw, adb = SO.dwconv2d_bwd(dout, x, w, pad)
    assert _rel(din, xr.grad * (x > 0)) < TOL
    assert _rel(dw, w.grad[:, 0]) < TOL and _rel(db, b.grad) < TOL
    assert _bounds(cdin, din) and _bounds(adw, dw) and _bounds(adb, db) and not din[x <= 0].any()
    a = SO.dwconv2d_bwd(dout.abs(), x.abs(), w.abs(), pad)
    assert _rel(cdin, a[0]) < TOL and _rel(adw, a[2]) < TOL and _rel(adb, a[3]) < TOL


def test_tap_reduce():
    p = torch.tensor([[[1.0, -2.0], [0.5, 4.0]], [[-1.0, -3.0], [0.25, -4.0]]])   # [P = 2, KS + 1 = 2, d = 2]
    s, a = SO.tap_reduce(p)
    assert torch.equal(s, torch.tensor([[0.0, -5.0], [0.75, 0.0]], dtype=F64))
    assert torch.equal(a, torch.tensor([[2.0, 5.0], [0.75, 8.0]], dtype=F64))


# ------------------------------------------------------------------------------------------------ extents
@pytest.mark.parametrize("pad", PADS)
def test_extent_formulas_agree(pad):
    """ops.half_len, the encoder's valid-length recurrence and the launchers' formula against the oracle's extents, which
    test_*_equals_* above pin to the output shape of F.conv2d; here also directly for every n"""
    from nemo_amd import ops
    from nemo_amd.modules.conformer_encoder import ConformerEncoder
    enc = types.SimpleNamespace(pre_encode=types.SimpleNamespace(_pad=pad))   # all that _lens reads of its encoder
    n = torch.arange(0, 41)
    lens = ConformerEncoder._lens(enc, n, 3)
    assert torch.equal(lens[0], n)
    want = n
    for stage in (1, 2, 3):
        want = torch.tensor([SO.half_len(int(v), pad) for v in want])
        assert torch.equal(lens[stage], want), (pad, stage)
    w = torch.ones(1, 1, 3, 3, dtype=F64)
    for v in range(0, 41):
        assert ops.half_len(v, pad) == SO.half_len(v, pad) == (v + pad + 1 - 3) // 2 + 1
        if v >= 1:
            assert F.conv2d(F.pad(torch.ones(1, 1, v, 1, dtype=F64), (pad, 1, pad, 1)), w, stride=2).shape[2] == SO.half_len(v, pad)
            assert len(SO._taps(torch.ones(1, v, 1), pad)) == 9 and SO._taps(torch.ones(1, v, 1), pad)[8].shape[1] == SO.half_len(v, pad)
    assert SO.half_len(0, 1) == 0 and SO.half_len(0, 2) == 1   # an empty utterance still yields the frame of the causal padding


# ------------------------------------------------------------------------------------------------ float32 column-sum error
def f32_col_error(terms, prefill):
    """the reduced columns of the GPU file, summed the plain way: prefill + torch.sum(terms.float(), 0) in float32 on the CPU
    against the float64 sum, per column of its conditioning |prefill| + sum |term|; returns the worst column's error.
    terms [N, d] (float64, exact products of the stored operands), prefill [d] float32"""
    terms = terms.double().reshape(-1, terms.shape[-1])
    pre = prefill.flatten()
    got = (pre.float() + torch.sum(terms.float(), 0)).double()
    ref, cond = pre.double() + terms.sum(0), pre.double().abs() + terms.abs().sum(0)
    return ((got - ref).abs() / cond).max().item()


def test_f32_col_error_measures_rounding_only():
    g = _gen(9)
    ints = torch.randint(-8, 9, (300, 6), generator=g).double()
    assert f32_col_error(ints, torch.ones(6)) == 0.0                          # exactly representable: no error at all
    e = f32_col_error(torch.randn(300, 6, generator=g, dtype=F64), torch.randn(6, generator=g))
    assert 0.0 < e < 300 * 2.0 ** -24                                         # within the worst case of 300 float32 additions
