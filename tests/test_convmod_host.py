"""The conv module without a GPU: the float64 reference of tests/convmod_oracle.py against a naive loop and against torch.nn
(F.conv1d, BatchNorm1d + SiLU with autograd, F.glu / F.silu + masked_fill), which is what makes it a reference for
tests/test_convmod_kernels_gpu.py."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convmod_oracle as CO  # noqa: E402

F64 = torch.float64
# every (k, pad_left) of tests/test_convmod_kernels_gpu.py: symmetric for all four kernel sizes, the five pads of k = 9 and 31
K_PAD = [(3, 1), (5, 2), (9, 4), (31, 15)] + [(k, p) for k in (9, 31) for p in (0, (k - 1) // 2 + 1, k - 1)]


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize("k,pad_left", K_PAD)
def test_dwconv_equals_the_naive_loop_and_conv1d(k, pad_left):
    B, T, d = 2, 11, 3   # T < k for k = 31: every output sees both zero pads
    g = torch.Generator().manual_seed(10 * k + pad_left)
    x = torch.randn(B, T, d, generator=g, dtype=F64).requires_grad_(True)
    w = torch.randn(d, k, generator=g, dtype=F64).requires_grad_(True)
    bias = torch.randn(d, generator=g, dtype=F64).requires_grad_(True)
    dy = torch.randn(B, T, d, generator=g, dtype=F64)
    y = CO.dwconv(x, w, bias, pad_left)
    naive = torch.zeros(B, T, d, dtype=F64)
    for b in range(B):
        for t in range(T):
            for c in range(d):
                a = bias[c].item()
                for j in range(k):
                    s = t + j - pad_left
                    if 0 <= s < T:
                        a += w[c, j].item() * x[b, s, c].item()
                naive[b, t, c] = a
    assert _rel(y.detach(), naive) < 1e-13
    ref = F.conv1d(F.pad(x.transpose(1, 2), (pad_left, k - 1 - pad_left)), w[:, None], bias, groups=d).transpose(1, 2)
    assert _rel(y.detach(), ref.detach()) < 1e-13
    ref.backward(dy)
    dx, dw, db, cdx, cdw, cdb = CO.dwconv_grads(dy, x, w, pad_left)
    assert _rel(dx, x.grad) < 1e-12 and _rel(dw, w.grad) < 1e-12 and _rel(db, bias.grad) < 1e-12
    # the conditioning sums bound their signed sums, term by term
    assert torch.all(cdx >= dx.abs() * (1 - 1e-12)) and torch.all(cdw >= dw.abs() * (1 - 1e-12)) and torch.all(cdb >= db.abs() * (1 - 1e-12))
    assert torch.all(CO.dwconv_cond(x, w, bias, pad_left) >= y.detach().abs() * (1 - 1e-12))
    assert _rel(cdb, dy.abs().sum((0, 1))) < 1e-13
    terms = list(CO.dwconv_dw_terms(dy, x.detach(), k, pad_left))
    assert _rel(torch.stack([t.sum(0) for t in terms], 1), w.grad) < 1e-12
    assert _rel(torch.stack([t.abs().sum(0) for t in terms], 1), cdw) < 1e-12


@pytest.mark.parametrize("M,d", [(2, 4), (33, 12), (450, 24)])
@pytest.mark.parametrize("training", [True, False])
def test_bn_swish_equals_batchnorm1d_silu_in_float64(M, d, training):
    g = torch.Generator().manual_seed(7 * M + d)
    c = (torch.randn(M, d, generator=g, dtype=F64) * 1.5 + 0.7).requires_grad_(True)
    dy = torch.randn(M, d, generator=g, dtype=F64)
    bn = torch.nn.BatchNorm1d(d, eps=1e-5, momentum=0.1, dtype=F64)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(d, generator=g, dtype=F64) + 0.5)
        bn.bias.copy_(torch.randn(d, generator=g, dtype=F64))
        bn.running_mean.copy_(torch.randn(d, generator=g, dtype=F64))
        bn.running_var.copy_(torch.rand(d, generator=g, dtype=F64) + 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    bn.train(training)
    y_ref = F.silu(bn(c))
    y_ref.backward(dy)
    gamma, beta = bn.weight.detach(), bn.bias.detach()
    cd = c.detach()
    if training:
        stats = CO.bn_stats(cd)
        assert _rel(stats[0], cd.sum(0)) < 1e-14 and _rel(stats[1], (cd * cd).sum(0)) < 1e-14
        mean, rstd, rm, rv = CO.bn_finalize(stats, M, rm0, rv0, 0.1, 1e-5)
        assert _rel(mean, cd.mean(0)) < 1e-12 and _rel(rstd, (cd.var(0, unbiased=False) + 1e-5).rsqrt()) < 1e-10
        assert _rel(rm, bn.running_mean) < 1e-12 and _rel(rv, bn.running_var) < 1e-10
        assert CO.bn_finalize(stats, M)[2:] == (None, None)
    else:
        mean, rstd = CO.bn_eval_stats(rm0, rv0, 1e-5)
        assert torch.equal(bn.running_mean, rm0) and torch.equal(bn.running_var, rv0)
    assert _rel(CO.bn_swish(cd, mean, rstd, gamma, beta), y_ref.detach()) < 1e-10
    sums, cond = CO.bn_swish_bwd_sums(dy, cd, mean, rstd, gamma, beta)
    assert _rel(sums[0], bn.bias.grad) < 1e-10 and _rel(sums[1], bn.weight.grad) < 1e-9
    assert torch.all(cond >= sums.abs() * (1 - 1e-12))
    # eval mode must not look at the sums
    dc = CO.bn_swish_bwd_apply(dy, cd, mean, rstd, gamma, beta, sums if training else sums * float("nan"), M, training)
    assert _rel(dc, c.grad) < 1e-9


def test_bn_finalize_count_one_keeps_the_biased_variance():
    c = torch.tensor([[1.0, -2.0, 3.0, 0.5]], dtype=F64)
    mean, rstd, rm, rv = CO.bn_finalize(CO.bn_stats(c), 1, torch.zeros(4), torch.ones(4), 0.1, 1e-5)
    assert torch.equal(mean, c[0]) and _rel(rstd, torch.full((4,), 1e-5, dtype=F64).rsqrt()) < 1e-14
    assert _rel(rm, 0.1 * c[0]) < 1e-14 and _rel(rv, torch.full((4,), 0.9, dtype=F64)) < 1e-14


@pytest.mark.parametrize("lens", [[9, 2, 0], [1, 9, 5]])
@pytest.mark.parametrize("act", [0, 1])
def test_glu_and_swish_masks_equal_torch(act, lens):
    B, T, d = 3, 9, 4
    g = torch.Generator().manual_seed(50 + act + lens[0])
    width = 2 * d if act == 0 else d
    p = torch.randn(B * T, width, generator=g, dtype=F64).requires_grad_(True)
    dout = torch.randn(B, T, d, generator=g, dtype=F64)
    pad = (torch.arange(T)[None] >= torch.tensor(lens)[:, None])[:, :, None]
    ref = (F.glu(p.view(B, T, width), -1) if act == 0 else F.silu(p.view(B, T, width))).masked_fill(pad, 0.0)
    ref.backward(dout)
    fn = CO.glu_mask if act == 0 else CO.swish_mask
    assert _rel(fn(p, lens, T).detach(), ref.detach()) < 1e-14
    din = CO.mask_bwd(fn, p, dout, lens, T)
    assert _rel(din, p.grad) < 1e-13 and bool((din.view(B, T, width)[pad.expand(B, T, width)] == 0).all())
    # packed rows: only the valid frames, utterance b at rows cu[b] ..
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    rows = torch.cat([torch.arange(n) + b * T for b, n in enumerate(lens)])
    pk = p.detach()[rows]
    assert torch.equal(fn(pk, lens, T, cu), fn(p.detach(), lens, T))
    assert _rel(CO.mask_bwd(fn, pk, dout, lens, T, cu), p.grad[rows]) < 1e-13


def test_colsum():
    t = torch.tensor([[1.0, -2.0], [-1.0, -3.0]], dtype=F64)
    s, a = CO.colsum(t)
    assert torch.equal(s, torch.tensor([0.0, -5.0], dtype=F64)) and torch.equal(a, torch.tensor([2.0, 5.0], dtype=F64))
