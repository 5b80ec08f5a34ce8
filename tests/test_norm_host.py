"""LayerNorm / log-softmax / column sums without a GPU: the float64 closed forms of tests/norm_oracle.py against torch.autograd
(what makes them a reference for tests/test_norm_kernels_gpu.py), and the argument checks of the C ABI that return before any
launch."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_oracle as NO  # noqa: E402

SHAPES = [(1, 4), (7, 36), (33, 516)]   # (M, d): the smallest row the kernels accept, one row only, an ordinary matrix


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


@pytest.mark.parametrize("M,d", SHAPES)
def test_layernorm_closed_forms_equal_autograd_in_float64(M, d):
    g = torch.Generator().manual_seed(100 + d)
    x = (torch.randn(M, d, generator=g, dtype=torch.float64) * 2 + 0.5).requires_grad_(True)
    gamma = torch.randn(d, generator=g, dtype=torch.float64).requires_grad_(True)
    beta = torch.randn(d, generator=g, dtype=torch.float64).requires_grad_(True)
    dy = torch.randn(M, d, generator=g, dtype=torch.float64)
    y_ref = F.layer_norm(x, (d,), gamma, beta, 1e-5)
    y_ref.backward(dy)
    y, mean, rstd = NO.layernorm_fwd(x, gamma, beta, 1e-5)
    assert _rel(y, y_ref.detach()) < 1e-12
    assert _rel(mean, x.detach().mean(-1)) < 1e-12
    assert _rel(rstd, (x.detach().var(-1, unbiased=False) + 1e-5).rsqrt()) < 1e-12
    dx, dgamma, dbeta, a_g, a_b = NO.layernorm_bwd(dy, x, gamma, mean, rstd)
    assert _rel(dx, x.grad) < 1e-12 and _rel(dgamma, gamma.grad) < 1e-12 and _rel(dbeta, beta.grad) < 1e-12
    # the conditioning sums bound their signed sums and are exact for a single row
    assert torch.all(a_g >= dgamma.abs() * (1 - 1e-12)) and torch.all(a_b >= dbeta.abs() * (1 - 1e-12))
    if M == 1:
        assert torch.equal(a_b, dy[0].abs())


@pytest.mark.parametrize("M,C", [(1, 4), (5, 1), (33, 129)])
def test_log_softmax_closed_forms_equal_autograd_in_float64(M, C):
    g = torch.Generator().manual_seed(200 + C)
    x = (torch.randn(M, C, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    dy = torch.randn(M, C, generator=g, dtype=torch.float64)
    y_ref = torch.log_softmax(x, -1)
    y_ref.backward(dy)
    y = NO.log_softmax_fwd(x)
    assert (y - y_ref.detach()).abs().max().item() <= 1e-12 * max(1.0, y_ref.detach().abs().max().item())
    dx = NO.log_softmax_bwd(dy, y, 1.0)
    assert (dx - x.grad).abs().max().item() <= 1e-12 * x.grad.abs().max().item() + (1e-14 if C == 1 else 0.0)
    assert torch.allclose(NO.log_softmax_bwd(dy, y, 0.125), 0.125 * dx, rtol=1e-15, atol=0)
    # -inf entries (never a whole row) stay -inf forward and pass scale * dy backward
    if C >= 4:
        xm = x.detach().clone()
        xm[:, ::3] = float("-inf")
        ym = NO.log_softmax_fwd(xm)
        assert torch.all(ym[:, ::3] == float("-inf")) and torch.isfinite(ym[:, 1::3]).all()
        keep = torch.ones(C, dtype=torch.bool); keep[::3] = False
        assert _rel(ym[:, keep], torch.log_softmax(x.detach()[:, keep], -1)) < 1e-12
        dm = NO.log_softmax_bwd(dy, ym, 0.5)
        assert torch.equal(dm[:, ::3], 0.5 * dy[:, ::3]) and torch.isfinite(dm).all()


def test_colsum_closed_form():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(37, 9, generator=g).to(torch.bfloat16)
    s, a = NO.colsum(x, -0.5)
    assert s.dtype == torch.float64 and torch.equal(s, -0.5 * x.double().sum(0)) and torch.equal(a, 0.5 * x.double().abs().sum(0))


def test_layernorm_bwd_rejects_exactly_one_parameter_gradient():
    """dgamma / dbeta: both or neither.  No kernel accumulates only one of them, so asking for one is an argument error
    (MI_ERR_ARG = 1), returned before any launch -- the pointers below are never dereferenced"""
    from nemo_amd import _lib
    buf = (ctypes.c_char * 320)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 31) // 32 * 32)   # 32-byte aligned: no alignment check answers instead
    assert p.value % 32 == 0

    def bwd(dgamma, dbeta):
        return _lib.lib.mi355x_layernorm_bwd(p, 0, p, 0, p, p, p, p, 0, dgamma, dbeta, 2, 8, None)

    def bwd_cast(dgamma, dbeta):
        return _lib.lib.mi355x_layernorm_bwd_cast(p, 0, p, 0, p, p, p, p, 0, dgamma, dbeta, 2, 8, p, 1.0, 0, 0, 1.0, None)

    for f in (bwd, bwd_cast):
        assert f(p, None) == 1
        assert f(None, p) == 1
    # the checks in front of it still answer first
    assert _lib.lib.mi355x_layernorm_bwd(None, 0, p, 0, p, p, p, p, 0, p, p, 2, 8, None) == 1
    assert _lib.lib.mi355x_layernorm_bwd(p, 0, p, 0, p, p, p, p, 0, p, p, 2, 6, None) == 1
    with pytest.raises(ValueError):
        _lib.check(bwd(p, None), "layernorm_bwd")
