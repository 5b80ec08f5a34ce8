"""-m gpu: `ops.ctc_loss` with gradients through every lattice form of nemo_amd/csrc/ctc.hip -- the wave-resident kernel at
P = 1, 2, 4, 8 pairs per lane (2*Umax+1 <= 128 / 256 / 512 / 1024) and the LDS / barrier kernel (above that, or with
`mi355x_ctc_config(0)` at any size) -- against `oracle.conformer_ref.ctc_loss_mean_batch` in float64 on the CPU, which
test_oracle_pinning.py pins to the known answers and to the numpy restatement.

Frames 60 / 129 / 240 / 340 / 560 straddle the emission chunks of the wave form (CtcTc<P>::v = 64 / 64 / 32 / 16 frames).  Per
shape three ragged feasible utterances and one that is infeasible by its length (seven equal labels against eight frames: loss
and gradient rows 0).  Every shape runs with the knob at 1 and at 0; both runs are held to the reference and to each other.

Bounds: what test_ctc_random_ragged_vs_oracle asks at T = 60, for every shape: rtol 1e-4 / atol 1e-5 on the loss, rtol 1e-3 /
atol 1e-5 on the gradient to the logits.  With plain random-normal logits the float32 lattice values grow with T (nll 350 / 690 /
1070 / 1870 at T = 129 / 240 / 340 / 560) and the build from before the lattice kernels shared their code has gradient errors of
0.66 / 1.3 / 5.3 / 11 times that bound there (largest |error| 9.8e-5 / 9.3e-4 / 4.4e-4 / 1.1e-3; the loss stays below 0.01 of its
bound): four times that is no bound worth having.  So the longer lattices are damped: the logits along one alignment of each
target get +6, which keeps nll in the tens.  On these inputs that build's largest errors, over both forms and the difference
between the forms, as |error| and as a share of the bound, were
    (Umax, Tmax)   nll <=   loss               gradient
    (12, 60)       158      3.1e-5   0.002     2.8e-5   0.14      (not damped)
    (100, 129)     20       4.4e-6   0.002     5.2e-6   0.013
    (200, 240)     33       1.9e-5   0.008     1.1e-5   0.023
    (300, 340)     50       3.9e-5   0.009     2.0e-5   0.049
    (520, 560)     81       4.3e-5   0.006     5.9e-5   0.090
so four times the largest error (which covers the order of the LDS float adds of ctc_grad_kernel, which nothing fixes between
runs) is below the T = 60 bound everywhere, and that bound is the one asserted."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"

C = 24                       # blank = C - 1
NLL_TOL = (1e-4, 1e-5)       # rtol, atol at T = 60
GRAD_TOL = (1e-3, 1e-5)
# (Umax, Tmax) -> what is added to the logits along one alignment of each feasible utterance.  Forms: P = 1, 2, 4, 8, LDS only.
# That is four wave forms: at (520, 560) both knob settings run ctc_kernel, so "wave-lds" there compares two runs of the same kernels
# (what differs between them is the order of the float adds in ctc_grad_kernel).
SHAPES = {(12, 60): 0.0, (100, 129): 6.0, (200, 240): 6.0, (300, 340): 6.0, (520, 560): 6.0}


@functools.lru_cache(maxsize=None)
def _case(U, T):
    """inputs and the float64 reference of one shape, computed once: (acts f32 [4,T,C], targets, in_len, tgt_len, nll f64 [4],
    gradient to the logits f64 [4,T,C])"""
    from oracle import conformer_ref as R
    targets = np.zeros((4, U), dtype=np.int64)
    targets[:3] = np.random.RandomState(0).randint(0, C - 1, size=(3, U))
    targets[3, :7] = 1                                  # needs 13 frames > 8: infeasible -> zero_infinity
    in_len = np.array([T, T - 1, T - 17, 8])
    tgt_len = np.array([U, U - 3, U // 2, 7])
    acts = np.random.RandomState(1).randn(4, T, C).astype(np.float32)
    for b in range(3):   # one monotone alignment per utterance: its labels in order, a blank between equal neighbours
        lab = targets[b, : tgt_len[b]]
        need = [lab[0]] + [x for p, c in zip(lab[:-1], lab[1:]) for x in ((C - 1, c) if p == c else (c,))]
        acts[b, np.arange(in_len[b]), np.array(need)[np.arange(in_len[b]) * len(need) // in_len[b]]] += SHAPES[(U, T)]
    acts = torch.from_numpy(acts)
    a64 = acts.double().requires_grad_(True)
    _, per = R.ctc_loss_mean_batch(torch.log_softmax(a64, -1), torch.from_numpy(targets), torch.from_numpy(in_len),
                                   torch.from_numpy(tgt_len), C - 1)
    per.sum().backward()
    return acts, targets, in_len, tgt_len, per.detach().numpy(), a64.grad.numpy()


def _run(U, T, wave):
    """nll [4] and the gradient to the logits [4,T,C] from the kernels, with the lattice knob at `wave`"""
    from nemo_amd import _lib, ops
    acts, targets, in_len, tgt_len, _, _ = _case(U, T)
    logp = torch.log_softmax(acts, -1).to(dev).contiguous()
    grad = torch.empty_like(logp)
    prev = _lib.lib.mi355x_ctc_config(wave)
    try:
        nll = ops.ctc_loss(logp, torch.from_numpy(targets).to(dev), torch.from_numpy(in_len).to(dev),
                           torch.from_numpy(tgt_len).to(dev), C - 1, grad=grad)
        torch.cuda.synchronize()
    finally:
        _lib.lib.mi355x_ctc_config(prev)
    g = grad.cpu()
    gx = g - torch.exp(logp.cpu()) * g.sum(-1, keepdim=True)   # log-softmax backward, as test_ctc_known_answers converts
    return nll.cpu().numpy().astype(np.float64), gx.numpy().astype(np.float64)


def _worst(got, ref, tol):
    """largest |got - ref| / (atol + rtol |ref|): <= 1 is what np.allclose accepts; and the largest |got - ref|"""
    err = np.abs(got - ref)
    return float((err / (tol[1] + tol[0] * np.abs(ref))).max()), float(err.max())


@pytest.mark.parametrize("U,T", list(SHAPES))
def test_ctc_loss_every_lattice_form_vs_float64(U, T):
    _, _, _, _, nll_ref, g_ref = _case(U, T)
    assert np.isfinite(nll_ref).all() and (nll_ref[:3] > 0).all() and nll_ref[3] == 0.0 and not g_ref[3].any()
    nll_w, g_w = _run(U, T, 1)
    nll_l, g_l = _run(U, T, 0)
    figures = {}
    for name, (nll, g), (nll_r, g_r) in (("wave", (nll_w, g_w), (nll_ref, g_ref)), ("lds", (nll_l, g_l), (nll_ref, g_ref)),
                                         ("wave-lds", (nll_w, g_w), (nll_l, g_l))):
        figures[name] = _worst(nll, nll_r, NLL_TOL) + _worst(g, g_r, GRAD_TOL)
        print(f"U {U} T {T} {name}: nll worst {figures[name][0]:.3g} of the T = 60 bound, max |err| {figures[name][1]:.3g} "
              f"(nll <= {nll_ref.max():.1f}); grad worst {figures[name][2]:.3g} of the T = 60 bound, max |err| {figures[name][3]:.3g}")
    for nll, g in ((nll_w, g_w), (nll_l, g_l)):
        assert nll[3] == 0.0 and not g[3].any()          # the infeasible utterance: exact zeros
    for name, (w_nll, _, w_grad, _) in figures.items():
        assert w_nll <= 1.0 and w_grad <= 1.0, (name, figures[name])
