"""-m gpu: the row walk that csrc/rnnt.hip and csrc/tdt.hip share (csrc/transducer_rows.h) on rows NARROWER than its alignment
peel: V1 in {2, 3, 5} gives head = min(V1, peel), no float4 group at all or a single one, and sometimes no tail; an odd V1 puts
consecutive dense rows on every 4-byte phase.  RNN-T (plain; FastEmit + clamp) and TDT, each through the dense f32 entry and
through the pitched entry (row pitch 8) with an f32 and a bf16 gradient, against the float64 oracles."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tdt_oracle as O  # noqa: E402
from oracle import rnnt_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu
dev = "cuda"

B, T, U1, LD = 2, 3, 2, 8
LENS, LABEL_LENS = [3, 2], [1, 0]   # utterance 1 leaves the cells t = 2 and u = 1 padded
DURATIONS, SIGMA = [0, 1], 0.02
RUNS = {"rnnt": dict(), "rnnt_fastemit_clamp": dict(fastemit_lambda=0.3, clamp=0.05), "tdt": None}


@functools.lru_cache(maxsize=None)
def _case(V1, blank, run):
    """inputs (CPU) and the float64 costs [B] and gradient [B, T, U1, W] of one case; W = V1, or V1 + 2 duration logits for TDT"""
    W = V1 + len(DURATIONS) if run == "tdt" else V1
    g = torch.Generator().manual_seed(100 * V1 + 10 * blank + len(run))
    acts = torch.randn(B, T, U1, W, generator=g) * 2.0
    labels = torch.randint(0, V1 - 1, (B, U1 - 1), generator=g)
    labels = labels + (labels >= blank).long()
    lens, ll = torch.tensor(LENS), torch.tensor(LABEL_LENS)
    if run == "tdt":
        rc, rg = O.tdt_loss_and_grad(acts, labels, lens, ll, DURATIONS, blank, SIGMA, "none")
    else:
        rc, rg = RR.rnnt_loss_and_grad(acts, labels, lens, ll, blank=blank, reduction="none", **RUNS[run])
    assert torch.isfinite(rc).all() and torch.isfinite(rg).all()
    return acts, labels, lens, ll, W, rc, rg


def _loss(run, acts, ld, V1, labels, lens, ll, blank, grads, ldg):
    from nemo_amd import ops
    if run == "tdt":
        if ld is None:
            return ops.tdt_loss(acts, labels, lens, ll, blank, DURATIONS, grads=grads, sigma=SIGMA)
        return ops.tdt_loss_pitched(acts, ld, B, T, U1, V1, DURATIONS, labels, lens, ll, blank, grads=grads, ld_grads=ldg, sigma=SIGMA)
    if ld is None:
        return ops.rnnt_loss(acts, labels, lens, ll, blank, grads=grads, **RUNS[run])
    return ops.rnnt_loss_pitched(acts, ld, B, T, U1, V1, labels, lens, ll, blank, grads, ldg, **RUNS[run])


@pytest.mark.parametrize("run", list(RUNS))
@pytest.mark.parametrize("V1,blank", [(V1, blank) for V1 in (2, 3, 5) for blank in (0, V1 - 1)])
def test_rows_narrower_than_the_alignment_peel(V1, blank, run):
    acts, labels, lens, ll, W, rc, rg = _case(V1, blank, run)
    lab, xl, yl = labels.to(dev), lens.to(dev), ll.to(dev)
    n = B * T * U1
    tol = 2e-5 * max(1.0, rg.abs().max().item())

    def check(costs, grads, what):   # grads [B, T, U1, W] f32
        assert torch.allclose(costs.cpu().double(), rc, rtol=2e-5, atol=1e-4), (what, costs, rc)
        err = (grads.cpu().double() - rg).abs().max().item()
        assert err <= tol, (what, err)
        for b in range(B):   # padded cells: exactly zero
            assert (grads[b, LENS[b]:] == 0).all() and (grads[b, :, LABEL_LENS[b] + 1:] == 0).all(), (what, b)

    a = acts.to(dev)
    gd = torch.full_like(a, 7.0)
    cd = _loss(run, a, None, V1, lab, xl, yl, blank, gd, None)
    torch.cuda.synchronize()
    check(cd, gd, "dense")

    ap = torch.full((n, LD), float("nan"), device=dev)
    ap[:, :W] = a.view(n, W)
    for dtype in (torch.float32, torch.bfloat16):
        gp = torch.full((n, LD), 7.0, device=dev, dtype=dtype)
        cp = _loss(run, ap, LD, V1, lab, xl, yl, blank, gp, LD)
        torch.cuda.synchronize()
        assert (gp[:, W:] == 0).all(), (dtype, "pad columns")
        if dtype == torch.float32:
            check(cp, gp[:, :W].reshape(B, T, U1, W), "pitched f32")
            assert torch.allclose(gp[:, :W], gd.view(n, W), rtol=3e-5, atol=1e-7)
            g32 = gp.clone()
        else:
            assert torch.allclose(cp.cpu().double(), rc, rtol=2e-5, atol=1e-4), (dtype, cp, rc)
            assert torch.equal(gp[:, :W], g32[:, :W].to(torch.bfloat16))   # same walk, rounded once
            pad = gp[:, :W].reshape(B, T, U1, W)
            for b in range(B):
                assert (pad[b, LENS[b]:] == 0).all() and (pad[b, :, LABEL_LENS[b] + 1:] == 0).all(), (dtype, b)
