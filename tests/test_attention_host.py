"""CPU checks of the attention test infrastructure (tests/attention_oracle.py): the float64 oracle against float64 autograd of
the reference's literal formulation, packed against padded rows, the restated dropout mask, and -- on every case the GPU suite
runs -- that the inputs reach the path they are named after and that a float32 / bf16 implementation of the kernels' documented
arithmetic (`kernel_model`) stays inside every per-element bound of tests/test_attention_kernels_gpu.py.  No GPU needed.
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import attention_oracle as AO  # noqa: E402
from oracle import relpos_blocks_ref as RB  # noqa: E402
from tools import attn_drop_stats as ADS  # noqa: E402

F64 = torch.float64


class _Drop:   # ops.Dropout's arithmetic (nemo_amd/ops.py) without importing the native library
    def __init__(self, p, seed, site):
        self.key = (seed * 0x9E3779B1 + site * 0x85EBCA77 + 0x1234567) & 0xFFFFFFFF
        self.threshold = max(1, min(0xFFFFFFFF, int(p * 4294967296.0)))
        self.scale = 1.0 / (1.0 - p)


# ------------------------------------------------------------------------------------------------ the literal reference
def rel_shift(x):
    """multi_head_attention.py:259-270, literally: pad one column on the left, view, drop the first row, view back"""
    b, h, qlen, pos_len = x.size()
    x = torch.nn.functional.pad(x, pad=(1, 0))
    x = x.view(b, h, -1, qlen)
    x = x[:, :, 1:].view(b, h, qlen, pos_len)
    return x


def literal(qu, qv, k, v, pos, lens, T, dk, keepf):
    """RelPositionMultiHeadAttention.forward + forward_attention in float64 on [B, H, T, dk] leaves (pos [H, 2T-1, dk]); the pad
    mask is the outer "or" of the two length masks, as the encoder builds it"""
    matrix_ac = torch.matmul(qu, k.transpose(-2, -1))
    matrix_bd = torch.matmul(qv, pos[None].transpose(-2, -1))
    matrix_bd = rel_shift(matrix_bd)[:, :, :, :T]
    scores = (matrix_ac + matrix_bd) / math.sqrt(dk)
    valid = torch.arange(T)[None] < torch.tensor(lens).clamp(max=T)[:, None]
    mask = ~(valid[:, :, None] & valid[:, None, :])[:, None]
    scores = scores.masked_fill(mask, -10000.0)
    attn = torch.softmax(scores, dim=-1).masked_fill(mask, 0.0)
    return torch.matmul(attn * keepf, v), attn


def _rel(a, b):
    return ((a - b).abs().max() / (b.abs().max() + 1e-300)).item()


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("T,lens", [(1, (1, 1)), (5, (5, 3)), (33, (33, 17)), (45, (45, 30))])
def test_oracle_matches_autograd_of_the_literal_reference(T, lens, drop):
    B, H, dk = 2, 2, 64
    z = AO.inputs(B, H, T, dk, seed=3)
    keep = AO.keep_masks(_Drop(0.25, 5, 9), B, H, T) if drop else None
    p = 0.25 if drop else 0.0
    f = AO.forward(z["qkv"], z["pos"], z["u"], z["v"], lens, B, H, T, dk, keep=keep, p=p)
    g = AO.backward(f, z["dO"])
    leaves = [f[n].clone().requires_grad_(True) for n in ("qu", "qv", "k", "v", "pos")]
    kf = torch.ones((), dtype=F64) if keep is None else keep.to(F64) / (1 - p)
    ctx, attn = literal(*leaves, lens, T, dk, kf)
    # rows beyond the length: the reference leaves a uniform row over masked keys (-10000 everywhere) times zero = 0
    ctx_rows = AO._rows(ctx)
    ctx_rows.backward(z["dO"].to(F64))
    assert _rel(f["ctx"], ctx_rows.detach()) < 1e-12
    assert _rel(f["P"], attn.detach()) < 1e-12
    got = dict(dqu=g["dqu"], dqv=g["dqv"], dk=g["dk"], dv=g["dv"])
    for n, leaf in zip(("dqu", "dqv", "dk", "dv"), leaves):
        assert _rel(got[n], AO._rows(leaf.grad)) < 1e-12, n
    assert _rel(g["dpos"], leaves[4].grad.permute(1, 0, 2).reshape(2 * T - 1, H * dk)) < 1e-12
    assert _rel(g["dq"], AO._rows(leaves[0].grad + leaves[1].grad)) < 1e-12
    assert _rel(g["bias_grads"], torch.cat([AO._rows(leaves[0].grad).sum(0), AO._rows(leaves[1].grad).sum(0)])) < 1e-12
    assert _rel(g["delta"], (AO._heads(z["dO"].to(F64), B, T, H, dk) * f["ctx_h"]).sum(-1)) < 1e-12
    # lse against the masked logsumexp of the literal scores
    s = (f["raw"] * f["scale"])
    for b in range(B):
        L = min(T, lens[b])
        assert _rel(f["lse"][b, :, :L], torch.logsumexp(s[b, :, :L, :L], -1)) < 1e-12
        assert (f["lse"][b, :, L:] == 0).all() and (f["ctx_h"][b, :, L:] == 0).all()


def test_zero_length_and_overlong_utterances():
    B, H, T, dk = 3, 1, 9, 64
    z = AO.inputs(B, H, T, dk)
    f = AO.forward(z["qkv"], z["pos"], z["u"], z["v"], (12, 0, 9), B, H, T, dk)
    g = AO.backward(f, z["dO"])
    f9 = AO.forward(z["qkv"], z["pos"], z["u"], z["v"], (9, 0, 9), B, H, T, dk)
    assert torch.equal(f["ctx"], f9["ctx"]) and torch.isfinite(f["ctx"]).all()
    assert (f["ctx"][T:2 * T] == 0).all() and (f["lse"][1] == 0).all()
    for n in ("dqu", "dqv", "dk", "dv"):
        assert (g[n][T:2 * T] == 0).all() and torch.isfinite(g[n]).all()


def test_packed_rows_equal_padded_rows():
    B, H, T, dk, lens = 3, 2, 37, 64, (37, 20, 1)
    z = AO.inputs(B, H, T, dk)
    zp, cu = AO.pack_inputs(z, lens, T)
    assert zp["qkv"].shape[0] == sum(lens)
    f, fp = (AO.forward(x["qkv"], x["pos"], x["u"], x["v"], lens, B, H, T, dk, cu=c) for x, c in ((z, None), (zp, cu)))
    g, gp = AO.backward(f, z["dO"]), AO.backward(fp, zp["dO"])
    for n in ("ctx", "cond_ctx"):
        assert torch.equal(fp[n], AO.pack_rows(f[n], lens, T, cu)), n
    assert torch.equal(fp["lse"], f["lse"])
    for n in ("dqu", "dqv", "dq", "dk", "dv", "cond_dqu", "cond_dk", "cond_dv", "dterm_dk"):
        assert torch.equal(gp[n], AO.pack_rows(g[n], lens, T, cu)), n
    for n in ("dpos", "bias_grads", "delta", "dS"):
        assert torch.equal(gp[n], g[n]), n


def test_ds_blocks_match_the_block_reference():
    B, H, T, dk, lens = 2, 2, 45, 64, (45, 30)
    z = AO.inputs(B, H, T, dk)
    f = AO.forward(z["qkv"], z["pos"], z["u"], z["v"], lens, B, H, T, dk)
    g = AO.backward(f, z["dO"])
    X, wr = AO.ds_blocks(g["dS"], lens, T)
    Xr, wrr = RB.ds_to_blocks(g["dS"].numpy(), lens)
    assert np.array_equal(X.numpy(), Xr) and np.array_equal(wr.numpy(), wrr)
    dp, cond, nterm = AO.dpos_from_blocks(X, wr, f["qv"], T)
    assert _rel(dp, g["dpos"]) < 1e-12
    assert (cond >= dp.abs() * (1 - 1e-12)).all() and nterm.max() <= 32 * B * 2 * 2


# ------------------------------------------------------------------------------------------------ dropout mask
@pytest.mark.parametrize("p", AO.DROP_P)
def test_keep_mask_is_the_tool_s_mask_and_has_the_right_rate(p):
    drop = _Drop(p, 5, 9)
    for T in (45, 128, 161):
        for b, h in ((0, 0), (2, 1)):
            akey = AO.attn_key(drop.key, b, h)
            # the key derivation restated with Python integers, against attention.hip's attn_key()
            m = lambda x: int(ADS.mix32(np.uint64(x)))  # noqa: E731
            assert akey == m((m(drop.key ^ (b * 0x632BE5AB % 2 ** 32)) + h * 0x9E3779B9) % 2 ** 32)
            assert np.array_equal(AO.keep_mask(drop.key, b, h, T, drop.threshold).numpy(), ADS.keep_mask(akey, T, p))
    for T, lens, B, H in ((45, (45, 30), 2, 2), (128, (128, 100), 2, 2), (161, AO.REGIME_LENS, 3, 2)):
        keep = AO.keep_masks(drop, B, H, T)
        used = torch.cat([keep[b, :, :L, :L].flatten() for b, L in enumerate(lens)])
        n = used.numel()
        rate = used.double().mean().item()
        print(f"p = {p}, T = {T}: keep rate {rate:.5f} over {n} elements (3 / sqrt(n) = {3 / math.sqrt(n):.5f})")
        assert abs(rate - (1 - p)) <= 3 / math.sqrt(n)


# ------------------------------------------------------------------------------------------------ GPU cases on the CPU
@functools.lru_cache(maxsize=None)
def solved(B, H, T, dk, lens, regime, p, rescale_tiles=None):
    z = AO.inputs(B, H, T, dk, regime)
    keep = AO.keep_masks(_Drop(p, 5, 9), B, H, T) if p else None
    f = AO.forward(z["qkv"], z["pos"], z["u"], z["v"], lens, B, H, T, dk, keep=keep, p=p)
    g = AO.backward(f, z["dO"])
    m = AO.kernel_model(z["qkv"], z["pos"], z["u"], z["v"], lens, B, H, T, dk, dO=z["dO"], keep=keep, p=p, rescale_tiles=rescale_tiles)
    return f, g, m


def ratios(f, g, m):
    b = AO.bounds(f, g)
    r = {n: AO.worst(m[n], (f if n in ("ctx", "lse") else g)[n], b[n])[0] for n in ("ctx", "lse", "dS", "dqu", "dqv", "dq", "dk", "dv", "dpos")}
    pre = AO.prefill(2 * f["H"] * f["dk"], 1)
    r["bias_grads"] = AO.worst(pre.double() + m["bias_grads"].double(), pre.double() + g["bias_grads"], AO.bias_bound(g, pre))[0]
    r["ctx_sum"] = AO.worst(m["ctx"].double() + m["ctx_lo"].double(), f["ctx"], b["ctx_sum"])[0]
    return r


@pytest.mark.parametrize("case", AO.all_cases(), ids=lambda c: "B%d-H%d-T%d-dk%d-%s-%s-p%s" % (c[0], c[1], c[2], c[3], "_".join(map(str, c[4])), c[5], c[6]))
def test_gpu_cases_reach_their_path_and_the_bounds_hold_for_the_documented_arithmetic(case):
    B, H, T, dk, lens, regime, p = case
    f, g, m = solved(*case)
    sd = f["sdelta"].max().item()
    resc, later = m["rescales"], m["later_tiles"]
    print(f"{case}: sdelta {sd * 1024:.3f} x 2^-10; re-scales after tile 0: {int(resc.sum())} (waves x later full tiles: {int(later.sum()) * H})")
    assert sd <= 2.0 ** -10
    if regime == "plain" and p == 0.0:
        assert int(resc.sum()) == 0
    if regime == "stair-up":
        assert (resc >= later[:, None, :]).all() and int(later.sum()) > 0
    if regime in ("stair-down", "shifted-down", "uniform-row"):
        assert int(resc.sum()) == 0
    r = ratios(f, g, m)
    print("   worst kernel_model / bound: " + "  ".join(f"{n} {v:.3f}" for n, v in r.items()))
    assert max(r.values()) <= 1.0, r
    if regime == "uniform-row":   # the rows are uniform and their dS cancels, to float64 rounding
        for b, L in enumerate(lens):
            rows = [i for i in range(L) if i % 32 == 7]
            assert (f["raw"][b, :, rows, :L] == 0).all() and ((f["P"][b, :, rows, :L] * L - 1).abs() <= 2.0 ** -48).all()
            assert g["dS"][b, :, rows].sum(-1).abs().max() <= 2.0 ** -44 * g["A"][b, :, rows].sum(-1).max()


def test_a_rescale_that_skips_accumulator_columns_breaks_the_bound():
    """the defect this suite was written to decide (the forward's re-scale multiplying two of the four 32-column accumulator
    tiles at head width 128), restated in kernel_model: the stair-up case exceeds the context bound by orders of magnitude in
    columns 64.. and nowhere else, the plain case does not notice"""
    case = (3, 2, AO.REGIME_T, 128, AO.REGIME_LENS, "stair-up", 0.0)
    f, g, good = solved(*case)
    _, _, bad = solved(*case, rescale_tiles=2)
    b = AO.bounds(f)
    rg, rb = AO.worst(good["ctx"], f["ctx"], b["ctx"]), AO.worst(bad["ctx"], f["ctx"], b["ctx"])
    col = rb[1] % 256 % 128
    err = (bad["ctx"].double() - f["ctx"]).abs().amax(1).max().item()
    print(f"stair-up, d_k = 128: worst ratio {rg[0]:.3f} with the documented rule, {rb[0]:.1f} with columns 64.. not re-scaled "
          f"(head column {col}, worst row error {err:.3f})")
    assert rg[0] <= 1.0 and rb[0] > 10.0 and col >= 64
    lo = bad["ctx"].double().reshape(-1, 2, 128)[..., :64].reshape(-1, 128)
    assert AO.worst(lo, f["ctx"].reshape(-1, 2, 128)[..., :64].reshape(-1, 128), b["ctx"].reshape(-1, 2, 128)[..., :64].reshape(-1, 128))[0] <= 1.0
    plain = (3, 2, AO.REGIME_T, 128, AO.REGIME_LENS, "plain", 0.0)
    fp, _, _ = solved(*plain)
    _, _, bp = solved(*plain, rescale_tiles=2)
    assert AO.worst(bp["ctx"], fp["ctx"], AO.bounds(fp)["ctx"])[0] <= 1.0
