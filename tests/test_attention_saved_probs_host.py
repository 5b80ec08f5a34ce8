"""CPU: the "saved probabilities" attention backward (mi355x_relpos_flash_fwd_p / _bwd_dq_p / _bwd_dkv_p, include/mi355x_asr.h)
restated in float32 / bf16 next to the float64 oracle of tests/attention_oracle.py, the way tests/test_attention_host.py restates
the recomputing kernels.

The forward exports, per (query block of 32, key tile of 32), its un-normalised probabilities p~ = exp2((s - mref) c2) as bf16 and
the reference point mref of that step; the backward takes P = bf16(p~) * exp2(mref c2 - lse log2 e) where it used to recompute
P = exp(s - lse).  That is ONE more bf16 rounding of every probability (2^-9 relative), so in the bounds of
tests/test_attention_kernels_gpu.py the terms that multiply `cond` (and `A` for the dS blocks) grow from 2^-8 to 3 * 2^-9 for
dqu, dqv, dq_out, dk, dv and the dS blocks (`bounds_p`); every other term and every forward bound stays.

This file holds what tests/test_attention_saved_probs_gpu.py shares with it: the cases, the widened bounds and the export layout.
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_oracle as AO  # noqa: E402
from test_attention_host import _Drop  # noqa: E402

F64 = torch.float64
SEED, SITE = 5, 9
B_, H_, DK = 2, 2, 64

# (T, lens, regime, p): one query tile with a partial last key tile; two query tiles; more than 6 key tiles (the band ring wraps)
# next to a single-frame utterance; a zero-length utterance; dropout; the regime that re-scales in every later key tile
CASES = ((45, (45, 33), "plain", 0.0), (160, (160, 97), "plain", 0.0), (230, (230, 1), "plain", 0.0), (45, (45, 0), "plain", 0.0),
         (45, (45, 33), "plain", 0.1), (160, (160, 97), "plain", 0.1), (230, (230, 1), "plain", 0.1),
         (160, (160, 97), "stair-up", 0.0), (160, (160, 97), "stair-up", 0.1))
CASE_IDS = ["T%d-%s-%s-p%s" % (c[0], "_".join(map(str, c[1])), c[2], c[3]) for c in CASES]


def nt4(T):
    """32-row blocks each way of the exported grid: padded to whole 128-row workgroups"""
    return 4 * ((T + 127) // 128)


def probs_elems(B, H, T):
    return B * H * nt4(T) * nt4(T) * 1024


def mref_elems(B, H, T):
    return probs_elems(B, H, T) // 32


def _lane_reg_maps():
    """(query-in-block, key-in-tile) of every (lane, register) of an exported block: the forward kernel's accumulator layout"""
    lane, r = torch.arange(64)[:, None], torch.arange(16)[None, :]
    return (lane & 31).expand(64, 16), ((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)).expand(64, 16)


def blocks_to_dense(blocks, B, H, T):
    """probs [B*H, nt4, nt4, 64, 16] -> [B, H, 32 nt4, 32 nt4] (query, key)"""
    n = nt4(T)
    qi, kj = _lane_reg_maps()
    x = blocks.reshape(B, H, n, n, 64, 16)
    out = torch.zeros(B, H, n, n, 32, 32, dtype=x.dtype)
    out[..., qi, kj] = x
    return out.permute(0, 1, 2, 4, 3, 5).reshape(B, H, 32 * n, 32 * n)


def dense_to_blocks(dense, B, H, T):
    n = nt4(T)
    qi, kj = _lane_reg_maps()
    x = dense.reshape(B, H, n, 32, n, 32).permute(0, 1, 2, 4, 3, 5)
    return x[..., qi, kj].reshape(B * H, n, n, 64, 16)


def mref_to_dense(mref, B, H, T):
    """mref [B*H, nt4 (key tile), 32 nt4 (query)] -> [B, H, query, key tile]"""
    n = nt4(T)
    return mref.reshape(B, H, n, 32 * n).permute(0, 1, 3, 2)


def bounds_p(f, g):
    """AO.bounds with the `cond` / `A` factor of the given-P outputs at 3 * 2^-9"""
    b = AO.bounds(f, g)
    e8, e9 = 2.0 ** -8, 2.0 ** -9
    for n in ("dqu", "dqv", "dq", "dk", "dv"):
        b[n] = 3 * e9 * g["cond_" + n] + e8 * g[n].abs() + g["dterm_" + n]
    b["dS"] = e8 * g["dS"].abs() + 3 * e9 * g["A"] + g["E"]
    return b


def exported_P(ptilde, mref, lse, scale, B, H, T):
    """float64 P[b,h,i,j] = p~ * exp(mref * scale - lse) of what a forward exported (dense p~ [B,H,Tq,Tq], mref [B,H,Tq,nt4])"""
    fac = torch.exp(mref[:, :, :T].double() * scale - lse.double()[..., None])            # [B, H, T, nt4]
    fac = fac.repeat_interleave(32, dim=-1)[..., :T]
    return ptilde[:, :, :T, :T].double() * fac


@functools.lru_cache(maxsize=None)
def solved(T, lens, regime, p):
    B, H, dk = B_, H_, DK
    z = AO.inputs(B, H, T, dk, regime)
    keep = AO.keep_masks(_Drop(p, SEED, SITE), B, H, T) if p else None
    f = AO.forward(z["qkv"], z["pos"], z["u"], z["v"], lens, B, H, T, dk, keep=keep, p=p)
    g = AO.backward(f, z["dO"])
    return z, keep, f, g


def model_p(z, keep, lens, B, H, T, dk, p):
    """float32 / bf16 restatement of the DOCUMENTED arithmetic of the three _p kernels (the forward part is AO.kernel_model's
    loop with the export added).  Returns the exported dense p~ / mref and the backward outputs."""
    f32 = torch.float32
    scale = 1.0 / math.sqrt(dk)
    qu, qv, k, vv, pp = (x.to(f32) for x in AO._operands(z["qkv"], z["pos"], z["u"], z["v"], lens, B, H, T, dk, None))
    idx = AO._shift_index(T).expand(B, H, T, T)
    raw = qu @ k.transpose(-1, -2) + (qv @ pp.transpose(-1, -2)[None]).gather(-1, idx)
    rowm, pair = AO._valid(lens, T)
    c2 = float(np.float32(scale * 1.4426950408889634))
    tau = float(np.float32(8.0) / np.float32(c2))
    n = nt4(T)
    Tq = 32 * n
    kp = torch.ones(B, H, T, T, dtype=f32) if keep is None else keep.to(f32)
    m = torch.full((B, H, Tq), -float("inf"), dtype=f32)
    l = torch.zeros(B, H, Tq, dtype=f32)
    rawp = torch.full((B, H, Tq, Tq), -float("inf"), dtype=f32)
    rawp[:, :, :T, :T] = raw.masked_fill(~pair, -float("inf"))
    pt_all = torch.zeros(B, H, Tq, Tq, dtype=f32)
    mref = torch.full((B, H, Tq, n), float("nan"), dtype=f32)
    moved = torch.zeros(B, H, n, dtype=torch.int64)     # key tiles after the first in which a wave's reference point moved
    Ls = AO._lens(lens, T)
    for t in range((max(Ls) + 31) // 32):
        st = rawp[..., 32 * t:32 * t + 32]
        mx = st.amax(-1)
        trig = (mx > m + tau).reshape(B, H, n, 32).any(-1)
        trig_q = trig[..., None].expand(B, H, n, 32).reshape(B, H, Tq)
        m_new = torch.maximum(m, mx)
        alpha = torch.where(m_new == -float("inf"), torch.ones((), dtype=f32), torch.exp2((m - m_new) * c2))
        l = l * torch.where(trig_q, alpha, torch.ones((), dtype=f32))
        m = torch.where(trig_q, m_new, m)
        if t > 0:
            moved += trig.to(torch.int64)
        mc = torch.where(m == -float("inf"), torch.zeros((), dtype=f32), m * c2)
        pt = torch.exp2(st * c2 - mc[..., None])
        l = l + pt.sum(-1)
        pt_all[..., 32 * t:32 * t + 32] = AO.bf(pt).to(f32)          # the export: bf16, before dropout
        mref[..., t] = m
    qvalid = torch.zeros(B, H, Tq, dtype=torch.bool)
    qvalid[:, :, :T] = rowm[:, None, :].expand(B, H, T)
    lse = torch.where(qvalid, m * float(np.float32(scale)) + torch.log(l), torch.zeros((), dtype=f32))[:, :, :T]
    # the forward's context (not exported: identical to AO.kernel_model's) feeds delta
    km = AO.kernel_model(z["qkv"], z["pos"], z["u"], z["v"], lens, B, H, T, dk, dO=z["dO"], keep=keep, p=p)
    delta = km["delta"]
    dOh = AO._heads(z["dO"].to(f32), B, T, H, dk)
    lse2 = lse * float(np.float32(1.4426950408889634))
    fac = torch.exp2(mref[:, :, :T] * c2 - lse2[..., None])                      # [B, H, T, n]
    fac = torch.where(torch.isnan(fac), torch.zeros((), dtype=f32), fac)        # (key tiles beyond the longest utterance)
    Pb = pt_all[:, :, :T, :T] * fac.repeat_interleave(32, dim=-1)[..., :T]
    Pb = torch.where(pair, Pb, torch.zeros((), dtype=f32))
    ks = float(np.float32(scale / (1.0 - p)))
    dPd = dOh @ vv.transpose(-1, -2)
    dS = AO.bf(Pb * (dPd * kp * ks - (delta * float(np.float32(scale)))[..., None])).to(f32)
    dSg = torch.zeros(B, H, T, 2 * T - 1, dtype=f32).scatter_(-1, idx, dS)
    dqu, dqv = dS @ k, dSg @ pp[None]
    R = AO._rows
    return dict(ptilde=pt_all, mref=mref, lse=lse, moved=moved, dS=dS, dqu=R(AO.bf(dqu)), dqv=R(AO.bf(dqv)), dq=R(AO.bf(dqu + dqv)),
                dk=R(AO.bf(dS.transpose(-1, -2) @ qu)),
                dv=R(AO.bf((AO.bf(Pb * kp).to(f32).transpose(-1, -2) @ dOh) * float(np.float32(1.0 / (1.0 - p))))))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_widened_bounds_hold_for_the_documented_given_p_arithmetic(case):
    T, lens, regime, p = case
    z, keep, f, g = solved(*case)
    assert f["sdelta"].max().item() <= 2.0 ** -10
    m = model_p(z, keep, lens, B_, H_, T, DK, p)
    b = bounds_p(f, g)
    r = {n: AO.worst(m[n], g[n], b[n])[0] for n in ("dS", "dqu", "dqv", "dq", "dk", "dv")}
    print(f"{case}: worst model / widened bound: " + "  ".join(f"{n} {v:.3f}" for n, v in r.items()))
    assert max(r.values()) < 1.0, r
    # the export against the float64 forward: p~ with its own reference point and the row's lse IS the probability
    Pg = exported_P(m["ptilde"], m["mref"], m["lse"], f["scale"], B_, H_, T)
    Pg = torch.where(torch.isnan(Pg), torch.zeros((), dtype=F64), Pg)
    rp = AO.worst(Pg, f["P"], 2.0 ** -8 * f["P"])[0]
    print(f"   exported probabilities / (2^-8 |ref|): {rp:.3f}; largest p~ {m['ptilde'].max().item():.1f}; "
          f"reference points moved after tile 0 in {int(m['moved'].sum())} (wave, tile) steps")
    assert rp < 1.0
    assert m["ptilde"].max().item() <= 256.0          # the lazy re-scaling bound
    Ls = AO._lens(lens, T)
    for bi, L in enumerate(Ls):                       # masked keys export exactly 0
        nk = (L + 31) // 32 * 32
        assert (m["ptilde"][bi, :, :, L:nk] == 0).all()
    if regime == "stair-up":
        # + 6 nats per key tile: every wave with valid queries moves its reference point in every later full key tile, and
        # a tile's p~ is useless without the mref of ITS step (the final maximum gives a different matrix)
        assert int(m["moved"].sum()) > 0
        last = m["mref"][:, :, :T, (Ls[0] + 31) // 32 - 1]
        wrong = m["ptilde"][:, :, :T, :T].double() * torch.exp(last.double() * f["scale"] - m["lse"].double())[..., None]
        assert AO.worst(wrong[0], f["P"][0], 2.0 ** -8 * f["P"][0])[0] > 100.0
    else:
        assert int(m["moved"].sum()) == 0


def test_export_layout_is_the_documented_register_order():
    """include/mi355x_asr.h: lane = (query & 31) + 32 * ((key >> 2) & 1), register = (key & 3) + 4 * ((key & 31) >> 3)"""
    B, H, T = 1, 2, 130
    n = nt4(T)
    assert n == 8 and probs_elems(B, H, T) == B * H * 64 * 1024 and mref_elems(B, H, T) == B * H * 8 * 256
    dense = torch.arange(B * H * (32 * n) ** 2, dtype=torch.float64).reshape(B, H, 32 * n, 32 * n)
    blocks = dense_to_blocks(dense, B, H, T)
    assert torch.equal(blocks_to_dense(blocks, B, H, T), dense)
    flat = blocks.flatten()
    for (b, h, i, j) in ((0, 0, 0, 0), (0, 1, 37, 70), (0, 0, 129, 5), (0, 1, 255, 255), (0, 0, 64, 47)):
        lane = (i & 31) + 32 * ((j >> 2) & 1)
        reg = (j & 3) + 4 * ((j & 31) >> 3)
        off = ((((b * H + h) * n + i // 32) * n + j // 32) * 64 + lane) * 16 + reg
        assert flat[off] == dense[b, h, i, j]
    m = torch.arange(B * H * n * 32 * n, dtype=torch.float64)
    md = mref_to_dense(m, B, H, T)
    assert md[0, 1, 70, 3] == ((0 * H + 1) * n + 3) * (32 * n) + 70
