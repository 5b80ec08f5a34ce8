"""TEST INFRASTRUCTURE ONLY -- float64 closed forms of the fused relative-position attention of nemo_amd/csrc/attention.hip, with
the conditioning of every output element, and a float32 / bf16 model of the kernels' DOCUMENTED arithmetic.

Layouts are the kernels': qkv [B*T, 3d] (q | k | v thirds, heads of dk lanes), pos [2T-1, d], u / v f32 [d], lens i64 [B].
Inside, everything is [B, H, T, ...] float64.  The only rounding the oracle shares with the kernels is their documented input
rounding qu = bf16(f32(q) + u), qv = bf16(f32(q) + v); after that:

    raw[i, j] = qu_i . k_j + qv_i . p_{T-1+j-i}          s = raw * scale            L = min(T, len[b])
    P[i, j]   = softmax_j(s) over j < L, rows i < L      lse_i = log sum_j exp(s)   (0 beyond L)
    ctx_i     = sum_j P[i, j] * keep[i, j] / (1 - p) * V_j

and the backward in closed form (no autograd; tests/test_attention_host.py pins it against autograd of the reference's literal
pad / view / slice rel_shift):

    dPd = dO V^T     dP = dPd * keep / (1 - p)     delta_i = sum_j P dP = dO_i . ctx_i     dS = P * (dP - delta) * scale
    dqu_i = sum_j dS k_j      dqv_i = sum_j dS p_{c(i,j)}      dk_j = sum_i dS qu_i      dv_j = sum_i P keep / (1-p) dO_i
    dpos_c = sum_{b, i, j: c = T-1+j-i} dS qv_i      dq = dqu + dqv      bias grads = column sums of dqu | dqv over all rows

CONDITIONING of an element = the sum of the magnitudes of the terms of its last contraction.  dS = P * (dP - delta) * scale
cancels (its row sums are zero), so everything downstream of dS uses the PRE-cancellation magnitude
A = P * scale * (|dPd| * keep / (1 - p) + |delta|) in place of |dS|.  delta_i (returned as `sdelta`, to keep it apart from the
backward's delta) = scale * (2 dk + 2) * 2^-24 * max_j (sum |qu . k| + sum |qv . p|): the f32 error bound of a score.

Packed rows: with `cu` (i64 [B+1]) the activation matrices hold utterance b at rows cu[b] .. cu[b] + L - 1; the functions unpack,
compute on the padded grid and return the valid rows, so packed == padded's valid rows by construction of the INPUT handling
only -- the test compares the two.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tools import attn_drop_stats as ADS  # noqa: E402  (the element rule of attn_keep(): not restated here)

F64 = torch.float64
ABQ, ABK = 128, 32     # queries per workgroup, keys per step (attention.hip)


def bf(x):
    return x.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ dropout mask
def _mix32(x: int) -> int:
    return int(ADS.mix32(np.uint64(x & 0xFFFFFFFF)))


def attn_key(key: int, b: int, h: int) -> int:
    """attn_key() of attention.hip: the per-(utterance, head) key of the element rule"""
    return _mix32(_mix32(key ^ ((b * 0x632BE5AB) & 0xFFFFFFFF)) + h * 0x9E3779B9)


def keep_mask(key: int, b: int, h: int, T: int, threshold: int) -> torch.Tensor:
    """bool [T, T]: keep(i, j) of utterance b, head h for ops.Dropout's (key, threshold); no step word"""
    if threshold == 0:
        return torch.ones(T, T, dtype=torch.bool)
    return torch.from_numpy(ADS.keep_mask(attn_key(key, b, h), T, threshold / 2.0 ** 32))


def keep_masks(drop, B, H, T) -> torch.Tensor:
    """bool [B, H, T, T] for an ops.Dropout-like object (key, threshold)"""
    return torch.stack([torch.stack([keep_mask(drop.key, b, h, T, drop.threshold) for h in range(H)]) for b in range(B)])


# ------------------------------------------------------------------------------------------------ layout helpers
def _lens(lens, T):
    return [min(T, max(0, int(x))) for x in lens]


def unpack_rows(x, lens, T, cu):
    """packed [sum L, w] -> padded [B*T, w] (zeros beyond the length); cu = None: x is padded already"""
    if cu is None:
        return x
    B = len(lens)
    out = torch.zeros(B * T, x.shape[1], dtype=x.dtype)
    for b, L in enumerate(_lens(lens, T)):
        out[b * T:b * T + L] = x[int(cu[b]):int(cu[b]) + L]
    return out


def pack_rows(x, lens, T, cu):
    """padded [B*T, w] -> the valid rows in packed order"""
    if cu is None:
        return x
    return torch.cat([x[b * T:b * T + L] for b, L in enumerate(_lens(lens, T))], 0)


def _heads(x, B, T, H, dk):   # [B*T, H*dk] -> [B, H, T, dk]
    return x.reshape(B, T, H, dk).permute(0, 2, 1, 3)


def _rows(x):                 # [B, H, T, dk] -> [B*T, H*dk]
    B, H, T, dk = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * T, H * dk)


def _shift_index(T):
    """c(i, j) = T - 1 + j - i: the oracle's statement of rel_shift (the host test pins it against pad / view / slice)"""
    return (T - 1 + torch.arange(T)[None, :] - torch.arange(T)[:, None])


def _valid(lens, T):
    Lc = torch.tensor(_lens(lens, T))
    m = torch.arange(T)[None] < Lc[:, None]                    # [B, T]
    return m, (m[:, :, None] & m[:, None, :])[:, None]         # rows, [B, 1, T, T] pairs


def _operands(qkv, pos, u, v, lens, B, H, T, dk, cu):
    d = H * dk
    qkv = unpack_rows(qkv, lens, T, cu)
    q32 = qkv[:, :d].float()
    qu = _heads(bf(q32 + u.float()[None]).to(F64), B, T, H, dk)
    qv = _heads(bf(q32 + v.float()[None]).to(F64), B, T, H, dk)
    k = _heads(qkv[:, d:2 * d].to(F64), B, T, H, dk)
    vv = _heads(qkv[:, 2 * d:].to(F64), B, T, H, dk)
    p = pos.to(F64).reshape(2 * T - 1, H, dk).permute(1, 0, 2)   # [H, 2T-1, dk]
    return qu, qv, k, vv, p


# ------------------------------------------------------------------------------------------------ forward
def forward(qkv, pos, u, v, lens, B, H, T, dk, keep=None, p=0.0, cu=None, scale=None):
    """float64 forward.  keep: bool [B, H, T, T] or None.  Returns a dict; row matrices ([rows, d]) are packed when cu is given,
    per-query statistics are always [B, H, T]."""
    scale = 1.0 / math.sqrt(dk) if scale is None else scale
    qu, qv, k, vv, pp = _operands(qkv, pos, u, v, lens, B, H, T, dk, cu)
    idx = _shift_index(T).expand(B, H, T, T)
    ac = qu @ k.transpose(-1, -2)
    G = qv @ pp.transpose(-1, -2)[None]                          # [B, H, T, 2T-1]
    raw = ac + G.gather(-1, idx)
    absraw = qu.abs() @ k.abs().transpose(-1, -2) + (qv.abs() @ pp.abs().transpose(-1, -2)[None]).gather(-1, idx)
    rowm, pair = _valid(lens, T)
    s = (raw * scale).masked_fill(~pair, -float("inf"))
    lse = torch.logsumexp(s, -1)
    lse = torch.where(rowm[:, None, :], lse, torch.zeros((), dtype=F64))
    P = torch.exp(s - torch.where(rowm[:, None, :], lse, torch.zeros((), dtype=F64))[..., None])
    P = torch.where(pair, P, torch.zeros((), dtype=F64))
    kf = torch.ones((), dtype=F64) if keep is None else keep.to(F64) / (1.0 - p)
    Pd = P * kf
    ctx = Pd @ vv
    cond = Pd @ vv.abs()
    sdelta = scale * (2 * dk + 2) * 2.0 ** -24 * absraw.masked_fill(~pair, 0.0).amax(-1)   # [B, H, T]
    pk = lambda x: pack_rows(_rows(x), lens, T, cu)  # noqa: E731
    return dict(B=B, H=H, T=T, dk=dk, scale=scale, p=p, lens=list(lens), cu=cu, qu=qu, qv=qv, k=k, v=vv, pos=pp, raw=raw, P=P,
                Pd=Pd, kf=kf, lse=lse, sdelta=sdelta, ctx_h=ctx, cond_h=cond, ctx=pk(ctx), cond_ctx=pk(cond), qu_rows=pk(qu), qv_rows=pk(qv))


# ------------------------------------------------------------------------------------------------ backward
def backward(f, dO):
    """closed-form float64 backward of forward()'s result for the context gradient dO ([rows, d], packed like the forward)"""
    B, H, T, dk, scale, lens, cu = f["B"], f["H"], f["T"], f["dk"], f["scale"], f["lens"], f["cu"]
    dOh = _heads(unpack_rows(dO, lens, T, cu).to(F64), B, T, H, dk)
    P, kf, qu, qv, k, vv, pp = f["P"], f["kf"], f["qu"], f["qv"], f["k"], f["v"], f["pos"]
    idx = _shift_index(T).expand(B, H, T, T)
    dPd = dOh @ vv.transpose(-1, -2)
    dP = dPd * kf
    delta = (P * dP).sum(-1)                                     # == sum_dv dO * ctx
    dS = P * (dP - delta[..., None]) * scale
    A = P * scale * (dPd.abs() * kf + delta.abs()[..., None])     # pre-cancellation magnitude of dS
    dOO = (dOh * f["ctx_h"]).abs().sum(-1)                       # sum_dv |dO * O|: what a relative error of O moves delta by
    # "delta term" per score: the kernels' delta is sum_dv dO * (O + O_lo) of THEIR context.  O_lo removes the output rounding
    # (what is left is 2^-16 |O|), but not what the bf16 rounding of the probabilities and the f32 score error did to O in
    # front of it: |O_kernel - O| <= (2^-9 + 2 sdelta) cond_ctx <= 2^-8 cond_ctx, element by element -- the forward bound without
    # its output-rounding term.  Hence |delta_kernel - delta| <= 2^-8 sum_dv |dO| cond_ctx + 2^-16 sum_dv |dO O|, and dS moves by
    # P * scale times that.  (The first term was missing from the first derivation; kernel_model exceeded the bound 18x
    # without it at T = 257.)
    dOc = (dOh.abs() * f["cond_h"]).sum(-1)
    E = (2.0 ** -8 * dOc + 2.0 ** -16 * dOO)[..., None] * P * scale
    z = lambda: torch.zeros(B, H, T, 2 * T - 1, dtype=F64)  # noqa: E731
    out = dict(delta=delta, dP=dP, dS=dS, A=A, E=E)
    mats = {}
    for name, W in (("", dS), ("cond_", A), ("dterm_", E)):
        a = name != ""
        ab = (lambda x: x.abs()) if a else (lambda x: x)
        Wg = z().scatter_(-1, idx, W)                            # un-shifted: dG[i, c]
        mats[name + "dqu"] = W @ ab(k)
        mats[name + "dqv"] = Wg @ ab(pp)[None]
        mats[name + "dk"] = W.transpose(-1, -2) @ ab(qu)
        out[name + "dpos"] = (Wg.transpose(-1, -2) @ ab(qv)).sum(0).permute(1, 0, 2).reshape(2 * T - 1, H * dk)
    mats["dv"] = f["Pd"].transpose(-1, -2) @ dOh
    mats["cond_dv"] = f["Pd"].transpose(-1, -2) @ dOh.abs()
    mats["dterm_dv"] = torch.zeros_like(mats["dv"])
    for pre in ("", "cond_", "dterm_"):
        mats[pre + "dq"] = mats[pre + "dqu"] + mats[pre + "dqv"]
    for n, x in mats.items():
        out[n] = pack_rows(_rows(x), lens, T, cu)
    # bias gradients: column sums over every row (rows beyond a length are zero), with the sums' own conditioning
    out["bias_grads"] = torch.cat([_rows(mats["dqu"]).sum(0), _rows(mats["dqv"]).sum(0)])
    out["abs_bias_grads"] = torch.cat([_rows(mats["dqu"]).abs().sum(0), _rows(mats["dqv"]).abs().sum(0)])
    return out


# ------------------------------------------------------------------------------------------------ dS blocks
def n_tiles(T):
    return (T + 31) // 32


def ds_blocks(W, lens, T, packed=False):
    """W [B, H, T, T] (zero outside the valid corner) -> (X [H, B, nT, nT+1, 32, 32], written [H, B, nT, nT+1]): the layout of
    oracle/relpos_blocks_ref.ds_to_blocks, vectorised (the host test compares the two).  X[h][b][it][s][q][cl] = W[b,h,i,j] at
    i = 32 it + q, T-1+j-i = T-32 + 32 (s-it) + cl.  `written` is relpos_blocks_ref's rule (slots 0 .. ceil(L/32) of every query
    tile); with packed rows the 128-query workgroups beyond the utterance write nothing."""
    B, H = W.shape[:2]
    nT = n_tiles(T)
    Tq = nT * 32
    Wg = torch.zeros(B, H, Tq, (nT + 1) * 32, dtype=W.dtype)
    # column of X's flattened (s, cl) axis: rel = c - (T-32) + 32 it = j - i + 31 + 32 it = j + 31 - q
    i = torch.arange(T)
    rel = (torch.arange(T)[None, :] + 31 - (i % 32)[:, None]).expand(B, H, T, T)
    Wg[:, :, :T].scatter_(-1, rel, W)
    X = Wg.reshape(B, H, nT, 32, nT + 1, 32).permute(1, 0, 2, 4, 3, 5).contiguous()
    written = torch.zeros(H, B, nT, nT + 1, dtype=torch.bool)
    for b, L in enumerate(_lens(lens, T)):
        nkt = (L + 31) // 32
        n_it = nT if not packed else min(nT, 4 * ((L + ABQ - 1) // ABQ))
        written[:, b, :n_it, :nkt + 1] = True
    return X, written


def dpos_from_blocks(X, written, qv, T):
    """plain float64 product of GIVEN blocks with qv [B, H, T, dk] -> (dpos [2T-1, H*dk], sum of |term|, number of terms per
    position [2T-1]); unwritten blocks are skipped, rows of qv past T are clamped (their X rows are zero)"""
    H, B, nT = X.shape[:3]
    dk = qv.shape[-1]
    rows = torch.clamp(torch.arange(nT * 32), max=T - 1)
    qt = qv.to(F64)[:, :, rows].reshape(B, H, nT, 32, dk).permute(1, 0, 2, 3, 4)        # [H, B, nT, 32, dk]
    Xw = torch.where(written[..., None, None], X.to(F64), torch.zeros((), dtype=F64))
    out = torch.zeros(2 * T - 1 + 64 * (nT + 1), H, dk, dtype=F64)
    cond = torch.zeros_like(out)
    nterm = torch.zeros(out.shape[0], dtype=F64)
    base = 32 * nT      # offset that keeps every c0 + cl non-negative
    for it in range(nT):
        for s in range(nT + 1):
            c0 = T - 32 + 32 * (s - it) + base
            blk = torch.einsum("hbqc,hbqd->chd", Xw[:, :, it, s], qt[:, :, it])
            ablk = torch.einsum("hbqc,hbqd->chd", Xw[:, :, it, s].abs(), qt[:, :, it].abs())
            out[c0:c0 + 32] += blk
            cond[c0:c0 + 32] += ablk
            nterm[c0:c0 + 32] += 32.0 * float(written[0, :, it, s].sum())
    sl = slice(base, base + 2 * T - 1)
    return out[sl].reshape(2 * T - 1, H * dk), cond[sl].reshape(2 * T - 1, H * dk), nterm[sl]


# ------------------------------------------------------------------------------------------------ kernel model
def kernel_model(qkv, pos, u, v, lens, B, H, T, dk, dO=None, keep=None, p=0.0, scale=None, rescale_tiles=None):
    """float32 / bf16 restatement of the kernels' DOCUMENTED arithmetic (not of their loops) -- used on the CPU only, to check
    that the per-element bounds of tests/test_attention_kernels_gpu.py hold for an implementation that does exactly what the
    comments of attention.hip say, and to show what a restated defect does to them.  Never a reference for the GPU.

      * scores in f32 from the bf16 operands; P = exp2(raw c2 - m c2) relative to a LAZY reference maximum m: per group of 32
        queries (a wave) and per tile of 32 keys, m moves to max(m, tile max) -- and the accumulators are re-scaled -- only
        when some query of the group finds a score more than tau = 8 / c2 above its own m;
      * the row sum is taken from the unrounded P, P is rounded to bf16 in front of P.V and in front of dV;
      * O = acc / l in f32, stored as bf16 with the rounding residual O_lo = bf16(O - bf16(O));
      * delta = sum dO * (O + O_lo) in f32; P of the backward = exp(s - lse); dS = P * (keep dP / (1-p) - delta) * scale rounded
        to bf16 in front of dQu, dQv, dK and in the dS blocks; bf16 outputs.

    rescale_tiles: the number of 32-column accumulator tiles the re-scale multiplies (None = all dk / 32 of them: the documented
    rule).  Returns a dict with `rescales` = re-scales after key tile 0, [B, H, ceil(T / 32)] (per wave),
    and `later_tiles` [B, ceil(T / 32)] = the FULL key tiles after tile 0 that a wave with valid queries walks (a last tile
    that holds a key or two tops the maximum over the 32 keys of the tile before it by less than a full stair step)."""
    scale = 1.0 / math.sqrt(dk) if scale is None else scale
    f32 = torch.float32
    qu, qv, k, vv, pp = (x.to(f32) for x in _operands(qkv, pos, u, v, lens, B, H, T, dk, None))
    idx = _shift_index(T).expand(B, H, T, T)
    raw = qu @ k.transpose(-1, -2) + (qv @ pp.transpose(-1, -2)[None]).gather(-1, idx)
    rowm, pair = _valid(lens, T)
    c2 = float(np.float32(scale * 1.4426950408889634))
    tau = float(np.float32(8.0) / np.float32(c2))
    nW = n_tiles(T)
    Tq = nW * 32
    kp = torch.ones(B, H, T, T, dtype=f32) if keep is None else keep.to(f32)
    m = torch.full((B, H, Tq), -float("inf"), dtype=f32)
    l = torch.zeros(B, H, Tq, dtype=f32)
    o = torch.zeros(B, H, Tq, dk, dtype=f32)
    resc = torch.zeros(B, H, nW, dtype=torch.int64)
    ncol = dk if rescale_tiles is None else 32 * rescale_tiles
    rawp = torch.full((B, H, Tq, T), -float("inf"), dtype=f32)
    rawp[:, :, :T] = raw.masked_fill(~pair, -float("inf"))
    kpp = torch.zeros(B, H, Tq, T, dtype=f32)
    kpp[:, :, :T] = kp
    Lmax = max(_lens(lens, T))
    for t in range((Lmax + ABK - 1) // ABK):
        j0, j1 = t * ABK, min(T, (t + 1) * ABK)
        st = rawp[..., j0:j1]
        mx = st.amax(-1)
        trig = (mx > m + tau).reshape(B, H, nW, 32).any(-1)                       # wave-uniform decision
        trig_q = trig[..., None].expand(B, H, nW, 32).reshape(B, H, Tq)
        m_new = torch.maximum(m, mx)
        alpha = torch.where(m_new == -float("inf"), torch.ones((), dtype=f32), torch.exp2((m - m_new) * c2))
        alpha = torch.where(trig_q, alpha, torch.ones((), dtype=f32))
        l = l * alpha
        o[..., :ncol] = o[..., :ncol] * alpha[..., None]
        m = torch.where(trig_q, m_new, m)
        if t > 0:
            Lb = torch.tensor(_lens(lens, T))
            live = (j0 < Lb)[:, None, None] & (torch.arange(nW)[None, None] * 32 < Lb[:, None, None])
            resc += (trig & live).to(torch.int64)
        mc = torch.where(m == -float("inf"), torch.zeros((), dtype=f32), m * c2)
        pt = torch.exp2(st * c2 - mc[..., None])
        l = l + pt.sum(-1)
        o = o + bf(pt * kpp[..., j0:j1]).to(f32) @ vv[:, :, j0:j1]
    qvalid = torch.zeros(B, H, Tq, dtype=torch.bool)
    qvalid[:, :, :T] = rowm[:, None, :].expand(B, H, T)
    inv = torch.where(qvalid & (l > 0), float(np.float32(1.0 / (1.0 - p))) / l, torch.zeros((), dtype=f32))
    O = (o * inv[..., None])[:, :, :T]
    lse = torch.where(qvalid, m * float(np.float32(scale)) + torch.log(l), torch.zeros((), dtype=f32))[:, :, :T]
    ctx = bf(O)
    ctx_lo = bf(O - ctx.to(f32))
    Lb = torch.tensor(_lens(lens, T))
    later = ((torch.arange(2, nW + 1)[None, None] * 32 <= Lb[:, None, None]) & (torch.arange(nW)[None, :, None] * 32 < Lb[:, None, None])).sum(-1)
    out = dict(ctx=_rows(ctx), ctx_lo=_rows(ctx_lo), lse=lse, rescales=resc, later_tiles=later)   # later: [B, waves]
    if dO is None:
        return out
    dOh = _heads(dO.to(f32), B, T, H, dk)
    delta = (dOh * ctx.to(f32)).sum(-1) + (dOh * ctx_lo.to(f32)).sum(-1)
    Pb = torch.where(pair, torch.exp(raw * float(np.float32(scale)) - lse[..., None]), torch.zeros((), dtype=f32))
    ks = float(np.float32(scale / (1.0 - p)))
    dPd = dOh @ vv.transpose(-1, -2)
    dS = bf(Pb * (dPd * kp * ks - (delta * float(np.float32(scale)))[..., None])).to(f32)
    dSg = torch.zeros(B, H, T, 2 * T - 1, dtype=f32).scatter_(-1, idx, dS)
    dqu, dqv = dS @ k, dSg @ pp[None]
    out.update(delta=delta, dS=dS, dqu=_rows(bf(dqu)), dqv=_rows(bf(dqv)), dq=_rows(bf(dqu + dqv)),
               dk=_rows(bf(dS.transpose(-1, -2) @ qu)),
               dv=_rows(bf((bf(Pb * kp).to(f32).transpose(-1, -2) @ dOh) * float(np.float32(1.0 / (1.0 - p))))),
               dpos=(dSg.transpose(-1, -2) @ bf(qv).to(f32)).sum(0).permute(1, 0, 2).reshape(2 * T - 1, H * dk),
               bias_grads=torch.cat([_rows(dqu).sum(0), _rows(dqv).sum(0)]))
    return out


# ------------------------------------------------------------------------------------------------ inputs, cases and bounds
# (shared by tests/test_attention_host.py, which validates them on the CPU, and tests/test_attention_kernels_gpu.py)
AMP = 0.5   # std of the random part of q, k and pos: keeps sdelta <= 2^-10 in every regime below (asserted by the host test)
REGIMES = ("plain", "stair-up", "stair-down", "spike", "uniform-row", "shifted-down")


def inputs(B, H, T, dk, regime="plain", seed=0):
    """bf16 operands of one problem (padded layout).  A shift of n nats per score = n / 4 added to every lane of a key, against
    q + 4 e (e = 1 / sqrt(dk) in every lane): sum_lanes 4 e * n / 4 * scale = n."""
    assert regime in REGIMES
    d = H * dk
    g = torch.Generator().manual_seed(7919 * T + 131 * dk + 17 * B + H + 1000003 * seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    q, k, vv, pos = AMP * r(B * T, d), AMP * r(B * T, d), r(B * T, d), AMP * r(2 * T - 1, d)
    u, v, dO = 0.3 * r(d), 0.3 * r(d), r(B * T, d)
    e = 1.0 / math.sqrt(dk)
    tile = (torch.arange(B * T) % T // ABK).double()[:, None]
    if regime != "plain" and regime != "uniform-row":
        # the random parts of q and of u are centred over every head's lanes, so that a constant added to the lanes of a key moves
        # the score of EVERY query by the stated number of nats (otherwise by n * (1 + N(0, 1) * AMP / 4 ...): a wave holding a
        # single query would step over the re-scale threshold or not by chance)
        q = (q.view(B * T, H, dk) - q.view(B * T, H, dk).mean(-1, keepdim=True)).reshape(B * T, d) + 4 * e
        u = (u.view(H, dk) - u.view(H, dk).mean(-1, keepdim=True)).reshape(d)
    if regime == "stair-up":
        k = k + tile * 1.5                      # + 6 nats per key tile: above the 5.55-nat re-scale threshold
    elif regime == "stair-down":
        k = k + (4 - tile) * 1.5                # tile 0 dominates, later probabilities near underflow
    elif regime == "spike":
        k[(torch.arange(B * T) % T) == 100] += 3.0    # + 12 nats at key 100 of every utterance
    elif regime == "shifted-down":
        k = k - 2.0                             # every score near - 8 nats
    elif regime == "uniform-row":
        u, v = torch.zeros(d), torch.zeros(d)
        q[(torch.arange(B * T) % T) % 32 == 7] = 0.0   # one query per 32-query tile: exactly uniform attention, dS cancels
    return dict(qkv=bf(torch.cat([q.float(), k.float(), vv], 1)), pos=bf(pos), u=u.float(), v=v.float(), dO=bf(dO))


def pack_inputs(z, lens, T):
    """the packed-row form of padded inputs: (inputs with the valid rows only, cu)"""
    Ls = _lens(lens, T)
    cu = torch.tensor([0] + list(np.cumsum(Ls)), dtype=torch.int64)
    out = dict(z)
    for n in ("qkv", "dO"):
        out[n] = pack_rows(z[n], lens, T, cu)
    return out, cu


def bounds(f, g=None):
    """the per-element bounds of the GPU suite (float64 tensors shaped like the outputs); origins in the header of
    tests/test_attention_kernels_gpu.py"""
    e8 = 2.0 ** -8
    b = dict(ctx=e8 * f["cond_ctx"] + e8 * f["ctx"].abs(),
             ctx_sum=e8 * f["cond_ctx"] + 2.0 ** -15 * f["ctx"].abs(),
             lse=f["sdelta"] + 8 * 2.0 ** -24 * torch.clamp(f["lse"].abs(), min=1.0))
    if g is not None:
        for n in ("dqu", "dqv", "dq", "dk", "dv"):
            b[n] = e8 * g["cond_" + n] + e8 * g[n].abs() + g["dterm_" + n]
        b["dS"] = e8 * g["dS"].abs() + e8 * g["A"] + g["E"]
        b["dpos"] = e8 * g["cond_dpos"] + g["dterm_dpos"]
    return b


def worst(got, ref, bound):
    """(worst |got - ref| / bound, flat index); an element with a zero bound must be matched exactly"""
    err = (got.double() - ref).abs()
    ratio = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones((), dtype=F64)),
                        torch.where(err == 0, torch.zeros((), dtype=F64), torch.full((), float("inf"), dtype=F64)))
    ratio = torch.where(torch.isnan(err), torch.full((), float("inf"), dtype=F64), ratio).flatten()
    if ratio.numel() == 0:
        return 0.0, -1
    i = int(ratio.argmax())
    return ratio[i].item(), i


# (T, lengths, H) of the geometry sweep, B = 3; every one runs at both head widths
GEOMETRY = ((1, (1, 1, 1), 2), (1, (1, 1, 1), 1), (31, (31, 30, 1), 2), (32, (32, 31, 1), 2), (33, (33, 32, 1), 2),
            (33, (33, 32, 1), 1), (127, (127, 96, 97), 2), (128, (128, 96, 97), 2), (129, (129, 96, 97), 2),
            (129, (129, 128, 1), 2), (161, (161, 160, 33), 2), (161, (166, 0, 161), 2), (257, (257, 193, 225), 2))
REGIME_T, REGIME_LENS = 161, (161, 97, 33)
DROP_P = (0.1, 0.25)


def all_cases():
    """(B, H, T, dk, lens, regime, p) of every case of tests/test_attention_kernels_gpu.py that is judged against the oracle"""
    out = []
    for dk in (64, 128):
        for T, lens, H in GEOMETRY:
            out.append((3, H, T, dk, lens, "plain", 0.0))
        for reg in REGIMES[1:]:
            out.append((3, 2, REGIME_T, dk, REGIME_LENS, reg, 0.0))
        for p in DROP_P:
            out.append((3, 2, REGIME_T, dk, REGIME_LENS, "plain", p))
        out.append((3, 2, 161, dk, (161, 97, 1), "plain", 0.0))         # packed rows
    for B in (8, 9):
        out.append((B, 1, 45, 64, tuple(45 - 3 * b for b in range(B)), "plain", 0.0))   # dpos batch chunks
    return out


def prefill(n, seed):
    """what a `+=` output holds before the call"""
    return torch.randn(n, generator=torch.Generator().manual_seed(4242 + seed))


# Per-column error of a float32 column sum against float64, relative to |prefill| + sum |term|: measured the project's way (the
# same sums by float32 torch.sum on the CPU, worst column over every case of all_cases() (the dropout cases without their mask), `python tests/test_attention_kernels_gpu.py`)
# and 8x that for a kernel that adds in another order:   measured 1.07e-07 -> bound 8.6e-07
TOL_COL = 8.6e-7


def bias_bound(g, pre, tol=None):
    """bound of bias_grads (f32 [2d] += column sums of dQu | dQv): the summation error tol * (|prefill| + sum |term|) plus what
    the TERMS are allowed to be off by -- the kernel sums its own f32 dQu / dQv, whose elements carry the bf16 rounding of dS and
    the delta term like the outputs do (without the outputs' own rounding): column sums of 2^-8 cond + delta term.  (The second
    part was missing from the first derivation: kernel_model, which sums in float64, exceeded the first part alone.)"""
    tol = TOL_COL if tol is None else tol
    terms = torch.cat([(2.0 ** -8 * g["cond_dqu"] + g["dterm_dqu"]).sum(0), (2.0 ** -8 * g["cond_dqv"] + g["dterm_dqv"]).sum(0)])
    return tol * (pre.double().abs() + g["abs_bias_grads"]) + terms


def measure_column_sums():
    """the figure TOL_COL is derived from"""
    w = 0.0
    for c in all_cases():
        B, H, T, dk, lens, regime, p = c
        z = inputs(B, H, T, dk, regime)
        f = forward(z["qkv"], z["pos"], z["u"], z["v"], lens, B, H, T, dk)
        g = backward(f, z["dO"])
        terms = torch.cat([g["dqu"], g["dqv"]], 1)
        pre = prefill(terms.shape[1], 1)
        s32 = torch.cat([pre[None], terms.float()], 0).sum(0)
        e = (s32.double() - (pre.double() + terms.float().double().sum(0))).abs() / (pre.double().abs() + terms.abs().sum(0))
        w = max(w, e.max().item())
    return w
