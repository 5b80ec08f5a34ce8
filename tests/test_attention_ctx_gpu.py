"""-m gpu: the windowed rel-pos flash attention of nemo_amd/csrc/attention_ctx.hip (forward, dQ, dK/dV, linear_pos gradient)
through nemo_amd.ops against float64.  The reference is tests/attention_oracle.py with ONE restated function: forward_win() is
AO.forward with `pair &= window(...)`; AO.backward and AO.bounds apply to its result as they are, so every bound is the per-element
bound of tests/test_attention_kernels_gpu.py (its header derives them; nothing there depends on which terms are present),
computed from the windowed reference.  The backward kernels run on the forward kernel's own ctx, ctx_lo and lse.
"""
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_oracle as AO  # noqa: E402

pytestmark = pytest.mark.gpu
dev = "cuda"
F32, BF16, F64, I64 = torch.float32, torch.bfloat16, torch.float64, torch.int64
NAN = float("nan")
REG, CHK = 1, 2   # ctx_style of include/mi355x_asr.h


def window(style, left, right, T):
    """bool [T, T]: query i (row) sees key j -- the rule of include/mi355x_asr.h"""
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    if style == CHK and right >= 0:
        dc = i // (right + 1) - j // (right + 1)
        return (dc >= 0) & ((dc <= left // (right + 1)) if left >= 0 else torch.ones(T, T, dtype=torch.bool))
    return ((j - i >= -left) if left >= 0 else torch.ones(T, T, dtype=torch.bool)) & \
           ((j - i <= right) if right >= 0 else torch.ones(T, T, dtype=torch.bool))


def forward_win(qkv, pos, u, v, lens, B, H, T, dk, win, keep=None, p=0.0):
    """AO.forward (padded rows) with the pairs restricted to the window; same dict keys"""
    scale = 1.0 / math.sqrt(dk)
    qu, qv, k, vv, pp = AO._operands(qkv, pos, u, v, lens, B, H, T, dk, None)
    idx = AO._shift_index(T).expand(B, H, T, T)
    raw = qu @ k.transpose(-1, -2) + (qv @ pp.transpose(-1, -2)[None]).gather(-1, idx)
    absraw = qu.abs() @ k.abs().transpose(-1, -2) + (qv.abs() @ pp.abs().transpose(-1, -2)[None]).gather(-1, idx)
    rowm, pair = AO._valid(lens, T)
    pair = pair & window(*win, T)
    zero = torch.zeros((), dtype=F64)
    s = (raw * scale).masked_fill(~pair, -float("inf"))
    lse = torch.where(rowm[:, None, :], torch.logsumexp(s, -1), zero)
    P = torch.where(pair, torch.exp(s - lse[..., None]), zero)
    kf = torch.ones((), dtype=F64) if keep is None else keep.to(F64) / (1.0 - p)
    Pd = P * kf
    ctx, cond = Pd @ vv, Pd @ vv.abs()
    sdelta = scale * (2 * dk + 2) * 2.0 ** -24 * absraw.masked_fill(~pair, 0.0).amax(-1)
    return dict(B=B, H=H, T=T, dk=dk, scale=scale, p=p, lens=list(lens), cu=None, qu=qu, qv=qv, k=k, v=vv, pos=pp, raw=raw, P=P,
                Pd=Pd, kf=kf, lse=lse, sdelta=sdelta, ctx_h=ctx, cond_h=cond, ctx=AO._rows(ctx), cond_ctx=AO._rows(cond),
                qu_rows=AO._rows(qu), qv_rows=AO._rows(qv))


#        style left right  T    dk  p    (B, H, lens)
CASES = [(REG, 5, 3, 70, 64, 0.0, None),         # window far inside one tile
         (REG, 100, 0, 300, 64, 0.0, None),      # left only: whole waves see nothing in the first visited tile; kt_lo > 0
         (REG, -1, 10, 300, 64, 0.0, None),      # unlimited left, limited right: kt_hi < nkt
         (REG, 40, 40, 300, 128, 0.0, None),     # the second head width
         (CHK, 24, 7, 300, 64, 0.0, None),       # chunk 8 divides the tiles
         (CHK, 70, 13, 300, 64, 0.0, None),      # recipe window: chunk 14 divides neither 32 nor 128
         (CHK, 70, 13, 300, 64, 0.1, None),      # dropout: the mask of the full run restricted to the window
         (CHK, -1, 13, 200, 64, 0.0, None),      # unlimited left chunks
         (REG, 128, 128, 1056, 64, 0.0, (1, 1, (1056,)))]   # above the soft-max kernel's limit: nine query tiles, ring started
                                                            # mid-table, tiles skipped at both ends


@functools.lru_cache(maxsize=None)
def case(style, left, right, T, dk, p, geo):
    """inputs, float64 reference and bounds of one case (computed once, shared, never modified)"""
    from nemo_amd import ops
    B, H, lens = geo or (3, 2, (T, 2 * T // 3 + 1, 1))
    assert geo or lens[1] % 32
    z = AO.inputs(B, H, T, dk)
    drop = ops.Dropout(p, seed=5, site=9)
    keep = AO.keep_masks(drop, B, H, T) if p else None
    f = forward_win(z["qkv"], z["pos"], z["u"], z["v"], lens, B, H, T, dk, (style, left, right), keep, p)
    g = AO.backward(f, z["dO"])
    return dict(B=B, H=H, T=T, dk=dk, d=H * dk, lens=lens, Ls=AO._lens(lens, T), win=(style, left, right), drop=drop, z=z, f=f, g=g,
                bnd=AO.bounds(f, g), pre_bg=AO.prefill(2 * H * dk, 1), pre_dpos=AO.prefill((2 * T - 1) * H * dk, 2).view(2 * T - 1, H * dk))


def nans(*shape, dtype=BF16):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def run(c):
    """forward, prep, dQ (separate and fused outputs, dS blocks), dK/dV, linear_pos gradient -- as the encoder issues them"""
    from nemo_amd import ops
    B, H, T, dk, d, z, win, drop = c["B"], c["H"], c["T"], c["dk"], c["d"], c["z"], c["win"], c["drop"]
    M, Tp, scale = B * T, (T + 7) // 8 * 8, 1.0 / math.sqrt(dk)
    qkv, pos, u, v, dO = (z[n].to(dev) for n in ("qkv", "pos", "u", "v", "dO"))
    lens = torch.tensor(c["lens"], dtype=I64, device=dev)
    o = dict(ctx=nans(M, d), lo=nans(M, d), lse=nans(B, H, T, dtype=F32), delta=nans(B, H, T, dtype=F32), qu=nans(M, d), qv=nans(M, d),
             dqu=nans(M, d), dqv=nans(M, d), dq3=nans(M, 3 * d), bg=c["pre_bg"].to(dev), dqkv=nans(M, 3 * d),
             ds=ops.relpos_ds_buffer(B, H, T, dev, fill=NAN), dpos=c["pre_dpos"].to(dev), dcast=nans(2 * T - 1, d))
    ops.relpos_flash_fwd(qkv, 3 * d, pos, d, u, v, lens, o["ctx"], d, o["lse"], B, H, T, dk, Tp, scale, drop, ctx_lo=o["lo"], ctx=win)
    ops.attn_bwd_prep(dO, o["ctx"], o["delta"], qkv, 3 * d, u, v, o["qu"], o["qv"], B, H, T, d, O_lo=o["lo"], lens=lens)
    ops.relpos_flash_bwd_dq(o["qu"], o["qv"], qkv, 3 * d, pos, d, lens, dO, o["lse"], o["delta"], o["dqu"], o["dqv"], B, H, T, dk,
                            scale, drop, ds_out=o["ds"], dq_out=o["dq3"], ld_dq=3 * d, bias_grads=o["bg"], ctx=win)
    ops.relpos_flash_bwd_dkv(o["qu"], o["qv"], qkv, 3 * d, pos, d, lens, dO, o["lse"], o["delta"], o["dqkv"], 3 * d, B, H, T, dk, Tp,
                             scale, drop, ctx=win)
    ops.relpos_flash_bwd_dpos(o["qv"], o["ds"], lens, o["dpos"], B, H, T, dk, dpos_cast=o["dcast"], ctx=win)
    torch.cuda.synchronize()
    return {n: t.cpu() for n, t in o.items()}


def judge(what, got, ref, bound):
    r, i = AO.worst(got, ref, bound)
    idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(max(i, 0)), ref.shape))
    print(f"{what}: worst |got - ref| / bound {r:.3f} at {idx}")
    assert r <= 1.0, f"{what}: element {idx} is off by {r:.3f} x its bound"


def padded_rows_zero(c, name, x):
    x = x.view(c["B"], c["T"], -1)
    for b, L in enumerate(c["Ls"]):
        assert (x[b, L:] == 0).all(), f"{name}: utterance {b} has non-zero rows beyond its length {L}"


@pytest.mark.parametrize("style,left,right,T,dk,p,geo", CASES)
def test_windowed_kernels_against_float64(style, left, right, T, dk, p, geo):
    c = case(style, left, right, T, dk, p, geo)
    f, g, bnd, d = c["f"], c["g"], c["bnd"], c["d"]
    o = run(c)
    judge("ctx", o["ctx"].float(), f["ctx"], bnd["ctx"])
    judge("ctx + ctx_lo", o["ctx"].double() + o["lo"].double(), f["ctx"], bnd["ctx_sum"])
    judge("lse", o["lse"], f["lse"], bnd["lse"])
    for b, L in enumerate(c["Ls"]):
        assert (o["lse"][b, :, L:] == 0).all(), "lse beyond the length is not zero"
    for n in ("dqu", "dqv"):
        judge(n, o[n].float(), g[n], bnd[n])
    judge("dq_out", o["dq3"][:, :d].float(), g["dq"], bnd["dq"])
    judge("dk", o["dqkv"][:, d:2 * d].float(), g["dk"], bnd["dk"])
    judge("dv", o["dqkv"][:, 2 * d:].float(), g["dv"], bnd["dv"])
    judge("bias_grads", o["bg"], c["pre_bg"].double() + g["bias_grads"], AO.bias_bound(g, c["pre_bg"]))
    assert torch.isnan(o["dq3"][:, d:].float()).all() and torch.isnan(o["dqkv"][:, :d].float()).all(), "another third was written"
    for n, x in (("ctx", o["ctx"]), ("ctx_lo", o["lo"]), ("dqu", o["dqu"]), ("dqv", o["dqv"]), ("dq_out", o["dq3"][:, :d]),
                 ("dk | dv", o["dqkv"][:, d:])):
        padded_rows_zero(c, n, x.float())
    again = run(c)   # forward plus backward twice: the same bits (NaN prefill of untouched blocks included)
    for n in sorted(set(o) - {"bg"}):   # (bias_grads: the shared second-stage reduction adds eight partial sums atomically, as on
        #                                  the unlimited path -- tests/test_attention_kernels_gpu.py leaves it out for the same reason)
        assert torch.equal(o[n].view(torch.int16 if o[n].dtype == BF16 else torch.int32),
                           again[n].view(torch.int16 if o[n].dtype == BF16 else torch.int32)), f"{n} differs between two runs"


def test_ds_blocks_and_dpos_touch_only_the_window():
    """regular [100, 0] at T = 300: key tiles in front of the window are skipped, their dS blocks stay unwritten and unread"""
    c = case(REG, 100, 0, 300, 64, 0.0, None)
    g, T, nT = c["g"], c["T"], AO.n_tiles(c["T"])
    o = run(c)
    X = o["ds"].view(c["H"], c["B"], nT, nT + 1, 32, 32).float()
    ref, _ = AO.ds_blocks(g["dS"], c["lens"], T)
    bound, _ = AO.ds_blocks(c["bnd"]["dS"], c["lens"], T)
    needed = (bound > 0).flatten(-2).any(-1)           # blocks that hold a (query, key) pair of some window
    written = torch.isfinite(X).flatten(-2).all(-1)
    untouched = torch.isnan(X).flatten(-2).all(-1)
    assert (written | untouched).all() and (written | ~needed).all(), "a dS block the linear_pos gradient needs is not fully written"
    assert untouched[:, 0, 8:, :4].all(), "queries 256 .. 299 see no key below 156: key tiles 0 .. 3 must not be walked"
    m = written[..., None, None].expand_as(X)
    judge("dS blocks", X[m], ref[m], bound[m])
    pre = c["pre_dpos"].double()
    judge("dpos (oracle)", o["dpos"], pre + g["dpos"],
          2.0 ** -8 * g["cond_dpos"] + g["dterm_dpos"] + 2.0 ** -23 * (pre.abs() + g["dpos"].abs()))
    out = g["cond_dpos"].sum(-1) == 0                  # positions no window reaches: c = T-1+j-i outside [T-101, T-1]
    assert int(out.sum()) == 2 * T - 1 - 101
    assert torch.equal(o["dpos"][out].view(torch.int32), c["pre_dpos"][out].view(torch.int32)), "dpos outside every window changed"
    assert torch.equal(o["dcast"].view(torch.int16), o["dpos"].to(BF16).view(torch.int16)), "dpos_cast != bf16(dpos)"
