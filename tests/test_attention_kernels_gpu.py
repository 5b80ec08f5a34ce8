"""-m gpu: every kernel path of nemo_amd/csrc/attention.hip (fused relative-position attention forward, delta / prep, dQ, dK/dV,
linear_pos gradient and its reduction) through the C ABI against the float64 closed forms of tests/attention_oracle.py.

Operands are generated in bf16 and the oracle up-casts them; its only shared rounding is the kernels' documented
qu = bf16(q + u), qv = bf16(q + v).  Every output is a NaN-prefilled view between two 64-byte sentinel guards (the harness of
tests/test_norm_kernels_gpu.py); `+=` outputs (bias_grads, dpos) are prefilled with random values the reference adds.
The backward kernels run as in production: on the forward kernel's own ctx, ctx_lo and lse.

Every measure is PER ELEMENT, |got - ref| <= bound[element]; the worst ratio and its index are printed.  cond = the oracle's
conditioning (sum of magnitudes of the terms of the element's last contraction; downstream of dS the pre-cancellation magnitude
P scale (|dP| keep / (1-p) + |delta|)), sdelta_i = scale (2 dk + 2) 2^-24 max_j (sum |qu.k| + sum |qv.p|) <= 2^-10 on every case
(asserted by tests/test_attention_host.py, which also shows that a float32 / bf16 implementation of the documented arithmetic
stays below 1.0 x every bound here).  Bounds and their origins:

  ctx          2^-8 cond + 2^-8 |ref|            derived: bf16 rounding of each probability (2^-9 cond), of the output (2^-9 |ref|),
                                                 f32 score error 2 sdelta cond with sdelta <= 2^-10
  lse          sdelta + 8 2^-24 max(1, |ref|)    derived; exactly 0 beyond the length
  ctx_lo       |lo| <= 2^-8 |ctx|, not all zero; |(ctx + lo) - ref| <= 2^-8 cond + 2^-15 |ref|      derived
  delta        (dk + 2) 2^-24 sum |dO (O + O_lo)| against float64 of the kernel's OWN O, O_lo       derived (dk f32 additions)
  dqu dqv dk   2^-8 cond + 2^-8 |ref| + delta term            derived: bf16 rounding of dS + f32 error of P (2^-8 cond), of the
  dv dq_out                                      output; delta term = sum over the contraction of E |operand| with
                                                 E = (2^-8 sum_dv |dO| cond_ctx + 2^-16 sum_dv |dO O|) P scale: the kernels' delta
                                                 is taken from THEIR context, which differs from the oracle's by the forward bound
                                                 (O_lo only removes the output rounding) -- see attention_oracle.backward
  dS blocks    2^-8 |ref| + 2^-8 A + E           derived (same terms, no contraction)
  bias_grads   8.6e-7 (|prefill| + sum |term|) + column sums of (2^-8 cond + delta term) of dQu | dQv
                                                 first part: measured 1.07e-07 -> bound 8.6e-07 (float32 torch.sum on the CPU against
                                                 float64, worst column over every case, x8 for another order of additions;
                                                 `python tests/test_attention_kernels_gpu.py` re-measures it); second part derived:
                                                 the kernel sums its own f32 dQu / dQv
  dpos         own blocks: (n_terms + 1) 2^-24 (sum |x qv| + |prefill|)    derived (f32 accumulation of exact bf16 products)
               oracle: 2^-8 cond + delta term + 2^-23 (|prefill| + |ref|)   derived (the last term: the f32 addition to the prefill)
               dpos_cast == bf16(dpos) exactly
  padded rows of ctx, dqu, dqv, dq_out, dk, dv: exactly zero; other thirds of dq_out / dqkv, pad columns, guards: untouched
"""
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_oracle as AO  # noqa: E402
from test_norm_kernels_gpu import Guarded, assert_intact, bits, put  # noqa: E402

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, BF16, F64, I64 = torch.float32, torch.bfloat16, torch.float64, torch.int64
NAN = float("nan")
MI_ERR_ARG = 1
SEED, SITE = 5, 9      # of ops.Dropout in every dropout case (tests/test_attention_host.py restates the key for the same pair)


@pytest.fixture(autouse=True)
def stop_after_a_gpu_error():
    """a launch that failed leaves the device in an unknown state: nothing more of this file is started on it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, no further test is started: {e}", returncode=3)


def ops():
    from nemo_amd import ops as _ops
    return _ops


def lib():
    from nemo_amd._lib import lib as _lib
    return _lib


def P(x):
    """device pointer of a tensor / Guarded / None"""
    if x is None:
        return None
    if isinstance(x, Guarded):
        x = x.t
    assert x.is_cuda
    return x.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def nan_bits_kept(t):
    """every element of a NaN-prefilled bf16 / f32 tensor is still NaN"""
    return bool(torch.isnan(t.float()).all())


# ------------------------------------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def case(B, H, T, dk, lens, regime="plain", p=0.0, packed=False):
    """inputs of one problem and its float64 reference (computed once, shared, never modified)"""
    z = AO.inputs(B, H, T, dk, regime)
    drop = ops().Dropout(p, seed=SEED, site=SITE)
    keep = AO.keep_masks(drop, B, H, T) if p else None
    cu = None
    if packed:
        z, cu = AO.pack_inputs(z, lens, T)
    f = AO.forward(z["qkv"], z["pos"], z["u"], z["v"], lens, B, H, T, dk, keep=keep, p=p, cu=cu)
    g = AO.backward(f, z["dO"])
    bnd = AO.bounds(f, g)
    X, written = AO.ds_blocks(g["dS"], lens, T, packed)
    Xb, _ = AO.ds_blocks(bnd["dS"], lens, T, packed)
    d = H * dk
    return dict(B=B, H=H, T=T, dk=dk, d=d, lens=lens, p=p, drop=drop, cu=cu, z=z, f=f, g=g, bnd=bnd, X=X, Xb=Xb, written=written,
                rows=z["qkv"].shape[0], scale=1.0 / math.sqrt(dk), pre_bg=AO.prefill(2 * d, 1), pre_dpos=AO.prefill((2 * T - 1) * d, 2)
                .view(2 * T - 1, d), Ls=AO._lens(lens, T))


def device_inputs(c, ldp_pad=0):
    z, d = c["z"], c["d"]
    s = dict(qkv=put(z["qkv"]), u=put(z["u"]), v=put(z["v"]), dO=put(z["dO"]), lens=torch.tensor(c["lens"], dtype=I64, device=dev),
             cu=None if c["cu"] is None else c["cu"].to(dev))
    if ldp_pad:   # pos embedded in a wider matrix
        wide = torch.full((2 * c["T"] - 1, d + ldp_pad), 3.0, dtype=BF16)
        wide[:, :d] = z["pos"]
        s["pos"], s["ldp"] = put(wide), d + ldp_pad
    else:
        s["pos"], s["ldp"] = put(z["pos"]), d
    return s


def drop_args(c):
    dr = c["drop"]
    return dr.key, dr.threshold, dr.scale


# ------------------------------------------------------------------------------------------------ launches (C ABI)
def run_fwd(c, s, want_lse=True, want_lo=True, ldo_pad=0):
    B, H, T, dk, d = c["B"], c["H"], c["T"], c["dk"], c["d"]
    ldo = d + ldo_pad
    ctx = Guarded((c["rows"], ldo), BF16, fill=NAN)
    lo = Guarded((c["rows"], ldo), BF16, fill=NAN) if want_lo else None
    lse = Guarded((B, H, T), F32, fill=NAN) if want_lse else None
    rc = lib().mi355x_relpos_flash_fwd(P(s["qkv"]), 3 * d, P(s["pos"]), s["ldp"], P(s["u"]), P(s["v"]), P(s["lens"]), P(ctx), P(lo), ldo,
                                       P(lse), B, H, T, dk, (T + 7) // 8 * 8, c["scale"], *drop_args(c), P(s["cu"]), stream())
    assert rc == 0, rc
    assert_intact(ctx=ctx, **(dict(ctx_lo=lo) if lo else {}), **(dict(lse=lse) if lse else {}))
    return ctx, lo, lse


def run_prep(c, s, ctx, lo, fused=True):
    B, H, T, d = c["B"], c["H"], c["T"], c["d"]
    delta = Guarded((B, H, T), F32, fill=NAN)
    qu, qv = Guarded((c["rows"], d), BF16, fill=NAN), Guarded((c["rows"], d), BF16, fill=NAN)
    if fused:
        rc = lib().mi355x_attn_bwd_prep(P(s["dO"]), P(ctx), P(lo), P(delta), P(s["qkv"]), 3 * d, P(s["u"]), P(s["v"]), P(qu), P(qv), B, H,
                                        T, d, P(s["lens"]), P(s["cu"]), stream())
    else:
        rc = lib().mi355x_attn_delta(P(s["dO"]), P(ctx), P(lo), P(delta), B, H, T, d, P(s["lens"]), P(s["cu"]), stream())
    assert rc == 0, rc
    assert_intact(delta=delta, qu=qu, qv=qv)
    return delta, qu, qv


def run_dq(c, s, st, sep=True, fused=True, bias=True, ds=True):
    """st: dict(qu, qv, lse, delta) on the device.  Returns dict of Guarded outputs (absent ones None)."""
    B, H, T, dk, d, rows = c["B"], c["H"], c["T"], c["dk"], c["d"], c["rows"]
    o = dict(dqu=Guarded((rows, d), BF16, fill=NAN) if sep else None, dqv=Guarded((rows, d), BF16, fill=NAN) if sep else None,
             dq3=Guarded((rows, 3 * d), BF16, fill=NAN) if fused else None,
             bg=Guarded(2 * d, F32, src=c["pre_bg"]) if (fused and bias) else None,
             ds=Guarded(lib().mi355x_relpos_ds_elems(B, H, T), BF16, fill=NAN) if ds else None)
    n_cs = B * ((T + 127) // 128) * 2 * d
    o["cs"] = Guarded(n_cs, F32, fill=NAN) if o["bg"] else None
    rc = lib().mi355x_relpos_flash_bwd_dq(P(st["qu"]), P(st["qv"]), P(s["qkv"]), 3 * d, P(s["pos"]), s["ldp"], P(s["lens"]), P(s["dO"]),
                                          P(st["lse"]), P(st["delta"]), P(o["dqu"]), P(o["dqv"]), P(o["ds"]), P(o["dq3"]), 3 * d,
                                          P(o["bg"]), P(o["cs"]), n_cs if o["cs"] else 0, B, H, T, dk,
                                          o["ds"].t.numel() if ds else 0, c["scale"], *drop_args(c), P(s["cu"]), stream())
    assert rc == 0, rc
    assert_intact(**{k: v for k, v in o.items() if v is not None})
    return o


def run_dkv(c, s, st):
    B, H, T, dk, d = c["B"], c["H"], c["T"], c["dk"], c["d"]
    dqkv = Guarded((c["rows"], 3 * d), BF16, fill=NAN)
    rc = lib().mi355x_relpos_flash_bwd_dkv(P(st["qu"]), P(st["qv"]), P(s["qkv"]), 3 * d, P(s["pos"]), s["ldp"], P(s["lens"]), P(s["dO"]),
                                           P(st["lse"]), P(st["delta"]), P(dqkv), 3 * d, B, H, T, dk, (T + 7) // 8 * 8, c["scale"],
                                           *drop_args(c), P(s["cu"]), stream())
    assert rc == 0, rc
    assert_intact(dqkv=dqkv)
    return dqkv


def run_dpos(c, s, qv, ds, two_stage=True, cast=True):
    B, H, T, dk, d = c["B"], c["H"], c["T"], c["dk"], c["d"]
    dpos = Guarded((2 * T - 1, d), F32, src=c["pre_dpos"])
    dcast = Guarded((2 * T - 1, d), BF16, fill=NAN) if (cast and two_stage) else None
    n = lib().mi355x_relpos_dpos_partial_elems(B, H, T)
    part = Guarded(n, F32, fill=NAN) if two_stage else None
    rc = lib().mi355x_relpos_flash_bwd_dpos(P(qv), P(ds), P(s["lens"]), P(dpos), d, P(dcast), P(part), n if two_stage else 0, B, H, T, dk,
                                            ds.t.numel(), P(s["cu"]), stream())
    assert rc == 0, rc
    assert_intact(dpos=dpos, **(dict(dpos_cast=dcast, partial=part) if two_stage else {}))
    return dpos, dcast


# ------------------------------------------------------------------------------------------------ measures
def judge(what, got, ref, bound):
    r, i = AO.worst(got.detach().cpu(), ref, bound)
    idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(max(i, 0)), ref.shape)) if ref.numel() else ()
    print(f"{what}: worst |got - ref| / bound {r:.3f} at {idx}")
    assert r <= 1.0, f"{what}: element {idx} is off by {r:.3f} x its bound: got {got.detach().cpu().flatten()[i].item()!r}, " \
                     f"reference {ref.flatten()[i].item()!r}, bound {bound.flatten()[i].item():.3e}"
    return r


def padded_rows_zero(c, name, x):
    """padded mode: rows len <= i < T of every utterance hold exactly zero"""
    if c["cu"] is not None:
        return
    x = x.detach().cpu().view(c["B"], c["T"], -1)
    for b, L in enumerate(c["Ls"]):
        assert (x[b, L:] == 0).all(), f"{name}: utterance {b} has non-zero rows beyond its length {L}"


def check_fwd(c, ctx, lo, lse, tag=""):
    f, bnd, d = c["f"], c["bnd"], c["d"]
    got = ctx.cpu()[:, :d].float()
    judge(tag + "ctx", got, f["ctx"], bnd["ctx"])
    padded_rows_zero(c, "ctx", got)
    if ctx.t.shape[1] > d:
        assert nan_bits_kept(ctx.cpu()[:, d:]), "ctx: pad columns were written"
    if lo is not None:
        l = lo.cpu()[:, :d].float()
        assert torch.isfinite(l).all() and (l.abs() <= got.abs() * 2.0 ** -8).all(), "ctx_lo exceeds half an ulp of ctx"
        if max(c["Ls"]) >= 2:   # (a single key: the context IS its bf16 value row, nothing is dropped)
            assert l.abs().max() > 0, "ctx_lo is all zero"
        judge(tag + "ctx + ctx_lo", got.double() + l.double(), f["ctx"], bnd["ctx_sum"])
        if lo.t.shape[1] > d:
            assert nan_bits_kept(lo.cpu()[:, d:]), "ctx_lo: pad columns were written"
    if lse is not None:
        gl = lse.cpu()
        judge(tag + "lse", gl, f["lse"], bnd["lse"])
        for b, L in enumerate(c["Ls"]):
            assert (gl[b, :, L:] == 0).all(), "lse beyond the length is not zero"


def check_prep(c, s, ctx, lo, delta, qu, qv, tag=""):
    f, B, H, T, dk = c["f"], c["B"], c["H"], c["T"], c["dk"]
    assert torch.equal(bits(qu.t), bits(AO.bf(f["qu_rows"]))) and torch.equal(bits(qv.t), bits(AO.bf(f["qv_rows"]))), "qu / qv"
    O = ctx.cpu().double() + (lo.cpu().double() if lo is not None else 0.0)
    dOp = AO._heads(AO.unpack_rows(c["z"]["dO"].double(), c["lens"], T, c["cu"]), B, T, H, dk)
    Op = AO._heads(AO.unpack_rows(O, c["lens"], T, c["cu"]), B, T, H, dk)
    judge(tag + "delta (own O)", delta.cpu(), (dOp * Op).sum(-1), (dk + 2) * 2.0 ** -24 * (dOp * Op).abs().sum(-1))
    for b, L in enumerate(c["Ls"]):
        assert (delta.cpu()[b, :, L:] == 0).all(), "delta beyond the length is not zero"


def check_dq(c, o, tag=""):
    g, bnd, d = c["g"], c["bnd"], c["d"]
    if o["dqu"] is not None:
        for n in ("dqu", "dqv"):
            judge(tag + n, o[n].cpu().float(), g[n], bnd[n])
            padded_rows_zero(c, n, o[n].cpu().float())
    if o["dq3"] is not None:
        q3 = o["dq3"].cpu()
        judge(tag + "dq_out", q3[:, :d].float(), g["dq"], bnd["dq"])
        padded_rows_zero(c, "dq_out", q3[:, :d].float())
        assert nan_bits_kept(q3[:, d:]), "dq_out: the K / V thirds were written"
    if o["bg"] is not None:
        pre = c["pre_bg"]
        judge(tag + "bias_grads", o["bg"].cpu(), pre.double() + g["bias_grads"], AO.bias_bound(g, pre))
    if o["ds"] is not None:
        check_blocks(c, o["ds"], tag)


def blocks_of(c, ds):
    nT = AO.n_tiles(c["T"])
    return ds.cpu().view(c["H"], c["B"], nT, nT + 1, 32, 32)


def check_blocks(c, ds, tag=""):
    X, wr = blocks_of(c, ds).float(), c["written"]
    nanb = torch.isnan(X).flatten(-2).all(-1)
    fin = torch.isfinite(X).flatten(-2).all(-1)
    assert (fin[wr]).all(), "a dS block the linear_pos gradient reads was not (fully) written"
    assert (nanb[~wr]).all(), "a dS block outside the written set was touched"
    m = wr[..., None, None].expand_as(X)
    judge(tag + "dS blocks", X[m], c["X"][m], c["Xb"][m])


def check_dkv(c, dqkv, tag=""):
    g, bnd, d = c["g"], c["bnd"], c["d"]
    x = dqkv.cpu()
    judge(tag + "dk", x[:, d:2 * d].float(), g["dk"], bnd["dk"])
    judge(tag + "dv", x[:, 2 * d:].float(), g["dv"], bnd["dv"])
    padded_rows_zero(c, "dk | dv", x[:, d:].float())
    assert nan_bits_kept(x[:, :d]), "dqkv: the Q third was written"


def check_dpos(c, ds, dpos, dcast, tag=""):
    g, f, T = c["g"], c["f"], c["T"]
    pre = c["pre_dpos"].double()
    own, cond, nterm = AO.dpos_from_blocks(blocks_of(c, ds), c["written"], f["qv"], T)
    judge(tag + "dpos (own blocks)", dpos.cpu(), pre + own, (nterm[:, None] + 1) * 2.0 ** -24 * (cond + pre.abs()))
    judge(tag + "dpos (oracle)", dpos.cpu(), pre + g["dpos"],
          2.0 ** -8 * g["cond_dpos"] + g["dterm_dpos"] + 2.0 ** -23 * (pre.abs() + g["dpos"].abs()))
    if dcast is not None:
        assert torch.equal(bits(dcast.t), bits(dpos.t.to(BF16))), "dpos_cast != bf16(dpos)"


def run_all(c, tag="", ldp_pad=0):
    """the production sequence: forward, prep, dQ (every output at once), dK/dV, dpos (two-stage) -- each judged"""
    s = device_inputs(c, ldp_pad)
    ctx, lo, lse = run_fwd(c, s)
    check_fwd(c, ctx, lo, lse, tag)
    delta, qu, qv = run_prep(c, s, ctx, lo)
    check_prep(c, s, ctx, lo, delta, qu, qv, tag)
    st = dict(qu=qu, qv=qv, lse=lse, delta=delta)
    o = run_dq(c, s, st)
    check_dq(c, o, tag)
    dqkv = run_dkv(c, s, st)
    check_dkv(c, dqkv, tag)
    dpos, dcast = run_dpos(c, s, qv, o["ds"])
    check_dpos(c, o["ds"], dpos, dcast, tag=tag)
    return dict(s=s, ctx=ctx, lo=lo, lse=lse, delta=delta, qu=qu, qv=qv, dq=o, dqkv=dqkv, dpos=dpos, dcast=dcast, st=st)


# ------------------------------------------------------------------------------------------------ geometry and values
@pytest.mark.parametrize("dk", [64, 128])
@pytest.mark.parametrize("T,lens,H", AO.GEOMETRY, ids=lambda x: "_".join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_geometry(T, lens, H, dk):
    run_all(case(3, H, T, dk, lens))


@pytest.mark.parametrize("dk", [64, 128])
@pytest.mark.parametrize("regime", AO.REGIMES)
def test_value_regimes(regime, dk):
    """stair-up at dk = 128 is the case that decides whether the forward's re-scale reaches all four accumulator tiles"""
    run_all(case(3, 2, AO.REGIME_T, dk, AO.REGIME_LENS, regime))


@pytest.mark.parametrize("dk", [64, 128])
def test_packed_rows(dk):
    """utterance b at rows cu[b] .. cu[b] + len - 1: every kernel against the oracle's valid rows; nothing beyond row sum(len) (the
    guards), lse / delta beyond a length zero, query tiles beyond an utterance leave their column-sum slab zero (bias_grads)"""
    run_all(case(3, 2, 161, dk, (161, 97, 1), packed=True))


# ------------------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("T,dk", [(45, 64), (128, 128)])
def test_dropout_mask_is_the_restated_mask(T, dk):
    """one-hot V: the context IS the dropped probability matrix; the keep pattern read out of it equals attention_oracle.keep_mask
    exactly on every element whose undropped probability exceeds 1e-3 (the read-out cannot decide the others: they stay below
    the cap of tests/test_kernels_gpu.py's dropout test)"""
    B, H, p, lens = 2, 2, 0.25, (T, 2 * T // 3)
    d = H * dk
    z = dict(AO.inputs(B, H, T, dk))
    eye = torch.zeros(T, dk)
    eye[torch.arange(T), torch.arange(T)] = 1.0
    qkv = z["qkv"].clone()
    qkv[:, 2 * d:] = eye.repeat(B, H).to(BF16)
    drop = ops().Dropout(p, seed=SEED, site=SITE)
    f = AO.forward(qkv, z["pos"], z["u"], z["v"], lens, B, H, T, dk)
    c = dict(B=B, H=H, T=T, dk=dk, d=d, lens=lens, rows=B * T, scale=1.0 / math.sqrt(dk), drop=drop, cu=None, z=dict(z, qkv=qkv))
    s = device_inputs(c)
    ctx, _, _ = run_fwd(c, s)
    Pd = ctx.cpu().float().view(B, T, H, dk)[..., :T].permute(0, 2, 1, 3).double()
    Pu = f["P"]
    big = Pu > 1e-3
    read = Pd > 0.5 * Pu / (1 - p)
    keep = AO.keep_masks(drop, B, H, T)
    n = int(big.sum())
    print(f"T = {T}, dk = {dk}: {n} decidable elements, keep rate {read[big].double().mean().item():.4f}, "
          f"{int((read != keep)[big].sum())} differ from the restated mask")
    assert n > 500 and torch.equal(read[big], keep[big])
    assert (Pd[~big].abs() <= (1e-3 / (1 - p)) * (1 + 2.0 ** -7)).all()


@pytest.mark.parametrize("dk", [64, 128])
@pytest.mark.parametrize("p", AO.DROP_P)
def test_dropout_per_element(p, dk):
    """the restated mask as a reference input: forward, dQ, dK/dV, dS blocks and dpos per element -- the lane = query (forward, dQ)
    and lane = key (dK/dV) layouts must regenerate the same mask across query tiles, utterances and heads"""
    run_all(case(3, 2, AO.REGIME_T, dk, AO.REGIME_LENS, "plain", p))


# ------------------------------------------------------------------------------------------------ paths
@pytest.mark.parametrize("dk", [64, 128])
def test_forward_optional_outputs_and_pitches(dk):
    c = case(3, 2, 33, dk, (33, 32, 1))
    s = device_inputs(c)
    ctx, lo, lse = run_fwd(c, s)
    for kw in (dict(want_lse=False), dict(want_lo=False), dict(want_lse=False, want_lo=False)):
        ctx2, _, _ = run_fwd(c, s, **kw)
        assert torch.equal(bits(ctx2.t), bits(ctx.t)), kw
    # pitched: ldo = d + 8, pos inside a wider matrix (ldp = d + 16); ld_dq = 3d is what run_dq uses throughout
    sp = device_inputs(c, ldp_pad=16)
    ctx3, lo3, lse3 = run_fwd(c, sp, ldo_pad=8)
    check_fwd(c, ctx3, lo3, lse3, "pitched ")
    assert torch.equal(bits(ctx3.t[:, :c["d"]]), bits(ctx.t)) and torch.equal(bits(lo3.t[:, :c["d"]]), bits(lo.t))
    assert torch.equal(bits(lse3.t), bits(lse.t))
    delta, qu, qv = run_prep(c, s, ctx, lo)
    st = dict(qu=qu, qv=qv, lse=lse, delta=delta)
    o, o2 = run_dq(c, s, st), run_dq(c, sp, st)
    k, k2 = run_dkv(c, s, st), run_dkv(c, sp, st)
    for n in ("dqu", "dqv", "dq3", "ds"):
        assert torch.equal(bits(o[n].t), bits(o2[n].t)), n
    assert torch.equal(bits(k.t), bits(k2.t))


@pytest.mark.parametrize("dk", [64, 128])
def test_dq_output_combinations(dk):
    """(dqu, dqv) only; dq_out only; dq_out + bias_grads -- each with and without the dS blocks: no output's bits depend on which
    others are requested"""
    c = case(3, 2, 129, dk, (129, 96, 97))
    s = device_inputs(c)
    ctx, lo, lse = run_fwd(c, s)
    delta, qu, qv = run_prep(c, s, ctx, lo)
    st = dict(qu=qu, qv=qv, lse=lse, delta=delta)
    full = run_dq(c, s, st)
    check_dq(c, full)
    for ds in (True, False):
        a = run_dq(c, s, st, sep=True, fused=False, ds=ds)
        b = run_dq(c, s, st, sep=False, fused=True, bias=False, ds=ds)
        e = run_dq(c, s, st, sep=False, fused=True, bias=True, ds=ds)
        check_dq(c, a), check_dq(c, b), check_dq(c, e)
        assert torch.equal(bits(a["dqu"].t), bits(full["dqu"].t)) and torch.equal(bits(a["dqv"].t), bits(full["dqv"].t))
        assert torch.equal(bits(b["dq3"].t), bits(full["dq3"].t)) and torch.equal(bits(e["dq3"].t), bits(full["dq3"].t))
        # (bias_grads is finished through atomic adds: judged against its bound by check_dq, not bit for bit)
        if ds:
            for x in (a, b, e):
                assert torch.equal(bits(x["ds"].t), bits(full["ds"].t))


@pytest.mark.parametrize("B,H,T,dk,lens", [(3, 2, 33, 64, (33, 32, 1)), (3, 2, 33, 128, (33, 32, 1)),
                                           (8, 1, 45, 64, tuple(45 - 3 * b for b in range(8))),
                                           (9, 1, 45, 64, tuple(45 - 3 * b for b in range(9)))])
def test_dpos_atomic_path_and_batch_chunks(B, H, T, dk, lens):
    """partial = NULL (atomic adds into dpos) against the two-stage path on the same blocks; B >= 8 walks utterances in chunks of
    four (B = 9: a last chunk of one); T = 33: block pairs that fall partly outside [0, nT]"""
    c = case(B, H, T, dk, lens)
    r = run_all(c)
    dpos_a, _ = run_dpos(c, r["s"], r["qv"], r["dq"]["ds"], two_stage=False)
    check_dpos(c, r["dq"]["ds"], dpos_a, None, tag="atomic ")
    # through ops (scratch of its own), without the cast
    dp = Guarded((2 * T - 1, c["d"]), F32, src=c["pre_dpos"])
    ops().relpos_flash_bwd_dpos(r["qv"].t, r["dq"]["ds"].t, r["s"]["lens"], dp.t, B, H, T, dk)
    assert_intact(dpos=dp)
    assert torch.equal(bits(dp.t), bits(r["dpos"].t))


@pytest.mark.parametrize("H,dk,B,T", [(9, 64, 2, 5), (5, 128, 3, 7), (2, 64, 3, 33)])
@pytest.mark.parametrize("with_lo", [True, False])
def test_delta_and_prep_wide_rows(H, dk, B, T, with_lo):
    """d = 576 / 640: the column loop's second pass, partly used; B * T no multiple of the four rows of a workgroup; the fused
    prologue equals attn_delta + qbias bit for bit"""
    d = H * dk
    g = torch.Generator().manual_seed(d + T)
    r = lambda *sh: torch.randn(*sh, generator=g)  # noqa: E731
    z = dict(qkv=AO.bf(r(B * T, 3 * d)), u=r(d), v=r(d), dO=AO.bf(r(B * T, d)), pos=AO.bf(r(2 * T - 1, d)))
    O = r(B * T, d)
    ctx, lo = AO.bf(O), AO.bf(O - AO.bf(O).float())
    lens = tuple([T] * B)
    c = dict(B=B, H=H, T=T, dk=dk, d=d, lens=lens, Ls=list(lens), rows=B * T, cu=None, z=z,
             f=dict(qu_rows=AO.bf(z["qkv"][:, :d].float() + z["u"]), qv_rows=AO.bf(z["qkv"][:, :d].float() + z["v"])))
    s = device_inputs(c)
    ctx_d, lo_d = Guarded((B * T, d), BF16, src=ctx), (Guarded((B * T, d), BF16, src=lo) if with_lo else None)
    delta, qu, qv = run_prep(c, s, ctx_d, lo_d)
    check_prep(c, s, ctx_d, lo_d, delta, qu, qv)
    delta2, qu2, _ = run_prep(c, s, ctx_d, lo_d, fused=False)
    assert torch.equal(bits(delta2.t), bits(delta.t)) and nan_bits_kept(qu2.t)
    q1, q2 = Guarded((B * T, d), BF16, fill=NAN), Guarded((B * T, d), BF16, fill=NAN)
    ops().qbias(s["qkv"], 3 * d, s["u"], s["v"], q1.t, q2.t, B * T, d)
    assert_intact(qu=q1, qv=q2)
    assert torch.equal(bits(q1.t), bits(qu.t)) and torch.equal(bits(q2.t), bits(qv.t))


@pytest.mark.parametrize("dk", [64, 128])
def test_every_kernel_is_deterministic(dk):
    """forward, prep, dQ and dK/dV twice on the T = 257 case: identical bits (a missing barrier or an LDS slot read before it is
    written shows here)"""
    c = case(3, 2, 257, dk, (257, 193, 225))
    s = device_inputs(c)
    runs = []
    for _ in range(2):
        ctx, lo, lse = run_fwd(c, s)
        delta, qu, qv = run_prep(c, s, ctx, lo)
        st = dict(qu=qu, qv=qv, lse=lse, delta=delta)
        o = run_dq(c, s, st)
        runs.append(dict(ctx=ctx, lo=lo, lse=lse, delta=delta, qu=qu, qv=qv, dqu=o["dqu"], dqv=o["dqv"], ds=o["ds"], dq3=o["dq3"],
                         dqkv=run_dkv(c, s, st)))
    for n in runs[0]:
        a, b = bits(runs[0][n].t), bits(runs[1][n].t)
        assert torch.equal(a, b), f"{n} differs between two runs"


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks():
    """every MI_ERR_ARG branch of the six entry points returns before anything is launched: outputs stay NaN, guards intact"""
    L = lib()
    B, H, T, dk = 2, 2, 9, 64
    d = H * dk
    t = lambda *sh, dt=BF16: Guarded(sh, dt, fill=NAN)  # noqa: E731
    qkv, pos, dO, qu, qv = t(B * T, 3 * d), t(2 * T - 1, d), t(B * T, d), t(B * T, d), t(B * T, d)
    u, v = t(d, dt=F32), t(d, dt=F32)
    lens = torch.tensor([T, 3], dtype=I64, device=dev)
    cu = torch.tensor([0, T, T + 3], dtype=I64, device=dev)
    ctx, lo, lse, delta = t(B * T, d), t(B * T, d), t(B, H, T, dt=F32), t(B, H, T, dt=F32)
    dqu, dqv, dq3, dqkv, bg = t(B * T, d), t(B * T, d), t(B * T, 3 * d), t(B * T, 3 * d), t(2 * d, dt=F32)
    n_ds, n_pt, n_cs = L.mi355x_relpos_ds_elems(B, H, T), L.mi355x_relpos_dpos_partial_elems(B, H, T), B * 2 * d
    ds, part, cs = t(n_ds), t(n_pt, dt=F32), t(n_cs, dt=F32)
    dpos, dcast = t(2 * T - 1, d, dt=F32), t(2 * T - 1, d)
    outs = dict(ctx=ctx, lo=lo, lse=lse, delta=delta, dqu=dqu, dqv=dqv, dq3=dq3, dqkv=dqkv, bg=bg, ds=ds, part=part, cs=cs, dpos=dpos,
                dcast=dcast, qu=qu, qv=qv)
    sc, Tp, st = 0.125, 16, stream()

    def fwd(**k):
        a = dict(qkv=P(qkv), ldq=3 * d, pos=P(pos), ldp=d, u=P(u), v=P(v), len=P(lens), ctx=P(ctx), lo=P(lo), ldo=d, lse=P(lse), B=B, H=H,
                 T=T, dk=dk, cu=None)
        a.update(k)
        return L.mi355x_relpos_flash_fwd(a["qkv"], a["ldq"], a["pos"], a["ldp"], a["u"], a["v"], a["len"], a["ctx"], a["lo"], a["ldo"],
                                         a["lse"], a["B"], a["H"], a["T"], a["dk"], Tp, sc, 0, 0, 1.0, a["cu"], st)

    def dlt(**k):
        a = dict(dO=P(dO), O=P(ctx), delta=P(delta), B=B, H=H, T=T, d=d, len=P(lens), cu=None)
        a.update(k)
        return L.mi355x_attn_delta(a["dO"], a["O"], None, a["delta"], a["B"], a["H"], a["T"], a["d"], a["len"], a["cu"], st)

    def prep(**k):
        a = dict(dO=P(dO), O=P(ctx), delta=P(delta), qkv=P(qkv), ldq=3 * d, u=P(u), v=P(v), qu=P(qu), qv=P(qv), B=B, H=H, T=T, d=d,
                 len=P(lens), cu=None)
        a.update(k)
        return L.mi355x_attn_bwd_prep(a["dO"], a["O"], None, a["delta"], a["qkv"], a["ldq"], a["u"], a["v"], a["qu"], a["qv"], a["B"],
                                      a["H"], a["T"], a["d"], a["len"], a["cu"], st)

    def dq(**k):
        a = dict(qu=P(qu), qkv=P(qkv), ldq=3 * d, pos=P(pos), ldp=d, len=P(lens), dqu=P(dqu), dqv=P(dqv), ds=P(ds), dq3=P(dq3),
                 ld_dq=3 * d, bg=P(bg), cs=P(cs), n_cs=n_cs, B=B, H=H, T=T, dk=dk, n_ds=n_ds)
        a.update(k)
        return L.mi355x_relpos_flash_bwd_dq(a["qu"], P(qv), a["qkv"], a["ldq"], a["pos"], a["ldp"], a["len"], P(dO), P(lse), P(delta),
                                            a["dqu"], a["dqv"], a["ds"], a["dq3"], a["ld_dq"], a["bg"], a["cs"], a["n_cs"], a["B"],
                                            a["H"], a["T"], a["dk"], a["n_ds"], sc, 0, 0, 1.0, None, st)

    def dkv(**k):
        a = dict(qu=P(qu), ldq=3 * d, ldp=d, len=P(lens), dqkv=P(dqkv), ldd=3 * d, B=B, H=H, T=T, dk=dk)
        a.update(k)
        return L.mi355x_relpos_flash_bwd_dkv(a["qu"], P(qv), P(qkv), a["ldq"], P(pos), a["ldp"], a["len"], P(dO), P(lse), P(delta),
                                             a["dqkv"], a["ldd"], a["B"], a["H"], a["T"], a["dk"], Tp, sc, 0, 0, 1.0, None, st)

    def dps(**k):
        a = dict(qv=P(qv), ds=P(ds), len=P(lens), dpos=P(dpos), dcast=P(dcast), part=P(part), n_pt=n_pt, B=B, H=H, T=T, dk=dk, n_ds=n_ds)
        a.update(k)
        return L.mi355x_relpos_flash_bwd_dpos(a["qv"], a["ds"], a["len"], a["dpos"], d, a["dcast"], a["part"], a["n_pt"], a["B"], a["H"],
                                              a["T"], a["dk"], a["n_ds"], None, st)

    bad = []
    for fn, name, variants in (
        (fwd, "fwd", [dict(dk=32), dict(dk=96), dict(ldq=3 * d + 8), dict(ldp=d + 4), dict(ldo=d + 4), dict(qkv=P(qkv) + 2),
                      dict(pos=P(pos) + 8), dict(ctx=P(ctx) + 4), dict(lo=P(lo) + 2), dict(B=0), dict(H=0), dict(T=0), dict(T=-1),
                      dict(qkv=None), dict(pos=None), dict(u=None), dict(v=None), dict(ctx=None), dict(len=None, cu=P(cu)),
                      dict(len=None)]),
        (dlt, "delta", [dict(d=H * 32), dict(d=d + 8), dict(B=0), dict(H=0), dict(T=0), dict(dO=None), dict(O=None), dict(delta=None),
                        dict(len=None, cu=P(cu))]),
        (prep, "prep", [dict(d=H * 32), dict(ldq=3 * d + 4), dict(qkv=P(qkv) + 2), dict(qu=P(qu) + 2), dict(qv=P(qv) + 8),
                        dict(u=P(u) + 4), dict(v=P(v) + 4), dict(B=0), dict(H=-1), dict(T=0), dict(qu=None), dict(qv=None),
                        dict(u=None), dict(qkv=None), dict(len=None, cu=P(cu))]),
        (dq, "dq", [dict(dk=32), dict(ldq=3 * d + 8), dict(ldp=d + 4), dict(dq3=None, dqu=None), dict(dq3=None, dqv=None),
                    dict(ld_dq=3 * d + 4), dict(dq3=P(dq3) + 2), dict(cs=None), dict(n_cs=n_cs - 1), dict(ds=P(ds) + 2),
                    dict(n_ds=n_ds - 1), dict(n_ds=0), dict(B=0), dict(H=0), dict(T=0), dict(qu=None), dict(len=None), dict(pos=None)]),
        (dkv, "dkv", [dict(dk=96), dict(ldq=3 * d + 8), dict(ldp=d + 4), dict(ldd=3 * d + 8), dict(B=0), dict(H=0), dict(T=0),
                      dict(dqkv=None), dict(qu=None), dict(len=None)]),
        (dps, "dpos", [dict(dk=32), dict(ds=P(ds) + 2), dict(n_ds=n_ds - 1), dict(n_pt=n_pt - 1), dict(part=None), dict(B=0), dict(H=0),
                       dict(T=0), dict(qv=None), dict(ds=None), dict(len=None), dict(dpos=None)])):
        for kw in variants:
            rc = fn(**kw)
            if rc != MI_ERR_ARG:
                bad.append((name, kw, rc))
    torch.cuda.synchronize()
    assert not bad, bad
    assert_intact(**outs)
    for n, o in outs.items():
        assert nan_bits_kept(o.t), f"{n} was written by a call that returned MI_ERR_ARG"


# ------------------------------------------------------------------------------------------------ CPU re-measurement
if __name__ == "__main__":
    w = AO.measure_column_sums()
    print(f"float32 column sums of dQu | dQv against float64, worst column over {len(AO.all_cases())} cases: {w:.3e} "
          f"-> bound {8 * w:.2e} (attention_oracle.TOL_COL = {AO.TOL_COL:.2e})")
