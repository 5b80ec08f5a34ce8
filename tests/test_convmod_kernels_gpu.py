"""-m gpu: every kernel path of nemo_amd/csrc/convmod.hip (depthwise Conv1d forward / backward, the streaming kernels, the GLU /
Swish and BatchNorm fusions, the eight BatchNorm kernels) through the C ABI against the float64 reference of
tests/convmod_oracle.py.

Operands are generated in their storage dtype and the oracle up-casts them.  Every output sits between 64-byte guards of -0.0f
and is pre-filled with NaN; the `+=` outputs (stats, sums, dw, dbias, dgamma, dbeta, the running statistics) are pre-filled with
random values and the reference adds the prefill.  Each kernel is judged alone: the BatchNorm kernels get a `c` generated in the
storage dtype and the oracle's statistics, the statistics the forward writes are compared with float64 sums of the kernel's OWN
output, and the fused backward's convolution with the oracle applied to the gradient the stand-alone BatchNorm backward kernel
wrote (the fusion's contract is that its tile holds exactly those values).

Error measures
  convolution outputs (y, dx), per element:  |got - ref| <= (k + 1) * 2^-24 * (|bias| + sum_k |w * x|)  [+ 2^-8 * |ref| for bf16]:
      the worst case of a float32 FMA chain of k + 1 terms, plus one bf16 ulp of the stored value.  Derived, no margin.
  reduced columns, per column:  |got - ref| / (|prefill| + sum |term|) < TOL_COL, the measure of tests/test_norm_kernels_gpu.py
  BatchNorm elementwise outputs (y, dc), per row: row_err of the norm tests, the tolerances of test_dwconv_bn_swish
  mean / rstd: 1e-6 relative per channel
`python tests/test_convmod_kernels_gpu.py` re-measures, on the CPU, the float32 figures that the measured bounds are derived from.
"""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convmod_oracle as CO  # noqa: E402
from test_norm_kernels_gpu import Guarded, assert_intact, assert_rows, bits, col_err, put, rel_err, row_err  # noqa: E402

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
DT = {F32: "f32", BF16: "bf16"}
EPS, MOM = 1e-5, 0.1
NAN = float("nan")
MI_ERR_ARG = 1

# ---- the project's own tolerances (test_dwconv_bn_swish of tests/test_kernels_gpu.py), per row
TOL_Y = {F32: 4e-5, BF16: 2e-2}      # BatchNorm + Swish forward
TOL_G = {F32: 1e-4, BF16: 5e-2}      # gradients
TOL_STAT = 1e-6                      # mean, rstd per channel (a few float32 ulp)
# GLU / Swish written by the fused forward: sigmoid from v_exp_f32 / v_rcp_f32 (a few float32 ulp, 1e-5 of the row's largest entry
# is generous), then one rounding to the activation type
TOL_ACT = {F32: 1e-5, BF16: 2.0 ** -8 + 1e-5}
# ---- measured bounds.  Per-column error of every reduced column of this file (stats, sums, dw, dbias, dgamma, dbeta): the same
# sums taken in float32 by torch.sum on the CPU (prefill included) against float64, worst column over every input of this file,
# and 8x that for the kernels (another order of additions, finished through atomics).
#   measured 3.27e-07 -> bound 2.6e-06
TOL_COL = 2.6e-6
# Offset inputs c = +-c0 + s * randn (d = 64, M = 450): the cancellation in c - mean costs about 2^-24 * |c0| / s, so the bounds
# above do not apply by construction.  Measured: F.batch_norm + SiLU and its autograd (rstd: torch.var, two passes) in float32 on
# the CPU against the oracle on these inputs, worst channel / row; the kernels are allowed 4x that.  bf16 outputs keep TOL_Y /
# TOL_G: their own rounding (2^-9 per element) is larger than any of these figures.
#   (c0, s) = (30, 1):    rstd 1.06e-07 -> 4.2e-07    y 5.65e-06 -> 2.3e-05    dc 6.23e-06 -> 2.5e-05
#   (c0, s) = (100, 1):   rstd 7.85e-08 -> 3.1e-07    y 1.14e-05 -> 4.6e-05    dc 1.13e-05 -> 4.5e-05
TOL_OFF = {(30.0, 1.0): (4.2e-7, 2.3e-5, 2.5e-5), (100.0, 1.0): (3.1e-7, 4.6e-5, 4.5e-5)}   # (c0, s) -> (rstd, y, dc)
OFF_CS = ((30.0, 1.0), (100.0, 1.0))
OFF_B, OFF_T, OFF_D = 2, 225, 64


def ops():
    from nemo_amd import ops as _ops
    return _ops


def clib():
    from nemo_amd._lib import lib
    return lib


def ptr(t):
    return 0 if t is None else t.data_ptr()


class dwconv_level:
    """mi355x_dwconv_config(level) for the block: 0 = LDS-tile kernels, 1 = streaming forward, 2 = streaming backward too"""

    def __init__(self, level):
        self.level = level

    def __enter__(self):
        self.prev = clib().mi355x_dwconv_config(self.level)

    def __exit__(self, *exc):
        clib().mi355x_dwconv_config(self.prev)


# ------------------------------------------------------------------------------------------------ measures
def assert_conv(got, ref, cond, k, dtype, what):
    """per element: a float32 FMA chain of k + 1 terms (+ one bf16 ulp of the stored value)"""
    got, ref, cond = got.detach().double().cpu(), ref.detach().double(), cond.detach().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert not torch.isnan(got).any(), f"{what}: NaN survived in the output"
    bound = (k + 1) * 2.0 ** -24 * cond + (2.0 ** -8 * ref.abs() if dtype == BF16 else 0.0)
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")))
    worst = ratio.max().item()
    i = [int(v) for v in (ratio == ratio.max()).nonzero()[0]]
    print(f"{what}: worst element at {worst:.3f} of its bound (index {i})")
    assert worst <= 1.0, f"{what}: element {i} is off by {err[tuple(i)].item():.3e}, {worst:.2f}x its bound; got {got[tuple(i)].item()!r}, " \
                         f"reference {ref[tuple(i)].item()!r}"


def assert_col(got, prefill, ref_sum, abs_sum, what, tol=None):
    tol = TOL_COL if tol is None else tol
    got, prefill = got.detach().flatten(), prefill.detach().flatten()
    e, c = col_err(got, prefill, ref_sum.flatten(), abs_sum.flatten())
    print(f"{what}: worst column error {e:.3e} of its conditioning (column {c}; bound {tol:.1e})")
    assert e < tol, f"{what}: column {c} is off by {e:.3e} of its sum of magnitudes (bound {tol:.1e})"


def assert_chan(got, ref, tol, what, scale=None):
    """per channel, relative to |ref| (or to `scale`)"""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    e = (got - ref).abs() / (ref.abs() if scale is None else scale)
    e = torch.where(torch.isnan(e), torch.where(got == ref, 0.0, float("inf")), e)
    c = int(e.argmax())
    print(f"{what}: worst channel error {e[c].item():.3e} (channel {c}; bound {tol:.1e})")
    assert e[c].item() < tol, f"{what}: channel {c} is off by {e[c].item():.3e} (bound {tol:.1e}): got {got[c].item()!r}, reference {ref[c].item()!r}"


def rows2(t):
    return t.reshape(-1, t.shape[-1])


def check_stats(st, pre, y_own, what):
    """stats += (sum y, sum y^2) of the kernel's own (stored) output"""
    yo = rows2(y_own.detach().cpu().double())
    for i, terms in enumerate((yo, yo * yo)):
        s, a = CO.colsum(terms)
        assert_col(st.cpu()[i], pre[i], s, a, f"stats[{i}] {what}")


# ------------------------------------------------------------------------------------------------ convolution inputs
@functools.lru_cache(maxsize=None)
def conv_case(B, T, d, k, dtype, pad_left=-1, bias_off=0.0):
    """seeded operands of one depthwise-convolution problem and its float64 reference (computed once, shared, never modified);
    the taps are random, hence asymmetric: a missing flip or a pad off by one shows.  bias_off: bias = +-bias_off, unit-variance y"""
    g = torch.Generator().manual_seed(100000 * k + 100 * T + d)   # (not the pad: every pad_left sees the same operands)
    r = dict(generator=g)
    pl = (k - 1) // 2 if pad_left < 0 else pad_left
    z = dict(B=B, T=T, d=d, k=k, dtype=dtype, pad_left=pad_left, pl=pl)
    z["x"] = torch.randn(B, T, d, **r).to(dtype)
    z["w"] = torch.randn(d, 1, k, **r) * (k ** -0.5 if bias_off else 0.2)
    z["bias"] = torch.randn(d, **r) if not bias_off else bias_off * (1.0 - 2.0 * (torch.arange(d) % 2))
    z["dy"] = torch.randn(B, T, d, **r).to(dtype)
    z["pre_stats"] = torch.randn(2, d, dtype=F64, **r)
    z["pre_dw"], z["pre_db"] = torch.randn(d, 1, k, **r), torch.randn(d, **r)
    z["y"] = CO.dwconv(z["x"], z["w"], z["bias"], pl)
    z["cy"] = CO.dwconv_cond(z["x"], z["w"], z["bias"], pl)
    z["dx"], z["dw"], z["db"], z["cdx"], z["cdw"], z["cdb"] = CO.dwconv_grads(z["dy"], z["x"], z["w"], pl)
    return z


def run_fwd(z, stats=True, check=True):
    o, (B, T, d, k, dtype) = ops(), (z[n] for n in ("B", "T", "d", "k", "dtype"))
    what = f"B={B} T={T} d={d} k={k} pad_left={z['pad_left']} {DT[dtype]}"
    y = Guarded((B, T, d), dtype, fill=NAN)
    st = Guarded((2, d), F64, src=z["pre_stats"]) if stats else None
    o.dwconv_fwd(put(z["x"]), put(z["w"]), put(z["bias"]), y.t, st.t if stats else None, B, T, d, k, z["pad_left"])
    assert_intact(y=y, **(dict(stats=st) if stats else {}))
    if check:
        assert_conv(y.cpu(), z["y"], z["cy"], k, dtype, f"y {what}")
        if stats:
            check_stats(st, z["pre_stats"], y.t, what)
    return y, st


def run_bwd(z, scratch=True, dbias=True, check=True, dy=None, ref=None):
    """mi355x_dwconv_bwd_ctx; `scratch`: the two-stage reduction (ops always passes one), else float atomics"""
    o, (B, T, d, k, dtype) = ops(), (z[n] for n in ("B", "T", "d", "k", "dtype"))
    what = f"B={B} T={T} d={d} k={k} pad_left={z['pad_left']} {DT[dtype]} scratch={scratch} dbias={dbias}"
    dx = Guarded((B, T, d), dtype, fill=NAN)
    dw = Guarded((d, 1, k), F32, src=z["pre_dw"])
    db = Guarded(d, F32, src=z["pre_db"])
    dyd, xd, wd = put(z["dy"] if dy is None else dy), put(z["x"]), put(z["w"])
    if scratch and dbias:
        o.dwconv_bwd(dyd, xd, wd, dx.t, dw.t, db.t, B, T, d, k, z["pad_left"])
    else:
        n = 4 * B * (k + 1) * d
        sc = Guarded(n, F32, fill=NAN) if scratch else None
        rc = clib().mi355x_dwconv_bwd_ctx(ptr(dyd), ptr(xd), ptr(wd), ptr(dx.t), ptr(dw.t), ptr(db.t) if dbias else 0, o.dt(xd), B, T, d,
                                          k, z["pad_left"], ptr(sc.t) if scratch else 0, n if scratch else 0, o._stream())
        assert rc == 0, rc
        if scratch:
            assert_intact(scratch=sc)
    assert_intact(dx=dx, dw=dw, dbias=db)
    if check:
        check_bwd(z if ref is None else ref, dx, dw, db, what, dbias)
    return dx, dw, db


def check_bwd(ref, dx, dw, db, what, dbias=True):
    k, dtype = ref["k"], ref["dtype"]
    if dx is not None:
        assert_conv(dx.cpu(), ref["dx"], ref["cdx"], k, dtype, f"dx {what}")
    assert_col(dw.cpu(), ref["pre_dw"], ref["dw"], ref["cdw"], f"dw {what}")
    if dbias:
        assert_col(db.cpu(), ref["pre_db"], ref["db"], ref["cdb"], f"dbias {what}")
    else:
        assert torch.equal(bits(db.t), bits(ref["pre_db"])), f"{what}: dbias = NULL, yet the buffer that was not passed changed"


# ------------------------------------------------------------------------------------------------ tile kernels
# DW_CH = 64 channels x DW_TT = 64 frames per workgroup; backward: DW_SEG = 4 segments of ceil(tiles / 4) tiles.  T = 257: 5 tiles,
# 2 per segment, the third segment holds one and the last none.  d: one 16-byte chunk, a full block, a block and one chunk.
TILE_K, TILE_T = (3, 5, 9, 31), (1, 14, 63, 64, 65, 257)
TILE_D = {BF16: (8, 64, 72), F32: (4, 64, 68)}
TILE_CASES = []
for _dt in (F32, BF16):
    _kt = sorted({(k, T) for k in TILE_K for T in (14, 65)} | {(k, T) for k in (3, 31) for T in TILE_T})
    _shapes = [(k, T, TILE_D[_dt][2]) for k, T in _kt] + [(31, 65, d) for d in TILE_D[_dt][:2]]
    TILE_CASES += [pytest.param(_dt, k, T, d, id=f"tile<{DT[_dt]},{k}>-T{T}-d{d}") for k, T, d in _shapes]


@pytest.mark.parametrize("dtype,k,T,d", TILE_CASES)
def test_dwconv_tile_fwd(dtype, k, T, d):
    z = conv_case(2, T, d, k, dtype)
    with dwconv_level(0):
        y, _ = run_fwd(z)
        y2, _ = run_fwd(z, stats=False, check=False)   # stats = NULL: the same y, bit for bit
    assert torch.equal(bits(y2.t), bits(y.t))


@pytest.mark.parametrize("dtype,k,T,d", TILE_CASES)
def test_dwconv_tile_bwd(dtype, k, T, d):
    """with the slab + tap_reduce, with float atomics (scratch = NULL), and without a bias gradient"""
    z = conv_case(2, T, d, k, dtype)
    with dwconv_level(0):
        dx, _, _ = run_bwd(z)
        for scratch, dbias in ((False, True), (True, False), (False, False)):
            dx2, _, _ = run_bwd(z, scratch=scratch, dbias=dbias)
            assert torch.equal(bits(dx2.t), bits(dx.t))


# ------------------------------------------------------------------------------------------------ asymmetric padding
PAD_CASES = [pytest.param(dt_, k, T, id=f"tile<{DT[dt_]},{k}>-T{T}") for dt_ in (F32, BF16) for k in (9, 31) for T in (14, 65)]


def pads(k):
    return (-1, 0, (k - 1) // 2, (k - 1) // 2 + 1, k - 1)


@pytest.mark.parametrize("dtype,k,T", PAD_CASES)
def test_dwconv_pad_left(dtype, k, T):
    """forward pad_shift and the ASYM backward (dy of the tap gradients read from LDS at o + PADR); (k - 1) / 2 is the symmetric
    kernel again and must give -1's bits (y, dx: the reductions end in atomics, whose order is free)"""
    d = TILE_D[dtype][2]
    out = {}
    with dwconv_level(0):
        for p in pads(k):
            z = conv_case(2, T, d, k, dtype, p)
            y, _ = run_fwd(z)
            dx, _, _ = run_bwd(z)
            run_bwd(z, scratch=False)
            out[p] = (bits(y.t), bits(dx.t))
    for a, b2 in zip(out[-1], out[(k - 1) // 2]):
        assert torch.equal(a, b2), f"pad_left = {(k - 1) // 2} is not the symmetric kernel's result"


@pytest.mark.parametrize("k", [9, 31])
def test_dwconv_pad_left_out_of_range_is_an_argument_error(k):
    o, lib = ops(), clib()
    B, T, d = 2, 14, 8
    x, w, b = (torch.zeros(*n, device=dev) for n in ((B, T, d), (d, 1, k), (d,)))
    y, dw, db = torch.zeros_like(x), torch.zeros_like(w), torch.zeros_like(b)
    for p in (k, -2):
        assert lib.mi355x_dwconv_fwd_ctx(ptr(x), ptr(w), ptr(b), ptr(y), 0, 0, B, T, d, k, p, o._stream()) == MI_ERR_ARG
        assert lib.mi355x_dwconv_bwd_ctx(ptr(x), ptr(x), ptr(w), ptr(y), ptr(dw), ptr(db), 0, B, T, d, k, p, 0, 0, o._stream()) == MI_ERR_ARG


# ------------------------------------------------------------------------------------------------ streaming kernels (bf16, k = 31)
# DS_BT = 256 outputs per workgroup in 8 waves of DS_WT = 32, DS_CG = 128 channels; a wave's tile is interior when
# t0 >= 15, t0 + 47 <= T and the channel group is full: wave 1 (t0 = 32) first at T = 79.  Weight gradient: DSW_BT = 128 outputs per
# tile, 4 segments: T = 513 gives segment 0 a second tile.  D templates: 512, 256, run-time (8 / 136: a partly filled group -> edge).
STREAM_T, STREAM_D = (1, 31, 32, 33, 78, 79, 256, 257, 513), (8, 128, 136, 256, 512)
STREAM_CASES = [pytest.param(T, d, id=f"stream<D={d if d in (256, 512) else 0}>-T{T}-d{d}") for d in STREAM_D for T in STREAM_T]


@pytest.mark.parametrize("T,d", STREAM_CASES)
def test_dwconv_stream(T, d):
    z = conv_case(2, T, d, 31, BF16)
    with dwconv_level(2):
        y, _ = run_fwd(z)                                 # STATS = true
        y2, _ = run_fwd(z, stats=False, check=False)      # STATS = false
        dx, _, _ = run_bwd(z)                             # dx: the forward kernel with flipped taps; dw / dbias: slab + tap_reduce
        run_bwd(z, dbias=False)
    assert torch.equal(bits(y2.t), bits(y.t))
    with dwconv_level(1):                                 # forward streams, the backward is still the tile kernel
        y1, _ = run_fwd(z, check=False)
        dx1, _, _ = run_bwd(z)
    with dwconv_level(0):
        dx0, _, _ = run_bwd(z, check=False)
    assert torch.equal(bits(y1.t), bits(y.t)) and torch.equal(bits(dx1.t), bits(dx0.t))


# ------------------------------------------------------------------------------------------------ BatchNorm inputs
@functools.lru_cache(maxsize=None)
def bn_case(M, d, dtype, c0=0.0, s=1.5):
    """c generated directly in the storage dtype, statistics and sums by the oracle; c0: channels centred on +-c0 (else on 0.3)"""
    g = torch.Generator().manual_seed(31 * d + M + int(c0))
    r = dict(generator=g)
    off = c0 * (1.0 - 2.0 * (torch.arange(d) % 2)) if c0 else 0.3
    z = dict(M=M, d=d, dtype=dtype)
    z["c"] = (torch.randn(M, d, **r) * s + off).to(dtype)
    z["gamma"], z["beta"] = torch.rand(d, **r) + 0.5, torch.randn(d, **r) * 0.1
    z["dy"] = torch.randn(M, d, **r).to(dtype)
    z["rm"], z["rv"] = torch.randn(d, **r), torch.rand(d, **r) + 0.5
    z["pre_sums"] = torch.randn(2, d, dtype=F64, **r)
    z["pre_dg"], z["pre_db"] = torch.randn(d, **r), torch.randn(d, **r)
    z["stats"] = CO.bn_stats(z["c"])
    z["mean"], z["rstd"], z["rm1"], z["rv1"] = CO.bn_finalize(z["stats"], M, z["rm"], z["rv"], MOM, EPS)
    z["emean"], z["erstd"] = CO.bn_eval_stats(z["rm"], z["rv"], EPS)
    for mode, (m, rs) in (("", (z["mean"], z["rstd"])), ("e", (z["emean"], z["erstd"]))):   # what the kernels are given: rounded to f32
        m, rs = m.float(), rs.float()
        z[mode + "mean32"], z[mode + "rstd32"] = m, rs
        z[mode + "y"] = CO.bn_swish(z["c"], m, rs, z["gamma"], z["beta"])
        z[mode + "sums"], z[mode + "cond"] = CO.bn_swish_bwd_sums(z["dy"], z["c"], m, rs, z["gamma"], z["beta"])
        z[mode + "dc"] = CO.bn_swish_bwd_apply(z["dy"], z["c"], m, rs, z["gamma"], z["beta"], z[mode + "sums"], M, mode == "")
    return z


# thread mapping CP = min(d / V, 256) chunks x RS = 256 / CP rows: 24 / 12 give CP = 3 and one idle thread, 2056 / 1028 give 257
# chunks (a second channel pass with one live chunk); M = 33: a second reduce workgroup with one row; M = 1: count = 1
BN_M = (1, 33, 450)
BN_CASES = [pytest.param(dt_, d, id=f"{DT[dt_]}-d{d}") for dt_, ds in ((BF16, (8, 24, 512, 2056)), (F32, (4, 12, 512, 1028))) for d in ds]


def dev_count(M):
    return torch.tensor([float(M)], device=dev, dtype=F64)


def check_finalized(z, mean, rstd, rm, rv, what):
    assert_chan(mean.cpu(), z["mean"], TOL_STAT, f"mean {what}", scale=z["mean"].abs().clamp_min(1e-30))
    assert_chan(rstd.cpu(), z["rstd"], TOL_STAT, f"rstd {what}")
    if rm is not None:
        assert_chan(rm.cpu(), z["rm1"], TOL_STAT, f"running_mean {what}", scale=(1 - MOM) * z["rm"].abs().double() + MOM * z["mean"].abs())
        assert_chan(rv.cpu(), z["rv1"], TOL_STAT, f"running_var {what}")


def run_finalize(z, count, running):
    M, d = z["M"], z["d"]
    mean, rstd = Guarded(d, F32, fill=NAN), Guarded(d, F32, fill=NAN)
    rm, rv = (Guarded(d, F32, src=z["rm"]), Guarded(d, F32, src=z["rv"])) if running else (None, None)
    ops().bn_finalize(put(z["stats"]), count, mean.t, rstd.t, rm.t if running else None, rv.t if running else None, MOM, EPS, d)
    assert_intact(mean=mean, rstd=rstd, **(dict(rm=rm, rv=rv) if running else {}))
    return mean, rstd, rm, rv


@pytest.mark.parametrize("dtype,d", BN_CASES)
def test_bn_finalize(dtype, d):
    """bn_finalize_kernel, host and device count, running statistics given and NULL; M = 1 takes the count = 1 branch of the
    running variance"""
    for M in BN_M:
        z = bn_case(M, d, dtype)
        ref = None
        for count in (M, dev_count(M)):
            for running in (True, False):
                mean, rstd, rm, rv = run_finalize(z, count, running)
                check_finalized(z, mean.t, rstd.t, rm.t if running else None, rv.t if running else None, f"M={M} d={d} running={running}")
                ref = ref or (bits(mean.t), bits(rstd.t))
                assert torch.equal(bits(mean.t), ref[0]) and torch.equal(bits(rstd.t), ref[1])


@pytest.mark.parametrize("d", [4, 260, 1028])
def test_bn_eval_stats(d):
    z = bn_case(33, d, F32)
    mean, rstd = Guarded(d, F32, fill=NAN), Guarded(d, F32, fill=NAN)
    ops().bn_eval_stats(put(z["rm"]), put(z["rv"]), mean.t, rstd.t, EPS, d)
    assert_intact(mean=mean, rstd=rstd)
    assert torch.equal(bits(mean.t), bits(z["rm"]))
    assert_chan(rstd.cpu(), z["erstd"], TOL_STAT, f"eval rstd d={d}")


def run_bn_fwd(z, mean32, rstd32):
    M, d, dtype = z["M"], z["d"], z["dtype"]
    y = Guarded((M, d), dtype, fill=NAN)
    ops().bn_swish_fwd(put(z["c"]), put(mean32), put(rstd32), put(z["gamma"]), put(z["beta"]), y.t, M, d)
    assert_intact(y=y)
    return y


def run_bn_stats_fwd(z, count, running):
    M, d, dtype = z["M"], z["d"], z["dtype"]
    y, mean, rstd = Guarded((M, d), dtype, fill=NAN), Guarded(d, F32, fill=NAN), Guarded(d, F32, fill=NAN)
    rm, rv = (Guarded(d, F32, src=z["rm"]), Guarded(d, F32, src=z["rv"])) if running else (None, None)
    ops().bn_stats_swish_fwd(put(z["c"]), put(z["stats"]), count, put(z["gamma"]), put(z["beta"]), y.t, mean.t, rstd.t,
                             rm.t if running else None, rv.t if running else None, MOM, EPS, M, d)
    assert_intact(y=y, mean=mean, rstd=rstd, **(dict(rm=rm, rv=rv) if running else {}))
    return y, mean, rstd, rm, rv


@pytest.mark.parametrize("dtype,d", BN_CASES)
def test_bn_swish_fwd(dtype, d):
    """bn_swish_fwd_kernel on the oracle's statistics (batch and running), and bn_stats_swish_fwd_kernel: the oracle's y, and the
    bits of bn_finalize + bn_swish_fwd"""
    for M in BN_M:
        z = bn_case(M, d, dtype)
        for mode in ("", "e"):
            y = run_bn_fwd(z, z[mode + "mean32"], z[mode + "rstd32"])
            assert_rows(y.cpu(), z[mode + "y"], TOL_Y[dtype], f"y M={M} d={d} {'eval' if mode else 'train'}")
        for count in (M, dev_count(M)):
            for running in (True, False):
                what = f"bn_stats_swish_fwd M={M} d={d} running={running}"
                y, mean, rstd, rm, rv = run_bn_stats_fwd(z, count, running)
                check_finalized(z, mean.t, rstd.t, rm.t if running else None, rv.t if running else None, what)
                assert_rows(y.cpu(), z["y"], TOL_Y[dtype], f"y {what}")
                mean2, rstd2, rm2, rv2 = run_finalize(z, count, running)
                y2 = run_bn_fwd(z, mean2.t, rstd2.t)
                for a, b2 in ((y, y2), (mean, mean2), (rstd, rstd2)) + (((rm, rm2), (rv, rv2)) if running else ()):
                    assert torch.equal(bits(a.t), bits(b2.t)), f"{what}: not the bits of the two-launch form"


def run_bn_reduce(z, scratch, grads, mode=""):
    o, (M, d) = ops(), (z["M"], z["d"])
    sums = Guarded((2, d), F64, src=z["pre_sums"])
    dg, db = (Guarded(d, F32, src=z["pre_dg"]), Guarded(d, F32, src=z["pre_db"])) if grads else (None, None)
    a = [put(z[n]) for n in ("dy", "c", mode + "mean32", mode + "rstd32", "gamma", "beta")]
    if scratch:
        o.bn_swish_bwd_reduce(*a, sums.t, M, d, dgamma=dg.t if grads else None, dbeta=db.t if grads else None)
    else:   # ops always passes a slab: the single-stage path (f64 atomics per workgroup) through the library
        rc = clib().mi355x_bn_swish_bwd_reduce(*[ptr(t) for t in a], ptr(sums.t), ptr(dg.t) if grads else 0, ptr(db.t) if grads else 0,
                                               o.dt(a[0]), M, d, 0, 0, o._stream())
        assert rc == 0, rc
    assert_intact(sums=sums, **(dict(dgamma=dg, dbeta=db) if grads else {}))
    return sums, dg, db


@pytest.mark.parametrize("dtype,d", BN_CASES)
def test_bn_swish_bwd_reduce(dtype, d):
    """sums, dgamma and dbeta all accumulate: dgamma / dbeta get the LOCAL sums of the call, whatever sums held before"""
    for M in BN_M:
        z = bn_case(M, d, dtype)
        for scratch in (True, False):
            for grads in (True, False):
                what = f"M={M} d={d} scratch={scratch} grads={grads}"
                sums, dg, db = run_bn_reduce(z, scratch, grads)
                for i in (0, 1):
                    assert_col(sums.cpu()[i], z["pre_sums"][i], z["sums"][i], z["cond"][i], f"sums[{i}] {what}")
                if grads:
                    assert_col(db.cpu(), z["pre_db"], z["sums"][0], z["cond"][0], f"dbeta {what}")
                    assert_col(dg.cpu(), z["pre_dg"], z["sums"][1], z["cond"][1], f"dgamma {what}")
        dg, db = Guarded(d, F32, src=z["pre_dg"]), Guarded(d, F32, src=z["pre_db"])
        ops().bn_param_grad(put(z["sums"]), dg.t, db.t, d)   # dbeta += (float)sums[0], dgamma += (float)sums[1]
        assert_intact(dgamma=dg, dbeta=db)
        assert_col(db.cpu(), z["pre_db"], z["sums"][0], z["sums"][0].abs(), f"bn_param_grad dbeta M={M} d={d}")
        assert_col(dg.cpu(), z["pre_dg"], z["sums"][1], z["sums"][1].abs(), f"bn_param_grad dgamma M={M} d={d}")


def run_bn_apply(z, count, training, tol=None):
    M, d, dtype = z["M"], z["d"], z["dtype"]
    mode = "" if training else "e"
    # eval mode must not look at the sums: NaN
    sums = z["sums"] if training else torch.full((2, d), NAN, dtype=F64)
    dc = Guarded((M, d), dtype, fill=NAN)
    ops().bn_swish_bwd_apply(put(z["dy"]), put(z["c"]), put(z[mode + "mean32"]), put(z[mode + "rstd32"]), put(z["gamma"]), put(z["beta"]),
                             put(sums), count, training, dc.t, M, d)
    assert_intact(dc=dc)
    what = f"dc M={M} d={d} training={training}"
    if M <= 2 and training:
        # one row is its own mean and two rows have xhat = +-1: dz - sums[0] / M - xhat * sums[1] / M cancels (to exactly zero for
        # M = 1, to eps / var of its terms for M = 2), so the rows are measured against the cancellation-free gamma * rstd * dz
        dz = CO.bn_swish_bwd_terms(z["dy"], z["c"], z["mean32"], z["rstd32"], z["gamma"], z["beta"])[0]
        scale = (z["gamma"].double() * z["rstd32"].double() * dz).abs().amax(1)
        e = ((dc.cpu().double() - z["dc"]).abs().amax(1) / scale).max().item()
        print(f"{what}: {e:.3e} of the row's largest term")
        assert e < (tol or TOL_G[dtype]), what
    else:
        assert_rows(dc.cpu(), z[mode + "dc"], tol or TOL_G[dtype], what)
    return dc


@pytest.mark.parametrize("dtype,d", BN_CASES)
def test_bn_swish_bwd_apply(dtype, d):
    for M in BN_M:
        z = bn_case(M, d, dtype)
        for training in (1, 0):
            a = run_bn_apply(z, M, training)
            b2 = run_bn_apply(z, dev_count(M), training)
            assert torch.equal(bits(a.t), bits(b2.t)), f"M={M} d={d} training={training}: host and device count differ"


def test_bn_backward_null_statistics_are_argument_errors():
    """mean, rstd, gamma, beta are dereferenced by the kernels: NULL must come back as MI_ERR_ARG before any launch"""
    o, lib = ops(), clib()
    M, d = 4, 8
    t = torch.zeros(M, d, device=dev)
    v = torch.ones(d, device=dev)
    sums = torch.zeros(2, d, device=dev, dtype=F64)
    good = [ptr(t), ptr(t), ptr(v), ptr(v), ptr(v), ptr(v)]
    out, slab, cnt = torch.zeros(M, d, device=dev), torch.zeros(2 * d, device=dev), dev_count(M)
    for i in range(2, 6):
        a = list(good)
        a[i] = 0
        for sc in (0, ptr(slab)):
            assert lib.mi355x_bn_swish_bwd_reduce(*a, ptr(sums), 0, 0, 0, M, d, sc, 2 * d if sc else 0, o._stream()) == MI_ERR_ARG
        assert lib.mi355x_bn_swish_bwd_apply(*a, ptr(sums), float(M), 1, ptr(out), 0, M, d, o._stream()) == MI_ERR_ARG
        assert lib.mi355x_bn_swish_bwd_apply_dev_count(*a, ptr(sums), ptr(cnt), 0, ptr(out), 0, M, d, o._stream()) == MI_ERR_ARG
    torch.cuda.synchronize()
    assert not sums.any() and not out.any()
    assert lib.mi355x_bn_swish_bwd_apply(*good, ptr(sums), float(M), 1, ptr(out), 0, M, d, o._stream()) == 0


# ------------------------------------------------------------------------------------------------ fused BatchNorm + Swish backward
@functools.lru_cache(maxsize=None)
def fused_case(B, T, d, k, dtype):
    """the convolution problem of conv_case with a BatchNorm + Swish in front of its backward: cc (the BatchNorm input) is generated
    directly in the storage dtype, its statistics and the sums come from the oracle"""
    z = dict(conv_case(B, T, d, k, dtype))
    bn = bn_case(B * T, d, dtype)
    z.update({n: bn[n] for n in bn if n not in ("M", "d", "dtype", "pre_db")})
    return z


def own_dc(z, training):
    """what bn_swish_bwd_apply_kernel writes for this case: the values the fused kernel's tile holds"""
    B, T, d, dtype = z["B"], z["T"], z["d"], z["dtype"]
    bn = bn_case(B * T, d, dtype)
    return run_bn_apply(bn, B * T, training).t.view(B, T, d)


def own_ref(z, training):
    """the oracle's convolution backward of that gradient"""
    ref = dict(z)
    ref["dx"], ref["dw"], ref["db"], ref["cdx"], ref["cdw"], ref["cdb"] = CO.dwconv_grads(own_dc(z, training), z["x"], z["w"], z["pl"])
    return ref


def run_fused(z, training, count=None, scratch="ops", defer=False, dbias=True, glu=None):
    """mi355x_dwconv_bwd_bnswish; scratch: 'ops' (the wrapper's shared slab), 'own' (a guarded slab of the caller's) or None"""
    o, (B, T, d, k, dtype) = ops(), (z[n] for n in ("B", "T", "d", "k", "dtype"))
    mode = "" if training else "e"
    sums = z["sums"] if training else torch.full((2, d), NAN, dtype=F64)
    dx = Guarded((B, T, d), dtype, fill=NAN) if glu is None else None
    dw, db = Guarded((d, 1, k), F32, src=z["pre_dw"]), Guarded(d, F32, src=z["pre_db"])
    n = 4 * B * (k + 1) * d
    sc = Guarded(n, F32, fill=NAN) if scratch == "own" else None
    a = [put(z["dy"]), put(rows2(z["c"]).view(B, T, d)), put(z[mode + "mean32"]), put(z[mode + "rstd32"]), put(z["gamma"]), put(z["beta"]),
         put(sums)]
    count = B * T if count is None else count
    g = glu or {}
    xd, wd = put(z["x"]), put(z["w"])
    if scratch is None or not dbias:
        cd = count if isinstance(count, torch.Tensor) else None
        rc = clib().mi355x_dwconv_bwd_bnswish(*[ptr(t) for t in a], 0.0 if cd is not None else float(count), ptr(cd), int(training),
                                              ptr(xd), ptr(wd), ptr(dx.t) if dx else 0, ptr(dw.t), ptr(db.t) if dbias else 0,
                                              ptr(g.get("glu_in")), ptr(g.get("glu_din")), ptr(g.get("glu_len")), ptr(g.get("glu_cu")),
                                              g.get("glu_act", 0), o.dt(a[0]), B, T, d, k, ptr(sc.t) if sc else 0, n if sc else 0,
                                              int(defer), o._stream())
        torch.cuda.synchronize()
        if defer and not sc:
            assert rc == MI_ERR_ARG, rc
            return dx, dw, db, sc
        assert rc == 0, rc
    else:
        o.dwconv_bwd_bnswish(*a, count, training, xd, wd, dx.t if dx else None, dw.t, db.t, B, T, d, k,
                             scratch=sc.t if sc else None, defer_reduce=defer, **g)
    assert_intact(dw=dw, dbias=db, **(dict(dx=dx) if dx else {}), **(dict(scratch=sc) if sc else {}))
    return dx, dw, db, sc


@pytest.mark.parametrize("dtype,k,T,d", TILE_CASES)
def test_dwconv_bwd_bnswish(dtype, k, T, d):
    """dwconv_bwd_kernel<BN>: train and eval coefficients, host and device count, the slab, float atomics, the deferred tap
    reduction, no bias gradient.  The convolution is judged on the gradient the stand-alone BatchNorm backward wrote (per element
    and per column), the whole fusion per row against the oracle with the intermediate rounded to the activation type."""
    B = 2
    z = fused_case(B, T, d, k, dtype)
    what = f"fused T={T} d={d} k={k} {DT[dtype]}"
    with dwconv_level(0):
        for training in (1, 0):
            ref = own_ref(z, training)
            dx, dw, db, _ = run_fused(z, training)
            check_bwd(ref, dx, dw, db, f"{what} training={training}")
            if not (training and B * T <= 2):   # (two rows in training mode: dc is the remainder of a cancellation, see run_bn_apply)
                dcc = z["dc" if training else "edc"].view(B, T, d).to(dtype)   # the oracle's, rounded as the tile rounds it
                assert_rows(rows2(dx.cpu()), rows2(CO.dwconv_grads(dcc, z["x"], z["w"], z["pl"])[0]), TOL_G[dtype],
                            f"dx {what} training={training}")
            dx2, dw2, db2, _ = run_fused(z, training, count=dev_count(B * T))
            assert torch.equal(bits(dx2.t), bits(dx.t)), f"{what}: host and device count differ"
            check_bwd(ref, None, dw2, db2, f"{what} device count")
            dx3, dw3, db3, _ = run_fused(z, training, scratch=None)            # float atomics
            assert torch.equal(bits(dx3.t), bits(dx.t))
            check_bwd(ref, None, dw3, db3, f"{what} scratch=NULL")
            _, dw4, db4, _ = run_fused(z, training, dbias=False, scratch="own")
            check_bwd(ref, None, dw4, db4, f"{what} dbias=NULL", dbias=False)
        # defer_tap_reduce: the kernel leaves the slabs, mi355x_dwconv_tap_reduce adds them.  The slabs and dx are deterministic and
        # must be the non-deferred call's bits; dw / dbias end in 4-way float atomics either way, whose order is free
        dx5, dw5, db5, sc5 = run_fused(z, 1, scratch="own")
        dx6, dw6, db6, sc6 = run_fused(z, 1, scratch="own", defer=True)
        assert torch.equal(bits(dx6.t), bits(dx5.t)) and torch.equal(bits(sc6.t), bits(sc5.t))
        assert not torch.isnan(sc6.t).any(), "a slab entry was left unwritten"
        assert torch.equal(bits(dw6.t), bits(z["pre_dw"])) and torch.equal(bits(db6.t), bits(z["pre_db"])), "deferred, yet dw / dbias changed"
        ops().dwconv_tap_reduce(sc6.t, B, d, k, dw6.t, db6.t)
        assert_intact(dw=dw6, dbias=db6)
        check_bwd(own_ref(z, 1), None, dw6, db6, f"{what} deferred + tap_reduce")
        assert rel_err(dw6.t, dw5.t) < 1e-6 and rel_err(db6.t, db5.t) < 1e-6
        # defer without a slab of the caller's: an argument error, and nothing was launched
        _, dw7, db7, _ = run_fused(z, 1, scratch=None, defer=True)
        assert torch.equal(bits(dw7.t), bits(z["pre_dw"])) and torch.equal(bits(db7.t), bits(z["pre_db"])), \
            "MI_ERR_ARG came back, yet the kernel had been launched and added to dw / dbias"


# ------------------------------------------------------------------------------------------------ GLU / Swish fused variants
GLU_T, GLU_K = 70, 31   # two time tiles, the halo of the second reaches into the first


def glu_lens(which, T):
    return [T, T - 7, 0] if which == 0 else [1, T, 5]


@functools.lru_cache(maxsize=None)
def glu_case(dtype, act, which):
    """pointwise-conv output p on the padded grid; frames beyond len[b] hold finite garbage (+-1e4) that a kernel must not use"""
    B, T, d = 3, GLU_T, TILE_D[dtype][2]
    z = dict(fused_case(B, T, d, GLU_K, dtype))
    g = torch.Generator().manual_seed(500 + 10 * act + which)
    lens = glu_lens(which, T)
    width = 2 * d if act == 0 else d
    p = torch.randn(B, T, width, generator=g)
    pad = torch.arange(T)[None] >= torch.tensor(lens)[:, None]
    p[pad] = 1e4 * (1.0 - 2.0 * (torch.arange(width) % 2))
    z["p"] = p.view(B * T, width).to(dtype)
    z["lens"] = lens
    z["cu"] = [0] + [sum(lens[:i + 1]) for i in range(B)]
    z["rows"] = torch.cat([torch.arange(n) + b * T for b, n in enumerate(lens)])
    z["fn"] = CO.glu_mask if act == 0 else CO.swish_mask
    z["gout"] = z["fn"](z["p"], lens, T)
    return z


GLU_CASES = [pytest.param(dt_, act, packed, which, id=f"{DT[dt_]}-{'swish' if act else 'glu'}-{'packed' if packed else 'padded'}-lens{which}")
             for dt_ in (F32, BF16) for act in (0, 1) for packed in (0, 1) for which in (0, 1)]


@pytest.mark.parametrize("dtype,act,packed,which", GLU_CASES)
def test_dwconv_fwd_glu(dtype, act, packed, which):
    o = ops()
    z = glu_case(dtype, act, which)
    B, T, d, k, lens = z["B"], z["T"], z["d"], z["k"], z["lens"]
    what = f"{DT[dtype]} act={act} packed={packed} lens={lens}"
    pin = put(z["p"][z["rows"]] if packed else z["p"])
    lens_d = torch.tensor(lens, dtype=torch.int64, device=dev)
    cu_d = torch.tensor(z["cu"], dtype=torch.int64, device=dev) if packed else None
    with dwconv_level(0):
        for stats in (True, False):
            gout, y = Guarded((B, T, d), dtype, fill=NAN), Guarded((B, T, d), dtype, fill=NAN)
            st = Guarded((2, d), F64, src=z["pre_stats"]) if stats else None
            o.dwconv_fwd_glu(pin, lens_d, cu_d, gout.t, put(z["w"]), put(z["bias"]), y.t, st.t if stats else None, B, T, d, k, act=act)
            assert_intact(gout=gout, y=y, **(dict(stats=st) if stats else {}))
            assert_rows(rows2(gout.cpu()), rows2(z["gout"]), TOL_ACT[dtype], f"activation {what}")
            for b in range(B):
                assert not gout.cpu()[b, lens[b]:].any(), f"{what}: utterance {b} is not zero beyond its length"
            # the convolution on the kernel's own activation output (what its tile held)
            assert_conv(y.cpu(), CO.dwconv(gout.cpu(), z["w"], z["bias"], z["pl"]), CO.dwconv_cond(gout.cpu(), z["w"], z["bias"], z["pl"]),
                        k, dtype, f"y {what}")
            if stats:
                check_stats(st, z["pre_stats"], y.t, what)
        # the two-launch form: stand-alone activation + mask, then the plain forward (the stand-alone Swish has no packed form)
        if act == 0 or not packed:
            g2, y2 = Guarded((B, T, d), dtype, fill=NAN), Guarded((B, T, d), dtype, fill=NAN)
            if act == 0:
                o.glu_fwd(pin, g2.t.view(B * T, d), lens_d, T, B * T, d, cu=cu_d)
            else:
                o.swish_mask_fwd(pin, g2.t.view(B * T, d), lens_d, T, B * T, d)
            o.dwconv_fwd(g2.t, put(z["w"]), put(z["bias"]), y2.t, None, B, T, d, k)
            torch.cuda.synchronize()
            assert torch.equal(bits(gout.t), bits(g2.t)) and rel_err(y.t, y2.t) < 1e-6


@pytest.mark.parametrize("dtype,act,packed,which", GLU_CASES)
def test_dwconv_bwd_bnswish_glu(dtype, act, packed, which):
    """the GLU / Swish backward on the way out of the fused backward's tile: the oracle's mask backward of the oracle's dx (on the
    stand-alone kernel's dc, rounded to the activation type as the two-launch form rounds it), and the two-launch form itself"""
    o = ops()
    z = glu_case(dtype, act, which)
    B, T, d, k, lens = z["B"], z["T"], z["d"], z["k"], z["lens"]
    what = f"{DT[dtype]} act={act} packed={packed} lens={lens}"
    p = z["p"][z["rows"]] if packed else z["p"]
    pin = put(p)
    lens_d = torch.tensor(lens, dtype=torch.int64, device=dev)
    cu_d = torch.tensor(z["cu"], dtype=torch.int64, device=dev) if packed else None
    with dwconv_level(0):
        ref = own_ref(z, 1)
        din = Guarded(p.shape, dtype, fill=NAN)
        glu = dict(glu_in=pin, glu_din=din.t, glu_len=lens_d, glu_cu=cu_d, glu_act=act)
        _, dw, db, _ = run_fused(z, 1, glu=glu)
        assert_intact(glu_din=din)
        check_bwd(ref, None, dw, db, f"fused + mask backward {what}")
        e = ref["dx"].to(dtype)
        want = CO.mask_bwd(z["fn"], p, e, lens, T, z["cu"] if packed else None)
        got = din.cpu()
        assert torch.isfinite(got.float()).all(), f"{what}: a row was left unwritten or took garbage in"
        assert_rows(got, want, TOL_G[dtype], f"d(activation input) {what}")
        if not packed:
            pad = (torch.arange(T)[None] >= torch.tensor(lens)[:, None]).view(B * T)
            assert not got[pad].any(), f"{what}: rows beyond the length are not zero"
        if act == 0 or not packed:   # the two-launch form: fused dx, then the stand-alone mask backward
            dx, _, _, _ = run_fused(z, 1)
            two = Guarded(p.shape, dtype, fill=NAN)
            if act == 0:
                o.glu_bwd(pin, dx.t.view(B * T, d), two.t, lens_d, T, B * T, d, cu=cu_d)
            else:
                o.swish_mask_bwd(pin, dx.t.view(B * T, d), two.t, lens_d, T, B * T, d)
            torch.cuda.synchronize()
            assert rel_err(din.t, two.t) < 1e-5, rel_err(din.t, two.t)


# ------------------------------------------------------------------------------------------------ offset inputs
def off_conv_case(dtype, c0):
    return conv_case(OFF_B, OFF_T, OFF_D, 31, dtype, -1, c0)


def off_bn_case(dtype, c0, s):
    return bn_case(OFF_B * OFF_T, OFF_D, dtype, c0, s)


def off_tol(dtype, c0, s):
    rstd, y, dc = TOL_OFF[(c0, s)]
    return (rstd, y, dc) if dtype == F32 else (rstd, TOL_Y[BF16], TOL_G[BF16])


OFF_CASES = [pytest.param(dt_, lvl, c0, s, id=f"{'stream' if lvl else 'tile'}<{DT[dt_]}>-c{int(c0)}-s{int(s)}")
             for dt_, lvl in ((F32, 0), (BF16, 0), (BF16, 1)) for c0, s in OFF_CS]


@pytest.mark.parametrize("dtype,level,c0,s", OFF_CASES)
def test_forward_statistics_of_an_offset_output(dtype, level, c0, s):
    """a depthwise bias of c0 standard deviations: the raw sums the forward leaves must still give the rstd of its own output"""
    z = off_conv_case(dtype, c0)
    B, T, d = z["B"], z["T"], z["d"]
    with dwconv_level(level):
        y, st = run_fwd(z)
    zero = Guarded((2, d), F64, fill=0.0)
    with dwconv_level(level):
        ops().dwconv_fwd(put(z["x"]), put(z["w"]), put(z["bias"]), y.t, zero.t, B, T, d, z["k"], -1)
    mean, rstd = Guarded(d, F32, fill=NAN), Guarded(d, F32, fill=NAN)
    ops().bn_finalize(zero.t, B * T, mean.t, rstd.t, None, None, MOM, EPS, d)
    assert_intact(stats=zero, mean=mean, rstd=rstd)
    own = CO.bn_finalize(CO.bn_stats(y.cpu()), B * T, None, None, MOM, EPS)
    std = 1.0 / own[1]
    print(f"output: |mean| / std between {(own[0].abs() / std).min().item():.1f} and {(own[0].abs() / std).max().item():.1f}")
    assert_chan(mean.cpu(), own[0], TOL_STAT, f"mean c0={c0}")
    assert_chan(rstd.cpu(), own[1], TOL_OFF[(c0, s)][0], f"rstd c0={c0}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("c0,s", OFF_CS)
def test_bn_kernels_on_offset_inputs(dtype, c0, s):
    z = off_bn_case(dtype, c0, s)
    M, d = z["M"], z["d"]
    tol_rstd, tol_y, tol_dc = off_tol(dtype, c0, s)
    y = run_bn_fwd(z, z["mean32"], z["rstd32"])
    assert_rows(y.cpu(), z["y"], tol_y, f"y c0={c0} s={s}")
    y2, mean, rstd, _, _ = run_bn_stats_fwd(z, M, True)
    assert_chan(mean.cpu(), z["mean"], TOL_STAT, f"mean c0={c0} s={s}")
    assert_chan(rstd.cpu(), z["rstd"], tol_rstd, f"rstd c0={c0} s={s}")
    assert_rows(y2.cpu(), z["y"], tol_y, f"bn_stats_swish_fwd y c0={c0} s={s}")
    sums, dg, db = run_bn_reduce(z, True, True)
    for i in (0, 1):
        assert_col(sums.cpu()[i], z["pre_sums"][i], z["sums"][i], z["cond"][i], f"sums[{i}] c0={c0} s={s}")
    run_bn_apply(z, M, 1, tol=tol_dc)


# ------------------------------------------------------------------------------------------------ reference-error measurement
def _f32_col(terms, prefill):
    """error of prefill + torch.sum(terms.float(), 0) against float64, per column of its conditioning: the worst column"""
    terms = rows2(terms.double())
    s, a = CO.colsum(terms)
    got = prefill.flatten() + torch.sum(terms.float(), 0).to(prefill.dtype)
    return col_err(got, prefill.flatten(), s, a)[0]


def _conv_cols(z, dy=None, stats=True):
    worst = 0.0
    d, k = z["d"], z["k"]
    if stats:
        y = rows2(z["y"].to(z["dtype"]).double())
        worst = max(worst, _f32_col(y, z["pre_stats"][0]), _f32_col(y * y, z["pre_stats"][1]))
    dy = z["dy"] if dy is None else dy
    worst = max(worst, _f32_col(dy, z["pre_db"]))
    for j, t in enumerate(CO.dwconv_dw_terms(dy, z["x"], k, z["pl"])):
        worst = max(worst, _f32_col(t, z["pre_dw"].view(d, k)[:, j]))
    return worst


def _bn_cols(z):
    dz, dzx, _ = CO.bn_swish_bwd_terms(z["dy"], z["c"], z["mean32"], z["rstd32"], z["gamma"], z["beta"])
    return max(_f32_col(dz, z["pre_sums"][0]), _f32_col(dzx, z["pre_sums"][1]), _f32_col(dz, z["pre_db"]), _f32_col(dzx, z["pre_dg"]))


def _cpu_f32_offset_errors(c0, s):
    """(rstd per channel, y per row, dc per row) of float32 torch on the CPU against the oracle"""
    z = off_bn_case(F32, c0, s)
    c = z["c"].clone().requires_grad_(True)
    y = F.silu(F.batch_norm(c, None, None, z["gamma"], z["beta"], True, MOM, EPS))
    y.backward(z["dy"])
    rstd = (z["c"].var(0, unbiased=False) + EPS).rsqrt()
    y64 = CO.bn_swish(z["c"], z["mean"], z["rstd"], z["gamma"], z["beta"])
    sums, _ = CO.bn_swish_bwd_sums(z["dy"], z["c"], z["mean"], z["rstd"], z["gamma"], z["beta"])
    dc64 = CO.bn_swish_bwd_apply(z["dy"], z["c"], z["mean"], z["rstd"], z["gamma"], z["beta"], sums, z["M"], True)
    return ((rstd.double() - z["rstd"]).abs() / z["rstd"]).max().item(), row_err(y.detach(), y64)[0], row_err(c.grad, dc64)[0]


def measure_reference_errors():
    """the float32 CPU figures the measured bounds at the top of this file are derived from (no GPU needed)"""
    worst = 0.0
    for p in TILE_CASES:
        dtype, k, T, d = p.values
        worst = max(worst, _conv_cols(conv_case(2, T, d, k, dtype)))
        z = fused_case(2, T, d, k, dtype)
        for mode in ("dc", "edc"):
            worst = max(worst, _conv_cols(z, dy=z[mode].view(2, T, d).to(dtype), stats=False))
    for p in PAD_CASES:
        dtype, k, T = p.values
        for pl in pads(k):
            worst = max(worst, _conv_cols(conv_case(2, T, TILE_D[dtype][2], k, dtype, pl)))
    for p in STREAM_CASES:
        T, d = p.values
        worst = max(worst, _conv_cols(conv_case(2, T, d, 31, BF16)))
    for p in GLU_CASES:
        dtype, act, _, which = p.values
        z = glu_case(dtype, act, which)
        y = rows2(CO.dwconv(z["gout"].to(dtype), z["w"], z["bias"], z["pl"]).to(dtype).double())
        worst = max(worst, _f32_col(y, z["pre_stats"][0]), _f32_col(y * y, z["pre_stats"][1]),
                    _conv_cols(z, dy=z["dc"].view(3, GLU_T, z["d"]).to(dtype), stats=False))
    for p in BN_CASES:
        dtype, d = p.values
        for M in BN_M:
            worst = max(worst, _bn_cols(bn_case(M, d, dtype)))
    for c0, s in OFF_CS:
        for dtype in (F32, BF16):
            worst = max(worst, _conv_cols(off_conv_case(dtype, c0)), _bn_cols(off_bn_case(dtype, c0, s)))
    print(f"reduced columns, float32 torch.sum, worst column: {worst:.3e} -> x8 = {8 * worst:.3e}")
    for c0, s in OFF_CS:
        r, y, dc = _cpu_f32_offset_errors(c0, s)
        print(f"(c0, s) = ({c0}, {s}): float32 torch: rstd {r:.3e} -> x4 = {4 * r:.3e}; y {y:.3e} -> x4 = {4 * y:.3e}; "
              f"dc {dc:.3e} -> x4 = {4 * dc:.3e}")


if __name__ == "__main__":
    measure_reference_errors()
