"""-m gpu: every kernel path of nemo_amd/csrc/subsample.hip (conv1 forward / backward, im2col, col2im) and nemo_amd/csrc/dwconv2d.hip
(depthwise 3x3 stride-2 forward, input gradient, weight gradient), and tap_reduce_kernel of common.h behind both weight gradients,
through the C ABI against the float64 reference of tests/subsample_oracle.py.

Operands are generated in their storage dtype and the oracle up-casts them.  Every overwritten output (out1, col, din, out) sits
between 64-byte guards of -0.0f and is pre-filled with NaN; the `+=` outputs (dw, db, dbias) are pre-filled with random values and
the reference adds the prefill; the scratch slab is guarded at exactly the element count the launcher demands, NaN-filled, and
must come back fully written.  Activations fed to the gated kernels are post-ReLU: about half are exactly zero, some are -0.0.

Error measures (no element and no case is excluded from any of them)
  convolution outputs (conv1 fwd, dwconv2d fwd, dwconv2d bwd-data, col2im), per element:
      |got - ref| <= n * 2^-24 * cond  [+ 2^-8 * |ref| for bf16 outputs],  cond = |bias| + sum |w * x|,
      n = float32 operations in the chain: 10 for the two forwards, 4 for the two input gradients (at most 2 x 2 taps reach an
      input position).  Derived, no margin (assert_conv of tests/test_convmod_kernels_gpu.py).  conv1's output is judged after
      the ReLU with the pre-activation's cond (ReLU is 1-Lipschitz); rows t1 >= len1 must be exactly zero; input gradients must
      be exactly zero where the stored activation is <= 0.
  im2col: the oracle's bits; taps outside the grid are all-zero words.
  reduced columns (conv1 dw / db, dwconv2d dw / dbias, tap_reduce on the slab the first stage left), per column:
      |got - (prefill + sum)| / (|prefill| + sum |term|) < TOL_COL
      Measured: the same sums taken in float32 by torch.sum on the CPU (f32_col_error of tests/test_subsample_host.py) against
      the oracle, worst column over every input of this file, and 8x that for the kernels (another order of additions, finished
      through atomics):   measured 1.80e-07 -> bound 1.4e-06
`python tests/test_subsample_kernels_gpu.py` re-measures that figure on the CPU.

Which case reaches which lane layout (V = 4 channels per lane in f32, 8 in bf16; chunks = C / V)
  conv1_bwd_kernel: CL lanes over chunks, NF = 64 / CL f1 positions per wave step, ceil(chunks / CL) passes over c0
      f32   C =    4   chunks   1   CL  1  NF 64  butterfly over 6 levels; F1 = 1, 2, 9, 10, 40, 41, 64, 65 around NF
            C =  176           44   CL 64  NF  1  20 idle lanes
            C =  256           64   CL 64  NF  1  exactly one wave
            C =  324           81   CL 64  NF  1  2 passes, the second with 17 live lanes
            C =  512          128   CL 64  NF  1  2 full passes
            C = 1024          256   CL 64  NF  1  4 passes
            C = 2048          512   CL 64  NF  1  8 passes (backward only: the forward rejects chunks > 256)
      bf16  C =    8            1   CL  1  NF 64
            C =   32            4   CL  4  NF 16  butterfly over 4 levels
            C =  176           22   CL 64  NF  1  42 idle lanes
            C =  256           32   CL 32  NF  2  butterfly over 1 level
            C =  328           41   CL 64  NF  1  23 idle lanes
            C = 2048          256   CL 64  NF  1  4 passes
      row blocks C1_TB = 32 (backward) and C1_TR = 4 (forward): T1 = 1, 2 | 19, 31 (partial last block) | 20, 32 (full) | 33, 65
      (a last block of one row) | 66; parts = B * ceil(T1 / 32) = 3, 6, 9, and 1, 3, 16, 17, 67 in test_tap_reduce_part_counts
  conv1_fwd_kernel / dwconv2d kernels: FS = PS = 256 / chunks positions in flight, 256 - PS * chunks idle threads
      f32   C = 4: 256 | 176: 5 (36 idle) | 256: 4 | 324: 3 (13 idle) | 512: 2 | 1024: 1
      bf16  C = 8: 256 | 32: 64 | 176: 11 (14 idle) | 256: 8 | 328: 6 (10 idle) | 2048: 1
  dwconv2d_s2_bwd_w_kernel: parts = ceil(npos / 64) below 65536 output positions, else 1024
      npos = 1, 63, 64 -> 1 part | 65 -> 2 parts, the second holds the last positions | B = 3 grids: 1 .. 16 parts
      npos = 65792 -> 1024 parts of 65, the last 11 empty (test_dwconv2d_bwd_w_many_parts)
  grid-stride second trips: im2col / col2im above 16384 * 256 vectors (test_im2col_col2im_second_trip), dwconv2d fwd / bwd-data
      above 8192 * PS positions at PS = 1 (test_dwconv2d_second_trip)
Out of reach: the `long long` index instantiation of the three dwconv2d kernels is chosen at B * T1 * F1 > 2^32 - 2^21 positions,
at least 68 GB of input even at C = 8 in bf16.  No test runs it, and there is no hook to force it.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subsample_oracle as SO  # noqa: E402
from test_convmod_kernels_gpu import assert_col as _assert_col, assert_conv  # noqa: E402
from test_norm_kernels_gpu import Guarded, assert_intact, bits, put  # noqa: E402
from test_subsample_host import f32_col_error  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16, I64 = torch.float32, torch.bfloat16, torch.int64
DT = {F32: "f32", BF16: "bf16"}
VEC = {F32: 4, BF16: 8}
NAN = float("nan")
MI_ERR_ARG = 1
N_FWD, N_DGRAD = 10, 4    # float32 operations in a forward chain (bias + 9 taps) / an input-gradient chain (at most 2 x 2 taps)
TOL_COL = 1.4e-6          # measured 1.80e-07 -> bound 1.4e-06 (see the header)

PADS = (1, 2)
CH = {F32: (4, 176, 256, 324, 512, 1024), BF16: (8, 32, 176, 256, 328, 2048)}
CH_BWD = {F32: CH[F32] + (2048,), BF16: CH[BF16]}
GEOM = ((80, 61), (17, 38), (18, 37), (128, 64), (3, 130), (2, 2), (1, 1))          # (F, T) of the mel
GRIDS = ((31, 40), (19, 9), (18, 9), (1, 1), (2, 2), (65, 3))                         # (T1, F1) of the depthwise input
COL_GRIDS = ((31, 40), (19, 9), (18, 9), (1, 1), (2, 3))                              # (T1, F1) of im2col / col2im
COL_CH = (8, 176)


def _params(ch):
    return [pytest.param(dt_, C, pad, id=f"{DT[dt_]}-C{C}-pad{pad}") for dt_ in (F32, BF16) for C in ch[dt_] for pad in PADS]


def ops():
    from nemo_amd import ops as _ops
    return _ops


def clib():
    from nemo_amd._lib import lib
    return lib


def ptr(t):
    return 0 if t is None else (t.t if isinstance(t, Guarded) else t).data_ptr()


def code(dtype):
    return ops().dt(dtype)


def on_dev(z, *names):
    """the named operands on the device; the caller holds them until it has synchronised"""
    return [put(z[n]) for n in names]


def assert_col(got, prefill, ref_sum, abs_sum, what):
    _assert_col(got, prefill, ref_sum.contiguous(), abs_sum.contiguous(), what, tol=TOL_COL)


def gen(*key):
    return torch.Generator().manual_seed(sum(int(v) * 1009 ** i for i, v in enumerate(key)) % (2 ** 31))


def post_relu(shape, dtype, g):
    """a stored ReLU output: about half the entries exactly zero, some of them -0.0"""
    r = torch.randn(*shape, generator=g)
    return torch.where(r < -1.2, torch.tensor(-0.0), torch.relu(r)).to(dtype)


def std_len0(T):
    return [T, min(T, max(1, (2 * T // 3) | 1)), 1]


def next_lens(lens, pad):
    return [max(0, SO.half_len(int(n), pad)) for n in lens]


def assert_zero_where(got, mask, what):
    got = got.detach().cpu()
    assert not got[mask.expand_as(got)].any(), f"{what}: not exactly zero"


def check_slab(sc, P, C, dw, db, pre_dw, pre_db, what):
    """tap_reduce_kernel alone: dw / db against the float64 sums of the slab the first stage left (every entry written)"""
    part = sc.cpu().view(P, 10, C)
    assert not torch.isnan(part).any(), f"{what}: a slab entry was left unwritten"
    s, a = SO.tap_reduce(part)
    assert_col(dw.cpu().view(C, 9), pre_dw.view(C, 9), s[:9].t(), a[:9].t(), f"tap_reduce dw P={P} {what}")
    assert_col(db.cpu(), pre_db, s[9], a[9], f"tap_reduce db P={P} {what}")


# ------------------------------------------------------------------------------------------------ conv1
def conv1_inputs(F_, T, C, dtype, pad, B=3, len0=None, len1=None):
    """seeded operands of one conv1 problem; the mel is dense beyond len0 and dout beyond len1: only the kernels' masks zero them"""
    g = gen(F_, T, C, pad, dtype == BF16, B)
    z = dict(B=B, F=F_, T=T, C=C, dtype=dtype, pad=pad, T1=SO.half_len(T, pad), F1=SO.half_len(F_, pad))
    z["mel"] = torch.randn(B, F_, T, generator=g)
    z["w"], z["b"] = torch.randn(C, 1, 3, 3, generator=g) * 0.3, torch.randn(C, generator=g) * 0.2
    z["len0"] = torch.tensor(std_len0(T) if len0 is None else len0, dtype=I64)
    z["len1"] = torch.tensor(next_lens(z["len0"], pad) if len1 is None else len1, dtype=I64)
    z["dout"] = torch.randn(B, z["T1"], z["F1"], C, generator=g).to(dtype)
    z["pre_dw"], z["pre_db"] = torch.randn(C, 1, 3, 3, generator=g), torch.randn(C, generator=g)
    z["what"] = f"{DT[dtype]} C={C} pad={pad} F={F_} T={T} B={B} len0={z['len0'].tolist()} len1={z['len1'].tolist()}"
    return z


def run_conv1_fwd(z):
    B, T1, F1, C, dtype = z["B"], z["T1"], z["F1"], z["C"], z["dtype"]
    out = Guarded((B, T1, F1, C), dtype, fill=NAN)
    mel, w, b, l0, l1 = on_dev(z, "mel", "w", "b", "len0", "len1")
    rc = clib().mi355x_subsample_conv1_fwd_pad(ptr(mel), ptr(w), ptr(b), ptr(out), code(dtype), ptr(l0), ptr(l1), B, z["F"], z["T"], C,
                                               z["pad"], ops()._stream())
    assert rc == 0, (rc, z["what"])
    assert_intact(out1=out)
    return out


def check_conv1_fwd(z):
    _, cond, ref = SO.conv1_fwd(z["mel"], z["w"], z["b"], z["len0"], z["len1"], z["pad"])
    out = run_conv1_fwd(z)
    assert_conv(out.cpu(), ref, cond, N_FWD - 1, z["dtype"], f"conv1_fwd {z['what']}")
    dead = torch.arange(z["T1"])[None, :] >= z["len1"][:, None]
    assert_zero_where(out.t, dead[:, :, None, None], f"conv1_fwd {z['what']}: rows t1 >= len1")


def conv1_parts(z):
    return z["B"] * ((z["T1"] + 31) // 32)


def run_conv1_bwd(z, scratch):
    """scratch: the slab at exactly B * ceil(T1 / 32) * 10 * C floats, tap_reduce finishes; else float atomics into dw / db"""
    B, C, dtype = z["B"], z["C"], z["dtype"]
    dw, db = Guarded((C, 1, 3, 3), F32, src=z["pre_dw"]), Guarded(C, F32, src=z["pre_db"])
    n = conv1_parts(z) * 10 * C
    sc = Guarded(n, F32, fill=NAN) if scratch else None
    dout, mel, l0 = on_dev(z, "dout", "mel", "len0")
    rc = clib().mi355x_subsample_conv1_bwd_pad(ptr(dout), code(dtype), ptr(mel), ptr(l0), ptr(dw), ptr(db), B, z["F"], z["T"], C, z["pad"],
                                               ptr(sc), n if scratch else 0, ops()._stream())
    assert rc == 0, (rc, z["what"])
    assert_intact(dw=dw, db=db, **(dict(scratch=sc) if scratch else {}))
    return dw, db, sc


def check_conv1_bwd(z):
    rdw, rdb, adw, adb = SO.conv1_bwd(z["dout"], z["mel"], z["len0"], z["pad"])
    for scratch in (True, False):
        what = f"{z['what']} scratch={scratch}"
        dw, db, sc = run_conv1_bwd(z, scratch)
        assert_col(dw.cpu(), z["pre_dw"], rdw, adw, f"conv1_bwd dw {what}")
        assert_col(db.cpu(), z["pre_db"], rdb, adb, f"conv1_bwd db {what}")
        if scratch:
            check_slab(sc, conv1_parts(z), z["C"], dw, db, z["pre_dw"], z["pre_db"], f"conv1_bwd {z['what']}")


@pytest.mark.parametrize("dtype,C,pad", _params(CH))
def test_conv1_fwd(dtype, C, pad):
    for F_, T in GEOM:
        check_conv1_fwd(conv1_inputs(F_, T, C, dtype, pad))


@pytest.mark.parametrize("dtype,C,pad", _params(CH_BWD))
def test_conv1_bwd(dtype, C, pad):
    """each geometry twice: the slab + tap_reduce, and scratch = NULL (float atomics).  dout is dense, beyond len1 too: the
    reference masks the mel only"""
    for F_, T in GEOM:
        check_conv1_bwd(conv1_inputs(F_, T, C, dtype, pad))


LEN_CASES = [pytest.param(dt_, C, pad, id=f"{DT[dt_]}-C{C}-pad{pad}") for dt_, C in ((F32, 176), (BF16, 32)) for pad in PADS]


@pytest.mark.parametrize("dtype,C,pad", LEN_CASES)
def test_conv1_lengths(dtype, C, pad):
    """an empty utterance, a length beyond T (the kernels clamp, the reference clamps), len1 inside a 4-row block, len1 = 0 with
    a full len0, len1 beyond T1"""
    F_, T = 80, 61
    T1 = SO.half_len(T, pad)
    for len0, len1 in (([0, T], None), ([T + 5, T], None), ([T + 5, T], [T1 + 7, 0]), ([T, 41, 1], [0, 6, T1 + 3]), ([T, T, 9], [T1, 13, 1])):
        z = conv1_inputs(F_, T, C, dtype, pad, B=len(len0), len0=len0, len1=len1)
        check_conv1_fwd(z)
        check_conv1_bwd(z)


@pytest.mark.parametrize("dtype,C", [(F32, 4), (BF16, 8), (F32, 324)], ids=["f32-C4", "bf16-C8", "f32-C324"])
def test_tap_reduce_part_counts(dtype, C):
    """tap_reduce_kernel has 16 y-slices of ceil(P / 16) parts, four accumulators per slice: one part, fewer parts than slices,
    one per slice, 17 (slices 9 .. 15 empty), 67 (5 per slice: one round of four and a tail; the last slice holds 2)"""
    for P in (1, 3, 16, 17, 67):
        check_conv1_bwd(conv1_inputs(5, 6, C, dtype, 1 + P % 2, B=P, len0=[6 - (i % 3) for i in range(P)]))


# ------------------------------------------------------------------------------------------------ im2col / col2im
def col_inputs(T1, F1, C, dtype, pad, B=3):
    g = gen(T1, F1, C, pad, dtype == BF16, B, 17)
    T2, F2 = SO.half_len(T1, pad), SO.half_len(F1, pad)
    z = dict(B=B, T1=T1, F1=F1, T2=T2, F2=F2, C=C, dtype=dtype, pad=pad)
    z["act"] = post_relu((B, T1, F1, C), dtype, g)
    z["dcol"] = torch.randn(B * T2 * F2, 9 * C, generator=g).to(dtype)
    z["what"] = f"{DT[dtype]} C={C} pad={pad} T1={T1} F1={F1} B={B}"
    return z


def check_im2col(z):
    B, T1, F1, T2, F2, C, dtype = (z[n] for n in ("B", "T1", "F1", "T2", "F2", "C", "dtype"))
    col = Guarded((B * T2 * F2, 9 * C), dtype, fill=NAN)
    act, = on_dev(z, "act")
    rc = clib().mi355x_im2col_3x3s2_pad(ptr(act), ptr(col), code(dtype), B, T1, F1, C, z["pad"], ops()._stream())
    assert rc == 0, (rc, z["what"])
    assert_intact(col=col)
    want = bits(SO.im2col(z["act"], z["pad"]).to(dtype))
    same = bits(col.t) == want
    assert bool(same.all()), f"im2col {z['what']}: {int((~same).sum())} words differ, the first at (row, column) " \
                             f"{[int(v) for v in (~same).nonzero()[0]]}"


def check_col2im(z):
    B, T1, F1, C, dtype = (z[n] for n in ("B", "T1", "F1", "C", "dtype"))
    ref, cond = SO.col2im_relu(z["dcol"], z["act"], z["pad"])
    din = Guarded((B, T1, F1, C), dtype, fill=NAN)
    dcol, act = on_dev(z, "dcol", "act")
    rc = clib().mi355x_col2im_3x3s2_relu_pad(ptr(dcol), ptr(act), ptr(din), code(dtype), B, T1, F1, C, z["pad"], ops()._stream())
    assert rc == 0, (rc, z["what"])
    assert_intact(din=din)
    assert_conv(din.cpu(), ref, cond, N_DGRAD - 1, dtype, f"col2im {z['what']}")
    assert_zero_where(din.t, z["act"] <= 0, f"col2im {z['what']}: gradient where the activation is <= 0")


COL_CASES = [pytest.param(dt_, C, pad, id=f"{DT[dt_]}-C{C}-pad{pad}") for dt_ in (F32, BF16) for C in COL_CH for pad in PADS]


@pytest.mark.parametrize("dtype,C,pad", COL_CASES)
def test_im2col(dtype, C, pad):
    for T1, F1 in COL_GRIDS:
        check_im2col(col_inputs(T1, F1, C, dtype, pad))


@pytest.mark.parametrize("dtype,C,pad", COL_CASES)
def test_col2im_relu(dtype, C, pad):
    for T1, F1 in COL_GRIDS:
        check_col2im(col_inputs(T1, F1, C, dtype, pad))


BIG_COL = (1450, 1450, 8, BF16)   # 1 x 1450 x 1450 x (8 / 4) = 4 205 000 col2im vectors, 1 x 725^2 (726^2) x 9 = 4.73 M im2col vectors


@pytest.mark.parametrize("which", ["im2col-pad2", "col2im-pad1"])
def test_im2col_col2im_second_trip(which):
    """more vectors than 16384 workgroups x 256 threads (4 194 304): the grid-stride loops take a second trip"""
    T1, F1, C, dtype = BIG_COL
    if which.startswith("im2col"):
        z = col_inputs(T1, F1, C, dtype, 2, B=1)
        assert z["T2"] * z["F2"] * 9 * (C // VEC[dtype]) > 16384 * 256
        check_im2col(z)
    else:
        z = col_inputs(T1, F1, C, dtype, 1, B=1)
        assert T1 * F1 * (C // 4) > 16384 * 256
        check_col2im(z)


# ------------------------------------------------------------------------------------------------ depthwise 3x3 stride 2
def dw_inputs(T1, F1, C, dtype, pad, B=3):
    g = gen(T1, F1, C, pad, dtype == BF16, B, 29)
    T2, F2 = SO.half_len(T1, pad), SO.half_len(F1, pad)
    z = dict(B=B, T1=T1, F1=F1, T2=T2, F2=F2, C=C, dtype=dtype, pad=pad, npos=B * T2 * F2)
    z["x"] = post_relu((B, T1, F1, C), dtype, g)
    z["w"], z["b"] = torch.randn(C, 1, 3, 3, generator=g) * 0.3, torch.randn(C, generator=g) * 0.2
    z["dout"] = torch.randn(B, T2, F2, C, generator=g).to(dtype)
    z["pre_dw"], z["pre_db"] = torch.randn(C, 1, 3, 3, generator=g), torch.randn(C, generator=g)
    z["what"] = f"{DT[dtype]} C={C} pad={pad} T1={T1} F1={F1} B={B} npos={z['npos']}"
    return z


def dw_parts(npos):
    return (npos + 63) // 64 if npos < 1024 * 64 else 1024


def check_dw_fwd(z):
    B, T1, F1, T2, F2, C, dtype = (z[n] for n in ("B", "T1", "F1", "T2", "F2", "C", "dtype"))
    ref, cond = SO.dwconv2d_fwd(z["x"], z["w"], z["b"], z["pad"])
    out = Guarded((B, T2, F2, C), dtype, fill=NAN)
    x, w, b = on_dev(z, "x", "w", "b")
    rc = clib().mi355x_dwconv2d_s2_fwd_pad(ptr(x), ptr(w), ptr(b), ptr(out), code(dtype), B, T1, F1, C, z["pad"], ops()._stream())
    assert rc == 0, (rc, z["what"])
    assert_intact(out=out)
    assert_conv(out.cpu(), ref, cond, N_FWD - 1, dtype, f"dwconv2d_fwd {z['what']}")


def check_dw_bwd(z):
    B, T1, F1, C, dtype = (z[n] for n in ("B", "T1", "F1", "C", "dtype"))
    rdin, cdin, rdw, rdb, adw, adb = SO.dwconv2d_bwd(z["dout"], z["x"], z["w"], z["pad"])
    din = Guarded((B, T1, F1, C), dtype, fill=NAN)
    dw, db = Guarded((C, 1, 3, 3), F32, src=z["pre_dw"]), Guarded(C, F32, src=z["pre_db"])
    P = dw_parts(z["npos"])
    sc = Guarded(P * 10 * C, F32, fill=NAN)
    dout, x, w = on_dev(z, "dout", "x", "w")
    rc = clib().mi355x_dwconv2d_s2_bwd_pad(ptr(dout), ptr(x), ptr(w), ptr(din), ptr(dw), ptr(db), code(dtype), B, T1, F1, C, z["pad"],
                                           ptr(sc), P * 10 * C, ops()._stream())
    assert rc == 0, (rc, z["what"])
    assert_intact(din=din, dw=dw, dbias=db, scratch=sc)
    assert_conv(din.cpu(), rdin, cdin, N_DGRAD - 1, dtype, f"dwconv2d_bwd_data {z['what']}")
    assert_zero_where(din.t, z["x"] <= 0, f"dwconv2d_bwd_data {z['what']}: gradient where the activation is <= 0")
    assert_col(dw.cpu(), z["pre_dw"], rdw, adw, f"dwconv2d_bwd_w dw {z['what']}")
    assert_col(db.cpu(), z["pre_db"], rdb, adb, f"dwconv2d_bwd_w dbias {z['what']}")
    check_slab(sc, P, C, dw, db, z["pre_dw"], z["pre_db"], f"dwconv2d_bwd_w {z['what']}")


@pytest.mark.parametrize("dtype,C,pad", _params(CH))
def test_dwconv2d_fwd(dtype, C, pad):
    for T1, F1 in GRIDS:
        check_dw_fwd(dw_inputs(T1, F1, C, dtype, pad))


@pytest.mark.parametrize("dtype,C,pad", _params(CH))
def test_dwconv2d_bwd(dtype, C, pad):
    for T1, F1 in GRIDS:
        check_dw_bwd(dw_inputs(T1, F1, C, dtype, pad))


def grid_for(t2, f2, pad):
    """an input grid whose output grid is t2 x f2"""
    n1 = [(2 * v - 1 if pad == 1 else max(1, 2 * v - 2)) for v in (t2, f2)]
    assert [SO.half_len(v, pad) for v in n1] == [t2, f2]
    return n1


@pytest.mark.parametrize("dtype,C", [(BF16, 8), (F32, 176), (BF16, 328)], ids=["bf16-C8", "f32-C176", "bf16-C328"])
@pytest.mark.parametrize("pad", PADS)
def test_dwconv2d_bwd_w_few_parts(dtype, C, pad):
    """npos = 1, 63, 64 (one part), 65 (two parts, 33 + 32 positions): fewer parts than tap_reduce's 16 y-slices, position
    slots of the workgroup that see no position at all"""
    for t2, f2 in ((1, 1), (7, 9), (8, 8), (5, 13)):
        T1, F1 = grid_for(t2, f2, pad)
        z = dw_inputs(T1, F1, C, dtype, pad, B=1)
        assert z["npos"] == t2 * f2 and dw_parts(z["npos"]) == (2 if z["npos"] == 65 else 1)
        check_dw_fwd(z)
        check_dw_bwd(z)


@pytest.mark.parametrize("pad", PADS)
def test_dwconv2d_bwd_w_many_parts(pad):
    """npos = 257 x 256 = 65792 >= 65536: 1024 parts of ceil(npos / 1024) = 65 positions, so the last 11 parts hold none"""
    T1, F1 = grid_for(257, 256, pad)
    z = dw_inputs(T1, F1, 8, BF16, pad, B=1)
    assert z["npos"] == 65792 and dw_parts(z["npos"]) == 1024
    check_dw_bwd(z)


def test_dwconv2d_second_trip():
    """C = 1024 in f32: PS = 1 position per workgroup, 8192 workgroups at most; 91 x 91 = 8281 output positions give the forward's
    grid-stride loop a second trip, the 180 x 181 input positions give the input gradient's four"""
    T1, F1 = 180, 181
    z = dw_inputs(T1, F1, 1024, F32, 2, B=1)
    assert z["npos"] > 8192 and T1 * F1 > 8192
    check_dw_fwd(z)
    check_dw_bwd(z)


# ------------------------------------------------------------------------------------------------ reject paths
class Rejects:
    """one launcher, one valid argument list; every perturbed list must come back as MI_ERR_ARG before any launch: outputs keep
    their prefill bit for bit, guards intact.  The buffers are sized for the largest perturbed problem."""

    def __init__(self, fn, args, outputs):
        self.fn, self.args, self.outputs = fn, list(args), outputs
        self.before = [bits(o.t).clone() for o in outputs]

    def reject(self, why, **changes):
        a = list(self.args)
        for i, v in changes.items():
            a[int(i[1:])] = v
        assert self.fn(*a) == MI_ERR_ARG, f"{self.fn.__name__}: accepted {why}"

    def finish(self):
        torch.cuda.synchronize()
        for o, b in zip(self.outputs, self.before):
            assert o.intact() and torch.equal(bits(o.t), b), f"{self.fn.__name__}: a rejected call wrote to an output"
        assert self.fn(*self.args) == 0, f"{self.fn.__name__}: the unperturbed arguments are not accepted"
        torch.cuda.synchronize()


RJ_B, RJ_F, RJ_T, RJ_CMAX = 1, 6, 7, 2056    # extents after one stage: at most 5 x 5 with pad = 3


def _rj_buf(n, dtype, fill=None):
    g = gen(n, 3)
    return Guarded(n, dtype, fill=fill) if fill is not None else Guarded(n, dtype, src=torch.randn(n, generator=g))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_conv1_launchers_reject(dtype):
    lib, s, V = clib(), ops()._stream(), VEC[dtype]
    C = 2 * V
    mel = put(torch.randn(RJ_B, 256, RJ_T))   # (wide enough for the F = 256 case)
    w, b = put(torch.randn(RJ_CMAX, 1, 3, 3)), put(torch.randn(RJ_CMAX))
    l0, l1 = put(torch.tensor([RJ_T], dtype=I64)), put(torch.tensor([4], dtype=I64))
    out = _rj_buf(RJ_B * 5 * 5 * RJ_CMAX, dtype, fill=NAN)
    r = Rejects(lib.mi355x_subsample_conv1_fwd_pad,
                [ptr(mel), ptr(w), ptr(b), ptr(out), code(dtype), ptr(l0), ptr(l1), RJ_B, RJ_F, RJ_T, C, 1, s], [out])
    for i in (0, 1, 2, 3, 5, 6):
        r.reject(f"a null pointer (argument {i})", **{f"a{i}": 0})
    r.reject("pad = 0", a11=0)
    r.reject("pad = 3", a11=3)
    r.reject("C % V != 0", a10=C + V // 2)
    r.reject("C / V > 256", a10=257 * V)
    r.finish()
    # backward: dout is read at [B, T1, 129, Cmax] in the F = 256 case
    dout = put(torch.randn(RJ_B * 5 * 130 * RJ_CMAX).to(dtype))
    dw, db = _rj_buf(RJ_CMAX * 9, F32), _rj_buf(RJ_CMAX, F32)
    n = RJ_B * 10 * C
    sc = _rj_buf(n, F32, fill=NAN)
    r = Rejects(lib.mi355x_subsample_conv1_bwd_pad,
                [ptr(dout), code(dtype), ptr(mel), ptr(l0), ptr(dw), ptr(db), RJ_B, RJ_F, RJ_T, C, 1, ptr(sc), n, s], [dw, db, sc])
    for i in (0, 2, 3, 4, 5):
        r.reject(f"a null pointer (argument {i})", **{f"a{i}": 0})
        r.reject(f"a null pointer (argument {i}), no scratch", **{f"a{i}": 0}, a11=0, a12=0)
    r.reject("pad = 0", a10=0)
    r.reject("pad = 3", a10=3)
    r.reject("C % V != 0", a9=C + V // 2)
    r.reject("a scratch one element short", a12=n - 1)
    r.reject("F = 256: an LDS image above 64 KB", a7=256)
    r.reject("F = 256 without scratch", a7=256, a11=0, a12=0)
    r.finish()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_im2col_col2im_launchers_reject(dtype):
    lib, s = clib(), ops()._stream()
    B, T1, F1, C = 1, 6, 7, 16
    x = put(post_relu((B * (T1 + 2) * (F1 + 2) * 32,), dtype, gen(5)))
    col = _rj_buf(B * 5 * 5 * 9 * 32, dtype, fill=NAN)
    r = Rejects(lib.mi355x_im2col_3x3s2_pad, [ptr(x), ptr(col), code(dtype), B, T1, F1, C, 1, s], [col])
    r.reject("a null input", a0=0)
    r.reject("a null output", a1=0)
    r.reject("pad = 0", a7=0)
    r.reject("pad = 3", a7=3)
    r.reject("C = 12: not a multiple of 8", a6=12)
    r.finish()
    dcol = put(torch.randn(B * 5 * 5 * 9 * 32).to(dtype))
    din = _rj_buf(B * (T1 + 2) * (F1 + 2) * 32, dtype, fill=NAN)
    r = Rejects(lib.mi355x_col2im_3x3s2_relu_pad, [ptr(dcol), ptr(x), ptr(din), code(dtype), B, T1, F1, C, 1, s], [din])
    for i in (0, 1, 2):
        r.reject(f"a null pointer (argument {i})", **{f"a{i}": 0})
    r.reject("pad = 0", a8=0)
    r.reject("pad = 3", a8=3)
    r.reject("C = 6: not a multiple of 4", a7=6)
    r.finish()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_dwconv2d_launchers_reject(dtype):
    lib, s, V = clib(), ops()._stream(), VEC[dtype]
    B, T1, F1, C = 1, 6, 7, 2 * V
    CM = 257 * V
    x = put(post_relu((B * T1 * F1 * CM,), dtype, gen(6)))
    w, b = put(torch.randn(CM, 1, 3, 3)), put(torch.randn(CM))
    out = _rj_buf(B * 5 * 5 * CM, dtype, fill=NAN)
    r = Rejects(lib.mi355x_dwconv2d_s2_fwd_pad, [ptr(x), ptr(w), ptr(b), ptr(out), code(dtype), B, T1, F1, C, 1, s], [out])
    for i in (0, 1, 2, 3):
        r.reject(f"a null pointer (argument {i})", **{f"a{i}": 0})
    r.reject("pad = 0", a9=0)
    r.reject("pad = 3", a9=3)
    r.reject("C % V != 0", a8=C + V // 2)
    r.reject("C / V > 256", a8=CM)
    r.finish()
    dout = put(torch.randn(B * 5 * 5 * CM).to(dtype))
    din = _rj_buf(B * T1 * F1 * CM, dtype, fill=NAN)
    dw, db = _rj_buf(CM * 9, F32), _rj_buf(CM, F32)
    n = dw_parts(B * 3 * 4) * 10 * C
    sc = _rj_buf(10 * CM, F32, fill=NAN)   # one part at every perturbed size; the launcher is told n
    r = Rejects(lib.mi355x_dwconv2d_s2_bwd_pad,
                [ptr(dout), ptr(x), ptr(w), ptr(din), ptr(dw), ptr(db), code(dtype), B, T1, F1, C, 1, ptr(sc), n, s], [din, dw, db, sc])
    for i in (0, 1, 2, 3, 4, 5, 12):
        r.reject(f"a null pointer (argument {i})", **{f"a{i}": 0})
    r.reject("pad = 0", a11=0)
    r.reject("pad = 3", a11=3)
    r.reject("C % V != 0", a10=C + V // 2)
    r.reject("C / V > 256", a10=CM, a13=10 * CM)
    r.reject("a scratch one element short", a13=n - 1)
    r.finish()


# ------------------------------------------------------------------------------------------------ reference-error measurement
def _cols(terms, pre_dw, pre_db):
    """worst column of the ten reduced columns per channel, summed in float32 on the CPU"""
    worst = 0.0
    for k, t in enumerate(terms):
        worst = max(worst, f32_col_error(t, pre_dw.view(-1, 9)[:, k] if k < 9 else pre_db))
    return worst


def measure_reference_errors():
    """the float32 CPU figure TOL_COL is derived from (no GPU needed): every conv1_bwd and dwconv2d_bwd input of this file"""
    worst = 0.0

    def conv1(z):
        return _cols(SO.conv1_bwd_terms(z["dout"], z["mel"], z["len0"], z["pad"]), z["pre_dw"], z["pre_db"])

    def dw(z):
        return _cols(SO.dwconv2d_dw_terms(z["dout"], z["x"], z["pad"]), z["pre_dw"], z["pre_db"])

    for p in _params(CH_BWD):
        dtype, C, pad = p.values
        for F_, T in GEOM:
            worst = max(worst, conv1(conv1_inputs(F_, T, C, dtype, pad)))
    for p in LEN_CASES:
        dtype, C, pad = p.values
        T1 = SO.half_len(61, pad)
        for len0, len1 in (([0, 61], None), ([66, 61], None), ([66, 61], [T1 + 7, 0]), ([61, 41, 1], [0, 6, T1 + 3]), ([61, 61, 9], [T1, 13, 1])):
            worst = max(worst, conv1(conv1_inputs(80, 61, C, dtype, pad, B=len(len0), len0=len0, len1=len1)))
    for dtype, C in ((F32, 4), (BF16, 8), (F32, 324)):
        for P in (1, 3, 16, 17, 67):
            worst = max(worst, conv1(conv1_inputs(5, 6, C, dtype, 1 + P % 2, B=P, len0=[6 - (i % 3) for i in range(P)])))
    print(f"conv1_bwd inputs: worst column so far {worst:.3e}")
    for p in _params(CH):
        dtype, C, pad = p.values
        for T1, F1 in GRIDS:
            worst = max(worst, dw(dw_inputs(T1, F1, C, dtype, pad)))
    for pad in PADS:
        for dtype, C in ((BF16, 8), (F32, 176), (BF16, 328)):
            for t2, f2 in ((1, 1), (7, 9), (8, 8), (5, 13)):
                worst = max(worst, dw(dw_inputs(*grid_for(t2, f2, pad), C, dtype, pad, B=1)))
        worst = max(worst, dw(dw_inputs(*grid_for(257, 256, pad), 8, BF16, pad, B=1)))
    worst = max(worst, dw(dw_inputs(180, 181, 1024, F32, 2, B=1)))
    print(f"reduced columns, float32 torch.sum, worst column: {worst:.3e} -> x8 = {8 * worst:.3e}")


if __name__ == "__main__":
    measure_reference_errors()
