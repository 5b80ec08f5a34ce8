"""-m gpu: every kernel path of nemo_amd/csrc/elementwise.hip except GLU (tests/test_convmod_kernels_gpu.py sweeps it) and the
SpecAugment parameter kernel (tests/test_kernels_gpu.py compares it exactly) through the C ABI against the float64 closed forms
of tests/elementwise_oracle.py.

Operands are generated in their storage dtype and the oracle up-casts them, so a kernel is judged on its own arithmetic.  A saved
intermediate a kernel is given (`s` of the softmax backward) is an input.  Every output is a view into a buffer filled with a
sentinel word, 64 bytes of it in front of and behind the view; pitched outputs are pre-filled with NaN.  Guards and pad columns
must come back untouched.  Every test clears the device step word first, so dropout keys are used as passed.

What is asserted:
  data movement (rows_pack / rows_unpack, fill_rects, untouched and zeroed regions)   bit equality
  one float32 rounding (qbias, add2, add2_colsum's `out`, row_scale)                   out == round_out(round_f32(float64 result))
  drop_scale_cast      zero set == keep_mask(); kept values to 4 * 2^-24 relative (three float32 roundings: the host's 1 / (1 - p),
                       alpha * mask, the product), plus half a bf16 ulp of the value for a bf16 output
  add2_colsum sums     per column against the sum's conditioning, |got - ref| / (|prefill| + sum_m |term|), and whole-vector 1e-5
  rel-pos softmax      per row, max_j |got - ref| / max_j |ref| on the worst row, the tolerances of test_relpos_softmax
                       (tests/test_kernels_gpu.py): forward 1e-5 (f32) / 1e-2 (bf16), backward 3x that; all-zero rows, masked
                       entries and pad columns exactly 0; the zero set of pd_out among unmasked entries == keep_mask()

Measured bound.  Column sums of add2_colsum: the same sums taken in float32 by torch.sum on the CPU (prefill included) against
float64, worst column over A2C_CASES, and 8x that for the kernel (another order of additions, finished through a second reduction):
  measured 5.96e-08 -> bound 4.7e-07
The float32 CPU restatement of the softmax (torch.softmax / autograd in float32 on the same inputs) meets the project's bounds at
every case of this file, T = 1024 included (forward worst row 4.6e-07, backward 1.8e-07), so those stay as they are.
`python tests/test_elementwise_kernels_gpu.py` re-measures these figures on the CPU.

The case tables are module-level and need no device: tests/test_elementwise_host.py imports them to prove that they reach every
path (idle threads, RS > 32, RS = 1 and two column passes of add2_colsum; a second grid-stride trip of every grid-stride kernel).
"""
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elementwise_oracle as EO  # noqa: E402

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DT = {F32: "f32", BF16: "bf16"}
PAIRS = ((F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16))
NAN = float("nan")

TOL_DSC_F32 = 4 * 2.0 ** -24                                 # three float32 roundings; a bf16 output adds half a bf16 ulp
TOL_SM_FWD = {F32: 1e-5, BF16: 1e-2}                         # test_relpos_softmax's own
TOL_SM_BWD = {F32: 3e-5, BF16: 3e-2}
TOL_COLSUM_VEC = 1e-5                                        # test_add2_colsum's own, whole vector
TOL_COL_A2C = 4.7e-7                                         # measured, see the header
GRID_CAP = EO.GRID_CAP["elementwise"]                        # grid_for(): at most 4096 blocks of 256 threads


def ops():
    from nemo_amd import ops as _ops
    return _ops


def fresh_ops():
    """the wrappers, with the device step word cleared: keys as passed"""
    o = ops()
    o.set_step_counter(None)
    return o


# ------------------------------------------------------------------------------------------------ harness
GUARD = 64            # bytes in front of and behind every output
SENTINEL = -2 ** 31   # guard word 0x80000000


class Guarded:
    """a tensor `t` that starts GUARD + off bytes into a sentinel-filled buffer and ends GUARD bytes before its end"""

    def __init__(self, shape, dtype, off=0, fill=None, src=None):
        shape = tuple(shape) if not isinstance(shape, int) else (shape,)
        n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.words = torch.full(((self.hi + GUARD + 3) // 4,), SENTINEL, dtype=torch.int32, device=dev)
        self.t = self.words.view(torch.uint8)[self.lo:self.hi].view(dtype).view(shape)
        assert self.t.data_ptr() % 32 == off % 32
        if src is not None:
            self.t.copy_(src.to(dtype))
        elif fill is not None:
            self.t.fill_(fill)

    def intact(self):
        """the whole words outside the view still hold the sentinel (a view that ends inside a word shares it)"""
        w = self.words
        return bool((w[:self.lo // 4] == SENTINEL).all()) and bool((w[(self.hi + 3) // 4:] == SENTINEL).all())

    def untouched(self):
        """every word, the view's included, still holds the sentinel"""
        return bool((self.words == SENTINEL).all())

    def cpu(self):
        return self.t.detach().cpu()


def put(src, off=0):
    """an input on the device at the given alignment offset"""
    return Guarded(src.shape, src.dtype, off, src=src).t


def assert_intact(**bufs):
    torch.cuda.synchronize()
    for name, b in bufs.items():
        assert b.intact(), f"{name}: bytes outside the output were written"


def rel_err(a, b):
    """whole-tensor measure of tests/test_kernels_gpu.py"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def row_err(got, ref):
    """(worst row's max_j |got - ref| / max_j |ref|, that row, its worst column); a row whose reference is all zero must be
    matched exactly"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    if got.dim() == 1:
        got, ref = got[None], ref[None]
    err = (got - ref).abs()
    den = ref.abs().amax(1)
    e = err.amax(1)
    rel = torch.where(den > 0, e / den, torch.where(e == 0, 0.0, float("inf")))
    rel = torch.where(torch.isnan(e), float("inf"), rel)
    r = int(rel.argmax())
    return rel[r].item(), r, int(err[r].nan_to_num(float("inf")).argmax())


def assert_rows(got, ref, tol, what):
    e, r, c = row_err(got, ref)
    print(f"{what}: worst row error {e:.3e} (row {r}, column {c}; bound {tol:.1e})")
    assert e < tol, f"{what}: row {r} is off by {e:.3e} of its largest entry (bound {tol:.1e}), worst at column {c}"


def col_err(got, prefill, ref_sum, abs_sum):
    """(worst column's |got - (prefill + ref_sum)| / (|prefill| + sum_m |term|), that column)"""
    got, prefill = got.detach().double().cpu(), prefill.detach().double().cpu()
    e = (got - (prefill + ref_sum)).abs() / (prefill.abs() + abs_sum)
    e = torch.where(torch.isnan(e), float("inf"), e)
    c = int(e.argmax())
    return e[c].item(), c


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, f"{what}: shape {tuple(g.shape)} != {tuple(w.shape)}"
    bad = g != w
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at flat index " \
                                f"{int(bad.flatten().nonzero()[0])}"


def all_nan(t):
    return bool(torch.isnan(t.detach().float()).all())


def nonzero_randn(shape, g, dtype=F32, scale=1.0):
    """sign * U(0.5, 2) * scale: no zeros, in any storage dtype"""
    sign = torch.randint(0, 2, shape, generator=g).to(F32) * 2 - 1
    return (sign * (0.5 + 1.5 * torch.rand(shape, generator=g)) * scale).to(dtype)


def up64(n):
    return (n + 63) // 64 * 64


# ------------------------------------------------------------------------------------------------ drop_scale_cast
DSC_BIG = 8 * (GRID_CAP * 256 + 3)      # a second grid-stride trip
DSC_ALPHA_P = [(a, p) for a in (1.0, 0.5, 22.6) for p in (0.0, 0.1, 0.5)]
DSC_CASES = [(i, o_, n, DSC_ALPHA_P) for i, o_ in PAIRS for n in (8, 8 * 257)]
DSC_CASES += [(F32, BF16, DSC_BIG, [(22.6, 0.1)]), (BF16, F32, DSC_BIG, [(0.5, 0.5)])]


@functools.lru_cache(maxsize=None)
def dsc_input(n, idt):
    return nonzero_randn((n,), torch.Generator().manual_seed(n % 100003 + 17), idt)


def check_dsc(got, x, alpha, p, keep, odt, tag):
    """the zero set is the mask's; returns the worst kept value's |got - ref| / bound, bound = 4 * 2^-24 * |ref| and, for a bf16
    output, half a bf16 ulp of the float32 result more (8 significant bits: 2^(e - 8) for a value in [2^e, 2^(e + 1)), between
    2^-9 and 2^-8 of the value)"""
    got = got.double()
    assert torch.equal(got != 0, keep), f"{tag}: {int(((got != 0) != keep).sum())} elements are not masked as drop_mask() defines"
    ref = EO.drop_scale_cast(x, EO.f32(alpha), keep, p).abs()
    bound = TOL_DSC_F32 * ref
    if odt == BF16:
        bound = bound + 2.0 ** (torch.floor(torch.log2((ref * (1 + TOL_DSC_F32)).clamp_min(1e-300))) - 8)
    e = ((got.abs() - ref).abs() / bound)[keep]
    return e.max().item() if e.numel() else 0.0


@pytest.mark.parametrize("idt,odt,n,alpha_p", DSC_CASES, ids=[f"{DT[c[0]]}-{DT[c[1]]}-n{c[2]}" for c in DSC_CASES])
def test_drop_scale_cast(idt, odt, n, alpha_p):
    o = fresh_ops()
    x = dsc_input(n, idt)
    assert bool((x.float() != 0).all())
    xd = put(x)
    for alpha, p in alpha_p:
        tag = f"n={n} alpha={alpha} p={p}"
        drop = o.Dropout(p, 7, 21)
        out = Guarded(n, odt, fill=NAN)
        o.drop_scale_cast(xd, out.t, n, alpha, drop)
        assert_intact(out=out)
        keep = EO.keep_mask(drop, 0, n)
        if p > 0 and n > 1000:
            assert abs(1 - keep.float().mean().item() - p) < 0.05
        assert bool(((out.cpu().double() == 0) | (out.cpu().double().sign() == x.double().sign())).all()), f"{tag}: a sign flipped"
        worst = check_dsc(out.cpu(), x, alpha, p, keep, odt, tag)
        print(f"drop_scale_cast {tag}: worst kept value at {worst:.3f} of its bound")
        assert worst <= 1.0, f"{tag}: a kept value is off by {worst:.3f} times its bound"


def test_drop_scale_cast_adds_the_registered_step_word_to_its_key():
    o = fresh_ops()
    n, p, w = 8 * 257, 0.5, 0x1234ABCD
    x = dsc_input(n, F32)
    drop = o.Dropout(p, 7, 21)
    word = torch.tensor([w], dtype=torch.int32, device=dev)
    out = Guarded(n, F32, fill=NAN)
    try:
        o.set_step_counter(word)
        o.drop_scale_cast(put(x), out.t, n, 1.0, drop)
        assert_intact(out=out)
    finally:
        o.set_step_counter(None)
    with_word, without = EO.keep_mask(drop, 0, n, step_word=w), EO.keep_mask(drop, 0, n)
    assert not torch.equal(with_word, without)
    assert torch.equal(out.cpu() != 0, with_word), "not the mask of key + step word"


# ------------------------------------------------------------------------------------------------ rows_pack / rows_unpack
ROWS_LENS, ROWS_T = (19, 0, 7, 1), 19
ROWS_BIG_T = 29200                       # f32 width 36: 4 * 29200 * 9 vectors > 4096 * 256
ROWS_CASES = [(dt_, w, ROWS_T, ROWS_LENS) for dt_, ws in ((F32, (4, 36)), (BF16, (8, 40))) for w in ws]
ROWS_CASES += [(F32, 36, ROWS_BIG_T, (ROWS_BIG_T, 0, 7, ROWS_BIG_T - 1))]


def rows_vec(dtype):
    return 4 if dtype == F32 else 8


@pytest.mark.parametrize("dtype,width,T,lens", ROWS_CASES, ids=[f"{DT[c[0]]}-w{c[1]}-T{c[2]}" for c in ROWS_CASES])
def test_rows_pack_and_unpack(dtype, width, T, lens):
    o = fresh_ops()
    B, V = len(lens), rows_vec(dtype)
    M, cu = B * T, EO.row_offsets(lens, T)
    N = cu[-1]
    lens_d, cu_d = torch.tensor(lens, dtype=torch.int64, device=dev), torch.tensor(cu, dtype=torch.int64, device=dev)
    g = torch.Generator().manual_seed(31 * width + T)
    pitches = ((width, width),) if T == ROWS_BIG_T else ((width, width), (width + V, width), (width, width + V), (width + V, width + V))
    for ld_src, ld_dst in pitches:
        tag = f"width={width} ld_src={ld_src} ld_dst={ld_dst}"
        x = torch.randn(M, ld_src, generator=g).to(dtype)            # what lies between the rows is data too
        packed = Guarded((N, ld_dst), dtype, fill=NAN)
        o.rows_pack(put(x), packed.t, lens_d, cu_d, T, M, width, ld_src=ld_src, ld_dst=ld_dst)
        assert_intact(packed=packed)
        got = packed.cpu()
        assert_bits(got[:, :width], EO.rows_pack(x, lens, T, width), f"rows_pack {tag}")
        assert all_nan(got[:, width:]), f"rows_pack {tag}: pad columns were written"

        y = torch.randn(N, ld_src, generator=g).to(dtype)
        padded = Guarded((M, ld_dst), dtype, fill=NAN)
        o.rows_unpack(put(y), padded.t, lens_d, cu_d, T, M, width, ld_src=ld_src, ld_dst=ld_dst)
        assert_intact(padded=padded)
        got = padded.cpu()
        assert_bits(got[:, :width], EO.rows_unpack(y, lens, T, width), f"rows_unpack {tag}")
        assert all_nan(got[:, width:]), f"rows_unpack {tag}: pad columns were written"

        # round trip through the kernels' own packed rows: x on the valid rows, zero beyond
        back = Guarded((M, width), dtype, fill=NAN)
        o.rows_unpack(packed.t, back.t, lens_d, cu_d, T, M, width, ld_src=ld_dst, ld_dst=width)
        assert_intact(back=back)
        valid = (torch.arange(T)[None] < torch.tensor(lens)[:, None]).reshape(-1, 1)
        assert_bits(back.cpu(), torch.where(valid, x[:, :width], torch.zeros((), dtype=dtype)), f"round trip {tag}")


# ------------------------------------------------------------------------------------------------ qbias
QB_BIG_M = 8200                          # d = 512: 8200 * 128 vectors > 4096 * 256
QB_CASES = [(dt_, d, ldm) for dt_ in (F32, BF16) for d in (4, 36, 512) for ldm in (1, 3)]


def run_qbias(o, dtype, M, d, ldq):
    g = torch.Generator().manual_seed(1000 * d + M)
    qkv = torch.randn(M, ldq, generator=g).to(dtype)
    u, v = torch.randn(d, generator=g), torch.randn(d, generator=g)
    qu, qv = Guarded((M, d), dtype, fill=NAN), Guarded((M, d), dtype, fill=NAN)
    o.qbias(put(qkv), ldq, put(u), put(v), qu.t, qv.t, M, d)
    assert_intact(qu=qu, qv=qv)
    tag = f"{DT[dtype]} M={M} d={d} ldq={ldq}"
    assert_bits(qu.cpu(), EO.round_to(EO.add(qkv[:, :d], u), dtype), f"qu {tag}")
    assert_bits(qv.cpu(), EO.round_to(EO.add(qkv[:, :d], v), dtype), f"qv {tag}")


@pytest.mark.parametrize("dtype,d,ldm", QB_CASES, ids=[f"{DT[c[0]]}-d{c[1]}-ldq{c[2]}d" for c in QB_CASES])
def test_qbias(dtype, d, ldm):
    o = fresh_ops()
    for M in (1, 67):
        run_qbias(o, dtype, M, d, ldm * d)


def test_qbias_second_grid_stride_trip():
    run_qbias(fresh_ops(), BF16, QB_BIG_M, 512, 3 * 512)


# ------------------------------------------------------------------------------------------------ add2
ADD2_BIG_M = 116600                      # d = 36: 116600 * 9 vectors > 4096 * 256
ADD2_CASES = [(i, o_, d, ldm) for i, o_ in PAIRS for d in (4, 36) for ldm in (1, 3)]


def run_add2(o, idt, odt, M, d, ldo, out_off):
    g = torch.Generator().manual_seed(2000 * d + M)
    a, b = torch.randn(M, d, generator=g).to(idt), torch.randn(M, d, generator=g).to(idt)
    out = Guarded((M, ldo), odt, fill=NAN)
    o.add2(put(a), put(b), out.t, ldo, M, d, out_off=out_off)
    assert_intact(out=out)
    got = out.cpu()
    tag = f"add2 {DT[idt]}->{DT[odt]} M={M} d={d} ldo={ldo} out_off={out_off}"
    assert_bits(got[:, out_off:out_off + d], EO.round_to(EO.add(a, b), odt), tag)
    assert all_nan(got[:, :out_off]) and all_nan(got[:, out_off + d:]), f"{tag}: columns outside [out_off, out_off + d) were written"


@pytest.mark.parametrize("idt,odt,d,ldm", ADD2_CASES, ids=[f"{DT[c[0]]}-{DT[c[1]]}-d{c[2]}-ldo{c[3]}d" for c in ADD2_CASES])
def test_add2(idt, odt, d, ldm):
    o = fresh_ops()
    for M in (1, 67):
        for out_off in ((0,) if ldm == 1 else (0, d, 2 * d)):
            run_add2(o, idt, odt, M, d, ldm * d, out_off)


def test_add2_second_grid_stride_trip():
    run_add2(fresh_ops(), F32, BF16, ADD2_BIG_M, 36, 36, 0)


# ------------------------------------------------------------------------------------------------ add2_colsum
A2C_CASES = [(8, 1003, 1), (8, 1, 3), (24, 33, 3), (24, 31, 1), (176, 1003, 3), (176, 32, 1), (512, 33, 1), (512, 1, 3),
             (2048, 33, 3), (2048, 1003, 1), (2056, 33, 1), (2056, 1, 3)]   # (d, M, ldo / d)


@functools.lru_cache(maxsize=None)
def a2c_case(d, M):
    g = torch.Generator().manual_seed(3000 + 7 * d + M)
    a, b = torch.randn(M, d, generator=g).to(BF16), torch.randn(M, d, generator=g).to(BF16)
    return dict(a=a, b=b, pre=torch.randn(2 * d, generator=g),
                sum=torch.cat([a.double().sum(0), b.double().sum(0)]), abs=torch.cat([a.double().abs().sum(0), b.double().abs().sum(0)]))


@pytest.mark.parametrize("d,M,ldm", A2C_CASES, ids=[f"d{c[0]}-M{c[1]}-ldo{c[2]}d" for c in A2C_CASES])
def test_add2_colsum(d, M, ldm):
    o = fresh_ops()
    z, ldo = a2c_case(d, M), ldm * d
    out = Guarded((M, ldo), BF16, fill=NAN)
    sums = Guarded(2 * d, F32, src=z["pre"])            # non-zero: the kernel accumulates
    o.add2_colsum(put(z["a"]), put(z["b"]), out.t, ldo, M, d, sums.t)
    assert_intact(out=out, sum_ab=sums)
    got = out.cpu()
    assert_bits(got[:, :d], EO.round_to(EO.add(z["a"], z["b"]), BF16), f"out d={d} M={M}")
    assert all_nan(got[:, d:]), f"d={d} M={M}: columns [d, ldo) of out were written"
    e, c = col_err(sums.cpu(), z["pre"], z["sum"], z["abs"])
    print(f"add2_colsum d={d} M={M}: worst column error {e:.3e} of its conditioning (column {c}; bound {TOL_COL_A2C:.1e})")
    assert e < TOL_COL_A2C, f"d={d} M={M}: sum {c} ({'a' if c < d else 'b'}, column {c % d}) is off by {e:.3e} of its sum of magnitudes"
    ref = z["pre"].double() + z["sum"]
    assert rel_err(sums.cpu()[:d], ref[:d]) < TOL_COLSUM_VEC and rel_err(sums.cpu()[d:], ref[d:]) < TOL_COLSUM_VEC


# ------------------------------------------------------------------------------------------------ rel-pos softmax
def sm_lens(T, B):
    """lengths T, 0, > T and 1 among the utterances, as far as B allows; the single utterance of T = 1024 ends 24 frames early"""
    return (T - 24,) if B == 1 else (T, 0, T + 5, 1)[:B]


def sm_bwd_dtypes(T, k):
    """(s, dpd) dtype pairs: all four at T = 45 / 65, both pure ones at T = 1024, alternating elsewhere"""
    pure = ((F32, F32), (BF16, BF16))
    return PAIRS if T in (45, 65) else pure if T == 1024 else pure[k:k + 1]


SM_T = (1, 45, 63, 64, 65, 129, 1024)
SM_CTX = [(1, 4, 0), (1, -1, 2), (1, 3, -1), (1, 0, 0), (2, 8, 3), (2, -1, 3), (2, 6, -1), (2, 7, 3)]
# (H, B, T, Tp, Pp, out dtype, ctx)
SM_FWD_CASES = []
for _T in SM_T:
    _H, _B = (1, 1) if _T == 1024 else ((1, 3) if _T in (1, 63) else (2, 4))     # H * B * T = 3 and 189: not a multiple of 4
    for _k, (_Tp, _Pp) in enumerate(((_T, 2 * _T - 1), (up64(_T), 2 * _T + 6))):
        for _odt in (F32, BF16):
            SM_FWD_CASES.append((_H, _B, _T, _Tp, _Pp, _odt, (0, -1, -1)))
for _k, _ctx in enumerate(SM_CTX):
    SM_FWD_CASES.append((2, 4, 45, 64, 96, F32, _ctx))
    if _k in (0, 4):
        SM_FWD_CASES.append((2, 4, 45, 45, 89, BF16, _ctx))
# (H, B, T, Tp, Pp, s dtype, dpd dtype)
SM_BWD_CASES = []
for _T in SM_T:
    _H, _B = (1, 1) if _T == 1024 else ((1, 3) if _T in (1, 63) else (2, 4))
    for _k, (_Tp, _Pp) in enumerate(((_T, 2 * _T - 1), (up64(_T), 2 * _T + 6))):
        for _sdt, _ddt in sm_bwd_dtypes(_T, _k):
            SM_BWD_CASES.append((_H, _B, _T, _Tp, _Pp, _sdt, _ddt))
SM_SCALE, SM_P = 0.3, 0.2
NO_CTX = (0, -1, -1)


def sm_id(c):
    return "-".join(f"{k}{v}" if not isinstance(v, (torch.dtype, tuple)) else (DT[v] if isinstance(v, torch.dtype) else "ctx" + "_".join(map(str, v)))
                    for k, v in zip(("H", "B", "T", "Tp", "Pp", "", ""), c))


@functools.lru_cache(maxsize=None)
def sm_case(H, B, T, Tp, Pp, ctx):
    """inputs of one problem (pad columns of ac and the columns of bdf beyond 2T - 1 hold NaN: the kernels must not use them)
    and the float64 forward"""
    g = torch.Generator().manual_seed(10000 * T + 10 * Tp + H + B)
    ac = torch.full((H, B, T, Tp), NAN); ac[..., :T] = 2 * torch.randn(H, B, T, T, generator=g)
    bdf = torch.full((H, B, T, Pp), NAN); bdf[..., :2 * T - 1] = 2 * torch.randn(H, B, T, 2 * T - 1, generator=g)
    dpd = torch.full((H, B, T, Tp), NAN); dpd[..., :T] = torch.randn(H, B, T, T, generator=g)
    lens = sm_lens(T, B)
    return dict(ac=ac, bdf=bdf, dpd=dpd, lens=lens, ok=EO.relpos_allowed(lens, B, T, ctx)[None].expand(H, B, T, T),
                s=EO.relpos_softmax_fwd(ac, bdf, lens, T, SM_SCALE, ctx))


def sm_keep(drop, H, B, T, Tp):
    """mask index = row * Tp + j"""
    return EO.keep_mask(drop, 0, H * B * T * Tp).view(H, B, T, Tp)[..., :T]


@pytest.mark.parametrize("H,B,T,Tp,Pp,odt,ctx", SM_FWD_CASES, ids=[sm_id(c) for c in SM_FWD_CASES])
def test_relpos_softmax_fwd(H, B, T, Tp, Pp, odt, ctx):
    o = fresh_ops()
    z = sm_case(H, B, T, Tp, Pp, ctx)
    rows = H * B * T
    ac_d, bdf_d, lens_d = put(z["ac"]), put(z["bdf"]), torch.tensor(z["lens"], dtype=torch.int64, device=dev)
    s = Guarded((H, B, T, Tp), odt, fill=NAN)
    o.relpos_softmax_fwd(ac_d, bdf_d, s.t, None, lens_d, H, B, T, Tp, Pp, SM_SCALE, ctx=ctx)
    assert_intact(s=s)
    got = s.cpu().float()
    assert bool((got[..., T:] == 0).all()), "pad columns of s are not zero"
    assert bool((got[..., :T][~z["ok"]] == 0).all()), "a masked entry (length or context) is not exactly zero"
    assert_rows(got[..., :T].reshape(rows, T), z["s"].reshape(rows, T), TOL_SM_FWD[odt], f"s T={T} Tp={Tp} ctx={ctx}")
    assert bool((got[..., :T][z["ok"]] > 0).all()), "an unmasked probability underflowed: the dropout zero set could not be read"

    drop = o.Dropout(SM_P, 3, 5)
    s2, pd = Guarded((H, B, T, Tp), odt, fill=NAN), Guarded((H, B, T, Tp), odt, fill=NAN)
    o.relpos_softmax_fwd(ac_d, bdf_d, s2.t, pd.t, lens_d, H, B, T, Tp, Pp, SM_SCALE, drop=drop, ctx=ctx)
    assert_intact(s=s2, pd=pd)
    assert_bits(s2.t, s.t, "s with pd_out given")
    gpd = pd.cpu().float()
    keep = sm_keep(drop, H, B, T, Tp)
    assert bool((gpd[..., T:] == 0).all()), "pad columns of pd are not zero"
    assert bool((gpd[..., :T][~z["ok"]] == 0).all())
    assert torch.equal((gpd[..., :T] != 0)[z["ok"]], keep[z["ok"]]), "pd_out is not masked as drop_mask(row * Tp + j) defines"
    assert_rows(gpd[..., :T].reshape(rows, T), (z["s"] * keep / (1 - SM_P)).reshape(rows, T), TOL_SM_FWD[odt], f"pd T={T} Tp={Tp}")


@pytest.mark.parametrize("H,B,T,Tp,Pp,sdt,ddt", SM_BWD_CASES, ids=[sm_id(c) for c in SM_BWD_CASES])
def test_relpos_softmax_bwd(H, B, T, Tp, Pp, sdt, ddt):
    o = fresh_ops()
    z = sm_case(H, B, T, Tp, Pp, NO_CTX)
    rows = H * B * T
    s_in = torch.full((H, B, T, Tp), NAN, dtype=sdt); s_in[..., :T] = z["s"].to(sdt)      # the oracle's forward, rounded: an input
    dpd = z["dpd"].to(ddt)
    s_d, dpd_d = put(s_in), put(dpd)
    band = torch.zeros(T, Pp, dtype=torch.bool)
    for i in range(T):
        band[i, T - 1 - i:2 * T - 1 - i] = True
    for p in (0.0, SM_P):
        drop = o.Dropout(p, 3, 5)
        keep = sm_keep(drop, H, B, T, Tp) if p > 0 else None
        ds_ref, dbdf_ref = EO.relpos_softmax_bwd(dpd, s_in, T, Pp, SM_SCALE, keep, p)
        dscore, dbdf = Guarded((H, B, T, Tp), sdt, fill=NAN), Guarded((H, B, T, Pp), sdt, fill=NAN)
        o.relpos_softmax_bwd(dpd_d, s_d, dscore.t, dbdf.t, H, B, T, Tp, Pp, SM_SCALE, drop=drop)
        assert_intact(dscore=dscore, dbdf=dbdf)
        gs, gb = dscore.cpu().float(), dbdf.cpu().float()
        tag = f"T={T} Tp={Tp} Pp={Pp} p={p}"
        assert bool((gs[..., T:] == 0).all()), f"{tag}: pad columns of dscore are not zero"
        assert bool((gb[:, :, ~band] == 0).all()), f"{tag}: dbdf outside [T-1-i, 2T-2-i] is not zero"
        assert_rows(gs[..., :T].reshape(rows, T), ds_ref.reshape(rows, T), TOL_SM_BWD[sdt], f"dscore {tag}")
        assert_rows(gb.reshape(rows, Pp), dbdf_ref.reshape(rows, Pp), TOL_SM_BWD[sdt], f"dbdf {tag}")


# ------------------------------------------------------------------------------------------------ row_scale
RS_BIG = (5, 209720)                     # 5 * 209720 elements > 4096 * 256
RS_CASES = [(r, c) for r in (1, 5) for c in (1, 300)] + [RS_BIG]


@pytest.mark.parametrize("rows,cols", RS_CASES, ids=[f"{r}x{c}" for r, c in RS_CASES])
def test_row_scale(rows, cols):
    o = fresh_ops()
    g = torch.Generator().manual_seed(rows * 1000 + cols % 1000)
    x0, vec = torch.randn(rows, cols, generator=g), torch.randn(rows, generator=g)
    x = Guarded((rows, cols), F32, src=x0)
    o.row_scale(x.t, put(vec), rows, cols)
    assert_intact(x=x)
    assert_bits(x.cpu(), (x0.double() * vec.double()[:, None]).float(), f"row_scale {rows}x{cols}")   # one float32 multiply


# ------------------------------------------------------------------------------------------------ fill_rects
def rects_for(B, F, T):
    """(b, f0, f1, t0, t1): empty ones, one clipped on each side, b out of range, overlapping ones, the whole of one row"""
    return [(0, 1, 1, 0, T), (0, 3, 2, 0, T), (1, 0, F, 4, 4), (1, 0, F, 5, 3),              # empty
            (0, -3, 2, 1, 3), (0, F - 2, F + 9, 0, 2), (1, 1, 3, -5, 2), (1, 2, 4, T - 3, T + 70),   # clipped
            (-1, 0, F, 0, T), (B, 0, F, 0, T), (B + 7, 1, 2, 1, 2),                               # b out of range
            (1, F // 2, F, 2, T - 1), (1, F // 2 - 1, F - 1, 1, T - 2), (0, 0, F, T // 2, T // 2 + 1),   # overlapping, every row
            (0, F - 1, F, 0, T)]


@pytest.mark.parametrize("F,T", [(5, 7), (80, 7), (5, 600), (80, 600)], ids=lambda v: str(v))   # 80 > 64 row-blocks, 600 > 256 threads
def test_fill_rects(F, T):
    o = fresh_ops()
    B = 2
    x0 = torch.randn(B, F, T, generator=torch.Generator().manual_seed(F * T))
    rects = rects_for(B, F, T)
    rd = torch.tensor(rects, dtype=torch.int32, device=dev)
    for value in (-0.0, 1.5):
        x = Guarded((B, F, T), F32, src=x0)
        o.fill_rects(x.t, rd, value)
        assert_intact(x=x)
        want = EO.fill_rects(x0, rects, value)
        assert not torch.equal(bits(want), bits(x0))
        assert_bits(x.cpu(), want, f"fill_rects F={F} T={T} value={value}")      # outside the rectangles: bit-identical to before
    x = Guarded((B, F, T), F32, src=x0)
    o.fill_rects(x.t, rd[:0], 0.0)
    assert_intact(x=x)
    assert_bits(x.cpu(), x0, "no rectangles")


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_return_before_any_launch():
    """MI_ERR_ARG (1) for every condition the launchers test, and nothing written: every pointer is the same sentinel-filled
    buffer, which must come back whole"""
    from nemo_amd import _lib
    L = _lib.lib
    fresh_ops()
    buf = Guarded(4096, torch.uint8)
    p = buf.t.data_ptr()
    assert p % 16 == 0
    rc = {
        "drop_scale_cast n % 8": L.mi355x_drop_scale_cast(p, 0, p, 1, 12, 1.0, 0, 0, 1.0, None),
        "drop_scale_cast n = 0": L.mi355x_drop_scale_cast(p, 0, p, 1, 0, 1.0, 0, 0, 1.0, None),
        "qbias d % 4": L.mi355x_qbias(p, 8, p, p, p, p, 0, 2, 6, None),
        "qbias ldq % 4": L.mi355x_qbias(p, 10, p, p, p, p, 0, 2, 8, None),
        "add2 d % 4": L.mi355x_add2(p, p, 0, p, 0, 8, 2, 6, None),
        "add2 ldo % 4": L.mi355x_add2(p, p, 0, p, 0, 10, 2, 8, None),
        "add2_colsum d % 8": L.mi355x_add2_colsum(p, p, p, 16, 2, 12, p, p, 1 << 20, None),
        "add2_colsum ldo % 8": L.mi355x_add2_colsum(p, p, p, 20, 2, 16, p, p, 1 << 20, None),
        "add2_colsum scratch too small": L.mi355x_add2_colsum(p, p, p, 16, 33, 16, p, p, 2 * 2 * 16 - 1, None),
        "rows_pack width % V (f32)": L.mi355x_rows_pack(p, p, 0, 8, 8, p, p, 4, 8, 6, 0, None),
        "rows_pack width % V (bf16)": L.mi355x_rows_pack(p, p, 1, 16, 16, p, p, 4, 8, 12, 0, None),
        "rows_pack ld_src % V": L.mi355x_rows_pack(p, p, 0, 10, 8, p, p, 4, 8, 8, 0, None),
        "rows_pack ld_dst % V": L.mi355x_rows_pack(p, p, 0, 8, 10, p, p, 4, 8, 8, 1, None),
        "rows_pack misaligned src": L.mi355x_rows_pack(p + 4, p, 0, 8, 8, p, p, 4, 8, 8, 0, None),
        "rows_pack misaligned dst": L.mi355x_rows_pack(p, p + 8, 0, 8, 8, p, p, 4, 8, 8, 1, None),
        "rows_pack direction 2": L.mi355x_rows_pack(p, p, 0, 8, 8, p, p, 4, 8, 8, 2, None),
        "softmax fwd T > 1024": L.mi355x_relpos_softmax_fwd_ctx(p, p, p, None, 0, p, 1, 1, 1025, 1025, 2049, 1.0, 0, 0, 1.0, 0, -1, -1, None),
        "softmax fwd Tp > 1024": L.mi355x_relpos_softmax_fwd_ctx(p, p, p, None, 0, p, 1, 1, 8, 1088, 15, 1.0, 0, 0, 1.0, 0, -1, -1, None),
        "softmax fwd Tp < T": L.mi355x_relpos_softmax_fwd_ctx(p, p, p, None, 0, p, 1, 1, 8, 7, 15, 1.0, 0, 0, 1.0, 0, -1, -1, None),
        "softmax fwd Pp < 2T - 1": L.mi355x_relpos_softmax_fwd_ctx(p, p, p, None, 0, p, 1, 1, 8, 8, 14, 1.0, 0, 0, 1.0, 0, -1, -1, None),
        "softmax fwd ctx_style 3": L.mi355x_relpos_softmax_fwd_ctx(p, p, p, None, 0, p, 1, 1, 8, 8, 15, 1.0, 0, 0, 1.0, 3, -1, -1, None),
        "softmax fwd left < -1": L.mi355x_relpos_softmax_fwd_ctx(p, p, p, None, 0, p, 1, 1, 8, 8, 15, 1.0, 0, 0, 1.0, 1, -2, 0, None),
        "softmax fwd right < -1": L.mi355x_relpos_softmax_fwd_ctx(p, p, p, None, 0, p, 1, 1, 8, 8, 15, 1.0, 0, 0, 1.0, 1, 0, -2, None),
        "softmax fwd T = 0": L.mi355x_relpos_softmax_fwd(p, p, p, None, 0, p, 1, 1, 0, 8, 15, 1.0, 0, 0, 1.0, None),
        "softmax bwd T > 1024": L.mi355x_relpos_softmax_bwd(p, 0, p, p, p, 0, 1, 1, 1025, 1025, 2049, 1.0, 0, 0, 1.0, None),
        "softmax bwd Tp < T": L.mi355x_relpos_softmax_bwd(p, 0, p, p, p, 0, 1, 1, 8, 7, 15, 1.0, 0, 0, 1.0, None),
        "softmax bwd Pp < 2T - 1": L.mi355x_relpos_softmax_bwd(p, 0, p, p, p, 0, 1, 1, 8, 8, 14, 1.0, 0, 0, 1.0, None),
        "row_scale rows = 0": L.mi355x_row_scale(p, p, 0, 4, None),
        "fill_rects F = 0": L.mi355x_fill_rects(p, p, 1, 1, 0, 4, 0.0, None),
        "fill_rects n > 0 without rects": L.mi355x_fill_rects(p, None, 1, 1, 4, 4, 0.0, None),
    }
    torch.cuda.synchronize()
    assert all(v == 1 for v in rc.values()), {k: v for k, v in rc.items() if v != 1}
    assert buf.untouched(), "an argument error was returned after something had been written"
    with pytest.raises(ValueError):
        _lib.check(rc["qbias d % 4"], "qbias")


# ------------------------------------------------------------------------------------------------ what the host test reads
def grid_stride_vectors():
    """kernel -> items (one per thread and trip) of its largest case in this file; grid_for() caps the grid at 4096 blocks"""
    return {
        "drop_scale_cast": max(c[2] for c in DSC_CASES) // 8,
        "rows_pack": max(len(c[3]) * c[2] * (c[1] // rows_vec(c[0])) for c in ROWS_CASES),
        "qbias": QB_BIG_M * 512 // 4,
        "add2": ADD2_BIG_M * 36 // 4,
        "row_scale": max(r * c for r, c in RS_CASES),
    }


# ------------------------------------------------------------------------------------------------ reference-error measurement
def measure_reference_errors():
    """the float32 CPU figures the header quotes (no GPU needed)"""
    worst = 0.0
    for d, M, _ in A2C_CASES:
        z = a2c_case(d, M)
        s32 = z["pre"] + torch.cat([torch.sum(z["a"].float(), 0), torch.sum(z["b"].float(), 0)])
        worst = max(worst, col_err(s32, z["pre"], z["sum"], z["abs"])[0])
    print(f"add2_colsum, float32 torch.sum, worst column: {worst:.3e} -> x8 = {8 * worst:.3e}")
    wf = wb = 0.0
    for H, B, T, Tp, Pp, _, _ in SM_BWD_CASES:
        z = sm_case(H, B, T, Tp, Pp, NO_CTX)
        rows = H * B * T
        ac = z["ac"][..., :T].clone().requires_grad_(True)
        bdf = z["bdf"][..., :2 * T - 1].clone().requires_grad_(True)
        i, j = torch.arange(T)[:, None], torch.arange(T)[None]
        sc = (ac + bdf[..., i, T - 1 + j - i]) * SM_SCALE
        s = torch.softmax(sc.masked_fill(~z["ok"], -10000.0), -1).masked_fill(~z["ok"], 0.0)
        wf = max(wf, row_err(s.detach().reshape(rows, T), z["s"].reshape(rows, T))[0])
        (s * z["dpd"][..., :T]).sum().backward()
        ds_ref, dbdf_ref = EO.relpos_softmax_bwd(z["dpd"], s.detach(), T, 2 * T - 1, SM_SCALE)
        wb = max(wb, row_err(ac.grad.reshape(rows, T), ds_ref.reshape(rows, T))[0],
                 row_err(bdf.grad.reshape(rows, 2 * T - 1), dbdf_ref.reshape(rows, 2 * T - 1))[0])
    print(f"rel-pos softmax, float32 torch on the CPU, worst row: forward {wf:.3e} (bound {TOL_SM_FWD[F32]:.0e}), "
          f"backward {wb:.3e} (bound {TOL_SM_BWD[F32]:.0e})")


if __name__ == "__main__":
    measure_reference_errors()
