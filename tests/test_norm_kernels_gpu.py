"""-m gpu: every kernel path of nemo_amd/csrc/norm.hip (LayerNorm forward / backward, log-softmax, column sums) through the C ABI
against the float64 closed forms of tests/norm_oracle.py.

Operands are generated in their storage dtype and the oracle up-casts them, so a kernel is judged on its own arithmetic.
Every output is a view into a buffer filled with a sentinel word, 64 bytes of it in front of and behind the view: the guards
must come back untouched (writes past row M or column d), and starting the view 16 bytes later breaks the 32-byte alignment
the launchers test for, which is how the generic kernels are reached at d = 512 / 1024 / 2048.

Error measures: matrices per ROW, max_j |got - ref| / max_j |ref|, asserted on the worst row; column sums (dgamma, dbeta,
colsum) per COLUMN against the sum's conditioning, |got - ref| / (|prefill| + sum_m |term|), next to the whole-vector measure
of tests/test_kernels_gpu.py.  `python tests/test_norm_kernels_gpu.py` re-measures, on the CPU, the float32 reference errors
that the measured bounds below are derived from.
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_oracle as NO  # noqa: E402

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DT = {F32: "f32", BF16: "bf16"}
EPS = 1e-5

# ---- tolerances for ordinary inputs: the project's own (test_layernorm / test_colsum_logsoftmax of tests/test_kernels_gpu.py)
TOL_FWD = {F32: 1e-5, BF16: 5e-3}   # forward outputs by output dtype; 1e-5 also for mean (relative to the row's mean |x|) / rstd
TOL_BWD = 1e-4                      # backward, per row and per vector
TOL_LSM = 1e-5                      # log-softmax (f32 outputs; bf16 outputs: 5e-3)
TOL_COLSUM = 1e-5                   # column sums, whole vector
# ---- measured bounds.  Per-column error of dgamma / dbeta and of the column sums: the same sums taken in float32 by torch.sum
# on the CPU (prefill included) against float64, worst column over every input of this file, and 8x that for the kernels (another
# order of additions, finished through atomics).
#   LayerNorm dgamma / dbeta: measured 1.79e-07 -> bound 1.4e-06
#   colsum:                   measured 5.96e-08 -> bound 4.7e-07
TOL_COL_LN = 1.4e-6
TOL_COL_COLSUM = 4.7e-7
# Rows x = c + s * randn: the cancellation in x - mean costs about eps_f32 * |c| / s, so the 1e-5 / 1e-4 bounds do not apply by
# construction.  Measured: F.layer_norm (and its autograd) in float32 on the CPU against the float64 oracle on these inputs, worst
# row over d in SHIFT_D; the kernels (the same two-pass scheme, another order of additions) are allowed 4x that.
#   (c, s) = (100, 0.1):   y 6.07e-05 -> 2.4e-04    dx 2.54e-05 -> 1.0e-04
#   (c, s) = (-3000, 1):   y 2.08e-04 -> 8.3e-04    dx 8.66e-05 -> 3.4e-04
TOL_SHIFT = {(100.0, 0.1): (2.4e-4, 1.0e-4), (-3000.0, 1.0): (8.3e-4, 3.4e-4)}
SHIFT_D = (176, 512, 1024)
SHIFT_M = 67


def ops():
    from nemo_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------------------------------------ harness
GUARD = 64            # bytes in front of and behind every output
SENTINEL = -2 ** 31   # guard word 0x80000000 = -0.0f: even an atomic add of +0.0 outside the output turns it into +0.0


class Guarded:
    """a tensor `t` that starts GUARD + off bytes into a sentinel-filled buffer and ends GUARD bytes before its end;
    off = 0 keeps 32-byte alignment, off = 16 (4 floats / 8 bf16) breaks it"""

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
    """(worst row's max_j |got - ref| / max_j |ref|, that row, its worst column).  Entries where the reference is infinite
    must be matched exactly and do not enter the maxima; a row whose reference is all zero must be matched exactly."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    if got.dim() == 1:
        got, ref = got[None], ref[None]
    inf = torch.isinf(ref)
    err = torch.where(inf, torch.where(got == ref, 0.0, float("inf")), (got - torch.where(inf, 0.0, ref)).abs())
    den = torch.where(inf, 0.0, ref).abs().amax(1)
    e = err.amax(1)
    rel = torch.where(den > 0, e / den, torch.where(e == 0, 0.0, float("inf")))
    rel = torch.where(torch.isnan(e), float("inf"), rel)
    r = int(rel.argmax())
    return rel[r].item(), r, int(err[r].nan_to_num(float("inf")).argmax())


def assert_rows(got, ref, tol, what):
    e, r, c = row_err(got, ref)
    print(f"{what}: worst row error {e:.3e} (row {r}, column {c}; bound {tol:.1e})")
    assert e < tol, f"{what}: row {r} is off by {e:.3e} of its largest entry (bound {tol:.1e}), worst at column {c}: " \
                    f"got {got[r].flatten()[c].item() if got.dim() > 1 else got[c].item()!r}"


def col_err(got, prefill, ref_sum, abs_sum):
    """(worst column's |got - (prefill + ref_sum)| / (|prefill| + sum_m |term|), that column)"""
    got, prefill = got.detach().double().cpu(), prefill.detach().double().cpu()
    e = (got - (prefill + ref_sum)).abs() / (prefill.abs() + abs_sum)
    e = torch.where(torch.isnan(e), float("inf"), e)
    c = int(e.argmax())
    return e[c].item(), c


def assert_cols(got, prefill, ref_sum, abs_sum, tol, what):
    e, c = col_err(got, prefill, ref_sum, abs_sum)
    print(f"{what}: worst column error {e:.3e} of its conditioning (column {c}; bound {tol:.1e})")
    assert e < tol, f"{what}: column {c} is off by {e:.3e} of its sum of magnitudes (bound {tol:.1e})"
    v = rel_err(got.detach().cpu() - prefill.cpu(), ref_sum)
    assert v < TOL_BWD, f"{what}: whole-vector error {v:.3e}"


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


# ------------------------------------------------------------------------------------------------ LayerNorm inputs
@functools.lru_cache(maxsize=None)
def ln_case(M, d, xdt=F32, dydt=F32, c=0.5, s=2.0, zero_rows=()):
    """seeded inputs of one LayerNorm problem and its float64 reference (computed once, shared, never modified)"""
    g = torch.Generator().manual_seed(1000 * d + M)
    k = dict(generator=g)
    x = (torch.randn(M, d, **k) * s + c).to(xdt)
    for r in zero_rows:
        x[r] = 0
    z = dict(x=x, gamma=torch.randn(d, **k), beta=torch.randn(d, **k), dy=torch.randn(M, d, **k).to(dydt),
             pre=torch.randn(M, d, **k), pg=torch.randn(d, **k), pb=torch.randn(d, **k))
    z["y"], z["mean"], z["rstd"] = NO.layernorm_fwd(x, z["gamma"], z["beta"], EPS)
    z["mean32"], z["rstd32"] = z["mean"].float(), z["rstd"].float()   # the backward kernels' input: the oracle's, rounded
    z["dx"], z["dgamma"], z["dbeta"], z["abs_g"], z["abs_b"] = NO.layernorm_bwd(z["dy"], x, z["gamma"], z["mean32"], z["rstd32"])
    return z


def fwd_kernel(d, off):
    """the kernel mi355x_layernorm_fwd's launcher selects: a mirror of norm.hip kept in step by hand, it only names the cases"""
    if off == 0 and d in (512, 1024, 2048):
        return f"ln_fwd_reg<{d // 512}>"
    return "ln_fwd_generic"


def bwd_kernel(d, off):
    """the kernel(s) layernorm_bwd_impl selects (a hand-kept mirror of norm.hip, like fwd_kernel)"""
    if off == 0 and d in (512, 1024):
        return f"ln_bwd_fused8<{d // 512}>"
    if d <= 1024:
        return f"ln_bwd_fused<{min(4, (d // 4 + 63) // 64)}>"
    return "ln_bwd_param+dx"


def run_fwd(z, M, d, ydt, off, stats=True):
    o = ops()
    y = Guarded((M, d), ydt, off, fill=float("nan"))
    mean = Guarded(M, F32, 0, fill=float("nan")) if stats else None
    rstd = Guarded(M, F32, 0, fill=float("nan")) if stats else None
    o.layernorm_fwd(put(z["x"], off), put(z["gamma"]), put(z["beta"]), y.t, mean.t if stats else None, rstd.t if stats else None,
                    M, d, EPS)
    assert_intact(y=y, **(dict(mean=mean, rstd=rstd) if stats else {}))
    return y, mean, rstd


def check_stats(z, mean, rstd, tag):
    mean_abs_x = z["x"].double().abs().mean(-1)
    e = ((mean.cpu().double() - z["mean"]).abs() / mean_abs_x)
    assert not torch.isnan(e).any() and e.max().item() < 1e-5, f"{tag}: mean of row {int(e.argmax())} off by {e.max().item():.3e} of its mean |x|"
    e = ((rstd.cpu().double() - z["rstd"]).abs() / z["rstd"])
    assert not torch.isnan(e).any() and e.max().item() < 1e-5, f"{tag}: rstd of row {int(e.argmax())} off by {e.max().item():.3e}"


# ------------------------------------------------------------------------------------------------ LayerNorm forward
FWD_M = (1, 3, 4, 5, 67)   # 4 rows per workgroup
FWD_CASES = []
for _d in (4, 8, 252, 256, 260, 512, 516, 1020, 1024, 1028, 2048, 2052):   # 256 / 260: the generic kernel's loop takes a second trip
    for _off in ((0, 16) if _d in (512, 1024, 2048) else (0,)):
        for _xdt, _ydt in ((F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)):
            if (_xdt, _ydt) == (F32, F32) or _d in (260, 512, 1024):
                FWD_CASES.append(pytest.param(_d, _off, _xdt, _ydt, id=f"{fwd_kernel(_d, _off)}-d{_d}-{DT[_xdt]}-{DT[_ydt]}"))


@pytest.mark.parametrize("d,off,xdt,ydt", FWD_CASES)
def test_layernorm_fwd(d, off, xdt, ydt):
    for M in FWD_M:
        z = ln_case(M, d, xdt)
        tag = f"M={M} d={d}"
        y, mean, rstd = run_fwd(z, M, d, ydt, off)
        assert_rows(y.cpu(), z["y"], TOL_FWD[ydt], f"y {tag}")
        check_stats(z, mean, rstd, tag)
        y2, _, _ = run_fwd(z, M, d, ydt, off, stats=False)   # mean = rstd = NULL: the same y, bit for bit
        assert torch.equal(bits(y2.t), bits(y.t)), f"{tag}: y differs without the statistics outputs"


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def run_bwd(z, M, d, off, accumulate, grads=True, stats=None, cast=None, cast_scale=1.0, drop=None):
    """one launch; returns (dres, prefill of dres or None, dgamma, dbeta, cast_out) as Guarded buffers"""
    o = ops()
    dres = Guarded((M, d), F32, off, src=z["pre"]) if accumulate else Guarded((M, d), F32, off, fill=float("nan"))
    dg = Guarded(d, F32, 0, src=z["pg"]) if grads else None
    db = Guarded(d, F32, 0, src=z["pb"]) if grads else None
    co = Guarded((M, d), BF16, off, fill=float("nan")) if cast else None
    mean, rstd = stats if stats is not None else (put(z["mean32"]), put(z["rstd32"]))
    o.layernorm_bwd(put(z["dy"], off), put(z["x"], off), put(z["gamma"]), mean, rstd, dres.t, bool(accumulate),
                    dg.t if grads else None, db.t if grads else None, M, d, cast_out=co.t if cast else None,
                    cast_scale=cast_scale, cast_drop=drop)
    live = dict(dres=dres)
    if grads:
        live.update(dgamma=dg, dbeta=db)
    if cast:
        live.update(cast_out=co)
    assert_intact(**live)
    return dres, dg, db, co


def check_bwd(z, M, d, off, ref=None, stats=None, tol_dx=TOL_BWD, tag=""):
    ref = ref or z
    for accumulate in (0, 1):
        t = f"{tag} M={M} d={d} accumulate={accumulate}"
        dres, dg, db, _ = run_bwd(z, M, d, off, accumulate, stats=stats)
        got = dres.cpu()
        assert torch.isfinite(got).all(), f"{t}: dres not finite (accumulate=0 must overwrite, not read)"
        assert_rows(got.double() - (z["pre"].double() if accumulate else 0.0), ref["dx"], tol_dx, f"dres {t}")
        assert_cols(dg.cpu(), z["pg"], ref["dgamma"], ref["abs_g"], TOL_COL_LN, f"dgamma {t}")
        assert_cols(db.cpu(), z["pb"], ref["dbeta"], ref["abs_b"], TOL_COL_LN, f"dbeta {t}")
        only_dx, _, _, _ = run_bwd(z, M, d, off, accumulate, grads=False, stats=stats)   # dgamma = dbeta = NULL
        assert torch.equal(bits(only_dx.t), bits(dres.t)), f"{t}: dres differs when no parameter gradient is requested"


BWD_TABLE = {  # layernorm_bwd_impl, one line per row of its dispatch (read off norm.hip; keep in step with it by hand)
    "ln_bwd_fused<1>": [(4, 0), (252, 0)],
    "ln_bwd_fused<2>": [(260, 0), (512, 16)],
    "ln_bwd_fused<3>": [(516, 0), (768, 0)],
    "ln_bwd_fused<4>": [(772, 0), (1020, 0), (1024, 16)],
    "ln_bwd_fused8<1>": [(512, 0)],
    "ln_bwd_fused8<2>": [(1024, 0)],
    "ln_bwd_param+dx": [(1028, 0), (2048, 0)],
}
BWD_M_SWEEP = (1, 15, 16, 17, 63, 64, 65, 129)   # 64 rows per workgroup, 16 waves, wave w takes rows w, w + 16, ...
BWD_CASES = []
for _name, _rows in BWD_TABLE.items():
    for _d, _off in _rows:
        for _M in (BWD_M_SWEEP if _d in (260, 512, 1024) else (67,)):
            BWD_CASES.append(pytest.param(_d, _off, F32, F32, _M, id=f"{_name}-d{_d}-f32-f32-M{_M}"))
        if _d in (260, 512, 1024, 1028):
            for _xdt, _dydt in ((F32, BF16), (BF16, F32), (BF16, BF16)):
                BWD_CASES.append(pytest.param(_d, _off, _xdt, _dydt, 65, id=f"{_name}-d{_d}-{DT[_xdt]}-{DT[_dydt]}-M65"))


@pytest.mark.parametrize("d,off,xdt,dydt,M", BWD_CASES)
def test_layernorm_bwd(d, off, xdt, dydt, M):
    """statistics = the oracle's, rounded to f32: a forward error cannot mask a backward one"""
    check_bwd(ln_case(M, d, xdt, dydt), M, d, off)


@pytest.mark.parametrize("d,off", [(176, 0), (512, 0), (1024, 0), (1024, 16), (1028, 0)],
                         ids=lambda v: str(v))
def test_layernorm_bwd_on_the_kernels_own_statistics(d, off):
    M = 67
    z = ln_case(M, d)
    _, mean, rstd = run_fwd(z, M, d, F32, off)
    ref = dict(zip(("dx", "dgamma", "dbeta", "abs_g", "abs_b"), NO.layernorm_bwd(z["dy"], z["x"], z["gamma"], mean.cpu(), rstd.cpu())))
    check_bwd(z, M, d, off, ref=ref, stats=(mean.t, rstd.t), tag="own statistics")


CAST_CASES = [pytest.param(512, 0, id="ln_bwd_fused8<1>-d512"), pytest.param(1024, 0, id="ln_bwd_fused8<2>-d1024"),
              pytest.param(512, 16, id="ln_bwd_fused<2>+cast_after-d512"), pytest.param(260, 0, id="ln_bwd_fused<2>+cast_after-d260"),
              pytest.param(1028, 0, id="ln_bwd_param+dx+cast_after-d1028")]


@pytest.mark.parametrize("d,off", CAST_CASES)
def test_layernorm_bwd_cast_out_is_the_rounded_residual_gradient(d, off):
    """cast_out = bf16(cast_scale * dres_new), from the kernel's own f32 dres, to the last bit: pack_bf2 (common.h) is
    __builtin_convertvector float -> __bf16, round to nearest even, which is what torch's .to(bfloat16) does"""
    M, scale = 66, 0.37   # M * d % 8 == 0 is required by the separate cast pass
    z = ln_case(M, d)
    for accumulate in (0, 1):
        dres, dg, db, co = run_bwd(z, M, d, off, accumulate, cast=True, cast_scale=scale)
        got = dres.cpu()
        assert_rows(got.double() - (z["pre"].double() if accumulate else 0.0), z["dx"], TOL_BWD, f"dres d={d} accumulate={accumulate}")
        assert_cols(dg.cpu(), z["pg"], z["dgamma"], z["abs_g"], TOL_COL_LN, f"dgamma d={d}")
        assert_cols(db.cpu(), z["pb"], z["dbeta"], z["abs_b"], TOL_COL_LN, f"dbeta d={d}")
        want = (got * torch.tensor(scale, dtype=F32)).to(BF16)
        assert torch.equal(bits(co.t), bits(want)), f"d={d} accumulate={accumulate}: {int((bits(co.t) != bits(want)).sum())} cast_out elements differ"


def host_keep_mask(drop, n):
    """drop_mask() of common.h in numpy: element e of hash group g is kept iff output (e % 8) + 1 of the xorshift32 stream
    seeded by the group's hash is >= threshold"""
    def mix32(x):
        x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x7feb352d); x = x ^ (x >> np.uint32(15)); x = x * np.uint32(0x846ca68b)
        return x ^ (x >> np.uint32(16))
    key = drop.key & 0xFFFFFFFF
    grp = np.arange(n // 8, dtype=np.uint32)
    with np.errstate(over="ignore"):
        s = mix32(mix32(grp ^ np.uint32(key)) + np.uint32((0x9E3779B9 * (key | 1)) & 0xFFFFFFFF)) | np.uint32(1)
        keep = np.empty((n // 8, 8), dtype=bool)
        for j in range(8):
            s = s ^ (s << np.uint32(13)); s = s ^ (s >> np.uint32(17)); s = s ^ (s << np.uint32(5))
            keep[:, j] = s >= np.uint32(drop.threshold)
    return torch.from_numpy(keep.reshape(-1))


@pytest.mark.parametrize("d,share_tol", [(512, 0.04), (1024, 0.03)])
def test_layernorm_bwd_cast_out_dropout_mask(d, share_tol):
    """fused8 (aligned) and the separate cast pass (16-byte offset) index the mask by linear element: the same zero set, which
    is the one drop_mask() of common.h defines; kept values are dres * cast_scale / (1 - p) to a bf16 ulp; dres is not masked.
    (The mask is decided per element -- 8 consecutive elements share one hash, not one decision -- so zeros do not come in
    groups of 8.)"""
    o = ops()
    o.set_step_counter(None)   # keys as passed: a test that wants a step word registers its own, none relies on one being left
    M, scale, p = 65, 0.5, 0.25
    z = ln_case(M, d)
    drop = o.Dropout(p, 11, 3)
    outs = []
    for off in (0, 16):
        dres, _, _, co = run_bwd(z, M, d, off, 0, cast=True, cast_scale=scale, drop=drop)
        plain, _, _, _ = run_bwd(z, M, d, off, 0)
        assert torch.equal(bits(plain.t), bits(dres.t)), f"d={d} off={off}: the mask leaked into dres"
        assert_rows(dres.cpu(), z["dx"], TOL_BWD, f"dres d={d} off={off}")
        outs.append((dres.cpu(), co.cpu()))
    zero = [c.float().flatten() == 0 for _, c in outs]
    assert torch.equal(zero[0], zero[1]), f"d={d}: {int((zero[0] != zero[1]).sum())} elements dropped on one path only"
    assert torch.equal(~zero[0], host_keep_mask(drop, M * d)), f"d={d}: not the mask drop_mask() defines"
    share = zero[0].float().mean().item()
    assert abs(share - p) < share_tol, share
    for (dres, co), zz in zip(outs, zero):
        kept = ~zz.view(M, d)
        want = dres.double() * scale / (1 - p)
        ulp = 2.0 ** (torch.floor(torch.log2(want.abs().clamp_min(1e-30))) - 7)   # bf16: 8 significant bits
        assert bool((((co.double() - want).abs() <= ulp) | ~kept).all()), f"d={d}: a kept value is off by more than a bf16 ulp"


# ------------------------------------------------------------------------------------------------ LayerNorm edges
@pytest.mark.parametrize("d", [176, 512, 1024])
def test_layernorm_zero_rows(d):
    """padded frames are zero rows: y = beta exactly, mean = 0, rstd = 1/sqrt(eps); backward finite and within tolerance"""
    M, zero_rows = 9, (0, 3, 4, 8)
    z = ln_case(M, d, zero_rows=zero_rows)
    for ydt in (F32, BF16):
        y, mean, rstd = run_fwd(z, M, d, ydt, 0)
        for r in zero_rows:
            assert torch.equal(bits(y.t[r]), bits(z["beta"].to(ydt))), f"row {r}: y != beta"
            assert mean.cpu()[r].item() == 0.0
            assert abs(rstd.cpu()[r].item() * math.sqrt(EPS) - 1) < 1e-6
        assert_rows(y.cpu(), z["y"], TOL_FWD[ydt], f"y d={d}")
        live = [r for r in range(M) if r not in zero_rows]   # the ordinary rows between them: statistics as everywhere else
        check_stats({k: z[k][live] for k in ("x", "mean", "rstd")}, mean.t[live], rstd.t[live], f"d={d} ordinary rows")
    check_bwd(z, M, d, 0, tag="zero rows")


def _shift_case(c, s, d):
    return ln_case(SHIFT_M, d, F32, F32, c, s)


def _cpu_f32_shift_errors(c, s):
    """(worst row error of y, worst row error of dx) of F.layer_norm in float32 on the CPU against the oracle, over SHIFT_D"""
    ey = ex = 0.0
    for d in SHIFT_D:
        z = _shift_case(c, s, d)
        x = z["x"].clone().requires_grad_(True)
        y = F.layer_norm(x, (d,), z["gamma"], z["beta"], EPS)
        y.backward(z["dy"])
        dx64 = NO.layernorm_bwd(z["dy"], z["x"], z["gamma"], z["mean"], z["rstd"])[0]
        ey, ex = max(ey, row_err(y.detach(), z["y"])[0]), max(ex, row_err(x.grad, dx64)[0])
    return ey, ex


@pytest.mark.parametrize("d", SHIFT_D)
@pytest.mark.parametrize("c,s", list(TOL_SHIFT))
def test_layernorm_rows_whose_mean_dwarfs_their_spread(c, s, d):
    tol_y, tol_dx = TOL_SHIFT[(c, s)]
    z = _shift_case(c, s, d)
    y, mean, rstd = run_fwd(z, SHIFT_M, d, F32, 0)
    assert_rows(y.cpu(), z["y"], tol_y, f"y c={c} s={s} d={d}")
    check_stats(z, mean, rstd, f"c={c} s={s} d={d}")
    check_bwd(z, SHIFT_M, d, 0, tol_dx=tol_dx, tag=f"c={c} s={s}")


# ------------------------------------------------------------------------------------------------ log-softmax
LSM_C = (1, 2, 63, 64, 65, 129, 1025)   # one wave per row, 64-column stride
LSM_M = (1, 5, 130)
LSM_KINDS = ("unit", "shifted", "neginf")


@functools.lru_cache(maxsize=None)
def lsm_case(M, C, kind):
    g = torch.Generator().manual_seed(7000 + 10 * C + M)
    x = torch.randn(M, C, generator=g)
    if kind == "shifted":
        x = 30 * x + 1e4                 # a kernel without the max subtraction overflows
    if kind == "neginf":
        x[:, ::3] = float("-inf")        # a third of each row, never the whole row (C >= 2)
    y = NO.log_softmax_fwd(x)
    return dict(x=x, y=y, y32=y.float(), dy=torch.randn(M, C, generator=g))


LSM_CASES = [pytest.param(C, kind, id=f"C{C}-{kind}") for kind in LSM_KINDS for C in LSM_C
             if not (kind == "neginf" and C < 2)]   # a row of one class cannot be partly -inf


@pytest.mark.parametrize("C,kind", LSM_CASES)
def test_log_softmax_fwd(C, kind):
    o = ops()
    ld_in, ld_out = C + 3, C + 5
    for M in LSM_M:
        z = lsm_case(M, C, kind)
        xin = torch.full((M, ld_in), float("nan")); xin[:, :C] = z["x"]
        out = Guarded((M, ld_out), F32, 0, fill=7.0)
        o.log_softmax_fwd(put(xin), ld_in, out.t, ld_out, M, C)
        assert_intact(logp=out)
        got = out.cpu()
        assert bool((got[:, C:] == 7.0).all()), f"M={M} C={C}: columns [C, ld_out) of logp were written"
        if kind == "neginf":
            assert bool((got[:, :C][:, ::3] == float("-inf")).all()) and bool(torch.isfinite(got[:, :C][:, 1::3]).all())
        if kind == "shifted":
            assert torch.isfinite(got[:, :C]).all(), f"M={M} C={C}: overflow"
        assert_rows(got[:, :C], z["y"], TOL_LSM, f"logp M={M} C={C} {kind}")


@pytest.mark.parametrize("odt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C,kind", LSM_CASES)
def test_log_softmax_bwd(C, kind, odt):
    """input: the oracle's log-probabilities rounded to f32.  Pad columns [C, ld_out) are exactly zero, nothing beyond ld_out
    is written; where log p = -inf the gradient is exactly scale * dy"""
    o = ops()
    for M in LSM_M:
        z = lsm_case(M, C, kind)
        dy_d, y_d = put(z["dy"]), put(z["y32"])
        for scale in (1.0, 0.125):
            ref = NO.log_softmax_bwd(z["dy"], z["y32"], scale)
            for ld_out in (C, (C + 7) // 8 * 8 + 8):
                t = f"dlogits M={M} C={C} {kind} scale={scale} ld_out={ld_out}"
                out = Guarded((M, ld_out), odt, 0, fill=float("nan"))
                o.log_softmax_bwd(dy_d, y_d, C, out.t, ld_out, M, C, scale)
                assert_intact(dlogits=out)
                got = out.cpu().float()
                assert bool((got[:, C:] == 0).all()), f"{t}: pad columns not zero"
                assert torch.isfinite(got).all(), t
                if kind == "neginf":
                    assert torch.equal(got[:, :C][:, ::3], (scale * z["dy"][:, ::3]).to(odt).float()), f"{t}: not scale * dy where p = 0"
                assert_rows(got[:, :C], ref, TOL_LSM if odt == F32 else TOL_FWD[BF16], t)


# ------------------------------------------------------------------------------------------------ column sums
@functools.lru_cache(maxsize=None)
def colsum_case(M, N, dtype, ld, x_off):
    g = torch.Generator().manual_seed(9000 + 7 * N + M)
    buf = torch.randn(x_off + M * ld + 16, generator=g).to(dtype)   # what lies between the rows is data too, not zeros
    x = buf[x_off:x_off + M * ld].view(M, ld)[:, :N]
    return dict(buf=buf, x=x, pre=torch.randn(N, generator=g))


def run_colsum(z, M, N, ld, x_off, alpha, buf_shift=0):
    """buf_shift: elements by which the whole buffer is moved on the device (x_off grows by it, the data stay the same)"""
    o = ops()
    out = Guarded(N, F32, 0, src=z["pre"])
    b = z["buf"] if not buf_shift else torch.cat([torch.zeros(buf_shift, dtype=z["buf"].dtype), z["buf"]])
    o.colsum(put(b), out.t, M, N, ld=ld, alpha=alpha, x_off=x_off + buf_shift)
    assert_intact(out=out)
    return out.cpu()


def check_colsum(got, z, alpha, tag):
    s, a = NO.colsum(z["x"], alpha)
    e, c = col_err(got, z["pre"], s, a)
    print(f"colsum {tag}: worst column error {e:.3e} (column {c}; bound {TOL_COL_COLSUM:.1e})")
    assert e < TOL_COL_COLSUM, f"colsum {tag}: column {c} is off by {e:.3e} of its sum of magnitudes"
    v = rel_err(got, z["pre"].double() + s)
    assert v < TOL_COLSUM, f"colsum {tag}: whole-vector error {v:.3e}"


COLSUM_GENERIC_M = (1, 255, 256, 257, 600)   # 256 rows per workgroup
COLSUM_X8_M = (1, 63, 64, 65, 200)           # 64 rows per workgroup


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N", [1, 63, 65, 129])   # N % 8 != 0: bf16 stays on the generic kernel
def test_colsum_generic(N, dtype):
    ld, x_off = N + 3, 5
    for M in COLSUM_GENERIC_M:
        z = colsum_case(M, N, dtype, ld, x_off)
        for alpha in (1.0, -0.5):
            check_colsum(run_colsum(z, M, N, ld, x_off, alpha), z, alpha, f"M={M} N={N} alpha={alpha}")


@pytest.mark.parametrize("N", [8, 16, 24, 136, 256, 520])   # 24: 3 chunks, does not divide 64; 520: a partial second 512-column block
def test_colsum_bf16x8(N):
    """colsum_bf16x8_kernel, and the same x one element (2 bytes) further on, which takes the generic kernel"""
    ld, x_off = N + 8, 8
    for M in COLSUM_X8_M:
        z = colsum_case(M, N, BF16, ld, x_off)
        for alpha in (1.0, -0.5):
            a = run_colsum(z, M, N, ld, x_off, alpha)
            b = run_colsum(z, M, N, ld, x_off, alpha, buf_shift=1)
            check_colsum(a, z, alpha, f"bf16x8 M={M} N={N} alpha={alpha}")
            check_colsum(b, z, alpha, f"generic at a 2-byte offset M={M} N={N} alpha={alpha}")
            assert rel_err(a, b) < TOL_COLSUM


# ------------------------------------------------------------------------------------------------ reference-error measurement
def measure_reference_errors():
    """the float32 CPU figures the measured bounds at the top of this file are derived from (no GPU needed)"""
    worst = 0.0
    cases = {(p.values[0], p.values[2], p.values[3], p.values[4]) for p in BWD_CASES}
    cases |= {(d, F32, F32, M) for d, M in [(176, 67), (512, 67), (1024, 67), (1028, 67), (512, 66), (1024, 66), (260, 66), (1028, 66),
                                            (512, 65), (1024, 65)]}
    zs = [ln_case(M, d, xdt, dydt) for d, xdt, dydt, M in sorted(cases, key=str)]
    zs += [ln_case(9, d, zero_rows=(0, 3, 4, 8)) for d in (176, 512, 1024)]
    zs += [_shift_case(c, s, d) for c, s in TOL_SHIFT for d in SHIFT_D]
    for z in zs:
        xhat = (z["x"].float() - z["mean32"][:, None]) * z["rstd32"][:, None]
        dy = z["dy"].float()
        worst = max(worst, col_err(z["pg"] + torch.sum(dy * xhat, 0), z["pg"], z["dgamma"], z["abs_g"])[0],
                    col_err(z["pb"] + torch.sum(dy, 0), z["pb"], z["dbeta"], z["abs_b"])[0])
    print(f"LayerNorm dgamma / dbeta, float32 torch.sum, worst column: {worst:.3e} -> x8 = {8 * worst:.3e}")
    worst = 0.0
    todo = [(M, N, dt_, N + 3, 5) for N in (1, 63, 65, 129) for dt_ in (F32, BF16) for M in COLSUM_GENERIC_M]
    todo += [(M, N, BF16, N + 8, 8) for N in (8, 16, 24, 136, 256, 520) for M in COLSUM_X8_M]
    for M, N, dt_, ld, x_off in todo:
        z = colsum_case(M, N, dt_, ld, x_off)
        for alpha in (1.0, -0.5):
            s, a = NO.colsum(z["x"], alpha)
            worst = max(worst, col_err(z["pre"] + alpha * torch.sum(z["x"].float(), 0), z["pre"], s, a)[0])
    print(f"colsum, float32 torch.sum, worst column: {worst:.3e} -> x8 = {8 * worst:.3e}")
    for c, s in TOL_SHIFT:
        ey, ex = _cpu_f32_shift_errors(c, s)
        print(f"(c, s) = ({c}, {s}): F.layer_norm float32 worst row: y {ey:.3e} -> x4 = {4 * ey:.3e}; dx {ex:.3e} -> x4 = {4 * ex:.3e}")


if __name__ == "__main__":
    measure_reference_errors()
