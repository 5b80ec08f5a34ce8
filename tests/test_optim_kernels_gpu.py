"""-m gpu: every kernel path of nemo_amd/csrc/optim.hip (AdamW step, gradient sum of squares, clip coefficient, fill, weight-image
pack) through the Python wrappers against the float64 closed forms of tests/elementwise_oracle.py.  The harness (sentinel-guarded
outputs, bit comparison) is the one of tests/test_elementwise_kernels_gpu.py.

AdamW.  One step from a drawn state (p, g, m, v, ema in float32, the oracle up-casts them) at a given step number, so each step's
bias corrections are tested on their own.  Gradients span 1e-6 .. 1e3 and include exact zeros; |p| <= lr / 16, so that the rounding
of p cannot hide an error in the update.  Measures, per element, worst element asserted:
  dp    |dp_got - dp_ref| / max(|dp_ref|, floor), dp = p_new - p_old, floor = lr * (sqrt(bc2) / bc1) / 8: relative above the floor
  m     |m_got - m_ref| / (|beta1 * m| + |(1 - beta1) * g * scale|), its conditioning
  v     |v_got - v_ref| / v_ref
  ema   |ema_got - ema_ref| / (|decay * ema| + (1 - decay) * (|p_old| + |dp_ref|)), its conditioning: the kernel feeds it the p_new
        it has just made, whose own error is relative to |p_old| + |dp|, not to a |p_new| that may have cancelled
Bounds: a float32 torch restatement of the kernel's operation order on the CPU (bias corrections taken in float64 and rounded
once) against the float64 oracle, worst element over ADAMW_CASES; the kernel is allowed 4x that (FMA contraction, another
rounding order).
  dp   measured 5.03e-07 -> bound 2.0e-06
  m    measured 1.53e-07 -> bound 6.1e-07
  v    measured 1.19e-07 -> bound 4.7e-07
  ema  measured 7.37e-07 -> bound 2.9e-06
(With the bias corrections taken in float32 on the host, `1.f - powf(beta2, step)`, the same restatement gives dp 3.6e-06 at beta2 =
0.999 and step 2, 3.2e-06 at step 3, 2.7e-06 at step 5: above the bound.  adamw_launch takes them in double and rounds once.)

grad_sumsq: |got - ref| / (|prefill| + sum g^2) against the float64 sum; float32 torch.sum(g * g) on the CPU measures 6.35e-08 on
these inputs, the kernel (float32 block partials, one float64 atomic per block) is allowed 8x: 5.0e-07.
clip_coef: both outputs to 4 * 2^-24 relative (sqrt, scale, add and divide in float32 after a float64 sum).
fill_f32 and the pack kernel move data: bit equality, pad columns zero, everything around the images untouched.
`python tests/test_optim_kernels_gpu.py` re-measures the float32 figures on the CPU.
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elementwise_oracle as EO  # noqa: E402
from test_elementwise_kernels_gpu import Guarded, assert_bits, assert_intact, dev, fresh_ops, put  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64

TOL_ADAMW = dict(dp=2.0e-6, m=6.1e-7, v=4.7e-7, ema=2.9e-6)   # measured, see the header
TOL_SUMSQ = 5.0e-7                                          # measured, see the header
TOL_CLIP = 4 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ AdamW
LR = 1e-3
GRAD_SCALE, CLIP = 0.5, 0.37
CLIP_F32 = EO.f32(CLIP)                             # the coefficient is a float32 on the device
ADAMW_BIG = 4 * (EO.GRID_CAP["adamw"] * 256 + 5)    # a second grid-stride trip
# (n, step, beta2, wd, eps, clip, ema_decay or None); beta1 = 0.9
ADAMW_CASES = [(4 * 257, step, b2, 1e-2, 1e-8, False, None) for b2 in (0.98, 0.999) for step in (1, 2, 3, 4, 5, 6, 100000)]
ADAMW_CASES += [(4 * 257, 3, b2, wd, eps, False, None) for b2 in (0.98, 0.999) for wd, eps in ((0.0, 1e-8), (0.0, 1e-3), (1e-2, 1e-3))]
ADAMW_CASES += [(4 * 257, 2, 0.999, 1e-2, 1e-8, True, None)]
ADAMW_CASES += [(4 * 257, 2, b2, 1e-2, 1e-8, clip, d) for b2 in (0.98, 0.999) for clip, d in ((True, 0.0), (True, 0.999), (False, 1.0))]
ADAMW_CASES += [(4, 1, 0.999, 1e-2, 1e-8, False, None), (4, 4, 0.98, 0.0, 1e-3, True, 0.999)]
ADAMW_CASES += [(ADAMW_BIG, 3, 0.999, 1e-2, 1e-8, True, 0.999)]
BETA1 = 0.9


def adamw_id(c):
    n, step, b2, wd, eps, clip, d = c
    return f"n{n}-step{step}-b2_{b2}-wd{wd}-eps{eps}" + ("-clip" if clip else "") + (f"-ema{d}" if d is not None else "")


@functools.lru_cache(maxsize=4)
def adamw_state(n, clip):
    """a drawn optimizer state: gradient magnitudes h = 10^U(-6, 3) with every eighth gradient exactly zero, moments of the
    size a history of such gradients leaves, |p| and |ema| <= lr / 16"""
    g = torch.Generator().manual_seed(n + int(clip))
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(n, generator=g)   # noqa: E731
    h = 10.0 ** u(-6, 3)
    gs = GRAD_SCALE * CLIP if clip else 1.0
    grad = h * u(0.5, 1.5) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
    grad[torch.randperm(n, generator=g)[:max(1, n // 8)]] = 0.0
    return dict(g=grad.float(), m=(h * gs * u(-1, 1)).float(), v=((h * gs) ** 2 * u(0.5, 2)).float(),
                p=(LR / 16 * u(-1, 1)).float(), ema=(LR / 16 * u(-1, 1)).float())


def adamw_reference(case):
    n, step, b2, wd, eps, clip, d = case
    z = adamw_state(n, clip)
    return EO.adamw_step(z["p"], z["g"], z["m"], z["v"], LR, BETA1, b2, eps, wd, step, GRAD_SCALE if clip else 1.0,
                         CLIP_F32 if clip else None, z["ema"] if d is not None else None, d or 0.0)


def adamw_errors(case, got):
    """the four measures of the header for (p, m, v, ema) = got"""
    n, step, b2, wd, eps, clip, d = case
    z = adamw_state(n, clip)
    p, m, v, ema = adamw_reference(case)
    b1 = EO.f32(BETA1)
    bc1, bc2s = EO.bias_corrections(BETA1, b2, step)
    floor = EO.f32(LR) * (bc2s / bc1) / 8
    p0, gr = z["p"].double(), z["g"].double() * (EO.f32(GRAD_SCALE) * CLIP_F32 if clip else 1.0)
    dp_ref = p - p0
    out = dict(dp=((got[0].double() - p0 - dp_ref).abs() / dp_ref.abs().clamp_min(floor)).max().item(),
               m=((got[1].double() - m).abs() / ((b1 * z["m"].double()).abs() + ((1 - b1) * gr).abs())).max().item(),
               v=((got[2].double() - v).abs() / v).max().item())
    if d is not None:
        dd = EO.f32(d)
        cond_p = p0.abs() + dp_ref.abs()     # p_new is made in the same pass: its own conditioning, not |p_new|, which can cancel
        out["ema"] = ((got[3].double() - ema).abs() / ((dd * z["ema"].double()).abs() + (1 - dd) * cond_p)).max().item()
    assert all(math.isfinite(e) for e in out.values()), out
    return out, int((dp_ref.abs() >= floor).sum())


def adamw_float32(case, f32_bias_corrections=False):
    """the kernel's operation order in float32 torch on the CPU; bias corrections from float64, rounded once (or, for the figure
    the header quotes, taken in float32 as `1.f - powf(beta, step)`)"""
    n, step, b2, wd, eps, clip, d = case
    z = adamw_state(n, clip)
    f = np.float32
    t = lambda x: torch.tensor(x, dtype=F32)   # noqa: E731
    lr, b1, b2, eps, wd = f(LR), f(BETA1), f(b2), f(eps), f(wd)
    if f32_bias_corrections:
        bc1, bc2s = f(1) - f(float(b1) ** step), np.sqrt(f(1) - f(float(b2) ** step))   # powf correctly rounded
    else:
        bc1, bc2s = (f(x) for x in EO.bias_corrections(BETA1, b2, step))
    gs = f(GRAD_SCALE) * f(CLIP) if clip else f(1)
    gr = z["g"] * t(gs)
    p = z["p"] * t(f(1) - lr * wd)
    m = t(b1) * z["m"] + t(f(1) - b1) * gr
    v = t(b2) * z["v"] + t(f(1) - b2) * gr * gr
    p = p - t(lr / bc1) * (m / (v.sqrt() / t(bc2s) + t(eps)))
    ema = None
    if d is not None:
        ema = z["ema"] * t(f(d)) + t(f(1) - f(d)) * p
    return p, m, v, ema


@pytest.mark.parametrize("case", ADAMW_CASES, ids=[adamw_id(c) for c in ADAMW_CASES])
def test_adamw_step(case):
    o = fresh_ops()
    n, step, b2, wd, eps, clip, d = case
    z = adamw_state(n, clip)
    p, m, v = (Guarded(n, F32, src=z[k]) for k in ("p", "m", "v"))
    ema = Guarded(n, F32, src=z["ema"]) if d is not None else None
    coef = put(torch.tensor([CLIP, 0.0])) if clip else None
    o.adamw_step(p.t, put(z["g"]), m.t, v.t, LR, BETA1, b2, eps, wd, step, grad_scale=GRAD_SCALE if clip else 1.0,
                 clip_coef=coef, ema=ema.t if ema else None, ema_decay=d or 0.0)
    assert_intact(p=p, m=m, v=v, **(dict(ema=ema) if ema else {}))
    errs, counted = adamw_errors(case, (p.cpu(), m.cpu(), v.cpu(), ema.cpu() if ema else None))
    print(f"adamw {adamw_id(case)}: " + ", ".join(f"{k} {e:.3e} (bound {TOL_ADAMW[k]:.1e})" for k, e in errs.items())
          + f"; {counted} of {n} updates above the floor")
    if n > 1000:
        assert counted > n // 4, "too few updates above the floor for the relative measure to mean anything"
    for k, e in errs.items():
        assert e < TOL_ADAMW[k], f"{adamw_id(case)}: {k} is off by {e:.3e} (bound {TOL_ADAMW[k]:.1e})"
    if d == 1.0:
        assert_bits(ema.cpu(), z["ema"], "ema at decay 1")
    if d == 0.0:
        assert_bits(ema.cpu(), p.cpu(), "ema at decay 0")


# ------------------------------------------------------------------------------------------------ grad_sumsq / clip_coef / fill
SUMSQ_N = (4, 4 * 300, 4 * (EO.GRID_CAP["sumsq"] * 256 + 7))   # the last: a second grid-stride trip
SUMSQ_PRE = (3.0, -7.0, 11.0)


@functools.lru_cache(maxsize=None)
def sumsq_input(n, k):
    return torch.randn(n, generator=torch.Generator().manual_seed(n + k))


def sumsq_err(got, pre, gs):
    ref = pre + sum(float(g.double().square().sum()) for g in gs)
    return abs(got - ref) / (abs(pre) + sum(float(g.double().square().sum()) for g in gs))


@pytest.mark.parametrize("n", SUMSQ_N)
def test_grad_sumsq_accumulates_into_its_slot(n):
    o = fresh_ops()
    g1, g2, g3 = (sumsq_input(n, k) for k in range(3))
    slots = Guarded(3, F64, src=torch.tensor(SUMSQ_PRE, dtype=F64))
    o.grad_sumsq(put(g1), slots.t[0:1])
    o.grad_sumsq(put(g2), slots.t[0:1])     # two buffers into one slot
    o.grad_sumsq(put(g3), slots.t[2:3])
    assert_intact(slots=slots)
    got = slots.cpu()
    assert got[1].item() == SUMSQ_PRE[1], "a slot no call named was written"
    for slot, gs in ((0, (g1, g2)), (2, (g3,))):
        e = sumsq_err(got[slot].item(), SUMSQ_PRE[slot], gs)
        print(f"grad_sumsq n={n} slot {slot}: off by {e:.3e} (bound {TOL_SUMSQ:.1e})")
        assert e < TOL_SUMSQ, f"n={n} slot {slot}: off by {e:.3e} of its sum (bound {TOL_SUMSQ:.1e})"


CLIP_CASES = [((4.0,), 1.0, 3.0), ((4.0,), 1.0, 2.0), ((4.0,), 1.0, 1.0), ((1.0, 2.5, 0.75), 1.0, 1.7), ((1.0, 2.5, 0.75), 0.5, 1.0),
              ((1.0, 2.5, 0.75), 0.5, 1.1), ((9.0e6, 1.0e-3, 4.0), 0.5, 1.0), ((0.0,), 1.0, 1.0), ((0.0, 0.0, 0.0), 0.5, 0.25)]


@pytest.mark.parametrize("sums,scale,max_norm", CLIP_CASES, ids=[f"nbuf{len(c[0])}-{k}" for k, c in enumerate(CLIP_CASES)])
def test_clip_coef(sums, scale, max_norm):
    """norms below, at and above max_norm, one and three buffers, a scale of 0.5; a sum of 0 gives coefficient 1"""
    o = fresh_ops()
    out = Guarded(2, F32, fill=float("nan"))
    o.clip_coef(put(torch.tensor(sums, dtype=F64)), scale, max_norm, out.t)
    assert_intact(coef=out)
    coef, norm = (x.item() for x in out.cpu())
    rc, rn = EO.clip_coef(sums, scale, max_norm)
    if sum(sums) == 0:
        assert coef == 1.0 and norm == 0.0
    assert abs(coef - rc) <= TOL_CLIP * rc, f"coefficient {coef!r}, reference {rc!r}"
    assert abs(norm - rn) <= TOL_CLIP * rn, f"norm {norm!r}, reference {rn!r}"
    assert coef <= 1.0


FILL_N = (1, 255, EO.GRID_CAP["fill_f32"] * 256 + 3)


@pytest.mark.parametrize("n", FILL_N)
def test_fill_f32(n):
    o = fresh_ops()
    for value in (-0.0, 2.5):
        x = Guarded(n, F32, fill=float("nan"))
        o.fill_f32(x.t, value)
        assert_intact(x=x)
        assert_bits(x.cpu(), torch.full((n,), value), f"fill_f32 n={n} value={value}")


# ------------------------------------------------------------------------------------------------ pack
def pack_sources(device):
    """float32 master weights; `mis` starts 4 bytes into its storage: vector-eligible tiles on a source that is not 16-byte aligned"""
    g = torch.Generator().manual_seed(13)
    r = lambda *s: torch.randn(*s, generator=g).to(device)   # noqa: E731
    flat = r(128 * 64 + 1)
    return dict(m64=r(64, 64), m70=r(70, 45), m200=r(200, 136), mis=flat[1:].view(128, 64), cat=[r(8, 40), r(16, 40), r(24, 40)],
                conv=r(16, 8, 3, 3), fc=r(24, 40), flat=flat)


def declare_pack(plan, w):
    """every PackPlan declaration, both orientations, in ONE plan: 18 entries, a one-tile entry first and last"""
    plan.add_matrix("m64", w["m64"])
    for k in ("m70", "m200", "mis"):
        plan.add_matrix(k, w[k]); plan.add_matrix(k + ".t", w[k], transpose=True)
    plan.add_concat("cat", w["cat"]); plan.add_concat("cat.t", w["cat"], transpose=True)
    plan.add_conv3x3("conv", w["conv"]); plan.add_conv3x3("conv.t", w["conv"], transpose=True)
    plan.add_fc_permuted("fc", w["fc"], 8, 5); plan.add_fc_permuted("fc.t", w["fc"], 8, 5, transpose=True)
    plan.add_matrix("m64.t", w["m64"], transpose=True)
    return plan


def pack_entries(plan):
    """the declared blocks as dicts (what elementwise_oracle.pack_path and pack_image read)"""
    keys = ("name", "src", "rows", "cols", "row_off", "col_off", "nr2", "nc2", "sr1", "sr2", "sc1", "sc2")
    out = [dict(zip(keys, p)) for p in plan._pending]
    for e in out:
        e["src_addr"] = e["src"].data_ptr()
    return out


def pack_images(plan, dtype):
    """name -> the float64-free oracle image [rows, pitch] in `dtype`: zeros, then every block by plain indexing"""
    imgs = {name: torch.zeros(rows, pitch) for name, (_, rows, pitch) in plan._images.items()}
    for e in pack_entries(plan):
        imgs[e["name"]][e["row_off"]:e["row_off"] + e["rows"], e["col_off"]:e["col_off"] + e["cols"]] = \
            EO.pack_image(e["src"], e["rows"], e["cols"], e["nr2"], e["nc2"], e["sr1"], e["sr2"], e["sc1"], e["sc2"])
    return {k: v.to(dtype) for k, v in imgs.items()}


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_pack_weights_every_declaration_in_one_plan(dtype):
    from nemo_amd.packing import PackPlan
    fresh_ops()
    w = pack_sources(dev)
    assert w["mis"].data_ptr() % 16 == 4 and w["mis"].is_contiguous()
    plan = declare_pack(PackPlan(dtype, dev), w)
    plan.finalize()
    assert plan._n >= 12
    ints = plan.arena.view(torch.int16 if dtype == BF16 else torch.int32)
    pattern = 0x7FC1 if dtype == BF16 else 0x7FC00001     # a NaN no kernel produces
    ints.fill_(pattern)
    plan.run()
    torch.cuda.synchronize()
    want = pack_images(plan, dtype)
    covered = torch.zeros(plan.arena.numel(), dtype=torch.bool)
    for name, (off, rows, pitch) in plan._images.items():
        assert_bits(plan[name], want[name], f"image {name}")      # columns [cols, pitch) included: zero
        covered[off:off + rows * pitch] = True
    assert not bool(covered.all()), "no gap between the images to watch"
    assert bool((ints.cpu()[~covered] == pattern).all()), "arena words between the images were written"
    # the pad columns, said once more in the terms of the declarations
    assert bool((plan["m70"][:, 45:] == 0).all()) and bool((plan["m70.t"][:, 70:] == 0).all())


def test_optimizer_argument_checks_return_before_any_launch():
    from nemo_amd import _lib
    L = _lib.lib
    fresh_ops()
    buf = Guarded(4096, torch.uint8)
    p = buf.t.data_ptr()
    rc = {
        "adamw n % 4": L.mi355x_adamw_step(p, p, p, p, 6, 1e-3, 0.9, 0.98, 1e-8, 0.0, 1, 1.0, None),
        "adamw step 0": L.mi355x_adamw_step(p, p, p, p, 8, 1e-3, 0.9, 0.98, 1e-8, 0.0, 0, 1.0, None),
        "adamw ema_decay > 1": L.mi355x_adamw_step_ex(p, p, p, p, 8, 1e-3, 0.9, 0.98, 1e-8, 0.0, 1, 1.0, None, p, 1.5, None),
        "grad_sumsq n % 4": L.mi355x_grad_sumsq(p, 6, p, None),
        "clip_coef nbuf 0": L.mi355x_clip_coef(p, 0, 1.0, 1.0, p, None),
        "clip_coef max_norm 0": L.mi355x_clip_coef(p, 1, 1.0, 0.0, p, None),
        "pack_weights no entries": L.mi355x_pack_weights(p, 0, 1, 1, None),
        "pack_weights no tiles": L.mi355x_pack_weights(p, 1, 0, 1, None),
        "fill_f32 n 0": L.mi355x_fill_f32(p, 0, 1.0, None),
    }
    torch.cuda.synchronize()
    assert all(v == 1 for v in rc.values()), {k: v for k, v in rc.items() if v != 1}
    assert buf.untouched(), "an argument error was returned after something had been written"


# ------------------------------------------------------------------------------------------------ what the host test reads
def grid_stride_vectors():
    """kernel -> (items of its largest case in this file, the launcher's block cap)"""
    return {"adamw": (max(c[0] for c in ADAMW_CASES) // 4, EO.GRID_CAP["adamw"]),
            "sumsq": (max(SUMSQ_N) // 4, EO.GRID_CAP["sumsq"]),
            "fill_f32": (max(FILL_N), EO.GRID_CAP["fill_f32"])}


# ------------------------------------------------------------------------------------------------ reference-error measurement
def measure_reference_errors():
    """the float32 CPU figures the header quotes (no GPU needed)"""
    worst, worst32 = {}, {}
    for case in ADAMW_CASES:
        for tab, flag in ((worst, False), (worst32, True)):
            for k, e in adamw_errors(case, adamw_float32(case, flag))[0].items():
                if e > tab.get(k, (0.0, None))[0]:
                    tab[k] = (e, adamw_id(case))
    for k, (e, where) in worst.items():
        print(f"adamw {k}: float32 restatement, worst element {e:.3e} ({where}) -> x4 = {4 * e:.3e}")
    e, where = worst32["dp"]
    print(f"adamw dp with `1.f - powf(beta, step)` bias corrections: {e:.3e} ({where})")
    for case in ADAMW_CASES:
        if case[:2] in [(4 * 257, s) for s in (1, 2, 3, 5, 10)] and case[3:] == (1e-2, 1e-8, False, None):
            print(f"   {adamw_id(case)}: dp {adamw_errors(case, adamw_float32(case, True))[0]['dp']:.3e}")
    w = 0.0
    for n in SUMSQ_N:
        for k in range(3):
            g = sumsq_input(n, k)
            w = max(w, sumsq_err(SUMSQ_PRE[0] + float(torch.sum(g * g)), SUMSQ_PRE[0], (g,)))
    print(f"grad_sumsq, float32 torch.sum(g * g), worst: {w:.3e} -> x8 = {8 * w:.3e}")


if __name__ == "__main__":
    measure_reference_errors()
