"""elementwise.hip / optim.hip without a GPU: the float64 closed forms of tests/elementwise_oracle.py against a literal scalar
transcription of drop_mask(), torch.autograd through the reference's literal rel_shift, the reference's context masks,
torch.optim.AdamW + clip_grad_norm_ + the _foreach EMA, and torch permute / reshape / cat for the weight images (what makes them a
reference for tests/test_elementwise_kernels_gpu.py and tests/test_optim_kernels_gpu.py) -- and the proof that the case tables
of those two files reach every kernel path."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import elementwise_oracle as EO  # noqa: E402
import test_elementwise_kernels_gpu as EK  # noqa: E402  (case tables only: nothing in it touches a device at import)
import test_optim_kernels_gpu as OP  # noqa: E402
from oracle import conformer_ref as R  # noqa: E402

F64 = torch.float64
U32 = 0xFFFFFFFF


def _rel(a, b):
    return ((a - b).abs().max() / (b.abs().max() + 1e-300)).item()


# ------------------------------------------------------------------------------------------------ dropout mask
def _mix32(x):
    x ^= x >> 16; x = (x * 0x7feb352d) & U32; x ^= x >> 15; x = (x * 0x846ca68b) & U32; x ^= x >> 16
    return x


def scalar_drop_mask(key, threshold, idx):
    """drop_mask() of common.h, line by line, on Python integers: True = kept"""
    if threshold == 0:
        return True
    s = _mix32((_mix32(((idx >> 3) ^ key) & U32) + 0x9E3779B9 * (key | 1)) & U32) | 1
    for _ in range((idx & 7) + 1):
        s ^= (s << 13) & U32; s ^= s >> 17; s ^= (s << 5) & U32
    return s >= threshold


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("start", [0, 3, 4, 8, 8 * 1000 + 5, 2 ** 32 - 5])   # 2^32 - 5: the index wraps like the kernel's uint32
def test_keep_mask_is_the_scalar_drop_mask(start, p):
    drop = EO.Drop(p, 7, 21)
    n = 37                                           # crosses four group boundaries
    got = EO.keep_mask(drop, start, n)
    want = torch.tensor([scalar_drop_mask(drop.key, drop.threshold, (start + k) & U32) for k in range(n)])
    assert torch.equal(got, want)
    assert 0 < int(got.sum()) < n
    w = 0x1234ABCD                                   # the registered step word is added to the key
    want = torch.tensor([scalar_drop_mask((drop.key + w) & U32, drop.threshold, (start + k) & U32) for k in range(n)])
    assert torch.equal(EO.keep_mask(drop, start, n, step_word=w), want)
    assert bool(EO.keep_mask(EO.Drop(0.0), start, n).all())


def test_drop_restates_the_wrappers_dropout():
    from nemo_amd import ops
    for p, seed, site in ((0.0, 1, 2), (0.1, 7, 21), (0.5, 123456, 9), (0.2, 3, 5)):
        a, b = EO.Drop(p, seed, site), ops.Dropout(p, seed, site)
        assert (a.key, a.threshold, a.scale) == (b.key, b.threshold, b.scale)


# ------------------------------------------------------------------------------------------------ rel-pos softmax
def rel_shift(x):
    """multi_head_attention.py:259-270, literally: pad one column on the left, view, drop the first row, view back"""
    b, h, qlen, pos_len = x.size()
    x = torch.nn.functional.pad(x, pad=(1, 0))
    x = x.view(b, h, -1, qlen)
    x = x[:, :, 1:].view(b, h, qlen, pos_len)
    return x


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("ctx", [(0, -1, -1), (1, 3, 1), (2, 5, 2)])
@pytest.mark.parametrize("T,lens", [(1, (1, 0, 4)), (5, (5, 3, 0)), (33, (33, 17, 40))])
def test_softmax_closed_forms_equal_autograd_through_the_literal_rel_shift(T, lens, ctx, p):
    H, B, scale = 2, len(lens), 0.3
    g = torch.Generator().manual_seed(10 * T + ctx[0])
    ac = torch.randn(H, B, T, T, generator=g, dtype=F64).requires_grad_(True)
    bdf = torch.randn(H, B, T, 2 * T - 1, generator=g, dtype=F64).requires_grad_(True)
    dpd = torch.randn(H, B, T, T, generator=g, dtype=F64)
    ok = EO.relpos_allowed(lens, B, T, ctx)[None]
    keep = EO.keep_mask(EO.Drop(p, 3, 5), 0, H * B * T * T).view(H, B, T, T) if p > 0 else torch.ones(H, B, T, T, dtype=torch.bool)
    scores = ((ac + rel_shift(bdf)[..., :T]) * scale).masked_fill(~ok, -10000.0)
    s_ref = torch.softmax(scores, -1).masked_fill(~ok, 0.0)
    (s_ref * keep / (1 - p) * dpd).sum().backward()

    s = EO.relpos_softmax_fwd(ac, bdf, lens, T, scale, ctx)
    assert _rel(s, s_ref.detach()) < 1e-12
    assert bool((s[~ok.expand_as(s)] == 0).all())
    ds, dbdf = EO.relpos_softmax_bwd(dpd, s, T, 2 * T - 1, scale, keep, p)
    assert _rel(ds, ac.grad) < 1e-12 and _rel(dbdf, bdf.grad) < 1e-12
    # a wider dbdf: the same band, zeros beyond column 2T - 2
    ds2, wide = EO.relpos_softmax_bwd(dpd, s, T, 2 * T + 6, scale, keep, p)
    assert torch.equal(ds2, ds) and torch.equal(wide[..., :2 * T - 1], dbdf) and bool((wide[..., 2 * T - 1:] == 0).all())


@pytest.mark.parametrize("style", [1, 2])
def test_context_predicate_is_the_reference_mask(style):
    name = {1: "regular", 2: "chunked_limited"}[style]
    for T in (1, 5, 17):
        for left in (-1, 0, 3, 8, 12):
            for right in (-1, 0, 3):
                cfg = types.SimpleNamespace(att_context_size=[left, right], att_context_style=name)
                assert torch.equal(EO.ctx_allows(style, left, right, T), R.context_mask(cfg, T)), (style, T, left, right)
    assert bool(EO.ctx_allows(0, 3, 3, 9).all())


# ------------------------------------------------------------------------------------------------ AdamW, clip, EMA
@pytest.mark.parametrize("beta2", [0.98, 0.999])
@pytest.mark.parametrize("wd,eps", [(0.0, 1e-8), (1e-2, 1e-3)])
def test_adamw_closed_form_equals_torch_adamw_with_clip_and_ema(beta2, wd, eps):
    n, lr, b1, decay, max_norm, grad_scale = 64, EO.f32(3e-3), EO.f32(0.9), EO.f32(0.999), 0.7, 0.5
    b2, wd, eps = EO.f32(beta2), EO.f32(wd), EO.f32(eps)
    g = torch.Generator().manual_seed(5)
    p0 = torch.randn(n, generator=g, dtype=F64)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    ema_ref = [p0.clone()]
    p, m, v, ema = p0.clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64), p0.clone()
    clipped = 0
    for step in range(1, 7):
        grad = torch.randn(n, generator=g, dtype=F64) * (3.0 if step % 2 else 0.01)
        ref.grad = grad * grad_scale
        total = torch.nn.utils.clip_grad_norm_([ref], max_norm)
        opt.step()
        torch._foreach_mul_(ema_ref, decay); torch._foreach_add_(ema_ref, [ref.detach()], alpha=1 - decay)
        coef, norm = EO.clip_coef([grad.square().sum()], grad_scale, max_norm)
        assert abs(norm - total.item()) <= 1e-12 * norm
        clipped += coef < 1
        p, m, v, ema = EO.adamw_step(p, grad, m, v, lr, b1, b2, eps, wd, step, grad_scale, coef, ema, decay)
        assert _rel(p, ref.detach()) < 1e-12 and _rel(ema, ema_ref[0]) < 1e-12, step
        st = opt.state[ref]
        assert _rel(m, st["exp_avg"]) < 1e-12 and _rel(v, st["exp_avg_sq"]) < 1e-12
    assert 0 < clipped < 6                           # both sides of max_norm were seen
    assert EO.clip_coef([0.0, 0.0], 0.5, 1.0) == (1.0, 0.0)


def test_bias_corrections_in_float32_lose_the_first_steps():
    """why adamw_launch takes them in double: with beta2 = 0.999 the float32 `1 - beta2^step` is tens of ulps off at steps 2 - 5"""
    import numpy as np
    f = np.float32
    for b2, steps, floor, ceil in ((0.999, (2, 3, 5), 1e-6, 1e-5), (0.98, (1, 2, 3, 5, 10), 0.0, 2.5e-7)):
        for step in steps:
            got = float(np.sqrt(f(1) - f(float(f(b2)) ** step)))        # a correctly rounded powf, then float32 throughout
            e = abs(got - EO.bias_corrections(0.9, b2, step)[1]) / EO.bias_corrections(0.9, b2, step)[1]
            assert floor <= e < ceil, (b2, step, e)


# ------------------------------------------------------------------------------------------------ weight images
def test_pack_reference_equals_torch_for_every_declaration():
    from nemo_amd.packing import PackPlan
    w = OP.pack_sources("cpu")
    plan = OP.declare_pack(PackPlan(torch.float32, "cpu"), w)
    img = OP.pack_images(plan, torch.float32)

    def padded(t):
        out = torch.zeros(t.shape[0], (t.shape[1] + 7) // 8 * 8)
        out[:, :t.shape[1]] = t
        return out

    cat = torch.cat(w["cat"])
    conv = w["conv"].permute(0, 2, 3, 1).reshape(16, 72)          # [co, (kh, kw, ci)]
    fc = w["fc"].view(24, 8, 5).permute(0, 2, 1).reshape(24, 40)  # column c * F + f -> f * C + c
    want = {"m64": w["m64"], "m70": w["m70"], "m200": w["m200"], "mis": w["mis"], "cat": cat, "conv": conv, "fc": fc}
    assert set(img) == set(want) | {k + ".t" for k in want}
    for k, t in want.items():
        assert torch.equal(img[k], padded(t)), k
        assert torch.equal(img[k + ".t"], padded(t.t())), k + ".t"
        assert tuple(img[k].shape) == (t.shape[0], plan.pitch(k))
    # EO.pack_image on its own: the formula of the PackEntry comment
    src = torch.arange(2 * 3 * 5 * 7, dtype=torch.float32)
    got = EO.pack_image(src, 6, 35, nr2=3, nc2=7, sr1=105, sr2=35, sc1=7, sc2=1)
    assert torch.equal(got, src.view(6, 35))


# ------------------------------------------------------------------------------------------------ coverage of the case tables
def test_pack_cases_reach_every_path_of_the_kernel():
    from nemo_amd.packing import PackPlan
    plan = OP.declare_pack(PackPlan(torch.bfloat16, "cpu"), OP.pack_sources("cpu"))
    entries = OP.pack_entries(plan)
    assert len(entries) >= 12
    paths = {e["name"] + f"#{k}": [EO.pack_path(e, t) for t in EO.pack_tiles(e["rows"], e["cols"])] for k, e in enumerate(entries)}
    assert {p for ps in paths.values() for p in ps} == set(EO.PACK_PATHS)
    first, last = list(paths.values())[0], list(paths.values())[-1]
    assert first == ["vec_colfast"] and last == ["vec_rowfast"]      # one-tile entries at both ends of the binary search
    by = {k.split("#")[0]: v for k, v in paths.items() if not k.startswith("cat")}
    assert set(by["m70"]) == set(by["m70.t"]) == {"scalar_plain"}        # ragged, stride % 4 != 0
    assert set(by["m200"]) == {"vec_colfast", "scalar_plain"} and set(by["m200.t"]) == {"vec_rowfast", "scalar_plain"}
    assert set(by["mis"]) == set(by["mis.t"]) == {"scalar_plain"}        # whole tiles, stride % 4 == 0: only the address is off
    aligned = [dict(e, src_addr=0) for e in entries if e["name"].startswith("mis")]
    assert {EO.pack_path(e, (0, 0)) for e in aligned} == {"vec_colfast", "vec_rowfast"}
    assert all(set(by[k]) == {"scalar_split"} for k in ("conv", "conv.t", "fc", "fc.t"))
    assert all(r.shape[0] % 8 == 0 for r in OP.pack_sources("cpu")["cat"])


def test_add2_colsum_cases_reach_every_thread_layout():
    shapes = {d: EO.add2_colsum_shape(d) for d, _, _ in EK.A2C_CASES}
    assert set(shapes) == {8, 24, 176, 512, 2048, 2056}
    assert any(idle > 0 for _, _, idle, _ in shapes.values())
    assert any(RS > 32 for _, RS, _, _ in shapes.values())        # more row lanes than the 32 rows of a block
    assert any(RS == 1 for _, RS, _, _ in shapes.values())
    assert {passes for _, _, _, passes in shapes.values()} == {1, 2}
    assert shapes[2056][3] == 2 and shapes[2048] == (256, 1, 0, 1) and shapes[24] == (3, 85, 1, 1)
    assert {M for _, M, _ in EK.A2C_CASES} == {1, 31, 32, 33, 1003}
    assert {ldm for _, _, ldm in EK.A2C_CASES} == {1, 3}


def test_every_grid_stride_kernel_has_a_case_with_a_second_trip():
    assert EO.strides(1, 4096) == 1 and EO.strides(4096 * 256, 4096) == 1 and EO.strides(4096 * 256 + 1, 4096) == 2
    ek = EK.grid_stride_vectors()
    assert set(ek) == {"drop_scale_cast", "rows_pack", "qbias", "add2", "row_scale"}
    for name, nv in ek.items():
        assert EO.strides(nv, EO.GRID_CAP["elementwise"]) >= 2, name
    op = OP.grid_stride_vectors()
    assert set(op) == {"adamw", "sumsq", "fill_f32"}
    for name, (nv, cap) in op.items():
        assert EO.strides(nv, cap) >= 2, name
    # and the small cases stay on the first trip
    assert EO.strides(8 * 257 // 8, 4096) == 1 and EO.strides(4 * 257 // 4, 8192) == 1


def test_softmax_cases_reach_every_edge():
    fwd, bwd = EK.SM_FWD_CASES, EK.SM_BWD_CASES
    for cases in (fwd, bwd):
        assert {c[2] for c in cases} == {1, 45, 63, 64, 65, 129, 1024}
        for T in {c[2] for c in cases}:
            assert {(c[3], c[4]) for c in cases if c[2] == T} >= {(T, 2 * T - 1), ((T + 63) // 64 * 64, 2 * T + 6)}
        assert all(c[3] <= 1024 for c in cases) and all((c[0], c[1]) == (1, 1) for c in cases if c[2] == 1024)
        assert any(c[0] * c[1] * c[2] % 4 for c in cases)            # the last workgroup holds fewer than 4 rows
        assert max((c[2] + 63) // 64 for c in cases) == 16           # every register slot of a lane
    assert {c[5] for c in fwd} == {torch.float32, torch.bfloat16}
    assert {c[6] for c in fwd if c[6][0] == 1} == {(1, 4, 0), (1, -1, 2), (1, 3, -1), (1, 0, 0)}
    assert {c[6] for c in fwd if c[6][0] == 2} == {(2, 8, 3), (2, -1, 3), (2, 6, -1), (2, 7, 3)}
    assert all(c[2] == 45 for c in fwd if c[6][0])
    assert {(c[5], c[6]) for c in bwd} == set(EK.PAIRS)
    lens = EK.sm_lens(45, 4)
    assert 0 in lens and 1 in lens and 45 in lens and max(lens) > 45
    # the style-2 windows of the table differ from their `<` neighbours: a mask off by one chunk cannot pass
    for style, left, right in EK.SM_CTX:
        if style == 2 and right >= 0 and left >= 0:
            assert not torch.equal(EO.ctx_allows(2, left, right, 45), EO.ctx_allows(2, left - (right + 1), right, 45))


def test_drop_scale_cast_cases():
    assert {(c[0], c[1]) for c in EK.DSC_CASES} == set(EK.PAIRS)
    assert {c[2] for c in EK.DSC_CASES} == {8, 8 * 257, 8 * (4096 * 256 + 3)}
    assert {ap for c in EK.DSC_CASES for ap in c[3]} == {(a, p) for a in (1.0, 0.5, 22.6) for p in (0.0, 0.1, 0.5)}
