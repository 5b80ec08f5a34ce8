"""-m gpu: the epilogue of the phase-staggered 256x256 GEMM structure (gemm_bf16_v8_kernel, `mi355x_gemm_config(8, 2)`), generic and
specialised rounds (`mi355x_gemm_config(10, .)`: per-launch element types / swish_g / dropout as template parameters, window reads
with counted waits).  Every epilogue kind the structure serves, with and without dropout, bf16 and f32 outputs:
  * bit-identical, `aux_out` included, to the lock-step 256x256 structure on the same operands -- same products in the same k
    order, same epilogue arithmetic; the dropout mask is a pure function of (key, element index), so it is part of the identity;
  * three launches into fresh outputs, all equal (a stale window or a value carried from one tile to the next would differ);
  * without dropout and with f32 outputs: rel_l2 < 2e-6 against the same epilogue applied in fp32 to the fp32 product of the
    bf16-rounded operands (the bound tests/test_gemm_v8_gpu.py uses for this structure).  Narrower than "every kind, with and
    without dropout": bf16 outputs carry 2^-9 per element and cannot meet 2e-6, and the dropout mask is defined by the kernels' own
    hash -- both are held bit for bit to the lock-step structure, whose f32 no-dropout outputs meet the bound, instead;
  * every launch is checked to have taken the intended path (`mi355x_gemm_config(11, 0)`: structure and specialised round of the
    last launch): the phase-staggered kernel, and with key 10 on the specialised round for the bf16 kinds that have one.
Shapes: two and eight K-tiles, partial row tiles (M = 300, 513), a partial column tile (N = 264), and 272 tiles on 256 CUs at
K = 128 (workgroups of one and of two tiles).  K = 64 is ONE K-tile: the structure needs two (its pipeline is primed two half-tile
rounds deep), the dispatcher sends such launches to the older structures even when forced, and the two K = 64 cases only check that
fall-back (path 0) against the lock-step structure."""
import pytest
import torch

pytestmark = pytest.mark.gpu

dev = "cuda"
bf16 = torch.bfloat16

KINDS = ("store", "swish", "swish_g", "resid", "dswish", "dswish_g", "relu_mask", "mul_pos")


def ops():
    from nemo_amd import ops as _ops
    return _ops


def rel_l2(a, b):
    a, b = a.detach().float(), b.detach().float()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _sig(x):
    return 1.0 / (1.0 + torch.exp(-x))


@pytest.mark.parametrize("M,N,K", [(512, 512, 64), (512, 512, 128), (768, 512, 512), (300, 512, 512), (513, 768, 128),
                                   (600, 264, 128), (4352, 4096, 64), (4352, 4096, 128)])
def test_every_epilogue_kind_matches_the_lock_step_structure_and_fp32(M, N, K):
    o = ops()
    g = torch.Generator(device=dev).manual_seed(M * 7 + N * 3 + K)
    A = (torch.rand(M, K, device=dev, generator=g) * 2 - 1).to(bf16)
    W = ((torch.rand(N, K, device=dev, generator=g) * 2 - 1) * 0.1).to(bf16)
    bias = torch.randn(N, device=dev, generator=g)
    res = torch.randn(M, N, device=dev, generator=g)          # EPI_RESID: f32 aux_in
    pre = torch.randn(M, N, device=dev, generator=g)          # pre-activation / stored gradient factor / gate
    rows_inner, rows_per_b = 4, 128                           # ReLU + time mask: M rows = batches of 32 frames x 4
    nb = (M + rows_per_b - 1) // rows_per_b
    row_len = torch.randint(1, 33, (nb,), device=dev, generator=g).to(torch.int64)
    prod = A.float() @ W.float().t()
    frame = (torch.arange(M, device=dev) % rows_per_b) // rows_inner
    live = (frame < row_len[torch.arange(M, device=dev) // rows_per_b])[:, None]

    def run(kind, cdt, drop):
        aux_dt = cdt
        c = torch.full((M, N), float("nan"), device=dev, dtype=cdt)
        kw = dict(drop=drop) if drop is not None else {}
        if kind == "store":
            o.gemm(A, W, c, M, N, K, K, K, N, bias=bias, alpha=0.5, **kw)
            return (c,)
        if kind in ("swish", "swish_g"):
            h = torch.full((M, N), float("nan"), device=dev, dtype=aux_dt)
            o.gemm(A, W, c, M, N, K, K, K, N, bias=bias, epi=o.EPI_SWISH_DROP if kind == "swish" else o.EPI_SWISH_DROP_G, aux_out=h, **kw)
            return (c, h)
        if kind == "resid":
            o.gemm(A, W, c, M, N, K, K, K, N, bias=bias, alpha=0.5, epi=o.EPI_RESID, aux_in=res, **kw)
            return (c,)
        if kind in ("dswish", "dswish_g"):
            o.gemm(A, W, c, M, N, K, K, K, N, epi=o.EPI_DSWISH if kind == "dswish" else o.EPI_DSWISH_G, aux_in=pre.to(aux_dt), **kw)
            return (c,)
        if kind == "relu_mask":
            o.gemm(A, W, c, M, N, K, K, K, N, bias=bias, epi=o.EPI_RELU_MASK, row_len=row_len, rows_per_b=rows_per_b, rows_inner=rows_inner)
            return (c,)
        o.gemm(A, W, c, M, N, K, K, K, N, epi=o.EPI_MUL_POS, aux_in=pre.to(aux_dt))
        return (c,)

    def want_path(kind, cdt, drop, spec):
        if K < 128:
            return 0           # one K-tile: not this structure
        if not spec or cdt != bf16:
            return 800
        if kind == "swish_g":
            return 801 if drop is not None else 802
        return {"dswish_g": 803, "store": 804 if drop is None else 800}.get(kind, 800)

    def fp32_ref(kind):
        v = prod + bias
        if kind == "store":
            return (0.5 * v,)
        if kind == "swish":
            return (v * _sig(v), v)
        if kind == "swish_g":
            s = _sig(v)
            return (v * s, v * s * (1 - s) + s)
        if kind == "resid":
            return (res + 0.5 * v,)
        if kind == "dswish":
            s = _sig(pre)
            return (prod * (s * (1 + pre * (1 - s))),)
        if kind == "dswish_g":
            return (prod * pre,)
        if kind == "relu_mask":
            return (torch.where(live & (v > 0), v, torch.zeros_like(v)),)
        return (torch.where(pre > 0, prod, torch.zeros_like(prod)),)

    for kind in KINDS:
        for cdt in (bf16, torch.float32):
            for drop in (None, o.Dropout(0.1, 11, 5)):
                if drop is not None and kind in ("relu_mask", "mul_pos"):
                    continue  # (these two kinds have no dropout)
                with ops().gemm_modes(k8=0, k4=2, k5=0, k6=0):   # the lock-step 256x256 structure
                    want = run(kind, cdt, drop)
                    assert o.gemm_config(11, 0) == 0
                for spec in (0, 1):                    # the generic round everywhere / specialised rounds where the dispatcher has one
                    with ops().gemm_modes(k8=2, k5=0, k10=spec):
                        for rep in range(3):
                            got = run(kind, cdt, drop)
                            path = o.gemm_config(11, 0)
                            assert path == want_path(kind, cdt, drop, spec), (kind, cdt, drop is not None, spec, path)
                            torch.cuda.synchronize()
                            for w_, g_ in zip(want, got):
                                assert torch.equal(w_, g_), (kind, cdt, drop is not None, spec, rep,
                                                             (w_.float() - g_.float()).abs().max().item())
                if drop is None and cdt == torch.float32:
                    for r_, g_ in zip(fp32_ref(kind), got):   # (got: the last launch, key 10 on)
                        e = rel_l2(g_, r_)
                        print(f"M={M} N={N} K={K} {kind}: rel_l2 vs fp32 {e:.3e}")
                        assert e < 2e-6, (kind, e)
