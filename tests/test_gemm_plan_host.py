"""CPU-side pin of the GEMM dispatcher (run without a GPU): `ops.gemm_plan` -- mi355x_gemm_plan: the argument checks and the plan of
mi355x_gemm without the launch -- over a fixed list of descriptors and knob settings, compared row by row with
tests/data/gemm_plan_golden.json.  The golden table was recorded from the dispatcher as it was BEFORE it was split into
gemm_fill / gemm_plan / gemm_launch (every launch site of the old mi355x_gemm instrumented to record what it was about to launch), so
it pins the dispatch rules themselves: a row changes only when a rule or a default changes, and then the table is recorded again from
a commit whose step time was measured.  Pointers are fake, suitably aligned integers; nothing dereferences them.

Also here: mi355x_gemm_config returns the effective previous value, and ops.gemm_modes restores it."""
import ctypes as C
import json
import os

import pytest

from nemo_amd import ops
from nemo_amd._lib import ConvGather, GemmDesc, RowMap

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "gemm_plan_golden.json")
F32, BF16 = ops.F32, ops.BF16
# out[0] of mi355x_gemm_plan: enum GemmKernel of csrc/gemm.hip, the rows of gemm_launch's table
KERNELS = [
    "gemm_bf16_kernel<0,0>", "gemm_bf16_kernel<0,1>", "gemm_bf16_kernel<1,1>", "gemm_bf16_kernel<1,0>",
    "gemm_bf16_v2_kernel<0,0>", "gemm_bf16_v2_kernel<0,0,reg>", "gemm_bf16_v2_kernel<0,1>", "gemm_bf16_v2_kernel<1,1>",
    "gemm_bf16_v4_kernel<0,0,0>", "gemm_bf16_v4_kernel<0,0,1>", "gemm_bf16_v4_kernel<0,1,0>", "gemm_bf16_v4_kernel<1,1,0>",
    "gemm_bf16_v4_kernel<1,1,2>", "gemm_bf16_v6_kernel<0>", "gemm_bf16_v6_kernel<1>",
    "gemm_bf16_v8_kernel<0,nt>", "gemm_bf16_v8_kernel<1,nt>", "gemm_bf16_v8_kernel<0,tn>", "gemm_bf16_v8_kernel<2,tn>",
    "gemm_bf16_v8_kernel<es1>", "gemm_bf16_v8_kernel<es2>", "gemm_bf16_v8_kernel<es3>", "gemm_bf16_v8_kernel<es4>",
    "gemm_bf16_v8_kernel<half>",
    "gemm_bf16_v5_kernel<store>", "gemm_bf16_v5_kernel<swish_drop>", "gemm_bf16_v5_kernel<resid>", "gemm_bf16_v5_kernel<dswish>",
    "gemm_f32_kernel", "gemm_f32_mfma_kernel",
]
PATHS = {0, 800, 801, 802, 803, 804, 810}
A_, B_, C_, AUXI, AUXO, BIAS, ROWLEN = (0x10000000 * (i + 1) for i in range(7))  # 32-byte aligned "device pointers"
_keep = []  # the gather / row-map structs the descriptors point to


def up8(n):
    return (n + 7) & ~7


def desc(M, N, K, ta=0, tb=0, dt=BF16, cdt=BF16, epi=0, aux_in=None, aux_out=None, drop=0, atomic=0, splitk=1, batch=1, ldc=None,
         csc=1, bias=1, gather=None, rowmap=None, **over):
    """a descriptor the way ops.gemm fills it: dense operands with the smallest legal pitches unless `over` says otherwise"""
    d = GemmDesc()
    d.A, d.B, d.C = A_, B_, C_
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb = (up8(M) if ta else up8(K)), (up8(N) if tb else up8(K))
    d.ldc = ldc if ldc is not None else up8(N) * csc
    d.c_col_stride = csc
    d.transA, d.transB, d.in_dtype, d.c_dtype = ta, tb, dt, cdt
    d.batch = d.nb0 = batch
    if batch > 1:
        d.sA0, d.sB0, d.sC0 = up8(M) * up8(K), up8(N) * up8(K), M * d.ldc
    d.bias = BIAS if bias else 0
    d.alpha = 1.0
    d.epilogue, d.atomic, d.splitk = epi, atomic, splitk
    if aux_in is not None:
        d.aux_in, d.aux_in_dtype = AUXI, aux_in
    if aux_out is not None:
        d.aux_out, d.aux_out_dtype = AUXO, aux_out
    d.ldaux = d.ldc
    d.drop_key, d.drop_threshold, d.drop_scale = (0x1234, 0x19999999, 1.0 / 0.9) if drop else (0, 0, 1.0)
    if epi == ops.EPI_RELU_MASK:
        d.row_len, d.rows_per_b, d.rows_inner = ROWLEN, M, 1
    if gather is not None:
        g = ConvGather()
        g.nI, g.nJ, g.SI, g.SJ, g.C, g.si, g.sj = (gather[k] for k in ("nI", "nJ", "SI", "SJ", "C", "si", "sj"))
        g.ntaps, g.operand = len(gather["taps"]), gather.get("operand", 0)
        for t, (di, dj) in enumerate(gather["taps"]):
            g.di[t], g.dj[t] = di, dj
        _keep.append(g)
        d.gather = C.cast(C.pointer(g), C.c_void_p)
    if rowmap is not None:
        r = RowMap()
        r.nI, r.nJ, r.OI, r.OJ, r.si, r.sj, r.oi, r.oj = rowmap
        _keep.append(r)
        d.rowmap = C.cast(C.pointer(r), C.c_void_p)
    for k, v in over.items():
        setattr(d, k, v)
    return d


MS = [8, 191, 192, 300, 3000, 8032, 16032, 32768]
NS = [64, 95, 96, 128, 129, 324, 512, 520, 1024, 1536, 2048, 4096]
KS = [8, 64, 128, 192, 512, 576, 768, 1024, 2048, 8192]
LAYOUTS = [(0, 0), (0, 1), (1, 1), (1, 0)]
TAPS9 = [(kh - 1, kw - 1) for kh in range(3) for kw in range(3)]


def epilogue_variants():
    """every epilogue 0..7 with the aux / C dtypes and the dropout switch a decision depends on"""
    E = ops
    out = []
    for drop in (0, 1):
        out += [dict(epi=E.EPI_STORE, cdt=c, drop=drop) for c in (BF16, F32)]
        out += [dict(epi=e, aux_out=a, drop=drop) for e in (E.EPI_SWISH_DROP, E.EPI_SWISH_DROP_G) for a in (BF16, F32)]
        out += [dict(epi=E.EPI_RESID, cdt=c, aux_in=F32, drop=drop) for c in (BF16, F32)]
        out += [dict(epi=e, aux_in=a, drop=drop) for e in (E.EPI_DSWISH, E.EPI_DSWISH_G) for a in (BF16, F32)]
    out += [dict(epi=E.EPI_RELU_MASK), dict(epi=E.EPI_MUL_POS, aux_in=BF16), dict(epi=E.EPI_STORE, bias=0), dict(epi=E.EPI_STORE, cdt=F32, bias=0)]
    return out


def conv_descs():
    """the conv2 launches of ConvSubsampling (modules/conformer_encoder.py): gathered-A forward, gathered-B weight gradient, the
    gathered + row-mapped input gradient of one parity class; a row-mapped dense problem"""
    out = []
    for Bz, T1, F1, Cc in ((16, 200, 40, 256), (64, 400, 40, 256)):
        T2, F2 = T1 // 2, F1 // 2
        M2 = Bz * T2 * F2
        geo = dict(nI=T2, nJ=F2, SI=T1, SJ=F1, C=Cc, si=2, sj=2, taps=TAPS9)
        out.append(("conv2_fwd", desc(M2, Cc, 9 * Cc, epi=ops.EPI_RELU_MASK, gather=geo, lda=Cc)))
        for sk in (1, 4):
            out.append(("conv2_wgrad", desc(Cc, Cc, M2, ta=1, tb=1, cdt=F32, atomic=1, splitk=sk, batch=9, csc=9, bias=0, ldc=9 * Cc,
                                            gather=dict(geo, operand=1), sA0=0, sB0=0, sC0=1)))
        nI, nJ = T1 // 2, F1 // 2
        out.append(("conv2_dgrad", desc(Bz * nI * nJ, Cc, 4 * Cc, epi=ops.EPI_MUL_POS, aux_in=BF16, bias=0, lda=Cc,
                                        gather=dict(nI=nI, nJ=nJ, SI=T2, SJ=F2, C=Cc, si=1, sj=1, taps=[(0, 0), (0, 1), (1, 0), (1, 1)]),
                                        rowmap=(nI, nJ, T1, F1, 2, 2, 1, 1))))
        out.append(("rowmap", desc(Bz * nI * nJ, 512, 512, rowmap=(nI, nJ, T1, F1, 2, 2, 0, 1))))
    return out


def rejected_descs():
    """one list per kind of descriptor mi355x_gemm must reject"""
    small = dict(nI=4, nJ=4, SI=8, SJ=8, C=256, si=2, sj=2, taps=TAPS9)
    return {
        "bad alignment": [desc(300, 512, 512, A=A_ + 2), desc(300, 512, 512, B=B_ + 8), desc(300, 512, 512, lda=516),
                          desc(300, 512, 512, ta=1, tb=1, ldb=516), desc(300, 512, 512, batch=4, sA0=300 * 512 + 4)],
        "pitch too small": [desc(300, 512, 512, lda=504), desc(300, 512, 520, ldb=512), desc(300, 512, 512, ta=1, tb=1, lda=296),
                            desc(300, 512, 512, tb=1, ldb=504)],
        "splitk without atomic": [desc(512, 512, 8192, cdt=F32, splitk=4), desc(512, 512, 8192, dt=F32, cdt=F32, splitk=2)],
        "gather on a small problem": [desc(128, 256, 9 * 256, gather=small, lda=256), desc(192, 64, 9 * 64, gather=dict(small, C=64, nI=12), lda=64)],
        "epilogue without its operand": [desc(300, 512, 512, epi=ops.EPI_RESID, cdt=F32), desc(300, 512, 512, epi=ops.EPI_SWISH_DROP),
                                         desc(300, 512, 512, atomic=1)],
    }


def base_descs():
    """(label, descriptor) under the default modes"""
    out = [(f"nt {M}x{N}x{K}", desc(M, N, K)) for M in MS for N in NS for K in KS]
    for ta, tb in LAYOUTS[1:]:
        out += [(f"ta{ta} tb{tb} {M}x{N}x{K}", desc(M, N, K, ta, tb, cdt=F32))
                for M in (8, 191, 192, 3000, 16032) for N in (95, 96, 128, 129, 512, 2048) for K in (8, 128, 512, 8192)]
    out += [(f"f32 ta{ta} tb{tb} {M}x{N}x{K}", desc(M, N, K, ta, tb, dt=F32, cdt=F32, batch=b))
            for ta, tb in LAYOUTS for M in (8, 300) for N in (64, 129) for K in (8, 192) for b in (1, 4)]
    for M, N, K in ((8032, 512, 2048), (300, 324, 512)):
        out += [(f"epi {M}x{N}x{K} {v}", desc(M, N, K, **v)) for v in epilogue_variants()]
    return out + core_descs()


def core_descs():
    """the bf16 descriptors that are also run under every non-default mode"""
    out = [(f"nt {M}x{N}x{K}", desc(M, N, K)) for M in (3000, 8032, 16032) for N in (129, 512, 1536, 2048) for K in (128, 512, 576, 1024)]
    for ta, tb in LAYOUTS[1:3]:
        out += [(f"ta{ta} tb{tb} {M}x{N}x{K}", desc(M, N, K, ta, tb, cdt=F32)) for M in (512, 3000) for N in (324, 2048) for K in (192, 8192)]
    for M, N, K in ((8032, 2048, 512), (8032, 1536, 512), (16032, 512, 1024)):
        out += [(f"epi {M}x{N}x{K} {v}", desc(M, N, K, **v)) for v in epilogue_variants()]
    for M, N, K in ((512, 512, 8192), (192, 129, 2048), (8032, 2048, 576)):
        out += [(f"atomic ta{ta} tb{tb} {M}x{N}x{K} sk{sk}", desc(M, N, K, ta, tb, cdt=F32, atomic=1, splitk=sk, bias=0))
                for ta, tb in ((0, 0), (1, 1), (0, 1)) for sk in (1, 2, 4, 16)]
    out += [(f"batch4 ta{ta} tb{tb} {M}x{N}x{K}", desc(M, N, K, ta, tb, batch=4))
            for ta, tb in LAYOUTS for M, N, K in ((300, 129, 64), (3000, 512, 512), (8032, 1024, 512))]
    for M, K in ((8032, 512), (32768, 1024)):  # N = 324: pitch a multiple of 4, not of 8; interleaved columns
        out += [(f"ldc324 {M}x324x{K} {v}", desc(M, 324, K, ldc=324, **v))
                for v in (dict(), dict(cdt=F32), dict(epi=ops.EPI_DSWISH_G, aux_in=BF16), dict(epi=ops.EPI_RESID, cdt=F32, aux_in=F32))]
        out += [(f"csc2 {M}x{N}x{K}", desc(M, N, K, csc=2, cdt=F32)) for N in (324, 2048)]
    return out + conv_descs()


MODES = [{8: 0}, {8: 2}, {8: 3}, {8: 4}, {8: 5}, {4: 0}, {4: 2}, {5: 0}, {5: 2}, {6: 1}, {6: 2}, {7: 0}, {10: 0}, {9: 3},
         # the older structures only show behind the phase-staggered one
         {8: 0, 4: 2}, {8: 0, 6: 1}, {8: 0, 6: 2}, {8: 2, 10: 0}]


def cases():
    """[(modes, label, descriptor)]: the whole list under the defaults, the bf16 core under every other mode, fp32 under key 3"""
    out = [({}, label, d) for label, d in base_descs()]
    out += [({}, f"rejected: {kind}", d) for kind, ds in rejected_descs().items() for d in ds]
    out += [({3: 0}, label, d) for label, d in base_descs() if d.in_dtype == F32]
    for modes in MODES:
        out += [(modes, label, d) for label, d in core_descs()]
    return out


def rows(plan=ops.gemm_plan, modes_ctx=ops.gemm_modes):
    """[rc, kernel, path, gx, gy, gz, block, lds, delay] per case"""
    out, cur, ctx = [], None, None
    try:
        for modes, _, d in cases():
            if modes != cur:
                if ctx is not None:
                    ctx.__exit__(None, None, None)
                ctx, cur = modes_ctx(modes), modes
                ctx.__enter__()
            rc, o = plan(d)
            out.append([rc] + o)
    finally:
        if ctx is not None:
            ctx.__exit__(None, None, None)
    return out


def test_plan_matches_the_table_recorded_before_the_split():
    golden = json.load(open(GOLDEN))["rows"]
    cs, got = cases(), rows()
    assert 2000 <= len(cs) <= 6000 and len(golden) == len(cs)
    bad = [(modes, label, g, w) for (modes, label, _), g, w in zip(cs, got, golden) if g != w]
    assert not bad, f"{len(bad)} of {len(cs)} rows differ, first: {bad[:5]}"


def test_golden_table_reaches_every_kernel_path_and_rejection():
    golden = json.load(open(GOLDEN))["rows"]
    cs = cases()
    ok = [r for r in golden if r[0] == 0]
    assert {r[1] for r in ok} == set(range(len(KERNELS))), [KERNELS[i] for i in set(range(len(KERNELS))) - {r[1] for r in ok}]
    assert {r[2] for r in ok} == PATHS
    assert all(r[1:] == [0] * 8 for r in golden if r[0] != 0)
    for kind in rejected_descs():
        rcs = [r[0] for (_, label, _), r in zip(cs, golden) if label == f"rejected: {kind}"]
        assert rcs and all(rc == 1 for rc in rcs), (kind, rcs)  # MI_ERR_ARG


def test_plan_needs_no_launch_state():
    """a rejected descriptor leaves `out` alone; key 11 (the last LAUNCH of this thread) is not touched by a plan"""
    before = ops.gemm_config(11, 0)
    rc, out = ops.gemm_plan(desc(8032, 2048, 512))
    assert rc == 0 and out[1] == 804 and ops.gemm_config(11, 0) == before
    rc, out = ops.gemm_plan(GemmDesc())
    assert rc == 1 and out == [0] * 8


def test_gemm_config_returns_the_effective_value_and_gemm_modes_restores_it():
    first = {k: ops.gemm_config(k, 7) for k in range(3, 11)}
    assert all(v >= 0 for v in first.values()), first  # never "-1 = not read yet"
    for k, v in first.items():
        assert ops.gemm_config(k, v) == 7
    with ops.gemm_modes({8: 2, 9: 3, 6: 1}):
        assert [ops.gemm_config(k, v) for k, v in ((8, 2), (9, 3), (6, 1))] == [2, 3, 1]
    with ops.gemm_modes({4: 0}, k8=2, k5=0):  # keys by number and by name, as the GPU tests write them
        assert [ops.gemm_config(k, v) for k, v in ((4, 0), (8, 2), (5, 0))] == [0, 2, 0]
    with ops.gemm_modes(k8=3):
        assert ops.gemm_config(8, 3) == 3
    with pytest.raises(KeyError):
        with ops.gemm_modes({4: 0, 5: 2}):
            raise KeyError("body fails")
    assert {k: ops.gemm_config(k, first[k]) for k in first} == first
    assert ops.gemm_config(11, 12345) == ops.gemm_config(11, 0)  # read only
    assert [ops.gemm_config(k, 1) for k in (-1, 0, 1, 2, 12, 100)] == [-1] * 6
