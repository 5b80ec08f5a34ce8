"""No GPU needed: the case tables of tests/test_gemm_kernels_gpu.py reach what they claim, and tests/gemm_oracle.py restates
mi355x_gemm correctly.

With ops.gemm_plan (the dispatcher without the launch): every one of the 30 kernel ids is reached, each case lands on the id it
names, the edge list is covered per structure family, every exact case's operands keep sum_k |a||b| below 2^22 quanta, no case is
larger than a stated element count.  The grouped kernels have no plan call; their cases are checked against group_plan's rules as
the header of the GPU file states them.

The oracle against independent restatements: the gather against F.conv2d and its gradients, the row map against direct strided
indexing, the two-level batch against an einsum, the epilogues against the fp32 closed forms of test_gemm_epilogues
(tests/test_kernels_gpu.py)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import elementwise_oracle as EO  # noqa: E402
import gemm_oracle as GO  # noqa: E402
import test_gemm_kernels_gpu as GK  # noqa: E402  (case tables only: nothing in it touches a device at import)
from test_gemm_plan_host import KERNELS  # noqa: E402

F64 = torch.float64
NAMES = [c["name"] for c in GK.CASES]


def test_every_kernel_id_is_reached_and_every_case_lands_where_it_says():
    reached = set()
    for c in GK.CASES:
        P = GK.problem(c["name"])
        rc, plan = GK.plan_of(P, GK.fake_addr(P))
        assert rc == 0, c["name"]
        assert KERNELS[plan[0]] == c["kernel"], (c["name"], KERNELS[plan[0]])
        reached.add(plan[0])
        if c["kernel"].startswith("gemm_bf16_v8"):
            assert plan[1] in (800, 801, 802, 803, 804, 810), (c["name"], plan[1])
            for es in "1234":
                assert (plan[1] == 800 + int(es)) == (c["kernel"] == f"gemm_bf16_v8_kernel<es{es}>"), (c["name"], plan[1])
            assert (plan[1] == 810) == (c["kernel"] == "gemm_bf16_v8_kernel<half>")
        else:
            assert plan[1] == 0
        if "v8_delay" in c["edges"]:
            assert plan[7] == c["modes"][9] > 0 and plan[2] * plan[3] * plan[4] > 256
    assert reached == set(range(len(KERNELS))), [KERNELS[i] for i in set(range(len(KERNELS))) - reached]
    print("kernel ids reached:", len(reached), "of", len(KERNELS), "; grouped:", sorted(GK.GROUPED))


def test_split_k_rejects_what_every_slice_would_repeat():
    """found by the v8 split-K case of the GPU file when it still carried a bias: every K slice runs the whole epilogue, so a bias (or
    a residual) came out once per slice.  mi355x_gemm now rejects more than one slice with a bias or with an epilogue that is not
    linear in the sum; a split that clamps to one slice stays legal"""
    from nemo_amd import ops
    from test_gemm_plan_host import F32 as PF32, desc
    assert ops.gemm_plan(desc(300, 264, 320, cdt=PF32, atomic=1, splitk=2, bias=0))[0] == 0
    assert ops.gemm_plan(desc(300, 264, 320, cdt=PF32, atomic=1, splitk=2, bias=1))[0] == 1
    assert ops.gemm_plan(desc(300, 264, 64, cdt=PF32, atomic=1, splitk=2, bias=1))[0] == 0        # one K-tile: one slice
    for epi, kw in ((ops.EPI_RESID, dict(aux_in=PF32)), (ops.EPI_SWISH_DROP, dict(aux_out=PF32)), (ops.EPI_RELU_MASK, {})):
        assert ops.gemm_plan(desc(300, 264, 320, cdt=PF32, atomic=1, splitk=2, bias=0, epi=epi, **kw))[0] == 1, epi
    for epi in (ops.EPI_DSWISH, ops.EPI_MUL_POS, ops.EPI_DSWISH_G):
        assert ops.gemm_plan(desc(300, 264, 320, cdt=PF32, atomic=1, splitk=2, bias=0, epi=epi, aux_in=PF32))[0] == 0, epi


def test_grouped_cases_follow_group_plan_rules():
    """gemm_bf16_grouped_tn_kernel by default; gemm_bf16_grouped_tn8_kernel under key 8 = 3 (or 2) when every N > 128 and
    K >= 4 K-tiles"""
    a, b = GK.GROUPED["grouped_tn"], GK.GROUPED["grouped_tn8"]
    assert a["modes"].get(8, 1) not in (2, 3)
    assert b["modes"][8] == 3 and all(ni > 128 for _, ni in b["shapes"]) and (b["rows"] + 63) // 64 >= 4
    for G in (a, b):   # M and N tails, a K tail, more than one problem, one without a bias gradient
        assert any(no % 256 for no, _ in G["shapes"]) and any(ni % 128 for _, ni in G["shapes"]) and G["rows"] % 64 and len(G["shapes"]) > 2


def test_edges_are_covered_per_structure_family():
    have = {}
    for c in GK.CASES:
        have.setdefault(c["family"], set()).update(c["edges"])
    assert set(have) == set(GK.REQUIRED_EDGES), set(have) ^ set(GK.REQUIRED_EDGES)
    for fam, need in GK.REQUIRED_EDGES.items():
        assert need <= have[fam], (fam, need - have[fam])
    real = {c["family"] for c in GK.CASES if c["kind"] == "real"}
    assert real == set(GK.REQUIRED_EDGES), set(GK.REQUIRED_EDGES) - real      # a real-valued case on every family
    assert any(c["kind"] == "real" and c["kernel"] == "gemm_bf16_v8_kernel<half>" for c in GK.CASES)


def _tile_rows(c):
    return [(m0, min(m0 + 256, c["M"]) - 1) for m0 in range(0, c["M"], 256)]


def zero_filled_tiles(c, P):
    """row tiles the v4 / v8 kernels fill with zeros without a K loop, by their own rule (csrc/gemm.hip, `mask_tile` / `gate_tile`):
    no split-K, no aux_out, a bf16 C with dense columns, vec_ok & 1 (32-byte aligned C and aux, pitches % 8), N % 8 == 0, the whole
    256-row tile inside one utterance (b0 == b1) and its first row's t0 >= row_len[b0]"""
    kw = P.kw
    ok = (c["family"] in ("v4", "v8") and c["splitk"] <= 1 and "aux_out" not in P.t and c["c_dt"] == "bf16" and c["csc"] == 1
          and c["c_mis"] == 0 and kw["ldc"] % 8 == 0 and ("aux_in" not in P.t or kw["ldaux"] % 8 == 0) and c["N"] % 8 == 0)
    if not ok or c["lens"] is None:
        return []
    rpb, ri = c["rows_per_b"], c["rows_inner"]
    return [(m0, m1) for m0, m1 in _tile_rows(c) if m0 // rpb == m1 // rpb and (m0 % rpb) // ri >= c["lens"][m0 // rpb]]


def live_tiles(c, P):
    dead = zero_filled_tiles(c, P)
    return [t for t in _tile_rows(c) if t not in dead]


def dead_ktiles(c):
    """whole 64-position K-tiles (not the K tail) the gathered weight gradient skips: inside one utterance, first position beyond
    that utterance's valid positions (`dead` in csrc/gemm.hip)"""
    if c["lens"] is None:
        return 0
    rpb, n = c["rows_per_b"], 0
    for k0 in range(0, c["K"] - 63, 64):
        u = k0 // rpb
        n += (k0 + 63) // rpb == u and k0 - u * rpb >= min(rpb, c["lens"][u] * c["rows_inner"])
    return n


def test_edge_tags_say_what_the_case_is():
    for c in GK.CASES:
        P = GK.problem(c["name"])
        e, kw, M, N, K = c["edges"], P.kw, c["M"], c["N"], c["K"]
        nk = (K + 63) // 64
        tile_m = 128 if c["family"] == "s" else 256
        tile_n = 128 if c["family"] in ("s", "v2", "v5") else 256
        vec_ok = None
        if N == 324:   # gemm_fill's vec_ok: bit 0 = 8-wide (f32 pitch % 4, bf16 pitch % 8), bit 1 = 4-wide (pitch % 4), both need a 32-byte aligned C
            al = c["c_mis"] == 0
            ld_ok8 = all(ld % (4 if dt == "f32" else 8) == 0 for ld, dt in ((kw["ldc"], c["c_dt"]),) + (((kw["ldaux"], c["aux_dt"]),) if "aux_out" in P.t else ()))
            ld_ok4 = kw["ldc"] % 4 == 0 and kw["ldaux"] % 4 == 0
            vec_ok = (1 if al and ld_ok8 else 0) | (2 if al and ld_ok4 else 0)
        checks = {
            "n129": N == 129, "n128": N == 128, "one_ktile": nk == 1, "tile_tail": M % tile_m != 0 and N % tile_n != 0 or c["family"] in ("v5", "v8") and M % tile_m != 0,
            "m_lt_tile": M < 64, "odd_n_scalar": N % 2 == 1 and c["c_mis"] != 0, "k_mod8": K % 8 != 0,
            "k_tail64": K % 64 != 0, "odd_ktiles": nk % 2 == 1 and nk > 1, "pitch_garbage": c["garbage"] and c["lda_pad"] > 0,
            "splitk_gt_nk": c["splitk"] > nk and c["atomic"], "splitk_uneven": c["atomic"] and 1 < c["splitk"] <= nk and nk % c["splitk"] != 0,
            "colsum_tail": c["colsum"] and M % 64 != 0 and c["atomic"] | (c["lay"] == "TN"), "two_level_batch": 0 < kw.get("nb0", 0) < c["batch"] and kw.get("b_off", 0) > 0,
            "plain_batch": c["batch"] > 1 and c["style"] == "dense", "resid_inplace": c["inplace"] and c["epi"] == GO.RESID,
            "relu_len0": c["lens"] is not None and 0 in c["lens"] and c["epi"] == GO.RELU_MASK,
            "relu_full": c["lens"] is not None and max(c["lens"]) * c["rows_inner"] >= min(c["rows_per_b"], M) and c["epi"] == GO.RELU_MASK,
            "relu_dead_tile": c["epi"] == GO.RELU_MASK and c["rowmap"] is None and zero_filled_tiles(c, P) and live_tiles(c, P),
            "gate_dead_tile": c["epi"] == GO.MUL_POS and c["rowmap"] is not None and zero_filled_tiles(c, P) and live_tiles(c, P),
            "gather_b_dead_ktile": c["style"] == "gatherB" and c["family"] in ("v2", "v4", "v8") and dead_ktiles(c) > 0,
            "n324_vec3": vec_ok == 3, "n324_vec2": vec_ok == 2, "n324_vec0": vec_ok == 0, "rowmap_store": c["rowmap"] is not None and c["epi"] == GO.STORE,
            "col_stride": c["csc"] > 1, "dropout": c["p"] > 0, "v8_delay": c["modes"].get(9, 0) > 0,
            "gather_a": c["style"] == "gatherA", "gather_b": c["style"] == "gatherB", "gather_b_hint": c["style"] == "gatherB" and c["lens"] is not None,
            "v5_short_last_round": c["family"] == "v5" and 0 < (((M + 255) // 256) * (N // 128)) % 256 < 256,
        }
        for tag in e:
            assert checks[tag], (c["name"], tag)


def test_exact_cases_stay_below_2_to_22_quanta_and_no_case_is_too_large():
    for c in GK.CASES:
        P = GK.problem(c["name"])
        assert c["batch"] * c["M"] * c["N"] <= GK.MAX_ELEMS, c["name"]
        if c["kind"] != "exact":
            continue
        worst, q = GK.exactness(P)
        assert worst < GK.QUANTA, (c["name"], worst)
        # every operand and every exact-kind ingredient is a whole number of quanta
        for k in ("bias", "colsum"):
            if k in P.t:
                v = P.t[k].double() / q
                assert bool((v == v.round()).all()), (c["name"], k)
        v = P.e.acc / q
        assert bool((v == v.round()).all()), c["name"]
        # what an equality assertion compares with is a float32 number itself: no rounding is hidden in the "exact" value
        if c["epi"] in GK.EXACT_EPIS and (c["p"] == 0.0 or c["epi"] in (GO.RELU_MASK, GO.MUL_POS, GO.DSWISH_G)):
            for v in (P.e.value, P.e.pre, P.e.C[P.e.written]) + ((P.e.colsum,) if P.e.colsum is not None else ()):
                assert bool((v.float().double() == v).all()), c["name"]
        if c["epi"] == GO.SWISH_DROP:
            assert bool((P.e.pre.float().double() == P.e.pre).all()), c["name"]
        if c["epi"] in (GO.SWISH_DROP, GO.SWISH_DROP_G):
            assert P.e.pre.abs().max().item() <= 10.0, (c["name"], P.e.pre.abs().max().item())
    for name in GK.GROUPED:
        for e in GK.grouped_problem(name)[1]:
            assert e.abs.max().item() < GK.QUANTA, name
    assert GK.parity_problem()[6] < GK.QUANTA


# ------------------------------------------------------------------------------------------------ the oracle against independent forms
def test_oracle_gather_is_conv2d_and_its_gradients():
    g = torch.Generator().manual_seed(3)
    Bn, C_, Co, T1, F1 = 2, 8, 5, 9, 6
    T2, F2 = (T1 - 1) // 2 + 1, (F1 - 1) // 2 + 1
    x = torch.randn(Bn, T1, F1, C_, generator=g, dtype=F64)
    w = torch.randn(Co, C_, 3, 3, generator=g, dtype=F64)
    dy = torch.randn(Bn, T2, F2, Co, generator=g, dtype=F64)
    taps = [(kh - 1, kw - 1) for kh in range(3) for kw in range(3)]
    geo = dict(nI=T2, nJ=F2, SI=T1, SJ=F1, C=C_, si=2, sj=2, taps=taps)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xr.permute(0, 3, 1, 2), wr, None, stride=2, padding=1)
    y.backward(dy.permute(0, 3, 1, 2))
    M2 = Bn * T2 * F2
    # forward: gathered A rows against the weight image [Co, 9 * C]
    wp = w.permute(0, 2, 3, 1).reshape(Co, 9 * C_).contiguous()
    e = GO.gemm(x, wp, torch.zeros(M2 * Co), M2, Co, 9 * C_, C_, 9 * C_, Co, gather=geo)
    assert torch.allclose(e.C.view(Bn, T2, F2, Co), y.detach().permute(0, 2, 3, 1), atol=1e-12)
    # weight gradient: gathered reduction-major B, batch = taps, column stride 9 -> [Co, C, 3, 3]
    e = GO.gemm(dy, x, torch.zeros(Co * C_ * 9), Co, C_, M2, Co, C_, 9 * C_, transA=True, transB=True, atomic=True, splitk=3, batch=9,
                nb0=9, sC=(1, 0), c_col_stride=9, gather=dict(geo, operand=1))
    assert torch.allclose(e.C.view(Co, C_, 3, 3), wr.grad, atol=1e-12) and bool(e.written.all())
    # input gradient: four parity classes, gathered dY, row map
    dx = torch.full((Bn * T1 * F1 * C_,), float("nan"), dtype=F64)
    for pt in (0, 1):
        for pf in (0, 1):
            nI, nJ = (T1 - pt + 1) // 2, (F1 - pf + 1) // 2
            slots = [(kh, kw) for kh in ([1] if pt == 0 else [0, 2]) for kw in ([1] if pf == 0 else [0, 2])]
            taps_d = [(1 if kh == 0 else 0, 1 if kw == 0 else 0) for kh, kw in slots]
            wimg = torch.cat([w[:, :, kh, kw].t() for kh, kw in slots], dim=1).contiguous()
            K = len(slots) * Co
            dx = GO.gemm(dy, wimg, dx, Bn * nI * nJ, C_, K, Co, K, C_, gather=dict(nI=nI, nJ=nJ, SI=T2, SJ=F2, C=Co, si=1, sj=1, taps=taps_d),
                         rowmap=dict(nI=nI, nJ=nJ, OI=T1, OJ=F1, si=2, sj=2, oi=pt, oj=pf)).C
    assert torch.allclose(dx.view(Bn, T1, F1, C_), xr.grad, atol=1e-12)


def test_oracle_row_map_is_strided_indexing_and_column_stride_leaves_gaps():
    g = torch.Generator().manual_seed(4)
    Bn, nI, nJ, OI, OJ, N, K = 2, 3, 4, 7, 9, 5, 6
    A, W = torch.randn(Bn * nI * nJ, K, generator=g, dtype=F64), torch.randn(N, K, generator=g, dtype=F64)
    e = GO.gemm(A, W, torch.full((Bn * OI * OJ * N,), float("nan"), dtype=F64), Bn * nI * nJ, N, K, K, K, N,
                rowmap=dict(nI=nI, nJ=nJ, OI=OI, OJ=OJ, si=2, sj=2, oi=1, oj=0))
    grid = e.C.view(Bn, OI, OJ, N)
    want = (A @ W.t()).view(Bn, nI, nJ, N)
    assert torch.equal(grid[:, 1:1 + 2 * nI:2, 0:2 * nJ:2], want)
    hit = torch.zeros(Bn, OI, OJ, N, dtype=torch.bool)
    hit[:, 1:1 + 2 * nI:2, 0:2 * nJ:2] = True
    assert torch.equal(e.written.view(Bn, OI, OJ, N), hit) and bool(torch.isnan(grid[~hit]).all())
    e = GO.gemm(A, W, torch.zeros(Bn * nI * nJ * N * 3), Bn * nI * nJ, N, K, K, K, 3 * N, c_col_stride=3, c_off=1)
    assert torch.equal(e.C.view(-1, N, 3)[:, :, 1], A @ W.t()) and torch.equal(e.written.view(-1, N, 3)[0, 0], torch.tensor([False, True, False]))


def test_oracle_two_level_batch_is_an_einsum():
    """attention-style head slices of one [B*T, 3d] matrix (test_gemm_batched_strided_bf16)"""
    g = torch.Generator().manual_seed(5)
    Bn, H, T, dk, Tp = 3, 2, 5, 4, 8
    d = H * dk
    qkv = torch.randn(Bn * T, 3 * d, generator=g, dtype=F64)
    e = GO.gemm(qkv, qkv, torch.zeros(H * Bn * T * Tp), T, T, dk, 3 * d, 3 * d, Tp, batch=H * Bn, nb0=Bn, sA=(T * 3 * d, dk),
                sB=(T * 3 * d, dk), sC=(T * Tp, Bn * T * Tp), b_off=d)
    ref = torch.einsum("bihe,bjhe->hbij", qkv[:, :d].view(Bn, T, H, dk), qkv[:, d:2 * d].view(Bn, T, H, dk))
    assert torch.allclose(e.C.view(H, Bn, T, Tp)[..., :T], ref, atol=1e-12)
    assert not bool(e.written.view(H, Bn, T, Tp)[..., T:].any())
    # NN with a reduction-major B slice and a strided C: P @ V
    p = torch.rand(H, Bn, T, Tp, generator=g, dtype=F64)
    p[..., T:] = 0
    vpad = torch.cat([qkv, torch.zeros(Tp, 3 * d, dtype=F64)])
    e = GO.gemm(p, vpad, torch.zeros(Bn * T * d), T, dk, Tp, Tp, 3 * d, d, transB=True, batch=H * Bn, nb0=Bn, sA=(T * Tp, Bn * T * Tp),
                sB=(T * 3 * d, dk), sC=(T * d, dk), b_off=2 * d)
    ref2 = torch.einsum("hbij,bjhe->bihe", p[..., :T], qkv[:, 2 * d:].view(Bn, T, H, dk)).reshape(Bn * T, d)
    assert torch.allclose(e.C.view(Bn * T, d), ref2, atol=1e-12)


def test_oracle_epilogues_are_the_closed_forms_of_test_gemm_epilogues():
    g = torch.Generator().manual_seed(2)
    M, N, K = 26, 12, 9
    A, W = torch.randn(M, K, generator=g, dtype=F64), torch.randn(N, K, generator=g, dtype=F64) * 0.1
    bias, res, pre = (torch.randn(s, generator=g, dtype=F64) for s in ((N,), (M, N), (M, N)))
    acc = A @ W.t() + bias
    run = lambda **kw: GO.gemm(A, W, kw.pop("C", torch.zeros(M * N)), M, N, K, K, K, N, **kw)
    sg = torch.sigmoid(pre)
    assert torch.allclose(run(bias=bias, alpha=0.5).C.view(M, N), 0.5 * acc, atol=1e-13)
    e = run(bias=bias, epi=GO.SWISH_DROP, aux_out=M * N)
    assert torch.allclose(e.aux.view(M, N), acc, atol=1e-13) and torch.allclose(e.C.view(M, N), acc * torch.sigmoid(acc), atol=1e-13)
    assert torch.allclose(run(bias=bias, alpha=0.5, epi=GO.RESID, aux_in=res).C.view(M, N), res + 0.5 * acc, atol=1e-13)
    assert torch.allclose(run(epi=GO.DSWISH, aux_in=pre).C.view(M, N), (acc - bias) * (sg * (1 + pre * (1 - sg))), atol=1e-13)
    assert torch.allclose(run(epi=GO.DSWISH_G, aux_in=pre).C.view(M, N), (acc - bias) * pre, atol=1e-13)
    assert torch.allclose(run(epi=GO.MUL_POS, aux_in=pre).C.view(M, N), (acc - bias) * (pre > 0), atol=1e-13)
    lens = torch.tensor([3, 1, 0], dtype=torch.int64)
    m = torch.arange(M)
    keep = ((m % 12) // 4) < lens[m // 12]
    assert torch.allclose(run(bias=bias, epi=GO.RELU_MASK, row_len=lens, rows_per_b=12, rows_inner=4).C.view(M, N),
                          torch.relu(acc) * keep[:, None], atol=1e-13)
    assert torch.allclose(run(C=torch.ones(M * N), atomic=True, splitk=3).C.view(M, N), 1.0 + (acc - bias), atol=1e-13)
    # dropout: the mask of drop_scale_cast at idx = z*M*N + m*N + n, scaled by 1 / (1 - p); SWISH_DROP_G stores swish' * mask
    drop = EO.Drop(0.25, 7, 3)
    mask = EO.keep_mask(drop, 0, M * N).view(M, N).double() / 0.75
    assert torch.allclose(run(bias=bias, alpha=2.0, drop=drop).C.view(M, N), 2.0 * acc * mask, atol=1e-13)
    e = run(bias=bias, epi=GO.SWISH_DROP_G, aux_out=M * N, drop=drop)
    sa = torch.sigmoid(acc)
    assert torch.allclose(e.aux.view(M, N), sa * (1 + acc * (1 - sa)) * mask, atol=1e-13)
    # the derivative is the derivative
    h = torch.linspace(-8, 8, 101, dtype=F64, requires_grad=True)
    (h * torch.sigmoid(h)).sum().backward()
    assert torch.allclose(GO.swish_grad(h.detach()), h.grad, atol=1e-14)
    # transposed layouts and the column sums of a reduction-major A
    At, Wt = A.t().contiguous(), W.t().contiguous()
    e = GO.gemm(At, Wt, torch.zeros(M * N), M, N, K, M, N, N, transA=True, transB=True, atomic=True, colsum_out=torch.ones(M + 2))
    assert torch.allclose(e.C.view(M, N), A @ W.t(), atol=1e-13) and torch.allclose(e.colsum[:M], 1 + A.sum(1), atol=1e-13)
    assert torch.equal(e.colsum[M:], torch.ones(2, dtype=F64)) and not bool(e.colsum_written[M:].any())
    gr = GO.wgrad_grouped([(At, M, 0, Wt, N, 0, torch.zeros(M, N), M, N, None)], K)
    assert torch.allclose(gr[0].C.view(M, N), A @ W.t(), atol=1e-13)
