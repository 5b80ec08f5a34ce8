"""-m gpu: every kernel instantiation behind mi355x_gemm (the 30 ids of tests/test_gemm_plan_host.KERNELS) and both grouped
kernels of nemo_amd/csrc/gemm.hip, element by element against the float64 restatement of tests/gemm_oracle.py.

Harness.  Outputs are `Guarded` views (imported from tests/test_elementwise_kernels_gpu.py): sentinel words in front of and behind
every output.  C and aux_out of a non-atomic launch start as NaN; after the launch every element the oracle says is written must
be finite and every other element (pad columns of a pitched output, rows the row map does not hit, the gaps of a column-strided
C) must hold the bits it held before.  The device step word is cleared first, so dropout keys are used as passed.  Before each
launch ops.gemm_plan is asked, under the same gemm_modes, which kernel the descriptor reaches, and the case's intended id is
asserted; after the launch key 11 must report the plan's code.  The grouped kernels have no plan call: which one runs is taken
from group_plan's rules (the v2 body by default; the v8 body under key 8 = 3 when every N > 128 and K >= 4 K-tiles), not asserted.
Every case is launched twice into fresh outputs; non-atomic launches must give the same bits.

Exact accumulators.  Operands are bf16 values s * m * 2^e (m over the 8-bit significands, about a quarter zero, signs and widths
drawn differently for A and B) such that for every output element sum_k |a_k||b_k| < 2^22 quanta (tests/test_gemm_cases_host.py
asserts it): every product and every partial sum is then a float32 number, whatever the order, the structure or the split.
Bias, residual, pre-fill and the DSWISH_G factor lie on the same quantum, alpha is a power of two.

What is asserted, per element:
  f32 outputs without a transcendental (STORE, RESID, RELU_MASK, MUL_POS, DSWISH_G, atomic accumulation, colsum_out, the aux_out
  of SWISH_DROP)                          got == float64 value (compared as floats: -0 == +0)
  bf16 outputs of the same kinds          got == round-to-nearest-even bf16 of the float64 value
  dropout on STORE / RESID                zero set among written elements with a non-zero reference == keep_mask's; kept values to
                                          4 * 2^-24 relative (the host's 1 / (1 - p), alpha * mask, the product), RESID: of the scaled
                                          term, plus 2^-24 of the result for the final add; plus half a bf16 ulp for a bf16 output
  Swish kinds (C of SWISH_DROP / SWISH_DROP_G, aux_out of SWISH_DROP_G, C of DSWISH)
                                          |got - ref| <= tol * |ref| (swish': tol * the value with swish' replaced by its
                                          conditioning sum) against the float64 closed form on the exact pre-activation,
                                          plus the dropout term above when a mask is on and half a bf16 ulp for a bf16 output; a
                                          bf16 aux_in is an input (the oracle reads the stored value) and adds nothing
  real-valued cases (uniform operands, f32 STORE, one per structure family, v8<half> too)
                                          |got - ref| <= K * 2^-24 * sum_k |a_k||b_k|: K - 1 float32 additions in any order (and,
                                          for the fp32 kernels, whose operands are not bf16 numbers, the product's own rounding)

Measured bound for the Swish kinds: the float32 CPU restatement of swish_pair / swish_grad (torch.exp and a division in float32)
against float64 on each case's own pre-activations, worst element over the cases, and 8x that for the device's approximate exp and
rcp (`python tests/test_gemm_kernels_gpu.py` re-measures on the CPU):
  swish(h)            measured 1.7e-07 -> bound 1.3e-06   relative to |swish(h)|
  swish'(h)           measured 4.1e-07 -> bound 3.3e-06   relative to s (1 + |h| (1 - s)), see swish_grad_cond(): relative to
                      |swish'(h)| itself the float32 restatement is already 3.3e-2 off next to the sign change at h = -1.278
Pre-activations are scaled to lie within about +-8 (the largest of these cases: 6.0).

Outcome of the exact-accumulation assumption on the device: it holds.  Every exact case -- all 30 kernel ids, both grouped kernels,
split-K atomics, the 32x32x16, 16x16x32 and fp32 matrix-core paths -- came back equal to the float64 value, bit for bit; the
any-order bound is used for the real-valued cases only.

Found by this file and fixed in csrc/gemm.hip (the cases stay):
  v2_rowmap   a row map with an epilogue other than MUL_POS: the full-width tile epilogues (fast_epilogue, v8_round_fast) apply the
              map for MUL_POS only and wrote such a launch to unmapped rows.  gemm_fill now keeps those launches off them.
  v8_nt_sk    split-K with a bias: every K slice runs the whole epilogue, so the bias was added once per slice (all 79 200 elements
              off by the bias).  More than one slice with a bias, a residual, Swish or ReLU is now rejected (MI_ERR_ARG); the case
              runs without a bias, tests/test_gemm_cases_host.py holds the rejections.

Edges that do not apply: a single K-tile on v8 (the structure needs two K-tiles a workgroup) and on v6 (four); K % 8 != 0 on the
K-contiguous v8 / v6 / v5 kernels (whole K-tiles only: v8 meets it in the TN layout); v5 and v6 take dense NT launches without
batch, split-K, row map or gather, so only M tails, dropout, the in-place residual and the real-valued case remain for them; the
dead-tile zero fill and the dead K-tile skip exist in v4 and v8 only (v2 runs the same descriptors through its ordinary path).
The plan assertion builds its descriptor with ops.gemm_desc, the function ops.gemm fills its own with.

Not covered at a small shape: gemm_bf16_v8_kernel<half> needs 224 workgroups (16032 x 512) and the persistent v5 kernels 256
tiles of 256 x 128 (5400 x 1536, 8100..8300 x 1024); their float64 references are computed once per module.  The v5 tile list is
tm2 * tn, so a tile wholly past M does not exist; a last round with a few tiles and a partly filled last row tile are covered.
"""
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import elementwise_oracle as EO  # noqa: E402
import gemm_oracle as GO  # noqa: E402
from test_elementwise_kernels_gpu import Guarded, assert_intact  # noqa: E402
from test_gemm_plan_host import KERNELS  # noqa: E402

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
TDT = {"f32": F32, "bf16": BF16}
NAN = float("nan")
U = 2.0 ** -24
QUANTA = 2 ** 22                       # sum_k |a||b| stays below this many quanta
TOL_DROP = 4 * U                       # three float32 roundings, as drop_scale_cast's
TOL_SWISH = {"act": 1.3e-6, "grad": 3.3e-6}   # measured, see the header
MAX_ELEMS = 8300 * 1024                # no case has more output elements than this
TAPS9 = [(kh - 1, kw - 1) for kh in range(3) for kw in range(3)]
GRID = dict(nI=4, nJ=5, SI=8, SJ=10, si=2, sj=2)      # the conv2 geometry of the gathered cases: batch of 10, 200 positions
GRID16 = dict(nI=16, nJ=16, SI=32, SJ=32, si=2, sj=2)  # 256 positions an utterance: one utterance per 256-row tile
DGRID16 = dict(nI=16, nJ=16, SI=16, SJ=16, si=1, sj=1)  # the input gradient's gather of dY (one parity class), same tiles
ROWMAP16 = dict(nI=16, nJ=16, OI=32, OJ=32, si=2, sj=2, oi=1, oj=1)
GRID8 = dict(nI=8, nJ=8, SI=16, SJ=16, si=2, sj=2)     # 64 positions an utterance: one utterance per K-tile of the weight gradient
TAPS4 = [(0, 0), (0, 1), (1, 0), (1, 1)]
V4, V8 = {4: 2, 5: 0, 8: 0}, {8: 2, 5: 0}
EXACT_EPIS = (GO.STORE, GO.RESID, GO.RELU_MASK, GO.MUL_POS, GO.DSWISH_G)


def up8(n):
    return (n + 7) & ~7


# ------------------------------------------------------------------------------------------------ case table (no device)
def case(name, kernel, M, N, K, lay="NT", modes=None, family=None, edges=(), **opt):
    c = dict(name=name, kernel=kernel, M=M, N=N, K=K, lay=lay, modes=dict(modes or {}), edges=set(edges),
             in_dt="bf16", c_dt="f32", epi=GO.STORE, aux_dt="f32", p=0.0, alpha=1.0, bias=False, batch=1, splitk=1, atomic=False,
             lda_pad=0, garbage=False, ldc=None, ldaux=None, csc=1, c_mis=0, style="dense", geo=None, rowmap=None, lens=None,
             rows_per_b=1, rows_inner=1, colsum=False, kind="exact", inplace=False)
    assert not set(opt) - set(c), set(opt) - set(c)
    c.update(opt)
    c["family"] = family or kernel.split("_kernel")[0].replace("gemm_bf16_", "").replace("gemm_bf16", "s").replace("gemm_f32_mfma", "f32").replace("gemm_", "")
    return c


def _cases():
    S, R = GO.STORE, GO.RESID
    out = [
        # ---- gemm_bf16_kernel: 128 x 128 tiles
        case("s_nt", "gemm_bf16_kernel<0,0>", 130, 129, 64, bias=True, alpha=0.5, edges={"n129", "one_ktile", "tile_tail"}),
        case("s_nn", "gemm_bf16_kernel<0,1>", 130, 129, 64, "NN", c_dt="bf16", bias=True, p=0.1, c_mis=2,
             edges={"odd_n_scalar", "dropout"}),
        case("s_tn", "gemm_bf16_kernel<1,1>", 130, 129, 64, "TN", atomic=True, splitk=4, colsum=True, garbage=True,
             edges={"splitk_gt_nk", "colsum_tail"}),
        case("s_tt", "gemm_bf16_kernel<1,0>", 300, 200, 136, "TT", epi=R, alpha=0.5, bias=True, inplace=True,
             edges={"resid_inplace", "odd_ktiles", "k_tail64"}),
        case("s_small", "gemm_bf16_kernel<0,0>", 33, 31, 70, c_dt="bf16", epi=GO.RELU_MASK, bias=True, c_mis=2, lens=[3, 0, 2],
             rows_per_b=12, rows_inner=4, edges={"m_lt_tile", "k_mod8", "odd_n_scalar", "relu_len0", "relu_full"}),
        case("s_attn", "gemm_bf16_kernel<0,0>", 77, 77, 32, style="attn", batch=12, edges={"two_level_batch"}),
        case("s_324", "gemm_bf16_kernel<0,0>", 100, 324, 136, c_dt="bf16", aux_dt="bf16", epi=GO.SWISH_DROP_G, bias=True, p=0.25,
             ldc=328, ldaux=328, edges={"n324_vec3", "dropout"}),
        case("s_real", "gemm_bf16_kernel<0,0>", 130, 129, 64, kind="real"),
        # ---- gemm_bf16_v2_kernel: 256 x 128 tiles
        case("v2_nt", "gemm_bf16_v2_kernel<0,0>", 300, 200, 136, epi=GO.DSWISH, aux_dt="bf16", p=0.1,
             edges={"tile_tail", "odd_ktiles", "k_tail64", "dropout"}),
        case("v2_reg", "gemm_bf16_v2_kernel<0,0,reg>", 300, 200, 256, epi=GO.SWISH_DROP, bias=True),
        case("v2_nn", "gemm_bf16_v2_kernel<0,1>", 300, 200, 136, "NN", c_dt="bf16", epi=GO.MUL_POS, aux_dt="bf16"),
        case("v2_tn", "gemm_bf16_v2_kernel<1,1>", 300, 200, 136, "TN", atomic=True, splitk=2, colsum=True,
             edges={"splitk_uneven", "colsum_tail"}),
        case("v2_324_bf16", "gemm_bf16_v2_kernel<0,0>", 300, 324, 136, c_dt="bf16", bias=True, p=0.25, ldc=324,
             edges={"n324_vec2", "dropout"}),
        case("v2_324_f32", "gemm_bf16_v2_kernel<0,0>", 300, 324, 136, epi=R, alpha=0.5, bias=True, ldc=324, inplace=True,
             edges={"n324_vec3", "resid_inplace"}),
        case("v2_324_mis", "gemm_bf16_v2_kernel<0,0>", 300, 324, 136, bias=True, alpha=2.0, ldc=328, c_mis=4, edges={"n324_vec0"}),
        case("v2_odd", "gemm_bf16_v2_kernel<0,0>", 300, 201, 70, c_dt="bf16", bias=True, c_mis=2, lda_pad=16, garbage=True,
             edges={"odd_n_scalar", "k_mod8", "pitch_garbage"}),
        case("v2_n128", "gemm_bf16_v2_kernel<0,0>", 300, 128, 64, c_dt="bf16", bias=True, alpha=0.25, batch=3,
             edges={"n128", "one_ktile", "plain_batch"}),
        case("v2_rowmap", "gemm_bf16_v2_kernel<0,0>", 200, 128, 64, bias=True, rowmap=dict(nI=4, nJ=5, OI=8, OJ=10, si=2, sj=2, oi=1, oj=0),
             edges={"rowmap_store"}),
        case("v2_csc", "gemm_bf16_v2_kernel<0,0>", 300, 200, 136, csc=2, edges={"col_stride"}),
        case("v2_dswish_g", "gemm_bf16_v2_kernel<0,0,reg>", 300, 256, 256, epi=GO.DSWISH_G, aux_dt="bf16", c_dt="bf16", bias=True),
        case("v2_real", "gemm_bf16_v2_kernel<0,0>", 300, 200, 136, kind="real"),
        # ---- gemm_bf16_v4_kernel / v6: 256 x 256 tiles, lock step
        case("v4_nt", "gemm_bf16_v4_kernel<0,0,0>", 300, 264, 136, modes=V4, c_dt="bf16", epi=GO.RELU_MASK, bias=True,
             lens=[2, 5, 0], rows_per_b=100, rows_inner=20, edges={"tile_tail", "k_tail64", "odd_ktiles"}),
        case("v4_nn", "gemm_bf16_v4_kernel<0,1,0>", 300, 264, 136, "NN", modes=V4, epi=GO.DSWISH_G, aux_dt="f32", bias=True),
        case("v4_tn", "gemm_bf16_v4_kernel<1,1,0>", 300, 264, 136, "TN", modes=V4, atomic=True, splitk=5, colsum=True,
             edges={"splitk_gt_nk", "colsum_tail"}),
        case("v4_324", "gemm_bf16_v4_kernel<0,0,0>", 300, 324, 128, modes=V4, c_dt="bf16", aux_dt="bf16", epi=GO.SWISH_DROP_G, p=0.1,
             bias=True, ldc=328, ldaux=328, edges={"n324_vec3", "dropout"}),
        case("v4_real", "gemm_bf16_v4_kernel<0,0,0>", 300, 264, 136, modes=V4, kind="real"),
        case("v6_1", "gemm_bf16_v6_kernel<1>", 300, 264, 256, modes={**V4, 6: 1}, c_dt="bf16", bias=True, p=0.1, edges={"dropout"}),
        case("v6_0", "gemm_bf16_v6_kernel<0>", 300, 264, 256, modes={**V4, 6: 2}, epi=R, alpha=0.5, bias=True),
        # ---- gemm_bf16_v8_kernel: 256 x 256 tiles, phase-staggered
        case("v8_nt", "gemm_bf16_v8_kernel<0,nt>", 300, 264, 128, modes={**V8, 10: 0}, epi=R, alpha=0.5, bias=True, p=0.1,
             edges={"tile_tail", "dropout"}),
        case("v8_nt_324", "gemm_bf16_v8_kernel<0,nt>", 300, 324, 192, modes={**V8, 10: 0}, c_dt="bf16", bias=True, ldc=324,
             edges={"n324_vec2", "odd_ktiles"}),
        case("v8_nt_sk", "gemm_bf16_v8_kernel<0,nt>", 300, 264, 320, modes={**V8, 10: 0}, atomic=True, splitk=2, alpha=0.5,
             edges={"splitk_uneven"}),
        case("v8_tn", "gemm_bf16_v8_kernel<0,tn>", 300, 264, 203, "TN", modes={8: 2}, colsum=True, garbage=True,
             edges={"k_tail64", "colsum_tail", "k_mod8"}),
        case("v8_es1", "gemm_bf16_v8_kernel<es1>", 300, 264, 128, modes={**V8, 10: 1}, c_dt="bf16", aux_dt="bf16", epi=GO.SWISH_DROP_G,
             bias=True, p=0.1, edges={"dropout"}),
        case("v8_es2", "gemm_bf16_v8_kernel<es2>", 300, 264, 128, modes={**V8, 10: 1}, c_dt="bf16", aux_dt="bf16", epi=GO.SWISH_DROP_G,
             bias=True),
        case("v8_es3", "gemm_bf16_v8_kernel<es3>", 300, 264, 128, modes={**V8, 10: 1}, c_dt="bf16", aux_dt="bf16", epi=GO.DSWISH_G),
        case("v8_es4", "gemm_bf16_v8_kernel<es4>", 300, 264, 128, modes={**V8, 10: 1}, c_dt="bf16", bias=True, alpha=0.5),
        case("v8_delay", "gemm_bf16_v8_kernel<0,nt>", 300, 264, 128, modes={**V8, 10: 0, 9: 3}, batch=65, bias=True,
             edges={"v8_delay", "plain_batch"}),
        case("v8_real", "gemm_bf16_v8_kernel<0,nt>", 300, 264, 128, modes={**V8, 10: 0}, kind="real"),
        case("v8_half", "gemm_bf16_v8_kernel<half>", 16032, 512, 128, modes=V8, c_dt="bf16", bias=True, p=0.1,
             edges={"tile_tail", "dropout"}),
        # ---- gemm_bf16_v5_kernel: persistent 256 x 128 tiles
        case("v5_store", "gemm_bf16_v5_kernel<store>", 5400, 1536, 512, modes={5: 2, 8: 0}, c_dt="bf16", bias=True, alpha=0.5,
             edges={"tile_tail", "v5_short_last_round"}),
        case("v5_swish", "gemm_bf16_v5_kernel<swish_drop>", 8192, 1024, 512, modes={5: 2, 8: 0}, c_dt="bf16", aux_dt="bf16",
             epi=GO.SWISH_DROP, bias=True, p=0.1, edges={"dropout"}),
        case("v5_resid", "gemm_bf16_v5_kernel<resid>", 8300, 1024, 512, modes={5: 2, 8: 0}, epi=R, alpha=0.5, bias=True, inplace=True,
             edges={"tile_tail", "v5_short_last_round", "resid_inplace"}),
        case("v5_dswish", "gemm_bf16_v5_kernel<dswish>", 8100, 1024, 512, modes={5: 2, 8: 0}, c_dt="bf16", aux_dt="bf16",
             epi=GO.DSWISH_G, edges={"tile_tail"}),
        # ---- fp32 operands
        case("f32_valu", "gemm_f32_kernel", 33, 31, 7, modes={3: 0}, in_dt="f32", epi=R, alpha=0.5, bias=True,
             edges={"m_lt_tile", "k_mod8"}),
        case("f32_mfma", "gemm_f32_mfma_kernel", 33, 31, 7, "TT", modes={3: 1}, in_dt="f32", bias=True, atomic=True, splitk=3,
             edges={"m_lt_tile", "k_mod8", "splitk_gt_nk"}),
        # ---- gathered A rows (conv forward): nine taps, stride 2, batch of 10
        case("ga_v2", "gemm_bf16_v2_kernel<0,0>", 200, 128, 576, style="gatherA", geo=dict(GRID, C=64, taps=TAPS9), c_dt="bf16",
             epi=GO.RELU_MASK, bias=True, lens=[4, 0, 2, 1, 4, 3, 0, 4, 2, 1], rows_per_b=20, rows_inner=5,
             edges={"relu_len0", "relu_full", "gather_a"}),
        case("ga_v4", "gemm_bf16_v4_kernel<0,0,1>", 200, 136, 576, modes=V4, style="gatherA", geo=dict(GRID, C=64, taps=TAPS9),
             c_dt="bf16", epi=GO.RELU_MASK, bias=True, lens=[0] * 10, rows_per_b=20, rows_inner=5, edges={"relu_len0", "gather_a"}),
        case("ga_v8", "gemm_bf16_v8_kernel<1,nt>", 200, 136, 576, modes={8: 2}, style="gatherA", geo=dict(GRID, C=64, taps=TAPS9),
             epi=GO.RELU_MASK, bias=True, lens=[4, 0, 2, 1, 4, 3, 0, 4, 2, 1], rows_per_b=20, rows_inner=5,
             edges={"relu_len0", "relu_full", "gather_a"}),
        # one utterance per 256-row tile: the second tile lies wholly beyond its utterance's length and is zero-filled without a K loop
        case("ga_v4_dead", "gemm_bf16_v4_kernel<0,0,1>", 512, 136, 576, modes=V4, style="gatherA", geo=dict(GRID16, C=64, taps=TAPS9),
             c_dt="bf16", epi=GO.RELU_MASK, bias=True, lens=[5, 0], rows_per_b=256, rows_inner=16, edges={"relu_dead_tile"}),
        case("ga_v8_dead", "gemm_bf16_v8_kernel<1,nt>", 512, 136, 576, modes={8: 2}, style="gatherA", geo=dict(GRID16, C=64, taps=TAPS9),
             c_dt="bf16", epi=GO.RELU_MASK, bias=True, lens=[5, 0], rows_per_b=256, rows_inner=16, edges={"relu_dead_tile"}),
        # the input gradient's form of the same hint: MUL_POS with row_len, the zeros written through the row map
        case("ga_v4_gate", "gemm_bf16_v4_kernel<0,0,1>", 512, 136, 256, modes=V4, style="gatherA", geo=dict(DGRID16, C=64, taps=TAPS4),
             c_dt="bf16", aux_dt="bf16", epi=GO.MUL_POS, rowmap=ROWMAP16, lens=[5, 0], rows_per_b=256, rows_inner=16,
             edges={"gate_dead_tile"}),
        case("ga_v8_gate", "gemm_bf16_v8_kernel<1,nt>", 512, 136, 256, modes={8: 2}, style="gatherA", geo=dict(DGRID16, C=64, taps=TAPS4),
             c_dt="bf16", aux_dt="bf16", epi=GO.MUL_POS, rowmap=ROWMAP16, lens=[5, 0], rows_per_b=256, rows_inner=16,
             edges={"gate_dead_tile"}),
        # ---- gathered reduction-major B (conv weight gradient): batch = 9 taps, column stride 9
        case("gb_v2", "gemm_bf16_v2_kernel<1,1>", 200, 136, 200, "TN", style="gatherB", geo=dict(GRID, C=136, taps=TAPS9, operand=1),
             batch=9, csc=9, atomic=True, splitk=2, lens=[4, 0, 2, 1, 4, 3, 0, 4, 2, 1], rows_per_b=20, rows_inner=5,
             edges={"gather_b", "gather_b_hint", "col_stride"}),
        case("gb_v4", "gemm_bf16_v4_kernel<1,1,2>", 200, 136, 200, "TN", modes=V4, style="gatherB",
             geo=dict(GRID, C=136, taps=TAPS9, operand=1), batch=9, csc=9, atomic=True, splitk=2, edges={"gather_b", "col_stride"}),
        case("gb_v8", "gemm_bf16_v8_kernel<2,tn>", 200, 136, 200, "TN", modes={8: 2}, style="gatherB",
             geo=dict(GRID, C=136, taps=TAPS9, operand=1), batch=9, csc=9, atomic=True, splitk=1, edges={"gather_b", "col_stride"}),
        case("gb_v8_hint", "gemm_bf16_v8_kernel<2,tn>", 200, 136, 200, "TN", modes={8: 2}, style="gatherB",
             geo=dict(GRID, C=136, taps=TAPS9, operand=1), batch=9, csc=9, atomic=True, splitk=1,
             lens=[4, 0, 2, 1, 4, 3, 0, 4, 2, 1], rows_per_b=20, rows_inner=5, edges={"gather_b_hint"}),
        # 64 positions per utterance: the second K-tile lies wholly beyond its utterance's length (skipped by v4 and v8)
        case("gb_v2_dead", "gemm_bf16_v2_kernel<1,1>", 200, 136, 256, "TN", style="gatherB", geo=dict(GRID8, C=136, taps=TAPS9, operand=1),
             batch=9, csc=9, atomic=True, splitk=2, lens=[8, 0, 3, 8], rows_per_b=64, rows_inner=8, edges={"gather_b_dead_ktile"}),
        case("gb_v4_dead", "gemm_bf16_v4_kernel<1,1,2>", 200, 136, 256, "TN", modes=V4, style="gatherB",
             geo=dict(GRID8, C=136, taps=TAPS9, operand=1), batch=9, csc=9, atomic=True, splitk=1, lens=[8, 0, 3, 8], rows_per_b=64,
             rows_inner=8, edges={"gather_b_dead_ktile", "gather_b_hint"}),
        case("gb_v8_dead", "gemm_bf16_v8_kernel<2,tn>", 200, 136, 256, "TN", modes={8: 2}, style="gatherB",
             geo=dict(GRID8, C=136, taps=TAPS9, operand=1), batch=9, csc=9, atomic=True, splitk=1, lens=[8, 0, 3, 8], rows_per_b=64,
             rows_inner=8, edges={"gather_b_dead_ktile", "gather_b_hint"}),
        # ---- the edges of the small structures once more on the 256 x 256 ones
        case("v4_odd", "gemm_bf16_v4_kernel<0,0,0>", 300, 265, 64, modes=V4, c_dt="bf16", bias=True, c_mis=2,
             edges={"odd_n_scalar", "one_ktile"}),
        case("v8_odd", "gemm_bf16_v8_kernel<0,nt>", 300, 265, 128, modes={**V8, 10: 0}, c_dt="bf16", bias=True, c_mis=2,
             edges={"odd_n_scalar"}),
        case("v4_resid", "gemm_bf16_v4_kernel<0,0,0>", 300, 264, 136, modes=V4, epi=R, alpha=0.5, bias=True, inplace=True,
             edges={"resid_inplace"}),
        case("v8_resid", "gemm_bf16_v8_kernel<0,nt>", 300, 264, 128, modes={**V8, 10: 0}, epi=R, alpha=0.5, bias=True, inplace=True,
             edges={"resid_inplace"}),
        case("v4_rowmap", "gemm_bf16_v4_kernel<0,0,0>", 200, 264, 128, modes=V4, bias=True,
             rowmap=dict(nI=4, nJ=5, OI=8, OJ=10, si=2, sj=2, oi=1, oj=0), edges={"rowmap_store"}),
        case("v8_rowmap", "gemm_bf16_v8_kernel<0,nt>", 200, 264, 128, modes={**V8, 10: 0}, c_dt="bf16", bias=True,
             rowmap=dict(nI=4, nJ=5, OI=8, OJ=10, si=2, sj=2, oi=1, oj=0), edges={"rowmap_store"}),
        case("v2_attn", "gemm_bf16_v2_kernel<0,0>", 200, 200, 64, style="attn", batch=4, edges={"two_level_batch"}),
        case("v4_attn", "gemm_bf16_v4_kernel<0,0,0>", 200, 200, 128, modes=V4, style="attn", batch=4, edges={"two_level_batch"}),
        case("v8_attn", "gemm_bf16_v8_kernel<0,nt>", 200, 200, 128, modes={**V8, 10: 0}, style="attn", batch=4, edges={"two_level_batch"}),
        # ---- real-valued operands on the remaining families
        case("v6_real", "gemm_bf16_v6_kernel<1>", 300, 264, 256, modes={**V4, 6: 1}, kind="real"),
        case("v5_real", "gemm_bf16_v5_kernel<store>", 5400, 1536, 512, modes={5: 2, 8: 0}, kind="real"),
        case("v8_half_real", "gemm_bf16_v8_kernel<half>", 16032, 512, 128, modes=V8, kind="real"),
        case("f32_valu_real", "gemm_f32_kernel", 33, 31, 7, modes={3: 0}, in_dt="f32", kind="real"),
        case("f32_mfma_real", "gemm_f32_mfma_kernel", 33, 31, 7, "NN", modes={3: 1}, in_dt="f32", kind="real"),
    ]
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# (structure family, edge) pairs tests/test_gemm_cases_host.py requires of the table; the families are the kernel templates
REQUIRED_EDGES = {
    "s": {"n129", "one_ktile", "tile_tail", "m_lt_tile", "odd_n_scalar", "k_mod8", "k_tail64", "odd_ktiles", "splitk_gt_nk",
          "colsum_tail", "two_level_batch", "resid_inplace", "relu_len0", "relu_full", "n324_vec3", "dropout"},
    "v2": {"n128", "one_ktile", "tile_tail", "odd_n_scalar", "k_mod8", "k_tail64", "odd_ktiles", "pitch_garbage", "splitk_uneven",
           "colsum_tail", "n324_vec3", "n324_vec2", "n324_vec0", "resid_inplace", "rowmap_store", "col_stride", "dropout",
           "gather_a", "gather_b", "gather_b_hint", "relu_len0", "relu_full", "plain_batch", "two_level_batch"},
    "v4": {"tile_tail", "k_tail64", "odd_ktiles", "one_ktile", "odd_n_scalar", "splitk_gt_nk", "colsum_tail", "n324_vec3", "dropout",
           "gather_a", "gather_b", "gather_b_hint", "gather_b_dead_ktile", "relu_len0", "relu_dead_tile", "gate_dead_tile",
           "resid_inplace", "rowmap_store", "two_level_batch"},
    "v8": {"tile_tail", "k_tail64", "odd_ktiles", "k_mod8", "odd_n_scalar", "splitk_uneven", "colsum_tail", "n324_vec2", "dropout",
           "v8_delay", "gather_a", "gather_b", "gather_b_hint", "gather_b_dead_ktile", "relu_len0", "relu_full", "relu_dead_tile",
           "gate_dead_tile", "resid_inplace", "rowmap_store", "two_level_batch"},
    "v5": {"tile_tail", "v5_short_last_round", "resid_inplace", "dropout"},
    "v6": {"dropout"},
    "f32": {"m_lt_tile", "k_mod8", "splitk_gt_nk"},
}
# grouped launches (ops.wgrad_grouped): (n_out, n_in) per problem, rows, split-K, modes
GROUPED = {
    "grouped_tn": dict(shapes=[(200, 136), (130, 64), (264, 129)], rows=200, splitk=3, modes={}),
    "grouped_tn8": dict(shapes=[(200, 136), (264, 264), (300, 129)], rows=328, splitk=2, modes={8: 3}),
}
# the four conv2 input-gradient launches (gathered dY, ReLU gate, row map): one per parity class into ONE grid
PARITY = dict(B=10, T1=9, F1=10, C=128, N=264)     # K = 128 .. 512; one full-width 256-column tile and a partial one
PARITY_MODES = {"v2": {8: 0, 4: 0}, "v4": V4, "v8": {8: 2}}
PARITY_KERNEL = {"v2": "gemm_bf16_v2_kernel<0,0>", "v4": "gemm_bf16_v4_kernel<0,0,1>", "v8": "gemm_bf16_v8_kernel<1,nt>"}


# ------------------------------------------------------------------------------------------------ operands
def exact_ints(shape, g, bits, erange, p_pos):
    """s * m * 2^e as float64 integers: m uniform over 1 .. 2^bits - 1, e over 0 .. erange, a quarter of the entries zero"""
    m = torch.randint(1, 2 ** bits, shape, generator=g).to(F64)
    e = torch.randint(0, erange + 1, shape, generator=g).to(F64)
    s = torch.where(torch.rand(shape, generator=g) < p_pos, 1.0, -1.0).to(F64)
    nz = (torch.rand(shape, generator=g) >= 0.25).to(F64)
    return m * 2.0 ** e * s * nz


def b_bits(K):
    """significand width of B: the widest (<= 8) that keeps the expected sum_k |a||b| (a: 8 bits, b: two exponents; 9/16 of the
    products non-zero: K * 54 * 2^bits) a factor 2 under 2^22 quanta"""
    return max(2, min(8, int(math.floor(math.log2(38836.0 / K)))))


def real_vals(shape, g, scale):
    return (torch.rand(shape, generator=g, dtype=F64) * 2 - 1) * scale


def stored(vals, trans, ld, dtype, garbage):
    """logical [nb, rows, K] -> storage [nb, rows, ld] (K contiguous; elements K .. roundup8(K) zero, as the contract asks) or
    [nb, K, ld] (reduction-major); what lies beyond is zero, or NaN where the case says the pitch holds garbage"""
    nb, rows, K = vals.shape
    fill = NAN if garbage else 0.0
    if trans:
        st = torch.full((nb, K, ld), fill, dtype=F64)
        st[..., :rows] = vals.transpose(1, 2)
    else:
        st = torch.full((nb, rows, ld), fill, dtype=F64)
        st[..., :K] = vals
        st[..., K:up8(K)] = 0.0
    return st.to(dtype)


class Problem:
    """CPU tensors (`t`), the scalar arguments of ops.gemm (`kw`), byte misalignments (`mis`) and the oracle's Expect (`e`)"""


@functools.lru_cache(maxsize=None)
def problem(name):
    c = BY_NAME[name]
    P = Problem()
    P.c = c
    M, N, K, Z = c["M"], c["N"], c["K"], c["batch"]
    tA, tB = c["lay"][0] == "T", c["lay"][1] == "N"
    idt, cdt, adt = TDT[c["in_dt"]], TDT[c["c_dt"]], TDT[c["aux_dt"]]
    g = torch.Generator().manual_seed(sum(map(ord, name)) * 7919 + M + N + K)
    exact = c["kind"] == "exact"
    bb = b_bits(K)
    # scale: pre-activations within about +-8 -- a power of two on A keeps everything exact.  sigma: the sum's spread from the
    # second moments of the two draws (3/4 non-zero; m uniform over 1 .. n: mean m^2 = (n + 1)(2n + 1) / 6; 4^e over {0, 1}: 2.5)
    m2 = lambda n: (n + 1) * (2 * n + 1) / 6.0
    sigma = math.sqrt(K * 0.75 * m2(255) * 0.75 * m2(2 ** bb - 1) * 2.5)
    P.q = q = 2.0 ** math.floor(math.log2(1.0 / sigma)) if exact else 1.0
    mkA = (lambda s: exact_ints(s, g, 8, 0, 0.7) * q) if exact else (lambda s: real_vals(s, g, 1.0))
    mkB = (lambda s: exact_ints(s, g, bb, 1, 0.4)) if exact else (lambda s: real_vals(s, g, 0.05))
    t, kw, P.mis = {}, dict(M=M, N=N, K=K, transA=tA, transB=tB, batch=Z, splitk=c["splitk"], atomic=c["atomic"], alpha=c["alpha"],
                            epi=c["epi"], c_col_stride=c["csc"]), {"C": c["c_mis"], "aux_out": c["c_mis"]}
    geo = c["geo"]
    lens = torch.tensor(c["lens"], dtype=torch.int64) if c["lens"] is not None else None
    pos_ok = None
    if lens is not None and geo is not None:   # positions (b, i, j) inside their utterance
        pos = torch.arange(len(c["lens"]) * geo["nI"] * geo["nJ"])
        pos_ok = ((pos % c["rows_per_b"]) // c["rows_inner"]) < lens[pos // c["rows_per_b"]]
    if c["style"] == "dense":
        a, b = mkA((Z, M, K)), mkB((Z, N, K))
        lda, ldb = (up8(M) if tA else up8(K)) + c["lda_pad"], (up8(N) if tB else up8(K))
        t["A"], t["B"] = stored(a, tA, lda, idt, c["garbage"]), stored(b, tB, ldb, idt, c["garbage"] and tB)
        kw.update(lda=lda, ldb=ldb, sA=(t["A"][0].numel() if Z > 1 else 0, 0), sB=(t["B"][0].numel() if Z > 1 else 0, 0))
        if idt == F32:   # fp32 operands have no pitch contract: dense rows
            t["A"], t["B"] = (a.transpose(1, 2) if tA else a).contiguous().to(idt), (b.transpose(1, 2) if tB else b).contiguous().to(idt)
            kw.update(lda=M if tA else K, ldb=N if tB else K)
    elif c["style"] == "attn":   # q and k head slices of one [B*T, 3d] matrix, scores [H, B, T, Tp]: test_gemm_batched_strided_bf16
        H = 4 if Z == 12 else 2
        Bn, T, dk, Tp = Z // H, M, K, up8(M) + 8 if M != 77 else 128
        d = H * dk
        qkv = torch.zeros(Bn * T + Tp, 3 * d, dtype=F64)   # zero rows behind the operand: a reduction may walk past its own rows
        qkv[:Bn * T, :d], qkv[:Bn * T, d:2 * d] = mkA((Bn * T, d)), mkB((Bn * T, d))
        qkv[:Bn * T, 2 * d:] = NAN                          # the v slice is not an operand of this product
        t["A"] = t["B"] = qkv.to(idt)
        kw.update(lda=3 * d, ldb=3 * d, nb0=Bn, sA=(T * 3 * d, dk), sB=(T * 3 * d, dk), sC=(T * Tp, Bn * T * Tp), b_off=d)
        c = dict(c, ldc=Tp)
    elif c["style"] == "gatherA":
        nb = M // (geo["nI"] * geo["nJ"])
        t["A"] = mkA((nb, geo["SI"], geo["SJ"], geo["C"])).to(idt)
        t["B"] = stored(mkB((1, N, K)), False, K, idt, False)
        kw.update(lda=geo["C"], ldb=K, gather=geo)
    else:                        # gatherB: A = dY [positions][channels] reduction-major, B = the activation grid
        nb = K // (geo["nI"] * geo["nJ"])
        a = mkA((1, M, K))
        if pos_ok is not None:   # the hint's promise: dY is zero beyond the utterances
            a = a * pos_ok.to(F64)
        t["A"] = stored(a, True, up8(M), idt, False)
        t["B"] = mkB((nb, geo["SI"], geo["SJ"], geo["C"])).to(idt)
        kw.update(lda=up8(M), ldb=geo["C"], nb0=Z, sC=(1, 0), gather=geo)
    S = 2 ** max(1, round(math.log2(max(sigma, 2.0)))) if exact else 1    # bias / residual / pre-fill: integers of about the sum's size
    ints = lambda shape, k=1: torch.randint(-k * S, k * S + 1, shape, generator=g).to(F64)
    if c["bias"]:
        t["bias"] = (ints((N,)) * q).to(F32) if exact else real_vals((N,), g, 1.0).to(F32)
    # C and aux geometry
    rows_c = M
    if c["rowmap"] is not None:
        r = c["rowmap"]
        rows_c = (M // (r["nI"] * r["nJ"])) * r["OI"] * r["OJ"]
        kw["rowmap"] = r
    ldc = c["ldc"] if c["ldc"] is not None else N * c["csc"]
    ldaux = c["ldaux"] if c["ldaux"] is not None else (ldc if c["csc"] == 1 else N)
    kw.update(ldc=ldc, ldaux=ldaux)
    if c["style"] == "attn":
        n_c = Z * M * ldc
    elif c["style"] == "gatherB":
        n_c = M * ldc
        kw["ldc"] = ldc = N * 9
        n_c = M * ldc
    else:
        n_c = Z * rows_c * ldc
        if Z > 1:
            kw["sC"] = (rows_c * ldc, 0)
    epi = c["epi"]
    qa = q * min(c["alpha"], 1.0)
    if c["atomic"]:
        t["C"] = (ints((n_c,), 4) * q).to(cdt)
    elif c["inplace"]:
        t["C"] = (ints((n_c,), 4) * qa).to(cdt)
    else:
        t["C"] = torch.full((n_c,), NAN, dtype=cdt)
    n_aux = Z * rows_c * ldaux
    if epi == GO.RESID and not c["inplace"]:
        t["aux_in"] = (ints((n_aux,), 4) * qa).to(F32)
    elif epi == GO.DSWISH:
        t["aux_in"] = real_vals((n_aux,), g, 6.0).to(adt)
    elif epi == GO.DSWISH_G:   # two significant bits: acc * factor stays a float32 number
        t["aux_in"] = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0, 3.0, -3.0])[
            torch.randint(0, 11, (n_aux,), generator=g)].to(adt)
    elif epi == GO.MUL_POS:
        t["aux_in"] = (real_vals((n_aux,), g, 2.0) * (torch.rand(n_aux, generator=g) > 0.2)).to(adt)
    if epi == GO.MUL_POS and lens is not None:   # the hint's promise: the gate is <= 0 on rows beyond their utterance's length
        mm = torch.arange(M)
        beyond = ((mm % c["rows_per_b"]) // c["rows_inner"]) >= lens[mm // c["rows_per_b"]]
        gate = t["aux_in"].view(-1, ldaux)
        rows_b = GO.row_map(mm, c["rowmap"])[beyond]
        gate[rows_b] = -gate[rows_b].abs()
    if epi in (GO.SWISH_DROP, GO.SWISH_DROP_G):
        t["aux_out"] = torch.full((n_aux,), NAN, dtype=adt)
    if lens is not None:
        t["row_len"] = lens
        kw.update(rows_per_b=c["rows_per_b"], rows_inner=c["rows_inner"])
    if c["colsum"]:
        t["colsum"] = (ints((M + 3,), 4) * q).to(F32)    # three more than the launch owns: they must stay
    P.drop = (c["p"], 7, 21)
    P.t, P.kw, P.adt = t, kw, adt
    P.e = oracle(P)
    return P


def oracle(P, **over):
    t = P.t
    return GO.gemm(t["A"], t["B"], t["C"], **{**P.kw, **over}, bias=t.get("bias"), drop=EO.Drop(*P.drop),
                   aux_in=t["C"] if P.c["inplace"] else t.get("aux_in"), aux_out=t.get("aux_out"), row_len=t.get("row_len"),
                   colsum_out=t.get("colsum"))


def exactness(P):
    """(worst sum_k |a||b| over the outputs, in quanta; the quantum)"""
    qq = P.q          # A carries the scale, B is integers
    return P.e.abs.max().item() / qq, qq


def desc_of(P, addr):
    """the GemmDesc of problem P from ops.gemm_desc -- the function ops.gemm itself fills its descriptor with -- with addr(name) for
    the address of every tensor that is there"""
    from nemo_amd import ops
    c = P.c
    code = lambda name: ops.BF16 if name == "bf16" else ops.F32
    A = lambda n: addr(n) if n in P.t else None
    aux_in = addr("C") if c["inplace"] else A("aux_in")
    return ops.gemm_desc(addr("A"), addr("B"), addr("C"), **P.kw, bias=A("bias"), drop=ops.Dropout(*P.drop), aux_in=aux_in,
                         aux_out=A("aux_out"), row_len=A("row_len"), colsum_out=A("colsum"), in_dtype=code(c["in_dt"]),
                         c_dtype=code(c["c_dt"]), aux_in_dtype=ops.F32 if c["epi"] == GO.RESID else code(c["aux_dt"]),
                         aux_out_dtype=code(c["aux_dt"]))


def fake_addr(P):
    """suitably (mis)aligned integers instead of device pointers: the plan looks at alignment only"""
    names = ["A", "B", "C", "bias", "aux_in", "aux_out", "row_len", "colsum"]
    return lambda n: (0x10000000 * (names.index(n) + 1) + P.mis.get(n, 0)) if n in P.t else 0


def plan_of(P, addr):
    """(rc, plan) under the case's modes"""
    from nemo_amd import ops
    with ops.gemm_modes(P.c["modes"]):
        return ops.gemm_plan(desc_of(P, addr))


# ------------------------------------------------------------------------------------------------ comparisons
def swish_grad_cond(h):
    """s * (1 + |h| (1 - s)) >= |swish'(h)|: the terms of swish' taken by magnitude.  swish' changes sign at h = -1.278; next to it
    the error relative to the value itself is unbounded in any arithmetic (the float32 CPU restatement: 3.3e-2 on these cases), so
    errors of swish' are measured and bounded against this sum"""
    s = GO.sigmoid(h)
    return s * (1.0 + h.abs() * (1.0 - s))


def half_ulp_bf16(ref):
    """half a bf16 ulp of |ref| (8 significant bits)"""
    return 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(1e-300) * (1 + TOL_DROP))) - 8)


def rounded(x64, dtype):
    return EO.round_to(x64, dtype).to(F64)


def assert_untouched(got, init, written, what):
    gb, ib = got.view(torch.int16 if got.dtype == BF16 else torch.int32), init.view(torch.int16 if init.dtype == BF16 else torch.int32)
    bad = (gb != ib) & ~written
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements outside the written set changed, first at {int(bad.nonzero()[0])}"


def assert_equal(got, ref64, where, what):
    """got == the float64 value rounded once to got's dtype, on `where`"""
    g, w = got.to(F64)[where], rounded(ref64, got.dtype)[where]
    bad = ~(g == w)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact value, first (index, " \
                                f"got, want): {int(bad.nonzero()[0])}, {g[bad][0].item()!r}, {w[bad][0].item()!r}"


def assert_bound(got, ref64, bound, where, what):
    g, r, b = got.to(F64)[where], ref64[where], bound[where]
    if got.dtype == BF16:
        b = b + half_ulp_bf16(r)
    err = (g - r).abs()
    ratio = torch.where(err == 0, 0.0, err / b.clamp_min(1e-300)).nan_to_num(float("inf"))
    worst = ratio.max().item() if ratio.numel() else 0.0
    print(f"{what}: worst element at {worst:.3f} of its bound")
    assert worst <= 1.0, f"{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements beyond their bound, worst {worst:.3f}x at " \
                         f"{int(ratio.argmax())} (got {g[ratio.argmax()].item()!r}, want {r[ratio.argmax()].item()!r})"


def check_c(P, got, what):
    """C's storage `got` (CPU) against the Expect"""
    c, e = P.c, P.e
    idx = e.ci.reshape(-1)
    w = e.written
    assert bool(torch.isfinite(got.float()[w]).all()), f"{what}: a written element is not finite"
    assert_untouched(got, P.t["C"], w, what)
    epi, p = c["epi"], c["p"]
    if c["kind"] == "real":
        bound = torch.zeros(e.C.numel(), dtype=F64)
        bound[idx] = (c["K"] * U * e.abs).reshape(-1)
        assert_bound(got, e.C, bound, w, what)
        return
    if epi in EXACT_EPIS and (p == 0.0 or epi in (GO.RELU_MASK, GO.MUL_POS, GO.DSWISH_G)):
        assert_equal(got, e.C, w, what)
        return
    # one value per written element from here on (non-atomic): logical order
    g, ref = got[idx], e.value.reshape(-1)
    keep = e.keep.reshape(-1)
    term = ref - (e.aux_in.reshape(-1) if epi == GO.RESID else 0.0)      # the masked, scaled part
    if p > 0.0 and epi != GO.RESID:
        nomask_nz = torch.ones_like(keep)
        if epi == GO.STORE:
            nomask_nz = e.pre.reshape(-1) != 0
        elif epi in (GO.SWISH_DROP, GO.SWISH_DROP_G):
            nomask_nz = e.pre.reshape(-1) != 0
        elif epi == GO.DSWISH:
            nomask_nz = (e.pre.reshape(-1) != 0) & (GO.swish_grad(e.aux_in.reshape(-1)) != 0)
        bad = ((g.to(F64) != 0) != keep) & nomask_nz
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements are not masked as drop_mask() defines"
    bound = TOL_DROP * term.abs() * (p > 0.0)
    if epi == GO.RESID:
        bound = bound + U * ref.abs()
    if epi in (GO.SWISH_DROP, GO.SWISH_DROP_G):
        bound = bound + TOL_SWISH["act"] * ref.abs()
    if epi == GO.DSWISH:
        bound = bound + TOL_SWISH["grad"] * (e.pre * e.keep * e.scale).reshape(-1).abs() * swish_grad_cond(e.aux_in.reshape(-1))
    assert_bound(g, ref, bound, torch.ones_like(keep), what)


def check_aux(P, got, what):
    c, e = P.c, P.e
    assert bool(torch.isfinite(got.float()[e.aux_written]).all()), f"{what}: a written element is not finite"
    assert_untouched(got, P.t["aux_out"], e.aux_written, what)
    if c["epi"] == GO.SWISH_DROP:
        assert_equal(got, e.aux, e.aux_written, what)        # the exact pre-activation
        return
    idx = e.ai.reshape(-1)
    g, ref, keep = got[idx], e.aux_value.reshape(-1), e.keep.reshape(-1)
    if c["p"] > 0.0:
        bad = ((g.to(F64) != 0) != keep) & (GO.swish_grad(e.pre.reshape(-1)) != 0)
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements are not masked as drop_mask() defines"
    bound = TOL_SWISH["grad"] * swish_grad_cond(e.pre.reshape(-1)) * keep * e.scale + TOL_DROP * (c["p"] > 0.0) * ref.abs()
    assert_bound(g, ref, bound, torch.ones_like(keep), what)


# ------------------------------------------------------------------------------------------------ the launches
def ops():
    from nemo_amd import ops as _ops
    return _ops


def launch(P):
    """one launch of problem P into fresh guarded buffers: {name: Guarded} of the outputs"""
    o = ops()
    o.set_step_counter(None)
    t, c = P.t, P.c
    d = {k: Guarded(v.shape, v.dtype, P.mis.get(k, 0) if k in ("C", "aux_out") else 0, src=v) for k, v in t.items() if k != "B" or t["B"] is not t["A"]}
    if "B" not in d:
        d["B"] = d["A"]
    addr = lambda n: d[n].t.data_ptr() if n in d else 0
    rc, plan = plan_of(P, addr)
    assert rc == 0 and KERNELS[plan[0]] == c["kernel"], (c["name"], rc, KERNELS[plan[0]] if rc == 0 else None)
    if "v8_delay" in c["edges"]:
        assert plan[7] > 0, "the key-9 delay does not apply to this shape"
    T = lambda n: d[n].t if n in d else None
    with o.gemm_modes(c["modes"]):
        o.gemm(T("A"), T("B"), T("C"), **{k: v for k, v in P.kw.items()}, bias=T("bias"), drop=o.Dropout(*P.drop),
               aux_in=T("C") if c["inplace"] else T("aux_in"), aux_out=T("aux_out"), row_len=T("row_len"), colsum_out=T("colsum"),
               in_dtype=o.BF16 if c["in_dt"] == "bf16" else o.F32)
        torch.cuda.synchronize()
        assert o.gemm_config(11, 0) == plan[1], (c["name"], o.gemm_config(11, 0), plan[1])
    assert_intact(**d)
    return d


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_gemm_kernel_against_float64(name):
    P = problem(name)
    outs = [launch(P) for _ in range(2)]
    for rep, d in enumerate(outs):
        what = f"{name} launch {rep}"
        check_c(P, d["C"].cpu(), what + " C")
        if "aux_out" in d:
            check_aux(P, d["aux_out"].cpu(), what + " aux_out")
        if "colsum" in d:
            got = d["colsum"].cpu()
            assert_untouched(got, P.t["colsum"], P.e.colsum_written, what + " colsum_out")
            assert_equal(got, P.e.colsum, P.e.colsum_written, what + " colsum_out")
        for k in ("A", "B", "bias", "aux_in", "row_len"):     # inputs are inputs
            if k in d and not (k == "aux_in" and P.c["inplace"]):
                assert torch.equal(d[k].cpu().view(torch.uint8), P.t[k].view(torch.uint8)), f"{what}: input {k} was written"
    if not P.c["atomic"]:
        for k in ("C", "aux_out"):
            if k in outs[0]:
                assert torch.equal(outs[0][k].cpu().view(torch.uint8), outs[1][k].cpu().view(torch.uint8)), f"{name}: two launches differ in {k}"


# ------------------------------------------------------------------------------------------------ grouped weight gradients
@functools.lru_cache(maxsize=None)
def grouped_problem(name):
    G = GROUPED[name]
    g = torch.Generator().manual_seed(len(name) * 131)
    rows, bb = G["rows"], b_bits(G["rows"])
    wide = exact_ints((rows, 480), g, 8, 0, 0.7).to(BF16)     # the first two problems slice columns of one matrix
    probs = []
    for i, (no, ni) in enumerate(G["shapes"]):
        if i < 2:
            dY, ldy, off = wide, 480, i * 208
        else:
            dY, ldy, off = exact_ints((rows, up8(no)), g, 8, 0, 0.7).to(BF16), up8(no), 0
        X = exact_ints((rows, up8(ni)), g, bb, 1, 0.4).to(BF16)
        dW = torch.randint(-4096, 4097, (no, ni), generator=g).to(F32)
        db = torch.randint(-4096, 4097, (no + 3,), generator=g).to(F32) if i != 1 else None
        probs.append((dY, ldy, off, X, up8(ni), 0, dW, no, ni, db))
    return probs, GO.wgrad_grouped(probs, rows)


@pytest.mark.parametrize("name", list(GROUPED))
def test_grouped_weight_gradients_against_float64(name):
    o = ops()
    o.set_step_counter(None)
    probs, exp = grouped_problem(name)
    G = GROUPED[name]
    for rep in range(2):
        dev_t, bufs, dprobs = {}, {}, []
        for i, (dY, ldy, off, X, ldx, xo, dW, no, ni, db) in enumerate(probs):
            for src in (dY, X):
                if id(src) not in dev_t:
                    dev_t[id(src)] = Guarded(src.shape, src.dtype, src=src)
            bufs[f"dW{i}"] = Guarded(dW.shape, F32, src=dW)
            if db is not None:
                bufs[f"db{i}"] = Guarded(db.shape, F32, src=db)
            dprobs.append((dev_t[id(dY)].t, ldy, off, dev_t[id(X)].t, ldx, xo, bufs[f"dW{i}"].t, no, ni, bufs[f"db{i}"].t if db is not None else None))
        with o.gemm_modes(G["modes"]):
            o.wgrad_grouped(dprobs, G["rows"], G["splitk"])
            torch.cuda.synchronize()
        assert_intact(**bufs)
        for i, (e, pr) in enumerate(zip(exp, probs)):
            assert e.abs.max().item() < QUANTA
            assert_equal(bufs[f"dW{i}"].cpu().reshape(-1), e.C, e.written, f"{name} launch {rep} dW{i}")
            if pr[9] is not None:
                got = bufs[f"db{i}"].cpu()
                assert_untouched(got, pr[9], e.colsum_written, f"{name} db{i}")
                assert_equal(got, e.colsum, e.colsum_written, f"{name} launch {rep} db{i}")


# ------------------------------------------------------------------------------------------------ row map: four parity classes, one grid
def parity_launches():
    """the four (M, K, gather, rowmap, weight image columns) of a stride-2 3x3 convolution's input gradient"""
    Q = PARITY
    T1, F1, Cc = Q["T1"], Q["F1"], Q["C"]
    T2, F2 = (T1 - 1) // 2 + 1, (F1 - 1) // 2 + 1
    out = []
    for pt in (0, 1):
        for pf in (0, 1):
            nI, nJ = (T1 - pt + 1) // 2, (F1 - pf + 1) // 2
            slots = [(kh, kw) for kh in ([1] if pt == 0 else [0, 2]) for kw in ([1] if pf == 0 else [0, 2])]
            taps = [(1 if kh == 0 else 0, 1 if kw == 0 else 0) for kh, kw in slots]
            out.append(dict(M=Q["B"] * nI * nJ, K=len(slots) * Cc, gather=dict(nI=nI, nJ=nJ, SI=T2, SJ=F2, C=Cc, si=1, sj=1, taps=taps),
                            rowmap=dict(nI=nI, nJ=nJ, OI=T1, OJ=F1, si=2, sj=2, oi=pt, oj=pf)))
    return out


@functools.lru_cache(maxsize=None)
def parity_problem():
    Q = PARITY
    g = torch.Generator().manual_seed(77)
    T2, F2 = (Q["T1"] - 1) // 2 + 1, (Q["F1"] - 1) // 2 + 1
    dy = (exact_ints((Q["B"], T2, F2, Q["C"]), g, 8, 0, 0.7) * 2.0 ** -12).to(BF16)
    gate = (real_vals((Q["B"] * Q["T1"] * Q["F1"], Q["N"]), g, 1.0) * (torch.rand(Q["B"] * Q["T1"] * Q["F1"], Q["N"], generator=g) > 0.2)).to(BF16)
    Ls = parity_launches()
    ws = [stored(exact_ints((1, Q["N"], L["K"]), g, b_bits(512), 1, 0.4), False, L["K"], BF16, False) for L in Ls]
    C0 = torch.full((Q["B"] * Q["T1"] * Q["F1"] * Q["N"],), NAN, dtype=F64)
    written = torch.zeros(C0.numel(), dtype=torch.bool)
    worst = 0.0
    for L, w in zip(Ls, ws):
        e = GO.gemm(dy, w, C0, L["M"], Q["N"], L["K"], Q["C"], L["K"], Q["N"], epi=GO.MUL_POS, aux_in=gate, ldaux=Q["N"],
                    gather=L["gather"], rowmap=L["rowmap"])
        assert not bool((written & e.written).any()), "two parity classes write the same element"
        C0, written, worst = e.C, written | e.written, max(worst, e.abs.max().item() / 2.0 ** -12)
    return dy, gate, Ls, ws, C0, written, worst


@pytest.mark.parametrize("family", list(PARITY_MODES))
def test_row_map_four_parity_classes_fill_one_grid(family):
    o = ops()
    o.set_step_counter(None)
    Q = PARITY
    dy, gate, Ls, ws, want, written, worst = parity_problem()
    assert bool(written.all()) and worst < QUANTA
    for dt_ in (F32, BF16):
        dx = Guarded((Q["B"] * Q["T1"] * Q["F1"], Q["N"]), dt_, fill=NAN)
        dyd, gd = Guarded(dy.shape, BF16, src=dy).t, Guarded(gate.shape, BF16, src=gate).t
        with o.gemm_modes(PARITY_MODES[family]):
            for L, w in zip(Ls, ws):
                wd = Guarded(w.shape, BF16, src=w).t
                args = (dyd, wd, dx.t, L["M"], Q["N"], L["K"], Q["C"], L["K"], Q["N"])
                kw = dict(epi=o.EPI_MUL_POS, aux_in=gd, ldaux=Q["N"], gather=L["gather"], rowmap=L["rowmap"])
                rc, plan = o.gemm_plan(o.gemm_desc(*args, **kw))
                assert rc == 0 and KERNELS[plan[0]] == PARITY_KERNEL[family], (family, L["K"], rc, KERNELS[plan[0]])
                o.gemm(*args, **kw)
                torch.cuda.synchronize()
        assert_intact(dx=dx)
        got = dx.cpu().reshape(-1)
        assert bool(torch.isfinite(got.float()).all()), "the four classes left a hole in the grid"
        assert_equal(got, want, written, f"parity grid {family} {dt_}")


# ------------------------------------------------------------------------------------------------ the measured Swish bound
def measure_swish(P):
    """worst per-element relative error of the float32 CPU restatement of swish_pair / swish_grad against float64 on P's own
    pre-activations: (activation, derivative)"""
    e, c = P.e, P.c
    if c["epi"] in (GO.SWISH_DROP, GO.SWISH_DROP_G):
        h = e.pre
    elif c["epi"] == GO.DSWISH:
        h = e.aux_in
    else:
        return None
    h32 = h.to(F32)
    s = 1.0 / (1.0 + torch.exp(-h32))
    sw = h32 * s
    act32, g32 = sw, sw * (1.0 - s) + s
    rel = lambda a, b, den: (((a.to(F64) - b).abs() / den)[den != 0]).max().item()
    return rel(act32, GO.swish(h), GO.swish(h).abs()), rel(g32, GO.swish_grad(h), swish_grad_cond(h)), h.abs().max().item()


if __name__ == "__main__":
    worst = [0.0, 0.0]
    for c_ in CASES:
        m_ = measure_swish(problem(c_["name"]))
        if m_ is not None:
            print(f"{c_['name']:12s} swish {m_[0]:.3e}  swish' {m_[1]:.3e}  max |h| {m_[2]:.2f}")
            worst = [max(worst[0], m_[0]), max(worst[1], m_[1])]
    print(f"measured: swish {worst[0]:.3e} -> bound {8 * worst[0]:.1e}; swish' {worst[1]:.3e} -> bound {8 * worst[1]:.1e}")
