"""float64 reference for nemo_amd/csrc/gemm.hip: `mi355x_gemm` and `mi355x_gemm_grouped` restated in plain torch on the CPU.

gemm() takes the arguments of nemo_amd.ops.gemm, with CPU tensors standing for the device storage, and returns an Expect: the
expected content of C, of aux_out and of colsum_out over their whole storage, the set of elements the kernel may write, and the
logical [batch, M, N] pieces the tests judge one by one (sum of products, its conditioning sum_k |a||b|, the pre-activation, the
dropout keep mask, the storage index of every element).  Operands arrive in their storage dtype and are up-cast, so a bf16 operand
is the bf16-rounded value: a kernel is then judged on its own arithmetic only.

Covered: the four operand layouts with pitches and element offsets; the two-level batch (z0 = z % nb0, z1 = z / nb0); a column
stride of C; split-K with atomic accumulation onto what C held; the gather of A rows and of the reduction-major B from a
channels-last grid (zero outside the grid); the row map; the eight epilogue codes with alpha and the bias added before the
epilogue; colsum_out.  The dropout mask is elementwise_oracle.keep_mask at idx = z*M*N + m*N + n.

tests/test_gemm_cases_host.py pins these closed forms to F.conv2d and its gradients, to direct strided indexing, to an einsum and
to the fp32 statements of tests/test_kernels_gpu.py.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elementwise_oracle as EO  # noqa: E402

F64 = torch.float64
STORE, SWISH_DROP, RESID, DSWISH, RELU_MASK, MUL_POS, SWISH_DROP_G, DSWISH_G = range(8)
NO_DROP = EO.Drop()


def _flat64(t):
    return t.detach().to("cpu").reshape(-1).to(F64)


def sigmoid(h):
    return 1.0 / (1.0 + torch.exp(-h))


def swish(h):
    return h * sigmoid(h)


def swish_grad(h):
    """d/dh h * sigmoid(h)"""
    s = sigmoid(h)
    return s * (1.0 + h * (1.0 - s))


class Expect:
    """what one launch must leave behind (whole-storage float64 vectors and bool masks) and its logical [Z, M, N] pieces"""
    __slots__ = ("acc", "abs", "pre", "keep", "scale", "ci", "ai", "value", "aux_value", "aux_in", "C", "written", "aux",
                 "aux_written", "colsum", "colsum_written")


def row_map(m, r):
    """storage row of logical row m = (b*nI + i)*nJ + j: (b*OI + i*si + oi)*OJ + j*sj + oj"""
    if r is None:
        return m
    per_b = r["nI"] * r["nJ"]
    b, rem = m // per_b, m % per_b
    i, j = rem // r["nJ"], rem % r["nJ"]
    return (b * r["OI"] + i * r["si"] + r["oi"]) * r["OJ"] + j * r["sj"] + r["oj"]


def gather_rows(src, base, g, rows, taps):
    """[rows, len(taps) * C]: position p = (b*nI + i)*nJ + j takes, for every tap t, the C channels of grid point
    (b, i*si + di[t], j*sj + dj[t]) of the channels-last [.., SI, SJ, C] grid that starts at element `base` of `src`; zero outside"""
    nI, nJ, SI, SJ, Cc = (g[k] for k in ("nI", "nJ", "SI", "SJ", "C"))
    p = torch.arange(rows)
    b, rem = p // (nI * nJ), p % (nI * nJ)
    i, j = rem // nJ, rem % nJ
    nb = (rows + nI * nJ - 1) // (nI * nJ)
    grid = src[base:base + nb * SI * SJ * Cc].view(nb, SI, SJ, Cc)
    out = []
    for di, dj in taps:
        ii, jj = i * g["si"] + di, j * g["sj"] + dj
        ok = (ii >= 0) & (ii < SI) & (jj >= 0) & (jj < SJ)
        out.append(grid[b, ii.clamp(0, SI - 1), jj.clamp(0, SJ - 1)] * ok[:, None].to(F64))
    return torch.cat(out, 1)


def _dense(src, base, rows, K, ld, trans):
    """[rows, K] view of an operand stored [rows][K] (trans = 0) or [K][rows] (trans = 1) with pitch ld"""
    return torch.as_strided(src, (rows, K), (1, ld) if trans else (ld, 1), base)


def gemm(A, B, Cm, M, N, K, lda, ldb, ldc, *, transA=False, transB=False, in_dtype=None, c_dtype=None, batch=1, nb0=0,
         sA=(0, 0), sB=(0, 0), sC=(0, 0), bias=None, alpha=1.0, epi=STORE, atomic=False, splitk=1, aux_in=None, aux_out=None,
         ldaux=0, drop=NO_DROP, row_len=None, rows_per_b=1, rows_inner=1, a_off=0, b_off=0, c_off=0, c_col_stride=1,
         colsum_out=None, colsum_off=0, colsum_stride=0, gather=None, rowmap=None, step_word=0):
    """the Expect of ops.gemm(...) with the same arguments.  Cm is C's storage as the launch finds it (only an atomic launch reads
    it); aux_out may be a tensor or just its element count; splitk does not change the value (an atomic launch adds the same sum
    in slices)."""
    e = Expect()
    Af, Bf = _flat64(A), _flat64(B)
    nb0 = nb0 if nb0 > 0 else batch
    ldaux = ldaux if ldaux else ldc
    csc = c_col_stride if c_col_stride > 0 else 1
    op = int(gather.get("operand", 0)) if gather is not None else -1
    acc = torch.empty(batch, M, N, dtype=F64)
    absum = torch.empty(batch, M, N, dtype=F64)
    coff = torch.empty(batch, dtype=torch.int64)
    colsum = None
    if colsum_out is not None:
        colsum = _flat64(colsum_out).clone()
        cs_written = torch.zeros(colsum.numel(), dtype=torch.bool)
    for z in range(batch):
        z0, z1 = z % nb0, z // nb0
        if op == 0:
            a = gather_rows(Af, a_off, gather, M, gather["taps"])
        else:
            a = _dense(Af, a_off + z0 * sA[0] + z1 * sA[1], M, K, lda, transA)
        if op == 1:
            b = gather_rows(Bf, b_off, gather, K, [gather["taps"][z]]).t()
        else:
            b = _dense(Bf, b_off + z0 * sB[0] + z1 * sB[1], N, K, ldb, transB)
        acc[z] = a @ b.t()
        absum[z] = a.abs() @ b.abs().t()
        coff[z] = z0 * sC[0] + z1 * sC[1]
        if colsum is not None:
            lo = colsum_off + z0 * colsum_stride
            colsum[lo:lo + M] += a.sum(1)
            cs_written[lo:lo + M] = True
    m, n = torch.arange(M), torch.arange(N)
    mr = row_map(m, rowmap)
    e.ci = c_off + coff[:, None, None] + mr[None, :, None] * ldc + n[None, None, :] * csc
    e.ai = coff[:, None, None] + mr[None, :, None] * ldaux + n[None, None, :]
    e.acc, e.abs = acc, absum
    e.pre = v = acc + (_flat64(bias)[:N] if bias is not None else 0.0)
    assert batch * M * N < 2 ** 32
    e.keep = EO.keep_mask(drop, 0, batch * M * N, step_word).view(batch, M, N)
    e.scale = float(drop.scale)
    dm = e.keep.to(F64) * e.scale
    e.aux_in = x = _flat64(aux_in)[e.ai] if aux_in is not None else None
    e.aux_value = None
    if epi == STORE:
        val = alpha * v * dm
    elif epi in (SWISH_DROP, SWISH_DROP_G):
        e.aux_value = v if epi == SWISH_DROP else swish_grad(v) * dm
        val = swish(v) * dm
    elif epi == RESID:
        val = x + alpha * v * dm
    elif epi == DSWISH:
        val = v * dm * swish_grad(x)
    elif epi == DSWISH_G:
        val = v * x
    elif epi == RELU_MASK:
        L = row_len.detach().cpu().to(torch.int64)
        ok = ((m % rows_per_b) // rows_inner) < L[m // rows_per_b]
        val = torch.where((v > 0) & ok[None, :, None], v, torch.zeros((), dtype=F64))
    elif epi == MUL_POS:
        val = torch.where(x > 0, v, torch.zeros((), dtype=F64))
    else:
        raise ValueError(epi)
    e.value = val
    e.C = _flat64(Cm).clone()
    e.written = torch.zeros(e.C.numel(), dtype=torch.bool)
    flat_ci = e.ci.reshape(-1)
    e.written[flat_ci] = True
    if atomic:
        e.C.index_add_(0, flat_ci, val.reshape(-1))
    else:
        assert int(e.written.sum()) == flat_ci.numel(), "a non-atomic launch writes every element once"
        e.C[flat_ci] = val.reshape(-1)
    e.aux = e.aux_written = None
    if e.aux_value is not None:
        n_aux = aux_out.numel() if isinstance(aux_out, torch.Tensor) else int(aux_out)
        e.aux = torch.full((n_aux,), float("nan"), dtype=F64)
        e.aux_written = torch.zeros(n_aux, dtype=torch.bool)
        e.aux[e.ai.reshape(-1)] = e.aux_value.reshape(-1)
        e.aux_written[e.ai.reshape(-1)] = True
    e.colsum, e.colsum_written = (colsum, cs_written) if colsum is not None else (None, None)
    return e


def wgrad_grouped(problems, rows):
    """mi355x_gemm_grouped through ops.wgrad_grouped: per problem (dY, ldy, y_off, X, ldx, x_off, dW, n_out, n_in, bias_grad) the
    Expect of dW[n_out, n_in] += dY[:, y_off:+n_out]^T @ X[:, x_off:+n_in] and bias_grad += column sums of that dY slice"""
    return [gemm(dY, X, dW, n_out, n_in, rows, ldy, ldx, n_in, transA=True, transB=True, atomic=True, a_off=y_off, b_off=x_off,
                 colsum_out=db)
            for dY, ldy, y_off, X, ldx, x_off, dW, n_out, n_in, db in problems]
