"""Thin Python wrappers over the C ABI (include/mi355x_asr.h): torch tensors in, device pointers + sizes out.

torch is used for device memory, streams and torch.distributed only.  Every function launches on
`torch.cuda.current_stream()` and returns immediately.  No CPU / eager fallbacks exist: a CPU tensor raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Optional

import torch

from ._lib import ConvGather, GemmDesc, PackEntry, RowMap, TransducerConf, TransducerGreedyDesc, TransducerLstmLayers, check, lib

F32, BF16 = 0, 1
EPI_STORE, EPI_SWISH_DROP, EPI_RESID, EPI_DSWISH, EPI_RELU_MASK, EPI_MUL_POS, EPI_SWISH_DROP_G, EPI_DSWISH_G = range(8)

_DT = {torch.float32: F32, torch.bfloat16: BF16}


def dt(t) -> int:
    try:
        return _DT[t.dtype if isinstance(t, torch.Tensor) else t]
    except KeyError:
        raise ValueError(f"unsupported dtype {t.dtype if isinstance(t, torch.Tensor) else t}")


def _ptr(t: Optional[torch.Tensor]) -> int:
    if t is None:
        return 0
    if not t.is_cuda:
        raise RuntimeError("nemo_amd kernels run on MI355X only: got a CPU tensor (there is no CPU fallback)")
    return t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class Dropout:
    """(key, threshold, scale) triple understood by the kernels; p == 0 -> off."""
    __slots__ = ("key", "threshold", "scale")

    def __init__(self, p: float = 0.0, seed: int = 0, site: int = 0):
        if p <= 0.0:
            self.key, self.threshold, self.scale = 0, 0, 1.0
        else:
            self.key = (seed * 0x9E3779B1 + site * 0x85EBCA77 + 0x1234567) & 0xFFFFFFFF
            self.threshold = max(1, min(0xFFFFFFFF, int(p * 4294967296.0)))
            self.scale = 1.0 / (1.0 - p)


NO_DROP = Dropout()

# when set to a list, every gemm() appends (variant, M, N, K, batch, start_event, end_event): bench.py's roofline pass
GEMM_PROFILE = None


def gemm_config(key: int, value: int) -> int:
    """kernel-structure knob (tests / A-B benchmarks), see mi355x_gemm_config in include/mi355x_asr.h: key 3 = fp32 problems on the
    matrix cores (1 default / 0 vector unit), key 5 = persistent overlapped-epilogue GEMM (0 off / 1 default), ...
    Returns the previous effective value (>= 0): writing it back restores the earlier state."""
    return lib.mi355x_gemm_config(key, value)


@contextlib.contextmanager
def gemm_modes(modes=None, **kv):
    """`with gemm_modes({8: 2, 5: 0}):` or `with gemm_modes(k8=2, k5=0):` -- gemm_config keys set for the block, the earlier values
    written back on exit"""
    modes = {**(modes or {}), **{int(k[1:]): v for k, v in kv.items()}}
    old = {}
    try:
        for k, v in modes.items():
            old[k] = gemm_config(k, v)
        yield
    finally:
        for k, v in old.items():
            gemm_config(k, v)


def gemm_plan(desc: GemmDesc):
    """(rc, [kernel id, key-11 code, grid x, y, z, workgroup size, dynamic LDS bytes, key-9 delay]) of the launch mi355x_gemm would
    make for `desc` under the current gemm_config modes -- see mi355x_gemm_plan; nothing is launched and no GPU is needed"""
    out = (C.c_int * 8)()
    rc = lib.mi355x_gemm_plan(C.byref(desc), C.byref(out))
    return rc, list(out)


# value added to the device-side step word per training step (odd: the word walks through all 2^32 values)
STEP_WORD_INC = -1640531535  # 0x9E3779B1 as int32


def set_step_counter(word: Optional[torch.Tensor]) -> None:
    """register (or, with None, clear) the device-side int32 step word that every dropout kernel issued from now on adds to its
    key at entry -- see mi355x_set_step_counter (include/mi355x_asr.h) and nemo_amd/graphs.py"""
    if word is not None and (word.dtype != torch.int32 or word.numel() != 1):
        raise ValueError("the step word is one int32 on the device")
    check(lib.mi355x_set_step_counter(_ptr(word)), "set_step_counter")


def wgrad_grouped(problems, rows, splitk):
    """problems: list of (dY, ldy, y_off, X, ldx, x_off, dW, n_out, n_in, bias_grad_or_None);
    dW[n_out, n_in] += dY[:, y_off:+n_out]^T @ X[:, x_off:+n_in] for all of them in ONE launch (bf16 in, f32 atomics)."""
    n = len(problems)
    arr = (GemmDesc * n)()
    for d, (dY, ldy, y_off, X, ldx, x_off, dW, n_out, n_in, bias_grad) in zip(arr, problems):
        d.A = _ptr(dY) + y_off * dY.element_size()
        d.B = _ptr(X) + x_off * X.element_size()
        d.C = _ptr(dW)
        d.M, d.N, d.K = n_out, n_in, rows
        d.lda, d.ldb, d.ldc = ldy, ldx, n_in
        d.c_col_stride = 1
        d.transA = d.transB = 1
        d.in_dtype, d.c_dtype = BF16, F32
        d.batch = d.nb0 = 1
        d.alpha = 1.0
        d.epilogue, d.atomic, d.splitk = EPI_STORE, 1, splitk
        d.colsum_out = _ptr(bias_grad) if bias_grad is not None else 0
    if GEMM_PROFILE is None:
        check(lib.mi355x_gemm_grouped(arr, n, _stream()), "gemm_grouped")
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(lib.mi355x_gemm_grouped(arr, n, _stream()), "gemm_grouped")
    e1.record()
    # recorded as one launch of the TN variant: sum of the problems' M*N, shared K
    GEMM_PROFILE.append(("bf16_TN", sum(q[7] * q[8] for q in problems), 1, rows, 1, e0, e1))


def gemm(A, B, Cm, M, N, K, lda, ldb, ldc, *, transA=False, transB=False, in_dtype=None, c_dtype=None, batch=1, nb0=0,
         sA=(0, 0), sB=(0, 0), sC=(0, 0), bias=None, alpha=1.0, epi=EPI_STORE, atomic=False, splitk=1, aux_in=None,
         aux_out=None, ldaux=0, drop: Dropout = NO_DROP, row_len=None, rows_per_b=1, rows_inner=1,
         a_off=0, b_off=0, c_off=0, c_col_stride=1, colsum_out=None, colsum_off=0, colsum_stride=0, gather=None,
         rowmap=None):
    """C[M,N] = epi(A @ B^T) -- see mi355x_gemm.  A/B/Cm are tensors whose storage holds the (strided) operands;
    *_off are element offsets into them (head / column slices)."""
    d = GemmDesc()
    esA, esC = A.element_size(), Cm.element_size()
    d.A = _ptr(A) + a_off * esA
    d.B = _ptr(B) + b_off * B.element_size()
    d.C = _ptr(Cm) + c_off * esC
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc = lda, ldb, ldc
    d.c_col_stride = c_col_stride
    d.transA, d.transB = int(transA), int(transB)
    d.in_dtype = dt(A) if in_dtype is None else in_dtype
    d.c_dtype = dt(Cm) if c_dtype is None else c_dtype
    d.batch, d.nb0 = batch, (nb0 if nb0 > 0 else batch)
    d.sA0, d.sA1 = sA
    d.sB0, d.sB1 = sB
    d.sC0, d.sC1 = sC
    d.bias = _ptr(bias)
    d.alpha = alpha
    d.epilogue, d.atomic, d.splitk = epi, int(atomic), splitk
    d.aux_in = _ptr(aux_in)
    d.aux_in_dtype = dt(aux_in) if aux_in is not None else 0
    d.aux_out = _ptr(aux_out)
    d.aux_out_dtype = dt(aux_out) if aux_out is not None else 0
    d.ldaux = ldaux if ldaux else ldc
    d.drop_key, d.drop_threshold, d.drop_scale = drop.key, drop.threshold, drop.scale
    d.row_len = _ptr(row_len)
    d.rows_per_b, d.rows_inner = rows_per_b, rows_inner
    d.colsum_out = (_ptr(colsum_out) + 4 * colsum_off) if colsum_out is not None else 0
    d.colsum_stride = colsum_stride
    keep = []
    if gather is not None:  # dict(nI, nJ, SI, SJ, C, si, sj, taps=[(di, dj), ...]): implicit-GEMM gather of the A operand
        g = ConvGather()
        g.nI, g.nJ, g.SI, g.SJ, g.C, g.si, g.sj = (gather[k] for k in ("nI", "nJ", "SI", "SJ", "C", "si", "sj"))
        g.ntaps = len(gather["taps"])
        g.operand = int(gather.get("operand", 0))
        for t, (di, dj) in enumerate(gather["taps"]):
            g.di[t], g.dj[t] = di, dj
        keep.append(g)
        d.gather = C.cast(C.pointer(g), C.c_void_p)
    if rowmap is not None:  # dict(nI, nJ, OI, OJ, si, sj, oi, oj): scattered C / aux rows
        r = RowMap()
        r.nI, r.nJ, r.OI, r.OJ, r.si, r.sj, r.oi, r.oj = (rowmap[k] for k in ("nI", "nJ", "OI", "OJ", "si", "sj", "oi", "oj"))
        keep.append(r)
        d.rowmap = C.cast(C.pointer(r), C.c_void_p)
    if GEMM_PROFILE is None:
        check(lib.mi355x_gemm(C.byref(d), _stream()), "gemm")
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(lib.mi355x_gemm(C.byref(d), _stream()), "gemm")
    e1.record()
    variant = ("bf16" if d.in_dtype == BF16 else "f32") + "_" + ("T" if transA else "N") + ("N" if transB else "T")
    GEMM_PROFILE.append((variant, M, N, K, batch, e0, e1))


# ------------------------------------------------------------------------------------------------ front-end
def logmel(audio, audio_len, window, fb_sparse, n_mels, *, hop=160, n_fft=512, preemph=0.97, dither=0.0, seed=0,
           log_guard=2.0 ** -24, out=None):
    B, S = audio.shape
    T = 1 + S // hop
    if out is None:
        out = torch.empty(B, n_mels, T, device=audio.device, dtype=torch.float32)
    st, ln, off, w = fb_sparse
    check(lib.mi355x_logmel_fwd(_ptr(audio), _ptr(audio_len), _ptr(window), window.numel(), hop, n_fft, _ptr(st), _ptr(ln),
                                _ptr(off), _ptr(w), n_mels, preemph if preemph is not None else 0.0, dither, seed & 0xFFFFFFFF,
                                log_guard, _ptr(out), B, S, T, _stream()), "logmel_fwd")
    return out


def feat_normalize(x, seq_len, out=None, normalize=True, pad_value=0.0, out_dtype=torch.float32):
    B, n_mels, T = x.shape
    if out is None:
        out = torch.empty(B, n_mels, T, device=x.device, dtype=out_dtype)
    check(lib.mi355x_feat_normalize(_ptr(x), _ptr(seq_len), _ptr(out), dt(out), B, n_mels, T, int(normalize), pad_value,
                                    _stream()), "feat_normalize")
    return out


# ------------------------------------------------------------------------------------------------ sub-sampling
def half_len(n, pad=1):
    """extent after one 3x3 stride-2 stage with `pad` zeros in front and one behind: pad 1 = Conv2d(padding=1), 2 = CausalConv2D"""
    return (n + pad - 2) // 2 + 1


def conv1_fwd(mel, w, bias, out, len0, len1, C_, pad=1):
    B, F, T = mel.shape
    check(lib.mi355x_subsample_conv1_fwd_pad(_ptr(mel), _ptr(w), _ptr(bias), _ptr(out), dt(out), _ptr(len0), _ptr(len1), B, F, T,
                                             C_, pad, _stream()), "subsample_conv1_fwd")


def conv1_bwd(dout, mel, len0, dw, db, C_, pad=1):
    B, F, T = mel.shape
    T1 = half_len(T, pad)
    n = ((T1 + 31) // 32) * B * 10 * C_
    sc = _scratch("conv1_bwd", n, dout.device)
    check(lib.mi355x_subsample_conv1_bwd_pad(_ptr(dout), dt(dout), _ptr(mel), _ptr(len0), _ptr(dw), _ptr(db), B, F, T, C_, pad,
                                             _ptr(sc), n, _stream()), "subsample_conv1_bwd")


def im2col(x, col, B, T1, F1, C_, pad=1):
    check(lib.mi355x_im2col_3x3s2_pad(_ptr(x), _ptr(col), dt(x), B, T1, F1, C_, pad, _stream()), "im2col")


def col2im_relu(dcol, act, din, B, T1, F1, C_, pad=1):
    check(lib.mi355x_col2im_3x3s2_relu_pad(_ptr(dcol), _ptr(act), _ptr(din), dt(dcol), B, T1, F1, C_, pad, _stream()), "col2im")


def dwconv2d_s2_fwd(x, w, bias, out, B, T1, F1, C_, pad=1):
    """depthwise 3x3 stride-2 conv on channels-last [B,T1,F1,C] -> [B,T2,F2,C]  ('dw_striding' sub-sampling)"""
    check(lib.mi355x_dwconv2d_s2_fwd_pad(_ptr(x), _ptr(w), _ptr(bias), _ptr(out), dt(x), B, T1, F1, C_, pad, _stream()),
          "dwconv2d_s2_fwd")


def dwconv2d_s2_bwd(dout, x, w, din, dw, dbias, B, T1, F1, C_, pad=1):
    T2, F2 = half_len(T1, pad), half_len(F1, pad)
    npos = B * T2 * F2
    nblk = (npos + 63) // 64 if npos < 1024 * 64 else 1024
    n = nblk * 10 * C_
    sc = _scratch("dwconv2d_bwd", n, dout.device)
    check(lib.mi355x_dwconv2d_s2_bwd_pad(_ptr(dout), _ptr(x), _ptr(w), _ptr(din), _ptr(dw), _ptr(dbias), dt(x), B, T1, F1, C_, pad,
                                         _ptr(sc), n, _stream()), "dwconv2d_s2_bwd")


# ------------------------------------------------------------------------------------------------ transducer head
def embed_sos_fwd(targets, emb, out, B, U, H, blank):
    check(lib.mi355x_embed_sos_fwd(_ptr(targets), _ptr(emb), _ptr(out), dt(out), B, U, H, blank, _stream()), "embed_sos_fwd")


def embed_sos_bwd(targets, dx, demb, B, U, H, blank):
    check(lib.mi355x_embed_sos_bwd(_ptr(targets), _ptr(dx), dt(dx), _ptr(demb), B, U, H, blank, _stream()), "embed_sos_bwd")


def lstm_cell_fwd(z, b_hh, c_prev, c, h, h_lp, B, H):
    check(lib.mi355x_lstm_cell_fwd(_ptr(z), _ptr(b_hh), _ptr(c_prev), _ptr(c), _ptr(h), _ptr(h_lp), dt(h_lp), B, H, _stream()),
          "lstm_cell_fwd")


def lstm_cell_bwd(dh, dc, act, c, c_prev, dz, B, H):
    check(lib.mi355x_lstm_cell_bwd(_ptr(dh), _ptr(dc), _ptr(act), _ptr(c), _ptr(c_prev), _ptr(dz), dt(dz), B, H, _stream()),
          "lstm_cell_bwd")


def joint_combine_fwd(f, g, h, B, T, U1, J, drop: Dropout = NO_DROP):
    check(lib.mi355x_joint_combine_fwd(_ptr(f), _ptr(g), _ptr(h), dt(h), drop.key, drop.threshold, drop.scale, B, T, U1, J,
                                       _stream()), "joint_combine_fwd")


def joint_combine_bwd(dh, h, df, B, T, U1, J, drop_scale=1.0):
    check(lib.mi355x_joint_combine_bwd(_ptr(dh), _ptr(h), _ptr(df), dt(h), drop_scale, B, T, U1, J, _stream()), "joint_combine_bwd")


def cast_rows(src, ld_in, dst, ld_out, M, N, Np, alpha=1.0):
    check(lib.mi355x_cast_rows(_ptr(src), ld_in, _ptr(dst), dt(dst), ld_out, M, N, Np, alpha, _stream()), "cast_rows")


# ------------------------------------------------------------------------------------------------ norms / reductions
def ffn_fwd(y, w1p, b1, w2p, b2, x, h, out, M, d, dff, alpha=0.5, drop_in: Dropout = NO_DROP, drop_res: Dropout = NO_DROP):
    """fused feed-forward block (mi355x_ffn_fwd): h = y @ W1^T + b1 (bf16, kept for backward), out = x + alpha * drop(drop(swish(h))
    @ W2^T + b2); w1p / w2p are the packed images of PackPlan.add_ffn (mi355x_ffn_pack).  d = 512 only."""
    check(lib.mi355x_ffn_fwd(_ptr(y), d, _ptr(w1p), _ptr(b1), _ptr(w2p), _ptr(b2), _ptr(x), d, _ptr(h), dff, _ptr(out), d, M, d, dff,
                             alpha, drop_in.key, drop_in.threshold, drop_in.scale, drop_res.key, drop_res.threshold,
                             drop_res.scale, _stream()), "ffn_fwd")


def ffn_pack(table_dev, n_entries, max_dff):
    check(lib.mi355x_ffn_pack(_ptr(table_dev), n_entries, max_dff, _stream()), "ffn_pack")


def ffn_bwd_dgrad(df, w2tp, w1tp, h, dh, act, dy, M, d, dff, drop_in: Dropout = NO_DROP):
    """input-gradient chain of the fused feed-forward block (mi355x_ffn_bwd_dgrad): dh, the recomputed activation `act` (both
    bf16 [M, dff], the weight-gradient operands) and dy = dh @ W1 (bf16 [M, d])"""
    check(lib.mi355x_ffn_bwd_dgrad(_ptr(df), d, _ptr(w2tp), _ptr(w1tp), _ptr(h), dff, _ptr(dh), _ptr(act), _ptr(dy), d, M, d, dff,
                                   drop_in.key, drop_in.threshold, drop_in.scale, _stream()), "ffn_bwd_dgrad")


def layernorm2_fwd(x, gamma1, beta1, y1, mean1, rstd1, gamma2, beta2, y2, mean2, rstd2, M, d, eps=1e-5):
    """y1 = LN1(x) (f32), y2 = LN2(y1) (dtype of y2) in one launch; d = 512"""
    check(lib.mi355x_layernorm2_fwd(_ptr(x), _ptr(gamma1), _ptr(beta1), _ptr(y1), _ptr(mean1), _ptr(rstd1), _ptr(gamma2), _ptr(beta2),
                                    _ptr(y2), dt(y2), _ptr(mean2), _ptr(rstd2), M, d, eps, _stream()), "layernorm2_fwd")


def layernorm_fwd(x, gamma, beta, y, mean, rstd, M, d, eps=1e-5):
    check(lib.mi355x_layernorm_fwd(_ptr(x), dt(x), _ptr(gamma), _ptr(beta), _ptr(y), dt(y), _ptr(mean), _ptr(rstd), M, d, eps,
                                   _stream()), "layernorm_fwd")


def layernorm_bwd(dy, x, gamma, mean, rstd, dres, accumulate, dgamma, dbeta, M, d, cast_out=None, cast_scale=1.0,
                  cast_drop: "Dropout" = None):
    """cast_out (bf16 [M,d], optional) = cast_scale * dropmask(cast_drop) * dres_new, written in the same pass"""
    if cast_out is None:
        check(lib.mi355x_layernorm_bwd(_ptr(dy), dt(dy), _ptr(x), dt(x), _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(dres),
                                       int(accumulate), _ptr(dgamma), _ptr(dbeta), M, d, _stream()), "layernorm_bwd")
    else:
        dr = cast_drop if cast_drop is not None else NO_DROP
        check(lib.mi355x_layernorm_bwd_cast(_ptr(dy), dt(dy), _ptr(x), dt(x), _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(dres),
                                            int(accumulate), _ptr(dgamma), _ptr(dbeta), M, d, _ptr(cast_out), cast_scale,
                                            dr.key, dr.threshold, dr.scale, _stream()), "layernorm_bwd_cast")


def layernorm2_bwd(dy1, x1, gamma1, mean1, rstd1, dgamma1, dbeta1, dres_in, x2, gamma2, mean2, rstd2, dgamma2, dbeta2, dres_out,
                   M, d, cast_out=None, cast_scale=1.0, cast_drop: "Dropout" = None):
    """backward of layernorm2_fwd's pair in one launch (include/mi355x_asr.h: mi355x_layernorm2_bwd)"""
    dr = cast_drop if cast_drop is not None else NO_DROP
    check(lib.mi355x_layernorm2_bwd(_ptr(dy1), dt(dy1), _ptr(x1), _ptr(gamma1), _ptr(mean1), _ptr(rstd1), _ptr(dgamma1),
                                    _ptr(dbeta1), _ptr(dres_in), _ptr(x2), _ptr(gamma2), _ptr(mean2), _ptr(rstd2), _ptr(dgamma2),
                                    _ptr(dbeta2), _ptr(dres_out), M, d, _ptr(cast_out), cast_scale, dr.key, dr.threshold, dr.scale,
                                    _stream()), "layernorm2_bwd")


def colsum(x, out, M, N, ld=None, alpha=1.0, x_off=0):
    check(lib.mi355x_colsum(_ptr(x) + x_off * x.element_size(), dt(x), ld if ld is not None else N, _ptr(out), M, N, alpha,
                            _stream()), "colsum")


def log_softmax_fwd(logits, ld_in, logp, ld_out, M, C_):
    check(lib.mi355x_log_softmax_fwd(_ptr(logits), ld_in, _ptr(logp), ld_out, M, C_, _stream()), "log_softmax_fwd")


def log_softmax_bwd(dlogp, logp, ld, dlogits, ld_out, M, C_, scale=1.0):
    check(lib.mi355x_log_softmax_bwd(_ptr(dlogp), _ptr(logp), ld, _ptr(dlogits), dt(dlogits), ld_out, M, C_, scale, _stream()),
          "log_softmax_bwd")


# ------------------------------------------------------------------------------------------------ block glue
def glu_fwd(x, out, lens, T, M, d, cu=None):
    """cu (i64 [B+1], "packed rows"): x holds the valid frames only (utterance b at rows cu[b] ..), out is the padded [B*T, d] grid"""
    check(lib.mi355x_glu_fwd(_ptr(x), _ptr(out), dt(x), _ptr(lens), T, M, d, _ptr(cu), _stream()), "glu_fwd")


def glu_bwd(x, dout, din, lens, T, M, d, cu=None):
    check(lib.mi355x_glu_bwd(_ptr(x), _ptr(dout), _ptr(din), dt(x), _ptr(lens), T, M, d, _ptr(cu), _stream()), "glu_bwd")


def rows_pack(src, dst, lens, cu, T, M, width, ld_src=None, ld_dst=None):
    """dst[cu[b] + t, :width] = src[b*T + t, :width] for t < lens[b]   (padded grid -> packed rows; M = B * T)"""
    check(lib.mi355x_rows_pack(_ptr(src), _ptr(dst), dt(src), ld_src or width, ld_dst or width, _ptr(lens), _ptr(cu), T, M, width, 0,
                               _stream()), "rows_pack")


def rows_unpack(src, dst, lens, cu, T, M, width, ld_src=None, ld_dst=None):
    """dst[b*T + t, :width] = src[cu[b] + t, :width] if t < lens[b] else 0   (packed rows -> padded grid, zero rows beyond)"""
    check(lib.mi355x_rows_pack(_ptr(src), _ptr(dst), dt(src), ld_src or width, ld_dst or width, _ptr(lens), _ptr(cu), T, M, width, 1,
                               _stream()), "rows_unpack")


# ------------------------------------------------------------------------------------------------ Squeezeformer glue
def scale_bias_fwd(x, scale, bias, y, M, d, ld):
    check(lib.mi355x_scale_bias_fwd(_ptr(x), _ptr(scale), _ptr(bias), _ptr(y), dt(y), M, d, ld, _stream()), "scale_bias_fwd")


def scale_bias_bwd(dy, ld, x, scale, dres, dscale, dbias, M, d):
    sc = _scratch("scale_bias_bwd", min(M, 512) * 2 * d, dy.device) if dscale is not None else None
    check(lib.mi355x_scale_bias_bwd(_ptr(dy), dt(dy), ld, _ptr(x), _ptr(scale), _ptr(dres), _ptr(dscale), _ptr(dbias), M, d,
                                    _ptr(sc), sc.numel() if sc is not None else 0, _stream()), "scale_bias_bwd")


def cast_pitched(x, y, M, d, ld, alpha=1.0, drop: Dropout = NO_DROP):
    check(lib.mi355x_cast_pitched(_ptr(x), _ptr(y), dt(y), M, d, ld, alpha, drop.key, drop.threshold, drop.scale, _stream()),
          "cast_pitched")


def swish_mask_fwd(x, out, lens, T, M, C_):
    check(lib.mi355x_swish_mask_fwd(_ptr(x), _ptr(out), dt(x), _ptr(lens), T, M, C_, _stream()), "swish_mask_fwd")


def swish_mask_bwd(x, dout, din, lens, T, M, C_):
    check(lib.mi355x_swish_mask_bwd(_ptr(x), _ptr(dout), _ptr(din), dt(x), _ptr(lens), T, M, C_, _stream()), "swish_mask_bwd")


def time_reduce_dwconv_fwd(x, lens, w, bias, out, B, T, d, ld):
    check(lib.mi355x_time_reduce_dwconv_fwd(_ptr(x), _ptr(lens), _ptr(w), _ptr(bias), _ptr(out), dt(out), B, T, d, ld, _stream()),
          "time_reduce_dwconv_fwd")


def time_reduce_dwconv_bwd(dout, ld, x, lens, w, dx, dw, dbias, B, T, d):
    check(lib.mi355x_time_reduce_dwconv_bwd(_ptr(dout), dt(dout), ld, _ptr(x), _ptr(lens), _ptr(w), _ptr(dx), _ptr(dw), _ptr(dbias),
                                            B, T, d, _stream()), "time_reduce_dwconv_bwd")


def time_recover_fwd(skip, ys, out, B, T, d):
    check(lib.mi355x_time_recover_fwd(_ptr(skip), _ptr(ys), _ptr(out), B, T, d, _stream()), "time_recover_fwd")


def time_recover_bwd(dx, dys, B, T, d, ld):
    check(lib.mi355x_time_recover_bwd(_ptr(dx), _ptr(dys), dt(dys), B, T, d, ld, _stream()), "time_recover_bwd")


def drop_scale_cast(x, out, n, alpha=1.0, drop: Dropout = NO_DROP):
    check(lib.mi355x_drop_scale_cast(_ptr(x), dt(x), _ptr(out), dt(out), n, alpha, drop.key, drop.threshold, drop.scale,
                                     _stream()), "drop_scale_cast")


def qbias(qkv, ldq, u, v, qu, qv, M, d):
    check(lib.mi355x_qbias(_ptr(qkv), ldq, _ptr(u), _ptr(v), _ptr(qu), _ptr(qv), dt(qkv), M, d, _stream()), "qbias")


def _ctc_greedy(level, logp, lens, blank, *conf_args):
    """one call of the greedy CTC entry of `level` (0: tokens, 1: and frames, 2: and confidences, `conf_args` = what that entry takes
    behind `blank`): allocates the level's outputs -> (tokens, out_len, score[, tok_start, tok_end[, frame_conf, tok_conf]])"""
    entry, name = {0: (lib.mi355x_ctc_greedy_decode, "ctc_greedy_decode"), 1: (lib.mi355x_ctc_greedy_decode_ts, "ctc_greedy_decode_ts"),
                   2: (lib.mi355x_ctc_greedy_decode_conf, "ctc_greedy_decode_conf")}[level]
    B, T, C_ = logp.shape
    i32, f32 = (dict(dtype=d, device=logp.device) for d in (torch.int32, torch.float32))
    tokens, out_len, score = torch.empty(B, T, **i32), torch.empty(B, **i32), torch.empty(B, **f32)
    extra = []   # what the level adds behind `score`
    if level >= 1:
        extra += [torch.empty(B, T, **i32), torch.empty(B, T, **i32)]   # tok_start, tok_end
    if level >= 2:
        extra += [torch.empty(B, T, **f32), torch.empty(B, T, **f32)]   # frame_conf, tok_conf
    check(entry(_ptr(logp), _ptr(lens), _ptr(tokens), _ptr(out_len), _ptr(score), *[_ptr(t) for t in extra], B, T, C_, blank,
                *conf_args, _stream()), name)
    return (tokens, out_len, score, *extra)


def ctc_greedy_decode(logp, lens, blank):
    """logp f32 [B,T,C] -> (tokens i32 [B,T] folded / blank-free / -1 padded, out_len i32 [B], score f32 [B])"""
    return _ctc_greedy(0, logp, lens, blank)


def ctc_greedy_decode_ts(logp, lens, blank):
    """ctc_greedy_decode plus the frames: -> (tokens, out_len, score, tok_start i32 [B,T], tok_end i32 [B,T]); start / end = first /
    last frame of the run of equal arg-max labels behind each kept token, -1 padded"""
    return _ctc_greedy(1, logp, lens, blank)


def ctc_greedy_decode_conf(logp, lens, blank, method, aggregation=1, exclude_blank=True):
    """ctc_greedy_decode_ts plus confidences (mi355x_ctc_greedy_decode_conf): `method` = (method, norm, alpha, k0, k1, k2) for
    V = C (modules.confidence.ConfidenceMethodConfig.kernel_args), aggregation 0..3 = mean / min / max / prod -> (tokens, out_len,
    score, tok_start, tok_end, frame_conf f32 [B,T]: 0.0 beyond the utterance, tok_conf f32 [B,T]: the aggregation of frame_conf
    over each token's frames (exclude_blank: its own run; else from behind the previous token's run), 0.0 padded)"""
    return _ctc_greedy(2, logp, lens, blank, *method, int(aggregation), int(bool(exclude_blank)))


def ctc_align(logp, targets, in_len, tgt_len, blank):
    """Viterbi forced alignment (mi355x_ctc_align): logp f32 [B,T,C] contiguous, targets i64 [B,U], in_len / tgt_len i64 [B] ->
    (path i32 [B,T]: state 0..2U per frame, tok_start i32 [B,U], tok_end i32 [B,U]: first / last frame of each label, score f32 [B]);
    -1 padded; an infeasible utterance has score -inf and -1 everywhere"""
    B, T, C_ = logp.shape
    U = targets.shape[1]
    if U == 0:   # (a batch of empty transcripts: the kernel wants a column to point at)
        if int(tgt_len.max()) > 0:
            raise ValueError("ctc_align: target lengths exceed the width of `targets` (0)")
        targets = targets.new_zeros(B, 1)
    Uk = targets.shape[1]
    bp = torch.empty(B * T * ((Uk + 8) & ~7), dtype=torch.uint8, device=logp.device)
    path = torch.empty(B, T, dtype=torch.int32, device=logp.device)
    tok_start, tok_end = (torch.empty(B, Uk, dtype=torch.int32, device=logp.device) for _ in range(2))
    score = torch.empty(B, dtype=torch.float32, device=logp.device)
    check(lib.mi355x_ctc_align(_ptr(logp), _ptr(targets), _ptr(in_len), _ptr(tgt_len), _ptr(bp), _ptr(path), _ptr(tok_start),
                               _ptr(tok_end), _ptr(score), B, T, C_, Uk, blank, _stream()), "ctc_align")
    return path, tok_start[:, :U], tok_end[:, :U], score


class _CTCBeamStateC(C.Structure):   # mi355x_ctc_beam_stream_state
    _fields_ = [(n, C.c_void_p) for n in ("node", "par", "tok", "len", "h", "hp", "pb", "pnb", "tot", "brank", "lm_state", "lm_sum",
                                           "nb", "frames_done")]

    @classmethod
    def of(cls, state):
        a = state.arrays()
        return cls(**{n: (_ptr(a[n]) if n in a else None) for n, _ in cls._fields_})


class _CTCBeamFusionC(C.Structure):   # mi355x_ctc_beam_fusion
    _fields_ = ([(n, C.c_void_p) for n in ("state_arc_begin", "arc_tok", "arc_logp", "arc_next", "state_bo", "state_bo_next",
                                            "state_final")] +
                [("n_states", C.c_int), ("n_arcs", C.c_int), ("alpha", C.c_float), ("ub", C.c_float)])


class _CTCBeamFusedStateC(C.Structure):   # mi355x_ctc_beam_fused_state
    _fields_ = [("beams", _CTCBeamStateC), ("fs_state", C.c_void_p), ("fs_sum", C.c_void_p)]

    @classmethod
    def of(cls, state):
        a = state.arrays()
        return cls(beams=_CTCBeamStateC.of(state), fs_state=_ptr(a["fs_state"]) if "fs_state" in a else None,
                   fs_sum=_ptr(a["fs_sum"]) if "fs_sum" in a else None)


class _CTCBeamWindowC(C.Structure):   # mi355x_ctc_beam_window
    _fields_ = [(n, C.c_void_p) for n in ("tok_base", "frame_base", "kept", "frame_map")]

    @classmethod
    def of(cls, state):
        a = state.window_arrays()
        w = cls(**{n: _ptr(t) for n, t in a.items()})
        w.keep = a   # (an uncommitted state's all-zero window lives as long as the record)
        return w


def _ctc_beam_lm_check(what, lm, logp):
    """`lm` of the entries that take one n-gram model: an NGramLM over the labels of `logp`"""
    from .modules.ngram_lm import NGramLM
    if not isinstance(lm, NGramLM):
        raise TypeError(f"{what}: `lm` must be an NGramLM, got {type(lm).__name__}")
    if lm.vocab_size != logp.shape[2] - 1:
        raise ValueError(f"{what}: the LM has {lm.vocab_size} labels, the log-probabilities {logp.shape[2]} classes "
                         f"(labels + the blank)")


def _ctc_beam_fusion_check(what, models, logp):
    """`models` = [(NGramLM | BoostingTree, alpha), ...], one or two, over the labels of `logp`"""
    from .modules.ngram_lm import NGramLM
    models = list(models) if models is not None else []
    if not 1 <= len(models) <= 2:
        raise ValueError(f"{what}: `models` must hold one or two (model, alpha) pairs, got {len(models)}")
    for i, pair in enumerate(models):
        if not (isinstance(pair, (tuple, list)) and len(pair) == 2 and isinstance(pair[0], NGramLM)):
            got = type(pair[0]).__name__ if isinstance(pair, (tuple, list)) and len(pair) else type(pair).__name__
            raise TypeError(f"{what}: `models` holds (NGramLM | BoostingTree, alpha) pairs, got {got}")
        if pair[0].vocab_size != logp.shape[2] - 1:
            raise ValueError(f"{what}: model {i} has {pair[0].vocab_size} labels, the log-probabilities {logp.shape[2]} classes "
                             f"(labels + the blank)")
    return models


class _CTCBeamSixTables:
    """a model as the entries that take one n-gram model pass it on: its six tables, without a BoostingTree's `state_final`"""

    def __init__(self, model):
        self.model, self.num_states, self.num_arcs, self.lm_ub = model, model.num_states, model.num_arcs, model.lm_ub

    def to(self, device):
        return self.model.to(device)[:6]


def _ctc_beam_fusion_array(models, logp):
    """the `mi355x_ctc_beam_fusion` array of checked `models` and the tensors it points into"""
    arr, keep = (_CTCBeamFusionC * len(models))(), []
    for i, (m, alpha) in enumerate(models):
        tables = m.to(logp.device)   # (cached on the model: they outlive the launch)
        keep.append(tables)
        arr[i] = _CTCBeamFusionC(*(_ptr(t) for t in tables[:6]), _ptr(tables[6]) if len(tables) > 6 else None, m.num_states,
                                 m.num_arcs, float(alpha), float(m.lm_ub))
    return arr, keep


def _ctc_beam_checked(models, fused, logp, suffix):
    """the models of a call as its public entry checks and passes them on, and that entry's name for messages (`suffix`: '' or
    '_stream').  `fused`: the entries that take (NGramLM | BoostingTree, alpha) pairs; else the ones that take no model or one n-gram
    model, of which six tables reach the kernel"""
    if fused:
        what = "ctc_beam_decode_fused" + suffix
        return what, _ctc_beam_fusion_check(what, models, logp)
    what = "ctc_beam_decode" + (suffix if suffix or not models else "_lm")
    for lm, _ in models:
        _ctc_beam_lm_check(what, lm, logp)
    return what, [(_CTCBeamSixTables(lm), alpha) for lm, alpha in models]


def _ctc_beam_search(what, logp, lens, blank, beam_size, beam_threshold, beam_beta, models):
    """the one-shot search behind every public entry: `models` = [(NGramLM | BoostingTree, alpha), ...], checked by the caller, none
    (mi355x_ctc_beam_decode) to two (mi355x_ctc_beam_decode_fused); `what` names the caller where the library refuses the arguments"""
    B, T, C_ = logp.shape
    W = int(beam_size)
    if lens is None:
        lens = torch.full((B,), T, dtype=torch.int64, device=logp.device)
    i32, f32 = (dict(dtype=d, device=logp.device) for d in (torch.int32, torch.float32))
    ws = torch.empty(B * max(2, int(lib.mi355x_ctc_beam_workspace_elems(T, W))), **i32)   # (a fresh allocation: 8-byte aligned)
    Wa = max(W, 0)   # (a width the entry refuses still reaches it, for its ValueError)
    tokens, tok_frame = torch.empty(B, Wa, T, **i32), torch.empty(B, Wa, T, **i32)
    hyp_len, score, n_hyp = torch.empty(B, Wa, **i32), torch.empty(B, Wa, **f32), torch.empty(B, **i32)
    arr, keep = _ctc_beam_fusion_array(models, logp)
    entry, fusion = ((lib.mi355x_ctc_beam_decode_fused, (C.cast(arr, C.c_void_p), len(arr))) if models else
                     (lib.mi355x_ctc_beam_decode, ()))
    check(entry(_ptr(logp), _ptr(lens), _ptr(ws), _ptr(tokens), _ptr(tok_frame), _ptr(hyp_len), _ptr(score), _ptr(n_hyp), B, T, C_,
                int(blank), W, float(beam_threshold), float(beam_beta), *fusion, _stream()), what)
    return tokens, tok_frame, hyp_len, score, n_hyp


def _ctc_beam_search_stream(what, logp, lens, blank, beam_size, beam_threshold, beam_beta, state, models, emit):
    """one chunk of the resumable search behind every public entry (mi355x_ctc_beam_decode_stream without a model, else
    mi355x_ctc_beam_decode_fused_stream; from a committed state mi355x_ctc_beam_decode_window_stream, whose n-best holds the tails
    behind `state.committed`): `_ctc_beam_search`'s arguments, `state` a CTCBeamStreamState of this batch, width and model
    count (None: fresh streams) -> (the n-best so far in the state's buffers, or None with emit=False; the next state)"""
    from .modules.ctc_decoding import CTCBeamStreamState
    B, T, C_ = logp.shape
    W = int(beam_size)
    if state is None:
        state = CTCBeamStreamState.fresh(B, W, logp.device, lm=len(models) >= 1, second=len(models) == 2)
    if state.B != B or state.W != W or int(state.lm) + (state.fs is not None) != len(models):
        raise ValueError(f"{what}: the state is of {state.B} streams, {state.W} beams, "
                         f"{int(state.lm) + (state.fs is not None)} fusion models; the call of {B}, {W}, {len(models)}")
    if lens is None:
        lens = torch.full((B,), T, dtype=torch.int64, device=logp.device)
    state.reserve(T)
    nxt = state.next(T)
    i32, f32 = (dict(dtype=d, device=logp.device) for d in (torch.int32, torch.float32))
    outs = (state.tokens, state.tok_frame, torch.empty(B, W, **i32), torch.empty(B, W, **f32), torch.empty(B, **i32)) if emit else None
    arr, keep = _ctc_beam_fusion_array(models, logp)
    entry, fusion = ((lib.mi355x_ctc_beam_decode_fused_stream, (C.cast(arr, C.c_void_p), len(arr))) if models else
                     (lib.mi355x_ctc_beam_decode_stream, ()))
    window = ()
    if state.win is not None:   # a committed state: the search that reads its window (the outputs hold the tails)
        entry, fusion = lib.mi355x_ctc_beam_decode_window_stream, (C.cast(arr, C.c_void_p) if models else None, len(arr))
        win = _CTCBeamWindowC.of(state)
        window = (C.byref(win),)
    s_in, s_out = _CTCBeamFusedStateC.of(state), _CTCBeamFusedStateC.of(nxt)   # (the model-less entry's state is its first member)
    check(entry(_ptr(logp), _ptr(lens), _ptr(state.tree), *((_ptr(t) for t in outs) if emit else (None,) * 5), B, T, C_, int(blank), W,
                float(beam_threshold), float(beam_beta), *fusion, state.capacity, C.byref(s_in), C.byref(s_out), *window, _stream()),
          what)
    return outs, nxt


def ctc_beam_commit(state, stable_frames=None):
    """commit the stable prefix of every stream of `state` (a `modules.CTCBeamStreamState`; mi355x_ctc_beam_commit, which
    include/mi355x_asr.h states): the tokens every live hypothesis shares leave the tree, which is re-rooted and compacted into a
    new tree of the same capacity.  `stable_frames` = S >= 0 forces it: only the beams that agree with the best one on everything
    older than S frames survive, and at most S frames stay in the tree.  None: the exact commit, which changes no result.
    -> ([(token ids, global frames)] newly committed per stream, the committed state).  Out of place: `state` stays what it was.
    One D2H copy of [4, B] integers (the window and the counts, from which the new state's host `bound` is taken) and one of the
    new tokens."""
    from .modules.ctc_decoding import CTCBeamStreamState
    S = -1 if stable_frames is None else int(stable_frames)
    if S < -1:
        raise ValueError(f"ctc_beam_commit: stable_frames must be None or >= 0; got {stable_frames}")
    B, W, cap, dev_ = state.B, state.W, state.capacity, state.device
    i32 = dict(dtype=torch.int32, device=dev_)
    out = CTCBeamStreamState(torch.empty_like(state.h64), torch.empty_like(state.beams), torch.empty_like(state.utt),
                             torch.empty_like(state.tree),   # (only the frames the commit keeps, then the search's, are ever read)
                             state.tokens, state.tok_frame, state.lm, 0, fs=None if state.fs is None else torch.empty_like(state.fs),
                             win=torch.empty(4, B, **i32), frame_map=torch.empty(B, cap, **i32), steps=state.steps)
    com = torch.empty(2, B, cap, **i32)
    ws = torch.empty(B * max(1, int(lib.mi355x_ctc_beam_commit_workspace_elems(cap, W))), **i32)
    s_in, s_out = _CTCBeamFusedStateC.of(state), _CTCBeamFusedStateC.of(out)
    w_in, w_out = _CTCBeamWindowC.of(state), _CTCBeamWindowC.of(out)
    check(lib.mi355x_ctc_beam_commit(C.byref(s_in), C.byref(w_in), _ptr(state.tree), C.byref(s_out), C.byref(w_out), _ptr(out.tree),
                                     _ptr(com[0]), _ptr(com[1]), _ptr(out.win[3]), _ptr(ws), B, W, cap, state.n_models, S, _stream()),
          "ctc_beam_commit")
    head = out.win.cpu()
    out.bound = int(head[2].max())
    n_max = int(head[3].max())
    new = com[:, :, :n_max].cpu() if n_max else None
    fresh, out.committed = [], []
    for b in range(B):
        n = int(head[3, b])
        ids, frames = (tuple(new[0, b, :n].tolist()), tuple(new[1, b, :n].tolist())) if n else ((), ())
        fresh.append((list(ids), list(frames)))
        out.committed.append((tuple(state.committed[b][0]) + ids, tuple(state.committed[b][1]) + frames))
    return fresh, out


def ctc_beam_decode(logp, lens, blank, beam_size, beam_threshold=20.0, beam_beta=0.0):
    """CTC prefix beam search (mi355x_ctc_beam_decode; `ctc_beam_decode_lm` fuses an n-gram model): logp f32 [B,T,C] contiguous, lens
    i64 [B] (None: T for every utterance) -> (tokens i32 [B,W,T]: hypotheses best first, -1 padded; tok_frame i32 [B,W,T]: the frame
    each token was created in; hyp_len i32 [B,W]; score f32 [B,W]: tot + beam_beta * len, -inf for absent hypotheses; n_hyp i32 [B]).
    The node workspace (2 * T * W integers per utterance) is allocated here and dropped."""
    return _ctc_beam_search("ctc_beam_decode", logp, lens, blank, beam_size, beam_threshold, beam_beta, [])


def ctc_beam_decode_lm(logp, lens, blank, beam_size, beam_threshold, beam_beta, lm, alpha):
    """`ctc_beam_decode` with shallow fusion of an n-gram model (the search of mi355x_ctc_beam_decode_lm): the hypotheses are ranked by
    (tot + beam_beta * len) + alpha * lm(prefix), which is also the score returned.  `lm` is an `NGramLM` (modules/ngram_lm.py), not
    loose tensors: only tables its loader built and checked reach the kernel (a BoostingTree's seventh table is not this entry's).
    alpha = 0 gives the bits of `ctc_beam_decode`."""
    what, models = _ctc_beam_checked([(lm, alpha)], False, logp, "")
    return _ctc_beam_search(what, logp, lens, blank, beam_size, beam_threshold, beam_beta, models)


def ctc_beam_decode_stream(logp, lens, blank, beam_size, beam_threshold, beam_beta, state, lm=None, alpha=0.0, emit=True):
    """one chunk of the resumable CTC prefix beam search (mi355x_ctc_beam_decode_stream; with `lm`, an NGramLM, and `alpha` the search
    of mi355x_ctc_beam_decode_lm_stream): logp f32 [B,T,C] contiguous and lens i64 [B] (None: T) of THIS chunk, `state` the
    `modules.CTCBeamStreamState` the previous chunk returned (None: fresh streams) -> ((tokens, tok_frame, hyp_len, score, n_hyp) of
    all frames so far, or None with emit=False; the next state).  tokens / tok_frame are the state's buffers [B, W, capacity]: valid
    up to hyp_len, not padded, rewritten by the next emitting step; tok_frame counts from the stream's first frame.  The input
    state's beams are not written (its tree is appended to, and grown here so that the kernel's capacity clamp never acts).  Any cut
    into chunks gives the bits of `ctc_beam_decode` / `ctc_beam_decode_lm` over the whole sequence."""
    what, models = _ctc_beam_checked([] if lm is None else [(lm, alpha)], False, logp, "_stream")
    if state is not None and (state.B != logp.shape[0] or state.W != int(beam_size) or state.lm != (lm is not None)):
        raise ValueError(f"ctc_beam_decode_stream: the state is of {state.B} streams, {state.W} beams, "
                         f"{'an' if state.lm else 'no'} LM; the call of {logp.shape[0]}, {int(beam_size)}, "
                         f"{'an' if lm is not None else 'no'} LM")
    return _ctc_beam_search_stream(what, logp, lens, blank, beam_size, beam_threshold, beam_beta, state, models, emit)


def ctc_beam_decode_fused(logp, lens, blank, beam_size, beam_threshold, beam_beta, models):
    """`ctc_beam_decode` with one or two fusion models (mi355x_ctc_beam_decode_fused): `models` is a list of (NGramLM | BoostingTree,
    alpha), not loose tensors.  The search ranks by ((tot + beam_beta * len) + alpha1 * m1(prefix)) + alpha2 * m2(prefix); the score
    returned adds each BoostingTree's final term (the boost of a phrase begun and not finished is taken back) and the n-best is
    ordered by it.  Same outputs as `ctc_beam_decode`."""
    what, models = _ctc_beam_checked(models, True, logp, "")
    return _ctc_beam_search(what, logp, lens, blank, beam_size, beam_threshold, beam_beta, models)


def ctc_beam_decode_fused_stream(logp, lens, blank, beam_size, beam_threshold, beam_beta, state, models, emit=True):
    """one chunk of the resumable `ctc_beam_decode_fused` (mi355x_ctc_beam_decode_fused_stream): `ctc_beam_decode_stream`'s
    arguments and results with `models` as in `ctc_beam_decode_fused`.  The state holds the search's order and ranks; the emitted
    n-best carries the final terms.  Any cut into chunks gives the bits of `ctc_beam_decode_fused` over the whole sequence."""
    what, models = _ctc_beam_checked(models, True, logp, "_stream")
    return _ctc_beam_search_stream(what, logp, lens, blank, beam_size, beam_threshold, beam_beta, state, models, emit)


def specaug_rects(u_tw, u_ts, u_fw, u_fs, length, rects, B, nt, nf, F, T, time_width, freq_width):
    """mask rectangles of SpecAugment's vectorised path from its four uniform draws (one launch instead of ~40 tensor ops)"""
    frac = isinstance(time_width, float)
    check(lib.mi355x_specaug_rects(_ptr(u_tw) if nt else 0, _ptr(u_ts) if nt else 0, _ptr(u_fw) if nf else 0, _ptr(u_fs) if nf else 0,
                                   _ptr(length), _ptr(rects), B, nt, nf, F, T, float(time_width), int(frac), int(freq_width),
                                   _stream()), "specaug_rects")
    return rects


def fill_rects(x, rects, value=0.0):
    """x[b, f0:f1, t0:t1] = value for rects [n,5] int32 = (b, f0, f1, t0, t1); x f32 [B,F,T], in place"""
    B, F, T = x.shape
    n = int(rects.shape[0])
    if n:
        check(lib.mi355x_fill_rects(_ptr(x), _ptr(rects), n, B, F, T, float(value), _stream()), "fill_rects")
    return x


def add2_colsum(a, b, out, ldo, M, d, sum_ab):
    """out[:, :d] = a + b; sum_ab[0:d] += colsum(a), sum_ab[d:2d] += colsum(b)   (bf16 in/out, f32 sums)"""
    n = ((M + 31) // 32) * 2 * d
    sc = _scratch("add2_colsum", n, a.device)
    check(lib.mi355x_add2_colsum(_ptr(a), _ptr(b), _ptr(out), ldo, M, d, _ptr(sum_ab), _ptr(sc), n, _stream()), "add2_colsum")


def add2(a, b, out, ldo, M, d, out_off=0):
    check(lib.mi355x_add2(_ptr(a), _ptr(b), dt(a), _ptr(out) + out_off * out.element_size(), dt(out), ldo, M, d, _stream()),
          "add2")


def relpos_softmax_fwd(ac, bdf, s_out, pd_out, lens, H, B, T, Tp, Pp, scale, drop: Dropout = NO_DROP, ctx=(0, -1, -1)):
    """ctx = (style, left, right): limited attention context, style 0 none / 1 'regular' / 2 'chunked_limited'"""
    check(lib.mi355x_relpos_softmax_fwd_ctx(_ptr(ac), _ptr(bdf), _ptr(s_out), _ptr(pd_out), dt(s_out), _ptr(lens), H, B, T, Tp, Pp,
                                            scale, drop.key, drop.threshold, drop.scale, int(ctx[0]), int(ctx[1]), int(ctx[2]),
                                            _stream()), "relpos_softmax_fwd")


def relpos_softmax_bwd(dpd, s_in, dscore, dbdf, H, B, T, Tp, Pp, scale, drop: Dropout = NO_DROP):
    check(lib.mi355x_relpos_softmax_bwd(_ptr(dpd), dt(dpd), _ptr(s_in), _ptr(dscore), _ptr(dbdf), dt(s_in), H, B, T, Tp, Pp,
                                        scale, drop.key, drop.threshold, drop.scale, _stream()), "relpos_softmax_bwd")


def relpos_flash_fwd(qkv, ldq, pos, ldp, bias_u, bias_v, lens, ctx, ldo, lse, B, H, T, dk, Tp, scale, drop: Dropout = NO_DROP,
                     ctx_lo=None, cu=None):
    """cu (i64 [B+1]): "packed rows" -- the activation matrices hold the valid frames only (include/mi355x_asr.h); the same
    argument on every fused attention call below"""
    check(lib.mi355x_relpos_flash_fwd(_ptr(qkv), ldq, _ptr(pos), ldp, _ptr(bias_u), _ptr(bias_v), _ptr(lens), _ptr(ctx),
                                      _ptr(ctx_lo), ldo, _ptr(lse), B, H, T, dk, Tp, scale, drop.key, drop.threshold, drop.scale,
                                      _ptr(cu), _stream()), "relpos_flash_fwd")


def attn_delta(dO, O, delta, B, H, T, d, O_lo=None, lens=None, cu=None):
    check(lib.mi355x_attn_delta(_ptr(dO), _ptr(O), _ptr(O_lo), _ptr(delta), B, H, T, d, _ptr(lens), _ptr(cu), _stream()), "attn_delta")


def attn_bwd_prep(dO, O, delta, qkv, ldq, bias_u, bias_v, qu, qv, B, H, T, d, O_lo=None, lens=None, cu=None):
    """attn_delta + qbias in one launch (the prologue of the fused attention backward)"""
    check(lib.mi355x_attn_bwd_prep(_ptr(dO), _ptr(O), _ptr(O_lo), _ptr(delta), _ptr(qkv), ldq, _ptr(bias_u), _ptr(bias_v), _ptr(qu),
                                   _ptr(qv), B, H, T, d, _ptr(lens), _ptr(cu), _stream()), "attn_bwd_prep")


def relpos_ds_buffer(B, H, T, device, fill=None):
    """bf16 buffer for the dQ kernel's score-gradient blocks (un-shifted matrix_bd layout, see include/mi355x_asr.h)"""
    n = lib.mi355x_relpos_ds_elems(B, H, T)
    buf = torch.empty(n, dtype=torch.bfloat16, device=device)
    if fill is not None:
        buf.fill_(fill)
    return buf


def relpos_flash_bwd_dq(qu, qv, qkv, ldq, pos, ldp, lens, dO, lse, delta, dqu, dqv, B, H, T, dk, scale,
                        drop: Dropout = NO_DROP, ds_out=None, dq_out=None, ld_dq=0, bias_grads=None, cu=None):
    """dqu / dqv: the two gradients separately (may both be None when `dq_out` is given); dq_out: their sum as rows of pitch
    ld_dq; bias_grads f32 [2 * H * dk] += column sums of dQu | dQv (pos_bias_u | pos_bias_v gradients)"""
    sc, n = None, 0
    if bias_grads is not None:
        n = B * ((T + 127) // 128) * 2 * H * dk
        sc = _scratch("relpos_flash_bwd_dq", n, qu.device)
    check(lib.mi355x_relpos_flash_bwd_dq(_ptr(qu), _ptr(qv), _ptr(qkv), ldq, _ptr(pos), ldp, _ptr(lens), _ptr(dO), _ptr(lse),
                                         _ptr(delta), _ptr(dqu), _ptr(dqv), _ptr(ds_out), _ptr(dq_out), ld_dq, _ptr(bias_grads),
                                         _ptr(sc), n, B, H, T, dk, 0 if ds_out is None else ds_out.numel(), scale, drop.key,
                                         drop.threshold, drop.scale, _ptr(cu), _stream()), "relpos_flash_bwd_dq")


def relpos_flash_bwd_dkv(qu, qv, qkv, ldq, pos, ldp, lens, dO, lse, delta, dqkv, ldd, B, H, T, dk, Tp, scale,
                         drop: Dropout = NO_DROP, cu=None):
    check(lib.mi355x_relpos_flash_bwd_dkv(_ptr(qu), _ptr(qv), _ptr(qkv), ldq, _ptr(pos), ldp, _ptr(lens), _ptr(dO), _ptr(lse),
                                          _ptr(delta), _ptr(dqkv), ldd, B, H, T, dk, Tp, scale, drop.key, drop.threshold,
                                          drop.scale, _ptr(cu), _stream()), "relpos_flash_bwd_dkv")


def relpos_flash_fwd_p(qkv, ldq, pos, ldp, bias_u, bias_v, lens, ctx, ldo, lse, probs, mref, B, H, T, dk, Tp, scale,
                       drop: Dropout = NO_DROP, ctx_lo=None):
    """relpos_flash_fwd that also exports its un-normalised probabilities (`probs`: bf16, >= mi355x_relpos_probs_elems) and
    their per-step reference points (`mref`: f32, >= mi355x_relpos_mref_elems) for the *_p backward kernels; d_k = 64, padded rows"""
    check(lib.mi355x_relpos_flash_fwd_p(_ptr(qkv), ldq, _ptr(pos), ldp, _ptr(bias_u), _ptr(bias_v), _ptr(lens), _ptr(ctx),
                                        _ptr(ctx_lo), ldo, _ptr(lse), _ptr(probs), probs.numel(), _ptr(mref), mref.numel(), B, H, T,
                                        dk, Tp, scale, drop.key, drop.threshold, drop.scale, None, _stream()), "relpos_flash_fwd_p")


def relpos_flash_bwd_dq_p(probs, mref, qkv, ldq, pos, ldp, lens, dO, lse, delta, dqu, dqv, B, H, T, dk, scale,
                          drop: Dropout = NO_DROP, ds_out=None, dq_out=None, ld_dq=0, bias_grads=None):
    """relpos_flash_bwd_dq on the probabilities relpos_flash_fwd_p exported (same outputs; needs neither qu nor qv)"""
    sc, n = None, 0
    if bias_grads is not None:
        n = B * ((T + 127) // 128) * 2 * H * dk
        sc = _scratch("relpos_flash_bwd_dq", n, qkv.device)
    check(lib.mi355x_relpos_flash_bwd_dq_p(_ptr(probs), probs.numel(), _ptr(mref), mref.numel(), _ptr(qkv), ldq, _ptr(pos), ldp,
                                           _ptr(lens), _ptr(dO), _ptr(lse), _ptr(delta), _ptr(dqu), _ptr(dqv), _ptr(ds_out),
                                           _ptr(dq_out), ld_dq, _ptr(bias_grads), _ptr(sc), n, B, H, T, dk,
                                           0 if ds_out is None else ds_out.numel(), scale, drop.key, drop.threshold, drop.scale,
                                           None, _stream()), "relpos_flash_bwd_dq_p")


def relpos_flash_bwd_dkv_p(probs, mref, qu, qkv, ldq, lens, dO, lse, delta, dqkv, ldd, B, H, T, dk, scale, drop: Dropout = NO_DROP):
    """relpos_flash_bwd_dkv on the probabilities relpos_flash_fwd_p exported"""
    check(lib.mi355x_relpos_flash_bwd_dkv_p(_ptr(probs), probs.numel(), _ptr(mref), mref.numel(), _ptr(qu), _ptr(qkv), ldq,
                                            _ptr(lens), _ptr(dO), _ptr(lse), _ptr(delta), _ptr(dqkv), ldd, B, H, T, dk, scale,
                                            drop.key, drop.threshold, drop.scale, None, _stream()), "relpos_flash_bwd_dkv_p")


def relpos_flash_bwd_dpos(qv, ds, lens, dpos, B, H, T, dk, dpos_cast=None, cu=None):
    """`dpos_cast` (bf16, shape of dpos): the GEMM-operand copy of the updated gradient, written by the reduction stage"""
    n = lib.mi355x_relpos_dpos_partial_elems(B, H, T)
    scratch = _scratch("relpos_flash_bwd_dpos", n, dpos.device)
    check(lib.mi355x_relpos_flash_bwd_dpos(_ptr(qv), _ptr(ds), _ptr(lens), _ptr(dpos), dpos.shape[-1], _ptr(dpos_cast),
                                           _ptr(scratch), n, B, H, T, dk, ds.numel(), _ptr(cu), _stream()), "relpos_flash_bwd_dpos")


# ------------------------------------------------------------------------------------------------ conv module
def dwconv_fwd(x, w, bias, y, stats, B, T, d, k, pad_left=-1):
    """pad_left: zero frames in front of the sequence (conv_context_size[0]; k - 1 = causal), -1 = symmetric"""
    check(lib.mi355x_dwconv_fwd_ctx(_ptr(x), _ptr(w), _ptr(bias), _ptr(y), dt(x), _ptr(stats), B, T, d, k, pad_left, _stream()),
          "dwconv_fwd")


_SCRATCH = {}
_SCRATCH_RETIRED = []   # outgrown buffers are KEPT: a recorded launch sequence (hipGraph) may still hold their address


def _scratch(name, n, device):
    """work space of a kernel's two-stage reductions: one buffer per (kernel, device, STREAM) -- launches of the same kernel on
    two streams may overlap -- that grows geometrically and is never freed (a hipGraph recorded at a smaller shape replays with
    the address it captured; freeing the old buffer would let that replay scribble over whatever the allocator put there next:
    round-3 advisor finding; `ConformerEncoder._buf` and `Arena` retire for the same reason)"""
    key = (name, str(device), torch.cuda.current_stream(device).cuda_stream if torch.cuda.is_available() else 0)
    t = _SCRATCH.get(key)
    if t is None or t.numel() < n:
        if t is not None:
            _SCRATCH_RETIRED.append(t)
        t = _SCRATCH[key] = torch.empty(max(n, int(t.numel() * 1.5) if t is not None else n), dtype=torch.float32, device=device)
    return t


def dwconv_fwd_glu(glu_in, lens, cu, glu_out, w, bias, y, stats, B, T, d, k, act=0):
    """glu_fwd (act=0) / swish_mask_fwd (act=1) + dwconv_fwd in one launch: the activation's output is written (backward needs it)
    but never read back"""
    check(lib.mi355x_dwconv_fwd_glu(_ptr(glu_in), _ptr(lens), _ptr(cu), _ptr(glu_out), _ptr(w), _ptr(bias), _ptr(y), dt(glu_in),
                                    _ptr(stats), B, T, d, k, act, _stream()), "dwconv_fwd_glu")


def dwconv_bwd(dy, x, w, dx, dw, dbias, B, T, d, k, pad_left=-1):
    n = 4 * B * (k + 1) * d
    sc = _scratch("dwconv_bwd", n, dy.device)
    check(lib.mi355x_dwconv_bwd_ctx(_ptr(dy), _ptr(x), _ptr(w), _ptr(dx), _ptr(dw), _ptr(dbias), dt(x), B, T, d, k, pad_left, _ptr(sc),
                                    n, _stream()), "dwconv_bwd")


def bn_finalize(stats, count, mean, rstd, running_mean, running_var, momentum, eps, d):
    """`count`: python number, or a device f64 scalar tensor (SyncBatchNorm: all-reduced with the sums)"""
    if isinstance(count, torch.Tensor):
        check(lib.mi355x_bn_finalize_dev_count(_ptr(stats), _ptr(count), _ptr(mean), _ptr(rstd), _ptr(running_mean),
                                               _ptr(running_var), momentum, eps, d, _stream()), "bn_finalize_dev_count")
        return
    check(lib.mi355x_bn_finalize(_ptr(stats), float(count), _ptr(mean), _ptr(rstd), _ptr(running_mean), _ptr(running_var),
                                 momentum, eps, d, _stream()), "bn_finalize")


def bn_eval_stats(running_mean, running_var, mean, rstd, eps, d):
    check(lib.mi355x_bn_eval_stats(_ptr(running_mean), _ptr(running_var), _ptr(mean), _ptr(rstd), eps, d, _stream()),
          "bn_eval_stats")


def bn_swish_fwd(x, mean, rstd, gamma, beta, y, M, d):
    check(lib.mi355x_bn_swish_fwd(_ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(y), dt(x), M, d, _stream()),
          "bn_swish_fwd")


def bn_swish_bwd_reduce(dy, x, mean, rstd, gamma, beta, sums, M, d, dgamma=None, dbeta=None):
    """sums f64 [2, d] += (sum dz, sum dz * xhat); dgamma / dbeta (optional): the parameter gradients in the same launches"""
    n = ((M + 15) // 16) * 2 * d  # (room for 16-row workgroups: MI355X_BNR_ROWS; the kernel's default needs ceil(M/32)*2*d)
    sc = _scratch("bn_swish_bwd_reduce", n, dy.device)
    check(lib.mi355x_bn_swish_bwd_reduce(_ptr(dy), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(sums),
                                         _ptr(dgamma), _ptr(dbeta), dt(x), M, d, _ptr(sc), n, _stream()), "bn_swish_bwd_reduce")


def bn_stats_swish_fwd(x, stats, count, gamma, beta, y, mean, rstd, running_mean, running_var, momentum, eps, M, d):
    """training forward: bn_finalize + bn_swish_fwd in one launch; `count`: python number or device f64 scalar tensor"""
    dev_count = count if isinstance(count, torch.Tensor) else None
    check(lib.mi355x_bn_stats_swish_fwd(_ptr(x), _ptr(stats), 0.0 if dev_count is not None else float(count), _ptr(dev_count),
                                        _ptr(gamma), _ptr(beta), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(running_mean),
                                        _ptr(running_var), momentum, eps, dt(x), M, d, _stream()), "bn_stats_swish_fwd")


def dwconv_tap_scratch(tag, B, d, k, device):
    """a per-caller (per-layer) slab buffer for dwconv_bwd_bnswish(..., scratch=, defer_reduce=True) + dwconv_tap_reduce"""
    return _scratch(f"dwconv_bwd_tap:{tag}", 4 * B * (k + 1) * d, device)


def dwconv_tap_reduce(scratch, B, d, k, dw, dbias):
    check(lib.mi355x_dwconv_tap_reduce(_ptr(scratch), scratch.numel(), B, d, k, _ptr(dw), _ptr(dbias), _stream()), "dwconv_tap_reduce")


def dwconv_bwd_bnswish(dy, cc, mean, rstd, gamma, beta, sums, count, training, x, w, dx, dw, dbias, B, T, d, k, glu_in=None,
                       glu_din=None, glu_len=None, glu_cu=None, scratch=None, defer_reduce=False, glu_act=0):
    """bn_swish_bwd_apply + dwconv_bwd in one launch (the gradient w.r.t. the BatchNorm input stays in the kernel's LDS tile);
    `count`: python number or device f64 scalar tensor.  glu_in / glu_din: the GLU backward as well -- the kernel writes the gradient
    of the GLU's [rows, 2d] input instead of dx (glu_bwd's semantics: zeros beyond glu_len, packed rows with glu_cu)"""
    n = 4 * B * (k + 1) * d
    sc = scratch if scratch is not None else _scratch("dwconv_bwd", n, dy.device)
    dev_count = count if isinstance(count, torch.Tensor) else None
    check(lib.mi355x_dwconv_bwd_bnswish(_ptr(dy), _ptr(cc), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(sums),
                                        0.0 if dev_count is not None else float(count), _ptr(dev_count), int(training), _ptr(x),
                                        _ptr(w), _ptr(dx), _ptr(dw), _ptr(dbias), _ptr(glu_in), _ptr(glu_din), _ptr(glu_len),
                                        _ptr(glu_cu), glu_act, dt(x), B, T, d, k, _ptr(sc), n, int(bool(defer_reduce)), _stream()),
          "dwconv_bwd_bnswish")


def bn_swish_bwd_apply(dy, x, mean, rstd, gamma, beta, sums, count, training, dx, M, d):
    if isinstance(count, torch.Tensor):
        check(lib.mi355x_bn_swish_bwd_apply_dev_count(_ptr(dy), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta),
                                                      _ptr(sums), _ptr(count), int(training), _ptr(dx), dt(x), M, d, _stream()),
              "bn_swish_bwd_apply_dev_count")
        return
    check(lib.mi355x_bn_swish_bwd_apply(_ptr(dy), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(sums),
                                        float(count), int(training), _ptr(dx), dt(x), M, d, _stream()), "bn_swish_bwd_apply")


def bn_param_grad(sums, dgamma, dbeta, d):
    check(lib.mi355x_bn_param_grad(_ptr(sums), _ptr(dgamma), _ptr(dbeta), d, _stream()), "bn_param_grad")


# ------------------------------------------------------------------------------------------------ loss / optimizer
def ctc_loss(logp, targets, in_len, tgt_len, blank, grad=None, grad_scale=1.0, zero_infinity=True):
    """logp f32 [B,T,C] contiguous; returns per-utterance nll [B]; fills `grad` (same shape as logp) if given."""
    B, T, C_ = logp.shape
    U = targets.shape[1]
    S = 2 * U + 1
    alpha = torch.empty(B, T, S, device=logp.device, dtype=torch.float32)
    beta = torch.empty(B, T, S, device=logp.device, dtype=torch.float32)
    nll = torch.empty(B, device=logp.device, dtype=torch.float32)
    check(lib.mi355x_ctc_loss(_ptr(logp), _ptr(targets), _ptr(in_len), _ptr(tgt_len), _ptr(alpha), _ptr(beta), _ptr(nll),
                              _ptr(grad), B, T, C_, U, blank, grad_scale, int(zero_infinity), _stream()), "ctc_loss")
    return nll


def _transducer_loss(name, acts, ld_acts, labels, act_lens, label_lens, B, T, U1, V1, params, ws_per_row, grads, ld_grads):
    """one call of a transducer loss entry (`params`: what the entry takes between V1 and costs): allocates the costs and the
    workspace of `ws_per_row` floats per lattice cell + 2 per utterance, resolves the gradient's dtype and pitch -> costs f32 [B]"""
    n = ws_per_row * B * T * U1 + 2 * B
    ws = torch.empty(n, device=acts.device, dtype=torch.float32)
    costs = torch.empty(B, device=acts.device, dtype=torch.float32)
    gdt, ldg = (dt(grads), ld_grads) if grads is not None else (F32, 0)
    check(getattr(lib, "mi355x_" + name)(_ptr(acts), ld_acts, _ptr(labels), _ptr(act_lens), _ptr(label_lens), B, T, U1, V1, *params,
                                         _ptr(costs), _ptr(grads), gdt, ldg, _ptr(ws), n, _stream()), name)
    return costs


def rnnt_loss_pitched(acts, ld_acts, B, T, U1, V1, labels, act_lens, label_lens, blank, grads, ld_grads, fastemit_lambda=0.0,
                      clamp=0.0, grad_scale=1.0):
    """acts f32, rows of pitch ld_acts; grads (f32 or bf16, or None: loss only) rows of pitch ld_grads, pad columns zero-filled
    -> costs f32 [B]"""
    return _transducer_loss("rnnt_loss_ex", acts, ld_acts, labels, act_lens, label_lens, B, T, U1, V1,
                            (blank, fastemit_lambda, clamp, grad_scale), 5, grads, ld_grads)


def rnnt_loss(acts, labels, act_lens, label_lens, blank, grads=None, fastemit_lambda=0.0, clamp=0.0, grad_scale=1.0):
    """acts f32 [B,T,U1,V1] logits (contiguous); labels i64 [B,U1-1]; returns costs f32 [B]; fills `grads` (f32, same shape)"""
    B, T, U1, V1 = acts.shape
    return rnnt_loss_pitched(acts, V1, B, T, U1, V1, labels, act_lens, label_lens, blank, grads, V1, fastemit_lambda=fastemit_lambda,
                             clamp=clamp, grad_scale=grad_scale)


def _greedy_search(what, enc_proj, enc_len, emb, w_ih, ld_ih, w_hh, ld_hh, b_ih, b_hh, w_pred, ld_pred, b_pred, w_out, ld_out, b_out,
                   blank, durations, max_symbols, max_out, *, with_state=False, stream=None, state=None, method=None, models=None,
                   upper_layers=None):
    """every greedy transducer search: the outputs, the descriptor and the one entry (mi355x_transducer_greedy_decode).  `durations`
    given: TDT.  `stream` = the state class of the resumable search (None: one-shot), `state` = the state to start from (None: fresh
    streams).  `method` = the confidence measure, `models` = the checked fusion models.  -> (tokens, times, out_len), then whatever
    was asked for, in this order: score (every search but the resumable one without models), (h, c) (`with_state`), the next state
    (`stream`), tok_conf (`method`).  `upper_layers` = [(w_ih, ld_ih, w_hh, ld_hh, b_ih, b_hh), ...] for layers 1 .. L-1 of the
    prediction network (mi355x_transducer_greedy_decode_layers; weights in w_ih's dtype, biases fp32): every LSTM state is then
    [L, B, H].  None or empty: the one-layer search, as ever."""
    upper_layers = list(upper_layers) if upper_layers else []
    L = 1 + len(upper_layers)
    if L > 4:
        raise ValueError(f"{what}: at most 4 LSTM layers in the prediction network (3 `upper_layers`), got {L}")
    if state is not None and not isinstance(state, stream):
        raise TypeError(f"{what}: `state` must be an {stream.__name__}, got {type(state).__name__}")
    B, T, J = enc_proj.shape
    V1, H = emb.shape
    if max_out is None:
        max_out = T * max_symbols if max_symbols > 0 else 4 * T
    dev = enc_proj.device
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    tokens = torch.empty(B, max_out, dtype=torch.int32, device=dev)
    times = torch.empty(B, max_out, dtype=torch.int32, device=dev)
    out_len = torch.empty(B, dtype=torch.int32, device=dev)
    d = TransducerGreedyDesc(
        enc_proj=_ptr(enc_proj), f_dtype=dt(enc_proj), ldf=enc_proj.stride(1), enc_len=_ptr(enc_len), emb=_ptr(emb),
        w_ih=_ptr(w_ih), ld_ih=ld_ih, w_hh=_ptr(w_hh), ld_hh=ld_hh, w_pred=_ptr(w_pred), ld_pred=ld_pred, w_out=_ptr(w_out),
        ld_out=ld_out, w_dtype=dt(w_ih), b_ih=_ptr(b_ih), b_hh=_ptr(b_hh), b_pred=_ptr(b_pred), b_out=_ptr(b_out),
        B=B, T=T, J=J, H=H, V1=V1, blank=blank, max_symbols=max_symbols, max_out=max_out,
        tokens=_ptr(tokens), times=_ptr(times), out_len=_ptr(out_len))
    out = (tokens, times, out_len)
    keep = []   # what the descriptor points to on the host, alive until the call returns
    if durations is not None:
        d.D, dur = _tdt_durations(durations)
        d.durations = C.addressof(dur)
        keep.append(dur)
    if stream is None or models is not None:
        score = f32(B)
        d.score = _ptr(score)
        out += (score,)
    if with_state:
        h, c = (f32(B, H), f32(B, H)) if L == 1 else (f32(L, B, H), f32(L, B, H))
        d.h_out, d.c_out = _ptr(h), _ptr(c)
        out += ((h, c),)
    if stream is not None:
        nxt = stream.empty(B, H, dev, layers=L)
        if durations is None:   # (not written by the RNN-T search)
            nxt.skip.zero_(); nxt.zero_run.zero_()
        for field, st in (("state_in", state), ("state_out", nxt)):
            if st is not None:
                keep.append(st._c(B, H, layers=L))
                setattr(d, field, C.addressof(keep[-1]))
                if models is not None:
                    setattr(d, "m_" + field, _ptr(st.m_state))
        out += (nxt,)
    if method is not None:   # the confidence of every emitted label
        tok_conf = f32(B, max_out)
        keep.append(TransducerConf(*method))
        d.conf, d.tok_conf = C.addressof(keep[-1]), _ptr(tok_conf)
        out += (tok_conf,)
    if models is not None:
        arr, tables = _ctc_beam_fusion_array(models, enc_proj)
        keep += [arr, tables]
        d.models, d.n_models = C.addressof(arr), len(arr)
    if L == 1:
        check(lib.mi355x_transducer_greedy_decode(C.byref(d), _stream()), what)
        return out
    up = TransducerLstmLayers(n_upper=L - 1)
    for l, (u_ih, uld_ih, u_hh, uld_hh, ub_ih, ub_hh) in enumerate(upper_layers):
        if dt(u_ih) != d.w_dtype or dt(u_hh) != d.w_dtype or ub_ih.dtype != torch.float32 or ub_hh.dtype != torch.float32:
            raise ValueError(f"{what}: layer {l + 1} of the prediction network: weights in the dtype of layer 0, biases fp32")
        if (min(uld_ih, uld_hh) < H or u_ih.numel() < (4 * H - 1) * uld_ih + H or u_hh.numel() < (4 * H - 1) * uld_hh + H
                or min(ub_ih.numel(), ub_hh.numel()) < 4 * H):
            raise ValueError(f"{what}: layer {l + 1} of the prediction network: weights [4H, H], biases [4H] for H = {H}")
        up.w_ih[l], up.w_hh[l], up.b_ih[l], up.b_hh[l] = _ptr(u_ih), _ptr(u_hh), _ptr(ub_ih), _ptr(ub_hh)
        up.ld_ih[l], up.ld_hh[l] = uld_ih, uld_hh
    check(lib.mi355x_transducer_greedy_decode_layers(C.byref(d), C.byref(up), _stream()), what)
    return out


def rnnt_greedy_decode(enc_proj, enc_len, emb, w_ih, ld_ih, w_hh, ld_hh, b_ih, b_hh, w_pred, ld_pred, b_pred, w_out, ld_out, b_out,
                       blank, max_symbols, max_out=None, with_state=False, *, upper_layers=None):
    """greedy transducer search of a whole batch in one launch (mi355x_transducer_greedy_decode).  enc_proj [B, T, J] = joint.enc(
    encoder output); weights fp32 or bf16 (all four the same dtype).  -> (tokens i32 [B, max_out] -1 padded, frame indices likewise,
    lengths i32 [B], score f32 [B][, (h, c) f32 [B, H]])"""
    return _greedy_search("rnnt_greedy_decode", enc_proj, enc_len, emb, w_ih, ld_ih, w_hh, ld_hh, b_ih, b_hh, w_pred, ld_pred, b_pred,
                          w_out, ld_out, b_out, blank, None, max_symbols, max_out, with_state=with_state, upper_layers=upper_layers)


def rnnt_greedy_decode_conf(enc_proj, enc_len, emb, w_ih, ld_ih, w_hh, ld_hh, b_ih, b_hh, w_pred, ld_pred, b_pred, w_out, ld_out,
                            b_out, blank, max_symbols, method, max_out=None, with_state=False, *, upper_layers=None):
    """rnnt_greedy_decode plus the confidence of every emitted label (mi355x_transducer_greedy_decode with a measure): `method` =
    (method, norm, alpha, k0, k1, k2) for V = V1 (modules.confidence.ConfidenceMethodConfig.kernel_args) -> rnnt_greedy_decode's
    tuple with tok_conf f32 [B, max_out] (0.0 padded) appended"""
    return _greedy_search("rnnt_greedy_decode_conf", enc_proj, enc_len, emb, w_ih, ld_ih, w_hh, ld_hh, b_ih, b_hh, w_pred, ld_pred,
                          b_pred, w_out, ld_out, b_out, blank, None, max_symbols, max_out, with_state=with_state, method=method,
                          upper_layers=upper_layers)


def _tdt_durations(durations):
    d = [int(x) for x in durations]
    return len(d), (C.c_int * len(d))(*d)


def tdt_loss_pitched(acts, ld_acts, B, T, U1, V1, durations, labels, act_lens, label_lens, blank, grads=None, ld_grads=0,
                     sigma=0.0, grad_scale=1.0):
    """Token-and-Duration Transducer loss (mi355x_tdt_loss_ex): acts f32 logits [.., V1 + D] in rows of pitch ld_acts (V1 label
    logits, then one per duration); grads (f32 or bf16, optional) rows of pitch ld_grads, pad columns zero-filled -> costs f32 [B]"""
    D, dur = _tdt_durations(durations)
    return _transducer_loss("tdt_loss_ex", acts, ld_acts, labels, act_lens, label_lens, B, T, U1, V1,
                            (D, dur, blank, sigma, grad_scale), 4 + 2 * D, grads, ld_grads)


def tdt_loss(acts, labels, act_lens, label_lens, blank, durations, grads=None, sigma=0.0, grad_scale=1.0):
    """acts f32 [B,T,U1,V1+D] logits (contiguous); labels i64 [B,U1-1]; returns costs f32 [B]; fills `grads` (f32, same shape)"""
    B, T, U1, W = acts.shape
    V1 = W - len(durations)
    return tdt_loss_pitched(acts, W, B, T, U1, V1, durations, labels, act_lens, label_lens, blank, grads=grads, ld_grads=W,
                            sigma=sigma, grad_scale=grad_scale)


def tdt_greedy_decode(enc_proj, enc_len, emb, w_ih, ld_ih, w_hh, ld_hh, b_ih, b_hh, w_pred, ld_pred, b_pred, w_out, ld_out, b_out,
                      blank, durations, max_symbols, max_out=None, with_state=False, *, upper_layers=None):
    """greedy TDT search of a whole batch in one launch (mi355x_transducer_greedy_decode with a duration set): as rnnt_greedy_decode,
    with w_out / b_out holding V1 + len(durations) rows (label logits, then duration logits); frames advance by the predicted duration"""
    return _greedy_search("tdt_greedy_decode", enc_proj, enc_len, emb, w_ih, ld_ih, w_hh, ld_hh, b_ih, b_hh, w_pred, ld_pred, b_pred,
                          w_out, ld_out, b_out, blank, durations, max_symbols, max_out, with_state=with_state,
                          upper_layers=upper_layers)


def tdt_greedy_decode_conf(enc_proj, enc_len, emb, w_ih, ld_ih, w_hh, ld_hh, b_ih, b_hh, w_pred, ld_pred, b_pred, w_out, ld_out,
                           b_out, blank, durations, max_symbols, method, max_out=None, with_state=False, *, upper_layers=None):
    """tdt_greedy_decode plus the confidence of every emitted label over the V1 label logits (mi355x_transducer_greedy_decode with
    a duration set and a measure)"""
    return _greedy_search("tdt_greedy_decode_conf", enc_proj, enc_len, emb, w_ih, ld_ih, w_hh, ld_hh, b_ih, b_hh, w_pred, ld_pred,
                          b_pred, w_out, ld_out, b_out, blank, durations, max_symbols, max_out, with_state=with_state, method=method,
                          upper_layers=upper_layers)


class _StreamStateC(C.Structure):   # mi355x_rnnt_stream_state
    _fields_ = [(n, C.c_void_p) for n in ("h", "c", "last", "score", "frames_done", "skip", "zero_run")]


class RNNTStreamState:
    """decoder state of a batch of streams between two chunks of the resumable greedy search (mi355x_rnnt_stream_state): h, c f32
    [B, H] (committed LSTM state), last i32 [B] (last emitted label), score f32 [B] (running log-probability), frames_done i32 [B],
    skip / zero_run i32 [B] (TDT; zeros and unused for RNN-T).  All on the device; every step returns a new object.  A prediction
    network of `layers` = L > 1 LSTM layers: h, c are [L, B, H] (torch's LSTM state layout, the batch on dimension 1)."""
    __slots__ = ("h", "c", "last", "score", "frames_done", "skip", "zero_run")

    def __init__(self, h, c, last, score, frames_done, skip, zero_run):
        self.h, self.c, self.last, self.score, self.frames_done, self.skip, self.zero_run = h, c, last, score, frames_done, skip, zero_run

    @staticmethod
    def _hc_shape(B, H, layers):
        return (B, H) if layers == 1 else (layers, B, H)

    @classmethod
    def empty(cls, B, H, device, layers=1):
        i32 = lambda: torch.empty(B, dtype=torch.int32, device=device)
        hc = lambda: torch.empty(cls._hc_shape(B, H, layers), dtype=torch.float32, device=device)
        return cls(hc(), hc(), i32(), torch.empty(B, dtype=torch.float32, device=device), i32(), i32(), i32())

    @classmethod
    def fresh(cls, B, H, blank, device, layers=1):
        """the state of B streams that have seen nothing (what a null state_in means to the kernel)"""
        z = lambda: torch.zeros(B, dtype=torch.int32, device=device)
        hc = lambda: torch.zeros(cls._hc_shape(B, H, layers), dtype=torch.float32, device=device)
        return cls(hc(), hc(), torch.full((B,), int(blank), dtype=torch.int32, device=device),
                   torch.zeros(B, dtype=torch.float32, device=device), z(), z(), z())

    def tensors(self):
        return tuple(getattr(self, n) for n in self.__slots__)

    @staticmethod
    def _pick(t, b):
        """stream b of a state tensor as a batch of one: the batch is dimension 1 of a layered h / c, dimension 0 of the others"""
        return t[:, b:b + 1].contiguous() if t.dim() == 3 else t[b:b + 1]

    def select(self, b):
        """the state of stream b as a batch of one (views; a layered h / c: a copy, so that it stays contiguous)"""
        return RNNTStreamState(*(self._pick(t, b) for t in self.tensors()))

    @classmethod
    def stack(cls, states):
        return cls(*(torch.cat(ts, dim=1 if ts[0].dim() == 3 else 0).contiguous() for ts in zip(*(s.tensors() for s in states))))

    def _c(self, B, H, layers=1):
        hc = self._hc_shape(B, H, layers)
        want = (hc, hc, (B,), (B,), (B,), (B,), (B,))
        dts = (torch.float32, torch.float32, torch.int32, torch.float32, torch.int32, torch.int32, torch.int32)
        for n, t, shp, d in zip(self.__slots__, self.tensors(), want, dts):
            if tuple(t.shape) != shp or t.dtype != d or not t.is_contiguous():
                raise ValueError(f"stream state `{n}`: expected contiguous {d} {shp}, got {t.dtype} {tuple(t.shape)}")
        return _StreamStateC(*(_ptr(t) for t in self.tensors()))


def rnnt_greedy_decode_stream(enc_proj, enc_len, emb, w_ih, ld_ih, w_hh, ld_hh, b_ih, b_hh, w_pred, ld_pred, b_pred, w_out, ld_out,
                              b_out, blank, max_symbols, state=None, max_out=None, *, upper_layers=None):
    """one chunk of the resumable greedy transducer search (mi355x_transducer_greedy_decode with a state to write):
    rnnt_greedy_decode's arguments, with enc_len = the frames of this chunk per stream, and `state` = the RNNTStreamState the
    previous chunk returned (None: fresh streams).  -> (tokens, global frame indices, lengths of THIS chunk's labels, the next RNNTStreamState; its `score` is the
    stream's running score).  Any cut of a stream into chunks gives bit-identical results to one launch over all of it."""
    return _greedy_search("rnnt_greedy_decode_stream", enc_proj, enc_len, emb, w_ih, ld_ih, w_hh, ld_hh, b_ih, b_hh, w_pred, ld_pred,
                          b_pred, w_out, ld_out, b_out, blank, None, max_symbols, max_out, stream=RNNTStreamState, state=state,
                          upper_layers=upper_layers)


def tdt_greedy_decode_stream(enc_proj, enc_len, emb, w_ih, ld_ih, w_hh, ld_hh, b_ih, b_hh, w_pred, ld_pred, b_pred, w_out, ld_out,
                             b_out, blank, durations, max_symbols, state=None, max_out=None, *, upper_layers=None):
    """one chunk of the resumable greedy TDT search (mi355x_transducer_greedy_decode with a duration set and a state to write): as
    rnnt_greedy_decode_stream; a duration that jumps past the chunk's end is carried in the state (`skip`) and taken off the next
    chunk(s)"""
    return _greedy_search("tdt_greedy_decode_stream", enc_proj, enc_len, emb, w_ih, ld_ih, w_hh, ld_hh, b_ih, b_hh, w_pred, ld_pred,
                          b_pred, w_out, ld_out, b_out, blank, durations, max_symbols, max_out, stream=RNNTStreamState, state=state,
                          upper_layers=upper_layers)


def rnnt_greedy_decode_stream_conf(enc_proj, enc_len, emb, w_ih, ld_ih, w_hh, ld_hh, b_ih, b_hh, w_pred, ld_pred, b_pred, w_out, ld_out,
                                   b_out, blank, max_symbols, method, state=None, max_out=None, *, upper_layers=None):
    """rnnt_greedy_decode_stream plus the confidence of this chunk's labels (mi355x_transducer_greedy_decode with a state to write
    and a measure) -> (tokens, global frame indices, lengths, next state, tok_conf f32 [B, max_out] 0.0 padded); bit-identical to one launch for any cut"""
    return _greedy_search("rnnt_greedy_decode_stream_conf", enc_proj, enc_len, emb, w_ih, ld_ih, w_hh, ld_hh, b_ih, b_hh, w_pred,
                          ld_pred, b_pred, w_out, ld_out, b_out, blank, None, max_symbols, max_out, stream=RNNTStreamState,
                          state=state, method=method, upper_layers=upper_layers)


def tdt_greedy_decode_stream_conf(enc_proj, enc_len, emb, w_ih, ld_ih, w_hh, ld_hh, b_ih, b_hh, w_pred, ld_pred, b_pred, w_out, ld_out,
                                  b_out, blank, durations, max_symbols, method, state=None, max_out=None, *, upper_layers=None):
    """tdt_greedy_decode_stream plus the confidence of this chunk's labels (mi355x_transducer_greedy_decode with a duration set, a
    state to write and a measure)"""
    return _greedy_search("tdt_greedy_decode_stream_conf", enc_proj, enc_len, emb, w_ih, ld_ih, w_hh, ld_hh, b_ih, b_hh, w_pred,
                          ld_pred, b_pred, w_out, ld_out, b_out, blank, durations, max_symbols, max_out, stream=RNNTStreamState,
                          state=state, method=method, upper_layers=upper_layers)


class RNNTFusedStreamState(RNNTStreamState):
    """the state of the fused greedy search (the descriptor's states and m_state_in / m_state_out): RNNTStreamState and m_state i32
    [B, 2], the automaton state of fusion model m in column m (fresh stream: 1; column 1 stays 1 with one model).  `score` is the
    running score without the models' final terms."""
    __slots__ = ("m_state",)
    _base = RNNTStreamState.__slots__

    def __init__(self, h, c, last, score, frames_done, skip, zero_run, m_state):
        super().__init__(h, c, last, score, frames_done, skip, zero_run)
        self.m_state = m_state

    @classmethod
    def empty(cls, B, H, device, layers=1):
        return cls(*RNNTStreamState.empty(B, H, device, layers).tensors(), torch.ones(B, 2, dtype=torch.int32, device=device))

    @classmethod
    def fresh(cls, B, H, blank, device, layers=1):
        return cls(*RNNTStreamState.fresh(B, H, blank, device, layers).tensors(), torch.ones(B, 2, dtype=torch.int32, device=device))

    def tensors(self):
        return tuple(getattr(self, n) for n in self._base + self.__slots__)

    def select(self, b):
        return RNNTFusedStreamState(*(self._pick(t, b) for t in self.tensors()))

    def _c(self, B, H, layers=1):
        m = self.m_state
        if tuple(m.shape) != (B, 2) or m.dtype != torch.int32 or not m.is_contiguous():
            raise ValueError(f"stream state `m_state`: expected contiguous torch.int32 {(B, 2)}, got {m.dtype} {tuple(m.shape)}")
        return RNNTStreamState(*self.tensors()[:len(self._base)])._c(B, H, layers)   # (m_state travels beside it in the descriptor)


def _transducer_fusion_check(what, models, V1):
    """`models` = [(NGramLM | BoostingTree, alpha), ...], one or two, over the V1 - 1 labels of the joint"""
    from .modules.ngram_lm import NGramLM
    models = list(models) if models is not None else []
    if not 1 <= len(models) <= 2:
        raise ValueError(f"{what}: `models` must hold one or two (model, alpha) pairs, got {len(models)}")
    for i, pair in enumerate(models):
        if not (isinstance(pair, (tuple, list)) and len(pair) == 2 and isinstance(pair[0], NGramLM)):
            got = type(pair[0]).__name__ if isinstance(pair, (tuple, list)) and len(pair) else type(pair).__name__
            raise TypeError(f"{what}: `models` holds (NGramLM | BoostingTree, alpha) pairs, got {got}")
        if pair[0].vocab_size != V1 - 1:
            raise ValueError(f"{what}: model {i} has {pair[0].vocab_size} labels, the joint {V1} classes (labels + the blank)")
    return models


def transducer_greedy_decode_fused(enc_proj, enc_len, emb, w_ih, ld_ih, w_hh, ld_hh, b_ih, b_hh, w_pred, ld_pred, b_pred, w_out, ld_out,
                                   b_out, blank, max_symbols, models, durations=None, state=None, max_out=None, *, upper_layers=None):
    """the greedy transducer search with shallow fusion (mi355x_transducer_greedy_decode with models, which include/mi355x_asr.h states):
    rnnt_greedy_decode's arguments, `models` = a list of one or two (NGramLM | BoostingTree, alpha) as in `ctc_beam_decode_fused`,
    `durations` for the TDT search.  A step whose arg-max is a label emits the label that ranks highest with the models' look-ups
    added; a blank stays a blank.  `state` None: the one-shot search -> (tokens, frame indices, lengths, score, (h, c)).  `state` an
    RNNTFusedStreamState (`fresh` for the first chunk): one chunk of the resumable search, enc_len = this chunk's frames ->
    (tokens, GLOBAL frame indices, lengths of this chunk's labels, score, the next RNNTFusedStreamState).  `score` is the score
    of the stream so far with each BoostingTree's final term (a phrase begun and not finished is not paid for); the state's own
    `score` is the running one.  Any cut into chunks gives the bits of one launch; every alpha = 0 the bits of the searches
    without models."""
    what = "transducer_greedy_decode_fused"
    return _greedy_search(what, enc_proj, enc_len, emb, w_ih, ld_ih, w_hh, ld_hh, b_ih, b_hh, w_pred, ld_pred, b_pred, w_out, ld_out,
                          b_out, blank, durations, max_symbols, max_out, with_state=state is None,
                          stream=None if state is None else RNNTFusedStreamState, state=state,
                          models=_transducer_fusion_check(what, models, emb.shape[0]), upper_layers=upper_layers)


def row_scale(x, vec, rows, cols):
    check(lib.mi355x_row_scale(_ptr(x), _ptr(vec), rows, cols, _stream()), "row_scale")


def adamw_step(params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0,
               clip_coef=None, ema=None, ema_decay=0.0):
    if clip_coef is None and ema is None:
        check(lib.mi355x_adamw_step(_ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq), params.numel(), lr, beta1,
                                    beta2, eps, weight_decay, step, grad_scale, _stream()), "adamw_step")
    else:
        check(lib.mi355x_adamw_step_ex(_ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq), params.numel(), lr, beta1,
                                       beta2, eps, weight_decay, step, grad_scale, _ptr(clip_coef), _ptr(ema), ema_decay,
                                       _stream()), "adamw_step_ex")


def grad_sumsq(grads, out_f64):
    check(lib.mi355x_grad_sumsq(_ptr(grads), grads.numel(), _ptr(out_f64), _stream()), "grad_sumsq")


def clip_coef(sumsq_f64, scale, max_norm, coef):
    check(lib.mi355x_clip_coef(_ptr(sumsq_f64), int(sumsq_f64.numel()), float(scale), float(max_norm), _ptr(coef), _stream()),
          "clip_coef")



def pack_weights(table_dev, n_entries, total_tiles, out_dtype):
    check(lib.mi355x_pack_weights(_ptr(table_dev), n_entries, total_tiles, out_dtype, _stream()), "pack_weights")


def fill_f32(t, value=0.0):
    check(lib.mi355x_fill_f32(_ptr(t), t.numel(), value, _stream()), "fill_f32")


# ------------------------------------------------------------------------------------------------ cache-aware streaming
def stream_cache_assemble(cache, y, kv_in, cache_next, B, C, Tq, d):
    """kv_in [B*(C+Tq), d] = cat(cache [B, C, d] f32, y [B*Tq, d]) along time; cache_next [B, C, d] f32 = its last C rows"""
    check(lib.mi355x_stream_cache_assemble(_ptr(cache) if C else 0, _ptr(y), _ptr(kv_in), _ptr(cache_next) if C else 0, dt(y),
                                           B, C, Tq, d, _stream()), "stream_cache_assemble")


def stream_attn(q, ldq, kv, ldkv, v_off, pos, ldp, bias_u, bias_v, cache_len, chunk_len, ctx, ldo, B, H, Tq, Tk, dk, scale,
                chunk=0, left_chunks=-1):
    """chunk attention of Tq queries against Tk = C + Tq keys (see mi355x_stream_attn); chunk = 0: no chunked_limited rule"""
    check(lib.mi355x_stream_attn(_ptr(q), ldq, _ptr(kv), ldkv, v_off, _ptr(pos), ldp, _ptr(bias_u), _ptr(bias_v), _ptr(cache_len),
                                 _ptr(chunk_len), _ptr(ctx), ldo, dt(q), B, H, Tq, Tk, dk, chunk, left_chunks, scale, _stream()),
          "stream_attn")


def stream_dwconv(x, cache, w, bias, y, cache_next, B, Tq, d, k):
    """causal depthwise conv whose k - 1 left taps come from cache [B, d, k-1] f32; cache_next = last k - 1 frames of cat(cache, x)"""
    check(lib.mi355x_stream_dwconv(_ptr(x), _ptr(cache), _ptr(w), _ptr(bias), _ptr(y), _ptr(cache_next), dt(x), B, Tq, d, k,
                                   _stream()), "stream_dwconv")
