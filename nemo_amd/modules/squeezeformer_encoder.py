"""Drop-in `SqueezeformerEncoder` NeuralModule (BASELINE.json configs[4]) on the MI355X engine.

Replaces `nemo/collections/asr/modules/squeezeformer_encoder.py:40-400` + `parts/submodules/squeezeformer_modules.py:30-203`
behind the same constructor arguments, state-dict keys and (audio_signal, length) -> (encoded [B, D, T'], lengths) contract:

    'dw_striding' sub-sampling -> x*sqrt(d) (+dropout) -> pre_ln -> L x [ MHA -> FFN -> Conv -> FFN ], every sub-block
    x <- LayerNorm(x + dropout(f(x * scale + bias)))   (post-LN, squeezeformer_modules.py:139-181), with the temporal U-Net
    detour: at `time_reduce_idx` a masked depthwise Conv1d(k=5, s=2) + pointwise conv halves the frame rate (own positional
    table), at `time_recovery_idx` the frames are repeated x2, passed through a Linear and added to the cached full-rate
    activations (squeezeformer_encoder.py:340-361).

What is shared with the Conformer engine (conformer_encoder.py): the sub-sampling stack, the MFMA GEMM with fused epilogues,
rel-pos attention (flash kernels at d_k = 64, GEMM + fused softmax otherwise), depthwise k=31 conv / BatchNorm / Swish kernels
(run here on 2*d_model channels: 'swish' point-wise activation keeps both halves, conformer_modules.py:267-275), LayerNorm,
side-stream weight gradients, flat parameters.  What is new: csrc/squeezeformer.hip.

Odd geometries.  Squeezeformer-Medium is d_model = 324 with 4 heads: d_k = 81 and neither is a multiple of 8, while bf16 MFMA
operands need 16-byte aligned rows and heads.  Nothing is special-cased in the kernels; the operands are laid out so that the
arithmetic is unchanged:
  * heads are padded to d_k' = roundup8(d_k) INSIDE THE PACKED WEIGHT IMAGES (q|k|v, linear_pos, linear_out, pos_bias_u/v
    get zero rows / columns for the pad lanes), so q, k, v, p come out of their GEMMs with exact zeros in the pad lanes and
    every score, context vector and gradient is what the 81-wide heads give; softmax scale stays 1/sqrt(81);
  * [M, d] bf16 activations that feed a GEMM have row pitch roundup8(d) with zero pad columns (the kernels of
    squeezeformer.hip take the pitch); weight gradients of the padded heads are produced per head by batched TN GEMMs whose
    batch strides step over the pad lanes;
  * the sub-sampling stack's channel count (= d_model by default) is padded the same way: zero-padded copies of its small
    f32 weights / biases and zero rows / columns in the packed pointwise and output images make the pad channels exact
    zeros through ReLU, depthwise and pointwise stages; weight gradients land in a zeroed scratch of the padded shapes and the
    real part is added into the parameters' gradients (a handful of KB-sized adds per step).
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch
from torch import nn

from .. import ops
from ..packing import _pad8
from .conformer_encoder import (ConformerEncoder, ConvSubsampling, RelPositionalEncoding, _DwGrads, _DwWeights, _FeedForward, _LnSaved,
                                _RelPosMHA, _Step, _SubIO, _record)
from .engine import declare_padded_heads
from ..core import NeuralModule


class ScaleBiasLayer(nn.Module):  # squeezeformer_modules.py:30-57
    def __init__(self, d_model: int, adaptive_scale: bool):
        super().__init__()
        self.adaptive_scale = adaptive_scale
        if adaptive_scale:
            self.scale = nn.Parameter(torch.ones(d_model))
            self.bias = nn.Parameter(torch.zeros(d_model))
        else:
            self.register_buffer("scale", torch.ones(d_model), persistent=True)
            self.register_buffer("bias", torch.zeros(d_model), persistent=True)


class _SwishConvolution(nn.Module):  # conformer_modules.py:236 ConformerConvolution(pointwise_activation='swish')
    def __init__(self, d_model, kernel_size):
        super().__init__()
        c2 = 2 * d_model  # 'swish' is in the activation registry: no GLU halving, the depthwise stage runs on 2*d channels
        self.pointwise_conv1 = nn.Conv1d(d_model, c2, 1)
        self.depthwise_conv = nn.Conv1d(c2, c2, kernel_size, padding=(kernel_size - 1) // 2, groups=c2)
        self.batch_norm = nn.BatchNorm1d(c2)
        self.pointwise_conv2 = nn.Conv1d(c2, d_model, 1)
        pw_max, dw_max = d_model ** -0.5, kernel_size ** -0.5  # reset_parameters_conv (conformer_modules.py:352-363)
        with torch.no_grad():
            for m, b in ((self.pointwise_conv1, pw_max), (self.pointwise_conv2, pw_max), (self.depthwise_conv, dw_max)):
                nn.init.uniform_(m.weight, -b, b)
                nn.init.uniform_(m.bias, -b, b)


class SqueezeformerLayer(nn.Module):  # squeezeformer_modules.py:60-203 (parameter layout only; compute lives in the encoder)
    def __init__(self, d_model, d_ff, n_heads, conv_kernel_size, adaptive_scale=True):
        super().__init__()
        self.norm_feed_forward1 = nn.LayerNorm(d_model)
        self.feed_forward1 = _FeedForward(d_model, d_ff)
        self.feed_forward1_scale = ScaleBiasLayer(d_model, adaptive_scale)
        self.norm_conv = nn.LayerNorm(d_model)
        self.conv = _SwishConvolution(d_model, conv_kernel_size)
        self.conv_scale = ScaleBiasLayer(d_model, adaptive_scale)
        self.norm_self_att = nn.LayerNorm(d_model)
        self.self_attn = _RelPosMHA(n_heads, d_model)
        self.self_attn_scale = ScaleBiasLayer(d_model, adaptive_scale)
        self.norm_feed_forward2 = nn.LayerNorm(d_model)
        self.feed_forward2 = _FeedForward(d_model, d_ff)
        self.feed_forward2_scale = ScaleBiasLayer(d_model, adaptive_scale)
        ffn1_max, ffn2_max = d_model ** -0.5, d_ff ** -0.5  # reset_parameters_ff (conformer_modules.py:400-408)
        with torch.no_grad():
            for ff in (self.feed_forward1, self.feed_forward2):
                nn.init.uniform_(ff.linear1.weight, -ffn1_max, ffn1_max); nn.init.uniform_(ff.linear1.bias, -ffn1_max, ffn1_max)
                nn.init.uniform_(ff.linear2.weight, -ffn2_max, ffn2_max); nn.init.uniform_(ff.linear2.bias, -ffn2_max, ffn2_max)


class TimeReductionModule(nn.Module):  # subsampling.py:589-656 (parameter layout only)
    def __init__(self, d_model: int, out_dim: int, kernel_size: int = 5, stride: int = 2):
        super().__init__()
        self.dw_conv = nn.Conv1d(d_model, d_model, kernel_size, stride=stride, padding=max(0, kernel_size - stride), groups=d_model)
        self.pw_conv = nn.Conv1d(d_model, out_dim, 1)
        dw_max, pw_max = kernel_size ** -0.5, d_model ** -0.5
        with torch.no_grad():
            for m, b in ((self.dw_conv, dw_max), (self.pw_conv, pw_max)):
                nn.init.uniform_(m.weight, -b, b)
                nn.init.uniform_(m.bias, -b, b)


class _Geo:
    """one frame rate of the temporal U-Net: B x T frames, valid lengths, positional table as a GEMM operand"""
    __slots__ = ("B", "T", "M", "lens", "pos", "P")


class _SqStep(_Step):
    """the step record of the Squeezeformer sequencer: + the frame-rate geometry of every layer and the temporal U-Net's detour"""
    __slots__ = ("geos", "front", "tr", "rec")

    def __init__(self, *grid):
        super().__init__(*grid)
        self.geos = []       # per layer: the _Geo it ran on
        self.front = None    # _LnSaved of pre_ln (x: its input)
        self.tr = self.rec = None   # _TimeReduce / _TimeRecover when the stages ran


_TimeReduce = _record("_TimeReduce", "x geo dwo")     # full-rate input, its _Geo, the depthwise conv's output
_TimeRecover = _record("_TimeRecover", "xs_c geo")    # the Linear's operand, the half-rate _Geo
# post-LN sub-blocks: x -> scale / bias -> y -> f -> r = x + dropout d_res (f(y)) -> LayerNorm (mean, rstd) -- layouts of their own, not the
# Conformer blocks' under the same names (d_in None: h holds swish'(h) * mask; core: _AttnCore / _ConvCore)
_SqFfSaved = _record("_SqFfSaved", "x y h a d_in d_res r mean rstd")
_SqAttSaved = _record("_SqAttSaved", "x y qkv p core ctx d_att d_res r mean rstd")
_SqConvSaved = _record("_SqConvSaved", "x y pw1 core z d_res r mean rstd")
_SqLayerSaved = _record("_SqLayerSaved", "att ff1 conv ff2")


class SqueezeformerEncoder(ConformerEncoder):
    def __init__(self, feat_in: int, n_layers: int, d_model: int, feat_out: int = -1, subsampling: str = "dw_striding",
                 subsampling_factor: int = 4, subsampling_conv_channels: int = -1, ff_expansion_factor: int = 4,
                 self_attention_model: str = "rel_pos", n_heads: int = 4, att_context_size=None, xscaling: bool = True,
                 untie_biases: bool = True, pos_emb_max_len: int = 5000, conv_kernel_size: int = 31,
                 conv_norm_type: str = "batch_norm", dropout: float = 0.1, dropout_emb: float = 0.1, dropout_att: float = 0.0,
                 adaptive_scale: bool = True, time_reduce_idx: Optional[int] = None, time_recovery_idx: Optional[int] = None,
                 compute_dtype: Optional[torch.dtype] = None):
        NeuralModule.__init__(self)
        bad = []
        if not (subsampling == "dw_striding" and subsampling_factor in (4, 8)):
            bad.append(f"subsampling={subsampling} x{subsampling_factor} (implemented: dw_striding x4 / x8)")
        if self_attention_model != "rel_pos": bad.append(f"self_attention_model={self_attention_model}")
        if att_context_size not in (None, [-1, -1], (-1, -1)): bad.append("limited att_context_size")
        if not untie_biases: bad.append("tied pos biases")
        if conv_norm_type != "batch_norm": bad.append(f"conv_norm_type={conv_norm_type}")
        if feat_out > 0 and feat_out != d_model: bad.append("feat_out projection")
        if conv_kernel_size not in (5, 9, 31): bad.append(f"conv_kernel_size={conv_kernel_size}")
        if d_model % n_heads or d_model % 4: bad.append("d_model not divisible by n_heads / 4")
        if bad:
            raise NotImplementedError("MI355X SqueezeformerEncoder does not implement: " + ", ".join(bad))
        self.time_reduce_idx = time_reduce_idx
        self.time_recovery_idx = None
        if time_reduce_idx is not None:
            self.time_recovery_idx = n_layers - 1 if time_recovery_idx is None else time_recovery_idx
            if time_reduce_idx < 0 or self.time_recovery_idx >= n_layers:
                raise ValueError(f"Time reduce index must lie between [0, {n_layers})")  # squeezeformer_encoder.py:169-173
            if self.time_recovery_idx < 0 or self.time_recovery_idx >= n_layers:
                raise ValueError(f"Time recovery index must lie between [0, {n_layers})")
            if self.time_recovery_idx <= time_reduce_idx:
                raise NotImplementedError("time_recovery_idx must follow time_reduce_idx")
        d_ff = d_model * ff_expansion_factor
        self.d_model, self.n_layers, self._feat_in = d_model, n_layers, feat_in
        self.n_heads, self.d_k, self.d_ff = n_heads, d_model // n_heads, d_ff
        self.conv_kernel_size = conv_kernel_size
        self.subsampling_factor = subsampling_factor
        self.self_attention_model = self_attention_model
        self.att_context_size = [-1, -1]
        self.att_context_size_all, self.att_context_probs, self._ctx = [[-1, -1]], [1.0], (0, -1, -1)
        self.layer_drop_probs, self.capture_layers, self.captured = [0.0] * n_layers, [], {}
        self.adaptive_scale = adaptive_scale
        self.xscale = math.sqrt(d_model) if xscaling else None
        # (RelPositionalEncoding's dropout on x is `dropout` here: squeezeformer_encoder.py:207-213)
        self.dropout, self.dropout_pre_encoder, self.dropout_att, self.dropout_emb = dropout, dropout, dropout_att, dropout_emb
        if subsampling_conv_channels == -1:
            subsampling_conv_channels = d_model
        self.subsampling = subsampling
        self.pre_encode = ConvSubsampling(subsampling, subsampling_factor, feat_in, d_model, subsampling_conv_channels)
        self._reset_pre_encode()
        self._feat_out = d_model
        self.pos_emb_max_len = pos_emb_max_len
        self.pos_enc = RelPositionalEncoding(d_model, dropout, pos_emb_max_len, self.xscale, dropout_emb)
        self.layers = nn.ModuleList([SqueezeformerLayer(d_model, d_ff, n_heads, conv_kernel_size, adaptive_scale)
                                     for _ in range(n_layers)])
        self.time_reduce_layer = self.time_recovery_layer = self.time_reduce_pos_enc = None
        if time_reduce_idx is not None:
            self.time_reduce_layer = TimeReductionModule(d_model, d_model, kernel_size=5, stride=2)
            self.time_recovery_layer = nn.Linear(d_model, d_model)
            self.time_reduce_pos_enc = RelPositionalEncoding(d_model, 0.0, pos_emb_max_len, None, 0.0)
        self.pre_ln = nn.LayerNorm(d_model)
        self.out_proj = None
        self.max_audio_length = pos_emb_max_len
        self.sync_max_audio_length = True
        self._init_engine(compute_dtype, tail=None)
        self.packed_rows = False  # (the packed token chain is built for the Conformer layer stack; the time-reduction stages keep the grid)

    def _reset_pre_encode(self):
        """ConvSubsampling.reset_parameters for 'dw_striding' (subsampling.py:438-459): Squeezeformer's initialisation"""
        pe = self.pre_encode
        with torch.no_grad():
            scale = 1.0 / 3
            dw_max, pw_max = 9 ** -0.5, pe._conv_channels ** -0.5
            nn.init.uniform_(pe.conv[0].weight, -scale, scale); nn.init.uniform_(pe.conv[0].bias, -scale, scale)
            for dw, pw in pe.dw_stages():
                nn.init.uniform_(dw.weight, -dw_max, dw_max); nn.init.uniform_(dw.bias, -dw_max, dw_max)
                nn.init.uniform_(pw.weight, -pw_max, pw_max); nn.init.uniform_(pw.bias, -pw_max, pw_max)
            fc = (self.d_model * self._feat_in / pe._sampling_num) ** -0.5
            nn.init.uniform_(pe.out.weight, -fc, fc); nn.init.uniform_(pe.out.bias, -fc, fc)

    # ------------------------------------------------------------------ geometry helpers
    @property
    def input_types(self):   # squeezeformer_encoder.py:37-45 (no bypass_pre_encode port)
        from collections import OrderedDict
        from ..core import LengthsType, NeuralType, SpectrogramType
        return OrderedDict({"audio_signal": NeuralType(("B", "D", "T"), SpectrogramType()),
                            "length": NeuralType(tuple("B"), LengthsType())})

    def _geometry(self, cdt):
        """(row pitch of [M, d] GEMM operands, padded head width, padded attention width)"""
        dp, dkp = _pad8(self.d_model), _pad8(self.d_k)  # (same layout in fp32: one code path, exercised by the parity tests)
        if cdt == torch.bfloat16 and self.use_flash_attention and self.flash_pad_heads and dkp < 64:
            dkp = 64  # narrow heads ride the fused d_k' = 64 attention kernels (ConformerEncoder._geometry)
        elif cdt == torch.bfloat16 and self.use_flash_attention and self.flash_pad_heads and 64 < dkp < 128:
            dkp = 128  # Medium: d = 324, 4 heads, d_k = 81 -> the fused kernels' second width (round 5)
        return dp, dkp, self.n_heads * dkp

    def _sub_channels(self, cdt):
        """(real, padded) channel count of the sub-sampling stack"""
        C_ = self.pre_encode._conv_channels
        return C_, (_pad8(C_) if cdt == torch.bfloat16 else C_)

    def _sub_io(self, Wf, cdt, dev, backward=False):
        C_, Cp = self._sub_channels(cdt)
        if Cp == C_:
            return super()._sub_io(Wf, cdt, dev, backward)
        pe = self.pre_encode
        d, F2 = self.d_model, pe._feat_after
        n = len(pe.dw_stages())
        io = _SubIO(Cp, Wf["pre.c0w"], Wf["pre.c0b"], [_DwWeights(Wf[f"pre.dw{i}w"], Wf[f"pre.dw{i}b"], Wf[f"pre.pw{i}b"]) for i in range(n)])
        if backward:
            sizes = [Cp * 9, Cp] + [Cp * 9, Cp, Cp * Cp, Cp] * n + [d * Cp * F2]
            offs = [0]
            for k in sizes:
                offs.append(offs[-1] + (k + 63) // 64 * 64)
            g = torch.zeros(offs[-1], dtype=torch.float32, device=dev)
            v = [g[offs[i]: offs[i] + sizes[i]] for i in range(len(sizes))]
            io.g_c0w, io.g_c0b = v[0], v[1]
            io.g_dw = [_DwGrads(*v[2 + 4 * i: 6 + 4 * i]) for i in range(n)]
            io.g_out = v[-1]

            def finish():  # real part of the padded gradients -> the parameters' gradients
                pe.conv[0].weight.grad.view(-1).add_(io.g_c0w[: C_ * 9])
                pe.conv[0].bias.grad.add_(io.g_c0b[:C_])
                for (dw, pw), gr in zip(pe.dw_stages(), io.g_dw):
                    dw.weight.grad.view(-1).add_(gr.dw_w[: C_ * 9])
                    dw.bias.grad.add_(gr.dw_b[:C_])
                    pw.weight.grad.view(C_, C_).add_(gr.pw_w.view(Cp, Cp)[:C_, :C_])
                    pw.bias.grad.add_(gr.pw_b[:C_])
                pe.out.weight.grad.add_(io.g_out.view(d, Cp * F2)[:, : C_ * F2])
            io.finish = finish
        return io

    def _declare_images(self, p, pf):
        cdt = p.dtype
        d, H, dk = self.d_model, self.n_heads, self.d_k
        dp, dkp, dA = self._geometry(cdt)
        pe = self.pre_encode
        C_, F2 = pe._conv_channels, pe._feat_after
        Cs, Cp = self._sub_channels(cdt)
        if Cp == Cs:
            for si_, (_, pw) in enumerate(pe.dw_stages()):
                p.add_matrix(f"pre.pw{si_}", pw.weight.data.view(C_, C_))
                p.add_matrix(f"pre.pw{si_}t", pw.weight.data.view(C_, C_), True)
            p.add_fc_permuted("pre.out", pe.out.weight.data, C_, F2)
            p.add_fc_permuted("pre.outt", pe.out.weight.data, C_, F2, transpose=True)
        else:  # zero-padded channels (see the module docstring): dense [Cp, 9] / [Cp] f32 copies + padded GEMM images
            def dense(name, t, n_pad):
                pf.new_image(name, 1, n_pad)
                pf.add_block(name, t.view(-1), 1, t.numel(), sr1=0, sc1=1)
            dense("pre.c0w", pe.conv[0].weight.data, Cp * 9); dense("pre.c0b", pe.conv[0].bias.data, Cp)
            for si_, (dw, pw) in enumerate(pe.dw_stages()):
                dense(f"pre.dw{si_}w", dw.weight.data, Cp * 9); dense(f"pre.dw{si_}b", dw.bias.data, Cp)
                dense(f"pre.pw{si_}b", pw.bias.data, Cp)
                w = pw.weight.data.view(C_, C_)
                p.new_image(f"pre.pw{si_}", Cp, Cp); p.add_block(f"pre.pw{si_}", w, C_, C_, sr1=C_, sc1=1)
                p.new_image(f"pre.pw{si_}t", Cp, Cp); p.add_block(f"pre.pw{si_}t", w, C_, C_, sr1=1, sc1=C_)
            wo_ = pe.out.weight.data  # [d, C*F2], column c*F2 + f  ->  image column f*Cp + c
            p.new_image("pre.out", d, F2 * Cp); p.new_image("pre.outt", F2 * Cp, d)
            for f in range(F2):
                p.add_block("pre.out", wo_.view(-1)[f:], d, C_, col_off=f * Cp, sr1=C_ * F2, sc1=F2)
                p.add_block("pre.outt", wo_.view(-1)[f:], C_, d, row_off=f * Cp, sr1=F2, sc1=C_ * F2)

        for i, L in enumerate(self.layers):
            for ff, m in (("ff1", L.feed_forward1), ("ff2", L.feed_forward2)):
                p.add_matrix(f"L{i}.{ff}.w1", m.linear1.weight.data); p.add_matrix(f"L{i}.{ff}.w1t", m.linear1.weight.data, True)
                p.add_matrix(f"L{i}.{ff}.w2", m.linear2.weight.data); p.add_matrix(f"L{i}.{ff}.w2t", m.linear2.weight.data, True)
            declare_padded_heads(p, pf, f"L{i}.att", L.self_attn, d, H, dk, dkp, dA)
            c = L.conv
            p.add_matrix(f"L{i}.conv.pw1", c.pointwise_conv1.weight.data); p.add_matrix(f"L{i}.conv.pw1t", c.pointwise_conv1.weight.data, True)
            p.add_matrix(f"L{i}.conv.pw2", c.pointwise_conv2.weight.data); p.add_matrix(f"L{i}.conv.pw2t", c.pointwise_conv2.weight.data, True)
        if self.time_reduce_layer is not None:
            p.add_matrix("tr.pw", self.time_reduce_layer.pw_conv.weight.data); p.add_matrix("tr.pwt", self.time_reduce_layer.pw_conv.weight.data, True)
            p.add_matrix("rec.w", self.time_recovery_layer.weight.data); p.add_matrix("rec.wt", self.time_recovery_layer.weight.data, True)

    def _geo(self, B, T, lens, pos_enc, d_emb, cdt, dev, dp):
        g = _Geo()
        g.B, g.T, g.M, g.lens, g.P = B, T, B * T, lens, 2 * T - 1
        key = (T, cdt, str(dev), dp, id(pos_enc))
        tab = self._pos_cache.get(key)
        if tab is None:
            tab = pos_enc.table(T, dev, torch.float32)
            if len(self._pos_cache) >= 32:
                self._pos_cache = {}
            self._pos_cache[key] = tab
        g.pos = self._new(g.P, dp, dtype=cdt, device=dev)
        ops.cast_pitched(tab, g.pos, g.P, self.d_model, dp, 1.0, d_emb)  # (+ dropout_emb on the table, :1097-1098)
        return g

    # ------------------------------------------------------------------ forward
    def _forward_impl(self, mel, length, save=False):
        dev = mel.device
        self._phase("f", dev)
        self._fwd_serial += 1
        cdt = self._cdt()
        training = self.training
        W, Wf = self._plan(cdt, dev)
        B, F_, T = mel.shape
        mel = mel.to(torch.float32).contiguous()
        d = self.d_model
        dp, dkp, dA = self._geometry(cdt)
        T1, F1 = (T - 1) // 2 + 1, (F_ - 1) // 2 + 1
        lens = self._lens(length, self.pre_encode._sampling_num)
        T2, F2 = T, F_
        for _ in range(self.pre_encode._sampling_num):
            T2, F2 = (T2 - 1) // 2 + 1, (F2 - 1) // 2 + 1
        M = B * T2
        self.update_max_seq_length(T2, dev)
        if training:
            self._step_seed = (self._step_seed + 1) & 0x3FFFFFFF
        seed = self._step_seed

        def drop(p, site):
            return ops.Dropout(p if training else 0.0, seed, site)

        S = _SqStep(B, F_, T, T1, F1, T2, F2, M, cdt, training, seed)
        S.serial, S.arena = self._fwd_serial, self._arena is not None
        S.mel, S.len0, S.len2, S.lens_all = mel, lens[0], lens[-1], lens
        S.drop_pre = drop(self.dropout_pre_encoder, 100000)
        x = self._sub_fwd_dw(S, mel, lens, W, cdt, save, Wf=Wf)
        # ---- pre_ln
        x0, pmean, prstd = self._ln_fwd(self.pre_ln, x, M, d, torch.float32, dev)
        S.front = _LnSaved(x, pmean, prstd)
        g_full = self._geo(B, T2, lens[-1], self.pos_enc, drop(self.dropout_emb, 100001), cdt, dev, dp)
        C2 = 2 * d
        S.bn_stats = torch.zeros(self.n_layers, 2 * C2 + 8, dtype=torch.float64, device=dev) if training else None
        S.bn_world = self._syncbn_world() if training else 1
        g = g_full
        x = x0
        for i, L in enumerate(self.layers):
            if self.time_reduce_idx is not None and i == self.time_reduce_idx:
                Th = (g.T + 1) // 2
                lens_h = (torch.div(g.lens + 1, 2, rounding_mode="floor")).contiguous()
                dwo = self._new(B * Th, dp, dtype=cdt, device=dev)
                tr = self.time_reduce_layer
                ops.time_reduce_dwconv_fwd(x, g.lens, tr.dw_conv.weight, tr.dw_conv.bias, dwo, B, g.T, d, dp)
                xh = self._new(B * Th, d, dtype=torch.float32, device=dev)
                ops.gemm(dwo, W["tr.pw"], xh, B * Th, d, d, dp, W.pitch("tr.pw"), d, bias=tr.pw_conv.bias)
                S.tr = _TimeReduce(x, g, dwo)
                g = self._geo(B, Th, lens_h, self.time_reduce_pos_enc, ops.NO_DROP, cdt, dev, dp)
                x = xh
            if self.time_reduce_idx is not None and i == self.time_recovery_idx:
                xs_in, g_skip = S.tr.x, S.tr.geo
                xs_c = self._new(g.M, dp, dtype=cdt, device=dev)
                ops.scale_bias_fwd(x, None, None, xs_c, g.M, d, dp)
                ys = self._new(g.M, d, dtype=torch.float32, device=dev)
                rec = self.time_recovery_layer
                ops.gemm(xs_c, W["rec.w"], ys, g.M, d, d, dp, W.pitch("rec.w"), d, bias=rec.bias)
                xr = self._new(g_skip.M, d, dtype=torch.float32, device=dev)
                ops.time_recover_fwd(xs_in, ys, xr, B, g_skip.T, d)
                S.rec = _TimeRecover(xs_c, g)
                g, x = g_skip, xr
            if training and S.bn_world > 1:
                S.bn_stats[i, 2 * C2] = float(g.M)
            x, sl = self._sq_layer_fwd(i, L, x, g, S, W, Wf, drop)
            S.layers.append(sl)
            S.geos.append(g)
        if training:
            torch._foreach_add_([L.conv.batch_norm.num_batches_tracked for L in self.layers], 1)
        out = x.view(B, T2, d).transpose(1, 2)
        return out, lens[-1], (S if save else None)

    def _sb_fwd(self, sb, x, M, cdt, dp):
        y = self._new(M, dp, dtype=cdt, device=x.device)
        ops.scale_bias_fwd(x, sb.scale, sb.bias, y, M, self.d_model, dp)
        return y

    def _post_ln(self, ln, r, M):
        return self._ln_fwd(ln, r, M, self.d_model, torch.float32, r.device)

    def _sq_ffn_fwd(self, S, pfx, ff, sb, ln, x, g, W, drop, site):
        M, d, dff, cdt, dev = g.M, self.d_model, self.d_ff, S.cdt, x.device
        dp = self._geometry(cdt)[0]
        y = self._sb_fwd(sb, x, M, cdt, dp)
        h = self._new(M, dff, dtype=cdt, device=dev)
        a = self._new(M, dff, dtype=cdt, device=dev)
        d_in, d_res = drop(self.dropout, site), drop(self.dropout, site + 1)
        g_form = self.swish_g and cdt == torch.bfloat16  # `h` then holds swish'(h) * mask (ConformerEncoder.__init__)
        ops.gemm(y, W[pfx + ".w1"], a, M, dff, d, dp, W.pitch(pfx + ".w1"), dff, bias=ff.linear1.bias,
                 epi=ops.EPI_SWISH_DROP_G if g_form else ops.EPI_SWISH_DROP, aux_out=h, drop=d_in)
        r = self._new(M, d, dtype=torch.float32, device=dev)
        ops.gemm(a, W[pfx + ".w2"], r, M, d, dff, dff, W.pitch(pfx + ".w2"), d, bias=ff.linear2.bias, epi=ops.EPI_RESID,
                 aux_in=x, drop=d_res)  # fc_factor = 1.0 (squeezeformer_modules.py:103)
        xo, mean, rstd = self._post_ln(ln, r, M)
        return xo, _SqFfSaved(x, y, h, a, None if g_form else d_in, d_res, r, mean, rstd)

    def _sq_layer_fwd(self, i, L, x, g, S, W, Wf, drop):
        B, T, M, cdt = g.B, g.T, g.M, S.cdt
        dev = x.device
        d = self.d_model
        dp, dkp, dA = self._geometry(cdt)
        site = i * 16
        # ---- rel-pos multi-head self-attention
        a = L.self_attn
        y = self._sb_fwd(L.self_attn_scale, x, M, cdt, dp)
        qkv = self._new(M, 3 * dA, dtype=cdt, device=dev)
        ops.gemm(y, W[f"L{i}.att.wqkv"], qkv, M, 3 * dA, d, dp, W.pitch(f"L{i}.att.wqkv"), 3 * dA, bias=Wf[f"L{i}.att.bqkv"])
        p = self._new(g.P, dA, dtype=cdt, device=dev)
        ops.gemm(g.pos, W[f"L{i}.att.wpos"], p, g.P, dA, d, dp, W.pitch(f"L{i}.att.wpos"), dA)
        d_att, d_res = drop(self.dropout_att, site + 2), drop(self.dropout, site + 3)
        ctx, core = self._attn_fwd(S, qkv, p, Wf[f"L{i}.att.bu"], Wf[f"L{i}.att.bv"], g.lens, B, T, dA, dkp, d_att)
        r = self._new(M, d, dtype=torch.float32, device=dev)
        ops.gemm(ctx, W[f"L{i}.att.wo"], r, M, d, dA, dA, W.pitch(f"L{i}.att.wo"), d, bias=a.linear_out.bias, epi=ops.EPI_RESID,
                 aux_in=x, drop=d_res)
        x1, mean, rstd = self._post_ln(L.norm_self_att, r, M)
        att = _SqAttSaved(x, y, qkv, p, core, ctx, d_att, d_res, r, mean, rstd)
        # ---- feed forward 1
        x2, ff1 = self._sq_ffn_fwd(S, f"L{i}.ff1", L.feed_forward1, L.feed_forward1_scale, L.norm_feed_forward1, x1, g, W, drop, site + 4)
        # ---- convolution module (Swish point-wise activation: 2*d channels through depthwise conv / BatchNorm)
        c = L.conv
        C2 = 2 * d
        y3 = self._sb_fwd(L.conv_scale, x2, M, cdt, dp)
        pw1 = self._new(M, C2, dtype=cdt, device=dev)
        ops.gemm(y3, W[f"L{i}.conv.pw1"], pw1, M, C2, d, dp, W.pitch(f"L{i}.conv.pw1"), C2, bias=c.pointwise_conv1.bias)
        ccore, z = self._conv_core_fwd(S, i, c, pw1, g.lens, B, T, C2, act=1)
        r3 = self._new(M, d, dtype=torch.float32, device=dev)
        d_cres = drop(self.dropout, site + 6)
        ops.gemm(z, W[f"L{i}.conv.pw2"], r3, M, d, C2, C2, W.pitch(f"L{i}.conv.pw2"), d, bias=c.pointwise_conv2.bias,
                 epi=ops.EPI_RESID, aux_in=x2, drop=d_cres)
        x3, mean3, rstd3 = self._post_ln(L.norm_conv, r3, M)
        conv = _SqConvSaved(x2, y3, pw1, ccore, z, d_cres, r3, mean3, rstd3)
        # ---- feed forward 2
        x4, ff2 = self._sq_ffn_fwd(S, f"L{i}.ff2", L.feed_forward2, L.feed_forward2_scale, L.norm_feed_forward2, x3, g, W, drop, site + 7)
        return x4, _SqLayerSaved(att, ff1, conv, ff2)

    # ------------------------------------------------------------------ backward
    def _branch_grad(self, S, ln, dxo, sv, M):
        """post-LN sub-block (sv: its saved record): -> (dr f32 [M,d] = d/d(x + branch), operand copy of the branch gradient [M, dp])"""
        d, dev, dp = self.d_model, dxo.device, self._geometry(S.cdt)[0]
        dr = self._new(M, d, dtype=torch.float32, device=dev)
        ops.layernorm_bwd(dxo, sv.r, ln.weight, sv.mean, sv.rstd, dr, False, ln.weight.grad, ln.bias.grad, M, d)
        df = self._new(M, dp, dtype=S.cdt, device=dev)
        ops.cast_pitched(dr, df, M, d, dp, 1.0, sv.d_res)
        return dr, df

    def _sb_bwd(self, sb, dy, x, dr, M, dp):
        ad = sb.adaptive_scale
        ops.scale_bias_bwd(dy, dp, x, sb.scale, dr, sb.scale.grad if ad else None, sb.bias.grad if ad else None, M, self.d_model)
        return dr

    def _sq_ffn_bwd(self, S, pfx, ff, sb, ln, sv, dxo, g, W):
        M, d, dff, cdt, dev = g.M, self.d_model, self.d_ff, S.cdt, dxo.device
        dp = self._geometry(cdt)[0]
        dr, df = self._branch_grad(S, ln, dxo, sv, M)
        self._wgrad(df, dp, 0, sv.a, dff, 0, ff.linear2.weight.grad, d, dff, M, bias_grad=ff.linear2.bias.grad)
        dh = self._new(M, dff, dtype=cdt, device=dev)
        if sv.d_in is None:
            ops.gemm(df, W[pfx + ".w2t"], dh, M, dff, d, dp, W.pitch(pfx + ".w2t"), dff, epi=ops.EPI_DSWISH_G, aux_in=sv.h)
        else:
            ops.gemm(df, W[pfx + ".w2t"], dh, M, dff, d, dp, W.pitch(pfx + ".w2t"), dff, epi=ops.EPI_DSWISH, aux_in=sv.h, drop=sv.d_in)
        self._wgrad(dh, dff, 0, sv.y, dp, 0, ff.linear1.weight.grad, dff, d, M, bias_grad=ff.linear1.bias.grad)
        dy = self._new(M, dp, dtype=cdt, device=dev)
        ops.gemm(dh, W[pfx + ".w1t"], dy, M, d, dff, dff, W.pitch(pfx + ".w1t"), dp)
        return self._sb_bwd(sb, dy, sv.x, dr, M, dp)

    # (the padded-head projection gradients and the conv core live in ConformerEncoder)
    def _sq_layer_bwd(self, i, L, dxo, g, S, sl, W, Wf):
        B, T, M, cdt = g.B, g.T, g.M, S.cdt
        dev = dxo.device
        d = self.d_model
        dp, dkp, dA = self._geometry(cdt)
        padded = dkp != self.d_k
        C2 = 2 * d
        # ---- feed forward 2
        dx = self._sq_ffn_bwd(S, f"L{i}.ff2", L.feed_forward2, L.feed_forward2_scale, L.norm_feed_forward2, sl.ff2, dxo, g, W)
        # ---- convolution module
        c, cv = L.conv, sl.conv
        dr, db = self._branch_grad(S, L.norm_conv, dx, cv, M)
        self._wgrad(db, dp, 0, cv.z, C2, 0, c.pointwise_conv2.weight.grad, d, C2, M, bias_grad=c.pointwise_conv2.bias.grad)
        dz = self._new(M, C2, dtype=cdt, device=dev)
        ops.gemm(db, W[f"L{i}.conv.pw2t"], dz, M, C2, d, dp, W.pitch(f"L{i}.conv.pw2t"), C2)
        dpw1, conv_tmp = self._conv_core_bwd(S, i, c, cv.core, cv.pw1, dz, g.lens, B, T, C2, act=1)   # noqa: F841 (conv_tmp: see there)
        self._wgrad(dpw1, C2, 0, cv.y, dp, 0, c.pointwise_conv1.weight.grad, C2, d, M, bias_grad=c.pointwise_conv1.bias.grad)
        dy3 = self._new(M, dp, dtype=cdt, device=dev)
        ops.gemm(dpw1, W[f"L{i}.conv.pw1t"], dy3, M, d, C2, C2, W.pitch(f"L{i}.conv.pw1t"), dp)
        dx = self._sb_bwd(L.conv_scale, dy3, cv.x, dr, M, dp)
        # ---- feed forward 1
        dx = self._sq_ffn_bwd(S, f"L{i}.ff1", L.feed_forward1, L.feed_forward1_scale, L.norm_feed_forward1, sl.ff1, dx, g, W)
        # ---- self-attention
        a, at = L.self_attn, sl.att
        dr, dao = self._branch_grad(S, L.norm_self_att, dx, at, M)
        if not padded:
            self._wgrad(dao, dp, 0, at.ctx, dA, 0, a.linear_out.weight.grad, d, d, M, bias_grad=a.linear_out.bias.grad)
        else:
            self._heads_out_wgrad(a, dao, at.ctx, M, ldx=dp)
        dctx = self._new(M, dA, dtype=cdt, device=dev)
        ops.gemm(dao, W[f"L{i}.att.wot"], dctx, M, dA, d, dp, W.pitch(f"L{i}.att.wot"), dA)
        dpos = torch.zeros(g.P, dA, dtype=torch.float32, device=dev)
        dpos_c = self._new(g.P, dA, dtype=cdt, device=dev)
        dqkv, dqu, dqv = self._attn_bwd(S, at.core, at.qkv, at.p, Wf[f"L{i}.att.bu"], Wf[f"L{i}.att.bv"], at.ctx, dctx, g.lens, B, T, dA,
                                        dkp, at.d_att, dpos, dpos_c)
        # q / k / v / linear_pos weight gradients (the flash path produced dpos_c on the weight-gradient stream: its consumer runs
        # there too; the GEMM path produced it on the main stream, which _wgrad_scope waits for)
        if not padded:
            ops.colsum(dqu, a.pos_bias_u.grad, M, dA)
            ops.colsum(dqv, a.pos_bias_v.grad, M, dA)
            ops.add2(dqu, dqv, dqkv, 3 * dA, M, dA)
            for j, lin in enumerate((a.linear_q, a.linear_k, a.linear_v)):
                self._wgrad(dqkv, 3 * dA, j * dA, at.y, dp, 0, lin.weight.grad, d, d, M, bias_grad=lin.bias.grad)
            self._wgrad(dpos_c, dA, 0, g.pos, dp, 0, a.linear_pos.weight.grad, d, d, g.P)
        else:
            sc, bias_sums = self._heads_qkv_grads(a, dqkv, dqu, dqv, at.y, M, ldx=dp)   # noqa: F841 (bias_sums: released with this frame)
            del sc   # (the pos-bias sums have always gone first here; off the step arena the order decides what the allocator reuses)
            self._heads_wgrad(dpos_c, dA, 0, g.pos, dp, a.linear_pos.weight.grad, g.P, 1, 0, 0)
        dy = self._new(M, dp, dtype=cdt, device=dev)
        ops.gemm(dqkv, W[f"L{i}.att.wqkvt"], dy, M, d, 3 * dA, 3 * dA, W.pitch(f"L{i}.att.wqkvt"), dp)
        return self._sb_bwd(L.self_attn_scale, dy, at.x, dr, M, dp)

    def _backward_impl(self, S, dout):
        B, M, cdt = S.B, S.M, S.cdt
        dev = dout.device
        self._check_serial(S)
        self._phase("b", dev)
        d = self.d_model
        W, Wf = self._plan(cdt, dev)
        fp = self._flatp
        dp, dkp, dA = self._geometry(cdt)
        dx = dout.transpose(1, 2).contiguous().view(M, d).to(torch.float32)
        C2 = 2 * d
        S.bn_sums = torch.zeros(self.n_layers, 2, C2, dtype=torch.float64, device=dev)
        # (the grouped launch takes any n_out / n_in: its operands are pitched, its epilogue is per-element atomics)
        self._wg_pending = [] if (self.wgrad_grouped and cdt == torch.bfloat16) else None
        dskip = None
        for i in range(self.n_layers - 1, -1, -1):
            g = S.geos[i]
            dx = self._sq_layer_bwd(i, self.layers[i], dx, g, S, S.layers[i], W, Wf)
            self._wgrad_flush()
            S.layers[i] = None
            if self.time_reduce_idx is not None and i == self.time_recovery_idx:
                # x = skip + Linear(repeat_interleave(x_small, 2)[:, :T]): the skip gradient waits for the time-reduction backward
                xs_c, g_small = S.rec.xs_c, S.rec.geo
                rec = self.time_recovery_layer
                dskip = dx
                dys = self._new(g_small.M, dp, dtype=cdt, device=dev)
                ops.time_recover_bwd(dx, dys, B, g.T, d, dp)
                self._wgrad(dys, dp, 0, xs_c, dp, 0, rec.weight.grad, d, d, g_small.M, bias_grad=rec.bias.grad)
                self._wgrad_flush()
                dx = self._new(g_small.M, d, dtype=torch.float32, device=dev)
                ops.gemm(dys, W["rec.wt"], dx, g_small.M, d, d, dp, W.pitch("rec.wt"), d)
            if self.time_reduce_idx is not None and i == self.time_reduce_idx:
                x_in, g_full, dwo = S.tr.x, S.tr.geo, S.tr.dwo
                tr = self.time_reduce_layer
                Mh = g.M
                dxc = self._new(Mh, dp, dtype=cdt, device=dev)
                ops.cast_pitched(dx, dxc, Mh, d, dp)
                self._wgrad(dxc, dp, 0, dwo, dp, 0, tr.pw_conv.weight.grad, d, d, Mh, bias_grad=tr.pw_conv.bias.grad)
                self._wgrad_flush()
                ddw = self._new(Mh, dp, dtype=cdt, device=dev)
                ops.gemm(dxc, W["tr.pwt"], ddw, Mh, d, d, dp, W.pitch("tr.pwt"), dp)
                ops.time_reduce_dwconv_bwd(ddw, dp, x_in, g_full.lens, tr.dw_conv.weight, dskip, tr.dw_conv.weight.grad,
                                           tr.dw_conv.bias.grad, B, g_full.T, d)
                dx, dskip = dskip, None
            if self.grad_ready_hook is not None:
                if self._wgrad_join_per_layer:
                    self._wgrad_join()
                self._hook(*fp.range_of(f"layers.{i}."))
        self._wg_pending = None
        dpre = self._new(M, d, dtype=torch.float32, device=dev)
        ops.layernorm_bwd(dx, S.front.x, self.pre_ln.weight, S.front.mean, S.front.rstd, dpre, False, self.pre_ln.weight.grad, self.pre_ln.bias.grad, M, d)
        self._wgrad_join()
        if self.grad_ready_hook is not None:
            for pfx in ("pre_ln.", "time_reduce_layer.", "time_recovery_layer."):
                try:
                    self._hook(*fp.range_of(pfx))
                except KeyError:
                    pass
        return self._sub_bwd_dw(S, dpre, W, cdt, Wf=Wf)
