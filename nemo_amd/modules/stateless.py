"""Drop-in for `nemo.collections.asr.modules.StatelessTransducerDecoder` (the `StatelessNet` prediction network) on MI355X: the
prediction network without a recurrence.  It embeds the last `context_size` labels, one embedding table per position (state-dict keys
`prediction.embeds.{i}.weight`, i = 0 the most recent label, row `blank` the zero padding row), and concatenates the results.
include/mi355x_asr.h states the rule (mi355x_stateless_*); it was written from memory of the reference, so parity with the
reference's numbers is not claimed -- the rule is the contract.

Same typed call as `RNNTDecoder` (`targets`, `target_length` -> `[B, pred_hidden, U + 1]`, lengths, None), so the joint, the fused
joint + loss step and the models take it unchanged.  Forward and backward are the two training kernels of csrc/stateless.hip under one
autograd node; the greedy decoders recognise the class and search with `ops.stateless_greedy_decode` over the prediction tables
(`search_tables`, rebuilt when the weights moved).  Not implemented, refused by name: `normalization_mode` (LayerNorm inside the net),
`random_state_sampling`, `blank_as_pad=False`, `context_size` > 4."""
from __future__ import annotations

from collections import OrderedDict
from typing import Any, Dict, Optional

import torch
from torch import nn

from .. import ops
from ..core import ElementType, EmbeddedTextType, LabelsType, LengthsType, NeuralType, typecheck
from .rnnt import _TransducerModule


class _StatelessFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, token, module, targets):
        g, saved = module._forward_impl(targets)
        ctx.module, ctx.saved = module, saved
        return g

    @staticmethod
    def backward(ctx, dg):
        ctx.module._backward_impl(ctx.saved, dg)
        ctx.saved = None
        return None, None, None


class StatelessTransducerDecoder(_TransducerModule):
    @property
    def input_types(self):
        return OrderedDict({"targets": NeuralType(("B", "T"), LabelsType()),
                            "target_length": NeuralType(tuple("B"), LengthsType()),
                            "states": NeuralType(("D", "B", "D"), ElementType(), optional=True)})

    @property
    def output_types(self):
        return OrderedDict({"outputs": NeuralType(("B", "D", "T"), EmbeddedTextType()),
                            "prednet_lengths": NeuralType(tuple("B"), LengthsType()),
                            "states": NeuralType(("D", "B", "D"), ElementType(), optional=True)})

    def __init__(self, prednet: Dict[str, Any], vocab_size: int, context_size: int = 1, normalization_mode: Optional[str] = None,
                 random_state_sampling: bool = False, blank_as_pad: bool = True, compute_dtype: Optional[torch.dtype] = None):
        super().__init__()
        bad = []
        if normalization_mode is not None: bad.append(f"normalization_mode={normalization_mode} (LayerNorm inside the stateless net)")
        if random_state_sampling: bad.append("random_state_sampling")
        if not blank_as_pad: bad.append("blank_as_pad=False")
        if int(context_size) > 4: bad.append(f"context_size={context_size} (at most 4)")
        if bad:
            raise NotImplementedError("MI355X StatelessTransducerDecoder does not implement: " + ", ".join(bad))
        self.pred_hidden = int(prednet["pred_hidden"])
        self.context_size = int(context_size)
        self.vocab_size, self.blank_idx, self.blank_as_pad = vocab_size, vocab_size, blank_as_pad
        self.dropout = float(prednet.get("dropout", 0.0) or 0.0)
        if self.pred_hidden % 4:
            raise ValueError("pred_hidden must be a multiple of 4 (8 for bf16 compute): 16-byte vector accesses")
        self.widths = ops.stateless_widths(self.pred_hidden, self.context_size)   # ValueError for context_size < 1
        self.prediction = nn.ModuleDict({"embeds": nn.ModuleList(
            [nn.Embedding(vocab_size + 1, e, padding_idx=self.blank_idx) for e in self.widths])})
        self._init_engine(compute_dtype)
        self._tables = None   # (key, tables): the search's prediction tables of the current weights

    def _declare_images(self, p, pf):   # no GEMM operands: the network is C table look-ups
        pass

    def _embs(self):
        return [e.weight for e in self.prediction["embeds"]]

    @typecheck()
    def forward(self, targets, target_length, states=None):
        if states is not None:
            raise NotImplementedError("stateful prediction (decoding) is not on the training hot path")
        self._flatp.ensure(targets.device)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            g = _StatelessFn.apply(self._tok(targets.device), self, targets)
        else:
            g = self._forward_impl(targets)[0]
        return g, target_length, None

    def _forward_impl(self, targets):
        if self.training:
            self._step_seed = (self._step_seed + 1) & 0x3FFFFFFF
        drop = ops.Dropout(self.dropout if self.training else 0.0, self._step_seed, 200)
        tg = targets.to(torch.int64).contiguous()
        g = ops.stateless_pred_fwd(tg, self._embs(), self.blank_idx, out_dtype=self._cdt(), drop=drop)
        return g.transpose(1, 2), (tg, drop)   # [B, E, U + 1] (a view: the joint re-lays it out once)

    def _backward_impl(self, saved, dg):
        tg, drop = saved
        dg = dg.transpose(1, 2).contiguous()   # [B, U + 1, E]; no copy for the joint's gradient
        if dg.dtype not in (torch.float32, torch.bfloat16):
            dg = dg.float()
        ops.stateless_embed_bwd(tg, dg, [w.grad for w in self._embs()], self.blank_idx, accumulate=True, drop=drop)
        if self.grad_ready_hook is not None:
            self.grad_ready_hook(0, self._flatp.flat.numel())

    @torch.no_grad()
    def search_tables(self, joint, device):
        """the prediction tables P_i = emb_i . W_pred[:, slice i]^T f32 [C, V1, J] of the greedy search, from the joint's bf16 image
        of W_pred in bf16 compute and its fp32 master otherwise.  Cached under the engine's contract for weight images, in fp32
        too: rebuilt when either module's `weights_updated()` was called (the optimizers and `load_state_dict` call it) or its flat
        storage was rebuilt -- an in-place edit of an embedding or of W_pred without `weights_updated()` leaves the tables stale"""
        self._flatp.ensure(device)
        cdt = joint._cdt()
        key = (cdt, str(device), self._weights_version, self._flatp.generation, joint._weights_version, joint._flatp.generation)
        if self._tables is None or self._tables[0] != key:
            if cdt == torch.bfloat16:
                Wj = joint._plan(cdt, device)[0]
                w, ld = Wj["pred.w"], Wj.pitch("pred.w")
            else:
                w, ld = joint.pred.weight, self.pred_hidden
            self._tables = (key, ops.stateless_tables(self._embs(), w, ld, self.blank_idx))
        return self._tables[1]
