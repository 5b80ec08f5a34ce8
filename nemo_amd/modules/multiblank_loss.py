"""Drop-in for `MultiblankRNNTLossNumba` (`nemo/collections/asr/parts/numba/rnnt_loss/rnnt_pytorch.py`, selected as loss_name
'multiblank_rnnt' by `losses/rnnt.py`): the multi-blank transducer objective (Xu et al., 2022).  The joint network's logits
`acts [B, T, U+1, V+1+nb]` go in -- the V labels, then the nb big blanks, the standard blank last (`blank` = V + nb, big blank i =
output blank - 1 - i, consuming `big_blank_durations[i]` frames); the log-softmax over all of them is fused into the loss kernels,
and the gradient w.r.t. the logits is produced in the forward call and handed out (scaled by the upstream gradient) in backward
(`csrc/multiblank.hip`, C-ABI `mi355x_multiblank_loss_ex`; `include/mi355x_asr.h` states the rule, written from memory of the
reference).  There is no CPU path: CPU tensors raise."""
from __future__ import annotations

from typing import Sequence

import torch  # noqa: F401
from torch import nn

from .. import ops
from .rnnt_loss import _TransducerLossFn, prepare_inputs


def check_big_blank_durations(durations: Sequence[int]) -> list:
    """the big-blank set: 1 to 7 integers in 2..8, strictly ascending"""
    d = list(durations) if durations is not None else []
    if not all(isinstance(x, int) and not isinstance(x, bool) for x in d):
        raise ValueError(f"big_blank_durations must be integers, got {d}")
    if not 1 <= len(d) <= 7 or d[0] < 2 or d[-1] > 8 or any(b <= a for a, b in zip(d, d[1:])):
        raise ValueError(f"big_blank_durations must be 1 to 7 strictly ascending integers in 2..8, got {d}")
    return d


class MultiblankRNNTLoss(nn.Module):
    """`MultiblankRNNTLossNumba(blank, big_blank_durations, reduction='mean', fastemit_lambda=0.0, clamp=-1, sigma=0.0)`.
    FastEmit and gradient clamping have no multi-blank form here: fastemit_lambda > 0 or clamp > 0 raise NotImplementedError."""

    def __init__(self, blank: int, big_blank_durations, reduction: str = "mean", fastemit_lambda: float = 0.0, clamp: float = -1,
                 sigma: float = 0.0):
        super().__init__()
        if fastemit_lambda and fastemit_lambda > 0:
            raise NotImplementedError("multi-blank loss: fastemit_lambda > 0 is not implemented")
        if clamp is not None and clamp > 0:
            raise NotImplementedError("multi-blank loss: clamp > 0 is not implemented")
        if sigma < 0:
            raise ValueError(f"multi-blank loss: sigma must be >= 0, got {sigma}")
        self.blank = int(blank)
        self.big_blank_durations = check_big_blank_durations(big_blank_durations)
        self.reduction = reduction
        self.fastemit_lambda = 0.0
        self.clamp = 0.0
        self.sigma = float(sigma)

    def forward(self, acts, labels, act_lens, label_lens):
        """acts (batch x seqLength x labelLength x (V+1+nb)) logits; labels zero-padded [B, U]; lens [B]"""
        inputs = prepare_inputs("MultiblankRNNTLoss", acts, labels, act_lens, label_lens)

        def kernels(acts, labels, act_lens, label_lens, grads, scale):
            B, T, U1, N = acts.shape
            return ops.multiblank_loss_pitched(acts, N, B, T, U1, N, self.big_blank_durations, labels, act_lens, label_lens,
                                               self.blank, grads=grads, ld_grads=N, sigma=self.sigma, grad_scale=scale)

        return _TransducerLossFn.apply(*inputs, self.reduction, kernels)


MultiblankRNNTLossNumba = MultiblankRNNTLoss
