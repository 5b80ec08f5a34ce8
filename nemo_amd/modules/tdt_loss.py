"""Drop-in for `TDTLossNumba` (`nemo/collections/asr/parts/numba/rnnt_loss/rnnt_pytorch.py`, selected as loss_name 'tdt' by
`losses/rnnt.py`): the Token-and-Duration Transducer objective (Xu et al., 2023).  The joint network's logits
`acts [B, T, U+1, V+1+D]` go in -- V+1 label logits (blank = V), then one logit per duration -- both log-softmaxes are fused
into the loss kernels, and the gradient w.r.t. the logits is produced in the forward call and handed out (scaled by the
upstream gradient) in backward (`csrc/tdt.hip`, C-ABI `mi355x_tdt_loss_ex`).  There is no CPU path: CPU tensors raise."""
from __future__ import annotations

from typing import Sequence

import torch
from torch import nn

from .. import ops
from .rnnt_loss import _TransducerLossFn, certify_inputs, prepare_inputs  # noqa: F401  (certify_inputs: a public name here)


def check_durations(durations: Sequence[int]) -> list:
    """the duration set: integers, strictly ascending, starting at 0, ending at <= 8, at most 8 entries, one of them non-zero"""
    d = list(durations)
    if not all(isinstance(x, int) and not isinstance(x, bool) for x in d):
        raise ValueError(f"TDT durations must be integers, got {d}")
    if len(d) < 2 or len(d) > 8 or d[0] != 0 or d[-1] > 8 or any(b <= a for a, b in zip(d, d[1:])):
        raise ValueError(f"TDT durations must be strictly ascending, start at 0, end at <= 8 and have at most 8 entries "
                         f"(at least one non-zero), got {d}")
    return d


def draw_rnnt_call(omega: float) -> bool:
    """Whether this loss call computes the conventional RNN-T loss of the label logits instead of TDT.

    Restated from memory of the reference's GPU implementation (`gpu_rnnt.py`, `GPUTDT`), which could not be re-read: with
    probability `omega` a call uses the RNN-T loss of `acts[..., :V+1]` (no sigma, zero duration gradients).  One host-side
    uniform draw per call from torch's default CPU generator; `omega = 0` and `omega = 1` draw nothing and are deterministic."""
    if omega <= 0.0:
        return False
    if omega >= 1.0:
        return True
    return float(torch.rand(()).item()) < omega


class TDTLoss(nn.Module):
    """`TDTLossNumba(blank, durations=None, reduction='mean', fastemit_lambda=0.0, clamp=-1, sigma=0.0, omega=0.0)`.
    FastEmit and gradient clamping have no TDT form here: fastemit_lambda > 0 or clamp > 0 raise NotImplementedError."""

    def __init__(self, blank: int, durations=None, reduction: str = "mean", fastemit_lambda: float = 0.0, clamp: float = -1,
                 sigma: float = 0.0, omega: float = 0.0):
        super().__init__()
        if fastemit_lambda and fastemit_lambda > 0:
            raise NotImplementedError("TDT loss: fastemit_lambda > 0 is not implemented")
        if clamp is not None and clamp > 0:
            raise NotImplementedError("TDT loss: clamp > 0 is not implemented")
        if sigma < 0:
            raise ValueError(f"TDT loss: sigma must be >= 0, got {sigma}")
        if not 0.0 <= omega <= 1.0:
            raise ValueError(f"TDT loss: omega must lie in [0, 1], got {omega}")
        self.blank = blank
        self.durations = check_durations(durations if durations is not None else [])
        self.reduction = reduction
        self.fastemit_lambda = 0.0
        self.clamp = 0.0
        self.sigma = float(sigma)
        self.omega = float(omega)

    def forward(self, acts, labels, act_lens, label_lens):
        """acts (batch x seqLength x labelLength x (V+1+D)) logits; labels zero-padded [B, U]; lens [B]"""
        inputs = prepare_inputs("TDTLoss", acts, labels, act_lens, label_lens)
        use_rnnt = draw_rnnt_call(self.omega)

        def kernels(acts, labels, act_lens, label_lens, grads, scale):
            B, T, U1, W = acts.shape
            V1 = W - len(self.durations)
            if use_rnnt:
                # the RNN-T loss of the label logits: the loss kernels read the [.., :V1] columns of the pitched rows and write the
                # duration columns of the gradient as zeros (pad columns of a pitched row)
                return ops.rnnt_loss_pitched(acts, W, B, T, U1, V1, labels, act_lens, label_lens, self.blank, grads, W,
                                             grad_scale=scale)
            return ops.tdt_loss_pitched(acts, W, B, T, U1, V1, self.durations, labels, act_lens, label_lens, self.blank,
                                        grads=grads, ld_grads=W, sigma=self.sigma, grad_scale=scale)

        return _TransducerLossFn.apply(*inputs, self.reduction, kernels)


TDTLossNumba = TDTLoss
