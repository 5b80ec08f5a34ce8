"""Forced alignment of known token ids on a transducer head (RNN-T or TDT): the decoder's teacher-forced forward, the joint's
sub-batched forward, and the Viterbi pass over the lattice the losses sum over (`csrc/transducer_align.hip`,
`mi355x_transducer_align_rows` / `mi355x_transducer_align`; include/mi355x_asr.h states the rule).  The [B, T, U+1, V+1] logits
exist for one sub-batch of `joint.fused_batch_size` utterances at a time, as in the fused loss; what stays per cell are 2 + D
log-probabilities.  There is no CPU path: CPU tensors raise."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from .. import ops


class TransducerAligner:
    """`decoder`: RNNTDecoder (any number of layers) or StatelessTransducerDecoder -- whatever has the training forward; `joint`:
    RNNTJoint; `durations` given: the joint's extra outputs are the TDT duration logits."""

    def __init__(self, decoder, joint, durations: Optional[Sequence[int]] = None):
        self.decoder, self.joint = decoder, joint
        self.durations = [int(d) for d in durations] if durations else None
        extra = int(getattr(joint, "_num_extra_outputs", 0))
        if extra != (len(self.durations) if self.durations else 0):
            raise ValueError(f"the joint has {extra} extra outputs for {len(self.durations or [])} durations")
        self.blank_id = int(decoder.blank_idx)

    @torch.no_grad()
    def __call__(self, encoder_output: torch.Tensor, encoded_lengths: torch.Tensor, targets: torch.Tensor,
                 target_lengths: torch.Tensor, return_rows: bool = False):
        """encoder_output [B, D, T], encoded_lengths [B], targets [B, U], target_lengths [B] (device) -> (tok_frame i32 [B, U]: the
        frame each label is emitted on, tok_dur i32 [B, U]: its duration (RNN-T: 0), score f32 [B]), -1 padded; an utterance that
        cannot be aligned has score -inf and -1 everywhere.  return_rows: also the lattice inputs f32 [B, T, U+1, 2 + D]."""
        decoder, joint = self.decoder, self.joint
        if decoder.training or joint.training:
            raise RuntimeError("TransducerAligner runs in eval mode (no dropout): call .eval() on the decoder and the joint")
        if encoder_output.dim() != 3:
            raise ValueError(f"`encoder_output` must be a tensor of shape [B, D, T]. Provided shape = {tuple(encoder_output.shape)}")
        dev = encoder_output.device
        U = targets.shape[1]
        tg = targets.to(torch.int64)
        if U == 0:   # (a batch of empty transcripts: the prediction network wants a column)
            tg = tg.new_zeros(tg.shape[0], 1)
        tg = tg.contiguous()
        el, tl = encoded_lengths.to(torch.int64).contiguous(), target_lengths.to(torch.int64).contiguous()
        dec_out, _, _ = decoder(targets=tg, target_length=tl)
        joint._flatp.ensure(dev)
        cdt = joint._cdt()
        W, _ = joint._plan(cdt, dev)
        B, _, T = encoder_output.shape
        U1 = dec_out.shape[2]
        D = len(self.durations) if self.durations else 0
        width, V1 = joint._num_classes, joint._num_classes - D   # the whole logit row; its label part
        _, _, f, g = joint._project(encoder_output, dec_out, W, cdt)
        rows = torch.empty(B, T, U1, 2 + D, dtype=torch.float32, device=dev)
        fbs = int(joint.fused_batch_size or B)
        for b0 in range(0, B, fbs):
            nb = min(fbs, B - b0)
            h, logits = joint._sub_fwd(f, g, b0, nb, T, U1, W, cdt, ops.NO_DROP)
            ops.transducer_align_rows(logits, width, tg[b0:b0 + nb], el[b0:b0 + nb], tl[b0:b0 + nb], nb, T, U1, V1, D, self.blank_id,
                                      rows[b0:b0 + nb])
            del h, logits
        tok_frame, tok_dur, score = ops.transducer_align(rows, el, tl, self.durations)
        out = (tok_frame[:, :U], tok_dur[:, :U], score)
        return out + (rows,) if return_rows else out
