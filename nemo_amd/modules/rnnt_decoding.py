"""Greedy transducer decoding and WER for the drop-in FastConformer-Transducer model.

Mirrors the pieces of the reference a training run touches (names, argument meaning, return shapes):
  * `GreedyBatchedRNNTInfer` (parts/submodules/rnnt_greedy_decoding.py:529): `forward(encoder_output [B, D, T], encoded_lengths)`
    -> a 1-tuple holding the list of `Hypothesis` (y_sequence, timestamp, score);
  * `RNNTDecoding.rnnt_decoder_predictions_tensor` (parts/submodules/rnnt_decoding.py:430-520): hypotheses with `.text`;
  * `WER` for transducers (metrics/wer.py:210-356: `update(predictions = encoder output, predictions_lengths, targets,
    targets_lengths)` decodes, then accumulates edit distance / reference words).
The reference's search is a Python loop over frames with a device -> host sync per inner iteration; here the whole batch is ONE
launch (`mi355x_transducer_greedy_decode`, csrc/rnnt_decode.hip): the encoder projection is a GEMM, a workgroup per utterance runs the
LSTM / joint / arg-max recurrence out of LDS, and only the token ids leave the device -- when text is asked for.

Four documented differences to the reference's search (token ids / time stamps / lengths are bit-identical to it, tests/test_rnnt_decoding.py):
  * `Hypothesis.score` is the sum of the emitted labels' log-probabilities (the reference's CPU behaviour); on CUDA tensors the
    reference sums raw maximum logits because `_joint_step(log_normalize=None)` skips log_softmax there (rnnt_greedy_decoding.py:257-259);
  * `max_symbols_per_step=None` is unbounded per frame in the reference; here an utterance stops once 4 * T labels are out
    (a model that never emits blank cannot hang the device; `out_len == 4 * T` marks the cut);
  * streaming (`partial_hypotheses`): `Hypothesis.timestamp` holds GLOBAL frame indices (frames of all earlier chunks counted);
    the reference appends chunk-local ones;
  * streaming with `max_symbols_per_step=None`: the safety budget of 4 * T labels applies per chunk (T = the chunk's frames).

Streaming: `forward(..., partial_hypotheses=hyps)` (the first chunk: `hyps = decoder.fresh_hypotheses(B)`; without
`partial_hypotheses` the call is the one-shot search it has always been) resumes every stream from the decoder state its hypothesis carries
(`Hypothesis.dec_state`, an `ops.RNNTStreamState` of batch 1 on the device: committed LSTM state, last label, running score, frames
done, and for TDT the frames a duration already jumped over) through the resumable search (the same entry with a
state to write); the returned hypotheses cover the whole stream so far and are new objects.  Over the same
encoder-projection values, any cut into chunks gives bit-identical hypotheses to one call over the concatenation.

Confidence (`confidence_cfg`, modules/confidence.py): with token or word confidence asked for the search runs through the `_conf`
functions of `ops` (the same entry with a measure in the descriptor): the measure of the label distribution of every step that emitted
a label, computed inside the search from the logits it already holds.  `Hypothesis.token_confidence` has one value per label
(streaming: appended chunk by chunk) whenever token OR word confidence is preserved, since `RNNTDecoding` folds the words'
`word_confidence` from it.  Blank steps are not kept, so
`preserve_frame_confidence` (and `preserve_alignments`) stay unavailable.

Shallow fusion (`fusion_models=[(NGramLM | BoostingTree, alpha), ...]`, one or two; `decoding.greedy.ngram_lm_arpa` /
`decoding.greedy.boosting_tree` in a model's config): the search runs through `ops.transducer_greedy_decode_fused`, whose rule
include/mi355x_asr.h states -- a step whose arg-max is a label emits the label that ranks highest with the models' look-ups added,
a blank stays a blank, and the score of a hypothesis carries the models' terms, a phrase begun and not finished taken back.  The
stream state is an `ops.RNNTFusedStreamState` (one automaton state per model and stream) and a streaming `Hypothesis.score` is the
kernel's `score` output, so it equals the one-shot score.  Without models every call is exactly what it was.  Together with token
or word confidence it is refused (the measure belongs to the unfused distribution).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, NamedTuple, Optional, Sequence

import torch

from .. import ops
from .ctc_decoding import _levenshtein


@dataclass
class Hypothesis:  # parts/utils/rnnt_utils.py:35-110 (the fields greedy decoding fills)
    score: float
    y_sequence: torch.Tensor
    timestamp: List[int] = field(default_factory=list)
    text: Optional[str] = None
    dec_state: Optional[object] = None   # one-shot search: the final (h, c) ([H] each; L > 1 layers: [L, H]); streaming: ops.RNNTStreamState of this stream (batch 1, device)
    length: int = 0
    last_token: Optional[torch.Tensor] = None   # i32 [1] on the device (= dec_state.last); blank before the first label
    frame_confidence: Optional[List[float]] = None   # CTC: one value per frame of the utterance
    token_confidence: Optional[List[float]] = None   # one value per label of y_sequence
    word_confidence: Optional[List[float]] = None    # one value per word of the text
    n_best: Optional[list] = None   # streaming CTC beam search with return_best_hypothesis off: (text, ids, score), best first
    stable_length: int = 0   # streaming CTC beam search: the leading tokens of y_sequence that are committed (final); monotone


class FusedChunk(NamedTuple):
    """what `decode_ids_stream` returns with `fusion_models`: the plain search's four results under their names, and `score`"""
    tokens: torch.Tensor    # i32 [B, N], -1 padded: this chunk's labels
    frames: torch.Tensor    # i32 [B, N]: their GLOBAL frame indices
    lengths: torch.Tensor   # i32 [B]
    state: object           # ops.RNNTFusedStreamState: the next state (its `score` is the running score)
    score: torch.Tensor     # f32 [B]: the stream's score so far, the models' final terms included


class GreedyBatchedRNNTInfer:
    def __init__(self, decoder_model, joint_model, blank_index: int, max_symbols_per_step: Optional[int] = None,
                 preserve_alignments: bool = False, preserve_frame_confidence: bool = False, confidence_cfg=None,
                 fusion_models=None, **unused):
        from .confidence import confidence_from
        self.confidence_cfg = confidence_from(confidence_cfg)   # None: no confidence, the search is what it was
        self.fusion_models = list(fusion_models) if fusion_models else None   # None: no fusion, the search is what it was
        if self.fusion_models is not None and self.confidence_cfg is not None and self.confidence_cfg.wants_tokens:
            raise NotImplementedError("`fusion_models` together with a `confidence_cfg` that preserves token or word confidence: the "
                                      "fused search computes no confidences")
        if preserve_alignments or preserve_frame_confidence or (self.confidence_cfg is not None
                                                                and self.confidence_cfg.preserve_frame_confidence):
            # the search keeps the steps that emitted a label: per-step blank confidences / alignments are not stored
            raise NotImplementedError("alignments / frame confidences are not produced by the on-device search")
        if max_symbols_per_step is not None and max_symbols_per_step <= 0:
            raise ValueError(f"Expected max_symbols_per_step > 0 (or None), got {max_symbols_per_step}")  # rnnt_greedy_decoding.py:187
        self.pred_layers = int(getattr(decoder_model, "pred_rnn_layers", 1))
        if not 1 <= self.pred_layers <= 4:
            raise NotImplementedError(f"on-device greedy search: at most 4 LSTM layers in the prediction network, got pred_rnn_layers = "
                                      f"{self.pred_layers}")
        self.decoder, self.joint = decoder_model, joint_model
        self._blank_index = int(blank_index)
        self.max_symbols = max_symbols_per_step

    def _project(self, encoder_output: torch.Tensor):
        """encoder_output [B, D, T] -> (enc_proj [B, T, J] in the compute dtype, the search's weight arguments)"""
        if encoder_output.dim() != 3:
            raise ValueError(f"`encoder_output` must be [B, D, T]; got shape {tuple(encoder_output.shape)}")
        dec, jnt = self.decoder, self.joint
        dev = encoder_output.device
        B, D, T = encoder_output.shape
        cdt = jnt._cdt()
        lstm = dec.prediction["dec_rnn"].lstm
        emb = dec.prediction["embed"].weight
        out = jnt.joint_net[-1]
        xe32 = encoder_output.transpose(1, 2).contiguous().view(B * T, D).float()
        J = jnt.joint_hidden
        if cdt == torch.bfloat16:   # the GEMM operand images the training step keeps up to date
            Wj, Wd = jnt._plan(cdt, dev)[0], dec._plan(cdt, dev)[0]
            xe = torch.empty(B * T, D, dtype=cdt, device=dev)
            ops.drop_scale_cast(xe32, xe, B * T * D, 1.0)
            f = torch.empty(B * T, J, dtype=cdt, device=dev)
            ops.gemm(xe, Wj["enc.w"], f, B * T, J, D, D, Wj.pitch("enc.w"), J, bias=jnt.enc.bias)
            w = (Wd["l0.wih"], Wd.pitch("l0.wih"), Wd["l0.whh"], Wd.pitch("l0.whh"), Wj["pred.w"], Wj.pitch("pred.w"), Wj["out.w"],
                 Wj.pitch("out.w"))
        else:
            f = torch.empty(B * T, J, dtype=torch.float32, device=dev)
            ops.gemm(xe32, jnt.enc.weight, f, B * T, J, D, D, D, J, bias=jnt.enc.bias)
            H = dec.pred_hidden
            w = (lstm.weight_ih_l0, H, lstm.weight_hh_l0, H, jnt.pred.weight, H, out.weight, J)
        args = (emb, w[0], w[1], w[2], w[3], lstm.bias_ih_l0, lstm.bias_hh_l0, w[4], w[5], jnt.pred.bias, w[6], w[7], out.bias,
                self._blank_index, self.max_symbols or 0)
        return f.view(B, T, J), args

    def _upper(self, device):
        """layers 1 .. L-1 of the prediction network as the searches' `upper_layers` (None with one layer): the bf16 images and
        their pitches in bf16 compute, else the fp32 masters; the biases are fp32 either way"""
        if self.pred_layers == 1:
            return None
        dec = self.decoder
        lstm, H = dec.prediction["dec_rnn"].lstm, dec.pred_hidden
        cdt = self.joint._cdt()
        Wd = dec._plan(cdt, device)[0] if cdt == torch.bfloat16 else None
        upper = []
        for l in range(1, self.pred_layers):
            b_ih, b_hh = getattr(lstm, f"bias_ih_l{l}"), getattr(lstm, f"bias_hh_l{l}")
            if Wd is not None:
                upper.append((Wd[f"l{l}.wih"], Wd.pitch(f"l{l}.wih"), Wd[f"l{l}.whh"], Wd.pitch(f"l{l}.whh"), b_ih, b_hh))
            else:
                upper.append((getattr(lstm, f"weight_ih_l{l}"), H, getattr(lstm, f"weight_hh_l{l}"), H, b_ih, b_hh))
        return upper

    @property
    def _with_confidence(self) -> bool:
        return self.confidence_cfg is not None and self.confidence_cfg.wants_tokens

    def _method(self, args):
        """the measure's kernel arguments for this decoder's label distribution (V1 = rows of the embedding table)"""
        return self.confidence_cfg.method_cfg.kernel_args(args[0].shape[0])

    @torch.no_grad()
    def decode_ids(self, encoder_output: torch.Tensor, encoded_lengths: torch.Tensor, with_state: bool = False,
                   with_confidence: bool = False):
        """encoder_output [B, D, T] (device) -> (tokens i32 [B, N] -1 padded, frame indices, lengths i32 [B], scores f32 [B]
        [, (h, c)][, tok_conf f32 [B, N] 0.0 padded: with_confidence, needs a `confidence_cfg`])"""
        self._no_fused_confidence(with_confidence)
        f, args = self._project(encoder_output)
        lens = encoded_lengths.to(device=encoder_output.device, dtype=torch.int64).contiguous()
        up = self._upper(f.device)
        if self.fusion_models is not None:
            out = self._search_fused(f, lens, *args, upper_layers=up)
            return out if with_state else out[:4]
        if with_confidence:
            return self._search_conf(f, lens, *args, method=self._method(args), with_state=with_state, upper_layers=up)
        return self._search(f, lens, *args, with_state=with_state, upper_layers=up)

    _search = staticmethod(ops.rnnt_greedy_decode)
    _search_stream = staticmethod(ops.rnnt_greedy_decode_stream)

    def _search_conf(self, *args, method, **kw):
        return ops.rnnt_greedy_decode_conf(*args, method, **kw)

    def _search_stream_conf(self, *args, method, **kw):
        return ops.rnnt_greedy_decode_stream_conf(*args, method, **kw)

    def _search_fused(self, *args, **kw):
        """the search with `fusion_models` -> (tokens, frame indices, lengths, score, (h, c) | the next state)"""
        return ops.transducer_greedy_decode_fused(*args, self.fusion_models, **kw)

    def _no_fused_confidence(self, with_confidence):
        if with_confidence and self.fusion_models is not None:
            raise NotImplementedError("`with_confidence` together with `fusion_models`: the fused search computes no confidences")

    @torch.no_grad()
    def decode_ids_stream(self, encoder_output: torch.Tensor, encoded_lengths: torch.Tensor, state=None, with_confidence: bool = False):
        """one chunk of every stream: encoder_output [B, D, T_chunk], encoded_lengths = this chunk's frames per stream, `state` the
        ops.RNNTStreamState of the previous chunk (None: fresh streams) -> (tokens, GLOBAL frame indices, lengths of this chunk's
        labels, the next state[, tok_conf of this chunk's labels: with_confidence]).  With `fusion_models`: a `FusedChunk`, the
        same four under their names (the state an ops.RNNTFusedStreamState) and `score`, the stream's score so far with the
        models' final terms; `with_confidence` is refused"""
        self._no_fused_confidence(with_confidence)
        f, args = self._project(encoder_output)
        lens = encoded_lengths.to(device=encoder_output.device, dtype=torch.int64).contiguous()
        up = self._upper(f.device)
        if self.fusion_models is not None:
            if state is None:
                state = ops.RNNTFusedStreamState.fresh(f.shape[0], args[0].shape[1], self._blank_index, f.device, layers=self.pred_layers)
            tokens, times, out_len, score, nxt = self._search_fused(f, lens, *args, state=state, upper_layers=up)
            return FusedChunk(tokens, times, out_len, nxt, score)
        if with_confidence:
            return self._search_stream_conf(f, lens, *args, method=self._method(args), state=state, upper_layers=up)
        return self._search_stream(f, lens, *args, state=state, upper_layers=up)

    def fresh_hypotheses(self, batch_size: int, device=None):
        """empty hypotheses of `batch_size` streams that have seen nothing, carrying a fresh decoder state: what a stream's FIRST
        chunk is resumed from (`forward(chunk, lengths, partial_hypotheses=decoder.fresh_hypotheses(B))`)"""
        dec = self.decoder
        device = device if device is not None else dec.prediction["embed"].weight.device
        state_cls = ops.RNNTFusedStreamState if self.fusion_models is not None else ops.RNNTStreamState
        st = state_cls.fresh(batch_size, dec.pred_hidden, self._blank_index, device, layers=self.pred_layers)
        return [Hypothesis(score=0.0, y_sequence=torch.zeros(0, dtype=torch.long), timestamp=[], dec_state=st.select(b), length=0,
                           last_token=st.select(b).last, token_confidence=[] if self._with_confidence else None)
                for b in range(batch_size)]

    def forward(self, encoder_output: torch.Tensor, encoded_lengths: torch.Tensor, partial_hypotheses=None):
        """Without `partial_hypotheses`: the one-shot search of whole utterances, as ever (`dec_state` = the final (h, c)).
        With them (a list of hypotheses this decoder returned for earlier chunks, or `fresh_hypotheses(B)` for the first chunk):
        the resumable search; the returned hypotheses cover the whole stream so far and carry the next decoder state."""
        B = encoder_output.shape[0]
        conf = self._with_confidence
        if partial_hypotheses is None:
            tokens, times, out_len, score, (h, c), *tc = self.decode_ids(encoder_output, encoded_lengths, with_state=True,
                                                                         with_confidence=conf)
            tokens, times, out_len, score = tokens.cpu(), times.cpu(), out_len.cpu(), score.cpu()   # the only D2H copies
            tc = tc[0].cpu() if conf else None
            hyps = []
            for b in range(B):
                n = int(out_len[b])
                hyps.append(Hypothesis(score=float(score[b]), y_sequence=tokens[b, :n].to(torch.long), timestamp=times[b, :n].tolist(),
                                       dec_state=(h[b], c[b]) if h.dim() == 2 else (h[:, b], c[:, b]), length=int(encoded_lengths[b]),
                                       token_confidence=tc[b, :n].tolist() if conf else None))
            return (hyps,)
        if len(partial_hypotheses) != B:
            raise ValueError(f"{len(partial_hypotheses)} partial hypotheses for a batch of {B}")
        if any(h is None or not isinstance(h.dec_state, ops.RNNTStreamState) for h in partial_hypotheses):
            raise ValueError("`partial_hypotheses` must carry a stream state in `dec_state`: hypotheses this decoder returned for "
                             "earlier chunks, or `fresh_hypotheses(batch_size)` for the first chunk of a stream")
        fused = self.fusion_models is not None
        if fused and any(not isinstance(h.dec_state, ops.RNNTFusedStreamState) for h in partial_hypotheses):
            raise ValueError("`partial_hypotheses` of a decoder with `fusion_models` must carry the fused stream state: hypotheses "
                             "this decoder returned for earlier chunks, or `fresh_hypotheses(batch_size)`")
        state = (ops.RNNTFusedStreamState if fused else ops.RNNTStreamState).stack([h.dec_state for h in partial_hypotheses])
        if fused:   # the kernel's `score` output carries the models' final terms; the state keeps the running score
            chunk = self.decode_ids_stream(encoder_output, encoded_lengths, state)
            tokens, times, out_len, nxt, score, tc = chunk.tokens, chunk.frames, chunk.lengths, chunk.state, chunk.score, ()
        else:
            tokens, times, out_len, nxt, *tc = self.decode_ids_stream(encoder_output, encoded_lengths, state, with_confidence=conf)
            score = nxt.score
        tokens, times, out_len, score = tokens.cpu(), times.cpu(), out_len.cpu(), score.cpu()   # the only D2H copies
        tc = tc[0].cpu() if conf else None
        lens = encoded_lengths.cpu()
        hyps = []
        for b in range(B):   # the whole stream so far, in new objects: the inputs stay as they are
            n = int(out_len[b])
            prev = partial_hypotheses[b]
            y = torch.cat((prev.y_sequence.to(torch.long).cpu(), tokens[b, :n].to(torch.long)))
            st = nxt.select(b)
            hyps.append(Hypothesis(score=float(score[b]), y_sequence=y, timestamp=list(prev.timestamp) + times[b, :n].tolist(),
                                   dec_state=st, length=int(prev.length) + int(lens[b]), last_token=st.last,
                                   token_confidence=list(prev.token_confidence or []) + tc[b, :n].tolist() if conf else None))
        return (hyps,)

    __call__ = forward


class GreedyBatchedTDTInfer(GreedyBatchedRNNTInfer):
    """`GreedyBatchedTDTInfer` (parts/submodules/tdt_loop_labels_computer.py and rnnt_greedy_decoding.py): greedy search of a
    Token-and-Duration Transducer, whose joint appends one logit per duration behind the V+1 label logits.  Per utterance the
    label is the arg-max of the label logits, the duration the arg-max of the duration logits; a blank moves on by
    max(duration, 1) frames, a label by its duration, and the `max_symbols`-th consecutive label of duration 0 by one frame.
    One launch for the batch (`mi355x_transducer_greedy_decode` with the duration set; streaming: a duration that jumps past the end
    of a chunk is taken off the next one)."""

    def __init__(self, decoder_model, joint_model, blank_index: int, durations, max_symbols_per_step: Optional[int] = None,
                 **kw):
        super().__init__(decoder_model, joint_model, blank_index, max_symbols_per_step=max_symbols_per_step, **kw)
        from .tdt_loss import check_durations
        self.durations = check_durations(list(durations))
        if getattr(joint_model, "_num_extra_outputs", len(self.durations)) != len(self.durations):
            raise ValueError(f"the joint has {joint_model._num_extra_outputs} extra outputs for {len(self.durations)} durations")

    def _search_fused(self, *args, **kw):
        return ops.transducer_greedy_decode_fused(*args, self.fusion_models, durations=self.durations, **kw)

    def _search(self, *args, **kw):
        return ops.tdt_greedy_decode(*args[:16], self.durations, args[16], **kw)

    def _search_stream(self, *args, **kw):
        return ops.tdt_greedy_decode_stream(*args[:16], self.durations, args[16], **kw)

    def _search_conf(self, *args, method, **kw):
        return ops.tdt_greedy_decode_conf(*args[:16], self.durations, args[16], method, **kw)

    def _search_stream_conf(self, *args, method, **kw):
        return ops.tdt_greedy_decode_stream_conf(*args[:16], self.durations, args[16], method, **kw)


def transducer_fusion_from_config(greedy, vocabulary=None, text_to_ids=None, what: str = "transducer"):
    """The fusion models of a transducer head's `decoding.greedy` sub-section, read by the CTC head's readers (modules/
    ctc_decoding.py) under the section name `greedy`: ngram_lm_arpa, ngram_lm_alpha, ngram_lm_token_offset, boosting_tree
    {key_phrases_list, key_phrases_file, context_score, depth_scaling}, boosting_tree_alpha, with the same refusals
    (`ngram_lm_model` / `kenlm_path` by name, a weight without a model, a missing file, a phrase that tokenises to nothing, the
    three tree keys that are not provided).  `vocabulary`: the labels, in id order (None: the section is only checked);
    `text_to_ids` tokenises the phrases.  -> [(NGramLM, alpha)][(BoostingTree, alpha)], the LM first, or None without the keys."""
    from .ctc_decoding import _boosting_tree_from_config, _ngram_lm_from_config
    greedy = dict(greedy or {})
    alpha = float(greedy.get("ngram_lm_alpha") or 0.0)
    if alpha < 0:
        raise ValueError(f"{what} decoding: `greedy.ngram_lm_alpha` must be >= 0; got {alpha}")
    lm = _ngram_lm_from_config(greedy, vocabulary, what, sec="greedy")
    tree, tree_alpha = _boosting_tree_from_config(greedy, vocabulary, what, text_to_ids, sec="greedy")
    models = ([(lm, alpha)] if lm is not None else []) + ([(tree, tree_alpha)] if tree is not None else [])
    return models or None


class RNNTDecoding:
    """`strategy: greedy_batch` of AbstractRNNTDecoding (rnnt_decoding.py:216-330) for a character / word-piece vocabulary;
    blank id = len(vocabulary) (rnnt_decoding.py:1170).  `fusion_models` (None: the search without models): what
    `transducer_fusion_from_config` reads from `decoding.greedy`."""

    def __init__(self, decoder, joint, vocabulary: Optional[Sequence[str]] = None, max_symbols: Optional[int] = 10,
                 tokenizer=None, model_type: str = "rnnt", durations: Optional[Sequence[int]] = None, confidence_cfg=None,
                 fusion_models=None):
        from .confidence import confidence_from
        self.vocabulary = list(vocabulary) if vocabulary is not None else None
        self.tokenizer = tokenizer
        self.blank_id = decoder.blank_idx
        self.confidence_cfg = confidence_from(confidence_cfg)
        if model_type == "tdt":   # rnnt_decoding.py: `model_type: tdt` with the duration set of the joint's extra outputs
            if not durations:
                raise ValueError("decoding with model_type 'tdt' needs `durations`")
            self.decoding = GreedyBatchedTDTInfer(decoder, joint, self.blank_id, durations, max_symbols_per_step=max_symbols,
                                                  confidence_cfg=self.confidence_cfg, fusion_models=fusion_models)
        elif model_type == "rnnt":
            self.decoding = GreedyBatchedRNNTInfer(decoder, joint, self.blank_id, max_symbols_per_step=max_symbols,
                                                   confidence_cfg=self.confidence_cfg, fusion_models=fusion_models)
        else:
            raise NotImplementedError(f"transducer decoding model_type '{model_type}' (implemented: rnnt, tdt)")

    def ids_to_text(self, ids: Sequence[int]) -> str:
        ids = [int(i) for i in ids if int(i) != self.blank_id]
        if self.tokenizer is not None:
            return self.tokenizer.ids_to_text(ids)
        if self.vocabulary is None:
            raise ValueError("no vocabulary: text is not available")
        text = "".join(self.vocabulary[i] for i in ids)
        return text.replace("▁", " ").strip() if "▁" in text else text

    def rnnt_decoder_predictions_tensor(self, encoder_output: torch.Tensor, encoded_lengths: torch.Tensor,
                                        return_hypotheses: bool = False, partial_hypotheses=None):
        hyps = self.decoding(encoder_output=encoder_output, encoded_lengths=encoded_lengths,
                             partial_hypotheses=partial_hypotheses)[0]
        words = self.confidence_cfg is not None and self.confidence_cfg.preserve_word_confidence
        for h in hyps:
            h.text = self.ids_to_text(h.y_sequence.tolist())
            if words:
                h.word_confidence = self.word_confidence(h.y_sequence.tolist(), h.token_confidence)
        return hyps

    def ids_to_tokens(self, ids: Sequence[int]) -> List[str]:
        ids = [int(i) for i in ids]
        if self.tokenizer is not None:
            return list(self.tokenizer.ids_to_tokens(ids))
        if self.vocabulary is None:
            raise ValueError("no vocabulary: tokens are not available")
        return [self.vocabulary[i] for i in ids]

    def word_confidence(self, ids: Sequence[int], token_conf: Sequence[float]) -> List[float]:
        """the configured aggregation of the token confidences over every word (the grouping of `ctc_offsets`)"""
        from .confidence import word_confidence
        toks = self.ids_to_tokens(ids)
        pieces = any(t.startswith("▁") for t in (self.vocabulary if self.vocabulary is not None else toks))
        return word_confidence(toks, token_conf, pieces, self.confidence_cfg.aggregation)


class RNNTWER:
    """metrics/wer.py:210-356 with a transducer decoding object: `predictions` = the ENCODER output [B, D, T]"""

    def __init__(self, decoding: RNNTDecoding, use_cer: bool = False):
        self.decoding, self.use_cer = decoding, use_cer
        self.scores = 0
        self.words = 0
        self._to_sync = True

    def update(self, predictions: torch.Tensor, predictions_lengths, targets: torch.Tensor, targets_lengths):
        hyps = [h.text for h in self.decoding.rnnt_decoder_predictions_tensor(predictions, predictions_lengths)]
        tg, tl = targets.cpu(), targets_lengths.cpu()
        refs = [self.decoding.ids_to_text(tg[b, : int(tl[b])].tolist()) for b in range(tg.shape[0])]
        for h, r in zip(hyps, refs):
            h_list, r_list = (list(h), list(r)) if self.use_cer else (h.split(), r.split())
            self.words += len(r_list)
            self.scores += _levenshtein(h_list, r_list)

    def compute(self):
        wer = self.scores / self.words if self.words else float("inf")
        return wer, self.scores, self.words

    def reset(self):
        self.scores = self.words = 0
