"""Greedy CTC decoding and WER for the drop-in model.

The reference decodes on the host: `GreedyCTCInfer` copies the log-probabilities to the CPU utterance by utterance and
folds them in Python (parts/submodules/ctc_greedy_decoding.py:333-361, ctc_decoding.py:545-575), a D2H sync of
[B, T, V+1] floats (8 MB at the headline shape) on every logging step.  Here arg-max, score, repeat folding and blank
removal are one kernel launch (`mi355x_ctc_greedy_decode`); only the folded token ids (<= 64 KB) ever leave the device,
and only when text is asked for.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from .. import ops


class GreedyCTCDecoder:
    """blank_id = len(vocabulary) as in CTCDecoding.__init__ (ctc_decoding.py:1044); `vocabulary` maps ids to strings
    (characters, or word pieces whose leading U+2581 marks a word start -- the SentencePiece convention)."""

    def __init__(self, vocabulary: Optional[Sequence[str]] = None, blank_id: Optional[int] = None, confidence_cfg=None):
        if vocabulary is None and blank_id is None:
            raise ValueError("either a vocabulary or a blank_id is required")
        self.vocabulary = list(vocabulary) if vocabulary is not None else None
        self.blank_id = len(self.vocabulary) if blank_id is None else int(blank_id)
        from .confidence import confidence_from
        self.confidence_cfg = confidence_from(confidence_cfg)   # None: no confidence is computed, decoding is what it was

    @property
    def word_pieces(self) -> bool:
        return self.vocabulary is not None and any(v.startswith("▁") for v in self.vocabulary)

    @torch.no_grad()
    def decode_ids(self, log_probs: torch.Tensor, lengths: Optional[torch.Tensor] = None, return_timestamps: bool = False):
        """log_probs [B, T, V+1] (device) -> (tokens i32 [B,T] folded / blank-free / -1 padded, lengths i32 [B], score [B]);
        with return_timestamps also (start, end) i32 [B,T]: the first / last frame of the run of equal arg-max labels behind each
        token (`mi355x_ctc_greedy_decode_ts`; the `compute_timestamps` of AbstractCTCDecoding, ctc_decoding.py:290-340)"""
        if log_probs.dim() != 3:
            raise ValueError(f"`decoder_output` must be a tensor of shape [B, T, V] (log probs, float). Provided shape = "
                             f"{tuple(log_probs.shape)}")
        lp = log_probs.to(torch.float32).contiguous()
        lens = lengths.to(torch.int64).contiguous() if lengths is not None else None
        if return_timestamps:
            return ops.ctc_greedy_decode_ts(lp, lens, self.blank_id)
        return ops.ctc_greedy_decode(lp, lens, self.blank_id)

    @torch.no_grad()
    def decode_ids_confidence(self, log_probs: torch.Tensor, lengths: Optional[torch.Tensor] = None):
        """`decode_ids(..., return_timestamps=True)` with confidences (needs a `confidence_cfg`): its tuple plus (frame_conf f32
        [B,T], tok_conf f32 [B,T]), 0.0 padded -- the configured measure of every frame and its aggregation over each token's
        frames, from the same launch (`mi355x_ctc_greedy_decode_conf`)"""
        cfg = self.confidence_cfg
        if cfg is None:
            raise ValueError("confidence needs a decoder built with a `confidence_cfg` that preserves a confidence")
        if log_probs.dim() != 3:
            raise ValueError(f"`decoder_output` must be a tensor of shape [B, T, V] (log probs, float). Provided shape = "
                             f"{tuple(log_probs.shape)}")
        from .confidence import AGGREGATIONS
        lp = log_probs.to(torch.float32).contiguous()
        lens = lengths.to(torch.int64).contiguous() if lengths is not None else None
        return ops.ctc_greedy_decode_conf(lp, lens, self.blank_id, cfg.method_cfg.kernel_args(lp.shape[2]),
                                          AGGREGATIONS[cfg.aggregation], cfg.exclude_blank)

    def offsets(self, ids: Sequence[int], starts: Sequence[int], ends: Sequence[int]):
        """(char offsets, word offsets) of a token sequence with its first / last frames, see `ctc_offsets`"""
        if self.vocabulary is None:
            raise ValueError("no vocabulary: offsets are not available")
        return ctc_offsets([self.vocabulary[i] for i in ids], starts, ends, word_pieces=self.word_pieces)

    def word_confidence(self, ids: Sequence[int], token_conf: Sequence[float]):
        """one confidence per word of `offsets(ids, ...)`: the configured aggregation over the word's token confidences"""
        if self.vocabulary is None or self.confidence_cfg is None:
            raise ValueError("word confidence needs a vocabulary and a `confidence_cfg`")
        from .confidence import word_confidence
        return word_confidence([self.vocabulary[i] for i in ids], token_conf, self.word_pieces, self.confidence_cfg.aggregation)

    def ids_to_text(self, ids: Sequence[int]) -> str:
        if self.vocabulary is None:
            raise ValueError("no vocabulary: text is not available")
        text = "".join(self.vocabulary[i] for i in ids)             # decode_tokens_to_str, ctc_decoding.py:1075-1086
        return text.replace("▁", " ").strip() if "▁" in text else text

    def __call__(self, log_probs, lengths=None) -> List[str]:
        tokens, out_len, _ = self.decode_ids(log_probs, lengths)
        tokens, out_len = tokens.cpu(), out_len.cpu()                  # the only D2H copy: folded ids
        return [self.ids_to_text(tokens[b, : int(out_len[b])].tolist()) for b in range(tokens.shape[0])]


def ctc_offsets(tokens: Sequence[str], starts: Sequence[int], ends: Sequence[int], word_pieces: bool = False):
    """The offsets of AbstractCTCDecoding (`_compute_offsets`, `_get_word_offsets_chars` / `_get_word_offsets_subwords_sentencepiece`,
    ctc_decoding.py:620-800), built on the host from tokens and their first / last frames; `end_offset` is exclusive (last frame + 1).
    -> (char: one {char, start_offset, end_offset} per token, word: {word, start_offset, end_offset}).  Word pieces: a token with a
    leading U+2581 starts a word.  Characters: the space token separates words and belongs to none.  A word spans its first token's
    start to its last token's end."""
    char = [{"char": tok, "start_offset": int(s), "end_offset": int(e) + 1} for tok, s, e in zip(tokens, starts, ends)]
    words, cur = [], None
    for c in char:
        tok = c["char"]
        if word_pieces:
            if tok.startswith("▁") or cur is None:
                cur = {"word": "", "start_offset": c["start_offset"], "end_offset": c["end_offset"]}
                words.append(cur)
            cur["word"] += tok.replace("▁", "")
            cur["end_offset"] = c["end_offset"]
        elif tok == " ":
            cur = None
        else:
            if cur is None:
                cur = {"word": "", "start_offset": c["start_offset"], "end_offset": c["end_offset"]}
                words.append(cur)
            cur["word"] += tok
            cur["end_offset"] = c["end_offset"]
    return char, [w for w in words if w["word"]]


class CTCAligner:
    """Forced alignment of known token ids to log-probabilities: the Viterbi pass of the reference's forced aligner
    (tools/nemo_forced_aligner/utils/viterbi_decoding.py, a Python loop over T) as one launch per batch (`mi355x_ctc_align`).
    blank_id = len(vocabulary), as in GreedyCTCDecoder."""

    def __init__(self, vocabulary: Optional[Sequence[str]] = None, blank_id: Optional[int] = None):
        if vocabulary is None and blank_id is None:
            raise ValueError("either a vocabulary or a blank_id is required")
        self.vocabulary = list(vocabulary) if vocabulary is not None else None
        self.blank_id = len(self.vocabulary) if blank_id is None else int(blank_id)

    @torch.no_grad()
    def __call__(self, log_probs: torch.Tensor, lengths: torch.Tensor, targets: torch.Tensor, target_lengths: torch.Tensor):
        """log_probs [B, T, V+1], lengths [B], targets [B, U], target_lengths [B] (device) -> (path i32 [B,T]: state 0..2U of the
        blank-extended transcript per frame, tok_start i32 [B,U], tok_end i32 [B,U], score f32 [B]); -1 padded; an utterance
        that cannot be aligned has score -inf and -1 everywhere"""
        if log_probs.dim() != 3:
            raise ValueError(f"`log_probs` must be a tensor of shape [B, T, V]. Provided shape = {tuple(log_probs.shape)}")
        return ops.ctc_align(log_probs.to(torch.float32).contiguous(), targets.to(torch.int64).contiguous(),
                             lengths.to(torch.int64).contiguous(), target_lengths.to(torch.int64).contiguous(), self.blank_id)


def _levenshtein(a, b) -> int:
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def word_error_rate(hypotheses: List[str], references: List[str], use_cer: bool = False) -> float:
    """nemo/collections/asr/metrics/wer.py:35-73"""
    if len(hypotheses) != len(references):
        raise ValueError("In word error rate calculation, hypotheses and reference lists must have the same number of "
                         "elements. But I got:{0} and {1} correspondingly".format(len(hypotheses), len(references)))
    scores = words = 0
    for h, r in zip(hypotheses, references):
        h_list, r_list = (list(h), list(r)) if use_cer else (h.split(), r.split())
        words += len(r_list)
        scores += _levenshtein(h_list, r_list)
    return 1.0 * scores / words if words != 0 else float("inf")


class WER:
    """metrics/wer.py:210-356: accumulates edit distance and reference word counts over batches; `compute()` returns
    (wer, scores, words) like the torchmetrics object of the reference."""

    def __init__(self, decoding: GreedyCTCDecoder, use_cer: bool = False):
        self.decoding, self.use_cer = decoding, use_cer
        self.scores = 0
        self.words = 0

    def update(self, predictions: torch.Tensor, predictions_lengths, targets: torch.Tensor, targets_lengths):
        hyps = self.decoding(predictions, predictions_lengths)
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
