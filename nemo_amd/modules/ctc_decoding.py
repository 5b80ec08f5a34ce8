"""Greedy CTC decoding, CTC prefix beam search and WER for the drop-in model.

The reference decodes on the host: `GreedyCTCInfer` copies the log-probabilities to the CPU utterance by utterance and
folds them in Python (parts/submodules/ctc_greedy_decoding.py:333-361, ctc_decoding.py:545-575), a D2H sync of
[B, T, V+1] floats (8 MB at the headline shape) on every logging step.  Here arg-max, score, repeat folding and blank
removal are one kernel launch (`mi355x_ctc_greedy_decode`); only the folded token ids (<= 64 KB) ever leave the device,
and only when text is asked for.

`BeamBatchedCTCDecoder` is the reference's `strategy: beam_batch` (its batched GPU CTC beam search; `beam` there is the pyctcdecode /
KenLM decoder and stays refused here), with or without shallow fusion of a token-level n-gram language model (`NGramLM`, read from
an ARPA file: `beam.ngram_lm_arpa`, `beam.ngram_lm_alpha`; the reference's NGramGPULanguageModel).  What it runs is the classic CTC
prefix beam search as include/mi355x_asr.h states it in full -- that statement, not a recollection of the reference's internals,
is what the kernel and the test oracles (tests/ctc_beam_oracle.py, tests/ctc_beam_lm_oracle.py) implement: pb / pnb per prefix,
stays and extensions merged where they name the same prefix, the `beam_size` prefixes of the largest log-probability (+ beam_beta
per token, + ngram_lm_alpha * the LM's log-probability of the prefix) kept per frame, one launch per batch.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence

import torch

from .. import ops


class _CTCText:
    """what every CTC decoding object knows about its labels: blank_id = len(vocabulary) as in CTCDecoding.__init__
    (ctc_decoding.py:1044); `vocabulary` maps ids to strings (characters, or word pieces whose leading U+2581 marks a word start --
    the SentencePiece convention)."""

    def _set_labels(self, vocabulary, blank_id):
        if vocabulary is None and blank_id is None:
            raise ValueError("either a vocabulary or a blank_id is required")
        self.vocabulary = list(vocabulary) if vocabulary is not None else None
        self.blank_id = len(self.vocabulary) if blank_id is None else int(blank_id)

    @property
    def word_pieces(self) -> bool:
        return self.vocabulary is not None and any(v.startswith("▁") for v in self.vocabulary)

    def offsets(self, ids: Sequence[int], starts: Sequence[int], ends: Sequence[int]):
        """(char offsets, word offsets) of a token sequence with its first / last frames, see `ctc_offsets`"""
        if self.vocabulary is None:
            raise ValueError("no vocabulary: offsets are not available")
        return ctc_offsets([self.vocabulary[i] for i in ids], starts, ends, word_pieces=self.word_pieces)

    def ids_to_text(self, ids: Sequence[int]) -> str:
        if self.vocabulary is None:
            raise ValueError("no vocabulary: text is not available")
        text = "".join(self.vocabulary[i] for i in ids)             # decode_tokens_to_str, ctc_decoding.py:1075-1086
        return text.replace("▁", " ").strip() if "▁" in text else text


def _check_log_probs(log_probs):
    if log_probs.dim() != 3:
        raise ValueError(f"`decoder_output` must be a tensor of shape [B, T, V] (log probs, float). Provided shape = "
                         f"{tuple(log_probs.shape)}")


class GreedyCTCDecoder(_CTCText):
    """blank_id = len(vocabulary) as in CTCDecoding.__init__ (ctc_decoding.py:1044); `vocabulary` maps ids to strings
    (characters, or word pieces whose leading U+2581 marks a word start -- the SentencePiece convention)."""

    def __init__(self, vocabulary: Optional[Sequence[str]] = None, blank_id: Optional[int] = None, confidence_cfg=None):
        self._set_labels(vocabulary, blank_id)
        from .confidence import confidence_from
        self.confidence_cfg = confidence_from(confidence_cfg)   # None: no confidence is computed, decoding is what it was

    @torch.no_grad()
    def decode_ids(self, log_probs: torch.Tensor, lengths: Optional[torch.Tensor] = None, return_timestamps: bool = False):
        """log_probs [B, T, V+1] (device) -> (tokens i32 [B,T] folded / blank-free / -1 padded, lengths i32 [B], score [B]);
        with return_timestamps also (start, end) i32 [B,T]: the first / last frame of the run of equal arg-max labels behind each
        token (`mi355x_ctc_greedy_decode_ts`; the `compute_timestamps` of AbstractCTCDecoding, ctc_decoding.py:290-340)"""
        _check_log_probs(log_probs)
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
        _check_log_probs(log_probs)
        from .confidence import AGGREGATIONS
        lp = log_probs.to(torch.float32).contiguous()
        lens = lengths.to(torch.int64).contiguous() if lengths is not None else None
        return ops.ctc_greedy_decode_conf(lp, lens, self.blank_id, cfg.method_cfg.kernel_args(lp.shape[2]),
                                          AGGREGATIONS[cfg.aggregation], cfg.exclude_blank)

    def word_confidence(self, ids: Sequence[int], token_conf: Sequence[float]):
        """one confidence per word of `offsets(ids, ...)`: the configured aggregation over the word's token confidences"""
        if self.vocabulary is None or self.confidence_cfg is None:
            raise ValueError("word confidence needs a vocabulary and a `confidence_cfg`")
        from .confidence import word_confidence
        return word_confidence([self.vocabulary[i] for i in ids], token_conf, self.word_pieces, self.confidence_cfg.aggregation)

    def __call__(self, log_probs, lengths=None) -> List[str]:
        tokens, out_len, _ = self.decode_ids(log_probs, lengths)
        tokens, out_len = tokens.cpu(), out_len.cpu()                  # the only D2H copy: folded ids
        return [self.ids_to_text(tokens[b, : int(out_len[b])].tolist()) for b in range(tokens.shape[0])]


class CTCBeamStreamState:
    """The beam search of a batch of B streams between two chunks (`mi355x_ctc_beam_stream_state`, include/mi355x_asr.h): the beams
    of every stream, the prefix tree they point into, and the buffers the n-best is written to.
      h64    i64 [2, B, W]   h, hp: the hashes of each beam's prefix and of its parent's prefix
      beams  i32 [10, B, W]  node, par, tok, len, lm_state, then (float32 bits) pb, pnb, tot, brank, lm_sum; `arrays()` names them
      utt    i32 [2, B]      nb (live beams), frames_done
      tree   i32 [B, Tcap, W, 2]   (parent node, token) of node 1 + frame * W + slot; append-only, SHARED by the states of a stream
      tokens, tok_frame  i32 [B, W, Tcap]   the n-best of the last emitting step, valid up to hyp_len; allocated once, reused by
                             every step (copy what has to outlive the next one)
    `lm`: the state of an LM-fused search (lm_state / lm_sum are meaningful).  `bound`: an upper bound of the frames consumed -- the
    sum of the T of the steps taken, kept on the host, so that capacity never needs a device read.
    A step never writes the beam arrays of the state it starts from; it appends to the tree.  Stepping one state twice with the
    same chunk rewrites the same nodes with the same values; two DIFFERENT continuations of one state need a `gather` copy each.
    A COMMITTED state (`ops.ctc_beam_commit`, `mi355x_ctc_beam_window`) also carries
      win        i32 [4, B]       tok_base, frame_base, kept of the window, and the token count of the last commit
      frame_map  i32 [B, Tcap]    the global frame of the first `kept` tree frames
      committed  per stream (token ids, global frames): the tokens taken out of the tree so far, on the host
    (`win` is None for a state that was never committed; its window is all zero).  Its tree is its own, re-rooted and compacted;
    its `bound` is the largest `kept` of its streams, so its capacity follows the window, not the stream's length, and the n-best
    buffers hold the TAIL of each hypothesis behind the committed tokens."""
    INT_FIELDS, FLOAT_FIELDS = ("node", "par", "tok", "len", "lm_state"), ("pb", "pnb", "tot", "brank", "lm_sum")
    ROOT_HASH = 0x243F6A8885A308D3
    MAX_NODES = 0x3FFFFFFF   # capacity * W: node ids are 32-bit

    def __init__(self, h64, beams, utt, tree, tokens, tok_frame, lm, bound, fs=None, win=None, frame_map=None, committed=None,
                 steps=0):
        self.h64, self.beams, self.utt, self.tree, self.tokens, self.tok_frame = h64, beams, utt, tree, tokens, tok_frame
        self.fs = fs   # i32 [2, B, W] or None: fs_state, fs_sum (float32 bits) of a search with a SECOND fusion model
        self.B, self.W, self.lm, self.bound = int(beams.shape[1]), int(beams.shape[2]), bool(lm), int(bound)
        self.win, self.frame_map = win, frame_map
        self.committed = list(committed) if committed is not None else [((), ())] * self.B
        self.steps = int(steps)   # the steps taken so far (host): what `stream_commit_every` counts

    @property
    def n_models(self) -> int:
        return int(self.lm) + (self.fs is not None)

    def window_arrays(self):
        """name -> the arrays of `mi355x_ctc_beam_window`; of a state that was never committed new all-zero ones (the state is left
        as it is)"""
        win, frame_map = self.win, self.frame_map
        if win is None:
            i32 = dict(dtype=torch.int32, device=self.device)
            win, frame_map = torch.zeros(4, self.B, **i32), torch.zeros(self.B, self.capacity, **i32)
        return dict(tok_base=win[0], frame_base=win[1], kept=win[2], frame_map=frame_map)

    @property
    def capacity(self) -> int:
        return int(self.tree.shape[1])

    @property
    def device(self):
        return self.beams.device

    @classmethod
    def _check_capacity(cls, capacity, W):
        if capacity < 1 or capacity * W > cls.MAX_NODES:
            raise ValueError(f"CTC beam stream state: capacity {capacity} frames x {W} beams is outside 1..{cls.MAX_NODES} nodes "
                             "(node ids are 32-bit)")

    @staticmethod
    def _buffers(B, W, capacity, device):
        i32 = dict(dtype=torch.int32, device=device)
        return torch.zeros(B, capacity, W, 2, **i32), torch.empty(B, W, capacity, **i32), torch.empty(B, W, capacity, **i32)

    @classmethod
    def fresh(cls, B, W, device, capacity: int = 64, lm: bool = False, second: bool = False):
        """B streams that have seen nothing, with room for `capacity` frames (it grows by doubling: `reserve`); `second`: with the
        per-beam arrays of a second fusion model (`mi355x_ctc_beam_fused_state`)"""
        B, W, capacity = int(B), int(W), int(capacity)
        if B < 1 or not 1 <= W <= 64:
            raise ValueError(f"CTC beam stream state: B = {B}, W = {W} (B >= 1, 1 <= W <= 64)")
        cls._check_capacity(capacity, W)
        h64 = torch.zeros(2, B, W, dtype=torch.int64, device=device)
        h64[0] = cls.ROOT_HASH
        ints = torch.tensor([0, -1, -1, 0, 1], dtype=torch.int32, device=device)
        flts = torch.tensor([float("-inf")] * 4 + [0.0], dtype=torch.float32, device=device)
        beams = torch.cat((ints, flts.view(torch.int32))).view(10, 1, 1).repeat(1, B, W)
        beams[5:9:2, :, 0] = 0   # slot 0, the empty prefix: pb = tot = 0
        beams[8, :, 0] = 0       # and its rank
        utt = torch.zeros(2, B, dtype=torch.int32, device=device)
        utt[0] = 1
        fs = None
        if second:
            fs = torch.zeros(2, B, W, dtype=torch.int32, device=device)
            fs[0] = 1
        return cls(h64, beams, utt, *cls._buffers(B, W, capacity, device), lm=lm, bound=0, fs=fs)

    def arrays(self):
        """name -> [B, W] (nb, frames_done: [B]) views of the arrays the search carries (lm_state / lm_sum only for an LM search)"""
        out = {"h": self.h64[0], "hp": self.h64[1]}
        out.update({n: self.beams[i] for i, n in enumerate(self.INT_FIELDS)})
        out.update({n: self.beams[5 + i].view(torch.float32) for i, n in enumerate(self.FLOAT_FIELDS)})
        if not self.lm:
            del out["lm_state"], out["lm_sum"]
        out.update(nb=self.utt[0], frames_done=self.utt[1])
        if self.fs is not None:
            out.update(fs_state=self.fs[0], fs_sum=self.fs[1].view(torch.float32))
        return out

    def reserve(self, T: int):
        """room for T more frames: while bound + T exceeds the capacity it doubles -- a new tree with the frames of the old one
        copied in (node ids do not depend on the capacity) and new output buffers"""
        need, cap = self.bound + int(T), self.capacity
        if need <= cap:
            return self
        while cap < need:
            cap *= 2
        cap = max(need, min(cap, self.MAX_NODES // self.W))   # (the last doubling stops at what node ids can name)
        self._check_capacity(cap, self.W)
        old = self.tree
        self.tree, self.tokens, self.tok_frame = self._buffers(self.B, self.W, cap, self.device)
        self.tree[:, : old.shape[1]] = old
        if self.frame_map is not None:
            old, self.frame_map = self.frame_map, torch.zeros(self.B, cap, dtype=torch.int32, device=self.device)
            self.frame_map[:, : old.shape[1]] = old
        return self

    def next(self, T: int):
        """the state a step over T frames writes: new beam arrays (uninitialised), this state's tree and buffers"""
        return CTCBeamStreamState(torch.empty_like(self.h64), torch.empty_like(self.beams), torch.empty_like(self.utt), self.tree,
                                  self.tokens, self.tok_frame, self.lm, self.bound + int(T),
                                  fs=None if self.fs is None else torch.empty_like(self.fs), win=self.win, frame_map=self.frame_map,
                                  committed=self.committed, steps=self.steps + 1)

    @classmethod
    def gather(cls, pairs):
        """a new state of len(pairs) streams: row i is stream `row` of `state` for the i-th (state, row) -- for a server that drops
        finished streams or regroups them.  Beams, trees and windows are copied; the new state shares nothing with the old ones.
        Committed and uncommitted streams mix: an uncommitted stream has the all-zero window."""
        pairs = list(pairs)
        if not pairs:
            raise ValueError("CTC beam stream state: gather of no streams")
        first = pairs[0][0]
        for s, r in pairs:
            if s.W != first.W or s.lm != first.lm or s.device != first.device or (s.fs is None) != (first.fs is None):
                raise ValueError("CTC beam stream state: gather over states of different beam width, LM-ness or device")
            if not 0 <= int(r) < s.B:
                raise ValueError(f"CTC beam stream state: row {r} of a state of {s.B} streams")
        cap = max(s.capacity for s, _ in pairs)
        tree, tokens, tok_frame = cls._buffers(len(pairs), first.W, cap, first.device)
        for i, (s, r) in enumerate(pairs):
            tree[i, : s.capacity] = s.tree[int(r)]
        pick = lambda name: torch.stack([getattr(s, name)[:, int(r)] for s, r in pairs], dim=1).contiguous()
        win = frame_map = None
        if any(s.win is not None for s, _ in pairs):
            i32 = dict(dtype=torch.int32, device=first.device)
            win, frame_map = torch.zeros(4, len(pairs), **i32), torch.zeros(len(pairs), cap, **i32)
            for i, (s, r) in enumerate(pairs):
                if s.win is not None:
                    win[:, i], frame_map[i, : s.capacity] = s.win[:, int(r)], s.frame_map[int(r)]
        return cls(pick("h64"), pick("beams"), pick("utt"), tree, tokens, tok_frame, first.lm, max(s.bound for s, _ in pairs),
                   fs=None if first.fs is None else pick("fs"), win=win, frame_map=frame_map,
                   committed=[s.committed[int(r)] for s, r in pairs], steps=max(s.steps for s, _ in pairs))


def _stream_commit_keys(every, stable, what="BeamBatchedCTCDecoder"):
    """`stream_commit_every` (chunks, >= 1, or None) and `stream_stable_frames` (frames, >= 0, or None; only with the former)"""
    every = None if every is None else int(every)
    stable = None if stable is None else int(stable)
    if every is not None and every < 1:
        raise ValueError(f"{what}: `stream_commit_every` must be None or >= 1 chunks; got {every}")
    if stable is not None and stable < 0:
        raise ValueError(f"{what}: `stream_stable_frames` must be None or >= 0 frames; got {stable}")
    if stable is not None and every is None:
        raise ValueError(f"{what}: `stream_stable_frames` without `stream_commit_every` (nothing would ever be committed)")
    return every, stable


class BeamBatchedCTCDecoder(_CTCText):
    """CTC prefix beam search on the device (`mi355x_ctc_beam_decode`, with `ngram_lm` `mi355x_ctc_beam_decode_fused`): the `beam_batch`
    strategy.  `beam_size` hypotheses per utterance (1..64), `beam_threshold`: a class is looked at in a frame only if its
    log-probability is within that much of the frame's best (inf: every class), `beam_beta`: bonus per token, `ngram_lm`: an `NGramLM`
    over the labels, fused with weight `ngram_lm_alpha` >= 0; the score of a hypothesis is the log-probability of its LABEL SEQUENCE
    (all of its alignments the search kept) + beam_beta * length + ngram_lm_alpha * the LM's log-probability of the sequence.
    `return_best_hypothesis=False` makes `__call__` return the n-best lists.
    `boosting_tree`: a `BoostingTree` of key phrases, fused with weight `boosting_tree_alpha` >= 0 (alone or beside the LM:
    `mi355x_ctc_beam_decode_fused`): the search adds boosting_tree_alpha * boost(sequence) to its rank, and the score returned holds
    the boost of the completed phrases only -- a phrase begun and not finished is not paid for -- with the n-best ordered by it.
    Every method makes one call with the models there are (`_fusion_models`): none, the LM, the tree, or both.
    `stream_commit_every` = N (None: never): the streaming step of the models commits the state after every N-th chunk
    (`commit_stream`), with `stream_stable_frames` = S (None: the exact commit) as the age beyond which a partial result is final."""

    confidence_cfg = None   # (the greedy decoder's attribute: confidences are not defined for the beam search)

    def __init__(self, vocabulary: Optional[Sequence[str]] = None, blank_id: Optional[int] = None, beam_size: int = 4,
                 return_best_hypothesis: bool = True, beam_threshold: float = 20.0, beam_beta: float = 0.0, ngram_lm=None,
                 ngram_lm_alpha: float = 0.0, boosting_tree=None, boosting_tree_alpha: float = 0.0,
                 stream_commit_every: Optional[int] = None, stream_stable_frames: Optional[int] = None):
        self._set_labels(vocabulary, blank_id)
        self.stream_commit_every, self.stream_stable_frames = _stream_commit_keys(stream_commit_every, stream_stable_frames)
        self.boosting_tree, self.boosting_tree_alpha = boosting_tree, float(boosting_tree_alpha)
        if not self.boosting_tree_alpha >= 0:
            raise ValueError(f"boosting_tree_alpha must be >= 0; got {boosting_tree_alpha}")
        if boosting_tree is not None:
            from .boosting_tree import BoostingTree
            if not isinstance(boosting_tree, BoostingTree):
                raise TypeError(f"boosting_tree must be a BoostingTree (BoostingTree.from_phrases), got {type(boosting_tree).__name__}")
            if boosting_tree.vocab_size != self.blank_id:
                raise ValueError(f"the boosting tree has {boosting_tree.vocab_size} labels, the decoder {self.blank_id} (blank_id = the "
                                 "label count)")
        self.beam_size, self.return_best_hypothesis = int(beam_size), bool(return_best_hypothesis)
        self.beam_threshold, self.beam_beta = float(beam_threshold), float(beam_beta)
        self.ngram_lm, self.ngram_lm_alpha = ngram_lm, float(ngram_lm_alpha)
        if not self.ngram_lm_alpha >= 0:
            raise ValueError(f"ngram_lm_alpha must be >= 0; got {ngram_lm_alpha}")
        if ngram_lm is not None:
            from .ngram_lm import NGramLM
            if not isinstance(ngram_lm, NGramLM):
                raise TypeError(f"ngram_lm must be an NGramLM (NGramLM.from_arpa), got {type(ngram_lm).__name__}")
            if ngram_lm.vocab_size != self.blank_id:
                raise ValueError(f"the LM has {ngram_lm.vocab_size} labels, the decoder {self.blank_id} (blank_id = the label count)")
        if not 1 <= self.beam_size <= 64:
            raise ValueError(f"beam_size must lie in 1..64 (one wave holds the beams of an utterance); got {beam_size}")
        if not self.beam_threshold > 0:
            raise ValueError(f"beam_threshold must be positive (inf: no pruning); got {beam_threshold}")

    @torch.no_grad()
    def decode_ids(self, log_probs: torch.Tensor, lengths: Optional[torch.Tensor] = None):
        """log_probs [B, T, V+1] (device) -> (tokens i32 [B,W,T]: hypotheses best first, -1 padded; tok_frame i32 [B,W,T]: the frame
        each token entered its hypothesis; hyp_len i32 [B,W]; score f32 [B,W], -inf for absent hypotheses; n_hyp i32 [B])"""
        _check_log_probs(log_probs)
        lp = log_probs.to(torch.float32).contiguous()
        lens = lengths.to(torch.int64).contiguous() if lengths is not None else None
        what, models = ops._ctc_beam_checked(self._fusion_models(), self.boosting_tree is not None, lp, "")
        return ops._ctc_beam_search(what, lp, lens, self.blank_id, self.beam_size, self.beam_threshold, self.beam_beta, models)

    def _fusion_models(self):
        """the (model, alpha) list of the search: the LM, where there is one, then the tree, where there is one"""
        lm = [(self.ngram_lm, self.ngram_lm_alpha)] if self.ngram_lm is not None else []
        return lm + ([(self.boosting_tree, self.boosting_tree_alpha)] if self.boosting_tree is not None else [])

    def nbest(self, log_probs, lengths=None):
        """per utterance the list of (token ids, score), best first: the D2H copy is the folded hypotheses, W * T integers an utterance"""
        tokens, _, hyp_len, score, n_hyp = (t.cpu() for t in self.decode_ids(log_probs, lengths))
        return [[(tokens[b, k, : int(hyp_len[b, k])].tolist(), float(score[b, k])) for k in range(int(n_hyp[b]))]
                for b in range(tokens.shape[0])]

    @torch.no_grad()
    def decode_stream(self, log_probs: torch.Tensor, lengths: Optional[torch.Tensor] = None,
                      state: Optional[CTCBeamStreamState] = None, emit: bool = True):
        """one chunk of the resumable search (`mi355x_ctc_beam_decode_stream` / `_fused_stream`): log_probs [B, T, V+1] and lengths
        [B] of THIS chunk (0: the stream has ended, its state passes through), `state` what the previous chunk returned (None: fresh
        streams) -> (the n-best of all frames so far, or None with emit=False; the next state).  The n-best is `decode_ids`'
        tuple with tokens / tok_frame i32 [B, W, capacity] in the state's buffers: NOT padded, valid up to hyp_len, overwritten by
        the next step; tok_frame counts from the stream's first frame.  Any cut of a stream into chunks gives the bits of
        `decode_ids` over all of it.  Of a COMMITTED state (`commit_stream`) the buffers hold the TAIL of each hypothesis -- the
        tokens behind `state.committed`, hyp_len their number -- with global frames and the whole hypothesis' score; `nbest_stream`
        puts the two together."""
        _check_log_probs(log_probs)
        lp = log_probs.to(torch.float32).contiguous()
        lens = lengths.to(torch.int64).contiguous() if lengths is not None else None
        what, models = ops._ctc_beam_checked(self._fusion_models(), self.boosting_tree is not None, lp, "_stream")
        return ops._ctc_beam_search_stream(what, lp, lens, self.blank_id, self.beam_size, self.beam_threshold, self.beam_beta, state,
                                           models, emit)

    def nbest_stream(self, log_probs, lengths=None, state=None, best_only: bool = False):
        """`decode_stream` to host lists: per stream the (token ids, score, global frame of each token) of its hypotheses so far,
        best first (best_only: the first one alone), and the next state.  The D2H copy is the hypotheses up to the longest one; of a
        committed state their tails, in front of which the committed tokens the state keeps on the host are put: the hypotheses
        are whole either way."""
        (tokens, tok_frame, hyp_len, score, n_hyp), nxt = self.decode_stream(log_probs, lengths, state, emit=True)
        hyp_len, score, n_hyp = hyp_len.cpu(), score.cpu(), n_hyp.cpu()
        K = 1 if best_only else int(n_hyp.max())
        L = int(hyp_len[:, :K].max()) if K else 0
        tokens, tok_frame = tokens[:, :K, :L].cpu(), tok_frame[:, :K, :L].cpu()
        done = [(list(ids), list(frames)) for ids, frames in nxt.committed]
        out = [[(done[b][0] + tokens[b, k, : int(hyp_len[b, k])].tolist(), float(score[b, k]),
                 done[b][1] + tok_frame[b, k, : int(hyp_len[b, k])].tolist())
                for k in range(min(K, int(n_hyp[b])))] for b in range(tokens.shape[0])]
        return out, nxt

    def commit_stream(self, state: CTCBeamStreamState, stable_frames: Optional[int] = None):
        """commit what the live hypotheses of every stream agree on (`ops.ctc_beam_commit`): -> (per stream the NEWLY committed
        (token ids, global frames), the next state), whose tree holds only what is still open.  stable_frames None: the exact
        commit -- every later result is what it would have been.  stable_frames = S: partial-result stabilisation -- the beams that
        differ from the best one in anything older than S frames are dropped first, so the text older than S frames is final and
        the tree holds at most S frames.  A dropped beam is identified by its node: one that spells the same old text under another
        node goes too.  The beam that always survives is the best one of the SEARCH order.  With a boosting tree the n-best is
        ordered by the scores with the final terms, so the hypothesis shown first at the step of a forced commit can be a beam that
        commit drops: that one hypothesis may leave the newly committed text (the models' `stable_length` then counts what was
        committed before it); every later n-best starts with all that is committed."""
        return ops.ctc_beam_commit(state, stable_frames)

    def __call__(self, log_probs, lengths=None):
        texts = [[self.ids_to_text(ids) for ids, _ in hyps] for hyps in self.nbest(log_probs, lengths)]
        return [(t[0] if t else "") for t in texts] if self.return_best_hypothesis else texts

    def best_texts(self, log_probs, lengths=None) -> List[str]:
        """the best hypothesis of every utterance, whatever `return_best_hypothesis` says: what WER and predict_step score"""
        return [(self.ids_to_text(hyps[0][0]) if hyps else "") for hyps in self.nbest(log_probs, lengths)]


_LM_KEYS = ("ngram_lm_model", "kenlm_path")


def _ngram_lm_from_config(beam, vocabulary, what, sec="beam"):
    """the LM of a `beam` sub-section (None without one): `ngram_lm_arpa` = the path of an ARPA text file or an NGramLM,
    `ngram_lm_token_offset` (100; None: the file's words are the vocabulary's strings).  KenLM binaries and `.nemo` LM archives are
    not read: the reference's keys for them are refused by name.  `sec` names the sub-section in messages (the transducer
    heads read `greedy`)."""
    for key in _LM_KEYS:
        if beam.get(key):
            raise NotImplementedError(f"{what} decoding: `{sec}.{key}` (KenLM binaries and .nemo LM archives are not read here; give "
                                      f"an ARPA text file under `{sec}.ngram_lm_arpa`)")
    arpa = beam.get("ngram_lm_arpa")
    if arpa is None or (isinstance(arpa, str) and not arpa):
        if float(beam.get("ngram_lm_alpha") or 0.0) != 0.0:
            raise NotImplementedError(f"{what} decoding: `{sec}.ngram_lm_alpha` != 0 without `{sec}.ngram_lm_arpa` (there is no language "
                                      "model to weigh)")
        return None
    from .ngram_lm import NGramLM
    if isinstance(arpa, NGramLM):
        return arpa
    if not os.path.isfile(str(arpa)):
        raise FileNotFoundError(f"{what} decoding: `{sec}.ngram_lm_arpa` = {arpa!r} is not a file")
    if vocabulary is None:   # (the section is only being checked)
        return None
    offset = beam.get("ngram_lm_token_offset", 100)
    return NGramLM.from_arpa(arpa, len(vocabulary), token_offset=offset, vocabulary=list(vocabulary) if offset is None else None)


_BOOST_REFUSED = {"unk_score": 0.0, "final_eos_score": 0.0, "score_per_phrase": 0.0}   # the reference's keys that are not provided


def _boosting_tree_from_config(beam, vocabulary, what, text_to_ids, sec="beam"):
    """the boosting tree of a `beam` sub-section (None without one): `boosting_tree` = a BoostingTree, or {key_phrases_list: [...],
    key_phrases_file: a text file with one phrase per line, context_score (1.0), depth_scaling (2.0)}; the phrases are tokenised with
    `text_to_ids` (the model's own: its tokenizer, or its character parser).  `unk_score`, `final_eos_score` and `score_per_phrase`
    of the reference are refused by name where they are not their defaults; so are a weight without phrases, a phrase that tokenises
    to nothing and a file that is not there.  `sec` names the sub-section in messages."""
    alpha = float(beam.get("boosting_tree_alpha") or 0.0)
    if alpha < 0:
        raise ValueError(f"{what} decoding: `{sec}.boosting_tree_alpha` must be >= 0; got {alpha}")
    section = beam.get("boosting_tree")
    from .boosting_tree import BoostingTree
    if isinstance(section, BoostingTree):
        return section, alpha
    section = dict(section or {})
    for key, default in _BOOST_REFUSED.items():
        if section.get(key) is not None and float(section[key]) != default:
            raise NotImplementedError(f"{what} decoding: `{sec}.boosting_tree.{key}` = {section[key]!r} (only the default {default} is "
                                      "provided)")
    phrases = [str(p) for p in (section.get("key_phrases_list") or [])]
    path = section.get("key_phrases_file")
    if path is not None and str(path):
        if not os.path.isfile(str(path)):
            raise FileNotFoundError(f"{what} decoding: `{sec}.boosting_tree.key_phrases_file` = {path!r} is not a file")
        with open(str(path), encoding="utf-8") as f:
            phrases += [line.strip() for line in f if line.strip()]
    if not phrases:
        if alpha != 0.0:
            raise ValueError(f"{what} decoding: `{sec}.boosting_tree_alpha` != 0 without key phrases (`{sec}.boosting_tree."
                             "key_phrases_list` / `key_phrases_file`): there is nothing to boost")
        return None, alpha
    if vocabulary is None:   # (the section is only being checked)
        return None, alpha
    if text_to_ids is None:
        raise ValueError(f"{what} decoding: `{sec}.boosting_tree` needs the model's text_to_ids to tokenise its phrases")
    ids = []
    for p in phrases:
        t = [int(i) for i in text_to_ids(p)]
        if not t:
            raise ValueError(f"{what} decoding: the key phrase {p!r} tokenises to nothing")
        ids.append(t)
    return BoostingTree.from_phrases(ids, len(vocabulary), context_score=float(section.get("context_score", 1.0)),
                                     depth_scaling=float(section.get("depth_scaling", 2.0))), alpha


def ctc_decoder_from_config(decoding_cfg, vocabulary=None, what: str = "CTC", text_to_ids=None):
    """The one place that reads a CTC head's `decoding` section (`what` names the head in messages): checks it and, with a
    vocabulary, returns its decoding object -- GreedyCTCDecoder for `greedy` / `greedy_batch`, BeamBatchedCTCDecoder for
    `beam_batch` (its `beam` sub-section: beam_size, return_best_hypothesis, beam_threshold, beam_beta, ngram_lm_arpa,
    ngram_lm_alpha, ngram_lm_token_offset, boosting_tree, boosting_tree_alpha: `_boosting_tree_from_config`, whose phrases
    `text_to_ids` tokenises; stream_commit_every, stream_stable_frames: `_stream_commit_keys`, both None by default).
    Everything else the reference knows (beam = pyctcdecode / KenLM, flashlight, wfst: ctc_decoding.py:231-236), its keys for
    KenLM / .nemo language models, and an LM weight without an LM raise NotImplementedError."""
    dcfg = dict(decoding_cfg or {})
    strategy = str(dcfg.get("strategy", "greedy_batch"))
    if strategy in ("greedy", "greedy_batch"):
        return None if vocabulary is None else GreedyCTCDecoder(vocabulary=list(vocabulary), confidence_cfg=dcfg.get("confidence_cfg"))
    if strategy != "beam_batch":
        raise NotImplementedError(f"{what} decoding strategy '{strategy}' (implemented: greedy, greedy_batch, beam_batch)")
    beam = dict(dcfg.get("beam") or {})
    alpha = float(beam.get("ngram_lm_alpha") or 0.0)
    if alpha < 0:
        raise ValueError(f"{what} decoding: `beam.ngram_lm_alpha` must be >= 0; got {alpha}")
    from .confidence import confidence_from
    if confidence_from(dcfg.get("confidence_cfg")) is not None:
        raise NotImplementedError(f"{what} decoding: `confidence_cfg` with strategy 'beam_batch' (confidences come from the greedy search)")
    lm = _ngram_lm_from_config(beam, vocabulary, what)
    tree, tree_alpha = _boosting_tree_from_config(beam, vocabulary, what, text_to_ids)
    every, stable = _stream_commit_keys(beam.get("stream_commit_every"), beam.get("stream_stable_frames"), f"{what} decoding")
    if vocabulary is None:
        return None
    return BeamBatchedCTCDecoder(vocabulary=list(vocabulary), beam_size=beam.get("beam_size", 4),
                                 return_best_hypothesis=beam.get("return_best_hypothesis", True),
                                 beam_threshold=beam.get("beam_threshold", 20.0), beam_beta=beam.get("beam_beta", 0.0),
                                 ngram_lm=lm, ngram_lm_alpha=alpha, boosting_tree=tree, boosting_tree_alpha=tree_alpha,
                                 stream_commit_every=every, stream_stable_frames=stable)


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

    def __init__(self, decoding, use_cer: bool = False):
        self.decoding, self.use_cer = decoding, use_cer
        self.scores = 0
        self.words = 0

    def update(self, predictions: torch.Tensor, predictions_lengths, targets: torch.Tensor, targets_lengths):
        hyps = getattr(self.decoding, "best_texts", self.decoding)(predictions, predictions_lengths)   # (beam search: the best hypothesis)
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
