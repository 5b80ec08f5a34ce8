"""Phrase boosting (context biasing) for the CTC prefix beam search (`mi355x_ctc_beam_decode_fused`): the key phrases of a
deployment as an Aho-Corasick automaton over token ids, flattened into the back-off automaton the kernel already walks for an n-gram
model (include/mi355x_asr.h states the semantics; this is the reference's boosting tree / the icefall context graph).

Trie children are the arcs, the failure link is the back-off, and the back-off weight takes back the boost of the part of a phrase
that no longer matches.  With `context_score` cs and `depth_scaling` ds the k-th token of a phrase is worth ts(k) = cs (k = 1) or
cs * ds (k > 1), part(m) = ts(1) + .. + ts(m), full(p) = part(|p|):
  arc into node n      ts(depth n) + out(n), out(n) = the sum of full over the phrases that end at n or on n's failure chain
  back-off of node n   part(depth fail(n)) - part(depth n), to fail(n)
  state 0              the root, V arcs: a label that starts no phrase has value 0 and leads back to the root
  state 1              where the search starts: an arc-less alias of the root, back-off 0
  state_final[s]       -part(depth s): what the output adds, so that a phrase begun and not finished is not paid for
The tables satisfy everything `NGramLM._check` asks and `lm_ub` is NGramLM's bound (arc values are positive here: the search's
early-outs need it).  `score` walks the tables on the host in float64: the check of the flattening that needs no GPU."""
from __future__ import annotations

from typing import Sequence

import numpy as np

from .ngram_lm import NGramLM


class BoostingTree(NGramLM):
    """the six tables of NGramLM and `state_final`; `phrases` (de-duplicated tuples), `context_score`, `depth_scaling`"""

    def __init__(self, vocab_size, order, state_arc_begin, arc_tok, arc_logp, arc_next, state_bo, state_bo_next, state_len, state_final,
                 phrases=(), context_score=1.0, depth_scaling=2.0):
        super().__init__(vocab_size, order, state_arc_begin, arc_tok, arc_logp, arc_next, state_bo, state_bo_next, state_len)
        self.state_final = np.ascontiguousarray(state_final, dtype=np.float32)
        if self.state_final.shape != (self.num_states,) or not np.isfinite(self.state_final).all():
            raise ValueError("boosting tree: state_final is not one finite value per state")
        self.phrases = tuple(phrases)
        self.context_score, self.depth_scaling = float(context_score), float(depth_scaling)

    @classmethod
    def from_phrases(cls, phrases_ids: Sequence[Sequence[int]], vocab_size: int, context_score: float = 1.0, depth_scaling: float = 2.0):
        V, cs, ds = int(vocab_size), float(context_score), float(depth_scaling)
        if not (cs > 0 and np.isfinite(cs) and ds > 0 and np.isfinite(ds)):
            raise ValueError(f"boosting tree: context_score and depth_scaling must be positive and finite; got {context_score}, "
                             f"{depth_scaling}")
        if V < 1:
            raise ValueError(f"boosting tree: vocab_size {vocab_size}")
        phrases_ids = list(phrases_ids) if phrases_ids is not None else []
        if not phrases_ids:
            raise ValueError("boosting tree: the phrase list is empty")
        phrases = []
        for n, p in enumerate(phrases_ids):
            p = tuple(int(c) for c in p)
            if not p:
                raise ValueError(f"boosting tree: phrase {n} is empty")
            if min(p) < 0 or max(p) >= V:
                raise ValueError(f"boosting tree: phrase {n} = {list(p)} has an id outside 0..{V - 1}")
            if p not in phrases:
                phrases.append(p)

        def part(m):   # float64
            return 0.0 if m == 0 else cs + (m - 1) * (cs * ds)

        # trie: node 0 = the root; nodes in order of creation, then renumbered by breadth
        kids, depth, ends = [{}], [0], [0.0]
        for p in phrases:
            n = 0
            for c in p:
                if c not in kids[n]:
                    kids[n][c] = len(kids)
                    kids.append({})
                    depth.append(depth[n] + 1)
                    ends.append(0.0)
                n = kids[n][c]
            ends[n] += part(len(p))
        fail, out, bfs = [0] * len(kids), list(ends), []
        queue = [(0, c, n) for c, n in sorted(kids[0].items())]
        while queue:   # breadth first: a node's failure target is shallower, so its `out` is complete when it is used
            nxt = []
            for parent, c, n in queue:
                f = fail[parent]
                while parent and f and c not in kids[f]:
                    f = fail[f]
                fail[n] = kids[f][c] if (parent and c in kids[f]) else 0
                out[n] = ends[n] + out[fail[n]]
                bfs.append(n)
                nxt += [(n, cc, nn) for cc, nn in sorted(kids[n].items())]
            queue = nxt
        state = {0: 0}   # trie node -> automaton state; state 1 is the alias of the root
        state.update({n: 2 + i for i, n in enumerate(bfs)})
        ts = lambda d: cs if d == 1 else cs * ds
        begin, tok, val, nxt_state = [0], [], [], []
        for c in range(V):   # the root: every label
            n = kids[0].get(c)
            tok.append(c)
            val.append(ts(1) + out[n] if n is not None else 0.0)
            nxt_state.append(state[n] if n is not None else 0)
        begin += [V, V]   # (state 1 has no arcs)
        for n in bfs:
            for c, m in sorted(kids[n].items()):
                tok.append(c)
                val.append(ts(depth[m]) + out[m])
                nxt_state.append(state[m])
            begin.append(len(tok))
        nodes = [0, 0] + bfs   # state -> trie node
        bo = [0.0, 0.0] + [part(depth[fail[n]]) - part(depth[n]) for n in bfs]
        bo_next = [0, 0] + [state[fail[n]] for n in bfs]
        slen = [0, 1] + [depth[n] for n in bfs]
        final = [0.0, 0.0] + [-part(depth[n]) for n in bfs]
        assert len(nodes) == len(bo)
        return cls(V, max(depth) + 1, begin, tok, val, nxt_state, bo, bo_next, slen, final, phrases, cs, ds)

    def score(self, ids: Sequence[int]):
        """(boost(ids), boost_final(ids)) in float64: the walk of the kernel over the tables, and the final term of the last state"""
        total, s = 0.0, 1
        for c in ids:
            v, s = self.lookup(s, int(c))
            total += v
        return total, total + float(self.state_final[s])

    def to(self, device):
        """the seven tables on `device`: the six of the C ABI in its order, then state_final; cached per device"""
        import torch
        key = str(torch.device(device))
        if key not in self._device:
            self._device[key] = NGramLM.to(self, device) + (torch.from_numpy(self.state_final).to(device),)
        return self._device[key]
