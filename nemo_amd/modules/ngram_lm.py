"""Token-level back-off n-gram language model for the CTC prefix beam search (`mi355x_ctc_beam_decode_lm`): an ARPA reader and
the flattening of the model into the back-off automaton that include/mi355x_asr.h states and the kernel walks.

ARPA is plain text (log10 values); KenLM binaries and `.nemo` LM archives are not read.  A word of the file is a LABEL: with
`token_offset=k` the single character chr(id + k) (the reference's DEFAULT_TOKEN_OFFSET = 100 convention for LMs trained on BPE
ids), with `token_offset=None` a string of `vocabulary`.  `<s>` is the start context (never scored), n-grams with `</s>` are dropped
(no end-of-sentence term is ever added by the search), and so are n-grams of order > 1 that contain `<unk>`; `<unk>`'s unigram
value stands in for labels that have no unigram.

Automaton: a state is a context the file holds as an n-gram of order < N (closed under prefixes; state 0 = the empty context,
state 1 = <s>), its arcs are the file's n-grams context.c sorted by c; state 0 has exactly V arcs, arc c = label c, so every look-up
ends there.  `score` walks these tables on the host in float64: the check of the flattening that needs no GPU."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np

BOS = -1          # <s> inside n-gram tuples
_LN10 = math.log(10.0)
_UB_SLACK = 1e-3  # lm_ub is a float64 bound; the kernel's float32 sums, whatever their association, stay below it with this


class NGramLM:
    """the six tables (numpy; `to(device)` gives them as device tensors), `order`, `vocab_size`, `lm_ub`"""

    def __init__(self, vocab_size: int, order: int, state_arc_begin, arc_tok, arc_logp, arc_next, state_bo, state_bo_next, state_len):
        self.vocab_size, self.order = int(vocab_size), int(order)
        self.state_arc_begin = np.ascontiguousarray(state_arc_begin, dtype=np.int32)
        self.arc_tok = np.ascontiguousarray(arc_tok, dtype=np.int32)
        self.arc_logp = np.ascontiguousarray(arc_logp, dtype=np.float32)
        self.arc_next = np.ascontiguousarray(arc_next, dtype=np.int32)
        self.state_bo = np.ascontiguousarray(state_bo, dtype=np.float32)
        self.state_bo_next = np.ascontiguousarray(state_bo_next, dtype=np.int32)
        self.state_len = np.ascontiguousarray(state_len, dtype=np.int32)   # tokens in the state's context (<s> counts)
        self._check()
        self.lm_ub = self._upper_bound()
        self._device = {}

    # ------------------------------------------------------------------------------------------ what the kernel relies on
    def _check(self):
        V, S, A = self.vocab_size, self.num_states, self.num_arcs
        beg = self.state_arc_begin
        if V < 1 or self.order < 1 or S < 2 or A < V:
            raise ValueError(f"n-gram LM: vocab_size {V}, order {self.order}, {S} states, {A} arcs")
        if beg.shape != (S + 1,) or self.state_bo_next.shape != (S,) or self.state_len.shape != (S,):
            raise ValueError("n-gram LM: the state arrays differ in length")
        if self.arc_logp.shape != (A,) or self.arc_next.shape != (A,):
            raise ValueError("n-gram LM: the arc arrays differ in length")
        if beg[0] != 0 or beg[-1] != A or (np.diff(beg) < 0).any() or beg[1] != V:
            raise ValueError("n-gram LM: state_arc_begin is not an ascending partition of the arcs with V arcs in state 0")
        if not np.array_equal(self.arc_tok[:V], np.arange(V, dtype=np.int32)):
            raise ValueError("n-gram LM: the arcs of state 0 are not the labels 0..V-1 in order")
        if A and (self.arc_tok.min() < 0 or self.arc_tok.max() >= V):
            raise ValueError("n-gram LM: an arc label is outside 0..V-1")
        first = np.zeros(A, dtype=bool)
        first[beg[:-1][beg[:-1] < A]] = True
        if (np.diff(self.arc_tok)[~first[1:]] <= 0).any():
            raise ValueError("n-gram LM: the arcs of a state are not sorted by label")
        if self.arc_next.min() < 0 or self.arc_next.max() >= S or self.state_bo_next.min() < 0 or self.state_bo_next.max() >= S:
            raise ValueError("n-gram LM: a state index is out of range")
        if self.state_len[0] != 0 or self.state_bo_next[0] != 0 or (self.state_len[1:] < 1).any():
            raise ValueError("n-gram LM: state 0 is not the empty context")
        if (self.state_len[self.state_bo_next[1:]] >= self.state_len[1:]).any():
            raise ValueError("n-gram LM: a back-off chain does not shorten")
        if not (np.isfinite(self.arc_logp).all() and np.isfinite(self.state_bo).all()):
            raise ValueError("n-gram LM: a table value is not finite")

    def _upper_bound(self) -> float:
        """ub(s) = max(max arc logp of s, bo[s] + ub(bo_next[s])) in float64 over the states by context length; + slack, rounded up
        to float32.  Back-off weights may be positive and models unnormalised: 0 is not assumed."""
        S, beg = self.num_states, self.state_arc_begin
        lp = self.arc_logp.astype(np.float64)
        own = np.full(S, -np.inf)
        nz = np.flatnonzero(np.diff(beg) > 0)
        own[nz] = np.maximum.reduceat(lp, beg[:-1][nz])
        ub = np.full(S, -np.inf)
        for s in np.argsort(self.state_len, kind="stable"):
            ub[s] = own[s] if s == 0 else max(own[s], float(self.state_bo[s]) + ub[self.state_bo_next[s]])
        bound = np.float32(ub.max() + _UB_SLACK)
        if float(bound) < ub.max() + _UB_SLACK:
            bound = np.nextafter(bound, np.float32(np.inf))
        return float(bound)

    @property
    def num_states(self) -> int:
        return int(self.state_bo.shape[0])

    @property
    def num_arcs(self) -> int:
        return int(self.arc_tok.shape[0])

    # ------------------------------------------------------------------------------------------ host scorer over the tables
    def lookup(self, state: int, c: int):
        """(ln p(c | state) in float64, next state): the walk of the kernel"""
        if not 0 <= c < self.vocab_size:
            raise ValueError(f"label {c} outside 0..{self.vocab_size - 1}")
        acc, s = 0.0, int(state)
        while s != 0:
            lo, hi = int(self.state_arc_begin[s]), int(self.state_arc_begin[s + 1])
            k = lo + int(np.searchsorted(self.arc_tok[lo:hi], c))
            if k < hi and self.arc_tok[k] == c:
                return acc + float(self.arc_logp[k]), int(self.arc_next[k])
            acc += float(self.state_bo[s])
            s = int(self.state_bo_next[s])
        return acc + float(self.arc_logp[c]), int(self.arc_next[c])

    def score(self, ids: Sequence[int]) -> float:
        """lm(ids): the sum of ln p(token | <s> and the tokens before it), float64, no </s> term"""
        total, s = 0.0, 1
        for c in ids:
            v, s = self.lookup(s, int(c))
            total += v
        return total

    def to(self, device):
        """the tables on `device`, in the order of the C ABI; cached per device"""
        import torch
        key = str(torch.device(device))
        if key not in self._device:
            self._device[key] = tuple(torch.from_numpy(a).to(device) for a in (
                self.state_arc_begin, self.arc_tok, self.arc_logp, self.arc_next, self.state_bo, self.state_bo_next))
        return self._device[key]

    # ------------------------------------------------------------------------------------------ ARPA
    @classmethod
    def from_arpa(cls, path, vocab_size: int, token_offset: Optional[int] = 100, vocabulary: Optional[Sequence[str]] = None):
        V = int(vocab_size)
        if token_offset is None:
            if vocabulary is None:
                raise ValueError("token_offset=None: the words of the file are looked up in `vocabulary`, which is missing")
            words = {w: i for i, w in enumerate(list(vocabulary)[:V])}
            if len(words) != V:
                raise ValueError(f"`vocabulary` has {len(words)} distinct strings for vocab_size {V}")
            bad = [w for w in words if not w or " " in w or "\t" in w or "\n" in w or w in ("<s>", "</s>", "<unk>")]
            if bad:
                raise ValueError(f"`vocabulary` strings {bad[:4]} cannot be words of an ARPA file (empty, blank inside, or a "
                                 "reserved word): train the LM on chr(id + token_offset) and pass that token_offset")
        else:
            words = {chr(i + int(token_offset)): i for i in range(V)}
        grams, order, unk = _read_arpa(str(path), words)
        return cls._from_ngrams(grams, order, V, unk)

    @classmethod
    def _from_ngrams(cls, grams, order, V, unk):
        """grams: {tuple of ids (BOS = -1 first, perhaps): (log10 p, log10 backoff)}, </s> and <unk> n-grams already dropped"""
        for c in range(V):
            if (c,) not in grams:
                if unk is None:
                    raise ValueError(f"ARPA: label {c} has no unigram and the file has no <unk> to stand in for it")
                grams[(c,)] = (unk, 0.0)
        contexts = {g for g in grams if 1 <= len(g) < order} | {g[:-1] for g in grams if len(g) > 1}
        for g in list(contexts):   # closed under prefixes: the longest suffix that is a state can then be found from a state alone
            while len(g) > 1:
                g = g[:-1]
                contexts.add(g)
        contexts.discard(())
        contexts.discard((BOS,))
        states = [(), (BOS,)] + sorted(contexts, key=lambda g: (len(g), g))
        index = {g: i for i, g in enumerate(states)}

        def suffix_state(g):   # the longest suffix of g that is a state
            for k in range(len(g) + 1):
                if g[k:] in index:
                    return index[g[k:]]
            raise AssertionError

        arcs = [[] for _ in states]
        for g, (lp, _) in grams.items():
            if g == (BOS,):
                continue
            nxt = suffix_state(g[-(order - 1):]) if order > 1 else 0
            arcs[index[g[:-1]]].append((g[-1], np.float32(lp * _LN10), nxt))
        begin, tok, logp, nxt = [0], [], [], []
        for a in arcs:
            a.sort(key=lambda x: x[0])
            tok += [x[0] for x in a]
            logp += [x[1] for x in a]
            nxt += [x[2] for x in a]
            begin.append(len(tok))
        bo = [np.float32(grams[g][1] * _LN10) if (g in grams and order > 1) else np.float32(0.0) for g in states]
        bo[0] = np.float32(0.0)
        bo_next = [0] + [suffix_state(g[1:]) for g in states[1:]]
        return cls(V, order, begin, tok, logp, nxt, bo, bo_next, [len(g) for g in states])


def _number(text, path, n, line):
    try:
        v = float(text)
    except ValueError:
        raise ValueError(f"{path}:{n}: '{text}' is not a number in: {line!r}") from None
    if not math.isfinite(v):
        raise ValueError(f"{path}:{n}: non-finite number in: {line!r}")
    return v


def _read_arpa(path, words):
    """-> ({ids tuple: (log10 p, log10 backoff)}, order, log10 p of <unk> or None).  Fields are separated by tabs (probability, the
    words with single spaces between them, the optional back-off), or by spaces throughout.  Lines are split at '\\n' only and never
    stripped of anything but '\\r': a label's character may be one that Unicode calls white space."""
    with open(path, encoding="utf-8", newline="\n") as f:
        lines = f.read().split("\n")
    counts, grams, seen, unk = {}, {}, {}, None
    section = None   # None before \data\, 0 inside it, n inside \n-grams:
    ended = False
    for n, raw in enumerate(lines, 1):
        line = raw.rstrip("\r")
        if not line.strip(" \t"):
            continue
        if ended:
            raise ValueError(f"{path}:{n}: text behind \\end\\: {line!r}")
        if line.startswith("\\"):
            head = line.strip(" \t")
            if head == "\\data\\" and section is None:
                section = 0
            elif head == "\\end\\" and section is not None:
                ended = True
            elif head.endswith("-grams:") and head[1:-7].isdigit() and section is not None and int(head[1:-7]) in counts:
                section = int(head[1:-7])
                seen.setdefault(section, 0)
            else:
                raise ValueError(f"{path}:{n}: unexpected section line {line!r}")
            continue
        if section is None:
            continue   # (text in front of \data\ is a comment)
        if section == 0:
            body = line.strip(" \t")
            if not body.startswith("ngram ") or "=" not in body:
                raise ValueError(f"{path}:{n}: expected 'ngram N=count', got {line!r}")
            k, cnt = body[6:].split("=", 1)
            if not (k.strip().isdigit() and cnt.strip().isdigit()) or int(k) < 1:
                raise ValueError(f"{path}:{n}: expected 'ngram N=count', got {line!r}")
            counts[int(k)] = int(cnt)
            continue
        fields = line.split("\t")
        if len(fields) == 1:
            parts = [p for p in line.split(" ") if p]
            fields = [parts[0], " ".join(parts[1:1 + section])] + parts[1 + section:]
        if len(fields) not in (2, 3):
            raise ValueError(f"{path}:{n}: expected 'log10p<TAB>words[<TAB>backoff]', got {line!r}")
        ws = fields[1].split(" ")
        if len(ws) != section:
            raise ValueError(f"{path}:{n}: {len(ws)} words in the {section}-grams section: {line!r}")
        lp = _number(fields[0], path, n, line)
        bo = _number(fields[2], path, n, line) if len(fields) == 3 else 0.0
        seen[section] += 1
        ids, drop = [], False
        for k, w in enumerate(ws):
            if w == "<s>":
                if k != 0:
                    raise ValueError(f"{path}:{n}: <s> behind the first word of an n-gram: {line!r}")
                ids.append(BOS)
            elif w == "</s>":
                drop = True
            elif w in words:
                ids.append(words[w])
            elif w == "<unk>":
                if section == 1:
                    unk = lp
                drop = True
            else:
                raise ValueError(f"{path}:{n}: unknown word {w!r} (not a label, <s>, </s> or <unk>): {line!r}")
        if drop:
            continue
        g = tuple(ids)
        if g in grams:
            raise ValueError(f"{path}:{n}: the n-gram is in the file twice: {line!r}")
        grams[g] = (lp, bo)
    if section is None or not ended:
        raise ValueError(f"{path}: not an ARPA file (no \\data\\ ... \\end\\)")
    if not counts or sorted(counts) != list(range(1, max(counts) + 1)):
        raise ValueError(f"{path}: the \\data\\ section does not list the orders 1..N")
    for k, cnt in counts.items():
        if seen.get(k, 0) != cnt:
            raise ValueError(f"{path}: \\data\\ announces {cnt} {k}-grams, the \\{k}-grams: section has {seen.get(k, 0)}")
    return grams, max(counts), unk
