"""Oracle of the CTC prefix beam search with phrase boosting (`mi355x_ctc_beam_decode_fused`; include/mi355x_asr.h states it): the
search of tests/ctc_beam_lm_oracle.py over token tuples with
    rank = ((tot + beta * len) + lm_alpha * lm(prefix)) + boost_alpha * boost(prefix)          (the LM term only with a model)
and, at output, score = rank + boost_alpha * (-pending(prefix)), the n-best ordered by that score (ties: the slot in the search
order).  boost is computed from the PHRASE SET by string matching -- `boost_parts` compares slices of the prefix with every phrase at
every end position -- and shares nothing with nemo_amd/modules/boosting_tree.py: there is no trie, no failure link, no automaton here.
`_Boost.row` gives boost(prefix . c) for every label at once by the same definition (the slices of prefix . c looked up in the set of
phrases and in the set of their prefixes), cached per prefix so that the search stays fast; tests compare it with `boost_parts`.

With positive boosts the extensions cannot be pre-selected by their acoustic value: ALL live extensions are ranked with the fused
rank (as tests/ctc_beam_lm_oracle.py does).  Also here: the generator of the phrase sets, which takes its phrases from the inputs
themselves (random phrases would never complete at C = 129)."""
import numpy as np

import ctc_beam_lm_oracle as L
import ctc_beam_oracle as O

NEG = -np.inf


def ts(k, cs, ds):
    """the worth of the k-th token (1-based) of a phrase"""
    return cs if k == 1 else cs * ds


def part(m, cs, ds):
    return sum(ts(k, cs, ds) for k in range(1, m + 1))


def dedup(phrases):
    out = []
    for p in phrases:
        p = tuple(int(c) for c in p)
        assert p
        if p not in out:
            out.append(p)
    return out


def boost_parts(phrases, y, cs=1.0, ds=2.0):
    """(complete(y), pending(y)) in float64 by brute force: every end position of y against every phrase, slice by slice"""
    phrases, y = dedup(phrases), tuple(y)
    complete = 0.0
    for end in range(1, len(y) + 1):
        for p in phrases:
            if len(p) <= end and y[end - len(p):end] == p:
                complete += part(len(p), cs, ds)
    m = 0
    for k in range(1, len(y) + 1):   # the longest suffix of y that is a prefix of some phrase (a whole phrase counts)
        if any(len(p) >= k and p[:k] == y[len(y) - k:] for p in phrases):
            m = k
    return complete, part(m, cs, ds)


class _Boost:
    """complete / pending of a prefix and the row boost(prefix . c), c = 0..V-1, float64, cached per prefix"""

    def __init__(self, phrases, V, cs, ds):
        self.phrases, self.V, self.cs, self.ds = set(dedup(phrases)), V, cs, ds
        self.heads = {p[:k] for p in self.phrases for k in range(1, len(p) + 1)}
        self.longest = max(len(p) for p in self.phrases)
        self.labels = sorted({c for p in self.phrases for c in p})
        self.parts = {(): (0.0, 0.0)}   # prefix -> (complete, pending)
        self.rows = {}

    def _extend(self, prefix, c):
        y = prefix + (c,)
        if y not in self.parts:
            complete = self.parts[prefix][0]
            m = 0
            for k in range(1, min(len(y), self.longest) + 1):
                tail = y[len(y) - k:]
                if tail in self.phrases:
                    complete += part(k, self.cs, self.ds)
                if tail in self.heads:
                    m = k
            self.parts[y] = (complete, part(m, self.cs, self.ds))
        return self.parts[y]

    def of(self, prefix):
        if prefix not in self.parts:
            self.of(prefix[:-1])
            self._extend(prefix[:-1], prefix[-1])
        return self.parts[prefix]

    def row(self, prefix):
        if prefix not in self.rows:
            complete = self.of(prefix)[0]
            r = np.full(self.V, complete, dtype=np.float64)   # a label no phrase holds: nothing completes, nothing is pending
            for c in self.labels:
                r[c] = sum(self._extend(prefix, c))
            self.rows[prefix] = r
        return self.rows[prefix]


def beam_search_boost(lp, blank, W, theta=np.inf, beta=0.0, phrases=(), boost_alpha=0.0, cs=1.0, ds=2.0, ng=None, order=1,
                      lm_alpha=0.0, dtype=np.float64):
    """-> dict(nbest = [(tokens, final score)] in output order, search = [(tokens, rank)] in search order, pending = {tokens:
    pending}, complete = {tokens: complete}, margin = the cut margin of the SEARCH ranks, min_candidates)"""
    lp32 = np.asarray(lp, dtype=np.float32)
    T, C = lp32.shape
    assert blank == C - 1
    lpd = lp32.astype(dtype)
    beta, lm_alpha, boost_alpha = dtype(beta), dtype(lm_alpha), dtype(boost_alpha)
    bt = _Boost(phrases, C - 1, cs, ds)
    rows = L._Rows(ng, order, C - 1, dtype) if ng is not None else None
    lm = {(): dtype(0.0)}

    def lm_ext(prefix):
        return (lm[prefix] + rows.cond_row(L.context_of(prefix, order))).astype(dtype)

    def rank_of(tot, prefix):
        r = dtype(tot + beta * dtype(len(prefix)))
        if rows is not None:
            r = dtype(r + dtype(lm_alpha * lm[prefix]))
        return dtype(r + dtype(boost_alpha * dtype(sum(bt.of(prefix)))))

    beams = {(): (dtype(0.0), dtype(NEG))}
    margin, min_cand = np.inf, None
    for t in range(T):
        ok = O.considered(lp32[t], theta)
        row = lpd[t]
        stay, exts = {}, []
        for prefix, (pb, pnb) in beams.items():
            tot = O.logaddexp(pb, pnb, dtype)[()]
            spb = tot + row[blank] if ok[blank] else dtype(NEG)
            spnb = dtype(NEG)
            e = (tot + row).astype(dtype)
            if prefix:
                last = prefix[-1]
                if ok[last]:
                    spnb = pnb + row[last]
                e[last] = pb + row[last]
            e[~ok] = NEG
            e[blank] = NEG
            stay[prefix] = [dtype(spb), dtype(spnb)]
            exts.append((prefix, e))
        for prefix, e in exts:
            for q in stay:
                if len(q) == len(prefix) + 1 and q[:-1] == prefix and e[q[-1]] != NEG:
                    stay[q][1] = O.logaddexp(stay[q][1], e[q[-1]], dtype)[()]
                    e[q[-1]] = NEG
        cands = []
        for prefix, (spb, spnb) in stay.items():
            tot = O.logaddexp(spb, spnb, dtype)[()]
            if tot != NEG:
                cands.append((rank_of(tot, prefix), prefix, spb, spnb))
        E = np.stack([e for _, e in exts])
        R = np.full(E.shape, NEG, dtype=dtype)
        Lm = np.stack([lm_ext(prefix) for prefix, _ in exts]) if rows is not None else None
        for i, (prefix, e) in enumerate(exts):   # every live extension, with the fused rank
            r = (e[: C - 1] + beta * dtype(len(prefix) + 1)).astype(dtype)
            if rows is not None:
                r = (r + (lm_alpha * Lm[i]).astype(dtype)).astype(dtype)
            R[i, : C - 1] = (r + (boost_alpha * bt.row(prefix).astype(dtype)).astype(dtype)).astype(dtype)
        R[E == NEG] = NEG
        n_ext = int((E != NEG).sum())
        flat = R.ravel()
        top = np.argsort(-flat, kind="stable")[: min(n_ext, W + 1)]
        for f in top:
            i, c = divmod(int(f), C)
            q = exts[i][0] + (c,)
            if rows is not None:
                lm[q] = dtype(Lm[i, c])
            cands.append((dtype(flat[f]), q, dtype(NEG), dtype(E[i, c])))
        n_cand = len(cands) - len(top) + n_ext
        cands.sort(key=lambda x: (-x[0], x[1]))
        min_cand = n_cand if min_cand is None else min(min_cand, n_cand)
        if len(cands) > W:
            margin = min(margin, float(cands[W - 1][0]) - float(cands[W][0]))
        beams = {p: (pb, pnb) for _, p, pb, pnb in cands[:W]}
    search = []
    for prefix, (pb, pnb) in beams.items():
        search.append((prefix, rank_of(O.logaddexp(pb, pnb, dtype)[()], prefix)))
    search.sort(key=lambda x: (-x[1], x[0]))
    final = [(p, dtype(r + dtype(boost_alpha * dtype(-bt.of(p)[1]))), slot) for slot, (p, r) in enumerate(search)]
    final.sort(key=lambda x: (-x[1], x[2]))
    return dict(nbest=[(p, s) for p, s, _ in final], search=search, pending={p: bt.of(p)[1] for p, _ in search},
                complete={p: bt.of(p)[0] for p, _ in search}, margin=margin, min_candidates=min_cand if min_cand is not None else 0)


def collapse(path, blank):
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(int(c))
        prev = c
    return out


def make_phrases(T, C, seeds=range(24)):
    """the phrase set of a shape, from its inputs: of the collapsed arg-max path of each `O.make_logp(seed, T, C)` two random runs
    of 1..4 tokens; for every fourth phrase a sibling that differs in the last token; for every fifth of length >= 2 its nested
    prefix without the last token; for every sixth an overlap: a phrase that starts with the last token of that one"""
    rng = np.random.default_rng(4242 + 31 * T + C)
    V = C - 1
    base = []
    for s in seeds:
        path = collapse(O.make_logp(s, T, C).argmax(axis=1).tolist(), C - 1)
        for _ in range(2):
            if not path:
                continue
            n = int(rng.integers(1, 5))
            a = int(rng.integers(0, max(1, len(path) - n + 1)))
            base.append(tuple(path[a:a + n]))
    out = list(base)
    for k, p in enumerate(base):
        if k % 4 == 0:
            out.append(p[:-1] + ((p[-1] + 1 + int(rng.integers(V - 1))) % V,) if V > 1 else p)
        if k % 5 == 0 and len(p) >= 2:
            out.append(p[:-1])
        if k % 6 == 0:
            out.append((p[-1],) + tuple(int(c) for c in rng.integers(0, V, size=int(rng.integers(1, 3)))))
    return dedup(out)
