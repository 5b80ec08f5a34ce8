"""Oracle of the CTC prefix beam search with n-gram fusion (`mi355x_ctc_beam_decode_lm`; include/mi355x_asr.h states it): the
search of tests/ctc_beam_oracle.py over token tuples with rank = (tot + beta * len) + alpha * lm(prefix), and an n-gram model that
shares nothing with nemo_amd/modules/ngram_lm.py: a dict from n-gram tuple to (log10 p, log10 backoff), scored by the textbook
back-off recursion on tuples.  There is no automaton here.

`cond_logp` is that recursion as written in the ARPA definition, one value at a time, float64.  `cond_row` gives the same values
for every label of a context at once (the search needs beam * C of them per frame) and, in float32, restates the device's
arithmetic: the back-off weights are summed from the longest context down and the probability is added last.  Values are
float64(file value) * ln 10 in float64 and that product rounded to float32 in float32, which is what the tables of the device hold.
Also here: the generator of the test models and the ARPA writer."""
import math

import numpy as np

import ctc_beam_oracle as O

NEG = -np.inf
BOS = -1
LN10 = math.log(10.0)


def make_lm(seed, V, order):
    rng = np.random.default_rng(1000 + seed)
    ng = {}
    for c in range(V):
        ng[(c,)] = [float(-rng.uniform(0.3, 3.0)), 0.0]
    ng[(BOS,)] = [-99.0, 0.0]
    prev = [k for k in ng]
    for n in range(2, order + 1):
        cnt = min(4 * V, (V * V) // 2) if n == 2 else max(V, (4 * V) >> (n - 2))
        cur, tries = [], 0
        while len(cur) < cnt and tries < 20 * cnt:
            tries += 1
            ctx = prev[int(rng.integers(len(prev)))]
            g = ctx + (int(rng.integers(V)),)
            if g in ng: continue
            ng[g] = [float(-rng.uniform(0.05, 2.5)), 0.0]
            cur.append(g)
        prev = cur
    for g in ng:
        if len(g) < order:
            ng[g][1] = float(rng.uniform(-1.0, 0.3))   # positive back-offs occur: lm_ub matters
    return ng


def context_of(prefix, order):
    """the last order-1 tokens of <s> followed by the prefix"""
    return ((BOS,) + tuple(prefix))[-(order - 1):] if order > 1 else ()


def cond_logp(ng, ctx, c):
    """ln p(c | ctx), float64, the ARPA definition: the n-gram's probability where the file has ctx.c, else backoff(ctx) (0 for a
    ctx the file does not have) + ln p(c | ctx[1:]); the unigrams end it"""
    g = tuple(ctx) + (c,)
    if g in ng:
        return ng[g][0] * LN10
    if not ctx:
        raise KeyError(f"label {c} has no unigram")
    return (ng[tuple(ctx)][1] * LN10 if tuple(ctx) in ng else 0.0) + cond_logp(ng, tuple(ctx)[1:], c)


def lm_score(ng, order, ids):
    """lm(ids) in float64: the sum of the conditional log-probabilities, no </s> term"""
    return sum(cond_logp(ng, context_of(ids[:k], order), int(c)) for k, c in enumerate(ids))


class _Rows:
    """cond_row for one model and dtype, cached per context"""

    def __init__(self, ng, order, V, dtype):
        self.ng, self.order, self.V, self.dtype = ng, order, V, dtype
        self.succ = {}
        for g, (lp, _) in ng.items():
            if g != (BOS,):
                self.succ.setdefault(g[:-1], []).append((g[-1], self.value(lp)))
        self.rows = {}

    def value(self, log10):
        v = float(log10) * LN10
        return v if self.dtype is np.float64 else np.float32(v)

    def cond_row(self, ctx):
        """[V] values of ln p(c | ctx) in dtype: for each c the number of back-off steps to the longest suffix of ctx that has c,
        the back-off weights summed in that order, the probability added last"""
        if ctx not in self.rows:
            K, dt = len(ctx), self.dtype
            depth = np.full(self.V, K, dtype=np.int64)
            logp = np.zeros(self.V, dtype=dt)
            found = np.zeros(self.V, dtype=bool)
            for k in range(K, -1, -1):   # the shortest suffix first: longer ones overwrite
                for c, v in self.succ.get(ctx[k:], ()):
                    depth[c], logp[c], found[c] = k, v, True
            assert found.all()   # every label has a unigram
            acc = [dt(0.0)]
            for k in range(K):
                acc.append(dt(acc[-1] + (self.value(self.ng[ctx[k:]][1]) if ctx[k:] in self.ng else dt(0.0))))
            self.rows[ctx] = (np.asarray(acc, dtype=dt)[depth] + logp).astype(dt)
        return self.rows[ctx]


def beam_search_lm(lp, blank, W, theta=np.inf, beta=0.0, alpha=0.0, ng=None, order=1, dtype=np.float64):
    """`O.beam_search` with rank = dtype(dtype(tot + beta * len) + alpha * lm(prefix)); the same dict(nbest, margin, min_candidates)"""
    lp32 = np.asarray(lp, dtype=np.float32)
    T, C = lp32.shape
    assert blank == C - 1
    lpd = lp32.astype(dtype)
    beta, alpha = dtype(beta), dtype(alpha)
    rows = _Rows(ng, order, C - 1, dtype)
    lm = {(): dtype(0.0)}   # prefix -> lm(prefix) in dtype; a function of the prefix alone

    def lm_ext(prefix):   # [C-1]: lm(prefix . c)
        return (lm[prefix] + rows.cond_row(context_of(prefix, order))).astype(dtype)

    def rank_of(tot, prefix):
        return dtype(dtype(tot + beta * dtype(len(prefix))) + dtype(alpha * lm[prefix]))

    beams = {(): (dtype(0.0), dtype(NEG))}   # prefix -> (pb, pnb)
    margin, min_cand = np.inf, None
    for t in range(T):
        ok = O.considered(lp32[t], theta)
        row = lpd[t]
        stay = {}
        exts = []   # (prefix, ext pnb over the classes, -inf where there is none)
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
        for prefix, e in exts:   # an extension that IS a prefix of the set: merged into that prefix's stay
            for q in stay:
                if len(q) == len(prefix) + 1 and q[:-1] == prefix and e[q[-1]] != NEG:
                    stay[q][1] = O.logaddexp(stay[q][1], e[q[-1]], dtype)[()]
                    e[q[-1]] = NEG
        cands = []   # (rank, prefix, pb, pnb)
        for prefix, (spb, spnb) in stay.items():
            tot = O.logaddexp(spb, spnb, dtype)[()]
            if tot != NEG:
                cands.append((rank_of(tot, prefix), prefix, spb, spnb))
        # of the extensions only the W + 1 of the largest rank can matter to the selection and to the margin: tuples for those only
        E = np.stack([e for _, e in exts])
        L = np.stack([lm_ext(prefix) for prefix, _ in exts])   # [beams, C-1]
        R = np.full(E.shape, NEG, dtype=dtype)
        for i, (prefix, e) in enumerate(exts):
            R[i, : C - 1] = ((e[: C - 1] + beta * dtype(len(prefix) + 1)).astype(dtype) + (alpha * L[i]).astype(dtype)).astype(dtype)
        R[E == NEG] = NEG
        n_ext = int((E != NEG).sum())
        flat = R.ravel()
        top = np.argsort(-flat, kind="stable")[: min(n_ext, W + 1)]
        for f in top:
            i, c = divmod(int(f), C)
            q = exts[i][0] + (c,)
            lm[q] = dtype(L[i, c])
            cands.append((dtype(flat[f]), q, dtype(NEG), dtype(E[i, c])))
        n_cand = len(cands) - len(top) + n_ext
        cands.sort(key=lambda x: (-x[0], x[1]))
        min_cand = n_cand if min_cand is None else min(min_cand, n_cand)
        if len(cands) > W:
            margin = min(margin, float(cands[W - 1][0]) - float(cands[W][0]))
        beams = {p: (pb, pnb) for _, p, pb, pnb in cands[:W]}
    out = []
    for prefix, (pb, pnb) in beams.items():
        tot = O.logaddexp(pb, pnb, dtype)[()]
        out.append((prefix, rank_of(tot, prefix)))
    out.sort(key=lambda x: (-x[1], x[0]))
    return dict(nbest=out, margin=margin, min_candidates=min_cand if min_cand is not None else 0)


def write_arpa(ng, path, token_offset=100, vocabulary=None):
    """the model as ARPA text: log10 p <TAB> words separated by one space [<TAB> log10 backoff]; a label is chr(id + token_offset),
    or vocabulary[id] with token_offset=None; <s> for BOS"""
    def word(i):
        return "<s>" if i == BOS else (chr(i + token_offset) if token_offset is not None else vocabulary[i])
    order = max(len(g) for g in ng)
    by_len = {n: [g for g in ng if len(g) == n] for n in range(1, order + 1)}
    with open(path, "w", encoding="utf-8", newline="\n") as f:
        f.write("\\data\\\n")
        for n in range(1, order + 1):
            f.write(f"ngram {n}={len(by_len[n])}\n")
        for n in range(1, order + 1):
            f.write(f"\n\\{n}-grams:\n")
            for g in by_len[n]:
                lp, bo = ng[g]
                tail = f"\t{bo!r}" if n < order else ""
                f.write(f"{lp!r}\t{' '.join(word(i) for i in g)}{tail}\n")
        f.write("\n\\end\\\n")
