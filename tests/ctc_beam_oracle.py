"""Oracle of the CTC prefix beam search (`mi355x_ctc_beam_decode`; include/mi355x_asr.h states the search): the same search over
token TUPLES -- the candidates of a frame are a dict keyed by prefix, so an extension that lands on a prefix of the current set is
merged with that prefix's stay by construction -- in float64, or in float32 (`dtype`) as the restatement of the device's arithmetic.
Token pruning is the same float32 subtract and compare in both.  Besides the n-best it returns the CUT MARGIN: the minimum over the
frames of rank[W-1] - rank[W] among that frame's sorted candidates (+inf where no frame had more than W candidates), i.e. how far
the selection was from going the other way, and the smallest number of candidates any frame had.  Also here: an exact CTC
log-likelihood in float64 and the generator of the test inputs."""
import numpy as np

NEG = -np.inf


def logaddexp(a, b, dtype=np.float64):
    """max + log1p(exp(-|a-b|)) in `dtype`, -inf handled; arrays or scalars"""
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    m = np.maximum(a, b)
    with np.errstate(invalid="ignore"):
        r = m + np.log1p(np.exp(-np.abs(a - b)))
    return np.where(m == NEG, dtype(NEG), r).astype(dtype)


def considered(row32, theta):
    """the classes of a frame that pass the token pruning: float32 subtract, float32 compare"""
    row32 = np.asarray(row32, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        lo = np.float32(row32.max()) - np.float32(theta)
    return row32 >= lo


def beam_search(lp, blank, W, theta=np.inf, beta=0.0, dtype=np.float64):
    """lp [T, C] float32 log-probabilities of ONE utterance -> dict(
         nbest = [(tokens tuple, rank)], best first (at most W),
         margin = the cut margin, min_candidates = the smallest number of candidates (tot > -inf) of any frame)"""
    lp32 = np.asarray(lp, dtype=np.float32)
    T, C = lp32.shape
    lpd = lp32.astype(dtype)
    beta = dtype(beta)
    beams = {(): (dtype(0.0), dtype(NEG))}   # prefix -> (pb, pnb)
    margin, min_cand = np.inf, None
    for t in range(T):
        ok = considered(lp32[t], theta)
        row = lpd[t]
        stay = {}
        exts = []   # (prefix, ext pnb over the classes, -inf where there is none)
        for prefix, (pb, pnb) in beams.items():
            tot = logaddexp(pb, pnb, dtype)[()]
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
                    stay[q][1] = logaddexp(stay[q][1], e[q[-1]], dtype)[()]
                    e[q[-1]] = NEG
        cands = []   # (rank, prefix, pb, pnb)
        for prefix, (spb, spnb) in stay.items():
            tot = logaddexp(spb, spnb, dtype)[()]
            if tot != NEG:
                cands.append((dtype(tot + beta * dtype(len(prefix))), prefix, spb, spnb))
        # of the extensions only the W + 1 of the largest rank can matter to the selection and to the margin: tuples for those only
        E = np.stack([e for _, e in exts])
        R = np.stack([(e + beta * dtype(len(prefix) + 1)).astype(dtype) for prefix, e in exts])
        R[E == NEG] = NEG
        n_ext = int((E != NEG).sum())
        flat = R.ravel()
        top = np.argsort(-flat, kind="stable")[: min(n_ext, W + 1)]
        for f in top:
            i, c = divmod(int(f), C)
            cands.append((dtype(flat[f]), exts[i][0] + (c,), dtype(NEG), dtype(E[i, c])))
        n_cand = len(cands) - len(top) + n_ext
        cands.sort(key=lambda x: (-x[0], x[1]))
        min_cand = n_cand if min_cand is None else min(min_cand, n_cand)
        if len(cands) > W:
            margin = min(margin, float(cands[W - 1][0]) - float(cands[W][0]))
        beams = {p: (pb, pnb) for _, p, pb, pnb in cands[:W]}
    out = []
    for prefix, (pb, pnb) in beams.items():
        tot = logaddexp(pb, pnb, dtype)[()]
        out.append((prefix, dtype(tot + beta * dtype(len(prefix)))))
    out.sort(key=lambda x: (-x[1], x[0]))
    return dict(nbest=out, margin=margin, min_candidates=min_cand if min_cand is not None else 0)


def ctc_loglik(lp, labels, blank):
    """exact log-probability of the label sequence under CTC, float64 (the alpha recursion over the blank-extended sequence)"""
    lp = np.asarray(lp, dtype=np.float64)
    T = lp.shape[0]
    ext = [blank]
    for l in labels:
        ext += [int(l), blank]
    S = len(ext)
    if T == 0:
        return 0.0 if not labels else NEG
    a = np.full(S, NEG)
    a[0] = lp[0, blank]
    if S > 1:
        a[1] = lp[0, ext[1]]
    for t in range(1, T):
        n = np.full(S, NEG)
        for s in range(S):
            v = a[s]
            if s >= 1:
                v = np.logaddexp(v, a[s - 1])
            if s >= 2 and ext[s] != blank and ext[s] != ext[s - 2]:
                v = np.logaddexp(v, a[s - 2])
            n[s] = v + lp[t, ext[s]] if v != NEG else NEG
        a = n
    return float(np.logaddexp(a[S - 1], a[S - 2]) if S > 1 else a[0])


def make_logp(seed, T, C, blank=None):
    """float32 log-probabilities [T, C] with a planted path: N(0,1) * 1.5, a random path (blank with probability 0.6, a uniform
    label otherwise) gets +5.0 on its class, log-softmax"""
    blank = C - 1 if blank is None else blank
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, C)) * 1.5
    labels = [c for c in range(C) if c != blank]
    for t in range(T):
        c = blank if rng.random() < 0.6 else labels[int(rng.integers(len(labels)))]
        x[t, c] += 5.0
    x = x - x.max(axis=1, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=1, keepdims=True))).astype(np.float32)
