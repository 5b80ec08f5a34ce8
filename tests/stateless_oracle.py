"""TEST INFRASTRUCTURE ONLY -- plain numpy restatement of the stateless prediction network's rule (include/mi355x_asr.h,
mi355x_stateless_*) in `dtype` (float64: the oracle; float32: its own rounding error): training forward, embedding gradient,
prediction tables and the greedy search (RNN-T and TDT, with a state in and out).  `bf16=True` rounds the two MFMA operands the rule
names (emb_i in the tables, relu(enc_proj + gp) in the joint) to bf16, round to nearest even.  No device code."""
import numpy as np


def bf16_round(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def widths(E, C):
    return [E - (C - 1) * (E // 2 // C)] + [E // 2 // C] * (C - 1)


def _labels(targets, i, blank):
    """[B, U1]: the label table i sees at every position of s = [blank, y_0, ...]; -1 where it sees nothing or a blank"""
    B, U = targets.shape
    s = np.concatenate([np.full((B, 1), blank), targets], 1)
    lab = np.full((B, U + 1), -1)
    lab[:, i:] = s[:, :U + 1 - i]
    lab[lab == blank] = -1
    return lab


def forward(embs, targets, blank):   # -> g [B, U1, E] float64
    labs = [_labels(targets, i, blank) for i in range(len(embs))]
    return np.concatenate([np.where(l[..., None] >= 0, e.astype(np.float64)[np.maximum(l, 0)], 0.0) for l, e in zip(labs, embs)], 2)


def embed_grad(embs, targets, dg, blank, dtype=np.float64):
    """-> [d emb_i], summed in (b, u) order in `dtype`"""
    out, off = [], 0
    for i, e in enumerate(embs):
        lab, g = _labels(targets, i, blank), np.zeros(e.shape, dtype)
        for b, u in zip(*np.nonzero(lab >= 0)):   # row-major: the (b, u) order of the rule
            g[lab[b, u]] = g[lab[b, u]] + dg[b, u, off:off + e.shape[1]].astype(dtype)
        out.append(g)
        off += e.shape[1]
    return out


def tables(embs, w_pred, blank, dtype=np.float64, bf16=False):
    """-> P [C, V1, J] in `dtype`; w_pred [J, E] holds the values of its image"""
    P, off = [], 0
    for e in embs:
        a = (bf16_round(e) if bf16 else e).astype(dtype)
        P.append(a @ w_pred[:, off:off + e.shape[1]].astype(dtype).T)
        P[-1][blank] = 0
        off += e.shape[1]
    return np.stack(P)


def search(P, b_pred, w_out, b_out, f, length, blank, max_symbols, max_out, durations=None, dtype=np.float64, bf16=False, state=None):
    """one stream (or one chunk of it: `state` = the dict a previous call returned) -> dict(tok, fr, score, gap, state); gap = the
    smallest top-two gap met among the label logits (TDT: and the duration logits)"""
    C, V1, _ = P.shape
    P, b_pred, w_out, b_out, f = (np.asarray(x).astype(dtype) for x in (P, b_pred, w_out, b_out, f))
    st = dict(state) if state else dict(ctx=[blank] * C, score=dtype(0), fd=0, sym=0, skip=0)
    ctx, score, fd, tdt = list(st["ctx"]), dtype(st["score"]), st["fd"], durations is not None
    tok, fr, res = [], [], dict(n=0, gap=np.inf)

    def step(t):
        gp = P[0, ctx[0]]
        for i in range(1, C):
            gp = gp + P[i, ctx[i]]
        a = np.maximum(f[t] + (gp + b_pred), 0)
        lg = w_out @ (bf16_round(a).astype(dtype) if bf16 else a) + b_out
        for part in (lg[:V1], lg[V1:]) if tdt else (lg[:V1],):
            top = np.sort(part)[-2:]
            res["gap"] = min(res["gap"], float(top[1] - top[0]))
        k = int(np.argmax(lg[:V1]))
        lp = -np.log(np.sum(np.exp(lg[:V1] - lg[k])))
        return k, lp, (durations[int(np.argmax(lg[V1:]))] if tdt else 0)

    def emit(k, lp, t):
        nonlocal score, ctx
        if res["n"] < max_out:
            tok.append(k); fr.append(fd + t)
        res["n"], score, ctx = res["n"] + 1, dtype(score + lp), [k] + ctx[:-1]

    skip, sym = 0, 0
    if tdt:
        t, sym = st["skip"], st["sym"]
        while t < length and res["n"] < max_out:
            k, lp, d = step(t)
            if k == blank:
                t, sym = t + max(d, 1), 0
            else:
                emit(k, lp, t)
                sym = sym + 1 if d == 0 else 0
                if d == 0 and max_symbols > 0 and sym >= max_symbols:
                    d, sym = 1, 0
                t += d
        skip = max(t - length, 0)
    else:
        for t in range(length):
            s = 0
            while s < max_symbols if max_symbols > 0 else res["n"] < max_out:
                k, lp, _ = step(t)
                if k == blank:
                    break
                emit(k, lp, t)
                s += 1
    return dict(tok=tok, fr=fr, score=score, gap=res["gap"], state=dict(ctx=ctx, score=score, fd=fd + length, sym=sym, skip=skip))
