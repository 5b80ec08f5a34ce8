"""Plain numpy restatement of the fused transducer beam search's rule (include/mi355x_asr.h, mi355x_transducer_beam_decode_fused) in
`dtype`: the search of tests/rnnt_beam_oracle.py (same fields of the result, same `margin` and `ranks`) where every label
candidate of a live hypothesis gains dtype(alpha * ln p(label | context)), the context being the last order-1 tokens of <s>
followed by the hypothesis' tokens.  The model is the n-gram dict of tests/ctc_beam_lm_oracle.py scored by its back-off recursion
on tuples (`_Rows.cond_row`: float64, or the float32 arithmetic the rule states); there is no automaton here.
`depth`: the longest back-off chain a scored hypothesis had -- the non-empty suffixes of its context that the file holds."""
import numpy as np

import ctc_beam_lm_oracle as L
from rnnt_beam_oracle import bf16_round


def beam_search_lm(m, f, length, W, blank, max_symbols, max_out, ng, order, alpha, durations=None, dtype=np.float64, bf16=False):
    one = np.dtype(dtype).type(1)
    rnd = (lambda x: bf16_round(x).astype(dtype)) if bf16 else (lambda x: x)
    w = {k: np.asarray(v, dtype) for k, v in m.items()}
    V1, H = w["emb"].shape
    assert blank == V1 - 1
    D = len(durations) if durations else 0
    rows, alpha = L._Rows(ng, order, V1 - 1, dtype), dtype(alpha)
    sig = lambda x: one / (one + np.exp(-x))
    lse = lambda x: x.max() + np.log(np.exp(x - x.max()).sum(dtype=dtype))

    def pred(x, h, c):
        z = ((w["w_hh"] @ rnd(h) + w["b_hh"]) + w["w_ih"] @ rnd(x)) + w["b_ih"]
        c2 = sig(z[H:2 * H]) * c + sig(z[:H]) * np.tanh(z[2 * H:3 * H])
        h2 = sig(z[3 * H:]) * np.tanh(c2)
        return h2, c2, w["w_pred"] @ rnd(h2) + w["b_pred"]

    zero = np.zeros(H, dtype)
    beam = [dict(tok=(), fr=(), t=0, score=one * 0, st=pred(zero, zero, zero), sym=0)] + [None] * (W - 1)
    margin, merges, ranks, depth = np.inf, 0, [], 0
    vo = np.where(np.arange(V1) == blank, 0, np.arange(V1) + 1)
    for _ in range(length + max_out):
        if not any(b is not None and b["t"] < length for b in beam):
            break
        CS, PAR, ORD = [], [], []
        for s, b in enumerate(beam):
            if b is None:
                continue
            if b["t"] >= length:   # finished: offers itself, no LM term
                cs, od = np.array([b["score"]]), np.array([0])
            else:
                lg = w["w_out"] @ rnd(np.maximum(np.asarray(f[b["t"]], dtype) + b["st"][2], 0)) + w["b_out"]
                lpf = lg[:V1] - lse(lg[:V1])
                ctx = L.context_of(b["tok"], order)
                depth = max(depth, sum(ctx[k:] in ng for k in range(len(ctx))))
                lpf[:V1 - 1] = lpf[:V1 - 1] + (alpha * rows.cond_row(ctx)).astype(dtype)   # the blank (last) gets no term
                gain = lpf[:, None] + ((lg[V1:] - lse(lg[V1:]))[None, :] if D else 0)
                cs = b["score"] + gain
                od = vo[:, None] * 8 + np.arange(gain.shape[1])[None, :]
                ok = cs > -np.inf
                if len(b["tok"]) >= max_out or (not D and max_symbols > 0 and b["sym"] >= max_symbols):
                    ok &= (np.arange(V1) == blank)[:, None]
                cs, od = cs[ok], od[ok]
            CS.append(cs); PAR.append(np.full(cs.shape, s)); ORD.append(od)
        CS, PAR, ORD = np.concatenate(CS), np.concatenate(PAR), np.concatenate(ORD)
        order_ = np.lexsort((ORD, PAR, -CS))
        if len(order_) > W:
            margin = min(margin, float(CS[order_[W - 1]] - CS[order_[W]]))
        new = []
        for k in order_[:W]:
            b, cs, vi, i = beam[PAR[k]], CS[k], ORD[k] // 8, ORD[k] % 8
            own = np.sort(CS[PAR == PAR[k]])[::-1]
            if len(own) > 1:
                margin = min(margin, float(own[0] - own[1]))
            ranks.append(float(cs))
            if b["t"] >= length:
                new.append(dict(b, x=None))
                continue
            v = blank if vi == 0 else vi - 1
            if D:
                d = durations[i]
                sym = 0 if v == blank or d else b["sym"] + 1
                if v == blank:
                    d = max(d, 1)
                elif d == 0 and max_symbols > 0 and sym >= max_symbols:
                    d, sym = 1, 0
                t = b["t"] + d
            else:
                t, sym = (b["t"] + 1, 0) if v == blank else (b["t"], b["sym"] + 1)
            lab = v != blank
            new.append(dict(tok=b["tok"] + ((v,) if lab else ()), fr=b["fr"] + ((b["t"],) if lab else ()), t=t, score=cs,
                            st=b["st"], sym=sym, x=v if lab else None))
        for k in range(len(new)):   # merge into the best-ranked equal hypothesis, in rank order
            for j in range(k):
                if new[j] is not None and new[j]["tok"] == new[k]["tok"] and new[j]["t"] == new[k]["t"]:
                    a, c = new[j]["score"], new[k]["score"]
                    margin = min(margin, ranks[len(ranks) - len(new) + j] - float(c))
                    hi, lo = max(a, c), min(a, c)
                    new[j]["score"] = hi + np.log1p(np.exp(lo - hi))
                    new[k], merges = None, merges + 1
                    break
        for b in new:   # advance
            if b is not None and b["x"] is not None:
                b["st"] = pred(w["emb"][b["x"]], b["st"][0], b["st"][1])
        beam = new + [None] * (W - len(new))
    live = sorted((b for b in beam if b is not None), key=lambda b: -b["score"])   # (stable: ties stay in slot order)
    for a, b in zip(live, live[1:]):
        margin = min(margin, float(a["score"] - b["score"]))
    ranks += [float(b["score"]) for b in live]
    return dict(nbest=[(b["tok"], b["fr"], float(b["score"])) for b in live], margin=margin, merges=merges, ranks=ranks, depth=depth)
