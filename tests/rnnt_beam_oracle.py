"""Plain numpy restatement of the transducer beam search's rule (include/mi355x_asr.h, mi355x_transducer_beam_decode) in `dtype`
(float64: the reference; float32: the reference's own rounding error).  `bf16=True` rounds the activation operands of the four
contractions (h, emb[v], h', relu(enc_proj + gp)) to bf16, as the kernel does with the bf16 weight images.

`margin` is the smallest decision margin met: per step rank[W-1] - rank[W] over all candidates; for every parent with a selected
candidate the gap between its best and second-best candidate; the score gap that decides a merge's survivor; and the gaps of the
final best-first order.  `ranks` lists every selected candidate's score, step by step, then the final scores."""
import numpy as np


def bf16_round(x):
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def beam_search(m, f, length, W, blank, max_symbols, max_out, durations=None, dtype=np.float64, bf16=False):
    """m: emb [V1, H], w_ih, w_hh [4H, H], b_ih, b_hh, w_pred [J, H], b_pred, w_out [V1 + D, J], b_out; f: enc_proj [T, J]"""
    one = np.dtype(dtype).type(1)
    rnd = (lambda x: bf16_round(x).astype(dtype)) if bf16 else (lambda x: x)
    w = {k: np.asarray(v, dtype) for k, v in m.items()}
    V1, H = w["emb"].shape
    D = len(durations) if durations else 0
    sig = lambda x: one / (one + np.exp(-x))
    lse = lambda x: x.max() + np.log(np.exp(x - x.max()).sum(dtype=dtype))

    def pred(x, h, c):
        z = ((w["w_hh"] @ rnd(h) + w["b_hh"]) + w["w_ih"] @ rnd(x)) + w["b_ih"]
        c2 = sig(z[H:2 * H]) * c + sig(z[:H]) * np.tanh(z[2 * H:3 * H])
        h2 = sig(z[3 * H:]) * np.tanh(c2)
        return h2, c2, w["w_pred"] @ rnd(h2) + w["b_pred"]

    zero = np.zeros(H, dtype)
    beam = [dict(tok=(), fr=(), t=0, score=one * 0, st=pred(zero, zero, zero), sym=0)] + [None] * (W - 1)
    margin, merges, ranks = np.inf, 0, []
    vo = np.where(np.arange(V1) == blank, 0, np.arange(V1) + 1)
    for _ in range(length + max_out):
        if not any(b is not None and b["t"] < length for b in beam):
            break
        CS, PAR, ORD = [], [], []
        for s, b in enumerate(beam):
            if b is None:
                continue
            if b["t"] >= length:   # finished: offers itself
                cs, od = np.array([b["score"]]), np.array([0])
            else:
                lg = w["w_out"] @ rnd(np.maximum(np.asarray(f[b["t"]], dtype) + b["st"][2], 0)) + w["b_out"]
                lp = lg[:V1] - lse(lg[:V1])
                gain = lp[:, None] + ((lg[V1:] - lse(lg[V1:]))[None, :] if D else 0)
                cs = b["score"] + gain
                od = vo[:, None] * 8 + np.arange(gain.shape[1])[None, :]
                ok = cs > -np.inf
                if len(b["tok"]) >= max_out or (not D and max_symbols > 0 and b["sym"] >= max_symbols):
                    ok &= (np.arange(V1) == blank)[:, None]
                cs, od = cs[ok], od[ok]
            CS.append(cs); PAR.append(np.full(cs.shape, s)); ORD.append(od)
        CS, PAR, ORD = np.concatenate(CS), np.concatenate(PAR), np.concatenate(ORD)
        order = np.lexsort((ORD, PAR, -CS))
        if len(order) > W:
            margin = min(margin, float(CS[order[W - 1]] - CS[order[W]]))
        new = []
        for k in order[:W]:
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
            new.append(dict(tok=b["tok"] + ((v,) if lab else ()), fr=b["fr"] + ((b["t"],) if lab else ()), t=t, score=cs, cs=cs,
                            st=b["st"], sym=sym, x=v if lab else None))
        for k in range(len(new)):   # merge into the best-ranked equal hypothesis, in rank order
            for j in range(k):
                if new[j] is not None and new[j]["tok"] == new[k]["tok"] and new[j]["t"] == new[k]["t"]:
                    a, c = new[j]["score"], new[k]["score"]   # (nothing was merged into k: c is its candidate score)
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
    return dict(nbest=[(b["tok"], b["fr"], float(b["score"])) for b in live], margin=margin, merges=merges, ranks=ranks)
