"""float64 oracle of the Token-and-Duration Transducer (TDT) objective and a Python restatement of its greedy search, for
tests/test_tdt_host.py and tests/test_tdt_gpu.py.

Lattice cells (t, u), 0 <= t < T, 0 <= u <= U; joint logit rows z(t, u) of width V1 + D (V1 label logits with the blank among
them, then D duration logits).  Blank arcs of duration d >= 1: (t, u) -> (t + d, u); label arcs y_{u+1}: (t, u) -> (t + d, u + 1)
with t + d < T; a path ends with a blank arc landing exactly on (T, U).  Arc weight = lp(label) + dp(duration) - sigma."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

NEG = -np.inf


def _lse(v):
    v = np.asarray(v, dtype=np.float64)
    if v.size == 0:
        return NEG
    m = v.max()
    return NEG if m == NEG else m + np.log(np.exp(v - m).sum())


def arc_weights(z, labels, U, durations, blank, sigma):
    """z [T, U1, V1 + D] float64 -> wb, wl [T, U1, D] (blank / label arc weights, -inf where no arc), lp, dp"""
    D = len(durations)
    V1 = z.shape[-1] - D
    lp = z[..., :V1] - np.log(np.exp(z[..., :V1] - z[..., :V1].max(-1, keepdims=True)).sum(-1, keepdims=True)) \
        - z[..., :V1].max(-1, keepdims=True)
    zd = z[..., V1:]
    dp = zd - zd.max(-1, keepdims=True) - np.log(np.exp(zd - zd.max(-1, keepdims=True)).sum(-1, keepdims=True))
    dur = np.asarray(durations)
    wb = np.where(dur[None, None, :] >= 1, lp[..., blank:blank + 1] + dp - sigma, NEG)
    wl = np.full(wb.shape, NEG)
    for u in range(U):
        wl[:, u, :] = lp[:, u, labels[u]][:, None] + dp[:, u, :] - sigma
    return wb, wl, lp, dp


def lattice(z, labels, T, U, durations, blank, sigma):
    """one utterance: z [>= T, >= U + 1, V1 + D] -> alpha, beta [T, U + 1], ll (forward), ll (backward), wb, wl"""
    z = np.asarray(z, dtype=np.float64)[:T, :U + 1]
    wb, wl, _, _ = arc_weights(z, labels, U, durations, blank, sigma)
    alpha = np.full((T, U + 1), NEG)
    for t in range(T):
        for u in range(U + 1):
            if t == 0 and u == 0:
                alpha[t, u] = 0.0
                continue
            terms = []
            for i, d in enumerate(durations):
                if t - d < 0:
                    continue
                if d >= 1:
                    terms.append(alpha[t - d, u] + wb[t - d, u, i])
                if u >= 1:
                    terms.append(alpha[t - d, u - 1] + wl[t - d, u - 1, i])
            alpha[t, u] = _lse(terms)
    ll_f = _lse([alpha[T - d, U] + wb[T - d, U, i] for i, d in enumerate(durations) if d >= 1 and T - d >= 0])
    beta = np.full((T, U + 1), NEG)
    for t in range(T - 1, -1, -1):
        for u in range(U, -1, -1):
            terms = []
            for i, d in enumerate(durations):
                if d >= 1:
                    if t + d < T:
                        terms.append(beta[t + d, u] + wb[t, u, i])
                    elif t + d == T and u == U:
                        terms.append(wb[t, u, i])
                if u < U and t + d < T:
                    terms.append(beta[t + d, u + 1] + wl[t, u, i])
            beta[t, u] = _lse(terms)
    return alpha, beta, ll_f, beta[0, 0], wb, wl


def grad_closed_form(z, labels, T, U, durations, blank, sigma):
    """one utterance: (cost = -ll, d cost / d z [T, U + 1, V1 + D]) by the closed form (arc posteriors and cell occupancy)"""
    z = np.asarray(z, dtype=np.float64)[:T, :U + 1]
    alpha, beta, ll, _, wb, wl = lattice(z, labels, T, U, durations, blank, sigma)
    D = len(durations)
    V1 = z.shape[-1] - D
    sm = np.exp(z[..., :V1] - z[..., :V1].max(-1, keepdims=True))
    sm /= sm.sum(-1, keepdims=True)
    smd = np.exp(z[..., V1:] - z[..., V1:].max(-1, keepdims=True))
    smd /= smd.sum(-1, keepdims=True)
    g = np.zeros_like(z)
    for t in range(T):
        for u in range(U + 1):
            occ = np.exp(alpha[t, u] + beta[t, u] - ll)
            pb, pl = np.zeros(D), np.zeros(D)
            for i, d in enumerate(durations):
                if d >= 1:
                    bd = beta[t + d, u] if t + d < T else (0.0 if (t + d == T and u == U) else NEG)
                    pb[i] = np.exp(alpha[t, u] + wb[t, u, i] + bd - ll)
                if u < U and t + d < T:
                    pl[i] = np.exp(alpha[t, u] + wl[t, u, i] + beta[t + d, u + 1] - ll)
            g[t, u, :V1] = sm[t, u] * occ
            g[t, u, blank] -= pb.sum()
            if u < U:
                g[t, u, labels[u]] -= pl.sum()
            g[t, u, V1:] = smd[t, u] * occ - (pb + pl)
    return -ll, g


def enumerate_paths(T, U, durations):
    """every complete path as a list of arcs (t, u, kind, i) with kind 0 = blank, 1 = label"""
    out = []

    def walk(t, u, arcs):
        for i, d in enumerate(durations):
            if d >= 1:
                if t + d < T:
                    walk(t + d, u, arcs + [(t, u, 0, i)])
                elif t + d == T and u == U:
                    out.append(arcs + [(t, u, 0, i)])
            if u < U and t + d < T:
                walk(t + d, u + 1, arcs + [(t, u, 1, i)])

    walk(0, 0, [])
    return out


def brute_force(z, labels, T, U, durations, blank, sigma):
    """(cost, d cost / d z) by enumerating every path, differentiated by torch autograd in float64"""
    D = len(durations)
    zt = torch.tensor(np.asarray(z, dtype=np.float64)[:T, :U + 1], requires_grad=True)
    V1 = zt.shape[-1] - D
    lp = torch.log_softmax(zt[..., :V1], -1)
    dp = torch.log_softmax(zt[..., V1:], -1)
    scores = []
    for path in enumerate_paths(T, U, durations):
        s = zt.new_zeros(())
        for t, u, kind, i in path:
            s = s + (lp[t, u, blank] if kind == 0 else lp[t, u, labels[u]]) + dp[t, u, i] - sigma
        scores.append(s)
    cost = -torch.logsumexp(torch.stack(scores), 0)
    cost.backward()
    return cost.item(), zt.grad.numpy()


def tdt_loss_and_grad(acts, labels, act_lens, label_lens, durations, blank, sigma=0.0, reduction="mean"):
    """batch [B, T, U1, V1 + D] -> (costs: [B] for 'none', else the reduced [1]; the gradient of the reduced cost w.r.t. acts
    ('none': of the per-utterance costs with an upstream gradient of 1), zero beyond every utterance's cells), float64 torch"""
    a = acts.double().numpy()
    B = a.shape[0]
    costs = np.zeros(B)
    grads = np.zeros_like(a)
    for b in range(B):
        T, U = int(act_lens[b]), int(label_lens[b])
        c, g = grad_closed_form(a[b], labels[b].tolist(), T, U, durations, blank, sigma)
        costs[b] = c
        grads[b, :T, :U + 1] = g
    if reduction == "none":
        return torch.from_numpy(costs), torch.from_numpy(grads)
    if reduction == "mean":
        return torch.tensor([costs.mean()]), torch.from_numpy(grads / B)
    return torch.tensor([costs.sum()]), torch.from_numpy(grads)


def tdt_greedy_decode(Pd, Pj, enc, enc_len, blank, durations, max_symbols=10, f_all=None, max_out=None):
    """The greedy TDT search, utterance by utterance (fp32 torch on the CPU):
        t = 0, last = blank, state = 0, same = 0
        while t < T_b:  z = out(relu(f[t] + pred_proj(pred(emb[last], state)))); k = argmax z[:V1]; d = durations[argmax z[V1:]]
            blank: t += max(d, 1), same = 0
            else:  emit (k, t), commit the state, last = k; same = same + 1 if d == 0 else 0;
                   a run of max_symbols labels of duration 0 moves on by one frame; t += d
    stopping once max_out labels are out.  -> list of (tokens, frame indices)"""
    emb = Pd["prediction.embed.weight"]
    q = "prediction.dec_rnn.lstm."
    w_ih, w_hh, b_ih, b_hh = (Pd[q + n + "_l0"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
    out = [k[:-len("weight")] for k in Pj if k.startswith("joint_net.") and k.endswith(".weight")][0]
    if f_all is None:
        f_all = F.linear(enc.transpose(1, 2), Pj["enc.weight"], Pj["enc.bias"])
    H = w_hh.shape[1]
    D = len(durations)
    V1 = Pj[out + "weight"].shape[0] - D
    T = enc.shape[2]
    cap = max_out if max_out is not None else (T * max_symbols if max_symbols else 4 * T)

    def pred(last, h, c):
        x = emb[last]
        zz = F.linear(x, w_ih, b_ih) + F.linear(h, w_hh, b_hh)
        i, f, g, o = zz[:H], zz[H:2 * H], zz[2 * H:3 * H], zz[3 * H:]
        c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h2 = torch.sigmoid(o) * torch.tanh(c2)
        return F.linear(h2, Pj["pred.weight"], Pj["pred.bias"]), h2, c2

    hyps = []
    for b in range(enc.shape[0]):
        h, c = torch.zeros(H), torch.zeros(H)
        toks, times = [], []
        gp, hn, cn = pred(blank, h, c)
        t, same = 0, 0
        while t < int(enc_len[b]) and len(toks) < cap:
            z = F.linear(torch.relu(f_all[b, t] + gp), Pj[out + "weight"], Pj[out + "bias"])
            k = int(torch.argmax(z[:V1]))
            d = durations[int(torch.argmax(z[V1:]))]
            if k == blank:
                t += max(d, 1)
                same = 0
            else:
                toks.append(k); times.append(t)
                h, c = hn, cn
                gp, hn, cn = pred(k, h, c)
                same = same + 1 if d == 0 else 0
                if d == 0 and max_symbols and same >= max_symbols:
                    d, same = 1, 0
                t += d
        hyps.append((toks, times))
    return hyps
