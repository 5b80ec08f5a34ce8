"""Plain restatement of the multi-blank transducer's two rules (include/mi355x_asr.h): the loss as a torch lattice on the CPU whose gradient
comes from autograd, the greedy search in numpy.  float64 is the reference; a float32 run of the same code gives the tolerance."""
import numpy as np
import torch


def loss_and_grad(acts, labels, act_lens, label_lens, durations, sigma, dtype=torch.float64):
    """acts [B, T, U1, N] logits, the standard blank = N - 1, big blank i = N - 2 - i -> (costs [B], d sum(costs) / d acts)"""
    x = acts.detach().to(dtype).requires_grad_(True)
    lp = torch.log_softmax(x, -1) - sigma
    blank = x.shape[-1] - 1
    jumps = [(1, blank)] + [(d, blank - 1 - i) for i, d in enumerate(durations)]   # (frames, output) of every blank-like arc
    costs = []
    for b in range(x.shape[0]):
        Tb, Ub = int(act_lens[b]), int(label_lens[b])
        alpha = {(0, 0): lp.new_zeros(())}
        for t in range(Tb):
            for u in range(Ub + 1):
                arcs = [alpha[t, u - 1] + lp[b, t, u - 1, labels[b, u - 1]]] if u > 0 else []
                arcs += [alpha[t - d, u] + lp[b, t - d, u, o] for d, o in jumps if t - d >= 0]
                if arcs:
                    alpha[t, u] = torch.logsumexp(torch.stack(arcs), 0)
        costs.append(-torch.logsumexp(torch.stack([alpha[Tb - d, Ub] + lp[b, Tb - d, Ub, o] for d, o in jumps if Tb - d >= 0]), 0))
    costs = torch.stack(costs)
    costs.sum().backward()
    return costs.detach(), x.grad


def greedy(m, f, length, durations, max_symbols, dtype=np.float64):
    """m: the weights by name, w_out [V1 + nb, J]; f: enc_proj [T, J] -> tokens, frames, score, the smallest arg-max `margin`, `jumps`"""
    one = np.dtype(dtype).type(1)
    w = {k: np.asarray(v, dtype) for k, v in m.items()}
    V1, H = w["emb"].shape
    bo = V1 - 1 + len(durations)   # the standard blank's row
    sig = lambda x: one / (one + np.exp(-x))

    def pred(x, h, c):   # the LSTM step of tests/rnnt_beam_oracle.py
        z = ((w["w_hh"] @ h + w["b_hh"]) + w["w_ih"] @ x) + w["b_ih"]
        c2 = sig(z[H:2 * H]) * c + sig(z[:H]) * np.tanh(z[2 * H:3 * H])
        h2 = sig(z[3 * H:]) * np.tanh(c2)
        return h2, c2, w["w_pred"] @ h2 + w["b_pred"]

    h = c = np.zeros(H, dtype)
    h2, c2, gp = pred(h, h, c)
    t, sym, score, margin, tokens, frames, jumps = 0, 0, one * 0, np.inf, [], [], []
    while t < length:
        if sym >= max_symbols:
            t, sym = t + 1, 0
            continue
        lg = w["w_out"] @ np.maximum(np.asarray(f[t], dtype) + gp, 0) + w["b_out"]
        k = int(np.argmax(lg))
        top = np.sort(lg)
        margin = min(margin, float(top[-1] - top[-2]))
        if k == bo:
            t, sym = t + 1, 0
        elif k >= V1 - 1:
            d = durations[bo - 1 - k]
            jumps.append((t, d))
            t, sym = t + d, 0
        else:
            tokens.append(k); frames.append(t)
            score = score + (lg[k] - (lg.max() + np.log(np.exp(lg - lg.max()).sum(dtype=dtype))))
            h, c = h2, c2
            h2, c2, gp = pred(w["emb"][k], h, c)
            sym += 1
    return dict(tokens=tokens, frames=frames, score=float(score), margin=margin, jumps=jumps)
