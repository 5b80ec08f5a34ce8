"""TEST INFRASTRUCTURE ONLY -- CPU restatement of the greedy transducer search for a prediction network of L LSTM layers
(csrc/rnnt_decode.hip: mi355x_transducer_greedy_decode_layers, RNN-T and TDT, one-shot and resumable), torch, utterance by utterance.

tests/stream_decode_oracle.py restated for L layers: the same loops, the same state fields, with h / c of shape [L, H] and the
prediction step of include/mi355x_asr.h,
    z = W_ih[l] in_l + b_ih[l] + W_hh[l] h[l] + b_hh[l],   in_0 = emb[last], in_l = hn[l-1]      (torch gate order i, f, g, o)
    cn[l] = sigmoid(f) c[l] + sigmoid(i) tanh(g),   hn[l] = sigmoid(o) tanh(cn[l]),   gp = W_pred hn[L-1] + b_pred
(eval mode: no dropout between the layers; a label commits every layer).  At L = 1 it returns exactly what that file returns.

State dicts use the reference's keys (`prediction.dec_rnn.lstm.{weight,bias}_{ih,hh}_l{l}`).  Layer 0 and the joint of a random case
are `stream_decode_oracle.random_transducer(seed, ...)` unchanged; the upper layers come from a generator of their own
(`upper_layers`).  `forced_walk` is the checker of a device search whose arithmetic differs (rule 2 of tests/test_stream_decode_gpu.py);
`replay_confidence` gives the label distribution of every emitted label to tests/confidence_oracle.py."""
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor

from stream_decode_oracle import SMALL, random_transducer, recipe_enc, small_enc  # noqa: F401  (the tests take them from here)

Q = "prediction.dec_rnn.lstm."
DUR = [0, 1, 2, 3, 4]
RECIPE = dict(V=1024, H=640, D=512, J=640, T=40, lens=[40, 31, 0, 40, 17, 1], max_symbols=10)   # the recipe's widths, 40 frames


def n_layers(Pd) -> int:
    L = 0
    while Q + f"weight_ih_l{L}" in Pd:
        L += 1
    return L


def upper_layers(Pd, seed: int, L: int, scale: float):
    """Pd with layers 1 .. L-1 added: drawn in the order weight_ih, weight_hh, bias_ih, bias_hh per layer from a generator seeded
    seed * 1000 + 7, each uniform in +-scale / sqrt(H)"""
    H = Pd[Q + "weight_hh_l0"].shape[1]
    g2 = torch.Generator().manual_seed(seed * 1000 + 7)
    Pd = dict(Pd)
    for l in range(1, L):
        for name, shape in (("weight_ih", (4 * H, H)), ("weight_hh", (4 * H, H)), ("bias_ih", (4 * H,)), ("bias_hh", (4 * H,))):
            Pd[Q + f"{name}_l{l}"] = (torch.rand(shape, generator=g2) * 2 - 1) * (scale / H ** 0.5)
    return Pd


def layered_transducer(seed: int, L: int, V: int, H: int, D: int, J: int, scale: float = 1.0, **kw):
    Pd, Pj = random_transducer(seed, V, H, D, J, scale=scale, **kw)
    return upper_layers(Pd, seed, L, scale), Pj


def small_case(kind: str, L: int):
    """the SMALL case of tests/stream_decode_oracle.py (seed 1, scale 4, its blank and duration biases) with L layers"""
    V, H, D, J = (SMALL[k] for k in "VHDJ")
    if kind == "tdt":
        return layered_transducer(1, L, V, H, D, J, scale=4.0, n_dur=5, blank_bias=-1.0, dur0_bias=1.0)
    return layered_transducer(1, L, V, H, D, J, scale=4.0, blank_bias=8.0)


def recipe_case(kind: str, L: int = 2):
    V, H, D, J = (RECIPE[k] for k in "VHDJ")
    if kind == "tdt":
        return layered_transducer(5, L, V, H, D, J, scale=4.0, n_dur=5, blank_bias=-1.0, dur0_bias=1.0)
    return layered_transducer(5, L, V, H, D, J, scale=4.0, blank_bias=22.0)


def bf16_images(Pd, Pj, enc):
    """what the bf16 search reads: every layer's weights, the joint's and the projection rounded to bf16, widened to float32 (as
    tests/test_stream_decode_gpu._bf16_images for one layer)"""
    rb = lambda w: w.to(torch.bfloat16).to(torch.float32)   # noqa: E731
    Pd16, Pj16 = dict(Pd), dict(Pj)
    for l in range(n_layers(Pd)):
        for k in (Q + f"weight_ih_l{l}", Q + f"weight_hh_l{l}"):
            Pd16[k] = rb(Pd[k])
    outk = _out_key(Pj) + "weight"
    for k in ("pred.weight", "enc.weight", outk):
        Pj16[k] = rb(Pj[k])
    f16 = rb(F.linear(rb(enc.transpose(1, 2)), Pj16["enc.weight"], Pj["enc.bias"]))
    return Pd16, Pj16, f16


def _out_key(Pj) -> str:
    return [k[:-len("weight")] for k in Pj if k.startswith("joint_net.") and k.endswith(".weight")][0]


def _out(Pj):
    k = _out_key(Pj)
    return Pj[k + "weight"], Pj[k + "bias"]


def pred_step(Pd, Pj, last: int, h: Tensor, c: Tensor):
    """one prediction step on emb[last] with the committed state h, c [L, H] -> (gp [J], hn [L, H], cn [L, H])"""
    L, H = h.shape
    inp = Pd["prediction.embed.weight"][last]
    hn, cn = [], []
    for l in range(L):
        w_ih, w_hh, b_ih, b_hh = (Pd[Q + f"{n}_l{l}"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
        z = F.linear(inp, w_ih, b_ih) + F.linear(h[l], w_hh, b_hh)
        i, f, g, o = z[:H], z[H:2 * H], z[2 * H:3 * H], z[3 * H:]
        c2 = torch.sigmoid(f) * c[l] + torch.sigmoid(i) * torch.tanh(g)
        inp = torch.sigmoid(o) * torch.tanh(c2)
        hn.append(inp); cn.append(c2)
    return F.linear(inp, Pj["pred.weight"], Pj["pred.bias"]), torch.stack(hn), torch.stack(cn)


def fresh_state(L: int, H: int, blank: int, dtype=torch.float32) -> Dict:
    return dict(h=torch.zeros(L, H, dtype=dtype), c=torch.zeros(L, H, dtype=dtype), last=int(blank), score=0.0, frames_done=0, skip=0,
                zero_run=0)


def decode_chunk(Pd, Pj, f: Tensor, state: Dict, blank: int, max_symbols: int, durations: Optional[Sequence[int]] = None,
                 max_out: Optional[int] = None, gaps: Optional[list] = None):
    """stream_decode_oracle.decode_chunk for L layers: one chunk of one stream, f [frames, J] -> (tokens, GLOBAL frame indices, next
    state, events).  `gaps` (optional list) gets (top-2 gap of the decision, max |logit|) per decision; TDT: the smaller of the
    label and the duration gap"""
    w_out, b_out = _out(Pj)
    n = f.shape[0]
    h, c, last, score, base = state["h"], state["c"], state["last"], state["score"], state["frames_done"]
    skip, same = state["skip"], state["zero_run"]
    toks, times, full = [], [], 0
    tdt = durations is not None
    cap = max_out if max_out is not None else (n * max_symbols if max_symbols else 4 * n)
    if n > (skip if tdt else 0):
        gp, hn, cn = pred_step(Pd, Pj, last, h, c)   # the step `emit` ran after `last` (a fresh stream: the start-of-sequence step)

    def logits(t):
        z = F.linear(torch.relu(f[t] + gp), w_out, b_out)
        if gaps is not None:
            nl = z.shape[0] - (len(durations) if tdt else 0)
            top = torch.topk(z[:nl], 2).values
            gap = float(top[0] - top[1])
            if tdt:
                td = torch.topk(z[nl:], 2).values
                gap = min(gap, float(td[0] - td[1]))
            gaps.append((gap, float(z.abs().max())))
        return z

    if tdt:
        V1 = w_out.shape[0] - len(durations)
        t = skip
        while t < n and len(toks) < cap:
            z = logits(t)
            k = int(torch.argmax(z[:V1]))
            d = durations[int(torch.argmax(z[V1:]))]
            if k == blank:
                t += max(d, 1)
                same = 0
            else:
                toks.append(k); times.append(base + t)
                score += float(torch.log_softmax(z[:V1], 0)[k])
                h, c, last = hn, cn, k
                gp, hn, cn = pred_step(Pd, Pj, k, h, c)
                same = same + 1 if d == 0 else 0
                if d == 0 and max_symbols and same >= max_symbols:
                    d, same = 1, 0
                    full += 1
                t += d
        skip = max(t - n, 0)
    else:
        for t in range(n):
            sym = 0
            while (sym < max_symbols) if max_symbols else (len(toks) < cap):
                z = logits(t)
                k = int(torch.argmax(z))
                if k == blank:
                    break
                toks.append(k); times.append(base + t)
                score += float(torch.log_softmax(z, 0)[k])
                h, c, last = hn, cn, k
                gp, hn, cn = pred_step(Pd, Pj, k, h, c)
                sym += 1
            full += int(bool(max_symbols) and sym == max_symbols)
        skip = 0
    nxt = dict(h=h, c=c, last=last, score=score, frames_done=base + n, skip=skip, zero_run=same)
    return toks, times, nxt, dict(full_frames=full, crossed=skip > 0)


def decode_chunked(Pd, Pj, enc: Tensor, enc_len: Tensor, blank: int, max_symbols: int, cuts: Sequence[int],
                   durations: Optional[Sequence[int]] = None, f_all: Optional[Tensor] = None, gaps: Optional[list] = None):
    """cut every utterance at the frame positions `cuts` (ascending, inside (0, T)) and decode chunk by chunk.  enc [B, D, T].
    -> (list of (tokens, frame indices), list of final states, dict(full_frames, crossings))"""
    if f_all is None:
        f_all = F.linear(enc.transpose(1, 2), Pj["enc.weight"], Pj["enc.bias"])
    L, H = n_layers(Pd), Pd[Q + "weight_hh_l0"].shape[1]
    T = f_all.shape[1]
    edges = [0] + [int(x) for x in cuts] + [T]
    assert edges == sorted(set(edges)), edges
    hyps, finals, full, crossings = [], [], 0, 0
    for b in range(f_all.shape[0]):
        st = fresh_state(L, H, blank)
        toks, times = [], []
        n = int(enc_len[b])
        for lo, hi in zip(edges[:-1], edges[1:]):
            m = max(0, min(hi, n) - lo)
            tk, tm, st, ev = decode_chunk(Pd, Pj, f_all[b, lo:lo + m], st, blank, max_symbols, durations, gaps=gaps)
            toks += tk; times += tm
            full += ev["full_frames"]
            crossings += int(ev["crossed"] and lo + m < n)   # (a jump past the END of the utterance crosses no chunk edge)
        hyps.append((toks, times))
        finals.append(st)
    return hyps, finals, dict(full_frames=full, crossings=crossings)


def forced_walk(Pd, Pj, f_all: Tensor, enc_len: Tensor, blank: int, max_symbols: int, hyps,
                durations: Optional[Sequence[int]] = None) -> List[list]:
    """Walk the search ALONG given hypotheses (list of (tokens, frame indices)) and report per decision
    (frame, followed, own, margin, max |logit|): oracle/transducer_ref.forced_decode_margins (RNN-T: followed / own are labels,
    margin = logit[own] - logit[followed]) and stream_decode_oracle.tdt_forced_decode_margins (TDT: (label, duration) pairs, the
    larger of the label and the duration margin; the walk follows its own duration wherever that does not jump over the hypothesis's
    next label, else the best one that does not) for L layers.  A margin of 0 everywhere: the hypotheses are this restatement's own."""
    w_out, b_out = _out(Pj)
    L, H = n_layers(Pd), Pd[Q + "weight_hh_l0"].shape[1]
    tdt = durations is not None
    D = len(durations) if tdt else 0
    V1 = w_out.shape[0] - D
    report = []
    for b in range(f_all.shape[0]):
        toks, times = list(hyps[b][0]), list(hyps[b][1])
        n = int(enc_len[b])
        st = fresh_state(L, H, blank)
        h, c = st["h"], st["c"]
        gp, hn, cn = pred_step(Pd, Pj, blank, h, c)
        t, pos, same, sym, rows = 0, 0, 0, 0, []
        while t < n:
            assert not (pos < len(toks) and times[pos] < t), (b, t, pos, times[pos])   # the walk went past a label of the hypothesis
            z = F.linear(torch.relu(f_all[b, t] + gp), w_out, b_out)
            own_k = int(torch.argmax(z[:V1]))
            on_frame = pos < len(toks) and times[pos] == t
            k = toks[pos] if on_frame else blank
            if not tdt:
                rows.append((t, k, own_k, float(z[own_k] - z[k]), float(z.abs().max())))
                if k == blank:
                    t, sym = t + 1, 0
                    continue
                pos += 1
                h, c = hn, cn
                gp, hn, cn = pred_step(Pd, Pj, k, h, c)
                sym += 1
                if sym == max_symbols:   # the frame used up its emissions: the hypothesis must not hold more labels on it
                    assert not (pos < len(toks) and times[pos] == t), (b, t)
                    t, sym = t + 1, 0
                continue
            own_i = int(torch.argmax(z[V1:]))
            nxt_pos = pos + 1 if on_frame else pos
            limit = times[nxt_pos] if nxt_pos < len(toks) else None   # the frame the next decision may reach at most

            def step_of(i):
                d = durations[i]
                if k == blank:
                    return max(d, 1)
                if d == 0 and max_symbols and same + 1 >= max_symbols:
                    return 1
                return d
            ok = [i for i in range(D) if limit is None or t + step_of(i) <= limit]
            assert ok, (b, t, pos)
            fol_i = own_i if own_i in ok else max(ok, key=lambda i: (float(z[V1 + i]), -i))
            margin = max(float(z[own_k] - z[k]), float(z[V1 + own_i] - z[V1 + fol_i]))
            rows.append((t, (k, durations[fol_i]), (own_k, durations[own_i]), margin, float(z.abs().max())))
            d = durations[fol_i]
            if k == blank:
                t += max(d, 1)
                same = 0
            else:
                pos += 1
                h, c = hn, cn
                gp, hn, cn = pred_step(Pd, Pj, k, h, c)
                same = same + 1 if d == 0 else 0
                if d == 0 and max_symbols and same >= max_symbols:
                    d, same = 1, 0
                t += d
        assert pos == len(toks), (b, pos, len(toks))   # every label of the hypothesis was consumed in frame order
        report.append(rows)
    return report


def replay_confidence(Pd, Pj, f: Tensor, tokens, times, blank: int, cfg, n_dur: int = 0, dtype=None):
    """confidence_oracle.replay_transducer_confidence for L layers: walk ONE utterance along given tokens and (global) frame
    indices and give the label logits of every step that emitted one to `confidence_oracle.frame_confidence`, all arithmetic in
    `dtype` (float64 by default; float32 gives the restatement's own rounding error).  f [T, J].  -> numpy array, one per label"""
    from confidence_oracle import frame_confidence
    dtype = torch.float64 if dtype is None else dtype
    npdt = np.float64 if dtype == torch.float64 else np.float32
    Pd = {k: v.to(dtype) for k, v in Pd.items()}
    Pj = {k: v.to(dtype) for k, v in Pj.items()}
    f = f.to(dtype)
    w_out, b_out = _out(Pj)
    V1 = w_out.shape[0] - n_dur
    st = fresh_state(n_layers(Pd), Pd[Q + "weight_hh_l0"].shape[1], blank, dtype)
    h, c = st["h"], st["c"]
    gp, hn, cn = pred_step(Pd, Pj, blank, h, c)
    out = []
    for k, t in zip(tokens, times):
        z = F.linear(torch.relu(f[int(t)] + gp), w_out, b_out)
        out.append(frame_confidence(torch.log_softmax(z[:V1], 0).numpy(), cfg, dtype=npdt))
        h, c = hn, cn
        gp, hn, cn = pred_step(Pd, Pj, int(k), h, c)
    return np.array(out, dtype=npdt)
