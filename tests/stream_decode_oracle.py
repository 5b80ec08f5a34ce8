"""TEST INFRASTRUCTURE ONLY -- CPU restatement of the RESUMABLE greedy transducer search (csrc/rnnt_decode.hip:
mi355x_transducer_greedy_decode with a state to write, RNN-T and TDT), fp32 torch, utterance by utterance.

Written from oracle/transducer_ref.greedy_decode and tests/tdt_oracle.tdt_greedy_decode plus the per-stream decoder state:
    h, c          committed LSTM state                                   fresh: 0
    last          last emitted label                                     fresh: blank (zero embedding row)
    score         running sum of the emitted labels' log-probabilities   fresh: 0
    frames_done   frames consumed by earlier chunks                      fresh: 0
    skip          TDT: frames of this chunk already jumped over          fresh: 0
    zero_run      TDT: current run of labels of duration 0               fresh: 0
A chunk rebuilds (gp, hn, cn) from (h, c, emb[last]) at entry, runs the one-shot loop over its frames with `frames_done` added
to every frame index, and returns the next state.  `decode_chunked` cuts a batch at given frame positions; for any cuts it must
return what the two one-shot functions return for the whole sequence (tests/test_hybrid_host.py).

`tdt_forced_decode_margins` is the TDT counterpart of oracle/transducer_ref.forced_decode_margins (the checker of a
reduced-precision device search)."""
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn.functional as F
from torch import Tensor


def _weights(Pd, Pj):
    q = "prediction.dec_rnn.lstm."
    assert q + "weight_ih_l1" not in Pd, "one LSTM layer"
    w_ih, w_hh, b_ih, b_hh = (Pd[q + n + "_l0"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
    out = [k[:-len("weight")] for k in Pj if k.startswith("joint_net.") and k.endswith(".weight")][0]
    return Pd["prediction.embed.weight"], w_ih, w_hh, b_ih, b_hh, Pj[out + "weight"], Pj[out + "bias"]


def _pred(Pd, Pj, last, h, c):
    emb, w_ih, w_hh, b_ih, b_hh, _, _ = _weights(Pd, Pj)
    H = w_hh.shape[1]
    z = F.linear(emb[last], w_ih, b_ih) + F.linear(h, w_hh, b_hh)
    i, f, g, o = z[:H], z[H:2 * H], z[2 * H:3 * H], z[3 * H:]
    c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    h2 = torch.sigmoid(o) * torch.tanh(c2)
    return F.linear(h2, Pj["pred.weight"], Pj["pred.bias"]), h2, c2


def random_transducer(seed: int, V: int, H: int, D: int, J: int, n_dur: int = 0, scale: float = 1.0, blank_bias: float = 0.0,
                      dur0_bias: float = 0.0):
    """state-dicts (the reference's keys) of a random prediction network + joint: torch's default LSTM / Linear initialisation
    ranges times `scale`, `blank_bias` added to the blank logit's bias, `dur0_bias` to the bias of the first (zero) duration"""
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape, k: (torch.rand(*shape, generator=g) * 2 - 1) * (scale / k ** 0.5)   # noqa: E731
    emb = torch.randn(V + 1, H, generator=g) * scale
    emb[V] = 0.0
    Pd = {"prediction.embed.weight": emb,
          "prediction.dec_rnn.lstm.weight_ih_l0": u(4 * H, H, k=H), "prediction.dec_rnn.lstm.weight_hh_l0": u(4 * H, H, k=H),
          "prediction.dec_rnn.lstm.bias_ih_l0": u(4 * H, k=H), "prediction.dec_rnn.lstm.bias_hh_l0": u(4 * H, k=H)}
    Pj = {"enc.weight": u(J, D, k=D), "enc.bias": u(J, k=D), "pred.weight": u(J, H, k=H), "pred.bias": u(J, k=H),
          "joint_net.2.weight": u(V + 1 + n_dur, J, k=J), "joint_net.2.bias": u(V + 1 + n_dur, k=J)}
    Pj["joint_net.2.bias"][V] += blank_bias
    if n_dur:
        Pj["joint_net.2.bias"][V + 1] += dur0_bias
    return Pd, Pj


def fresh_state(H: int, blank: int) -> Dict:
    return dict(h=torch.zeros(H), c=torch.zeros(H), last=int(blank), score=0.0, frames_done=0, skip=0, zero_run=0)


def decode_chunk(Pd, Pj, f: Tensor, state: Dict, blank: int, max_symbols: int, durations: Optional[Sequence[int]] = None,
                 max_out: Optional[int] = None, gaps: Optional[list] = None):
    """(`gaps`, optional list: gets (top-2 gap of the decision, max |logit|) appended per decision -- for TDT the smaller of the
    label and the duration gap)
    one chunk of one stream: f [L, J] = this chunk's rows of the encoder projection.  -> (tokens, GLOBAL frame indices, next
    state, events) with events = dict(full_frames = frames that emitted max_symbols labels, crossed = the last jump left the chunk)"""
    _, _, _, _, _, w_out, b_out = _weights(Pd, Pj)
    L = f.shape[0]
    h, c, last, score, base = state["h"], state["c"], state["last"], state["score"], state["frames_done"]
    skip, same = state["skip"], state["zero_run"]
    toks, times, full = [], [], 0
    tdt = durations is not None
    cap = max_out if max_out is not None else (L * max_symbols if max_symbols else 4 * L)
    if L > (skip if tdt else 0):
        gp, hn, cn = _pred(Pd, Pj, last, h, c)   # the step `emit` ran after `last` (a fresh stream: the start-of-sequence step)

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
        D = len(durations)
        V1 = w_out.shape[0] - D
        t = skip
        while t < L and len(toks) < cap:
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
                gp, hn, cn = _pred(Pd, Pj, k, h, c)
                same = same + 1 if d == 0 else 0
                if d == 0 and max_symbols and same >= max_symbols:
                    d, same = 1, 0
                    full += 1
                t += d
        skip = max(t - L, 0)
    else:
        for t in range(L):
            sym = 0
            while (sym < max_symbols) if max_symbols else (len(toks) < cap):
                z = logits(t)
                k = int(torch.argmax(z))
                if k == blank:
                    break
                toks.append(k); times.append(base + t)
                score += float(torch.log_softmax(z, 0)[k])
                h, c, last = hn, cn, k
                gp, hn, cn = _pred(Pd, Pj, k, h, c)
                sym += 1
            full += int(bool(max_symbols) and sym == max_symbols)
        skip = 0
    nxt = dict(h=h, c=c, last=last, score=score, frames_done=base + L, skip=skip, zero_run=same)
    return toks, times, nxt, dict(full_frames=full, crossed=skip > 0)


def decode_chunked(Pd, Pj, enc: Tensor, enc_len: Tensor, blank: int, max_symbols: int, cuts: Sequence[int],
                   durations: Optional[Sequence[int]] = None, f_all: Optional[Tensor] = None, gaps: Optional[list] = None):
    """cut every utterance of the batch at the frame positions `cuts` (ascending, inside (0, T); a short utterance gets chunks of
    length 0 behind its end) and decode chunk by chunk.  enc [B, D, T].  -> (list of (tokens, frame indices), list of final
    states, dict(full_frames, crossings))"""
    if f_all is None:
        f_all = F.linear(enc.transpose(1, 2), Pj["enc.weight"], Pj["enc.bias"])
    H = Pd["prediction.dec_rnn.lstm.weight_hh_l0"].shape[1]
    T = enc.shape[2]
    edges = [0] + [int(x) for x in cuts] + [T]
    assert edges == sorted(set(edges)), edges
    hyps, finals, full, crossings = [], [], 0, 0
    for b in range(enc.shape[0]):
        st = fresh_state(H, blank)
        toks, times = [], []
        n = int(enc_len[b])
        for lo, hi in zip(edges[:-1], edges[1:]):
            L = max(0, min(hi, n) - lo)
            tk, tm, st, ev = decode_chunk(Pd, Pj, f_all[b, lo:lo + L], st, blank, max_symbols, durations, gaps=gaps)
            toks += tk; times += tm
            full += ev["full_frames"]
            crossings += int(ev["crossed"] and lo + L < n)   # (a jump past the END of the utterance crosses no chunk edge)
        hyps.append((toks, times))
        finals.append(st)
    return hyps, finals, dict(full_frames=full, crossings=crossings)


def tdt_forced_decode_margins(Pd, Pj, enc: Tensor, enc_len: Tensor, blank: int, durations: Sequence[int], max_symbols: int, hyps,
                              f_all: Optional[Tensor] = None) -> List[list]:
    """Walk the greedy TDT search ALONG given hypotheses (list of (tokens, frame indices)) and report, per decision,
    (frame, followed (label, duration), own (label, duration), margin, max |logit|): margin = the larger of
    logit[own label] - logit[followed label] and logit[own duration] - logit[followed duration]; 0 everywhere means the hypotheses
    are this restatement's own.  The followed label is the hypothesis's label on this frame (else blank).  A hypothesis does not
    record durations, so the walk follows its own duration arg-max wherever that does not jump over the hypothesis's next label,
    and otherwise the best-scoring duration that does not (a decision the two sides took differently, reported with its
    margin); a hypothesis the walk cannot consume that way fails the final assertion."""
    _, _, _, _, _, w_out, b_out = _weights(Pd, Pj)
    if f_all is None:
        f_all = F.linear(enc.transpose(1, 2), Pj["enc.weight"], Pj["enc.bias"])
    H = Pd["prediction.dec_rnn.lstm.weight_hh_l0"].shape[1]
    D = len(durations)
    V1 = w_out.shape[0] - D
    report = []
    for b in range(enc.shape[0]):
        toks, times = list(hyps[b][0]), list(hyps[b][1])
        L = int(enc_len[b])
        h, c = torch.zeros(H), torch.zeros(H)
        gp, hn, cn = _pred(Pd, Pj, blank, h, c)
        t, pos, same, rows = 0, 0, 0, []
        while t < L:
            assert not (pos < len(toks) and times[pos] < t), (b, t, pos, times[pos])   # the walk jumped over a label of the hypothesis
            z = F.linear(torch.relu(f_all[b, t] + gp), w_out, b_out)
            own_k, own_i = int(torch.argmax(z[:V1])), int(torch.argmax(z[V1:]))
            on_frame = pos < len(toks) and times[pos] == t
            k = toks[pos] if on_frame else blank
            # the frame the next decision may reach at most: the hypothesis's next label
            nxt_pos = pos + 1 if on_frame else pos
            limit = times[nxt_pos] if nxt_pos < len(toks) else None

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
                gp, hn, cn = _pred(Pd, Pj, k, h, c)
                same = same + 1 if d == 0 else 0
                if d == 0 and max_symbols and same >= max_symbols:
                    d, same = 1, 0
                t += d
        assert pos == len(toks), (b, pos, len(toks))
        report.append(rows)
    return report


# ---- the two settings the tests share (tests/test_hybrid_host.py shows on the CPU that they hit the hard cases; the GPU tests run them)
SMALL = dict(V=48, H=32, D=24, J=32, T=37, lens=[37, 30, 9, 37])
RECIPE = dict(V=1024, H=640, D=512, J=640, T=100, lens=[100, 77, 0, 100, 17, 1], max_symbols=10)   # fast-conformer_transducer_bpe.yaml widths


def small_case(kind: str):
    """RNN-T: a blank bias that leaves frames with 0, some and max_symbols labels; TDT: blank held down and duration 0 pushed up, so
    that runs of zero-duration labels reach max_symbols while other durations jump over chunk edges"""
    V, H, D, J = (SMALL[k] for k in "VHDJ")
    if kind == "tdt":
        return random_transducer(1, V, H, D, J, n_dur=5, scale=4.0, blank_bias=-1.0, dur0_bias=1.0)
    return random_transducer(1, V, H, D, J, scale=4.0, blank_bias=SMALL_RNNT_BLANK_BIAS)


SMALL_RNNT_BLANK_BIAS = 8.0


def small_enc():
    return torch.randn(len(SMALL["lens"]), SMALL["D"], SMALL["T"], generator=torch.Generator().manual_seed(101)) * 1.5


def recipe_case(kind: str):
    """built as tests/test_rnnt_decoding.py builds its recipe-geometry case: the modules' own initialisation under seed 5, every
    parameter times 4, blank bias + 2 (TDT: five duration outputs behind the labels)"""
    from nemo_amd.modules import RNNTDecoder, RNNTJoint
    V, H, D, J = (RECIPE[k] for k in "VHDJ")
    torch.manual_seed(5)
    dec = RNNTDecoder(prednet={"pred_hidden": H, "pred_rnn_layers": 1, "dropout": 0.0}, vocab_size=V, compute_dtype=torch.float32)
    joint = RNNTJoint(jointnet={"encoder_hidden": D, "pred_hidden": H, "joint_hidden": J, "activation": "relu", "dropout": 0.0},
                      num_classes=V, num_extra_outputs=5 if kind == "tdt" else 0, compute_dtype=torch.float32)
    with torch.no_grad():
        for p in list(dec.parameters()) + list(joint.parameters()):
            p.mul_(4.0)
        joint.joint_net[-1].bias[V] += 2.0
    return ({k: v.detach().clone() for k, v in dec.state_dict().items()}, {k: v.detach().clone() for k, v in joint.state_dict().items()})


def recipe_enc():
    return torch.randn(len(RECIPE["lens"]), RECIPE["D"], RECIPE["T"], generator=torch.Generator().manual_seed(105)) * 1.5
