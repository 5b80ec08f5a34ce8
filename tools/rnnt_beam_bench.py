"""Time the transducer beam search (ops.transducer_beam_decode) against the greedy search at recipe geometry: B = 32, T = 250,
H = J = 640, V1 = 1025, bf16 weight images, the seeded random model of tools/decode_ab.py.  Greedy, W = 1, 4 and 16 are alternated
round by round in one process (device events around each call), so drift hits all of them alike.  Prints one JSON line per
decoder: median / min / max ms per call, the steps of a call (T + the labels of the best hypothesis, averaged over the batch: every
step of either search consumes one frame or one label) and the ratio of the time per step to the greedy search's.
With `--lm ORDER` every beam is also timed with an n-gram model fused (ops.transducer_beam_decode_fused; the model of the CTC
bench: the tests' generator at this order, through ARPA text and NGramLM.from_arpa) at `--alpha`, alternated with the plain search
in the same rounds; those lines add the ratio to the plain search of the same width and the back-off chain depths (states before
state 0) of the automaton states the best hypotheses passed through, found by walking their labels through the tables on the host.

    python tools/rnnt_beam_bench.py [--decoder rnnt|tdt|both] [--rounds 7] [--warmup 2] [--lm ORDER] [--alpha 0.5]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nemo_amd import ops  # noqa: E402

DUR = [0, 1, 2, 3, 4]


def chain_depths(lm, tokens, lengths):
    """histogram {depth: count} of the back-off chain depths of the states the label sequences pass through, <s> first"""
    begin, tok, _, nxt, _, bo_next = (t.tolist() for t in lm.to("cpu")[:6])
    hist = {}
    for row, n in zip(tokens.tolist(), lengths.tolist()):
        s = 1
        for c in [None] + row[:n]:
            while c is not None:   # the look-up: the arc of c in s or in the first state down the chain that has one
                arcs = tok[begin[s]:begin[s + 1]] if s else None
                if s == 0 or c in arcs:
                    s = nxt[c if s == 0 else begin[s] + arcs.index(c)]
                    break
                s = bo_next[s]
            d, q = 0, s
            while q:
                d, q = d + 1, bo_next[q]
            hist[d] = hist.get(d, 0) + 1
    return dict(sorted(hist.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decoder", default="both", choices=["rnnt", "tdt", "both"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--beams", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--lm", type=int, default=0, metavar="ORDER", help="also time every beam with an n-gram model of this order fused")
    ap.add_argument("--alpha", type=float, default=0.5, help="the fusion weight of the --lm runs")
    args = ap.parse_args()
    dev = "cuda"
    B, T, H, J, V1, ms = 32, 250, 640, 640, 1025, 10
    lm = None
    if args.lm:
        from ctc_beam_bench import make_ngram_lm
        lm = make_ngram_lm(V1 - 1, args.lm)
    for kind in (["rnnt", "tdt"] if args.decoder == "both" else [args.decoder]):
        D = len(DUR) if kind == "tdt" else 0
        g = torch.Generator(device=dev).manual_seed(0)
        r = lambda *s, k=1.0: torch.randn(*s, device=dev, generator=g) * k   # noqa: E731
        bf = lambda t: t.to(torch.bfloat16).contiguous()   # noqa: E731
        f = bf(r(B, T, J, k=1.5))
        lens = torch.full((B,), T, dtype=torch.int64, device=dev)
        emb = r(V1, H)
        emb[V1 - 1] = 0.0
        w_ih, w_hh, w_pred = bf(r(4 * H, H, k=0.15)), bf(r(4 * H, H, k=0.15)), bf(r(J, H, k=0.15))
        b_ih, b_hh, b_pred = r(4 * H, k=0.1), r(4 * H, k=0.1), r(J, k=0.1)
        w_out, b_out = bf(r(V1 + D, J, k=0.15)), r(V1 + D, k=0.1)
        b_out[V1 - 1] += 2.0
        model = (f, lens, emb, w_ih, H, w_hh, H, b_ih, b_hh, w_pred, H, b_pred, w_out, J, b_out, V1 - 1)
        dur = DUR if kind == "tdt" else None

        def greedy():
            out = ops.tdt_greedy_decode(*model, dur, ms) if dur else ops.rnnt_greedy_decode(*model, ms)
            return out[2].float().mean()

        calls = {"greedy": greedy}
        for W in args.beams:
            calls[f"beam{W}"] = lambda W=W: ops.transducer_beam_decode(*model, ms, W, durations=dur)[2][:, 0].float().mean()
            if lm is not None:
                calls[f"beam{W}_lm"] = lambda W=W: ops.transducer_beam_decode_fused(*model, ms, W, [(lm, args.alpha)],
                                                                                    durations=dur)[2][:, 0].float().mean()
        times = {k: [] for k in calls}
        labels = {}
        for rnd in range(args.warmup + args.rounds):
            for name, call in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                n = call()
                e1.record()
                torch.cuda.synchronize()
                labels[name] = float(n)
                if rnd >= args.warmup:
                    times[name].append(e0.elapsed_time(e1))
        per_step = {k: statistics.median(v) / (T + labels[k]) for k, v in times.items()}
        for name, v in times.items():
            extra = {}
            if name.endswith("_lm"):
                tk, _, n, _, _ = ops.transducer_beam_decode_fused(*model, ms, int(name[4:-3]), [(lm, args.alpha)], durations=dur)
                extra = dict(lm=dict(order=lm.order, states=lm.num_states, arcs=lm.num_arcs, alpha=args.alpha),
                             step_ratio_to_plain=round(per_step[name] / per_step[name[:-3]], 3),
                             chain_depths=chain_depths(lm, tk[:, 0].cpu(), n[:, 0].cpu()))
            print(json.dumps(dict(decoder=kind, search=name, B=B, T=T, H=H, J=J, V1=V1, rounds=args.rounds,
                                  ms_median=round(statistics.median(v), 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3),
                                  labels_best=round(labels[name], 1), us_per_step=round(1e3 * per_step[name], 2),
                                  step_ratio_to_greedy=round(per_step[name] / per_step["greedy"], 3),
                                  call_ratio_to_greedy=round(statistics.median(v) / statistics.median(times["greedy"]), 3), **extra)),
                  flush=True)


if __name__ == "__main__":
    main()
