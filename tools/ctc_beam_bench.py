"""CTC prefix beam search on one GPU (profiles/ctc_beam.md is made with this).

Per shape (B, T, C), beam width W and threshold, `--rounds` rounds; in every round each candidate runs its launches between two
device events, the candidates alternating inside the round (same process, same buffers), so that drift of the box hits all of
them alike:
  * mi355x_ctc_beam_decode for every (W, threshold) asked for,
  * mi355x_ctc_greedy_decode at the same shape: the scale (one pass over the log-probabilities, no search),
  * mi355x_ctc_greedy_decode and mi355x_ctc_greedy_decode_ts of every library given with `--lib name=path` (e.g. a build of the
    parent commit), alternating with the in-tree library's: the spread between builds of entry points this search does not touch.
Input: log-softmax of 1.5 * N(0,1) with +5 on the class of a random path (blank with probability 0.6), the generator of the tests --
peaked like a trained model's output, so that the threshold prunes; lengths = T.  The launches of a candidate per round are sized
from one timed launch so that a round of it takes about `--round-ms`.  Reported per candidate: median, min and max of the
per-round means, in microseconds per launch.

    python tools/ctc_beam_bench.py [--shapes 32,501,129 32,501,1025] [--beams 4 16 64] [--thresholds 20 inf] [--rounds 7]
                                   [--lib parent=PATH ...] [--json OUT]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

dev = "cuda"
GREEDY = ("mi355x_ctc_greedy_decode", "mi355x_ctc_greedy_decode_ts")


def load(path):
    from nemo_amd import _lib
    lib = ctypes.CDLL(path)
    for name in GREEDY:
        getattr(lib, name).argtypes = _lib.SIGNATURES[name]
        getattr(lib, name).restype = ctypes.c_int
    return lib


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def rounds(cands, n_rounds, round_ms):
    iters = {}
    for k, fn in cands.items():   # warm-up: code objects loaded, every shape seen; then one timed launch sizes the rounds
        fn(); fn()
        torch.cuda.synchronize()
        iters[k] = max(2, min(200, int(round_ms * 1e3 / max(1.0, timed(fn, 1)))))
    per = {k: [] for k in cands}
    for _ in range(n_rounds):
        for k, fn in cands.items():
            per[k].append(timed(fn, iters[k]))
    return {k: dict(median_us=round(statistics.median(v), 1), min_us=round(min(v), 1), max_us=round(max(v), 1), iters=iters[k])
            for k, v in per.items()}


def make_logp(B, T, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, C, generator=g) * 1.5
    path = torch.where(torch.rand(B, T, generator=g) < 0.6, torch.full((B, T), C - 1), torch.randint(0, C - 1, (B, T), generator=g))
    x.scatter_add_(2, path.unsqueeze(-1), torch.full((B, T, 1), 5.0))
    return torch.log_softmax(x, -1).to(dev)


def one_shape(B, T, C, beams, thresholds, libs, n_rounds, round_ms):
    from nemo_amd import _lib
    lib = _lib.lib
    logp = make_logp(B, T, C)
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)
    Wmax = max(beams)
    i32 = dict(dtype=torch.int32, device=dev)
    ws = torch.empty(B * int(lib.mi355x_ctc_beam_workspace_elems(T, Wmax)), **i32)
    tokens, frames = torch.empty(B, Wmax, T, **i32), torch.empty(B, Wmax, T, **i32)
    hyp_len, n_hyp, score = torch.empty(B, Wmax, **i32), torch.empty(B, **i32), torch.empty(B, Wmax, device=dev)
    gtok, gst, gen = (torch.empty(B, T, **i32) for _ in range(3))
    glen, gscore = torch.empty(B, **i32), torch.empty(B, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()   # noqa: E731

    def beam(W, th):
        def fn():
            rc = lib.mi355x_ctc_beam_decode(p(logp), p(lens), p(ws), p(tokens), p(frames), p(hyp_len), p(score), p(n_hyp), B, T, C, C - 1,
                                            W, th, 0.0, stream)
            assert rc == 0, rc
        return fn

    def greedy(l, ts):
        def fn():
            if ts:
                rc = l.mi355x_ctc_greedy_decode_ts(p(logp), p(lens), p(gtok), p(glen), p(gscore), p(gst), p(gen), B, T, C, C - 1, stream)
            else:
                rc = l.mi355x_ctc_greedy_decode(p(logp), p(lens), p(gtok), p(glen), p(gscore), B, T, C, C - 1, stream)
            assert rc == 0, rc
        return fn
    cands = {"greedy": greedy(lib, False), "greedy_ts": greedy(lib, True)}
    for name, l in libs.items():
        cands[f"greedy[{name}]"] = greedy(l, False)
        cands[f"greedy_ts[{name}]"] = greedy(l, True)
    for W in beams:
        for th in thresholds:
            cands[f"beam W={W} threshold={th}"] = beam(W, th)
    row = dict(shape=dict(B=B, T=T, C=C), **rounds(cands, n_rounds, round_ms))
    # what the search found at the widest setting: hypotheses per utterance and how often the best one differs from the greedy one
    beam(Wmax, thresholds[0])(); greedy(lib, False)()
    torch.cuda.synchronize()
    same = sum(int(hyp_len[b, 0]) == int(glen[b]) and torch.equal(tokens[b, 0, : int(glen[b])], gtok[b, : int(glen[b])]) for b in range(B))
    row["n_hyp_mean"] = float(n_hyp.float().mean())
    row["best_equals_greedy"] = f"{same}/{B}"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["32,501,129", "32,501,1025"])
    ap.add_argument("--beams", nargs="+", type=int, default=[4, 16, 64])
    ap.add_argument("--thresholds", nargs="+", type=float, default=[20.0, float("inf")])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--round-ms", type=float, default=50.0)
    ap.add_argument("--lib", nargs="*", default=[], help="name=path of further builds of the library")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    libs = {a.split("=", 1)[0]: load(a.split("=", 1)[1]) for a in args.lib}
    out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, round_ms=args.round_ms, shapes=[])
    for s in args.shapes:
        B, T, C = (int(x) for x in s.split(","))
        row = one_shape(B, T, C, args.beams, args.thresholds, libs, args.rounds, args.round_ms)
        out["shapes"].append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
