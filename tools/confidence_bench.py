"""Cost of confidence estimation on one GPU (profiles/confidence.md is made with this).

  * mi355x_ctc_greedy_decode_conf against mi355x_ctc_greedy_decode_ts at the shape of tools/align_bench.py (B = 32, T = 501,
    C = 129), per method;
  * the four *_conf searches against their plain siblings at the shape of tools/decode_ab.py (B = 32, T = 250, H = J = 640,
    V1 = 1025, bf16 weights), default method.
`--rounds` rounds; in every round each candidate runs `--iters` launches between two device events, the candidates alternating
inside the round (same process, same buffers).  Reported: median, min and max of the per-round means, microseconds per launch.

    python tools/confidence_bench.py [--rounds 7] [--iters 50] [--search-rounds 3] [--search-iters 2] [--only ctc|search] [--json OUT]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

dev = "cuda"


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def rounds(cands, n_rounds, iters):
    for fn in cands.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    per = {k: [] for k in cands}
    for _ in range(n_rounds):
        for k, fn in cands.items():
            per[k].append(timed(fn, iters))
    return {k: dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2)) for k, v in per.items()}


def ctc(n_rounds, iters, B=32, T=501, C=129):
    from nemo_amd import ops
    from nemo_amd.modules import ConfidenceMethodConfig
    g = torch.Generator().manual_seed(0)
    logp = torch.log_softmax(torch.randn(B, T, C, generator=g), -1).to(dev)
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)
    cands = {"ts": lambda: ops.ctc_greedy_decode_ts(logp, lens, C - 1)}
    for name, kw in (("max_prob", dict(name="max_prob")), ("tsallis exp 0.33", {}), ("gibbs lin 0.5", dict(entropy_type="gibbs", alpha=0.5, entropy_norm="lin")),
                     ("renyi exp 2", dict(entropy_type="renyi", alpha=2.0))):
        m = ConfidenceMethodConfig(**kw).kernel_args(C)
        cands["conf " + name] = lambda m=m: ops.ctc_greedy_decode_conf(logp, lens, C - 1, m, 1, True)
    return rounds(cands, n_rounds, iters)


def search(n_rounds, iters, B=32, T=250, H=640, J=640, V1=1025, ms=10):
    from nemo_amd import ops
    from nemo_amd.modules import ConfidenceMethodConfig
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s, k=1.0: torch.randn(*s, device=dev, generator=g) * k   # noqa: E731
    bf = lambda t: t.to(torch.bfloat16).contiguous()   # noqa: E731
    f = bf(r(B, T, J, k=1.5))
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)
    emb = r(V1, H)
    emb[V1 - 1] = 0.0
    w_ih, w_hh, w_pred = bf(r(4 * H, H, k=0.15)), bf(r(4 * H, H, k=0.15)), bf(r(J, H, k=0.15))
    b_ih, b_hh, b_pred = r(4 * H, k=0.1), r(4 * H, k=0.1), r(J, k=0.1)
    w_out, b_out = bf(r(V1 + 5, J, k=0.15)), r(V1 + 5, k=0.1)
    b_out[V1 - 1] += 2.0
    DUR = [0, 1, 2, 3, 4]
    m = ConfidenceMethodConfig().kernel_args(V1)
    a_r = (f, lens, emb, w_ih, H, w_hh, H, b_ih, b_hh, w_pred, H, b_pred, w_out[:V1], J, b_out[:V1].contiguous(), V1 - 1)
    a_t = (f, lens, emb, w_ih, H, w_hh, H, b_ih, b_hh, w_pred, H, b_pred, w_out, J, b_out, V1 - 1)
    cands = {
        "rnnt": lambda: ops.rnnt_greedy_decode(*a_r, ms), "rnnt conf": lambda: ops.rnnt_greedy_decode_conf(*a_r, ms, m),
        "tdt": lambda: ops.tdt_greedy_decode(*a_t, DUR, ms), "tdt conf": lambda: ops.tdt_greedy_decode_conf(*a_t, DUR, ms, m),
        "rnnt stream": lambda: ops.rnnt_greedy_decode_stream(*a_r, ms),
        "rnnt stream conf": lambda: ops.rnnt_greedy_decode_stream_conf(*a_r, ms, m),
        "tdt stream": lambda: ops.tdt_greedy_decode_stream(*a_t, DUR, ms),
        "tdt stream conf": lambda: ops.tdt_greedy_decode_stream_conf(*a_t, DUR, ms, m),
    }
    out = rounds(cands, n_rounds, iters)
    out["labels"] = {"rnnt": int(ops.rnnt_greedy_decode(*a_r, ms)[2].sum()), "tdt": int(ops.tdt_greedy_decode(*a_t, DUR, ms)[2].sum())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--search-rounds", type=int, default=3)   # (an RNN-T search of this shape takes seconds)
    ap.add_argument("--search-iters", type=int, default=2)
    ap.add_argument("--only", default=None, choices=["ctc", "search"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    res = {}
    if args.only != "search":
        res["ctc B=32 T=501 C=129"] = ctc(args.rounds, args.iters)
    if args.only != "ctc":
        res["search B=32 T=250"] = search(args.search_rounds, args.search_iters)
    for shape, row in res.items():
        print(shape)
        for k, v in row.items():
            print(f"  {k:20s} {v}")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
