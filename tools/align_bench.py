"""CTC forced alignment and greedy timestamps on one GPU (profiles/ctc_align.md is made with this).

Per shape (B, T, C, U), `--rounds` rounds; in every round each candidate runs `--iters` launches between two device events, the
candidates alternating inside the round (same process, same buffers), so that drift of the box hits all of them alike:
  * mi355x_ctc_align in the wave-resident form (where 2U+1 <= 1024) and in the LDS form,
  * mi355x_ctc_loss with grad = NULL at the same shape: the yardstick (two lattice walks with log-sum-exp, no backtrace),
  * the same entry point of every library given with `--lib name=path` (variants built by tools/ab_build.py, e.g.
    fwd="@ctc:-DCTC_ALIGN_BACKTRACE=0" = forward walk alone, naive="@ctc:-DCTC_ALIGN_BACKTRACE=2" = single-lane chase in global memory),
  * mi355x_ctc_greedy_decode_ts against mi355x_ctc_greedy_decode (and the latter out of every `--lib` library: the spread between builds),
  * for context, one D2H copy of the [B,T,C] log-probabilities against the [B,U] integers that leave the device now.
Reported per candidate: median, min and max of the per-round means, in microseconds per launch.

    python tools/align_bench.py [--shapes 32,501,129,100 4,4000,129,1500] [--rounds 7] [--iters 50] [--lib fwd=PATH ...] [--json OUT]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

dev = "cuda"


def load(path):
    from nemo_amd import _lib
    lib = ctypes.CDLL(path)
    for name in ("mi355x_ctc_align", "mi355x_ctc_align_config", "mi355x_ctc_greedy_decode", "mi355x_ctc_greedy_decode_ts", "mi355x_ctc_loss"):
        if hasattr(lib, name):   # (a build of an older commit has no alignment)
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


def rounds(cands, n_rounds, iters):
    for fn in cands.values():   # warm-up: code objects loaded, every shape seen
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    per = {k: [] for k in cands}
    for _ in range(n_rounds):
        for k, fn in cands.items():
            per[k].append(timed(fn, iters))
    return {k: dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2)) for k, v in per.items()}


def one_shape(B, T, C, U, libs, n_rounds, iters):
    from nemo_amd import _lib
    g = torch.Generator().manual_seed(0)
    logp = torch.log_softmax(torch.randn(B, T, C, generator=g), -1).to(dev)
    tg = torch.randint(0, C - 1, (B, U), generator=g).to(dev)
    in_len = torch.full((B,), T, dtype=torch.int64, device=dev)
    tgt_len = torch.full((B,), U, dtype=torch.int64, device=dev)
    S = 2 * U + 1
    bp = torch.empty(B * T * ((U + 8) & ~7), dtype=torch.uint8, device=dev)
    path = torch.empty(B, T, dtype=torch.int32, device=dev)
    ts, te = torch.empty(B, U, dtype=torch.int32, device=dev), torch.empty(B, U, dtype=torch.int32, device=dev)
    score = torch.empty(B, device=dev)
    alpha, beta = torch.empty(B, T, S, device=dev), torch.empty(B, T, S, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()   # noqa: E731

    def align(lib, form):
        def fn():
            lib.mi355x_ctc_align_config(form)
            rc = lib.mi355x_ctc_align(p(logp), p(tg), p(in_len), p(tgt_len), p(bp), p(path), p(ts), p(te), p(score), B, T, C, U, C - 1, stream)
            assert rc == 0, rc
        return fn

    def loss():
        rc = _lib.lib.mi355x_ctc_loss(p(logp), p(tg), p(in_len), p(tgt_len), p(alpha), p(beta), p(score), None, B, T, C, U, C - 1, 1.0, 1, stream)
        assert rc == 0, rc
    cands = {}
    if S <= 1024:
        cands["align_wave"] = align(_lib.lib, 1)
    cands["align_lds"] = align(_lib.lib, 0)
    cands["ctc_loss_nograd"] = loss
    for name, lib in libs.items():
        if hasattr(lib, "mi355x_ctc_align"):
            if S <= 1024:
                cands[f"align_wave[{name}]"] = align(lib, 1)
            cands[f"align_lds[{name}]"] = align(lib, 0)
    row = dict(shape=dict(B=B, T=T, C=C, U=U), **rounds(cands, n_rounds, iters))
    # what leaves the device: the log-probabilities (host-side Viterbi) against the first / last frames
    torch.cuda.synchronize()
    for name, fn in (("d2h_logp", lambda: logp.cpu()), ("d2h_frames", lambda: (ts.cpu(), te.cpu(), score.cpu()))):
        fn()
        v = []
        for _ in range(n_rounds):
            t0 = time.perf_counter()
            fn()
            v.append((time.perf_counter() - t0) * 1e6)
        row[name] = dict(median_us=round(statistics.median(v), 1), min_us=round(min(v), 1), max_us=round(max(v), 1))
    return row


def greedy(B, T, C, libs, n_rounds, iters):
    from nemo_amd import _lib
    g = torch.Generator().manual_seed(1)
    logp = torch.log_softmax(torch.randn(B, T, C, generator=g), -1).to(dev)
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)
    tok, st, en = (torch.empty(B, T, dtype=torch.int32, device=dev) for _ in range(3))
    olen, score = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()   # noqa: E731

    def plain(lib):
        def fn():
            assert lib.mi355x_ctc_greedy_decode(p(logp), p(lens), p(tok), p(olen), p(score), B, T, C, C - 1, stream) == 0
        return fn

    def with_ts():
        assert _lib.lib.mi355x_ctc_greedy_decode_ts(p(logp), p(lens), p(tok), p(olen), p(score), p(st), p(en), B, T, C, C - 1, stream) == 0
    cands = {"greedy": plain(_lib.lib), "greedy_ts": with_ts}
    for name, lib in libs.items():
        cands[f"greedy[{name}]"] = plain(lib)
    return dict(shape=dict(B=B, T=T, C=C), **rounds(cands, n_rounds, iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["32,501,129,100", "4,4000,129,1500"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--lib", nargs="*", default=[], help="name=path of further builds of the library")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    libs = {a.split("=", 1)[0]: load(a.split("=", 1)[1]) for a in args.lib}
    out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, align=[], greedy=None)
    for s in args.shapes:
        B, T, C, U = (int(x) for x in s.split(","))
        row = one_shape(B, T, C, U, libs, args.rounds, max(2, args.iters // 10) if T * U > 1_000_000 else args.iters)
        out["align"].append(row)
        print(json.dumps(row), flush=True)
    B, T, C, _ = (int(x) for x in args.shapes[0].split(","))
    out["greedy"] = greedy(B, T, C, libs, args.rounds, args.iters)
    print(json.dumps(out["greedy"]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
