"""Transducer forced alignment on one GPU (profiles/transducer_align.md is made with this): the rows kernel and the lattice kernel
of `mi355x_transducer_align*`, timed separately at recipe geometry and alternated in one process with the loss of the same head
without gradient (`mi355x_rnnt_loss_ex` / `mi355x_tdt_loss_ex`) on the same logits, and with `mi355x_ctc_align` at its documented
shape.  Device events around `--launches` launches, `--rounds` rounds, median and spread per entry.  Needs a GPU: no fallback.

    python tools/transducer_align_bench.py [--B 32 --T 250 --U 60 --V1 1025 --rounds 7 --launches 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("B", 32), ("T", 250), ("U", 60), ("V1", 1025), ("rounds", 7), ("launches", 20)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("transducer_align_bench needs an MI355X: a CPU run says nothing about the kernels")
    from nemo_amd import _lib, ops
    lib, dev = _lib.lib, "cuda"
    B, T, U1, V1 = a.B, a.T, a.U + 1, a.V1
    g = torch.Generator(device=dev).manual_seed(0)
    act = torch.randint(T - T // 5, T + 1, (B,), device=dev, generator=g)
    lab = torch.randint(a.U - a.U // 5, a.U + 1, (B,), device=dev, generator=g)
    labels = torch.randint(0, V1 - 1, (B, a.U), device=dev, generator=g)
    p, s = ops._ptr, ops._stream
    entries = {}
    for head, durations in (("rnnt", None), ("tdt", [0, 1, 2, 3, 4])):
        D = len(durations or [])
        W = V1 + D
        acts = torch.randn(B, T, U1, W, device=dev, generator=g)
        rows = torch.empty(B, T, U1, 2 + D, device=dev)
        nbytes = lib.mi355x_transducer_align_workspace_bytes(B, T, U1)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        tf, td = (torch.empty(B, a.U, dtype=torch.int32, device=dev) for _ in range(2))
        score, costs = torch.empty(B, device=dev), torch.empty(B, device=dev)
        dur = (_lib.C.c_int * D)(*durations) if D else None
        n_loss = (4 + 2 * D if D else 5) * B * T * U1 + 2 * B
        lws = torch.empty(n_loss, device=dev)
        entries[head + " rows kernel"] = lambda acts=acts, rows=rows, D=D, W=W: lib.mi355x_transducer_align_rows(
            p(acts), W, p(labels), p(act), p(lab), B, T, U1, V1, D, V1 - 1, p(rows), s())
        entries[head + " lattice kernel"] = lambda rows=rows, dur=dur, D=D, ws=ws: lib.mi355x_transducer_align(
            p(rows), p(act), p(lab), dur, D, B, T, U1, p(ws), nbytes, p(tf), p(td), p(score), s())
        if D:
            entries[head + " loss, no gradient"] = lambda acts=acts, dur=dur, D=D, W=W, lws=lws, n=n_loss: lib.mi355x_tdt_loss_ex(
                p(acts), W, p(labels), p(act), p(lab), B, T, U1, V1, D, dur, V1 - 1, 0.0, 1.0, p(costs), None, 0, 0, p(lws), n, s())
        else:
            entries[head + " loss, no gradient"] = lambda acts=acts, W=W, lws=lws, n=n_loss: lib.mi355x_rnnt_loss_ex(
                p(acts), W, p(labels), p(act), p(lab), B, T, U1, V1, V1 - 1, 0.0, 0.0, 1.0, p(costs), None, 0, 0, p(lws), n, s())
    Bc, Tc, Cc, Uc = 32, 501, 129, 100   # the shape profiles/ctc_align.md documents
    logp = torch.log_softmax(torch.randn(Bc, Tc, Cc, device=dev, generator=g), -1)
    ctg = torch.randint(0, Cc - 1, (Bc, Uc), device=dev, generator=g)
    cin, ctl = torch.full((Bc,), Tc, device=dev), torch.full((Bc,), Uc, device=dev)
    entries["ctc_align (B 32, T 501, C 129, U 100)"] = lambda: ops.ctc_align(logp, ctg, cin, ctl, Cc - 1) and 0
    times = {k: [] for k in entries}
    for k, fn in entries.items():   # warm-up: code objects, allocator
        for _ in range(3):
            _lib.check(fn() or 0, k)
    torch.cuda.synchronize()
    for _ in range(a.rounds):       # alternated: every round times every entry
        for k, fn in entries.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / a.launches)
    out = {k: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for k, v in times.items()}
    print(json.dumps({"shape": dict(B=B, T=T, U=a.U, V1=V1), "rounds": a.rounds, "launches": a.launches, "entries": out}, indent=1))


if __name__ == "__main__":
    main()
