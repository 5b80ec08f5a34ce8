"""Time the greedy searches (RNN-T and TDT, one-shot and resumable from a fresh state) of ONE library build, chosen per process
through MI355X_ASR_LIB (default: the in-tree library; `tools/ab_build.py` builds variants).  Loads the library with ctypes
directly: a build that exports mi355x_transducer_greedy_decode is called through its descriptor, an older one through the
positional entries it has (the resumable rows only where it has them), so both can be timed.  B = 32, T = 250, H = J = 640, V1 = 1025, bf16 weights,
seeded random weights and projection (the same work in every process).  Prints one JSON line; alternate processes of the
builds to compare inside one GPU session, and a build against itself for the spread.

    MI355X_ASR_LIB=nemo_amd/lib_ab/libmi355x_asr_parent.so python tools/decode_ab.py [--iters 20] [--warmup 3]
"""
import argparse
import ctypes as C
import json
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, i32, i64 = C.c_void_p, C.c_int, C.c_longlong
HEAD = [vp, i32, i64, vp, vp, vp, i64, vp, i64, vp, vp, vp, i64, vp, vp, i64, vp, i32, i32, i32, i32, i32, i32]
TAIL = [i32, i32, vp, vp, vp, vp, i32, vp, vp, vp]
STAIL = [i32, i32, vp, vp, vp, i32, vp, vp, vp]   # the resumable forms: no score / h / c, state_in and state_out instead


class StreamState(C.Structure):   # mi355x_rnnt_stream_state
    _fields_ = [(n, vp) for n in ("h", "c", "last", "score", "frames_done", "skip", "zero_run")]


class GreedyDesc(C.Structure):   # mi355x_transducer_greedy_desc
    _fields_ = ([(n, vp) for n in ("enc_proj", "enc_len", "emb", "w_ih", "w_hh", "w_pred", "w_out", "b_ih", "b_hh", "b_pred", "b_out",
                                   "durations", "tokens", "times", "out_len", "score", "h_out", "c_out", "state_in", "state_out",
                                   "conf", "tok_conf", "models", "m_state_in", "m_state_out")]
                + [(n, i64) for n in ("ldf", "ld_ih", "ld_hh", "ld_pred", "ld_out")]
                + [(n, i32) for n in ("f_dtype", "w_dtype", "B", "T", "J", "H", "V1", "blank", "max_symbols", "max_out", "D",
                                      "n_models")])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    path = os.environ.get("MI355X_ASR_LIB", os.path.join(ROOT, "nemo_amd", "lib", "libmi355x_asr.so"))
    lib = C.CDLL(path)
    dev = "cuda"
    B, T, H, J, V1, D, ms = 32, 250, 640, 640, 1025, 5, 10
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s, k=1.0: torch.randn(*s, device=dev, generator=g) * k   # noqa: E731
    f = r(B, T, J, k=1.5).to(torch.bfloat16)
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)
    emb = r(V1, H)
    emb[V1 - 1] = 0.0
    bf = lambda t: t.to(torch.bfloat16).contiguous()   # noqa: E731
    w_ih, w_hh, w_pred = bf(r(4 * H, H, k=0.15)), bf(r(4 * H, H, k=0.15)), bf(r(J, H, k=0.15))
    b_ih, b_hh, b_pred = r(4 * H, k=0.1), r(4 * H, k=0.1), r(J, k=0.1)
    w_out, b_out = bf(r(V1 + D, J, k=0.15)), r(V1 + D, k=0.1)
    b_out[V1 - 1] += 2.0
    max_out = T * ms
    tokens = torch.empty(B, max_out, dtype=torch.int32, device=dev)
    times = torch.empty_like(tokens)
    out_len = torch.empty(B, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    p = lambda t: t.data_ptr()   # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    dur = (C.c_int * D)(0, 1, 2, 3, 4)
    st = [torch.empty(B, H, device=dev), torch.empty(B, H, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
          torch.empty(B, device=dev)] + [torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3)]
    sout = StreamState(*(p(t) for t in st))
    if hasattr(lib, "mi355x_transducer_greedy_decode"):   # the descriptor entry: one call, four settings
        lib.mi355x_transducer_greedy_decode.argtypes = [C.POINTER(GreedyDesc), vp]

        def desc(tdt, resumable):
            d = GreedyDesc(enc_proj=p(f), f_dtype=1, ldf=J, enc_len=p(lens), emb=p(emb), w_ih=p(w_ih), ld_ih=H, w_hh=p(w_hh), ld_hh=H,
                           b_ih=p(b_ih), b_hh=p(b_hh), w_pred=p(w_pred), ld_pred=H, b_pred=p(b_pred), w_out=p(w_out), ld_out=J,
                           b_out=p(b_out), w_dtype=1, B=B, T=T, J=J, H=H, V1=V1, blank=V1 - 1, max_symbols=ms, max_out=max_out,
                           tokens=p(tokens), times=p(times), out_len=p(out_len))
            if tdt:
                d.D, d.durations = D, C.addressof(dur)
            if resumable:   # from fresh streams; no score / h / c, as the former resumable entries
                d.state_out = C.addressof(sout)
            else:
                d.score = p(score)
            return d

        descs = {"rnnt": desc(False, False), "tdt": desc(True, False), "rnnt_stream": desc(False, True), "tdt_stream": desc(True, True)}
        calls = {k: (lambda d=d: lib.mi355x_transducer_greedy_decode(C.byref(d), stream)) for k, d in descs.items()}
    else:   # a build from before the descriptor: its positional entries
        lib.mi355x_rnnt_greedy_decode.argtypes = HEAD + TAIL
        lib.mi355x_tdt_greedy_decode.argtypes = HEAD + [i32, vp] + TAIL
        head = (p(f), 1, J, p(lens), p(emb), p(w_ih), H, p(w_hh), H, p(b_ih), p(b_hh), p(w_pred), H, p(b_pred), p(w_out), J, p(b_out),
                1, B, T, J, H, V1)
        tail = (V1 - 1, ms, p(tokens), p(times), p(out_len), p(score), max_out, None, None, stream)
        calls = {"rnnt": lambda: lib.mi355x_rnnt_greedy_decode(*head, *tail),
                 "tdt": lambda: lib.mi355x_tdt_greedy_decode(*head, D, dur, *tail)}
        if hasattr(lib, "mi355x_rnnt_greedy_decode_stream"):
            lib.mi355x_rnnt_greedy_decode_stream.argtypes = HEAD + STAIL
            lib.mi355x_tdt_greedy_decode_stream.argtypes = HEAD + [i32, vp] + STAIL
            stail = (V1 - 1, ms, p(tokens), p(times), p(out_len), max_out, None, C.byref(sout), stream)
            calls["rnnt_stream"] = lambda: lib.mi355x_rnnt_greedy_decode_stream(*head, *stail)
            calls["tdt_stream"] = lambda: lib.mi355x_tdt_greedy_decode_stream(*head, D, dur, *stail)
    row = {"lib": os.path.basename(path)}
    for name, fn in calls.items():
        for _ in range(args.warmup):
            assert fn() == 0
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        row[name + "_ms"] = round(e0.elapsed_time(e1) / args.iters, 4)
        row[name + "_labels"] = int(out_len.sum())
        row[name + "_checksum"] = int(tokens.clamp(min=0).sum())
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
