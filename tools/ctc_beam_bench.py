"""CTC prefix beam search on one GPU (profiles/ctc_beam.md is made with this).

Per shape (B, T, C), beam width W and threshold, `--rounds` rounds; in every round each candidate runs its launches between two
device events, the candidates alternating inside the round (same process, same buffers; every other round in reverse order), so
that drift of the box hits all of them alike:
  * mi355x_ctc_beam_decode for every (W, threshold) asked for,
  * with `--lm ORDER` mi355x_ctc_beam_decode_lm at the same settings with the n-gram model of the tests' generator
    (tests/ctc_beam_lm_oracle.py `make_lm(0, C-1, ORDER)`, through ARPA text and NGramLM.from_arpa) at `--alpha`, and once more at
    alpha = 0: the same selections as the LM-less search, so the difference to it is what carrying the LM state costs, and the rest
    of the fused time is look-ups and the candidates they let in,
  * mi355x_ctc_greedy_decode at the same shape: the scale (one pass over the log-probabilities, no search),
  * mi355x_ctc_greedy_decode, mi355x_ctc_greedy_decode_ts and mi355x_ctc_beam_decode of every library given with `--lib name=path`
    (e.g. a build of the parent commit), alternating with the in-tree library's: the spread between builds of entry points a
    change does not touch.
  * with `--stream CHUNK` the resumable entries (mi355x_ctc_beam_decode_stream, with --lm also mi355x_ctc_beam_decode_lm_stream)
    over the same T frames cut into chunks of CHUNK frames, one candidate = the whole utterance: every step carries the state
    through device arrays and appends to a tree of T frames; `emit=all` chases the n-best out on every chunk, `emit=last` on the
    last one only.  Next to the one-shot time, the difference is launches + state load and store + the chases.
  * with `--boost N` mi355x_ctc_beam_decode_fused with a boosting tree of N key phrases (runs of 2..4 tokens cut from the arg-max
    paths of the input itself, so that they are begun and completed) at `--boost-alpha`, alone and, with --lm, beside the n-gram
    model (two fusion models); with --lm and --lib also mi355x_ctc_beam_decode_lm of the other builds.
  * with --stream and --lib also the resumable entries of the other builds, alternating with the in-tree library's.
  * with `--commit` (instead of all of the above; profiles/ctc_beam_commit.md is made with it) mi355x_ctc_beam_commit alone, on the
    states that `--commit-windows` frames of the stream leave, exact and forced with `--stable-frames`; and the whole stream through
    the decoding object (`nbest_stream`: search, chase and the D2H copy of the n-best) in chunks of --stream frames (14 if not
    given), without a commit and with `commit_stream` after every `--commit-every`-th chunk: wall time per step (host lists
    included) at the head (steps 3 to 8) and at the tail (the six steps before the last) of the stream, the D2H bytes of those
    steps, between device events the step's search alone and what chasing the n-best out adds, and the capacity the tree ended with.
Input: log-softmax of 1.5 * N(0,1) with +5 on the class of a random path (blank with probability 0.6), the generator of the tests --
peaked like a trained model's output, so that the threshold prunes; lengths = T.  The launches of a candidate per round are sized
from one timed launch so that a round of it takes about `--round-ms`.  Reported per candidate: median, min and max of the
per-round means, in microseconds per launch.

    python tools/ctc_beam_bench.py [--shapes 32,501,129 32,501,1025] [--beams 4 16 64] [--thresholds 20 inf] [--rounds 7]
                                   [--lm ORDER] [--alpha 0.5] [--stream CHUNK] [--boost N] [--boost-alpha 1.0]
                                   [--lib parent=PATH ...] [--json OUT]
                                   [--commit [--commit-windows 28 280] [--stable-frames 28] [--commit-every 2]]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

dev = "cuda"
GREEDY = ("mi355x_ctc_greedy_decode", "mi355x_ctc_greedy_decode_ts")
BEAM = "mi355x_ctc_beam_decode"
BEAM_LM = "mi355x_ctc_beam_decode_lm"
STREAMED = ("mi355x_ctc_beam_decode_stream", "mi355x_ctc_beam_decode_lm_stream")


def load(path):
    from nemo_amd import _lib
    lib = ctypes.CDLL(path)
    for name in GREEDY + (BEAM, BEAM_LM) + STREAMED:
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
    for r in range(n_rounds):   # every other round backwards: no candidate always runs behind the same neighbour
        for k in (list(cands) if r % 2 == 0 else list(cands)[::-1]):
            per[k].append(timed(cands[k], iters[k]))
    return {k: dict(median_us=round(statistics.median(v), 1), min_us=round(min(v), 1), max_us=round(max(v), 1), iters=iters[k])
            for k, v in per.items()}


def make_logp(B, T, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, C, generator=g) * 1.5
    path = torch.where(torch.rand(B, T, generator=g) < 0.6, torch.full((B, T), C - 1), torch.randint(0, C - 1, (B, T), generator=g))
    x.scatter_add_(2, path.unsqueeze(-1), torch.full((B, T, 1), 5.0))
    return torch.log_softmax(x, -1).to(dev)


def make_ngram_lm(V, order):
    """the tests' model, written as ARPA text and read back the way a user's model is"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import ctc_beam_lm_oracle as L
    from nemo_amd.modules import NGramLM
    with tempfile.TemporaryDirectory() as d:
        L.write_arpa(L.make_lm(0, V, order), os.path.join(d, "lm.arpa"))
        return NGramLM.from_arpa(os.path.join(d, "lm.arpa"), V)


def make_boosting_tree(logp, n_phrases, seed=0):
    """n_phrases runs of 2..4 tokens from the collapsed arg-max paths of the input, as a BoostingTree"""
    from nemo_amd.modules import BoostingTree
    C = logp.shape[2]
    g = torch.Generator().manual_seed(seed)
    paths = []
    for row in logp.argmax(-1).cpu().tolist():
        ids, prev = [], None
        for c in row:
            if c != prev and c != C - 1:
                ids.append(c)
            prev = c
        paths.append(ids)
    paths = [x for x in paths if len(x) >= 4]
    phrases, tries = [], 0
    while len(phrases) < n_phrases and tries < 100 * n_phrases:
        tries += 1
        ids = paths[int(torch.randint(len(paths), (1,), generator=g))]
        n = int(torch.randint(2, 5, (1,), generator=g))
        a = int(torch.randint(0, len(ids) - n + 1, (1,), generator=g))
        if tuple(ids[a:a + n]) not in phrases:
            phrases.append(tuple(ids[a:a + n]))
    return BoostingTree.from_phrases(phrases, C - 1)


def one_shape(B, T, C, beams, thresholds, libs, n_rounds, round_ms, lm_order=0, alpha=0.5, chunk=0, boost=0, boost_alpha=1.0):
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

    def beam(W, th, l=lib):
        def fn():
            rc = l.mi355x_ctc_beam_decode(p(logp), p(lens), p(ws), p(tokens), p(frames), p(hyp_len), p(score), p(n_hyp), B, T, C, C - 1,
                                          W, th, 0.0, stream)
            assert rc == 0, rc
        return fn

    lm = make_ngram_lm(C - 1, lm_order) if lm_order else None
    tables = [p(t) for t in lm.to(dev)[:6]] if lm else None

    def beam_lm(W, th, a, l=lib):
        def fn():
            rc = l.mi355x_ctc_beam_decode_lm(p(logp), p(lens), p(ws), p(tokens), p(frames), p(hyp_len), p(score), p(n_hyp), B, T, C,
                                               C - 1, W, th, 0.0, *tables, lm.num_states, lm.num_arcs, a, lm.lm_ub, stream)
            assert rc == 0, rc
        return fn

    tree = make_boosting_tree(logp, boost) if boost else None

    def beam_fused(W, th, models):
        """mi355x_ctc_beam_decode_fused with `models` = [(NGramLM | BoostingTree, alpha), ...]"""
        from nemo_amd.ops import _ctc_beam_fusion_array
        arr, keep = _ctc_beam_fusion_array(models, logp)

        def fn():
            rc = lib.mi355x_ctc_beam_decode_fused(p(logp), p(lens), p(ws), p(tokens), p(frames), p(hyp_len), p(score), p(n_hyp), B, T, C,
                                                  C - 1, W, th, 0.0, ctypes.cast(arr, ctypes.c_void_p), len(arr), stream)
            assert rc == 0, rc
        fn._keep = (arr, keep)
        return fn

    chunks = [logp[:, t:t + chunk].contiguous() for t in range(0, T, chunk)] if chunk else []
    chunk_lens = {n: torch.full((B,), n, dtype=torch.int64, device=dev) for n in {c.shape[1] for c in chunks}}

    def streamed(W, th, emit_all, a=None, lib=lib):
        """the utterances in chunks through the resumable entry (of `lib`): two states written in turn, a tree of T frames"""
        from nemo_amd.modules import CTCBeamStreamState
        from nemo_amd.ops import _CTCBeamStateC
        st = [CTCBeamStreamState.fresh(B, W, dev, capacity=T, lm=a is not None) for _ in range(2)]
        cs = [_CTCBeamStateC.of(x) for x in st]
        outs = (p(st[0].tokens), p(st[0].tok_frame), p(hyp_len), p(score), p(n_hyp))

        def fn():
            for i, c in enumerate(chunks):
                n = c.shape[1]
                o = outs if emit_all or i == len(chunks) - 1 else (None,) * 5
                head = (p(c), p(chunk_lens[n]), p(st[0].tree), *o, B, n, C, C - 1, W, th, 0.0)
                tail = (T, ctypes.byref(cs[(i + 1) & 1]) if i else None, ctypes.byref(cs[i & 1]), stream)
                if a is None:
                    rc = lib.mi355x_ctc_beam_decode_stream(*head, *tail)
                else:
                    rc = lib.mi355x_ctc_beam_decode_lm_stream(*head, *tables, lm.num_states, lm.num_arcs, a, lm.lm_ub, *tail)
                assert rc == 0, rc
        fn._keep = st
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
            for name, l in libs.items():
                cands[f"beam[{name}] W={W} threshold={th}"] = beam(W, th, l)
            if lm:
                cands[f"beam+lm W={W} threshold={th} alpha={alpha}"] = beam_lm(W, th, alpha)
                cands[f"beam+lm W={W} threshold={th} alpha=0"] = beam_lm(W, th, 0.0)
                for name, l in libs.items():
                    cands[f"beam+lm[{name}] W={W} threshold={th} alpha={alpha}"] = beam_lm(W, th, alpha, l)
            if tree:
                cands[f"beam+boost W={W} threshold={th} alpha={boost_alpha}"] = beam_fused(W, th, [(tree, boost_alpha)])
                if lm:
                    cands[f"beam+lm+boost W={W} threshold={th} alpha={alpha},{boost_alpha}"] = beam_fused(W, th, [(lm, alpha),
                                                                                                               (tree, boost_alpha)])
            if chunk:
                for emit_all in (True, False):
                    tag = f"W={W} threshold={th} chunk={chunk} emit={'all' if emit_all else 'last'}"
                    cands[f"stream {tag}"] = streamed(W, th, emit_all)
                    for name, l in libs.items():
                        cands[f"stream[{name}] {tag}"] = streamed(W, th, emit_all, lib=l)
                    if lm:
                        cands[f"stream+lm {tag} alpha={alpha}"] = streamed(W, th, emit_all, alpha)
                        for name, l in libs.items():
                            cands[f"stream+lm[{name}] {tag} alpha={alpha}"] = streamed(W, th, emit_all, alpha, lib=l)
    row = dict(shape=dict(B=B, T=T, C=C), **rounds(cands, n_rounds, round_ms))
    if lm:
        row["lm"] = dict(order=lm.order, states=lm.num_states, arcs=lm.num_arcs, lm_ub=lm.lm_ub)
        # what the fusion changed at the widest setting: utterances whose best hypothesis differs from the LM-less search's
        beam(Wmax, thresholds[0])()
        torch.cuda.synchronize()
        t0, l0 = tokens.clone(), hyp_len.clone()
        beam_lm(Wmax, thresholds[0], alpha)()
        torch.cuda.synchronize()
        row["best_changed_by_lm"] = f"{sum(int(l0[b, 0]) != int(hyp_len[b, 0]) or not torch.equal(t0[b, 0], tokens[b, 0]) for b in range(B))}/{B}"
    if tree:
        row["boost"] = dict(phrases=len(tree.phrases), states=tree.num_states, arcs=tree.num_arcs, ub=tree.lm_ub)
        beam(Wmax, thresholds[0])()
        torch.cuda.synchronize()
        t0, l0 = tokens.clone(), hyp_len.clone()
        beam_fused(Wmax, thresholds[0], [(tree, boost_alpha)])()
        torch.cuda.synchronize()
        row["best_changed_by_boost"] = f"{sum(int(l0[b, 0]) != int(hyp_len[b, 0]) or not torch.equal(t0[b, 0], tokens[b, 0]) for b in range(B))}/{B}"
    # what the search found at the widest setting: hypotheses per utterance and how often the best one differs from the greedy one
    beam(Wmax, thresholds[0])(); greedy(lib, False)()
    torch.cuda.synchronize()
    same = sum(int(hyp_len[b, 0]) == int(glen[b]) and torch.equal(tokens[b, 0, : int(glen[b])], gtok[b, : int(glen[b])]) for b in range(B))
    row["n_hyp_mean"] = float(n_hyp.float().mean())
    row["best_equals_greedy"] = f"{same}/{B}"
    return row


def commit_shape(B, T, C, beams, n_rounds, round_ms, chunk, windows, stable, every):
    """--commit: the kernel alone on the states of `windows` frames, and the stream with and without commits"""
    from nemo_amd import _lib, ops
    from nemo_amd.modules import BeamBatchedCTCDecoder, CTCBeamStreamState
    from nemo_amd.ops import _CTCBeamFusedStateC, _CTCBeamWindowC
    lib = _lib.lib
    logp = make_logp(B, T, C)
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()   # noqa: E731
    i32 = dict(dtype=torch.int32, device=dev)
    row, cands, notes = dict(shape=dict(B=B, T=T, C=C)), {}, {}
    for W in beams:
        for n in windows:
            n = min(n, T)
            _, st = ops.ctc_beam_decode_stream(logp[:, :n].contiguous(), None, C - 1, W, 20.0, 0.0,
                                               CTCBeamStreamState.fresh(B, W, dev, capacity=n), emit=False)
            for S in (-1, stable):
                out = CTCBeamStreamState.fresh(B, W, dev, capacity=n)
                out.win, out.frame_map = torch.zeros(4, B, **i32), torch.zeros(B, n, **i32)
                com, ws = torch.empty(2, B, n, **i32), torch.empty(B * int(lib.mi355x_ctc_beam_commit_workspace_elems(n, W)), **i32)
                args = (_CTCBeamFusedStateC.of(st), _CTCBeamWindowC.of(st), _CTCBeamFusedStateC.of(out), _CTCBeamWindowC.of(out))

                def fn(st=st, out=out, com=com, ws=ws, args=args, W=W, n=n, S=S):
                    rc = lib.mi355x_ctc_beam_commit(ctypes.byref(args[0]), ctypes.byref(args[1]), p(st.tree), ctypes.byref(args[2]),
                                                    ctypes.byref(args[3]), p(out.tree), p(com[0]), p(com[1]), p(out.win[3]), p(ws), B, W,
                                                    n, 0, S, stream)
                    assert rc == 0, rc
                key = f"commit W={W} window={n} {'exact' if S < 0 else f'stable={S}'}"
                cands[key] = fn
                fn()
                torch.cuda.synchronize()
                notes[key] = dict(kept_max=int(out.win[2].max()), committed_mean=float(out.win[3].float().mean()),
                                  nb_mean=float(out.utt[0].float().mean()))
    row.update(rounds(cands, n_rounds, round_ms))
    for k, v in notes.items():
        row[k].update(v)
    # the whole stream through the decoding object
    chunks = [logp[:, t:t + chunk].contiguous() for t in range(0, T, chunk)]
    for W in beams:
        dec = BeamBatchedCTCDecoder(vocabulary=[str(i) for i in range(C - 1)], beam_size=W, return_best_hypothesis=False)
        for tag, commit in (("plain", False), (f"commit_every={every} stable={stable}", True)):
            per_round = []
            for r in range(n_rounds + 1):   # (round 0: warm-up)
                state, steps, d2h, search, chase = None, [], [], [], []
                for i, c in enumerate(chunks):
                    # on the device alone (a step is out of place, so it can be repeated): the search of this step without and
                    # with the n-best chased out
                    quiet = timed(lambda: dec.decode_stream(c, None, state, emit=False), 3)
                    search.append(quiet)
                    chase.append(timed(lambda: dec.decode_stream(c, None, state, emit=True), 3) - quiet)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    hyps, state = dec.nbest_stream(c, None, state)
                    # what nbest_stream copied: two [B, K, L] slices (L: the longest tail) and hyp_len, score, n_hyp
                    tail = max(len(ids) - len(state.committed[b][0]) for b, h in enumerate(hyps) for ids, _, _ in h)
                    nbytes = 2 * 4 * B * max(len(h) for h in hyps) * tail + 4 * B * (2 * W + 1)
                    if commit and (i + 1) % every == 0:
                        new, state = dec.commit_stream(state, stable)
                        nbytes += 4 * 4 * B + 2 * 4 * B * max(len(x[0]) for x in new)
                    torch.cuda.synchronize()
                    steps.append((time.perf_counter() - t0) * 1e6)
                    d2h.append(nbytes)
                if r:
                    per_round.append(dict(total_ms=sum(steps) / 1e3, head_us=statistics.mean(steps[2:8]), tail_us=statistics.mean(steps[-7:-1]),
                                          d2h_head=statistics.mean(d2h[2:8]), d2h_tail=statistics.mean(d2h[-7:-1]),
                                          search_head=statistics.mean(search[2:8]), search_tail=statistics.mean(search[-7:-1]),
                                          chase_head=statistics.mean(chase[2:8]), chase_tail=statistics.mean(chase[-7:-1])))
            med = lambda k: round(statistics.median(x[k] for x in per_round), 1)   # noqa: E731
            row[f"stream W={W} chunk={chunk} {tag}"] = dict(
                total_ms=med("total_ms"), total_ms_min=round(min(x["total_ms"] for x in per_round), 1),
                total_ms_max=round(max(x["total_ms"] for x in per_round), 1), step_us_head=med("head_us"), step_us_tail=med("tail_us"),
                d2h_bytes_head=med("d2h_head"), d2h_bytes_tail=med("d2h_tail"), capacity=state.capacity,
                search_us_head=med("search_head"), search_us_tail=med("search_tail"), chase_us_head=med("chase_head"),
                chase_us_tail=med("chase_tail"),
                chase_us_tail_range=[round(f(x["chase_tail"] for x in per_round), 1) for f in (min, max)],
                committed_mean=statistics.mean(len(x[0]) for x in state.committed))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["32,501,129", "32,501,1025"])
    ap.add_argument("--beams", nargs="+", type=int, default=[4, 16, 64])
    ap.add_argument("--thresholds", nargs="+", type=float, default=[20.0, float("inf")])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--round-ms", type=float, default=50.0)
    ap.add_argument("--lm", type=int, default=0, metavar="ORDER", help="also time the search with an n-gram model of this order fused")
    ap.add_argument("--alpha", type=float, default=0.5, help="the fusion weight of the --lm runs")
    ap.add_argument("--stream", type=int, default=0, metavar="CHUNK", help="also time the resumable search over chunks of CHUNK frames")
    ap.add_argument("--boost", type=int, default=0, metavar="N", help="also time the search with a boosting tree of N key phrases")
    ap.add_argument("--boost-alpha", type=float, default=1.0, help="the weight of the --boost runs")
    ap.add_argument("--commit", action="store_true", help="time mi355x_ctc_beam_commit and the stream with and without commits")
    ap.add_argument("--commit-windows", nargs="+", type=int, default=[28, 280], help="frames in the tree when the commit is timed")
    ap.add_argument("--stable-frames", type=int, default=28)
    ap.add_argument("--commit-every", type=int, default=2)
    ap.add_argument("--lib", nargs="*", default=[], help="name=path of further builds of the library")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    libs = {a.split("=", 1)[0]: load(a.split("=", 1)[1]) for a in args.lib}
    out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, round_ms=args.round_ms, shapes=[])
    for s in args.shapes:
        B, T, C = (int(x) for x in s.split(","))
        if args.commit:
            row = commit_shape(B, T, C, args.beams, args.rounds, args.round_ms, args.stream or 14, args.commit_windows, args.stable_frames,
                               args.commit_every)
            out["shapes"].append(row)
            print(json.dumps(row), flush=True)
            continue
        row = one_shape(B, T, C, args.beams, args.thresholds, libs, args.rounds, args.round_ms, args.lm, args.alpha, args.stream, args.boost,
                        args.boost_alpha)
        out["shapes"].append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
