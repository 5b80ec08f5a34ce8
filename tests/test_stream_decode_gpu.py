"""-m gpu: the resumable greedy transducer search (mi355x_rnnt_greedy_decode_stream / mi355x_tdt_greedy_decode_stream, csrc/
rnnt_decode.hip) and `partial_hypotheses` in the decoding objects (modules/rnnt_decoding.py).

  1. a stream cut into ANY chunks gives bit-identical tokens, frame indices, lengths, score and final (h, c, last) to one launch;
  2. against the CPU restatement (tests/stream_decode_oracle.py): fp32 exact; bf16 weight images by the forced walk with the
     rules and numbers of tests/test_rnnt_decoding.py (every differing decision within 2e-4 * scale, at most 2 % differing);
  4. GreedyBatchedRNNTInfer / GreedyBatchedTDTInfer with partial_hypotheses over three chunks against forward over the whole.
The settings (seeds, blank / duration biases) are shown to hit the hard cases on the CPU by tests/test_hybrid_host.py."""
import pytest
import torch

from oracle import transducer_ref as TR

import stream_decode_oracle as S

pytestmark = pytest.mark.gpu
dev = "cuda"
DUR = [0, 1, 2, 3, 4]


def _dev_args(Pd, Pj, wdt):
    """the search's weight arguments on the device (fp32 masters or bf16 images; biases and the embedding stay fp32)"""
    w = lambda t: t.to(dev).to(wdt).contiguous()   # noqa: E731
    f = lambda t: t.to(dev).float().contiguous()   # noqa: E731
    q = "prediction.dec_rnn.lstm."
    H = Pd[q + "weight_hh_l0"].shape[1]
    J = Pj["pred.weight"].shape[0]
    out = [k[:-len("weight")] for k in Pj if k.startswith("joint_net.") and k.endswith(".weight")][0]
    return (f(Pd["prediction.embed.weight"]), w(Pd[q + "weight_ih_l0"]), H, w(Pd[q + "weight_hh_l0"]), H, f(Pd[q + "bias_ih_l0"]),
            f(Pd[q + "bias_hh_l0"]), w(Pj["pred.weight"]), H, f(Pj["pred.bias"]), w(Pj[out + "weight"]), J,
            f(Pj[out + "bias"]))


def _run_chunked(ops, f_all, lens, args, blank, ms, edges, durations):
    """-> per-stream (tokens, times), the final state, list of (skip_out, frames_done_out) per chunk"""
    B = f_all.shape[0]
    toks, times = [[] for _ in range(B)], [[] for _ in range(B)]
    state, trail = None, []
    for lo, hi in zip(edges[:-1], edges[1:]):
        cl = (lens - lo).clamp(min=0, max=hi - lo).to(dev)
        fc = f_all[:, lo:hi].contiguous()
        if durations is None:
            tk, tm, n, state = ops.rnnt_greedy_decode_stream(fc, cl, *args, blank, ms, state=state)
        else:
            tk, tm, n, state = ops.tdt_greedy_decode_stream(fc, cl, *args, blank, durations, ms, state=state)
        tk, tm, n = tk.cpu(), tm.cpu(), n.cpu()
        for b in range(B):
            toks[b] += tk[b, : int(n[b])].tolist()
            times[b] += tm[b, : int(n[b])].tolist()
            assert (tk[b, int(n[b]):] == -1).all()
        trail.append((state.skip.cpu().clone(), state.frames_done.cpu().clone()))
    return list(zip(toks, times)), state, trail


def _cuttings(T):
    g = torch.Generator().manual_seed(77)
    rnd = sorted(set(torch.randint(1, T, (6,), generator=g).tolist()))
    return {"every frame": list(range(T + 1)), "width 5": list(range(0, T, 5)) + [T], "random": [0] + rnd + [T]}


@pytest.mark.parametrize("max_symbols", [2, 10])
@pytest.mark.parametrize("kind", ["rnnt", "tdt"])
@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16])
def test_chunked_search_equals_one_launch_bit_for_bit(wdt, kind, max_symbols):
    from nemo_amd import ops
    V, H, D, J, B, T = S.SMALL["V"], S.SMALL["H"], S.SMALL["D"], S.SMALL["J"], 4, S.SMALL["T"]
    lens = torch.tensor(S.SMALL["lens"])
    durations = DUR if kind == "tdt" else None
    Pd, Pj = S.small_case(kind)
    enc = S.small_enc()
    f_all = torch.nn.functional.linear(enc.transpose(1, 2), Pj["enc.weight"], Pj["enc.bias"]).to(dev).contiguous()
    assert 5 * 7 != T and T % 5 != 0
    args = _dev_args(Pd, Pj, wdt)
    # one launch over the whole sequence, through the resumable entry (fresh state) and through the one-shot entry
    (one, st1, _) = _run_chunked(ops, f_all, lens, args, V, max_symbols, [0, T], durations)
    if kind == "rnnt":
        tk, tm, n, sc, (h, c) = ops.rnnt_greedy_decode(f_all, lens.to(dev), *args, V, max_symbols, with_state=True)
    else:
        tk, tm, n, sc, (h, c) = ops.tdt_greedy_decode(f_all, lens.to(dev), *args, V, DUR, max_symbols, with_state=True)
    for b in range(B):
        assert tk[b, : int(n[b])].tolist() == one[b][0] and tm[b, : int(n[b])].tolist() == one[b][1], b
    assert torch.equal(sc, st1.score) and torch.equal(h, st1.h) and torch.equal(c, st1.c)
    assert st1.frames_done.tolist() == lens.tolist()
    assert sum(len(o[0]) for o in one) > 20
    per_frame = torch.cat([torch.bincount(torch.tensor(o[1], dtype=torch.long), minlength=T)[: int(n_b)] for o, n_b in zip(one, lens)])
    assert int(per_frame.max()) == max_symbols, per_frame     # a frame emitted max_symbols labels
    assert int(per_frame.min()) == 0                          # and the search is not stuck on them
    crossed = False
    for name, edges in _cuttings(T).items():
        got, st, trail = _run_chunked(ops, f_all, lens, args, V, max_symbols, edges, durations)
        assert got == one, name
        for a in ("h", "c", "last", "score", "frames_done", "skip", "zero_run"):
            assert torch.equal(getattr(st, a), getattr(st1, a)), (name, a)
        crossed |= any(bool(((skip > 0) & (done < lens)).any()) for skip, done in trail)
    if kind == "tdt":
        assert crossed   # a predicted duration jumped over a chunk edge inside an utterance
    # the shortest stream's later chunks had length 0: its state passed through, nothing was emitted
    assert one[2][1] == [] or max(one[2][1]) < int(lens[2])


def _rule2(rows_per_utt, n_labels):
    """tests/test_rnnt_decoding.py's rules for a reduced-precision search walked along the restatement"""
    decisions = [r for rows in rows_per_utt for r in rows]
    flips = [r for r in decisions if r[1] != r[2]]
    assert len(decisions) > 150 and n_labels > 40, (len(decisions), n_labels)
    for t, follow, own, margin, scale in flips:
        assert margin <= 2e-4 * scale, (t, follow, own, margin, scale)
    assert len(flips) <= 0.02 * len(decisions), (len(flips), len(decisions))
    return len(flips), len(decisions)


def _bf16_images(Pd, Pj, enc):
    rb = lambda w: w.to(torch.bfloat16).to(torch.float32)   # noqa: E731
    Pd16, Pj16 = dict(Pd), dict(Pj)
    for k in ("prediction.dec_rnn.lstm.weight_ih_l0", "prediction.dec_rnn.lstm.weight_hh_l0"):
        Pd16[k] = rb(Pd[k])
    outk = [k for k in Pj if k.startswith("joint_net.") and k.endswith(".weight")][0]
    for k in ("pred.weight", "enc.weight", outk):
        Pj16[k] = rb(Pj[k])
    f16 = rb(torch.nn.functional.linear(rb(enc.transpose(1, 2)), Pj16["enc.weight"], Pj["enc.bias"]))
    return Pd16, Pj16, f16


@pytest.mark.parametrize("kind", ["rnnt", "tdt"])
def test_stream_search_against_the_cpu_restatement_at_the_recipe_geometry(kind):
    """fp32 weights: one launch and chunked == tests/stream_decode_oracle.py exactly.  bf16 images: the device's hypotheses walked
    through the forced walk over bf16-rounded weights and projection (rule 2)."""
    from nemo_amd import ops
    R = S.RECIPE
    V, T, ms = R["V"], R["T"], R["max_symbols"]
    lens = torch.tensor(R["lens"])
    durations = DUR if kind == "tdt" else None
    Pd, Pj = S.recipe_case(kind)
    enc = S.recipe_enc()
    edges = [0, 1, 14, 27, 64, T]
    want, _, _ = S.decode_chunked(Pd, Pj, enc, lens, V, ms, edges[1:-1], durations)
    f_all = torch.nn.functional.linear(enc.transpose(1, 2), Pj["enc.weight"], Pj["enc.bias"])
    args = _dev_args(Pd, Pj, torch.float32)
    one, _, _ = _run_chunked(ops, f_all.to(dev), lens, args, V, ms, [0, T], durations)
    chk, _, _ = _run_chunked(ops, f_all.to(dev), lens, args, V, ms, edges, durations)
    assert one == want and chk == want
    assert sum(len(w[0]) for w in want) > 40
    # bf16 weight images, bf16 projection
    Pd16, Pj16, f16 = _bf16_images(Pd, Pj, enc)
    args16 = _dev_args(Pd, Pj, torch.bfloat16)
    f16d = f16.to(dev).to(torch.bfloat16)
    one16, _, _ = _run_chunked(ops, f16d, lens, args16, V, ms, [0, T], durations)
    chk16, _, _ = _run_chunked(ops, f16d, lens, args16, V, ms, edges, durations)
    assert chk16 == one16   # (chunking itself never changes a bit)
    if kind == "rnnt":
        rep = TR.forced_decode_margins(Pd16, Pj16, enc, lens, V, ms, one16, f_all=f16)
    else:
        rep = S.tdt_forced_decode_margins(Pd16, Pj16, enc, lens, V, DUR, ms, one16, f_all=f16)
    print("bf16 flips / decisions:", _rule2(rep, sum(len(o[0]) for o in one16)))


@pytest.mark.parametrize("kind", ["rnnt", "tdt"])
def test_decoder_objects_resume_from_partial_hypotheses(kind):
    """three chunks through `forward(..., partial_hypotheses=...)` against `forward` over the concatenated encoder output.  Where
    the per-chunk projection GEMM gives the same values as the whole-sequence one, the hypotheses must be EQUAL (tokens, frame
    indices, score, length); in any case the chunked hypotheses pass rule 2 against the fp32 CPU restatement.  On the MI355X the
    per-chunk projections of this case ARE bit-equal to the whole-sequence one (both kinds), so the equality branch is the one that
    ran there.  A second pass hands the decoder slices of the whole-sequence projection in place of its per-chunk GEMM: there
    equality with the one-shot call (tokens, frame indices, score, length, final h / c) is asserted unconditionally."""
    from nemo_amd.modules import GreedyBatchedRNNTInfer, GreedyBatchedTDTInfer, RNNTDecoder, RNNTJoint
    R = S.RECIPE
    V, H, D, J, T, ms = R["V"], R["H"], R["D"], R["J"], R["T"], R["max_symbols"]
    lens = torch.tensor(R["lens"])
    Pd, Pj = S.recipe_case(kind)
    enc = S.recipe_enc()
    dec = RNNTDecoder(prednet={"pred_hidden": H, "pred_rnn_layers": 1, "dropout": 0.0}, vocab_size=V, compute_dtype=torch.float32)
    joint = RNNTJoint(jointnet={"encoder_hidden": D, "pred_hidden": H, "joint_hidden": J, "activation": "relu", "dropout": 0.0},
                      num_classes=V, num_extra_outputs=len(DUR) if kind == "tdt" else 0, compute_dtype=torch.float32)
    dec.load_state_dict(Pd); joint.load_state_dict(Pj)
    dec, joint = dec.to(dev).eval(), joint.to(dev).eval()
    if kind == "tdt":
        infer = GreedyBatchedTDTInfer(dec, joint, V, DUR, max_symbols_per_step=ms)
    else:
        infer = GreedyBatchedRNNTInfer(dec, joint, V, max_symbols_per_step=ms)
    encd = enc.to(dev)
    whole = infer(encoder_output=encd, encoded_lengths=lens.to(dev))[0]
    edges = [0, 33, 66, T]
    assert isinstance(whole[0].dec_state, tuple) and len(whole[0].dec_state) == 2   # the one-shot call is what it was: final (h, c)
    with pytest.raises(ValueError, match="fresh_hypotheses"):   # and its hypotheses are not a stream to resume
        infer(encoder_output=encd[:, :, :4].contiguous(), encoded_lengths=lens.clamp(max=4).to(dev), partial_hypotheses=whole)
    hyps, same_proj = infer.fresh_hypotheses(len(lens)), True
    assert all(h.length == 0 and h.timestamp == [] and h.y_sequence.numel() == 0 for h in hyps)
    f_whole, _ = infer._project(encd)
    for lo, hi in zip(edges[:-1], edges[1:]):
        cl = (lens - lo).clamp(min=0, max=hi - lo).to(dev)
        chunk = encd[:, :, lo:hi].contiguous()
        before = None if hyps is None else [(h.y_sequence.clone(), list(h.timestamp), h.score, h.dec_state.h.clone()) for h in hyps]
        new = infer(encoder_output=chunk, encoded_lengths=cl, partial_hypotheses=hyps)[0]
        if hyps is not None:   # new objects; the inputs are as they were
            for h, n, (y, ts, sc, hh) in zip(hyps, new, before):
                assert h is not n and h.dec_state is not n.dec_state
                assert torch.equal(h.y_sequence, y) and h.timestamp == ts and h.score == sc and torch.equal(h.dec_state.h, hh)
        same_proj &= torch.equal(infer._project(chunk)[0], f_whole[:, lo:hi])
        hyps = new
    got = [(h.y_sequence.tolist(), h.timestamp) for h in hyps]
    for b, (h, w) in enumerate(zip(hyps, whole)):
        assert h.length == int(lens[b]) == w.length
        assert h.dec_state.h.is_cuda and h.last_token.is_cuda and int(h.last_token) == (got[b][0][-1] if got[b][0] else V)
        if same_proj:
            assert got[b] == (w.y_sequence.tolist(), w.timestamp) and h.score == w.score, b
    # the same three calls with the projection step handing out slices of the whole-sequence projection: equality, unconditionally
    _, args = infer._project(encd)
    project = infer._project
    hyps2 = infer.fresh_hypotheses(len(lens))
    try:
        for lo, hi in zip(edges[:-1], edges[1:]):
            infer._project = lambda chunk, lo=lo, hi=hi: (f_whole[:, lo:hi].contiguous(), args)
            cl = (lens - lo).clamp(min=0, max=hi - lo).to(dev)
            hyps2 = infer(encoder_output=encd[:, :, lo:hi].contiguous(), encoded_lengths=cl, partial_hypotheses=hyps2)[0]
    finally:
        infer._project = project
    for b, (h, w) in enumerate(zip(hyps2, whole)):
        assert h.y_sequence.tolist() == w.y_sequence.tolist() and h.timestamp == w.timestamp and h.score == w.score, b
        assert h.length == w.length and torch.equal(h.dec_state.h[0], w.dec_state[0]) and torch.equal(h.dec_state.c[0], w.dec_state[1])
    if kind == "rnnt":
        rep = TR.forced_decode_margins(Pd, Pj, enc, lens, V, ms, got)
    else:
        rep = S.tdt_forced_decode_margins(Pd, Pj, enc, lens, V, DUR, ms, got)
    print("per-chunk projection equals the whole-sequence one:", same_proj, "flips / decisions:",
          _rule2(rep, sum(len(g[0]) for g in got)))
