"""-m gpu: confidence estimation in greedy CTC / RNN-T / TDT decoding (mi355x_ctc_greedy_decode_conf, csrc/ctc.hip; the CONF
instantiations of the greedy search, csrc/rnnt_decode.hip) against the float64 restatement (tests/confidence_oracle.py), and through
the decoding objects and models.

Tolerance: per case the restatement is also run in float32 on the same inputs; e32 = its largest absolute difference to the
float64 result (reference against reference, never the device).  The device must be within max(8 * e32, 16 * 2^-23): the margin
covers its summation order (64 strided lanes and shuffles against numpy's pairwise sums) and its expf / logf, the floor is 16 ulps
of an O(1) value.  Every case prints its measured error in front of the assertion (profiles/confidence.md records them)."""
import functools

import numpy as np
import pytest
import torch

import confidence_oracle as CO
import stream_decode_oracle as S

pytestmark = pytest.mark.gpu
dev = "cuda"
DUR = [0, 1, 2, 3, 4]
FLOOR = 16 * 2.0 ** -23
METHODS = [("max_prob", "tsallis"), ("entropy", "gibbs"), ("entropy", "tsallis"), ("entropy", "renyi")]
NORMS = ["lin", "exp"]
ALPHAS = [0.33, 1.0, 2.0]
AGGS = ["mean", "min", "max", "prod"]


def _method(name, etype, alpha, norm):
    from nemo_amd.modules import ConfidenceMethodConfig
    return ConfidenceMethodConfig(name=name, entropy_type=etype, alpha=alpha, entropy_norm=norm)


# ------------------------------------------------------------------------------------------------------------------ CTC
CTC_B, CTC_T, CTC_LENS = 4, 70, [70, 64, 1, 0]
# + 6 against noise of deviation 3 wins a frame about every second time: the seeds are those at which the arg-max sequences have
# the runs the case is about (asserted where the case is built, on the CPU)
CTC_SEEDS = {37: 5, 129: 22}


@functools.lru_cache(maxsize=None)
def _ctc_logp(C):
    """log_softmax of seeded random logits x 3 with + 6 on a label that changes every 5 frames (on blank every third block):
    repeats, blank gaps and a run across frames 63 / 64; two frames with eight classes at -inf.
    -> (logp f32 [B, T, C], lens, the arg-max labels of every utterance's valid frames)"""
    g = torch.Generator().manual_seed(CTC_SEEDS[C])
    z = torch.randn(CTC_B, CTC_T, C, generator=g, dtype=torch.float64) * 3
    blank = C - 1
    for b in range(CTC_B):
        for t in range(CTC_T):
            j = t // 5
            z[b, t, blank if j % 3 == 2 else (5 * (j // 2) + b) % (C - 1)] += 6.0
    logp = torch.log_softmax(z, -1).to(torch.float32)
    for b, t in ((0, 10), (1, 63)):
        k = int(logp[b, t].argmax())
        logp[b, t, [(k + 1 + i) % C for i in range(8)]] = -float("inf")
    labels = [logp[b, : CTC_LENS[b]].argmax(-1).tolist() for b in range(CTC_B)]
    runs = [CO.ctc_fold(l, blank) for l in labels]
    assert any(s <= 63 < e for r in runs[:1] for _, s, e in r)                                    # a run across the 64-frame group
    assert any(a == c for r in runs for (a, _, _), (c, _, _) in zip(r, r[1:]))                    # a token repeated behind a gap
    assert any(e + 1 < s for r in runs for (_, _, e), (_, s, _) in zip(r, r[1:]))                 # blank frames between tokens
    assert any(e - s >= 2 for r in runs for _, s, e in r)                                         # a run of several frames
    return logp, torch.tensor(CTC_LENS, dtype=torch.int64), labels


@functools.lru_cache(maxsize=None)
def _ctc_case(C):
    """-> (logp, lens, what mi355x_ctc_greedy_decode_ts gives for them, the arg-max labels): computed once per C"""
    from nemo_amd import ops
    logp, lens, labels = _ctc_logp(C)
    ts = tuple(x.cpu() for x in ops.ctc_greedy_decode_ts(logp.to(dev), lens.to(dev), C - 1))
    return logp, lens, ts, labels


@pytest.mark.parametrize("C", [37, 129])
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("name,etype", METHODS)
def test_ctc_confidence_against_float64(name, etype, norm, alpha, C):
    from nemo_amd import ops
    from nemo_amd.modules.confidence import AGGREGATIONS
    combo = NORMS.index(norm) * len(ALPHAS) + ALPHAS.index(alpha) + (2 if C == 129 else 0)   # per method: all four aggregations,
    how, exclude_blank = AGGS[combo % 4], bool((combo // 2) % 2)                                # both exclude_blank values
    cfg = _method(name, etype, alpha, norm)
    logp, lens, ts, labels = _ctc_case(C)
    blank = C - 1
    got = [x.cpu() for x in ops.ctc_greedy_decode_conf(logp.to(dev), lens.to(dev), blank, cfg.kernel_args(C), AGGREGATIONS[how],
                                                       exclude_blank)]
    for a, w, what in zip(got[:5], ts, ("tokens", "out_len", "score", "tok_start", "tok_end")):
        assert torch.equal(a, w), what
    tokens, out_len, _, tok_start, tok_end, frame_conf, tok_conf = got
    assert out_len.tolist()[2:] in ([0, 0], [1, 0]) and int(out_len.sum()) > 20
    x = logp.numpy()
    err_f = err_t = e32 = 0.0
    for b in range(CTC_B):
        T, n = CTC_LENS[b], int(out_len[b])
        # padding
        assert (frame_conf[b, T:] == 0.0).all() and (tok_conf[b, n:] == 0.0).all()
        assert (tokens[b, n:] == -1).all() and (tok_start[b, n:] == -1).all() and (tok_end[b, n:] == -1).all()
        if T == 0:
            continue
        f64, f32 = CO.frame_confidence(x[b, :T], cfg), CO.frame_confidence(x[b, :T], cfg, dtype=np.float32)
        t64 = CO.ctc_token_confidence(labels[b], f64, blank, exclude_blank, how)
        t32 = CO.ctc_token_confidence(labels[b], f32, blank, exclude_blank, how)
        assert len(t64) == n
        fc, tc = frame_conf[b, :T].numpy(), tok_conf[b, :n].numpy()
        assert np.isfinite(fc).all() and np.isfinite(f64).all()
        e32 = max(e32, float(np.abs(f32 - f64).max()), float(np.abs(t32 - t64).max()) if n else 0.0)
        err_f = max(err_f, float(np.abs(fc - f64).max()))
        err_t = max(err_t, float(np.abs(tc - t64).max()) if n else 0.0)
        ranges = CO.ctc_token_ranges(labels[b], blank, exclude_blank)
        if exclude_blank:
            assert ranges == list(zip(tok_start[b, :n].tolist(), tok_end[b, :n].tolist()))
        if how in ("min", "max"):   # exactly the min / max of the device's own frame confidences over the restatement's range
            pick = np.min if how == "min" else np.max
            assert tc.tolist() == [float(pick(fc[lo:hi + 1])) for lo, hi in ranges], b
    tol = max(8 * e32, FLOOR)
    print(f"CONF_ERR ctc {CO.method_row(cfg)} {norm} alpha={alpha} C={C} agg={how} exclude_blank={exclude_blank} "
          f"frame={err_f:.3e} token={err_t:.3e} e32={e32:.3e} tol={tol:.3e}")
    assert err_f <= tol and err_t <= tol, (err_f, err_t, tol)


@pytest.mark.parametrize("exclude_blank", [True, False])
@pytest.mark.parametrize("how", AGGS)
def test_ctc_token_confidence_over_ranges_wider_than_a_wave(how, exclude_blank):
    """a token's range of 64 frames or more is folded by a whole wave, a shorter one inside a lane: runs of 100 and 70 frames, 150
    blank frames in front of a token, next to tokens of a few frames, in one utterance and across the two kinds of range"""
    from nemo_amd import ops
    from nemo_amd.modules.confidence import AGGREGATIONS
    C, T, blank = 37, 230, 36
    plan = [[(blank, 150), (5, 50), (blank, 3), (7, 2), (8, 1), (blank, 24)],       # 150 blanks, then short tokens
            [(3, 100), (blank, 30), (3, 70), (4, 5), (blank, 1), (4, 24)]]         # runs of 100 and 70 frames, a repeat behind a blank
    g = torch.Generator().manual_seed(9)
    z = torch.randn(2, T, C, generator=g, dtype=torch.float64)
    labels = []
    for b, segs in enumerate(plan):
        seq = [k for k, n in segs for _ in range(n)]
        assert len(seq) == T
        z[b, torch.arange(T), torch.tensor(seq)] += 8.0
        labels.append(seq)
    logp = torch.log_softmax(z, -1).to(torch.float32)
    assert [logp[b].argmax(-1).tolist() for b in range(2)] == labels
    widths = [hi - lo + 1 for l in labels for lo, hi in CO.ctc_token_ranges(l, blank, exclude_blank)]
    assert max(widths) >= 100 and min(widths) <= 2 and 64 <= sorted(widths)[-2]
    cfg = _method("entropy", "tsallis", 0.33, "exp")
    lens = torch.tensor([T, T], dtype=torch.int64)
    got = [x.cpu() for x in ops.ctc_greedy_decode_conf(logp.to(dev), lens.to(dev), blank, cfg.kernel_args(C), AGGREGATIONS[how],
                                                       exclude_blank)]
    for a, w in zip(got[:5], ops.ctc_greedy_decode_ts(logp.to(dev), lens.to(dev), blank)):
        assert torch.equal(a, w.cpu())
    out_len, frame_conf, tok_conf = got[1], got[5], got[6]
    err = e32 = 0.0
    for b in range(2):
        n = int(out_len[b])
        f64 = CO.frame_confidence(logp[b].numpy(), cfg)
        f32 = CO.frame_confidence(logp[b].numpy(), cfg, dtype=np.float32)
        t64 = CO.ctc_token_confidence(labels[b], f64, blank, exclude_blank, how)
        t32 = CO.ctc_token_confidence(labels[b], f32, blank, exclude_blank, how)
        assert len(t64) == n and (tok_conf[b, n:] == 0.0).all()
        fc, tc = frame_conf[b].numpy(), tok_conf[b, :n].numpy()
        e32 = max(e32, float(np.abs(f32 - f64).max()), float(np.abs(t32 - t64).max()))
        err = max(err, float(np.abs(fc - f64).max()), float(np.abs(tc - t64).max()))
        if how in ("min", "max"):
            pick = np.min if how == "min" else np.max
            assert tc.tolist() == [float(pick(fc[lo:hi + 1])) for lo, hi in CO.ctc_token_ranges(labels[b], blank, exclude_blank)]
    tol = max(8 * e32, FLOOR)
    print(f"CONF_ERR ctc wide ranges agg={how} exclude_blank={exclude_blank} err={err:.3e} e32={e32:.3e} tol={tol:.3e}")
    assert err <= tol, (err, tol)


# ---------------------------------------------------------------------------------------------------------- transducers
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


def _bf16_images(Pd, Pj, enc):
    """what the bf16 search reads: bf16-rounded weights and projection, widened to float32 (as tests/test_stream_decode_gpu.py)"""
    rb = lambda w: w.to(torch.bfloat16).to(torch.float32)   # noqa: E731
    Pd16, Pj16 = dict(Pd), dict(Pj)
    for k in ("prediction.dec_rnn.lstm.weight_ih_l0", "prediction.dec_rnn.lstm.weight_hh_l0"):
        Pd16[k] = rb(Pd[k])
    outk = [k for k in Pj if k.startswith("joint_net.") and k.endswith(".weight")][0]
    for k in ("pred.weight", "enc.weight", outk):
        Pj16[k] = rb(Pj[k])
    f16 = rb(torch.nn.functional.linear(rb(enc.transpose(1, 2)), Pj16["enc.weight"], Pj["enc.bias"]))
    return Pd16, Pj16, f16


def _cuttings(T):
    g = torch.Generator().manual_seed(77)
    rnd = sorted(set(torch.randint(1, T, (6,), generator=g).tolist()))
    return {"every frame": list(range(T + 1)), "width 5": list(range(0, T, 5)) + [T], "random": [0] + rnd + [T]}


def _run_chunked_conf(ops, f_all, lens, args, blank, ms, edges, durations, method):
    """-> per stream (tokens, times, confidences as float32 bit patterns), the final state"""
    B = f_all.shape[0]
    toks, times, conf = [[] for _ in range(B)], [[] for _ in range(B)], [[] for _ in range(B)]
    state = None
    for lo, hi in zip(edges[:-1], edges[1:]):
        cl = (lens - lo).clamp(min=0, max=hi - lo).to(dev)
        fc = f_all[:, lo:hi].contiguous()
        if durations is None:
            tk, tm, n, state, tc = ops.rnnt_greedy_decode_stream_conf(fc, cl, *args, blank, ms, method, state=state)
        else:
            tk, tm, n, state, tc = ops.tdt_greedy_decode_stream_conf(fc, cl, *args, blank, durations, ms, method, state=state)
        tk, tm, n, tc = tk.cpu(), tm.cpu(), n.cpu(), tc.cpu()
        for b in range(B):
            k = int(n[b])
            toks[b] += tk[b, :k].tolist()
            times[b] += tm[b, :k].tolist()
            conf[b] += tc[b, :k].view(torch.int32).tolist()
            assert (tc[b, k:] == 0.0).all() and (tk[b, k:] == -1).all()
    return list(zip(toks, times, conf)), state


TRANSDUCER_METHODS = {"default": ("entropy", "tsallis", 0.33, "exp"), "gibbs lin": ("entropy", "gibbs", 0.5, "lin"),
                      "max_prob": ("max_prob", "tsallis", 0.33, "exp")}


@pytest.mark.parametrize("which", list(TRANSDUCER_METHODS))
@pytest.mark.parametrize("max_symbols", [2, 10])
@pytest.mark.parametrize("kind", ["rnnt", "tdt"])
@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_transducer_confidence_against_the_float64_replay(wdt, kind, max_symbols, which):
    from nemo_amd import ops
    from nemo_amd.modules import ConfidenceMethodConfig
    V, B, T = S.SMALL["V"], len(S.SMALL["lens"]), S.SMALL["T"]
    lens = torch.tensor(S.SMALL["lens"])
    durations = DUR if kind == "tdt" else None
    cfg = _method(*TRANSDUCER_METHODS[which])
    if which == "default":
        assert cfg == ConfidenceMethodConfig()
    method = cfg.kernel_args(V + 1)
    Pd, Pj = S.small_case(kind)
    enc = S.small_enc()
    if wdt == torch.bfloat16:
        Pd_r, Pj_r, f_r = _bf16_images(Pd, Pj, enc)
        f_dev = f_r.to(dev).to(torch.bfloat16)
    else:
        Pd_r, Pj_r = Pd, Pj
        f_r = torch.nn.functional.linear(enc.transpose(1, 2), Pj["enc.weight"], Pj["enc.bias"])
        f_dev = f_r.to(dev).contiguous()
    args = _dev_args(Pd, Pj, wdt)
    if kind == "rnnt":
        plain = ops.rnnt_greedy_decode(f_dev, lens.to(dev), *args, V, max_symbols, with_state=True)
        withc = ops.rnnt_greedy_decode_conf(f_dev, lens.to(dev), *args, V, max_symbols, method, with_state=True)
    else:
        plain = ops.tdt_greedy_decode(f_dev, lens.to(dev), *args, V, DUR, max_symbols, with_state=True)
        withc = ops.tdt_greedy_decode_conf(f_dev, lens.to(dev), *args, V, DUR, max_symbols, method, with_state=True)
    # everything the plain entry writes, bit for bit
    for a, w, what in zip(withc[:4], plain[:4], ("tokens", "times", "out_len", "score")):
        assert torch.equal(a, w), what
    assert torch.equal(withc[4][0], plain[4][0]) and torch.equal(withc[4][1], plain[4][1])
    tokens, times, out_len, tok_conf = withc[0].cpu(), withc[1].cpu(), withc[2].cpu(), withc[5].cpu()
    assert int(out_len.sum()) > 20
    # against the replay along the device's own tokens and frames
    err = e32 = 0.0
    for b in range(B):
        n = int(out_len[b])
        assert (tok_conf[b, n:] == 0.0).all()
        tk, tm = tokens[b, :n].tolist(), times[b, :n].tolist()
        w64 = CO.replay_transducer_confidence(Pd_r, Pj_r, f_r[b], tk, tm, V, cfg, n_dur=len(DUR) if durations else 0)
        w32 = CO.replay_transducer_confidence(Pd_r, Pj_r, f_r[b], tk, tm, V, cfg, n_dur=len(DUR) if durations else 0,
                                              dtype=torch.float32)
        if n:
            e32 = max(e32, float(np.abs(w32 - w64).max()))
            err = max(err, float(np.abs(tok_conf[b, :n].numpy() - w64).max()))
    tol = max(8 * e32, FLOOR)
    print(f"CONF_ERR {kind} {'bf16' if wdt == torch.bfloat16 else 'fp32'} max_symbols={max_symbols} {which} "
          f"token={err:.3e} e32={e32:.3e} tol={tol:.3e} labels={int(out_len.sum())}")
    # the resumable entry: one launch equals the one-shot entry, and any cutting equals one launch, bit for bit
    one, st1 = _run_chunked_conf(ops, f_dev, lens, args, V, max_symbols, [0, T], durations, method)
    for b in range(B):
        n = int(out_len[b])
        assert one[b] == (tokens[b, :n].tolist(), times[b, :n].tolist(), tok_conf[b, :n].view(torch.int32).tolist()), b
    if durations is None:
        _, _, _, st_plain = ops.rnnt_greedy_decode_stream(f_dev, lens.to(dev), *args, V, max_symbols)
    else:
        _, _, _, st_plain = ops.tdt_greedy_decode_stream(f_dev, lens.to(dev), *args, V, DUR, max_symbols)
    for a in ("h", "c", "last", "score", "frames_done", "skip", "zero_run"):
        assert torch.equal(getattr(st1, a), getattr(st_plain, a)), a
    for name, edges in _cuttings(T).items():
        got, st = _run_chunked_conf(ops, f_dev, lens, args, V, max_symbols, edges, durations, method)
        assert got == one, name
        for a in ("h", "c", "last", "score", "frames_done", "skip", "zero_run"):
            assert torch.equal(getattr(st, a), getattr(st1, a)), (name, a)
    assert err <= tol, (err, tol)


# --------------------------------------------------------------------------------------------------------------- objects
def test_greedy_ctc_decoder_with_a_confidence_config():
    from nemo_amd import ops
    from nemo_amd.modules import GreedyCTCDecoder
    from nemo_amd.modules.confidence import AGGREGATIONS
    C = 37
    logp, lens, ts, _ = _ctc_case(C)
    vocab = [" "] + [chr(ord("a") + i % 26) + str(i) for i in range(C - 2)]
    ccfg = {"preserve_token_confidence": True, "aggregation": "mean", "exclude_blank": False,
            "method_cfg": {"name": "entropy", "entropy_type": "renyi", "alpha": 0.5, "entropy_norm": "lin"}}
    dec = GreedyCTCDecoder(vocab, confidence_cfg=ccfg)
    got = dec.decode_ids_confidence(logp.to(dev), lens.to(dev))
    want = ops.ctc_greedy_decode_conf(logp.to(dev), lens.to(dev), C - 1, dec.confidence_cfg.method_cfg.kernel_args(C),
                                      AGGREGATIONS["mean"], False)
    assert len(got) == 7 and all(torch.equal(a, b) for a, b in zip(got, want))
    # without a config nothing changes: the plain paths, and no confidence path
    plain = GreedyCTCDecoder(vocab)
    assert plain.confidence_cfg is None
    for a, b in zip(dec.decode_ids(logp.to(dev), lens.to(dev), return_timestamps=True), ts):
        assert torch.equal(a.cpu(), b)
    for a, b in zip(plain.decode_ids(logp.to(dev), lens.to(dev)), ts[:3]):
        assert torch.equal(a.cpu(), b)
    with pytest.raises(ValueError, match="confidence_cfg"):
        plain.decode_ids_confidence(logp.to(dev), lens.to(dev))
    n = int(got[1][0])
    words = dec.word_confidence(got[0][0, :n].tolist(), got[6][0, :n].tolist())
    assert len(words) == len(dec.offsets(got[0][0, :n].tolist(), got[3][0, :n].tolist(), got[4][0, :n].tolist())[1])


def _small_modules(kind):
    from nemo_amd.modules import RNNTDecoder, RNNTJoint
    V, H, D, J = (S.SMALL[k] for k in "VHDJ")
    Pd, Pj = S.small_case(kind)
    dec = RNNTDecoder(prednet={"pred_hidden": H, "pred_rnn_layers": 1, "dropout": 0.0}, vocab_size=V, compute_dtype=torch.float32)
    joint = RNNTJoint(jointnet={"encoder_hidden": D, "pred_hidden": H, "joint_hidden": J, "activation": "relu", "dropout": 0.0},
                      num_classes=V, num_extra_outputs=len(DUR) if kind == "tdt" else 0, compute_dtype=torch.float32)
    last = f"joint_net.{len(joint.joint_net) - 1}."   # (without dropout the output layer sits one place further up)
    dec.load_state_dict(Pd); joint.load_state_dict({k.replace("joint_net.2.", last): v for k, v in Pj.items()})
    return dec.to(dev).eval(), joint.to(dev).eval()


@pytest.mark.parametrize("kind", ["rnnt", "tdt"])
def test_greedy_transducer_objects_with_a_confidence_config(kind):
    from nemo_amd.modules import GreedyBatchedRNNTInfer, GreedyBatchedTDTInfer
    V, T, ms = S.SMALL["V"], S.SMALL["T"], 10
    lens = torch.tensor(S.SMALL["lens"])
    dec, joint = _small_modules(kind)
    ccfg = {"preserve_token_confidence": True}
    make = (lambda **kw: GreedyBatchedTDTInfer(dec, joint, V, DUR, max_symbols_per_step=ms, **kw)) if kind == "tdt" else \
        (lambda **kw: GreedyBatchedRNNTInfer(dec, joint, V, max_symbols_per_step=ms, **kw))
    infer, plain = make(confidence_cfg=ccfg), make()
    encd = S.small_enc().to(dev)
    whole = infer(encoder_output=encd, encoded_lengths=lens.to(dev))[0]
    ref = plain(encoder_output=encd, encoded_lengths=lens.to(dev))[0]
    tok_conf = infer.decode_ids(encd, lens.to(dev), with_confidence=True)[-1].cpu()
    assert sum(len(h.y_sequence) for h in whole) > 20
    for b, (h, r) in enumerate(zip(whole, ref)):
        assert h.y_sequence.tolist() == r.y_sequence.tolist() and h.timestamp == r.timestamp and h.score == r.score
        assert r.token_confidence is None and r.word_confidence is None and r.frame_confidence is None
        assert h.token_confidence == tok_conf[b, : len(h.y_sequence)].tolist() and len(h.token_confidence) == len(h.y_sequence)
        assert all(-0.01 < c < 1.01 for c in h.token_confidence)
    # two chunks through partial_hypotheses equal one call (over slices of the same projection values)
    f_whole, args = infer._project(encd)
    project = infer._project
    hyps = infer.fresh_hypotheses(len(lens))
    assert all(h.token_confidence == [] for h in hyps) and all(h.token_confidence is None for h in plain.fresh_hypotheses(2))
    try:
        for lo, hi in ((0, 20), (20, T)):
            infer._project = lambda chunk, lo=lo, hi=hi: (f_whole[:, lo:hi].contiguous(), args)
            cl = (lens - lo).clamp(min=0, max=hi - lo).to(dev)
            hyps = infer(encoder_output=encd[:, :, lo:hi].contiguous(), encoded_lengths=cl, partial_hypotheses=hyps)[0]
    finally:
        infer._project = project
    for h, w in zip(hyps, whole):
        assert h.y_sequence.tolist() == w.y_sequence.tolist() and h.timestamp == w.timestamp
        assert h.token_confidence == w.token_confidence
    # per-step blank confidences are not kept: frame confidence (and alignments) stay refused
    for kw in (dict(preserve_frame_confidence=True), dict(confidence_cfg={"preserve_frame_confidence": True}),
               dict(preserve_alignments=True)):
        with pytest.raises(NotImplementedError):
            make(**kw)


VOCAB = [" "] + list("abcdefghijklmnopqrs")
MODEL_CONF = {"preserve_frame_confidence": True, "preserve_token_confidence": True, "preserve_word_confidence": True,
              "aggregation": "prod", "exclude_blank": True, "method_cfg": {"name": "entropy", "entropy_type": "gibbs", "alpha": 0.5}}


def _waves():
    g = torch.Generator().manual_seed(7)
    return [0.1 * torch.randn(16000, generator=g), 0.1 * torch.randn(9600, generator=g)]


def _check_words(h, how):
    from nemo_amd.modules import aggregate
    toks = [VOCAB[i] for i in h.y_sequence.tolist()]
    groups, cur = [], None
    for i, t in enumerate(toks):   # characters: the space token separates words and belongs to none
        if t == " ":
            cur = None
        elif cur is None:
            cur = [i]
            groups.append(cur)
        else:
            cur.append(i)
    assert len(h.token_confidence) == len(toks)
    assert h.word_confidence == [aggregate([h.token_confidence[i] for i in g], how) for g in groups]
    assert len(h.word_confidence) == len(h.text.split())


def test_ctc_model_transcribe_carries_confidence():
    from nemo_amd.models import EncDecCTCModel, conformer_ctc_config
    torch.manual_seed(3)
    cfg = conformer_ctc_config("small", vocab_size=len(VOCAB), d_model=64, n_heads=4, n_layers=2, dropout=0.0,
                               dropout_pre_encoder=0.0, dropout_att=0.0)
    cfg["preprocessor"]["dither"] = 0.0
    cfg["decoder"]["vocabulary"] = VOCAB
    cfg["labels"] = VOCAB
    cfg["decoding"] = {"strategy": "greedy", "confidence_cfg": MODEL_CONF}
    m = EncDecCTCModel(cfg)
    with torch.no_grad():
        m.decoder.decoder_layers[0].bias[-1] -= 3.0   # random weights with fewer blanks: the hypotheses are not empty
    m = m.to(dev).eval()
    waves = _waves()
    hyps = m.transcribe(waves, batch_size=2, timestamps=True)
    assert any(len(h.y_sequence) for h in hyps) and [h.text for h in hyps] == m.transcribe(waves, batch_size=2)
    for h in hyps:
        assert len(h.frame_confidence) == h.length and all(np.isfinite(h.frame_confidence))
        for c, tc in zip(h.timestamp["char"], h.token_confidence):   # prod over the token's own run of frames
            assert tc == pytest.approx(float(np.prod(np.float32(h.frame_confidence[c["start_offset"]: c["end_offset"]]))), rel=1e-5)
        _check_words(h, "prod")
    # return_hypotheses without timestamps keeps returning its triples
    triples = m.transcribe(waves, batch_size=2, return_hypotheses=True)
    assert all(isinstance(t, tuple) and len(t) == 3 for t in triples)


def test_hybrid_model_transcribe_carries_confidence_on_both_heads():
    from nemo_amd.models import EncDecHybridRNNTCTCModel, fastconformer_hybrid_config
    torch.manual_seed(4)
    cfg = fastconformer_hybrid_config("small", vocab_size=len(VOCAB), ctc_loss_weight=0.3, d_model=64, n_heads=4, n_layers=2,
                                      subsampling_conv_channels=32, dropout=0.0, dropout_pre_encoder=0.0, dropout_att=0.0,
                                      compute_dtype=torch.float32)
    cfg["labels"] = VOCAB
    cfg["preprocessor"]["dither"] = 0.0
    cfg["decoder"]["prednet"].update(pred_hidden=64, dropout=0.0)
    cfg["joint"]["jointnet"].update(joint_hidden=64, dropout=0.0)
    rnnt_conf = {"preserve_token_confidence": True, "preserve_word_confidence": True, "aggregation": "min"}
    cfg["decoding"] = dict(cfg.get("decoding") or {}, confidence_cfg=rnnt_conf)
    cfg["aux_ctc"]["decoding"] = dict(cfg["aux_ctc"].get("decoding") or {}, confidence_cfg=MODEL_CONF)
    m = EncDecHybridRNNTCTCModel(cfg)
    with torch.no_grad():
        m.ctc_decoder.decoder_layers[0].bias[-1] -= 3.0
        for p in list(m.decoder.parameters()) + list(m.joint.parameters()):   # and a transducer head that emits labels and blanks
            p.mul_(4.0)
        m.joint.joint_net[-1].bias[len(VOCAB)] += 2.0
    m = m.to(dev).eval()
    waves = _waves()
    # the transducer head
    hyps = m.transcribe(waves, batch_size=2, return_hypotheses=True)
    assert [h.text for h in hyps] == m.transcribe(waves, batch_size=2) and any(len(h.y_sequence) for h in hyps)
    for h in hyps:
        assert h.frame_confidence is None and len(h.timestamp) == len(h.y_sequence)
        _check_words(h, "min")
    # a new decoding section replaces the confidence settings with it
    m.change_decoding_strategy(decoding_cfg=dict(m._cfg["decoding"], confidence_cfg=dict(rnnt_conf, aggregation="max")),
                               decoder_type="rnnt")
    for h, old in zip(m.transcribe(waves, batch_size=2, return_hypotheses=True), hyps):
        assert h.token_confidence == old.token_confidence
        _check_words(h, "max")
    # the CTC head
    m.change_decoding_strategy(decoder_type="ctc")
    for h in m.transcribe(waves, batch_size=2, timestamps=True):
        assert len(h.frame_confidence) == h.length
        _check_words(h, "prod")
    for h in m.transcribe(waves, batch_size=2, return_hypotheses=True):
        assert len(h.frame_confidence) == h.length
        _check_words(h, "prod")
