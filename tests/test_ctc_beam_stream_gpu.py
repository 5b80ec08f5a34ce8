"""-m gpu: the resumable CTC prefix beam search (`mi355x_ctc_beam_decode_stream`, `mi355x_ctc_beam_decode_lm_stream`) through
`ops.ctc_beam_decode_stream`, the decoding object and the streaming step of the CTC and hybrid models.

The reference of every comparison is the one-shot entry point on the same input (`ops.ctc_beam_decode`, `ops.ctc_beam_decode_lm`),
which tests/test_ctc_beam_gpu.py and tests/test_ctc_beam_lm_gpu.py hold to float64.  A streamed frame does the float32 operations
of the one-shot frame in the same order, so every comparison is BITWISE and no case is left out: scores through an int32 view,
tokens and tok_frame up to hyp_len (the streamed outputs are not padded), hyp_len and n_hyp equal."""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch

import ctc_beam_lm_oracle as L
import ctc_beam_oracle as O

pytestmark = pytest.mark.gpu
dev = "cuda"
INF = float("inf")
SEEDS = (0, 1, 2)

# (T, C, W, threshold, beta); blank = C - 1.  Each the smallest shape at which its path can go wrong.
SHAPES = [
    (37, 5, 4, INF, 0.0),        # C < 64
    (70, 29, 8, INF, 0.0),       # crossing 64 frames
    (200, 33, 3, INF, 0.0),      # odd W, long chase; the initial capacity is 64, so the tree grows twice
    (24, 129, 16, 8.0, 0.5),     # three class groups, pruning, beta
    (12, 1025, 64, 6.0, 0.0),    # full wave, BPE width
    (24, 70, 64, INF, 0.0),      # full wave, no pruning
]
LM_SHAPES = [SHAPES[3], SHAPES[4]]
LM_ORDER, ALPHA = 3, 0.5


def _cuts(T, kind):
    """chunk lengths summing to T"""
    m = min(64, T // 2)   # the frame the parity cuts straddle: 64 where the utterance has it
    bounds = {
        "one": [],
        "ones": list(range(1, T)),
        "c14": list(range(14, T, 14)),
        "straddle": [m - 1, m, m + 1],      # chunks of m-1, 1, 1: the row parity restarts at m-1, m and m+1
        "even_odd": [2, m],                 # an even chunk, then a restart at m
        "odd_even": [1, m + 1],             # an odd chunk, then a restart at m+1
        "random": sorted(set(np.random.default_rng(T).integers(1, T, size=max(2, T // 9)).tolist())),
    }[kind]
    edges = [0] + [b for b in bounds if 0 < b < T] + [T]
    return [b - a for a, b in zip(edges, edges[1:])]


CHUNKINGS = ("one", "ones", "c14", "straddle", "even_odd", "odd_even", "random")


@functools.lru_cache(maxsize=None)
def _logp(T, C):
    """[len(SEEDS), T, C] on the device: the oracle module's generator; shared and never written"""
    return torch.from_numpy(np.stack([O.make_logp(s, T, C) for s in SEEDS])).to(dev)


@functools.lru_cache(maxsize=None)
def _lm(V):
    """the trigram of the oracle module through the product's own path: ARPA text -> NGramLM"""
    from nemo_amd.modules import NGramLM
    with tempfile.TemporaryDirectory() as d:
        L.write_arpa(L.make_lm(0, V, LM_ORDER), os.path.join(d, "lm.arpa"))
        return NGramLM.from_arpa(os.path.join(d, "lm.arpa"), V)


def _host(out):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().copy() for t in out)


def _one_shot_on(lp, lens, shape, lm=False, alpha=ALPHA):
    from nemo_amd import ops
    _, C, W, theta, beta = shape
    ln = None if lens is None else torch.as_tensor(lens, dtype=torch.int64, device=dev)
    if lm:
        return _host(ops.ctc_beam_decode_lm(lp.contiguous(), ln, C - 1, W, theta, beta, _lm(C - 1), alpha))
    return _host(ops.ctc_beam_decode(lp.contiguous(), ln, C - 1, W, theta, beta))


@functools.lru_cache(maxsize=None)
def _one_shot(shape, upto=None, lm=False):
    """the reference: the one-shot search over the first `upto` frames (all of them: None); computed once per case"""
    T, C = shape[:2]
    return _one_shot_on(_logp(T, C)[:, : (T if upto is None else upto)], None, shape, lm)


def _step(lp, lens, shape, state, lm=False, alpha=ALPHA, emit=True):
    from nemo_amd import ops
    _, C, W, theta, beta = shape
    ln = None if lens is None else torch.as_tensor(lens, dtype=torch.int64, device=dev)
    out, nxt = ops.ctc_beam_decode_stream(lp.contiguous(), ln, C - 1, W, theta, beta, state, lm=_lm(C - 1) if lm else None, alpha=alpha,
                                          emit=emit)
    return (_host(out) if emit else None), nxt


def _same(got, want, what=""):
    """bitwise: got may be wider than want (capacity >= T) and is compared up to hyp_len only"""
    gt, gf, gl, gs, gn = got
    wt, wf, wl, ws, wn = want
    assert np.array_equal(gn, wn) and np.array_equal(gl, wl), (what, gn, wn, gl, wl)
    assert np.array_equal(gs.view(np.int32), ws.view(np.int32)), (what, gs, ws)
    Lmax = int(wl.max()) if wl.size else 0
    assert gt.shape[2] >= Lmax and wt.shape[2] >= Lmax
    mask = np.arange(Lmax)[None, None, :] < wl[:, :, None]
    assert np.array_equal(gt[:, :, :Lmax][mask], wt[:, :, :Lmax][mask]), what
    assert np.array_equal(gf[:, :, :Lmax][mask], wf[:, :, :Lmax][mask]), what


def _state_bits(state):
    torch.cuda.synchronize()
    return {n: t.cpu().numpy().copy() for n, t in state.arrays().items()}


def _stream(shape, cuts, lm=False, alpha=ALPHA, emit=lambda i, last: True, each=None, capacity=64):
    """the whole input in chunks; -> (the last emitted result, the final state).  each(i, frames_so_far, result or None)"""
    from nemo_amd.modules import CTCBeamStreamState
    T, C, W = shape[:3]
    lp = _logp(T, C)
    state = CTCBeamStreamState.fresh(len(SEEDS), W, dev, capacity=capacity, lm=lm)
    t0, res = 0, None
    for i, n in enumerate(cuts):
        e = emit(i, i == len(cuts) - 1)
        r, state = _step(lp[:, t0:t0 + n], None, shape, state, lm, alpha, e)
        t0 += n
        res = r if e else res
        if each is not None:
            each(i, t0, r)
    assert t0 == T and state.bound == T
    return res, state


def _cases(shapes, kinds):
    return [pytest.param(s, k, id=f"T{s[0]}-C{s[1]}-W{s[2]}-{k}") for s in shapes for k in kinds if k != "ones" or s[0] <= 37]


# ------------------------------------------------------------------------------------------------ 1. final result, every chunking
@pytest.mark.parametrize("shape,kind", _cases(SHAPES, CHUNKINGS))
def test_any_chunking_gives_the_one_shot_bits(shape, kind):
    cuts = _cuts(shape[0], kind)
    assert sum(cuts) == shape[0] and min(cuts) >= 1
    got, state = _stream(shape, cuts)
    _same(got, _one_shot(shape), (shape, cuts))
    assert _state_bits(state)["frames_done"].tolist() == [shape[0]] * len(SEEDS)
    if shape[0] == 200:
        assert state.capacity == 256   # 64 -> 128 -> 256: the tree was copied twice (once, in one step, for a single chunk)


# ------------------------------------------------------------------------------------------------ 2. ragged streams
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"T{s[0]}-C{s[1]}-W{s[2]}")
def test_ragged_streams_and_ended_streams_pass_through(shape):
    from nemo_amd.modules import CTCBeamStreamState
    T, C, W = shape[:3]
    lens = [T, T - 1, 1, 0]
    lp = torch.from_numpy(np.stack([O.make_logp(10 + b, T, C) for b in range(4)])).to(dev)
    for b, n in enumerate(lens):
        lp[b, n:] = float("nan")   # rows beyond the length are never read
    want = _one_shot_on(lp, lens, shape)
    state, t0, got, ended = CTCBeamStreamState.fresh(4, W, dev), 0, None, None
    for n in _cuts(T, "c14" if T > 14 else "straddle"):
        chunk_lens = [min(max(l - t0, 0), n) for l in lens]
        got, state = _step(lp[:, t0:t0 + n], chunk_lens, shape, state)
        t0 += n
        bits = _state_bits(state)
        if ended is not None:   # streams 2 and 3 ended in the first chunk: later steps leave their state as it is, bit for bit
            for name, v in bits.items():
                assert np.array_equal(v[2:].view(np.uint8), ended[name][2:].view(np.uint8)), name
        ended = bits
    _same(got, want, shape)
    assert ended["frames_done"].tolist() == lens and want[4].tolist()[3] == 1 and want[3][3, 0] == 0.0   # (an empty hypothesis, score 0)


# ------------------------------------------------------------------------------------------------ 3. intermediate results
@pytest.mark.parametrize("shape,kind", _cases(SHAPES, ("c14", "random")))
def test_every_intermediate_result_is_the_one_shot_over_the_frames_so_far(shape, kind):
    cuts = _cuts(shape[0], kind)
    seen = {}

    def check(i, frames, res):
        _same(res, _one_shot(shape, frames), (shape, frames))
        seen[i] = res

    _stream(shape, cuts, each=check)
    assert len(seen) == len(cuts)

    def check_sparse(i, frames, res):   # steps that only advance the state in between change nothing
        assert (res is None) == (i % 2 == 0 and i != len(cuts) - 1)
        if res is not None:
            _same(res, seen[i], (shape, frames))

    _stream(shape, cuts, emit=lambda i, last: last or i % 2 == 1, each=check_sparse)


# ------------------------------------------------------------------------------------------------ 4. out of place
@pytest.mark.parametrize("lm", [False, True], ids=["plain", "lm"])
def test_a_step_is_out_of_place_and_repeatable(lm):
    from nemo_amd.modules import CTCBeamStreamState
    shape = SHAPES[3]
    T, C, W = shape[:3]
    lp = _logp(T, C)
    _, s0 = _step(lp[:, :9], None, shape, CTCBeamStreamState.fresh(len(SEEDS), W, dev, lm=lm), lm)
    before = _state_bits(s0)
    r1, s1 = _step(lp[:, 9:20], None, shape, s0, lm)
    b1 = _state_bits(s1)
    r2, s2 = _step(lp[:, 9:20], None, shape, s0, lm)
    _same(r2, r1)
    after, b2 = _state_bits(s0), _state_bits(s2)
    assert s1.beams.data_ptr() != s0.beams.data_ptr() != s2.beams.data_ptr() and s1.tree is s0.tree
    for name in before:
        assert np.array_equal(before[name].view(np.uint8), after[name].view(np.uint8)), name
        assert np.array_equal(b1[name].view(np.uint8), b2[name].view(np.uint8)), name
    assert b1["frames_done"].tolist() == [20] * len(SEEDS) and before["frames_done"].tolist() == [9] * len(SEEDS)
    r3, _ = _step(lp[:, 20:], None, shape, s2, lm)   # and the stream goes on to the one-shot result
    _same(r3, _one_shot(shape, None, lm))


# ------------------------------------------------------------------------------------------------ 5. LM
@pytest.mark.parametrize("shape,kind", _cases(LM_SHAPES, ("ones", "c14", "random")))
def test_lm_fused_stream_gives_the_one_shot_bits(shape, kind):
    cuts = _cuts(shape[0], kind)
    got, state = _stream(shape, cuts, lm=True)
    want = _one_shot(shape, None, True)
    _same(got, want, (shape, cuts))
    plain = _one_shot(shape)
    assert not (np.array_equal(want[3].view(np.int32), plain[3].view(np.int32)))   # (the LM takes part)
    zero, _ = _stream(shape, cuts, lm=True, alpha=0.0)   # alpha = 0: the bits of the LM-less stream
    bare, _ = _stream(shape, cuts)
    _same(zero, bare, (shape, cuts))
    _same(zero, plain, (shape, cuts))


# ------------------------------------------------------------------------------------------------ 6. capacity clamp
GUARD, SENT = 8, 0x5A5A5A5A


def _guarded(n):
    """n int32 elements followed by eight guard words, all filled with a sentinel"""
    return torch.full((n + GUARD,), SENT, dtype=torch.int32, device=dev)


def test_the_kernel_stops_at_the_capacity_of_the_tree():
    """reads the clamp: frames_done = Tcap - 3 and a chunk of 8 consume 3 frames.  Every buffer the kernel could overrun in such a
    step is allocated with guard words behind it, so nothing here can touch memory that is not the test's."""
    import ctypes
    from nemo_amd import _lib
    from nemo_amd.modules import CTCBeamStreamState as S
    from nemo_amd.ops import _CTCBeamStateC
    B, Tcap, C, W = len(SEEDS), 16, 29, 8
    shape = (Tcap + 5, C, W, INF, 0.0)
    lp = _logp(shape[0], C)
    tree, tokens, frames = _guarded(B * Tcap * W * 2), _guarded(B * W * Tcap), _guarded(B * W * Tcap)
    n_tree, n_out = B * Tcap * W * 2, B * W * Tcap
    st = [S(torch.empty(2, B, W, dtype=torch.int64, device=dev), torch.empty(10, B, W, dtype=torch.int32, device=dev),
            torch.empty(2, B, dtype=torch.int32, device=dev), tree[:n_tree].view(B, Tcap, W, 2), tokens[:n_out].view(B, W, Tcap),
            frames[:n_out].view(B, W, Tcap), False, 0) for _ in range(2)]
    hyp_len, n_hyp = torch.empty(B, W, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    score = torch.empty(B, W, dtype=torch.float32, device=dev)

    def call(chunk, s_in, s_out, outs=True):
        chunk = chunk.contiguous()
        lens = torch.full((B,), chunk.shape[1], dtype=torch.int64, device=dev)
        o = [t.data_ptr() for t in (tokens, frames, hyp_len, score, n_hyp)] if outs else [None] * 5
        cin, cout = (_CTCBeamStateC.of(s) if s is not None else None for s in (s_in, s_out))
        rc = _lib.lib.mi355x_ctc_beam_decode_stream(chunk.data_ptr(), lens.data_ptr(), tree.data_ptr(), *o, B, chunk.shape[1], C, C - 1, W,
                                                    INF, 0.0, Tcap, ctypes.byref(cin) if cin is not None else None, ctypes.byref(cout),
                                                    None)
        torch.cuda.synchronize()
        return rc

    assert call(lp[:, : Tcap - 3], None, st[0], outs=False) == 0   # a null state_in: fresh streams; no outputs: the state only
    assert _state_bits(st[0])["frames_done"].tolist() == [Tcap - 3] * B
    assert (tokens == SENT).all() and (frames == SENT).all()
    assert call(lp[:, Tcap - 3: Tcap + 5], st[0], st[1]) == 0        # 8 frames offered, 3 fit
    assert _state_bits(st[1])["frames_done"].tolist() == [Tcap] * B
    got = _host((tokens[:n_out].view(B, W, Tcap), frames[:n_out].view(B, W, Tcap), hyp_len, score, n_hyp))
    _same(got, _one_shot(shape, Tcap))
    for buf, n in ((tree, n_tree), (tokens, n_out), (frames, n_out)):
        assert buf[n:].tolist() == [SENT] * GUARD
    # nothing at or beyond hyp_len is written: the buffers still hold the sentinel there
    mask = np.arange(Tcap)[None, None, :] >= got[2][:, :, None]
    assert (got[0][mask] == SENT).all() and (got[1][mask] == SENT).all()
    assert call(lp[:, :4], st[1], st[0]) == 0                        # a full tree: the state passes through
    full, prev = _state_bits(st[0]), _state_bits(st[1])
    assert all(np.array_equal(full[k].view(np.uint8), prev[k].view(np.uint8)) for k in full)
    assert tree[n_tree:].tolist() == [SENT] * GUARD


# ------------------------------------------------------------------------------------------------ 7. bad arguments
def test_bad_arguments_raise():
    import ctypes
    from nemo_amd import _lib, ops
    from nemo_amd.modules import CTCBeamStreamState as S
    from nemo_amd.ops import _CTCBeamStateC
    shape = SHAPES[0]
    T, C, W = shape[:3]
    lp, B = _logp(T, C)[:, :5].contiguous(), len(SEEDS)
    for state, lm in ((S.fresh(B + 1, W, dev), False), (S.fresh(B, W + 1, dev), False), (S.fresh(B, W, dev, lm=True), False),
                      (S.fresh(B, W, dev), True)):
        with pytest.raises(ValueError):
            ops.ctc_beam_decode_stream(lp, None, C - 1, W, INF, 0.0, state, lm=_lm(C - 1) if lm else None, alpha=ALPHA)
    with pytest.raises(ValueError):   # more nodes than 32-bit ids name: refused before anything is allocated
        S.fresh(B, W, dev, capacity=0x3fffffff // W + 1)
    s_in, s_out = S.fresh(B, W, dev, capacity=8), S.fresh(B, W, dev, capacity=8)
    lens = torch.full((B,), 5, dtype=torch.int64, device=dev)
    hyp_len = torch.empty(B, W, dtype=torch.int32, device=dev)

    def call(Tcap=8, outs=(1, 1, 1, 1, 1)):
        o = [t.data_ptr() if k else None for t, k in zip((s_in.tokens, s_in.tok_frame, hyp_len, hyp_len, hyp_len), outs)]
        cin, cout = _CTCBeamStateC.of(s_in), _CTCBeamStateC.of(s_out)
        return _lib.lib.mi355x_ctc_beam_decode_stream(lp.data_ptr(), lens.data_ptr(), s_in.tree.data_ptr(), *o, B, 5, C, C - 1, W, INF, 0.0,
                                                      Tcap, ctypes.byref(cin), ctypes.byref(cout), None)

    assert call(Tcap=0x3fffffff // W + 1) == 1
    assert call(outs=(1, 1, 0, 1, 1)) == 1 and call(outs=(0, 1, 1, 1, 1)) == 1 and call(outs=(1, 0, 0, 0, 0)) == 1
    with pytest.raises(ValueError):
        _lib.check(call(Tcap=0), "ctc_beam_decode_stream")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 8. models
VOCAB = [chr(ord("a") + i) for i in range(20)]
LABELS = [chr(ord("a") + i) for i in range(26)] + [" ", "'"]
GREEDY = dict(strategy="greedy_batch")


def _beam4(arpa=None, best=True):
    beam = dict(beam_size=4, return_best_hypothesis=best)
    if arpa is not None:
        beam.update(ngram_lm_arpa=arpa, ngram_lm_alpha=0.5)
    return dict(strategy="beam_batch", beam=beam)


def _randomise(enc, seed):
    """non-trivial BatchNorm statistics, LayerNorm affine and positional biases (the defaults are 0 / 1)"""
    g = torch.Generator().manual_seed(seed)
    sd = enc.state_dict()
    for k, v in sd.items():
        if k.endswith("running_mean"):
            v.copy_(0.2 * torch.randn(v.shape, generator=g))
        elif k.endswith("running_var"):
            v.copy_(0.5 + torch.rand(v.shape, generator=g))
        elif k.endswith(("pos_bias_u", "pos_bias_v")) or ("norm" in k and k.endswith(("weight", "bias"))):
            v.add_(0.1 * torch.randn(v.shape, generator=g))
    enc.load_state_dict(sd)
    return enc


STREAM_ENC = dict(subsampling="striding", subsampling_factor=4, causal_downsampling=True, att_context_size=[16, 3],
                  att_context_style="chunked_limited", conv_kernel_size=9, conv_context_size="causal")


def _ctc_model(decoding):
    from nemo_amd.models import EncDecCTCModel, conformer_ctc_config
    cfg = conformer_ctc_config("small", vocab_size=len(VOCAB), d_model=64, n_heads=4, n_layers=2, dropout=0.0, dropout_pre_encoder=0.0,
                               dropout_att=0.0, compute_dtype=torch.float32, **STREAM_ENC)
    cfg["decoder"]["vocabulary"] = VOCAB
    cfg["preprocessor"]["dither"] = 0.0
    cfg["decoding"] = decoding
    torch.manual_seed(11)
    m = EncDecCTCModel(cfg)
    _randomise(m.encoder, 12)
    with torch.no_grad():
        m.decoder.decoder_layers[0].bias[-1] -= 3.0   # random weights with fewer blanks: the hypotheses are not empty
    return m.to(dev).eval(), VOCAB


def _hybrid_model(decoding):
    from nemo_amd.models import EncDecHybridRNNTCTCModel, fastconformer_hybrid_config
    cfg = fastconformer_hybrid_config("small", vocab_size=len(LABELS), ctc_loss_weight=0.3, durations=None, d_model=64, n_heads=4,
                                      n_layers=2, subsampling_conv_channels=32, dropout=0.0, dropout_pre_encoder=0.0, dropout_att=0.0,
                                      compute_dtype=torch.float32, **STREAM_ENC)
    cfg["labels"] = LABELS
    cfg["preprocessor"]["dither"] = 0.0
    cfg["decoder"]["prednet"].update(pred_hidden=64, dropout=0.0)
    cfg["joint"]["jointnet"].update(joint_hidden=64, dropout=0.0)
    torch.manual_seed(11)
    m = EncDecHybridRNNTCTCModel(cfg)
    _randomise(m.encoder, 12)
    with torch.no_grad():
        m.ctc_decoder.decoder_layers[0].bias[-1] -= 3.0
    m = m.to(dev).eval()
    m.change_decoding_strategy(decoding, decoder_type="ctc")
    return m, LABELS


def _stream_model(m, drop_at=None):
    """every chunk of three streams through conformer_stream_step, best_hyp passed back as previous_hypotheses; with drop_at the
    middle stream leaves after that many chunks (`gather` regroups the other two).  -> (per stream: hypothesis, text, greedy
    predictions, log-probabilities of its frames), the last best_hyp list"""
    from nemo_amd.streaming import CacheAwareStreamingAudioBuffer
    g = torch.Generator().manual_seed(13)
    audio = (0.1 * torch.randn(3, 24000, generator=g)).to(dev)
    alen = torch.tensor([24000, 17000, 24000]).to(dev)
    with torch.no_grad():
        mel, mel_len = m.preprocessor(input_signal=audio, length=alen)
    ch, tm, ln = m.encoder.get_initial_cache_state(batch_size=3)
    rows, prev, hyps, lps, final = [0, 1, 2], None, None, {0: [], 1: [], 2: []}, {}
    buf = CacheAwareStreamingAudioBuffer(m, mel, mel_len)
    for i, (chunk, cl) in enumerate(buf):
        if drop_at is not None and i == drop_at:
            keep = [0, 2]
            chunk_sel = torch.tensor(keep, device=dev)
            ch, tm, ln = ch[:, chunk_sel].contiguous(), tm[:, chunk_sel].contiguous(), ln[chunk_sel].contiguous()
            prev, hyps, rows = [prev[k] for k in keep], [hyps[k] for k in keep], keep
        if len(rows) < 3:
            sel = torch.tensor(rows, device=dev)
            chunk, cl = chunk[sel].contiguous(), cl[sel].contiguous()
        res = m.conformer_stream_step(processed_signal=chunk, processed_signal_length=cl, cache_last_channel=ch, cache_last_time=tm,
                                      cache_last_channel_len=ln, previous_pred_out=prev, previous_hypotheses=hyps,
                                      drop_extra_pre_encoded=buf.drop_extra_pre_encoded, return_transcription=True, return_log_probs=True)
        prev, texts, ch, tm, ln, hyps, slp, slen = res
        n_prev = {r: sum(x.shape[0] for x in lps[r]) for r in rows}
        for k, r in enumerate(rows):
            lps[r].append(slp[k, : int(slen[k]) - n_prev[r]])
            final[r] = (hyps[k] if hyps is not None else None, texts[k], prev[k])
    torch.cuda.synchronize()
    return {r: final[r] + (torch.cat(lps[r]),) for r in final}, hyps


def _check_rows(dec, out, best=True):
    """every stream's last hypothesis = the one-shot search over the log-probabilities that stream was given, bitwise"""
    n_tokens = 0
    for r, (hyp, text, _, lp) in out.items():
        tokens, tok_frame, hyp_len, score, n_hyp = _host(dec.decode_ids(lp[None]))
        n = int(hyp_len[0, 0])
        assert hyp.y_sequence.tolist() == tokens[0, 0, :n].tolist() and hyp.timestamp == tok_frame[0, 0, :n].tolist()
        assert np.float32(hyp.score).view(np.int32) == score[0, 0].view(np.int32) and hyp.length == n
        assert text == hyp.text == dec.ids_to_text(tokens[0, 0, :n].tolist())
        if not best:
            assert [(i, np.float32(s).view(np.int32)) for _, i, s in hyp.n_best] == \
                [(tokens[0, k, : int(hyp_len[0, k])].tolist(), score[0, k].view(np.int32)) for k in range(int(n_hyp[0]))]
            assert [t for t, _, _ in hyp.n_best] == [dec.ids_to_text(i) for _, i, _ in hyp.n_best]
        else:
            assert hyp.n_best is None
        n_tokens += n
    assert n_tokens > 0


def _check_streamed_model(build, arpa, best=True):
    m, vocab = build(_beam4(arpa, best))
    dec = m.ctc_wer.decoding if hasattr(m, "ctc_wer") else m.wer.decoding
    assert type(dec).__name__ == "BeamBatchedCTCDecoder" and dec.beam_size == 4 and (dec.ngram_lm is not None) == (arpa is not None)
    out, last = _stream_model(m)
    assert last[0].dec_state[0] is last[2].dec_state[0] and [h.dec_state[1] for h in last] == [0, 1, 2]
    _check_rows(dec, out, best)
    return m, dec, out


@pytest.mark.parametrize("build", [_ctc_model, _hybrid_model], ids=["ctc", "hybrid"])
def test_models_stream_the_beam_search(build, tmp_path):
    arpa = str(tmp_path / "lm.arpa")
    n_labels = len(VOCAB) if build is _ctc_model else len(LABELS)
    L.write_arpa(L.make_lm(0, n_labels, LM_ORDER), arpa)
    m, dec, out = _check_streamed_model(build, None, best=False)
    _, _, out_lm = _check_streamed_model(build, arpa)
    assert any(out[r][0].y_sequence.tolist() != out_lm[r][0].y_sequence.tolist() or out[r][0].score != out_lm[r][0].score for r in out)
    # greedy: best_hyp stays None, and element 0 of the beam run is what greedy returns
    g, _ = build(GREEDY)
    greedy, last = _stream_model(g)
    assert last is None
    for r in out:
        assert greedy[r][0] is None and torch.equal(greedy[r][2], out[r][2]) and torch.equal(greedy[r][2], out_lm[r][2])
    # regrouping: the middle stream leaves after two chunks (`gather`); the other two still end at the one-shot result over
    # what they were given
    part, last = _stream_model(m, drop_at=2)
    assert len(last) == 2 and last[0].dec_state[0].B == 2 and sorted(part) == [0, 1, 2]
    _check_rows(dec, {r: part[r] for r in (0, 2)}, best=False)
    assert part[1][3].shape[0] < out[1][3].shape[0]
