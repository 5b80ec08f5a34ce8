"""-m gpu: phrase boosting in the CTC prefix beam search -- `mi355x_ctc_beam_decode_fused` / `_fused_stream` with a `BoostingTree`,
alone and beside an n-gram model -- against the float64 oracle tests/ctc_beam_boost_oracle.py (boost by string matching from the
phrase set, no automaton), and `beam.boosting_tree` through the decoding object, the CTC model, the hybrid model's CTC head and the
streaming step.

Parity rule, the one of test_ctc_beam_lm_gpu.py: a (shape, seed) case is compared only if the float64 oracle's cut margin -- min over
the frames of rank[W-1] - rank[W], search ranks -- is >= 1e-3 (a condition on the input, not a measurement of the device).  Seeds
0..23 of `O.make_logp` are taken per shape, with the phrase set `B.make_phrases(T, C)` (46 .. 75 phrases cut from the arg-max paths
of those inputs, with siblings, nested prefixes and overlaps) and, where the shape has one, the model `make_lm(0, C-1, order)`; at
least 5 must pass the rule, else the test FAILS.  Kept by the oracle on a CPU: 24, 16, 17, 17, 14, 10, 8 seeds for the seven shapes
(the BPE-width shape included, with the boost alpha and seed window as listed: nothing had to be changed for it).  On every kept
case there: the float32 restatement keeps the float64 set and differs from it by <= 1.4e-4, the n-best differs from the boost-less
search's, and a hypothesis holds a completed phrase; in every shape kept cases end with a pending boost and have the n-best
re-ordered by the final term (3 .. 16 of them).  All of that is asserted on the references below before they are used.

In a kept case: the device's set of hypotheses equals the oracle's, n_hyp and hyp_len are equal, device scores are non-increasing,
each score is within max(8 * e32, 16 ulp of the score) of float64 where e32 is the float32 restatement's own largest error on that
case (reference against reference, never the device), every tok_frame is strictly increasing along its hypothesis and lies in
[0, len), and the -1 / -inf padding is exact.  The streaming comparisons are bitwise against the one-shot fused entry."""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch

import ctc_beam_boost_oracle as B
import ctc_beam_lm_oracle as L
import ctc_beam_oracle as O

pytestmark = pytest.mark.gpu
dev = "cuda"
INF = float("inf")
MARGIN = 1e-3

# (T, C, W, threshold, beta, boost alpha, context_score, depth_scaling, LM order or 0, LM alpha); blank = C - 1
SHAPES = [
    (37, 5, 4, INF, 0.0, 1.0, 1.0, 2.0, 0, 0.0),       # C < 64; five classes: phrases overlap and nest all the time
    (70, 29, 8, INF, 0.0, 0.5, 1.0, 2.0, 0, 0.0),      # crossing 64 frames
    (200, 33, 3, INF, 0.0, 1.0, 1.0, 1.0, 0, 0.0),     # W not a power of two, long chase, no depth scaling
    (24, 129, 16, 8.0, 0.5, 1.0, 1.0, 2.0, 3, 0.5),    # two models: trigram + tree; three class groups, pruning, beta
    (66, 129, 8, 8.0, 0.5, 0.5, 2.0, 1.0, 2, 0.3),     # two models: bigram + tree, other scores
    (24, 70, 64, INF, 0.0, 1.0, 1.0, 2.0, 3, 0.5),     # two models, full wave: the re-ordering moves up to 64 hypotheses
    (12, 1025, 64, 6.0, 0.0, 1.0, 1.0, 2.0, 0, 0.0),   # full wave, BPE width
]
IDS = [f"T{s[0]}-C{s[1]}-W{s[2]}" for s in SHAPES]


@functools.lru_cache(maxsize=None)
def _phrases(T, C):
    return tuple(B.make_phrases(T, C))


@functools.lru_cache(maxsize=None)
def _tree(T, C, cs, ds):
    from nemo_amd.modules import BoostingTree
    return BoostingTree.from_phrases(_phrases(T, C), C - 1, context_score=cs, depth_scaling=ds)


@functools.lru_cache(maxsize=None)
def _model(V, order):
    return L.make_lm(0, V, order)


@functools.lru_cache(maxsize=None)
def _device_lm(V, order):
    from nemo_amd.modules import NGramLM
    with tempfile.TemporaryDirectory() as d:
        L.write_arpa(_model(V, order), os.path.join(d, "lm.arpa"))
        return NGramLM.from_arpa(os.path.join(d, "lm.arpa"), V)


def _models(shape, boost_alpha=None, lm_alpha=None):
    T, C, _, _, _, ba, cs, ds, order, la = shape
    lm = [(_device_lm(C - 1, order), la if lm_alpha is None else lm_alpha)] if order else []
    return lm + [(_tree(T, C, cs, ds), ba if boost_alpha is None else boost_alpha)]


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


@functools.lru_cache(maxsize=None)
def _reference(seed, shape, T=None):
    """(logp, float64 result, float32 result or None) of one utterance (of T frames of the shape's phrase set where T is given); the
    float32 run only where the case is kept"""
    T0, C, W, theta, beta, ba, cs, ds, order, la = shape
    lp = O.make_logp(seed, T0 if T is None else T, C)
    ng = _model(C - 1, order) if order else None
    args = (lp, C - 1, W, theta, beta, _phrases(T0, C), ba, cs, ds, ng, max(order, 1), la)
    r64 = B.beam_search_boost(*args)
    r32 = B.beam_search_boost(*args, dtype=np.float32) if r64["margin"] >= MARGIN else None
    return lp, r64, r32


def _plain_nbest(lp, shape):
    _, C, W, theta, beta, _, _, _, order, la = shape
    if order:
        return L.beam_search_lm(lp, C - 1, W, theta, beta, la, _model(C - 1, order), order)["nbest"]
    return O.beam_search(lp, C - 1, W, theta, beta)["nbest"]


def _e32(r64, r32):
    d64 = dict(r64["nbest"])
    common = [abs(float(s) - float(d64[p])) for p, s in r32["nbest"] if p in d64]
    return max(common) if common else 0.0


def _host(out):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().copy() for t in out)


def _decode(logp, lens, shape, models=None):
    from nemo_amd import ops
    _, C, W, theta, beta = shape[:5]
    lp = torch.from_numpy(np.ascontiguousarray(logp)).to(dev) if isinstance(logp, np.ndarray) else logp.contiguous()
    ln = None if lens is None else torch.as_tensor(lens, dtype=torch.int64, device=dev)
    out = _host(ops.ctc_beam_decode_fused(lp, ln, C - 1, W, theta, beta, _models(shape) if models is None else models))
    tokens, tok_frame, hyp_len, score, n_hyp = out
    assert tokens.dtype == tok_frame.dtype == hyp_len.dtype == n_hyp.dtype == np.int32 and score.dtype == np.float32
    assert tokens.shape == tok_frame.shape == (lp.shape[0], W, lp.shape[1]) and score.shape == hyp_len.shape == (lp.shape[0], W)
    return out


def _check_row(tag, T, W, tokens, tok_frame, hyp_len, score, n_hyp, expect, e32):
    """one utterance of the device's output against `expect` = {token tuple: float64 score}; -> its largest score error and bound"""
    n = int(n_hyp)
    assert n == len(expect), (tag, n, len(expect))
    got = [tuple(tokens[k, : hyp_len[k]].tolist()) for k in range(n)]
    assert len(set(got)) == n and set(got) == set(expect), (tag, set(got) ^ set(expect))
    assert all(score[k] >= score[k + 1] for k in range(n - 1)), (tag, score[:n])
    worst, bound = 0.0, 0.0
    for k, p in enumerate(got):
        assert hyp_len[k] == len(p)
        err, tol = abs(float(score[k]) - float(expect[p])), max(8 * e32, 16 * _ulp(expect[p]))
        if err / tol >= worst / max(bound, 1e-300) or bound == 0.0:
            worst, bound = err, tol
        assert err <= tol, (tag, p, float(score[k]), float(expect[p]), err, tol)
        fr = tok_frame[k, : len(p)]
        assert (np.diff(fr) > 0).all() and (len(p) == 0 or (fr[0] >= 0 and fr[-1] < T)), (tag, p, fr)
        assert (tokens[k, len(p):] == -1).all() and (tok_frame[k, len(p):] == -1).all(), (tag, k)
    assert (tokens[n:] == -1).all() and (tok_frame[n:] == -1).all() and (hyp_len[n:] == 0).all() and np.isneginf(score[n:]).all(), tag
    return worst, bound


# ------------------------------------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_boosted_beam_search_matches_the_oracle(shape):
    T, C, W = shape[:3]
    kept = [s for s in range(24) if _reference(s, shape)[2] is not None]
    print(f"CTC_BEAM_BOOST kept {shape}: {len(kept)} of 24 seeds {kept}, {len(_phrases(T, C))} phrases")
    assert len(kept) >= 5, kept
    refs = [_reference(s, shape) for s in kept]
    for lp, r64, r32 in refs:   # conditions on the references, per kept case
        assert set(p for p, _ in r32["nbest"]) == set(p for p, _ in r64["nbest"])
        assert [p for p, _ in _plain_nbest(lp, shape)] != [p for p, _ in r64["nbest"]]          # the boost matters
        assert any(v > 0 for v in r64["complete"].values())                                     # a completed phrase is held
        print(f"CTC_BEAM_BOOST e32 {_e32(r64, r32):.3e}")
    assert any(any(v > 0 for v in r64["pending"].values()) for _, r64, _ in refs)               # per shape: a pending boost at the end
    assert any([p for p, _ in r64["nbest"]] != [p for p, _ in r64["search"]] for _, r64, _ in refs)   # and a re-ordered n-best
    logp = np.stack([lp for lp, _, _ in refs])
    out = _decode(logp, [T] * len(kept), shape)
    worst = (0.0, 0.0)
    for b, (seed, (_, r64, r32)) in enumerate(zip(kept, refs)):
        w = _check_row(shape + (seed,), T, W, *(o[b] for o in out), dict(r64["nbest"]), _e32(r64, r32))
        if w[0] / max(w[1], 1e-300) >= worst[0] / max(worst[1], 1e-300):
            worst = w
    print(f"CTC_BEAM_BOOST err {shape}: largest score error {worst[0]:.3e} against its bound {worst[1]:.3e}")


# ------------------------------------------------------------------------------------------------ 2. alpha = 0, and the LM path
def _ragged_inputs(shape):
    T, C = shape[:2]
    return np.stack([O.make_logp(s, T, C) for s in range(6)]), [T, T - 1, T, 3, T, T // 2]


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3], SHAPES[5]], ids=[IDS[1], IDS[3], IDS[5]])
def test_boost_alpha_zero_gives_the_bits_of_the_tree_less_entry(shape):
    from nemo_amd import ops
    _, C, W, theta, beta, _, _, _, order, la = shape
    logp, lens = _ragged_inputs(shape)
    lp, ln = torch.from_numpy(logp).to(dev), torch.tensor(lens, dtype=torch.int64, device=dev)
    if order:
        plain = _host(ops.ctc_beam_decode_lm(lp, ln, C - 1, W, theta, beta, _device_lm(C - 1, order), la))
    else:
        plain = _host(ops.ctc_beam_decode(lp, ln, C - 1, W, theta, beta))
    fused = _decode(logp, lens, shape, _models(shape, boost_alpha=0.0))
    for name, a, b in zip(("tokens", "tok_frame", "hyp_len", "score", "n_hyp"), plain, fused):
        assert a.tobytes() == b.tobytes(), name
    assert _decode(logp, lens, shape)[3].tobytes() != plain[3].tobytes()   # (and alpha > 0 is another search)
    if order:   # the n-gram model alone through the fused entry: the one-model instantiation gives the LM entry's bits
        alone = _decode(logp, lens, shape, _models(shape)[:1])
        for name, a, b in zip(("tokens", "tok_frame", "hyp_len", "score", "n_hyp"), plain, alone):
            assert a.tobytes() == b.tobytes(), name


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[6]], ids=[IDS[0], IDS[6]])
def test_a_tree_through_the_lm_entry_is_the_fused_search_without_the_final_term(shape):
    """the tree's six tables as a plain NGramLM (no state_final) through `mi355x_ctc_beam_decode_lm` and through the fused entry:
    the same bits, in search order -- and the fused entry with the tree itself differs from that by the final term alone"""
    from nemo_amd import ops
    from nemo_amd.modules import NGramLM
    T, C, W, theta, beta, ba, cs, ds = shape[:8]
    t = _tree(T, C, cs, ds)
    bare = NGramLM(t.vocab_size, t.order, t.state_arc_begin, t.arc_tok, t.arc_logp, t.arc_next, t.state_bo, t.state_bo_next, t.state_len)
    logp, lens = _ragged_inputs(shape)
    lp, ln = torch.from_numpy(logp).to(dev), torch.tensor(lens, dtype=torch.int64, device=dev)
    legacy = _host(ops.ctc_beam_decode_lm(lp, ln, C - 1, W, theta, beta, bare, ba))
    via_tree = _host(ops.ctc_beam_decode_lm(lp, ln, C - 1, W, theta, beta, t, ba))   # (the tree itself: its seventh table is not passed)
    fused = _decode(logp, lens, shape, [(bare, ba)])
    for name, a, b, c in zip(("tokens", "tok_frame", "hyp_len", "score", "n_hyp"), legacy, fused, via_tree):
        assert a.tobytes() == b.tobytes() == c.tobytes(), name
    final = _decode(logp, lens, shape, [(t, ba)])
    assert np.array_equal(final[4], legacy[4])
    for b in range(logp.shape[0]):   # the same hypotheses; each score = its search rank minus alpha * pending, to the last bit
        n = int(legacy[4][b])
        rank = {tuple(legacy[0][b, k, : legacy[2][b, k]].tolist()): legacy[3][b, k] for k in range(n)}
        got = [tuple(final[0][b, k, : final[2][b, k]].tolist()) for k in range(n)]
        assert set(got) == set(rank) and len(set(got)) == n
        for k, p in enumerate(got):
            pending = np.float32(B.boost_parts(_phrases(T, C), p, cs, ds)[1])
            assert final[3][b, k] == np.float32(rank[p] + np.float32(np.float32(ba) * -pending)), (b, p)
        assert all(final[3][b, k] >= final[3][b, k + 1] for k in range(n - 1))


# ------------------------------------------------------------------------------------------------ 3. hand-written and ragged
def test_the_phrase_flips_a_hand_written_case():
    """T = 3, C = 4 (a, b, c, blank).  Frame 0 says a; frame 1 prefers b over c by 0.2; frame 2 says blank.  The phrase `a c` with
    alpha 1 makes `a c` the best hypothesis, and the hypothesis `a` -- a begun `a c` -- is returned without its pending boost."""
    from nemo_amd.modules import BoostingTree
    p1b = 0.45
    p = np.array([[0.90, 0.03, 0.03, 0.04], [0.08, p1b, p1b * np.exp(-0.2), 1.0 - 0.08 - p1b - p1b * np.exp(-0.2)],
                  [0.02, 0.02, 0.02, 0.94]])
    lp = np.log(p).astype(np.float32)
    phrases = [(0, 2)]
    tree = BoostingTree.from_phrases(phrases, 3)
    shape = (3, 4, 64, INF, 0.0)   # every prefix fits (<= 40): no cut, no tie at a cut
    plain = O.beam_search(lp, 3, 64)
    assert plain["nbest"][0][0] == (0, 1) and abs((dict(plain["nbest"])[(0, 1)] - dict(plain["nbest"])[(0, 2)]) - 0.2) < 5e-3
    for alpha, best in ((0.0, (0, 1)), (1.0, (0, 2))):
        r64 = B.beam_search_boost(lp, 3, 64, INF, 0.0, phrases, alpha)
        r32 = B.beam_search_boost(lp, 3, 64, INF, 0.0, phrases, alpha, dtype=np.float32)
        assert r64["nbest"][0][0] == best and r64["nbest"][0][1] - r64["nbest"][1][1] > 0.1
        out = _decode(lp[None], [3], shape, [(tree, alpha)])
        assert tuple(out[0][0, 0, : out[2][0, 0]].tolist()) == best
        _check_row(("flip", alpha), 3, 64, *(o[0] for o in out), dict(r64["nbest"]), _e32(r64, r32))
    # the dangling `a`: pending 1 in the search, nothing of it in what is returned
    assert r64["pending"][(0,)] == 1.0 and r64["complete"][(0,)] == 0.0 and (0,) in dict(plain["nbest"])
    assert abs(dict(r64["nbest"])[(0,)] - dict(plain["nbest"])[(0,)]) < 1e-9
    assert abs(dict(r64["search"])[(0,)] - dict(r64["nbest"])[(0,)] - 1.0) < 1e-9
    got = {tuple(out[0][0, k, : out[2][0, k]].tolist()): float(out[3][0, k]) for k in range(int(out[4][0]))}
    assert abs(got[(0,)] - dict(plain["nbest"])[(0,)]) < 1e-5 and abs(got[(0, 2)] - (dict(plain["nbest"])[(0, 2)] + 3.0)) < 1e-5


def _first_kept(shape, T, start=0):
    for s in range(start, start + 64):
        if _reference(s, shape, T)[2] is not None:
            return s
    raise AssertionError("no seed passes the cut-margin rule")


def test_ragged_batch_with_junk_beyond_the_lengths():
    """one batch: lengths {11, 10, 1, 0, 4} with NaN beyond each length; the length-0 row is one empty hypothesis with score 0"""
    shape = (11, 5, 8, INF, 0.0, 1.0, 1.0, 2.0, 0, 0.0)
    T, C, W = shape[:3]
    lens = [T, T - 1, 1, 0, 4]
    seeds = [_first_kept(shape, T), _first_kept(shape, T - 1, 100), _first_kept(shape, 1, 7), 0, _first_kept(shape, 4, 3)]
    logp = np.full((len(lens), T, C), np.nan, dtype=np.float32)
    refs = []
    for b, (n, s) in enumerate(zip(lens, seeds)):
        if n:
            lp, r64, r32 = _reference(s, shape, n)
            logp[b, :n] = lp
        else:
            r64 = r32 = dict(nbest=[((), 0.0)], margin=np.inf, min_candidates=0)
        refs.append((r64, r32))
    out = _decode(logp, lens, shape)
    for b, (r64, r32) in enumerate(refs):
        err, tol = _check_row(("ragged", b), lens[b], W, *(o[b] for o in out), dict(r64["nbest"]), _e32(r64, r32))
        print(f"CTC_BEAM_BOOST ragged row {b} len={lens[b]}: n_hyp={out[4][b]} err={err:.3e} tol={tol:.3e}")
    assert out[4][3] == 1 and out[3][3, 0] == 0.0 and out[2][3, 0] == 0


# ------------------------------------------------------------------------------------------------ 4. streaming, bitwise
STREAM_SHAPES = [SHAPES[0], SHAPES[1], SHAPES[3]]
STREAM_SEEDS = (0, 1, 2)


def _cuts(T, kind):
    bounds = {"one": [], "ones": list(range(1, T)), "first": [1], "last": [T - 1], "c14": list(range(14, T, 14)),
              "random": sorted(set(np.random.default_rng(T).integers(1, T, size=max(2, T // 9)).tolist()))}[kind]
    edges = [0] + bounds + [T]
    return [b - a for a, b in zip(edges, edges[1:])]


@functools.lru_cache(maxsize=None)
def _stream_logp(T, C):
    return torch.from_numpy(np.stack([O.make_logp(s, T, C) for s in STREAM_SEEDS])).to(dev)


@functools.lru_cache(maxsize=None)
def _one_shot(shape, upto):
    return _decode(_stream_logp(shape[0], shape[1])[:, :upto], None, shape)


def _same(got, want, what=""):
    """bitwise: got may be wider than want (capacity >= T) and is compared up to hyp_len only"""
    gt, gf, gl, gs, gn = got
    wt, wf, wl, ws, wn = want
    assert np.array_equal(gn, wn) and np.array_equal(gl, wl), (what, gn, wn, gl, wl)
    assert np.array_equal(gs.view(np.int32), ws.view(np.int32)), (what, gs, ws)
    Lmax = int(wl.max()) if wl.size else 0
    mask = np.arange(Lmax)[None, None, :] < wl[:, :, None]
    assert np.array_equal(gt[:, :, :Lmax][mask], wt[:, :, :Lmax][mask]), what
    assert np.array_equal(gf[:, :, :Lmax][mask], wf[:, :, :Lmax][mask]), what


def _state_bits(state):
    torch.cuda.synchronize()
    return {n: t.cpu().numpy().copy() for n, t in state.arrays().items()}


@pytest.mark.parametrize("shape", STREAM_SHAPES, ids=[IDS[0], IDS[1], IDS[3]])
def test_any_chunking_gives_the_one_shot_bits_and_one_final_state(shape):
    from nemo_amd import ops
    T, C, W, theta, beta = shape[:5]
    lp = _stream_logp(T, C)
    models = _models(shape)
    want = _one_shot(shape, T)
    search = _decode(lp, None, shape, [(m, 0.0) if i == len(models) - 1 else (m, a) for i, (m, a) in enumerate(models)])
    assert want[3].tobytes() != search[3].tobytes()   # (the boost takes part)
    states = {}
    for kind in ("one", "ones", "first", "last", "c14", "random"):
        cuts = _cuts(T, kind)
        assert sum(cuts) == T and min(cuts) >= 1
        state, t0 = None, 0
        for n in cuts:
            out, state = ops.ctc_beam_decode_fused_stream(lp[:, t0:t0 + n].contiguous(), None, C - 1, W, theta, beta, state, models)
            t0 += n
            _same(_host(out), _one_shot(shape, t0), (shape, kind, t0))   # every emitted n-best: the one-shot search so far
        assert (state.fs is not None) == (len(models) == 2) and state.bound == T
        states[kind] = _state_bits(state)
        assert states[kind]["frames_done"].tolist() == [T] * len(STREAM_SEEDS)
    live = np.arange(W)[None, :] < states["one"]["nb"][:, None]   # (slots without a beam hold what the frame loop left in them)
    for kind, bits in states.items():
        assert set(bits) == set(states["one"])
        for name, v in bits.items():
            a, b = (v, states["one"][name]) if v.ndim == 1 else (v[live], states["one"][name][live])
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (kind, name)
    # the state holds the SEARCH's ranks and order, not the final ones: brank is non-increasing along the slots
    br = states["one"]["brank"]
    assert all((np.diff(br[b, : states["one"]["nb"][b]]) <= 0).all() for b in range(br.shape[0]))
    # steps that only advance the state in between change nothing
    state, t0 = None, 0
    for i, n in enumerate(_cuts(T, "c14")):
        last = t0 + n == T
        out, state = ops.ctc_beam_decode_fused_stream(lp[:, t0:t0 + n].contiguous(), None, C - 1, W, theta, beta, state, models, emit=last)
        t0 += n
        assert (out is None) == (not last)
    _same(_host(out), want, (shape, "sparse"))


def test_one_ngram_model_streams_the_same_through_both_entries():
    """the streamed form of the one-model equivalence: `ctc_beam_decode_stream` with an LM and `ctc_beam_decode_fused_stream` with
    that LM alone, over the same chunks (T = 70 in tens of 7, the n-best asked for on the last one), give the same n-best and write
    the same state, byte for byte"""
    from nemo_amd import ops
    T, C, W, alpha = 70, 70, 8, 0.5
    lp, lm = _stream_logp(T, C), _device_lm(C - 1, 3)
    ends = {}
    for via in ("lm", "fused"):
        state = None
        for t0 in range(0, T, 7):
            args = (lp[:, t0:t0 + 7].contiguous(), None, C - 1, W, INF, 0.0, state)
            last = t0 + 7 == T
            if via == "lm":
                out, state = ops.ctc_beam_decode_stream(*args, lm=lm, alpha=alpha, emit=last)
            else:
                out, state = ops.ctc_beam_decode_fused_stream(*args, [(lm, alpha)], emit=last)
            assert (out is None) == (not last)
        ends[via] = (_host(out), _state_bits(state))
    (a, sa), (b, sb) = ends["lm"], ends["fused"]
    assert a[4].tolist() == [W] * len(STREAM_SEEDS)   # (full sets: every slot of the state is a beam)
    _same(b, a, "fused against lm")
    assert set(sa) == set(sb) and {"lm_state", "lm_sum"} <= set(sa)
    for name in sa:
        assert sa[name].tobytes() == sb[name].tobytes(), name


# ------------------------------------------------------------------------------------------------ 5. bad arguments
def test_bad_arguments_raise():
    from nemo_amd import ops
    from nemo_amd.modules import CTCBeamStreamState as S
    lp = torch.zeros(1, 4, 5, device=dev)
    lens = torch.tensor([4], device=dev)
    t = _tree(37, 5, 1.0, 2.0)
    lm = _device_lm(4, 3)
    args = dict(blank=4, beam_size=4, beam_threshold=20.0, beam_beta=0.0, models=[(lm, 0.5), (t, 1.0)])
    for kw in (dict(models=[(lm, 0.5), (t, -1.0)]), dict(models=[(lm, float("nan")), (t, 1.0)]), dict(models=[(t, -0.5)]), dict(blank=3),
               dict(beam_size=65), dict(beam_size=0), dict(beam_threshold=0.0), dict(models=[]), dict(models=[(t, 1.0)] * 3),
               dict(models=[(_device_lm(28, 3), 0.5), (t, 1.0)])):
        with pytest.raises(ValueError):
            ops.ctc_beam_decode_fused(lp, lens, **dict(args, **kw))
        with pytest.raises(ValueError):
            ops.ctc_beam_decode_fused_stream(lp, lens, state=None, **dict(args, **kw))
    with pytest.raises(TypeError):
        ops.ctc_beam_decode_fused(lp, lens, **dict(args, models=[(t.to(dev), 1.0)]))   # loose tensors are not taken
    for state in (S.fresh(1, 4, dev, lm=True), S.fresh(1, 4, dev), S.fresh(2, 4, dev, lm=True, second=True)):
        with pytest.raises(ValueError):
            ops.ctc_beam_decode_fused_stream(lp, lens, state=state, **args)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. decoding object and models
def _letters_run(ids, vocab, n=3):
    """the first run of 2..n letter tokens of a hypothesis (no space, no apostrophe: what every text parser keeps as it is)"""
    run = []
    for i in ids:
        if vocab[i].isalpha():
            run.append(i)
            if len(run) == n:
                break
        elif len(run) >= 2:
            break
        else:
            run = []
    return run if len(run) >= 2 else None


def _phrases_of(plain_lists, vocab):
    """key phrases from the model's own plain-beam n-best: a run of letters from the SECOND hypothesis of each utterance (the best
    one where there is no other), so that the boost changes the ranking"""
    out = []
    for l in plain_lists:
        for _, ids, _ in (l[1:] + l[:1]):
            run = _letters_run(ids, vocab)
            if run is not None:
                out.append("".join(vocab[i] for i in run))
                break
    assert out
    return out


def _boost_cfg(phrases, alpha=2.0, path=None):
    tree = dict(context_score=1.0, depth_scaling=2.0)
    if path is None:
        tree["key_phrases_list"] = phrases
    else:
        with open(path, "w", encoding="utf-8") as f:
            f.write("\n".join(phrases) + "\n")
        tree["key_phrases_file"] = str(path)
    return dict(strategy="beam_batch", beam=dict(beam_size=4, return_best_hypothesis=False, boosting_tree=tree, boosting_tree_alpha=alpha))


def _check_model(model, waves, phrases):
    """transcribe under beam_batch = the decoding object on the model's own log-probabilities"""
    from nemo_amd.models.ctc_models import _audio_batch, _inference_setup
    dec = model._ctc_decoding()
    assert type(dec).__name__ == "BeamBatchedCTCDecoder" and dec.beam_size == 4 and not dec.return_best_hypothesis
    if phrases is None:
        assert dec.boosting_tree is None
    else:
        want_ids = tuple(dict.fromkeys(tuple(dec.vocabulary.index(c) for c in p) for p in phrases))
        assert dec.boosting_tree.phrases == want_ids and dec.boosting_tree_alpha == 2.0
    with torch.no_grad(), _inference_setup(model):
        lp, n = model._ctc_log_probs(*_audio_batch(model, waves))
    want = dec.nbest(lp, n)
    lists = model.transcribe(waves, batch_size=2, return_hypotheses=True)
    assert len(lists) == len(waves) and any(ids for l in lists for _, ids, _ in l)
    for l, w in zip(lists, want):
        assert 1 <= len(l) <= 4 and [(ids, s) for _, ids, s in l] == w
        assert [t for t, _, _ in l] == [dec.ids_to_text(ids) for ids, _ in w]
        assert all(a[2] >= b[2] for a, b in zip(l, l[1:]))   # best first, by the final score
    if phrases is not None:   # what is returned holds the completed phrases only: score - alpha * boost_final is an acoustic score,
        # which the exact likelihood bounds (the slack of test_ctc_beam_lm_gpu.py: <= 32 frames, 4 roundings a frame, ulp(256))
        lp_cpu, n_cpu = lp.float().cpu().numpy(), n.cpu().tolist()
        assert max(n_cpu) <= 32
        for b, w in enumerate(want):
            for ids, s in w:
                am = s - dec.boosting_tree_alpha * dec.boosting_tree.score(ids)[1]
                assert abs(s) < 256 and am <= O.ctc_loglik(lp_cpu[b, : n_cpu[b]], ids, len(dec.vocabulary)) + 3.9e-3, (b, ids)
    return lists


def test_ctc_model_transcribes_with_the_boosted_search(tmp_path):
    import test_ctc_beam_lm_gpu as LG
    waves = LG._waves()
    plain = _check_model(LG._ctc_model(LG.BEAM4), waves, None)
    phrases = _phrases_of(plain, LG.VOCAB)
    model = LG._ctc_model(_boost_cfg(phrases))
    lists = _check_model(model, waves, phrases)
    assert LG._predict_best(model) == [l[0][0] for l in lists]
    assert [[(ids, s) for _, ids, s in l] for l in lists] != [[(ids, s) for _, ids, s in l] for l in plain]
    assert any(any(p in t for p in phrases) for l in lists for t, _, _ in l[:1])     # a boosted phrase is in a best hypothesis
    from_file = _check_model(LG._ctc_model(_boost_cfg(phrases, path=tmp_path / "phrases.txt")), waves, phrases)   # the file form
    assert from_file == lists


def test_hybrid_ctc_head_transcribes_with_the_boosted_search(tmp_path):
    import test_ctc_beam_lm_gpu as LG
    waves = LG._waves()
    model = LG._hybrid_model()
    model.change_decoding_strategy(LG.BEAM4, decoder_type="ctc")
    plain = _check_model(model, waves, None)
    phrases = _phrases_of(plain, LG.VOCAB)
    with pytest.raises(FileNotFoundError):   # refused before anything is replaced
        model.change_decoding_strategy(dict(strategy="beam_batch", beam=dict(boosting_tree=dict(key_phrases_file=str(tmp_path / "no.txt")),
                                                                             boosting_tree_alpha=1.0)), decoder_type="ctc")
    assert model._ctc_decoding().boosting_tree is None and _check_model(model, waves, None) == plain
    model.change_decoding_strategy(_boost_cfg(phrases), decoder_type="ctc")
    lists = _check_model(model, waves, phrases)
    assert LG._predict_best(model) == [l[0][0] for l in lists]
    assert [[(ids, s) for _, ids, s in l] for l in lists] != [[(ids, s) for _, ids, s in l] for l in plain]


def test_the_streaming_step_returns_the_offline_n_best():
    """conformer_stream_step under beam_batch with a boosting tree: every stream's last hypotheses = the one-shot fused search over
    the log-probabilities that stream was given, bitwise (the helpers of test_ctc_beam_stream_gpu.py)"""
    import test_ctc_beam_stream_gpu as SG
    m, vocab = SG._ctc_model(SG._beam4(None, best=False))
    plain, _ = SG._stream_model(m)
    phrases = []
    for r in plain:
        for _, ids, _ in (plain[r][0].n_best[1:] + plain[r][0].n_best[:1]):
            if len(ids) >= 2:
                phrases.append("".join(vocab[i] for i in ids[:3]))
                break
    assert phrases
    cfg = _boost_cfg(phrases)
    m, _ = SG._ctc_model(cfg)
    dec = m.wer.decoding
    assert dec.boosting_tree is not None and dec.ngram_lm is None
    out, last = SG._stream_model(m)
    assert last[0].dec_state[0] is last[2].dec_state[0] and [h.dec_state[1] for h in last] == [0, 1, 2]
    SG._check_rows(dec, out, best=False)
    assert any([(i, s) for _, i, s in out[r][0].n_best] != [(i, s) for _, i, s in plain[r][0].n_best] for r in out)
