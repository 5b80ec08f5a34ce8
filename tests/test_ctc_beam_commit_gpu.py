"""-m gpu: committing the stable prefix of a streamed CTC beam search (`mi355x_ctc_beam_commit`) and searching on over the window
it leaves (`mi355x_ctc_beam_decode_window_stream`), through `ops.ctc_beam_commit`, the decoding object and the models.

Nothing here has a tolerance.  The commit is integer work, held bit for bit to its numpy restatement
(tests/ctc_beam_commit_oracle.py); the search keeps its bits, so committed tokens + the tail it returns are held to the one-shot
search over the same frames, which tests/test_ctc_beam_gpu.py holds to float64.  Inputs, seeds and shapes are those of
tests/test_ctc_beam_stream_gpu.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ctc_beam_boost_oracle as BO
import ctc_beam_commit_oracle as R
import ctc_beam_oracle as O
import test_ctc_beam_stream_gpu as T

pytestmark = pytest.mark.gpu
dev = "cuda"
SEEDS, SHAPES, LM_SHAPES, INF = T.SEEDS, T.SHAPES, T.LM_SHAPES, T.INF
IDS = [f"T{s[0]}-C{s[1]}-W{s[2]}" for s in SHAPES]
B = len(SEEDS)


def _chunks(Tn, n=None):
    """14-frame chunks; 5-frame chunks where the utterance is shorter than two of them (T = 12 and 24: a 14-frame chunk would leave
    nothing, or one commit, before the last chunk); or chunks of n frames"""
    n = n or (14 if Tn >= 28 else 5)
    return [min(n, Tn - t) for t in range(0, Tn, n)]


def _np(t):
    return t.detach().cpu().numpy().copy()


def _bits(state):
    """a state on the host: (arrays, window, tree [B, Tcap, W, 2])"""
    torch.cuda.synchronize()
    arrays = {n: _np(t) for n, t in state.arrays().items()}
    win = {n: _np(t) for n, t in state.window_arrays().items()}
    return arrays, win, _np(state.tree)


def _eq(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def _commit_checked(state, stable, what):
    """the device commit of `state`, held to the restatement on the host copy of the same state -> (new tokens, the next state)"""
    from nemo_amd import ops
    arrays, win, tree = _bits(state)
    want_state, want_win, want_tree, want_com = R.commit(arrays, win, tree, stable)
    new, nxt = ops.ctc_beam_commit(state, stable)
    got_state, got_win, got_tree = _bits(nxt)
    assert set(got_state) == set(want_state)
    for name in want_state:
        _eq(got_state[name], want_state[name], (what, name))
    for name in ("tok_base", "frame_base", "kept"):
        _eq(got_win[name], want_win[name], (what, name))
    for b in range(state.B):
        k = int(want_win["kept"][b])
        _eq(got_win["frame_map"][b, :k], want_win["frame_map"][b, :k], (what, "frame_map", b))
        _eq(got_tree[b, :k], want_tree[b, :k], (what, "tree", b))
        assert (new[b][0], new[b][1]) == want_com[b], (what, "committed", b)
        assert nxt.committed[b] == (tuple(state.committed[b][0]) + tuple(want_com[b][0]),
                                    tuple(state.committed[b][1]) + tuple(want_com[b][1]))
    assert _np(nxt.win[3]).tolist() == [len(c[0]) for c in want_com] and nxt.bound == int(want_win["kept"].max())
    return new, nxt


def _search(shape, models=()):
    """(step(lp, state, emit) -> (host result or None, next state), fresh() -> state, one_shot(frames) -> host result)"""
    from nemo_amd import ops
    from nemo_amd.modules import CTCBeamStreamState
    Tn, C, W, theta, beta = shape
    lp = T._logp(Tn, C)
    models = list(models)

    def step(chunk, state, emit=True):
        if models:
            out, nxt = ops.ctc_beam_decode_fused_stream(chunk.contiguous(), None, C - 1, W, theta, beta, state, models, emit=emit)
        else:
            out, nxt = ops.ctc_beam_decode_stream(chunk.contiguous(), None, C - 1, W, theta, beta, state, emit=emit)
        return (T._host(out) if emit else None), nxt

    def fresh(capacity=64):
        return CTCBeamStreamState.fresh(B, W, dev, capacity=capacity, lm=len(models) >= 1, second=len(models) == 2)

    def one_shot(frames):
        if models:
            return T._host(ops.ctc_beam_decode_fused(lp[:, :frames].contiguous(), None, C - 1, W, theta, beta, models))
        return T._one_shot(shape, frames)

    return lp, step, fresh, one_shot


def _whole(res, state):
    """the hypotheses of a result in full: the state's committed tokens and frames in front of the tails"""
    tokens, frames, hyp_len, score, n_hyp = res
    done = [len(c[0]) for c in state.committed]
    Lmax = max(1, int(hyp_len.max()) + max(done))
    wt, wf = (np.full(tokens.shape[:2] + (Lmax,), -7, dtype=np.int32) for _ in range(2))
    wl = hyp_len.copy()
    for b in range(tokens.shape[0]):
        for k in range(int(n_hyp[b])):
            n = int(hyp_len[b, k])
            wt[b, k, : done[b] + n] = list(state.committed[b][0]) + tokens[b, k, :n].tolist()
            wf[b, k, : done[b] + n] = list(state.committed[b][1]) + frames[b, k, :n].tolist()
            wl[b, k] = done[b] + n
    return wt, wf, wl, score, n_hyp


# ------------------------------------------------------------------------------------------------ 1. the kernel against the restatement
@pytest.mark.parametrize("stable", [None, 0, 7, 28], ids=lambda s: f"S{s}")
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_commit_is_its_restatement_bit_for_bit(shape, stable):
    """after every chunk the state is committed on the device and, from its host copy, by the restatement: every state array, the
    window, the frame map, the kept frames of the tree and the committed tokens are equal; the stream goes on from the committed
    state, so later commits compose windows"""
    lp, step, fresh, _ = _search(shape)
    state, t0, early = fresh(), 0, [0] * B
    chunks = _chunks(shape[0])
    for i, n in enumerate(chunks):
        _, state = step(lp[:, t0:t0 + n], state, emit=False)
        t0 += n
        _, state = _commit_checked(state, stable, (shape, stable, t0))
        arrays, win, _ = _bits(state)
        assert (win["frame_base"] == t0).all() and (arrays["frames_done"] == win["kept"]).all()
        if stable is not None:
            assert (win["kept"] <= stable).all()
        if i < len(chunks) - 1:
            early = [len(c[0]) for c in state.committed]
    if stable is None:   # against a vacuous pass: a seed of this shape commits something before its last chunk
        assert max(early) >= 1, (shape, early)


# ------------------------------------------------------------------------------------------------ 2. the exact commit changes nothing
def _exact_commit_run(shape, every, models=(), chunk=None):
    lp, step, fresh, one_shot = _search(shape, models)
    state, t0, early, dropped = fresh(), 0, 0, 0
    chunks = _chunks(shape[0], chunk)
    for i, n in enumerate(chunks):
        res, state = step(lp[:, t0:t0 + n], state)
        t0 += n
        T._same(_whole(res, state), one_shot(t0), (shape, every, t0))
        if i < len(chunks) - 1:
            if (i + 1) % every == 0:
                frames = state.utt[1].clone()
                _, state = ops_commit(state)
                dropped += int((frames - state.win[2]).sum())
            early = max(len(c[0]) for c in state.committed)
    assert t0 == shape[0]
    print(f"{shape} every {every} models {[(type(m).__name__, a) for m, a in models]}: before the last chunk at most {early} tokens of a "
          f"stream committed, {dropped} tree frames of all streams dropped")
    return early, dropped


def ops_commit(state, stable=None):
    from nemo_amd import ops
    return ops.ctc_beam_commit(state, stable)


@pytest.mark.parametrize("every", [1, 3], ids=["every-chunk", "every-third"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_exact_commit_changes_no_result(shape, every):
    """stable_frames None: at every step committed + tail = the one-shot search over the frames so far -- tokens, frames, lengths,
    score bits, n_hyp.  (T = 12 and 24 in 5-frame chunks: with 14 frames a chunk nothing would be committed before the end.  Every
    third chunk: T = 37 in 5-frame and T = 12 in 3-frame chunks, which puts a commit at frames 15 and 30, and at frame 9, where the
    float32 oracle's n-best shares 3 / 3 / 4 and 2 / 0 / 0 leading tokens over the three seeds; in their usual chunks these two
    streams have three chunks and would never be committed.)"""
    chunk = {37: 5, 12: 3}.get(shape[0]) if every == 3 else None
    early, _ = _exact_commit_run(shape, every, chunk=chunk)
    assert early >= 1, (shape, every)   # against a vacuous pass: a seed committed a token while the stream was running


@functools.lru_cache(maxsize=None)
def _boost(Tn, C):
    from nemo_amd.modules import BoostingTree
    return BoostingTree.from_phrases(BO.make_phrases(Tn, C), C - 1, context_score=1.0, depth_scaling=2.0)


@pytest.mark.parametrize("kind", ["trigram", "tree", "trigram+tree", "light-trigram", "light-trigram+tree"])
@pytest.mark.parametrize("shape", LM_SHAPES, ids=[IDS[3], IDS[4]])
def test_the_exact_commit_changes_no_result_with_fusion_models(shape, kind):
    """the same with the trigram (one model, no final term), a boosting tree (the final re-ordering of the output) and both: the
    three fused window kernels.  Against a vacuous pass a seed must commit a token before the last chunk, so that the kernel runs
    with a non-zero tok_base.  At the stream test's trigram weight 0.5 that does not happen on these two shapes (measured: 0 tokens
    with the trigram and with trigram + tree on both; the model spreads the hypotheses), so those four runs can only ask that the
    frame map was not the identity (a tree frame was dropped), and the `light` runs, the same models at weight 0.1 (measured: 3 / 2
    tokens with the trigram, 8 / 3 with the tree beside it; the tree alone 14 / 1), carry the condition for those kernels."""
    Tn, C = shape[:2]
    alpha = 0.1 if "light" in kind else T.ALPHA   # (a lighter model spreads the hypotheses less: more is committed)
    models = ([(T._lm(C - 1), alpha)] if "trigram" in kind else []) + ([(_boost(Tn, C), 1.0)] if "tree" in kind else [])
    early, dropped = _exact_commit_run(shape, 1, models)
    if "light" in kind or kind == "tree":
        assert early >= 1, (shape, kind)
    else:
        assert dropped >= 1, (shape, kind)


# ------------------------------------------------------------------------------------------------ 3. the forced commit
@functools.lru_cache(maxsize=None)
def _logp600():
    return torch.from_numpy(np.stack([O.make_logp(s, 600, 33) for s in SEEDS])).to(dev)


@pytest.mark.parametrize("Tn", [200, 600])
def test_the_forced_commit_bounds_the_tree_and_only_adds_text(Tn):
    from nemo_amd.modules import BeamBatchedCTCDecoder
    lp = T._logp(200, 33) if Tn == 200 else _logp600()
    _, step, fresh, _ = _search(SHAPES[2])
    dec = BeamBatchedCTCDecoder(vocabulary=[str(i) for i in range(32)], beam_size=3, beam_threshold=INF, return_best_hypothesis=False)
    state, t0, commits = fresh(capacity=64), 0, 0
    for i, n in enumerate(_chunks(Tn)):
        before = state
        res, state = step(lp[:, t0:t0 + n], state)
        hyps, same = dec.nbest_stream(lp[:, t0:t0 + n], None, before)   # the same step through the decoding object: whole hypotheses
        t0 += n
        assert state.capacity == 64 and same.capacity == 64
        wt, wf, wl, score, n_hyp = _whole(res, state)
        for b in range(B):
            assert [(ids, np.float32(s).view(np.int32), fr) for ids, s, fr in hyps[b]] == \
                [(wt[b, k, : wl[b, k]].tolist(), score[b, k].view(np.int32), wf[b, k, : wl[b, k]].tolist()) for k in range(int(n_hyp[b]))]
            done = list(state.committed[b][0])
            assert all(ids[: len(done)] == done for ids, _, _ in hyps[b])
        if i % 2 == 1:
            old = state.committed
            _, state = _commit_checked(state, 28, (Tn, t0))
            commits += 1
            assert int(state.win[2].max()) <= 28 and state.bound <= 28
            for b in range(B):   # the committed text only grows
                assert state.committed[b][0][: len(old[b][0])] == old[b][0] and state.committed[b][1][: len(old[b][1])] == old[b][1]
    assert commits >= 7 and all(len(c[0]) >= 1 for c in state.committed) and state.capacity == 64
    assert all(list(c[1]) == sorted(c[1]) for c in state.committed)


def test_stable_frames_zero_commits_the_whole_best_hypothesis():
    shape = SHAPES[2]
    lp, step, fresh, _ = _search(shape)
    state, t0 = fresh(), 0
    for n in _chunks(shape[0])[:6]:
        res, state = step(lp[:, t0:t0 + n], state)
        t0 += n
        tokens, frames, hyp_len = res[0], res[1], res[2]
        new, state = _commit_checked(state, 0, (shape, t0))
        arrays, win, _ = _bits(state)
        assert arrays["nb"].tolist() == [1] * B and win["kept"].tolist() == [0] * B and arrays["node"][:, 0].tolist() == [0] * B
        for b in range(B):   # no final term here: output place 0 is slot 0 of the search
            assert new[b] == (tokens[b, 0, : hyp_len[b, 0]].tolist(), frames[b, 0, : hyp_len[b, 0]].tolist())
    assert all(len(c[0]) >= 1 for c in state.committed)


# ------------------------------------------------------------------------------------------------ 4. out of place, repeatable, gather
def test_a_commit_is_out_of_place_and_repeatable_and_gather_mixes_states():
    from nemo_amd.modules import CTCBeamStreamState
    shape = SHAPES[3]
    lp, step, fresh, one_shot = _search(shape)
    _, s0 = step(lp[:, :10], fresh())
    _, s0 = ops_commit(s0)                  # a committed state as the input: its window is not the zero one
    _, s1 = step(lp[:, 10:15], s0)
    before = _bits(s1)
    n1, c1 = ops_commit(s1)
    n2, c2 = ops_commit(s1)
    after = _bits(s1)
    for x, y in zip(before[:2], after[:2]):
        for name in x:
            _eq(x[name], y[name], name)
    _eq(before[2], after[2], "tree")
    assert n1 == n2 and c1.committed == c2.committed and c1.tree.data_ptr() != s1.tree.data_ptr() != c2.tree.data_ptr()
    b1, b2 = _bits(c1), _bits(c2)
    for x, y in zip(b1[:2], b2[:2]):
        for name in x:
            if name != "frame_map":
                _eq(x[name], y[name], name)
    for b in range(B):
        k = int(b1[1]["kept"][b])
        _eq(b1[1]["frame_map"][b, :k], b2[1]["frame_map"][b, :k], "frame_map")
        _eq(b1[2][b, :k], b2[2][b, :k], "tree")
    # gather: stream 0 from a state that was never committed, streams 1 and 2 from the committed one
    _, u = step(lp[:, :15], fresh())
    g = CTCBeamStreamState.gather([(u, 0), (c1, 1), (c1, 2)])
    assert g.win is not None and g.committed == [u.committed[0], c1.committed[1], c1.committed[2]]
    rg, g2 = step(lp[:, 15:], g)
    ru, u2 = step(lp[:, 15:], u)
    rc, c3 = step(lp[:, 15:], c1)
    want = one_shot(shape[0])
    for res, st in ((rg, g2), (ru, u2), (rc, c3)):
        T._same(_whole(res, st), want, "gather")
    ga, ua, ca = _bits(g2)[0], _bits(u2)[0], _bits(c3)[0]
    for name in ga:
        _eq(ga[name][:1], ua[name][:1], name)
        _eq(ga[name][1:], ca[name][1:], name)


# ------------------------------------------------------------------------------------------------ 5. bad arguments, clamps
def test_bad_arguments_raise():
    from nemo_amd import _lib, ops
    from nemo_amd.modules import CTCBeamStreamState as S
    from nemo_amd.ops import _CTCBeamFusedStateC, _CTCBeamWindowC
    W, cap = 4, 8
    a, b = S.fresh(B, W, dev, capacity=cap, lm=True), S.fresh(B, W, dev, capacity=cap, lm=True)
    plain = S.fresh(B, W, dev, capacity=cap)
    buf = torch.zeros(B * 3 * cap, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        ops.ctc_beam_commit(a, stable_frames=-2)

    def call(s_in=a, s_out=b, w_in=a, w_out=b, t_in=a, t_out=b, beam=W, Tcap=cap, n_models=1, nB=B, com=buf, ws=buf, hole=None):
        si, so = (_CTCBeamFusedStateC.of(s) if s is not None else None for s in (s_in, s_out))
        wi, wo = (_CTCBeamWindowC.of(s) if s is not None else None for s in (w_in, w_out))
        if hole is not None:   # one null array inside a record that is otherwise whole
            rec = dict(s_in=si.beams, s_out=so.beams, w_in=wi, w_out=wo)[hole[0]]
            assert getattr(rec, hole[1]) is not None
            setattr(rec, hole[1], None)
        ref = lambda x: ctypes.byref(x) if x is not None else None
        ptr = lambda t: t.data_ptr() if t is not None else None
        return _lib.lib.mi355x_ctc_beam_commit(ref(si), ref(wi), ptr(t_in.tree) if t_in is not None else None, ref(so), ref(wo),
                                               ptr(t_out.tree) if t_out is not None else None, ptr(com), ptr(buf), ptr(buf), ptr(ws), nB,
                                               beam, Tcap, n_models, -1, None)

    b.win, b.frame_map = torch.zeros(4, B, dtype=torch.int32, device=dev), torch.zeros(B, cap, dtype=torch.int32, device=dev)
    a.win, a.frame_map = torch.zeros_like(b.win), torch.zeros_like(b.frame_map)
    for bad in (dict(s_in=None), dict(s_out=None), dict(w_in=None), dict(w_out=None), dict(t_in=None), dict(t_out=None),
                dict(com=None), dict(ws=None), dict(beam=0), dict(beam=65), dict(Tcap=0), dict(Tcap=0x3fffffff // W + 1),
                dict(n_models=-1), dict(n_models=3), dict(nB=0), dict(n_models=2), dict(s_in=plain), dict(s_out=plain),
                dict(s_out=a), dict(t_out=a), dict(w_out=a),
                dict(hole=("w_in", "frame_map")), dict(hole=("w_in", "kept")), dict(hole=("w_out", "tok_base")),
                dict(hole=("w_out", "frame_base")), dict(hole=("s_in", "node")), dict(hole=("s_out", "node")),
                dict(hole=("s_in", "hp")), dict(hole=("s_out", "brank")), dict(hole=("s_in", "lm_sum")), dict(hole=("s_out", "nb"))):
        assert call(**bad) == 1, bad
    # the window entry: a null window, a window with a null array, the one-shot's refusals
    lp = T._logp(*SHAPES[0][:2])[:, :5].contiguous()
    C = lp.shape[2]
    lens = torch.full((B,), 5, dtype=torch.int64, device=dev)
    hl = torch.empty(B, W, dtype=torch.int32, device=dev)

    def search(window="ok", n_models=0, Tcap=cap, outs=5):
        so, si = _CTCBeamFusedStateC.of(b), _CTCBeamFusedStateC.of(a)
        w = _CTCBeamWindowC.of(a)
        if window == "hole":
            w.kept = None
        o = [t.data_ptr() for t in (a.tokens, a.tok_frame, hl, hl, hl)][:outs] + [None] * (5 - outs)
        return _lib.lib.mi355x_ctc_beam_decode_window_stream(lp.data_ptr(), lens.data_ptr(), a.tree.data_ptr(), *o, B, 5, C, C - 1, W,
                                                             INF, 0.0, None, n_models, Tcap, ctypes.byref(si), ctypes.byref(so),
                                                             ctypes.byref(w) if window else None, None)

    assert search(window=None) == 1 and search(window="hole") == 1 and search(n_models=1) == 1 and search(n_models=3) == 1
    assert search(Tcap=0) == 1 and search(outs=3) == 1
    assert search() == 0
    torch.cuda.synchronize()


GUARD, SENT = T.GUARD, T.SENT


def test_a_foreign_state_stays_inside_its_arrays():
    """reads the clamps: a state, a window and a tree of random words (node ids, parents, frames_done, nb, kept far outside their
    ranges) through the commit, exact and forced, and through the window search.  Every array the test hands over has guard words
    behind it and holds a sentinel, so a store that left its array would land in the test's own memory and be seen."""
    from nemo_amd import _lib
    from nemo_amd.modules import CTCBeamStreamState as S
    from nemo_amd.ops import _CTCBeamFusedStateC, _CTCBeamWindowC
    W, cap, C = 8, 16, 29
    g = torch.Generator().manual_seed(5)
    sizes = dict(h64=2 * B * W * 2, beams=10 * B * W, utt=2 * B, tree=B * cap * W * 2, tokens=B * W * cap, tok_frame=B * W * cap,
                 win=4 * B, frame_map=B * cap)

    def make(fill):
        bufs = {}
        for name, n in sizes.items():
            t = T._guarded(n)
            if fill:   # any word: half of them small, so that some ids and counts are plausible
                r = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64)
                small = torch.randint(-3, cap * W + 9, (n,), generator=g, dtype=torch.int64)
                t[:n] = torch.where(torch.rand(n, generator=g) < 0.5, r, small).to(torch.int32).to(dev)
            bufs[name] = t
        v = lambda name, *shape: bufs[name][: sizes[name]].view(*shape)
        st = S(v("h64", 2 * B * W * 2).view(torch.int64).view(2, B, W), v("beams", 10, B, W), v("utt", 2, B), v("tree", B, cap, W, 2),
               v("tokens", B, W, cap), v("tok_frame", B, W, cap), False, 0, win=v("win", 4, B), frame_map=v("frame_map", B, cap))
        return st, bufs

    def intact(bufs, untouched=()):
        torch.cuda.synchronize()
        for name, t in bufs.items():
            assert t[sizes[name]:].tolist() == [SENT] * GUARD, name
            if name in untouched:
                assert (t == SENT).all(), name

    com, n_com, ws = T._guarded(2 * B * cap), T._guarded(B), T._guarded(B * 3 * cap)
    for stable in (-1, 0, 5, 2 ** 31 - 1):
        src, src_bufs = make(True)
        keep = {n: t.clone() for n, t in src_bufs.items()}
        dst, dst_bufs = make(False)
        rc = _lib.lib.mi355x_ctc_beam_commit(ctypes.byref(_CTCBeamFusedStateC.of(src)), ctypes.byref(_CTCBeamWindowC.of(src)),
                                             src.tree.data_ptr(), ctypes.byref(_CTCBeamFusedStateC.of(dst)),
                                             ctypes.byref(_CTCBeamWindowC.of(dst)), dst.tree.data_ptr(), com.data_ptr(),
                                             com[B * cap:].data_ptr(), n_com.data_ptr(), ws.data_ptr(), B, W, cap, 0, stable, None)
        assert rc == 0
        intact(dst_bufs, untouched=("tokens", "tok_frame"))
        for name, t in src_bufs.items():   # the input is read only
            assert torch.equal(t, keep[name]), name
        for t, n in ((com, 2 * B * cap), (n_com, B), (ws, B * 3 * cap)):
            assert t[n:].tolist() == [SENT] * GUARD
        assert all(0 <= int(x) <= cap for x in n_com[:B].tolist()) and all(0 <= int(x) <= cap for x in dst.win[2].tolist())
        assert all(0 <= int(x) <= W for x in dst.utt[0].tolist())
    # the window search: a state and a tree of its own (8 frames of a stream), under a window of random words; what the window
    # adds to the search is the three values it clamps
    from nemo_amd import ops
    lp = T._logp(70, C)
    _, own = ops.ctc_beam_decode_stream(lp[:, :8].contiguous(), None, C - 1, W, INF, 0.0, S.fresh(B, W, dev, capacity=cap), emit=False)
    src, src_bufs = make(True)
    dst, dst_bufs = make(False)
    chunk = lp[:, 8:16].contiguous()
    lens = torch.full((B,), 8, dtype=torch.int64, device=dev)
    hl, sc, nh = T._guarded(B * W), T._guarded(B * W), T._guarded(B)
    rc = _lib.lib.mi355x_ctc_beam_decode_window_stream(chunk.data_ptr(), lens.data_ptr(), own.tree.data_ptr(), dst.tokens.data_ptr(),
                                                       dst.tok_frame.data_ptr(), hl.data_ptr(), sc.data_ptr(), nh.data_ptr(), B, 8, C,
                                                       C - 1, W, INF, 0.0, None, 0, cap, ctypes.byref(_CTCBeamFusedStateC.of(own)),
                                                       ctypes.byref(_CTCBeamFusedStateC.of(dst)), ctypes.byref(_CTCBeamWindowC.of(src)),
                                                       None)
    assert rc == 0
    intact(dst_bufs, untouched=("tree", "win", "frame_map"))
    for t, n in ((hl, B * W), (sc, B * W), (nh, B)):
        assert t[n:].tolist() == [SENT] * GUARD
    assert all(0 <= int(x) <= cap for x in hl[: B * W].tolist()) and dst.utt[1].tolist() == [16] * B


# ------------------------------------------------------------------------------------------------ 6. models
def _beam4(**keys):
    return dict(strategy="beam_batch", beam=dict(beam_size=4, return_best_hypothesis=True, **keys))


def _run(build, **keys):
    """the streams of T._stream_model through the model's streaming step, with the hypotheses of every step kept"""
    m, _ = build(_beam4(**keys))
    steps, inner = [], m.conformer_stream_step

    def recording(*a, **kw):
        res = inner(*a, **kw)
        steps.append(list(res[5]))
        return res

    m.conformer_stream_step = recording
    out, _ = T._stream_model(m)
    return out, steps


@pytest.mark.parametrize("build", [T._ctc_model, T._hybrid_model], ids=["ctc", "hybrid"])
def test_models_commit_while_they_stream(build):
    plain, plain_steps = _run(build)
    exact, exact_steps = _run(build, stream_commit_every=2)
    assert len(exact_steps) == len(plain_steps) >= 4
    for a, b in zip(plain_steps, exact_steps):   # the exact commit: every step returns what it returned without it
        for ha, hb in zip(a, b):
            assert ha.text == hb.text and ha.y_sequence.tolist() == hb.y_sequence.tolist() and ha.timestamp == hb.timestamp
            assert np.float32(ha.score).view(np.int32) == np.float32(hb.score).view(np.int32) and ha.length == hb.length
            assert ha.stable_length == 0 and 0 <= hb.stable_length <= hb.length
    for r in plain:
        assert plain[r][1] == exact[r][1] and torch.equal(plain[r][2], exact[r][2])
    assert exact_steps[-1][0].dec_state[0].win is not None and plain_steps[-1][0].dec_state[0].win is None
    forced, forced_steps = _run(build, stream_commit_every=2, stream_stable_frames=14)
    dec = forced_steps[-1][0].dec_state[0]
    assert dec.capacity == 64 and int(dec.win[2].max()) <= 14
    for k in range(3):
        stable, text = 0, ""
        for hyps in forced_steps:
            h = hyps[k]
            assert h.stable_length >= stable and h.stable_length <= h.length   # monotone
            ids = h.y_sequence.tolist()
            committed = h.dec_state[0].committed[h.dec_state[1]][0]
            assert list(committed[: h.stable_length]) == ids[: h.stable_length]
            assert h.text.startswith(text)   # the text starts with the committed text, and that only grows
            stable = h.stable_length
            text = _text_of(build, ids[:stable])
    assert max(h.stable_length for h in forced_steps[-1]) >= 1


def _text_of(build, ids):
    vocab = T.VOCAB if build is T._ctc_model else T.LABELS
    return "".join(vocab[i] for i in ids)
