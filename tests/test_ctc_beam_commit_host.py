"""No GPU: the numpy restatement of the commit (tests/ctc_beam_commit_oracle.py) on hand-built trees, where the answer is written
down by hand; the `beam` keys of the decoding section; the book-keeping of `CTCBeamStreamState` (on CPU tensors: nothing is
launched); and what the library refuses before it launches anything.

The first six tests run the restatement alone, against answers written down by hand: they guard the oracle that
tests/test_ctc_beam_commit_gpu.py holds the kernel to, not the product, and pass without it.  The others need the new code."""
import ctypes

import numpy as np
import pytest
import torch

import ctc_beam_commit_oracle as R

W, TCAP = 3, 8


def _nid(frame, slot):
    return 1 + frame * W + slot


def _state(nodes, tree, frames_done, lens=None):
    """one stream: beams at `nodes` (parents read from the tree), distinct float bits and hashes per slot"""
    nb = len(nodes)
    i32 = lambda v: np.array([list(v) + [0] * (W - nb)], dtype=np.int32)
    f32 = lambda k: np.array([[-(k + 0.25 * s) for s in range(W)]], dtype=np.float32)
    par = [int(tree[0, (n - 1) // W, (n - 1) % W, 0]) if n else -1 for n in nodes]
    tok = [int(tree[0, (n - 1) // W, (n - 1) % W, 1]) if n else -1 for n in nodes]
    return dict(node=i32(nodes), par=i32(par), tok=i32(tok), len=i32(lens or [0] * nb), pb=f32(1), pnb=f32(2), tot=f32(3), brank=f32(4),
                h=np.array([[101 + s for s in range(W)]], dtype=np.int64), hp=np.array([[201 + s for s in range(W)]], dtype=np.int64),
                nb=np.array([nb], dtype=np.int32), frames_done=np.array([frames_done], dtype=np.int32))


def _tree(pairs):
    """{(frame, slot): (parent, token)} -> [1, TCAP, W, 2]; everything else (0, -1)"""
    t = np.zeros((1, TCAP, W, 2), dtype=np.int32)
    t[..., 1] = -1
    for (f, s), v in pairs.items():
        t[0, f, s] = v
    return t


# frames 0, 2, 3 and 5 hold nodes, 1 and 4 are silence.  a = (0,0) tok 7; b = (2,1) tok 8 under a; c = (3,0) tok 9 and d = (3,2) tok 4
# under b; e = (5,1) tok 5 under c; u = (3,1) tok 6 under a: on no live chain
A_, B_, C_, D_, E_, U_ = _nid(0, 0), _nid(2, 1), _nid(3, 0), _nid(3, 2), _nid(5, 1), _nid(3, 1)
TREE = _tree({(0, 0): (0, 7), (2, 1): (A_, 8), (3, 0): (B_, 9), (3, 2): (B_, 4), (5, 1): (C_, 5), (3, 1): (A_, 6)})


def test_the_common_ancestor_is_committed_and_the_frames_behind_it_are_compacted():
    st = _state([E_, D_, C_], TREE, 6, lens=[4, 3, 3])
    out, win, tree, com = R.commit(st, R.fresh_window(1, TCAP), TREE)
    assert com == [([7, 8], [0, 2])]                       # root -> b, with the frames they were created in
    assert (int(win["tok_base"][0]), int(win["frame_base"][0]), int(win["kept"][0])) == (2, 6, 2)
    assert win["frame_map"][0, :2].tolist() == [3, 5]      # frames 3 and 5 stay; the silence frames 1 and 4 and frames 0, 2 go
    assert int(out["frames_done"][0]) == 2 and int(out["nb"][0]) == 3
    # the parent b became the root (0); u is in a kept frame and unreachable: (0, -1)
    assert tree[0, 0].tolist() == [[0, 9], [0, -1], [0, 4]] and tree[0, 1].tolist() == [[0, -1], [1, 5], [0, -1]]
    assert out["node"][0].tolist() == [_nid(1, 1), _nid(0, 2), _nid(0, 0)] and out["par"][0].tolist() == [1, 0, 0]
    for name in ("tok", "len", "h", "hp", "pb", "pnb", "tot", "brank"):   # everything else bit for bit
        assert out[name].tobytes() == st[name].tobytes(), name


def test_a_beam_that_is_the_ancestor_becomes_the_root():
    st = _state([E_, C_], TREE, 6)
    out, win, tree, com = R.commit(st, R.fresh_window(1, TCAP), TREE)
    assert com == [([7, 8, 9], [0, 2, 3])] and int(win["kept"][0]) == 1 and win["frame_map"][0, 0] == 5
    assert out["node"][0].tolist() == [_nid(0, 1), 0, 0] and out["par"][0].tolist() == [0, -1, -1]
    assert tree[0, 0].tolist() == [[0, -1], [0, 5], [0, -1]]
    # the empty third slot: what the search leaves in one
    assert out["tok"][0, 2] == -1 and out["h"][0, 2] == R.ROOT_HASH and out["hp"][0, 2] == 0
    assert out["tot"][0, 2:].view(np.uint32).tolist() == [0xFF800000]


def test_nothing_in_common_commits_nothing_and_still_drops_silence():
    tree = _tree({(0, 0): (0, 7), (0, 1): (0, 3), (2, 0): (_nid(0, 1), 8)})
    st = _state([_nid(0, 0), _nid(2, 0), 0], tree, 4)
    out, win, t2, com = R.commit(st, R.fresh_window(1, TCAP), tree)
    assert com == [([], [])] and int(win["kept"][0]) == 2 and win["frame_map"][0, :2].tolist() == [0, 2]
    assert int(win["frame_base"][0]) == 4 and out["node"][0].tolist() == [1, _nid(1, 0), 0] and out["par"][0].tolist() == [0, 2, -1]
    assert t2[0, 1, 0].tolist() == [2, 8]


def test_a_second_commit_composes_the_frame_map():
    st = _state([E_, D_, C_], TREE, 6)
    out, win, tree, _ = R.commit(st, R.fresh_window(1, TCAP), TREE)
    # two more frames: global 6 is silence, global 7 extends the beam at e (new frame 1) by token 2 in slot 0
    tree[0, 3, 0] = (_nid(1, 1), 2)
    st2 = {k: v.copy() for k, v in out.items()}
    st2["node"][0], st2["par"][0], st2["nb"][0], st2["frames_done"][0] = [_nid(3, 0), _nid(1, 1), 0], [_nid(1, 1), _nid(0, 0), -1], 2, 4
    out2, win2, tree2, com2 = R.commit(st2, win, tree)
    assert com2 == [([9, 5], [3, 5])]                      # global frames, through the first window
    assert (int(win2["tok_base"][0]), int(win2["frame_base"][0]), int(win2["kept"][0])) == (4, 8, 1)
    assert win2["frame_map"][0, 0] == 7 and out2["node"][0].tolist()[:2] == [1, 0] and tree2[0, 0, 0].tolist() == [0, 2]


def test_forced_pruning_keeps_the_beams_that_share_the_old_part_with_the_best():
    # slot 0 = e (a b c e), slot 1 = d (a b d), slot 2 = u (a u).  G = 6
    st = _state([E_, D_, U_], TREE, 6)
    win0 = R.fresh_window(1, TCAP)
    out, win, tree, com = R.commit(st, win0, TREE, stable_frames=3)   # cut 3: old = b, b, a -> u goes
    assert int(out["nb"][0]) == 2 and com == [([7, 8], [0, 2])] and int(win["kept"][0]) == 2 <= 3
    assert out["pb"][0, :2].tobytes() == st["pb"][0, :2].tobytes() and out["tok"][0].tolist() == [5, 4, -1]
    out, win, tree, com = R.commit(st, win0, TREE, stable_frames=2)   # cut 4: old = c, d, u -> slot 0 alone, and it is its own ancestor
    assert int(out["nb"][0]) == 1 and com == [([7, 8, 9, 5], [0, 2, 3, 5])] and int(win["kept"][0]) == 0
    out, win, tree, com = R.commit(st, win0, TREE, stable_frames=0)   # everything is old: slot 0's whole prefix
    assert int(out["nb"][0]) == 1 and com == [([7, 8, 9, 5], [0, 2, 3, 5])] and int(win["kept"][0]) == 0
    assert out["node"][0].tolist() == [0, 0, 0] and out["par"][0].tolist() == [-1, -1, -1]
    out, win, tree, com = R.commit(st, win0, TREE, stable_frames=6)   # nothing is old: the exact commit
    assert int(out["nb"][0]) == 3 and com == [([7], [0])]


def test_a_foreign_tree_ends_every_walk():
    tree = _tree({(1, 0): (_nid(1, 1), 3), (1, 1): (_nid(1, 0), 4), (2, 0): (_nid(5, 0), 5)})   # a cycle inside a frame; a parent ahead
    st = _state([_nid(1, 0), _nid(2, 0), _nid(6, 1)], tree, 3)   # and a beam at a node of a frame that is not done
    out, win, t2, com = R.commit(st, R.fresh_window(1, TCAP), tree)
    assert com == [([], [])] and out["node"][0].tolist() == [1, _nid(1, 0), 0]


# ------------------------------------------------------------------------------------------------ config
def test_the_decoding_section_takes_the_two_keys():
    from nemo_amd.modules.ctc_decoding import BeamBatchedCTCDecoder, ctc_decoder_from_config
    vocab = list("abcd")
    dec = ctc_decoder_from_config(dict(strategy="beam_batch", beam=dict(beam_size=4)), vocab)
    assert dec.stream_commit_every is None and dec.stream_stable_frames is None
    dec = ctc_decoder_from_config(dict(strategy="beam_batch", beam=dict(stream_commit_every=2, stream_stable_frames=14)), vocab)
    assert isinstance(dec, BeamBatchedCTCDecoder) and (dec.stream_commit_every, dec.stream_stable_frames) == (2, 14)
    dec = ctc_decoder_from_config(dict(strategy="beam_batch", beam=dict(stream_commit_every=3)), vocab)
    assert (dec.stream_commit_every, dec.stream_stable_frames) == (3, None)
    for beam in (dict(stream_stable_frames=14), dict(stream_commit_every=0), dict(stream_commit_every=2, stream_stable_frames=-1)):
        with pytest.raises(ValueError):
            ctc_decoder_from_config(dict(strategy="beam_batch", beam=beam), vocab)
        with pytest.raises(ValueError):   # also where the section is only being checked
            ctc_decoder_from_config(dict(strategy="beam_batch", beam=beam))


# ------------------------------------------------------------------------------------------------ the state's book-keeping
def _committed(B, cap, kept, ids):
    from nemo_amd.modules import CTCBeamStreamState as S
    s = S.fresh(B, W, "cpu", capacity=cap)
    s.win = torch.tensor([[len(ids)] * B, [40] * B, [kept] * B, [0] * B], dtype=torch.int32)
    s.frame_map = torch.arange(B * cap, dtype=torch.int32).view(B, cap)
    s.committed, s.bound = [(tuple(ids), tuple(range(len(ids))))] * B, kept
    return s


def test_the_state_carries_its_window_through_next_reserve_and_gather():
    from nemo_amd.modules import CTCBeamStreamState as S
    f = S.fresh(2, W, "cpu", capacity=8)
    assert f.win is None and f.committed == [((), ())] * 2 and f.steps == 0 and f.n_models == 0
    w = f.window_arrays()
    assert f.win is None and all(int(t.abs().sum()) == 0 for t in w.values()) and w["frame_map"].shape == (2, 8)
    s = _committed(2, 8, 5, [3, 4])
    n = s.next(6)
    assert n.win is s.win and n.frame_map is s.frame_map and n.committed == s.committed and n.bound == 11 and n.steps == 1
    n.reserve(6)   # 11 + 6 > 8: the tree and the map grow together, the map's frames copied
    assert n.capacity == 32 and n.frame_map.shape == (2, 32) and torch.equal(n.frame_map[:, :8], s.frame_map)
    s.reserve(3)   # 5 + 3 <= 8: the bound of a committed state is its window, so nothing grows
    assert s.capacity == 8
    g = S.gather([(f, 1), (n, 0)])   # an uncommitted stream and a committed one
    assert g.win[:, 0].tolist() == [0, 0, 0, 0] and g.win[:, 1].tolist() == [2, 40, 5, 0] and g.capacity == 32
    assert torch.equal(g.frame_map[1, :8], s.frame_map[0]) and int(g.frame_map[0].abs().sum()) == 0
    assert g.committed == [((), ()), ((3, 4), (0, 1))] and g.bound == 11 and g.steps == 1
    assert S.gather([(f, 0), (f, 1)]).win is None


def test_the_library_refuses_bad_commit_arguments_before_any_launch():
    from nemo_amd import _lib
    from nemo_amd.ops import _CTCBeamFusedStateC, _CTCBeamWindowC
    assert _lib.lib.mi355x_ctc_beam_commit_workspace_elems(8, 4) == 24
    assert _lib.lib.mi355x_ctc_beam_commit_workspace_elems(0, 4) == 0 and _lib.lib.mi355x_ctc_beam_commit_workspace_elems(8, 65) == 0
    # states of host tensors: every call below is refused by the argument checks, so nothing is launched or dereferenced
    a, b = _committed(1, 8, 2, [1]), _committed(1, 8, 2, [1])
    buf = torch.zeros(64, dtype=torch.int32)
    ptr = lambda t: t.data_ptr()

    def state_c(s):   # (the records by hand: `of` takes device tensors only)
        arr = s.arrays()
        c = _CTCBeamFusedStateC()
        for name, _ in type(c.beams)._fields_:
            setattr(c.beams, name, ptr(arr[name]) if name in arr else None)
        return c

    def window_c(s):
        return _CTCBeamWindowC(**{n: ptr(t) for n, t in s.window_arrays().items()})

    def call(s_in=a, s_out=b, w_in=a, w_out=b, t_in=a, t_out=b, beam=W, Tcap=8, n_models=0, B=1, com=buf, hole=None):
        si, so = (state_c(s) if s is not None else None for s in (s_in, s_out))
        wi, wo = (window_c(s) if s is not None else None for s in (w_in, w_out))
        if hole is not None:   # one null array inside a record that is otherwise whole
            rec = dict(s_in=si.beams, s_out=so.beams, w_in=wi, w_out=wo)[hole[0]]
            assert getattr(rec, hole[1]) is not None
            setattr(rec, hole[1], None)
        ref = lambda x: ctypes.byref(x) if x is not None else None
        return _lib.lib.mi355x_ctc_beam_commit(ref(si), ref(wi), ptr(t_in.tree) if t_in is not None else None, ref(so), ref(wo),
                                               ptr(t_out.tree) if t_out is not None else None, ptr(com) if com is not None else None,
                                               ptr(buf), ptr(buf), ptr(buf), B, beam, Tcap, n_models, -1, None)

    for bad in (dict(s_in=None), dict(s_out=None), dict(w_in=None), dict(w_out=None), dict(t_in=None), dict(t_out=None),
                dict(com=None), dict(beam=0), dict(beam=65), dict(Tcap=0), dict(n_models=-1), dict(n_models=3), dict(B=0),
                dict(n_models=1),                 # the states have no lm arrays
                dict(s_out=a), dict(t_out=a), dict(w_out=a),   # aliasing
                dict(hole=("w_in", "frame_map")), dict(hole=("w_out", "kept")), dict(hole=("s_in", "node")), dict(hole=("s_out", "tot"))):
        assert call(**bad) == 1, bad
    with pytest.raises(ValueError):
        _lib.check(call(Tcap=0), "ctc_beam_commit")
