"""CPU-side checks of CTC forced alignment and timestamps (no GPU): the float32 oracle (tests/ctc_align_oracle.py) against brute
force over every path, the C ABI's symbols and argument checks, the host-side offset builder on hand-written cases, and the
defaults of the public signatures."""
import ctypes
import inspect
import itertools

import numpy as np
import pytest

import ctc_align_oracle as A

BLANK = 2   # C = 3: labels 0, 1 and the blank


def _targets():
    out = [[]]
    for U in (1, 2, 3):
        out += [list(t) for t in itertools.product((0, 1), repeat=U)]   # every label sequence, repeats included
    return out


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_matches_brute_force(seed):
    """all T <= 6, U <= 3, C = 3: the oracle's score is the maximum over every frame-to-state path, its path is valid and attains
    it, and it reports infeasible exactly when there is no path (T < U + adjacent repeats)"""
    rng = np.random.RandomState(seed)
    n_inf = 0
    for T in range(0, 7):
        x = rng.randn(T, 3).astype(np.float32)
        logp = (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)
        for tgt in _targets():
            score, path, start, end = A.viterbi(logp, tgt, BLANK)
            best, arg = A.brute_force(logp, tgt, BLANK)
            assert (best is None) == (not A.feasible_by_length(T, tgt)), (T, tgt)
            if best is None:
                n_inf += 1
                assert path is None and score == -np.inf and start == [-1] * len(tgt) and end == [-1] * len(tgt)
                continue
            assert A.path_valid(path, tgt, T), (T, tgt, path)
            assert np.float32(score).tobytes() == np.float32(best).tobytes(), (T, tgt)
            assert A.path_score(logp, path, tgt, BLANK).tobytes() == np.float32(best).tobytes()
            assert tuple(path) in arg
            for u in range(len(tgt)):   # first / last frame in state 2u+1
                frames = [t for t, s in enumerate(path) if s == 2 * u + 1]
                assert frames and (start[u], end[u]) == (frames[0], frames[-1])
    assert n_inf > 0


def test_oracle_tie_rule_and_inf_emissions():
    """uniform emissions: every path has the same bits, the tie rule alone decides (stay first, final state S-1 first);
    -inf emissions on every path: infeasible although the lengths would allow a path"""
    logp = np.full((5, 3), np.float32(-1.25))
    score, path, start, end = A.viterbi(logp, [0, 0], BLANK)   # S = 5; needs 3 frames at least
    # backwards from S-1 = 4, `stay` wherever the same state was reachable one frame earlier: state 4 is reachable from frame 3 on
    # (1, 2, 3, 4 from state 1 at frame 0: no skip between equal labels), states 3, 2 not before frames 2, 1
    assert path == [1, 2, 3, 4, 4] and (start, end) == ([0, 2], [0, 2])
    assert score == np.float32(-1.25) * 5
    score, path, _, _ = A.viterbi(logp, [0, 1], BLANK)
    assert A.path_valid(path, [0, 1], 5) and path[-1] == 4
    bad = logp.copy()
    bad[2, :] = -np.inf
    assert A.viterbi(bad, [0], BLANK)[1] is None and A.viterbi(bad, [0], BLANK)[0] == -np.inf
    path, ts, te, sc = A.align_batch(bad[None], np.array([[0]]), [5], [1], BLANK)
    assert (path == -1).all() and (ts == -1).all() and (te == -1).all() and sc[0] == -np.inf
    # T = 0: feasible only for the empty target, score 0
    assert A.viterbi(logp[:0], [], BLANK)[0] == 0.0 and A.viterbi(logp[:0], [1], BLANK)[1] is None


def test_new_symbols_are_exported():
    from nemo_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mi355x_ctc_align", "mi355x_ctc_align_config", "mi355x_ctc_greedy_decode_ts"):
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS, name
    from nemo_amd import modules
    assert hasattr(modules, "CTCAligner") and hasattr(modules, "ctc_offsets")


def test_invalid_alignment_arguments_are_rejected_without_a_gpu():
    """the checks run before any launch: rc 1 = MI_ERR_ARG.  Non-null dummy pointers are never dereferenced on the host."""
    from nemo_amd import _lib
    L = _lib.lib
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 8   # 8-byte aligned, as the workspace has to be
    ok_ptrs = [p] * 9
    ok_sizes = dict(B=1, Tmax=4, C=3, Umax=2, blank=2)

    def align(ptrs=ok_ptrs, **kw):
        z = dict(ok_sizes, **kw)
        return L.mi355x_ctc_align(*ptrs, z["B"], z["Tmax"], z["C"], z["Umax"], z["blank"], None)
    for i in range(9):   # every pointer
        assert align([None if j == i else p for j in range(9)]) == 1, i
    for kw in (dict(B=0), dict(B=-1), dict(Tmax=0), dict(C=0), dict(Umax=0), dict(Umax=-3), dict(blank=-1), dict(blank=3),
               dict(Umax=2049)):   # non-positive sizes, blank outside [0, C), S = 4099: no form supports it
        assert align(**kw) == 1, kw
    assert align([p, p, p, p, p + 4, p, p, p, p]) == 1   # workspace not 8-byte aligned

    def greedy(ptrs, B=1, T=4, C=3, blank=2):
        return L.mi355x_ctc_greedy_decode_ts(*ptrs, B, T, C, blank, None)
    for i in (0, 2, 3, 4, 5, 6):   # (lens may be NULL: every utterance has T frames)
        assert greedy([None if j == i else p for j in range(7)]) == 1, i
    for kw in (dict(B=0), dict(T=0), dict(C=0), dict(blank=-1), dict(blank=3), dict(blank=4), dict(T=8193)):   # (blank = C is outside [0, C); T: labels + log-probs exceed the LDS)
        assert greedy([p] * 7, **kw) == 1, kw
    with pytest.raises(ValueError):
        _lib.check(align(B=0), "ctc_align")


def test_cpu_tensors_fail_loudly():
    import torch
    from nemo_amd import ops
    lp = torch.zeros(1, 4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ctc_align(lp, torch.zeros(1, 2, dtype=torch.int64), torch.tensor([4]), torch.tensor([2]), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ctc_greedy_decode_ts(lp, torch.tensor([4]), 2)


@pytest.mark.parametrize("case", sorted(A.OFFSET_CASES))
def test_offsets_on_hand_written_cases(case):
    from nemo_amd.modules import ctc_offsets
    (tokens, starts, ends, word_pieces), (char, word) = A.OFFSET_CASES[case]
    got_char, got_word = ctc_offsets(tokens, starts, ends, word_pieces=word_pieces)
    assert got_char == char
    assert got_word == word


def test_decoder_offsets_pick_the_vocabulary_kind():
    from nemo_amd.modules import GreedyCTCDecoder
    pieces = GreedyCTCDecoder(["▁he", "llo", "▁", "wor", "ld", "▁a"])
    (_, starts, ends, _), (char, word) = A.OFFSET_CASES["word_pieces"]
    assert pieces.offsets([0, 1, 2, 3, 4, 5], starts, ends) == (char, word)
    chars = GreedyCTCDecoder(["h", "i", " ", "y", "o", "u"])
    (_, starts, ends, _), (char, word) = A.OFFSET_CASES["chars"]
    assert chars.offsets([0, 1, 2, 3, 4, 5], starts, ends) == (char, word)
    assert chars.offsets([], [], []) == ([], [])
    with pytest.raises(ValueError):
        GreedyCTCDecoder(blank_id=4).offsets([0], [0], [0])


def test_signatures_default_to_todays_behaviour():
    from nemo_amd.models import EncDecCTCModel, EncDecHybridRNNTCTCModel
    from nemo_amd.modules import CTCAligner, GreedyCTCDecoder
    sig = inspect.signature(GreedyCTCDecoder.decode_ids)
    assert list(sig.parameters) == ["self", "log_probs", "lengths", "return_timestamps"]
    assert sig.parameters["return_timestamps"].default is False
    for cls in (EncDecCTCModel, EncDecHybridRNNTCTCModel):
        sig = inspect.signature(cls.transcribe)
        assert list(sig.parameters)[:7] == ["self", "audio", "batch_size", "return_hypotheses", "num_workers", "channel_selector",
                                            "verbose"]
        assert sig.parameters["timestamps"].default is False and sig.parameters["return_hypotheses"].default is False
        assert list(inspect.signature(cls.align).parameters)[:4] == ["self", "audio", "texts", "batch_size"]
        assert isinstance(cls.frame_stride_s, property)
    assert CTCAligner(vocabulary=list("abc")).blank_id == 3 and CTCAligner(blank_id=7).blank_id == 7
    with pytest.raises(ValueError):
        CTCAligner()


def test_frame_stride_and_text_to_ids():
    from nemo_amd.models import EncDecCTCModel, conformer_ctc_config
    vocab = [" "] + list("abcdefghij")
    cfg = conformer_ctc_config("small", vocab_size=len(vocab), d_model=32, n_heads=2, n_layers=1)
    cfg["decoder"]["vocabulary"] = vocab
    m = EncDecCTCModel(cfg)
    assert abs(m.frame_stride_s - 0.04) < 1e-12   # 10 ms hop x 4
    assert m._text_to_ids("ab c") == [1, 2, 0, 3] and m._text_to_ids("a?b") == [1, 2]   # characters outside the vocabulary are dropped
