"""No GPU: the resumable CTC beam search's C ABI (header, ctypes list, struct mirror, argument checks that come before any launch)
and `modules.CTCBeamStreamState` on CPU tensors (fresh values, `reserve`, `gather`, the mismatches `ops.ctc_beam_decode_stream`
refuses)."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mi355x_ctc_beam_decode_stream", "mi355x_ctc_beam_decode_lm_stream")
FIELDS = ("node", "par", "tok", "len", "h", "hp", "pb", "pnb", "tot", "brank", "lm_state", "lm_sum", "nb", "frames_done")
NEG = float("-inf")


def test_symbols_and_struct_are_declared_and_listed():
    from nemo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mi355x_asr.h")).read()
    declared = set(re.findall(r"\b(mi355x_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    body = re.search(r"typedef struct mi355x_ctc_beam_stream_state \{(.*?)\} mi355x_ctc_beam_stream_state;", hdr, re.S)
    assert body, "the state struct is not declared"
    assert tuple(re.findall(r"\*\s*([a-z_]+);", body.group(1))) == FIELDS


def test_struct_mirror_matches_the_header():
    from nemo_amd.ops import _CTCBeamStateC
    assert tuple(n for n, _ in _CTCBeamStateC._fields_) == FIELDS
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mi355x_asr.h"\nint main(){ printf("%zu", sizeof(mi355x_ctc_beam_stream_state));\n'
           + "".join(f' printf(" %zu", offsetof(mi355x_ctc_beam_stream_state, {f}));\n' for f in FIELDS) + " return 0; }\n")
    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "t.c"), os.path.join(tmp, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = list(map(int, subprocess.check_output([exe]).decode().split()))
    assert vals == [ctypes.sizeof(_CTCBeamStateC)] + [getattr(_CTCBeamStateC, f).offset for f in FIELDS]


def _call(lm=False, **over):
    """a stream entry with plausible non-null arguments (nothing is launched where the arguments are refused) and `over` applied"""
    from nemo_amd import _lib
    from nemo_amd.ops import _CTCBeamStateC
    keep = [torch.zeros(64, dtype=torch.int64) for _ in range(12)]   # host memory: never dereferenced by a refused call
    p = lambda i: keep[i].data_ptr()
    state = lambda base: _CTCBeamStateC(**{f: p(base) for f in FIELDS})
    a = dict(logp=p(0), lens=p(1), ws=p(2), tokens=p(3), tok_frame=p(4), hyp_len=p(5), score=p(6), n_hyp=p(7), B=1, T=2, C=5, blank=4,
             W=4, theta=20.0, beta=0.0, Tcap=8, s_in=state(8), s_out=state(9))
    a.update(over)
    ref = lambda s: ctypes.byref(s) if s is not None else None
    head = (a["logp"], a["lens"], a["ws"], a["tokens"], a["tok_frame"], a["hyp_len"], a["score"], a["n_hyp"], a["B"], a["T"], a["C"],
            a["blank"], a["W"], a["theta"], a["beta"])
    tail = (a["Tcap"], ref(a["s_in"]), ref(a["s_out"]), None)
    if lm:
        return _lib.lib.mi355x_ctc_beam_decode_lm_stream(*head, p(10), p(10), p(10), p(10), p(10), p(10), a.get("n_states", 2),
                                                         a.get("n_arcs", 4), a.get("alpha", 0.5), 0.0, *tail)
    return _lib.lib.mi355x_ctc_beam_decode_stream(*head, *tail)


def _state_without(field, base=9):
    from nemo_amd.ops import _CTCBeamStateC
    t = torch.zeros(16, dtype=torch.int64)
    s = _CTCBeamStateC(**{f: t.data_ptr() + 8 * base for f in FIELDS if f != field})
    s._keep = t
    return s


@pytest.mark.parametrize("lm", [False, True])
def test_bad_arguments_are_refused_before_any_launch(lm):
    bad = [dict(s_out=None), dict(s_out=_state_without("brank")), dict(s_in=_state_without("frames_done")), dict(Tcap=0),
           dict(Tcap=0x3fffffff // 4 + 1), dict(tokens=None), dict(n_hyp=None, score=None), dict(W=65), dict(W=0), dict(C=8193),
           dict(theta=0.0), dict(beta=float("nan")), dict(logp=None), dict(ws=None), dict(blank=5), dict(T=0)]
    if lm:
        bad += [dict(s_out=_state_without("lm_sum")), dict(s_in=_state_without("lm_state")), dict(alpha=-1.0), dict(n_states=1),
                dict(blank=3)]
    for over in bad:
        assert _call(lm, **over) == 1, over
    same = _state_without(None)
    assert _call(lm, s_in=same, s_out=same) == 1   # in place


def test_fresh_shapes_dtypes_and_values():
    from nemo_amd.modules import CTCBeamStreamState as S
    s = S.fresh(3, 5, "cpu", capacity=16, lm=True)
    assert (s.B, s.W, s.lm, s.bound, s.capacity) == (3, 5, True, 0, 16)
    assert s.tree.shape == (3, 16, 5, 2) and s.tokens.shape == s.tok_frame.shape == (3, 5, 16)
    assert s.tree.dtype == s.tokens.dtype == s.tok_frame.dtype == s.beams.dtype == s.utt.dtype == torch.int32 and s.h64.dtype == torch.int64
    a = s.arrays()
    assert set(a) == set(FIELDS)
    for n, t in a.items():
        assert t.shape == ((3,) if n in ("nb", "frames_done") else (3, 5)) and t.is_contiguous(), n
        assert t.dtype == (torch.int64 if n in ("h", "hp") else torch.float32 if n in ("pb", "pnb", "tot", "brank", "lm_sum") else torch.int32)
    # the one-shot search's initial values
    first = torch.tensor([0.0] + [NEG] * 4).expand(3, 5)
    assert torch.equal(a["pb"], first) and torch.equal(a["tot"], first) and torch.equal(a["brank"], first)
    assert (a["pnb"] == NEG).all() and (a["lm_sum"] == 0).all() and (a["lm_state"] == 1).all()
    assert (a["node"] == 0).all() and (a["par"] == -1).all() and (a["tok"] == -1).all() and (a["len"] == 0).all()
    assert (a["h"] == 0x243F6A8885A308D3).all() and (a["hp"] == 0).all() and (a["nb"] == 1).all() and (a["frames_done"] == 0).all()
    assert set(S.fresh(2, 4, "cpu").arrays()) == set(FIELDS) - {"lm_state", "lm_sum"}
    for B, W, cap in ((0, 4, 8), (1, 0, 8), (1, 65, 8), (1, 4, 0), (1, 64, 0x3fffffff // 64 + 1)):   # (refused before any allocation)
        with pytest.raises(ValueError):
            S.fresh(B, W, "cpu", capacity=cap)


def test_reserve_doubles_and_keeps_the_tree():
    from nemo_amd.modules import CTCBeamStreamState as S
    s = S.fresh(2, 3, "cpu", capacity=4)
    pattern = torch.arange(2 * 4 * 3 * 2, dtype=torch.int32).view(2, 4, 3, 2) + 7
    s.tree.copy_(pattern)
    s.bound = 3
    tree = s.tree
    assert s.reserve(1) is s and s.tree is tree and s.capacity == 4   # 3 + 1 fits
    s.reserve(2)                                                        # 5 > 4: one doubling
    assert s.capacity == 8 and s.tree.shape == (2, 8, 3, 2) and s.tokens.shape == s.tok_frame.shape == (2, 3, 8)
    assert torch.equal(s.tree[:, :4], pattern) and s.tree.is_contiguous()
    s.reserve(30)                                                       # 33 > 8: doubles to 64
    assert s.capacity == 64 and torch.equal(s.tree[:, :4], pattern) and s.bound == 3
    n = s.next(30)
    assert n.bound == 33 and n.tree is s.tree and n.tokens is s.tokens and n.beams is not s.beams and (n.B, n.W, n.lm) == (2, 3, False)


def test_gather_selects_rows():
    from nemo_amd.modules import CTCBeamStreamState as S
    a, b = S.fresh(3, 2, "cpu", capacity=4), S.fresh(2, 2, "cpu", capacity=8)
    for k, s in enumerate((a, b)):
        s.beams.copy_(torch.arange(s.beams.numel(), dtype=torch.int32).view_as(s.beams) + 1000 * k)
        s.h64.copy_(torch.arange(s.h64.numel()).view_as(s.h64) + 50 * k)
        s.utt.copy_(torch.arange(s.utt.numel(), dtype=torch.int32).view_as(s.utt) + 10 * k)
        s.tree.copy_(torch.arange(s.tree.numel(), dtype=torch.int32).view_as(s.tree) + 100000 * k)
        s.bound = 3 + 4 * k
    g = S.gather([(a, 2), (b, 0), (a, 0)])
    assert (g.B, g.W, g.capacity, g.bound, g.lm) == (3, 2, 8, 7, False)
    for i, (s, r) in enumerate(((a, 2), (b, 0), (a, 0))):
        assert torch.equal(g.beams[:, i], s.beams[:, r]) and torch.equal(g.h64[:, i], s.h64[:, r]) and torch.equal(g.utt[:, i], s.utt[:, r])
        assert torch.equal(g.tree[i, : s.capacity], s.tree[r])
    assert g.beams.is_contiguous() and g.h64.is_contiguous() and g.utt.is_contiguous() and g.tree.data_ptr() != a.tree.data_ptr()
    with pytest.raises(ValueError):
        S.gather([(a, 3)])
    with pytest.raises(ValueError):
        S.gather([(a, 0), (S.fresh(1, 3, "cpu"), 0)])
    with pytest.raises(ValueError):
        S.gather([(a, 0), (S.fresh(1, 2, "cpu", lm=True), 0)])
    with pytest.raises(ValueError):
        S.gather([])


def test_state_mismatch_raises_before_any_launch():
    import ctc_beam_lm_oracle as L
    from nemo_amd import ops
    from nemo_amd.modules import CTCBeamStreamState as S, NGramLM
    logp = torch.zeros(2, 3, 5)
    with tempfile.TemporaryDirectory() as d:
        L.write_arpa(L.make_lm(0, 4, 2), os.path.join(d, "lm.arpa"))
        lm = NGramLM.from_arpa(os.path.join(d, "lm.arpa"), 4)
    for state, use_lm in ((S.fresh(3, 4, "cpu"), False), (S.fresh(2, 8, "cpu"), False), (S.fresh(2, 4, "cpu", lm=True), False),
                          (S.fresh(2, 4, "cpu"), True)):
        with pytest.raises(ValueError):
            ops.ctc_beam_decode_stream(logp, None, 4, 4, 20.0, 0.0, state, lm=lm if use_lm else None, alpha=0.5)
    with pytest.raises(ValueError):
        ops.ctc_beam_decode_stream(logp, None, 4, 65, 20.0, 0.0, None)


def test_config_still_builds_the_same_decoder():
    from nemo_amd.modules import BeamBatchedCTCDecoder, ctc_decoder_from_config
    d = ctc_decoder_from_config({"strategy": "beam_batch", "beam": {"beam_size": 8, "beam_threshold": 9.0, "beam_beta": 0.25}}, list("abc"))
    assert type(d) is BeamBatchedCTCDecoder
    assert (d.beam_size, d.beam_threshold, d.beam_beta, d.ngram_lm, d.ngram_lm_alpha, d.blank_id, d.return_best_hypothesis) == \
        (8, 9.0, 0.25, None, 0.0, 3, True)
    assert callable(d.decode_stream) and callable(d.nbest_stream)
