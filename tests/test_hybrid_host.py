"""Host side (no GPU) of the hybrid transducer-CTC model and of streaming transducer decoding:
  * tests/stream_decode_oracle.py (the CPU restatement of the resumable greedy search) gives, for any chunking, what
    oracle/transducer_ref.greedy_decode and tests/tdt_oracle.tdt_greedy_decode give for the whole sequence -- and the settings the
    GPU tests run do hit the hard cases (a TDT jump over a chunk edge, frames with max_symbols labels) and meet the conditions of
    the 2 % rule (more than 150 decisions, more than 40 labels, fewer than 2 % near-ties in the fp32 search);
  * EncDecHybridRNNTCTCModel construction from a config with `aux_ctc`;
  * the two new C-ABI symbols are exported by the built library and declared in the header.
The first group checks the test helper against the existing oracles on the CPU, as the feature's issue asks, and so passes on a
tree without the feature once the helper is there; the model and symbol tests (and every GPU test) fail without it."""
import os
import re

import pytest
import torch

from oracle import transducer_ref as TR

import stream_decode_oracle as S
import tdt_oracle as O

DUR = [0, 1, 2, 3, 4]


def _cuttings(T):
    g = torch.Generator().manual_seed(77)
    rnd = sorted(set(torch.randint(1, T, (6,), generator=g).tolist()))
    return {"every frame": list(range(1, T)), "width 5": list(range(5, T, 5)), "random": rnd}


@pytest.mark.parametrize("max_symbols", [2, 10])
@pytest.mark.parametrize("kind", ["rnnt", "tdt"])
def test_chunked_oracle_equals_the_one_shot_oracles_and_hits_the_hard_cases(kind, max_symbols):
    V, T = S.SMALL["V"], S.SMALL["T"]
    lens = torch.tensor(S.SMALL["lens"])
    Pd, Pj = S.small_case(kind)
    enc = S.small_enc()
    if kind == "rnnt":
        want = TR.greedy_decode(Pd, Pj, enc, lens, V, max_symbols)
    else:
        want = O.tdt_greedy_decode(Pd, Pj, enc, lens, V, DUR, max_symbols)
    assert sum(len(w[0]) for w in want) > 20
    per_frame = torch.cat([torch.bincount(torch.tensor(w[1], dtype=torch.long), minlength=T)[: int(n)] for w, n in zip(want, lens)])
    assert int(per_frame.max()) == max_symbols and int(per_frame.min()) == 0, per_frame
    whole, fin1, _ = S.decode_chunked(Pd, Pj, enc, lens, V, max_symbols, [], DUR if kind == "tdt" else None)
    assert whole == want
    crossings = 0
    for name, cuts in _cuttings(T).items():
        got, fin, ev = S.decode_chunked(Pd, Pj, enc, lens, V, max_symbols, cuts, DUR if kind == "tdt" else None)
        assert got == want, name
        assert ev["full_frames"] > 0, name
        crossings += ev["crossings"]
        for a, b in zip(fin, fin1):
            assert torch.equal(a["h"], b["h"]) and torch.equal(a["c"], b["c"]) and a["last"] == b["last"]
            assert a["frames_done"] == b["frames_done"] and a["zero_run"] == b["zero_run"]
    if kind == "tdt":
        assert crossings > 0


@pytest.mark.parametrize("kind", ["rnnt", "tdt"])
def test_recipe_geometry_case_meets_the_conditions_of_the_two_percent_rule(kind):
    R = S.RECIPE
    V, ms = R["V"], R["max_symbols"]
    lens = torch.tensor(R["lens"])
    Pd, Pj = S.recipe_case(kind)
    enc = S.recipe_enc()
    gaps = []
    got, _, _ = S.decode_chunked(Pd, Pj, enc, lens, V, ms, [1, 14, 27, 64], DUR if kind == "tdt" else None, gaps=gaps)
    if kind == "rnnt":
        assert got == TR.greedy_decode(Pd, Pj, enc, lens, V, ms)
        rep = TR.forced_decode_margins(Pd, Pj, enc, lens, V, ms, got)
    else:
        assert got == O.tdt_greedy_decode(Pd, Pj, enc, lens, V, DUR, ms)
        rep = S.tdt_forced_decode_margins(Pd, Pj, enc, lens, V, DUR, ms, got)
    # the forced walk along the search's own output: every decision is its arg-max
    assert all(r[1] == r[2] and r[3] == 0.0 for rows in rep for r in rows)
    assert sum(len(rows) for rows in rep) == len(gaps) > 150 and sum(len(g[0]) for g in got) > 40
    near = sum(1 for gap, scale in gaps if gap < 2e-4 * scale)
    assert near < 0.02 * len(gaps), (near, len(gaps))


def test_tdt_forced_walk_flags_a_wrong_label():
    V, T = S.SMALL["V"], S.SMALL["T"]
    lens = torch.tensor(S.SMALL["lens"])
    Pd, Pj = S.small_case("tdt")
    enc = S.small_enc()
    hy = O.tdt_greedy_decode(Pd, Pj, enc, lens, V, DUR, 10)
    toks, times = list(hy[0][0]), list(hy[0][1])
    toks[2] = (toks[2] + 1) % V
    rep = S.tdt_forced_decode_margins(Pd, Pj, enc[:1], lens[:1], V, DUR, 10, [(toks, times)])
    bad = [r for r in rep[0] if r[1] != r[2]]
    assert bad and bad[0][3] > 0.0


def test_tdt_forced_walk_and_time_stamps():
    """what the walk sees of the DURATIONS, which hypotheses do not record: a label moved to a later frame than the search put it on
    is either refused (the walk cannot consume the hypothesis) or reported with a positive margin; a label moved EARLIER, onto a
    frame the walk's own durations jump over, is refused.  Not seen: a different duration that still lands on frames where the
    walk's own search says blank up to the next label -- such a hypothesis has the same labels on the same frames."""
    V = S.SMALL["V"]
    lens = torch.tensor(S.SMALL["lens"])
    Pd, Pj = S.small_case("tdt")
    enc = S.small_enc()
    toks, times = O.tdt_greedy_decode(Pd, Pj, enc, lens, V, DUR, 10)[0]
    caught = 0
    for pos in range(len(toks)):
        for shift in (1, -1):
            t2 = list(times)
            t2[pos] += shift
            if t2 != sorted(t2) or not 0 <= t2[pos] < int(lens[0]):
                continue
            try:
                rep = S.tdt_forced_decode_margins(Pd, Pj, enc[:1], lens[:1], V, DUR, 10, [(list(toks), t2)])
            except AssertionError:
                caught += 1
                continue
            assert any(r[1] != r[2] and r[3] > 0.0 for r in rep[0]), (pos, shift)
            caught += 1
    assert caught > 10


# ------------------------------------------------------------------------------------------------ the model class
def _cfg(**aux):
    from nemo_amd.models import fastconformer_hybrid_config
    labels = [chr(ord("a") + i) for i in range(26)] + [" ", "'"]
    cfg = fastconformer_hybrid_config("small", vocab_size=len(labels), d_model=32, n_heads=4, n_layers=1, subsampling_conv_channels=16,
                                      streaming=True, att_context_size=[16, 3])
    cfg["labels"] = labels
    cfg["decoder"]["prednet"].update(pred_hidden=32, dropout=0.0)
    cfg["joint"]["jointnet"].update(joint_hidden=32, dropout=0.0)
    cfg["aux_ctc"].update(aux)
    return cfg


def test_hybrid_model_construction():
    from nemo_amd.core import resolve_target
    from nemo_amd.models import EncDecHybridRNNTCTCModel, EncDecRNNTModel
    cfg = _cfg()
    m = EncDecHybridRNNTCTCModel(cfg)
    keys = list(m.state_dict())
    assert "ctc_decoder.decoder_layers.0.weight" in keys and "ctc_decoder.decoder_layers.0.bias" in keys
    assert {k.split(".")[0] for k in keys} >= {"encoder", "decoder", "joint", "ctc_decoder"}
    assert tuple(m.state_dict()["ctc_decoder.decoder_layers.0.weight"].shape) == (29, 32, 1)
    mods = m.trainable_modules()
    assert len(mods) == 4 and mods[3] is m.ctc_decoder
    assert m.ctc_loss_weight == 0.3 and m.ctc_decoder.vocabulary == cfg["labels"]
    assert m.encoder.att_context_style == "chunked_limited"
    cfg2 = _cfg()
    del cfg2["aux_ctc"]["ctc_loss_weight"]
    assert EncDecHybridRNNTCTCModel(cfg2).ctc_loss_weight == 0.5
    for name in ("EncDecHybridRNNTCTCModel", "EncDecHybridRNNTCTCBPEModel"):
        assert resolve_target("nemo.collections.asr.models." + name) is EncDecHybridRNNTCTCModel
    no_aux = _cfg()
    del no_aux["aux_ctc"]
    with pytest.raises(ValueError, match="aux_ctc"):
        EncDecHybridRNNTCTCModel(no_aux)
    with pytest.raises(NotImplementedError, match="aux_ctc"):   # the parent class keeps refusing the section
        EncDecRNNTModel(cfg)


def test_hybrid_change_decoding_strategy():
    from nemo_amd.models import EncDecHybridRNNTCTCModel
    m = EncDecHybridRNNTCTCModel(_cfg())
    assert m.cur_decoder == "rnnt"
    m.change_decoding_strategy(decoder_type="ctc")
    assert m.cur_decoder == "ctc" and m.ctc_decoding is not None
    m.change_decoding_strategy(dict(strategy="greedy_batch", greedy=dict(max_symbols=5)), decoder_type="rnnt")
    assert m.cur_decoder == "rnnt" and m.decoding.decoding.max_symbols == 5
    m.change_decoding_strategy(decoder_type="ctc")
    m.change_decoding_strategy(None, None)
    assert m.cur_decoder == "rnnt"
    with pytest.raises(ValueError, match="not supported"):
        m.change_decoding_strategy(decoder_type="aed")
    with pytest.raises(NotImplementedError, match="beam"):
        m.change_decoding_strategy(dict(strategy="beam"), decoder_type="ctc")
    with pytest.raises(NotImplementedError, match="beam"):
        EncDecHybridRNNTCTCModel(_cfg(decoding=dict(strategy="beam")))


def test_stream_decode_symbols_are_exported_and_declared():
    from nemo_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mi355x_asr.h")).read()
    name = "mi355x_transducer_greedy_decode"   # the resumable searches: this entry with state_out in its descriptor
    assert name in _lib.EXPORTED_SYMBOLS
    assert callable(getattr(_lib.lib, name))
    assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert "mi355x_transducer_greedy_desc" in header and "mi355x_rnnt_stream_state" in header
