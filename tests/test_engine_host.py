"""CPU-side pins of nemo_amd/modules/engine.py (run without a GPU).

A. The weight images every module family declares -- offsets, shapes and pack entries of `_build_plan(cdt, "cpu")` -- against
   tests/golden/engine_plans.json.  The fixture was recorded by `python tests/test_engine_host.py` from the commit BEFORE the four
   hand-copied plan caches were folded into EngineModule (the recorder only needs `flat_parameters()` and `_plan`, so it runs on both
   sides of that change); it changes only when a module's image layout is meant to change.
B. The plan cache: when the pack runs, when a plan is rebuilt.
C. The split-K chooser against the three expressions it replaced, written out here as they stood.
"""
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nemo_amd.packing import PackPlan

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_plans.json")
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


# ---------------------------------------------------------------------------------------------------- the cases
def _conformer_striding():
    from nemo_amd.modules.conformer_encoder import ConformerEncoder
    return ConformerEncoder(80, 2, 64, n_heads=4, subsampling_conv_channels=64)  # un-padded heads, conv2 + its four dgrad parity images


def _conformer_dw(pad_heads):
    from nemo_amd.modules.conformer_encoder import ConformerEncoder
    m = ConformerEncoder(80, 2, 176, n_heads=4, subsampling="dw_striding", subsampling_factor=8, subsampling_conv_channels=64)
    m.flash_pad_heads = pad_heads  # bf16 heads 44 -> 64 (the default) or 44 -> 48
    return m


def _conformer_ffn():
    from nemo_amd.modules.conformer_encoder import ConformerEncoder
    m = ConformerEncoder(80, 1, 512, n_heads=8, ff_expansion_factor=1)
    m.ffn_fused = True  # add_ffn
    return m


def _squeezeformer(channels, time_reduce_idx):
    from nemo_amd.modules.squeezeformer_encoder import SqueezeformerEncoder
    return SqueezeformerEncoder(80, 4, 84, n_heads=4, subsampling_conv_channels=channels, time_reduce_idx=time_reduce_idx)


def _ctc_decoder():
    from nemo_amd.modules.conv_asr import ConvASRDecoder
    return ConvASRDecoder(64, 29)


def _rnnt_decoder():
    from nemo_amd.modules.rnnt import RNNTDecoder
    return RNNTDecoder({"pred_hidden": 32, "pred_rnn_layers": 2}, 28)


def _rnnt_joint():
    from nemo_amd.modules.rnnt import RNNTJoint
    return RNNTJoint({"joint_hidden": 32, "encoder_hidden": 64, "pred_hidden": 32}, 28, num_extra_outputs=5)


# name -> (builder, dtypes)
CASES = {
    "conformer_striding": (_conformer_striding, ("fp32", "bf16")),
    "conformer_dw_pad64": (lambda: _conformer_dw(True), ("fp32", "bf16")),
    "conformer_dw_pad48": (lambda: _conformer_dw(False), ("fp32", "bf16")),
    "conformer_ffn_fused": (_conformer_ffn, ("bf16",)),
    "squeezeformer_padded_channels": (lambda: _squeezeformer(20, 1), ("fp32", "bf16")),  # + padded d, tr.* / rec.*
    "squeezeformer_dense_channels": (lambda: _squeezeformer(24, None), ("fp32", "bf16")),
    "ctc_decoder": (_ctc_decoder, ("fp32", "bf16")),
    "rnnt_decoder": (_rnnt_decoder, ("fp32", "bf16")),
    "rnnt_joint": (_rnnt_joint, ("fp32", "bf16")),
}
PARAMS = [(name, dt) for name, (_, dts) in CASES.items() for dt in dts]


def describe(plans, flat):
    """per plan: the ordered image table name -> (offset, rows, pitch) and the sorted pack entries, every source tensor as its
    element offset inside the module's flat parameter buffer"""
    plans = plans if isinstance(plans, (tuple, list)) else (plans,)
    off = lambda t: (t.data_ptr() - flat.data_ptr()) // 4
    return [{"images": [[n, *v] for n, v in p._images.items()],
             "entries": sorted([e[0], off(e[1])] + list(e[2:]) for e in p._pending),
             "ffn": sorted([f[0], off(f[1]), off(f[2]), f[3]] for f in p._ffn)} for p in plans if p is not None]


def record():
    """what `_plan` declares on this checkout, with the pack itself replaced by a no-op"""
    run, PackPlan.run = PackPlan.run, lambda self: None
    try:
        out = {}
        for name, dt in PARAMS:
            m = CASES[name][0]()
            flat = m.flat_parameters().flat
            out[f"{name}/{dt}"] = describe(m._plan(DTYPES[dt], "cpu"), flat)
        return out
    finally:
        PackPlan.run = run


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture
def runs(monkeypatch):
    """PackPlan.run replaced by a counter"""
    n = []
    monkeypatch.setattr(PackPlan, "run", lambda self: n.append(self))
    return n


# ---------------------------------------------------------------------------------------------------- A. declared images
@pytest.mark.parametrize("name,dt", PARAMS)
def test_declared_images_match_the_recorded_plans(name, dt, golden, runs):
    m = CASES[name][0]()
    flat = m.flat_parameters().flat
    got = json.loads(json.dumps(describe(m._build_plan(DTYPES[dt], "cpu"), flat)))
    want = golden[f"{name}/{dt}"]
    assert not runs   # building a plan launches nothing
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g["images"] == w["images"]      # an ordered list: names, offsets, rows, pitches, and the order of declaration
        assert g["entries"] == w["entries"]    # sorted on both sides: the order of add_block calls only permutes the pack table
        assert g["ffn"] == w["ffn"]


def test_fixture_covers_every_declaration_branch(golden):
    assert set(golden) == {f"{n}/{dt}" for n, dt in PARAMS}
    names = lambda key: [im[0] for plan in golden[key] for im in plan["images"]]
    pitch = lambda key, image: next(im[3] for plan in golden[key] for im in plan["images"] if im[0] == image)
    assert {"pre.w2", "pre.w2t", "pre.w2d00", "pre.w2d01", "pre.w2d10", "pre.w2d11"} <= set(names("conformer_striding/bf16"))
    assert "L0.att.bu" not in names("conformer_striding/fp32")              # un-padded heads: add_concat / add_matrix
    assert pitch("conformer_striding/bf16", "L0.att.wo") == 4 * 64          # ... in bf16 d_k = 16 rides the fused kernels' 64
    assert pitch("conformer_dw_pad64/bf16", "L0.att.wo") == 4 * 64 and pitch("conformer_dw_pad48/bf16", "L0.att.wo") == 4 * 48
    assert "L0.att.bu" not in names("conformer_dw_pad64/fp32")              # fp32 keeps d_k = 44
    assert golden["conformer_ffn_fused/bf16"][0]["ffn"] and "L0.ff1.w1p" in names("conformer_ffn_fused/bf16")
    assert "pre.c0w" in names("squeezeformer_padded_channels/bf16") and "pre.c0w" not in names("squeezeformer_dense_channels/bf16")
    assert {"tr.pw", "tr.pwt", "rec.w", "rec.wt"} <= set(names("squeezeformer_padded_channels/fp32"))
    assert "tr.pw" not in names("squeezeformer_dense_channels/fp32")
    assert names("ctc_decoder/bf16") == ["dec.w", "dec.wt"]
    assert names("rnnt_decoder/fp32")[:4] == ["l0.wih", "l0.wiht", "l0.whh", "l0.whht"]
    assert names("rnnt_joint/fp32") == ["enc.w", "enc.wt", "pred.w", "pred.wt", "out.w", "out.wt"]


# ---------------------------------------------------------------------------------------------------- B. the plan cache
@pytest.mark.parametrize("name", ["conformer_striding", "squeezeformer_dense_channels", "ctc_decoder", "rnnt_decoder", "rnnt_joint"])
def test_plan_cache_packs_only_when_the_weights_moved(name, runs):
    m = CASES[name][0]()
    m.flat_parameters()
    W, Wf = m._plan(torch.float32, "cpu")
    per_pack = 1 if Wf is None else 2      # one PackPlan.run per plan
    assert (Wf is None) == (name in ("ctc_decoder", "rnnt_decoder", "rnnt_joint"))
    assert len(runs) == per_pack
    assert m._plan(torch.float32, "cpu")[0] is W and len(runs) == per_pack          # nothing changed: no pack
    m.weights_updated()
    assert m._plan(torch.float32, "cpu")[0] is W and len(runs) == 2 * per_pack      # ... one pack
    assert m._plan(torch.float32, "cpu")[0] is W and len(runs) == 2 * per_pack
    m._force_pack = True
    for k in (3, 4):
        assert m._plan(torch.float32, "cpu")[0] is W and len(runs) == k * per_pack  # every call packs
    m._force_pack = False
    assert m._plan(torch.float32, "cpu")[0] is W and len(runs) == 4 * per_pack
    m.load_state_dict(m.state_dict())
    assert m._plan(torch.float32, "cpu")[0] is W and len(runs) == 5 * per_pack


@pytest.mark.parametrize("name", ["conformer_striding", "ctc_decoder", "rnnt_joint"])
def test_rebuilt_flat_buffer_builds_a_new_plan_and_drops_the_old_one(name, runs):
    m = CASES[name][0]()
    fp = m.flat_parameters()
    W = m._plan(torch.float32, "cpu")[0]
    old_key, = m._plans
    gen = fp.generation
    fp.build()
    assert fp.generation == gen + 1
    W2 = m._plan(torch.float32, "cpu")[0]
    new_key, = m._plans            # one key: the images of the old storage are gone
    assert W2 is not W and new_key != old_key
    assert W2.source_ptrs() != W.source_ptrs()
    n = len(runs)
    assert m._plan(torch.bfloat16, "cpu")[0].dtype == torch.bfloat16 and len(m._plans) == 1 and len(runs) > n   # another dtype: likewise


def test_encoder_plan_key_follows_the_head_geometry(runs):
    m = _conformer_dw(True)
    m.flat_parameters()
    k64 = m._plan_key(torch.bfloat16, "cpu")
    assert k64 == (torch.bfloat16, "cpu", m._flatp.generation, m._geometry(torch.bfloat16)) and k64[3] == (176, 64, 256)
    W = m._plan(torch.bfloat16, "cpu")[0]
    m.flash_pad_heads = False
    k48 = m._plan_key(torch.bfloat16, "cpu")
    assert k48 != k64 and k48[3] == (176, 48, 192)
    W2 = m._plan(torch.bfloat16, "cpu")[0]
    assert W2 is not W and W2.pitch("L0.att.wo") == 192 and W.pitch("L0.att.wo") == 256
    assert m._plan_key(torch.float32, "cpu")[3] == (176, 44, 176)      # fp32 does not pad: the flag is not in its geometry


def test_transducer_cdt_keeps_its_divisibility_check():
    from nemo_amd.modules.rnnt import RNNTJoint
    j = RNNTJoint({"joint_hidden": 36, "encoder_hidden": 64, "pred_hidden": 32}, 28, compute_dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="bf16 compute needs hidden sizes divisible by 8; use compute_dtype=torch.float32"):
        j._cdt()
    j.compute_dtype = torch.float32
    assert j._cdt() == torch.float32
    assert _ctc_decoder()._cdt() == torch.float32 and _conformer_striding()._cdt() == torch.float32


# ---------------------------------------------------------------------------------------------------- C. split-K factors
ROWS = list(range(1, 3000, 7)) + [8032, 16032, 65536, 320640, 1000000]


def _encoder_strided(tiles, K):      # ConformerEncoder._splitk(tiles, K, strided_c=True) as it stood
    nk = (K + 63) // 64
    return max(1, min(nk // 4 if nk >= 8 else 1, 256 // max(tiles, 1), 16))


def _transducer(tiles, rows):        # inside rnnt._ModuleBase._wgrad as it stood
    nk = (rows + 63) // 64
    return max(1, min(max(1, nk // 4), max(1, 256 // tiles), 16))


def _ctc_decoder_rule(tiles, M):     # inside ConvASRDecoder._backward_impl as it stood
    nk = (M + 63) // 64
    return max(1, min(max(1, nk // 4), 256 // tiles))


def test_splitk_chooser_equals_the_three_rules_it_replaced():
    from nemo_amd.modules.conformer_encoder import ConformerEncoder
    from nemo_amd.modules.engine import splitk
    assert len(ROWS) * 699 == 303366
    differ = 0
    for tiles in range(1, 700):
        for rows in ROWS:
            capped, uncapped = splitk(tiles, rows, strided_c=True), splitk(tiles, rows, strided_c=True, cap=None)
            assert capped == _encoder_strided(tiles, rows) == _transducer(tiles, rows), (tiles, rows)
            assert uncapped == _ctc_decoder_rule(tiles, rows), (tiles, rows)
            assert ConformerEncoder._splitk(tiles, rows, strided_c=True) == capped
            if capped != uncapped:
                differ += 1
                assert tiles < 16
    assert differ == 75


def test_ctc_decoder_rule_is_not_the_capped_one():
    from nemo_amd.modules.engine import splitk
    assert splitk(1, 8032, strided_c=True, cap=None) == 31 and splitk(1, 8032, strided_c=True) == 16


def test_tile_count_and_chooser_have_one_home():
    from nemo_amd.modules import engine
    from nemo_amd.modules.conformer_encoder import ConformerEncoder
    assert ConformerEncoder._tiles(1025, 640, True) == engine.tiles(1025, 640, True) == 5 * 5
    assert ConformerEncoder._tiles(1025, 640, False) == engine.tiles(1025, 640, False) == 17 * 10
    for tiles, K in [(184, 16032), (32, 16032), (72, 320640), (8, 16032), (2, 320640), (300, 16032), (1, 64 * 40)]:
        assert ConformerEncoder._splitk(tiles, K) == engine.splitk(tiles, K)


if __name__ == "__main__":
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    rec = record()
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    for k, v in rec.items():
        print(k, [len(p["images"]) for p in v], [len(p["entries"]) for p in v])
