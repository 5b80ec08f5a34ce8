"""The saved-state records of the encoder sequencers (modules/conformer_encoder.py, squeezeformer_encoder.py): host-only properties
no other test pins."""
import copy

import pytest
import torch

from nemo_amd.modules import conformer_encoder as C
from nemo_amd.modules import squeezeformer_encoder as Q


def _step(cls=C._Step):
    return cls(2, 80, 37, 19, 40, 10, 20, 20, torch.float32, True, 7)


@pytest.mark.parametrize("rec", [_step(), _step(Q._SqStep), C._RowPacking(peek=True), C._SubIO(8, None, None, [])])
def test_records_reject_undeclared_attributes(rec):
    with pytest.raises(AttributeError):
        rec.no_such_field = 1
    assert not hasattr(rec, "__dict__")


def test_step_record_names_the_grid_and_declares_its_defaults():
    S = _step(Q._SqStep)
    assert (S.B, S.F, S.T, S.T1, S.F1, S.T2, S.F2, S.M, S.cdt, S.training, S.seed) == (2, 80, 37, 19, 40, 10, 20, 20, torch.float32, True, 7)
    for name in C._Step.__slots__ + Q._SqStep.__slots__:
        getattr(S, name)    # every declared field reads without a probe
    assert S.pk is None and S.pre_ln is None and S.pre_bwd is None and not S.bypass and not S.arena
    assert S.sd == [] and S.cap_layers == [] and S.geos == []


def test_copy_of_a_step_record_is_shallow_and_gets_a_layer_list_of_its_own():
    S = _step()
    S.mel, S.layers = torch.zeros(3), ["l0", "l1"]
    S2 = copy.copy(S)
    assert type(S2) is C._Step and S2.mel is S.mel and S2.layers is S.layers and S2.T2 == S.T2
    S2.layers = list(S.layers)      # what the live backward over a replayed forward does
    S2.layers[1] = None
    S2.serial = 5
    assert S.layers == ["l0", "l1"] and S.serial == 0


def test_conformer_and_squeezeformer_block_records_are_distinct_types():
    pairs = [(C._FfSaved, Q._SqFfSaved), (C._AttSaved, Q._SqAttSaved), (C._ConvSaved, Q._SqConvSaved), (C._LayerSaved, Q._SqLayerSaved)]
    for a, b in pairs:
        assert a is not b and a._fields != b._fields
    ff = C._FfSaved(*range(8))
    with pytest.raises(AttributeError):
        ff.x = 0     # immutable
    with pytest.raises(TypeError):
        Q._SqFfSaved(*range(8))     # nine fields: a Conformer layout does not fit
    assert C._LnSaved._fields[0] == "x" and C._PreNorm._fields[0] == "y"    # a norm's input and a norm's output are not one slot
    core = C._AttnCore(ctx_lo=1, lse=2)
    assert (core.qu, core.qv, core.s, core.pd) == (None,) * 4 and core.ctx_lo == 1 and core.lse == 2


def test_peek_packing_plan_is_told_apart_from_a_full_one():
    decision, peek = C._RowPacking(peek=True), C._RowPacking(peek=True, Mp=11)
    full = C._RowPacking(peek=False, Mp=11, cu=torch.tensor([0, 5, 11]), host_lens=torch.tensor([5, 6]))
    assert decision.peek and decision.Mp is None and decision.cu is None
    assert peek.peek and peek.cu is None and peek.host_lens is None
    assert not full.peek and full.cu is not None and full.Mp == peek.Mp
