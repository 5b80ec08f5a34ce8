"""CPU: the adapter interface of ConformerEncoder and the models (modules/adapter.py) -- refusals by name, the reference's state-dict
layout, FlatParams rebuild, enabled-adapter bookkeeping.  No kernel is launched."""
import pytest
import torch

CFG = dict(in_features=32, dim=8, activation="swish", norm_position="pre", dropout=0.0)


def _enc(cls="ConformerEncoder"):
    from nemo_amd import modules
    kw = dict(feat_in=80, n_layers=2, d_model=32, n_heads=4, subsampling_conv_channels=16)
    return getattr(modules, cls)(**kw)


@pytest.mark.parametrize("over,name", [
    (dict(norm_position="post"), "norm_position: post"), (dict(dropout=0.1), "dropout > 0"), (dict(activation="relu"), "activation"),
    (dict(adapter_strategy=dict(stochastic_depth=0.1)), "stochastic_depth > 0"), (dict(adapter_strategy=dict(l2_lambda=0.1)), "l2_lambda > 0"),
    (dict(dim=12), "dim=12"), (dict(dim=136), "dim=136")])
def test_config_refusals_name_the_option(over, name):
    with pytest.raises(NotImplementedError, match=name):
        _enc().add_adapter("a", dict(CFG, **over))


def test_refusals_by_place():
    from nemo_amd.modules import adapter
    with pytest.raises(NotImplementedError, match="SqueezeformerEncoder"):
        _enc("SqueezeformerEncoder").add_adapter("a", dict(CFG))
    for name in ("decoder:a", "joint:a"):
        with pytest.raises(NotImplementedError, match=name):
            _enc().add_adapter(name, dict(CFG))
    with pytest.raises(NotImplementedError, match="kernel's limit"):
        adapter.read_config(dict(CFG, in_features=1032), 1032)
    enc = _enc()
    enc.add_adapter("a", dict(CFG))
    with pytest.raises(NotImplementedError, match="cache_aware_stream_step with an adapter enabled"):
        enc.cache_aware_stream_step(torch.zeros(1, 80, 16))
    ch, tm, n = torch.zeros(2, 1, 4, 32), torch.zeros(2, 1, 32, 30), torch.zeros(1, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="cache_aware_stream_step with an adapter enabled"):   # the encoder's own cache path
        enc(audio_signal=torch.zeros(1, 80, 16), length=torch.tensor([16]), cache_last_channel=ch, cache_last_time=tm,
            cache_last_channel_len=n)


def test_layout_generation_and_enabled_bookkeeping():
    enc = _enc()
    keys = set(enc.state_dict())
    assert not enc.is_adapter_available()
    gen = enc.flat_parameters().generation
    enc.add_adapter("encoder:a", dict(CFG))
    enc.add_adapter("b", dict(CFG, dim=16))
    assert enc.flat_parameters().generation > gen and enc.flat_parameters().is_valid()
    new = {k: tuple(v.shape) for k, v in enc.state_dict().items() if k not in keys}
    want = {"module.0.weight": (32,), "module.0.bias": (32,), "module.1.weight": (8, 32), "module.3.weight": (32, 8)}
    assert {k: s for k, s in new.items() if ".adapter_layer.a." in k} == {f"layers.{i}.adapter_layer.a.{k}": s for i in range(2) for k, s in want.items()}
    assert not enc.layers[0].adapter_layer["a"].module[3].weight.any()
    assert enc.is_adapter_available() and enc.get_enabled_adapters() == ["a", "b"]
    enc.set_enabled_adapters("a", False)
    assert enc.get_enabled_adapters() == ["b"]
    enc.set_enabled_adapters(enabled=False)
    assert enc.get_enabled_adapters() == []
    enc.set_enabled_adapters("encoder:a", True)
    assert enc.get_enabled_adapters() == ["a"]
    assert set(_enc().state_dict()) == keys
