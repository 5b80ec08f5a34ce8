"""CPU-side checks of the greedy transducer search for prediction networks of L LSTM layers (no kernel is launched here):
the restatement tests/rnnt_layers_oracle.py against torch.nn.LSTM and against the one-layer restatement, the C ABI of
mi355x_transducer_greedy_decode_layers (declaration, mirror, refusals before any launch), the decoder objects' constructors and
the layered stream state."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import rnnt_layers_oracle as O
import stream_decode_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("L", [1, 2, 3])
def test_oracle_prediction_step_is_torch_lstm(L):
    """the restatement's step, fed a label sequence, against torch.nn.LSTM(H, H, L) in eval mode stepped over the same embeddings"""
    V, H, J = 20, 32, 16
    Pd, Pj = O.layered_transducer(3, L, V, H, 8, J)
    lstm = torch.nn.LSTM(H, H, L).eval()
    with torch.no_grad():
        for l in range(L):
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                getattr(lstm, f"{n}_l{l}").copy_(Pd[O.Q + f"{n}_l{l}"])
        labels = [V, 3, 7, 7, 0, 19, 11]   # the start-of-sequence blank (zero row), then labels
        h, c = torch.zeros(L, H), torch.zeros(L, H)
        state = (h.unsqueeze(1), c.unsqueeze(1))
        err = 0.0
        for k in labels:
            gp, h, c = O.pred_step(Pd, Pj, k, h, c)
            y, state = lstm(Pd["prediction.embed.weight"][k].view(1, 1, H), state)
            want_gp = torch.nn.functional.linear(y.view(H), Pj["pred.weight"], Pj["pred.bias"])
            err = max(err, float((h - state[0][:, 0]).abs().max()), float((c - state[1][:, 0]).abs().max()),
                      float((gp - want_gp).abs().max()))
    assert err <= 1e-6, err


@pytest.mark.parametrize("max_symbols", [2, 10])
@pytest.mark.parametrize("kind", ["rnnt", "tdt"])
def test_oracle_at_one_layer_is_the_one_layer_oracle(kind, max_symbols):
    V, T = S.SMALL["V"], S.SMALL["T"]
    lens = torch.tensor(S.SMALL["lens"])
    dur = O.DUR if kind == "tdt" else None
    Pd, Pj = S.small_case(kind)
    Pd1, Pj1 = O.small_case(kind, 1)
    assert all(torch.equal(Pd[k], Pd1[k]) for k in Pd) and all(torch.equal(Pj[k], Pj1[k]) for k in Pj) and len(Pd) == len(Pd1)
    enc = S.small_enc()
    cuts = list(range(5, T, 5))
    want, fin_w, ev_w = S.decode_chunked(Pd, Pj, enc, lens, V, max_symbols, cuts, dur)
    got, fin_g, ev_g = O.decode_chunked(Pd1, Pj1, enc, lens, V, max_symbols, cuts, dur)
    assert got == want and ev_g == ev_w and sum(len(g[0]) for g in got) > 20
    for a, b in zip(fin_g, fin_w):
        assert torch.equal(a["h"][0], b["h"]) and torch.equal(a["c"][0], b["c"])
        assert all(a[k] == b[k] for k in ("last", "score", "frames_done", "skip", "zero_run"))
    # and the forced walk along its own hypotheses has margin 0 everywhere
    f_all = torch.nn.functional.linear(enc.transpose(1, 2), Pj["enc.weight"], Pj["enc.bias"])
    rep = O.forced_walk(Pd1, Pj1, f_all, lens, V, max_symbols, got, dur)
    assert all(r[1] == r[2] and r[3] == 0.0 for rows in rep for r in rows)


def test_header_declares_the_layers_entry_and_the_mirror_matches():
    from nemo_amd import _lib
    from nemo_amd._lib import TransducerLstmLayers
    hdr = open(os.path.join(ROOT, "include", "mi355x_asr.h")).read()
    assert re.search(r"typedef struct mi355x_transducer_lstm_layers \{", hdr)
    assert len(re.findall(r"\bmi355x_transducer_greedy_decode_layers\s*\(", hdr)) == 1   # declared once, not named with `(` in prose
    assert "mi355x_transducer_greedy_decode_layers" in _lib.EXPORTED_SYMBOLS
    cname = "mi355x_transducer_lstm_layers"
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mi355x_asr.h"\nint main(){\n'
           + f'  printf("%zu\\n", sizeof({cname}));\n'
           + "".join(f'  printf("%zu\\n", offsetof({cname}, {f[0]}));\n' for f in TransducerLstmLayers._fields_) + "  return 0; }")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(tmp, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = list(map(int, subprocess.check_output([exe]).decode().split()))
    M = TransducerLstmLayers
    assert len(M._fields_) == 7
    assert vals == [ctypes.sizeof(M)] + [getattr(M, f[0]).offset for f in M._fields_]


def _valid_desc(H=32, J=32, V1=49):
    """a descriptor the one-layer entry would launch: dummy non-null pointers, which the host never dereferences; no durations, no
    models, no states -- for refusal cases only"""
    from nemo_amd._lib import TransducerGreedyDesc
    p = 0x1000
    return TransducerGreedyDesc(enc_proj=p, enc_len=p, emb=p, w_ih=p, w_hh=p, w_pred=p, w_out=p, b_ih=p, b_hh=p, b_pred=p, b_out=p,
                                tokens=p, times=p, out_len=p, score=p, ldf=J, ld_ih=H, ld_hh=H, ld_pred=H, ld_out=J, f_dtype=0,
                                w_dtype=0, B=2, T=3, J=J, H=H, V1=V1, blank=V1 - 1, max_symbols=2, max_out=6)


def _upper(n, H=32):
    from nemo_amd._lib import TransducerLstmLayers
    up = TransducerLstmLayers(n_upper=n)
    for l in range(max(0, min(n, 3))):
        up.w_ih[l] = up.w_hh[l] = up.b_ih[l] = up.b_hh[l] = 0x1000
        up.ld_ih[l] = up.ld_hh[l] = H
    return up


def test_layers_entry_refuses_before_any_launch():
    from nemo_amd import _lib
    call = _lib.lib.mi355x_transducer_greedy_decode_layers
    d = _valid_desc()
    assert call(ctypes.byref(d), ctypes.byref(_upper(-1)), None) == 1
    assert call(ctypes.byref(d), ctypes.byref(_upper(4)), None) == 1
    up = _upper(1)
    up.w_hh[0] = None
    assert call(ctypes.byref(d), ctypes.byref(up), None) == 1
    up = _upper(1)
    up.ld_ih[0] = 6
    assert call(ctypes.byref(d), ctypes.byref(up), None) == 1
    # LDS: 4 * (5H + 4LH + 2J + V1 + D + 4) bytes against 160 KiB - 256.  H = 2048, J = 32, V1 = 49: L = 4 needs 172 500 bytes and is
    # refused where L = 3 (139 732 bytes) would not be -- so the refusal below is the layers' share, not the descriptor's
    H = 2048
    need = lambda L: 4 * (5 * H + 4 * L * H + 2 * 32 + 49 + 4)   # noqa: E731
    assert need(3) <= 160 * 1024 - 256 < need(4)
    assert call(ctypes.byref(_valid_desc(H=H)), ctypes.byref(_upper(3, H)), None) == 1
    # what the one-layer entry refuses is refused here too, with and without upper layers
    bad = _valid_desc()
    bad.ld_hh = 6
    assert call(ctypes.byref(bad), None, None) == 1 and call(ctypes.byref(bad), ctypes.byref(_upper(1)), None) == 1
    assert call(None, None, None) == 1


@pytest.mark.parametrize("kind", ["rnnt", "tdt"])
def test_decoder_objects_accept_up_to_four_layers(kind):
    from nemo_amd.modules import GreedyBatchedRNNTInfer, GreedyBatchedTDTInfer, RNNTDecoder, RNNTJoint

    def build(L):
        dec = RNNTDecoder({"pred_hidden": 32, "pred_rnn_layers": L}, 28)
        joint = RNNTJoint(jointnet={"encoder_hidden": 16, "pred_hidden": 32, "joint_hidden": 32, "activation": "relu", "dropout": 0.0},
                          num_classes=28, num_extra_outputs=5 if kind == "tdt" else 0)
        if kind == "tdt":
            return GreedyBatchedTDTInfer(dec, joint, 28, O.DUR, max_symbols_per_step=4)
        return GreedyBatchedRNNTInfer(dec, joint, 28, max_symbols_per_step=4)

    infer = build(2)
    hyps = infer.fresh_hypotheses(3, device="cpu")
    assert all(tuple(h.dec_state.h.shape) == (2, 1, 32) and tuple(h.dec_state.c.shape) == (2, 1, 32) for h in hyps)
    assert tuple(build(1).fresh_hypotheses(2, device="cpu")[0].dec_state.h.shape) == (1, 32)
    build(4)
    with pytest.raises(NotImplementedError, match="4"):
        build(5)


@pytest.mark.parametrize("cls", ["RNNTStreamState", "RNNTFusedStreamState"])
def test_stream_state_with_layers(cls):
    from nemo_amd import ops
    State = getattr(ops, cls)
    B, H = 3, 8
    # one layer: the shapes it has always had, whichever way it is asked for
    for st in (State.fresh(B, H, 5, "cpu"), State.fresh(B, H, 5, "cpu", layers=1), State.empty(B, H, "cpu")):
        assert tuple(st.h.shape) == (B, H) and tuple(st.c.shape) == (B, H) and tuple(st.last.shape) == (B,)
    st = State.fresh(B, H, 5, "cpu")
    assert st.last.tolist() == [5] * B and not st.h.any() and tuple(st.select(1).h.shape) == (1, H)
    assert tuple(State.stack([st.select(b) for b in range(B)]).h.shape) == (B, H)
    # three layers: the batch on dimension 1 of h / c
    st = State.fresh(B, H, 5, "cpu", layers=3)
    assert tuple(st.h.shape) == (3, B, H) and tuple(st.c.shape) == (3, B, H) and tuple(State.empty(B, H, "cpu", layers=3).h.shape) == (3, B, H)
    st.h.copy_(torch.arange(3 * B * H, dtype=torch.float32).view(3, B, H))
    st.c.copy_(-st.h)
    st.score.copy_(torch.tensor([1.0, 2.0, 3.0]))
    one = st.select(2)
    assert type(one) is State and tuple(one.h.shape) == (3, 1, H) and one.h.is_contiguous() and torch.equal(one.h[:, 0], st.h[:, 2])
    assert float(one.score) == 3.0 and tuple(one.last.shape) == (1,)
    back = State.stack([st.select(b) for b in range(B)])
    for a, b in zip(back.tensors(), st.tensors()):
        assert torch.equal(a, b) and a.is_contiguous()
    # _c checks the shapes for the given layer count (and then refuses host tensors, like every wrapper)
    with pytest.raises(ValueError, match="stream state `h`"):
        st._c(B, H)
    with pytest.raises(ValueError, match="stream state `h`"):
        st._c(B, H, layers=2)
    with pytest.raises(RuntimeError, match="MI355X"):
        st._c(B, H, layers=3)
