"""Token-and-Duration Transducer (TDT) without a GPU: the float64 oracle of tests/tdt_oracle.py against brute-force path
enumeration differentiated by autograd (what makes the objective and its closed-form gradient trustworthy), the joint's
reference state-dict shapes with duration outputs, the FastConformer-TDT config and its .nemo round trip, and the argument
checks of the Python classes and of the C ABI (no kernel is launched)."""
import ctypes
import sys
import os

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tdt_oracle as O  # noqa: E402


def _case(T, U, durations, V1=5, seed=0, pad=(0, 0)):
    rng = np.random.default_rng(seed)
    z = rng.normal(size=(T + pad[0], U + 1 + pad[1], V1 + len(durations))) * 1.5
    labels = rng.integers(0, V1 - 1, size=U).tolist()
    return z, labels


@pytest.mark.parametrize("durations", [[0, 1, 2], [0, 1, 2, 3, 4], [0, 2, 3]])
@pytest.mark.parametrize("T,U", [(1, 0), (3, 0), (4, 1), (5, 2), (6, 3), (2, 3)])
@pytest.mark.parametrize("sigma", [0.0, 0.05])
def test_oracle_equals_brute_force_enumeration(durations, T, U, sigma):
    blank = 4
    z, labels = _case(T, U, durations, seed=T * 10 + U)
    alpha, beta, ll_f, ll_b, _, _ = O.lattice(z, labels, T, U, durations, blank, sigma)
    assert np.isclose(ll_f, ll_b, rtol=1e-12, atol=1e-12), (ll_f, ll_b)
    cost, g = O.grad_closed_form(z, labels, T, U, durations, blank, sigma)
    if not O.enumerate_paths(T, U, durations):   # no path (e.g. T = 1 with durations [0, 2, 3]): infinite cost
        assert cost == np.inf
        return
    bc, bg = O.brute_force(z, labels, T, U, durations, blank, sigma)
    assert np.isclose(cost, bc, rtol=1e-12, atol=1e-12), (cost, bc)
    assert np.allclose(g, bg, rtol=1e-9, atol=1e-12), np.abs(g - bg).max()


def test_oracle_batch_is_ragged_and_zero_beyond_the_lengths():
    durations, blank = [0, 1, 2], 4
    rng = np.random.default_rng(3)
    acts = torch.from_numpy(rng.normal(size=(3, 5, 4, 5 + 3)))
    labels = torch.tensor([[0, 1, 2], [3, 0, 0], [1, 1, 0]])
    lens, ll = torch.tensor([5, 3, 4]), torch.tensor([3, 1, 0])
    c, g = O.tdt_loss_and_grad(acts, labels, lens, ll, durations, blank, 0.02, "none")
    for b in range(3):
        T, U = int(lens[b]), int(ll[b])
        bc, bg = O.brute_force(acts[b].numpy(), labels[b].tolist(), T, U, durations, blank, 0.02)
        assert np.isclose(c[b].item(), bc) and np.allclose(g[b, :T, :U + 1].numpy(), bg)
        assert float(g[b, T:].abs().sum()) == 0.0 and float(g[b, :, U + 1:].abs().sum()) == 0.0
    cm, gm = O.tdt_loss_and_grad(acts, labels, lens, ll, durations, blank, 0.02, "mean")
    assert np.isclose(cm.item(), c.mean().item()) and torch.allclose(gm, g / 3)


def test_greedy_restatement_follows_durations():
    """the Python restatement of the search: frames advance by the predicted duration, blank by at least one frame, and a run
    of duration-0 labels is cut at max_symbols"""
    H, J, V, durations = 4, 4, 3, [0, 1, 2]
    Pd = {"prediction.embed.weight": torch.zeros(V + 1, H),
          "prediction.dec_rnn.lstm.weight_ih_l0": torch.zeros(4 * H, H), "prediction.dec_rnn.lstm.weight_hh_l0": torch.zeros(4 * H, H),
          "prediction.dec_rnn.lstm.bias_ih_l0": torch.zeros(4 * H), "prediction.dec_rnn.lstm.bias_hh_l0": torch.zeros(4 * H)}
    out_b = torch.tensor([0.0, 5.0, 0.0, 1.0, 9.0, 0.0, 0.0])   # label 1 always, duration 0 always
    Pj = {"enc.weight": torch.zeros(J, 2), "enc.bias": torch.zeros(J), "pred.weight": torch.zeros(J, H), "pred.bias": torch.zeros(J),
          "joint_net.2.weight": torch.zeros(V + 1 + 3, J), "joint_net.2.bias": out_b}
    enc = torch.zeros(1, 2, 3)
    hyps = O.tdt_greedy_decode(Pd, Pj, enc, torch.tensor([3]), V, durations, max_symbols=2)
    assert hyps[0] == ([1] * 6, [0, 0, 1, 1, 2, 2])
    Pj["joint_net.2.bias"] = torch.tensor([0.0, 0.0, 0.0, 9.0, 9.0, 0.0, 0.0])   # blank with duration 0 -> one frame
    assert O.tdt_greedy_decode(Pd, Pj, enc, torch.tensor([3]), V, durations, max_symbols=2)[0] == ([], [])


def test_joint_with_duration_outputs_has_the_reference_state_dict():
    from nemo_amd.modules import RNNTJoint
    j = RNNTJoint(jointnet={"encoder_hidden": 32, "pred_hidden": 16, "joint_hidden": 24, "activation": "relu", "dropout": 0.2},
                  num_classes=10, num_extra_outputs=5)
    assert {k: tuple(v.shape) for k, v in j.state_dict().items()} == {
        "pred.weight": (24, 16), "pred.bias": (24,), "enc.weight": (24, 32), "enc.bias": (24,),
        "joint_net.2.weight": (16, 24), "joint_net.2.bias": (16,)}
    assert j.num_classes_with_blank == 16
    j0 = RNNTJoint(jointnet={"encoder_hidden": 32, "pred_hidden": 16, "joint_hidden": 24, "activation": "relu"}, num_classes=10)
    assert j0.num_classes_with_blank == 11 and tuple(j0.joint_net[-1].weight.shape) == (11, 24)


def test_fastconformer_tdt_config_builds_and_round_trips(tmp_path):
    from nemo_amd.models import EncDecRNNTModel, fastconformer_tdt_config
    from nemo_amd.modules import GreedyBatchedTDTInfer, TDTLoss
    cfg = fastconformer_tdt_config("small", vocab_size=30, d_model=64, n_heads=4, n_layers=1, subsampling_conv_channels=32)
    cfg["decoder"]["prednet"].update(pred_hidden=64)
    cfg["joint"]["jointnet"].update(joint_hidden=64)
    cfg["labels"] = [chr(ord("a") + i) for i in range(26)] + [" ", "'", ".", "-"]
    m = EncDecRNNTModel(cfg)
    assert isinstance(m.loss, TDTLoss) and m.loss.durations == [0, 1, 2, 3, 4]
    assert m.loss.sigma == 0.02 and m.loss.omega == 0.1 and m.loss.blank == 30
    assert m.joint.num_classes_with_blank == 36 and tuple(m.joint.joint_net[-1].weight.shape) == (36, 64)
    assert m.joint.loss is m.loss
    assert isinstance(m.decoding.decoding, GreedyBatchedTDTInfer) and m.decoding.decoding.durations == [0, 1, 2, 3, 4]
    path = str(tmp_path / "tdt.nemo")
    m.save_to(path)
    r = EncDecRNNTModel.restore_from(path)
    assert isinstance(r.loss, TDTLoss) and r.loss.durations == [0, 1, 2, 3, 4]
    sd0, sd1 = m.state_dict(), r.state_dict()
    assert sd0.keys() == sd1.keys() and all(torch.equal(sd0[k], sd1[k]) for k in sd0)


def test_tdt_options_are_refused_by_name():
    from nemo_amd.modules import TDTLoss, TDTLossNumba
    assert TDTLossNumba is TDTLoss
    for bad in ([1, 2], [0], [0, 0, 1], [0, 2, 1], [0, 1, 9], list(range(9)), [0, 1.5], []):
        with pytest.raises(ValueError):
            TDTLoss(blank=4, durations=bad)
    with pytest.raises(NotImplementedError, match="fastemit_lambda"):
        TDTLoss(blank=4, durations=[0, 1, 2], fastemit_lambda=0.001)
    with pytest.raises(NotImplementedError, match="clamp"):
        TDTLoss(blank=4, durations=[0, 1, 2], clamp=0.5)
    TDTLoss(blank=4, durations=[0, 1, 2], fastemit_lambda=0.0, clamp=-1)
    from nemo_amd.models import EncDecRNNTModel, fastconformer_tdt_config
    cfg = fastconformer_tdt_config("small", vocab_size=8, d_model=32, n_heads=4, n_layers=1, subsampling_conv_channels=16)
    cfg["loss"]["tdt_kwargs"]["fastemit_lambda"] = 0.01
    with pytest.raises(NotImplementedError, match="fastemit_lambda"):
        EncDecRNNTModel(cfg)
    cfg["loss"]["tdt_kwargs"].update(fastemit_lambda=0.0, durations=[1, 2])
    with pytest.raises(ValueError):
        EncDecRNNTModel(cfg)


def test_omega_draw_is_exact_at_the_ends():
    from nemo_amd.modules.tdt_loss import draw_rnnt_call
    torch.manual_seed(0)
    s0 = torch.get_rng_state()
    assert not any(draw_rnnt_call(0.0) for _ in range(50)) and all(draw_rnnt_call(1.0) for _ in range(50))
    assert torch.equal(torch.get_rng_state(), s0)   # the two ends draw nothing
    draws = [draw_rnnt_call(0.3) for _ in range(2000)]
    assert 0.25 < sum(draws) / len(draws) < 0.35


def test_tdt_abi_rejects_bad_arguments_without_a_gpu():
    from nemo_amd import _lib
    lib = _lib.lib
    n = ctypes.c_longlong(0)
    assert lib.mi355x_tdt_workspace_elems(2, 3, 4, 5, ctypes.byref(n)) == 0 and n.value == (4 + 10) * 24 + 4
    assert lib.mi355x_tdt_workspace_elems(2, 3, 4, 9, ctypes.byref(n)) == 1
    dur = lambda *d: (ctypes.c_int * len(d))(*d)
    fake = ctypes.c_void_p(16)   # never dereferenced: every call below fails its argument checks first
    args = lambda durs, D, V1=8, ld=13, U1=3: (fake, ld, fake, fake, fake, 2, 4, U1, V1, D, durs, 7, 0.0, 1.0, fake, None, 0, 0,
                                               fake, 1 << 20, None)
    for d, D in ((dur(1, 2, 3), 3), (dur(0, 2, 1), 3), (dur(0, 1, 9), 3), (dur(0, 0), 2), (dur(0), 1), (None, 3)):
        assert lib.mi355x_tdt_loss_ex(*args(d, D)) == 1
    assert lib.mi355x_tdt_loss_ex(*args(dur(0, 1, 2), 3, ld=10)) == 1         # row pitch < V1 + D
    assert lib.mi355x_tdt_loss_ex(*args(dur(0, 1, 2), 3, U1=1025)) == 1       # U1 > 1024
    a = list(args(dur(0, 1, 2), 3)); a[12] = -0.5                              # sigma < 0
    assert lib.mi355x_tdt_loss_ex(*a) == 1
    a = list(args(dur(0, 1, 2), 3)); a[19] = 10                                # workspace too small
    assert lib.mi355x_tdt_loss_ex(*a) == 1
    a = list(args(dur(0, 1, 2), 3)); a[15] = fake; a[16] = 1; a[17] = 13       # bf16 gradient pitch not a multiple of 8
    assert lib.mi355x_tdt_loss_ex(*a) == 1
    a = list(args(dur(0, 1, 2), 3)); a[15] = fake; a[16] = 0; a[17] = 10       # gradient pitch < V1 + D
    assert lib.mi355x_tdt_loss_ex(*a) == 1

    def greedy(durs=dur(0, 1, 2), **kw):   # the TDT search through the descriptor entry; valid but for what a case overrides
        d = _lib.TransducerGreedyDesc(
            enc_proj=16, f_dtype=0, ldf=16, enc_len=16, emb=16, w_ih=16, ld_ih=16, w_hh=16, ld_hh=16, b_ih=16, b_hh=16, w_pred=16,
            ld_pred=16, b_pred=16, w_out=16, ld_out=16, b_out=16, w_dtype=0, B=2, T=4, J=16, H=16, V1=9, D=len(durs),
            durations=ctypes.addressof(durs), blank=8, max_symbols=10, tokens=16, times=16, out_len=16, score=16, max_out=40)
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.mi355x_transducer_greedy_decode(ctypes.byref(d), None)
    assert greedy(dur(1, 2, 3)) == 1                                           # durations not starting at 0
    assert greedy(dur(*range(9))) == 1                                         # nine durations
    assert greedy(blank=9) == 1                                                # blank outside the V1 label logits


def test_rnnt_abi_rejects_the_same_bad_arguments_without_a_gpu():
    """mi355x_rnnt_loss_ex goes through the argument checks it shares with mi355x_tdt_loss_ex: every kind of bad call refused
    there is refused here (one valid call with one argument spoiled at a time; nothing is launched)"""
    from nemo_amd import _lib
    lib = _lib.lib
    B, T, U1, V1 = 2, 4, 3, 8
    n = ctypes.c_longlong(0)
    assert lib.mi355x_rnnt_workspace_elems(B, T, U1, ctypes.byref(n)) == 0 and n.value == 5 * B * T * U1 + 2 * B
    fake = ctypes.c_void_p(16)   # aligned, never dereferenced: every call below fails its argument checks first
    names = ("acts", "ld", "labels", "act_lens", "label_lens", "B", "T", "U1", "V1", "blank", "fastemit", "clamp", "scale", "costs",
             "grads", "gdt", "ldg", "ws", "ws_elems", "stream")
    good = dict(zip(names, (fake, V1, fake, fake, fake, B, T, U1, V1, V1 - 1, 0.0, 0.0, 1.0, fake, fake, 0, V1, fake, n.value, None)))
    bad = {"row pitch < V1": dict(ld=V1 - 1),
           "gradient pitch < V1": dict(ldg=V1 - 1),
           "U1 > 1024": dict(U1=1025, ws_elems=1 << 30),
           "bf16 gradient pitch not a multiple of 8": dict(gdt=1, ldg=V1 + 4),
           "bf16 gradient pointer not 16-byte aligned": dict(gdt=1, grads=ctypes.c_void_p(24)),
           "workspace one element short": dict(ws_elems=n.value - 1),
           "clamp < 0": dict(clamp=-0.5),
           "fastemit_lambda < 0": dict(fastemit=-0.5),
           "blank >= V1": dict(blank=V1),
           "unknown gradient dtype": dict(gdt=2)}
    for why, change in bad.items():
        assert lib.mi355x_rnnt_loss_ex(*{**good, **change}.values()) == 1, why
