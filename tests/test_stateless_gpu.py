"""-m gpu: the stateless prediction network (csrc/stateless.hip) against the float64 restatement of its rule (tests/
stateless_oracle.py).  Values are within max(8 x |float32 restatement - float64 restatement|, 16 ulp) of the float64 restatement, the
margin of tests/test_rnnt_beam_gpu.py::test_beam_search_matches_the_oracle (for a tensor: the largest errors over the tensor, since the
device's summation order is not numpy's).  Tokens, frames and lengths are equal: every search case ASSERTS from the oracle alone a
smallest top-two logit gap >= 1e-3; its seed is the first of 0, 1, 2, ... that passes (picked on the CPU), no case is skipped.  What
feeds the bf16-rounded operand relu(enc_proj + gp) lies on a dyadic grid: it is exact in float32 and float64 and rounds alike."""
import functools

import numpy as np
import pytest
import torch

import stateless_oracle as O

pytestmark = pytest.mark.gpu
CE = {1: 32, 2: 32, 3: 40}   # context size -> pred_hidden; (3, 40): slices 28 / 6 / 6
B, U, V1, J, T, DUR = 3, 7, 13, 24, 9, [0, 1, 2]
LENS = [9, 0, 5, 9, 1, 7, 3, 9, 2, 8, 4, 6, 9, 0, 5, 7, 9]   # 17 streams: two workgroups, the second with one live row
DT = {False: torch.float32, True: torch.bfloat16}


def _dev(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)


def _tol(r32, r64):
    return max(8 * float(np.max(np.abs(np.asarray(r32, np.float64) - r64))), 16 * float(np.spacing(np.float32(np.max(np.abs(r64))))))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [1, 2, 3])
def test_forward_gradient_and_tables_against_float64(C, bf16):
    """tables with a zero blank row; targets [3, 7]: row 0 repeats one token, row 1 is padded with blanks, id 3 never occurs"""
    from nemo_amd import ops
    rng = np.random.default_rng(C)
    embs = [rng.standard_normal((V1, e)).astype(np.float32) for e in O.widths(CE[C], C)]
    for e in embs:
        e[V1 - 1] = 0
    tg = rng.integers(0, V1 - 1, (B, U))
    tg[tg == 3], tg[0], tg[1, 4:] = 4, 5, V1 - 1
    dg = O.bf16_round(rng.standard_normal((B, U + 1, CE[C])))
    w = (O.bf16_round if bf16 else np.asarray)(rng.standard_normal((J, CE[C])).astype(np.float32) * CE[C] ** -0.5)
    d_embs, d_tg = [_dev(e) for e in embs], _dev(tg, torch.int64)
    g = ops.stateless_pred_fwd(d_tg, d_embs, V1 - 1, out_dtype=DT[bf16]).float().cpu().numpy()
    want = O.forward(embs, tg, V1 - 1).astype(np.float32)
    assert np.array_equal(g, O.bf16_round(want) if bf16 else want)   # a copy (bf16: rounded)
    runs = []
    for _ in range(2):
        grads = [torch.full(e.shape, 7.0, device="cuda") for e in embs]   # every row is written: no memset
        ops.stateless_embed_bwd(d_tg, _dev(dg, DT[bf16]), grads, V1 - 1)
        runs.append([x.cpu().numpy() for x in grads])
    g64, g32 = (O.embed_grad(embs, tg, dg, V1 - 1, dt) for dt in (np.float64, np.float32))
    for a, again, r32, r64 in zip(runs[0], runs[1], g32, g64):
        assert np.array_equal(a, again)                                   # two runs: the same bits
        assert not a[3].any() and not a[V1 - 1].any() and r64[5].any()    # unused row and padding row: exactly 0
        assert np.max(np.abs(a - r64)) <= _tol(r32, r64)
    got = ops.stateless_tables(d_embs, _dev(w, DT[bf16]), CE[C], V1 - 1).cpu().numpy()   # J = 24: no multiple of the bf16 K block
    r64, r32 = (O.tables(embs, w, V1 - 1, dt, bf16) for dt in (np.float64, np.float32))
    print(f"STATELESS_TABLES C={C} bf16={bf16} err {np.max(np.abs(got - r64)):.3e} tol {_tol(r32, r64):.3e}")
    assert got.shape == (C, V1, J) and not got[:, V1 - 1].any() and np.max(np.abs(got - r64)) <= _tol(r32, r64)


SEEDS = {(13, 1, True, False, 2): 2, (13, 1, True, False, 0): 2, (13, 1, True, True, 2): 1, (13, 2, True, False, 2): 2,
         (13, 2, True, True, 2): 2, (13, 2, True, True, 0): 1, (37, 1, False, True, 2): 1, (37, 1, False, True, 0): 1,
         (37, 2, False, True, 2): 1, (37, 2, False, True, 0): 1, (37, 2, True, False, 2): 2, (37, 2, True, True, 2): 2,
         (37, 3, True, True, 2): 1}   # (V1, C, tdt, bf16, max_symbols) -> seed; absent: 0


@functools.lru_cache(maxsize=None)
def _search_case(v1, C, tdt, bf16, ms=2, max_out=10):
    """model on the dyadic grid, enc_proj [17, T, J], per stream (float64 result, float32 result); the joint is biased to labels"""
    rng = np.random.default_rng(SEEDS.get((v1, C, tdt, bf16, ms), 0))
    E, N = CE[C], v1 + (len(DUR) if tdt else 0)
    grid = lambda k, *s: (np.rint(rng.standard_normal(s) * k) / 8).astype(np.float32)
    embs = [grid(4, v1, e) for e in O.widths(E, C)]
    for e in embs:
        e[v1 - 1] = 0
    m = dict(embs=embs, w_pred=grid(16 * E ** -0.5, J, E), b_pred=grid(1, J), w_out=(rng.standard_normal((N, J)) * 3 * J ** -0.5),
             b_out=(rng.standard_normal(N) * 0.1).astype(np.float32))
    m["w_out"] = (O.bf16_round(m["w_out"]) if bf16 else m["w_out"]).astype(np.float32)
    m["b_out"][v1 - 1] -= 1.0
    f = grid(8, len(LENS), T, J)
    run = lambda b, dt: O.search(O.tables(embs, m["w_pred"], v1 - 1, dt, bf16), m["b_pred"], m["w_out"], m["b_out"], f[b], LENS[b],
                                 v1 - 1, ms, max_out, DUR if tdt else None, dt, bf16)
    return m, f, [(run(b, np.float64), run(b, np.float32)) for b in range(len(LENS))]


def _device_search(m, f, lens, v1, tdt, bf16, ms, max_out, state=None, stream=False):
    from nemo_amd import ops
    tabs = ops.stateless_tables([_dev(e) for e in m["embs"]], _dev(m["w_pred"], DT[bf16]), m["w_pred"].shape[1], v1 - 1)
    out = ops.stateless_greedy_decode(_dev(f, DT[bf16]), torch.tensor(lens, dtype=torch.int64, device="cuda"), tabs, _dev(m["b_pred"]),
                                      _dev(m["w_out"], DT[bf16]), J, _dev(m["b_out"]), v1 - 1, ms, durations=DUR if tdt else None,
                                      max_out=max_out, state=state, stream=stream)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("ms", [2, 0])   # 0: no cap per frame, the output budget ends a stream
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("tdt", [False, True], ids=["rnnt", "tdt"])
@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("v1", [13, 37])
def test_search_matches_the_oracle(v1, C, tdt, bf16, ms):
    m, f, refs = _search_case(v1, C, tdt, bf16, ms)
    assert min(r64["gap"] for r64, _ in refs) >= 1e-3, [r64["gap"] for r64, _ in refs]
    # two labels on one frame (max_symbols / duration 0), and max_out binds
    assert any(len(set(r64["fr"])) < len(r64["fr"]) for r64, _ in refs) and any(len(r64["tok"]) == 10 for r64, _ in refs)
    tokens, times, out_len, score = (o.cpu().numpy() for o in _device_search(m, f, LENS, v1, tdt, bf16, ms, 10))
    for b, (r64, r32) in enumerate(refs):
        n = out_len[b]
        assert list(tokens[b, :n]) == r64["tok"] and list(times[b, :n]) == r64["fr"], (b, r64["tok"], tokens[b])
        assert (tokens[b, n:] == -1).all() and (times[b, n:] == -1).all(), b
        tol = _tol(r32["score"], np.float64(r64["score"]))
        print(f"STATELESS_SEARCH b={b} score {score[b]:.7g} oracle {float(r64['score']):.7g} tol {tol:.3e}")
        assert abs(float(score[b]) - float(r64["score"])) <= tol, (b, float(score[b]), float(r64["score"]), tol)


@pytest.mark.parametrize("v1,C,tdt,bf16", [(13, 2, False, False), (37, 3, True, True)], ids=["rnnt-fp32", "tdt-bf16"])
def test_any_cut_and_any_row_give_the_bits_of_one_launch(v1, C, tdt, bf16):
    m, f, refs = _search_case(v1, C, tdt, bf16, 2, 2 * T)
    assert min(r64["gap"] for r64, _ in refs) >= 1e-3
    one, jumped = [o.cpu() for o in _device_search(m, f, LENS, v1, tdt, bf16, 2, 2 * T)], False
    for cut in [(9,), (1,) * 9, (4, 5), (3, 2, 4)]:
        state, a, toks = None, 0, [[] for _ in LENS]
        for n in cut:
            lens = [min(max(l - a, 0), n) for l in LENS]
            tokens, times, out_len, score, state = _device_search(m, f[:, a:a + n], lens, v1, tdt, bf16, 2, 2 * T, state=state, stream=True)
            jumped |= bool((state.skip > 0).any()) and a + n < T
            for b in range(len(LENS)):
                toks[b] += list(zip(tokens[b, :out_len[b]].tolist(), times[b, :out_len[b]].tolist()))
            a += n
        for b in range(len(LENS)):
            assert toks[b] == list(zip(one[0][b, :one[2][b]].tolist(), one[1][b, :one[2][b]].tolist())) and toks[b] == list(
                zip(refs[b][0]["tok"], refs[b][0]["fr"])), (cut, b)
        assert torch.equal(score.cpu().view(torch.int32), one[3].view(torch.int32)), cut   # score bits
    assert jumped or not tdt   # a chunk ended inside a TDT jump
    perm = np.random.default_rng(1).permutation(len(LENS))
    moved = [o.cpu() for o in _device_search(m, f[perm], [LENS[i] for i in perm], v1, tdt, bf16, 2, 2 * T)]
    for o, p in zip(one, moved):
        assert torch.equal(o[perm].view(torch.int32), p.view(torch.int32))


@pytest.mark.parametrize("tdt", [False, True], ids=["rnnt", "tdt"])
def test_decoders_resume_partial_hypotheses_and_cache_the_tables(tdt):
    from nemo_amd import ops
    from nemo_amd.modules import GreedyBatchedRNNTInfer, GreedyBatchedTDTInfer, RNNTJoint, StatelessTransducerDecoder
    torch.manual_seed(2)
    pred = StatelessTransducerDecoder(prednet=dict(pred_hidden=32, dropout=0.0), vocab_size=12, context_size=2).cuda().eval()
    joint = RNNTJoint(jointnet=dict(encoder_hidden=16, pred_hidden=32, joint_hidden=24, activation="relu", dropout=0.0), num_classes=12,
                      num_extra_outputs=3 * tdt).cuda().eval()
    joint.joint_net[-1].bias.data[12] -= 1.0
    infer = GreedyBatchedTDTInfer(pred, joint, 12, DUR, max_symbols_per_step=2) if tdt else GreedyBatchedRNNTInfer(
        pred, joint, 12, max_symbols_per_step=2)
    enc, lens = torch.randn(3, 16, T, device="cuda"), torch.tensor([T, 4, 0], device="cuda")
    one, hyps, tabs = infer(enc, lens)[0], infer.fresh_hypotheses(3), pred.search_tables(joint, enc.device)
    for a, b in ((0, 4), (4, T)):
        hyps = infer(enc[:, :, a:b], (lens - a).clamp(0, b - a), partial_hypotheses=hyps)[0]
    assert pred.search_tables(joint, enc.device) is tabs and sum(len(h.timestamp) for h in one) > 0   # not rebuilt per call
    for h, o in zip(hyps, one):
        assert (h.y_sequence.tolist(), h.timestamp, h.score, h.length) == (o.y_sequence.tolist(), o.timestamp, o.score, o.length)
    pred.prediction["embeds"][0].weight.data[1] += 1.0
    pred.weights_updated()   # what an optimizer step and load_state_dict call
    fresh = pred.search_tables(joint, enc.device)
    assert fresh is not tabs and torch.equal(fresh, ops.stateless_tables(pred._embs(), joint.pred.weight, 32, 12))


def test_model_trains_and_transcribes_through_the_stateless_decoder():
    from nemo_amd import ops
    from nemo_amd.models import EncDecRNNTModel, fastconformer_transducer_config
    from oracle import rnnt_ref, transducer_ref
    vocab = [chr(ord("a") + i) for i in range(12)]
    cfg = fastconformer_transducer_config("small", vocab_size=12, d_model=32, n_heads=4, n_layers=1, subsampling_conv_channels=16,
                                          stateless_context=2, dropout=0.0, dropout_pre_encoder=0.0, dropout_att=0.0)
    cfg["labels"], cfg["preprocessor"]["dither"] = vocab, 0.0
    cfg["decoder"]["prednet"].update(pred_hidden=32, dropout=0.0)
    cfg["joint"]["jointnet"].update(joint_hidden=24, dropout=0.0)
    torch.manual_seed(0)
    model = EncDecRNNTModel(cfg).to("cuda").train()
    model.joint.joint_net[-1].bias.data[12] -= 1.0
    rng = np.random.default_rng(0)
    audio = torch.from_numpy(rng.standard_normal((2, 12000)).astype(np.float32) * 0.1).cuda()
    audio[1, 9000:] = 0
    alen, tl = torch.tensor([12000, 9000], device="cuda"), torch.tensor([5, 3], device="cuda")
    tg = torch.from_numpy(rng.integers(0, 12, (2, 5))).cuda()
    out = model.training_step([audio, alen, tg, tl])
    out["loss"].backward()
    enc, enc_len = (x.detach() for x in model.forward(input_signal=audio, input_signal_length=alen))
    # the oracle: stateless forward -> the joint / loss oracle in float64 -> d dec -> the stateless embedding gradient
    embs = [e.detach().cpu().numpy() for e in model.decoder._embs()]
    dec = torch.from_numpy(O.forward(embs, tg.cpu().numpy(), 12)).transpose(1, 2).requires_grad_(True)
    logits = transducer_ref.joint_network({k: v.detach().cpu().double() for k, v in model.joint.state_dict().items()}, enc.cpu().double(), dec)
    nll, dlogits = rnnt_ref.rnnt_nll_autograd(logits, tg.cpu(), enc_len.cpu(), tl.cpu(), blank=12)
    logits.backward(dlogits / 2)   # mean_batch
    assert abs(out["loss"].item() - nll.item() / 2) <= 1e-4 * abs(nll.item() / 2), (out["loss"].item(), nll.item() / 2)
    for e, r64 in zip(model.decoder._embs(), O.embed_grad(embs, tg.cpu().numpy(), dec.grad.transpose(1, 2).numpy(), 12)):
        assert np.abs(e.grad.cpu().numpy() - r64).max() <= 1e-4 * np.abs(r64).max() and not e.grad[12].any()
    # transcribe == the ops-level search over the same encoder output
    hyps = model.transcribe([audio[0].cpu().numpy(), audio[1, :9000].cpu().numpy()], batch_size=2, return_hypotheses=True)
    enc, enc_len = model.eval().forward(input_signal=audio, input_signal_length=alen)
    tabs, o = ops.stateless_tables(model.decoder._embs(), model.joint.pred.weight, 32, 12), model.joint.joint_net[-1]
    tokens, times, out_len, score = ops.stateless_greedy_decode(model.decoding.decoding._enc_proj(enc, torch.float32), enc_len.to(torch.int64),
                                                                tabs, model.joint.pred.bias, o.weight, 24, o.bias, 12, 10)
    for b, h in enumerate(hyps):
        n = int(out_len[b])
        assert h.y_sequence.tolist() == tokens[b, :n].tolist() and h.timestamp == times[b, :n].tolist() and h.dec_state is None
        assert h.score == float(score[b]) and h.text == "".join(vocab[i] for i in tokens[b, :n].tolist()) and out_len.sum() > 0
