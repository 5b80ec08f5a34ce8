"""-m gpu: the greedy transducer search for prediction networks of L = 2..4 LSTM layers (mi355x_transducer_greedy_decode_layers, the
DEEP instantiations of csrc/rnnt_decode.hip) against the CPU restatement tests/rnnt_layers_oracle.py, and through the decoding
objects and the models.

  1. SMALL geometry: one-shot == resumable with a fresh state == any cut into chunks, bit for bit, every state field included;
     fp32 weights: the hypotheses are the restatement's exactly (its smallest top-2 gap, relative to the largest |logit|, is 2.4e-4
     for RNN-T and 1.2e-3 for TDT; the one-layer SMALL case passes the same exact comparison at 2.9e-5);
  2. `upper_layers=[]` is `upper_layers=None`, in all six forms;
  3. recipe widths, L = 2: chunked == one launch, and the device's hypotheses walked through the restatement (rule 2 of
     tests/test_stream_decode_gpu.py: every flip within 2e-4 x the largest |logit|, at most 2 % of the decisions flipped) -- exact
     equality is not asked there: the restatement's own smallest relative gap is 8e-5 / 1.7e-4, too close to the float32
     summation error over K = 640;
  4. confidences against the float64 measure (the bound of tests/test_confidence_gpu.py) and fusion models (zero weights, chunking,
     an effect), L = 2;
  5. the decoder objects with `partial_hypotheses`, and two-layer models: transcribe and the transducer stream step."""
import numpy as np
import pytest
import torch

import confidence_oracle as CO
import rnnt_fused_oracle as R
import rnnt_layers_oracle as O
from test_confidence_gpu import FLOOR, TRANSDUCER_METHODS, _method
from test_stream_decode_gpu import _cuttings, _dev_args

pytestmark = pytest.mark.gpu
dev = "cuda"
DUR = O.DUR
STATE = ("h", "c", "last", "score", "frames_done", "skip", "zero_run")
SMALL_LABELS = {("rnnt", 2): (135, 631), ("rnnt", 3): (120, 581), ("rnnt", 4): (145, 624),
                ("tdt", 2): (54, 80), ("tdt", 3): (54, 96), ("tdt", 4): (67, 115)}   # the restatement's, at max_symbols 2 / 10
SMALL_GAP = {"rnnt": 2.3e-4, "tdt": 1.2e-3}   # floors of its smallest top-2 gap over the largest |logit|


def _upper_args(Pd, wdt):
    """layers 1 .. L-1 as the searches' `upper_layers` (fp32 masters or bf16 images; biases fp32)"""
    H = Pd[O.Q + "weight_hh_l0"].shape[1]
    w = lambda t: t.to(dev).to(wdt).contiguous()   # noqa: E731
    f = lambda t: t.to(dev).float().contiguous()   # noqa: E731
    return [(w(Pd[O.Q + f"weight_ih_l{l}"]), H, w(Pd[O.Q + f"weight_hh_l{l}"]), H, f(Pd[O.Q + f"bias_ih_l{l}"]),
             f(Pd[O.Q + f"bias_hh_l{l}"])) for l in range(1, O.n_layers(Pd))]


def _hyps(tk, tm, n):
    tk, tm, n = tk.cpu(), tm.cpu(), n.cpu()
    for b in range(tk.shape[0]):
        assert (tk[b, int(n[b]):] == -1).all() and (tm[b, int(n[b]):] == -1).all()
    return [(tk[b, : int(n[b])].tolist(), tm[b, : int(n[b])].tolist()) for b in range(tk.shape[0])]


def _run_chunked(ops, f_all, lens, args, up, blank, ms, edges, durations, method=None, pairs=None):
    """-> per stream (tokens, times[, tok_conf bit patterns]), the final state, per chunk (skip_out, frames_done_out)[, the last
    `score` output: with models]"""
    B = f_all.shape[0]
    rows = [([], [], []) for _ in range(B)]
    state, trail, score = None, [], None
    if pairs is not None:
        state = ops.RNNTFusedStreamState.fresh(B, args[0].shape[1], blank, dev, layers=1 + len(up))
    for lo, hi in zip(edges[:-1], edges[1:]):
        cl = (lens - lo).clamp(min=0, max=hi - lo).to(dev)
        fc = f_all[:, lo:hi].contiguous()
        tc = None
        if pairs is not None:
            tk, tm, n, score, state = ops.transducer_greedy_decode_fused(fc, cl, *args, blank, ms, pairs, durations=durations, state=state,
                                                                         upper_layers=up)
        elif method is not None and durations is None:
            tk, tm, n, state, tc = ops.rnnt_greedy_decode_stream_conf(fc, cl, *args, blank, ms, method, state=state, upper_layers=up)
        elif method is not None:
            tk, tm, n, state, tc = ops.tdt_greedy_decode_stream_conf(fc, cl, *args, blank, durations, ms, method, state=state,
                                                                     upper_layers=up)
        elif durations is None:
            tk, tm, n, state = ops.rnnt_greedy_decode_stream(fc, cl, *args, blank, ms, state=state, upper_layers=up)
        else:
            tk, tm, n, state = ops.tdt_greedy_decode_stream(fc, cl, *args, blank, durations, ms, state=state, upper_layers=up)
        for b, (t_b, f_b) in enumerate(_hyps(tk, tm, n)):
            rows[b][0].extend(t_b); rows[b][1].extend(f_b)
            if tc is not None:
                k = len(t_b)
                assert (tc[b, k:] == 0.0).all()
                rows[b][2].extend(tc[b, :k].cpu().view(torch.int32).tolist())
        trail.append((state.skip.cpu().clone(), state.frames_done.cpu().clone()))
    hyps = [(r[0], r[1]) + ((r[2],) if method is not None else ()) for r in rows]
    return (hyps, state, trail) + ((score,) if pairs is not None else ())


def _one_shot(ops, kind, f, lens, args, up, V, ms, **kw):
    if kind == "rnnt":
        return ops.rnnt_greedy_decode(f, lens, *args, V, ms, with_state=True, upper_layers=up, **kw)
    return ops.tdt_greedy_decode(f, lens, *args, V, DUR, ms, with_state=True, upper_layers=up, **kw)


_small = {}


def _small_reference(kind, L, ms):
    """the restatement's hypotheses and gaps of a SMALL case, computed once"""
    key = (kind, L, ms)
    if key not in _small:
        Pd, Pj = O.small_case(kind, L)
        gaps = []
        hyps, _, _ = O.decode_chunked(Pd, Pj, O.small_enc(), torch.tensor(O.SMALL["lens"]), O.SMALL["V"], ms, [],
                                      DUR if kind == "tdt" else None, gaps=gaps)
        _small[key] = (hyps, min(g / s for g, s in gaps))
    return _small[key]


@pytest.mark.parametrize("L", [2, 3, 4])
@pytest.mark.parametrize("max_symbols", [2, 10])
@pytest.mark.parametrize("kind", ["rnnt", "tdt"])
@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_small_geometry_one_shot_resumable_chunked_and_the_restatement(wdt, kind, max_symbols, L):
    from nemo_amd import ops
    V, H, B, T = O.SMALL["V"], O.SMALL["H"], 4, O.SMALL["T"]
    lens = torch.tensor(O.SMALL["lens"])
    durations = DUR if kind == "tdt" else None
    Pd, Pj = O.small_case(kind, L)
    f_all = torch.nn.functional.linear(O.small_enc().transpose(1, 2), Pj["enc.weight"], Pj["enc.bias"]).to(dev).contiguous()
    args, up = _dev_args(Pd, Pj, wdt), _upper_args(Pd, wdt)
    assert len(up) == L - 1
    one, st1, _ = _run_chunked(ops, f_all, lens, args, up, V, max_symbols, [0, T], durations)
    tk, tm, n, sc, (h, c) = _one_shot(ops, kind, f_all, lens.to(dev), args, up, V, max_symbols)
    assert _hyps(tk, tm, n) == one
    assert tuple(h.shape) == (L, B, H) and tuple(st1.h.shape) == (L, B, H) and tuple(st1.c.shape) == (L, B, H)
    assert torch.equal(sc, st1.score) and torch.equal(h, st1.h) and torch.equal(c, st1.c)
    assert st1.frames_done.tolist() == lens.tolist()
    assert bool(st1.h[L - 1].any()) and not torch.equal(st1.h[0], st1.h[L - 1])   # the upper layers carry a state of their own
    assert sum(len(o[0]) for o in one) > 20
    per_frame = torch.cat([torch.bincount(torch.tensor(o[1], dtype=torch.long), minlength=T)[: int(n_b)] for o, n_b in zip(one, lens)])
    assert int(per_frame.max()) == max_symbols and int(per_frame.min()) == 0, per_frame
    crossed = False
    for name, edges in _cuttings(T).items():
        got, st, trail = _run_chunked(ops, f_all, lens, args, up, V, max_symbols, edges, durations)
        assert got == one, name
        for a in STATE:
            assert torch.equal(getattr(st, a), getattr(st1, a)), (name, a)
        crossed |= any(bool(((skip > 0) & (done < lens)).any()) for skip, done in trail)
    if kind == "tdt":
        assert crossed   # a predicted duration jumped over a chunk edge inside an utterance
    if wdt == torch.float32:
        want, gap = _small_reference(kind, L, max_symbols)
        assert sum(len(w[0]) for w in want) == SMALL_LABELS[kind, L][max_symbols == 10] and gap >= SMALL_GAP[kind], gap
        assert one == want


def test_an_empty_layer_list_is_the_one_layer_search():
    """`upper_layers=[]` and `upper_layers=None`: equal results and shapes in the six forms (one-shot, stream, conf, stream-conf,
    fused one-shot, fused stream)"""
    from nemo_amd import ops
    V, T, ms = O.SMALL["V"], O.SMALL["T"], 10
    lens = torch.tensor(O.SMALL["lens"]).to(dev)
    Pd, Pj = O.small_case("rnnt", 1)
    f = torch.nn.functional.linear(O.small_enc().transpose(1, 2), Pj["enc.weight"], Pj["enc.bias"]).to(dev).contiguous()
    args = _dev_args(Pd, Pj, torch.float32)
    method = _method(*TRANSDUCER_METHODS["default"]).kernel_args(V + 1)
    case = dict(V=V, ng=R.LO.make_lm(R.LM_SEED, V, R.LM_ORDER), phrases=[(1, 2), (3, 4, 5)])
    _, pairs = R.case_models(case, "both")
    half = f[:, :20].contiguous()
    hl = lens.clamp(max=20)

    def flat(out):
        res = []
        for x in out:
            if isinstance(x, ops.RNNTStreamState):
                res += list(x.tensors())
            elif isinstance(x, tuple):
                res += list(x)
            else:
                res.append(x)
        return res

    def forms(up):
        st = ops.rnnt_greedy_decode_stream(half, hl, *args, V, ms, upper_layers=up)[3]
        stc = ops.rnnt_greedy_decode_stream_conf(half, hl, *args, V, ms, method, upper_layers=up)[3]
        stf = ops.transducer_greedy_decode_fused(half, hl, *args, V, ms, pairs, upper_layers=up,
                                                 state=ops.RNNTFusedStreamState.fresh(4, args[0].shape[1], V, dev))[4]
        rest, rl = f[:, 20:].contiguous(), (lens - 20).clamp(min=0)
        return [ops.rnnt_greedy_decode(f, lens, *args, V, ms, with_state=True, upper_layers=up),
                ops.rnnt_greedy_decode_stream(rest, rl, *args, V, ms, state=st, upper_layers=up),
                ops.rnnt_greedy_decode_conf(f, lens, *args, V, ms, method, with_state=True, upper_layers=up),
                ops.rnnt_greedy_decode_stream_conf(rest, rl, *args, V, ms, method, state=stc, upper_layers=up),
                ops.transducer_greedy_decode_fused(f, lens, *args, V, ms, pairs, upper_layers=up),
                ops.transducer_greedy_decode_fused(rest, rl, *args, V, ms, pairs, state=stf, upper_layers=up)]

    for i, (a, b) in enumerate(zip(forms(None), forms([]))):
        fa, fb = flat(a), flat(b)
        assert len(fa) == len(fb) and int(a[2].sum()) > 20, i
        for x, y in zip(fa, fb):
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), i


@pytest.mark.parametrize("kind", ["rnnt", "tdt"])
def test_layers_entry_without_upper_layers_is_the_one_layer_entry(kind):
    """the C entry itself: mi355x_transducer_greedy_decode_layers with a null struct and with n_upper = 0 against
    mi355x_transducer_greedy_decode on the same descriptor (one-shot with score and h / c [B, H]): the same bits"""
    import ctypes as C
    from nemo_amd import _lib
    V, H, J, B, T, ms = O.SMALL["V"], O.SMALL["H"], O.SMALL["J"], 4, O.SMALL["T"], 10
    Pd, Pj = O.small_case(kind, 1)
    f = torch.nn.functional.linear(O.small_enc().transpose(1, 2), Pj["enc.weight"], Pj["enc.bias"]).to(dev).contiguous()
    lens = torch.tensor(O.SMALL["lens"]).to(dev)
    emb, w_ih, _, w_hh, _, b_ih, b_hh, w_pred, _, b_pred, w_out, _, b_out = _dev_args(Pd, Pj, torch.float32)
    dur = (C.c_int * len(DUR))(*DUR)
    stream = torch.cuda.current_stream().cuda_stream

    def run(call):
        i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=dev)   # noqa: E731
        f32 = lambda *shape: torch.full(shape, -7.0, dtype=torch.float32, device=dev)   # noqa: E731
        out = [i32(B, T * ms), i32(B, T * ms), i32(B), f32(B), f32(B, H), f32(B, H)]
        p = lambda t: t.data_ptr()   # noqa: E731
        d = _lib.TransducerGreedyDesc(
            enc_proj=p(f), f_dtype=0, ldf=J, enc_len=p(lens), emb=p(emb), w_ih=p(w_ih), ld_ih=H, w_hh=p(w_hh), ld_hh=H, b_ih=p(b_ih),
            b_hh=p(b_hh), w_pred=p(w_pred), ld_pred=H, b_pred=p(b_pred), w_out=p(w_out), ld_out=J, b_out=p(b_out), w_dtype=0, B=B, T=T,
            J=J, H=H, V1=V + 1, blank=V, max_symbols=ms, max_out=T * ms, tokens=p(out[0]), times=p(out[1]), out_len=p(out[2]),
            score=p(out[3]), h_out=p(out[4]), c_out=p(out[5]))
        if kind == "tdt":
            d.D, d.durations = len(DUR), C.addressof(dur)
        assert call(d) == 0
        torch.cuda.synchronize()
        return out

    lib = _lib.lib
    want = run(lambda d: lib.mi355x_transducer_greedy_decode(C.byref(d), stream))
    assert int(want[2].sum()) > 20
    empty = _lib.TransducerLstmLayers(n_upper=0)
    for name, call in (("null", lambda d: lib.mi355x_transducer_greedy_decode_layers(C.byref(d), None, stream)),
                       ("n_upper = 0", lambda d: lib.mi355x_transducer_greedy_decode_layers(C.byref(d), C.byref(empty), stream))):
        for x, y in zip(run(call), want):
            assert torch.equal(x, y), name


def _rule2(rows_per_utt, n_labels):
    """rule 2 of tests/test_stream_decode_gpu.py with the floors of these cases (the TDT restatement takes 120 decisions)"""
    decisions = [r for rows in rows_per_utt for r in rows]
    flips = [r for r in decisions if r[1] != r[2]]
    assert len(decisions) > 100 and n_labels > 40, (len(decisions), n_labels)
    for t, follow, own, margin, scale in flips:
        assert margin <= 2e-4 * scale, (t, follow, own, margin, scale)
    assert len(flips) <= 0.02 * len(decisions), (len(flips), len(decisions))
    return len(flips), len(decisions)


@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["rnnt", "tdt"])
def test_recipe_widths_two_layers_by_the_forced_walk(kind, wdt):
    from nemo_amd import ops
    C = O.RECIPE
    V, T, ms = C["V"], C["T"], C["max_symbols"]
    lens = torch.tensor(C["lens"])
    durations = DUR if kind == "tdt" else None
    Pd, Pj = O.recipe_case(kind, 2)
    enc = O.recipe_enc()[:, :, :T]
    if wdt == torch.bfloat16:
        Pd_r, Pj_r, f_r = O.bf16_images(Pd, Pj, enc)
        f_dev = f_r.to(dev).to(torch.bfloat16)
    else:
        Pd_r, Pj_r = Pd, Pj
        f_r = torch.nn.functional.linear(enc.transpose(1, 2), Pj["enc.weight"], Pj["enc.bias"])
        f_dev = f_r.to(dev).contiguous()
    args, up = _dev_args(Pd, Pj, wdt), _upper_args(Pd, wdt)
    one, st1, _ = _run_chunked(ops, f_dev, lens, args, up, V, ms, [0, T], durations)
    chk, st, _ = _run_chunked(ops, f_dev, lens, args, up, V, ms, [0, 1, 14, 27, T], durations)
    assert chk == one
    for a in STATE:
        assert torch.equal(getattr(st, a), getattr(st1, a)), a
    rep = O.forced_walk(Pd_r, Pj_r, f_r, lens, V, ms, one, durations)
    print(kind, wdt, "flips / decisions:", _rule2(rep, sum(len(o[0]) for o in one)))


@pytest.mark.parametrize("which", list(TRANSDUCER_METHODS))
@pytest.mark.parametrize("kind", ["rnnt", "tdt"])
def test_confidence_with_two_layers(kind, which):
    """tok_conf against the float64 measure over the restatement's label logits, within max(8 x the float32 restatement's own
    error, 16 ulp); everything else the bits of the search without a measure; chunked tok_conf the bits of one launch"""
    from nemo_amd import ops
    V, B, T, ms = O.SMALL["V"], 4, O.SMALL["T"], 10
    lens = torch.tensor(O.SMALL["lens"])
    durations = DUR if kind == "tdt" else None
    cfg = _method(*TRANSDUCER_METHODS[which])
    method = cfg.kernel_args(V + 1)
    Pd, Pj = O.small_case(kind, 2)
    f_r = torch.nn.functional.linear(O.small_enc().transpose(1, 2), Pj["enc.weight"], Pj["enc.bias"])
    f_dev = f_r.to(dev).contiguous()
    args, up = _dev_args(Pd, Pj, torch.float32), _upper_args(Pd, torch.float32)
    plain = _one_shot(ops, kind, f_dev, lens.to(dev), args, up, V, ms)
    if kind == "rnnt":
        withc = ops.rnnt_greedy_decode_conf(f_dev, lens.to(dev), *args, V, ms, method, with_state=True, upper_layers=up)
    else:
        withc = ops.tdt_greedy_decode_conf(f_dev, lens.to(dev), *args, V, DUR, ms, method, with_state=True, upper_layers=up)
    for a, w, what in zip(withc[:4], plain[:4], ("tokens", "times", "out_len", "score")):
        assert torch.equal(a, w), what
    assert torch.equal(withc[4][0], plain[4][0]) and torch.equal(withc[4][1], plain[4][1])
    tokens, times, out_len, tok_conf = withc[0].cpu(), withc[1].cpu(), withc[2].cpu(), withc[5].cpu()
    assert int(out_len.sum()) > 20
    err = e32 = 0.0
    for b in range(B):
        n = int(out_len[b])
        assert (tok_conf[b, n:] == 0.0).all()
        tk, tm = tokens[b, :n].tolist(), times[b, :n].tolist()
        w64 = O.replay_confidence(Pd, Pj, f_r[b], tk, tm, V, cfg, n_dur=len(DUR) if durations else 0)
        w32 = O.replay_confidence(Pd, Pj, f_r[b], tk, tm, V, cfg, n_dur=len(DUR) if durations else 0, dtype=torch.float32)
        if n:
            e32 = max(e32, float(np.abs(w32 - w64).max()))
            err = max(err, float(np.abs(tok_conf[b, :n].numpy() - w64).max()))
    tol = max(8 * e32, FLOOR)
    print(f"CONF_ERR L=2 {kind} {which} token={err:.3e} e32={e32:.3e} tol={tol:.3e} labels={int(out_len.sum())}")
    one, st1, _ = _run_chunked(ops, f_dev, lens, args, up, V, ms, [0, T], durations, method=method)
    for b in range(B):
        n = int(out_len[b])
        assert one[b] == (tokens[b, :n].tolist(), times[b, :n].tolist(), tok_conf[b, :n].view(torch.int32).tolist()), b
    for name, edges in _cuttings(T).items():
        got, st, _ = _run_chunked(ops, f_dev, lens, args, up, V, ms, edges, durations, method=method)
        assert got == one, name
        for a in STATE:
            assert torch.equal(getattr(st, a), getattr(st1, a)), (name, a)
    assert err <= tol, (err, tol)
    assert CO.method_row(cfg) in ("max_prob", "gibbs", "tsallis")


@pytest.mark.parametrize("which", ["tree", "both"])
@pytest.mark.parametrize("kind", ["rnnt", "tdt"])
def test_fusion_models_with_two_layers(kind, which):
    """one model (a tree) and two (an n-gram model and a tree), built as tests/test_rnnt_fused_gpu.py builds them over the
    two-layer restatement's own hypotheses: zero weights give the bits of the model-less search, non-zero weights change a
    hypothesis, and any cut gives the bits of one launch, `m_state` included"""
    from nemo_amd import ops
    V, T, ms = O.SMALL["V"], O.SMALL["T"], R.MAX_SYMBOLS
    lens = torch.tensor([37, 30, 0, 9])   # ragged, one stream without a frame
    durations = DUR if kind == "tdt" else None
    Pd, Pj = O.small_case(kind, 2)
    f_cpu = torch.nn.functional.linear(O.small_enc().transpose(1, 2), Pj["enc.weight"], Pj["enc.bias"])
    f_all = f_cpu.to(dev).contiguous()
    base, _, _ = O.decode_chunked(Pd, Pj, None, lens, V, ms, [], durations, f_all=f_cpu)
    case = dict(V=V, ng=R.LO.make_lm(R.LM_SEED, V, R.LM_ORDER), phrases=R.phrases_from(base, V))
    args, up = _dev_args(Pd, Pj, torch.float32), _upper_args(Pd, torch.float32)
    fused = lambda pairs, **kw: ops.transducer_greedy_decode_fused(f_all, lens.to(dev), *args, V, ms, pairs, durations=durations,  # noqa: E731
                                                                   upper_layers=up, **kw)
    # every alpha 0: the model-less two-layer search, one-shot and resumable
    _, zero = R.case_models(case, which, tree_alpha=0.0, lm_alpha=0.0)
    got = fused(zero)
    want = _one_shot(ops, kind, f_all, lens.to(dev), args, up, V, ms)
    assert _hyps(*want[:3]) == base and sum(len(b[0]) for b in base) > 40
    for name, a, b in zip(("tokens", "frames", "lengths", "score"), got[:4], want[:4]):
        assert torch.equal(a, b), name
    assert torch.equal(got[4][0], want[4][0]) and torch.equal(got[4][1], want[4][1]) and got[4][0].shape[0] == 2
    _, wst, _ = _run_chunked(ops, f_all, lens, args, up, V, ms, [0, T], durations)
    _, zst, _, zsc = _run_chunked(ops, f_all, lens, args, up, V, ms, [0, T], durations, pairs=zero)
    assert torch.equal(zsc, wst.score)
    for a in STATE:
        assert torch.equal(getattr(zst, a), getattr(wst, a)), a
    # the models at work
    _, pairs = R.case_models(case, which)
    tk, tm, n, sc, (h, c) = fused(pairs)
    assert _hyps(tk, tm, n) != base
    one, st1, _, sc1 = _run_chunked(ops, f_all, lens, args, up, V, ms, [0, T], durations, pairs=pairs)
    assert _hyps(tk, tm, n) == one and torch.equal(sc, sc1) and torch.equal(h, st1.h) and torch.equal(c, st1.c)
    assert bool((st1.m_state[:, : len(pairs)] != 1).any()) and one[2] == ([], [])
    g = torch.Generator().manual_seed(78)
    rnd = sorted(set(torch.randint(1, T, (5,), generator=g).tolist()))
    for edges in (list(range(T + 1)), [0, 1, 14, 27, T], [0] + rnd + [T]):
        got, st, _, sc = _run_chunked(ops, f_all, lens, args, up, V, ms, edges, durations, pairs=pairs)
        assert got == one and torch.equal(sc, sc1), edges
        for a in STATE + ("m_state",):
            assert torch.equal(getattr(st, a), getattr(st1, a)), (edges, a)


@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["rnnt", "tdt"])
def test_decoder_objects_over_a_two_layer_prediction_network(kind, cdt):
    """three chunks through `forward(..., partial_hypotheses=...)` equal `forward` over the concatenation (the projection step
    hands out slices of the whole-sequence projection, as tests/test_stream_decode_gpu.py does for the unconditional comparison);
    the object's arguments are the op's: its one-shot result is the op called with the restatement's weights"""
    from nemo_amd import ops
    from nemo_amd.modules import GreedyBatchedRNNTInfer, GreedyBatchedTDTInfer, RNNTDecoder, RNNTJoint
    V, H, D, J, T = (O.SMALL[k] for k in "VHDJT")
    ms = 10
    lens = torch.tensor(O.SMALL["lens"])
    Pd, Pj = O.small_case(kind, 2)
    dec = RNNTDecoder(prednet={"pred_hidden": H, "pred_rnn_layers": 2, "dropout": 0.0}, vocab_size=V, compute_dtype=cdt)
    joint = RNNTJoint(jointnet={"encoder_hidden": D, "pred_hidden": H, "joint_hidden": J, "activation": "relu", "dropout": 0.0},
                      num_classes=V, num_extra_outputs=len(DUR) if kind == "tdt" else 0, compute_dtype=cdt)
    out = [k[:-len("weight")] for k in joint.state_dict() if k.startswith("joint_net.") and k.endswith(".weight")][0]
    dec.load_state_dict(Pd); joint.load_state_dict({k.replace("joint_net.2.", out): v for k, v in Pj.items()})
    dec, joint = dec.to(dev).eval(), joint.to(dev).eval()
    if kind == "tdt":
        infer = GreedyBatchedTDTInfer(dec, joint, V, DUR, max_symbols_per_step=ms)
    else:
        infer = GreedyBatchedRNNTInfer(dec, joint, V, max_symbols_per_step=ms)
    encd = O.small_enc().to(dev)
    whole = infer(encoder_output=encd, encoded_lengths=lens.to(dev))[0]
    assert sum(len(w.y_sequence) for w in whole) > 20
    assert all(isinstance(w.dec_state, tuple) and tuple(w.dec_state[0].shape) == (2, H) == tuple(w.dec_state[1].shape) for w in whole)
    f_whole, args = infer._project(encd)
    up = infer._upper(dev)
    assert len(up) == 1 and up[0][0].dtype == cdt and up[0][4].dtype == torch.float32
    if cdt == torch.float32:   # the masters: what the op gives for the restatement's weights
        tk, tm, n, sc, _ = _one_shot(ops, kind, f_whole, lens.to(dev), _dev_args(Pd, Pj, cdt), _upper_args(Pd, cdt), V, ms)
        assert _hyps(tk, tm, n) == [(w.y_sequence.tolist(), w.timestamp) for w in whole] and sc.tolist() == [w.score for w in whole]
    hyps = infer.fresh_hypotheses(len(lens))
    assert all(tuple(h.dec_state.h.shape) == (2, 1, H) and h.dec_state.h.is_cuda for h in hyps)
    project = infer._project
    try:
        for lo, hi in zip([0, 13, 26], [13, 26, T]):
            infer._project = lambda chunk, lo=lo, hi=hi: (f_whole[:, lo:hi].contiguous(), args)
            cl = (lens - lo).clamp(min=0, max=hi - lo).to(dev)
            hyps = infer(encoder_output=encd[:, :, lo:hi].contiguous(), encoded_lengths=cl, partial_hypotheses=hyps)[0]
    finally:
        infer._project = project
    for b, (h, w) in enumerate(zip(hyps, whole)):
        assert h.y_sequence.tolist() == w.y_sequence.tolist() and h.timestamp == w.timestamp and h.score == w.score, b
        assert h.length == w.length and tuple(h.dec_state.h.shape) == (2, 1, H)
        assert torch.equal(h.dec_state.h[:, 0], w.dec_state[0]) and torch.equal(h.dec_state.c[:, 0], w.dec_state[1])


VOCAB = [chr(ord("a") + i) for i in range(26)] + [" ", "'"]


def _two_layer_model(hybrid, greedy=None, confidence=None, prepare=None, seed=4, **enc):
    from nemo_amd.models import EncDecHybridRNNTCTCModel, EncDecRNNTModel, fastconformer_hybrid_config, fastconformer_transducer_config
    over = dict(d_model=64, n_heads=4, n_layers=2, subsampling_conv_channels=32, dropout=0.0, dropout_pre_encoder=0.0, dropout_att=0.0,
                compute_dtype=torch.float32)
    over.update(enc)
    cfg = (fastconformer_hybrid_config("small", vocab_size=len(VOCAB), ctc_loss_weight=0.3, **over) if hybrid else
           fastconformer_transducer_config("small", vocab_size=len(VOCAB), **over))
    cfg["labels"] = VOCAB
    cfg["preprocessor"]["dither"] = 0.0
    cfg["decoder"]["prednet"].update(pred_hidden=64, pred_rnn_layers=2, dropout=0.0)
    cfg["joint"]["jointnet"].update(joint_hidden=64, dropout=0.0)
    cfg["decoding"] = dict(strategy="greedy_batch", greedy=dict(greedy or {}, max_symbols=3))
    if confidence:
        cfg["decoding"]["confidence_cfg"] = confidence
    torch.manual_seed(seed)
    m = (EncDecHybridRNNTCTCModel if hybrid else EncDecRNNTModel)(cfg)
    assert m.decoder.pred_rnn_layers == 2
    with torch.no_grad():   # a transducer head that emits labels
        for p in list(m.decoder.parameters()) + list(m.joint.parameters()):
            p.mul_(4.0)
        if prepare is not None:
            prepare(m)
    return m.to(dev).eval()


@pytest.mark.parametrize("hybrid", [False, True], ids=["rnnt", "hybrid"])
def test_two_layer_models_transcribe(hybrid):
    """transcribe returns text; with `greedy.boosting_tree` the fused search runs and changes it; with a `confidence_cfg` every
    label and word carries a confidence"""
    g = torch.Generator().manual_seed(7)
    waves = [0.1 * torch.randn(32000, generator=g), 0.1 * torch.randn(19200, generator=g)]
    m = _two_layer_model(hybrid)
    before = m.transcribe(waves, batch_size=2, return_hypotheses=True)
    ids = [h.y_sequence.tolist() for h in before]
    assert all(isinstance(h.text, str) for h in before) and sum(len(i) for i in ids) >= 12, ids
    assert all(tuple(h.dec_state[0].shape) == (2, 64) for h in before)
    phrases = ["".join(VOCAB[j] for j in i[k:k + 2]) + VOCAB[(i[k + 2] + 1 + k) % 26] for i in ids for k in range(0, len(i) - 2, 2)]
    phrases = sorted({p for p in phrases if p.isalpha()})
    assert len(phrases) >= 3
    boosted = _two_layer_model(hybrid, greedy=dict(boosting_tree=dict(key_phrases_list=phrases, context_score=1.0, depth_scaling=2.0),
                                                   boosting_tree_alpha=4.0))
    assert boosted.decoding.decoding.fusion_models is not None
    after = boosted.transcribe(waves, batch_size=2, return_hypotheses=True)
    assert [h.y_sequence.tolist() for h in after] != ids and all(isinstance(h.text, str) for h in after)
    conf = _two_layer_model(hybrid, confidence=dict(preserve_token_confidence=True, preserve_word_confidence=True))
    hc = conf.transcribe(waves, batch_size=2, return_hypotheses=True)
    assert [h.y_sequence.tolist() for h in hc] == ids
    for h in hc:
        assert len(h.token_confidence) == len(h.y_sequence) and len(h.word_confidence) == len(h.text.split())
        assert all(np.isfinite(h.token_confidence))


STREAM_SEED = 4   # the model seed of the streaming case: chosen for the condition on the OFFLINE search that the test asserts first


def _stream_case(seed):
    """a two-layer hybrid model with a cache-aware encoder, three utterances: the offline forward and its one-launch hypotheses,
    the CPU restatement's search on the offline encoder output with its per-decision gaps, and the hypotheses streamed chunk by
    chunk through `conformer_stream_step` (the encoder's chunk outputs recorded)"""
    from nemo_amd.streaming import CacheAwareStreamingAudioBuffer
    from test_streaming_gpu import _randomise

    def prepare(m):   # (on the host, before the model moves to the device)
        _randomise(m.encoder, seed + 8)
        m.joint.joint_net[-1].bias[len(VOCAB)] += 2.0
    m = _two_layer_model(True, prepare=prepare, seed=seed, subsampling="striding", subsampling_factor=4, causal_downsampling=True,
                         att_context_size=[16, 3], att_context_style="chunked_limited", conv_kernel_size=9, conv_context_size="causal")
    V, ms = len(VOCAB), 3
    g = torch.Generator().manual_seed(13)
    audio, alen = (0.1 * torch.randn(3, 48000, generator=g)).to(dev), torch.tensor([48000, 34000, 18000]).to(dev)
    with torch.no_grad():
        mel, mel_len = m.preprocessor(input_signal=audio, length=alen)
        enc_off, enc_len = m.forward(processed_signal=mel, processed_signal_length=mel_len)
    offline = m.decoding.rnnt_decoder_predictions_tensor(enc_off, enc_len)
    Pd = {k: v.detach().float().cpu() for k, v in m.decoder.state_dict().items()}
    Pj = {k: v.detach().float().cpu() for k, v in m.joint.state_dict().items()}
    assert O.n_layers(Pd) == 2
    f_off = torch.nn.functional.linear(enc_off.float().cpu().transpose(1, 2), Pj["enc.weight"], Pj["enc.bias"])
    gaps = []
    want, _, _ = O.decode_chunked(Pd, Pj, None, enc_len.cpu(), V, ms, [], f_all=f_off, gaps=gaps)
    rec, step = [], m.encoder.cache_aware_stream_step

    def recording(**kw):
        res = step(**kw)
        rec.append((res[0].detach().clone(), res[1].detach().clone()))
        return res
    m.encoder.cache_aware_stream_step = recording
    ch, tm, ln = m.encoder.get_initial_cache_state(batch_size=3)
    hyps = None
    buf = CacheAwareStreamingAudioBuffer(m, mel, mel_len)
    try:
        for chunk, cl in buf:
            _, hyps, ch, tm, ln, _ = m.conformer_stream_step(
                processed_signal=chunk, processed_signal_length=cl, cache_last_channel=ch, cache_last_time=tm,
                cache_last_channel_len=ln, previous_hypotheses=hyps, drop_extra_pre_encoded=buf.drop_extra_pre_encoded)
            assert all(tuple(h.dec_state.h.shape) == (2, 1, 64) for h in hyps)
    finally:
        m.encoder.cache_aware_stream_step = step
    return dict(m=m, V=V, ms=ms, enc_off=enc_off, enc_len=enc_len, offline=offline, Pd=Pd, Pj=Pj, f_off=f_off, gaps=gaps, want=want,
                hyps=hyps, rec=rec)


def test_two_layer_model_streams_through_the_transducer_stream_step():
    """rnnt_conformer_stream_step chunk by chunk (decoder state [2, 1, H] carried in the hypotheses) EQUALS the offline transcript:
    text, token ids and frame indices.  The cache-aware encoder's chunk outputs are the offline values up to float32 rounding, not
    their bits, so equality can be asked only where the offline search has no near-tie; that condition is asserted first, on the
    restatement's search over the offline encoder output (as tests/test_hybrid_gpu.py checks its one-layer case): no decision with a
    top-2 gap below 2e-4 x its largest |logit|, and the device's offline hypotheses are the restatement's.  In addition the streamed
    hypotheses are the one-launch search over the collected streamed encoder output when its projection is handed out in slices,
    and they pass the forced walk along the offline output."""
    c = _stream_case(STREAM_SEED)
    m, V, ms, enc_off, enc_len, offline, hyps, rec = (c[k] for k in ("m", "V", "ms", "enc_off", "enc_len", "offline", "hyps", "rec"))
    # the condition: the offline fp32 search is decided everywhere
    near = sum(1 for gap, scale in c["gaps"] if gap < 2e-4 * scale)
    print("offline fp32 search: decisions", len(c["gaps"]), "near-ties", near, "smallest relative gap",
          min(gap / scale for gap, scale in c["gaps"]))
    assert len(c["gaps"]) > 100 and sum(len(w[0]) for w in c["want"]) > 40 and near == 0
    assert [(o.y_sequence.tolist(), o.timestamp) for o in offline] == c["want"]
    # streamed == offline
    assert len(rec) >= 3 and all(isinstance(h.text, str) for h in hyps)
    got = [(h.y_sequence.tolist(), h.timestamp) for h in hyps]
    assert [h.text for h in hyps] == [o.text for o in offline]
    assert got == [(o.y_sequence.tolist(), o.timestamp) for o in offline]
    assert [h.length for h in hyps] == enc_len.tolist()
    # the collected streamed encoder output in one launch; then the same chunks with slices of ITS projection: equal, unconditionally
    infer = m.decoding.decoding
    Tm, D = int(enc_len.max()), enc_off.shape[1]
    coll, fill = torch.zeros(3, D, Tm, device=dev), [0, 0, 0]
    for e, l in rec:
        for b in range(3):
            n = int(l[b])
            coll[b, :, fill[b]:fill[b] + n] = e[b, :, :n]
            fill[b] += n
    assert fill == enc_len.tolist()
    one = m.decoding.rnnt_decoder_predictions_tensor(coll, enc_len)
    f_whole, args = infer._project(coll)
    project, hyps2, off = infer._project, infer.fresh_hypotheses(3), [0, 0, 0]
    try:
        for e, l in rec:
            fc = torch.zeros(3, e.shape[2], f_whole.shape[2], dtype=f_whole.dtype, device=dev)
            for b in range(3):
                n = int(l[b])
                fc[b, :n] = f_whole[b, off[b]:off[b] + n]
                off[b] += n
            infer._project = lambda chunk, fc=fc: (fc, args)
            hyps2 = m.decoding.rnnt_decoder_predictions_tensor(e, l, return_hypotheses=True, partial_hypotheses=hyps2)
    finally:
        infer._project = project
    for h, o in zip(hyps2, one):
        assert torch.equal(h.y_sequence, o.y_sequence) and h.timestamp == o.timestamp and h.score == o.score and h.text == o.text
    # and the forced walk along the offline encoder output
    rep = O.forced_walk(c["Pd"], c["Pj"], c["f_off"], enc_len.cpu(), V, ms, got)
    print("streamed vs offline, flips / decisions:", _rule2(rep, sum(len(g_[0]) for g_ in got)))
