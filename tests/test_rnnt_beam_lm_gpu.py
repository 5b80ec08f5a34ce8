"""-m gpu: `ops.transducer_beam_decode_fused` (csrc/rnnt_beam.hip, the LM instantiations) against the float64 oracle of its rule
(tests/rnnt_beam_lm_oracle.py: the n-gram dict scored by the back-off recursion; the device reads the same model through
`write_arpa` and `NGramLM.from_arpa`).  Geometry, weights and the parity rule are those of tests/test_rnnt_beam_gpu.py: tokens,
frames, lengths, n_hyp and order equal the float64 oracle's, every score within max(8 x |float32 oracle - float64 oracle|, 16 ulp);
the conditions on the input are asserted, never skipped: the oracle's decision margin >= 1e-3 (bf16: >= 64 x the float32 / float64
rank drift), and the float64 n-best with the model differs from the one without.  The seed of every case (its last entry; it seeds
the weights and the model) was picked on the CPU as the first of 0, 1, 2, ... that passes them."""
import functools

import numpy as np
import pytest
import torch

import ctc_beam_lm_oracle as L
import rnnt_beam_lm_oracle as O
from test_rnnt_beam_gpu import DUR, LENS, MAX_SYMBOLS, _case as _plain_case, _kept

pytestmark = pytest.mark.gpu
CHAIN = 6   # RB_LM_CHAIN of csrc/rnnt_beam.hip: chains of up to 6 states before state 0 are walked row-wise

# (H, J, V1, W, tdt, bf16, order, alpha, seed); order 0: the model whose chains exceed CHAIN (the per-label fallback)
CASES = [
    (40, 24, 13, 1, False, False, 2, 0.5, 0),
    (64, 64, 13, 3, False, False, 3, 0.5, 0),
    (40, 64, 13, 4, True, False, 3, 0.5, 0),
    (64, 24, 13, 16, False, False, 3, 0.5, 1),
    (64, 64, 1025, 4, True, False, 3, 0.5, 0),   # the BPE width, once: the N tail and a mask tail
    (40, 24, 13, 16, True, True, 3, 0.5, 0),
    (40, 24, 13, 4, False, False, 0, 2.0, 3),
]


def _model(seed, V, order):
    if order:
        return L.make_lm(seed, V, order), order
    ng = L.make_lm(seed, V, 2)   # a run of label 0 is a context of every length up to 8: a chain of 8 states
    for n in range(2, 10):
        ng[(0,) * n] = [-0.02, 0.1 if n < 9 else 0.0]
    return ng, 9


@functools.lru_cache(maxsize=None)
def _case(H, J, V1, W, tdt, bf16, order, alpha, seed):
    m, f, plain = _plain_case(H, J, V1, W, tdt, bf16, 24, seed)
    ng, order = _model(seed, V1 - 1, order)
    run = lambda b, dt: O.beam_search_lm(m, f[b], LENS[b], W, V1 - 1, MAX_SYMBOLS, 24, ng, order, alpha, DUR if tdt else None, dt, bf16)
    return m, f, ng, plain, [(run(b, np.float64), run(b, np.float32)) for b in range(len(LENS))]


def _lm(ng, V, tmp_path):
    from nemo_amd.modules import NGramLM
    L.write_arpa(ng, tmp_path / "lm.arpa")
    return NGramLM.from_arpa(str(tmp_path / "lm.arpa"), V, token_offset=100)


def _device(m, f, W, tdt, bf16, models):
    from nemo_amd import ops
    t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)
    wdt = torch.bfloat16 if bf16 else torch.float32
    H, J = m["emb"].shape[1], m["w_pred"].shape[0]
    args = (t(f), torch.tensor(LENS, dtype=torch.int64, device="cuda"), t(m["emb"]), t(m["w_ih"], wdt), H, t(m["w_hh"], wdt), H,
            t(m["b_ih"]), t(m["b_hh"]), t(m["w_pred"], wdt), H, t(m["b_pred"]), t(m["w_out"], wdt), J, t(m["b_out"]),
            m["emb"].shape[0] - 1, MAX_SYMBOLS, W)
    kw = dict(durations=DUR if tdt else None, max_out=24)
    out = ops.transducer_beam_decode_fused(*args, models, **kw) if models else ops.transducer_beam_decode(*args, **kw)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("H,J,V1,W,tdt,bf16,order,alpha,seed", CASES)
def test_fused_beam_search_matches_the_oracle(H, J, V1, W, tdt, bf16, order, alpha, seed, tmp_path):
    m, f, ng, plain, refs = _case(H, J, V1, W, tdt, bf16, order, alpha, seed)
    assert all(_kept(r64, r32, bf16) for r64, r32 in refs), [r64["margin"] for r64, _ in refs]
    assert any([h[:2] for h in r64["nbest"]] != [h[:2] for h in p64["nbest"]] for (r64, _), (p64, _) in zip(refs, plain))
    depth = max(r64["depth"] for r64, _ in refs)
    assert depth > CHAIN if order == 0 else depth == order - 1 <= CHAIN, depth   # (the longest chain a scored row had)
    tokens, times, out_len, score, n_hyp = _device(m, f, W, tdt, bf16, [(_lm(ng, V1 - 1, tmp_path), alpha)])
    for b, (r64, r32) in enumerate(refs):
        nb = r64["nbest"]
        assert n_hyp[b] == len(nb) and (LENS[b] > 0 or (len(nb) == 1 and nb[0][0] == () and score[b, 0] == 0.0))
        for k, (tok, fr, s64) in enumerate(nb):
            n = out_len[b, k]
            assert n == len(tok) and tuple(tokens[b, k, :n]) == tok and tuple(times[b, k, :n]) == fr, (b, k, tok, tokens[b, k])
            assert (tokens[b, k, n:] == -1).all() and (times[b, k, n:] == -1).all()
            tol = max(8 * abs(r32["nbest"][k][2] - s64), 16 * float(np.spacing(np.float32(abs(s64)))))
            print(f"RNNT_BEAM_LM b={b} k={k} score {score[b, k]:.7g} oracle {s64:.7g} err {abs(score[b, k] - s64):.3e} tol {tol:.3e}")
            assert abs(float(score[b, k]) - s64) <= tol, (b, k, float(score[b, k]), s64, tol)
        assert (tokens[b, len(nb):] == -1).all() and (out_len[b, len(nb):] == 0).all() and np.isneginf(score[b, len(nb):]).all()


@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=["rnnt", "tdt"])
def test_a_zero_weight_gives_the_bits_of_the_plain_search(case, tmp_path):
    H, J, V1, W, tdt, bf16 = case[:6]
    m, f, ng, _, _ = _case(*case)
    fused = _device(m, f, W, tdt, bf16, [(_lm(ng, V1 - 1, tmp_path), 0.0)])
    for a, b in zip(fused, _device(m, f, W, tdt, bf16, None)):
        assert a.dtype == b.dtype and (a.view(np.int32) == b.view(np.int32)).all()


def test_a_model_transcribes_through_the_fused_beam(tmp_path):
    from nemo_amd import ops
    from nemo_amd.models import EncDecRNNTModel
    from test_rnnt_fused_gpu import VOCAB, _model_cfg
    L.write_arpa(L.make_lm(0, len(VOCAB), 3), tmp_path / "lm.arpa")
    cfg = _model_cfg(False, {})
    cfg["decoding"] = dict(strategy="malsd_batch", beam=dict(beam_size=4, return_best_hypothesis=False, max_symbols_per_step=3,
                                                              ngram_lm_arpa=str(tmp_path / "lm.arpa"), ngram_lm_alpha=0.5,
                                                              ngram_lm_token_offset=100))
    torch.manual_seed(4)
    model = EncDecRNNTModel(cfg)
    with torch.no_grad():   # a transducer head that emits labels
        for p in list(model.decoder.parameters()) + list(model.joint.parameters()):
            p.mul_(4.0)
    model = model.to("cuda").eval()
    g = torch.Generator().manual_seed(7)
    waves = [0.1 * torch.randn(32000, generator=g), 0.1 * torch.randn(19200, generator=g)]
    hyps = model.transcribe(waves, batch_size=2, return_hypotheses=True)
    sig = torch.zeros(2, 32000)
    for r, w in enumerate(waves):
        sig[r, : w.numel()] = w
    with torch.no_grad():
        enc, enc_len = model.forward(input_signal=sig.to("cuda"), input_signal_length=torch.tensor([32000, 19200]).to("cuda"))
    infer = model.decoding.decoding
    (lm, alpha), = infer.fusion_models
    f, args = infer._project(enc)
    tk, tm, n, sc, nh = (o.cpu() for o in ops.transducer_beam_decode_fused(f, enc_len.to(torch.int64), *args, 4, [(lm, 0.5)]))
    plain = ops.transducer_beam_decode(f, enc_len.to(torch.int64), *args, 4)[3].cpu()
    print("labels of the kept hypotheses:", n.tolist())
    assert alpha == 0.5 and int(n.sum()) > 0 and not torch.equal(sc, plain)   # labels are emitted, and the model moved the scores
    for b, h in enumerate(hyps):
        assert len(h.n_best) == int(nh[b]) > 1
        for k, alt in enumerate(h.n_best):
            assert alt.y_sequence.tolist() == tk[b, k, :n[b, k]].tolist() and alt.timestamp == tm[b, k, :n[b, k]].tolist()
            assert alt.score == float(sc[b, k]) and alt.text == model.decoding.ids_to_text(alt.y_sequence.tolist())
