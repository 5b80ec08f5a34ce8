"""-m gpu: `ops.transducer_beam_decode` (csrc/rnnt_beam.hip) against the float64 oracle of its rule (tests/rnnt_beam_oracle.py).

Parity rule, as for the CTC beam search: float32 sums cannot reproduce a float64 selection through a near-tie, so a case needs the
oracle's decision margin >= 1e-3 and, with bf16 operands, >= 64 x the largest rank difference between the float32 and the float64
oracle on that case -- a condition on the input, computed from the references alone and ASSERTED (no case is skipped).  The seed of
every case was picked on the CPU as the first of 0, 1, 2, ... whose three utterances pass that condition (and, where the case
says so, show a merge / reach max_out / beat the greedy search); it is the last entry of the case.  Seed 0 passes in every case
(the smallest margin is 1.07e-3, at H = J = 64, W = 3).
Tokens, frames, lengths, n_hyp and the best-first order equal the float64 oracle's; every score is within
max(8 x |float32 oracle - float64 oracle|, 16 ulp) of it."""
import functools

import numpy as np
import pytest
import torch

import rnnt_beam_oracle as O

pytestmark = pytest.mark.gpu
MARGIN, T, LENS, MAX_SYMBOLS, DUR = 1e-3, 12, (12, 7, 0), 2, [0, 1, 2, 4]

# (H, J, V1, W, tdt, bf16, max_out, seed): H = 40 / J = 24 leave a K tail behind (or instead of) a full MFMA block, V1 = 13 an N tail
CASES = [
    (40, 24, 13, 1, False, False, 24, 0),
    (40, 24, 13, 1, True, False, 24, 0),
    (64, 64, 13, 3, False, False, 24, 0),
    (40, 64, 13, 4, True, False, 24, 0),
    (64, 24, 13, 16, False, False, 24, 0),
    (40, 24, 13, 3, False, False, 3, 0),      # max_out is reached: blank-only candidates
    (64, 64, 1025, 4, True, False, 24, 0),    # BPE width, once
    (64, 64, 13, 4, False, True, 24, 0),
    (40, 24, 13, 16, True, True, 24, 0),
]


@functools.lru_cache(maxsize=None)
def _case(H, J, V1, W, tdt, bf16, max_out, seed):
    """(model, enc_proj [B, T, J], per utterance (float64 result, float32 result)); blank = V1 - 1"""
    rng = np.random.default_rng(seed)
    g = lambda *s, k=1.0: (rng.standard_normal(s) * k).astype(np.float32)
    N = V1 + (len(DUR) if tdt else 0)
    m = dict(emb=g(V1, H), w_ih=g(4 * H, H, k=H ** -0.5), w_hh=g(4 * H, H, k=H ** -0.5), b_ih=g(4 * H, k=0.1), b_hh=g(4 * H, k=0.1),
             w_pred=g(J, H, k=2 * H ** -0.5), b_pred=g(J, k=0.1), w_out=g(N, J, k=3 * J ** -0.5), b_out=g(N, k=0.1))
    if bf16:   # the weight images hold bf16 values
        m.update({k: O.bf16_round(m[k]) for k in ("w_ih", "w_hh", "w_pred", "w_out")})
    f = g(len(LENS), T, J)
    run = lambda b, dt: O.beam_search(m, f[b], LENS[b], W, V1 - 1, MAX_SYMBOLS, max_out, DUR if tdt else None, dt, bf16)
    return m, f, [(run(b, np.float64), run(b, np.float32)) for b in range(len(LENS))]


def _kept(r64, r32, bf16):
    same = len(r64["ranks"]) == len(r32["ranks"])
    drift = max((abs(a - b) for a, b in zip(r64["ranks"], r32["ranks"])), default=0.0) if same else np.inf
    return r64["margin"] >= MARGIN and (not bf16 or r64["margin"] >= 64 * drift)


def _device(m, f, W, tdt, bf16, max_out, greedy=False):
    from nemo_amd import ops
    t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)
    wdt = torch.bfloat16 if bf16 else torch.float32
    H, J = m["emb"].shape[1], m["w_pred"].shape[0]
    args = (t(f), torch.tensor(LENS, dtype=torch.int64, device="cuda"), t(m["emb"]), t(m["w_ih"], wdt), H, t(m["w_hh"], wdt), H,
            t(m["b_ih"]), t(m["b_hh"]), t(m["w_pred"], wdt), H, t(m["b_pred"]), t(m["w_out"], wdt), J, t(m["b_out"]), m["emb"].shape[0] - 1)
    if greedy:
        out = (ops.tdt_greedy_decode(*args, DUR, MAX_SYMBOLS, max_out) if tdt else ops.rnnt_greedy_decode(*args, MAX_SYMBOLS, max_out))
    else:
        out = ops.transducer_beam_decode(*args, MAX_SYMBOLS, W, durations=DUR if tdt else None, max_out=max_out)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("H,J,V1,W,tdt,bf16,max_out,seed", CASES)
def test_beam_search_matches_the_oracle(H, J, V1, W, tdt, bf16, max_out, seed):
    m, f, refs = _case(H, J, V1, W, tdt, bf16, max_out, seed)
    assert all(_kept(r64, r32, bf16) for r64, r32 in refs), [r64["margin"] for r64, _ in refs]
    assert any(len(tok) for tok, _, _ in refs[0][0]["nbest"])   # labels are emitted
    if max_out == 3:
        assert any(len(tok) == 3 for tok, _, _ in refs[0][0]["nbest"])
    if W == 3 and not tdt and max_out > 3:
        assert refs[0][0]["merges"] > 0   # this case shows a merge: its scores are logaddexp sums
    tokens, times, out_len, score, n_hyp = _device(m, f, W, tdt, bf16, max_out)
    assert tokens.shape == times.shape == (len(LENS), W, max_out) and score.shape == out_len.shape == (len(LENS), W)
    for b, (r64, r32) in enumerate(refs):
        nb = r64["nbest"]
        assert n_hyp[b] == len(nb) and (LENS[b] > 0 or (len(nb) == 1 and nb[0][0] == () and score[b, 0] == 0.0))
        for k, (tok, fr, s64) in enumerate(nb):
            n = out_len[b, k]
            assert n == len(tok) and tuple(tokens[b, k, :n]) == tok and tuple(times[b, k, :n]) == fr, (b, k, tok, tokens[b, k])
            assert (tokens[b, k, n:] == -1).all() and (times[b, k, n:] == -1).all()
            tol = max(8 * abs(r32["nbest"][k][2] - s64), 16 * float(np.spacing(np.float32(abs(s64)))))
            print(f"RNNT_BEAM b={b} k={k} score {score[b, k]:.7g} oracle {s64:.7g} err {abs(score[b, k] - s64):.3e} tol {tol:.3e}")
            assert abs(float(score[b, k]) - s64) <= tol, (b, k, float(score[b, k]), s64, tol)
        assert (tokens[b, len(nb):] == -1).all() and (out_len[b, len(nb):] == 0).all() and np.isneginf(score[b, len(nb):]).all()


@pytest.mark.parametrize("case", CASES[:2], ids=["rnnt", "tdt"])
def test_beam_of_one_takes_the_greedy_decisions(case):
    m, f, _ = _case(*case)
    tokens, times, out_len, _, _ = _device(m, f, 1, case[4], False, 24)
    g_tokens, g_times, g_len, _ = _device(m, f, 1, case[4], False, 24, greedy=True)
    assert (out_len[:, 0] == g_len).all() and (tokens[:, 0] == g_tokens).all() and (times[:, 0] == g_times).all()


def test_the_beam_finds_a_better_hypothesis_than_the_greedy_search():
    case = (64, 64, 13, 4, False, False, 24, 0)   # seed: the first whose W = 4 best differs from the W = 1 result in utterance 0
    m, f, refs = _case(*case)
    one = _case(*case[:3], 1, *case[4:])[2][0][0]["nbest"][0]
    assert all(_kept(r64, r32, False) for r64, r32 in refs) and refs[0][0]["nbest"][0][0] != one[0]
    tokens, _, out_len, score, _ = _device(m, f, 4, False, False, 24)
    g_tokens, _, g_len, _ = _device(m, f, 1, False, False, 24, greedy=True)
    best, greedy = tuple(tokens[0, 0, :out_len[0, 0]]), tuple(g_tokens[0, :g_len[0]])
    assert best == refs[0][0]["nbest"][0][0] and greedy == one[0] and best != greedy
    assert score[0, 0] > one[2]   # (the greedy path's score under the beam's rule, blanks counted: the W = 1 oracle)
