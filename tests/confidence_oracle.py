"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the confidence measures of greedy CTC / RNN-T / TDT decoding
(include/mi355x_asr.h, MI355X_CONF_*; mi355x_ctc_greedy_decode_conf and the *_greedy_decode*_conf searches).  float64 by default;
the same functions in float32 (`dtype=`) give the tests the reference's own rounding error, from which their tolerance is derived.

For a distribution over V >= 2 classes with natural log-probabilities x_v, p_v = exp(x_v), S = sum_v p_v^alpha and
G = sum_v p_v^alpha x_v (a class with x_v = -inf adds 0 to both), alpha > 0:
    method                 lin                                   exp
    max_prob               (V max p - 1) / (V - 1)               same
    gibbs, alpha = 1       1 + G / ln V                          (V exp(G) - 1) / (V - 1)
    gibbs, alpha != 1      1 + G / (V^(1-alpha) ln V)            (exp(alpha G) - b) / (1 - b),  b = exp(-alpha V^(1-alpha) ln V)
    tsallis, alpha != 1    1 + (1 - S) / (V^(1-alpha) - 1)       (exp((S-1)/(alpha-1)) - b) / (1 - b),  b = exp((V^(1-alpha) - 1)/(alpha-1))
    renyi, alpha != 1      1 + ln S / ((alpha-1) ln V)           (V S^(1/(alpha-1)) - 1) / (V - 1)
tsallis / renyi at alpha == 1 exactly are the gibbs alpha = 1 row.  Nothing is clamped."""
import math
from collections import namedtuple

import numpy as np

# the fields of the reference's ConfidenceMethodConfig (any object with these attributes will do)
Method = namedtuple("Method", "name entropy_type alpha entropy_norm", defaults=("entropy", "tsallis", 0.33, "exp"))


def method_row(cfg) -> str:
    if cfg.name == "max_prob":
        return "max_prob"
    assert cfg.name == "entropy", cfg.name
    return "gibbs" if float(cfg.alpha) == 1.0 else cfg.entropy_type


def constants(V: int, cfg):
    """(ln V, V^(1-alpha), b of the row in use or 0), in double"""
    a, row = float(cfg.alpha), method_row(cfg)
    lnv, vpow, b = math.log(V), float(V) ** (1.0 - a), 0.0
    if a != 1.0 and cfg.entropy_norm == "exp":
        if row == "gibbs":
            b = math.exp(-a * vpow * lnv)
        elif row == "tsallis":
            b = math.exp((vpow - 1.0) / (a - 1.0))
    return lnv, vpow, b


def frame_confidence(logp, cfg, dtype=np.float64):
    """logp [..., V] natural log-probabilities -> confidence [...] of every row, all arithmetic in `dtype`"""
    x = np.asarray(logp).astype(dtype)
    V = x.shape[-1]
    assert V >= 2 and float(cfg.alpha) > 0.0
    a = dtype(cfg.alpha)
    lnv, vpow, b = (dtype(k) for k in constants(V, cfg))
    one, Vf = dtype(1.0), dtype(V)
    row, ex = method_row(cfg), cfg.entropy_norm == "exp"
    assert cfg.entropy_norm in ("lin", "exp")
    finite = x != -np.inf
    xs = np.where(finite, x, dtype(0.0))
    with np.errstate(over="ignore", under="ignore"):
        if row == "max_prob":
            return ((Vf * np.exp(x.max(axis=-1)) - one) / (Vf - one)).astype(dtype)
        pa = np.where(finite, np.exp(a * xs), dtype(0.0)).astype(dtype)
        S = pa.sum(axis=-1, dtype=dtype)
        G = (pa * xs).sum(axis=-1, dtype=dtype)
        if row == "gibbs" and float(cfg.alpha) == 1.0:
            out = (Vf * np.exp(G) - one) / (Vf - one) if ex else one + G / lnv
        elif row == "gibbs":
            out = (np.exp(a * G) - b) / (one - b) if ex else one + G / (vpow * lnv)
        elif row == "tsallis":
            out = (np.exp((S - one) / (a - one)) - b) / (one - b) if ex else one + (one - S) / (vpow - one)
        elif row == "renyi":
            out = (Vf * np.power(S, one / (a - one)) - one) / (Vf - one) if ex else one + np.log(S) / ((a - one) * lnv)
        else:
            raise AssertionError(row)
    return np.asarray(out).astype(dtype)


def aggregate(values, how):
    v = np.asarray(values)
    assert v.size > 0
    return {"mean": np.mean, "min": np.min, "max": np.max, "prod": np.prod}[how](v).astype(v.dtype)


def ctc_fold(labels, blank):
    """plain fold of an arg-max sequence: [(label, first frame, last frame)] of every run of equal non-blank labels"""
    runs, prev = [], blank
    for t, k in enumerate(labels):
        k = int(k)
        if k != blank and k != prev:
            runs.append([k, t, t])
        elif k != blank:
            runs[-1][2] = t
        prev = k
    return [tuple(r) for r in runs]


def ctc_token_ranges(labels, blank, exclude_blank):
    """inclusive frame range behind every token: its own run, or (exclude_blank False) from behind the previous token's run
    (the first token: from frame 0); the frames behind the last token belong to none"""
    out, nxt = [], 0
    for _, s, e in ctc_fold(labels, blank):
        out.append((s if exclude_blank else nxt, e))
        nxt = e + 1
    return out


def ctc_token_confidence(labels, frame_conf, blank, exclude_blank, how):
    """labels = the arg-max label of every valid frame, frame_conf their confidences -> one confidence per token"""
    fc = np.asarray(frame_conf)
    return np.array([aggregate(fc[lo:hi + 1], how) for lo, hi in ctc_token_ranges(labels, blank, exclude_blank)], dtype=fc.dtype)


def replay_transducer_confidence(Pd, Pj, f, tokens, times, blank, cfg, n_dur=0, dtype=None):
    """Walk ONE utterance along given tokens and (global) frame indices: the start-of-sequence prediction step, then per label the
    logits at times[i], the confidence of the label logits (the last n_dur rows of the output layer are duration logits and take
    no part), the prediction step on tokens[i].  f [T, J] = the utterance's rows of the encoder projection.  All arithmetic in
    `dtype` (torch.float64 by default; torch.float32 gives the reference's own rounding error).  -> numpy array, one value per label"""
    import torch
    import torch.nn.functional as F
    from stream_decode_oracle import _pred, _weights
    dtype = torch.float64 if dtype is None else dtype
    npdt = np.float64 if dtype == torch.float64 else np.float32
    Pd = {k: v.to(dtype) for k, v in Pd.items()}
    Pj = {k: v.to(dtype) for k, v in Pj.items()}
    f = f.to(dtype)
    _, _, w_hh, _, _, w_out, b_out = _weights(Pd, Pj)
    H = w_hh.shape[1]
    V1 = w_out.shape[0] - n_dur
    h, c = torch.zeros(H, dtype=dtype), torch.zeros(H, dtype=dtype)
    gp, hn, cn = _pred(Pd, Pj, blank, h, c)
    out = []
    for k, t in zip(tokens, times):
        z = F.linear(torch.relu(f[int(t)] + gp), w_out, b_out)
        logp = torch.log_softmax(z[:V1], 0)
        out.append(frame_confidence(logp.numpy(), cfg, dtype=npdt))
        h, c = hn, cn
        gp, hn, cn = _pred(Pd, Pj, int(k), h, c)
    return np.array(out, dtype=npdt)
