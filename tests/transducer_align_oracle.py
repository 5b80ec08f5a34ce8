"""Plain numpy restatement of what `mi355x_transducer_align` computes (include/mi355x_asr.h states the rule), a double loop over
the cells in a given dtype, for tests/test_transducer_align_gpu.py (bit equality with the kernel in float32)."""
import numpy as np


def _arcs(durations):
    """-> (blank arcs, label arcs) as (duration, column of `rows` with its duration term or None), in the rule's tie order"""
    if durations is None:
        return [(1, None)], [(0, None)]
    return [(d, 2 + i) for i, d in enumerate(durations) if d >= 1], [(d, 2 + i) for i, d in enumerate(durations)]


def _w(rows, t, u, col, dcol):
    return rows[t, u, col] if dcol is None else rows[t, u, col] + rows[t, u, dcol]


def viterbi(rows, T, U, durations=None, dtype=np.float32):
    """rows [>= T, >= U + 1, 2 + D] = (lpb, lpl, ld[..]) -> (score, tok_frame, tok_dur); (-inf, None, None) without a path"""
    rows = np.asarray(rows, dtype=dtype)
    none = (dtype(-np.inf), None, None)
    if T == 0:
        return (dtype(0), [], []) if U == 0 else none
    blank, label = _arcs(durations)
    v = np.full((T + 1, U + 1), -np.inf, dtype=dtype)
    bp = {}
    v[0, 0] = 0
    with np.errstate(invalid="ignore"):
        for t in range(T + 1):
            for u in range(U + 1) if t < T else [U]:   # row T: the terminal (T, U) alone, reached by blank arcs only
                if t == 0 and u == 0:
                    continue
                best, arc = dtype(-np.inf), None
                for d, col in blank:
                    if t - d >= 0:
                        cand = v[t - d, u] + _w(rows, t - d, u, 0, col)
                        if cand > best:
                            best, arc = cand, (d, 0)
                for d, col in label if t < T else []:
                    if u > 0 and t - d >= 0:
                        cand = v[t - d, u - 1] + _w(rows, t - d, u - 1, 1, col)
                        if cand > best:
                            best, arc = cand, (d, 1)
                v[t, u], bp[t, u] = best, arc
    if not v[T, U] > -np.inf:
        return none
    frame, dur, t, u = [0] * U, [0] * U, T, U
    while (t, u) != (0, 0):
        d, is_label = bp[t, u]
        t, u = t - d, u - is_label
        if is_label:
            frame[u], dur[u] = t, d
    return v[T, U], frame, dur


def align_batch(rows, act_lens, label_lens, durations=None, dtype=np.float32):
    """-> (tok_frame i32 [B, U1-1], tok_dur i32 [B, U1-1], score [B]), -1 padded as the kernel pads"""
    B, T, U1 = rows.shape[:3]
    frame, dur = np.full((B, U1 - 1), -1, np.int32), np.full((B, U1 - 1), -1, np.int32)
    score = np.zeros(B, dtype)
    for b in range(B):
        Tb, Ub = max(0, min(T, int(act_lens[b]))), max(0, min(U1 - 1, int(label_lens[b])))
        score[b], f, d = viterbi(rows[b], Tb, Ub, durations, dtype)
        if f is not None:
            frame[b, :Ub], dur[b, :Ub] = f, d
    return frame, dur, score


def path_score(rows, frames, T, durations=None, dtype=np.float32):
    """float32 sum, arc by arc, of the alignment that emits label n on frames[n] with duration 0 and moves on by blanks of
    duration 1 (TDT: both durations must be in the set)"""
    rows = np.asarray(rows, dtype=dtype)
    cb, cl = (None, None) if durations is None else (2 + list(durations).index(1), 2 + list(durations).index(0))
    s, u = dtype(0), 0
    for t in range(T):
        while u < len(frames) and frames[u] == t:
            s, u = s + _w(rows, t, u, 1, cl), u + 1
        s = s + _w(rows, t, u, 0, cb)
    assert u == len(frames)
    return s


def rows_ref(acts, labels, V1, D, blank, dtype):
    """acts [T, U1, >= V1 + D] of ONE utterance without padding -> rows [T, U1, 2 + D] in `dtype` (lpl of the last column -inf)"""
    x = np.asarray(acts, dtype=dtype)
    def lsm(z):
        m = z.max(-1, keepdims=True)
        return z - (m + np.log(np.exp(z - m).sum(-1, keepdims=True)))
    lab = lsm(x[..., :V1])
    out = np.full(x.shape[:2] + (2 + D,), -np.inf, dtype=dtype)
    out[..., 0] = lab[..., blank]
    for u, y in enumerate(labels):
        out[:, u, 1] = lab[:, u, y]
    if D:
        out[..., 2:] = lsm(x[..., V1:V1 + D])
    return out
