"""float32 numpy restatement of what `mi355x_ctc_align` and `mi355x_ctc_greedy_decode_ts` compute (include/mi355x_asr.h), for
tests/test_ctc_align_host.py (against brute force) and tests/test_ctc_align_gpu.py (bit equality with the kernels).

Viterbi over the blank-extended sequence (S = 2U+1 states), plain float32, natural log:
    v[0][0] = e(0,0), v[0][1] = e(0,1), the rest -inf
    v[t][s] = max(v[t-1][s], v[t-1][s-1], v[t-1][s-2] if allowed) + e(t,s)
the skip allowed only into a label state whose label differs from the one two states back.  Ties: the first maximum in the order
(stay, s-1, s-2); at the last frame state S-1 unless v[S-2] > v[S-1] strictly.  A best score of -inf (too few frames, no frames for
a non-empty target, or -inf emissions on every path) is infeasible: score -inf, no path.  T = 0 and U = 0: score 0, empty path.
One max and one add per state and step, so a float32 machine that follows the same rules produces the same bits."""
import itertools

import numpy as np

NEG = np.float32(-np.inf)


def viterbi(logp, target, blank):
    """logp f32 [T, C], target: U ids -> (score f32, path: T states or None when infeasible, tok_start [U], tok_end [U])"""
    logp = np.asarray(logp, dtype=np.float32)
    T, U = logp.shape[0], len(target)
    S = 2 * U + 1
    none = (NEG, None, [-1] * U, [-1] * U)
    if T == 0:
        return (np.float32(0.0), [], [], []) if U == 0 else none
    ext = np.full(S, blank, dtype=np.int64)
    ext[1::2] = np.asarray(target, dtype=np.int64)
    allow = np.zeros(S, dtype=bool)
    allow[3::2] = ext[3::2] != ext[1:-2:2]
    v = np.full(S, NEG, dtype=np.float32)
    v[0] = logp[0, blank]
    if U > 0:
        v[1] = logp[0, ext[1]]
    bp = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        s1 = np.concatenate(([NEG], v[:-1])).astype(np.float32)
        s2 = np.where(allow, np.concatenate(([NEG, NEG], v[:-2]))[:S], NEG).astype(np.float32)
        m, k = v.copy(), np.zeros(S, dtype=np.int8)
        up = s1 > m
        m[up], k[up] = s1[up], 1
        up = s2 > m
        m[up], k[up] = s2[up], 2
        v = (m + logp[t, ext]).astype(np.float32)
        bp[t] = k
    s = S - 1
    if S > 1 and v[S - 2] > v[S - 1]:
        s = S - 2
    score = v[s]
    if score == NEG:
        return none
    path = [0] * T
    path[T - 1] = s
    for t in range(T - 1, 0, -1):
        s -= int(bp[t, s])
        path[t - 1] = s
    start, end = [-1] * U, [-1] * U
    for t, s in enumerate(path):
        if s & 1:
            if start[s >> 1] < 0:
                start[s >> 1] = t
            end[s >> 1] = t
    return score, path, start, end


def align_batch(logp, targets, in_len, tgt_len, blank):
    """the kernel's outputs: (path i32 [B,Tmax], tok_start i32 [B,Umax], tok_end i32 [B,Umax], score f32 [B]), -1 padded"""
    logp = np.asarray(logp, dtype=np.float32)
    B, Tmax, _ = logp.shape
    Umax = targets.shape[1]
    path = np.full((B, Tmax), -1, dtype=np.int32)
    ts, te = np.full((B, Umax), -1, dtype=np.int32), np.full((B, Umax), -1, dtype=np.int32)
    score = np.zeros(B, dtype=np.float32)
    for b in range(B):
        T, U = max(0, min(Tmax, int(in_len[b]))), max(0, min(Umax, int(tgt_len[b])))
        sc, p, s, e = viterbi(logp[b, :T], [int(x) for x in targets[b, :U]], blank)
        score[b] = sc
        if p is not None:
            path[b, :T], ts[b, :U], te[b, :U] = p, s, e
    return path, ts, te, score


def path_valid(path, target, T):
    """a frame-to-state path of the blank-extended target: starts in state 0 / 1, ends in S-1 / S-2, moves by 0, 1, or 2 (the
    latter only between different labels)"""
    S = 2 * len(target) + 1
    if len(path) != T or T == 0:
        return len(path) == T and len(target) == 0
    if path[0] not in (0, 1) or path[-1] not in (S - 1, S - 2) or min(path) < 0 or max(path) >= S:
        return False
    for a, b in zip(path, path[1:]):
        if b - a not in (0, 1, 2):
            return False
        if b - a == 2 and not (b & 1 and target[b >> 1] != target[(b >> 1) - 1]):
            return False
    return True


def path_score(logp, path, target, blank):
    """float32, summed frame by frame in time order (what the recursion adds up along one path)"""
    sc = None
    for t, s in enumerate(path):
        e = np.float32(logp[t, target[s >> 1] if s & 1 else blank])
        sc = e if sc is None else np.float32(sc + e)
    return np.float32(0.0) if sc is None else sc


def brute_force(logp, target, blank):
    """every frame-to-state path -> (best score or None when there is no path, the set of paths that attain it)"""
    T, S = logp.shape[0], 2 * len(target) + 1
    best, arg = None, []
    for path in itertools.product(range(S), repeat=T):
        if not path_valid(list(path), target, T):
            continue
        sc = path_score(logp, path, target, blank)
        if best is None or sc > best:
            best, arg = sc, [path]
        elif sc == best:
            arg.append(path)
    return best, arg


def feasible_by_length(T, target):
    """T >= U + the number of adjacent repeated labels (and at least one frame for a non-empty target)"""
    rep = sum(1 for a, b in zip(target, target[1:]) if a == b)
    return T >= len(target) + rep and (T > 0 or len(target) == 0)


def greedy_ts(logp, lens, blank):
    """per utterance (tokens, start frames, end frames): arg-max per frame (first maximum), runs of equal labels folded, blanks
    dropped; start / end = first / last frame of the run behind each token"""
    out = []
    logp = np.asarray(logp, dtype=np.float32)
    for b in range(logp.shape[0]):
        T = int(lens[b]) if lens is not None else logp.shape[1]
        lab = logp[b, :T].argmax(-1) if T else np.zeros(0, dtype=np.int64)
        tok, st, en = [], [], []
        for t in range(T):
            if lab[t] != blank and (t == 0 or lab[t] != lab[t - 1]):
                tok.append(int(lab[t])); st.append(t); en.append(t)
            elif lab[t] != blank:
                en[-1] = t
        out.append((tok, st, en))
    return out


# ---------------------------------------------------------------------------------------------- offsets, written out by hand
# (tokens, start frames, end frames (inclusive), word_pieces) -> (char offsets, word offsets); end_offset is exclusive
def _c(ch, s, e):
    return {"char": ch, "start_offset": s, "end_offset": e}


def _w(w, s, e):
    return {"word": w, "start_offset": s, "end_offset": e}


OFFSET_CASES = {
    "word_pieces": ((["▁he", "llo", "▁", "wor", "ld", "▁a"], [1, 3, 7, 8, 9, 14], [2, 5, 7, 8, 12, 14], True),
                    ([_c("▁he", 1, 3), _c("llo", 3, 6), _c("▁", 7, 8), _c("wor", 8, 9), _c("ld", 9, 13), _c("▁a", 14, 15)],
                     [_w("hello", 1, 6), _w("world", 7, 13), _w("a", 14, 15)])),
    "word_pieces_no_leading_mark": ((["ab", "c", "▁d"], [0, 2, 5], [1, 2, 5], True),
                                    ([_c("ab", 0, 2), _c("c", 2, 3), _c("▁d", 5, 6)], [_w("abc", 0, 3), _w("d", 5, 6)])),
    "chars": ((["h", "i", " ", "y", "o", "u"], [0, 2, 3, 5, 6, 9], [1, 2, 4, 5, 8, 9], False),
              ([_c("h", 0, 2), _c("i", 2, 3), _c(" ", 3, 5), _c("y", 5, 6), _c("o", 6, 9), _c("u", 9, 10)],
               [_w("hi", 0, 3), _w("you", 5, 10)])),
    "chars_leading_and_double_space": (([" ", "a", " ", " ", "b", "c", " "], [0, 1, 2, 4, 6, 7, 9], [0, 1, 3, 5, 6, 8, 9], False),
                                       ([_c(" ", 0, 1), _c("a", 1, 2), _c(" ", 2, 4), _c(" ", 4, 6), _c("b", 6, 7), _c("c", 7, 9),
                                         _c(" ", 9, 10)], [_w("a", 1, 2), _w("bc", 6, 9)])),
    "empty": (([], [], [], False), ([], [])),
    "empty_word_pieces": (([], [], [], True), ([], [])),
}
