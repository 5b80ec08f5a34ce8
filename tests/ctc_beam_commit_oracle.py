"""Restatement of `mi355x_ctc_beam_commit` (include/mi355x_asr.h states it) in numpy, over integers and raw bits: sets and lists
where the kernel walks in lock-step, so the two share the statement and nothing else.

A state is a dict name -> array: the per-beam arrays [B, W] under the names of `CTCBeamStreamState.arrays()` (float32 fields as
float32; they are only ever copied), `nb` and `frames_done` [B].  A window is a dict tok_base, frame_base, kept [B] and frame_map
[B, Tcap].  A tree is int32 [B, Tcap, W, 2]: (parent, token) of node 1 + frame * W + slot."""
import numpy as np

ROOT_HASH = 0x243F6A8885A308D3
EMPTY_INT = dict(node=0, par=-1, tok=-1, len=0, lm_state=1, fs_state=1)
NEG_BITS = np.array([0xFF800000], dtype=np.uint32).view(np.float32)[0]
EMPTY_FLOAT = dict(pb=NEG_BITS, pnb=NEG_BITS, tot=NEG_BITS, brank=NEG_BITS, lm_sum=np.float32(0), fs_sum=np.float32(0))


def fresh_window(B, Tcap):
    z = lambda *s: np.zeros(s, dtype=np.int32)
    return dict(tok_base=z(B), frame_base=z(B), kept=z(B), frame_map=z(B, Tcap))


def _clip(v, lo, hi):
    return int(min(max(int(v), lo), hi))


def commit_one(state, win, tree, b, stable_frames):
    """stream b -> (beams' = {name: list over the W slots}, nb', dict(tok_base, frame_base, kept, frame_map list), tree rows
    [kept', W, 2], committed tokens, committed global frames)"""
    Tcap, W = tree.shape[1], tree.shape[2]
    fd = _clip(state["frames_done"][b], 0, Tcap)
    nb = _clip(state["nb"][b], 0, W)
    kept = _clip(win["kept"][b], 0, fd)
    fbase, tbase = _clip(win["frame_base"][b], 0, 0x3FFFFFFF), _clip(win["tok_base"][b], 0, 0x3FFFFFFF)
    G = fbase + fd - kept
    lim = fd * W
    frame = lambda n: (n - 1) // W
    gf = lambda i: int(win["frame_map"][b, i]) if i < kept else i - kept + fbase

    def parent(n):
        p = int(tree[b, frame(n), (n - 1) % W, 0])
        return p if p > 0 and frame(p) < frame(n) else 0

    def chain(n):   # the node and its ancestors, without the root
        out = []
        while n > 0:
            out.append(n)
            n = parent(n)
        return out

    nodes = [int(state["node"][b, x]) for x in range(nb)]
    nodes = [n if 0 < n <= lim else 0 for n in nodes]
    chains = [chain(n) for n in nodes]
    # 1. forced pruning
    surv = list(range(nb))
    if stable_frames is not None and stable_frames >= 0:
        cut = G - int(stable_frames)
        old = [next((n for n in c if gf(frame(n)) < cut), 0) for c in chains]
        surv = [x for x in range(nb) if old[x] == old[0]]
    # 2. the common ancestor: all common nodes lie on one chain, the deepest has the largest id
    A = 0
    if surv:
        common = set(chains[surv[0]])
        for x in surv[1:]:
            common &= set(chains[x])
        A = max(common) if common else 0
    path = chain(A)[::-1]
    com_tokens = [int(tree[b, frame(n), (n - 1) % W, 1]) for n in path]
    com_frames = [gf(frame(n)) for n in path]
    # 3. re-root and compact
    reach = set()
    for x in surv:
        for n in chains[x]:
            if n == A:
                break
            reach.add(n)
    frames = sorted({frame(n) for n in reach})
    new = {f: i for i, f in enumerate(frames)}

    def remap(p):
        if p == A or p <= 0 or p > lim or frame(p) not in new:
            return 0
        return 1 + new[frame(p)] * W + (p - 1) % W

    rows = np.zeros((len(frames), W, 2), dtype=np.int32)
    rows[:, :, 1] = -1
    for n in reach:
        rows[new[frame(n)], (n - 1) % W] = (remap(parent(n)), int(tree[b, frame(n), (n - 1) % W, 1]))
    beams = {}
    for name, arr in state.items():
        if name in ("nb", "frames_done"):
            continue
        empty = ROOT_HASH if name == "h" else 0 if name == "hp" else EMPTY_INT[name] if name in EMPTY_INT else EMPTY_FLOAT[name]
        col = [arr[b, x] for x in surv] + [arr.dtype.type(empty)] * (W - len(surv))
        beams[name] = np.array(col, dtype=arr.dtype)
    beams["node"] = np.array([remap(nodes[x]) for x in surv] + [0] * (W - len(surv)), dtype=np.int32)
    beams["par"] = np.array([-1 if nodes[x] == A else remap(int(state["par"][b, x])) for x in surv] + [-1] * (W - len(surv)),
                            dtype=np.int32)
    window = dict(tok_base=tbase + len(path), frame_base=G, kept=len(frames), frame_map=[gf(f) for f in frames])
    return beams, len(surv), window, rows, com_tokens, com_frames


def commit(state, win, tree, stable_frames=None):
    """-> (state', window', tree' [B, Tcap, W, 2] with the rows at and beyond kept' zero, committed = [(tokens, frames)] per stream);
    of frame_map' only [:kept'] means anything"""
    B, Tcap, W, _ = tree.shape
    out = {n: np.empty_like(a) for n, a in state.items()}
    wout = fresh_window(B, Tcap)
    tout = np.zeros_like(tree)
    committed = []
    for b in range(B):
        beams, nb, window, rows, ct, cf = commit_one(state, win, tree, b, stable_frames)
        for n, col in beams.items():
            out[n][b] = col
        out["nb"][b], out["frames_done"][b] = nb, window["kept"]
        for n in ("tok_base", "frame_base", "kept"):
            wout[n][b] = window[n]
        wout["frame_map"][b, : window["kept"]] = window["frame_map"]
        tout[b, : window["kept"]] = rows
        committed.append((ct, cf))
    return out, wout, tout, committed
