"""float64 reference for nemo_amd/csrc/elementwise.hip (dropout-scale-cast, packed rows, q + bias, add2, rel-pos softmax forward /
backward, row scale, rectangle fill) and nemo_amd/csrc/optim.hip (AdamW step, clip coefficient, weight-image pack).

Closed forms in plain torch / numpy on the CPU, no autograd.  Operands arrive in their storage dtype and are up-cast, so a bf16
operand is the bf16-rounded value: a kernel is then judged on its own arithmetic only.  tests/test_elementwise_host.py pins these
closed forms to torch.autograd / torch.optim in float64, and uses the path predicates at the end of this file to prove that the
case tables of the two GPU files reach every kernel path.
"""
import math

import numpy as np
import torch

F64 = torch.float64


def _f64(t):
    return t.detach().to("cpu").to(F64)


def f32(x):
    """a Python float rounded to float32 -- what a kernel receives for a `float` argument"""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ dropout mask
class Drop:
    """(key, threshold, scale) of nemo_amd.ops.Dropout, restated so that nothing here needs the library"""

    def __init__(self, p=0.0, seed=0, site=0):
        if p <= 0.0:
            self.key, self.threshold, self.scale = 0, 0, 1.0
        else:
            self.key = (seed * 0x9E3779B1 + site * 0x85EBCA77 + 0x1234567) & 0xFFFFFFFF
            self.threshold = max(1, min(0xFFFFFFFF, int(p * 4294967296.0)))
            self.scale = 1.0 / (1.0 - p)


def _mix32(x):
    x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x7feb352d); x = x ^ (x >> np.uint32(15)); x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def keep_mask(drop, start, n, step_word=0):
    """drop_mask() of common.h for the n linear indices start, start + 1, ... (modulo 2^32): bool [n], True = kept.  Index idx
    belongs to hash group idx >> 3 and is kept iff output (idx & 7) + 1 of the xorshift32 stream seeded by the group's hash is
    >= threshold.  step_word: the registered device step word, which every dropout kernel adds to its key at entry."""
    if drop.threshold == 0:
        return torch.ones(n, dtype=torch.bool)
    key = (drop.key + step_word) & 0xFFFFFFFF
    idx = ((np.arange(n, dtype=np.uint64) + np.uint64(start & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    grp, e = idx >> np.uint32(3), idx & np.uint32(7)
    with np.errstate(over="ignore"):
        s = _mix32(_mix32(grp ^ np.uint32(key)) + np.uint32((0x9E3779B9 * (key | 1)) & 0xFFFFFFFF)) | np.uint32(1)
        keep = np.zeros(n, dtype=bool)
        for j in range(8):
            s = s ^ (s << np.uint32(13)); s = s ^ (s >> np.uint32(17)); s = s ^ (s << np.uint32(5))
            keep = np.where(e == j, s >= np.uint32(drop.threshold), keep)
    return torch.from_numpy(keep)


# ------------------------------------------------------------------------------------------------ simple element-wise kernels
def drop_scale_cast(x, alpha, keep, p):
    """alpha * keep / (1 - p) * x over the flat input"""
    return _f64(x).flatten() * alpha * keep.to(F64) / (1.0 - p)


def add(a, b):
    return _f64(a) + _f64(b)


def round_to(x64, dtype):
    """round_out(round_f32(x)): one float32 operation is correctly rounded, so the float64 value determines the kernel's result.
    (float64 -> float32 -> bf16 each round to nearest even, as the hardware add and pack_bf2 do.  The float64 sum of two float32
    values is itself exact unless their exponents lie more than 29 apart, which the tests' operands never do.)"""
    return x64.to(torch.float32).to(dtype)


def rows_pack(x, lens, T, width):
    """padded grid x [B*T, >= width] -> packed [sum_b min(T, lens[b]), width]: the valid frames of every utterance back to back"""
    rows = [b * T + t for b, L in enumerate(lens) for t in range(min(T, L))]
    return x[rows, :width] if rows else x[:0, :width]


def rows_unpack(packed, lens, T, width):
    """packed [sum L, >= width] -> padded grid [B*T, width], zero rows beyond each utterance"""
    out = torch.zeros(len(lens) * T, width, dtype=packed.dtype)
    r = 0
    for b, L in enumerate(lens):
        L = min(T, L)
        out[b * T:b * T + L] = packed[r:r + L, :width]
        r += L
    return out


def row_offsets(lens, T):
    """cu[b] = first packed row of utterance b, cu[B] = the number of packed rows"""
    cu = [0]
    for L in lens:
        cu.append(cu[-1] + min(T, L))
    return cu


def fill_rects(x, rects, value):
    """x[b, f0:f1, t0:t1] = value, every rectangle clipped to the tensor, a rectangle whose b is out of range ignored"""
    x = x.clone()
    B, F, T = x.shape
    for b, f0, f1, t0, t1 in rects:
        if 0 <= b < B:
            x[b, max(f0, 0):max(min(f1, F), 0), max(t0, 0):max(min(t1, T), 0)] = value
    return x


# ------------------------------------------------------------------------------------------------ rel-pos softmax
def ctx_allows(style, left, right, T):
    """[T, T] bool, True = query i may see key j; style 0 none / 1 'regular' / 2 'chunked_limited'"""
    i, j = torch.arange(T)[:, None], torch.arange(T)[None]
    ok = torch.ones(T, T, dtype=torch.bool)
    if style == 1 or (style == 2 and right < 0):
        if left >= 0:
            ok &= (j - i) >= -left
        if right >= 0:
            ok &= (j - i) <= right
    elif style == 2:
        chunk = right + 1
        dc = i // chunk - j // chunk
        ok &= (dc >= 0) & (dc <= (left // chunk if left >= 0 else 10000))
    return ok


def relpos_allowed(lens, B, T, ctx=(0, -1, -1)):
    """[B, T, T] bool: row and key inside the utterance (L = min(T, lens[b])) and key inside the context window"""
    L = torch.tensor([min(T, int(l)) for l in lens])
    valid = torch.arange(T)[None] < L[:, None]
    return valid[:, :, None] & valid[:, None, :] & ctx_allows(*ctx, T)[None]


def relpos_softmax_fwd(ac, bdf, lens, T, scale, ctx=(0, -1, -1)):
    """ac [H,B,T,>=T], bdf [H,B,T,>=2T-1] -> s [H,B,T,T]: scores (ac[..., j] + bdf[..., T-1+j-i]) * scale, masked entries -10000,
    softmax over j, masked entries 0"""
    ac, bdf = _f64(ac)[..., :T], _f64(bdf)
    B = ac.shape[1]
    i, j = torch.arange(T)[:, None], torch.arange(T)[None]
    idx = (T - 1 + j - i).expand(ac.shape)
    sc = (ac + torch.gather(bdf, -1, idx)) * scale
    ok = relpos_allowed(lens, B, T, ctx)[None]
    sc = torch.where(ok, sc, torch.tensor(-10000.0, dtype=F64))
    sc = sc - sc.amax(-1, keepdim=True)
    e = sc.exp()
    return torch.where(ok, e / e.sum(-1, keepdim=True), torch.tensor(0.0, dtype=F64))


def relpos_softmax_bwd(dpd, s, T, Pp, scale, keep=None, p=0.0):
    """dpd [H,B,T,>=T] (gradient of dropout(s)), s [H,B,T,>=T] (the saved forward output, an input), keep [H,B,T,T] bool or None
    -> dscore [H,B,T,T] = s * (dp - sum_j s * dp) * scale with dp = dpd * keep / (1 - p), and dbdf [H,B,T,Pp] with
    dbdf[..., i, T-1-i+j] = dscore[..., i, j], zero elsewhere"""
    dp, s = _f64(dpd)[..., :T], _f64(s)[..., :T]
    if keep is not None:
        dp = dp * keep.to(F64) / (1.0 - p)
    ds = s * (dp - (s * dp).sum(-1, keepdim=True)) * scale
    i, j = torch.arange(T)[:, None], torch.arange(T)[None]
    dbdf = torch.zeros(*ds.shape[:3], Pp, dtype=F64)
    dbdf.scatter_(-1, (T - 1 - i + j).expand(ds.shape), ds)
    return ds, dbdf


# ------------------------------------------------------------------------------------------------ optimizer
def bias_corrections(beta1, beta2, step):
    """(1 - beta1^step, sqrt(1 - beta2^step)) in float64 from the float32-rounded betas"""
    return 1.0 - f32(beta1) ** step, math.sqrt(1.0 - f32(beta2) ** step)


def clip_coef(sums, scale, max_norm):
    """(coefficient, norm) of torch.nn.utils.clip_grad_norm_ from the per-buffer sums of squares"""
    norm = scale * math.sqrt(float(sum(float(s) for s in sums)))
    return min(1.0, max_norm / (norm + 1e-6)), norm


def adamw_step(p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale=1.0, clip=None, ema=None, ema_decay=0.0):
    """one AdamW step with decoupled weight decay in float64; the scalars are the float32 values the kernel receives.
    Returns (p, m, v, ema or None)."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    lr, b1, b2, eps, wd = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(wd)
    gs = f32(grad_scale) * (float(clip) if clip is not None else 1.0)
    bc1, bc2s = bias_corrections(beta1, beta2, step)
    gr = g * gs
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * gr
    v = b2 * v + (1.0 - b2) * gr * gr
    p = p - (lr / bc1) * (m / (v.sqrt() / bc2s + eps))
    if ema is not None:
        d = f32(ema_decay)
        ema = _f64(ema) * d + (1.0 - d) * p
    return p, m, v, ema


def pack_image(src, rows, cols, nr2=1, nc2=1, sr1=0, sr2=0, sc1=0, sc2=0):
    """dst[r, c] = src.flat[r1*sr1 + r2*sr2 + c1*sc1 + c2*sc2], r = r1*nr2 + r2, c = c1*nc2 + c2"""
    r, c = torch.arange(rows), torch.arange(cols)
    idx = ((r // nr2) * sr1 + (r % nr2) * sr2)[:, None] + ((c // nc2) * sc1 + (c % nc2) * sc2)[None]
    return src.detach().cpu().reshape(-1)[idx]


# ------------------------------------------------------------------------------------------------ path predicates
PK_T = 64
PACK_PATHS = ("vec_colfast", "vec_rowfast", "scalar_plain", "scalar_split")


def pack_tiles(rows, cols):
    """the (tile row, tile column) pairs of one entry, in launch order"""
    tiles_c = (cols + PK_T - 1) // PK_T
    return [(t // tiles_c, t % tiles_c) for t in range(((rows + PK_T - 1) // PK_T) * tiles_c)]


def pack_path(entry, tile):
    """which branch of pack_kernel loads tile (tr, tc) of an entry -- a dict with rows, cols, nr2, nc2, sr1, sc1, sc2 and src_addr
    (the address of the source modulo 16 is what matters).  Restated from the conditions of optim.hip."""
    tr, tc = tile
    col_fast = (entry["sc2"] == 1 and entry["nc2"] > 1) or (entry["nc2"] == 1 and entry["sc1"] == 1)
    plain = entry["nr2"] == 1 and entry["nc2"] == 1
    fast_stride, slow_stride = (entry["sc1"], entry["sr1"]) if col_fast else (entry["sr1"], entry["sc1"])
    fast_n = entry["cols"] if col_fast else entry["rows"]
    f0 = (tc if col_fast else tr) * PK_T
    if plain and fast_stride == 1 and slow_stride % 4 == 0 and entry["src_addr"] % 16 == 0 and f0 + PK_T <= fast_n:
        return "vec_colfast" if col_fast else "vec_rowfast"
    return "scalar_plain" if plain else "scalar_split"


def add2_colsum_shape(d):
    """(CP column groups of 8 per pass, RS row lanes, idle threads of the 256, column passes) of add2_colsum_kernel"""
    CP = min(d // 8, 256)
    RS = 256 // CP
    return CP, RS, 256 - CP * RS, (d + CP * 8 - 1) // (CP * 8)


def strides(n_vectors, cap):
    """trips of a grid-stride loop over n_vectors items, 256 threads per block, the grid capped at `cap` blocks"""
    blocks = max(1, min(cap, (n_vectors + 255) // 256))
    return (n_vectors + blocks * 256 - 1) // (blocks * 256)


GRID_CAP = {"elementwise": 4096, "adamw": 8192, "sumsq": 2048, "fill_f32": 8192}
