"""-m gpu: the "saved probabilities" entry points of nemo_amd/csrc/attention.hip (mi355x_relpos_flash_fwd_p, _bwd_dq_p, _bwd_dkv_p)
through the C ABI, in the harness of tests/test_attention_kernels_gpu.py (NaN-prefilled outputs between sentinel guards, float64
oracle of tests/attention_oracle.py, per-element bounds).

  forward with export   ctx, ctx_lo, lse bit-identical to mi355x_relpos_flash_fwd
  exported blocks       p~ * exp(mref * scale - lse) within 2^-8 |ref| of the oracle's probabilities; masked keys exactly 0;
                        key tiles beyond an utterance untouched
  dQ / dK/dV (_p)       the bounds of the recomputing kernels with the `cond` (dS blocks: `A`) factor at 3 * 2^-9 instead of 2^-8
                        (one more bf16 rounding of each probability; tests/test_attention_saved_probs_host.py shows that the
                        documented arithmetic stays below them); padded rows exactly zero; the dS blocks feed the unchanged
                        linear_pos gradient kernel
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_oracle as AO  # noqa: E402
import test_attention_kernels_gpu as K  # noqa: E402
import test_attention_saved_probs_host as SP  # noqa: E402
from test_norm_kernels_gpu import Guarded, assert_intact, bits  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16, F64, I64 = torch.float32, torch.bfloat16, torch.float64, torch.int64
NAN = float("nan")
MI_ERR_ARG = 1
P, lib, stream = K.P, K.lib, K.stream


@pytest.fixture(autouse=True)
def stop_after_a_gpu_error():
    """a launch that failed leaves the device in an unknown state: nothing more of this file is started on it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, no further test is started: {e}", returncode=3)


def run_fwd_p(c, s):
    B, H, T, dk, d = c["B"], c["H"], c["T"], c["dk"], c["d"]
    ctx, lo = Guarded((c["rows"], d), BF16, fill=NAN), Guarded((c["rows"], d), BF16, fill=NAN)
    lse = Guarded((B, H, T), F32, fill=NAN)
    n_p, n_m = lib().mi355x_relpos_probs_elems(B, H, T), lib().mi355x_relpos_mref_elems(B, H, T)
    assert (n_p, n_m) == (SP.probs_elems(B, H, T), SP.mref_elems(B, H, T))
    probs, mref = Guarded(n_p, BF16, fill=NAN), Guarded(n_m, F32, fill=NAN)
    rc = lib().mi355x_relpos_flash_fwd_p(P(s["qkv"]), 3 * d, P(s["pos"]), s["ldp"], P(s["u"]), P(s["v"]), P(s["lens"]), P(ctx), P(lo), d,
                                         P(lse), P(probs), n_p, P(mref), n_m, B, H, T, dk, (T + 7) // 8 * 8, c["scale"],
                                         *K.drop_args(c), None, stream())
    assert rc == 0, rc
    assert_intact(ctx=ctx, ctx_lo=lo, lse=lse, probs=probs, mref=mref)
    return ctx, lo, lse, probs, mref


def run_dq_p(c, s, st):
    B, H, T, dk, d, rows = c["B"], c["H"], c["T"], c["dk"], c["d"], c["rows"]
    o = dict(dqu=Guarded((rows, d), BF16, fill=NAN), dqv=Guarded((rows, d), BF16, fill=NAN), dq3=Guarded((rows, 3 * d), BF16, fill=NAN),
             bg=Guarded(2 * d, F32, src=c["pre_bg"]), ds=Guarded(lib().mi355x_relpos_ds_elems(B, H, T), BF16, fill=NAN))
    n_cs = B * ((T + 127) // 128) * 2 * d
    o["cs"] = Guarded(n_cs, F32, fill=NAN)
    rc = lib().mi355x_relpos_flash_bwd_dq_p(P(st["probs"]), st["probs"].t.numel(), P(st["mref"]), st["mref"].t.numel(), P(s["qkv"]), 3 * d,
                                            P(s["pos"]), s["ldp"], P(s["lens"]), P(s["dO"]), P(st["lse"]), P(st["delta"]), P(o["dqu"]),
                                            P(o["dqv"]), P(o["ds"]), P(o["dq3"]), 3 * d, P(o["bg"]), P(o["cs"]), n_cs, B, H, T, dk,
                                            o["ds"].t.numel(), c["scale"], *K.drop_args(c), None, stream())
    assert rc == 0, rc
    assert_intact(**o)
    return o


def run_dkv_p(c, s, st):
    B, H, T, dk, d = c["B"], c["H"], c["T"], c["dk"], c["d"]
    dqkv = Guarded((c["rows"], 3 * d), BF16, fill=NAN)
    rc = lib().mi355x_relpos_flash_bwd_dkv_p(P(st["probs"]), st["probs"].t.numel(), P(st["mref"]), st["mref"].t.numel(), P(st["qu"]),
                                             P(s["qkv"]), 3 * d, P(s["lens"]), P(s["dO"]), P(st["lse"]), P(st["delta"]), P(dqkv), 3 * d,
                                             B, H, T, dk, c["scale"], *K.drop_args(c), None, stream())
    assert rc == 0, rc
    assert_intact(dqkv=dqkv)
    return dqkv


@functools.lru_cache(maxsize=None)
def solved(T, lens, regime, p):
    """one case: the oracle (shared, never modified), the widened bounds and every kernel's output"""
    c = K.case(SP.B_, SP.H_, T, SP.DK, lens, regime, p)
    bp = SP.bounds_p(c["f"], c["g"])
    Xb, _ = AO.ds_blocks(bp["dS"], lens, T, False)
    s = K.device_inputs(c)
    ctx0, lo0, lse0 = K.run_fwd(c, s)
    ctx, lo, lse, probs, mref = run_fwd_p(c, s)
    delta, qu, qv = K.run_prep(c, s, ctx, lo)
    st = dict(qu=qu, qv=qv, lse=lse, delta=delta, probs=probs, mref=mref)
    return dict(c=c, bp=bp, Xb=Xb, s=s, fwd0=(ctx0, lo0, lse0), fwd=(ctx, lo, lse), st=st, dq=run_dq_p(c, s, st), dqkv=run_dkv_p(c, s, st))


cases = pytest.mark.parametrize("case", SP.CASES, ids=SP.CASE_IDS)


@cases
def test_forward_with_export_is_the_forward_bit_for_bit(case):
    r = solved(*case)
    for n, a, b in zip(("ctx", "ctx_lo", "lse"), r["fwd0"], r["fwd"]):
        assert torch.equal(bits(a.t), bits(b.t)), f"{n} of the exporting forward differs"
    K.check_fwd(r["c"], *r["fwd"])


@cases
def test_exported_blocks_are_the_oracle_probabilities(case):
    T, lens, regime, p = case
    r = solved(*case)
    c, f, B, H = r["c"], r["c"]["f"], SP.B_, SP.H_
    n = SP.nt4(T)
    blocks = r["st"]["probs"].cpu().float().view(B * H, n, n, 64, 16)
    mref = SP.mref_to_dense(r["st"]["mref"].cpu(), B, H, T)
    lse = r["fwd"][2].cpu()
    for b, L in enumerate(c["Ls"]):
        nkt = (L + 31) // 32
        blk = blocks.view(B, H, n, n, 64, 16)[b]
        assert torch.isfinite(blk[:, :, :nkt]).all(), "a block of a key tile with valid keys was not (fully) written"
        assert torch.isnan(blk[:, :, nkt:]).all(), "a block of a key tile beyond the utterance was touched"
        assert torch.isfinite(mref[b, :, :L, :nkt]).all() and torch.isnan(mref[b, :, :, nkt:]).all()
    dense = torch.nan_to_num(SP.blocks_to_dense(blocks, B, H, T), nan=0.0)
    assert dense.max().item() <= 256.0
    Pg = SP.exported_P(dense, torch.nan_to_num(mref, nan=0.0, neginf=-1e30), lse, f["scale"], B, H, T)
    _, pair = AO._valid(lens, T)
    pair = pair.expand(B, H, T, T)
    assert (dense[:, :, :T, :T][~pair & (torch.arange(T)[None, None, :, None] < torch.tensor(c["Ls"])[:, None, None, None])] == 0).all(), \
        "a masked key of a valid query was exported as non-zero"
    Pg = torch.where(pair, Pg, torch.zeros((), dtype=F64))
    K.judge("exported p~ * exp(mref scale - lse)", Pg, f["P"], 2.0 ** -8 * f["P"])


@cases
def test_dq_with_given_probabilities(case):
    r = solved(*case)
    c, g, bp, o, d = r["c"], r["c"]["g"], r["bp"], r["dq"], r["c"]["d"]
    for n in ("dqu", "dqv"):
        K.judge(n, o[n].cpu().float(), g[n], bp[n])
        K.padded_rows_zero(c, n, o[n].cpu().float())
    q3 = o["dq3"].cpu()
    K.judge("dq_out", q3[:, :d].float(), g["dq"], bp["dq"])
    K.padded_rows_zero(c, "dq_out", q3[:, :d].float())
    assert K.nan_bits_kept(q3[:, d:]), "dq_out: the K / V thirds were written"
    pre = c["pre_bg"]
    e9 = 2.0 ** -9
    terms = torch.cat([(3 * e9 * g["cond_dqu"] + g["dterm_dqu"]).sum(0), (3 * e9 * g["cond_dqv"] + g["dterm_dqv"]).sum(0)])
    K.judge("bias_grads", o["bg"].cpu(), pre.double() + g["bias_grads"], AO.TOL_COL * (pre.double().abs() + g["abs_bias_grads"]) + terms)
    X, wr = K.blocks_of(c, o["ds"]).float(), c["written"]
    assert torch.isfinite(X).flatten(-2).all(-1)[wr].all(), "a dS block the linear_pos gradient reads was not (fully) written"
    assert torch.isnan(X).flatten(-2).all(-1)[~wr].all(), "a dS block outside the written set was touched"
    m = wr[..., None, None].expand_as(X)
    K.judge("dS blocks", X[m], c["X"][m], r["Xb"][m])


@cases
def test_dkv_with_given_probabilities(case):
    r = solved(*case)
    c, g, bp, d = r["c"], r["c"]["g"], r["bp"], r["c"]["d"]
    x = r["dqkv"].cpu()
    K.judge("dk", x[:, d:2 * d].float(), g["dk"], bp["dk"])
    K.judge("dv", x[:, 2 * d:].float(), g["dv"], bp["dv"])
    K.padded_rows_zero(c, "dk | dv", x[:, d:].float())
    assert K.nan_bits_kept(x[:, :d]), "dqkv: the Q third was written"


@pytest.mark.parametrize("case", [SP.CASES[2], SP.CASES[8]], ids=[SP.CASE_IDS[2], SP.CASE_IDS[8]])
def test_ds_blocks_feed_the_unchanged_dpos_kernel(case):
    r = solved(*case)
    c = r["c"]
    dpos, dcast = K.run_dpos(c, r["s"], r["st"]["qv"], r["dq"]["ds"])
    K.check_dpos(c, r["dq"]["ds"], dpos, dcast)


def test_two_runs_give_the_same_bits():
    r = solved(*SP.CASES[6])
    c, s, st = r["c"], r["s"], r["st"]
    ctx, lo, lse, probs, mref = run_fwd_p(c, s)
    for n, a, b in (("probs", probs, st["probs"]), ("mref", mref, st["mref"]), ("ctx", ctx, r["fwd"][0]), ("lse", lse, r["fwd"][2])):
        assert torch.equal(bits(a.t), bits(b.t)), f"{n} differs between two runs"
    o, dqkv = run_dq_p(c, s, st), run_dkv_p(c, s, st)
    for n in ("dqu", "dqv", "dq3", "ds"):
        assert torch.equal(bits(o[n].t), bits(r["dq"][n].t)), f"{n} differs between two runs"
    assert torch.equal(bits(dqkv.t), bits(r["dqkv"].t)), "dqkv differs between two runs"


def test_argument_checks():
    """dk = 128, a row-offset table and short buffers return MI_ERR_ARG before anything is launched: outputs stay NaN"""
    L = lib()
    B, H, T = 2, 2, 9
    d = H * 64
    t = lambda *sh, dt=BF16: Guarded(sh, dt, fill=NAN)  # noqa: E731
    qkv, pos, dO, qu = t(B * T, 3 * d), t(2 * T - 1, d), t(B * T, d), t(B * T, d)
    u, v = t(d, dt=F32), t(d, dt=F32)
    lens = torch.tensor([T, 3], dtype=I64, device=K.dev)
    cu = torch.tensor([0, T, T + 3], dtype=I64, device=K.dev)
    ctx, lo, lse, delta = t(B * T, d), t(B * T, d), t(B, H, T, dt=F32), t(B, H, T, dt=F32)
    dqu, dqv, dqkv = t(B * T, d), t(B * T, d), t(B * T, 3 * d)
    n_p, n_m = L.mi355x_relpos_probs_elems(B, H, T), L.mi355x_relpos_mref_elems(B, H, T)
    probs, mref = t(n_p), t(n_m, dt=F32)
    outs = dict(ctx=ctx, lo=lo, lse=lse, dqu=dqu, dqv=dqv, dqkv=dqkv, probs=probs, mref=mref)
    st = stream()

    def fwd(dk=64, cu=None, n_p=n_p, n_m=n_m, probs=P(probs), mref=P(mref)):
        return L.mi355x_relpos_flash_fwd_p(P(qkv), 3 * d, P(pos), d, P(u), P(v), P(lens), P(ctx), P(lo), d, P(lse), probs, n_p, mref, n_m,
                                           B, H, T, dk, 16, 0.125, 0, 0, 1.0, cu, st)

    def dq(dk=64, cu=None, n_p=n_p, n_m=n_m, probs=P(probs), mref=P(mref)):
        return L.mi355x_relpos_flash_bwd_dq_p(probs, n_p, mref, n_m, P(qkv), 3 * d, P(pos), d, P(lens), P(dO), P(lse), P(delta), P(dqu),
                                              P(dqv), None, None, 0, None, None, 0, B, H, T, dk, 0, 0.125, 0, 0, 1.0, cu, st)

    def dkv(dk=64, cu=None, n_p=n_p, n_m=n_m, probs=P(probs), mref=P(mref)):
        return L.mi355x_relpos_flash_bwd_dkv_p(probs, n_p, mref, n_m, P(qu), P(qkv), 3 * d, P(lens), P(dO), P(lse), P(delta), P(dqkv),
                                               3 * d, B, H, T, dk, 0.125, 0, 0, 1.0, cu, st)

    bad = []
    for fn in (fwd, dq, dkv):
        for kw in (dict(dk=128), dict(dk=32), dict(cu=P(cu)), dict(n_p=n_p - 1), dict(n_m=n_m - 1), dict(n_p=0), dict(probs=None),
                   dict(mref=None), dict(probs=P(probs) + 2)):
            rc = fn(**kw)
            if rc != MI_ERR_ARG:
                bad.append((fn.__name__, kw, rc))
    torch.cuda.synchronize()
    assert not bad, bad
    for n, x in outs.items():
        assert K.nan_bits_kept(x.cpu()), f"{n} was written by a rejected call"
    assert_intact(**outs)
    for B_, H_, T_ in ((1, 1, 1), (2, 3, 128), (2, 3, 129), (32, 8, 501)):
        assert L.mi355x_relpos_probs_elems(B_, H_, T_) == SP.probs_elems(B_, H_, T_)
        assert L.mi355x_relpos_mref_elems(B_, H_, T_) == SP.mref_elems(B_, H_, T_)
