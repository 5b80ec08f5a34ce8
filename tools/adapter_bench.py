"""Times the fused linear-adapter kernels (csrc/adapter.hip) against the same math through the existing ops -- LayerNorm, ops.gemm,
an elementwise Swish, ops.gemm and their backward -- alternating the two in one process (profiles/adapter.md).

    python tools/adapter_bench.py [--rows 16000] [--d 512] [--reps 30]
    python tools/adapter_bench.py --step [--dim 32] [--steps 10] [--rounds 4]

--step times bench.py's workload (Conformer-CTC-Large, bf16, 32 x 20 s) three ways, alternated in one process: the model as it is,
the same model with an adapter in every layer and everything trained, and with the base frozen and only the adapters trained.

The "plain" backward allocates its torch temporaries (the bf16 copy of dy, the Swish gradient) per call, which the encoder's own
unfused path would not; and every candidate re-uses one x / dy pair, which at 32 MB each stays in the 256 MB last-level cache across
the back-to-back repetitions.  Both favour small absolute times; read the ratios with that in mind."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nemo_amd import ops  # noqa: E402

dev = "cuda"


def timed(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) * 1e3 for a, b in ev)


def case(M, d, dim, cdt, reps):
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    x, dy, gam, bet = r(M, d), r(M, d), 1 + 0.1 * r(d), 0.1 * r(d)
    wd32, wu32 = r(dim, d) / d ** 0.5, r(d, dim) / dim ** 0.5
    wd, wu = wd32.to(cdt), wu32.to(cdt)
    wdt, wut = wd.t().contiguous(), wu.t().contiguous()
    y, dx = torch.empty_like(x), torch.empty_like(x)
    grads = [torch.zeros(dim, d, device=dev), torch.zeros(d, dim, device=dev), torch.zeros(d, device=dev), torch.zeros(d, device=dev)]
    ws = torch.empty(ops.adapter_workspace_bytes(M, d, dim, cdt), dtype=torch.uint8, device=dev)
    n, mean, rstd = torch.empty(M, d, device=dev, dtype=cdt), torch.empty(M, device=dev), torch.empty(M, device=dev)
    h, a, da, dn = (torch.empty(M, k, device=dev, dtype=cdt) for k in (dim, dim, dim, d))

    def fused_f(): ops.adapter_fwd(x, gam, bet, wd, wu, y, M, d, dim)
    def fused_b(): ops.adapter_bwd(x, dy, gam, bet, wd, wut, wdt, dx, *grads, ws, M, d, dim)

    def plain_f():
        ops.layernorm_fwd(x, gam, bet, n, mean, rstd, M, d, 1e-5)
        ops.gemm(n, wd, h, M, dim, d, d, d, dim)
        torch.mul(h, torch.sigmoid(h), out=a)
        ops.gemm(a, wu, y, M, d, dim, dim, dim, d, epi=ops.EPI_RESID, aux_in=x)

    def plain_b():
        dyc = dy.to(cdt)
        ops.gemm(dyc, wut, da, M, dim, d, d, d, dim)
        s = torch.sigmoid(h.float())
        dh = (da.float() * (s * (1 + h.float() * (1 - s)))).to(cdt)
        ops.gemm(dyc, a, grads[1], d, dim, M, d, dim, dim, transA=True, transB=True, atomic=True, c_dtype=ops.F32)
        ops.gemm(dh, n, grads[0], dim, d, M, dim, d, d, transA=True, transB=True, atomic=True, c_dtype=ops.F32)
        ops.gemm(dh, wdt, dn, M, d, dim, dim, dim, d)
        dx.copy_(dy)
        ops.layernorm_bwd(dn, x, gam, mean, rstd, dx, True, grads[2], grads[3], M, d)

    for f in (fused_f, fused_b, plain_f, plain_b):
        f()
    t = {k: [] for k in ("fused_fwd", "plain_fwd", "fused_bwd", "plain_bwd")}
    for _ in range(4):   # alternate the candidates: drift of the box lands on both
        t["fused_fwd"] += timed(fused_f, reps); t["plain_fwd"] += timed(plain_f, reps)
        t["fused_bwd"] += timed(fused_b, reps); t["plain_bwd"] += timed(plain_b, reps)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    med.update(M=M, d=d, dim=dim, dtype=str(cdt).split(".")[1], floor_fwd_us_at_8TBs=2 * M * d * 4 / 8e12 * 1e6)
    return med


def step_bench(dim, steps, rounds):
    from nemo_amd.models import EncDecCTCModel, conformer_ctc_config
    g = torch.Generator().manual_seed(1234)   # bench.py's synthetic batch: 32 utterances of 20 s, 60 tokens each, full lengths
    B, S, U = 32, 320000, 60
    batch = [0.1 * torch.randn(B, S, generator=g), torch.full((B,), S, dtype=torch.int64), torch.randint(0, 128, (B, U), generator=g),
             torch.full((B,), U, dtype=torch.int64)]
    batch = [t.to(dev) for t in batch]

    def make(kind):
        torch.manual_seed(0)
        model = EncDecCTCModel(conformer_ctc_config("large", vocab_size=128, spec_augment=True, compute_dtype=torch.bfloat16))
        model.decoder.compute_dtype = torch.bfloat16
        model = model.to(dev).train()
        if kind != "base":
            model.add_adapter("a", dict(in_features=model.encoder.d_model, dim=dim, activation="swish", norm_position="pre", dropout=0.0))
            with torch.no_grad():
                for n, p in model.named_parameters():
                    if n.endswith("module.3.weight"):
                        p.normal_(0.0, 0.02)
            model.encoder.weights_updated()
        if kind == "adapters_only":
            model.freeze(); model.unfreeze_enabled_adapters(); model.train()
        model.setup_optimization()
        for i in range(24):   # warm-up until the encoder has settled on live launches or replay
            loss = model.fit_step(batch)["loss"]
            torch.cuda.synchronize()
            if i >= 5 and model.encoder.graphs_settled():
                break
        return model, float(loss.item())

    kinds = ("base", "adapters_all_trained", "adapters_only")
    models = {k: make(k) for k in kinds}
    ms = {k: [] for k in kinds}
    for _ in range(rounds):
        for k in kinds:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = models[k][0].fit_step(batch)["loss"]
            torch.cuda.synchronize()
            ms[k].append(round((time.perf_counter() - t0) / steps * 1e3, 2))
            assert torch.isfinite(loss), k
    print(json.dumps({"dim": dim, "steps": steps, "ms_per_step_by_round": ms, "warmup_loss": {k: models[k][1] for k in kinds}}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--rows", type=int, default=32 * 500)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    if a.step:
        step_bench(a.dim, a.steps, a.rounds)
        sys.exit(0)
    for dim in (32, 64):
        for cdt in (torch.bfloat16, torch.float32):
            print(json.dumps(case(a.rows, a.d, dim, cdt, a.reps)))
