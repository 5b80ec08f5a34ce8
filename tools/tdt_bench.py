"""TDT against RNN-T on one GPU, one process:
  1. per-kernel time of the three TDT loss kernels (tdt_row / tdt_lattice / tdt_grad) against the three RNN-T ones (rnnt_denom /
     rnnt_lattice / rnnt_grad) at one FastConformer-Large joint sub-batch, 4 x 250 x 81 x (1025 [+ 5]), bf16 pitched gradient
     as in the fused joint + loss;
  2. training step time of FastConformer-TDT-Large against FastConformer-Transducer-Large (bf16, same synthetic batch).

    python tools/tdt_bench.py [--batch 16] [--secs 20] [--steps 10] [--warmup 3] [--skip-steps]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

dev = "cuda"


def kernel_times(reps):
    from torch.profiler import ProfilerActivity, profile
    from nemo_amd import ops
    B, T, U1, V1, durations = 4, 250, 81, 1025, [0, 1, 2, 3, 4]
    g = torch.Generator(device=dev).manual_seed(0)
    lab = torch.randint(0, V1 - 1, (B, U1 - 1), device=dev, generator=g)
    lens = torch.full((B,), T, device=dev, dtype=torch.int64)
    ll = torch.full((B,), U1 - 1, device=dev, dtype=torch.int64)
    out = {}
    for name, W in (("rnnt", V1), ("tdt", V1 + len(durations))):
        ld = (W + 7) // 8 * 8
        acts = torch.randn(B * T * U1, ld, device=dev, generator=g)
        grads = torch.empty(B * T * U1, ld, device=dev, dtype=torch.bfloat16)

        def call():
            if name == "rnnt":
                ops.rnnt_loss_pitched(acts, ld, B, T, U1, V1, lab, lens, ll, V1 - 1, grads, ld, grad_scale=0.25)
            else:
                ops.tdt_loss_pitched(acts, ld, B, T, U1, V1, durations, lab, lens, ll, V1 - 1, grads=grads, ld_grads=ld, sigma=0.02,
                                     grad_scale=0.25)
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                call()
            torch.cuda.synchronize()
        for ev in prof.key_averages():
            key = ev.key[5:] if ev.key.startswith("void ") else ev.key   # templated kernels: "void name<T>(...)"
            if key.startswith(name + "_"):
                us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                out[key.split("(")[0].split("<")[0]] = us / max(1, ev.count)
    return out


def step_time(kind, batch, secs, steps, warmup):
    from bench import synthetic_batch
    from nemo_amd.models import EncDecRNNTModel, fastconformer_tdt_config, fastconformer_transducer_config
    cdt = torch.bfloat16
    torch.manual_seed(0)
    make = fastconformer_tdt_config if kind == "tdt" else fastconformer_transducer_config
    model = EncDecRNNTModel(make("large", vocab_size=1024, spec_augment=True, compute_dtype=cdt))
    model.decoder.compute_dtype = model.joint.compute_dtype = cdt
    model = model.to(dev).train()
    model.setup_optimization(dict(name="adamw", lr=1e-4, betas=[0.9, 0.98], weight_decay=1e-3))
    audio, alen, tok, tl = synthetic_batch(batch, secs, vocab=1024, seed=1234)
    b = [audio.to(dev), alen.to(dev), tok.to(dev), tl.to(dev)]
    for _ in range(warmup):
        model.fit_step(b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = model.fit_step(b)["loss"]
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    del model
    torch.cuda.empty_cache()
    return ms, float(loss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--secs", type=float, default=20.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-steps", action="store_true")
    a = ap.parse_args()
    kt = kernel_times(a.reps)
    for k in sorted(kt):
        print(f"kernel {k:28s} {kt[k]:9.1f} us")
    for r, t in (("rnnt_denom_kernel", "tdt_row_kernel"), ("rnnt_lattice_kernel", "tdt_lattice_kernel"),
                 ("rnnt_grad_kernel", "tdt_grad_kernel")):
        if r in kt and t in kt:
            print(f"ratio {t} / {r}: {kt[t] / kt[r]:.3f}")
    if not a.skip_steps:
        res = {k: step_time(k, a.batch, a.secs, a.steps, a.warmup) for k in ("rnnt", "tdt")}
        for k, (ms, loss) in res.items():
            print(f"step FastConformer-{'TDT' if k == 'tdt' else 'Transducer'}-Large bf16 batch {a.batch} x {a.secs:g} s: "
                  f"{ms:.2f} ms (loss {loss:.3f})")
        print(f"ratio TDT / Transducer step: {res['tdt'][0] / res['rnnt'][0]:.3f}")


if __name__ == "__main__":
    main()
