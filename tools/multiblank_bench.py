"""The multi-blank transducer on one GPU, one process:
  1. the three multi-blank loss kernels (mb_row / mb_lattice / mb_grad) at B = 32, T = 250, U = 60, N = 1028 next to the RNN-T ones at
     V1 = 1025 and the TDT ones at V1 = 1025, D = 4, bf16 pitched gradient, from the same library; rounds alternate between the three
     losses, the report gives the median per kernel and the spread (min .. max) over the rounds;
  2. the multi-blank greedy search next to the RNN-T greedy search at B = 32, T = 250, H = J = 640, V1 = 1025, bf16 images, seeded
     random weights with a bias on every blank-like row (large: blanks dominate as in a trained model; small: nearly every frame
     emits max_symbols labels; the saving on random weights is whatever that bias produces), and the number
     of search steps (joint evaluations) each took, counted by a batched float32 restatement of the rule in torch on the device
     whose label count is printed next to the kernel's.

    python tools/multiblank_bench.py [--rounds 5] [--reps 5] [--iters 10] [--bias 14 [1 ...]] [--skip-loss]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

dev = "cuda"
BIG = [2, 4, 8]


def loss_kernel_times(rounds, reps):
    from torch.profiler import ProfilerActivity, profile
    from nemo_amd import ops
    B, T, U1, V1 = 32, 250, 61, 1025
    g = torch.Generator(device=dev).manual_seed(0)
    lab = torch.randint(0, V1 - 1, (B, U1 - 1), device=dev, generator=g)
    lens = torch.full((B,), T, device=dev, dtype=torch.int64)
    ll = torch.full((B,), U1 - 1, device=dev, dtype=torch.int64)
    ld = (V1 + 4 + 7) // 8 * 8   # one pitch for the three row widths 1025, 1028, 1029
    acts = torch.randn(B * T * U1, ld, device=dev, generator=g)
    grads = torch.empty(B * T * U1, ld, device=dev, dtype=torch.bfloat16)
    calls = {
        "rnnt": lambda: ops.rnnt_loss_pitched(acts, ld, B, T, U1, V1, lab, lens, ll, V1 - 1, grads, ld, grad_scale=0.25),
        "tdt": lambda: ops.tdt_loss_pitched(acts, ld, B, T, U1, V1, [0, 1, 2, 3], lab, lens, ll, V1 - 1, grads=grads, ld_grads=ld,
                                            sigma=0.02, grad_scale=0.25),
        "mb": lambda: ops.multiblank_loss_pitched(acts, ld, B, T, U1, V1 + len(BIG), BIG, lab, lens, ll, V1 - 1 + len(BIG), grads=grads,
                                                  ld_grads=ld, sigma=0.02, grad_scale=0.25),
    }
    for call in calls.values():
        for _ in range(2):
            call()
    torch.cuda.synchronize()
    out = {}
    for _ in range(rounds):
        for name, call in calls.items():
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(reps):
                    call()
                torch.cuda.synchronize()
            for ev in prof.key_averages():
                key = ev.key[5:] if ev.key.startswith("void ") else ev.key
                if key.startswith(name + "_"):
                    us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                    out.setdefault(key.split("(")[0].split("<")[0], []).append(us / max(1, ev.count))
    return out


@torch.no_grad()
def count_steps(m, f, lens, big, max_symbols):
    """the search rule in float32 torch, the batch in lock step -> (joint evaluations, labels) over the batch"""
    B, T, _ = f.shape
    V1, H = m["emb"].shape
    bo = V1 - 1 + len(big)
    jump = torch.ones(bo + 1, dtype=torch.int64, device=dev)
    for i, d in enumerate(big):
        jump[bo - 1 - i] = d
    W = {k: v.float() for k, v in m.items()}

    def pred(x, h, c):
        z = ((h @ W["w_hh"].T + W["b_hh"]) + x @ W["w_ih"].T) + W["b_ih"]
        i, fg, g, o = z.split(H, 1)
        c2 = torch.sigmoid(fg) * c + torch.sigmoid(i) * torch.tanh(g)
        h2 = torch.sigmoid(o) * torch.tanh(c2)
        return h2, c2, h2 @ W["w_pred"].T + W["b_pred"]

    h = c = torch.zeros(B, H, device=dev)
    h2, c2, gp = pred(torch.zeros(B, H, device=dev), h, c)
    t = torch.zeros(B, dtype=torch.int64, device=dev)
    sym = torch.zeros_like(t)
    steps = labels = 0
    ar = torch.arange(B, device=dev)
    while True:
        full = (sym >= max_symbols) & (t < lens)
        t, sym = t + full.long(), sym * (~full).long()
        live = t < lens
        if not bool(live.any()):
            return steps, labels
        lg = torch.relu(f[ar, t.clamp(max=T - 1)].float() + gp) @ W["w_out"].T + W["b_out"]
        k = lg.argmax(1)
        lab = live & (k < V1 - 1)
        blk = live & ~lab
        steps += int(live.sum()); labels += int(lab.sum())
        t = t + blk.long() * jump[k.clamp(max=bo)]
        sym = torch.where(lab, sym + 1, torch.zeros_like(sym))
        nh, nc, ngp = pred(W["emb"][k.clamp(max=V1 - 2)], h2, c2)
        sel = lab[:, None]
        h, c = torch.where(sel, h2, h), torch.where(sel, c2, c)
        h2, c2, gp = torch.where(sel, nh, h2), torch.where(sel, nc, c2), torch.where(sel, ngp, gp)


def greedy_times(rounds, iters, bias):
    from nemo_amd import ops
    B, T, H, J, V1, ms = 32, 250, 640, 640, 1025, 10
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s, k=1.0: torch.randn(*s, device=dev, generator=g) * k   # noqa: E731
    bf = lambda x: x.to(torch.bfloat16).contiguous()   # noqa: E731
    f = bf(r(B, T, J, k=1.5))
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)
    m = dict(emb=r(V1, H), w_ih=bf(r(4 * H, H, k=0.15)), w_hh=bf(r(4 * H, H, k=0.15)), b_ih=r(4 * H, k=0.1), b_hh=r(4 * H, k=0.1),
             w_pred=bf(r(J, H, k=0.15)), b_pred=r(J, k=0.1), w_out=bf(r(V1 + len(BIG), J, k=0.15)), b_out=r(V1 + len(BIG), k=0.1))
    m["emb"][V1 - 1] = 0.0
    m["b_out"][V1 - 1:] += 2.0 + bias   # every blank-like row; the RNN-T model below keeps the standard blank's
    rn = dict(m, w_out=torch.cat([m["w_out"][:V1 - 1], m["w_out"][-1:]]).contiguous(), b_out=torch.cat([m["b_out"][:V1 - 1], m["b_out"][-1:]]).contiguous())
    arg = lambda w: (w["emb"], w["w_ih"], H, w["w_hh"], H, w["b_ih"], w["b_hh"], w["w_pred"], H, w["b_pred"], w["w_out"], J, w["b_out"], V1 - 1)  # noqa: E731
    calls = {"rnnt": lambda: ops.rnnt_greedy_decode(f, lens, *arg(rn), ms), "mb": lambda: ops.multiblank_greedy_decode(f, lens, *arg(m), BIG, ms)}
    res = {k: dict(ms=[]) for k in calls}
    for k, call in calls.items():
        for _ in range(2):
            out = call()
        res[k]["labels"] = int(out[2].sum())
        res[k]["steps"], res[k]["labels_restated"] = count_steps(rn if k == "rnnt" else m, f, lens, [] if k == "rnnt" else BIG, ms)
    for _ in range(rounds):
        for k, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                call()
            e1.record()
            torch.cuda.synchronize()
            res[k]["ms"].append(e0.elapsed_time(e1) / iters)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--bias", type=float, nargs="+", default=[14.0], help="added to the +2 of every blank-like row of b_out, one search run each")
    ap.add_argument("--skip-loss", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multiblank_bench measures on the GPU: none found")
    kt = {} if a.skip_loss else loss_kernel_times(a.rounds, a.reps)
    for k in sorted(kt):
        print(f"kernel {k:22s} median {statistics.median(kt[k]):9.1f} us  ({min(kt[k]):.1f} .. {max(kt[k]):.1f}, {len(kt[k])} rounds)", flush=True)
    for bias in a.bias:
        for k, v in greedy_times(a.rounds, a.iters, bias).items():
            med = statistics.median(v["ms"])
            print(f"greedy bias {bias:g} {k:5s} median {med:8.2f} ms ({min(v['ms']):.2f} .. {max(v['ms']):.2f}); steps {v['steps']}, labels "
                  f"{v['labels']} (restatement: {v['labels_restated']}, {v['labels'] / 8000:.2f} per frame); {1e3 * med / max(1, v['steps']) * 32:.1f} us "
                  f"per step of an utterance (batch mean; a launch lasts as long as its slowest utterance)", flush=True)


if __name__ == "__main__":
    main()
