"""Training kernels and the tables launch of the stateless prediction network next to the LSTM prediction network (recipe widths,
bf16 compute): forward + backward of `StatelessTransducerDecoder` (csrc/stateless.hip) and of `RNNTDecoder` on the same targets,
alternating rounds in ONE process, and `ops.stateless_tables` alone.  Medians over the rounds with the smallest and largest round.

    python tools/stateless_bench.py [--batch 32] [--labels 100] [--context 2] [--steps 10] [--warmup 3] [--json OUT]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nemo_amd import ops  # noqa: E402
from nemo_amd.modules import RNNTDecoder, StatelessTransducerDecoder  # noqa: E402
from tools.stream_bench import timed  # noqa: E402

dev = torch.device("cuda", 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--labels", type=int, default=100)
    ap.add_argument("--context", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    V, E, J = 1024, 640, 640
    torch.manual_seed(1)
    nets = {"stateless": StatelessTransducerDecoder(prednet={"pred_hidden": E, "dropout": 0.2}, vocab_size=V, context_size=args.context,
                                                    compute_dtype=torch.bfloat16),
            "lstm": RNNTDecoder(prednet={"pred_hidden": E, "pred_rnn_layers": 1, "dropout": 0.2}, vocab_size=V,
                                compute_dtype=torch.bfloat16)}
    tg = torch.randint(0, V, (args.batch, args.labels), device=dev)
    tl = torch.full((args.batch,), args.labels, dtype=torch.int64, device=dev)
    dg = torch.randn(args.batch, E, args.labels + 1, device=dev)
    fns = {}
    for name, net in nets.items():
        net = net.to(dev).train()

        def fwd_bwd(net=net):
            g = net(targets=tg, target_length=tl)[0]
            g.backward(dg.to(g.dtype))
        fns[name + "_fwd_bwd"] = fwd_bwd
        fns[name + "_fwd"] = lambda net=net: torch.no_grad()(lambda: net(targets=tg, target_length=tl))()
    w_pred = torch.randn(J, E, device=dev).to(torch.bfloat16)
    embs = [e.weight for e in nets["stateless"].prediction["embeds"]]
    tabs = torch.empty(args.context, V + 1, J, device=dev)
    fns["tables"] = lambda: ops.stateless_tables(embs, w_pred, E, V, out=tabs)
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(7):
        for k, fn in fns.items():
            ms[k].append(timed(fn, args.steps))
    row = dict(batch=args.batch, labels=args.labels, context=args.context,
               ms={k: dict(median=round(statistics.median(v), 4), range=[round(min(v), 4), round(max(v), 4)]) for k, v in ms.items()})
    print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
