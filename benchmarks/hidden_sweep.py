"""FastEGNN eager-mode train-step time per hidden width.

Companion to the headline bench.py (fixed at hidden_nf=64, which owns the
BASELINE contract): one forward+loss+backward+Adam step of FastEGNN (L=4,
C=3, bf16 autocast, no hipGraph) on the seeded synthetic Water-3D batch of
the docs/KERNELS.md figures, for each hidden_nf in --widths. Run on a GPU
box:

    python benchmarks/hidden_sweep.py [--steps 30] [--repeats 3]

Timing: every width is warmed up first (code-object loads, weight-prep
caches, allocator), each timed window is --steps full steps between two
device events ending in a synchronise, and windows of the widths are
interleaved --repeats times so drift on a shared host hits all widths alike.
The median window and the min..max spread are printed per width, then one
JSON line with the medians.
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def make_step(hidden, batch, device):
    from distegnn_amd.models import FastEGNN
    from distegnn_amd.runtime.trainer import model_forward
    from distegnn_amd.utils import fix_seed

    fix_seed(0)
    model = FastEGNN(node_feat_nf=2, node_attr_nf=0, edge_attr_nf=2,
                     hidden_nf=hidden, virtual_channels=3, world_size=1,
                     n_layers=4).to(device)
    opt = torch.optim.Adam(model.parameters(), lr=5e-4)

    def step():
        opt.zero_grad(set_to_none=False)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            pred, _ = model_forward(model, "FastEGNN", batch, device)
        loss = torch.nn.functional.mse_loss(pred.float(), batch.target)
        loss.backward()
        opt.step()
        return loss

    return step


def window(step, steps):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        step()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=7806)
    ap.add_argument("--graphs-per-batch", type=int, default=4)
    ap.add_argument("--widths", type=str, default="32,64,128")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hidden_sweep.py measures GPU step time; no GPU found")
    device = torch.device("cuda:0")

    from distegnn_amd.data.graph import collate
    from distegnn_amd.data.synthetic import make_cutoff_dataset
    from distegnn_amd.utils import fix_seed

    fix_seed(0)
    batch = collate(make_cutoff_dataset(
        "Water-3D", args.graphs_per_batch, seed=0,
        n_override=args.nodes // args.graphs_per_batch)).to(device)
    print(f"# {batch.num_nodes} nodes, {batch.num_edges} edges, "
          f"{batch.num_graphs} graphs, FastEGNN L=4 C=3 bf16 eager-mode, "
          f"{args.steps} steps/window x {args.repeats}")
    widths = [int(w) for w in args.widths.split(",")]
    steps = {}
    for hdim in widths:
        steps[hdim] = make_step(hdim, batch, device)
        for _ in range(args.warmup):
            loss = steps[hdim]()
        torch.cuda.synchronize()
        if not torch.isfinite(loss):
            sys.exit(f"H={hdim}: non-finite loss {loss.item()}")
    times = {hdim: [] for hdim in widths}
    for _ in range(args.repeats):
        for hdim in widths:
            times[hdim].append(window(steps[hdim], args.steps))
    result = {}
    for hdim in widths:
        ts = sorted(times[hdim])
        med = ts[len(ts) // 2]
        result[f"H{hdim}_ms_per_step"] = round(med, 3)
        print(f"H={hdim:<4d} {med:9.2f} ms/step   "
              f"(min {ts[0]:.2f}, max {ts[-1]:.2f})")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
