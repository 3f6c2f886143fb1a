"""Node block (phi_h + phi_v of one FastEGNN layer), forward + backward in
bf16: the fused HIP kernel pair vs the eager composition.

Times ``ops.fused_node_block`` through autograd (forward, then the gradients
of h, agg_e, agg_v and every parameter) at N = 113,140 nodes (LargeFluid)
for each hidden_nf in --widths, in three modes: ``a2`` (node_attr_nf = 2),
``a0`` (no node attributes) and ``vel`` (vel-only: phi_v alone). Arm
``fused`` is the kernel pair (csrc/fused_node.hip, csrc/fused_node_h128.hip
at hidden_nf = 128), arm ``eager`` the same call under
``DISTEGNN_NODE_EAGER=1``; the dispatch reads the variable per call, so both
run in one process. Run on a GPU box:

    python benchmarks/node_block.py [--steps 10] [--repeats 3]

Timing as in eval_forward.py: every arm is warmed up first, a timed window
is --steps forward + backward passes between two device events ending in a
synchronise, and the windows of the two arms are interleaved --repeats
times. Printed per arm: the median window, the min..max spread and the peak
allocated memory of one pass above what is resident before it; per row
whether the fused median is below the eager median by more than the larger
of the two spreads; then one JSON line.
"""

import argparse
import json
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)

import torch
from torch import nn

N_LARGEFLUID = 113140
MODES = (("a2", 2, False), ("a0", 0, False), ("vel", 0, True))
ARMS = (("fused", False), ("eager", True))
_SWITCH = "DISTEGNN_NODE_EAGER"


def make_pass(n, hidden, attr_nf, vel_only, eager, device):
    from distegnn_amd import ops
    from distegnn_amd.ops.linear import SplitKLinear

    torch.manual_seed(0)
    bf = torch.bfloat16
    k1 = 3 * hidden + attr_nf
    node_mlp = nn.Sequential(SplitKLinear(k1, hidden), nn.SiLU(),
                             SplitKLinear(hidden, hidden)).to(device)
    vel_mlp = nn.Sequential(SplitKLinear(hidden, hidden), nn.SiLU(),
                            SplitKLinear(hidden, 1)).to(device)
    ins = [torch.randn(n, hidden, device=device).to(bf).requires_grad_()
           for _ in range(3)]
    attr = (torch.randn(n, attr_nf, device=device).to(bf)
            if attr_nf else None)
    dh_out = torch.randn(n, hidden, device=device).to(bf)
    params = list(vel_mlp.parameters())
    if not vel_only:
        params = list(node_mlp.parameters()) + params
    wrt = (ins[:1] if vel_only else ins) + params

    def run():
        os.environ.pop(_SWITCH, None)
        if eager:
            os.environ[_SWITCH] = "1"
        try:
            with torch.autocast("cuda", dtype=bf):
                h_out, phiv = ops.fused_node_block(
                    ins[0], ins[1], ins[2], attr, node_mlp, vel_mlp, True,
                    vel_only=vel_only)
            outs, cots = [phiv], [torch.ones_like(phiv)]
            if not vel_only:
                outs.append(h_out)
                cots.append(dh_out.to(h_out.dtype))
            return torch.autograd.grad(outs, wrt, cots)
        finally:
            os.environ.pop(_SWITCH, None)

    return run


def window(run, steps):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        run()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / steps


def peak_mib(run):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    run()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--widths", type=str, default="32,64,128")
    ap.add_argument("--modes", type=str, default="a2,a0,vel")
    ap.add_argument("--nodes", type=int, default=N_LARGEFLUID)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("node_block.py measures GPU time; no GPU found")
    device = torch.device("cuda:0")
    widths = [int(w) for w in args.widths.split(",")]
    modes = [m for m in MODES if m[0] in args.modes.split(",")]
    print(f"# node block forward + backward, bf16, N = {args.nodes}, "
          f"{args.steps} passes/window x {args.repeats}", flush=True)
    result = {}
    for hdim in widths:
        for mode, attr_nf, vel_only in modes:
            runs = {}
            for name, eager in ARMS:
                run = make_pass(args.nodes, hdim, attr_nf, vel_only, eager,
                                device)
                for _ in range(args.warmup):
                    grads = run()
                torch.cuda.synchronize()
                if not all(bool(torch.isfinite(g).all()) for g in grads):
                    sys.exit(f"H={hdim} {mode} {name}: non-finite gradient")
                runs[name] = run
            times = {name: [] for name in runs}
            for _ in range(args.repeats):
                for name, run in runs.items():
                    times[name].append(window(run, args.steps))
            row = {}
            for name, run in runs.items():
                ts = sorted(times[name])
                row[name] = (ts[len(ts) // 2], ts[0], ts[-1], peak_mib(run))
                med, lo, hi, peak = row[name]
                print(f"H={hdim:<4d} {mode:<4s} {name:<6s} {med:8.3f} "
                      f"ms/pass (min {lo:.3f}, max {hi:.3f})  peak "
                      f"{peak:7.0f} MiB")
                key = f"H{hdim}_{mode}_{name}"
                result[f"{key}_ms"] = round(med, 4)
                result[f"{key}_min_ms"] = round(lo, 4)
                result[f"{key}_max_ms"] = round(hi, 4)
                result[f"{key}_peak_mib"] = round(peak)
            spread = max(row[k][2] - row[k][1] for k in row)
            faster = row["eager"][0] - row["fused"][0] > spread
            print(f"H={hdim:<4d} {mode:<4s} eager / fused "
                  f"{row['eager'][0] / row['fused'][0]:.2f}x (larger spread "
                  f"{spread:.3f} ms: fused is "
                  f"{'faster beyond it' if faster else 'NOT faster beyond it'}"
                  f")", flush=True)
            result[f"H{hdim}_{mode}_speedup"] = round(
                row["eager"][0] / row["fused"][0], 3)
            result[f"H{hdim}_{mode}_fused_faster"] = faster
            del runs
            torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
