"""FastEGNN no-grad fp32 evaluation forward: fused fp32 kernels vs eager.

Evaluation (runtime/trainer.py ``_eval``) runs the model under
``torch.no_grad()`` in fp32 unless ``train.bf16_eval`` is set. This times that
forward (FastEGNN, L=4, normalisation as in the workload) with the
forward-only fp32 kernels (csrc/fused_edge_f32.hip, fused_virtual_f32.hip,
fused_node_f32.hip: arm ``fused``), with ``DISTEGNN_NODE_EAGER=1`` (arm
``node-eager``: the same forward with the node block on its eager
composition, which is what fp32 evaluation ran before the fp32 node kernel)
and with ``DISTEGNN_DISABLE_FUSED=1`` (arm ``eager``: the composition every
fp32 evaluation took before any of those kernels existed), on the two
headline graphs of
bench.py: the synthetic LargeFluid-113K graph (C=5) and the Water-3D batch of
15 graphs (C=3), for each hidden_nf in --widths. Run on a GPU box:

    python benchmarks/eval_forward.py [--steps 10] [--repeats 3]

Timing as in hidden_sweep.py: every arm is warmed up first, a timed window
is --steps forwards between two device events ending in a synchronise, and
the windows of all arms are interleaved --repeats times in one process. The
median window and the min..max spread are printed per arm, with the peak
allocated memory of one forward (above what is resident before it), the
``eager`` / ``fused`` speed-up, the ``fused`` / ``node-eager`` ratio judged
against the larger of those two arms' spreads, and the relative L2 distance
of the fused displacement from each other arm's; then one JSON line.
"""

import argparse
import json
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)

import torch


def load_batch(workload, device):
    import bench

    if workload == "largefluid":
        _, nodes, _, radius, *_ = bench.WORKLOADS[workload]
        bt = bench.build_rank_batches(0, 1, 1, nodes, radius, "random",
                                      seed=43)[0]
    else:
        gpb = bench.WORKLOADS[workload][2]
        bt = bench.build_cutoff_batches(workload, 1, gpb, seed=43)[0]
    return bt.to(device)


# arm -> the opt-out variable its forwards run under
ARMS = (("fused", None),
        ("node-eager", "DISTEGNN_NODE_EAGER"),
        ("eager", "DISTEGNN_DISABLE_FUSED"))
_SWITCHES = tuple(v for _, v in ARMS if v is not None)


def make_forward(workload, hidden, batch, device, switch):
    import bench
    from distegnn_amd.models import FastEGNN
    from distegnn_amd.runtime.trainer import model_forward
    from distegnn_amd.utils import fix_seed

    (_, _, _, _, feat_nf, attr_nf, vch, _, _, _,
     normalize) = bench.WORKLOADS[workload]
    fix_seed(0)
    model = FastEGNN(node_feat_nf=feat_nf, node_attr_nf=attr_nf,
                     edge_attr_nf=2, hidden_nf=hidden, virtual_channels=vch,
                     world_size=1, n_layers=4, normalize=normalize).to(device)
    model.eval()

    def forward():
        for var in _SWITCHES:
            os.environ.pop(var, None)
        if switch is not None:
            os.environ[switch] = "1"
        try:
            with torch.no_grad():
                return model_forward(model, "FastEGNN", batch, device)
        finally:
            for var in _SWITCHES:
                os.environ.pop(var, None)

    return forward


def window(forward, steps):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        forward()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / steps


def peak_mib(forward):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    forward()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--widths", type=str, default="32,64,128")
    ap.add_argument("--workloads", type=str, default="largefluid,water3d")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_forward.py measures GPU time; no GPU found")
    device = torch.device("cuda:0")
    widths = [int(w) for w in args.widths.split(",")]
    result = {}
    for workload in args.workloads.split(","):
        batch = load_batch(workload, device)
        print(f"# {workload}: {batch.num_nodes} nodes, {batch.num_edges} "
              f"edges, {batch.num_graphs} graphs, FastEGNN L=4 fp32 no_grad, "
              f"{args.steps} forwards/window x {args.repeats}", flush=True)
        arms = {}
        for hdim in widths:
            for name, switch in ARMS:
                fwd = make_forward(workload, hdim, batch, device, switch)
                for _ in range(args.warmup):
                    loc, vloc = fwd()
                torch.cuda.synchronize()
                if not bool(torch.isfinite(loc).all()):
                    sys.exit(f"{workload} H={hdim} {name}: non-finite output")
                arms[(hdim, name)] = (fwd, loc, vloc)
        times = {k: [] for k in arms}
        for _ in range(args.repeats):
            for k, (fwd, _, _) in arms.items():
                times[k].append(window(fwd, args.steps))
        for hdim in widths:
            row = {}
            for name, _ in ARMS:
                fwd = arms[(hdim, name)][0]
                ts = sorted(times[(hdim, name)])
                row[name] = (ts[len(ts) // 2], ts[0], ts[-1], peak_mib(fwd))
            pos = batch.pos
            lf = arms[(hdim, "fused")][1]

            def distance(other):
                lo_ = arms[(hdim, other)][1]
                return float(((lf - lo_).double().norm()
                              / (lo_ - pos).double().norm()))

            dist, dist_ne = distance("eager"), distance("node-eager")
            for name, _ in ARMS:
                med, lo, hi, peak = row[name]
                key = name.replace("-", "_")
                print(f"{workload:<10s} H={hdim:<4d} {name:<10s} {med:9.2f} "
                      f"ms/forward (min {lo:.2f}, max {hi:.2f})  peak "
                      f"{peak:8.0f} MiB")
                result[f"{workload}_H{hdim}_{key}_ms"] = round(med, 3)
                result[f"{workload}_H{hdim}_{key}_min_ms"] = round(lo, 3)
                result[f"{workload}_H{hdim}_{key}_max_ms"] = round(hi, 3)
                result[f"{workload}_H{hdim}_{key}_peak_mib"] = round(peak)
            print(f"{workload:<10s} H={hdim:<4d} speed-up "
                  f"{row['eager'][0] / row['fused'][0]:.2f}x, displacement "
                  f"of the two arms differs by {dist:.2e} (relative L2)")
            result[f"{workload}_H{hdim}_speedup"] = round(
                row["eager"][0] / row["fused"][0], 3)
            # fused against the same forward with the node block on the
            # composition; "within spread": the fused median is not above
            # the node-eager median by more than the larger min..max spread
            ratio = row["fused"][0] / row["node-eager"][0]
            spread = max(row[k][2] - row[k][1] for k in ("fused",
                                                         "node-eager"))
            slower = row["fused"][0] - row["node-eager"][0] > spread
            print(f"{workload:<10s} H={hdim:<4d} fused / node-eager "
                  f"{ratio:.3f} (larger spread {spread:.2f} ms: fused is "
                  f"{'SLOWER beyond it' if slower else 'not slower beyond it'}"
                  f"), displacement of the two arms differs by "
                  f"{dist_ne:.2e} (relative L2)")
            result[f"{workload}_H{hdim}_fused_over_node_eager"] = round(
                ratio, 3)
            result[f"{workload}_H{hdim}_node_eager_distance"] = dist_ne
            result[f"{workload}_H{hdim}_fused_not_slower"] = not slower
        del arms, batch
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
