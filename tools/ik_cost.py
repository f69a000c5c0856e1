"""Cost of pnr_get_jacobian and pnr_solve_ik (PioneerVectorEnv.jacobian / solve_ik) into preallocated outputs: device events
around K back-to-back graph-replayed calls after a warm-up, the median of ROUNDS.

Table 1: pnr_get_jacobian at N envs (default 65 536 and 1 048 576) for a caller's [N, 12] joint buffer, measured in the same
run as pnr_get_link_states at the same size, alternating round by round; the rate is counted against (144 + 48) B per env
(link states: 572 + 48).
Table 2: pnr_solve_ik at 65 536 envs, default parameters, targets uniform in the reference's box (15, -10, 2) .. (25, 10, 6),
from the rest pose: us per call, the histogram of iterations_out, us per iteration-env, and the share of targets left further
than done_distance (unreachable).  Usage: python tools/ik_cost.py [N ...] [--rounds R] [--calls K] [--ik-envs M]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pioneer_amd import PioneerVectorEnv  # noqa: E402

HBM_PEAK = 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument("sizes", nargs="*", type=int, default=[65536, 1048576])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=100)
ap.add_argument("--ik-envs", type=int, default=65536)
args = ap.parse_args()
dev = torch.device("cuda:0")
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(fn):
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3                 # us


def captured(fn, calls):
    """A graph of `calls` back-to-back fn() on one stream."""
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        fn()                                         # warm-up on the capture stream
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            for _ in range(calls):
                fn()
    torch.cuda.synchronize()
    g.replay()
    return g


def median(xs):
    return sorted(xs)[len(xs) // 2]


for n in args.sizes:
    env = PioneerVectorEnv(n, device=dev, seed=0)
    js = torch.randn((n, 12), dtype=torch.float32, device=dev)
    jac = torch.empty((n, 6, 6), dtype=torch.float32, device=dev)
    rec = torch.empty((n, 11, 13), dtype=torch.float32, device=dev)
    graphs = {"jacobian": captured(lambda: env.jacobian(joint_state=js, out=jac), args.calls),
              "link_states": captured(lambda: env.link_states(js, out=rec), args.calls)}
    times = {k: [] for k in graphs}
    for _ in range(args.rounds):                     # alternating
        for k, g in graphs.items():
            times[k].append(timed(g.replay) / args.calls)
    row = {"table": 1, "envs": n}
    for k, b in (("jacobian", 144 + 48), ("link_states", 572 + 48)):
        us = median(times[k])
        row[k] = {"us_per_call_graph": us, "all_us": times[k], "bytes_per_env": b, "TBps": n * b / (us * 1e-6) / 1e12,
                  "frac_of_8TBps": n * b / (us * 1e-6) / HBM_PEAK}
    print(json.dumps(row), flush=True)
    del graphs
    env.close()

n = args.ik_envs
env = PioneerVectorEnv(n, device=dev, seed=0)
env.reset()                                          # targets uniform in the reference's box
out = {"q": torch.empty((n, 6), device=dev), "residual": torch.empty(n, device=dev),
       "iterations": torch.empty(n, dtype=torch.int32, device=dev)}
g = captured(lambda: env.solve_ik(out=out), args.calls)
us = median([timed(g.replay) / args.calls for _ in range(args.rounds)])
its = out["iterations"].cpu()
hist = torch.bincount(its).tolist()
# the wave runs until its slowest lane stops: what the kernel executes is 64 x the maximum of each wave
pad = (-n) % 64
wave_iters = torch.cat([its, its.new_zeros(pad)]).view(-1, 64).max(dim=1).values.sum().item() * 64
print(json.dumps({"table": 2, "envs": n, "us_per_call_graph": us, "iterations_histogram": hist,
                  "mean_iterations": float(its.float().mean()), "us_per_iteration_env": us / float(its.sum()),
                  "ns_per_executed_iteration_lane": us * 1e3 / wave_iters,
                  "unreachable_share": float((out["residual"] > env.config.done_distance).float().mean()),
                  "not_converged_share": float((its == 32).float().mean())}), flush=True)
env.close()
