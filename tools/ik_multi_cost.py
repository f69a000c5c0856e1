"""Cost of pnr_solve_ik_multi (PioneerVectorEnv.solve_ik_multi) into preallocated outputs, pose task, full orientation: device
events around K back-to-back graph-replayed calls after a warm-up.

65 536 envs; the poses are those of joints at 0.8-0.9 of the limits (the FK poses come from pnr_get_link_states, as in
tools/ik_cost.py's "rest" set); the starts are the default table (scene.ik_start_table).  Per S in 1, 8, 16, 64 three variants are
timed on the same inputs: policy BEST, policy FIRST, and what a caller does without the call ("today"): S launches of
pnr_solve_ik_pose, each from one row of the table (the selection in torch that would follow is NOT in the time).  All variants
of all S are replayed in turn, block by block, in one process; reported are the median block with the smallest and the largest,
us per call (today: per S launches), the share of envs with a converged start and the winner's mean iterations.
Usage: python tools/ik_multi_cost.py [--envs N] [--blocks B] [--starts S ...]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pioneer_amd import PioneerVectorEnv  # noqa: E402
from pioneer_amd.scene import ik_start_table  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--starts", nargs="*", type=int, default=[1, 8, 16, 64])
args = ap.parse_args()
dev = torch.device("cuda:0")
n = args.envs
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


env = PioneerVectorEnv(n, device=dev, seed=0)
gen = torch.Generator(device="cpu").manual_seed(1)
limits = torch.from_numpy(env.r_hi).float()
uniform = lambda lo, hi, *shape: lo + (hi - lo) * torch.rand(*shape, generator=gen)  # noqa: E731
q_t = uniform(-1.0, 1.0, n, 6) * uniform(0.8, 0.9, n, 1) * limits
pointer = env.link_states(torch.cat([q_t, torch.zeros(n, 6)], dim=1).to(dev))[:, 10]
pos, quat = pointer[:, 0:3].contiguous(), pointer[:, 3:7].contiguous()

graphs, calls, outs = {}, {}, {}
for S in args.starts:
    K = max(2, 32 // S)
    table = torch.from_numpy(ik_start_table(S)).to(dev)
    for policy in ("best", "first"):
        env.solve_ik_multi(quat, pos, starts=S)                                  # (the table reaches the device before the capture)
        out = {k: torch.empty_like(v) for k, v in env.solve_ik_multi(quat, pos, starts=S).items()}
        graphs[(S, policy)] = captured(lambda S=S, policy=policy, out=out: env.solve_ik_multi(quat, pos, starts=S, policy=policy, out=out), K)
        calls[(S, policy)], outs[(S, policy)] = K, out
    rows = [table[k].expand(n, 6).contiguous() for k in range(S)]
    one = {"q": torch.empty((n, 6), device=dev), "residual": torch.empty(n, device=dev), "angle": torch.empty(n, device=dev),
           "iterations": torch.empty(n, dtype=torch.int32, device=dev)}

    def today(rows=rows, one=one):
        for r in rows:
            env.solve_ik_pose(quat, pos, r, out=one)
    graphs[(S, "today")] = captured(today, K)
    calls[(S, "today")] = K

times = {k: [] for k in graphs}
for _ in range(args.blocks):                         # alternating
    for k, g in graphs.items():
        times[k].append(timed(g.replay) / calls[k])
for (S, what), ts in times.items():
    row = {"envs": n, "starts": S, "variant": what, "us_per_call_median": sorted(ts)[len(ts) // 2], "us_min": min(ts), "us_max": max(ts),
           "calls_per_block": calls[(S, what)], "blocks": len(ts)}
    if what != "today":
        o = outs[(S, what)]
        row["converged_share"] = float((o["converged"] > 0).float().mean())
        row["winner_mean_iterations"] = float(o["iterations"].float().mean())
        row["mean_converged_starts"] = float(o["converged"].float().mean())
    print(json.dumps(row), flush=True)
env.close()
