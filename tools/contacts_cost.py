"""Cost of pnr_get_contacts (PioneerVectorEnv.contacts) into preallocated outputs: device events around K back-to-back
graph-replayed calls after a warm-up, the median of ROUNDS, at N envs (default 65 536 and 1 048 576) with three shared bodies
(a plane, an oriented box, a sphere) for a caller's [N, 12] joint buffer.  Measured in the same run as pnr_get_link_states at the
same size, alternating round by round: the yardstick (same sweep over the chain, 572 B out per env).  Rows: points + summary
(counted against 828 + 16 + 48 B per env), all three outputs (+ 24 B), summary alone (16 + 48 B: what a terminate-on-touch rule
reads), points + summary with a position per env for every body (+ 36 B in), link states (572 + 48 B).
Usage: python tools/contacts_cost.py [N ...] [--rounds R] [--calls K]"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pioneer_amd import PioneerVectorEnv  # noqa: E402
from pioneer_amd.config import scene_box, scene_plane, scene_sphere  # noqa: E402

HBM_PEAK = 8.0e12
BODIES = [scene_plane((0.0, 0.0, 1.0)), scene_box((2.0, 1.5, 4.0), (12.0, 4.0, 4.0), (0.0, 0.0, math.sin(0.25), math.cos(0.25))),
          scene_sphere(3.0, (14.0, -6.0, 5.0))]

ap = argparse.ArgumentParser()
ap.add_argument("sizes", nargs="*", type=int, default=[65536, 1048576])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=100)
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
    bp = torch.tensor([b.position for b in BODIES], dtype=torch.float32, device=dev).repeat(n, 1, 1).contiguous()
    out = {"points": torch.empty((n, 23, 9), device=dev), "summary": torch.empty((n, 4), device=dev),
           "joint_torques": torch.empty((n, 6), device=dev)}
    rec = torch.empty((n, 11, 13), dtype=torch.float32, device=dev)
    cases = {
        "points_summary": (lambda: env.contacts(js, BODIES, out=out), 828 + 16 + 48),
        "all_three": (lambda: env.contacts(js, BODIES, joint_torques=True, out=out), 828 + 16 + 24 + 48),
        "summary_only": (lambda: env.contacts(js, BODIES, points=False, out=out), 16 + 48),
        "points_summary_per_env_bodies": (lambda: env.contacts(js, BODIES, body_positions=bp, out=out), 828 + 16 + 48 + 36),
        "link_states": (lambda: env.link_states(js, out=rec), 572 + 48),
    }
    graphs = {k: captured(fn, args.calls) for k, (fn, _) in cases.items()}
    times = {k: [] for k in graphs}
    for _ in range(args.rounds):                     # alternating
        for k, g in graphs.items():
            times[k].append(timed(g.replay) / args.calls)
    row = {"envs": n, "bodies": len(BODIES)}
    for k, (_, b) in cases.items():
        us = median(times[k])
        row[k] = {"us_per_call_graph": us, "all_us": times[k], "bytes_per_env": b, "TBps": n * b / (us * 1e-6) / 1e12,
                  "frac_of_8TBps": n * b / (us * 1e-6) / HBM_PEAK}
    print(json.dumps(row), flush=True)
    del graphs
    env.close()
