"""Cost of pnr_world_step_wrenches (PioneerVectorEnv.world_step(link_wrenches=...)): device events around K back-to-back
graph-replayed calls after a warm-up, the median of ROUNDS, at N envs (default 65 536 and 1 048 576) on a dynamics-mode handle
(gravity, the env-wide PD motors, no contacts).  Measured in the same run as pnr_world_step_torques at the same size, alternating
round by round: the yardstick (the same sub-steps with six joint torques per env).  Rows: the torque call; K = 1 link-frame; K = 1
world-frame; K = 4 mixed frames; K = 4 mixed frames together with joint torques.  Every call is one World.step of frame_skip = 10
sub-steps; the state runs on from call to call (the arithmetic does not depend on the values).
Usage: python tools/external_force_cost.py [N ...] [--rounds R] [--calls K]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pioneer_amd import EngineConfig, PioneerVectorEnv, SimulationConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("sizes", nargs="*", type=int, default=[65536, 1048576])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=20)
args = ap.parse_args()
dev = torch.device("cuda:0")
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
MIXED = [(3, "link"), (5, "world"), (7, "link"), (10, "world")]


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
    env = PioneerVectorEnv(n, device=dev, seed=0, simulation_config=SimulationConfig(gravity=9.81),
                           engine_config=EngineConfig(mode="dynamic", auto_reset=False, max_episode_steps=0))
    env.reset()
    gen = torch.Generator(device=dev).manual_seed(1)
    tau = torch.randn((n, 6), dtype=torch.float32, device=dev, generator=gen)
    w1 = torch.randn((n, 1, 9), dtype=torch.float32, device=dev, generator=gen)
    w4 = torch.randn((n, 4, 9), dtype=torch.float32, device=dev, generator=gen)
    cases = {
        "torques": lambda: env.world_step(joint_torques=tau),
        "k1_link": lambda: env.world_step(link_wrenches=([(10, "link")], w1)),
        "k1_world": lambda: env.world_step(link_wrenches=([(10, "world")], w1)),
        "k4_mixed": lambda: env.world_step(link_wrenches=(MIXED, w4)),
        "k4_mixed_torques": lambda: env.world_step(joint_torques=tau, link_wrenches=(MIXED, w4)),
    }
    graphs = {k: captured(fn, args.calls) for k, fn in cases.items()}
    times = {k: [] for k in graphs}
    for _ in range(args.rounds):                     # alternating
        for k, g in graphs.items():
            times[k].append(timed(g.replay) / args.calls)
    row = {"envs": n, "frame_skip": env.simulation_config.frame_skip}
    base = median(times["torques"])
    for k in cases:
        us = median(times[k])
        row[k] = {"us_per_call_graph": us, "all_us": times[k], "ratio_to_torques": us / base}
    print(json.dumps(row), flush=True)
    del graphs
    env.close()
