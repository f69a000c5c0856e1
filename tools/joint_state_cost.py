"""Cost of pnr_get_joint_states (PioneerVectorEnv.joint_states) into preallocated outputs: device events around K back-to-back
graph-replayed calls after a warm-up, the median of ROUNDS, alternating round by round with its two yardsticks on the same handle:
pnr_inverse_dynamics (a Newton-Euler sweep alone) and one pnr_world_step of a frame_skip = 1 handle (one sub-step alone).

The handle: dynamics mode, frame_skip 1, gravity, randomised links, the env-wide PD motors; then the same with a ground plane and
link contacts (the contact instantiation).  The query is timed with and without reaction_out, plain and with four wrench records
and joint torques.  Usage: python tools/joint_state_cost.py [N ...] [--rounds R] [--calls K]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pioneer_amd import EngineConfig, PioneerVectorEnv, SimulationConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("sizes", nargs="*", type=int, default=[65536])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=100)
args = ap.parse_args()
dev = torch.device("cuda:0")
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
SPECS = [(3, "link"), (5, "world"), (7, "link"), (10, "world")]


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
    for contacts in (False, True):
        eng = dict(ground_z=0.0, link_contacts=True) if contacts else {}
        env = PioneerVectorEnv(n, device=dev, seed=0, simulation_config=SimulationConfig(gravity=9.81, frame_skip=1),
                               engine_config=EngineConfig(mode="dynamic", auto_reset=False, max_episode_steps=0, randomize=True, **eng))
        env.reset()
        d0 = env.get_dyn_state().clone()
        tau = torch.randn((n, 6), dtype=torch.float32, device=dev)
        wr = torch.randn((n, len(SPECS), 9), dtype=torch.float32, device=dev)
        out = dict(joints=torch.empty((n, 6, 4), dtype=torch.float32, device=dev), reaction=torch.empty((n, 6, 6), dtype=torch.float32, device=dev))
        lean = dict(joints=out["joints"])
        idt = torch.empty((n, 6), dtype=torch.float32, device=dev)
        graphs = {
            "joint_states": captured(lambda: env.joint_states(out=out), args.calls),
            "joint_states_no_reaction": captured(lambda: env.joint_states(reaction=False, out=lean), args.calls),
            "joint_states_wrenches_torques": captured(lambda: env.joint_states(joint_torques=tau, link_wrenches=(SPECS, wr), out=out), args.calls),
            "joint_states_wrenches_torques_no_reaction": captured(
                lambda: env.joint_states(joint_torques=tau, link_wrenches=(SPECS, wr), reaction=False, out=lean), args.calls),
            "inverse_dynamics": captured(lambda: env.inverse_dynamics(joint_losses=True, out=idt), args.calls),
            "world_step": captured(lambda: env.world_step(), args.calls),
        }
        times = {k: [] for k in graphs}
        for _ in range(args.rounds):
            for k, g in graphs.items():
                env.set_dyn_state(d0)                # the world step moves the state: every round starts from the same one
                times[k].append(timed(g.replay) / args.calls)
        row = {"envs": n, "contacts": contacts, "calls": args.calls, "rounds": args.rounds}
        for k in graphs:
            row[k] = {"us_per_call_graph": median(times[k]), "all_us": times[k]}
        base = row["world_step"]["us_per_call_graph"]
        row["joint_states_over_world_step"] = row["joint_states"]["us_per_call_graph"] / base
        print(json.dumps(row), flush=True)
        del graphs
        env.close()
