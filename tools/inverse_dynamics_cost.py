"""Cost of pnr_inverse_dynamics, pnr_mass_matrix and pnr_world_step_torques (PioneerVectorEnv.inverse_dynamics / mass_matrix /
world_step(joint_torques=...)) into preallocated outputs: device events around K back-to-back graph-replayed calls after a
warm-up, the median of ROUNDS.

Table 1: pnr_inverse_dynamics (a caller's [N, 12] joint buffer and [N, 6] accelerations on a dynamics-mode handle with
randomised links, gravity and the joint losses) and pnr_mass_matrix at N envs (default 65 536 and 1 048 576), measured in the same
run as pnr_get_jacobian at the same size, alternating round by round.  Bytes per env, counted from the shapes: inverse dynamics
48 (joints) + 24 (accelerations) + 92 (11 scales, 6 friction, 6 damping) + 24 (torques) = 188; mass matrix 48 + 44 + 144 = 236;
Jacobian 48 + 144 = 192.
Table 2: pnr_world_step_torques against pnr_world_step on the same handle (PD law with zero gains, gravity, randomised links, no
contacts), alternating.  Usage: python tools/inverse_dynamics_cost.py [N ...] [--rounds R] [--calls K]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pioneer_amd import EngineConfig, PioneerVectorEnv, SimulationConfig, _lib  # noqa: E402

HBM_PEAK = 8.0e12
BYTES = {"inverse_dynamics": 48 + 24 + 4 * (11 + 6 + 6) + 24, "mass_matrix": 48 + 4 * 11 + 144, "jacobian": 48 + 144}

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


def alternating(graphs):
    times = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for k, g in graphs.items():
            times[k].append(timed(g.replay) / args.calls)
    return times


for n in args.sizes:
    env = PioneerVectorEnv(n, device=dev, seed=0, simulation_config=SimulationConfig(gravity=9.81),
                           engine_config=EngineConfig(mode="dynamic", auto_reset=False, max_episode_steps=0, randomize=True))
    env.reset()
    for j in range(6):                               # zero gains: the joints are driven by the torques alone
        env.set_joint_motor(j, _lib.CONTROL_VELOCITY, target_velocity=0.0, velocity_gain=0.0, max_force=0.0)
    js = torch.randn((n, 12), dtype=torch.float32, device=dev)
    acc = torch.randn((n, 6), dtype=torch.float32, device=dev)
    tau = torch.empty((n, 6), dtype=torch.float32, device=dev)
    mm = torch.empty((n, 6, 6), dtype=torch.float32, device=dev)
    jac = torch.empty((n, 6, 6), dtype=torch.float32, device=dev)
    times = alternating({"inverse_dynamics": captured(lambda: env.inverse_dynamics(acc, js, joint_losses=True, out=tau), args.calls),
                         "mass_matrix": captured(lambda: env.mass_matrix(js, out=mm), args.calls),
                         "jacobian": captured(lambda: env.jacobian(joint_state=js, out=jac), args.calls)})
    row = {"table": 1, "envs": n}
    for k, b in BYTES.items():
        us = median(times[k])
        row[k] = {"us_per_call_graph": us, "all_us": times[k], "bytes_per_env": b, "TBps": n * b / (us * 1e-6) / 1e12,
                  "frac_of_8TBps": n * b / (us * 1e-6) / HBM_PEAK}
    print(json.dumps(row), flush=True)
    # the world step with and without the torque input: the same handle, the state restored before each round
    d0 = env.get_dyn_state().clone()
    zero = torch.zeros((n, 6), dtype=torch.float32, device=dev)
    graphs = {"world_step_torques": captured(lambda: env.world_step(joint_torques=zero), args.calls),
              "world_step": captured(lambda: env.world_step(), args.calls)}
    times = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for k, g in graphs.items():
            env.set_dyn_state(d0)
            times[k].append(timed(g.replay) / args.calls)
    row = {"table": 2, "envs": n}
    for k in graphs:
        row[k] = {"us_per_call_graph": median(times[k]), "all_us": times[k]}
    row["torques_over_plain"] = row["world_step_torques"]["us_per_call_graph"] / row["world_step"]["us_per_call_graph"]
    print(json.dumps(row), flush=True)
    del graphs
    env.close()
