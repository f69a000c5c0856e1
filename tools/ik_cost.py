"""Cost of pnr_get_jacobian and pnr_solve_ik (PioneerVectorEnv.jacobian / solve_ik) into preallocated outputs: device events
around K back-to-back graph-replayed calls after a warm-up, the median of ROUNDS.

Table 1: pnr_get_jacobian at N envs (default 65 536 and 1 048 576) for a caller's [N, 12] joint buffer, measured in the same
run as pnr_get_link_states at the same size, alternating round by round; the rate is counted against (144 + 48) B per env
(link states: 572 + 48).
Table 2: pnr_solve_ik at 65 536 envs, default parameters, targets uniform in the reference's box (15, -10, 2) .. (25, 10, 6),
from the rest pose: us per call, the histogram of iterations_out, us per iteration-env, and the share of targets left further
than done_distance (unreachable).
Table 3: pnr_solve_ik_pose at the same 65 536 envs, default parameters, full orientation, on two input sets made here from a seed
(the FK poses come from pnr_get_link_states): "near" = the pose of joints U(-0.8, 0.8) x limits with |q5| in (0.4, 1.2), started
within +-0.2 rad of them; "rest" = the pose of joints at 0.8-0.9 of the limits, started from the rest pose.  Each is replayed
alternating, round by round, with Table 2's pnr_solve_ik graph: us per call of both, the iteration histogram, us per
iteration-env, ns per executed iteration-lane and the share that did not converge.
Usage: python tools/ik_cost.py [N ...] [--rounds R] [--calls K] [--ik-envs M]"""
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


def iteration_figures(us, its):
    """What a call's time means per iteration.  The wave runs until its slowest lane stops: what the kernel executes is 64 x
    the maximum of each wave."""
    pad = (-n) % 64
    wave_iters = torch.cat([its, its.new_zeros(pad)]).view(-1, 64).max(dim=1).values.sum().item() * 64
    return {"us_per_call_graph": us, "iterations_histogram": torch.bincount(its).tolist(), "mean_iterations": float(its.float().mean()),
            "us_per_iteration_env": us / float(its.sum()), "ns_per_executed_iteration_lane": us * 1e3 / wave_iters,
            "not_converged_share": float((its == 32).float().mean())}


print(json.dumps({"table": 2, "envs": n, **iteration_figures(us, out["iterations"].cpu()),
                  "unreachable_share": float((out["residual"] > env.config.done_distance).float().mean())}), flush=True)

gen = torch.Generator(device="cpu").manual_seed(1)
limits = torch.from_numpy(env.r_hi).float()
uniform = lambda lo, hi, *shape: lo + (hi - lo) * torch.rand(*shape, generator=gen)  # noqa: E731
near_q = uniform(-0.8, 0.8, n, 6) * limits
near_q[:, 4] = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0) * uniform(0.4, 1.2, n)
rest_q = uniform(-1.0, 1.0, n, 6) * uniform(0.8, 0.9, n, 1) * limits
pose_out = {k: torch.empty_like(v) for k, v in out.items()}     # its own outputs: the two graphs are replayed in turn
pose_out["angle"] = torch.empty(n, device=dev)
for name, q_t, start in (("near", near_q, near_q + uniform(-0.2, 0.2, n, 6)), ("rest", rest_q, None)):
    pointer = env.link_states(torch.cat([q_t, torch.zeros(n, 6)], dim=1).to(dev))[:, 10]
    pos, quat = pointer[:, 0:3].contiguous(), pointer[:, 3:7].contiguous()
    start = None if start is None else start.to(dev)
    gp = captured(lambda: env.solve_ik_pose(quat, pos, start, out=pose_out), args.calls)
    times = {"pose": [], "position": []}
    for _ in range(args.rounds):                     # alternating
        times["pose"].append(timed(gp.replay) / args.calls)
        times["position"].append(timed(g.replay) / args.calls)
    print(json.dumps({"table": 3, "envs": n, "set": name, **iteration_figures(median(times["pose"]), pose_out["iterations"].cpu()),
                      "all_us": times["pose"], "solve_ik_us_per_call_same_run": median(times["position"]),
                      "solve_ik_all_us": times["position"]}), flush=True)
    del gp
env.close()
