"""Cost of pnr_retime_path and pnr_sample_trajectory against the same law written in torch on the device: device events around
graph-replayed calls after a warm-up.

65 536 envs, a path per env (per-joint sinusoids, tests/retime_cases.py's SMOOTH recipe), C = 17, 33 and 256 points, with and
without torque rows (tau_max 3 000 for every joint: never infeasible, often active).  Per point, timed on the same inputs:
  retime              one pnr_retime_path call (with torque rows: the rows launch, then the passes) writing summary, times, sdot2
  sample x 64         one pnr_sample_trajectory call of 64 steps
  torch               the yardstick, what a caller can write today: 2 (C - 1) sequential steps of batched [N, R, R] tensor
                      operations (R = 7 or 13: the pair rule backward, the greedy pass forward, the times), float32.  Its torque
                      rows are READ from the call's own workspace and their cost (3 C inverse-dynamics launches for a caller)
                      is NOT in its time, which favours the yardstick.
All variants of a point are replayed in turn, round by round, in one process; reported are the median round with the smallest and
the largest, us per call.  The recompute form of the passes (torque rows by rnea inside both passes instead of the workspace)
is not built, so there is nothing to compare the workspace form with.
Usage: python tools/retime_cost.py [--envs N] [--rounds R] [--points 17,33,256]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pioneer_amd import EngineConfig, PioneerVectorEnv, SimulationConfig, _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--points", type=str, default="17,33,256")
args = ap.parse_args()
dev = torch.device("cuda:0")
n = args.envs
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
V_MAX, A_MAX, TAU_MAX, STEPS = 2.0, 10.0, 3000.0, 64


def timed(fn):
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3                 # us


def captured(fn):
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        fn()                                         # warm-up on the capture stream
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            fn()
    torch.cuda.synchronize()
    g.replay()
    return g


def smooth(Cn, seed=1):
    rng = np.random.default_rng(seed)
    lim = np.array([3.1416, 1.309, 1.309, 3.1416, 1.5708, 3.1416])
    centre = rng.uniform(-0.3, 0.3, size=(n, 1, 6)) * lim
    amp = rng.uniform(0.1, 0.6, size=(n, 1, 6)) * rng.choice([-1.0, 1.0], size=(n, 1, 6))
    f = rng.uniform(0.3, 1.0, size=(n, 1, 6))
    s = (np.arange(Cn) / (Cn - 1))[None, :, None]
    return torch.from_numpy((centre + amp * np.sin(np.pi * f * (s - 0.5))).astype(np.float32)).to(dev)


inf = torch.tensor(float("inf"), device=dev)      # (made here: a host-to-device copy cannot be captured)


def torch_law(P, rows, lim_t, out_x, out_t):
    """The law of include/pioneer_amd.h in torch, float32, n envs at once.  rows: None or the workspace [C, 18, n]."""
    Cn = P.shape[1]
    d = torch.empty_like(P)
    e = torch.zeros_like(P)
    d[:, 0] = P[:, 1] - P[:, 0]
    d[:, -1] = P[:, -1] - P[:, -2]
    d[:, 1:-1] = (P[:, 2:] - P[:, :-2]) * 0.5
    e[:, 1:-1] = (P[:, 2:] - 2.0 * P[:, 1:-1]) + P[:, :-2]
    A, B, c = d, e, torch.zeros_like(d)
    lim = torch.full((6,), A_MAX, device=dev)
    if rows is not None:
        r = rows.permute(2, 0, 1)
        A, B, c = torch.cat([A, r[..., 0:6]], dim=2), torch.cat([B, r[..., 6:12]], dim=2), torch.cat([c, r[..., 12:18]], dim=2)
        lim = torch.cat([lim, lim_t])
    neg = A < 0
    A, B, c = torch.where(neg, -A, A), torch.where(neg, -B, B), torch.where(neg, -c, c)
    ad = d.abs()
    X = torch.where(ad > 0, (V_MAX / ad) ** 2, torch.full_like(ad, float("inf"))).amin(dim=2)
    X = torch.where((ad > 0).any(dim=2), X, torch.zeros_like(X))
    R = A.shape[2]
    two, one, zero = (torch.full((n, 1), v, device=dev) for v in (2.0, 1.0, 0.0))
    off = ~torch.eye(R + 1, dtype=torch.bool, device=dev)[None]
    K = [None] * Cn
    K[Cn - 1] = torch.zeros(n, device=dev)
    for k in range(Cn - 2, -1, -1):
        la, lb = torch.cat([A[:, k], two], dim=1), torch.cat([B[:, k], one], dim=1)
        lL, lH = torch.cat([-lim - c[:, k], zero], dim=1), torch.cat([lim - c[:, k], K[k + 1][:, None]], dim=1)
        slope = la[:, :, None] * lb[:, None, :] - la[:, None, :] * lb[:, :, None]
        rhs = la[:, :, None] * lH[:, None, :] - la[:, None, :] * lL[:, :, None]
        bound = rhs / slope
        K[k] = torch.minimum(torch.where((slope > 0) & off, bound, inf).amin(dim=(1, 2)), X[:, k])
    x = torch.zeros(n, device=dev)
    t = torch.zeros(n, device=dev)
    out_x[:, 0] = x
    out_t[:, 0] = t
    for k in range(Cn - 1):
        ui = ((lim - c[:, k]) - B[:, k] * x[:, None]) / A[:, k]
        u = torch.where(A[:, k] > 0, ui, inf).amin(dim=1)
        x1 = torch.minimum(torch.clamp_min(x + 2.0 * u, 0.0), K[k + 1])
        t = t + 2.0 / (x.sqrt() + x1.sqrt())
        x = x1
        out_x[:, k + 1] = x
        out_t[:, k + 1] = t


env = PioneerVectorEnv(n, device=dev, seed=0, simulation_config=SimulationConfig(gravity=9.81),
                       engine_config=EngineConfig(mode="dynamic", auto_reset=False, max_episode_steps=0, randomize=True))
env.reset()
lim_t = torch.full((6,), TAU_MAX, device=dev)
for Cn in [int(v) for v in args.points.split(",")]:
    P = smooth(Cn)
    for torque in (False, True):
        tau = TAU_MAX if torque else None
        out = {"summary": torch.empty((n, _lib.RETIME_SUMMARY_DIM), device=dev), "times": torch.empty((n, Cn), device=dev),
               "sdot2": torch.empty((n, Cn), device=dev)}
        targets = torch.empty((n, STEPS, 12), device=dev)
        res = env.retime_path(P, V_MAX, A_MAX, tau, out=out)                          # (the workspace is allocated before the capture)
        rows = env._retime_workspaces[(Cn, n)].view(Cn, 18, n) if torque else None
        tx, tt = torch.empty((n, Cn), device=dev), torch.empty((n, Cn), device=dev)
        variants = {"retime": lambda: env.retime_path(P, V_MAX, A_MAX, tau, out=out),
                    f"sample x {STEPS}": lambda: env.sample_trajectory(P, out["times"], out["sdot2"], out["summary"], STEPS, out=targets),
                    "torch": lambda: torch_law(P, rows, lim_t, tx, tt)}
        graphs = {k: captured(fn) for k, fn in variants.items()}
        torch.cuda.synchronize()
        feasible = float((out["summary"][:, 0] > 0).float().mean())
        ok = out["summary"][:, 0] > 0
        agree = float(((tt[:, -1] - out["summary"][:, 1]).abs()[ok] <= 1e-3 * out["summary"][:, 1][ok]).float().mean())
        times = {k: [] for k in graphs}
        for _ in range(args.rounds):                     # alternating
            for k, g in graphs.items():
                times[k].append(timed(g.replay))
        for what, ts in times.items():
            med = sorted(ts)[len(ts) // 2]
            print(json.dumps({"envs": n, "points": Cn, "torque_rows": torque, "variant": what, "us_per_call_median": round(med, 1),
                              "us_min": round(min(ts), 1), "us_max": round(max(ts), 1), "rounds": len(ts),
                              "feasible_share": round(feasible, 4), "torch_duration_within_1e-3": round(agree, 4)}), flush=True)
env.close()
