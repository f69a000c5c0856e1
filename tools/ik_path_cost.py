"""Cost of pnr_solve_ik_path against what a caller does today on the same targets: device events around graph-replayed calls after
a warm-up.

65 536 envs, two input families: LINE (position task: K waypoints uniform in the inner box (15, -8, 2)..(22, 8, 6), from the rest
pose) and HOLD (pose task: the pose of random joints q_t, the orientation held while the position moves 1 along a random
direction per segment, from q_t + U(-0.2, 0.2)).  (K, M) = (2, 8) and (5, 8), C = 9 and 33 configurations; S = 1 and 8 starts.
Per point, timed on the same inputs:
  path/summary        one pnr_solve_ik_path call, the summary alone
  path/rows=launch    .. with q_path, the winner's rows by a second launch (S = 1: written as the start is tracked)
  path/rows=pass      .. with q_path, the winner's rows by a second pass inside the launch (S > 1 only)
  multi x C           the yardstick: C chained pnr_solve_ik_multi(starts = 1, q_init = the row before) launches on the same
                      interpolated targets, max_iterations 32 for the first and 8 for the others; for S = 8 the first is one
                      8-start launch and the others start from its winner.  The torch interpolation of the targets and the
                      bookkeeping (did it stay on the line, travel) that would surround them are NOT in the time, which favours
                      the yardstick.
All variants of a point are replayed in turn, round by round, in one process; reported are the median round with the smallest and
the largest, us per call (the yardstick: per C launches).
Usage: python tools/ik_path_cost.py [--envs N] [--rounds R]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pioneer_amd import PioneerVectorEnv, _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--rounds", type=int, default=7)
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
limits = torch.from_numpy(env.r_hi).float().to(dev)
gen = torch.Generator(device="cpu").manual_seed(1)
rand = lambda *shape: torch.rand(*shape, generator=gen).to(dev)  # noqa: E731


def inputs(family, K):
    """(waypoints [n, K, 3], orientations [n, K, 4] or None, q_init [n, 6] or None)"""
    if family == "LINE":
        lo, hi = torch.tensor([15.0, -8.0, 2.0], device=dev), torch.tensor([22.0, 8.0, 6.0], device=dev)
        return (lo + (hi - lo) * rand(n, K, 3)).contiguous(), None, None
    q_t = (2.0 * rand(n, 6) - 1.0) * 0.8 * limits
    q_t[:, 4] = torch.where(rand(n) < 0.5, -1.0, 1.0) * (0.4 + 0.8 * rand(n))
    pose = env.link_states(torch.cat([q_t, torch.zeros_like(q_t)], dim=1).contiguous())[:, 10]
    d = torch.randn(n, K, 3, generator=gen).to(dev)
    d = d / d.norm(dim=2, keepdim=True)
    d[:, 0] = 0.0
    pos = (pose[:, None, 0:3] + torch.cumsum(d, dim=1)).contiguous()
    quat = pose[:, None, 3:7].expand(n, K, 4).contiguous()
    return pos, quat, (q_t + 0.4 * rand(n, 6) - 0.2).contiguous()


def targets(pos, quat, M):
    """The C targets by the call's own rule, as lists of [n, 3] and [n, 4] (or None) tensors."""
    tp, tq = [pos[:, 0].contiguous()], [None if quat is None else quat[:, 0].contiguous()]
    for i in range(pos.shape[1] - 1):
        for j in range(1, M + 1):
            u = (torch.tensor(float(j)) / torch.tensor(float(M))).item()
            a, b = pos[:, i], pos[:, i + 1]
            tp.append((b if j == M else a + u * (b - a)).contiguous())
            if quat is None:
                tq.append(None)
                continue
            qa, qb = quat[:, i], quat[:, i + 1]
            h = torch.where((qa * qb).sum(dim=1, keepdim=True) < 0, -1.0, 1.0)
            tq.append((qb if j == M else (1.0 - u) * qa + u * h * qb).contiguous())
    return tp, tq


for family in ("LINE", "HOLD"):
    for K, M in ((2, 8), (5, 8)):
        Cn = 1 + (K - 1) * M
        pos, quat, q_init = inputs(family, K)
        tp, tq = targets(pos, quat, M)
        for S in (1, 8):
            out = {"summary": torch.empty((n, _lib.IK_PATH_SUMMARY_DIM), device=dev), "q_path": torch.empty((n, Cn, 6), device=dev)}
            multi_out = [{k: torch.empty_like(v) for k, v in env.solve_ik_multi(tq[0], tp[0], starts=1).items()} for _ in range(2)]
            env.solve_ik_path(pos, quat, substeps=M, starts=S, q_init=q_init, path=False)      # (the start table reaches the device)

            def path(rows, want_path):
                env.solve_ik_path(pos, quat, substeps=M, starts=S, q_init=q_init, path=want_path, winner_rows=rows, out=out)

            def yardstick():
                prev = env.solve_ik_multi(tq[0], tp[0], starts=S, q_init=q_init, out=multi_out[0])["q"]
                for c in range(1, Cn):
                    prev = env.solve_ik_multi(tq[c], tp[c], starts=1, q_init=prev, max_iterations=8, out=multi_out[c % 2])["q"]

            reps = 4 if Cn <= 16 else 2
            variants = {"path/summary": (lambda: path(0, False), reps),
                        "path/rows=launch": (lambda: path(_lib.IK_PATH_ROWS_SECOND_LAUNCH, True), reps)}
            if S > 1:
                variants["path/rows=pass"] = (lambda: path(_lib.IK_PATH_ROWS_SECOND_PASS, True), reps)
            variants[f"multi x {Cn}"] = (yardstick, 1)
            graphs = {k: captured(fn, calls) for k, (fn, calls) in variants.items()}
            path(0, True)
            torch.cuda.synchronize()
            tracked = float((out["summary"][:, 0] > 0).float().mean())
            times = {k: [] for k in graphs}
            for _ in range(args.rounds):                     # alternating
                for k, g in graphs.items():
                    times[k].append(timed(g.replay) / variants[k][1])
            for what, ts in times.items():
                med = sorted(ts)[len(ts) // 2]
                print(json.dumps({"envs": n, "family": family, "waypoints": K, "substeps": M, "configurations": Cn, "starts": S, "variant": what,
                                  "us_per_call_median": round(med, 1), "us_min": round(min(ts), 1), "us_max": round(max(ts), 1),
                                  "calls_per_round": variants[what][1], "rounds": len(ts), "tracked_share": round(tracked, 4)}), flush=True)
env.close()
