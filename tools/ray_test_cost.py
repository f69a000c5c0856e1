#!/usr/bin/env python3
"""Cost of pnr_ray_test (PioneerVectorEnv.ray_test): device-event time per call into preallocated outputs, the median
of alternated rounds, over the box + plane scene of tools/render_cost.py, for
  a  65 536 envs x 32 rays in the pointer's frame (scene.ray_fan), arm + target + bodies, hits + fractions
  b  4 096 envs x 1 024 world rays (one origin above the scene, a grid of end points), arm + target + bodies, hits + fractions
  c  65 536 envs x 32 pointer-frame rays, bodies only
Prints one JSON line per case: us per call, G rays / s, output bytes / s and their share of the 8 TB/s HBM peak.  The yardstick is
pnr_render's pixels / s (tools/render_cost.py case b: the same primitives, one ray per pixel) measured in the same session.
Kernel-only times: run the same cases under `rocprofv3 --kernel-trace --stats -- python tools/ray_test_cost.py --rounds 5`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM = 8e12


def scene():
    from pioneer_amd.config import scene_box, scene_plane
    return [scene_box((1.0, 1.0, 3.0), (10.0, 5.0, 0.0)), scene_plane((0.0, 0.0, 1.0), (0.0, 0.0, -0.5))]


def world_grid(side):
    """side x side rays from one point above the scene to a grid on z = -1."""
    x, y = np.meshgrid(np.linspace(-25.0, 25.0, side), np.linspace(-25.0, 25.0, side))
    to = np.stack([x.ravel(), y.ravel(), np.full(side * side, -1.0)], axis=1)
    return np.concatenate([np.tile((30.0, -20.0, 25.0), (side * side, 1)), to], axis=1).astype(np.float32)


def setup(name, n, rays, parent_link, arm, target):
    from pioneer_amd import PioneerVectorEnv
    env = PioneerVectorEnv(n, device="cuda:0", seed=0)
    env.reset()
    rays = torch.from_numpy(rays).cuda()
    R = rays.shape[0]
    out = {"hits": torch.empty((n, R, 8), dtype=torch.float32, device="cuda:0"), "fractions": torch.empty((n, R), dtype=torch.float32, device="cuda:0")}
    bodies = scene()
    run = lambda: env.ray_test(rays, parent_link=parent_link, hit_arm=arm, hit_target=target, bodies=bodies, fractions=True, out=out)  # noqa: E731
    for _ in range(3):
        run()
    return dict(name=name, env=env, run=run, n=n, R=R, mask=("arm+target+bodies" if arm else "bodies"), parent_link=parent_link, times=[])


def time_round(c, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        c["run"]()
    b.record()
    b.synchronize()
    c["times"].append(a.elapsed_time(b) * 1e3 / calls)


def result(c):
    us = float(np.median(c["times"]))
    nrays = c["n"] * c["R"]
    nbytes = nrays * 36
    c["env"].close()
    return dict(case=c["name"], envs=c["n"], rays_per_env=c["R"], parent_link=c["parent_link"], hit=c["mask"], us_per_call=round(us, 1),
                us_rounds=[round(t, 1) for t in c["times"]], grays_per_s=round(nrays / us / 1e3, 2),
                out_bytes_per_s=round(nbytes / (us * 1e-6)), hbm_share=round(nbytes / (us * 1e-6) / HBM, 3))


def main():
    from pioneer_amd.scene import ray_fan
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="launches per timed round")
    ap.add_argument("--cases", default="abc")
    args = ap.parse_args()
    cases = []
    if "a" in args.cases:
        cases.append(setup("a", 65536, ray_fan(32, 40.0, start=0.25), 10, True, True))
    if "b" in args.cases:
        cases.append(setup("b", 4096, world_grid(32), -1, True, True))
    if "c" in args.cases:
        cases.append(setup("c", 65536, ray_fan(32, 40.0, start=0.25), 10, False, False))
    for _ in range(args.rounds):                            # alternated rounds
        for c in cases:
            time_round(c, args.calls)
    for c in cases:
        print(json.dumps(result(c)), flush=True)


if __name__ == "__main__":
    main()
