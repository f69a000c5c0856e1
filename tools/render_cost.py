#!/usr/bin/env python3
"""Cost of pnr_render (PioneerVectorEnv.render_frames): device-event time per call into preallocated outputs, the
median of alternated rounds, for
  a  4 096 envs x 84 x 84 RGB, default camera at distance 60, box + plane scene (the pixel-observation shape)
  b  65 536 envs x 64 x 64 RGB + segmentation, same scene
  c  one env at 1280 x 800 through the façade (render("rgb_array") with EngineConfig.renderer = "engine", copy to the host
     included) next to the host stick figure (render_rgb) on the same box.
--cameras times the per-env cameras instead (pnr_render_cameras): case a through the shared camera, through the same
camera given as a row per env, and through a camera on each env's pointer, alternated in the same rounds.
Prints one JSON line per case: us per call, G pixels / s, output bytes / s and their share of the 8 TB/s HBM peak.
Kernel-only times: run the same cases under `rocprofv3 --kernel-trace --stats -- python tools/render_cost.py --rounds 5`."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM = 8e12


def scene():
    from pioneer_amd.config import scene_box, scene_plane
    return [(scene_box((1.0, 1.0, 3.0), (10.0, 5.0, 0.0)), (0.3, 0.3, 0.3, 1.0)),
            (scene_plane((0.0, 0.0, 1.0), (0.0, 0.0, -0.5)), (0.4, 0.4, 0.4, 1.0))]


def batch_setup(name, n, W, H, seg):
    from pioneer_amd import PioneerVectorEnv, RenderConfig
    env = PioneerVectorEnv(n, device="cuda:0", seed=0)
    env.reset()
    cfg = RenderConfig(render_width=W, render_height=H, camera_distance=60.0)
    out = {"rgb": torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda:0")}
    if seg:
        out["seg"] = torch.empty((n, H, W), dtype=torch.uint8, device="cuda:0")
    bodies = scene()
    run = lambda: env.render_frames(cfg, bodies=bodies, segmentation=seg, out=out)  # noqa: E731
    for _ in range(3):
        run()
    return dict(name=name, env=env, run=run, n=n, W=W, H=H, seg=seg, times=[])


def camera_setups(n=4096, W=84, H=84):
    """--cameras: case a's batch three times over, one env batch and one output: the shared world camera (pnr_render), the same
    camera as a row per env through the camera form (pnr_render_cameras: the same picture, so the difference is the form's own
    cost), and a camera mounted on each env's pointer (another picture: near geometry fills the screen, the rectangles cull less)."""
    from pioneer_amd import PioneerVectorEnv, RenderConfig, render
    env = PioneerVectorEnv(n, device="cuda:0", seed=0)
    env.reset()
    cfg = RenderConfig(render_width=W, render_height=H, camera_distance=60.0)
    wrist = RenderConfig(render_width=W, render_height=H, projection_fov=60.0, projection_near=0.05)
    out = {"rgb": torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda:0")}
    bodies = scene()
    rows = torch.as_tensor(render.camera_pose(render.view_matrix(cfg)), dtype=torch.float32, device="cuda:0").repeat(n, 1).contiguous()
    mount = torch.tensor([0.0, 0.0, 0.3, 1.0, 0.0, 0.0, 0.0], dtype=torch.float32, device="cuda:0")
    runs = {"a_shared_camera": lambda: env.render_frames(cfg, bodies=bodies, out=out),
            "a_same_camera_per_env_rows": lambda: env.render_frames(cfg, bodies=bodies, out=out, cameras=rows),
            "a_pointer_mount": lambda: env.render_frames(wrist, bodies=bodies, out=out, camera_link=10, cameras=mount)}
    cases = []
    for name, run in runs.items():
        for _ in range(3):
            run()
        cases.append(dict(name=name, env=env, run=run, n=n, W=W, H=H, seg=False, times=[]))
    return cases


def time_round(c, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        c["run"]()
    b.record()
    b.synchronize()
    c["times"].append(a.elapsed_time(b) * 1e3 / calls)


def batch_result(c):
    us = float(np.median(c["times"]))
    px = c["n"] * c["W"] * c["H"]
    nbytes = px * (4 if c["seg"] else 3)
    c["env"].close()
    return dict(case=c["name"], envs=c["n"], size=[c["W"], c["H"]], outputs="rgb+seg" if c["seg"] else "rgb", us_per_call=round(us, 1),
                us_rounds=[round(t, 1) for t in c["times"]], gpix_per_s=round(px / us / 1e3, 2),
                out_bytes_per_s=round(nbytes / (us * 1e-6)), hbm_share=round(nbytes / (us * 1e-6) / HBM, 3))


def facade_case(rounds):
    from pioneer_amd import EngineConfig, PioneerKinematicEnv
    from pioneer_amd.render import render_rgb
    eng = PioneerKinematicEnv(engine_config=EngineConfig(renderer="engine"))
    host = PioneerKinematicEnv()
    for e in (eng, host):
        e.reset()
        e.render("rgb_array")
    t_eng, t_host = [], []
    for _ in range(rounds):                                 # alternated: engine, host stick figure
        t0 = time.perf_counter(); frame = eng.render("rgb_array"); t_eng.append(time.perf_counter() - t0)
        st = host._state()
        t0 = time.perf_counter(); render_rgb(st["r"][0], st["target"][0], host.render_config); t_host.append(time.perf_counter() - t0)
    assert frame.shape == (800, 1280, 3)
    e, h = float(np.median(t_eng)) * 1e6, float(np.median(t_host)) * 1e6
    eng.close(); host.close()
    return dict(case="c", envs=1, size=[1280, 800], engine_us=round(e, 1), host_stick_figure_us=round(h, 1), speedup=round(h / e, 1))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="launches per timed round (cases a, b)")
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--cameras", action="store_true", help="the per-env camera leg alone: case a through the shared camera, the same camera "
                    "as per-env rows, and a pointer mount")
    args = ap.parse_args()
    if args.cameras:
        cases = camera_setups()
        for _ in range(args.rounds):                        # alternated rounds
            for c in cases:
                time_round(c, args.calls)
        results = [batch_result(c) for c in cases]
        for r in results:
            r["vs_shared_camera"] = round(r["us_per_call"] / results[0]["us_per_call"], 3)
            print(json.dumps(r), flush=True)
        return
    cases = []
    if "a" in args.cases:
        cases.append(batch_setup("a", 4096, 84, 84, False))
    if "b" in args.cases:
        cases.append(batch_setup("b", 65536, 64, 64, True))
    for _ in range(args.rounds):                            # alternated rounds
        for c in cases:
            time_round(c, args.calls)
    for c in cases:
        print(json.dumps(batch_result(c)), flush=True)
    if "c" in args.cases:
        print(json.dumps(facade_case(args.rounds)), flush=True)


if __name__ == "__main__":
    main()
