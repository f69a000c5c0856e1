"""Cost of the scene queries' per-env world (pnr_render_bodies, pnr_set_body_queries): device-event time per call at N
envs (default 65 536) of each of the three queries in its earlier form against its new form on the same inputs, into preallocated
outputs, on ONE dynamics-mode handle with a moving sphere in every env:
  render    96 x 64 rgb + segmentation, box + sphere + plane: shared positions (pnr_render) | per-env positions | per-env positions
            and the moving sphere | shared positions and the moving sphere
  rays      32 rays per env from the pointer link, bodies + arm, per-env body positions: without | with the moving sphere
  contacts  points + summary + joint torques, per-env body positions: without | with the moving sphere
The forms are timed in alternation, ROUNDS times, and the median of each is reported.
Usage: python tools/scene_queries_cost.py [N] [ROUNDS]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pioneer_amd import EngineConfig, PioneerVectorEnv, RenderConfig  # noqa: E402
from pioneer_amd.config import scene_box, scene_plane, scene_sphere  # noqa: E402
from pioneer_amd.scene import ray_fan  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda:0")
W, H, R = 96, 64, 32

env = PioneerVectorEnv(n, device=dev, seed=0, engine_config=EngineConfig(mode="dynamic"))
env.reset()
g = torch.Generator(device=dev).manual_seed(1)
rand = lambda *shape: torch.rand(shape, device=dev, generator=g)  # noqa: E731
# a sphere in every env, in the arm's workspace and in the camera's view
env.set_body(mass=0.5 + 3.5 * rand(n), radius=1.0 + 2.0 * rand(n), position=(rand(n, 3) - 0.5) * torch.tensor([30.0, 30.0, 10.0], device=dev)
             + torch.tensor([0.0, 0.0, 6.0], device=dev), velocity=(rand(n, 3) - 0.5) * 4.0)
bodies = [(scene_box((1.0, 1.5, 3.0), (10.0, 5.0, 0.0), (0.0, 0.0, 0.38268343, 0.92387953)), (0.8, 0.2, 0.6, 1.0)),
          (scene_sphere(2.0, (-8.0, -6.0, 4.0)), (0.2, 0.7, 0.9, 1.0)), (scene_plane((0.0, 0.0, 1.0), (0.0, 0.0, -0.5)), (0.4, 0.4, 0.4, 1.0))]
plain = [b for b, _ in bodies]
bp = torch.tensor([b.position for b in plain], device=dev).repeat(n, 1, 1)
bp[:, 0:2] += (rand(n, 2, 3) - 0.5) * 6.0
cfg = RenderConfig(render_width=W, render_height=H, camera_distance=60.0)
img = {"rgb": torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev), "seg": torch.empty((n, H, W), dtype=torch.uint8, device=dev)}
rays = torch.from_numpy(ray_fan(R, 40.0, start=0.25)).to(dev)
hit = {"hits": torch.empty((n, R, 8), device=dev)}
con = {"points": torch.empty((n, 23, 9), device=dev), "summary": torch.empty((n, 4), device=dev), "joint_torques": torch.empty((n, 6), device=dev)}

render = lambda **kw: env.render_frames(cfg, bodies=bodies, segmentation=True, out=img, **kw)  # noqa: E731
cast = lambda: env.ray_test(rays, parent_link=10, hit_arm=True, bodies=plain, body_positions=bp, out=hit)  # noqa: E731
touch = lambda: env.contacts(bodies=plain, body_positions=bp, joint_torques=True, out=con)  # noqa: E731
# name -> (which queries see the sphere, the call, launches per timed round)
forms = {
    "render_shared": ({}, render, 10),
    "render_per_env": ({}, lambda: render(body_positions=bp), 10),
    "render_per_env_sphere": (dict(render=True), lambda: render(body_positions=bp), 10),
    "render_shared_sphere": (dict(render=True), render, 10),
    "rays": ({}, cast, 50),
    "rays_sphere": (dict(rays=True), cast, 50),
    "contacts": ({}, touch, 50),
    "contacts_sphere": (dict(contacts=True), touch, 50),
}
times = {m: [] for m in forms}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for bits, run, _ in forms.values():
    env.set_body_queries(**bits)
    for _ in range(3):
        run()
torch.cuda.synchronize()
for _ in range(rounds):
    for m, (bits, run, calls) in forms.items():
        env.set_body_queries(**bits)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            run()
        e1.record()
        torch.cuda.synchronize()
        times[m].append(e0.elapsed_time(e1) / calls * 1e3)
med = {m: sorted(t)[len(t) // 2] for m, t in times.items()}
seen = {"pixels_21": float((img["seg"] == 21).float().mean())}
env.set_body_queries(rays=True, contacts=True)
seen["rays_21"] = float((cast()["hits"][..., 7] == 21).float().mean())
seen["pairs_body_8"] = float((touch()["points"][..., 7] == 8).float().mean())
print(json.dumps({"envs": n, "image": [W, H], "rays_per_env": R, "us_per_call": med, "all_us": times, "share_that_sees_the_sphere": seen,
                  "ratio_render_per_env": med["render_per_env"] / med["render_shared"],
                  "ratio_render_per_env_sphere": med["render_per_env_sphere"] / med["render_shared"],
                  "ratio_render_shared_sphere": med["render_shared_sphere"] / med["render_shared"],
                  "ratio_rays": med["rays_sphere"] / med["rays"], "ratio_contacts": med["contacts_sphere"] / med["contacts"]}))
env.close()
