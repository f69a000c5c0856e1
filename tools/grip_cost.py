"""Cost of the grip (pnr_set_body_grip_params): time per plain pnr_world_step at N envs (default 65 536; frame_skip 10) of a handle
with a sphere of mass 2 and radius 0.5 at each env's anchor point, in four configurations: the grip NEVER enabled, DISABLED after
use (both launch the kernels without the grip), enabled with every env RELEASED, enabled with every env GRIPPED.  Twice: in the
world of tests/moving_sphere_cases.py's family A (gravity, ground, pointer-only contacts: the kernels' PHYS 1) and of family B (link
contacts, scene plane and box, randomised links, inertia-scaled motors: PHYS 3).  The four handles are timed in alternation, ROUNDS
blocks of BLOCK steps each, every block from the same restored state, after WARM warm-up steps; the median of each is reported.
Usage: python tools/grip_cost.py [N] [ROUNDS]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import moving_sphere_cases as msc  # noqa: E402
from gpu_support import engine_config_from_oracle_names  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 15
BLOCK, WARM = 100, 30
CONFIGS = ("never", "disabled", "released", "gripped")


def make(family, config):
    from pioneer_amd import PioneerVectorEnv, SimulationConfig
    f = msc.FAMILIES[family]
    env = PioneerVectorEnv(N, device="cuda:0", seed=f["seed"], simulation_config=SimulationConfig(gravity=f["gravity"], frame_skip=10),
                           engine_config=engine_config_from_oracle_names(dict(f["dyn"]), auto_reset=False, max_episode_steps=0))
    env.reset()
    d = env.get_dyn_state()
    d[0:6] = env.get_state().view(torch.float32)[12:18]               # the arm at its command state, at rest
    d[6:12] = 0.0
    env.set_dyn_state(d)
    env.set_body(mass=2.0, radius=0.5, position=(0.0, 0.0, 0.0), velocity=(0.0, 0.0, 0.0))
    if config == "disabled":
        env.set_body_grip(max_force=1e4)
        env.world_step()
        env.set_body_grip(False)
    elif config == "released":
        env.set_body_grip(max_force=0.0)
    elif config == "gripped":
        env.set_body_grip(max_force=1e4)
    env.set_dyn_state(d)
    env.set_body(position=env.grip_anchor(), velocity=(0.0, 0.0, 0.0))
    return env, env.get_dyn_state().clone(), env.body_state().clone()


def block(env, d0, b0):
    env.set_dyn_state(d0)
    env.set_body_state(b0)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(BLOCK):
        env.world_step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / BLOCK          # us per world step


out = {}
for family, phys in (("A", 1), ("B", 3)):
    envs = {c: make(family, c) for c in CONFIGS}
    for c in CONFIGS:
        for _ in range(WARM):
            envs[c][0].world_step()
    times = {c: [] for c in CONFIGS}
    for r in range(ROUNDS):
        for c in (CONFIGS if r % 2 == 0 else CONFIGS[::-1]):
            times[c].append(block(*envs[c]))
    for c in CONFIGS:
        t = np.array(times[c])
        out[f"phys{phys}_{c}"] = dict(median_us=float(np.median(t)), min_us=float(t.min()), max_us=float(t.max()))
        print(f"PHYS {phys} {c:9s}: median {np.median(t):8.2f} us per world step (min {t.min():.2f}, max {t.max():.2f}; {ROUNDS} blocks of {BLOCK})", flush=True)
    for c in CONFIGS:
        envs[c][0].close()
print(json.dumps(out))
