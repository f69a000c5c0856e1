"""Cost of Bullet's constraint motor (pnr_set_joint_motor, PNR_CONTROL_*_CONSTRAINT): time per pnr_world_step at N envs
(default 65 536; gravity, randomised links, frame_skip 10) with the handle's own PD law on every joint, against the same handle
with six constraint motors — position motors on Bullet's defaults (the active set settles in one pass) and velocity motors with
a force too small to reach their target (every joint clamped: two passes).  The three handles are timed in alternation, ROUNDS
times, and the median of each is reported.  Usage: python tools/world_step_motor_cost.py [N] [ROUNDS]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pioneer_amd import EngineConfig, PioneerVectorEnv, SimulationConfig, _lib  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
K = 200
dev = torch.device("cuda:0")
nan = float("nan")


def make(motor):
    env = PioneerVectorEnv(n, device=dev, seed=0, simulation_config=SimulationConfig(gravity=9.81),
                           engine_config=EngineConfig(mode="dynamic", randomize=True))
    env.reset()
    for j in range(_lib.DOF):
        if motor == "constraint":
            env.set_joint_motor(j, _lib.CONTROL_POSITION_CONSTRAINT, target_position=0.3 * (-1) ** j)
        elif motor == "constraint_saturated":
            env.set_joint_motor(j, _lib.CONTROL_VELOCITY_CONSTRAINT, target_velocity=50.0, max_force=1.0)
    return env


envs = {m: make(m) for m in ("pd", "constraint", "constraint_saturated")}
times = {m: [] for m in envs}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for env in envs.values():
    for _ in range(20):
        env.world_step()
torch.cuda.synchronize()
for _ in range(rounds):
    for m, env in envs.items():
        state = env.get_dyn_state().clone()           # each round from the same state: the saturated motors must not run away
        torch.cuda.synchronize()
        e0.record()
        for _ in range(K):
            env.world_step()
        e1.record()
        torch.cuda.synchronize()
        times[m].append(e0.elapsed_time(e1) / K * 1e3)
        assert torch.isfinite(env.get_dyn_state()[:12]).all(), m
        env.set_dyn_state(state)
med = {m: sorted(t)[len(t) // 2] for m, t in times.items()}
print(json.dumps({"envs": n, "frame_skip": 10, "us_per_world_step": med, "all_us": times,
                  "ratio_constraint": med["constraint"] / med["pd"], "ratio_constraint_saturated": med["constraint_saturated"] / med["pd"]}))
for env in envs.values():
    env.close()
