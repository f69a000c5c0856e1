"""Cost of per-env motor targets (pnr_world_step_targets): time per call at N envs (default 65 536; gravity, randomised links,
frame_skip 10) against pnr_world_step on the SAME handle with the same motor table, for a PD table (the handle's own law on every
joint) and for six constraint position motors on Bullet's defaults.  The scheme of tools/world_step_motor_cost.py: the legs are
timed in alternation, ROUNDS times, each round from the same state, and the median of each is reported.  Every baseline is timed
twice per round (`*_again`), so that its ratio against itself shows what the alternation leaves of noise; the targets legs also run
with joint torques (PD table only).  Usage: python tools/world_step_targets_cost.py [N] [ROUNDS]"""
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


def make(motor):
    env = PioneerVectorEnv(n, device=dev, seed=0, simulation_config=SimulationConfig(gravity=9.81),
                           engine_config=EngineConfig(mode="dynamic", randomize=True))
    env.reset()
    if motor == "constraint":
        for j in range(_lib.DOF):
            env.set_joint_motor(j, _lib.CONTROL_POSITION_CONSTRAINT, target_position=0.3 * (-1) ** j)
    return env


envs = {m: make(m) for m in ("pd", "constraint")}
gen = torch.Generator(device=dev).manual_seed(1)
hi = torch.as_tensor(envs["pd"].r_hi, device=dev)
targets = torch.cat([(torch.rand(n, 6, device=dev, generator=gen) * 2 - 1) * 0.3 * hi, torch.zeros(n, 6, device=dev)], dim=1).contiguous()
torques = ((torch.rand(n, 6, device=dev, generator=gen) * 2 - 1) * 10.0).contiguous()
# the constraint table's own targets in every row: the same data as the baseline, so what differs from it is the kernel alone
# (the boxed solve's pass count depends on the data)
same = torch.tensor([0.3 * (-1) ** j for j in range(6)] + [0.0] * 6, device=dev).repeat(n, 1).contiguous()
legs = {
    "pd": (envs["pd"], lambda e: e.world_step()),
    "pd_targets": (envs["pd"], lambda e: e.world_step(motor_targets=targets)),
    "pd_again": (envs["pd"], lambda e: e.world_step()),
    "pd_targets_torques": (envs["pd"], lambda e: e.world_step(motor_targets=targets, joint_torques=torques)),
    "pd_torques": (envs["pd"], lambda e: e.world_step(joint_torques=torques)),
    "constraint": (envs["constraint"], lambda e: e.world_step()),
    "constraint_targets": (envs["constraint"], lambda e: e.world_step(motor_targets=targets)),
    "constraint_again": (envs["constraint"], lambda e: e.world_step()),
    "constraint_targets_same": (envs["constraint"], lambda e: e.world_step(motor_targets=same)),
}
times = {m: [] for m in legs}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
start = {m: env.get_dyn_state().clone() for m, env in envs.items()}
for m, (env, call) in legs.items():
    for _ in range(20):
        call(env)
torch.cuda.synchronize()
for _ in range(rounds):
    for m, (env, call) in legs.items():
        env.set_dyn_state(start["pd" if m.startswith("pd") else "constraint"])    # each leg of each round from the same state
        torch.cuda.synchronize()
        e0.record()
        for _ in range(K):
            call(env)
        e1.record()
        torch.cuda.synchronize()
        times[m].append(e0.elapsed_time(e1) / K * 1e3)
        assert torch.isfinite(env.get_dyn_state()[:12]).all(), m
med = {m: sorted(t)[len(t) // 2] for m, t in times.items()}
print(json.dumps({"envs": n, "frame_skip": 10, "us_per_call": med, "all_us": times,
                  "ratio_pd_targets": med["pd_targets"] / med["pd"], "ratio_pd_again": med["pd_again"] / med["pd"],
                  "ratio_pd_targets_torques_vs_torques": med["pd_targets_torques"] / med["pd_torques"],
                  "ratio_constraint_targets": med["constraint_targets"] / med["constraint"],
                  "ratio_constraint_again": med["constraint_again"] / med["constraint"],
                  "ratio_constraint_targets_same": med["constraint_targets_same"] / med["constraint"]}))
for env in envs.values():
    env.close()
