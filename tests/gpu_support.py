"""What the GPU tests share on the torch side, one definition each: conversions, the raw state of a handle, env makers, the motor
table, the kinematic suite's engine / oracle pair and the render and ray tests' scene.  The bars are tests/bars.py's."""
import numpy as np
import torch

from bars import POS_TOL, POT_TOL, REW_TOL, check_obs

LIMITS = np.array([3.1416, 1.309, 1.309, 3.1416, 1.5708, 3.1416], dtype=np.float32)


def lib():
    from pioneer_amd import _lib
    return _lib


# ---- conversions ------------------------------------------------------------------------------------------------------------------
def dev(x, dtype=torch.float32):
    """a device tensor (float32 unless told otherwise) of a contiguous copy"""
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype, device="cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


def f64(t):
    return t.double().cpu().numpy()


# ---- a handle's raw state -----------------------------------------------------------------------------------------------------------
def words(env):
    """the canonical state words [24, N] as uint32"""
    return env.get_state().cpu().numpy().view(np.uint32)


def dyn_words(env):
    """the dynamics words [*, N] float32: q 0-5, qd 6-11, the per-env draws 12-34"""
    return env.get_dyn_state().cpu().numpy()


def kin_joints(env):
    """(q, qd) float32 [N, 6] of a kinematic-mode env: r (state words 12-17) and v (6-11)"""
    f = env.get_state().view(torch.float32).cpu().numpy()
    return f[12:18].T.copy(), f[6:12].T.copy()


def dyn_joints(env):
    """(q, qd) float32 [N, 6] of a dynamics-mode env: dyn words 0-5 and 6-11"""
    d = dyn_words(env)
    return d[0:6].T.copy(), d[6:12].T.copy()


def load_joints(env, q, qd=None):
    """q, qd [N, 6] into a dynamics-mode env's simulated joints, rounded to float32 once; qd None = at rest"""
    d = env.get_dyn_state()
    d[0:6] = dev(np.asarray(q).T)
    d[6:12] = 0.0 if qd is None else dev(np.asarray(qd).T)
    env.set_dyn_state(d)


def set_motors(env, motors):
    """pnr_set_joint_motor for every motor dict of tests/constraint_motor_ref.py's form (kind "pd" with its control_mode,
    "position_constraint", "velocity_constraint") that is not None; None = uncommanded: the env-wide law on the command state"""
    L = lib()
    modes = {"velocity_constraint": L.CONTROL_VELOCITY_CONSTRAINT, "position_constraint": L.CONTROL_POSITION_CONSTRAINT}
    for j, m in enumerate(motors):
        if m is None:
            continue
        mode = modes.get(m["kind"])
        if mode is None:
            mode = L.CONTROL_VELOCITY if m["control_mode"] == 1 else L.CONTROL_POSITION
        env.set_joint_motor(j, mode, **{k: v for k, v in m.items() if k not in ("kind", "control_mode")})


# ---- env makers -------------------------------------------------------------------------------------------------------------------
def dyn_env(n, seed, gravity, frame_skip=10, reset=True, **eng):
    """a dynamics-mode env without auto-reset or TimeLimit, reset"""
    from pioneer_amd import EngineConfig, PioneerVectorEnv, SimulationConfig
    env = PioneerVectorEnv(n, device="cuda:0", seed=seed, simulation_config=SimulationConfig(gravity=gravity, frame_skip=frame_skip),
                           engine_config=EngineConfig(mode="dynamic", auto_reset=False, max_episode_steps=0, **eng))
    if reset:
        env.reset()
    return env


def kin_env(n, seed, reset=True, sim=None, **eng):
    """a kinematic-mode env of EngineConfig(**eng), reset; sim: SimulationConfig arguments, if any"""
    from pioneer_amd import EngineConfig, PioneerVectorEnv, SimulationConfig
    env = PioneerVectorEnv(n, device="cuda:0", seed=seed, simulation_config=SimulationConfig(**(sim or {})), engine_config=EngineConfig(**eng))
    if reset:
        env.reset()
    return env


def engine_config_from_oracle_names(dyn, **engine_kwargs):
    """A dynamics-mode EngineConfig from the oracle's `dyn` names (kp, kd, ground_z, ...; whatever is left out takes the value
    both sides default to) and further EngineConfig arguments as they are."""
    from pioneer_amd import EngineConfig
    from pioneer_amd.config import SceneBody
    ek = dict(dyn)
    eng = EngineConfig(mode="dynamic", **engine_kwargs,
                       pd_kp=ek.pop("kp", 4000.0), pd_kd=ek.pop("kd", 400.0), torque_limit=ek.pop("torque_limit", 0.0),
                       teleport=bool(ek.pop("teleport", 0)), randomize=bool(ek.pop("randomize", 0)),
                       joint_damping=ek.pop("joint_damping", 0.0), joint_friction=ek.pop("joint_friction", 0.0),
                       ground_z=ek.pop("ground_z", float("nan")),
                       contact_kp=ek.pop("contact_kp", 2000.0), contact_kd=ek.pop("contact_kd", 50.0),
                       obstacle_position=ek.pop("obstacle_position", (10.0, 5.0, 0.0)),
                       obstacle_half_extents=ek.pop("obstacle_half_extents", (0.0, 0.0, 0.0)),
                       pointer_radius=ek.pop("pointer_radius", 0.2),
                       control_mode={0: "position", 1: "velocity"}[ek.pop("control_mode", 0)],
                       max_velocity=ek.pop("max_velocity", 0.0), link_contacts=bool(ek.pop("link_contacts", 0)),
                       pd_inertia_scaled=bool(ek.pop("pd_inertia_scaled", 0)),
                       scene=tuple(SceneBody(sh, tuple(p), tuple(q), tuple(sz)) for sh, p, q, sz in ek.pop("scene", ())))
    assert not ek, f"oracle names without an EngineConfig counterpart: {sorted(ek)}"
    return eng


# ---- the kinematic suite: the engine next to the CPU oracle ----------------------------------------------------------------------------
def make_pair(n, seed=0, layout="env_major", act_layout="env_major", auto_reset=True, max_steps=500, **cfg):
    from oracle import COracle
    from oracle.binding import ORC_DEV
    from pioneer_amd import PioneerVectorEnv, EngineConfig, PioneerKinematicConfig
    env = PioneerVectorEnv(n, device="cuda:0", seed=seed,
                           pioneer_config=PioneerKinematicConfig(**cfg),
                           engine_config=EngineConfig(auto_reset=auto_reset, obs_layout=layout,
                                                      action_layout=act_layout, max_episode_steps=max_steps))
    orc = COracle(n, seed=seed, precision=ORC_DEV, auto_reset=auto_reset, max_episode_steps=max_steps,
                  nthreads=8, **cfg)
    return env, orc


def to_env_major(env, obs):
    o = obs.double().cpu().numpy()
    return o.T if env.feature_major_obs else o


def _worst(got, want):
    return float(np.abs(got - want).max())


def check_state_exact(env, orc):
    w = words(env)
    ow = orc.state_words()
    assert np.array_equal(w[:21], ow[:21]), f"a, v, r, target must be bit-exact: {int((w[:21] != ow[:21]).sum())} words differ"
    assert np.array_equal(w[22:], ow[22:]), f"step_index / episode must match: {int((w[22:] != ow[22:]).sum())} words differ"
    pot = w[21].view(np.float32).astype(np.float64)
    opot = ow[21].view(np.float32).astype(np.float64)
    worst = _worst(pot, opot)
    assert worst <= POT_TOL, f"potential: worst deviation {worst:.3e} exceeds POT_TOL {POT_TOL:.1e}"


def run_parity(n, steps, layout="env_major", act_layout="env_major", seed=3, action_scale=1.0, **kw):
    env, orc = make_pair(n, seed=seed, layout=layout, act_layout=act_layout, **kw)
    obs = env.reset()
    check_obs(to_env_major(env, obs), orc.reset())
    rng = np.random.RandomState(seed)
    for t in range(steps):
        act = (rng.uniform(-1, 1, size=(n, 6)) * env.a_max * action_scale).astype(np.float32)
        a_dev = torch.from_numpy(act.T.copy() if env.feature_major_act else act).cuda()
        obs, rew, done, trunc, info = env.vector_step(a_dev, want_info=True)
        oobs, orew, odone, otrunc, oinfo = orc.step(act, want_info=True)
        # done / truncated are bytes the caller branches on: identical for EVERY env (the engine re-evaluates the
        # predicate in float64 wherever the float32 distance comes near done_distance, pnr_device.h done_predicate)
        d, tr = done.cpu().numpy(), trunc.cpu().numpy()
        assert np.array_equal(d, odone) and np.array_equal(tr, otrunc), \
            f"step {t}: done differs in {int((d != odone).sum())} envs, truncated in {int((tr != otrunc).sum())}"
        worst = _worst(rew.double().cpu().numpy(), orew)
        assert worst <= REW_TOL, f"step {t}: reward off by {worst:.3e}, REW_TOL {REW_TOL:.1e}"
        i = info.double().cpu().numpy()
        worst = _worst(i[:, :3], oinfo[:, :3])
        assert worst <= REW_TOL, f"step {t}: info's reward terms off by {worst:.3e}, REW_TOL {REW_TOL:.1e}"
        worst = _worst(i[:, 3], oinfo[:, 3])
        assert worst <= POS_TOL, f"step {t}: info's distance off by {worst:.3e}, POS_TOL {POS_TOL:.1e}"
        check_obs(to_env_major(env, obs), oobs)
    check_state_exact(env, orc)
    env.close()


# ---- the MLP tests' model ------------------------------------------------------------------------------------------------------------
def mlp_make(B, seed, rows=None, with_filter=False):
    """(model, its HipMLP for batch B, obs [rows, 137], the row gather idx or None, the observation filter or None), seeded"""
    from pioneer_amd.ppo import ActorCritic, PPOConfig
    from pioneer_amd.mlp import HipMLP
    device = torch.device("cuda", 0)
    torch.manual_seed(seed)
    model = ActorCritic(PPOConfig()).to(device)
    with torch.no_grad():                                   # heads of visible size, non-zero biases
        for net in (model.policy, model.value):
            for l in net:
                if isinstance(l, torch.nn.Linear):
                    l.bias.normal_(0, 0.1)
        model.policy[4].weight.mul_(30.0)
    g = torch.Generator(device=device).manual_seed(seed + 1)
    rows = rows or B
    obs = torch.randn(rows, 137, generator=g, device=device) * 2.0 + 0.3
    idx = torch.randperm(rows, generator=g, device=device)[:B].contiguous() if rows != B else None
    filt = None
    if with_filter:
        loc = torch.randn(137, generator=g, device=device) * 0.5
        inv = torch.rand(137, generator=g, device=device) + 0.5
        hi = torch.full((137,), 2.5, device=device)
        filt = (loc, inv, -hi, hi)
    return model, HipMLP(model, B, device), obs, idx, filt


def unpack_flat(flat):
    """The padded gradient bucket [2][107 024] as the twelve parameter-shaped gradients (policy six, value six)."""
    E = flat.numel() // 2
    out = []
    for n in range(2):
        f = flat[n * E:(n + 1) * E]
        n3 = 12 if n == 0 else 1
        out += [f[:256 * 144].view(256, 144)[:, :137], f[102400 + 4096:102400 + 4096 + 256],
                f[36864:36864 + 65536].view(256, 256), f[102400 + 4096 + 256:102400 + 4096 + 512],
                f[102400:102400 + 4096].view(16, 256)[:n3], f[102400 + 4096 + 512:102400 + 4096 + 512 + 16][:n3]]
    return out


# ---- the render and ray tests' scene ---------------------------------------------------------------------------------------------------
def coloured_bodies():
    """[(SceneBody, rgba)]: a rotated box, a sphere, the plane at z = -0.5"""
    from pioneer_amd.config import scene_box, scene_plane, scene_sphere
    return [(scene_box((1.0, 1.5, 3.0), (10.0, 5.0, 0.0), (0.0, 0.0, 0.38268343, 0.92387953)), (0.8, 0.2, 0.6, 1.0)),
            (scene_sphere(2.0, (-8.0, -6.0, 4.0)), (0.2, 0.7, 0.9, 1.0)),
            (scene_plane((0.0, 0.0, 1.0), (0.0, 0.0, -0.5)), (0.4, 0.4, 0.4, 1.0))]


def random_state(n, seed):
    """(q [n, 6] inside the limits, targets [n, 3] in the target box), float32"""
    rng = np.random.default_rng(seed)
    q = (rng.uniform(-1.0, 1.0, size=(n, 6)) * LIMITS).astype(np.float32)
    tgt = rng.uniform((15, -10, 2), (25, 10, 6), size=(n, 3)).astype(np.float32)
    return q, tgt
