"""The inputs of the moving-sphere tests, shared by the CPU tests (which assert on the float64 reference that the inputs are well
conditioned) and the GPU tests (which run the kernel on exactly these inputs), and the sphere's bars, which are taken from the
reference's own float32-storage deviation on these inputs.  The reference itself is tests/world_step_ref.py's world_step(sphere=...)
with the sphere's law of tests/moving_sphere_ref.py.

Every input is a float32 number, held in float64 where the reference reads it, and comes from a generator of its own sized N_MAX,
so the inputs of n envs are the first n rows of those of N_MAX envs.

Families.  PHYS is the kernel instantiation a family runs (bit 0 contacts, bit 1 the inertia-scaled motor):
    A   gravity, the ground plane, pointer-only contacts, the env-wide PD motors on the command state.  The sphere's centre sits
        at the pointer plus a random vector of length uniform in [0.5, 1.5] (radius + pointer_radius)                       PHYS 1
    B   link contacts, a tilted scene plane and an oriented scene box, randomised link masses, friction and damping, the
        inertia-scaled motors.  The sphere is placed the same way relative to a randomly chosen one of the 23 samples         PHYS 3
    C   the arm far away: the sphere lies on the ground near the static obstacle box, beyond the arm's reach, and slides towards
        it with a tangential velocity of up to 5.  A tenth of the envs have mass 0 (no sphere)                                 PHYS 1
Masses are uniform in [0.5, 4] (the explicit spring is stable above 0.21), radii in [0.3, 1.5].  Each family runs with the three
call forms of FORMS: the plain call, joint torques, targets on four joints with torques.
"""
import functools

import numpy as np

import bars
import ik_ref
import link_kinematics_ref as lk
import moving_sphere_ref as ref
import oracle_cases as ocases
import world_step_ref as wref
from oracle import DynOracle

DOF = 6
N_MAX = 1000
SIZES = (97, 1000)                    # one full wave plus a ragged one of 33; 16 waves, the last one partial
STEPS = 3
H = 1.0 / 240
FRAME_SKIP = 10
POINTER_RADIUS = 0.2
Q_TOL, QD_TOL, PTR_TOL = bars.Q_TOL, bars.QD_TOL, bars.PTR_TOL

TRACK = [None] * DOF                  # the env-wide law on the env's command state
FORMS = ("plain", "torques", "targets")
TARGET_JOINTS = (0, 2, 3, 5)
TORQUE_SCALE = np.array([20.0, 20.0, 20.0, 5.0, 5.0, 2.0])
BOX_C, BOX_H = (45.0, 0.0, 1.0), (1.0, 2.0, 1.0)                     # family C's obstacle: beyond the 30-unit arm's reach

_SCENE_B = [("plane", (0.0, 0.0, -0.5), (0.0, 0.0, 0.0, 1.0), (0.0, 0.1, 1.0)),
            ("box", (10.0, 5.0, 0.0), (0.0, 0.0, 0.38268343, 0.92387953), (1.0, 1.5, 3.0))]
# `dyn`: the oracle's names (tests/gpu_support.engine_config_from_oracle_names makes the EngineConfig of them); gravity apart
FAMILIES = {
    "A": dict(seed=71, gravity=9.81, dyn=dict(ground_z=0.0), near=0.05, qd=0.5),
    "B": dict(seed=72, gravity=0.0, dyn=dict(link_contacts=1, randomize=1, pd_inertia_scaled=1, kp=400.0, kd=40.0, torque_limit=2e4, scene=_SCENE_B),
              near=0.05, qd=0.5),
    "C": dict(seed=73, gravity=9.81, dyn=dict(ground_z=0.0, obstacle_position=BOX_C, obstacle_half_extents=BOX_H), near=0.05, qd=0.5),
}
PHYS = {"A": 1, "B": 3, "C": 1}


def followed(n):
    """The envs the reference follows: all of a small batch; of 1000, every 8th and the whole partial last wave."""
    return np.arange(n) if n <= 97 else np.array([e for e in range(n) if e % 8 == 0 or e >= (n // 64) * 64])


def make_oracle(family, n, reset=True):
    f = FAMILIES[family]
    return ocases.make_oracle(f["seed"], n, FRAME_SKIP, f["gravity"], f["dyn"], reset=reset)


def states(family, r_cmd):
    """q, qd [n, 6] float32 for the command positions r_cmd [n, 6] (the first n envs): near the command state, so that the PD
    law's pull stays moderate"""
    f = FAMILIES[family]
    n = r_cmd.shape[0]
    lo, hi = (v.astype(np.float64) for v in ik_ref.limits_f32())
    rng = np.random.default_rng(f["seed"] + 100)
    q = np.clip(r_cmd.astype(np.float64) + rng.uniform(-f["near"], f["near"], size=(N_MAX, DOF))[:n], 0.98 * lo, 0.98 * hi)
    qd = np.random.default_rng(f["seed"] + 101).uniform(-f["qd"], f["qd"], size=(N_MAX, DOF))[:n]
    return q.astype(np.float32), qd.astype(np.float32)


@functools.lru_cache(maxsize=None)
def sample_table(link_contacts):
    """[(body, c, radius)] of the arm's contact samples as the oracle lists them: the pointer's alone, or all 23"""
    tab = DynOracle(1, dyn=dict(link_contacts=int(link_contacts))).contact_samples()
    return [(b, c, r if r >= 0 else POINTER_RADIUS) for b, c, r in tab]            # (the oracle's table marks the pointer's radius with -1)


def sample_positions(q, link_contacts):
    """(positions [n, S, 3], radii [S]) of the samples at q [n, 6]"""
    import external_force_ref as ext
    R, o, _, _ = lk.link_frames(np.asarray(q, dtype=np.float64))
    links = ext.body_links()
    tab = sample_table(bool(link_contacts))
    pos = np.stack([o[:, links[b]] + np.einsum("nij,j->ni", R[:, links[b]], c) for b, c, _ in tab], axis=1)
    return pos, np.array([r for _, _, r in tab])


def spheres(family, q):
    """The spheres' words [8, n] float32 for the arms at q [n, 6]"""
    f = FAMILIES[family]
    n = q.shape[0]
    rng = np.random.default_rng(f["seed"] + 200)
    mass = rng.uniform(0.5, 4.0, size=N_MAX)[:n]
    radius = rng.uniform(0.3, 1.5, size=N_MAX)[:n]
    direction = rng.normal(size=(N_MAX, 3))[:n]
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    gap = rng.uniform(0.5, 1.5, size=N_MAX)[:n]
    pick = rng.integers(0, 23, size=N_MAX)[:n]
    vel = rng.uniform(-1.0, 1.0, size=(N_MAX, 3))[:n]
    speed = rng.uniform(0.0, 5.0, size=N_MAX)[:n]
    side = rng.uniform(-1.5, 1.5, size=N_MAX)[:n]
    off = rng.uniform(-0.1, 0.5, size=N_MAX)[:n]
    gone = rng.uniform(size=N_MAX)[:n] < 0.1
    if family == "C":
        # on the ground (a little into it), west of the box, sliding east towards it; a tenth of the envs without a sphere
        x = np.stack([BOX_C[0] - BOX_H[0] - radius - off, BOX_C[1] + side, 0.999 * radius], axis=1)
        vel = np.stack([speed, 0.2 * vel[:, 1], np.zeros(n)], axis=1)
        mass = np.where(gone, 0.0, mass)
    else:
        pos, rad = sample_positions(q, f["dyn"].get("link_contacts", 0))
        k = pick if len(rad) > 1 else np.zeros(n, dtype=int)
        x = pos[np.arange(n), k] + (gap * (radius + rad[k]))[:, None] * direction
    return np.concatenate([x.T, vel.T, mass[None], radius[None]], axis=0).astype(np.float32)


def joint_torques(family, n):
    tau = np.random.default_rng(FAMILIES[family]["seed"] + 103).uniform(-1.0, 1.0, size=(N_MAX, DOF)) * TORQUE_SCALE
    return tau[:n].astype(np.float32)


def targets(family, r_cmd):
    """[n, 12] float32: positions near the command state and small velocities on TARGET_JOINTS; NaN elsewhere (never read)"""
    n = r_cmd.shape[0]
    rng = np.random.default_rng(FAMILIES[family]["seed"] + 104)
    t = np.full((n, 12), np.nan)
    dp, dv = rng.uniform(-0.05, 0.05, size=(N_MAX, DOF))[:n], rng.uniform(-0.2, 0.2, size=(N_MAX, DOF))[:n]
    for j in TARGET_JOINTS:
        t[:, j] = r_cmd[:, j] + dp[:, j]
        t[:, 6 + j] = dv[:, j]
    return t.astype(np.float32)


def form_inputs(form, tau, tg):
    """(tau_ext, targets, joints) of a call form for the reference's world_step"""
    return (None if form == "plain" else tau.astype(np.float64), tg.astype(np.float64) if form == "targets" else None,
            TARGET_JOINTS if form == "targets" else ())


def scenario(family, orc, idx):
    """The family's inputs for the envs idx of a batch of max(idx) + 1, loaded into the oracle (whose command state must be in
    place): (sphere state dict, tau [len(idx), 6], targets [len(idx), 12])"""
    n = int(idx.max()) + 1
    r_all = np.zeros((n, DOF))
    r_all[idx] = orc.state["r"]
    q, qd = states(family, r_all)
    ocases.load_states(orc, q[idx], qd[idx])
    w = spheres(family, q)
    return ref.from_words(w[:, idx]), joint_torques(family, n)[idx], targets(family, r_all.astype(np.float32))[idx]


@functools.lru_cache(maxsize=None)
def reference_margins(family):
    """The reference's own float32-storage deviation on this family's inputs at n = 97, per world step from a common start, worst
    over the three call forms and STEPS steps: dict(x, v: the sphere's position and velocity; q, qd: the joints).  The sphere's
    bars are 4 x these (sphere_bars): the ratio tests/test_external_force_cpu.py and this family's CPU test hold the joint bars to."""
    n = SIZES[0]
    idx = followed(n)
    worst = dict(x=0.0, v=0.0, q=0.0, qd=0.0)
    for form in FORMS:
        a, b = make_oracle(family, n), make_oracle(family, n)
        s, tau, tg = scenario(family, a, idx)
        te, tt, joints = form_inputs(form, tau, tg)
        for _ in range(STEPS):
            b.dstate[:] = a.dstate
            sb = {k: v.copy() for k, v in s.items()}
            wref.world_step(a, TRACK, sphere=s, tau_ext=te, targets=tt, joints=joints, storage32=True)
            wref.world_step(b, TRACK, sphere=sb, tau_ext=te, targets=tt, joints=joints, storage32=False)
            live = s["m"] > 0
            worst["x"] = max(worst["x"], float(np.abs(s["x"] - sb["x"])[live].max()))
            worst["v"] = max(worst["v"], float(np.abs(s["v"] - sb["v"])[live].max()))
            worst["q"] = max(worst["q"], float(np.abs(a.dstate["q"] - b.dstate["q"]).max()))
            worst["qd"] = max(worst["qd"], float(np.abs(a.dstate["qd"] - b.dstate["qd"]).max()))
    return worst


def sphere_bars(family):
    """(position bar, velocity bar): 4 x the reference's float32-storage deviation, the position bar capped at PTR_TOL (the sphere
    moves under the pointer's force)"""
    m = reference_margins(family)
    return min(4.0 * m["x"], PTR_TOL), 4.0 * m["v"]
