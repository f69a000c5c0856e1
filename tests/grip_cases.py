"""The inputs of the grip's tests, shared by the CPU tests (which assert on the float64 reference that the inputs are well
conditioned) and the GPU tests (which run the kernel on exactly these inputs), and the grip's bars, which are taken from the
reference's own float32-storage deviation on these inputs.  The reference is tests/grip_ref.py's world_step.

Every input is a float32 number, held in float64 where the reference reads it, and comes from a generator of its own sized N_MAX,
so the inputs of n envs are the first n rows of those of N_MAX envs.  The arms, their motors, their static worlds, the joint
torques, the per-env targets and the sizes are tests/moving_sphere_cases.py's families A and B (`base`).

Families.  PHYS is the kernel instantiation a family runs (bit 0 contacts, bit 1 the inertia-scaled motor):
    G1  on family A (gravity 9.81, the ground, pointer-only contacts), the grip's default params.  The sphere starts within 0.3 of
        its anchor point with a velocity relative to it of up to 1; max_force 1e4 is never reached                          PHYS 1
    G2  on family B (link contacts, randomised link scales, the inertia-scaled motors, the scene's bodies); a non-zero anchor, a
        zero direction, grip_kp 2000.  The sphere sits at a distance uniform in [0, 0.5] from its anchor; max_force 300 caps the
        spring of about 0.7 of the gripped envs, which is about half of all envs                                               PHYS 3
In both a fifth of the envs are released and have their spheres where the base family places them (they touch the arm), and a
tenth have mass 0.  Each family runs with the three call forms of FORMS.

HOLD and CARRY are the two scenarios at n = 64 whose bounds come from the reference's run: hold_steps() and carry_reference().
"""
import functools

import numpy as np

import bars
import grip_ref as gref
import moving_sphere_cases as msc
import moving_sphere_ref as sref
import oracle_cases as ocases

DOF = 6
N_MAX, SIZES, STEPS, H, FRAME_SKIP = msc.N_MAX, msc.SIZES, msc.STEPS, msc.H, msc.FRAME_SKIP
POINTER_RADIUS = msc.POINTER_RADIUS
Q_TOL, QD_TOL, PTR_TOL = bars.Q_TOL, bars.QD_TOL, bars.PTR_TOL
TRACK, FORMS, TARGET_JOINTS = msc.TRACK, msc.FORMS, msc.TARGET_JOINTS
followed, form_inputs = msc.followed, msc.form_inputs

FAMILIES = {
    "G1": dict(base="A", seed=91, reach=0.3, max_force=1e4, grip=None),
    "G2": dict(base="B", seed=92, reach=0.5, max_force=300.0, grip=dict(anchor=(0.3, -0.2, 0.4), direction=(0.0, 0.0, 0.0), grip_kp=2000.0)),
}
PHYS = {"G1": 1, "G2": 3}


def base_family(family):
    """moving_sphere_cases' family (its FAMILIES entry: seed, gravity, the oracle's `dyn` names) that `family` is built on"""
    return msc.FAMILIES[FAMILIES[family]["base"]]


def make_oracle(family, n, reset=True):
    return msc.make_oracle(FAMILIES[family]["base"], n, reset=reset)


def spheres(family, q, qd):
    """(the spheres' words [8, n] float32, max_force [n] float32) for the arms at q, qd [n, 6]"""
    f = FAMILIES[family]
    n = q.shape[0]
    w = msc.spheres(f["base"], q).astype(np.float64)                   # mass, radius; position and velocity of the released envs
    rng = np.random.default_rng(f["seed"] + 300)
    direction = rng.normal(size=(N_MAX, 3))[:n]
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    dist = rng.uniform(0.0, f["reach"], size=N_MAX)[:n]
    vdir = rng.normal(size=(N_MAX, 3))[:n]
    vdir /= np.linalg.norm(vdir, axis=1, keepdims=True)
    speed = rng.uniform(0.0, 1.0, size=N_MAX)[:n]
    released = rng.uniform(size=N_MAX)[:n] < 0.2
    gone = rng.uniform(size=N_MAX)[:n] < 0.1
    _, pa, va, _ = gref.anchor_kinematics(q, qd, w[7], POINTER_RADIUS, gref.geometry_of(f["grip"]))
    x = np.where(released[:, None], w[0:3].T, pa + dist[:, None] * direction)
    v = np.where(released[:, None], w[3:6].T, va + speed[:, None] * vdir)
    mass = np.where(gone, 0.0, w[6])
    words = np.concatenate([x.T, v.T, mass[None], w[7][None]], axis=0).astype(np.float32)
    return words, np.where(released, 0.0, f["max_force"]).astype(np.float32)


def scenario(family, orc, idx):
    """The family's inputs for the envs idx of a batch of max(idx) + 1, loaded into the oracle (whose command state must be in
    place): (sphere state dict, max_force [len(idx)], tau [len(idx), 6], targets [len(idx), 12])"""
    base = FAMILIES[family]["base"]
    n = int(idx.max()) + 1
    r_all = np.zeros((n, DOF))
    r_all[idx] = orc.state["r"]
    q, qd = msc.states(base, r_all)
    ocases.load_states(orc, q[idx], qd[idx])
    w, fmax = spheres(family, q, qd)
    return (sref.from_words(w[:, idx]), fmax[idx].astype(np.float64), msc.joint_torques(base, n)[idx],
            msc.targets(base, r_all.astype(np.float32))[idx])


@functools.lru_cache(maxsize=None)
def reference_margins(family):
    """The reference's own float32-storage deviation on this family's inputs at n = 97, per world step from a common start, worst
    over the three call forms and STEPS steps: dict(x, v: the sphere's position and velocity; f: the reported force; q, qd: the
    joints), and `capped`: the share of all envs whose spring exceeds its cap in the first sub-step of the first step."""
    n = SIZES[0]
    idx = followed(n)
    worst = dict(x=0.0, v=0.0, f=0.0, q=0.0, qd=0.0, capped=None)
    for form in FORMS:
        a, b = make_oracle(family, n), make_oracle(family, n)
        s, fmax, tau, tg = scenario(family, a, idx)
        te, tt, joints = form_inputs(form, tau, tg)
        kw = dict(max_force=fmax, grip_params=FAMILIES[family]["grip"], tau_ext=te, targets=tt, joints=joints)
        for step in range(STEPS):
            b.dstate[:] = a.dstate
            sb = {k: v.copy() for k, v in s.items()}
            ra = gref.world_step(a, TRACK, sphere=s, storage32=True, **kw)
            rb = gref.world_step(b, TRACK, sphere=sb, storage32=False, **kw)
            live, on = s["m"] > 0, gref.held(s, fmax)
            if step == 0 and worst["capped"] is None:
                first = rb["records"][0]
                worst["capped"] = float((first["held"] & (np.linalg.norm(first["grip_raw"], axis=1) > fmax)).mean())
            worst["x"] = max(worst["x"], float(np.abs(s["x"] - sb["x"])[live].max()))
            worst["v"] = max(worst["v"], float(np.abs(s["v"] - sb["v"])[live].max()))
            worst["f"] = max(worst["f"], float(np.abs(ra["force"] - rb["force"])[on].max()))
            worst["q"] = max(worst["q"], float(np.abs(a.dstate["q"] - b.dstate["q"]).max()))
            worst["qd"] = max(worst["qd"], float(np.abs(a.dstate["qd"] - b.dstate["qd"]).max()))
    return worst


def grip_bars(family):
    """(position bar, velocity bar, force bar): 4 x the reference's float32-storage deviation (as moving_sphere_cases.sphere_bars), the
    position bar capped at PTR_TOL"""
    m = reference_margins(family)
    return min(4.0 * m["x"], PTR_TOL), 4.0 * m["v"], 4.0 * m["f"]


# ---- hold at rest and carry: n = 64, gravity, no static world.  The inertia-scaled motors of family B hold the arm against gravity
# (under the plain PD law's default gains the arm itself swings by 0.6 rad for seconds: nothing to hold a sphere at rest on) -----------
HOLD = dict(seed=93, n=64, gravity=9.81, dyn=dict(pd_inertia_scaled=1, kp=400.0, kd=40.0, torque_limit=2e4), mass=2.0, radius=0.5, max_force=1e4)
CARRY = dict(HOLD, seed=94, steps=20, turn=0.3)
GRIP_KP, G = 2000.0, 9.81                                             # the defaults' grip_kp (the sphere's contact_kp); HOLD's gravity


def hold_bound(mass=HOLD["mass"]):
    """|x - p_a| of a sphere held at rest: the static sag m g / grip_kp, plus half of it for the arm's residual motion"""
    return 1.5 * mass * G / GRIP_KP


def held_oracle(case):
    """(oracle, sphere, max_force) of HOLD or CARRY: the arm at its command state at rest, the sphere at its anchor point at rest"""
    orc = ocases.make_oracle(case["seed"], case["n"], FRAME_SKIP, case["gravity"], case["dyn"])
    n = orc.n
    ocases.load_states(orc, orc.state["r"].astype(np.float32), np.zeros((n, DOF)))
    radius = np.full(n, case["radius"])
    _, pa, _, _ = gref.anchor_kinematics(orc.dstate["q"], orc.dstate["qd"], radius, POINTER_RADIUS, gref.geometry_of())
    s = sref.sphere(pa.astype(np.float32), np.zeros((n, 3)), np.full(n, case["mass"]), radius)
    return orc, s, np.full(n, case["max_force"])


def anchor_error(orc, s):
    """|x - p_a| [n] at the oracle's joints"""
    _, pa, _, _ = gref.anchor_kinematics(orc.dstate["q"], orc.dstate["qd"], s["r"], POINTER_RADIUS, gref.geometry_of())
    return np.linalg.norm(s["x"] - pa, axis=1)


@functools.lru_cache(maxsize=None)
def hold_steps(limit=200):
    """K: the smallest multiple of 10 world steps after which every env of HOLD satisfies hold_bound() on the reference (the bound
    is fixed; K is what is chosen), and the error there"""
    orc, s, fmax = held_oracle(HOLD)
    for k in range(1, limit + 1):
        gref.world_step(orc, TRACK, sphere=s, max_force=fmax)
        if k % 10 == 0:
            err = float(anchor_error(orc, s).max())
            if err <= hold_bound():
                return k, err
    raise AssertionError(f"the reference does not reach the hold bound within {limit} world steps")


def carry_targets(r_cmd, step):
    """[n, 12] float32: world step `step`'s targets (0 .. steps - 1) on the way from the command positions r_cmd [n, 6] to a pose
    CARRY['turn'] rad away per joint (towards the middle of the joint's range), target velocity 0"""
    n = r_cmd.shape[0]
    away = -np.sign(np.where(r_cmd == 0, 1.0, r_cmd)) * CARRY["turn"]
    t = np.zeros((n, 12))
    t[:, 0:6] = r_cmd + away * (step + 1) / CARRY["steps"]
    return t.astype(np.float32)


@functools.lru_cache(maxsize=None)
def carry_reference():
    """The worst |x - p_a| over CARRY's trajectory (after each of its world steps, over the envs) on the reference"""
    orc, s, fmax = held_oracle(CARRY)
    r = orc.state["r"].astype(np.float32)
    worst = 0.0
    for step in range(CARRY["steps"]):
        tg = carry_targets(r, step).astype(np.float64)
        gref.world_step(orc, TRACK, sphere=s, max_force=fmax, targets=tg, joints=tuple(range(DOF)))
        worst = max(worst, float(anchor_error(orc, s).max()))
    return worst
