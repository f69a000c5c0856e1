"""The input sets of the per-env motor-target tests (pnr_world_step_targets), shared by the CPU tests (which assert on the float64
oracle that the inputs bite) and the GPU tests (which run the kernel on exactly these inputs), and the per-env form of the two
references the project already has.  Nothing here restates a law: the PD reference is orc_dyn_world_step, called env by env with
that env's own OrcJointMotor table (the oracle is per env already); the constraint reference is tests/world_step_ref.py, which
takes one motor list for all envs and is therefore run once per TARGET SET, each env being compared with the run of its own set.

A motor law is a dict in the form of tests/world_step_ref.py (kind "pd" / "position_constraint" / "velocity_constraint") or
None (nobody commanded the joint: the handle's own law).  Its target_position / target_velocity are what pnr_set_joint_motor puts
into the table; a masked joint's are replaced, per env, by that env's row of `targets` [n, 12] = position[6] | velocity[6].
"""
import numpy as np

import bars
import oracle_cases as ocases
from oracle import DynOracle

DOF = 6
Q_TOL, QD_TOL = bars.Q_TOL, bars.QD_TOL                               # read through this module by tests/test_motor_targets_cpu.py
FULL = tuple(range(DOF))


def pd(control_mode, **kw):
    """a PD motor of the table; arguments left out take the handle's configured values (pnr_set_joint_motor's NaN)"""
    return dict(dict(kind="pd", control_mode=control_mode, target_position=0.0, target_velocity=0.0), **kw)


def vel(v, f):
    return dict(kind="velocity_constraint", target_velocity=v, max_force=f)


# ---- the PD input set -------------------------------------------------------------------------------------------------------------
# gravity, randomised links, a torque cap the far targets saturate; the position law on the even joints, the velocity law on the
# odd ones, all six commanded through pnr_set_joint_motor with table targets of 0 (which no env's own targets equal)
PD = dict(n=37, seed=5, frame_skip=10, gravity=9.81, frac=0.6, qd=0.5, steps=3,
          engine=dict(pd_kp=4000.0, pd_kd=400.0, torque_limit=2000.0, joint_damping=0.2, joint_friction=0.1, randomize=True),
          laws=[pd(j % 2) for j in range(DOF)])
# the inertia-scaled law takes the gains the project's other tests give it (an acceleration request, not a torque)
PD_SCALED_ENGINE = dict(PD["engine"], pd_kp=400.0, pd_kd=40.0, pd_inertia_scaled=True)
BOX = dict(obstacle_position=(10.0, 5.0, 0.0), obstacle_half_extents=(0.5, 0.5, 5.0))
PD_CONTACT_ENGINE = dict(PD["engine"], ground_z=0.0, link_contacts=True, **BOX)

# ---- a partial mask next to everything else ------------------------------------------------------------------------------------
# masked: joint 0 (commanded, position law), joint 3 (NOBODY commanded it: the handle's law, the env's targets standing in for its
# command state) and joint 4 (commanded, velocity law).  Unmasked: joint 1 commanded uniformly, joints 2 and 5 uncommanded on a
# command state that `command_steps` vector steps moved off its reset values.
PARTIAL = dict(n=37, seed=6, frame_skip=10, gravity=9.81, frac=0.6, qd=0.5, steps=2, command_steps=3, mask=(0, 3, 4),
               engine=PD["engine"],
               laws=[pd(0), pd(0, target_position=-0.2, target_velocity=0.1, position_gain=9000.0, velocity_gain=700.0),
                     None, None, pd(1, velocity_gain=300.0), None])

# ---- constraint motors, in the spirit of tests/constraint_motor_cases.py's "subset" ---------------------------------------------
# S = {0, 2, 3, 5}: position motors with gains of their own and a maxVelocity on joints 0 and 3, velocity motors on 2 and 5 (the
# latter's force saturates), a PD joint (1) and an uncommanded joint (4).  No contacts (that file's comment: every env may then be
# compared).
CMOTOR = dict(seed=12, frame_skip=1, gravity=9.81, frac=0.8, qd=1.5, command_steps=3, K=3, engine=dict(randomize=True),
              laws=[dict(kind="position_constraint", target_position=0.3, target_velocity=0.2, position_gain=0.004, velocity_gain=0.5,
                         max_force=2e4, max_velocity=0.75),
                    dict(kind="pd", control_mode=0, target_position=-0.2, target_velocity=0.1, position_gain=9000.0, velocity_gain=700.0,
                         max_force=2.5e4, max_velocity=0.0),
                    vel(0.6, 2e4),
                    dict(kind="position_constraint", target_position=-0.5, position_gain=0.003, velocity_gain=0.8, max_force=300.0,
                         max_velocity=1.0),
                    None,
                    vel(1.2, 300.0)])
# (n, mask, steps): the full mask, and one that leaves the saturating velocity motor of joint 5 on the table's own target
CMOTOR_SETS = [(37, FULL, 2), (64, (0, 1, 2, 3, 4), 2), (1000, FULL, 1)]


_LIMITS = []


def limits():
    if not _LIMITS:
        orc = DynOracle(1)
        _LIMITS.append((orc.r_lo.astype(np.float64), orc.r_hi.astype(np.float64)))
    return _LIMITS[0]


def states(case, n, step):
    """(q, qd) [n, 6] float32 of re-randomised step `step`: q uniform within frac x the limits, qd uniform in +-qd"""
    rng = np.random.default_rng([case["seed"], n, step, 0])
    lo, hi = limits()
    return (rng.uniform(case["frac"] * lo, case["frac"] * hi, size=(n, DOF)).astype(np.float32),
            rng.uniform(-case["qd"], case["qd"], size=(n, DOF)).astype(np.float32))


def targets(case, n, step, mask=FULL, poison=False):
    """[n, 12] float32, fresh for every step: position targets uniform within frac x the limits, velocity targets uniform in
    +-0.5; every env's row its own.  poison: the entries of the joints outside `mask` are NaN."""
    rng = np.random.default_rng([case["seed"], n, step, 1])
    lo, hi = limits()
    t = np.concatenate([rng.uniform(case["frac"] * lo, case["frac"] * hi, size=(n, DOF)), rng.uniform(-0.5, 0.5, size=(n, DOF))], axis=1)
    t = t.astype(np.float32)
    if poison:
        for j in range(DOF):
            if j not in mask:
                t[:, j] = t[:, DOF + j] = np.nan
    return t


def target_sets(case, n, step, mask=FULL):
    """K target rows [K, 12] and the set each env takes [n], drawn at random (e mod K would alias with lane patterns); the
    targets tensor is sets[pick]"""
    rng = np.random.default_rng([case["seed"], n, step, 2])
    lo, hi = limits()
    K = case.get("K", 3)
    # per entry the K sets take one value each from K strata of the range (in an order of the entry's own), so that two sets
    # differ in every entry by 4/9 of the half range at least (K = 3): positions within 0.5 x the limits, velocities within +-1.5
    half = np.concatenate([0.5 * hi, np.full(DOF, 1.5)])
    centre = (2.0 * np.arange(K) + 1.0) / K - 1.0                    # of stratum k, in units of the half range
    u = np.stack([centre[rng.permutation(K)] for _ in range(2 * DOF)], axis=1) + rng.uniform(-1.0 / (3 * K), 1.0 / (3 * K), size=(K, 2 * DOF))
    sets = (u * half).astype(np.float32)
    pick = rng.integers(0, K, size=n)
    if n >= K:
        pick[rng.permutation(n)[:K]] = np.arange(K)                  # every set is somebody's
    return sets, pick


def make_oracle(case, n, engine=None):
    return ocases.make_oracle(case["seed"], n, case["frame_skip"], case["gravity"], case["engine"] if engine is None else engine,
                              case.get("command_steps", 0))


def law_for_env(law, tgt, j):
    """law (not None) with env's own targets tgt [12] for joint j"""
    return dict(law, target_position=float(tgt[j]), target_velocity=float(tgt[DOF + j]))


def oracle_world_step(orc, laws, tgt=None, mask=()):
    """One pnr_world_step of every env of the oracle's batch by orc_dyn_world_step, env by env, in place on orc.dstate.  The table
    is `laws` (PD laws and None only); with tgt [n, 12], env e's table holds tgt[e]'s entries as the targets of the joints in
    `mask`.  A masked joint nobody commanded keeps the handle's own law: its targets stand in for the env's command state r, v,
    which is put back afterwards."""
    import ctypes as C
    for j, m in enumerate(laws):
        if m is not None:
            assert m["kind"] == "pd"
            orc.set_joint_motor(j, m["control_mode"], m["target_position"], m["target_velocity"], m.get("position_gain"),
                                m.get("velocity_gain"), m.get("max_force"), m.get("max_velocity"))
    motors = getattr(orc, "motors", None)
    for e in range(orc.n):
        row = orc.state[e:e + 1].copy()
        if tgt is not None:
            for j in mask:
                if laws[j] is None:
                    row["r"][0, j], row["v"][0, j] = tgt[e, j], tgt[e, DOF + j]
                else:
                    motors[j].target_position, motors[j].target_velocity = float(tgt[e, j]), float(tgt[e, DOF + j])
        orc.lib.orc_dyn_world_step(C.byref(orc.d), C.byref(orc.p), C.c_void_p(row.ctypes.data), orc._one(e), motors)
    for j, m in enumerate(laws):                                      # the table's own targets again
        if m is not None:
            motors[j].target_position, motors[j].target_velocity = float(m["target_position"]), float(m["target_velocity"])


def constraint_reference_step(orc, laws, sets, pick, mask, frame_skip):
    """One world step of every env under the constraint-motor reference, env e with the targets sets[pick[e]] on the joints of
    `mask`: the reference runs once per set with that set's motors for everybody, and each env keeps the run of its own set.
    In place on orc.dstate; returns the last sub-step's info dicts, one per set."""
    import world_step_ref as wref
    start = orc.dstate.copy()
    out = start.copy()
    infos = []
    uncommanded = [j for j in mask if laws[j] is None]                # the handle's law: the targets stand in for r, v
    for k in range(len(sets)):
        orc.dstate[:] = start
        motors = [law_for_env(m, sets[k], j) if (j in mask and m is not None) else m for j, m in enumerate(laws)]
        infos.append(wref.world_step(orc, motors, targets=np.broadcast_to(sets[k], (orc.n, 2 * DOF)), joints=uncommanded,
                                     frame_skip=frame_skip)[-1])
        mine = pick == k
        out[mine] = orc.dstate[mine]
    orc.dstate[:] = out
    return infos
