"""The inputs of the time-parameterisation tests, shared by the CPU tests (tests/test_retime_cpu.py: the reference's own
properties and the float32 floor the bars come from) and the GPU tests (tests/test_gpu_retime.py: the kernels on exactly these
paths).  Nothing here is a reference: that is tests/retime_ref.py.

Families (every path a float32 array [n, C, 6]; the paths of n envs are the first n of the family's generator):
    CORNER   3 random waypoints at +-0.8 x the joint limits, 8 sub-steps per segment: C = 17, a corner in the middle
    SMOOTH   per-joint sinusoids around a random posture, amplitude <= 0.6 rad, C in SIZES_C: every joint sweeps part of a sine's
             monotone half (an S-curve).  With torque rows it is used at C in TORQUE_SIZES_C: a 4-point path, whose only
             interior points are next to the ends, ends stuck under torque rows in 10 .. 30 of 130 envs (float64; a stop at
             point 2 is a stop next to the rest at point 3), and the float32 verdict differs in a few of them.  Sinusoids that
             reverse (wavy) end stuck in 1 .. 5 % of the paths at C = 17 and 33 for the same reason: a finding about the law
             (DESIGN 3aa), counted by tests/test_retime_cpu.py, not a family the kernels are held to
    HEAVY    the stretched-out arm starts against gravity: tau_max[1] is below |G_1| at grid point HEAVY_POINT = 0 and above it
             everywhere else (unit link scales)
    DUP      a SMOOTH path whose last DUP_ROWS rows repeat (the tail solve_ik_path leaves after a failure)
    NAN      a SMOOTH batch with one NaN in env NAN_ENV's point NAN_POINT
(IKLINE, a q_path that solve_ik_path wrote, is made on the device by the GPU tests.)
Limits: v_max 2, a_max 10 for every joint; tau_max per joint 1.5 x the largest |G_j| over the batch's paths, and at least
TAU_FLOOR_FRACTION of the largest of those (joint 0 turns about the vertical: its G is 0, and a limit must be > 0).
"""
import numpy as np

import ik_ref
import inverse_dynamics_ref as idref

DOF = 6
SIZES_N = (1, 37, 64, 130)
SIZES_C = (3, 4, 17, 33, 256)
TORQUE_SIZES_C = (3, 17, 33, 256)
V_MAX = np.full(DOF, 2.0)
A_MAX = np.full(DOF, 10.0)
GRAVITY = 9.81
TAU_FACTOR, TAU_FLOOR_FRACTION = 1.5, 0.1
CORNER_SUBSTEPS = 8
DUP_ROWS = 4
NAN_ENV, NAN_POINT = 5, 9
HEAVY_POINT = 0


def limits():
    lo, hi = (v.astype(np.float64) for v in ik_ref.limits_f32())
    return lo, hi


def corner(n, seed=101):
    lo, hi = limits()
    wp = np.random.default_rng(seed).uniform(0.8 * lo, 0.8 * hi, size=(n, 3, DOF))
    u = (np.arange(1, CORNER_SUBSTEPS + 1) / CORNER_SUBSTEPS)[None, :, None]
    segs = [wp[:, :1]] + [wp[:, i:i + 1] + u * (wp[:, i + 1:i + 2] - wp[:, i:i + 1]) for i in range(2)]
    return np.concatenate(segs, axis=1).astype(np.float32)


def smooth(n, C, seed=202):
    """q_j(s) = centre_j + amp_j sin(pi f_j (s - 1/2)), s = k / (C - 1): each joint sweeps a part f_j in 0.3 .. 1 of a sine's
    rising (or, amp < 0, falling) half, an S-curve whose curvature changes sign in the middle"""
    lo, hi = limits()
    rng = np.random.default_rng(seed)
    centre = rng.uniform(0.3 * lo, 0.3 * hi, size=(n, 1, DOF))
    amp = rng.uniform(0.1, 0.6, size=(n, 1, DOF)) * rng.choice([-1.0, 1.0], size=(n, 1, DOF))
    f = rng.uniform(0.3, 1.0, size=(n, 1, DOF))
    s = (np.arange(C) / (C - 1))[None, :, None]
    return (centre + amp * np.sin(np.pi * f * (s - 0.5))).astype(np.float32)


def wavy(n, C, seed=202):
    """sinusoids that reverse: 0.25 .. 1 cycles per joint over the path.  NOT a family the kernels are held to a verdict on: it
    is what the CPU tests count the law's interior stops and stuck endings on"""
    lo, hi = limits()
    rng = np.random.default_rng(seed)
    centre = rng.uniform(0.3 * lo, 0.3 * hi, size=(n, 1, DOF))
    amp = rng.uniform(0.1, 0.6, size=(n, 1, DOF))
    cycles = rng.uniform(0.25, 1.0, size=(n, 1, DOF))
    phase = rng.uniform(0.0, 2 * np.pi, size=(n, 1, DOF))
    s = (np.arange(C) / (C - 1))[None, :, None]
    return (centre + amp * np.sin(2 * np.pi * cycles * s + phase)).astype(np.float32)


def heavy(n, C=17, seed=303):
    """joint 1 moves the stretched-out arm (q_1 = 0, where |G_1| is largest on the path) to q_1 = -0.9: with unit link scales
    |G_1| falls from 467 at point 0 to 424 at point 1, and heavy_tau_limits puts tau_max[1] between the two.  At point 0 the
    arm is at rest (x_0 = 0) and has to start against gravity, so no acceleration relieves the joint: K_0 is empty."""
    rng = np.random.default_rng(seed)
    s = (np.arange(C) / (C - 1))[None, :, None]
    P = rng.uniform(-0.02, 0.02, size=(n, 1, DOF)) + s * rng.uniform(-0.05, 0.05, size=(n, 1, DOF))
    P[:, :, 1] = -0.9 * s[..., 0]
    return P.astype(np.float32)


def heavy_tau_limits(P, scales, gravity=GRAVITY):
    """tau_limits, but joint 1's limit halfway between the smallest |G_1| at point 0 and the largest at point 1 of the batch"""
    G = gravity_torques(P, scales, gravity)
    tau = tau_limits(P, scales, gravity)
    assert G[:, 0, 1].min() > G[:, 1, 1].max(), "HEAVY needs link scales alike enough (unit scales)"
    tau[1] = 0.5 * (G[:, 0, 1].min() + G[:, 1, 1].max())
    return tau


def dup(n, C=17, seed=404):
    P = wavy(n, C, seed)
    P[:, C - DUP_ROWS:] = P[:, C - DUP_ROWS:C - DUP_ROWS + 1]
    return P


def with_nan(n, C=17, seed=505):
    P = smooth(n, C, seed)
    if n > NAN_ENV:
        P[NAN_ENV, NAN_POINT, 2] = np.nan
    return P


def scales_drawn(n, seed=606):
    """link scales [n, 11] for the CPU tests' torque rows (the GPU tests read the handle's own)"""
    return np.random.default_rng(seed).uniform(0.5, 1.5, size=(n, 11)).astype(np.float32)


def gravity_torques(P, scales, gravity=GRAVITY):
    """|G| [n, C, 6] in float64 at every point of the paths (a NaN point: NaN)"""
    P = np.asarray(P, dtype=np.float64)
    n, C, _ = P.shape
    flat = P.reshape(n * C, DOF)
    zero = np.zeros_like(flat)
    with np.errstate(all="ignore"):
        G = idref.newton_euler(flat, zero, zero, np.repeat(np.asarray(scales, dtype=np.float64), C, axis=0), gravity)
    return np.abs(G).reshape(n, C, DOF)


def tau_limits(P, scales, gravity=GRAVITY):
    """tau_max [6] for a batch of paths: TAU_FACTOR x the largest |G_j| on them, floored at TAU_FLOOR_FRACTION of the largest"""
    g = np.nanmax(gravity_torques(P, scales, gravity), axis=(0, 1))
    return TAU_FACTOR * np.maximum(g, TAU_FLOOR_FRACTION * g.max())
