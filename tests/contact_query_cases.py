"""The inputs of the contact-query tests, shared by the CPU tests (which measure on them what float32 arithmetic alone costs and
assert the conditions the comparisons rest on) and the GPU tests (which run the kernel on exactly these inputs).  Nothing here
is a reference: that is tests/contact_query_ref.py.

Inputs: q uniform in +-0.9 x the URDF limits, qd in +-3, each from a generator of its own, so the inputs of n envs are the first
n rows of the inputs of N_MAX envs and what is measured at N_MAX covers every smaller batch.  All values are float32 numbers.

Family A: three bodies shared by all envs (SCENE_A).  Measured in float64 on the N_MAX envs (test_contact_query_cpu.py prints
them): 5.7 % of the (env, sample) pairs penetrate, 22 % of the envs have a contact, the nearest body is plane / box / sphere for
59 / 32 / 9 % of the pairs.
Family B: the same plane and box, and a sphere per env (body_positions): its centre is one of the env's own sample centres
(chosen by the seed) plus an offset of length U(0.5, 1.5) x (sphere radius + sample radius) in a random direction, so about
half the envs penetrate that body with the chosen sample (measured: 74 % with any sample; 18 % of the pairs penetrate).

THE FLOAT32 FLOOR.  contact_query_ref.query runs the same arithmetic in float32 and in float64 on the same float32 inputs; the
largest difference over the batch (outside the exclusions) is what float32 alone costs.  The *_FLOOR constants are those
maxima over both families (numpy 2.x, x86-64; N_MAX envs), rounded up to two digits (measured, A | B: distance 3.95e-6 | 4.13e-6,
normal 2.75e-6 | 2.34e-6, position 3.77e-6 | 3.80e-6, velocity 1.78e-5, force 4.49e-3 | 6.95e-3, torque 0.278 | 0.412 where the
torques reach 1e5);
test_contact_query_cpu.py::test_float32_floors_hold_and_sit_inside_the_hard_bars asserts floor <= constant <= 2 floor.  The
kernel is allowed FLOOR_MARGIN = 8 times these (as tests/inverse_dynamics_cases.py: another order of operations, fused
multiply-adds, sincos_any against libm) and, whatever the floor, never more than the hard bars.
"""
import numpy as np

import contact_query_ref as ref
import link_kinematics_ref as lk

SEED = 20261017
N_MAX = 1000
SIZES = (1, 37, 64, 1000)
KP, KD, POINTER_RADIUS = 2000.0, 50.0, 0.2
FLOOR_MARGIN = 8.0
SPHERE_RADIUS = 3.0

SCENE_A = (
    ref.plane((0.0, 0.0, 1.0), (0.0, 0.0, 0.0)),
    ref.box((2.0, 1.5, 4.0), (12.0, 4.0, 4.0), (0.0, 0.0, float(np.sin(0.25)), float(np.cos(0.25)))),
    ref.sphere(SPHERE_RADIUS, (14.0, -6.0, 5.0)),
)
SPHERE_BODY = 2

# measured float32 floors (module docstring): largest |float32 - float64| over both families, outside the exclusions
DIST_FLOOR = 4.2e-06        # points[..., 0] and summary[..., 0]
NORMAL_FLOOR = 2.8e-06      # points[..., 1:4]
POS_FLOOR = 3.8e-06         # points[..., 4:7]
VEL_FLOOR = 1.8e-05         # the sample centres' world velocity (enters the force through kd)
FORCE_FLOOR = 7.0e-03       # points[..., 8]
TORQUE_FLOOR = 4.2e-01      # joint_torques
LEVER_MAX = 28.4            # the longest |x_s - o_j| the samples have (measured 28.379: joint 1's axis to the pointer)

# hard bars, from the project's own: distances and positions 1e-4 (the FK is at 3e-5), normals 1e-4,
# forces kp 1e-4 + kd (float32 velocity floor), torques the force bar x the longest lever
DIST_HARD = 1e-4
NORMAL_HARD = 1e-4
FORCE_HARD = KP * 1e-4 + KD * VEL_FLOOR
TORQUE_HARD = FORCE_HARD * LEVER_MAX


def limits():
    ch = [j for j in lk.load_chain() if j["type"] == "revolute"]
    return np.array([j["lower"] for j in ch]), np.array([j["upper"] for j in ch])


def joints(n, frac=0.9, qd_max=3.0, seed=SEED):
    """q, qd [n, 6] float32"""
    lo, hi = limits()
    q = np.random.default_rng(seed).uniform(frac * lo, frac * hi, size=(N_MAX, 6))[:n]
    qd = np.random.default_rng(seed + 1).uniform(-qd_max, qd_max, size=(N_MAX, 6))[:n]
    return q.astype(np.float32), qd.astype(np.float32)


def joint_state(n):
    q, qd = joints(n)
    return np.concatenate([q, qd], axis=1)


def family_b_positions(n, seed=SEED + 2):
    """body_positions [n, 3, 3] float32: the plane's and the box's own positions, the sphere near one of the env's samples"""
    q, qd = joints(N_MAX)
    centres = ref.query(q, qd, ())["centres"]
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, ref.SAMPLES, size=N_MAX)
    radii = np.array([POINTER_RADIUS if r < 0 else r for _, _, r in ref.sample_table()])
    d = rng.normal(size=(N_MAX, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    length = rng.uniform(0.5, 1.5, size=N_MAX) * (SPHERE_RADIUS + radii[pick])
    bp = np.zeros((N_MAX, 3, 3))
    for b in range(3):
        bp[:, b] = SCENE_A[b]["position"]
    bp[:, SPHERE_BODY] = centres[np.arange(N_MAX), pick] + length[:, None] * d
    return bp[:n].astype(np.float32)


_CACHE = {}


def reference(family, dtype=np.float64):
    """The reference's outputs on the N_MAX envs of family "A" / "B" (computed once, shared, left unchanged)"""
    key = (family, np.dtype(dtype).name)
    if key not in _CACHE:
        q, qd = joints(N_MAX)
        bp = family_b_positions(N_MAX) if family == "B" else None
        _CACHE[key] = ref.query(q, qd, SCENE_A, bp, KP, KD, POINTER_RADIUS, dtype)
    return _CACHE[key]


def floors(family):
    """per output kind, the largest |float32 - float64| over the batch outside the exclusions"""
    r64, r32 = reference(family), reference(family, np.float32)
    ex = ref.exclusions(r64)
    geo, frc = ~ex["geometry"], ~ex["force"]
    d = lambda key, sl: np.abs(r32[key][..., sl].astype(np.float64) - r64[key][..., sl])  # noqa: E731
    env_ok = frc.all(axis=1)
    return dict(dist=d("points", slice(0, 1))[geo].max(), normal=d("points", slice(1, 4))[geo].max(),
                pos=d("points", slice(4, 7))[geo].max(), force=d("points", slice(8, 9))[frc].max(),
                vel=d("velocities", slice(0, 3)).max(), torque=d("torques", slice(0, 6))[env_ok].max(),
                lever=r64["lever"].max())
