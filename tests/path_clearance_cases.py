"""The inputs of the path-clearance tests, shared by the CPU tests (which measure on them what float32 arithmetic alone costs and
assert the conditions the GPU comparisons rest on) and the GPU tests (which run the kernel on exactly these inputs).  Nothing
here is a reference: that is tests/path_clearance_ref.py.

Waypoints: uniform in +-0.9 x the URDF limits, from a generator of their own per shape, drawn for N_MAX envs so that the inputs
of n envs are the first n rows.  All values are float32 numbers.  The bodies are contact_query_cases.SCENE_A.  Family A: the three
bodies where they are, for all envs.  Family B: the same plane and box, and the sphere per env (body_positions) near one of the
env's sample centres AT WAYPOINT 1 of its path (the last waypoint of a path of one), placed as
contact_query_cases.family_b_positions places it.

Measured with the float64 reference on the N_MAX envs (test_path_clearance_cpu.py prints them), shape (K 4, M 5), family A:
14 % of the configurations penetrate, 32 % of the envs are free at margin 0, no clearance lies within 1e-3 of margin 0 or of
margin 0.5 (over all shapes and families at most 5 of 10 530 configurations do); 18 % of the envs have two configurations within 1e-3 of the path's minimum (configurations
whose nearest pair is the base sample at its constant 2.3 above the plane tie with each other), which is why the index outputs
are not compared by equality under an exclusion cap but through the reference's distance of the reported triple.

THE FLOAT32 FLOOR: the largest |float32 - float64| of the reference's clearance over every shape and family (the interpolation
in each dtype), rounded up to two digits: DIST_FLOOR; test_path_clearance_cpu.py asserts floor <= DIST_FLOOR <= 2 floor.  The
kernel is allowed FLOOR_MARGIN = 8 times it, never more than the contact query's hard bar DIST_HARD = 1e-4.
"""
import numpy as np

import contact_query_cases as cqc
import contact_query_ref as cq
import path_clearance_ref as ref

SEED = 20261021
N_MAX = 130
SIZES = (1, 37, 64, 130)                    # one env, a partial wave, a full one, more than two
POINTER_RADIUS = cqc.POINTER_RADIUS
SCENE_A = cqc.SCENE_A
MARGINS = (0.0, 0.5)
NEAR = 1e-3
FLOOR_MARGIN = cqc.FLOOR_MARGIN
DIST_HARD = cqc.DIST_HARD
DIST_FLOOR = 4.6e-06                        # measured 4.54e-06 (module docstring)
BAR = min(FLOOR_MARGIN * DIST_FLOOR, DIST_HARD)

# name: (K given waypoints, M sub-steps, lanes_per_env values (0: auto), from_current)
SHAPES = {
    "k4_m5": (4, 5, (0,), False),           # C = 16
    "k3_m3": (3, 3, (4, 64), False),        # C = 7: not a multiple of P, and C < P
    "k5_m20": (5, 20, (64,), False),        # C = 81: two trips with a short last trip
    "k1_m4_current": (1, 4, (0,), True),    # from_current: C = 5
    "k16_m1": (16, 1, (0,), False),         # the candidate-set use: C = 16
}


def given_waypoints(name, n=N_MAX):
    """[n, K, 6] float32: the waypoints handed to the call"""
    K = SHAPES[name][0]
    lo, hi = cqc.limits()
    seed = SEED + 10 * list(SHAPES).index(name)
    return np.random.default_rng(seed).uniform(0.9 * lo, 0.9 * hi, size=(N_MAX, K, 6))[:n].astype(np.float32)


def current_joints(n=N_MAX):
    """[n, 6] float32: the envs' own joints of the from_current shape"""
    lo, hi = cqc.limits()
    return np.random.default_rng(SEED + 1).uniform(0.9 * lo, 0.9 * hi, size=(N_MAX, 6))[:n].astype(np.float32)


def path_waypoints(name, n=N_MAX):
    """[n, W, 6] float32: the whole path, the env's own joints in front where the shape starts from them"""
    w = given_waypoints(name, n)
    return np.concatenate([current_joints(n)[:, None, :], w], axis=1) if SHAPES[name][3] else w


def family_b_positions(name, n=N_MAX):
    """body_positions [n, 3, 3] float32: the plane's and the box's own positions, the sphere near one of the env's samples at waypoint 1"""
    w = path_waypoints(name)
    q = w[:, min(1, w.shape[1] - 1)]
    centres = cq.query(q, np.zeros_like(q), ())["centres"]
    rng = np.random.default_rng(SEED + 2 + 10 * list(SHAPES).index(name))
    pick = rng.integers(0, cq.SAMPLES, size=N_MAX)
    radii = np.array([POINTER_RADIUS if r < 0 else r for _, _, r in cq.sample_table()])
    d = rng.normal(size=(N_MAX, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    length = rng.uniform(0.5, 1.5, size=N_MAX) * (cqc.SPHERE_RADIUS + radii[pick])
    bp = np.zeros((N_MAX, 3, 3))
    for b in range(3):
        bp[:, b] = SCENE_A[b]["position"]
    bp[:, cqc.SPHERE_BODY] = centres[np.arange(N_MAX), pick] + length[:, None] * d
    return bp[:n].astype(np.float32)


_CACHE = {}


def reference(name, family, margin=0.0, dtype=np.float64):
    """The reference's sweep of the N_MAX envs of a shape and family (computed once, shared, left unchanged)"""
    key = (name, family, margin, np.dtype(dtype).name)
    if key not in _CACHE:
        bp = family_b_positions(name) if family == "B" else None
        _CACHE[key] = ref.sweep(path_waypoints(name), SHAPES[name][1], SCENE_A, bp, margin, pointer_radius=POINTER_RADIUS, dtype=dtype)
    return _CACHE[key]


def floor():
    """the largest |float32 - float64| clearance over every shape and family"""
    return max(float(np.abs(reference(name, f, dtype=np.float32)["clearance"] - reference(name, f)["clearance"]).max())
               for name in SHAPES for f in "AB")


# ---- the solve_ik_free scenario ---------------------------------------------------------------------------------------------------
# The position task on ik_multi_ref's target box with the default table of 16 starts, q_ref the rest pose (start 0), and ONE box
# on the ground in front of the target box, where the branches nearest to the rest pose pass.  Measured with the float64
# references on the IK_ENVS envs (test_path_clearance_cpu.py prints and asserts it): in 54 % of the envs solve_ik_multi's own
# winner is more than IK_CLEAR inside the box while another converged start is more than IK_CLEAR clear of it; 90 % of the envs
# have a converged free start.  (The first placement tried, a box of half extents (3, 6, 1.5) at (12, 0, 1.5), gave 1 %.)
IK_ENVS = 130
IK_STARTS = 16
IK_MARGIN = 0.0
IK_CLEAR = 0.05
IK_BOX = cq.box((2.0, 6.0, 2.0), (15.0, 0.0, 2.0))
IK_COLLIDING_SHARE = 0.538                  # measured (70 of 130 envs); the tests ask for at least one env in ten


def ik_scenario():
    """dict of the float64 references' view: targets [n, 3] float32, per (ik_multi_ref.solve_multi's dict), clearance [n, S] of
    every start's solution, counted [n] (the envs whose multi-start winner collides while another converged start is free, both
    by more than IK_CLEAR)"""
    if "ik" not in _CACHE:
        import ik_multi_ref as mref
        tgt = mref.box_targets(IK_ENVS)
        per = mref.solve_multi(mref.POSITION, tgt, None, mref.start_table(IK_STARTS), **mref.POSITION_DEFAULTS)
        clr = ref.sweep(per["all_q"].astype(np.float32), 1, (IK_BOX,), pointer_radius=POINTER_RADIUS)["clearance"]
        rows = np.arange(IK_ENVS)
        conv = per["converged_starts"]
        counted = (conv.any(axis=1) & (clr[rows, per["start"]] < IK_MARGIN - IK_CLEAR)
                   & (conv & (clr > IK_MARGIN + IK_CLEAR)).any(axis=1))
        _CACHE["ik"] = dict(targets=tgt, per=per, clearance=clr, counted=counted)
    return _CACHE["ik"]
