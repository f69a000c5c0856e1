"""CPU tests of the time parameterisation (pnr_retime_path, pnr_sample_trajectory): the float64 reference of tests/retime_ref.py
against a second statement of its backward step and against the rows it must satisfy, the facts about the shared input families
(tests/retime_cases.py) that the GPU tests rely on, the float32 floor of the law on those inputs, and the binding's structs.
Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

import retime_cases as cases
import retime_ref as ref

_cache = {}


def family(name, n, C=17):
    key = (name, n, C)
    if key not in _cache:
        P = {"CORNER": lambda: cases.corner(n), "SMOOTH": lambda: cases.smooth(n, C), "HEAVY": lambda: cases.heavy(n, C),
             "DUP": lambda: cases.dup(n, C), "NAN": lambda: cases.with_nan(n, C)}[name]()
        scales = np.ones((n, 11), np.float32) if name == "HEAVY" else cases.scales_drawn(n)
        tau = cases.heavy_tau_limits(P, scales) if name == "HEAVY" else cases.tau_limits(P, scales)
        _cache[key] = (P, scales, tau)
    return _cache[key]


def timed(name, n, C=17, torque=True, dtype=np.float64):
    key = ("timed", name, n, C, torque, dtype)
    if key not in _cache:
        P, scales, tau = family(name, n, C)
        _cache[key] = ref.retime(P, cases.V_MAX, cases.A_MAX, tau if torque else None, scales, cases.GRAVITY, dtype=dtype)
    return _cache[key]


STEP_CASES = [("CORNER", 3, 17), ("SMOOTH", 2, 3), ("SMOOTH", 2, 4), ("SMOOTH", 2, 17), ("SMOOTH", 2, 33), ("SMOOTH", 1, 256),
              ("HEAVY", 2, 17), ("DUP", 2, 17)]


@pytest.mark.parametrize("torque", [False, True])
@pytest.mark.parametrize("name, n, C", STEP_CASES)
def test_the_pair_rule_equals_the_brute_force_step(name, n, C, torque):
    """Every backward step of the cases: K_k and the largest lower bound of the pair rule against the polygon's vertices."""
    r = timed(name, n, C, torque)
    A, B, c, lim = r["rows"]
    worst_hi = worst_lo = 0.0
    empties = steps = 0
    for e in range(n):
        for k in range(C - 2, -1, -1):
            Knext = r["K"][e, k + 1]
            got = ref.brute_backward_step(A[e, k], B[e, k], c[e, k], lim[e, k], r["X"][e, k], Knext)
            K, lo, empty = ref.backward_step(A[e:e + 1, k], B[e:e + 1, k], c[e:e + 1, k], lim[e:e + 1, k], r["X"][e:e + 1, k], r["K"][e:e + 1, k + 1])
            steps += 1
            if got is None:
                empties += 1
                assert empty[0] or lo[0] > K[0], (name, e, k, K, lo)
                continue
            assert not empty[0] and lo[0] <= K[0] * (1 + 1e-9) + 1e-12, (name, e, k, K, lo, got)
            scale = max(abs(got[1]), 1e-12)
            worst_hi = max(worst_hi, abs(K[0] - got[1]) / scale)
            worst_lo = max(worst_lo, abs(lo[0] - got[0]) / scale)
    print(f"{name} n={n} C={C} torque={torque}: {steps} steps, {empties} empty; |K - brute| / K <= {worst_hi:.2e}, lower end {worst_lo:.2e}")
    assert worst_hi <= 1e-9 and worst_lo <= 1e-9


FEASIBLE_CASES = [("CORNER", 17, False), ("CORNER", 17, True)] + [("SMOOTH", C, False) for C in cases.SIZES_C] \
    + [("SMOOTH", C, True) for C in cases.TORQUE_SIZES_C]


@pytest.mark.parametrize("name, C, torque", FEASIBLE_CASES)
def test_corner_and_smooth_are_feasible_and_satisfy_every_row(name, C, torque):
    n = max(cases.SIZES_N)
    P, scales, tau = family(name, n, C)
    r = timed(name, n, C, torque)
    r32 = timed(name, n, C, torque, np.float32)
    util, vel = ref.row_utilisation(P, r["sdot2"], cases.V_MAX, cases.A_MAX, tau if torque else None, scales, cases.GRAVITY)
    util32, vel32 = ref.row_utilisation(P, r32["sdot2"], cases.V_MAX, cases.A_MAX, tau if torque else None, scales, cases.GRAVITY)
    stops = int((r["sdot2"][:, 1:-1] == 0).sum())
    rel = np.abs(r32["duration"].astype(np.float64) - r["duration"]) / r["duration"]
    print(f"{name} C={C} torque={torque}: durations {r['duration'].min():.3f} .. {r['duration'].max():.3f} s; float64 utilisation "
          f"{util.max():.9f}, x / X {vel.max():.9f}; float32 {util32.max():.7f}, {vel32.max():.7f}; interior stops {stops}; "
          f"float32 duration off by {rel.max():.2e}")
    assert r["feasible"].all() and (r["fail_at"] == -1).all() and (r["reason"] == ref.FEASIBLE).all()
    assert r32["feasible"].all(), "the float32 verdict agrees"
    assert (r["sdot2"][:, 0] == 0).all() and (r["sdot2"][:, -1] == 0).all() and (r["sdot2"] >= 0).all()
    assert util.max() <= 1 + 1e-9 and vel.max() <= 1 + 1e-9
    assert np.abs(r["utilisation"] - util).max() <= 1e-9, "the summary's utilisation is that of the profile"
    assert np.maximum(util, vel).min() >= 1 - 1e-9, "time-optimal on the grid: some limit is active somewhere on every path"
    assert (np.diff(r["times"], axis=1) > 0).all() and np.array_equal(r["times"][:, -1], r["duration"])
    assert np.allclose(r["max_sdot"], np.sqrt(r["sdot2"].max(axis=1)), rtol=1e-15)


def test_halving_tau_max_never_shortens_a_path():
    P, scales, tau = family("CORNER", 37)
    full = timed("CORNER", 37)
    half = ref.retime(P, cases.V_MAX, cases.A_MAX, 0.75 * tau, scales, cases.GRAVITY)
    free = timed("CORNER", 37, torque=False)
    ok = half["feasible"]
    print(f"durations: no torque rows {free['duration'].mean():.3f}, tau_max {full['duration'].mean():.3f}, 0.75 tau_max "
          f"{half['duration'][ok].mean():.3f} ({int(ok.sum())} of 37 feasible)")
    assert (half["duration"] >= full["duration"]).all() and (full["duration"] >= free["duration"]).all()


def test_count_the_stops_and_stuck_endings_of_reversing_sinusoids():
    """What the header says about coarse grids, counted (nothing to hold a kernel to): sinusoids that reverse, and 4-point paths
    under torque rows."""
    n = max(cases.SIZES_N)
    scales = cases.scales_drawn(n)
    counts = {}
    for C in (17, 33, 256):
        P = cases.wavy(n, C)
        r = ref.retime(P, cases.V_MAX, cases.A_MAX)
        counts[C] = (int((~r["feasible"]).sum()), int(((r["sdot2"][:, 1:-1] == 0).any(axis=1) & r["feasible"]).sum()))
    P = cases.smooth(n, 4)
    r4 = ref.retime(P, cases.V_MAX, cases.A_MAX, cases.tau_limits(P, scales), scales, cases.GRAVITY)
    print(f"reversing sinusoids, {n} paths, acceleration rows: (stuck, feasible with an interior stop) per C: {counts}; "
          f"SMOOTH at C = 4 under torque rows: {int((~r4['feasible']).sum())} stuck, reasons {sorted(set(r4['reason']))}")
    assert counts[256] == (0, 0), "a fine grid has neither"
    assert set(r4["reason"]) <= {ref.FEASIBLE, ref.STUCK}


def test_heavy_reports_its_grid_point():
    r = timed("HEAVY", 8)
    P, scales, tau = family("HEAVY", 8)
    G = cases.gravity_torques(P, scales)
    print("HEAVY: |G_1| at points 0, 1:", G[0, :2, 1], "tau_max[1]", tau[1], "fail_at", r["fail_at"], "reason", r["reason"])
    assert (G[:, 0, 1] > tau[1]).all() and (G[:, 1:, 1] < tau[1]).all()
    assert not r["feasible"].any() and (r["fail_at"] == cases.HEAVY_POINT).all() and (r["reason"] == ref.EMPTY).all()
    assert np.isinf(r["duration"]).all() and (r["sdot2"] == 0).all() and (r["times"][:, 0] == 0).all() and np.isinf(r["times"][:, 1:]).all()
    assert (r["max_sdot"] == 0).all() and (r["utilisation"] == 0).all()
    assert timed("HEAVY", 8, torque=False)["feasible"].all(), "without the torque rows the same path is fine"


def test_duplicated_rows_report_stuck():
    C = 17
    r = timed("DUP", 8, C, torque=False)
    at = C - cases.DUP_ROWS + 1                     # rows 13 .. 16 are equal: d_14 = d_15 = 0, so x_14 = x_15 = 0
    print("DUP: fail_at", r["fail_at"], "reason", r["reason"])
    assert not r["feasible"].any() and (r["fail_at"] == at).all() and (r["reason"] == ref.STUCK).all()
    assert np.isfinite(r["times"][:, :at + 1]).all() and np.isinf(r["times"][:, at + 1:]).all() and np.isinf(r["duration"]).all()
    assert (r["sdot2"][:, at - 1] > 0).all() and (r["sdot2"][:, at:] == 0).all()
    two = cases.wavy(4, C, 404)
    two[:, -1] = two[:, -2]                         # two equal rows at the end only cost time: d_(C-2) is not 0
    assert ref.retime(two, cases.V_MAX, cases.A_MAX)["feasible"].all()


def test_a_nan_env_is_alone_in_failing():
    n, C = 8, 17
    r = timed("NAN", n, C, torque=False)
    clean = ref.retime(cases.smooth(n, C, 505), cases.V_MAX, cases.A_MAX)
    others = np.arange(n) != cases.NAN_ENV
    print("NAN: fail_at", r["fail_at"], "reason", r["reason"])
    assert r["feasible"][others].all() and not r["feasible"][cases.NAN_ENV]
    assert r["reason"][cases.NAN_ENV] == ref.NONFINITE and r["fail_at"][cases.NAN_ENV] == cases.NAN_POINT + 1      # the largest k whose rows see it
    for key in ("times", "sdot2", "duration", "utilisation"):
        assert np.array_equal(r[key][others], clean[key][others]), key


def test_sampling_follows_the_profile():
    """The reference's samples: at the grid times they are the grid points, the velocity is the profile's, the hold rows hold."""
    n, C = 6, 17
    P, _, _ = family("CORNER", n)
    r = timed("CORNER", n, torque=False)
    dt = 1.0 / 24
    from pioneer_amd.scene import steps_for
    T = steps_for(float(r["duration"].max()), dt) + 3
    out = ref.sample(P, r["times"], r["sdot2"], r["feasible"], r["duration"], 0.0, dt, T)
    assert out.shape == (n, T, 12)
    for e in range(n):
        last = steps_for(float(r["duration"][e]), dt)
        assert (out[e, last - 1:, :6] == P[e, -1]).all() and (out[e, last - 1:, 6:] == 0).all()
        assert last == 1 or not (out[e, last - 2, :6] == P[e, -1]).all()
    # inside an interval q is a quadratic of time: the central difference of three samples of one interval IS qd (to rounding).
    # |qd| may exceed v_max there: the velocity row bounds the central difference d_k at the grid points, the interval moves
    # along p_(k+1) - p_k (first-order collocation; at CORNER's corner the two differ most)
    tau = dt * np.arange(1, T + 1)
    worst = 0.0
    for e in range(n):
        k = np.searchsorted(r["times"][e], tau, side="right") - 1
        same = (k[2:] == k[:-2]) & (tau[2:] < r["duration"][e])
        fd = (out[e, 2:, :6] - out[e, :-2, :6]) / (2 * dt)
        worst = max(worst, np.abs(fd - out[e, 1:-1, 6:])[same].max())
        assert same.sum() >= 10
    print(f"sampling: |central difference of q - qd| inside an interval <= {worst:.2e}; |qd| up to {np.abs(out[..., 6:]).max():.3f} "
          f"against v_max {cases.V_MAX[0]}; {T} samples")
    assert worst <= 1e-9
    # an exact hit of a grid time gives the grid point
    e, k = 0, 5
    one = ref.sample(P[e:e + 1], r["times"][e:e + 1], r["sdot2"][e:e + 1], [True], r["duration"][e:e + 1], r["times"][e, k] - dt, dt, 1)
    assert np.abs(one[0, 0, :6] - P[e, k]).max() <= 1e-12
    assert steps_for(1.0, 0.25) == 4 and steps_for(1.01, 0.25) == 5 and steps_for(float("inf"), 0.25) == 1 and steps_for(0.0, 0.25) == 1


def test_binding_structs_defaults_and_refusals(hip_lib):
    from pioneer_amd import _lib
    assert (C.sizeof(_lib.PnrRetimeParams), C.sizeof(_lib.PnrRetimeBuffers), C.sizeof(_lib.PnrTrajSampleParams)) == (160, 48, 32)
    p = _lib.PnrRetimeParams()
    assert hip_lib.pnr_retime_params_default(p) == 0
    assert (p.struct_size, p.n_points, p.path_per_env, p.flags) == (160, 3, 0, 0)
    assert list(p.v_max) == [2.0] * 6 and list(p.a_max) == [10.0] * 6 and list(p.tau_max) == [0.0] * 6
    s = _lib.PnrTrajSampleParams()
    assert hip_lib.pnr_traj_sample_params_default(s) == 0
    assert (s.struct_size, s.n_points, s.path_per_env, s.n_samples, s.t0, s.dt) == (32, 3, 0, 1, 0.0, 10.0 / 240.0)
    assert (_lib.MAX_TRAJ_POINTS, _lib.MAX_TRAJ_SAMPLES, _lib.RETIME_SUMMARY_DIM, _lib.RETIME_ROW_DIM, _lib.RETIME_TORQUE) == (256, 65536, 8, 18, 1)
    assert (_lib.RETIME_FEASIBLE, _lib.RETIME_EMPTY, _lib.RETIME_STUCK, _lib.RETIME_NONFINITE) == (ref.FEASIBLE, ref.EMPTY, ref.STUCK, ref.NONFINITE)
    header = open(_lib.HEADER).read()
    for name, value in (("PNR_MAX_TRAJ_POINTS", 256), ("PNR_MAX_TRAJ_SAMPLES", 65536), ("PNR_RETIME_SUMMARY_DIM", 8), ("PNR_RETIME_ROW_DIM", 18)):
        assert f"#define {name} {value}\n" in header
    # refusals that need no device: NULL structs and a NULL handle
    assert hip_lib.pnr_retime_params_default(None) == -1 and b"null params" in hip_lib.pnr_last_error(None)
    assert hip_lib.pnr_traj_sample_params_default(None) == -1
    b = _lib.PnrRetimeBuffers()
    b.struct_size = C.sizeof(_lib.PnrRetimeBuffers)
    nbytes = C.c_uint64(7)
    assert hip_lib.pnr_retime_path(None, p, b, None) == -1 and b"null handle" in hip_lib.pnr_last_error(None)
    assert hip_lib.pnr_retime_workspace_bytes(None, p, C.byref(nbytes)) == -1 and nbytes.value == 7
    assert hip_lib.pnr_sample_trajectory(None, s, None, None, None, None, None, None) == -1
