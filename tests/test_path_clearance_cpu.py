"""CPU tests of the path-clearance reference (tests/path_clearance_ref.py), of the conditions the GPU comparisons rest on
(tests/path_clearance_cases.py), of scene.path_substeps, of the solve_ik_free scenario and of the call's host side (defaults and
the refusals that need no device).  Every test prints its figures before it asserts."""
import ctypes as C
import math

import numpy as np
import pytest

import contact_query_ref as cq
import path_clearance_cases as cases
import path_clearance_ref as ref


def test_reference_against_the_pointers_circle():
    """Only joint 1 turns: the pointer runs on a circle of radius rho about the z axis, a sphere body sits ON that circle at the
    angle phi, the pointer's sample alone is asked.  The centres are a chord 2 rho |sin((q1 - phi) / 2)| apart, so the clearance of
    every configuration, the smallest one and where it falls follow in closed form."""
    p0 = cq.query(np.zeros((1, 6)), np.zeros((1, 6)), ())["centres"][0, 22]
    rho, phi0 = math.hypot(p0[0], p0[1]), math.atan2(p0[1], p0[0])
    R, r, phi, M = 1.5, cases.POINTER_RADIUS, 0.5, 4
    body = cq.sphere(R, (rho * math.cos(phi0 + phi), rho * math.sin(phi0 + phi), p0[2]))
    way = np.zeros((1, 2, 6))
    way[0, 1, 0] = 1.2                                                   # q1: 0, 0.3, 0.6, 0.9, 1.2
    out = ref.sweep(way, M, (body,), mask=1 << 22, pointer_radius=r)
    q1 = np.array([0.0, 0.3, 0.6, 0.9, 1.2])
    want = 2 * rho * np.abs(np.sin((q1 - phi) / 2)) - R - r
    print(f"rho {rho:.4f}: clearance {out['clearance'][0]}, closed form {want}")
    assert rho > 10 and np.abs(out["clearance"][0] - want).max() <= 1e-9
    sm = out["summary"][0]
    assert abs(sm[0] - (2 * rho * math.sin(0.05) - R - r)) <= 1e-9 and sm[1] == 0.5 and sm[2] == 22 and sm[3] == 0
    hit = want < 0
    assert hit.sum() == 1 and sm[4] == 0.5 and sm[5] == 1 and sm[6] == 0 and sm[7] == 0
    wide = ref.sweep(way, M, (body,), margin=3.0, mask=1 << 22, pointer_radius=r)["summary"][0]
    assert wide[4] == 0.25 and wide[5] == (want < 3.0).sum() == 2 and wide[6] == 0      # configurations 1 and 2
    far = ref.sweep(way, M, (body,), margin=-5.0, mask=1 << 22, pointer_radius=r)["summary"][0]
    assert far[4] == -1 and far[5] == 0 and far[6] == 1


def test_reference_rules():
    """the interpolation rule, the -inf rule, the tie rules and the body-less answer"""
    w = cases.given_waypoints("k3_m3", 4)
    q = ref.configurations(w, 3)
    assert q.shape == (4, 7, 6) and np.array_equal(q[:, 0], w[:, 0]) and np.array_equal(q[:, 3], w[:, 1]) and np.array_equal(q[:, 6], w[:, 2])
    assert np.allclose(q[:, 4], w[:, 1] + (w[:, 2].astype(np.float64) - w[:, 1]) / 3, atol=1e-12)
    q32 = ref.configurations(w, 3, np.float32)
    assert q32.dtype == np.float32 and np.array_equal(q32[:, 3], w[:, 1])                # exactly b at j = M
    assert np.array_equal(ref.path_coordinates(3, 3), [0, 1 / 3, 2 / 3, 1, 1 + 1 / 3, 1 + 2 / 3, 2])
    assert ref.path_coordinates(3, 3, np.float32)[4] == np.float32(1) + np.float32(1) / np.float32(3)
    none = ref.sweep(w, 3, ())["summary"]
    assert np.array_equal(none, np.tile([np.inf, 0, 0, -1, -1, 0, 1, 0], (4, 1)))
    bad = w.copy()
    bad[2, 1, 3] = np.nan
    out = ref.sweep(bad, 3, cases.SCENE_A)
    good = ref.sweep(w, 3, cases.SCENE_A)
    assert out["summary"][2, 0] == -np.inf and out["summary"][2, 6] == 0
    assert np.array_equal(np.isneginf(out["clearance"][2]), [False, True, True, True, True, True, False])
    # the lowest configuration, then the lowest sample that joint 4 moves (15, the first of rotator2), then the lowest body
    assert out["summary"][2, 1] == 1 / 3 and out["summary"][2, 2] == 15 and out["summary"][2, 3] == 0
    assert np.array_equal(np.delete(out["summary"], 2, axis=0), np.delete(good["summary"], 2, axis=0))
    same = np.repeat(w[:, :1], 3, axis=1)
    tie = ref.sweep(same, 3, cases.SCENE_A)["summary"]
    assert (tie[:, 1] == 0).all() and np.isin(tie[:, 4], (0.0, -1.0)).all()
    only = ref.sweep(w, 3, cases.SCENE_A, mask=1 << 22)
    assert (only["summary"][:, 2] == 22).all() and (only["clearance"] >= good["clearance"]).all()


def test_the_conditions_the_gpu_comparisons_rest_on():
    """near-margin pairs are at most 1 % of all pairs (0 on the (K 4, M 5) set); the float32 floor holds and 8 x floor is inside
    the hard bar"""
    near = total = 0
    for name in cases.SHAPES:
        for family in "AB":
            cl = cases.reference(name, family)["clearance"]
            counts = [int(ref.near_margin(cl, m, cases.NEAR).sum()) for m in cases.MARGINS]
            srt = np.sort(cl, axis=1)
            print(f"{name} {family}: C {cl.shape[1]}, penetrating {(cl < 0).mean():.3f}, free envs {(cl >= 0).all(axis=1).mean():.3f}, "
                  f"near margins {cases.MARGINS}: {counts}, envs with two configurations within 1e-3 of the minimum "
                  f"{(srt[:, 1] - srt[:, 0] < 1e-3).mean():.2f}")
            assert np.isfinite(cl).all()
            assert max(counts) <= 0.01 * cl.size
            if name == "k4_m5":
                assert counts == [0, 0]
            near += sum(counts); total += 2 * cl.size
    cl = cases.reference("k4_m5", "A")["clearance"]
    assert abs((cl < 0).mean() - 0.14) < 0.01 and abs((cl >= 0).all(axis=1).mean() - 0.32) < 0.01
    floor = cases.floor()
    print(f"near-margin pairs {near} of {total}; float32 floor {floor:.3g}, constant {cases.DIST_FLOOR:.3g}, bar {cases.BAR:.3g}")
    assert floor <= cases.DIST_FLOOR <= 2 * floor
    assert cases.BAR == cases.FLOOR_MARGIN * cases.DIST_FLOOR <= cases.DIST_HARD


def test_path_substeps():
    from pioneer_amd.scene import path_substeps
    import torch
    w = np.zeros((3, 6))
    w[1, 2], w[2, 4] = 1.0, -0.5                                       # the longest joint move of a segment: 1.0, then 1.0 and 0.5
    assert path_substeps(w, 1.0) == 1 and path_substeps(w, 0.5) == 2 and path_substeps(w, 0.3) == 4 and path_substeps(w, 0.25) == 4
    assert path_substeps(w, 0.1) == 10 and path_substeps(w, 5.0) == 1 and path_substeps(w[:1], 0.1) == 1
    assert path_substeps(torch.from_numpy(w), 0.3) == 4 and path_substeps(np.stack([w, 2 * w]), 0.5) == 4
    for name in cases.SHAPES:                                           # the rule, on the case set: M is enough and M - 1 is not
        wp = cases.path_waypoints(name)
        if wp.shape[1] < 2:
            continue
        step = 0.2
        M = path_substeps(wp, step)
        longest = np.abs(np.diff(wp.astype(np.float64), axis=1)).max()
        assert longest / M <= step and (M == 1 or longest / (M - 1) > step)
        assert np.abs(np.diff(ref.configurations(wp, M), axis=1)).max() <= step + 1e-12
    with pytest.raises(AssertionError):
        path_substeps(w, 0.01)                                          # 100 sub-steps
    with pytest.raises(AssertionError):
        path_substeps(w, 0.0)
    with pytest.raises(AssertionError):
        path_substeps(np.zeros((3, 5)), 0.1)


def test_the_ik_scenario_has_envs_whose_winner_collides():
    s = cases.ik_scenario()
    per, clr = s["per"], s["clearance"]
    rows = np.arange(cases.IK_ENVS)
    share = s["counted"].mean()
    free = (per["converged_starts"] & (clr >= cases.IK_MARGIN)).any(axis=1)
    print(f"{cases.IK_ENVS} envs x {cases.IK_STARTS} starts: the winner collides while another converged start is free in "
          f"{share:.3f} of the envs (recorded {cases.IK_COLLIDING_SHARE}); the winner collides in "
          f"{(clr[rows, per['start']] < cases.IK_MARGIN).mean():.3f}; a converged free start exists in {free.mean():.3f}")
    assert share >= 0.1 and abs(share - cases.IK_COLLIDING_SHARE) <= 0.005
    assert 0 < free.mean() < 1                                          # both outcomes of `free` are exercised


def test_defaults_and_deviceless_refusals(hip_lib):
    from pioneer_amd import _lib
    p = _lib.PnrPathParams()
    assert hip_lib.pnr_path_params_default(p) == 0
    assert p.struct_size == C.sizeof(_lib.PnrPathParams) and (p.n_waypoints, p.substeps, p.from_current, p.waypoints_per_env) == (1, 8, 0, 0)
    assert p.lanes_per_env == 0 and p.sample_mask == (1 << _lib.CONTACT_SAMPLES) - 1 == ref.ALL_SAMPLES and p.margin == 0.0 and p.n_bodies == 0
    assert hip_lib.pnr_path_params_default(None) == -1
    assert hip_lib.pnr_path_clearance(None, p, None, None, None, None, None) == -1 and b"null handle" in hip_lib.pnr_last_error(None)
    header = open(_lib.HEADER).read()
    for name, value in (("PNR_MAX_PATH_WAYPOINTS", _lib.MAX_PATH_WAYPOINTS), ("PNR_MAX_PATH_SUBSTEPS", _lib.MAX_PATH_SUBSTEPS),
                        ("PNR_PATH_SUMMARY_DIM", _lib.PATH_SUMMARY_DIM)):
        assert f"#define {name} {value}\n" in header
    assert _lib.MAX_PATH_WAYPOINTS == 256 and _lib.MAX_PATH_SUBSTEPS == 64 and ref.SUMMARY_DIM == _lib.PATH_SUMMARY_DIM == 8
