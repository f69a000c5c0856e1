"""CPU tests of the contact query's reference (tests/contact_query_ref.py), of the inputs and floors the GPU tests rest on
(tests/contact_query_cases.py), and of the binding table.  Tests 1-5 need no HIP library; the oracle is the dynamics mode's own
float64 C oracle (oracle/pnr_dyn_oracle.c), whose contact model the query restates from outside."""
import ctypes as C

import numpy as np
import pytest

import contact_query_cases as cases
import contact_query_ref as ref
import link_kinematics_ref as lk
from oracle import DynOracle

GROUND_Z = 0.5
OBSTACLE = dict(obstacle_position=(10.0, 5.0, 0.0), obstacle_half_extents=(0.5, 0.5, 5.0))
SCENE = [("box", (12.0, -4.0, 3.0), (0.0, 0.0, float(np.sin(0.3)), float(np.cos(0.3))), (2.0, 1.0, 3.0)),
         ("sphere", (8.0, 8.0, 6.0), (0.0, 0.0, 0.0, 1.0), (3.0, 0.0, 0.0))]
N_ORC = 200


def _oracle(n):
    orc = DynOracle(n, dyn=dict(gravity=9.81, ground_z=GROUND_Z, link_contacts=1, scene=SCENE, **OBSTACLE))
    q, qd = cases.joints(n)
    orc.dstate["q"], orc.dstate["qd"] = q.astype(np.float64), qd.astype(np.float64)
    return orc, q.astype(np.float64), qd.astype(np.float64)


def _oracle_bodies():
    """the oracle's collision world as the query's body list: ground, obstacle box, scene (PioneerVectorEnv.collision_bodies' order)"""
    return [ref.plane((0, 0, 1), (0, 0, GROUND_Z)), ref.box(OBSTACLE["obstacle_half_extents"], OBSTACLE["obstacle_position"]),
            ref.box(SCENE[0][3], SCENE[0][1], SCENE[0][2]), ref.sphere(SCENE[1][3][0], SCENE[1][1])]


def _wrenches(res, q, e):
    """the reference's per-sample forces of env e as per-body spatial wrenches (moment about the body origin | force, body frame)"""
    R, p, _, _ = lk.link_frames(q[e:e + 1])
    f = np.zeros((6, 6))
    for s, (link, c, _) in enumerate(ref.sample_table()):
        fb = R[0, link].T @ res["force"][e, s]
        f[ref.LINK_TO_BODY[link], 0:3] += np.cross(c, fb)
        f[ref.LINK_TO_BODY[link], 3:6] += fb
    return f


def test_the_sample_table_is_the_oracles(oracle_built):
    orc = DynOracle(1, dyn=dict(link_contacts=1))
    got = orc.contact_samples()
    want = ref.sample_table()
    assert len(got) == len(want) == ref.SAMPLES == 23
    for (body, c, radius), (link, cw, rw) in zip(got, want):
        assert body == ref.LINK_TO_BODY[link] and np.array_equal(c, cw) and radius == rw
    assert got[22][2] < 0 and np.array_equal(got[22][1], [3.6, 0.0, 1.9])       # sample 22 is the pointer
    assert ref.SAMPLE_LINKS[:22] == tuple(link for link, _, _ in want[:22]) and ref.SAMPLE_LINKS[22] == 10


def test_the_sweep_in_float64_is_link_frames():
    """the two forms of the joint rotation, through the one walk: entry by entry (the float32 query's) against Rodrigues"""
    q, qd = cases.joints(50)
    for a, b in zip(lk.link_frames(q, qd, rotation=lk.coordinate_rotation), lk.link_frames(q, qd)):
        assert a.dtype == b.dtype == np.float64 and np.abs(a - b).max() < 1e-12
    with pytest.raises(AssertionError):                              # the entry-wise form is for +- a coordinate axis only
        lk.coordinate_rotation((0.6, 0.8, 0.0), q[:, 0])
    assert np.abs(lk.coordinate_rotation((0, -1, 0), q[:, 0], np.float32) - lk.axis_rotation((0, -1, 0), q[:, 0])).max() < 1e-7


def test_forces_as_body_wrenches_equal_the_oracles(oracle_built):
    orc, q, qd = _oracle(N_ORC)
    res = ref.query(q, qd, _oracle_bodies(), kp=orc.d.contact_kp, kd=orc.d.contact_kd, pointer_radius=orc.d.pointer_radius)
    active, worst = 0, 0.0
    for e in range(N_ORC):
        any_, want = orc.contact_wrenches(e)
        got = _wrenches(res, q, e)
        assert any_ == bool(np.abs(res["force"][e]).max() > 0)
        active += any_
        scale = max(np.abs(want).max(), 1.0)
        worst = max(worst, np.abs(got - want).max() / scale)
    print(f"{active} of {N_ORC} envs in contact; worst relative wrench difference {worst:.2e}")
    assert active >= N_ORC // 5
    assert worst <= 1e-9


def test_contact_torques_are_the_external_wrenches(oracle_built):
    """aba_ext(0, g, fext) == aba(tau_c, g): the query's joint torques do to the arm what the step's contact wrenches do"""
    orc, q, qd = _oracle(N_ORC)
    res = ref.query(q, qd, _oracle_bodies(), kp=orc.d.contact_kp, kd=orc.d.contact_kd, pointer_radius=orc.d.pointer_radius)
    worst, checked = 0.0, 0
    for e in range(N_ORC):
        any_, fext = orc.contact_wrenches(e)
        if not any_:
            continue
        a = orc.aba_ext(np.zeros(6), 9.81, fext, e=e)
        b = orc.aba(res["torques"][e], 9.81, e=e)
        worst = max(worst, np.abs(a - b).max() / max(np.abs(a).max(), 1.0))
        checked += 1
    print(f"{checked} envs; worst relative qdd difference {worst:.2e}")
    assert checked >= N_ORC // 5 and worst <= 1e-9


def test_exclusions_are_rare_and_contacts_are_common():
    for family in "AB":
        r = cases.reference(family)
        ex = ref.exclusions(r)
        d = r["points"][:, :, 0]
        near = [float((r["points"][:, :, 7] == b).mean()) for b in range(3)]
        pen_switch = int(((d < 0) & (r["box_gap"] < 1e-3)).sum())
        print(f"family {family}: penetrating pairs {(d < 0).mean():.4f}, envs with a contact {(d < 0).any(axis=1).mean():.3f}, nearest body "
              f"{near}, excluded geometry {ex['geometry'].mean():.5f} force {ex['force'].mean():.5f}, envs with an excluded pair "
              f"{ex['force'].any(axis=1).mean():.4f}, penetrating pairs at a face switch {pen_switch}")
        assert ex["geometry"].mean() <= 0.01 and ex["force"].mean() <= 0.01
        assert ex["force"].any(axis=1).mean() <= 0.05          # the torque comparison leaves out whole envs
        assert (d < 0).mean() >= 0.02
        for n in cases.SIZES[1:]:                              # .. and on every batch the GPU tests run
            assert ex["force"][:n].mean() <= 0.01
        # the summary's sample index is decided: samples 14 and 15 are one sphere (counted as one), and between any other two the
        # smallest distances differ by more than twice the tight distance bar on every env
        assert np.abs(r["centres"][:, ref.TWIN_SAMPLES[0]] - r["centres"][:, ref.TWIN_SAMPLES[1]]).max() < 1e-12
        two = np.sort(np.delete(d, ref.TWIN_SAMPLES[1], axis=1), axis=1)[:, :2]
        print(f"  smallest gap between the two nearest distinct samples {(two[:, 1] - two[:, 0]).min():.2e}")
        assert (two[:, 1] - two[:, 0]).min() > 2 * cases.FLOOR_MARGIN * cases.DIST_FLOOR
    sph = cases.reference("B")["dist"][:, :, cases.SPHERE_BODY]
    assert 0.3 <= (sph < 0).any(axis=1).mean() <= 0.9


def test_float32_floors_hold_and_sit_inside_the_hard_bars():
    fl = {k: max(cases.floors("A")[k], cases.floors("B")[k]) for k in cases.floors("A")}
    print({k: f"{v:.3e}" for k, v in fl.items()})
    for key, const in (("dist", cases.DIST_FLOOR), ("normal", cases.NORMAL_FLOOR), ("pos", cases.POS_FLOOR), ("vel", cases.VEL_FLOOR),
                       ("force", cases.FORCE_FLOOR), ("torque", cases.TORQUE_FLOOR)):
        assert fl[key] <= const <= 2 * fl[key], (key, fl[key], const)
    assert fl["lever"] <= cases.LEVER_MAX <= 1.01 * fl["lever"]
    m = cases.FLOOR_MARGIN
    assert m * cases.DIST_FLOOR <= cases.DIST_HARD and m * cases.POS_FLOOR <= cases.DIST_HARD
    assert m * cases.NORMAL_FLOOR <= cases.NORMAL_HARD
    assert m * cases.FORCE_FLOOR <= cases.FORCE_HARD and m * cases.TORQUE_FLOOR <= cases.TORQUE_HARD


def test_binding_table_has_the_contact_query():
    from pioneer_amd import _lib
    assert "pnr_get_contacts" in _lib.SIGNATURES and "pnr_contact_params_default" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["pnr_get_contacts"][1]) == 8
    assert _lib.CONTACT_SAMPLES == ref.SAMPLES and _lib.CONTACT_DIM == ref.DIM
    from pioneer_amd.scene import CONTACT_SAMPLE_LINKS
    assert CONTACT_SAMPLE_LINKS == ref.SAMPLE_LINKS


def test_contact_params_struct_matches_the_library(hip_lib):
    from pioneer_amd import _lib
    p = _lib.PnrContactParams()
    assert hip_lib.pnr_contact_params_default(p) == 0
    assert p.struct_size == C.sizeof(_lib.PnrContactParams)
    assert p.n_bodies == 0 and p.contact_kp == 2000.0 and p.contact_kd == 50.0
    assert hip_lib.pnr_contact_params_default(None) == -1 and b"null params" in hip_lib.pnr_last_error(None)
