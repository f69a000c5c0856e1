"""CPU tests of the grip's float64 reference (tests/grip_ref.py), of the inputs the GPU tests run on (tests/grip_cases.py) and of
the binding table: with nothing gripped the reference is tests/world_step_ref.py's sphere step to the last bit, the grip and its
reaction are equal and opposite, the cap holds, the inputs are well conditioned, the hold scenario reaches its bound after the K
world steps that tests/test_gpu_grip.py then runs, and pioneer_amd/_lib.py states what include/pioneer_amd.h declares."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import external_force_ref as ext
import grip_cases as cases
import grip_ref as gref
import moving_sphere_ref as sref
import world_step_ref as wref
from bars import Q_TOL, QD_TOL


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_built):
    return oracle_built


def _pair(family, n):
    """two oracles with the family's inputs, the sphere's state twice, and the inputs"""
    idx = cases.followed(n)
    a, b = cases.make_oracle(family, n), cases.make_oracle(family, n)
    s, fmax, tau, tg = cases.scenario(family, a, idx)
    b.dstate[:] = a.dstate
    return a, b, s, {k: v.copy() for k, v in s.items()}, fmax, tau, tg


@pytest.mark.parametrize("storage32", [False, True])
@pytest.mark.parametrize("form", cases.FORMS)
@pytest.mark.parametrize("family", list(cases.FAMILIES))
def test_nothing_gripped_is_the_world_step_reference_bit_for_bit(family, form, storage32):
    a, b, sa, sb, fmax, tau, tg = _pair(family, cases.SIZES[0])
    te, tt, joints = cases.form_inputs(form, tau, tg)
    for _ in range(2):
        got = gref.world_step(a, cases.TRACK, sphere=sa, max_force=np.zeros_like(fmax), grip_params=cases.FAMILIES[family]["grip"],
                              tau_ext=te, targets=tt, joints=joints, storage32=storage32)
        want = wref.world_step(b, cases.TRACK, sphere=sb, tau_ext=te, targets=tt, joints=joints, storage32=storage32)
        for k in ("q", "qd"):
            assert np.array_equal(a.dstate[k], b.dstate[k]), (family, form, k)
        for k in ("x", "v"):
            assert np.array_equal(sa[k], sb[k]), (family, form, k)
        assert not got["force"].any()
        assert np.array_equal(got["records"][0]["arm_force"], want[0]["arm_force"]) and want[0]["on_arm"].any()


@pytest.mark.parametrize("family", list(cases.FAMILIES))
def test_grip_and_reaction_are_equal_and_opposite(family):
    """Newton's third law, stated in the world frame: the reaction on body 5 is -F, and its moment about body 5's origin is that of
    -F acting at the anchor point p_a, which in body coordinates is c_a x f."""
    orc = cases.make_oracle(family, cases.SIZES[0])
    s, fmax, _, _ = cases.scenario(family, orc, cases.followed(cases.SIZES[0]))
    g = gref.grip_force(orc, s, fmax, gref.params_of(sref.params_of(orc), cases.FAMILIES[family]["grip"]))
    on = g["held"]
    assert on.sum() > 0.5 * len(on) and np.abs(g["F"][on]).max() > 1.0 and not g["F"][~on].any() and not g["fext"][~on].any()
    assert not g["fext"][:, :gref.POINTER_BODY].any()
    R, o = ext.body_frames(orc.dstate["q"])
    R5, o5 = R[:, gref.POINTER_BODY], o[:, gref.POINTER_BODY]
    f_world = np.einsum("nij,nj->ni", R5, g["fext"][:, gref.POINTER_BODY, 3:6])
    n_world = np.einsum("nij,nj->ni", R5, g["fext"][:, gref.POINTER_BODY, 0:3])
    scale = max(1.0, np.abs(g["F"]).max())
    assert np.abs(g["F"] + f_world).max() <= 1e-12 * scale
    assert np.abs(n_world - np.cross(g["p_a"] - o5, -g["F"])).max() <= 1e-10 * scale
    c = g["c_a"]
    assert np.abs(g["fext"][:, gref.POINTER_BODY, 0:3] - np.cross(c, g["fext"][:, gref.POINTER_BODY, 3:6])).max() <= 1e-10 * scale


@pytest.mark.parametrize("family", list(cases.FAMILIES))
def test_the_cap(family):
    """|F| <= max_force (1 + 1e-12) in every sub-step of every held env, F = F_r where |F_r| <= max_force; F = 0 at F_r = 0"""
    orc = cases.make_oracle(family, cases.SIZES[0])
    s, fmax, _, _ = cases.scenario(family, orc, cases.followed(cases.SIZES[0]))
    capped = 0
    for _ in range(cases.STEPS):
        for rec in gref.world_step(orc, cases.TRACK, sphere=s, max_force=fmax, grip_params=cases.FAMILIES[family]["grip"])["records"]:
            on = rec["held"]
            size, raw = np.linalg.norm(rec["grip_force"], axis=1), np.linalg.norm(rec["grip_raw"], axis=1)
            assert (size[on] <= fmax[on] * (1 + 1e-12)).all()
            below = on & (raw <= fmax)
            assert np.array_equal(rec["grip_force"][below], rec["grip_raw"][below])
            above = on & (raw > fmax)
            assert np.abs(size[above] - fmax[above]).max(initial=0.0) <= 1e-9 * cases.FAMILIES[family]["max_force"]
            capped += int(above.sum())
    assert (capped > 0) == (family == "G2")
    # at the anchor, at its velocity: F_r = 0 and F = 0, no 0 / 0
    orc = cases.make_oracle(family, 4)
    gp = gref.params_of(sref.params_of(orc), cases.FAMILIES[family]["grip"])
    radius = np.full(4, 0.5)
    _, pa, va, _ = gref.anchor_kinematics(orc.dstate["q"], orc.dstate["qd"], radius, orc.d.pointer_radius, gp)
    g = gref.grip_force(orc, sref.sphere(pa, va, np.ones(4), radius), np.full(4, 10.0), gp)
    assert g["held"].all() and np.isfinite(g["F"]).all() and np.abs(g["F"]).max() <= 1e-9


def test_the_inputs_are_well_conditioned_and_set_the_bars():
    """4 x the reference's own float32-storage deviation of q and qd stays under Q_TOL / QD_TOL for both families and all forms (the
    same ratio sets the sphere's and the force's bars); G1 never reaches its cap, G2's caps between 0.3 and 0.7 of its envs"""
    for family in cases.FAMILIES:
        m = cases.reference_margins(family)
        bx, bv, bf = cases.grip_bars(family)
        print(f"family {family}: float32 storage moves q {m['q']:.3e} qd {m['qd']:.3e}, the sphere's x {m['x']:.3e} v {m['v']:.3e}, the force "
              f"{m['f']:.3e}; bars {bx:.3e} {bv:.3e} {bf:.3e}; capped share {m['capped']:.2%}")
        assert 4 * m["q"] <= Q_TOL and 4 * m["qd"] <= QD_TOL, (family, m)
        assert m["x"] > 0 and m["v"] > 0 and m["f"] > 0
        if family == "G1":
            assert m["capped"] == 0.0
        else:
            assert 0.3 <= m["capped"] <= 0.7
    for family in cases.FAMILIES:                                       # a fifth released, a tenth without a sphere
        orc = cases.make_oracle(family, cases.N_MAX)
        q, qd = cases.msc.states(cases.FAMILIES[family]["base"], orc.state["r"])
        w, fmax = cases.spheres(family, q, qd)
        released, gone = float((fmax <= 0).mean()), float((w[6] <= 0).mean())
        print(f"family {family}: {released:.2%} released, {gone:.2%} without a sphere")
        assert 0.15 <= released <= 0.25 and 0.07 <= gone <= 0.13
        w97, f97 = cases.spheres(family, q[:97], qd[:97])
        assert np.array_equal(w97, w[:, :97]) and np.array_equal(f97, fmax[:97])      # the inputs of n envs are a prefix


def test_hold_at_rest_reaches_its_bound():
    """PD targets held, gravity on, the sphere gripped at the anchor at rest: after K world steps |x - p_a| <= 1.5 m g / grip_kp.
    K is what is chosen (the smallest multiple of 10 on the reference), never the bound."""
    K, err = cases.hold_steps()
    print(f"hold: K = {K} world steps, |x - p_a| {err:.3e} of {cases.hold_bound():.3e} (static sag {cases.HOLD['mass'] * cases.G / cases.GRIP_KP:.3e})")
    assert K % 10 == 0 and K >= 10 and err <= cases.hold_bound()
    assert err >= 0.5 * cases.HOLD["mass"] * cases.G / cases.GRIP_KP        # .. and it does sag: the weight hangs on the spring


def test_the_binding_table_states_what_the_header_declares():
    from pioneer_amd import _lib
    header = open(_lib.HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert int(re.search(r"^#define\s+PNR_BODY_GRIP_WORDS\s+(\d+)", header, re.M).group(1)) == _lib.BODY_GRIP_WORDS == 4
    struct = re.search(r"typedef struct pnr_body_grip_params \{(.*?)\} pnr_body_grip_params;", code, re.S).group(1)
    assert re.sub(r"\s+", " ", struct).strip() == "uint32_t struct_size; float anchor[3], direction[3]; float grip_kp, grip_kd;"
    fields = [(n, t) for n, t in _lib.PnrBodyGripParams._fields_]
    assert fields == [("struct_size", C.c_uint32), ("anchor", C.c_float * 3), ("direction", C.c_float * 3), ("grip_kp", C.c_float),
                      ("grip_kd", C.c_float)] and C.sizeof(_lib.PnrBodyGripParams) == 36
    VP, P = C.c_void_p, C.POINTER(_lib.PnrBodyGripParams)
    want = {"pnr_body_grip_params_default": ("pnr_body_grip_params* p", [P]),
            "pnr_set_body_grip_params": ("pnr_handle h, const pnr_body_grip_params* params", [VP, P]),
            "pnr_set_body_grip": ("pnr_handle h, const float* max_force, const uint8_t* mask, void* stream", [VP, VP, VP, VP]),
            "pnr_get_body_grip": ("pnr_handle h, float* out, void* stream", [VP, VP, VP])}
    for name, (args, types) in want.items():
        assert re.search(r"\bint %s\(%s\);" % (name, re.escape(args)), code), name
        assert _lib.SIGNATURES[name] == (C.c_int, types), name
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(os.path.dirname(_lib.HEADER), "..", doc)).read()
        for name in want:
            assert name in text, (doc, name)
