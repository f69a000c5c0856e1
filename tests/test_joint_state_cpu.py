"""CPU tests of the float64 reference of pnr_get_joint_states (tests/joint_state_ref.py) and of the inputs and bars the GPU tests
use (tests/joint_state_cases.py): the bars' constants are the measured float32 floors, the bars are small against what they
measure, the reference's physics holds in float64, and the bars tell the mistakes a kernel could make apart.  Every test prints its
figures before it asserts.  No GPU.
"""
import numpy as np
import pytest

import external_force_ref as xref
import inverse_dynamics_ref as idref
import joint_state_cases as cases
import joint_state_ref as ref
import world_step_ref as wref

DOF = 6
ALL = cases.FAMILIES + ["hold"] + cases.CONSTRAINT

_CACHE = {}


def scenario(name):
    """(oracle, inputs, {form: reference}) of a scenario at N_MAX envs, computed once"""
    if name not in _CACHE:
        orc, I = cases.inputs(name)
        _CACHE[name] = (orc, I, {cases.form_name(*f): cases.reference(orc, I, *f) for f in cases.forms(name)})
    return _CACHE[name]


# ---- the conditions the bars rest on -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_floor_constants_hold_on_the_inputs(name):
    """floor <= constant <= 2 floor for every constant of the scenario, and every bar <= 1e-3 of its own quantity's batch median
    (hold's q̈, zero by construction: of the same arm's free-fall q̈)"""
    measured = cases.floors(name)
    cm = name in cases.CONSTRAINT
    table = cases.REACTION_AT_QDD if cm else cases.FLOORS
    assert set(table[name]) == set(measured)
    free_fall = None
    if name == "hold":
        orc, I = cases.hold_inputs()
        free_fall = np.median(np.abs(wref.accelerations(orc, I["motors"])), axis=0)
        print(f"hold: free-fall median |qdd| {free_fall}")
    for form, by_class in measured.items():
        assert set(table[name][form]) == set(by_class)
        for cls, o in by_class.items():
            consts = table[name][form][cls]
            for k, const in consts.items():
                if k == "tau_median":                                  # the motor torque's own batch median, rounded down
                    print(f"{name} {form} {cls} {k}: measured {o['median']['tau']}  constant {const}")
                    assert np.all(const <= o["median"]["tau"]) and np.all(o["median"]["tau"] <= 1.1 * const + 1e-300), (name, form, cls, k)
                    continue
                floor, med = o[("at_" + k) if cm else k], o["median"][("at_" + k) if cm else k].copy()
                if name == "hold" and k == "qdd":
                    med = free_fall
                allowed = cases.FLOOR_MARGIN * const
                if k == "tau":                                         # capped as cases.bars() caps it
                    allowed = np.minimum(allowed, cases.MAX_SHARE * consts["tau_median"])
                    print(f"{name} {form} {cls} tau: the bar is {(allowed / np.where(floor > 0, floor, 1.0))[floor > 0].min() if (floor > 0).any() else 0:.2f} floors at the least")
                ratio = allowed / np.where(allowed > 0, med, 1.0)
                print(f"{name} {form} {cls} {k}: measured {floor}  constant {const}  bar / median {ratio.max():.2e}")
                assert np.all(floor <= const) and np.all(const <= 2 * floor), (name, form, cls, k)
                assert np.all(ratio <= cases.MAX_SHARE), (name, form, cls, k, ratio)
                assert np.all(allowed >= floor), "a bar below the float32 floor could not be met by any float32 kernel"


@pytest.mark.parametrize("name", cases.FAMILIES + ["hold"])
def test_no_compared_joint_is_within_the_limit_clamps_reach(name):
    """q + h (qd + h q̈) stays inside the joint limits on the envs the GPU tests follow: the clamp, which is an integrator select
    and in neither output, does not act in the sub-step the query looks at.  Dc alone, whose motors pull at up to 7.7e3 rad/s^2,
    drives ONE followed joint onto a limit within the sub-step: that joint (any joint that ends within CLAMP_MARGIN of a limit) is
    what the step-against-preview test leaves out.  The count is exact, so that a drift of the inputs shows."""
    orc, I, refs = scenario(name)
    idx = np.union1d(np.arange(64), cases.followed(cases.N_MAX))
    for form, R in refs.items():
        room = cases.clamp_room(orc, I, R["qdd"])[idx]
        near = room <= cases.CLAMP_MARGIN
        print(f"{name} {form}: the nearest joint ends {room.min():.3e} rad inside its limits; {near.sum()} of {near.size} joints within the margin")
        assert near.sum() == (1 if name == "Dc" else 0)


@pytest.mark.parametrize("family", ["C", "Dc"])
def test_a_share_of_the_followed_envs_is_in_contact(family):
    hit = scenario(family)[2]["ext"]["hit"]
    for idx in (np.arange(64), cases.followed(cases.N_MAX)):
        share = hit[idx].mean()
        print(f"family {family}: {share:.1%} of {len(idx)} followed envs in contact")
        assert 0.05 <= share <= 0.95


# ---- the reference's physics, in float64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", cases.FAMILIES)
def test_the_axis_moment_is_the_total_joint_torque(family):
    """The reaction's moment along the joint axis (world-frame Newton-Euler over 11 links) equals the joint torque that gives the
    same q̈ on the oracle's merged six-body model, M (q̈ - ABA(0, fext)): the two statements of the model agree; and where the
    motor's law is known directly (PD), tau_motor + joint_torque - damping - friction."""
    orc, I, refs = scenario(family)
    n = 64
    for form, R in refs.items():
        M, _, _ = idref.mass_and_bias(orc, orc.d.gravity)
        qdd0 = np.stack([orc.aba_ext(np.zeros(DOF), orc.d.gravity, R["fext"][e], e) for e in range(n)])
        total = np.einsum("nij,nj->ni", M[:n], R["qdd"][:n] - qdd0)
        axis = ref.axis_moment(R["reaction"])[:n]
        err = np.abs(axis - total).max() / np.abs(total).max()
        print(f"family {family} {form}: axis moment vs M (qdd - ABA(0)): relative {err:.2e} at torques up to {np.abs(total).max():.3e}")
        assert err <= 1e-9
        law = wref.table_law(orc, I["motors"])
        if not np.isnan(law).any():
            tx = I["tau"].astype(np.float64) if form in ("ext", "torque") else 0.0
            stated = law + tx - wref.losses(orc)
            err = np.abs(ref.axis_moment(R["reaction"]) - stated).max() / max(np.abs(stated).max(), 1.0)
            print(f"family {family} {form}: axis moment vs tau_motor + joint_torque - losses: relative {err:.2e}")
            assert err <= 1e-9


def test_the_held_arm_rests_and_joint_0_carries_its_weight_and_the_payload():
    orc, I = cases.hold_inputs(rounded=False)
    R = cases.reference(orc, I)
    fall = wref.accelerations(orc, I["motors"])
    rel = np.abs(R["qdd"]).max() / np.abs(fall).max()
    print(f"hold: |qdd| {np.abs(R['qdd']).max():.3e} against a free fall of {np.abs(fall).max():.3e}: {rel:.2e}")
    assert rel <= 1e-9
    Rb, _ = xref.body_frames(I["q"].astype(np.float64))
    world = np.einsum("nij,nj->ni", Rb[:, 0], R["reaction"][:, 0, 0:3])
    weight = orc.dstate["mass_scale"][:, 1:].sum(axis=1) * 9.81 + cases.HOLD_W
    err = np.abs(world - np.stack([0 * weight, 0 * weight, weight], axis=1)).max()
    print(f"hold: joint 0's force in the world against (0, 0, sum m g + W): {err:.3e} at weights of {weight.min():.1f} .. {weight.max():.1f}")
    assert err <= 1e-9 * weight.max()
    assert np.all(R["tau_motor"] == 0.0)


# ---- the bars bite ---------------------------------------------------------------------------------------------------------------------
MISTAKES = {
    "the wrenches left out": (dict(use_wrenches=False), ["B", "D"], "all"),
    "the contacts left out": (dict(contacts=False), ["C", "Dc"], "contact"),
    "gravity left out": (dict(gravity=0.0), ["A"], "all"),
    "the caller's torques left in the motor torque": (dict(use_torques=False), ["D", "Dc"], "all"),
    "the reaction in the parent's frame": (dict(frame="parent"), ["A", "B"], "all"),
}


@pytest.mark.parametrize("mistake", list(MISTAKES))
def test_the_bars_tell_a_mistake_apart(mistake):
    """each mistake moves the reference by more than 10 bars on most of the envs it can show on, in at least one family"""
    kw, families, who = MISTAKES[mistake]
    shares = []
    for family in families:
        orc, I, refs = scenario(family)
        good = refs["ext"]
        bad = cases.reference(orc, I, **kw)
        bar = cases.bars(family, "ext", good["hit"])
        gf, gm = cases.split(good["reaction"])
        bf, bm = cases.split(bad["reaction"])
        moved = (np.abs(bf - gf).max(axis=2) > 10 * bar["force"]) | (np.abs(bm - gm).max(axis=2) > 10 * bar["moment"]) \
            | (np.abs(bad["tau_motor"] - good["tau_motor"]) > 10 * np.maximum(bar["tau"], 1e-300))
        envs = good["hit"] if who == "contact" else np.ones(orc.n, dtype=bool)
        shares.append(moved.any(axis=1)[envs].mean())
        print(f"{mistake}, family {family}: more than 10 bars on {shares[-1]:.1%} of {int(envs.sum())} envs")
    assert max(shares) > 0.5
