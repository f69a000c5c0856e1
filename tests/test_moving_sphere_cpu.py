"""CPU tests of the moving sphere's float64 reference (tests/moving_sphere_ref.py, stepped by tests/world_step_ref.py) and of the inputs the GPU tests run on
(tests/moving_sphere_cases.py): closed forms of the law, the conditions on the inputs, and the reference's own float32-storage
deviation, which sets the sphere's bars in tests/test_gpu_moving_sphere.py (4 x) and is written to moving_sphere_margins.json."""
import numpy as np
import pytest

import moving_sphere_cases as cases
import moving_sphere_ref as ref
import world_step_ref as wref
from bars import Q_TOL, QD_TOL


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_built):
    return oracle_built


def test_a_sphere_at_rest_on_the_ground_sits_where_spring_and_weight_balance():
    """z = ground_z + radius - m g / kp, v = 0 is a fixed point of the law, and a sphere dropped near it settles there"""
    orc = cases.make_oracle("C", 4)
    kp, g, gz = orc.d.contact_kp, orc.d.gravity, orc.d.ground_z
    m, r = np.array([0.5, 1.0, 2.0, 4.0]), np.array([0.3, 0.5, 1.0, 1.5])
    x = np.stack([np.full(4, 60.0), np.full(4, 30.0), gz + r - m * g / kp], axis=1)          # away from the box, beyond the pointer
    s = ref.sphere(x, np.zeros((4, 3)), m, r)
    wref.world_step(orc, cases.TRACK, sphere=s)
    assert np.abs(s["x"] - x).max() < 1e-12 and np.abs(s["v"]).max() < 1e-12
    s = ref.sphere(x + [0.0, 0.0, 0.01], np.zeros((4, 3)), m, r)
    for _ in range(100):
        wref.world_step(orc, cases.TRACK, sphere=s)
    assert np.abs(s["x"] - x).max() < 1e-9 and np.abs(s["v"]).max() < 1e-8


@pytest.mark.parametrize("family", ["A", "B"])
def test_arm_and_sphere_exchange_opposite_forces(family):
    """the force on the sphere and the reactions on the arm's bodies (taken back to the world frame) sum to zero, and so do their
    moments about the origin"""
    import external_force_ref as ext
    orc = cases.make_oracle(family, cases.SIZES[0])
    s, _, _ = cases.scenario(family, orc, cases.followed(cases.SIZES[0]))
    F, fext, on = ref.arm_forces(orc, s, ref.params_of(orc))
    assert on.any()
    R, o = ext.body_frames(orc.dstate["q"])
    f_world = np.einsum("nbij,nbj->nbi", R, fext[:, :, 3:6])
    n_world = np.einsum("nbij,nbj->nbi", R, fext[:, :, 0:3]) + np.cross(o, f_world)
    assert np.abs(F + f_world.sum(axis=1)).max() <= 1e-9 * max(1.0, np.abs(F).max())
    # the sphere's force acts along the line of centres, so its moment may be taken at the sphere's centre
    assert np.abs(np.cross(s["x"], F) + n_world.sum(axis=1)).max() <= 1e-8 * max(1.0, np.abs(np.cross(s["x"], F)).max())


@pytest.mark.parametrize("n", cases.SIZES)
@pytest.mark.parametrize("family", list(cases.FAMILIES))
def test_the_inputs_are_well_conditioned(family, n):
    """A, B: between 5 % and 95 % of the followed envs' spheres touch the arm at step 0 and the sphere moves qd by more than
    10 x QD_TOL; C: at least 90 % of the followed envs that have a sphere touch the ground, a tenth of the envs have none"""
    idx = cases.followed(n)
    full = cases.make_oracle(family, n)
    orc, plain = cases.make_oracle(family, len(idx), reset=False), cases.make_oracle(family, len(idx), reset=False)
    for o in (orc, plain):
        o.state[:] = full.state[idx]
        o.dstate[:] = full.dstate[idx]
    s, _, _ = cases.scenario(family, orc, idx)
    plain.dstate[:] = orc.dstate
    first = wref.world_step(orc, cases.TRACK, sphere=s)[0]
    on_arm, on_static = first["on_arm"], first["on_static"]
    gone = {k: v.copy() for k, v in s.items()}
    gone["m"][:] = 0.0
    wref.world_step(plain, cases.TRACK, sphere=gone)
    effect = np.abs(orc.dstate["qd"] - plain.dstate["qd"]).max()
    live = s["m"] > 0
    print(f"family {family} n={n}: {on_arm.mean():.2%} touch the arm, {on_static[live].mean():.2%} of the spheres touch the static world, "
          f"{1 - live.mean():.2%} of the envs have none; the sphere moves qd by {effect:.3e}")
    if family == "C":
        assert on_static[live].mean() >= 0.90 and not on_arm.any() and 0.05 <= 1 - live.mean() <= 0.15
    else:
        assert 0.05 <= on_arm.mean() <= 0.95 and effect > 10 * QD_TOL


def test_float32_storage_stays_within_a_quarter_of_the_joint_bars_and_sets_the_sphere_bars():
    from test_gpu_dynamics import _record_margin as record     # the dynamics tests' margin files: this one's goes next to them
    for family in cases.FAMILIES:
        m = cases.reference_margins(family)
        bx, bv = cases.sphere_bars(family)
        print(f"family {family}: float32 storage moves q {m['q']:.3e} qd {m['qd']:.3e}, the sphere's x {m['x']:.3e} v {m['v']:.3e}; bars {bx:.3e} {bv:.3e}")
        assert m["q"] <= Q_TOL / 4 and m["qd"] <= QD_TOL / 4, (family, m)
        assert m["x"] > 0 and m["v"] > 0
        record(family, None, None, file="moving_sphere_margins.json", figures=dict(m, position_bar=bx, velocity_bar=bv))
