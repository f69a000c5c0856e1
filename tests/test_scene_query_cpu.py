"""CPU tests of the scene queries' per-env world (pnr_render_bodies, pnr_set_body_queries): the two symbols are declared and
exported, and the conditions hold on tests/scene_query_cases.py under which the GPU comparisons of tests/test_gpu_scene_queries.py
cannot pass on nothing: the composed references (tests/scene_query_ref.py) show every env's moving sphere on at least 20 pixels
and to at least 10 % of the rays outside their ambiguity bands, at least 0.9 of all pixels and rays lie outside the bands, the env
without a sphere shows none, and the contact cases touch the sphere with a damping term that matters."""
import ctypes as C

import numpy as np
import pytest

import contact_query_ref as cq
import scene_query_cases as cases
import scene_query_ref as sref
from test_abi import declared_functions

def test_the_two_symbols_are_declared_and_exported(hip_lib):
    from pioneer_amd import _lib
    names = declared_functions()
    for name, nargs in (("pnr_render_bodies", 8), ("pnr_set_body_queries", 3)):
        assert name in names and hasattr(hip_lib, name)
        assert _lib.SIGNATURES[name][0] is C.c_int and len(_lib.SIGNATURES[name][1]) == nargs
    assert (_lib.BODY_IN_RENDER, _lib.BODY_IN_RAYS, _lib.BODY_IN_CONTACTS) == (1, 2, 4)
    assert _lib.SEG_MOVING_BODY == _lib.SEG_BODY0 + _lib.MAX_SCENE == cases.SEG_MOVING_BODY == sref.SEG_MOVING_BODY == 21
    header = open(_lib.HEADER).read()
    assert "PNR_SEG_MOVING_BODY = 21" in header and "PNR_BODY_IN_RENDER = 1, PNR_BODY_IN_RAYS = 2, PNR_BODY_IN_CONTACTS = 4" in header
    assert hip_lib.pnr_set_body_queries(None, 0, None) == -1 and hip_lib.pnr_render_bodies(None, None, None, None, None, None, None, None) == -1


def test_the_case_table_has_the_shape_the_issue_asks_for():
    for n in cases.SIZES:
        q, qd, tgt = cases.state(n)
        assert q.shape == qd.shape == (n, 6) and tgt.shape == (n, 3) and q.dtype == np.float32
        bp = cases.body_positions(n)
        own = cases.shared_positions(n)
        assert bp.shape == (n, 3, 3) and np.array_equal(bp[:, 2], own[:, 2])                   # the plane stays
        assert (np.abs(bp[:, 0:2] - own[:, 0:2]).max(axis=2) > 0.05).all()                       # the box and the sphere move
        for w in (cases.sphere_view(n), cases.sphere_touch(n)):
            assert w.shape == (n, 8) and w.dtype == np.float32
            assert (w[:, 6] > 0).sum() == n - 1 and w[cases.NO_SPHERE[n], 6] == 0.0             # one env without a sphere
            assert len(np.unique(w[:, 7])) == n                                                  # radii per env
    assert 3 % 64 != 0 and 67 > 64


@pytest.mark.parametrize("size", cases.IMAGE_SIZES)
@pytest.mark.parametrize("n", cases.SIZES)
def test_every_sphere_is_in_view(n, size):
    shares = []
    for k, want in enumerate(cases.render_reference(n, size)):
        ok = ~want["band"]
        seen = int((ok & (want["seg"] == sref.SEG_MOVING_BODY)).sum())
        shares.append(ok.mean())
        if k == cases.NO_SPHERE[n]:
            assert not (want["seg"] == sref.SEG_MOVING_BODY).any()
        else:
            assert seen >= 20, (n, size, k, seen)
    print(f"n={n} {size}: share of pixels outside the band, smallest over the envs: {min(shares):.4f}")
    assert min(shares) >= 0.9


@pytest.mark.parametrize("which", ["world", "pointer"])
@pytest.mark.parametrize("n", cases.SIZES)
def test_every_sphere_is_hit_by_its_rays(n, which):
    shares = []
    for k, (want, _) in enumerate(cases.ray_reference(n, which)):
        ok = ~want["band"]
        shares.append(ok.mean())
        hit = (ok & (want["label"] == sref.SEG_MOVING_BODY)).mean()
        if k == cases.NO_SPHERE[n]:
            assert not (want["label"] == sref.SEG_MOVING_BODY).any()
        else:
            assert hit >= 0.10, (n, which, k, hit)
    print(f"n={n} {which}: share of rays outside the band, smallest over the envs: {min(shares):.4f}")
    assert min(shares) >= 0.9


@pytest.mark.parametrize("n", cases.SIZES)
def test_the_contact_cases_touch_the_sphere_and_the_damping_matters(n):
    r, still = cases.contact_reference(n), cases.contact_reference(n, moving=False)
    nearest = r["points"][:, :, 7] == sref.BODY_MOVING
    pushed = (r["sphere_force"] > 0).any(axis=1)
    none = cases.NO_SPHERE[n]
    ex = cq.exclusions(r)
    differ = np.abs(r["sphere_force"] - still["sphere_force"]).max()
    print(f"n={n}: the sphere is the nearest body of {nearest.mean():.3f} of the pairs, pushes {pushed.sum()} of {n} envs; its force "
          f"up to {r['sphere_force'].max():.1f}, differs from the zero-velocity force by up to {differ:.1f}; compared pairs "
          f"{(~ex['geometry']).mean():.4f} / {(~ex['force']).mean():.4f}")
    assert not nearest[none].any() and not pushed[none] and np.isinf(r["sphere_dist"][none]).all()
    assert nearest.mean() >= 0.2 and pushed.sum() >= max(1, n // 4)
    assert differ > 10.0                                               # kd 50 x a relative velocity of a few units/s
    assert (~ex["geometry"]).mean() >= 0.97 and (~ex["force"]).mean() >= 0.97
    # without caller's bodies an env with a sphere reports the sphere, an env without one nothing
    alone = cases.contact_reference(n, with_bodies=False)
    assert (alone["points"][np.arange(n) != none, :, 7] == sref.BODY_MOVING).all()
    assert np.isinf(alone["points"][none, :, 0]).all() and (alone["points"][none, :, 7] == -1).all()
