"""GPU tests of the scene queries' per-env world: pnr_render_bodies (body_positions in render_frames) and pnr_set_body_queries
(the moving sphere in render_frames, ray_test and contacts), against the float64 references composed by tests/scene_query_ref.py
on the inputs of tests/scene_query_cases.py (tests/test_scene_query_cpu.py asserts that the references show the sphere).

Criteria.  Render: tests/test_gpu_render.py's check_env (labels equal outside the reference's ambiguity band, rgb within 1, depth
within 1e-4 relative).  Rays: tests/test_gpu_ray_test.py's compare (its POS_TOL_REL, NORMAL_TOL).  Contacts: the bars of
tests/test_gpu_contact_query.py (FLOOR_MARGIN x the float32 floors of tests/contact_query_cases.py, inside its hard bars), leaving
out what contact_query_ref.exclusions names, the moving sphere counted as one more body there.  The step twin: Q_TOL / QD_TOL
(tests/bars.py).  Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import contact_query_cases as cq_cases
import contact_query_ref as cq
import scene_query_cases as cases
import scene_query_ref as sref
from bars import Q_TOL, QD_TOL
from gpu_support import dev, dyn_env, f64, kin_env, lib as _lib, load_joints
from test_gpu_ray_test import compare, world_length

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
SOURCES = ("buffer", "dynamic_own", "kinematic_own")


def source(kind, n, words=None):
    """(env, joint_state argument) of a joint source that holds the cases' q | qd and targets; a dynamics-mode env carries the
    spheres `words` [n, 8] (no query sees them until set_body_queries); a kinematic-mode env can have none"""
    q, qd, tgt = cases.state(n)
    if kind == "kinematic_own":
        env = kin_env(n, 3, reset=False, auto_reset=False, max_episode_steps=0)
        env.reset(joint_positions=q, target_positions=tgt)           # r = q (and v = 0)
        return env, None
    env = dyn_env(n, 3, 0.0, frame_skip=1, reset=False)
    env.reset(joint_positions=q, target_positions=tgt)
    if words is not None:
        env.set_body()
        env.set_body_state(dev(words))
    if kind == "buffer":
        return env, dev(np.concatenate([q, qd], axis=1))
    load_joints(env, q, qd)
    return env, None


def frames(env, cfg, js=None, **kw):
    fr = env.render_frames(cfg, joint_state=js, bodies=cases.bodies(), rgb=True, depth=True, segmentation=True, **kw)
    return {k: v.cpu().numpy() for k, v in fr.items()}


def check_pixels(fr, k, want, what):
    """tests/test_gpu_render.py check_env's criteria for env k against a reference computed elsewhere"""
    seg, rgb, dep = fr["seg"][k].reshape(-1), fr["rgb"][k].reshape(-1, 3).astype(np.int32), fr["depth"][k].reshape(-1).astype(np.float64)
    ok = ~want["band"]
    assert ok.mean() >= 0.9, (what, ok.mean())
    bad = ok & (seg != want["seg"])
    assert not bad.any(), f"{what}: {bad.sum()} labels differ outside the band, e.g. pixels {np.argwhere(bad)[:5].ravel()}: {seg[bad][:5]} vs {want['seg'][bad][:5]}"
    same = ok & (seg == want["seg"])
    assert np.abs(rgb[same] - want["rgb"][same].astype(np.int32)).max(initial=0) <= 1, what
    fin = same & np.isfinite(want["depth"])
    assert np.array_equal(np.isinf(dep[same]), np.isinf(want["depth"][same])), what
    assert (np.abs(dep[fin] - want["depth"][fin]) <= 1e-4 * want["depth"][fin]).all(), what
    return ok


# ---- 1. render ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SOURCES)
@pytest.mark.parametrize("size", cases.IMAGE_SIZES)
@pytest.mark.parametrize("n", cases.SIZES)
def test_render_against_the_composed_reference(n, size, kind):
    from pioneer_amd import render
    cfg = cases.render_config(size)
    words = cases.sphere_view(n)
    env, js = source(kind, n, words)
    bp = dev(cases.body_positions(n))
    none = cases.NO_SPHERE[n]
    if kind == "kinematic_own":                                       # no sphere in kinematic mode: the per-env bodies alone
        fr = frames(env, cfg, js, body_positions=bp)
        q, _, tgt = cases.state(n)
        view = render.view_matrix(cfg)
        for k in sorted({0, none, n - 1}):
            want = sref.render_env(q[k], tgt[k], cfg, view, cases.bodies(), cases.body_positions(n)[k], None)
            check_pixels(fr, k, want, f"{kind} n={n} {size} env {k}")
        assert not (fr["seg"] == sref.SEG_MOVING_BODY).any()
    else:
        env.set_body_queries(render=True)
        keep = None if js is None else js.clone()
        fr = frames(env, cfg, js, body_positions=bp)
        assert js is None or torch.equal(js, keep)
        seen = 0
        for k, want in enumerate(cases.render_reference(n, size)):
            ok = check_pixels(fr, k, want, f"{kind} n={n} {size} env {k}")
            seen += int((ok & (fr["seg"][k].reshape(-1) == sref.SEG_MOVING_BODY)).sum())
            if k == none:                                             # mass 0: no label 21 outside the band
                assert not (ok & (fr["seg"][k].reshape(-1) == sref.SEG_MOVING_BODY)).any()
        print(f"{kind} n={n} {size}: {seen} pixels show the moving sphere outside the band")
        assert seen >= 20 * (n - 1)
    env.close()


def test_render_without_positions_and_with_the_bit_clear_is_pnr_render():
    n, size = 67, cases.IMAGE_SIZES[0]
    cfg = cases.render_config(size)
    env, js = source("buffer", n, cases.sphere_view(n))
    plain = env.render_frames(cfg, joint_state=js, bodies=cases.bodies(), rgb=True, depth=True, segmentation=True)   # pnr_render
    # pnr_render_bodies with body_positions == NULL, bit clear, raw
    L = _lib()
    out = {"rgb": torch.zeros_like(plain["rgb"]), "depth": torch.zeros_like(plain["depth"]), "seg": torch.zeros_like(plain["seg"])}
    p = _render_params(env, cfg)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert env.lib.pnr_render_bodies(env._h, P(js), p, None, P(out["rgb"]), P(out["depth"]), P(out["seg"]), env._stream()) == 0
    torch.cuda.synchronize()
    for key in out:
        assert torch.equal(out[key], plain[key]), key
    # body_positions equal to the shared positions: the same labels outside the band (the records are built on the device)
    same = frames(env, cfg, js, body_positions=dev(cases.shared_positions(n)))
    from pioneer_amd import render
    q, _, tgt = cases.state(n)
    view = render.view_matrix(cfg)
    plain_np = {k: v.cpu().numpy() for k, v in plain.items()}
    for k in (0, 33, n - 1):
        want = sref.render_env(q[k], tgt[k], cfg, view, cases.bodies(), None, None)
        ok = check_pixels(same, k, want, f"shared positions env {k}")
        assert np.array_equal(same["seg"][k].reshape(-1)[ok], plain_np["seg"][k].reshape(-1)[ok])
    # the bit set and cleared again: pnr_render's bytes again
    env.set_body_queries(render=True)
    assert (env.render_frames(cfg, joint_state=js, bodies=cases.bodies(), segmentation=True)["seg"] == sref.SEG_MOVING_BODY).any()
    env.set_body_queries()
    again = env.render_frames(cfg, joint_state=js, bodies=cases.bodies(), rgb=True, depth=True, segmentation=True)
    for key in again:
        assert torch.equal(again[key], plain[key]), key
    assert L.SEG_MOVING_BODY == sref.SEG_MOVING_BODY
    env.close()


def _render_params(env, cfg, bodies=None):
    """a filled pnr_render_params, as render_frames builds it"""
    from pioneer_amd import render
    from pioneer_amd.config import fill_scene_body
    L = _lib()
    p = L.PnrRenderParams()
    p.struct_size = C.sizeof(L.PnrRenderParams)
    bodies = cases.bodies() if bodies is None else bodies
    p.width, p.height, p.n_bodies = cfg.render_width, cfg.render_height, len(bodies)
    for k, v in enumerate(np.asarray(render.view_matrix(cfg), dtype=np.float64).reshape(-1)):
        p.view[k] = float(v)
    p.fov_y, p.near_clip, p.far_clip = cfg.projection_fov, cfg.projection_near, cfg.projection_far
    p.light_direction[:] = (0.4, 0.2, 1.0)
    p.ambient, p.diffuse = 0.45, 0.55
    p.background[:] = (1.0, 1.0, 1.0)
    p.target_rgba[:] = env.config.target_rgba
    for i, (b, rgba) in enumerate(bodies):
        fill_scene_body(p.bodies[i], b, f"body {i}")
        p.body_rgba[i][:] = rgba
    return p


def test_the_sphere_is_drawn_in_the_colour_given():
    n, size = 3, cases.IMAGE_SIZES[0]
    cfg = cases.render_config(size)
    from pioneer_amd import render
    env, js = source("dynamic_own", n, cases.sphere_view(n))
    rgba = (0.9, 0.1, 0.2, 1.0)
    env.set_body_queries(render=True, rgba=rgba)
    env.set_body_queries(render=True)                                 # rgba None keeps the colour
    fr = frames(env, cfg, js, body_positions=dev(cases.body_positions(n)))
    q, _, tgt = cases.state(n)
    want = sref.render_env(q[0], tgt[0], cfg, render.view_matrix(cfg), cases.bodies(), cases.body_positions(n)[0], cases.sphere_view(n)[0], rgba)
    ok = check_pixels(fr, 0, want, "coloured sphere")
    assert (ok & (want["seg"] == sref.SEG_MOVING_BODY)).sum() >= 20
    env.close()


# ---- 2. rays --------------------------------------------------------------------------------------------------------------------------
def cast(env, rays, which, js=None, **kw):
    m = cases.RAY_MASKS[which]
    return env.ray_test(dev(rays), parent_link=-1 if which == "world" else cases.POINTER, hit_bodies=bool(m & 1), hit_arm=bool(m & 2),
                        hit_target=bool(m & 4), bodies=[b for b, _ in cases.bodies()], joint_state=js, **kw)


@pytest.mark.parametrize("kind", ["buffer", "dynamic_own"])
@pytest.mark.parametrize("which", ["world", "pointer"])
@pytest.mark.parametrize("n", cases.SIZES)
def test_rays_against_the_composed_reference(n, which, kind):
    env, js = source(kind, n, cases.sphere_view(n))
    env.set_body_queries(rays=True)
    rays = cases.world_rays(n) if which == "world" else cases.pointer_rays(n)
    res = cast(env, rays, which, js, body_positions=dev(cases.body_positions(n)), fractions=True)
    hits = res["hits"].cpu().numpy()
    assert hits[..., 0].tobytes() == res["fractions"].cpu().numpy().tobytes()
    seen = 0
    for k, (want, tr) in enumerate(cases.ray_reference(n, which)):
        compare(hits[k], want, world_length(tr), what=f"{kind} n={n} {which} env {k}")
        seen += int((~want["band"] & (hits[k, :, 7] == sref.SEG_MOVING_BODY)).sum())
    none = cases.NO_SPHERE[n]
    assert not (hits[none, :, 7] == sref.SEG_MOVING_BODY).any()
    print(f"{kind} n={n} {which}: {seen} of {hits.shape[0] * hits.shape[1]} rays hit the moving sphere outside the band")
    assert seen >= 0.1 * rays.shape[1] * (n - 1)
    # without the bodies bit in the mask the sphere is not a solid
    arm_only = env.ray_test(dev(rays), parent_link=-1 if which == "world" else cases.POINTER, hit_bodies=False, hit_arm=True,
                            bodies=[b for b, _ in cases.bodies()], joint_state=js)["hits"]
    assert not bool((arm_only[..., 7] >= 13).any())
    env.close()


def test_a_ray_that_starts_inside_the_sphere_does_not_hit_it():
    n = 3
    w = cases.sphere_view(n)
    env, js = source("buffer", n, w)
    env.set_body_queries(rays=True)
    c, r = w[:, 0:3].astype(np.float64), w[:, 7:8].astype(np.float64)
    axis = np.array([0.0, 0.0, 1.0])
    inside = np.concatenate([c + 0.5 * r * axis, c + 3.0 * r * axis], axis=1)            # from inside, out through the top
    outside = np.concatenate([c + 3.0 * r * axis, c + 0.5 * r * axis], axis=1)           # the same segment, from outside in
    rays = np.stack([inside, outside], axis=1).astype(np.float32)                        # [n, 2, 6]
    hits = env.ray_test(dev(rays), bodies=[], joint_state=js)["hits"].cpu().numpy()
    none = cases.NO_SPHERE[n]
    for k in range(n):
        print(f"env {k}: from inside label {hits[k, 0, 7]:.0f} fraction {hits[k, 0, 0]:.4f}; from outside label {hits[k, 1, 7]:.0f} fraction {hits[k, 1, 0]:.4f}")
        assert hits[k, 0, 7] == 0 and hits[k, 0, 0] == 1.0
        if k == none:
            assert hits[k, 1, 7] == 0
        else:
            assert hits[k, 1, 7] == sref.SEG_MOVING_BODY and abs(hits[k, 1, 0] - 0.8) <= 1e-5   # enters at 2 r of the 2.5 r
            assert np.abs(hits[k, 1, 4:7] - axis).max() <= 1e-4
    env.close()


def test_rays_and_pixels_agree_on_the_moving_sphere():
    """tests/test_gpu_ray_test.py::test_agreement_with_render with the sphere: one ray per pixel from the near to the far plane"""
    import ray_ref as ry
    import render_ref as rr
    from pioneer_amd import render
    n, size = 3, cases.IMAGE_SIZES[1]
    cfg = cases.render_config(size)
    W, H = size
    near, far = cfg.projection_near, cfg.projection_far
    env, js = source("buffer", n, cases.sphere_view(n))
    env.set_body_queries(render=True, rays=True)
    yy, xx = np.mgrid[0:H, 0:W]
    view = render.view_matrix(cfg)
    eye, d = rr.rays(view, cfg.projection_fov, W, H, xx.ravel(), yy.ravel())
    rays = np.concatenate([eye[None] + near * d, eye[None] + far * d], axis=1).astype(np.float32)
    bp = dev(cases.body_positions(n))
    fr = frames(env, cfg, js, body_positions=bp)
    hits = env.ray_test(dev(rays), hit_arm=True, hit_target=True, bodies=[b for b, _ in cases.bodies()], body_positions=bp,
                        joint_state=js)["hits"].cpu().numpy()
    q, _, tgt = cases.state(n)
    agreed = 0
    for k in range(n):
        a, _ = sref.rays_env(q[k], tgt[k], rays, ry.HIT_ARM | ry.HIT_BODIES | ry.HIT_TARGET, cases.bodies(), cases.body_positions(n)[k], cases.sphere_view(n)[k])
        b = cases.render_reference(n, size)[k]
        ok = ~a["band"] & ~b["band"]
        assert ok.mean() >= 0.9
        assert np.array_equal(a["label"][ok], b["seg"][ok].astype(np.int64))             # the two references agree on these pixels
        seg = fr["seg"][k].reshape(-1)
        assert np.array_equal(hits[k, ok, 7].astype(np.int64), seg[ok].astype(np.int64)), k
        agreed += int((ok & (seg == sref.SEG_MOVING_BODY)).sum())
    print(f"rays and pixels agree on label 21 at {agreed} pixels")
    assert agreed >= 20 * (n - 1)
    env.close()


# ---- 3. contacts ----------------------------------------------------------------------------------------------------------------------
def scene_bodies():
    return [b for b, _ in cases.bodies()]


def check_contacts(res, r, what):
    """tests/test_gpu_contact_query.py check_against_reference's figures and bars against the reference dict r"""
    ex = cq.exclusions(r)
    geo, frc = ~ex["geometry"], ~ex["force"]
    pts, want = f64(res["points"]), r["points"]
    fin = np.isfinite(want[..., 0])                                  # (an env without a body reports +inf, compared as such)
    assert np.array_equal(np.isinf(pts[..., 0]), ~fin)
    def err(sl, mask):
        with np.errstate(invalid="ignore"):                           # (inf - inf where there is no body: not compared)
            return float(np.abs(pts[..., sl] - want[..., sl])[mask & fin].max(initial=0.0))

    e_dist, e_nrm, e_pos, e_force = err(slice(0, 1), geo), err(slice(1, 4), geo), err(slice(4, 7), geo), err(slice(8, 9), frc)
    body_ok = bool(np.array_equal(pts[..., 7][geo], want[..., 7][geo]))
    sm, swant = f64(res["summary"]), r["summary"]
    env_geo = geo.all(axis=1)
    sfin = np.isfinite(swant[:, 0])
    e_sdist = float(np.abs(sm[sfin, 0] - swant[sfin, 0]).max(initial=0.0))
    idx_ok = bool(np.array_equal(cq.merge_twins(sm[env_geo, 1]), cq.merge_twins(swant[env_geo, 1])) and np.array_equal(sm[env_geo, 2], swant[env_geo, 2]))
    count_env = (np.abs(want[..., 0]) >= 1e-4).all(axis=1)
    count_ok = bool(np.array_equal(sm[count_env, 3], swant[count_env, 3]))
    env_frc = frc.all(axis=1)
    e_tau = float(np.abs(f64(res["joint_torques"]) - r["torques"])[env_frc].max(initial=0.0))
    m = cq_cases.FLOOR_MARGIN
    print(f"{what}: distance {e_dist:.2e} (tight {m * cq_cases.DIST_FLOOR:.1e}) normal {e_nrm:.2e} ({m * cq_cases.NORMAL_FLOOR:.1e}) position {e_pos:.2e} "
          f"({m * cq_cases.POS_FLOOR:.1e}) force {e_force:.2e} ({m * cq_cases.FORCE_FLOOR:.1e}) torque {e_tau:.2e} ({m * cq_cases.TORQUE_FLOOR:.1e}) "
          f"summary distance {e_sdist:.2e} | the sphere is nearest for {(want[..., 7] == sref.BODY_MOVING).mean():.3f} of the pairs | compared "
          f"{geo.mean():.4f} / {frc.mean():.4f}, envs {env_frc.mean():.3f}")
    assert body_ok and idx_ok and count_ok
    assert e_dist <= m * cq_cases.DIST_FLOOR <= cq_cases.DIST_HARD and e_sdist <= m * cq_cases.DIST_FLOOR
    assert e_pos <= m * cq_cases.POS_FLOOR <= cq_cases.DIST_HARD
    assert e_nrm <= m * cq_cases.NORMAL_FLOOR <= cq_cases.NORMAL_HARD
    assert e_force <= m * cq_cases.FORCE_FLOOR <= cq_cases.FORCE_HARD
    assert e_tau <= m * cq_cases.TORQUE_FLOOR <= cq_cases.TORQUE_HARD


@pytest.mark.parametrize("kind", ["buffer", "dynamic_own"])
@pytest.mark.parametrize("n", cases.SIZES)
def test_contacts_against_the_composed_reference(n, kind):
    env, js = source(kind, n, cases.sphere_touch(n))
    env.set_body_queries(contacts=True)
    res = env.contacts(joint_state=js, bodies=scene_bodies(), body_positions=dev(cases.body_positions(n)), joint_torques=True)
    torch.cuda.synchronize()
    check_contacts(res, cases.contact_reference(n), f"{kind} n={n} three bodies")
    # no caller's bodies: an env with a sphere reports the sphere, the env without one what it always reported
    res = env.contacts(joint_state=js, bodies=[], joint_torques=True)
    check_contacts(res, cases.contact_reference(n, with_bodies=False), f"{kind} n={n} the sphere alone")
    none = cases.NO_SPHERE[n]
    pts = res["points"]
    assert bool((pts[none, :, 7] == -1).all()) and bool(torch.isinf(pts[none, :, 0]).all()) and bool((res["joint_torques"][none] == 0).all())
    assert bool((pts[torch.as_tensor(np.arange(n) != none, device=pts.device)][:, :, 7] == sref.BODY_MOVING).all())
    env.close()


def test_the_force_differs_from_the_zero_velocity_workaround():
    """what scene.py's docstring used to point to: contacts(bodies=[scene_sphere(r)], body_positions=centres) has one radius for
    all envs and no velocity in the law"""
    from pioneer_amd.config import scene_sphere
    n = 67
    w = cases.sphere_touch(n).copy()
    w[:, 7] = 3.0                                                     # one radius, so that the workaround can express the geometry
    w[:, 6] = 1.0                                                     # .. and a sphere in every env
    env, js = source("buffer", n, w)
    env.set_body_queries(contacts=True)
    new = env.contacts(joint_state=js, bodies=[])["points"].cpu().numpy()
    env.set_body_queries()
    old = env.contacts(joint_state=js, bodies=[scene_sphere(3.0, (0.0, 0.0, 0.0))], body_positions=dev(w[:, None, 0:3].copy()))["points"].cpu().numpy()
    touching = new[..., 0] < -1e-3
    dforce = np.abs(new[..., 8] - old[..., 8])[touching]
    print(f"{touching.sum()} touching pairs: distance differs by up to {np.abs(new[..., 0] - old[..., 0]).max():.2e}, the force by up to {dforce.max():.1f}")
    assert touching.sum() >= 20 and np.abs(new[..., 0] - old[..., 0]).max() <= 1e-4    # the same geometry ..
    assert dforce.max() > 10.0                                                          # .. another force: kd x the sphere's velocity
    env.close()


def test_world_step_equals_a_sphere_less_twin_driven_by_the_query():
    """Independent of the reference: a dynamics handle (frame_skip 1, no gravity, no static bodies, link_contacts so that step and
    query both see all 23 samples) whose sphere touches the arm, against a twin without a sphere that takes
    contacts(joint_torques=True) of the first as its joint torques."""
    L = _lib()
    n = 67
    q, qd, _ = cases.state(n)
    q = (0.7 * q).astype(np.float32)                                  # off the limits: the integrator's clamp is no force
    centres = cq.query(q, qd, ())["centres"]
    rng = np.random.default_rng(77)
    radius = rng.uniform(1.0, 2.0, size=n)
    pick = rng.integers(0, cq.SAMPLES, size=n)
    sample_r = np.array([cases.POINTER_RADIUS if r < 0 else r for _, _, r in cq.sample_table()])
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    depth = rng.uniform(0.01, 0.2, size=n)                           # shallow: forces of the order of the arm's weight
    x = centres[np.arange(n), pick] + (radius + sample_r[pick] - depth)[:, None] * d
    w = np.concatenate([x, rng.uniform(-2.0, 2.0, size=(n, 3)), np.full((n, 1), 2.0), radius[:, None]], axis=1).astype(np.float32)
    w[5, 6] = 0.0                                                     # one env without a sphere
    P, Q, Q0 = (dyn_env(n, 5, 0.0, frame_skip=1, randomize=True, link_contacts=True) for _ in range(3))
    state = P.get_dyn_state()
    state[0:6], state[6:12] = dev(q.T), dev(qd.T)
    for env in (P, Q, Q0):
        env.set_dyn_state(state.clone())
        for j in range(6):                                            # zero gains: no motor torque at all
            env.set_joint_motor(j, L.CONTROL_VELOCITY, target_velocity=0.0, velocity_gain=0.0, max_force=0.0)
    P.set_body()
    P.set_body_state(dev(w))
    P.set_body_queries(contacts=True)
    got = P.contacts(bodies=[], joint_torques=True)
    tau = got["joint_torques"]
    touching = int((got["summary"][:, 3] > 0).sum())
    P.world_step()
    Q.world_step(joint_torques=tau)
    Q0.world_step()
    torch.cuda.synchronize()
    p, qq, q0 = (f64(e.get_dyn_state()) for e in (P, Q, Q0))
    eq, eqd = np.abs(p[0:6] - qq[0:6]).max(), np.abs(p[6:12] - qq[6:12]).max()
    without = np.abs(p[6:12] - q0[6:12]).max()
    print(f"{touching} of {n} envs touch their sphere; |tau| up to {float(tau.abs().max()):.1f}; with the sphere against the twin: |dq| {eq:.2e} "
          f"(bar {Q_TOL:.0e}) |dqd| {eqd:.2e} (bar {QD_TOL:.0e}); without the torques |dqd| {without:.2e}")
    assert touching >= n // 2 and bool((tau[5] == 0).all())
    assert without > 10 * QD_TOL
    assert eq <= Q_TOL and eqd <= QD_TOL
    for env in (P, Q, Q0):
        env.close()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing():
    n, size = 3, cases.IMAGE_SIZES[1]
    cfg = cases.render_config(size)
    W, H = size
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    rgba = (C.c_float * 4)(0.1, 0.2, 0.3, 1.0)
    # a kinematic-mode handle
    kin, _ = source("kinematic_own", n)
    assert kin.lib.pnr_set_body_queries(kin._h, 1, None) == UNSUPPORTED and b"dynamics mode" in kin.lib.pnr_last_error(kin._h)
    with pytest.raises(Exception):
        kin.set_body_queries(render=True)
    kin.close()
    # before the first pnr_set_body_params: no buffer
    env, js = source("buffer", n)
    lib, h = env.lib, env._h
    assert lib.pnr_set_body_queries(h, 7, rgba) == INVALID and b"before pnr_set_body_params" in lib.pnr_last_error(h)
    env.set_body()
    env.set_body_state(dev(cases.sphere_view(n)))
    for bits in (8, 15, 0x80000001):                                  # unknown bits
        assert lib.pnr_set_body_queries(h, bits, rgba) == INVALID and b"unknown bits" in lib.pnr_last_error(h)
    for bad in ((float("nan"), 0, 0, 1), (0, float("inf"), 0, 1), (0, 0, 0, float("nan"))):
        assert lib.pnr_set_body_queries(h, 1, (C.c_float * 4)(*bad)) == INVALID and b"non-finite colour" in lib.pnr_last_error(h)
    assert b"PNR_" not in lib.pnr_last_error(h)
    assert lib.pnr_set_body_queries(None, 1, None) == INVALID
    # every refused call left the switch at 0: the three queries are what they were
    before = frames(env, cfg, js)
    assert not (before["seg"] == sref.SEG_MOVING_BODY).any()
    assert not bool((env.ray_test(dev(cases.world_rays(n)), bodies=[], joint_state=js)["hits"][..., 7] == sref.SEG_MOVING_BODY).any())
    assert bool((env.contacts(joint_state=js, bodies=[])["points"][..., 7] == -1).all())
    # pnr_render_bodies: pnr_render's refusals and the alignment of body_positions, no output touched
    m = n * W * H
    rgb = torch.full((3 * m + 64,), 7, dtype=torch.uint8, device="cuda:0")
    dep = torch.full((m + 16,), 3.0, dtype=torch.float32, device="cuda:0")
    seg = torch.full((m + 16,), 9, dtype=torch.uint8, device="cuda:0")
    bp = torch.zeros(n * 3 * 3 * 4 + 8, dtype=torch.uint8, device="cuda:0")
    p = _render_params(env, cfg)
    st = env._stream()
    assert lib.pnr_render_bodies(h, P(js), p, P(bp, 2), P(rgb), P(dep), P(seg), st) == INVALID and b"4-byte aligned" in lib.pnr_last_error(h)
    assert lib.pnr_render_bodies(h, P(js), None, P(bp), P(rgb), P(dep), P(seg), st) == INVALID
    assert lib.pnr_render_bodies(h, P(js), p, P(bp), None, None, None, st) == INVALID
    assert lib.pnr_render_bodies(h, P(js), p, P(bp), P(rgb, 1), P(dep), P(seg), st) == INVALID
    bad = _render_params(env, cfg); bad.n_bodies = 9
    assert lib.pnr_render_bodies(h, P(js), bad, P(bp), P(rgb), P(dep), P(seg), st) == INVALID
    bad = _render_params(env, cfg); bad.width = 0
    assert lib.pnr_render_bodies(h, P(js), bad, P(bp), P(rgb), P(dep), P(seg), st) == INVALID
    fresh = dyn_env(n, 4, 0.0, frame_skip=1, reset=False)
    assert fresh.lib.pnr_render_bodies(fresh._h, P(js), p, P(bp), P(rgb), P(dep), P(seg), st) == INVALID
    assert b"before the first pnr_reset" in fresh.lib.pnr_last_error(fresh._h)
    fresh.close()
    torch.cuda.synchronize()
    assert (rgb == 7).all() and (dep == 3.0).all() and (seg == 9).all()
    # the ray mask keeps its three bits with the sphere shown
    env.set_body_queries(rays=True)
    from test_gpu_ray_test import _params, _raw
    hits = torch.full((n * 8 + 16,), -7.25, dtype=torch.float32, device="cuda:0")
    for mask in (8, 15):
        assert _raw(env, _params(env, 1, mask=mask), dev(cases.world_rays(n)[0, :1]), hits, None, js=js) == INVALID
    torch.cuda.synchronize()
    assert (hits == -7.25).all()
    # the unrefused call runs and stops at its last byte
    assert lib.pnr_render_bodies(h, P(js), p, P(bp), P(rgb), P(dep), P(seg), st) == 0
    torch.cuda.synchronize()
    assert (rgb[3 * m:] == 7).all() and (dep[m:] == 3.0).all() and (seg[m:] == 9).all() and not (seg[:m] == 9).all()
    env.close()


# ---- 5. untouched calls ------------------------------------------------------------------------------------------------------------------
def test_with_all_bits_clear_a_handle_with_a_sphere_answers_as_one_without():
    n, size = 67, cases.IMAGE_SIZES[0]
    cfg = cases.render_config(size)
    with_sphere, _ = source("dynamic_own", n, cases.sphere_touch(n))
    without, _ = source("dynamic_own", n)
    bp = dev(cases.body_positions(n))
    rays = dev(cases.pointer_rays(n))
    outs = []
    for env in (with_sphere, without):
        fr = env.render_frames(cfg, bodies=cases.bodies(), rgb=True, depth=True, segmentation=True)
        hits = env.ray_test(rays, parent_link=cases.POINTER, hit_arm=True, hit_target=True, bodies=scene_bodies(), body_positions=bp, fractions=True)
        con = env.contacts(bodies=scene_bodies(), body_positions=bp, joint_torques=True)
        outs.append({**fr, **hits, **con})
    torch.cuda.synchronize()
    for key in outs[0]:
        assert torch.equal(outs[0][key], outs[1][key]), key
    # .. and a bit concerns its own query alone
    with_sphere.set_body_queries(rays=True)
    con = with_sphere.contacts(bodies=scene_bodies(), body_positions=bp, joint_torques=True)
    fr = with_sphere.render_frames(cfg, bodies=cases.bodies(), rgb=True, depth=True, segmentation=True)
    for key in (*con, *fr):
        assert torch.equal({**con, **fr}[key], outs[1][key]), key
    with_sphere.close(); without.close()


# ---- 6. the facade -----------------------------------------------------------------------------------------------------------------------
def test_facade_sees_its_moving_sphere():
    from pioneer_amd import EngineConfig, PioneerKinematicEnv
    env = PioneerKinematicEnv(device="cuda:0", engine_config=EngineConfig(mode="dynamic", renderer="engine"))
    q0 = np.array([0.3, 0.4, -0.2, 0.1, 0.5, 0.0])
    env.reset_world(q0, (18.0, 2.0, 4.0))
    env.scene.create_body_box("crate", True, 0, (1.0, 1.0, 1.0), (-20.0, -20.0, 0.0), (0, 0, 0, 1))
    import link_kinematics_ref as lk
    pose = env.scene.links_by_name["robot:pointer"].pose()
    tip, axis = np.array(pose.position), lk.matrix_from_quat(pose.orientation)[:, 2]     # the needle's direction: nothing of the arm beyond
    centre = tip + (1.0 + 0.2 - 0.05) * axis                          # resting against the pointer's tip, 0.05 deep
    env.scene.create_body_sphere("ball", True, 2.0, 1.0, tuple(centre), (0, 0, 0, 1))
    ball = env.scene.items_by_name["ball"]
    assert env.scene.body_id(ball) == 2 and env.scene.body_id(env.scene.items_by_name["crate"]) == 1
    cps = env.scene.contact_points()
    print([(c.linkIndexA, c.bodyUniqueIdB, round(c.contactDistance, 4), round(c.normalForce, 1)) for c in cps])
    mine = [c for c in cps if c.bodyUniqueIdB == 2]
    assert mine and any(c.linkIndexA == 10 and abs(c.contactDistance + 0.05) <= 1e-4 for c in mine)
    assert env.scene.contact_points(item=ball) == mine and env.scene.contact_points(item=env.scene.items_by_name["crate"]) == []
    assert len(env.scene.closest_points(1e9)) == 23
    hit = env.scene.ray_test(tuple(centre + 10.0 * axis), tuple(centre - 0.5 * axis))     # from beyond the sphere, down the needle's axis
    assert hit[:2] == (2, -1) and hit.hitFraction == pytest.approx(9.0 / 10.5, abs=1e-5)
    assert hit.hitNormal == pytest.approx(tuple(axis), abs=1e-4)
    # render("rgb_array") draws the sphere once: as the static body it always was, not as the handle's sphere too
    frame = env.render("rgb_array")
    seg = env._vec.render_frames(env.render_config, bodies=env.scene.render_bodies(), rgb=False, segmentation=True)["seg"]
    assert frame.ndim == 3 and not bool((seg == sref.SEG_MOVING_BODY).any()) and bool((seg == 13 + 1).any())       # (the ball is the second created body)
    env.close()
