"""GPU tests of pnr_ray_test (PioneerVectorEnv.ray_test, Scene.ray_test / ray_test_batch): hits against the independent float64
reference of tests/ray_ref.py outside its ambiguity band, agreement with pnr_render, every joint source, parent links, ray
layouts, per-env body positions, batch independence and determinism, output bounds (a > 2^31-byte hits batch included),
validation, graph capture and the façade.

Tolerances.  Position (and with it the fraction, position error / length): the ceiling is 1e-4 x |to - from|, what the project
grants pnr_render's depth.  Measured on an MI355X over every comparison with the reference in this file (the 81 parity cases, the
joint sources, the moved box, the 65 537 x 1 024 batch, the graph replay), outside the band: worst position deviation
9.42e-7 x |to - from| (parity cases alone: 5.3e-7), more than 10x below the ceiling, so 4x the measured value is asserted
(POS_TOL_REL).  Normal: worst deviation from the reference 1.43e-5 (on the 0.2-radius spheres, position error / radius); 4x that
is asserted (NORMAL_TOL), far below the 1e-3 cap.  Where two engine answers are compared with each other, each lies within the
tolerance of the truth, so twice the tolerance is asserted (plus the float32 rounding of rays transformed on the host)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import link_kinematics_ref as lk
import ray_ref as ry
import render_ref as rr
from gpu_support import LIMITS, coloured_bodies, random_state

pytestmark = pytest.mark.gpu

POS_TOL_REL = 4 * 9.42e-7          # x |to - from|; see the module docstring
NORMAL_TOL = 4 * 1.43e-5
MASKS = {"bodies": ry.HIT_BODIES, "arm_bodies": ry.HIT_ARM | ry.HIT_BODIES, "all": ry.HIT_ARM | ry.HIT_BODIES | ry.HIT_TARGET}
POINTER = 10


def scene_bodies():
    """The render tests' three bodies, without their colours."""
    return [b for b, _ in coloured_bodies()]


def ref_bodies(bodies, positions=None):
    return [(b.shape, b.position if positions is None else positions[i], b.orientation, b.size) for i, b in enumerate(bodies)]


def fan(n=32):
    from pioneer_amd.scene import ray_fan
    return ray_fan(n, 40.0, start=0.25)


def ray_set(name, tgt):
    """(rays, parent_link): rays float32 [R0, 6] shared, or [N, R0, 6] per env (set C)."""
    if name == "A":                                                  # a fan on the pointer
        return fan(), POINTER
    if name == "B":                                                  # an 8 x 8 grid of world rays onto z = -1
        x, y = np.meshgrid(np.linspace(-22.0, 20.0, 8), np.linspace(-8.0, 14.0, 8))
        to = np.stack([x.ravel(), y.ravel(), np.full(64, -1.0)], axis=1)
        return np.concatenate([np.tile((30.0, -20.0, 25.0), (64, 1)), to], axis=1).astype(np.float32), -1
    frm = np.tile((0.0, 0.0, 30.0), (len(tgt), 1))                   # C: at the env's own target, 20 % beyond it
    return np.concatenate([frm, frm + 1.2 * (tgt.astype(np.float64) - frm)], axis=1).astype(np.float32)[:, None, :], -1


def cycled(rays, R):
    """The set's rays repeated to R rays per env."""
    return np.ascontiguousarray(np.take(rays, np.arange(R) % rays.shape[-2], axis=-2))


def checked_envs(n):
    return list(range(n)) if n <= 37 else sorted({0, n - 1, *np.random.default_rng(n).choice(n, 10, replace=False).tolist()})


def parity_state(n):
    return random_state(n, 300 + n)


@functools.lru_cache(maxsize=None)
def parity_traces(n, name):
    """The mask-independent part of the reference for the parity cases, once per (n, ray set): {env: trace}."""
    q, tgt = parity_state(n)
    rays, parent = ray_set(name, tgt)
    bodies = ref_bodies(scene_bodies())
    return {k: ry.trace(q[k], tgt[k], rays[k] if rays.ndim == 3 else rays, bodies, parent) for k in checked_envs(n)}


@functools.lru_cache(maxsize=None)
def parity_reference(n, name, mask):
    return {k: ry.resolve(tr, mask) for k, tr in parity_traces(n, name).items()}


def compare(got, want, rays_world_len, idx=None, what=""):
    """Engine rows got [R, 8] against the reference dict (its rows idx) outside the band; returns the worst deviations."""
    idx = np.arange(len(got)) if idx is None else idx
    ok = ~want["band"][idx]
    lab = got[:, 7].astype(np.int64)
    wl = want["label"][idx]
    bad = ok & (lab != wl)
    assert not bad.any(), f"{what}: {bad.sum()} labels differ outside the band, e.g. rays {np.argwhere(bad)[:5].ravel()}: {lab[bad][:5]} vs {wl[bad][:5]}"
    hit = ok & (wl != 0)
    miss = ok & (wl == 0)
    length = rays_world_len[idx]
    perr = np.linalg.norm(got[:, 1:4].astype(np.float64) - want["position"][idx], axis=1) / length
    nerr = np.linalg.norm(got[:, 4:7].astype(np.float64) - want["normal"][idx], axis=1)
    ferr = np.abs(got[:, 0].astype(np.float64) - want["fraction"][idx])
    worst = dict(pos=perr[ok].max(initial=0.0), nrm=nerr[hit].max(initial=0.0), frac=ferr[ok].max(initial=0.0))
    print(f"{what}: checked {ok.sum()} of {len(ok)} rays, worst position {worst['pos']:.3e} x length, normal {worst['nrm']:.3e}, "
          f"fraction {worst['frac']:.3e}")
    assert (perr[ok] <= POS_TOL_REL).all(), (what, worst)
    assert (ferr[ok] <= POS_TOL_REL).all(), (what, worst)
    assert (np.abs(np.linalg.norm(got[hit, 4:7].astype(np.float64), axis=1) - 1.0) <= 1e-5).all(), what
    assert (nerr[hit] <= NORMAL_TOL).all(), (what, worst)
    assert (got[miss, 0] == 1.0).all() and (got[miss, 4:7] == 0.0).all(), what
    return worst


def world_length(tr):
    return np.linalg.norm(tr["D"], axis=1)


def make_env(n, q, tgt, seed=1, **kw):
    from pioneer_amd import PioneerVectorEnv
    env = PioneerVectorEnv(n, device="cuda:0", seed=seed, **kw)
    env.reset(joint_positions=q, target_positions=tgt)
    return env


def cast(env, rays, parent, mask, **kw):
    return env.ray_test(torch.from_numpy(np.ascontiguousarray(rays)).cuda(), parent_link=parent, hit_bodies=bool(mask & 1), hit_arm=bool(mask & 2),
                        hit_target=bool(mask & 4), bodies=kw.pop("bodies", scene_bodies()), **kw)


@pytest.mark.parametrize("mask", sorted(MASKS))
@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("R", [1, 32, 67])
@pytest.mark.parametrize("n", [1, 37, 1000])
def test_parity_outside_the_band(n, R, name, mask):
    q, tgt = parity_state(n)
    env = make_env(n, q, tgt)
    rays, parent = ray_set(name, tgt)
    res = cast(env, cycled(rays, R), parent, MASKS[mask], hits=True, fractions=True)
    hits, frac = res["hits"].cpu().numpy(), res["fractions"].cpu().numpy()
    assert hits.shape == (n, R, 8) and frac.shape == (n, R)
    assert hits[..., 0].tobytes() == frac.tobytes()
    idx = np.arange(R) % rays.shape[-2]
    want, traces = parity_reference(n, name, MASKS[mask]), parity_traces(n, name)
    outside = np.concatenate([~want[k]["band"][idx] for k in want])
    assert outside.mean() >= 0.9, outside.mean()
    for k in want:
        compare(hits[k], want[k], world_length(traces[k]), idx, f"n={n} R={R} {name} {mask} env {k}")
    env.close()


def test_parity_cases_cover_the_arm_the_target_and_every_body():
    """What the parity cases saw outside the band (the labels asserted equal to the engine's there)."""
    seen = {name: set() for name in "ABC"}
    for n in (1, 37, 1000):
        for name in "ABC":
            for want in parity_reference(n, name, MASKS["all"]).values():
                seen[name] |= set(want["label"][~want["band"]].tolist())
    every = seen["A"] | seen["B"] | seen["C"]
    assert any(rr.SEG_LINK0 < s < rr.SEG_TARGET for s in every), every
    assert rr.SEG_TARGET in seen["C"], seen["C"]
    assert {rr.SEG_BODY0, rr.SEG_BODY0 + 1, rr.SEG_BODY0 + 2} <= every, every
    assert 0 in every                                                # and misses


def test_agreement_with_render():
    from pioneer_amd import RenderConfig, render
    n, W, H = 5, 24, 16
    cfg = RenderConfig(render_width=W, render_height=H, camera_distance=60.0)
    near, far = cfg.projection_near, cfg.projection_far
    q, tgt = random_state(n, 21)
    env = make_env(n, q, tgt)
    bodies = scene_bodies()
    yy, xx = np.mgrid[0:H, 0:W]
    view = render.view_matrix(cfg)
    eye, d = rr.rays(view, cfg.projection_fov, W, H, xx.ravel(), yy.ravel())
    rays = np.concatenate([eye[None] + near * d, eye[None] + far * d], axis=1).astype(np.float32)
    fr = env.render_frames(cfg, bodies=[(b, (0.5, 0.5, 0.5, 1.0)) for b in bodies], rgb=False, depth=True, segmentation=True)
    hits = cast(env, rays, -1, MASKS["all"])["hits"].cpu().numpy()
    seg, depth = fr["seg"].cpu().numpy().reshape(n, -1), fr["depth"].cpu().numpy().reshape(n, -1).astype(np.float64)
    length = np.linalg.norm(rays[:, 3:6].astype(np.float64) - rays[:, 0:3], axis=1)
    checked = 0
    for k in range(n):
        a = ry.ray_test(q[k], tgt[k], rays, MASKS["all"], ref_bodies(bodies))
        b = rr.render_pixels(q[k].astype(np.float64), tgt[k].astype(np.float64), xx.ravel(), yy.ravel(), view, cfg.projection_fov, near, far, W, H,
                             bodies=[(*body, (0.5, 0.5, 0.5, 1.0)) for body in ref_bodies(bodies)])
        ok = ~a["band"] & ~b["band"]
        assert np.array_equal(a["label"][ok], b["seg"][ok].astype(np.int64))          # the two references agree on these pixels
        assert ok.mean() >= 0.9
        assert np.array_equal(hits[k, ok, 7].astype(np.int64), seg[k, ok].astype(np.int64)), k
        miss = ok & (seg[k] == 0)
        assert np.isinf(depth[k, miss]).all() and (hits[k, miss, 0] == 1.0).all()
        hit = ok & (seg[k] != 0)
        along = near + hits[k, hit, 0].astype(np.float64) * (far - near)
        # each engine answer lies within its own tolerance of the truth: the renderer's 1e-4 relative depth, the ray's position
        print(f"render env {k}: {hit.sum()} hits, worst depth difference {(np.abs(along - depth[k, hit]) / depth[k, hit]).max():.3e} relative")
        assert (np.abs(along - depth[k, hit]) <= 1e-4 * depth[k, hit] + POS_TOL_REL * length[hit]).all(), k
        checked += int(hit.sum())
    assert checked > 100
    env.close()


def test_joint_sources():
    from pioneer_amd import EngineConfig
    n = 37
    q, tgt = random_state(n, 5)
    rng = np.random.default_rng(6)
    rays, parent = ray_set("A", tgt)
    bodies = ref_bodies(scene_bodies())
    for mode in ("kinematic", "dynamic"):
        env = make_env(n, q, tgt, seed=2, engine_config=EngineConfig(mode=mode))
        qb = (rng.uniform(-1.2, 1.2, size=(n, 6)) * LIMITS).astype(np.float32)       # a caller's buffer (q | qd), only read
        js = torch.from_numpy(np.concatenate([qb, rng.uniform(-3, 3, size=(n, 6)).astype(np.float32)], axis=1)).cuda()
        keep = js.clone()
        hits = cast(env, rays, parent, MASKS["all"], joint_state=js)["hits"].cpu().numpy()
        assert torch.equal(js, keep)
        for k in (0, 17, n - 1):
            tr = ry.trace(qb[k], tgt[k], rays, bodies, parent)
            compare(hits[k], ry.resolve(tr, MASKS["all"]), world_length(tr), what=f"{mode} buffer env {k}")
        if mode == "dynamic":                                        # the handle's own joints
            d = env.get_dyn_state()
            d[6:12] = torch.from_numpy(rng.uniform(-2, 2, size=(6, n)).astype(np.float32)).cuda()
            env.set_dyn_state(d)
            for _ in range(3):
                env.world_step()
            qs = env.get_dyn_state()[0:6].T.cpu().numpy()
            assert np.abs(qs - q).max() > 1e-3                                          # the simulated joints moved
        else:
            qs = env.get_state().view(torch.float32)[12:18].T.cpu().numpy()
        hits = cast(env, rays, parent, MASKS["all"])["hits"].cpu().numpy()
        for k in (0, 17, n - 1):
            tr = ry.trace(qs[k], tgt[k], rays, bodies, parent)
            compare(hits[k], ry.resolve(tr, MASKS["all"]), world_length(tr), what=f"{mode} own joints env {k}")
        env.close()


def test_parent_link():
    n = 37
    q, tgt = random_state(n, 31)
    env = make_env(n, q, tgt)
    rays = fan()
    mask = MASKS["all"]
    a, b = cast(env, rays, -1, mask)["hits"], cast(env, rays, 0, mask)["hits"]
    assert torch.equal(a, b)                                          # link 0 is the base: the identity
    ls = env.link_states().double().cpu().numpy()
    bodies = ref_bodies(scene_bodies())
    for link in (3, 10):
        R = lk.matrix_from_quat(ls[:, link, 3:7])
        p = ls[:, link, 0:3]
        world = np.concatenate([p[:, None] + np.einsum("nij,rj->nri", R, rays[:, 0:3].astype(np.float64)),
                                p[:, None] + np.einsum("nij,rj->nri", R, rays[:, 3:6].astype(np.float64))], axis=2).astype(np.float32)
        mounted = cast(env, rays, link, mask)["hits"].cpu().numpy()
        free = cast(env, world, -1, mask)["hits"].cpu().numpy()
        for k in (0, 11, n - 1):
            ok = ~ry.ray_test(q[k], tgt[k], rays, mask, bodies, link)["band"]
            assert ok.mean() >= 0.9
            assert np.array_equal(mounted[k, ok, 7], free[k, ok, 7]), (link, k)
            # both lie within the position tolerance of the truth for their own rays; the host's rays are rounded to float32
            length = np.linalg.norm(world[k, :, 3:6].astype(np.float64) - world[k, :, 0:3], axis=1)
            rounding = 2 * np.finfo(np.float32).eps * np.abs(world[k]).max()
            dpos = np.linalg.norm(mounted[k, ok, 1:4].astype(np.float64) - free[k, ok, 1:4], axis=1)
            dfrac = np.abs(mounted[k, ok, 0].astype(np.float64) - free[k, ok, 0])
            print(f"parent_link {link} env {k}: worst position difference {(dpos / length[ok]).max():.3e} x length, fraction {dfrac.max():.3e}")
            assert (dpos <= 2 * POS_TOL_REL * length[ok] + rounding).all(), (link, k)
            assert (dfrac <= 2 * POS_TOL_REL + rounding / length[ok]).all(), (link, k)
        assert len(set(mounted[..., 7].ravel().tolist())) > 3
    env.close()


def test_shared_and_per_env_rays_give_the_same_bits():
    n, R = 37, 67
    q, tgt = random_state(n, 41)
    env = make_env(n, q, tgt)
    rays = cycled(fan(), R)
    for parent in (-1, POINTER):
        a = cast(env, rays, parent, MASKS["all"], fractions=True)
        b = cast(env, np.broadcast_to(rays, (n, R, 6)), parent, MASKS["all"], fractions=True)
        assert torch.equal(a["hits"], b["hits"]) and torch.equal(a["fractions"], b["fractions"])
    env.close()


def test_body_positions_move_one_envs_obstacle():
    n, k = 37, 23
    q, tgt = random_state(n, 51)
    env = make_env(n, q, tgt)
    bodies = scene_bodies()
    rays, parent = ray_set("B", tgt)
    pos = np.tile(np.array([b.position for b in bodies], dtype=np.float32), (n, 1, 1))
    base = cast(env, rays, parent, MASKS["arm_bodies"])["hits"]
    assert torch.equal(cast(env, rays, parent, MASKS["arm_bodies"], body_positions=torch.from_numpy(pos).cuda())["hits"], base)
    pos[k, 0] = (4.0, -3.0, 2.0)                                      # env k's box, into the grid's view
    moved = cast(env, rays, parent, MASKS["arm_bodies"], body_positions=torch.from_numpy(pos).cuda())["hits"]
    others = [e for e in range(n) if e != k]
    assert torch.equal(moved[others], base[others]) and not torch.equal(moved[k], base[k])
    tr = ry.trace(q[k], tgt[k], rays, ref_bodies(bodies, pos[k].astype(np.float64)), parent)
    want = ry.resolve(tr, MASKS["arm_bodies"])
    assert (want["label"][~want["band"]] == rr.SEG_BODY0).any()
    compare(moved[k].cpu().numpy(), want, world_length(tr), what="moved box")
    env.close()


def test_batch_independence_and_determinism():
    n, R, k, j = 1000, 67, 511, 38
    q, tgt = random_state(n, 61)
    q[j], tgt[j] = q[k], tgt[k]                                       # the same env at another place in the batch
    env = make_env(n, q, tgt)
    rays = cycled(fan(), R)
    a = cast(env, rays, POINTER, MASKS["all"], fractions=True)
    b = cast(env, rays, POINTER, MASKS["all"], fractions=True)
    assert torch.equal(a["hits"], b["hits"]) and torch.equal(a["fractions"], b["fractions"])
    assert torch.equal(a["hits"][k], a["hits"][j]) and torch.equal(a["fractions"][k], a["fractions"][j])
    one = make_env(1, q[k:k + 1], tgt[k:k + 1], seed=4)
    alone = cast(one, rays, POINTER, MASKS["all"], fractions=True)
    assert torch.equal(alone["hits"][0], a["hits"][k]) and torch.equal(alone["fractions"][0], a["fractions"][k])
    assert len(set(a["hits"][k, :, 7].cpu().numpy().tolist())) > 2
    env.close(); one.close()


def _params(env, n_rays, mask=ry.HIT_BODIES, parent=-1, per_env=0, bodies=()):
    from pioneer_amd import _lib
    from pioneer_amd.config import fill_scene_body
    p = _lib.PnrRayParams()
    assert env.lib.pnr_ray_params_default(p) == 0
    assert p.struct_size == C.sizeof(_lib.PnrRayParams) and p.hit_mask == _lib.RAY_HIT_BODIES and p.parent_link == -1
    p.n_rays, p.rays_per_env, p.parent_link, p.hit_mask, p.n_bodies = n_rays, per_env, parent, mask, len(bodies)
    for i, b in enumerate(bodies):
        fill_scene_body(p.bodies[i], b, f"body {i}")
    return p


def _raw(env, p, rays, hits, fractions, js=None, bp=None):
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    return env.lib.pnr_ray_test(env._h, ptr(js), p, ptr(rays), ptr(bp), ptr(hits), ptr(fractions), env._stream())


@pytest.mark.parametrize("n,R", [(1, 1), (37, 67), (1000, 3)])
def test_outputs_stop_at_their_last_row(n, R):
    q, tgt = random_state(n, 71)
    env = make_env(n, q, tgt)
    rays = torch.from_numpy(cycled(fan(), R)).cuda()
    guard = 4096
    hits = torch.full((n * R * 8 + guard,), -7.25, dtype=torch.float32, device="cuda:0")
    frac = torch.full((n * R + guard,), -7.25, dtype=torch.float32, device="cuda:0")
    p = _params(env, R, MASKS["all"], POINTER, bodies=scene_bodies())
    assert _raw(env, p, rays, hits, frac) == 0
    want = cast(env, rays.cpu().numpy(), POINTER, MASKS["all"], fractions=True)
    torch.cuda.synchronize()
    assert (hits[n * R * 8:] == -7.25).all() and (frac[n * R:] == -7.25).all()
    assert torch.equal(hits[:n * R * 8], want["hits"].reshape(-1)) and torch.equal(frac[:n * R], want["fractions"].reshape(-1))
    # either output alone writes the same rows and nothing else
    only_h = torch.full_like(hits, -7.25)
    only_f = torch.full_like(frac, -7.25)
    assert _raw(env, p, rays, only_h, None) == 0 and _raw(env, p, rays, None, only_f) == 0
    assert torch.equal(only_h, hits) and torch.equal(only_f, frac)
    env.close()


def test_hits_batch_beyond_two_gigabytes():
    n, R = 65537, 1024
    assert n * R * 8 * 4 > 2 ** 31
    q, tgt = random_state(n, 81)
    env = make_env(n, q, tgt)
    rays = fan(R)
    try:
        out = {"hits": torch.empty((n, R, 8), dtype=torch.float32, device="cuda:0")}
    except torch.cuda.OutOfMemoryError:
        pytest.skip("no room for a 2.1 GB hits tensor on this device")
    hits = cast(env, rays, POINTER, MASKS["all"], out=out)["hits"]
    bodies = ref_bodies(scene_bodies())
    for k in sorted({0, n - 1, *np.random.default_rng(82).choice(n, 3, replace=False).tolist()}):
        tr = ry.trace(q[k], tgt[k], rays, bodies, POINTER)
        want = ry.resolve(tr, MASKS["all"])
        assert (~want["band"]).mean() >= 0.9
        compare(hits[k].cpu().numpy(), want, world_length(tr), what=f"large batch env {k}")
    env.close()


def test_invalid_calls_touch_nothing():
    from pioneer_amd import PioneerVectorEnv
    from pioneer_amd.config import scene_box
    n, R = 5, 4
    fresh = PioneerVectorEnv(n, device="cuda:0", seed=9)
    rays = torch.from_numpy(cycled(fan(), R)).cuda()
    hits = torch.full((n * R * 8 + 16,), -7.25, dtype=torch.float32, device="cuda:0")
    frac = torch.full((n * R + 16,), -7.25, dtype=torch.float32, device="cuda:0")
    js = torch.zeros((n * 12 + 4,), dtype=torch.float32, device="cuda:0")
    box = [scene_box((1, 1, 1), (5, 0, 0))]
    # before the first reset: the handle's own joints and the target do not exist yet ..
    assert _raw(fresh, _params(fresh, R, bodies=box), rays, hits, frac) == -1
    assert b"before the first pnr_reset" in fresh.lib.pnr_last_error(fresh._h)
    assert _raw(fresh, _params(fresh, R, mask=ry.HIT_BODIES | ry.HIT_TARGET, bodies=box), rays, hits, frac, js=js[:n * 12]) == -1
    assert b"before the first pnr_reset" in fresh.lib.pnr_last_error(fresh._h)
    torch.cuda.synchronize()
    assert (hits == -7.25).all() and (frac == -7.25).all()
    # .. but a caller's joints without the target bit need nothing of the state
    accepted = torch.full_like(hits, -7.25)
    assert _raw(fresh, _params(fresh, R, mask=ry.HIT_BODIES | ry.HIT_ARM, parent=POINTER, bodies=box), rays, accepted, None, js=js[:n * 12]) == 0
    torch.cuda.synchronize()
    assert not (accepted[:n * R * 8] == -7.25).any() and (accepted[n * R * 8:] == -7.25).all()
    env = fresh
    env.reset()

    def bad(mutate=lambda p: None, r=rays, outs=(hits, frac), js=None, bp=None):
        p = _params(env, R, MASKS["all"], POINTER, bodies=box)
        mutate(p)
        return _raw(env, p, r, *outs, js=js, bp=bp)

    nan = float("nan")
    cases = [lambda p: setattr(p, "struct_size", 12), lambda p: setattr(p, "n_rays", 0), lambda p: setattr(p, "n_rays", 1025),
             lambda p: setattr(p, "parent_link", -2), lambda p: setattr(p, "parent_link", 11), lambda p: setattr(p, "n_bodies", -1),
             lambda p: setattr(p, "n_bodies", 9), lambda p: setattr(p, "hit_mask", 0), lambda p: setattr(p, "hit_mask", 8),
             lambda p: setattr(p, "hit_mask", 15), lambda p: setattr(p, "rays_per_env", 2), lambda p: setattr(p, "rays_per_env", -1),
             lambda p: setattr(p.bodies[0], "shape", 7), lambda p: p.bodies[0].position.__setitem__(0, nan),
             lambda p: p.bodies[0].size.__setitem__(1, 0.0), lambda p: [p.bodies[0].orientation.__setitem__(k, 0.0) for k in range(4)]]
    for i, mutate in enumerate(cases):
        assert bad(mutate) == -1, i
        assert b"PNR_" not in env.lib.pnr_last_error(env._h)
    assert _raw(env, None, rays, hits, frac) == -1                                 # null params
    assert env.lib.pnr_ray_test(None, None, _params(env, R), C.c_void_p(rays.data_ptr()), None, C.c_void_p(hits.data_ptr()), None, None) == -1
    assert bad(r=None) == -1 and bad(outs=(None, None)) == -1
    bytes_ = torch.zeros(rays.numel() * 4 + 8, dtype=torch.uint8, device="cuda:0")
    assert bad(r=bytes_[2:]) == -1                                                  # rays off a 4-byte boundary
    assert bad(outs=(hits[1:], frac)) == -1 and bad(outs=(hits, frac[1:])) == -1 and bad(outs=(hits[2:], None)) == -1
    assert bad(js=js[1:]) == -1
    assert bad(bp=bytes_[1:]) == -1
    torch.cuda.synchronize()
    assert (hits == -7.25).all() and (frac == -7.25).all()
    assert bad() == 0                                                               # the unmutated call runs
    torch.cuda.synchronize()
    assert not (hits[:n * R * 8] == -7.25).any() and (hits[n * R * 8:] == -7.25).all()
    assert not (frac[:n * R] == -7.25).any() and (frac[n * R:] == -7.25).all()
    with pytest.raises(AssertionError):
        env.ray_test(rays, hits=False, fractions=False)
    with pytest.raises(AssertionError):
        env.ray_test(torch.zeros((n + 1, R, 6), device="cuda:0"))
    env.close()


def test_graph_capture_replays_on_new_joints():
    n, R = 37, 32
    q, tgt = random_state(n, 91)
    env = make_env(n, q, tgt)
    rays, parent = ray_set("A", tgt)
    bodies = ref_bodies(scene_bodies())
    js = torch.from_numpy(np.concatenate([q, np.zeros((n, 6), np.float32)], axis=1)).cuda()
    dev_rays = torch.from_numpy(rays).cuda()
    out = {"hits": torch.zeros((n, R, 8), device="cuda:0"), "fractions": torch.zeros((n, R), device="cuda:0")}
    kw = dict(parent_link=parent, hit_arm=True, hit_target=True, bodies=scene_bodies(), joint_state=js, fractions=True, out=out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        env.ray_test(dev_rays, **kw)                                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.ray_test(dev_rays, **kw)
    q2, _ = random_state(n, 92)
    js[:, 0:6] = torch.from_numpy(q2).cuda()                          # in place: the captured pointer stays
    out["hits"].zero_(); out["fractions"].zero_()
    graph.replay()
    torch.cuda.synchronize()
    hits = out["hits"].cpu().numpy()
    assert hits[..., 0].tobytes() == out["fractions"].cpu().numpy().tobytes()
    for k in (0, n - 1):
        tr = ry.trace(q2[k], tgt[k], rays, bodies, parent)
        compare(hits[k], ry.resolve(tr, MASKS["all"]), world_length(tr), what=f"replay env {k}")
    assert not np.array_equal(hits, cast(env, rays, parent, MASKS["all"])["hits"].cpu().numpy())     # (the handle's own joints differ)
    env.close()


@pytest.mark.parametrize("mode", ["kinematic", "dynamic"])
def test_facade(mode):
    from pioneer_amd import EngineConfig, PioneerKinematicEnv
    from pioneer_amd.scene import RayHit
    env = PioneerKinematicEnv(engine_config=EngineConfig(mode=mode))
    q0 = np.array([0.3, 0.4, -0.2, 0.1, 0.5, 0.0])
    env.reset_world(q0, (18.0, 2.0, 4.0))
    env.scene.create_body_sphere("marker", False, 0, 1.0, (-20.0, 20.0, 8.0), (0, 0, 0, 1))      # no collision shape: never hit
    env.scene.create_body_plane("ground", 0, (0, 0, 1), (0, 0, -1.0), (0, 0, 0, 1))
    env.scene.create_body_box("crate", True, 0, (1.0, 1.0, 1.0), (-20.0, -20.0, 0.0), (0, 0, 0, 1))
    down = env.scene.ray_test((-20.0, 20.0, 19.0), (-20.0, 20.0, -21.0))        # through the marker onto the plane
    assert down[:2] == (1, -1) and down.hitFraction == pytest.approx(0.5, abs=1e-5)
    assert down.hitNormal == pytest.approx((0.0, 0.0, 1.0), abs=1e-6) and down.hitPosition == pytest.approx((-20.0, 20.0, -1.0), abs=1e-4)
    crate = env.scene.ray_test((-20.0, -20.0, 11.0), (-20.0, -20.0, -9.0))
    assert crate[:2] == (2, -1) and crate.hitFraction == pytest.approx(0.5, abs=1e-5)
    assert env.scene.ray_test((-20.0, 20.0, 19.0), (-20.0, 30.0, 25.0)) == RayHit(-1, -1, 1.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    vec = env._vec
    q = (vec.get_dyn_state()[0:6, 0] if mode == "dynamic" else env.scene._bullet[0, 0:6]).cpu().numpy().astype(np.float64)
    bodies = [("plane", (0, 0, -1.0), (0, 0, 0, 1), (0, 0, 1)), ("box", (-20.0, -20.0, 0.0), (0, 0, 0, 1), (1.0, 1.0, 1.0))]
    # a ray down the base's axis meets the arm: body 0 with the URDF link's index
    axis = np.array([[0.2, 0.1, 30.0, 0.2, 0.1, 0.5]], dtype=np.float32)
    want = ry.ray_test(q, (18.0, 2.0, 4.0), axis, ry.HIT_ARM | ry.HIT_BODIES, bodies)
    assert not want["band"][0] and 1 < want["label"][0] < 12
    arm = env.scene.ray_test(axis[0, 0:3], axis[0, 3:6])
    assert arm[:2] == (0, want["label"][0] - 1) and arm.hitFraction == pytest.approx(want["fraction"][0], abs=1e-5)
    # a fan mounted on the pointer
    rays = fan()
    got = env.scene.ray_test_batch(rays[:, 0:3], rays[:, 3:6], parent_item=env.scene.links_by_name["robot:pointer"])
    want = ry.ray_test(q, (18.0, 2.0, 4.0), rays, ry.HIT_ARM | ry.HIT_BODIES, bodies, POINTER)
    assert len(got) == 32 and (~want["band"]).mean() >= 0.9
    for r in np.flatnonzero(~want["band"]):
        lab = want["label"][r]
        ids = (-1, -1) if lab == 0 else ((0, lab - 1) if lab < 12 else (1 + lab - 13, -1))
        assert got[r][:2] == ids, (r, got[r], lab)
        assert got[r].hitFraction == pytest.approx(want["fraction"][r], abs=1e-5)
    assert {g.objectUniqueId for g in got} >= {0, 1}
    with pytest.raises(AssertionError):
        env.scene.ray_test_batch(rays[:, 0:3], rays[:, 3:6], parent_item=env.scene.items_by_name["crate"])
    env.close()
