"""GPU tests of pnr_path_clearance (PioneerVectorEnv.path_clearance / solve_ik_free, Scene.path_clearance) against the float64
reference of tests/path_clearance_ref.py, on the inputs of tests/path_clearance_cases.py.

The bar (cases.BAR): min(FLOOR_MARGIN (8) x what float32 arithmetic alone costs on these inputs, the contact query's hard bar
1e-4); tests/test_path_clearance_cpu.py asserts the floor.  The minimum of continuous distances needs no exclusion.  The index
outputs are checked through the reference's distance of the reported triple, and by equality only where the reference's
runner-up is more than 1e-3 away; first_hit / violations / free are exact on every env without a configuration within 1e-3 of
the margin.  Every test prints its figures before it asserts.  MEASURED VALUES ON AN MI355X: see DESIGN.md 3y (the worst
clearance error of any case was 3.6e-6 of the 3.7e-5 bar).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import contact_query_ref as cq
import path_clearance_cases as cases
import path_clearance_ref as ref
from gpu_support import dev, dyn_env, f64, kin_env, lib as _lib, load_joints

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
FAMILIES = "AB"


def scene_bodies(bodies=cases.SCENE_A):
    from pioneer_amd.config import scene_box, scene_plane, scene_sphere
    make = {"plane": lambda b: scene_plane(b["size"], b["position"], b["quat"]),
            "box": lambda b: scene_box(b["size"], b["position"], b["quat"]),
            "sphere": lambda b: scene_sphere(b["size"][0], b["position"])}
    return [make[b["shape"]](b) for b in bodies]


def make_kin(n, reset=True):
    return kin_env(n, cases.SEED, reset, auto_reset=False, max_episode_steps=0)


def make_env(name, n, mode="dynamic"):
    """an env for a shape: any for a path of given waypoints, one holding cases.current_joints for the from_current shape"""
    if not cases.SHAPES[name][3]:
        return make_kin(n)
    q = cases.current_joints(n)
    if mode == "dynamic":
        env = dyn_env(n, cases.SEED, 9.81, 1)
        load_joints(env, q)
        return env
    env = make_kin(n)                                                   # the env's r (state words 12-17)
    w = env.get_state()
    w.view(torch.float32)[12:18] = dev(q.T)
    env.set_state(w)
    return env


def sweep(env, name, n, family, lanes=0, margin=0.0, **kw):
    K, M, _, current = cases.SHAPES[name]
    bp = dev(cases.family_b_positions(name, n)) if family == "B" else None
    return env.path_clearance(dev(cases.given_waypoints(name, n)), substeps=M, from_current=current, bodies=scene_bodies(), body_positions=bp,
                              margin=margin, profile=True, lanes_per_env=lanes, **kw)


def check_against_reference(res, name, family, n, margin, what):
    r = cases.reference(name, family, margin)
    K, M, _, current = cases.SHAPES[name]
    W = K + int(current)
    rows = np.arange(n)
    sm, cl = f64(res["summary"]), f64(res["clearance"])
    want, wsm = r["clearance"][:n], r["summary"][:n]
    e_prof, e_min = float(np.abs(cl - want).max()), float(np.abs(sm[:, 0] - wsm[:, 0]).max())
    # the reported triple, evaluated in the reference
    t32 = ref.path_coordinates(W, M, np.float32).astype(np.float64)
    known = np.isin(sm[:, 1], t32)
    c = np.searchsorted(t32, sm[:, 1]).clip(0, len(t32) - 1)
    s, b = sm[:, 2].astype(int), sm[:, 3].astype(int)
    in_range = known & (s >= 0) & (s < cq.SAMPLES) & (b >= 0) & (b < len(cases.SCENE_A))
    pairs = r["pairs"][:n]
    d_triple = pairs[rows, c, s.clip(0, cq.SAMPLES - 1), b.clip(0, 2)]
    e_triple = float((d_triple - wsm[:, 0]).max())
    flat = np.sort(pairs.reshape(n, -1), axis=1)
    clear_winner = flat[:, 1] - flat[:, 0] > 1e-3
    same = (c == r["config"][:n]) & (s == wsm[:, 2]) & (b == wsm[:, 3])
    # the margin's outputs, exact outside the near-margin envs
    ok = ~ref.near_margin(want, margin, cases.NEAR).any(axis=1)
    first32 = np.where(r["first"][:n] >= 0, t32[np.maximum(r["first"][:n], 0)], -1.0)
    exact = (np.array_equal(sm[ok, 4], first32[ok]) and np.array_equal(sm[ok, 5], wsm[ok, 5]) and np.array_equal(sm[ok, 6], wsm[ok, 6])
             and bool((sm[:, 7] == 0).all()))
    print(f"{what} {name} family {family} n={n} margin {margin}: profile {e_prof:.2e} minimum {e_min:.2e} (bar {cases.BAR:.1e}); reported triple "
          f"above the reference's minimum by {e_triple:.2e} (bar {2 * cases.BAR:.1e}); envs with a clear winner {clear_winner.mean():.2f}, "
          f"of them equal {same[clear_winner].mean() if clear_winner.any() else 1.0:.2f}; envs compared on the margin {ok.mean():.3f}, "
          f"free {wsm[:, 6].mean():.2f}: {'exact' if exact else 'DIFFERENT'}")
    assert e_prof <= cases.BAR and e_min <= cases.BAR
    assert in_range.all() and e_triple <= 2 * cases.BAR
    assert same[clear_winner].all()
    assert exact and ok.mean() >= 0.9 or n < 37
    assert exact or not ok.any()
    # the dict's named tensors are the summary's columns
    for col, key in enumerate(("min_distance", "at", "sample", "body", "first_hit", "violations")):
        assert np.array_equal(f64(res[key]), sm[:, col]), key
    assert res["free"].dtype == torch.bool and np.array_equal(res["free"].cpu().numpy(), sm[:, 6] > 0)


# ---- 1. parity with the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.SHAPES))
def test_path_clearance_against_the_reference(name):
    for n in cases.SIZES:
        env = make_env(name, n)
        for lanes in cases.SHAPES[name][2]:
            for family in FAMILIES:
                for margin in (cases.MARGINS if n == cases.N_MAX else cases.MARGINS[:1]):
                    res = sweep(env, name, n, family, lanes, margin)
                    torch.cuda.synchronize()
                    check_against_reference(res, name, family, n, margin, f"lanes {lanes}")
        env.close()


# ---- 2. the tie rules -----------------------------------------------------------------------------------------------------------
def test_identical_waypoints_tie_at_the_first_configuration():
    n = cases.N_MAX
    env = make_kin(n)
    w = cases.given_waypoints("k3_m3", n)
    same = dev(np.repeat(w[:, :1], 3, axis=1))
    for lanes in (0, 1, 64):
        res = env.path_clearance(same, substeps=3, bodies=scene_bodies(), profile=True, lanes_per_env=lanes)
        torch.cuda.synchronize()
        sm, cl = f64(res["summary"]), f64(res["clearance"])
        print(f"lanes {lanes}: at {np.unique(sm[:, 1])}, first_hit {np.unique(sm[:, 4])}, free {sm[:, 6].mean():.2f}")
        assert (cl == cl[:, :1]).all()                                  # one configuration seven times: the same bits
        assert (sm[:, 1] == 0).all() and np.isin(sm[:, 4], (0.0, -1.0)).all()
        assert np.array_equal(sm[:, 4] == 0, sm[:, 6] == 0) and np.array_equal(sm[:, 5], np.where(sm[:, 6] == 0, 7.0, 0.0))
    env.close()


# ---- 3. lanes_per_env -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k5_m20", "k3_m3", "k1_m4_current"])
def test_every_lanes_per_env_gives_the_same_bits(name):
    n = cases.N_MAX
    env = make_env(name, n)
    base = sweep(env, name, n, "B", 0, 0.5)
    for lanes in (1, 2, 4, 8, 16, 32, 64):
        res = sweep(env, name, n, "B", lanes, 0.5)
        torch.cuda.synchronize()
        same = torch.equal(res["summary"], base["summary"]) and torch.equal(res["clearance"], base["clearance"])
        print(f"{name}: lanes_per_env {lanes} against auto: {'bit-identical' if same else 'DIFFERENT'}")
        assert same
    alone = env.path_clearance(dev(cases.given_waypoints(name, n)), substeps=cases.SHAPES[name][1], from_current=cases.SHAPES[name][3],
                               bodies=scene_bodies(), body_positions=dev(cases.family_b_positions(name, n)), margin=0.5)
    assert "clearance" not in alone and torch.equal(alone["summary"], base["summary"])     # the summary without the profile
    env.close()


# ---- 4. batch independence ------------------------------------------------------------------------------------------------------
def test_an_envs_results_do_not_depend_on_the_batch():
    name, k = "k5_m20", 77
    K, M = cases.SHAPES[name][:2]
    w, bp = cases.given_waypoints(name), cases.family_b_positions(name)
    big, one = make_kin(cases.N_MAX), make_kin(1)
    in_batch = big.path_clearance(dev(w), substeps=M, bodies=scene_bodies(), body_positions=dev(bp), profile=True)
    shared = big.path_clearance(dev(w[k]), substeps=M, bodies=scene_bodies(), body_positions=dev(np.repeat(bp[k:k + 1], cases.N_MAX, axis=0)),
                                profile=True)
    for lanes in (0, 1):
        alone = one.path_clearance(dev(w[k:k + 1]), substeps=M, bodies=scene_bodies(), body_positions=dev(bp[k:k + 1]), profile=True, lanes_per_env=lanes)
        torch.cuda.synchronize()
        for key in ("summary", "clearance"):
            same = torch.equal(in_batch[key][k], alone[key][0]) and torch.equal(shared[key][5], alone[key][0])
            print(f"{key}: env {k} alone (lanes {lanes}) / in a batch of {cases.N_MAX} / as the path shared by all: {'bit-identical' if same else 'DIFFERENT'}")
            assert same
    assert torch.equal(shared["summary"], shared["summary"][:1].expand(cases.N_MAX, -1))
    big.close(); one.close()


# ---- 5. agreement with contacts() -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sphere", [False, True])
def test_the_waypoints_clearance_is_the_contact_querys_distance(sphere):
    name, n = "k16_m1", 64
    K = cases.SHAPES[name][0]
    w = cases.given_waypoints(name, n)
    bp = dev(cases.family_b_positions(name, n))
    env = dyn_env(n, cases.SEED, 0.0, 1)
    if sphere:                                                          # a moving sphere near every env's path, none in every fifth env
        centre = cq.query(w[:, 3], np.zeros_like(w[:, 3]), ())["centres"][:, 12] + np.array([0.0, 1.0, 0.5])
        env.set_body(mass=np.where(np.arange(n) % 5 == 0, 0.0, 1.0), radius=1.2, position=centre, velocity=(0.3, 0.0, 0.0))
        env.set_body_queries(contacts=True)
    res = env.path_clearance(dev(w), substeps=1, bodies=scene_bodies(), body_positions=bp, profile=True)
    ptr = env.path_clearance(dev(w), substeps=1, bodies=scene_bodies(), body_positions=bp, profile=True, samples=[22])
    worst = worst_ptr = 0.0
    bodies_seen = set()
    for k in range(K):
        js = dev(np.concatenate([w[:, k], np.zeros((n, 6), np.float32)], axis=1))
        got = env.contacts(joint_state=js, bodies=scene_bodies(), body_positions=bp)
        worst = max(worst, float((res["clearance"][:, k] - got["summary"][:, 0]).abs().max()))
        worst_ptr = max(worst_ptr, float((ptr["clearance"][:, k] - got["points"][:, 22, 0]).abs().max()))
        bodies_seen |= set(got["summary"][:, 2].long().tolist())
    torch.cuda.synchronize()
    sm = res["summary"]
    print(f"sphere {sphere}: |profile - contacts().summary| {worst:.2e}, pointer alone against points[:, 22, 0] {worst_ptr:.2e} (bar {cases.BAR:.1e}); "
          f"nearest bodies seen {sorted(bodies_seen)}; path minima on the sphere {(sm[:, 3] == 8).float().mean():.2f}")
    assert worst <= cases.BAR and worst_ptr <= cases.BAR
    assert (ptr["sample"] == 22).all() and (ptr["clearance"] >= res["clearance"]).all()
    assert (8 in bodies_seen) == sphere and bool((sm[:, 3] == 8).any()) == sphere
    if sphere:
        assert not bool((sm[::5, 3] == 8).any())                        # mass 0: no sphere in that env
    env.close()


# ---- 6. from_current ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dynamic", "kinematic"])
def test_from_current_reads_the_envs_own_joints(mode):
    name, n = "k1_m4_current", cases.N_MAX
    env = make_env(name, n, mode)
    for family in FAMILIES:
        res = sweep(env, name, n, family)
        torch.cuda.synchronize()
        check_against_reference(res, name, family, n, 0.0, mode)
    # the same path with the env's joints handed in as waypoint 0: the same bits
    both = dev(cases.path_waypoints(name, n))
    given = env.path_clearance(both, substeps=4, bodies=scene_bodies(), profile=True)
    own = env.path_clearance(both[:, 1:], substeps=4, from_current=True, bodies=scene_bodies(), profile=True)
    stand = env.path_clearance(None, from_current=True, bodies=scene_bodies(), profile=True)
    torch.cuda.synchronize()
    assert torch.equal(given["summary"], own["summary"]) and torch.equal(given["clearance"], own["clearance"])
    assert stand["clearance"].shape == (n, 1) and torch.equal(stand["clearance"][:, 0], own["clearance"][:, 0])
    env.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing():
    L = _lib()
    n, K = 64, 3
    env = make_kin(n)
    lib, h, st = env.lib, env._h, env._stream()
    way = dev(cases.given_waypoints("k3_m3", n))
    bp = dev(cases.family_b_positions("k3_m3", n))
    sm = torch.full((n + 1, 8), SENTINEL, device="cuda:0")
    cl = torch.full((n + 1, 7), SENTINEL, device="cuda:0")
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731

    def params(**kw):
        from pioneer_amd.config import fill_scene_body
        p = L.PnrPathParams()
        assert lib.pnr_path_params_default(p) == 0
        bodies = scene_bodies()
        p.n_waypoints, p.substeps, p.waypoints_per_env, p.n_bodies = K, 3, 1, len(bodies)
        for i, b in enumerate(bodies):
            fill_scene_body(p.bodies[i], b, "body")
        for key, v in kw.items():
            setattr(p, key, v)
        return p

    def refused(what, hh, p, wp, bpp, a, b):
        rc = lib.pnr_path_clearance(hh, p, wp, bpp, a, b, st)
        msg = lib.pnr_last_error(hh).decode()
        torch.cuda.synchronize()
        print(f"{what!r}: rc {rc}, {msg!r}")
        assert rc == -1 and what in msg, (what, rc, msg)
        assert bool((sm == SENTINEL).all()) and bool((cl == SENTINEL).all())

    ok = params()
    refused("null handle", None, ok, P(way), None, P(sm), P(cl))
    refused("null params", h, None, P(way), None, P(sm), P(cl))
    refused("struct_size", h, params(struct_size=8), P(way), None, P(sm), P(cl))
    refused("n_bodies", h, params(n_bodies=-1), P(way), None, P(sm), P(cl))
    refused("n_bodies", h, params(n_bodies=9), P(way), None, P(sm), P(cl))
    bad = params(); bad.bodies[1].shape = 7
    refused("bad shape", h, bad, P(way), None, P(sm), P(cl))
    bad = params(); bad.bodies[2].position[1] = float("nan")
    refused("non-finite data", h, bad, P(way), None, P(sm), P(cl))
    bad = params()
    for i in range(4):
        bad.bodies[1].orientation[i] = 0.0
    refused("zero orientation quaternion", h, bad, P(way), None, P(sm), P(cl))
    bad = params(); bad.bodies[1].size[0] = 0.0
    refused("box half extents", h, bad, P(way), None, P(sm), P(cl))
    bad = params(); bad.bodies[2].size[0] = -1.0
    refused("sphere radius", h, bad, P(way), None, P(sm), P(cl))
    bad = params()
    for i in range(3):
        bad.bodies[0].size[i] = 0.0
    refused("zero plane normal", h, bad, P(way), None, P(sm), P(cl))
    refused("16-byte aligned", h, ok, P(way), None, P(sm, 8), P(cl))
    refused("4-byte aligned", h, ok, P(way), None, P(sm), P(cl, 2))
    refused("8-byte aligned", h, ok, P(way, 4), None, P(sm), P(cl))
    refused("4-byte aligned", h, ok, P(way), P(bp, 2), P(sm), P(cl))
    refused("every output is NULL", h, ok, P(way), None, None, None)
    refused("n_waypoints", h, params(n_waypoints=-1), P(way), None, P(sm), P(cl))
    refused("n_waypoints", h, params(n_waypoints=257), P(way), None, P(sm), P(cl))
    refused("n_waypoints 0 without from_current", h, params(n_waypoints=0), P(way), None, P(sm), P(cl))
    refused("null waypoints", h, ok, None, None, P(sm), P(cl))
    refused("substeps", h, params(substeps=0), P(way), None, P(sm), P(cl))
    refused("substeps", h, params(substeps=65), P(way), None, P(sm), P(cl))
    for lanes in (-1, 3, 128):
        refused("lanes_per_env", h, params(lanes_per_env=lanes), P(way), None, P(sm), P(cl))
    refused("from_current", h, params(from_current=2), P(way), None, P(sm), P(cl))
    refused("waypoints_per_env", h, params(waypoints_per_env=-1), P(way), None, P(sm), P(cl))
    refused("sample_mask", h, params(sample_mask=0), P(way), None, P(sm), P(cl))
    refused("sample_mask", h, params(sample_mask=1 << 23), P(way), None, P(sm), P(cl))
    refused("sample_mask", h, params(sample_mask=(1 << 23) | 1), P(way), None, P(sm), P(cl))
    for margin in (float("nan"), float("inf")):
        refused("margin", h, params(margin=margin), P(way), None, P(sm), P(cl))
    fresh = make_kin(n, reset=False)                                    # its own joints do not exist before the first reset
    refused("before the first pnr_reset", fresh._h, params(from_current=1), P(way), None, P(sm), P(cl))
    assert fresh.lib.pnr_path_clearance(fresh._h, ok, P(way), None, P(sm), P(cl), st) == 0      # given waypoints need no reset
    torch.cuda.synchronize()
    assert not bool((sm[:n] == SENTINEL).any()) and bool((sm[n:] == SENTINEL).all())
    assert not bool((cl[:n] == SENTINEL).any()) and bool((cl[n:] == SENTINEL).all())             # nothing past row n
    with pytest.raises(AssertionError):
        env.path_clearance(way, samples=[23])
    with pytest.raises(AssertionError):
        env.path_clearance(way[:, :, :5])
    fresh.close()
    env.close()


# ---- 8. graph capture -----------------------------------------------------------------------------------------------------------
def test_the_call_is_captured_and_replayed():
    name, n = "k5_m20", cases.N_MAX
    M = cases.SHAPES[name][1]
    env = make_kin(n)
    w_a = dev(cases.given_waypoints(name, n))
    w_b = dev(cases.given_waypoints(name, n)[::-1].copy())
    bp = dev(cases.family_b_positions(name, n))
    w = w_a.clone()
    out = {"summary": torch.empty((n, 8), device="cuda:0"), "clearance": torch.empty((n, 81), device="cuda:0")}
    call = lambda: env.path_clearance(w, substeps=M, bodies=scene_bodies(), body_positions=bp, margin=0.5, profile=True, out=out)  # noqa: E731
    s = torch.cuda.Stream(device=env.device)
    s.wait_stream(torch.cuda.current_stream(env.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        call()                                                          # warm-up on the capture stream
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):                             # a single chain: one kernel node
            call()
    torch.cuda.synchronize()
    for label, src in (("first replay", w_b), ("second replay", w_a)):
        w.copy_(src)
        for v in out.values():
            v.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        eager = env.path_clearance(src, substeps=M, bodies=scene_bodies(), body_positions=bp, margin=0.5, profile=True)
        torch.cuda.synchronize()
        same = all(torch.equal(out[k], eager[k]) for k in out)
        print(f"{label}: replayed outputs {'equal' if same else 'DIFFER from'} the eager call's bits")
        assert same
    env.close()


# ---- 9. solve_ik_free -----------------------------------------------------------------------------------------------------------
def test_solve_ik_free_returns_the_nearest_free_solution():
    import ik_multi_ref as mref
    s = cases.ik_scenario()
    n, S = cases.IK_ENVS, cases.IK_STARTS
    env = make_kin(n)
    box = scene_bodies((cases.IK_BOX,))
    tgt = dev(s["targets"])
    res = env.solve_ik_free(target=tgt, starts=S, bodies=box, margin=cases.IK_MARGIN)
    multi = env.solve_ik_multi(target=tgt, starts=S, return_all=True)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in res.items()}
    rows = np.arange(n)
    assert np.array_equal(out["all_q"], multi["all_q"].cpu().numpy())
    # the references on the kernel's own per-start solutions: clearance in float64, convergence as the kernel tests it
    clr = ref.sweep(out["all_q"], 1, (cases.IK_BOX,), pointer_radius=cases.POINTER_RADIUS)["clearance"]
    e_clr = float(np.abs(out["all_clearance"] - clr).max())
    conv = out["all_residual"] <= np.float32(mref.POSITION_DEFAULTS["tolerance"])
    decided = ~(ref.near_margin(clr, cases.IK_MARGIN, cases.NEAR) & conv).any(axis=1)
    ok = conv & (clr >= cases.IK_MARGIN)
    free = ok.any(axis=1)
    cost = ((out["all_q"].astype(np.float64) - mref.start_table(S)[0]) ** 2).sum(axis=2)
    best = np.where(ok, cost, np.inf).min(axis=1)
    pick = out["start"].astype(int)
    chosen_cost = cost[rows, pick]
    winner = multi["start"].cpu().numpy().astype(int)
    counted = s["counted"]
    winner_collides = clr[rows, winner] < cases.IK_MARGIN
    print(f"clearance of the starts against the reference {e_clr:.2e} (bar {cases.BAR:.1e}); decided envs {decided.mean():.3f}; free {free.mean():.3f} "
          f"(reference scenario {(s['per']['converged_starts'] & (s['clearance'] >= cases.IK_MARGIN)).any(axis=1).mean():.3f}); counted envs "
          f"{counted.sum()}, of them solve_ik_multi's winner collides in {winner_collides[counted].sum()}, solve_ik_free's choice differs from it in "
          f"{(pick != winner)[counted].sum()}")
    assert e_clr <= cases.BAR and decided.mean() >= 0.9
    d = decided
    assert np.array_equal(out["free"][d], free[d])
    f = d & free
    assert conv[rows, pick][f].all() and (clr[rows, pick][f] >= cases.IK_MARGIN).all()             # converged and free ..
    assert (chosen_cost[f] <= best[f] * (1 + 1e-5) + 1e-6).all()                                     # .. and the nearest such
    assert np.array_equal(pick[d & ~free], winner[d & ~free])                                        # none: solve_ik_multi's own winner
    for key in ("q", "residual", "iterations"):
        assert np.array_equal(out[key], out["all_" + key][rows, pick]), key
    assert np.array_equal(out["clearance"], out["all_clearance"][rows, pick])
    assert counted.mean() >= 0.1 and winner_collides[counted].all()
    assert (out["free"] & (pick != winner))[counted].all()                                           # the feature: another, free start
    env.close()


# ---- 10. a NaN waypoint ---------------------------------------------------------------------------------------------------------
def test_a_nan_waypoint_makes_its_env_not_free_and_touches_no_other():
    name, n, k = "k3_m3", cases.N_MAX, 70
    env = make_kin(n)
    w = cases.given_waypoints(name, n)
    bp = dev(cases.family_b_positions(name, n))
    bad = w.copy()
    bad[k, 1, 3] = np.nan
    for lanes in (0, 1, 64):
        good = env.path_clearance(dev(w), substeps=3, bodies=scene_bodies(), body_positions=bp, profile=True, lanes_per_env=lanes)
        res = env.path_clearance(dev(bad), substeps=3, bodies=scene_bodies(), body_positions=bp, profile=True, lanes_per_env=lanes)
        torch.cuda.synchronize()
        sm, cl = f64(res["summary"]), f64(res["clearance"])
        print(f"lanes {lanes}: env {k} summary {sm[k].tolist()}, profile {cl[k].tolist()}")
        assert sm[k, 0] == -np.inf and sm[k, 6] == 0 and not bool(res["free"][k])
        assert np.array_equal(np.isneginf(cl[k]), [False, True, True, True, True, True, False])      # the two segments at the waypoint
        assert sm[k, 1] == np.float32(1) / np.float32(3) and sm[k, 2] == 15 and sm[k, 3] == 0       # as the reference's tie rules say
        assert sm[k, 5] >= 5 and sm[k, 4] in (0.0, float(np.float32(1) / np.float32(3)))
        others = np.arange(n) != k
        assert torch.equal(res["summary"][others], good["summary"][others]) and torch.equal(res["clearance"][others], good["clearance"][others])
        assert np.isfinite(f64(good["clearance"])).all()
    none = env.path_clearance(dev(bad), substeps=3, bodies=[], profile=True)
    torch.cuda.synchronize()
    assert np.array_equal(f64(none["summary"]), np.tile([np.inf, 0, 0, -1, -1, 0, 1, 0], (n, 1)))      # no pair: nothing to be -inf
    env.close()


# ---- 11. the facade -------------------------------------------------------------------------------------------------------------
def test_facade_path_clearance():
    from pioneer_amd import PioneerKinematicEnv
    from pioneer_amd.scene import PathClearance
    env = PioneerKinematicEnv(device="cuda:0")
    quat = env.scene.rpy2quat((0, 0, 0))
    env.scene.create_body_plane(name="ground", mass=0.0, normal=(0, 0, 1.0), position=(0, 0, -1.0), orientation=quat)
    env.scene.create_body_box(name="obstacle:1", collision=True, mass=0.0, half_extents=(2.0, 6.0, 2.0), position=(15.0, 0.0, 2.0),
                              orientation=quat, rgba_color=(0, 0, 0, 1))
    env.reset_world()
    w = np.zeros((2, 6), np.float32)
    w[1, 1] = 0.8                                                       # joint 2 leans the arm forward and down, into the box
    got = env.scene.path_clearance(w, substeps=8)
    want = ref.sweep(w[None], 8, (cq.plane((0, 0, 1.0), (0, 0, -1.0)), cases.IK_BOX), pointer_radius=cases.POINTER_RADIUS)["summary"][0]
    print(got, want.tolist())
    assert isinstance(got, PathClearance) and PathClearance._fields == ("free", "min_distance", "at", "link_name", "body_id", "first_hit")
    assert got.free is False and got.min_distance < 0 and abs(got.min_distance - want[0]) <= cases.BAR
    assert got.at == float(np.float32(want[1])) and got.first_hit == float(np.float32(want[4])) and 0 < got.first_hit <= got.at
    assert got.body_id == 2 == env.scene.body_id(env.scene.items_by_name["obstacle:1"])            # the box was created second
    assert want[2] == 16 and got.link_name == env.scene.links[cq.SAMPLE_LINKS[16]].name == "robot:rotator2"
    clear = env.scene.path_clearance(w[:1], substeps=1)
    assert clear.free is True and clear.first_hit == -1.0 and clear.at == 0.0 and clear.min_distance > 0
    env.close()
