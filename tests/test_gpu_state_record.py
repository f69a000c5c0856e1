"""The engine's state record (pnr_device.h): planes 0 and 1, a hot half (r[3p+2] and potential | step_index, 8 bytes per half
record) and a cold part (target xyz, episode: 16 bytes per env) that a step loads but stores only where it resets the env.  The
canonical [24][n] words of include/pioneer_amd.h do not change; these tests go through them.

  * round trip: pnr_set_state -> pnr_get_state returns every word bit for bit;
  * the cold words survive steps that do not reset (and the hot words are the oracle's);
  * the cold words are rewritten by a reset inside a step;
  * the kernels that read joints or the target straight from the record (link states, ray casts, IK) find them.

Sizes: 1, 31, 32, 33, 65 — one env, a ragged tile, a full tile, a tile and one env, two tiles and one env; 32 768 and 32 800, the
last size of the one-pass form without the row pass and the first with it (step_row_pass, pnr_api.hip).  Equalities and
tolerances are the kinematic suite's (tests/bars.py): a, v, r, target, step_index, episode bit-exact, potential within POT_TOL.
"""
import numpy as np
import pytest
import torch

from bars import POT_TOL
from gpu_support import check_state_exact, dev, make_pair, words

pytestmark = pytest.mark.gpu

SMALL = [1, 31, 32, 33, 65]
NAN1, NAN2, PINF, NINF = 0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000


def _env(n, mode="kinematic", seed=3, auto_reset=False, max_steps=0, env_id_offset=0):
    from pioneer_amd import EngineConfig, PioneerVectorEnv
    return PioneerVectorEnv(n, device="cuda:0", seed=seed, env_id_offset=env_id_offset,
                            engine_config=EngineConfig(mode=mode, auto_reset=auto_reset, max_episode_steps=max_steps))


def _state_tensor(w):
    return dev(w.view(np.int32), torch.int32)


def _distinct_words(n):
    """every (word, env) its own bit pattern; non-finite floats in the target and the episode of the first, a middle and the last env"""
    k, e = np.meshgrid(np.arange(24, dtype=np.uint64), np.arange(n, dtype=np.uint64), indexing="ij")
    w = (((k + 1) << np.uint64(26)) ^ (e * np.uint64(2654435761) & np.uint64(0x3FFFFFF)) ^ (e << np.uint64(7))).astype(np.uint32)
    for j, env in enumerate(sorted({0, n // 2, n - 1})):
        w[18:21, env] = np.roll([NAN1, PINF, NINF], j)
        w[23, env] = (NAN2, 0xFFFFFFFF, PINF)[j]
    return w


def _state_with_odd_cold_words(env, n):
    """the env's own state after a reset (finite, inside the limits), with distinctive episode words everywhere and non-finite
    target and episode words in the first and the last env"""
    w = words(env).copy()
    w[23] = 0x00ABC000 + 3 * np.arange(n, dtype=np.uint32)
    for j, e in enumerate(sorted({0, n - 1})):
        w[18 + j, e] = (NAN1, NINF)[j]
        w[23, e] = (NAN2, 0xFFFFFFFF)[j]
    return w


@pytest.mark.parametrize("mode", ["kinematic", "dynamic"])
@pytest.mark.parametrize("n", SMALL)
def test_set_state_get_state_round_trip_is_bit_exact(n, mode):
    env = _env(n, mode)
    env.reset()
    w = _distinct_words(n)
    env.set_state(_state_tensor(w))
    got = words(env)
    for k in range(24):
        assert np.array_equal(got[k], w[k]), f"word {k} did not come back"
    env.close()


def _check_hot_words(got, orc):
    ow = orc.state_words()
    assert np.array_equal(got[:18], ow[:18]), "a, v, r must be bit-exact"
    assert np.array_equal(got[22], ow[22]), "step_index must match"
    pot, opot = got[21].view(np.float32).astype(np.float64), ow[21].view(np.float32).astype(np.float64)
    assert np.array_equal(np.isnan(pot), np.isnan(opot))         # (a non-finite target makes the potential NaN in both)
    fin = ~np.isnan(opot)
    if fin.any():
        assert np.abs(pot[fin] - opot[fin]).max() <= POT_TOL


def _survive(n, rollout):
    env, orc = make_pair(n, seed=5, auto_reset=False, max_steps=0)
    env.reset()
    w = _state_with_odd_cold_words(env, n)
    env.set_state(_state_tensor(w))
    orc.load_state_words(w)
    rng = np.random.RandomState(n)
    acts = (rng.uniform(-1, 1, size=(3, n, 6)) * env.a_max).astype(np.float32)
    if rollout:
        env.rollout(torch.from_numpy(acts).cuda())
    for t in range(3):
        if not rollout:
            env.vector_step(torch.from_numpy(acts[t]).cuda())
        orc.step(acts[t], want_obs=False)
    got = words(env)
    for k in (18, 19, 20, 23):
        assert np.array_equal(got[k], w[k]), f"cold word {k} changed"
    _check_hot_words(got, orc)
    env.close()


@pytest.mark.parametrize("n", SMALL)
def test_cold_words_survive_three_steps_without_a_reset(n):
    _survive(n, rollout=False)


def test_cold_words_survive_a_rollout_of_three_steps_in_the_general_form():
    _survive(33, rollout=True)


@pytest.mark.parametrize("n", [33])
def test_cold_words_survive_three_steps_in_dynamics_mode(n):
    env = _env(n, "dynamic")
    env.reset()
    w = _state_with_odd_cold_words(env, n)
    env.set_state(_state_tensor(w))
    rng = np.random.RandomState(n)
    for t in range(3):
        env.vector_step(torch.from_numpy((rng.uniform(-1, 1, size=(n, 6)) * env.a_max).astype(np.float32)).cuda())
    got = words(env)
    for k in (18, 19, 20, 23):
        assert np.array_equal(got[k], w[k]), f"cold word {k} changed"
    assert np.all(got[22] == w[22] + 3)
    env.close()


@pytest.mark.parametrize("n,offset", [(33, 1000), (32800, 77), (32768, 0)])
def test_cold_words_are_rewritten_by_the_reset_inside_a_step(n, offset):
    from oracle import COracle
    from oracle.binding import ORC_DEV
    env = _env(n, seed=11, auto_reset=True, max_steps=2, env_id_offset=offset)
    orc = COracle(n, seed=11, precision=ORC_DEV, auto_reset=True, max_episode_steps=2, env_id_offset=offset, nthreads=8)
    env.reset(); orc.reset(want_obs=False)
    before = words(env).copy()
    assert np.all(before[23] == 1)
    rng = np.random.RandomState(n)
    cut, never_done = np.zeros(n, dtype=np.int64), np.ones(n, dtype=bool)
    for t in range(3):
        act = (rng.uniform(-1, 1, size=(n, 6)) * env.a_max).astype(np.float32)
        obs, rew, done, trunc = env.vector_step(torch.from_numpy(act).cuda())
        oobs, orew, odone, otrunc = orc.step(act, want_obs=False)
        assert np.array_equal(done.cpu().numpy(), odone) and np.array_equal(trunc.cpu().numpy(), otrunc)
        cut += trunc.cpu().numpy()
        never_done &= odone == 0
    got = words(env)
    # an env that never came within done_distance was truncated exactly once, by the second step: one new episode, a new target
    assert never_done.mean() > 0.99 and np.all(cut[never_done] == 1)
    assert np.all(got[23][never_done] == 2)
    assert np.all((got[18:21] != before[18:21]).any(axis=0)[never_done]), "a reset draws a new target"
    check_state_exact(env, orc)           # target, r (and a, v), step_index, episode: the oracle's bits; potential to POT_TOL
    env.close()


def test_link_state_ray_and_ik_kernels_read_joints_and_target_from_the_record():
    n = 65
    env = _env(n, seed=2)
    env.reset()
    w = words(env).copy()
    f = w.view(np.float32)
    rng = np.random.RandomState(4)
    q = (rng.uniform(-0.9, 0.9, size=(n, 6)) * env.r_hi).astype(np.float32)
    qd = rng.uniform(-0.5, 0.5, size=(n, 6)).astype(np.float32)
    tgt = (np.array((15.0, -8.0, 2.0)) + np.array((7.0, 16.0, 4.0)) * rng.random((n, 3))).astype(np.float32)
    f[12:18], f[6:12], f[18:21] = q.T, qd.T, tgt.T
    env.set_state(_state_tensor(w))
    js = torch.from_numpy(np.concatenate([q, qd], axis=1)).cuda()
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t  # noqa: E731

    assert torch.equal(bits(env.link_states()), bits(env.link_states(js)))

    # rays from above the workspace down through each env's own target and through the arm: the target sphere is read from the record
    rays = np.zeros((n, 4, 6), dtype=np.float32)
    rays[:, 0, 0:3] = tgt + (0.0, 0.0, 30.0); rays[:, 0, 3:6] = tgt - (0.0, 0.0, 30.0)
    rays[:, 1, 0:3] = tgt + (30.0, 0.0, 0.0); rays[:, 1, 3:6] = tgt - (30.0, 0.0, 0.0)
    rays[:, 2] = (0.0, 0.0, 40.0, 0.0, 0.0, -5.0)
    rays[:, 3] = (40.0, 0.0, 2.0, -5.0, 0.0, 2.0)
    rays_d = torch.from_numpy(rays).cuda()
    own = env.ray_test(rays_d, hit_arm=True, hit_target=True, hit_bodies=False)["hits"]
    buf = env.ray_test(rays_d, hit_arm=True, hit_target=True, hit_bodies=False, joint_state=js)["hits"]
    assert torch.equal(bits(own), bits(buf))
    hit = own.cpu().numpy()
    from pioneer_amd import _lib
    on_target = hit[:, 0:2, 7] == _lib.SEG_TARGET
    assert on_target.mean() > 0.5, "the rays aimed at each env's own target find it (unless the arm is in the way)"

    q_own = env.solve_ik(None, torch.from_numpy(0.3 * q).cuda(), max_iterations=6)
    q_arg = env.solve_ik(torch.from_numpy(tgt).cuda(), torch.from_numpy(0.3 * q).cuda(), max_iterations=6)
    for a, b in zip(q_own, q_arg):
        assert torch.equal(bits(a), bits(b))
    env.close()
