"""step_kernel (pnr_env_kernels.h) at the sizes where pnr_step runs its row-pass instantiation, against the CPU oracle.

The parity tests of tests/test_gpu_parity.py run at n <= 4 096 and at 65 536 envs; `step_kernel<.., ONE_PASS, ROW_PASS>` — one-pass
form, env-major observations, 32 768 < n <= 65 536 (step_row_pass, pnr_api.hip) — is what bench.py's headline launches, and its
integrator (integrate_joints3, pnr_device.h: the lane's three joints side by side, one branch on "some joint saturates", the
quotients and the clip as selects) is shared with every other step_kernel form.  The cases drive that block every way it can go:
all lanes of a wave saturating, exactly one, none, non-finite and oversized actions.  Checks, tolerances and the oracle
(ORC_DEV) are those of tests/test_gpu_parity.py.

Sizes: 32 800 = 1 025 tiles, the smallest batch on the row pass; 32 823: a ragged last tile of 23 envs (the scalar tail of the
flush); 33 and 4 096: the one-pass form without the row pass; 65 568: the general form, one tile past the one-pass cap; and
pnr_rollout with T = 2 at 64 envs: the general form's t loop.

Not included: an action of exactly -eps (a zero divisor in the saturation quotient).  The default eps is 1e-5, and float32(-1e-5)
is -9.99999974737875e-06: not representable, so no float32 action reaches that divisor.
"""
import numpy as np
import pytest
import torch

import bars
from gpu_support import check_state_exact, make_pair, run_parity

pytestmark = pytest.mark.gpu

ROW_SIZES = [32800, 32823]
ONE_PASS_SIZES = [33, 4096]
GENERAL_SIZE = 65568


def _step_both(env, orc, act, check_obs=True):
    obs, rew, done, trunc = env.vector_step(torch.from_numpy(act).cuda())
    oobs, orew, odone, otrunc = orc.step(act, want_obs=check_obs)
    assert np.array_equal(done.cpu().numpy(), odone) and np.array_equal(trunc.cpu().numpy(), otrunc)
    assert np.abs(rew.double().cpu().numpy() - orew).max() <= bars.REW_TOL
    if check_obs:
        bars.check_obs(obs.double().cpu().numpy(), oobs)


@pytest.mark.parametrize("n", ROW_SIZES + ONE_PASS_SIZES + [GENERAL_SIZE])
def test_random_actions_across_truncation_resets(n):
    """Eight steps of random actions with max_episode_steps = 5: the truncation resets land in the middle of the run; every
    step's outputs are checked and the state is bit-exact at the end."""
    run_parity(n, 8, max_steps=5)


@pytest.mark.parametrize("n", ROW_SIZES + [GENERAL_SIZE])
def test_unclipped_actions_at_five_times_a_max(n):
    run_parity(n, 8, action_scale=5.0, max_steps=0, auto_reset=False)


@pytest.mark.parametrize("n", ROW_SIZES + ONE_PASS_SIZES + [GENERAL_SIZE])
def test_constant_sign_actions_saturate_every_joint_into_its_limit(n):
    """Thirty steps of +-a_max (the sign alternates from env to env, so the two halves of a wave saturate at opposite bounds): every
    lane takes the saturation block in every joint, then every joint is parked at a limit."""
    env, orc = make_pair(n, seed=1, auto_reset=False, max_steps=0)
    env.reset(); orc.reset(want_obs=False)
    sign = np.where(np.arange(n)[:, None] % 2 == 0, 1.0, -1.0) * np.ones((1, 6))
    act = (sign * env.a_max).astype(np.float32)
    for t in range(30):
        _step_both(env, orc, act, check_obs=(t % 6 == 5 or t < 6))
    st = env.state_dict()
    assert np.all((st["r"] == env.r_hi) | (st["r"] == env.r_lo)), "every joint must be parked at a limit"
    check_state_exact(env, orc)
    env.close()


@pytest.mark.parametrize("n", ROW_SIZES + [ONE_PASS_SIZES[0], GENERAL_SIZE])
def test_one_saturating_env_per_wave_and_none(n):
    """Exactly one env of every 32 (one lane pair of each wave; a different pair from tile to tile) gets a_max, the rest zero
    action from rest: one pair of a wave takes the saturation block, the quotients of the other lanes are computed and dropped.
    Then the same with all-zero actions: no lane saturates and the block is skipped."""
    for some in (True, False):
        env, orc = make_pair(n, seed=2, auto_reset=False, max_steps=0)
        env.reset(); orc.reset(want_obs=False)
        e = np.arange(n)
        pick = some & ((e % 32) == (e // 32) % 32)
        act = np.where(pick[:, None], env.a_max[None, :], 0.0).astype(np.float32)
        for t in range(6):                 # v reaches v_max in the third integrated step (v_max / (a_max dt) = 2.4)
            _step_both(env, orc, act)
        st = env.state_dict()
        # a picked env's joints run at v_max (or sit at the upper limit they ran into); nobody else has moved
        assert np.all((st["v"][pick] == env.v_max) | (st["r"][pick] == env.r_hi))
        assert np.all(st["v"][~pick] == 0.0)
        check_state_exact(env, orc)
        env.close()


@pytest.mark.parametrize("n", ROW_SIZES + [ONE_PASS_SIZES[0], GENERAL_SIZE])
def test_non_finite_actions_propagate_as_in_the_oracle(n):
    """auto_reset = False; a few envs (in the first, a middle and the ragged last tile) are given NaN, +inf and -inf actions among
    random ones, in some joints or in all of them: a, v, r words equal the oracle's, so a NaN passes through the predictor, the
    clip and the limits exactly as NumPy lets it."""
    env, orc = make_pair(n, seed=4, auto_reset=False, max_steps=0)
    env.reset(); orc.reset(want_obs=False)
    rng = np.random.RandomState(8)
    for t in range(4):
        act = (rng.uniform(-1, 1, size=(n, 6)) * env.a_max).astype(np.float32)
        for k, e in enumerate((0, 1, 2, 5, n // 2, n // 2 + 7, n - 3, n - 2, n - 1)):
            bad = (np.nan, np.inf, -np.inf)[k % 3]
            if k < 6:
                act[e, :] = bad
            else:
                act[e, (k + t) % 6] = bad
        env.vector_step(torch.from_numpy(act).cuda())
        orc.step(act, want_obs=False)
        w = env.get_state().cpu().numpy().view(np.uint32)
        assert np.array_equal(w[:18], orc.state_words()[:18]), f"a, v, r words differ at step {t}"
    assert np.isnan(w[6:18, 0].view(np.float32)).all() and np.isinf(w[0:6, 1].view(np.float32)).all()
    env.close()


def test_rollout_of_two_steps_in_the_general_form():
    """pnr_rollout with T = 2 at 64 envs: the general form's t loop, against the oracle stepped twice; saturating actions on half
    of the envs."""
    n, T = 64, 2
    env, orc = make_pair(n, seed=6, auto_reset=True, max_steps=3)
    bars.check_obs(env.reset().double().cpu().numpy(), orc.reset())
    rng = np.random.RandomState(1)
    for launch in range(3):
        acts = (rng.uniform(-1, 1, size=(T, n, 6)) * env.a_max).astype(np.float32)
        acts[:, ::2] = np.sign(acts[:, ::2]) * env.a_max
        obs, rew, done, trunc = env.rollout(torch.from_numpy(acts).cuda())
        for t in range(T):
            oobs, orew, odone, otrunc = orc.step(acts[t])
            assert np.array_equal(done[t].cpu().numpy(), odone) and np.array_equal(trunc[t].cpu().numpy(), otrunc)
            assert np.abs(rew[t].double().cpu().numpy() - orew).max() <= bars.REW_TOL
            bars.check_obs(obs[t].double().cpu().numpy(), oobs)
    check_state_exact(env, orc)
    env.close()
