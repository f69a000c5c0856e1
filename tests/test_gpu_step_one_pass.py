"""The two forms of step_kernel (pnr_env_kernels.h) against each other and against the CPU oracle.

pnr_step at n <= 65 536 envs runs the ONE-PASS instantiation (a wave = one tile, one step); pnr_rollout and larger batches run
the general form (persistent tile loop, next-tile / next-step prefetch).  The rule is `step_one_pass` in pnr_api.hip.  Both
are instantiations of one body, so whatever they both compute must be identical bit for bit; the tolerances against the
float64 oracle are those of tests/test_gpu_parity.py.
"""
import numpy as np
import pytest
import torch

from gpu_support import make_pair, run_parity

pytestmark = pytest.mark.gpu

ONE_PASS_MAX = 65536        # 2 048 tiles of 32 envs: the single-step grid cap


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("layout", ["env_major", "feature_major"])
def test_general_and_one_pass_kernels_agree_at_the_selection_boundary(layout):
    """65 536 + 40 envs as ONE handle are 2 050 tiles: the general kernel, four waves walk two tiles each, the last tile is
    ragged.  The same envs as two handles [0, 65 536) and [65 536, 65 576) both run the one-pass kernel (the second: a full tile
    and a ragged one of 8 envs).  Same seed, same actions, 3 steps with max_episode_steps = 2, so step 2 truncates and auto-resets
    every env: obs, reward, done, truncated and the state are equal after every step."""
    from pioneer_amd import PioneerVectorEnv, EngineConfig
    n_lo, n_hi = ONE_PASS_MAX, 40
    n = n_lo + n_hi
    fm = layout == "feature_major"
    eng = dict(auto_reset=True, max_episode_steps=2, obs_layout=layout, action_layout=layout)
    one = PioneerVectorEnv(n, device="cuda:0", seed=13, engine_config=EngineConfig(**eng))
    lo = PioneerVectorEnv(n_lo, device="cuda:0", seed=13, env_id_offset=0, engine_config=EngineConfig(**eng))
    hi = PioneerVectorEnv(n_hi, device="cuda:0", seed=13, env_id_offset=n_lo, engine_config=EngineConfig(**eng))
    env_dim = 1 if fm else 0                      # feature-major batches are [features, envs]

    def join(a, b, dim):
        return np.concatenate([_np(a), _np(b)], axis=dim)

    assert np.array_equal(_np(one.reset()), join(lo.reset(), hi.reset(), env_dim))
    g = torch.Generator(device="cpu").manual_seed(6)
    amax = torch.from_numpy(one.a_max)
    n_trunc = 0
    for t in range(3):
        act = (torch.rand(n, 6, generator=g) * 2 - 1) * amax                # [n, 6]
        a_one, a_lo, a_hi = ((x.T.contiguous() if fm else x.contiguous()).cuda() for x in (act, act[:n_lo], act[n_lo:]))
        o, r, d, tr = one.vector_step(a_one)
        ol, rl, dl, tl = lo.vector_step(a_lo)
        oh, rh, dh, th = hi.vector_step(a_hi)
        assert np.array_equal(_np(o), join(ol, oh, env_dim)), f"obs differ at step {t}"
        assert np.array_equal(_np(r), join(rl, rh, 0)), f"rewards differ at step {t}"
        assert np.array_equal(_np(d), join(dl, dh, 0)) and np.array_equal(_np(tr), join(tl, th, 0)), f"flags differ at step {t}"
        assert np.array_equal(_np(one.get_state()), join(lo.get_state(), hi.get_state(), 1)), f"state differs at step {t}"
        n_trunc += int(tr.sum())
    assert n_trunc > n // 2                       # step 2 cut (and re-drew) every env that had not finished at step 1
    for e in (one, lo, hi):
        e.close()


@pytest.mark.parametrize("n", [1, 31, 33, ONE_PASS_MAX - 5])
def test_ragged_sizes_through_the_one_pass_kernel_against_the_oracle(n):
    """A single pair, a tile one env short, one env over a tile, and the largest grid with a ragged last tile: two steps with
    an auto-reset of every env in between (max_episode_steps = 1), both layouts."""
    run_parity(n, 2, "env_major", "env_major", max_steps=1)
    run_parity(n, 2, "feature_major", "feature_major", max_steps=1)


@pytest.mark.parametrize("layout", ["env_major", "feature_major"])
def test_rollout_in_one_general_launch_equals_one_pass_steps(layout):
    """test_rollout_equals_steps across the two kernels at a ragged size: pnr_rollout(T = 2) at 96 + 5 envs is one launch of the
    general form, two pnr_step calls (info requested) are two launches of the one-pass form; every env is truncated and
    re-drawn at each step."""
    n, T = 96 + 5, 2
    env1, _ = make_pair(n, seed=9, layout=layout, max_steps=1)
    env2, _ = make_pair(n, seed=9, layout=layout, max_steps=1)
    assert torch.equal(env1.reset(), env2.reset())
    g = torch.Generator(device="cpu").manual_seed(2)
    acts = ((torch.rand(T, n, 6, generator=g) * 2 - 1) * torch.from_numpy(env1.a_max)).cuda()
    obs_r, rew_r, done_r, trunc_r = env1.rollout(acts)
    for t in range(T):
        obs, rew, done, trunc, info = env2.vector_step(acts[t], want_info=True)
        assert torch.equal(obs, obs_r[t]) and torch.equal(rew, rew_r[t])
        assert torch.equal(done, done_r[t]) and torch.equal(trunc, trunc_r[t])
        assert torch.equal((info[:, 0] + info[:, 1]) + info[:, 2], rew)     # the info rows are this step's (pioneer_knm_env.py:165)
    assert bool(((done_r | trunc_r) == 1).all())
    assert torch.equal(env1.get_state(), env2.get_state())
    env1.close(); env2.close()
