"""The reference of tests/test_gpu_dynamics_outputs.py, checked on the CPU oracle alone.

1. The zero-sub-step oracle (dyn_outputs_ref.phase_b_oracle) IS the full oracle's phase B: fed with the full oracle's pre-step
   state words and post-step dyn words it returns row, reward, done, truncated and info bit for bit; so it does when it runs
   unsynced over a chain of steps and is fed nothing but columns 0:6 and 90:96 of each row (all that a rollout launch returns).
2. dyn_outputs_ref.check_outputs bites: each of the bugs that the GPU tests are there to catch, applied to the full oracle's own
   outputs one at a time, makes it raise.
"""
import numpy as np
import pytest

from dyn_outputs_ref import TILE, check_outputs, full_oracle, phase_b_oracle, targets_near
from oracle_cases import load_states

N, STEPS = 256, 10


def _scenario(done_distance, seed=5, n=N):
    """Gravity, randomised parameters, TimeLimit at 3 steps (no auto-reset: it fires from step 3 on), `done` on a large share."""
    kw = dict(seed=seed, auto_reset=False, max_episode_steps=3, dyn=dict(gravity=9.81, randomize=1), done_distance=done_distance)
    full, pb = full_oracle(n, **kw), phase_b_oracle(n, **kw)
    rng = np.random.RandomState(seed)
    jp = rng.uniform(full.r_lo, full.r_hi, size=(n, 6)).astype(np.float32)
    tp = targets_near(full, jp, 0.5 * done_distance, 1.5 * done_distance, rng)
    for o in (full, pb):
        o.reset(joint_pos=jp.astype(np.float64), target_pos=tp.astype(np.float64))
    acts = (rng.uniform(-0.3, 0.3, (STEPS, n, 6)) * full.a_max).astype(np.float32)
    return full, pb, acts


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("done_distance", [6.0, 10.0])
def test_zero_substep_oracle_fed_with_words_is_the_full_oracles_phase_b(oracle_built, done_distance):
    full, pb, acts = _scenario(done_distance)
    n_done = n_trunc = 0
    for t in range(STEPS):
        pre = full.state_words()
        want = full.step(acts[t], want_info=True)
        pb.load_state_words(pre); pb.load_dyn_words(full.dyn_words())
        got = pb.step(acts[t], want_info=True)
        assert _same(got, want), t
        assert np.array_equal(pb.state_words(), full.state_words())
        n_done += int(want[2].sum()); n_trunc += int(want[3].sum())
    assert n_done > 0.2 * N * STEPS and n_trunc > 0.2 * N * (STEPS - 2)      # both flags fire under the comparison


@pytest.mark.parametrize("done_distance", [6.0, 10.0])
def test_zero_substep_oracle_chained_on_row_columns_is_the_full_oracles_phase_b(oracle_built, done_distance):
    full, pb, acts = _scenario(done_distance)
    n_done = n_trunc = 0
    for t in range(STEPS - 1):
        want = full.step(acts[t], want_info=True)
        load_states(pb, want[0][:, 0:6], want[0][:, 90:96])        # never re-synced: only the row's q, qd
        got = pb.step(acts[t], want_info=True)
        assert _same(got, want), t
        n_done += int(want[2].sum()); n_trunc += int(want[3].sum())
    assert np.array_equal(pb.state_words(), full.state_words())
    assert n_done > 0.2 * N * (STEPS - 1) and n_trunc > 0.2 * N * (STEPS - 3)


# ---- the checker bites -----------------------------------------------------------------------------------------------------

def _one_step(t_stop=2):
    """The full oracle's outputs of step `t_stop` (the arm is moving by then) and the command state that produced them."""
    full, _, acts = _scenario(6.0)
    for t in range(t_stop):
        full.step(acts[t])
    pre_pot = full.state["potential"].copy()
    want = full.step(acts[t_stop], want_info=True)
    return full, pre_pot, want


def _copy(out):
    return tuple(np.array(x, copy=True) for x in out)


def test_checker_accepts_the_reference_itself(oracle_built):
    _, _, want = _one_step()
    check_outputs(_copy(want), want)
    check_outputs(_copy(want)[:4] + (None,), want[:4] + (None,))            # a rollout's results: no info


def test_checker_rejects_v_trig_taken_from_the_command_velocity(oracle_built):
    full, _, want = _one_step()
    got = _copy(want)
    v_cmd = full.state["v"].astype(np.float64)
    assert np.abs(v_cmd - want[0][:, 90:96]).max() > 1e-3                   # the simulated qd is not the command v
    got[0][:, 96:102] = np.cos(v_cmd).astype(np.float32); got[0][:, 102:108] = np.sin(v_cmd).astype(np.float32)
    with pytest.raises(AssertionError):
        check_outputs(got, want)


def test_checker_rejects_two_envs_of_a_tile_swapped_in_the_row(oracle_built):
    _, _, want = _one_step()
    got = _copy(want)
    a, b = TILE + 3, TILE + 17                                              # both in the second 32-env tile
    got[0][[a, b]] = got[0][[b, a]]
    with pytest.raises(AssertionError):
        check_outputs(got, want)


def near_threshold_pass(n=N,done_distance=6.0, seed=11):
    """The inputs of the GPU suite's near-threshold test on the oracle alone: pass 1 takes a step and gives the pose it ends in,
    pass 2 repeats it with targets at done_distance + U(-2e-5, 2e-5) from that pose."""
    kw = dict(seed=seed, auto_reset=False, max_episode_steps=0, dyn=dict(gravity=9.81), done_distance=done_distance)
    rng = np.random.RandomState(seed)
    one, two = full_oracle(n, **kw), full_oracle(n, **kw)
    jp = rng.uniform(one.r_lo, one.r_hi, size=(n, 6)).astype(np.float32)
    act = (rng.uniform(-0.3, 0.3, (n, 6)) * one.a_max).astype(np.float32)
    one.reset(joint_pos=jp.astype(np.float64), target_pos=targets_near(one, jp, 3.0, 9.0, rng).astype(np.float64))
    one.step(act); one.step(act)
    tp = targets_near(one, one.dstate["q"], done_distance - 2e-5, done_distance + 2e-5, rng)
    two.reset(joint_pos=jp.astype(np.float64), target_pos=tp.astype(np.float64))
    two.step(act)
    want = two.step(act, want_info=True)
    assert np.array_equal(two.dstate["q"], one.dstate["q"])                 # the targets do not enter the motion
    return want


def test_checker_rejects_done_from_the_float32_distance(oracle_built):
    want = near_threshold_pass()
    assert np.abs(want[4][:, 3] - 6.0).max() < 3e-5 and 0.25 < want[2].mean() < 0.75
    got = _copy(want)
    ptr, tgt = want[0][:, 126:129].astype(np.float32), want[0][:, 129:132].astype(np.float32)
    d = tgt - ptr
    dist32 = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2], dtype=np.float32)
    got[2][:] = dist32 < np.float32(6.0)
    assert (got[2] != want[2]).sum() > 0                                    # float32 decides some of these envs differently
    with pytest.raises(AssertionError):
        check_outputs(got, want)


def test_checker_rejects_a_reward_formed_with_the_post_step_potential(oracle_built):
    _, pre_pot, want = _one_step()
    got = _copy(want)
    post_pot = want[0][:, 136]
    assert np.abs(post_pot - pre_pot).max() > 1e-2
    got[1][:] = want[1] - (post_pot - pre_pot)                              # pot - pot instead of pot - old_potential
    with pytest.raises(AssertionError):
        check_outputs(got, want)


@pytest.mark.parametrize("col", range(126, 136))
def test_checker_rejects_a_pointer_target_or_distance_column_off_by_1e_4(oracle_built, col):
    _, _, want = _one_step()
    got = _copy(want)
    got[0][5, col] += 1e-4
    with pytest.raises(AssertionError):
        check_outputs(got, want)
