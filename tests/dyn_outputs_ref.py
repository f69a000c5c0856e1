"""Helpers of tests/test_gpu_dynamics_outputs.py and tests/test_dyn_outputs_ref_cpu.py: a float64 statement of the dynamics
kernels' PHASE B alone, and one checker for everything a step returns.

The dynamics kernels work in two phases: phase A (dyn_core) integrates the command state and runs the sub-steps, phase B
(dyn_finish_tile) turns the simulated q, qd into reward, done, truncated, info and the 137-float row.  The dynamics oracle loops
`d->frame_skip` sub-steps while the command integrator's dt comes from `p->frame_skip`, so a DynOracle built with
dyn={"frame_skip": 0} integrates the command state, runs NO sub-step and evaluates reward / done / truncated / info / row at
whatever q, qd it was loaded with.  Loaded with the engine's pre-step state words and the engine's own post-step q, qd it states
phase B alone: the integration error of phase A (Q_TOL) drops out and the kinematic suite's tight tolerances apply to all 137
columns, the reward and the flags (tests/test_dyn_outputs_ref_cpu.py proves the identity on the oracle itself).
"""
import numpy as np

from bars import POS_IDX, POS_TOL, REW_TOL, TRIG_IDX, check_obs
from oracle import DynOracle
from oracle.binding import ORC_DEV

TILE = 32            # a workgroup of the dynamics kernels owns 64 envs and finishes them as two 32-env tiles


def full_oracle(n, seed=0, auto_reset=False, max_episode_steps=0, dyn=None, **tunables):
    """The dynamics oracle as the GPU tests build it (ORC_DEV storage model, 8 threads)."""
    return DynOracle(n, seed=seed, precision=ORC_DEV, auto_reset=auto_reset, max_episode_steps=max_episode_steps, nthreads=8,
                     dyn=dict(dyn or {}), **tunables)


def phase_b_oracle(n, seed=0, auto_reset=False, max_episode_steps=0, dyn=None, **tunables):
    """The same oracle with zero sub-steps: command integration, then reward / flags / info / row at the loaded q, qd."""
    return full_oracle(n, seed=seed, auto_reset=auto_reset, max_episode_steps=max_episode_steps,
                       dyn=dict(dyn or {}, frame_skip=0), **tunables)


def targets_near(orc, jp, lo, hi, rng):
    """float32 targets at distance U(lo, hi) from the pointer at joints jp [n, 6], in a random direction."""
    ptr = orc.fk(np.asarray(jp, dtype=np.float64))
    u = rng.normal(size=ptr.shape)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (ptr + u * rng.uniform(lo, hi, size=(ptr.shape[0], 1))).astype(np.float32)


def check_outputs(got, want, award_done=5.0):
    """got / want: (row [n, 137], reward [n], done [n], truncated [n], info [n, 4] or None) of one step, float64 / uint8 arrays,
    rows env-major.  The row through check_obs (exact linear columns, TRIG_TOL, POS_TOL, POT_TOL), the flags equal for EVERY
    env, the reward within REW_TOL, info's reward terms within REW_TOL and its distance within POS_TOL, and the success award
    exactly `award_done` where done and 0 elsewhere.  A rollout returns no info: pass None on both sides."""
    g_obs, g_rew, g_done, g_trunc, g_info = got
    w_obs, w_rew, w_done, w_trunc, w_info = want
    g_done, w_done = np.asarray(g_done), np.asarray(w_done)
    if g_done.size == 0:
        return
    assert np.array_equal(g_done, w_done), "done must be equal for every env"
    assert np.array_equal(np.asarray(g_trunc), np.asarray(w_trunc)), "truncated must be equal for every env"
    check_obs(np.asarray(g_obs, dtype=np.float64), np.asarray(w_obs, dtype=np.float64))
    assert np.abs(np.asarray(g_rew, dtype=np.float64) - w_rew).max() <= REW_TOL, "reward"
    assert (g_info is None) == (w_info is None)
    if g_info is not None:
        gi = np.asarray(g_info, dtype=np.float64)
        assert np.abs(gi[:, :3] - w_info[:, :3]).max() <= REW_TOL, "info: reward terms"
        assert np.abs(gi[:, 3] - w_info[:, 3]).max() <= POS_TOL, "info: distance"
        assert np.array_equal(gi[:, 2], float(np.float32(award_done)) * g_done.astype(np.float64)), "info: award_done * done"


def worst_outputs(got, want):
    """The measured worst deviations behind check_outputs, for the margins file (never part of a verdict)."""
    g_obs, g_rew, _, _, g_info = got
    w_obs, w_rew, _, _, w_info = want
    if len(np.asarray(g_rew)) == 0:
        return {}
    g_obs = np.asarray(g_obs, dtype=np.float64)
    fig = {"trig": float(np.abs(g_obs[:, TRIG_IDX] - w_obs[:, TRIG_IDX]).max()),
           "pos": float(np.abs(g_obs[:, POS_IDX] - w_obs[:, POS_IDX]).max()),
           "pot": float(np.abs(g_obs[:, 136] - w_obs[:, 136]).max()),
           "rew": float(np.abs(np.asarray(g_rew, dtype=np.float64) - w_rew).max())}
    if g_info is not None:
        gi = np.asarray(g_info, dtype=np.float64)
        fig["info_rew"] = float(np.abs(gi[:, :3] - w_info[:, :3]).max())
        fig["info_dist"] = float(np.abs(gi[:, 3] - w_info[:, 3]).max())
    return fig


def merge_worst(acc, fig):
    for k, v in fig.items():
        acc[k] = max(acc.get(k, 0.0), v)
    return acc
