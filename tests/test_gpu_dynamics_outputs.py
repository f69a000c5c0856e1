"""Dynamics mode's whole output: every one of the 137 columns, the reward, done, truncated and info of dyn_step_kernel and
dyn_rollout_kernel in all 2 x 32 instantiations <OBS_EM, ACT_EM, RAND, PHYS 0..3>, success-driven auto-reset, and joint stops.

tests/test_gpu_dynamics.py compares phase A (the sub-steps: q, qd) with the float64 dynamics oracle at Q_TOL / QD_TOL.  This file
adds phase B (dyn_finish_tile: reward, done with its float64 re-evaluation, TimeLimit, auto-reset, the row) against the
zero-sub-step oracle of tests/dyn_outputs_ref.py, which is loaded with the engine's OWN post-step q, qd: phase A's integration
error drops out and the kinematic suite's tolerances (tests/bars.py: exact linear columns, TRIG_TOL, POS_TOL, POT_TOL,
REW_TOL, flags equal for every env) hold for every env.  Parity unpinned, like all of dynamics mode.

Shared setup: gravity 9.81 and done_distance = 6.0, reset with explicit joints (uniform inside the limits) and targets 3 .. 9
away from the pointer in a random direction, so that about half of the envs are `done` at the first step (asserted 20 % .. 80 %
on the oracle's side) and the award_done term, the success reset and the rollout kernel's reset note are under comparison.

Instantiations, derived from the parameters (O = obs env-major, A = actions env-major, R = randomize, PHYS = contacts | 2 x
inertia-scaled motor): test 1 launches dyn_step_kernel<O, A, R, P> and test 3 dyn_rollout_kernel<O, A, R, P> (and its twin
dyn_step_kernel<O, A, R, P>) for every (O, A, R, P) in {0, 1}^3 x {0, 1, 2, 3}, one parameter case each; test 2 both kernels
<0|1, 1, 0, 0>; test 4 both kernels <1, 0|1, 1, 0>; test 5 both kernels <1, 1, 1, 0> (pnr_set_dyn_state selects RAND).

Every test writes its measured worst deviations to dyn_outputs_margins.json, next to the dynamics tests' margins (the
_record_margin of tests/test_gpu_dynamics.py); never part of a verdict.  Measured on
an MI355X (worst over all cases of a test): phase B trig 1.2e-7 (TRIG_TOL 4e-7), pointer / diff / distance 5.6e-6 (POS_TOL 3e-5),
potential 2.3e-5 (POT_TOL 1e-4), reward 3.3e-5 (REW_TOL 2e-4); phase A |dq| 7.2e-7, |dqd| 2.0e-5 (Q_TOL 5e-5, QD_TOL 2e-3) with no env
outside them, contacts and joint stops included; rollout against steps 7.6e-6 (ROLL tolerances 2e-3), bit-identical with RAND.
Exempt: 3 of 8 192 env-steps of the success-reset step test (0.04 %, cap 0.5 %), none anywhere else.  `done` at the first step
44 % .. 65 % of the envs; 49 % .. 50 % inside the threshold's noise, where float32 alone would flip 30 (step) / 38 (rollout) of
2 048 envs; 44 % of the envs (8.4 % .. 8.8 % of the joints) parked after the joint-stop step.
"""
import numpy as np
import pytest
import torch

from bars import POS_TOL, POT_TOL, PTR_TOL, Q_TOL, QD_TOL, REW_TOL, ROLL_OBS_TOL, ROLL_REW_TOL, TRIG_TOL
from dyn_outputs_ref import check_outputs, full_oracle, merge_worst, phase_b_oracle, targets_near, worst_outputs
from gpu_support import dyn_words, engine_config_from_oracle_names, words
from oracle_cases import load_states
from test_gpu_dynamics import _record_margin

pytestmark = pytest.mark.gpu

DONE_DISTANCE, AWARD_DONE = 6.0, 5.0
PHYS = {
    0: dict(),
    1: dict(ground_z=8.0),
    2: dict(pd_inertia_scaled=1, kp=400.0, kd=40.0),
    3: dict(pd_inertia_scaled=1, kp=400.0, kd=40.0, ground_z=8.0),
}
MARGINS = "dyn_outputs_margins.json"


def record(case, figures):
    _record_margin(case, None, None, file=MARGINS, figures=figures)


def make_env(n, seed, layout="env_major", act_layout="env_major", auto_reset=False, max_steps=3, done_distance=DONE_DISTANCE, **dyn):
    """A dynamics-mode env with gravity 9.81; `dyn` in the oracle's names."""
    from pioneer_amd import PioneerKinematicConfig, PioneerVectorEnv, SimulationConfig
    eng = engine_config_from_oracle_names(dyn, auto_reset=auto_reset, max_episode_steps=max_steps, obs_layout=layout, action_layout=act_layout)
    return PioneerVectorEnv(n, device="cuda:0", seed=seed, pioneer_config=PioneerKinematicConfig(done_distance=done_distance),
                            simulation_config=SimulationConfig(gravity=9.81), engine_config=eng)


def orc_kw(seed, auto_reset=False, max_steps=3, done_distance=DONE_DISTANCE, **dyn):
    return dict(seed=seed, auto_reset=auto_reset, max_episode_steps=max_steps, dyn=dict(dyn, gravity=9.81), done_distance=done_distance)


def rows(env, obs):
    """An obs batch (one step's, or a rollout's [T, ...]) as float64 env-major rows."""
    o = obs.double().cpu().numpy()
    return np.swapaxes(o, -1, -2) if env.feature_major_obs else o


def dev_actions(env, act):
    """Host actions [n, 6] or [T, n, 6] in the env's action layout, on the device."""
    a = np.swapaxes(act, -1, -2) if env.feature_major_act else act
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(*tensors):
    return tuple(None if t is None else t.double().cpu().numpy() if t.dtype.is_floating_point else t.cpu().numpy() for t in tensors)


def start(n, seed, rng_seed, envs, orcs, lo=3.0, hi=9.0):
    """Reset every env and oracle with the same explicit joints and targets U(lo, hi) away from the pointer."""
    rng = np.random.RandomState(rng_seed)
    ref = orcs[0]
    jp = rng.uniform(ref.r_lo, ref.r_hi, size=(n, 6)).astype(np.float32)
    tp = targets_near(ref, jp, lo, hi, rng)
    obs = [e.reset(joint_positions=jp, target_positions=tp) for e in envs]
    oobs = [o.reset(joint_pos=jp.astype(np.float64), target_pos=tp.astype(np.float64)) for o in orcs]
    for e, ob in zip(envs, obs):
        assert np.abs(rows(e, ob) - oobs[0]).max() < POS_TOL
    return rng, jp, tp


def check_state_words(env, orc, sel=slice(None)):
    """Command state, targets and counters equal the oracle's; the potential within POT_TOL.  Returns the potential's deviation."""
    w, ow = words(env)[:, sel], orc.state_words()[:, sel]
    assert np.array_equal(w[:21], ow[:21]) and np.array_equal(w[22:], ow[22:])
    if w.shape[1] == 0:
        return 0.0
    dpot = float(np.abs(w[21].view(np.float32).astype(np.float64) - ow[21].view(np.float32).astype(np.float64)).max())
    assert dpot <= POT_TOL
    return dpot


def phase_a(got_q, got_qd, orc, loose):
    """q, qd [n, 6] against the full oracle's: every env, or (contacts: one-sided springs switch on at depth 0 and an env within
    float32 noise of a surface may take the other branch for a sub-step) tests/test_gpu_dynamics.py's loose rule.  Returns the
    worst deviations (the 99.5 % quantile under the loose rule) and the share of envs outside the tolerance."""
    eq = np.abs(got_q - orc.dstate["q"]).max(1); eqd = np.abs(got_qd - orc.dstate["qd"]).max(1)
    ok = (eq <= Q_TOL) & (eqd <= QD_TOL)
    if loose:
        assert ok.mean() >= 0.995 and eq.max() < 5e-3 and eqd.max() < 0.5, (ok.mean(), eq.max(), eqd.max())
        return float(np.quantile(eq, 0.995)), float(np.quantile(eqd, 0.995)), float(1.0 - ok.mean())
    assert ok.all(), (eq.max(), eqd.max())
    return float(eq.max()), float(eqd.max()), 0.0


CASES = [(o, a, r, p) for o in ("env_major", "feature_major") for a in ("env_major", "feature_major") for r in (0, 1) for p in range(4)]


# ---- 1. every instantiation of dyn_step_kernel: both phases per step -----------------------------------------------------------

@pytest.mark.parametrize("layout,act_layout,randomize,phys", CASES)
def test_step_kernel_every_instantiation_both_phases(layout, act_layout, randomize, phys):
    """dyn_step_kernel<layout, act_layout, randomize, phys>, 5 steps without auto-reset under a 3-step TimeLimit (truncated
    fires from step 3 on), the full oracle re-synced before every step.  Phase A: q, qd against the full oracle.  Phase B: the
    zero-sub-step oracle, loaded with the pre-step state words and the engine's post-step dyn words, through check_outputs for
    EVERY env; then the state words.  n = 1 (one lane), 37 (second tile partial), 129 (a third workgroup with one env) without
    contacts; 1 029 with contacts, where phase A is held to the loose rule."""
    contact = bool(phys & 1)
    dyn = dict(PHYS[phys], randomize=randomize)
    fig = {}
    for n in ((1029,) if contact else (1, 37, 129)):
        env = make_env(n, seed=5, layout=layout, act_layout=act_layout, **dyn)
        full, pb = full_oracle(n, **orc_kw(5, **dyn)), phase_b_oracle(n, **orc_kw(5, **dyn))
        rng, _, _ = start(n, 5, 100 + n, [env], [full, pb])
        for t in range(5):
            act = (rng.uniform(-0.3, 0.3, (n, 6)) * env.a_max).astype(np.float32)
            pre = words(env)
            full.load_state_words(pre); full.load_dyn_words(dyn_words(env))
            obs, rew, done, trunc, info = env.vector_step(dev_actions(env, act), want_info=True)
            full.step(act)
            w = dyn_words(env)
            wq, wqd, out = phase_a(w[0:6].T.astype(np.float64), w[6:12].T.astype(np.float64), full, contact)
            merge_worst(fig, {"dq": wq, "dqd": wqd, "phase_a_outside_share": out})
            pb.load_state_words(pre); pb.load_dyn_words(w)
            want = pb.step(act, want_info=True)
            got = (rows(env, obs),) + host(rew, done, trunc, info)
            merge_worst(fig, worst_outputs(got, want))
            check_outputs(got, want, AWARD_DONE)
            merge_worst(fig, {"state_pot": check_state_words(env, pb)})
            if t == 0 and n >= 37:
                assert 0.2 <= want[2].mean() <= 0.8, want[2].mean()
                fig["done_share_step0_n%d" % n] = float(want[2].mean())
            assert np.array_equal(want[3], (t >= 2) & (want[2] == 0))
        env.close()
    record("step/%s/%s/rand%d/phys%d" % (layout, act_layout, randomize, phys),
           dict(fig, Q_TOL=Q_TOL, QD_TOL=QD_TOL, TRIG_TOL=TRIG_TOL, POS_TOL=POS_TOL, POT_TOL=POT_TOL, REW_TOL=REW_TOL))


# ---- 2. `done` inside float32 noise of the threshold, while the arm moves -------------------------------------------------------

@pytest.mark.parametrize("kernel", ["step", "rollout"])
@pytest.mark.parametrize("layout", ["env_major", "feature_major"])
def test_done_is_exact_inside_float32_noise_of_the_threshold_while_the_arm_moves(layout, kernel):
    """Kinematic mode's test_done_is_bit_exact_inside_float32_noise_of_the_threshold for the dynamics kernels, whose pose is
    the simulated one.  Pass 1 takes the step(s) and gives the pose q the arm ends in; pass 2, a fresh env with the same seed,
    joints and actions (randomize = 0: no draw depends on the episode counter), is reset with targets at
    done_distance + U(-2e-5, 2e-5) from the oracle's pointer at that q — and must repeat pass 1's q bit for bit.  The rollout
    kernel (T = 2) is judged on both steps: the even envs' targets are placed on the pose after its first step, the odd envs'
    on the pose after its second.  Every env's `done` equals the phase-B oracle's; the engine's own float32 distance would have
    decided some of them differently."""
    n, T = 2048, (1 if kernel == "step" else 2)
    kw = orc_kw(7, max_steps=0)
    pb = phase_b_oracle(n, **kw)
    rng = np.random.RandomState(21)
    jp = rng.uniform(pb.r_lo, pb.r_hi, size=(n, 6)).astype(np.float32)
    acts = (rng.uniform(-0.3, 0.3, (T, n, 6)) * pb.a_max).astype(np.float32)

    def run(tp):
        env = make_env(n, seed=7, layout=layout, max_steps=0)
        env.reset(joint_positions=jp, target_positions=tp)
        if kernel == "step":
            obs, rew, done, trunc, info = env.vector_step(dev_actions(env, acts[0]), want_info=True)
            w = dyn_words(env)
            o = rows(env, obs)[None]
            assert np.array_equal(o[0][:, 0:6], w[0:6].T.astype(np.float64)) and np.array_equal(o[0][:, 90:96], w[6:12].T.astype(np.float64))
            res = o, host(rew)[0][None], host(done)[0][None], host(trunc)[0][None], host(info)[0][:, 3].astype(np.float32)[None]
        else:
            obs, rew, done, trunc = env.rollout(dev_actions(env, acts))
            o = rows(env, obs)
            res = (o,) + host(rew, done, trunc) + (o[:, :, 135].astype(np.float32),)
        env.close()
        return res

    one = run(targets_near(pb, jp, 3.0, 9.0, rng))
    judged = np.zeros(n, dtype=np.int64) if T == 1 else (np.arange(n) % 2)          # the step at which an env sits on the threshold
    q_at = one[0][judged, np.arange(n), 0:6]
    tp = targets_near(pb, q_at, DONE_DISTANCE - 2e-5, DONE_DISTANCE + 2e-5, rng)
    two = run(tp)
    assert np.array_equal(two[0][:, :, 0:6], one[0][:, :, 0:6]) and np.array_equal(two[0][:, :, 90:96], one[0][:, :, 90:96])

    pb.reset(joint_pos=jp.astype(np.float64), target_pos=tp.astype(np.float64))
    fig, flips, near_done = {}, 0, np.zeros(n, dtype=bool)
    for t in range(T):
        load_states(pb, two[0][t][:, 0:6], two[0][t][:, 90:96])
        want = pb.step(acts[t], want_info=True)
        sel = judged == t
        assert np.abs(want[4][sel, 3] - DONE_DISTANCE).max() < 3e-5                 # construction: every env within the noise
        near_done[sel] = want[2][sel] != 0
        got = (two[0][t], two[1][t], two[2][t], two[3][t], None)
        merge_worst(fig, worst_outputs(got, want[:4] + (None,)))
        check_outputs(got, want[:4] + (None,))                                      # `done` for every env, and the rest of the step
        flips += int(((two[4][t] < np.float32(DONE_DISTANCE)) != (want[2] != 0))[sel].sum())
    assert 0.25 <= near_done.mean() <= 0.75
    assert flips > 0, "the float32 distance alone would have decided some envs wrongly"
    record("near_threshold/%s/%s" % (kernel, layout), dict(fig, done_share=float(near_done.mean()), float32_would_flip=flips, n=n))


# ---- 3. dyn_rollout_kernel, every instantiation: the chain --------------------------------------------------------------------

@pytest.mark.parametrize("layout,act_layout,randomize,phys", CASES)
def test_rollout_kernel_every_instantiation_through_the_chain(layout, act_layout, randomize, phys):
    """dyn_rollout_kernel<layout, act_layout, randomize, phys>, T = 7 in one launch, no auto-reset, 3-step TimeLimit.  Phase B:
    the zero-sub-step oracle runs UNSYNCED next to the launch and is fed nothing but columns 0:6 / 90:96 of each returned row;
    every step's row, reward, done and truncated go through check_outputs (a rollout returns no info), then the state words, and
    the dyn words' q, qd equal the last row's.  Phase A: T pnr_step launches on a twin env, rows and rewards at ROLL_OBS_TOL /
    ROLL_REW_TOL (with contacts tests/test_gpu_dynamics.py's rule for the two separately compiled kernels: all but 1 % of the
    envs to rounding, the rest bounded)."""
    contact = bool(phys & 1)
    dyn = dict(PHYS[phys], randomize=randomize)
    T, fig = 7, {}
    for n in ((1029,) if contact else (1, 37, 129)):
        env = make_env(n, seed=8, layout=layout, act_layout=act_layout, **dyn)
        twin = make_env(n, seed=8, layout=layout, act_layout=act_layout, **dyn)
        pb = phase_b_oracle(n, **orc_kw(8, **dyn))
        rng, _, _ = start(n, 8, 200 + n, [env, twin], [pb])
        acts = (rng.uniform(-0.3, 0.3, (T, n, 6)) * env.a_max).astype(np.float32)
        obs, rew, done, trunc = env.rollout(dev_actions(env, acts))
        o = rows(env, obs); rew, done, trunc = host(rew, done, trunc)
        for t in range(T):
            load_states(pb, o[t][:, 0:6], o[t][:, 90:96])
            want = pb.step(acts[t])
            got = (o[t], rew[t], done[t], trunc[t], None)
            merge_worst(fig, worst_outputs(got, want + (None,)))
            check_outputs(got, want + (None,))
            if t == 0 and n >= 37:
                assert 0.2 <= want[2].mean() <= 0.8, want[2].mean()
                fig["done_share_step0_n%d" % n] = float(want[2].mean())
            assert np.array_equal(want[3], (t >= 2) & (want[2] == 0))
            # phase A of this kernel against the single-step kernel
            to, tr, td, tt = twin.vector_step(dev_actions(twin, acts[t]))
            err = np.abs(rows(twin, to) - o[t]).max(1); rerr = np.abs(host(tr)[0] - rew[t])
            if contact:
                ok = (err <= ROLL_OBS_TOL) & (rerr <= ROLL_REW_TOL)
                assert ok.mean() >= 0.99 and err.max() < 1.0, (t, ok.mean(), err.max())
                merge_worst(fig, {"twin_row": float(np.quantile(err, 0.99)), "twin_rew": float(np.quantile(rerr, 0.99)),
                                  "twin_outside_share": float(1.0 - ok.mean())})
            else:
                assert err.max() <= ROLL_OBS_TOL and rerr.max() <= ROLL_REW_TOL, (t, err.max(), rerr.max())
                merge_worst(fig, {"twin_row": float(err.max()), "twin_rew": float(rerr.max())})
        merge_worst(fig, {"state_pot": check_state_words(env, pb)})
        w = dyn_words(env)
        assert np.array_equal(w[0:6].T.astype(np.float64), o[-1][:, 0:6]) and np.array_equal(w[6:12].T.astype(np.float64), o[-1][:, 90:96])
        assert np.array_equal(words(env)[:21], words(twin)[:21]) and np.array_equal(words(env)[22:], words(twin)[22:])
        env.close(); twin.close()
    record("rollout/%s/%s/rand%d/phys%d" % (layout, act_layout, randomize, phys),
           dict(fig, ROLL_OBS_TOL=ROLL_OBS_TOL, ROLL_REW_TOL=ROLL_REW_TOL, TRIG_TOL=TRIG_TOL, POS_TOL=POS_TOL, POT_TOL=POT_TOL, REW_TOL=REW_TOL))


# ---- 4. success-driven auto-reset ---------------------------------------------------------------------------------------------

EXEMPT_CAP = 0.005


@pytest.mark.parametrize("act_layout", ["env_major", "feature_major"])
@pytest.mark.parametrize("n", [129, 2048])
def test_success_reset_in_the_step_kernel(n, act_layout):
    """auto_reset with randomisation and a 3-step TimeLimit, 4 steps of dyn_step_kernel, the full oracle re-synced before each:
    about half of the envs succeed at the first step and are re-drawn inside the kernel.  The full oracle's pose differs from the
    engine's by up to Q_TOL, so its flags are required of every env whose oracle distance is at least 1e-3 (the pointer
    tolerance) from done_distance; at most 0.5 % of the env-steps may be exempt.  A reset env: state words, dyn words (q = r,
    qd = 0, fresh draws) equal the oracle's, the row is the oracle's fresh row, info's award is award_done where done.  An env
    that was not reset: phase B against the zero-sub-step oracle as in test 1."""
    dyn = dict(randomize=1)
    env = make_env(n, seed=13, act_layout=act_layout, auto_reset=True, **dyn)
    full = full_oracle(n, **orc_kw(13, auto_reset=True, **dyn))
    pb = phase_b_oracle(n, **orc_kw(13, auto_reset=False, **dyn))
    rng, _, _ = start(n, 13, 300 + n, [env], [full, pb])
    fig, exempt_steps, resets, successes = {}, 0, 0, 0
    for t in range(4):
        act = (rng.uniform(-0.3, 0.3, (n, 6)) * env.a_max).astype(np.float32)
        pre, pre_dyn = words(env), dyn_words(env)
        full.load_state_words(pre); full.load_dyn_words(pre_dyn)
        obs, rew, done, trunc, info = env.vector_step(dev_actions(env, act), want_info=True)
        oobs, orew, odone, otrunc, oinfo = full.step(act, want_info=True)
        got = (rows(env, obs),) + host(rew, done, trunc, info)
        exempt = np.abs(oinfo[:, 3] - DONE_DISTANCE) < PTR_TOL
        exempt_steps += int(exempt.sum())
        keep = ~exempt
        assert np.array_equal(got[2][keep], odone[keep]) and np.array_equal(got[3][keep], otrunc[keep])
        was_reset = keep & ((odone | otrunc) != 0)
        stays = keep & ~was_reset
        resets += int(was_reset.sum()); successes += int((keep & (odone != 0)).sum())
        if t == 0 and n >= 37:
            assert 0.2 <= odone.mean() <= 0.8
        # reset envs
        w, wd, ow = words(env), dyn_words(env), full.state_words()
        assert np.array_equal(w[:21, was_reset], ow[:21, was_reset]) and np.array_equal(w[22:, was_reset], ow[22:, was_reset])
        assert np.array_equal(wd[0:35, was_reset], full.dyn_words()[0:35, was_reset])
        if was_reset.any():
            fresh = float(np.abs(got[0][was_reset] - oobs[was_reset]).max())
            assert fresh < POS_TOL
            merge_worst(fig, {"fresh_row": fresh})
        dn = keep & (odone != 0)
        assert np.array_equal(got[4][dn, 2], np.full(int(dn.sum()), AWARD_DONE)) and not got[4][keep & (odone == 0), 2].any()
        # envs that go on: phase B on the engine's own q, qd
        pb.load_state_words(pre); pb.load_dyn_words(wd)
        want = pb.step(act, want_info=True)
        g_s, w_s = tuple(x[stays] for x in got), tuple(x[stays] for x in want)
        merge_worst(fig, worst_outputs(g_s, w_s))
        check_outputs(g_s, w_s, AWARD_DONE)
        merge_worst(fig, {"state_pot": check_state_words(env, pb, stays)})
    share = exempt_steps / (4.0 * n)
    assert share <= EXEMPT_CAP, share
    assert successes >= 0.2 * n and resets > successes                     # successes and TimeLimit cuts both re-drew envs
    env.close()
    record("success_reset/step/n%d/%s" % (n, act_layout), dict(fig, exempt_share=share, cap=EXEMPT_CAP, resets=resets, successes=successes))


@pytest.mark.parametrize("act_layout", ["env_major", "feature_major"])
@pytest.mark.parametrize("n", [129, 2048])
def test_success_reset_in_the_rollout_kernel(n, act_layout):
    """The same episode through dyn_rollout_kernel, T = 6 in one launch, against a twin env that takes 6 pnr_step launches: an
    env that succeeds in step t continues in step t + 1 from the new draw (the pair lanes' reset note to the sub-step lane).
    Flags equal the twin's, except for envs whose twin distance is within 1e-3 of done_distance at their first disagreement
    (at most 0.5 % of the envs; those are compared no further).  All the others: rows and rewards at the ROLL tolerances at
    every step; command state, counters and draws exact."""
    T, dyn = 6, dict(randomize=1)
    env = make_env(n, seed=14, act_layout=act_layout, auto_reset=True, **dyn)
    twin = make_env(n, seed=14, act_layout=act_layout, auto_reset=True, **dyn)
    ref = phase_b_oracle(n, **orc_kw(14, **dyn))
    rng, _, _ = start(n, 14, 400 + n, [env, twin], [ref])
    acts = (rng.uniform(-0.3, 0.3, (T, n, 6)) * env.a_max).astype(np.float32)
    obs, rew, done, trunc = env.rollout(dev_actions(env, acts))
    o = rows(env, obs); rew, done, trunc = host(rew, done, trunc)
    exempt = np.zeros(n, dtype=bool)
    fig, successes, later_successes = {}, 0, 0
    for t in range(T):
        to, tr, td, tt, ti = twin.vector_step(dev_actions(twin, acts[t]), want_info=True)
        to = rows(twin, to); tr, td, tt, ti = host(tr, td, tt, ti)
        differ = ((td != done[t]) | (tt != trunc[t])) & ~exempt
        assert (np.abs(ti[differ, 3] - DONE_DISTANCE) < PTR_TOL).all(), "flags differ away from the threshold"
        exempt |= differ
        keep = ~exempt
        err = np.abs(to[keep] - o[t][keep]).max(); rerr = np.abs(tr[keep] - rew[t][keep]).max()
        assert err <= ROLL_OBS_TOL and rerr <= ROLL_REW_TOL, (t, err, rerr)
        merge_worst(fig, {"twin_row": float(err), "twin_rew": float(rerr)})
        successes += int(done[t][keep].sum()); later_successes += int(done[t][keep].sum()) if t > 0 else 0
        if t == 0:
            assert 0.2 <= td.mean() <= 0.8
    assert exempt.mean() <= EXEMPT_CAP, exempt.mean()
    keep = ~exempt
    w, tw = words(env), words(twin)
    assert np.array_equal(w[:21, keep], tw[:21, keep]) and np.array_equal(w[22:, keep], tw[22:, keep])
    assert np.array_equal(dyn_words(env)[12:35, keep], dyn_words(twin)[12:35, keep])
    assert successes >= 0.2 * n
    env.close(); twin.close()
    record("success_reset/rollout/n%d/%s" % (n, act_layout),
           dict(fig, exempt_share=float(exempt.mean()), cap=EXEMPT_CAP, successes=successes, successes_after_step0=later_successes,
                ROLL_OBS_TOL=ROLL_OBS_TOL, ROLL_REW_TOL=ROLL_REW_TOL))


# ---- 5. joint stops -------------------------------------------------------------------------------------------------------------

def _ulp_noise(x, rng):
    """Every float32 entry moved by one ulp up or down."""
    x = np.asarray(x, dtype=np.float32)
    return np.nextafter(x, np.where(rng.rand(*x.shape) < 0.5, -np.inf, np.inf).astype(np.float32))


@pytest.mark.parametrize("kernel", ["step", "rollout"])
@pytest.mark.parametrize("n", [129, 2048])
def test_joint_stops(n, kernel):
    """Every joint starts within 0.05 rad of one of its stops, moving at U(-2, 8) rad/s towards it (joint_damping = 0.05), and
    the step runs with a zero action: the clamp to the float32 limit, the zeroing of qd and the angle actually turned, which
    rotates the joint's carried cos/sin pair (pnr_dyn.h), are reached by construction — at least 30 % of the envs have a parked
    joint after the step (asserted on the oracle).  Then 3 re-synced steps of +-0.3 a_max actions (rollout kernel: T = 2, the
    second step with such an action; both steps are judged by row columns 0:6 / 90:96, the oracle fed with the first row's).
    Hitting a stop inside a sub-step is a branch: float32 noise may take it one sub-step later, so Q_TOL / QD_TOL hold for all
    but 0.5 % of the envs (the project's allowance for such a branch), the exempt envs stay finite and inside the limits, and
    outside them the set of parked joints (q == the float32 limit and qd == 0, exactly) equals the oracle's.  The reference
    alone, under one-ulp noise on the constructed q and qd, moves no env by more than Q_TOL / QD_TOL in the first step (on the
    oracle about one env-step in 25 000 of this scenario sits on such a branch under that noise; the seeds here are ones where
    none does).  The later steps start from the engine's own state, so there the noisy reference is only held to the same 0.5 %
    and its worst figure recorded."""
    dyn = dict(joint_damping=0.05)
    env = make_env(n, seed=17, max_steps=0, **dyn)
    full = full_oracle(n, **orc_kw(17, max_steps=0, **dyn))
    noisy = full_oracle(n, **orc_kw(17, max_steps=0, **dyn))
    rng, _, _ = start(n, 17, 500 + n, [env], [full, noisy])
    noise_rng = np.random.RandomState(600 + n)
    lo, hi = env.r_lo.astype(np.float64), env.r_hi.astype(np.float64)
    side = np.where(rng.rand(n, 6) < 0.5, -1.0, 1.0)                                 # -1: the lower stop, +1: the upper
    gap = rng.uniform(0.0, 0.05, (n, 6))
    q0 = np.where(side > 0, hi - gap, lo + gap).astype(np.float32)
    qd0 = (side * rng.uniform(-2.0, 8.0, (n, 6))).astype(np.float32)
    w = env.get_dyn_state()
    w[0:6] = torch.from_numpy(q0.T.copy()).cuda(); w[6:12] = torch.from_numpy(qd0.T.copy()).cuda()
    env.set_dyn_state(w)
    T = 4 if kernel == "step" else 2
    acts = np.zeros((T, n, 6), np.float32)
    acts[1:] = (np.where(rng.rand(T - 1, n, 6) < 0.5, -0.3, 0.3) * env.a_max).astype(np.float32)
    if kernel == "rollout":
        full.load_state_words(words(env)); noisy.load_state_words(words(env))
        first_dyn = dyn_words(env)
        obs, _, _, _ = env.rollout(dev_actions(env, acts))
        o = rows(env, obs)
    fig = {"dq": 0.0, "dqd": 0.0, "ref_noise_dq": 0.0, "ref_noise_dqd": 0.0}
    exempt_all = np.zeros(n, dtype=bool)
    for t in range(T):
        if kernel == "step":
            full.load_state_words(words(env)); noisy.load_state_words(words(env))
            pre_dyn = dyn_words(env)
            env.vector_step(dev_actions(env, acts[t]))
            post = dyn_words(env)
            gq, gqd = post[0:6].T, post[6:12].T
        else:
            pre_dyn = first_dyn
            if t > 0:
                pre_dyn = first_dyn.copy(); pre_dyn[0:6] = o[t - 1][:, 0:6].T; pre_dyn[6:12] = o[t - 1][:, 90:96].T
            gq, gqd = o[t][:, 0:6].astype(np.float32), o[t][:, 90:96].astype(np.float32)
        full.load_dyn_words(pre_dyn)
        nz = pre_dyn.copy(); nz[0:6] = _ulp_noise(pre_dyn[0:6], noise_rng); nz[6:12] = _ulp_noise(pre_dyn[6:12], noise_rng)
        noisy.load_dyn_words(nz)
        full.step(acts[t]); noisy.step(acts[t])
        oq, oqd = full.dstate["q"], full.dstate["qd"]
        # the reference alone
        nq, nqd = np.abs(noisy.dstate["q"] - oq).max(1), np.abs(noisy.dstate["qd"] - oqd).max(1)
        ndq, ndqd = nq.max(), nqd.max()
        if t == 0:          # the constructed inputs; later steps start from the engine's own state, where the seeds decide nothing
            assert ndq <= Q_TOL and ndqd <= QD_TOL, (t, ndq, ndqd)
        assert ((nq > Q_TOL) | (nqd > QD_TOL)).mean() <= EXEMPT_CAP
        o_parked = ((oq == lo) | (oq == hi)) & (oqd == 0)
        if t == 0:
            assert o_parked.any(1).mean() >= 0.30, o_parked.any(1).mean()
            fig["parked_env_share"] = float(o_parked.any(1).mean()); fig["parked_joint_share"] = float(o_parked.mean())
        # the engine
        eq = np.abs(gq.astype(np.float64) - oq).max(1); eqd = np.abs(gqd.astype(np.float64) - oqd).max(1)
        exempt = ~((eq <= Q_TOL) & (eqd <= QD_TOL))
        exempt_all |= exempt
        assert exempt.mean() <= EXEMPT_CAP, (t, exempt.mean(), eq.max(), eqd.max())
        assert np.isfinite(gq).all() and np.isfinite(gqd).all() and (gq >= env.r_lo).all() and (gq <= env.r_hi).all()
        g_parked = ((gq == env.r_lo) | (gq == env.r_hi)) & (gqd == 0)
        assert np.array_equal(g_parked[~exempt], o_parked[~exempt])
        fig["dq"] = max(fig["dq"], float(eq[~exempt].max())); fig["dqd"] = max(fig["dqd"], float(eqd[~exempt].max()))
        if t == 0:
            fig["ref_noise_dq"], fig["ref_noise_dqd"] = float(ndq), float(ndqd)
        fig["ref_noise_dq_later"] = max(fig.get("ref_noise_dq_later", 0.0), float(ndq) if t else 0.0)
        fig["ref_noise_dqd_later"] = max(fig.get("ref_noise_dqd_later", 0.0), float(ndqd) if t else 0.0)
        fig["exempt_share_step%d" % t] = float(exempt.mean())
    env.close()
    record("joint_stops/%s/n%d" % (kernel, n), dict(fig, exempt_share_any_step=float(exempt_all.mean()), cap=EXEMPT_CAP, Q_TOL=Q_TOL, QD_TOL=QD_TOL))
