"""The project's accuracy bars, each stated and justified once, and the numpy-only checks that apply them.  Imports nothing heavier
than numpy: the CPU tests and the reference models read their bars here without loading torch or the oracle.

KINEMATIC MODE (float32 engine vs float64 oracle, ORC_DEV storage model; tests/test_gpu_parity.py):
  * joint state a, v, r and target: BIT-EXACT (the integrator reproduces the
    reference's mixed-precision arithmetic; reset draws share Philox4x32-10);
  * cos/sin observation entries: 4e-7 absolute (<= ~2 float32 ulp at 1.0 on top
    of the oracle's own float32 rounding);
  * pointer xyz / diff / distance: 3e-5 absolute in a ~30-unit workspace
    (relative 1e-6);
  * potential 1e-4, reward 2e-4 absolute: potential = 95/(d/10+1) <= 95 is a float32
    (ulp 7.6e-6 near 95) with |d pot / d dist| <= 9.5, so a 3e-5 distance error alone can
    move it by ~3e-4 at dist -> 0 and by < 1e-4 in the target box; the reward is a
    difference of two such potentials.

DYNAMICS MODE (float32 kernel, 10 sub-steps, vs the float64 dynamics oracle; tests/test_gpu_dynamics.py):
  re-synchronised single steps: |dq| <= 5e-5 rad, |dqd| <= 2e-3 rad/s.
Where Q_TOL = 5e-5 comes from (measured worst single-step deviations over 2 048 envs x 25 steps, MI355X, r02;
every run rewrites dyn_parity_margins.json): pd 4.3e-6, gravity_friction 9.5e-7, ground 9.5e-7,
box 7.2e-7, randomized 1.2e-5, torque_limited 2.1e-5 rad (= 88 float32 ulps of a joint angle near pi); |dqd| at most
1.2e-3 rad/s (randomized).  The two large ones are the scenarios that weaken the PD loop's contraction of rounding
differences: a saturated torque cap applies the same clipped torque whatever the tracking error, so float32-vs-float64
differences of the ABA accelerations (|qdd| up to ~500 rad/s^2 here, relative error ~1e-6 x the conditioning of the
articulated inertia) are integrated open-loop over the ten sub-steps; per-env link scales down to 0.5 raise the
accelerations the same way.  r01 first set 2e-5 from the pd / gravity scenarios alone and torque_limited missed it
by 5 % (2.098e-5); 5e-5 is 2.4x the worst measured value, QD_TOL = 2e-3 is 1.7x.
"""
import numpy as np

TRIG_TOL = 4e-7
POS_TOL = 3e-5
POT_TOL = 1e-4
REW_TOL = 2e-4

Q_TOL, QD_TOL = 5e-5, 2e-3
PTR_TOL = 1e-3          # the pointer after a dynamics step: a 30-unit arm x 2e-5 rad

# pnr_step and pnr_rollout run two separately compiled kernels in dynamics mode (dyn_step_kernel / dyn_rollout_kernel)
# that share one text of the arithmetic, compiled with fp contraction allowed: the same expression may be fused
# differently in the two, so their float32 results agree to rounding, not to the bit (kinematic mode, which has a
# bit-exactness contract, is compiled without contraction and IS identical between the two entry points).
ROLL_OBS_TOL = 2e-3     # abs, after <= 11 steps of rounding-level differences through the PD loop (positions up to ~30)
ROLL_REW_TOL = 2e-3

TRIG_IDX = np.r_[6:18, 24:36, 42:54, 60:72, 78:90, 96:108, 114:126]
LIN_IDX = np.r_[0:6, 18:24, 36:42, 90:96, 108:114, 129:132]      # exact float32 copies
SUB_IDX = np.r_[54:60, 72:78]                                      # float32 subtractions (exact vs oracle)
POS_IDX = np.r_[126:129, 132:136]


def _within(got, want, tol, what):
    worst = np.abs(got - want).max()
    assert worst <= tol, f"{what}: worst deviation {worst:.3e} exceeds {tol:.1e}"


def check_obs(got, want):
    """got/want [n,137] float64."""
    g, w = got, want
    for idx, what in ((LIN_IDX, "linear obs entries must be exact"), (SUB_IDX, "r - r_lo / r_hi - r must be exact float32")):
        assert np.array_equal(g[:, idx], w[:, idx]), f"{what}: {int((g[:, idx] != w[:, idx]).sum())} entries differ"
    _within(g[:, TRIG_IDX], w[:, TRIG_IDX], TRIG_TOL, "cos/sin obs entries (TRIG_TOL)")
    _within(g[:, POS_IDX], w[:, POS_IDX], POS_TOL, "pointer xyz / diff / distance (POS_TOL)")
    _within(g[:, 136], w[:, 136], POT_TOL, "potential (POT_TOL)")
