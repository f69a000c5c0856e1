"""The inputs and bars of the joint-state tests, shared by the CPU tests (which measure on them what float32 alone costs and assert
the conditions the bars rest on) and the GPU tests (which run the kernel on exactly these inputs).  Nothing here is a reference:
that is tests/joint_state_ref.py.

INPUTS.  Families A, B, C, D, Dc of tests/external_force_cases.py with their states, wrench records and joint torques (the four
PHYS instantiations; 7 of the first 64 envs of C and 15 of Dc touch the plane); the constraint cases mixed, subset and scaled of
tests/constraint_motor_cases.py (frame_skip 1) at their step-0 states; and one gravity-hold scenario, `hold`: hold_poses of
tests/inverse_dynamics_cases.py at g = 9.81, qd = 0, free motors, drawn link scales without joint losses, joint_torques = the
float64 gravity torques plus J^T of a payload HOLD_W hanging on the pointer, and the payload itself as a world-frame record
(0, 0, -HOLD_W) at the pointer: the arm rests, and joint 0 carries the arm's weight plus the payload.

BARS.  The project's method (tests/inverse_dynamics_cases.py): the FLOOR of a quantity is what float32 alone costs on these inputs,
measured on the CPU by `floors()` as the larger of
  (a) |float32 restatement - float64| of the Newton-Euler part (joint_state_ref.newton_euler_reaction for the reaction and the
      torques recovered from it, joint_state_ref.forward32 for q̈, the env-wide PD law restated below for family A's motor torque),
  (b) the change of the float64 reference when q and qd are moved by one float32 ulp with random signs (which also sees the penalty
      contacts' stiffness, kp = 2000 per sample, and the PD gains),
per quantity and joint, the maximum over N_MAX = 1000 envs, rounded up to two digits; separately for the call's four forms ("ext": with
the family's wrench records and joint torques; "wrench": the records alone; "torque": the torques alone, the kernel's path with
external inputs and no record; "plain": neither, which is another instantiation and has other magnitudes) and
for the envs in and out of contact (a penalty spring carries a float32 ulp of the pose into the forces of the env that touches, and of
no other).  The reaction's quantities are the joint's force and moment VECTORS: the floor is the worst component's, the magnitude the
vector's (a component the pose happens to make small is no quantity of its own).  The kernel is allowed FLOOR_MARGIN = 8 times them (a different
order of operations, fused multiply-adds, packed pairs, sincos against libm).  tests/test_joint_state_cpu.py asserts
floor <= constant <= 2 floor and that every bar is <= 1e-3 of its quantity's batch median magnitude.  In `hold` q̈ is zero by construction, and its bar is held
against the same arm's free-fall q̈.  A motor torque RECOVERED from the reaction (the inertia-scaled law: tau = the moment's axis
component - joint_torque + losses) has the joint's moment's floor, and 8 x that floor is up to 1.9e-3 of the torque's own median (Dc in
contact, wrist joints): there the bar is CAPPED at 1e-3 of the torque's batch median (`tau_median`, the measured median rounded
down), so it is less than 8 floors (4.2 at the least) and the condition holds as stated.

The constraint cases are held to the project's velocity bar of a sub-step instead: h |dq̈| <= QD_TOL and h |M^-1 d tau| <= QD_TOL
over all six joints (a torque error counts as the velocity it would cause; on the constraint joints this is the issue's
h |A_SS d tau|), every env compared: the boxed solution is Lipschitz in its data (tests/test_gpu_constraint_motor.py).  Their
reaction is a function of (q, qd, q̈): it is compared with the reference evaluated AT THE KERNEL'S q̈, to the float32 floor of that
function measured as above (REACTION_AT_QDD).  constraint_motor_cases.states draws a batch's states from the batch size, so these
floors are those of the cases' distribution, measured on its 1000-env draw, not of the very envs a smaller batch runs.

MEASURED (numpy 2.x, x86-64, N_MAX envs; scenario, form, class, quantity, the six joints' floors, the largest ratio of 8 floors to
the quantity's batch median magnitude, and for the motor torque that median); the constants below are these rounded up (medians: down):
    A      ext    free    qdd       5.025e-05 1.116e-05 2.722e-05 6.603e-04 5.352e-04 1.077e-03   (8 x floor / median <= 2.5e-04)
    A      ext    free    tau       9.656e-04 4.888e-04 4.888e-04 9.656e-04 4.888e-04 9.656e-04   (8 x floor / median <= 6.6e-05); median 1.182e+02 1.221e+02 1.118e+02 1.163e+02 1.131e+02 1.221e+02
    A      ext    free    force     5.941e-04 5.941e-04 5.941e-04 5.509e-04 4.827e-04 4.793e-04   (8 x floor / median <= 7.0e-05)
    A      ext    free    moment    9.251e-03 8.496e-03 7.058e-03 7.097e-03 3.247e-03 3.143e-03   (8 x floor / median <= 1.5e-04)
    A      wrench free    qdd       5.025e-05 1.116e-05 2.720e-05 6.603e-04 5.352e-04 1.077e-03   (8 x floor / median <= 2.5e-04)
    A      wrench free    tau       9.656e-04 4.888e-04 4.888e-04 9.656e-04 4.888e-04 9.656e-04   (8 x floor / median <= 6.6e-05); median 1.182e+02 1.221e+02 1.118e+02 1.163e+02 1.131e+02 1.221e+02
    A      wrench free    force     6.153e-04 6.153e-04 6.153e-04 5.504e-04 4.823e-04 4.794e-04   (8 x floor / median <= 7.3e-05)
    A      wrench free    moment    1.277e-02 1.318e-02 7.056e-03 7.092e-03 3.247e-03 3.142e-03   (8 x floor / median <= 2.3e-04)
    A      torque free    qdd       4.953e-05 7.641e-06 2.449e-05 6.492e-04 1.527e-04 8.925e-04   (8 x floor / median <= 6.6e-04)
    A      torque free    tau       9.656e-04 4.888e-04 4.888e-04 9.656e-04 4.888e-04 9.656e-04   (8 x floor / median <= 6.6e-05); median 1.182e+02 1.221e+02 1.118e+02 1.163e+02 1.131e+02 1.221e+02
    A      torque free    force     5.730e-04 5.730e-04 5.730e-04 5.280e-04 5.140e-04 3.809e-04   (8 x floor / median <= 1.2e-04)
    A      torque free    moment    9.445e-03 8.014e-03 6.885e-03 6.942e-03 2.257e-03 1.990e-03   (8 x floor / median <= 2.0e-04)
    A      plain  free    qdd       4.921e-05 7.646e-06 2.446e-05 6.492e-04 1.528e-04 8.925e-04   (8 x floor / median <= 6.7e-04)
    A      plain  free    tau       9.656e-04 4.888e-04 4.888e-04 9.656e-04 4.888e-04 9.656e-04   (8 x floor / median <= 6.6e-05); median 1.182e+02 1.221e+02 1.118e+02 1.163e+02 1.131e+02 1.221e+02
    A      plain  free    force     6.462e-04 6.462e-04 6.462e-04 6.932e-04 6.757e-04 4.965e-04   (8 x floor / median <= 1.6e-04)
    A      plain  free    moment    9.464e-03 7.820e-03 7.805e-03 8.402e-03 2.257e-03 1.989e-03   (8 x floor / median <= 2.1e-04)
    B      ext    free    qdd       2.336e-06 1.609e-06 2.723e-06 3.939e-05 1.448e-05 3.833e-05   (8 x floor / median <= 7.6e-05)
    B      ext    free    tau       0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00   (8 x floor / median <= 0.0e+00)
    B      ext    free    force     6.054e-05 6.928e-05 6.853e-05 7.173e-05 6.408e-05 5.021e-05   (8 x floor / median <= 2.2e-05)
    B      ext    free    moment    1.026e-03 9.169e-04 8.004e-04 8.142e-04 8.280e-05 8.503e-05   (8 x floor / median <= 9.8e-05)
    B      wrench free    qdd       2.309e-06 1.423e-06 2.913e-06 3.713e-05 1.448e-05 3.817e-05   (8 x floor / median <= 7.1e-05)
    B      wrench free    tau       0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00   (8 x floor / median <= 0.0e+00)
    B      wrench free    force     6.573e-05 6.573e-05 6.001e-05 6.180e-05 5.969e-05 5.075e-05   (8 x floor / median <= 2.0e-05)
    B      wrench free    moment    1.382e-03 1.146e-03 8.109e-04 7.677e-04 1.352e-04 1.372e-04   (8 x floor / median <= 9.5e-05)
    B      torque free    qdd       1.841e-06 1.359e-06 2.452e-06 3.352e-05 5.060e-06 3.699e-05   (8 x floor / median <= 3.2e-04)
    B      torque free    tau       0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00   (8 x floor / median <= 0.0e+00)
    B      torque free    force     4.840e-05 5.920e-05 4.558e-05 4.467e-05 4.939e-05 3.864e-05   (8 x floor / median <= 2.2e-05)
    B      torque free    moment    1.196e-03 9.934e-04 7.112e-04 5.314e-04 5.474e-05 5.879e-05   (8 x floor / median <= 1.2e-04)
    B      plain  free    qdd       1.573e-06 1.357e-06 2.642e-06 3.425e-05 4.800e-06 3.805e-05   (8 x floor / median <= 4.7e-04)
    B      plain  free    tau       0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00   (8 x floor / median <= 0.0e+00)
    B      plain  free    force     4.830e-05 4.830e-05 4.830e-05 5.192e-05 5.186e-05 4.220e-05   (8 x floor / median <= 2.4e-05)
    B      plain  free    moment    1.352e-03 8.772e-04 5.986e-04 7.803e-04 6.339e-05 6.202e-05   (8 x floor / median <= 1.4e-04)
    C      ext    free    qdd       2.392e-06 1.854e-06 2.641e-06 7.579e-05 1.444e-05 7.149e-05   (8 x floor / median <= 1.5e-04)
    C      ext    free    tau       0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00   (8 x floor / median <= 0.0e+00)
    C      ext    free    force     7.971e-05 8.125e-05 8.066e-05 8.207e-05 7.743e-05 6.540e-05   (8 x floor / median <= 2.6e-05)
    C      ext    free    moment    1.184e-03 1.006e-03 9.959e-04 1.039e-03 1.450e-04 1.373e-04   (8 x floor / median <= 1.3e-04)
    C      ext    contact qdd       5.213e-05 1.471e-04 1.323e-04 5.779e-04 1.262e-03 1.055e-03   (8 x floor / median <= 5.7e-05)
    C      ext    contact tau       0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00   (8 x floor / median <= 0.0e+00)
    C      ext    contact force     4.290e-03 5.517e-03 5.593e-03 5.321e-03 6.718e-03 3.928e-03   (8 x floor / median <= 3.3e-05)
    C      ext    contact moment    5.304e-02 4.820e-02 3.402e-02 3.661e-02 1.023e-02 7.866e-03   (8 x floor / median <= 2.4e-04)
    C      wrench free    qdd       2.419e-06 1.916e-06 2.971e-06 7.596e-05 1.438e-05 7.251e-05   (8 x floor / median <= 1.5e-04)
    C      wrench free    tau       0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00   (8 x floor / median <= 0.0e+00)
    C      wrench free    force     7.046e-05 7.046e-05 6.665e-05 7.010e-05 5.896e-05 4.768e-05   (8 x floor / median <= 2.0e-05)
    C      wrench free    moment    1.569e-03 1.275e-03 7.471e-04 7.726e-04 9.822e-05 8.949e-05   (8 x floor / median <= 9.9e-05)
    C      wrench contact qdd       5.214e-05 1.471e-04 1.323e-04 5.804e-04 1.262e-03 1.055e-03   (8 x floor / median <= 5.7e-05)
    C      wrench contact tau       0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00   (8 x floor / median <= 0.0e+00)
    C      wrench contact force     4.290e-03 5.517e-03 4.796e-03 5.196e-03 6.718e-03 3.372e-03   (8 x floor / median <= 3.2e-05)
    C      wrench contact moment    4.849e-02 4.366e-02 3.189e-02 3.707e-02 1.362e-02 1.263e-02   (8 x floor / median <= 2.5e-04)
    C      torque free    qdd       1.912e-06 1.098e-06 2.258e-06 5.812e-05 4.262e-06 5.768e-05   (8 x floor / median <= 5.8e-04)
    C      torque free    tau       0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00   (8 x floor / median <= 0.0e+00)
    C      torque free    force     3.664e-05 3.802e-05 3.817e-05 3.710e-05 3.699e-05 3.305e-05   (8 x floor / median <= 1.9e-05)
    C      torque free    moment    7.440e-04 6.478e-04 3.415e-04 3.874e-04 3.952e-05 4.088e-05   (8 x floor / median <= 7.8e-05)
    C      torque contact qdd       5.229e-05 1.472e-04 1.162e-04 7.794e-04 1.261e-03 1.058e-03   (8 x floor / median <= 5.4e-05)
    C      torque contact tau       0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00   (8 x floor / median <= 0.0e+00)
    C      torque contact force     6.283e-03 6.607e-03 5.309e-03 5.199e-03 6.722e-03 4.442e-03   (8 x floor / median <= 3.9e-05)
    C      torque contact moment    5.530e-02 6.324e-02 4.550e-02 5.329e-02 1.430e-02 1.824e-02   (8 x floor / median <= 3.7e-04)
    C      plain  free    qdd       1.938e-06 1.160e-06 2.097e-06 5.829e-05 4.963e-06 5.919e-05   (8 x floor / median <= 9.0e-04)
    C      plain  free    tau       0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00   (8 x floor / median <= 0.0e+00)
    C      plain  free    force     4.038e-05 5.145e-05 4.391e-05 3.553e-05 4.078e-05 3.196e-05   (8 x floor / median <= 1.9e-05)
    C      plain  free    moment    9.856e-04 8.845e-04 4.444e-04 4.166e-04 5.265e-05 5.177e-05   (8 x floor / median <= 1.2e-04)
    C      plain  contact qdd       5.229e-05 1.472e-04 1.162e-04 8.423e-04 1.261e-03 1.058e-03   (8 x floor / median <= 5.4e-05)
    C      plain  contact tau       0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00   (8 x floor / median <= 0.0e+00)
    C      plain  contact force     4.293e-03 5.521e-03 4.394e-03 5.199e-03 6.722e-03 4.010e-03   (8 x floor / median <= 3.3e-05)
    C      plain  contact moment    3.712e-02 4.110e-02 5.245e-02 6.692e-02 1.376e-02 1.422e-02   (8 x floor / median <= 4.7e-04)
    D      ext    free    qdd       1.576e-04 1.456e-04 3.485e-04 7.170e-04 5.089e-04 1.040e-03   (8 x floor / median <= 1.3e-04)
    D      ext    free    tau       1.842e-01 4.100e-02 2.696e-02 2.546e-03 1.057e-03 6.383e-04   (8 x floor / median <= 3.8e-04); median 3.929e+03 7.453e+03 5.185e+03 7.937e+01 1.842e+02 8.019e+01
    D      ext    free    force     1.014e-02 1.014e-02 1.014e-02 8.488e-03 6.786e-03 4.906e-03   (8 x floor / median <= 6.1e-05)
    D      ext    free    moment    1.842e-01 1.897e-01 8.277e-02 8.137e-02 6.604e-03 6.047e-03   (8 x floor / median <= 1.3e-04)
    D      wrench free    qdd       1.576e-04 1.456e-04 3.485e-04 7.169e-04 5.089e-04 1.040e-03   (8 x floor / median <= 1.3e-04)
    D      wrench free    tau       1.842e-01 4.100e-02 2.696e-02 3.148e-03 1.124e-03 6.383e-04   (8 x floor / median <= 3.8e-04); median 3.929e+03 7.453e+03 5.185e+03 7.937e+01 1.842e+02 8.019e+01
    D      wrench free    force     1.014e-02 1.014e-02 1.014e-02 8.488e-03 6.786e-03 4.905e-03   (8 x floor / median <= 6.1e-05)
    D      wrench free    moment    1.842e-01 1.897e-01 8.277e-02 8.137e-02 6.604e-03 6.047e-03   (8 x floor / median <= 1.3e-04)
    D      torque free    qdd       1.504e-04 1.443e-04 3.425e-04 4.886e-04 5.329e-04 7.622e-04   (8 x floor / median <= 1.5e-04)
    D      torque free    tau       1.842e-01 4.100e-02 2.696e-02 2.250e-03 1.011e-03 6.383e-04   (8 x floor / median <= 3.8e-04); median 3.929e+03 7.453e+03 5.185e+03 7.937e+01 1.842e+02 8.019e+01
    D      torque free    force     1.022e-02 1.022e-02 1.022e-02 8.481e-03 6.835e-03 4.867e-03   (8 x floor / median <= 6.5e-05)
    D      torque free    moment    1.842e-01 1.897e-01 8.199e-02 8.069e-02 5.144e-03 4.724e-03   (8 x floor / median <= 1.3e-04)
    D      plain  free    qdd       1.504e-04 1.443e-04 3.425e-04 4.885e-04 5.329e-04 7.622e-04   (8 x floor / median <= 1.5e-04)
    D      plain  free    tau       1.842e-01 4.100e-02 2.696e-02 2.136e-03 1.011e-03 6.383e-04   (8 x floor / median <= 3.8e-04); median 3.929e+03 7.453e+03 5.185e+03 7.937e+01 1.842e+02 8.019e+01
    D      plain  free    force     1.022e-02 1.022e-02 1.022e-02 8.481e-03 6.835e-03 4.866e-03   (8 x floor / median <= 6.5e-05)
    D      plain  free    moment    1.842e-01 1.897e-01 8.199e-02 8.069e-02 5.144e-03 4.724e-03   (8 x floor / median <= 1.3e-04)
    Dc     ext    free    qdd       1.370e-04 1.453e-04 3.328e-04 6.194e-04 5.786e-04 1.020e-03   (8 x floor / median <= 1.2e-04)
    Dc     ext    free    tau       1.855e-01 4.091e-02 2.577e-02 3.316e-03 1.272e-03 6.383e-04   (8 x floor / median <= 3.9e-04); median 3.788e+03 7.155e+03 5.074e+03 9.407e+01 1.747e+02 7.652e+01
    Dc     ext    free    force     9.945e-03 9.945e-03 9.945e-03 8.474e-03 6.765e-03 4.930e-03   (8 x floor / median <= 6.1e-05)
    Dc     ext    free    moment    1.855e-01 1.842e-01 8.317e-02 8.079e-02 7.442e-03 6.122e-03   (8 x floor / median <= 1.3e-04)
    Dc     ext    contact qdd       1.600e-04 5.472e-04 6.046e-04 5.246e-03 5.126e-03 7.893e-03   (8 x floor / median <= 9.7e-05)
    Dc     ext    contact tau       1.780e-01 2.355e-01 1.352e-01 2.629e-02 3.825e-02 1.994e-02   (8 x floor / median <= 1.9e-03); median 4.677e+03 6.674e+03 5.502e+03 1.104e+02 1.876e+02 8.313e+01
    Dc     ext    contact force     2.362e-02 2.291e-02 2.068e-02 1.378e-02 1.374e-02 1.063e-02   (8 x floor / median <= 3.5e-05)
    Dc     ext    contact moment    2.632e-01 2.354e-01 1.350e-01 1.268e-01 3.825e-02 3.418e-02   (8 x floor / median <= 1.6e-04)
    Dc     wrench free    qdd       1.373e-04 1.453e-04 3.328e-04 6.194e-04 5.786e-04 1.020e-03   (8 x floor / median <= 1.2e-04)
    Dc     wrench free    tau       1.855e-01 4.091e-02 2.577e-02 3.076e-03 1.298e-03 6.613e-04   (8 x floor / median <= 3.9e-04); median 3.788e+03 7.155e+03 5.074e+03 9.407e+01 1.747e+02 7.652e+01
    Dc     wrench free    force     9.945e-03 9.945e-03 9.945e-03 8.474e-03 6.765e-03 4.930e-03   (8 x floor / median <= 6.1e-05)
    Dc     wrench free    moment    1.855e-01 1.842e-01 8.317e-02 8.079e-02 7.442e-03 6.122e-03   (8 x floor / median <= 1.3e-04)
    Dc     wrench contact qdd       1.600e-04 5.472e-04 6.046e-04 5.309e-03 5.118e-03 7.447e-03   (8 x floor / median <= 9.8e-05)
    Dc     wrench contact tau       1.780e-01 2.579e-01 1.290e-01 2.617e-02 2.909e-02 1.523e-02   (8 x floor / median <= 1.9e-03); median 4.677e+03 6.674e+03 5.502e+03 1.104e+02 1.876e+02 8.313e+01
    Dc     wrench contact force     2.221e-02 2.386e-02 1.928e-02 1.745e-02 2.205e-02 1.280e-02   (8 x floor / median <= 3.5e-05)
    Dc     wrench contact moment    2.435e-01 2.579e-01 1.290e-01 1.466e-01 2.909e-02 2.912e-02   (8 x floor / median <= 1.3e-04)
    Dc     torque free    qdd       1.417e-04 1.482e-04 3.428e-04 5.004e-04 5.263e-04 8.119e-04   (8 x floor / median <= 1.4e-04)
    Dc     torque free    tau       1.855e-01 4.091e-02 2.577e-02 2.138e-03 1.004e-03 6.383e-04   (8 x floor / median <= 3.9e-04); median 3.788e+03 7.155e+03 5.074e+03 9.407e+01 1.747e+02 7.652e+01
    Dc     torque free    force     9.971e-03 9.971e-03 9.971e-03 8.504e-03 6.706e-03 4.838e-03   (8 x floor / median <= 6.4e-05)
    Dc     torque free    moment    1.855e-01 1.844e-01 8.306e-02 8.081e-02 4.880e-03 4.391e-03   (8 x floor / median <= 1.3e-04)
    Dc     torque contact qdd       1.657e-04 5.472e-04 6.062e-04 4.655e-03 4.177e-03 6.524e-03   (8 x floor / median <= 9.0e-05)
    Dc     torque contact tau       1.780e-01 4.029e-01 1.448e-01 2.684e-02 2.756e-02 1.985e-02   (8 x floor / median <= 1.9e-03); median 4.677e+03 6.674e+03 5.502e+03 1.104e+02 1.876e+02 8.313e+01
    Dc     torque contact force     2.048e-02 2.152e-02 2.131e-02 1.605e-02 1.706e-02 1.229e-02   (8 x floor / median <= 3.0e-05)
    Dc     torque contact moment    4.521e-01 4.030e-01 1.446e-01 1.177e-01 2.756e-02 3.126e-02   (8 x floor / median <= 2.0e-04)
    Dc     plain  free    qdd       1.417e-04 1.482e-04 3.428e-04 5.003e-04 5.263e-04 8.119e-04   (8 x floor / median <= 1.4e-04)
    Dc     plain  free    tau       1.855e-01 4.091e-02 2.577e-02 2.138e-03 1.180e-03 6.383e-04   (8 x floor / median <= 3.9e-04); median 3.788e+03 7.155e+03 5.074e+03 9.407e+01 1.747e+02 7.652e+01
    Dc     plain  free    force     9.971e-03 9.971e-03 9.971e-03 8.504e-03 6.706e-03 4.838e-03   (8 x floor / median <= 6.4e-05)
    Dc     plain  free    moment    1.855e-01 1.844e-01 8.306e-02 8.081e-02 4.880e-03 4.391e-03   (8 x floor / median <= 1.3e-04)
    Dc     plain  contact qdd       1.657e-04 5.472e-04 6.062e-04 4.655e-03 4.168e-03 6.079e-03   (8 x floor / median <= 9.0e-05)
    Dc     plain  contact tau       1.780e-01 1.908e-01 1.119e-01 2.295e-02 3.176e-02 2.014e-02   (8 x floor / median <= 1.9e-03); median 4.677e+03 6.674e+03 5.502e+03 1.104e+02 1.876e+02 8.313e+01
    Dc     plain  contact force     1.850e-02 1.908e-02 1.842e-02 1.488e-02 1.413e-02 1.064e-02   (8 x floor / median <= 2.7e-05)
    Dc     plain  contact moment    2.646e-01 1.908e-01 1.192e-01 1.083e-01 3.176e-02 3.406e-02   (8 x floor / median <= 1.2e-04)
    hold   ext    free    qdd       5.752e-07 4.931e-07 1.076e-06 1.448e-05 1.754e-05 3.632e-05   (8 x floor / median <= 8.7e+02)
    hold   ext    free    tau       0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00 0.000e+00   (8 x floor / median <= 0.0e+00)
    hold   ext    free    force     3.143e-05 1.990e-05 2.302e-05 2.042e-05 1.889e-05 2.664e-05   (8 x floor / median <= 4.3e-06)
    hold   ext    free    moment    3.773e-04 3.662e-04 1.831e-04 3.264e-04 6.212e-05 6.806e-05   (8 x floor / median <= 5.3e-06)
    mixed  plain  free    at_force  2.908e-03 2.908e-03 2.915e-03 2.415e-03 1.899e-03 1.757e-03   (8 x floor / median <= 5.5e-06)
    mixed  plain  free    at_moment 6.106e-02 5.089e-02 2.735e-02 2.520e-02 2.891e-03 2.670e-03   (8 x floor / median <= 2.1e-05)
    subset plain  free    at_force  2.192e-03 2.290e-03 1.841e-03 2.013e-03 1.720e-03 1.544e-03   (8 x floor / median <= 7.1e-06)
    subset plain  free    at_moment 3.940e-02 3.851e-02 2.199e-02 2.165e-02 5.653e-03 5.588e-03   (8 x floor / median <= 1.4e-05)
    scaled plain  free    at_force  7.187e-03 7.187e-03 7.187e-03 6.435e-03 6.446e-03 5.667e-03   (8 x floor / median <= 2.1e-05)
    scaled plain  free    at_moment 1.127e-01 1.065e-01 9.379e-02 8.409e-02 1.039e-02 1.305e-02   (8 x floor / median <= 2.5e-05)
"""
import numpy as np

import constraint_motor_cases as ccases
import external_force_cases as xcases
import ik_ref
import inverse_dynamics_cases as idcases
import inverse_dynamics_ref as idref
import joint_state_ref as ref
import oracle_cases as ocases
import world_step_ref as wref

DOF = 6
N_MAX = 1000
H = 1.0 / 240
FLOOR_MARGIN = 8.0
SIZES = [1, 37, 64, 1000]
FAMILIES = list(xcases.FAMILIES)                                      # A B C D Dc
CONSTRAINT = ["mixed", "subset", "scaled"]
HOLD_W = 20.0                                                         # N: about two links' weight (50 N left the wrist's float32 floor above 1e-3 of its free fall)
HOLD_SPECS = [(10, "world")]
followed = xcases.followed


def round_down(x, digits=2):
    """x rounded down to `digits` significant digits (0 stays 0)"""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    nz = x > 0
    e = np.floor(np.log10(x[nz])) - (digits - 1)
    out[nz] = np.floor(x[nz] / 10.0 ** e + 1e-9) * 10.0 ** e
    return out


def round_up(x, digits=2):
    """x rounded up to `digits` significant digits (0 stays 0)"""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    nz = x > 0
    e = np.floor(np.log10(x[nz])) - (digits - 1)
    out[nz] = np.ceil(x[nz] / 10.0 ** e - 1e-9) * 10.0 ** e
    return out


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def family_inputs(family, n=N_MAX):
    """The oracle of a family's first n envs with the family's states loaded, and the call's inputs (float32 numbers)."""
    orc = xcases.make_oracle(family, n)
    q, qd = xcases.states(family, orc.state["r"][:n])
    ocases.load_states(orc, q, qd)
    f = xcases.FAMILIES[family]
    return orc, dict(motors=f["motors"], specs=f["specs"], wrenches=xcases.wrenches(family, q), tau=xcases.joint_torques(family, n), q=q, qd=qd)


def hold_oracle(n):
    orc = idcases.make_oracle(n, 9.81, True, seed=idcases.HOLD_SEED)
    orc.dstate["friction"] = 0.0
    orc.dstate["damping"] = 0.0
    return orc


def hold_inputs(n=N_MAX, orc=None, rounded=True):
    """The gravity-hold scenario: (oracle, inputs).  rounded: the torques as the engine receives them, float32."""
    orc = orc or hold_oracle(n)
    q = idcases.hold_poses(n)
    ocases.load_states(orc, q, np.zeros_like(q))
    q64 = q.astype(np.float64)
    tip = ik_ref.point_position(q64, 10)
    J = ik_ref.jacobian(q64, 10)
    tau = idref.inverse_dynamics(orc, None, 9.81) + HOLD_W * J[:, 2, :]
    w = np.zeros((n, 1, 9))
    w[:, 0, 2] = -HOLD_W
    w[:, 0, 3:6] = tip
    if rounded:
        tau, w = tau.astype(np.float32), w.astype(np.float32)
    return orc, dict(motors=idcases.FREE_MOTORS, specs=HOLD_SPECS, wrenches=w, tau=tau, q=q, qd=np.zeros_like(q))


def constraint_inputs(case, n=N_MAX):
    orc = ccases.make_oracle(case, n)
    q, qd = ccases.states(case, n, 0)
    ocases.load_states(orc, q, qd)
    return orc, dict(motors=ccases.CASES[case]["motors"], specs=(), wrenches=None, tau=None, q=q, qd=qd)


def inputs(name, n=N_MAX):
    return hold_inputs(n) if name == "hold" else constraint_inputs(name, n) if name in CONSTRAINT else family_inputs(name, n)


def forms(name):
    """the forms of the call a scenario is measured and run in: (with wrench records, with joint torques)"""
    return [(True, True)] if name == "hold" else [(False, False)] if name in CONSTRAINT else [(True, True), (True, False), (False, True), (False, False)]


def form_name(with_w, with_t):
    return {(True, True): "ext", (True, False): "wrench", (False, True): "torque", (False, False): "plain"}[(bool(with_w), bool(with_t))]


def reference(orc, I, with_w=True, with_t=True, **kw):
    return ref.joint_states(orc, I["motors"], I["specs"] if with_w else (), I["wrenches"] if with_w else None,
                            I["tau"] if with_t else None, **kw)


# ---- the float32 floor ---------------------------------------------------------------------------------------------------------------
def pd_law32(orc, motors):
    """The PD table law of the families' motors in float32: None is the env-wide position law on the command state (kp (r - q) +
    kd (v - qd), capped at torque_limit where > 0), a zero-gain dictionary is no torque.  None under pd_inertia_scaled: NaN."""
    f = np.float32
    q, qd = orc.dstate["q"].astype(f), orc.dstate["qd"].astype(f)
    out = np.zeros(q.shape, dtype=f)
    for i, m in enumerate(motors):
        if m is None:
            if orc.d.pd_inertia_scaled:
                out[:, i] = np.nan
                continue
            t = f(orc.d.kp) * (orc.state["r"][:, i].astype(f) - q[:, i]) + f(orc.d.kd) * (orc.state["v"][:, i].astype(f) - qd[:, i])
            out[:, i] = np.clip(t, -f(orc.d.torque_limit), f(orc.d.torque_limit)) if orc.d.torque_limit > 0 else t
        else:
            assert m["kind"] == "pd" and m["position_gain"] == 0.0 and m["velocity_gain"] == 0.0
    return out


def _ulp_moved(x, rng):
    x32 = np.asarray(x, dtype=np.float32)
    up = rng.integers(0, 2, size=x32.shape).astype(bool)
    return np.where(up, np.nextafter(x32, np.float32(np.inf)), np.nextafter(x32, np.float32(-np.inf))).astype(np.float32)


QUANTITIES = ("qdd", "tau", "force", "moment")


def split(reaction):
    """force [n, 6, 3] and moment [n, 6, 3] of reaction records [n, 6, 6]"""
    return reaction[:, :, 0:3], reaction[:, :, 3:6]


def classes(hit):
    """the envs by contact state, {"free": mask, "contact": mask}, those that have an env"""
    return {k: m for k, m in (("free", ~hit), ("contact", hit)) if m.any()}


def floors(name, n=N_MAX, seed=7):
    """{form: {class: {quantity: floor [6], "median": {quantity: [6]}}}} of a scenario.  Forms: "ext" (the call with the scenario's
    wrench records and joint torques), "wrench" (the records alone) and "plain" (neither: another instantiation of the kernel, and
    other magnitudes).  Classes: the envs out of contact ("free") and in
    contact ("contact"), whose penalty springs (kp = 2000 per sample) carry a float32 ulp of the pose into the forces.  Quantities:
    qdd, tau (per joint), force, moment (per joint: the worst component's error against the VECTOR's magnitude: a component
    that the pose happens to make small is not a quantity of its own) and at_force, at_moment: the reaction's floor as a function
    of (q, qd, q̈) with q̈ held fixed (what the constraint cases use)."""
    orc, I = inputs(name, n)
    cm = name in CONSTRAINT
    f32 = lambda x: np.asarray(x, dtype=np.float32)  # noqa: E731
    keys = QUANTITIES + ("at_force", "at_moment")
    res = {}
    for with_w, with_t in forms(name):
        out = res.setdefault(form_name(with_w, with_t), {})
        ocases.load_states(orc, I["q"], I["qd"])
        R = reference(orc, I, with_w, with_t)
        sc, g = orc.dstate["mass_scale"].copy(), orc.d.gravity
        tx = np.zeros((n, DOF)) if not with_t else np.asarray(I["tau"], dtype=np.float64)
        # (a) the float32 restatements on the same float32 inputs
        r32 = ref.newton_euler_reaction(f32(I["q"]), f32(I["qd"]), f32(R["qdd"]), f32(sc), g, f32(R["fext"]), np.float32).astype(np.float64)
        d_react = np.abs(r32 - R["reaction"])
        rec32 = (ref.axis_moment(f32(r32)) - f32(tx) + f32(wref.losses(orc))).astype(np.float64)
        law32 = np.full((n, DOF), np.nan) if cm else pd_law32(orc, I["motors"]).astype(np.float64)
        d_tau = np.where(np.isnan(law32), np.abs(rec32 - R["tau_motor"]), np.abs(law32 - R["tau_motor"]))
        q32 = ref.forward32(f32(I["q"]), f32(I["qd"]), f32(sc), g, f32(R["fext"]), f32(R["total"]), np.float32).astype(np.float64)
        q64 = ref.forward32(I["q"], I["qd"], sc, g, R["fext"], R["total"], np.float64)
        d_qdd = np.abs(q32 - q64)
        # (b) one float32 ulp on q and qd, random signs, through the whole float64 reference
        rng = np.random.default_rng(seed)
        qm, qdm = _ulp_moved(I["q"], rng), _ulp_moved(I["qd"], rng)
        ocases.load_states(orc, qm, qdm)
        P = reference(orc, I, with_w, with_t)
        at = ref.newton_euler_reaction(qm.astype(np.float64), qdm.astype(np.float64), R["qdd"], sc, g, P["fext"], np.float64)
        ocases.load_states(orc, I["q"], I["qd"])
        whole, fixed = np.maximum(d_react, np.abs(P["reaction"] - R["reaction"])), np.maximum(d_react, np.abs(at - R["reaction"]))
        cand = dict(qdd=np.maximum(d_qdd, np.abs(P["qdd"] - R["qdd"])), tau=np.maximum(d_tau, np.abs(P["tau_motor"] - R["tau_motor"])),
                    force=split(whole)[0].max(axis=2), moment=split(whole)[1].max(axis=2),
                    at_force=split(fixed)[0].max(axis=2), at_moment=split(fixed)[1].max(axis=2))
        F, M = (np.linalg.norm(v, axis=2) for v in split(R["reaction"]))
        mags = dict(qdd=np.abs(R["qdd"]), tau=np.abs(R["tau_motor"]), force=F, moment=M, at_force=F, at_moment=M)
        for cls, m in classes(R["hit"]).items():
            o = out.setdefault(cls, dict({k: np.zeros(DOF) for k in keys}, median={k: np.full(DOF, np.inf) for k in keys}))
            for k in keys:
                o[k] = np.maximum(o[k], cand[k][m].max(axis=0))
                o["median"][k] = np.minimum(o["median"][k], np.median(mags[k][m], axis=0))
    return res


# measured by floors(): see the module docstring; rounded up to two digits
A6 = lambda *v: np.array(v, dtype=np.float64)  # noqa: E731
FLOORS = {
    "A": {
        "ext": {
            "free": dict(qdd=A6(5.1e-05, 1.2e-05, 2.8e-05, 6.7e-04, 5.4e-04, 1.1e-03),
                           tau=A6(9.7e-04, 4.9e-04, 4.9e-04, 9.7e-04, 4.9e-04, 9.7e-04),
                           force=A6(6.0e-04, 6.0e-04, 6.0e-04, 5.6e-04, 4.9e-04, 4.8e-04),
                           moment=A6(9.3e-03, 8.5e-03, 7.1e-03, 7.1e-03, 3.3e-03, 3.2e-03),
                           tau_median=A6(1.1e+02, 1.2e+02, 1.1e+02, 1.1e+02, 1.1e+02, 1.2e+02)),
        },
        "wrench": {
            "free": dict(qdd=A6(5.1e-05, 1.2e-05, 2.8e-05, 6.7e-04, 5.4e-04, 1.1e-03),
                           tau=A6(9.7e-04, 4.9e-04, 4.9e-04, 9.7e-04, 4.9e-04, 9.7e-04),
                           force=A6(6.2e-04, 6.2e-04, 6.2e-04, 5.6e-04, 4.9e-04, 4.8e-04),
                           moment=A6(1.3e-02, 1.4e-02, 7.1e-03, 7.1e-03, 3.3e-03, 3.2e-03),
                           tau_median=A6(1.1e+02, 1.2e+02, 1.1e+02, 1.1e+02, 1.1e+02, 1.2e+02)),
        },
        "torque": {
            "free": dict(qdd=A6(5.0e-05, 7.7e-06, 2.5e-05, 6.5e-04, 1.6e-04, 9.0e-04),
                           tau=A6(9.7e-04, 4.9e-04, 4.9e-04, 9.7e-04, 4.9e-04, 9.7e-04),
                           force=A6(5.8e-04, 5.8e-04, 5.8e-04, 5.3e-04, 5.2e-04, 3.9e-04),
                           moment=A6(9.5e-03, 8.1e-03, 6.9e-03, 7.0e-03, 2.3e-03, 2.0e-03),
                           tau_median=A6(1.1e+02, 1.2e+02, 1.1e+02, 1.1e+02, 1.1e+02, 1.2e+02)),
        },
        "plain": {
            "free": dict(qdd=A6(5.0e-05, 7.7e-06, 2.5e-05, 6.5e-04, 1.6e-04, 9.0e-04),
                           tau=A6(9.7e-04, 4.9e-04, 4.9e-04, 9.7e-04, 4.9e-04, 9.7e-04),
                           force=A6(6.5e-04, 6.5e-04, 6.5e-04, 7.0e-04, 6.8e-04, 5.0e-04),
                           moment=A6(9.5e-03, 7.9e-03, 7.9e-03, 8.5e-03, 2.3e-03, 2.0e-03),
                           tau_median=A6(1.1e+02, 1.2e+02, 1.1e+02, 1.1e+02, 1.1e+02, 1.2e+02)),
        },
    },
    "B": {
        "ext": {
            "free": dict(qdd=A6(2.4e-06, 1.7e-06, 2.8e-06, 4.0e-05, 1.5e-05, 3.9e-05),
                           tau=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
                           force=A6(6.1e-05, 7.0e-05, 6.9e-05, 7.2e-05, 6.5e-05, 5.1e-05),
                           moment=A6(1.1e-03, 9.2e-04, 8.1e-04, 8.2e-04, 8.3e-05, 8.6e-05),
                           tau_median=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)),
        },
        "wrench": {
            "free": dict(qdd=A6(2.4e-06, 1.5e-06, 3.0e-06, 3.8e-05, 1.5e-05, 3.9e-05),
                           tau=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
                           force=A6(6.6e-05, 6.6e-05, 6.1e-05, 6.2e-05, 6.0e-05, 5.1e-05),
                           moment=A6(1.4e-03, 1.2e-03, 8.2e-04, 7.7e-04, 1.4e-04, 1.4e-04),
                           tau_median=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)),
        },
        "torque": {
            "free": dict(qdd=A6(1.9e-06, 1.4e-06, 2.5e-06, 3.4e-05, 5.1e-06, 3.7e-05),
                           tau=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
                           force=A6(4.9e-05, 6.0e-05, 4.6e-05, 4.5e-05, 5.0e-05, 3.9e-05),
                           moment=A6(1.2e-03, 1.0e-03, 7.2e-04, 5.4e-04, 5.5e-05, 5.9e-05),
                           tau_median=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)),
        },
        "plain": {
            "free": dict(qdd=A6(1.6e-06, 1.4e-06, 2.7e-06, 3.5e-05, 4.8e-06, 3.9e-05),
                           tau=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
                           force=A6(4.9e-05, 4.9e-05, 4.9e-05, 5.2e-05, 5.2e-05, 4.3e-05),
                           moment=A6(1.4e-03, 8.8e-04, 6.0e-04, 7.9e-04, 6.4e-05, 6.3e-05),
                           tau_median=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)),
        },
    },
    "C": {
        "ext": {
            "free": dict(qdd=A6(2.4e-06, 1.9e-06, 2.7e-06, 7.6e-05, 1.5e-05, 7.2e-05),
                           tau=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
                           force=A6(8.0e-05, 8.2e-05, 8.1e-05, 8.3e-05, 7.8e-05, 6.6e-05),
                           moment=A6(1.2e-03, 1.1e-03, 1.0e-03, 1.1e-03, 1.5e-04, 1.4e-04),
                           tau_median=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)),
            "contact": dict(qdd=A6(5.3e-05, 1.5e-04, 1.4e-04, 5.8e-04, 1.3e-03, 1.1e-03),
                              tau=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
                              force=A6(4.3e-03, 5.6e-03, 5.6e-03, 5.4e-03, 6.8e-03, 4.0e-03),
                              moment=A6(5.4e-02, 4.9e-02, 3.5e-02, 3.7e-02, 1.1e-02, 7.9e-03),
                              tau_median=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)),
        },
        "wrench": {
            "free": dict(qdd=A6(2.5e-06, 2.0e-06, 3.0e-06, 7.6e-05, 1.5e-05, 7.3e-05),
                           tau=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
                           force=A6(7.1e-05, 7.1e-05, 6.7e-05, 7.1e-05, 5.9e-05, 4.8e-05),
                           moment=A6(1.6e-03, 1.3e-03, 7.5e-04, 7.8e-04, 9.9e-05, 9.0e-05),
                           tau_median=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)),
            "contact": dict(qdd=A6(5.3e-05, 1.5e-04, 1.4e-04, 5.9e-04, 1.3e-03, 1.1e-03),
                              tau=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
                              force=A6(4.3e-03, 5.6e-03, 4.8e-03, 5.2e-03, 6.8e-03, 3.4e-03),
                              moment=A6(4.9e-02, 4.4e-02, 3.2e-02, 3.8e-02, 1.4e-02, 1.3e-02),
                              tau_median=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)),
        },
        "torque": {
            "free": dict(qdd=A6(2.0e-06, 1.1e-06, 2.3e-06, 5.9e-05, 4.3e-06, 5.8e-05),
                           tau=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
                           force=A6(3.7e-05, 3.9e-05, 3.9e-05, 3.8e-05, 3.7e-05, 3.4e-05),
                           moment=A6(7.5e-04, 6.5e-04, 3.5e-04, 3.9e-04, 4.0e-05, 4.1e-05),
                           tau_median=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)),
            "contact": dict(qdd=A6(5.3e-05, 1.5e-04, 1.2e-04, 7.8e-04, 1.3e-03, 1.1e-03),
                              tau=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
                              force=A6(6.3e-03, 6.7e-03, 5.4e-03, 5.2e-03, 6.8e-03, 4.5e-03),
                              moment=A6(5.6e-02, 6.4e-02, 4.6e-02, 5.4e-02, 1.5e-02, 1.9e-02),
                              tau_median=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)),
        },
        "plain": {
            "free": dict(qdd=A6(2.0e-06, 1.2e-06, 2.1e-06, 5.9e-05, 5.0e-06, 6.0e-05),
                           tau=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
                           force=A6(4.1e-05, 5.2e-05, 4.4e-05, 3.6e-05, 4.1e-05, 3.2e-05),
                           moment=A6(9.9e-04, 8.9e-04, 4.5e-04, 4.2e-04, 5.3e-05, 5.2e-05),
                           tau_median=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)),
            "contact": dict(qdd=A6(5.3e-05, 1.5e-04, 1.2e-04, 8.5e-04, 1.3e-03, 1.1e-03),
                              tau=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
                              force=A6(4.3e-03, 5.6e-03, 4.4e-03, 5.2e-03, 6.8e-03, 4.1e-03),
                              moment=A6(3.8e-02, 4.2e-02, 5.3e-02, 6.7e-02, 1.4e-02, 1.5e-02),
                              tau_median=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)),
        },
    },
    "D": {
        "ext": {
            "free": dict(qdd=A6(1.6e-04, 1.5e-04, 3.5e-04, 7.2e-04, 5.1e-04, 1.1e-03),
                           tau=A6(1.9e-01, 4.1e-02, 2.7e-02, 2.6e-03, 1.1e-03, 6.4e-04),
                           force=A6(1.1e-02, 1.1e-02, 1.1e-02, 8.5e-03, 6.8e-03, 5.0e-03),
                           moment=A6(1.9e-01, 1.9e-01, 8.3e-02, 8.2e-02, 6.7e-03, 6.1e-03),
                           tau_median=A6(3.9e+03, 7.4e+03, 5.1e+03, 7.9e+01, 1.8e+02, 8.0e+01)),
        },
        "wrench": {
            "free": dict(qdd=A6(1.6e-04, 1.5e-04, 3.5e-04, 7.2e-04, 5.1e-04, 1.1e-03),
                           tau=A6(1.9e-01, 4.1e-02, 2.7e-02, 3.2e-03, 1.2e-03, 6.4e-04),
                           force=A6(1.1e-02, 1.1e-02, 1.1e-02, 8.5e-03, 6.8e-03, 5.0e-03),
                           moment=A6(1.9e-01, 1.9e-01, 8.3e-02, 8.2e-02, 6.7e-03, 6.1e-03),
                           tau_median=A6(3.9e+03, 7.4e+03, 5.1e+03, 7.9e+01, 1.8e+02, 8.0e+01)),
        },
        "torque": {
            "free": dict(qdd=A6(1.6e-04, 1.5e-04, 3.5e-04, 4.9e-04, 5.4e-04, 7.7e-04),
                           tau=A6(1.9e-01, 4.1e-02, 2.7e-02, 2.3e-03, 1.1e-03, 6.4e-04),
                           force=A6(1.1e-02, 1.1e-02, 1.1e-02, 8.5e-03, 6.9e-03, 4.9e-03),
                           moment=A6(1.9e-01, 1.9e-01, 8.2e-02, 8.1e-02, 5.2e-03, 4.8e-03),
                           tau_median=A6(3.9e+03, 7.4e+03, 5.1e+03, 7.9e+01, 1.8e+02, 8.0e+01)),
        },
        "plain": {
            "free": dict(qdd=A6(1.6e-04, 1.5e-04, 3.5e-04, 4.9e-04, 5.4e-04, 7.7e-04),
                           tau=A6(1.9e-01, 4.1e-02, 2.7e-02, 2.2e-03, 1.1e-03, 6.4e-04),
                           force=A6(1.1e-02, 1.1e-02, 1.1e-02, 8.5e-03, 6.9e-03, 4.9e-03),
                           moment=A6(1.9e-01, 1.9e-01, 8.2e-02, 8.1e-02, 5.2e-03, 4.8e-03),
                           tau_median=A6(3.9e+03, 7.4e+03, 5.1e+03, 7.9e+01, 1.8e+02, 8.0e+01)),
        },
    },
    "Dc": {
        "ext": {
            "free": dict(qdd=A6(1.4e-04, 1.5e-04, 3.4e-04, 6.2e-04, 5.8e-04, 1.1e-03),
                           tau=A6(1.9e-01, 4.1e-02, 2.6e-02, 3.4e-03, 1.3e-03, 6.4e-04),
                           force=A6(1.0e-02, 1.0e-02, 1.0e-02, 8.5e-03, 6.8e-03, 5.0e-03),
                           moment=A6(1.9e-01, 1.9e-01, 8.4e-02, 8.1e-02, 7.5e-03, 6.2e-03),
                           tau_median=A6(3.7e+03, 7.1e+03, 5.0e+03, 9.4e+01, 1.7e+02, 7.6e+01)),
            "contact": dict(qdd=A6(1.7e-04, 5.5e-04, 6.1e-04, 5.3e-03, 5.2e-03, 7.9e-03),
                              tau=A6(1.8e-01, 2.4e-01, 1.4e-01, 2.7e-02, 3.9e-02, 2.0e-02),
                              force=A6(2.4e-02, 2.3e-02, 2.1e-02, 1.4e-02, 1.4e-02, 1.1e-02),
                              moment=A6(2.7e-01, 2.4e-01, 1.4e-01, 1.3e-01, 3.9e-02, 3.5e-02),
                              tau_median=A6(4.6e+03, 6.6e+03, 5.5e+03, 1.1e+02, 1.8e+02, 8.3e+01)),
        },
        "wrench": {
            "free": dict(qdd=A6(1.4e-04, 1.5e-04, 3.4e-04, 6.2e-04, 5.8e-04, 1.1e-03),
                           tau=A6(1.9e-01, 4.1e-02, 2.6e-02, 3.1e-03, 1.3e-03, 6.7e-04),
                           force=A6(1.0e-02, 1.0e-02, 1.0e-02, 8.5e-03, 6.8e-03, 5.0e-03),
                           moment=A6(1.9e-01, 1.9e-01, 8.4e-02, 8.1e-02, 7.5e-03, 6.2e-03),
                           tau_median=A6(3.7e+03, 7.1e+03, 5.0e+03, 9.4e+01, 1.7e+02, 7.6e+01)),
            "contact": dict(qdd=A6(1.7e-04, 5.5e-04, 6.1e-04, 5.4e-03, 5.2e-03, 7.5e-03),
                              tau=A6(1.8e-01, 2.6e-01, 1.3e-01, 2.7e-02, 3.0e-02, 1.6e-02),
                              force=A6(2.3e-02, 2.4e-02, 2.0e-02, 1.8e-02, 2.3e-02, 1.3e-02),
                              moment=A6(2.5e-01, 2.6e-01, 1.3e-01, 1.5e-01, 3.0e-02, 3.0e-02),
                              tau_median=A6(4.6e+03, 6.6e+03, 5.5e+03, 1.1e+02, 1.8e+02, 8.3e+01)),
        },
        "torque": {
            "free": dict(qdd=A6(1.5e-04, 1.5e-04, 3.5e-04, 5.1e-04, 5.3e-04, 8.2e-04),
                           tau=A6(1.9e-01, 4.1e-02, 2.6e-02, 2.2e-03, 1.1e-03, 6.4e-04),
                           force=A6(1.0e-02, 1.0e-02, 1.0e-02, 8.6e-03, 6.8e-03, 4.9e-03),
                           moment=A6(1.9e-01, 1.9e-01, 8.4e-02, 8.1e-02, 4.9e-03, 4.4e-03),
                           tau_median=A6(3.7e+03, 7.1e+03, 5.0e+03, 9.4e+01, 1.7e+02, 7.6e+01)),
            "contact": dict(qdd=A6(1.7e-04, 5.5e-04, 6.1e-04, 4.7e-03, 4.2e-03, 6.6e-03),
                              tau=A6(1.8e-01, 4.1e-01, 1.5e-01, 2.7e-02, 2.8e-02, 2.0e-02),
                              force=A6(2.1e-02, 2.2e-02, 2.2e-02, 1.7e-02, 1.8e-02, 1.3e-02),
                              moment=A6(4.6e-01, 4.1e-01, 1.5e-01, 1.2e-01, 2.8e-02, 3.2e-02),
                              tau_median=A6(4.6e+03, 6.6e+03, 5.5e+03, 1.1e+02, 1.8e+02, 8.3e+01)),
        },
        "plain": {
            "free": dict(qdd=A6(1.5e-04, 1.5e-04, 3.5e-04, 5.1e-04, 5.3e-04, 8.2e-04),
                           tau=A6(1.9e-01, 4.1e-02, 2.6e-02, 2.2e-03, 1.2e-03, 6.4e-04),
                           force=A6(1.0e-02, 1.0e-02, 1.0e-02, 8.6e-03, 6.8e-03, 4.9e-03),
                           moment=A6(1.9e-01, 1.9e-01, 8.4e-02, 8.1e-02, 4.9e-03, 4.4e-03),
                           tau_median=A6(3.7e+03, 7.1e+03, 5.0e+03, 9.4e+01, 1.7e+02, 7.6e+01)),
            "contact": dict(qdd=A6(1.7e-04, 5.5e-04, 6.1e-04, 4.7e-03, 4.2e-03, 6.1e-03),
                              tau=A6(1.8e-01, 2.0e-01, 1.2e-01, 2.3e-02, 3.2e-02, 2.1e-02),
                              force=A6(1.9e-02, 2.0e-02, 1.9e-02, 1.5e-02, 1.5e-02, 1.1e-02),
                              moment=A6(2.7e-01, 2.0e-01, 1.2e-01, 1.1e-01, 3.2e-02, 3.5e-02),
                              tau_median=A6(4.6e+03, 6.6e+03, 5.5e+03, 1.1e+02, 1.8e+02, 8.3e+01)),
        },
    },
    "hold": {
        "ext": {
            "free": dict(qdd=A6(5.8e-07, 5.0e-07, 1.1e-06, 1.5e-05, 1.8e-05, 3.7e-05),
                           tau=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
                           force=A6(3.2e-05, 2.0e-05, 2.4e-05, 2.1e-05, 1.9e-05, 2.7e-05),
                           moment=A6(3.8e-04, 3.7e-04, 1.9e-04, 3.3e-04, 6.3e-05, 6.9e-05),
                           tau_median=A6(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)),
        },
    },
}
REACTION_AT_QDD = {
    "mixed": {
        "plain": {
            "free": dict(force=A6(3.0e-03, 3.0e-03, 3.0e-03, 2.5e-03, 1.9e-03, 1.8e-03),
                           moment=A6(6.2e-02, 5.1e-02, 2.8e-02, 2.6e-02, 2.9e-03, 2.7e-03)),
        },
    },
    "subset": {
        "plain": {
            "free": dict(force=A6(2.2e-03, 2.3e-03, 1.9e-03, 2.1e-03, 1.8e-03, 1.6e-03),
                           moment=A6(4.0e-02, 3.9e-02, 2.2e-02, 2.2e-02, 5.7e-03, 5.6e-03)),
        },
    },
    "scaled": {
        "plain": {
            "free": dict(force=A6(7.2e-03, 7.2e-03, 7.2e-03, 6.5e-03, 6.5e-03, 5.7e-03),
                           moment=A6(1.2e-01, 1.1e-01, 9.4e-02, 8.5e-02, 1.1e-02, 1.4e-02)),
        },
    },
}


def clamp_room(orc, I, qdd):
    """[n, 6]: how far inside its limits each joint ends the sub-step, q + h (qd + h q̈); <= 0: the integrator's clamp acts"""
    lo, hi = np.array(orc.p.r_lo[:], dtype=np.float64), np.array(orc.p.r_hi[:], dtype=np.float64)
    qn = np.asarray(I["q"], dtype=np.float64) + H * (np.asarray(I["qd"], dtype=np.float64) + H * qdd)
    return np.minimum(qn - lo, hi - qn)


CLAMP_MARGIN = 1e-3                                                   # rad: a joint that ends nearer to a limit is not compared with the step


MAX_SHARE = 1e-3                                                      # a bar is at most this share of its quantity's batch median magnitude


def bars(name, form, hit):
    """{quantity: [n, 6]}: what the kernel is allowed per env and joint on a family or on `hold`, in the call's form ("ext" |
    "wrench" | "torque" | "plain"); hit [n]: who is in contact.  FLOOR_MARGIN times the floor; the motor torque's bar is capped at
    MAX_SHARE of the torque's own batch median (tau_median), which binds where the torque is recovered from the reaction."""
    hit = np.asarray(hit, dtype=bool)
    F = FLOORS[name][form]
    free, contact = F["free"], F.get("contact", F["free"])
    allowed = lambda c: dict({k: FLOOR_MARGIN * c[k] for k in QUANTITIES}, tau=np.minimum(FLOOR_MARGIN * c["tau"], MAX_SHARE * c["tau_median"]))  # noqa: E731
    a, b = allowed(free), allowed(contact)
    return {k: np.where(hit[:, None], b[k][None], a[k][None]) for k in QUANTITIES}
