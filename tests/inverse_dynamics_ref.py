"""Independent float64 reference of pnr_inverse_dynamics and pnr_mass_matrix.  (pnr_world_step_torques' is
tests/world_step_ref.py's world_step(tau_ext=...): the forward dynamics of losses + motor law + tau_ext, directly.)

Built on the float64 oracle's forward dynamics alone (DynOracle.aba_ext, which tests/test_dyn_oracle.py validates); it reads
nothing of pioneer_amd and restates neither a mass-matrix algorithm nor an inverse-dynamics recursion:
  * M^-1 comes column by column from the ABA's affinity in tau (ABA(e_j) at qd = 0 without gravity), and M = inv(M^-1);
  * bias = C(q, qd) qd + G(q) = -M ABA(0, gravity);
  * tau = M qdd + bias, plus the engine's joint losses (world_step_ref.losses) when asked for.

newton_euler() is a SECOND statement of the same torques, from tests/golden/urdf_chain.json alone: a world-frame Newton-Euler
sweep over the 11 URDF links (mass s_l, inertia s_l 1 about the link frame origin), projected on the joint axes.  Every array
of it has the dtype it is called with: in float64 the CPU tests hold it against the ABA-based reference; in float32 it is the
"float32 floor" the GPU tests derive their tight bars from (what float32 arithmetic alone costs on the test's inputs).
"""
import numpy as np

import ik_ref
import link_kinematics_ref as lk
import world_step_ref as wref

DOF = 6
LINKS = 11


def aba(orc, tau, gravity):
    """qdd [n, 6] of the oracle's ABA at its current states: no contacts, motors, damping or friction."""
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (orc.n, DOF))
    return np.stack([orc.aba_ext(tau[e], gravity, None, e) for e in range(orc.n)])


def mass_and_bias(orc, gravity):
    """M [n, 6, 6], M^-1 [n, 6, 6] and bias = C qd + G [n, 6] at the oracle's current states.  M^-1 depends on q alone: its
    columns are taken at qd = 0 without gravity, where ABA(e_j) IS column j (no difference of two large accelerations)."""
    n = orc.n
    qdd0 = aba(orc, np.zeros(DOF), gravity)
    qd = orc.dstate["qd"].copy()
    orc.dstate["qd"] = 0.0
    Minv = np.empty((n, DOF, DOF))
    eye = np.eye(DOF)
    for j in range(DOF):
        Minv[:, :, j] = aba(orc, eye[j], 0.0)
    orc.dstate["qd"] = qd
    M = np.linalg.inv(Minv)
    return M, Minv, -np.einsum("nij,nj->ni", M, qdd0)


def inverse_dynamics(orc, qdd=None, gravity=0.0, joint_losses=False):
    """tau [n, 6] = M qdd + C qd + G (+ the joint losses)."""
    M, _, bias = mass_and_bias(orc, gravity)
    tau = bias if qdd is None else bias + np.einsum("nij,nj->ni", M, np.asarray(qdd, dtype=np.float64))
    return tau + wref.losses(orc) if joint_losses else tau


# ---- the second statement: world-frame Newton-Euler over the URDF links, in the caller's dtype -----------------------------------
def joints_upstream(chain):
    """per link, the number of revolute joints up to it"""
    idx = ik_ref.revolute_links(chain)[0]
    return [sum(k <= l for k in idx) for l in range(len(chain))]


def newton_euler(q, qd, qdd, scales, gravity, dtype=np.float64, chain=None):
    """tau [n, 6] in `dtype`: sum over the links l and their upstream joints j of
    (a_j x (p_l - o_j)) . s_l acc_l + a_j . s_l alpha_l   (mass 1 and inertia 1 per link, scaled; omega x I omega = 0)."""
    T = np.dtype(dtype).type
    chain = chain or lk.load_chain()
    q, qd, qdd, scales = (np.atleast_2d(np.asarray(x, dtype=T)) for x in (q, qd, qdd, scales))
    _, p, _, _, al, acc, axes, origins = lk.link_frames(q, qd, chain, qdd=qdd, gravity=gravity, dtype=T)
    tau = np.zeros((q.shape[0], DOF), dtype=T)
    for l, nj in enumerate(joints_upstream(chain)):
        s = scales[:, l:l + 1]
        F, N = s * acc[:, l], s * al[:, l]
        for j in range(nj):
            a, o = axes[:, j], origins[:, j]
            tau[:, j] += (np.cross(a, p[:, l] - o) * F).sum(axis=1) + (a * N).sum(axis=1)
    assert tau.dtype == np.dtype(dtype)
    return tau


def newton_euler_mass_matrix(q, scales, dtype=np.float64, chain=None):
    """M [n, 6, 6] in `dtype`: column j is newton_euler at qd = 0, no gravity, qdd = e_j."""
    q = np.atleast_2d(np.asarray(q, dtype=dtype))
    zero = np.zeros_like(q)
    cols = []
    for j in range(DOF):
        e = zero.copy()
        e[:, j] = 1
        cols.append(newton_euler(q, zero, e, scales, 0.0, dtype, chain))
    return np.stack(cols, axis=2)
