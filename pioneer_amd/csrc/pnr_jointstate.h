// pnr_jointstate.h — pnr_get_joint_states: PyBullet's getJointState for every env of a dynamics-mode handle, one launch: per
// revolute joint q, qd, the acceleration qdd and the motor torque, and optionally the joint's reaction wrench.  The call LOOKS AT
// the first sub-step of pnr_world_step / _torques / _wrenches with the same arguments and takes nothing: no state word is written.
// Included by pnr_queries.hip only, whose code object holds no step kernel.
//
// Shape: one env per lane, one 64-lane wave per workgroup (pnr_query.h).  Per lane
//   1. joints (the caller's [n][12] or the handle's planes: a wave-uniform run-time branch, not a template argument, which
//      halves the instantiations of a kernel that holds a whole ABA), link scales, friction, damping, the command state r, v;
//   2. the motor law of one sub-step (motor_law, pnr_dyn.h: dyn_core's), keeping the law's own torque and the joint losses apart;
//   3. the external body forces: the caller's records (wrench_prepare / wrench_forces at the current pose, which is that call's
//      q0) and the penalty contacts (contact_wrenches), added into one fext[6] HERE and handed to aba<.., EXT = true> as external
//      forces.  aba then runs without its own contact code: fext[b] is subtracted from body b's bias force either way, so the
//      arithmetic is that of aba<PHYS | 1, EXT>, the contacts are evaluated once, and the sweep below reads the same fext;
//   4. aba, and motor_constraints where the table holds constraint motors: qdd, before the integrator and its limit clamp;
//   5. an inward Newton-Euler sweep in body frames at that qdd, as rnea (pnr_invdyn.h) but keeping each body's whole spatial
//      force and with fext subtracted: f_b = I_b a_b + p_b - fext_b + X^T f_(b+1).  f_b is the wrench the parent exerts on body
//      b through joint b, about body b's origin, in body b's coordinates; its moment along the joint axis is the joint's total
//      torque;
//   6. the motor torque: a PD joint's table law after its cap is written as evaluated in 2.  The inertia-scaled law's
//      clip(D_i ades_i, +-tcap) and the boxed solve's torque are formed inside aba / motor_constraints and not handed out:
//      there tau_motor = (axis moment of f_b) - joint_torque + damping + friction, the identity of include/pioneer_amd.h;
//   7. stores: joints_out's 24 floats per env as six plain float4 stores per lane (the wave's stores cover one contiguous
//      6 144-B span, every 128-B line of it written whole by this wave: nothing to gain from a trip through LDS, and the
//      mass-matrix tile's 9.5 KB stay free); reaction_out's 36 floats through the 6 x 6 LDS tile and flush_mat6_tile.
// sin / cos by sincos_any: a caller's joints are unbounded.  No scratch; registers: DESIGN.md 3n.
#pragma once

#include <hip/hip_runtime.h>

#include "pnr_device.h"
#include "pnr_dyn.h"
#include "pnr_query.h"
#include "pnr_invdyn.h"

// float32 against a float64 reference, tolerance-checked: let a*b+c fuse
#pragma clang fp contract(fast)

namespace pnr {

struct JointStateArgs {
    const float* joints_in;    // caller's [n][12] (q | qd), or null: the handle's own planes
    const float4* state;       // the handle's state records: the command state r, v
    const float* dyn;          // the handle's dyn words [36][n]
    const float* tau_ext;      // [n][6] or null
    const float* wrenches;     // [n][T.n][9] or null (EXT only)
    float* joints;             // [n][6][4], 16-byte aligned
    float* reaction;           // [n][6][6], 16-byte aligned, or null: not computed
    long long n;
};

// f[b]: the spatial force body b's joint transmits (see 5. above), at the accelerations qdd, with the external forces fext
// (body coordinates, as aba takes them) subtracted
template <bool EXTF>
__device__ __forceinline__ void reaction_sweep(float gravity, const DynModel& M, const float (&c)[kDof], const float (&s)[kDof],
                                               const float (&qd)[kDof], const float (&qdd)[kDof], const P3 (&fext)[kDof],
                                               P3 (&f)[kDof])
{
    P3 v[kDof], a[kDof];
    const P3 v0 = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
    const P3 a0 = {{0.f, 0.f}, {0.f, 0.f}, {0.f, gravity}};
    static_for<kDof>([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        constexpr int AXJ = (int)kJoints[J].axis;
        if constexpr (J == 0) {
            vel_outward<J>(v0, c[J], s[J], qd[J], v[J]);
            a[J] = to_child<J>(a0, c[J], s[J]) + cross_axis<AXJ>(v[J], qd[J]);
        } else {
            vel_outward<J>(v[J - 1], c[J], s[J], qd[J], v[J]);
            a[J] = to_child<J>(a[J - 1], c[J], s[J]) + cross_axis<AXJ>(v[J], qd[J]);
        }
        pr<AXJ>(a[J]).x += qdd[J];
    });
    P3 carried = v0;                                                  // the children's force, in body J's frame
    static_for<kDof>([&](auto t_) {
        constexpr int J = kDof - 1 - decltype(t_)::value;
        SIp I; P3 p;
        rigid_body<J>(M, v[J], I, p);
        P3 fj = inertia_times<J>(M, I, a[J]) + p + carried;
        if constexpr (EXTF) fj = fj - fext[J];
        f[J] = fj;
        if constexpr (J > 0) carried = force_to_parent<J>(fj, c[J], s[J]);
    });
}

// PHYS: bit 0 contacts, bit 1 the inertia-scaled motor (the world step's dyn_phys).  CMOTOR: the table holds a constraint motor.
// EXT: the caller brought joint torques or wrench records (never with CMOTOR: the host refuses, as the world step does).
template <int PHYS, bool CMOTOR, bool EXT>
__global__ __launch_bounds__(kWave) void joint_state_kernel(const JointStateArgs A, const DynParams D, const JointMotorTable W,
                                                            const LinkWrenchTable T)
{
    constexpr bool CONTACT = (PHYS & 1) != 0, SCALED = (PHYS & 2) != 0;
    constexpr bool EXTF = CONTACT || EXT;                             // any external body force at all
    __shared__ __attribute__((aligned(16))) float tile[kMat6TileFloats];
    const EnvLane L = env_lane(A.n);
    const long long n = A.n;

    // 1. everything the lane reads, behind ONE branch (a lane past the batch computes on a rest pose and stores nothing)
    float q[kDof], qd[kDof], r[kDof], v[kDof], sc[kNumLinks], fric[kDof], damp[kDof], tx[kDof];
    [[maybe_unused]] WrenchLane XL;
#pragma unroll
    for (int i = 0; i < kDof; ++i) { q[i] = 0.f; qd[i] = 0.f; r[i] = 0.f; v[i] = 0.f; fric[i] = 0.f; damp[i] = 0.f; tx[i] = 0.f; }
#pragma unroll
    for (int l = 0; l < kNumLinks; ++l) sc[l] = 1.0f;
    if constexpr (EXT) {
        static_for<kMaxWrench>([&](auto j_) {
            constexpr int j = decltype(j_)::value;
#pragma unroll
            for (int i = 0; i < 9; ++i) XL.w[j][i] = 0.f;
        });
    }
    if (L.live) {
        const long long e = L.e;
        if (A.joints_in) load_joints<kJointSrcBuffer>(A.joints_in, nullptr, n, e, q, qd);       // (wave-uniform)
        else load_joints<kJointSrcDyn>(A.dyn, nullptr, n, e, q, qd);
        HalfRec k[2];
        load_env_halves(A.state, n, e, 0, k);
        float a[kDof];
#pragma unroll
        for (int p = 0; p < 2; ++p) unpack_record(k[p], a + 3 * p, v + 3 * p, r + 3 * p);
#pragma unroll
        for (int i = 0; i < kDof; ++i) {
            fric[i] = A.dyn[(long long)(kDynFric + i) * n + e];
            damp[i] = A.dyn[(long long)(kDynDamp + i) * n + e];
        }
#pragma unroll
        for (int l = 0; l < kNumLinks; ++l) sc[l] = A.dyn[(long long)(kDynScale + l) * n + e];
        if constexpr (EXT) {
            if (A.tau_ext) load_joint_torques(A.tau_ext, e, tx);
            if (A.wrenches) load_wrench_records(A.wrenches, T, e, XL);
        }
    }

    DynModel M;
    build_model(sc, M);
    float c[kDof], s[kDof];
#pragma unroll
    for (int i = 0; i < kDof; ++i) sincos_any(q[i], s[i], c[i]);

    // 2. the motor law of one sub-step: tau = what aba receives, law = the joint's own motor in it
    float tau[kDof], ades[kDof], tc[kDof], law[kDof], loss[kDof];
#pragma unroll
    for (int i = 0; i < kDof; ++i) {
        const bool cmd = W.from_cmd[i];
        const float rr = cmd ? r[i] : W.r_ref[i], vr = cmd ? v[i] : W.v_ref[i];
        tc[i] = W.tcap[i];
        float tq = motor_law<SCALED>(rr, vr, q[i], qd[i], W.kp[i], W.kd[i], W.cpos[i], W.vcap[i], tc[i], ades[i]);
        if constexpr (CMOTOR) {
            if (W.kind[i] != kMotorPD) { ades[i] = 0.f; tq = 0.f; }
        }
        law[i] = tq;
        if constexpr (EXT) tq += tx[i];
        loss[i] = damp[i] * qd[i] + fric[i] * qd[i] * __builtin_amdgcn_rsqf(qd[i] * qd[i] + kFrictionEps * kFrictionEps);
        tau[i] = tq - loss[i];
    }

    // 3. the external body forces, contacts included
    P3 fx[kDof];
#pragma unroll
    for (int i = 0; i < kDof; ++i) fx[i] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
    if constexpr (EXT) {
        if (A.wrenches) {                                             // (wave-uniform)
            wrench_prepare(T, c, s, XL);
            wrench_forces(T, c, s, XL, fx);
        }
    }
    if constexpr (CONTACT) {
        P3 vb[kDof];
        const P3 v0 = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
        vel_outward<0>(v0, c[0], s[0], qd[0], vb[0]);
        vel_outward<1>(vb[0], c[1], s[1], qd[1], vb[1]);
        vel_outward<2>(vb[1], c[2], s[2], qd[2], vb[2]);
        vel_outward<3>(vb[2], c[3], s[3], qd[3], vb[3]);
        vel_outward<4>(vb[3], c[4], s[4], qd[4], vb[4]);
        vel_outward<5>(vb[4], c[5], s[5], qd[5], vb[5]);
        contact_wrenches(D, c, s, vb, fx);
    }

    // 4. the acceleration the sub-step would integrate
    float qdd[kDof];
    if constexpr (EXTF) aba<PHYS & 2, true>(D, M, c, s, qd, tau, ades, tc, qdd, fx);
    else aba<PHYS & 2>(D, M, c, s, qd, tau, ades, tc, qdd);
    if constexpr (CMOTOR) motor_constraints(D, M, c, s, q, qd, W, 1.0f / D.dt_sub, qdd);

    // 5. + 6. the reaction sweep; the motor torques it alone knows
    constexpr bool RECOVER = SCALED || CMOTOR;
    float tm[kDof];
#pragma unroll
    for (int i = 0; i < kDof; ++i) tm[i] = law[i];
    if (RECOVER || A.reaction) {                                      // (wave-uniform)
        P3 f[kDof];
        reaction_sweep<EXTF>(D.gravity, M, c, s, qd, qdd, fx, f);
        if constexpr (RECOVER) {
            static_for<kDof>([&](auto i_) {
                constexpr int i = decltype(i_)::value;
                const float total = pc<(int)kJoints[i].axis>(f[i]).x;
                const bool direct = !SCALED && W.kind[i] == kMotorPD;  // (wave-uniform) a capped table law is known exactly
                if (!direct) tm[i] = total - tx[i] + loss[i];
            });
        }
        if (A.reaction) {
            float* row = tile + L.lane * kMat6RowStride;
            static_for<kDof>([&](auto b_) {
                constexpr int b = decltype(b_)::value;
                const V3 F = lin(f[b]), Mo = ang(f[b]);
                row[6 * b + 0] = F.x; row[6 * b + 1] = F.y; row[6 * b + 2] = F.z;
                row[6 * b + 3] = Mo.x; row[6 * b + 4] = Mo.y; row[6 * b + 5] = Mo.z;
            });
            wave_lds_sync();
            flush_mat6_tile(tile, A.reaction + L.tile0 * kMat6Dim, L.nvalid, L.lane);
        }
    }

    // 7. q, qd, qdd, tau_motor
    if (!L.live) return;
    float4* o = reinterpret_cast<float4*>(A.joints) + kDof * L.e;
#pragma unroll
    for (int i = 0; i < kDof; ++i) o[i] = make_float4(q[i], qd[i], qdd[i], tm[i]);
}

}  // namespace pnr

#pragma clang fp contract(off)
