// pnr_invdyn.h — pnr_inverse_dynamics and pnr_mass_matrix: PyBullet's calculateInverseDynamics and calculateMassMatrix for
// every env, one launch each, on the rigid-body model the ABA of pnr_dyn.h steps (six merged bodies, per-env link scales).
// Included by pnr_queries.hip only, whose code object holds no step kernel.
//
// Shape of both: one env per lane, one 64-lane wave per workgroup (pnr_query.h).  The joints come through load_joints<SRC>;
// a dynamics-mode handle's link scales, friction and damping are read planar (plane w of env e at dyn[w * n + e]: consecutive
// lanes, consecutive words); a kinematic-mode handle has no such planes (dyn == null, a wave-uniform branch): scales 1 and the
// config's joint_damping / joint_friction as kernel arguments.  sin / cos by sincos_any: a caller's joints are unbounded.
//
// inverse_dynamics_kernel: recursive Newton-Euler (rnea below) on the ABA's own helpers.  Gravity and the two flags are
// wave-uniform kernel arguments — PNR_INVDYN_NO_GRAVITY is g = 0, PNR_INVDYN_JOINT_LOSSES a 0/1 gain on the loss terms — so
// there is one instantiation per joint source and none per flag.  Output 24 B per env: three plain float2 stores per lane, as
// the IK outputs (the wave's three stores cover one contiguous 1 536-B span, every line of it written whole by this wave).
//
// mass_matrix_kernel: mass_matrix() of pnr_dyn.h (the CRBA the constraint motor uses) gives the packed lower triangle; each
// value is written to both triangles of the env's row of the 6 x 6 LDS tile of pnr_query.h, which leaves through its flush.
#pragma once

#include <hip/hip_runtime.h>

#include "pnr_device.h"
#include "pnr_dyn.h"
#include "pnr_query.h"

// float32 against a float64 reference, tolerance-checked: let a*b+c fuse
#pragma clang fp contract(fast)

namespace pnr {

// I a for the spatial inertia of rigid_body<J>: (n_i, f_i) = sum_j (A_ij, C_ij) (a.a_j, a.l_j) + (B_ij, B_ji) (a.l_j, a.a_j).
// Bodies 0..4 are A = C = m 1, B = 0: one packed product per component.
template <int J>
__device__ __forceinline__ P3 inertia_times(const DynModel& M, const SIp& I, const P3& a)
{
    if constexpr (J < kDof - 1) {
        const float m = M.m[J];
        return {m * a.x, m * a.y, m * a.z};
    } else {
        P3 f;
        static_for<3>([&](auto i_) {
            constexpr int i = decltype(i_)::value;
            f2 acc = {0.f, 0.f};
            static_for<3>([&](auto j_) {
                constexpr int j = decltype(j_)::value;
                acc += I.ac[SIDX<i, j>] * pc<j>(a);
                if constexpr (i != j) acc += bpair<i, j>(I) * pc<j>(a).yx;      // B = skew(h): its diagonal is zero
            });
            pr<i>(f) = acc;
        });
        return f;
    }
}

// tau = M(q) qdd + C(q, qd) qd + G(q) by recursive Newton-Euler.  c, s: cos / sin of the joint angles.  gravity: along -z,
// entering as the base acceleration +g z (as pass 3 of aba).
//   outward: v_J = X v_parent + S qd_J,  a_J = X a_parent + v_J x (S qd_J) + S qdd_J
//   inward:  f_J = I_J a_J + p_J (+ the children's forces, carried by force_to_parent),  tau_J = S^T f_J
__device__ __forceinline__ void rnea(float gravity, const DynModel& M, const float (&c)[kDof], const float (&s)[kDof],
                                     const float (&qd)[kDof], const float (&qdd)[kDof], float (&tau)[kDof])
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
        constexpr int AXJ = (int)kJoints[J].axis;
        SIp I; P3 p;
        rigid_body<J>(M, v[J], I, p);
        const P3 f = inertia_times<J>(M, I, a[J]) + p + carried;
        tau[J] = pc<AXJ>(f).x;
        if constexpr (J > 0) carried = force_to_parent<J>(f, c[J], s[J]);
    });
}

// what both kernels read of an env: joints, link scales (and for the losses friction and damping)
template <int SRC, bool LOSSES>
__device__ __forceinline__ void invdyn_load(const float* __restrict__ src, const float4* __restrict__ state,
                                            const float* __restrict__ dyn, const long long n, const EnvLane& L,
                                            const float damping0, const float friction0, float (&q)[kDof], float (&qd)[kDof],
                                            float (&sc)[kNumLinks], float (&fric)[kDof], float (&damp)[kDof])
{
#pragma unroll
    for (int i = 0; i < kDof; ++i) { q[i] = 0.f; qd[i] = 0.f; fric[i] = friction0; damp[i] = damping0; }
#pragma unroll
    for (int l = 0; l < kNumLinks; ++l) sc[l] = 1.0f;
    if (!L.live) return;                                              // ONE branch around every load: not load_lane_joints
    const long long e = L.e;
    load_joints<SRC>(src, state, n, e, q, qd);
    if (dyn) {                                                        // wave-uniform: a dynamics-mode handle
#pragma unroll
        for (int l = 0; l < kNumLinks; ++l) sc[l] = dyn[(long long)(kDynScale + l) * n + e];
        if (LOSSES) {
#pragma unroll
            for (int i = 0; i < kDof; ++i) {
                fric[i] = dyn[(long long)(kDynFric + i) * n + e];
                damp[i] = dyn[(long long)(kDynDamp + i) * n + e];
            }
        }
    }
}

struct InvDynArgs {
    const float* src;          // caller's [n][12], or the handle's dyn words (SRC)
    const float4* state;       // kinematic-mode state planes (kJointSrcKin only)
    const float* dyn;          // the handle's dyn words [36][n] (link scales, friction, damping), or null: kinematic mode
    const float* accel;        // [n][6] or null: qdd = 0
    float* out;                // [n][6], 16-byte aligned
    long long n;
    float gravity;             // 0 with PNR_INVDYN_NO_GRAVITY
    float loss_gain;           // 1 with PNR_INVDYN_JOINT_LOSSES, else 0
    float damping0, friction0; // kinematic mode: the config's joint_damping / joint_friction
};

template <int SRC>
__global__ __launch_bounds__(kWave) void inverse_dynamics_kernel(const InvDynArgs A)
{
    const EnvLane L = env_lane(A.n);
    float q[kDof], qd[kDof], sc[kNumLinks], fric[kDof], damp[kDof], qdd[kDof];
    invdyn_load<SRC, true>(A.src, A.state, A.dyn, A.n, L, A.damping0, A.friction0, q, qd, sc, fric, damp);
#pragma unroll
    for (int i = 0; i < kDof; ++i) qdd[i] = 0.f;
    if (L.live && A.accel) {
        const float2* a2 = reinterpret_cast<const float2*>(A.accel) + 3 * L.e;
        const float2 x0 = a2[0], x1 = a2[1], x2 = a2[2];
        qdd[0] = x0.x; qdd[1] = x0.y; qdd[2] = x1.x; qdd[3] = x1.y; qdd[4] = x2.x; qdd[5] = x2.y;
    }
    DynModel M;
    build_model(sc, M);
    float c[kDof], s[kDof];
#pragma unroll
    for (int i = 0; i < kDof; ++i) sincos_any(q[i], s[i], c[i]);
    float tau[kDof];
    rnea(A.gravity, M, c, s, qd, qdd, tau);
#pragma unroll
    for (int i = 0; i < kDof; ++i) {                                  // the engine's joint losses (dyn_core's terms, sign turned)
        const float loss = damp[i] * qd[i] + fric[i] * qd[i] * __builtin_amdgcn_rsqf(qd[i] * qd[i] + kFrictionEps * kFrictionEps);
        tau[i] += A.loss_gain * loss;
    }
    if (!L.live) return;
    float2* o = reinterpret_cast<float2*>(A.out) + 3 * L.e;
    o[0] = make_float2(tau[0], tau[1]); o[1] = make_float2(tau[2], tau[3]); o[2] = make_float2(tau[4], tau[5]);
}

template <int SRC>
__global__ __launch_bounds__(kWave) void mass_matrix_kernel(const float* __restrict__ src, const float4* __restrict__ state,
                                                            const float* __restrict__ dyn, float* __restrict__ out, const long long n)
{
    __shared__ __attribute__((aligned(16))) float tile[kMat6TileFloats];
    const EnvLane L = env_lane(n);
    float q[kDof], qd[kDof], sc[kNumLinks], fric[kDof], damp[kDof];
    invdyn_load<SRC, false>(src, state, dyn, n, L, 0.f, 0.f, q, qd, sc, fric, damp);
    DynModel M;
    build_model(sc, M);
    float c[kDof], s[kDof];
#pragma unroll
    for (int i = 0; i < kDof; ++i) sincos_any(q[i], s[i], c[i]);
    float H[kTri];
    mass_matrix(M, c, s, H);
    float* row = tile + L.lane * kMat6RowStride;
    static_for<kDof>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        static_for<kDof>([&](auto j_) {
            constexpr int j = decltype(j_)::value;
            row[kDof * i + j] = H[TRI<i, j>];                         // one computed value for both triangles
        });
    });
    wave_lds_sync();
    flush_mat6_tile(tile, out + L.tile0 * kMat6Dim, L.nvalid, L.lane);
}

}  // namespace pnr

#pragma clang fp contract(off)
