// pnr_ik.h — pnr_get_jacobian, pnr_solve_ik, pnr_solve_ik_pose and pnr_solve_ik_multi: the Jacobian of a point of a URDF link (PyBullet's
// calculateJacobian), position-only damped-least-squares inverse kinematics (calculateInverseKinematics without an orientation)
// and pose inverse kinematics (with targetOrientation: a full orientation or one axis to point) for every env, one launch each;
// multi-start inverse kinematics (either law from S starts per env, the nearest solution found) at the end of the file.
// Included by pnr_queries.hip only, whose code object holds no step kernel.
//
// Shape of all but the multi-start kernels: one env per lane, one 64-lane wave per workgroup (pnr_query.h).  The host resolves (link,
// local_point) into the moving body that carries the link and the point's offset in that body's frame; both arrive as
// kernel arguments, so every `J <= body` test below is a scalar branch.
//
// jacobian_kernel: one outward sweep (pose_outward) gives each joint's world axis a_j and origin o_j and the point; column j
// is a_j x (point - o_j) | a_j.  The 36 floats of an env go into the 6 x 6 LDS tile of pnr_query.h and leave through its flush.
//
// ik_kernel: q[6], the six sin/cos pairs, the 18 entries of the linear Jacobian and the 3 x 3 system live in registers; the
// loop's trip count is the wave-uniform max_iterations, a converged lane is frozen by selects, and the wave leaves early once
// a ballot finds every lane frozen.  The pose code exists ONCE in the loop (the residual of the result is the loop's own last
// pose), so a lane's arithmetic does not depend on how many trips its neighbours need: results are bit-identical whatever
// the batch around an env.  Outputs are 32 B per env: plain per-lane stores (three float2 of q, one float, one int).
//
// ik_pose_kernel: ik_kernel's shape with a 6 x 6 system.  The target's rotation matrix is formed once from the normalised
// quaternion; per trip chain_jacobian also hands out the carrying body's rotation R (= the link's: every fixed joint has rpy 0),
// the rotation still to make comes as its sine vector s and cosine c (FULL: s = 1/2 sum_k r_k x t_k over the columns of R and
// R_target, c = (trace - 1) / 2; AXIS: s = u x v, c = u . v), angle = atan2(|s|, c), e_o = s angle / max(|s|, 1e-12): where
// the axis cannot be formed (half a turn, opposite vectors) the orientation step is zero and everything stays finite.  The
// orientation weight is folded into the angular rows once; the 21 unique entries of J J^T + lambda^2 I are summed joint by
// joint and solved by an unrolled L D L^T whose pivots are held at >= lambda^2 (their exact-arithmetic floor: float32 rounding
// of a near-singular J J^T must not make one zero or negative).  Outputs are 36 B per env.
#pragma once

#include <hip/hip_runtime.h>

#include "pnr_device.h"
#include "pnr_dyn.h"
#include "pnr_query.h"

// float32 against a float64 reference, tolerance-checked: let a*b+c fuse
#pragma clang fp contract(fast)

namespace pnr {

// the point a Jacobian or an IK solve is about: offset `off` in the frame of moving body `body` (-1: the static base)
struct ChainPoint { int body; float ox, oy, oz; };

// The chain's Jacobian at the joint angles whose cosines / sines are c, s: per joint J <= body the world axis (ang) and
// axis x (point - origin) (lin); exactly zero for the joints beyond the body.  point: the point's world position.
// Rbody, where asked for: the body's world rotation (the identity for the static base).
__device__ __forceinline__ void chain_jacobian(const float (&c)[kDof], const float (&s)[kDof], const ChainPoint& P,
                                               V3 (&lin)[kDof], V3 (&ang)[kDof], V3& point, M3* Rbody = nullptr)
{
    const V3 off = {P.ox, P.oy, P.oz};
    V3 org[kDof];
    M3 R = diag3(1.f);
    V3 p = {0.f, 0.f, 0.f};
    point = off;
    static_for<kDof>([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        ang[J] = {0.f, 0.f, 0.f};
        org[J] = {0.f, 0.f, 0.f};
        if (J <= P.body) {
            M3 Rn; V3 pn;
            pose_outward<J>(R, p, c[J], s[J], Rn, pn);
            R = Rn; p = pn;
            ang[J] = col(R, (int)kJoints[J].axis);
            org[J] = p;
            if (J == P.body) point = p + mul(R, off);
        }
    });
    static_for<kDof>([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        lin[J] = {0.f, 0.f, 0.f};
        if (J <= P.body) lin[J] = cross(ang[J], point - org[J]);
    });
    if (Rbody) *Rbody = R;
}

template <int SRC>
__global__ __launch_bounds__(kWave) void jacobian_kernel(const float* __restrict__ src, const float4* __restrict__ state,
                                                         float* __restrict__ out, const long long n, const ChainPoint P)
{
    __shared__ __attribute__((aligned(16))) float tile[kMat6TileFloats];
    const EnvLane L = env_lane(n);
    float q[kDof], qd[kDof];
    load_lane_joints<SRC>(src, state, n, L, q, qd);
    float c[kDof], s[kDof];
#pragma unroll
    for (int i = 0; i < kDof; ++i) sincos_any(q[i], s[i], c[i]);       // any finite joint value, as pnr_get_link_states
    V3 lin[kDof], ang[kDof], point;
    chain_jacobian(c, s, P, lin, ang, point);
    float* row = tile + L.lane * kMat6RowStride;
    static_for<kDof>([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        row[J] = lin[J].x; row[kDof + J] = lin[J].y; row[2 * kDof + J] = lin[J].z;
        row[3 * kDof + J] = ang[J].x; row[4 * kDof + J] = ang[J].y; row[5 * kDof + J] = ang[J].z;
    });
    wave_lds_sync();
    flush_mat6_tile(tile, out + L.tile0 * kMat6Dim, L.nvalid, L.lane);
}

struct IkArgs {
    const float* target;       // [n][3], or null: the env's own target (state words 18-20)
    const float4* state;       // the handle's state planes (read only when target is null)
    const float* q_init;       // [n][6], or null: the rest pose
    float* q_out;              // [n][6], 8-byte aligned
    float* residual;           // [n] or null
    int* iterations;           // [n] or null
    long long n;
    ChainPoint point;
    int max_iter;
    float lambda2, max_step, tol;
};

// The iteration law of include/pioneer_amd.h (pnr_solve_ik), one env per lane.
__global__ __launch_bounds__(kWave) void ik_kernel(const IkArgs A)
{
    const long long e = (long long)blockIdx.x * kWave + threadIdx.x;
    const bool live = e < A.n;
    float q[kDof];
    V3 tgt = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < kDof; ++i) q[i] = 0.f;
    if (live) {
        if (A.target) { const float* t = A.target + 3 * e; tgt = {t[0], t[1], t[2]}; }
        else { const float4 w = state_cold(A.state, A.n)[e]; tgt = {w.x, w.y, w.z}; }
        if (A.q_init) {
            const float* qi = A.q_init + kDof * e;
#pragma unroll
            for (int i = 0; i < kDof; ++i) q[i] = qi[i];
        }
    }
    static_for<kDof>([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        q[J] = fminf(fmaxf(q[J], limit_lo(J)), limit_hi(J));
    });
    bool frozen = !live;
    int iters = 0;
    float dist = 0.f;
    for (int it = 0; ; ++it) {
        float c[kDof], s[kDof];
#pragma unroll
        for (int i = 0; i < kDof; ++i) sincos_bounded(q[i], s[i], c[i]);     // q is inside the limits
        V3 lin[kDof], ang[kDof], point;
        chain_jacobian(c, s, A.point, lin, ang, point);
        const V3 err = tgt - point;
        dist = sqrtf(dot(err, err));
        if (it == A.max_iter) break;                                         // the pose of the result: its residual
        frozen = frozen || dist <= A.tol;
        if (__builtin_amdgcn_ballot_w64(!frozen) == 0) break;
        // A = J J^T + lambda^2 I (symmetric positive definite: every pivot below is >= lambda^2), solved as L D L^T
        float a00 = A.lambda2, a01 = 0.f, a02 = 0.f, a11 = A.lambda2, a12 = 0.f, a22 = A.lambda2;
        static_for<kDof>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            const V3 g = lin[J];
            a00 += g.x * g.x; a01 += g.x * g.y; a02 += g.x * g.z;
            a11 += g.y * g.y; a12 += g.y * g.z; a22 += g.z * g.z;
        });
        const float i0 = fast_rcp(a00);
        const float l10 = a01 * i0, l20 = a02 * i0;
        const float d1 = a11 - l10 * a01, u12 = a12 - l20 * a01;
        const float i1 = fast_rcp(d1);
        const float l21 = u12 * i1;
        const float d2 = a22 - l20 * a02 - l21 * u12;
        const float i2 = fast_rcp(d2);
        const float z0 = err.x, z1 = err.y - l10 * z0, z2 = err.z - l20 * z0 - l21 * z1;
        const float y2 = z2 * i2, y1 = z1 * i1 - l21 * y2, y0 = z0 * i0 - l10 * y1 - l20 * y2;
        const V3 y = {y0, y1, y2};
        float dq[kDof], big = 0.f;
        static_for<kDof>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            dq[J] = dot(lin[J], y);
            big = fmaxf(big, fabsf(dq[J]));
        });
        const float scale = big > A.max_step ? A.max_step * fast_rcp(big) : 1.f;
        static_for<kDof>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            const float qn = fminf(fmaxf(q[J] + scale * dq[J], limit_lo(J)), limit_hi(J));
            q[J] = frozen ? q[J] : qn;
        });
        iters += frozen ? 0 : 1;
    }
    if (!live) return;
    float2* qo = reinterpret_cast<float2*>(A.q_out) + 3 * e;
    qo[0] = make_float2(q[0], q[1]); qo[1] = make_float2(q[2], q[3]); qo[2] = make_float2(q[4], q[5]);
    if (A.residual) A.residual[e] = dist;
    if (A.iterations) A.iterations[e] = iters;
}

struct IkPoseArgs {
    const float* target;       // [n][3], or null: the env's own target (state words 18-20)
    const float4* state;       // the handle's state planes (read only when target is null)
    const float* quat;         // [n][4] x, y, z, w; normalised here
    const float* q_init;       // [n][6], or null: the rest pose
    float* q_out;              // [n][6], 8-byte aligned
    float* residual;           // [n] or null
    float* angle;              // [n] or null
    int* iterations;           // [n] or null
    long long n;
    ChainPoint point;
    int max_iter, axis_mode;   // axis_mode: PNR_IK_ORIENT_AXIS (align `axis` only), else the full orientation
    V3 axis;                   // unit, in the link's frame
    float damping2, error_damping, weight, max_step, tol, angle_tol;
};

constexpr float kIkSineFloor = 1e-12f;                           // below it the rotation axis is not formed: a zero step
template <int I, int J> constexpr int kLow = I * (I + 1) / 2 + J;   // entry (I, J <= I) of a packed lower triangle

// The iteration law of include/pioneer_amd.h (pnr_solve_ik_pose), one env per lane.
__global__ __launch_bounds__(kWave) void ik_pose_kernel(const IkPoseArgs A)
{
    constexpr int kPose = 6, kTriN = kPose * (kPose + 1) / 2;
    const long long e = (long long)blockIdx.x * kWave + threadIdx.x;
    const bool live = e < A.n;
    float q[kDof];
    V3 tgt = {0.f, 0.f, 0.f};
    float qx = 0.f, qy = 0.f, qz = 0.f, qw = 1.f;
#pragma unroll
    for (int i = 0; i < kDof; ++i) q[i] = 0.f;
    if (live) {
        if (A.target) { const float* t = A.target + 3 * e; tgt = {t[0], t[1], t[2]}; }
        else { const float4 w = state_cold(A.state, A.n)[e]; tgt = {w.x, w.y, w.z}; }
        const float* tq = A.quat + 4 * e;
        qx = tq[0]; qy = tq[1]; qz = tq[2]; qw = tq[3];
        if (A.q_init) {
            const float* qi = A.q_init + kDof * e;
#pragma unroll
            for (int i = 0; i < kDof; ++i) q[i] = qi[i];
        }
    }
    static_for<kDof>([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        q[J] = fminf(fmaxf(q[J], limit_lo(J)), limit_hi(J));
    });
    // the target's rotation, columns t0 t1 t2 (the quaternion's sign cancels in every product); in AXIS mode only v = R_target a
    const float qinv = 1.0f / sqrtf(qx * qx + qy * qy + qz * qz + qw * qw);
    qx *= qinv; qy *= qinv; qz *= qinv; qw *= qinv;
    const V3 t0 = {1.f - 2.f * (qy * qy + qz * qz), 2.f * (qx * qy + qz * qw), 2.f * (qx * qz - qy * qw)};
    const V3 t1 = {2.f * (qx * qy - qz * qw), 1.f - 2.f * (qx * qx + qz * qz), 2.f * (qy * qz + qx * qw)};
    const V3 t2 = {2.f * (qx * qz + qy * qw), 2.f * (qy * qz - qx * qw), 1.f - 2.f * (qx * qx + qy * qy)};
    const V3 tv = A.axis.x * t0 + A.axis.y * t1 + A.axis.z * t2;
    bool frozen = !live;
    int iters = 0;
    float dist = 0.f, angle = 0.f;
    for (int it = 0; ; ++it) {
        float c[kDof], s[kDof];
#pragma unroll
        for (int i = 0; i < kDof; ++i) sincos_bounded(q[i], s[i], c[i]);     // q is inside the limits
        V3 lin[kDof], ang[kDof], point;
        M3 R;
        chain_jacobian(c, s, A.point, lin, ang, point, &R);
        const V3 err = tgt - point;
        const float dist2 = dot(err, err);
        dist = sqrtf(dist2);
        V3 sv;
        float cs;
        if (A.axis_mode) {
            const V3 u = mul(R, A.axis);
            sv = cross(u, tv); cs = dot(u, tv);
        } else {
            const V3 r0 = col(R, 0), r1 = col(R, 1), r2 = col(R, 2);
            sv = 0.5f * (cross(r0, t0) + cross(r1, t1) + cross(r2, t2));
            cs = 0.5f * (dot(r0, t0) + dot(r1, t1) + dot(r2, t2) - 1.f);
        }
        const float sn = sqrtf(dot(sv, sv));
        angle = atan2f(sn, cs);
        if (it == A.max_iter) break;                                         // the pose of the result: its residuals
        frozen = frozen || (dist <= A.tol && angle <= A.angle_tol);
        if (__builtin_amdgcn_ballot_w64(!frozen) == 0) break;
        // e = [e_p ; w e_o], rows g[J] = column J of [J_lin ; w J_ang]
        const float wa = A.weight * angle;
        const float ko = wa * fast_rcp(fmaxf(sn, kIkSineFloor));
        const float er[kPose] = {err.x, err.y, err.z, ko * sv.x, ko * sv.y, ko * sv.z};
        const float lambda2 = A.damping2 + A.error_damping * (dist2 + wa * wa);
        float g[kDof][kPose];
        static_for<kDof>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            g[J][0] = lin[J].x; g[J][1] = lin[J].y; g[J][2] = lin[J].z;
            g[J][3] = A.weight * ang[J].x; g[J][4] = A.weight * ang[J].y; g[J][5] = A.weight * ang[J].z;
        });
        // a = J J^T + lambda^2 I, its lower triangle: symmetric positive definite, every pivot of L D L^T >= lambda^2
        float a[kTriN];
        static_for<kPose>([&](auto ic) {
            constexpr int I = decltype(ic)::value;
            static_for<I + 1>([&](auto kc) {
                constexpr int K = decltype(kc)::value;
                float sum = I == K ? lambda2 : 0.f;
                static_for<kDof>([&](auto jc) { constexpr int J = decltype(jc)::value; sum += g[J][I] * g[J][K]; });
                a[kLow<I, K>] = sum;
            });
        });
        float u[kTriN], l[kTriN], inv[kPose];                                // u_ik = l_ik d_k
        static_for<kPose>([&](auto kc) {
            constexpr int K = decltype(kc)::value;
            float d = a[kLow<K, K>];
            static_for<K>([&](auto mc_) { constexpr int M = decltype(mc_)::value; d -= l[kLow<K, M>] * u[kLow<K, M>]; });
            inv[K] = fast_rcp(fmaxf(d, lambda2));
            static_for<kPose>([&](auto ic) {
                constexpr int I = decltype(ic)::value;
                if constexpr (I > K) {
                    float t = a[kLow<I, K>];
                    static_for<K>([&](auto mc_) { constexpr int M = decltype(mc_)::value; t -= l[kLow<I, M>] * u[kLow<K, M>]; });
                    u[kLow<I, K>] = t;
                    l[kLow<I, K>] = t * inv[K];
                }
            });
        });
        float z[kPose], y[kPose];
        static_for<kPose>([&](auto ic) {
            constexpr int I = decltype(ic)::value;
            z[I] = er[I];
            static_for<I>([&](auto mc_) { constexpr int M = decltype(mc_)::value; z[I] -= l[kLow<I, M>] * z[M]; });
        });
        static_for<kPose>([&](auto ic) {
            constexpr int I = kPose - 1 - decltype(ic)::value;
            y[I] = z[I] * inv[I];
            static_for<kPose>([&](auto mc_) {
                constexpr int M = decltype(mc_)::value;
                if constexpr (M > I) y[I] -= l[kLow<M, I>] * y[M];
            });
        });
        float dq[kDof], big = 0.f;
        static_for<kDof>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            dq[J] = 0.f;
            static_for<kPose>([&](auto ic) { constexpr int I = decltype(ic)::value; dq[J] += g[J][I] * y[I]; });
            big = fmaxf(big, fabsf(dq[J]));
        });
        const float scale = big > A.max_step ? A.max_step * fast_rcp(big) : 1.f;
        static_for<kDof>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            const float qn = fminf(fmaxf(q[J] + scale * dq[J], limit_lo(J)), limit_hi(J));
            q[J] = frozen ? q[J] : qn;
        });
        iters += frozen ? 0 : 1;
    }
    if (!live) return;
    float2* qo = reinterpret_cast<float2*>(A.q_out) + 3 * e;
    qo[0] = make_float2(q[0], q[1]); qo[1] = make_float2(q[2], q[3]); qo[2] = make_float2(q[4], q[5]);
    if (A.residual) A.residual[e] = dist;
    if (A.angle) A.angle[e] = angle;
    if (A.iterations) A.iterations[e] = iters;
}

// ---- multi-start inverse kinematics (pnr_solve_ik_multi) ---------------------------------------------------------------------
// One START per lane: lane = g S + s is start s of the wave's env g, S = 1 << log2s a wave-uniform runtime argument (one kernel
// per system size, none per S: a start's arithmetic is the same code whatever S is, so start k of an S-start call ends bit for bit
// where a one-start call from the same joints ends).  A workgroup is one wave of 64 / S envs; thread t of the grid is start
// t & (S - 1) of env t >> log2s, which is also its place in the per-start outputs.  The per-iteration steps below are the two
// solves of ik_kernel / ik_pose_kernel restated as functions (those two kernels keep their own text: calling the functions from
// them changed their device code), with the one damping lambda^2 = damping^2 + error_damping (|e_p|^2 +
// w^2 angle^2).  Lanes freeze by selects; policy FIRST freezes a whole env from the ballot of the lanes still running, masked to the
// lane's group.  After the loop the env's winner is the smallest (not converged, cost, start) of a butterfly of log2s
// __shfl_xor exchanges (ds_bpermute: no LDS is allocated), which leaves every lane of the group with the same winner; the
// winner's lane stores the env's record.
struct IkMultiArgs {
    const float* target;       // [n][3], or null: the env's own target (state words 18-20)
    const float4* state;       // the handle's state planes (read only when target is null)
    const float* quat;         // [n][4] x, y, z, w (the pose kernel only)
    const float* starts;       // [S][6], per_env: [n][S][6]; null (S = 1 only): start 0 is q_init or the rest pose
    const float* q_init;       // [n][6] or null: replaces start 0
    const float* q_ref;        // [n][6] or null: the env's clamped start 0
    float* q_out;              // [n][6], 8-byte aligned: the winner's
    float* residual;           // [n] or null
    float* angle;              // [n] or null
    int* iterations;           // [n] or null
    int* start_out;            // [n] or null: the winner's start
    int* converged;            // [n] or null: converged starts of the env
    float* all_q;              // [n][S][6], 8-byte aligned, or null
    float* all_residual;       // [n][S] or null
    float* all_angle;          // [n][S] or null
    int* all_iterations;       // [n][S] or null
    long long n;
    ChainPoint point;
    int log2s, per_env, first; // first: policy FIRST
    int max_iter, axis_mode;
    V3 axis;
    float damping2, error_damping, weight, max_step, tol, angle_tol;
};

// start s of env e, clamped into the limits (s = 0: q_init where given; no table: the rest pose)
__device__ __forceinline__ void ik_multi_start(const IkMultiArgs& A, const long long e, const int s, float (&q)[kDof])
{
    const float* row = nullptr;
    if (s == 0 && A.q_init) row = A.q_init + kDof * e;
    else if (A.starts) row = A.starts + kDof * ((A.per_env ? (e << A.log2s) : 0ll) + s);
#pragma unroll
    for (int i = 0; i < kDof; ++i) q[i] = row ? row[i] : 0.f;
    static_for<kDof>([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        q[J] = fminf(fmaxf(q[J], limit_lo(J)), limit_hi(J));
    });
}

// dq = J^T (J J^T + lambda^2 I)^-1 err for the three linear rows (ik_kernel's solve); big = max_j |dq_j|
__device__ __forceinline__ void ik_position_step(const V3 (&lin)[kDof], const V3& err, const float lambda2, float (&dq)[kDof], float& big)
{
    float a00 = lambda2, a01 = 0.f, a02 = 0.f, a11 = lambda2, a12 = 0.f, a22 = lambda2;
    static_for<kDof>([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        const V3 g = lin[J];
        a00 += g.x * g.x; a01 += g.x * g.y; a02 += g.x * g.z;
        a11 += g.y * g.y; a12 += g.y * g.z; a22 += g.z * g.z;
    });
    const float i0 = fast_rcp(a00);
    const float l10 = a01 * i0, l20 = a02 * i0;
    const float d1 = a11 - l10 * a01, u12 = a12 - l20 * a01;
    const float i1 = fast_rcp(d1);
    const float l21 = u12 * i1;
    const float d2 = a22 - l20 * a02 - l21 * u12;
    const float i2 = fast_rcp(d2);
    const float z0 = err.x, z1 = err.y - l10 * z0, z2 = err.z - l20 * z0 - l21 * z1;
    const float y2 = z2 * i2, y1 = z1 * i1 - l21 * y2, y0 = z0 * i0 - l10 * y1 - l20 * y2;
    const V3 y = {y0, y1, y2};
    big = 0.f;
    static_for<kDof>([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        dq[J] = dot(lin[J], y);
        big = fmaxf(big, fabsf(dq[J]));
    });
}

// the same for the 6 x 6 system e = [err ; w e_o], J = [lin ; w ang] (ik_pose_kernel's solve: L D L^T, pivots held at >= lambda^2);
// sv, sn, angle: the sine vector of the rotation still to make, its length and the angle
__device__ __forceinline__ void ik_pose_step(const V3 (&lin)[kDof], const V3 (&ang)[kDof], const V3& err, const float dist2, const V3& sv,
                                             const float sn, const float angle, const float weight, const float damping2,
                                             const float error_damping, float (&dq)[kDof], float& big)
{
    constexpr int kPose = 6, kTriN = kPose * (kPose + 1) / 2;
    const float wa = weight * angle;
    const float ko = wa * fast_rcp(fmaxf(sn, kIkSineFloor));
    const float er[kPose] = {err.x, err.y, err.z, ko * sv.x, ko * sv.y, ko * sv.z};
    const float lambda2 = damping2 + error_damping * (dist2 + wa * wa);
    float g[kDof][kPose];
    static_for<kDof>([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        g[J][0] = lin[J].x; g[J][1] = lin[J].y; g[J][2] = lin[J].z;
        g[J][3] = weight * ang[J].x; g[J][4] = weight * ang[J].y; g[J][5] = weight * ang[J].z;
    });
    float a[kTriN];
    static_for<kPose>([&](auto ic) {
        constexpr int I = decltype(ic)::value;
        static_for<I + 1>([&](auto kc) {
            constexpr int K = decltype(kc)::value;
            float sum = I == K ? lambda2 : 0.f;
            static_for<kDof>([&](auto jc) { constexpr int J = decltype(jc)::value; sum += g[J][I] * g[J][K]; });
            a[kLow<I, K>] = sum;
        });
    });
    float u[kTriN], l[kTriN], inv[kPose];                                // u_ik = l_ik d_k
    static_for<kPose>([&](auto kc) {
        constexpr int K = decltype(kc)::value;
        float d = a[kLow<K, K>];
        static_for<K>([&](auto mc_) { constexpr int M = decltype(mc_)::value; d -= l[kLow<K, M>] * u[kLow<K, M>]; });
        inv[K] = fast_rcp(fmaxf(d, lambda2));
        static_for<kPose>([&](auto ic) {
            constexpr int I = decltype(ic)::value;
            if constexpr (I > K) {
                float t = a[kLow<I, K>];
                static_for<K>([&](auto mc_) { constexpr int M = decltype(mc_)::value; t -= l[kLow<I, M>] * u[kLow<K, M>]; });
                u[kLow<I, K>] = t;
                l[kLow<I, K>] = t * inv[K];
            }
        });
    });
    float z[kPose], y[kPose];
    static_for<kPose>([&](auto ic) {
        constexpr int I = decltype(ic)::value;
        z[I] = er[I];
        static_for<I>([&](auto mc_) { constexpr int M = decltype(mc_)::value; z[I] -= l[kLow<I, M>] * z[M]; });
    });
    static_for<kPose>([&](auto ic) {
        constexpr int I = kPose - 1 - decltype(ic)::value;
        y[I] = z[I] * inv[I];
        static_for<kPose>([&](auto mc_) {
            constexpr int M = decltype(mc_)::value;
            if constexpr (M > I) y[I] -= l[kLow<M, I>] * y[M];
        });
    });
    big = 0.f;
    static_for<kDof>([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        dq[J] = 0.f;
        static_for<kPose>([&](auto ic) { constexpr int I = decltype(ic)::value; dq[J] += g[J][I] * y[I]; });
        big = fmaxf(big, fabsf(dq[J]));
    });
}

// POSE: the 6 x 6 system (FULL, or AXIS by the wave-uniform axis_mode), else the 3 x 3 one
template <bool POSE>
__global__ __launch_bounds__(kWave) void ik_multi_kernel(const IkMultiArgs A)
{
    const int lane = threadIdx.x;
    const int S = 1 << A.log2s;
    const int s = lane & (S - 1);
    const long long t = (long long)blockIdx.x * kWave + lane;                  // = e S + s
    const long long e = t >> A.log2s;
    const bool live = e < A.n;                                                 // (a group is live or not as a whole)
    const unsigned long long group = (~0ull >> (kWave - S)) << (lane - s);     // the env's lanes in a ballot (S = 64: no shift by 64)
    float q[kDof];
    V3 tgt = {0.f, 0.f, 0.f};
    float qx = 0.f, qy = 0.f, qz = 0.f, qw = 1.f;
#pragma unroll
    for (int i = 0; i < kDof; ++i) q[i] = 0.f;
    if (live) {
        if (A.target) { const float* tp = A.target + 3 * e; tgt = {tp[0], tp[1], tp[2]}; }
        else { const float4 w = state_cold(A.state, A.n)[e]; tgt = {w.x, w.y, w.z}; }
        if constexpr (POSE) {
            const float* tq = A.quat + 4 * e;
            qx = tq[0]; qy = tq[1]; qz = tq[2]; qw = tq[3];
        }
        ik_multi_start(A, e, s, q);
    }
    // the target's rotation as ik_pose_kernel forms it
    const float qinv = 1.0f / sqrtf(qx * qx + qy * qy + qz * qz + qw * qw);
    qx *= qinv; qy *= qinv; qz *= qinv; qw *= qinv;
    const V3 t0 = {1.f - 2.f * (qy * qy + qz * qz), 2.f * (qx * qy + qz * qw), 2.f * (qx * qz - qy * qw)};
    const V3 t1 = {2.f * (qx * qy - qz * qw), 1.f - 2.f * (qx * qx + qz * qz), 2.f * (qy * qz + qx * qw)};
    const V3 t2 = {2.f * (qx * qz + qy * qw), 2.f * (qy * qz - qx * qw), 1.f - 2.f * (qx * qx + qy * qy)};
    const V3 tv = A.axis.x * t0 + A.axis.y * t1 + A.axis.z * t2;
    bool frozen = !live, conv = false;
    int iters = 0;
    float dist = 0.f, angle = 0.f;
    for (int it = 0; ; ++it) {
        float c[kDof], sj[kDof];
#pragma unroll
        for (int i = 0; i < kDof; ++i) sincos_bounded(q[i], sj[i], c[i]);    // q is inside the limits
        V3 lin[kDof], ang[kDof], point;
        M3 R;
        chain_jacobian(c, sj, A.point, lin, ang, point, POSE ? &R : nullptr);
        const V3 err = tgt - point;
        const float dist2 = dot(err, err);
        dist = sqrtf(dist2);
        V3 sv = {0.f, 0.f, 0.f};
        float sn = 0.f;
        if constexpr (POSE) {
            float cs;
            if (A.axis_mode) {
                const V3 u = mul(R, A.axis);
                sv = cross(u, tv); cs = dot(u, tv);
            } else {
                const V3 r0 = col(R, 0), r1 = col(R, 1), r2 = col(R, 2);
                sv = 0.5f * (cross(r0, t0) + cross(r1, t1) + cross(r2, t2));
                cs = 0.5f * (dot(r0, t0) + dot(r1, t1) + dot(r2, t2) - 1.f);
            }
            sn = sqrtf(dot(sv, sv));
            angle = atan2f(sn, cs);
        }
        conv = POSE ? (dist <= A.tol && angle <= A.angle_tol) : dist <= A.tol;   // of the pose q is at: a frozen lane's stays
        if (it == A.max_iter) break;                                         // the pose of the result: its residuals
        frozen = frozen || conv;
        unsigned long long running = __builtin_amdgcn_ballot_w64(!frozen);
        if (A.first) {                                                       // a lane of the env has converged: the env stops
            frozen = frozen || (~running & group) != 0;
            running = __builtin_amdgcn_ballot_w64(!frozen);
        }
        if (running == 0) break;
        float dq[kDof], big;
        if constexpr (POSE) ik_pose_step(lin, ang, err, dist2, sv, sn, angle, A.weight, A.damping2, A.error_damping, dq, big);
        else ik_position_step(lin, err, A.damping2 + A.error_damping * dist2, dq, big);
        const float scale = big > A.max_step ? A.max_step * fast_rcp(big) : 1.f;
        static_for<kDof>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            const float qn = fminf(fmaxf(q[J] + scale * dq[J], limit_lo(J)), limit_hi(J));
            q[J] = frozen ? q[J] : qn;
        });
        iters += frozen ? 0 : 1;
    }
    // the env's winner: the smallest (not converged, cost, start); a cost that is not finite is +inf (costs are >= 0, so their
    // bit patterns order as they do, and the top bit is free for "not converged")
    const unsigned long long conv_mask = __builtin_amdgcn_ballot_w64(conv && live);
    float cost = dist + A.weight * angle;
    if (conv) {
        float ref[kDof];
        if (live && A.q_ref) {
#pragma unroll
            for (int i = 0; i < kDof; ++i) ref[i] = A.q_ref[kDof * e + i];
        } else {
            ik_multi_start(A, live ? e : 0ll, 0, ref);
        }
        cost = 0.f;
#pragma unroll
        for (int i = 0; i < kDof; ++i) cost += (q[i] - ref[i]) * (q[i] - ref[i]);
    }
    cost = cost < __builtin_inff() ? cost : __builtin_inff();
    unsigned key = __float_as_uint(cost) | (conv ? 0u : 0x80000000u);
    int win = s;
    for (int m = 1; m < S; m <<= 1) {
        const unsigned okey = (unsigned)__shfl_xor((int)key, m);
        const int owin = __shfl_xor(win, m);
        const bool take = okey < key || (okey == key && owin < win);
        key = take ? okey : key;
        win = take ? owin : win;
    }
    if (!live) return;
    if (A.all_q) {
        float2* qa = reinterpret_cast<float2*>(A.all_q) + 3 * t;
        qa[0] = make_float2(q[0], q[1]); qa[1] = make_float2(q[2], q[3]); qa[2] = make_float2(q[4], q[5]);
    }
    if (A.all_residual) A.all_residual[t] = dist;
    if (A.all_angle) A.all_angle[t] = angle;
    if (A.all_iterations) A.all_iterations[t] = iters;
    if (s != win) return;
    float2* qo = reinterpret_cast<float2*>(A.q_out) + 3 * e;
    qo[0] = make_float2(q[0], q[1]); qo[1] = make_float2(q[2], q[3]); qo[2] = make_float2(q[4], q[5]);
    if (A.residual) A.residual[e] = dist;
    if (A.angle) A.angle[e] = angle;
    if (A.iterations) A.iterations[e] = iters;
    if (A.start_out) A.start_out[e] = s;
    if (A.converged) A.converged[e] = __builtin_popcountll(conv_mask & group);
}

// ---- Cartesian path inverse kinematics (pnr_solve_ik_path) -------------------------------------------------------------------
// ik_multi_kernel's layout (lane = g S + s, a workgroup is one wave of 64 / S envs) around a loop over the C configurations of a
// pointer path: configuration c is one solve of the task's law from the joints configuration c - 1 ended at, towards the target
// interpolated between two waypoints (ik_path_target, contraction off: its roundings are the stated ones), under the cap
// max_iter (configuration 0) or track_iter.  A start that does not reach a configuration stops there by selects: its joints and
// its recorded residuals stay, so the rows after it are copies; once a ballot finds every lane of the wave stopped the remaining
// configurations only store.  After the loop the env's winner is the smallest (not tracked, cost, start) of the same butterfly.
// The winner's rows under S > 1 come from tracking its start again with the same code: `passes` 2 runs the configuration loop a
// second time in the launch with only the winners' lanes live; `replay` is a second launch at one lane per env that takes the
// start index from the summary the first launch wrote (DESIGN.md 3z has the measurement that chose).  No LDS, no scratch.
constexpr int kIkPathSummary = 8;                                // floats per env of the summary

struct IkPathArgs {
    const float* wp_pos;       // [K][3], wp_per_env: [n][K][3]
    const float* wp_quat;      // [K][4], wp_per_env: [n][K][4]: x, y, z, w (the pose kernel only)
    const float* starts;       // [S][6], starts_per_env: [n][S][6]; null (S = 1 only)
    const float* q_init;       // [n][6] or null: replaces start 0
    const float* q_ref;        // [n][6] or null: travel starts with |q_0 - q_ref|
    float* summary;            // [n][8], 16-byte aligned (replay: read, column 6 is the start to track)
    float* q_path;             // [n][C][6], 8-byte aligned, or null
    float* residual;           // [n][C] or null
    float* angle;              // [n][C] or null
    int* iterations;           // [n][C] or null
    float* all_summary;        // [n][S][4], 16-byte aligned, or null
    long long n;
    ChainPoint point;
    int log2s;                 // lanes per env of this launch (replay: 0)
    int log2t;                 // starts per env of the table
    int starts_per_env, wp_per_env;
    int passes, store, replay; // store: the last pass writes the rows; replay: no selection, no summary
    int K, M, C;
    int max_iter, track_iter, axis_mode;
    V3 axis;
    float damping2, error_damping, weight, max_step, tol, angle_tol;
};

// start s of env e as ik_multi_start gives it (the table's stride is its own S, whatever the launch's lanes per env)
__device__ __forceinline__ void ik_path_start(const IkPathArgs& A, const long long e, const int s, float (&q)[kDof])
{
    const float* row = nullptr;
    if (s == 0 && A.q_init) row = A.q_init + kDof * e;
    else if (A.starts) row = A.starts + kDof * ((A.starts_per_env ? (e << A.log2t) : 0ll) + s);
#pragma unroll
    for (int i = 0; i < kDof; ++i) q[i] = row ? row[i] : 0.f;
    static_for<kDof>([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        q[J] = fminf(fmaxf(q[J], limit_lo(J)), limit_hi(J));
    });
}

// The target of the configuration j of segment i (j = 0: waypoint i itself, only configuration 0; j = M: waypoint i + 1 itself):
// a + u (b - a), u = (float)j / (float)M, each operation rounded once; the quaternion (1 - u) q_a + u h q_b, h = -1 where
// q_a . q_b < 0, NOT normalised here (the kernel normalises every target quaternion).
template <bool POSE>
__device__ __forceinline__ void ik_path_target(const IkPathArgs& A, const long long wp0, const int i, const int j, V3& tgt, float (&tq)[4])
{
#pragma clang fp contract(off)
    const int ib = i + 1 < A.K ? i + 1 : A.K - 1;
    const float* pa = A.wp_pos + 3 * (wp0 + i);
    const float* pb = A.wp_pos + 3 * (wp0 + ib);
    const float u = (float)j / (float)A.M;
    const V3 a = {pa[0], pa[1], pa[2]}, b = {pb[0], pb[1], pb[2]};
    const V3 mid = {a.x + u * (b.x - a.x), a.y + u * (b.y - a.y), a.z + u * (b.z - a.z)};
    tgt = j == 0 ? a : (j == A.M ? b : mid);
    if constexpr (POSE) {
        const float* qa = A.wp_quat + 4 * (wp0 + i);
        const float* qb = A.wp_quat + 4 * (wp0 + ib);
        float d = qa[0] * qb[0];
        d = d + qa[1] * qb[1]; d = d + qa[2] * qb[2]; d = d + qa[3] * qb[3];
        const float v = 1.f - u, w = d < 0.f ? -u : u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float m = v * qa[k] + w * qb[k];
            tq[k] = j == 0 ? qa[k] : (j == A.M ? qb[k] : m);
        }
    }
}

// POSE: the 6 x 6 system (FULL, or AXIS by the wave-uniform axis_mode), else the 3 x 3 one
template <bool POSE>
__global__ __launch_bounds__(kWave) void ik_path_kernel(const IkPathArgs A)
{
    const int lane = threadIdx.x;
    const int S = 1 << A.log2s;
    const int sl = lane & (S - 1);
    const long long t = (long long)blockIdx.x * kWave + lane;                  // = e S + s
    const long long e = t >> A.log2s;
    const bool live = e < A.n;                                                 // (a group is live or not as a whole)
    const long long er = live ? e : 0ll;                                       // (a lane past the batch reads env 0's inputs and stores nothing)
    const unsigned long long group = (~0ull >> (kWave - S)) << (lane - sl);
    int s = sl;
    if (A.replay) s = min(max((int)A.summary[kIkPathSummary * er + 6], 0), (1 << A.log2t) - 1);
    const long long wp0 = A.wp_per_env ? er * A.K : 0ll;
    const long long row0 = er * A.C;
    int win = s;
    for (int pass = 0; pass < A.passes; ++pass) {
        const bool store = A.store && pass == A.passes - 1;                    // wave-uniform
        const bool mine = live && s == win;                                    // (pass 0: every live lane)
        bool stopped = !mine;
        float q[kDof];
        ik_path_start(A, er, s, q);
        int cfail = -1, seg = 0, j = 0;
        float max_res = 0.f, max_ang = 0.f, travel = 0.f, max_jump = 0.f, rdist = 0.f, rang = 0.f;
        for (int cfg = 0; cfg < A.C; ++cfg) {
            const bool was = stopped;
            int iters = 0;
            if (__builtin_amdgcn_ballot_w64(!stopped) != 0) {
                float prev[kDof];
#pragma unroll
                for (int i = 0; i < kDof; ++i) prev[i] = q[i];
                V3 tgt;
                float tq[4] = {0.f, 0.f, 0.f, 1.f};
                ik_path_target<POSE>(A, wp0, seg, j, tgt, tq);
                // the target's rotation as ik_multi_kernel forms it
                float qx = tq[0], qy = tq[1], qz = tq[2], qw = tq[3];
                const float qinv = 1.0f / sqrtf(qx * qx + qy * qy + qz * qz + qw * qw);
                qx *= qinv; qy *= qinv; qz *= qinv; qw *= qinv;
                const V3 t0 = {1.f - 2.f * (qy * qy + qz * qz), 2.f * (qx * qy + qz * qw), 2.f * (qx * qz - qy * qw)};
                const V3 t1 = {2.f * (qx * qy - qz * qw), 1.f - 2.f * (qx * qx + qz * qz), 2.f * (qy * qz + qx * qw)};
                const V3 t2 = {2.f * (qx * qz + qy * qw), 2.f * (qy * qz - qx * qw), 1.f - 2.f * (qx * qx + qy * qy)};
                const V3 tv = A.axis.x * t0 + A.axis.y * t1 + A.axis.z * t2;
                const int cap = cfg == 0 ? A.max_iter : A.track_iter;
                bool frozen = stopped, conv = false;
                float dist = 0.f, angle = 0.f;
                for (int it = 0; ; ++it) {
                    float c[kDof], sj[kDof];
#pragma unroll
                    for (int i = 0; i < kDof; ++i) sincos_bounded(q[i], sj[i], c[i]);    // q is inside the limits
                    V3 lin[kDof], ang[kDof], point;
                    M3 R;
                    chain_jacobian(c, sj, A.point, lin, ang, point, POSE ? &R : nullptr);
                    const V3 err = tgt - point;
                    const float dist2 = dot(err, err);
                    dist = sqrtf(dist2);
                    V3 sv = {0.f, 0.f, 0.f};
                    float sn = 0.f;
                    if constexpr (POSE) {
                        float cs;
                        if (A.axis_mode) {
                            const V3 u = mul(R, A.axis);
                            sv = cross(u, tv); cs = dot(u, tv);
                        } else {
                            const V3 r0 = col(R, 0), r1 = col(R, 1), r2 = col(R, 2);
                            sv = 0.5f * (cross(r0, t0) + cross(r1, t1) + cross(r2, t2));
                            cs = 0.5f * (dot(r0, t0) + dot(r1, t1) + dot(r2, t2) - 1.f);
                        }
                        sn = sqrtf(dot(sv, sv));
                        angle = atan2f(sn, cs);
                    }
                    conv = POSE ? (dist <= A.tol && angle <= A.angle_tol) : dist <= A.tol;
                    if (it == cap) break;                                        // the pose of the row: its residuals
                    frozen = frozen || conv;
                    if (__builtin_amdgcn_ballot_w64(!frozen) == 0) break;
                    float dq[kDof], big;
                    if constexpr (POSE) ik_pose_step(lin, ang, err, dist2, sv, sn, angle, A.weight, A.damping2, A.error_damping, dq, big);
                    else ik_position_step(lin, err, A.damping2 + A.error_damping * dist2, dq, big);
                    const float scale = big > A.max_step ? A.max_step * fast_rcp(big) : 1.f;
                    static_for<kDof>([&](auto jc) {
                        constexpr int J = decltype(jc)::value;
                        const float qn = fminf(fmaxf(q[J] + scale * dq[J], limit_lo(J)), limit_hi(J));
                        q[J] = frozen ? q[J] : qn;
                    });
                    iters += frozen ? 0 : 1;
                }
                // the bookkeeping of the lanes still tracking; a stopped lane keeps what it recorded at its last configuration
                rdist = was ? rdist : dist;
                rang = was ? rang : angle;
                max_res = was || rdist <= max_res ? max_res : rdist;             // (a residual that is not a number is the largest)
                max_ang = was || rang <= max_ang ? max_ang : rang;
                const float* refp = A.q_ref ? A.q_ref + kDof * er : nullptr;
#pragma unroll
                for (int i = 0; i < kDof; ++i) {
                    const float base = cfg > 0 ? prev[i] : (refp ? refp[i] : q[i]);
                    const float d = fabsf(q[i] - base);
                    travel = was ? travel : travel + d;
                    max_jump = was || cfg == 0 ? max_jump : fmaxf(max_jump, d);
                }
                cfail = !was && !conv ? cfg : cfail;
                stopped = was || !conv;
            } else if (!store) {
                break;                                                           // every lane of the wave has stopped: nothing left to do
            }
            if (store && mine) {
                const long long r = row0 + cfg;
                if (A.q_path) {
                    float2* qo = reinterpret_cast<float2*>(A.q_path) + 3 * r;
                    qo[0] = make_float2(q[0], q[1]); qo[1] = make_float2(q[2], q[3]); qo[2] = make_float2(q[4], q[5]);
                }
                if (A.residual) A.residual[r] = rdist;
                if (A.angle) A.angle[r] = rang;
                if (A.iterations) A.iterations[r] = iters;
            }
            if (++j > A.M) { j = 1; ++seg; }
        }
        if (pass > 0 || A.replay) continue;
        // the env's winner: the smallest (not tracked, cost, start); a cost that is not finite is +inf (costs are >= 0, so their
        // bit patterns order as they do, and the top bit is free for "not tracked")
        const bool tracked = live && cfail < 0;
        const unsigned long long tracked_mask = __builtin_amdgcn_ballot_w64(tracked);
        float cost = tracked ? travel : (float)(A.C - cfail);
        cost = cost < __builtin_inff() ? cost : __builtin_inff();
        unsigned key = __float_as_uint(cost) | (tracked ? 0u : 0x80000000u);
        for (int m = 1; m < S; m <<= 1) {
            const unsigned okey = (unsigned)__shfl_xor((int)key, m);
            const int owin = __shfl_xor(win, m);
            const bool take = okey < key || (okey == key && owin < win);
            key = take ? okey : key;
            win = take ? owin : win;
        }
        if (!live) continue;
        if (A.all_summary)
            reinterpret_cast<float4*>(A.all_summary)[t] = make_float4(tracked ? 1.f : 0.f, (float)cfail, travel, max_jump);
        if (s != win) continue;
        float4* sm = reinterpret_cast<float4*>(A.summary) + 2 * e;
        sm[0] = make_float4(tracked ? 1.f : 0.f, (float)cfail, max_res, max_ang);
        sm[1] = make_float4(travel, max_jump, (float)s, (float)__builtin_popcountll(tracked_mask & group));
    }
}

}  // namespace pnr

#pragma clang fp contract(off)
