// pnr_contacts.h — pnr_get_contacts: for every env, the signed distance of each of the arm's 23 contact sample spheres
// (pnr_model.h kCapsules, in table order; sample 22 is the pointer) to the nearest of up to eight static bodies, the contact
// normal, point and penalty force there, a per-env summary and the joint torques of all contact forces: the batched form of
// getContactPoints / getClosestPoints.  Included by pnr_queries.hip only, whose code object holds no step kernel.
//
// Per env: q[6], qd[6] in (48-96 B), 23 records of 9 floats out (828 B) + one float4 + six floats.  The signed-distance forms
// (plane, sphere, oriented box with the nearest-face rule inside), the penalty law max(0, kp depth - kd v.n) and the walk over
// the samples are the step's own: body_distance, penalty and for_body_samples of pnr_dyn.h, the one statement of each.  Every sample
// touches with its SURFACE; the step's one quirk (link_contacts = 0: the pointer meets ground_z with its centre) is not part
// of the query.
//
// Shape: the tile kernel of pnr_query.h.  The pose and velocity sweep over the six moving bodies runs in registers, the 23
// samples are unrolled from the compile-time table, the body loop is a wave-uniform runtime loop over the by-value kernel
// argument (scalar loads).  Each output is a wave-uniform branch on its pointer.  The records go to a dense LDS tile of
// [64][207] floats (52 992 B); summary and joint_torques are 16 + 24 B per lane and go out as plain per-lane stores.  No
// cross-lane arithmetic: an env's results do not depend on the batch around it.
//
// The scene form (contacts_kernel<SRC | kQueryScene>, pnr_query.h; a handle whose moving sphere the query reports): the lane loads
// its env's eight sphere words once, and every sample meets the sphere after the body loop, as body kMaxScene.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "pnr_device.h"
#include "pnr_dyn.h"
#include "pnr_query.h"

// float32 against a float64 reference, tolerance-checked: let a*b+c fuse
#pragma clang fp contract(fast)

namespace pnr {

constexpr int kContactDim = 9;
constexpr int kContactRowFloats = kContactSamples * kContactDim;     // 207 floats = 828 B per env
constexpr int kContactTileFloats = kWave * kContactRowFloats;         // 13 248 floats = 52 992 B per wave
static_assert(kNumCapsules == 5 && kContactSamples == 23, "the sample table is pnr_model.h kCapsules");
static_assert(kContactRowFloats % 2 == 1, "an odd row stride keeps the per-lane LDS writes conflict-free");
static_assert(kContactTileFloats * sizeof(float) <= 65536, "the tile is static LDS");

struct ContactArgs {
    const float* src;           // joint source (pnr_query.h load_joints)
    const float4* state;        // kinematic-mode state planes (kJointSrcKin) or null
    const float* body_pos;      // [n][n_bodies][3] per-env body positions or null
    float* points;              // [n][23][9] or null
    float* summary;             // [n][4] or null
    float* torques;             // [n][6] or null
    long long n;
    float ckp, ckd, ptr_radius;
    int n_bodies;
    SceneBody bodies[kMaxScene];   // as the step uploads them: world position, row-major rotation (plane: unit normal in rot[0..2]), size
};

// The bodies are read where the launch put them, in the kernel-argument segment (constant address space), 16 scalar dwords per
// body at a wave-uniform index: indexing the by-value argument itself with the loop counter makes the compiler copy the whole
// struct to scratch first.  ContactArgs is the kernel's only argument, so the segment starts with it.
typedef const __attribute__((address_space(4))) int* ContactBodyWords;
static_assert(sizeof(SceneBody) == 16 * sizeof(int) && offsetof(ContactArgs, bodies) % 4 == 0, "a SceneBody is 16 dwords");

__device__ __forceinline__ ContactBodyWords contact_body_words()
{
    typedef const __attribute__((address_space(4))) char* Bytes;
    return (ContactBodyWords)((Bytes)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(ContactArgs, bodies));
}

__device__ __forceinline__ SceneBody load_contact_body(ContactBodyWords w, int b)
{
    w += 16 * b;
    SceneBody S;
    S.shape = w[0];
#pragma unroll
    for (int k = 0; k < 3; ++k) { S.pos[k] = __int_as_float(w[1 + k]); S.size[k] = __int_as_float(w[13 + k]); }
#pragma unroll
    for (int k = 0; k < 9; ++k) S.rot[k] = __int_as_float(w[4 + k]);
    return S;
}

// world pose and velocity of one moving body's frame
struct ContactFrame { M3 R; V3 p, v, w; };

// body J from its parent B: pose_outward at the full angle's cos / sin, velocity_outward; axis = the joint's world axis
template <int J>
__device__ __forceinline__ void contact_frame_outward(const ContactFrame& B, float q, float qd, ContactFrame& C, V3& axis)
{
    float sn, cs;
    sincos_any(q, sn, cs);
    pose_outward<J>(B.R, B.p, cs, sn, C.R, C.p);
    velocity_outward<J>(B, qd, C, axis);
}

// per-env running summary: smallest distance, its sample and body, number of penetrating samples
struct ContactSummary { float dist, sample, body, count; };

// The scene form's argument: ContactArgs first (contact_body_words), then the handle's moving-sphere words
struct ContactSceneArgs : ContactArgs { const float* sphere; };   // [PNR_BODY_STATE_WORDS][n] (pnr_dyn.h WorldBody::words)

// One sample sphere (centre c in the frame B, radius) against every body: its record into rec (9 floats of this lane's LDS
// row, or null), the summary, and F = the sum over ALL bodies of the penalty force on it; pos = its centre in the world.
// SPHERE: after the caller's bodies the env's moving sphere sp (mass <= 0: none), as body kMaxScene: the step's arm-sphere pair
// (pnr_dyn.h sample_contact) seen from the sample, with the relative velocity in the law; it loses a tie to a caller's body.
template <bool SPHERE>
__device__ __forceinline__ void contact_sample(const ContactArgs& A, ContactBodyWords bw, const float* __restrict__ bp, const ContactFrame& B, V3 c,
                                               float radius, int s, float* rec, ContactSummary& sm, V3& pos, V3& F, const SphereLane& sp)
{
    const V3 rel = mul(B.R, c);
    pos = B.p + rel;
    const V3 vel = B.v + cross(B.w, rel);
    float best = INFINITY, bestf = 0.f, bestb = -1.f;
    V3 bestn = {0.f, 0.f, 0.f};
    F = {0.f, 0.f, 0.f};
    // software-pipelined: body b + 1 is on its way (scalar loads) while body b is worked on; with one wave per SIMD nothing else
    // hides that latency.  The index stays inside bodies[kMaxScene] whatever n_bodies is.
    SceneBody next = load_contact_body(bw, 0);
#pragma unroll 1
    for (int b = 0; b < A.n_bodies; ++b) {             // wave-uniform
        const SceneBody S = next;
        next = load_contact_body(bw, b + 1 < kMaxScene ? b + 1 : b);
        V3 o = {S.pos[0], S.pos[1], S.pos[2]};
        if (bp) o = {bp[3 * b], bp[3 * b + 1], bp[3 * b + 2]};
        float sdf;
        V3 nrm;
        body_distance(S, o, pos, sdf, nrm);
        const float depth = radius - sdf;              // surface to surface
        float fn;
        const float f = penalty(A.ckp, A.ckd, depth, dot(vel, nrm), fn) ? fn : 0.f;
        F = F + f * nrm;
        if (-depth < best) { best = -depth; bestn = nrm; bestb = (float)b; bestf = f; }
    }
    if constexpr (SPHERE) {
        // body_distance's sphere, asked from the sample's side: the unit vector towards the sphere's centre, (0, 0, 1) at zero
        // distance, is the step's n; the normal on the sphere towards the sample is its mirror
        SceneBody S = SceneBody{};
        S.shape = 3;
        S.size[0] = sp.r;
        float sdf;
        V3 towards;
        body_distance(S, pos, sp.x, sdf, towards);
        const V3 nrm = -1.f * towards;
        const float depth = radius - sdf;                  // surface to surface: radius + r - |x - pos|
        const bool there = sp.m > 0.f;
        float fn;
        const float f = (penalty(A.ckp, A.ckd, depth, dot(vel - sp.v, nrm), fn) && there) ? fn : 0.f;
        F = F + f * nrm;
        if (there && -depth < best) { best = -depth; bestn = nrm; bestb = (float)kMaxScene; bestf = f; }
    }
    if (rec) {
        const V3 on = pos - radius * bestn;
        rec[0] = best;
        rec[1] = bestn.x; rec[2] = bestn.y; rec[3] = bestn.z;
        rec[4] = on.x; rec[5] = on.y; rec[6] = on.z;
        rec[7] = bestb;
        rec[8] = bestf;
    }
    if (s == 0 || best < sm.dist) { sm.dist = best; sm.sample = (float)s; sm.body = bestb; }
    sm.count += best < 0.f ? 1.f : 0.f;
}

// one env: the 23 records into `row` (207 floats, or null), the summary, tau_j = sum_s a_j . ((pos_s - o_j) x F_s)
template <bool SPHERE>
__device__ __forceinline__ void contacts_env(const ContactArgs& A, const float* __restrict__ bp, const float (&q)[kDof],
                                             const float (&qd)[kDof], float* row, ContactSummary& sm, float (&tau)[kDof], const SphereLane& sp)
{
    const bool want_tau = A.torques != nullptr;
    const ContactBodyWords bw = contact_body_words();
    ContactFrame b;
    b.R = diag3(1.f); b.p = {0.f, 0.f, 0.f}; b.v = {0.f, 0.f, 0.f}; b.w = {0.f, 0.f, 0.f};
    V3 axis[kDof], org[kDof];
    sm = {INFINITY, 0.f, -1.f, 0.f};
#pragma unroll
    for (int j = 0; j < kDof; ++j) tau[j] = 0.f;
    static_for<kDof>([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        ContactFrame c;
        contact_frame_outward<J>(b, q[J], qd[J], c, axis[J]);
        b = c;
        org[J] = b.p;
        for_body_samples<J>([&](auto s_, V3 cen, float radius, auto) {
            constexpr int s = decltype(s_)::value;
            V3 pos, F;
            contact_sample<SPHERE>(A, bw, bp, b, cen, radius < 0.f ? A.ptr_radius : radius, s, row ? row + kContactDim * s : nullptr, sm, pos, F, sp);
            if (want_tau) {
                static_for<J + 1>([&](auto k_) {                        // the joints between the base and this body
                    constexpr int k = decltype(k_)::value;
                    tau[k] += dot(axis[k], cross(pos - org[k], F));
                });
            }
        });
    });
}

template <int SRC>
__global__ __launch_bounds__(kWave) void contacts_kernel(const QueryArgs<SRC, ContactArgs, ContactSceneArgs> A)
{
    constexpr bool SCENE = (SRC & kQueryScene) != 0;
    __shared__ __attribute__((aligned(16))) float tile[kContactTileFloats];
    const EnvLane L = env_lane(A.n);
    float q[kDof], qd[kDof];
    load_lane_joints<(SRC & kJointSrcMask)>(A.src, A.state, A.n, L, q, qd);
    // a lane past the batch computes on the last env's body positions and stores nothing
    const float* bp = A.body_pos ? A.body_pos + (L.live ? L.e : A.n - 1) * (3 * A.n_bodies) : nullptr;
    ContactSummary sm;
    float tau[kDof];
    SphereLane sp = {};                                 // (a lane past the batch: mass 0, no sphere)
    if constexpr (SCENE) {
        if (L.live) {                                   // the env's eight words, once per env
            const float* w = A.sphere + L.e;
            sp.x = {w[0], w[A.n], w[2 * A.n]}; sp.v = {w[3 * A.n], w[4 * A.n], w[5 * A.n]};
            sp.m = w[6 * A.n]; sp.r = w[7 * A.n];
        }
    }
    contacts_env<SCENE>(A, bp, q, qd, A.points ? tile + L.lane * kContactRowFloats : nullptr, sm, tau, sp);
    if (L.live) {
        if (A.summary) reinterpret_cast<float4*>(A.summary)[L.e] = make_float4(sm.dist, sm.sample, sm.body, sm.count);
        if (A.torques) {
            float2* t2 = reinterpret_cast<float2*>(A.torques) + 3 * L.e;
            t2[0] = make_float2(tau[0], tau[1]); t2[1] = make_float2(tau[2], tau[3]); t2[2] = make_float2(tau[4], tau[5]);
        }
    }
    if (A.points) {
        wave_lds_sync();
        flush_dense_tile(tile, A.points + L.tile0 * kContactRowFloats, L.nvalid * kContactRowFloats, L.lane);
    }
}

}  // namespace pnr

#pragma clang fp contract(off)
