// pnr_path.h — pnr_path_clearance: for every env, the arm swept along a piecewise-linear joint path of W waypoints at M sub-steps
// per segment, C = 1 + (W - 1) M configurations, each one's clearance (the smallest surface-to-surface distance of the sample
// spheres in the call's mask to the static bodies, the per-env body positions and the env's moving sphere) and the path's summary:
// the batched edge check of a sampling planner.  A SAMPLED check: what is thinner than the samples' travel between two
// configurations can be missed.  Included by pnr_queries.hip only.
//
// Per configuration: two waypoints in (at most 48 B; neighbouring lanes read the same lines), the interpolation, six sincos_any,
// the outward pose sweep (pose_outward), the samples unrolled from the compile-time table (for_body_samples), each behind a
// scalar branch on its mask bit, and pnr_contacts.h's software-pipelined scalar body loads from the kernel-argument segment.
// The distance forms are body_distance (pnr_dyn.h): no velocity, normal or force is kept, so the compiler drops them.
//
// Shape: ik_multi_kernel's.  One configuration per lane per trip; lane = g P + p is lane p of the wave's env g, P = lanes_per_env
// a wave-uniform power of two, a workgroup one wave of 64 / P envs.  A lane walks c = p, p + P, .. in ascending order over the
// wave-uniform ceil(C / P) trips; lanes past C or past the batch carry +inf, the count 0 and "no hit" through selects.  The env's
// result is a butterfly of log2 P __shfl_xor steps (no LDS): the lexicographic minimum of (clearance, c) with its sample and
// body, the integer minimum of the first violating c, the integer sum of the count.  A configuration's arithmetic is the same
// code whatever P, C and the batch are: the outputs are bit-identical for every lanes_per_env and do not depend on the envs
// around one.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "pnr_device.h"
#include "pnr_dyn.h"
#include "pnr_query.h"
#include "pnr_contacts.h"

// float32 against a float64 reference, tolerance-checked: let a*b+c fuse
#pragma clang fp contract(fast)

namespace pnr {

constexpr int kPathSummaryDim = 8;
constexpr unsigned kPathAllSamples = (1u << kContactSamples) - 1u;

struct PathArgs {
    const float* src;           // from_current: the env's own joints (pnr_query.h load_joints, kJointSrcDyn / kJointSrcKin) or null
    const float4* state;        // .. kinematic-mode state planes or null
    const float* waypoints;     // [n][K][6] (per_env) or [K][6], 8-byte aligned; null with K == 0
    const float* body_pos;      // [n][n_bodies][3] per-env body positions or null
    float* summary;             // [n][8] or null
    float* clearance;           // [n][C] or null
    long long n;
    float ptr_radius, margin;
    int n_bodies;
    int K, M, C;                // given waypoints, sub-steps per segment, configurations
    int log2p;                  // P = 1 << log2p lanes per env
    int per_env;
    unsigned mask;              // bit s: sample s takes part
    SceneBody bodies[kMaxScene];   // as ContactArgs::bodies
};
static_assert(offsetof(PathArgs, bodies) % 4 == 0, "the bodies are read as scalar dwords");

// The scene form's argument: PathArgs first (path_body_words), then the handle's moving-sphere words
struct PathSceneArgs : PathArgs { const float* sphere; };   // [PNR_BODY_STATE_WORDS][n]

// PathArgs is the kernel's only argument, so the kernel-argument segment starts with it (pnr_contacts.h contact_body_words)
__device__ __forceinline__ ContactBodyWords path_body_words()
{
    typedef const __attribute__((address_space(4))) char* Bytes;
    return (ContactBodyWords)((Bytes)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(PathArgs, bodies));
}

// a distance that is not finite counts as -inf: the order is total, and a NaN waypoint or body position makes the path not free
__device__ __forceinline__ float path_total_order(float d) { return fabsf(d) < INFINITY ? d : -INFINITY; }

// the smallest distance of one configuration, its sample and its body
struct PathNearest { float dist; int sample, body; };

// One sample sphere (centre c in the frame R, p; radius) against every body and, SPHERE, the env's sphere sp (mass <= 0: none)
// as body kMaxScene: contact_sample's walk without velocities, normals and forces.  The lowest body wins a tie within the
// sample, the lowest sample within the configuration (the caller walks them in table order).
template <bool SPHERE>
__device__ __forceinline__ void path_sample(const PathArgs& A, ContactBodyWords bw, const float* __restrict__ bp, const M3& R, V3 p, V3 c,
                                            float radius, int s, PathNearest& N, const SphereLane& sp)
{
    const V3 pos = p + mul(R, c);
    float best = INFINITY;
    int bestb = -1;
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
        const float d = path_total_order(sdf - radius);    // surface to surface
        if (d < best) { best = d; bestb = b; }
    }
    if constexpr (SPHERE) {
        SceneBody S = SceneBody{};
        S.shape = 3;
        S.size[0] = sp.r;
        float sdf;
        V3 towards;
        body_distance(S, pos, sp.x, sdf, towards);         // as contact_sample asks it: radius + r - |x - pos| deep
        const float d = path_total_order(sdf - radius);
        if (sp.m > 0.f && d < best) { best = d; bestb = kMaxScene; }
    }
    if (best < N.dist) { N.dist = best; N.sample = s; N.body = bestb; }
}

// one configuration q: the outward sweep and the samples of the mask
template <bool SPHERE>
__device__ __forceinline__ PathNearest path_configuration(const PathArgs& A, const float* __restrict__ bp, const float (&q)[kDof], const SphereLane& sp)
{
    const ContactBodyWords bw = path_body_words();
    PathNearest N = {INFINITY, 0, -1};
    M3 R = diag3(1.f);
    V3 p = {0.f, 0.f, 0.f};
    static_for<kDof>([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        float sn, cs;
        sincos_any(q[J], sn, cs);
        M3 Rn;
        V3 pn;
        pose_outward<J>(R, p, cs, sn, Rn, pn);
        R = Rn; p = pn;
        for_body_samples<J>([&](auto s_, V3 cen, float radius, auto) {
            constexpr int s = decltype(s_)::value;
            if (A.mask & (1u << s))                    // scalar
                path_sample<SPHERE>(A, bw, bp, R, p, cen, radius < 0.f ? A.ptr_radius : radius, s, N, sp);
        });
    });
    return N;
}

// the path coordinate of configuration c: 0 for c = 0, else i + j / M on segment i = (c - 1) / M at sub-step j = 1 .. M
__device__ __forceinline__ float path_coordinate(int c, int M)
{
    if (c <= 0) return 0.f;
    const int i = (c - 1) / M, j = c - 1 - i * M + 1;
    return j == M ? (float)(i + 1) : (float)i + (float)j / (float)M;
}

// six joints of waypoint w of the path (w = 0 with from_current: the env's own q0), the given ones at `given`
__device__ __forceinline__ void path_waypoint(const float* __restrict__ given, int w, int fc, const float (&q0)[kDof], float (&q)[kDof])
{
    if (w - fc < 0) {
#pragma unroll
        for (int i = 0; i < kDof; ++i) q[i] = q0[i];
    } else {
        const float2* g = reinterpret_cast<const float2*>(given) + 3 * (w - fc);
        const float2 a = g[0], b = g[1], c = g[2];
        q[0] = a.x; q[1] = a.y; q[2] = b.x; q[3] = b.y; q[4] = c.x; q[5] = c.y;
    }
}

// SRC & kJointSrcMask: where waypoint 0 comes from with from_current (kJointSrcDyn, kJointSrcKin), kJointSrcBuffer: no from_current
template <int SRC>
__global__ __launch_bounds__(kWave) void path_clearance_kernel(const QueryArgs<SRC, PathArgs, PathSceneArgs> A)
{
    constexpr bool SCENE = (SRC & kQueryScene) != 0;
    constexpr int JS = SRC & kJointSrcMask;
    constexpr int FC = JS != kJointSrcBuffer ? 1 : 0;
    const int lane = threadIdx.x;
    const int P = 1 << A.log2p;
    const int p = lane & (P - 1);
    const long long e = (((long long)blockIdx.x * kWave) + lane) >> A.log2p;
    const bool live = e < A.n;                          // (a group is live or not as a whole)
    const long long el = live ? e : A.n - 1;            // a lane past the batch reads the last env's data and stores nothing
    const float* bp = A.body_pos ? A.body_pos + el * (3 * A.n_bodies) : nullptr;
    const float* given = A.waypoints ? A.waypoints + (A.per_env ? el * ((long long)A.K * kDof) : 0ll) : nullptr;
    float q0[kDof];
#pragma unroll
    for (int i = 0; i < kDof; ++i) q0[i] = 0.f;
    if constexpr (FC != 0) {
        float qd0[kDof];
        load_joints<JS>(A.src, A.state, A.n, el, q0, qd0);
    }
    SphereLane sp = {};
    if constexpr (SCENE) {
        const float* w = A.sphere + el;
        sp.x = {w[0], w[A.n], w[2 * A.n]};
        sp.m = w[6 * A.n]; sp.r = w[7 * A.n];
    }
    float best = INFINITY;
    int bestc = 0x7fffffff, bests = 0, bestb = -1, first = 0x7fffffff, count = 0;
    const int trips = (A.C + P - 1) >> A.log2p;         // wave-uniform
#pragma unroll 1
    for (int trip = 0; trip < trips; ++trip) {
        const int c = p + (trip << A.log2p);
        const bool valid = c < A.C;
        float q[kDof];
#pragma unroll
        for (int i = 0; i < kDof; ++i) q[i] = 0.f;
        if (valid) {
            // configuration 0 is waypoint 0; 1 + i M + (j - 1) is a + (j / M)(b - a) on segment i, and EXACTLY b at j = M
            const int i = c > 0 ? (c - 1) / A.M : 0, j = c > 0 ? c - 1 - i * A.M + 1 : A.M;
            float b[kDof];
            path_waypoint(given, c > 0 ? i + 1 : 0, FC, q0, b);
            if (j == A.M) {
#pragma unroll
                for (int k = 0; k < kDof; ++k) q[k] = b[k];
            } else {
                float a[kDof];
                path_waypoint(given, i, FC, q0, a);
                const float t = (float)j / (float)A.M;
#pragma unroll
                for (int k = 0; k < kDof; ++k) q[k] = a[k] + t * (b[k] - a[k]);
            }
        }
        const PathNearest N = path_configuration<SCENE>(A, bp, q, sp);
        if (valid && live) {
            if (A.clearance) A.clearance[e * A.C + c] = N.dist;
            if (N.dist < best || bestc == 0x7fffffff) { best = N.dist; bestc = c; bests = N.sample; bestb = N.body; }
            if (N.dist < A.margin) { first = first < c ? first : c; count += 1; }
        }
    }
    for (int m = 1; m < P; m <<= 1) {
        const float od = __shfl_xor(best, m);
        const int oc = __shfl_xor(bestc, m), os = __shfl_xor(bests, m), ob = __shfl_xor(bestb, m);
        const int of = __shfl_xor(first, m), on = __shfl_xor(count, m);
        const bool take = od < best || (od == best && oc < bestc);      // (a lane without a configuration: +inf at the largest c)
        best = take ? od : best; bestc = take ? oc : bestc; bests = take ? os : bests; bestb = take ? ob : bestb;
        first = of < first ? of : first;
        count += on;
    }
    if (!live || p != 0 || !A.summary) return;
    float4* out = reinterpret_cast<float4*>(A.summary) + 2 * e;
    out[0] = make_float4(best, path_coordinate(bestc, A.M), (float)bests, (float)bestb);
    out[1] = make_float4(first == 0x7fffffff ? -1.f : path_coordinate(first, A.M), (float)count, count == 0 ? 1.f : 0.f, 0.f);
}

}  // namespace pnr

#pragma clang fp contract(off)
