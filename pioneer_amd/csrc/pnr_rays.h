// pnr_rays.h — pnr_ray_test: a few rays per env against that env's solids, the batched form of rayTest / rayTestBatch.  Rays are
// segments from + t (to - from), t in [0, 1], given in the world frame or in the frame of one URDF link of EACH env (a sensor
// mounted on the arm).  Solids, by mask: the caller's static bodies (planes are half-spaces below their surface), the URDF's 14
// visual shapes posed by the env's joints (pnr_render.h kVisuals: a ray and a pixel see the same arm), the target sphere.
// Included by pnr_queries.hip only, whose code object holds no step kernel.
//
// Hit rule: a ray hits a convex solid at its entering parameter tn when tn <= tf (the line meets it) and 0 <= tn <= 1.  A ray
// that starts inside has tn < 0 and does not hit that solid (Bullet's rule for convex shapes); a plane is hit only from above
// (o.z > 0).  The smallest tn wins; on a tie the first in the order arm visuals (table order), target, bodies (by index).  A
// zero-length ray misses.
//
// Shape: one lane per (env, ray) in flat order g = e * n_rays + r; a workgroup covers `span` consecutive pairs (<= 256) and so a
// run of at most kRayMaxEnvs consecutive envs (the host caps span accordingly: with one ray per env a workgroup is 27 pairs, not
// 256 envs' records).  Prologue, once per workgroup and env, into dynamic LDS sized for the envs a span can touch: one lane per
// env sweeps the six body poses (link_body_outward) and the parent link's frame; one lane per (env, primitive) writes a
// world-space record (world -> primitive rotation, centre, half sizes, squared bounding radius, shape, label); one lane per
// (env, body) the body's centre (body_positions, else the body's own).  The sweep and the arm records sit behind a scalar branch:
// a bodies-only call with world rays reads no joints at all.  The static bodies' records are built on the host (kernel argument).
// Per ray: from / to through the parent frame, then a loop over the enabled records with a wave-uniform index and shape (every
// env has the same table); a lane whose segment stays farther from the record's centre than its bounding radius skips the
// intersection; the rest rotate the origin into the primitive frame and run pnr_render.h's intersect_at; the nearest hit is
// selected branch-free, one hit_normal_at from the winner.  No cross-lane arithmetic: an env's results do not depend on the
// batch around it.  hits leaves as two 16-byte non-temporal stores per lane (a lane's row is 32 contiguous bytes, a wave's 2 KB:
// staging through LDS would add a barrier and 8 KB of LDS for the same bytes), fractions as one coalesced dword store.
//
// The scene form (ray_kernel<SRC | kQueryScene>, pnr_query.h; a handle whose moving sphere the rays see): one more record per
// staged env, built from the sphere's words, tested after the caller's bodies.
#pragma once

#include <hip/hip_runtime.h>

#include "pnr_device.h"
#include "pnr_dyn.h"
#include "pnr_links.h"
#include "pnr_query.h"
#include "pnr_render.h"

// float32 against a float64 reference with an ambiguity band: let a*b+c fuse
#pragma clang fp contract(fast)

namespace pnr {

constexpr int kRayDim = 8;
constexpr int kRayThreads = 256;
constexpr int kRayMaxEnvs = 28;                                   // envs staged per workgroup, at most (46 336 B of LDS)
constexpr int kRayHitBodies = 1, kRayHitArm = 2, kRayHitTarget = 4;
constexpr int kRayEnvPrims = kNumVisuals + 1;                     // per-env records: the visuals, then the target

// One primitive in world space, as the per-ray loop reads it (20 words, a multiple of 16 bytes).
struct RayPrim {
    float rt[9];           // world -> primitive frame (rows); the identity for a sphere; a plane: row 2 = its unit normal
    float c[3];            // centre (a plane: a point on it); a body's is replaced by the env's own (centres below)
    float h[3];            // box half extents | cylinder radius, radius, half length | sphere radius
    float bound2;          // squared bounding radius with a margin (a plane: +inf)
    int shape, label;
    int pad[2];
};
static_assert(sizeof(RayPrim) == 80, "a record is 20 words");

// dynamic LDS of a workgroup that stages up to E envs, in floats
constexpr int kRayPrimWords = sizeof(RayPrim) / 4;
constexpr int kRayEnvWords = kRayEnvPrims * kRayPrimWords + 3 * kMaxScene + 12 + 12 * kDof;   // records, centres, frame, poses
__host__ __device__ constexpr int ray_lds_words(int E) { return kMaxScene * kRayPrimWords + E * kRayEnvWords; }
static_assert(ray_lds_words(kRayMaxEnvs) * 4 <= 48 * 1024, "three workgroups fit a CU's 160 KB of LDS");

struct RayArgs {
    const float* src;           // joint source (pnr_query.h load_joints)
    const float4* state;        // the state planes: kinematic joints, and every mode's target
    const float* rays;          // [n_rays][6] or [n][n_rays][6]
    const float* body_pos;      // [n][n_bodies][3] or null
    float* hits;                // [n][n_rays][8] or null
    float* fractions;           // [n][n_rays] or null
    long long n, total;         // envs, n * n_rays
    int n_rays, per_env;
    int parent_body, parent_tip;   // the parent link's moving body (-1: world or the base, no transform) and whether it adds kTip
    int mask, n_bodies;
    int span, max_envs;         // pairs per workgroup, envs a span can touch (the LDS is sized for it)
    float target_radius;
    RayPrim bodies[kMaxScene];
};

// the squared bounding radius the reject compares with: the float32 sums on both sides carry a few ulp
__host__ __device__ inline float ray_bound2(float r) { return r * r * 1.001f + 1e-12f; }

// record of a shape whose world rotation is R (shape frame -> world) and centre c
__device__ __forceinline__ void put_ray_prim(RayPrim& Q, const M3& R, V3 c, int shape, const float* half, float bound, int label)
{
    const V3 c0 = col(R, 0), c1 = col(R, 1), c2 = col(R, 2);          // rows of R^T
    Q.rt[0] = c0.x; Q.rt[1] = c0.y; Q.rt[2] = c0.z;
    Q.rt[3] = c1.x; Q.rt[4] = c1.y; Q.rt[5] = c1.z;
    Q.rt[6] = c2.x; Q.rt[7] = c2.y; Q.rt[8] = c2.z;
    Q.c[0] = c.x; Q.c[1] = c.y; Q.c[2] = c.z;
    Q.h[0] = half[0]; Q.h[1] = half[1]; Q.h[2] = half[2];
    Q.bound2 = ray_bound2(bound);
    Q.shape = shape; Q.label = label;
}

// the running nearest hit of one ray
struct RayBest { float t; int idx; };

// one record against the segment from + t d: idx is taken when it enters nearer than the best so far
__device__ __forceinline__ void ray_against(const RayPrim& Q, V3 c, int shape, int idx, V3 from, V3 d, float inv_dd, RayBest& best)
{
    const V3 w = from - c;
    bool close_by = true;
    if (shape != kVisPlane) {                                        // the segment's closest approach to the centre
        const float tc = fminf(fmaxf(-dot(w, d) * inv_dd, 0.f), 1.f);
        const V3 v = w + tc * d;
        close_by = dot(v, v) <= Q.bound2;
    }
    if (close_by) {
        const V3 o = {Q.rt[0] * w.x + Q.rt[1] * w.y + Q.rt[2] * w.z, Q.rt[3] * w.x + Q.rt[4] * w.y + Q.rt[5] * w.z,
                      Q.rt[6] * w.x + Q.rt[7] * w.y + Q.rt[8] * w.z};
        float tn, tf;
        intersect_at(o, Q.rt, Q.h, shape, d, tn, tf);
        const bool take = tn <= tf && tn >= 0.f && tn <= 1.f && tn < best.t && (shape != kVisPlane || o.z > 0.f);
        best.t = take ? tn : best.t;
        best.idx = take ? idx : best.idx;
    }
}

// The scene form's argument and dynamic LDS: one more record per staged env, behind the poses
struct RaySceneArgs : RayArgs { const float* sphere; };          // [PNR_BODY_STATE_WORDS][n] (pnr_dyn.h WorldBody::words)
__host__ __device__ constexpr int ray_scene_lds_words(int E) { return ray_lds_words(E) + E * kRayPrimWords; }
static_assert(ray_scene_lds_words(kRayMaxEnvs) * 4 <= 48 * 1024, "three workgroups fit a CU's 160 KB of LDS");
constexpr int kRayIdxSphere = kRayEnvPrims + kMaxScene;           // the moving sphere's place in the tie order: after the bodies

template <int SRC>
__global__ __launch_bounds__(kRayThreads) void ray_kernel(const QueryArgs<SRC, RayArgs, RaySceneArgs> A)
{
    constexpr bool SCENE = (SRC & kQueryScene) != 0;
    extern __shared__ __attribute__((aligned(16))) float ray_lds[];
    RayPrim* const bodies = reinterpret_cast<RayPrim*>(ray_lds);                        // [kMaxScene], shared by the envs
    RayPrim* const recs = bodies + kMaxScene;                                           // [max_envs][kRayEnvPrims]
    float* const centres = reinterpret_cast<float*>(recs + A.max_envs * kRayEnvPrims);  // [max_envs][kMaxScene][3]
    float* const frames = centres + A.max_envs * (3 * kMaxScene);                       // [max_envs][12]: R (rows), p
    float* const poses = frames + A.max_envs * 12;                                      // [max_envs][kDof][12]

    const int tid = threadIdx.x, nthreads = blockDim.x;
    const long long g0 = (long long)blockIdx.x * A.span;                                // the workgroup's first pair
    const long long glast = (g0 + A.span < A.total ? g0 + A.span : A.total) - 1;
    const long long e0 = g0 / A.n_rays;
    const int nenv = (int)(glast / A.n_rays - e0) + 1;                                  // <= max_envs
    const bool arm = (A.mask & kRayHitArm) != 0, with_target = (A.mask & kRayHitTarget) != 0;
    const int nb = (A.mask & kRayHitBodies) ? A.n_bodies : 0;

    // ---- prologue: body poses and the parent frame (one lane per env), then the records ----
    if (arm || A.parent_body >= 0) {
        if (tid < nenv) {
            float q[kDof], qd[kDof];
            load_joints<(SRC & kJointSrcMask)>(A.src, A.state, A.n, e0 + tid, q, qd);
            LinkBody b = link_base();
            static_for<kDof>([&](auto jc) {
                constexpr int J = decltype(jc)::value;
                LinkBody c;
                link_body_outward<J>(b, q[J], 0.f, c);
                b = c;
                float* w = poses + (tid * kDof + J) * 12;
                w[0] = b.R.r0.x; w[1] = b.R.r0.y; w[2] = b.R.r0.z; w[3] = b.R.r1.x; w[4] = b.R.r1.y; w[5] = b.R.r1.z;
                w[6] = b.R.r2.x; w[7] = b.R.r2.y; w[8] = b.R.r2.z; w[9] = b.p.x; w[10] = b.p.y; w[11] = b.p.z;
                if (J == A.parent_body) {
                    const V3 p = A.parent_tip ? b.p + mul(b.R, V3{(float)kTipX, (float)kTipY, (float)kTipZ}) : b.p;
                    float* f = frames + tid * 12;
                    f[0] = b.R.r0.x; f[1] = b.R.r0.y; f[2] = b.R.r0.z; f[3] = b.R.r1.x; f[4] = b.R.r1.y; f[5] = b.R.r1.z;
                    f[6] = b.R.r2.x; f[7] = b.R.r2.y; f[8] = b.R.r2.z; f[9] = p.x; f[10] = p.y; f[11] = p.z;
                }
            });
        }
        __syncthreads();
    }
    if (arm) {
        for (int k = tid; k < nenv * kNumVisuals; k += nthreads) {
            const int slot = k / kNumVisuals, i = k - slot * kNumVisuals;
            const VisualDef& D = kVisuals[i];
            const float* w = poses + (slot * kDof + D.body) * 12;
            const M3 Rb = {{w[0], w[1], w[2]}, {w[3], w[4], w[5]}, {w[6], w[7], w[8]}};
            const M3 Rv = {{D.rot[0], D.rot[1], D.rot[2]}, {D.rot[3], D.rot[4], D.rot[5]}, {D.rot[6], D.rot[7], D.rot[8]}};
            // Rb Rv (each row of Rb times Rv); a sphere is intersected in world axes
            const M3 R = D.shape == kVisSphere ? diag3(1.f) : M3{mulT(Rv, Rb.r0), mulT(Rv, Rb.r1), mulT(Rv, Rb.r2)};
            const V3 c = V3{w[9], w[10], w[11]} + mul(Rb, V3{D.t[0], D.t[1], D.t[2]});
            const float bound = D.shape == kVisBox ? sqrtf(D.half[0] * D.half[0] + D.half[1] * D.half[1] + D.half[2] * D.half[2])
                              : (D.shape == kVisSphere ? D.half[0] : sqrtf(D.half[0] * D.half[0] + D.half[2] * D.half[2]));
            put_ray_prim(recs[slot * kRayEnvPrims + i], R, c, D.shape, D.half, bound, kSegLink0 + D.link);
        }
    }
    if (with_target) {
        for (int slot = tid; slot < nenv; slot += nthreads) {         // the target (state words 18-20)
            const float4 w = state_cold(A.state, A.n)[e0 + slot];
            const float half[3] = {A.target_radius, A.target_radius, A.target_radius};
            put_ray_prim(recs[slot * kRayEnvPrims + kNumVisuals], diag3(1.f), V3{w.x, w.y, w.z}, kVisSphere, half, A.target_radius, kSegTarget);
        }
    }
    if (nb > 0) {
        if (tid < nb) bodies[tid] = A.bodies[tid];
        for (int k = tid; k < nenv * nb; k += nthreads) {
            const int slot = k / nb, b = k - slot * nb;
            float* c = centres + (slot * kMaxScene + b) * 3;
            if (A.body_pos) {
                const float* bp = A.body_pos + ((e0 + slot) * A.n_bodies + b) * 3;
                c[0] = bp[0]; c[1] = bp[1]; c[2] = bp[2];
            } else {
                c[0] = A.bodies[b].c[0]; c[1] = A.bodies[b].c[1]; c[2] = A.bodies[b].c[2];
            }
        }
    }
    if constexpr (SCENE) {
        // the env's moving sphere (words 0-2 centre, 6 mass, 7 radius), label kSegMovingBody; an env without one (mass <= 0) gets a
        // negative bound2: no segment comes that close, so every ray's early-out skips it
        RayPrim* const spheres = reinterpret_cast<RayPrim*>(poses + A.max_envs * (12 * kDof));   // [max_envs]
        for (int slot = tid; slot < nenv; slot += nthreads) {
            const float* w = A.sphere + (e0 + slot);
            const float m = w[6 * A.n], r = w[7 * A.n];
            const float half[3] = {r, r, r};
            RayPrim& Q = spheres[slot];
            put_ray_prim(Q, diag3(1.f), V3{w[0], w[A.n], w[2 * A.n]}, kVisSphere, half, r, kSegMovingBody);
            if (!(m > 0.f)) Q.bound2 = -1.f;
        }
    }
    __syncthreads();

    // ---- per ray ----
    const long long g = g0 + tid;
    if (tid >= A.span || g >= A.total) return;
    const long long e = g / A.n_rays;
    const int slot = (int)(e - e0);
    const float* ray = A.rays + (A.per_env ? g : g - e * A.n_rays) * 6;
    V3 from = {ray[0], ray[1], ray[2]}, to = {ray[3], ray[4], ray[5]};
    if (A.parent_body >= 0) {
        const float* f = frames + slot * 12;
        const M3 R = {{f[0], f[1], f[2]}, {f[3], f[4], f[5]}, {f[6], f[7], f[8]}};
        const V3 p = {f[9], f[10], f[11]};
        from = p + mul(R, from);
        to = p + mul(R, to);
    }
    const V3 d = to - from;
    const float dd = dot(d, d);
    const float inv_dd = dd > 0.f ? 1.f / dd : 0.f;
    RayBest best = {INFINITY, -1};
    const RayPrim* mine = recs + slot * kRayEnvPrims;
    if (arm) {
        for (int i = 0; i < kNumVisuals; ++i) {
            const RayPrim& Q = mine[i];
            // every env's table has the same shape at index i
            ray_against(Q, V3{Q.c[0], Q.c[1], Q.c[2]}, __builtin_amdgcn_readfirstlane(Q.shape), i, from, d, inv_dd, best);
        }
    }
    if (with_target) {
        const RayPrim& Q = mine[kNumVisuals];
        ray_against(Q, V3{Q.c[0], Q.c[1], Q.c[2]}, kVisSphere, kNumVisuals, from, d, inv_dd, best);
    }
    const float* cen = centres + slot * (3 * kMaxScene);
    for (int b = 0; b < nb; ++b) {
        const RayPrim& Q = bodies[b];
        ray_against(Q, V3{cen[3 * b], cen[3 * b + 1], cen[3 * b + 2]}, __builtin_amdgcn_readfirstlane(Q.shape), kRayEnvPrims + b, from, d,
                    inv_dd, best);
    }
    const RayPrim* sphere_rec = nullptr;
    if constexpr (SCENE) {
        sphere_rec = reinterpret_cast<const RayPrim*>(poses + A.max_envs * (12 * kDof)) + slot;
        ray_against(*sphere_rec, V3{sphere_rec->c[0], sphere_rec->c[1], sphere_rec->c[2]}, kVisSphere, kRayIdxSphere, from, d, inv_dd, best);
    }
    const bool hit = best.idx >= 0 && dd > 0.f;                       // a zero-length ray misses
    float frac = 1.f, label = 0.f;
    V3 pos = to, nrm = {0.f, 0.f, 0.f};
    if (hit) {
        const bool sph = SCENE && best.idx == kRayIdxSphere;
        const bool own = best.idx < kRayEnvPrims || sph;               // a record that carries its own centre
        const RayPrim& Q = sph ? *sphere_rec : own ? mine[best.idx] : bodies[best.idx - kRayEnvPrims];
        const int b = own ? 0 : best.idx - kRayEnvPrims;
        const V3 c = own ? V3{Q.c[0], Q.c[1], Q.c[2]} : V3{cen[3 * b], cen[3 * b + 1], cen[3 * b + 2]};
        const V3 w = from - c;
        const V3 o = {Q.rt[0] * w.x + Q.rt[1] * w.y + Q.rt[2] * w.z, Q.rt[3] * w.x + Q.rt[4] * w.y + Q.rt[5] * w.z,
                      Q.rt[6] * w.x + Q.rt[7] * w.y + Q.rt[8] * w.z};
        const V3 nu = hit_normal_at(o, Q.rt, Q.h, Q.shape, d, best.t);
        const float nn = dot(nu, nu);
        nrm = (nn > 0.f ? 1.f / sqrtf(nn) : 0.f) * nu;
        frac = best.t;
        pos = from + best.t * d;
        label = (float)Q.label;
    }
    if (A.hits) {
        float4* out = reinterpret_cast<float4*>(A.hits + g * kRayDim);
        stream_store(out, make_float4(frac, pos.x, pos.y, pos.z));
        stream_store(out + 1, make_float4(nrm.x, nrm.y, nrm.z, label));
    }
    if (A.fractions) stream_store(A.fractions + g, frac);
}

}  // namespace pnr

#pragma clang fp contract(off)
