// pnr_render.h — pnr_render: camera images of every env (rgb, eye depth, segmentation) from the URDF's <visual> shapes, the
// target sphere and the caller's static bodies: the batched form of the reference's render('rgb_array')
// (bullet_env.py:156-185 -> getCameraImage).  Included by pnr_queries.hip only, whose code object holds no step kernel.
//
// Scene of one env: the 14 visuals of the URDF posed by the env's joints (table below, in moving-body frames), the target
// sphere (translucent) and up to kMaxScene static bodies shared by all envs.  Every shape is analytic: a ray meets a box by
// slabs, a capped cylinder by a quadratic and a slab, a sphere by a quadratic, a plane by one division.
//
// Shape: one 256-thread workgroup per (env, tile of kRenderThreads * ppl consecutive pixels in row-major order): a tile is one
// contiguous span of each output.  Prologue: wave 0 sweeps the six body poses (link_body_outward, as pnr_get_link_states does)
// into LDS; lanes then build one world-space record per primitive (the eye in the primitive's frame, the world -> primitive
// rotation, half sizes, colour, a conservative pixel rectangle from the bounding sphere).  Per pixel: one world ray (depth along
// the view axis = the ray parameter), a loop over the primitives with a wave-uniform index whose records are LDS broadcasts,
// skipped where the primitive's rectangle misses the wave's 64 pixels (a scalar branch), a branch-free nearest hit, one shading
// from the winner's record.  The tile's bytes are staged in LDS and leave as lane-linear 16-byte non-temporal stores; only the
// partial 16-byte chunks at a span's two ends are written byte by byte.
//
// The scene form (render_kernel<SRC | kQueryScene>, pnr_query.h; pnr_render_bodies, and pnr_render where the handle shows its moving
// sphere): each body's lane re-places the host's record at the env's own position, and one more lane builds the env's moving
// sphere as one more primitive in one more slot.  The per-pixel loop is the same text.
//
// The camera form (render_kernel<SRC | kQueryScene | kQueryCamera>; pnr_render_cameras): a camera per env, in the world or on a
// link of the env's arm.  Lane 0, once its sweep has filled pose[][], reads the env's camera row (position | quaternion in the
// parent frame), composes it with the parent link's body pose and writes eye, right, up, back as one more 12-word row behind
// the poses; the prologue's barrier covers it.  Every record is then built from that row (the static bodies too: their centres
// travel in the argument, as the host's records hold none), and the per-pixel loop takes right, up, back from it into SGPRs.
#pragma once

#include <hip/hip_runtime.h>

#include "pnr_device.h"
#include "pnr_dyn.h"
#include "pnr_links.h"

// float32 against a float64 reference with an ambiguity band: let a*b+c fuse
#pragma clang fp contract(fast)

namespace pnr {

enum : int { kVisBox = 0, kVisCylinder = 1, kVisSphere = 2, kVisPlane = 3 };
enum : int { kSegBackground = 0, kSegLink0 = 1, kSegTarget = 12, kSegBody0 = 13, kSegMovingBody = kSegBody0 + kMaxScene };

// One <visual> of the URDF (pioneer_knm_6dof.urdf:36-202), in the frame of moving body `body` (pnr_model.h: kLinkBody of its
// link; every fixed joint is the identity except effector_to_pointer, so the pointer's sphere sits at kTip).  rot: visual
// frame -> body frame, row-major, built from the rpy text values (0 -1.5708 0 | 0 3.1416 0 | 0 1.5708 0: rotations about y);
// a cylinder lies along its visual frame's z axis.  half: box half extents | cylinder (radius, radius, length / 2) | sphere
// (radius x 3).  rgba: the visual's <material>.
struct VisualDef { int link, body, shape; float rot[9]; float t[3]; float half[3]; float rgba[4]; };
constexpr int kNumVisuals = 14;
constexpr VisualDef kVisuals[kNumVisuals] = {
    // link body shape        rotation (visual -> body, row-major)                                                  translation         half sizes            rgba
    {1, 0, kVisCylinder, {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {0.f, 0.f, 0.5f}, {4.f, 4.f, 0.5f}, {0.175f, 0.175f, 0.175f, 1.f}},
    {2, 0, kVisBox, {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {0.f, 0.f, 1.5f}, {1.f, 1.5f, 0.5f}, {1.f, 0.5f, 0.05f, 1.f}},
    {2, 0, kVisBox, {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {0.f, -1.f, 3.f}, {1.f, 0.5f, 1.f}, {1.f, 0.5f, 0.05f, 1.f}},
    {2, 0, kVisBox, {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {0.f, 1.f, 3.f}, {1.f, 0.5f, 1.f}, {1.f, 0.5f, 0.05f, 1.f}},
    {3, 1, kVisBox, {kCos1_5708, 0.f, -kSin1_5708, 0.f, 1.f, 0.f, kSin1_5708, 0.f, kCos1_5708}, {0.f, 0.f, 6.f}, {6.f, 0.5f, 1.f}, {0.07f, 0.25f, 0.54f, 1.f}},
    {4, 2, kVisBox, {kCos3_1416, 0.f, kSin3_1416, 0.f, 1.f, 0.f, -kSin3_1416, 0.f, kCos3_1416}, {4.f, 1.f, 0.f}, {5.f, 0.5f, 1.f}, {0.07f, 0.25f, 0.54f, 1.f}},
    {5, 3, kVisCylinder, {kCos1_5708, 0.f, kSin1_5708, 0.f, 1.f, 0.f, -kSin1_5708, 0.f, kCos1_5708}, {9.2f, 0.f, 0.f}, {1.f, 1.f, 0.2f}, {0.175f, 0.175f, 0.175f, 1.f}},
    {6, 3, kVisBox, {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {10.4f, 0.f, 0.f}, {1.f, 0.25f, 0.5f}, {1.f, 0.5f, 0.05f, 1.f}},
    {7, 4, kVisBox, {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {1.f, 0.5f, 0.f}, {1.5f, 0.25f, 0.5f}, {0.07f, 0.25f, 0.54f, 1.f}},
    {7, 4, kVisBox, {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {1.f, -0.5f, 0.f}, {1.5f, 0.25f, 0.5f}, {0.07f, 0.25f, 0.54f, 1.f}},
    {8, 5, kVisCylinder, {kCos1_5708, 0.f, kSin1_5708, 0.f, 1.f, 0.f, -kSin1_5708, 0.f, kCos1_5708}, {2.6f, 0.f, 0.f}, {1.f, 1.f, 0.2f}, {0.175f, 0.175f, 0.175f, 1.f}},
    {9, 5, kVisBox, {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {3.2f, 0.f, 0.f}, {0.5f, 0.1f, 0.1f}, {1.f, 0.5f, 0.05f, 1.f}},
    {9, 5, kVisBox, {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {3.6f, 0.f, 0.5f}, {0.1f, 0.1f, 1.25f}, {1.f, 0.5f, 0.05f, 1.f}},
    {10, 5, kVisSphere, {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {3.6f, 0.f, 1.9f}, {0.2f, 0.2f, 0.2f}, {0.1f, 0.9f, 0.1f, 1.f}},
};
static_assert(kVisuals[kNumVisuals - 1].t[0] == (float)kTipX && kVisuals[kNumVisuals - 1].t[1] == (float)kTipY &&
              kVisuals[kNumVisuals - 1].t[2] == (float)kTipZ, "the pointer's sphere sits at kTip");

constexpr int kRenderThreads = 256;
constexpr int kRenderMaxPpl = 4;                                  // pixels per lane (tile = 256 * ppl pixels)
constexpr int kRenderMaxTile = kRenderThreads * kRenderMaxPpl;
constexpr int kRenderPrims = 1 + kNumVisuals + kMaxScene;        // target, visuals, static bodies

// One primitive in world space, as the per-pixel loop reads it (24 words).
struct RenderPrim {
    float rt[9];           // world -> primitive frame (rows); a sphere's is unused (the identity)
    float o[3];            // the eye in the primitive frame (a plane: o[2] = n . (eye - point))
    float h[3];            // box half extents | cylinder radius, radius, half length | sphere radius
    float rgb[3];
    int shape, label;
    int x0, x1, y0, y1;    // conservative pixel rectangle, inclusive; x0 > x1: nothing to draw
};

// The launch's constants (kernel argument): the camera and the static bodies, built on the host.
struct RenderParams {
    float eye[3];
    float right[3], up[3], back[3];   // rows of the view rotation: eye axes in the world frame
    float sx, sy;                     // x_eye / depth = ndc_x * sx, y_eye / depth = ndc_y * sy
    float near_clip, far_clip;
    float light[3];                   // unit, towards the light
    float ambient, diffuse;
    float bg[3];
    float target_rgb[3], target_alpha, target_radius;
    int W, H, HW;
    int ppl, tiles;                   // pixels per lane, tiles per env
    int n_static;
    RenderPrim bodies[kMaxScene];
};

// Conservative pixel rectangle of a sphere (eye-space centre x, y, depth along the view axis; radius r): the box
// [x +- r] x [depth +- r] contains it, so the extremes of x / depth over the box's corners bound its projection.  Empty beyond
// the far plane, the whole screen where it reaches the near plane; one pixel of margin.
__host__ __device__ inline void sphere_rect(float cx, float cy, float depth, float r, const RenderParams& P, int& x0, int& x1,
                                            int& y0, int& y1)
{
    if (!(depth - r < P.far_clip)) { x0 = 1; x1 = 0; y0 = 1; y1 = 0; return; }
    if (!(depth - r > P.near_clip)) { x0 = 0; x1 = P.W - 1; y0 = 0; y1 = P.H - 1; return; }
    const float zl = depth - r, zh = depth + r;
    const float xa = cx + r, xb = cx - r, ya = cy + r, yb = cy - r;
    const float sxmax = (xa >= 0.f ? xa / zl : xa / zh) / P.sx, sxmin = (xb >= 0.f ? xb / zh : xb / zl) / P.sx;
    const float symax = (ya >= 0.f ? ya / zl : ya / zh) / P.sy, symin = (yb >= 0.f ? yb / zh : yb / zl) / P.sy;
    // pixel x = (ndc_x + 1) W / 2 - 1/2, pixel y = (1 - ndc_y) H / 2 - 1/2
    const float W = (float)P.W, H = (float)P.H;
    const float fx0 = fminf(fmaxf(floorf((sxmin + 1.f) * 0.5f * W - 0.5f) - 1.f, -1.f), W);
    const float fx1 = fminf(fmaxf(ceilf((sxmax + 1.f) * 0.5f * W - 0.5f) + 1.f, -1.f), W);
    const float fy0 = fminf(fmaxf(floorf((1.f - symax) * 0.5f * H - 0.5f) - 1.f, -1.f), H);
    const float fy1 = fminf(fmaxf(ceilf((1.f - symin) * 0.5f * H - 0.5f) + 1.f, -1.f), H);
    x0 = (int)fx0; x1 = (int)fx1; y0 = (int)fy0; y1 = (int)fy1;
}

__device__ __forceinline__ float nonzero(float d) { return fabsf(d) < 1e-20f ? (d < 0.f ? -1e-20f : 1e-20f) : d; }

// A camera as the prologue reads it: the eye and the eye axes in the world frame.  RenderParams holds the shared one under these
// names (the plain and the scene form pass P itself for it); the camera form builds one per env in LDS.
struct RenderCamera { float eye[3]; float right[3], up[3], back[3]; };

// the eye-space centre of a world point seen by camera C
template <class Cam>
__device__ __forceinline__ void eye_space(const Cam& C, V3 c, float& cx, float& cy, float& depth)
{
    const V3 d = c - V3{C.eye[0], C.eye[1], C.eye[2]};
    cx = dot(V3{C.right[0], C.right[1], C.right[2]}, d);
    cy = dot(V3{C.up[0], C.up[1], C.up[2]}, d);
    depth = -dot(V3{C.back[0], C.back[1], C.back[2]}, d);
}

// record of a shape whose world rotation is R (shape frame -> world) and centre c, seen by camera C
template <class Cam>
__device__ __forceinline__ void put_prim(RenderPrim& Q, const RenderParams& P, const Cam& C, const M3& R, V3 c, int shape,
                                         const float* half, float bound, const float* rgb, int label)
{
    const V3 e = V3{C.eye[0], C.eye[1], C.eye[2]} - c;
    const V3 c0 = col(R, 0), c1 = col(R, 1), c2 = col(R, 2);          // rows of R^T
    Q.rt[0] = c0.x; Q.rt[1] = c0.y; Q.rt[2] = c0.z;
    Q.rt[3] = c1.x; Q.rt[4] = c1.y; Q.rt[5] = c1.z;
    Q.rt[6] = c2.x; Q.rt[7] = c2.y; Q.rt[8] = c2.z;
    Q.o[0] = dot(c0, e); Q.o[1] = dot(c1, e); Q.o[2] = dot(c2, e);
    Q.h[0] = half[0]; Q.h[1] = half[1]; Q.h[2] = half[2];
    Q.rgb[0] = rgb[0]; Q.rgb[1] = rgb[1]; Q.rgb[2] = rgb[2];
    Q.shape = shape; Q.label = label;
    float cx, cy, depth;
    eye_space(C, c, cx, cy, depth);
    sphere_rect(cx, cy, depth, bound, P, Q.x0, Q.x1, Q.y0, Q.y1);
}

// the ray o + t d against one primitive: the entering and the leaving parameter (tn <= tf when it hits).  o: the ray's origin in
// the primitive frame; rt: world -> primitive rotation (rows), h: half sizes, dw: the world direction.  Shared with pnr_rays.h,
// whose origins differ per ray.
__device__ __forceinline__ void intersect_at(V3 o, const float* rt, const float* h, int shape, V3 dw, float& tn, float& tf)
{
    if (shape == kVisSphere) {                                       // |o + t d|^2 = r^2 from the closest approach
        const float a = dot(dw, dw), tc = -dot(o, dw) * fast_rcp(a);
        const V3 v = o + tc * dw;
        const float disc = h[0] * h[0] - dot(v, v);
        const float half = sqrtf(fmaxf(disc, 0.f) * fast_rcp(a));
        tn = disc >= 0.f ? tc - half : 1.f;
        tf = disc >= 0.f ? tc + half : 0.f;
        return;
    }
    const V3 d = {rt[0] * dw.x + rt[1] * dw.y + rt[2] * dw.z, rt[3] * dw.x + rt[4] * dw.y + rt[5] * dw.z,
                  rt[6] * dw.x + rt[7] * dw.y + rt[8] * dw.z};
    if (shape == kVisPlane) {
        tn = tf = -o.z * fast_rcp(nonzero(d.z));
        return;
    }
    const float iz = fast_rcp(nonzero(d.z));
    const float za = (-h[2] - o.z) * iz, zb = (h[2] - o.z) * iz;
    if (shape == kVisBox) {
        const float ix = fast_rcp(nonzero(d.x)), iy = fast_rcp(nonzero(d.y));
        const float xa = (-h[0] - o.x) * ix, xb = (h[0] - o.x) * ix;
        const float ya = (-h[1] - o.y) * iy, yb = (h[1] - o.y) * iy;
        tn = fmaxf(fmaxf(fminf(xa, xb), fminf(ya, yb)), fminf(za, zb));
        tf = fminf(fminf(fmaxf(xa, xb), fmaxf(ya, yb)), fmaxf(za, zb));
        return;
    }
    // capped cylinder along z: the side's interval (all of t when the ray runs along the axis inside it) and the caps' slab
    const float a = d.x * d.x + d.y * d.y;
    const bool along = a < 1e-24f;
    const float tc = along ? 0.f : -(o.x * d.x + o.y * d.y) * fast_rcp(a);
    const float vx = o.x + tc * d.x, vy = o.y + tc * d.y;
    const float disc = h[0] * h[0] - (vx * vx + vy * vy);
    const float half = along ? 1e30f : sqrtf(fmaxf(disc, 0.f) * fast_rcp(a));
    tn = disc >= 0.f ? fmaxf(tc - half, fminf(za, zb)) : 1.f;
    tf = disc >= 0.f ? fminf(tc + half, fmaxf(za, zb)) : 0.f;
}

// .. of the ray from the eye (t = eye depth): the record holds the eye in the primitive frame
__device__ __forceinline__ void intersect(const RenderPrim& Q, int shape, V3 dw, float& tn, float& tf)
{
    intersect_at(V3{Q.o[0], Q.o[1], Q.o[2]}, Q.rt, Q.h, shape, dw, tn, tf);
}

// outward normal (world, not normalised) of a primitive at the parameter t of the ray o + t d (arguments as intersect_at's)
__device__ __forceinline__ V3 hit_normal_at(V3 o, const float* rt, const float* h, int shape, V3 dw, float t)
{
    const V3 r0 = {rt[0], rt[1], rt[2]}, r1 = {rt[3], rt[4], rt[5]}, r2 = {rt[6], rt[7], rt[8]};
    if (shape == kVisSphere) return o + t * dw;
    if (shape == kVisPlane) return r2;
    const V3 p = o + t * V3{dot(r0, dw), dot(r1, dw), dot(r2, dw)};      // hit point in the primitive frame
    V3 nl;
    if (shape == kVisBox) {                                         // the face whose slab the point lies on
        const float ax = fabsf(p.x) / h[0], ay = fabsf(p.y) / h[1], az = fabsf(p.z) / h[2];
        nl = (ax >= ay && ax >= az) ? V3{p.x, 0.f, 0.f} : (ay >= az ? V3{0.f, p.y, 0.f} : V3{0.f, 0.f, p.z});
    } else {                                                        // cylinder: a cap or the side
        const float rad = sqrtf(p.x * p.x + p.y * p.y);
        nl = fabsf(p.z) / h[2] >= rad / h[0] ? V3{0.f, 0.f, p.z} : V3{p.x, p.y, 0.f};
    }
    return nl.x * r0 + nl.y * r1 + nl.z * r2;                       // R n = R^T's rows weighted
}

// .. of primitive Q at the eye ray's parameter t
__device__ __forceinline__ V3 hit_normal(const RenderPrim& Q, V3 dw, float t)
{
    return hit_normal_at(V3{Q.o[0], Q.o[1], Q.o[2]}, Q.rt, Q.h, Q.shape, dw, t);
}

// Lambert with ambient: rgb (ambient + diffuse max(0, n . l)), clamped to [0, 1]; the normal faces the viewer
__device__ __forceinline__ V3 shade(const RenderParams& P, const float* rgb, V3 n, V3 dw)
{
    const float nn = dot(n, n);
    const float s = (dot(n, dw) > 0.f ? -1.f : 1.f) * (nn > 0.f ? 1.f / sqrtf(nn) : 0.f);
    const float ndl = s * dot(n, V3{P.light[0], P.light[1], P.light[2]});
    const float k = P.ambient + P.diffuse * fmaxf(ndl, 0.f);
    return {fminf(fmaxf(rgb[0] * k, 0.f), 1.f), fminf(fmaxf(rgb[1] * k, 0.f), 1.f), fminf(fmaxf(rgb[2] * k, 0.f), 1.f)};
}

__device__ __forceinline__ uint8_t to_byte(float c) { return (uint8_t)(int)floorf(255.f * c + 0.5f); }

typedef unsigned v4u_t __attribute__((ext_vector_type(4)));

// bytes [head, head + bytes) of the 16-byte aligned LDS buffer `lds` -> the same bytes of `dst` (16-byte aligned, `head` bytes
// before the span): whole 16-byte chunks as lane-linear non-temporal stores, the partial chunks at both ends byte by byte.
// Nothing outside the span is written.
__device__ __forceinline__ void flush_span(const uint8_t* __restrict__ lds, uint8_t* __restrict__ dst, int head, int bytes, int tid)
{
    const int end = head + bytes;
    const int nchunk = (end + 15) >> 4;
    for (int c = tid; c < nchunk; c += kRenderThreads) {
        const int b0 = c << 4;
        if (b0 >= head && b0 + 16 <= end) {
            __builtin_nontemporal_store(*reinterpret_cast<const v4u_t*>(lds + b0), reinterpret_cast<v4u_t*>(dst + b0));
        } else {
            const int lo = b0 > head ? b0 : head, hi = b0 + 16 < end ? b0 + 16 : end;
            for (int b = lo; b < hi; ++b) stream_store(dst + b, lds[b]);
        }
    }
}

// The scene form's argument: RenderParams (render_kernel<0..2>'s as it was) and the per-env world, either pointer may be null.
struct RenderSceneParams : RenderParams {
    const float* body_pos;     // [n][n_static][3] world positions that replace the bodies', or null
    const float* sphere;       // [PNR_BODY_STATE_WORDS][n] (pnr_dyn.h WorldBody::words) where the sphere is drawn, or null
    float sphere_rgb[3];
};

// The camera form's argument: the scene form's and the camera mount.  P's eye / right / up / back hold the camera in the PARENT
// frame where `cameras` is null (the inverse of the caller's view); body_centre is what the host's records lack.
struct RenderCameraParams : RenderSceneParams {
    const float* cameras;      // [7] or [n][7]: position | quaternion (x, y, z, w) in the parent frame, or null
    int cam_per_env;           // 1: a row per env
    int cam_body;              // the moving body that carries the parent link; -1: the world
    int cam_tip;               // the parent is the pointer: the body's frame moved by kTip
    float body_centre[kMaxScene][3];   // the static bodies' world centres (a plane: the point it passes through)
};
template <int SRC>
using RenderArgs = std::conditional_t<(SRC & kQueryCamera) != 0, RenderCameraParams, QueryArgs<SRC, RenderParams, RenderSceneParams>>;

// the camera the prologue builds its records from: the launch's (P itself) or, in the camera form, the env's 12-word row in LDS
template <bool CAMERA, class Args>
__device__ __forceinline__ const auto& render_camera(const Args& P, const float* row)
{
    if constexpr (CAMERA) return *reinterpret_cast<const RenderCamera*>(row);
    else return P;
}

// an eye axis for the per-pixel loop: the launch's lies in SGPRs as it is; the env's is an LDS broadcast, made provably uniform
template <bool CAMERA>
__device__ __forceinline__ V3 eye_axis(const float* a)
{
    if constexpr (CAMERA)
        return {__int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a[0]))), __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a[1]))),
                __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a[2])))};
    else
        return {a[0], a[1], a[2]};
}

// env e's camera: its row composed with the parent link's body pose (pose[][], filled by this lane), into `cam`
__device__ __forceinline__ void build_camera(const RenderCameraParams& P, const long long e, const float (*pose)[12], RenderCamera& cam)
{
    V3 le = {P.eye[0], P.eye[1], P.eye[2]};                          // the camera in the parent frame: eye, then its x, y, z axes
    V3 lr = {P.right[0], P.right[1], P.right[2]}, lu = {P.up[0], P.up[1], P.up[2]}, lb = {P.back[0], P.back[1], P.back[2]};
    if (P.cameras) {
        const float* c = P.cameras + (P.cam_per_env ? e * 7 : 0);
        le = {c[0], c[1], c[2]};
        const float s = 1.f / sqrtf(c[3] * c[3] + c[4] * c[4] + c[5] * c[5] + c[6] * c[6]);
        const float x = s * c[3], y = s * c[4], z = s * c[5], w = s * c[6];
        lr = {1.f - 2.f * (y * y + z * z), 2.f * (x * y + z * w), 2.f * (x * z - y * w)};       // the rotation's columns
        lu = {2.f * (x * y - z * w), 1.f - 2.f * (x * x + z * z), 2.f * (y * z + x * w)};
        lb = {2.f * (x * z + y * w), 2.f * (y * z - x * w), 1.f - 2.f * (x * x + y * y)};
    }
    if (P.cam_body >= 0) {
        const float* w = pose[P.cam_body];
        const M3 Rb = {{w[0], w[1], w[2]}, {w[3], w[4], w[5]}, {w[6], w[7], w[8]}};
        V3 pb = {w[9], w[10], w[11]};
        if (P.cam_tip) pb = pb + mul(Rb, V3{(float)kTipX, (float)kTipY, (float)kTipZ});
        le = pb + mul(Rb, le);
        lr = mul(Rb, lr); lu = mul(Rb, lu); lb = mul(Rb, lb);
    }
    cam.eye[0] = le.x; cam.eye[1] = le.y; cam.eye[2] = le.z;
    cam.right[0] = lr.x; cam.right[1] = lr.y; cam.right[2] = lr.z;
    cam.up[0] = lu.x; cam.up[1] = lu.y; cam.up[2] = lu.z;
    cam.back[0] = lb.x; cam.back[1] = lb.y; cam.back[2] = lb.z;
}

template <int SRC>
__global__ __launch_bounds__(kRenderThreads) void render_kernel(const float* __restrict__ src, const float4* __restrict__ state,
                                                                const long long n, const RenderArgs<SRC> P,
                                                                uint8_t* __restrict__ rgb, float* __restrict__ depth, uint8_t* __restrict__ seg)
{
    constexpr bool SCENE = (SRC & kQueryScene) != 0, CAMERA = (SRC & kQueryCamera) != 0;
    static_assert(SCENE || !CAMERA, "the camera form is a scene form");
    static_assert(sizeof(RenderCamera) == 12 * sizeof(float), "the env's camera is one more row behind the poses");
    __shared__ RenderPrim prims[kRenderPrims + (SCENE ? 1 : 0)];    // (the scene form: one more slot, the moving sphere's)
    __shared__ float pose[kDof + (CAMERA ? 1 : 0)][12];               // R (rows), p of the six moving bodies (the camera form: the env's camera behind them)
    const auto& C = render_camera<CAMERA>(P, pose[kDof - 1] + 12);
    __shared__ __attribute__((aligned(16))) uint8_t st_rgb[16 + 3 * kRenderMaxTile];
    __shared__ __attribute__((aligned(16))) uint8_t st_seg[16 + kRenderMaxTile];
    __shared__ __attribute__((aligned(16))) float st_depth[4 + kRenderMaxTile];

    const int tid = threadIdx.x;
    const long long e = (long long)blockIdx.x / P.tiles;
    const int tile = (int)((long long)blockIdx.x - e * P.tiles);
    const int tile_px = kRenderThreads * P.ppl;
    const int px0 = tile * tile_px;
    const int npx = (P.HW - px0) < tile_px ? (P.HW - px0) : tile_px;

    // ---- prologue: body poses (wave 0), then one record per primitive ----
    if (tid < kWave) {
        float q[kDof], qd[kDof];
        load_joints<(SRC & kJointSrcMask)>(src, state, n, e, q, qd);
        LinkBody b = link_base();
        static_for<kDof>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            LinkBody c;
            link_body_outward<J>(b, q[J], 0.f, c);
            b = c;
            if (tid == 0) {
                float* w = pose[J];
                w[0] = b.R.r0.x; w[1] = b.R.r0.y; w[2] = b.R.r0.z; w[3] = b.R.r1.x; w[4] = b.R.r1.y; w[5] = b.R.r1.z;
                w[6] = b.R.r2.x; w[7] = b.R.r2.y; w[8] = b.R.r2.z; w[9] = b.p.x; w[10] = b.p.y; w[11] = b.p.z;
            }
        });
        if constexpr (CAMERA)
            if (tid == 0) build_camera(P, e, pose, *reinterpret_cast<RenderCamera*>(pose[kDof]));    // (behind this lane's own pose writes)
    }
    __syncthreads();
    int nprim = 1 + kNumVisuals + P.n_static;
    if constexpr (SCENE) {
        if (tid > kNumVisuals && tid < nprim) {                      // a static body: the host's record, re-placed at the env's position
            RenderPrim& Q = prims[tid];
            Q = P.bodies[tid - 1 - kNumVisuals];
            if (CAMERA || P.body_pos) {                              // (the camera form: always, the host's record is no env's camera's)
                const float* bp;
                if constexpr (CAMERA) bp = P.body_pos ? P.body_pos + (e * P.n_static + (tid - 1 - kNumVisuals)) * 3 : P.body_centre[tid - 1 - kNumVisuals];
                else bp = P.body_pos + (e * P.n_static + (tid - 1 - kNumVisuals)) * 3;
                const V3 c = {bp[0], bp[1], bp[2]};
                if (Q.shape == kVisPlane) {                          // the host's form: o[2] = n . (eye - point), the whole screen
                    Q.o[2] = dot(V3{Q.rt[6], Q.rt[7], Q.rt[8]}, V3{C.eye[0], C.eye[1], C.eye[2]} - c);
                } else {
                    const M3 R = {{Q.rt[0], Q.rt[3], Q.rt[6]}, {Q.rt[1], Q.rt[4], Q.rt[7]}, {Q.rt[2], Q.rt[5], Q.rt[8]}};   // (rt is R^T)
                    const float half[3] = {Q.h[0], Q.h[1], Q.h[2]}, colour[3] = {Q.rgb[0], Q.rgb[1], Q.rgb[2]};
                    const float bound = Q.shape == kVisBox ? sqrtf(half[0] * half[0] + half[1] * half[1] + half[2] * half[2]) : half[0];
                    put_prim(Q, P, C, R, c, Q.shape, half, bound, colour, Q.label);
                }
            }
        } else if (tid == nprim && P.sphere) {                       // the env's moving sphere (words 0-2 centre, 6 mass, 7 radius)
            const float* w = P.sphere + e;
            const float m = w[6 * n], r = w[7 * n];
            const float half[3] = {r, r, r};
            RenderPrim& Q = prims[tid];
            put_prim(Q, P, C, diag3(1.f), V3{w[0], w[n], w[2 * n]}, kVisSphere, half, r, P.sphere_rgb, kSegMovingBody);
            if (!(m > 0.f)) { Q.x0 = 0x7fffffff; Q.x1 = -1; Q.y0 = 0x7fffffff; Q.y1 = -1; }      // no sphere: a rectangle no wave meets
        }
        nprim += P.sphere ? 1 : 0;
    }
    if (tid == 0) {                                                  // the target (state words 18-20)
        const float4 w = state_cold(state, n)[e];
        const float half[3] = {P.target_radius, P.target_radius, P.target_radius};
        put_prim(prims[0], P, C, diag3(1.f), V3{w.x, w.y, w.z}, kVisSphere, half, P.target_radius, P.target_rgb, kSegTarget);
    } else if (tid <= kNumVisuals) {
        const VisualDef& D = kVisuals[tid - 1];
        const float* w = pose[D.body];
        const M3 Rb = {{w[0], w[1], w[2]}, {w[3], w[4], w[5]}, {w[6], w[7], w[8]}};
        const M3 Rv = {{D.rot[0], D.rot[1], D.rot[2]}, {D.rot[3], D.rot[4], D.rot[5]}, {D.rot[6], D.rot[7], D.rot[8]}};
        // Rb Rv (each row of Rb times Rv); a sphere is intersected in world axes
        const M3 R = D.shape == kVisSphere ? diag3(1.f) : M3{mulT(Rv, Rb.r0), mulT(Rv, Rb.r1), mulT(Rv, Rb.r2)};
        const V3 c = V3{w[9], w[10], w[11]} + mul(Rb, V3{D.t[0], D.t[1], D.t[2]});
        const float bound = sqrtf(D.half[0] * D.half[0] + D.half[1] * D.half[1] + D.half[2] * D.half[2]);
        put_prim(prims[tid], P, C, R, c, D.shape, D.half, D.shape == kVisBox ? bound : (D.shape == kVisSphere ? D.half[0] :
                 sqrtf(D.half[0] * D.half[0] + D.half[2] * D.half[2])), D.rgba, kSegLink0 + D.link);
    } else if (!SCENE && tid < nprim) {
        prims[tid] = P.bodies[tid - 1 - kNumVisuals];
    }
    __syncthreads();

    // ---- per pixel ----
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const V3 right = eye_axis<CAMERA>(C.right), up = eye_axis<CAMERA>(C.up), back = eye_axis<CAMERA>(C.back);
    const float invW = 2.f / (float)P.W, invH = 2.f / (float)P.H;
    const int hrgb = (int)((3 * ((unsigned long long)e * P.HW + px0)) & 15);
    const int hdep = (int)(((unsigned long long)e * P.HW + px0) & 3);
    const int hseg = (int)(((unsigned long long)e * P.HW + px0) & 15);
    for (int k = 0; k < P.ppl; ++k) {
        const int wfirst = px0 + k * kRenderThreads + wave * kWave;   // the wave's first pixel (uniform)
        if (wfirst >= P.HW) break;
        const int wlast = (wfirst + kWave - 1) < (P.HW - 1) ? (wfirst + kWave - 1) : (P.HW - 1);
        const int wy0 = wfirst / P.W, wy1 = wlast / P.W;
        const int wx0 = wy0 == wy1 ? wfirst - wy0 * P.W : 0, wx1 = wy0 == wy1 ? wlast - wy1 * P.W : P.W - 1;
        const int pix = px0 + k * kRenderThreads + tid;
        const bool live = pix < P.HW;
        const int y = pix / P.W, x = pix - y * P.W;
        const float ex = ((float)(2 * x + 1) * 0.5f * invW - 1.f) * P.sx;
        const float ey = (1.f - (float)(2 * y + 1) * 0.5f * invH) * P.sy;
        const V3 dw = ex * right + ey * up - back;                     // eye-space (ex, ey, -1): the parameter is the depth
        float best = INFINITY;
        int bi = -1;
        for (int i = 1; i < nprim; ++i) {
            const RenderPrim& Q = prims[i];
            const int x0 = __builtin_amdgcn_readfirstlane(Q.x0), x1 = __builtin_amdgcn_readfirstlane(Q.x1);
            const int y0 = __builtin_amdgcn_readfirstlane(Q.y0), y1 = __builtin_amdgcn_readfirstlane(Q.y1);
            if (x0 > wx1 || x1 < wx0 || y0 > wy1 || y1 < wy0) continue;
            float tn, tf;
            intersect(Q, __builtin_amdgcn_readfirstlane(Q.shape), dw, tn, tf);
            const float t = tn > P.near_clip ? tn : tf;
            const bool take = tn <= tf && t > P.near_clip && t < P.far_clip && t < best;
            best = take ? t : best;
            bi = take ? i : bi;
        }
        V3 c = {P.bg[0], P.bg[1], P.bg[2]};
        int label = kSegBackground;
        if (bi >= 0) {
            const RenderPrim& Q = prims[bi];
            c = shade(P, Q.rgb, hit_normal(Q, dw, best), dw);
            label = Q.label;
        }
        {   // the translucent target in front of the opaque hit
            const RenderPrim& Q = prims[0];
            const int x0 = __builtin_amdgcn_readfirstlane(Q.x0), x1 = __builtin_amdgcn_readfirstlane(Q.x1);
            const int y0 = __builtin_amdgcn_readfirstlane(Q.y0), y1 = __builtin_amdgcn_readfirstlane(Q.y1);
            if (!(x0 > wx1 || x1 < wx0 || y0 > wy1 || y1 < wy0)) {
                float tn, tf;
                intersect(Q, kVisSphere, dw, tn, tf);
                const float t = tn > P.near_clip ? tn : tf;
                if (tn <= tf && t > P.near_clip && t < P.far_clip && t < best) {
                    const V3 ct = shade(P, Q.rgb, hit_normal(Q, dw, t), dw);
                    const float a = P.target_alpha;
                    c = a * ct + (1.f - a) * c;
                    best = t;
                    label = kSegTarget;
                }
            }
        }
        if (live) {
            const int j = pix - px0;
            if (rgb) { st_rgb[hrgb + 3 * j] = to_byte(c.x); st_rgb[hrgb + 3 * j + 1] = to_byte(c.y); st_rgb[hrgb + 3 * j + 2] = to_byte(c.z); }
            if (depth) st_depth[hdep + j] = best;
            if (seg) st_seg[hseg + j] = (uint8_t)label;
        }
    }
    __syncthreads();
    const unsigned long long g0 = (unsigned long long)e * P.HW + px0;     // the tile's first pixel in the whole batch
    if (rgb) flush_span(st_rgb, rgb + (3 * g0 - hrgb), hrgb, 3 * npx, tid);
    if (depth) flush_span(reinterpret_cast<const uint8_t*>(st_depth), reinterpret_cast<uint8_t*>(depth + (g0 - hdep)), 4 * hdep, 4 * npx, tid);
    if (seg) flush_span(st_seg, seg + (g0 - hseg), hseg, npx, tid);
}

}  // namespace pnr

#pragma clang fp contract(off)
