// pnr_links.h — pnr_get_link_states: world pose and velocity of every URDF link of every env, the batched form of
// Item.pose() / Item.velocity() on a link item (bullet_scene.py:53-67 -> getLinkState(computeLinkVelocity=1,
// computeForwardKinematics=1)).  Included by pnr_api.hip only; it adds a kernel and edits none of the step kernels.
//
// Per env: q[6], qd[6] in, 11 link records of 13 floats out ([0:3] position, [3:7] quaternion x y z w with w >= 0,
// [7:10] linear velocity of the frame origin, [10:13] angular velocity; world frame).  Link k is Bullet's link_index
// = the URDF joint order (pnr_model.h kLinkBody).  Every link's inertial frame sits at its link frame origin, so the
// frame origin's velocity is Bullet's COM velocity.
//
// Shape: one env per lane, one 64-lane wave per workgroup.  The forward sweep (pose, then velocity) runs over the
// six moving bodies of pnr_model.h in registers and drops each link's record into an LDS tile of [64][143] floats
// (row stride 143 is odd: the lanes' ds_write_b32 hit 64 distinct banks); the tile then leaves as ONE contiguous
// 36 608-B span of 16-byte non-temporal stores, as flush_tile writes the observation.  572 B out per env against
// 48-96 B in and a few hundred FLOPs: the kernel is write-bound.
#pragma once

#include <hip/hip_runtime.h>

#include "pnr_device.h"
#include "pnr_dyn.h"

// no bit-exactness contract here (float32 against a float64 reference, tolerance-checked): let a*b+c fuse
#pragma clang fp contract(fast)

namespace pnr {

constexpr int kLinkStateDim = 13;
constexpr int kLinkRowFloats = kNumLinks * kLinkStateDim;       // 143 floats = 572 B per env
constexpr int kLinkTileFloats = kWave * kLinkRowFloats;         // 9 152 floats = 36 608 B per wave
static_assert(kLinkRowFloats % 2 == 1, "an odd row stride keeps the per-lane LDS writes conflict-free");

// where the joint state comes from
enum : int {
    kLinkSrcBuffer = 0,   // caller's [n][12] float32 (q | qd), 16-byte aligned
    kLinkSrcDyn = 1,      // dynamics-mode planar words [36][n]: q = words 0-5, qd = 6-11
    kLinkSrcKin = 2,      // kinematic-mode state planes (load_state_raw's layout): q = r (words 12-17), qd = v (6-11)
};

struct LinkBody {
    M3 R;                 // world rotation
    V3 p;                 // world position of the frame origin
    float qx, qy, qz, qw; // world rotation as a quaternion
    V3 v, w;              // linear velocity of the origin, angular velocity
};

// one record: 13 consecutive floats of this lane's LDS row
__device__ __forceinline__ void put_link(float* rec, V3 p, float qx, float qy, float qz, float qw, V3 v, V3 w)
{
    // canonical sign: w >= 0 (q and -q are the same rotation)
    const float sg = qw < 0.f ? -1.f : 1.f;
    rec[0] = p.x; rec[1] = p.y; rec[2] = p.z;
    rec[3] = sg * qx; rec[4] = sg * qy; rec[5] = sg * qz; rec[6] = sg * qw;
    rec[7] = v.x; rec[8] = v.y; rec[9] = v.z;
    rec[10] = w.x; rec[11] = w.y; rec[12] = w.z;
}

// body J from its parent B: R = Rp R(axis, q), p = pp + Rp o_J (pose_outward), quaternion Qp (x) (sin(q/2) axis, cos(q/2)),
// omega = omega_p + qd axis_world, v = v_p + omega_p x (p - pp) (the joint's axis passes through the child's origin)
template <int J>
__device__ __forceinline__ void link_body_outward(const LinkBody& B, float q, float qd, LinkBody& C)
{
    constexpr int AXJ = (int)kJoints[J].axis;
    float sh, ch;
    sincos_any(0.5f * q, sh, ch);
    const float c = (ch - sh) * (ch + sh), s = 2.f * sh * ch;
    pose_outward<J>(B.R, B.p, c, s, C.R, C.p);
    const float x = B.qx, y = B.qy, z = B.qz, w = B.qw;
    if (AXJ == (int)AX) { C.qx = w * sh + x * ch; C.qy = y * ch + z * sh; C.qz = z * ch - y * sh; C.qw = w * ch - x * sh; }
    else if (AXJ == (int)AY) { C.qx = x * ch - z * sh; C.qy = w * sh + y * ch; C.qz = x * sh + z * ch; C.qw = w * ch - y * sh; }
    else { C.qx = x * ch + y * sh; C.qy = y * ch - x * sh; C.qz = w * sh + z * ch; C.qw = w * ch - z * sh; }
    const V3 axis = col(C.R, AXJ);
    C.w = B.w + qd * axis;
    C.v = B.v + cross(B.w, C.p - B.p);
}

// the 11 records of one env into `row` (143 floats)
__device__ __forceinline__ void link_states_env(const float (&q)[kDof], const float (&qd)[kDof], float* row)
{
    LinkBody b;
    b.R = diag3(1.f); b.p = {0.f, 0.f, 0.f};
    b.qx = b.qy = b.qz = 0.f; b.qw = 1.f;
    b.v = {0.f, 0.f, 0.f}; b.w = {0.f, 0.f, 0.f};
    put_link(row, b.p, b.qx, b.qy, b.qz, b.qw, b.v, b.w);            // link 0, robot:base: static at the origin
    static_for<kDof>([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        LinkBody c;
        link_body_outward<J>(b, q[J], qd[J], c);
        b = c;
#pragma unroll
        for (int k = 1; k < kNumLinks; ++k)                          // every link lumped into moving body J
            if (kLinkBody[k] == J && k != kNumLinks - 1)
                put_link(row + kLinkStateDim * k, b.p, b.qx, b.qy, b.qz, b.qw, b.v, b.w);
    });
    // link 10, robot:pointer: body 6's frame moved by kTip (effector_to_pointer, rpy 0)
    static_assert(kLinkBody[kNumLinks - 1] == kDof - 1, "the pointer is the last link, on the last body");
    const V3 tip = mul(b.R, V3{(float)kTipX, (float)kTipY, (float)kTipZ});
    put_link(row + kLinkStateDim * (kNumLinks - 1), b.p + tip, b.qx, b.qy, b.qz, b.qw, b.v + cross(b.w, tip), b.w);
}

// Copy a wave's tile (rows [0, nvalid) of 143 floats) to its contiguous place in out[n][11][13]: 16-byte lane-linear
// non-temporal stores (dst is 16-byte aligned: the caller's buffer is, and every tile starts 36 608 B further on), the
// last partial float4 of a short tile as single floats.  Nothing past row nvalid is written.
__device__ __forceinline__ void flush_link_tile(const float* __restrict__ lds, float* __restrict__ dst, int nvalid, int lane)
{
    const int total = nvalid * kLinkRowFloats;
    const int nvec = total >> 2;
    const float4* src4 = reinterpret_cast<const float4*>(lds);
    float4* dst4 = reinterpret_cast<float4*>(dst);
    for (int j = lane; j < nvec; j += kWave) stream_store(dst4 + j, src4[j]);
    for (int j = (nvec << 2) + lane; j < total; j += kWave) stream_store(dst + j, lds[j]);
}

// env e's joints from the source SRC (also pnr_render.h's)
template <int SRC>
__device__ __forceinline__ void load_link_joints(const float* __restrict__ src, const float4* __restrict__ state, const long long n,
                                                 const long long e, float (&q)[kDof], float (&qd)[kDof])
{
    if (SRC == kLinkSrcBuffer) {
        const float4* js = reinterpret_cast<const float4*>(src) + 3 * e;
        const float4 a = js[0], b = js[1], c = js[2];
        q[0] = a.x; q[1] = a.y; q[2] = a.z; q[3] = a.w; q[4] = b.x; q[5] = b.y;
        qd[0] = b.z; qd[1] = b.w; qd[2] = c.x; qd[3] = c.y; qd[4] = c.z; qd[5] = c.w;
    } else if (SRC == kLinkSrcDyn) {
#pragma unroll
        for (int i = 0; i < kDof; ++i) { q[i] = src[(long long)i * n + e]; qd[i] = src[(long long)(kDynQd + i) * n + e]; }
    } else {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const RawState raw = load_state_raw(state, n, 2 * e + p);
            qd[3 * p] = raw.p0.w; qd[3 * p + 1] = raw.p1.x; qd[3 * p + 2] = raw.p1.y;
            q[3 * p] = raw.p1.z; q[3 * p + 1] = raw.p1.w; q[3 * p + 2] = raw.p2.x;
        }
    }
}

template <int SRC>
__global__ __launch_bounds__(kWave) void link_state_kernel(const float* __restrict__ src, const float4* __restrict__ state,
                                                           float* __restrict__ out, const long long n)
{
    __shared__ __attribute__((aligned(16))) float tile[kLinkTileFloats];
    const int lane = threadIdx.x;
    const long long tile0 = (long long)blockIdx.x * kWave;
    const long long e = tile0 + lane;
    const int nvalid = (int)((n - tile0) < kWave ? (n - tile0) : kWave);
    float q[kDof], qd[kDof];
#pragma unroll
    for (int i = 0; i < kDof; ++i) { q[i] = 0.f; qd[i] = 0.f; }
    if (e < n) load_link_joints<SRC>(src, state, n, e, q, qd);
    link_states_env(q, qd, tile + lane * kLinkRowFloats);
    wave_lds_sync();
    flush_link_tile(tile, out + tile0 * kLinkRowFloats, nvalid, lane);
}

}  // namespace pnr

#pragma clang fp contract(off)
