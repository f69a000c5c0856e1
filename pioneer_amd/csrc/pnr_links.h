// pnr_links.h — pnr_get_link_states: world pose and velocity of every URDF link of every env, the batched form of
// Item.pose() / Item.velocity() on a link item (bullet_scene.py:53-67 -> getLinkState(computeLinkVelocity=1,
// computeForwardKinematics=1)).  Included by pnr_queries.hip only, whose code object holds no step kernel.
//
// Per env: q[6], qd[6] in, 11 link records of 13 floats out ([0:3] position, [3:7] quaternion x y z w with w >= 0,
// [7:10] linear velocity of the frame origin, [10:13] angular velocity; world frame).  Link k is Bullet's link_index
// = the URDF joint order (pnr_model.h kLinkBody).  Every link's inertial frame sits at its link frame origin, so the
// frame origin's velocity is Bullet's COM velocity.
//
// Shape: the tile kernel of pnr_query.h.  The forward sweep (pose, then velocity) runs over the six moving bodies of
// pnr_model.h in registers and drops each link's record into a dense LDS tile of [64][143] floats (36 608 B).  572 B
// out per env against 48-96 B in and a few hundred FLOPs: the kernel is write-bound.
#pragma once

#include <hip/hip_runtime.h>

#include "pnr_device.h"
#include "pnr_dyn.h"
#include "pnr_query.h"

// no bit-exactness contract here (float32 against a float64 reference, tolerance-checked): let a*b+c fuse
#pragma clang fp contract(fast)

namespace pnr {

constexpr int kLinkStateDim = 13;
constexpr int kLinkRowFloats = kNumLinks * kLinkStateDim;       // 143 floats = 572 B per env
constexpr int kLinkTileFloats = kWave * kLinkRowFloats;         // 9 152 floats = 36 608 B per wave
static_assert(kLinkRowFloats % 2 == 1, "an odd row stride keeps the per-lane LDS writes conflict-free");

struct LinkBody {
    M3 R;                 // world rotation
    V3 p;                 // world position of the frame origin
    float qx, qy, qz, qw; // world rotation as a quaternion
    V3 v, w;              // linear velocity of the origin, angular velocity
};

// the static base the sweep starts from: the world frame, at rest
__device__ __forceinline__ LinkBody link_base() { return {diag3(1.f), {0.f, 0.f, 0.f}, 0.f, 0.f, 0.f, 1.f, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}}; }

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

// body J from its parent B: pose_outward at the cos / sin built from the half angle, quaternion Qp (x) (sin(q/2) axis, cos(q/2)),
// velocity_outward
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
    V3 axis;
    velocity_outward<J>(B, qd, C, axis);
}

// the 11 records of one env into `row` (143 floats)
__device__ __forceinline__ void link_states_env(const float (&q)[kDof], const float (&qd)[kDof], float* row)
{
    LinkBody b = link_base();
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

template <int SRC>
__global__ __launch_bounds__(kWave) void link_state_kernel(const float* __restrict__ src, const float4* __restrict__ state,
                                                           float* __restrict__ out, const long long n)
{
    __shared__ __attribute__((aligned(16))) float tile[kLinkTileFloats];
    const EnvLane L = env_lane(n);
    float q[kDof], qd[kDof];
    load_lane_joints<SRC>(src, state, n, L, q, qd);
    link_states_env(q, qd, tile + L.lane * kLinkRowFloats);
    wave_lds_sync();
    flush_dense_tile(tile, out + L.tile0 * kLinkRowFloats, L.nvalid * kLinkRowFloats, L.lane);
}

}  // namespace pnr

#pragma clang fp contract(off)
