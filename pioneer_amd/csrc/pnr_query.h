// pnr_query.h — what the per-env query kernels share (pnr_links.h, pnr_ik.h, pnr_invdyn.h, pnr_jointstate.h, pnr_contacts.h, pnr_render.h):
// where an env's joints come from, the "one env per lane" prologue, the two LDS-tile flushes and the velocity half of the outward
// sweep.  It defines no kernel and touches none of the step kernels' headers.  Included, with them, by pnr_queries.hip only.
//
// The tile kernels' shape: one env per lane, one 64-lane wave per workgroup.  A lane computes its env's record in registers and
// drops it into its row of an LDS tile whose row stride is ODD (the lanes' ds_write_b32 then hit distinct banks); after
// wave_lds_sync the tile leaves as ONE contiguous span of lane-linear 16-byte non-temporal stores, as flush_tile writes the
// observation.  dst is 16-byte aligned: the caller's buffer is, and a full tile is a multiple of 16 B long.  Nothing past row
// nvalid is written.  Two flushes, on purpose: a dense tile (stride = row length: 143, 207) is copied as it lies, a short last
// tile's tail float by float; the 6 x 6 tile (36 floats at stride 37) is gathered row by row, which the dense kernels do not want.
//
// Deliberately NOT shared: flush_tile of pnr_device.h (its alignment branch).  The contact geometry (box_sdf, body_distance, the
// penalty law, the walk over the sample spheres) is stated once, in pnr_dyn.h, for the step and for pnr_contacts.h alike.  The
// outward sweep is pose_outward (pnr_dyn.h), then velocity_outward, as two calls: link_body_outward's quaternion product sits
// between them, and on either side of one fused call it changes link_state_kernel's register allocation.  chain_jacobian
// (pnr_ik.h) keeps its own walk over pose_outward: it skips the joints beyond the body on a scalar branch and carries no velocity.
#pragma once

#include <hip/hip_runtime.h>

#include "pnr_device.h"
#include "pnr_dyn.h"

// no bit-exactness contract in the queries (float32 against a float64 reference, tolerance-checked): let a*b+c fuse
#pragma clang fp contract(fast)

namespace pnr {

// where the joint state comes from
enum : int {
    kJointSrcBuffer = 0,   // caller's [n][12] float32 (q | qd), 16-byte aligned
    kJointSrcDyn = 1,      // dynamics-mode planar words [36][n]: q = words 0-5, qd = 6-11
    kJointSrcKin = 2,      // kinematic-mode state records (load_env_halves, pnr_device.h): q = r (words 12-17), qd = v (6-11)
};

// The scene queries (pnr_render.h, pnr_rays.h, pnr_contacts.h) have a second form each, for a per-env world: the handle's moving
// sphere and, in the renderer, per-env body positions.  It is the same kernel template at SRC | kQueryScene, so that the forms
// every earlier call launches keep their names (<0>, <1>, <2>) and, their `if constexpr`s being false, their code; the scene
// form's argument struct is the plain one with the per-env world appended (QueryArgs), so the plain forms keep their argument too.
constexpr int kQueryScene = 4;
constexpr int kQueryCamera = 8;        // the renderer's third form (pnr_render.h): SRC | kQueryScene | kQueryCamera, a camera per env
constexpr int kJointSrcMask = 3;
template <int SRC, class Plain, class Scene>
using QueryArgs = std::conditional_t<(SRC & kQueryScene) != 0, Scene, Plain>;

// env e's joints from the source SRC
template <int SRC>
__device__ __forceinline__ void load_joints(const float* __restrict__ src, const float4* __restrict__ state, const long long n,
                                            const long long e, float (&q)[kDof], float (&qd)[kDof])
{
    if (SRC == kJointSrcBuffer) {
        const float4* js = reinterpret_cast<const float4*>(src) + 3 * e;
        const float4 a = js[0], b = js[1], c = js[2];
        q[0] = a.x; q[1] = a.y; q[2] = a.z; q[3] = a.w; q[4] = b.x; q[5] = b.y;
        qd[0] = b.z; qd[1] = b.w; qd[2] = c.x; qd[3] = c.y; qd[4] = c.z; qd[5] = c.w;
    } else if (SRC == kJointSrcDyn) {
#pragma unroll
        for (int i = 0; i < kDof; ++i) { q[i] = src[(long long)i * n + e]; qd[i] = src[(long long)(kDynQd + i) * n + e]; }
    } else {
        HalfRec k[2];
        load_env_halves(state, n, e, 0, k);
        float a[kDof];
#pragma unroll
        for (int p = 0; p < 2; ++p) unpack_record(k[p], a + 3 * p, qd + 3 * p, q + 3 * p);
    }
}

// this lane's env e in a kernel of one env per lane and one wave per workgroup; the wave's tile is envs [tile0, tile0 + nvalid).
// live: e < n (a lane past the batch computes on zero joints and stores nothing)
struct EnvLane { int lane; long long tile0, e; int nvalid; bool live; };

__device__ __forceinline__ EnvLane env_lane(const long long n)
{
    const int lane = threadIdx.x;
    const long long tile0 = (long long)blockIdx.x * kWave, e = tile0 + lane;
    return {lane, tile0, e, (int)((n - tile0) < kWave ? (n - tile0) : kWave), e < n};
}

// q, qd of this lane's env, zero for a lane past the batch
template <int SRC>
__device__ __forceinline__ void load_lane_joints(const float* __restrict__ src, const float4* __restrict__ state, const long long n,
                                                 const EnvLane& L, float (&q)[kDof], float (&qd)[kDof])
{
#pragma unroll
    for (int i = 0; i < kDof; ++i) { q[i] = 0.f; qd[i] = 0.f; }
    if (L.live) load_joints<SRC>(src, state, n, L.e, q, qd);
}

// a wave's dense tile (`total` floats from lds) to its contiguous place at dst
__device__ __forceinline__ void flush_dense_tile(const float* __restrict__ lds, float* __restrict__ dst, int total, int lane)
{
    const int nvec = total >> 2;
    const float4* src4 = reinterpret_cast<const float4*>(lds);
    float4* dst4 = reinterpret_cast<float4*>(dst);
    for (int j = lane; j < nvec; j += kWave) stream_store(dst4 + j, src4[j]);
    for (int j = (nvec << 2) + lane; j < total; j += kWave) stream_store(dst + j, lds[j]);
}

// the 6 x 6 tile of the Jacobian and the mass matrix: 36 floats per env at LDS row stride 37
constexpr int kMat6Dim = kDof * kDof;
constexpr int kMat6RowStride = kMat6Dim + 1;
constexpr int kMat6TileFloats = kWave * kMat6RowStride;          // 2 368 floats = 9 472 B per wave
static_assert(kMat6RowStride % 2 == 1, "an odd row stride keeps the per-lane LDS writes conflict-free");
static_assert(kMat6Dim % 4 == 0, "an env's row is a whole number of float4s: the flush has no partial tail");

// rows [0, nvalid) of it to their contiguous place in out[n][6][6]; a float4 never straddles two rows (36 = 9 x 4)
__device__ __forceinline__ void flush_mat6_tile(const float* __restrict__ lds, float* __restrict__ dst, int nvalid, int lane)
{
    constexpr int kVecPerRow = kMat6Dim / 4;
    const int nvec = nvalid * kVecPerRow;
    float4* dst4 = reinterpret_cast<float4*>(dst);
    for (int j = lane; j < nvec; j += kWave) {
        const int r = j / kVecPerRow;
        const float* src = lds + r * kMat6RowStride + 4 * (j - r * kVecPerRow);
        stream_store(dst4 + j, make_float4(src[0], src[1], src[2], src[3]));
    }
}

// The velocity half of the outward sweep, for any frame type with R, p (of C: already set by pose_outward<J>), v, w: axis = the
// joint's world axis, omega = omega_p + qd axis, v = v_p + omega_p x (p - pp) (the joint's axis passes through the child's origin)
template <int J, class F>
__device__ __forceinline__ void velocity_outward(const F& B, float qd, F& C, V3& axis)
{
    axis = col(C.R, (int)kJoints[J].axis);
    C.w = B.w + qd * axis;
    C.v = B.v + cross(B.w, C.p - B.p);
}

}  // namespace pnr

#pragma clang fp contract(off)
