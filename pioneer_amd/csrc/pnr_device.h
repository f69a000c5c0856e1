// pnr_device.h — device-side building blocks of the kinematic ("parity mode")
// step: integrator, forward kinematics, reward, reset draws, obs packing.
//
// Work decomposition: TWO lanes per env (a lane pair 2e, 2e+1), three joints per
// lane.  Lane p of the pair owns joints 3p..3p+2: it integrates them, evaluates
// their 15 sin/cos pairs and writes their 63 observation entries; the 12 values
// the other half needs (cos/sin of the partner's joints for the forward
// kinematics) cross by DPP quad_perm, which never touches LDS.  A 64-lane wave
// therefore steps 32 envs and stages a 17.5 KB obs tile, so two waves fit per
// SIMD at 65 536 envs: one wave's stores overlap the other's arithmetic.
//
// Compiled with -ffp-contract=off: the integrator reproduces the reference's
// mixed float32/float64 arithmetic (NumPy 1.x promotion) operation by
// operation, so nothing may be fused behind its back.  Where a fused
// multiply-add is wanted (FK, polynomials) it is written as __builtin_fmaf.
//
// Reference lines are relative to xdralex/pioneer.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "pnr_model.h"

namespace pnr {

constexpr int kWave = 64;
constexpr int kLanesPerEnv = 2;
constexpr int kJpl = kDof / kLanesPerEnv;      // joints per lane
constexpr int kEnvsPerWave = kWave / kLanesPerEnv;
constexpr int kTileFloats = kEnvsPerWave * kObsDim;

// Kernel parameters (by value -> kernarg segment -> scalar loads).
struct KParams {
    float4* state;             // 6n float4 (library-owned), see load_state_raw
    const float* actions;      // step / rollout
    float* obs;
    float* reward;
    uint8_t* done;
    uint8_t* trunc;            // may be null
    float* info;               // may be null, [n][4]
    const uint8_t* mask;       // reset: may be null
    const float* joint_pos;    // reset: may be null, [n][6]
    const float* target_pos;   // reset: may be null, [n][3]
    long long n;
    unsigned long long env_off;
    unsigned seed_lo, seed_hi;
    int T;                     // steps per launch (rollout); 1 for step
    int max_steps;             // TimeLimit; 0 = off
    int auto_reset;
    int diag;                  // timing-only ablation bits (PNR_DIAG), 0 in production
    double dt, eps;            // pioneer_knm_env.py:60-61
    double tlo[3], tspan[3];   // target_lo, target_hi - target_lo
    float v_max[kDof];         // max_v_to_r * (r_hi - r_lo); the limits themselves are constexpr (pnr_model.h)
    float pot_m, pot_s;        // award_max - award_done, award_potential_slope
    float penalty, award_done, done_dist;
    float pad1;
    double done_dist_d;        // done_distance as the reference compares it (a Python float, pioneer_knm_env.py:160)
};

// Per-lane state: this lane's three joints plus the env's common words (held by
// both lanes of the pair after load).
struct LaneState {
    float a[kJpl], v[kJpl], r[kJpl];
    float tgt[3];
    float pot;
    uint32_t step, episode;
};

// LDS hand-off between the lanes of ONE wave (every workgroup here is a single wave).  A wave's DS
// instructions execute in issue order, so a ds_write followed by another lane's ds_read needs no
// s_barrier and, unlike __syncthreads(), no s_waitcnt vmcnt(0): outstanding global stores (the
// previous tile's obs flush) keep draining while the next tile is packed.  The fences only pin
// the compiler's ordering of LDS accesses.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// partner lane's value (lane ^ 1) by DPP quad_perm [1,0,3,2]
__device__ __forceinline__ float xchg(float x)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xF, 0xF, false));
}

// State in HBM: 6n float4 (96 B per env, sizeof(float4) * kStatePlanes * 2 * n), in four parts.  Record (e, p) has index 2e + p:
//   plane 0   float4 [2n] at float4 index 0:    a[3p] a[3p+1] a[3p+2] v[3p]
//   plane 1   float4 [2n] at float4 index 2n:   v[3p+1] v[3p+2] r[3p] r[3p+1]
//   hot half  float2 [2n] at float4 index 4n:   r[3p+2] H        p = 0: H = potential; p = 1: H = step_index
//   cold part float4 [n]  at float4 index 5n:   target x, y, z, episode         (index e)
// so a wave of lane pairs reads / writes planes 0 and 1 with one lane-contiguous 1-KiB dwordx4 each and the hot half with one
// 512-B dwordx2: the 80 bytes of an env that every step changes.  The cold part changes only where an env is reset (or the
// caller sets the state): a step loads it (both lanes of a pair the same 16 bytes) and stores it inside the reset branch only.
struct RawState { float4 p0, p1; float2 h; float4 c; };     // what a lane of the pair loads: its half record and the env's cold words

__device__ __forceinline__ float2* state_hot(float4* st, long long n) { return reinterpret_cast<float2*>(st + 4 * n); }
__device__ __forceinline__ const float2* state_hot(const float4* st, long long n) { return reinterpret_cast<const float2*>(st + 4 * n); }
__device__ __forceinline__ float4* state_cold(float4* st, long long n) { return st + 5 * n; }
__device__ __forceinline__ const float4* state_cold(const float4* st, long long n) { return st + 5 * n; }

__device__ __forceinline__ RawState load_state_raw(const float4* __restrict__ st, long long n, long long rec)
{
    return {st[rec], st[2 * n + rec], state_hot(st, n)[rec], state_cold(st, n)[rec >> 1]};
}

// cold: the env's target or episode changed (both lanes of the pair pass the same; the pair's first lane writes the 16 bytes)
__device__ __forceinline__ void store_state_raw(float4* __restrict__ st, long long n, long long rec, int p, const RawState& w, bool cold)
{
    st[rec] = w.p0; st[2 * n + rec] = w.p1; state_hot(st, n)[rec] = w.h;
    if (cold && !p) state_cold(st, n)[rec >> 1] = w.c;
}

// The one statement of the packing: a half record <-> a, v, r of its three joints
__device__ __forceinline__ void unpack_record(const RawState& k, float* a, float* v, float* r)
{
    a[0] = k.p0.x; a[1] = k.p0.y; a[2] = k.p0.z; v[0] = k.p0.w;
    v[1] = k.p1.x; v[2] = k.p1.y; r[0] = k.p1.z; r[1] = k.p1.w;
    r[2] = k.h.x;
}

__device__ __forceinline__ RawState pack_state(int p, const LaneState& s)
{
    return {make_float4(s.a[0], s.a[1], s.a[2], s.v[0]), make_float4(s.v[1], s.v[2], s.r[0], s.r[1]),
            make_float2(s.r[2], p ? __uint_as_float(s.step) : s.pot),
            make_float4(s.tgt[0], s.tgt[1], s.tgt[2], __uint_as_float(s.episode))};
}

// the pair's lanes each hold one of potential / step_index: one DPP exchange
__device__ __forceinline__ void unpack_state(const RawState& raw, int p, LaneState& s)
{
    unpack_record(raw, s.a, s.v, s.r);
    s.tgt[0] = raw.c.x; s.tgt[1] = raw.c.y; s.tgt[2] = raw.c.z;
    s.episode = __float_as_uint(raw.c.w);
    const float o = xchg(raw.h.y);
    s.pot = p ? o : raw.h.y;
    s.step = __float_as_uint(p ? raw.h.y : o);
}

__device__ __forceinline__ void load_state(const float4* __restrict__ st, long long n, long long rec, int p, LaneState& s)
{
    unpack_state(load_state_raw(st, n, rec), p, s);
}

__device__ __forceinline__ void store_state(float4* __restrict__ st, long long n, long long rec, int p, const LaneState& s, bool cold)
{
    store_state_raw(st, n, rec, p, pack_state(p, s), cold);
}

// One lane, both halves of env base + off (kernels of one env per lane): the env's two half records with their common words
// alongside — C = target xyz for the first half, potential, step_index, episode for the second — as the dynamics kernels carry
// them in registers and through their LDS hand-off.  The addresses are (plane pointer + the wave's first env) + lane offset.
struct HalfRec { float4 p0, p1, p2; };                      // p2 = r[3p+2] C0 C1 C2

__device__ __forceinline__ void load_env_halves(const float4* __restrict__ st, long long n, long long base, int off, HalfRec (&k)[2])
{
    const float4* s0 = st + 2 * base;
    const float4* s1 = st + 2 * n + 2 * base;
    const float2* sh = state_hot(st, n) + 2 * base;
    const float4 c = (state_cold(st, n) + base)[off];
    const float2 h0 = sh[2 * off], h1 = sh[2 * off + 1];
    k[0] = {s0[2 * off], s1[2 * off], make_float4(h0.x, c.x, c.y, c.z)};
    k[1] = {s0[2 * off + 1], s1[2 * off + 1], make_float4(h1.x, h0.y, h1.y, c.w)};
}

__device__ __forceinline__ void unpack_record(const HalfRec& k, float* a, float* v, float* r, float* c = nullptr)
{
    a[0] = k.p0.x; a[1] = k.p0.y; a[2] = k.p0.z; v[0] = k.p0.w;
    v[1] = k.p1.x; v[2] = k.p1.y; r[0] = k.p1.z; r[1] = k.p1.w;
    r[2] = k.p2.x;
    if (c) { c[0] = k.p2.y; c[1] = k.p2.z; c[2] = k.p2.w; }
}

__device__ __forceinline__ HalfRec pack_record(const float* a, const float* v, const float* r, float c0, float c1, float c2)
{
    return {make_float4(a[0], a[1], a[2], v[0]), make_float4(v[1], v[2], r[0], r[1]), make_float4(r[2], c0, c1, c2)};
}

// a pair lane's LaneState from its half record: the common words of the other half cross by DPP
__device__ __forceinline__ void unpack_state(const HalfRec& raw, int p, LaneState& s)
{
    const float4 p2 = raw.p2;
    unpack_record(raw, s.a, s.v, s.r);
    const float o1 = xchg(p2.y), o2 = xchg(p2.z), o3 = xchg(p2.w);
    s.tgt[0] = p ? o1 : p2.y; s.tgt[1] = p ? o2 : p2.z; s.tgt[2] = p ? o3 : p2.w;
    s.pot = p ? p2.y : o1;
    s.step = __float_as_uint(p ? p2.z : o2);
    s.episode = __float_as_uint(p ? p2.w : o3);
}

__device__ __forceinline__ void zero_state(LaneState& s)
{
#pragma unroll
    for (int i = 0; i < kJpl; ++i) { s.a[i] = 0.f; s.v[i] = 0.f; s.r[i] = 0.f; }
    s.tgt[0] = s.tgt[1] = s.tgt[2] = 0.f; s.pot = 0.f; s.step = 0; s.episode = 0;
}

// Per-joint constants of this lane's joints (joint 3p + i), built ONCE per kernel from constexpr
// locals.  Written this way on purpose: `p ? table[3 + i] : table[i]` makes LLVM fold the select
// into a dynamically indexed load from the constant array — a global load plus s_waitcnt vmcnt(0)
// (which also waits for every outstanding store) in the middle of the hot loop.
struct LaneConsts {
    float lim[kJpl];   // r_hi (= -r_lo)
    float lc[kJpl];    // cos(r_hi)
    float ls[kJpl];    // sin(r_hi)
};

__device__ __forceinline__ LaneConsts lane_consts(int p)
{
    constexpr float l0 = limit_hi(0), l1 = limit_hi(1), l2 = limit_hi(2), l3 = limit_hi(3), l4 = limit_hi(4), l5 = limit_hi(5);
    constexpr float c0 = kLimitCos[0], c1 = kLimitCos[1], c2 = kLimitCos[2], c3 = kLimitCos[3], c4 = kLimitCos[4], c5 = kLimitCos[5];
    constexpr float s0 = kLimitSin[0], s1 = kLimitSin[1], s2 = kLimitSin[2], s3 = kLimitSin[3], s4 = kLimitSin[4], s5 = kLimitSin[5];
    static_assert(kJpl == 3, "lane_consts is written for three joints per lane");
    LaneConsts k;
    k.lim[0] = p ? l3 : l0; k.lim[1] = p ? l4 : l1; k.lim[2] = p ? l5 : l2;
    k.lc[0] = p ? c3 : c0;  k.lc[1] = p ? c4 : c1;  k.lc[2] = p ? c5 : c2;
    k.ls[0] = p ? s3 : s0;  k.ls[1] = p ? s4 : s1;  k.ls[2] = p ? s5 : s2;
    return k;
}

// ---- sin/cos -------------------------------------------------------------------------
// np.sin / np.cos of the float32 observation pieces (pioneer_knm_env.py:195-203).
// Cody-Waite reduction by pi/2 with three float32 constants and FMA, then
// degree-7/8 minimax polynomials on [-pi/4, pi/4]; max abs error 9.3e-8 for
// |x| <= 2^16 (tests/test_gpu_sincos.py sweeps it against float64).  Every trig
// argument of the obs except the raw action is bounded by construction
// (|r| <= pi, |r - r_lo| <= 2 pi, |v| <= v_max); ~22 VALU ops per pair instead
// of ocml's sincosf with its inlined Payne-Hanek path.
__device__ __forceinline__ void sincos_bounded(float x, float& sn, float& cs)
{
    const float k = __builtin_rintf(x * 0x1.45f306p-1f);                 // x * 2/pi
    float r = __builtin_fmaf(-k, 0x1.921fb6p+0f, x);                     // pi/2 hi
    r = __builtin_fmaf(-k, -0x1.777a5cp-25f, r);                         // pi/2 mid
    r = __builtin_fmaf(-k, -0x1.ee59dap-50f, r);                         // pi/2 lo
    const float z = r * r;
    float ps = __builtin_fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f);
    ps = __builtin_fmaf(z, ps, -1.6666654611e-1f);
    const float s0 = __builtin_fmaf(r * z, ps, r);
    float pc = __builtin_fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f);
    pc = __builtin_fmaf(z, pc, 4.166664568298827e-2f);
    const float c0 = __builtin_fmaf(z * z, pc, __builtin_fmaf(z, -0.5f, 1.0f));
    const int q = (int)k;
    const float ss = (q & 1) ? c0 : s0;
    const float cc = (q & 1) ? s0 : c0;
    sn = (q & 2) ? -ss : ss;
    cs = ((q + 1) & 2) ? -cc : cc;
}

// The raw action is not bounded by the env (RLlib clips it, the env does not):
// beyond 2^17 fall back to ocml's fully-reduced sincosf.
__device__ __forceinline__ void sincos_any(float x, float& sn, float& cs)
{
    if (__builtin_fabsf(x) <= 131072.0f) sincos_bounded(x, sn, cs);
    else sincosf(x, &sn, &cs);
}

// ---- integrator: pioneer_knm_env.py:113-146 -------------------------------------
// One joint.  Cast sequence = the reference's NumPy 1.x arithmetic (float32
// stores, float64 intermediates); bit-exact against oracle/pnr_oracle.c.
// The arithmetic is stated once, in three pieces, and put together twice: integrate_joint branches round the saturation
// piece per joint; integrate_joints3 (step_kernel) runs the pieces of a lane's three joints side by side.
struct JointStep {
    float v1;                  // the new velocity, before the position limits
    bool hi, lo;               // it left [-vmax, vmax]
    double dt_p1, dt_p2;       // the step's two parts: up to the saturation, and at vsat
};

__device__ __forceinline__ JointStep joint_predict(float a0, float v0, float vmax, double dt)
{
    JointStep j;
    j.v1 = (float)((double)v0 + (double)a0 * dt);                // :121
    j.dt_p1 = dt; j.dt_p2 = 0.0;                                 // :122-123
    j.hi = j.v1 > vmax; j.lo = j.v1 < -vmax;                     // :125, :129
    return j;
}

// the time at which the velocity reaches its bound; meaningful where j.hi || j.lo (elsewhere a number nobody uses)
__device__ __forceinline__ double joint_sat_time(const JointStep& j, float a0, float v0, float vmax, double eps)
{
    const float vsat = j.hi ? vmax : -vmax;
    const float num = vsat - v0;                                 // float32 - float32
    return (double)num / ((double)a0 + eps);                     // :126, :130 (eps added, not sign-matched)
}

// `sat`: this joint saturates (the literal true under integrate_joint's branch, a select per value in integrate_joints3)
__device__ __forceinline__ void joint_saturate(JointStep& j, bool sat, double q, float vmax, double dt)
{
    // np.clip(q, 0, dt), NaN-propagating: q != q ? q : (q < 0 ? 0 : (q > dt ? dt : q)), as two flat selects (both compares are false
    // for a NaN, which so passes through; nested, the three tests came out as three levels of exec-mask regions per joint)
    const double qc = q > dt ? dt : q;
    q = q < 0.0 ? 0.0 : qc;
    j.dt_p1 = sat ? q : dt;
    j.dt_p2 = sat ? dt - q : 0.0;                                // :127, :131
    j.v1 = sat ? (j.hi ? vmax : -vmax) : j.v1;                   // :128, :132
}

__device__ __forceinline__ void joint_finish(const JointStep& j, float v0, float r0, float rlo, float rhi, float& v_out, float& r_out)
{
    float v1 = j.v1;
    const float vs = v0 + v1;                                    // float32 + float32
    const double half = 0.5 * (double)vs;
    const double r1d = ((double)r0 + half * j.dt_p1) + (double)v1 * j.dt_p2;  // :134
    float r1 = (float)r1d;
    if (r1 >= rhi) { r1 = rhi; v1 = 0.0f; }                      // :135-137
    if (r1 <= rlo) { r1 = rlo; v1 = 0.0f; }                      // :139-141
    v_out = v1;
    r_out = r1;
}

__device__ __forceinline__ void integrate_joint(float a0, float v0, float r0, float vmax, float rlo, float rhi,
                                                double dt, double eps, float& v_out, float& r_out)
{
    JointStep j = joint_predict(a0, v0, vmax, dt);
    if (j.hi || j.lo) joint_saturate(j, true, joint_sat_time(j, a0, v0, vmax, eps), vmax, dt);
    joint_finish(j, v0, r0, rlo, rhi, v_out, r_out);
}

// A lane's three joints (limits -lim[i], lim[i]) side by side: ONE branch on "some joint of this lane saturates" — a wave in which
// nothing does skips the block — and under it the three quotients in one basic block, so that their strictly dependent f64
// division chains (v_div_scale, v_rcp_f64, four FMAs, ..) interleave, with the clip and the choice per joint as selects.  The
// values are integrate_joint's: a joint that does not saturate computes a quotient and drops it (no floating-point traps here).
// The empty asm holds the block together: with plain selects LLVM sinks each division back under a branch of its own
// (a select whose operand is a division becomes a branch), three chains one after the other again.
__device__ __forceinline__ void integrate_joints3(const float (&a0)[kJpl], float (&v)[kJpl], float (&r)[kJpl], const float (&vmax)[kJpl],
                                                  const float (&lim)[kJpl], double dt, double eps)
{
    static_assert(kJpl == 3, "integrate_joints3 is written for three joints per lane");
    JointStep j[kJpl] = {joint_predict(a0[0], v[0], vmax[0], dt), joint_predict(a0[1], v[1], vmax[1], dt),
                         joint_predict(a0[2], v[2], vmax[2], dt)};
    if ((j[0].hi || j[0].lo) || (j[1].hi || j[1].lo) || (j[2].hi || j[2].lo)) {
        double q0 = joint_sat_time(j[0], a0[0], v[0], vmax[0], eps), q1 = joint_sat_time(j[1], a0[1], v[1], vmax[1], eps),
               q2 = joint_sat_time(j[2], a0[2], v[2], vmax[2], eps);
        asm volatile("" : "+v"(q0), "+v"(q1), "+v"(q2));
        joint_saturate(j[0], j[0].hi || j[0].lo, q0, vmax[0], dt);
        joint_saturate(j[1], j[1].hi || j[1].lo, q1, vmax[1], dt);
        joint_saturate(j[2], j[2].hi || j[2].lo, q2, vmax[2], dt);
    }
#pragma unroll
    for (int i = 0; i < kJpl; ++i) joint_finish(j[i], v[i], r[i], -lim[i], lim[i], v[i], r[i]);
}

// ---- forward kinematics of robot:pointer ---------------------------------------
// Replaces Item.pose() -> getLinkState(computeForwardKinematics=1)
// (bullet_scene.py:53-59) for the serial chain of pnr_model.h; unrolled over the
// constexpr joint table from the tip to the base.
__device__ __forceinline__ void fk_pointer(const float (&c)[kDof], const float (&s)[kDof], float (&p)[3])
{
    float x = (float)kTipX, y = (float)kTipY, z = (float)kTipZ;
#pragma unroll
    for (int j = kDof - 1; j >= 0; --j) {
        const float cj = c[j], sj = s[j];
        if (kJoints[j].axis == AX) {
            const float ny = __builtin_fmaf(cj, y, -(sj * z));
            const float nz = __builtin_fmaf(sj, y, cj * z);
            y = ny; z = nz;
        } else if (kJoints[j].axis == AY) {
            const float nx = __builtin_fmaf(cj, x, sj * z);
            const float nz = __builtin_fmaf(cj, z, -(sj * x));
            x = nx; z = nz;
        } else {
            const float nx = __builtin_fmaf(cj, x, -(sj * y));
            const float ny = __builtin_fmaf(sj, x, cj * y);
            x = nx; y = ny;
        }
        if (kJoints[j].ox != 0.0) x += (float)kJoints[j].ox;
        if (kJoints[j].oy != 0.0) y += (float)kJoints[j].oy;
        if (kJoints[j].oz != 0.0) z += (float)kJoints[j].oz;
    }
    p[0] = x; p[1] = y; p[2] = z;
}

// ---- Philox4x32-10 (Salmon et al. SC'11) ----------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t (&out)[4])
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ double u01(uint32_t x) { return (double)(x >> 8) * (1.0 / 16777216.0); }

// ---- reset: reset_world, pioneer_knm_env.py:76-105 --------------------------------
// Draws r ~ U(r_lo, r_hi), target ~ U(target_lo, target_hi) from
// Philox(key = seed, counter = (episode, global env id, block)): words 0..5 are
// the joints, 6..8 the target; a = v = 0; potential = 0 (quirk Q3);
// step_index = 0.  jp / tp (this ENV's rows) override the draws, as
// reset_world's joint_positions / target_position arguments do.  Both lanes of
// a pair run this and keep their own three joints.
__device__ __forceinline__ void reset_env(const KParams& P, const LaneConsts& K, LaneState& s, int p,
                                          unsigned long long genv, const float* jp, const float* tp)
{
    uint32_t w[12];
#pragma unroll
    for (uint32_t b = 0; b < 3; ++b) {
        uint32_t o[4];
        philox4x32_10(s.episode, (uint32_t)genv, (uint32_t)(genv >> 32), b, P.seed_lo, P.seed_hi, o);
        w[4 * b + 0] = o[0]; w[4 * b + 1] = o[1]; w[4 * b + 2] = o[2]; w[4 * b + 3] = o[3];
    }
#pragma unroll
    for (int i = 0; i < kJpl; ++i) {
        const double hi = (double)K.lim[i], lo = -hi;
        const uint32_t word = p ? w[kJpl + i] : w[i];
        const float drawn = (float)(lo + (hi - lo) * u01(word));             // :80-81
        s.r[i] = jp ? jp[kJpl * p + i] : drawn;                              // :94 (stored as float32)
        s.a[i] = 0.0f;                                                       // :92
        s.v[i] = 0.0f;                                                       // :93
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float drawn = (float)(P.tlo[k] + P.tspan[k] * u01(w[6 + k])); // :83-90
        s.tgt[k] = tp ? tp[k] : drawn;
    }
    s.pot = 0.0f;                                                            // :105
    s.step = 0;                                                              // bullet_env.py:99
    s.episode += 1;
}

// ---- pose-dependent quantities -----------------------------------------------------
struct Pose {
    float c[kJpl], s[kJpl];  // cos r, sin r of this lane's joints
    float ptr[3];            // pointer xyz
    float diff[3];
    float dist;
};

__device__ __forceinline__ void compute_pose(const LaneState& s, int p, Pose& q)
{
    float c6[kDof], s6[kDof];
#pragma unroll
    for (int i = 0; i < kJpl; ++i) {
        sincos_bounded(s.r[i], q.s[i], q.c[i]);
        const float oc = xchg(q.c[i]), os = xchg(q.s[i]);
        c6[i] = p ? oc : q.c[i];        s6[i] = p ? os : q.s[i];
        c6[kJpl + i] = p ? q.c[i] : oc; s6[kJpl + i] = p ? q.s[i] : os;
    }
    fk_pointer(c6, s6, q.ptr);
#pragma unroll
    for (int k = 0; k < 3; ++k) q.diff[k] = s.tgt[k] - q.ptr[k];          // :154
    q.dist = sqrtf(__builtin_fmaf(q.diff[2], q.diff[2],
                   __builtin_fmaf(q.diff[1], q.diff[1], q.diff[0] * q.diff[0])));  // :155
}

// ---- `done`, bit for bit: pioneer_knm_env.py:154-160 ------------------------------------
// `done = distance < done_distance` is a byte the caller branches on (episode end, +award_done, reset), so it is held to
// the integer bar: the reference forms it from Bullet's float64 link position and Python floats.  The float32 pose above is
// good to 3e-5; whenever its distance lies within kDoneBand of the threshold, the lanes concerned re-evaluate the forward
// kinematics and the distance in float64 from (double)r — the operation order of the float64 restatement
// (oracle/pnr_oracle.c orc_fk_pointer / orc_reward), no fused multiply-adds — and take the predicate from that.  The branch
// is rare (a pointer crosses the threshold at ~1 unit per step, the band is 2e-3 wide), pair-uniform (both lanes of an env
// hold the same float32 distance, so the DPP exchange below finds its partner live), and costs the common path one
// compare.
#ifndef PNR_DONE_BAND
#define PNR_DONE_BAND 1.0e-3f          // -DPNR_DONE_BAND=0.0f folds the branch away (the float32 predicate of rounds 1-4: A/B only)
#endif
constexpr float kDoneBand = PNR_DONE_BAND;

// The float64 constants of this rare path live in a table and are fetched into VECTOR registers by the lanes that need them
// (the index is made opaque, so the loads are vector loads inside the branch): as literals they would be 40 scalar
// registers materialised next to a kernel that already runs at the scalar-register limit, and the spills that makes room
// for them land on the common path (+112 instructions per step, +3.7 % on step_kernel at 65 536 envs, A/B r05).
constexpr double kPio2Inv = 6.36619772367581382433e-01, kPio2Hi = 1.57079632673412561417e+00, kPio2Lo = 6.07710050650619224932e-11;
__device__ const double kDoneTable[15 + 3 + 3 * kDof] = {
    kPio2Inv, kPio2Hi, kPio2Lo,
    // sin kernel, highest power first (Sun fdlibm __kernel_sin S6..S1), then cos kernel (C6..C1)
    1.58969099521155010221e-10, -2.50507602534068634195e-08, 2.75573137070700676789e-06,
    -1.98412698298579493134e-04, 8.33333333332248946124e-03, -1.66666666666666324348e-01,
    -1.13596475577881948265e-11, 2.08757232129817482790e-09, -2.75573143513906633035e-07,
    2.48015872894767294178e-05, -1.38888888888741095749e-03, 4.16666666666666019037e-02,
    kTipX, kTipY, kTipZ,
    kJoints[0].ox, kJoints[0].oy, kJoints[0].oz, kJoints[1].ox, kJoints[1].oy, kJoints[1].oz,
    kJoints[2].ox, kJoints[2].oy, kJoints[2].oz, kJoints[3].ox, kJoints[3].oy, kJoints[3].oz,
    kJoints[4].ox, kJoints[4].oy, kJoints[4].oz, kJoints[5].ox, kJoints[5].oy, kJoints[5].oz,
};

// sin / cos of a float64 argument bounded by the joint limits (|x| <= 2 pi here; accurate to < 1 ulp for |x| < 2^20):
// Cody-Waite reduction by pi/2 in two pieces (k * hi is exact: hi carries 33 bits), then the classic degree-13 / 14
// minimax kernels on [-pi/4, pi/4].  T = the table above.
__device__ __forceinline__ void sincos_f64(const double* __restrict__ T, double x, double& sn, double& cs)
{
    const double k = __builtin_rint(x * T[0]);
    double r = __builtin_fma(-k, T[1], x);
    r = __builtin_fma(-k, T[2], r);
    const double z = r * r;
    double ps = __builtin_fma(z, T[3], T[4]);
    ps = __builtin_fma(z, ps, T[5]);
    ps = __builtin_fma(z, ps, T[6]);
    ps = __builtin_fma(z, ps, T[7]);
    ps = __builtin_fma(z, ps, T[8]);
    const double s0 = __builtin_fma(r * z, ps, r);
    double pc = __builtin_fma(z, T[9], T[10]);
    pc = __builtin_fma(z, pc, T[11]);
    pc = __builtin_fma(z, pc, T[12]);
    pc = __builtin_fma(z, pc, T[13]);
    pc = __builtin_fma(z, pc, T[14]);
    const double c0 = __builtin_fma(z * z, pc, __builtin_fma(z, -0.5, 1.0));
    const int q = (int)k;
    const double ss = (q & 1) ? c0 : s0;
    const double cc = (q & 1) ? s0 : c0;
    sn = (q & 2) ? -ss : ss;
    cs = ((q + 1) & 2) ? -cc : cc;
}

// orc_fk_pointer's arithmetic: plain float64 multiplies and adds from the tip to the base, over the constexpr joint table
// (which offsets exist is decided at compile time; their values come from the table)
__device__ __forceinline__ void fk_pointer_f64(const double* __restrict__ T, const double (&c)[kDof], const double (&s)[kDof], double (&p)[3])
{
    double x = T[15], y = T[16], z = T[17];
#pragma unroll
    for (int j = kDof - 1; j >= 0; --j) {
        const double cj = c[j], sj = s[j];
        if (kJoints[j].axis == AX) {
            const double ny = cj * y - sj * z, nz = sj * y + cj * z;
            y = ny; z = nz;
        } else if (kJoints[j].axis == AY) {
            const double nx = cj * x + sj * z, nz = -sj * x + cj * z;
            x = nx; z = nz;
        } else {
            const double nx = cj * x - sj * y, ny = sj * x + cj * y;
            x = nx; y = ny;
        }
        if (kJoints[j].ox != 0.0) x += T[18 + 3 * j];
        if (kJoints[j].oy != 0.0) y += T[19 + 3 * j];
        if (kJoints[j].oz != 0.0) z += T[20 + 3 * j];
    }
    p[0] = x; p[1] = y; p[2] = z;
}

// `s` holds this lane's three joints (r) and the env's target; `dist` is the pair's float32 distance.
__device__ __forceinline__ bool done_predicate(const LaneState& s, int p, float dist, float done_dist, double done_dist_d)
{
    bool done = dist < done_dist;
    if (__builtin_fabsf(dist - done_dist) < kDoneBand) {
        int zero;
        asm volatile("v_mov_b32 %0, 0" : "=v"(zero));      // opaque, per-lane: the table is read with vector loads, here
        const double* __restrict__ T = kDoneTable + zero;
        double c6[kDof], s6[kDof];
#pragma unroll
        for (int i = 0; i < kJpl; ++i) {
            const float mine = s.r[i], other = xchg(mine);
            sincos_f64(T, (double)(p ? other : mine), s6[i], c6[i]);
            sincos_f64(T, (double)(p ? mine : other), s6[kJpl + i], c6[kJpl + i]);
        }
        double ptr[3];
        fk_pointer_f64(T, c6, s6, ptr);
        const double d0 = (double)s.tgt[0] - ptr[0], d1 = (double)s.tgt[1] - ptr[1], d2 = (double)s.tgt[2] - ptr[2];
        done = __builtin_sqrt(d0 * d0 + d1 * d1 + d2 * d2) < done_dist_d;
    }
    return done;
}

// ---- observation: observe(), pioneer_knm_env.py:184-211 -----------------------------
// Sink::putj(f, v) writes per-joint feature f of this lane's joint column (the
// sink adds 3p); Sink::putt(f0, f1, v) writes tail feature f0 (lane 0) or f1
// (lane 1).  Tail pieces (126..136): lane 0 writes pointer + target, lane 1
// diff + distance + potential.
// [18:54]: r_lo, cos r_lo, sin r_lo, r_hi, cos r_hi, sin r_hi — the same 36 numbers for every env
// and every step.  With an LDS-tile sink they are written ONCE per kernel (the tile slots are never
// overwritten by anything else), at kernel start while the state loads are in flight.
template <class Sink>
__device__ __forceinline__ void emit_obs_const(const LaneConsts& K, Sink& out)
{
#pragma unroll
    for (int i = 0; i < kJpl; ++i) {
        const float lim = K.lim[i], lc = K.lc[i], ls = K.ls[i];
        out.putj(18 + i, -lim); out.putj(24 + i, lc); out.putj(30 + i, -ls);
        out.putj(36 + i, lim);  out.putj(42 + i, lc); out.putj(48 + i, ls);
    }
}

template <bool WITH_CONST = true, class Sink>
__device__ __forceinline__ void emit_obs(const LaneConsts& K, const LaneState& s, const Pose& q, int p, Sink& out)
{
    if (WITH_CONST) emit_obs_const(K, out);
#pragma unroll
    for (int i = 0; i < kJpl; ++i) {
        float sn, cs;
        const float lim = K.lim[i];
        // [0:18]  r, cos r, sin r
        out.putj(0 + i, s.r[i]); out.putj(6 + i, q.c[i]); out.putj(12 + i, q.s[i]);
        // [54:72] r - r_lo (float32 subtraction, :191)
        const float dlo = s.r[i] - (-lim);
        sincos_bounded(dlo, sn, cs);
        out.putj(54 + i, dlo); out.putj(60 + i, cs); out.putj(66 + i, sn);
        // [72:90] r_hi - r (:192)
        const float dhi = lim - s.r[i];
        sincos_bounded(dhi, sn, cs);
        out.putj(72 + i, dhi); out.putj(78 + i, cs); out.putj(84 + i, sn);
        // [90:108] v
        sincos_bounded(s.v[i], sn, cs);
        out.putj(90 + i, s.v[i]); out.putj(96 + i, cs); out.putj(102 + i, sn);
        // [108:126] a (the action just given, quirk Q1)
        sincos_any(s.a[i], sn, cs);
        out.putj(108 + i, s.a[i]); out.putj(114 + i, cs); out.putj(120 + i, sn);
    }
    // [126:137] p = 0: pointer xyz (126..128), target xyz (129..131)
    //           p = 1: diff (132..134), distance (135), potential (136)
#pragma unroll
    for (int k = 0; k < 3; ++k) out.putt(126 + k, 132 + k, p ? q.diff[k] : q.ptr[k]);
    out.putt(129, 135, p ? q.dist : s.tgt[0]);
    out.putt(130, 136, p ? s.pot : s.tgt[1]);
    out.putt0(131, s.tgt[2]);
}

// Sinks -------------------------------------------------------------------------
// env-major through an LDS tile [32][137]: the row stride of 137 dwords is odd, so
// a pair-interleaved ds_write_b32 is at worst 2-way conflicted (free for writes)
struct SinkLdsTile {
    float* row;    // tile + env_local * 137
    int jo;        // 3p
    int p;
    __device__ __forceinline__ void putj(int f, float v) { row[f + jo] = v; }
    __device__ __forceinline__ void putt(int f0, int f1, float v) { row[p ? f1 : f0] = v; }
    __device__ __forceinline__ void putt0(int f0, float v) { if (!p) row[f0] = v; }
};
// feature-major through an LDS tile [137][32]
struct SinkLdsFeatureTile {
    float* col;    // tile + env_local
    int jo;
    int p;
    __device__ __forceinline__ void putj(int f, float v) { col[(f + jo) * kEnvsPerWave] = v; }
    __device__ __forceinline__ void putt(int f0, int f1, float v) { col[(p ? f1 : f0) * kEnvsPerWave] = v; }
    __device__ __forceinline__ void putt0(int f0, float v) { if (!p) col[f0 * kEnvsPerWave] = v; }
};
// direct global stores with an element stride (masked reset only: rows / columns
// of other envs must stay untouched); stride 1 = env-major row, n = feature-major
struct SinkDirect {
    float* base; long long stride; int jo; int p; bool on;
    __device__ __forceinline__ void putj(int f, float v) { if (on) base[(long long)(f + jo) * stride] = v; }
    __device__ __forceinline__ void putt(int f0, int f1, float v) { if (on) base[(long long)(p ? f1 : f0) * stride] = v; }
    __device__ __forceinline__ void putt0(int f0, float v) { if (on && !p) base[(long long)f0 * stride] = v; }
};

// Streaming outputs (observations, rewards, flags) are written once and read by another kernel much
// later: non-temporal stores keep them from displacing the state planes in L2 and were worth 8 % at
// 65 536 envs and 31 % at 1 M envs per launch (178 -> 122 us).
typedef float v4f_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void stream_store(float4* dst, const float4& v)
{
    v4f_t x = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(x, reinterpret_cast<v4f_t*>(dst));
}
__device__ __forceinline__ void stream_store(float* dst, float v) { __builtin_nontemporal_store(v, dst); }
__device__ __forceinline__ void stream_store(uint8_t* dst, uint8_t v) { __builtin_nontemporal_store(v, dst); }

// Copy a wave's LDS tile (rows [0, nvalid) of 137 floats) to its contiguous
// place in an env-major obs batch with 16-byte lane-linear stores.
__device__ __forceinline__ void flush_tile(const float* __restrict__ lds, float* __restrict__ dst,
                                           int nvalid, int lane)
{
    const int total = nvalid * kObsDim;
    if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        const int nvec = total >> 2;
        const float4* src4 = reinterpret_cast<const float4*>(lds);
        float4* dst4 = reinterpret_cast<float4*>(dst);
        for (int j = lane; j < nvec; j += kWave) stream_store(dst4 + j, src4[j]);
        for (int j = (nvec << 2) + lane; j < total; j += kWave) stream_store(dst + j, lds[j]);
    } else {
        for (int j = lane; j < total; j += kWave) stream_store(dst + j, lds[j]);
    }
}

// Flush a [137][32] feature tile to obs[f*n + tile0 + 0..31]: 8 lanes x 16 B cover
// one feature's 32 envs (128 B), a wave instruction covers eight features.
__device__ __forceinline__ void flush_feature_tile(const float* __restrict__ lds, float* __restrict__ dst,
                                                   long long n, int nvalid, int lane)
{
    if (nvalid == kEnvsPerWave && ((reinterpret_cast<uintptr_t>(dst) | (uintptr_t)(n * 4)) & 15u) == 0) {
        const int sub = lane >> 3, col4 = (lane & 7) * 4;
        for (int f0 = 0; f0 < kObsDim; f0 += 8) {
            const int f = f0 + sub;
            if (f < kObsDim) {
                const float4 v = *reinterpret_cast<const float4*>(lds + f * kEnvsPerWave + col4);
                stream_store(reinterpret_cast<float4*>(dst + (long long)f * n + col4), v);
            }
        }
    } else {
        const int col = lane & (kEnvsPerWave - 1), half = lane >> 5;
        for (int f = half; f < kObsDim; f += 2)
            if (col < nvalid) stream_store(dst + (long long)f * n + col, lds[f * kEnvsPerWave + col]);
    }
}

// ---- the one obs path of the tile kernels: this lane's entries into its wave's LDS tile, then the tile out as whole lines ----
template <bool OBS_EM>
__device__ __forceinline__ std::conditional_t<OBS_EM, SinkLdsTile, SinkLdsFeatureTile> tile_sink(float* tile, int el, int p)
{
    return {tile + el * (OBS_EM ? kObsDim : 1), kJpl * p, p};
}

// the 36 constant entries of this lane's tile slots
template <bool OBS_EM>
__device__ __forceinline__ void obs_tile_const(const LaneConsts& K, float* tile, int el, int p)
{
    auto sink = tile_sink<OBS_EM>(tile, el, p);
    emit_obs_const(K, sink);
}

// emit, sync, flush.  obs: the batch this tile's 32 envs (first env tile0, nvalid of them live) go to, [n][137] or [137][n].
// emit / flush = false: the timing-only ablations of a -DPNR_DIAG_BUILD=1 variant (literal true in the product library).
template <bool OBS_EM, bool WITH_CONST = false>
__device__ __forceinline__ void obs_tile_out(const LaneConsts& K, const LaneState& s, const Pose& q, float* tile, int el, int p, int lane,
                                             float* obs, long long tile0, long long n, int nvalid, bool emit = true, bool flush = true)
{
    auto sink = tile_sink<OBS_EM>(tile, el, p);
    if (emit) emit_obs<WITH_CONST>(K, s, q, p, sink);
    wave_lds_sync();
    if (!flush) return;
    if (OBS_EM) flush_tile(tile, obs + tile0 * kObsDim, nvalid, lane);
    else flush_feature_tile(tile, obs + tile0, n, nvalid, lane);
}

// ---- the one-pass step_kernel's obs path for the env-major tile: the linear entries first, then the trig in ROW order with the flush under it ----
// obs_tile_out finishes all 32 rows at once — every lane evaluates the twelve sin / cos pairs of its own half row before any
// lane has a complete row — so no obs store leaves before the last of them.  Here a lane writes in phase 1 only what needs no new
// trig: r, cos r, sin r, the tail, and the ARGUMENTS dlo, dhi, v, a (the floats emit_obs forms) in their own columns 54.., 72..,
// 90.., 108...  Phase 2 takes the tile's 32 x 24 arguments as one flat list j = 64 it + lane (row j / 24, argument j % 24, cos
// to column + 6, sin to column + 12), twelve unrolled iterations: after iteration `it` the rows below 64 (it + 1) / 24 are
// complete, and every 1-KiB chunk of the tile inside them goes out right then, the rest of the trig running under the stores.
// Each argument goes through the function emit_obs gives it (sincos_bounded; sincos_any for a): the same bits.
constexpr int kTrigArgs = 4 * kDof;                                  // per row: dlo, dhi, v, a of six joints
constexpr int kTrigIters = kEnvsPerWave * kTrigArgs / kWave;         // 12
constexpr int kChunkFloats = 4 * kWave;                              // one wave-wide dwordx4 store
// (row, argument) of iteration it + 3 is that of iteration it, eight rows on: three tile offsets per lane, the rest immediates
constexpr int kTrigPeriod = 3, kTrigPeriodRows = kTrigPeriod * kWave / kTrigArgs;
static_assert(kEnvsPerWave * kTrigArgs == kTrigIters * kWave && kTrigPeriod * kWave == kTrigPeriodRows * kTrigArgs &&
              kTrigIters % kTrigPeriod == 0, "the row pass is written for 32 rows of 24 arguments on 64 lanes");

// whole chunks inside the rows that are complete after `iters` iterations
constexpr int row_pass_chunks(int iters) { return (kWave * iters / kTrigArgs) * kObsDim / kChunkFloats; }

// where this lane's arguments sit
struct RowPassLane {
    int off[kTrigPeriod];      // tile offset of the argument of iterations 0, 1, 2
    bool is_a[kTrigPeriod];    // .. and whether it is an action (sincos_any)
    int tail;                  // phase 1: tile offset of this lane's first tail entry (column 126, or 132 for the pair's second lane)
};

// Nothing here depends on a loaded value: step_kernel forms it in the head of the launch, under the latency of the first loads
// (the `/ 24` arithmetic and the tail columns were ~55 instructions between the state stores and the first obs store).
__device__ __forceinline__ RowPassLane row_pass_lane(int lane)
{
    RowPassLane L;
    L.tail = (lane >> 1) * kObsDim + 126 + 6 * (lane & 1);
#pragma unroll
    for (int k = 0; k < kTrigPeriod; ++k) {
        const int j = kWave * k + lane, row = j / kTrigArgs, arg = j - kTrigArgs * row, grp = arg / kDof;
        L.off[k] = row * kObsDim + 54 + arg + 2 * kDof * grp;             // column 54 + 18 grp + joint
        L.is_a[k] = grp == 3;
    }
    return L;
}

// dst: the tile's place in the batch, obs + tile0 * 137.  emit / flush as in obs_tile_out: no emit skips both phases.
// L: row_pass_lane(lane), formed by the caller ahead of time.
__device__ __forceinline__ void obs_tile_rows_out(const LaneConsts& K, const LaneState& s, const Pose& q, const RowPassLane& L, float* tile,
                                                  int el, int p, int lane, float* __restrict__ dst, int nvalid, bool emit = true,
                                                  bool flush = true)
{
    // -- phase 1: this lane's half row, everything but the new sin / cos
    if (emit) {
        SinkLdsTile out = tile_sink<true>(tile, el, p);
#pragma unroll
        for (int i = 0; i < kJpl; ++i) {
            const float lim = K.lim[i];
            out.putj(0 + i, s.r[i]); out.putj(6 + i, q.c[i]); out.putj(12 + i, q.s[i]);
            out.putj(54 + i, s.r[i] - (-lim));                            // float32 subtractions, :191-192
            out.putj(72 + i, lim - s.r[i]);
            out.putj(90 + i, s.v[i]);
            out.putj(108 + i, s.a[i]);
        }
        // the tail as emit_obs writes it (putt: columns 126.. for the pair's first lane, 132.. for its second), from one offset
        float* tl = tile + L.tail;
#pragma unroll
        for (int k = 0; k < 3; ++k) tl[k] = p ? q.diff[k] : q.ptr[k];
        tl[3] = p ? q.dist : s.tgt[0];
        tl[4] = p ? s.pot : s.tgt[1];
        if (!p) tl[5] = s.tgt[2];
    }
    wave_lds_sync();

    // -- phase 2: the arguments of all twelve iterations leave LDS first (their columns are not written below)
    float x[kTrigIters];
    if (emit) {
#pragma unroll
        for (int it = 0; it < kTrigIters; ++it) x[it] = tile[L.off[it % kTrigPeriod] + (it / kTrigPeriod) * kTrigPeriodRows * kObsDim];
    }
    const int total = nvalid * kObsDim;
    const bool vec = (reinterpret_cast<uintptr_t>(dst) & 15u) == 0;
    const int nchunk = (flush && vec) ? total / kChunkFloats : 0;        // wave-uniform; <= row_pass_chunks(kTrigIters)
    const float4* src4 = reinterpret_cast<const float4*>(tile);
    float4* dst4 = reinterpret_cast<float4*>(dst);
#pragma unroll
    for (int it = 0; it < kTrigIters; ++it) {
        if (emit) {
            float* o = tile + L.off[it % kTrigPeriod] + (it / kTrigPeriod) * kTrigPeriodRows * kObsDim;
            float sn, cs;
            const bool far = L.is_a[it % kTrigPeriod] & !(__builtin_fabsf(x[it]) <= 131072.0f);
            if (far) sincosf(x[it], &sn, &cs);                           // sincos_any's rare branch
            else sincos_bounded(x[it], sn, cs);
            o[kDof] = cs; o[2 * kDof] = sn;
        }
        wave_lds_sync();
#pragma unroll
        for (int c = row_pass_chunks(it); c < row_pass_chunks(it + 1); ++c)
            if (c < nchunk) stream_store(dst4 + c * kWave + lane, src4[c * kWave + lane]);
    }
    if (!flush) return;
    // the ragged end behind the last whole chunk; an unaligned destination goes out as single floats
    if (vec) {
        const int nvec = total >> 2;
        for (int j = nchunk * kWave + lane; j < nvec; j += kWave) stream_store(dst4 + j, src4[j]);
        for (int j = (nvec << 2) + lane; j < total; j += kWave) stream_store(dst + j, tile[j]);
    } else {
        for (int j = lane; j < total; j += kWave) stream_store(dst + j, tile[j]);
    }
}

// step_kernel's choice.  The row pass pays where all waves of a launch reach the emit together, HBM idles until the first store and
// the launch is long enough to be bound by its stores: the one-pass form at more than one wave per SIMD (9.87 -> 9.40 us at 65 536
// envs, 8.10 -> 7.89 at 49 152; same-box A/B).  Elsewhere it only lengthens a wave's own chain (twelve LDS round trips, ~170 more
// instructions): one wave per SIMD and fewer (5.5 -> 6.4 us at 16 384 envs, 5.1 -> 6.1 at 8 192; equal at 32 768), and the persistent
// general form, whose waves are out of phase and feed the store stream anyway (pnr_rollout 6.24 -> 7.37 us per step, 262 144 envs
// 31.2 -> 32.3 us).  Those keep obs_tile_out.
template <bool OBS_EM, bool ROW_PASS>
__device__ __forceinline__ void step_obs_out(const LaneConsts& K, const LaneState& s, const Pose& q, const RowPassLane& L, float* tile, int el,
                                             int p, int lane, float* obs, long long tile0, long long n, int nvalid, bool emit, bool flush)
{
    static_assert(OBS_EM || !ROW_PASS, "the row pass is written for the env-major tile");
    if constexpr (ROW_PASS) obs_tile_rows_out(K, s, q, L, tile, el, p, lane, obs + tile0 * kObsDim, nvalid, emit, flush);
    else obs_tile_out<OBS_EM>(K, s, q, tile, el, p, lane, obs, tile0, n, nvalid, emit, flush);
}

}  // namespace pnr
