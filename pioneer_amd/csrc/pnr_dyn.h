// pnr_dyn.h — dynamics mode: articulated-body forward dynamics (Featherstone ABA)
// + PD joint torques + joint limits + pointer/ground penalty contact, frame_skip
// sub-steps per env-step (World.step of the reference, bullet_scene.py:273-275,
// is where Bullet would do this; under the reference's defaults it is a no-op,
// SURVEY.md a6).  PARITY UNPINNED: checked against oracle/pnr_dyn_oracle.c.
//
// One env per lane (the recursion over the chain is serial), float32, everything
// in registers.  The chain is the constexpr table of pnr_model.h: every joint
// axis is a coordinate axis, so S_i is a unit vector (U_i is a column of the
// articulated inertia, D_i a diagonal element) and every Pluecker transform is a
// Givens rotation plus a constexpr translation; the unrolled code drops the terms
// that vanish for this arm.  VALU-bound (~1.3 k FMA per ABA, 10 per env-step);
// no MFMA: per-lane 6x6 recursions with data-dependent pivots, not a contraction.
//
// State: planar float32 words [36][n] (the canonical pnr_get_dyn_state layout):
//   0-5 q, 6-11 qd, 12-22 per-link mass scale, 23-28 friction, 29-34 damping, 35 pad.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "../../include/pioneer_amd.h"
#include "pnr_device.h"

// The dynamics arithmetic has no bit-exactness contract (float32 vs a float64 oracle, tolerance-
// checked), so let a*b+c fuse here; integrate_joint (pnr_device.h) keeps its per-instruction
// no-contract flags when it is inlined into these kernels.  Restored at the end of this header.
#pragma clang fp contract(fast)

namespace pnr {

// first plane of each group of the dyn words above (pnr_get_dyn_state's layout, include/pioneer_amd.h: "q[6] qd[6] link-mass
// scale[11], friction[6], damping[6], 1 pad"); plane w of env e lies at dyn[w * n + e]
constexpr int kDynQ = 0, kDynQd = kDynQ + kDof, kDynScale = kDynQd + kDof, kDynFric = kDynScale + kNumLinks,
              kDynDamp = kDynFric + kDof;
static_assert(kDynQd == 6 && kDynScale == 12 && kDynFric == 23 && kDynDamp == 29 && kDynDamp + kDof + 1 == PNR_DYN_STATE_WORDS,
              "the dyn planes are the ABI's 36 words: 35 used + 1 pad");

// a static scene body as the kernels want it: world position, rotation matrix (row-major; a plane keeps its unit world
// normal in rot[0..2]), size (box half extents | sphere radius in size[0])
constexpr int kMaxScene = 8;
struct SceneBody { int shape; float pos[3]; float rot[9]; float size[3]; };

struct DynParams {
    float* dyn;                 // [36][n]
    float kp, kd, tau_max;      // PD gains, torque cap (<= 0: none)
    float gravity;
    float dt_sub;               // SimulationConfig.timestep
    int nsub;                   // SimulationConfig.frame_skip
    int teleport;
    int randomize;
    int has_ground;
    int has_box;
    float ground_z, ckp, ckd;
    float box_c[3], box_h[3], ptr_radius;   // static box obstacle for the pointer sphere
    float joint_damping, joint_friction;
    double mass_lo, mass_span, fric_lo, fric_span, damp_lo, damp_span;
    // motor law (bullet_scene.py:123-155), one form for POSITION_CONTROL, its maxVelocity cap and VELOCITY_CONTROL:
    //   tau = clip(kp_eff (r - q) + kd (clamp(v + c_pos (r - q), +-v_cap) - qd), +-tau_max)
    float kp_eff, c_pos, v_cap;
    int link_contacts;          // 1: the link capsules' sample spheres collide too (pnr_model.h kCapsules)
    int inertia_scaled;         // 1: the motor law is an acceleration request scaled by each joint's articulated inertia
    int n_scene;                // static bodies of create_body_plane / _box / _sphere (bullet_scene.py:193-228)
    const SceneBody* scene;     // [n_scene] in device memory (a by-value array indexed by the loop counter went to scratch)
};

// pnr_world_step (World.step, bullet_scene.py:273-275): the motor of every joint as Joint.control_position / control_velocity
// left it (bullet_scene.py:123-155), in the terms of the one motor law above — the same for every env of the handle.  A joint
// nobody commanded keeps the handle's own motor (DynParams), tracking the env's command state r, v (from_cmd).
// kind != kMotorPD: Bullet's velocity-level constraint motor instead (PNR_CONTROL_*_CONSTRAINT, motor_constraints below); its
// entries are then kp = positionGain, kd = velocityGain, vcap = maxVelocity (+inf: none), tcap = force (> 0), r_ref, v_ref.
enum : int { kMotorPD = 0, kMotorPositionConstraint = 1, kMotorVelocityConstraint = 2 };
struct JointMotorTable {
    float kp[kDof], kd[kDof], cpos[kDof], vcap[kDof], tcap[kDof];   // kp_eff, kd, c_pos, v_cap, torque cap (+inf: none) per joint
    float r_ref[kDof], v_ref[kDof];                                  // targetPosition / targetVelocity
    int from_cmd[kDof];                                              // 1: targets = the env's own r, v (no per-joint command)
    int kind[kDof];                                                  // kMotorPD | kMotor*Constraint
};

constexpr float kFrictionEps = 0.05f;   // smooth sign(qd) = qd / sqrt(qd^2 + eps^2)

// 1/x: hardware reciprocal (1 ulp) + one Newton step, instead of the ~10-instruction IEEE division
__device__ __forceinline__ float fast_rcp(float x)
{
    const float r = __builtin_amdgcn_rcpf(x);
    return r * (2.0f - x * r);
}

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(float s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ V3 cross(V3 a, V3 b)
{
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float comp(V3 a, int k) { return k == 0 ? a.x : (k == 1 ? a.y : a.z); }
__device__ __forceinline__ void add_comp(V3& a, int k, float v) { if (k == 0) a.x += v; else if (k == 1) a.y += v; else a.z += v; }

// R(axis, angle) v : child coordinates -> parent coordinates.  R^T v = rot<AX>(v, c, -s).
template <int AXn>
__device__ __forceinline__ V3 rot(V3 v, float c, float s)
{
    if (AXn == (int)AX) return {v.x, c * v.y - s * v.z, s * v.y + c * v.z};
    if (AXn == (int)AY) return {c * v.x + s * v.z, v.y, c * v.z - s * v.x};
    return {c * v.x - s * v.y, s * v.x + c * v.y, v.z};
}

// r_J x v with the constexpr joint origin r_J; vanishing terms are dropped at compile time
template <int J>
__device__ __forceinline__ V3 cross_r(V3 v)
{
    constexpr float rx = (float)kJoints[J].ox, ry = (float)kJoints[J].oy, rz = (float)kJoints[J].oz;
    V3 o = {0.f, 0.f, 0.f};
    if (ry != 0.f) { o.x += ry * v.z; o.z -= ry * v.x; }
    if (rz != 0.f) { o.x -= rz * v.y; o.y += rz * v.x; }
    if (rx != 0.f) { o.y -= rx * v.z; o.z += rx * v.y; }
    return o;
}

// 3x3 matrix as rows
struct M3 { V3 r0, r1, r2; };
__device__ __forceinline__ V3 mul(const M3& m, V3 v) { return {dot(m.r0, v), dot(m.r1, v), dot(m.r2, v)}; }
__device__ __forceinline__ V3 mulT(const M3& m, V3 v) { return v.x * m.r0 + v.y * m.r1 + v.z * m.r2; }
__device__ __forceinline__ V3 col(const M3& m, int k) { return {comp(m.r0, k), comp(m.r1, k), comp(m.r2, k)}; }
__device__ __forceinline__ V3 row(const M3& m, int k) { return k == 0 ? m.r0 : (k == 1 ? m.r1 : m.r2); }
__device__ __forceinline__ M3 operator+(const M3& a, const M3& b) { return {a.r0 + b.r0, a.r1 + b.r1, a.r2 + b.r2}; }
__device__ __forceinline__ M3 operator-(const M3& a, const M3& b) { return {a.r0 - b.r0, a.r1 - b.r1, a.r2 - b.r2}; }
__device__ __forceinline__ M3 transpose(const M3& m)
{
    return {{m.r0.x, m.r1.x, m.r2.x}, {m.r0.y, m.r1.y, m.r2.y}, {m.r0.z, m.r1.z, m.r2.z}};
}
__device__ __forceinline__ M3 outer(V3 a, V3 b) { return {a.x * b, a.y * b, a.z * b}; }
__device__ __forceinline__ M3 diag3(float d) { return {{d, 0.f, 0.f}, {0.f, d, 0.f}, {0.f, 0.f, d}}; }

// R M R^T
template <int AXn>
__device__ __forceinline__ M3 rot_block(const M3& m, float c, float s)
{
    // rows: R M  (each column transformed like a vector) == transform the row-vectors' mixing
    const M3 t = transpose(m);                                   // columns of m as rows
    const M3 rm = transpose(M3{rot<AXn>(t.r0, c, s), rot<AXn>(t.r1, c, s), rot<AXn>(t.r2, c, s)});  // R M
    return {rot<AXn>(rm.r0, c, s), rot<AXn>(rm.r1, c, s), rot<AXn>(rm.r2, c, s)};                   // (R M) R^T: rows times R^T
}

// R S R^T for a SYMMETRIC S: six unique entries.  With (a, b) the two coordinates the rotation mixes
// (v_a' = c v_a - s v_b, v_b' = s v_a + c v_b) and k the axis:
//   S'aa = c^2 Saa - 2cs Sab + s^2 Sbb     S'bb = s^2 Saa + 2cs Sab + c^2 Sbb
//   S'ab = cs (Saa - Sbb) + (c^2 - s^2) Sab  S'ak = c Sak - s Sbk   S'bk = s Sak + c Sbk   S'kk = Skk
template <int AXn>
__device__ __forceinline__ M3 rot_sym(const M3& m, float c, float s)
{
    constexpr int a = (AXn + 1) % 3, b = (AXn + 2) % 3, k = AXn;
    const float Saa = comp(row(m, a), a), Sbb = comp(row(m, b), b), Sab = comp(row(m, a), b);
    const float Sak = comp(row(m, a), k), Sbk = comp(row(m, b), k), Skk = comp(row(m, k), k);
    const float cc = c * c, ss = s * s, cs = c * s;
    const float naa = cc * Saa - 2.f * cs * Sab + ss * Sbb;
    const float nbb = ss * Saa + 2.f * cs * Sab + cc * Sbb;
    const float nab = cs * (Saa - Sbb) + (cc - ss) * Sab;
    const float nak = c * Sak - s * Sbk, nbk = s * Sak + c * Sbk;
    float e[3][3];
    e[a][a] = naa; e[b][b] = nbb; e[k][k] = Skk;
    e[a][b] = e[b][a] = nab; e[a][k] = e[k][a] = nak; e[b][k] = e[k][b] = nbk;
    return {{e[0][0], e[0][1], e[0][2]}, {e[1][0], e[1][1], e[1][2]}, {e[2][0], e[2][1], e[2][2]}};
}

// a a^T scaled: symmetric, six products
__device__ __forceinline__ M3 outer_sym(float k, V3 a)
{
    const float xx = k * a.x * a.x, yy = k * a.y * a.y, zz = k * a.z * a.z;
    const float xy = k * a.x * a.y, xz = k * a.x * a.z, yz = k * a.y * a.z;
    return {{xx, xy, xz}, {xy, yy, yz}, {xz, yz, zz}};
}

// ---- packed spatial algebra ---------------------------------------------------------
// CDNA4's fp32 vector peak needs v_pk_{fma,mul,add}_f32 (two results per instruction), and the
// compiler's SLP pass cannot find the pairs in this code without burying them in shuffles.  So the
// pairing is done by hand, by layout: every spatial quantity keeps its ANGULAR and LINEAR halves in
// one 64-bit register pair, because the recursion treats the two halves alike almost everywhere
// (same rotation, same axis products).  hipcc turns `f2` arithmetic straight into v_pk_* ops: a
// scalar operand becomes an op_sel_hi splat and `.yx` an op_sel swap, neither costs an instruction.
typedef float f2 __attribute__((ext_vector_type(2)));

// compile-time loops: every index below is a constant in the AST already (no local array or struct is
// ever indexed by a loop variable, so nothing can be left behind in scratch)
template <class F, int... Is>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) { (f(std::integral_constant<int, Is>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

template <int K> __device__ __forceinline__ float vc(const V3& a) { if constexpr (K == 0) return a.x; else if constexpr (K == 1) return a.y; else return a.z; }
template <int I, int J> __device__ __forceinline__ float mc(const M3& m)
{
    if constexpr (I == 0) return vc<J>(m.r0); else if constexpr (I == 1) return vc<J>(m.r1); else return vc<J>(m.r2);
}

// spatial vector: component i = (angular_i, linear_i)
struct P3 { f2 x, y, z; };
template <int K> __device__ __forceinline__ f2& pr(P3& a) { if constexpr (K == 0) return a.x; else if constexpr (K == 1) return a.y; else return a.z; }
template <int K> __device__ __forceinline__ const f2& pc(const P3& a) { if constexpr (K == 0) return a.x; else if constexpr (K == 1) return a.y; else return a.z; }
__device__ __forceinline__ P3 operator+(P3 a, P3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ P3 operator-(P3 a, P3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 ang(const P3& a) { return {a.x.x, a.y.x, a.z.x}; }
__device__ __forceinline__ V3 lin(const P3& a) { return {a.x.y, a.y.y, a.z.y}; }
__device__ __forceinline__ P3 pack(V3 a, V3 l) { return {{a.x, l.x}, {a.y, l.y}, {a.z, l.z}}; }

// both halves rotated by R(axis, angle): child -> parent; R^T = rotp<AX>(v, c, -s)
template <int AXn>
__device__ __forceinline__ P3 rotp(const P3& v, float c, float s)
{
    if (AXn == (int)AX) return {v.x, c * v.y - s * v.z, s * v.y + c * v.z};
    if (AXn == (int)AY) return {c * v.x + s * v.z, v.y, c * v.z - s * v.x};
    return {c * v.x - s * v.y, s * v.x + c * v.y, v.z};
}

// (v.a, v.l) x (e_k qd) for both halves: two packed products, component k is zero
template <int K>
__device__ __forceinline__ P3 cross_axis(const P3& v, float qd)
{
    constexpr int a = (K + 1) % 3, b = (K + 2) % 3;
    P3 c = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
    pr<a>(c) = pc<b>(v) * qd;
    pr<b>(c) = pc<a>(v) * (-qd);
    return c;
}

// E (v - [0; r_J x v.a]): the motion transform parent -> child of joint J
template <int J>
__device__ __forceinline__ P3 to_child(const P3& vp, float c, float s)
{
    constexpr int AXJ = (int)kJoints[J].axis;
    const V3 rxw = cross_r<J>(ang(vp));
    P3 t = vp;
    t.x.y -= rxw.x; t.y.y -= rxw.y; t.z.y -= rxw.z;
    return rotp<AXJ>(t, c, -s);
}

// spatial (articulated) inertia [[A, B], [B^T, C]] acting on [w; v]: n = A w + B v, f = B^T w + C v.
// A and C are symmetric and always transform alike: stored as six pairs (A_ij, C_ij).  B is general;
// its transpose transforms like B itself, so the off-diagonal entries are the pairs (B_ij, B_ji).
struct SIp {
    f2 ac[6];     // (A_ij, C_ij) for ij = 00 01 02 11 12 22
    float bd[3];  // B_00 B_11 B_22
    f2 bo[3];     // (B_01, B_10) (B_02, B_20) (B_12, B_21)
};
// compile-time index maps (variable templates, so they are constants wherever they are used)
constexpr int sidx_fn(int i, int j) { const int a = i < j ? i : j, b = i < j ? j : i; return a == 0 ? b : (a == 1 ? 2 + b : 5); }
template <int I, int J> constexpr int SIDX = sidx_fn(I, J);
template <int I, int J> constexpr int OIDX = I + J - 1;
// (B_ij, B_ji)
template <int I_, int J_>
__device__ __forceinline__ f2 bpair(const SIp& I)
{
    if constexpr (I_ == J_) return (f2)(I.bd[I_]);
    else if constexpr (I_ < J_) return I.bo[OIDX<I_, J_>];
    else return I.bo[OIDX<I_, J_>].yx;
}
template <int I_, int J_>
__device__ __forceinline__ float bget(const SIp& I)
{
    if constexpr (I_ == J_) return I.bd[I_];
    else if constexpr (I_ < J_) return I.bo[OIDX<I_, J_>].x;
    else return I.bo[OIDX<I_, J_>].y;
}
template <int I_, int J_>
__device__ __forceinline__ void bset(SIp& I, f2 v)     // v = (B_ij, B_ji), I_ != J_
{
    if constexpr (I_ < J_) I.bo[OIDX<I_, J_>] = v; else I.bo[OIDX<I_, J_>] = v.yx;
}
__device__ __forceinline__ M3 unpackB(const SIp& I)
{
    return {{I.bd[0], I.bo[0].x, I.bo[1].x}, {I.bo[0].y, I.bd[1], I.bo[2].x}, {I.bo[1].y, I.bo[2].y, I.bd[2]}};
}
__device__ __forceinline__ M3 unpackC(const SIp& I)
{
    return {{I.ac[0].y, I.ac[1].y, I.ac[2].y}, {I.ac[1].y, I.ac[3].y, I.ac[4].y}, {I.ac[2].y, I.ac[4].y, I.ac[5].y}};
}

// R I R^T of all four blocks.  (a, b) are the coordinates the rotation mixes (v_a' = c v_a - s v_b,
// v_b' = s v_a + c v_b), k the axis.  Symmetric pairs as rot_sym; for B
//   B'aa = cc Baa - cs (Bab + Bba) + ss Bbb          B'bb = ss Baa + cs (Bab + Bba) + cc Bbb
//   (B'ab, B'ba) = cs (Baa - Bbb) + cc (Bab, Bba) - ss (Bba, Bab)
//   (B'ak, B'ka) = c (Bak, Bka) - s (Bbk, Bkb)       (B'bk, B'kb) = s (Bak, Bka) + c (Bbk, Bkb)
template <int AXn>
__device__ __forceinline__ SIp rot_inertia(const SIp& I, float c, float s)
{
    constexpr int a = (AXn + 1) % 3, b = (AXn + 2) % 3, k = AXn;
    const float cc = c * c, ss = s * s, cs = c * s;
    SIp o;
    const f2 Saa = I.ac[SIDX<a, a>], Sbb = I.ac[SIDX<b, b>], Sab = I.ac[SIDX<a, b>];
    const f2 Sak = I.ac[SIDX<a, k>], Sbk = I.ac[SIDX<b, k>];
    const f2 x2 = (2.f * cs) * Sab;
    o.ac[SIDX<a, a>] = cc * Saa - x2 + ss * Sbb;
    o.ac[SIDX<b, b>] = ss * Saa + x2 + cc * Sbb;
    o.ac[SIDX<a, b>] = cs * (Saa - Sbb) + (cc - ss) * Sab;
    o.ac[SIDX<a, k>] = c * Sak - s * Sbk;
    o.ac[SIDX<b, k>] = s * Sak + c * Sbk;
    o.ac[SIDX<k, k>] = I.ac[SIDX<k, k>];
    const float Baa = I.bd[a], Bbb = I.bd[b];
    const f2 pab = bpair<a, b>(I), pak = bpair<a, k>(I), pbk = bpair<b, k>(I);
    const float m = cs * (pab.x + pab.y);
    o.bd[a] = cc * Baa - m + ss * Bbb;
    o.bd[b] = ss * Baa + m + cc * Bbb;
    o.bd[k] = I.bd[k];
    const f2 nab = cs * (Baa - Bbb) + cc * pab - ss * pab.yx;
    const f2 nak = c * pak - s * pbk;
    const f2 nbk = s * pak + c * pbk;
    bset<a, b>(o, nab);
    bset<a, k>(o, nak);
    bset<b, k>(o, nbk);
    return o;
}

// skew(r_J) * M (each column crossed with r) and M * skew(r_J)
template <int J>
__device__ __forceinline__ M3 rx_mul(const M3& m)
{
    const M3 t = transpose(m);
    return transpose(M3{cross_r<J>(t.r0), cross_r<J>(t.r1), cross_r<J>(t.r2)});
}
template <int J>
__device__ __forceinline__ M3 mul_rx(const M3& m)
{
    // (M rx) = -(rx M^T)^T  since rx^T = -rx
    const M3 t = rx_mul<J>(transpose(m));
    const M3 tt = transpose(t);
    return {-1.f * tt.r0, -1.f * tt.r1, -1.f * tt.r2};
}

// IP += X^T Ia X: body J's (articulated or composite) inertia, in J's frame, rotated into the parent's orientation and shifted
// to the parent's origin:  C_p = C', B_p = B' + rx C', A_p = A' - P - P^T - (rx C') rx  with P = B' rx
template <int J>
__device__ __forceinline__ void fold_inertia(const SIp& Ia, float cJ, float sJ, SIp& IP)
{
    constexpr int AXJ = (int)kJoints[J].axis;
    const SIp I1 = rot_inertia<AXJ>(Ia, cJ, sJ);
    const M3 C1 = unpackC(I1), B1 = unpackB(I1);
    const M3 T = rx_mul<J>(C1);
    const M3 Pm = mul_rx<J>(B1);
    const M3 Q = mul_rx<J>(T);
    static_for<3>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        IP.bd[i] += I1.bd[i] + mc<i, i>(T);
        static_for<3>([&](auto j_) {
            constexpr int j = decltype(j_)::value;
            if constexpr (j >= i) {
                IP.ac[SIDX<i, j>] += I1.ac[SIDX<i, j>];
                IP.ac[SIDX<i, j>].x -= mc<i, j>(Pm) + mc<j, i>(Pm) + mc<i, j>(Q);
            }
            if constexpr (j > i) {
                IP.bo[OIDX<i, j>] += I1.bo[OIDX<i, j>];
                IP.bo[OIDX<i, j>].x += mc<i, j>(T);
                IP.bo[OIDX<i, j>].y += mc<j, i>(T);
            }
        });
    });
}

struct DynBody {   // what pass 3 needs from pass 2
    P3 U;          // (Ua_i, Ul_i)
    float D, u;
};

struct DynModel {  // per-env rigid-body data from the 11 link scales
    float m[kDof];      // body masses (== isotropic inertia for bodies 0..4)
    V3 h6;              // first moment of body 6 (pointer offset)
    M3 I6;              // rotational inertia of body 6 about its origin
};

__device__ __forceinline__ void build_model(const float (&sc)[kNumLinks], DynModel& M)
{
    M.m[0] = sc[1] + sc[2]; M.m[1] = sc[3]; M.m[2] = sc[4]; M.m[3] = sc[5] + sc[6]; M.m[4] = sc[7];
    M.m[5] = sc[8] + sc[9] + sc[10];
    constexpr float tx = (float)kTipX, ty = (float)kTipY, tz = (float)kTipZ;
    const float mp = sc[10];
    M.h6 = {mp * tx, mp * ty, mp * tz};
    const float t2 = tx * tx + ty * ty + tz * tz;
    M.I6 = {{M.m[5] + mp * (t2 - tx * tx), -mp * tx * ty, -mp * tx * tz},
            {-mp * ty * tx, M.m[5] + mp * (t2 - ty * ty), -mp * ty * tz},
            {-mp * tz * tx, -mp * tz * ty, M.m[5] + mp * (t2 - tz * tz)}};
}

// one joint of pass 2 (tip -> base).  IA/pA: articulated inertia / bias force of body J in its own
// frame (children already folded in).  Emits U, D, u and folds body J into its parent (IP, pP).
// SCALED: the joint's motor asks for the acceleration adesJ; its torque is clip(D adesJ, +-tcap), D being the articulated
// inertia about the joint axis that this step forms anyway (pnr_config.pd_inertia_scaled)
template <int J, bool SCALED>
__device__ __forceinline__ void aba_inward(const SIp& IA, const P3& pA, const P3& vJ, float qdJ, float tauJ, float adesJ, float tcap,
                                           float cJ, float sJ, DynBody& out, SIp& IP, P3& pP)
{
    constexpr int k = (int)kJoints[J].axis;
    // U = I S: (Ua_j, Ul_j) = (A_jk, B_kj)
    P3 u;
    static_for<3>([&](auto j_) {
        constexpr int j = decltype(j_)::value;
        pr<j>(u) = (f2){IA.ac[SIDX<j, k>].x, bget<k, j>(IA)};
    });
    out.U = u;
    out.D = pc<k>(u).x;
    float tq = tauJ;
    if constexpr (SCALED) tq += fminf(fmaxf(out.D * adesJ, -tcap), tcap);
    out.u = tq - pc<k>(pA).x;
    if (J == 0) return;
    const float invD = fast_rcp(out.D);
    // Ia = IA - U U^T / D
    const P3 w = {invD * u.x, invD * u.y, invD * u.z};
    SIp Ia;
    static_for<3>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        Ia.bd[i] = IA.bd[i] - pc<i>(w).x * pc<i>(u).y;                // B_ij -= Ua_i Ul_j / D
        static_for<3>([&](auto j_) {
            constexpr int j = decltype(j_)::value;
            if constexpr (j >= i) Ia.ac[SIDX<i, j>] = IA.ac[SIDX<i, j>] - pc<i>(w) * pc<j>(u);
            if constexpr (j > i) {
                Ia.bo[OIDX<i, j>].x = IA.bo[OIDX<i, j>].x - pc<i>(w).x * pc<j>(u).y;
                Ia.bo[OIDX<i, j>].y = IA.bo[OIDX<i, j>].y - pc<j>(w).x * pc<i>(u).y;
            }
        });
    });
    // c = v x (S qd); pa = pA + Ia c + U u / D:
    //   (pa.a_i, pa.l_i) += (A_ij, C_ij) (ca_j, cl_j) + (B_ij, B_ji) (cl_j, ca_j)
    const P3 cv = cross_axis<k>(vJ, qdJ);
    const float ud = out.u * invD;
    P3 pa;
    static_for<3>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        f2 acc = pc<i>(pA) + ud * pc<i>(u);
        static_for<3>([&](auto j_) {
            constexpr int j = decltype(j_)::value;
            if constexpr (j != k) {                                   // c_k = 0
                acc += Ia.ac[SIDX<i, j>] * pc<j>(cv);
                acc += bpair<i, j>(Ia) * pc<j>(cv).yx;
            }
        });
        pr<i>(pa) = acc;
    });
    fold_inertia<J>(Ia, cJ, sJ, IP);
    constexpr int AXJ = (int)kJoints[J].axis;
    const P3 p1 = rotp<AXJ>(pa, cJ, sJ);
    const V3 rxf = cross_r<J>(lin(p1));
    pP = pP + p1;
    pP.x.x += rxf.x; pP.y.x += rxf.y; pP.z.x += rxf.z;
}

// rigid-body inertia and velocity-product bias of body J
template <int J>
__device__ __forceinline__ void rigid_body(const DynModel& M, const P3& vp, SIp& I, P3& p)
{
    const V3 va = ang(vp), vl = lin(vp);
    const float m = M.m[J];
    const f2 mm = {m, m}, zz = {0.f, 0.f};
    if (J < kDof - 1) {                    // A = C = m 1, B = 0
        I.ac[0] = mm; I.ac[1] = zz; I.ac[2] = zz; I.ac[3] = mm; I.ac[4] = zz; I.ac[5] = mm;
        I.bd[0] = I.bd[1] = I.bd[2] = 0.f;
        I.bo[0] = zz; I.bo[1] = zz; I.bo[2] = zz;
        p = pack(V3{0.f, 0.f, 0.f}, m * cross(va, vl));
    } else {                               // A = I6, B = skew(h), C = m 1
        const V3 h = M.h6;
        const float a00 = M.I6.r0.x, a01 = M.I6.r0.y, a02 = M.I6.r0.z, a11 = M.I6.r1.y, a12 = M.I6.r1.z, a22 = M.I6.r2.z;
        I.ac[0] = (f2){a00, m};   I.ac[1] = (f2){a01, 0.f}; I.ac[2] = (f2){a02, 0.f};
        I.ac[3] = (f2){a11, m};   I.ac[4] = (f2){a12, 0.f}; I.ac[5] = (f2){a22, m};
        I.bd[0] = I.bd[1] = I.bd[2] = 0.f;
        I.bo[0] = (f2){-h.z, h.z}; I.bo[1] = (f2){h.y, -h.y}; I.bo[2] = (f2){-h.x, h.x};
        const V3 n = V3{a00 * va.x + a01 * va.y + a02 * va.z, a01 * va.x + a11 * va.y + a12 * va.z,
                        a02 * va.x + a12 * va.y + a22 * va.z} + cross(h, vl);
        const V3 f = m * vl - cross(h, va);
        p = pack(cross(va, n) + cross(vl, f), cross(va, f));
    }
}

template <int J>
__device__ __forceinline__ void vel_outward(const P3& vp, float c, float s, float qd, P3& v)
{
    constexpr int AXJ = (int)kJoints[J].axis;
    v = to_child<J>(vp, c, s);
    pr<AXJ>(v).x += qd;
}

template <int J>
__device__ __forceinline__ void acc_outward(const P3& ap, const P3& vJ, float c, float s, float qd, const DynBody& b,
                                            float& qdd, P3& a)
{
    constexpr int AXJ = (int)kJoints[J].axis;
    a = to_child<J>(ap, c, s) + cross_axis<AXJ>(vJ, qd);
    const f2 d = b.U.x * a.x + b.U.y * a.y + b.U.z * a.z;             // (Ua . a.a, Ul . a.l)
    qdd = (b.u - (d.x + d.y)) * fast_rcp(b.D);
    pr<AXJ>(a).x += qdd;
}

// R = Rp * R(axis_J, q_J): each row of Rp times R, (row * R) = rot(row, c, -s)
template <int J>
__device__ __forceinline__ M3 rot_outward(const M3& Rp, float c, float s)
{
    constexpr int AXJ = (int)kJoints[J].axis;
    return {rot<AXJ>(Rp.r0, c, -s), rot<AXJ>(Rp.r1, c, -s), rot<AXJ>(Rp.r2, c, -s)};
}

// world pose of body J from its parent's (for the pointer/ground contact)
template <int J>
__device__ __forceinline__ void pose_outward(const M3& Rp, V3 pp, float c, float s, M3& R, V3& p)
{
    constexpr float ox = (float)kJoints[J].ox, oy = (float)kJoints[J].oy, oz = (float)kJoints[J].oz;
    p = pp + mul(Rp, V3{ox, oy, oz});
    R = rot_outward<J>(Rp, c, s);
}

// ---------------------------------------------------------------------------------
// pnr_set_body_params: ONE MOVING SPHERE per env that the world step integrates with the arm (the law is stated in
// include/pioneer_amd.h): a point mass with a radius — position and linear velocity, no orientation, no spin; rolling is not
// modelled.  The buffer and the params are the kernel argument WorldBody (its own slot, pnr_env_kernels.h kArgBody); the lane keeps
// the env's eight words and the sub-step's force in SphereLane.  An env with mass <= 0 has no sphere: it takes and gives no force.
// ---------------------------------------------------------------------------------
struct WorldBody {
    float* words;                        // [PNR_BODY_STATE_WORDS][n]: x[3] v[3] mass radius
    float kp, kd, friction, slip_eps, linear_damping;
    unsigned joint_mask;                 // the targets form's joint mask rides here (that form has no slot left for kArgMask)
};
struct SphereLane { V3 x, v; float m, r; V3 F; };
// pnr_set_body_grip_params (kWorldGrip): the forms with the grip take this argument in WorldBody's place (kArgGripBody) and carry this
// lane; every other form's argument and lane are the ones above, untouched.  Where a kWorldGrip instantiation holds a WorldBody or a
// SphereLane pointer, the object is one of these.
struct WorldGrip : WorldBody {
    float* grip;                         // [PNR_BODY_GRIP_WORDS][n]: max_force, then the last sub-step's force on the sphere[3]
    float grip_kp, grip_kd;
    float anchor[3], direction[3];       // c_a = kTip + anchor + (radius + pointer_radius) direction, in moving body 5's frame; wave-uniform
};
struct GripLane : SphereLane {
    float g;                             // the env's grip word max_force (> 0: held)
    V3 G;                                // the grip's force on the sphere in this sub-step
};

// ---------------------------------------------------------------------------------
// The contact geometry of the static bodies and the penalty law, stated once for the step's arm samples (sample_contact), the
// moving sphere (sphere_static) and pnr_get_contacts (pnr_contacts.h contact_sample): the nearest-face tie rule, the fallback of
// a zero-length normal and the surface-to-surface convention are the same text for all three.
// ---------------------------------------------------------------------------------
// signed distance of l (in the box's frame) to the box of half extents h and the outward normal there: outside the direction of
// the nearest surface point, inside out through the nearest face
__device__ __forceinline__ void box_sdf(V3 l, const float (&h)[3], float& sdf, V3& nl)
{
    const V3 q = {fabsf(l.x) - h[0], fabsf(l.y) - h[1], fabsf(l.z) - h[2]};
    const V3 o = {fmaxf(q.x, 0.f), fmaxf(q.y, 0.f), fmaxf(q.z, 0.f)};
    const float out2 = dot(o, o);
    if (out2 > 0.f) {
        const float len = sqrtf(out2);
        sdf = len;
        nl = {(l.x < 0.f ? -o.x : o.x) / len, (l.y < 0.f ? -o.y : o.y) / len, (l.z < 0.f ? -o.z : o.z) / len};
    } else {                                           // inside: out through the nearest face
        const int km = (q.x >= q.y && q.x >= q.z) ? 0 : (q.y >= q.z ? 1 : 2);
        sdf = comp(q, km);
        nl = {km == 0 ? (l.x < 0.f ? -1.f : 1.f) : 0.f, km == 1 ? (l.y < 0.f ? -1.f : 1.f) : 0.f,
              km == 2 ? (l.z < 0.f ? -1.f : 1.f) : 0.f};
    }
}

// signed distance of the point `pos` to the body S placed at `o`, and the body's unit outward normal there (world frame)
__device__ __forceinline__ void body_distance(const SceneBody& S, V3 o, V3 pos, float& sdf, V3& nrm)
{
    const V3 dd = pos - o;
    if (S.shape == 1) {                                // plane: unit world normal in rot[0..2]
        nrm = {S.rot[0], S.rot[1], S.rot[2]};
        sdf = dot(nrm, dd);
    } else if (S.shape == 3) {                         // sphere
        const float len = sqrtf(dot(dd, dd));
        sdf = len - S.size[0];
        nrm = len > 0.f ? (1.f / len) * dd : V3{0.f, 0.f, 1.f};
    } else {                                           // oriented box: into its frame, out again with the normal
        const V3 l = {S.rot[0] * dd.x + S.rot[3] * dd.y + S.rot[6] * dd.z, S.rot[1] * dd.x + S.rot[4] * dd.y + S.rot[7] * dd.z,
                      S.rot[2] * dd.x + S.rot[5] * dd.y + S.rot[8] * dd.z};
        V3 nl;
        box_sdf(l, S.size, sdf, nl);
        nrm = {S.rot[0] * nl.x + S.rot[1] * nl.y + S.rot[2] * nl.z, S.rot[3] * nl.x + S.rot[4] * nl.y + S.rot[5] * nl.z,
               S.rot[6] * nl.x + S.rot[7] * nl.y + S.rot[8] * nl.z};
    }
}

// The penalty law of every contact: fn = kp depth - kd vn for a contact of depth `depth` whose surfaces part at vn along the normal.
// True while it acts, depth > 0 and fn > 0: the force is max(0, fn) gated on depth > 0.  The test and fn are handed out separately so
// that a caller's `if` is the one the kernels were tuned with (the other forms tried: DESIGN.md 3s)
__device__ __forceinline__ bool penalty(float kp, float kd, float depth, float vn, float& fn)
{
    fn = kp * depth - kd * vn;
    return depth > 0.f && fn > 0.f;
}

// one static contact of the sphere, surface to surface: the penalty force along n plus the regularised sliding friction
__device__ __forceinline__ void sphere_touch(const WorldBody& B, SphereLane& S, float sdf, V3 n)
{
    const float vn = dot(S.v, n);
    float fn;
    if (penalty(B.kp, B.kd, S.r - sdf, vn, fn)) {
        const V3 vt = S.v - vn * n;
        const float k = B.friction * fn * __builtin_amdgcn_rsqf(dot(vt, vt) + B.slip_eps * B.slip_eps);
        S.F = S.F + fn * n - k * vt;
    }
}

// S.F = the static world's force on the sphere at the sub-step's start: the ground plane, the axis-aligned box, the scene's bodies
__device__ __forceinline__ void sphere_static(const DynParams& D, const WorldBody& B, SphereLane& S)
{
    S.F = {0.f, 0.f, 0.f};
    if (D.has_ground) sphere_touch(B, S, S.x.z - D.ground_z, V3{0.f, 0.f, 1.f});
    if (D.has_box) {
        V3 nrm; float sdf;
        box_sdf(S.x - V3{D.box_c[0], D.box_c[1], D.box_c[2]}, D.box_h, sdf, nrm);
        sphere_touch(B, S, sdf, nrm);
    }
#pragma unroll 1
    for (int b = 0; b < D.n_scene; ++b) {
        const SceneBody Sb = D.scene[b];
        V3 nrm; float sdf;
        body_distance(Sb, V3{Sb.pos[0], Sb.pos[1], Sb.pos[2]}, S.x, sdf, nrm);
        sphere_touch(B, S, sdf, nrm);
    }
}

// the sphere's semi-implicit Euler step under S.F, linear damping and gravity (inv_m: 1 / mass)
__device__ __forceinline__ void sphere_integrate(const DynParams& D, const WorldBody& B, float inv_m, SphereLane& S)
{
    const float h = D.dt_sub;
    S.v = S.v + h * (inv_m * S.F - B.linear_damping * S.v - V3{0.f, 0.f, D.gravity});
    S.x = S.x + h * S.v;
}

// Penalty contact of ONE sample sphere (centre c in the frame of the body whose world pose is R, p and whose spatial
// velocity in body coordinates is vb) with the ground plane, the static axis-aligned box (the reference demo's scene
// extras, pioneer_knm_env.py:249-261; create_body_plane / create_body_box, bullet_scene.py:206-228) and the scene's bodies: the
// contact force is added to the body's external spatial force in body coordinates.
// SPHERE (kWorldBody): the sample also meets the env's moving sphere S; the pair's force goes to S.F and, reversed, into F here.
// kSphereGrip (kWorldGrip): .. unless the env's sphere is held (S.g > 0), which takes no arm contact from any sample.
enum : int { kSphereNone = 0, kSphereFree = 1, kSphereGrip = 2 };
template <int SPHERE = kSphereNone>
__device__ __forceinline__ void sample_contact(const DynParams& D, const M3& R, V3 p, const P3& vb, V3 c, float radius, P3& fext,
                                               const WorldBody* B = nullptr, SphereLane* S = nullptr)
{
    const V3 pos = p + mul(R, c);                           // world position of the sphere centre
    const V3 vw = mul(R, lin(vb) + cross(ang(vb), c));      // its world velocity
    V3 F = {0.f, 0.f, 0.f};
    // the ground: the pointer alone touches with its centre (the r01 form); with link contacts every sphere with its surface.
    // F is zero still, so this is an assignment (why not `+=`: DESIGN.md 3s)
    if (D.has_ground) {
        float fz;
        F.z = penalty(D.ckp, D.ckd, D.ground_z - pos.z + (D.link_contacts ? radius : 0.f), vw.z, fz) ? fz : 0.f;
    }
    if (D.has_box) {
        V3 nrm; float sdf;
        box_sdf(pos - V3{D.box_c[0], D.box_c[1], D.box_c[2]}, D.box_h, sdf, nrm);
        float fn;
        if (penalty(D.ckp, D.ckd, radius - sdf, dot(vw, nrm), fn)) F = F + fn * nrm;
    }
    // the scene's static bodies: wave-uniform loop over a small device array, the sample touches with its surface
#pragma unroll 1
    for (int b = 0; b < D.n_scene; ++b) {
        const SceneBody Sb = D.scene[b];
        V3 nrm; float sdf;
        body_distance(Sb, V3{Sb.pos[0], Sb.pos[1], Sb.pos[2]}, pos, sdf, nrm);
        float fn;
        if (penalty(D.ckp, D.ckd, radius - sdf, dot(vw, nrm), fn)) F = F + fn * nrm;
    }
    if constexpr (SPHERE != kSphereNone) {
        const V3 d = S->x - pos;
        const float len = sqrtf(dot(d, d));
        const V3 nrm = len > 0.f ? (1.f / len) * d : V3{0.f, 0.f, 1.f};
        float fn;
        const bool hit = penalty(B->kp, B->kd, S->r + radius - len, dot(S->v - vw, nrm), fn);
        bool on = S->m > 0.f && hit;
        if constexpr (SPHERE == kSphereGrip) on = on && !(static_cast<const GripLane*>(S)->g > 0.f);
        if (on) { S->F = S->F + fn * nrm; F = F - fn * nrm; }
    }
    const V3 fb = mulT(R, F);                             // R^T F
    fext = fext + pack(cross(c, fb), fb);
}

// first sample index of capsule ci in table order; of kNumCapsules: the number of samples
__host__ __device__ constexpr int contact_sample_base(int ci)
{
    int k = 0;
    for (int i = 0; i < ci; ++i) k += kCapsules[i].n;
    return k;
}
constexpr int kContactSamples = contact_sample_base(kNumCapsules);

// The sample spheres of moving body BODY, in the order of the compile-time table kCapsules: f(s, c, radius, tip) with the sample's
// table index s (an integral_constant), its centre c in the body's frame, its radius (< 0: the pointer's, a run-time parameter)
// and whether it is the pointer itself, the last sample of the last capsule (a bool_constant); every one a constant in the callee.
template <int BODY, class F>
__device__ __forceinline__ void for_body_samples(F&& f)
{
    static_for<kNumCapsules>([&](auto ci_) {
        constexpr int ci = decltype(ci_)::value;
        if constexpr (kCapsules[ci].body == BODY) {
            static_for<kCapsules[ci].n>([&](auto i_) {
                constexpr int i = decltype(i_)::value;
                constexpr CapsuleDef K = kCapsules[ci];
                constexpr float t = K.n > 1 ? (float)((double)i / (double)(K.n - 1)) : 0.f;
                constexpr bool tip = (ci == kNumCapsules - 1) && (i == K.n - 1);
                const V3 c = tip ? V3{(float)kTipX, (float)kTipY, (float)kTipZ}
                                 : V3{K.ax + t * (K.bx - K.ax), K.ay + t * (K.by - K.ay), K.az + t * (K.bz - K.az)};
                f(std::integral_constant<int, contact_sample_base(ci) + i>{}, c, K.radius, std::bool_constant<tip>{});
            });
        }
    });
}

// every sample sphere of moving body BODY; without link contacts only the pointer
template <int BODY, int SPHERE = kSphereNone>
__device__ __forceinline__ void body_contacts(const DynParams& D, const M3& R, V3 p, const P3& vb, P3& fext, const WorldBody* B = nullptr,
                                              SphereLane* S = nullptr)
{
    for_body_samples<BODY>([&](auto, V3 c, float radius, auto tip) {
        if (tip || D.link_contacts) sample_contact<SPHERE>(D, R, p, vb, c, radius < 0.f ? D.ptr_radius : radius, fext, B, S);
    });
}

// pnr_set_body_grip_params (the law is stated in include/pioneer_amd.h): the soft point-to-point constraint between the anchor point
// c_a of moving body 5 (world pose R, p; spatial velocity vb in body coordinates) and the sphere's centre, capped at the lane's
// max_force S.g.  +F goes to S.F (and to S.G, for the report), -F enters fext at c_a as a contact reaction does.  A lane that is
// not held (S.g <= 0 or no sphere) adds exact zeros: selects, no branch.
__device__ __forceinline__ void grip_force(const DynParams& D, const WorldGrip& B, const M3& R, V3 p, const P3& vb, P3& fext, GripLane& S)
{
    const float reach = S.r + D.ptr_radius;
    const V3 c = {(float)kTipX + B.anchor[0] + reach * B.direction[0], (float)kTipY + B.anchor[1] + reach * B.direction[1],
                  (float)kTipZ + B.anchor[2] + reach * B.direction[2]};
    const V3 pos = p + mul(R, c);                           // exactly how sample_contact gets pos, vw
    const V3 vw = mul(R, lin(vb) + cross(ang(vb), c));
    const V3 Fr = (-B.grip_kp) * (S.x - pos) - B.grip_kd * (S.v - vw);
    const bool held = S.g > 0.f && S.m > 0.f;
    const float k = fminf(1.f, S.g / sqrtf(dot(Fr, Fr)));   // |Fr| = 0: max_force / 0 = +inf, k = 1
    const V3 F = {held ? k * Fr.x : 0.f, held ? k * Fr.y : 0.f, held ? k * Fr.z : 0.f};
    S.F = S.F + F;
    S.G = F;
    const V3 fb = mulT(R, V3{-F.x, -F.y, -F.z});
    fext = fext + pack(cross(c, fb), fb);
}

// the external spatial force of all active contacts on every body, in body coordinates
template <int SPHERE = kSphereNone>
__device__ __forceinline__ void contact_wrenches(const DynParams& D, const float (&c)[kDof], const float (&s)[kDof],
                                                 const P3 (&v)[kDof], P3 (&fext)[kDof], const WorldBody* B = nullptr, SphereLane* S = nullptr)
{
    M3 R = {{1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}}, Rn;
    V3 p = {0.f, 0.f, 0.f}, pn;
    pose_outward<0>(R, p, c[0], s[0], Rn, pn); R = Rn; p = pn;          // body 0 (rotator1 + hinge1) carries no samples
    pose_outward<1>(R, p, c[1], s[1], Rn, pn); R = Rn; p = pn; body_contacts<1, SPHERE>(D, R, p, v[1], fext[1], B, S);
    pose_outward<2>(R, p, c[2], s[2], Rn, pn); R = Rn; p = pn; body_contacts<2, SPHERE>(D, R, p, v[2], fext[2], B, S);
    pose_outward<3>(R, p, c[3], s[3], Rn, pn); R = Rn; p = pn; body_contacts<3, SPHERE>(D, R, p, v[3], fext[3], B, S);
    pose_outward<4>(R, p, c[4], s[4], Rn, pn); R = Rn; p = pn; body_contacts<4, SPHERE>(D, R, p, v[4], fext[4], B, S);
    pose_outward<5>(R, p, c[5], s[5], Rn, pn); R = Rn; p = pn; body_contacts<5, SPHERE>(D, R, p, v[5], fext[5], B, S);
    if constexpr (SPHERE == kSphereGrip) grip_force(D, *static_cast<const WorldGrip*>(B), R, p, v[5], fext[5], *static_cast<GripLane*>(S));
}

// ---------------------------------------------------------------------------------
// pnr_world_step_wrenches: the caller's wrenches on links of the arm (PyBullet's applyExternalForce / applyExternalTorque; the law
// is stated in include/pioneer_amd.h).  The call-uniform part of the records travels by value, as the motor table does: every
// branch on it is wave-uniform, and no per-lane array is ever indexed by it (body and record indices are compile-time, the table
// only decides whether a piece of code runs).
// ---------------------------------------------------------------------------------
constexpr int kMaxWrench = PNR_MAX_LINK_WRENCHES;
struct LinkWrenchTable {
    int n;                          // records per env, 1..kMaxWrench (the stride of the input; the kernel loads records 0..n-1)
    // the dynamic body (0..5) of the record's link, in the entry of the record's frame; the other entry, and both for a record that
    // does nothing (beyond n, or on robot:base, which is welded to the world), are -1: one scalar compare decides a block
    int lbody[kMaxWrench];          // PNR_FRAME_LINK records
    int wbody[kMaxWrench];          // PNR_FRAME_WORLD records
    float d[kMaxWrench][3];         // the link origin in its body's coordinates (kTip for the pointer, 0 for every other link)
    int last_world_body;            // the outermost body that carries a world-frame record; -1: none (no rotation is built)
    int hold;                       // the records act in sub-steps 0 .. hold - 1 (1 .. nsub)
};
// One lane's records, nine floats each.  As loaded: force | position | torque.  After wrench_prepare, a link-frame record is
// f_b | n_b | - (its constant body wrench) and a world-frame record F | p_b | T (the world force and torque, the material point
// in body coordinates).
struct WrenchLane { float w[kMaxWrench][9]; };

// env e's records 0 .. T.n - 1 of wrenches [n][T.n][9] (env-major); the lane's other records stay as the caller set them
__device__ __forceinline__ void load_wrench_records(const float* __restrict__ wrenches, const LinkWrenchTable& T, long long e, WrenchLane& L)
{
    const float* wr = wrenches + e * (9 * T.n);
    static_for<kMaxWrench>([&](auto j_) {
        constexpr int j = decltype(j_)::value;
        if (j < T.n) {
#pragma unroll
            for (int i = 0; i < 9; ++i) L.w[j][i] = wr[9 * j + i];
        }
    });
}

// env e's six joint torques of tau_ext [n][6] (env-major, 24 B per env, 8-byte aligned since the buffer is 16-byte aligned)
__device__ __forceinline__ void load_joint_torques(const float* __restrict__ tau_ext, long long e, float (&tx)[kDof])
{
    const float2* t2 = reinterpret_cast<const float2*>(tau_ext) + 3 * e;
    const float2 x0 = t2[0], x1 = t2[1], x2 = t2[2];
    tx[0] = x0.x; tx[1] = x0.y; tx[2] = x1.x; tx[3] = x1.y; tx[4] = x2.x; tx[5] = x2.y;
}

// before the sub-steps, at the pose q0 of the call's start (c, s = cos / sin q0)
__device__ __forceinline__ void wrench_prepare(const LinkWrenchTable& T, const float (&c)[kDof], const float (&s)[kDof], WrenchLane& L)
{
    static_for<kMaxWrench>([&](auto j_) {
        constexpr int j = decltype(j_)::value;
        if (T.lbody[j] >= 0) {                                         // n_b = (d + position) x force + torque
            float (&w)[9] = L.w[j];
            const V3 F = {w[0], w[1], w[2]}, P = {w[3] + T.d[j][0], w[4] + T.d[j][1], w[5] + T.d[j][2]};
            const V3 nb = cross(P, F) + V3{w[6], w[7], w[8]};
            w[3] = nb.x; w[4] = nb.y; w[5] = nb.z;
        }
    });
    if (T.last_world_body < 0) return;
    M3 R = diag3(1.f);
    V3 p = {0.f, 0.f, 0.f};
    static_for<kDof>([&](auto b_) {
        constexpr int B = decltype(b_)::value;
        if (B <= T.last_world_body) {
            M3 Rn; V3 pn;
            pose_outward<B>(R, p, c[B], s[B], Rn, pn); R = Rn; p = pn;
            static_for<kMaxWrench>([&](auto j_) {
                constexpr int j = decltype(j_)::value;
                if (T.wbody[j] == B) {                                // p_b = R_b(q0)^T (position - o_b(q0))
                    float (&w)[9] = L.w[j];
                    const V3 pb = mulT(R, V3{w[3], w[4], w[5]} - p);
                    w[3] = pb.x; w[4] = pb.y; w[5] = pb.z;
                }
            });
        }
    });
}

// one sub-step's fext[body] = (n_b, f_b) of all records, at the pose whose cos / sin are c, s
__device__ __forceinline__ void wrench_forces(const LinkWrenchTable& T, const float (&c)[kDof], const float (&s)[kDof], const WrenchLane& L,
                                              P3 (&fext)[kDof])
{
#pragma unroll
    for (int i = 0; i < kDof; ++i) fext[i] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
    static_for<kMaxWrench>([&](auto j_) {
        constexpr int j = decltype(j_)::value;
        if (T.lbody[j] >= 0) {
            const float (&w)[9] = L.w[j];
            const P3 f = pack(V3{w[3], w[4], w[5]}, V3{w[0], w[1], w[2]});
            static_for<kDof>([&](auto b_) {
                constexpr int B = decltype(b_)::value;
                if (T.lbody[j] == B) fext[B] = fext[B] + f;
            });
        }
    });
    if (T.last_world_body < 0) return;
    M3 R = diag3(1.f);
    static_for<kDof>([&](auto b_) {
        constexpr int B = decltype(b_)::value;
        if (B <= T.last_world_body) {
            R = rot_outward<B>(R, c[B], s[B]);
            static_for<kMaxWrench>([&](auto j_) {
                constexpr int j = decltype(j_)::value;
                if (T.wbody[j] == B) {                                // f_b = R^T F, n_b = p_b x f_b + R^T T
                    const float (&w)[9] = L.w[j];
                    const V3 fb = mulT(R, V3{w[0], w[1], w[2]});
                    const V3 nb = cross(V3{w[3], w[4], w[5]}, fb) + mulT(R, V3{w[6], w[7], w[8]});
                    fext[B] = fext[B] + pack(nb, fb);
                }
            });
        }
    });
}

// qdd = ABA(q, qd, tau).  CONTACT: the penalty contacts' external forces are subtracted from the bodies' bias forces
// (a separate instantiation: the contact-free kernels carry none of that code or its registers)
// c, s: cos / sin of the joint angles (dyn_core carries them across the sub-steps)
// PHYS: bit 0 = contacts, bit 1 = the inertia-scaled motor (its acceleration requests in ades, torque cap tcap)
// EXT (pnr_world_step_wrenches): ext[6], the caller's wrenches of this sub-step in body coordinates; the contacts add into the same
// fext, and body 0 (which carries no contact samples) has its bias force reduced as well
// SPHERE (kWorldBody): the contact samples also meet the env's moving sphere, whose force accumulator sphere->F takes its share;
// kSphereGrip (kWorldGrip): and the grip holds it at body 5's anchor point
template <int PHYS, bool EXT = false, int SPHERE = kSphereNone>
__device__ __forceinline__ void aba(const DynParams& D, const DynModel& M, const float (&c)[kDof], const float (&s)[kDof],
                                    const float (&qd)[kDof], const float (&tau)[kDof], const float (&ades)[kDof], const float (&tcap)[kDof],
                                    float (&qdd)[kDof], const P3* ext = nullptr, const WorldBody* sphere_p = nullptr, SphereLane* sphere = nullptr)
{
    constexpr bool CONTACT = (PHYS & 1) != 0, SCALED = (PHYS & 2) != 0;

    // pass 1: body velocities
    P3 v[kDof];
    const P3 v0 = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
    vel_outward<0>(v0, c[0], s[0], qd[0], v[0]);
    vel_outward<1>(v[0], c[1], s[1], qd[1], v[1]);
    vel_outward<2>(v[1], c[2], s[2], qd[2], v[2]);
    vel_outward<3>(v[2], c[3], s[3], qd[3], v[3]);
    vel_outward<4>(v[3], c[4], s[4], qd[4], v[4]);
    vel_outward<5>(v[4], c[5], s[5], qd[5], v[5]);

    P3 fext[kDof];
    if (CONTACT || EXT) {
#pragma unroll
        for (int i = 0; i < kDof; ++i) fext[i] = EXT ? ext[i] : v0;
    }
    if (CONTACT) contact_wrenches<SPHERE>(D, c, s, v, fext, sphere_p, sphere);

    // pass 2: tip -> base
    DynBody B[kDof];
    SIp IA, IP; P3 pA, pP;
    rigid_body<5>(M, v[5], IA, pA);
    if (CONTACT || EXT) pA = pA - fext[5];
    rigid_body<4>(M, v[4], IP, pP);
    if (CONTACT || EXT) pP = pP - fext[4];
    aba_inward<5, SCALED>(IA, pA, v[5], qd[5], tau[5], ades[5], tcap[5], c[5], s[5], B[5], IP, pP);
    IA = IP; pA = pP; rigid_body<3>(M, v[3], IP, pP);
    if (CONTACT || EXT) pP = pP - fext[3];
    aba_inward<4, SCALED>(IA, pA, v[4], qd[4], tau[4], ades[4], tcap[4], c[4], s[4], B[4], IP, pP);
    IA = IP; pA = pP; rigid_body<2>(M, v[2], IP, pP);
    if (CONTACT || EXT) pP = pP - fext[2];
    aba_inward<3, SCALED>(IA, pA, v[3], qd[3], tau[3], ades[3], tcap[3], c[3], s[3], B[3], IP, pP);
    IA = IP; pA = pP; rigid_body<1>(M, v[1], IP, pP);
    if (CONTACT || EXT) pP = pP - fext[1];
    aba_inward<2, SCALED>(IA, pA, v[2], qd[2], tau[2], ades[2], tcap[2], c[2], s[2], B[2], IP, pP);
    IA = IP; pA = pP; rigid_body<0>(M, v[0], IP, pP);
    if (EXT) pP = pP - fext[0];
    aba_inward<1, SCALED>(IA, pA, v[1], qd[1], tau[1], ades[1], tcap[1], c[1], s[1], B[1], IP, pP);
    IA = IP; pA = pP;
    aba_inward<0, SCALED>(IA, pA, v[0], qd[0], tau[0], ades[0], tcap[0], c[0], s[0], B[0], IP, pP);

    // pass 3: base -> tip; gravity as a base acceleration +g along z
    P3 a0 = {{0.f, 0.f}, {0.f, 0.f}, {0.f, D.gravity}}, a1;
    acc_outward<0>(a0, v[0], c[0], s[0], qd[0], B[0], qdd[0], a1); a0 = a1;
    acc_outward<1>(a0, v[1], c[1], s[1], qd[1], B[1], qdd[1], a1); a0 = a1;
    acc_outward<2>(a0, v[2], c[2], s[2], qd[2], B[2], qdd[2], a1); a0 = a1;
    acc_outward<3>(a0, v[3], c[3], s[3], qd[3], B[3], qdd[3], a1); a0 = a1;
    acc_outward<4>(a0, v[4], c[4], s[4], qd[4], B[4], qdd[4], a1); a0 = a1;
    acc_outward<5>(a0, v[5], c[5], s[5], qd[5], B[5], qdd[5], a1);
}

// ---------------------------------------------------------------------------------
// Bullet's joint motor (btMultiBodyJointMotor, pybullet's setJointMotorControl2): a velocity-level constraint per motorised
// joint, solved per sub-step of length h over the coupled chain (pnr_set_joint_motor's PNR_CONTROL_*_CONSTRAINT).  With S the
// constraint joints, qdd_free the ABA with tau_S = 0 and M the joint-space mass matrix, tau_S solves the boxed problem
//   qd+ = qd + h (qdd_free + M^-1 tau),   per i in S: qd+_i = rhs_i with |tau_i| < F_i, or tau_i = +-F_i with qd+_i short of
//   rhs_i on that side.
// Active-set solve in the unknowns dv = qd+ - (qd + h qdd_free) and tau, with M dv = h tau (tau = 0 off S): a FREE joint has
// its dv known (rhs - b), every other joint its tau (0, or +-F when clamped).  The known dv are moved to the right-hand side,
// which leaves an SPD system G dv = r (M's block over the unknown dv, identity rows for the known ones), factored by a 6x6
// Cholesky with compile-time indices — the per-lane free / clamped pattern only selects entries, so nothing is indexed at run
// time.  Each pass clamps the free joints whose torque exceeds F and frees the clamped ones whose velocity passed rhs; at most
// kMotorPasses passes (the last one's solve stands if the pattern still changed).
// ---------------------------------------------------------------------------------
constexpr int kMotorPasses = 2 * kDof;

// packed lower triangle of a symmetric 6x6
template <int I, int J> constexpr int TRI = I >= J ? I * (I + 1) / 2 + J : J * (J + 1) / 2 + I;
constexpr int kTri = kDof * (kDof + 1) / 2;

// the force transform of joint J: body J's frame -> its parent's (as pass 2 of the ABA carries the bias force)
template <int J>
__device__ __forceinline__ P3 force_to_parent(const P3& f, float c, float s)
{
    constexpr int AXJ = (int)kJoints[J].axis;
    P3 p = rotp<AXJ>(f, c, s);
    const V3 rxf = cross_r<J>(lin(p));
    p.x.x += rxf.x; p.y.x += rxf.y; p.z.x += rxf.z;
    return p;
}

// H = M(q) by the composite-rigid-body algorithm on the ABA's own rigid-body inertias and joint transforms
__device__ __forceinline__ void mass_matrix(const DynModel& M, const float (&c)[kDof], const float (&s)[kDof], float (&H)[kTri])
{
    const P3 v0 = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
    SIp IC; P3 unused;
    rigid_body<kDof - 1>(M, v0, IC, unused);
    static_for<kDof>([&](auto t_) {
        constexpr int i = kDof - 1 - decltype(t_)::value;
        constexpr int k = (int)kJoints[i].axis;
        P3 F;                                                         // IC_i S_i: (A_jk, B_kj), as U in aba_inward
        static_for<3>([&](auto j_) {
            constexpr int j = decltype(j_)::value;
            pr<j>(F) = (f2){IC.ac[SIDX<j, k>].x, bget<k, j>(IC)};
        });
        H[TRI<i, i>] = pc<k>(F).x;
        static_for<i>([&](auto u_) {                                  // up the chain: H_{i, j-1} = S_{j-1}^T X^T ... F
            constexpr int j = i - decltype(u_)::value;
            F = force_to_parent<j>(F, c[j], s[j]);
            H[TRI<i, j - 1>] = pc<(int)kJoints[j - 1].axis>(F).x;
        });
        if constexpr (i > 0) {
            SIp IP;
            rigid_body<i - 1>(M, v0, IP, unused);
            fold_inertia<i>(IC, c[i], s[i], IP);
            IC = IP;
        }
    });
}

// x = G^-1 r for an SPD G (packed lower triangle, overwritten by its Cholesky factor)
__device__ __forceinline__ void chol_solve6(float (&G)[kTri], const float (&r)[kDof], float (&x)[kDof])
{
    float inv[kDof];                                                  // 1 / L_jj
    static_for<kDof>([&](auto j_) {
        constexpr int j = decltype(j_)::value;
        float d = G[TRI<j, j>];
        static_for<j>([&](auto k_) { constexpr int k = decltype(k_)::value; d -= G[TRI<j, k>] * G[TRI<j, k>]; });
        inv[j] = __builtin_amdgcn_rsqf(d);
        static_for<kDof - 1 - j>([&](auto o_) {
            constexpr int i = j + 1 + decltype(o_)::value;
            float a = G[TRI<i, j>];
            static_for<j>([&](auto k_) { constexpr int k = decltype(k_)::value; a -= G[TRI<i, k>] * G[TRI<j, k>]; });
            G[TRI<i, j>] = a * inv[j];
        });
    });
    float y[kDof];
    static_for<kDof>([&](auto i_) {                                   // L y = r
        constexpr int i = decltype(i_)::value;
        float a = r[i];
        static_for<i>([&](auto k_) { constexpr int k = decltype(k_)::value; a -= G[TRI<i, k>] * y[k]; });
        y[i] = a * inv[i];
    });
    static_for<kDof>([&](auto t_) {                                   // L^T x = y
        constexpr int i = kDof - 1 - decltype(t_)::value;
        float a = y[i];
        static_for<kDof - 1 - i>([&](auto o_) { constexpr int k = i + 1 + decltype(o_)::value; a -= G[TRI<k, i>] * x[k]; });
        x[i] = a * inv[i];
    });
}

// qdd: in qdd_free (the constraint joints' motor torque 0), out qdd_free + M^-1 tau_S.  q, qd: the sub-step's start.
// LANE_REF (pnr_world_step_targets): a joint with from_cmd set takes its targets from the lane's r, v, as the PD law of dyn_core
// does, instead of the table's r_ref, v_ref; every other instantiation keeps the table's and never looks at r, v.
template <bool LANE_REF = false>
__device__ __forceinline__ void motor_constraints(const DynParams& D, const DynModel& M, const float (&c)[kDof], const float (&s)[kDof],
                                                  const float (&q)[kDof], const float (&qd)[kDof], const JointMotorTable& W,
                                                  float inv_h, float (&qdd)[kDof], const float* r = nullptr, const float* v = nullptr)
{
    float H[kTri];
    mass_matrix(M, c, s, H);
    const float h = D.dt_sub;
    float d[kDof], rhs[kDof], b[kDof], tcl[kDof];                    // dv of a free joint, its target, the free velocity, clamped tau
    bool in_s[kDof], fr[kDof];                                        // in S (wave-uniform), free (per lane)
#pragma unroll
    for (int i = 0; i < kDof; ++i) {
        in_s[i] = W.kind[i] != kMotorPD;
        float r_ref = W.r_ref[i], v_ref = W.v_ref[i];
        if constexpr (LANE_REF) {
            if (W.from_cmd[i]) { r_ref = r[i]; v_ref = v[i]; }
        }
        const float vp = W.kp[i] * (r_ref - q[i]) * inv_h + qd[i] + W.kd[i] * (v_ref - qd[i]);
        rhs[i] = W.kind[i] == kMotorVelocityConstraint ? v_ref : fminf(fmaxf(vp, -W.vcap[i]), W.vcap[i]);
        b[i] = qd[i] + h * qdd[i];
        d[i] = rhs[i] - b[i];
        fr[i] = in_s[i];
        tcl[i] = 0.f;
    }
    float dv[kDof];
    for (int pass = 0;; ++pass) {
        float G[kTri], r[kDof];
        static_for<kDof>([&](auto i_) {
            constexpr int i = decltype(i_)::value;
            float acc = h * tcl[i];
            static_for<kDof>([&](auto j_) {
                constexpr int j = decltype(j_)::value;
                if constexpr (j <= i) G[TRI<i, j>] = (fr[i] || fr[j]) ? (i == j ? 1.f : 0.f) : H[TRI<i, j>];
                acc -= fr[j] ? H[TRI<i, j>] * d[j] : 0.f;
            });
            r[i] = fr[i] ? d[i] : acc;
        });
        chol_solve6(G, r, dv);
        bool changed = false;
        static_for<kDof>([&](auto i_) {
            constexpr int i = decltype(i_)::value;
            if (in_s[i]) {
                float ht = 0.f;                                       // h tau_i = (M dv)_i
                static_for<kDof>([&](auto j_) { constexpr int j = decltype(j_)::value; ht += H[TRI<i, j>] * dv[j]; });
                const float vn = b[i] + dv[i];
                if (fr[i]) {
                    if (fabsf(ht) > h * W.tcap[i]) { fr[i] = false; tcl[i] = ht > 0.f ? W.tcap[i] : -W.tcap[i]; changed = true; }
                } else if (tcl[i] > 0.f ? vn > rhs[i] : vn < rhs[i]) {
                    fr[i] = true; changed = true;
                }
            }
        });
        if (!changed || pass == kMotorPasses - 1) break;
    }
#pragma unroll
    for (int i = 0; i < kDof; ++i) qdd[i] += dv[i] * inv_h;
}

// `in` carries the pointers and integrator constants the kernel received as preloaded leading arguments
// (so that the first loads and the integrator do not wait for the kernarg structs).
struct DynLead {
    const float4* state; const float* dyn; const float* actions;
    long long n; double dt, eps; float max_v_to_r;
};

// What a phase-A lane keeps in registers for its env across the steps of one launch.
struct DynLane {
    float a[kDof], v[kDof], r[kDof];            // the kinematic command state
    float q[kDof], qd[kDof];                    // the simulated joints
    float sc[kNumLinks], fric[kDof], damp[kDof];
    float cw[2][3];                             // the env's common words as loaded (target | potential, step, episode):
                                                // passed on to phase B with the first hand-off, not used after it
    float act[kDof];                            // the action of the NEXT advance, requested one step ahead
};

// All phase-A addresses are formed as (wave-uniform plane pointer incl. the workgroup's first env) + lane: the
// uniform part is scalar arithmetic and the loads take the SGPR-base + 32-bit-offset form.  Written as
// `ptr[i * n + e]` with a 64-bit per-lane `e`, the 40-odd plane addresses became v_mad_u64_u32 chains whose
// temporaries overlapped load destinations, so the compiler split the load burst with s_waitcnt vmcnt(0) —
// one more memory round trip per split before the first sub-step.
template <bool ACT_EM>
__device__ __forceinline__ void dyn_load_action(const float* __restrict__ actions, long long n, long long base, int lane,
                                                float (&act)[kDof])
{
    if (ACT_EM) {
        const float2* a2 = reinterpret_cast<const float2*>(actions + base * kDof);
        const float2 x0 = a2[3 * lane], x1 = a2[3 * lane + 1], x2 = a2[3 * lane + 2];
        act[0] = x0.x; act[1] = x0.y; act[2] = x1.x; act[3] = x1.y; act[4] = x2.x; act[5] = x2.y;
    } else {
#pragma unroll
        for (int i = 0; i < kDof; ++i) act[i] = (actions + (long long)i * n + base)[lane];
    }
}

// RAND = per-env link scales (domain randomisation): loaded from the dyn words; otherwise every scale
// is 1 and the model folds into literals.  Every load of the kernel is issued here, before the first wait.
template <bool ACT_EM, bool RAND>
__device__ __forceinline__ void dyn_lane_load(const DynLead& in, long long base, int lane, DynLane& L)
{
    const long long n = in.n;
    HalfRec k[2];
    load_env_halves(in.state, n, base, lane, k);                  // (the workgroup's first env in the uniform part of the addresses)
    // the 35 planar dyn words through ONE walking pointer (plane p at dyn + p * n): two address registers in all
    const float* w = in.dyn + base + lane;
#pragma unroll
    for (int i = 0; i < kDof; ++i) { L.q[i] = *w; w += n; }
#pragma unroll
    for (int i = 0; i < kDof; ++i) { L.qd[i] = *w; w += n; }
#pragma unroll
    for (int l = 0; l < kNumLinks; ++l) { L.sc[l] = RAND ? *w : 1.0f; w += n; }
#pragma unroll
    for (int i = 0; i < kDof; ++i) { L.fric[i] = *w; w += n; }
#pragma unroll
    for (int i = 0; i < kDof; ++i) { L.damp[i] = *w; w += n; }
    dyn_load_action<ACT_EM>(in.actions, n, base, lane, L.act);   // the first step's action, with everything else
#pragma unroll
    for (int p = 0; p < 2; ++p) unpack_record(k[p], L.a + 3 * p, L.v + 3 * p, L.r + 3 * p, L.cw[p]);
}

// One joint's motor law, for the env step, the world step and pnr_get_joint_states alike: the torque before the caller's joint
// torque, damping and friction.  SCALED (PHYS bit 1): the law is an acceleration request instead, handed out in ades and scaled
// and capped inside the ABA; the torque is then 0.
template <bool SCALED>
__device__ __forceinline__ float motor_law(float rr, float vr, float q, float qd, float kp, float kd, float cpos, float vcap, float tcap,
                                           float& ades)
{
    const float dq = rr - q;
    const float v_ask = fminf(fmaxf(vr + cpos * dq, -vcap), vcap);
    float tq = kp * dq + kd * (v_ask - qd);
    if constexpr (SCALED) { ades = tq; tq = 0.f; }
    else { ades = 0.f; tq = fminf(fmaxf(tq, -tcap), tcap); }
    return tq;
}

// The world step's options (dyn_core's FORM, dyn_world_kernel's) ..
enum : int {
    kWorld = 1,
    kWorldCMotor = 2,    // W holds constraint motors as well: motor_constraints adds their boxed solve to each sub-step's accelerations
    kWorldTorque = 4,    // pnr_world_step_torques: tau_ext, the caller's joint torques of this call, are added to each joint's torque in
                         // every sub-step, after the motor law's own cap and before damping and friction (PyBullet's TORQUE_CONTROL)
    kWorldWrench = 8,    // pnr_world_step_wrenches: the lane's link wrench records XL under the table X; converted once at the call's
                         // first pose, they give each of the first X.hold sub-steps its fext (a wave-uniform compare on the loop counter)
    kWorldTargets = 16,  // pnr_world_step_targets: the caller has put the env's own targets into the lane's r, v for the from_cmd joints.
                         // The PD law tracks those anyway; a constraint joint with from_cmd set does so only here
    kWorldBody = 32,     // pnr_set_body_params: the env's moving sphere (SphereLane, under the params of WorldBody) is integrated with the
                         // joints: in every sub-step the static world's and the arm samples' forces on it, the samples' reactions in fext
    kWorldGrip = 64,     // pnr_set_body_grip_params, with kWorldBody only: the lane's max_force (GripLane::g) > 0 holds the sphere at the
                         // pointer's anchor point (grip_force) and switches the arm samples' contact with it off; the last sub-step's
                         // force is stored inside that sub-step (a wave-uniform compare on the loop counter)
};
// .. and its operands: an option's are read only where the option is set.  The joint torques are an argument of their own (dyn_core's
// tau_ext): with the array's address kept in a struct, the kernel's zero fill of it stops being promoted as one vector, the `0 + tau`
// of the inertia-scaled law is folded into the null-pointer branch, and the targets form with PD motors and PHYS 3 goes from 256
// VGPRs / 0 AGPRs / two waves per SIMD to 256 / 2 / one.
struct WorldOperands {
    const JointMotorTable& W;
    const LinkWrenchTable* X;      // null without kWorldWrench
    WrenchLane& XL;
};

// The arithmetic of phase A, shared by the single-step and the rollout kernels (one text, so that both produce
// the same bits): command integration with the action latched for the next step, then nsub sub-steps of ABA + PD.
// FORM: 0 as above (pnr_step, pnr_rollout), or kWorld with the world step's options (pnr_world_step*, World.step): the sub-steps
// alone — no command integration, no teleport — with the operands `world` refers to.
// `env`: the lane's env index, read by the kWorldGrip forms alone (the address of the grip's report).
template <int PHYS, int FORM = 0>
__device__ __forceinline__ void dyn_core(const DynLead& in, const DynParams& D, float (&a)[kDof], float (&v)[kDof],
                                         float (&r)[kDof], float (&q)[kDof], float (&qd)[kDof], const float (&sc)[kNumLinks],
                                         const float (&fric_)[kDof], const float (&damp_)[kDof], const float (&act)[kDof],
                                         const WorldOperands* world = nullptr, const float* tau_ext = nullptr,
                                         const WorldBody* body = nullptr, SphereLane* sphere = nullptr, long long env = 0)
{
    constexpr bool WORLD = (FORM & kWorld) != 0, CMOTOR = (FORM & kWorldCMotor) != 0, TORQUE = (FORM & kWorldTorque) != 0,
                   WRENCH = (FORM & kWorldWrench) != 0, TARGETS = (FORM & kWorldTargets) != 0, BODY = (FORM & kWorldBody) != 0,
                   GRIP = (FORM & kWorldGrip) != 0;
    static_assert(!GRIP || BODY, "the grip holds the moving sphere");
    static_assert(WORLD ? !(CMOTOR && (TORQUE || WRENCH)) : FORM == 0, "the options are the world step's; torque or wrench input with the boxed solve is not built");
    static_assert(!BODY || (TORQUE && !WRENCH && !CMOTOR && (PHYS & 1)), "the sphere is built into the torque forms, with contacts");
    if constexpr (!WORLD) {
#pragma unroll
    for (int i = 0; i < kDof; ++i) {
        integrate_joint(a[i], v[i], r[i], in.max_v_to_r * (limit_hi(i) - limit_lo(i)), limit_lo(i), limit_hi(i),
                        in.dt, in.eps, v[i], r[i]);
        a[i] = act[i];
    }
    }

    DynModel M;
    build_model(sc, M);
    // the copies stay: with the loop reading the caller's arrays, the register allocation of dyn_rollout_kernel<0,1,1,0> moved (270 -> 268 VGPRs)
    float fric[kDof], damp[kDof];
#pragma unroll
    for (int i = 0; i < kDof; ++i) { fric[i] = fric_[i]; damp[i] = damp_[i]; }

    if (!WORLD && D.teleport) {   // resetJointState semantics: pioneer_knm_env.py:148, bullet_scene.py:157-165
#pragma unroll
        for (int i = 0; i < kDof; ++i) { q[i] = r[i]; qd[i] = 0.f; }
    }
    // wave-uniform options folded into the arithmetic once, so the sub-step loop carries no branches:
    // teleport = no motor torque (gains 0), no torque cap = cap at +inf
    const float kp = D.teleport ? 0.f : D.kp_eff, kd = D.teleport ? 0.f : D.kd;
    const float cpos = D.c_pos, vcap = D.v_cap;            // 0 and +inf for the plain PD motor: v_ask == v[i] exactly
    const float tcap = D.tau_max > 0.f ? D.tau_max : __builtin_inff();
    // cos / sin of the joint angles: evaluated once per step and then ROTATED by each sub-step's actual angle change
    // (|dq| = |qd| / 240 is normally a few hundredths of a radian; sin / cos of it by Taylor polynomials to dq^11 / dq^12:
    // exact to float32 up to |dq| = 1.3 — the parity suite's wildest transient spins at 265 rad/s = 1.1 rad per sub-step,
    // and polynomials two terms shorter left 7e-6 there, which that trajectory amplified to 1.4e-3 rad), as (c, s) pairs in
    // packed registers: ~10 instructions per joint and sub-step instead of the ~35 of a range-reduced sincos.
    // Ten rotations drift the pair's norm by < 1e-6, and the next step starts from the exact values again.
    f2 cs[kDof];
#pragma unroll
    for (int i = 0; i < kDof; ++i) { float sn, cn; sincos_bounded(q[i], sn, cn); cs[i] = (f2){cn, sn}; }
    [[maybe_unused]] const float inv_h = CMOTOR ? 1.0f / D.dt_sub : 0.f;
    [[maybe_unused]] float inv_m = 0.f;
    if constexpr (BODY) inv_m = sphere->m > 0.f ? 1.0f / sphere->m : 0.f;
    if constexpr (WRENCH) {
        float c[kDof], s[kDof];
#pragma unroll
        for (int i = 0; i < kDof; ++i) { c[i] = cs[i].x; s[i] = cs[i].y; }
        wrench_prepare(*world->X, c, s, world->XL);
    }
    for (int k = 0; k < D.nsub; ++k) {
        float tau[kDof], qdd[kDof], ades[kDof], tc[kDof];
#pragma unroll
        for (int i = 0; i < kDof; ++i) {
            // WORLD: the joint's own motor (wave-uniform table entries), which may track a reference of its own instead of the env's
            // command state
            const bool cmd = !WORLD || world->W.from_cmd[i];
            const float rr = cmd ? r[i] : world->W.r_ref[i], vr = cmd ? v[i] : world->W.v_ref[i];
            const float kpi = WORLD ? world->W.kp[i] : kp, kdi = WORLD ? world->W.kd[i] : kd;
            const float cpi = WORLD ? world->W.cpos[i] : cpos, vci = WORLD ? world->W.vcap[i] : vcap;
            tc[i] = WORLD ? world->W.tcap[i] : tcap;
            float tq = motor_law<(PHYS & 2) != 0>(rr, vr, q[i], qd[i], kpi, kdi, cpi, vci, tc[i], ades[i]);
            if constexpr (CMOTOR) {
                if (world->W.kind[i] != kMotorPD) { ades[i] = 0.f; tq = 0.f; }
            }
            if constexpr (TORQUE) tq += tau_ext[i];
            tq -= damp[i] * qd[i];
            tq -= fric[i] * qd[i] * __builtin_amdgcn_rsqf(qd[i] * qd[i] + kFrictionEps * kFrictionEps);
            tau[i] = tq;
        }
        {
            float c[kDof], s[kDof];
#pragma unroll
            for (int i = 0; i < kDof; ++i) { c[i] = cs[i].x; s[i] = cs[i].y; }
            if constexpr (BODY) {      // every force at the state the sub-step starts from, then the sphere's own step
                sphere_static(D, *body, *sphere);
                aba<PHYS, false, GRIP ? kSphereGrip : kSphereFree>(D, M, c, s, qd, tau, ades, tc, qdd, nullptr, body, sphere);
                if constexpr (GRIP) {  // the report (getConstraintState): the call's last sub-step's force, by held lanes
                    const GripLane& GL = *static_cast<const GripLane*>(sphere);
                    if (k == D.nsub - 1 && GL.g > 0.f && GL.m > 0.f) {
                        float* gw = static_cast<const WorldGrip*>(body)->grip + env;
                        gw[in.n] = GL.G.x; gw[2 * in.n] = GL.G.y; gw[3 * in.n] = GL.G.z;
                    }
                }
                sphere_integrate(D, *body, inv_m, *sphere);
            } else
            if constexpr (WRENCH) {
                P3 fx[kDof];
                if (k < world->X->hold) wrench_forces(*world->X, c, s, world->XL, fx);
                else {
#pragma unroll
                    for (int i = 0; i < kDof; ++i) fx[i] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
                }
                aba<PHYS, true>(D, M, c, s, qd, tau, ades, tc, qdd, fx);
            } else aba<PHYS>(D, M, c, s, qd, tau, ades, tc, qdd);
            if constexpr (CMOTOR) motor_constraints<TARGETS>(D, M, c, s, q, qd, world->W, inv_h, qdd, r, v);
        }
#pragma unroll
        for (int i = 0; i < kDof; ++i) {   // semi-implicit Euler + inelastic joint limits (selects, no branches)
            const float hi = limit_hi(i), lo = limit_lo(i);
            const float qdn = qd[i] + qdd[i] * D.dt_sub;
            const float qn = q[i] + qdn * D.dt_sub;
            const bool over = qn > hi, under = qn < lo;
            const float qnew = over ? hi : (under ? lo : qn);
            const float dq = qnew - q[i];                          // the angle actually turned (clamps included)
            q[i] = qnew;
            qd[i] = ((over && qdn > 0.f) || (under && qdn < 0.f)) ? 0.f : qdn;
            // (cd, sd) = (cos dq, sin dq) as one packed Horner chain in x = dq^2, then (c, s) <- cd (c, s) + sd (-s, c)
            const float x = dq * dq;
            f2 p = (f2){1.0f / 479001600.0f, -1.0f / 39916800.0f};
            p = p * x + (f2){-1.0f / 3628800.0f, 1.0f / 362880.0f};
            p = p * x + (f2){1.0f / 40320.0f, -1.0f / 5040.0f};
            p = p * x + (f2){-1.0f / 720.0f, 1.0f / 120.0f};
            p = p * x + (f2){1.0f / 24.0f, -1.0f / 6.0f};
            p = p * x + (f2){-0.5f, 1.0f};
            const float cd = p.x * x + 1.0f, sd = p.y * dq;
            const f2 rot = (f2){-cs[i].y, cs[i].x};
            cs[i] = cs[i] * cd + rot * sd;
        }
    }
}

template <bool ACT_EM, bool RAND, int PHYS>
__device__ __forceinline__ void dyn_lane_advance(const DynLead& in, const DynParams& D, long long base, int lane,
                                                 const float* __restrict__ next_actions, DynLane& L)
{
    float act[kDof];
#pragma unroll
    for (int i = 0; i < kDof; ++i) act[i] = L.act[i];
    // the action after this one is requested now: it arrives under the sub-steps (next_actions: null on the last step)
    if (next_actions) dyn_load_action<ACT_EM>(next_actions, in.n, base, lane, L.act);
    dyn_core<PHYS>(in, D, L.a, L.v, L.r, L.q, L.qd, L.sc, L.fric, L.damp, act);
}

// The per-env parameter draws of a reset: Philox blocks 3..8 of the env's counter (the joints and the target
// use blocks 0..2, reset_env), 11 link-mass scales, 6 friction and 6 damping coefficients; the configured
// defaults without randomisation.
__device__ __forceinline__ void dyn_draw_params(const KParams& P, const DynParams& D, unsigned long long genv,
                                                uint32_t episode_drawn, float (&sc)[kNumLinks], float (&fric)[kDof],
                                                float (&damp)[kDof])
{
    float u[24] = {};
    if (D.randomize) {
#pragma unroll
        for (uint32_t b = 0; b < 6; ++b) {
            uint32_t o[4];
            philox4x32_10(episode_drawn, (uint32_t)genv, (uint32_t)(genv >> 32), 3 + b, P.seed_lo, P.seed_hi, o);
#pragma unroll
            for (int k = 0; k < 4; ++k) u[4 * b + k] = (float)u01(o[k]);
        }
    }
#pragma unroll
    for (int l = 0; l < kNumLinks; ++l) sc[l] = D.randomize ? (float)(D.mass_lo + D.mass_span * (double)u[l]) : 1.0f;
#pragma unroll
    for (int j = 0; j < kDof; ++j) {
        fric[j] = D.randomize ? (float)(D.fric_lo + D.fric_span * (double)u[11 + j]) : D.joint_friction;
        damp[j] = D.randomize ? (float)(D.damp_lo + D.damp_span * (double)u[17 + j]) : D.joint_damping;
    }
}

// ---------------------------------------------------------------------------------
// Single-step form of phase A (pnr_step): load, dyn_core, in one piece.  Kept next to the rollout
// kernel's dyn_lane_load + dyn_lane_advance: that split form has the same instruction counts but ran 2 % slower as
// the single-step kernel (A/B inside one library: 32.15 vs 32.85 us per 65 536-env step; SQ_WAIT_INST_ANY +40 %).
// In: nothing but the env index.  Out: the env's two state records as they lie in HBM (a, v, r updated), q, qd.
// ---------------------------------------------------------------------------------
template <bool ACT_EM, bool RAND, int PHYS>
__device__ __forceinline__ void dyn_substeps_lane(const DynLead& in, const DynParams& D, long long e, HalfRec (&k)[2],
                                                  float (&q)[kDof], float (&qd)[kDof])
{
    const long long n = in.n;
    load_env_halves(in.state, n, e, 0, k);
    // dynamics state: every load is issued here, before the first wait — with one wave per SIMD
    // (65 536 envs) nothing else hides a memory round trip
    float sc[kNumLinks], fric[kDof], damp[kDof];
#pragma unroll
    for (int i = 0; i < kDof; ++i) {
        q[i] = in.dyn[(long long)(kDynQ + i) * n + e]; qd[i] = in.dyn[(long long)(kDynQd + i) * n + e];
        fric[i] = in.dyn[(long long)(kDynFric + i) * n + e]; damp[i] = in.dyn[(long long)(kDynDamp + i) * n + e];
    }
#pragma unroll
    for (int l = 0; l < kNumLinks; ++l) sc[l] = RAND ? in.dyn[(long long)(kDynScale + l) * n + e] : 1.0f;
    float a[kDof], v[kDof], r[kDof];
#pragma unroll
    for (int p = 0; p < 2; ++p) unpack_record(k[p], a + 3 * p, v + 3 * p, r + 3 * p);
    float act[kDof];
    if (ACT_EM) {
        const float2* a2 = reinterpret_cast<const float2*>(in.actions + e * kDof);
        const float2 x0 = a2[0], x1 = a2[1], x2 = a2[2];
        act[0] = x0.x; act[1] = x0.y; act[2] = x1.x; act[3] = x1.y; act[4] = x2.x; act[5] = x2.y;
    } else {
#pragma unroll
        for (int i = 0; i < kDof; ++i) act[i] = in.actions[(long long)i * n + e];
    }
    dyn_core<PHYS>(in, D, a, v, r, q, qd, sc, fric, damp, act);
#pragma unroll
    for (int p = 0; p < 2; ++p) k[p] = pack_record(a + 3 * p, v + 3 * p, r + 3 * p, k[p].p2.y, k[p].p2.z, k[p].p2.w);
}

// reset of the dynamics words for this lane's joints (called by the pair kernels after reset_env):
// q = r, qd = 0, and the per-env parameter draws (Philox blocks 3..8 of the same counter).
__device__ __forceinline__ void dyn_reset_lane(const KParams& P, const DynParams& D, const LaneState& s, int p,
                                               long long e, unsigned long long genv, uint32_t episode_drawn)
{
    const long long n = P.n;
#pragma unroll
    for (int i = 0; i < kJpl; ++i) {
        D.dyn[(long long)(kJpl * p + i) * n + e] = s.r[i];
        D.dyn[(long long)(kDynQd + kJpl * p + i) * n + e] = 0.f;
    }
    float sc[kNumLinks], fric[kDof], damp[kDof];
    dyn_draw_params(P, D, genv, episode_drawn, sc, fric, damp);
    // lane 0 writes the link scales, each lane its own joints' friction / damping
    if (p == 0) {
#pragma unroll
        for (int l = 0; l < kNumLinks; ++l) D.dyn[(long long)(kDynScale + l) * n + e] = sc[l];
    }
#pragma unroll
    for (int i = 0; i < kJpl; ++i) {
        const int j = kJpl * p + i;
        // both candidates become plain register values first: left as `p ? x[a] : x[b]`, LLVM folds the
        // select into the address and the whole array is demoted to scratch (cf. lane_consts)
        float f0 = fric[i], f1 = fric[kJpl + i], d0 = damp[i], d1 = damp[kJpl + i];
        asm volatile("" : "+v"(f0), "+v"(f1), "+v"(d0), "+v"(d1));
        D.dyn[(long long)(kDynFric + j) * n + e] = p ? f1 : f0;
        D.dyn[(long long)(kDynDamp + j) * n + e] = p ? d1 : d0;
    }
}

}  // namespace pnr

#pragma clang fp contract(off)
