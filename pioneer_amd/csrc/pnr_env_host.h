// pnr_env_host.h — host-side pieces that both of the env engine's translation units need (pnr_api.hip: the core, every step and
// world-step kernel; pnr_queries.hip: the query entry points): the handle, the error call, small argument helpers, the flag ->
// template-argument dispatch, the static scene bodies and the world step's table builders (which pnr_get_joint_states shares).  Nothing here is exported, and pnr_learn.hip does not include it (a
// handle is opaque to the learner).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <type_traits>

#include "../../include/pioneer_amd.h"
#include "pnr_host.h"
#include "pnr_device.h"
#include "pnr_dyn.h"

struct pnr_env_s {
    pnr_config cfg;
    pnr_constants k;
    pnr::KParams base;        // constants pre-filled; pointers set per call
    pnr::DynParams dbase;     // dynamics-mode constants (zeroed in kinematic mode)
    pnr::JointMotorTable motors;   // pnr_world_step's per-joint motors (pnr_set_joint_motor); fill_base: every joint on the handle's own law
    long long n;
    unsigned long long env_off;
    int device;
    float4* state;
    float* dyn;          // dynamics-mode planar words [36][n] or null
    pnr::SceneBody* scene;    // dynamics-mode static scene bodies [kMaxScene] or null
    pnr::WorldGrip sphere;    // pnr_set_body_params: the moving sphere's buffer (words; null before the first call) and resolved params;
                              // pnr_set_body_grip_params: the grip's buffer (grip; null before the first call) and resolved params
    bool sphere_on;           // .. and whether the world step moves it (the kWorldBody forms)
    bool grip_on;             // pnr_set_body_grip_params: the grip is enabled (the kWorldGrip forms; its buffer and operands are in `sphere`)
    unsigned body_queries;    // pnr_set_body_queries: which scene queries see the sphere (0: none), a host-side switch
    bool body_rgb_set;        // .. and its drawn colour, once the caller gave one (else the obstacle material's grey)
    float body_rgb[3];
    int diag;            // -DPNR_DIAG_BUILD=1 variant only: the PNR_DIAG environment variable at create time; else 0
    bool ready;          // a full reset has happened, or the state was set explicitly
    bool kin_set, dyn_set;  // pnr_set_state / pnr_set_dyn_state seen (both needed in dynamics mode)
    char err[512];
};

// records the message in the handle (h == nullptr: in the thread's buffer) and returns `code`; defined in pnr_api.hip on pnr_failv
__attribute__((visibility("hidden"))) int fail(pnr_handle h, int code, const char* fmt, ...);

static inline bool aligned_to(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

// a call's pointer arguments against their alignment, in the order given (a null pointer passes); `call` names it in the message
struct AlignedArg { const void* p; const char* name; unsigned align; };
static int check_aligned(pnr_handle h, const char* call, std::initializer_list<AlignedArg> args)
{
    for (const AlignedArg& a : args)
        if (!aligned_to(a.p, a.align)) return fail(h, PNR_ERR_INVALID, "%s: %s must be %u-byte aligned", call, a.name, a.align);
    return PNR_OK;
}

// a constraint motor anywhere in the handle's table (the kernels' instantiation with motor_constraints); *joint: the first such joint
static inline bool has_constraint_motor(pnr_handle h, int* joint = nullptr)
{
    for (int i = 0; i < pnr::kDof; ++i)
        if (h->motors.kind[i] != pnr::kMotorPD) { if (joint) *joint = i; return true; }
    return false;
}

template <class T>
static bool finite_all(const T* v, int k)
{
    for (int i = 0; i < k; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

static double sum_sq(const double* v, int k)      // v[0]^2 + v[1]^2 + .. in that order
{
    double s = 0;
    for (int i = 0; i < k; ++i) s += v[i] * v[i];
    return s;
}

// Runtime flags -> template arguments: f is called with a std::integral_constant whose value is `b` (or `v`, which must be one of
// Vs: only the listed values are instantiated).  Every kernel launch of the env units is written once inside such a call.
template <class F>
static inline void with_bool(bool b, F&& f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
template <int... Vs, class F>
static inline void with_int(int v, F&& f) { (void)((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...); }

// One static body of the scene, checked: `who` names the call in the message, `finite` adds pnr_render's rule
static int check_scene_body(pnr_handle h, const char* who, int b, const pnr_scene_body& S, bool finite)
{
    const auto bad = [&](const char* what) { return fail(h, PNR_ERR_INVALID, "%s %d: %s", who, b, what); };
    if (S.shape != PNR_SHAPE_PLANE && S.shape != PNR_SHAPE_BOX && S.shape != PNR_SHAPE_SPHERE)
        return fail(h, PNR_ERR_INVALID, "%s %d: bad shape %d", who, b, S.shape);
    if (finite && !(finite_all(S.position, 3) && finite_all(S.orientation, 4) && finite_all(S.size, 3))) return bad("non-finite data");
    if (!(sum_sq(S.orientation, 4) > 0)) return bad("zero orientation quaternion");
    if (S.shape == PNR_SHAPE_PLANE && !(sum_sq(S.size, 3) > 0)) return bad("zero plane normal");
    if (S.shape == PNR_SHAPE_BOX && !(S.size[0] > 0 && S.size[1] > 0 && S.size[2] > 0)) return bad("box half extents must be > 0");
    if (S.shape == PNR_SHAPE_SPHERE && !(S.size[0] > 0)) return bad("sphere radius must be > 0");
    return PNR_OK;
}

// .. and its frame: the normalised quaternion as a row-major rotation R; for a plane also the unit world normal R n / |n|
static void scene_body_frame(const pnr_scene_body& S, double (&R)[9], double (&normal)[3])
{
    const double qn = std::sqrt(sum_sq(S.orientation, 4));
    const double x = S.orientation[0] / qn, y = S.orientation[1] / qn, z = S.orientation[2] / qn, w = S.orientation[3] / qn;
    const double r[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                         2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                         2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
    for (int k = 0; k < 9; ++k) R[k] = r[k];
    if (S.shape != PNR_SHAPE_PLANE) return;
    const double nl = std::sqrt(sum_sq(S.size, 3));
    for (int k = 0; k < 3; ++k) normal[k] = (R[3 * k] * S.size[0] + R[3 * k + 1] * S.size[1] + R[3 * k + 2] * S.size[2]) / nl;
}

// .. and as the kernels want it (pnr_dyn.h SceneBody): float32, pre-rotated; a plane keeps its unit world normal in rot[0..2]
static pnr::SceneBody scene_body_device(const pnr_scene_body& B)
{
    pnr::SceneBody S = pnr::SceneBody{};
    double R[9], normal[3];
    scene_body_frame(B, R, normal);
    S.shape = B.shape;
    for (int k = 0; k < 3; ++k) { S.pos[k] = (float)B.position[k]; S.size[k] = (float)B.size[k]; }
    if (B.shape == PNR_SHAPE_PLANE) {
        for (int k = 0; k < 3; ++k) S.rot[k] = (float)normal[k];
    } else {
        for (int k = 0; k < 9; ++k) S.rot[k] = (float)R[k];
    }
    return S;
}

// the dynamics kernels' PHYS template argument: bit 0 contacts (contact-free handles run instantiations without any contact
// code), bit 1 the inertia-scaled motor
// with the moving sphere enabled a world-step call with wrenches, a constraint motor, or pnr_get_joint_states is not built
static inline int refuse_sphere(pnr_handle h, const char* call, const char* what)
{
    return fail(h, PNR_ERR_UNSUPPORTED, "%s: the moving sphere is enabled (pnr_set_body_params) and %s with the sphere is not built", call, what);
}

static inline int dyn_phys(const pnr::DynParams& D) { return ((D.has_ground || D.has_box || D.n_scene > 0) ? 1 : 0) | (D.inertia_scaled ? 2 : 0); }

// pnr_world_step_wrenches' and pnr_get_joint_states' records: a table without records ..
static inline void empty_wrench_table(pnr::LinkWrenchTable& T)
{
    T = pnr::LinkWrenchTable{};
    T.last_world_body = -1;
    for (int j = 0; j < pnr::kMaxWrench; ++j) T.lbody[j] = T.wbody[j] = -1;
}

// .. and the caller's specs, checked (`call` names the entry point in the message); T.hold is the caller's to set
static int fill_wrench_table(pnr_handle h, const char* call, const pnr_link_wrench_spec* specs, int n_specs, pnr::LinkWrenchTable& T)
{
    using namespace pnr;
    if (n_specs < 1 || n_specs > PNR_MAX_LINK_WRENCHES)
        return fail(h, PNR_ERR_INVALID, "%s: n_specs %d out of [1, %d]", call, n_specs, PNR_MAX_LINK_WRENCHES);
    empty_wrench_table(T);
    T.n = n_specs;
    for (int j = 0; j < n_specs; ++j) {
        const int link = specs[j].link, frame = specs[j].frame;
        if (link < 0 || link >= kNumLinks) return fail(h, PNR_ERR_INVALID, "%s: record %d: link %d out of [0, %d)", call, j, link, kNumLinks);
        if (frame != PNR_FRAME_LINK && frame != PNR_FRAME_WORLD)
            return fail(h, PNR_ERR_INVALID, "%s: record %d: unknown frame %d (1: link, 2: world)", call, j, frame);
        (frame == PNR_FRAME_WORLD ? T.wbody : T.lbody)[j] = kLinkBody[link];   // -1: robot:base, welded to the world: the record does nothing
        if (link == kNumLinks - 1) { T.d[j][0] = (float)kTipX; T.d[j][1] = (float)kTipY; T.d[j][2] = (float)kTipZ; }   // every other link origin is its body's
        if (T.wbody[j] > T.last_world_body) T.last_world_body = T.wbody[j];
    }
    return PNR_OK;
}
