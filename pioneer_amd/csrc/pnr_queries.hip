// pnr_queries.hip — the query entry points of the C ABI (include/pioneer_amd.h) and their kernels: link states, Jacobian,
// inverse dynamics and mass matrix, joint states, the IK solvers, contacts, path clearance, time parameterisation, render, ray casts.  A query reads the handle (or the
// caller's joints) and writes the caller's buffers; it never changes an env.  The kernels are the query headers' (pnr_query.h:
// their shared scaffold); the handle and the host helpers shared with the core unit pnr_api.hip are pnr_env_host.h's.  A unit
// of its own so that a query's code object holds no step kernel and a change to one recompiles neither.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <initializer_list>

#include "../../include/pioneer_amd.h"

#include "pnr_env_host.h"
#include "pnr_links.h"
#include "pnr_render.h"
#include "pnr_ik.h"
#include "pnr_invdyn.h"
#include "pnr_jointstate.h"
#include "pnr_contacts.h"
#include "pnr_rays.h"
#include "pnr_path.h"
#include "pnr_retime.h"

using namespace pnr;

static const char g_unit_fp[] = "pnr_build_fp:queries=" PNR_UNIT_FINGERPRINT ";";
extern "C" const char* pnr_unit_fingerprint_queries(void) { return g_unit_fp; }

// One static body of the scene (pnr_env_host.h: checked, its frame) as the ray casters want it (pnr_render, pnr_ray_test): the
// world -> primitive rotation rows rt, the half sizes h and the bounding radius (a plane: rows 0 and 1 zero, row 2 its unit world normal, no bound).  Returns the kVis* shape.
static int scene_body_prim(const pnr_scene_body& S, double (&rt)[9], float (&h)[3], double& bound)
{
    double R[9], normal[3];
    scene_body_frame(S, R, normal);
    const double ident[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int k = 0; k < 9; ++k) rt[k] = ident[k];
    h[0] = h[1] = h[2] = 0.f;
    bound = 0;
    if (S.shape == PNR_SHAPE_BOX) {
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 3; ++k) rt[3 * i + k] = R[3 * k + i];
        for (int i = 0; i < 3; ++i) h[i] = (float)S.size[i];
        bound = std::sqrt(sum_sq(S.size, 3));
        return kVisBox;
    }
    if (S.shape == PNR_SHAPE_SPHERE) {
        for (int i = 0; i < 3; ++i) h[i] = (float)S.size[0];
        bound = S.size[0];
        return kVisSphere;
    }
    for (int k = 0; k < 6; ++k) rt[k] = 0;           // unit world normal R n / |n| as the frame's z row
    for (int k = 0; k < 3; ++k) rt[6 + k] = normal[k];
    return kVisPlane;
}

// whose joints a query or a render reads (pnr_query.h): the caller's buffer, else the handle's own (h->dyn; kinematic: the state)
struct JointSource { int kind; const float* src; const float4* state; };
static inline JointSource joint_source(pnr_handle h, const float* js)
{
    return js ? JointSource{kJointSrcBuffer, js, nullptr} : h->dyn ? JointSource{kJointSrcDyn, h->dyn, nullptr} : JointSource{kJointSrcKin, nullptr, h->state};
}

// one launch of a kernel of one env per lane and one wave per workgroup: kernel(S)(args...), S = the joint source `kind`
template <class K, class... Args>
static int launch_env_waves(pnr_handle h, void* stream, int kind, K&& kernel, Args... args)
{
    DeviceGuard g(h->device);
    const dim3 grid((unsigned)((h->n + kWave - 1) / kWave));
    with_int<kJointSrcBuffer, kJointSrcDyn, kJointSrcKin>(kind, [&](auto S) {
        hipLaunchKernelGGL(kernel(S), grid, dim3(kWave), 0, (hipStream_t)stream, args...);
    });
    HIP_TRY(h, hipGetLastError());
    return PNR_OK;
}

// What a query needs of the handle when the caller brings no data of its own, one predicate per rule.  They differ, and
// pnr_get_link_states' is the odd one: it takes a dynamics handle whose joints were never set.
static inline bool has_own_joints(pnr_handle h) { return h->ready || (h->dyn && h->dyn_set); }     // pnr_get_jacobian, pnr_get_contacts
static inline bool has_own_joints_or_planes(pnr_handle h) { return h->ready || h->dyn; }           // pnr_get_link_states
static inline bool has_link_scales(pnr_handle h) { return h->ready || h->dyn_set; }                // dynamics mode: drawn by the first reset
static inline bool has_own_target(pnr_handle h) { return h->ready || h->kin_set; }                 // pnr_solve_ik, pnr_render
static int before_first_reset(pnr_handle h, const char* call, const char* why = "") { return fail(h, PNR_ERR_INVALID, "%s before the first pnr_reset (or pnr_set_state)%s", call, why); }

// the handle's moving-sphere words where the query `bit` (pnr_set_body_queries) sees the sphere, else null
static inline const float* shown_sphere(pnr_handle h, unsigned bit) { return (h->body_queries & bit) ? h->sphere.words : nullptr; }

extern "C" {

int pnr_set_body_queries(pnr_handle h, uint32_t queries, const float* rgba)
{
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (h->cfg.mode != PNR_MODE_DYNAMIC)
        return fail(h, PNR_ERR_UNSUPPORTED, "pnr_set_body_queries: the moving sphere exists in dynamics mode only");
    if (!h->sphere.words) return fail(h, PNR_ERR_INVALID, "pnr_set_body_queries before pnr_set_body_params (the handle has no sphere buffer)");
    if (queries & ~(uint32_t)(PNR_BODY_IN_RENDER | PNR_BODY_IN_RAYS | PNR_BODY_IN_CONTACTS))
        return fail(h, PNR_ERR_INVALID, "pnr_set_body_queries: unknown bits in 0x%x", (unsigned)queries);
    if (rgba && !finite_all(rgba, 4)) return fail(h, PNR_ERR_INVALID, "pnr_set_body_queries: non-finite colour");
    h->body_queries = queries;
    if (rgba) {
        for (int k = 0; k < 3; ++k) h->body_rgb[k] = rgba[k];
        h->body_rgb_set = true;
    }
    return PNR_OK;
}

int pnr_get_link_states(pnr_handle h, const float* joint_state, float* out, void* stream)
{
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (!out) return fail(h, PNR_ERR_INVALID, "pnr_get_link_states: null out");
    if (const int rc = check_aligned(h, "pnr_get_link_states", {{out, "out", 16}, {joint_state, "joint_state", 16}})) return rc;
    if (!joint_state && !has_own_joints_or_planes(h)) return before_first_reset(h, "pnr_get_link_states");
    const JointSource J = joint_source(h, joint_state);
    return launch_env_waves(h, stream, J.kind, [](auto S) { return link_state_kernel<S()>; }, J.src, J.state, out, (long long)h->n);
}

// (link, local_point) -> the moving body that carries the link and the point's offset in that body's frame: every fixed joint of
// the URDF has rpy 0 and, but for effector_to_pointer (kTip), xyz 0, so a link's frame is its body's frame moved by a constant
static ChainPoint chain_point(int link, const double* local_point)
{
    double o[3] = {0, 0, 0};
    if (local_point) for (int k = 0; k < 3; ++k) o[k] = local_point[k];
    if (link == kNumLinks - 1) { o[0] += kTipX; o[1] += kTipY; o[2] += kTipZ; }
    return {kLinkBody[link], (float)o[0], (float)o[1], (float)o[2]};
}

int pnr_get_jacobian(pnr_handle h, const float* joint_state, int32_t link, const double* local_point, float* out, void* stream)
{
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (!out) return fail(h, PNR_ERR_INVALID, "pnr_get_jacobian: null out");
    if (link < 0 || link >= kNumLinks) return fail(h, PNR_ERR_INVALID, "pnr_get_jacobian: link %d outside 0..%d", link, kNumLinks - 1);
    if (local_point && !finite_all(local_point, 3)) return fail(h, PNR_ERR_INVALID, "pnr_get_jacobian: non-finite local_point");
    if (const int rc = check_aligned(h, "pnr_get_jacobian", {{out, "out", 16}, {joint_state, "joint_state", 16}})) return rc;
    if (!joint_state && !has_own_joints(h)) return before_first_reset(h, "pnr_get_jacobian");
    const JointSource J = joint_source(h, joint_state);
    return launch_env_waves(h, stream, J.kind, [](auto S) { return jacobian_kernel<S()>; }, J.src, J.state, out, (long long)h->n,
                            chain_point(link, local_point));
}

// the checks pnr_inverse_dynamics and pnr_mass_matrix share (nothing launched, nothing written on failure)
static int check_invdyn_call(pnr_handle h, const char* call, const float* joint_state, const float* joint_accel, const float* out)
{
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (!out) return fail(h, PNR_ERR_INVALID, "%s: null out", call);
    if (const int rc = check_aligned(h, call, {{out, "out", 16}, {joint_state, "joint_state", 16}, {joint_accel, "joint_accel", 16}})) return rc;
    // a dynamics-mode handle's link scales are drawn by the first reset: no model before it, whatever the joint source
    if (h->dyn ? !has_link_scales(h) : (!joint_state && !has_own_joints(h))) return before_first_reset(h, call);
    return PNR_OK;
}

int pnr_inverse_dynamics(pnr_handle h, const float* joint_state, const float* joint_accel, int32_t flags, float* out, void* stream)
{
    if (const int rc = check_invdyn_call(h, "pnr_inverse_dynamics", joint_state, joint_accel, out)) return rc;
    if (flags & ~(PNR_INVDYN_NO_GRAVITY | PNR_INVDYN_JOINT_LOSSES))
        return fail(h, PNR_ERR_INVALID, "pnr_inverse_dynamics: unknown flags 0x%x", (unsigned)flags);
    const JointSource J = joint_source(h, joint_state);
    InvDynArgs A;
    A.src = J.src; A.state = J.state;
    A.dyn = h->dyn; A.accel = joint_accel; A.out = out; A.n = h->n;
    A.gravity = (flags & PNR_INVDYN_NO_GRAVITY) ? 0.f : (float)h->cfg.gravity;
    A.loss_gain = (flags & PNR_INVDYN_JOINT_LOSSES) ? 1.f : 0.f;
    A.damping0 = (float)h->cfg.joint_damping; A.friction0 = (float)h->cfg.joint_friction;
    return launch_env_waves(h, stream, J.kind, [](auto S) { return inverse_dynamics_kernel<S()>; }, A);
}

int pnr_mass_matrix(pnr_handle h, const float* joint_state, float* out, void* stream)
{
    if (const int rc = check_invdyn_call(h, "pnr_mass_matrix", joint_state, nullptr, out)) return rc;
    const JointSource J = joint_source(h, joint_state);
    return launch_env_waves(h, stream, J.kind, [](auto S) { return mass_matrix_kernel<S()>; }, J.src, J.state, (const float*)h->dyn, out,
                            (long long)h->n);
}

int pnr_get_joint_states(pnr_handle h, const float* joint_state, const float* joint_torques, const pnr_link_wrench_spec* specs,
                         int32_t n_specs, const float* wrenches, float* joints_out, float* reaction_out, void* stream)
{
    const char* call = "pnr_get_joint_states";
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (h->cfg.mode != PNR_MODE_DYNAMIC)
        return fail(h, PNR_ERR_UNSUPPORTED, "%s: motor torques, accelerations and reactions exist in dynamics mode only", call);
    if (!joints_out) return fail(h, PNR_ERR_INVALID, "%s: null joints_out", call);
    if (const int rc = check_aligned(h, call, {{joints_out, "joints_out", 16}, {reaction_out, "reaction_out", 16}, {joint_state, "joint_state", 16},
                                               {joint_torques, "joint_torques", 16}, {wrenches, "wrenches", 16}})) return rc;
    LinkWrenchTable T;
    if (n_specs == 0) {
        if (specs || wrenches) return fail(h, PNR_ERR_INVALID, "%s: n_specs 0 goes with NULL specs and NULL wrenches", call);
        empty_wrench_table(T);
    } else {
        if (!specs) return fail(h, PNR_ERR_INVALID, "%s: null specs", call);
        if (!wrenches) return fail(h, PNR_ERR_INVALID, "%s: null wrenches", call);
        if (const int rc = fill_wrench_table(h, call, specs, n_specs, T)) return rc;
    }
    if (!h->ready) return before_first_reset(h, call);
    const bool cm = has_constraint_motor(h);
    const bool ext = joint_torques || n_specs > 0;
    if (cm && ext)
        return fail(h, PNR_ERR_UNSUPPORTED, "%s: a joint is on a constraint motor (torque or wrench input with the boxed solve is not built)", call);
    if (h->sphere_on) return refuse_sphere(h, call, "the joint states");
    T.hold = 1;                                        // (one sub-step is looked at: the records act in it)
    JointStateArgs A;
    A.joints_in = joint_state; A.state = h->state; A.dyn = h->dyn;
    A.tau_ext = joint_torques; A.wrenches = wrenches;
    A.joints = joints_out; A.reaction = reaction_out; A.n = h->n;
    DeviceGuard g(h->device);
    const DynParams& D = h->dbase;
    const dim3 grid((unsigned)((h->n + kWave - 1) / kWave));
    // the world step's own distinctions: contacts / inertia-scaled (dyn_phys), constraint motors, external inputs present or not
    with_int<0, 1, 2, 3>(dyn_phys(D), [&](auto C) {
        with_int<0, 1, 2>(cm ? 2 : (ext ? 1 : 0), [&](auto K) {
            hipLaunchKernelGGL((joint_state_kernel<C(), K() == 2, K() == 1>), grid, dim3(kWave), 0, (hipStream_t)stream, A, D, h->motors, T);
        });
    });
    HIP_TRY(h, hipGetLastError());
    return PNR_OK;
}

int pnr_ik_params_default(pnr_ik_params* p)
{
    if (!p) return fail(nullptr, PNR_ERR_INVALID, "pnr_ik_params_default: null params");
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(pnr_ik_params);
    p->link = kNumLinks - 1;
    p->max_iterations = 32;
    p->damping = 1.0;
    p->max_step = 0.5;
    p->tolerance = 1e-3;
    return PNR_OK;
}

int pnr_solve_ik(pnr_handle h, const pnr_ik_params* p, const float* target_pos, const float* q_init,
                 float* q_out, float* residual_out, int32_t* iterations_out, void* stream)
{
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (!p) return fail(h, PNR_ERR_INVALID, "pnr_solve_ik: null params");
    if (!q_out) return fail(h, PNR_ERR_INVALID, "pnr_solve_ik: null q_out");
    if (p->struct_size != sizeof(pnr_ik_params))
        return fail(h, PNR_ERR_INVALID, "pnr_solve_ik: params struct_size %u, want %zu", p->struct_size, sizeof(pnr_ik_params));
    if (p->link < 0 || p->link >= kNumLinks) return fail(h, PNR_ERR_INVALID, "pnr_solve_ik: link %d outside 0..%d", p->link, kNumLinks - 1);
    if (p->max_iterations < 1 || p->max_iterations > 1024)
        return fail(h, PNR_ERR_INVALID, "pnr_solve_ik: max_iterations %d outside 1..1024", p->max_iterations);
    if (!(std::isfinite(p->damping) && p->damping > 0)) return fail(h, PNR_ERR_INVALID, "pnr_solve_ik: damping must be finite and > 0");
    if (!(std::isfinite(p->max_step) && p->max_step > 0)) return fail(h, PNR_ERR_INVALID, "pnr_solve_ik: max_step must be finite and > 0");
    if (!(std::isfinite(p->tolerance) && p->tolerance >= 0)) return fail(h, PNR_ERR_INVALID, "pnr_solve_ik: tolerance must be finite and >= 0");
    if (!finite_all(p->local_point, 3)) return fail(h, PNR_ERR_INVALID, "pnr_solve_ik: non-finite local_point");
    if (const int rc = check_aligned(h, "pnr_solve_ik", {{q_out, "q_out", 8}, {target_pos, "target_pos", 4}, {q_init, "q_init", 4},
                                                          {residual_out, "residual_out", 4}, {iterations_out, "iterations_out", 4}})) return rc;
    if (!target_pos && !has_own_target(h)) return before_first_reset(h, "pnr_solve_ik", ": the target comes from the state");
    IkArgs A;
    A.target = target_pos; A.state = h->state; A.q_init = q_init;
    A.q_out = q_out; A.residual = residual_out; A.iterations = iterations_out;
    A.n = h->n;
    A.point = chain_point(p->link, p->local_point);
    A.max_iter = p->max_iterations;
    A.lambda2 = (float)(p->damping * p->damping); A.max_step = (float)p->max_step; A.tol = (float)p->tolerance;
    return launch_env_waves(h, stream, kJointSrcBuffer, [](auto) { return ik_kernel; }, A);      // (no joint source: one form)
}

int pnr_ik_pose_params_default(pnr_ik_pose_params* p)
{
    if (!p) return fail(nullptr, PNR_ERR_INVALID, "pnr_ik_pose_params_default: null params");
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(pnr_ik_pose_params);
    p->link = kNumLinks - 1;
    p->max_iterations = 32;
    p->mode = PNR_IK_ORIENT_FULL;
    p->local_axis[0] = 1.0;
    p->damping = 0.03;
    p->error_damping = 0.01;
    p->orientation_weight = 10.0;
    p->max_step = 0.5;
    p->tolerance = 1e-3;
    p->angle_tolerance = 1e-3;
    return PNR_OK;
}

int pnr_solve_ik_pose(pnr_handle h, const pnr_ik_pose_params* p, const float* target_pos, const float* target_quat, const float* q_init,
                      float* q_out, float* residual_out, float* angle_out, int32_t* iterations_out, void* stream)
{
    const char* call = "pnr_solve_ik_pose";
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (!p) return fail(h, PNR_ERR_INVALID, "%s: null params", call);
    if (!q_out) return fail(h, PNR_ERR_INVALID, "%s: null q_out", call);
    if (!target_quat) return fail(h, PNR_ERR_INVALID, "%s: null target_quat", call);
    if (p->struct_size != sizeof(pnr_ik_pose_params))
        return fail(h, PNR_ERR_INVALID, "%s: params struct_size %u, want %zu", call, p->struct_size, sizeof(pnr_ik_pose_params));
    if (p->link < 0 || p->link >= kNumLinks) return fail(h, PNR_ERR_INVALID, "%s: link %d outside 0..%d", call, p->link, kNumLinks - 1);
    if (p->mode != PNR_IK_ORIENT_FULL && p->mode != PNR_IK_ORIENT_AXIS)
        return fail(h, PNR_ERR_INVALID, "%s: mode %d outside {0, 1} (full orientation, one axis)", call, p->mode);
    if (p->max_iterations < 1 || p->max_iterations > 1024)
        return fail(h, PNR_ERR_INVALID, "%s: max_iterations %d outside 1..1024", call, p->max_iterations);
    const struct { double v; const char* name; bool zero_ok; } scalars[] = {
        {p->damping, "damping", false}, {p->max_step, "max_step", false}, {p->orientation_weight, "orientation_weight", false},
        {p->error_damping, "error_damping", true}, {p->tolerance, "tolerance", true}, {p->angle_tolerance, "angle_tolerance", true}};
    for (const auto& s : scalars)
        if (!(std::isfinite(s.v) && (s.zero_ok ? s.v >= 0 : s.v > 0)))
            return fail(h, PNR_ERR_INVALID, "%s: %s must be finite and %s 0", call, s.name, s.zero_ok ? ">=" : ">");
    if (!finite_all(p->local_point, 3)) return fail(h, PNR_ERR_INVALID, "%s: non-finite local_point", call);
    const double* ax = p->local_axis;
    const double axis_len = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
    if (!finite_all(ax, 3) || !std::isfinite(axis_len) || !(axis_len > 0))
        return fail(h, PNR_ERR_INVALID, "%s: local_axis must be finite and not zero", call);
    if (const int rc = check_aligned(h, call, {{q_out, "q_out", 8}, {target_pos, "target_pos", 4}, {target_quat, "target_quat", 4},
                                               {q_init, "q_init", 4}, {residual_out, "residual_out", 4}, {angle_out, "angle_out", 4},
                                               {iterations_out, "iterations_out", 4}})) return rc;
    if (!target_pos && !has_own_target(h)) return before_first_reset(h, call, ": the target comes from the state");
    IkPoseArgs A;
    A.target = target_pos; A.state = h->state; A.quat = target_quat; A.q_init = q_init;
    A.q_out = q_out; A.residual = residual_out; A.angle = angle_out; A.iterations = iterations_out;
    A.n = h->n;
    A.point = chain_point(p->link, p->local_point);
    A.max_iter = p->max_iterations; A.axis_mode = p->mode == PNR_IK_ORIENT_AXIS;
    A.axis = {(float)(ax[0] / axis_len), (float)(ax[1] / axis_len), (float)(ax[2] / axis_len)};
    A.damping2 = (float)(p->damping * p->damping); A.error_damping = (float)p->error_damping; A.weight = (float)p->orientation_weight;
    A.max_step = (float)p->max_step; A.tol = (float)p->tolerance; A.angle_tol = (float)p->angle_tolerance;
    return launch_env_waves(h, stream, kJointSrcBuffer, [](auto) { return ik_pose_kernel; }, A);  // (no joint source: one form)
}

int pnr_ik_multi_params_default(pnr_ik_multi_params* p, int32_t task)
{
    if (!p) return fail(nullptr, PNR_ERR_INVALID, "pnr_ik_multi_params_default: null params");
    if (task != PNR_IK_TASK_POSITION && task != PNR_IK_TASK_POSE && task != PNR_IK_TASK_AXIS)
        return fail(nullptr, PNR_ERR_INVALID, "pnr_ik_multi_params_default: task %d outside {0, 1, 2} (position, pose, axis)", task);
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(pnr_ik_multi_params);
    p->task = task;
    p->policy = PNR_IK_MULTI_BEST;
    p->num_starts = 8;
    p->link = kNumLinks - 1;
    p->max_iterations = 32;
    p->local_axis[0] = 1.0;
    const bool pose = task != PNR_IK_TASK_POSITION;           // each task's own defaults (pnr_ik_params_default, pnr_ik_pose_params_default)
    p->damping = pose ? 0.03 : 1.0;
    p->error_damping = pose ? 0.01 : 0.0;
    p->orientation_weight = 10.0;
    p->max_step = 0.5;
    p->tolerance = 1e-3;
    p->angle_tolerance = 1e-3;
    return PNR_OK;
}

int pnr_solve_ik_multi(pnr_handle h, const pnr_ik_multi_params* p, const pnr_ik_multi_buffers* b, void* stream)
{
    const char* call = "pnr_solve_ik_multi";
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (!p) return fail(h, PNR_ERR_INVALID, "%s: null params", call);
    if (!b) return fail(h, PNR_ERR_INVALID, "%s: null buffers", call);
    if (p->struct_size != sizeof(pnr_ik_multi_params))
        return fail(h, PNR_ERR_INVALID, "%s: params struct_size %u, want %zu", call, p->struct_size, sizeof(pnr_ik_multi_params));
    if (b->struct_size != sizeof(pnr_ik_multi_buffers))
        return fail(h, PNR_ERR_INVALID, "%s: buffers struct_size %u, want %zu", call, b->struct_size, sizeof(pnr_ik_multi_buffers));
    if (p->task != PNR_IK_TASK_POSITION && p->task != PNR_IK_TASK_POSE && p->task != PNR_IK_TASK_AXIS)
        return fail(h, PNR_ERR_INVALID, "%s: task %d outside {0, 1, 2} (position, pose, axis)", call, p->task);
    if (p->policy != PNR_IK_MULTI_BEST && p->policy != PNR_IK_MULTI_FIRST)
        return fail(h, PNR_ERR_INVALID, "%s: policy %d outside {0, 1} (best, first)", call, p->policy);
    const bool pose = p->task != PNR_IK_TASK_POSITION;
    if (!b->q_out) return fail(h, PNR_ERR_INVALID, "%s: null q_out", call);
    if (pose && !b->target_quat) return fail(h, PNR_ERR_INVALID, "%s: null target_quat", call);
    int log2s = -1;
    for (int k = 0; k <= 6; ++k) if (p->num_starts == (1 << k)) log2s = k;
    if (log2s < 0) return fail(h, PNR_ERR_INVALID, "%s: num_starts %d is not one of 1, 2, 4, 8, 16, 32, 64", call, p->num_starts);
    if (!b->starts && p->num_starts > 1) return fail(h, PNR_ERR_INVALID, "%s: null starts with num_starts %d", call, p->num_starts);
    if (p->link < 0 || p->link >= kNumLinks) return fail(h, PNR_ERR_INVALID, "%s: link %d outside 0..%d", call, p->link, kNumLinks - 1);
    if (p->max_iterations < 1 || p->max_iterations > 1024)
        return fail(h, PNR_ERR_INVALID, "%s: max_iterations %d outside 1..1024", call, p->max_iterations);
    const struct { double v; const char* name; bool zero_ok, pose_only; } scalars[] = {
        {p->damping, "damping", false, false}, {p->max_step, "max_step", false, false}, {p->orientation_weight, "orientation_weight", false, true},
        {p->error_damping, "error_damping", true, false}, {p->tolerance, "tolerance", true, false}, {p->angle_tolerance, "angle_tolerance", true, true}};
    for (const auto& s : scalars)
        if ((pose || !s.pose_only) && !(std::isfinite(s.v) && (s.zero_ok ? s.v >= 0 : s.v > 0)))
            return fail(h, PNR_ERR_INVALID, "%s: %s must be finite and %s 0", call, s.name, s.zero_ok ? ">=" : ">");
    if (!finite_all(p->local_point, 3)) return fail(h, PNR_ERR_INVALID, "%s: non-finite local_point", call);
    const double* ax = p->local_axis;
    const double axis_len = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
    if (pose && (!finite_all(ax, 3) || !std::isfinite(axis_len) || !(axis_len > 0)))
        return fail(h, PNR_ERR_INVALID, "%s: local_axis must be finite and not zero", call);
    if (const int rc = check_aligned(h, call, {{b->q_out, "q_out", 8}, {b->all_q, "all_q", 8}, {b->target_pos, "target_pos", 4},
                                               {b->target_quat, "target_quat", 4}, {b->starts, "starts", 4}, {b->q_init, "q_init", 4},
                                               {b->q_ref, "q_ref", 4}, {b->residual_out, "residual_out", 4}, {b->angle_out, "angle_out", 4},
                                               {b->iterations_out, "iterations_out", 4}, {b->start_out, "start_out", 4},
                                               {b->converged_out, "converged_out", 4}, {b->all_residual, "all_residual", 4},
                                               {b->all_angle, "all_angle", 4}, {b->all_iterations, "all_iterations", 4}})) return rc;
    if (!b->target_pos && !has_own_target(h)) return before_first_reset(h, call, ": the target comes from the state");
    IkMultiArgs A;
    A.target = b->target_pos; A.state = h->state; A.quat = b->target_quat; A.starts = b->starts; A.q_init = b->q_init; A.q_ref = b->q_ref;
    A.q_out = b->q_out; A.residual = b->residual_out; A.angle = b->angle_out; A.iterations = b->iterations_out;
    A.start_out = b->start_out; A.converged = b->converged_out;
    A.all_q = b->all_q; A.all_residual = b->all_residual; A.all_angle = b->all_angle; A.all_iterations = b->all_iterations;
    A.n = h->n;
    A.point = chain_point(p->link, p->local_point);
    A.log2s = log2s; A.per_env = p->starts_per_env != 0; A.first = p->policy == PNR_IK_MULTI_FIRST;
    A.max_iter = p->max_iterations; A.axis_mode = p->task == PNR_IK_TASK_AXIS;
    A.axis = pose ? V3{(float)(ax[0] / axis_len), (float)(ax[1] / axis_len), (float)(ax[2] / axis_len)} : V3{1.f, 0.f, 0.f};
    A.damping2 = (float)(p->damping * p->damping); A.error_damping = (float)p->error_damping;
    A.weight = pose ? (float)p->orientation_weight : 0.f;                      // (the position task: no orientation rows, angle 0)
    A.max_step = (float)p->max_step; A.tol = (float)p->tolerance; A.angle_tol = pose ? (float)p->angle_tolerance : 0.f;
    DeviceGuard g(h->device);
    const long long lanes = h->n << log2s;                                     // one start per lane, 64 >> log2s envs per wave
    const dim3 grid((unsigned)((lanes + kWave - 1) / kWave));
    if (pose) hipLaunchKernelGGL(ik_multi_kernel<true>, grid, dim3(kWave), 0, (hipStream_t)stream, A);
    else hipLaunchKernelGGL(ik_multi_kernel<false>, grid, dim3(kWave), 0, (hipStream_t)stream, A);
    HIP_TRY(h, hipGetLastError());
    return PNR_OK;
}

int pnr_ik_path_params_default(pnr_ik_path_params* p, int32_t task)
{
    if (!p) return fail(nullptr, PNR_ERR_INVALID, "pnr_ik_path_params_default: null params");
    if (task != PNR_IK_TASK_POSITION && task != PNR_IK_TASK_POSE && task != PNR_IK_TASK_AXIS)
        return fail(nullptr, PNR_ERR_INVALID, "pnr_ik_path_params_default: task %d outside {0, 1, 2} (position, pose, axis)", task);
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(pnr_ik_path_params);
    p->task = task;
    p->num_starts = 1;
    p->n_waypoints = 1; p->substeps = 8;
    p->link = kNumLinks - 1;
    p->max_iterations = 32; p->track_iterations = 8;
    p->local_axis[0] = 1.0;
    const bool pose = task != PNR_IK_TASK_POSITION;           // each task's own defaults, as pnr_ik_multi_params_default
    p->damping = pose ? 0.03 : 1.0;
    p->error_damping = pose ? 0.01 : 0.0;
    p->orientation_weight = 10.0;
    p->max_step = 0.5;
    p->tolerance = 1e-3;
    p->angle_tolerance = 1e-3;
    return PNR_OK;
}

int pnr_solve_ik_path(pnr_handle h, const pnr_ik_path_params* p, const pnr_ik_path_buffers* b, void* stream)
{
    const char* call = "pnr_solve_ik_path";
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (!p) return fail(h, PNR_ERR_INVALID, "%s: null params", call);
    if (!b) return fail(h, PNR_ERR_INVALID, "%s: null buffers", call);
    if (p->struct_size != sizeof(pnr_ik_path_params))
        return fail(h, PNR_ERR_INVALID, "%s: params struct_size %u, want %zu", call, p->struct_size, sizeof(pnr_ik_path_params));
    if (b->struct_size != sizeof(pnr_ik_path_buffers))
        return fail(h, PNR_ERR_INVALID, "%s: buffers struct_size %u, want %zu", call, b->struct_size, sizeof(pnr_ik_path_buffers));
    if (p->task != PNR_IK_TASK_POSITION && p->task != PNR_IK_TASK_POSE && p->task != PNR_IK_TASK_AXIS)
        return fail(h, PNR_ERR_INVALID, "%s: task %d outside {0, 1, 2} (position, pose, axis)", call, p->task);
    const bool pose = p->task != PNR_IK_TASK_POSITION;
    if (!b->waypoint_pos) return fail(h, PNR_ERR_INVALID, "%s: null waypoint_pos", call);
    if (!b->summary) return fail(h, PNR_ERR_INVALID, "%s: null summary", call);
    if (pose && !b->waypoint_quat) return fail(h, PNR_ERR_INVALID, "%s: null waypoint_quat", call);
    int log2s = -1;
    for (int k = 0; k <= 6; ++k) if (p->num_starts == (1 << k)) log2s = k;
    if (log2s < 0) return fail(h, PNR_ERR_INVALID, "%s: num_starts %d is not one of 1, 2, 4, 8, 16, 32, 64", call, p->num_starts);
    if (!b->starts && p->num_starts > 1) return fail(h, PNR_ERR_INVALID, "%s: null starts with num_starts %d", call, p->num_starts);
    if (p->n_waypoints < 1 || p->n_waypoints > PNR_MAX_PATH_WAYPOINTS)
        return fail(h, PNR_ERR_INVALID, "%s: n_waypoints %d outside 1..%d", call, p->n_waypoints, PNR_MAX_PATH_WAYPOINTS);
    if (p->substeps < 1 || p->substeps > PNR_MAX_PATH_SUBSTEPS)
        return fail(h, PNR_ERR_INVALID, "%s: substeps %d outside 1..%d", call, p->substeps, PNR_MAX_PATH_SUBSTEPS);
    if (p->winner_rows != PNR_IK_PATH_ROWS_AUTO && p->winner_rows != PNR_IK_PATH_ROWS_SECOND_PASS && p->winner_rows != PNR_IK_PATH_ROWS_SECOND_LAUNCH)
        return fail(h, PNR_ERR_INVALID, "%s: winner_rows %d outside {0, 1, 2} (auto, second pass, second launch)", call, p->winner_rows);
    if (p->link < 0 || p->link >= kNumLinks) return fail(h, PNR_ERR_INVALID, "%s: link %d outside 0..%d", call, p->link, kNumLinks - 1);
    if (p->max_iterations < 1 || p->max_iterations > 1024)
        return fail(h, PNR_ERR_INVALID, "%s: max_iterations %d outside 1..1024", call, p->max_iterations);
    if (p->track_iterations < 1 || p->track_iterations > 1024)
        return fail(h, PNR_ERR_INVALID, "%s: track_iterations %d outside 1..1024", call, p->track_iterations);
    const struct { double v; const char* name; bool zero_ok, pose_only; } scalars[] = {
        {p->damping, "damping", false, false}, {p->max_step, "max_step", false, false}, {p->orientation_weight, "orientation_weight", false, true},
        {p->error_damping, "error_damping", true, false}, {p->tolerance, "tolerance", true, false}, {p->angle_tolerance, "angle_tolerance", true, true}};
    for (const auto& s : scalars)
        if ((pose || !s.pose_only) && !(std::isfinite(s.v) && (s.zero_ok ? s.v >= 0 : s.v > 0)))
            return fail(h, PNR_ERR_INVALID, "%s: %s must be finite and %s 0", call, s.name, s.zero_ok ? ">=" : ">");
    if (!finite_all(p->local_point, 3)) return fail(h, PNR_ERR_INVALID, "%s: non-finite local_point", call);
    const double* ax = p->local_axis;
    const double axis_len = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
    if (pose && (!finite_all(ax, 3) || !std::isfinite(axis_len) || !(axis_len > 0)))
        return fail(h, PNR_ERR_INVALID, "%s: local_axis must be finite and not zero", call);
    if (const int rc = check_aligned(h, call, {{b->summary, "summary", 16}, {b->all_summary, "all_summary", 16}, {b->q_path, "q_path", 8},
                                               {b->waypoint_pos, "waypoint_pos", 4}, {b->waypoint_quat, "waypoint_quat", 4},
                                               {b->starts, "starts", 4}, {b->q_init, "q_init", 4}, {b->q_ref, "q_ref", 4},
                                               {b->residual_path, "residual_path", 4}, {b->angle_path, "angle_path", 4},
                                               {b->iterations_path, "iterations_path", 4}})) return rc;
    const long long groups = ((h->n << log2s) + kWave - 1) / kWave;           // one start per lane, 64 >> log2s envs per wave
    if (groups > 0x7fffffffLL) return fail(h, PNR_ERR_INVALID, "%s: %lld envs x %d starts exceed one launch", call, h->n, p->num_starts);
    IkPathArgs A;
    A.wp_pos = b->waypoint_pos; A.wp_quat = b->waypoint_quat; A.starts = b->starts; A.q_init = b->q_init; A.q_ref = b->q_ref;
    A.summary = b->summary; A.q_path = b->q_path; A.residual = b->residual_path; A.angle = b->angle_path;
    A.iterations = b->iterations_path; A.all_summary = b->all_summary;
    A.n = h->n;
    A.point = chain_point(p->link, p->local_point);
    A.log2s = log2s; A.log2t = log2s; A.starts_per_env = p->starts_per_env != 0; A.wp_per_env = p->waypoints_per_env != 0;
    A.K = p->n_waypoints; A.M = p->substeps; A.C = 1 + (p->n_waypoints - 1) * p->substeps;
    A.max_iter = p->max_iterations; A.track_iter = p->track_iterations; A.axis_mode = p->task == PNR_IK_TASK_AXIS;
    A.axis = pose ? V3{(float)(ax[0] / axis_len), (float)(ax[1] / axis_len), (float)(ax[2] / axis_len)} : V3{1.f, 0.f, 0.f};
    A.damping2 = (float)(p->damping * p->damping); A.error_damping = (float)p->error_damping;
    A.weight = pose ? (float)p->orientation_weight : 0.f;                      // (the position task: no orientation rows, angle 0)
    A.max_step = (float)p->max_step; A.tol = (float)p->tolerance; A.angle_tol = pose ? (float)p->angle_tolerance : 0.f;
    // the winner's rows: a one-start call writes them as it tracks; under S > 1 the winner's start is tracked a second time,
    // in the launch (two passes) or by a second launch at one lane per env (auto: kIkPathAutoRows, measured: DESIGN.md 3z)
    const bool rows = b->q_path || b->residual_path || b->angle_path || b->iterations_path;
    constexpr int kIkPathAutoRows = PNR_IK_PATH_ROWS_SECOND_LAUNCH;
    const int how = p->winner_rows == PNR_IK_PATH_ROWS_AUTO ? kIkPathAutoRows : p->winner_rows;
    const bool again = rows && log2s > 0;
    const bool relaunch = again && how == PNR_IK_PATH_ROWS_SECOND_LAUNCH;
    A.replay = 0; A.passes = again && !relaunch ? 2 : 1; A.store = rows && !relaunch;
    DeviceGuard g(h->device);
    const auto launch = [&](const IkPathArgs& X, const long long waves) {
        if (pose) hipLaunchKernelGGL(ik_path_kernel<true>, dim3((unsigned)waves), dim3(kWave), 0, (hipStream_t)stream, X);
        else hipLaunchKernelGGL(ik_path_kernel<false>, dim3((unsigned)waves), dim3(kWave), 0, (hipStream_t)stream, X);
    };
    launch(A, groups);
    HIP_TRY(h, hipGetLastError());
    if (relaunch) {
        IkPathArgs B = A;
        B.log2s = 0; B.replay = 1; B.passes = 1; B.store = 1; B.all_summary = nullptr;
        launch(B, (h->n + kWave - 1) / kWave);
        HIP_TRY(h, hipGetLastError());
    }
    return PNR_OK;
}

int pnr_contact_params_default(pnr_contact_params* p)
{
    if (!p) return fail(nullptr, PNR_ERR_INVALID, "pnr_contact_params_default: null params");
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(pnr_contact_params);
    p->contact_kp = 2000.0; p->contact_kd = 50.0;       // pnr_config_default's
    return PNR_OK;
}

int pnr_get_contacts(pnr_handle h, const float* joint_state, const pnr_contact_params* p, const float* body_positions, float* points,
                     float* summary, float* joint_torques, void* stream)
{
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (!p) return fail(h, PNR_ERR_INVALID, "pnr_get_contacts: null params");
    if (p->struct_size != sizeof(pnr_contact_params))
        return fail(h, PNR_ERR_INVALID, "pnr_get_contacts: params struct_size %u, want %zu", p->struct_size, sizeof(pnr_contact_params));
    if (!points && !summary && !joint_torques) return fail(h, PNR_ERR_INVALID, "pnr_get_contacts: every output is NULL");
    if (const int rc = check_aligned(h, "pnr_get_contacts", {{points, "points", 16}, {summary, "summary", 16}, {joint_torques, "joint_torques", 16},
                                                              {joint_state, "joint_state", 16}, {body_positions, "body_positions", 4}})) return rc;
    if (p->n_bodies < 0 || p->n_bodies > PNR_MAX_SCENE)
        return fail(h, PNR_ERR_INVALID, "pnr_get_contacts: n_bodies %d outside 0..%d", p->n_bodies, PNR_MAX_SCENE);
    if (!(std::isfinite(p->contact_kp) && std::isfinite(p->contact_kd) && p->contact_kp >= 0 && p->contact_kd >= 0))
        return fail(h, PNR_ERR_INVALID, "pnr_get_contacts: contact_kp and contact_kd must be finite and >= 0");
    for (int b = 0; b < p->n_bodies; ++b)
        if (const int rc = check_scene_body(h, "pnr_get_contacts: body", b, p->bodies[b], true)) return rc;
    if (!joint_state && !has_own_joints(h)) return before_first_reset(h, "pnr_get_contacts");
    const JointSource J = joint_source(h, joint_state);
    ContactArgs A;
    memset(&A, 0, sizeof(A));
    A.src = J.src; A.state = J.state;
    A.body_pos = p->n_bodies > 0 ? body_positions : nullptr;
    A.points = points; A.summary = summary; A.torques = joint_torques;
    A.n = h->n;
    A.ckp = (float)p->contact_kp; A.ckd = (float)p->contact_kd; A.ptr_radius = (float)h->cfg.pointer_radius;
    A.n_bodies = p->n_bodies;
    for (int b = 0; b < p->n_bodies; ++b) A.bodies[b] = scene_body_device(p->bodies[b]);
    if (const float* sphere = shown_sphere(h, PNR_BODY_IN_CONTACTS)) {
        ContactSceneArgs X;
        static_cast<ContactArgs&>(X) = A;
        X.sphere = sphere;
        return launch_env_waves(h, stream, J.kind, [](auto S) { return contacts_kernel<S() | kQueryScene>; }, X);
    }
    return launch_env_waves(h, stream, J.kind, [](auto S) { return contacts_kernel<S()>; }, A);
}

int pnr_path_params_default(pnr_path_params* p)
{
    if (!p) return fail(nullptr, PNR_ERR_INVALID, "pnr_path_params_default: null params");
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(pnr_path_params);
    p->n_waypoints = 1; p->substeps = 8;
    p->sample_mask = kPathAllSamples;
    return PNR_OK;
}

int pnr_path_clearance(pnr_handle h, const pnr_path_params* p, const float* waypoints, const float* body_positions, float* summary,
                       float* clearance, void* stream)
{
    const char* call = "pnr_path_clearance";
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (!p) return fail(h, PNR_ERR_INVALID, "%s: null params", call);
    if (p->struct_size != sizeof(pnr_path_params))
        return fail(h, PNR_ERR_INVALID, "%s: params struct_size %u, want %zu", call, p->struct_size, sizeof(pnr_path_params));
    if (!summary && !clearance) return fail(h, PNR_ERR_INVALID, "%s: every output is NULL", call);
    if (const int rc = check_aligned(h, call, {{summary, "summary", 16}, {clearance, "clearance", 4}, {waypoints, "waypoints", 8},
                                               {body_positions, "body_positions", 4}})) return rc;
    if (p->n_waypoints < 0 || p->n_waypoints > PNR_MAX_PATH_WAYPOINTS)
        return fail(h, PNR_ERR_INVALID, "%s: n_waypoints %d outside 0..%d", call, p->n_waypoints, PNR_MAX_PATH_WAYPOINTS);
    if (p->substeps < 1 || p->substeps > PNR_MAX_PATH_SUBSTEPS)
        return fail(h, PNR_ERR_INVALID, "%s: substeps %d outside 1..%d", call, p->substeps, PNR_MAX_PATH_SUBSTEPS);
    if (p->from_current != 0 && p->from_current != 1) return fail(h, PNR_ERR_INVALID, "%s: from_current must be 0 or 1", call);
    if (p->waypoints_per_env != 0 && p->waypoints_per_env != 1) return fail(h, PNR_ERR_INVALID, "%s: waypoints_per_env must be 0 or 1", call);
    int log2p = -1;
    for (int k = 0; k <= 6; ++k) if (p->lanes_per_env == (1 << k)) log2p = k;
    if (log2p < 0 && p->lanes_per_env != 0)
        return fail(h, PNR_ERR_INVALID, "%s: lanes_per_env %d is not one of 0 (auto), 1, 2, 4, 8, 16, 32, 64", call, p->lanes_per_env);
    const int W = p->n_waypoints + p->from_current;
    if (W < 1) return fail(h, PNR_ERR_INVALID, "%s: n_waypoints 0 without from_current: the path has no waypoint", call);
    if (!waypoints && p->n_waypoints > 0) return fail(h, PNR_ERR_INVALID, "%s: null waypoints with n_waypoints %d", call, p->n_waypoints);
    if ((p->sample_mask & kPathAllSamples) == 0 || (p->sample_mask & ~kPathAllSamples))
        return fail(h, PNR_ERR_INVALID, "%s: sample_mask 0x%x has no bit among the %d samples or a bit above them", call, (unsigned)p->sample_mask, kContactSamples);
    if (!std::isfinite(p->margin)) return fail(h, PNR_ERR_INVALID, "%s: non-finite margin", call);
    if (p->n_bodies < 0 || p->n_bodies > PNR_MAX_SCENE)
        return fail(h, PNR_ERR_INVALID, "%s: n_bodies %d outside 0..%d", call, p->n_bodies, PNR_MAX_SCENE);
    for (int b = 0; b < p->n_bodies; ++b)
        if (const int rc = check_scene_body(h, "pnr_path_clearance: body", b, p->bodies[b], true)) return rc;
    if (p->from_current && !has_own_joints(h)) return before_first_reset(h, call, ": from_current reads the env's joints");
    PathArgs A;
    memset(&A, 0, sizeof(A));
    int kind = kJointSrcBuffer;                         // (no from_current: no joint source)
    if (p->from_current) {
        const JointSource J = joint_source(h, nullptr);
        kind = J.kind; A.src = J.src; A.state = J.state;
    }
    A.waypoints = p->n_waypoints > 0 ? waypoints : nullptr;
    A.body_pos = p->n_bodies > 0 ? body_positions : nullptr;
    A.summary = summary; A.clearance = clearance;
    A.n = h->n;
    A.ptr_radius = (float)h->cfg.pointer_radius; A.margin = (float)p->margin;
    A.n_bodies = p->n_bodies;
    A.K = p->n_waypoints; A.M = p->substeps; A.C = 1 + (W - 1) * p->substeps;
    if (log2p < 0)                                      // auto: the smallest power of two >= C, at most 32 (measured: DESIGN.md 3y)
        for (log2p = 0; log2p < 5 && (1 << log2p) < A.C; ++log2p) {}
    A.log2p = log2p;
    A.per_env = p->waypoints_per_env;
    A.mask = p->sample_mask;
    for (int b = 0; b < p->n_bodies; ++b) A.bodies[b] = scene_body_device(p->bodies[b]);
    const long long groups = ((h->n << log2p) + kWave - 1) / kWave;       // one configuration per lane, 64 >> log2p envs per wave
    if (groups > 0x7fffffffLL) return fail(h, PNR_ERR_INVALID, "%s: %lld envs x %d lanes exceed one launch", call, h->n, 1 << log2p);
    DeviceGuard g(h->device);
    const dim3 grid((unsigned)groups);
    const float* sphere = shown_sphere(h, PNR_BODY_IN_CONTACTS);
    PathSceneArgs X;
    static_cast<PathArgs&>(X) = A;
    X.sphere = sphere;
    with_int<kJointSrcBuffer, kJointSrcDyn, kJointSrcKin>(kind, [&](auto S) {
        if (sphere) hipLaunchKernelGGL(path_clearance_kernel<S() | kQueryScene>, grid, dim3(kWave), 0, (hipStream_t)stream, X);
        else hipLaunchKernelGGL(path_clearance_kernel<S()>, grid, dim3(kWave), 0, (hipStream_t)stream, A);
    });
    HIP_TRY(h, hipGetLastError());
    return PNR_OK;
}

int pnr_retime_params_default(pnr_retime_params* p)
{
    if (!p) return fail(nullptr, PNR_ERR_INVALID, "pnr_retime_params_default: null params");
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(pnr_retime_params);
    p->n_points = 3;
    for (int j = 0; j < kDof; ++j) { p->v_max[j] = 2.0; p->a_max[j] = 10.0; }     // (tau_max: 0, to be set with the torque flag)
    return PNR_OK;
}

// the checks of pnr_retime_params that pnr_retime_workspace_bytes and pnr_retime_path share
static int check_retime_params(pnr_handle h, const char* call, const pnr_retime_params* p)
{
    if (!p) return fail(h, PNR_ERR_INVALID, "%s: null params", call);
    if (p->struct_size != sizeof(pnr_retime_params))
        return fail(h, PNR_ERR_INVALID, "%s: params struct_size %u, want %zu", call, p->struct_size, sizeof(pnr_retime_params));
    if (p->n_points < 3 || p->n_points > PNR_MAX_TRAJ_POINTS)
        return fail(h, PNR_ERR_INVALID, "%s: n_points %d outside 3..%d (two points cannot move under this discretisation)", call, p->n_points,
                    PNR_MAX_TRAJ_POINTS);
    if (p->path_per_env != 0 && p->path_per_env != 1) return fail(h, PNR_ERR_INVALID, "%s: path_per_env must be 0 or 1", call);
    if (p->flags & ~PNR_RETIME_TORQUE) return fail(h, PNR_ERR_INVALID, "%s: unknown flags 0x%x", call, (unsigned)p->flags);
    const struct { const double* v; const char* name; bool used; } limits[] = {
        {p->v_max, "v_max", true}, {p->a_max, "a_max", true}, {p->tau_max, "tau_max", (p->flags & PNR_RETIME_TORQUE) != 0}};
    for (const auto& l : limits)
        for (int j = 0; l.used && j < kDof; ++j)
            if (!(std::isfinite(l.v[j]) && l.v[j] > 0 && std::isfinite((float)l.v[j]) && (float)l.v[j] > 0.f))
                return fail(h, PNR_ERR_INVALID, "%s: %s[%d] must be finite and > 0", call, l.name, j);
    return PNR_OK;
}

int pnr_retime_workspace_bytes(pnr_handle h, const pnr_retime_params* p, uint64_t* bytes)
{
    const char* call = "pnr_retime_workspace_bytes";
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (!bytes) return fail(h, PNR_ERR_INVALID, "%s: null bytes", call);
    if (const int rc = check_retime_params(h, call, p)) return rc;
    *bytes = (p->flags & PNR_RETIME_TORQUE) ? (uint64_t)p->n_points * kRetimeRowFloats * (uint64_t)h->n * sizeof(float) : 0;
    return PNR_OK;
}

int pnr_retime_path(pnr_handle h, const pnr_retime_params* p, const pnr_retime_buffers* b, void* stream)
{
    const char* call = "pnr_retime_path";
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (const int rc = check_retime_params(h, call, p)) return rc;
    if (!b) return fail(h, PNR_ERR_INVALID, "%s: null buffers", call);
    if (b->struct_size != sizeof(pnr_retime_buffers))
        return fail(h, PNR_ERR_INVALID, "%s: buffers struct_size %u, want %zu", call, b->struct_size, sizeof(pnr_retime_buffers));
    const bool torque = (p->flags & PNR_RETIME_TORQUE) != 0;
    if (!b->q_path) return fail(h, PNR_ERR_INVALID, "%s: null q_path", call);
    if (!b->summary) return fail(h, PNR_ERR_INVALID, "%s: null summary", call);
    if (torque && !b->workspace) return fail(h, PNR_ERR_INVALID, "%s: null workspace with torque rows", call);
    if (const int rc = check_aligned(h, call, {{b->summary, "summary", 16}, {b->q_path, "q_path", 8}, {b->workspace, "workspace", 4},
                                               {b->times, "times", 4}, {b->sdot2, "sdot2", 4}})) return rc;
    // a dynamics-mode handle's link scales are drawn by the first reset: no model for the torque rows before it
    if (torque && h->dyn && !has_link_scales(h)) return before_first_reset(h, call, ": the torque rows use the env's link scales");
    RetimeArgs A;
    A.q_path = b->q_path; A.dyn = h->dyn; A.rows = torque ? (float*)b->workspace : nullptr;
    A.summary = b->summary; A.times = b->times; A.sdot2 = b->sdot2;
    A.n = h->n; A.C = p->n_points; A.per_env = p->path_per_env;
    A.gravity = (float)h->cfg.gravity;
    for (int j = 0; j < kDof; ++j) { A.v_max[j] = (float)p->v_max[j]; A.a_max[j] = (float)p->a_max[j]; A.tau_max[j] = torque ? (float)p->tau_max[j] : 1.f; }
    DeviceGuard g(h->device);
    const unsigned waves = (unsigned)((h->n + kWave - 1) / kWave);
    const size_t lds = (size_t)A.C * kWave * sizeof(float);            // K_k per lane: 64 KB at C = 256
    if (torque) {
        hipLaunchKernelGGL(retime_rows_kernel, dim3(waves, (unsigned)A.C), dim3(kWave), 0, (hipStream_t)stream, A);
        HIP_TRY(h, hipGetLastError());
        hipLaunchKernelGGL(retime_pass_kernel<true>, dim3(waves), dim3(kWave), lds, (hipStream_t)stream, A);
    } else {
        hipLaunchKernelGGL(retime_pass_kernel<false>, dim3(waves), dim3(kWave), lds, (hipStream_t)stream, A);
    }
    HIP_TRY(h, hipGetLastError());
    return PNR_OK;
}

int pnr_traj_sample_params_default(pnr_traj_sample_params* p)
{
    if (!p) return fail(nullptr, PNR_ERR_INVALID, "pnr_traj_sample_params_default: null params");
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(pnr_traj_sample_params);
    p->n_points = 3;
    p->n_samples = 1;
    p->dt = 10.0 / 240.0;                               // pnr_config_default's timestep x frame_skip: one world step
    return PNR_OK;
}

int pnr_sample_trajectory(pnr_handle h, const pnr_traj_sample_params* p, const float* q_path, const float* times, const float* sdot2,
                          const float* summary, float* targets, void* stream)
{
    const char* call = "pnr_sample_trajectory";
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (!p) return fail(h, PNR_ERR_INVALID, "%s: null params", call);
    if (p->struct_size != sizeof(pnr_traj_sample_params))
        return fail(h, PNR_ERR_INVALID, "%s: params struct_size %u, want %zu", call, p->struct_size, sizeof(pnr_traj_sample_params));
    if (p->n_points < 3 || p->n_points > PNR_MAX_TRAJ_POINTS)
        return fail(h, PNR_ERR_INVALID, "%s: n_points %d outside 3..%d", call, p->n_points, PNR_MAX_TRAJ_POINTS);
    if (p->path_per_env != 0 && p->path_per_env != 1) return fail(h, PNR_ERR_INVALID, "%s: path_per_env must be 0 or 1", call);
    if (p->n_samples < 1 || p->n_samples > PNR_MAX_TRAJ_SAMPLES)
        return fail(h, PNR_ERR_INVALID, "%s: n_samples %d outside 1..%d", call, p->n_samples, PNR_MAX_TRAJ_SAMPLES);
    if (!(std::isfinite(p->t0) && p->t0 >= 0)) return fail(h, PNR_ERR_INVALID, "%s: t0 must be finite and >= 0", call);
    if (!(std::isfinite(p->dt) && (float)p->dt > 0.f && std::isfinite((float)p->dt))) return fail(h, PNR_ERR_INVALID, "%s: dt must be finite and > 0", call);
    const struct { const void* ptr; const char* name; } need[] = {{q_path, "q_path"}, {times, "times"}, {sdot2, "sdot2"}, {summary, "summary"},
                                                                  {targets, "targets"}};
    for (const auto& a : need)
        if (!a.ptr) return fail(h, PNR_ERR_INVALID, "%s: null %s", call, a.name);
    if (const int rc = check_aligned(h, call, {{targets, "targets", 16}, {summary, "summary", 16}, {q_path, "q_path", 8}, {times, "times", 4},
                                               {sdot2, "sdot2", 4}})) return rc;
    const long long groups = (h->n * (long long)p->n_samples + kWave - 1) / kWave;     // one (env, sample) per lane
    if (groups > 0x7fffffffLL) return fail(h, PNR_ERR_INVALID, "%s: %lld envs x %d samples exceed one launch", call, h->n, p->n_samples);
    TrajSampleArgs A;
    A.q_path = q_path; A.times = times; A.sdot2 = sdot2; A.summary = summary; A.targets = targets;
    A.n = h->n; A.C = p->n_points; A.per_env = p->path_per_env; A.T = p->n_samples;
    A.t0 = (float)p->t0; A.dt = (float)p->dt;
    DeviceGuard g(h->device);
    hipLaunchKernelGGL(traj_sample_kernel, dim3((unsigned)groups), dim3(kWave), 0, (hipStream_t)stream, A);
    HIP_TRY(h, hipGetLastError());
    return PNR_OK;
}

}  // extern "C"

// pnr_render's checks of its params (nothing launched, nothing written on failure) and the kernel's constants built from them;
// use_view false (pnr_render_cameras with camera rows): p->view is neither checked nor read, the camera is the identity
static int render_setup(pnr_handle h, const pnr_render_params* p, RenderParams& P, bool use_view = true)
{
    if (p->struct_size != sizeof(pnr_render_params))
        return fail(h, PNR_ERR_INVALID, "pnr_render: params struct_size %u, want %zu", p->struct_size, sizeof(pnr_render_params));
    if (p->width < 1 || p->width > 4096 || p->height < 1 || p->height > 4096)
        return fail(h, PNR_ERR_INVALID, "pnr_render: image size %d x %d outside 1..4096", p->width, p->height);
    if (!(p->fov_y > 0 && p->fov_y < 180)) return fail(h, PNR_ERR_INVALID, "pnr_render: fov_y must lie in (0, 180) degrees");
    if (!(std::isfinite(p->near_clip) && std::isfinite(p->far_clip) && p->near_clip > 0 && p->far_clip > 0))
        return fail(h, PNR_ERR_INVALID, "pnr_render: near_clip and far_clip must be finite and > 0");
    if (!(p->near_clip < p->far_clip)) return fail(h, PNR_ERR_INVALID, "pnr_render: near_clip must be < far_clip");
    static const double kIdentityView[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const double* V = use_view ? p->view : kIdentityView;
    if (!finite_all(V, 16)) return fail(h, PNR_ERR_INVALID, "pnr_render: non-finite view matrix");
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const double d = V[4 * a] * V[4 * b] + V[4 * a + 1] * V[4 * b + 1] + V[4 * a + 2] * V[4 * b + 2];
            if (!(std::fabs(d - (a == b ? 1.0 : 0.0)) <= 1e-5))
                return fail(h, PNR_ERR_INVALID, "pnr_render: the view matrix's rotation is not orthonormal");
        }
    if (!finite_all(p->light_direction, 3)) return fail(h, PNR_ERR_INVALID, "pnr_render: non-finite light_direction");
    const double ll = std::sqrt(sum_sq(p->light_direction, 3));
    if (!(ll > 0)) return fail(h, PNR_ERR_INVALID, "pnr_render: zero light_direction");
    if (!std::isfinite(p->ambient) || !std::isfinite(p->diffuse)) return fail(h, PNR_ERR_INVALID, "pnr_render: non-finite ambient or diffuse");
    if (!finite_all(p->background, 3)) return fail(h, PNR_ERR_INVALID, "pnr_render: non-finite background");
    if (!finite_all(p->target_rgba, 4)) return fail(h, PNR_ERR_INVALID, "pnr_render: non-finite target_rgba");
    if (p->n_bodies < 0 || p->n_bodies > PNR_MAX_SCENE)
        return fail(h, PNR_ERR_INVALID, "pnr_render: n_bodies %d outside 0..%d", p->n_bodies, PNR_MAX_SCENE);
    for (int b = 0; b < p->n_bodies; ++b) {
        const int rc = check_scene_body(h, "pnr_render: body", b, p->bodies[b], true);
        if (rc) return rc;
        if (!finite_all(p->body_rgba[b], 4)) return fail(h, PNR_ERR_INVALID, "pnr_render: body %d: non-finite colour", b);
    }

    memset(&P, 0, sizeof(P));
    // the eye axes are the rows of the view rotation; the eye sits at -R^T t
    double eye[3];
    for (int k = 0; k < 3; ++k) eye[k] = -(V[k] * V[3] + V[4 + k] * V[7] + V[8 + k] * V[11]);
    for (int k = 0; k < 3; ++k) {
        P.eye[k] = (float)eye[k];
        P.right[k] = (float)V[k]; P.up[k] = (float)V[4 + k]; P.back[k] = (float)V[8 + k];
        P.light[k] = (float)(p->light_direction[k] / ll);
        P.bg[k] = p->background[k];
        P.target_rgb[k] = p->target_rgba[k];
    }
    const double tan_half = std::tan(0.5 * p->fov_y * M_PI / 180.0);
    P.sy = (float)tan_half;
    P.sx = (float)(tan_half * (double)p->width / (double)p->height);
    P.near_clip = (float)p->near_clip; P.far_clip = (float)p->far_clip;
    P.ambient = (float)p->ambient; P.diffuse = (float)p->diffuse;
    P.target_alpha = p->target_rgba[3];
    P.target_radius = (float)h->cfg.target_radius;
    P.W = p->width; P.H = p->height; P.HW = p->width * p->height;
    // pixels per lane: 4 (1 024-pixel tiles) unless that leaves fewer than ~4 096 workgroups (one env at 1280 x 800: 4 000 of 256)
    const long long total = h->n * (long long)P.HW;
    P.ppl = total >= 4096LL * 1024 ? 4 : (total >= 4096LL * 512 ? 2 : 1);
    const int tile_px = kRenderThreads * P.ppl;
    P.tiles = (P.HW + tile_px - 1) / tile_px;
    if (h->n * (long long)P.tiles > 0x7fffffffLL)
        return fail(h, PNR_ERR_INVALID, "pnr_render: %lld envs x %d tiles exceed one launch", h->n, P.tiles);
    // the static bodies, in world space once for all envs
    P.n_static = p->n_bodies;
    for (int b = 0; b < p->n_bodies; ++b) {
        const pnr_scene_body& S = p->bodies[b];
        RenderPrim& Q = P.bodies[b];
        const double e[3] = {eye[0] - S.position[0], eye[1] - S.position[1], eye[2] - S.position[2]};
        double rt[9], bound;
        Q.shape = scene_body_prim(S, rt, Q.h, bound);
        double o[3];                                 // the eye in the primitive frame (a plane: o[2] = n . (eye - point))
        for (int i = 0; i < 3; ++i) o[i] = rt[3 * i] * e[0] + rt[3 * i + 1] * e[1] + rt[3 * i + 2] * e[2];
        for (int k = 0; k < 9; ++k) Q.rt[k] = (float)rt[k];
        for (int k = 0; k < 3; ++k) { Q.o[k] = (float)o[k]; Q.rgb[k] = p->body_rgba[b][k]; }
        Q.label = kSegBody0 + b;
        if (S.shape == PNR_SHAPE_PLANE) { Q.x0 = 0; Q.x1 = P.W - 1; Q.y0 = 0; Q.y1 = P.H - 1; }
        else {
            const double d[3] = {-e[0], -e[1], -e[2]};
            const float cx = (float)(V[0] * d[0] + V[1] * d[1] + V[2] * d[2]), cy = (float)(V[4] * d[0] + V[5] * d[1] + V[6] * d[2]);
            const float dz = (float)-(V[8] * d[0] + V[9] * d[1] + V[10] * d[2]);
            sphere_rect(cx, cy, dz, (float)bound, P, Q.x0, Q.x1, Q.y0, Q.y1);
        }
    }
    return PNR_OK;
}

// the moving sphere's colour where the caller never set one: the URDF's obstacle_mat (render.OBSTACLE_RGBA)
static const float kObstacleRgb[3] = {0.3f, 0.3f, 0.3f};

// pnr_render_cameras' mount: the parent link (-1 or 0: the world), the camera rows (null: the inverse of the params' view)
struct CameraMount { int link; const float* cameras; int per_env; };

// pnr_render and pnr_render_bodies: render_kernel where every env sees the caller's bodies where they are and no moving sphere
// (what pnr_render always launched), else its scene form; pnr_render_cameras (mount non-null): the same two through the world
// camera of the params' view, else the camera form
static int render_call(pnr_handle h, const float* joint_state, const pnr_render_params* p, const float* body_positions, uint8_t* rgb,
                       float* depth, uint8_t* seg, void* stream, const CameraMount* mount = nullptr)
{
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (!p) return fail(h, PNR_ERR_INVALID, "pnr_render: null params");
    if (!rgb && !depth && !seg) return fail(h, PNR_ERR_INVALID, "pnr_render: every output is NULL");
    if (const int rc = check_aligned(h, "pnr_render", {{rgb, "rgb", 16}, {depth, "depth", 16}, {seg, "seg", 16}, {joint_state, "joint_state", 16},
                                                        {body_positions, "body_positions", 4}})) return rc;
    if (mount) {
        if (mount->link < -1 || mount->link >= kNumLinks)
            return fail(h, PNR_ERR_INVALID, "pnr_render_cameras: camera_link %d outside -1..%d", mount->link, kNumLinks - 1);
        if (mount->per_env != 0 && mount->per_env != 1) return fail(h, PNR_ERR_INVALID, "pnr_render_cameras: cameras_per_env must be 0 or 1");
        if (const int rc = check_aligned(h, "pnr_render_cameras", {{mount->cameras, "cameras", 4}})) return rc;
    }
    if (!has_own_target(h)) return before_first_reset(h, "pnr_render", ": the target comes from the state");
    const bool own_camera = mount && (mount->cameras || mount->link >= 1);      // (link 0 is the base: the world frame)
    RenderParams P;
    const int rc = render_setup(h, p, P, !(mount && mount->cameras));
    if (rc) return rc;
    DeviceGuard g(h->device);
    const dim3 grid((unsigned)(h->n * P.tiles)), block(kRenderThreads);
    hipStream_t st = (hipStream_t)stream;
    const JointSource J = joint_source(h, joint_state);       // (the kernel reads the target from h->state whatever the source)
    RenderSceneParams X;
    static_cast<RenderParams&>(X) = P;
    X.body_pos = p->n_bodies > 0 ? body_positions : nullptr;
    X.sphere = shown_sphere(h, PNR_BODY_IN_RENDER);
    for (int k = 0; k < 3; ++k) X.sphere_rgb[k] = h->body_rgb_set ? h->body_rgb[k] : kObstacleRgb[k];
    RenderCameraParams Y;
    if (own_camera) {                                   // P's camera is the mount's, in the parent frame; the kernel composes each env's
        static_cast<RenderSceneParams&>(Y) = X;
        Y.cameras = mount->cameras; Y.cam_per_env = mount->per_env;
        Y.cam_body = mount->link >= 1 ? kLinkBody[mount->link] : -1;
        Y.cam_tip = mount->link == kNumLinks - 1;
        memset(Y.body_centre, 0, sizeof(Y.body_centre));
        for (int b = 0; b < p->n_bodies; ++b)
            for (int k = 0; k < 3; ++k) Y.body_centre[b][k] = (float)p->bodies[b].position[k];
    }
    with_int<kJointSrcBuffer, kJointSrcDyn, kJointSrcKin>(J.kind, [&](auto S) {
        if (own_camera)
            hipLaunchKernelGGL(render_kernel<S() | kQueryScene | kQueryCamera>, grid, block, 0, st, J.src, h->state, (long long)h->n, Y, rgb, depth, seg);
        else if (X.body_pos || X.sphere)
            hipLaunchKernelGGL(render_kernel<S() | kQueryScene>, grid, block, 0, st, J.src, h->state, (long long)h->n, X, rgb, depth, seg);
        else
            hipLaunchKernelGGL(render_kernel<S()>, grid, block, 0, st, J.src, h->state, (long long)h->n, P, rgb, depth, seg);
    });
    HIP_TRY(h, hipGetLastError());
    return PNR_OK;
}

extern "C" {

int pnr_render(pnr_handle h, const float* joint_state, const pnr_render_params* p, uint8_t* rgb, float* depth, uint8_t* seg,
               void* stream)
{
    return render_call(h, joint_state, p, nullptr, rgb, depth, seg, stream);
}

int pnr_render_bodies(pnr_handle h, const float* joint_state, const pnr_render_params* p, const float* body_positions, uint8_t* rgb,
                      float* depth, uint8_t* seg, void* stream)
{
    return render_call(h, joint_state, p, body_positions, rgb, depth, seg, stream);
}

int pnr_render_cameras(pnr_handle h, const float* joint_state, const pnr_render_params* p, const float* body_positions,
                       int32_t camera_link, const float* cameras, int32_t cameras_per_env, uint8_t* rgb, float* depth,
                       uint8_t* seg, void* stream)
{
    const CameraMount mount = {camera_link, cameras, cameras_per_env};
    return render_call(h, joint_state, p, body_positions, rgb, depth, seg, stream, &mount);
}

}  // extern "C"

// one static body as pnr_ray_test's kernel reads it (pnr_rays.h RayPrim), in world space once for all envs
static RayPrim ray_body_record(const pnr_scene_body& S, int b)
{
    RayPrim Q;
    memset(&Q, 0, sizeof(Q));
    double rt[9], bound;
    Q.shape = scene_body_prim(S, rt, Q.h, bound);
    Q.bound2 = Q.shape == kVisPlane ? INFINITY : ray_bound2((float)bound);
    for (int k = 0; k < 9; ++k) Q.rt[k] = (float)rt[k];
    for (int k = 0; k < 3; ++k) Q.c[k] = (float)S.position[k];
    Q.label = kSegBody0 + b;
    return Q;
}

extern "C" {

int pnr_ray_params_default(pnr_ray_params* p)
{
    if (!p) return fail(nullptr, PNR_ERR_INVALID, "pnr_ray_params_default: null params");
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(pnr_ray_params);
    p->n_rays = 1; p->parent_link = -1; p->hit_mask = PNR_RAY_HIT_BODIES;
    return PNR_OK;
}

int pnr_ray_test(pnr_handle h, const float* joint_state, const pnr_ray_params* p, const float* rays, const float* body_positions,
                 float* hits, float* fractions, void* stream)
{
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (!p) return fail(h, PNR_ERR_INVALID, "pnr_ray_test: null params");
    if (p->struct_size != sizeof(pnr_ray_params))
        return fail(h, PNR_ERR_INVALID, "pnr_ray_test: params struct_size %u, want %zu", p->struct_size, sizeof(pnr_ray_params));
    if (p->n_rays < 1 || p->n_rays > PNR_MAX_RAYS) return fail(h, PNR_ERR_INVALID, "pnr_ray_test: n_rays %d outside 1..%d", p->n_rays, PNR_MAX_RAYS);
    if (p->rays_per_env != 0 && p->rays_per_env != 1) return fail(h, PNR_ERR_INVALID, "pnr_ray_test: rays_per_env must be 0 or 1");
    if (p->parent_link < -1 || p->parent_link >= kNumLinks)
        return fail(h, PNR_ERR_INVALID, "pnr_ray_test: parent_link %d outside -1..%d", p->parent_link, kNumLinks - 1);
    constexpr int all = PNR_RAY_HIT_BODIES | PNR_RAY_HIT_ARM | PNR_RAY_HIT_TARGET;
    if (p->hit_mask == 0 || (p->hit_mask & ~all)) return fail(h, PNR_ERR_INVALID, "pnr_ray_test: hit_mask %d is empty or has unknown bits", p->hit_mask);
    if (p->n_bodies < 0 || p->n_bodies > PNR_MAX_SCENE)
        return fail(h, PNR_ERR_INVALID, "pnr_ray_test: n_bodies %d outside 0..%d", p->n_bodies, PNR_MAX_SCENE);
    if (!rays) return fail(h, PNR_ERR_INVALID, "pnr_ray_test: null rays");
    if (!hits && !fractions) return fail(h, PNR_ERR_INVALID, "pnr_ray_test: every output is NULL");
    if (const int rc = check_aligned(h, "pnr_ray_test", {{rays, "rays", 4}, {hits, "hits", 16}, {fractions, "fractions", 16},
                                                          {joint_state, "joint_state", 16}, {body_positions, "body_positions", 4}})) return rc;
    for (int b = 0; b < p->n_bodies; ++b)
        if (const int rc = check_scene_body(h, "pnr_ray_test: body", b, p->bodies[b], true)) return rc;
    if (!joint_state && !has_own_joints(h)) return before_first_reset(h, "pnr_ray_test");
    if ((p->hit_mask & PNR_RAY_HIT_TARGET) && !has_own_target(h)) return before_first_reset(h, "pnr_ray_test", ": the target comes from the state");
    const JointSource J = joint_source(h, joint_state);
    RayArgs A;
    memset(&A, 0, sizeof(A));
    A.src = J.src; A.state = h->state;                 // (the target is read from h->state whatever the joint source)
    A.rays = rays; A.body_pos = p->n_bodies > 0 ? body_positions : nullptr;
    A.hits = hits; A.fractions = fractions;
    A.n = h->n; A.total = h->n * (long long)p->n_rays;
    A.n_rays = p->n_rays; A.per_env = p->rays_per_env;
    A.parent_body = p->parent_link >= 1 ? kLinkBody[p->parent_link] : -1;       // link 0 is the base: the world frame
    A.parent_tip = p->parent_link == kNumLinks - 1;
    A.mask = p->hit_mask; A.n_bodies = p->n_bodies;
    // pairs per workgroup: 256, or fewer where 256 pairs would span more than kRayMaxEnvs envs; whole waves where it can
    long long span = (long long)(kRayMaxEnvs - 1) * p->n_rays;
    span = span >= kRayThreads ? kRayThreads : (span >= kWave ? span / kWave * kWave : span);
    A.span = (int)span;
    const long long touched = (span + p->n_rays - 2) / p->n_rays + 1;
    A.max_envs = (int)(touched < h->n ? touched : h->n);
    A.target_radius = (float)h->cfg.target_radius;
    for (int b = 0; b < p->n_bodies; ++b) A.bodies[b] = ray_body_record(p->bodies[b], b);
    const long long groups = (A.total + span - 1) / span;
    if (groups > 0x7fffffffLL) return fail(h, PNR_ERR_INVALID, "pnr_ray_test: %lld envs x %d rays exceed one launch", h->n, p->n_rays);
    DeviceGuard g(h->device);
    const dim3 grid((unsigned)groups), block((unsigned)((span + kWave - 1) / kWave * kWave));
    // the moving sphere is one of the bodies: seen with the bodies bit of the mask
    const float* sphere = (p->hit_mask & PNR_RAY_HIT_BODIES) ? shown_sphere(h, PNR_BODY_IN_RAYS) : nullptr;
    const size_t lds = sizeof(float) * (size_t)(sphere ? ray_scene_lds_words(A.max_envs) : ray_lds_words(A.max_envs));
    RaySceneArgs X;
    static_cast<RayArgs&>(X) = A;
    X.sphere = sphere;
    with_int<kJointSrcBuffer, kJointSrcDyn, kJointSrcKin>(J.kind, [&](auto S) {
        if (sphere) hipLaunchKernelGGL(ray_kernel<S() | kQueryScene>, grid, block, lds, (hipStream_t)stream, X);
        else hipLaunchKernelGGL(ray_kernel<S()>, grid, block, lds, (hipStream_t)stream, A);
    });
    HIP_TRY(h, hipGetLastError());
    return PNR_OK;
}

}  // extern "C"
