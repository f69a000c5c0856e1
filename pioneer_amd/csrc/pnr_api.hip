// pnr_api.hip — the core unit of the MI355X-native Pioneer-arm engine's C ABI (include/pioneer_amd.h): the handle, the error
// plumbing, config / create / destroy, reset / observe / step / rollout / world step with every one of their argument checks,
// the joint motors, the state getters and setters.  It launches every kernel of pnr_env_kernels.h: step_kernel, reset_kernel,
// the dynamics-mode step, rollout and world-step kernels, kin_world_kernel, the two state converters and diag_sincos_kernel
// (why the dynamics kernels compile here: DESIGN.md 3m).  The queries are pnr_queries.hip's.  gfx950 only; no CPU fallback.
//
// Execution shape of the step kernels: a lane PAIR per env (three joints per lane), one 64-lane wave
// = 32 envs per workgroup.  State lives in HBM as two float4 planes [2][2n], a
// float2 hot half [2n] and a float4 cold part [n] (24 words per env, pnr_device.h),
// so a wave moves each plane with one 1-KiB dwordx4 instruction and stores the
// cold part only where it resets an env.  Observations are staged through a 17.5 KB LDS tile and leave as
// 16-byte stores: env-major rows of a wave are one contiguous 17.5 KB span;
// feature-major columns leave as 128-B segments, eight features per
// instruction, as non-temporal stores (write-once streaming data must not churn
// the L2s that hold the state planes).  The grid is persistent (<= 2 048
// one-wave workgroups striding over 32-env tiles, next tile prefetched ahead of
// the current tile's stores: a wave's VMEM operations retire in order), and the
// LDS hand-off inside the single-wave workgroup is a compiler-only barrier.
// Envs never interact, so there is no cross-workgroup traffic and block -> XCD
// placement only matters for L2 residency of the state planes (block b touches
// the same lines every launch).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <new>
#include <string>
#include <tuple>

#include "../../include/pioneer_amd.h"

// Ablation switches (timing-only builds whose OUTPUTS ARE WRONG: stores, the integrator or the obs flush gated off; grid-cap
// overrides) exist only in a variant library built with -DPNR_DIAG_BUILD=1 (`_lib.build_library(extra_flags=["-DPNR_DIAG_BUILD=1"],
// out_path=...)`), which reads them from the environment at pnr_create.  The product library ignores the environment
// (tests/test_abi.py checks that it holds no such string).
#ifndef PNR_DIAG_BUILD
#define PNR_DIAG_BUILD 0
#endif

#include "pnr_env_host.h"
#include "pnr_env_kernels.h"

// =====================================================================================
// host side
// =====================================================================================
using namespace pnr;

static thread_local char g_err[512] = "";

// the one place error messages are written (pnr_host.h: shared with pnr_learn.hip, not exported)
int pnr_failv(char* handle_err, int code, const char* fmt, va_list ap)
{
    char* dst = handle_err ? handle_err : g_err;
    vsnprintf(dst, 512, fmt, ap);
    if (handle_err) { strncpy(g_err, handle_err, sizeof(g_err) - 1); g_err[sizeof(g_err) - 1] = 0; }
    return code;
}

int fail(pnr_handle h, int code, const char* fmt, ...)       // (pnr_env_host.h: the env units' one error call)
{
    va_list ap;
    va_start(ap, fmt);
    const int rc = pnr_failv(h ? h->err : nullptr, code, fmt, ap);
    va_end(ap);
    return rc;
}

static inline bool aligned16(const void* p) { return aligned_to(p, 16); }
static inline bool aligned8(const void* p) { return aligned_to(p, 8); }

// an optional double argument left out (NaN) takes its default, as setJointMotorControl2's optional arguments take Bullet's
static inline double or_default(double given, double dflt) { return given == given ? given : dflt; }

// One joint's entries of the JointMotorTable, assigned in one place
struct JointMotor { float kp, kd, cpos, vcap, tcap, r_ref = 0.f, v_ref = 0.f; int from_cmd = 0, kind = kMotorPD; };

static void set_motor(JointMotorTable& W, int j, const JointMotor& m)
{
    W.kp[j] = m.kp; W.kd[j] = m.kd; W.cpos[j] = m.cpos; W.vcap[j] = m.vcap; W.tcap[j] = m.tcap;
    W.r_ref[j] = m.r_ref; W.v_ref[j] = m.v_ref; W.from_cmd[j] = m.from_cmd; W.kind[j] = m.kind;
}

// The one motor law of pnr_dyn.h (oracle: orc_dyn_motor_torque), folded:
//   tau = clip(kp (r - q) + kd (clamp(v + cpos (r - q), +-vcap) - qd), +-tcap)
// A velocity cap turns the position term into the velocity asked for; teleport: no motor at all.
static JointMotor pd_motor(bool velocity, double kp, double kd, double force_limit, double max_velocity, bool teleport)
{
    const bool capped = max_velocity > 0;
    JointMotor m;
    m.kp = (teleport || velocity || capped) ? 0.f : (float)kp;
    m.kd = teleport ? 0.f : (float)kd;
    m.cpos = (!velocity && capped) ? (float)(kp / kd) : 0.f;
    m.vcap = capped ? (float)max_velocity : INFINITY;
    m.tcap = force_limit > 0 ? (float)force_limit : INFINITY;
    return m;
}

// the argument checks of pnr_get_state / pnr_set_state and their dyn twins
static int check_state_call(pnr_handle h, const void* words, const char* call, bool dyn)
{
    if (!h || !words) return fail(h, PNR_ERR_INVALID, "%s: null argument", call);
    if (dyn && !h->dyn) return fail(h, PNR_ERR_UNSUPPORTED, "handle is not in dynamics mode");
    return PNR_OK;
}

static inline unsigned grid_for(long long n) { return (unsigned)((n + kEnvsPerWave - 1) / kEnvsPerWave); }

// reset_kernel<MODE, OBS, DYN>, MODE 0: pnr_reset, 1: pnr_observe; OBS: 0 no obs, env-major rows 2 (all envs) / 3 (masked),
// feature-major columns 4 (all) / 1 (masked).  KINDS lists the OBS values the call can ask for: only those are instantiated.
template <int MODE, int... KINDS>
static int launch_reset(pnr_handle h, const KParams& P, int obs_kind, void* stream)
{
    DeviceGuard g(h->device);
    with_int<KINDS...>(obs_kind, [&](auto O) { with_bool(h->dyn != nullptr, [&](auto Dyn) {
        hipLaunchKernelGGL((reset_kernel<MODE, O(), Dyn()>), dim3(grid_for(h->n)), dim3(kWave), 0, (hipStream_t)stream, P, h->dbase);
    }); });
    HIP_TRY(h, hipGetLastError());
    return PNR_OK;
}

// what the form's argument slot holds (pnr_env_kernels.h): the argument of the slot's role, or nothing
template <int FORM, int SLOT, class Args>
static WorldSlot<FORM, SLOT> slot_value(const Args& args)
{
    constexpr int role = world_role_at(FORM, SLOT);
    if constexpr (role == kWorldRoles) return NoArg{}; else return std::get<role>(args);
}

static const char g_unit_fp[] = "pnr_build_fp:api=" PNR_UNIT_FINGERPRINT ";";

extern "C" {

int pnr_abi_version(void) { return PNR_ABI_VERSION; }

const char* pnr_build_fingerprint(void)
{
    static const std::string joined = [] {                  // every unit's "<tag>=<sha16>;" (past "pnr_build_fp:"), in _lib.UNITS order
        std::string s;
        for (const char* fp : {g_unit_fp, pnr_unit_fingerprint_queries(), pnr_unit_fingerprint_learn()}) s += fp + 13;
        return s;
    }();
    return joined.c_str();
}

int pnr_config_default(pnr_config* c)
{
    if (!c) return fail(nullptr, PNR_ERR_INVALID, "pnr_config_default: null config");
    memset(c, 0, sizeof(*c));
    c->struct_size = (uint32_t)sizeof(pnr_config);
    c->abi_version = PNR_ABI_VERSION;
    // PioneerKinematicConfig, pioneer_knm_env.py:19-34
    c->max_v_to_r = 2; c->max_a_to_v = 10; c->done_distance = 0.1;
    c->award_max = 100.0; c->award_done = 5.0; c->award_potential_slope = 10.0;
    c->penalty_step = 1.0 / 100;
    c->target_lo[0] = 15; c->target_lo[1] = -10; c->target_lo[2] = 2;
    c->target_hi[0] = 25; c->target_hi[1] = 10; c->target_hi[2] = 6;
    c->target_radius = 0.2;
    // SimulationConfig, bullet_env.py:36-41
    c->timestep = 1.0 / 240; c->frame_skip = 10; c->gravity = 0;
    c->max_episode_steps = 500;  // pioneer_knm_train.py:27
    c->auto_reset = 1;
    c->obs_layout = PNR_ENV_MAJOR; c->action_layout = PNR_ENV_MAJOR;
    c->mode = PNR_MODE_KINEMATIC;
    // dynamics mode (no reference values)
    c->pd_kp = 4000.0; c->pd_kd = 400.0; c->torque_limit = 0.0;
    c->joint_damping = 0.0; c->joint_friction = 0.0;
    c->teleport = 0; c->randomize = 0;
    c->rand_mass_lo = 0.5; c->rand_mass_hi = 1.5;
    c->rand_friction_lo = 0.0; c->rand_friction_hi = 0.1;
    c->rand_damping_lo = 0.0; c->rand_damping_hi = 0.1;
    c->ground_z = NAN; c->contact_kp = 2000.0; c->contact_kd = 50.0;
    c->obstacle_position[0] = 10.0; c->obstacle_position[1] = 5.0; c->obstacle_position[2] = 0.0;  // pioneer_knm_env.py:253
    c->obstacle_half_extents[0] = c->obstacle_half_extents[1] = c->obstacle_half_extents[2] = 0.0; // disabled
    c->pointer_radius = 0.2;
    c->control_mode = PNR_CONTROL_POSITION; c->max_velocity = 0.0; c->link_contacts = 0;
    c->n_scene = 0;                                         // scene[] zeroed by the memset above
    c->pd_inertia_scaled = 0;
    return PNR_OK;
}

static int check_config(const pnr_config* c)
{
    if (!c) return fail(nullptr, PNR_ERR_INVALID, "null config");
    if (c->struct_size != sizeof(pnr_config) || c->abi_version != PNR_ABI_VERSION)
        return fail(nullptr, PNR_ERR_INVALID, "pnr_config size/version mismatch (got %u/%u, want %zu/%d)",
                    c->struct_size, c->abi_version, sizeof(pnr_config), PNR_ABI_VERSION);
    if (!(c->timestep > 0) || c->frame_skip < 1)
        return fail(nullptr, PNR_ERR_INVALID, "timestep must be > 0 and frame_skip >= 1");
    if (c->obs_layout != PNR_ENV_MAJOR && c->obs_layout != PNR_FEATURE_MAJOR)
        return fail(nullptr, PNR_ERR_INVALID, "bad obs_layout %d", c->obs_layout);
    if (c->action_layout != PNR_ENV_MAJOR && c->action_layout != PNR_FEATURE_MAJOR)
        return fail(nullptr, PNR_ERR_INVALID, "bad action_layout %d", c->action_layout);
    if (c->mode != PNR_MODE_KINEMATIC && c->mode != PNR_MODE_DYNAMIC)
        return fail(nullptr, PNR_ERR_INVALID, "bad mode %d", c->mode);
    if (c->max_episode_steps < 0) return fail(nullptr, PNR_ERR_INVALID, "max_episode_steps < 0");
    if (c->control_mode != PNR_CONTROL_POSITION && c->control_mode != PNR_CONTROL_VELOCITY)
        return fail(nullptr, PNR_ERR_INVALID, "bad control_mode %d", c->control_mode);
    if (c->max_velocity > 0 && !(c->pd_kd > 0))
        return fail(nullptr, PNR_ERR_INVALID, "max_velocity needs pd_kd > 0 (the cap acts on the velocity the motor asks for)");
    for (int k = 0; k < 3; ++k)
        if (!(c->target_hi[k] >= c->target_lo[k]))
            return fail(nullptr, PNR_ERR_INVALID, "target_hi[%d] < target_lo[%d]", k, k);
    if (c->n_scene < 0 || c->n_scene > PNR_MAX_SCENE)
        return fail(nullptr, PNR_ERR_INVALID, "n_scene %d outside 0..%d", c->n_scene, PNR_MAX_SCENE);
    if (c->n_scene > 0 && c->mode != PNR_MODE_DYNAMIC)
        return fail(nullptr, PNR_ERR_INVALID, "scene bodies collide in dynamics mode only (the kinematic arm passes through everything, as the reference's does)");
    for (int b = 0; b < c->n_scene; ++b) {
        const int rc = check_scene_body(nullptr, "scene body", b, c->scene[b], false);
        if (rc) return rc;
    }
    return PNR_OK;
}

int pnr_get_constants(const pnr_config* c, pnr_constants* out)
{
    int rc = check_config(c);
    if (rc) return rc;
    if (!out) return fail(nullptr, PNR_ERR_INVALID, "pnr_get_constants: null out");
    for (int i = 0; i < kDof; ++i) {
        // joint_limits(): float32 of the URDF limits, pioneer_knm_env.py:217-220
        out->r_lo[i] = (float)(-kJoints[i].limit);
        out->r_hi[i] = (float)(kJoints[i].limit);
        // :57-58  python scalar * float32 array stays float32
        const float span = out->r_hi[i] - out->r_lo[i];
        out->v_max[i] = (float)c->max_v_to_r * span;
        out->a_max[i] = (float)c->max_a_to_v * out->v_max[i];
    }
    out->dt = c->timestep * (double)c->frame_skip;  // bullet_scene.py:277-279
    out->eps = 1e-5;                                // pioneer_knm_env.py:61
    return PNR_OK;
}

static void fill_base(pnr_handle h)
{
    KParams& P = h->base;
    memset(&P, 0, sizeof(P));
    const pnr_config& c = h->cfg;
    P.state = h->state;
    P.n = h->n;
    P.env_off = h->env_off;
    P.T = 1;
    P.max_steps = c.max_episode_steps;
    P.auto_reset = c.auto_reset;
    P.dt = h->k.dt; P.eps = h->k.eps;
    for (int k = 0; k < 3; ++k) { P.tlo[k] = c.target_lo[k]; P.tspan[k] = c.target_hi[k] - c.target_lo[k]; }
    for (int i = 0; i < kDof; ++i) P.v_max[i] = h->k.v_max[i];
    DynParams& D = h->dbase;
    memset(&D, 0, sizeof(D));
    D.dyn = h->dyn;
    D.kp = (float)c.pd_kp; D.kd = (float)c.pd_kd; D.tau_max = (float)c.torque_limit;
    D.gravity = (float)c.gravity; D.dt_sub = (float)c.timestep; D.nsub = c.frame_skip;
    D.teleport = c.teleport; D.randomize = c.randomize;
    D.has_ground = (c.ground_z == c.ground_z) ? 1 : 0;
    D.ground_z = D.has_ground ? (float)c.ground_z : 0.f;
    D.ckp = (float)c.contact_kp; D.ckd = (float)c.contact_kd;
    D.has_box = (c.obstacle_half_extents[0] > 0 && c.obstacle_half_extents[1] > 0 && c.obstacle_half_extents[2] > 0) ? 1 : 0;
    for (int k = 0; k < 3; ++k) { D.box_c[k] = (float)c.obstacle_position[k]; D.box_h[k] = (float)c.obstacle_half_extents[k]; }
    D.ptr_radius = (float)c.pointer_radius;
    const bool velocity = c.control_mode == PNR_CONTROL_VELOCITY;
    D.kp_eff = pd_motor(velocity, c.pd_kp, c.pd_kd, c.torque_limit, c.max_velocity, false).kp;    // the kernels apply teleport themselves
    // pnr_world_step: until a joint is commanded it runs the handle's motor on the env's own r, v
    JointMotor own = pd_motor(velocity, c.pd_kp, c.pd_kd, c.torque_limit, c.max_velocity, c.teleport);
    own.from_cmd = 1;
    D.c_pos = own.cpos; D.v_cap = own.vcap;
    for (int i = 0; i < kDof; ++i) set_motor(h->motors, i, own);
    D.link_contacts = c.link_contacts ? 1 : 0;
    D.inertia_scaled = c.pd_inertia_scaled ? 1 : 0;
    D.n_scene = h->scene ? c.n_scene : 0;
    D.scene = h->scene;
    SceneBody host_scene[kMaxScene];
    for (int b = 0; b < kMaxScene; ++b) {
        SceneBody& S = host_scene[b];
        S = SceneBody{};
        if (b >= c.n_scene) continue;
        S = scene_body_device(c.scene[b]);
    }
    if (h->scene) (void)hipMemcpy(h->scene, host_scene, sizeof(host_scene), hipMemcpyHostToDevice);
    D.joint_damping = (float)c.joint_damping; D.joint_friction = (float)c.joint_friction;
    D.mass_lo = c.rand_mass_lo; D.mass_span = c.rand_mass_hi - c.rand_mass_lo;
    D.fric_lo = c.rand_friction_lo; D.fric_span = c.rand_friction_hi - c.rand_friction_lo;
    D.damp_lo = c.rand_damping_lo; D.damp_span = c.rand_damping_hi - c.rand_damping_lo;
    P.pot_m = (float)(c.award_max - c.award_done);
    P.pot_s = (float)c.award_potential_slope;
    P.penalty = (float)c.penalty_step;
    P.award_done = (float)c.award_done;
    P.done_dist = (float)c.done_distance;
    P.done_dist_d = c.done_distance;
}

int pnr_create(const pnr_config* cfg, int64_t num_envs, int64_t env_id_offset, int device_id,
               uint64_t seed, pnr_handle* out)
{
    if (!out) return fail(nullptr, PNR_ERR_INVALID, "pnr_create: null out");
    *out = nullptr;
    int rc = check_config(cfg);
    if (rc) return rc;
    if (num_envs < 1) return fail(nullptr, PNR_ERR_INVALID, "num_envs must be >= 1 (got %lld)", (long long)num_envs);
    if (env_id_offset < 0) return fail(nullptr, PNR_ERR_INVALID, "env_id_offset < 0");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, PNR_ERR_NODEVICE, "no HIP device visible (this engine has no CPU backend)");
    if (device_id < 0 || device_id >= ndev)
        return fail(nullptr, PNR_ERR_NODEVICE, "device_id %d out of range [0,%d)", device_id, ndev);
    hipDeviceProp_t prop;
    HIP_TRY(nullptr, hipGetDeviceProperties(&prop, device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, PNR_ERR_NODEVICE, "device %d is %s; this library is built for gfx950 only",
                    device_id, prop.gcnArchName);

    for (int i = 0; i < kDof; ++i) {
        // the obs constants of pnr_model.h must be np.cos/np.sin of the float32 limits
        const float c = (float)std::cos((double)limit_hi(i)), s = (float)std::sin((double)limit_hi(i));
        if (c != kLimitCos[i] || s != kLimitSin[i])
            return fail(nullptr, PNR_ERR_INVALID, "model table: cos/sin constants of joint %d are stale", i);
    }

    // the half-built handle is pnr_destroy's on every early return
    struct Destroy { void operator()(pnr_handle p) const { pnr_destroy(p); } };
    std::unique_ptr<pnr_env_s, Destroy> owner(new (std::nothrow) pnr_env_s());
    const pnr_handle h = owner.get();
    if (!h) return fail(nullptr, PNR_ERR_NOMEM, "host allocation failed");
    memset(h, 0, sizeof(*h));
    h->cfg = *cfg;
    h->n = num_envs;
    h->env_off = (unsigned long long)env_id_offset;
    h->device = device_id;
    pnr_get_constants(cfg, &h->k);

    DeviceGuard g(device_id);
    const auto alloc = [](void** p, size_t bytes, const char* what, bool zero) {      // *p stays null unless the memory is there
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes);
        if (e != hipSuccess) return fail(nullptr, PNR_ERR_NOMEM, "hipMalloc(%s) failed: %s", what, hipGetErrorString(e));
        *p = q;
        if (zero) (void)hipMemset(q, 0, bytes);
        return (int)PNR_OK;
    };
    if ((rc = alloc((void**)&h->state, sizeof(float4) * kStatePlanes * 2 * (size_t)num_envs, "state", true))) return rc;
    if (cfg->mode == PNR_MODE_DYNAMIC) {
        if ((rc = alloc((void**)&h->dyn, sizeof(float) * PNR_DYN_STATE_WORDS * (size_t)num_envs, "dyn", true))) return rc;
        if (cfg->n_scene > 0 && (rc = alloc((void**)&h->scene, sizeof(SceneBody) * kMaxScene, "scene", false))) return rc;
    }
    // The zero fills above run on the NULL stream; the caller's first pnr_reset may be issued on a non-blocking stream (every
    // torch.cuda.Stream is one), which is not ordered after NULL-stream work, and reset_env reads the episode counters from
    // these planes.  pnr_create is the one call that synchronises (include/pioneer_amd.h, Conventions): when it returns, the
    // planes are zero for every stream.
    const hipError_t e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return fail(nullptr, PNR_ERR_HIP, "pnr_create: zero fill of the state planes failed: %s", hipGetErrorString(e));
#if PNR_DIAG_BUILD
    { const char* e_ = getenv("PNR_DIAG"); h->diag = e_ ? atoi(e_) : 0; }
#endif
    fill_base(h);
    h->base.seed_lo = (unsigned)seed; h->base.seed_hi = (unsigned)(seed >> 32);
    *out = owner.release();
    return PNR_OK;
}

int pnr_destroy(pnr_handle h)
{
    if (!h) return PNR_OK;
    DeviceGuard g(h->device);
    if (h->state) (void)hipFree(h->state);
    if (h->dyn) (void)hipFree(h->dyn);
    if (h->scene) (void)hipFree(h->scene);
    if (h->sphere.words) (void)hipFree(h->sphere.words);
    if (h->sphere.grip) (void)hipFree(h->sphere.grip);
    delete h;
    return PNR_OK;
}

int pnr_seed(pnr_handle h, uint64_t seed)
{
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    h->base.seed_lo = (unsigned)seed; h->base.seed_hi = (unsigned)(seed >> 32);
    return PNR_OK;
}

int64_t pnr_num_envs(pnr_handle h) { return h ? h->n : -1; }

const char* pnr_last_error(pnr_handle h) { return h ? h->err : g_err; }

// step kernels are persistent over tiles: at most 8 one-wave workgroups per CU (256 CUs)
// Persistent grid of one-wave workgroups.  One launch per step: 2 048 (two waves per SIMD; with a single tile
// per wave the second wave is what overlaps one tile's stores with another's arithmetic).  Long rollouts
// (pnr_rollout, T >= 8): 1 024 = ONE wave per SIMD — a second wave on the SIMD only contends for issue slots
// (a wave's own flush does NOT drain under its next step: the t loop's back edge waits vmcnt(0) for the prefetched
// action, which is queued behind the flush; DESIGN_HISTORY.md) (6.5-7.2 vs 7.2-7.5 us per 65 536-env
// step at T = 32; 768 and 1 536 are worse than either; at T = 2, 4 the 2 048 grid still wins: 8.7 / 8.1 vs
// 10.0 / 8.6 us).  The -DPNR_DIAG_BUILD=1 variant reads overrides from the environment (grid-cap experiments).
// Which form of step_kernel runs is a pure function of (T, n): the ONE-PASS instantiation (a wave = one tile, one step; no
// loops, no prefetch) when T == 1 and grid_for(n) <= the single-step cap of 2 048 waves, i.e. pnr_step at n <= 65 536, where
// every tile has a wave of its own; the general form for everything else (pnr_rollout, batches above 65 536 envs).
static inline unsigned step_grid_for(long long n, int T)
{
#if PNR_DIAG_BUILD
    static int cap = -1, cap_roll = -1;
    if (cap < 0) { const char* e_ = getenv("PNR_GRID_CAP"); cap = e_ ? atoi(e_) : 2048; if (cap < 1) cap = 2048; }
    if (cap_roll < 0) { const char* e_ = getenv("PNR_GRID_CAP_ROLLOUT"); cap_roll = e_ ? atoi(e_) : 1024; if (cap_roll < 1) cap_roll = 1024; }
#else
    constexpr int cap = 2048, cap_roll = 1024;
#endif
    const unsigned tiles = grid_for(n);
    const unsigned c = (unsigned)(T >= 8 ? cap_roll : cap);
    return tiles < c ? tiles : c;
}
static inline bool step_one_pass(long long n, int T) { return T == 1 && step_grid_for(n, T) == grid_for(n); }
// .. and whether the one-pass form takes the row-ordered obs path (obs_tile_rows_out; env-major observations only): when the launch
// has more waves than SIMDs (256 CUs x 4), i.e. 32 768 < n <= 65 536.  There two waves share a SIMD, the launch is bound by its store
// stream and the early flush shortens it (-4.3 % at 65 536 envs, -2.6 % at 49 152); up to one wave per SIMD the longer per-wave
// chain is what the launch waits for (equal at 32 768, +17 % at 16 384, +20 % at 8 192).
constexpr unsigned kOneWavePerSimd = 1024;
static inline bool step_row_pass(long long n, int T) { return step_one_pass(n, T) && grid_for(n) > kOneWavePerSimd; }

int pnr_reset(pnr_handle h, const uint8_t* mask, const float* joint_pos, const float* target_pos,
              float* obs_out, void* stream)
{
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (mask && !h->ready)
        return fail(h, PNR_ERR_INVALID, "the first pnr_reset must be a full one (mask == NULL)");
    if (!mask) h->ready = true;
    KParams P = h->base;
    P.mask = mask; P.joint_pos = joint_pos; P.target_pos = target_pos; P.obs = obs_out;
    const bool fm = h->cfg.obs_layout == PNR_FEATURE_MAJOR;
    return launch_reset<0, 0, 1, 2, 3, 4>(h, P, !obs_out ? 0 : (fm ? (mask ? 1 : 4) : (mask ? 3 : 2)), stream);
}

int pnr_observe(pnr_handle h, float* obs_out, void* stream)
{
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (!obs_out) return fail(h, PNR_ERR_INVALID, "pnr_observe: null obs_out");
    if (!h->ready) return fail(h, PNR_ERR_INVALID, "pnr_observe before the first pnr_reset");
    KParams P = h->base;
    P.obs = obs_out;
    return launch_reset<1, 2, 4>(h, P, h->cfg.obs_layout == PNR_FEATURE_MAJOR ? 4 : 2, stream);
}

static int launch_step(pnr_handle h, int T, const float* actions, float* obs, float* reward,
                       uint8_t* done, uint8_t* truncated, float* info, void* stream)
{
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (!actions || !obs || !reward || !done)
        return fail(h, PNR_ERR_INVALID, "actions, obs, reward and done must be non-null");
    if (T < 1) return fail(h, PNR_ERR_INVALID, "T must be >= 1 (got %d)", T);
    if (!h->ready) return fail(h, PNR_ERR_INVALID, "pnr_step before the first pnr_reset (or pnr_set_state)");
    if (!aligned16(info)) return fail(h, PNR_ERR_INVALID, "info must be 16-byte aligned");
    if (h->cfg.action_layout == PNR_ENV_MAJOR && !aligned8(actions))
        return fail(h, PNR_ERR_INVALID, "env-major actions must be 8-byte aligned");
    DeviceGuard g(h->device);
    KParams P = h->base;
    P.diag = h->diag;
    P.T = T; P.actions = actions; P.obs = obs; P.reward = reward; P.done = done; P.trunc = truncated; P.info = info;
    const dim3 grid((step_grid_for(h->n, T) + kStepWaves - 1) / kStepWaves), block(kWave * kStepWaves);   // the cap counts WAVES
    hipStream_t st = (hipStream_t)stream;
    const DynParams& D = h->dbase;
    const bool oem = h->cfg.obs_layout == PNR_ENV_MAJOR, aem = h->cfg.action_layout == PNR_ENV_MAJOR;
    const float mvr = (float)h->cfg.max_v_to_r;
    with_bool(oem, [&](auto O) { with_bool(aem, [&](auto A) {
        if (h->cfg.mode != PNR_MODE_DYNAMIC) {
            with_bool(step_one_pass(h->n, T), [&](auto S) { with_bool(step_row_pass(h->n, T), [&](auto R) {
                hipLaunchKernelGGL((step_kernel<O(), A(), S(), R() && S() && O()>), grid, block, 0, st, P.state, P.actions, P.n, P.dt,
                                   P.eps, mvr, P);
            }); });
            return;
        }
        // one launch: the dynamics kernels run the sub-steps one env per lane, then finish each step (reward / TimeLimit /
        // auto-reset / obs) as lane pairs, T times.  T > 1: dyn_rollout_kernel loops over the steps inside the launch (state in
        // registers, stores of step t under the sub-steps of t + 1); T == 1: the lean single-step kernel.
        const unsigned wgs = (unsigned)((h->n + kDynEnvsPerWg - 1) / kDynEnvsPerWg);
        // link scales differ from 1 only under randomisation (or after pnr_set_dyn_state, which marks it)
        with_bool(h->cfg.randomize || h->dyn_set, [&](auto R) { with_int<0, 1, 2, 3>(dyn_phys(D), [&](auto C) {
            if (T > 1) hipLaunchKernelGGL((dyn_rollout_kernel<O(), A(), R(), C()>), dim3((wgs + kDynRolloutWaves - 1) / kDynRolloutWaves),
                                          dim3(kWave * kDynRolloutWaves), 0, st, P.state, D.dyn, P.actions, P.n, P.dt, P.eps, mvr, P, D);
            else hipLaunchKernelGGL((dyn_step_kernel<O(), A(), R(), C()>), dim3(wgs), dim3(kWave * kDynStepWaves), 0, st, P.state, D.dyn,
                                    P.actions, P.n, P.dt, P.eps, mvr, P, D);
        }); });
    }); });
    HIP_TRY(h, hipGetLastError());
    return PNR_OK;
}

// PNR_CONTROL_*_CONSTRAINT (the header's second law): everything is checked before the table is touched
static int set_constraint_motor(pnr_handle h, int joint, bool position, double target_position, double target_velocity,
                                double position_gain, double velocity_gain, double max_force, double max_velocity)
{
    if (position ? !std::isfinite(target_position) : !std::isfinite(target_velocity))
        return fail(h, PNR_ERR_INVALID, "pnr_set_joint_motor: the %s target must be finite", position ? "position" : "velocity");
    const double vt = or_default(target_velocity, PNR_BULLET_TARGET_VELOCITY);
    const double kp = or_default(position_gain, PNR_BULLET_POSITION_GAIN), kd = or_default(velocity_gain, PNR_BULLET_VELOCITY_GAIN);
    const double fmax = or_default(max_force, PNR_BULLET_MAX_FORCE), vmax = or_default(max_velocity, PNR_BULLET_MAX_VELOCITY);
    if (!std::isfinite(vt)) return fail(h, PNR_ERR_INVALID, "pnr_set_joint_motor: targetVelocity must be finite");
    if (!std::isfinite(kp) || !std::isfinite(kd) || kp < 0 || kd < 0)
        return fail(h, PNR_ERR_INVALID, "pnr_set_joint_motor: gains must be finite and >= 0 (%g, %g)", kp, kd);
    if (!(fmax >= 0)) return fail(h, PNR_ERR_INVALID, "pnr_set_joint_motor: force must be >= 0 (%g)", fmax);
    JointMotor m = pd_motor(false, 0.0, 0.0, 0.0, 0.0, false);   // fmax == 0, Bullet: no motor, the joint is free (the PD law with zero gains, no cap)
    if (fmax > 0) {
        m.kind = position ? kMotorPositionConstraint : kMotorVelocityConstraint;
        m.kp = (float)kp; m.kd = (float)kd;
        m.vcap = (position && vmax > 0) ? (float)vmax : INFINITY;
        m.tcap = (float)fmax;
        m.r_ref = position ? (float)target_position : 0.f;
        m.v_ref = (float)vt;
    }
    set_motor(h->motors, joint, m);
    return PNR_OK;
}

int pnr_set_joint_motor(pnr_handle h, int joint, int control_mode, double target_position, double target_velocity,
                        double position_gain, double velocity_gain, double max_force, double max_velocity)
{
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (h->cfg.mode != PNR_MODE_DYNAMIC) return fail(h, PNR_ERR_INVALID, "pnr_set_joint_motor: motors exist in dynamics mode only");
    if (joint < 0 || joint >= kDof) return fail(h, PNR_ERR_INVALID, "pnr_set_joint_motor: joint %d out of [0, 6)", joint);
    if (control_mode == PNR_CONTROL_POSITION_CONSTRAINT || control_mode == PNR_CONTROL_VELOCITY_CONSTRAINT)
        return set_constraint_motor(h, joint, control_mode == PNR_CONTROL_POSITION_CONSTRAINT, target_position, target_velocity,
                                    position_gain, velocity_gain, max_force, max_velocity);
    if (control_mode != PNR_CONTROL_POSITION && control_mode != PNR_CONTROL_VELOCITY)
        return fail(h, PNR_ERR_INVALID, "pnr_set_joint_motor: control_mode %d", control_mode);
    const pnr_config& c = h->cfg;
    // an argument left out (NaN) takes the handle's own value
    const double kp = or_default(position_gain, c.pd_kp), kd = or_default(velocity_gain, c.pd_kd);
    const double fmax = or_default(max_force, c.torque_limit), vmax = or_default(max_velocity, c.max_velocity);
    const bool velocity = control_mode == PNR_CONTROL_VELOCITY;
    if (kd <= 0 && !velocity && vmax > 0)
        return fail(h, PNR_ERR_INVALID, "pnr_set_joint_motor: maxVelocity needs velocity_gain > 0");
    JointMotor m = pd_motor(velocity, kp, kd, fmax, velocity ? 0.0 : vmax, false);      // VELOCITY_CONTROL has no maxVelocity
    m.r_ref = velocity ? 0.f : (float)target_position;
    m.v_ref = (float)or_default(target_velocity, 0.0);
    set_motor(h->motors, joint, m);
    return PNR_OK;
}

// The dynamics-mode world step's one launch, for the four calls below (their checks have passed): dyn_world_kernel<RAND, PHYS, form>
// with the call's inputs, its motor table W and, for wrenches, its record table.  `form` is one of the ten listed here; no other
// is instantiated.  With the handle's sphere enabled the torque and the targets form are the ones with kWorldBody (PHYS 1 or 3 only:
// always with contact code), which the plain call takes too, its joint torques null; with the grip enabled as well
// (pnr_set_body_grip_params) those two with kWorldGrip, and with it disabled or never enabled the two without: the kernels of a handle
// that knows no grip.  (Always the instantiation that reads the per-env link scales: without randomisation they are stored as 1.)
struct WorldStepInputs {
    const float* targets = nullptr; unsigned mask = 0;      // pnr_world_step_targets
    const float* tau_ext = nullptr;
    const float* wrenches = nullptr; LinkWrenchTable T = {};   // pnr_world_step_wrenches
};

static int launch_world_step(pnr_handle h, int form, const JointMotorTable& W, const WorldStepInputs& in, void* stream)
{
    DeviceGuard g(h->device);
    const dim3 grid((unsigned)((h->n + kWave - 1) / kWave));
    bool launched = false;
    int phys = dyn_phys(h->dbase);
    WorldGrip body = h->sphere;
    if (h->sphere_on) { form |= kWorldBody | kWorldTorque | (h->grip_on ? kWorldGrip : 0); phys |= 1; body.joint_mask = in.mask; }
    // (forms outermost, in this order: the compiler emits the instantiations in the reverse of it)
    const auto args = std::make_tuple(in.wrenches, in.targets, in.tau_ext, in.mask, h->dbase, W, in.T, static_cast<const WorldBody&>(body), body);      // by WorldRole
    with_int<kWorldGrip | kWorldBody | kWorldTargets | kWorldTorque, kWorldGrip | kWorldBody | kWorldTorque,
             kWorldBody | kWorldTargets | kWorldTorque, kWorldBody | kWorldTorque, kWorldWrench | kWorldTorque, kWorldTargets | kWorldTorque,
             kWorldTargets | kWorldCMotor, kWorldTorque, 0, kWorldCMotor>(form, [&](auto F_) {
        constexpr int F = decltype(F_)::value;
        const auto launch = [&](auto C) {
            hipLaunchKernelGGL((dyn_world_kernel<true, C(), F>), grid, dim3(kWave), 0, (hipStream_t)stream, h->state, h->dyn, (long long)h->n,
                               slot_value<F, 0>(args), slot_value<F, 1>(args), slot_value<F, 2>(args), slot_value<F, 3>(args), slot_value<F, 4>(args));
            launched = true;
        };
        if constexpr ((F & kWorldBody) != 0) with_int<1, 3>(phys, launch); else with_int<0, 1, 2, 3>(phys, launch);
    });
    if (!launched) return fail(h, PNR_ERR_INVALID, "world step: form %d is not built", form);
    HIP_TRY(h, hipGetLastError());
    return PNR_OK;
}

// joint torques or wrenches (`input`) next to a constraint motor on `joint`
static int refuse_constraint_motor(pnr_handle h, const char* call, int joint, const char* input)
{
    return fail(h, PNR_ERR_UNSUPPORTED, "%s: joint %d is on a constraint motor (%s input with the boxed solve is not built)", call, joint, input);
}

int pnr_world_step(pnr_handle h, float* joint_state, void* stream)
{
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (!h->ready) return fail(h, PNR_ERR_INVALID, "pnr_world_step before the first pnr_reset (or pnr_set_state)");
    if (h->cfg.mode != PNR_MODE_DYNAMIC) {
        if (!joint_state) return fail(h, PNR_ERR_INVALID, "pnr_world_step: a kinematic-mode handle steps the caller's joint_state [n][12]");
        DeviceGuard g(h->device);
        const long long items = h->n * kDof;
        hipLaunchKernelGGL(kin_world_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, joint_state, (long long)h->n, (float)h->k.dt);
        HIP_TRY(h, hipGetLastError());
        return PNR_OK;
    }
    if (joint_state) return fail(h, PNR_ERR_INVALID, "pnr_world_step: joint_state must be NULL in dynamics mode (the simulated joints are the handle's)");
    if (h->sphere_on && has_constraint_motor(h)) return refuse_sphere(h, "pnr_world_step", "a constraint motor");
    return launch_world_step(h, has_constraint_motor(h) ? kWorldCMotor : 0, h->motors, {}, stream);
}

int pnr_world_step_torques(pnr_handle h, const float* joint_torques, void* stream)
{
    const char* call = "pnr_world_step_torques";
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (h->cfg.mode != PNR_MODE_DYNAMIC) return fail(h, PNR_ERR_UNSUPPORTED, "%s: joint torques exist in dynamics mode only", call);
    if (!joint_torques) return fail(h, PNR_ERR_INVALID, "%s: null joint_torques", call);
    if (const int rc = check_aligned(h, call, {{joint_torques, "joint_torques", 16}})) return rc;
    if (!h->ready) return fail(h, PNR_ERR_INVALID, "%s before the first pnr_reset (or pnr_set_state)", call);
    int joint;
    if (has_constraint_motor(h, &joint)) return refuse_constraint_motor(h, call, joint, "torque");
    WorldStepInputs in;
    in.tau_ext = joint_torques;
    return launch_world_step(h, kWorldTorque, h->motors, in, stream);
}

int pnr_world_step_targets(pnr_handle h, uint32_t joint_mask, const float* targets, const float* joint_torques, void* stream)
{
    const char* call = "pnr_world_step_targets";
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "%s: null handle", call);
    if (h->cfg.mode != PNR_MODE_DYNAMIC) return fail(h, PNR_ERR_UNSUPPORTED, "%s: joint motors exist in dynamics mode only", call);
    if (!targets) return fail(h, PNR_ERR_INVALID, "%s: null targets", call);
    if (const int rc = check_aligned(h, call, {{targets, "targets", 16}, {joint_torques, "joint_torques", 16}})) return rc;
    if (joint_mask == 0 || joint_mask >> kDof)
        return fail(h, PNR_ERR_INVALID, "%s: joint_mask 0x%x must name at least one of joints 0..5 and no other bit", call, joint_mask);
    if (!h->ready) return fail(h, PNR_ERR_INVALID, "%s before the first pnr_reset (or pnr_set_state)", call);
    int joint;
    const bool cm = has_constraint_motor(h, &joint);
    if (cm && joint_torques) return refuse_constraint_motor(h, call, joint, "torque");
    if (cm && h->sphere_on) return refuse_sphere(h, call, "a constraint motor");
    // this call's table: the masked joints track the lane's r, v, where the kernel puts the env's targets; h->motors stays as it is
    JointMotorTable W = h->motors;
    for (int i = 0; i < kDof; ++i)
        if ((joint_mask >> i) & 1u) W.from_cmd[i] = 1;
    WorldStepInputs in;
    in.targets = targets; in.mask = joint_mask; in.tau_ext = joint_torques;
    return launch_world_step(h, kWorldTargets | (cm ? kWorldCMotor : kWorldTorque), W, in, stream);
}

int pnr_world_step_wrenches(pnr_handle h, const pnr_link_wrench_spec* specs, int n_specs, const float* wrenches,
                            const float* joint_torques, int hold_substeps, void* stream)
{
    const char* call = "pnr_world_step_wrenches";
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "null handle");
    if (h->cfg.mode != PNR_MODE_DYNAMIC) return fail(h, PNR_ERR_UNSUPPORTED, "%s: link wrenches exist in dynamics mode only", call);
    if (!specs) return fail(h, PNR_ERR_INVALID, "%s: null specs", call);
    if (!wrenches) return fail(h, PNR_ERR_INVALID, "%s: null wrenches", call);
    if (const int rc = check_aligned(h, call, {{wrenches, "wrenches", 16}, {joint_torques, "joint_torques", 16}})) return rc;
    WorldStepInputs in;
    if (const int rc = fill_wrench_table(h, call, specs, n_specs, in.T)) return rc;      // (pnr_env_host.h)
    if (!h->ready) return fail(h, PNR_ERR_INVALID, "%s before the first pnr_reset (or pnr_set_state)", call);
    int joint;
    if (has_constraint_motor(h, &joint)) return refuse_constraint_motor(h, call, joint, "wrench");
    if (h->sphere_on) return refuse_sphere(h, call, "link wrenches");
    const int nsub = h->dbase.nsub;
    in.T.hold = (hold_substeps <= 0 || hold_substeps >= nsub) ? nsub : hold_substeps;
    in.wrenches = wrenches; in.tau_ext = joint_torques;
    return launch_world_step(h, kWorldWrench | kWorldTorque, h->motors, in, stream);
}

int pnr_body_params_default(pnr_body_params* p)
{
    if (!p) return fail(nullptr, PNR_ERR_INVALID, "pnr_body_params_default: null params");
    *p = pnr_body_params{(uint32_t)sizeof(pnr_body_params), NAN, NAN, 0.5f, kFrictionEps, 0.f};
    return PNR_OK;
}

int pnr_set_body_params(pnr_handle h, const pnr_body_params* p)
{
    const char* call = "pnr_set_body_params";
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "%s: null handle", call);
    if (h->cfg.mode != PNR_MODE_DYNAMIC) return fail(h, PNR_ERR_UNSUPPORTED, "%s: the moving sphere exists in dynamics mode only", call);
    if (!p) { h->sphere_on = false; return PNR_OK; }
    if (p->struct_size != sizeof(pnr_body_params))
        return fail(h, PNR_ERR_INVALID, "%s: struct_size %u, want %zu", call, p->struct_size, sizeof(pnr_body_params));
    const float kp = p->contact_kp == p->contact_kp ? p->contact_kp : (float)h->cfg.contact_kp;
    const float kd = p->contact_kd == p->contact_kd ? p->contact_kd : (float)h->cfg.contact_kd;
    const float all[5] = {kp, kd, p->friction, p->slip_eps, p->linear_damping};
    if (!finite_all(all, 5)) return fail(h, PNR_ERR_INVALID, "%s: non-finite parameter", call);
    if (!(kp > 0) || kd < 0) return fail(h, PNR_ERR_INVALID, "%s: contact_kp must be > 0 and contact_kd >= 0 (%g, %g)", call, kp, kd);
    if (p->friction < 0 || p->linear_damping < 0 || !(p->slip_eps > 0))
        return fail(h, PNR_ERR_INVALID, "%s: friction and linear_damping must be >= 0 and slip_eps > 0 (%g, %g, %g)", call, p->friction,
                    p->linear_damping, p->slip_eps);
    if (!h->sphere.words) {
        DeviceGuard g(h->device);
        const size_t bytes = sizeof(float) * PNR_BODY_STATE_WORDS * (size_t)h->n;
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, bytes);
        if (e != hipSuccess) return fail(h, PNR_ERR_NOMEM, "%s: hipMalloc(sphere) failed: %s", call, hipGetErrorString(e));
        // zero = mass 0 = no sphere in any env; waited for, as pnr_create waits for its fill (a set_body_state on a non-blocking
        // stream is not ordered after NULL-stream work)
        e = hipMemset(q, 0, bytes);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) { (void)hipFree(q); return fail(h, PNR_ERR_HIP, "%s: zero fill of the sphere buffer failed: %s", call, hipGetErrorString(e)); }
        h->sphere.words = (float*)q;
    }
    h->sphere.kp = kp; h->sphere.kd = kd; h->sphere.friction = p->friction; h->sphere.slip_eps = p->slip_eps;
    h->sphere.linear_damping = p->linear_damping;
    h->sphere_on = true;
    return PNR_OK;
}

// the argument checks of pnr_set_body_state / pnr_get_body_state
static int check_body_state_call(pnr_handle h, const void* words, const char* name, const char* call)
{
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "%s: null handle", call);
    if (!h->sphere.words) return fail(h, PNR_ERR_INVALID, "%s before pnr_set_body_params (the handle has no sphere buffer)", call);
    if (!words) return fail(h, PNR_ERR_INVALID, "%s: null %s", call, name);
    return check_aligned(h, call, {{words, name, 16}});
}

int pnr_set_body_state(pnr_handle h, const float* words, const uint8_t* mask, void* stream)
{
    if (const int rc = check_body_state_call(h, words, "words", "pnr_set_body_state")) return rc;
    DeviceGuard g(h->device);
    hipLaunchKernelGGL(body_set_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->sphere.words, words, mask,
                       (long long)h->n);
    HIP_TRY(h, hipGetLastError());
    return PNR_OK;
}

int pnr_get_body_state(pnr_handle h, float* out, void* stream)
{
    if (const int rc = check_body_state_call(h, out, "out", "pnr_get_body_state")) return rc;
    DeviceGuard g(h->device);
    const size_t bytes = sizeof(float) * PNR_BODY_STATE_WORDS * (size_t)h->n;      // (outside HIP_TRY, which quotes its argument in the message)
    HIP_TRY(h, hipMemcpyAsync(out, h->sphere.words, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PNR_OK;
}

int pnr_body_grip_params_default(pnr_body_grip_params* p)
{
    if (!p) return fail(nullptr, PNR_ERR_INVALID, "pnr_body_grip_params_default: null params");
    // direction: the unit vector along the tip offset, so that the held sphere sits tangent to the pointer's own sample sphere
    const double tl = std::sqrt(kTipX * kTipX + kTipY * kTipY + kTipZ * kTipZ);
    *p = pnr_body_grip_params{(uint32_t)sizeof(pnr_body_grip_params), {0.f, 0.f, 0.f},
                              {(float)(kTipX / tl), (float)(kTipY / tl), (float)(kTipZ / tl)}, NAN, NAN};
    return PNR_OK;
}

int pnr_set_body_grip_params(pnr_handle h, const pnr_body_grip_params* p)
{
    const char* call = "pnr_set_body_grip_params";
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "%s: null handle", call);
    if (h->cfg.mode != PNR_MODE_DYNAMIC) return fail(h, PNR_ERR_UNSUPPORTED, "%s: the moving sphere exists in dynamics mode only", call);
    if (!h->sphere.words) return fail(h, PNR_ERR_INVALID, "%s before pnr_set_body_params (the handle has no sphere buffer)", call);
    if (!p) { h->grip_on = false; return PNR_OK; }
    if (p->struct_size != sizeof(pnr_body_grip_params))
        return fail(h, PNR_ERR_INVALID, "%s: struct_size %u, want %zu", call, p->struct_size, sizeof(pnr_body_grip_params));
    const float kp = p->grip_kp == p->grip_kp ? p->grip_kp : h->sphere.kp;
    const float kd = p->grip_kd == p->grip_kd ? p->grip_kd : h->sphere.kd;
    const float all[8] = {kp, kd, p->anchor[0], p->anchor[1], p->anchor[2], p->direction[0], p->direction[1], p->direction[2]};
    if (!finite_all(all, 8)) return fail(h, PNR_ERR_INVALID, "%s: non-finite parameter", call);
    if (!(kp > 0) || kd < 0) return fail(h, PNR_ERR_INVALID, "%s: grip_kp must be > 0 and grip_kd >= 0 (%g, %g)", call, kp, kd);
    // the direction: zero (the anchor is a plain point of the link) or normalised here, in double
    const double dv[3] = {p->direction[0], p->direction[1], p->direction[2]};
    const double dl = std::sqrt(sum_sq(dv, 3));
    const bool zero = dv[0] == 0 && dv[1] == 0 && dv[2] == 0;
    if (!zero && !(dl > 1e-6 && std::isfinite(dl)))
        return fail(h, PNR_ERR_INVALID, "%s: direction (%g, %g, %g) is neither zero nor normalisable", call, dv[0], dv[1], dv[2]);
    if (!h->sphere.grip) {
        DeviceGuard g(h->device);
        const size_t bytes = sizeof(float) * PNR_BODY_GRIP_WORDS * (size_t)h->n;
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, bytes);
        if (e != hipSuccess) return fail(h, PNR_ERR_NOMEM, "%s: hipMalloc(grip) failed: %s", call, hipGetErrorString(e));
        // zero = max_force 0 = every env released; waited for, as the sphere buffer's fill is
        e = hipMemset(q, 0, bytes);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) { (void)hipFree(q); return fail(h, PNR_ERR_HIP, "%s: zero fill of the grip buffer failed: %s", call, hipGetErrorString(e)); }
        h->sphere.grip = (float*)q;
    }
    h->sphere.grip_kp = kp; h->sphere.grip_kd = kd;
    for (int k = 0; k < 3; ++k) {
        h->sphere.anchor[k] = p->anchor[k];
        h->sphere.direction[k] = zero ? 0.f : (float)(dv[k] / dl);
    }
    h->grip_on = true;
    return PNR_OK;
}

// the argument checks of pnr_set_body_grip / pnr_get_body_grip
static int check_body_grip_call(pnr_handle h, const void* p, const char* name, unsigned align, const char* call)
{
    if (!h) return fail(nullptr, PNR_ERR_INVALID, "%s: null handle", call);
    if (!h->sphere.grip) return fail(h, PNR_ERR_INVALID, "%s before pnr_set_body_grip_params (the handle has no grip buffer)", call);
    if (!p) return fail(h, PNR_ERR_INVALID, "%s: null %s", call, name);
    return check_aligned(h, call, {{p, name, align}});
}

int pnr_set_body_grip(pnr_handle h, const float* max_force, const uint8_t* mask, void* stream)
{
    if (const int rc = check_body_grip_call(h, max_force, "max_force", 4, "pnr_set_body_grip")) return rc;
    DeviceGuard g(h->device);
    hipLaunchKernelGGL(grip_set_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->sphere.grip, max_force, mask,
                       (long long)h->n);
    HIP_TRY(h, hipGetLastError());
    return PNR_OK;
}

int pnr_get_body_grip(pnr_handle h, float* out, void* stream)
{
    if (const int rc = check_body_grip_call(h, out, "out", 16, "pnr_get_body_grip")) return rc;
    DeviceGuard g(h->device);
    const size_t bytes = sizeof(float) * PNR_BODY_GRIP_WORDS * (size_t)h->n;
    HIP_TRY(h, hipMemcpyAsync(out, h->sphere.grip, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PNR_OK;
}

}  // extern "C"

int pnr_env_rollout_params(pnr_handle h, pnr::KParams* out, float* max_v_to_r, int* device)
{
    if (!h || !out || !max_v_to_r || !device) return fail(nullptr, PNR_ERR_INVALID, "pnr_ppo_rollout: null handle");
    if (h->cfg.mode != PNR_MODE_KINEMATIC)
        return fail(h, PNR_ERR_INVALID, "pnr_ppo_rollout runs kinematic-mode handles (dynamics mode: pnr_mlp_act + pnr_step per step)");
    if (h->cfg.obs_layout != PNR_ENV_MAJOR || h->cfg.action_layout != PNR_ENV_MAJOR)
        return fail(h, PNR_ERR_INVALID, "pnr_ppo_rollout needs env-major observations and actions");
    if (!h->ready) return fail(h, PNR_ERR_INVALID, "pnr_ppo_rollout before the first pnr_reset (or pnr_set_state)");
    *out = h->base;
    out->diag = 0;
    *max_v_to_r = (float)h->cfg.max_v_to_r;
    *device = h->device;
    return PNR_OK;
}

extern "C" {

int pnr_step(pnr_handle h, const float* actions, float* obs, float* reward, uint8_t* done,
             uint8_t* truncated, float* info, void* stream)
{
    return launch_step(h, 1, actions, obs, reward, done, truncated, info, stream);
}

int pnr_rollout(pnr_handle h, int32_t T, const float* actions, float* obs, float* reward,
                uint8_t* done, uint8_t* truncated, void* stream)
{
    return launch_step(h, T, actions, obs, reward, done, truncated, nullptr, stream);
}

int pnr_diag_sincos(const float* x, float* sin_out, float* cos_out, int64_t n, int bounded, void* stream)
{
    if (!x || !sin_out || !cos_out || n < 0) return fail(nullptr, PNR_ERR_INVALID, "pnr_diag_sincos: bad argument");
    if (n == 0) return PNR_OK;
    hipLaunchKernelGGL(diag_sincos_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       x, sin_out, cos_out, (long long)n, bounded);
    HIP_TRY(nullptr, hipGetLastError());
    return PNR_OK;
}

int pnr_get_state(pnr_handle h, uint32_t* words_out, void* stream)
{
    if (const int rc = check_state_call(h, words_out, "pnr_get_state", false)) return rc;
    DeviceGuard g(h->device);
    hipLaunchKernelGGL(state_to_words_kernel, dim3((unsigned)((2 * h->n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, h->state, words_out, h->n);
    HIP_TRY(h, hipGetLastError());
    return PNR_OK;
}

int pnr_set_state(pnr_handle h, const uint32_t* words_in, void* stream)
{
    if (const int rc = check_state_call(h, words_in, "pnr_set_state", false)) return rc;
    DeviceGuard g(h->device);
    h->kin_set = true;
    if (!h->dyn || h->dyn_set) h->ready = true;
    hipLaunchKernelGGL(words_to_state_kernel, dim3((unsigned)((2 * h->n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, h->state, words_in, h->n);
    HIP_TRY(h, hipGetLastError());
    return PNR_OK;
}

int pnr_get_dyn_state(pnr_handle h, float* words_out, void* stream)
{
    if (const int rc = check_state_call(h, words_out, "pnr_get_dyn_state", true)) return rc;
    DeviceGuard g(h->device);
    const size_t bytes = sizeof(float) * PNR_DYN_STATE_WORDS * (size_t)h->n;
    HIP_TRY(h, hipMemcpyAsync(words_out, h->dyn, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PNR_OK;
}

int pnr_set_dyn_state(pnr_handle h, const float* words_in, void* stream)
{
    if (const int rc = check_state_call(h, words_in, "pnr_set_dyn_state", true)) return rc;
    DeviceGuard g(h->device);
    h->dyn_set = true;
    if (h->kin_set) h->ready = true;
    const size_t bytes = sizeof(float) * PNR_DYN_STATE_WORDS * (size_t)h->n;
    HIP_TRY(h, hipMemcpyAsync(h->dyn, words_in, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PNR_OK;
}

}  // extern "C"
