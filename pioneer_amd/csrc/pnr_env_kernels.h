// pnr_env_kernels.h — the env-side kernels of the engine: step / rollout (kinematic), the dynamics-mode step and rollout
// kernels, reset / observe, and the state-layout converters.  Included by pnr_api.hip only (which holds the C ABI and the
// launches); kept in a file of its own so that the counter passes under profiles/ can be tied to exactly the sources that
// define these kernels (pioneer_amd._lib.source_fingerprint, bench.py's `roofline.traffic`).
//
// Execution shape: see the header of pnr_api.hip and DESIGN.md section 3.
#pragma once

#include <hip/hip_runtime.h>

#include <tuple>

#include "pnr_device.h"
#include "pnr_dyn.h"

#ifndef PNR_DIAG_BUILD
#define PNR_DIAG_BUILD 0
#endif

namespace pnr {

// ---------------------------------------------------------------------------------
// The outcome of one env step, for the kinematic and the dynamics kernels alike: the reward block of
// pioneer_knm_env.py:157-165 and gym.wrappers.TimeLimit.  Both lanes of a pair compute the same.
// ---------------------------------------------------------------------------------
struct Outcome { float pot, r_pot, r_step, r_done, rw; bool done, trunc; };

// `o`: what the reward sees — this lane's joints, the env's target, its potential before the step and its step count after it
template <bool DYN>
__device__ __forceinline__ Outcome step_outcome(const KParams& P, const LaneState& o, int p, float dist)
{
    Outcome c;
    c.pot = P.pot_m / (dist / P.pot_s + 1.0f);                    // :232-236
    c.done = done_predicate(o, p, dist, P.done_dist, P.done_dist_d);   // :160
    c.r_pot = c.pot - o.pot;
    c.r_step = -P.penalty;
    c.r_done = c.done ? P.award_done : 0.0f;
    c.rw = (c.r_pot + c.r_step) + c.r_done;                       // :165
    // gym.wrappers.TimeLimit: truncated = elapsed >= max and not done
    c.trunc = (P.max_steps > 0) && (o.step >= (uint32_t)P.max_steps) && !c.done;
    // a lane whose simulation diverged (non-finite pose) is cut like a time-out, so auto-reset recovers
    // it instead of carrying NaNs forever (kinematic mode keeps the reference's NaN-propagating behaviour)
    if (DYN && !(dist == dist && __builtin_fabsf(dist) <= 3.0e38f)) c.trunc = !c.done;
    return c;
}

// the env's four results at output index o = t * n + e (one lane of the pair)
__device__ __forceinline__ void store_outcome(const KParams& P, const Outcome& c, float dist, long long o)
{
    stream_store(P.reward + o, c.rw);
    stream_store(P.done + o, (uint8_t)c.done);
    if (P.trunc) stream_store(P.trunc + o, (uint8_t)c.trunc);
    if (P.info) stream_store(reinterpret_cast<float4*>(P.info) + o, make_float4(c.r_pot, c.r_step, c.r_done, dist));
}

// ---------------------------------------------------------------------------------
// step / rollout kernel: BulletEnv.step (bullet_env.py:192-197) for T steps.
// One wave = 32 envs (lane pair per env), one wave per workgroup.
// ---------------------------------------------------------------------------------
// The leading scalar parameters repeat P.state / P.actions / P.n / P.dt / P.eps and carry max_v_to_r (v_max
// is formed from it and the constexpr limits): plain leading arguments (up to 14 dwords) are preloaded into SGPRs by the command processor (-mllvm
// -amdgpu-kernarg-preload-count), so neither the first state and action loads nor the integrator wait for
// a kernarg fetch; the by-value struct, needed from the reward block on, is fetched behind them.
// PNR_STEP_WAVES waves per workgroup (default 4).  The waves of a workgroup share nothing — each has its own obs tile and walks its
// own tiles, no barrier — so this only changes what the dispatcher places: with four-wave workgroups a rollout's 1 024 waves are 256
// workgroups = exactly one per CU, one wave per SIMD, where 1 024 one-wave workgroups landed unevenly (A/B r03 in one run, twice:
// 7.36 -> 6.33 us per rollout step at 65 536 envs; single steps unchanged, 10.38 vs 10.31 us).
// Two forms of one body (which runs when: step_one_pass, pnr_api.hip).  The GENERAL form is persistent: a wave strides over tiles
// and loops over the T steps of a launch, with the next tile's and the next step's loads requested ahead of the stores.  ONE_PASS
// folds both loops and the prefetch blocks away — a wave is one tile and one step, T is the literal 1 — for pnr_step at
// n <= 65 536, where every tile has a wave of its own, all 2 048 waves walk load / compute / emit / flush in lock-step and the head
// is paid in full.  What the loops cost there is everything LLVM hoists in front of them (the reset path's Philox key schedule,
// prefetch addresses, rollout strides): gfx950 listing, <true, true>: 447 instructions between the first loads and the integrator,
// 193 VGPRs, 106 SGPRs and 92 v_writelane / v_readlane scalar spills in the general form; 48 instructions (the tile's 36 constant
// entries among them), 119 VGPRs, 74 SGPRs and no spill in the one-pass form.  Both forms request the state record's four parts and the
// first action back to back, fetch P's scalars and write the constants behind them, and wait first for plane 0 alone.  The
// integrator takes the lane's three joints side by side (integrate_joints3, pnr_device.h: one branch, three interleaved f64 division
// chains, where three nested exec-mask regions per joint ran one after the other).  The new action: the general form waits for it
// where the state store consumes it; the one-pass form right behind the integrator, in front of every store of the step, so that no
// `s_waitcnt vmcnt` stands behind a store (it would wait for that store's acknowledgement) anywhere between the first outcome store
// and the first obs store.  ROW_PASS (one-pass form, env-major observations, more than one wave per
// SIMD: step_row_pass, pnr_api.hip) also starts the obs stores early: the tile's sin / cos are evaluated in row order with the
// flush under them (obs_tile_rows_out, pnr_device.h; what that pass derives from the lane id alone is formed in the head, under
// the first loads); every other launch emits a lane's half row at once (obs_tile_out).
#ifndef PNR_STEP_WAVES
#define PNR_STEP_WAVES 4
#endif
constexpr int kStepWaves = PNR_STEP_WAVES;

template <bool OBS_EM, bool ACT_EM, bool ONE_PASS = false, bool ROW_PASS = false>
__global__ __launch_bounds__(kWave * kStepWaves) void step_kernel(float4* __restrict__ state_, const float* __restrict__ actions_,
                                                     const long long n_, const double dt_, const double eps_,
                                                     const float max_v_to_r_, const KParams P)
{
    static_assert(!ROW_PASS || (OBS_EM && ONE_PASS), "the row-ordered obs path belongs to the one-pass form with an env-major tile");
    __shared__ __attribute__((aligned(16))) float tiles_[kStepWaves * kTileFloats];
    float* tile = tiles_ + (threadIdx.x >> 6) * kTileFloats;

    const int lane = threadIdx.x & (kWave - 1);
    const int p = lane & 1;                 // which half of the env's joints
    const int el = lane >> 1;               // env within the wave's tile
    const long long n = n_;
    const long long ntiles = (n + kEnvsPerWave - 1) / kEnvsPerWave;

    // timing-only ablations (outputs are wrong when set; DESIGN.md "Where the time goes"): compiled in by -DPNR_DIAG_BUILD=1
    // only — in the product library `diag` is the literal 0 and every branch on it folds away
    const int diag = PNR_DIAG_BUILD ? P.diag : 0;
    const bool diag_noflush = diag & 2, diag_noemit = diag & 4, diag_nostate = diag & 8;

    const LaneConsts K = lane_consts(p);
    // v_max = max_v_to_r * (r_hi - r_lo) (pioneer_knm_env.py:57), the same float32 product pnr_get_constants forms
    const float vmax[kJpl] = {max_v_to_r_ * (K.lim[0] - (-K.lim[0])), max_v_to_r_ * (K.lim[1] - (-K.lim[1])),
                              max_v_to_r_ * (K.lim[2] - (-K.lim[2]))};

    // Persistent tile loop: the grid is capped (host: <= 8 waves per CU) and every wave strides over
    // tiles.  The NEXT tile's state and first action are requested before the current tile is
    // processed, so they never queue behind this CU's own obs stores.
    const auto load_act0 = [&](long long e_, float (&a_)[kJpl]) {
        if (ACT_EM) {
            const float* a3 = actions_ + e_ * kDof + kJpl * p;         // 12 B per lane, lanes contiguous
            a_[0] = a3[0]; a_[1] = a3[1]; a_[2] = a3[2];
        } else {
#pragma unroll
            for (int i = 0; i < kJpl; ++i) a_[i] = actions_[(long long)(kJpl * p + i) * n + e_];
        }
    };

    const long long tstride = (long long)gridDim.x * kStepWaves;
    long long tix = (long long)blockIdx.x * kStepWaves + (threadIdx.x >> 6);
    if (tix >= ntiles) return;              // a whole wave past the last tile (no barrier follows in this kernel)

    // The head of the launch.  Every wave of a launch is here at the same time and HBM idles until the first flush, so what
    // stands between kernel entry and the integrator is paid in full: the state record's four parts (planes 0 and 1, hot half,
    // cold part: the integrator waits for the first three only) and the first action are requested back to back, with no branch
    // round them (the join's register copies would wait for the first plane before the last load is out): a lane past the end
    // reads the tile's first env again — in bounds, and nothing of such a lane is ever stored.
    RawState raw;
    float act0[kJpl];
    {
        const bool in = tix * kEnvsPerWave + el < n;
        raw = load_state_raw(state_, n, 2 * tix * kEnvsPerWave + (in ? lane : p));
        load_act0(tix * kEnvsPerWave + (in ? el : 0), act0);
        __builtin_amdgcn_sched_barrier(0);  // nothing that needs a loaded value is scheduled in between
    }
    bool first_tile = true;

    // the 36 constant obs entries of this lane's tile slots: once per kernel, under the load latency
    obs_tile_const<OBS_EM>(K, tile, el, p);
    // .. and where the row pass finds this lane's trig arguments and tail columns: integer work on the lane id alone; the asm keeps
    // the results in registers from here on (unpinned, the `/ 24` arithmetic is sunk back between the state stores and the first
    // obs store, where every wave of the launch pays for it with HBM idle)
    RowPassLane rowl = {};
    if (ROW_PASS) {
        rowl = row_pass_lane(lane);
        asm volatile("" : "+v"(rowl.off[0]), "+v"(rowl.off[1]), "+v"(rowl.off[2]), "+v"(rowl.tail));
    }
    if (ONE_PASS) {
        // .. and so are the common path's words of P: asked for here, they are scalar loads issued before the first vmcnt wait;
        // the barrier keeps the integrator's converts (and with them that wait) below the constants
        asm volatile("" :: "s"(P.obs), "s"(P.reward), "s"(P.done), "s"(P.trunc), "s"(P.info), "s"(P.max_steps), "s"(P.auto_reset),
                     "s"(P.pot_m), "s"(P.pot_s), "s"(P.penalty), "s"(P.award_done), "s"(P.done_dist), "s"(P.done_dist_d));
        __builtin_amdgcn_sched_barrier(0);
    }

    const int T = ONE_PASS ? 1 : P.T;
    for (; tix < ntiles; tix += tstride) {  // ONE_PASS: left at the end of the first pass, i.e. a plain `if` (true here)
    const long long tile0 = tix * kEnvsPerWave;
    const long long e = tile0 + el;
    const long long rec = 2 * tile0 + lane; // state record index (2e + p)
    const bool valid = e < n;               // the pair shares `valid`, so DPP partners are live
    const int nvalid = (int)((n - tile0) < kEnvsPerWave ? (n - tile0) : kEnvsPerWave);

    LaneState s;
    unpack_state(raw, p, s);                // lanes past the end: the tile's first env (first tile) or all-zero records
    float act_first[kJpl] = {act0[0], act0[1], act0[2]};

    // prefetch the next tile (ONE_PASS: there is none)
    if (!ONE_PASS) {
        const long long nt = tix + tstride;
        if (nt < ntiles && nt * kEnvsPerWave + el < n) {
            raw = load_state_raw(state_, n, 2 * nt * kEnvsPerWave + lane);
            load_act0(nt * kEnvsPerWave + el, act0);
        } else {
            raw = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), make_float2(0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
        }
    }

    if (diag & 16) {                                               // launch + state-load floor
        if (valid) P.reward[e] = s.pot;
        if (ONE_PASS) break;                                       // .. the one-pass form's `continue`
        continue;
    }

    bool cold = false;                      // some step of this launch reset the env: its target and episode go out with the state
    for (int t = 0; t < T; ++t) {
        {
            // -- action of this step (this lane's three joints) ----------------------
            // this step's action was requested one step (or one tile) ago; request the next one now,
            // ahead of this step's obs stores (VMEM ops of a wave retire in order)
            float act[kJpl] = {act_first[0], act_first[1], act_first[2]};
            if (t + 1 < T && valid) {
                const float* A = actions_ + (long long)(t + 1) * n * kDof;
                if (ACT_EM) {
                    const float* a3 = A + e * kDof + kJpl * p;
                    act_first[0] = a3[0]; act_first[1] = a3[1]; act_first[2] = a3[2];
                } else {
#pragma unroll
                    for (int i = 0; i < kJpl; ++i) act_first[i] = A[(long long)(kJpl * p + i) * n + e];
                }
            }
            // -- act(): integrate the PREVIOUS action, then latch the new one -------
            if (!(diag & 32)) integrate_joints3(s.a, s.v, s.r, vmax, K.lim, dt_, eps_);
#pragma unroll
            for (int i = 0; i < kJpl; ++i) s.a[i] = act[i];           // :144 (quirk Q1)
            // One-pass form: the new action is waited for HERE, unconditionally, in front of every store of the step.  On gfx9
            // vmcnt counts stores too, until the write is acknowledged: left to its first consumer, the wait sat in front of the
            // state stores (behind the outcome stores, whose acknowledgement it then waited for as well) and, that one being
            // inside the `valid` branch, again in phase 1 of the row pass (behind the state stores).  The action is the last load
            // issued and the integrator has run since, so the wait costs nothing here; the asm has side effects, so neither the
            // scheduler nor the stores move across it.
            if (ONE_PASS) asm volatile("" :: "v"(s.a[0]), "v"(s.a[1]), "v"(s.a[2]));
        }
        s.step += 1;                                                  // bullet_env.py:193

        Pose q;
        compute_pose(s, p, q);

        const Outcome oc = step_outcome<false>(P, s, p, q.dist);
        s.pot = oc.pot;
        if (valid && p == 0) store_outcome(P, oc, q.dist, (long long)t * n + e);

        // -- in-kernel auto-reset (BulletEnv.reset as the sampler would call it) -----
        // `done`/`trunc` are identical in both lanes of a pair, so pairs stay together
        if (P.auto_reset && (oc.done || oc.trunc)) {
            reset_env(P, K, s, p, P.env_off + (unsigned long long)e, nullptr, nullptr);
            compute_pose(s, p, q);
            cold = true;
        }

        // state goes out before the obs is packed: its stores drain under the LDS emit
        if (t == T - 1 && valid && !diag_nostate) store_state(state_, n, rec, p, s, cold);

        // -- observe() ----------------------------------------------------------------
        if (t > 0 || !first_tile) wave_lds_sync();   // previous flush done before the tile is rewritten
        step_obs_out<OBS_EM, ROW_PASS>(K, s, q, rowl, tile, el, p, lane, P.obs + (long long)t * n * kObsDim, tile0, n, nvalid, !diag_noemit, !diag_noflush);
    }
    first_tile = false;
    if (ONE_PASS) break;
    }   // tile loop
}

// ---------------------------------------------------------------------------------
// dynamics-mode step: ONE launch per pnr_step / pnr_rollout.  A workgroup is one wave and owns 64 envs.
//   phase A  one env per lane: command integration + the ABA sub-steps (pnr_dyn.h); a, v, r, q, qd of the
//            env stay in that lane's registers for all T steps of the launch and are handed to phase B
//            through LDS every step;
//   phase B  the lanes regroup as pairs (as in step_kernel) and finish two 32-env tiles: reward,
//            TimeLimit, auto-reset, observation through the LDS tile; the pair lanes keep target,
//            potential, step and episode counters of their envs in registers.  A reset is reported back
//            to the env's phase-A lane through a small LDS note (episode counter + the new r), which
//            re-draws the per-env parameters itself.
// The hand-off area is the head of the obs tile: both tiles' values are read into registers before the
// first observation is packed.  With T > 1 the obs stores of step t drain under the sub-steps of t + 1.
// ---------------------------------------------------------------------------------
constexpr int kDynEnvsPerWg = kWave;                       // phase A: one env per lane
constexpr int kHandRecFloats = 3 * 2 * kDynEnvsPerWg * 4;  // three float4 planes of 2 records per env
constexpr int kHandFloats = kHandRecFloats + 2 * kDof * kDynEnvsPerWg;
static_assert(kHandFloats <= kTileFloats, "the hand-off area must fit into the obs tile it aliases");

struct DynTileRegs {      // what phase A handed over for this lane's record of one env
    HalfRec raw;          // a, v, r of the lane's three joints (+ the common words on the first step)
    float q[kJpl], qd[kJpl];
};

// phase A's results for the lane's env: its two state records and the simulated q, qd
__device__ __forceinline__ void dyn_write_handoff(float* hand, int lane, const HalfRec (&k)[2], const float (&q)[kDof],
                                                  const float (&qd)[kDof])
{
    float4* hrec = reinterpret_cast<float4*>(hand);               // [3][2 * 64] records, index 2 * env + p
    float* hq = hand + kHandRecFloats;                            // [12][64]: q then qd
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        hrec[2 * lane + p] = k[p].p0;
        hrec[2 * kDynEnvsPerWg + 2 * lane + p] = k[p].p1;
        hrec[4 * kDynEnvsPerWg + 2 * lane + p] = k[p].p2;
    }
#pragma unroll
    for (int i = 0; i < kDof; ++i) {
        hq[i * kDynEnvsPerWg + lane] = q[i];
        hq[(kDof + i) * kDynEnvsPerWg + lane] = qd[i];
    }
}

__device__ __forceinline__ void dyn_read_handoff(const float* hand, int env, int p, DynTileRegs& g)
{
    const float4* hrec = reinterpret_cast<const float4*>(hand);
    const float* hq = hand + kHandRecFloats;
    const int r = 2 * env + p;
    g.raw = {hrec[r], hrec[2 * kDynEnvsPerWg + r], hrec[4 * kDynEnvsPerWg + r]};
#pragma unroll
    for (int i = 0; i < kJpl; ++i) {
        g.q[i] = hq[(kJpl * p + i) * kDynEnvsPerWg + env];
        g.qd[i] = hq[(kDof + kJpl * p + i) * kDynEnvsPerWg + env];
    }
}

// One 32-env tile of phase B at step t of the launch, for both dynamics kernels.  ROLLOUT (dyn_rollout_kernel): the env's common
// words (target | potential, step, episode) arrive with the first hand-off; between the steps of the looped launch they wait in
// `com` (LDS), so that nothing of phase B stays in registers during the sub-steps; a reset is noted in `rst` for the env's phase-A
// lane, and state / dyn words go back to memory on the last step only.  Otherwise (dyn_step_kernel: t = 0, no com, no rst) every
// step is the last.
template <bool OBS_EM, bool ROLLOUT>
__device__ __forceinline__ void dyn_finish_tile(const KParams& P, const DynParams& D, const LaneConsts& K, const DynTileRegs& in,
                                                float4* com, float* rst, float* tile, long long tile0, int t, int lane,
                                                bool tile_in_use)
{
    const int p = lane & 1, el = lane >> 1;
    const long long n = P.n;
    const long long e = tile0 + el;
    const bool valid = e < n;               // the pair shares `valid`, so DPP partners are live
    const int nvalid = (int)((n - tile0) < kEnvsPerWave ? (n - tile0) : kEnvsPerWave);
    const bool last = !ROLLOUT || t == P.T - 1;

    LaneState s;
    {
        HalfRec raw = in.raw;               // all-zero records for lanes past the end
        if (ROLLOUT && t > 0) { const float4 c = *com; raw.p2.y = c.y; raw.p2.z = c.z; raw.p2.w = c.w; }
        unpack_state(raw, p, s);            // a, v, r of this lane's joints + the env's common words
    }
    LaneState o = s;                        // what reward / obs see: the simulated q, qd
#pragma unroll
    for (int i = 0; i < kJpl; ++i) {
        o.r[i] = in.q[i];
        // teleport = reference semantics: obs shows the env's own v (pioneer_knm_env.py:202)
        o.v[i] = D.teleport ? s.v[i] : in.qd[i];
    }
    s.step += 1;                                                  // bullet_env.py:193
    o.step = s.step;

    Pose q;
    compute_pose(o, p, q);

    const Outcome oc = step_outcome<true>(P, o, p, q.dist);
    s.pot = oc.pot;
    o.pot = oc.pot;
    if (valid && p == 0) store_outcome(P, oc, q.dist, (long long)t * n + e);

    // -- in-kernel auto-reset (BulletEnv.reset as the sampler would call it) -----
    // `done`/`trunc` are identical in both lanes of a pair, so pairs stay together
    const bool redraw = P.auto_reset && (oc.done || oc.trunc);
    if (redraw) {
        reset_env(P, K, s, p, P.env_off + (unsigned long long)e, nullptr, nullptr);
        if (valid) {
            dyn_reset_lane(P, D, s, p, e, P.env_off + (unsigned long long)e, s.episode - 1);   // q = r, qd = 0, new draws
            if (ROLLOUT) {
                // note for the env's phase-A lane: the counter after the reset (>= 1) and the new joints
                const int env = el + (int)(tile0 & (kDynEnvsPerWg - 1));
                if (p == 0) rst[env] = __uint_as_float(s.episode);
#pragma unroll
                for (int i = 0; i < kJpl; ++i) rst[(1 + kJpl * p + i) * kDynEnvsPerWg + env] = s.r[i];
            }
        }
        o = s;
        compute_pose(o, p, q);
    }
    if (valid && last) {
        store_state(P.state, n, 2 * tile0 + lane, p, s, ROLLOUT || redraw);   // (a rollout: some earlier step may have reset the env)
        if (!redraw) {
#pragma unroll
            for (int i = 0; i < kJpl; ++i) {
                D.dyn[(long long)(kDynQ + kJpl * p + i) * n + e] = in.q[i];
                D.dyn[(long long)(kDynQd + kJpl * p + i) * n + e] = in.qd[i];
            }
        }
    }
    if (ROLLOUT) *com = make_float4(0.f, p ? s.pot : s.tgt[0], p ? __uint_as_float(s.step) : s.tgt[1],
                                    p ? __uint_as_float(s.episode) : s.tgt[2]);

    // -- observe() ----------------------------------------------------------------
    // (timing-only ablations of a -DPNR_DIAG_BUILD=1 variant, PNR_DIAG bits as in step_kernel: 2 no obs flush, 4 no obs emit; in the
    // product library `diag` is the literal 0)
    const int diag = PNR_DIAG_BUILD ? P.diag : 0;
    if (tile_in_use) wave_lds_sync();       // previous flush done before the tile is rewritten
    obs_tile_out<OBS_EM>(K, o, q, tile, el, p, lane, P.obs + (long long)t * n * kObsDim, tile0, n, nvalid, !(diag & 4), !(diag & 2));
}

// Leading scalar arguments as in step_kernel: preloaded into SGPRs, they repeat P.state / D.dyn / P.actions /
// P.n / P.dt / P.eps and carry max_v_to_r.
// The workgroup is TWO waves.  Wave 0 runs phase A for the 64 envs (wave 1 waits at the barrier and takes no issue slot); in
// phase B each wave finishes ONE of the two 32-env tiles in an obs tile of its own, side by side on two SIMDs, instead of wave 0
// finishing them one after the other (phase B is ~40 % of the step's fixed cost; the one-wave form: DESIGN_HISTORY.md).
constexpr int kDynStepWaves = 2;

template <bool OBS_EM, bool ACT_EM, bool RAND, int PHYS>
__global__ __launch_bounds__(kWave * kDynStepWaves) void dyn_step_kernel(const float4* __restrict__ state_, const float* __restrict__ dyn_,
                                                         const float* __restrict__ actions_, const long long n_,
                                                         const double dt_, const double eps_, const float max_v_to_r_,
                                                         const KParams P, const DynParams D)
{
    __shared__ __attribute__((aligned(16))) float lds[kDynStepWaves * kTileFloats];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
    const long long n = n_;
    const long long base = (long long)blockIdx.x * kDynEnvsPerWg;
    float* tile = lds + wv * kTileFloats;                         // this wave's obs tile
    float* hand = lds;                                            // the hand-off area: the head of tile 0

    // ---- phase A: one env per lane (wave 0)
    if (wv == 0) {
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        HalfRec k[2] = {{z4, z4, z4}, {z4, z4, z4}};               // all-zero records for lanes past the end
        float q[kDof] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, qd[kDof] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const DynLead lead = {state_, dyn_, actions_, n_, dt_, eps_, max_v_to_r_};
        if (base + lane < n) dyn_substeps_lane<ACT_EM, RAND, PHYS>(lead, D, base + lane, k, q, qd);
        // dyn_write_handoff's text, spelled out: through the call, this kernel's register allocation moved by 1-6 VGPRs in 24 of its
        // 32 instantiations (same instruction mix; listings compared with tools/device_code_diff.py), so the call waits for a compiler
        // that does not care
        float4* hrec = reinterpret_cast<float4*>(hand);
        float* hq = hand + kHandRecFloats;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            hrec[2 * lane + p] = k[p].p0;
            hrec[2 * kDynEnvsPerWg + 2 * lane + p] = k[p].p1;
            hrec[4 * kDynEnvsPerWg + 2 * lane + p] = k[p].p2;
        }
#pragma unroll
        for (int i = 0; i < kDof; ++i) {
            hq[i * kDynEnvsPerWg + lane] = q[i];
            hq[(kDof + i) * kDynEnvsPerWg + lane] = qd[i];
        }
    }
    __syncthreads();

    // ---- phase B: lane pairs, wave wv takes tile wv; both tiles' hand-off values leave LDS before tile 0 (which they alias) is reused
    const int p = lane & 1, el = lane >> 1;
    DynTileRegs g;
    dyn_read_handoff(hand, kEnvsPerWave * wv + el, p, g);
    __syncthreads();
    const LaneConsts K = lane_consts(p);
    // the 36 constant obs entries of this lane's tile slots: once per kernel
    obs_tile_const<OBS_EM>(K, tile, el, p);

    if (base + (long long)kEnvsPerWave * wv < n)
        dyn_finish_tile<OBS_EM, false>(P, D, K, g, nullptr, nullptr, tile, base + (long long)kEnvsPerWave * wv, 0, lane, false);
}

// independent waves per workgroup of dyn_rollout_kernel (own LDS slice, own 64 envs each).  A/B r03 in one run, twice: 25.60 us per
// rollout step with four (256 workgroups = one wave per SIMD by construction) against 25.65 with one: its waves already landed one per
// SIMD, so the r02 form stays.
#ifndef PNR_DYN_ROLLOUT_WAVES
#define PNR_DYN_ROLLOUT_WAVES 1
#endif
constexpr int kDynRolloutWaves = PNR_DYN_ROLLOUT_WAVES;
constexpr int kComFloats = 2 * kWave * 4;                  // common words of each lane's two envs between steps: float4 [2][64]
constexpr int kRstFloats = (1 + kDof) * kDynEnvsPerWg;     // reset notes: episode flag + new r [7][64]

// pnr_rollout in dynamics mode: P.T steps in ONE launch.  Same two phases as dyn_step_kernel, but the env's
// a, v, r, q, qd and parameters stay in its phase-A lane's registers from step to step, the pair lanes keep the
// common words (target | potential, step, episode) in LDS between steps, and a reset travels back to the phase-A
// lane as a small LDS note (episode counter + the new r) from which that lane re-draws the parameters itself.
// The obs stores of step t drain under the sub-steps of step t + 1.  The hand-off has its own 9 KB here (the
// kernel runs one wave per SIMD anyway), so a tile's values are read right before that tile is finished and
// nothing of phase B is live during the sub-steps.
template <bool OBS_EM, bool ACT_EM, bool RAND, int PHYS>
__global__ __launch_bounds__(kWave * kDynRolloutWaves) void dyn_rollout_kernel(const float4* __restrict__ state_, const float* __restrict__ dyn_,
                                                         const float* __restrict__ actions_, const long long n_,
                                                         const double dt_, const double eps_, const float max_v_to_r_,
                                                         const KParams P, const DynParams D)
{
    // kDynRolloutWaves independent waves per workgroup (each with its own LDS slice and its own 64 envs; no barrier between them):
    // at 65 536 envs the 1 024 waves are 256 workgroups = exactly one wave per SIMD, whatever the dispatcher does
    constexpr int kPerWave = kTileFloats + kComFloats + kRstFloats + kHandFloats;
    __shared__ __attribute__((aligned(16))) float lds_all[kDynRolloutWaves * kPerWave];
    float* lds = lds_all + (threadIdx.x >> 6) * kPerWave;
    float* tile = lds;
    float4* com = reinterpret_cast<float4*>(lds + kTileFloats);   // [2][64] common words between steps, index tile * 64 + lane
    float* rst = lds + kTileFloats + kComFloats;                  // [7][64] reset notes, phase B -> phase A
    float* hand = lds + kTileFloats + kComFloats + kRstFloats;    // records + q, qd planes (kHandFloats)
    const int lane = threadIdx.x & (kWave - 1);
    const int p = lane & 1, el = lane >> 1;
    const long long n = n_;
    const long long base = ((long long)blockIdx.x * kDynRolloutWaves + (threadIdx.x >> 6)) * kDynEnvsPerWg;
    const long long eA = base + lane;                             // phase A: this lane's env
    const bool liveA = eA < n;
    const DynLead lead = {state_, dyn_, actions_, n_, dt_, eps_, max_v_to_r_};

    DynLane L;
#pragma unroll
    for (int i = 0; i < kDof; ++i) { L.a[i] = L.v[i] = L.r[i] = L.q[i] = L.qd[i] = 0.f; L.fric[i] = L.damp[i] = 0.f; }
#pragma unroll
    for (int l = 0; l < kNumLinks; ++l) L.sc[l] = 1.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) { L.cw[0][k] = 0.f; L.cw[1][k] = 0.f; }
#pragma unroll
    for (int i = 0; i < kDof; ++i) L.act[i] = 0.f;
    if (liveA) dyn_lane_load<ACT_EM, RAND>(lead, base, lane, L);
    // the 36 constant obs entries of this lane's tile slots: once per kernel (nothing else writes them)
    obs_tile_const<OBS_EM>(lane_consts(p), tile, el, p);

    const int T = P.T;
    if (base >= n) return;          // a wave past the end of the batch (whole wave: no barrier follows in this kernel)
    for (int t = 0; t < T; ++t) {
        // ---- phase A: one env per lane
        if (liveA) dyn_lane_advance<ACT_EM, RAND, PHYS>(lead, D, base, lane, t + 1 < T ? actions_ + (long long)(t + 1) * n * kDof : nullptr, L);
        {
            const HalfRec k[2] = {pack_record(L.a, L.v, L.r, L.cw[0][0], L.cw[0][1], L.cw[0][2]),
                                   pack_record(L.a + 3, L.v + 3, L.r + 3, L.cw[1][0], L.cw[1][1], L.cw[1][2])};
            dyn_write_handoff(hand, lane, k, L.q, L.qd);
        }
        rst[lane] = 0.f;                                // no reset noted yet (episode counters are >= 1)
        wave_lds_sync();

        // ---- phase B: lane pairs
        {
            // everything phase B derives from the lane id (pair constants, tile and output addresses) is re-derived
            // from an opaque copy each step: hoisted out of the t loop it would sit in registers during the sub-steps
            int lane_b = lane;
            asm volatile("" : "+v"(lane_b));
            const int pb = lane_b & 1, elb = lane_b >> 1;
            const LaneConsts Kb = lane_consts(pb);
            {
                DynTileRegs g;
                dyn_read_handoff(hand, elb, pb, g);
                dyn_finish_tile<OBS_EM, true>(P, D, Kb, g, com + lane_b, rst, tile, base, t, lane_b, t > 0);
            }
            if (base + kEnvsPerWave < n) {
                DynTileRegs g;
                dyn_read_handoff(hand, kEnvsPerWave + elb, pb, g);
                dyn_finish_tile<OBS_EM, true>(P, D, Kb, g, com + kWave + lane_b, rst, tile, base + kEnvsPerWave, t, lane_b, true);
            }
            // ---- back to phase A: envs that were reset continue from the new draw
            if (t + 1 < T) {
                wave_lds_sync();
                const uint32_t ep = __float_as_uint(rst[lane]);
                if (liveA && ep != 0u) {
#pragma unroll
                    for (int j = 0; j < kDof; ++j) {
                        L.r[j] = rst[(1 + j) * kDynEnvsPerWg + lane];
                        L.a[j] = 0.f; L.v[j] = 0.f; L.q[j] = L.r[j]; L.qd[j] = 0.f;
                    }
                    if (RAND) dyn_draw_params(P, D, P.env_off + (unsigned long long)eA, ep - 1u, L.sc, L.fric, L.damp);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------
// reset / observe kernel.  MODE 0: reset (mask / overrides), 1: observe only.
// OBS: 0 none, 1 feature-major direct (masked reset), 2 env-major via LDS tile
//      (all rows written), 3 env-major direct rows (masked reset), 4 feature-major
//      via LDS tile (all columns written).
// ---------------------------------------------------------------------------------
template <int MODE, int OBS, bool DYN>
__global__ __launch_bounds__(kWave) void reset_kernel(const KParams P, const DynParams D)
{
    __shared__ __attribute__((aligned(16))) float tile[(OBS == 2 || OBS == 4) ? kTileFloats : 4];
    const int lane = threadIdx.x;
    const int p = lane & 1, el = lane >> 1;
    const long long n = P.n;
    const long long tile0 = (long long)blockIdx.x * kEnvsPerWave;
    const long long e = tile0 + el;
    const long long rec = 2 * tile0 + lane;
    const bool valid = e < n;
    const int nvalid = (int)((n - tile0) < kEnvsPerWave ? (n - tile0) : kEnvsPerWave);

    const LaneConsts K = lane_consts(p);
    LaneState s;
    if (valid) load_state(P.state, n, rec, p, s);
    else zero_state(s);
    bool active = valid;
    if (MODE == 0) {
        if (valid && P.mask) active = P.mask[e] != 0;
        if (active) {   // both lanes of a pair take the same branch
            reset_env(P, K, s, p, P.env_off + (unsigned long long)e,
                      P.joint_pos ? P.joint_pos + e * kDof : nullptr,
                      P.target_pos ? P.target_pos + e * 3 : nullptr);
            store_state(P.state, n, rec, p, s, true);
            if (DYN) dyn_reset_lane(P, D, s, p, e, P.env_off + (unsigned long long)e, s.episode - 1);
        }
    }
    if (DYN && !(MODE == 0 && active)) {
        // observe the simulated joints (a freshly reset env has q = r, qd = 0 already in s)
#pragma unroll
        for (int i = 0; i < kJpl; ++i) {
            const float qi = valid ? D.dyn[(long long)(kJpl * p + i) * n + e] : 0.f;
            const float qdi = valid ? D.dyn[(long long)(kDynQd + kJpl * p + i) * n + e] : 0.f;
            s.r[i] = qi;
            if (!D.teleport) s.v[i] = qdi;
        }
    }
    if (OBS != 0) {
        Pose q;
        compute_pose(s, p, q);   // every lane takes part: the DPP exchange needs live partners
        if (OBS == 1) {
            SinkDirect sink{P.obs + e, n, kJpl * p, p, active};
            emit_obs(K, s, q, p, sink);
        } else if (OBS == 2 || OBS == 4) {
            obs_tile_out<OBS == 2, true>(K, s, q, tile, el, p, lane, P.obs, tile0, n, nvalid);
        } else {
            SinkDirect sink{P.obs + e * kObsDim, 1, kJpl * p, p, active};
            emit_obs(K, s, q, p, sink);
        }
    }
}

// ---------------------------------------------------------------------------------
// World.step (bullet_scene.py:273-275), the four pnr_world_step* calls: frame_skip sub-steps of the simulator and NOTHING else — no
// command integration, reward, TimeLimit, reset or observation.  One env per lane (the phase-A shape of dyn_step_kernel); the
// joints' motors are the per-joint table W (Joint.control_position / control_velocity, bullet_scene.py:123-155).  FORM: the
// call's options (kWorld*, pnr_dyn.h); the host launches ten of their combinations (launch_world_step, pnr_api.hip) and no other
// is instantiated.  Every load is issued before the sub-step loop, and every branch on an option's input is wave-uniform.
//   kWorldCMotor   W holds at least one of Bullet's constraint motors (motor_constraints, pnr_dyn.h); launched only then.
//   kWorldTorque   tau_ext [n][6], the lane's six joint torques.  PD motors only: the host refuses them next to a constraint
//                  motor.  Next to wrenches or targets the pointer may be null: the branch loads zeros instead, so the call
//                  without joint torques costs no second set of instantiations.
//   kWorldWrench   up to four link wrench records per env (wrenches [n][T.n][9], env-major: force | position | torque) under the
//                  by-value table T.  The records stay in registers over the loop (36 VGPRs; the kernel has no scratch).
//   kWorldTargets  the env's OWN motor targets (targets [n][12], env-major: position[6] | velocity[6], 48 B per env, 16-byte
//                  aligned) for the joints of `mask`.  The kernel holds the env's command state r, v in registers for the from_cmd
//                  joints anyway; the masked joints' r, v are the lane's targets instead (a wave-uniform select per joint, before
//                  the loop: the twelve loaded values die there and the loop carries what the plain form's carries), and the host
//                  hands over a copy of the table with from_cmd set for the masked joints.  The row is loaded whole and the
//                  unmasked joints' entries are dropped by the select, never used in arithmetic.
// Behind `state, dyn, n` a form takes the arguments that it reads and no other, in the order wrenches | targets | tau_ext | mask |
// D | W | T: the argument list, the kernarg offsets and the preloaded leading arguments of a kernel written for that form alone.
// They matter: with D and W eight bytes further on (behind empty one-byte arguments) the plain step measured 0.2 us more per
// launch at 65 536 envs, and without the targets forms' row, torque pointer and mask preloaded the PD form at PHYS 3 falls to one
// wave per SIMD.  So the five parameters behind n are slots: slot i holds the form's i-th argument (WorldSlot; an empty struct behind
// the last), and the body finds an argument by its role (world_arg).  The targets form with constraint motors keeps the torque
// pointer (never read) between its row and its mask.
//   kWorldBody     the env's moving sphere (pnr_set_body_params; pnr_dyn.h): its buffer [8][n] and params are the argument WorldBody,
//                  behind W.  Built into two forms, both with kWorldTorque (tau_ext may be null) and PHYS 1 or 3: the plain one and
//                  the targets one, whose joint mask rides in WorldBody (five slots: targets | tau_ext | D | W | body).  The eight
//                  words are loaded with the other first loads; words 0-5 are stored at the end, by lanes with mass > 0 only.
//   kWorldGrip     the grip on the sphere (pnr_set_body_grip_params; pnr_dyn.h grip_force), with kWorldBody only: two more forms x PHYS 1
//                  and 3.  No slot of its own: the grip buffer [4][n] and the wave-uniform operands ride in the sphere's argument,
//                  which these forms take as WorldGrip (role kArgGripBody in kArgBody's place; the forms without the grip keep the
//                  argument list they had).  The lane's max_force is loaded with the sphere's words; words 1-3 are stored inside
//                  the last sub-step, by held lanes only.
// ---------------------------------------------------------------------------------
struct NoArg {};
enum WorldRole : int { kArgWrenches, kArgTargets, kArgTau, kArgMask, kArgD, kArgW, kArgT, kArgBody, kArgGripBody, kWorldRoles };
template <int ROLE> using WorldRoleType = std::tuple_element_t<ROLE, std::tuple<const float*, const float*, const float*, unsigned, DynParams,
                                                                                  JointMotorTable, LinkWrenchTable, WorldBody, WorldGrip>>;
constexpr int kWorldSlots = 5;
// (named functions of plain ints: an expression on the flag enum written into a parameter type is mangled into the kernel's name,
// and for an unnamed enum the host and the device pass number it differently: the launch then finds no such symbol)
constexpr bool world_has(int form, int role)
{
    const bool tg = (form & kWorldTargets) != 0, wr = (form & kWorldWrench) != 0, bd = (form & kWorldBody) != 0;
    if (role == kArgBody) return bd && (form & kWorldGrip) == 0;
    if (role == kArgGripBody) return bd && (form & kWorldGrip) != 0;
    if (role == kArgMask) return tg && !bd;
    return role == kArgD || role == kArgW || (role == kArgTau ? tg || (form & kWorldTorque) != 0 : (role == kArgWrenches || role == kArgT) ? wr : tg);
}
constexpr int world_slot(int form, int role)        // the role's slot in this form
{
    int slot = 0;
    for (int r = 0; r < role; ++r) slot += world_has(form, r);
    return slot;
}
constexpr int world_role_at(int form, int slot)     // .. and the slot's role; kWorldRoles: none
{
    for (int r = 0; r < kWorldRoles; ++r)
        if (world_has(form, r) && world_slot(form, r) == slot) return r;
    return kWorldRoles;
}
template <int FORM, int SLOT, int ROLE = world_role_at(FORM, SLOT)>
using WorldSlot = std::conditional_t<ROLE == kWorldRoles, NoArg, WorldRoleType<ROLE == kWorldRoles ? 0 : ROLE>>;
template <int I, class A, class... R>
__host__ __device__ __forceinline__ const auto& world_nth(const A& a, const R&... r)
{
    if constexpr (I == 0) return a; else return world_nth<I - 1>(r...);
}
// the argument of `role` among the form's slots s...
template <int FORM, int ROLE, class... S>
__host__ __device__ __forceinline__ const WorldRoleType<ROLE>& world_arg(const S&... s) { return world_nth<world_slot(FORM, ROLE)>(s...); }

template <bool RAND, int PHYS, int FORM>
__global__ __launch_bounds__(kWave) void dyn_world_kernel(const float4* __restrict__ state, float* __restrict__ dyn, const long long n,
                                                          const WorldSlot<FORM, 0> s0, const WorldSlot<FORM, 1> s1, const WorldSlot<FORM, 2> s2,
                                                          const WorldSlot<FORM, 3> s3, const WorldSlot<FORM, 4> s4)
{
    const DynParams& D = world_arg<FORM, kArgD>(s0, s1, s2, s3, s4);
    const JointMotorTable& W = world_arg<FORM, kArgW>(s0, s1, s2, s3, s4);
    constexpr bool TORQUE = (FORM & kWorldTorque) != 0, WRENCH = (FORM & kWorldWrench) != 0, TARGETS = (FORM & kWorldTargets) != 0,
                   BODY = (FORM & kWorldBody) != 0, GRIP = (FORM & kWorldGrip) != 0;
    const long long e = (long long)blockIdx.x * kWave + threadIdx.x;
    if (e >= n) return;
    float a[kDof], v[kDof], r[kDof], q[kDof], qd[kDof], sc[kNumLinks], fric[kDof], damp[kDof], act[kDof], tx[kDof];
    HalfRec k[2];                           // the env's command state r, v: what a joint without a command of its own tracks
    load_env_halves(state, n, e, 0, k);
    [[maybe_unused]] float4 g0, g1, g2;     // the env's targets row
    if constexpr (TARGETS) {
        const float4* g4 = reinterpret_cast<const float4*>(world_arg<FORM, kArgTargets>(s0, s1, s2, s3, s4)) + 3 * e;
        g0 = g4[0]; g1 = g4[1]; g2 = g4[2];
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) unpack_record(k[p], a + 3 * p, v + 3 * p, r + 3 * p);
#pragma unroll
    for (int i = 0; i < kDof; ++i) {
        q[i] = dyn[(long long)i * n + e]; qd[i] = dyn[(long long)(kDynQd + i) * n + e];
        fric[i] = dyn[(long long)(kDynFric + i) * n + e]; damp[i] = dyn[(long long)(kDynDamp + i) * n + e];
        act[i] = 0.f; tx[i] = 0.f;
    }
#pragma unroll
    for (int l = 0; l < kNumLinks; ++l) sc[l] = RAND ? dyn[(long long)(kDynScale + l) * n + e] : 1.0f;
    constexpr int kBodyRole = GRIP ? kArgGripBody : kArgBody;      // the sphere's argument: WorldGrip with the grip, else WorldBody
    [[maybe_unused]] std::conditional_t<GRIP, GripLane, SphereLane> S;
    if constexpr (BODY) {
        const float* bw = world_arg<FORM, kBodyRole>(s0, s1, s2, s3, s4).words + e;
        S.x = {bw[0], bw[n], bw[2 * n]}; S.v = {bw[3 * n], bw[4 * n], bw[5 * n]};
        S.m = bw[6 * n]; S.r = bw[7 * n];
        if constexpr (GRIP) S.g = world_arg<FORM, kBodyRole>(s0, s1, s2, s3, s4).grip[e];
    }
    WrenchLane XL;
    if constexpr (WRENCH) {
        static_for<kMaxWrench>([&](auto j_) {
#pragma unroll
            for (int i = 0; i < 9; ++i) XL.w[decltype(j_)::value][i] = 0.f;
        });
        load_wrench_records(world_arg<FORM, kArgWrenches>(s0, s1, s2, s3, s4), world_arg<FORM, kArgT>(s0, s1, s2, s3, s4), e, XL);
    }
    if constexpr (TORQUE) {
        const float* tau_ext = world_arg<FORM, kArgTau>(s0, s1, s2, s3, s4);
        if (!(WRENCH || TARGETS || BODY) || tau_ext) load_joint_torques(tau_ext, e, tx);
    }
    if constexpr (TARGETS) {
        const float tp[kDof] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y}, tv[kDof] = {g1.z, g1.w, g2.x, g2.y, g2.z, g2.w};
        unsigned mask;
        if constexpr (BODY) mask = world_arg<FORM, kBodyRole>(s0, s1, s2, s3, s4).joint_mask;
        else mask = world_arg<FORM, kArgMask>(s0, s1, s2, s3, s4);
#pragma unroll
        for (int i = 0; i < kDof; ++i) {
            const bool own = (mask >> i) & 1u;
            r[i] = own ? tp[i] : r[i];
            v[i] = own ? tv[i] : v[i];
        }
    }
    const DynLead lead = {state, dyn, nullptr, n, 0.0, 0.0, 0.f};
    const LinkWrenchTable* X = nullptr;
    if constexpr (WRENCH) X = &world_arg<FORM, kArgT>(s0, s1, s2, s3, s4);
    const WorldOperands world = {W, X, XL};
    if constexpr (BODY) dyn_core<PHYS, kWorld | FORM>(lead, D, a, v, r, q, qd, sc, fric, damp, act, &world, tx, &world_arg<FORM, kBodyRole>(s0, s1, s2, s3, s4), &S, e);
    else dyn_core<PHYS, kWorld | FORM>(lead, D, a, v, r, q, qd, sc, fric, damp, act, &world, tx);
#pragma unroll
    for (int i = 0; i < kDof; ++i) { dyn[(long long)i * n + e] = q[i]; dyn[(long long)(kDynQd + i) * n + e] = qd[i]; }
    if constexpr (BODY) {
        if (S.m > 0.f) {               // an env without a sphere keeps its eight words as they are
            float* bw = world_arg<FORM, kBodyRole>(s0, s1, s2, s3, s4).words + e;
            bw[0] = S.x.x; bw[n] = S.x.y; bw[2 * n] = S.x.z; bw[3 * n] = S.v.x; bw[4 * n] = S.v.y; bw[5 * n] = S.v.z;
        }
    }
}

// pnr_set_body_grip: the caller's max_force into word 0 of the handle's grip buffer and zeros into the reported force (words 1-3),
// for every env or the masked ones (the device-side "grip the envs that just came within reach")
__global__ void grip_set_kernel(float* __restrict__ dst, const float* __restrict__ max_force, const uint8_t* __restrict__ mask, long long n)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n || (mask && !mask[e])) return;
    dst[e] = max_force[e];
#pragma unroll
    for (int w = 1; w < PNR_BODY_GRIP_WORDS; ++w) dst[(long long)w * n + e] = 0.f;
}

// pnr_set_body_state: the caller's eight words per env into the handle's sphere buffer, for every env or the masked ones (the
// device-side "reset the sphere of the envs that just finished")
__global__ void body_set_kernel(float* __restrict__ dst, const float* __restrict__ src, const uint8_t* __restrict__ mask, long long n)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n || (mask && !mask[e])) return;
#pragma unroll
    for (int w = 0; w < PNR_BODY_STATE_WORDS; ++w) dst[(long long)w * n + e] = src[(long long)w * n + e];
}

// The same call on a kinematic-mode handle: there is no simulated state, the caller holds the joints as Bullet would after
// resetJointState(position, velocity) — js [n][12] = q[6] | qd[6] — and with no gravity, no motor and no collision shapes
// (the reference's URDF and defaults) frame_skip x stepSimulation carries each joint on at its velocity:
// q += qd * step_time, stopped at its limit with the velocity zeroed there.
__global__ void kin_world_kernel(float* __restrict__ js, long long n, float step_time)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * kDof) return;
    const long long e = i / kDof; const int j = (int)(i % kDof);
    constexpr float lim[kDof] = {limit_hi(0), limit_hi(1), limit_hi(2), limit_hi(3), limit_hi(4), limit_hi(5)};
    const float hi = lim[j];
    float q = js[e * 12 + j], qd = js[e * 12 + 6 + j];
    q = __builtin_fmaf(qd, step_time, q);
    if (q >= hi) { q = hi; qd = 0.f; }
    if (q <= -hi) { q = -hi; qd = 0.f; }
    js[e * 12 + j] = q; js[e * 12 + 6 + j] = qd;
}

// canonical planar words [24][n] (include/pioneer_amd.h) <-> the engine's records (pnr_device.h): one thread per half record
__global__ void state_to_words_kernel(const float4* __restrict__ st, uint32_t* __restrict__ w, long long n)
{
    const long long rec = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (rec >= 2 * n) return;
    const long long e = rec >> 1; const int p = (int)(rec & 1);
    const RawState k = load_state_raw(st, n, rec);
    float a[kJpl], v[kJpl], r[kJpl];
    unpack_record(k, a, v, r);
#pragma unroll
    for (int i = 0; i < kJpl; ++i) {
        w[(long long)(0 + kJpl * p + i) * n + e] = __float_as_uint(a[i]);
        w[(long long)(6 + kJpl * p + i) * n + e] = __float_as_uint(v[i]);
        w[(long long)(12 + kJpl * p + i) * n + e] = __float_as_uint(r[i]);
    }
    if (p == 0) {
        w[18LL * n + e] = __float_as_uint(k.c.x); w[19LL * n + e] = __float_as_uint(k.c.y); w[20LL * n + e] = __float_as_uint(k.c.z);
        w[21LL * n + e] = __float_as_uint(k.h.y);                   // potential
        w[23LL * n + e] = __float_as_uint(k.c.w);                   // episode
    } else {
        w[22LL * n + e] = __float_as_uint(k.h.y);                   // step_index
    }
}

__global__ void words_to_state_kernel(float4* __restrict__ st, const uint32_t* __restrict__ w, long long n)
{
    const long long rec = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (rec >= 2 * n) return;
    const long long e = rec >> 1; const int p = (int)(rec & 1);
    const auto word = [&](int k) { return __uint_as_float(w[(long long)k * n + e]); };
    RawState k;
    k.p0 = make_float4(word(0 + kJpl * p), word(1 + kJpl * p), word(2 + kJpl * p), word(6 + kJpl * p));
    k.p1 = make_float4(word(7 + kJpl * p), word(8 + kJpl * p), word(12 + kJpl * p), word(13 + kJpl * p));
    k.h = make_float2(word(14 + kJpl * p), word(p ? 22 : 21));
    k.c = make_float4(word(18), word(19), word(20), word(23));
    store_state_raw(st, n, rec, p, k, true);
}

__global__ void diag_sincos_kernel(const float* __restrict__ x, float* __restrict__ sn, float* __restrict__ cs,
                                   long long n, int bounded)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s, c;
    if (bounded) sincos_bounded(x[i], s, c); else sincos_any(x[i], s, c);
    sn[i] = s; cs[i] = c;
}

}  // namespace pnr
