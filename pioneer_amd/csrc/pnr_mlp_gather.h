// pnr_mlp_gather.h — an SGD epoch's shuffle applied once: record_pack_kernel (the rollout record as one row per sample) and
// mlp_gather_kernel (the nets' filtered inputs and the record in minibatch order; pnr_ppo_pack_record, pnr_mlp_gather).
#pragma once

#include "pnr_mlp.h"
#pragma clang fp contract(fast)      // as in pnr_mlp.h: the TU is compiled -ffp-contract=off for the env integrator
namespace pnr {

// ---------------------------------------------------------------------------------------------------------------
// An SGD epoch's shuffle applied ONCE: row i of the outputs is row idx[i] of the rollout — the observation filtered and
// rounded as mlp_forward_kernel's stage 0 does it (mlp_filter) ([B][144] bf16, columns 137.. zero) and the rollout record (22 floats).  The
// epoch's 16 minibatch updates then read contiguous rows (mlp_forward_kernel's xs_in path: a plain 18 KB copy per tile
// instead of 64 scattered 548-byte rows and the filter arithmetic, no idx gather in the loss, and no `xs` store: the
// weight-gradient kernel reads these rows directly).  One block = 64 samples, four threads per row, like stage 0.
// ---------------------------------------------------------------------------------------------------------------
// The rollout record of one sample as one 96-byte row: actions 0..5 | mean 6..11 | log_std 12..17 | logp, adv, vtarg, value |
// 2 pad.  Packed once per iteration (contiguous reads and writes), with the advantages standardised on the way
// ((adv - mu) / den, PPO's batch standardisation, the same float32 operations as the element-wise form): the epoch
// gathers then touch one or two cache lines per sample for the record instead of seven.
constexpr int kRecAos = 24;
struct RecordPackParams {
    const float* actions; const float* logp; const float* mean; const float* log_std;
    const float* adv; const float* vtarg; const float* values;
    const float* adv_mu; const float* adv_den;      // device scalars, or null: advantages as they are
    float* aos;                                     // [rows][24]
    long long rows;
};

__global__ __launch_bounds__(256) void record_pack_kernel(const RecordPackParams P)
{
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= P.rows) return;
    float o[kRecAos];
#pragma unroll
    for (int j = 0; j < 6; ++j) { o[j] = P.actions[r * 6 + j]; o[6 + j] = P.mean[r * 6 + j]; o[12 + j] = P.log_std[r * 6 + j]; }
    o[18] = P.logp[r];
    const float a = P.adv[r];
    o[19] = P.adv_mu ? __fdiv_rn(__fsub_rn(a, *P.adv_mu), *P.adv_den) : a;
    o[20] = P.vtarg[r]; o[21] = P.values[r]; o[22] = 0.f; o[23] = 0.f;
    f32x4* dst = reinterpret_cast<f32x4*>(P.aos + r * kRecAos);
#pragma unroll
    for (int q = 0; q < 6; ++q) dst[q] = (f32x4){o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]};
}

struct MlpGatherParams {
    const float* obs; const long long* idx;
    const float* f_loc; const float* f_inv; const float* f_lo; const float* f_hi;     // all four or none
    const float* actions; const float* logp; const float* mean; const float* log_std;
    const float* adv; const float* vtarg; const float* values;
    const float* rec_aos;      // [rows][24] the same record as ONE 96-byte row per sample (record_pack_kernel), or null: the seven arrays
    const __bf16* xs_src;      // [rows][144] the nets' inputs as the sampler saw them (pnr_mlp_act's xs_out), or null: made from obs
    __bf16* xs_out;            // [planes][B][144]
    int planes;                // 1, or 2 / 3 split planes of the filtered float32 input (then xs_src must be null)
    float* actions_out; float* logp_out; float* mean_out; float* log_std_out; float* adv_out; float* vtarg_out; float* values_out;
    long long B;
};

__global__ __launch_bounds__(kMlpThreads) void mlp_gather_kernel(const MlpGatherParams P)
{
    __shared__ __attribute__((aligned(16))) float fv[4 * kMlpInPad];
    const int tid = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * 64;
    if (P.f_loc) {
        for (int i = tid; i < 4 * kMlpInPad; i += kMlpThreads) {
            const int which = i / kMlpInPad, k = i % kMlpInPad;
            const float* src = which == 0 ? P.f_loc : (which == 1 ? P.f_inv : (which == 2 ? P.f_lo : P.f_hi));
            fv[i] = k < kMlpIn ? src[k] : 0.f;
        }
    }
    __syncthreads();
    constexpr int TPR = kMlpThreads / 64, CPT = kMlpInPad / TPR, NV = CPT / 4;
    const int row = tid / TPR, part = tid % TPR;
    const long long b = row0 + row;
    if (b >= P.B) return;
    const long long r = P.idx ? P.idx[b] : b;
    if (P.xs_src) {     // a 288-byte row copied as 18 16-byte pieces (thread `part` takes pieces part, part + 4, ...): 3 lines, not 5
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int cc = part + TPR * j;
            if (cc < kMlpInPad / 8)
                *reinterpret_cast<uint4*>(P.xs_out + b * kMlpInPad + cc * 8) = *reinterpret_cast<const uint4*>(P.xs_src + r * kMlpInPad + cc * 8);
        }
    }
    // a row's four threads take its 16-byte pieces INTERLEAVED (thread `part`: pieces part, part + 4, ...), so that one load instruction
    // reads 64 contiguous bytes of each of the wave's 16 random rows; with a contiguous 36-column share per thread (r02 - r04) every
    // instruction touched 64 different cache lines for 16 bytes each, four times the L2 sectors per row
    const float* src = P.obs + r * kMlpIn;
    typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
    f32x4 v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int col = 4 * TPR * j + 4 * part;
        v[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (P.xs_src) continue;
        if (col + 3 < kMlpIn) v[j] = *reinterpret_cast<const f32x4u*>(src + col);
        else if (col < kMlpIn) v[j][0] = src[col];
    }
    float recv[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};             // this thread's share of the record: part 0 actions, 1 mean, 2 log_std
    float sc[4] = {0.f, 0.f, 0.f, 0.f};                         // part 3: logp, adv, vtarg, values
    if (P.rec_aos) {                                            // the row's four threads read its 96 contiguous bytes
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        const f32x2* a2 = reinterpret_cast<const f32x2*>(P.rec_aos + r * kRecAos + 6 * part);
        const f32x2 x0 = a2[0], x1 = a2[1], x2 = a2[2];
        if (part < 3) { recv[0] = x0[0]; recv[1] = x0[1]; recv[2] = x1[0]; recv[3] = x1[1]; recv[4] = x2[0]; recv[5] = x2[1]; }
        else { sc[0] = x0[0]; sc[1] = x0[1]; sc[2] = x1[0]; sc[3] = x1[1]; }
    } else if (part < 3) {
        const float* a = (part == 0 ? P.actions : (part == 1 ? P.mean : P.log_std)) + r * 6;
#pragma unroll
        for (int j = 0; j < 6; ++j) recv[j] = a[j];
    } else { sc[0] = P.logp[r]; sc[1] = P.adv[r]; sc[2] = P.vtarg[r]; sc[3] = P.values[r]; }
    if (!P.xs_src) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int col = 4 * TPR * j + 4 * part;
        f32x4 x = v[j];
        if (P.f_loc) {
            f32x4 f[4];                                      // loc, inv, lo, hi of the four columns
#pragma unroll
            for (int i = 0; i < 4; ++i) f[i] = *reinterpret_cast<const f32x4*>(fv + i * kMlpInPad + col);
#pragma unroll
            for (int k = 0; k < 4; ++k) x[k] = mlp_filter(x[k], [&](int i) { return f[i][k]; });
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) if (col + k >= kMlpIn) x[k] = 0.f;
        if (P.planes == 2) {                             // two fp16 planes of the input x 2^4 (Fmt<2>)
            const float xv[4] = {x[0], x[1], x[2], x[3]};
            bf16x4_t hp[2];
            split_quad<2>(xv, hp, Fmt<2>::kSX);
            *reinterpret_cast<bf16x4*>(P.xs_out + b * kMlpInPad + col) = hp[0];
            *reinterpret_cast<bf16x4*>(P.xs_out + ((size_t)P.B + b) * kMlpInPad + col) = hp[1];
        } else {
        bf16x4 pk;
#pragma unroll
        for (int k = 0; k < 4; ++k) pk[k] = (__bf16)x[k];
        *reinterpret_cast<bf16x4*>(P.xs_out + b * kMlpInPad + col) = pk;
        for (int pl = 1; pl < P.planes; ++pl) {          // the residual planes of the split float32 input
#pragma unroll
            for (int k = 0; k < 4; ++k) { x[k] = x[k] - (float)pk[k]; pk[k] = (__bf16)x[k]; }
            *reinterpret_cast<bf16x4*>(P.xs_out + ((size_t)pl * P.B + b) * kMlpInPad + col) = pk;
        }
        }
    }
    }
    if (part < 3) {
        float* o = (part == 0 ? P.actions_out : (part == 1 ? P.mean_out : P.log_std_out)) + b * 6;
#pragma unroll
        for (int j = 0; j < 6; ++j) o[j] = recv[j];
    } else { P.logp_out[b] = sc[0]; P.adv_out[b] = sc[1]; P.vtarg_out[b] = sc[2]; P.values_out[b] = sc[3]; }
}

}  // namespace pnr
#pragma clang fp contract(off)
