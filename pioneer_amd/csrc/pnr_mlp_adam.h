// pnr_mlp_adam.h — mlp_adam_kernel: Adam on the float32 master parameters, with the slab reduction in front of it, the weight
// packing behind it and the update's loss means beside it (pnr_mlp_train_step, pnr_mlp_adam).
#pragma once

#include "pnr_mlp.h"
#include "pnr_ppo.h"
#pragma clang fp contract(fast)      // as in pnr_mlp.h: the TU is compiled -ffp-contract=off for the env integrator
namespace pnr {

// ---------------------------------------------------------------------------------------------------------------
// Adam on the float32 master parameters, fused with the slab reduction in front of it and with the bf16 weight
// packing behind it: one launch turns per-slice partial gradients into the next forward's operands.  torch.optim.Adam
// semantics (no weight decay, no amsgrad): m += (g - m)(1 - b1); v = b2 v + (1 - b2) g^2;
// p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps), t = *step (incremented once per update by the loss
// kernel's finishing launch).  State m, v live in the padded slab layout [2][kGradElems].
// ---------------------------------------------------------------------------------------------------------------
struct MlpAdamParams {
    const float* grad;         // slices x [2][kGradElems] partial gradients (slabs), or one flat all-reduced gradient
    int slices;                // 1 for a flat gradient
    float grad_scale;          // e.g. 1 / world size after a summing all-reduce
    float* w1[kMlpNets]; float* b1[kMlpNets];      // master parameters (the caller's tensors)
    float* w2[kMlpNets]; float* b2[kMlpNets];
    float* w3[kMlpNets]; float* b3[kMlpNets];
    int n3[kMlpNets];
    float* m; float* v;        // [2][kGradElems]
    const float* step;         // device scalar: number of updates including this one
    float lr, beta1, beta2, eps;
    __bf16* wpack;             // [2][kPackElems]: refreshed in place
    float* bias;               // [2][kBiasElems]
    // the loss means of the update ride in this launch (one extra block; null partials: none)
    const float* partials;     // [loss_rows][8] of the fused forward + loss + backward kernel
    long long loss_rows, batch;
    float* means;              // [8]
    const float* kl_coeff; const float* ent_coeff; float vf_coeff;
    int first_net;             // blockIdx.y + first_net = net
    int planes;                // bf16 planes of the packed weights that are refreshed (1: bf16 operands; 2, 3: split float32)
};

constexpr int kAdamVec = 4;          // consecutive gradient-layout elements per thread (every region of the layout starts on a multiple of 4)
constexpr int kAdamBlocks = (kGradElems / kAdamVec + 255) / 256;     // + 1: the loss-means block
static_assert(kGradElems % kAdamVec == 0 && kGW2 % 4 == 0 && kGW3 % 4 == 0 && kGB1 % 4 == 0 && kGB2 % 4 == 0 && kGB3 % 4 == 0 && kMlpInPad % 4 == 0, "");

// r04: FOUR elements per thread — the bias corrections' two powf once per four elements, the 32 slabs as 32 16-byte loads in one batch
// (slice order in the sum: same bits as before), one 8-byte store per fragment-native bf16 group; 840 waves instead of 6 712.  Measured
// (tools/adam_floor.py, profiles/r04_g_adam_four_per_thread_ab.txt): 10.6 -> 10.1 us with the learner's 32 slabs, 8.0 -> 7.7 us back to
// back with ONE flat gradient — neither the instruction stream (~700 per wave before) nor the slabs' four dependent round trips were
// the bound: ~6 us of the launch are its floor (launch, one load round trip from HBM, the stores' drain) and ~4 us the 27 MB of slabs.
__global__ __launch_bounds__(256) void mlp_adam_kernel(const MlpAdamParams P)
{
    const int net = blockIdx.y + P.first_net;
    if (blockIdx.x == 0) {
        // the extra block (the FIRST one, so that it starts with the launch and not as its tail): the five loss means from the fused
        // kernel's per-workgroup rows (ppo_loss_finish_split_kernel's job), in the shadow of the other blocks instead of a launch of its own
        __shared__ float red[4][kPpoSums];
        if (blockIdx.y != 0 || !P.partials) return;
        ppo_loss_means_block(P.partials, P.loss_rows, P.batch, P.means, P.kl_coeff, P.ent_coeff, P.vf_coeff, red);
        return;
    }
    const int e = ((blockIdx.x - 1) * 256 + threadIdx.x) * kAdamVec;
    if (e >= kGradElems) return;
    const size_t si = (size_t)net * kGradElems + e;
    // requested first, so that they arrive under the slabs' round trip
    const float t = *P.step;
    const f32x4 m4 = *reinterpret_cast<const f32x4*>(P.m + si), v4 = *reinterpret_cast<const f32x4*>(P.v + si);

    // where the four elements live: master parameter (dst, `valid` of them exist), fragment-native bf16 copies (wp0: four consecutive
    // elements of one fragment row; wp1[j]: the transposed copy, one row each), bias copy
    float* dst = nullptr;
    int valid = kAdamVec, wp0 = -1, bp = -1;
    int wp1[kAdamVec] = {-1, -1, -1, -1};
    if (e < kGW2) {
        const int o = e / kMlpInPad, k = e % kMlpInPad;
        wp0 = kOffW1 + frag32_off(o, k, kMlpInPad / 16);
        dst = P.w1[net] + o * kMlpIn + k; valid = kMlpIn - k;
    } else if (e < kGW3) {
        const int r = e - kGW2, o = r / kMlpHid, i = r % kMlpHid;
        dst = P.w2[net] + r; wp0 = kOffW2 + frag32_off(o, i, kMlpHid / 16);
#pragma unroll
        for (int j = 0; j < kAdamVec; ++j) wp1[j] = kOffW2T + frag32_off(i + j, o, kMlpHid / 16);
    } else if (e < kGB1) {
        const int r = e - kGW3, row = r / kMlpHid, f = r % kMlpHid;
        wp0 = kOffW3 + frag16_off(row, f);
#pragma unroll
        for (int j = 0; j < kAdamVec; ++j) wp1[j] = kOffW3T + frag32_off(f + j, row, 1);
        dst = P.w3[net] + r; valid = row < P.n3[net] ? kAdamVec : 0;
    } else if (e < kGB2) { dst = P.b1[net] + (e - kGB1); bp = e - kGB1; }
    else if (e < kGB3) { dst = P.b2[net] + (e - kGB2); bp = kMlpHid + (e - kGB2); }
    else { bp = 2 * kMlpHid + (e - kGB3); dst = P.b3[net] + (e - kGB3); valid = P.n3[net] - (e - kGB3); }
    float p0[kAdamVec];
#pragma unroll
    for (int j = 0; j < kAdamVec; ++j) p0[j] = j < valid ? dst[j] : 0.f;

    // the slices' partial gradients, summed in slice order per element (the order mlp_reduce_flat_kernel uses: same bits)
    f32x4 g4 = {0.f, 0.f, 0.f, 0.f};
    if (valid > 0) {
        constexpr size_t kStride = (size_t)kMlpNets * kGradElems;
        const float* gp = P.grad + si;
        int k = 0;
        if (P.slices == 32) {                               // the learner's slab count: one batch of loads, one round trip
            f32x4 x[32];
#pragma unroll
            for (int j = 0; j < 32; ++j) x[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(gp + (size_t)j * kStride));
#pragma unroll
            for (int j = 0; j < 32; ++j) g4 += x[j];
            k = 32;
        }
        for (; k + 8 <= P.slices; k += 8) {
            f32x4 x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = *reinterpret_cast<const f32x4*>(gp + (size_t)(k + j) * kStride);
#pragma unroll
            for (int j = 0; j < 8; ++j) g4 += x[j];
        }
        for (; k < P.slices; ++k) g4 += *reinterpret_cast<const f32x4*>(gp + (size_t)k * kStride);
    }
    const float bc1 = 1.0f - powf(P.beta1, t), bc2 = 1.0f - powf(P.beta2, t);
    const float rbc2 = sqrtf(bc2), lr1 = P.lr / bc1;
    f32x4 mo = m4, vo = v4;
    float pv[kAdamVec];
#pragma unroll
    for (int j = 0; j < kAdamVec; ++j) {
        pv[j] = 0.f;
        if (j < valid) {
            const float g = g4[j] * P.grad_scale;
            const float m = m4[j] + (g - m4[j]) * (1.0f - P.beta1);
            const float v = P.beta2 * v4[j] + (1.0f - P.beta2) * g * g;
            const float denom = sqrtf(v) / rbc2 + P.eps;
            pv[j] = p0[j] - lr1 * (m / denom);
            mo[j] = m; vo[j] = v; dst[j] = pv[j];
        }
    }
    if (valid > 0) { *reinterpret_cast<f32x4*>(P.m + si) = mo; *reinterpret_cast<f32x4*>(P.v + si) = vo; }
    __bf16* wp = P.wpack + (size_t)net * kPackElems;
    float r[kAdamVec] = {pv[0], pv[1], pv[2], pv[3]};
    bf16x4_t hp[2];
    if (P.planes == 2) split_quad<2>(r, hp, Fmt<2>::kSW);          // two fp16 planes of the weight x 2^8 (Fmt<2>)
    for (int pl = 0; pl < P.planes; ++pl) {
        bf16x4 b;
        if (P.planes == 2) b = hp[pl];
        else {
#pragma unroll
            for (int j = 0; j < kAdamVec; ++j) { b[j] = (__bf16)r[j]; r[j] -= (float)b[j]; }
        }
        __bf16* w = wp + (size_t)pl * kWPlane;
        if (wp0 >= 0) *reinterpret_cast<bf16x4*>(w + wp0) = b;
#pragma unroll
        for (int j = 0; j < kAdamVec; ++j) if (wp1[j] >= 0) w[wp1[j]] = b[j];
    }
    if (bp >= 0) *reinterpret_cast<f32x4*>(P.bias + net * kBiasElems + bp) = f32x4{pv[0], pv[1], pv[2], pv[3]};
}

}  // namespace pnr
#pragma clang fp contract(off)
