// pnr_mlp_backward.h — mlp_backward_data_kernel: the backward-data pass as a launch of its own, from saved activations
// (pnr_mlp_backward, the autograd path; the learner's own runs inside mlp_forward_kernel<true>).
#pragma once

#include "pnr_mlp.h"
#pragma clang fp contract(fast)      // as in pnr_mlp.h: the TU is compiled -ffp-contract=off for the env integrator
namespace pnr {

struct MlpBwdParams {
    const float* g_head;       // [2][B][16] d loss / d head (float32)
    const __bf16* wpack;       // [2][kPackElems]
    const __bf16* h1;          // [2][B][256]
    const __bf16* h2;          // [2][B][256]
    __bf16* dz1;               // [2][B][256] d loss / d (pre-activation of layer 1)
    __bf16* dz2;               // [2][B][256]
    long long B;
};

// Backward-data of one BM-sample tile: dZ2 = (G W3) * (1 - H2^2), dZ1 = (dZ2 W2) * (1 - H1^2).
__global__ __launch_bounds__(kMlpThreads) void mlp_backward_data_kernel(const MlpBwdParams P)
{
    __shared__ __attribute__((aligned(16))) __bf16 lds[2 * kMlpBM * kHS + kMlpBM * kGS];
    __bf16* ht = lds;                       // H2, then H1
    __bf16* dz = lds + kMlpBM * kHS;        // dZ2, then dZ1
    __bf16* gt = lds + 2 * kMlpBM * kHS;    // head gradients as bf16 [BM][16]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int net = blockIdx.y;
    const long long row0 = (long long)blockIdx.x * kMlpBM;
    const __bf16* wp = P.wpack + (size_t)net * kPackElems;
    const int c = lane & 31, h = lane >> 5;

    if (tid < 2 * kMlpBM) {   // head gradients: thread = (row, half): eight floats -> one ds_write_b128
        const int row = tid >> 1, half = tid & 1;
        bf16x8 pk;
        f32x4 g0 = {0.f, 0.f, 0.f, 0.f}, g1 = g0;
        if (row0 + row < P.B) {
            const float* gp = P.g_head + ((size_t)net * P.B + row0 + row) * kMlpHead + 8 * half;
            g0 = *reinterpret_cast<const f32x4*>(gp); g1 = *reinterpret_cast<const f32x4*>(gp + 4);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { pk[j] = (__bf16)g0[j]; pk[4 + j] = (__bf16)g1[j]; }
        *reinterpret_cast<bf16x8*>(gt + row * kGS + 8 * half) = pk;
    }
    mlp_load_htile(ht, P.h2 + (size_t)net * P.B * kMlpHid, row0, P.B, tid);
    mlp_barrier();

    f32x16 acc[2][kMlpCB];
    // acc * (1 - h^2) with h from the activation tile, packed into the gradient tile (same quad layout as forward)
    const auto epilogue = [&]() {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int cb = 0; cb < kMlpCB; ++cb)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int off = (32 * cb + c) * kHS + 64 * w + 32 * rb + 8 * q + 4 * h;
                    const bf16x4 hv = *reinterpret_cast<const bf16x4*>(ht + off);
                    bf16x4 pk;
#pragma unroll
                    for (int j = 0; j < 4; ++j) { const float hf = (float)hv[j]; pk[j] = (__bf16)(acc[rb][cb][4 * q + j] * (1.0f - hf * hf)); }
                    *reinterpret_cast<bf16x4*>(dz + off) = pk;
                }
    };

    // ---- dH2^T = W3^T . G^T: one k-step of 16 (the padded head rows are zero)
    mlp_zero_acc(acc);
    {
        const __bf16* wa = wp + kOffW3T + 2 * w * 512 + lane * 8;     // fragment-native, one k-step per row-block
        bf16x8 a[2] = {ld_global_bf16x8(wa), ld_global_bf16x8(wa + 512)};
        bf16x8 b[kMlpCB];
#pragma unroll
        for (int cb = 0; cb < kMlpCB; ++cb) b[cb] = *reinterpret_cast<const bf16x8*>(gt + (32 * cb + c) * kGS + 8 * h);
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int cb = 0; cb < kMlpCB; ++cb)
                acc[rb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[rb], b[cb], acc[rb][cb], 0, 0, 0);
    }
    // the H1 tile is requested now (16 x 16 bytes per thread, held in registers) and lands under the epilogue below
    uint4 h1r[kMlpBM / 8];
    {
        const __bf16* src = P.h1 + (size_t)net * P.B * kMlpHid;
#pragma unroll
        for (int i = 0; i < kMlpBM / 8; ++i) {
            const int ch = tid + kMlpThreads * i, row = ch >> 5, cc = ch & 31;
            h1r[i] = make_uint4(0u, 0u, 0u, 0u);
            if (row0 + row < P.B) h1r[i] = *reinterpret_cast<const uint4*>(src + (row0 + row) * kMlpHid + cc * 8);
        }
    }
    epilogue();
    mlp_barrier();                                                               // every wave is done with H2
    mlp_store_htile(dz, P.dz2 + (size_t)net * P.B * kMlpHid, row0, P.B, tid);
#pragma unroll
    for (int i = 0; i < kMlpBM / 8; ++i) {
        const int ch = tid + kMlpThreads * i, row = ch >> 5, cc = ch & 31;
        *reinterpret_cast<uint4*>(ht + row * kHS + cc * 8) = h1r[i];
    }
    mlp_barrier();

    // ---- dH1^T = W2^T . dZ2^T
    mlp_zero_acc(acc);
    MlpGemm<kMlpHid, kHS> g;
    g.prefetch(wp + kOffW2T + 2 * w * (kMlpHid / 16) * 512, lane);
    g.run(dz, acc, lane, [] {});
    mlp_barrier();                         // all reads of dZ2 done before it is overwritten
    epilogue();
    mlp_barrier();
    mlp_store_htile(dz, P.dz1 + (size_t)net * P.B * kMlpHid, row0, P.B, tid);
}

}  // namespace pnr
#pragma clang fp contract(off)
