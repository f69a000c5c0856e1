// pnr_mlp.h — the PPO host driver's two MLPs (policy 137-256-256-12, value 137-256-256-1, tanh; the nets of
// pioneer/launch/pioneer_knm_train.py:59-61 under RLlib's FullyConnectedNetwork with vf_share_layers False) as
// hand-written bf16 MFMA kernels for gfx950: forward (three layers fused, activations never leave the CU between
// layers), backward-data (two layers fused), weight gradients (split over the batch axis into per-slice slabs,
// reduced in a fixed order: deterministic) and the weight packing.  Master weights stay float32 in the caller's
// tensors; bf16 copies (K padded 137 -> 144, head rows padded to 16, plus the transposes the backward pass reads)
// are packed once per update.
//
// Orientation.  Every GEMM is computed TRANSPOSED, Y^T = W . X^T, with the weight matrix as the MFMA's A operand
// (rows = output features; fragments are 16-byte loads straight from the packed row-major weights in L2) and the
// activation tile as the B operand (columns = samples; fragments are ds_read_b128 from a row-major [sample][feature]
// LDS tile).  A 32x32 accumulator block then holds, per lane, ONE sample (its column) and FOUR CONSECUTIVE features
// per register quad (rows (reg&3) + 8 (reg>>2) + 4 (lane>>5)): bias + tanh run in registers and each quad leaves as
// one 8-byte ds_write_b64 into the next layer's row-major tile — no 2-byte LDS stores, no lane shuffles.
// Weight gradients sum over SAMPLES, so both operands must be sample-contiguous per lane: they are read from the
// row-major LDS tiles with ds_read_b64_tr_b16 (the hardware 4x16 transpose read), rows strided 16 dwords mod 64 so
// that the transposed reads are bank-conflict-free.
//
// Work per sample and net: forward 106 496 MAC, backward-data 69 632 MAC, weight gradients 110 592 MAC.  These are
// 256-wide layers on 137-float inputs: measured (profiles/r02_*) the kernels sit at 0.6-0.8 PFLOP/s
// of the ~2.5 dense bf16 peak and 3-5 TB/s of HBM — bound by the chain of dependent products per tile and by the bytes
// of the saved activations, not by the matrix cores.
//
// This header: what every learner kernel is made of — layouts, the operand formats (Fmt, split_*, SplitPairs, mfma*), tanh, mlp_barrier,
// the products (MlpGemm, MlpGemm1), the hidden tile's copies, mlp_bias16, mlp_filter, the stamp macros — and mlp_pack_kernel.  The other
// kernels sit in a header each: pnr_mlp_forward.h (mlp_forward_kernel<FUSED, NS>; FUSED: + the tile's loss, backward-data and layer-3
// weight-gradient partials), pnr_mlp_gather.h (record_pack_kernel, mlp_gather_kernel), pnr_mlp_backward.h (mlp_backward_data_kernel),
// pnr_mlp_wgrad.h (mlp_wgrad_kernel, the two reduce kernels), pnr_mlp_adam.h (mlp_adam_kernel); pnr_sampler.h needs this header alone.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

// The TU is compiled -ffp-contract=off for the bit-exact env integrator; nothing here needs that: the epilogues
// (bias + tanh, (1 - h^2) dz, the filter, Adam) are a quarter of the fused kernel's issue slots and fuse into FMAs.
#pragma clang fp contract(fast)

namespace pnr {

constexpr int kMlpIn = 137;       // observation entries (pioneer_knm_env.py:194-211)
constexpr int kMlpInPad = 144;    // K of the first layer, padded to a multiple of 16 (zero columns)
constexpr int kMlpHid = 256;      // fcnet_hiddens [256, 256] (pioneer_knm_train.py:60)
constexpr int kMlpAct = 6;        // action dimensions (means 0..5, log-stds 6..11 of the policy head)
constexpr int kMlpHead = 16;      // head rows: 12 (6 means + 6 log-stds) or 1 (value), zero-padded to 16
constexpr int kMlpNets = 2;       // policy, value
constexpr int kMlpBM = 64;        // samples per workgroup tile (forward / backward-data): 53 / 71 KB of LDS and <= 256 registers, i.e.
                                  // two workgroups per CU whose phases overlap (128 rows left room for one: the A/B in DESIGN.md)
constexpr int kMlpCB = 2;         // 32-sample column blocks per tile
// PNR_MLP_DIAG: timing-only ablations of the forward kernel (results are wrong when set; tools/mlp_ablation.py): 1 no tanh,
// 2 no observation loads, 4 / 8 no layer-2 / layer-1 product, 16 no head, 32 no forward epilogues, 64 no tile stores (h1, h2,
// dz2, dz1), 128 no H1 reload, 256 no loss (record loads and arithmetic), 512 half the products' sample-fragment LDS reads
#ifndef PNR_MLP_RING
#define PNR_MLP_RING 5            // depth of the weight-fragment prefetch ring (A/B: tools/mlp_ab.sh)
#endif
#ifndef PNR_MLP_DIAG
#define PNR_MLP_DIAG 0
#endif
#ifndef PNR_MLP_LDS_PAD
#define PNR_MLP_LDS_PAD 0          // bf16 elements of unused LDS in the fused kernel: 20000 leaves ONE workgroup per CU (occupancy probe, tools/stamps.sh)
#endif
constexpr int kMlpThreads = 256;  // four waves
// PNR_MLP_STAMPS=1 (a diagnostic variant, tools/mlp_stamps.py): every wave of the fused kernel writes s_memtime at its phase
// boundaries into a buffer of its own (no output depends on it).  The product build carries none of it.
#ifndef PNR_MLP_STAMPS
#define PNR_MLP_STAMPS 0
#endif
constexpr int kMlpStampSlots = 26;   // 0..22 phase boundaries (s_memtime), 23 HW_REG_XCC_ID << 32 | HW_REG_HW_ID, 24 / 25 s_memrealtime (100 MHz) at start / end
#if PNR_MLP_STAMPS
// The stamps wait in LDS and leave for global memory at the kernel's end: written to global memory where they are taken (r03b - r03i),
// every stamp was a store that the next s_waitcnt vmcnt(..) of the wave — the weight ring's, in order — also waited for, i.e. the
// instrument stretched exactly the phases it was pointed at (found on mlp_wgrad_kernel, r03i).
#define MLP_STAMP_DECL __shared__ unsigned long long stamp_lds_[kFwdWaves][kMlpStampSlots]
#define MLP_STAMP(i) do { if (P.stamps && lane == 0) { stamp_lds_[w][(i)] = __builtin_amdgcn_s_memtime(); \
    if ((i) == 0) { stamp_lds_[w][24] = __builtin_amdgcn_s_memrealtime(); \
        stamp_lds_[w][23] = ((unsigned long long)__builtin_amdgcn_s_getreg(0xF814) << 32) | __builtin_amdgcn_s_getreg(0xF804); }   /* XCC_ID | HW_ID: where the wave runs */ \
    if ((i) == 22) stamp_lds_[w][25] = __builtin_amdgcn_s_memrealtime(); } } while (0)
#define MLP_STAMP_FLUSH do { if (P.stamps && lane < kMlpStampSlots) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
    P.stamps[(((size_t)blockIdx.x * stamp_ny_ + stamp_yi_) * kFwdWaves + w) * kMlpStampSlots + lane] = stamp_lds_[w][lane]; } } while (0)
#else
#define MLP_STAMP_DECL
#define MLP_STAMP(i) do { } while (0)
#define MLP_STAMP_FLUSH do { } while (0)
#endif

// packed bf16 weights of ONE net, element offsets.  Every matrix is stored FRAGMENT-NATIVE: the 32 x 16 (or 16 x 32) block
// that one MFMA consumes as its A operand is 1 KiB contiguous in lane order, so a wave's fragment load is one fully
// coalesced dwordx4 instruction (8 whole 128-byte lines).  Row-major weights made every fragment load touch 32
// different lines for 32 bytes each: 16.9 M L2 requests per 131 072-sample forward, the kernel's bottleneck
// (profiles/r02_d_mlp_forward_counters.json); the permutation costs nothing, the packing kernels apply it.
constexpr int kOffW1 = 0;                                  // [256][144]  as (rows / 32) x 9 blocks
constexpr int kOffW2 = kOffW1 + kMlpHid * kMlpInPad;       // [256][256]  as 8 x 16 blocks
constexpr int kOffW3 = kOffW2 + kMlpHid * kMlpHid;         // [16][256]   as 8 blocks of 16 x 32
constexpr int kOffW2T = kOffW3 + kMlpHead * kMlpHid;       // [256][256]  W2T[i][o] = W2[o][i], 8 x 16 blocks
constexpr int kOffW3T = kOffW2T + kMlpHid * kMlpHid;       // [256][16]   W3T[f][r] = W3[r][f], 8 x 1 blocks
constexpr int kPackElems = kOffW3T + kMlpHid * kMlpHead;   // 176 128
constexpr int kBiasElems = 2 * kMlpHid + kMlpHead;         // b1[256] b2[256] b3[16], float32
constexpr size_t kWPlane = (size_t)kMlpNets * kPackElems;  // elements between two PLANES of the packed weights ([planes][2][kPackElems]; r04, split float32 operands)

// gradient slab of ONE net and ONE batch slice, float32 element offsets (also the layout of the reduced gradient)
constexpr int kGW1 = 0;                                    // [256][144]
constexpr int kGW2 = kGW1 + kMlpHid * kMlpInPad;           // [256][256]
constexpr int kGW3 = kGW2 + kMlpHid * kMlpHid;             // [16][256]
constexpr int kGB1 = kGW3 + kMlpHead * kMlpHid;            // [256]
constexpr int kGB2 = kGB1 + kMlpHid;                       // [256]
constexpr int kGB3 = kGB2 + kMlpHid;                       // [16]
constexpr int kGradElems = kGB3 + kMlpHead;                // 107 024

// element offset of A[row][k] inside a matrix packed as 32 x 16 blocks (K = 16 KS): block (row / 32, k / 16), then the
// mfma_f32_32x32x16_bf16 A-operand lane map: lane = row % 32 + 32 * (k / 8 % 2), element k % 8
__host__ __device__ constexpr int frag32_off(int row, int k, int KS)
{
    return ((((row >> 5) * KS + (k >> 4)) * 64) + (row & 31) + 32 * ((k >> 3) & 1)) * 8 + (k & 7);
}
// the same for a 16-row matrix consumed by mfma_f32_16x16x32_bf16: block k / 32, lane = row + 16 * (k / 8 % 4)
__host__ __device__ constexpr int frag16_off(int row, int k)
{
    return (((k >> 5) * 64) + row + 16 * ((k >> 3) & 3)) * 8 + (k & 7);
}

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// LDS row strides (bf16 elements).  Tiles read with ds_read_b128 as the B operand: rows 16-byte aligned and
// shifted 4 (12) dwords mod 64, conflict-free for the four 16-lane groups.  Tiles read with ds_read_b64_tr_b16:
// rows shifted 16 dwords mod 64 (four rows x 16 dwords cover the 64 banks).
constexpr int kXS = 152;          // row stride of the [BM][144] input tile
constexpr int kHS = 264;          // row stride of the [BM][256] hidden tile
constexpr int kGS = 24;           // row stride of the [BM][16] head-gradient tile
constexpr int kTrH = 288;         // [64][256] tile for transposed reads (144 dwords = 16 mod 64)
constexpr int kTrX = 160;         // [64][160] (80 dwords = 16 mod 64): 144 inputs, a column of ones, zeros
constexpr int kTrHalf = 160;      // [64][128] half-width hidden tile (+32 pad)
constexpr int kTrG = 32;          // [64][16] head-gradient tile (16 dwords)
constexpr int kTilePlane = kMlpBM * kXS + kMlpBM * kHS;   // elements of one LDS plane of the forward / fused kernel (input tile | hidden tile)
constexpr int kWgChunk = 64;      // samples per weight-gradient chunk
constexpr int kWgParts = 4;       // weight-gradient workgroup roles (mlp_wgrad_kernel)

struct MlpNetParams {             // float32 master parameters of one net (torch nn.Linear layouts)
    const float* w1; const float* b1;   // [256][137], [256]
    const float* w2; const float* b2;   // [256][256], [256]
    const float* w3; const float* b3;   // [n3][256], [n3]
    int n3;                             // 12 (policy) or 1 (value)
};

// tanh through one exp2 and one reciprocal: 1 - 2 / (e^{2x} + 1); saturates correctly at +-inf.  Absolute error
// ~1e-7, far below the bf16 rounding of the stored activation.
__device__ __forceinline__ float tanh_fast(float x)
{
    const float e = __builtin_amdgcn_exp2f(x * 2.885390081777927f);      // 2 log2(e)
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}

// The same for two values, the three non-transcendental steps as packed instructions (v_pk_mul_f32, v_pk_add_f32, v_pk_fma_f32:
// one issue slot for both): per element the roundings of tanh_fast (2 r is exact, so the fused last step changes nothing).
// The learner kernels are bound by vector-instruction ISSUE (r03f: ~900 vector + 112 transcendental instructions per wave and
// tile against 84 MFMAs), not by the matrix pipe: every instruction taken out of the epilogues is time.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 tanh_fast2(f32x2 x)
{
    const f32x2 t = x * (f32x2){2.885390081777927f, 2.885390081777927f};
    f32x2 e = {__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])};
    e = e + (f32x2){1.0f, 1.0f};
    const f32x2 r = {__builtin_amdgcn_rcpf(e[0]), __builtin_amdgcn_rcpf(e[1])};
    return __builtin_elementwise_fma(r, (f32x2){-2.0f, -2.0f}, (f32x2){1.0f, 1.0f});
}
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));

// ---- r04: float32-accurate operands as SPLIT bf16 planes.  The reference's learner is float32 torch (pioneer_knm_train.py:47
// 'framework': 'torch', no mixed precision); one bf16 operand carries 8 significant bits.  A float32 value x is written as the sum of
// NS bf16 numbers, p0 = bf16(x), p1 = bf16(x - p0), p2 = bf16(x - p0 - p1) (each residual is exact in float32): 16 significant bits
// with two planes, 24 — all of float32 — with three.  A product a . b then takes the bf16 MFMAs of the plane pairs (i, j) with
// i + j < NS — 3 for NS = 2 (error ~2^-16: 8e-6 relative on the heads), 6 for NS = 3 (1.5e-7, the accuracy of a float32 GEMM) —
// accumulated in float32 like every product here.  Against the native float32 MFMA (v_mfma_f32_32x32x2_f32: 2 048 MAC in 64
// cycles per SIMD = 32 MAC/cycle) six bf16 MFMAs per 16 384 MAC (192 cycles = 85 MAC/cycle) are 2.7x the matrix-pipe rate, three
// are 5.3x (MI355X_MICROARCH.md cycle constants; tools/f32_product_probe.hip measures the three forms on the layer-2 product).
// Every tensor that is an MFMA operand exists as NS planes of the bf16 layout (packed weights, input rows, the LDS tiles, the saved
// activations and gradients); biases, heads, the loss, slabs, Adam and the master weights are float32 as before.  NS = 1 is the
// bf16 path, instruction for instruction what it was.
// ---- r05: NS = 2 is TWO FP16 PLANES, power-of-two scaled — the float32-accurate path ("f32").  An fp16 number carries 11
// significant bits, so two planes carry 22 of float32's 24 and the three products (0,0), (0,1), (1,0) leave an operand error of
// 2^-22: measured against float64 the heads are at 2.4e-7 and the weight gradients at 1.5-3.4e-7 relative, BELOW what a float32
// GEMM's own accumulation leaves (torch float32: 4.3e-7 / 4.4-6.7e-7; tools/split_accuracy.py) — at HALF the
// MFMAs and two thirds of the bytes of the three-bf16-plane form (NS = 3, kept: exact 24-bit split, no range caveat).  fp16's
// exponent range is the price: every operand tensor is stored multiplied by a power of two (exact; the accumulators are divided
// by the product of the two scales, also exact) so that residual planes stay out of the subnormals, and is clamped to +-65504:
//   weights x 2^8 (|w| < 255), activations tanh(.) x 2^8, net inputs x 2^4 (|x| < 4094: the filter clamps to +-10; raw obs <= 126),
//   gradients dZ, G x gscale = 4 * 2^ceil(log2 B) (per-sample |d loss / d z| < 16 384 before the 1 / B; larger ones saturate —
//   a float32 learner would be taking a step of that size, i.e. has already diverged).
// Buffers keep their __bf16 element type (16-bit payloads); Fmt<NS> says what the bits mean.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
template <int NS> struct Fmt {
    static constexpr bool kHalf = NS == 2;
    static constexpr float kSW = kHalf ? 256.f : 1.f;      // weights
    static constexpr float kSH = kHalf ? 256.f : 1.f;      // activations
    static constexpr float kSX = kHalf ? 16.f : 1.f;       // net inputs
};
constexpr float kHalfMax = 65504.f;
__host__ __device__ inline float mlp_grad_scale(int planes, long long B)      // gscale of a batch of B samples (1 unless planes == 2)
{
    if (planes != 2) return 1.f;
    float g = 4.f;
    for (long long n = 1; n < B; n <<= 1) g *= 2.f;
    return g;
}
__device__ __forceinline__ __bf16 half_bits(float v) { return __builtin_bit_cast(__bf16, (_Float16)v); }
__device__ __forceinline__ float half_value(__bf16 b) { return (float)__builtin_bit_cast(_Float16, b); }
// v * scale as NS planes: bf16 planes p0 = bf16(x), p1 = bf16(x - p0), .. (scale must be 1); fp16 planes of clamp(v * scale)
template <int NS>
__device__ __forceinline__ void split_quad(const float (&v)[4], bf16x4_t (&pk)[NS], float scale = 1.f)
{
    if constexpr (Fmt<NS>::kHalf) {
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = __builtin_amdgcn_fmed3f(v[j] * scale, -kHalfMax, kHalfMax);
        pk[0] = (bf16x4_t){half_bits(r[0]), half_bits(r[1]), half_bits(r[2]), half_bits(r[3])};
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] -= half_value(pk[0][j]);
        pk[1] = (bf16x4_t){half_bits(r[0]), half_bits(r[1]), half_bits(r[2]), half_bits(r[3])};
    } else {
        float r[4] = {v[0], v[1], v[2], v[3]};
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            pk[s] = (bf16x4_t){(__bf16)r[0], (__bf16)r[1], (__bf16)r[2], (__bf16)r[3]};
            if (s + 1 < NS) {
#pragma unroll
                for (int j = 0; j < 4; ++j) r[j] -= (float)pk[s][j];
            }
        }
    }
}
template <int NS>
__device__ __forceinline__ void split_scalar(float v, __bf16 (&p)[NS], float scale = 1.f)
{
    if constexpr (Fmt<NS>::kHalf) {
        float r = __builtin_amdgcn_fmed3f(v * scale, -kHalfMax, kHalfMax);
        p[0] = half_bits(r); r -= half_value(p[0]); p[1] = half_bits(r);
    } else {
        float r = v;
#pragma unroll
        for (int s = 0; s < NS; ++s) { p[s] = (__bf16)r; r -= (float)p[s]; }
    }
}
// the value NS planes add up to (the float32 original for bf16 planes; its 22-bit neighbour / scale for fp16 planes)
template <int NS>
__device__ __forceinline__ f32x4 planes_value(const bf16x4_t (&pk)[NS], float inv_scale = 1.f)
{
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = NS - 1; s >= 0; --s)
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] += Fmt<NS>::kHalf ? half_value(pk[s][j]) : (float)pk[s][j];
    if constexpr (Fmt<NS>::kHalf) x *= inv_scale;
    return x;
}
// the MFMAs on 16-bit payloads: bf16, or fp16 (NS == 2)
template <bool HALF>
__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c)
{
    if constexpr (HALF) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
template <bool HALF>
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c)
{
    if constexpr (HALF) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// the plane pairs of a product in the order they are accumulated: the large term first (it may carry the bias as its C operand)
template <int NS> struct SplitPairs;
template <> struct SplitPairs<1> { static constexpr int n = 1; static constexpr int a[1] = {0}, b[1] = {0}; };
template <> struct SplitPairs<2> { static constexpr int n = 3; static constexpr int a[3] = {0, 0, 1}, b[3] = {0, 1, 0}; };
template <> struct SplitPairs<3> { static constexpr int n = 6; static constexpr int a[6] = {0, 0, 1, 0, 2, 1}, b[6] = {0, 1, 0, 2, 0, 1}; };
constexpr int kMlpMaxPlanes = 3;

struct MlpPackParams { MlpNetParams net[kMlpNets]; __bf16* wpack; float* bias; int planes; };   // wpack: [planes][2][kPackElems]

// One thread per packed element; the transposes and the zero padding happen here, once per update.
__global__ __launch_bounds__(256) void mlp_pack_kernel(const MlpPackParams P)
{
    const int net = blockIdx.y;
    const MlpNetParams& N = P.net[net];
    const int e = blockIdx.x * 256 + threadIdx.x;
    __bf16* wp = P.wpack + (size_t)net * kPackElems;
    if (e < kPackElems) {
        // e walks the SOURCE matrices in row-major order; the destination is the fragment-native position
        float v; int dst;
        if (e < kOffW2) { const int o = e / kMlpInPad, k = e % kMlpInPad; v = k < kMlpIn ? N.w1[o * kMlpIn + k] : 0.f; dst = kOffW1 + frag32_off(o, k, kMlpInPad / 16); }
        else if (e < kOffW3) { const int r = e - kOffW2, o = r / kMlpHid, i = r % kMlpHid; v = N.w2[r]; dst = kOffW2 + frag32_off(o, i, kMlpHid / 16); }
        else if (e < kOffW2T) { const int r = (e - kOffW3) / kMlpHid, f = (e - kOffW3) % kMlpHid; v = r < N.n3 ? N.w3[r * kMlpHid + f] : 0.f; dst = kOffW3 + frag16_off(r, f); }
        else if (e < kOffW3T) { const int i = (e - kOffW2T) / kMlpHid, o = (e - kOffW2T) % kMlpHid; v = N.w2[o * kMlpHid + i]; dst = kOffW2T + frag32_off(i, o, kMlpHid / 16); }
        else { const int f = (e - kOffW3T) / kMlpHead, r = (e - kOffW3T) % kMlpHead; v = r < N.n3 ? N.w3[r * kMlpHid + f] : 0.f; dst = kOffW3T + frag32_off(f, r, 1); }
        if (P.planes == 2) {                             // two fp16 planes of the weight x 2^8 (Fmt<2>)
            __bf16 b[2];
            split_scalar<2>(v, b, Fmt<2>::kSW);
            wp[dst] = b[0]; wp[kWPlane + dst] = b[1];
        } else {
            for (int pl = 0; pl < P.planes; ++pl) {      // plane pl carries what planes 0 .. pl - 1 left of the value
                const __bf16 b = (__bf16)v;
                wp[pl * kWPlane + dst] = b;
                v -= (float)b;
            }
        }
    } else if (e < kPackElems + kBiasElems) {
        const int b = e - kPackElems;
        float v;
        if (b < kMlpHid) v = N.b1[b];
        else if (b < 2 * kMlpHid) v = N.b2[b - kMlpHid];
        else v = (b - 2 * kMlpHid) < N.n3 ? N.b3[b - 2 * kMlpHid] : 0.f;
        P.bias[net * kBiasElems + b] = v;
    }
}

// tanh of accumulator quad q (four consecutive features of one sample), rounded to bf16
template <class ACC>
__device__ __forceinline__ bf16x4_t tanh_quad(const ACC& acc, int q)
{
    const f32x2 lo = tanh_fast2((f32x2){acc[4 * q], acc[4 * q + 1]}), hi = tanh_fast2((f32x2){acc[4 * q + 2], acc[4 * q + 3]});
    return (bf16x4_t){(__bf16)lo[0], (__bf16)lo[1], (__bf16)hi[0], (__bf16)hi[1]};
}
// accumulator quad q times tanh' = 1 - h^2 of the stored activations hv, rounded to bf16.  h has 8 significant bits, h * h is
// exact in float32: the fused 1 - h * h rounds once, like the product-then-subtract it replaces — same bits, half the instructions
template <class ACC>
__device__ __forceinline__ bf16x4_t dtanh_quad(const ACC& acc, int q, bf16x4_t hv)
{
    const f32x2 h0 = {(float)hv[0], (float)hv[1]}, h1 = {(float)hv[2], (float)hv[3]};
    const f32x2 one = {1.0f, 1.0f};
    const f32x2 d0 = __builtin_elementwise_fma(-h0, h0, one), d1 = __builtin_elementwise_fma(-h1, h1, one);
    const f32x2 p0 = (f32x2){acc[4 * q], acc[4 * q + 1]} * d0, p1 = (f32x2){acc[4 * q + 2], acc[4 * q + 3]} * d1;
    return (bf16x4_t){(__bf16)p0[0], (__bf16)p0[1], (__bf16)p1[0], (__bf16)p1[1]};
}

__device__ __forceinline__ bf16x8 ld_global_bf16x8(const __bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }

// Workgroup rendezvous for hand-offs that go through LDS only (every tile exchange in these kernels): the wave's DS operations
// have completed (lgkmcnt), then s_barrier.  __syncthreads() additionally waits for vmcnt(0), i.e. for every global store
// and prefetched weight fragment still in flight — each barrier then costs a write acknowledgement from HBM (the tile stores of
// h1 / h2 / dz2 / dz1) or an L2 round trip (the next product's first weight fragments).
__device__ __forceinline__ void mlp_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// acc[rb][cb] += W[64 rows of this wave][K] . tile[BM samples][K]^T.  W: fragment-native packing (global, L2);
// tile: LDS, row stride STRIDE.  Two steps, so that the first D - 1 k-steps of weight fragments can be requested EARLY
// (prefetch()): ahead of a tile store to HBM — a wave's vector-memory operations return in order, so fragments requested
// behind a 32 KB store wait for its acknowledgement — and ahead of the epilogue / barrier in front of the product.
template <int K, int STRIDE>
struct MlpGemm {
    static constexpr int KS = K / 16;
    static constexpr int D = PNR_MLP_RING;     // A fragments run D - 1 k-steps ahead of their use (L2 latency ~ 2-3 k-steps of MFMAs)
    bf16x8 a[D][2];
    const __bf16* wa;
    // w_blocks: the first of this wave's two row-blocks in the fragment-native packing: block (rb, ks) at (rb KS + ks) * 512
    __device__ __forceinline__ void prefetch(const __bf16* __restrict__ w_blocks, int lane)
    {
        wa = w_blocks + lane * 8;
#pragma unroll
        for (int p = 0; p < D - 1; ++p) {
            if (p < KS) {
                a[p][0] = ld_global_bf16x8(wa + 512 * p);
                a[p][1] = ld_global_bf16x8(wa + 512 * (KS + p));
            }
        }
    }
    // `after_loads` runs once, right behind the product's LAST fragment load (k-step KS - D): the place for a tile store to
    // HBM — nothing this product still needs can queue behind it, and it drains under the remaining MFMAs and the epilogue
    template <class F>
    __device__ __forceinline__ void run(const __bf16* tile, f32x16 (&acc)[2][kMlpCB], int lane, F&& after_loads)
    {
        const int r = lane & 31, h = lane >> 5;
        const __bf16* tb = tile + r * STRIDE + 8 * h;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (ks + D - 1 < KS) {
                a[(ks + D - 1) % D][0] = ld_global_bf16x8(wa + 512 * (ks + D - 1));
                a[(ks + D - 1) % D][1] = ld_global_bf16x8(wa + 512 * (KS + ks + D - 1));
            }
            if (ks == (KS > D ? KS - D : 0)) {
                __builtin_amdgcn_sched_barrier(0);
                after_loads();
                __builtin_amdgcn_sched_barrier(0);
            }
            bf16x8 b[kMlpCB];
#pragma unroll
            for (int cb = 0; cb < kMlpCB; ++cb) b[cb] = *reinterpret_cast<const bf16x8*>(tb + cb * 32 * STRIDE + 16 * ks);
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int cb = 0; cb < kMlpCB; ++cb)
                    acc[rb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks % D][rb], b[cb], acc[rb][cb], 0, 0, 0);
        }
    }
};

// zero a wave's accumulator blocks
template <int N>
__device__ __forceinline__ void mlp_zero_acc(f32x16 (&acc)[N])
{
#pragma unroll
    for (int b = 0; b < N; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[b][i] = 0.f;
}
template <int M, int N>
__device__ __forceinline__ void mlp_zero_acc(f32x16 (&acc)[M][N])
{
#pragma unroll
    for (int a = 0; a < M; ++a) mlp_zero_acc(acc[a]);
}

// a wave's four 16-byte bias pieces of a layer (rows 32 w + 8 k + 4 h .. of b), and the four as ONE 16-register value: the first MFMA's C
// operand (MlpGemm1::run's `init`).  SCALED (fp16 planes): times the product's scale, which the epilogue divides out again (both exact)
__device__ __forceinline__ void mlp_bias_load(const float* b, int w, int h, f32x4 (&q)[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = *reinterpret_cast<const f32x4*>(b + 32 * w + 8 * k + 4 * h);
}
template <bool SCALED = false>
__device__ __forceinline__ f32x16 mlp_bias16(const f32x4 (&q)[4], float scale = 1.f)
{
    f32x16 b;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) b[4 * k + j] = SCALED ? q[k][j] * scale : q[k][j];
    return b;
}

// copy a [BM][256] bf16 tile between LDS (row stride kHS) and row-major global rows [row0, row0 + BM) of n_rows (kMlpThreads threads;
// mlp_store_htile_nt below is the fused kernel's form)
__device__ __forceinline__ void mlp_store_htile(const __bf16* tile, __bf16* __restrict__ dst, long long row0, long long n_rows, int tid)
{
#pragma unroll
    for (int i = 0; i < kMlpBM / 8; ++i) {
        const int ch = tid + kMlpThreads * i, row = ch >> 5, cc = ch & 31;
        if (row0 + row < n_rows)
            *reinterpret_cast<uint4*>(dst + (row0 + row) * kMlpHid + cc * 8) = *reinterpret_cast<const uint4*>(tile + row * kHS + cc * 8);
    }
}
__device__ __forceinline__ void mlp_load_htile(__bf16* tile, const __bf16* __restrict__ src, long long row0, long long n_rows, int tid)
{
#pragma unroll
    for (int i = 0; i < kMlpBM / 8; ++i) {
        const int ch = tid + kMlpThreads * i, row = ch >> 5, cc = ch & 31;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (row0 + row < n_rows) v = *reinterpret_cast<const uint4*>(src + (row0 + row) * kMlpHid + cc * 8);
        *reinterpret_cast<uint4*>(tile + row * kHS + cc * 8) = v;
    }
}

// ---- the forward / fused kernel's own geometry: EIGHT waves per 64-sample tile, each owning one 32-row block of every layer's
// output (r02 - r03b ran four waves with two row blocks each).  What decides the launch time is the length of a tile's dependent
// chain — a tile took 44 500 cycles even alone on its CU (profiles/r03_c_mlp_stamps_one_workgroup_per_cu.json: 5 600 of them
// MFMA) — and per wave that chain is products + epilogues + tile stores + reload, all proportional to the rows a wave owns.
constexpr int kFwdWaves = 8;
constexpr int kFwdThreads = 64 * kFwdWaves;
static_assert(kFwdWaves * 32 == kMlpHid, "one 32-row block of the 256 hidden units per wave");

// the one-row-block product: acc[cb] += W[32 rows of this wave][K] . tile[BM samples][K]^T (see MlpGemm for the two steps)
template <int K, int STRIDE, int NS = 1, int PLANE = kTilePlane, int DEPTH = PNR_MLP_RING>
struct MlpGemm1 {
    static constexpr int KS = K / 16;
    static constexpr int D = DEPTH;
    bf16x8 a[D][NS];
    const __bf16* wa;
    // w_block: this wave's row block in the fragment-native packing: k-step ks at ks * 512 (plane s: + s * kWPlane)
    __device__ __forceinline__ void prefetch(const __bf16* __restrict__ w_block, int lane)
    {
        wa = w_block + lane * 8;
#pragma unroll
        for (int p = 0; p < D - 1; ++p)
            if (p < KS) {
#pragma unroll
                for (int s = 0; s < NS; ++s) a[p][s] = ld_global_bf16x8(wa + s * kWPlane + 512 * p);
            }
    }
    // init: what every column block's accumulators start from (the bias rows of this wave, the same for every sample), read as
    // the FIRST MFMA's C operand — 16 copies per column block and product less than accumulators initialised beforehand; or null
    // tile: plane 0 of the LDS tile (plane s: + s * PLANE)
    template <class F>
    __device__ __forceinline__ void run(const __bf16* tile, f32x16 (&acc)[kMlpCB], int lane, F&& after_loads, const f32x16* init = nullptr)
    {
        const int r = lane & 31, h = lane >> 5;
        const __bf16* tb = tile + r * STRIDE + 8 * h;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (ks + D - 1 < KS) {
#pragma unroll
                for (int s = 0; s < NS; ++s) a[(ks + D - 1) % D][s] = ld_global_bf16x8(wa + s * kWPlane + 512 * (ks + D - 1));
            }
            if (ks == (KS > D ? KS - D : 0)) {
                __builtin_amdgcn_sched_barrier(0);
                after_loads();
                __builtin_amdgcn_sched_barrier(0);
            }
            // (reading the sample fragments one k-step ahead of their MFMAs — 16 more registers — changed nothing in the fused
            // kernel and cost the sampler's forward 9 us of 14: r03, dropped)
            bf16x8 b[NS][kMlpCB];
#pragma unroll
            for (int s = 0; s < NS; ++s)
#pragma unroll
                for (int cb = 0; cb < kMlpCB; ++cb) {
                    // (PNR_MLP_DIAG & 512, timing only: ONE sample-fragment read per k-step serves both column blocks — what a
                    // 4 row-groups x 2 sample-halves wave layout would save in LDS reads, without its doubled weight stream)
                    if ((PNR_MLP_DIAG & 512) && cb > 0) b[s][cb] = b[s][0];
                    else b[s][cb] = *reinterpret_cast<const bf16x8*>(tb + s * PLANE + cb * 32 * STRIDE + 16 * ks);
                }
#pragma unroll
            for (int pi = 0; pi < SplitPairs<NS>::n; ++pi)
#pragma unroll
                for (int cb = 0; cb < kMlpCB; ++cb)
                    acc[cb] = mfma32<Fmt<NS>::kHalf>(a[ks % D][SplitPairs<NS>::a[pi]], b[SplitPairs<NS>::b[pi]][cb],
                                                     (ks == 0 && pi == 0 && init) ? *init : acc[cb]);
        }
    }
};

// a [BM][256] bf16 tile between LDS (row stride kHS) and row-major global rows, by NT threads
template <int NT>
__device__ __forceinline__ void mlp_store_htile_nt(const __bf16* tile, __bf16* __restrict__ dst, long long row0, long long n_rows, int tid)
{
    if (row0 + kMlpBM <= n_rows) {
        // a whole tile (every tile but the batch's last): one uniform test, the tile's 32 KB are contiguous in global memory — thread
        // offset + a constant per piece, no per-piece row test and no 64-bit row * stride (mlp_wgrad_kernel's lesson, r03i)
        __bf16* base = dst + row0 * kMlpHid + tid * 8;
#pragma unroll
        for (int i = 0; i < kMlpBM * 32 / NT; ++i) {
            const int ch = tid + NT * i, row = ch >> 5, cc = ch & 31;
            *reinterpret_cast<uint4*>(base + (size_t)i * NT * 8) = *reinterpret_cast<const uint4*>(tile + row * kHS + cc * 8);
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < kMlpBM * 32 / NT; ++i) {
        const int ch = tid + NT * i, row = ch >> 5, cc = ch & 31;
        if (row0 + row < n_rows)
            *reinterpret_cast<uint4*>(dst + (row0 + row) * kMlpHid + cc * 8) = *reinterpret_cast<const uint4*>(tile + row * kHS + cc * 8);
    }
}

// MeanStdFilter (PPOTrainer.filter.prepare()) on one entry: x = clamp((obs - loc) * inv, lo, hi); v(0) .. v(3) = the column's loc,
// inv, lo, hi, read where the expression uses them.  Used by stage 0 of mlp_forward_kernel, mlp_gather_kernel and ppo_rollout_kernel's
// first tile; the sampler's next-input step keeps the expression written out (its listing).  Their agreement, bit for bit, is tested
template <class V>
__device__ __forceinline__ float mlp_filter(float x, V&& v) { return fminf(fmaxf((x - v(0)) * v(1), v(2)), v(3)); }
// .. of column col, the four vectors staged in LDS as fv[4 * 144] = loc | inv | lo | hi
__device__ __forceinline__ float mlp_filter_col(float x, const float* fv, int col)
{
    return mlp_filter(x, [&](int i) { return fv[i * kMlpInPad + col]; });
}

}  // namespace pnr

#pragma clang fp contract(off)
