// pnr_mlp_forward.h — mlp_forward_kernel<FUSED, NS>: one 64-sample tile through one net and, FUSED, the tile's loss, backward-data pass
// and layer-3 weight-gradient partials in the same launch (pnr_mlp_forward, pnr_mlp_act, pnr_mlp_train_step), with what only it is made
// of: its parameter block, the tile's record (MlpRecordTile, MlpLossRec), mlp_tile_loss and the per-tile layer-3 products.
#pragma once

#include "pnr_mlp.h"
#include "pnr_ppo.h"
#pragma clang fp contract(fast)      // as in pnr_mlp.h: the TU is compiled -ffp-contract=off for the env integrator
namespace pnr {

// The tile's share of the rollout record, FUSED kernel, contiguous rows (no idx): requested early by all 256 threads as 16-byte
// pieces (policy net: actions | mean | log_std [64][6], adv, logp [64]; value net: vtarg, values [64]), parked in the dead input
// tile before the loss.  Read by the loss wave with per-sample loads behind the idx gather it was a dependent HBM round trip in
// the middle of the tile's chain (7.7 us of the launch in the timing-only ablation, profiles/r03_b_mlp_fused_ablation.json).
constexpr int kRecLdsFloats = 3 * kMlpBM * kMlpAct + 2 * kMlpBM;          // 1 280
template <int NT>
struct MlpRecordTile {
    static constexpr int kN = (320 + NT - 1) / NT;
    f32x4 v[kN];
    __device__ __forceinline__ static const float* piece(const float* const (&src)[5], int net, int j, long long row0, long long B, bool& ok)
    {
        // piece j of the tile: policy 0..95 actions, 96..191 mean, 192..287 log_std, 288..303 adv, 304..319 logp; value 0..15 vtarg, 16..31 values
        int arr, off;
        if (net == 0) { if (j < 288) { arr = j / 96; off = (j % 96) * 4; } else { arr = 3 + (j - 288) / 16; off = ((j - 288) % 16) * 4; } }
        else { arr = 3 + j / 16; off = (j % 16) * 4; }
        const long long per = (net == 0 && arr < 3) ? kMlpAct : 1;
        const long long e = row0 * per + off;                   // first element of the piece in its array
        ok = e + 3 < B * per;
        return src[arr] + e;
    }
    __device__ __forceinline__ void load(const float* const (&src)[5], int net, long long row0, long long B, int tid)
    {
        const int n = net == 0 ? 320 : 32;
#pragma unroll
        for (int i = 0; i < kN; ++i) {
            const int j = tid + NT * i;
            v[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            bool ok = false;
            if (j < n) {
                const float* p = piece(src, net, j, row0, B, ok);
                typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));      // a caller's slice may start on any float
                if (ok) v[i] = *reinterpret_cast<const f32x4u*>(p);
                else {                                          // the batch's last, partial tile: element by element
                    const long long per = (net == 0 && j < 288) ? kMlpAct : 1;
                    const long long e0 = p - src[net == 0 ? (j < 288 ? j / 96 : 3 + (j - 288) / 16) : 3 + j / 16];
#pragma unroll
                    for (int k = 0; k < 4; ++k) if (e0 + k < B * per) v[i][k] = p[k];
                }
            }
        }
    }
    __device__ __forceinline__ void park(float* lds, int net, int tid) const
    {
        const int n = net == 0 ? 320 : 32;
#pragma unroll
        for (int i = 0; i < kN; ++i) {
            const int j = tid + NT * i;
            if (j < n) *reinterpret_cast<f32x4*>(lds + (net == 0 ? 4 * j : 3 * kMlpBM * kMlpAct + 4 * j)) = v[i];
        }
    }
};

struct MlpFwdParams {
    const float* obs;          // [rows][137] float32 observations (raw when the filter vectors are given)
    const long long* idx;      // [B] row of `obs` for sample b (minibatch gather), or null: row b
    const __bf16* xs_in;       // [B][144] the nets' input ALREADY filtered and rounded (mlp_gather_kernel: an epoch's shuffle applied
                               // once), or null: stage 0 makes it from obs / idx / the filter vectors
    const float* f_loc;        // [137] MeanStdFilter vectors of PPOTrainer.filter.prepare(), or null (identity):
    const float* f_inv;        //   x = clamp((obs - loc) * inv, lo, hi)
    const float* f_lo;
    const float* f_hi;
    const __bf16* wpack;       // [2][kPackElems]
    const float* bias;         // [2][kBiasElems]
    float* head;               // [2][B][16] raw head outputs (float32)
    __bf16* xs;                // [B][144] the nets' input as they saw it (saved for dW1), or null
    __bf16* h1;                // [2][B][256] tanh activations (saved for the backward pass), or null
    __bf16* h2;                // [2][B][256]
    long long B;
    int first_net, n_nets;     // blockIdx.y + first_net = net
    // the sampler's action draw, fused into the layer-3 epilogue (all null in the learner): a = mean + exp(log_std) * noise
    // with log_std = clamp(raw, -20, 2) (RLlib DiagGaussian's sample(); SquashedGaussian is not the reference's choice),
    // the env's action = clamp(a, -a_max, a_max) when a_max is given (RLlib clip_actions, the reference's default)
    const float* noise;        // [B][6] standard-normal draws
    const float* a_max;        // [6] or null
    float* mean;               // [B][6]
    float* log_std;            // [B][6] clamped
    float* actions;            // [B][6] the sampled (unclipped) action: what the log-prob is taken of
    float* env_actions;        // [B][6] what pnr_step is given (may equal `actions` when a_max is null)
    float* values;             // [B] value head
    // FUSED instantiation (pnr_mlp_train_step): the loss and the backward-data pass of the same tile follow in the same
    // launch.  Rollout record as in PpoLossParams (rows gathered by idx); each net's workgroup differentiates its own
    // half of the loss (the policy and the value terms share nothing but the sample)
    const float* rec_actions; const float* rec_logp; const float* rec_mean; const float* rec_log_std;
    const float* rec_adv; const float* rec_vtarg; const float* rec_values;
    const float* kl_coeff; const float* ent_coeff;
    float clip, vf_clip, vf_coeff;
    float* g_head;             // [2][B][16] d loss / d head (float32; the weight-gradient kernel reads it)
    float* partials;           // [tiles * nets][8] per-workgroup sums: policy rows (-surr, 0, kl, entropy), value rows (0, vf)
    float* adam_step;          // the optimiser's update count (device scalar), incremented once per launch; or null
    __bf16* dz1;               // [2][B][256]
    __bf16* dz2;
    float* w3part;             // [tiles * nets][kW3PartFloats] layer 3's weight-gradient partials per tile (then h2 may be null), or null
    size_t act_plane;          // NS > 1: elements between two planes of h1 / h2 / dz1 / dz2 ([NS][2][B][256]: 2 B 256)
    size_t xs_plane;           // NS > 1: elements between two planes of xs_in
    float gscale;              // NS == 2: the power of two the gradient planes (G, dZ2, dZ1) are stored multiplied by (mlp_grad_scale); else 1
    unsigned long long* stamps; // PNR_MLP_STAMPS builds only: [workgroups][4 waves][kMlpStampSlots] cycle stamps, or null
};

constexpr int kFusedScratchFloats = kMlpBM * kMlpHead + kMlpBM * kGS / 2 + kRecLdsFloats + 4 * 8;     // head rows, head gradients, record, loss sums: 13 KB
static_assert(kFusedScratchFloats % 4 == 0 && kFusedScratchFloats * 4 <= kMlpBM * kXS * 2, "head rows, head gradients, record and loss sums fit the dead input tile");

// a 16x16x32 operand fragment whose k index is the SAMPLE: eight consecutive rows s0 + 8g .. +7 (g = lane >> 4) of column
// col0 + (lane & 15) of a row-major LDS tile, by two transposed 4x16 reads (cdna_hip_programming.md T10; wg_frag32 of
// pnr_mlp_wgrad.h is the 32x32x16 form and shares its pair of reads as wg_tr_pair; this one's stay written out: the fused kernel's listing)
__device__ __forceinline__ bf16x8 wg_frag16(const __bf16* tile, int tstride, int s0, int col0, int lane)
{
    const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
    const __bf16* a = tile + (s0 + 8 * g + q) * tstride + col0 + 4 * p;
    typedef s16x4 __attribute__((address_space(3))) * lds_p;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(a));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(a + 4 * tstride));
    // whole-vector bit cast: built element by element (f[j] = bit_cast<__bf16>(lo[j])), hipcc 7.2 replicated element 0
    // of each read into all four slots (v_perm_b32 0x05040100 of one register with itself) — found in the ISA after
    // every sample = 0 mod 4 came out weighted four times and the others not at all
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}


// ---- layer 3's weight gradients per TILE (r03h).  dW3 = G^T . H2 is the only consumer of H2 outside the tile that made it: 32 KB
// of every tile's 128 KB of activation stores, read back by the weight-gradient kernel together with a second copy of dZ2 (for
// db2) — 30 % of that kernel's bytes, and it runs at HBM / Infinity-Cache bandwidth (215 MB per 32 768-sample update in 35 us).
// The fused kernel has G, H2 and dZ2 in LDS anyway: each wave multiplies its own 32 feature columns (the columns only it
// overwrites) with 16x16x32 MFMAs and writes the tile's partials — dW3 [16][256] | db2 [256] | db3 [16] float32, 17 KB — and the
// weight-gradient kernel's third role just adds a slice's 16 partial rows in tile order.  Both forms define the slice sum the same way
// (per 64-sample tile a product chained over its two 32-sample k-steps from zero, the tiles added in order), so they agree bit for bit.
constexpr int kW3PartFloats = kMlpHead * kMlpHid + kMlpHid + kMlpHead;
template <bool HALF = false>
__device__ __forceinline__ bf16x8 bf16x8_ones()
{
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = HALF ? half_bits(1.0f) : (__bf16)1.0f;
    return o;
}
// dW3 (this wave's feature columns 32 w ..) and db3 (wave 0) of one 64-sample tile: G tile [64][16] bf16, H2 tile [64][256] bf16
// (NS planes each: gplane / hplane elements apart)
template <int NS = 1>
__device__ __forceinline__ void mlp_tile_w3_products(const __bf16* gtile, int gstride, const __bf16* htile, int hstride, int lane, int w,
                                                     f32x4 (&aw3)[2], f32x4& ab3, int gplane = 0, int hplane = 0)
{
    const bf16x8 ones = bf16x8_ones<Fmt<NS>::kHalf>();
    aw3[0] = (f32x4){0.f, 0.f, 0.f, 0.f}; aw3[1] = aw3[0]; ab3 = aw3[0];
#pragma unroll
    for (int ks = 0; ks < kMlpBM / 32; ++ks) {
        bf16x8 fg[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) fg[s] = wg_frag16(gtile + s * gplane, gstride, 32 * ks, 0, lane);            // A: rows = head entries
        if (w == 0) {
#pragma unroll
            for (int s = 0; s < NS; ++s) ab3 = mfma16<Fmt<NS>::kHalf>(fg[s], ones, ab3);
        }
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            bf16x8 fh[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) fh[s] = wg_frag16(htile + s * hplane, hstride, 32 * ks, 32 * w + 16 * b, lane);
#pragma unroll
            for (int pi = 0; pi < SplitPairs<NS>::n; ++pi)
                aw3[b] = mfma16<Fmt<NS>::kHalf>(fg[SplitPairs<NS>::a[pi]], fh[SplitPairs<NS>::b[pi]], aw3[b]);
        }
    }
}
// db2 (this wave's feature columns) of one tile: every row of 1^T . dZ2
template <int NS = 1>
__device__ __forceinline__ void mlp_tile_b2_products(const __bf16* ztile, int zstride, int lane, int w, f32x4 (&ab2)[2], int zplane = 0)
{
    const bf16x8 ones = bf16x8_ones<Fmt<NS>::kHalf>();
    ab2[0] = (f32x4){0.f, 0.f, 0.f, 0.f}; ab2[1] = ab2[0];
#pragma unroll
    for (int ks = 0; ks < kMlpBM / 32; ++ks)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const bf16x8 fz = wg_frag16(ztile + s * zplane, zstride, 32 * ks, 32 * w + 16 * b, lane);
                ab2[b] = mfma16<Fmt<NS>::kHalf>(ones, fz, ab2[b]);
            }
}

// The tile's loss on all 512 threads of the fused kernels: eight lanes per sample, lane d < 6 = action dimension d of the policy head
// (ppo_policy_sample's arithmetic, its sums over the dimensions as three xor-shuffles inside the group), lane 0 the value head
// (ppo_value_sample).  hd: the tile's head rows [64][16] float32, gt: its head gradients [64][kGS] bf16 (written here, with the
// float32 copy to g_head), rl: the parked record (rec_early) — all LDS; wsum [8 waves][4]: the waves' partial loss sums.
// As one thread per sample on wave 0 the other seven waves waited 4 300 cycles of a tile's 38 000 for it (profiles/r03_d_mlp_stamps.json).
// A second statement of ppo_policy_sample, so it has a checker of its own: tests/test_gpu_fused_loss.py holds g_head, the means and
// layer 3's bias gradient against a float64 reference sample by sample (clamp bounds, both clip sides, every record path, one-hot batches
// at the tile edges), as test_gpu_ppo.py::test_fused_loss_matches_autograd does for the stand-alone kernel.
// this thread's share of the tile's record, in registers (the compact layout of the fused kernel has no LDS to park it in): requested
// early — from inside the layer-2 product — by the thread that uses it: sample tid >> 3, action dimension tid & 7
struct MlpLossRec {
    float a, m0, l0, adv, lp0;           // policy: action, old mean, old log-std (d < 6), advantage, old log-prob; value: adv = vtarg, lp0 = old value
    __device__ __forceinline__ void load(const MlpFwdParams& P, int net, long long row0, int tid)
    {
        const int sl = tid >> 3, d = tid & 7;
        const long long b = row0 + sl;
        a = m0 = l0 = adv = lp0 = 0.f;
        if (b >= P.B) return;
        if (net == 0) {
            if (d < kMlpAct) { a = P.rec_actions[b * 6 + d]; m0 = P.rec_mean[b * 6 + d]; l0 = P.rec_log_std[b * 6 + d]; }
            adv = P.rec_adv[b]; lp0 = P.rec_logp[b];
        } else if (d == 0) { adv = P.rec_vtarg[b]; lp0 = P.rec_values[b]; }
    }
};

template <int NS = 1>
__device__ __forceinline__ void mlp_tile_loss(const MlpFwdParams& P, int net, long long row0, int tid, const float* hd, __bf16* gt, const float* rl,
                                              float* wsum, bool rec_early, int gplane = kTilePlane, bool rec_regs = false, MlpLossRec rv = MlpLossRec())
{
    // (rec_regs: the record comes in registers, by value — behind a pointer that may be null it was demoted to scratch)
    const MlpLossRec* rr = rec_regs ? &rv : nullptr;
    const int lane = tid & 63, w = tid >> 6;
    const int sl = tid >> 3, d = tid & 7;                     // sample of the tile, lane of its group
    const long long b = row0 + sl;
    const bool live = b < P.B && !(PNR_MLP_DIAG & 256);
    const float invB = 1.0f / (float)P.B;
    const long long r = (!rec_early && live && P.idx) ? P.idx[b] : b;
    float g0 = 0.f, g1 = 0.f;                                 // head-gradient entries d and 6 + d (lanes 6, 7: padding 12 + ..)
    float s_surr = 0.f, s_vf = 0.f, s_kl = 0.f, s_ent = 0.f;  // the sample's loss terms (meaningful on lane 0 of the group)
    if (net == 0) {
        const bool dim = d < kMlpAct;
        float m = 0.f, raw = 0.f, a = 0.f, m0 = 0.f, l0 = 0.f, adv = 0.f, lp0 = 0.f;
        if (live) {
            if (dim) { m = hd[sl * kMlpHead + d]; raw = hd[sl * kMlpHead + kMlpAct + d]; }
            if (rr) { a = rr->a; m0 = rr->m0; l0 = rr->l0; adv = rr->adv; lp0 = rr->lp0; }
            else if (rec_early) {
                if (dim) { a = rl[sl * 6 + d]; m0 = rl[384 + sl * 6 + d]; l0 = rl[768 + sl * 6 + d]; }
                adv = rl[1152 + sl]; lp0 = rl[1216 + sl];
            } else {
                if (dim) { a = P.rec_actions[r * 6 + d]; m0 = P.rec_mean[r * 6 + d]; l0 = P.rec_log_std[r * 6 + d]; }
                adv = P.rec_adv[r]; lp0 = P.rec_logp[r];
            }
        }
        const bool pass = raw >= -20.0f && raw <= 2.0f;           // torch.clamp passes the gradient on [min, max]
        const float ls = fminf(fmaxf(raw, -20.0f), 2.0f);
        const float si = expf(-ls);
        const float z = (a - m) * si;
        const float ivar = si * si;
        const float dm = m0 - m;
        const float q = (expf(2.0f * l0) + dm * dm) * ivar;        // (var0 + (m0 - m)^2) / var
        float lp = dim ? (-0.5f * z * z - ls) : 0.f;
        float kl = dim ? (ls - l0 + 0.5f * q - 0.5f) : 0.f;
        float en = dim ? ls : 0.f;
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) { lp += __shfl_xor(lp, o, 64); kl += __shfl_xor(kl, o, 64); en += __shfl_xor(en, o, 64); }
        const float logp = lp - 0.5f * 6.0f * 1.8378770664093453f;  // -3 log(2 pi)
        const float ent = en + 6.0f * 1.4189385332046727f;          // 6 * 0.5 log(2 pi e)
        const float ratio = expf(logp - lp0);
        const float rc = fminf(fmaxf(ratio, 1.0f - P.clip), 1.0f + P.clip);
        const float s1 = adv * ratio, s2 = adv * rc;
        const float surr = fminf(s1, s2);
        const bool inrange = ratio >= 1.0f - P.clip && ratio <= 1.0f + P.clip;
        // torch.minimum: the smaller argument takes the gradient, a tie splits it; the clipped branch is constant outside the range
        float dsurr;
        if (s1 < s2) dsurr = s1;
        else if (s1 == s2) dsurr = 0.5f * s1 + (inrange ? 0.5f * s1 : 0.f);
        else dsurr = inrange ? s1 : 0.f;
        const float klc = *P.kl_coeff, entc = *P.ent_coeff;
        if (live && dim) {
            g0 = (-dsurr * z * si + klc * (-dm * ivar)) * invB;
            g1 = pass ? (-dsurr * (z * z - 1.0f) + klc * (1.0f - q) - entc) * invB : 0.f;
        }
        if (live) { s_surr = -surr; s_kl = kl; s_ent = ent; }
    } else if (d == 0 && live) {
        const float vt = rr ? rr->adv : (rec_early ? rl[1152 + sl] : P.rec_vtarg[r]), v0 = rr ? rr->lp0 : (rec_early ? rl[1216 + sl] : P.rec_values[r]);
        float dvf;
        ppo_value_sample(hd[sl * kMlpHead], vt, v0, P.vf_clip, s_vf, dvf);
        g0 = P.vf_coeff * dvf * invB;
    }
    // head gradients: entries d and 6 + d of the sample's row (lanes 6, 7: the zero padding 12 .. 15), float32 for the
    // weight-gradient kernel, bf16 for this tile's backward products
    const int e0 = d < kMlpAct ? d : 12 + 2 * (d - 6), e1 = d < kMlpAct ? kMlpAct + d : 13 + 2 * (d - 6);
    if (b < P.B && P.g_head) {          // (null when nothing outside the tile reads it: layer 3's products are made by the tile itself)
        float* gp = P.g_head + ((size_t)net * P.B + b) * kMlpHead;
        gp[e0] = g0; gp[e1] = g1;
    }
    if constexpr (NS == 1) {
        gt[sl * kGS + e0] = (__bf16)g0;
        gt[sl * kGS + e1] = (__bf16)g1;
    } else {                              // the gradient rows as NS planes (plane s of the tile: + s * kTilePlane)
        __bf16 p0[NS], p1[NS];
        split_scalar<NS>(g0, p0, P.gscale); split_scalar<NS>(g1, p1, P.gscale);
#pragma unroll
        for (int s = 0; s < NS; ++s) { gt[s * gplane + sl * kGS + e0] = p0[s]; gt[s * gplane + sl * kGS + e1] = p1[s]; }
    }
    // the tile's sums: lane 0 of every group, then across the wave's eight samples; the waves' partial sums meet in LDS
    float sums[4] = {d == 0 ? s_surr : 0.f, d == 0 ? s_vf : 0.f, d == 0 ? s_kl : 0.f, d == 0 ? s_ent : 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float x = sums[k];
#pragma unroll
        for (int off = 8; off < 64; off <<= 1) x += __shfl_xor(x, off, 64);
        sums[k] = x;
    }
    if (lane == 0) *reinterpret_cast<f32x4*>(wsum + 4 * w) = (f32x4){sums[0], sums[1], sums[2], sums[3]};
}

// Forward pass of one 64-sample tile through one net: grid (ceil(B / 64), nets), 512 threads.
// FUSED: followed, in the same workgroup, by the tile's loss (all 512 threads, mlp_tile_loss) and its backward-data
// pass — the activations are written once (for the weight-gradient kernel) and never read back; H1 also stays in the
// registers of the lanes that made it, for the dZ1 epilogue.  One 256-column LDS tile serves H1, H2, dZ2 (in place over H2)
// and dZ1, the dead input tile holds the head rows, their gradients and the tile's record: 53 KB.
// NS: bf16 planes per operand (1: the bf16 path; 2, 3: split float32 operands, one workgroup per CU — the LDS tile exists NS times,
// plane s at + s * kTilePlane; the packed weights at + s * kWPlane; the saved tiles at plane stride P.act_plane)
// COMPACT (r05; the fused kernel with fp16 planes, NS = 2): TWO workgroups per CU, as the bf16 form has them.  One tile's chain leaves
// a CU idle at every barrier — stamps at one workgroup per CU: 57 500 cycles per tile of which 21 800 are products, 16 000 barrier waits
// (profiles/r05_c_mlp_stamps_f32_one_workgroup_per_cu.json) — and only a second resident tile fills that.  78 KB of LDS instead of 106:
// the input planes ALIAS the hidden planes (a barrier between layer 1's product and its epilogue), the head rows / head gradients /
// loss sums get 10 KB of their own, the tile's record waits in registers (MlpLossRec) instead of LDS; <= 128 registers: layer 1's
// activations are not kept for the dZ1 epilogue but read back from the H1 planes this workgroup stored (L2), the weight ring is 3 deep.
#ifndef PNR_MLP_COMPACT
#define PNR_MLP_COMPACT 1
#endif
#ifndef PNR_MLP_COMPACT_RING
#define PNR_MLP_COMPACT_RING 3
#endif
template <bool FUSED, int NS = 1>
__global__ __launch_bounds__(kFwdThreads, ((FUSED && NS == 1) || (NS == 2 && PNR_MLP_COMPACT)) ? 4 : 2) void mlp_forward_kernel(const MlpFwdParams P)
{
    constexpr bool kCompact = PNR_MLP_COMPACT && NS == 2;          // (the plain forward too: the sampler's pnr_mlp_act then runs its 512 (tile, net) units in one round)
    constexpr int XPL = kCompact ? kMlpBM * kXS : kTilePlane;          // plane strides (elements) of the input, hidden and head-gradient tiles
    constexpr int HPL = kCompact ? kMlpBM * kHS : kTilePlane;
    constexpr int GPL = kCompact ? kMlpBM * kGS : kTilePlane;
    constexpr int RING = kCompact ? PNR_MLP_COMPACT_RING : PNR_MLP_RING;
    constexpr int kScrElems = kMlpBM * kMlpHead * 2 + NS * kMlpBM * kGS + 2 * 4 * kFwdWaves;      // head rows (float32) | gradient planes | loss sums
    constexpr int kLdsElems = kCompact ? NS * kMlpBM * kHS + kScrElems : NS * kTilePlane + ((FUSED && NS == 1) ? PNR_MLP_LDS_PAD : 0);
    __shared__ __attribute__((aligned(16))) __bf16 lds[kLdsElems];
    static_assert(NS >= 1 && NS <= kMlpMaxPlanes && kLdsElems * 2 + (PNR_MLP_STAMPS ? 2048 : 0) <= 160 * 1024, "the planes' tiles fit one CU");
    static_assert(!kCompact || (2 * (kLdsElems * 2 + (PNR_MLP_STAMPS ? 2048 : 0)) <= 160 * 1024 && NS * kMlpBM * kXS <= NS * kMlpBM * kHS), "two compact workgroups per CU");
    MLP_STAMP_DECL;
    __bf16* xt = lds;
    __bf16* ht = kCompact ? lds : lds + kMlpBM * kXS;
    const long long row0 = (long long)blockIdx.x * kMlpBM;
    // the dead input tile: head rows, head gradients, record, loss sums (compact: a block of their own behind the hidden planes)
    float* const scr = kCompact ? reinterpret_cast<float*>(lds + NS * kMlpBM * kHS) : reinterpret_cast<float*>(xt);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane & 31, h = lane >> 5;
    // this wave owns row block w of a layer's [256 rows][64 samples] output, column blocks 0 and 1: its accumulators acc[cb]
    // a layer's bias pieces (mlp_bias_load) are requested in FRONT of the product's weight-fragment prefetch, so that they are the
    // older operations (vector-memory results return in order: asked for behind the fragments, as the accumulators' initial
    // values, each bias load made the compiler wait for vmcnt(0), draining the prefetch ring inside the product)
    typedef Fmt<NS> F;
    constexpr float kS1 = F::kSW * F::kSX, kS2 = F::kSW * F::kSH;     // scale of layer 1's / layer 2's and the head's accumulators
    const auto bias_init = [&](f32x16 (&acc)[kMlpCB], const f32x16& b) {       // (timing-only builds that skip a product)
#pragma unroll
        for (int cb = 0; cb < kMlpCB; ++cb) acc[cb] = b;
    };
    const int yi = (int)blockIdx.y;                               // index of this (tile, net) unit among the tile's units
    const int net = yi + P.first_net;
    [[maybe_unused]] const int stamp_yi_ = yi, stamp_ny_ = (int)gridDim.y;
    const __bf16* wp = P.wpack + (size_t)net * kPackElems;
    const float* bias = P.bias + net * kBiasElems;
    // layer 1's bias and first weight fragments do not depend on the tile: requested before anything else
    MLP_STAMP(0);
    f32x4 bq1[4];
    mlp_bias_load(bias, w, h, bq1);
    __builtin_amdgcn_sched_barrier(0);
    MlpGemm1<kMlpInPad, kXS, NS, XPL, RING> g1;
    g1.prefetch(wp + kOffW1 + w * (kMlpInPad / 16) * 512, lane);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (FUSED) {       // this launch is one optimiser update: counted here, read by the Adam kernel two launches on
        if (blockIdx.x == 0 && yi == 0 && tid == 0 && P.adam_step) *P.adam_step += 1.0f;
    }

    // ---- stage 0: the tile's observations, filtered, as bf16 [BM][144] (columns 137.. zero)
    {
        float* fv = kCompact ? scr : reinterpret_cast<float*>(ht);   // loc | inv | lo | hi, 4 x 144 floats, in the idle tile (compact: the scratch block)
        static_assert(4 * kMlpInPad * 2 <= kScrElems, "the filter vectors fit the scratch block");
        if (P.xs_in) {                                            // the tile's 64 rows are 18 KB of contiguous bf16: a plain copy,
            // every load of the thread in flight before the first LDS write
            constexpr int kCh = kMlpBM * (kMlpInPad / 8), kIt = (kCh + kFwdThreads - 1) / kFwdThreads;
            uint4 v[NS][kIt];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
            const __bf16* xin = P.xs_in + (size_t)s * P.xs_plane;               // plane s of the pre-gathered rows
            if (row0 + kMlpBM <= P.B) {            // a whole tile: 18 KB contiguous — thread offset + constant per piece, one uniform test
                const __bf16* base = xin + row0 * kMlpInPad + tid * 8;
#pragma unroll
                for (int i = 0; i < kIt; ++i) {
                    v[s][i] = make_uint4(0u, 0u, 0u, 0u);
                    if (i < kCh / kFwdThreads || tid + kFwdThreads * i < kCh) v[s][i] = *reinterpret_cast<const uint4*>(base + (size_t)i * kFwdThreads * 8);
                }
            } else {
#pragma unroll
                for (int i = 0; i < kIt; ++i) {
                    const int ch = tid + kFwdThreads * i, row = ch / (kMlpInPad / 8), cc = ch % (kMlpInPad / 8);
                    v[s][i] = make_uint4(0u, 0u, 0u, 0u);
                    if (ch < kCh && row0 + row < P.B) v[s][i] = *reinterpret_cast<const uint4*>(xin + (row0 + row) * kMlpInPad + cc * 8);
                }
            }
            }
#pragma unroll
            for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int i = 0; i < kIt; ++i) {
                const int ch = tid + kFwdThreads * i, row = ch / (kMlpInPad / 8), cc = ch % (kMlpInPad / 8);
                if (ch < kCh) *reinterpret_cast<uint4*>(xt + s * XPL + row * kXS + cc * 8) = v[s][i];
            }
        } else {
        if (P.f_loc) {
            for (int i = tid; i < 4 * kMlpInPad; i += kFwdThreads) {
                const int which = i / kMlpInPad, k = i % kMlpInPad;
                const float* src = which == 0 ? P.f_loc : (which == 1 ? P.f_inv : (which == 2 ? P.f_lo : P.f_hi));
                fv[i] = k < kMlpIn ? src[k] : 0.f;
            }
        }
        mlp_barrier();
        // eight threads per row, 18 columns each: every load of the thread (a row starts on a 4-byte boundary only) is issued
        // before the first use.  Written as a loop over (row, column pair) with one dependent idx -> row load per iteration this
        // stage was a chain of ~36 memory round trips per thread: 35.8 us of a 16 384-sample launch (rocprof r02_b).
        {
            constexpr int TPR = kFwdThreads / kMlpBM;             // threads per row: 8
            constexpr int CPT = kMlpInPad / TPR;                  // 18 columns: four 16-byte loads + one 8-byte load
            static_assert(CPT == 18, "stage 0 is written for 18 columns per thread");
            const int row = tid / TPR, part = tid % TPR;
            const long long b = row0 + row;
            const bool live = b < P.B;
            const float* src = P.obs + (live ? (P.idx ? P.idx[b] : b) : 0) * kMlpIn + CPT * part;
            typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
            typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));
            float x[20];
#pragma unroll
            for (int j = 0; j < 20; ++j) x[j] = 0.f;
            if (live && !(PNR_MLP_DIAG & 2)) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int col = CPT * part + 4 * j;
                    if (col + 3 < kMlpIn) { const f32x4 v = *reinterpret_cast<const f32x4u*>(src + 4 * j); x[4 * j] = v[0]; x[4 * j + 1] = v[1]; x[4 * j + 2] = v[2]; x[4 * j + 3] = v[3]; }
                    else {
#pragma unroll
                        for (int k = 0; k < 4; ++k) if (col + k < kMlpIn) x[4 * j + k] = src[4 * j + k];
                    }
                }
                const int col = CPT * part + 16;
                if (col + 1 < kMlpIn) { const f32x2u v = *reinterpret_cast<const f32x2u*>(src + 16); x[16] = v[0]; x[17] = v[1]; }
                else if (col < kMlpIn) x[16] = src[16];
            }
#pragma unroll
            for (int j = 0; j < CPT; ++j) {
                const int col = CPT * part + j;
                float y = x[j];
                if (P.f_loc) y = mlp_filter_col(y, fv, col);
                x[j] = (live && col < kMlpIn) ? y : 0.f;
            }
            // 18 bf16 = 36 bytes per thread, 4-byte aligned in the tile: nine dword stores (per plane: the residual goes on)
#pragma unroll
            for (int j = 0; j < CPT; j += 2) {
                typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
                __bf16 p0[NS], p1[NS];
                split_scalar<NS>(x[j], p0, F::kSX); split_scalar<NS>(x[j + 1], p1, F::kSX);
#pragma unroll
                for (int s = 0; s < NS; ++s) *reinterpret_cast<bf16x2*>(xt + s * XPL + row * kXS + CPT * part + j) = (bf16x2){p0[s], p1[s]};
            }
        }
        }
        mlp_barrier();
        if (P.xs && net == 0) {                                   // the input is the same for both nets: saved once
            for (int ch = tid; ch < kMlpBM * (kMlpInPad / 8); ch += kFwdThreads) {
                const int row = ch / (kMlpInPad / 8), cc = ch % (kMlpInPad / 8);
                if (row0 + row < P.B)
                    *reinterpret_cast<uint4*>(P.xs + (row0 + row) * kMlpInPad + cc * 8) = *reinterpret_cast<const uint4*>(xt + row * kXS + cc * 8);
            }
        }
    }

    MLP_STAMP(1);                         // stage 0 done (tile in LDS, barrier passed)
    f32x16 acc[kMlpCB];
    // tanh in registers (the bias is what the accumulators started from), each register quad = four consecutive features
    // of one sample -> one ds_write_b64
    // FUSED: layer 1's activations additionally STAY in this lane's registers (32 bf16 = 16 registers: exactly the values the
    // dZ1 epilogue multiplies its own accumulators with), instead of coming back from L2 behind a vmcnt(0), two barriers and an
    // LDS round trip (3 500 of a tile's 44 000 cycles in the phase stamps)
    bf16x4 h1keep[(FUSED && NS == 1) ? kMlpCB * 4 : 1];
    f32x4 h1keep_f[(FUSED && NS > 1 && !kCompact) ? kMlpCB * 4 : 1];        // NS > 1: the float32 values themselves (what the planes add up to)
    const auto epilogue = [&](bool keep, [[maybe_unused]] float inv_scale) {
#pragma unroll
        for (int cb = 0; cb < kMlpCB; ++cb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if constexpr (NS == 1) {
                bf16x4 pk;
                if (PNR_MLP_DIAG & 1) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) pk[j] = (__bf16)acc[cb][4 * q + j];
                } else {
                    pk = tanh_quad(acc[cb], q);
                }
                *reinterpret_cast<bf16x4*>(ht + (32 * cb + c) * kHS + 32 * w + 8 * q + 4 * h) = pk;
                if constexpr (FUSED) { if (keep) h1keep[4 * cb + q] = pk; }
                } else {
                    f32x2 z0 = {acc[cb][4 * q], acc[cb][4 * q + 1]}, z1 = {acc[cb][4 * q + 2], acc[cb][4 * q + 3]};
                    if constexpr (F::kHalf) { z0 *= inv_scale; z1 *= inv_scale; }        // exact: a power of two
                    const f32x2 lo = tanh_fast2(z0), hi = tanh_fast2(z1);
                    const float t[4] = {lo[0], lo[1], hi[0], hi[1]};
                    bf16x4_t pk[NS];
                    split_quad<NS>(t, pk, F::kSH);
#pragma unroll
                    for (int s = 0; s < NS; ++s) *reinterpret_cast<bf16x4*>(ht + s * HPL + (32 * cb + c) * kHS + 32 * w + 8 * q + 4 * h) = pk[s];
                    if constexpr (FUSED && !kCompact) { if (keep) h1keep_f[4 * cb + q] = (f32x4){t[0], t[1], t[2], t[3]}; }
                }
            }
    };
    // a [BM][256] tile's NS planes to global rows (plane s of a saved tensor: + s * P.act_plane elements)
    const auto store_planes = [&](__bf16* dst) {
#pragma unroll
        for (int s = 0; s < NS; ++s)
            mlp_store_htile_nt<kFwdThreads>(ht + s * HPL, dst + (size_t)s * P.act_plane + (size_t)net * P.B * kMlpHid, row0, P.B, tid);
    };

    // ---- layer 1: H1^T = tanh(W1 . X^T + b1)
    {
        // (a one-element array filled by a loop, on purpose: as a plain variable hipcc 7.2 orders two zero moves of stage 0's xs_in copy
        // the other way round in the plain forward kernel, whose listing is compared with its last tuned one instruction for instruction.
        // The last trace of the two-row-block layout: make it a plain variable when the listing is next re-baselined)
        f32x16 b16[1];
#pragma unroll
        for (int r = 0; r < 1; ++r) b16[r] = mlp_bias16<F::kHalf>(bq1, kS1);
        if (PNR_MLP_DIAG & 8) bias_init(acc, b16[0]);
        else g1.run(xt, acc, lane, [] {}, &b16[0]);
    }
    if constexpr (kCompact) mlp_barrier();      // H1 is written over the input planes: every wave is done reading them
    MLP_STAMP(2);                         // layer-1 product issued
    if (!(PNR_MLP_DIAG & 32)) epilogue(true, 1.f / kS1);
    MLP_STAMP(3);                         // layer-1 epilogue
    // layer 2's bias and first weight fragments are requested ahead of the barrier (and of the tile store behind it)
    f32x4 bq2[4];
    mlp_bias_load(bias + kMlpHid, w, h, bq2);
    __builtin_amdgcn_sched_barrier(0);
    MlpGemm1<kMlpHid, kHS, NS, HPL, RING> g2;
    g2.prefetch(wp + kOffW2 + w * (kMlpHid / 16) * 512, lane);
    __builtin_amdgcn_sched_barrier(0);
    mlp_barrier();
    MLP_STAMP(4);                         // barrier after the layer-1 epilogue
    MLP_STAMP(5);

    // ---- layer 2: H2^T = tanh(W2 . H1^T + b2); the tile is overwritten once every wave has read it.  The H1 tile leaves for
    // HBM from INSIDE the product, behind its last weight-fragment load, and the tile's record is requested there too
    const f32x16 b16_2 = mlp_bias16<F::kHalf>(bq2, kS2);
    if (PNR_MLP_DIAG & 4) bias_init(acc, b16_2);
    MlpRecordTile<kCompact ? 100000 : kFwdThreads> rect;      // (compact: unused, no registers)
    MlpLossRec lrec;
    const bool rec_early = FUSED && !P.idx && !(PNR_MLP_DIAG & 256);
    const auto l2_hook = [&] {
        if constexpr (kCompact) {
            if (rec_early) lrec.load(P, net, row0, tid);
        } else if constexpr (FUSED) {
            if (rec_early) {
                // policy: actions, mean, log_std, adv, logp; value: -, -, -, vtarg, values
                const float* const src[5] = {P.rec_actions, P.rec_mean, P.rec_log_std, net == 0 ? P.rec_adv : P.rec_vtarg, net == 0 ? P.rec_logp : P.rec_values};
                rect.load(src, net, row0, P.B, tid);
            }
        }
        if (P.h1 && !(PNR_MLP_DIAG & 64)) store_planes(P.h1);
    };
    if (!(PNR_MLP_DIAG & 4)) {
        g2.run(ht, acc, lane, l2_hook, &b16_2);
    }
    if constexpr (FUSED && !kCompact) {      // the input tile is dead since the barrier above: the record waits there, behind the head rows and gradients
        if (rec_early) rect.park(scr + kMlpBM * kMlpHead + kMlpBM * kGS / 2, net, tid);
    }
    MLP_STAMP(6);                         // layer-2 product issued
    mlp_barrier();
    MLP_STAMP(7);
    if (!(PNR_MLP_DIAG & 32)) epilogue(false, 1.f / kS2);
    MLP_STAMP(8);                         // layer-2 epilogue
    mlp_barrier();
    MLP_STAMP(9);
    MLP_STAMP(10);

    // ---- layer 3: head^T [16][samples] = W3 . H2^T + b3 with 16x16x32 MFMAs; waves 0-3 own 16 samples each (waves 4-7 go on to
    // the H2 store)
    if (!(PNR_MLP_DIAG & 16) && w < 4) {
        const int r16 = lane & 15, g = lane >> 4;
        f32x4 a3 = *reinterpret_cast<const f32x4*>(bias + 2 * kMlpHid + 4 * g);    // rows 4g .. 4g+3: the accumulators' start
        if constexpr (F::kHalf) a3 *= kS2;
        const __bf16* w3 = wp + kOffW3 + lane * 8;                    // fragment-native: block ks at ks * 512
        bf16x8 w3f[kMlpHid / 32][NS];
#pragma unroll
        for (int ks = 0; ks < kMlpHid / 32; ++ks)
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                w3f[ks][s] = ld_global_bf16x8(w3 + s * kWPlane + 512 * ks);
            }
#pragma unroll
        for (int ks = 0; ks < kMlpHid / 32; ++ks) {
            bf16x8 b[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) b[s] = *reinterpret_cast<const bf16x8*>(ht + s * HPL + (16 * w + r16) * kHS + 32 * ks + 8 * g);
#pragma unroll
            for (int pi = 0; pi < SplitPairs<NS>::n; ++pi)
                a3 = mfma16<F::kHalf>(w3f[ks][SplitPairs<NS>::a[pi]], b[SplitPairs<NS>::b[pi]], a3);
        }
        if constexpr (F::kHalf) a3 *= 1.f / kS2;
        {
            const long long b = row0 + 16 * w + r16;                  // column = sample, rows 4g .. 4g+3 = head entries
            const f32x4 hq = a3;
            if (b < P.B && P.head) *reinterpret_cast<f32x4*>(P.head + ((size_t)net * P.B + b) * kMlpHead + 4 * g) = hq;
            if constexpr (FUSED) {                                    // head rows of the tile, float32 [64][16], in the dead input tile
                *reinterpret_cast<f32x4*>(scr + (16 * w + r16) * kMlpHead + 4 * g) = hq;
            } else if (P.noise) {
                if (net == 1) {
                    if (b < P.B && g == 0) P.values[b] = hq[0];
                } else {
                    // policy rows: g = 0 holds means 0..3, g = 1 means 4, 5 and raw log-stds 0, 1, g = 2 raw log-stds 2..5.
                    // Six cross-lane reads put each mean next to its log-std (executed by all lanes: no divergence around them).
                    const auto ls = [](float x) { return fminf(fmaxf(x, -20.f), 2.f); };
                    const float l0 = ls(__shfl(hq[2], r16 + 16)), l1 = ls(__shfl(hq[3], r16 + 16));
                    const float l2 = ls(__shfl(hq[0], r16 + 32)), l3 = ls(__shfl(hq[1], r16 + 32));
                    const float l4 = ls(__shfl(hq[2], r16 + 32)), l5 = ls(__shfl(hq[3], r16 + 32));
                    if (b < P.B && g <= 2) {
                        const size_t o = (size_t)b * kMlpAct;
                        typedef float f32x2 __attribute__((ext_vector_type(2)));
                        const auto st2 = [](float* dst, float x, float y) { *reinterpret_cast<f32x2*>(dst) = (f32x2){x, y}; };
                        const auto draw = [&](int j, float m, float l, float& a, float& e) {
                            a = fmaf(expf(l), P.noise[o + j], m);
                            e = P.a_max ? fminf(fmaxf(a, -P.a_max[j]), P.a_max[j]) : a;
                        };
                        if (g == 0) {
                            float a[4], e[4];
                            draw(0, hq[0], l0, a[0], e[0]); draw(1, hq[1], l1, a[1], e[1]);
                            draw(2, hq[2], l2, a[2], e[2]); draw(3, hq[3], l3, a[3], e[3]);
                            st2(P.mean + o, hq[0], hq[1]); st2(P.mean + o + 2, hq[2], hq[3]);
                            st2(P.actions + o, a[0], a[1]); st2(P.actions + o + 2, a[2], a[3]);
                            if (P.env_actions != P.actions) { st2(P.env_actions + o, e[0], e[1]); st2(P.env_actions + o + 2, e[2], e[3]); }
                        } else if (g == 1) {
                            float a[2], e[2];
                            draw(4, hq[0], l4, a[0], e[0]); draw(5, hq[1], l5, a[1], e[1]);
                            st2(P.mean + o + 4, hq[0], hq[1]);
                            st2(P.actions + o + 4, a[0], a[1]);
                            if (P.env_actions != P.actions) st2(P.env_actions + o + 4, e[0], e[1]);
                            st2(P.log_std + o, ls(hq[2]), ls(hq[3]));
                        } else {
                            st2(P.log_std + o + 2, ls(hq[0]), ls(hq[1])); st2(P.log_std + o + 4, ls(hq[2]), ls(hq[3]));
                        }
                    }
                }
            }
        }
    }
    MLP_STAMP(11);                        // head product + its stores

    if constexpr (!FUSED) {
        if (P.h2 && !(PNR_MLP_DIAG & 64)) store_planes(P.h2);
    }
    if constexpr (FUSED) {
        float* hd = scr;                                                  // [64][16] float32 head rows (written above)
        __bf16* gt = reinterpret_cast<__bf16*>(scr) + kMlpBM * kMlpHead * 2;    // [64][kGS] bf16 head gradients, behind them
        const float* rl = scr + kMlpBM * kMlpHead + kMlpBM * kGS / 2;     // the parked record (compact: none, MlpLossRec)
        float* wsum = kCompact ? scr + kMlpBM * kMlpHead + NS * kMlpBM * kGS / 2      // [8 waves][4] loss sums
                               : scr + kMlpBM * kMlpHead + kMlpBM * kGS / 2 + kRecLdsFloats;
        // W3^T's fragment for the first backward product: requested before the H2 store and the loss
        bf16x8 w3t[NS];                                                  // [plane]
#pragma unroll
        for (int s = 0; s < NS; ++s) w3t[s] = ld_global_bf16x8(wp + s * kWPlane + kOffW3T + w * 512 + lane * 8);
        __builtin_amdgcn_sched_barrier(0);
        if (P.h2 && !(PNR_MLP_DIAG & 64)) store_planes(P.h2);      // (null: layer 3's gradients are made here, below)
        mlp_barrier();
        MLP_STAMP(12);                    // barrier before the loss
        // ---- the tile's loss on all 512 threads (mlp_tile_loss)
        mlp_tile_loss<NS>(P, net, row0, tid, hd, gt, rl, wsum, rec_early, GPL, kCompact && rec_early, lrec);
        MLP_STAMP(13);                    // loss done
        mlp_barrier();
        MLP_STAMP(14);                    // barrier after the loss
        if (tid == 0) {                   // the eight waves' sums in wave order: one row of partial sums per workgroup
            f32x4 t = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < kFwdWaves; ++k) t += *reinterpret_cast<const f32x4*>(wsum + 4 * k);
            float* pr = P.partials + ((size_t)blockIdx.x * P.n_nets + yi) * 8;
            *reinterpret_cast<f32x4*>(pr) = t;
            *reinterpret_cast<f32x4*>(pr + 4) = (f32x4){0.f, 0.f, 0.f, 0.f};
        }

        // acc * (1 - h^2) with h read from the tile at this lane's own quads and the product written over it
        // acc * (1 - h^2) of quad q with h the float32 values hf, as NS planes into the tile at this lane's quads
        const auto dtanh_split = [&](int cb, int q, const f32x4& hf) {
            float d[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = (F::kHalf ? acc[cb][4 * q + j] * (1.f / F::kSW) : acc[cb][4 * q + j]) * __builtin_fmaf(-hf[j], hf[j], 1.0f);
            bf16x4_t pk[NS];
            split_quad<NS>(d, pk);               // (fp16 planes: d is the gradient times gscale already; the split clamps)
#pragma unroll
            for (int s = 0; s < NS; ++s) *reinterpret_cast<bf16x4*>(ht + s * HPL + (32 * cb + c) * kHS + 32 * w + 8 * q + 4 * h) = pk[s];
        };
        const auto bwd_epilogue = [&]() {
#pragma unroll
            for (int cb = 0; cb < kMlpCB; ++cb)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    __bf16* at = ht + (32 * cb + c) * kHS + 32 * w + 8 * q + 4 * h;
                    if constexpr (NS == 1) {
                    const bf16x4 hv = *reinterpret_cast<const bf16x4*>(at);
                    *reinterpret_cast<bf16x4*>(at) = dtanh_quad(acc[cb], q, hv);
                    } else {
                        bf16x4_t hv[NS];                                          // the planes add up to the activation (bf16 planes: exactly)
#pragma unroll
                        for (int s = 0; s < NS; ++s) hv[s] = *reinterpret_cast<const bf16x4*>(at + s * HPL);
                        dtanh_split(cb, q, planes_value<NS>(hv, 1.f / F::kSH));
                    }
                }
        };
        // ---- layer 3's weight-gradient partials of this tile (dW3 = G^T . H2, db3 = G^T . 1), while H2 is still in the tile: this wave's
        // 32 feature columns are the ones only it overwrites below
        float* w3p = P.w3part ? P.w3part + ((size_t)blockIdx.x * P.n_nets + yi) * kW3PartFloats : nullptr;
        [[maybe_unused]] const float inv_g = 1.f / P.gscale;       // (a power of two: exact)
        if (w3p) {
            f32x4 aw3[2], ab3;
            mlp_tile_w3_products<NS>(gt, kGS, ht, kHS, lane, w, aw3, ab3, GPL, HPL);
            const int c16 = lane & 15, g = lane >> 4;              // C: col = lane & 15, rows 4g .. 4g+3
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int j = 0; j < 4; ++j) w3p[(4 * g + j) * kMlpHid + 32 * w + 16 * b + c16] = F::kHalf ? aw3[b][j] * (inv_g * (1.f / F::kSH)) : aw3[b][j];
            if (w == 0 && c16 == 0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) w3p[kMlpHead * kMlpHid + kMlpHid + 4 * g + j] = F::kHalf ? ab3[j] * inv_g : ab3[j];     // every column of G^T . 1 is db3
            }
        }
        // ---- dH2^T = W3^T . G^T (one k-step of 16; the padded head rows are zero), dZ2 in place over H2
        mlp_zero_acc(acc);
        {
            bf16x8 b[NS][kMlpCB];
#pragma unroll
            for (int s = 0; s < NS; ++s)
#pragma unroll
                for (int cb = 0; cb < kMlpCB; ++cb) b[s][cb] = *reinterpret_cast<const bf16x8*>(gt + s * GPL + (32 * cb + c) * kGS + 8 * h);
#pragma unroll
            for (int pi = 0; pi < SplitPairs<NS>::n; ++pi)
#pragma unroll
                for (int cb = 0; cb < kMlpCB; ++cb)
                    acc[cb] = mfma32<F::kHalf>(w3t[SplitPairs<NS>::a[pi]], b[SplitPairs<NS>::b[pi]][cb], acc[cb]);
        }
        bwd_epilogue();
        const auto b2_products = [&] {                             // db2 = 1^T . dZ2 of this wave's columns 32 w .., now that they hold dZ2
            if (w3p) {
                f32x4 ab2[2];
                mlp_tile_b2_products<NS>(ht, kHS, lane, w, ab2, HPL);
                if ((lane >> 4) == 0) {
#pragma unroll
                    for (int b = 0; b < 2; ++b) w3p[kMlpHead * kMlpHid + 32 * w + 16 * b + (lane & 15)] = F::kHalf ? ab2[b][0] * inv_g : ab2[b][0];
                }
            }
        };
        b2_products();                                             // (only this wave wrote these columns)
        MLP_STAMP(15);                    // dH2 product + its epilogue
        MlpGemm1<kMlpHid, kHS, NS, HPL, RING> g4;    // W2^T's first fragments ahead of the barrier
        g4.prefetch(wp + kOffW2T + w * (kMlpHid / 16) * 512, lane);
        __builtin_amdgcn_sched_barrier(0);
        mlp_barrier();
        MLP_STAMP(16);                    // barrier after it

        // ---- dH1^T = W2^T . dZ2^T (the dZ2 tile leaves from inside the product), then H1 into the tile and dZ1 in place over it
        mlp_zero_acc(acc);
        const auto dz2_hook = [&] { if (!(PNR_MLP_DIAG & 64)) store_planes(P.dz2); };
        g4.run(ht, acc, lane, dz2_hook);
        MLP_STAMP(17);                    // dZ2 store + W2^T product issued
        // compact: layer 1's activations, this lane's quads, back from the H1 planes this workgroup stored during layer 2's product (the
        // stores have completed: every wave has since waited for later loads of its own, vector-memory operations complete in order,
        // and barriers followed) — requested here, consumed behind the barrier
        bf16x4 h1back[kCompact ? kMlpCB * 4 : 1][kCompact ? NS : 1];
        if constexpr (kCompact) {
#pragma unroll
            for (int cb = 0; cb < kMlpCB; ++cb) {
                const long long row = row0 + 32 * cb + c;
                const __bf16* src = P.h1 + ((size_t)net * P.B + (row < P.B ? row : 0)) * kMlpHid + 32 * w + 4 * h;
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int s = 0; s < NS; ++s) h1back[4 * cb + q][s] = *reinterpret_cast<const bf16x4*>(src + (size_t)s * P.act_plane + 8 * q);
            }
        }
        MLP_STAMP(18);
        mlp_barrier();                         // every read of dZ2 (the product and the store inside it) is done: the tile is free
        MLP_STAMP(19);
        MLP_STAMP(20);
        // dZ1 = dH1 * (1 - H1^2) with H1 from this lane's own registers, written into the free tile for the coalesced store
#pragma unroll
        for (int cb = 0; cb < kMlpCB; ++cb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if constexpr (NS == 1) *reinterpret_cast<bf16x4*>(ht + (32 * cb + c) * kHS + 32 * w + 8 * q + 4 * h) = dtanh_quad(acc[cb], q, h1keep[4 * cb + q]);
                else if constexpr (kCompact) dtanh_split(cb, q, planes_value<NS>(h1back[4 * cb + q], 1.f / F::kSH));
                else dtanh_split(cb, q, h1keep_f[4 * cb + q]);
            }
        MLP_STAMP(21);
        mlp_barrier();
        if (!(PNR_MLP_DIAG & 64)) store_planes(P.dz1);
        MLP_STAMP(22);                    // end
        MLP_STAMP_FLUSH;
    }
}

}  // namespace pnr
#pragma clang fp contract(off)
