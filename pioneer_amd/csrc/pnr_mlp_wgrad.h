// pnr_mlp_wgrad.h — the weight gradients: mlp_wgrad_kernel<NS> (per batch slice into that slice's slab) with its chunk staging,
// direct-to-LDS ring and transposing stores (wg_*, Wg*), and the two kernels that sum the slabs in slice order
// (mlp_reduce_kernel, mlp_reduce_flat_kernel).
#pragma once

#include "pnr_mlp.h"
#include "pnr_mlp_forward.h"      // the per-tile layer-3 products and their layout (kW3PartFloats)
#pragma clang fp contract(fast)      // as in pnr_mlp.h: the TU is compiled -ffp-contract=off for the env integrator
namespace pnr {

// ---------------------------------------------------------------------------------------------------------------
// weight gradients: dW = dZ^T . H over the samples of one batch slice, written to that slice's slab.
// grid (slices, 4 parts, nets): part 0 / 1 = the two 128-column halves of dW2, part 2 = dW1 and db1 (the input tile
// carries a column of ones at k = 144), part 3 = dW3, db3 and db2 (16x16x32 MFMAs, a fragment of ones).  One workgroup
// per CU.  (What was tried and dropped here in r02 / r03 — more roles, two chunks in flight, register-staged chunks: DESIGN_HISTORY.md.)
// ---------------------------------------------------------------------------------------------------------------
struct MlpWgradParams {
    const float* g_head;       // [2][B][16]
    const __bf16* xs;          // [B][144]
    const __bf16* h1;          // [2][B][256]
    const __bf16* h2;
    const __bf16* dz1;
    const __bf16* dz2;
    float* slabs;              // [slices][2][kGradElems]
    long long B;
    long long slice_rows;      // samples per slice, a multiple of kWgChunk
    int first_net;             // blockIdx.z + first_net = net
    const float* w3part;       // [tiles * n_nets][kW3PartFloats] the fused kernel's per-tile layer-3 partials (then h2 is not read), or null
    int n_nets;                // nets of the launch that wrote w3part (its row index is tile * n_nets + blockIdx.z)
    unsigned long long* stamps; // PNR_MLP_STAMPS builds only (tools/wgrad_stamps.py): [nets][roles][slices][8 waves][kMlpStampSlots], or null
    size_t act_plane;          // NS > 1: elements between two planes of h1 / dz1 / dz2
    size_t xs_plane;           // .. and of xs
    float gscale;              // NS == 2: what the gradient planes are stored multiplied by (MlpFwdParams::gscale); else 1
};
#if PNR_MLP_STAMPS
#define WG_STAMP(i) do { if (P.stamps && lane == 0) { unsigned long long* sp_ = P.stamps + ((((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 8 + w) * kMlpStampSlots; \
    sp_[(i)] = __builtin_amdgcn_s_memtime(); if ((i) == 0) sp_[24] = __builtin_amdgcn_s_memrealtime(); if ((i) == 22) sp_[25] = __builtin_amdgcn_s_memrealtime(); } } while (0)
#else
#define WG_STAMP(i) do { } while (0)
#endif

// A 64-row chunk of COLS bf16 columns (a multiple of 8) on its way from row-major global memory (row stride src_stride)
// into an LDS tile: loaded into registers first (every load of the chunk in flight together), written later — the
// weight-gradient loop requests chunk c + 1 before it multiplies chunk c.
// (eight waves per workgroup: two per SIMD — with the four of r02 every MFMA chain, LDS read and chunk hand-over of a workgroup
// was exposed on a SIMD that had nothing else to run)
constexpr int kWgThreads = 512;
template <int COLS>
struct WgChunk {
    static constexpr int kPieces = kWgChunk * (COLS / 8);
    static constexpr int kPerThread = (kPieces + kWgThreads - 1) / kWgThreads;
    static constexpr int kFull = kPieces / kWgThreads;             // iterations in which every thread has a piece
    uint4 v[kPerThread];
    // A WHOLE chunk (the common case: slices are multiples of 64 rows, only the batch's last chunk can be short) is requested with no
    // per-thread test and one per-thread offset that does not depend on the chunk: uniform base + thread offset + constant.  Written
    // with a bounds test, a zero fill and a 64-bit row * stride per piece, requesting a chunk's nine pieces cost ~1 000 of its
    // 3 150 cycles in address arithmetic alone (tools/wgrad_stamps.py, r03i).
    __device__ __forceinline__ void load(const __bf16* __restrict__ src, long long src_stride, long long row0, long long n_rows, int tid)
    {
        constexpr int cpr = COLS / 8;
        if (row0 + kWgChunk <= n_rows) {                            // uniform
            const __bf16* base = src + row0 * src_stride;
            const unsigned off = (unsigned)(tid / cpr) * (unsigned)src_stride + (unsigned)(tid % cpr) * 8u;
            const unsigned step = (unsigned)(kWgThreads / cpr) * (unsigned)src_stride;
#pragma unroll
            for (int i = 0; i < kPerThread; ++i) {
                if constexpr (kWgThreads % cpr == 0) {
                    // rows advance by kWgThreads / cpr per iteration, the column piece stays
                    if (i < kFull || tid < kPieces - kFull * kWgThreads) v[i] = *reinterpret_cast<const uint4*>(base + off + (size_t)i * step);
                    else v[i] = make_uint4(0u, 0u, 0u, 0u);
                } else {
                    const int ch = tid + kWgThreads * i, row = ch / cpr, cc = ch % cpr;
                    if (i < kFull || ch < kPieces) v[i] = *reinterpret_cast<const uint4*>(base + (unsigned)row * (unsigned)src_stride + (unsigned)cc * 8u);
                    else v[i] = make_uint4(0u, 0u, 0u, 0u);
                }
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < kPerThread; ++i) {
            const int ch = tid + kWgThreads * i, row = ch / cpr, cc = ch % cpr;
            v[i] = make_uint4(0u, 0u, 0u, 0u);
            if (ch < kWgChunk * cpr && row0 + row < n_rows) v[i] = *reinterpret_cast<const uint4*>(src + (row0 + row) * src_stride + cc * 8);
        }
    }
    __device__ __forceinline__ void store(__bf16* tile, int tstride, int tid) const
    {
        constexpr int cpr = COLS / 8;
#pragma unroll
        for (int i = 0; i < kPerThread; ++i) {
            const int ch = tid + kWgThreads * i, row = ch / cpr, cc = ch % cpr;
            if (ch < kWgChunk * cpr) *reinterpret_cast<uint4*>(tile + row * tstride + cc * 8) = v[i];
        }
    }
};

// two transposed 4x16 reads (ds_read_b64_tr_b16) at a and hi_a, four tile rows further on, as one 8-element MFMA operand fragment
// (put together by a whole-vector bit cast: wg_frag16 says why)
__device__ __forceinline__ bf16x8 wg_tr_pair(const void* a, const void* hi_a)
{
    typedef s16x4 __attribute__((address_space(3))) * lds_p;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(a));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(hi_a));
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}
// a 32x32x16 operand fragment whose k index is the SAMPLE: eight consecutive rows s0 + 8h .. +7 of column
// col0 + (lane & 31) of a row-major tile, by two transposed 4x16 reads (cdna_hip_programming.md T10)
__device__ __forceinline__ bf16x8 wg_frag32(const __bf16* tile, int tstride, int s0, int col0, int lane)
{
    const int G = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
    const __bf16* a = tile + (s0 + 8 * (G >> 1) + q) * tstride + col0 + 16 * (G & 1) + 4 * p;
    return wg_tr_pair(a, a + 4 * tstride);
}
#define PNR_SLAB_STORE(p, v) __builtin_nontemporal_store((v), (p))      // slabs are written once and read by another kernel: streaming stores
// store a 32x32 accumulator block to a row-major float32 matrix: rows row0.., cols col0.. (cols < ncols kept)
__device__ __forceinline__ void wg_store_block(float* __restrict__ m, int ld, int row0, int col0, int ncols, const f32x16& a, int lane)
{
    const int c = lane & 31, h = lane >> 5;
    if (col0 + c < ncols) {
#pragma unroll
        for (int i = 0; i < 16; ++i) PNR_SLAB_STORE(m + (size_t)(row0 + (i & 3) + 8 * (i >> 2) + 4 * h) * ld + col0 + c, a[i]);
    }
}


// ---------------------------------------------------------------------------------------------------------------
// r04: the hot roles of the weight-gradient kernel (dW2 halves; dW1 halves) stage their chunks with DIRECT-TO-LDS loads
// (global_load_lds_dwordx4, "glds": 1 KiB per wave-instruction, no VGPR destination, no ds_write pass) into a THREE-stage ring,
// one raw barrier per chunk and counted s_waitcnt vmcnt(N): chunk c + 2 is requested at the start of chunk c's products and has two
// chunks of MFMAs to arrive, where the register-staged form of r03 (bit-identical; git history) had one chunk of prefetch, two
// barriers and a VGPR -> LDS write pass per chunk: 3 150 cycles per 64-sample chunk for 16 MFMAs per wave (1 024 cycles of matrix
// pipe per SIMD), the same for every chunk (profiles/r03_i_wgrad_stamps.json) — a workgroup alone on its CU has nothing else to run
// while it waits (cdna_hip_programming.md section 5, "Pipelining across barriers": the regime where the 3-buffer span pays).
// A glds writes LDS lane-linearly (wave-uniform base + 16 lane), so the conflict-free image for the transposed reads cannot be
// made by padding rows: it is an XOR swizzle applied on the SOURCE address and again on the read (16-byte piece j of row r sits
// at piece j ^ 4 (r & 3): the four rows a ds_read_b64_tr_b16 half-wave touches land in four different 64-byte bank groups).
// X rows are 288 bytes (32 mod 256): stored as they are, the four rows overlap pairwise in the banks (2-way conflict on the
// B-operand reads of the dW1 roles, ~2 of 32 cycles per MFMA gap); db1 comes from a fragment of ones in registers instead of a
// column of ones in the tile.  The products, their k order and the chunk order are those of the register-staged form: same bits.
// ---------------------------------------------------------------------------------------------------------------
// the ring's geometry by the number of operand planes (NS > 1: float32-accurate split operands): chunks of 64 samples and three
// stages for bf16; 32-sample chunks for split operands (a stage holds every plane's tiles), three stages with two planes, two with three
template <int NS> struct WgGeom {
    static constexpr int CH = NS == 1 ? 64 : 32;                        // samples per chunk
    static constexpr int KS = CH / 16;                                  // k-steps per chunk
    static constexpr int STAGES = NS <= 2 ? 3 : 2;
    static constexpr int kPlane2 = CH * 512 + CH * 256;                 // dW2 roles, one plane: dZ2 [CH][256] | H1 half [CH][128], bf16
    static constexpr int kPlane1 = CH * 256 + CH * 288;                 // dW1 roles, one plane: dZ1 half [CH][128] | X [CH][144]
    static constexpr int kStage2 = NS * kPlane2, kStage1 = NS * kPlane1;
    static constexpr int kRing = STAGES * kStage2 + 64;                 // (+ slack: the last X block reads 32 bytes past its row)
    static constexpr int nA2 = CH / 16, nB2 = CH / 32;                  // a wave's pieces per plane and chunk: dZ2, H1 half
    static constexpr int nA1 = CH / 32, kXPieces = CH * 288 / 1024;     // dZ1 half; X pieces of the whole workgroup (18 or 9)
};
constexpr int kWgRingBytes = WgGeom<1>::kRing > WgGeom<2>::kRing ? (WgGeom<1>::kRing > WgGeom<3>::kRing ? WgGeom<1>::kRing : WgGeom<3>::kRing)
                                                                 : (WgGeom<2>::kRing > WgGeom<3>::kRing ? WgGeom<2>::kRing : WgGeom<3>::kRing);
static_assert(kWgRingBytes <= 150 * 1024, "the ring fits one CU beside the stamps");
constexpr int kWgLdsBytesOld = (kWgChunk * kTrH + kWgChunk * kTrH + kWgChunk * kTrG) * 2;
constexpr int kWgLdsBytes = kWgRingBytes > kWgLdsBytesOld ? kWgRingBytes : kWgLdsBytesOld;

// one direct-to-LDS piece: lane l's 16 bytes at sbase + voff land at LDS byte address lds_dst + 16 l (lds_dst, sbase wave-uniform).
// M0 carries the LDS base and is compiler-reserved: written and restored in the same statement (cdna_hip_programming.md, inline asm)
__device__ __forceinline__ void wg_glds16(unsigned voff, const void* sbase, unsigned lds_dst)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(lds_dst), "s"(sbase) : "memory");
}
template <int N> __device__ __forceinline__ void wg_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }
__device__ __forceinline__ const void* wg_uniform_ptr(const void* p)
{
    const unsigned long long b = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    return (const void*)(((unsigned long long)hi << 32) | lo);
}
// LDS byte address of a __shared__ pointer
__device__ __forceinline__ unsigned wg_lds_addr(const void* p)
{
    typedef char __attribute__((address_space(3))) * lds_c;
    return (unsigned)(unsigned long long)(lds_c)(p);
}
// the fragment of wg_frag32 from a SWIZZLED tile (rows of ROWB bytes, 16-byte piece j of row r at piece j ^ 4 (r & 3)); s0 a multiple of 16
template <int ROWB>
__device__ __forceinline__ bf16x8 wg_frag32_swz(const char* tile, int s0, int col0, int lane)
{
    const int G = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
    const int row = s0 + 8 * (G >> 1) + q;                      // row & 3 == q, and so for row + 4
    const int cb = (col0 + 16 * (G & 1) + 4 * p) * 2;           // byte of the column inside the row
    const char* a = tile + row * ROWB + (cb ^ (q << 6));
    return wg_tr_pair(a, a + 4 * ROWB);
}
// .. and from a LINEAR tile with rows of ROWB bytes
template <int ROWB>
__device__ __forceinline__ bf16x8 wg_frag32_lin(const char* tile, int s0, int col0, int lane)
{
    const int G = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
    const char* a = tile + (s0 + 8 * (G >> 1) + q) * ROWB + (col0 + 16 * (G & 1) + 4 * p) * 2;
    return wg_tr_pair(a, a + 4 * ROWB);
}
// a swizzled tile's piece i (1 KiB of LDS = 1024 / ROWB rows): the source byte offset of lane `lane` relative to the chunk's first row
// (global rows GROWB bytes apart, the tile's columns starting at byte col_off of a row)
template <int ROWB>
__device__ __forceinline__ unsigned wg_piece_src_swz(int i, int lane, int GROWB, int col_off, int& row)
{
    constexpr int kLanesPerRow = ROWB / 16;
    row = i * (1024 / ROWB) + lane / kLanesPerRow;
    const int jp = lane % kLanesPerRow;
    return (unsigned)(row * GROWB + col_off + ((jp ^ (4 * (row & 3))) << 4));
}

// The ring's schedule, shared by both roles.  NP = this wave's glds instructions per chunk.  Per chunk c:
//   wait until chunk c's pieces of THIS wave have landed (counted: chunk c + 1's may stay in flight) -> barrier (every wave's pieces
//   landed; every wave is done reading chunk c - 1) -> request chunk c + 2 into the stage chunk c - 1 used -> multiply chunk c.
// A chunk that is not whole (only the batch's last one can be) is staged by plain loads and ds_write into the same image, zeros
// for the rows past the end, at the place its glds would have been issued.
#if PNR_MLP_STAMPS
// (diagnostic build) phase stamps of the ring, parked in LDS and flushed at the kernel's end: a stamp written to global memory would be
// one more operation on the VM counter that the ring's counted waits are written against
#define WG_RING_STAMP(i) do { if (stamps && (threadIdx.x & 63) == 0) stamps[(i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define WG_RING_STAMP(i) do { } while (0)
#endif
template <int CH, int STAGES, int MAXP, class ISSUE, class SYNC, class MUL, class PRO>
__device__ __forceinline__ void wg_ring_loop(long long s_begin, long long s_end, int np, ISSUE&& issue, SYNC&& stage_sync, MUL&& multiply,
                                             PRO&& prologue_work, unsigned long long* stamps = nullptr)
{
    constexpr int D = STAGES - 1;                                     // chunks requested ahead of the one being multiplied
    const int nch = (int)((s_end - s_begin + CH - 1) / CH);
    const auto whole = [&](int c) { return s_begin + (long long)(c + 1) * CH <= s_end; };
    const auto request = [&](int c, int stage) {
        if (whole(c)) {
#pragma unroll
            for (int k = 0; k < MAXP; ++k) issue(c, stage, k);
        } else stage_sync(c, stage);
    };
#pragma unroll
    for (int c = 0; c < D; ++c)
        if (c < nch) request(c, c);
    // `late_work` (the requests of the layer-3 partial sums: sixteen 16-byte loads of a few threads, consumed after the accumulators'
    // stores) is issued at the top of the LAST chunk's products.  In front of the loop — even behind the first chunks' pieces — its 16
    // vector-memory instructions per wave queued up with the 12 pieces and the loop started 5 500 cycles later (8 250 against 2 750
    // cycles from the kernel's start, profiles/r04_b_wgrad_ring_stamps.json); no counted wait follows the last chunk's, so nothing
    // waits for these loads but their use.
    bool late_done = false;
    int stage = 0;
    WG_RING_STAMP(1);
    for (int c = 0; c < nch; ++c) {
        // glds of this wave that may stay in flight: those of the chunks c + 1 .. c + D - 1 (requested by glds; none with two stages)
        const int ahead = (D > 1 && c + 1 < nch && whole(c + 1)) ? np : 0;
        if (c >= 4 && c < 8) WG_RING_STAMP(2 + 4 * (c - 4));          // top of the chunk
        if (ahead == 0) wg_wait_vm<0>();
        else if (ahead == 4) wg_wait_vm<4>();
        else if (ahead == 5) wg_wait_vm<5>();
        else if (ahead == 6) wg_wait_vm<6>();
        else wg_wait_vm<0>();
        if (c >= 4 && c < 8) WG_RING_STAMP(3 + 4 * (c - 4));          // its pieces landed
        mlp_barrier();
        if (c >= 4 && c < 8) WG_RING_STAMP(4 + 4 * (c - 4));          // barrier passed
        const int nstage = stage == 0 ? STAGES - 1 : stage - 1;       // the stage chunk c - 1 used: every wave is done with it
        const bool glds_next = c + D < nch && whole(c + D);
        if (c + D < nch && !glds_next) stage_sync(c + D, nstage);
        if (c >= 4 && c < 8) WG_RING_STAMP(5 + 4 * (c - 4));
        if (c == nch - 1) { prologue_work(); late_done = true; }
        // chunk c + D's pieces are requested from INSIDE the products, a few behind each k-step's MFMAs: issuing the six
        // of them in one go cost 650 cycles per chunk in which the wave issued no MFMA (profiles/r04_a_wgrad_ring_stamps_issue_in_one_go.json)
        multiply(stage, [&](int k) { if (glds_next) issue(c + D, nstage, k); });
        stage = stage == STAGES - 1 ? 0 : stage + 1;
    }
    if (!late_done) prologue_work();
    WG_RING_STAMP(20);
}

// A wave's 32x32 accumulator block to a row-major float32 matrix through a wave-private LDS tile: 16-byte stores, eight lanes per
// 128-byte row segment (wg_store_block's one dword per lane cost ~96 cycles of issue per instruction: 6 000 cycles per dW2 wave).
constexpr int kWgTrS = 36;                                       // floats per row of the transposing tile (144 B: 16-byte aligned)
// (unscale: the power of two the accumulators are multiplied by on their way out — fp16 planes; 1 otherwise)
__device__ __forceinline__ void wg_store_block_lds(float* scratch, float* __restrict__ m, int ld, int row0, int col0, int ncols, const f32x16& a, int lane,
                                                   float unscale = 1.f)
{
    const int c = lane & 31, h = lane >> 5;
#pragma unroll
    for (int i = 0; i < 16; ++i) scratch[((i & 3) + 8 * (i >> 2) + 4 * h) * kWgTrS + c] = a[i] * unscale;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");           // wave-private tile: the wave's own DS operations complete in order
    const int r = lane >> 3, q = lane & 7;
#pragma unroll
    for (int pss = 0; pss < 4; ++pss) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(scratch + (r + 8 * pss) * kWgTrS + 4 * q);
        if (col0 + 4 * q < ncols) {
            f32x4* dst = reinterpret_cast<f32x4*>(m + (size_t)(row0 + r + 8 * pss) * ld + col0 + 4 * q);
            __builtin_nontemporal_store(v, dst);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");           // the reads are done before the next block overwrites the tile
}

// The fused kernel's per-tile layer-3 products of this slice (dW3 | db2 | db3, kW3PartFloats per tile), added in tile order: part `part`
// of `parts` takes that share of the elements, a thread ONE quad of them.  Two steps: the (at most 16) tiles' 16-byte pieces are
// REQUESTED before the ring starts and ADDED after it — one memory round trip (2-4 us under load) for a handful of threads, which as
// a serial step cost the whole workgroup that time wherever it stood (profiles/r04_b_wgrad_ring_stamps.json: 8 000 cycles in front of
// the loop, 7 400 behind it); now it travels under the products.
struct WgW3Sums {
    static constexpr int kTiles = 16;
    f32x4 x[kTiles];
    int q;                    // this thread's quad, or -1
    long long extra0, t1;     // tiles beyond the first 16 (none at the loop's slice size): added synchronously in finish()
    const float* pp; size_t stride;
    __device__ __forceinline__ void request(const MlpWgradParams& P, long long s_begin, long long s_end, int part, int parts, int tid)
    {
        const int quads = kW3PartFloats / 4 / parts;              // 273 with four parts: one per thread
        q = tid < quads ? part * quads + tid : -1;
        const long long t0 = s_begin / kWgChunk;
        t1 = (s_end + kWgChunk - 1) / kWgChunk;
        stride = (size_t)P.n_nets * kW3PartFloats;
        pp = P.w3part + ((size_t)t0 * P.n_nets + blockIdx.z) * kW3PartFloats + 4 * (q < 0 ? 0 : q);
        extra0 = t0 + kTiles;
#pragma unroll
        for (int j = 0; j < kTiles; ++j) x[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (q < 0) return;
        if (t0 + kTiles <= t1) {                                  // the usual case, one uniform test: sixteen requests back to back (written
            // with a test per tile, hipcc branched around every load and made the first one wait for its data before the next was issued)
            const float* a = pp;
#pragma unroll
            for (int j = 0; j < kTiles; ++j) { x[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a)); a += stride; }
        } else {
#pragma unroll
            for (int j = 0; j < kTiles; ++j)
                if (t0 + j < t1) x[j] = *reinterpret_cast<const f32x4*>(pp + (size_t)j * stride);
        }
    }
    __device__ __forceinline__ void finish(float* slab) const
    {
        if (q < 0) return;
        f32x4 sum = {0.f, 0.f, 0.f, 0.f};
        const long long t0 = extra0 - kTiles;
#pragma unroll
        for (int j = 0; j < kTiles; ++j) if (t0 + j < t1) sum += x[j];
        for (long long t = extra0; t < t1; ++t) sum += *reinterpret_cast<const f32x4*>(pp + (size_t)(t - t0) * stride);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = 4 * q + j;
            slab[e < kMlpHead * kMlpHid ? kGW3 + e : (e < kMlpHead * kMlpHid + kMlpHid ? kGB2 + (e - kMlpHead * kMlpHid) : kGB3 + (e - kMlpHead * kMlpHid - kMlpHid))] = sum[j];
        }
    }
};
static_assert(kW3PartFloats / 4 / kWgParts <= kWgThreads && kW3PartFloats % (4 * kWgParts) == 0, "one quad of the layer-3 partials per thread and role");

// dW2[:, 128 part .. +128] = dZ2^T . H1[:, that half] of one slice; waves 4 x 2, each 64 (o) x 64 (i)
template <int NS>
__device__ __forceinline__ void wgrad_dw2_glds(const MlpWgradParams& P, char* ring, int part, size_t nb, long long s_begin, long long s_end,
                                               float* slab, int tid, unsigned long long* stamps = nullptr)
{
    typedef WgGeom<NS> G;
    constexpr int CH = G::CH, NPP = G::nA2 + G::nB2, MAXP = NS * NPP;   // pieces per plane / per chunk of one wave
    const int lane = tid & 63, w = tid >> 6;
    const int wo = w >> 1, wi = w & 1;
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;
    // this wave's pieces of a chunk and plane: A (dZ2, pieces of two 512-byte rows) w, w + 8, ..; B (H1 half, pieces of four 256-byte
    // rows) w, ..  The per-lane source offsets depend on neither the chunk nor the plane.
    unsigned offA[G::nA2], offB[G::nB2];
    int rowA[G::nA2], rowB[G::nB2];
#pragma unroll
    for (int k = 0; k < G::nA2; ++k) offA[k] = wg_piece_src_swz<512>(w + 8 * k, lane, kMlpHid * 2, 0, rowA[k]);
#pragma unroll
    for (int k = 0; k < G::nB2; ++k) offB[k] = wg_piece_src_swz<256>(w + 8 * k, lane, kMlpHid * 2, 256 * part, rowB[k]);
    const char* gA = reinterpret_cast<const char*>(P.dz2 + nb);
    const char* gB = reinterpret_cast<const char*>(P.h1 + nb);
    const size_t plane_b = P.act_plane * 2;                          // bytes between two planes of a saved tensor
    const unsigned ring_addr = __builtin_amdgcn_readfirstlane(wg_lds_addr(ring));
    // piece k of this wave's MAXP of chunk c into stage `stage`: plane k / NPP, then A pieces, then B pieces
    const auto issue = [&](int c, int stage, int k) {
        const long long s = s_begin + (long long)c * CH;
        const int pl = k / NPP, r = k % NPP;
        const unsigned dst = __builtin_amdgcn_readfirstlane(ring_addr + stage * G::kStage2 + pl * G::kPlane2 + w * 1024);
        if (r < G::nA2) wg_glds16(offA[r], wg_uniform_ptr(gA + pl * plane_b + s * (kMlpHid * 2)), dst + r * 8192);
        else wg_glds16(offB[r - G::nA2], wg_uniform_ptr(gB + pl * plane_b + s * (kMlpHid * 2)), dst + CH * 512 + (r - G::nA2) * 8192);
    };
    const auto stage_sync = [&](int c, int stage) {
        const long long s = s_begin + (long long)c * CH;
#pragma unroll
        for (int pl = 0; pl < NS; ++pl) {
            char* dst = ring + stage * G::kStage2 + pl * G::kPlane2 + w * 1024 + lane * 16;
#pragma unroll
            for (int k = 0; k < G::nA2; ++k) {
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (s + rowA[k] < s_end) v = *reinterpret_cast<const uint4*>(gA + pl * plane_b + s * (kMlpHid * 2) + offA[k]);
                *reinterpret_cast<uint4*>(dst + k * 8192) = v;
            }
#pragma unroll
            for (int k = 0; k < G::nB2; ++k) {
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (s + rowB[k] < s_end) v = *reinterpret_cast<const uint4*>(gB + pl * plane_b + s * (kMlpHid * 2) + offB[k]);
                *reinterpret_cast<uint4*>(dst + CH * 512 + k * 8192) = v;
            }
        }
    };
    const auto multiply = [&](int stage, auto&& piece) {
        const char* ta = ring + stage * G::kStage2;
        const char* tb = ta + CH * 512;
        if constexpr (NS == 1) {
            bf16x8 fa[2][2], fb[2][2];
#pragma unroll
            for (int a = 0; a < 2; ++a) fa[0][a] = wg_frag32_swz<512>(ta, 0, 64 * wo + 32 * a, lane);
#pragma unroll
            for (int b = 0; b < 2; ++b) fb[0][b] = wg_frag32_swz<256>(tb, 0, 64 * wi + 32 * b, lane);
#pragma unroll
            for (int ks = 0; ks < G::KS; ++ks) {
                if (ks + 1 < G::KS) {
#pragma unroll
                    for (int a = 0; a < 2; ++a) fa[(ks + 1) & 1][a] = wg_frag32_swz<512>(ta, 16 * (ks + 1), 64 * wo + 32 * a, lane);
#pragma unroll
                    for (int b = 0; b < 2; ++b) fb[(ks + 1) & 1][b] = wg_frag32_swz<256>(tb, 16 * (ks + 1), 64 * wi + 32 * b, lane);
                }
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        acc[a][b] = mfma32<false>(fa[ks & 1][a], fb[ks & 1][b], acc[a][b]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = ks; k < MAXP; k += G::KS) piece(k);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < G::KS; ++ks) {
                bf16x8 fa[NS][2], fb[NS][2];
#pragma unroll
                for (int pl = 0; pl < NS; ++pl) {
#pragma unroll
                    for (int a = 0; a < 2; ++a) fa[pl][a] = wg_frag32_swz<512>(ta + pl * G::kPlane2, 16 * ks, 64 * wo + 32 * a, lane);
#pragma unroll
                    for (int b = 0; b < 2; ++b) fb[pl][b] = wg_frag32_swz<256>(tb + pl * G::kPlane2, 16 * ks, 64 * wi + 32 * b, lane);
                }
#pragma unroll
                for (int pi = 0; pi < SplitPairs<NS>::n; ++pi)
#pragma unroll
                    for (int a = 0; a < 2; ++a)
#pragma unroll
                        for (int b = 0; b < 2; ++b)
                            acc[a][b] = mfma32<Fmt<NS>::kHalf>(fa[SplitPairs<NS>::a[pi]][a], fb[SplitPairs<NS>::b[pi]][b], acc[a][b]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = ks; k < MAXP; k += G::KS) piece(k);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    WgW3Sums w3;
    w3.q = -1;
    wg_ring_loop<CH, G::STAGES, MAXP>(s_begin, s_end, MAXP, issue, stage_sync, multiply,
                                      [&] { if (P.w3part) w3.request(P, s_begin, s_end, part, kWgParts, tid); }, stamps);
    mlp_barrier();                                               // every wave is done with the ring: its memory carries the stores' tiles
    float* scratch = reinterpret_cast<float*>(ring) + w * (32 * kWgTrS);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
            wg_store_block_lds(scratch, slab + kGW2, kMlpHid, 64 * wo + 32 * a, 128 * part + 64 * wi + 32 * b, kMlpHid, acc[a][b], lane,
                               Fmt<NS>::kHalf ? 1.f / (P.gscale * Fmt<NS>::kSH) : 1.f);
    if (P.w3part) w3.finish(slab);                               // (behind the accumulators' stores: its loads have had that long to arrive)
}

// dW1[128 half .. +128, :] = dZ1[:, that half]^T . X and db1 of one slice; waves 4 (row blocks) x 2 (column groups: X blocks 0-2 | blocks
// 3-4 and db1 from a fragment of ones).  Every element's products are accumulated in the order of the register-staged form.
template <int NS>
__device__ __forceinline__ void wgrad_dw1_glds(const MlpWgradParams& P, char* ring, int half, size_t nb, long long s_begin, long long s_end,
                                               float* slab, int tid, unsigned long long* stamps = nullptr)
{
    typedef WgGeom<NS> G;
    constexpr int CH = G::CH, NXMAX = (G::kXPieces + 7) / 8, NPP = G::nA1 + NXMAX, MAXP = NS * NPP;
    const int lane = tid & 63, w = tid >> 6;
    const int rb = w & 3, cg = w >> 2;
    f32x16 acc[3];
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[b][i] = 0.f;
    // pieces per plane: A (dZ1 half, pieces of four 256-byte rows) w, ..; X (CH rows of 288 bytes, copied as they lie) w, w + 8, ..
    // below kXPieces (some waves have one piece less)
    unsigned offA[G::nA1];
    int rowA[G::nA1];
#pragma unroll
    for (int k = 0; k < G::nA1; ++k) offA[k] = wg_piece_src_swz<256>(w + 8 * k, lane, kMlpHid * 2, 256 * half, rowA[k]);
    const int nx = (G::kXPieces - w + 7) / 8;
    const char* gA = reinterpret_cast<const char*>(P.dz1 + nb);
    const char* gX = reinterpret_cast<const char*>(P.xs);
    const size_t plane_b = P.act_plane * 2, xplane_b = P.xs_plane * 2;
    const unsigned ring_addr = __builtin_amdgcn_readfirstlane(wg_lds_addr(ring));
    const auto issue = [&](int c, int stage, int k) {
        const long long s = s_begin + (long long)c * CH;
        const int pl = k / NPP, r = k % NPP;
        const unsigned dst = __builtin_amdgcn_readfirstlane(ring_addr + stage * G::kStage1 + pl * G::kPlane1 + w * 1024);
        if (r < G::nA1) wg_glds16(offA[r], wg_uniform_ptr(gA + pl * plane_b + s * (kMlpHid * 2)), dst + r * 8192);
        else if (r - G::nA1 < nx)
            wg_glds16((unsigned)((w + 8 * (r - G::nA1)) * 1024 + lane * 16), wg_uniform_ptr(gX + pl * xplane_b + s * (kMlpInPad * 2)), dst + CH * 256 + (r - G::nA1) * 8192);
    };
    const auto stage_sync = [&](int c, int stage) {
        const long long s = s_begin + (long long)c * CH;
#pragma unroll
        for (int pl = 0; pl < NS; ++pl) {
            char* dst = ring + stage * G::kStage1 + pl * G::kPlane1 + w * 1024 + lane * 16;
#pragma unroll
            for (int k = 0; k < G::nA1; ++k) {
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (s + rowA[k] < s_end) v = *reinterpret_cast<const uint4*>(gA + pl * plane_b + s * (kMlpHid * 2) + offA[k]);
                *reinterpret_cast<uint4*>(dst + k * 8192) = v;
            }
#pragma unroll
            for (int k = 0; k < NXMAX; ++k) {
                if (k < nx) {
                    const int o = (w + 8 * k) * 1024 + lane * 16;
                    uint4 v = make_uint4(0u, 0u, 0u, 0u);
                    if (s + o / (kMlpInPad * 2) < s_end) v = *reinterpret_cast<const uint4*>(gX + pl * xplane_b + s * (kMlpInPad * 2) + o);
                    *reinterpret_cast<uint4*>(dst + CH * 256 + k * 8192) = v;
                }
            }
        }
    };
    const bf16x8 ones = bf16x8_ones<Fmt<NS>::kHalf>();
    const auto multiply = [&](int stage, auto&& piece) {
        const char* ta = ring + stage * G::kStage1;
        const char* tb = ta + CH * 256;
#pragma unroll
        for (int ks = 0; ks < G::KS; ++ks) {
            bf16x8 fa[NS];
#pragma unroll
            for (int pl = 0; pl < NS; ++pl) fa[pl] = wg_frag32_swz<256>(ta + pl * G::kPlane1, 16 * ks, 32 * rb, lane);
            if (cg == 0) {
                bf16x8 fb[NS][3];
#pragma unroll
                for (int pl = 0; pl < NS; ++pl)
#pragma unroll
                    for (int b = 0; b < 3; ++b) fb[pl][b] = wg_frag32_lin<kMlpInPad * 2>(tb + pl * G::kPlane1, 16 * ks, 32 * b, lane);
#pragma unroll
                for (int pi = 0; pi < SplitPairs<NS>::n; ++pi)
#pragma unroll
                    for (int b = 0; b < 3; ++b) acc[b] = mfma32<Fmt<NS>::kHalf>(fa[SplitPairs<NS>::a[pi]], fb[SplitPairs<NS>::b[pi]][b], acc[b]);
            } else {
                bf16x8 fb[NS][2];
#pragma unroll
                for (int pl = 0; pl < NS; ++pl)
#pragma unroll
                    for (int b = 0; b < 2; ++b) fb[pl][b] = wg_frag32_lin<kMlpInPad * 2>(tb + pl * G::kPlane1, 16 * ks, 32 * (3 + b), lane);
#pragma unroll
                for (int pi = 0; pi < SplitPairs<NS>::n; ++pi)
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[b] = mfma32<Fmt<NS>::kHalf>(fa[SplitPairs<NS>::a[pi]], fb[SplitPairs<NS>::b[pi]][b], acc[b]);
#pragma unroll
                for (int pl = 0; pl < NS; ++pl)
                    acc[2] = mfma32<Fmt<NS>::kHalf>(fa[pl], ones, acc[2]);      // every column: db1 of this wave's rows
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = ks; k < MAXP; k += G::KS) piece(k);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    WgW3Sums w3;
    // (np differs by wave — some have one X piece less per plane — wave-uniform)
    wg_ring_loop<CH, G::STAGES, MAXP>(s_begin, s_end, NS * (G::nA1 + nx), issue, stage_sync, multiply,
                                      [&] { w3.request(P, s_begin, s_end, 2 + half, kWgParts, tid); }, stamps);
    mlp_barrier();
    float* scratch = reinterpret_cast<float*>(ring) + w * (32 * kWgTrS);
    const int row0 = 128 * half + 32 * rb;
    const float inv_g = 1.f / P.gscale, un1 = Fmt<NS>::kHalf ? inv_g * (1.f / Fmt<NS>::kSX) : 1.f;      // (powers of two: exact)
    if (cg == 0) {
#pragma unroll
        for (int b = 0; b < 3; ++b) wg_store_block_lds(scratch, slab + kGW1, kMlpInPad, row0, 32 * b, kMlpInPad, acc[b], lane, un1);
    } else {
#pragma unroll
        for (int b = 0; b < 2; ++b) wg_store_block_lds(scratch, slab + kGW1, kMlpInPad, row0, 32 * (3 + b), kMlpInPad, acc[b], lane, un1);
        if ((lane & 31) == 0) {
            const int hh = lane >> 5;
#pragma unroll
            for (int i = 0; i < 16; ++i) slab[kGB1 + row0 + (i & 3) + 8 * (i >> 2) + 4 * hh] = Fmt<NS>::kHalf ? acc[2][i] * inv_g : acc[2][i];
        }
    }
    w3.finish(slab);
}

template <int NS = 1>
__global__ __launch_bounds__(kWgThreads) void mlp_wgrad_kernel(const MlpWgradParams P)
{
    __shared__ __attribute__((aligned(1024))) char lds_raw[kWgLdsBytes];
    __bf16* lds = reinterpret_cast<__bf16*>(lds_raw);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int slice = blockIdx.x, part = blockIdx.y, net = blockIdx.z + P.first_net;
    const long long s_begin = (long long)slice * P.slice_rows;
    long long s_end = s_begin + P.slice_rows;
    if (s_end > P.B) s_end = P.B;
    float* slab = P.slabs + ((size_t)slice * kMlpNets + net) * kGradElems;
    const size_t nb = (size_t)net * P.B * kMlpHid;

#if PNR_MLP_STAMPS
    __shared__ unsigned long long wg_stamp_lds[8][kMlpStampSlots];
    unsigned long long* my_stamps = P.stamps ? wg_stamp_lds[w] : nullptr;
    if (my_stamps && lane < kMlpStampSlots) my_stamps[lane] = 0ull;
    const auto flush_stamps = [&]() {
        if (my_stamps) {
            if (lane == 0) { my_stamps[22] = __builtin_amdgcn_s_memtime(); my_stamps[25] = __builtin_amdgcn_s_memrealtime(); }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane < kMlpStampSlots)
                P.stamps[((((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 8 + w) * kMlpStampSlots + lane] = my_stamps[lane];
        }
    };
    if (my_stamps && lane == 0) { my_stamps[0] = __builtin_amdgcn_s_memtime(); my_stamps[24] = __builtin_amdgcn_s_memrealtime(); }
#else
    unsigned long long* my_stamps = nullptr;
    const auto flush_stamps = [] {};
#endif
    if (part < 2) {
        wgrad_dw2_glds<NS>(P, lds_raw, part, nb, s_begin, s_end, slab, tid, my_stamps);
        flush_stamps();
    } else if (P.w3part) {
        // ---- with the fused kernel's layer-3 partials the fourth role has next to nothing to do (9 us of adding 16 partial rows), and dW1 was the
        // longest role (27 us against dW2's 23.5: five MFMAs per wave and k-step against four, tools/wgrad_stamps.py): roles 2 and 3 each take
        // HALF of dW1's rows (128 output units = columns 128 (part - 2) .. of dZ1) and then adds half of the partials' elements.  Waves 4 (row blocks) x 2
        // (column groups: blocks 0-2 | blocks 3-4 of X's 160 columns).  Every element's products are accumulated in the same order as in the
        // one-role form below: the same bits.
        const int half = part - 2;
        wgrad_dw1_glds<NS>(P, lds_raw, half, nb, s_begin, s_end, slab, tid, my_stamps);
        flush_stamps();
    } else if (part == 2) {
        // dW1 = dZ1^T . X (144 columns) and db1 = dZ1^T . 1 (the tile's column 144 is all ones); wave w: rows 32w..
        __bf16* ta = lds;                        // dZ1 chunk [64][256]
        __bf16* tb = lds + kWgChunk * kTrH;      // X chunk [64][160]: 144 inputs | 1 | 15 zeros
        WG_STAMP(0);
        f32x16 acc[5];
#pragma unroll
        for (int b = 0; b < 5; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[b][i] = 0.f;
        WgChunk<kMlpHid> ca; WgChunk<kMlpInPad> cb;
        ca.load(P.dz1 + nb, kMlpHid, s_begin, s_end, tid);
        cb.load(P.xs, kMlpInPad, s_begin, s_end, tid);
        for (long long s = s_begin; s < s_end; s += kWgChunk) {
            mlp_barrier();
            ca.store(ta, kTrH, tid); cb.store(tb, kTrX, tid);
            if (tid < kWgChunk) {                                     // columns 144..159: a one (real rows only), zeros
                bf16x8 one = {(__bf16)((s + tid < s_end) ? 1.0f : 0.0f), (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};
                bf16x8 zero = {(__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};
                *reinterpret_cast<bf16x8*>(tb + tid * kTrX + kMlpInPad) = one;
                *reinterpret_cast<bf16x8*>(tb + tid * kTrX + kMlpInPad + 8) = zero;
            }
            mlp_barrier();
            if (s + kWgChunk < s_end) {
                ca.load(P.dz1 + nb, kMlpHid, s + kWgChunk, s_end, tid);
                cb.load(P.xs, kMlpInPad, s + kWgChunk, s_end, tid);
            }
#pragma unroll
            for (int ks = 0; ks < kWgChunk / 16; ++ks) {
                bf16x8 fb[5];
                const bf16x8 fa = wg_frag32(ta, kTrH, 16 * ks, 32 * w, lane);
#pragma unroll
                for (int b = 0; b < 5; ++b) fb[b] = wg_frag32(tb, kTrX, 16 * ks, 32 * b, lane);
#pragma unroll
                for (int b = 0; b < 5; ++b)
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb[b], acc[b], 0, 0, 0);
            }
        }
        {
#pragma unroll
            for (int b = 0; b < 5; ++b) wg_store_block(slab + kGW1, kMlpInPad, 32 * w, 32 * b, kMlpInPad, acc[b], lane);
            // column 144 of the product = db1: lane c == 16 of block b == 4
            if ((lane & 31) == 16) {
                const int hh = lane >> 5;
#pragma unroll
                for (int i = 0; i < 16; ++i) slab[kGB1 + 32 * w + (i & 3) + 8 * (i >> 2) + 4 * hh] = acc[4][i];
            }
        }
        WG_STAMP(22);
    } else {
        // dW3 [16][256] = G^T . H2, db3 = G^T . 1, db2 = 1^T . dZ2 of the slice from the stored H2 / dZ2 / G (no w3part: the weight-stationary
        // variant, pnr_mlp_backward) with 16x16x32 MFMAs — per 64-sample chunk a product chained over its two 32-sample k-steps from zero,
        // the chunks added in order: the same sums, bit for bit, as the fused kernel's per-tile products added in tile order above.
        __bf16* th = lds;                        // H2 chunk [64][256]
        __bf16* tz = lds + kWgChunk * kTrH;      // dZ2 chunk [64][256]
        __bf16* tg = lds + 2 * kWgChunk * kTrH;  // G chunk [64][16] as bf16
        f32x4 aw3[2], ab2[2], ab3 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < 2; ++b) { aw3[b] = ab3; ab2[b] = ab3; }
        WgChunk<kMlpHid> ch2, cz2;
        ch2.load(P.h2 + nb, kMlpHid, s_begin, s_end, tid);
        cz2.load(P.dz2 + nb, kMlpHid, s_begin, s_end, tid);
        for (long long s = s_begin; s < s_end; s += kWgChunk) {
            mlp_barrier();
            ch2.store(th, kTrH, tid); cz2.store(tz, kTrH, tid);
            if (tid < 2 * kWgChunk) {
                const int row = tid >> 1, half = tid & 1;
                f32x4 g0 = {0.f, 0.f, 0.f, 0.f}, g1 = g0;
                if (s + row < s_end) {
                    const float* gp = P.g_head + ((size_t)net * P.B + s + row) * kMlpHead + 8 * half;
                    g0 = *reinterpret_cast<const f32x4*>(gp); g1 = *reinterpret_cast<const f32x4*>(gp + 4);
                }
                bf16x8 pk;
#pragma unroll
                for (int j = 0; j < 4; ++j) { pk[j] = (__bf16)g0[j]; pk[4 + j] = (__bf16)g1[j]; }
                *reinterpret_cast<bf16x8*>(tg + row * kTrG + 8 * half) = pk;
            }
            mlp_barrier();
            if (s + kWgChunk < s_end) {
                ch2.load(P.h2 + nb, kMlpHid, s + kWgChunk, s_end, tid);
                cz2.load(P.dz2 + nb, kMlpHid, s + kWgChunk, s_end, tid);
            }
            f32x4 tw3[2], tb2[2], tb3;
            mlp_tile_w3_products(tg, kTrG, th, kTrH, lane, w, tw3, tb3);
            mlp_tile_b2_products(tz, kTrH, lane, w, tb2);
#pragma unroll
            for (int b = 0; b < 2; ++b) { aw3[b] += tw3[b]; ab2[b] += tb2[b]; }
            ab3 += tb3;
        }
        const int c16 = lane & 15, g = lane >> 4;                  // C: col = lane & 15, rows 4g .. 4g+3
#pragma unroll
        for (int b = 0; b < 2; ++b) {
#pragma unroll
            for (int j = 0; j < 4; ++j) slab[kGW3 + (4 * g + j) * kMlpHid + 32 * w + 16 * b + c16] = aw3[b][j];
            if (g == 0) slab[kGB2 + 32 * w + 16 * b + c16] = ab2[b][0];            // every row of 1^T . dZ2 is db2
        }
        if (w == 0 && c16 == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) slab[kGB3 + 4 * g + j] = ab3[j];           // every column of G^T . 1 is db3
        }
    }
}

struct MlpReduceParams {
    const float* slabs;        // [slices][2][kGradElems]
    int slices;
    float* gw1[kMlpNets]; float* gb1[kMlpNets];    // gradients in the master parameters' layouts
    float* gw2[kMlpNets]; float* gb2[kMlpNets];
    float* gw3[kMlpNets]; float* gb3[kMlpNets];
    int n3[kMlpNets];
    int accumulate;            // 1: add to what the gradient tensors hold (autograd accumulation), 0: overwrite
    const float* scale;        // device scalar multiplied into the sums (the upstream d / d loss), or null: 1
};

// Sum the slices' slabs in slice order (deterministic) and scatter into the parameter-shaped gradients.
__global__ __launch_bounds__(256) void mlp_reduce_kernel(const MlpReduceParams P)
{
    const int net = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= kGradElems) return;
    float* dst = nullptr;
    if (e < kGW2) { const int o = e / kMlpInPad, k = e % kMlpInPad; if (k < kMlpIn) dst = P.gw1[net] + o * kMlpIn + k; }
    else if (e < kGW3) dst = P.gw2[net] + (e - kGW2);
    else if (e < kGB1) { const int r = (e - kGW3) / kMlpHid; if (r < P.n3[net]) dst = P.gw3[net] + (e - kGW3); }
    else if (e < kGB2) dst = P.gb1[net] + (e - kGB1);
    else if (e < kGB3) dst = P.gb2[net] + (e - kGB2);
    else if (e - kGB3 < P.n3[net]) dst = P.gb3[net] + (e - kGB3);
    if (!dst) return;
    float s = 0.f;
    const float* p = P.slabs + (size_t)net * kGradElems + e;
    for (int k = 0; k < P.slices; ++k) s += p[(size_t)k * kMlpNets * kGradElems];
    if (P.scale) s *= *P.scale;
    *dst = P.accumulate ? (*dst + s) : s;
}

// slabs -> one flat gradient [2][kGradElems] (the bucket a multi-GPU run all-reduces), summed in slice order
// (elements [first, first + count) of the bucket: one net's half when the nets are driven as two chains)
__global__ __launch_bounds__(256) void mlp_reduce_flat_kernel(const float* __restrict__ slabs, int slices, float* __restrict__ flat, int first, int count)
{
    const int i = first + blockIdx.x * 256 + threadIdx.x;
    if (i >= first + count) return;
    constexpr size_t kStride = (size_t)kMlpNets * kGradElems;
    float s = 0.f;
    int k = 0;
    for (; k + 8 <= slices; k += 8) {                       // slice order, eight loads in flight (see mlp_adam_kernel)
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = slabs[(size_t)(k + j) * kStride + i];
#pragma unroll
        for (int j = 0; j < 8; ++j) s += x[j];
    }
    for (; k < slices; ++k) s += slabs[(size_t)k * kStride + i];
    flat[i] = s;
}

}  // namespace pnr
#pragma clang fp contract(off)
