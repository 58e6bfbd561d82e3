// grouped_gemm_img.hip -- the IMAGE path of the grouped GEMM (the default; overview in
// grouped_gemm.hip): gemm_tile_img, the three kernel families built on it -- grouped_gemm_img_kernel
// (fp32 semantics: operands as pre-split images, or the activation as fp32 rows), grouped_gemm_bf16_kernel
// and grouped_gemm_bf16_ext_kernel (bf16 tensors) -- and their launcher.
// Diagnostic builds of this unit (tools/variant.sh NAME grouped_gemm_img FLAG): -DGG_STAMP_DMA
// (tools/micro/gemm_stamps.py), -DGG_ABL_NO_A / _NO_B / _NO_EPI (tools/micro/gemm_abl.py).
#include "grouped_gemm.h"
#include "grouped_image.h"

namespace spt {

constexpr int GI_TILE = 16384;                  // bytes of one operand tile
constexpr int GI_STAGE = 2 * GI_TILE;           // A | B
constexpr int GI_LDS_FLOATS = 2 * GI_STAGE / 4; // two stages

__device__ __forceinline__ void gg_glds16(const char *src, char *lds_wave_base) {
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void *)src,
        (__attribute__((address_space(3))) void *)lds_wave_base, 16, 0, 0);
}

// Per-lane state of the image path's k-loop.
template <int NI, int NA>
struct GiLane {
    const char *a_src[NA];      // LDS-DMA sources of this lane, k-step 0
    const char *b_src[4];
    long long w_rowb;
    int wave, wm, wn, frow, fh, lane;
};
template <int NI>
struct GiFrags {
    Frag a[NI], b[2];
};
template <int NI, int NA, bool KC_B, bool A32 = false>
__device__ __forceinline__ void gi_read(const GiLane<NI, NA> &c, const char *As, const char *Bs,
                                        int q2, GiFrags<NI> &f) {
#pragma unroll
    for (int i = 0; i < NI; i++) {
        if constexpr (A32) {
            f.a[i] = gi_frag_a32(As, c.wm + 32 * i + c.frow, q2, c.fh);
        } else {
            f.a[i].hi = gi_frag_kc(As, c.wm + 32 * i + c.frow, q2, 0, c.fh);
            f.a[i].lo = gi_frag_kc(As, c.wm + 32 * i + c.frow, q2, 1, c.fh);
        }
    }
#pragma unroll
    for (int j = 0; j < 2; j++) {
        if constexpr (KC_B) {
            f.b[j].hi = gi_frag_kc(Bs, c.wn + 32 * j + c.frow, q2, 0, c.fh);
            f.b[j].lo = gi_frag_kc(Bs, c.wn + 32 * j + c.frow, q2, 1, c.fh);
        } else {
            f.b[j].hi = gi_frag_nc(Bs, c.wn + 32 * j, q2, 0, c.fh, c.lane);
            f.b[j].lo = gi_frag_nc(Bs, c.wn + 32 * j, q2, 1, c.fh, c.lane);
        }
    }
}
// BF16 (spt_grouped_gemm_bf16): the operands ARE bf16 and a stage holds 64 k -- the "hi" fragment
// is k 0 .. 31 of the step, the "lo" fragment k 32 .. 63 -- so a fragment pair is two plain products
template <int NI, bool BF16 = false>
__device__ __forceinline__ void gi_mma(const GiFrags<NI> &f, f32x16 (&acc)[NI][2]) {
#pragma unroll
    for (int i = 0; i < NI; i++) {
        if constexpr (BF16) {
#pragma unroll
            for (int j = 0; j < 2; j++) {
                acc[i][j] = mma(f.a[i].hi, f.b[j].hi, acc[i][j]);
                acc[i][j] = mma(f.a[i].lo, f.b[j].lo, acc[i][j]);
            }
        } else {
            acc[i][0] = mm<2, 2>(f.a[i], f.b[0], acc[i][0]);
            acc[i][1] = mm<2, 2>(f.a[i], f.b[1], acc[i][1]);
        }
    }
}
template <int NI, int NA, bool KC_B, bool BF16 = false>
__device__ __forceinline__ void gi_contract(const GiLane<NI, NA> &c, const char *As, const char *Bs,
                                            int q2, f32x16 (&acc)[NI][2]) {
    GiFrags<NI> f;
    gi_read<NI, NA, KC_B>(c, As, Bs, q2, f);
    gi_mma<NI, BF16>(f, acc);
}
// k-step k0 .. k0 + 31 into the LDS stage at `dma` (instruction t = wave + 4 j: 1 KiB each)
// (BF16: k-steps of 64 bf16 -- the same 128 bytes per row of a KC tile, k0 * 2 bytes into the row)
template <int NI, int NA, bool BN_LAYOUT, bool BF16 = false>
__device__ __forceinline__ void gi_stage(const GiLane<NI, NA> &c, char *dma, int k0) {
    const size_t ka = BF16 ? (size_t)k0 * 2 : (size_t)(k0 >> 5) * 128;
    // (ablation builds, tools/variant.sh: wrong results, for timing -- which operand's stream
    // the k-loop waits for)
#ifdef GG_ABL_NO_A
    if (k0 < 64)
#endif
#pragma unroll
    for (int j = 0; j < NA; j++) gg_glds16(c.a_src[j] + ka, dma + (c.wave + 4 * j) * 1024);
#ifdef GG_ABL_NO_B
    if (k0 < 64)
#endif
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if constexpr (!BN_LAYOUT)
            gg_glds16(c.b_src[j] + ka, dma + GI_TILE + (c.wave + 4 * j) * 1024);
        else
            gg_glds16(c.b_src[j] + (size_t)k0 * c.w_rowb, dma + GI_TILE + (c.wave + 4 * j) * 1024);
    }
}
// One k-step: issue the LDS-DMAs of the NEXT step into `dma`, contract the stage at `cur`.
// The two pointers are __restrict__ on purpose: inlined, they give the DMA stores and the
// ds_reads alias scopes, and only with those does hipcc (ROCm 7.2) leave out the
// `s_waitcnt vmcnt(0)` it otherwise puts in front of the first ds_read behind an LDS-DMA in
// flight -- which would wait for the next tile before the current one is contracted.
template <int NI, int NA, bool BN_LAYOUT, bool A32, bool BF16 = false>
__device__ __forceinline__ void gi_step(const GiLane<NI, NA> &c, char *__restrict__ dma,
                                        const char *__restrict__ cur, bool prefetch, int k_next,
                                        f32x16 (&acc)[NI][2]
#ifdef GG_STAMP_DMA
                                        // (diagnostic build, tools/micro/gemm_stamps.py: cycles of a step
                                        // spent issuing its LDS-DMAs / reading fragments / in its MFMAs)
                                        , unsigned long long (&st)[4]
#endif
                                        ) {
    // The order is pinned: the fragments of the step's second half are requested BEFORE the
    // MFMAs of the first, so that their LDS latency passes behind 12 MFMAs.  The wait for the
    // first half stands in front of those reads -- behind them hipcc makes it lgkmcnt(0) (no
    // counted wait is available to it while an LDS-DMA is pending), a wait for the reads just
    // issued.  Left alone, hipcc also sinks each group of reads to its first use and hoists the
    // barrier that follows (with its vmcnt(0), the wait for the NEXT tile) above half the MFMAs.
    GiFrags<NI> f0, f1;
#ifdef GG_STAMP_DMA
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#endif
    if (prefetch) gi_stage<NI, NA, BN_LAYOUT, BF16>(c, dma, k_next);
#ifdef GG_STAMP_DMA
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
#endif
    gi_read<NI, NA, !BN_LAYOUT, A32>(c, cur, cur + GI_TILE, 0, f0);
    __builtin_amdgcn_s_waitcnt(0xC07F);                 // lgkmcnt(0) only
    __builtin_amdgcn_sched_barrier(0);
    gi_read<NI, NA, !BN_LAYOUT, A32>(c, cur, cur + GI_TILE, 1, f1);
    __builtin_amdgcn_sched_barrier(0);
#ifdef GG_STAMP_DMA
    const unsigned long long t2 = __builtin_amdgcn_s_memtime();
#endif
    gi_mma<NI, BF16>(f0, acc);
    __builtin_amdgcn_sched_barrier(0);
    gi_mma<NI, BF16>(f1, acc);
    __builtin_amdgcn_sched_barrier(0);
#ifdef GG_STAMP_DMA
    const unsigned long long t3 = __builtin_amdgcn_s_memtime();
    st[0] += t1 - t0; st[1] += t2 - t1; st[2] += t3 - t2;
#endif
}

// BF16 (spt_grouped_gemm_bf16): a, w, bias and out hold bf16 (their float pointers of GroupedArgs
// carry bf16 tensors); both operands go global -> LDS by LDS-DMA straight from the tensors, 64 k per
// stage in the tiles' 128-byte rows (KC: chunk c = k 8 c .. 8 c + 7; NC: "part" 0 / 1 = k-rows
// kr / 32 + kr of the step), two plain MFMAs per fragment pair; no K extension
// SEG (spt_grouped_gemm_fused_w16 alone): the segmented contraction of the register path (a_seg_k,
// R up to 64, b2_seg) from the weight's image and the activation's fp32 rows -- the same k-steps in the
// same order, so the same bits -- for a weight stored in halves, which has no register-operand form
template <int BM, bool BN_LAYOUT, int EPI, bool EXT, bool A32, bool BF16 = false, bool SEG = false>
__device__ __forceinline__ void gemm_tile_img(const GroupedArgs &g, float *smem, int bucket,
                                              int row_lo, int row_hi, int col_tile) {
    static_assert(!(BF16 && A32), "bf16: no fp32 rows");
    static_assert(!SEG || (A32 && EPI == EPI_PLAIN), "segments: fp32 rows, plain epilogue");
    constexpr int NI = BM / 64;                 // 32-row sub-blocks per wave
    constexpr int NA = BM / 32;                 // LDS-DMA instructions per wave: A tile
    constexpr int KS = BF16 ? 2 * GG_BK : GG_BK;    // k per stage
#ifdef GG_STAMP_DMA
    const unsigned long long t_enter = __builtin_amdgcn_s_memtime();
#endif
    char *const lds0 = reinterpret_cast<char *>(smem);
    const int n0 = col_tile * GG_BN;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    GiLane<NI, NA> c;
    c.lane = lane;
    c.wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    c.wm = (c.wave >> 1) * (BM / 2);            // the wave's origin inside the tile
    c.wn = (c.wave & 1) * 64;
    c.frow = lane & 31;
    c.fh = lane >> 5;
    c.w_rowb = g.w_rowb;
    const int wave = c.wave, wm = c.wm, wn = c.wn;

    float *const extras = smem + GI_LDS_FLOATS;
    if (tid < BM) {
        const int p = min(row_lo + tid, row_hi - 1);
        const float rs = g.rowscale ? g.rowscale[p] : 1.0f;
        extras[384 + tid] = rs;
        if (EPI == EPI_ACT && g.act == ACT_RELU && g.a_norm)
            extras[256 + tid] = g.a_norm[g.gather ? g.gather[p] : p] * rs;
    }
    // ---- LDS-DMA sources.  KC tile: instruction t = wave + 4 j covers rows 8 t .. 8 t + 7,
    // lane -> row 8 t + (lane >> 3), physical chunk lane & 7.  Rows past the bucket end and
    // columns past N are computed but never stored: clamped, not predicated. ----
#pragma unroll
    for (int j = 0; j < NA; j++) {
        const int r = 8 * (wave + 4 * j) + (lane >> 3);
        const int p = min(row_lo + r, row_hi - 1);
        const long long src = g.gather ? g.gather[p] : p;
        // (A32: the fp32 rows themselves, a_rowb = 4 lda; 32 k = 128 bytes per k-step either way)
        c.a_src[j] = (A32 || BF16 ? reinterpret_cast<const char *>(g.a) : g.a_img) + src * g.a_rowb +
                     (((lane & 7) ^ ((r >> 1) & 7)) << 4);
    }
    const char *wg = BF16 ? reinterpret_cast<const char *>(g.w) + (size_t)bucket * g.gstride * 2
                          : g.w_img + (long long)bucket * g.w_grow * g.w_rowb + (size_t)bucket * g.w_gblk * 128;
    if constexpr (!BN_LAYOUT) {
        // W_g(n, k), k contiguous: image row = n, block = k / 32 (bf16: row n of the weight)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int r = 8 * (wave + 4 * j) + (lane >> 3);
            const long long n = min(n0 + r, g.N - 1);
            c.b_src[j] = wg + n * g.w_rowb + (((lane & 7) ^ ((r >> 1) & 7)) << 4);
        }
    } else {
        // W_g(n, k), n contiguous: image row = k, block = n / 32.  NC tile: instruction t
        // covers k-rows 2 t, 2 t + 1; lane -> k-row 2 t + (lane >> 5), physical chunk lane & 31
        const int nblocks = (g.N + 31) >> 5;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int kr = 2 * (wave + 4 * j) + (lane >> 5);
            const int pchunk = lane & 31;
            const int seg = (pchunk >> 2) ^ (kr & 3);               // logical segment
            const int nb = min((n0 >> 5) + (seg >> 1), nblocks - 1);
            if constexpr (BF16)     // part = seg & 1: weight row k = 32 part + kr, 32 n = 64 bytes
                c.b_src[j] = wg + (long long)(32 * (seg & 1) + kr) * g.w_rowb + (size_t)nb * 64 +
                             ((pchunk & 3) << 4);
            else
                c.b_src[j] = wg + (long long)kr * g.w_rowb + (size_t)nb * 128 + (seg & 1) * 64 +
                             ((pchunk & 3) << 4);
        }
    }

    f32x16 acc[NI][2];
#pragma unroll
    for (int i = 0; i < NI; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;

    // ---- k-loop: the LDS-DMAs of step t + 1 are in flight while step t is contracted; the
    // barrier at the end of a step (with the vmcnt(0) / lgkmcnt(0) hipcc puts in front of it)
    // both publishes stage (t + 1) & 1 and retires the reads of stage t & 1 ----
    gi_stage<NI, NA, BN_LAYOUT, BF16>(c, lds0, 0);
    __syncthreads();
#ifdef GG_STAMP_DMA
    unsigned long long st[4] = {0, 0, 0, 0};
    const unsigned long long loop0 = __builtin_amdgcn_s_memtime();
#define GG_ST , st
#define GG_BAR(x)                                                       \
    do {                                                                \
        const unsigned long long b0 = __builtin_amdgcn_s_memtime();     \
        __syncthreads();                                                \
        st[3] += __builtin_amdgcn_s_memtime() - b0;                     \
    } while (0)
#else
#define GG_ST
#define GG_BAR(x) __syncthreads()
#endif
    if constexpr (SEG) {
        // K in segments: gi_stage reads a_src + 4 k0 bytes, so when the NEXT step to be staged opens a
        // new segment the sources move on by what lies between the two matrices (the register path's a_adj)
        const long long seg_skip = (g.a_seg_stride - g.a_seg_k) * 4;
        int seg_left = g.a_seg_k > 0 ? g.a_seg_k - KS : 0x7FFFFFFF;      // (step 0 is staged)
        auto next_step = [&]() {
            if (seg_left <= 0) {
#pragma unroll
                for (int j = 0; j < NA; j++) c.a_src[j] += seg_skip;
                seg_left = g.a_seg_k;
            }
            seg_left -= KS;
        };
        for (int k0 = 0; k0 < g.K; k0 += 2 * KS) {
            next_step();
            gi_step<NI, NA, BN_LAYOUT, A32, BF16>(c, lds0 + GI_STAGE, lds0, k0 + KS < g.K, k0 + KS, acc GG_ST);
            GG_BAR(0);
            if (k0 + KS < g.K) {
                next_step();
                gi_step<NI, NA, BN_LAYOUT, A32, BF16>(c, lds0, lds0 + GI_STAGE, k0 + 2 * KS < g.K,
                                                      k0 + 2 * KS, acc GG_ST);
                GG_BAR(0);
            }
        }
    } else {
        for (int k0 = 0; k0 < g.K; k0 += 2 * KS) {
            gi_step<NI, NA, BN_LAYOUT, A32, BF16>(c, lds0 + GI_STAGE, lds0, k0 + KS < g.K, k0 + KS, acc GG_ST);
            GG_BAR(0);
            if (k0 + KS < g.K) {
                gi_step<NI, NA, BN_LAYOUT, A32, BF16>(c, lds0, lds0 + GI_STAGE, k0 + 2 * KS < g.K,
                                                      k0 + 2 * KS, acc GG_ST);
                GG_BAR(0);
            }
        }
    }
#ifdef GG_STAMP_DMA
    const unsigned long long loop1 = __builtin_amdgcn_s_memtime();
#endif
#undef GG_ST
#undef GG_BAR

    gg_scale_rows<NI>(g, acc, extras, wm);

    // ---- K extension: fp32 a2 [*, R] and b2 [n][R] split while staged into two KC tiles
    // (R <= 32: one k-step, zero beyond R).  BF16 (spt_grouped_gemm_bf16_ext): a2 is fp32 and b2 bf16;
    // a2's hi goes to k 0 .. 31 of the stage, its lo to k 32 .. 63, b2's row to both halves, and the
    // two plain products of a bf16 fragment pair form hi.b2 + lo.b2 (<= 2^-16 relative per product) ----
    if (EXT && BF16) {
        char *As = lds0, *Bs = lds0 + GI_TILE;
        const int kq = tid & 7, k = 4 * kq;                 // 8 lanes per row: 4 k's each
        auto put = [&](char *tile, int r, unsigned x0, unsigned x1, unsigned y0, unsigned y1) {
            const int sw = (r >> 1) & 7;
            char *row = tile + r * 128 + (kq & 1) * 8;
            *reinterpret_cast<uint2 *>(row + (((kq >> 1) ^ sw) << 4)) = make_uint2(x0, x1);
            *reinterpret_cast<uint2 *>(row + (((4 + (kq >> 1)) ^ sw) << 4)) = make_uint2(y0, y1);
        };
#pragma unroll
        for (int u = 0; u < BM / 32; u++) {
            const int r = (tid >> 3) + 32 * u;
            const int p = row_lo + r;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p < row_hi && k < g.R) {
                const long long src = g.gather2 ? g.gather2[p] : p;
                v = *reinterpret_cast<const float4 *>(g.a2 + src * g.lda2 + k);
            }
            const Split s0 = split2(v.x, v.y), s1 = split2(v.z, v.w);
            put(As, r, s0.hi, s1.hi, s0.lo, s1.lo);
        }
        const unsigned short *b2 = reinterpret_cast<const unsigned short *>(g.b2);
#pragma unroll
        for (int u = 0; u < GG_BN / 32; u++) {
            const int r = (tid >> 3) + 32 * u;
            const int n = n0 + r;
            uint2 b = make_uint2(0u, 0u);
            if (n < g.N && k < g.R)
                b = *reinterpret_cast<const uint2 *>(b2 + (size_t)bucket * g.b2_gstride + (size_t)n * g.b2_ldn + k);
            put(Bs, r, b.x, b.y, b.x, b.y);
        }
        __syncthreads();
        gi_contract<NI, NA, true, true>(c, As, Bs, 0, acc);
        if (g.R > 16) gi_contract<NI, NA, true, true>(c, As, Bs, 1, acc);
        __syncthreads();
    } else if constexpr (EXT && SEG) {
        // up to 64 columns, 32 per step as on the register path; b2 possibly in 16-column segments
        char *As = lds0, *Bs = lds0 + GI_TILE;
        const int kq = tid & 7;
        auto put4 = [&](char *tile, int r, const float4 &v) {
            const Split s0 = split2(v.x, v.y), s1 = split2(v.z, v.w);
            const int sw = (r >> 1) & 7;
            char *row = tile + r * 128 + (kq & 1) * 8;
            *reinterpret_cast<uint2 *>(row + (((kq >> 1) ^ sw) << 4)) = make_uint2(s0.hi, s1.hi);
            *reinterpret_cast<uint2 *>(row + (((4 + (kq >> 1)) ^ sw) << 4)) = make_uint2(s0.lo, s1.lo);
        };
        for (int r0 = 0; r0 < g.R; r0 += GG_BK) {
            const int k = r0 + 4 * kq;
#pragma unroll
            for (int u = 0; u < BM / 32; u++) {
                const int r = (tid >> 3) + 32 * u;
                const int p = row_lo + r;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (p < row_hi && k < g.R) {
                    const long long src = g.gather2 ? g.gather2[p] : p;
                    v = *reinterpret_cast<const float4 *>(g.a2 + src * g.lda2 + k);
                }
                put4(As, r, v);
            }
#pragma unroll
            for (int u = 0; u < GG_BN / 32; u++) {
                const int r = (tid >> 3) + 32 * u;
                const int n = n0 + r;
                float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
                if (n < g.N && k < g.R)
                    b = *reinterpret_cast<const float4 *>(
                        g.b2 + (size_t)bucket * g.b2_gstride + (size_t)n * g.b2_ldn +
                        (g.b2_seg ? (size_t)(k >> 4) * g.b2_seg + (k & 15) : (size_t)k));
                put4(Bs, r, b);
            }
            __syncthreads();
            gi_contract<NI, NA, true>(c, As, Bs, 0, acc);
            if (g.R - r0 > 16) gi_contract<NI, NA, true>(c, As, Bs, 1, acc);
            __syncthreads();
        }
    } else if (EXT) {
        char *As = lds0, *Bs = lds0 + GI_TILE;
        const int kq = tid & 7, k = 4 * kq;                 // 8 lanes per row: 4 k's each
        auto put4 = [&](char *tile, int r, const float4 &v) {
            const Split s0 = split2(v.x, v.y), s1 = split2(v.z, v.w);
            const int sw = (r >> 1) & 7;
            char *row = tile + r * 128 + (kq & 1) * 8;
            *reinterpret_cast<uint2 *>(row + (((kq >> 1) ^ sw) << 4)) = make_uint2(s0.hi, s1.hi);
            *reinterpret_cast<uint2 *>(row + (((4 + (kq >> 1)) ^ sw) << 4)) = make_uint2(s0.lo, s1.lo);
        };
#pragma unroll
        for (int u = 0; u < BM / 32; u++) {
            const int r = (tid >> 3) + 32 * u;
            const int p = row_lo + r;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p < row_hi && k < g.R) {
                const long long src = g.gather2 ? g.gather2[p] : p;
                v = *reinterpret_cast<const float4 *>(g.a2 + src * g.lda2 + k);
            }
            put4(As, r, v);
            const float ss = group_sum<8>(v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w);
            if (kq == 0) extras[r] = ss;                    // |a2 row|^2, for the epilogue
        }
#pragma unroll
        for (int u = 0; u < GG_BN / 32; u++) {
            const int r = (tid >> 3) + 32 * u;
            const int n = n0 + r;
            float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n < g.N && k < g.R)
                b = *reinterpret_cast<const float4 *>(g.b2 + (size_t)bucket * g.b2_gstride +
                                                      (size_t)n * g.b2_ldn + k);
            put4(Bs, r, b);
            const float ss = group_sum<8>(b.x * b.x + b.y * b.y + b.z * b.z + b.w * b.w);
            if (kq == 0) extras[128 + r] = ss;              // |b2 row|^2
        }
        __syncthreads();
        gi_contract<NI, NA, true>(c, As, Bs, 0, acc);
        if (g.R > 16) gi_contract<NI, NA, true>(c, As, Bs, 1, acc);
        __syncthreads();
    }
#ifdef GG_ABL_NO_EPI
    if (acc[0][0][0] == 123.456f) g.out[0] = acc[0][1][3] + acc[NI - 1][0][5];
    return;
#endif
#ifdef GG_STAMP_DMA
    const unsigned long long epi0 = __builtin_amdgcn_s_memtime();
#endif
    gg_epilogue<NI, EPI, BF16>(g, smem, acc, bucket, row_lo, row_hi, col_tile, wm, wn, extras, EXT);
#ifdef GG_STAMP_DMA
    if (lane == 0) {
        // eight counters per wave behind the launch's output (the caller allocates the room):
        // the loop's four phases; loop; entry -> loop; loop -> epilogue; epilogue
        unsigned long long *dst = reinterpret_cast<unsigned long long *>(g.out + (size_t)g.P * g.ldo) +
                                  ((size_t)blockIdx.x * 4 + wave) * 8;
        dst[0] = st[0]; dst[1] = st[1]; dst[2] = st[2]; dst[3] = st[3];
        dst[4] = loop1 - loop0; dst[5] = loop0 - t_enter; dst[6] = epi0 - loop1;
        dst[7] = __builtin_amdgcn_s_memtime() - epi0;
    }
#endif
}

// (Round 4 also built a persistent form of the kernel above whose finished tile waited in registers
// and was stored, a dword per lane straight from the accumulator layout, in the shadow of the next
// tile's MFMAs: 483 against 428 us at 4096 tiles, 56.2 against 55.0 ms in the step -- four times the
// store instructions of the LDS-transposed epilogue cost more than the overlap returns.  Not kept.)

template <bool BN_LAYOUT, int EPI, bool EXT, bool A32>
__global__ __launch_bounds__(GG_THREADS, 2) void grouped_gemm_img_kernel(GroupedArgs g) {
    // ALL of the kernel's LDS in one array (a second __shared__ object beside an LDS-DMA
    // target can make hipcc drain vmcnt before every ds_read: cdna guide, section 5)
    __shared__ __attribute__((aligned(1024))) float smem[GI_LDS_FLOATS + GG_EXTRAS];
    const GgWork w = gg_find_work(g);
    if (w.bucket < 0) return;
    if (w.half < 0)
        gemm_tile_img<GG_BM, BN_LAYOUT, EPI, EXT, A32>(g, smem, w.bucket, w.row_lo, w.row_hi, w.col_tile);
    else
        gemm_tile_img<GG_BM / 2, BN_LAYOUT, EPI, EXT, A32>(g, smem, w.bucket, w.row_lo, w.row_hi,
                                                           w.col_tile);
}

// the segmented form (gemm_tile_img: SEG): plain epilogue, the activation's fp32 rows
template <bool BN_LAYOUT, bool EXT>
__global__ __launch_bounds__(GG_THREADS, 2) void grouped_gemm_img_seg_kernel(GroupedArgs g) {
    __shared__ __attribute__((aligned(1024))) float smem[GI_LDS_FLOATS + GG_EXTRAS];
    const GgWork w = gg_find_work(g);
    if (w.bucket < 0) return;
    if (w.half < 0)
        gemm_tile_img<GG_BM, BN_LAYOUT, EPI_PLAIN, EXT, true, false, true>(g, smem, w.bucket, w.row_lo, w.row_hi,
                                                                           w.col_tile);
    else
        gemm_tile_img<GG_BM / 2, BN_LAYOUT, EPI_PLAIN, EXT, true, false, true>(g, smem, w.bucket, w.row_lo,
                                                                               w.row_hi, w.col_tile);
}

// spt_grouped_gemm_bf16: the image kernel's k-loop and epilogue on bf16 tensors (PLAIN / ACT / DACT)
template <bool BN_LAYOUT, int EPI>
__global__ __launch_bounds__(GG_THREADS, 2) void grouped_gemm_bf16_kernel(GroupedArgs g) {
    __shared__ __attribute__((aligned(1024))) float smem[GI_LDS_FLOATS + GG_EXTRAS];
    const GgWork w = gg_find_work(g);
    if (w.bucket < 0) return;
    if (w.half < 0)
        gemm_tile_img<GG_BM, BN_LAYOUT, EPI, false, false, true>(g, smem, w.bucket, w.row_lo, w.row_hi,
                                                                 w.col_tile);
    else
        gemm_tile_img<GG_BM / 2, BN_LAYOUT, EPI, false, false, true>(g, smem, w.bucket, w.row_lo, w.row_hi,
                                                                     w.col_tile);
}

// spt_grouped_gemm_bf16_ext: the same with the fp32-a2 / bf16-b2 K extension after the scaling
template <bool BN_LAYOUT, int EPI>
__global__ __launch_bounds__(GG_THREADS, 2) void grouped_gemm_bf16_ext_kernel(GroupedArgs g) {
    __shared__ __attribute__((aligned(1024))) float smem[GI_LDS_FLOATS + GG_EXTRAS];
    const GgWork w = gg_find_work(g);
    if (w.bucket < 0) return;
    if (w.half < 0)
        gemm_tile_img<GG_BM, BN_LAYOUT, EPI, true, false, true>(g, smem, w.bucket, w.row_lo, w.row_hi,
                                                                w.col_tile);
    else
        gemm_tile_img<GG_BM / 2, BN_LAYOUT, EPI, true, false, true>(g, smem, w.bucket, w.row_lo, w.row_hi,
                                                                    w.col_tile);
}

template <bool BN_LAYOUT, int EPI>
static GgKernel img_kernel(bool ext, int operands) {
    if (operands == GG_OPS_BF16)
        return ext ? grouped_gemm_bf16_ext_kernel<BN_LAYOUT, EPI> : grouped_gemm_bf16_kernel<BN_LAYOUT, EPI>;
    if (operands == GG_OPS_A32)
        return ext ? grouped_gemm_img_kernel<BN_LAYOUT, EPI, true, true> : grouped_gemm_img_kernel<BN_LAYOUT, EPI, false, true>;
    return ext ? grouped_gemm_img_kernel<BN_LAYOUT, EPI, true, false> : grouped_gemm_img_kernel<BN_LAYOUT, EPI, false, false>;
}
template <bool BN_LAYOUT>
static GgKernel img_kernel(int epilogue, bool ext, int operands) {
    return epilogue == EPI_PLAIN ? img_kernel<BN_LAYOUT, EPI_PLAIN>(ext, operands)
           : epilogue == EPI_ACT ? img_kernel<BN_LAYOUT, EPI_ACT>(ext, operands)
                                 : img_kernel<BN_LAYOUT, EPI_DACT>(ext, operands);
}

int launch_gemm_img(const GroupedArgs &g, int epilogue, bool ext, int operands, dim3 grid, hipStream_t s) {
    GgKernel kernel = g.ldk == 1 ? img_kernel<false>(epilogue, ext, operands) : img_kernel<true>(epilogue, ext, operands);
    if (operands == GG_OPS_A32 && gg_segmented(g)) {
        if (epilogue != EPI_PLAIN) return SPT_EUNSUP;
        kernel = g.ldk == 1 ? (ext ? grouped_gemm_img_seg_kernel<false, true> : grouped_gemm_img_seg_kernel<false, false>)
                            : (ext ? grouped_gemm_img_seg_kernel<true, true> : grouped_gemm_img_seg_kernel<true, false>);
    }
    hipLaunchKernelGGL(kernel, grid, dim3(GG_THREADS), 0, s, g);
    SPT_LAUNCH_CHECK();
    return SPT_OK;
}

}  // namespace spt
