// grouped_gemm_regs.hip -- the REGISTER path of the grouped GEMM (overview in grouped_gemm.hip):
// gemm_tile_regs, grouped_gemm_kernel and its launcher.
#include "grouped_gemm.h"

namespace spt {

// fp32 operands, split while they are staged.  LDS images of a tile: bf16, one image per part
// of the split (hi, lo and -- GEMMs in front of a ReLU -- mid).  k-contiguous tiles: rows of
// 32 k (64 B + 16 pad): a fragment (8 k of one row) is one conflict-free ds_read_b128 per
// part.  n-contiguous weight tiles stay [k][n] (rows of 128 n, 256 B + 64 pad) and are read
// with the transposing ds_read_b64_tr_b16.
constexpr int GG_KQ = GG_BK / 4;                 // float4 per tile row
constexpr int GG_RPP = GG_THREADS / GG_KQ;       // tile rows staged per pass
constexpr int GG_NU = GG_BN / GG_RPP;            // float4 of B per thread per k-step
constexpr int GG_BNK = GG_THREADS / 32;          // k rows of an n-contiguous B tile staged per pass
constexpr int GG_ROWB = GG_BK * 2 + 16;          // bytes per row of a k-contiguous image: 80
constexpr int GG_BNROWB = GG_BN * 2 + 64;        // bytes per k-row of an n-contiguous image: 320
constexpr int GG_AIMG = GG_BM * GG_ROWB;         // one part of the A tile: 10240 B
constexpr int GG_BIMG = GG_BN * GG_ROWB;         // one part of a B tile (either orientation)
static_assert(GG_BK * GG_BNROWB == GG_BIMG, "both B orientations fit the same slot");
constexpr int GG_REGS_LDS_FLOATS = 2 * (GG_AIMG + GG_BIMG) / 4;   // A | B, hi | lo each

// One output tile of BM x 128: BM = 128 (each wave a 64 x 64 quadrant) or BM = 64 (each
// wave 32 x 64), same B tile, same LDS image, same epilogue.
template <int BM, bool BN_LAYOUT, int EPI, bool EXT, bool KTAIL>
__device__ __forceinline__ void gemm_tile_regs(const GroupedArgs &g, float *smem, int bucket,
                                               int row_lo, int row_hi, int col_tile) {
    constexpr int NI = BM / 64;                  // 32-row sub-blocks per wave
    constexpr int NUA = BM / GG_RPP;             // float4 of A per thread per k-step
    constexpr int NPART = 2;                     // hi, lo
    char *const lds0 = reinterpret_cast<char *>(smem);
    char *As = lds0;                                      // [NPART][GG_AIMG]: hi | lo
    char *Bs = As + NPART * GG_AIMG;                      // [NPART][GG_BIMG]
    const int n0 = col_tile * GG_BN;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = (wave >> 1) * (BM / 2);       // the wave's origin inside the tile
    const int wn = (wave & 1) * 64;
    const float *wg = g.w + (size_t)bucket * g.gstride;

    float *const extras = smem + GG_REGS_LDS_FLOATS;
    if (tid < BM) {
        const int p = min(row_lo + tid, row_hi - 1);
        const float rs = g.rowscale ? g.rowscale[p] : 1.0f;
        extras[384 + tid] = rs;
        if (EPI == EPI_ACT && g.act == ACT_RELU && g.a_norm)
            extras[256 + tid] = g.a_norm[g.gather ? g.gather[p] : p] * rs;
    }
    // ---- staging assignment: tile = rows x GG_KQ float4 along k ----
    // (8 lanes per row; the two rows of a 16-lane ds_write_b64 group are 4 apart: 320 bytes = 64
    // mod 128, so their 64-byte pieces fall on disjoint banks -- adjacent rows, 80 bytes apart,
    // share four: SQ_LDS_BANK_CONFLICT was a third of the LDS-array cycles)
    static_assert(GG_KQ == 8, "row interleave below assumes 8 lanes per tile row");
    const int s_slot = (tid >> 3) & 7;
    const int s_row = (tid >> 6) * 8 + (((s_slot & 1) << 2) | (s_slot >> 1)), s_kq = tid & 7;
    // Rows past the bucket end and columns past N are computed but never stored, so their
    // operands only have to be readable: clamp them to the last valid row / column instead
    // of predicating the loads.
    const float *a_src[NUA];
#pragma unroll
    for (int u = 0; u < NUA; u++) {
        const int p = min(row_lo + s_row + GG_RPP * u, row_hi - 1);
        const int src = g.gather ? g.gather[p] : p;
        a_src[u] = g.a + (size_t)src * g.lda;
    }
    const float *b_src[GG_NU];
#pragma unroll
    for (int u = 0; u < GG_NU; u++)
        b_src[u] = wg + (size_t)min(n0 + s_row + GG_RPP * u, g.N - 1) * g.ldn;
    const float *bn_src = wg + min(n0 + 4 * (tid & 31), g.N - 4);

    f32x16 acc[NI][2];
#pragma unroll
    for (int i = 0; i < NI; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;

    const int frow = lane & 31, fh = lane >> 5;
    // ---- fragments: lane l holds A[row = l & 31][k = 16 q2 + 8 (l >> 5) + 0..7] (16 bytes of a
    // k-contiguous image) and B likewise; `bt_image`: B tile stored [n][k] (k-contiguous weights
    // and the K extension), else [k][n], read with the transposing ds_read_b64_tr_b16 ----
    auto frag_rows = [&](const char *img, int row, int q2) {
        return *reinterpret_cast<const uint4 *>(img + row * GG_ROWB + 32 * q2 + 16 * fh);
    };
    auto frag_cols = [&](const char *img, int ncol0, int q2) {
        const int gl = lane & 15;
        const char *p = img + (16 * q2 + 8 * fh + (gl >> 2)) * GG_BNROWB +
                        (ncol0 + 16 * ((lane >> 4) & 1) + 4 * (gl & 3)) * 2;
        const uint2 lo = lds_tr_b64(p), hi = lds_tr_b64(p + 4 * GG_BNROWB);
        return make_uint4(lo.x, lo.y, hi.x, hi.y);
    };
    auto b_frag = [&](int part, int j, int q2, bool bt_image) {
        const char *img = Bs + part * GG_BIMG;
        return bt_image ? frag_rows(img, wn + 32 * j + frow, q2) : frag_cols(img, wn + 32 * j, q2);
    };
    // 16 k's, two-way split: three products
    auto mfma_group16 = [&](int q2, bool bt_image) {
        Frag af[NI], bf[2];
#pragma unroll
        for (int i = 0; i < NI; i++) {
            af[i].hi = frag_rows(As, wm + 32 * i + frow, q2);
            af[i].lo = frag_rows(As + GG_AIMG, wm + 32 * i + frow, q2);
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
            bf[j].hi = b_frag(0, j, q2, bt_image);
            bf[j].lo = b_frag(1, j, q2, bt_image);
        }
#pragma unroll
        for (int i = 0; i < NI; i++) {
            acc[i][0] = mm<2, 2>(af[i], bf[0], acc[i][0]);
            acc[i][1] = mm<2, 2>(af[i], bf[1], acc[i][1]);
        }
    };
    // ---- staging: four fp32 values -> the 8-byte pieces of both parts of an image ----
    auto put4 = [&](char *img, int part_stride, int off, const float4 &v) {
        const Split s0 = split2(v.x, v.y), s1 = split2(v.z, v.w);
        *reinterpret_cast<uint2 *>(img + off) = make_uint2(s0.hi, s1.hi);
        *reinterpret_cast<uint2 *>(img + part_stride + off) = make_uint2(s0.lo, s1.lo);
    };
    auto contract = [&](int kmax, bool bt_image) {        // k = 0 .. kmax of the staged tiles
        for (int q2 = 0; q2 < (kmax + 15) / 16; q2++) mfma_group16(q2, bt_image);
    };

    // ---- software pipeline: the global loads of k-step t+1 are in flight while the MFMAs
    // of step t run; registers -> LDS happens at the top of the next step ----
    float4 av[NUA], bv[GG_NU];
    // segments of K (a_seg_k > 0; the calls below visit k0 = 0, 32, 64 .. in order): the offset of
    // the current segment's matrix, less the k's that lie before it
    long long a_adj = 0;
    int seg_left = g.a_seg_k > 0 ? g.a_seg_k : 0x7FFFFFFF;
    // KTAIL == false (K % GG_BK == 0): no predicate anywhere in the loads.  The predicated
    // form compiles into branches around the loads, 8 per k-step.
    auto load_tile = [&](int k0) {
        const int k = k0 + 4 * s_kq;
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < NUA; u++) {
            if constexpr (KTAIL)
                av[u] = k < g.K ? *reinterpret_cast<const float4 *>(a_src[u] + a_adj + k) : zero;
            else
                av[u] = *reinterpret_cast<const float4 *>(a_src[u] + a_adj + k);
        }
        seg_left -= GG_BK;
        if (seg_left <= 0) { a_adj += g.a_seg_stride - g.a_seg_k; seg_left = g.a_seg_k; }
        if constexpr (!BN_LAYOUT) {
#pragma unroll
            for (int u = 0; u < GG_NU; u++) {
                if constexpr (KTAIL)
                    bv[u] = k < g.K ? *reinterpret_cast<const float4 *>(b_src[u] + k) : zero;
                else
                    bv[u] = *reinterpret_cast<const float4 *>(b_src[u] + k);
            }
        } else {
            // W_g(n, k), n contiguous: thread -> k row (tid >> 5) + 8 u, n-quad tid & 31
#pragma unroll
            for (int u = 0; u < GG_NU; u++) {
                const int kk = k0 + (tid >> 5) + GG_BNK * u;
                if constexpr (KTAIL)
                    bv[u] = kk < g.K ? *reinterpret_cast<const float4 *>(bn_src + (size_t)kk * g.ldk)
                                     : zero;
                else
                    bv[u] = *reinterpret_cast<const float4 *>(bn_src + (size_t)kk * g.ldk);
            }
        }
    };
    // registers -> LDS images (component-wise: a struct copy of av[u] keeps the whole array in
    // scratch memory)
    auto stage_store = [&]() {
#pragma unroll
        for (int u = 0; u < NUA; u++)
            put4(As, GG_AIMG, (s_row + GG_RPP * u) * GG_ROWB + 8 * s_kq,
                 make_float4(av[u].x, av[u].y, av[u].z, av[u].w));
        if (!BN_LAYOUT) {
#pragma unroll
            for (int u = 0; u < GG_NU; u++)
                put4(Bs, GG_BIMG, (s_row + GG_RPP * u) * GG_ROWB + 8 * s_kq,
                     make_float4(bv[u].x, bv[u].y, bv[u].z, bv[u].w));
        } else {
            // n-contiguous weights keep their orientation in LDS: Bs[k][n] (transposing them
            // into the [n][k] image needs 4-byte writes 4 rows apart: 16-way bank conflicts)
#pragma unroll
            for (int u = 0; u < GG_NU; u++)
                put4(Bs, GG_BIMG, ((tid >> 5) + GG_BNK * u) * GG_BNROWB + 8 * (tid & 31),
                     make_float4(bv[u].x, bv[u].y, bv[u].z, bv[u].w));
        }
    };
    if (g.K > 0) load_tile(0);
    for (int k0 = 0; k0 < g.K; k0 += GG_BK) {
        __syncthreads();  // previous tile fully consumed
        stage_store();
        __syncthreads();
        if (k0 + GG_BK < g.K) load_tile(k0 + GG_BK);     // the registers are free again
#pragma unroll
        for (int q2 = 0; q2 < GG_BK / 16; q2++) mfma_group16(q2, !BN_LAYOUT);
    }

    gg_scale_rows<NI>(g, acc, extras, wm);

    // ---- K extension on top: acc += A2 . B2_g^T, 32 columns of the two operands per k-step (zero
    // beyond R; R > 32 -- several rank-16 side products side by side -- only without the ReLU
    // epilogue, whose `extras` hold the norms of ONE step's rows) ----
    if (EXT) {
        for (int r0 = 0; r0 < g.R; r0 += GG_BK) {
            __syncthreads();              // the last k-step's tiles are consumed
            const int k = r0 + 4 * s_kq;
#pragma unroll
            for (int u = 0; u < NUA; u++) {
                const int r = s_row + GG_RPP * u;
                const int p = row_lo + r;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (p < row_hi && k < g.R) {
                    const int src = g.gather2 ? g.gather2[p] : p;
                    v = *reinterpret_cast<const float4 *>(g.a2 + (size_t)src * g.lda2 + k);
                }
                put4(As, GG_AIMG, r * GG_ROWB + 8 * s_kq, v);
                const float ss = group_sum<8>(v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w);
                if (s_kq == 0) extras[r] = ss;              // |a2 row|^2, for the epilogue
            }
#pragma unroll
            for (int u = 0; u < GG_NU; u++) {
                const int r = s_row + GG_RPP * u;
                const int n = n0 + r;
                float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
                if (n < g.N && k < g.R)
                    b = *reinterpret_cast<const float4 *>(
                        g.b2 + (size_t)bucket * g.b2_gstride + (size_t)n * g.b2_ldn +
                        (g.b2_seg ? (size_t)(k >> 4) * g.b2_seg + (k & 15) : (size_t)k));
                put4(Bs, GG_BIMG, r * GG_ROWB + 8 * s_kq, b);
                const float ss = group_sum<8>(b.x * b.x + b.y * b.y + b.z * b.z + b.w * b.w);
                if (s_kq == 0) extras[128 + r] = ss;        // |b2 row|^2
            }
            __syncthreads();
            contract(min(GG_BK, g.R - r0), true);
        }
    }
    __syncthreads();   // all waves are done with the operand tiles
    gg_epilogue<NI, EPI, false, false>(g, smem, acc, bucket, row_lo, row_hi, col_tile, wm, wn, extras, EXT);
}

template <bool BN_LAYOUT, int EPI, bool EXT, bool KTAIL>
__global__ __launch_bounds__(GG_THREADS, 2) void grouped_gemm_kernel(GroupedArgs g) {
    // A | B images (hi | lo each), then the ReLU epilogue's extras; the epilogue reuses the
    // images as four per-wave C staging areas
    static_assert(GG_REGS_LDS_FLOATS >= (GG_THREADS / 64) * 32 * (64 + 4), "");
    __shared__ __attribute__((aligned(16))) float smem[GG_REGS_LDS_FLOATS + GG_EXTRAS];
    const GgWork w = gg_find_work(g);
    if (w.bucket < 0) return;  // uniform for the workgroup
    if (w.half < 0)
        gemm_tile_regs<GG_BM, BN_LAYOUT, EPI, EXT, KTAIL>(g, smem, w.bucket, w.row_lo, w.row_hi, w.col_tile);
    else
        gemm_tile_regs<GG_BM / 2, BN_LAYOUT, EPI, EXT, KTAIL>(g, smem, w.bucket, w.row_lo, w.row_hi,
                                                             w.col_tile);
}

template <bool BN_LAYOUT, int EPI>
static GgKernel regs_kernel(bool ext, bool k_tail) {
    if (ext) return k_tail ? grouped_gemm_kernel<BN_LAYOUT, EPI, true, true> : grouped_gemm_kernel<BN_LAYOUT, EPI, true, false>;
    return k_tail ? grouped_gemm_kernel<BN_LAYOUT, EPI, false, true> : grouped_gemm_kernel<BN_LAYOUT, EPI, false, false>;
}
template <bool BN_LAYOUT>
static GgKernel regs_kernel(int epilogue, bool ext, bool k_tail) {
    return epilogue == EPI_PLAIN ? regs_kernel<BN_LAYOUT, EPI_PLAIN>(ext, k_tail)
           : epilogue == EPI_ACT ? regs_kernel<BN_LAYOUT, EPI_ACT>(ext, k_tail)
                                 : regs_kernel<BN_LAYOUT, EPI_DACT>(ext, k_tail);
}

int launch_gemm_regs(const GroupedArgs &g, int epilogue, bool ext, bool k_tail, dim3 grid, hipStream_t s) {
    const GgKernel kernel = g.ldk == 1 ? regs_kernel<false>(epilogue, ext, k_tail) : regs_kernel<true>(epilogue, ext, k_tail);
    hipLaunchKernelGGL(kernel, grid, dim3(GG_THREADS), 0, s, g);
    SPT_LAUNCH_CHECK();
    return SPT_OK;
}

}  // namespace spt
