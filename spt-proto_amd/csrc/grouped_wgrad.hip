// grouped_wgrad.hip -- the weight gradient of the grouped GEMM: spt_grouped_gemm_wgrad and
// spt_grouped_gemm_wgrad_bf16 (kernels, launcher and C entries; nothing of it lives elsewhere).
//
// out_g(n, k) = sum over the rows p of group g of rowscale[p] G[srcG(p), n] A[srcA(p), k]: the
// contraction runs over the bucket rows, whose number only the device knows.  Each group's rows are
// cut into chunks of `rc` rows, a function of the total row count alone (wgrad_rows_per_chunk: the
// split never depends on the CU count, the bucket sizes or timing); a workgroup forms one 128 (n) x 128 (k) tile of one chunk's product into the workspace and a second
// launch adds each group's chunks up in chunk order -- the partial-then-reduce form of
// tall_tn_partial_kernel / tall_tn_reduce_kernel, reproducible to the bit.
//
// Both operands are row-major in the contraction index p, i.e. n-contiguous: per 32-row step a
// thread loads four float4 of G and of A (a wave covers two 512-byte row segments), splits them into
// hi / lo bf16 on the way and writes them to LDS in the NC layout of the image path ([32 p][512 B],
// 64-byte segment 2 (col / 32) + part at segment ^ (p & 3)), from where gi_frag_nc's transposing
// ds_read_b64_tr_b16 hands the MFMA both fragments -- for v_mfma_f32_32x32x16_bf16 the A and B
// operand maps are the same map, so one reader serves G^T and A.  Three MFMAs per product as in
// spt_grouped_gemm: <= 2^-16 relative error per product, fp32 accumulation.  Register prefetch of
// the next step's rows while the current one is contracted, two LDS stages, one barrier per step.
#include "grouped_gemm.h"
#include "grouped_image.h"

namespace spt {

constexpr int WG_RC = 512;                       // rows per chunk at least
constexpr int WG_MAX_CHUNKS = 16;                // ... and chunks of all rows at most (+ one per group)
constexpr int WG_T = 128;                        // tile edge (n and k)
constexpr int WG_LDS_BYTES = 2 * 2 * 16384;      // two stages of G | A, 16 KiB each

struct WgradArgs {
    const float *g;           // [*, ldg] rows of G
    const float *a;           // [*, lda] rows of A
    const int32_t *gather_g;  // [P] or null
    const int32_t *gather_a;  // [P] or null
    const float *rowscale;    // [P] or null
    const int32_t *offsets;   // [G + 1]
    float *partial;           // [chunks][N][K]
    float *pbias;             // [chunks][N] or null (no dbias)
    float *out;
    float *dbias;
    long long ldg, lda, gstride, ldn;
    int G, N, K, ktiles, rc;
};

// chunk c -> (group, first row, rows); the groups' chunk ranges are consecutive (g = -1: none)
__device__ __forceinline__ void wg_chunk(const int32_t *offsets, int G, int rc, int c, int &g,
                                         int &row0, int &rows) {
    int base = 0;
    g = -1; row0 = 0; rows = 0;
    for (int i = 0; i < G; i++) {
        const int lo = offsets[i], hi = offsets[i + 1];
        const int nc = (hi - lo + rc - 1) / rc;
        if (g < 0 && c < base + nc) {
            g = i; row0 = lo + (c - base) * rc;
            rows = min(rc, hi - row0);
        }
        base += nc;
    }
}

// float4 of (row, col) -> hi / lo halves in the NC layout of stage tile `t`
__device__ __forceinline__ void wg_put(char *t, int r, int c4, float4 v) {
    const Split s0 = split2(v.x, v.y), s1 = split2(v.z, v.w);
    const int seg = 2 * (c4 >> 3), within = (c4 & 7) * 8;
    *reinterpret_cast<uint2 *>(t + r * 512 + (((seg + 0) ^ (r & 3)) << 6) + within) = make_uint2(s0.hi, s1.hi);
    *reinterpret_cast<uint2 *>(t + r * 512 + (((seg + 1) ^ (r & 3)) << 6) + within) = make_uint2(s0.lo, s1.lo);
}

// BF16 (spt_grouped_gemm_wgrad_bf16): g, a, out and dbias hold bf16.  The rows are widened on load and
// staged exactly as above: A's lo half is then zero and its product is left out (two MFMAs: G's hi and
// lo parts -- G's lo is nonzero only where a rowscale multiplied it); without a rowscale every product
// is that of the stored bf16 values, exactly
template <bool BF16>
__device__ __forceinline__ void wgrad_partial(WgradArgs w, char *smem) {
    int g, row0, rows;
    wg_chunk(w.offsets, w.G, w.rc, blockIdx.y, g, row0, rows);
    if (g < 0) return;                           // past the last chunk: nothing reads this slot
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nt = blockIdx.x / w.ktiles, kt = blockIdx.x - nt * w.ktiles;
    const int n0 = nt * WG_T, k0 = kt * WG_T;
    // staging map: float4 column c4 of rows rs + 8 j; a half-wave writes two rows of different
    // (r & 3) parity, i.e. both 64-byte bank halves: ds_write_b64 at its 2-way minimum
    const int c4 = (lane & 15) + 16 * (lane >> 5);
    const int rs = 2 * wave + ((lane >> 4) & 1);
    const bool g_ok = n0 + 4 * c4 < w.N, a_ok = k0 + 4 * c4 < w.K;
    const float *gp = w.g + n0 + 4 * c4;
    const float *ap = w.a + k0 + 4 * c4;
    const unsigned short *gpb = reinterpret_cast<const unsigned short *>(w.g) + n0 + 4 * c4;
    const unsigned short *apb = reinterpret_cast<const unsigned short *>(w.a) + k0 + 4 * c4;
    const bool want_bias = w.pbias && kt == 0;
    float4 bias_acc = make_float4(0.f, 0.f, 0.f, 0.f);
    // the source rows and scales of a step are fetched one step ahead of its data
    float4 vg[4], va[4];
    float sv[4], sn[4];
    int ig[4], ia[4];
    auto fetch_rows = [&](int p0) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int p = row0 + min(p0 + rs + 8 * j, rows - 1);     // (rows past the end: weight 0)
            ig[j] = w.gather_g ? w.gather_g[p] : p;
            ia[j] = w.gather_a ? w.gather_a[p] : p;
            sn[j] = w.rowscale ? w.rowscale[p] : 1.0f;
        }
    };
    auto load = [&](int p0) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool in = p0 + rs + 8 * j < rows;
            if constexpr (BF16) {
                vg[j] = in && g_ok ? gg_bf4(gpb + (long long)ig[j] * w.ldg) : make_float4(0.f, 0.f, 0.f, 0.f);
                va[j] = in && a_ok ? gg_bf4(apb + (long long)ia[j] * w.lda) : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                vg[j] = in && g_ok ? *reinterpret_cast<const float4 *>(gp + (long long)ig[j] * w.ldg)
                                   : make_float4(0.f, 0.f, 0.f, 0.f);
                va[j] = in && a_ok ? *reinterpret_cast<const float4 *>(ap + (long long)ia[j] * w.lda)
                                   : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            sv[j] = sn[j];
        }
    };
    // MFMA tiles: wave quadrant n wm .. wm + 63, k wn .. wn + 63
    const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64, fh = lane >> 5;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;
    const int steps = (rows + 31) / 32;
    fetch_rows(0);
    load(0);
    if (steps > 1) fetch_rows(32);
    for (int s = 0; s < steps; s++) {
        char *gs = smem + (s & 1) * 32768, *as = gs + 16384;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int r = rs + 8 * j;
            const float c = sv[j];
            const float4 x = make_float4(c * vg[j].x, c * vg[j].y, c * vg[j].z, c * vg[j].w);
            if (want_bias) {
                bias_acc.x += x.x; bias_acc.y += x.y; bias_acc.z += x.z; bias_acc.w += x.w;
            }
            wg_put(gs, r, c4, x);
            wg_put(as, r, c4, va[j]);
        }
        __syncthreads();
        if (s + 1 < steps) {
            load(32 * (s + 1));
            if (s + 2 < steps) fetch_rows(32 * (s + 2));
        }
#pragma unroll
        for (int q2 = 0; q2 < 2; q2++) {
            Frag fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; i++) {
                fa[i].hi = gi_frag_nc(gs, wm + 32 * i, q2, 0, fh, lane);
                fa[i].lo = gi_frag_nc(gs, wm + 32 * i, q2, 1, fh, lane);
                fb[i].hi = gi_frag_nc(as, wn + 32 * i, q2, 0, fh, lane);
                fb[i].lo = gi_frag_nc(as, wn + 32 * i, q2, 1, fh, lane);
            }
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    if constexpr (BF16) {
                        acc[i][j] = mma(fa[i].lo, fb[j].hi, acc[i][j]);
                        acc[i][j] = mma(fa[i].hi, fb[j].hi, acc[i][j]);
                    } else {
                        acc[i][j] = mm<2, 2>(fa[i], fb[j], acc[i][j]);
                    }
                }
        }
    }
    // acc[i][j][r] = C[n = wm + 32 i + (r & 3) + 8 (r >> 2) + 4 fh][k = wn + 32 j + (lane & 31)]
    float *pp = w.partial + (size_t)blockIdx.y * w.N * w.K;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int k = k0 + wn + 32 * j + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int n = n0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * fh;
                if (n < w.N && k < w.K) pp[(size_t)n * w.K + k] = acc[i][j][r];
            }
        }
    if (want_bias) {
        // the eight row classes of a column, added in order (fixed tree)
        __syncthreads();                         // the stages are free
        float4 *red = reinterpret_cast<float4 *>(smem);
        red[rs * 32 + c4] = bias_acc;
        __syncthreads();
        if (tid < 32 && n0 + 4 * tid < w.N) {
            float4 t = red[tid];
#pragma unroll
            for (int q = 1; q < 8; q++) {
                const float4 u = red[q * 32 + tid];
                t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
            }
            *reinterpret_cast<float4 *>(w.pbias + (size_t)blockIdx.y * w.N + n0 + 4 * tid) = t;
        }
    }
}

__global__ __launch_bounds__(256, 2) void wgrad_partial_kernel(WgradArgs w) {
    __shared__ __attribute__((aligned(16))) char smem[WG_LDS_BYTES];
    wgrad_partial<false>(w, smem);
}

__global__ __launch_bounds__(256, 2) void wgrad_partial_bf16_kernel(WgradArgs w) {
    __shared__ __attribute__((aligned(16))) char smem[WG_LDS_BYTES];
    wgrad_partial<true>(w, smem);
}

// out_g = the sum of group g's chunk partials in chunk order (zero for a group without rows);
// elements N K .. N K + N - 1 of the index space are dbias.  A thread per four elements.
template <bool BF16>
__device__ __forceinline__ void wgrad_reduce(WgradArgs w) {
    const int g = blockIdx.y;
    const long long nk = (long long)w.N * w.K;
    const long long e = 4 * ((long long)blockIdx.x * 256 + threadIdx.x);
    const bool bias = e >= nk;
    if (e >= nk + (w.pbias ? w.N : 0)) return;
    int first = 0;
    for (int i = 0; i < g; i++) first += (w.offsets[i + 1] - w.offsets[i] + w.rc - 1) / w.rc;
    const int count = (w.offsets[g + 1] - w.offsets[g] + w.rc - 1) / w.rc;
    const float *src = bias ? w.pbias + (size_t)first * w.N + (e - nk) : w.partial + (size_t)first * nk + e;
    const size_t step = bias ? (size_t)w.N : (size_t)nk;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    int c = 0;
    for (; c + 4 <= count; c += 4) {             // four loads in flight, added in chunk order
        float4 u[4];
#pragma unroll
        for (int i = 0; i < 4; i++) u[i] = *reinterpret_cast<const float4 *>(src + (size_t)(c + i) * step);
#pragma unroll
        for (int i = 0; i < 4; i++) { t.x += u[i].x; t.y += u[i].y; t.z += u[i].z; t.w += u[i].w; }
    }
    for (; c < count; c++) {
        const float4 u = *reinterpret_cast<const float4 *>(src + (size_t)c * step);
        t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
    }
    if (BF16) {         // the one rounding of the bf16 parameter layout
        const uint2 v = make_uint2(pack_bf16(t.x, t.y), pack_bf16(t.z, t.w));
        const long long n = e / w.K, k = e - n * w.K;
        unsigned short *dst = bias ? reinterpret_cast<unsigned short *>(w.dbias) + (size_t)g * w.N + (e - nk)
                                   : reinterpret_cast<unsigned short *>(w.out) + g * w.gstride + n * w.ldn + k;
        *reinterpret_cast<uint2 *>(dst) = v;
    } else if (bias) {
        *reinterpret_cast<float4 *>(w.dbias + (size_t)g * w.N + (e - nk)) = t;
    } else {
        const long long n = e / w.K, k = e - n * w.K;
        *reinterpret_cast<float4 *>(w.out + g * w.gstride + n * w.ldn + k) = t;
    }
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(WgradArgs w) { wgrad_reduce<false>(w); }
__global__ __launch_bounds__(256) void wgrad_reduce_bf16_kernel(WgradArgs w) { wgrad_reduce<true>(w); }

}  // namespace spt

using namespace spt;

// ---- spt_grouped_gemm_wgrad ----
// rows per chunk: WG_RC, doubled until all rows make at most WG_MAX_CHUNKS chunks (the partials'
// traffic stays a bounded share of the operands' at any length)
static long long wgrad_rows_per_chunk(long long n_rows) {
    long long rc = WG_RC;
    while ((n_rows + rc - 1) / rc > WG_MAX_CHUNKS) rc *= 2;
    return rc;
}
// chunks of all groups together: each group ends with at most one short chunk, so at most
// ceil(rows / rc) + n_groups whatever the bucket sizes -- and ceil(rows / rc) <= WG_MAX_CHUNKS, equal
// to ceil(rows / WG_RC) below that: the bound never shrinks for more rows
static long long wgrad_chunks(long long n_rows, int n_groups) {
    const long long c = (n_rows + WG_RC - 1) / WG_RC;
    return (c < WG_MAX_CHUNKS ? c : WG_MAX_CHUNKS) + n_groups;
}

extern "C" long long spt_grouped_gemm_wgrad_workspace_bytes(long long n_rows, int n_groups, int n, int k) {
    if (n_rows < 0 || n_groups <= 0 || n <= 0 || k <= 0) return 0;
    return wgrad_chunks(n_rows, n_groups) * ((long long)n * k + n) * (long long)sizeof(float);
}

// both element types: the validation, the chunking and the two launches are the same
static int launch_wgrad(bool bf16, const void *g, long long ldg, const int32_t *gather_g, const void *a,
                        long long lda, const int32_t *gather_a, const float *rowscale, const int32_t *offsets,
                        int n_groups, long long n_rows, int n, int k, void *out, long long group_stride,
                        long long ldn, void *dbias, void *workspace, void *stream) {
    if (!g || !a || !offsets || !out || !workspace) return SPT_EINVAL;
    if (n_groups < 1 || n_rows < 0 || n <= 0 || k <= 0 || ldg < n || lda < k || ldn < k || group_stride < 0)
        return SPT_EINVAL;
    if (n % 4 != 0 || k % 4 != 0 || ldg % 4 != 0 || lda % 4 != 0 || ldn % 4 != 0 || group_stride % 4 != 0)
        return SPT_ESHAPE;
    // four elements per access: 16 bytes of fp32, 8 of bf16; the fp32 partials in the workspace: 16
    const uintptr_t operands = reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(a) |
                               reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(dbias);
    if ((operands & (bf16 ? 7 : 15)) != 0 || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0)
        return SPT_ESHAPE;
    const long long chunks = wgrad_chunks(n_rows, n_groups);
    const long long tiles = (long long)((n + WG_T - 1) / WG_T) * ((k + WG_T - 1) / WG_T);
    if (n_rows > 0x7FFFFFFFll || chunks > 65535 || tiles > 0x7FFFFFFFll ||
        ((long long)n * k + n + 3) / 4 / 256 + 1 > 0x7FFFFFFFll)
        return SPT_EUNSUP;
    WgradArgs w = {};
    w.g = static_cast<const float *>(g); w.a = static_cast<const float *>(a);
    w.gather_g = gather_g; w.gather_a = gather_a; w.rowscale = rowscale;
    w.offsets = offsets; w.out = static_cast<float *>(out); w.dbias = static_cast<float *>(dbias);
    w.partial = static_cast<float *>(workspace);
    w.pbias = dbias ? w.partial + chunks * n * (long long)k : nullptr;
    w.ldg = ldg; w.lda = lda; w.gstride = group_stride; w.ldn = ldn;
    w.G = n_groups; w.N = n; w.K = k; w.ktiles = (k + WG_T - 1) / WG_T;
    w.rc = (int)wgrad_rows_per_chunk(n_rows);
    hipStream_t s = (hipStream_t)stream;
    if (n_rows > 0) {
        hipLaunchKernelGGL(bf16 ? wgrad_partial_bf16_kernel : wgrad_partial_kernel,
                           dim3((unsigned)tiles, (unsigned)chunks), dim3(256), 0, s, w);
        SPT_LAUNCH_CHECK();
    }
    const long long elems = (long long)n * k + (dbias ? n : 0);
    hipLaunchKernelGGL(bf16 ? wgrad_reduce_bf16_kernel : wgrad_reduce_kernel,
                       dim3((unsigned)((elems / 4 + 255) / 256), (unsigned)n_groups), dim3(256), 0, s, w);
    SPT_LAUNCH_CHECK();
    return SPT_OK;
}

extern "C" int spt_grouped_gemm_wgrad(const float *g, long long ldg, const int32_t *gather_g,
                                      const float *a, long long lda, const int32_t *gather_a,
                                      const float *rowscale, const int32_t *offsets, int n_groups,
                                      long long n_rows, int n, int k, float *out,
                                      long long group_stride, long long ldn, float *dbias,
                                      void *workspace, void *stream) {
    return launch_wgrad(false, g, ldg, gather_g, a, lda, gather_a, rowscale, offsets, n_groups, n_rows, n, k,
                        out, group_stride, ldn, dbias, workspace, stream);
}

// ---- the bf16 entries ----
// the partials stay fp32: the same workspace as spt_grouped_gemm_wgrad
extern "C" long long spt_grouped_gemm_wgrad_bf16_workspace_bytes(long long n_rows, int n_groups, int n, int k) {
    return spt_grouped_gemm_wgrad_workspace_bytes(n_rows, n_groups, n, k);
}

extern "C" int spt_grouped_gemm_wgrad_bf16(const void *g, long long ldg, const int32_t *gather_g,
                                           const void *a, long long lda, const int32_t *gather_a,
                                           const float *rowscale, const int32_t *offsets, int n_groups,
                                           long long n_rows, int n, int k, void *out,
                                           long long group_stride, long long ldn, void *dbias,
                                           void *workspace, void *stream) {
    return launch_wgrad(true, g, ldg, gather_g, a, lda, gather_a, rowscale, offsets, n_groups, n_rows, n, k,
                        out, group_stride, ldn, dbias, workspace, stream);
}
