// spmm.hip -- batched CSR x dense and CSR^T x dense for gfx950 (no hipSPARSE).
//
// Replaces extension/spmm.cpp:27-69 of the reference (cusparseSpMM, op = N or T).
//   N: y[b,r,:]             = sum_{p in row r} values[b,p] * x[b, indices[b,p], :]
//   T: y[b,indices[b,p],:] += values[b,p] * x[b, row(p), :]
//
// N is a row gather: see gather4.h (E = 64 / 128, X LDS-resident when S*E*4 <= 128 KiB)
// and sparse_rows.h (any other shape).
//
// T is a scatter.  cuSPARSE does it with global atomics; on MI355X global float atomics
// run at ~1.3 TB/s of added bytes (MI355X_MICROARCH "Global float atomics") and LDS
// float atomics (ds_add_f32) were measured here at ~3 cycles PER LANE (2.7 ms for the
// 256-slice BERT-large case, profiles/r01_run1_kernel_stats.csv) -- both far under the
// HBM stream this op should be bound by.  So T is turned into a gather:
//   1. csr_transpose_kernel: per batch, a counting sort of the entries by column builds
//      the transposed structure  t_ptr [S+1], t_row [nnz] (source row of each entry),
//      t_perm [nnz] (position of the entry's value in `values`).  Integer LDS atomics on
//      per-wave private cursors; a wave walks its rows in ascending order, so the
//      transposed order -- and therefore the fp32 summation order -- is reproducible.
//   2. the N gather kernels run on (t_ptr, t_row) with values fetched through t_perm.
// The structure depends only on `indices`: the backward of one attention layer needs it
// twice (grad_K, grad_V), spt_csr_transpose + spt_spmm_transposed let callers share it.
#include "gather4.h"
#include "sparse_rows.h"
#include "mfma_tiles.h"
#include <stdlib.h>

namespace spt {

constexpr int SP_THREADS = 256;
constexpr int SP_THREADS_LDS = 1024;
constexpr int TR_THREADS = 1024;
constexpr int TR_WAVES = TR_THREADS / SPT_WAVE;

// ------------------------------------------------------------------ generic N (any E % 4 == 0)

template <int LPE, bool PERM>
__device__ __forceinline__ void spmm_row(const int32_t *__restrict__ idx_b,
                                         const int32_t *__restrict__ perm_b,
                                         const float *__restrict__ val_b,
                                         const float *__restrict__ xbase,  // global or LDS
                                         float *__restrict__ yrow, const RowChunk &chunk,
                                         int E) {
    constexpr int EPS = SPT_WAVE / LPE;
    const int lane = lane_id();
    const int sub = lane & (LPE - 1);
    const int grp = lane / LPE;
    const bool sub_live = (4 * sub) < E;
    const float *xrow0 = xbase + 4 * sub;

    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int my_idx = chunk.idx;
    float my_val = chunk.val;  // 0 weight beyond the row end: padding adds nothing
    for (int p0 = chunk.start; p0 < chunk.end; p0 += SPT_WAVE) {
        const int remaining = chunk.end - p0;
        if (p0 != chunk.start) {
            const bool in = lane < remaining;
            my_idx = in ? idx_b[p0 + lane] : 0;
            if (PERM) my_val = in ? val_b[perm_b[p0 + lane]] : 0.0f;
            else my_val = in ? val_b[p0 + lane] : 0.0f;
        }
        auto step = [&](int s) {
            const int e = s * EPS + grp;
            const int col = __shfl(my_idx, e, SPT_WAVE);
            const float v = __shfl(my_val, e, SPT_WAVE);
            if (sub_live) {
                const float4 x4 = *reinterpret_cast<const float4 *>(xrow0 + (size_t)col * E);
                acc.x = fmaf(v, x4.x, acc.x);
                acc.y = fmaf(v, x4.y, acc.y);
                acc.z = fmaf(v, x4.z, acc.z);
                acc.w = fmaf(v, x4.w, acc.w);
            }
        };
        if (remaining >= SPT_WAVE) {
#pragma unroll
            for (int s = 0; s < LPE; s++) step(s);
        } else {
            const int nsteps = (remaining + EPS - 1) / EPS;
            for (int s = 0; s < nsteps; s++) step(s);
        }
    }
    // sum the EPS groups (lanes with equal `sub`): true xor exchanges
    if constexpr (LPE <= 1) { acc.x += butterfly_partner<1>(acc.x); acc.y += butterfly_partner<1>(acc.y); acc.z += butterfly_partner<1>(acc.z); acc.w += butterfly_partner<1>(acc.w); }
    if constexpr (LPE <= 2) { acc.x += butterfly_partner<2>(acc.x); acc.y += butterfly_partner<2>(acc.y); acc.z += butterfly_partner<2>(acc.z); acc.w += butterfly_partner<2>(acc.w); }
    if constexpr (LPE <= 4) { acc.x += __shfl_xor(acc.x, 4, SPT_WAVE); acc.y += __shfl_xor(acc.y, 4, SPT_WAVE); acc.z += __shfl_xor(acc.z, 4, SPT_WAVE); acc.w += __shfl_xor(acc.w, 4, SPT_WAVE); }
    if constexpr (LPE <= 8) { acc.x += __shfl_xor(acc.x, 8, SPT_WAVE); acc.y += __shfl_xor(acc.y, 8, SPT_WAVE); acc.z += __shfl_xor(acc.z, 8, SPT_WAVE); acc.w += __shfl_xor(acc.w, 8, SPT_WAVE); }
    if constexpr (LPE <= 16) { acc.x += butterfly_partner<16>(acc.x); acc.y += butterfly_partner<16>(acc.y); acc.z += butterfly_partner<16>(acc.z); acc.w += butterfly_partner<16>(acc.w); }
    if constexpr (LPE <= 32) { acc.x += butterfly_partner<32>(acc.x); acc.y += butterfly_partner<32>(acc.y); acc.z += butterfly_partner<32>(acc.z); acc.w += butterfly_partner<32>(acc.w); }
    if (grp == 0 && sub_live) *reinterpret_cast<float4 *>(yrow + 4 * sub) = acc;
}

template <int LPE, bool PERM>
__global__ __launch_bounds__(SP_THREADS) void spmm_generic_kernel(
    const int32_t *__restrict__ ptr, int ptr_stride, const int32_t *__restrict__ indices,
    const int32_t *__restrict__ perm, const float *__restrict__ values,
    const float *__restrict__ x, float *__restrict__ y, int B, int S, int E, int nnz,
    int tiles_per_batch, int rows_per_block) {
    const unsigned lid = xcd_remap(blockIdx.x, gridDim.x);
    const int b = lid / tiles_per_batch;
    const int tile = lid - b * tiles_per_batch;
    if (b >= B) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int row0 = tile * rows_per_block;
    const int row1 = min(S, row0 + rows_per_block);
    const int32_t *idx_b = indices + (size_t)b * nnz;
    const int32_t *perm_b = PERM ? perm + (size_t)b * nnz : nullptr;
    const float *val_b = values + (size_t)b * nnz;
    const float *xb = x + (size_t)b * S * E;
    float *y_b = y + (size_t)b * S * E;
    // in PERM mode the chunk prefetcher must not read `values` in CSR order: it fetches
    // ids only and the values are gathered through perm here
    for_each_row<!PERM>(ptr + (size_t)b * ptr_stride, idx_b, val_b, row0 + wave,
                        SP_THREADS / SPT_WAVE, row1, [](int) { return 0; },
                        [&](int row, const RowChunk &chunk, int) {
                            RowChunk c = chunk;
                            if (PERM) {
                                const int lane = lane_id();
                                c.val = (lane < c.end - c.start)
                                            ? val_b[perm_b[c.start + lane]] : 0.0f;
                            }
                            spmm_row<LPE, PERM>(idx_b, perm_b, val_b, xb,
                                                y_b + (size_t)row * E, c, E);
                        });
}

// ------------------------------------------------------------------ fast path (gather4.h)

template <int LPE, int MODE>
__global__ __launch_bounds__(SP_THREADS_LDS) void spmm_g4_lds_kernel(
    const int32_t *__restrict__ ptr, int ptr_stride, const int32_t *__restrict__ indices,
    const int32_t *__restrict__ perm, const float *__restrict__ values,
    const float *__restrict__ x, float *__restrict__ y, int S, int nnz, int splits,
    int x_heads, int y_heads) {
    constexpr int E = 16 * LPE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *xtile = reinterpret_cast<float *>(smem);  // [S][E]
    const int b = blockIdx.x / splits;
    const int part = blockIdx.x - b * splits;
    const int tid = threadIdx.x;
    const DenseView xv = dense_view(b, S, E, x_heads), yv = dense_view(b, S, E, y_heads);
    stage_rows(xtile, x + xv.base, xv.ld, S, E, tid, SP_THREADS_LDS);
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int NW = SP_THREADS_LDS / SPT_WAVE;
    gather_rows<LPE, MODE>(ptr + (size_t)b * ptr_stride, indices + (size_t)b * nnz,
                           MODE == G_SPMM_PERM ? perm + (size_t)b * nnz : nullptr,
                           values + (size_t)b * nnz, xtile, nullptr, y + yv.base,
                           part * NW + wave, splits * NW, S, 1.0f, 0.0f, E, yv.ld);
}

// values in transposed order: vt[b, j] = values[b, t_perm[b, j]].  One workgroup per batch;
// the batch's values (nnz * 4 <= 128 KiB) are staged in LDS with coalesced loads, so the
// random 4-byte reads hit LDS instead of L2 (where 32 batches x 128 KiB per XCD thrash:
// the gather through t_perm inside the product cost 2.6x the algorithmic HBM bytes).
__global__ __launch_bounds__(SP_THREADS_LDS) void permute_values_kernel(
    const int32_t *__restrict__ t_perm, const float *__restrict__ values,
    float *__restrict__ vt, int nnz) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *tile = reinterpret_cast<float *>(smem);
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    stage_tile(tile, values + (size_t)b * nnz, nnz >> 2, tid, SP_THREADS_LDS);
    for (int i = (nnz & ~3) + tid; i < nnz; i += SP_THREADS_LDS) tile[i] = values[(size_t)b * nnz + i];
    __syncthreads();
    const int4 *perm4 = reinterpret_cast<const int4 *>(t_perm + (size_t)b * nnz);
    float4 *out4 = reinterpret_cast<float4 *>(vt + (size_t)b * nnz);
    for (int i = tid; i < (nnz >> 2); i += SP_THREADS_LDS) {
        const int4 p = perm4[i];
        out4[i] = make_float4(tile[p.x], tile[p.y], tile[p.z], tile[p.w]);
    }
    for (int i = (nnz & ~3) + tid; i < nnz; i += SP_THREADS_LDS)
        vt[(size_t)b * nnz + i] = tile[t_perm[(size_t)b * nnz + i]];
}

// transposed product, E = 64, one workgroup per batch: dynamic, wide-row aware
// (gather_rows_dynamic).  The ticket word lives behind the tile in the dynamic region.
// MODE G_SPMM: `values` are already in transposed order (permute_values_kernel).
//
// Measured and dropped (MI355X, lookup-shaped patterns: row lengths of A^T are 0 .. ~480,
// one outlier of ~2400 = column 0 with lookup's padding, mean 64): processing the rows in
// length order with one QUAD per row and 16 entries per round (no cross-lane reduction,
// 172 rounds per slice instead of 252) -- 76 us against 74: a long row then is 20-30
// sequential, latency-bound rounds on one wave, and sending rows over 256 entries to the
// whole-wave mode leaves 32 of them to be processed one by one.  Length-sorting alone
// (same 4 x 64 mapping): +-0.
template <int MODE>
__global__ __launch_bounds__(SP_THREADS_LDS) void spmm_t64_lds_kernel(
    const int32_t *__restrict__ t_ptr, const int32_t *__restrict__ t_row,
    const int32_t *__restrict__ t_perm, const float *__restrict__ values,
    const float *__restrict__ x, float *__restrict__ y, int S, int nnz, int x_heads,
    int y_heads) {
    constexpr int E = 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *xtile = reinterpret_cast<float *>(smem);  // [S][E]
    int *ticket = reinterpret_cast<int *>(smem + (size_t)S * E * sizeof(float));
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    if (tid == 0) *ticket = 0;
    const DenseView xv = dense_view(b, S, E, x_heads), yv = dense_view(b, S, E, y_heads);
    stage_rows(xtile, x + xv.base, xv.ld, S, E, tid, SP_THREADS_LDS);
    __syncthreads();
    gather_rows_dynamic<MODE>(t_ptr + (size_t)b * (S + 1), t_row + (size_t)b * nnz,
                              MODE == G_SPMM_PERM ? t_perm + (size_t)b * nnz : nullptr,
                              values + (size_t)b * nnz, xtile, y + yv.base, ticket, S, yv.ld);
}

template <int LPE, int MODE>
__global__ __launch_bounds__(SP_THREADS) void spmm_g4_global_kernel(
    const int32_t *__restrict__ ptr, int ptr_stride, const int32_t *__restrict__ indices,
    const int32_t *__restrict__ perm, const float *__restrict__ values,
    const float *__restrict__ x, float *__restrict__ y, int B, int S, int nnz,
    int blocks_per_batch) {
    constexpr int E = 16 * LPE;
    const unsigned lid = xcd_remap(blockIdx.x, gridDim.x);
    const int b = lid / blocks_per_batch;
    const int part = lid - b * blocks_per_batch;
    if (b >= B) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int NW = SP_THREADS / SPT_WAVE;
    gather_rows<LPE, MODE>(ptr + (size_t)b * ptr_stride, indices + (size_t)b * nnz,
                           MODE == G_SPMM_PERM ? perm + (size_t)b * nnz : nullptr,
                           values + (size_t)b * nnz, x + (size_t)b * S * E, nullptr,
                           y + (size_t)b * S * E, part * NW + wave, blocks_per_batch * NW, S,
                           1.0f, 0.0f);
}

// ------------------------------------------------------------------ CSR transpose

// One block per batch.  wcnt[w][c] = entries of column c in the rows owned by wave w
// (waves own contiguous row ranges).  After a scan over (c, w) each wave has private
// cursors, walks its rows in ascending order and places entries with ds_add_rtn_u32.
// When 16*S ints do not fit LDS a single shared cursor array is used (order then
// depends on wave timing).
template <bool PRIVATE>
__global__ __launch_bounds__(TR_THREADS) void csr_transpose_kernel(
    const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
    int32_t *__restrict__ t_ptr, int32_t *__restrict__ t_row, int32_t *__restrict__ t_perm,
    int S, int nnz) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *wave_tot = reinterpret_cast<int *>(smem);  // [TR_WAVES]
    int *wcnt = wave_tot + TR_WAVES;                // [PRIVATE ? TR_WAVES : 1][S]
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int NC = PRIVATE ? TR_WAVES : 1;
    const int32_t *idx_b = indices + (size_t)b * nnz;

    for (int i = tid; i < NC * S; i += TR_THREADS) wcnt[i] = 0;
    __syncthreads();

    // contiguous row range of this wave = contiguous entry range [p_lo, p_hi)
    const int rows_per_wave = (S + TR_WAVES - 1) / TR_WAVES;
    const int r0 = min(S, wave * rows_per_wave);
    const int r1 = min(S, r0 + rows_per_wave);
    const int p_lo = indptr[r0], p_hi = indptr[r1];
    int *mycnt = wcnt + (PRIVATE ? wave * S : 0);
    constexpr int KB = 16;  // 64-entry chunks whose loads are kept in flight together

    // ---- 1. histogram ----
    for (int base = p_lo; base < p_hi; base += KB * SPT_WAVE) {
        int cols[KB];
#pragma unroll
        for (int i = 0; i < KB; i++) {
            const int p = base + i * SPT_WAVE + lane;
            cols[i] = (p < p_hi) ? idx_b[p] : -1;
        }
#pragma unroll
        for (int i = 0; i < KB; i++)
            if (cols[i] >= 0) atomicAdd(&mycnt[cols[i]], 1);
    }
    __syncthreads();

    // ---- 2. exclusive scan over (column major, wave minor) ----
    // thread tid owns columns [c0, c1); its total, then a block scan of the totals
    const int cols_per_thread = (S + TR_THREADS - 1) / TR_THREADS;
    const int c0 = min(S, tid * cols_per_thread);
    const int c1 = min(S, c0 + cols_per_thread);
    int mine = 0;
    for (int c = c0; c < c1; c++)
        for (int w = 0; w < NC; w++) mine += wcnt[w * S + c];
    int inc = mine;  // wave inclusive scan
#pragma unroll
    for (int d = 1; d < SPT_WAVE; d <<= 1) {
        const int o = __shfl_up(inc, d, SPT_WAVE);
        if (lane >= d) inc += o;
    }
    if (lane == SPT_WAVE - 1) wave_tot[wave] = inc;
    __syncthreads();
    int base_pos = 0;
    for (int w = 0; w < wave; w++) base_pos += wave_tot[w];
    int run = base_pos + inc - mine;  // first position of column c0
    int32_t *tp = t_ptr + (size_t)b * (S + 1);
    for (int c = c0; c < c1; c++) {
        tp[c] = run;
        for (int w = 0; w < NC; w++) {
            const int n = wcnt[w * S + c];
            wcnt[w * S + c] = run;  // becomes the cursor of (wave w, column c)
            run += n;
        }
    }
    if (tid == TR_THREADS - 1) tp[S] = nnz;
    __syncthreads();

    // ---- 3. placement: entries in ascending order per wave ----
    int32_t *trow = t_row + (size_t)b * nnz;
    int32_t *tperm = t_perm + (size_t)b * nnz;
    int r = r0;  // row of this lane's current entry (entries only move forward)
    for (int base = p_lo; base < p_hi; base += KB * SPT_WAVE) {
        int cols[KB];
#pragma unroll
        for (int i = 0; i < KB; i++) {
            const int p = base + i * SPT_WAVE + lane;
            cols[i] = (p < p_hi) ? idx_b[p] : -1;
        }
#pragma unroll
        for (int i = 0; i < KB; i++) {
            const int p = base + i * SPT_WAVE + lane;
            if (cols[i] >= 0) {
                while (indptr[r + 1] <= p) r++;
                const int pos = atomicAdd(&mycnt[cols[i]], 1);
                trow[pos] = r;
                tperm[pos] = p;
            }
        }
    }
}

// ------------------------------------------------------------------ CSR transpose, bitmap form
//
// LDS atomics are the bottleneck of the counting sort above (measured ~7 cycles per lane,
// 212 us for 256 slices of 32768 entries).  For S <= 768 the (row, column) incidence
// matrix fits LDS as a bitmap, and the position of a DISTINCT entry needs no atomic:
//     pos(r, c) = start[c] + #{ r' < r : c in row r' }
//               = start[c] + cum[c][r / 32] + popcount(MT[c][r / 32] & lowbits(r % 32))
// MT[c][w] holds the bits of rows 32w .. 32w+31 for column c and is written only by the
// wave that owns those 32 rows (plain read-or-write, no atomics, no races).  Entries that
// repeat a (row, column) pair already seen in their row -- in the attention path only
// lookup's column-0 padding of rows < Z-1 -- are appended behind the column's distinct
// entries through a cursor (LDS atomic with return; rare).  The distinct part of every
// column is therefore in ascending row order, reproducibly; only the relative order of
// duplicate entries depends on wave timing.
__global__ __launch_bounds__(TR_THREADS) void csr_transpose_bitmap_kernel(
    const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
    int32_t *__restrict__ t_ptr, int32_t *__restrict__ t_row, int32_t *__restrict__ t_perm,
    int S, int nnz, int fb_words) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int W = (S + 31) >> 5;                                   // 32-row words per column
    // all carve offsets are multiples of 8 bytes (sizes rounded by the host the same way)
    uint32_t *MT = reinterpret_cast<uint32_t *>(smem);             // [S][W] incidence bits
    unsigned long long *firstbits =
        reinterpret_cast<unsigned long long *>(MT + (((size_t)S * W + 1) & ~(size_t)1));
    int *colstart = reinterpret_cast<int *>(firstbits + fb_words);  // [S]
    int *dupcur = colstart + S;                                    // [S] count, then cursor
    int *rowptr = dupcur + S;                                      // [S + 1] copy of indptr
    int *wave_tot = rowptr + ((S + 2) & ~1);                       // [TR_WAVES]
    int *wave_chunks = wave_tot + TR_WAVES;                        // [TR_WAVES]
    uint16_t *cum = reinterpret_cast<uint16_t *>(wave_chunks + TR_WAVES);      // [S][W]
    uint16_t *stage = cum + (((size_t)S * W + 3) & ~(size_t)3);    // [nnz] entry id by position
    uint8_t *scratch_all = reinterpret_cast<uint8_t *>(stage + (((size_t)nnz + 3) & ~(size_t)3));

    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int32_t *idx_b = indices + (size_t)b * nnz;
    uint8_t *scratch = scratch_all + (size_t)wave * S;   // "who saw this column first" bytes

    for (int i = tid; i < S * W; i += TR_THREADS) MT[i] = 0u;
    for (int i = tid; i < S; i += TR_THREADS) dupcur[i] = 0;
    for (int i = tid; i <= S; i += TR_THREADS) rowptr[i] = indptr[i];
    __syncthreads();

    // rows of this wave: 32-row words wave, wave + TR_WAVES, ...
    // how many 64-entry chunks will this wave visit?  (offset of its ballot words)
    int my_chunks = 0;
    for (int wi = wave; wi < W; wi += TR_WAVES) {
        const int r = 32 * wi + (lane & 31);
        int n = 0;
        if (lane < 32 && r < S) n = (rowptr[r + 1] - rowptr[r] + 63) >> 6;
#pragma unroll
        for (int d = 1; d < 32; d <<= 1) n += __shfl_xor(n, d, SPT_WAVE);
        my_chunks += __builtin_amdgcn_readlane(n, 0);
    }
    if (lane == 0) wave_chunks[wave] = my_chunks;
    __syncthreads();
    int fb_base = 0;
    for (int w = 0; w < wave; w++) fb_base += wave_chunks[w];
    unsigned long long *myfb = firstbits + fb_base;

    // the first 64 column ids of the NEXT row are requested before the current row is
    // processed: the serial walk over rows is otherwise bound by HBM latency per row
    auto first_chunk = [&](int r) {
        int v = 0;
        if (r < S) {
            const int st = rowptr[r], en = rowptr[r + 1];
            if (st + lane < en) v = idx_b[st + lane];
        }
        return v;
    };

    // ---- A. bitmap of distinct entries, count of duplicates ----
    int chunk_no = 0;
    for (int wi = wave; wi < W; wi += TR_WAVES) {
        int ncol = first_chunk(32 * wi);
        for (int rr = 0; rr < 32; rr++) {
            const int r = 32 * wi + rr;
            if (r >= S) break;
            const int start = rowptr[r], end = rowptr[r + 1];
            const int col0 = ncol;
            if (rr + 1 < 32) ncol = first_chunk(r + 1);
            for (int p0 = start; p0 < end; p0 += SPT_WAVE, chunk_no++) {
                const int p = p0 + lane;
                const bool live = p < end;
                const int col = (p0 == start) ? col0 : (live ? idx_b[p] : 0);
                // first occurrence within the row?  a later 64-entry chunk of the same row
                // must also lose against earlier chunks: test the bitmap bit first
                bool first = false;
                if (live) {
                    const bool seen = (MT[(size_t)col * W + wi] >> rr) & 1u;
                    if (!seen) scratch[col] = (uint8_t)lane;
                }
                __builtin_amdgcn_wave_barrier();
                if (live) {
                    const bool seen = (MT[(size_t)col * W + wi] >> rr) & 1u;
                    first = !seen && scratch[col] == (uint8_t)lane;
                    if (first) MT[(size_t)col * W + wi] |= (1u << rr);
                    else atomicAdd(&dupcur[col], 1);
                }
                const unsigned long long fb = __ballot(first);
                if (lane == 0) myfb[chunk_no] = fb;
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    __syncthreads();

    // ---- B. per column: prefix over words, totals, block scan -> column starts ----
    const int cols_per_thread = (S + TR_THREADS - 1) / TR_THREADS;
    const int c0 = min(S, tid * cols_per_thread);
    const int c1 = min(S, c0 + cols_per_thread);
    int mine = 0;
    for (int c = c0; c < c1; c++) {
        int runc = 0;
        for (int w = 0; w < W; w++) {
            cum[(size_t)c * W + w] = (uint16_t)runc;
            runc += __popc(MT[(size_t)c * W + w]);
        }
        colstart[c] = runc;            // distinct entries, for now
        mine += runc + dupcur[c];
    }
    int inc = mine;
#pragma unroll
    for (int d = 1; d < SPT_WAVE; d <<= 1) {
        const int o = __shfl_up(inc, d, SPT_WAVE);
        if (lane >= d) inc += o;
    }
    if (lane == SPT_WAVE - 1) wave_tot[wave] = inc;
    __syncthreads();
    int base_pos = 0;
    for (int w = 0; w < wave; w++) base_pos += wave_tot[w];
    int run = base_pos + inc - mine;
    int32_t *tp = t_ptr + (size_t)b * (S + 1);
    for (int c = c0; c < c1; c++) {
        const int distinct = colstart[c], dups = dupcur[c];
        tp[c] = run;
        colstart[c] = run;
        dupcur[c] = run + distinct;    // duplicates go behind the distinct entries
        run += distinct + dups;
    }
    if (tid == TR_THREADS - 1) tp[S] = nnz;
    __syncthreads();

    // ---- C. placement into the LDS stage (entry id by transposed position) ----
    chunk_no = 0;
    for (int wi = wave; wi < W; wi += TR_WAVES) {
        int ncol = first_chunk(32 * wi);
        for (int rr = 0; rr < 32; rr++) {
            const int r = 32 * wi + rr;
            if (r >= S) break;
            const int start = rowptr[r], end = rowptr[r + 1];
            const int col0 = ncol;
            if (rr + 1 < 32) ncol = first_chunk(r + 1);
            for (int p0 = start; p0 < end; p0 += SPT_WAVE, chunk_no++) {
                const int p = p0 + lane;
                if (p < end) {
                    const int col = (p0 == start) ? col0 : idx_b[p];
                    const unsigned long long fb = myfb[chunk_no];
                    int pos;
                    if ((fb >> lane) & 1ull) {
                        const uint32_t below = MT[(size_t)col * W + wi] & ((1u << rr) - 1u);
                        pos = colstart[col] + (int)cum[(size_t)col * W + wi] + __popc(below);
                    } else {
                        pos = atomicAdd(&dupcur[col], 1);
                    }
                    stage[pos] = (uint16_t)p;
                }
            }
        }
    }
    __syncthreads();

    // ---- D. coalesced write-out; the source row of entry p by binary search in rowptr ----
    int32_t *trow = t_row + (size_t)b * nnz;
    int32_t *tperm = t_perm + (size_t)b * nnz;
    for (int pos = tid; pos < nnz; pos += TR_THREADS) {
        const int p = stage[pos];
        int lo = 0, hi = S;            // largest r with rowptr[r] <= p
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (rowptr[mid] <= p) lo = mid;
            else hi = mid;
        }
        tperm[pos] = p;
        trow[pos] = lo;
    }
}

// ------------------------------------------------------------------ long sequences: chunked form
//
// S > 512 at E = 64: a slice of x (S x 256 bytes) no longer fits LDS, and the gather over
// the whole transposed structure reads 256-byte rows at random from a 512 KiB..2 MiB window per
// slice (33.5 M row reads per launch at S = 2048, B = 64: they miss L2; 2.3 ms measured), while the
// LDS counting sort above runs B workgroups on 256 CUs (2.2 ms).  The transposed structure is
// therefore built per ROW CHUNK of 512 rows: A = [A_0; A_1; ...], A^T x = sum_j A_j^T x_j, and
// each A_j^T x_j is the S = 512 problem again -- x_j (128 KiB) in LDS, one workgroup per
// (slice, chunk), 4 x as many workgroups -- producing S output rows that a last pass adds up
// (only chunks j >= c / 512 reach column c: the pattern is causal in practice, but nothing here
// relies on it).  The transposition is a three-launch counting sort over (slice, chunk,
// 128-row quarter) workgroups: count per column, prefix over quarters and columns, place.
// Entries of one (column, quarter) are placed through an LDS cursor: their order depends on
// wave timing (as the reference's atomic cuSPARSE path), the order across quarters is by row.
constexpr int CH_ROWS = 512;      // rows of x per chunk = one LDS tile at E = 64
constexpr int CH_QUARTERS = 4;    // counting-sort workgroups per chunk
constexpr int CH_QROWS = CH_ROWS / CH_QUARTERS;

__global__ __launch_bounds__(TR_THREADS) void chunk_count_kernel(
    const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
    int32_t *__restrict__ counts, int S, int nnz, int nchunks) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *hist = reinterpret_cast<int *>(smem);            // [S]
    const int q = blockIdx.x % CH_QUARTERS;
    const int bj = blockIdx.x / CH_QUARTERS;              // b * nchunks + j
    const int b = bj / nchunks, j = bj - b * nchunks;
    const int r0 = j * CH_ROWS + q * CH_QROWS;
    for (int i = threadIdx.x; i < S; i += TR_THREADS) hist[i] = 0;
    __syncthreads();
    const int e0 = indptr[r0], e1 = indptr[min(S, r0 + CH_QROWS)];
    const int32_t *idx_b = indices + (size_t)b * nnz;
    for (int e = e0 + threadIdx.x; e < e1; e += TR_THREADS) atomicAdd(&hist[idx_b[e]], 1);
    __syncthreads();
    int32_t *dst = counts + (size_t)blockIdx.x * S;
    for (int i = threadIdx.x; i < S; i += TR_THREADS) dst[i] = hist[i];
}

// counts[bj][q][c] -> first position of (c, q) inside the chunk's transposed arrays; t_ptr
__global__ __launch_bounds__(TR_THREADS) void chunk_scan_kernel(int32_t *__restrict__ counts,
                                                                int32_t *__restrict__ t_ptr,
                                                                int S) {
    __shared__ int wave_tot[TR_WAVES];
    const int bj = blockIdx.x;
    int32_t *cq = counts + (size_t)bj * CH_QUARTERS * S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cpt = (S + TR_THREADS - 1) / TR_THREADS;    // columns per thread
    const int c0 = min(S, tid * cpt), c1 = min(S, c0 + cpt);
    int mine = 0;
    for (int c = c0; c < c1; c++)
#pragma unroll
        for (int q = 0; q < CH_QUARTERS; q++) mine += cq[(size_t)q * S + c];
    int inc = mine;
#pragma unroll
    for (int d = 1; d < SPT_WAVE; d <<= 1) {
        const int o = __shfl_up(inc, d, SPT_WAVE);
        if (lane >= d) inc += o;
    }
    if (lane == SPT_WAVE - 1) wave_tot[wave] = inc;
    __syncthreads();
    int run = inc - mine;
    for (int w = 0; w < wave; w++) run += wave_tot[w];
    int32_t *tp = t_ptr + (size_t)bj * (S + 1);
    for (int c = c0; c < c1; c++) {
        tp[c] = run;
#pragma unroll
        for (int q = 0; q < CH_QUARTERS; q++) {
            const int n = cq[(size_t)q * S + c];
            cq[(size_t)q * S + c] = run;
            run += n;
        }
    }
    if (tid == TR_THREADS - 1) tp[S] = run;
}

__global__ __launch_bounds__(TR_THREADS) void chunk_place_kernel(
    const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
    const int32_t *__restrict__ base, int32_t *__restrict__ t_row, int32_t *__restrict__ t_perm,
    int S, int nnz, int nchunks) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *cursor = reinterpret_cast<int *>(smem);          // [S]
    const int q = blockIdx.x % CH_QUARTERS;
    const int bj = blockIdx.x / CH_QUARTERS;
    const int b = bj / nchunks, j = bj - b * nchunks;
    const int r0 = j * CH_ROWS + q * CH_QROWS;
    const int32_t *mybase = base + (size_t)blockIdx.x * S;
    for (int i = threadIdx.x; i < S; i += TR_THREADS) cursor[i] = mybase[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t *idx_b = indices + (size_t)b * nnz;
    const size_t out0 = (size_t)b * nnz + indptr[j * CH_ROWS];     // the chunk's entry range
    for (int r = r0 + wave; r < min(S, r0 + CH_QROWS); r += TR_WAVES) {
        const int st = indptr[r], en = indptr[r + 1];
        for (int e = st + lane; e < en; e += SPT_WAVE) {
            const int pos = atomicAdd(&cursor[idx_b[e]], 1);
            t_row[out0 + pos] = r - j * CH_ROWS;           // row inside the chunk's x tile
            t_perm[out0 + pos] = e;                        // position in the slice's values
        }
    }
}

// One (slice, chunk): partial[j][b] = A_j^T x_j, all S rows (zeros where the chunk has nothing).
__global__ __launch_bounds__(SP_THREADS_LDS) void spmm_t64_chunk_kernel(
    const int32_t *__restrict__ indptr, const int32_t *__restrict__ t_ptr,
    const int32_t *__restrict__ t_row, const int32_t *__restrict__ t_perm,
    const float *__restrict__ values, const float *__restrict__ x, float *__restrict__ partial,
    int B, int S, int nnz, int nchunks, int x_heads) {
    constexpr int E = 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *xtile = reinterpret_cast<float *>(smem);       // [CH_ROWS][E]
    int *ticket = reinterpret_cast<int *>(smem + (size_t)CH_ROWS * E * sizeof(float));
    const int bj = blockIdx.x;
    const int b = bj / nchunks, j = bj - b * nchunks;
    const int tid = threadIdx.x;
    if (tid == 0) *ticket = 0;
    const DenseView xv = dense_view(b, S, E, x_heads);
    stage_rows(xtile, x + xv.base + (size_t)j * CH_ROWS * xv.ld, xv.ld, CH_ROWS, E, tid,
               SP_THREADS_LDS);
    __syncthreads();
    const size_t e0 = (size_t)b * nnz + indptr[j * CH_ROWS];
    gather_rows_dynamic<G_SPMM_PERM>(t_ptr + (size_t)bj * (S + 1), t_row + e0, t_perm + e0,
                                     values + (size_t)b * nnz, xtile,
                                     partial + ((size_t)j * B + b) * S * E, ticket, S, E);
}

// y[b][c] = sum over chunks of partial[j][b][c]
__global__ __launch_bounds__(256) void chunk_reduce_kernel(const float *__restrict__ partial,
                                                           float *__restrict__ y, int B, int S,
                                                           int nchunks, int y_heads) {
    constexpr int E = 64;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;     // float4 index
    const long long total = (long long)B * S * (E / 4);
    if (i >= total) return;
    const int c4 = (int)(i % (E / 4));
    const long long row = i / (E / 4);
    const int b = (int)(row / S), c = (int)(row - (long long)b * S);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < nchunks; j++) {
        const float4 v = *reinterpret_cast<const float4 *>(
            partial + (((size_t)j * B + b) * S + c) * E + 4 * c4);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    const DenseView yv = dense_view(b, S, E, y_heads);
    *reinterpret_cast<float4 *>(y + yv.base + (size_t)c * yv.ld + 4 * c4) = acc;
}

// ------------------------------------------------------------------ host side

struct TransposedCsr {
    int32_t *t_ptr, *t_row, *t_perm, *counts;
};

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Which form does the product kernel for this head size want?
static bool chunked_layout(int S, int E) {
    return E == 64 && S > CH_ROWS && S % CH_ROWS == 0 && S <= 16384;
}

static int64_t transpose_bytes(int B, int S, int nnz, int E) {
    if (chunked_layout(S, E)) {
        const size_t nch = (size_t)S / CH_ROWS;
        return (int64_t)(align256((size_t)B * nch * (S + 1) * 4) + 2 * align256((size_t)B * nnz * 4) +
                         align256((size_t)B * nch * CH_QUARTERS * S * 4));
    }
    return (int64_t)(align256((size_t)B * (S + 1) * 4) + 2 * align256((size_t)B * nnz * 4));
}

static TransposedCsr carve(void *workspace, int B, int S, int nnz, int E = 0) {
    char *p = reinterpret_cast<char *>(workspace);
    const size_t nch = chunked_layout(S, E) ? (size_t)S / CH_ROWS : 1;
    TransposedCsr t;
    t.t_ptr = reinterpret_cast<int32_t *>(p);
    p += align256((size_t)B * nch * (S + 1) * 4);
    t.t_row = reinterpret_cast<int32_t *>(p);
    p += align256((size_t)B * nnz * 4);
    t.t_perm = reinterpret_cast<int32_t *>(p);
    p += align256((size_t)B * nnz * 4);
    t.counts = reinterpret_cast<int32_t *>(p);      // chunked form only
    return t;
}

static int launch_transpose_chunked(const int32_t *indptr, const int32_t *indices,
                                    TransposedCsr t, int B, int S, int nnz, hipStream_t s) {
    const int nch = S / CH_ROWS;
    const size_t lds = (size_t)S * sizeof(int);
    const unsigned nq = (unsigned)((size_t)B * nch * CH_QUARTERS);
    hipLaunchKernelGGL(chunk_count_kernel, dim3(nq), dim3(TR_THREADS), lds, s, indptr, indices,
                       t.counts, S, nnz, nch);
    SPT_LAUNCH_CHECK();
    hipLaunchKernelGGL(chunk_scan_kernel, dim3((unsigned)(B * nch)), dim3(TR_THREADS), 0, s,
                       t.counts, t.t_ptr, S);
    SPT_LAUNCH_CHECK();
    hipLaunchKernelGGL(chunk_place_kernel, dim3(nq), dim3(TR_THREADS), lds, s, indptr, indices,
                       t.counts, t.t_row, t.t_perm, S, nnz, nch);
    SPT_LAUNCH_CHECK();
    return SPT_OK;
}

static int launch_transpose(const int32_t *indptr, const int32_t *indices, TransposedCsr t,
                            int B, int S, int nnz, hipStream_t s) {
    // bitmap form (LDS carve must match csr_transpose_bitmap_kernel)
    if (nnz <= 65536) {
        const size_t W = (size_t)(S + 31) / 32;
        const size_t fb_words = ((size_t)nnz + 63) / 64 + (size_t)S;   // >= chunks visited
        size_t need = (((size_t)S * W + 1) & ~(size_t)1) * 4;          // MT
        need += fb_words * 8;                                          // firstbits
        need += 2 * (size_t)S * 4;                                     // colstart, dupcur
        need += (((size_t)S + 2) & ~(size_t)1) * 4;                    // rowptr
        need += 2 * (size_t)TR_WAVES * 4;                              // wave_tot, wave_chunks
        need += (((size_t)S * W + 3) & ~(size_t)3) * 2;                // cum
        need += (((size_t)nnz + 3) & ~(size_t)3) * 2;                  // stage
        need += (size_t)TR_WAVES * S;                                  // scratch
        if (need <= 158 * 1024) {
            SPT_HIP_TRY(hipFuncSetAttribute(
                reinterpret_cast<const void *>(&csr_transpose_bitmap_kernel),
                hipFuncAttributeMaxDynamicSharedMemorySize, (int)need));
            hipLaunchKernelGGL(csr_transpose_bitmap_kernel, dim3(B), dim3(TR_THREADS), need, s,
                               indptr, indices, t.t_ptr, t.t_row, t.t_perm, S, nnz,
                               (int)fb_words);
            SPT_LAUNCH_CHECK();
            return SPT_OK;
        }
    }
    const size_t head = TR_WAVES * sizeof(int);
    const size_t priv = head + (size_t)TR_WAVES * S * sizeof(int);
    const size_t shared = head + (size_t)S * sizeof(int);
    if (priv <= 144 * 1024) {
        SPT_HIP_TRY(hipFuncSetAttribute(
            reinterpret_cast<const void *>(&csr_transpose_kernel<true>),
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)priv));
        hipLaunchKernelGGL((csr_transpose_kernel<true>), dim3(B), dim3(TR_THREADS), priv, s,
                           indptr, indices, t.t_ptr, t.t_row, t.t_perm, S, nnz);
    } else {
        if (shared > 144 * 1024) return SPT_EUNSUP;
        SPT_HIP_TRY(hipFuncSetAttribute(
            reinterpret_cast<const void *>(&csr_transpose_kernel<false>),
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)shared));
        hipLaunchKernelGGL((csr_transpose_kernel<false>), dim3(B), dim3(TR_THREADS), shared, s,
                           indptr, indices, t.t_ptr, t.t_row, t.t_perm, S, nnz);
    }
    SPT_LAUNCH_CHECK();
    return SPT_OK;
}

// y = A . x on the structure (ptr, indices); PERM: values are fetched through `perm`
template <bool PERM>
static int launch_gather(const int32_t *ptr, int ptr_stride, const int32_t *indices,
                         const int32_t *perm, const float *values, const float *x, float *y,
                         int B, int S, int E, int nnz, int x_heads, int y_heads, hipStream_t s,
                         float *vt_scratch = nullptr) {
    constexpr int MODE = PERM ? G_SPMM_PERM : G_SPMM;
    if (x_heads < 0 || y_heads < 0) return SPT_EINVAL;
    if ((x_heads > 0 && B % x_heads != 0) || (y_heads > 0 && B % y_heads != 0)) return SPT_ESHAPE;
    const bool strided = x_heads > 0 || y_heads > 0;
    const size_t tile_bytes = (size_t)S * E * sizeof(float);
    if (PERM && E == 64 && tile_bytes <= 128 * 1024 && B >= 128) {
        const size_t lds_bytes = tile_bytes + 16;
        const size_t val_bytes = (size_t)nnz * sizeof(float);
        if (vt_scratch && val_bytes <= 128 * 1024) {
            // values -> transposed order through LDS, then the product streams them
            SPT_HIP_TRY(hipFuncSetAttribute(
                reinterpret_cast<const void *>(&permute_values_kernel),
                hipFuncAttributeMaxDynamicSharedMemorySize, (int)val_bytes));
            hipLaunchKernelGGL(permute_values_kernel, dim3((unsigned)B), dim3(SP_THREADS_LDS),
                               val_bytes, s, perm, values, vt_scratch, nnz);
            SPT_LAUNCH_CHECK();
            SPT_HIP_TRY(hipFuncSetAttribute(
                reinterpret_cast<const void *>(&spmm_t64_lds_kernel<G_SPMM>),
                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
            hipLaunchKernelGGL(spmm_t64_lds_kernel<G_SPMM>, dim3((unsigned)B),
                               dim3(SP_THREADS_LDS), lds_bytes, s, ptr, indices, perm,
                               vt_scratch, x, y, S, nnz, x_heads, y_heads);
        } else {
            SPT_HIP_TRY(hipFuncSetAttribute(
                reinterpret_cast<const void *>(&spmm_t64_lds_kernel<G_SPMM_PERM>),
                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
            hipLaunchKernelGGL(spmm_t64_lds_kernel<G_SPMM_PERM>, dim3((unsigned)B),
                               dim3(SP_THREADS_LDS), lds_bytes, s, ptr, indices, perm, values, x,
                               y, S, nnz, x_heads, y_heads);
        }
    } else if (E == 64 || E == 128) {
        const bool lds = tile_bytes <= 128 * 1024 && B >= 32;
        if (strided && !lds) return SPT_EUNSUP;  // head layout: LDS-resident path only
        int splits = 1;
        while ((long long)B * splits < 256 && splits < 8) splits <<= 1;
        const int bpb = (S + 63) / 64;
#define SPT_G4(L)                                                                              \
    do {                                                                                       \
        if (lds) {                                                                             \
            SPT_HIP_TRY(hipFuncSetAttribute(                                                   \
                reinterpret_cast<const void *>(&spmm_g4_lds_kernel<L, MODE>),                  \
                hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_bytes));                 \
            hipLaunchKernelGGL((spmm_g4_lds_kernel<L, MODE>), dim3((unsigned)(B * splits)),    \
                               dim3(SP_THREADS_LDS), tile_bytes, s, ptr, ptr_stride, indices,  \
                               perm, values, x, y, S, nnz, splits, x_heads, y_heads);          \
        } else {                                                                               \
            hipLaunchKernelGGL((spmm_g4_global_kernel<L, MODE>), dim3((unsigned)(B * bpb)),    \
                               dim3(SP_THREADS), 0, s, ptr, ptr_stride, indices, perm, values, \
                               x, y, B, S, nnz, bpb);                                          \
        }                                                                                      \
    } while (0)
        if (E == 64) SPT_G4(4);
        else SPT_G4(8);
#undef SPT_G4
    } else {
        if (strided) return SPT_EUNSUP;
        const int LPE = pow2_ceil(E / 4);
        const int rows_per_block = 16;
        const int tiles = (S + rows_per_block - 1) / rows_per_block;
        const long long nblk = (long long)B * tiles;
        if (nblk > 0x7FFFFFFFLL) return SPT_EUNSUP;
        dim3 grid((unsigned)nblk);
#define SPT_GEN(L)                                                                             \
    hipLaunchKernelGGL((spmm_generic_kernel<L, PERM>), grid, dim3(SP_THREADS), 0, s, ptr,      \
                       ptr_stride, indices, perm, values, x, y, B, S, E, nnz, tiles,           \
                       rows_per_block)
        switch (LPE) {
            case 1: SPT_GEN(1); break;
            case 2: SPT_GEN(2); break;
            case 4: SPT_GEN(4); break;
            case 8: SPT_GEN(8); break;
            case 16: SPT_GEN(16); break;
            case 32: SPT_GEN(32); break;
            default: SPT_GEN(64); break;
        }
#undef SPT_GEN
    }
    SPT_LAUNCH_CHECK();
    return SPT_OK;
}

static int check_spmm_args(const void *a, const void *b, const void *c, const void *d,
                           const void *e, int B, int S, int E, int nnz) {
    if (!a || !b || !c || !d || !e) return SPT_EINVAL;
    if (B <= 0 || S <= 0 || E <= 0 || nnz < 0) return SPT_EINVAL;
    if (E % 4 != 0) return SPT_ESHAPE;
    if (E > 256) return SPT_EUNSUP;
    return SPT_OK;
}

// A^T x on the chunked form: (slice, chunk) products into `partial`, then the sum over chunks
static int launch_gather_chunked(const int32_t *indptr, const TransposedCsr &t,
                                 const float *values, const float *x, float *y, float *partial,
                                 int B, int S, int nnz, int x_heads, int y_heads, hipStream_t s) {
    if (x_heads < 0 || y_heads < 0) return SPT_EINVAL;
    if ((x_heads > 0 && B % x_heads != 0) || (y_heads > 0 && B % y_heads != 0)) return SPT_ESHAPE;
    if (!partial) return SPT_EINVAL;
    const int nch = S / CH_ROWS;
    const size_t lds = (size_t)CH_ROWS * 64 * sizeof(float) + 16;
    SPT_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&spmm_t64_chunk_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(spmm_t64_chunk_kernel, dim3((unsigned)(B * nch)), dim3(SP_THREADS_LDS), lds,
                       s, indptr, t.t_ptr, t.t_row, t.t_perm, values, x, partial, B, S, nnz, nch,
                       x_heads);
    SPT_LAUNCH_CHECK();
    const long long total4 = (long long)B * S * 16;
    hipLaunchKernelGGL(chunk_reduce_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0,
                       s, partial, y, B, S, nch, y_heads);
    SPT_LAUNCH_CHECK();
    return SPT_OK;
}

static int64_t product_scratch_bytes(int B, int S, int E, int nnz) {
    if (chunked_layout(S, E))                                        // per-chunk partial outputs
        return (int64_t)(S / CH_ROWS) * B * S * E * (int64_t)sizeof(float);
    return (int64_t)B * nnz * (int64_t)sizeof(float);                 // permuted values
}

// ---- the dense-tile form on the matrix cores: spmm_mfma_kernel (spmm_mfma.hip) ----
// The shapes of the matrix-core spmm (non-transposed); everything else is for the gather form
// above.  All S keys of a row stripe are multiplied: worth it from a density of 1 / 16
// (lookup: 1 / 8); a row's first 64 entries live in registers: mean row length <= 64.
static bool spmm_mfma_takes(int B, int S, int E, int nnz) {
    if ((E != 64 && E != 128) || S < 64 || S > MA_MAXNT * MA_KT || B <= 0 || nnz <= 0) return false;
    if ((long long)nnz * 16 < (long long)S * S || (long long)nnz > 64ll * S) return false;
    // OPT-IN (SPT_SPMM_MFMA=1): measured at the configs[1] shape (256 slices x 512 x 64, 64 entries per
    // row; profiles/r04_ops_kernels.txt) this form takes 65.7 us against the gather form's 46.3 -- see
    // the kernel's header for where they go -- so the gather form stays the default.
    const char *on = getenv("SPT_SPMM_MFMA");
    return on && on[0] == '1';
}
static int spmm_mfma_launch(const int32_t *indptr, const int32_t *indices, const float *values, const float *x,
                            float *y, int B, int S, int E, int nnz, int x_heads, int y_heads, hipStream_t s) {
    if (!spmm_mfma_takes(B, S, E, nnz)) return SPT_EUNSUP;
    return E == 64 ? launch_spmm_mfma(indptr, indices, values, x, y, B, S, nnz, x_heads, y_heads, s)
                   : e128::launch_spmm_mfma(indptr, indices, values, x, y, B, S, nnz, x_heads, y_heads, s);
}

}  // namespace spt

using namespace spt;

extern "C" int64_t spt_csr_transpose_workspace_bytes(int batch_size, int seq_length, int nnz,
                                                     int d_head) {
    if (batch_size <= 0 || seq_length <= 0 || nnz < 0) return 0;
    return transpose_bytes(batch_size, seq_length, nnz, d_head);
}

extern "C" int spt_csr_transpose(const int32_t *indptr, const int32_t *indices, void *transposed,
                                 int batch_size, int seq_length, int nnz, int d_head,
                                 void *stream) {
    if (!indptr || !indices || !transposed) return SPT_EINVAL;
    if (batch_size <= 0 || seq_length <= 0 || nnz <= 0) return SPT_EINVAL;
    const TransposedCsr t = carve(transposed, batch_size, seq_length, nnz, d_head);
    if (chunked_layout(seq_length, d_head))
        return launch_transpose_chunked(indptr, indices, t, batch_size, seq_length, nnz,
                                        (hipStream_t)stream);
    return launch_transpose(indptr, indices, t, batch_size, seq_length, nnz, (hipStream_t)stream);
}

extern "C" int64_t spt_spmm_transposed_workspace_bytes(int batch_size, int seq_length, int d_head,
                                                       int nnz) {
    if (batch_size <= 0 || seq_length <= 0 || d_head <= 0 || nnz <= 0) return 0;
    return product_scratch_bytes(batch_size, seq_length, d_head, nnz);
}

extern "C" int spt_spmm_transposed(const int32_t *indptr, const void *transposed,
                                   const float *values, const float *x, float *y, void *workspace,
                                   int batch_size, int seq_length, int d_head, int nnz,
                                   int x_heads, int y_heads, void *stream) {
    const int rc =
        check_spmm_args(transposed, values, x, y, indptr, batch_size, seq_length, d_head, nnz);
    if (rc != SPT_OK) return rc;
    if (nnz == 0) return SPT_EINVAL;
    const TransposedCsr t =
        carve(const_cast<void *>(transposed), batch_size, seq_length, nnz, d_head);
    if (chunked_layout(seq_length, d_head))
        return launch_gather_chunked(indptr, t, values, x, y, reinterpret_cast<float *>(workspace),
                                     batch_size, seq_length, nnz, x_heads, y_heads,
                                     (hipStream_t)stream);
    return launch_gather<true>(t.t_ptr, seq_length + 1, t.t_row, t.t_perm, values, x, y,
                               batch_size, seq_length, d_head, nnz, x_heads, y_heads,
                               (hipStream_t)stream, reinterpret_cast<float *>(workspace));
}

extern "C" int spt_spmm_form(int trans_lhs, int batch_size, int seq_length, int d_head, int nnz) {
    return !trans_lhs && spt::spmm_mfma_takes(batch_size, seq_length, d_head, nnz) ? 1 : 0;
}

extern "C" int64_t spt_spmm_workspace_bytes(int trans_lhs, int batch_size, int seq_length,
                                            int d_head, int nnz) {
    if (!trans_lhs) return 0;
    return (int64_t)align256(
               (size_t)spt_csr_transpose_workspace_bytes(batch_size, seq_length, nnz, d_head)) +
           spt_spmm_transposed_workspace_bytes(batch_size, seq_length, d_head, nnz);
}

extern "C" int spt_spmm_forward(int trans_lhs, const int32_t *indptr, const int32_t *indices,
                                const float *values, const float *x, float *y, void *workspace,
                                int batch_size, int seq_length, int d_head, int nnz,
                                int x_heads, int y_heads, void *stream) {
    const int rc =
        check_spmm_args(indptr, indices, values, x, y, batch_size, seq_length, d_head, nnz);
    if (rc != SPT_OK) return rc;
    const int B = batch_size, S = seq_length, E = d_head;
    hipStream_t s = (hipStream_t)stream;
    if (nnz == 0) {
        // (a kernel, not hipMemsetAsync: memset nodes lose their place in a captured graph,
        // spt_common.h; the library makes no memset or memcpy call anywhere)
        if ((long long)B * S * E > 0x7fffffffLL) return SPT_EUNSUP;
        SPT_ZERO_WORDS(y, B * S * E, s);
        SPT_LAUNCH_CHECK();
        return SPT_OK;
    }
    if (!trans_lhs) {
        // patterns as dense as lookup's: the dense-tile form on the matrix cores (mfma_attention.hip)
        const int rc2 = spmm_mfma_launch(indptr, indices, values, x, y, B, S, E, nnz, x_heads, y_heads, s);
        if (rc2 != SPT_EUNSUP) return rc2;
        return launch_gather<false>(indptr, 0, indices, nullptr, values, x, y, B, S, E, nnz,
                                    x_heads, y_heads, s);
    }
    if (!workspace) return SPT_EINVAL;
    const TransposedCsr t = carve(workspace, B, S, nnz, E);
    float *scratch = reinterpret_cast<float *>(
        reinterpret_cast<char *>(workspace) +
        align256((size_t)spt_csr_transpose_workspace_bytes(B, S, nnz, E)));
    if (chunked_layout(S, E)) {
        const int rc2 = launch_transpose_chunked(indptr, indices, t, B, S, nnz, s);
        if (rc2 != SPT_OK) return rc2;
        return launch_gather_chunked(indptr, t, values, x, y, scratch, B, S, nnz, x_heads, y_heads,
                                     s);
    }
    const int rc2 = launch_transpose(indptr, indices, t, B, S, nnz, s);
    if (rc2 != SPT_OK) return rc2;
    return launch_gather<true>(t.t_ptr, S + 1, t.t_row, t.t_perm, values, x, y, B, S, E, nnz,
                               x_heads, y_heads, s, scratch);
}
