// attention_tiles.hip -- the cell-tile pass of the matrix-core attention: one pass over the CSR
// (spt_attention_mfma_prepare) that stores, per (32-row tile, 32-key tile), the multiplicity of
// every cell already permuted into the accumulator layout of the consumers (mfma_attention.hip), and
// the host side of that workspace.  Nothing here depends on d_head: compiled once.  The layout of
// the stored tiles and the consumers' view of them are in mfma_tiles.h.
#include "mfma_tiles.h"
#include <stdlib.h>

namespace spt {

// A wave owns a row tile and walks its key tiles in chunks of MB_CHUNK: the chunk's counts
// live in LDS as [tile][row][key] bytes (4 keys per word); every entry whose column falls into
// the chunk does one ds_add_u32 (LDS atomics run at about one lane per clock per CU, so they
// are the kernel's cost: the transposed tiles are gathered bytewise from the same counts
// rather than counted a second time).  (A first
// version bucketed the entries by key tile with a counting sort before counting: 33 us at
// the bench shape, latency-bound on its LDS read-modify-write chains and wave scans.)
// A byte saturates at 255: only Z = 256 can reach it, in a row whose 256 entries are ONE column
// (row 0 of a lookup pattern: column 0, 256 times); then the add that would carry into the
// neighbouring key is taken back and the row's bit is set in the row tile's word of `sat`
//   sat [batch][RT] uint32: bit r set <=> row 32 rt + r holds ONE live cell, of multiplicity 256,
//     stored as 255 -- the consumers add the 1 back (round 4: row_sum of such a row is exact).
constexpr int MB_WAVES = 4;
constexpr int MB_CHUNK = 8;                          // key tiles per pass over the entries
constexpr int MB_CNT_WORDS = MB_CHUNK * MA_WROWS * MA_CLD;     // one orientation: 2304 words
__host__ __device__ __forceinline__ size_t prepare_lds_per_wave() {
    return (size_t)MB_CNT_WORDS * 4;                 // 9216 B
}
template <bool SATURATE>
__global__ __launch_bounds__(MB_WAVES * SPT_WAVE) void attention_cell_tiles_kernel(
    const int32_t *__restrict__ indices, unsigned long long *__restrict__ masks,
    unsigned char *__restrict__ cells, unsigned char *__restrict__ cells_t,
    unsigned char *__restrict__ pool, unsigned char *__restrict__ pool_t,
    unsigned *__restrict__ sat, int S, int Z, int NT, int RT, int n_tiles_total) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gw = blockIdx.x * MB_WAVES + wave;
    if (gw >= n_tiles_total) return;                    // no workgroup barrier below
    const int b = gw / RT, rt = gw - b * RT, i0 = rt * MA_WROWS;
    unsigned *cnt = reinterpret_cast<unsigned *>(smem + wave * prepare_lds_per_wave());
    unsigned satrows = 0;                               // (per lane; OR-reduced at the end)

    // the tile's rows are one contiguous run of 32 * Z ints (Z % 4 == 0)
    const int nrows = min(MA_WROWS, S - i0);
    const int n4 = nrows * Z / 4;
    const int4 *src = reinterpret_cast<const int4 *>(indices + ((size_t)b * S + i0) * Z);
    const int slot_bytes = cell_slot_bytes(pool);
    unsigned char *out = cells + ((size_t)b * tri(RT) + tri(rt)) * slot_bytes;
    unsigned char *out_t = cells_t + ((size_t)b * tri(RT) + tri(rt)) * slot_bytes;
    const int c32 = lane & 31, h = lane >> 5;
    const int nbuckets = min(NT, rt + 1);               // live entries have col <= row
    unsigned long long mask = 0, multi = 0;

    auto count = [&](unsigned *word, unsigned sh, int rl) {
        if (!SATURATE) {
            atomicAdd(word, 1u << sh);
        } else {
            const unsigned old = atomicAdd(word, 1u << sh);
            if (((old >> sh) & 0xffu) == 0xffu) {       // the row's 256th copy of this column
                atomicSub(word, 1u << sh);
                satrows |= 1u << rl;
            }
        }
    };
    for (int t0 = 0; t0 < nbuckets; t0 += MB_CHUNK) {
        uint4 *c4 = reinterpret_cast<uint4 *>(cnt);     // 9 x 64 x 16 bytes
#pragma unroll
        for (int x = 0; x < MB_CNT_WORDS / 4 / SPT_WAVE; x++)
            c4[x * SPT_WAVE + lane] = make_uint4(0u, 0u, 0u, 0u);
        wave_lds_fence();
        for (int x = lane; x < n4; x += SPT_WAVE) {
            const int4 e4 = src[x];
            const int rl = 4 * x / Z;                   // an int4 never straddles rows
            const int c[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int tl = (c[q] >> 5) - t0;
                if (c[q] >= 0 && c[q] <= i0 + rl && c[q] < S && tl >= 0 && tl < MB_CHUNK) {
                    const unsigned jl = c[q] & 31;
                    count(&cnt[(tl * MA_WROWS + rl) * MA_CLD + (jl >> 2)], 8 * (jl & 3), rl);
                }
            }
        }
        wave_lds_fence();
        const int tend = min(MB_CHUNK, nbuckets - t0);
        for (int tl = 0; tl < tend; tl++) {
            // word 2 g + h of row c holds keys 8 g + 4 h .. + 3: exactly this lane's bytes 4 g ..
            const unsigned *row = cnt + (tl * MA_WROWS + c32) * MA_CLD + h;
            uint4 mine = make_uint4(row[0], row[2], row[4], row[6]);
            if (__ballot((mine.x | mine.y | mine.z | mine.w) != 0u) == 0ull) continue;
            mask |= 1ull << (t0 + tl);
            // transposed: byte 4 g + u of lane (c, h) = count of key c in row 8 g + 4 h + u
            const unsigned char *bytes = reinterpret_cast<const unsigned char *>(cnt) +
                                         (size_t)tl * MA_WROWS * MA_CLD * 4 + c32;
            unsigned w[4];
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const unsigned char *p0 = bytes + (8 * g + 4 * h) * MA_CLD * 4;
                w[g] = (unsigned)p0[0] | ((unsigned)p0[MA_CLD * 4] << 8) |
                       ((unsigned)p0[2 * MA_CLD * 4] << 16) | ((unsigned)p0[3 * MA_CLD * 4] << 24);
            }
            uint4 *slot = reinterpret_cast<uint4 *>(out + (size_t)(t0 + tl) * slot_bytes);
            uint4 *slot_t = reinterpret_cast<uint4 *>(out_t + (size_t)(t0 + tl) * slot_bytes);
            const bool big = ((mine.x | mine.y | mine.z | mine.w) & 0xFEFEFEFEu) != 0u;
            // (compact layout: byte forms exist for key tile 0 only -- the caller vouches that
            // no other tile repeats a column, as lookup patterns do not; a tile that breaks the
            // promise is stored as if its counts were 0 / 1 and flagged in the header)
            const bool pooled_ok = pool == nullptr || t0 + tl == 0;
            if (__ballot(big) != 0ull && pooled_ok) {
                multi |= 1ull << (t0 + tl);
                if (pool) {
                    slot = reinterpret_cast<uint4 *>(pool + ((size_t)b * RT + rt) * MA_CELLS);
                    slot_t = reinterpret_cast<uint4 *>(pool_t + ((size_t)b * RT + rt) * MA_CELLS);
                }
                slot[lane] = mine;
                slot_t[lane] = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
                if (__ballot(big) != 0ull) {
                    if (lane == 0) atomicOr(reinterpret_cast<unsigned *>(masks) - 64 + 1, 1u);
                    auto clamp1 = [](unsigned x) { return (x | (x >> 1) | (x >> 2) | (x >> 3) | (x >> 4) |
                                                           (x >> 5) | (x >> 6) | (x >> 7)) & 0x01010101u; };
                    mine = make_uint4(clamp1(mine.x), clamp1(mine.y), clamp1(mine.z), clamp1(mine.w));
#pragma unroll
                    for (int g = 0; g < 4; g++) w[g] = clamp1(w[g]);
                }
                // counts are 0 / 1: 16 of the row's (key's) 32 bits sit in this lane, the other
                // 16 in lane ^ 32; bytes -> nibble by one multiply (no carries: each product
                // term lands on its own bit)
                auto bits16 = [&](unsigned w0, unsigned w1, unsigned w2, unsigned w3) {
                    auto nib = [](unsigned x) { return ((x * 0x01020408u) >> 24) & 0xFu; };
                    return (nib(w0) | (nib(w1) << 8) | (nib(w2) << 16) | (nib(w3) << 24)) << (4 * h);
                };
                unsigned rm = bits16(mine.x, mine.y, mine.z, mine.w);
                unsigned cm = bits16(w[0], w[1], w[2], w[3]);
                rm |= (unsigned)__shfl_xor((int)rm, 32, SPT_WAVE);
                cm |= (unsigned)__shfl_xor((int)cm, 32, SPT_WAVE);
                if (h == 0) {
                    reinterpret_cast<unsigned *>(slot)[c32] = rm;
                    reinterpret_cast<unsigned *>(slot_t)[c32] = cm;
                }
            }
        }
        wave_lds_fence();
    }
#pragma unroll
    for (int off = 1; off < SPT_WAVE; off <<= 1) satrows |= (unsigned)__shfl_xor((int)satrows, off, SPT_WAVE);
    if (lane == 0) {
        masks[2 * (size_t)gw] = mask;
        masks[2 * (size_t)gw + 1] = multi;
        sat[gw] = satrows;
    }
}

// The compact layout's builder (round 3).  Its promise -- only columns < 32 repeat inside a row --
// means every key tile but the first holds 0 / 1 cells: ONE pass over the row tile's entries sets
// bits ([key tile][row] words, ds_or) for the columns >= 32 and counts the columns < 32 in 32-bit
// counters (the padding column 0 pre-summed per lane: a row of S = 2048 holds up to 256 of them);
// the byte-count kernel above walks the entries once per eight key tiles with a ds_add per entry
// (and, at Z = 256, a returning add and a conditional subtract): 241 us per launch at S = 2048,
// Z = 256, B = 64, 6 % of an OPT-1.3B block's step.  Same masks, slots and pool as the kernel above
// (tests/test_gpu_mfma_attention.py compares whole workspaces); a repeated column >= 32 shows as
// popcount(row) != the row's count of such entries and sets the header's promise flag.
__host__ __device__ __forceinline__ size_t cell_bits_lds_per_wave(int NT) {
    return ((size_t)MA_WROWS * 32 + (size_t)(NT > 1 ? NT - 1 : 1) * MA_WROWS + MA_WROWS) * 4;
}
__global__ __launch_bounds__(MB_WAVES * SPT_WAVE) void attention_cell_bits_kernel(
    const int32_t *__restrict__ indices, unsigned long long *__restrict__ masks,
    unsigned char *__restrict__ cells, unsigned char *__restrict__ cells_t,
    unsigned char *__restrict__ pool, unsigned char *__restrict__ pool_t,
    unsigned *__restrict__ sat, int S, int Z, int NT, int RT, int n_tiles_total) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gw = blockIdx.x * MB_WAVES + wave;
    if (gw >= n_tiles_total) return;                    // no workgroup barrier below
    const int b = gw / RT, rt = gw - b * RT, i0 = rt * MA_WROWS;
    unsigned *cnt0 = reinterpret_cast<unsigned *>(smem + wave * cell_bits_lds_per_wave(NT));   // [row][key < 32]
    unsigned *bits = cnt0 + MA_WROWS * 32;              // [key tile - 1][row]
    const int nbuckets = min(NT, rt + 1);               // live entries have col <= row
    unsigned *nval = bits + (size_t)(NT > 1 ? NT - 1 : 1) * MA_WROWS;   // [row]: entries with col >= 32
    const int nrows = min(MA_WROWS, S - i0);
    const int n4 = nrows * Z / 4;
    const int4 *src = reinterpret_cast<const int4 *>(indices + ((size_t)b * S + i0) * Z);
    const int c32 = lane & 31, h = lane >> 5;

    for (int x = lane; x < MA_WROWS * 32 + (nbuckets - 1) * MA_WROWS; x += SPT_WAVE) cnt0[x] = 0u;
    if (lane < MA_WROWS) nval[lane] = 0u;
    wave_lds_fence();
    for (int x = lane; x < n4; x += SPT_WAVE) {
        const int4 e4 = src[x];
        const int rl = 4 * x / Z;                       // an int4 never straddles rows
        const int c[4] = {e4.x, e4.y, e4.z, e4.w};
        unsigned nz = 0, nv = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (c[q] == 0) {
                nz++;
            } else if (c[q] > 0 && c[q] <= i0 + rl && c[q] < S) {
                if (c[q] < 32) {
                    atomicAdd(&cnt0[rl * 32 + c[q]], 1u);
                } else {
                    atomicOr(&bits[((c[q] >> 5) - 1) * MA_WROWS + rl], 1u << (c[q] & 31));
                    nv++;
                }
            }
        }
        if (nz) atomicAdd(&cnt0[rl * 32], nz);
        if (nv) atomicAdd(&nval[rl], nv);
    }
    wave_lds_fence();
    // a repeated column >= 32 breaks the layout's promise (its second entry set no new bit)
    {
        unsigned pc = 0;
        if (lane < MA_WROWS)
            for (int t = 1; t < nbuckets; t++) pc += __popc(bits[(t - 1) * MA_WROWS + lane]);
        const bool broke = lane < MA_WROWS && pc != nval[lane];
        if (__ballot(broke) != 0ull && lane == 0) atomicOr(reinterpret_cast<unsigned *>(masks) - 64 + 1, 1u);
    }
    unsigned long long mask = 0, multi = 0;
    unsigned char *out = cells + ((size_t)b * tri(RT) + tri(rt)) * 128;
    unsigned char *out_t = cells_t + ((size_t)b * tri(RT) + tri(rt)) * 128;
    // ---- key tile 0: counts ----
    {
        // lane (c, h): its 16 counts of row c (keys 8 g + 4 h + u), saturated to a byte
        unsigned mine[4], tr[4];
        bool big = false, full = false;                 // full: row c holds a column 256 times
#pragma unroll
        for (int g = 0; g < 4; g++) {
            unsigned wm = 0, wt = 0;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const unsigned raw = cnt0[c32 * 32 + 8 * g + 4 * h + u];                   // row c, key ..
                const unsigned a = min(raw, 255u);
                const unsigned t2 = min(cnt0[(8 * g + 4 * h + u) * 32 + c32], 255u);        // key c, row ..
                wm |= a << (8 * u);
                wt |= t2 << (8 * u);
                big |= a > 1u;
                full |= raw > 255u;
            }
            mine[g] = wm;
            tr[g] = wt;
        }
        const unsigned long long fb = __ballot(full);   // (the two lane halves hold disjoint keys)
        if (lane == 0) sat[gw] = (unsigned)fb | (unsigned)(fb >> 32);
        const bool any = (mine[0] | mine[1] | mine[2] | mine[3]) != 0u;
        if (__ballot(any) != 0ull) {
            mask |= 1ull;
            if (__ballot(big) != 0ull) {
                multi |= 1ull;
                reinterpret_cast<uint4 *>(pool + ((size_t)b * RT + rt) * MA_CELLS)[lane] =
                    make_uint4(mine[0], mine[1], mine[2], mine[3]);
                reinterpret_cast<uint4 *>(pool_t + ((size_t)b * RT + rt) * MA_CELLS)[lane] =
                    make_uint4(tr[0], tr[1], tr[2], tr[3]);
            } else {
                // counts are 0 / 1: bytes -> bits (the kernel above, `bits16`)
                auto nib = [](unsigned x) { return ((x * 0x01020408u) >> 24) & 0xFu; };
                auto bits16 = [&](const unsigned (&w)[4]) {
                    return (nib(w[0]) | (nib(w[1]) << 8) | (nib(w[2]) << 16) | (nib(w[3]) << 24)) << (4 * h);
                };
                unsigned rm = bits16(mine), cm = bits16(tr);
                rm |= (unsigned)__shfl_xor((int)rm, 32, SPT_WAVE);
                cm |= (unsigned)__shfl_xor((int)cm, 32, SPT_WAVE);
                if (h == 0) {
                    reinterpret_cast<unsigned *>(out)[c32] = rm;
                    reinterpret_cast<unsigned *>(out_t)[c32] = cm;
                }
            }
        }
    }
    // ---- key tiles 1 ..: bits ----
    for (int t = 1; t < nbuckets; t++) {
        const unsigned *tb = bits + (t - 1) * MA_WROWS;
        const unsigned rm = tb[c32];                    // row c: its 32 keys of this tile
        if (__ballot(rm != 0u) == 0ull) continue;
        mask |= 1ull << t;
        // key c: bit i = row i has it; each half of the wave gathers 16 rows (broadcast reads)
        unsigned cm = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) cm |= ((tb[16 * h + i] >> c32) & 1u) << (16 * h + i);
        cm |= (unsigned)__shfl_xor((int)cm, 32, SPT_WAVE);
        if (h == 0) {
            reinterpret_cast<unsigned *>(out + (size_t)t * 128)[c32] = rm;
            reinterpret_cast<unsigned *>(out_t + (size_t)t * 128)[c32] = cm;
        }
    }
    if (lane == 0) {
        masks[2 * (size_t)gw] = mask;
        masks[2 * (size_t)gw + 1] = multi;
    }
}

// ---- grouped key/value heads: the fixed-order sum of the key-owned kernel's partials ----
// parts [rows, heads, E] (one partial of grad_k / grad_v per QUERY head, as the key-owned kernel
// writes them) -> out [rows, kv_heads, E]: out[r, j] = ((p[r, j g] + p[r, j g + 1]) + p[r, j g + 2]) + ...
// over the g = heads / kv_heads query heads of kv head j, ascending, plain fp32 adds -- the same bits
// on every run.  A thread owns one float4 of the output; a row's partials are g runs of E floats E
// apart, so consecutive threads read consecutive 16 bytes.
__global__ __launch_bounds__(256) void head_group_sum_kernel(const float4 *__restrict__ parts,
                                                             float4 *__restrict__ out, long long n4,
                                                             int e4, int group) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const long long slot = i / e4;                      // (row, kv head)
    const int c = (int)(i - slot * e4);
    const float4 *p = parts + slot * group * e4 + c;
    float4 acc = p[0];
    for (int u = 1; u < group; u++) {
        const float4 x = p[(long long)u * e4];
        acc.x += x.x;
        acc.y += x.y;
        acc.z += x.z;
        acc.w += x.w;
    }
    out[i] = acc;
}

}  // namespace spt

extern "C" int spt_head_group_sum(const float *parts, float *out, long long rows, int heads,
                                  int kv_heads, int d_head, void *stream) {
    using namespace spt;
    if (!parts || !out) return SPT_EINVAL;
    if (heads <= 0 || kv_heads <= 0 || heads % kv_heads != 0) return SPT_ESHAPE;
    if (rows <= 0 || d_head <= 0 || d_head % 4 != 0) return SPT_ESHAPE;
    const int e4 = d_head / 4;
    const long long n4 = rows * kv_heads * e4;
    const long long blocks = (n4 + 255) / 256;
    if (blocks > 0x7FFFFFFFLL) return SPT_EUNSUP;
    hipLaunchKernelGGL(head_group_sum_kernel, dim3((unsigned)blocks), dim3(256), 0,
                       static_cast<hipStream_t>(stream), reinterpret_cast<const float4 *>(parts),
                       reinterpret_cast<float4 *>(out), n4, e4, heads / kv_heads);
    SPT_LAUNCH_CHECK();
    return SPT_OK;
}

extern "C" int spt_attention_mfma_supported(int seq_length, int d_head, int nnz) {
    return spt::mfma_shape_ok(seq_length, d_head, nnz) ? 1 : 0;
}

extern "C" int64_t spt_attention_mfma_tiles_bytes(int batch_size, int seq_length, int nnz,
                                                  int layout) {
    using namespace spt;
    if (batch_size <= 0 || !mfma_shape_ok(seq_length, 64, nnz)) return 0;   // (any d_head: same tiles)
    if (layout != SPT_TILES_FULL && layout != SPT_TILES_COMPACT) return 0;
    return (int64_t)(MA_HEADER + tile_mask_bytes(batch_size, seq_length) +
                     2 * tile_cells_bytes(batch_size, seq_length, layout) +
                     2 * tile_pool_bytes(batch_size, seq_length, layout));
}

extern "C" int spt_attention_mfma_prepare(const int32_t *indices, void *tiles, int batch_size,
                                          int seq_length, int nnz, int layout, void *stream) {
    using namespace spt;
    if (!indices || !tiles || batch_size <= 0) return SPT_EINVAL;
    if (layout != SPT_TILES_FULL && layout != SPT_TILES_COMPACT) return SPT_EINVAL;
    if (!mfma_shape_ok(seq_length, 64, nnz)) return SPT_EUNSUP;
    const int S = seq_length, Z = nnz / S, NT = (S + MA_KT - 1) / MA_KT;
    const int RT = (S + MA_WROWS - 1) / MA_WROWS, total = batch_size * RT;
    const TileSet ts = carve_tiles(tiles, batch_size, S, layout);
    const size_t lds = (size_t)MB_WAVES * prepare_lds_per_wave();
    const dim3 grid((total + MB_WAVES - 1) / MB_WAVES), block(MB_WAVES * SPT_WAVE);
    hipStream_t s = static_cast<hipStream_t>(stream);
    SPT_ZERO_WORDS(tiles, MA_HEADER / 4, s);
    SPT_LAUNCH_CHECK();
    // (at S <= 512 -- two chunks of key tiles -- the byte-count kernel is the faster one: 22.8 against
    // 26.0 us at the configs[2] shape; SPT_CELL_TILES_COUNTS / _BITS force either for A/B runs)
    const bool bits = layout == SPT_TILES_COMPACT && !getenv("SPT_CELL_TILES_COUNTS") &&
                      (NT > 2 * MB_CHUNK || getenv("SPT_CELL_TILES_BITS"));
    if (bits) {
        const size_t lds_bits = (size_t)MB_WAVES * cell_bits_lds_per_wave(NT);
        SPT_HIP_TRY(hipFuncSetAttribute((const void *)attention_cell_bits_kernel,
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bits));
        hipLaunchKernelGGL(attention_cell_bits_kernel, grid, block, lds_bits, s, indices, ts.masks,
                           ts.cells, ts.cells_t, ts.pool, ts.pool_t, ts.sat, S, Z, NT, RT, total);
    } else if (Z > 255) {
        SPT_HIP_TRY(hipFuncSetAttribute((const void *)attention_cell_tiles_kernel<true>,
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(attention_cell_tiles_kernel<true>, grid, block, lds, s, indices,
                           ts.masks, ts.cells, ts.cells_t, ts.pool, ts.pool_t, ts.sat, S, Z, NT, RT,
                           total);
    } else {
        SPT_HIP_TRY(hipFuncSetAttribute((const void *)attention_cell_tiles_kernel<false>,
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(attention_cell_tiles_kernel<false>, grid, block, lds, s, indices,
                           ts.masks, ts.cells, ts.cells_t, ts.pool, ts.pool_t, ts.sat, S, Z, NT, RT,
                           total);
    }
    SPT_LAUNCH_CHECK();
    return SPT_OK;
}

extern "C" int spt_attention_mfma_bounds_floats(int batch_size) {
    return batch_size > 0 ? batch_size * spt::MA_BOUND_SLOTS * 2 : 0;
}
