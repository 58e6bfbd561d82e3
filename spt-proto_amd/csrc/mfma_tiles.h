// mfma_tiles.h -- what the matrix-core attention units share and d_head does not touch: the
// geometry of a 32 x 32 score tile, the stored cell tiles (written by attention_tiles.hip, read by
// the kernels of mfma_attention.hip) and their workspace, and the launchers of the three per-d_head
// builds of mfma_attention.hip / spmm_mfma.hip.
#ifndef SPT_MFMA_TILES_H
#define SPT_MFMA_TILES_H

#include "spt_common.h"

namespace spt {

constexpr int MA_WROWS = 32;                       // rows per wave = one matrix-core tile
constexpr int MA_KT = 32;                          // keys per tile
constexpr int MA_MAXZ = 256;                       // entries per row (cell counts are bytes)
constexpr int MA_MAXNT = 64;                       // key tiles: S <= 2048
constexpr int MA_CLD = 9;                          // words per row of the multiplicity tile
constexpr int MA_CELLS = MA_WROWS * MA_KT;         // bytes of one stored cell tile

__device__ __forceinline__ void wave_lds_fence() {
    // LDS executes one wave's instructions in order; this only stops the compiler from
    // moving accesses of different lanes' data across the point
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// accumulator register r of lane half h holds tile row  (r & 3) + 8 (r >> 2) + 4 h
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// ---- cell tiles: multiplicity of every (row, key) cell, per 32 x 32 tile ----
//   masks [batch][RT][2] uint64: [0] bit t set <=> key tile t has a live entry in row tile rt;
//     [1] bit t set <=> some cell of that tile has multiplicity >= 2 ("multi" tile)
//   cells [batch][RT (RT + 1) / 2][64 lanes][16] uint8: tile (rt, t <= rt) at rt (rt + 1) / 2 + t;
//     byte 4 g + u of lane (c, h) = multiplicity of key 32 t + 8 g + 4 h + u in row 32 rt + c --
//     accumulator register 4 g + u of that lane when the tile is computed as D[key, row]
//   cells_t, same indexing: byte 4 g + u of lane (c, h) = multiplicity of key 32 t + c in row
//     32 rt + 8 g + 4 h + u -- the tile computed as D[row, key] (the key-owned backward)
//   A tile that is not "multi" (all counts 0 or 1: every tile of a lookup pattern except those
//     holding its zero padding) stores only 128 bytes per orientation instead: word c of the
//     tile's slot = the 32-bit key mask of row c (cells_t: the row mask of key c); a consumer
//     lane reads the 16 bytes holding its word and spreads its 16 bits back into the byte form.
//     The consumers are bound by the bytes they move: this takes 36 MB off each of them.
//   live = col <= row (softmax.cu:19-31 masks the others) and 0 <= col < S.
__host__ __device__ __forceinline__ size_t tri(size_t n) { return n * (n + 1) / 2; }
// bytes of a tile's slot: 1 KiB in the full layout, 128 in the compact one (see CellTiles)
__device__ __forceinline__ int cell_slot_bytes(const void *pool) { return pool ? 128 : MA_CELLS; }
// a tile's 16 bytes as loaded -> the four count words of this lane (byte form)
__device__ __forceinline__ uint4 cell_words(const uint4 &v, bool multi, int lane) {
    if (multi) return v;
    const int c = lane & 3;
    const unsigned m = (c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w) >> (4 * (lane >> 5));
    auto spread = [](unsigned n) { return ((n & 0xFu) * 0x00204081u) & 0x01010101u; };
    return make_uint4(spread(m), spread(m >> 8), spread(m >> 16), spread(m >> 24));
}
// Two layouts of the stored tiles (chosen by the caller of spt_attention_mfma_prepare):
//   full     every tile owns a 1 KiB slot, which holds its byte form or (first 128 bytes) its
//            mask form;
//   compact  every tile owns a 128-byte slot for its mask form; a byte form lives in a pool of
//            one 1 KiB slot per ROW TILE and is allowed for key tile 0 only -- what a lookup
//            pattern needs (its only repeated column is the padding column 0), at 1/4 of the
//            memory (S = 512: 66 instead of 272 KiB per slice and step).
// `pool == nullptr` selects the full layout.
// a consumer wave's view of its row tile's cell tiles
struct CellTiles {
    unsigned long long mask, multi;
    unsigned satrows;         // rows of this row tile whose one live cell holds 256 (stored 255)
    int last;                 // the row tile's own index = its last stored key tile
    int stride;               // uint4 per slot
    const uint4 *base;        // tile t of this row tile: base[t * stride + ...]
    const uint4 *pooled;      // compact layout: the byte form of key tile 0, else nullptr
    __device__ __forceinline__ CellTiles(const unsigned long long *masks,
                                         const unsigned char *cells, const unsigned char *pool,
                                         const unsigned *sat, int b, int RT, int rt, bool have) {
        mask = have ? masks[2 * ((size_t)b * RT + rt)] : 0ull;
        multi = have ? masks[2 * ((size_t)b * RT + rt) + 1] : 0ull;
        satrows = have ? sat[(size_t)b * RT + rt] : 0u;
        last = have ? rt : 0;
        stride = cell_slot_bytes(pool) / 16;
        base = reinterpret_cast<const uint4 *>(
            cells + ((size_t)b * tri(RT) + tri(have ? rt : 0)) * cell_slot_bytes(pool));
        pooled = pool ? reinterpret_cast<const uint4 *>(
                            pool + ((size_t)b * RT + (have ? rt : 0)) * MA_CELLS)
                      : nullptr;
    }
    __device__ __forceinline__ bool live(int t) const { return (mask >> t) & 1ull; }
    __device__ __forceinline__ bool is_multi(int t) const { return (multi >> min(t, 63)) & 1ull; }
    // always in bounds (t clamped), so the caller can load unconditionally; ONE 16-byte load
    // either way: the lane's own 16 counts, or the four row masks that include its row's
    __device__ __forceinline__ uint4 load(int t, int lane) const {
        const int tc = min(t, last);
        if (is_multi(tc)) return pooled ? pooled[lane] : base[tc * stride + lane];
        return base[tc * stride + ((lane & 31) >> 2)];
    }
    // (the 16 bytes loaded for tile t) -> count words
    __device__ __forceinline__ uint4 words(const uint4 &v, int t, int lane) const {
        return cell_words(v, is_multi(min(t, last)), lane);
    }
};
// byte u of a cell word as float (v_cvt_f32_ubyte<u>)
template <int U>
__device__ __forceinline__ float cell_count(unsigned word) {
    return (float)((word >> (8 * U)) & 0xffu);
}
// A row that is ONE column 256 times (row 0 of a lookup pattern at Z = 256) keeps a byte count of 255
// and its bit in `sat`.  Nothing in the tile loops knows: with m = 255 the forward's y and the
// backward's P = m e / (m e) are what m = 256 gives (the count cancels), and only the row sum the
// forward REPORTS is 255 / 256 of the true one.  So the forward stores rs * 256 / 255 for such rows,
// and the backward kernels take rs * 255 / 256 back for them where they load the row sums -- once per
// row, outside every loop.  (Round 4's first form fixed the count inside the loops, behind a
// wave-uniform branch: 7-13 % on every Z = 256 launch for one cell per slice.)
constexpr float MA_SAT_UP = 256.0f / 255.0f, MA_SAT_DOWN = 255.0f / 256.0f;

// bounds [batch][MA_BOUND_SLOTS][2] floats, written by the forward's workgroup g of a slice:
// [0] max over its rows of |q_i|^2, [1] an upper bound of max |k_j|^2 over the keys it staged
constexpr int MA_BOUND_SLOTS = 8;                   // workgroups per slice: S <= 2048

inline bool mfma_shape_ok(int S, int E, int nnz) {
    if ((E != 64 && E != 80 && E != 128) || S <= 0 || nnz <= 0 || nnz % S != 0) return false;
    const int Z = nnz / S;
    return Z <= MA_MAXZ && Z % 4 == 0 && S <= MA_MAXNT * MA_KT;
}
// Workspace: 256-byte header (word 0: layout, word 1: flags -- bit 0: a compact layout was
// given a pattern that repeats a column outside key tile 0) | masks, sat | cells | cells_t
// [| pool | pool_t in the compact layout].
struct TileSet {
    unsigned long long *masks;
    unsigned *sat;
    unsigned char *cells, *cells_t, *pool, *pool_t;
};
constexpr size_t MA_HEADER = 256;
inline size_t tile_cells_bytes(int B, int S, int layout) {
    const size_t RT = (S + MA_WROWS - 1) / MA_WROWS;
    return (size_t)B * tri(RT) * (layout == SPT_TILES_COMPACT ? 128 : MA_CELLS);
}
inline size_t tile_pool_bytes(int B, int S, int layout) {
    const size_t RT = (S + MA_WROWS - 1) / MA_WROWS;
    return layout == SPT_TILES_COMPACT ? (size_t)B * RT * MA_CELLS : 0;
}
inline size_t tile_mask_bytes(int B, int S) {
    const size_t RT = (S + MA_WROWS - 1) / MA_WROWS;
    return (((size_t)B * RT * (2 * sizeof(unsigned long long) + sizeof(unsigned))) + 255) & ~(size_t)255;
}
inline TileSet carve_tiles(void *ws, int B, int S, int layout) {
    TileSet t;
    char *p = static_cast<char *>(ws) + MA_HEADER;
    t.masks = reinterpret_cast<unsigned long long *>(p);
    t.sat = reinterpret_cast<unsigned *>(t.masks + 2 * (size_t)B * ((S + MA_WROWS - 1) / MA_WROWS));
    t.cells = reinterpret_cast<unsigned char *>(p + tile_mask_bytes(B, S));
    t.cells_t = t.cells + tile_cells_bytes(B, S, layout);
    t.pool = t.pool_t = nullptr;
    if (layout == SPT_TILES_COMPACT) {
        t.pool = t.cells_t + tile_cells_bytes(B, S, layout);
        t.pool_t = t.pool + tile_pool_bytes(B, S, layout);
    }
    return t;
}

// ---- launchers: one set per d_head, in spt (64), spt::e128 and spt::e80 ----
// dtype: SPT_F32 (float tensors) or SPT_BF16 (bf16 storage; row_sum and delta stay fp32).
// kv_heads: heads of k and v ([N, S, kv_heads, E]; == heads unless the heads are grouped -- then
// grad_k / grad_v are per-query-head partials [N, S, heads, E], see spt_common.h kv_view).
// (launch_spmm_mfma is defined for d_head 64 and 128 only: spmm_mfma.hip.)
#define MA_DECLARE_LAUNCHERS                                                                      \
    int launch_forward(const unsigned long long *masks, const unsigned char *cells,               \
                       const unsigned char *pool, const unsigned *sat, int dtype, const void *q,  \
                       const void *k, const void *v, void *y, float *row_sum, float *bounds,      \
                       int batch_size, int S, float scale, float clamp, int heads,                \
                       int kv_heads, int y_transposed, hipStream_t s);                            \
    int launch_backward(const unsigned long long *masks, const unsigned char *cells,              \
                        const unsigned char *cells_t, const unsigned char *pool,                  \
                        const unsigned char *pool_t, const unsigned *sat, int dtype,              \
                        const void *q, const void *k, const void *v, const void *y,               \
                        const void *grad_y, const float *row_sum, const float *bounds,            \
                        float *delta, void *grad_q, void *grad_k, void *grad_v, int batch_size,   \
                        int S, float scale, float clamp, int heads, int kv_heads,                 \
                        int transposed, hipStream_t s);                                           \
    int launch_spmm_mfma(const int32_t *indptr, const int32_t *indices, const float *values,      \
                         const float *x, float *y, int B, int S, int nnz, int x_heads,            \
                         int y_heads, hipStream_t s);
MA_DECLARE_LAUNCHERS
namespace e128 { MA_DECLARE_LAUNCHERS }
namespace e80 { MA_DECLARE_LAUNCHERS }
#undef MA_DECLARE_LAUNCHERS

}  // namespace spt

#endif  // SPT_MFMA_TILES_H
