// mfma_frag.h -- split-bf16 operand fragments and the bf16 LDS images of 32-row tiles, for one head
// dimension: what the kernels of mfma_attention.hip and spmm_mfma.hip are written in.
//
// The split itself (hi / lo parts, three MFMAs per product) is split_bf16.h's.
//
// A unit that includes this is compiled once per head dimension: for d_head 64 and, with
// -DMA_E_VALUE=128 / 80, for d_head 128 / 80.  What it puts between MA_NS_OPEN and MA_NS_CLOSE lands
// in namespace spt, spt::e128 or spt::e80; mfma_tiles.h declares the launchers of all three, and the
// d_head 64 units dispatch to them.
#ifndef SPT_MFMA_FRAG_H
#define SPT_MFMA_FRAG_H

#include "mfma_tiles.h"
#include "split_bf16.h"

#ifndef MA_E_VALUE
#define MA_E_VALUE 64
#endif
#if MA_E_VALUE == 64
#define MA_NS_OPEN namespace spt {
#define MA_NS_CLOSE }
#elif MA_E_VALUE == 128
#define MA_NS_OPEN namespace spt { namespace e128 {
#define MA_NS_CLOSE } }
#elif MA_E_VALUE == 80
#define MA_NS_OPEN namespace spt { namespace e80 {
#define MA_NS_CLOSE } }
#else
#error "MA_E_VALUE: 64, 80 or 128"
#endif

MA_NS_OPEN

#ifndef MA_THREADS_VALUE
#define MA_THREADS_VALUE 512
#endif
constexpr int MA_THREADS = MA_THREADS_VALUE;       // 512 or 256
constexpr int MA_WAVES = MA_THREADS / SPT_WAVE;    // 8 or 4
constexpr int MA_E = MA_E_VALUE;                   // d_head: 64, 80 or 128
constexpr int MA_EQ = MA_E / 4;                    // float4 per row of a tile
constexpr int MA_KS = MA_E / 16;                   // k-steps of a contraction over e (80: 5, exact)
// 32-column tiles of an [*, E] result.  d_head 80 takes a third tile whose last 16 columns are
// never stored: its B-operand reads repeat columns 64 .. 79 there (read_cols_tr, read_cols), so
// the padding lives in accumulator registers only -- no LDS image and no global access is wider
// than E.  (+20 % on the products that produce E columns)
constexpr int MA_ET = (MA_E + 31) / 32;
constexpr int MA_ELAST = MA_E - 32 * (MA_ET - 1);  // stored columns of the last tile: 32 or 16
constexpr int MA_ROWS = MA_WAVES * MA_WROWS;       // 256 rows per workgroup (the forward)

// LDS images of one key tile, bf16: rows padded so that the operand reads are conflict-free
constexpr int MA_KLD = MA_E * 2 + 16;              // bytes per row of a rows image: E bf16 + 16
constexpr int MA_VLD = 72;                         // bytes per e row of V^T: 32 bf16 + 8
// the forward's tile: K rows image (hi, lo) | V rows image (hi, lo)
constexpr int MA_KH = 0, MA_KL = MA_KT * MA_KLD, MA_VH = 2 * MA_KT * MA_KLD,
              MA_VL = 3 * MA_KT * MA_KLD, MA_IMG = 4 * MA_KT * MA_KLD;         // 18432 B
constexpr int MA_TLD = 36;                         // floats per row of the epilogue's [e][row] tile

// The lane id, from an instruction the compiler will not move.  For the kernels' RARE branches:
// whatever such a branch derives from the ordinary `lane` is loop-invariant, gets hoisted out of
// the tile loop, and then occupies registers (or scratch) for the whole kernel -- 16 hoisted shift
// counts of the saturation fix were spilled in the prologue of the key-owned backward.
__device__ __forceinline__ int rare_lane() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// ---- element types of the dense operands (q, k, v, y and their gradients) ----
// float: the reference's fp32 tensors, every value split in two bf16 parts on its way to the
// matrix cores.  bf16_t (raw 16-bit patterns): bf16 STORAGE -- a stored value is its own hi part
// and has no lo part, so operands that go to LDS unchanged (K, V, Q tiles) are copied, not
// converted, and their products cost one MFMA per part of the OTHER operand.  Values computed in
// fp32 on the way (scaled Q, probabilities, dS, weighted dY) are split in two as before, so the
// only rounding the bf16 path adds is that of its stored outputs.
typedef unsigned short bf16_t;
__device__ __forceinline__ float bf16_lo(unsigned w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __builtin_bit_cast(float, w & 0xffff0000u); }
template <typename T> struct Elem;
template <> struct Elem<float> {
    static constexpr int PARTS = 2;
    typedef float4 raw4;                                 // four consecutive elements, as loaded
    static __device__ __forceinline__ float4 f4(const float4 &r) { return r; }
};
template <> struct Elem<bf16_t> {
    static constexpr int PARTS = 1;
    typedef uint2 raw4;
    static __device__ __forceinline__ float4 f4(const uint2 &r) {
        return make_float4(bf16_lo(r.x), bf16_hi(r.x), bf16_lo(r.y), bf16_hi(r.y));
    }
};
template <typename T>
__device__ __forceinline__ typename Elem<T>::raw4 ld_raw4(const T *p) {
    return *reinterpret_cast<const typename Elem<T>::raw4 *>(p);
}
template <typename T>
__device__ __forceinline__ float4 ld4(const T *p) { return Elem<T>::f4(ld_raw4(p)); }
__device__ __forceinline__ void st4(float *p, const float4 &v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ void st4(bf16_t *p, const float4 &v) {
    *reinterpret_cast<uint2 *>(p) = make_uint2(pack_bf16(v.x, v.y), pack_bf16(v.z, v.w));
}
__device__ __forceinline__ void st1(float *p, float v) { *p = v; }
__device__ __forceinline__ void st1(bf16_t *p, float v) { *p = (bf16_t)(pack_bf16(v, 0.0f) & 0xffffu); }

// ---- 32-row tiles of a dense operand: global -> registers -> bf16 LDS images ----
// "rows" image [r][e] (144-byte rows): A-operand fragments by read_rows;
// "cols" image [e][r] (72-byte rows):  B-operand fragments in accumulator k order by read_cols.
// An image is a hi part followed (fp32 sources) by a lo part of the same shape.
constexpr int MA_RIMG = MA_KT * MA_KLD;            // one rows image part: 4608 B
constexpr int MA_CIMG = MA_E * MA_VLD;             // one cols image part: 4608 B
// four values of row r at e4 .. e4 + 3 into a rows image: fp32 (split, two parts) ...
__device__ __forceinline__ void put_rows4(char *img, int r, int e4, const float4 &x) {
    const Split a = split2(x.x, x.y), b = split2(x.z, x.w);
    *reinterpret_cast<uint2 *>(img + r * MA_KLD + e4 * 2) = make_uint2(a.hi, b.hi);
    *reinterpret_cast<uint2 *>(img + MA_RIMG + r * MA_KLD + e4 * 2) = make_uint2(a.lo, b.lo);
}
// ... or stored bf16 (copied, one part)
__device__ __forceinline__ void put_rows4(char *img, int r, int e4, const uint2 &x) {
    *reinterpret_cast<uint2 *>(img + r * MA_KLD + e4 * 2) = x;
}
// four fp32 values of column e at rows r4 .. r4 + 3 (an operand stored [E][S]) into a cols image
__device__ __forceinline__ void put_cols4(char *img, int e, int r4, const float4 &x) {
    const Split a = split2(x.x, x.y), b = split2(x.z, x.w);
    *reinterpret_cast<uint2 *>(img + e * MA_VLD + r4 * 2) = make_uint2(a.hi, b.hi);
    *reinterpret_cast<uint2 *>(img + MA_CIMG + e * MA_VLD + r4 * 2) = make_uint2(a.lo, b.lo);
}

// Key tiles of the forward and of the row-owned backward: K rows image | V rows image (each
// hi, lo).  With NT threads staging, thread t stages the four elements (row t / (E/4) + RPP u,
// columns 4 (t % (E/4)) ..) for u < RPT.  d_head 80 (EVEN false: 640 float4s per tile, 20 per
// row) numbers the tile's float4s f = t + NT u instead, row f / 20, columns 4 (f % 20) ..; the
// last round is partial: its loads are clamped to float4 F - 1, its stores skipped.
template <int NT>
struct Share {
    static constexpr int F = 32 * MA_EQ;             // float4s of a 32 x E tile
    static constexpr bool EVEN = F % NT == 0 && NT % MA_EQ == 0;
    static constexpr int RPT = (F + NT - 1) / NT;    // 32 x E tile: float4s per thread to stage
    static constexpr int RPP = NT / MA_EQ;           // tile rows covered by one float4 per thread (EVEN)
    static __device__ __forceinline__ int slot(int t, int u) { return min(t + NT * u, F - 1); }
    static __device__ __forceinline__ bool owns(int t, int u) { return F % NT == 0 || t + NT * u < F; }
};
template <typename T, int NT = MA_THREADS>
struct TileRegs { typename Elem<T>::raw4 kf[Share<NT>::RPT], vf[Share<NT>::RPT]; };
template <typename T, int NT = MA_THREADS>
struct TileStager {
    static constexpr int RPT = Share<NT>::RPT, RPP = Share<NT>::RPP;
    const T *k_b, *v_b;
    int ld, S, jl, e4, tid;
    __device__ __forceinline__ TileStager(const T *k, const T *v, int ld_, int S_, int tid_)
        : k_b(k), v_b(v), ld(ld_), S(S_), jl(tid_ / MA_EQ), e4((tid_ % MA_EQ) * 4), tid(tid_) {}
    // Unconditional loads with clamped rows: a load under a branch makes the compiler wait
    // with vmcnt(0) for OLDER loads too (it cannot count what the branch issued), which
    // exposed the full memory latency in every iteration.  Keys >= S read row S - 1: finite
    // data whose cells have multiplicity 0.
    __device__ __forceinline__ TileRegs<T, NT> load(int t) const {
        TileRegs<T, NT> r;
#pragma unroll
        for (int u = 0; u < RPT; u++) {
            if constexpr (Share<NT>::EVEN) {
                const int j = min(t * MA_KT + jl + RPP * u, S - 1);
                r.kf[u] = ld_raw4(k_b + (size_t)j * ld + e4);
                r.vf[u] = ld_raw4(v_b + (size_t)j * ld + e4);
            } else {
                const int f = Share<NT>::slot(tid, u);
                const int j = min(t * MA_KT + f / MA_EQ, S - 1), c4 = (f % MA_EQ) * 4;
                r.kf[u] = ld_raw4(k_b + (size_t)j * ld + c4);
                r.vf[u] = ld_raw4(v_b + (size_t)j * ld + c4);
            }
        }
        return r;
    }
    __device__ __forceinline__ void store(char *buf, const TileRegs<T, NT> &r) const {
#pragma unroll
        for (int u = 0; u < RPT; u++) {
            if constexpr (Share<NT>::EVEN) {
                put_rows4(buf + MA_KH, jl + RPP * u, e4, r.kf[u]);
                put_rows4(buf + MA_VH, jl + RPP * u, e4, r.vf[u]);
            } else if (Share<NT>::owns(tid, u)) {
                const int f = tid + NT * u;
                put_rows4(buf + MA_KH, f / MA_EQ, (f % MA_EQ) * 4, r.kf[u]);
                put_rows4(buf + MA_VH, f / MA_EQ, (f % MA_EQ) * 4, r.vf[u]);
            }
        }
    }
    // max over this thread's K rows of the tile of the sum of squares of its four columns (not
    // EVEN: of its float4s, whichever columns they hold)
    __device__ __forceinline__ float k_share(const TileRegs<T, NT> &r) const {
        float best = 0.f;
#pragma unroll
        for (int u = 0; u < RPT; u++) {
            const float4 x = Elem<T>::f4(r.kf[u]);
            best = fmaxf(best, fmaf(x.x, x.x, fmaf(x.y, x.y, fmaf(x.z, x.z, x.w * x.w))));
        }
        return best;
    }
};

// A-operand fragment of k-step ks from a row-major image: lane (r, h) reads row r, elements
// 8h + 16ks .. + 8 (16 bytes).  NP = parts the image holds (the lo read is skipped for 1).
template <int NP>
__device__ __forceinline__ Frag read_rows(const char *hi, const char *lo, int lane, int ks) {
    const int off = (lane & 31) * MA_KLD + 16 * (lane >> 5) + 32 * ks;
    Frag f;
    f.hi = *reinterpret_cast<const uint4 *>(hi + off);
    f.lo = NP == 2 ? *reinterpret_cast<const uint4 *>(lo + off) : make_uint4(0u, 0u, 0u, 0u);
    return f;
}
// B-operand fragment whose k order matches an accumulator tile used as the A operand
// (k-step s, element jj of lane half h <-> tile row 16s + 8(jj>>2) + 4h + (jj&3)):
// lane (c, h) reads row c of the transposed image at 16s + 4h .. +4 and 16s + 8 + 4h .. +4
// (rows >= E -- the last tile's unstored columns at d_head 80 -- read row row - 16 instead)
__device__ __forceinline__ Frag read_cols(const char *hi, const char *lo, int row, int h, int s) {
    if constexpr (MA_E % 32 != 0)
        if (row >= MA_E) row -= 16;
    const int off = row * MA_VLD + 32 * s + 8 * h;

    const uint2 a = *reinterpret_cast<const uint2 *>(hi + off),
                b = *reinterpret_cast<const uint2 *>(hi + off + 16),
                c = *reinterpret_cast<const uint2 *>(lo + off),
                d = *reinterpret_cast<const uint2 *>(lo + off + 16);
    Frag f;
    f.hi = make_uint4(a.x, a.y, b.x, b.y);
    f.lo = make_uint4(c.x, c.y, d.x, d.y);
    return f;
}

// The same B-operand fragment from a ROWS image through gfx950's transposing LDS read:
// ds_read_b64_tr_b16 hands lane i of a 16-lane group column i of a 4-row x 16-column block of
// 16-bit elements, rows in its elements 0..3; lane 4q + p of the group supplies the address of
// row q, columns 4p .. 4p + 3.  Two blocks (tile rows 16s + 4h .. and 16s + 8 + 4h ..) give
// elements 0..3 and 4..7; the group's columns are 16 (lane >> 4 & 1) .. + 15 of the 32-column
// half `col0`.  No transposed copy of the tile and none of its 2-byte scattered stores.
// (All 64 lanes must be active: the gather crosses lanes.)  A half whose upper 16 columns lie
// beyond E (d_head 80, col0 = 64) reads its lower 16 columns twice: output columns 80 .. 95 of
// the product are then copies of 64 .. 79 and are never stored.
template <int NP>
__device__ __forceinline__ Frag read_cols_tr(const char *hi, const char *lo, int col0, int lane,
                                             int s) {
    const int gl = lane & 15, q = gl >> 2, p = gl & 3, h = lane >> 5;
    int off = (16 * s + 4 * h + q) * MA_KLD + (col0 + 16 * ((lane >> 4) & 1) + 4 * p) * 2;
    if constexpr (MA_E % 32 != 0)
        if (col0 + 16 >= MA_E) off = (16 * s + 4 * h + q) * MA_KLD + (col0 + 4 * p) * 2;
    const uint2 a = lds_tr_b64(hi + off), b = lds_tr_b64(hi + off + 8 * MA_KLD);
    Frag f;
    f.hi = make_uint4(a.x, a.y, b.x, b.y);
    f.lo = make_uint4(0u, 0u, 0u, 0u);
    if (NP == 2) {
        const uint2 c = lds_tr_b64(lo + off), d = lds_tr_b64(lo + off + 8 * MA_KLD);
        f.lo = make_uint4(c.x, c.y, d.x, d.y);
    }
    return f;
}

// A-operand fragment of k-step ks from a COLS image [e][row] (an operand that arrives as
// [E][S]): lane (r, h) wants row r, elements 8h + 16ks .. + 8 -- columns of the image, again the
// transposing read: blocks of image rows e0 .. e0+3 and e0+4 .. e0+7, image columns = tile rows
__device__ __forceinline__ Frag read_rows_tr(const char *hi, const char *lo, int lane, int ks) {
    const int gl = lane & 15, q = gl >> 2, p = gl & 3, h = lane >> 5;
    const int off = (8 * h + 16 * ks + q) * MA_VLD + (16 * ((lane >> 4) & 1) + 4 * p) * 2;
    const uint2 a = lds_tr_b64(hi + off), b = lds_tr_b64(hi + off + 4 * MA_VLD),
                c = lds_tr_b64(lo + off), d = lds_tr_b64(lo + off + 4 * MA_VLD);
    Frag f;
    f.hi = make_uint4(a.x, a.y, b.x, b.y);
    f.lo = make_uint4(c.x, c.y, d.x, d.y);
    return f;
}

// B-operand fragments of a wave's own 32 rows of a dense operand x[row * ld + e]: lane (r, h)
// holds row i0 + r, elements 8h + 16ks .. + 8.
template <typename T>
__device__ __forceinline__ void load_own_rows_raw(float (&x)[MA_E / 2], const T *x_b, int ld, int S,
                                                  int i0, int lane) {
    // rows >= S read row S - 1 (unconditional loads; such rows are never stored)
    const int row = min(i0 + (lane & 31), S - 1), h = lane >> 5;
#pragma unroll
    for (int ks = 0; ks < MA_KS; ks++) {
        const T *p = x_b + (size_t)row * ld + 8 * h + 16 * ks;
        const float4 a = ld4(p), b = ld4(p + 4);
        x[8 * ks + 0] = a.x; x[8 * ks + 1] = a.y; x[8 * ks + 2] = a.z; x[8 * ks + 3] = a.w;
        x[8 * ks + 4] = b.x; x[8 * ks + 5] = b.y; x[8 * ks + 6] = b.z; x[8 * ks + 7] = b.w;
    }
}
// split into the four k-step fragments, optionally pre-multiplied (the score scale folded
// into the operand: one multiply per element here instead of one per cell per tile)
__device__ __forceinline__ void split_own_rows(Frag (&f)[MA_KS], const float (&x)[MA_E / 2],
                                               float mult = 1.0f) {
#pragma unroll
    for (int ks = 0; ks < MA_KS; ks++)
        f[ks] = split8(x[8 * ks] * mult, x[8 * ks + 1] * mult, x[8 * ks + 2] * mult,
                       x[8 * ks + 3] * mult, x[8 * ks + 4] * mult, x[8 * ks + 5] * mult,
                       x[8 * ks + 6] * mult, x[8 * ks + 7] * mult);
}

// ---- wide global accesses for operands whose register layout is element-wise ----
// A 4-byte load or store per lane moves 256 bytes per wave instruction; the kernels' own-row
// operands and results (8 KiB per wave and tensor) are therefore passed through a wave-private
// LDS tile of 32 x MA_TLD floats, one 32-column half at a time.
//
// One e-half of a wave's 32-row accumulator tile (column = lane & 31, rows in the registers)
// -> rows of `dst` (row stride ld elements), 8 rows x 32 elements per store instruction; only
// its first `cols` columns (32, or 16 for the last tile at d_head 80).
template <typename T>
__device__ __forceinline__ void store_acc_half(const f32x16 &acc, float mult, float *tile,
                                               T *dst, size_t ld, int rows_left, int lane,
                                               int cols = 32) {
    const int c32 = lane & 31, h = lane >> 5;
#pragma unroll
    for (int r = 0; r < 16; r++) tile[acc_row(r, h) * MA_TLD + c32] = acc[r] * mult;
    wave_lds_fence();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int row = (lane >> 3) + 8 * k, e4 = (lane & 7) * 4;
        const float4 o = *reinterpret_cast<const float4 *>(tile + row * MA_TLD + e4);
        if (row < rows_left && (MA_E % 32 == 0 || e4 < cols)) st4(dst + (size_t)row * ld + e4, o);
    }
    wave_lds_fence();
}
// A wave's own 32 rows of an operand stored [E][S] (row i0 .. of every e) into the fragment
// order of load_own_rows_raw: x[8 ks + j] = src[(8h + 16ks + j) * S + i0 + (lane & 31)].
template <typename T>
__device__ __forceinline__ void load_own_rows_transposed(float (&x)[MA_E / 2], const T *src, int S,
                                                         int i0, float *tile, int lane) {
    const int c32 = lane & 31, h = lane >> 5;
    const int i4 = min(i0 + (lane & 7) * 4, S - 4) - i0;      // (S % 4 == 0; rows >= S unused)
#pragma unroll
    for (int hf = 0; hf < MA_ET; hf++) {
        const int ne = hf + 1 < MA_ET ? 32 : MA_ELAST;        // e of this 32-e group (80: 32, 32, 16)
#pragma unroll
        for (int k = 0; k < ne / 8; k++) {
            const int el = (lane >> 3) + 8 * k;
            const float4 v4 = ld4(src + (size_t)(32 * hf + el) * S + i0 + i4);
            *reinterpret_cast<float4 *>(tile + el * MA_TLD + (lane & 7) * 4) = v4;
        }
        wave_lds_fence();
#pragma unroll
        for (int kk = 0; kk < ne / 16; kk++) {
#pragma unroll
            for (int j = 0; j < 8; j++)
                x[8 * (2 * hf + kk) + j] = tile[(8 * h + 16 * kk + j) * MA_TLD + c32];
        }
        wave_lds_fence();
    }
}

MA_NS_CLOSE

#endif  // SPT_MFMA_FRAG_H
