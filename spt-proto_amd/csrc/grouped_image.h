// grouped_image.h -- the LDS tile layouts of pre-split operands and their MFMA fragment readers:
// read by the image path (grouped_gemm_img.hip), the loader / consumer ring (grouped_gemm_ring.hip)
// and the weight gradient (grouped_wgrad.hip, which stages its rows in the NC layout).
#ifndef SPT_GROUPED_IMAGE_H
#define SPT_GROUPED_IMAGE_H

#include "split_bf16.h"

namespace spt {

// Global image of a [rows, cols] fp32 matrix (spt_split_bf16): row-major, every 32 columns
// one 128-byte block [hi: 32 bf16 | lo: 32 bf16].  One k-step of a k-contiguous operand tile
// is then ONE full 128-byte line per row, and a k-row of an n-contiguous weight tile
// (128 n) is 512 contiguous bytes.
//
// LDS tiles (16 KiB each, two stages of A | B = 64 KiB per workgroup):
//   KC  [rows][128 B]  k-contiguous operands (A; B of "BT" weights; the K extension).
//       The 16-byte chunk c = 4 part + (k / 8) of row r sits at chunk c ^ ((r >> 1) & 7):
//       a ds_read_b128 lane group (16 rows, one chunk each) then covers all 64 banks.
//   NC  [32 k][512 B]  n-contiguous weights ("BN"), read with ds_read_b64_tr_b16.
//       The 64-byte segment s = 2 (n / 32) + part of k-row k sits at segment s ^ (k & 3):
//       the four k-rows of a transposing read fall on four different 64-byte bank groups.
// An LDS-DMA writes base + 16 lane, so the swizzle is applied to the SOURCE: the lane that
// fills physical chunk pc of row r fetches logical chunk pc ^ swz(r) of that row.

// fragments: lane l holds A[row l & 31][k = 16 q2 + 8 (l >> 5) + 0..7] and
// B[k = same][col l & 31], 16 bytes per part
__device__ __forceinline__ uint4 gi_frag_kc(const char *tile, int row, int q2, int part, int fh) {
    const int c = 4 * part + 2 * q2 + fh;
    return *reinterpret_cast<const uint4 *>(tile + row * 128 + ((c ^ ((row >> 1) & 7)) << 4));
}
__device__ __forceinline__ uint4 gi_frag_nc(const char *tile, int ncol0, int q2, int part, int fh,
                                            int lane) {
    // lane 4 q + p of a 16-lane group supplies k-row q, columns 4 p .. 4 p + 3 of the
    // group's 16 n; lane i receives column i of the four k-rows: two blocks = 8 k's
    const int gl = lane & 15, q = gl >> 2, p = gl & 3, nhalf = (lane >> 4) & 1;
    const int seg = 2 * (ncol0 >> 5) + part;
    const char *ptr = tile + (16 * q2 + 8 * fh + q) * 512 + ((seg ^ q) << 6) + nhalf * 32 + p * 8;
    const uint2 lo = lds_tr_b64(ptr), hi = lds_tr_b64(ptr + 4 * 512);
    return make_uint4(lo.x, lo.y, hi.x, hi.y);
}
// The same fragment of an fp32 tile [row][32 k floats] (the A32 form: the activation goes
// global -> LDS by LDS-DMA as it is, 128 bytes per row and k-step like an image row, and is split
// HERE, on its way into the matrix cores): the lane's 8 floats are chunks 4 q2 + 2 fh and + 1 of
// its row, same swizzle, two conflict-free ds_read_b128; 24 VALU per fragment (96 per k-step and
// wave at NI = 2, under 24 MFMAs).  What it buys: no pre-split image of the activation -- no
// split pass, no second copy of the activation in memory, and every GEMM (the backward's dX
// products too, whose operand nobody else reads) takes the LDS-DMA k-loop.
__device__ __forceinline__ Frag gi_frag_a32(const char *tile, int row, int q2, int fh) {
    const int c0 = 4 * q2 + 2 * fh, sw = (row >> 1) & 7;
    const float4 x = *reinterpret_cast<const float4 *>(tile + row * 128 + ((c0 ^ sw) << 4));
    const float4 y = *reinterpret_cast<const float4 *>(tile + row * 128 + (((c0 | 1) ^ sw) << 4));
    // (value by value: given x and y by reference, hipcc loads their pairs from LDS as vectors and
    // the code of one ring kernel changes)
    return split8(x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w);
}

}  // namespace spt

#endif  // SPT_GROUPED_IMAGE_H
