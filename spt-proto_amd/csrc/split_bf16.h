// split_bf16.h -- the library's arithmetic contract, stated once.
//
// An fp32 operand of a matrix-core product is split in two bf16 parts
//     hi = RNE bf16 of x,   lo = RNE bf16 of (x - hi)
// and a product is three bf16 MFMAs with fp32 accumulation, small terms first:
//     lo . hi  +  hi . lo  +  hi . hi            (the lo . lo term is left out)
// <= 2^-16 relative error per product.  A value that IS a bf16 (bf16 storage) is its own hi part
// and has no lo part: its products take one MFMA per part of the other operand.
// tests/exact.py is the same arithmetic in numpy; tests/test_gpu_exact_arithmetic.py and
// tests/test_gpu_arith_contract.py hold every matrix-core kernel to it bit for bit.
//
// Included by the grouped GEMM units (grouped_gemm.h), the attention units (mfma_frag.h),
// sddmm_tile.hip and lora_side.hip.
#ifndef SPT_SPLIT_BF16_H
#define SPT_SPLIT_BF16_H

#include "spt_common.h"

namespace spt {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef short v4s16 __attribute__((ext_vector_type(4)));

// two floats -> a packed bf16 pair (first value in the low half), RNE.
// Whole-vector conversions: element-wise (__bf16) casts compile to one v_cvt_pk_bf16_f32 per
// ELEMENT plus re-packing (81 conversions per tile instead of 24).
__device__ __forceinline__ unsigned pack_bf16(float a, float b) {
    const f32x2 x = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(x, bf16x2));
}
// one float -> its bf16 bit pattern, RNE
__device__ __forceinline__ unsigned short round_bf16(float a) { return (unsigned short)pack_bf16(a, 0.0f); }

// two floats -> packed bf16 pairs: hi = RNE, lo = RNE(x - hi)
struct Split { unsigned hi, lo; };
__device__ __forceinline__ Split split2(float a, float b) {
    const f32x2 x = {a, b};
    Split s;
    s.hi = __builtin_bit_cast(unsigned, __builtin_convertvector(x, bf16x2));
    const f32x2 hf = {__builtin_bit_cast(float, s.hi << 16),
                      __builtin_bit_cast(float, s.hi & 0xffff0000u)};
    s.lo = __builtin_bit_cast(unsigned, __builtin_convertvector(x - hf, bf16x2));
    return s;
}
struct Frag { uint4 hi, lo; };      // 8 bf16 each: one MFMA operand fragment, split
__device__ __forceinline__ Frag split8(float a0, float a1, float a2, float a3, float a4,
                                       float a5, float a6, float a7) {
    const Split s0 = split2(a0, a1), s1 = split2(a2, a3), s2 = split2(a4, a5),
                s3 = split2(a6, a7);
    Frag f;
    f.hi = make_uint4(s0.hi, s1.hi, s2.hi, s3.hi);
    f.lo = make_uint4(s0.lo, s1.lo, s2.lo, s3.lo);
    return f;
}
__device__ __forceinline__ Frag split8(const float4 &a, const float4 &b) {
    return split8(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w);
}
// (word by word, as lora_down_kernel always had it: the order of these assignments reaches the
// instruction scheduler, and forwarding to the form above changes the code of one instantiation)
__device__ __forceinline__ Frag split8(const float (&v)[8]) {
    Frag f;
    Split s;
    s = split2(v[0], v[1]); f.hi.x = s.hi; f.lo.x = s.lo;
    s = split2(v[2], v[3]); f.hi.y = s.hi; f.lo.y = s.lo;
    s = split2(v[4], v[5]); f.hi.z = s.hi; f.lo.z = s.lo;
    s = split2(v[6], v[7]); f.hi.w = s.hi; f.lo.w = s.lo;
    return f;
}

// ds_read_b64_tr_b16: lane i of a 16-lane group receives column i of a 4-row x 16-column block of
// 16-bit elements; lane 4 q + p supplies the address of row q, columns 4 p .. 4 p + 3
__device__ __forceinline__ uint2 lds_tr_b64(const char *p) {
    const v4s16 r = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) v4s16 *)(p));
    return __builtin_bit_cast(uint2, r);
}

// one bf16 MFMA; the accumulator's type selects the shape: 32x32x16 (f32x16) or 16x16x32 (f32x4)
__device__ __forceinline__ f32x16 mma(const uint4 &a, const uint4 &b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a),
                                                   __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mma(const uint4 &a, const uint4 &b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                   __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// (a.hi + a.lo)(b.hi + b.lo) without the lo*lo term, small terms first.  PA / PB = parts of the
// operand: 2 = an fp32 value split in two, 1 = a value that IS a bf16 (bf16 storage: no lo part).
template <int PA, int PB, typename Acc>
__device__ __forceinline__ Acc mm(const Frag &a, const Frag &b, Acc c) {
    if (PA == 2) c = mma(a.lo, b.hi, c);
    if (PB == 2) c = mma(a.hi, b.lo, c);
    return mma(a.hi, b.hi, c);
}

}  // namespace spt

#endif  // SPT_SPLIT_BF16_H
