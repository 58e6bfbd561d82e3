// grouped_gemm.h -- what every unit of the grouped GEMM reads (the map of the units is in
// grouped_gemm.hip): the tile constants, GroupedArgs, the activations, the plain-fp32 recomputation of
// one pre-activation, the work distribution, the bf16 storage helpers, the epilogue all tile kernels
// share, and the launchers of the operand-path units.
#ifndef SPT_GROUPED_GEMM_H
#define SPT_GROUPED_GEMM_H

#include "split_bf16.h"

namespace spt {

constexpr int GG_THREADS = 256;
constexpr int GG_BM = 128;
constexpr int GG_BN = 128;
constexpr int GG_BK = 32;
// workgroups per CU the round arithmetic of the kernels counts on (both paths: two fit)
constexpr int GG_SLOTS_PER_CU = 2;
// behind the operand tiles either kernel's LDS array carries four rows of 128 floats: for the
// ReLU epilogue |a2 row|^2 and |b2 row|^2 of the K extension's operands (written while they
// are staged) and rowscale * |a row| of the tile's rows, and rowscale of the tile's rows itself
// (1 without one) -- both loaded in the prologue: the scaling after the k-loop and every row of the
// epilogue read them from LDS (as global loads inside the epilogue's row loop each was a
// memory latency in the open, eight per 32 rows)
constexpr int GG_EXTRAS = 4 * 128;
// The ReLU queue is cut into segments with a counter each (16 words apart: a line of their own),
// a workgroup appends to segment blockIdx % GG_FIX_SEGS: ONE returning atomic counter takes
// ~88 increments / us from the whole chip (MI355X_MICROARCH.md, "dequeue"), and a GEMM queues
// ~10,000 elements -- measured 105 us on one counter.
constexpr int GG_FIX_SEGS = 256;

enum { EPI_PLAIN = 0, EPI_ACT = 1, EPI_DACT = 2 };
enum { ACT_RELU = 0, ACT_GELU = 1, ACT_SILU = 2 };

struct GroupedArgs {
    const float *a;         // [*, K] row-major, leading dimension lda (register path)
    const int32_t *gather;  // [P] or null
    const float *w;
    const float *bias;      // [G, N] or null
    const float *rowscale;  // [P] or null
    const int32_t *offsets; // [G + 1]
    float *out;             // [P, N] row-major
    int P, K, N, G;
    int lda;
    // K in segments (register path): A(row, kk) = a[(kk / a_seg_k) * a_seg_stride + row * lda + kk % a_seg_k]
    // -- the k-loop walks several matrices [*, a_seg_k] that lie a_seg_stride floats apart (the sum
    // of the q / k / v products of a backward as ONE contraction); 0: one matrix [*, K]
    int a_seg_k;
    long long a_seg_stride;
    long long ldo;          // row stride of out / out2 / h_in / s_in (>= N; launch_grouped: 0 -> N)
    int accumulate;         // EPI_PLAIN: out += result (the sum of several products in one buffer)
    long long gstride;
    int ldn, ldk;
    // K extension (the LoRA side product), added AFTER rowscale / bias:
    //   v[p, n] += sum_{j < R} a2[src2(p), j] * b2[g * b2_gstride + n * b2_ldn + j]
    const float *a2;
    const int32_t *gather2;
    const float *b2;
    int lda2, R;
    long long b2_gstride;
    int b2_ldn;
    long long b2_seg;       // != 0: column j of b2 lies in segment j / 16, b2_seg floats apart (register path)
    // epilogue
    int act;
    float *out2;            // EPI_ACT: pre-activation (null: not kept, e.g. ReLU)
    const float *h_in;      // EPI_DACT: activated values [P, N] (used when s_in is null: ReLU)
    const float *s_in;      // EPI_DACT: pre-activation values [P, N] or null
    float *pdot_main;       // EPI_DACT: [P, pdot_ld]: sum_n v[p, n] * h[p, n], v = the value before act'
    float *pdot_act;        // EPI_DACT: [P, pdot_ld]: sum_n out[p, n] * s[p, n] per half tile
    int pdot_ld;
    // EPI_ACT with ReLU: row norms of a [rows of a] and of the weight [G, N] (upper bounds do),
    // from which the epilogue tells which pre-activations lie within the split's error of zero
    const float *a_norm;
    const float *w_norm;
    unsigned *fix_count;    // ... and where their (row, column) pairs are queued for
    int2 *fix_list;         // relu_fix_kernel (null / full: recomputed in the epilogue itself):
    int fix_cap;            // GG_FIX_SEGS segments of fix_cap entries, one counter each
    int slots;              // workgroups resident at a time (CUs x occupancy)
    // image path: pre-split operands (spt_split_bf16), byte strides of one image row
    const char *a_img;
    const char *w_img;
    long long a_rowb, w_rowb;
    long long w_grow;       // image rows / 128-byte blocks from W_g(0, 0) to W_{g+1}(0, 0)
    int w_gblk;
    // spt_grouped_gemm_fused_w16: `w` holds IEEE halves (same element strides).  The k-loops read the
    // image alone; only gg_exact_preact reads `w` itself.  (In the struct's tail padding: the argument
    // block of every kernel keeps its size and offsets.)
    int w_f16;
};

// four IEEE halves (8-byte aligned) / one -> fp32: exact, every half is an fp32 value
__device__ __forceinline__ float4 gg_h4(const _Float16 *p) {
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    const h4 v = *reinterpret_cast<const h4 *>(p);
    return make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);
}

__device__ __forceinline__ float act_forward(int act, float s) {
    if (act == ACT_RELU) return fmaxf(s, 0.0f);
    if (act == ACT_GELU) return 0.5f * s * (1.0f + erff(s * 0.70710678118654752f));
    return s / (1.0f + __expf(-s));
}

__device__ __forceinline__ float act_derivative(int act, float s) {
    if (act == ACT_RELU) return s > 0.0f ? 1.0f : 0.0f;
    if (act == ACT_GELU) {
        const float cdf = 0.5f * (1.0f + erff(s * 0.70710678118654752f));
        return cdf + s * 0.3989422804014327f * __expf(-0.5f * s * s);
    }
    const float sg = 1.0f / (1.0f + __expf(-s));
    return sg * (1.0f + s * (1.0f - sg));
}

// v[p, n] as a plain fp32 computation by one wave: rowscale (sum_k a[src, k] W_g(n, k) + bias)
// + sum_j a2[src2, j] b2[n, j], every lane 4 k's per pass, butterfly sum.  All lanes return it.
// BATCHED: the k-contiguous weights' four passes of loads in flight together (relu_fix_kernel; the
// epilogue's own rare fallback keeps the compact loop: inlined there the batched form cost the
// activation GEMM registers)
// w_f16 (wave-uniform): the weight's elements are halves, widened as they are loaded -- the same
// values in the same order of additions, so the same bits as from the fp32 upcast of that weight.
// (HALVES = false: a caller whose `w` is never halves -- the bf16-storage kernels -- keeps its code)
template <bool BATCHED = false, bool HALVES = true>
__device__ __forceinline__ float gg_exact_preact(const GroupedArgs &g, int bucket, int p, int n,
                                                 int lane) {
    const bool w_f16 = HALVES && g.w_f16;
    const long long src = g.gather ? g.gather[p] : p;
    const float *ar = g.a + src * g.lda;
    // (the same element strides at either width; of the two typed pointers only the weight's own is read)
    const float *wr = g.w + (size_t)bucket * g.gstride + (size_t)n * g.ldn;
    const _Float16 *wh = reinterpret_cast<const _Float16 *>(g.w) + (size_t)bucket * g.gstride + (size_t)n * g.ldn;
    float part = 0.0f;
    if (BATCHED && g.ldk == 1) {
        // four passes' loads in flight together (clamped addresses, zeroed past K): as one load pair
        // per pass an element cost the wave four dependent round trips -- relu_fix_kernel took 22 us
        // for ~40 elements per segment.  Same order of additions as the plain loop below.
        for (int k0 = 4 * lane; k0 < g.K; k0 += 1024) {
            float4 x[4], y[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int k = min(k0 + 256 * i, g.K - 4);
                x[i] = *reinterpret_cast<const float4 *>(ar + k);
                y[i] = w_f16 ? gg_h4(wh + k) : *reinterpret_cast<const float4 *>(wr + k);
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (k0 + 256 * i < g.K) {
                    part = fmaf(x[i].x, y[i].x, part); part = fmaf(x[i].y, y[i].y, part);
                    part = fmaf(x[i].z, y[i].z, part); part = fmaf(x[i].w, y[i].w, part);
                }
            }
        }
    } else {
        for (int k = 4 * lane; k < g.K; k += 256) {
            const float4 x = *reinterpret_cast<const float4 *>(ar + k);
            float4 y;
            if (w_f16) {
                if (g.ldk == 1) {
                    y = gg_h4(wh + k);
                } else {
                    y.x = (float)wh[(size_t)k * g.ldk]; y.y = (float)wh[(size_t)(k + 1) * g.ldk];
                    y.z = (float)wh[(size_t)(k + 2) * g.ldk]; y.w = (float)wh[(size_t)(k + 3) * g.ldk];
                }
            } else if (g.ldk == 1) {
                y = *reinterpret_cast<const float4 *>(wr + k);
            } else {            // n-contiguous weights: a strided column
                y.x = wr[(size_t)k * g.ldk]; y.y = wr[(size_t)(k + 1) * g.ldk];
                y.z = wr[(size_t)(k + 2) * g.ldk]; y.w = wr[(size_t)(k + 3) * g.ldk];
            }
            part = fmaf(x.x, y.x, part); part = fmaf(x.y, y.y, part);
            part = fmaf(x.z, y.z, part); part = fmaf(x.w, y.w, part);
        }
    }
    float side = 0.0f;
    if (g.a2 && 4 * lane < g.R) {
        const long long src2 = g.gather2 ? g.gather2[p] : p;
        const float4 x = *reinterpret_cast<const float4 *>(g.a2 + src2 * g.lda2 + 4 * lane);
        const float4 y = *reinterpret_cast<const float4 *>(
            g.b2 + (size_t)bucket * g.b2_gstride + (size_t)n * g.b2_ldn + 4 * lane);
        side = fmaf(x.x, y.x, fmaf(x.y, y.y, fmaf(x.z, y.z, x.w * y.w)));
    }
    part = group_sum<64>(part);
    side = group_sum<64>(side);
    const float bb = g.bias ? g.bias[(size_t)bucket * g.N + n] : 0.0f;
    const float rr = g.rowscale ? g.rowscale[p] : 1.0f;
    return fmaf(rr, part + bb, side);
}

// acc = rowscale * acc, in the MFMA C layout (row = 32 i + (r & 3) + 8 (r >> 2) + 4 (l >> 5)).
// Runs between the k-loop and the K extension: nothing is ever divided by rowscale (a router
// coefficient may be 0: 2 sigmoid(logit) underflows below logit -104).
template <int NI>
__device__ __forceinline__ void gg_scale_rows(const GroupedArgs &g, f32x16 (&acc)[NI][2],
                                              const float *extras, int wm) {
    if (!g.rowscale) return;
    const int fh = (threadIdx.x & 63) >> 5;
#pragma unroll
    for (int i = 0; i < NI; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float rs = extras[384 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * fh];
            acc[i][0][r] *= rs;
            acc[i][1][r] *= rs;
        }
}

// bf16 storage (spt_grouped_gemm_bf16 / _wgrad_bf16 / spt_rows_combine_bf16): widening is exact,
// narrowing is v_cvt_pk_bf16_f32 (round to nearest even), once per stored value
__device__ __forceinline__ float gg_bf(unsigned short b) { return __builtin_bit_cast(float, (unsigned)b << 16); }
__device__ __forceinline__ float4 gg_bf4(const unsigned short *p) {         // 8-byte aligned
    const uint2 v = *reinterpret_cast<const uint2 *>(p);
    return make_float4(__builtin_bit_cast(float, v.x << 16), __builtin_bit_cast(float, v.x & 0xffff0000u),
                       __builtin_bit_cast(float, v.y << 16), __builtin_bit_cast(float, v.y & 0xffff0000u));
}

// Epilogue of a (32 NI x 2) x 128 tile.  MFMA C layout: acc[i][j][r] =
// C[32 i + (r & 3) + 8 (r >> 2) + 4 (l >> 5)][32 j + (l & 31)] of the wave's (32 NI) x 64
// part.  Each wave transposes it through LDS, 32 rows at a time, into a row layout -- 16
// lanes x float4 = one 64-column row segment -- so that every global access (the stores, the
// h / s tiles of EPI_DACT, the bias) is 16 bytes per lane and 256 contiguous bytes per row,
// and a row dot is a 16-lane DPP reduction.  The caller has synchronised the workgroup: the
// operand tiles in `smem` are dead.
// (BF16: bias, out, out2, h_in and s_in hold bf16; the pdot rows are fp32 and optional.  HALVES: `w` may
// hold halves -- the image path's fp32 kernels; the register path never sees such a weight)
template <int NI, int EPI, bool BF16 = false, bool HALVES = !BF16>
__device__ __forceinline__ void gg_epilogue(const GroupedArgs &g, float *smem,
                                            f32x16 (&acc)[NI][2], int bucket, int row_lo,
                                            int row_hi, int col_tile, int wm, int wn,
                                            const float *extras, bool has_ext) {
    constexpr int CS_ROW = 64 + 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *cs = smem + wave * (32 * CS_ROW);
    const bool relu_exact = EPI == EPI_ACT && g.act == ACT_RELU && g.a_norm != nullptr;
    const int ccol = lane & 31, chalf = lane >> 5;
    const int rrow = lane >> 4, rcol = 4 * (lane & 15);
    const int pslot = 2 * col_tile + (wave & 1);   // this wave's half tile of columns
    const float *sh = (EPI == EPI_DACT) ? (g.s_in ? g.s_in : g.h_in) : nullptr;
    const int n = col_tile * GG_BN + wn + rcol;
    const bool vec = (g.N & 3) == 0;
    const bool vec_row = (g.ldo & 3) == 0;        // 16-byte aligned pieces of the N-wide rows
    float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (BF16 && g.bias) {
        const unsigned short *bp = reinterpret_cast<const unsigned short *>(g.bias) + (size_t)bucket * g.N + n;
        if (vec) {
            if (n < g.N) bias4 = gg_bf4(bp);
        } else {
            bias4.x = n + 0 < g.N ? gg_bf(bp[0]) : 0.f; bias4.y = n + 1 < g.N ? gg_bf(bp[1]) : 0.f;
            bias4.z = n + 2 < g.N ? gg_bf(bp[2]) : 0.f; bias4.w = n + 3 < g.N ? gg_bf(bp[3]) : 0.f;
        }
    } else if (g.bias) {
        const float *bp = g.bias + (size_t)bucket * g.N + n;
        if (vec) {
            if (n < g.N) bias4 = *reinterpret_cast<const float4 *>(bp);
        } else {
            bias4.x = n + 0 < g.N ? bp[0] : 0.f; bias4.y = n + 1 < g.N ? bp[1] : 0.f;
            bias4.z = n + 2 < g.N ? bp[2] : 0.f; bias4.w = n + 3 < g.N ? bp[3] : 0.f;
        }
    }
    // ReLU epilogue: this lane's four columns' share of the error bound (see below)
    float wn4[4] = {0.f, 0.f, 0.f, 0.f}, rn4[4] = {0.f, 0.f, 0.f, 0.f};
    if (EPI == EPI_ACT && relu_exact) {
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (n + e < g.N) {
                wn4[e] = g.w_norm[(size_t)bucket * g.N + n + e];
                rn4[e] = has_ext ? extras[128 + wn + rcol + e] : 0.0f;
            }
    }
#pragma unroll
    for (int i = 0; i < NI; i++) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * chalf;
            cs[row * CS_ROW + ccol] = acc[i][0][r];
            cs[row * CS_ROW + 32 + ccol] = acc[i][1][r];
        }
        // (a wave only reads what it wrote: no workgroup barrier)
        // (not unrolled: the body is long -- with the ReLU recomputation inlined eight times the
        // activation epilogues ran 30-45 us slower at the FFN shape; and requesting the saved
        // activations of all eight row groups of EPI_DACT ahead of an unrolled loop was measured
        // 15 us SLOWER than loading them inside it, 175 against 160 us)
        // EPI_DACT: the saved activations of row group t + 1 are requested while group t is worked on
        // (rows past the bucket end: clamped, never used)
        auto load_saved = [&](int t) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (EPI == EPI_DACT && BF16) {
                const int p = min(row_lo + wm + 32 * i + rrow + 4 * t, row_hi - 1);
                const size_t at = (size_t)p * g.ldo + n;
                const unsigned short *sb = reinterpret_cast<const unsigned short *>(sh);
                if (vec_row && n + 3 < g.N) {
                    v = gg_bf4(sb + at);
                } else {
                    v.x = n + 0 < g.N ? gg_bf(sb[at + 0]) : 0.f; v.y = n + 1 < g.N ? gg_bf(sb[at + 1]) : 0.f;
                    v.z = n + 2 < g.N ? gg_bf(sb[at + 2]) : 0.f; v.w = n + 3 < g.N ? gg_bf(sb[at + 3]) : 0.f;
                }
            } else if (EPI == EPI_DACT) {
                const int p = min(row_lo + wm + 32 * i + rrow + 4 * t, row_hi - 1);
                const size_t at = (size_t)p * g.ldo + n;
                if (vec_row && n + 3 < g.N) {
                    v = *reinterpret_cast<const float4 *>(sh + at);
                } else {
                    v.x = n + 0 < g.N ? sh[at + 0] : 0.f; v.y = n + 1 < g.N ? sh[at + 1] : 0.f;
                    v.z = n + 2 < g.N ? sh[at + 2] : 0.f; v.w = n + 3 < g.N ? sh[at + 3] : 0.f;
                }
            }
            return v;
        };
        float4 sv_next = load_saved(0);
#pragma unroll 1
        for (int t = 0; t < 8; t++) {
            const int row = rrow + 4 * t;
            const int p = row_lo + wm + 32 * i + row;
            const bool live = p < row_hi;
            const float4 c4 = *reinterpret_cast<const float4 *>(&cs[row * CS_ROW + rcol]);
            float c[4] = {c4.x, c4.y, c4.z, c4.w};
            const float b[4] = {bias4.x, bias4.y, bias4.z, bias4.w};
            const float rs = extras[384 + wm + 32 * i + row];
            const size_t at = (size_t)p * g.ldo + n;
            const float sv[4] = {sv_next.x, sv_next.y, sv_next.z, sv_next.w};
            if (EPI == EPI_DACT && t < 7) sv_next = load_saved(t + 1);
            float dot_h = 0.0f, dot_s = 0.0f;
            float pre[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                float v = fmaf(rs, b[e], c[e]);         // the accumulators are scaled already
                if (EPI == EPI_DACT) {
                    const float hv = g.s_in ? act_forward(g.act, sv[e]) : sv[e];
                    dot_h = fmaf(v, hv, dot_h);
                }
                pre[e] = v;
                if (EPI == EPI_ACT) v = act_forward(g.act, v);
                if (EPI == EPI_DACT) {
                    v *= act_derivative(g.act, sv[e]);
                    dot_s = fmaf(v, sv[e], dot_s);
                }
                c[e] = v;
            }
            if (EPI == EPI_ACT && relu_exact) {
                // ---- near the kink: |v| within the error bound of the split products ----
                // per product <= 2^-16 |a| |b| (hi.hi + hi.lo + lo.hi of RNE bf16 parts), so
                // |error of v| <= 2^-16 (rs |a_p| |w_n| + |a2_p| |b2_n|) by Cauchy-Schwarz; a
                // pre-activation inside 1.5 x that bound is recomputed as a plain fp32 dot product
                // by a whole wave (6e-4 of the elements at K = 1024: ~10 per tile)
                unsigned cand = 0;
                if (live) {
                    const float an = extras[256 + wm + 32 * i + row];      // rowscale |a row|
                    const float un2 = has_ext ? extras[wm + 32 * i + row] : 0.0f;
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const float bound = 2.2888e-5f * (an * wn4[e] + sqrtf(un2 * rn4[e]));
                        cand |= (n + e < g.N && fabsf(pre[e]) <= bound ? 1u : 0u) << e;
                    }
                }
                // queue them for relu_fix_kernel (one wave per element, all in parallel) ...
                if (cand && g.fix_list) {
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if (cand & (1u << e)) {
                            const unsigned seg = blockIdx.x % GG_FIX_SEGS;
                            const unsigned slot = atomicAdd(g.fix_count + 16 * seg, 1u);
                            if (slot < (unsigned)g.fix_cap) {
                                g.fix_list[(size_t)seg * g.fix_cap + slot] =
                                    make_int2(p, (n + e) | (bucket << 24));
                                cand &= ~(1u << e);
                            }
                        }
                }
                // ... or, without a queue (or with a full one), recompute here, wave by wave
                unsigned long long todo = __ballot(cand != 0);
                while (todo) {
                    const int owner = __ffsll(todo) - 1;
                    const unsigned m = __shfl(cand, owner, 64);
                    const int e = __ffs(m) - 1;
                    const float exact = gg_exact_preact<false, HALVES>(g, bucket, __shfl(p, owner, 64),
                                                        __shfl(n, owner, 64) + e, lane);
                    if (lane == owner) {
#pragma unroll
                        for (int ee = 0; ee < 4; ee++)
                            if (ee == e) {
                                pre[ee] = exact;
                                c[ee] = act_forward(g.act, exact);
                            }
                        cand &= ~(1u << e);
                    }
                    todo = __ballot(cand != 0);
                }
            }
            if (BF16 && EPI == EPI_PLAIN && g.accumulate && live) {
                const unsigned short *ob = reinterpret_cast<const unsigned short *>(g.out);
                if (vec_row && n + 3 < g.N) {
                    const float4 o4 = gg_bf4(ob + at);
                    c[0] += o4.x; c[1] += o4.y; c[2] += o4.z; c[3] += o4.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if (n + e < g.N) c[e] += gg_bf(ob[at + e]);
                }
            } else if (EPI == EPI_PLAIN && g.accumulate && live) {
                if (vec_row && n + 3 < g.N) {
                    const float4 o4 = *reinterpret_cast<const float4 *>(g.out + at);
                    c[0] += o4.x; c[1] += o4.y; c[2] += o4.z; c[3] += o4.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if (n + e < g.N) c[e] += g.out[at + e];
                }
            }
            if (BF16 && live) {
                unsigned short *ob = reinterpret_cast<unsigned short *>(g.out);
                unsigned short *pb = reinterpret_cast<unsigned short *>(g.out2);
                if (vec_row && n + 3 < g.N) {
                    *reinterpret_cast<uint2 *>(ob + at) = make_uint2(pack_bf16(c[0], c[1]), pack_bf16(c[2], c[3]));
                    if (EPI == EPI_ACT && pb)
                        *reinterpret_cast<uint2 *>(pb + at) =
                            make_uint2(pack_bf16(pre[0], pre[1]), pack_bf16(pre[2], pre[3]));
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if (n + e < g.N) {
                            ob[at + e] = round_bf16(c[e]);
                            if (EPI == EPI_ACT && pb) pb[at + e] = round_bf16(pre[e]);
                        }
                }
            } else if (live) {
                if (vec_row && n + 3 < g.N) {
                    {
                        *reinterpret_cast<float4 *>(g.out + at) = make_float4(c[0], c[1], c[2], c[3]);
                        if (EPI == EPI_ACT && g.out2)
                            *reinterpret_cast<float4 *>(g.out2 + at) =
                                make_float4(pre[0], pre[1], pre[2], pre[3]);
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if (n + e < g.N) {
                            g.out[at + e] = c[e];
                            if (EPI == EPI_ACT && g.out2) g.out2[at + e] = pre[e];
                        }
                }
            }
            if (EPI == EPI_DACT) {
                dot_h = group_sum<16>(dot_h);
                dot_s = group_sum<16>(dot_s);
                if (live && (lane & 15) == 0 && (!BF16 || g.pdot_main)) {
                    g.pdot_main[(size_t)p * g.pdot_ld + pslot] = dot_h;
                    g.pdot_act[(size_t)p * g.pdot_ld + pslot] = dot_s;
                }
            }
        }
    }
}

// K in segments, or a second term wider than one k-step or in 16-column segments: the forms only the
// register path takes -- and, for a weight stored in halves, the image path's segmented kernel
__host__ __device__ inline bool gg_segmented(const GroupedArgs &g) {
    return g.a_seg_k > 0 || (g.a2 && (g.R > GG_BK || g.b2_seg != 0));
}

struct GgWork {
    int bucket, row_lo, row_hi, col_tile, half;
};

// Work distribution.  `slots` workgroups run at a time (two per CU), so a launch of T tiles
// takes ceil(T / slots) rounds.  Measured on the register path with per-workgroup timestamps
// (P = 16384 rows ragged over 4 buckets, K = N = 1024): the tiles of the last, partial round
// ran one per CU for as long as a full round -- it is therefore cut into half-height tiles
// (64 x 128): twice as many workgroups.  The split is decided on the device -- bucket sizes
// never visit the host -- and workgroup ids are dispatched in order, so ids [0, main) take
// the full rounds, ids [main, main + 2 R) the halves of the R remaining tiles, and the rest of
// the (worst-case sized) grid exits at once.
__device__ __forceinline__ GgWork gg_find_work(const GroupedArgs &g) {
    GgWork w;
    w.bucket = -1;
    w.row_lo = w.row_hi = w.col_tile = 0;
    w.half = -1;
    const int n_col_tiles = (g.N + GG_BN - 1) / GG_BN;
    int row_tiles = 0;
    for (int i = 0; i < g.G; i++)
        row_tiles += (g.offsets[i + 1] - g.offsets[i] + GG_BM - 1) / GG_BM;
    const int total = row_tiles * n_col_tiles;
    const int main_tiles = (total / g.slots) * g.slots;
    const int rest = total - main_tiles;
    int id = blockIdx.x;
    int logical;
    // XCD-aware order inside each part: workgroups are dealt round-robin over the 8 XCDs
    // (each with its own 4 MiB L2); xcd_remap gives every XCD a contiguous run of logical
    // tiles, enumerated column-tile fastest, so the column tiles of one row tile (same A
    // panel) run back to back on one L2.
    if (id < main_tiles) {
        logical = (int)xcd_remap((unsigned)id, (unsigned)main_tiles);
    } else {
        id -= main_tiles;
        if (id >= 2 * rest) return w;
        const int h = (int)xcd_remap((unsigned)id, (unsigned)(2 * rest));
        logical = main_tiles + (h >> 1);
        w.half = h & 1;
    }
    w.col_tile = logical % n_col_tiles;
    int tile = logical / n_col_tiles;
    for (int i = 0; i < g.G; i++) {
        const int lo = g.offsets[i], hi = g.offsets[i + 1];
        const int tiles = (hi - lo + GG_BM - 1) / GG_BM;
        if (tile < tiles) {
            w.bucket = i;
            w.row_lo = lo + tile * GG_BM;
            w.row_hi = min(hi, w.row_lo + GG_BM);
            break;
        }
        tile -= tiles;
    }
    if (w.bucket >= 0 && w.half >= 0) {
        w.row_lo += (GG_BM / 2) * w.half;
        w.row_hi = min(w.row_hi, w.row_lo + GG_BM / 2);
        if (w.row_lo >= w.row_hi) w.bucket = -1;   // a ragged tile may have no second half
    }
    return w;
}

// ---- launchers of the operand-path units.  A kernel is launched only from the unit that defines
// it; the validation and the choice of the path are grouped_gemm.hip's (launch_grouped,
// launch_grouped_bf16).  Each returns SPT_OK or the HIP error of its launch. ----
using GgKernel = void (*)(GroupedArgs);     // every GEMM kernel's signature
// grouped_gemm_img.hip.  `operands`: both as pre-split bf16 images, or the weight as an image and the
// activation as its fp32 rows (image_path() returns these two), or bf16 tensors (spt_grouped_gemm_bf16*)
enum { GG_OPS_IMAGES = 1, GG_OPS_A32 = 2, GG_OPS_BF16 = 3 };
int launch_gemm_img(const GroupedArgs &g, int epilogue, bool ext, int operands, dim3 grid, hipStream_t s);
// grouped_gemm_regs.hip
int launch_gemm_regs(const GroupedArgs &g, int epilogue, bool ext, bool k_tail, dim3 grid, hipStream_t s);
// grouped_gemm_ring.hip: plain epilogue, GR_BM x GR_BN tiles, one workgroup per CU
constexpr int GR_BM = 128, GR_BN = 256;
int launch_gemm_ring(const GroupedArgs &g, bool ext, bool a32, dim3 grid, hipStream_t s);

}  // namespace spt

#endif  // SPT_GROUPED_GEMM_H
