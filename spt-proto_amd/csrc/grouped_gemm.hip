// grouped_gemm.hip -- token-bucketed grouped GEMM for the routed FFN and every frozen LoRA
// linear: fp32 semantics on the bf16 matrix cores.
//
// The reference evaluates a routed FFN with a Python loop over blocks, boolean-mask
// gathers (one device->host sync per block) and cuBLAS calls on the gathered rows
// (naive_gpt/layers/tuning/lora_ffn.py:87-111, layers/sparse/feedforward.py:66-85).
// Here the (token, block) pairs are sorted by block on the device; bucket g is the row
// range [offsets[g], offsets[g+1]) of the sorted order and ONE launch multiplies every
// bucket by its own weight block:
//
//     out[p, n] = rowscale[p] * ( sum_k A[src(p), k] * W_g(n, k)  +  bias[g, n] )  (+ A2 . B2_g^T)
//     src(p) = gather ? gather[p] : p          (fuses the token gather)
//     W_g(n, k) = w[g * gstride + n * ldn + k * ldk]
//         ldk == 1 : "BT" weights, k contiguous  (forward: x.W1_g^T, h.W2_g^T)
//         ldn == 1 : "BN" weights, n contiguous  (backward: dY.W2_g, dH.W1_g)
//
// Bucket sizes never visit the host: the grid is sized for the worst case
// (ceil(P/128) + G row tiles) and every workgroup finds its bucket from `offsets`.
//
// Arithmetic: an fp32 operand is split x = hi + lo (hi = RNE bf16 of x, lo = RNE bf16 of
// x - hi) and a product is three v_mfma_f32_32x32x16_bf16 (lo.hi + hi.lo + hi.hi, fp32
// accumulation): <= 2^-16 relative error per product at 1/5 of the time of the fp32 MFMA.
// One place cannot live with 2^-16: the pre-activation of a ReLU that lies within the error of
// zero (its derivative flips: an O(1) error in one token's gradients).  There the epilogue
// recomputes the element in plain fp32 (gg_epilogue: "near the kink").
//
// Two operand paths, one tile shape (128 x 128 per 256-thread workgroup, each wave a 64 x 64
// quadrant = 2 x 2 MFMA tiles, K in steps of 32), one epilogue:
//
//   * IMAGE path (gemm_tile_img): both operands arrive PRE-SPLIT as bf16 images in global
//     memory (spt_split_bf16: [row][k / 32][hi | lo][32], 128 contiguous bytes per row and
//     k-step) and go global -> LDS with global_load_lds_dwordx4, no registers, no VALU, no
//     ds_write in the k-loop; two LDS stages, the next step's 32 KiB in flight while the
//     current one is contracted, one barrier per k-step.  LDS tiles are conflict-free by an
//     XOR swizzle applied on the SOURCE address of each lane (the LDS side of an LDS-DMA is
//     lane-linear) and again on the fragment reads.
//   * REGISTER path (gemm_tile_regs): fp32 operands, split while they are staged
//     (global -> VGPR -> cvt -> ds_write).  Round 1's kernel; kept for callers without images
//     and for K % 32 != 0.
//
// Why the image path: per-phase shader-clock stamps of the register path
// had a k-step at 4390 cycles of which 1355 were the split + 16 ds_write_b64 per lane and
// 768 matrix-pipe time: the VGPR -> LDS store path, not the matrix cores, set the pace.
//
// The units (grouped_gemm.h: what they share, and the launchers this file calls):
//   grouped_gemm.hip        this file: the C entries, validation and choice of the path
//                           (launch_grouped, launch_grouped_bf16), and the kernels beside the GEMM:
//                           split_bf16_kernel, split_f16_kernel, relu_fix_kernel, rows_combine(_bf16)_kernel
//   grouped_gemm_img.hip    the IMAGE path (fp32 semantics and bf16 tensors)
//   grouped_gemm_ring.hip   the image path as a loader / consumer ring (opt-in, SPT_GEMM_RING=1)
//   grouped_gemm_regs.hip   the REGISTER path
//   grouped_wgrad.hip       the weight gradient (spt_grouped_gemm_wgrad*), self-contained
//   grouped_image.h         the LDS layouts of pre-split tiles and their fragment readers
//   split_bf16.h            the split and the three-term product (the whole library's)
#include "grouped_gemm.h"
#include <stdlib.h>

namespace spt {

// fp32 [rows, cols] (leading dimension ld) -> the bf16 image [row][cols / 32][hi | lo][32]:
// a thread converts 8 consecutive columns (32 bytes in, 16 + 16 bytes out); columns past
// `cols` inside the last block are zero.
__global__ __launch_bounds__(256) void split_bf16_kernel(const float *__restrict__ src,
                                                         char *__restrict__ img, long long rows,
                                                         int cols, long long ld, int blocks) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long chunk_row = idx >> 2;               // (row, block)
    const int c = (int)(idx & 3);
    const long long row = chunk_row / blocks;
    const int kb = (int)(chunk_row - row * blocks);
    if (row >= rows) return;
    const int col = kb * 32 + c * 8;
    const float *p = src + row * ld + col;
    float x[8];
    if (col + 8 <= cols) {
        const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
    } else {
#pragma unroll
        for (int e = 0; e < 8; e++) x[e] = col + e < cols ? p[e] : 0.0f;
    }
    const Frag f = split8(x);
    char *dst = img + (chunk_row * 128) + c * 16;
    *reinterpret_cast<uint4 *>(dst) = f.hi;
    *reinterpret_cast<uint4 *>(dst + 64) = f.lo;
}

// The same image from IEEE halves [rows, cols] (spt_split_f16): a thread's 8 columns are ONE 16-byte
// load, widened (exact: every half is an fp32 value) and split as above -- byte for byte the image
// of the fp32 upcast, read from half the bytes.
__global__ __launch_bounds__(256) void split_f16_kernel(const _Float16 *__restrict__ src,
                                                        char *__restrict__ img, long long rows,
                                                        int cols, long long ld, int blocks) {
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long chunk_row = idx >> 2;               // (row, block)
    const int c = (int)(idx & 3);
    const long long row = chunk_row / blocks;
    const int kb = (int)(chunk_row - row * blocks);
    if (row >= rows) return;
    const int col = kb * 32 + c * 8;
    const _Float16 *p = src + row * ld + col;
    float x[8];
    if (col + 8 <= cols) {
        const h8 v = *reinterpret_cast<const h8 *>(p);
#pragma unroll
        for (int e = 0; e < 8; e++) x[e] = (float)v[e];
    } else {
#pragma unroll
        for (int e = 0; e < 8; e++) x[e] = col + e < cols ? (float)p[e] : 0.0f;
    }
    const Frag f = split8(x);
    char *dst = img + (chunk_row * 128) + c * 16;
    *reinterpret_cast<uint4 *>(dst) = f.hi;
    *reinterpret_cast<uint4 *>(dst + 64) = f.lo;
}

// The queue of the GEMM in front of a ReLU: one wave per queued (row, column), recomputed in
// fp32 and written over what the epilogue stored.  (In the epilogue itself each costs the wave
// that found it a serial ~2 us of dependent loads: 80 us of a 120 us GEMM at the FFN shape.)
__global__ __launch_bounds__(256) void relu_fix_kernel(GroupedArgs g) {
    // grid = 4 GG_FIX_SEGS workgroups: 16 waves per segment
    const int lane = threadIdx.x & 63;
    const unsigned seg = blockIdx.x % GG_FIX_SEGS;
    const unsigned wave = (blockIdx.x / GG_FIX_SEGS) * 4 + (threadIdx.x >> 6);
    const unsigned count = min(g.fix_count[16 * seg], (unsigned)g.fix_cap);
    for (unsigned i = wave; i < count; i += 16) {
        const int2 q = g.fix_list[(size_t)seg * g.fix_cap + i];
        const int p = q.x, n = q.y & 0xFFFFFF, bucket = (unsigned)q.y >> 24;
        // an entry is an ADDRESS in the making: one that is not a cell of this launch's output (a
        // stale counter or list, as the out-of-order memset node of round 3 produced) is skipped,
        // not dereferenced
        if (p < 0 || p >= g.P || n >= g.N || bucket >= g.G) continue;
        const float exact = gg_exact_preact<true>(g, bucket, p, n, lane);
        if (lane == 0) {
            g.out[(size_t)p * g.ldo + n] = act_forward(g.act, exact);
            if (g.out2) g.out2[(size_t)p * g.ldo + n] = exact;
        }
    }
}

// y[t, :] = bias + sum_{j < k} rows[pos[t * k + j], :]  -- the un-bucketing of the routed
// FFN (reference: `y[mask] += ...` per block, lora_ffn.py:107-111): a gather in a fixed
// order instead of a scatter-add, so the result is deterministic.
// side != null: out[t, :] += sum_{j < ns} side[t, j] * side_w[j, :] on top (a per-token rank-ns
// product: the router's share of the routed FFN's input gradient, d logit . W_router, which would
// otherwise be a library GEMM with a 4-wide contraction and an addition pass)
__global__ __launch_bounds__(256) void rows_combine_kernel(
    const float *__restrict__ rows, const int32_t *__restrict__ pos,
    const float *__restrict__ bias, float *__restrict__ out, int n_tokens, int k, int d4,
    const float *__restrict__ side, const float *__restrict__ side_w, int ns) {
    const int t = blockIdx.x;
    for (int c = threadIdx.x; c < d4; c += 256) {
        float4 acc = bias ? reinterpret_cast<const float4 *>(bias)[c]
                          : make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < k; j++) {
            const int p = pos[(size_t)t * k + j];
            const float4 v = reinterpret_cast<const float4 *>(rows + (size_t)p * d4 * 4)[c];
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        if (side) {
            for (int j = 0; j < ns; j++) {
                const float s = side[(size_t)t * ns + j];
                const float4 w = reinterpret_cast<const float4 *>(side_w + (size_t)j * d4 * 4)[c];
                acc.x = fmaf(s, w.x, acc.x); acc.y = fmaf(s, w.y, acc.y);
                acc.z = fmaf(s, w.z, acc.z); acc.w = fmaf(s, w.w, acc.w);
            }
        }
        reinterpret_cast<float4 *>(out + (size_t)t * d4 * 4)[c] = acc;
    }
}

// spt_rows_combine_bf16: the same gather-sum over bf16 rows / bias, in fp32 in the same order, one
// rounding at the store (four columns per thread)
__global__ __launch_bounds__(256) void rows_combine_bf16_kernel(
    const unsigned short *__restrict__ rows, const int32_t *__restrict__ pos,
    const unsigned short *__restrict__ bias, unsigned short *__restrict__ out, int k, int d4) {
    const int t = blockIdx.x;
    for (int c = threadIdx.x; c < d4; c += 256) {
        float4 acc = bias ? gg_bf4(bias + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < k; j++) {
            const int p = pos[(size_t)t * k + j];
            const float4 v = gg_bf4(rows + (size_t)p * d4 * 4 + 4 * c);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        *reinterpret_cast<uint2 *>(out + (size_t)t * d4 * 4 + 4 * c) =
            make_uint2(pack_bf16(acc.x, acc.y), pack_bf16(acc.z, acc.w));
    }
}

}  // namespace spt

using namespace spt;

static int resident_slots() {
    static int slots = 0;
    if (slots == 0) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess) return -1;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            return -1;
        slots = GG_SLOTS_PER_CU * cus;
    }
    return slots;
}

// The image path takes a GEMM when both images are given, K is a whole number of k-steps and
// the group offsets of the weight fall on image rows / 128-byte blocks.
// -> 0: register path; GG_OPS_IMAGES (1): both operands as images; GG_OPS_A32 (2): the weight as an
// image, the activation as its fp32 rows (16-byte aligned, lda % 4 == 0: one LDS-DMA lane moves 16 bytes)
static int image_path(GroupedArgs &g, int epilogue) {
    if (!g.w_img || (!g.a_img && !g.a)) return 0;
    if (g.K % GG_BK != 0) return 0;
    // (segments and a wide second term: the register path's -- but for a weight in halves, which runs them
    // from its image and the activation's fp32 rows: grouped_gemm_img.hip, the segmented kernel)
    if (gg_segmented(g) && (!g.w_f16 || g.a_img || epilogue != EPI_PLAIN)) return 0;
    const long long row_len = g.ldk == 1 ? g.ldn : g.ldk;       // elements of one weight row
    if (row_len <= 0 || g.gstride % 32 != 0 || row_len % 32 != 0) return 0;
    g.w_grow = g.gstride / row_len;
    g.w_gblk = (int)((g.gstride % row_len) / 32);
    g.w_rowb = (row_len / 32) * 128;
    if (g.a_img) {
        g.a_rowb = (long long)(g.K / 32) * 128;
        return GG_OPS_IMAGES;
    }
    if ((reinterpret_cast<uintptr_t>(g.a) & 15) != 0 || g.lda % 4 != 0) return 0;
    g.a_rowb = (long long)g.lda * 4;
    return GG_OPS_A32;
}

static int launch_grouped(GroupedArgs g, int epilogue, void *stream) {
    if ((!g.a && !g.a_img) || (!g.w && !g.w_img) || !g.offsets || !g.out) return SPT_EINVAL;
    if (g.P <= 0 || g.K <= 0 || g.N <= 0 || g.G <= 0) return SPT_EINVAL;
    if (g.a_seg_k < 0 || g.lda < (g.a_seg_k > 0 ? g.a_seg_k : g.K)) return SPT_EINVAL;
    if (g.a_seg_k > 0) {
        if (g.a_seg_k % GG_BK != 0 || g.K % g.a_seg_k != 0 || g.a_seg_stride % 4 != 0) return SPT_ESHAPE;
        if (epilogue != EPI_PLAIN || !g.a) return SPT_EUNSUP;
    }
    if (g.ldo == 0) g.ldo = g.N;
    if (g.ldo < g.N) return SPT_EINVAL;
    if (g.accumulate && epilogue != EPI_PLAIN) return SPT_EUNSUP;
    if (g.K % 4 != 0 || g.lda % 4 != 0) return SPT_ESHAPE;       // float4 rows of A
    // 16-byte aligned weight rows (halves: 8, four per load); the queue's counters and int2 entries
    if ((reinterpret_cast<uintptr_t>(g.w) & (g.w_f16 ? 7 : 15)) != 0) return SPT_ESHAPE;
    if ((reinterpret_cast<uintptr_t>(g.fix_count) & 15) != 0) return SPT_ESHAPE;
    if (g.ldk != 1 && g.ldn != 1) return SPT_EUNSUP;
    if (g.ldk == 1 && (g.ldn % 4 != 0 || g.gstride % 4 != 0)) return SPT_ESHAPE;
    if (g.ldk != 1 && (g.ldk % 4 != 0 || g.N % 4 != 0 || g.gstride % 4 != 0)) return SPT_ESHAPE;
    const bool ext = g.a2 != nullptr;
    if (ext) {
        if (!g.b2 || g.R <= 0 || g.R > 2 * GG_BK) return SPT_EINVAL;
        if (g.R > GG_BK && epilogue != EPI_PLAIN) return SPT_EUNSUP;
        if (g.b2_seg != 0 && (g.b2_seg % 4 != 0 || g.R % 16 != 0 || epilogue != EPI_PLAIN)) return SPT_ESHAPE;
        if (g.R % 4 != 0 || g.lda2 % 4 != 0 || g.lda2 < g.R || g.b2_ldn % 4 != 0 ||
            g.b2_gstride % 4 != 0)
            return SPT_ESHAPE;
    }
    if (epilogue < EPI_PLAIN || epilogue > EPI_DACT) return SPT_EINVAL;
    if (epilogue != EPI_PLAIN && (g.act < ACT_RELU || g.act > ACT_SILU)) return SPT_EUNSUP;
    const unsigned row_tiles = (unsigned)((g.P + GG_BM - 1) / GG_BM + g.G);
    const unsigned col_tiles = (unsigned)((g.N + GG_BN - 1) / GG_BN);
    if ((unsigned long long)row_tiles * col_tiles > 0x3FFFFFFFull) return SPT_EUNSUP;
    if (epilogue == EPI_ACT && g.act == ACT_RELU) {
        // the near-the-kink recomputation reads the operands themselves (w_f16: the weight's halves)
        if (!g.a_norm || !g.w_norm || !g.a || !g.w) return SPT_EINVAL;
    }
    if (epilogue == EPI_DACT) {
        if ((!g.h_in && !g.s_in) || !g.pdot_main || !g.pdot_act) return SPT_EINVAL;
        if (!g.s_in && g.act != ACT_RELU) return SPT_EINVAL;   // only ReLU is a function of h
        if (g.pdot_ld < (int)(2 * col_tiles)) return SPT_ESHAPE;
    }
    // worst case: every tile in the halved last round
    dim3 grid(2 * row_tiles * col_tiles);
    hipStream_t s = (hipStream_t)stream;
    g.slots = resident_slots();
    if (g.slots <= 0) return SPT_EINVAL;
    const int img = image_path(g, epilogue);
    if (!img && (!g.a || !g.w)) return SPT_EUNSUP;              // images only, but not usable
    if (!img && g.w_f16) return SPT_EUNSUP;                     // no register-operand form of halves
    // the loader / consumer ring (grouped_gemm_ring.hip, which says why it is opt-in): plain epilogue, image
    // path, nothing to add into; one workgroup per CU (read at every call: tests switch it inside one process)
    const char *ring_env = getenv("SPT_GEMM_RING");
    const bool ring_on = ring_env && ring_env[0] == '1';
    if (img && epilogue == EPI_PLAIN && !g.accumulate && ring_on && !g.w_f16 && (g.slots % 16) == 0 &&
        (long long)GR_BM * g.ldo * 4 < 0x7fffffffLL && (!ext || g.R <= GG_BK))
        return launch_gemm_ring(g, ext, img == GG_OPS_A32, dim3(g.slots / GG_SLOTS_PER_CU), s);
    const bool k_tail = (g.K % GG_BK) != 0;
    const bool relu_queue = epilogue == EPI_ACT && g.act == ACT_RELU && g.fix_list && g.G < 256 &&
                            g.N < (1 << 24);
    if (relu_queue) {
        SPT_ZERO_WORDS(g.fix_count, GG_FIX_SEGS * 16, s);
        SPT_LAUNCH_CHECK();
    } else
        g.fix_list = nullptr;
    const int rc = img ? launch_gemm_img(g, epilogue, ext, img, grid, s)
                       : launch_gemm_regs(g, epilogue, ext, k_tail, grid, s);
    if (rc != SPT_OK) return rc;
    if (relu_queue) {
        hipLaunchKernelGGL(relu_fix_kernel, dim3(4 * GG_FIX_SEGS), dim3(256), 0, s, g);
        SPT_LAUNCH_CHECK();
    }
    return SPT_OK;
}

extern "C" int spt_grouped_gemm(const float *a, const int32_t *gather, const float *w,
                                const float *bias, const float *rowscale,
                                const int32_t *offsets, float *out, int n_rows, int k, int n,
                                int n_groups, int lda, long long w_group_stride, int w_ldn,
                                int w_ldk, void *stream) {
    GroupedArgs g = {};
    g.a = a; g.gather = gather; g.w = w; g.bias = bias; g.rowscale = rowscale;
    g.offsets = offsets; g.out = out;
    g.P = n_rows; g.K = k; g.N = n; g.G = n_groups; g.lda = lda;
    g.gstride = w_group_stride; g.ldn = w_ldn; g.ldk = w_ldk;
    return launch_grouped(g, EPI_PLAIN, stream);
}

extern "C" int spt_grouped_gemm_pdot_width(int n) { return n > 0 ? 2 * ((n + GG_BN - 1) / GG_BN) : 0; }

static GroupedArgs args_of(const SptGroupedGemm *d) {
    GroupedArgs g = {};
    g.a = d->a; g.gather = d->gather; g.w = d->w; g.bias = d->bias; g.rowscale = d->rowscale;
    g.offsets = d->offsets; g.out = d->out;
    g.P = d->n_rows; g.K = d->k; g.N = d->n; g.G = d->n_groups; g.lda = d->lda;
    g.gstride = d->w_group_stride; g.ldn = d->w_ldn; g.ldk = d->w_ldk;
    g.a2 = d->a2; g.gather2 = d->gather2; g.b2 = d->b2; g.lda2 = d->lda2; g.R = d->r;
    g.b2_gstride = d->b2_group_stride; g.b2_ldn = d->b2_ldn;
    g.act = d->activation; g.out2 = d->out2; g.h_in = d->h_in; g.s_in = d->s_in;
    g.pdot_main = d->pdot_main; g.pdot_act = d->pdot_act; g.pdot_ld = d->pdot_ld;
    g.a_img = reinterpret_cast<const char *>(d->a_image);
    g.w_img = reinterpret_cast<const char *>(d->w_image);
    g.a_norm = d->a_norm; g.w_norm = d->w_norm;
    g.ldo = d->ldo;
    g.accumulate = d->accumulate;
    g.a_seg_k = d->a_seg_k; g.a_seg_stride = d->a_seg_stride;
    g.b2_seg = d->b2_seg_stride;
    const long long header = GG_FIX_SEGS * 64;
    if (d->relu_queue && d->relu_queue_bytes >= header + GG_FIX_SEGS * 8) {
        g.fix_count = reinterpret_cast<unsigned *>(d->relu_queue);
        g.fix_list = reinterpret_cast<int2 *>(reinterpret_cast<char *>(d->relu_queue) + header);
        const long long cap = (d->relu_queue_bytes - header) / 8 / GG_FIX_SEGS;
        g.fix_cap = (int)(cap > 0x7FFFFF ? 0x7FFFFF : cap);
    }
    return g;
}

extern "C" int spt_grouped_gemm_fused(const SptGroupedGemm *d, void *stream) {
    if (!d) return SPT_EINVAL;
    return launch_grouped(args_of(d), d->epilogue, stream);
}

// `w` as IEEE halves: the k-loop kernels of the image path as they are (they read w_image alone); the
// recomputation in front of a ReLU widens the halves it loads.  Always the default kernels.
extern "C" int spt_grouped_gemm_fused_w16(const SptGroupedGemm *d, void *stream) {
    if (!d) return SPT_EINVAL;
    if ((!d->a && !d->a_image) || !d->w || !d->offsets || !d->out) return SPT_EINVAL;
    if (!d->w_image) return SPT_EUNSUP;
    if ((reinterpret_cast<uintptr_t>(d->w) & 7) != 0) return SPT_ESHAPE;      // four halves per load
    GroupedArgs g = args_of(d);
    g.w_f16 = 1;
    return launch_grouped(g, d->epilogue, stream);
}

static int image_path_of(const SptGroupedGemm *d, int w_f16) {
    if (!d) return 0;
    GroupedArgs g = {};
    g.w_f16 = w_f16;
    g.K = d->k; g.gstride = d->w_group_stride; g.ldn = d->w_ldn; g.ldk = d->w_ldk;
    g.act = d->activation;
    g.a = d->a; g.lda = d->lda;
    g.a2 = d->a2; g.R = d->r; g.a_seg_k = d->a_seg_k; g.b2_seg = d->b2_seg_stride;
    g.a_img = reinterpret_cast<const char *>(d->a_image);
    g.w_img = reinterpret_cast<const char *>(d->w_image);
    return image_path(g, d->epilogue);
}

extern "C" int spt_grouped_gemm_image_path(const SptGroupedGemm *d) { return image_path_of(d, 0); }

// ... of spt_grouped_gemm_fused_w16: the one place that says which forms halves admit (image_path)
extern "C" int spt_grouped_gemm_image_path_w16(const SptGroupedGemm *d) {
    return image_path_of(d, 1);
}

extern "C" size_t spt_split_bf16_bytes(long long rows, int cols) {
    if (rows <= 0 || cols <= 0) return 0;
    return (size_t)rows * (size_t)((cols + 31) / 32) * 128;
}

extern "C" int spt_split_bf16(const float *src, void *image, long long rows, int cols,
                              long long ld, void *stream) {
    if (!src || !image) return SPT_EINVAL;
    if (rows <= 0 || cols <= 0 || ld < cols) return SPT_EINVAL;
    if (ld % 4 != 0 || (reinterpret_cast<uintptr_t>(src) & 15) != 0 ||
        (reinterpret_cast<uintptr_t>(image) & 15) != 0)
        return SPT_ESHAPE;
    const int blocks = (cols + 31) / 32;
    const long long threads = rows * blocks * 4;
    if ((threads + 255) / 256 > 0x7FFFFFFFll) return SPT_EUNSUP;
    hipLaunchKernelGGL(split_bf16_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, src, reinterpret_cast<char *>(image), rows, cols, ld,
                       blocks);
    SPT_LAUNCH_CHECK();
    return SPT_OK;
}

extern "C" int spt_split_f16(const void *src_f16, void *image, long long rows, int cols, long long ld,
                             void *stream) {
    if (!src_f16 || !image) return SPT_EINVAL;
    if (rows <= 0 || cols <= 0 || ld < cols) return SPT_EINVAL;
    if (ld % 8 != 0 || (reinterpret_cast<uintptr_t>(src_f16) & 15) != 0 ||
        (reinterpret_cast<uintptr_t>(image) & 15) != 0)
        return SPT_ESHAPE;
    const int blocks = (cols + 31) / 32;
    const long long threads = rows * blocks * 4;
    if ((threads + 255) / 256 > 0x7FFFFFFFll) return SPT_EUNSUP;
    hipLaunchKernelGGL(split_f16_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, static_cast<const _Float16 *>(src_f16),
                       reinterpret_cast<char *>(image), rows, cols, ld, blocks);
    SPT_LAUNCH_CHECK();
    return SPT_OK;
}

// float4 per lane from rows, bias (NULL: none) and to out
static bool rc_misaligned(const void *rows, const void *bias, const void *out) {
    return ((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(bias) |
             reinterpret_cast<uintptr_t>(out)) & 15) != 0;
}

extern "C" int spt_rows_combine(const float *rows, const int32_t *pos, const float *bias,
                                float *out, int n_tokens, int k, int d, void *stream) {
    if (!rows || !pos || !out) return SPT_EINVAL;
    if (n_tokens <= 0 || k <= 0 || d <= 0) return SPT_EINVAL;
    if (d % 4 != 0 || rc_misaligned(rows, bias, out)) return SPT_ESHAPE;
    hipLaunchKernelGGL(rows_combine_kernel, dim3((unsigned)n_tokens), dim3(256), 0,
                       (hipStream_t)stream, rows, pos, bias, out, n_tokens, k, d / 4, nullptr, nullptr, 0);
    SPT_LAUNCH_CHECK();
    return SPT_OK;
}

extern "C" int spt_rows_combine_side(const float *rows, const int32_t *pos, const float *bias,
                                     const float *side, const float *side_w, int n_side, float *out,
                                     int n_tokens, int k, int d, void *stream) {
    if (!rows || !pos || !out || !side || !side_w) return SPT_EINVAL;
    if (n_tokens <= 0 || k <= 0 || d <= 0 || n_side <= 0 || n_side > 64) return SPT_EINVAL;
    if (d % 4 != 0 || (reinterpret_cast<uintptr_t>(side_w) & 15) != 0 || rc_misaligned(rows, bias, out))
        return SPT_ESHAPE;
    hipLaunchKernelGGL(rows_combine_kernel, dim3((unsigned)n_tokens), dim3(256), 0,
                       (hipStream_t)stream, rows, pos, bias, out, n_tokens, k, d / 4, side, side_w, n_side);
    SPT_LAUNCH_CHECK();
    return SPT_OK;
}

// spt_grouped_gemm_bf16 and, with `x` != NULL, spt_grouped_gemm_bf16_ext
static int launch_grouped_bf16(const SptGroupedGemmBf16 *d, const SptGroupedGemmBf16Ext *x, void *stream) {
    if (!d) return SPT_EINVAL;
    if (!d->a || !d->w || !d->offsets || !d->out) return SPT_EINVAL;
    if (d->n_rows <= 0 || d->k <= 0 || d->n <= 0 || d->n_groups <= 0 || d->lda < d->k) return SPT_EINVAL;
    const int epilogue = d->epilogue;
    if (epilogue < EPI_PLAIN || epilogue > EPI_DACT) return SPT_EINVAL;
    if (epilogue != EPI_PLAIN && (d->activation < ACT_RELU || d->activation > ACT_SILU)) return SPT_EUNSUP;
    if (d->accumulate && epilogue != EPI_PLAIN) return SPT_EUNSUP;
    const long long ldo = d->ldo == 0 ? d->n : d->ldo;
    if (ldo < d->n || d->w_group_stride < 0) return SPT_EINVAL;
    if (d->w_ldk != 1 && d->w_ldn != 1) return SPT_EUNSUP;
    // LDS-DMA moves 16 bytes per lane: 16-byte aligned rows of both operands; a stage is 64 k
    const auto misaligned = [](const void *p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & m) != 0; };
    if (d->k % (2 * GG_BK) != 0 || d->lda % 8 != 0 || d->w_group_stride % 8 != 0) return SPT_ESHAPE;
    if (misaligned(d->a, 15) || misaligned(d->w, 15)) return SPT_ESHAPE;
    if (d->w_ldk == 1 && (d->w_ldn < d->k || d->w_ldn % 8 != 0)) return SPT_ESHAPE;
    if (d->w_ldk != 1 && (d->w_ldk < d->n || d->w_ldk % 8 != 0 || d->n % 32 != 0)) return SPT_ESHAPE;
    // the epilogue's 4-column pieces: 8-byte aligned bf16 tensors
    if (misaligned(d->out, 7) || misaligned(d->out2, 7) || misaligned(d->bias, 7) || misaligned(d->h_in, 7) ||
        misaligned(d->s_in, 7))
        return SPT_ESHAPE;
    const unsigned row_tiles = (unsigned)((d->n_rows + GG_BM - 1) / GG_BM + d->n_groups);
    const unsigned col_tiles = (unsigned)((d->n + GG_BN - 1) / GG_BN);
    if ((unsigned long long)row_tiles * col_tiles > 0x3FFFFFFFull) return SPT_EUNSUP;
    if (epilogue == EPI_DACT) {
        if (!d->h_in && !d->s_in) return SPT_EINVAL;
        if (!d->s_in && d->activation != ACT_RELU) return SPT_EINVAL;   // only ReLU is a function of h
        if (!d->pdot_main != !d->pdot_act) return SPT_EINVAL;
        if (d->pdot_main && d->pdot_ld < (int)(2 * col_tiles)) return SPT_ESHAPE;
    }
    GroupedArgs g = {};
    // (the bf16 tensors travel in GroupedArgs' float pointers; the kernel reads them as bf16)
    g.a = static_cast<const float *>(d->a); g.gather = d->gather; g.w = static_cast<const float *>(d->w);
    g.bias = static_cast<const float *>(d->bias); g.rowscale = d->rowscale;
    g.offsets = d->offsets; g.out = static_cast<float *>(d->out);
    g.P = d->n_rows; g.K = d->k; g.N = d->n; g.G = d->n_groups; g.lda = d->lda;
    g.gstride = d->w_group_stride; g.ldn = d->w_ldn; g.ldk = d->w_ldk;
    g.ldo = ldo; g.accumulate = d->accumulate;
    g.act = d->activation; g.out2 = static_cast<float *>(d->out2);
    g.h_in = static_cast<const float *>(d->h_in); g.s_in = static_cast<const float *>(d->s_in);
    g.pdot_main = d->pdot_main; g.pdot_act = d->pdot_act; g.pdot_ld = d->pdot_ld;
    g.a_rowb = (long long)d->lda * 2;
    g.w_rowb = (long long)(d->w_ldk == 1 ? d->w_ldn : d->w_ldk) * 2;
    if (x) {
        // the K extension: fp32 a2 rows as float4 (16 bytes), bf16 b2 rows as four values (8 bytes)
        if (!x->a2 || !x->b2 || x->r <= 0 || x->lda2 < x->r || x->b2_ldn < x->r || x->b2_group_stride < 0)
            return SPT_EINVAL;
        if (x->r % 4 != 0 || x->r > GG_BK) return SPT_EUNSUP;
        if (x->lda2 % 4 != 0 || x->b2_ldn % 4 != 0 || x->b2_group_stride % 4 != 0 || misaligned(x->a2, 15) ||
            misaligned(x->b2, 7))
            return SPT_ESHAPE;
        g.a2 = x->a2; g.gather2 = x->gather2; g.b2 = static_cast<const float *>(x->b2);
        g.lda2 = x->lda2; g.R = x->r; g.b2_gstride = x->b2_group_stride; g.b2_ldn = x->b2_ldn;
    }
    g.slots = resident_slots();
    if (g.slots <= 0) return SPT_EINVAL;
    const dim3 grid(2 * row_tiles * col_tiles);
    hipStream_t s = (hipStream_t)stream;
    return launch_gemm_img(g, epilogue, x != nullptr, GG_OPS_BF16, grid, s);
}

extern "C" int spt_grouped_gemm_bf16(const SptGroupedGemmBf16 *d, void *stream) {
    return launch_grouped_bf16(d, nullptr, stream);
}

extern "C" int spt_grouped_gemm_bf16_ext(const SptGroupedGemmBf16 *d, const SptGroupedGemmBf16Ext *ext,
                                         void *stream) {
    if (!ext) return SPT_EINVAL;
    return launch_grouped_bf16(d, ext, stream);
}

extern "C" int spt_rows_combine_bf16(const void *rows, const int32_t *pos, const void *bias, void *out,
                                     int n_tokens, int k, int d, void *stream) {
    if (!rows || !pos || !out) return SPT_EINVAL;
    if (n_tokens <= 0 || k <= 0 || d <= 0) return SPT_EINVAL;
    if (d % 4 != 0 || ((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(bias) |
                        reinterpret_cast<uintptr_t>(out)) & 7) != 0)
        return SPT_ESHAPE;
    hipLaunchKernelGGL(rows_combine_bf16_kernel, dim3((unsigned)n_tokens), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const unsigned short *>(rows), pos, static_cast<const unsigned short *>(bias),
                       static_cast<unsigned short *>(out), k, d / 4);
    SPT_LAUNCH_CHECK();
    return SPT_OK;
}
