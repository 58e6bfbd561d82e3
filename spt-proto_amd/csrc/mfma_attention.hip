// mfma_attention.hip -- the sparse attention core on the matrix cores (gfx950).
//
// Reference: SparseVanillaAttentionV2._get_attn / _apply_attn
// (naive_gpt/layers/sparse/attention.py:106-142) and its backward through kernels/sddmm.py,
// kernels/spmm.py, extension/softmax.cu.  Same mathematics as fused_attention.hip, different
// machine mapping.  At the densities lookup produces (Z / S = 1/8 at S = 512) a gather kernel
// moves a 256-byte K or V row through LDS per CSR entry and is LDS-bandwidth bound at ~1/5 of
// the HBM roofline.  Here the CSR rows only decide WHICH cells of a dense
// 32 x 32 score tile are alive:
//
//   tile      D[j, i] = sum_e K[j, e] Q[i, e]       v_mfma_f32_32x32x16_bf16, fp32 accumulate
//   cells     p[j, i] = m[i, j] * exp(clamp(scale * D[j, i]))   m = multiplicity of column j in
//             CSR row i (0 for most cells; > 1 only for lookup's zero padding), col <= row only
//   product   Y[i, :] += sum_j p[j, i] V[j, :]      the accumulator tile is the next A operand
//   row       y = Y / max(1e-9, sum_j p)            (softmax.cu:30; no max-subtraction, as there)
//
// fp32 operands are split into two bf16 halves x = hi + lo (hi = RNE(x), lo = RNE(x - hi)) and
// every product is three MFMAs (lo*hi + hi*lo + hi*hi): relative error <= 2^-16 per product,
// 50x inside the 1e-3 parity bar, at 1/5 of the fp32-MFMA cost.
//
// A workgroup of 8 waves owns 256 rows of one (sample, head) slice, a wave 32 rows.  K and V
// stream through LDS 32 keys at a time as bf16 images (K row-major for the A operand, V
// transposed for the B operand, double-buffered, one barrier per tile); a wave skips the
// tiles its rows have no entries in, which includes everything right of the diagonal
// (softmax.cu:19-31 masks col > row).  The multiplicities m come from a one-off pass over the
// CSR (spt_attention_mfma_prepare) that stores, per (32-row tile, 32-key tile), the 1 KiB of
// cell counts already permuted into the accumulator layout: a consumer lane loads its 16
// bytes with one global_load_dwordx4 a tile ahead and touches no LDS for them.
#include "mfma_frag.h"

// Compiled three times: for d_head 64 (this is the unit that also holds the C entry points) and, with
// -DMA_E_VALUE=128 / 80, for d_head 128 / 80 into namespace spt::e128 / spt::e80
// (mfma_attention_e128.o / _e80.o), to which the entry points dispatch.
MA_NS_OPEN

// Row tile rt costs rt + 1 key tiles, so contiguous 256-row blocks would give the workgroups
// of a slice 36 : 100 of the work at S = 512 and, two to a CU, idle CUs at the end.  Folded
// instead: workgroup g of a slice takes row tiles 4g .. 4g+3 (waves 0-3) and the mirror
// images RTpad-4g-4 .. RTpad-4g-1 (waves 4-7; one short and one long wave per SIMD).
__device__ __forceinline__ int folded_row_tile(int g, int blocks_per_batch, int wave) {
    constexpr int HALF = MA_WAVES / 2;
    return wave < HALF ? HALF * g + wave
                       : MA_WAVES * blocks_per_batch - HALF * (g + 1) + (wave - HALF);
}

// ===================================== forward =============================================
// grid: batch * ceil(S / 256) workgroups.

// exp(clamp(scale d)) = exp2(med3(d * scale log2e, -+clamp log2e)); without a clamp the
// exponent is bounded at 2^127 so that dead cells (m = 0) stay 0 and not 0 * inf
struct ScoreMap {
    float sl2, bound;
    __device__ __forceinline__ ScoreMap(float scale, float clampv) {
        const float log2e = 1.4426950408889634f;
        sl2 = scale * log2e;
        bound = clampv > 0.0f ? clampv * log2e : 127.0f;
    }
    // d: the tile value with sl2 already folded into one operand (q or k pre-multiplied)
    __device__ __forceinline__ float exp_of(float d) const {
        return __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(d, -bound, bound));
    }
    // the clamp passes gradient strictly inside (-clamp, clamp) (attention.py:125-127 through
    // spt_softmax_backward_clamped: |clamped| < clamp)
    __device__ __forceinline__ bool inside(float d) const { return fabsf(d) < bound; }
    // the largest value `inside` accepts
    __device__ __forceinline__ float bound_in() const {
        return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, bound) - 1u);
    }
};

// ---- the clamp's gradient mask, decided on the EXACT score (round 4) ----
// `v = clamp(scale * sddmm, -10, 10)` (attention.py:125-127) passes gradient only inside the clamp.
// That mask is a discontinuous function of the score, and a score formed from split-bf16 operands
// carries an error of up to
//     (2^-15 (1 + 2^-7) [the lo * lo term, <= 2^-16, and the rounding of the two lo parts, <= 2^-17 each:
//     DESIGN.md section 3; 1.98 x 2^-16 measured on operands next to bf16 midpoints] + 3 E * 2^-24 [fp32
//     accumulation of the 3 E products, worst case]) * sum_e |q_e k_e|  <=  MA_SPLIT_ERR * |q| |k|
// so a cell that close to +-clamp can land on the other side of it than the reference's fp32 score
// (measured before this: 7e-3 of grad_q on a layer with 15 % of its scores on the clamp).  The
// backward kernels therefore recompute such cells -- |d| within eps of the bound, eps from the norm of
// the lane's own row and the slice-wide bound on the streamed operand's row norms that the forward
// left in `bounds` -- as the oracle does: an fp64 dot in ascending e, rounded to fp32, times scale in
// fp32, compared with the clamp.  A tile value on the wrong side is then moved onto the bound or just
// inside it, which `exp_of` and `inside` turn into the exact mask (the value changes by less than its
// own error; moving every recomputed cell to the bound changed probabilities by up to eps = 0.5 %).
// Cost on the common path: a scalar test per tile while no score of the slice can reach the clamp
// (Cauchy-Schwarz on the norms), else the smallest distance of the lane's 16 |d| from the bound and
// a ballot per tile; the recomputation
// sits behind a wave-uniform branch (about 1e-4 of the live cells of a layer with scores of
// standard deviation 10, none at all while the scores are O(1)).
constexpr float MA_SPLIT_ERR = (2.015625f + 3.0f * MA_E / 256.0f) * 1.52587890625e-5f;
struct ClampGuard {
    float thr;                 // bound - eps: a cell with | |d| - bound | <= eps calls for the recomputation
    float bound, eps;
    bool on;                   // false: no score of this wave can reach thr at all (Cauchy-Schwarz on the
                               // norms) -- the usual case, scores O(1): the tile loop then only tests a scalar
    // own2: |own row|^2 of this lane (unscaled operand); which: 1 = the streamed operand is K, 0 = Q
    __device__ __forceinline__ ClampGuard(const float *bounds, int b, int nslots, int which, float own2,
                                          const ScoreMap &sm, float clampv) {
        thr = __builtin_inff();
        bound = sm.bound;
        eps = 0.0f;
        on = false;
        if (bounds != nullptr && clampv > 0.0f) {
            float other2 = 0.0f;
            for (int g = 0; g < nslots; g++)
                other2 = fmaxf(other2, bounds[((size_t)b * MA_BOUND_SLOTS + g) * 2 + which]);
            // the WAVE's largest own row: one threshold per wave, held in a scalar register
#pragma unroll
            for (int off = 1; off < 32; off <<= 1) own2 = fmaxf(own2, __shfl_xor(own2, off, SPT_WAVE));
            const float reach = sqrtf(own2 * other2) * sm.sl2;      // |d| <= |own| |other| scale log2e
            thr = sm.bound - MA_SPLIT_ERR * reach;
            thr = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, thr)));
            eps = bound - thr;                                      // (as clamp_exact forms it)
            on = __builtin_amdgcn_readfirstlane((int)(reach * 1.0001f >= thr)) != 0;
        }
    }
    __device__ __forceinline__ bool wanted(const f32x16 &d) const {
#ifdef MA_NO_CLAMP_GUARD                                // (A/B builds: what the check costs)
        return false;
#endif
        if (!on) return false;
        // TWO-sided: the smallest distance of the lane's 16 |d| from the bound.  (The first form asked
        // for max |d| >= thr, which every tile answers with yes once scores lie BEYOND the clamp -- ten
        // steps into the bench's training run: max |score| 15-23 in the upper layers, and the key-owned
        // kernel went from 89 to 140-165 us there, all of it the second-level test behind the branch.)
        // (a cheaper necessary condition in front -- max |d| >= thr, 8 instructions and a ballot -- was
        // measured in the step: 105.7 / 80.8 us against 102.0 / 78.3 without it: not kept)
        float m = fminf(fabsf(fabsf(d[0]) - bound), fabsf(fabsf(d[1]) - bound));
#pragma unroll
        for (int r = 2; r < 16; r += 2)
            m = fminf(m, fminf(fabsf(fabsf(d[r]) - bound), fabsf(fabsf(d[r + 1]) - bound)));
        return __ballot(m <= eps) != 0ull;
    }
};
// extension/sddmm.cpp:27-69 as the oracle restates it: sum in fp64, e ascending, rounded once
template <typename T>
__device__ __forceinline__ float exact_dot(const T *a, const T *b) {
    double acc = 0.0;
#pragma unroll 1
    for (int e = 0; e < MA_E; e += 4) {
        const float4 x = ld4(a + e), y = ld4(b + e);
        acc = fma((double)x.x, (double)y.x, acc);
        acc = fma((double)x.y, (double)y.y, acc);
        acc = fma((double)x.z, (double)y.z, acc);
        acc = fma((double)x.w, (double)y.w, acc);
    }
    return (float)acc;
}
// d: the lane's 16 cells (own row x tile rows acc_row(r, h)); cw: their multiplicities as the
// four count words (byte form); dp: the tile's second product, which has nothing to do with the
// mask but is live here.  At the call sites the kernels hold 190-250 registers; this loop inlined
// beside them raised the allocation past 256 (spills inside the tile loop), as a non-inlined call
// the allocator kept the K / V fragments in scratch for the whole kernel, and in FRONT of the second
// product (where 16-32 registers fewer are live) the branch serialised the two MFMA chains: 205
// against 193 us for the backward pair.  So d and dp are parked in a wave-private LDS block for the
// duration of the loop -- a hand-placed spill, paid only inside the rare branch.
constexpr int MA_PARK = 32 * SPT_WAVE * 4;          // bytes per wave: d and dp, [register][lane]
// own: the own operand's slice base (rows of `ld` elements), own_row0: the wave's first own row
// (lane & 31 is added here); tile_rows: the streamed operand's tile (rows of `ld_tile` elements: with
// grouped key/value heads one of the two operands is K, whose rows are narrower than Q's); park0: the
// parking blocks' base (the wave's block is chosen here).  Everything lane-dependent is derived from
// rare_lane().
template <typename T>
__device__ __forceinline__ void clamp_exact(f32x16 &d, f32x16 &dp, char *park0, int wave, const uint4 &cw,
                                            float bound, float thr, const T *own, int own_row0, int S,
                                            const T *tile_rows, int ld, int ld_tile, float scale,
                                            float clampv) {
    const unsigned w[4] = {cw.x, cw.y, cw.z, cw.w};
    const float eps = bound - thr;
    unsigned near = 0, in = 0;
#pragma unroll
    for (int r = 0; r < 16; r++)
        if (((w[r >> 2] >> (8 * (r & 3))) & 0xffu) != 0u && fabsf(fabsf(d[r]) - bound) <= eps)
            near |= 1u << r;
    if (__ballot(near != 0u) == 0ull) return;       // close to the clamp, but no live cell is
    const int lane = rare_lane();
    float *park = reinterpret_cast<float *>(park0 + wave * MA_PARK) + lane;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        park[r * SPT_WAVE] = d[r];
        park[(16 + r) * SPT_WAVE] = dp[r];
    }
    asm volatile("" ::: "memory");                  // (no store-to-load forwarding past the loop)
    const T *own_row = own + (size_t)min(own_row0 + (lane & 31), S - 1) * ld;
    for (unsigned rem = near; rem != 0u; rem &= rem - 1u) {
        const int r = __builtin_ctz(rem);
        const float sc = exact_dot(own_row, tile_rows + (size_t)acc_row(r, lane >> 5) * ld_tile) * scale;
        if (fabsf(sc) < clampv) in |= 1u << r;
    }
    asm volatile("" ::: "memory");
    const float bound_in = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, bound) - 1u);
#pragma unroll
    for (int r = 0; r < 16; r++) {
        // the tile value moves only where it sits on the wrong side, and then by less than its own
        // error (onto the bound, or to the largest value inside it)
        float v = park[r * SPT_WAVE];
        const bool is_in = (in >> r) & 1u;
        if (((near >> r) & 1u) && is_in != (fabsf(v) < bound)) v = copysignf(is_in ? bound_in : bound, v);
        d[r] = v;
        dp[r] = park[(16 + r) * SPT_WAVE];
    }
}

// two workgroups per CU (4 waves per SIMD, 128 VGPRs): the barrier keeps the waves of one
// workgroup in the same phase, a second workgroup fills the other pipes meanwhile
constexpr int MA_WAVES_PER_EU = MA_E == 64 ? 4 : 2;    // (past 64: 64 + 64 registers of Q fragments
                                                       // and accumulators alone)
// One key tile per iteration in the forward and in the row-owned backward (two per iteration,
// i.e. fewer barriers and two independent chains, measured 58-71 against 48 us in the forward and
// no faster in the backward; sharing a row tile between the two waves of a SIMD -- alternate key
// tiles, partial grad_q summed through LDS -- measured 100 k against 89 k clocks: the two waves
// of a SIMD run the same program between the same barriers, so their MFMA phases coincide and
// their VALU phases coincide).
constexpr int MK_KTILES = MA_ET;    // 32-column tiles of grad_k per launch of the key-owned kernel
constexpr int MR_QTILES = MA_ET;    // 32-column tiles of grad_q per launch of the row-owned kernel
// grad_k and grad_v in ONE key-owned launch (MODE 0) only at d_head 64; past it the K and V
// fragments and both sets of accumulators do not fit 256 registers (MODE 1 + MODE 2)
constexpr bool MK_FUSED = MA_E <= 64;
#define MA_ROWS_WAVES_PER_EU 2
#define MA_KEYS_WAVES_PER_EU 2
template <typename T, bool YT>
__global__ __launch_bounds__(MA_THREADS)
__attribute__((amdgpu_waves_per_eu(MA_WAVES_PER_EU, MA_WAVES_PER_EU)))
void attention_mfma_forward_kernel(
    const unsigned long long *__restrict__ masks, const unsigned char *__restrict__ cells,
    const unsigned char *__restrict__ pool, const unsigned *__restrict__ sat,
    const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v,
    T *__restrict__ y, float *__restrict__ row_sum, float *__restrict__ bounds, int S, float scale,
    float clampv, int heads, int kv_heads, int blocks_per_batch) {
    constexpr int PI = Elem<T>::PARTS;                  // parts of the K / V images
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *img = smem;                                   // [2][MA_IMG]
    float *stat = reinterpret_cast<float *>(smem + 2 * MA_IMG);   // [waves][32] | [waves][2]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, c32 = lane & 31;
    const unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
    const int b = bid / blocks_per_batch;
    const int i0 = MA_WROWS * folded_row_tile(bid % blocks_per_batch, blocks_per_batch, wave);
    const DenseView dv = dense_view(b, S, MA_E, heads);
    // K and V alone: the kv head's slice (fp32; the bf16-storage entries have no grouped form)
    DenseView kv = dv;
    if constexpr (sizeof(T) == 4) kv = kv_view(b, S, MA_E, heads, kv_heads);
    const int RT = (S + MA_WROWS - 1) / MA_WROWS;
    const T *k_b = k + kv.base, *v_b = v + kv.base;

    const CellTiles ct(masks, cells, pool, sat, b, RT, i0 / MA_WROWS, i0 < S);
    // tiles any row of this workgroup can see: keys <= its last row (that of wave 7)
    const int last_tile = folded_row_tile(bid % blocks_per_batch, blocks_per_batch, MA_WAVES - 1);
    const int T_ = min(RT, last_tile + 1);
    const ScoreMap sm(scale, clampv);
    // every prologue load is issued before the first result is needed
    const TileStager<T> stager(k_b, v_b, kv.ld, S, tid);
    TileRegs<T> nxt = stager.load(0);
    uint4 mcur = ct.load(0, lane), mnxt;
    Frag qf[MA_KS];
    // for the backward's exact clamp mask (ClampGuard): |q_i|^2 of the own row, and the running
    // maximum of THIS thread's share of |k_j|^2 -- the four columns it stages, over all the rows it
    // stages; summed over the column groups at the end that bounds every staged key's |k_j|^2
    // (max_j sum_g <= sum_g max_j) without a cross-lane sum per tile.  About 3x the true maximum on
    // Gaussian rows (1.75x in the norm): the guard switches on that much earlier than it has to.  The
    // exact maximum -- |k_i|^2 of the own rows, one more read of K in the prologue -- was measured:
    // +3 us on every forward (44 -> 48 in the step), more than the guard's per-tile test costs while
    // it is on, so the loose bound stays.
    float q2 = 0.f, k2part = 0.f;
    {
        float xq[MA_E / 2];
        load_own_rows_raw(xq, q + dv.base, dv.ld, S, i0, lane);
        stager.store(img, nxt);
        if (bounds) {
            k2part = stager.k_share(nxt);
#pragma unroll
            for (int x = 0; x < MA_E / 2; x++) q2 = fmaf(xq[x], xq[x], q2);
        }
        split_own_rows(qf, xq, sm.sl2);
    }
    __syncthreads();

    f32x16 yacc[MA_ET];
#pragma unroll
    for (int eh = 0; eh < MA_ET; eh++)
#pragma unroll
        for (int r = 0; r < 16; r++) yacc[eh][r] = 0.f;
    float rs = 0.f;

    for (int t = 0; t < T_; t++) {
        const char *buf = img + (t & 1) * MA_IMG;
        // the next tile (K, V and this wave's cell counts) is in flight meanwhile
        nxt = stager.load(min(t + 1, T_ - 1));
        mnxt = ct.load(t + 1, lane);
        if (ct.live(t)) {
            f32x16 d;
#pragma unroll
            for (int r = 0; r < 16; r++) d[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < MA_KS; ks++)
                d = mm<PI, 2>(read_rows<PI>(buf + MA_KH, buf + MA_KL, lane, ks), qf[ks], d);
            // cells: this lane holds row i0 + c32, keys 32t + acc_row(r, h); byte 4g + u of
            // the cell word is the multiplicity of register 4g + u
            const uint4 mm4 = ct.words(mcur, t, lane);
            const unsigned mw[4] = {mm4.x, mm4.y, mm4.z, mm4.w};
            float p[16];
#pragma unroll
            for (int g = 0; g < 4; g++) {
                p[4 * g + 0] = cell_count<0>(mw[g]) * sm.exp_of(d[4 * g + 0]);
                p[4 * g + 1] = cell_count<1>(mw[g]) * sm.exp_of(d[4 * g + 1]);
                p[4 * g + 2] = cell_count<2>(mw[g]) * sm.exp_of(d[4 * g + 2]);
                p[4 * g + 3] = cell_count<3>(mw[g]) * sm.exp_of(d[4 * g + 3]);
                rs += (p[4 * g] + p[4 * g + 1]) + (p[4 * g + 2] + p[4 * g + 3]);
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; s2++) {
                const Frag pf = split8(p[8 * s2], p[8 * s2 + 1], p[8 * s2 + 2], p[8 * s2 + 3],
                                       p[8 * s2 + 4], p[8 * s2 + 5], p[8 * s2 + 6], p[8 * s2 + 7]);
#pragma unroll
                for (int eh = 0; eh < MA_ET; eh++)
                    yacc[eh] = mm<2, PI>(pf, read_cols_tr<PI>(buf + MA_VH, buf + MA_VL, 32 * eh, lane, s2),
                                         yacc[eh]);
            }
        }
        if (t + 1 < T_) stager.store(img + ((t + 1) & 1) * MA_IMG, nxt);
        if (bounds) k2part = fmaxf(k2part, stager.k_share(nxt));
        mcur = mnxt;
        __syncthreads();
    }

    if (bounds) {                                       // (kernel argument: uniform)
        // columns: lanes with equal tid % MA_EQ; rows: the other lane bits
        float km = k2part;
        if constexpr (Share<MA_THREADS>::EVEN) {
#pragma unroll
            for (int off = MA_EQ; off < SPT_WAVE; off <<= 1) km = fmaxf(km, __shfl_xor(km, off, SPT_WAVE));
#pragma unroll
            for (int off = 1; off < MA_EQ; off <<= 1) km += __shfl_xor(km, off, SPT_WAVE);
        } else {
            // a thread's float4s hold varying columns: |k_j|^2, a sum of MA_EQ four-column
            // shares, is at most MA_EQ times the largest share any thread staged (the maximum
            // over the waves is taken below)
#pragma unroll
            for (int off = 1; off < SPT_WAVE; off <<= 1) km = fmaxf(km, __shfl_xor(km, off, SPT_WAVE));
            km *= (float)MA_EQ;
        }
        float qm = q2 + __shfl_xor(q2, 32, SPT_WAVE);   // the two lane halves hold half a row each
#pragma unroll
        for (int off = 1; off < 32; off <<= 1) qm = fmaxf(qm, __shfl_xor(qm, off, SPT_WAVE));
        float *wb = stat + MA_WAVES * MA_WROWS;
        if (lane == 0) {
            wb[2 * wave] = qm;
            wb[2 * wave + 1] = km;
        }
        __syncthreads();
        if (tid < 2) {
            float best = 0.f;
#pragma unroll
            for (int w = 0; w < MA_WAVES; w++) best = fmaxf(best, wb[2 * w + tid]);
            bounds[((size_t)b * MA_BOUND_SLOTS + bid % blocks_per_batch) * 2 + tid] = best;
        }
    }

    // ---- rows: 1 / max(1e-9, sum); the two lane halves hold disjoint keys of the same row ----
    rs += __shfl_xor(rs, 32, SPT_WAVE);
    const float inv = 1.0f / fmaxf(1e-9f, rs);
    float *wstat = stat + wave * MA_WROWS;
    if (h == 0) {
        wstat[c32] = inv;
        if (i0 + c32 < S) row_sum[(size_t)b * S + i0 + c32] = ((ct.satrows >> c32) & 1u) ? rs * MA_SAT_UP : rs;
    }
    wave_lds_fence();
    T *y_b = y + (size_t)b * S * MA_E;
    if (i0 < S) {
        if (!YT) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int il = acc_row(r, h);
                const float sc = wstat[il];
                if (i0 + il < S) {
#pragma unroll
                    for (int eh = 0; eh < MA_ET; eh++)
                        if (MA_E % 32 == 0 || 32 * eh + c32 < MA_E)
                            st1(y_b + (size_t)(i0 + il) * MA_E + 32 * eh + c32, yacc[eh][r] * sc);
                }
            }
        } else {
            // [batch, E, S]: registers 4g .. 4g+3 are four consecutive rows of one e, but
            // stored straight from the accumulator layout every lane writes its own 16-byte
            // piece 4 S bytes from its neighbour's (14 us of partial-line writes).  Through a
            // wave-private LDS tile [e][row] instead: 8 lanes then cover 128 contiguous bytes
            // of one e and a store instruction writes 8 such runs.
            float *tile = reinterpret_cast<float *>(img) + wave * (32 * MA_TLD);
#pragma unroll
            for (int eh = 0; eh < MA_ET; eh++) {
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const int il = 8 * g + 4 * h;
                    *reinterpret_cast<float4 *>(tile + c32 * MA_TLD + il) = make_float4(
                        yacc[eh][4 * g] * wstat[il], yacc[eh][4 * g + 1] * wstat[il + 1],
                        yacc[eh][4 * g + 2] * wstat[il + 2], yacc[eh][4 * g + 3] * wstat[il + 3]);
                }
                wave_lds_fence();
#pragma unroll
                for (int k4 = 0; k4 < (eh + 1 < MA_ET ? 32 : MA_ELAST) / 8; k4++) {
                    const int el = (lane >> 3) + 8 * k4, i4 = (lane & 7) * 4;
                    const float4 o = *reinterpret_cast<const float4 *>(tile + el * MA_TLD + i4);
                    T *dst = y_b + (size_t)(el + 32 * eh) * S + i0 + i4;
                    if (i0 + i4 + 3 < S && (S & 3) == 0) {
                        st4(dst, o);
                    } else {
                        const float ov[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
                        for (int u = 0; u < 4; u++)
                            if (i0 + i4 + u < S) st1(dst + u, ov[u]);
                    }
                }
                wave_lds_fence();
            }
        }
    }
}

// ===================================== backward ============================================
// Nothing of size nnz was saved: both kernels recompute the score tiles from q, k and the
// probabilities from the forward's row sums.  With P = m exp(s) / row_sum and
//   delta_i = max(1e-9, sum_p P_p dP_p) = max(1e-9, dY_i . Y_i)        (softmax.cu:69; P dP
//             summed over a row is dY_i . (P V)_i = dY_i . Y_i)
//   dS      = scale * P * (dP - delta) inside the clamp, 0 outside      (softmax.cu:75-78)
// the row-owned kernel produces grad_q (+ delta for its sibling), the key-owned one grad_k
// and grad_v:
//   grad_q[i] = sum_j dS[i, j] k[j]     grad_k[j] = sum_i dS[i, j] q[i]     (kernels/sddmm.py)
//   grad_v[j] = sum_i P[i, j] dY[i]     dP[i, j]  = dY[i] . v[j]            (kernels/spmm.py)

// ---- the backward's workgroup shape ----
// Both kernels need a 256-register budget (2 waves per SIMD).  At 8 waves per workgroup that is one
// workgroup per CU (LDS alone: 102,400 / 119,040 B), and its barriers keep every wave of the CU in
// the same phase -- loads, then MFMA, then VALU, nothing overlapping.  At d_head
// 64 the backward therefore runs 4-wave workgroups of 128 rows (keys): 2 x 69,632 / 78,080 B of LDS
// and 2 x 4 waves at 256 registers fit a CU, and the two workgroups' barriers are independent, so
// one stages its next tile while the other multiplies.  d_head 128 keeps the 8-wave shape: its
// kernels already spill at 256 registers, and half the threads would double each one's staging share.
constexpr int BW_THREADS = MA_E == 64 ? 256 : MA_THREADS;
constexpr int BW_WAVES = BW_THREADS / SPT_WAVE;     // 4 (d_head 64) or 8
constexpr int BW_ROWS = BW_WAVES * MA_WROWS;        // rows (keys) per workgroup: 128 or 256
constexpr int BW_RPT = Share<BW_THREADS>::RPT, BW_RPP = Share<BW_THREADS>::RPP;
// Which 32-row (32-key) tiles a backward workgroup owns: wave w of block g of its slice takes tile
// BW_WAVES g + w.  Block g of the row-owned kernel walks BW_WAVES (g + 1) key tiles and block g of
// the key-owned one RT - BW_WAVES g row tiles, so at S = 512 a slice's blocks carry 1 : 2 : 3 : 4
// (rows) or 4 : 3 : 2 : 1 (keys) of the work.  blockIdx is therefore taken as rank * slices + slice,
// rank 0 being the HEAVIEST block: every slice's longest block is dispatched first, and the short
// ones fill the slots the long ones leave (1,024 workgroups on 512 slots at the bench shape, with
// no half-empty third round).  Consecutive ids go round-robin to the eight XCDs, so with a slice
// count divisible by 8 all blocks of a slice share one XCD's L2.  The 8-wave shape keeps the folded
// mapping of the forward (one short and one long wave per SIMD: a CU holds one workgroup).
struct BwBlock {
    int b, g;            // slice, block of the slice
    int tile;            // this wave's row (key) tile
    int first, last;     // the smallest and the largest tile of the workgroup's waves
};
__device__ __forceinline__ BwBlock bw_block(int blocks_per_batch, int wave, bool heavy_last) {
    BwBlock r;
    if constexpr (BW_WAVES == MA_WAVES) {
        const unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
        r.b = bid / blocks_per_batch;
        r.g = bid % blocks_per_batch;
        r.tile = folded_row_tile(r.g, blocks_per_batch, wave);
        r.first = (MA_WAVES / 2) * r.g;
        r.last = folded_row_tile(r.g, blocks_per_batch, MA_WAVES - 1);
    } else {
        const unsigned slices = gridDim.x / blocks_per_batch, rank = blockIdx.x / slices;
        r.b = blockIdx.x - rank * slices;
        r.g = heavy_last ? blocks_per_batch - 1 - (int)rank : (int)rank;
        r.tile = BW_WAVES * r.g + wave;
        r.first = BW_WAVES * r.g;
        r.last = r.first + BW_WAVES - 1;
    }
    return r;
}
// The exact clamp guard reads the bounds the FORWARD's workgroups left: one slot per forward block.
__device__ __forceinline__ int forward_slots(int S) { return (S + MA_ROWS - 1) / MA_ROWS; }

// ---- row-owned: same skeleton as the forward and the same images, K rows | V rows (the K
// rows image also feeds grad_q = dS^T K through the transposing read).
// Measured by compiling phases out (80 us whole): without the tile arithmetic 54 us (prologue --
// dY, Y, Q: 100 MB -- 23, the loop's loads 23, epilogue 6, image stores 2, barriers 0); WITH the
// arithmetic but without the loop's loads, stores and barriers 75 us.  So the loop's memory
// traffic hides behind the arithmetic, and the arithmetic (46 us for 16 us of MFMA-pipe time) is
// one wave per SIMD running its MFMA and VALU phases one after the other: at 187 VGPRs a CU holds
// one workgroup, and half of its waves (the short row tiles) finish early.  (That was the 8-wave
// shape; d_head 64 now runs two 4-wave workgroups per CU, see BW_THREADS.) ----
// GT: grad_y and y arrive as [batch, E, S] (the transposed forward output and its gradient)
template <typename T, bool GT>
__global__ __launch_bounds__(BW_THREADS)
__attribute__((amdgpu_waves_per_eu(MA_ROWS_WAVES_PER_EU, MA_ROWS_WAVES_PER_EU)))
void attention_mfma_backward_rows_kernel(
    const unsigned long long *__restrict__ masks, const unsigned char *__restrict__ cells,
    const unsigned char *__restrict__ pool, const unsigned *__restrict__ sat,
    const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v,
    const T *__restrict__ gy, const T *__restrict__ y,
    const float *__restrict__ row_sum, const float *__restrict__ bounds, T *__restrict__ grad_q,
    float *__restrict__ delta, int S, float scale, float clampv, int heads, int kv_heads,
    int blocks_per_batch, int half) {
    constexpr int PI = Elem<T>::PARTS;                  // parts of the K / V images
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *img = smem;                                   // [2][MA_IMG]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, c32 = lane & 31;
    const BwBlock blk = bw_block(blocks_per_batch, wave, true);
    const int b = blk.b;
    const DenseView dv = dense_view(b, S, MA_E, heads);
    // K and V alone: the kv head's slice (fp32; the bf16-storage entries have no grouped form)
    DenseView kv = dv;
    if constexpr (sizeof(T) == 4) kv = kv_view(b, S, MA_E, heads, kv_heads);
    const int RT = (S + MA_WROWS - 1) / MA_WROWS;
    const ScoreMap sm(scale, clampv);
    const int i0 = MA_WROWS * blk.tile;
    const CellTiles ct(masks, cells, pool, sat, b, RT, i0 / MA_WROWS, i0 < S);
    const int T_ = min(RT, blk.last + 1);
    const TileStager<T, BW_THREADS> stager(k + kv.base, v + kv.base, kv.ld, S, tid);
    TileRegs<T, BW_THREADS> nxt = stager.load(0);
    uint4 mcur = ct.load(0, lane), mnxt;
    // own rows: dY (B operand of dP = V dY^T), delta = max(1e-9, dY . Y), Q (B operand of D)
    Frag gf[MA_KS], qf[MA_KS];
    float delta_i, q2 = 0.f;
    const int row = i0 + c32;
    float rsum = row_sum[(size_t)b * S + min(row, S - 1)];
    if ((ct.satrows >> c32) & 1u) rsum *= MA_SAT_DOWN;          // (the sum the tiles' counts add up to)
    {
        float xr[MA_E / 2], yr[MA_E / 2], xq[MA_E / 2];
        const size_t ob = (size_t)b * S * MA_E;
        load_own_rows_raw(xq, q + dv.base, dv.ld, S, i0, lane);
        if (GT) {
            // [E][S] operands: wide loads through the wave's LDS tile (the image buffers
            // are free until the first key tile is staged)
            float *tile = reinterpret_cast<float *>(img) + wave * (32 * MA_TLD);
            load_own_rows_transposed(xr, gy + ob, S, i0, tile, lane);
            load_own_rows_transposed(yr, y + ob, S, i0, tile, lane);
            __syncthreads();
        } else {
            load_own_rows_raw(xr, gy + ob, MA_E, S, i0, lane);
            load_own_rows_raw(yr, y + ob, MA_E, S, i0, lane);
        }
        stager.store(img, nxt);
        float dl = 0.f;
#pragma unroll
        for (int x = 0; x < MA_E / 2; x++) dl = fmaf(xr[x], yr[x], dl);
        dl += __shfl_xor(dl, 32, SPT_WAVE);
        delta_i = fmaxf(1e-9f, dl);
        // scale / row_sum is a per-row factor of dS: folded into dY (and delta) once here
        // instead of into every cell: dS = m e (dP' - delta') with dP' = pscale dP
        const float pscale = scale / fmaxf(1e-9f, rsum);
        split_own_rows(gf, xr, pscale);
        split_own_rows(qf, xq, sm.sl2);
        // for the key-owned sibling: the row's weight 1 / row_sum (of the sum its tile counts add up
        // to) and the weighted delta -- it stages 32 rows per iteration and divides nothing
        if (h == 0 && row < S && half == 0) {
            const float w = 1.0f / fmaxf(1e-9f, rsum);
            delta[(size_t)b * S + row] = w;
            delta[((size_t)(gridDim.x / blocks_per_batch) + b) * S + row] = w * delta_i;
        }
        delta_i *= pscale;
        if (bounds) {
#pragma unroll
            for (int x = 0; x < MA_E / 2; x++) q2 = fmaf(xq[x], xq[x], q2);
            q2 += __shfl_xor(q2, 32, SPT_WAVE);
        }
    }
    const ClampGuard cg(bounds, b, forward_slots(S), 1, q2, sm, clampv);
    __syncthreads();

    f32x16 qacc[MR_QTILES];
#pragma unroll
    for (int e = 0; e < MR_QTILES; e++)
#pragma unroll
        for (int r = 0; r < 16; r++) qacc[e][r] = 0.f;

    for (int t = 0; t < T_; t++) {
        const char *buf = img + (t & 1) * MA_IMG;
        nxt = stager.load(min(t + 1, T_ - 1));
        mnxt = ct.load(t + 1, lane);
        if (ct.live(t)) {
            f32x16 d, dp;
#pragma unroll
            for (int r = 0; r < 16; r++) d[r] = dp[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < MA_KS; ks++) {
                d = mm<PI, 2>(read_rows<PI>(buf + MA_KH, buf + MA_KL, lane, ks), qf[ks], d);
                dp = mm<PI, 2>(read_rows<PI>(buf + MA_VH, buf + MA_VL, lane, ks), gf[ks], dp);
            }
            const uint4 cw = ct.words(mcur, t, lane);
            if (cg.wanted(d))                           // (wave-uniform, rare)
                clamp_exact(d, dp, smem + 2 * MA_IMG, wave, cw, sm.bound, cg.thr, q + dv.base, i0, S,
                            k + kv.base + (size_t)t * MA_KT * kv.ld, dv.ld, kv.ld, scale, clampv);
            const unsigned mw[4] = {cw.x, cw.y, cw.z, cw.w};
            float ds[16];
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const float m4[4] = {cell_count<0>(mw[g]), cell_count<1>(mw[g]),
                                     cell_count<2>(mw[g]), cell_count<3>(mw[g])};
#pragma unroll
                for (int x = 0; x < 4; x++) {
                    const int r = 4 * g + x;
                    const float pw = m4[x] * sm.exp_of(d[r]);
                    ds[r] = sm.inside(d[r]) ? pw * (dp[r] - delta_i) : 0.0f;
                }
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; s2++) {
                const Frag sf = split8(ds[8 * s2], ds[8 * s2 + 1], ds[8 * s2 + 2], ds[8 * s2 + 3],
                                       ds[8 * s2 + 4], ds[8 * s2 + 5], ds[8 * s2 + 6], ds[8 * s2 + 7]);
#pragma unroll
                for (int eh = 0; eh < MR_QTILES; eh++)
                    qacc[eh] = mm<2, PI>(sf, read_cols_tr<PI>(buf + MA_KH, buf + MA_KL,
                                                              32 * MR_QTILES * half + 32 * eh, lane, s2),
                                         qacc[eh]);
            }
        }
        if (t + 1 < T_) stager.store(img + ((t + 1) & 1) * MA_IMG, nxt);
        mcur = mnxt;
        __syncthreads();
    }
    if (i0 < S) {
        float *tile = reinterpret_cast<float *>(img) + wave * (32 * MA_TLD);
        T *gq_b = grad_q + dv.base + (size_t)i0 * dv.ld + 32 * MR_QTILES * half;
#pragma unroll
        for (int eh = 0; eh < MR_QTILES; eh++)
            store_acc_half(qacc[eh], 1.0f, tile, gq_b + 32 * eh, dv.ld, S - i0, lane,
                           eh + 1 < MR_QTILES ? 32 : MA_ELAST);
    }
}

// ---- key-owned: a wave owns 32 keys (K, V fragments and the grad_k, grad_v accumulators in
// registers) and walks the row tiles at or below the diagonal; 32 rows of Q and dY stream
// through LDS as images Q rows | dY rows | Q cols | dY cols, plus the rows' 1 / row_sum and
// delta.  Tiles are computed as D[row, key], so the sums over rows take the accumulator tile
// as the A operand.  Which key tiles a workgroup's waves own: bw_block (the 8-wave shape folds
// them like the rows; the 4-wave shape takes 4 consecutive key tiles, heaviest blocks first).
// images: Q rows | dY (rows image, or -- GT, the operand arriving as [E][S] -- a cols image:
// whichever its source layout fills with 8-byte stores; the other orientation of each operand
// comes from the transposing read) | the rows' scaled delta
constexpr int MK_GSLOT = MA_CIMG > MA_RIMG ? MA_CIMG : MA_RIMG;           // either orientation
constexpr int MK_QR = 0, MK_G = 2 * MA_RIMG, MK_ST = 2 * MA_RIMG + 2 * MK_GSLOT,
              MK_IMG = MK_ST + MA_WROWS * 4;                                // 18560 B at E = 64
template <typename T, bool GT>
struct KeysStager {
    const T *q_b, *gy_b;
    const float *w_b, *wd_b;    // the rows' 1 / row_sum and (1 / row_sum) delta, from the row-owned kernel
    int ld, S, tid;
    struct Regs {
        typename Elem<T>::raw4 qf[BW_RPT], gf[BW_RPT];
        float4 rs[BW_RPT];
        float st_wd;
    };
    // (not Share::EVEN -- d_head 80 -- float4 u of thread t is slot f = t + BW_THREADS u: tile
    // row f / MA_EQ, columns 4 (f % MA_EQ) .., or (GT) e = f / 8; loads clamped, stores skipped
    // past the tile, as in TileStager)
    static constexpr bool EVEN = Share<BW_THREADS>::EVEN;
    // unconditional, clamped loads (see TileStager::load); rows >= S are given weight 0 by
    // store(), so whatever finite data the clamped rows hold never counts.  Raw values only:
    // arithmetic on them here would wait for the loads at the top of the iteration.
    __device__ __forceinline__ Regs load(int rt) const {
        Regs r;
        const int i0 = rt * MA_WROWS;
        const int e4 = (tid % MA_EQ) * 4;
#pragma unroll
        for (int u = 0; u < BW_RPT; u++) {
            int il = tid / MA_EQ + BW_RPP * u, c4 = e4;
            if constexpr (!EVEN) {
                const int f = Share<BW_THREADS>::slot(tid, u);
                il = f / MA_EQ;
                c4 = (f % MA_EQ) * 4;
            }
            const int row = min(i0 + il, S - 1);
            r.qf[u] = ld_raw4(q_b + (size_t)row * ld + c4);
            if (!GT) {
                r.gf[u] = ld_raw4(gy_b + (size_t)row * MA_E + c4);
                r.rs[u] = make_float4(w_b[row], 0.f, 0.f, 0.f);
            } else {        // [E][S]: four consecutive rows of one e (S % 4 == 0)
                int e = (tid >> 3) + (BW_THREADS / 8) * u;
                if constexpr (!EVEN) e = Share<BW_THREADS>::slot(tid, u) >> 3;
                const int i4 = min(i0 + (tid & 7) * 4, S - 4);
                r.gf[u] = ld_raw4(gy_b + (size_t)e * S + i4);
                r.rs[u] = *reinterpret_cast<const float4 *>(w_b + i4);
            }
        }
        const int sr = min(i0 + (tid & (MA_WROWS - 1)), S - 1);
        r.st_wd = wd_b[sr];
        return r;
    }
    // 1 / row_sum is a per-row factor of both P (grad_v) and dS (grad_k): dY is staged
    // pre-multiplied by it (an fp32 product: two parts whatever the storage type), rows >= S
    // by 0, and the rows' delta likewise
    __device__ __forceinline__ void store(char *buf, const Regs &r, int rt) const {
        const int i0 = rt * MA_WROWS;
        const int e4 = (tid % MA_EQ) * 4;
        auto weight = [&](float w, int row) { return row < S ? w : 0.0f; };
#pragma unroll
        for (int u = 0; u < BW_RPT; u++) {
            int il = tid / MA_EQ + BW_RPP * u, c4 = e4;
            if constexpr (!EVEN) {
                if (!Share<BW_THREADS>::owns(tid, u)) continue;
                il = (tid + BW_THREADS * u) / MA_EQ;
                c4 = ((tid + BW_THREADS * u) % MA_EQ) * 4;
            }
            put_rows4(buf + MK_QR, il, c4, r.qf[u]);
            const float4 g = Elem<T>::f4(r.gf[u]);
            if (!GT) {
                const float w = weight(r.rs[u].x, i0 + il);
                put_rows4(buf + MK_G, il, c4, make_float4(w * g.x, w * g.y, w * g.z, w * g.w));
            } else {
                const int i4 = (tid & 7) * 4;
                put_cols4(buf + MK_G, (tid >> 3) + (BW_THREADS / 8) * u, i4,
                          make_float4(weight(r.rs[u].x, i0 + i4) * g.x,
                                      weight(r.rs[u].y, i0 + i4 + 1) * g.y,
                                      weight(r.rs[u].z, i0 + i4 + 2) * g.z,
                                      weight(r.rs[u].w, i0 + i4 + 3) * g.w));
            }
        }
        if (tid < MA_WROWS)
            reinterpret_cast<float *>(buf + MK_ST)[tid] = weight(r.st_wd, i0 + tid);
    }
};

// MODE 0: grad_k and grad_v together, 64 columns (`half`) per launch -- d_head 64.
// d_head 128 cannot hold K, V fragments (128 registers) and four accumulator tiles beside the
// tile arithmetic (the combined kernel spilled 41-60 registers: 281 us per launch), so there
// MODE 1: grad_v alone, all E columns (needs P only: no V fragments, no dP, no delta);
// MODE 2: grad_k alone, all E columns.  d_head 80 takes the same split (K, V: 80 registers, six
// accumulator tiles: 96) -- see MK_FUSED.
template <typename T, bool GT, int MODE>
__global__ __launch_bounds__(BW_THREADS)
__attribute__((amdgpu_waves_per_eu(MA_KEYS_WAVES_PER_EU, MA_KEYS_WAVES_PER_EU)))
void attention_mfma_backward_keys_kernel(
    const unsigned long long *__restrict__ masks, const unsigned char *__restrict__ cells_t,
    const unsigned char *__restrict__ pool_t, const unsigned *__restrict__ sat,
    const T *__restrict__ q, const T *__restrict__ k, const T *__restrict__ v,
    const T *__restrict__ gy, const float *__restrict__ row_sum, const float *__restrict__ bounds,
    const float *__restrict__ delta, T *__restrict__ grad_k, T *__restrict__ grad_v,
    int S, float scale, float clampv, int heads, int kv_heads, int blocks_per_batch, int half) {
    constexpr int PI = Elem<T>::PARTS;                  // parts of the Q image and of the V fragments
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *img = smem;                                   // [2][MK_IMG]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, c32 = lane & 31;
    const BwBlock blk = bw_block(blocks_per_batch, wave, false);
    const int b = blk.b;
    const int kt = blk.tile;
    const int j0 = kt * MA_KT;
    const DenseView dv = dense_view(b, S, MA_E, heads);
    // K and V are READ from the kv head's slice; grad_k and grad_v are WRITTEN per query slice (dv):
    // with grouped heads they are this query head's partials, summed by head_group_sum_kernel
    DenseView kv = dv;                                  // (fp32 only: bf16 storage has no grouped form)
    if constexpr (sizeof(T) == 4) kv = kv_view(b, S, MA_E, heads, kv_heads);
    const int RT = (S + MA_WROWS - 1) / MA_WROWS;
    const bool have = j0 < S;

    constexpr bool WANT_K = MODE != 1, WANT_V = MODE != 2;
    constexpr int NVT = MODE == 1 ? MA_ET : 2;           // 32-column tiles of grad_v produced
    const ScoreMap sm(scale, clampv);
    Frag kf[MA_KS], vf[WANT_K ? MA_KS : 1];
    float k2 = 0.f;
    {
        float xk[MA_E / 2];
        load_own_rows_raw(xk, k + kv.base, kv.ld, S, j0, lane);
        if (WANT_K && bounds) {
#pragma unroll
            for (int x = 0; x < MA_E / 2; x++) k2 = fmaf(xk[x], xk[x], k2);
            k2 += __shfl_xor(k2, 32, SPT_WAVE);
        }
        split_own_rows(kf, xk, sm.sl2);     // the score scale (log2 domain) folded into K
        if constexpr (WANT_K) {             // V only feeds dP, which only dS needs
            float xv[MA_E / 2];
            load_own_rows_raw(xv, v + kv.base, kv.ld, S, j0, lane);
            split_own_rows(vf, xv);         // (stored bf16: the lo parts are zero and unused)
        }
    }
    // Round 4: the exact clamp mask put this kernel five registers past its 256; hipcc's answer was
    // one 16-byte spill of a K / V fragment, reloaded from scratch in every iteration -- a VECTOR
    // memory load, whose wait also waits for the row tile requested at the top of the iteration
    // (vmcnt counts in order): 117.7 - 132.7 us against 106.9.  The last V fragment (8 registers with
    // both parts) is parked in a wave-private LDS block instead and read back once per iteration, an
    // LDS read among two dozen others, on lgkmcnt.
    constexpr bool STASH_V = WANT_K && MA_E == 64 && sizeof(T) == 4;
    char *const vstash = smem + 2 * MK_IMG + BW_WAVES * MA_PARK + wave * 2048 + 16 * lane;
    if constexpr (STASH_V) {
        *reinterpret_cast<uint4 *>(vstash) = make_uint4(vf[MA_KS - 1].hi.x, vf[MA_KS - 1].hi.y,
                                                        vf[MA_KS - 1].hi.z, vf[MA_KS - 1].hi.w);
        *reinterpret_cast<uint4 *>(vstash + 1024) = make_uint4(vf[MA_KS - 1].lo.x, vf[MA_KS - 1].lo.y,
                                                               vf[MA_KS - 1].lo.z, vf[MA_KS - 1].lo.w);
    }
    // the slice's row-tile masks live in registers (lane rt: mask of row tile rt), so that the
    // loop body has no load whose result it needs at once
    // (grad_v needs P alone, which is continuous in the score: no exact mask for MODE 1)
    const ClampGuard cg(WANT_K ? bounds : nullptr, b, forward_slots(S), 0, k2, sm, clampv);
    // (round 4: ONE register -- this wave's key tile needs two bits per row tile, lane rt holds bit 0:
    // tile (rt, kt) is live, bit 1: it is stored in byte form; the 64-bit masks were four registers
    // of a kernel that has none to spare)
    unsigned bits_reg = 0u;
    if (lane < RT) {
        const unsigned long long m0 = masks[2 * ((size_t)b * RT + lane)];
        const unsigned long long m1 = masks[2 * ((size_t)b * RT + lane) + 1];
        bits_reg = (unsigned)((m0 >> min(kt, 63)) & 1ull) | ((unsigned)((m1 >> min(kt, lane)) & 1ull) << 1);
    }
    // bits of tile (rt, kt) (0 past the last row tile)
    auto mask_of = [&](int rt) -> unsigned {
        return rt < RT ? (unsigned)__builtin_amdgcn_readlane((int)bits_reg, rt) : 0u;
    };
    // is the tile (row tile rt, this wave's key tile) stored in byte form?
    auto multi_of = [&](int rt) {
        return (bool)(((unsigned)__builtin_amdgcn_readlane((int)bits_reg, min(rt, RT - 1)) >> 1) & 1u);
    };
    const int cstride = cell_slot_bytes(pool_t) / 16;
    const uint4 *cell_b = reinterpret_cast<const uint4 *>(
        cells_t + (size_t)b * tri(RT) * cell_slot_bytes(pool_t));
    const uint4 *pool_b = pool_t ? reinterpret_cast<const uint4 *>(pool_t + (size_t)b * RT * MA_CELLS)
                                 : nullptr;
    auto live = [&](unsigned m, int rt) { return have && rt >= kt && rt < RT && (m & 1u); };
    // always in bounds: the row tile clamped to the last one, the key tile to the diagonal
    auto cell_load = [&](int rt) {
        const int rc = min(rt, RT - 1);
        if (multi_of(rt)) return pool_b ? pool_b[rc * 64 + lane] : cell_b[(tri(rc) + min(kt, rc)) * 64 + lane];
        return cell_b[(tri(rc) + min(kt, rc)) * cstride + (c32 >> 2)];
    };

    const int rt0 = blk.first;                          // the first row tile any wave needs
    const KeysStager<T, GT> stager{q + dv.base, gy + (size_t)b * S * MA_E, delta + (size_t)b * S,
                                   delta + ((size_t)(gridDim.x / blocks_per_batch) + b) * S, dv.ld, S, tid};
    stager.store(img, stager.load(min(rt0, RT - 1)), rt0);
    unsigned mcur_mask = mask_of(rt0);
    uint4 mcur = cell_load(rt0);
    __syncthreads();

    f32x16 kacc[MK_KTILES], vacc[NVT];
#pragma unroll
    for (int e = 0; e < MK_KTILES; e++)
#pragma unroll
        for (int r = 0; r < 16; r++) kacc[e][r] = 0.f;
#pragma unroll
    for (int e = 0; e < NVT; e++)
#pragma unroll
        for (int r = 0; r < 16; r++) vacc[e][r] = 0.f;

    for (int rt = rt0; rt < RT; rt++) {
        const char *buf = img + ((rt - rt0) & 1) * MK_IMG;
        const typename KeysStager<T, GT>::Regs nxt = stager.load(min(rt + 1, RT - 1));
        const unsigned mnxt_mask = mask_of(rt + 1);
        const uint4 mnxt = cell_load(rt + 1);
        if (live(mcur_mask, rt)) {
            f32x16 d, dp;
#pragma unroll
            for (int r = 0; r < 16; r++) d[r] = dp[r] = 0.f;
            Frag vlast;
            if constexpr (STASH_V) {
                vlast.hi = *reinterpret_cast<const uint4 *>(vstash);
                vlast.lo = *reinterpret_cast<const uint4 *>(vstash + 1024);
            }
#pragma unroll
            for (int ks = 0; ks < MA_KS; ks++) {
                d = mm<PI, 2>(read_rows<PI>(buf + MK_QR, buf + MK_QR + MA_RIMG, lane, ks), kf[ks], d);
                if constexpr (WANT_K)
                    dp = mm<2, PI>(GT ? read_rows_tr(buf + MK_G, buf + MK_G + MA_CIMG, lane, ks)
                                      : read_rows<2>(buf + MK_G, buf + MK_G + MA_RIMG, lane, ks),
                                   (STASH_V && ks == MA_KS - 1) ? vlast : vf[ks], dp);
            }
            // this lane: key j0 + c32, rows 8g + 4h + u of the tile in register 4g + u
            const bool mlt = multi_of(rt);
            const uint4 cw = cell_words(mcur, mlt, lane);
            if constexpr (WANT_K) {
                if (cg.wanted(d))                       // (wave-uniform, rare)
                    clamp_exact(d, dp, smem + 2 * MK_IMG, wave, cw, sm.bound, cg.thr, k + kv.base, j0, S,
                                q + dv.base + (size_t)rt * MA_WROWS * dv.ld, kv.ld, dv.ld, scale, clampv);
            }
            const float *st = reinterpret_cast<const float *>(buf + MK_ST);
            const unsigned mw[4] = {cw.x, cw.y, cw.z, cw.w};
            float p[16], ds[16];
#pragma unroll
            for (int g4 = 0; g4 < 4; g4++) {
                float4 del4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (WANT_K) del4 = *reinterpret_cast<const float4 *>(st + 8 * g4 + 4 * h);
                const float del[4] = {del4.x, del4.y, del4.z, del4.w};
                const float m4[4] = {cell_count<0>(mw[g4]), cell_count<1>(mw[g4]),
                                     cell_count<2>(mw[g4]), cell_count<3>(mw[g4])};
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int r = 4 * g4 + u;
                    p[r] = m4[u] * sm.exp_of(d[r]);          // x 1 / row_sum: in the dY images
                    ds[r] = 0.0f;
                    if constexpr (WANT_K)                    // x scale: in the epilogue
                        ds[r] = sm.inside(d[r]) ? p[r] * (dp[r] - del[u]) : 0.0f;
                }
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; s2++) {
                const Frag pf = split8(p[8 * s2], p[8 * s2 + 1], p[8 * s2 + 2], p[8 * s2 + 3],
                                       p[8 * s2 + 4], p[8 * s2 + 5], p[8 * s2 + 6], p[8 * s2 + 7]);
                const Frag sf = split8(ds[8 * s2], ds[8 * s2 + 1], ds[8 * s2 + 2], ds[8 * s2 + 3],
                                       ds[8 * s2 + 4], ds[8 * s2 + 5], ds[8 * s2 + 6], ds[8 * s2 + 7]);
                if constexpr (WANT_V) {
#pragma unroll
                    for (int eh = 0; eh < NVT; eh++) {
                        const int col0 = (MODE == 1 ? 0 : 64 * half) + 32 * eh;
                        vacc[eh] = mm<2, 2>(pf, GT ? read_cols(buf + MK_G, buf + MK_G + MA_CIMG,
                                                               c32 + col0, h, s2)
                                                   : read_cols_tr<2>(buf + MK_G, buf + MK_G + MA_RIMG,
                                                                     col0, lane, s2), vacc[eh]);
                    }
                }
                if constexpr (WANT_K) {
#pragma unroll
                    for (int eh = 0; eh < MK_KTILES; eh++)
                        kacc[eh] = mm<2, PI>(sf, read_cols_tr<PI>(buf + MK_QR, buf + MK_QR + MA_RIMG,
                                                                  32 * MK_KTILES * half + 32 * eh, lane, s2),
                                             kacc[eh]);
                }
            }
        }
        if (rt + 1 < RT) stager.store(img + ((rt + 1 - rt0) & 1) * MK_IMG, nxt, rt + 1);
        mcur = mnxt;
        mcur_mask = mnxt_mask;
        __syncthreads();
    }
    if (have) {
        // (the lane id from rare_lane(): the epilogue's lane offsets, formed before the loop and
        // kept across it, were the one value of the fp32 GT MODE 0 kernel that went to scratch)
        const int elane = rare_lane();
        float *tile = reinterpret_cast<float *>(img) + wave * (32 * MA_TLD);
        if constexpr (WANT_K) {
            T *gk_b = grad_k + dv.base + (size_t)j0 * dv.ld + 32 * MK_KTILES * half;
#pragma unroll
            for (int eh = 0; eh < MK_KTILES; eh++)
                store_acc_half(kacc[eh], scale, tile, gk_b + 32 * eh, dv.ld, S - j0, elane,
                               eh + 1 < MK_KTILES ? 32 : MA_ELAST);
        }
        if constexpr (WANT_V) {
            T *gv_b = grad_v + dv.base + (size_t)j0 * dv.ld + (MODE == 1 ? 0 : 64 * half);
#pragma unroll
            for (int eh = 0; eh < NVT; eh++)
                store_acc_half(vacc[eh], 1.0f, tile, gv_b + 32 * eh, dv.ld, S - j0, elane,
                               eh + 1 < NVT ? 32 : MA_ELAST);
        }
    }
}

// (Round 3 also built the backward as ONE launch per slice -- S, P, dP, dS once per tile pair, 60
// instead of 84 MFMA-equivalents, dQ carried through LDS: 164.6 us against the two kernels' 165.0 at
// the configs[1] shape, because neither form is bound by the matrix pipe.  DESIGN.md 5.11 keeps the
// measurements and the ablation; the kernel left the tree in round 4.)

static size_t mfma_forward_lds() {
    return 2 * MA_IMG + (size_t)MA_WAVES * (MA_WROWS + 2) * sizeof(float);
}

// ---- launchers of this head dimension (the d_head 64 unit dispatches to spt::e80's, e128's) ----
template <typename T>
static int launch_forward_t(const unsigned long long *masks, const unsigned char *cells,
                            const unsigned char *pool, const unsigned *sat, const T *q, const T *k,
                            const T *v, T *y, float *row_sum, float *bounds, int batch_size, int S,
                            float scale, float clamp, int heads, int kv_heads, int y_transposed,
                            hipStream_t s) {
    const int bpb = (S + MA_ROWS - 1) / MA_ROWS;
    const size_t lds = mfma_forward_lds();
    const dim3 grid((unsigned)batch_size * bpb), block(MA_THREADS);
#define SPT_MF(YT)                                                                               \
    do {                                                                                         \
        SPT_HIP_TRY(hipFuncSetAttribute((const void *)attention_mfma_forward_kernel<T, YT>,      \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));  \
        hipLaunchKernelGGL((attention_mfma_forward_kernel<T, YT>), grid, block, lds, s, masks, cells, pool, \
                           sat, q, k, v, y, row_sum, bounds, S, scale, clamp, heads, kv_heads,   \
                           bpb);                                                                 \
    } while (0)
    if (y_transposed) SPT_MF(true); else SPT_MF(false);
#undef SPT_MF
    SPT_LAUNCH_CHECK();
    return SPT_OK;
}

template <typename T>
static int launch_backward_t(const unsigned long long *masks, const unsigned char *cells,
                             const unsigned char *cells_t, const unsigned char *pool,
                             const unsigned char *pool_t, const unsigned *sat, const T *q, const T *k,
                             const T *v, const T *y, const T *grad_y, const float *row_sum,
                             const float *bounds, float *delta, T *grad_q, T *grad_k, T *grad_v,
                             int batch_size, int S, float scale, float clamp, int heads,
                             int kv_heads, int transposed, hipStream_t s) {
    const int bpb = (S + BW_ROWS - 1) / BW_ROWS;
    const dim3 grid((unsigned)batch_size * bpb), block(BW_THREADS);
    const size_t lds_r = 2 * MA_IMG + (size_t)BW_WAVES * MA_PARK,
                 lds_k = 2 * MK_IMG + (size_t)BW_WAVES * (MA_PARK + 2048);
    // 64 gradient columns per launch (the accumulators of 128 would not fit the registers
    // beside the operands' fragments): d_head 128 runs each kernel twice
#define SPT_MB(GT)                                                                              \
    do {                                                                                        \
        SPT_HIP_TRY(hipFuncSetAttribute(                                                        \
            (const void *)attention_mfma_backward_rows_kernel<T, GT>,                      \
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_r));                           \
        for (int half = 0; half < MA_ET / MR_QTILES; half++)                                    \
            hipLaunchKernelGGL((attention_mfma_backward_rows_kernel<T, GT>), grid, block, lds_r, \
                               s, masks, cells, pool, sat, q, k, v, grad_y, y, row_sum, bounds, \
                               grad_q, delta, S, scale, clamp, heads, kv_heads, bpb, half);     \
        if constexpr (MK_FUSED) {                                                               \
            SPT_KEYS(GT, 0, 0);                                                                 \
        } else {                                                                                \
            SPT_KEYS(GT, 1, 0);                                                                 \
            for (int half = 0; half < MA_ET / MK_KTILES; half++) SPT_KEYS(GT, 2, half);         \
        }                                                                                       \
    } while (0)
#define SPT_KEYS(GT, MODE, HALF)                                                                \
    do {                                                                                        \
        SPT_HIP_TRY(hipFuncSetAttribute(                                                        \
            (const void *)attention_mfma_backward_keys_kernel<T, GT, MODE>,                \
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_k));                           \
        hipLaunchKernelGGL((attention_mfma_backward_keys_kernel<T, GT, MODE>), grid, block, \
                           lds_k, s, masks, cells_t, pool_t, sat, q, k, v, grad_y, row_sum,     \
                           bounds, delta, grad_k, grad_v, S, scale, clamp, heads, kv_heads,     \
                           bpb, HALF);                                                          \
    } while (0)
    if (transposed) SPT_MB(true);
    else SPT_MB(false);
#undef SPT_MB
#undef SPT_KEYS
    SPT_LAUNCH_CHECK();
    return SPT_OK;
}

int launch_forward(const unsigned long long *masks, const unsigned char *cells,
                   const unsigned char *pool, const unsigned *sat, int dtype, const void *q,
                   const void *k, const void *v, void *y, float *row_sum, float *bounds,
                   int batch_size, int S, float scale, float clamp, int heads, int kv_heads,
                   int y_transposed, hipStream_t s) {
    if (dtype == SPT_BF16)
        return launch_forward_t<bf16_t>(masks, cells, pool, sat, (const bf16_t *)q, (const bf16_t *)k,
                                        (const bf16_t *)v, (bf16_t *)y, row_sum, bounds, batch_size, S,
                                        scale, clamp, heads, kv_heads, y_transposed, s);
    return launch_forward_t<float>(masks, cells, pool, sat, (const float *)q, (const float *)k,
                                   (const float *)v, (float *)y, row_sum, bounds, batch_size, S, scale,
                                   clamp, heads, kv_heads, y_transposed, s);
}

int launch_backward(const unsigned long long *masks, const unsigned char *cells,
                    const unsigned char *cells_t, const unsigned char *pool,
                    const unsigned char *pool_t, const unsigned *sat, int dtype, const void *q,
                    const void *k, const void *v, const void *y, const void *grad_y,
                    const float *row_sum, const float *bounds, float *delta, void *grad_q,
                    void *grad_k, void *grad_v, int batch_size, int S, float scale, float clamp,
                    int heads, int kv_heads, int transposed, hipStream_t s) {
    if (dtype == SPT_BF16)
        return launch_backward_t<bf16_t>(masks, cells, cells_t, pool, pool_t, sat, (const bf16_t *)q,
                                         (const bf16_t *)k, (const bf16_t *)v, (const bf16_t *)y,
                                         (const bf16_t *)grad_y, row_sum, bounds, delta,
                                         (bf16_t *)grad_q, (bf16_t *)grad_k, (bf16_t *)grad_v,
                                         batch_size, S, scale, clamp, heads, kv_heads, transposed, s);
    return launch_backward_t<float>(masks, cells, cells_t, pool, pool_t, sat, (const float *)q,
                                    (const float *)k, (const float *)v, (const float *)y,
                                    (const float *)grad_y, row_sum, bounds, delta, (float *)grad_q,
                                    (float *)grad_k, (float *)grad_v, batch_size, S, scale, clamp,
                                    heads, kv_heads, transposed, s);
}

MA_NS_CLOSE

#if MA_E_VALUE == 64    // the C entries: once
static int mfma_forward_any(const void *tiles, int layout, int dtype, const void *q,
                            const void *k, const void *v, void *y, float *row_sum, float *bounds,
                            int batch_size, int seq_length, int d_head, int nnz, float scale,
                            float clamp, int heads, int kv_heads, int y_transposed, void *stream) {
    using namespace spt;
    if (!tiles || !q || !k || !v || !y || !row_sum) return SPT_EINVAL;
    if (batch_size <= 0 || heads < 0) return SPT_EINVAL;
    if (layout != SPT_TILES_FULL && layout != SPT_TILES_COMPACT) return SPT_EINVAL;
    if (!mfma_shape_ok(seq_length, d_head, nnz)) return SPT_EUNSUP;
    if (heads > 0 && batch_size % heads != 0) return SPT_ESHAPE;
    const TileSet ts = carve_tiles(const_cast<void *>(tiles), batch_size, seq_length, layout);
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto fwd = d_head == 64 ? launch_forward : d_head == 80 ? e80::launch_forward : e128::launch_forward;
    return fwd(ts.masks, ts.cells, ts.pool, ts.sat, dtype, q, k, v, y, row_sum, bounds, batch_size,
               seq_length, scale, clamp, heads, kv_heads, y_transposed, s);
}

static int mfma_backward_any(const void *tiles, int layout, int dtype, const void *q,
                             const void *k, const void *v, const void *y, const void *grad_y,
                             const float *row_sum, const float *bounds, float *delta, void *grad_q,
                             void *grad_k, void *grad_v, int batch_size, int seq_length, int d_head,
                             int nnz, float scale, float clamp, int heads, int kv_heads,
                             int transposed, void *stream) {
    using namespace spt;
    if (!tiles || !q || !k || !v || !y || !grad_y || !row_sum || !delta || !grad_q || !grad_k ||
        !grad_v)
        return SPT_EINVAL;
    if (batch_size <= 0 || heads < 0) return SPT_EINVAL;
    if (layout != SPT_TILES_FULL && layout != SPT_TILES_COMPACT) return SPT_EINVAL;
    if (!mfma_shape_ok(seq_length, d_head, nnz)) return SPT_EUNSUP;
    if (heads > 0 && batch_size % heads != 0) return SPT_ESHAPE;
    if (transposed && (seq_length & 3)) return SPT_EUNSUP;
    const TileSet ts = carve_tiles(const_cast<void *>(tiles), batch_size, seq_length, layout);
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto bwd = d_head == 64 ? launch_backward : d_head == 80 ? e80::launch_backward : e128::launch_backward;
    return bwd(ts.masks, ts.cells, ts.cells_t, ts.pool, ts.pool_t, ts.sat, dtype, q, k, v, y, grad_y,
               row_sum, bounds, delta, grad_q, grad_k, grad_v, batch_size, seq_length, scale, clamp,
               heads, kv_heads, transposed, s);
}

extern "C" int spt_attention_mfma_forward(const void *tiles, int layout, const float *q,
                                          const float *k, const float *v, float *y,
                                          float *row_sum, float *bounds, int batch_size,
                                          int seq_length, int d_head, int nnz, float scale,
                                          float clamp, int heads, int y_transposed, void *stream) {
    return mfma_forward_any(tiles, layout, SPT_F32, q, k, v, y, row_sum, bounds, batch_size,
                            seq_length, d_head, nnz, scale, clamp, heads, heads, y_transposed, stream);
}

extern "C" int spt_attention_mfma_backward(const void *tiles, int layout, const float *q,
                                           const float *k, const float *v, const float *y,
                                           const float *grad_y, const float *row_sum,
                                           const float *bounds, float *delta, float *grad_q,
                                           float *grad_k, float *grad_v, int batch_size,
                                           int seq_length, int d_head, int nnz, float scale,
                                           float clamp, int heads, int transposed, void *stream) {
    return mfma_backward_any(tiles, layout, SPT_F32, q, k, v, y, grad_y, row_sum, bounds, delta,
                             grad_q, grad_k, grad_v, batch_size, seq_length, d_head, nnz, scale,
                             clamp, heads, heads, transposed, stream);
}

// Grouped key/value heads (fp32, [N, S, heads, E] layout only): k, v [N, S, kv_heads, E]; the
// backward's grad_k / grad_v are the per-QUERY-head partials [N, S, heads, E] (spt_head_group_sum
// reduces them).  Refusals before any launch.
static int kv_heads_ok(int batch_size, int heads, int kv_heads) {
    if (heads <= 0 || kv_heads <= 0) return SPT_ESHAPE;
    if (heads % kv_heads != 0 || batch_size <= 0 || batch_size % heads != 0) return SPT_ESHAPE;
    return SPT_OK;
}

extern "C" int spt_attention_mfma_forward_kv(const void *tiles, int layout, const float *q,
                                             const float *k, const float *v, float *y,
                                             float *row_sum, float *bounds, int batch_size,
                                             int seq_length, int d_head, int nnz, float scale,
                                             float clamp, int heads, int kv_heads,
                                             int y_transposed, void *stream) {
    if (!tiles || !q || !k || !v || !y || !row_sum) return SPT_EINVAL;
    if (const int rc = kv_heads_ok(batch_size, heads, kv_heads)) return rc;
    return mfma_forward_any(tiles, layout, SPT_F32, q, k, v, y, row_sum, bounds, batch_size,
                            seq_length, d_head, nnz, scale, clamp, heads, kv_heads, y_transposed,
                            stream);
}

extern "C" int spt_attention_mfma_backward_kv(const void *tiles, int layout, const float *q,
                                              const float *k, const float *v, const float *y,
                                              const float *grad_y, const float *row_sum,
                                              const float *bounds, float *delta, float *grad_q,
                                              float *grad_k_parts, float *grad_v_parts,
                                              int batch_size, int seq_length, int d_head, int nnz,
                                              float scale, float clamp, int heads, int kv_heads,
                                              int transposed, void *stream) {
    if (!tiles || !q || !k || !v || !y || !grad_y || !row_sum || !delta || !grad_q ||
        !grad_k_parts || !grad_v_parts)
        return SPT_EINVAL;
    if (const int rc = kv_heads_ok(batch_size, heads, kv_heads)) return rc;
    return mfma_backward_any(tiles, layout, SPT_F32, q, k, v, y, grad_y, row_sum, bounds, delta,
                             grad_q, grad_k_parts, grad_v_parts, batch_size, seq_length, d_head, nnz,
                             scale, clamp, heads, kv_heads, transposed, stream);
}

extern "C" int spt_attention_mfma_forward_bf16(const void *tiles, int layout, const uint16_t *q,
                                               const uint16_t *k, const uint16_t *v, uint16_t *y,
                                               float *row_sum, float *bounds, int batch_size,
                                               int seq_length, int d_head, int nnz, float scale,
                                               float clamp, int heads, int y_transposed,
                                               void *stream) {
    return mfma_forward_any(tiles, layout, SPT_BF16, q, k, v, y, row_sum, bounds, batch_size,
                            seq_length, d_head, nnz, scale, clamp, heads, heads, y_transposed, stream);
}

extern "C" int spt_attention_mfma_backward_bf16(const void *tiles, int layout, const uint16_t *q,
                                                const uint16_t *k, const uint16_t *v,
                                                const uint16_t *y, const uint16_t *grad_y,
                                                const float *row_sum, const float *bounds,
                                                float *delta, uint16_t *grad_q, uint16_t *grad_k,
                                                uint16_t *grad_v, int batch_size, int seq_length,
                                                int d_head, int nnz, float scale, float clamp,
                                                int heads, int transposed, void *stream) {
    return mfma_backward_any(tiles, layout, SPT_BF16, q, k, v, y, grad_y, row_sum, bounds, delta,
                             grad_q, grad_k, grad_v, batch_size, seq_length, d_head, nnz, scale,
                             clamp, heads, heads, transposed, stream);
}
#endif
