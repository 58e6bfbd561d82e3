// route_rank.h -- the routed FFN's top-k ranking of one token's block scores: ONE definition for the
// bucketing (routing.hip) and for the per-group selection counts the pass that forms the router's
// logits leaves (lora_side.hip).  Integer compares only; nothing here touches the matrix cores.
#ifndef SPT_ROUTE_RANK_H
#define SPT_ROUTE_RANK_H

#include "spt_common.h"

namespace spt {

constexpr int RT_MAXG = 8;
constexpr int RT_GROUP = 16;        // tokens per group of the selection counts (a tile of spt_lora_down)

// Orderable key of a probability: ascending unsigned order == ascending float order, -0 == +0,
// and every NaN is the LARGEST key (torch.topk also ranks NaN above every number).  The rank
// below is then a total order for any input, so exactly k bits are set per token: with the
// float comparisons used before, a NaN compared false against everything, ranked 0 and let
// a token select more than k blocks -- writes past the T * k rows the caller allocated.
__device__ __forceinline__ unsigned order_key(float x) {
    if (x != x) return 0xFFFFFFFFu;
    const unsigned b = __float_as_uint(x + 0.0f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

template <int MG>
__device__ __forceinline__ unsigned select_topk(const float (&v)[MG], int G, int k) {
    unsigned key[MG];
#pragma unroll
    for (int j = 0; j < MG; j++) key[j] = order_key(v[j]);
    unsigned mask = 0u;
#pragma unroll
    for (int j = 0; j < MG; j++) {
        int rank = 0;
#pragma unroll
        for (int i = 0; i < MG; i++)
            rank += (i < G) && (key[i] > key[j] || (key[i] == key[j] && i < j));
        if (j < G && rank < k) mask |= 1u << j;
    }
    return mask;
}

}  // namespace spt

#endif  // SPT_ROUTE_RANK_H
