"""Routed FFN on the MI355X: device-side bucketing + grouped MFMA GEMMs.

Used by the routed FFN layers when the activations live on the GPU and the base
weights are frozen (the LoRA variants the upgrader installs: the hot path).  Nothing
here reads a bucket size on the host: the (token, block) pairs are sorted by block with
device ops, bucket boundaries stay in a device int32 ``offsets`` tensor, and every
block GEMM of a layer is ONE launch of ``spt_grouped_gemm`` (fp32 MFMA,
``spt-proto_amd/csrc/grouped_gemm.hip`` and its units) -- compare the reference's loop of boolean-mask
gathers and per-block cuBLAS calls (``layers/tuning/lora_ffn.py:87-111``).

Row space: P = T * k rows, row p = the p-th (token, block) pair in block-major order
(stable in the token id, i.e. the reference's ``x[mask]`` order inside each block).

Trainable base weights (the plain RoutedFFN / RoutedLLaMaFFN in training) take the grouped path
too when ``TRAINABLE_WEIGHTS`` is on: their gradients are grouped products contracted over the
bucket rows (``spt_grouped_gemm_wgrad``), written straight into the parameters' layouts.

bf16 storage (the plain routed FFNs whose activations and weights are ALL bf16): the same bucketing
(the router's probabilities widened to fp32 for it) and the bf16 kernels -- ``spt_grouped_gemm_bf16``,
``spt_grouped_gemm_wgrad_bf16``, ``spt_rows_combine_bf16``, ``spt_swiglu_*_bf16``: fp32 accumulation of
the exact products of the stored bf16 values, each result rounded once when stored.  The LoRA routed
FFNs in bf16 (RoutedLoRAFFNBf16 / RoutedLoRALLaMAFFNBf16, opt-in through LORA_BF16) add the K extension
(``spt_grouped_gemm_bf16_ext``), ``spt_lora_down*_bf16`` and ``spt_tall_tn_bf16``, with fp32 rank-r sides.
"""
import os
from typing import NamedTuple

import torch

from naive_gpt import ext
from naive_gpt.layers.tuning import recompute


class Buckets(NamedTuple):
    token: torch.Tensor     # [P] int32: token id of each row
    token_long: torch.Tensor
    block: torch.Tensor     # [P] int64: block id of each row (ascending)
    offsets: torch.Tensor   # [G + 1] int32, device
    coeff: torch.Tensor     # [P] router probability of (token, block), differentiable
    n_blocks: int
    pos: torch.Tensor       # [T, k] int32: the rows of each token (inverse of `token`)


class _RouteTopK(torch.autograd.Function):
    """prob [T, G] -> the block-sorted rows AND their coefficients scale * prob[token, block], one
    launch (routing.hip); backward: the coefficients' gradient scattered back, one launch.
    (As torch operators: two int64 copies, two index computations, a gather and a product
    forward; a product, a zero fill and an index_add backward -- x 24 layers.)"""

    @staticmethod
    def forward(ctx, prob, k, scale):
        token, block, offsets, pos, token_long, block_long, coeff = \
            ext.route_topk_coeff(prob.contiguous(), k, scale)
        ctx.save_for_backward(pos, block)
        ctx.scale, ctx.n_blocks = scale, prob.size(1)
        ctx.mark_non_differentiable(token, block, offsets, pos, token_long, block_long)
        # (or autograd hands the backward a zero tensor for each of the six index outputs: six fills)
        ctx.set_materialize_grads(False)
        return token, block, offsets, pos, token_long, block_long, coeff

    @staticmethod
    def backward(ctx, *grads):
        if grads[6] is None:
            return None, None, None
        pos, block = ctx.saved_tensors
        return ext.route_coeff_backward(grads[6].contiguous(), pos, block, ctx.scale,
                                        ctx.n_blocks), None, None


def make_buckets(prob: torch.Tensor, k: int, scale: float = 1.0) -> Buckets:
    """prob [T, G] router probabilities -> block-sorted (token, block) rows; `coeff` =
    scale * the rows' probabilities."""
    n_tokens, n_blocks = prob.shape
    if prob.is_cuda and prob.dtype == torch.float32 \
            and ext.route_topk_supported(n_tokens, n_blocks):
        # one launch (routing.hip) instead of topk + argsort + bincount + cumsum + gathers
        token, _, offsets, pos, token_long, block_long, coeff = _RouteTopK.apply(prob, k, float(scale))
        ext.note_path('route_topk', 'kernel')
        return Buckets(token=token, token_long=token_long, block=block_long, offsets=offsets,
                       coeff=coeff, n_blocks=n_blocks, pos=pos)
    ext.note_path('route_topk', 'torch', fallback=prob.is_cuda,
                  why=lambda: 'prob {} {}: spt_route_topk takes fp32, <= 8 blocks, <= 65536 tokens'.format(
                      tuple(prob.shape), prob.dtype))
    indices = torch.topk(prob, k=k, dim=-1, sorted=False).indices       # [T, k]
    block = indices.reshape(-1)
    order = torch.argsort(block, stable=True)
    token_long = torch.div(order, k, rounding_mode='floor')
    block_sorted = block.index_select(0, order)
    counts = torch.bincount(block_sorted, minlength=n_blocks)
    offsets = torch.zeros([n_blocks + 1], dtype=torch.int32, device=prob.device)
    offsets[1:] = torch.cumsum(counts, dim=0)
    coeff = prob.reshape(-1).index_select(0, token_long * n_blocks + block_sorted)
    if scale != 1.0:
        coeff = scale * coeff
    # row p holds the flat (token, choice) pair order[p]: invert the permutation
    pos = torch.empty_like(order)
    pos[order] = torch.arange(order.numel(), device=order.device)
    return Buckets(token=token_long.int(), token_long=token_long, block=block_sorted,
                   offsets=offsets, coeff=coeff, n_blocks=n_blocks,
                   pos=pos.view(n_tokens, k).int())


# Trainable base weights of the plain routed FFNs on the grouped path (RoutedFFNTrain /
# RoutedLLaMAFFNTrain below) instead of the per-block loop.  Opt-in until it is measured as the
# default; read at call time (tests flip it).
TRAINABLE_WEIGHTS = os.environ.get('SPT_ROUTED_TRAINABLE', '0') != '0'

COEFF_FLOOR = 1e-12
# h (one reader) goes to its GEMM as fp32 rows, no image: -0.36 ms per configs[2] step, A/B on one
# box (the same for x: +0.26 ms, for dy: +-0: both keep their images)
H_A32 = os.environ.get('SPT_H_A32', '1') != '0'
ROUTER_RIDES = os.environ.get('SPT_ROUTER_RIDES', '1') != '0'
# the router's small launches: the selection counts ride the logits' launch (forward), and
# coefficient gradient + the two [T, r] combines + d logit are one launch (backward).  '0': the separate calls.
ROUTER_COUNTS = os.environ.get('SPT_ROUTER_COUNTS', '1') != '0'
ROUTER_BACKWARD_FUSED = os.environ.get('SPT_ROUTER_BACKWARD_FUSED', '1') != '0'


def _floor(coeff: torch.Tensor) -> torch.Tensor:
    """The coefficient gradients below are recovered as (a dot that contains c) / c, where the
    reference differentiates c * (x W^T + b) directly.  c = 2 sigmoid(logit) underflows to 0
    for logit < -104 (0 / 0 = NaN here, a finite number there) and the quotient amplifies the
    fp32 cancellation error of the numerator by 1 / c.  Both are harmless AFTER the chain
    rule -- d c / d logit = c (1 - c / 2), so the factor 1 / c cancels and what reaches the
    router is (numerator error) * (1 - c / 2) -- provided the division itself stays finite:
    hence a floor far below any coefficient that still has a gradient in fp32."""
    return coeff.clamp_min(COEFF_FLOOR)


class GroupedLinear(torch.autograd.Function):
    """out[p] = rowscale[p] * (a[gather[p]] @ W_g(p)^T + bias[g(p)]) for frozen weights.

    ``view`` = (n, k, group_stride, ldn, ldk) describes W_g(n, kk) inside ``weight``'s
    storage.  Gradients flow to ``a`` (through the opposite-orientation kernel and, when
    rows were gathered, an ``index_add_``) and to ``rowscale``."""

    @staticmethod
    def forward(ctx, a, weight, offsets, view, gather, gather_long, bias, rowscale):
        n, k, gstride, ldn, ldk = view
        n_groups = offsets.numel() - 1
        out = ext.grouped_gemm(a, weight, offsets, n_groups, n, k, gstride, ldn, ldk,
                               gather=gather, bias=bias, rowscale=rowscale)
        ctx.view = view
        ctx.a_rows = a.size(0)
        # (a and gather only when the weight wants a gradient: the frozen path keeps no activation)
        wants_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[6]
        ctx.save_for_backward(weight, offsets, gather_long, rowscale, out,
                              a if wants_w else None, gather if wants_w else None)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        weight, offsets, gather_long, rowscale, out, a, gather = ctx.saved_tensors
        n, k, gstride, ldn, ldk = ctx.view
        n_groups = offsets.numel() - 1
        grad_out = grad_out.contiguous()
        grad_a = grad_scale = None
        if ctx.needs_input_grad[7] and rowscale is not None:
            # out = s * u  ->  ds = <dout, u> = <dout, out> / s   (s = 2 sigmoid(.) > 0)
            grad_scale = (grad_out * out).sum(dim=-1) / _floor(rowscale)
        if ctx.needs_input_grad[0]:
            # d a[src(p), kk] = s[p] * sum_n dout[p, n] W_g(n, kk): roles of n and k swap
            rows = ext.grouped_gemm(grad_out, weight, offsets, n_groups, k, n, gstride,
                                    ldk, ldn, rowscale=rowscale)
            if gather_long is None:
                grad_a = rows
            else:
                grad_a = torch.zeros([ctx.a_rows, k], dtype=rows.dtype, device=rows.device)
                grad_a.index_add_(0, gather_long, rows)
        grad_w = grad_bias = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[6]:
            # dW_g(n, kk) = sum over the rows p of g of s[p] dout[p, n] a[src(p), kk]; d bias[g, n] =
            # sum_p s[p] dout[p, n]: one grouped product over the bucket rows, into W's own layout
            if ldk != 1:
                raise NotImplementedError('GroupedLinear: weight gradients of k-contiguous views only')
            covered = n_groups * n * k == weight.numel()
            grad_w = torch.empty_like(weight) if covered else torch.zeros_like(weight)
            _, grad_bias = ext.grouped_gemm_wgrad(grad_out, a, offsets, ctx.view, grad_out.size(0),
                                                  gather_a=gather, rowscale=rowscale, out=grad_w.view(-1),
                                                  want_bias=ctx.needs_input_grad[6])
            if not ctx.needs_input_grad[1]:
                grad_w = None
        return grad_a, grad_w, None, None, None, None, grad_bias, grad_scale


def grouped_linear(a, weight, offsets, view, gather=None, gather_long=None, bias=None,
                   rowscale=None):
    return GroupedLinear.apply(a, weight, offsets, view, gather, gather_long, bias, rowscale)


def dtype_mix(x: torch.Tensor, *weights):
    """None when x and every given weight are all fp32 or all bf16, else what mixes (the grouped
    paths take one storage type per layer: no silent conversion)."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        return 'x {}: fp32 or bf16 only'.format(x.dtype)
    for w in weights:
        if w is not None and w.dtype != x.dtype:
            return 'x {} with a {} weight {}: one dtype per layer'.format(x.dtype, w.dtype, tuple(w.shape))
    return None


def bf16_shapes(d: int, bs: int) -> bool:
    """spt_grouped_gemm_bf16 takes the routed FFN's four products (both views of fc1 / fc2 and their
    swapped dX views) when d and the block size are multiples of 64 (k % 64, 16-byte rows)."""
    return d % 64 == 0 and bs % 64 == 0


def trainable_unusable(x: torch.Tensor, act, *weights):
    """None when the trainable grouped path takes these operands, else the reason it does not."""
    if x.is_cuda and x.dtype == torch.bfloat16:
        if act is None:
            return 'activation without a fused epilogue (ReLU, exact GELU, SiLU)'
        for w in weights:
            if not w.is_cuda or w.dtype != torch.bfloat16 or not w.is_contiguous():
                return 'bf16 x with weight {} {}: bf16 contiguous CUDA weights only'.format(tuple(w.shape), w.dtype)
        return None
    if not x.is_cuda or x.dtype != torch.float32:
        return 'x {} {} (fp32 CUDA activations only)'.format(tuple(x.shape), x.dtype)
    if act is None:
        return 'activation without a fused epilogue (ReLU, exact GELU, SiLU)'
    for w in weights:
        if not w.is_cuda or w.dtype != torch.float32 or not w.is_contiguous():
            return 'weight {} {}: fp32 contiguous CUDA weights only'.format(tuple(w.shape), w.dtype)
    return None


def _fresh_image(w: torch.Tensor):
    """The split image of a TRAINABLE weight: made from its current values every call (a cache
    keyed on `_version` misses writes through `.data`, which optimizers and loaders use)."""
    return ext.split_bf16(w.detach())


class RoutedFFNTrain(torch.autograd.Function):
    """y = RoutedFFN(x) with trainable base weights (reference: layers/sparse/feedforward.py:66-85;
    the blocks are not weighted by the router, which therefore gets no gradient):

        h  = act(x[token] W1_g^T + b1_g)      spt_grouped_gemm_fused, EPI_ACT
        ys = h W2_g^T;  y = b2 + sum over the token's rows of ys     fused GEMM + spt_rows_combine
      backward
        ds  = (dy[token] W2_g) * act'(s)      EPI_DACT
        dW2 = dy[token]^T h per block,  dW1 = ds^T x[token] per block (+ db1)   spt_grouped_gemm_wgrad
        dx  = sum over the token's rows of ds W1_g

    For ReLU the derivative must be that of the EXACT fp32 pre-activation (a split-sign mask is an
    O(1) error in a row of dW1): the forward is the fused EPI_ACT with the row norms of x and of the
    current W1, which recomputes the elements within the split's error of zero in fp32, and the
    backward's mask is h > 0.  Norms and images are formed from the weights' values at the call."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, token, offsets, pos, nb: int, act: int):
        d_ff, d = w1.shape
        bs, rows = d_ff // nb, token.numel()
        relu = act == ext.ACT_RELU
        imgs = _images_usable(x, w1, w2, d, bs)
        w1_img, w2_img = (_fresh_image(w1), _fresh_image(w2)) if imgs else (None, None)
        h, s = ext.grouped_gemm_fused(
            x, w1, offsets, nb, n=bs, k=d, w_group_stride=bs * d, w_ldn=d, w_ldk=1, n_rows=rows,
            gather=token, bias=b1.detach().contiguous(), epilogue=ext.EPI_ACT, activation=act,
            keep_preact=not relu, w_image=w1_img,
            a_norm=ext.row_norms(x) if relu else None, w_norm=ext.row_norms(w1) if relu else None)
        ys = ext.grouped_gemm_fused(h, w2, offsets, nb, n=d, k=bs, w_group_stride=bs, w_ldn=d_ff,
                                    w_ldk=1, n_rows=rows, w_image=w2_img)
        y = ext.rows_combine(ys, pos, bias=b2.detach().contiguous())
        ctx.nb, ctx.act, ctx.imgs = nb, act, (w1_img, w2_img)
        ctx.save_for_backward(x, h, s, w1, w2, token, offsets, pos)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, h, s, w1, w2, token, offsets, pos = ctx.saved_tensors
        w1_img, w2_img = ctx.imgs
        nb, act = ctx.nb, ctx.act
        d_ff, d = w1.shape
        bs, rows = d_ff // nb, token.numel()
        dy = dy.contiguous()
        ds, _, _ = ext.grouped_gemm_fused(
            dy, w2, offsets, nb, n=bs, k=d, w_group_stride=bs, w_ldn=1, w_ldk=d_ff, n_rows=rows,
            gather=token, epilogue=ext.EPI_DACT, activation=act, h_in=h, s_in=s, w_image=w2_img,
            raw_dots=True)
        grad_w2 = grad_b2 = grad_w1 = grad_b1 = grad_x = None
        if ctx.needs_input_grad[3]:
            grad_w2, _ = ext.grouped_gemm_wgrad(dy, h, offsets, (d, bs, bs, d_ff, 1), rows, gather_grad=token)
            grad_w2 = grad_w2.view(d, d_ff)
        if ctx.needs_input_grad[4]:
            grad_b2 = dy.sum(dim=0)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            grad_w1, grad_b1 = ext.grouped_gemm_wgrad(ds, x, offsets, (bs, d, bs * d, d, 1), rows,
                                                      gather_a=token, want_bias=ctx.needs_input_grad[2])
            grad_w1 = grad_w1.view(d_ff, d) if ctx.needs_input_grad[1] else None
            grad_b1 = grad_b1.view(d_ff) if grad_b1 is not None else None
        if ctx.needs_input_grad[0]:
            dxs = ext.grouped_gemm_fused(ds, w1, offsets, nb, n=d, k=bs, w_group_stride=bs * d, w_ldn=1,
                                         w_ldk=d, n_rows=rows, w_image=w1_img)
            grad_x = ext.rows_combine(dxs, pos)
        return grad_x, grad_w1, grad_b1, grad_w2, grad_b2, None, None, None, None, None


class RoutedLLaMAFFNTrain(torch.autograd.Function):
    """y = RoutedLLaMaFFN(x) with trainable base weights (reference: feedforward.py:133-187):

        g = x[token] G_g^T,  sd = x[token] S_g^T      two grouped GEMMs
        h = act(g) * sd                               spt_swiglu_forward (SiLU), else torch
        y = sum over the token's rows of h D_g^T      fused GEMM + spt_rows_combine
      backward
        dh = dy[token] D_g;  dg, dsd through h = act(g) * sd     spt_swiglu_backward (SiLU)
        dD = dy[token]^T h,  dG = dg^T x[token],  dS = dsd^T x[token] per block   spt_grouped_gemm_wgrad
        dx = sum over the token's rows of dg G_g + dsd S_g      (the second GEMM accumulates)"""

    @staticmethod
    def forward(ctx, x, wg, ws, wd, token, offsets, pos, nb: int, activation):
        d_ff, d = wg.shape
        bs, rows = d_ff // nb, token.numel()
        imgs = _images_usable(x, wg, wd, d, bs)
        wg_img, ws_img, wd_img = (_fresh_image(wg), _fresh_image(ws), _fresh_image(wd)) if imgs \
            else (None, None, None)

        def up(w, img):
            return ext.grouped_gemm_fused(x, w, offsets, nb, n=bs, k=d, w_group_stride=bs * d, w_ldn=d,
                                          w_ldk=1, n_rows=rows, gather=token, w_image=img)

        g, sd = up(wg, wg_img), up(ws, ws_img)
        silu = isinstance(activation, torch.nn.SiLU) and ext.swiglu_supported(g, sd)
        ext.note_path('swiglu', 'kernel' if silu else 'torch', fallback=not silu,
                      why=lambda: 'activation {} on {}'.format(type(activation).__name__, tuple(g.shape)))
        h = ext.swiglu_forward(g, sd) if silu else activation(g) * sd
        ys = ext.grouped_gemm_fused(h, wd, offsets, nb, n=d, k=bs, w_group_stride=bs, w_ldn=d_ff,
                                    w_ldk=1, n_rows=rows, w_image=wd_img)
        y = ext.rows_combine(ys, pos)
        ctx.nb, ctx.activation, ctx.silu, ctx.imgs = nb, activation, silu, (wg_img, ws_img, wd_img)
        ctx.save_for_backward(x, g, sd, h, wg, ws, wd, token, offsets, pos)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g, sd, h, wg, ws, wd, token, offsets, pos = ctx.saved_tensors
        wg_img, ws_img, wd_img = ctx.imgs
        nb = ctx.nb
        d_ff, d = wg.shape
        bs, rows = d_ff // nb, token.numel()
        dy = dy.contiguous()
        dh = ext.grouped_gemm_fused(dy, wd, offsets, nb, n=bs, k=d, w_group_stride=bs, w_ldn=1,
                                    w_ldk=d_ff, n_rows=rows, gather=token, w_image=wd_img)
        grad_wg = grad_ws = grad_wd = grad_x = None
        if ctx.needs_input_grad[3]:
            grad_wd, _ = ext.grouped_gemm_wgrad(dy, h, offsets, (d, bs, bs, d_ff, 1), rows, gather_grad=token)
            grad_wd = grad_wd.view(d, d_ff)
        if ctx.silu:
            dg, dsd, _, _, _ = ext.swiglu_backward(dh, g, sd)
        else:
            with torch.enable_grad():
                g_ = g.detach().requires_grad_(True)
                ag = ctx.activation(g_)
                dg, = torch.autograd.grad(ag, g_, dh * sd)
            dsd = dh * ag.detach()
        del dh
        if ctx.needs_input_grad[1]:
            grad_wg = ext.grouped_gemm_wgrad(dg, x, offsets, (bs, d, bs * d, d, 1), rows,
                                             gather_a=token)[0].view(d_ff, d)
        if ctx.needs_input_grad[2]:
            grad_ws = ext.grouped_gemm_wgrad(dsd, x, offsets, (bs, d, bs * d, d, 1), rows,
                                             gather_a=token)[0].view(d_ff, d)
        if ctx.needs_input_grad[0]:
            dxs = ext.grouped_gemm_fused(dg, wg, offsets, nb, n=d, k=bs, w_group_stride=bs * d, w_ldn=1,
                                         w_ldk=d, n_rows=rows, w_image=wg_img)
            ext.grouped_gemm_fused(dsd, ws, offsets, nb, n=d, k=bs, w_group_stride=bs * d, w_ldn=1,
                                   w_ldk=d, n_rows=rows, w_image=ws_img, out=dxs, accumulate=True)
            grad_x = ext.rows_combine(dxs, pos)
        return grad_x, grad_wg, grad_ws, grad_wd, None, None, None, None, None


def usable(x: torch.Tensor, *frozen_weights) -> bool:
    """The grouped-GEMM path applies to fp32 CUDA activations and frozen base weights."""
    if not x.is_cuda or x.dtype != torch.float32:
        return False
    for w in frozen_weights:
        if w is None:
            continue
        if w.requires_grad or not w.is_contiguous() or w.dtype != torch.float32:
            return False
    return True


def f16_unusable(x: torch.Tensor, rank: int, fused: bool, d: int, bs: int):
    """Block weights stored in halves (utils.tuning.store_frozen_fp16) run from their images alone, which
    the FUSED grouped path with whole 32-element blocks provides: None when this call is such a one, else
    the reason it is not (the layer then upcasts the weights for the call and notes the fallback)."""
    if not x.is_cuda:
        return 'x on {}'.format(x.device)
    if not fused:
        return 'the fused grouped path does not take this layer (activation, rank {}, router, fc2.bias)'.format(rank)
    if d % 32 != 0 or bs % 32 != 0:
        return 'd_model {} / block size {}: the image path takes multiples of 32'.format(d, bs)
    return None


def _w_image(w: torch.Tensor, imgs: bool):
    """The weight's image where the call runs from images -- always, for a weight stored in halves (the
    GEMMs that read a fp32 weight through registers read a fp16 one from its image: the same MFMAs on
    the same fragments in the same order)."""
    return ext.weight_image(w) if imgs or w.dtype == torch.float16 else None


def bf16_usable(x: torch.Tensor, *frozen_weights) -> bool:
    """The bf16 grouped path of the PLAIN routed FFNs (feedforward.py; the LoRA routed variants have their
    own, lora_bf16_usable): bf16 CUDA activations and frozen bf16 base weights, every one of them."""
    if not x.is_cuda or x.dtype != torch.bfloat16:
        return False
    for w in frozen_weights:
        if w is None:
            continue
        if w.requires_grad or not w.is_contiguous() or w.dtype != torch.bfloat16:
            return False
    return True


class RoutedFFNTrainBf16(torch.autograd.Function):
    """RoutedFFNTrain on bf16 storage (x, weights, biases, activations and gradients bf16):

        h  = act(x[token] W1_g^T + b1_g)      spt_grouped_gemm_bf16, EPI_ACT (pre-activation kept but for ReLU)
        ys = h W2_g^T;  y = b2 + sum over the token's rows of ys     spt_grouped_gemm_bf16 + spt_rows_combine_bf16
      backward
        ds  = (dy[token] W2_g) * act'(s)      EPI_DACT
        dW2 = dy[token]^T h,  dW1 = ds^T x[token] (+ db1) per block      spt_grouped_gemm_wgrad_bf16
        dx  = sum over the token's rows of ds W1_g

    The products of bf16 values are exact in the fp32 accumulator, so there is no near-the-kink
    recomputation: the ReLU mask is the sign of the pre-activation the kernel computed (h > 0)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, token, offsets, pos, nb: int, act: int):
        d_ff, d = w1.shape
        bs, rows = d_ff // nb, token.numel()
        relu = act == ext.ACT_RELU
        h, s = ext.grouped_gemm_bf16(x, w1, offsets, nb, n=bs, k=d, w_group_stride=bs * d, w_ldn=d, w_ldk=1,
                                     n_rows=rows, gather=token, bias=b1.detach().contiguous(),
                                     epilogue=ext.EPI_ACT, activation=act, keep_preact=not relu)
        ys = ext.grouped_gemm_bf16(h, w2, offsets, nb, n=d, k=bs, w_group_stride=bs, w_ldn=d_ff, w_ldk=1,
                                   n_rows=rows)
        y = ext.rows_combine(ys, pos, bias=b2.detach().contiguous())
        ctx.nb, ctx.act = nb, act
        ctx.save_for_backward(x, h, s, w1, w2, token, offsets, pos)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, h, s, w1, w2, token, offsets, pos = ctx.saved_tensors
        nb, act = ctx.nb, ctx.act
        d_ff, d = w1.shape
        bs, rows = d_ff // nb, token.numel()
        dy = dy.contiguous()
        ds = ext.grouped_gemm_bf16(dy, w2, offsets, nb, n=bs, k=d, w_group_stride=bs, w_ldn=1, w_ldk=d_ff,
                                   n_rows=rows, gather=token, epilogue=ext.EPI_DACT, activation=act,
                                   h_in=h, s_in=s)
        grad_w2 = grad_b2 = grad_w1 = grad_b1 = grad_x = None
        if ctx.needs_input_grad[3]:
            grad_w2 = ext.grouped_gemm_wgrad(dy, h, offsets, (d, bs, bs, d_ff, 1), rows,
                                             gather_grad=token)[0].view(d, d_ff)
        if ctx.needs_input_grad[4]:
            grad_b2 = dy.sum(dim=0)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            grad_w1, grad_b1 = ext.grouped_gemm_wgrad(ds, x, offsets, (bs, d, bs * d, d, 1), rows,
                                                      gather_a=token, want_bias=ctx.needs_input_grad[2])
            grad_w1 = grad_w1.view(d_ff, d) if ctx.needs_input_grad[1] else None
            grad_b1 = grad_b1.view(d_ff) if grad_b1 is not None else None
        if ctx.needs_input_grad[0]:
            dxs = ext.grouped_gemm_bf16(ds, w1, offsets, nb, n=d, k=bs, w_group_stride=bs * d, w_ldn=1, w_ldk=d,
                                        n_rows=rows)
            grad_x = ext.rows_combine(dxs, pos)
        return grad_x, grad_w1, grad_b1, grad_w2, grad_b2, None, None, None, None, None


class RoutedLLaMAFFNTrainBf16(torch.autograd.Function):
    """RoutedLLaMAFFNTrain on bf16 storage: the four grouped products on spt_grouped_gemm_bf16, the
    gradients on spt_grouped_gemm_wgrad_bf16, h = silu(g) * sd and its derivative on
    spt_swiglu_*_bf16 (another activation: torch, as on the fp32 path)."""

    @staticmethod
    def forward(ctx, x, wg, ws, wd, token, offsets, pos, nb: int, activation):
        d_ff, d = wg.shape
        bs, rows = d_ff // nb, token.numel()

        def up(w):
            return ext.grouped_gemm_bf16(x, w, offsets, nb, n=bs, k=d, w_group_stride=bs * d, w_ldn=d, w_ldk=1,
                                         n_rows=rows, gather=token)

        g, sd = up(wg), up(ws)
        silu = isinstance(activation, torch.nn.SiLU) and ext.swiglu_bf16_supported(g, sd)
        ext.note_path('swiglu', 'kernel_bf16' if silu else 'torch', fallback=not silu,
                      why=lambda: 'activation {} on {}'.format(type(activation).__name__, tuple(g.shape)))
        h = ext.swiglu_forward_bf16(g, sd) if silu else activation(g) * sd
        ys = ext.grouped_gemm_bf16(h, wd, offsets, nb, n=d, k=bs, w_group_stride=bs, w_ldn=d_ff, w_ldk=1,
                                   n_rows=rows)
        y = ext.rows_combine(ys, pos)
        ctx.nb, ctx.activation, ctx.silu = nb, activation, silu
        ctx.save_for_backward(x, g, sd, h, wg, ws, wd, token, offsets, pos)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g, sd, h, wg, ws, wd, token, offsets, pos = ctx.saved_tensors
        nb = ctx.nb
        d_ff, d = wg.shape
        bs, rows = d_ff // nb, token.numel()
        dy = dy.contiguous()
        dh = ext.grouped_gemm_bf16(dy, wd, offsets, nb, n=bs, k=d, w_group_stride=bs, w_ldn=1, w_ldk=d_ff,
                                   n_rows=rows, gather=token)
        grad_wg = grad_ws = grad_wd = grad_x = None
        if ctx.needs_input_grad[3]:
            grad_wd = ext.grouped_gemm_wgrad(dy, h, offsets, (d, bs, bs, d_ff, 1), rows,
                                             gather_grad=token)[0].view(d, d_ff)
        if ctx.silu:
            dg, dsd = ext.swiglu_backward_bf16(dh, g, sd)
        else:
            with torch.enable_grad():
                g_ = g.detach().requires_grad_(True)
                ag = ctx.activation(g_)
                dg, = torch.autograd.grad(ag, g_, dh * sd)
            dsd = dh * ag.detach()
        del dh
        if ctx.needs_input_grad[1]:
            grad_wg = ext.grouped_gemm_wgrad(dg, x, offsets, (bs, d, bs * d, d, 1), rows,
                                             gather_a=token)[0].view(d_ff, d)
        if ctx.needs_input_grad[2]:
            grad_ws = ext.grouped_gemm_wgrad(dsd, x, offsets, (bs, d, bs * d, d, 1), rows,
                                             gather_a=token)[0].view(d_ff, d)
        if ctx.needs_input_grad[0]:
            dxs = ext.grouped_gemm_bf16(dg, wg, offsets, nb, n=d, k=bs, w_group_stride=bs * d, w_ldn=1, w_ldk=d,
                                        n_rows=rows)
            ext.grouped_gemm_bf16(dsd, ws, offsets, nb, n=d, k=bs, w_group_stride=bs * d, w_ldn=1, w_ldk=d,
                                  n_rows=rows, out=dxs, accumulate=True)
            grad_x = ext.rows_combine(dxs, pos)
        return grad_x, grad_wg, grad_ws, grad_wd, None, None, None, None, None


# ---------------------------------------------------------------- the fused LoRA routed FFN

def activation_code(module):
    """ext activation id of an nn activation module, or None when the fused epilogue does
    not implement it (the caller then composes the layer from grouped_linear + torch)."""
    from torch import nn
    if isinstance(module, nn.ReLU):
        return ext.ACT_RELU
    if isinstance(module, nn.GELU) and getattr(module, 'approximate', 'none') == 'none':
        return ext.ACT_GELU
    if isinstance(module, nn.SiLU):
        return ext.ACT_SILU
    return None


def _own_block(wide: torch.Tensor, block: torch.Tensor, n_blocks: int) -> torch.Tensor:
    """[P, nb * r] -> [P, r]: row p keeps the r columns of its own block."""
    rows, r = wide.size(0), wide.size(1) // n_blocks
    index = block.view(rows, 1, 1).expand(rows, 1, r)
    return wide.view(rows, n_blocks, r).gather(1, index).squeeze(1)


def _in_own_block(narrow: torch.Tensor, block: torch.Tensor, n_blocks: int) -> torch.Tensor:
    """[P, r] -> [P, nb * r], zero outside the row's own block (adjoint of _own_block)."""
    rows, r = narrow.shape
    wide = torch.zeros([rows, n_blocks, r], dtype=narrow.dtype, device=narrow.device)
    wide.scatter_(1, block.view(rows, 1, 1).expand(rows, 1, r), narrow.unsqueeze(1))
    return wide.view(rows, n_blocks * r)


def _block_major(cat: torch.Tensor, n_blocks: int) -> torch.Tensor:
    """[bs, nb * r] -> [nb * bs, r] (the layout of a LoRA table over d_feedforward)."""
    bs = cat.size(0)
    return cat.view(bs, n_blocks, -1).permute(1, 0, 2).reshape(n_blocks * bs, -1)


def _block_cat(table: torch.Tensor, n_blocks: int) -> torch.Tensor:
    """[nb * bs, r] -> [bs, nb * r]: all blocks' slices side by side."""
    bs = table.size(0) // n_blocks
    return table.view(n_blocks, bs, -1).permute(1, 0, 2).reshape(bs, -1)


def _down(a: torch.Tensor, table: torch.Tensor, want_image: bool, want_norms: bool):
    """(a @ table, split image of a | None, row norms of a | None): one pass over `a`
    (ext.lora_down) where its shapes allow, else the separate operators.  `want_norms` is asked
    for in front of a ReLU GEMM, and there the product is formed in exact fp32 (csrc/lora_side.hip:
    its error would otherwise pick the sign of pre-activations next to zero)."""
    if ext.lora_down_supported(a, table):
        ext.note_path('lora_down', 'kernel')
        if want_image or want_norms:
            return ext.lora_down(a, table, want_image=want_image, want_norms=want_norms, exact=want_norms)
        return ext.lora_down(a, table), None, None
    ext.note_path('lora_down', 'library', fallback=a.is_cuda,
                  why=lambda: 'a {} x table {}: spt_lora_down takes K % 32 == 0, 16-64 columns'.format(
                      tuple(a.shape), tuple(table.shape)))
    return (torch.matmul(a, table), ext.split_bf16(a) if want_image else None,
            ext.row_norms(a) if want_norms else None)


def _down_blocks(a: torch.Tensor, table: torch.Tensor, bk: Buckets, want_image: bool):
    """(a[p] @ table_g(p) [P, r], split image of a | None) for a per-block table [nb * bs, r] and
    rows sorted by block: one grouped pass (ext.lora_down_grouped) instead of the product with all
    blocks' tables side by side, a gather of the row's own block and a copy."""
    nb = bk.n_blocks
    tables = table.view(nb, table.size(0) // nb, table.size(1))
    if ext.lora_down_grouped_supported(a, tables):
        ext.note_path('lora_down_grouped', 'kernel')
        if want_image:
            return ext.lora_down_grouped(a, tables, bk.offsets, want_image=True)
        return ext.lora_down_grouped(a, tables, bk.offsets), None
    ext.note_path('lora_down_grouped', 'side_by_side', fallback=a.is_cuda,
                  why=lambda: 'a {} x tables {}'.format(tuple(a.shape), tuple(tables.shape)))
    wide, image, _ = _down(a, _block_cat(table, nb), want_image, False)
    return _own_block(wide, bk.block, nb).contiguous(), image


def _tn(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    from naive_gpt.layers.tuning.lora import tall_tn
    return tall_tn(a, b)


def _tn_blocks(wide: torch.Tensor, per_token: torch.Tensor, bk: Buckets) -> torch.Tensor:
    """The gradient of a per-block LoRA table [nb * bs, r]: for block g, wide[rows of g]^T .
    per_token[token of those rows] -- rows are sorted by block, so it is a grouped product
    (spt_tall_tn with the bucket offsets and the rows' token ids as the gather) instead of a
    [P, nb * r] matrix of mostly zeros times wide."""
    nb = bk.n_blocks
    if ext.tall_tn_supported(wide, per_token):
        ext.note_path('tall_tn_blocks', 'kernel')
        return ext.tall_tn(wide, per_token, gather=bk.token, offsets=bk.offsets).view(nb * wide.size(1), -1)
    ext.note_path('tall_tn_blocks', 'library', fallback=wide.is_cuda,
                  why=lambda: 'wide {} x per_token {}'.format(tuple(wide.shape), tuple(per_token.shape)))
    rows = per_token.index_select(0, bk.token_long)
    return _block_major(_tn(wide, _in_own_block(rows, bk.block, nb)), nb)


def _tn_blocks_many(pairs, bk: Buckets):
    """[_tn_blocks(wide, per_token, bk) for the pairs]: one pair of launches when they have one shape"""
    wides, narrows = [p[0] for p in pairs], [p[1] for p in pairs]
    if ext.tall_tn_batchable(wides, narrows):
        ext.note_path('tall_tn_blocks', 'kernel_batch')
        outs = ext.tall_tn_batch(wides, narrows, gather=bk.token, offsets=bk.offsets)
        return [t.view(bk.n_blocks * wides[0].size(1), -1) for t in outs]
    return [_tn_blocks(w, t, bk) for w, t in pairs]


def _router_rides(x: torch.Tensor, l1: torch.Tensor, rw: torch.Tensor, n_blocks: int) -> bool:
    """The router's logits as a second table of the x L1 pass (spt_lora_down2) and the routing from
    logits (spt_route_topk_logits): rank-16 adapter, <= 8 blocks, shapes spt_lora_down takes."""
    return (ROUTER_RIDES and x.is_cuda and l1.size(1) == 16 and n_blocks <= 8 and rw.is_contiguous()
            and rw.dtype == torch.float32 and rw.data_ptr() % 16 == 0
            and ext.lora_down_supported(x, l1) and ext.route_topk_supported(x.size(0), n_blocks))


def _route(x: torch.Tensor, rw: torch.Tensor, rb, n_blocks: int, k: int):
    """The router (sparse/feedforward.py:22-25: Linear + Sigmoid) and the bucketing of its top-k, inside
    the routed FFN's own autograd node: -> (prob [T, nb], Buckets with coeff = 2 prob
    (lora_ffn.py:96), block ids as int32 [P])."""
    prob = torch.sigmoid(torch.nn.functional.linear(x, rw, rb))
    if ext.route_topk_supported(prob.size(0), n_blocks):
        ext.note_path('route_topk', 'kernel')
        token, block, offsets, pos, token_long, block_long, coeff = ext.route_topk_coeff(prob, k, 2.0)
        return prob, Buckets(token=token, token_long=token_long, block=block_long, offsets=offsets,
                             coeff=coeff, n_blocks=n_blocks, pos=pos), block
    bk = make_buckets(prob, k, scale=2.0)
    return prob, bk, bk.block.int()


def _route_dlogit(grad_coeff, prob, bk: Buckets, block):
    """d coeff [P] -> d logit [T, nb]: the adjoint of the bucketing chained through the sigmoid"""
    nb = bk.n_blocks
    if grad_coeff.is_cuda and nb <= 8:
        return ext.route_coeff_backward(grad_coeff.contiguous(), bk.pos, block, 2.0, nb, prob=prob)
    dprob = torch.zeros_like(prob)
    dprob.view(-1).index_put_((bk.token_long * nb + bk.block,), 2.0 * grad_coeff)
    return dprob * (1.0 - prob) * prob


def _route_backward(ctx, grad_coeff, prob, bk: Buckets, block, x, rw, grad_x):
    """The router's share of the backward: d coeff [P] -> d logit [T, nb] (one launch: the adjoint of
    the bucketing chained through the sigmoid), its input gradient ADDED into `grad_x` (the FFN's
    own, same tensor: one sum inside one autograd node), and the gradients of its weight and bias.
    -> (grad_rw, grad_rb)."""
    from naive_gpt.layers.tuning.lora import tall_tn
    dlogit = _route_dlogit(grad_coeff, prob, bk, block)
    grad_x.addmm_(dlogit, rw)
    grad_rw = tall_tn(dlogit, x) if ctx.needs_input_grad[1] else None       # [nb, d]
    grad_rb = dlogit.sum(dim=0) if ctx.needs_input_grad[2] else None
    return grad_rw, grad_rb


class RoutedLoRAFFN(torch.autograd.Function):
    """y = LoRARoutedFFN(x) for frozen base weights (reference formula:
    naive_gpt/layers/tuning/lora_ffn.py:87-111), as four fused block GEMMs:

        h  = act(c (x W1_g^T + b1_g) + (x L1) R1_g^T)          spt_grouped_gemm_fused, EPI_ACT
        ys = c (h W2_g) + (h L2_g) R2^T                        spt_grouped_gemm_fused
        y  = b2 + sum over the token's rows of ys              spt_rows_combine
      backward
        ds = (c (dy W2_g^T) + (dy R2) L2_g^T) * act'(s)        EPI_DACT, + the two row dots
        dx = sum over the token's rows of c (ds W1_g) + (ds R1_g) L1^T

    Saved for backward: h (and the pre-activation only when act is not ReLU), the two
    [*, r] LoRA intermediates -- against ~8 [P, d] tensors of the op-by-op composition.
    The small [*, r] products and the LoRA table gradients are single calls of libspt_hip too
    (spt_lora_down[_grouped], spt_tall_tn).
    """

    @staticmethod
    def forward(ctx, x, rw, rb, l1, r1, l2, r2, w1, b1, w2, b2, nb: int, top_k: int, act: int,
                origin_input=None, origin_module=None, origin_lazy=None):
        d_ff, d = w1.shape
        x = x.contiguous()
        bs, rank = d_ff // nb, l1.size(1)
        relu = act == ext.ACT_RELU
        imgs = _images_usable(x, w1, w2, d, bs)
        if _router_rides(x, l1, rw, nb):
            # ONE pass over x: u = x L1, the router's logits x W_r^T (a second table of the same
            # launch, exact fp32: the top-k must not depend on a split's 2^-16), x's image and row
            # norms; the sigmoid is formed inside the routing launch.  (As torch operators: a library
            # GEMM with 4 output columns and a sigmoid pass, ~20 us per layer.)
            # The same launch ranks its 16 rows' logits + bias and leaves the per-group selection counts:
            # the routing launch sums those instead of ranking every token in every workgroup.
            ext.note_path('router', 'rides_lora_down')
            counts = None
            if ROUTER_COUNTS:
                ext.note_path('router_counts', 'ride_lora_down')
                pack, x_img, x_norm, counts = ext.lora_down(
                    x, l1, want_image=imgs, want_norms=relu, block_major=True, exact=True, table2=rw,
                    route=(rb, top_k))
            else:
                ext.note_path('router_counts', 'recounted')
                pack = ext.lora_down(x, l1, want_image=imgs, want_norms=relu, block_major=True, exact=True,
                                     table2=rw)
                pack, x_img, x_norm = pack if isinstance(pack, tuple) else (pack, None, None)
            u = pack[0]
            prob, token, block, offsets, pos, token_long, block_long, coeff = \
                ext.route_topk_logits(pack[1], rb, nb, top_k, 2.0, counts=counts)
            ext.note_path('route_topk', 'kernel')
            bk = Buckets(token=token, token_long=token_long, block=block_long, offsets=offsets,
                         coeff=coeff, n_blocks=nb, pos=pos)
        else:
            ext.note_path('router', 'library', fallback=x.is_cuda,
                          why=lambda: 'x {} L1 {} router {}'.format(tuple(x.shape), tuple(l1.shape), tuple(rw.shape)))
            prob, bk, block = _route(x, rw, rb, nb, top_k)
            # Both block GEMMs run from pre-split images: the weights' are made from the frozen
            # parameters, x's and h's cost one pass each -- the pass that also forms the LoRA down
            # product and, in front of a ReLU, the row norms the kernel wants (include/spt_hip.h:
            # a_norm): ext.lora_down, one read of the activation for all three.
            u, x_img, x_norm = _down(x, l1, imgs, relu)                      # [T, r]
        coeff = bk.coeff
        rows = bk.token.numel()
        h, s = ext.grouped_gemm_fused(
            x, w1, bk.offsets, nb, n=bs, k=d, w_group_stride=bs * d, w_ldn=d, w_ldk=1,
            n_rows=rows, gather=bk.token, bias=b1, rowscale=coeff,
            a2=u, gather2=bk.token, b2=r1, b2_group_stride=bs * rank,
            epilogue=ext.EPI_ACT, activation=act, keep_preact=not relu,
            a_image=x_img, w_image=_w_image(w1, imgs),
            a_norm=x_norm, w_norm=ext.weight_row_norms(w1) if relu else None)
        # (h has ONE reader: no image of it -- the GEMM splits its fp32 rows itself ("A32", +11 us)
        # and the down product runs without the image store (-20 us))
        z, h_img = _down_blocks(h, l2, bk, imgs and not H_A32)               # [P, r]
        ys = ext.grouped_gemm_fused(
            h, w2, bk.offsets, nb, n=d, k=bs, w_group_stride=bs, w_ldn=d_ff, w_ldk=1,
            n_rows=rows, rowscale=coeff, a2=z, b2=r2, b2_group_stride=0,
            a_image=h_img, w_image=_w_image(w2, imgs))
        y = ext.rows_combine(ys, bk.pos, bias=b2)
        ctx.bk, ctx.act = bk, act
        # x is a norm output the block can recompute: keep its origin instead (tuning/recompute.py)
        ctx.origin_module = origin_module
        # (recompute.lazy: the backward reads x in two table gradients alone, and they can form it from
        # the norm's input as they load it)
        ctx.lazy = origin_module is not None and origin_lazy is not None
        ctx.save_for_backward(x if origin_module is None else origin_input, coeff, u, h, s, z,
                              l1, r1, l2, r2, w1, w2, prob, block, rw, *(origin_lazy.norm if ctx.lazy else ()))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, coeff, u, h, s, z, l1, r1, l2, r2, w1, w2, prob, block, rw = ctx.saved_tensors[:15]
        norm = tuple(ctx.saved_tensors[15:19]) if ctx.lazy else None
        if ctx.origin_module is not None:
            # x: the norm's INPUT from here on; its output is formed on load or recomputed below
            x = x.view(-1, w1.size(1))
        bk, act = ctx.bk, ctx.act
        nb = bk.n_blocks
        d_ff, d = w1.shape
        bs, rank, rows = d_ff // nb, l1.size(1), bk.token.numel()
        dy = dy.contiguous()
        imgs = _images_usable(dy, w1, w2, d, bs)
        dzt, dy_img, _ = _down(dy, r2, imgs, False)                          # [T, r]
        ds, dot_main, dot_act = ext.grouped_gemm_fused(
            dy, w2, bk.offsets, nb, n=bs, k=d, w_group_stride=bs, w_ldn=1, w_ldk=d_ff,
            n_rows=rows, gather=bk.token, rowscale=coeff,
            a2=dzt, gather2=bk.token, b2=l2, b2_group_stride=bs * rank,
            epilogue=ext.EPI_DACT, activation=act, h_in=h, s_in=s,
            a_image=dy_img, w_image=_w_image(w2, imgs), raw_dots=True)
        du, _ = _down_blocks(ds, r1, bk, False)                              # [P, r]
        # d/dc = <dy W2_g^T, h> + <ds, x W1_g^T + b1_g>.  The kernel's dot_main = <v, h> with
        # v = c (dy W2_g^T) + dzt L2_g^T (the value before act'), dot_act = <ds, s> with
        # s = c (x W1^T + b1) + u R1^T; the LoRA parts of both are [*, r] dots:
        # <dzt L2_g^T, h> = <dzt, z> and <ds, u R1_g^T> = <du, u>
        # (dot_main + dot_act - <du, u[token]> - <dzt[token], z>) / _floor(coeff), one launch
        # LoRA tables (before the last GEMM: ds [P, bs] is released as soon as that has read it --
        # the step's peak memory is here, with h, ds, dxs and grad_x alive)
        # (two pairs of equal shape: one pair of launches each)
        from naive_gpt.layers.tuning.lora import tall_tn_many
        router_rides = du.is_cuda and nb <= 8 and d % 4 == 0
        dlogit = grad_rw = None
        if router_rides and ROUTER_BACKWARD_FUSED and rank == 16:
            # one launch: the coefficient gradient stays in registers on its way to d logit, and the
            # rows it reads of du and z are the ones the two [T, r] sums need
            ext.note_path('router_backward', 'one_launch')
            dlogit, du_tok, z_tok, _ = ext.ffn_coeff_grad(dot_main, dot_act, du, u, dzt, z, bk.token, coeff,
                                                          COEFF_FLOOR, router=(bk.pos, block, prob, 2.0))
        else:
            ext.note_path('router_backward', 'separate')
            grad_coeff = ext.ffn_coeff_grad(dot_main, dot_act, du, u, dzt, z, bk.token, coeff, COEFF_FLOOR)
            du_tok = ext.rows_combine(du, bk.pos)                            # [T, r]: du[pos].sum(1)
            z_tok = ext.rows_combine(z, bk.pos)
            if router_rides:
                dlogit = ext.route_coeff_backward(grad_coeff.contiguous(), bk.pos, block, 2.0, nb, prob=prob)
        if ctx.origin_module is not None:
            # The two readers of x are the gradients of L1 (x^T du) and of the router's weight (dlogit^T x).
            # From the norm's input, statistics and parameters one pass forms x on load and feeds both
            # (ext.tall_tn_batch: norms, narrows2); anything else recomputes the tensor as before.
            want_rw = router_rides and ctx.needs_input_grad[1]
            if norm is not None and router_rides and x.size(0) >= 512 \
                    and ext.tall_tn_batchable([x, dy], [du_tok, z_tok]) \
                    and ext.tall_tn_norm_supported(x, du_tok, norm, dlogit if want_rw else None):
                ext.note_path('norm_output', 'on_load')
                ext.note_path('tall_tn', 'kernel_batch')
                outs = ext.tall_tn_batch([x, dy], [du_tok, z_tok], norms=[norm, None],
                                         narrows2=[dlogit, None] if want_rw else None, transposed2=True)
                if want_rw:
                    outs[0], grad_rw = outs[0][0], outs[0][1][0]                    # [nb, d]
                grad_l1, grad_r2 = outs[0][0], outs[1][0]
                x = None                                                             # (not read again)
            else:
                ext.note_path('norm_output', 'recomputed', fallback=norm is not None,
                              why=lambda: 'routed FFN: x {} rank {} blocks {}'.format(tuple(x.shape), rank, nb))
                x = recompute.output(ctx.origin_module, x).view(-1, w1.size(1))
        if x is not None:
            grad_l1, grad_r2 = tall_tn_many([(x, du_tok), (dy, z_tok)])
        del z_tok
        grad_r1, grad_l2 = _tn_blocks_many([(ds, u), (h, dzt)], bk)
        del dot_main, dot_act, du_tok, dzt
        dxs = ext.grouped_gemm_fused(
            ds, w1, bk.offsets, nb, n=d, k=bs, w_group_stride=bs * d, w_ldn=1, w_ldk=d,
            n_rows=rows, rowscale=coeff, a2=du, b2=l1, b2_group_stride=0, w_image=_w_image(w1, False))
        del ds, du
        if router_rides:
            # the router's share d logit . W_r of grad_x inside the un-bucketing pass
            grad_x = ext.rows_combine(dxs, bk.pos, side=dlogit, side_weight=rw.contiguous())
            del dxs
            if x is not None and ctx.needs_input_grad[1]:
                from naive_gpt.layers.tuning.lora import tall_tn
                grad_rw = tall_tn(dlogit, x)                                        # [nb, d]
            grad_rb = dlogit.sum(dim=0) if ctx.needs_input_grad[2] else None
        else:
            grad_x = ext.rows_combine(dxs, bk.pos)
            del dxs
            grad_rw, grad_rb = _route_backward(ctx, grad_coeff, prob, bk, block, x, rw, grad_x)
        return (grad_x, grad_rw, grad_rb, grad_l1, grad_r1, grad_l2, grad_r2,
                None, None, None, None, None, None, None, None, None, None)


def routed_lora_ffn(x, rw, rb, l1, r1, l2, r2, w1, b1, w2, b2, n_blocks: int, top_k: int, act: int,
                    origin=None):
    """`rw`, `rb`: the router's Linear (its Sigmoid, the top-k and the bucketing run inside)."""
    if origin is None:
        return RoutedLoRAFFN.apply(x, rw, rb, l1, r1, l2, r2, w1, b1, w2, b2, n_blocks, top_k, act)
    return RoutedLoRAFFN.apply(x, rw, rb, l1, r1, l2, r2, w1, b1, w2, b2, n_blocks, top_k, act,
                               origin.input, origin.module, recompute.lazy(origin))


def _images_usable(a: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, d: int, bs: int) -> bool:
    """The image path of the grouped GEMM: contraction lengths and block offsets in whole
    32-element blocks (ext.grouped_gemm_fused falls back to the fp32 operands otherwise)."""
    return d % 32 == 0 and bs % 32 == 0 and a.is_contiguous()


def fused_usable(rank: int) -> bool:
    return rank % 4 == 0 and 0 < rank <= 32


class RoutedLoRALLaMAFFN(torch.autograd.Function):
    """y = LoRARoutedLLaMaFFN(x) for frozen base weights (reference formula:
    naive_gpt/layers/tuning/lora_ffn.py:196-222), with c the router coefficient of a row:

        g  = c (x G_g^T) + (x Lg) Rg_g^T,   sd = c (x S_g^T) + (x Ls) Rs_g^T     two fused GEMMs
        h  = act(g) * sd                                                        (torch)
        ys = c (h D_g) + (h Ld_g) Rd^T;   y = sum over the token's rows of ys   fused GEMM + combine

    Same building blocks as RoutedLoRAFFN (LoRA side products as the GEMMs' K extension, token
    gather and rowscale inside the kernel, rows_combine instead of index_add); the gating product
    and the activation derivative stay elementwise torch ops.  The coefficient gradient uses
    <A, h> = (<c A + E, h> - <E, h>) / c with <E, h> = <dy Rd, h Ld_g> (both [*, r]), and the same
    identity for the two up projections."""

    @staticmethod
    def forward(ctx, x, rw, rb, lg, rg, ls, rs, ld, rd, wg, ws, wd, nb: int, top_k: int, activation,
                origin_input=None, origin_module=None, origin_lazy=None):
        d_ff, d = wg.shape
        x = x.contiguous()
        prob, bk, block = _route(x, rw, rb, nb, top_k)
        coeff = bk.coeff
        bs, rank, rows = d_ff // nb, lg.size(1), bk.token.numel()
        imgs = _images_usable(x, wg, wd, d, bs)
        # one pass over x: both adapters' down products and the image both up projections read
        table = torch.cat([lg, ls], dim=1)
        if rank == 16 and ext.lora_down_supported(x, table):
            ext.note_path('lora_down', 'kernel')
            ugs, x_image, _ = ext.lora_down(x, table, want_image=True, block_major=True) if imgs \
                else (ext.lora_down(x, table, block_major=True), None, None)
            ug, us = ugs[0], ugs[1]                                               # [T, r]
        else:
            ext.note_path('lora_down', 'library', fallback=True,
                          why=lambda: 'gated FFN: x {} x [lg | ls] {}'.format(tuple(x.shape), tuple(table.shape)))
            ug, us = torch.matmul(x, lg), torch.matmul(x, ls)
            x_image = ext.split_bf16(x) if imgs else None

        def up(w, u, r_table):
            return ext.grouped_gemm_fused(
                x, w, bk.offsets, nb, n=bs, k=d, w_group_stride=bs * d, w_ldn=d, w_ldk=1,
                n_rows=rows, gather=bk.token, rowscale=coeff, a2=u, gather2=bk.token,
                b2=r_table, b2_group_stride=bs * rank,
                a_image=x_image, w_image=_w_image(w, imgs))

        g, sd = up(wg, ug, rg), up(ws, us, rs)
        silu = isinstance(activation, torch.nn.SiLU) and ext.swiglu_supported(g, sd)
        ext.note_path('swiglu', 'kernel' if silu else 'torch', fallback=not silu,
                      why=lambda: 'activation {} on {}'.format(type(activation).__name__, tuple(g.shape)))
        h = ext.swiglu_forward(g, sd) if silu else activation(g) * sd
        zw, h_img, _ = _down(h, _block_cat(ld, nb), imgs and not H_A32, False)
        z = _own_block(zw, bk.block, nb).contiguous()
        ys = ext.grouped_gemm_fused(
            h, wd, bk.offsets, nb, n=d, k=bs, w_group_stride=bs, w_ldn=d_ff, w_ldk=1,
            n_rows=rows, rowscale=coeff, a2=z, b2=rd, b2_group_stride=0,
            a_image=h_img, w_image=_w_image(wd, imgs))
        del x_image, h_img
        y = ext.rows_combine(ys, bk.pos)
        ctx.bk, ctx.activation = bk, activation
        ctx.origin_module = origin_module
        ctx.lazy = origin_module is not None and origin_lazy is not None      # (as RoutedLoRAFFN)
        ctx.save_for_backward(x if origin_module is None else origin_input, coeff, ug, us, g, sd,
                              h, z, lg, rg, ls, rs, ld, rd, wg, ws, wd, prob, block, rw,
                              *(origin_lazy.norm if ctx.lazy else ()))
        return y

    @staticmethod
    def backward(ctx, dy):
        (x, coeff, ug, us, g, sd, h, z, lg, rg, ls, rs, ld, rd, wg, ws, wd, prob, block,
         rw) = ctx.saved_tensors[:20]
        norm = tuple(ctx.saved_tensors[20:24]) if ctx.lazy else None
        if ctx.origin_module is not None:
            # x: the norm's INPUT from here on; its output is formed on load or recomputed below
            x = x.view(-1, wg.size(1))
        bk, activation = ctx.bk, ctx.activation
        nb = bk.n_blocks
        d_ff, d = wg.shape
        bs, rank, rows = d_ff // nb, lg.size(1), bk.token.numel()
        dy = dy.contiguous()
        imgs = _images_usable(dy, wg, wd, d, bs)
        dzt, dy_img, _ = _down(dy, rd, imgs, False)                           # [T, r]
        dz_rows = dzt.index_select(0, bk.token_long)
        dh = ext.grouped_gemm_fused(
            dy, wd, bk.offsets, nb, n=bs, k=d, w_group_stride=bs, w_ldn=1, w_ldk=d_ff,
            n_rows=rows, gather=bk.token, rowscale=coeff, a2=dzt, gather2=bk.token, b2=ld,
            b2_group_stride=bs * rank,
            a_image=dy_img, w_image=_w_image(wd, imgs))
        del dy_img
        silu = isinstance(activation, torch.nn.SiLU) and ext.swiglu_supported(g, sd)
        if silu:
            # through h = silu(g) * sd, and the row dots of the coefficient gradient, in one pass
            dg, dsd, dot_h, dot_g, dot_s = ext.swiglu_backward(dh, g, sd)
            del dh
        else:
            dot_h = (dh * h).sum(dim=-1)
            dot_g = dot_s = None
            with torch.enable_grad():
                g_ = g.detach().requires_grad_(True)
                ag = activation(g_)
                dg, = torch.autograd.grad(ag, g_, dh * sd)
            dsd = dh * ag.detach()
            del dh, ag, g_                   # [P, bs] each: the step's peak memory is in here
        grad_coeff = (dot_h - (dz_rows * z).sum(dim=-1)) / _floor(coeff)

        def down(dpre, pre, w, u, l_table, r_table, dot_pre=None, into=None):
            """-> (dx rows [P, d], d coefficient [P], du per token [T, r], grad of the `right` table)"""
            du, _ = _down_blocks(dpre, r_table, bk, False)
            u_rows = u.index_select(0, bk.token_long)
            if dot_pre is None:
                dot_pre = (dpre * pre).sum(dim=-1)
            dc = (dot_pre - (du * u_rows).sum(dim=-1)) / _floor(coeff)
            # (`into`: the other projection's dx rows -- this product is ADDED to them by the GEMM)
            dxs = ext.grouped_gemm_fused(
                dpre, w, bk.offsets, nb, n=d, k=bs, w_group_stride=bs * d, w_ldn=1, w_ldk=d,
                n_rows=rows, rowscale=coeff, a2=du, b2=l_table, b2_group_stride=0,
                out=into, accumulate=into is not None, w_image=_w_image(w, False))
            grad_r = _tn_blocks(dpre, u, bk)
            return dxs, dc, ext.rows_combine(du, bk.pos), grad_r

        dxs_g, dc_g, du_g, grad_rg = down(dg, g, wg, ug, lg, rg, dot_g)
        del dg
        dxs_g, dc_s, du_s, grad_rs = down(dsd, sd, ws, us, ls, rs, dot_s, into=dxs_g)
        del dsd
        grad_x = ext.rows_combine(dxs_g, bk.pos)
        del dxs_g
        grad_coeff = grad_coeff + dc_g + dc_s
        dlogit = _route_dlogit(grad_coeff, prob, bk, block)
        grad_x.addmm_(dlogit, rw)                                            # (as _route_backward)
        # The readers of x: the two `left` gradients and the router's weight gradient.  From the norm's
        # input, statistics and parameters one pair of launches forms x on load for all three
        # (ext.tall_tn_batch: norms, narrows2); anything else recomputes the tensor as before.
        want_rw = ctx.needs_input_grad[1]
        grad_rw = None
        if ctx.origin_module is not None:
            if norm is not None and x.size(0) >= 512 and ext.tall_tn_batchable([x, x], [du_g, du_s]) \
                    and ext.tall_tn_norm_supported(x, du_g, norm, dlogit if want_rw else None):
                ext.note_path('norm_output', 'on_load')
                ext.note_path('tall_tn', 'kernel_batch')
                outs = ext.tall_tn_batch([x, x], [du_g, du_s], norms=[norm, norm],
                                         narrows2=[dlogit, None] if want_rw else None, transposed2=True)
                if want_rw:
                    outs[0], grad_rw = outs[0][0], outs[0][1][0]                    # [nb, d]
                grad_lg, grad_ls = outs[0][0], outs[1][0]
                x = None
            else:
                ext.note_path('norm_output', 'recomputed', fallback=norm is not None,
                              why=lambda: 'gated routed FFN: x {} rank {} blocks {}'.format(tuple(x.shape), rank, nb))
                x = recompute.output(ctx.origin_module, x).view(-1, wg.size(1))
        if x is not None:
            grad_lg, grad_ls = _tn(x, du_g), _tn(x, du_s)
            grad_rw = _tn(dlogit, x) if want_rw else None                        # [nb, d]
        grad_rb = dlogit.sum(dim=0) if ctx.needs_input_grad[2] else None
        grad_ld = _tn_blocks(h, dzt, bk)
        grad_rd = _tn(dy, ext.rows_combine(z, bk.pos))
        return (grad_x, grad_rw, grad_rb, grad_lg, grad_rg, grad_ls, grad_rs, grad_ld, grad_rd,
                None, None, None, None, None, None, None, None, None)


def routed_lora_llama_ffn(x, rw, rb, lg, rg, ls, rs, ld, rd, wg, ws, wd, n_blocks: int, top_k: int,
                          activation, origin=None):
    if origin is None:
        return RoutedLoRALLaMAFFN.apply(x, rw, rb, lg, rg, ls, rs, ld, rd, wg, ws, wd, n_blocks, top_k,
                                        activation)
    return RoutedLoRALLaMAFFN.apply(x, rw, rb, lg, rg, ls, rs, ld, rd, wg, ws, wd, n_blocks, top_k,
                                    activation, origin.input, origin.module, recompute.lazy(origin))


# ---------------------------------------------------------------- the LoRA routed FFNs on bf16 storage
# The fused bf16 path of LoRARoutedFFN / LoRARoutedLLaMaFFN (tuning/lora_ffn.py): opt-in until it is measured
# as the default; read at call time (tests flip it).
LORA_BF16 = os.environ.get('SPT_ROUTED_LORA_BF16', '0') != '0'


def lora_bf16_unusable(x: torch.Tensor, rank: int, plain_router: bool, d: int, bs: int, frozen, trained):
    """None when the fused bf16 LoRA path takes these operands, else the reason it does not: the flag,
    bf16 CUDA activations, frozen contiguous bf16 base weights (`frozen`, None entries skipped), bf16
    contiguous LoRA tables and router (`trained`), d and the block size multiples of 64, a rank the
    K extension takes and a plain Linear + Sigmoid router."""
    if not LORA_BF16:
        return 'SPT_ROUTED_LORA_BF16 is off'
    if not x.is_cuda or x.dtype != torch.bfloat16:
        return 'x {} {}: bf16 CUDA activations only'.format(tuple(x.shape), x.dtype)
    for w in frozen:
        if w is None:
            continue
        if w.requires_grad or not w.is_cuda or not w.is_contiguous() or w.dtype != torch.bfloat16:
            return 'base weight {} {}: frozen contiguous bf16 CUDA weights only'.format(tuple(w.shape), w.dtype)
    for t in trained:
        if not t.is_cuda or not t.is_contiguous() or t.dtype != torch.bfloat16:
            return 'LoRA table / router {} {}: contiguous bf16 CUDA tensors only'.format(tuple(t.shape), t.dtype)
    if not bf16_shapes(d, bs):
        return 'd {} block {}: multiples of 64 only'.format(d, bs)
    if not fused_usable(rank):
        return 'rank {}: rank % 4 == 0 and rank <= 32 only'.format(rank)
    if not plain_router:
        return 'router: Linear + Sigmoid only'
    return None


def lora_bf16_usable(x: torch.Tensor, rank: int, plain_router: bool, d: int, bs: int, frozen, trained) -> bool:
    return lora_bf16_unusable(x, rank, plain_router, d, bs, frozen, trained) is None


def _route_bf16(x: torch.Tensor, rw: torch.Tensor, rb: torch.Tensor, n_blocks: int, k: int):
    """The router as the bf16 module computes it (Linear + Sigmoid in bf16), its probabilities widened to
    fp32 for the bucketing: -> (prob fp32 [T, nb], Buckets with coeff = 2 prob, block ids int32 [P])."""
    prob = torch.sigmoid(torch.nn.functional.linear(x, rw, rb)).float()
    if ext.route_topk_supported(prob.size(0), n_blocks):
        ext.note_path('route_topk', 'kernel')
        token, block, offsets, pos, token_long, block_long, coeff = ext.route_topk_coeff(prob, k, 2.0)
        return prob, Buckets(token=token, token_long=token_long, block=block_long, offsets=offsets,
                             coeff=coeff, n_blocks=n_blocks, pos=pos), block
    bk = make_buckets(prob, k, scale=2.0)
    return prob, bk, bk.block.int()


def _route_backward_bf16(ctx, grad_coeff, prob, bk: Buckets, block, x, rw, grad_x):
    """_route_backward for the bf16 router: d logit in fp32, its share of the input gradient added to the
    bf16 `grad_x` (a second rounding of grad_x), the router's gradients rounded once to its dtype.
    -> (grad_x, grad_rw, grad_rb)."""
    nb = bk.n_blocks
    if grad_coeff.is_cuda and nb <= 8:
        dlogit = ext.route_coeff_backward(grad_coeff.contiguous(), bk.pos, block, 2.0, nb, prob=prob)
    else:
        dprob = torch.zeros_like(prob)
        dprob.view(-1).index_put_((bk.token_long * nb + bk.block,), 2.0 * grad_coeff)
        dlogit = dprob * (1.0 - prob) * prob
    grad_x = torch.addmm(grad_x.float(), dlogit, rw.float()).to(grad_x.dtype)
    grad_rw = torch.matmul(dlogit.t(), x.float()).to(rw.dtype) if ctx.needs_input_grad[1] else None
    grad_rb = dlogit.sum(dim=0).to(rw.dtype) if ctx.needs_input_grad[2] else None
    return grad_x, grad_rw, grad_rb


def _tables(table: torch.Tensor, nb: int) -> torch.Tensor:
    """[nb * bs, r] -> [nb, bs, r]"""
    return table.view(nb, table.size(0) // nb, table.size(1))


class RoutedLoRAFFNBf16(torch.autograd.Function):
    """RoutedLoRAFFN on bf16 storage (x, base weights, LoRA tables, router, h, s and the gradients bf16; the
    rank-r intermediates u, z, dzt, du fp32):

        u  = x L1                                              spt_lora_down_bf16
        h  = act(c (x W1_g^T + b1_g) + u R1_g^T)               spt_grouped_gemm_bf16_ext, EPI_ACT
        z  = h L2_g;  ys = c (h W2_g) + z R2^T                 spt_lora_down_grouped_bf16, _bf16_ext
        y  = b2 + sum over the token's rows of ys              spt_rows_combine_bf16
      backward
        dzt = dy R2;  ds = (c (dy W2_g^T) + dzt L2_g^T) * act'(s), + the row dots     EPI_DACT
        du = ds R1_g;  dx = sum over the token's rows of c (ds W1_g) + du L1^T
        LoRA table gradients                                   spt_tall_tn_bf16

    The router is the module's bf16 Linear + Sigmoid; its probabilities are widened to fp32 for the
    bucketing and the coefficient gradient; d logit . W_r is added to dx by torch."""

    @staticmethod
    def forward(ctx, x, rw, rb, l1, r1, l2, r2, w1, b1, w2, b2, nb: int, top_k: int, act: int,
                origin_input=None, origin_module=None):
        d_ff, d = w1.shape
        x = x.contiguous()
        bs, rank = d_ff // nb, l1.size(1)
        relu = act == ext.ACT_RELU
        prob, bk, block = _route_bf16(x, rw, rb, nb, top_k)
        coeff, rows = bk.coeff, bk.token.numel()
        u = ext.lora_down_bf16(x, l1)                                        # [T, r] fp32
        h, s = ext.grouped_gemm_bf16_ext(
            x, w1, bk.offsets, nb, n=bs, k=d, w_group_stride=bs * d, w_ldn=d, w_ldk=1, n_rows=rows,
            gather=bk.token, bias=b1.view(nb, bs), rowscale=coeff, a2=u, gather2=bk.token, b2=r1,
            b2_group_stride=bs * rank, epilogue=ext.EPI_ACT, activation=act, keep_preact=not relu)
        z = ext.lora_down_grouped_bf16(h, _tables(l2, nb), bk.offsets)       # [P, r] fp32
        ys = ext.grouped_gemm_bf16_ext(
            h, w2, bk.offsets, nb, n=d, k=bs, w_group_stride=bs, w_ldn=d_ff, w_ldk=1, n_rows=rows,
            rowscale=coeff, a2=z, b2=r2, b2_group_stride=0)
        y = ext.rows_combine(ys, bk.pos, bias=b2)
        ctx.bk, ctx.act = bk, act
        ctx.origin_module = origin_module
        ctx.save_for_backward(x if origin_module is None else origin_input, coeff, u, h, s, z,
                              l1, r1, l2, r2, w1, w2, prob, block, rw)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, coeff, u, h, s, z, l1, r1, l2, r2, w1, w2, prob, block, rw = ctx.saved_tensors
        if ctx.origin_module is not None:
            x = recompute.output(ctx.origin_module, x).view(-1, w1.size(1))
        bk, act = ctx.bk, ctx.act
        nb = bk.n_blocks
        d_ff, d = w1.shape
        bs, rank, rows = d_ff // nb, l1.size(1), bk.token.numel()
        dy = dy.contiguous()
        dzt = ext.lora_down_bf16(dy, r2)                                     # [T, r] fp32
        ds, dot_main, dot_act = ext.grouped_gemm_bf16_ext(
            dy, w2, bk.offsets, nb, n=bs, k=d, w_group_stride=bs, w_ldn=1, w_ldk=d_ff, n_rows=rows,
            gather=bk.token, rowscale=coeff, a2=dzt, gather2=bk.token, b2=l2, b2_group_stride=bs * rank,
            epilogue=ext.EPI_DACT, activation=act, h_in=h, s_in=s, want_dots=True)
        du = ext.lora_down_grouped_bf16(ds, _tables(r1, nb), bk.offsets)     # [P, r] fp32
        # (dot_main + dot_act - <du, u[token]> - <dzt[token], z>) / c: RoutedLoRAFFN.backward
        grad_coeff = ext.ffn_coeff_grad(dot_main, dot_act, du, u, dzt, z, bk.token, coeff, COEFF_FLOOR)
        del dot_main, dot_act
        grad_l1 = ext.tall_tn_bf16(x, ext.rows_combine(du, bk.pos)).view(d, rank)
        grad_r2 = ext.tall_tn_bf16(dy, ext.rows_combine(z, bk.pos)).view(d, rank)
        grad_r1 = ext.tall_tn_bf16(ds, u, gather=bk.token, offsets=bk.offsets).view(d_ff, rank)
        grad_l2 = ext.tall_tn_bf16(h, dzt, gather=bk.token, offsets=bk.offsets).view(d_ff, rank)
        dxs = ext.grouped_gemm_bf16_ext(
            ds, w1, bk.offsets, nb, n=d, k=bs, w_group_stride=bs * d, w_ldn=1, w_ldk=d, n_rows=rows,
            rowscale=coeff, a2=du, b2=l1, b2_group_stride=0)
        del ds, du
        grad_x = ext.rows_combine(dxs, bk.pos)
        del dxs
        grad_x, grad_rw, grad_rb = _route_backward_bf16(ctx, grad_coeff, prob, bk, block, x, rw, grad_x)
        return (grad_x, grad_rw, grad_rb, grad_l1, grad_r1, grad_l2, grad_r2,
                None, None, None, None, None, None, None, None, None)


def routed_lora_ffn_bf16(x, rw, rb, l1, r1, l2, r2, w1, b1, w2, b2, n_blocks: int, top_k: int, act: int,
                         origin=None):
    if origin is None:
        return RoutedLoRAFFNBf16.apply(x, rw, rb, l1, r1, l2, r2, w1, b1, w2, b2, n_blocks, top_k, act)
    return RoutedLoRAFFNBf16.apply(x, rw, rb, l1, r1, l2, r2, w1, b1, w2, b2, n_blocks, top_k, act,
                                   origin.input, origin.module)


class RoutedLoRALLaMAFFNBf16(torch.autograd.Function):
    """RoutedLoRALLaMAFFN on bf16 storage (see RoutedLoRAFFNBf16; ug, us, z, dzt and the du's fp32):

        g  = c (x G_g^T) + ug Rg_g^T,  sd = c (x S_g^T) + us Rs_g^T     two spt_grouped_gemm_bf16_ext
        h  = silu(g) * sd                                               spt_swiglu_forward_bf16
        ys = c (h D_g) + (h Ld_g) Rd^T;  y = sum over the token's rows of ys
      backward: dh through the same GEMM, spt_swiglu_backward_dots_bf16 for dg, dsd and the row dots of
      the coefficient gradient, the two dX products accumulated into one bf16 buffer."""

    @staticmethod
    def forward(ctx, x, rw, rb, lg, rg, ls, rs, ld, rd, wg, ws, wd, nb: int, top_k: int, activation,
                origin_input=None, origin_module=None):
        d_ff, d = wg.shape
        x = x.contiguous()
        prob, bk, block = _route_bf16(x, rw, rb, nb, top_k)
        coeff = bk.coeff
        bs, rank, rows = d_ff // nb, lg.size(1), bk.token.numel()
        # one pass over x for both adapters: [T, 2 r], ug | us side by side
        ugs = ext.lora_down_bf16(x, torch.cat([lg, ls], dim=1))
        ug, us = ugs[:, :rank], ugs[:, rank:]

        def up(w, u, r_table):
            return ext.grouped_gemm_bf16_ext(
                x, w, bk.offsets, nb, n=bs, k=d, w_group_stride=bs * d, w_ldn=d, w_ldk=1, n_rows=rows,
                gather=bk.token, rowscale=coeff, a2=u, gather2=bk.token, b2=r_table, b2_group_stride=bs * rank)

        g, sd = up(wg, ug, rg), up(ws, us, rs)
        silu = isinstance(activation, torch.nn.SiLU) and ext.swiglu_bf16_supported(g, sd)
        ext.note_path('swiglu', 'kernel_bf16' if silu else 'torch', fallback=not silu,
                      why=lambda: 'activation {} on {}'.format(type(activation).__name__, tuple(g.shape)))
        h = ext.swiglu_forward_bf16(g, sd) if silu else activation(g) * sd
        z = ext.lora_down_grouped_bf16(h, _tables(ld, nb), bk.offsets)       # [P, r] fp32
        ys = ext.grouped_gemm_bf16_ext(
            h, wd, bk.offsets, nb, n=d, k=bs, w_group_stride=bs, w_ldn=d_ff, w_ldk=1, n_rows=rows,
            rowscale=coeff, a2=z, b2=rd, b2_group_stride=0)
        y = ext.rows_combine(ys, bk.pos)
        ctx.bk, ctx.activation, ctx.silu = bk, activation, silu
        ctx.origin_module = origin_module
        ctx.save_for_backward(x if origin_module is None else origin_input, coeff, ugs, g, sd, h, z,
                              lg, rg, ls, rs, ld, rd, wg, ws, wd, prob, block, rw)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x, coeff, ugs, g, sd, h, z, lg, rg, ls, rs, ld, rd, wg, ws, wd, prob, block,
         rw) = ctx.saved_tensors
        if ctx.origin_module is not None:
            x = recompute.output(ctx.origin_module, x).view(-1, wg.size(1))
        bk, activation = ctx.bk, ctx.activation
        nb = bk.n_blocks
        d_ff, d = wg.shape
        bs, rank, rows = d_ff // nb, lg.size(1), bk.token.numel()
        ug, us = ugs[:, :rank], ugs[:, rank:]
        dy = dy.contiguous()
        dzt = ext.lora_down_bf16(dy, rd)                                     # [T, r] fp32
        dh = ext.grouped_gemm_bf16_ext(
            dy, wd, bk.offsets, nb, n=bs, k=d, w_group_stride=bs, w_ldn=1, w_ldk=d_ff, n_rows=rows,
            gather=bk.token, rowscale=coeff, a2=dzt, gather2=bk.token, b2=ld, b2_group_stride=bs * rank)
        if ctx.silu:
            dg, dsd, dot_h, dot_g, dot_s = ext.swiglu_backward_dots_bf16(dh, g, sd)
        else:
            with torch.enable_grad():
                g_ = g.detach().requires_grad_(True)
                ag = activation(g_)
                dg, = torch.autograd.grad(ag, g_, dh * sd)
            dsd = dh * ag.detach()
            dot_h = (dh.float() * h.float()).sum(dim=-1)
            dot_g = (dg.float() * g.float()).sum(dim=-1)
            dot_s = (dsd.float() * sd.float()).sum(dim=-1)
            del ag, g_
        del dh
        dz_rows = dzt.index_select(0, bk.token_long)
        grad_coeff = (dot_h - (dz_rows * z).sum(dim=-1)) / _floor(coeff)

        def down(dpre, w, u, l_table, r_table, dot_pre, into=None):
            """-> (dx rows [P, d] bf16, d coefficient [P], grad of the two LoRA tables)"""
            du = ext.lora_down_grouped_bf16(dpre, _tables(r_table, nb), bk.offsets)
            dc = (dot_pre - (du * u.index_select(0, bk.token_long)).sum(dim=-1)) / _floor(coeff)
            dxs = ext.grouped_gemm_bf16_ext(
                dpre, w, bk.offsets, nb, n=d, k=bs, w_group_stride=bs * d, w_ldn=1, w_ldk=d, n_rows=rows,
                rowscale=coeff, a2=du, b2=l_table, b2_group_stride=0, out=into, accumulate=into is not None)
            grad_l = ext.tall_tn_bf16(x, ext.rows_combine(du, bk.pos)).view(d, rank)
            grad_r = ext.tall_tn_bf16(dpre, u, gather=bk.token, offsets=bk.offsets).view(d_ff, rank)
            return dxs, dc, grad_l, grad_r

        dxs, dc_g, grad_lg, grad_rg = down(dg, wg, ug, lg, rg, dot_g)
        del dg
        dxs, dc_s, grad_ls, grad_rs = down(dsd, ws, us, ls, rs, dot_s, into=dxs)
        del dsd
        grad_x = ext.rows_combine(dxs, bk.pos)
        del dxs
        grad_coeff = grad_coeff + dc_g + dc_s
        grad_x, grad_rw, grad_rb = _route_backward_bf16(ctx, grad_coeff, prob, bk, block, x, rw, grad_x)
        grad_ld = ext.tall_tn_bf16(h, dzt, gather=bk.token, offsets=bk.offsets).view(d_ff, rank)
        grad_rd = ext.tall_tn_bf16(dy, ext.rows_combine(z, bk.pos)).view(d, rank)
        return (grad_x, grad_rw, grad_rb, grad_lg, grad_rg, grad_ls, grad_rs, grad_ld, grad_rd,
                None, None, None, None, None, None, None, None)


def routed_lora_llama_ffn_bf16(x, rw, rb, lg, rg, ls, rs, ld, rd, wg, ws, wd, n_blocks: int, top_k: int,
                               activation, origin=None):
    if origin is None:
        return RoutedLoRALLaMAFFNBf16.apply(x, rw, rb, lg, rg, ls, rs, ld, rd, wg, ws, wd, n_blocks, top_k,
                                            activation)
    return RoutedLoRALLaMAFFNBf16.apply(x, rw, rb, lg, rg, ls, rs, ld, rd, wg, ws, wd, n_blocks, top_k,
                                        activation, origin.input, origin.module)
