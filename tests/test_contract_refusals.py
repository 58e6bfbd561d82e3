"""Every alignment / leading-dimension precondition include/spt_hip.h states is refused with SPT_ESHAPE
before anything touches the device.

One row of ROWS per stated condition: a call that satisfies everything else (the entry's BASE call,
which itself gets past every precondition) and violates only that condition.  Pointers are made-up
non-NULL addresses of the stated alignment; entries that take host arrays of device pointers get real
host arrays of made-up addresses.  No entry may dereference a device pointer on the host or launch
before it has validated.

This tier runs only where no GPU is visible: there a missing check is visible and harmless (the
launch returns HIP's "no device" error, a positive code, instead of -2).  Such a call must never reach
a real device, so there is no GPU variant of it.
"""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'spt_hip.h')

no_gpu = pytest.mark.skipif(torch.cuda.is_available(),
                            reason='below-contract pointers must never reach a real device')

SPT_EINVAL, SPT_ESHAPE, SPT_EUNSUP = -1, -2, -3
FAKE = 0x7f0000000000              # made-up device addresses: 1 MiB apart, 1 MiB aligned


def prototypes():
    """{entry: [parameter names]} of the header's prototypes"""
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r'\b(spt_[a-z_0-9]+)\s*\(([^)]*)\)', text):
        params = [p.strip() for p in m.group(2).split(',') if p.strip() and p.strip() != 'void']
        out[m.group(1)] = [re.sub(r'.*[\s*]', '', p) for p in params]
    return out


class Arr:
    """A host array of `count` made-up device addresses, the first `off` bytes off its alignment."""

    def __init__(self, count, off=0):
        self.count, self.off = count, off


def _bind(lib, entry, values):
    """The entry's arguments by name -> the ctypes call's arguments.  A parameter that is not named
    gets a made-up aligned address (the `stream`: NULL); an int `p` for a pointer parameter is that
    many bytes past one; None is NULL."""
    from naive_gpt import ext
    names = prototypes()[entry]
    argtypes = ext._PROTOTYPES[entry][0]
    assert len(names) == len(argtypes), entry
    unknown = set(values) - set(names)
    assert not unknown, (entry, unknown)
    args, keep = [], []
    for i, (name, ctype) in enumerate(zip(names, argtypes)):
        v = values.get(name, 0 if name != 'stream' else None)
        if ctype is ctypes.c_void_p:
            if isinstance(v, Arr):
                arr = (ctypes.c_void_p * v.count)(*[FAKE + (16 * i + j << 20) + (v.off if j == 0 else 0)
                                                    for j in range(v.count)])
                keep.append(arr)
                v = ctypes.cast(arr, ctypes.c_void_p)
            elif isinstance(v, ctypes.Structure):
                keep.append(v)
                v = ctypes.cast(ctypes.pointer(v), ctypes.c_void_p)
            elif v is not None:
                v = FAKE + (16 * i << 20) + v
        args.append(v)
    return args, keep


def _desc(cls, **fields):
    """A descriptor: pointer fields named with an int get a made-up address that many bytes off"""
    d = cls()
    for i, (name, ctype) in enumerate(cls._fields_):
        if name in fields:
            v = fields[name]
            if ctype is ctypes.c_void_p and v is not None:
                v = FAKE + (1 << 30) + (i << 20) + v
            setattr(d, name, v)
    return d


def _gg(**over):
    from naive_gpt import ext
    f = dict(a=0, w=0, offsets=0, out=0, n_rows=64, k=64, n=64, n_groups=2, lda=64, w_group_stride=4096,
             w_ldn=64, w_ldk=1)
    f.update(over)
    return _desc(ext._GroupedDesc, **f)


def _gg_ext(**over):
    return _gg(**dict(dict(a2=0, b2=0, lda2=16, r=16, b2_group_stride=1024, b2_ldn=16), **over))


def _gb(**over):
    from naive_gpt import ext
    f = dict(a=0, w=0, offsets=0, out=0, n_rows=64, k=64, n=64, n_groups=2, lda=64, w_group_stride=4096,
             w_ldn=64, w_ldk=1)
    f.update(over)
    return _desc(ext._GroupedDescBf16, **f)


def _gb_ext(**over):
    from naive_gpt import ext
    f = dict(a2=0, b2=0, lda2=16, r=16, b2_group_stride=1024, b2_ldn=16)
    f.update(over)
    return _desc(ext._GroupedExtBf16, **f)


WGRAD = dict(ldg=64, lda=32, n_groups=2, n_rows=100, n=64, k=32, group_stride=2048, ldn=32)
DOWN = dict(ldx=64, rows=100, k=64, n=16)
TALL = dict(ldw=64, ldn=16, n_groups=1, rows=100, width=64, n=16, gather=None, offsets=None)
NORM = dict(count=2, wides=Arr(2), narrows=Arr(2), outs=Arr(2), ldw=64, ldn=16, rows=100, width=64, n=16,
            narrows2=None, ldn2=0, n2=0, means=Arr(2), rstds=Arr(2), gammas=Arr(2), betas=Arr(2), outs2=None)
NORM2 = dict(NORM, narrows2=Arr(2), ldn2=4, n2=4, outs2=Arr(2))
ROUTE = dict(ld=8, scale=2.0, n_tokens=100, n_blocks=8, k=2)
LN = dict(rows=37, d=768, eps=1e-5, rms=0)
ROTARY = dict(x=Arr(3), n_parts=3, n_rot=2, out_stride=1 << 16, batch=2, seq_length=16, n_heads=4, d_head=64)
SWIGLU = dict(rows=33, n=100)
CSR = dict(batch_size=3, seq_length=100, nnz=1200)
ROUTER_BWD = dict(width=4, floor_value=1e-6, scale=2.0, n_tokens=100, n_blocks=8, k=2, rank=16, dcoeff=None)

# entry -> the arguments of a call that meets every precondition
BASE = {
    'spt_grouped_gemm': dict(n_rows=64, k=64, n=64, n_groups=2, lda=64, w_group_stride=4096, w_ldn=64, w_ldk=1,
                             gather=None, bias=None, rowscale=None),
    'spt_grouped_gemm_fused': dict(desc=_gg),
    'spt_grouped_gemm_fused_w16': dict(desc=lambda **o: _gg(**dict(dict(w_image=0), **o))),
    'spt_grouped_gemm_bf16': dict(desc=_gb),
    'spt_grouped_gemm_bf16_ext': dict(desc=_gb, ext=_gb_ext),
    'spt_grouped_gemm_wgrad': dict(WGRAD, gather_g=None, gather_a=None, rowscale=None),
    'spt_grouped_gemm_wgrad_bf16': dict(WGRAD, gather_g=None, gather_a=None, rowscale=None),
    'spt_split_bf16': dict(rows=33, cols=40, ld=40),
    'spt_split_f16': dict(rows=33, cols=40, ld=40),
    'spt_lora_down': dict(DOWN, ldu=0, u_block_major=0, norms=None, exact=0),
    'spt_lora_down_grouped': dict(DOWN, l_group_stride=1024, n_groups=2, ldu=0, norms=None),
    'spt_lora_down_grouped_cols': dict(DOWN, l_group_stride=1024, n_groups=2, ldu=32),
    'spt_lora_down_tables': dict(ldx=64, rows=100, k=64, n_tables=3, table_stride=1024, norms=None, exact=0),
    'spt_lora_down2': dict(DOWN, n=32, n2=5, ldu=0, u_block_major=1, norms=None, exact=1),
    'spt_lora_down2_route': dict(DOWN, n2=8, top_k=2, ldu=0, u_block_major=1, norms=None, exact=1),
    'spt_softmax_forward': CSR, 'spt_softmax_backward': CSR,
    'spt_softmax_backward_clamped': dict(CSR, scale=0.125, clamp=10.0),
    'spt_route_topk': dict(n_tokens=100, n_blocks=4, k=2),
    'spt_route_topk_coeff': dict(scale=2.0, n_tokens=100, n_blocks=4, k=2),
    'spt_ffn_coeff_grad': dict(width=4, floor_value=1e-6, n_rows=100, rank=16),
    'spt_embedding_rows_backward': dict(ldg=24, ldo=24, n_ids=40, width=24, n_rows=50),
    'spt_rows_combine': dict(n_tokens=100, k=2, d=100),
    'spt_lora_down_bf16': dict(DOWN, ldu=0, u_block_major=0),
    'spt_lora_down_grouped_bf16': dict(DOWN, l_group_stride=1024, n_groups=2, ldu=0),
    'spt_cross_entropy_grad': dict(ld=1004, rows=33, n_classes=1001, ignore_index=-100),
    'spt_cross_entropy_eval': dict(ld=1004, rows=33, n_classes=1001, ignore_index=-100),
    'spt_add_layernorm_forward': LN,
    'spt_layernorm_backward': dict(rows=37, d=768, rms=0, dbeta=768 * 4 - (16 << 20)),     # dgamma + d: the next parameter's made-up address lies 16 MiB on
    'spt_tall_tn': dict(TALL, transposed=0),
    'spt_tall_tn_batch': dict(TALL, count=2, wides=Arr(2), narrows=Arr(2), outs=Arr(2), transposed=0),
    'spt_tall_tn_norm': dict(NORM, transposed=0, transposed2=0),
    'spt_tall_tn_bf16': TALL,
    'spt_route_topk_logits': ROUTE,
    'spt_route_topk_counted': ROUTE,
    'spt_ffn_router_backward': ROUTER_BWD,
    'spt_rotary': dict(ROTARY, transpose=0),
    'spt_swiglu_forward': dict(n_elements=3300),
    'spt_swiglu_backward': SWIGLU,
    'spt_swiglu_forward_bf16': dict(n_elements=3300),
    'spt_swiglu_backward_bf16': dict(n_elements=3300),
    'spt_swiglu_backward_dots_bf16': SWIGLU,
    'spt_rows_combine_side': dict(n_side=8, n_tokens=100, k=2, d=100),
    'spt_rows_combine_bf16': dict(n_tokens=100, k=2, d=100),
}


def _call(entry, over=None, desc=None, ext=None):
    from naive_gpt import ext as binding
    lib = binding.load_library()
    values = dict(BASE[entry])
    for name, fields in (('desc', desc), ('ext', ext)):
        if name in values:
            values[name] = values[name](**(fields or {}))
    values.update(over or {})
    args, keep = _bind(lib, entry, values)
    rc = getattr(lib, entry)(*args)
    del keep
    return rc


def _row(entry, what, over=None, desc=None, ext=None):
    return pytest.param(entry, over, desc, ext, id='{}-{}'.format(entry[4:], what))


def _ptrs(entry, names, off, what='{} {} bytes off'):
    return [_row(entry, what.format(n, off), {n: off}) for n in names.split()]


def _descs(entry, names, off, field='desc'):
    return [_row(entry, '{} {} bytes off'.format(n, off), **{field: {n: off}}) for n in names.split()]


ROWS = (
    # spt_grouped_gemm: "k % 4 == 0, lda % 4 == 0 and 16-byte aligned weight rows"
    [_row('spt_grouped_gemm', 'lda % 4', dict(lda=66)),
     _row('spt_grouped_gemm', 'w_ldn % 4', dict(w_ldn=66)),
     _row('spt_grouped_gemm', 'w_group_stride % 4', dict(w_group_stride=4098))]
    + _ptrs('spt_grouped_gemm', 'w', 8)
    # SptGroupedGemm: the same, the K extension, the segments, the queue
    + [_row('spt_grouped_gemm_fused', 'lda % 4', desc=dict(lda=66)),
       _row('spt_grouped_gemm_fused', 'w_ldn % 4', desc=dict(w_ldn=66)),
       _row('spt_grouped_gemm_fused', 'a_seg_stride % 4', desc=dict(a_seg_k=32, a_seg_stride=4098)),
       _row('spt_grouped_gemm_fused', 'relu_queue 8 bytes off',
            desc=dict(epilogue=1, activation=0, a_norm=0, w_norm=0, relu_queue=8, relu_queue_bytes=1 << 20)),
       _row('spt_grouped_gemm_fused', 'lda2 % 4', desc=dict(a2=0, b2=0, r=16, lda2=18, b2_ldn=16, b2_group_stride=1024)),
       _row('spt_grouped_gemm_fused', 'b2_ldn % 4', desc=dict(a2=0, b2=0, r=16, lda2=16, b2_ldn=18, b2_group_stride=1024)),
       _row('spt_grouped_gemm_fused', 'b2_group_stride % 4',
            desc=dict(a2=0, b2=0, r=16, lda2=16, b2_ldn=16, b2_group_stride=1026)),
       _row('spt_grouped_gemm_fused', 'b2_seg_stride % 4',
            desc=dict(a2=0, b2=0, r=16, lda2=16, b2_ldn=16, b2_group_stride=1024, b2_seg_stride=1026))]
    + _descs('spt_grouped_gemm_fused', 'w', 8)
    # fp16 weights: "`w` pointing at fp16 elements (8-byte aligned)"
    + _descs('spt_grouped_gemm_fused_w16', 'w', 4)
    # the weight gradient: "n, k, ldg, lda, ldn and group_stride multiples of 4 and G, A, out, dbias and
    # workspace 16-byte aligned"; bf16: G, A, out, dbias 8-byte, workspace 16-byte
    + [_row(e, p + ' % 4', {p: WGRAD[p] + 2}) for e in ('spt_grouped_gemm_wgrad', 'spt_grouped_gemm_wgrad_bf16')
       for p in ('ldg', 'lda', 'ldn', 'group_stride')]
    + _ptrs('spt_grouped_gemm_wgrad', 'g a out dbias workspace', 8)
    + _ptrs('spt_grouped_gemm_wgrad_bf16', 'g a out dbias', 4) + _ptrs('spt_grouped_gemm_wgrad_bf16', 'workspace', 8)
    # bf16 storage: "k % 64 == 0, lda % 8 == 0, w_group_stride % 8 == 0, a and w 16-byte aligned; w_ldk == 1:
    # w_ldn % 8 == 0 ...; w_ldn == 1: w_ldk % 8 == 0 ...; out, out2, bias, h_in, s_in 8-byte aligned"
    + [_row('spt_grouped_gemm_bf16', 'lda % 8', desc=dict(lda=68)),
       _row('spt_grouped_gemm_bf16', 'w_group_stride % 8', desc=dict(w_group_stride=4100)),
       _row('spt_grouped_gemm_bf16', 'w_ldn % 8', desc=dict(w_ldn=68)),
       _row('spt_grouped_gemm_bf16', 'w_ldk % 8', desc=dict(w_ldn=1, w_ldk=68)),
       _row('spt_grouped_gemm_bf16', 'out2 4 bytes off', desc=dict(epilogue=1, activation=2, out2=4)),
       _row('spt_grouped_gemm_bf16', 'h_in 4 bytes off',
            desc=dict(epilogue=2, activation=0, h_in=4, pdot_main=0, pdot_act=0, pdot_ld=2)),
       _row('spt_grouped_gemm_bf16', 's_in 4 bytes off',
            desc=dict(epilogue=2, activation=2, s_in=4, pdot_main=0, pdot_act=0, pdot_ld=2))]
    + _descs('spt_grouped_gemm_bf16', 'a w', 8) + _descs('spt_grouped_gemm_bf16', 'out bias', 4)
    # its K extension: "lda2 % 4 == 0, b2_ldn % 4 == 0, b2_group_stride % 4 == 0, a2 16-byte and b2 8-byte aligned"
    + [_row('spt_grouped_gemm_bf16_ext', 'lda2 % 4', ext=dict(lda2=18)),
       _row('spt_grouped_gemm_bf16_ext', 'b2_ldn % 4', ext=dict(b2_ldn=18)),
       _row('spt_grouped_gemm_bf16_ext', 'b2_group_stride % 4', ext=dict(b2_group_stride=1026))]
    + _descs('spt_grouped_gemm_bf16_ext', 'a2', 8, 'ext') + _descs('spt_grouped_gemm_bf16_ext', 'b2', 4, 'ext')
    # the images: "ld % 4 == 0, 16-byte aligned"; halves: "ld % 8 == 0, 16-byte aligned"
    + [_row('spt_split_bf16', 'ld % 4', dict(ld=42)), _row('spt_split_f16', 'ld % 8', dict(ld=44))]
    + _ptrs('spt_split_bf16', 'src', 8) + _ptrs('spt_split_f16', 'src_f16', 8)
    # the down products: "x ... and image 16-byte aligned, ldx % 4 == 0 ... in every entry of this family";
    # "table_stride % 4 == 0"; "l2 ... 16-byte aligned"
    + [r for e in ('spt_lora_down', 'spt_lora_down_grouped', 'spt_lora_down_tables', 'spt_lora_down2',
                   'spt_lora_down2_route')
       for r in [_row(e, 'ldx % 4', dict(ldx=66))] + _ptrs(e, 'x image', 8)]
    + [_row('spt_lora_down_grouped_cols', 'ldx % 4', dict(ldx=66))] + _ptrs('spt_lora_down_grouped_cols', 'x', 8)
    + [_row('spt_lora_down_tables', 'table_stride % 4', dict(table_stride=1026))]
    + _ptrs('spt_lora_down2', 'l2', 8) + _ptrs('spt_lora_down2_route', 'l2', 8)
    # the CSR softmax: "indices and every [B, nnz] float operand of the three softmax entries 16-byte aligned"
    + _ptrs('spt_softmax_forward', 'indices values output', 8)
    + _ptrs('spt_softmax_backward', 'indices output grad_output grad_values', 8)
    + _ptrs('spt_softmax_backward_clamped', 'indices output grad_output clamped_scores grad_scores', 8)
    # "prob 16-byte aligned (... also in spt_route_topk_coeff)"
    + _ptrs('spt_route_topk', 'prob', 8) + _ptrs('spt_route_topk_coeff', 'prob', 8)
    # "rank % 4 == 0 and these four 16-byte aligned"
    + _ptrs('spt_ffn_coeff_grad', 'du u dzt z', 8)
    # "ldg % 4 == 0, ldo % 4 == 0 ..., grad and out 16-byte and workspace 8-byte aligned"
    + [_row('spt_embedding_rows_backward', 'ldg % 4', dict(ldg=26)),
       _row('spt_embedding_rows_backward', 'ldo % 4', dict(ldo=26))]
    + _ptrs('spt_embedding_rows_backward', 'grad out', 8) + _ptrs('spt_embedding_rows_backward', 'workspace', 4)
    # "rows, bias and out 16-byte aligned (... also in spt_rows_combine_side)"
    + _ptrs('spt_rows_combine', 'rows bias out', 8) + _ptrs('spt_rows_combine_side', 'rows bias out', 8)
    # "k % 64 == 0, ldx % 8 == 0, x 16-byte and l 8-byte aligned, l_group_stride % 4 == 0"
    + [_row(e, 'ldx % 8', dict(ldx=68)) for e in ('spt_lora_down_bf16', 'spt_lora_down_grouped_bf16')]
    + [_row('spt_lora_down_grouped_bf16', 'l_group_stride % 4', dict(l_group_stride=1026))]
    + _ptrs('spt_lora_down_bf16', 'x', 8) + _ptrs('spt_lora_down_bf16', 'l', 4)
    + _ptrs('spt_lora_down_grouped_bf16', 'x', 8) + _ptrs('spt_lora_down_grouped_bf16', 'l', 4)
    # the head loss: "ld % 4 == 0, 16-byte aligned"
    + [_row(e, 'ld % 4', dict(ld=1006)) for e in ('spt_cross_entropy_grad', 'spt_cross_entropy_eval')]
    + _ptrs('spt_cross_entropy_grad', 'logits', 8) + _ptrs('spt_cross_entropy_eval', 'logits', 8)
    # the norms: x, r, gamma, beta, s, y / s, dy, gamma, dskip, dx, partial 16-byte aligned
    + _ptrs('spt_add_layernorm_forward', 'x r gamma beta s y', 8)
    + _ptrs('spt_layernorm_backward', 's dy gamma dskip dx partial', 8)
    # tall_tn: "width, ldw even; wide 8-byte aligned; ldn a multiple of 4 and narrow 16-byte aligned"
    + [_row(e, 'ldw even', dict(ldw=65)) for e in ('spt_tall_tn', 'spt_tall_tn_batch', 'spt_tall_tn_norm', 'spt_tall_tn_bf16')]
    + [_row(e, 'ldn % 4', dict(ldn=18)) for e in ('spt_tall_tn', 'spt_tall_tn_batch', 'spt_tall_tn_norm', 'spt_tall_tn_bf16')]
    + _ptrs('spt_tall_tn', 'wide', 4) + _ptrs('spt_tall_tn', 'narrow', 8)
    + [_row(e, 'wides[0] 4 bytes off', dict(wides=Arr(2, 4))) for e in ('spt_tall_tn_batch', 'spt_tall_tn_norm')]
    + [_row(e, 'narrows[0] 8 bytes off', dict(narrows=Arr(2, 8))) for e in ('spt_tall_tn_batch', 'spt_tall_tn_norm')]
    # norm on load: "narrows2 16-byte aligned, ldn2 a multiple of 4, gammas / betas 8-byte aligned"
    + [_row('spt_tall_tn_norm', 'narrows2[0] 8 bytes off', dict(NORM2, narrows2=Arr(2, 8))),
       _row('spt_tall_tn_norm', 'ldn2 % 4', dict(NORM2, ldn2=6)),
       _row('spt_tall_tn_norm', 'gammas[0] 4 bytes off', dict(gammas=Arr(2, 4))),
       _row('spt_tall_tn_norm', 'betas[0] 4 bytes off', dict(betas=Arr(2, 4)))]
    # bf16 wide: "narrow ... (ldn % 4 == 0, 16-byte aligned); wide 4-byte aligned, width and ldw even"
    + _ptrs('spt_tall_tn_bf16', 'wide', 2) + _ptrs('spt_tall_tn_bf16', 'narrow', 8)
    # the router: "logits ... 16-byte aligned, ld >= n_blocks"
    + [_row(e, 'ld < n_blocks', dict(ld=4)) for e in ('spt_route_topk_logits', 'spt_route_topk_counted')]
    + _ptrs('spt_route_topk_logits', 'logits', 8) + _ptrs('spt_route_topk_counted', 'logits', 8)
    # "the [*, rank] operands 16-byte aligned"
    + _ptrs('spt_ffn_router_backward', 'du u dzt z du_tok z_tok', 8)
    # rotary: "all pointers 16-byte aligned; `x` is a host array of n_parts device pointers"
    + _ptrs('spt_rotary', 'out cos_table sin_table', 8) + [_row('spt_rotary', 'x[0] 8 bytes off', dict(x=Arr(3, 8)))]
    # the gated middle: "gate, side, h and the four gradients 16-byte aligned"; bf16: 8-byte; the dots 4-byte
    + _ptrs('spt_swiglu_forward', 'gate side h', 8)
    + _ptrs('spt_swiglu_backward', 'grad_h gate side grad_gate grad_side', 8)
    + _ptrs('spt_swiglu_forward_bf16', 'gate side h', 4)
    + _ptrs('spt_swiglu_backward_bf16', 'grad_h gate side grad_gate grad_side', 4)
    + _ptrs('spt_swiglu_backward_dots_bf16', 'grad_h gate side grad_gate grad_side', 4)
    + _ptrs('spt_swiglu_backward_dots_bf16', 'dots', 2)
    # un-bucketing: "side_w [n_side, d], 16-byte aligned"; "bf16 rows / bias / out (8-byte aligned)"
    + _ptrs('spt_rows_combine_side', 'side_w', 8) + _ptrs('spt_rows_combine_bf16', 'rows bias out', 4)
)


@no_gpu
@pytest.mark.parametrize('entry', sorted(BASE))
def test_base_call_meets_every_precondition(entry):
    """Each row below changes one thing of this call: it must itself get past the validation (any
    precondition code here would make its rows vacuous).  Without a device the launch then fails with a
    positive HIP error -- or, where the entry asks the device for its size first, with the code it gives
    a device that has none."""
    rc = _call(entry)
    assert rc > 0 or (rc == SPT_EINVAL and entry.startswith('spt_grouped_gemm') and 'wgrad' not in entry), rc


@no_gpu
@pytest.mark.parametrize('entry,over,desc,ext', ROWS)
def test_stated_precondition_is_refused_before_any_launch(entry, over, desc, ext):
    assert _call(entry, over, desc, ext) == SPT_ESHAPE


def test_every_entry_with_rows_has_a_base_call():
    entries = {p.values[0] for p in ROWS}
    assert entries == set(BASE), entries ^ set(BASE)
    assert len(ROWS) > 120
