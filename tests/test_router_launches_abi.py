"""The router's three additive C entries (spt_lora_down2_route, spt_route_topk_counted,
spt_ffn_router_backward) are declared, exported and bound, refuse bad arguments on the host, and leave the
ABI version where it was; the ranking header they share issues no matrix-core instruction (so
test_exact_coverage keeps classifying routing.hip as it did).  No GPU: every call here ends in an error code."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'spt_hip.h')
CSRC = os.path.join(ROOT, 'spt-proto_amd', 'csrc')
ENTRIES = ('spt_lora_down2_route', 'spt_route_topk_counted', 'spt_ffn_router_backward')
EINVAL, ESHAPE, EUNSUP = -1, -2, -3
P = 0x10000                     # a 16-byte aligned stand-in for a device address


def test_entries_are_declared_exported_and_bound():
    from naive_gpt import ext
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    lib = ext.load_library()
    for name in ENTRIES:
        assert re.search(r'\bint {}\s*\('.format(name), text), name + ' is not declared'
        assert hasattr(lib, name), name + ' is not exported'
        assert name in ext._PROTOTYPES and getattr(lib, name).argtypes == ext._PROTOTYPES[name][0]
        # the prototype binds as many arguments as the header declares
        decl = re.search(r'\bint {}\s*\((.*?)\)\s*;'.format(name), text, flags=re.S).group(1)
        assert len(decl.split(',')) == len(ext._PROTOTYPES[name][0]), name


def test_abi_version_stays_40():
    from naive_gpt import ext
    assert int(re.search(r'#define SPT_ABI_VERSION (\d+)', open(HEADER).read()).group(1)) == 40
    assert ext.ABI_VERSION == 40 and ext.load_library().spt_abi_version() == 40


def test_ranking_header_has_one_definition_and_no_matrix_core_code():
    head = open(os.path.join(CSRC, 'route_rank.h')).read()
    assert 'mfma' not in head.lower() and 'split_bf16.h' not in head
    assert re.findall(r'#include\s+"([\w.]+)"', head) == ['spt_common.h']
    for unit in ('routing.hip', 'lora_side.hip'):
        text = open(os.path.join(CSRC, unit)).read()
        assert '#include "route_rank.h"' in text, unit
        assert 'unsigned order_key(' not in text and 'unsigned select_topk(' not in text, unit
    assert head.count('unsigned order_key(') == 1 and head.count('unsigned select_topk(') == 1


def test_no_new_public_launching_function():
    """The entries are reached through keywords of lora_down, route_topk_logits and ffn_coeff_grad."""
    import ast
    from naive_gpt import ext
    tree = ast.parse(open(ext.__file__).read())
    users = {}
    for f in tree.body:
        if isinstance(f, ast.FunctionDef):
            for a in ast.walk(f):
                if isinstance(a, ast.Attribute) and a.attr in ENTRIES:
                    users[a.attr] = f.name
    assert users == {'spt_lora_down2_route': 'lora_down', 'spt_route_topk_counted': 'route_topk_logits',
                     'spt_ffn_router_backward': 'ffn_coeff_grad'}


def _down(lib, x=P, ldx=64, rows=32, k=64, l=P, n=16, l2=P, n2=4, bias=P, top_k=2, counts=P, u=P, ldu=0,
          block_major=1, image=None, norms=None, exact=1):
    return lib.spt_lora_down2_route(x, ldx, rows, k, l, n, l2, n2, bias, top_k, counts, u, ldu, block_major,
                                    image, norms, exact, None)


def _topk(lib, logits=P, ld=16, bias=None, counts=P, prob=P, token=P, block=P, offsets=P, pos=P, t64=P, b64=P,
          coeff=P, T=32, G=4, k=2):
    return lib.spt_route_topk_counted(logits, ld, bias, counts, prob, token, block, offsets, pos, t64, b64, coeff,
                                      2.0, T, G, k, None)


def _back(lib, dot_main=P, dot_act=P, w=2, du=P, u=P, dzt=P, z=P, pos=P, block=P, coeff=P, prob=P, dlogit=P,
          du_tok=P, z_tok=P, dcoeff=None, T=32, G=4, k=2, rank=16):
    return lib.spt_ffn_router_backward(dot_main, dot_act, w, du, u, dzt, z, pos, block, coeff, 1e-12, 2.0, prob,
                                       dlogit, du_tok, z_tok, dcoeff, T, G, k, rank, None)


def test_entries_validate_their_arguments_without_gpu():
    from naive_gpt import ext
    lib = ext.load_library()
    assert _down(lib, counts=None) == EINVAL and _down(lib, l2=None) == EINVAL and _down(lib, x=None) == EINVAL
    assert _down(lib, top_k=0) == EINVAL and _down(lib, top_k=5) == EINVAL
    assert _down(lib, n=32) == EUNSUP and _down(lib, n2=9, top_k=2) == EUNSUP and _down(lib, exact=0) == EUNSUP
    assert _down(lib, k=48) == EUNSUP and _down(lib, x=P + 4) == ESHAPE
    assert _topk(lib, counts=None) == EINVAL and _topk(lib, prob=None) == EINVAL and _topk(lib, coeff=None) == EINVAL
    assert _topk(lib, k=0) == EINVAL and _topk(lib, k=5) == EINVAL and _topk(lib, T=0) == EINVAL
    assert _topk(lib, G=9, k=2) == EUNSUP and _topk(lib, T=65537) == EUNSUP
    assert _topk(lib, ld=2) == ESHAPE and _topk(lib, logits=P + 4) == ESHAPE
    for missing in ('dot_main', 'dot_act', 'du', 'u', 'dzt', 'z', 'pos', 'block', 'coeff', 'prob', 'dlogit',
                    'du_tok', 'z_tok'):
        assert _back(lib, **{missing: None}) == EINVAL, missing
    assert _back(lib, T=0) == EINVAL and _back(lib, w=0) == EINVAL and _back(lib, k=0) == EINVAL
    assert _back(lib, k=5) == EINVAL
    assert _back(lib, rank=8) == EUNSUP and _back(lib, rank=32) == EUNSUP and _back(lib, G=9) == EUNSUP
    assert _back(lib, du=P + 4) == ESHAPE and _back(lib, z_tok=P + 8) == ESHAPE
