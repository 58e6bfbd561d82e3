"""Every public entry of naive_gpt/ext.py that launches a matrix-core kernel (its C entry lives in a csrc
file that issues MFMAs) or stores bf16 (`bf16` in its name) is called by the exact tier
(test_gpu_exact_arithmetic.py) or the contract tier (test_gpu_arith_contract.py), or has a reason here
why it is not."""
import ast
import os
import re

from test_poison_coverage import EXT, launching_entries

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'spt-proto_amd', 'csrc')
TIERS = ('test_gpu_exact_arithmetic.py', 'test_gpu_arith_contract.py')
# entries whose matrix-core form is dispatched from a C entry in another (gather) file, or whose own
# file issues no MFMA although they are a stage of a matrix-core path
ELSEWHERE = {
    'sddmm_forward_cuda': 'sddmm.hip dispatches to the dense-stripe form of sddmm_tile.hip',
    'spmm_forward_cuda': 'spmm.hip dispatches to spmm_mfma_kernel of spmm_mfma.hip (SPT_SPMM_MFMA=1)',
    'attention_mfma_prepare': 'attention_tiles.hip builds the cell tiles the kernels of mfma_attention.hip read',
}

EXEMPT = {
    'image_of': 'a memo in front of split_bf16 (its case)',
    'weight_image': 'a per-parameter memo in front of split_bf16 (its case)',
}


def _unit_text(name, seen):
    """The text of a csrc file and, transitively, of the local headers it includes."""
    if name in seen or not os.path.exists(os.path.join(CSRC, name)):
        return ''
    seen.add(name)
    text = open(os.path.join(CSRC, name)).read()
    return text + ''.join(_unit_text(h, seen) for h in re.findall(r'#include\s+"([\w.]+)"', text))


def _c_files():
    """C entry name -> True when its source file, or a local header it includes, issues MFMAs."""
    out = {}
    for name in os.listdir(CSRC):
        if not name.endswith('.hip'):
            continue
        text = _unit_text(name, set())
        mfma = '__builtin_amdgcn_mfma' in text or 'v_mfma' in text
        for c in re.findall(r'extern "C"[^(]*?\b(spt_\w+)\s*\(', text):
            out[c] = mfma
    return out


def matrix_core_entries():
    tree = ast.parse(open(EXT).read())
    funcs = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    c_entries = {name: {a.attr for a in ast.walk(f) if isinstance(a, ast.Attribute) and a.attr.startswith('spt_')}
                 for name, f in funcs.items()}
    calls = {name: {c.func.id for c in ast.walk(f) if isinstance(c, ast.Call) and isinstance(c.func, ast.Name)}
             for name, f in funcs.items()}
    mfma = _c_files()

    def reaches(name, seen=()):
        direct = any(mfma.get(c, False) for c in c_entries[name])
        return direct or any(reaches(c, seen + (name,)) for c in calls[name] if c in funcs and c not in seen)
    return sorted(e for e in launching_entries() if 'bf16' in e or e in ELSEWHERE or reaches(e))


def called_by_tiers(tiers=TIERS):
    names = set()
    for t in tiers:
        for node in ast.walk(ast.parse(open(os.path.join(HERE, t)).read())):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute):
                names.add(node.func.attr)
    return names


def test_every_matrix_core_or_bf16_entry_has_an_exact_or_contract_case():
    entries = matrix_core_entries()
    assert {'grouped_gemm_fused', 'grouped_gemm_bf16_ext', 'lora_down', 'tall_tn_bf16', 'sddmm_forward_cuda',
            'attention_mfma_forward'} <= set(entries), entries
    covered = called_by_tiers()
    missing = [e for e in entries if e not in covered and e not in EXEMPT]
    assert not missing, 'matrix-core / bf16 entries with neither a case in {} nor an EXEMPT reason: {}'.format(
        ' / '.join(TIERS), missing)
    stale = [e for e in EXEMPT if e not in entries or e in covered]
    assert not stale, 'EXEMPT names entries that are not matrix-core / bf16 entries or that have a case: {}'.format(stale)
    assert all(reason.strip() for reason in EXEMPT.values())
