"""Every public entry of naive_gpt/ext.py that launches a kernel (reaches `_stream(`, directly or
through another function of ext.py) has a poisoned-buffer case in
test_gpu_poisoned_buffers.CASES, or a reason here why it needs none."""
import ast
import os

import test_gpu_poisoned_buffers as suite

EXT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'spt-proto_amd', 'naive_gpt',
                   'ext.py')

EXEMPT = {
    'image_of': 'a memo in front of split_bf16 (its case); fresh_caches() empties the memo',
    'weight_image': 'a per-parameter memo in front of split_bf16 (its case); fresh_caches() empties it',
}


def launching_entries(path=EXT):
    tree = ast.parse(open(path).read())
    funcs = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    calls = {name: {c.func.id for c in ast.walk(f) if isinstance(c, ast.Call) and isinstance(c.func, ast.Name)}
             for name, f in funcs.items()}
    memo = {}

    def launches(name, seen=()):
        if name not in memo:
            memo[name] = '_stream' in calls[name] or any(
                launches(c, seen + (name,)) for c in calls[name] if c in funcs and c not in seen)
        return memo[name]
    return sorted(n for n in funcs if not n.startswith('_') and launches(n))


def test_every_launching_entry_has_a_poison_case():
    entries = launching_entries()
    assert len(entries) > 40 and 'grouped_gemm_wgrad' in entries and 'embedding_rows_backward' in entries
    missing = [e for e in entries if e not in suite.CASES and e not in EXEMPT]
    assert not missing, 'ext entries without a case in test_gpu_poisoned_buffers.CASES: {}'.format(missing)
    stale = [e for e in list(suite.CASES) + list(EXEMPT) if e not in entries]
    assert not stale, 'CASES / EXEMPT name entries that ext.py no longer has: {}'.format(stale)
    assert all(suite.CASES[e] for e in suite.CASES), 'an entry with an empty case list'
    assert all(c.kind in (suite.DET, suite.ATOMIC) for cases in suite.CASES.values() for c in cases)


def test_every_case_operand_reaches_the_device_through_dev():
    """No function defined above `CASES` in test_gpu_poisoned_buffers.py, nested ones included, calls
    `.cuda(` or passes `device='cuda'`, except `_dev` itself: test_gpu_guard_bands swaps `_dev` for
    guard.home, and an operand moved any other way would lie outside the guard bands."""
    source = open(suite.__file__).read()
    tree = ast.parse(source)
    cases_line = next(n.lineno for n in tree.body if isinstance(n, ast.Assign)
                      and any(isinstance(t, ast.Name) and t.id == 'CASES' for t in n.targets))
    funcs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.lineno < cases_line]
    assert len(funcs) > 40 and any(f.name == '_dev' for f in funcs)
    direct = []
    for f in funcs:
        if f.name == '_dev':
            assert any(isinstance(c, ast.Call) and isinstance(c.func, ast.Attribute) and c.func.attr == 'cuda'
                       for c in ast.walk(f)), '_dev no longer moves its argument itself'
            continue
        for c in ast.walk(f):
            if not isinstance(c, ast.Call):
                continue
            if isinstance(c.func, ast.Attribute) and c.func.attr == 'cuda':
                direct.append('{}:{} .cuda()'.format(f.name, c.lineno))
            for k in c.keywords:
                if k.arg == 'device' and not (isinstance(k.value, ast.Constant) and k.value.value in ('cpu', 'meta')) \
                        and 'cuda' in ast.unparse(k.value):
                    direct.append('{}:{} device={}'.format(f.name, c.lineno, ast.unparse(k.value)))
            if any(isinstance(a, ast.Constant) and a.value == 'cuda' for a in c.args):       # .to('cuda') and kin
                direct.append('{}:{} \'cuda\' as an argument'.format(f.name, c.lineno))
    assert not direct, 'operands that bypass _dev: {}'.format(direct)
    # the same in the text, comments and strings aside: the AST walk above and this agree
    above = source[:source.index('\nCASES = {')]
    lines = [l for l in above.split('\n') if ('.cuda(' in l or "device='cuda'" in l) and 'return t.cuda()' not in l]
    assert not lines, lines


def test_uint8_workspaces_are_classified():
    """Each `torch.empty([...], dtype=torch.uint8` of ext.py sits in a function that tests/poison.py
    classifies as float-only or as holding indices / counters."""
    import poison
    tree = ast.parse(open(EXT).read())
    sites = set()
    for f in tree.body:
        if isinstance(f, ast.FunctionDef):
            for c in ast.walk(f):
                if (isinstance(c, ast.Call) and isinstance(c.func, ast.Attribute) and c.func.attr == 'empty'
                        and any(k.arg == 'dtype' and ast.unparse(k.value) == 'torch.uint8' for k in c.keywords)):
                    sites.add(f.name)
    assert sites and not sites & set(poison.FLOAT_ONLY) & set(poison.INDEXED)
    assert sites <= set(poison.FLOAT_ONLY) | set(poison.INDEXED), sites - set(poison.FLOAT_ONLY) - set(poison.INDEXED)
