"""spt_cross_entropy_eval, the evaluation form of the head loss kernel: an additive C entry under ABI 40,
declared, exported and bound, reached through a keyword of ext.cross_entropy_grad_ (no new public
launching function), refusing bad arguments on the host.  No GPU: every call here ends in an error code."""
import ast
import re

from test_router_launches_abi import EINVAL, ESHAPE, EUNSUP, HEADER, P

ENTRY = 'spt_cross_entropy_eval'


def test_entry_is_declared_exported_and_bound():
    from naive_gpt import ext
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    lib = ext.load_library()
    assert re.search(r'\bint {}\s*\('.format(ENTRY), text), ENTRY + ' is not declared'
    assert hasattr(lib, ENTRY), ENTRY + ' is not exported'
    assert ENTRY in ext._PROTOTYPES and getattr(lib, ENTRY).argtypes == ext._PROTOTYPES[ENTRY][0]
    decl = re.search(r'\bint {}\s*\((.*?)\)\s*;'.format(ENTRY), text, flags=re.S).group(1)
    assert len(decl.split(',')) == len(ext._PROTOTYPES[ENTRY][0]) == 9
    assert 'const float *logits' in decl, 'the logits are read only'


def test_abi_version_stays_40():
    from naive_gpt import ext
    assert int(re.search(r'#define SPT_ABI_VERSION (\d+)', open(HEADER).read()).group(1)) == 40
    assert ext.ABI_VERSION == 40 and ext.load_library().spt_abi_version() == 40


def test_no_new_public_launching_function():
    from naive_gpt import ext
    tree = ast.parse(open(ext.__file__).read())
    users = {f.name for f in tree.body if isinstance(f, ast.FunctionDef)
             for a in ast.walk(f) if isinstance(a, ast.Attribute) and a.attr == ENTRY}
    assert users == {'cross_entropy_grad_'}
    import inspect
    assert inspect.signature(ext.cross_entropy_grad_).parameters['evaluate'].default is False


def _eval(lib, logits=P, ld=1056, rows=33, n_classes=1000, target=P, ignore=-100, loss=P, top=P):
    return lib.spt_cross_entropy_eval(logits, ld, rows, n_classes, target, ignore, loss, top, None)


def test_entry_validates_its_arguments_without_gpu():
    """The codes of spt_cross_entropy_grad, case by case."""
    from naive_gpt import ext
    lib = ext.load_library()
    assert lib.spt_cross_entropy_eval(None, 0, 0, 0, None, 0, None, None, None) == EINVAL
    for missing in ('logits', 'target', 'loss', 'top'):
        assert _eval(lib, **{missing: None}) == EINVAL, missing
    assert _eval(lib, rows=0) == EINVAL and _eval(lib, n_classes=0) == EINVAL and _eval(lib, ld=996) == EINVAL
    assert _eval(lib, ld=1002) == ESHAPE and _eval(lib, logits=P + 4) == ESHAPE
    assert _eval(lib, rows=1 << 31) == EUNSUP and _eval(lib, ld=1 << 31) == EUNSUP
    grad = lib.spt_cross_entropy_grad
    assert grad(None, 1056, 33, 1000, P, P, P, -100, None) == EINVAL
    assert grad(P, 1002, 33, 1000, P, P, P, -100, None) == ESHAPE and grad(P, 1 << 31, 33, 1000, P, P, P, -100, None) == EUNSUP
