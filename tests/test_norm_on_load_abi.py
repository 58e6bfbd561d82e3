"""spt_tall_tn_norm refuses bad arguments on the host, before any launch (no GPU: the pointers below
are never dereferenced -- every call here ends in an error code)."""
import ctypes

EINVAL, ESHAPE, EUNSUP = -1, -2, -3
P = 0x10000                     # a 16-byte aligned stand-in for a device address


def _call(lib, count=1, wides=(P,), ldw=1024, narrows=(P,), ldn=16, narrows2=None, ldn2=0, n2=0, means=None,
          rstds=None, gammas=None, betas=None, rows=1024, width=1024, n=16, outs=(P,), transposed=0, outs2=None,
          transposed2=0, workspace=P):
    arr = lambda v: None if v is None else (ctypes.c_void_p * len(v))(*v)
    return lib.spt_tall_tn_norm(count, arr(wides), ldw, arr(narrows), ldn, arr(narrows2), ldn2, n2, arr(means),
                                arr(rstds), arr(gammas), arr(betas), rows, width, n, arr(outs), transposed,
                                arr(outs2), transposed2, workspace, None)


def test_tall_tn_norm_validates_its_arguments_without_gpu():
    from naive_gpt import ext
    lib = ext.load_library()
    assert _call(lib, wides=None) == EINVAL and _call(lib, workspace=None) == EINVAL
    assert _call(lib, count=0) == EINVAL and _call(lib, count=5, wides=(P,) * 5, narrows=(P,) * 5,
                                                   outs=(P,) * 5) == EINVAL
    assert _call(lib, wides=(None,)) == EINVAL and _call(lib, rows=0) == EINVAL and _call(lib, ldw=1022) == EINVAL
    # the column counts the kernels are built for: 16, 48, 16 + 4
    assert _call(lib, n=4, ldn=4) == EUNSUP and _call(lib, n=32, ldn=32) == EUNSUP
    assert _call(lib, n=48, ldn=48, n2=4, narrows2=(P,), ldn2=4, outs2=(P,)) == EUNSUP
    # a second operand comes with its output, and only with n2
    assert _call(lib, n2=4, ldn2=4) == EINVAL and _call(lib, narrows2=(P,)) == EINVAL
    assert _call(lib, n2=4, narrows2=(P,), ldn2=4, outs2=(None,)) == EINVAL
    assert _call(lib, n2=4, narrows2=(None,), ldn2=4, outs2=(P,)) == EINVAL
    assert _call(lib, n2=4, narrows2=(P,), ldn2=2, outs2=(P,)) == EINVAL
    assert _call(lib, n2=4, narrows2=(P + 4,), ldn2=4, outs2=(P,)) == ESHAPE
    # a norm is (rstd, gamma) at least; statistics or parameters without rstd are an error
    assert _call(lib, means=(P,)) == EINVAL and _call(lib, rstds=(P,)) == EINVAL
    assert _call(lib, rstds=(None,), gammas=(P,)) == EINVAL and _call(lib, rstds=(P,), gammas=(None,)) == EINVAL
    assert _call(lib, rstds=(P,), gammas=(P + 4,)) == ESHAPE
    assert _call(lib, rstds=(P,), gammas=(P,), betas=(P + 4,)) == ESHAPE
    # layouts and alignment as spt_tall_tn
    assert _call(lib, transposed=3) == EINVAL and _call(lib, transposed2=2) == EINVAL
    assert _call(lib, width=1023, ldw=1023) == ESHAPE and _call(lib, wides=(P + 4,)) == ESHAPE
    assert _call(lib, ldn=18) == ESHAPE and _call(lib, narrows=(P + 8,)) == ESHAPE
