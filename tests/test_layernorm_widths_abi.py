"""spt_layernorm_form: the one width gate of the fused add + norm kernels (csrc/layernorm.hip), as the
header declares it, the library exports it and naive_gpt.ext binds it -- and the C entries and the
Python gate both decide from it.  No GPU: the pointers below are never dereferenced, every call here
ends in an error code or in a host-only answer."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'spt_hip.h')
EUNSUP = -3
P = 0x10000                     # a 16-byte aligned stand-in for a device address


def _ext():
    from naive_gpt import ext
    return ext


def test_form_is_declared_exported_and_bound():
    ext = _ext()
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    assert re.search(r'\bint\s+spt_layernorm_form\s*\(\s*int\s+d\s*,\s*int\s+rms\s*\)\s*;', text)
    assert 'spt_layernorm_form' in ext._PROTOTYPES
    lib = ext.load_library()
    assert hasattr(lib, 'spt_layernorm_form')
    assert lib.spt_layernorm_form(1024, 0) == ext.layernorm_form(1024, False) == 1


@pytest.mark.parametrize('rms', [False, True], ids=['layernorm', 'rms'])
def test_form_per_width(rms):
    form = _ext().layernorm_form
    for d in (256, 512, 768, 1024, 2048):
        assert form(d, rms) == 1, d
    assert form(2560, rms) > 1 and form(5120, rms) > 1
    assert form(4096, rms) == (1 if rms else form(4096, False)) and form(4096, False) > 1
    for d in (2560, 4096, 5120):
        assert form(d, rms) in (1, 2, 4)
    for d in (96, 2304, 8448, 0, -256):
        assert form(d, rms) == 0, d


@pytest.mark.parametrize('rms', [False, True], ids=['layernorm', 'rms'])
def test_python_gate_asks_the_same_function(rms):
    """`layernorm_supported` is `layernorm_takes` on the tensor's description; over every multiple of 64
    up to 8192 it answers what spt_layernorm_form answers."""
    ext = _ext()
    taken = []
    for d in range(64, 8193, 64):
        want = ext.layernorm_form(d, rms) > 0
        assert ext.layernorm_takes(True, torch.float32, (3, d), d, rms) == want, d
        if want:
            taken.append(d)
        # what refuses a tensor whatever the width: not on the device, not fp32, another last dimension, empty
        assert not ext.layernorm_takes(False, torch.float32, (3, d), d, rms)
        assert not ext.layernorm_takes(True, torch.bfloat16, (3, d), d, rms)
        assert not ext.layernorm_takes(True, torch.float32, (3, d + 64), d, rms)
        assert not ext.layernorm_takes(True, torch.float32, (0, d), d, rms)
        assert not ext.layernorm_supported(torch.zeros([2, d]), d, rms)          # a CPU tensor
    assert taken == [256, 512, 768, 1024, 2048, 2560, 4096, 5120]
    assert list(ext.LAYERNORM_WIDTHS) == taken and min(ext.LAYERNORM_WIDTHS) == 256


def test_entries_refuse_a_width_before_any_launch():
    lib = _ext().load_library()
    for d in (2304, 96, 8448):
        for rms in (0, 1):
            assert lib.spt_add_layernorm_forward(P, P, P, P, P, P, P, P, 4, d, 1e-5, rms, None) == EUNSUP
            assert lib.spt_layernorm_backward(P, P, P, P, P, P, P, P, P + 4 * d, P, 4, d, rms, None) == EUNSUP


def test_abi_version_is_unchanged():
    ext = _ext()
    lib = ext.load_library()
    lib.spt_abi_version.restype = ctypes.c_int
    header = int(re.search(r'#define SPT_ABI_VERSION (\d+)', open(HEADER).read()).group(1))
    assert header == 40 and lib.spt_abi_version() == 40 and ext.ABI_VERSION == 40
