"""Guard bands: make an access outside a buffer visible.

`guarded(pattern)` patches `torch.empty`, `torch.empty_like` and `torch.Tensor.new_empty`, the three
functions tests/poison.py patches, looked up on `torch` at call time by `naive_gpt.ext` and the
layers.  Every tensor they create on a listed device type becomes a view into one private uint8
allocation of its own,

    [lead band: band_bytes][the tensor's bytes][trail band: band_bytes]

whose first tensor byte is 512-byte aligned, as the caching allocator would give it (or, with
`skew`, lies that many bytes past a 512-byte boundary: the weakest placement the library's contract
still accepts, tests/test_gpu_placement.py), and whose trail band begins at the tensor's last byte
plus one, with no rounding gap.  One allocation per tensor,
never an arena: `ext.back_to_back` and `ext.spacing_of` compare `untyped_storage().data_ptr()`, and
`ext._bounds_behind` reads the storage size behind `row_sum` (of the forward's own `stats` buffer,
which always has the bounds; a foreign `row_sum` would find the trail band there).  `home(t, state)`
gives an existing tensor, an input, the same surroundings on the GPU.

The bands hold elements of the tensor's own dtype:

  pattern | floating  | integers, bool | uint8 workspaces
  zero    | 0         | 0              | all bytes 0
  nan     | quiet NaN | 1              | each 32-bit word 1 (counted from the tensor's first byte)

Integers never get a large or negative value, for the reason tests/poison.py gives: an over-read
index must stay a valid index.  The tensor's own bytes stay as the original function left them.
A store outside a buffer changes a band, and `state.verify()` (after the caller's device
synchronize) names it.  A store that happens to equal one pattern cannot equal the other, and a
result that depends on bytes outside an input differs between the two patterns: every case runs
under both.

What this tier cannot see: an overrun beyond the band (the default 1 MiB per side is above the
largest overrun a tile-granular store can make at the registry's shapes, 127 extra rows of at most
1024 floats = 508 KiB; a wilder store is outside it), an access outside an LDS array, and a read
outside a buffer that is masked before it is used.
"""
import contextlib
import sys

import torch

PATTERNS = ('zero', 'nan')
ALIGN = 512


class _Block:
    """One guarded allocation: `buf` uint8, the tensor's bytes at buf[lead : lead + nbytes]."""

    def __init__(self, buf, lead, nbytes, trail, tensor, caller):
        self.buf, self.lead, self.nbytes, self.trail = buf, lead, nbytes, trail
        self.shape, self.dtype, self.caller = tuple(tensor.shape), tensor.dtype, caller

    def bands(self):
        """(name, uint8 view, byte offset of its first byte relative to the tensor's first byte)"""
        end = self.lead + self.nbytes
        return (('lead', self.buf[self.lead - self.trail:self.lead], -self.trail),
                ('trail', self.buf[end:end + self.trail], self.nbytes))


class Guard:
    """What one `guarded` block did: `allocations` carved tensors, `homes` carved inputs,
    `unguarded` results of the patched functions that could not be rebuilt, by allocating function
    in `sites`.  Holds every allocation until `release()`."""

    def __init__(self, pattern, band_bytes, devices, originals, skew=0):
        assert pattern in PATTERNS, pattern
        assert band_bytes > 0 and band_bytes % ALIGN == 0, 'band_bytes: a positive multiple of 512'
        assert isinstance(skew, int) and 0 <= skew < ALIGN and skew % 16 == 0, 'skew: a multiple of 16 below 512'
        self.pattern, self.band_bytes, self.devices, self.skew = pattern, band_bytes, tuple(devices), skew
        self.empty, self.empty_like, self.new_empty = originals
        self.allocations = self.homes = self.unguarded = 0
        self.sites = {}
        self.blocks = []
        self._patterns = {}

    # -- the bands' contents

    def _band_pattern(self, dtype, device, first):
        """band_bytes bytes of the pattern for a band whose first byte lies `first` bytes (mod 4)
        from the tensor's first byte"""
        key = (dtype, device, first % 4 if dtype == torch.uint8 else 0)
        if key not in self._patterns:
            n = self.band_bytes
            if self.pattern == 'zero':
                pat = torch.zeros([n], dtype=torch.uint8, device=device)
            elif dtype == torch.uint8:
                pat = ((torch.arange(n, device=device) + key[2]) % 4 == 0).to(torch.uint8)
            else:
                value = float('nan') if dtype.is_floating_point or dtype.is_complex else 1
                unit = torch.full([1], value, dtype=dtype).view(torch.uint8)
                pat = unit.repeat(n // unit.numel()).to(device)
            self._patterns[key] = pat
        return self._patterns[key]

    # -- carving

    def carve(self, shape, dtype, device, strides, caller):
        """An uninitialised tensor of this description inside a guarded allocation of its own."""
        item = dtype.itemsize
        numel = 1
        for s in shape:
            numel *= s
        span = 0 if numel == 0 else 1 + sum((n - 1) * st for n, st in zip(shape, strides))
        nbytes, band = span * item, self.band_bytes
        if min(strides, default=0) < 0 or ALIGN % item:
            raise ValueError('cannot carve strides {} of {}'.format(strides, dtype))
        buf = self.empty([band + nbytes + band + 2 * ALIGN], dtype=torch.uint8, device=device)
        lead = (-buf.data_ptr()) % ALIGN + band          # the CPU allocator aligns to 64 only
        lead += self.skew
        block_view = buf[lead:lead + nbytes].view(dtype)
        t = block_view.as_strided(tuple(shape), tuple(strides), lead // item)
        block = _Block(buf, lead, nbytes, band, t, caller)
        for _, view, first in block.bands():
            view.copy_(self._band_pattern(dtype, buf.device, first))
        self.blocks.append(block)
        self.sites[caller] = self.sites.get(caller, 0) + 1
        assert numel == 0 or t.data_ptr() == buf.data_ptr() + lead and t.data_ptr() % ALIGN == self.skew
        return t

    def rebuild(self, t, caller):
        """`t`, fresh from one of the patched functions: carved if it is on a listed device."""
        if not isinstance(t, torch.Tensor) or t.device.type not in self.devices:
            return t
        try:
            if t.layout != torch.strided or t.is_quantized or t.storage_offset() != 0:
                raise ValueError('not a plain strided tensor')
            with torch.no_grad():
                out = self.carve(t.shape, t.dtype, t.device, t.stride(), caller)
            if t.requires_grad:
                out.requires_grad_(True)
        except (ValueError, RuntimeError, TypeError):
            self.unguarded += 1
            return t
        self.allocations += 1
        return out

    # -- the check

    def verify(self):
        """Every band still holds its pattern, byte for byte (synchronize the device first)."""
        for b in self.blocks:
            for name, view, first in b.bands():
                want = self._band_pattern(b.dtype, b.buf.device, first)
                if torch.equal(view, want):
                    continue
                changed = (view != want).nonzero()
                at = first + int(changed[0])
                raise AssertionError(
                    'a store outside a buffer: the {} band of the {} {} tensor that {} allocated changed under '
                    'pattern {!r}: {} byte(s), the first at byte offset {} from the tensor\'s first byte '
                    '({})'.format(
                        name, list(b.shape), b.dtype, b.caller, self.pattern, int(changed.size(0)), at,
                        '{} past its end'.format(at - b.nbytes) if name == 'trail'
                        else '{} before its start'.format(-at)))

    def release(self):
        self.blocks = []
        self._patterns = {}


@contextlib.contextmanager
def guarded(pattern: str, band_bytes: int = 1 << 20, devices=('cuda',), skew: int = 0):
    """Inside the block, what `torch.empty`, `torch.empty_like` and `torch.Tensor.new_empty` create
    on `devices` lies between two bands of `band_bytes` each (a multiple of 512) that hold `pattern`.
    Their first byte lies `skew` bytes (a multiple of 16 below 512) past a 512-byte boundary.
    Yields the `Guard`; call its `verify()` after a device synchronize.  The default band is for
    single entries; a whole training step keeps every allocation alive and takes a smaller one."""
    empty, empty_like, new_empty = torch.empty, torch.empty_like, torch.Tensor.new_empty
    state = Guard(pattern, band_bytes, devices, (empty, empty_like, new_empty), skew)

    def caller():
        return sys._getframe(2).f_code.co_name

    def g_empty(*args, **kwargs):
        return state.rebuild(empty(*args, **kwargs), caller())

    def g_empty_like(*args, **kwargs):
        return state.rebuild(empty_like(*args, **kwargs), caller())

    def g_new_empty(self, *args, **kwargs):
        return state.rebuild(new_empty(self, *args, **kwargs), caller())

    torch.empty, torch.empty_like, torch.Tensor.new_empty = g_empty, g_empty_like, g_new_empty
    try:
        yield state
    finally:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty


def home(t: torch.Tensor, state: Guard, caller: str = None, device='cuda'):
    """A copy of `t` (on the CPU, or on the device already) inside a guarded allocation on `device`
    whose bands hold the state's pattern, at the state's skew: same values, dtype, shape and, as
    `.cuda()` keeps them, strides."""
    caller = caller or sys._getframe(1).f_code.co_name
    with torch.no_grad():
        strides = state.empty_like(t, device='meta').stride()
        out = state.carve(t.shape, t.dtype, torch.device(device), strides, caller)
        out.copy_(t)
    state.homes += 1
    return out
