"""Inputs the matrix-core kernels must reproduce exactly, and the rounding rules of their contracts.

The fp32 split path (`split2` and `mm` of csrc/split_bf16.h: hi = RNE(x), lo = RNE(x - hi), a product
as hi.hi + hi.lo + lo.hi in fp32) is determined bit for bit when
  * the operands are integers;
  * one operand of every product has at most 16 significant bits (then hi + lo == x exactly) and the
    other is exact in bf16 (its lo is 0, so the dropped lo.lo is 0);
  * every partial sum stays below 2^24 (every fp32 sum is then exact, in any order, at any MFMA shape).
The fp32 result must then equal the int64 / fp64 reference.  The bf16 path: 8-bit integers give an
exact fp32 accumulator, and the stored value must be `rne_bf16` of it; results in [256, 4096) are
exact ties often enough that ties-to-even is pinned without a special construction.

Generators take the contraction length K and assert the 2^24 rule for the largest sum they allow.
"""
import torch

EXACT_LIMIT = 2 ** 24        # integers below this are exact in fp32, and so is every sum of them


def fits_fp32(bound: float, unit: float = 1.0) -> float:
    """Assert that sums of magnitude <= bound in multiples of `unit` stay exact in fp32."""
    assert bound / unit < EXACT_LIMIT, 'exact inputs: {} / {} >= 2^24'.format(bound, unit)
    return bound


def bf16_ints(gen: torch.Generator, shape, bound: int) -> torch.Tensor:
    """fp32 integers in [-bound, bound], exact in bf16 (|x| <= 256)."""
    assert 0 < bound <= 256
    return torch.randint(-bound, bound + 1, list(shape), generator=gen).float()


def two_part_ints(gen: torch.Generator, shape, bound: int) -> torch.Tensor:
    """fp32 odd integers with 257 <= |x| <= bound < 2^16, random sign: at most 16 significant bits, so
    hi + lo == x exactly, and never exact in bf16, so every lo is non-zero (asserted for >= 90 %)."""
    assert 1024 <= bound < 2 ** 16, bound
    mag = torch.randint(128, (bound + 1) // 2, list(shape), generator=gen) * 2 + 1
    sign = torch.randint(0, 2, list(shape), generator=gen) * 2 - 1
    x = (mag * sign).float()
    hi = x.bfloat16().float()
    assert torch.equal(hi + (x - hi).bfloat16().float(), x)
    assert (x != hi).float().mean().item() >= 0.9
    return x


def two_part_bound(k: int, other: int, extra: float = 0.0) -> int:
    """The largest two-part magnitude against a bf16-exact operand of magnitude <= `other` over a
    contraction of length k, leaving `extra` (bias, side terms) below 2^24.  hi and lo are each at most
    (1 + 2^-8) |x| in magnitude, so the partial sums of the three split products over k terms stay
    under (1 + 2^-7) k |x| other."""
    bound = int((EXACT_LIMIT - 1 - extra) / ((1 + 2 ** -7) * k * other))
    bound = min(bound, 2 ** 16 - 1)
    fits_fp32((1 + 2 ** -7) * k * bound * other + extra)
    return bound


def pow2_rowscale(gen: torch.Generator, n: int, low: int = -1, high: int = 2) -> torch.Tensor:
    """fp32 [n]: powers of two 2^low .. 2^high (exact scalings of an exact sum)."""
    return torch.pow(2.0, torch.randint(low, high + 1, [n], generator=gen).float())


def _mask(bits: int) -> int:
    return (1 << bits) - 1


def rne_bf16(x: torch.Tensor) -> torch.Tensor:
    """fp64 -> the nearest bf16 value (ties to even), as fp64: rounded directly from the fp64 pattern,
    not through fp32 (fp64 -> fp32 -> bf16 can round twice).  Finite values inside bf16's normal range
    (or zero) only."""
    assert x.dtype == torch.float64
    a = x.abs()
    assert torch.isfinite(x).all() and ((a == 0) | ((a >= 2.0 ** -126) & (a < 2.0 ** 127))).all()
    bits = x.contiguous().view(torch.int64)
    drop = 52 - 7                                  # fp64 keeps 52 fraction bits, bf16 7
    lsb = (bits >> drop) & 1
    out = (bits + (_mask(drop - 1) + lsb)) & ~_mask(drop)
    return out.view(torch.float64)


def bf16_brackets(x: torch.Tensor):
    """(toward zero, away from zero, midpoint) of the two bf16 values around each fp64 x (fp64)."""
    assert x.dtype == torch.float64
    bits = x.abs().contiguous().view(torch.int64)
    drop = 52 - 7
    low = bits & ~_mask(drop)
    sign = torch.where(x < 0, -1.0, 1.0).double()
    down = low.view(torch.float64)
    up = (low + (1 << drop)).view(torch.float64)
    mid = (low | (1 << (drop - 1))).view(torch.float64)
    return sign * down, sign * up, sign * mid


def assert_once_rounded(got: torch.Tensor, ref: torch.Tensor, band, what: str = ''):
    """`got` (bf16) must be rne_bf16(ref) (ref fp64, the exact result).  `band` (scalar or per element)
    bounds how far the fp32 value the kernel rounded may lie from ref: then `got` may be the RNE of any
    value in [ref - band, ref + band] -- rounding is monotone, so any bf16 value from rne(ref - band) to
    rne(ref + band).  An element is "in the band" when those two differ (a rounding midpoint lies inside);
    everywhere else exactly one value is right.  Returns (in band, total); both are in the failure
    message."""
    assert got.dtype == torch.bfloat16 and ref.dtype == torch.float64 and got.shape == ref.shape
    got = got.detach().double().cpu().reshape(-1)
    ref = ref.detach().cpu().reshape(-1)
    band = torch.as_tensor(band, dtype=torch.float64).cpu()
    band = band.reshape(-1) if band.dim() else band.expand_as(ref)
    assert (band >= 0).all()
    want = rne_bf16(ref)
    low, high = rne_bf16(ref - band), rne_bf16(ref + band)
    near = low != high
    ok = torch.where(near, (got >= low) & (got <= high), got == want)
    n_band, total = int(near.sum()), ref.numel()
    if not bool(ok.all()):
        i = int((~ok).nonzero()[0])
        raise AssertionError('{}: {} of {} elements not rounded once from the reference (first: got {!r}, '
                             'reference {!r}, RNE {!r}, band {!r}); {} elements ({:.3%}) in the band'.format(
                                 what, int((~ok).sum()), total, got[i].item(), ref[i].item(), want[i].item(),
                                 band[i].item(), n_band, n_band / max(total, 1)))
    return n_band, total


# Split-bf16 error of one product a.b (fp32 operands).  With RNE to bf16's 8 significant bits,
# |x - hi| <= 2^-8 |x| and lo = RNE(x - hi) is off by <= 2^-8 |x - hi| ... more sharply, by half an
# ulp of a value below 2^(e-8) when 2^e <= |x|: <= 2^-17 |x|.  With x = hi + lo + e_x,
#   a.b - (hi_a hi_b + hi_a lo_b + lo_a hi_b) = lo_a lo_b + (hi_a + lo_a) e_b + e_a (hi_b + lo_b) + e_a e_b
# and |lo_a lo_b| <= 2^-16 |a||b|, each cross term <= (1 + 2^-8) 2^-17 |a||b|: in all
# SPLIT_PRODUCT = 2^-15 (1 + 2^-7) per product: DESIGN section 3 ("Split error per product"), where
# 1.98 x 2^-16 is measured on operands next to bf16 midpoints.  Accumulation: the three products of each of the K terms are added in fp32 in some order, n
# = 3K additions of terms whose magnitudes sum to <= (1 + 2^-7) sum_k |a_k||b_k|; the worst case of
# any order is gamma_n = n u / (1 - n u), u = 2^-24, of that sum.
SPLIT_PRODUCT = 2.0 ** -15 * (1 + 2.0 ** -7)


def split_coefficient(k: int, extra_terms: int = 0) -> float:
    """c_K of `split_bound`: per-product split error plus worst-case fp32 accumulation of 3K products
    (and `extra_terms` more additions: bias, the K extension's products)."""
    n = 3 * k + extra_terms
    u = 2.0 ** -24
    return SPLIT_PRODUCT + (1 + 2.0 ** -7) * n * u / (1 - n * u)


def split_bound(mag: torch.Tensor, k: int, extra_terms: int = 0) -> torch.Tensor:
    """Per-element bound on |got - exact| of a split-bf16 contraction of length k: c_K sum_k |a_k||b_k|,
    `mag` the fp64 sum of |a_k||b_k| per element."""
    return split_coefficient(k, extra_terms) * mag


def fp32_sum_bound(mag: torch.Tensor, n: int) -> torch.Tensor:
    """Worst-case error of n fp32 additions (or fmas) of terms whose magnitudes sum to `mag`, plus the
    rounding of every exact product: gamma_(n + 1)."""
    u = 2.0 ** -24
    return (n + 1) * u / (1 - (n + 1) * u) * mag



def fp32_tree_bound(mag: torch.Tensor, depth) -> torch.Tensor:
    """Error of an fp32 sum in which every term passes through at most `depth` roundings (additions or
    fmas on its way to the result, its own product's rounding counted as one): gamma_depth * mag, `mag`
    the sum of the terms' magnitudes.  The caller states the depth from the kernel's summation
    structure (serial steps per lane, levels of the butterfly, partial sums); fp32_sum_bound is the
    any-order form, for short serial chains.  `depth`: an int, or a tensor that broadcasts against `mag`
    (rows of different lengths)."""
    assert float(torch.as_tensor(depth).min()) >= 0
    u = 2.0 ** -24
    return depth * u / (1 - depth * u) * mag


def eval_bound(value: torch.Tensor, ulps: float, arg=None) -> torch.Tensor:
    """Error of one device function evaluation: `ulps` u |value|, plus |arg| u |value| when the function
    is an exponential that scales its argument first (__expf(x) = v_exp_f32(x log2e): the product's
    rounding moves the result by |x| u relative)."""
    u = 2.0 ** -24
    out = ulps * u * value.abs()
    if arg is not None:
        out = out + arg.abs() * u * value.abs()
    return out


def assert_within(got: torch.Tensor, ref64: torch.Tensor, bound: torch.Tensor, what: str) -> float:
    """|got - ref64| <= bound for every element (exact equality where bound == 0).  Prints one
    `[contract]` line (worst ratio err / bound; share of elements below 1e-3 max|ref|), fails naming the
    worst element, returns the worst ratio."""
    assert ref64.dtype == torch.float64 and got.shape == ref64.shape, (what, got.shape, ref64.shape)
    got = got.detach().double().cpu().reshape(-1)
    ref = ref64.detach().cpu().reshape(-1)
    bound = torch.as_tensor(bound, dtype=torch.float64).cpu()
    bound = bound.expand(ref64.shape).reshape(-1) if bound.dim() else bound.expand_as(ref)
    assert ref.numel() > 0 and torch.isfinite(ref).all() and (bound >= 0).all(), what
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float('inf')))
    zero = bound == 0
    ratio = torch.where(zero, torch.where(err == 0, 0.0, float('inf')).double(), err / bound.clamp_min(1e-300))
    worst = float(ratio.max())
    share = float((ref.abs() < 1e-3 * ref.abs().max()).double().mean())
    print('[contract] {}: worst ratio {:.3f}, share of elements below 1e-3 max|ref| {:.1%}'.format(
        what, worst, share))
    if not worst <= 1.0:
        i = int(ratio.argmax())
        raise AssertionError('{}: element {} of {} is off its bound: got {!r}, reference {!r}, |err| {:.3e}, '
                             'bound {:.3e} (ratio {:.3f}); {} elements off'.format(
                                 what, i, ref.numel(), got[i].item(), ref[i].item(), err[i].item(),
                                 bound[i].item(), worst, int((ratio > 1).sum())))
    return worst
