"""CPU self-tests of tests/exact.py: the rounding reference, the bracket band and the generators' 2^24 rule."""
import pytest
import torch

import exact as X


def test_rne_bf16_is_torchs_rounding_on_fp32_values():
    gen = torch.Generator().manual_seed(0)
    x = torch.randn([1 << 16], generator=gen) * torch.pow(2.0, torch.randint(-60, 60, [1 << 16], generator=gen).float())
    ties = (torch.randint(-2 ** 15, 2 ** 15, [4096], generator=gen) * 2 + 1).float() * 2.0 ** -9   # exact ties
    for v in (x, ties, torch.tensor([0.0, -0.0, 1.0, 2.0 ** -126, 1.5e38, -1.5e38])):
        assert torch.equal(X.rne_bf16(v.double()), v.bfloat16().double())


def test_rne_bf16_rounds_fp64_once():
    """b + half an ulp + a little (fp64) rounds up; through fp32 the little is lost, the value becomes a
    tie and goes to the even b.  And the mirror case."""
    ulp = 2.0 ** -7
    for b, delta in ((1.0, 2.0 ** -40), (1.0 + 2 * ulp, 2.0 ** -35), (1.0 + ulp, -2.0 ** -40), (3.0 + 2 * ulp * 2, 2.0 ** -38)):
        e = 2.0 ** (int(torch.tensor(b).log2().floor()))
        x = torch.tensor([b + 0.5 * ulp * e + delta * e], dtype=torch.float64)
        direct = X.rne_bf16(x).item()
        twice = x.float().bfloat16().double().item()
        assert direct != twice, (b, delta)
        assert direct == (b + ulp * e if delta > 0 else b)
    # the same on integer values of the bf16 kernels' range
    x = torch.tensor([257.0 + 2.0 ** -30, -257.0 - 2.0 ** -30, 259.0 - 2.0 ** -30], dtype=torch.float64)
    assert X.rne_bf16(x).tolist() == [258.0, -258.0, 258.0]
    assert x.float().bfloat16().double().tolist() == [256.0, -256.0, 260.0]


def test_ties_go_to_even():
    x = torch.tensor([257.0, 259.0, 261.0, -257.0, -259.0, 514.0, 518.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8],
                     dtype=torch.float64)
    assert X.rne_bf16(x).tolist() == [256.0, 260.0, 260.0, -256.0, -260.0, 512.0, 520.0, 1.0, 1.0 + 2.0 ** -6]


def test_brackets_and_the_band():
    x = torch.tensor([257.0, 257.5, -300.25, 1.0], dtype=torch.float64)
    down, up, mid = X.bf16_brackets(x)
    assert down.tolist() == [256.0, 256.0, -300.0, 1.0]
    assert up.tolist() == [258.0, 258.0, -302.0, 1.0 + 2.0 ** -7]
    assert mid.tolist() == [257.0, 257.0, -301.0, 1.0 + 2.0 ** -8]
    got = torch.tensor([258.0, 258.0, -300.0, 1.0]).bfloat16()
    # 257 (a tie) must go to 256 without a band; with one, either neighbour is accepted
    with pytest.raises(AssertionError):
        X.assert_once_rounded(got, x, 0.0)
    assert X.assert_once_rounded(got, x, 0.5) == (3, 4)          # 1.0 lies 2^-8 from its midpoint
    with pytest.raises(AssertionError):           # 257.5 is outside a band of 0.25 and rounds to 258
        X.assert_once_rounded(torch.tensor([256.0, 256.0, -300.0, 1.0]).bfloat16(), x, 0.25)


def test_generators_keep_the_exact_rule_at_their_largest_k():
    gen = torch.Generator().manual_seed(1)
    for k, other in ((32, 256), (1024, 8), (4096, 3), (8192, 1)):
        bound = X.two_part_bound(k, other, extra=2 ** 12)
        a = X.two_part_ints(gen, [64, k], bound)
        b = X.bf16_ints(gen, [k, 8], other)
        hi = a.bfloat16().float()
        lo = (a - hi).bfloat16().float()
        worst = (hi.double().abs() + lo.double().abs()) @ b.double().abs()
        assert worst.max().item() < X.EXACT_LIMIT - 2 ** 12
        assert torch.equal(hi + lo, a)
    with pytest.raises(AssertionError):
        X.fits_fp32(2.0 ** 24)
    assert X.split_coefficient(64) < 2.0 ** -14 and X.split_coefficient(1024) > 3 * 1024 * 2.0 ** -24
