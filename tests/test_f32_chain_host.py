"""CPU: tests/f32_chain_ref.py's float32 fused multiply-add against exact rational arithmetic, and the chain restatement against a scalar
loop of it -- the yardstick of the exact-f32 GEMM's bit-pattern test must itself be proven."""
from fractions import Fraction

import numpy as np

from tests import f32_chain_ref as FR

F32_MIN_NORMAL = 2.0 ** -126


def _round_f32(q):
    """Round a Fraction inside the normal float32 range to the nearest float32, ties to even, in integer arithmetic."""
    if q == 0:
        return np.float32(0.0)
    sign = -1 if q < 0 else 1
    q = abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1                                                  # 2^e <= q < 2^(e + 1)
    assert -126 <= e <= 127
    scaled = q / Fraction(2) ** (e - 23)                        # in [2^23, 2^24): the unit is one ulp
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    return np.float32(sign * float(n) * 2.0 ** (e - 23))      # n <= 2^24 and the power are exact in float64, the product is a float32


def _triples():
    rng = np.random.default_rng(7)
    n = 9000
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
    out = [(a, b, c)]
    # cancellation: c = -fl32(a b), the fma returns the product's own rounding error
    out.append((a, b, (-(a.astype(np.float64) * b.astype(np.float64))).astype(np.float32)))
    # adversarial for double rounding: a b + c a hair off a float32 rounding tie, beyond float64's 53 bits.  a b = (1 + 2^-12)^2 =
    # 1 + 2^-11 + 2^-24 sits exactly on the tie between two float32 neighbours near 1; c is far smaller than the last float64 bit of the sum
    m = 1500
    x = np.full(m, 1 + 2.0 ** -12, np.float32)
    tiny = (np.float32(2.0) ** -rng.integers(60, 100, m).astype(np.float32)).astype(np.float32) * np.where(rng.random(m) < 0.5, -1, 1).astype(np.float32)
    out.append((x, x, tiny))
    out.append((x, -x, tiny))
    # ties that are exact (c = 0, and c a float32 that keeps the tie): must go to even
    out.append((x, x, np.zeros(m, np.float32)))
    out.append((x, x, np.full(m, 4.0, np.float32)))
    # a product with all 48 bits in use, p = (1 + 2^-23)(1 - 2^-24), against a small c and against c = -1 (nearly total cancellation)
    y = np.full(m, 1 + 2.0 ** -23, np.float32)
    z = np.full(m, 1 - 2.0 ** -24, np.float32)
    out.append((y, z, (rng.standard_normal(m) * 2.0 ** -30).astype(np.float32)))
    out.append((y, z, np.full(m, -1.0, np.float32)))
    # large against small: the product dwarfs c and the reverse
    out.append((a[:m], b[:m], (c[:m] * np.float32(2.0 ** 40)).astype(np.float32)))
    out.append((a[:m], b[:m], (c[:m] * np.float32(2.0 ** -40)).astype(np.float32)))
    return out


def test_fma32_equals_exact_rational_rounding():
    """>= 10^4 random and adversarial triples, operands, products and results in the normal range (results that cancel to less than
    2^-126, zero apart, are skipped and counted)."""
    checked = skipped = 0
    for a, b, c in _triples():
        got = FR.fma32(a, b, c)
        for ai, bi, ci, gi in zip(a.tolist(), b.tolist(), c.tolist(), got.tolist()):
            exact = Fraction(ai) * Fraction(bi) + Fraction(ci)
            if exact != 0 and abs(exact) < Fraction(F32_MIN_NORMAL):
                skipped += 1
                continue
            want = _round_f32(exact)
            assert np.float32(gi).view(np.uint32) == want.view(np.uint32) or (exact == 0 and gi == 0.0), (ai, bi, ci, gi, float(want))
            checked += 1
    assert checked >= 10000 and skipped < 100, (checked, skipped)


def test_double_rounding_cases_differ_from_the_naive_form():
    """The adversarial triples do what they are for: float32(float64(a b) + c) -- two roundings -- gets some of them wrong."""
    wrong = 0
    for a, b, c in _triples()[2:4]:
        naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
        wrong += int((naive.view(np.uint32) != FR.fma32(a, b, c).view(np.uint32)).sum())
    assert wrong > 100


def test_chain_product_is_the_scalar_chain():
    """chain_product against a scalar loop of fma32 and float32 additions, with chunks that do not divide K."""
    rng = np.random.default_rng(3)
    a = rng.standard_normal((5, 70)).astype(np.float32)
    b = rng.standard_normal((70, 3)).astype(np.float32)
    for chunk in (70, 32, 64):
        got = FR.chain_product(a, b, chunk)
        for i in range(5):
            for j in range(3):
                total = None
                for k0 in range(0, 70, chunk):
                    acc = np.float32(0)
                    for k in range(k0, min(70, k0 + chunk)):
                        acc = FR.fma32(a[i, k], b[k, j], acc)[()]
                    total = acc if total is None else np.float32(total + acc)
                assert got[i, j].view(np.uint32) == np.float32(total).view(np.uint32)
    # and it is not the float64 product rounded once: the chain's roundings are visible
    assert (FR.chain_product(a, b, 70) != (a.astype(np.float64) @ b.astype(np.float64)).astype(np.float32)).any()
