"""Host twin of tests/test_gpu_reduce_order.py: the inputs that test uses make the summation ORDER visible in the last bits.

The device test requires the bits of reduce_order_numpy.device_sum.  That proves the order only if another order gives other bits on the same
inputs, which this test measures: the plain serial sum of the same terms must differ from the device order in at least 90 % of the outputs
(shapes with n >= 63: a single element has one order).  It also checks what the emulation rests on: the products the device forms inside one
fused multiply-add are exact in a double, so numpy's multiply-then-add is that fused operation, and every term is summed exactly once.
"""
from fractions import Fraction

import numpy as np

import reduce_order_numpy as ro

SIZES = (63, 64, 65, 255, 256, 257, 1000, 262147)


def test_products_are_exact():
    rng = np.random.default_rng(1)
    for bits in (23, 25):
        a, _ = ro.values(rng, 2000, bits)
        b, _ = ro.values(rng, 2000, bits)
        for u, v in zip(a[:200], b[:200]):
            assert Fraction(float(u)) * Fraction(float(v)) == Fraction(float(u * v))
        x, exps = ro.cvalues(rng, 500, bits)
        y, _ = ro.cvalues(rng, 500, bits, exps)
        d = x - y                                       # shared exponents: the difference is exact and has bits + 1 bits
        for u, v, w in zip(x.real[:200], y.real[:200], d.real[:200]):
            assert Fraction(float(u)) - Fraction(float(v)) == Fraction(float(w))
            assert Fraction(float(w)) ** 2 == Fraction(float(w * w))


def test_float_storage_is_exact():
    x, _ = ro.cvalues(np.random.default_rng(2), 4096, 23)
    assert np.array_equal(x.astype(np.complex64).astype(np.complex128), x)


def test_emulation_sums_every_term_once():
    rng = np.random.default_rng(3)
    for n, W in ((1, 1), (65, 1), (1000, 2), (257, 1), (2 * 262144 + 6, 2)):
        t = np.ldexp(rng.integers(-99, 100, size=n).astype(np.float64), 0)      # small integers: every order is exact
        assert ro.device_sum((t,), n, W) == t.sum()
        assert ro.grid_blocks(n, W) == min(max(-(-(n // W) // 256), 1), 1024)


def test_another_order_changes_the_bits():
    """Per shape 16 dots (cancelling inputs, as the device test draws them) and one norm and one difference norm: the device test's outputs
    are dots in that proportion or more.  Sums of positive terms (the norms) are the less sensitive kind: two orders of some 60 additions
    agree in every bit about one time in four at n near 64, whatever the inputs, because both land within a unit or two in the last place of
    the truth.  Figures of this test: 605 of 608 dot outputs differ, 32 of 38 norm outputs, 98.6 % together."""
    rng = np.random.default_rng(4)
    differ = total = 0
    for n in SIZES:
        nj = 16
        for bits, W in ((25, 1), (23, 1), (23, 2)):
            if W == 2 and n % 2:
                continue
            xs, _ = ro.cvalues(rng, (nj, n), bits)
            y, _ = ro.cvalues(rng, (1, n), bits)
            ro.make_cancelling(rng, xs, y, n)
            x, exps = ro.cvalues(rng, (1, n), bits)
            z, _ = ro.cvalues(rng, (1, n), bits, exps)
            for re_t, im_t in (ro.dot_terms(xs, y), (ro.norm_terms(x), ro.diff_terms(x, z))):
                dev = ro.complex_sum(re_t, im_t, n, W)
                ser = ro.complex_sum(re_t, im_t, n, how=ro.serial_sum)
                differ += int(np.sum(dev.real != ser.real) + np.sum(dev.imag != ser.imag))
                total += 2 * dev.size
                # both are sums of the same terms: they agree to rounding
                scale = np.sum(np.abs(np.stack(re_t)), axis=(0, -1)) + np.sum(np.abs(np.stack(im_t)), axis=(0, -1))
                assert np.all(np.abs(dev - ser) <= 1e-12 * scale)
    assert differ >= 0.9 * total, (differ, total)
