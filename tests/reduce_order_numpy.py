"""The summation order of the library's two-stage reductions (csrc/qmg_batch.hip: batches, and the single-vector entry points as a batch of one), emulated in numpy, and inputs on which
numpy reproduces every device operation exactly, so that the emulation must match the device BIT FOR BIT.

The documented order of one output value over n elements read W at a time (W = 2 for complex<float> at even n on aligned arrays, else 1):
  1. grid g = min(max(ceil((n / W) / 256), 1), 1024) blocks of 256 threads; thread t of the grid takes the packs t, t + 256 g, ... in order and
     for each pack its W elements in order, adding the element's terms to its accumulator with one fused multiply-add each
     (dot: ax bx, ay by for the real part; ax by, -ay bx for the imaginary part; norm: ax ax, ay ay; difference norm: dx dx, dy dy);
  2. the 64 lanes of a wavefront by the xor tree, partner lane ^ 1, ^ 2, ^ 4, ^ 8, ^ 16, ^ 32: after level s every lane holds the sum of its
     group of 2^(s+1) lanes, each level adding the two halves' sums (a + b = b + a bit for bit, so every lane holds lane 0's bits);
  3. the block's four wavefronts in index order: ((w0 + w1) + w2) + w3;
  4. second stage, one block of 256 threads per output: thread t adds the partials t, t + 256, ... in order, then steps 2 and 3 again.

Inputs: each real number is m 2^e with an integer |m| < 2^bits and e spread over [-30, 30].  With bits <= 26 every product of two of them is
exact in a double, so the device's fma(a, b, v) is numpy's v + a * b: one rounding of the same exact sum.  The sums themselves round at
every step (the terms' exponents span 120 binades), so another order gives other last bits: test_host_reduce_order.py measures how often.
"""
import numpy as np

BLOCK, WAVE, MAX_BLOCKS = 256, 64, 1024


def values(rng, shape, bits, exps=None):
    """(m 2^(e - bits), e): integer mantissas below 2^bits, exponents e in [-30, 30] (or the ones given)"""
    m = rng.integers(-(2 ** bits) + 1, 2 ** bits, size=shape).astype(np.float64)
    e = rng.integers(-30, 31, size=shape) if exps is None else exps
    return np.ldexp(m, e - bits), e


def cvalues(rng, shape, bits, like=None):
    """complex numbers of such parts; like = (re exponents, im exponents): share them (differences of two such numbers are exact)"""
    re, er = values(rng, shape, bits, None if like is None else like[0])
    im, ei = values(rng, shape, bits, None if like is None else like[1])
    return re + 1j * im, (er, ei)


def make_cancelling(rng, x, y, n):
    """Rewrites elements n // 2 ... 2 (n // 2) - 1 of x and y (last axis; the same shuffle for every leading index) so that element h + i
    repeats element pi(i) of the first half with y negated: the terms of <x, y> cancel in exact arithmetic (an odd n keeps its last
    element), and what a floating-point sum returns is its rounding errors -- which depend on the order in nearly every bit."""
    h = n // 2
    pi = rng.permutation(h)
    x[..., h:2 * h] = x[..., :h][..., pi]
    y[..., h:2 * h] = -y[..., :h][..., pi]


def grid_blocks(n, W=1):
    return int(min(max((n // W + BLOCK - 1) // BLOCK, 1), MAX_BLOCKS))


def _tree(v):
    """the xor tree over the last axis (64 lanes); returns lane 0"""
    lanes = np.arange(WAVE)
    for s in range(6):
        v = v + v[..., lanes ^ (1 << s)]
    return v[..., 0]


def _block(v):
    """(..., 256) thread values -> the block's sum: tree per wavefront, wavefronts in index order"""
    w = _tree(v.reshape(v.shape[:-1] + (BLOCK // WAVE, WAVE)))
    r = w[..., 0]
    for i in range(1, BLOCK // WAVE):
        r = r + w[..., i]
    return r


def device_sum(terms, n, W=1):
    """terms: arrays (..., n); element e contributes terms[0][..., e], terms[1][..., e], ... in that order.  The device's result, (...)."""
    lead = terms[0].shape[:-1]
    g = grid_blocks(n, W)
    T, packs = g * BLOCK, n // W
    acc = np.zeros(lead + (T,))
    for first in range(0, packs, T):
        cnt = min(T, packs - first)
        a = acc[..., :cnt]
        for w in range(W):
            e = slice(first * W + w, (first + cnt) * W + w, W)
            for t in terms:
                a = a + t[..., e]
        acc[..., :cnt] = a
    part = _block(acc.reshape(lead + (g, BLOCK)))          # (..., g): the partials of the first stage
    t = np.zeros(lead + (BLOCK,))
    for first in range(0, g, BLOCK):
        seg = part[..., first:first + BLOCK]
        t[..., :seg.shape[-1]] = t[..., :seg.shape[-1]] + seg
    return _block(t)


def serial_sum(terms, n):
    """the same terms added one after the other in element order: ANOTHER order, for the host test"""
    inter = np.stack(terms, axis=-1).reshape(terms[0].shape[:-1] + (len(terms) * n,))
    return np.cumsum(inter, axis=-1)[..., -1]


def dot_terms(x, y):
    """<x, y> = sum conj(x) y: (terms of the real part, terms of the imaginary part)"""
    return (x.real * y.real, x.imag * y.imag), (x.real * y.imag, -x.imag * y.real)


def norm_terms(x):
    return (x.real * x.real, x.imag * x.imag)


def diff_terms(x, y):
    d = x - y
    return (d.real * d.real, d.imag * d.imag)


def complex_sum(re_terms, im_terms, n, W=1, how=device_sum):
    args = (n, W) if how is device_sum else (n,)
    return how(re_terms, *args) + 1j * how(im_terms, *args)
