"""Independent statement of the batch vector operations of csrc/qmg_batch.hip in np.clongdouble arithmetic.

A batch is `nrhs` vectors of `n` elements at a common `stride`; every function here takes and returns the vectors of ONE system (the
route tests of test_gpu_batch_routes.py cut the systems out of the batch themselves and hold everything outside the active systems to
its initial bytes).  Inputs are complex128 arrays that already hold what the device holds: for complex<float> storage they have been
rounded with r32 first.  Nothing here shares code with the kernels or the oracle.  (The single-vector BLAS-1 and reductions of the C ABI are these
same kernels at nrhs = 1.)

Next to each elementwise result comes the term-magnitude sum S = |out0| + sum |c| |x| per element and the number of terms of the sum, the
scale and length of the bound the kernels are held to (elementwise_bound: the form of transfer_numpy.elementwise_bound).
"""
import numpy as np

CLD = np.clongdouble
LD = np.longdouble

ZERO, COPY, CAX, CAXPY, CXPY, CAXPBYZ, CAXY, CXPAY, CAXPBY, CXPYZ = range(10)      # qmg_batch_op
NORM2, DOT, DIFFNORM2 = range(3)                      # qmg_batch_red


def r32(a):
    """round to complex<float> and widen back: what a complex<float> device array holds"""
    return np.ascontiguousarray(a, dtype=np.complex64).astype(np.complex128)


def _ld(v):
    return np.asarray(v).astype(CLD)


def _mag(v):
    return np.abs(_ld(v))


def blas(op, a, b, x, y, z):
    """(z', S, terms) of one qmg_batch_blas_t op: z' = 0 | x | a z | z + a x | z + x | a x + b y | a x | x + a z | a x + b z | x + y"""
    a, b = CLD(a), CLD(b)
    if op == ZERO:
        return np.zeros(len(z), dtype=CLD), np.zeros(len(z), dtype=LD), 0
    if op == COPY:
        return _ld(x), _mag(x), 0
    if op == CAX:
        return a * _ld(z), abs(a) * _mag(z), 1
    if op == CAXPY:
        return _ld(z) + a * _ld(x), _mag(z) + abs(a) * _mag(x), 1
    if op == CXPY:
        return _ld(z) + _ld(x), _mag(z) + _mag(x), 1
    if op == CAXPBYZ:
        return a * _ld(x) + b * _ld(y), abs(a) * _mag(x) + abs(b) * _mag(y), 2
    if op == CAXY:
        return a * _ld(x), abs(a) * _mag(x), 1
    if op == CXPAY:
        return _ld(x) + a * _ld(z), _mag(x) + abs(a) * _mag(z), 1
    if op == CAXPBY:
        return a * _ld(x) + b * _ld(z), abs(a) * _mag(x) + abs(b) * _mag(z), 2
    assert op == CXPYZ
    return _ld(x) + _ld(y), _mag(x) + _mag(y), 1


PASS_SETS = 8    # vector sets per pass over y: the entry points take more in several passes, and y is STORED between them


def multi_axpy(coeffs, xs, y, narrow=False):
    """(y + sum_j c_j x_j, S, terms, P).  The zero-coefficient rule: a vector whose coefficient is zero is NOT READ -- its slot may hold
    anything (NaN, Inf) -- so it adds neither to the sum nor to S.
    narrow (complex<float> storage) with more than PASS_SETS vector sets: y is rounded to complex<float> behind every pass of PASS_SETS, as
    the passes store it (the way gcr_update rounds w before it enters r); P is the sum of the magnitudes of those stored partial results,
    the scale of the float rounding by which a kernel's partial may differ from this one's (elementwise_bound's `slack`).  P = 0 for one pass."""
    out, S, terms, P = _ld(y), _mag(y), 0, np.zeros(len(y), dtype=LD)
    for j, (c, x) in enumerate(zip(coeffs, xs)):
        if narrow and j and j % PASS_SETS == 0:
            out = _ld(r32(out.astype(np.complex128)))
            P = P + np.abs(out)
        if c == 0:
            continue
        c = CLD(c)
        out = out + c * _ld(x)
        S = S + abs(c) * _mag(x)
        terms += 1
    return out, S, terms, P


def gcr_update(coeffs, ws, w, a, r, narrow):
    """The flexible GCR's update: w' = w + sum_j c_j W_j ; r' = r + a w' ; z_next = r'.  narrow (complex<float> storage): w' is rounded
    to complex<float> before it enters r, as a separate pass over the stored w would read it.
    Returns (w', S_w, terms_w, P_w, r', S_r, terms_r, r_slack): S_r = |r| + |a| S_w counts r's sum down to the W_j; P_w as multi_axpy's P;
    r_slack = |a| (|w'| + P_w) is the scale of the float roundings a kernel's w may differ by (narrow only; elementwise_bound's `slack`)."""
    a = CLD(a)
    wn, Sw, tw, Pw = multi_axpy(coeffs, ws, w, narrow)
    wr = _ld(r32(wn.astype(np.complex128))) if narrow else wn
    rn = _ld(r) + a * wr
    return wn, Sw, tw, Pw, rn, _mag(r) + abs(a) * Sw, tw + 1, abs(a) * (np.abs(wn) + Pw)


def cgm_update(a, z, c, x, p, r):
    """One (system, shift) pair of multi-shift CG, a, z, c real: x' = x + a p ; p' = z r + c p.  Returns (x', S_x, 1, p', S_p, 2)."""
    a, z, c = LD(a), LD(z), LD(c)
    return (_ld(x) + a * _ld(p), _mag(x) + abs(a) * _mag(p), 1,
            z * _ld(r) + c * _ld(p), abs(z) * _mag(r) + abs(c) * _mag(p), 2)


def norm2(x):
    return LD(np.sum(_ld(x).real ** 2 + _ld(x).imag ** 2))


def dot(x, y):
    """<x, y> = sum conj(x_i) y_i"""
    return CLD(np.sum(np.conj(_ld(x)) * _ld(y)))


def reduce(op, x, y):
    """(value, scale) of one qmg_batch_reduce_t op; scale = sqrt(|x|^2 |y|^2) (|x|^2 for the norm): what the reduction tolerance multiplies"""
    if op == NORM2:
        return CLD(norm2(x)), norm2(x)
    scale = np.sqrt(norm2(x) * norm2(y))
    if op == DOT:
        return dot(x, y), scale
    assert op == DIFFNORM2
    return CLD(norm2(_ld(x) - _ld(y))), scale


def multidot(xs, y):
    """([<x_j, y>], [scale_j])"""
    return [dot(x, y) for x in xs], [np.sqrt(norm2(x) * norm2(y)) for x in xs]


def mr_dots(r, p):
    """the MR slot of one system: (<p, r>, <p, p>) and their scales"""
    return dot(p, r), norm2(p), np.sqrt(norm2(p) * norm2(r)), norm2(p)


def mr_alpha(omega, pr, pp):
    """alpha = omega <p,r> / <p,p>, 0 when <p,p> = 0"""
    return CLD(0) if pp == 0 else CLD(omega) * CLD(pr) / LD(pp)


def mr_update(alpha, x, r_in, p, xset):
    """x' = x + alpha r_in (xset: alpha r_in, x is not read) ; r_out = r_in - alpha p.  Returns (x', S_x, 1, r_out, S_r, 1).  r_out aliasing
    r_in is the same statement: x' uses r_in's old value."""
    alpha = CLD(alpha)
    x0 = np.zeros(len(r_in), dtype=CLD) if xset else _ld(x)
    return (x0 + alpha * _ld(r_in), np.abs(x0) + abs(alpha) * _mag(r_in), 1,
            _ld(r_in) - alpha * _ld(p), _mag(r_in) + abs(alpha) * _mag(p), 1)


def elementwise_bound(terms, S, want=None, slack=None):
    """|got - want| <= (terms + 1) 2^-50 S for fp64 results; complex<float> results (want given) add one rounding of the result with a
    factor 2, 2^-23 |want|; slack adds 2^-23 slack: |a| |w| for r and z_next of a complex<float> GCR update, and the stored partial
    results of a complex<float> sum that takes several passes (multi_axpy's P) -- every value a kernel stores in complex<float> on the way
    may be the neighbouring float of the reference's.  (The standard summation bound is terms 2^-53 S; 8x over it leaves room for FMA
    contraction and the four real products of a complex one.)"""
    b = (terms + 1) * LD(2.0) ** -50 * S
    if want is not None:
        b = b + LD(2.0) ** -23 * np.abs(want)
    if slack is not None:
        b = b + LD(2.0) ** -23 * slack
    return b


RTOL_RED = 1e-12    # reductions: |got - want| <= RTOL_RED * scale (test_gpu_parity.py, test_gpu_reductions.py)
