"""Multi-shift CG on the GPU: the fused update kernel (qmg_batch_cgm_update_t), the solver core (bcg_m_core / minv_vector_cg_m, include/qmg/
krylov.hpp), the mass-scan helpers (Staggered2D / GaugedLaplace2D::solve_masses, include/qmg/operators.hpp) and the n20 driver's mass list.

Yardsticks, none of them the code under test: the element-wise batch kernels that every solver already uses (qmg_batch_blas_t) for the
kernel, BIT FOR BIT; numpy (tests/coordspace.py and a numpy twin of the whole procedure written here) and the single-shift CG
(minv_vector_cg, pinned in tests/test_gpu_krylov.py) for the solver; the reference's critical_mass.txt for the driver."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import coordspace as cs

qmg = importlib.import_module("quantum-mg_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVERS = os.path.join(ROOT, "quantum-mg_amd", "drivers")
INVALID = 1


@pytest.fixture(scope="module", autouse=True)
def _device():
    qmg.build()
    subprocess.check_call(["make", "-C", DRIVERS, "-j4"], stdout=subprocess.DEVNULL)
    qmg.init(0)
    yield
    qmg.sync()


# ---------------------------------------------------------------- the kernel, bit for bit ----------------------------------------------------------------
def _rand(rng, count, dtype):
    return (rng.standard_normal(count) + 1j * rng.standard_normal(count)).astype(qmg.NP_DTYPE[dtype])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def cgm_case(dtype, K, S, n, mask, shift_masks, seed, pad=0, misalign=False):
    """The fused kernel and the unfused qmg_batch_blas_t sequence on copies of the same random data; returns nothing, asserts equal bits of
    every byte of every x[s] and p[s] (active, frozen and the padding between systems alike) and that r is untouched.
    misalign: every base pointer 8 bytes past a 16-byte boundary (complex<float>: the 8-byte access path)."""
    rng = np.random.default_rng(seed)
    stride = n + pad
    lead = 1 if misalign else 0
    total = lead + K * stride
    hr = _rand(rng, total, dtype)
    hx = [_rand(rng, total, dtype) for _ in range(S)]
    hp = [_rand(rng, total, dtype) for _ in range(S)]
    a, z, c = rng.standard_normal((S, K)), rng.standard_normal((S, K)), rng.standard_normal((S, K))
    r = qmg.DeviceArray.from_host(hr)
    xf, pf = [qmg.DeviceArray.from_host(v) for v in hx], [qmg.DeviceArray.from_host(v) for v in hp]
    xu, pu = [qmg.DeviceArray.from_host(v) for v in hx], [qmg.DeviceArray.from_host(v) for v in hp]
    at = lambda d: d.offset(lead)
    qmg.batch_cgm_update_t(dtype, [at(v) for v in xf], [at(v) for v in pf], a, z, c, shift_masks, at(r), n, K, stride, mask)
    for s in range(S):
        act = mask & shift_masks[s]
        qmg.batch_blas_t(dtype, qmg.BOP_CAXPY, at(xu[s]), n, K, stride, act, a=a[s] + 0j, x=at(pu[s]))
        qmg.batch_blas_t(dtype, qmg.BOP_CAXPBYZ, at(pu[s]), n, K, stride, act, a=z[s] + 0j, b=c[s] + 0j, x=at(r), y=at(pu[s]))
    assert np.array_equal(_bits(r.to_host()), _bits(hr))
    for s in range(S):
        gx, gp, wx, wp = xf[s].to_host(), pf[s].to_host(), xu[s].to_host(), pu[s].to_host()
        assert np.array_equal(_bits(gx), _bits(wx)), (s, "x")
        assert np.array_equal(_bits(gp), _bits(wp)), (s, "p")
        for k in range(K):   # a frozen (system, shift) pair comes back as it went in; an active one does not
            sl = slice(lead + k * stride, lead + k * stride + n)
            frozen = not ((mask & shift_masks[s]) >> k) & 1
            assert np.array_equal(_bits(gx[sl]), _bits(hx[s][sl])) == frozen, (s, k)
            assert np.array_equal(_bits(gp[sl]), _bits(hp[s][sl])) == frozen, (s, k)
    for d in [r] + xf + pf + xu + pu:
        d.free()


def _full(K):
    return (1 << K) - 1


@pytest.mark.parametrize("dtype", [qmg.C64, qmg.C32])
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("S", [1, 4, 8, 16])
def test_cgm_update_equals_the_unfused_passes_bit_for_bit(dtype, K, S):
    """n odd (complex<float>: the 8-byte path), n below one wavefront, n even with padded strides; every system and every shift active"""
    for i, (n, pad) in enumerate([(4097, 0), (37, 3), (6144, 2)]):
        cgm_case(dtype, K, S, n, _full(K), [_full(K)] * S, seed=100 * S + 10 * K + i, pad=pad)


@pytest.mark.parametrize("dtype", [qmg.C64, qmg.C32])
@pytest.mark.parametrize("S", [4, 8, 16])
def test_cgm_update_masks_and_frozen_shifts(dtype, S):
    """system masks with holes; a fully frozen shift (mask 0), shifts frozen for some systems only, a system whose every shift is frozen:
    what is frozen is neither read nor written (bitwise unchanged), the rest equals the unfused passes"""
    K = 8
    rng = np.random.default_rng(S)
    sm = [int(v) for v in rng.integers(1, 256, size=S)]
    sm[1] = 0                                  # shift 1: frozen for every system
    sm = [m & ~(1 << 5) for m in sm]           # system 5: every shift frozen
    sm[S - 1] = 0xFF
    for mask in (0xFF, 0b10110101, 0b00000010):
        cgm_case(dtype, K, S, 2050, mask, sm, seed=7 * S + mask, pad=6)
    cgm_case(dtype, 3, S, 1001, 0b101, [0b111, 0b001, 0b100, 0b110] * (S // 4), seed=S)


@pytest.mark.parametrize("dtype,n", [(qmg.C64, 1 << 20), (qmg.C32, 1 << 21)])
@pytest.mark.parametrize("K,S", [(1, 4), (3, 8)])
def test_cgm_update_on_vectors_of_16_mb(dtype, n, K, S):
    """16 MB per vector: the size from which k_bmulti_caxpy takes its long-vector form"""
    sm = [_full(K)] * S
    if K > 1:
        sm[2] = 0b010
    cgm_case(dtype, K, S, n, _full(K), sm, seed=n % 1000 + S)


def test_cgm_update_with_non_temporal_reads_of_r():
    """8 systems of 32 MB: the batch is past `blas_nt_mb`, r is streamed non-temporally"""
    cgm_case(qmg.C64, 8, 2, 1 << 21, 0xFF, [0xFF, 0x0F], seed=5)


@pytest.mark.parametrize("S", [1, 4, 8])
def test_cgm_update_on_misaligned_complex_float_vectors(S):
    """complex<float> base pointers 8 bytes past a 16-byte boundary (the other `_t` kernels take them through 8-byte accesses)"""
    cgm_case(qmg.C32, 3, S, 4096, 0b111, [0b111] * S, seed=S, misalign=True)
    cgm_case(qmg.C32, 3, S, 4096, 0b101, [0b011] * S, seed=S + 1, pad=1)      # odd stride


def test_cgm_update_invalid_arguments():
    K, S, n = 2, 3, 64
    r = qmg.DeviceArray.zeros(K * n)
    xs, ps = [qmg.DeviceArray.zeros(K * n) for _ in range(S)], [qmg.DeviceArray.zeros(K * n) for _ in range(S)]
    co = np.zeros((S, K))
    sm = [3] * S
    call = lambda **kw: qmg.batch_cgm_update_status(**dict(dict(dtype=qmg.C64, xs=xs, ps=ps, a=co, z=co, c=co, shift_masks=sm, r=r, n=n, nrhs=K, stride=n, mask=3), **kw))
    assert call() == 0
    assert call(ns=0) == INVALID and call(ns=-1) == INVALID and call(ns=17) == INVALID
    assert call(dtype=7) == INVALID
    assert call(nrhs=0) == INVALID and call(nrhs=17) == INVALID
    for name in ("xs", "ps", "a", "z", "c", "shift_masks"):
        assert call(**{name: None, "ns": S}) == INVALID, name
    assert call(r=None) == INVALID
    assert call(xs=[xs[0], None, xs[2]]) == INVALID and call(ps=[ps[0], ps[1], None]) == INVALID
    assert call(xs=[xs[0], r, xs[2]]) == INVALID and call(ps=[r, ps[1], ps[2]]) == INVALID          # x[s] / p[s] aliasing r
    assert call(xs=[xs[0], ps[1], xs[2]]) == INVALID and call(xs=[xs[0], xs[0], xs[2]]) == INVALID  # ... or one another
    assert call(mask=0) == 0 and call(shift_masks=[0] * S) == 0 and call(n=0) == 0                   # nothing to do is not an error
    for d in [r] + xs + ps:
        d.free()


# ---------------------------------------------------------------- the solver ----------------------------------------------------------------
EPS = 1e-10
SOLVER_CASES = [
    (32, "l32t32b60_heatbath.dat", "staggered", (0.04, 0.06, 0.08, 0.1)),
    (32, "l32t32b60_heatbath.dat", "staggered", (0.01, 0.04, 0.1, 0.5)),
    (32, "l32t32b60_heatbath.dat", "laplace", (0.001, 0.01, 0.1, 1.0)),
    (64, "l64t64b60_heatbath.dat", "staggered", (0.04, 0.06, 0.08, 0.1)),
    (64, "l64t64b60_heatbath.dat", "staggered", (0.01, 0.04, 0.1, 0.5)),
    (64, "l64t64b60_heatbath.dat", "laplace", (0.001, 0.01, 0.1, 1.0)),
]
_runs = {}


def parity_run(golden_dir, tmp_path_factory, L, fname, kind, vals):
    key = (L, kind, vals)
    if key not in _runs:
        tmp = str(tmp_path_factory.mktemp("multishift"))
        out = subprocess.run([os.path.join(DRIVERS, "multishift_parity"), str(L), os.path.join(golden_dir, fname), tmp, kind, ",".join(repr(v) for v in vals)],
                             cwd=DRIVERS, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
        rows = {m[0]: (int(m[1]), int(m[2]), int(m[3]), float(m[4])) for m in re.findall(r"\[KRYLOV\] (\w+) success (\d) iter (\d+) ops (\d+) rel_res ([-\d.e+]+)", out.stdout)}
        load = lambda name: np.fromfile(os.path.join(tmp, name + ".bin"), dtype=np.complex128)
        _runs[key] = (out.stdout, rows, {"b": load("b"), "x": [load("x_%d" % s) for s in range(len(vals))], "xsolo": [load("xsolo_%d" % s) for s in range(len(vals))]})
    return _runs[key]


def numpy_twin(L, Ux, Uy, kind, vals, b):
    """the whole procedure in numpy on grids: multi-shift CG (Jegerlehner's variables) on -H^2 with sigma = m^2, then x = m y - H y
    (staggered); on the m^2 = 0 gauged Laplace operator with sigma = m^2 (laplace).  Returns the solutions and their true residuals."""
    if kind == "staggered":
        H = lambda v: cs.staggered_apply(v, Ux, Uy, 0.0)
        A0, sig = (lambda v: -H(H(v))), [m * m for m in vals]
        full, post = (lambda v, m: cs.staggered_apply(v, Ux, Uy, m)), (lambda y, m: m * y - H(y))
    else:
        A0, sig = (lambda v: cs.laplace_apply(v, Ux, Uy, 0.0)), list(vals)
        full, post = (lambda v, s: cs.laplace_apply(v, Ux, Uy, s)), (lambda y, s: y)
    S = len(sig)
    base = int(np.argmin(sig))
    xs, ps, r = [np.zeros_like(b) for _ in sig], [b.copy() for _ in sig], b.copy()
    rs = np.vdot(r, r).real
    bn = np.sqrt(rs)
    zo, z, bo, al, live, it = np.ones(S), np.ones(S), 1.0, 0.0, [True] * S, 0
    while it < 5000 and live[base]:
        p = ps[base]
        Ap = A0(p) + sig[base] * p
        be = -rs / np.vdot(p, Ap).real
        zn, bes = z.copy(), np.zeros(S)
        for s in range(S):
            if live[s]:
                zn[s] = z[s] * zo[s] * bo / (be * al * (zo[s] - z[s]) + zo[s] * bo * (1.0 - (sig[s] - sig[base]) * be))
                bes[s] = be * zn[s] / z[s]
                xs[s] = xs[s] - bes[s] * ps[s]
        r = r + be * Ap
        rn = np.vdot(r, r).real
        for s in range(S):
            if live[s]:
                ps[s] = zn[s] * r + (rn / rs) * zn[s] * bes[s] / (z[s] * be) * ps[s]
        zo, z, bo, al, rs, it = np.where(live, z, zo), zn, be, rn / rs, rn, it + 1
        for s in range(S):
            if live[s] and abs(z[s]) * np.sqrt(rs) < EPS * bn:
                live[s] = False
    sols = [post(xs[s], vals[s]) for s in range(S)]
    return sols, [float(np.linalg.norm(b - full(sols[s], vals[s])) / bn) for s in range(S)], full


@pytest.mark.parametrize("L,fname,kind,vals", SOLVER_CASES)
def test_solve_masses_against_numpy_and_the_single_shift_cg(golden_dir, tmp_path_factory, L, fname, kind, vals):
    """Per shift: (i) converged; (ii) the TRUE residual |b - D(m_s) x_s| / |b| under the numpy operator at most 10x the true residual of the
    numpy twin of the whole procedure on the same b (the shifted residuals are never recomputed by the algorithm, so the bar comes from
    the twin, not from eps.  Twin, numpy reductions, on this b: 7.2e-11 .. 1.0e-10 over the 24 (fixture, shift) cases, so the bar is about 1e-9;
    measured on the MI355X: 7.4e-11 .. 1.0e-10, iteration counts equal to the solo runs' on 22 cases and one more on two, |x - x_solo| <= 6.6e-11);
    (iii) iter within 1 of minv_vector_cg alone on A + sigma_s to the same eps, the operator applies of the whole solve within 1 of the
    smallest shift's solo run; (iv) x_s within 1e-7 relative of the solo solution (the bar tests/test_gpu_krylov.py holds two solves to)."""
    stdout, rows, vec = parity_run(golden_dir, tmp_path_factory, L, fname, kind, vals)
    assert stdout.count("[QMG-ERROR]") == (1 if kind == "laplace" else 0)   # (laplace: the refused non-zero guess of the batch part)
    Ux, Uy = cs.phases_to_links(np.loadtxt(os.path.join(golden_dir, fname)), L, L)
    b = cs.eo_to_grid(vec["b"], L, L, 1)
    twin_x, twin_res, full = numpy_twin(L, Ux, Uy, kind, vals, b)
    base = int(np.argmin(vals))
    for s, v in enumerate(vals):
        ok, it, ops, rel = rows["cgm_%d" % s]
        sok, sit, sops, srel = rows["solo_%d" % s]
        x = cs.eo_to_grid(vec["x"][s], L, L, 1)
        true_res = float(np.linalg.norm(b - full(x, v)) / np.linalg.norm(b))
        print("%s L=%d %g: iter %d (solo %d) ops %d (solo %d) recurrence %.3e true %.3e twin true %.3e |x - x_solo| %.3e |x - x_twin| %.3e" % (
            kind, L, v, it, sit, ops, sops, rel, true_res, twin_res[s], cs.rel_l2(vec["x"][s], vec["xsolo"][s]), cs.rel_l2(x, twin_x[s])))
        assert ok == 1 and sok == 1 and rel < EPS, (s, rows)
        assert true_res <= 10.0 * twin_res[s], (s, true_res, twin_res[s])
        assert abs(it - sit) <= 1, (s, it, sit)
        assert cs.rel_l2(vec["x"][s], vec["xsolo"][s]) < 1e-7, s
    assert abs(rows["cgm_%d" % base][2] - rows["solo_%d" % base][2]) <= 1
    assert len({rows["cgm_%d" % s][2] for s in range(len(vals))}) == 1      # one solve: every shift reports the same operator applies


@pytest.mark.parametrize("L,fname,kind,vals", SOLVER_CASES[:3])
def test_solve_masses_leaves_the_operator_alone(golden_dir, tmp_path_factory, L, fname, kind, vals):
    """the object's shift and its apply_M output are the same bits before and after solve_masses"""
    stdout = parity_run(golden_dir, tmp_path_factory, L, fname, kind, vals)[0]
    assert "[STATE] shift_unchanged 1 apply_unchanged 1" in stdout


@pytest.mark.parametrize("L,fname", [(32, "l32t32b60_heatbath.dat"), (64, "l64t64b60_heatbath.dat")])
def test_batch_of_three_systems_by_four_shifts(golden_dir, tmp_path_factory, L, fname):
    """K = 3 x S = 4 in lock step against three batches of one, per (system, shift): iteration counts within 1, solutions within 1e-7
    relative (the bar drivers/facade_selftest.cpp holds bcg_core batches to: a batched apply may sum in another order).  With the middle
    right-hand side zero: that system returns zeros as converged, the others are what they are alone.  A non-zero guess is refused."""
    stdout = parity_run(golden_dir, tmp_path_factory, L, fname, "laplace", (0.001, 0.01, 0.1, 1.0))[0]
    for tag in ("BATCH", "BATCH0"):
        rows = re.findall(r"^\[%s\] rhs (\d) shift (\d) success (\d) iter (\d+) alone_success (\d) alone_iter (\d+) x_norm ([-\d.e+naif]+) rel_diff ([-\d.e+naif]+)$" % tag, stdout, re.M)
        assert len(rows) == 12
        for k, s, ok, it, aok, ait, xn, rd in rows:
            assert ok == "1" and aok == "1", (tag, k, s)
            if tag == "BATCH0" and k == "1":
                assert int(it) == 0 and float(xn) == 0.0
            else:
                assert int(it) > 10 and abs(int(it) - int(ait)) <= 1 and float(rd) < 1e-7, (tag, k, s, it, ait, rd)
    assert "[GUESS] refused 1" in stdout
    assert len(re.findall(r"\[QMG-ERROR\]: CG-M: non-zero initial guess", stdout)) == 1 and stdout.count("[QMG-ERROR]") == 1


# ---------------------------------------------------------------- the n20 driver ----------------------------------------------------------------
def _n20(args, timeout):
    out = subprocess.run([os.path.join(DRIVERS, "n20_staggered_goldstone_u1_heatbath")] + args, cwd=DRIVERS, env=dict(os.environ, QMG_QUIET="1"),
                         capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    return out.stdout


def _correlator(block):
    body = block[block.index("[QMG-BEGIN-PION]"):block.index("[QMG-END-PION]")]
    rows = re.findall(r"^(\d+) ([-\d.e+]+) \+/- ([-\d.e+]+)$", body, re.M)
    return np.array([int(r[0]) for r in rows], dtype=float), np.array([float(r[1]) for r in rows]), np.array([float(r[2]) for r in rows])


def test_n20_mass_list_matches_the_reference_table_from_one_ensemble():
    """tests/n20_staggered_goldstone_u1_heatbath/critical_mass.txt:4-7 -- the four rows test_n20_staggered_pion_mass_matches_the_reference_table
    takes from four processes -- from ONE process and one ensemble: 32^2, beta = 6.0, 400 configurations, every propagator from
    Staggered2D::solve_masses; the same cosh fit over t = 7..16, the same +-0.006 band on every row."""
    from scipy.optimize import curve_fit
    table = [(0.1, 0.355891), (0.08, 0.308843), (0.06, 0.258516), (0.04, 0.202947)]
    stdout = _n20(["32", ",".join(str(m) for m, _ in table), "6.0", "400", "100", "1000", "1337"], 900)
    assert "400 measurements, 0 unconverged" in stdout
    blocks = stdout.split("[QMG-MASS]: ")[1:]
    assert len(blocks) == 4
    got = []
    for (mass, m_pi_ref), block in zip(table, blocks):
        assert float(block.split("\n", 1)[0]) == mass
        t, c, dc = _correlator(block)
        assert len(t) == 32 and np.all(c > 0)
        sel = (t >= 7) & (t <= 16)
        (amp, m_pi), cov = curve_fit(lambda tt, a, m: a * np.cosh(m * (tt - 16.0)), t[sel], c[sel], p0=(c[16], 0.3), sigma=dc[sel], absolute_sigma=True)
        got.append((mass, m_pi, m_pi_ref, float(np.sqrt(cov[1, 1]))))
    print(got)
    for mass, m_pi, m_pi_ref, err in got:
        assert abs(m_pi - m_pi_ref) < 0.006, (mass, m_pi, err)


def test_n20_single_mass_is_unchanged_and_the_list_agrees_with_it():
    """A single mass runs as before (BiCGStab-6; no [QMG-MASS] header, one correlator block); the same seed with a mass list gives the
    same ensemble (identical plaquette line) and, for the mass both runs share, the same correlator to the solver tolerance (two solves to
    1e-10 of well-conditioned systems: 1e-7 relative on |S|^2 summed over a timeslice is generous)."""
    args = ["6.0", "6", "10", "50", "1337"]
    one = _n20(["32", "0.1"] + args, 300)
    many = _n20(["32", "0.05,0.1"] + args, 300)
    assert "[QMG-MASS]" not in one and one.count("[QMG-BEGIN-PION]\n") == 1 and one.count("[QMG-BEGIN-PION-EFFMASS]") == 1
    assert many.count("[QMG-BEGIN-PION]\n") == 2
    line = lambda s: re.search(r"^\[QMG-GAUGE-FINAL\].*$", s, re.M).group(0)
    assert line(one) == line(many)
    assert "6 measurements, 0 unconverged" in one and "6 measurements, 0 unconverged" in many
    blocks = many.split("[QMG-MASS]: ")[1:]
    assert [float(b.split("\n", 1)[0]) for b in blocks] == [0.05, 0.1]
    _, c1, _ = _correlator(one)
    _, c2, _ = _correlator(blocks[1])
    assert np.all(np.abs(c1 - c2) <= 1e-7 * c1 + 2e-10)      # (the correlator is printed with ten decimals)
    _, c3, _ = _correlator(blocks[0])
    assert np.all(c3[1:] > c2[1:])      # the lighter mass falls off more slowly
