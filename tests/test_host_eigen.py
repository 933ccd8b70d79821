"""CPU-side checks of the dense Hermitian eigensolver of the coarsest-level Lanczos (qmg::jacobi_eigh, include/qmg/eigen.hpp),
compiled with g++ against the header (tests/host/eigen_host.cpp), against numpy.linalg.eigh."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("eigen") / "eigen_host")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-o", out, os.path.join(ROOT, "tests", "host", "eigen_host.cpp")])
    return out


def run(exe, tmp_path, A):
    n = A.shape[0]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.int32(n).tobytes())
        f.write(np.ascontiguousarray(A, dtype=np.complex128).tobytes())
    subprocess.check_call([exe, fin, fout], timeout=120)
    raw = np.fromfile(fout, dtype=np.uint8)
    w = raw[:8 * n].view(np.float64)
    Y = raw[8 * n:].view(np.complex128).reshape(n, n)
    return w, Y


def random_hermitian(rng, n):
    X = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    return 0.5 * (X + X.conj().T)


def check(A, w, Y):
    n = A.shape[0]
    assert np.all(np.diff(w) >= 0), "eigenvalues not ascending"
    np.testing.assert_allclose(w, np.linalg.eigh(A)[0], rtol=0, atol=1e-12 * max(np.linalg.norm(A, 2), 1e-300))
    anorm = np.linalg.norm(A, 2)
    assert np.linalg.norm(A @ Y - Y * w[None, :], 2) <= 1e-12 * anorm
    assert np.max(np.abs(Y.conj().T @ Y - np.eye(n))) <= 1e-13


@pytest.mark.parametrize("n", [1, 2, 3, 7, 16, 33, 64, 100, 128, 192])
def test_jacobi_matches_eigh_on_random_hermitian_matrices(exe, tmp_path, n):
    A = random_hermitian(np.random.default_rng(1000 + n), n)
    check(A, *run(exe, tmp_path, A))


@pytest.mark.parametrize("n", [5, 48, 96])
def test_jacobi_on_degenerate_spectra(exe, tmp_path, n):
    rng = np.random.default_rng(7 * n)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    lam = np.repeat(np.arange(1, n // 3 + 2, dtype=np.float64), 3)[:n]   # every eigenvalue (at least) threefold
    A = (Q * lam[None, :]) @ Q.conj().T
    A = 0.5 * (A + A.conj().T)
    check(A, *run(exe, tmp_path, A))


@pytest.mark.parametrize("n", [1, 10, 150])
def test_jacobi_on_diagonal_input(exe, tmp_path, n):
    d = np.random.default_rng(n).standard_normal(n)
    d[: n // 2] = d[0]   # with repeated entries
    A = np.diag(d).astype(np.complex128)
    w, Y = run(exe, tmp_path, A)
    check(A, w, Y)
    np.testing.assert_array_equal(w, np.sort(d))


def test_jacobi_is_deterministic(exe, tmp_path):
    A = random_hermitian(np.random.default_rng(3), 40)
    w1, Y1 = run(exe, tmp_path, A)
    w2, Y2 = run(exe, tmp_path, A)
    np.testing.assert_array_equal(w1, w2)
    np.testing.assert_array_equal(Y1, Y2)
