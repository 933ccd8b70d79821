// Host-only driver of qmg::jacobi_eigh (include/qmg/eigen.hpp), the dense projected eigensolver of the coarsest-level Lanczos.
//   ./eigen_host in.bin out.bin
// in.bin: int32 n, then the n x n matrix as complex128, row-major.  out.bin: n float64 eigenvalues, then the n x n eigenvector
// matrix Y (column j: eigenvector j) as complex128, row-major.  No GPU call is made.
#define QMG_EIGEN_HOST_ONLY
#include <complex>
#include <cstdio>
#include <vector>

#include "../../quantum-mg_amd/include/qmg/eigen.hpp"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: eigen_host in.bin out.bin\n"); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int n = 0;
  if (std::fread(&n, sizeof(int), 1, f) != 1 || n < 1) return 2;
  std::vector<std::complex<double> > A((size_t)n * n), Y;
  if (std::fread(A.data(), sizeof(std::complex<double>), A.size(), f) != A.size()) return 2;
  std::fclose(f);
  std::vector<double> w;
  qmg::jacobi_eigh(n, A, w, Y);
  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  std::fwrite(w.data(), sizeof(double), w.size(), f);
  std::fwrite(Y.data(), sizeof(std::complex<double>), Y.size(), f);
  std::fclose(f);
  return 0;
}
