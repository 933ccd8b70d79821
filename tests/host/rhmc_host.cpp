// Host-only driver of qmg::zolotarev_inv_sqrt (include/qmg/rational.hpp), the coefficients of one-flavour RHMC.
//   ./rhmc_host n ra rb
// Prints, at 17 significant digits: "ok <0|1>", and when ok "c0 <c0>", "delta <delta>" and the four lists "mu2 ...", "nu2 ...", "rho ...",
// "s ..." of n numbers each.  A refusal prints the library's [QMG-ERROR] line first and returns 1.  No GPU call is made.
#include <cstdio>
#include <cstdlib>

#include "../../quantum-mg_amd/include/qmg/rational.hpp"

static void row(const char* name, const std::vector<double>& v) {
  std::printf("%s", name);
  for (size_t i = 0; i < v.size(); i++) std::printf(" %.17g", v[i]);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: rhmc_host n ra rb\n"); return 2; }
  const qmg::ZolotarevInvSqrt z = qmg::zolotarev_inv_sqrt(std::atoi(argv[1]), std::atof(argv[2]), std::atof(argv[3]));
  std::cout.flush();
  std::printf("ok %d\n", z.ok ? 1 : 0);
  if (!z.ok) return 1;
  std::printf("c0 %.17g\ndelta %.17g\n", z.c0, z.delta);
  row("mu2", z.mu2); row("nu2", z.nu2); row("rho", z.rho); row("s", z.s);
  return 0;
}
