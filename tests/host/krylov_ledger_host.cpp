// Host-only driver of qmg::SolveLedger (include/qmg/krylov.hpp), the per-system book-keeping of the lock-step Krylov cores: no device
// code, no library.  Reads a script and writes the ledger's answers; tests/test_host_krylov_ledger.py writes the scenarios and holds the
// answers to the rules stated there in plain Python.
//   ./krylov_ledger_host script.txt out.txt
// One command per line (masks in hex, doubles in any notation strtod reads; `mask` may be the word run or act):
//   ledger nrhs mask max_iter eps per_system   then nrhs values |b_k|^2 and, with per_system = 1, nrhs values eps_k   -> `masks zero_b run act`
//   open mask r0_0 .. r0_{nrhs-1}               the systems of mask open with |r_k|^2 = r0_k                            -> `act m`
//   open_b mask                                  the same under zero_guess: |r_k|^2 = |b_k|^2                            -> `act m`
//   count mask                                   an apply handed to mask
//   recur k delta c                              rsq_k -= delta                                                         -> `renorm 0|1`
//   anchor k t | breakdown k | cap               (cap -> `act m`)
//   step k | settle k                            -> `done 0|1`
//   rows                                         -> `act m`, then per system `row k success iter resSq ops rel rsq_ref`
#define QMG_KRYLOV_HOST_ONLY
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../quantum-mg_amd/include/qmg/krylov.hpp"

int main(int argc, char** argv) {
  if (argc < 3) { printf("usage: ./krylov_ledger_host script.txt out.txt\n"); return 1; }
  std::ifstream in(argv[1]);
  FILE* out = fopen(argv[2], "w");
  if (!in || !out) { printf("cannot open the script or the output\n"); return 2; }
  qmg::SolveLedger* led = 0;
  std::string line, cmd, word;
  while (std::getline(in, line)) {
    std::istringstream s(line);
    if (!(s >> cmd)) continue;
    if (cmd != "ledger" && !led) { printf("no ledger before `%s`\n", line.c_str()); return 3; }
    int k = 0;
    double x = 0.0, c = 0.0;
    unsigned m = 0;
    if (cmd == "open" || cmd == "open_b" || cmd == "count") {
      s >> word;
      m = word == "run" ? led->run : word == "act" ? led->act : (unsigned)strtoul(word.c_str(), 0, 16);
    }
    if (cmd == "ledger") {
      int nrhs = 0, max_iter = 0, per_system = 0;
      s >> nrhs >> std::hex >> m >> std::dec >> max_iter >> x >> per_system;
      std::vector<double> bsq(nrhs), eps(nrhs);
      for (int i = 0; i < nrhs; i++) s >> bsq[i];
      for (int i = 0; i < nrhs && per_system; i++) s >> eps[i];
      if (!s) { printf("bad line `%s`\n", line.c_str()); return 3; }
      delete led;
      led = new qmg::SolveLedger(bsq, m, max_iter, x, per_system ? &eps : 0);
      fprintf(out, "masks %x %x %x\n", led->zero_b, led->run, led->act);
    } else if (cmd == "open") {
      std::vector<double> r0(led->nrhs);
      for (int i = 0; i < led->nrhs; i++) s >> r0[i];
      fprintf(out, "act %x\n", led->open(m, r0));
    } else if (cmd == "open_b") {
      fprintf(out, "act %x\n", led->open(m, led->bsq));
    } else if (cmd == "count") {
      led->count(m);
    } else if (cmd == "recur") {
      s >> k >> x >> c;
      fprintf(out, "renorm %d\n", led->recur(k, x, c) ? 1 : 0);
    } else if (cmd == "anchor") {
      s >> k >> x;
      led->anchor(k, x);
    } else if (cmd == "breakdown") {
      s >> k;
      led->breakdown(k);
    } else if (cmd == "cap") {
      led->cap();
      fprintf(out, "act %x\n", led->act);
    } else if (cmd == "step" || cmd == "settle") {
      s >> k;
      fprintf(out, "done %d\n", (cmd == "step" ? led->step(k) : led->settle(k)) ? 1 : 0);
    } else if (cmd == "rows") {
      fprintf(out, "act %x\n", led->act);
      for (int i = 0; i < led->nrhs; i++) {
        const qmg::SolveLedger::Row o = led->row(i);
        fprintf(out, "row %d %d %d %.17g %d %.17g %.17g\n", i, o.success ? 1 : 0, o.iter, o.resSq, o.ops_count, led->rel(i), led->rsq_ref[i]);
      }
    } else { printf("unknown command `%s`\n", line.c_str()); return 3; }
    if (!s) { printf("bad line `%s`\n", line.c_str()); return 3; }
  }
  delete led;
  fclose(out);
  return 0;
}
