// u1_make_config -- a thermalised, optionally prepared, genuinely L x L U(1) configuration file from the device heatbath.
//   ./u1_make_config L beta n_sweeps seed out.dat [ape_alpha ape_iters] [instanton_Q] [gauge_trans_seed]
// Cold start, n_sweeps sweeps of the four-colour non-compact heatbath (csrc/qmg_u1.hip), then -- in this order, each only if its
// arguments are given -- APE smearing, a charge-Q instanton at the centre, a random gauge transform; written with write_gauge_u1 in the
// reference's text format.  One "[QMG-GAUGE]: plaq <re> topo <Q> (<stage>)" line after every stage.  The K-cycle drivers read the file
// through their gauge-file argument; pass their tile argument = L to use it as it is and not as a tile:
//   ./u1_make_config 256 6.0 4000 1337 /tmp/l256b60.dat && ./n13_wilson_kcycle 256 -0.01 6.0 1 8 /tmp/l256b60.dat 256
#include <iomanip>
#include <iostream>
#include <string>

#include "../include/qmg/qmg.hpp"
#include "driver_common.hpp"

using namespace std;

static void report(const char* stage, complex<double>* gauge_field, Lattice2D* lat) {
  cout << "[QMG-GAUGE]: plaq " << std::real(get_plaquette_u1(gauge_field, lat)) << " topo " << get_topo_u1(gauge_field, lat) << " (" << stage << ")\n";
}

int main(int argc, char** argv) {
  qmg_driver::Guard guard;
  if (argc < 6 || argc == 7) { cout << "usage: ./u1_make_config L beta n_sweeps seed out.dat [ape_alpha ape_iters] [instanton_Q] [gauge_trans_seed]\n"; return -1; }
  if (!qmg::ok(qmg_init(getenv("LOCAL_RANK") ? atoi(getenv("LOCAL_RANK")) : 0), "qmg_init")) return 2;
  const int L = stoi(argv[1]);
  const double beta = stod(argv[2]);
  const int n_sweeps = stoi(argv[3]);
  HeatbathRng generator(stoull(argv[4]));
  const string out_file = argv[5];
  cout << setiosflags(ios::fixed) << setprecision(6);

  Lattice2D* lat = new Lattice2D(L, L, 1);
  const size_t n = (size_t)lat->get_size_gauge();
  complex<double>* gauge_field = allocate_vector<complex<double>>(n);
  double* phases = allocate_vector<double>(n);
  qmg::ok(qmg_memset_zero(phases, sizeof(double) * n, qmg::current_stream()), "qmg_memset_zero");   // cold start
  heatbath_noncompact_update(phases, lat, beta, n_sweeps, generator);
  polar_vector(phases, gauge_field, n);
  report("heatbath", gauge_field, lat);

  if (argc > 7) {
    apply_ape_smear_u1(gauge_field, gauge_field, lat, stod(argv[6]), stoi(argv[7]));
    report("ape smearing", gauge_field, lat);
  }
  if (argc > 8) {
    create_instanton_u1(gauge_field, lat, stod(argv[8]), L / 2, L / 2);
    report("instanton", gauge_field, lat);
  }
  if (argc > 9) {
    complex<double>* trans = allocate_vector<complex<double>>(lat->get_size_cm());
    HeatbathRng trans_generator(stoull(argv[9]));
    rand_trans_u1(trans, lat, trans_generator);
    apply_gauge_trans_u1(gauge_field, trans, lat);
    report("gauge transform", gauge_field, lat);
    deallocate_vector(&trans);
  }
  write_gauge_u1(gauge_field, lat, out_file);

  deallocate_vector(&phases); deallocate_vector(&gauge_field);
  delete lat;
  qmg::VecPool::release_all();
  return qmg_driver::leave(0);
}
