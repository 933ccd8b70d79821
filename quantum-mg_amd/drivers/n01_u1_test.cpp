// n01_u1_test -- the build's counterpart of tests/n01_u1_test/u1_test.cpp on the GPU: every U(1) field tool of include/qmg/u1.hpp
// once, in the reference's order and with its printed sentences -- unit field; Gaussian fields down the beta ladder 100, 10, ..., 1e-3,
// each APE-smeared (alpha 0.1, 3 iterations); hot field; write and read back; random gauge transform; a smooth field plus a
// charge-1 instanton at the centre.
//   ./n01_u1_test [L [scratch_cfg]]
// The reference hard-codes L = 16 and writes ./cfg/cfg16_hot.dat; here L defaults to 16 and the scratch configuration goes to the
// second argument (default /tmp/qmg_n01_cfg<L>_hot.dat).  The fields are other draws of the same distributions (HeatbathRng instead
// of std::mt19937), so the numbers differ from a reference run; what is fixed -- plaquette 1 and topology 0 of the unit field, the
// plaquette's gauge invariance, smearing raising it -- is what tests/test_gpu_u1_tools.py reads off the output.
#include <iomanip>
#include <iostream>
#include <string>

#include "../include/qmg/qmg.hpp"
#include "driver_common.hpp"

using namespace std;

int main(int argc, char** argv) {
  qmg_driver::Guard guard;
  if (!qmg::ok(qmg_init(getenv("LOCAL_RANK") ? atoi(getenv("LOCAL_RANK")) : 0), "qmg_init")) return 2;
  cout << setiosflags(ios::fixed) << setprecision(6);

  const int x_len = (argc > 1) ? stoi(argv[1]) : 16;
  const int y_len = x_len;
  const string cfg = (argc > 2) ? argv[2] : "/tmp/qmg_n01_cfg" + to_string(x_len) + "_hot.dat";
  double beta = 3.0;
  const double alpha = 0.1;
  const int n_iter = 3;
  HeatbathRng generator(1337ull);

  Lattice2D* lat = new Lattice2D(x_len, y_len, 1);
  complex<double>* field1 = allocate_vector<complex<double>>(lat->get_size_gauge());
  complex<double>* field2 = allocate_vector<complex<double>>(lat->get_size_gauge());
  complex<double>* trans1 = allocate_vector<complex<double>>(lat->get_size_cm());

  unit_gauge_u1(field1, lat);
  cout << "A unit gauge field has average plaquette " << get_plaquette_u1(field1, lat) << " and topology " << get_topo_u1(field1, lat) << "\n";

  for (beta = 100; beta > 1e-4; beta *= 0.1) {
    gauss_gauge_u1(field1, lat, generator, beta);
    cout << "A gauge field with beta " << beta << " has average plaquette " << get_plaquette_u1(field1, lat) << " and topology " << get_topo_u1(field1, lat) << "\n";
    apply_ape_smear_u1(field2, field1, lat, alpha, n_iter);
    cout << " and, after " << n_iter << " iteration(s) of ape smearing with alpha=" << alpha << ", has average plaquette " << get_plaquette_u1(field2, lat)
         << " and topology " << get_topo_u1(field2, lat) << "\n";
  }

  rand_gauge_u1(field1, lat, generator);
  cout << "A random gauge field has average plaquette " << get_plaquette_u1(field1, lat) << " and topology " << get_topo_u1(field1, lat) << "\n";

  cout << "Saving the random gauge field to file...\n";
  write_gauge_u1(field1, lat, cfg);
  cout << "Load the random gauge field from file...\n";
  if (!read_gauge_u1(field2, lat, cfg)) return qmg_driver::leave(1);
  cout << "The loaded gauge field has average plaquette " << get_plaquette_u1(field2, lat) << " and topology " << get_topo_u1(field2, lat) << "\n";

  cout << "Getting a random gauge transform.\n";
  rand_trans_u1(trans1, lat, generator);
  cout << "Applying the random gauge transform.\n";
  apply_gauge_trans_u1(field2, trans1, lat);
  cout << "After a random gauge transform, the average plaquette is " << get_plaquette_u1(field2, lat) << " and topology " << get_topo_u1(field2, lat) << "\n";

  cout << "Creating a rather smooth field for instanton tests.\n";
  gauss_gauge_u1(field2, lat, generator, 6.0);
  cout << "The smooth field has average plaquette " << get_plaquette_u1(field2, lat) << " and topology " << get_topo_u1(field2, lat) << "\n";
  create_instanton_u1(field2, lat, 1, x_len / 2, y_len / 2);
  cout << "After adding an instanton with charge 1, the average plaquette is " << get_plaquette_u1(field2, lat) << " and topology " << get_topo_u1(field2, lat) << "\n";

  deallocate_vector(&field1); deallocate_vector(&field2); deallocate_vector(&trans1);
  delete lat;
  qmg::VecPool::release_all();
  return qmg_driver::leave(0);
}
