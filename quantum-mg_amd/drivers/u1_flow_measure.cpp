// u1_flow_measure -- Wilson (gradient) flow of a U(1) configuration with scale-setting and confinement observables along the way
// (include/qmg/u1.hpp: WilsonFlowU1, get_wilson_loops_u1, get_polyakov_u1; everything on the device).
//   ./u1_flow_measure in.dat L eps n_steps measure_every r_max t_max [out.dat]
// in.dat: a file written by write_gauge_u1 (u1_make_config, schwinger_hmc, the stored fixtures), read as an L x L lattice.  The field is
// flowed n_steps third-order Runge-Kutta steps of size eps; at t = 0 and after every measure_every steps one row is printed:
//   [FLOW] t <t> E <S_w/V = 1 - Re plaq> plaq <Re plaq> Q <geometric charge> P <Re Im of the x loop, Re Im of the y loop>
//          W <Re W(R,T), R = 1..r_max outer, T = 1..t_max inner> chi <chi(R,T) in the same order>
// with the Creutz ratios chi(R,T) = -log[ W(R,T) W(R-1,T-1) / (W(R-1,T) W(R,T-1)) ], W(0,.) = W(.,0) = 1 (so chi(1,1) = -log W(1,1)); a ratio
// whose argument is not positive is printed as nan.  out.dat receives the flowed field through write_gauge_u1 and is read back through
// read_gauge_u1: [FLOW-READBACK] plaq <Re plaq> Q <charge>.
#include <cmath>
#include <iomanip>
#include <iostream>
#include <string>
#include <vector>

#include "../include/qmg/qmg.hpp"
#include "driver_common.hpp"

using namespace std;

static bool measure(WilsonFlowU1& flow, Lattice2D* lat, int r_max, int t_max) {
  complex<double>* g = flow.links();
  const double plaq = std::real(get_plaquette_u1(g, lat));
  vector<complex<double>> W((size_t)r_max * t_max), P(2);
  if (!get_wilson_loops_u1(g, lat, r_max, t_max, W.data()) || !get_polyakov_u1(g, lat, P.data())) return false;
  cout << "[FLOW] t " << flow.time() << " E " << 1.0 - plaq << " plaq " << plaq << " Q " << get_topo_u1(g, lat);
  cout << " P " << P[0].real() << " " << P[0].imag() << " " << P[1].real() << " " << P[1].imag() << " W";
  for (size_t i = 0; i < W.size(); i++) cout << " " << W[i].real();
  cout << " chi";
  auto w = [&](int R, int T) { return (R == 0 || T == 0) ? 1.0 : W[(size_t)(R - 1) * t_max + (T - 1)].real(); };
  for (int R = 1; R <= r_max; R++)
    for (int T = 1; T <= t_max; T++) {
      const double arg = w(R, T) * w(R - 1, T - 1) / (w(R - 1, T) * w(R, T - 1));
      cout << " " << (arg > 0.0 ? -log(arg) : NAN);
    }
  cout << "\n";
  return true;
}

int main(int argc, char** argv) {
  qmg_driver::Guard guard;
  if (argc < 8) { cout << "usage: ./u1_flow_measure in.dat L eps n_steps measure_every r_max t_max [out.dat]\n"; return -1; }
  if (!qmg::ok(qmg_init(0), "qmg_init")) return 2;
  const string in_cfg = argv[1];
  const int L = stoi(argv[2]);
  const double eps = stod(argv[3]);
  const int n_steps = stoi(argv[4]), measure_every = stoi(argv[5]), r_max = stoi(argv[6]), t_max = stoi(argv[7]);
  const string out_cfg = (argc > 8) ? argv[8] : "";
  if (L < 2 || (L & 1) || n_steps < 0 || measure_every < 1 || r_max < 1 || t_max < 1 || r_max > L / 2 || t_max > L / 2) {
    cout << "[QMG-ERROR]: need an even L, n_steps >= 0, measure_every >= 1 and 1 <= r_max, t_max <= L/2.\n";
    return qmg_driver::leave(3);
  }

  int rc = 0;
  Lattice2D lat(L, L, 1);
  const size_t n_links = (size_t)lat.get_size_gauge();
  complex<double>* gauge = allocate_vector<complex<double>>(n_links);
  if (!read_gauge_u1(gauge, &lat, in_cfg)) rc = 3;
  if (!rc) {
    WilsonFlowU1 flow(gauge, &lat);
    cout << setprecision(14);
    if (!flow.ok() || !measure(flow, &lat, r_max, t_max)) rc = 3;
    for (int done = 0; !rc && done < n_steps;) {
      const int k = (n_steps - done < measure_every) ? n_steps - done : measure_every;
      flow.flow(eps, k);
      done += k;
      if (!measure(flow, &lat, r_max, t_max)) rc = 3;
    }
    if (!rc && !out_cfg.empty()) {   // written, and read back the way the other drivers will read it
      write_gauge_u1(gauge, &lat, out_cfg);
      complex<double>* check = allocate_vector<complex<double>>(n_links);
      if (read_gauge_u1(check, &lat, out_cfg)) cout << "[FLOW-READBACK] plaq " << std::real(get_plaquette_u1(check, &lat)) << " Q " << get_topo_u1(check, &lat) << "\n";
      deallocate_vector(&check);
    }
  }
  deallocate_vector(&gauge);
  qmg::VecPool::release_all();
  return qmg_driver::leave(rc);
}
