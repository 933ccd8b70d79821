// Host-only check of the facade's routing policy (no GPU call is made; links libqmg_hip.so for the symbols only).
//   1. Stencil2D::resolve_route -- which arrays and which entry point serve an apply -- against the table below, written out by hand from the
//      policy: one row per rule and one for the nearest state in which the rule must not fire.  The states are fabricated: every
//      array is a distinct fake pointer, named after the allocation it stands for.
//   2. qmg_stencil_plan gives one plan for QMG_SE_APPLY and for QMG_SE_MASKED with one system and no holes, on every (Lx, Ly, nc, pieces) passed
//      on the command line (tests/test_host_stencil_route.py passes the fp64 rows of the stencil route table): run_route serves one vector
//      through qmg_stencil_apply_batch.
// Which of qmg_stencil_apply_h16 / _mat16_t serves 16-bit matrices under complex<float> vectors is run_route's choice by nc, not the route's:
// drivers/facade_selftest.cpp pins it on the GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../quantum-mg_amd/include/qmg/qmg.hpp"

typedef Stencil2D S;
enum Fake { NONE = 0, CLOVER, HOPPING, DAG_CL, DAG_HO, RBJ_CL, RBJ_HO, CINV, RBJD_HO, CL32, HO32, RBJ_HO32, CINV32,
            F_CL, F_HO, F_RBJ_HO, F_CINV, F_DAG_CL, F_DAG_HO, F_RBJD_HO, H_CL, H_HO, H_RBJ_HO, GAUGE, GAUGE32 };
static void* P(int i) { return reinterpret_cast<void*>((size_t)0x1000 * i); }
static const char* fake_name(const void* p) {
  static const char* n[] = {"0", "clover", "hopping", "dagger_clover", "dagger_hopping", "rbjacobi_clover", "rbjacobi_hopping", "rbjacobi_cinv", "rbj_dagger_hopping", "clover32",
                            "hopping32", "rbj_hopping32", "rbj_cinv32", "f32.clover", "f32.hopping", "f32.rbj_hopping", "f32.rbj_cinv", "f32.dagger_clover", "f32.dagger_hopping",
                            "f32.rbj_dagger_hopping", "f32.clover16", "f32.hopping16", "f32.rbj_hopping16", "gauge", "gauge32"};
  return n[(size_t)p / 0x1000];
}

// ---- states
enum { STORAGE = S::QMG_NARROW_STORAGE, SHADOW = S::QMG_NARROW_SHADOW, HALF = S::QMG_NARROW_SHADOW_HALF };
static void*& clover_copy(S::RouteState& s, int use, S::QMGArraySet set = S::QMG_ARR_ORIGINAL) { return s.narrow[use].copy[set][S::QMG_SLOT_CLOVER]; }
static void*& hopping_copy(S::RouteState& s, int use, S::QMGArraySet set = S::QMG_ARR_ORIGINAL) { return s.narrow[use].copy[set][S::QMG_SLOT_HOPPING]; }
static S::RouteState fine() {   // a Wilson operator (nc = 2) filled from its links, every variant built, nothing swapped in, no narrow copy of any kind
  S::RouteState s = S::RouteState();
  s.clover = P(CLOVER); s.hopping = P(HOPPING); s.dagger_clover = P(DAG_CL); s.dagger_hopping = P(DAG_HO);
  s.rbjacobi_hopping = P(RBJ_HO); s.rbjacobi_cinv = P(CINV); s.rbj_dagger_hopping = P(RBJD_HO);
  s.built_rbjacobi = true; s.generated = true; s.narrow[STORAGE].bits = 32; s.nc = 2;
  s.direct.on = true; s.direct.gauge = (complex<double>*)P(GAUGE); s.direct.kind = S::QMG_DIRECT_WILSON; s.direct.w = 1.0; s.direct.rbj_scale = 0.25;
  return s;
}
static S::RouteState dwf() { S::RouteState s = fine(); s.nc = 8; s.direct.kind = S::QMG_DIRECT_DWF; s.direct.Ls = 4; s.direct.rbj_scale = 0.0; return s; }
static S::RouteState coarse() { S::RouteState s = fine(); s.nc = 8; s.direct.on = false; s.direct.gauge = 0; s.direct.rbj_scale = 0.0; return s; }   // a Galerkin operator: no links
static S::RouteState shadow(S::RouteState s, bool half = false) {   // enable_f32_shadow(half) on a direct-apply operator: gauge32 comes with it
  s.narrow[SHADOW].on = true; clover_copy(s, SHADOW) = P(F_CL); hopping_copy(s, SHADOW) = P(F_HO);
  hopping_copy(s, SHADOW, S::QMG_ARR_RBJ_HOPPING) = P(F_RBJ_HO); clover_copy(s, SHADOW, S::QMG_ARR_RBJ_CINV) = P(F_CINV);
  clover_copy(s, SHADOW, S::QMG_ARR_DAGGER) = P(F_DAG_CL); hopping_copy(s, SHADOW, S::QMG_ARR_DAGGER) = P(F_DAG_HO); hopping_copy(s, SHADOW, S::QMG_ARR_RBJ_DAGGER) = P(F_RBJD_HO);
  if (half) { s.narrow[HALF].on = true; clover_copy(s, HALF) = P(H_CL); hopping_copy(s, HALF) = P(H_HO); hopping_copy(s, HALF, S::QMG_ARR_RBJ_HOPPING) = P(H_RBJ_HO); }
  if (s.direct.on) s.direct.gauge32 = P(GAUGE32);
  return s;
}
static S::RouteState unshadowed(S::RouteState s) { s.narrow[SHADOW] = s.narrow[HALF] = S::NarrowCopies(); return s; }   // disable_f32_shadow(): gauge32 survives it
static S::RouteState narrow(S::RouteState s, int bits) {   // enable_f32_matrices(bits)
  s.narrow[STORAGE].on = true; s.narrow[STORAGE].bits = bits; clover_copy(s, STORAGE) = P(CL32); hopping_copy(s, STORAGE) = P(HO32);
  hopping_copy(s, STORAGE, S::QMG_ARR_RBJ_HOPPING) = P(RBJ_HO32); clover_copy(s, STORAGE, S::QMG_ARR_RBJ_CINV) = P(CINV32);
  return s;
}
static S::RouteState swapped_dagger(S::RouteState s) { s.swap_dagger = true; std::swap(s.clover, s.dagger_clover); std::swap(s.hopping, s.dagger_hopping); return s; }
static S::RouteState swapped_rbj(S::RouteState s) {   // perform_swap_rbjacobi: `hopping` IS the right-block-Jacobi array now, `rbjacobi_hopping` the ORIGINAL one
  s.swap_rbjacobi = true; s.clover = P(RBJ_CL); std::swap(s.hopping, s.rbjacobi_hopping); return s;
}
static S::RouteState swapped_rbj_dagger(S::RouteState s) { s.swap_rbj_dagger = true; s.clover = 0; std::swap(s.hopping, s.rbj_dagger_hopping); return s; }
static S::RouteState with(S::RouteState s, bool S::RouteState::*flag, bool v) { s.*flag = v; return s; }
static S::RouteState rbj_scale(S::RouteState s, double v) { s.direct.rbj_scale = v; return s; }
static S::RouteState no_gauge32(S::RouteState s) { s.direct.gauge32 = 0; return s; }
static S::RouteState links_off(S::RouteState s) { s.direct.on = false; return s; }
static S::RouteState pruned(S::RouteState s, bool clover_too) { s.hopping = 0; if (clover_too) s.clover = 0; return s; }   // (as if the link copy had survived the prune)
static S::RouteState no_clover(S::RouteState s) { s.clover = 0; s.dagger_clover = 0; clover_copy(s, STORAGE) = 0; return s; }
static S::RouteState no_rbj_copies(S::RouteState s) { hopping_copy(s, STORAGE, S::QMG_ARR_RBJ_HOPPING) = 0; clover_copy(s, STORAGE, S::QMG_ARR_RBJ_CINV) = 0; return s; }
static S::RouteState on_slab(S::RouteState s) { s.slab_on = true; return s; }

// ---- requests
enum { WHOLE = S::QMG_ROUTE_WHOLE, SLAB = S::QMG_ROUTE_SLAB, EPI = S::QMG_ROUTE_EPILOGUE };
static const unsigned ALL = QMG_P_ALL | QMG_P_ZERO, OE = QMG_P_OE | QMG_P_ZERO_O;
static S::RouteRequest ptr(int cl, int ho, unsigned pieces, int mode) { S::RouteRequest q = {P(cl), P(ho), false, S::QMG_ARR_ORIGINAL, pieces, QMG_C64, mode, true}; return q; }
static S::RouteRequest set(S::QMGArraySet a, unsigned pieces, int dtype, int mode, bool wanted = true) { S::RouteRequest q = {0, 0, true, a, pieces, dtype, mode, wanted}; return q; }

// ---- expectations
static S::Route stored(int cl, int ho, int storage) { S::Route r = {false, S::QMG_LINKS_NONE, 0, P(cl), P(ho), storage}; return r; }
static S::Route links(int kind, int gauge, S::Route fallback) { fallback.links = kind; fallback.gauge = P(gauge); return fallback; }
static S::Route refused() { S::Route r = {true, S::QMG_LINKS_NONE, 0, 0, 0, S::QMG_MAT_C64}; return r; }
enum { C64 = S::QMG_MAT_C64, C32 = S::QMG_MAT_C32, C16 = S::QMG_MAT_C16, WILSON = S::QMG_LINKS_WILSON, DWF = S::QMG_LINKS_DWF, HOPS = S::QMG_LINKS_RBJ_HOPS };

struct Row { const char* what; S::RouteState s; S::RouteRequest q; S::Route want; };

int main(int argc, char** argv) {
  const S::QMGArraySet ORIGINAL = S::QMG_ARR_ORIGINAL, RBJ_HOPPING = S::QMG_ARR_RBJ_HOPPING, RBJ_CINV = S::QMG_ARR_RBJ_CINV, DAGGER = S::QMG_ARR_DAGGER, RBJ_DAGGER = S::QMG_ARR_RBJ_DAGGER;
  bool S::RouteState::*const generated = &S::RouteState::generated;
  bool S::RouteState::*const built_rbjacobi = &S::RouteState::built_rbjacobi;
  const Row table[] = {
    // ======== the ORIGINAL operator from the links
    {"ORIGINAL from Wilson links, one vector", fine(), ptr(CLOVER, HOPPING, ALL, WHOLE), links(WILSON, GAUGE, stored(CLOVER, HOPPING, C64))},
    {"... on a slab", on_slab(fine()), ptr(CLOVER, HOPPING, ALL, SLAB), links(WILSON, GAUGE, stored(CLOVER, HOPPING, C64))},
    {"... by set", fine(), set(ORIGINAL, ALL, QMG_C64, WHOLE), links(WILSON, GAUGE, stored(CLOVER, HOPPING, C64))},
    {"... by set on a slab", on_slab(fine()), set(ORIGINAL, ALL, QMG_C64, SLAB), links(WILSON, GAUGE, stored(CLOVER, HOPPING, C64))},
    {"... with an epilogue", fine(), set(ORIGINAL, ALL, QMG_C64, EPI), links(WILSON, GAUGE, stored(CLOVER, HOPPING, C64))},
    {"... any piece set is offered to the links entry (it declines what it does not serve)", fine(), ptr(CLOVER, HOPPING, QMG_P_CLOVER, WHOLE), links(WILSON, GAUGE, stored(CLOVER, HOPPING, C64))},
    {"not: the clover alone (apply_M_ee)", fine(), ptr(CLOVER, NONE, QMG_P_CLOVER_E | QMG_P_SHIFT_E, WHOLE), stored(CLOVER, NONE, C64)},
    {"not: the dagger stencil swapped in", swapped_dagger(fine()), ptr(DAG_CL, DAG_HO, ALL, WHOLE), stored(DAG_CL, DAG_HO, C64)},
    {"not: the dagger stencil swapped in, by set", swapped_dagger(fine()), set(ORIGINAL, ALL, QMG_C64, WHOLE), stored(DAG_CL, DAG_HO, C64)},
    {"not: the right-block-Jacobi stencil swapped in, full apply", swapped_rbj(fine()), ptr(RBJ_CL, RBJ_HO, ALL, WHOLE), stored(RBJ_CL, RBJ_HO, C64)},
    {"not: the rbj-dagger stencil swapped in", swapped_rbj_dagger(fine()), ptr(NONE, RBJD_HO, OE, WHOLE), stored(NONE, RBJD_HO, C64)},
    {"not: a null pair after a prune (0 == 0)", pruned(fine(), true), ptr(NONE, NONE, ALL, WHOLE), stored(NONE, NONE, C64)},
    {"not: the hopping term pruned", pruned(fine(), false), ptr(CLOVER, NONE, ALL, WHOLE), stored(CLOVER, NONE, C64)},
    {"not: generated false (clear_stencils)", with(fine(), generated, false), ptr(CLOVER, HOPPING, ALL, WHOLE), stored(CLOVER, HOPPING, C64)},
    {"not: the links dropped", links_off(fine()), ptr(CLOVER, HOPPING, ALL, WHOLE), stored(CLOVER, HOPPING, C64)},
    {"fp32 vectors: gauge32", shadow(fine()), set(ORIGINAL, ALL, QMG_C32, WHOLE), links(WILSON, GAUGE32, stored(F_CL, F_HO, C32))},
    {"fp32 vectors on a slab", on_slab(shadow(fine())), set(ORIGINAL, ALL, QMG_C32, SLAB), links(WILSON, GAUGE32, stored(F_CL, F_HO, C32))},
    {"fp32 vectors with an epilogue", shadow(fine()), set(ORIGINAL, ALL, QMG_C32, EPI), links(WILSON, GAUGE32, stored(F_CL, F_HO, C32))},
    {"not: fp32 vectors without gauge32", no_gauge32(shadow(fine())), set(ORIGINAL, ALL, QMG_C32, WHOLE), stored(F_CL, F_HO, C32)},
    {"domain-wall links, whole lattice", dwf(), ptr(CLOVER, HOPPING, ALL, WHOLE), links(DWF, GAUGE, stored(CLOVER, HOPPING, C64))},
    {"domain-wall links, whole lattice, fp32 by set", shadow(dwf()), set(ORIGINAL, ALL, QMG_C32, WHOLE), links(DWF, GAUGE32, stored(F_CL, F_HO, C32))},
    {"not: domain-wall links on a slab", on_slab(dwf()), ptr(CLOVER, HOPPING, ALL, SLAB), stored(CLOVER, HOPPING, C64)},
    {"not: domain-wall links on a slab, by set", on_slab(dwf()), set(ORIGINAL, ALL, QMG_C64, SLAB), stored(CLOVER, HOPPING, C64)},
    {"not: domain-wall links with an epilogue", dwf(), set(ORIGINAL, ALL, QMG_C64, EPI), stored(CLOVER, HOPPING, C64)},
    {"not: f32_matrices on (the narrow copies are the operator now)", narrow(dwf(), 32), ptr(CLOVER, HOPPING, ALL, WHOLE), stored(CL32, HO32, C32)},
    {"not: f32_matrices on, by set", narrow(dwf(), 16), set(ORIGINAL, ALL, QMG_C64, WHOLE), stored(CL32, HO32, C16)},
    // ======== the right-block-Jacobi hops from the links
    {"rbj hops from the links, one vector", fine(), ptr(NONE, RBJ_HO, OE, WHOLE), links(HOPS, GAUGE, stored(NONE, RBJ_HO, C64))},
    {"... on a slab", on_slab(fine()), ptr(NONE, RBJ_HO, QMG_P_EO, SLAB), links(HOPS, GAUGE, stored(NONE, RBJ_HO, C64))},
    {"... by set", fine(), set(RBJ_HOPPING, QMG_P_HOPPING | QMG_P_ZERO, QMG_C64, WHOLE), links(HOPS, GAUGE, stored(NONE, RBJ_HO, C64))},
    {"... by set with an epilogue", fine(), set(RBJ_HOPPING, OE, QMG_C64, EPI), links(HOPS, GAUGE, stored(NONE, RBJ_HO, C64))},
    {"... fp32 by set on a slab", on_slab(shadow(fine())), set(RBJ_HOPPING, OE, QMG_C32, SLAB), links(HOPS, GAUGE32, stored(NONE, F_RBJ_HO, C32))},
    {"... while swap_rbjacobi is on: `hopping` is the rbj array", swapped_rbj(fine()), ptr(NONE, RBJ_HO, OE, WHOLE), links(HOPS, GAUGE, stored(NONE, RBJ_HO, C64))},
    {"... while swap_rbjacobi is on, by set", swapped_rbj(fine()), set(RBJ_HOPPING, OE, QMG_C64, WHOLE), links(HOPS, GAUGE, stored(NONE, RBJ_HO, C64))},
    {"not: swap_rbjacobi on and the ORIGINAL hops asked for (they sit in rbjacobi_hopping)", swapped_rbj(fine()), ptr(NONE, HOPPING, OE, WHOLE), stored(NONE, HOPPING, C64)},
    {"not: swap_rbjacobi on, hops of the swapped-in pair with its clover", swapped_rbj(fine()), ptr(RBJ_CL, RBJ_HO, OE, WHOLE), stored(RBJ_CL, RBJ_HO, C64)},
    {"not: rbj_scale == 0", rbj_scale(fine(), 0.0), ptr(NONE, RBJ_HO, OE, WHOLE), stored(NONE, RBJ_HO, C64)},
    {"not: a clover bit in pieces", fine(), ptr(NONE, RBJ_HO, QMG_P_OE | QMG_P_CLOVER_O, WHOLE), stored(NONE, RBJ_HO, C64)},
    {"not: a shift bit in pieces", fine(), ptr(NONE, RBJ_HO, QMG_P_OE | QMG_P_SHIFT_E, WHOLE), stored(NONE, RBJ_HO, C64)},
    {"not: a shift bit in pieces, by set", fine(), set(RBJ_HOPPING, QMG_P_EO | QMG_P_SHIFT_O, QMG_C64, WHOLE), stored(NONE, RBJ_HO, C64)},
    {"not: swap_dagger on", swapped_dagger(fine()), ptr(NONE, RBJ_HO, OE, WHOLE), stored(NONE, RBJ_HO, C64)},
    {"not: swap_rbj_dagger on", swapped_rbj_dagger(fine()), ptr(NONE, RBJ_HO, OE, WHOLE), stored(NONE, RBJ_HO, C64)},
    {"not: the stencil is not built", with(fine(), built_rbjacobi, false), ptr(NONE, RBJ_HO, OE, WHOLE), stored(NONE, RBJ_HO, C64)},
    {"not: the ORIGINAL hops alone", fine(), ptr(NONE, HOPPING, OE, WHOLE), stored(NONE, HOPPING, C64)},
    {"not: the links dropped", links_off(fine()), ptr(NONE, RBJ_HO, OE, WHOLE), stored(NONE, RBJ_HO, C64)},
    {"not: fp32 vectors without gauge32", no_gauge32(shadow(fine())), set(RBJ_HOPPING, OE, QMG_C32, WHOLE), stored(NONE, F_RBJ_HO, C32)},
    // ======== the narrow triple under fp64 vectors (enable_f32_matrices)
    {"narrow ORIGINAL pair, complex<float>", narrow(coarse(), 32), ptr(CLOVER, HOPPING, ALL, WHOLE), stored(CL32, HO32, C32)},
    {"narrow ORIGINAL pair, complex<half>", narrow(coarse(), 16), ptr(CLOVER, HOPPING, ALL, WHOLE), stored(CL32, HO32, C16)},
    {"narrow ORIGINAL pair, by set on a slab", on_slab(narrow(coarse(), 16)), set(ORIGINAL, ALL, QMG_C64, SLAB), stored(CL32, HO32, C16)},
    {"narrow ORIGINAL pair, one vector on a slab", on_slab(narrow(coarse(), 32)), ptr(CLOVER, HOPPING, ALL, SLAB), stored(CL32, HO32, C32)},
    {"narrow ORIGINAL pair with an epilogue", narrow(coarse(), 32), set(ORIGINAL, ALL, QMG_C64, EPI), stored(CL32, HO32, C32)},
    {"narrow rbj hops alone, complex<float>", narrow(coarse(), 32), ptr(NONE, RBJ_HO, OE, WHOLE), stored(NONE, RBJ_HO32, C32)},
    {"narrow rbj hops alone, complex<half>", narrow(coarse(), 16), set(RBJ_HOPPING, OE, QMG_C64, WHOLE), stored(NONE, RBJ_HO32, C16)},
    {"narrow cinv alone, complex<float>", narrow(coarse(), 32), set(RBJ_CINV, QMG_P_CLOVER | QMG_P_ZERO, QMG_C64, WHOLE), stored(CINV32, NONE, C32)},
    {"narrow cinv alone, complex<half>", narrow(coarse(), 16), ptr(CINV, NONE, QMG_P_CLOVER | QMG_P_ZERO, WHOLE), stored(CINV32, NONE, C16)},
    {"narrow cinv alone with an epilogue", narrow(coarse(), 16), set(RBJ_CINV, QMG_P_CLOVER | QMG_P_ZERO, QMG_C64, EPI), stored(CINV32, NONE, C16)},
    {"not: f32_matrices off", coarse(), ptr(CLOVER, HOPPING, ALL, WHOLE), stored(CLOVER, HOPPING, C64)},
    {"not: the clover of the ORIGINAL pair alone", narrow(coarse(), 32), ptr(CLOVER, NONE, QMG_P_CLOVER, WHOLE), stored(CLOVER, NONE, C64)},
    {"not: the rbj hops without their copy (out of half range)", no_rbj_copies(narrow(coarse(), 16)), ptr(NONE, RBJ_HO, OE, WHOLE), stored(NONE, RBJ_HO, C64)},
    {"not: cinv without its copy", no_rbj_copies(narrow(coarse(), 16)), set(RBJ_CINV, QMG_P_CLOVER, QMG_C64, WHOLE), stored(CINV, NONE, C64)},
    {"not: the dagger stencil swapped in", swapped_dagger(narrow(coarse(), 32)), ptr(DAG_CL, DAG_HO, ALL, WHOLE), stored(DAG_CL, DAG_HO, C64)},
    {"not: the dagger stencil swapped in, by set", swapped_dagger(narrow(coarse(), 32)), set(ORIGINAL, ALL, QMG_C64, WHOLE), stored(DAG_CL, DAG_HO, C64)},
    {"not: the rbj stencil swapped in", swapped_rbj(narrow(coarse(), 16)), ptr(RBJ_CL, RBJ_HO, ALL, WHOLE), stored(RBJ_CL, RBJ_HO, C64)},
    {"not: the rbj stencil swapped in, its hops alone", swapped_rbj(narrow(coarse(), 16)), set(RBJ_HOPPING, OE, QMG_C64, WHOLE), stored(NONE, RBJ_HO, C64)},
    {"not: the dagger set", narrow(coarse(), 32), set(DAGGER, ALL, QMG_C64, WHOLE), stored(DAG_CL, DAG_HO, C64)},
    {"not: the dagger set on a slab", on_slab(narrow(coarse(), 32)), set(DAGGER, ALL, QMG_C64, SLAB), stored(DAG_CL, DAG_HO, C64)},
    {"not: the dagger set with an epilogue", narrow(coarse(), 16), set(DAGGER, ALL, QMG_C64, EPI), stored(DAG_CL, DAG_HO, C64)},
    {"not: the dagger set of an operator with no clover at all", no_clover(narrow(coarse(), 32)), set(DAGGER, ALL, QMG_C64, WHOLE), stored(NONE, DAG_HO, C64)},
    {"(that operator's ORIGINAL pair does match: a null clover and hopping32)", no_clover(narrow(coarse(), 32)), set(ORIGINAL, ALL, QMG_C64, WHOLE), stored(NONE, HO32, C32)},
    {"not: the rbj-dagger set", narrow(coarse(), 32), set(RBJ_DAGGER, OE, QMG_C64, WHOLE), stored(NONE, RBJD_HO, C64)},
    {"not: the rbj-dagger set of an operator with no clover at all", no_clover(narrow(coarse(), 16)), set(RBJ_DAGGER, OE, QMG_C64, WHOLE), stored(NONE, RBJD_HO, C64)},
    // ======== the stored route under fp32 vectors
    {"fp32 without the shadow, whole lattice: refused", links_off(fine()), set(ORIGINAL, ALL, QMG_C32, WHOLE), refused()},
    {"fp32 without the shadow, whole lattice, gauge32 left by disable_f32_shadow: the links, then refused", unshadowed(shadow(fine())), set(ORIGINAL, ALL, QMG_C32, WHOLE), links(WILSON, GAUGE32, refused())},
    {"... the rbj hops likewise", unshadowed(shadow(fine())), set(RBJ_HOPPING, OE, QMG_C32, WHOLE), links(HOPS, GAUGE32, refused())},
    {"fp32 without the shadow on a slab: refused before anything, gauge32 or not", on_slab(unshadowed(shadow(fine()))), set(ORIGINAL, ALL, QMG_C32, SLAB), refused()},
    {"fp32 with the shadow: ORIGINAL", shadow(coarse()), set(ORIGINAL, ALL, QMG_C32, WHOLE), stored(F_CL, F_HO, C32)},
    {"fp32 with the shadow: RBJ_HOPPING", shadow(coarse()), set(RBJ_HOPPING, OE, QMG_C32, WHOLE), stored(NONE, F_RBJ_HO, C32)},
    {"fp32 with the shadow: RBJ_CINV", shadow(coarse()), set(RBJ_CINV, QMG_P_CLOVER, QMG_C32, WHOLE), stored(F_CINV, NONE, C32)},
    {"fp32 with the shadow on a slab", on_slab(shadow(coarse())), set(ORIGINAL, ALL, QMG_C32, SLAB), stored(F_CL, F_HO, C32)},
    {"fp32 with the shadow: f32_matrices plays no part", narrow(shadow(coarse()), 16), set(ORIGINAL, ALL, QMG_C32, WHOLE), stored(F_CL, F_HO, C32)},
    {"half on: ORIGINAL, nc = 2", links_off(shadow(fine(), true)), set(ORIGINAL, ALL, QMG_C32, WHOLE), stored(H_CL, H_HO, C16)},
    {"half on: ORIGINAL, nc = 8", shadow(coarse(), true), set(ORIGINAL, ALL, QMG_C32, WHOLE), stored(H_CL, H_HO, C16)},
    {"half on: ORIGINAL, nc = 2, on a slab", on_slab(links_off(shadow(fine(), true))), set(ORIGINAL, ALL, QMG_C32, SLAB), stored(H_CL, H_HO, C16)},
    {"half on: RBJ_HOPPING has no clover16", shadow(coarse(), true), set(RBJ_HOPPING, OE, QMG_C32, WHOLE), stored(NONE, H_RBJ_HO, C16)},
    {"half on: RBJ_CINV stays complex<float>", shadow(coarse(), true), set(RBJ_CINV, QMG_P_CLOVER, QMG_C32, WHOLE), stored(F_CINV, NONE, C32)},
    {"half on: behind the links attempt", shadow(fine(), true), set(ORIGINAL, ALL, QMG_C32, WHOLE), links(WILSON, GAUGE32, stored(H_CL, H_HO, C16))},
    {"half on, nc = 8, with an epilogue: served", shadow(coarse(), true), set(ORIGINAL, ALL, QMG_C32, EPI), stored(H_CL, H_HO, C16)},
    // ======== the dagger and rbj-dagger sets
    {"dagger set, fp64", fine(), set(DAGGER, ALL, QMG_C64, WHOLE), stored(DAG_CL, DAG_HO, C64)},
    {"dagger set, fp64, on a slab", on_slab(fine()), set(DAGGER, ALL, QMG_C64, SLAB), stored(DAG_CL, DAG_HO, C64)},
    {"dagger set, fp32", shadow(fine()), set(DAGGER, ALL, QMG_C32, WHOLE), stored(F_DAG_CL, F_DAG_HO, C32)},
    {"dagger set, fp32, half on: no 16-bit copy", shadow(fine(), true), set(DAGGER, ALL, QMG_C32, WHOLE), stored(F_DAG_CL, F_DAG_HO, C32)},
    {"dagger set, fp32, with an epilogue", shadow(coarse()), set(DAGGER, ALL, QMG_C32, EPI), stored(F_DAG_CL, F_DAG_HO, C32)},
    {"rbj-dagger set, fp64", fine(), set(RBJ_DAGGER, OE, QMG_C64, WHOLE), stored(NONE, RBJD_HO, C64)},
    {"rbj-dagger set, fp64, while it is swapped in: `hopping`", swapped_rbj_dagger(fine()), set(RBJ_DAGGER, OE, QMG_C64, WHOLE), stored(NONE, RBJD_HO, C64)},
    {"rbj-dagger set, fp32", shadow(fine()), set(RBJ_DAGGER, OE, QMG_C32, WHOLE), stored(NONE, F_RBJD_HO, C32)},
    {"rbj-dagger set, fp32, half on, on a slab", on_slab(shadow(fine(), true)), set(RBJ_DAGGER, OE, QMG_C32, SLAB), stored(NONE, F_RBJD_HO, C32)},
    // ======== what an epilogue refuses
    {"epilogue: QMG_APPLY_EPILOGUE=0", fine(), set(ORIGINAL, ALL, QMG_C64, EPI, false), refused()},
    {"epilogue: slab mode", on_slab(fine()), set(ORIGINAL, ALL, QMG_C64, EPI), refused()},
    {"epilogue: fp32 vectors, 16-bit matrices, nc = 2 (kernel S has none)", links_off(shadow(fine(), true)), set(ORIGINAL, ALL, QMG_C32, EPI), refused()},
    {"epilogue: ... behind the links attempt", shadow(fine(), true), set(RBJ_HOPPING, OE, QMG_C32, EPI), links(HOPS, GAUGE32, refused())},
    {"epilogue: fp32 vectors without the shadow", coarse(), set(ORIGINAL, ALL, QMG_C32, EPI), refused()},
    {"epilogue: ... behind the links attempt", unshadowed(shadow(fine())), set(ORIGINAL, ALL, QMG_C32, EPI), links(WILSON, GAUGE32, refused())},
    {"epilogue: 16-bit matrices under fp32 vectors at nc = 2 only for the sets that have them", shadow(fine(), true), set(RBJ_CINV, QMG_P_CLOVER | QMG_P_ZERO, QMG_C32, EPI), stored(F_CINV, NONE, C32)},
  };
  int fails = 0;
  const int rows = (int)(sizeof table / sizeof table[0]);
  for (int i = 0; i < rows; i++) {
    const S::Route got = S::resolve_route(table[i].s, table[i].q), &want = table[i].want;
    if (got.refused != want.refused || got.links != want.links || got.gauge != want.gauge || got.clover != want.clover || got.hopping != want.hopping || got.storage != want.storage) {
      printf("FAIL row %d (%s): got refused %d links %d from %s, stored (%s, %s) storage %d; want refused %d links %d from %s, stored (%s, %s) storage %d\n", i, table[i].what,
             got.refused, got.links, fake_name(got.gauge), fake_name(got.clover), fake_name(got.hopping), got.storage,
             want.refused, want.links, fake_name(want.gauge), fake_name(want.clover), fake_name(want.hopping), want.storage);
      fails++;
    }
  }
  printf("%d route rows\n", rows);

  // ---- 2. one vector through the masked entry: the same plan
  int asked = 0;
  for (int a = 1; a + 3 < argc; a += 4) {
    const int Lx = atoi(argv[a]), Ly = atoi(argv[a + 1]), nc = atoi(argv[a + 2]);
    const unsigned pieces = (unsigned)strtoul(argv[a + 3], 0, 0);
    for (int form = 0; form < 8; form++) {   // lhs == rhs or not, with and without either array
      const int inplace = form & 1, has_clover = !(form & 2), has_hopping = !(form & 4);
      int pa[24], pm[24];
      const int ra = qmg_stencil_plan(QMG_SE_APPLY, 0, 0, Lx, Ly, nc, pieces, 1, 0, inplace, has_clover, has_hopping, 0, 0, pa, 24);
      const int rm = qmg_stencil_plan(QMG_SE_MASKED, 0, 0, Lx, Ly, nc, pieces, 1, 0, inplace, has_clover, has_hopping, 0, 0, pm, 24);
      asked++;
      if (ra != rm || (ra == QMG_SUCCESS && memcmp(pa, pm, sizeof pa) != 0)) {
        printf("FAIL plan of one system differs between QMG_SE_APPLY and QMG_SE_MASKED: %d x %d, nc %d, pieces 0x%x, inplace %d, clover %d, hopping %d\n", Lx, Ly, nc, pieces, inplace,
               has_clover, has_hopping);
        fails++;
      }
    }
  }
  printf("%d plan pairs\n", asked);
  printf("%s (%d failures)\n", fails ? "STENCIL ROUTE FAILED" : "stencil route ok", fails);
  return fails ? 1 : 0;
}
