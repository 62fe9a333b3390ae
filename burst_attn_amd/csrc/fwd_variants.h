// Forward-kernel variant selection: BA_FWD_* knob values -> one of the 12
// instantiated attn_fwd_kernel variants <VPATH, SUBT, NT, NBUF, KREG>.
//
// Host-only and free of HIP includes, so a plain C++17 compiler can build
// it (tests/test_fwd_variant_table_cpu.py does).  What each knob means and
// what was measured is recorded above attn_fwd_kernel in attn_fwd.hip.
#pragma once

struct ba_fwd_knobs {
  int vpath = 0;  // V^T image (tr16 path measured -3%)
  int subt = 1;   // per-subtile softmax (+3% over the joint form)
  int nt = 512;
  int nbuf = 2;
  int kreg = 0;
};

struct ba_fwd_variant {
  int vpath, subt, nt, nbuf, kreg;
};

constexpr bool operator==(const ba_fwd_variant& a, const ba_fwd_variant& b) {
  return a.vpath == b.vpath && a.subt == b.subt && a.nt == b.nt &&
         a.nbuf == b.nbuf && a.kreg == b.kreg;
}

// Every instantiated variant, X(VPATH, SUBT, NT, NBUF, KREG).  The
// launcher expands this list once; ba_fwd_select returns only its members.
#define BA_FWD_VARIANTS(X)                                            \
  X(0, 1, 512, 2, 1) X(0, 1, 512, 4, 2) X(0, 3, 256, 4, 0)            \
  X(0, 2, 512, 4, 0) X(0, 1, 512, 4, 0) X(1, 1, 512, 4, 0)            \
  X(0, 1, 256, 2, 0) X(1, 1, 256, 2, 0) X(0, 0, 512, 2, 0)            \
  X(0, 1, 512, 2, 0) X(1, 0, 512, 2, 0) X(1, 1, 512, 2, 0)

// Accepted values per knob, in ba_fwd_knobs field order.
struct ba_fwd_knob_spec {
  const char* env;
  int n_accepted;
  int accepted[4];
};
constexpr ba_fwd_knob_spec BA_FWD_KNOB_SPECS[5] = {
    {"BA_FWD_VPATH", 2, {0, 1}},
    {"BA_FWD_SUBT", 4, {0, 1, 2, 3}},
    {"BA_FWD_NT", 2, {256, 512}},
    {"BA_FWD_NBUF", 2, {2, 4}},
    {"BA_FWD_KREG", 3, {0, 1, 2}},
};

struct ba_fwd_choice {
  ba_fwd_variant variant;
  const char* bad_knob;  // nullptr = accepted; else the offending env name
  int bad_value;
};

// First match wins.  The experiment variants pin the knobs they require
// (KREG and SUBT=2/3 ignore VPATH/NT/NBUF; NBUF=4 and NT=256 exist for
// SUBT=1 only), so e.g. SUBT=0 with NBUF=4 runs SUBT=1.
constexpr ba_fwd_choice ba_fwd_select(const ba_fwd_knobs& k) {
  const int vals[5] = {k.vpath, k.subt, k.nt, k.nbuf, k.kreg};
  for (int i = 0; i < 5; ++i) {
    bool ok = false;
    for (int j = 0; j < BA_FWD_KNOB_SPECS[i].n_accepted; ++j)
      ok = ok || vals[i] == BA_FWD_KNOB_SPECS[i].accepted[j];
    if (!ok) return {{}, BA_FWD_KNOB_SPECS[i].env, vals[i]};
  }
  if (k.kreg == 1) return {{0, 1, 512, 2, 1}, nullptr, 0};
  if (k.kreg == 2) return {{0, 1, 512, 4, 2}, nullptr, 0};
  if (k.subt == 3) return {{0, 3, 256, 4, 0}, nullptr, 0};
  if (k.subt == 2) return {{0, 2, 512, 4, 0}, nullptr, 0};
  if (k.nbuf == 4 && k.nt == 512) return {{k.vpath, 1, 512, 4, 0}, nullptr, 0};
  if (k.nt == 256) return {{k.vpath, 1, 256, 2, 0}, nullptr, 0};
  return {{k.vpath, k.subt, 512, 2, 0}, nullptr, 0};
}

// What the defaults select: the variant the ring runs, and the one the
// .s -> hsaco side-build extracts for the module-launched forward.
constexpr ba_fwd_variant BA_FWD_PRODUCTION = ba_fwd_select(ba_fwd_knobs{}).variant;
static_assert(BA_FWD_PRODUCTION == ba_fwd_variant{0, 1, 512, 2, 0},
              "build_ext.py extracts <...,0,1,512,2,0> by mangled name");
