// fv3lm-hip: the host side of the linearised column physics -- boundary-layer turbulence with BL_DRIVER (turbulence.h, bldriver.h), RAS
// convection (convection.h) and the cloud scheme (cloud.h) -- behind fv3lm_turbulence_*, fv3lm_convection_* and fv3lm_cloud_*.
// A Physics serves one Dynamics: it reads the resident state and the geometry of its handle and reports through the handle's one error
// string; nothing of it touches the dycore.  A scheme is a kernel header plus its section here.  What the sections share is written
// once below: the owner of a feature's device memory, the refusals, the slot check, the two flags, the batches of columns, the packed
// columns and the scan for values that are not finite.
#pragma once
#include "dynamics.h"
#include "turbulence.h"
#include "bldriver.h"
#include "convection.h"
#include "cloud.h"
#include <array>

namespace fv3 {

// Every device allocation of one feature.  Whether the feature exists, the roll-back after a failed allocation and the release all
// come from this list: a pointer cannot be allocated in one place and forgotten in another.
struct DevList {
  std::vector<void*> p; bool failed = false;
  template <class T> T* get(size_t bytes) { void* q = dev_alloc(bytes); if (q) p.push_back(q); else failed = true; return (T*)q; }
  void refuse() { failed = true; }                                            // a request that is not even tried
  bool ok() { const bool r = !failed; failed = false; return r; }             // every get since the last ok() / release() gave memory
  bool empty() const { return p.empty(); }
  void release() { for (void* q : p) dev_free(q); p.clear(); failed = false; }
};

// the columns n of a call in dense batches of nb: fn(first, count)
template <class Fn> void for_batches(size_t n, size_t nb, const Fn& fn) { for (size_t first = 0; first < n; first += nb) fn((int)first, (int)(n - first < nb ? n - first : nb)); }
inline bool all_finite(const double* p, size_t n) { for (size_t i = 0; i < n; ++i) if (turb_stored_nonfinite(p + i)) return false; return true; }

struct Physics {
  Dynamics& d; const Geom& g; Exec& ex;
  explicit Physics(Dynamics& d_) : d(d_), g(d_.g), ex(d_.ex) {}
  // nothing allocated until the feature's create
  struct Turbulence {
    DevList mem; int nslots = 0; std::vector<double*> slot; std::vector<char> set; double* fro = nullptr; int* flag = nullptr;
    double *bl_sfc = nullptr, *bl_tbl = nullptr, *bl_raw = nullptr;      // BL_DRIVER (bldriver.h): surface planes and table at its first call, EKV FKV at the first raw_out
  } turb;
  struct Convection {
    DevList mem; int nslots = 0, mst = 0, icmin = 0; RasParams p;
    std::vector<double*> slot; std::vector<char> set; std::vector<int*> list; std::vector<int> nactive;
    ColWork w{}; double *src = nullptr, *tbl = nullptr, *sige = nullptr;
  } conv;
  struct Cloud {      // one slot per convection slot
    DevList mem; int iqi = 0, iql = 0; CldParams p;
    int iqc = 0;                    // fv3lm_cloud_bind_cfcn: cfcn is tracer iqc of the dycore (0: the feature's own array below)
    bool was_set = false;           // a slot has been set: too late to bind
    std::vector<double*> slot; std::vector<char> set;
    ColWork w{}; double* cfcn = nullptr;
  } cld;
  template <class F> static void drop(F& f) { f.mem.release(); f = F{}; }
  void release() { drop(turb); drop(cld); drop(conv); }

  // ---- what the sections share ----------------------------------------------------------------------------------------------------------
  bool no(const char* who, const std::string& m) { d.err = std::string(who) + ": " + m; return false; }
  bool sticky_clean() { if (sticky_error().empty()) return true; d.err = sticky_error(); return false; }
  bool slot_ok(const char* who, const char* feature, bool created, int nslots, int slot) {
    if (!created) return no(who, std::string("call fv3lm_") + feature + "_create first");
    if (slot < 0 || slot >= nslots) return no(who, "slot " + std::to_string(slot) + " out of range (0.." + std::to_string(nslots - 1) + ")");
    return true;
  }
  bool slot_set(const char* who, const char* what, const std::vector<char>& set, int slot, const char* by) {
    if (set[(size_t)slot]) return true;
    return no(who, std::string(what) + " " + std::to_string(slot) + " was never set" + (by ? std::string(" (") + by + ")" : std::string()));
  }
  // all-or-nothing: after a failed allocation the feature is as if never created and the handle stays usable.  clean: no sticky error
  // was pending before the feature allocated, so the one the failure left is this refusal's and goes with it
  template <class F> bool allocated(const char* who, F& f, size_t total, bool clean) {
    if (f.mem.ok()) return true;
    no(who, "allocation of " + std::to_string(total) + " bytes failed" + (sticky_error().empty() ? std::string() : ": " + sticky_error()));
    if (clean) sticky_error().clear();
    drop(f);
    return false;
  }
  // work spaces, checkpoints, tape and the two flags of one batch of nb columns
  static ColWork batch_work(DevList& m, size_t b_gw, size_t b_tw, size_t b_ew, size_t b_ck, int cap, size_t nb) {
    ColWork w{};
    w.gw = m.get<double>(b_gw); w.tw = m.get<double>(b_tw); w.ew = m.get<double>(b_ew); w.ck = m.get<double>(b_ck); w.flag = m.get<int>(8); w.nb = (int)nb;
    w.tape.part = m.get<TapePart>((size_t)cap * nb * sizeof(TapePart)); w.tape.idx = m.get<TapeIdx>((size_t)cap * nb * sizeof(TapeIdx));
    w.tape.adj = m.get<double>((size_t)cap * nb * 8); w.tape.overflow = w.flag ? w.flag + 1 : nullptr; w.tape.stride = nb; w.tape.cap = cap;
    return w;
  }
  // a feature's two flags: cleared before the launches that may raise them, read after them
  void clear_flags(int* flag) { dev_zero(ex, flag, 8); }
  std::array<int, 2> read_flags(const int* flag) { std::array<int, 2> f{{0, 0}}; d2h(ex, f.data(), flag, sizeof f); return f; }
  // packed columns: every resident tile at once, col = (tile ty + j) tx + i
  size_t ncol() const { return (size_t)d.ntile_all * g.tx * g.ty; }
  ColView col_view(double* slot, int ns) {
    ColView v; v.g = g; v.ntile = d.ntile_all; v.lm = g.npz; v.ns = ns; v.slot = slot; v.nc = ncol(); v.list = nullptr; v.first = 0; v.n = 0;
    return v;
  }
  // one vector between the host's compact [tile][level][point] and a slot's packed [level][column]; buf: (lm + 1) nc doubles
  void pack_columns(double* dev, const double* src, std::vector<double>& buf) {
    const size_t nc = ncol(), pc = (size_t)g.tx * g.ty; const int lm = g.npz;
    for (size_t col = 0; col < nc; ++col) for (int l = 0; l < lm; ++l) buf[(size_t)l * nc + col] = src[((col / pc) * lm + l) * pc + col % pc];
    h2d(ex, dev, buf.data(), buf.size() * 8);
  }
  template <class T> void unpack_columns(const double* dev, T* dst, std::vector<double>& buf) {      // T int: cloud_pertmod
    const size_t nc = ncol(), pc = (size_t)g.tx * g.ty; const int lm = g.npz;
    d2h(ex, buf.data(), dev, buf.size() * 8);
    for (size_t col = 0; col < nc; ++col) for (int l = 0; l < lm; ++l) dst[((col / pc) * lm + l) * pc + col % pc] = (T)buf[(size_t)l * nc + col];
  }
  // a padded field of nk levels at t, for the boundary copies
  static Fld plane(double* t, int nk) { Fld f; f.t = t; f.nk = nk; return f; }

  // ---- linearised boundary-layer turbulence (turbulence.h) ------------------------------------------------------------------------------
  // fv3lm_turbulence_create: nslots x (9 factor arrays + pk), padded planes
  bool turb_create(int nslots) {
    const char* who = "fv3lm_turbulence_create";
    if (!turb.mem.empty()) return no(who, "already created for this handle");
    if (nslots < 1) return no(who, "nslots < 1");
    if (g.npz < 2) return no(who, "npz < 2 (a tridiagonal system needs two levels)");
    const size_t bytes = (size_t)TURB_NARR * d.n3 * 8;
    if (std::getenv("FV3LM_VERBOSE")) std::fprintf(stderr, "fv3lm: turbulence arena %d slot(s) x %d arrays x %zu doubles = %zu bytes\n", nslots, TURB_NARR, d.n3, (size_t)nslots * bytes);
    const bool clean = sticky_error().empty();
    for (int n = 0; n < nslots; ++n) turb.slot.push_back(turb.mem.get<double>(bytes));
    turb.fro = turb.mem.get<double>((size_t)d.ntile_all * g.plane * 8); turb.flag = turb.mem.get<int>(8);
    if (!allocated(who, turb, (size_t)nslots * bytes, clean)) return false;
    turb.set.assign((size_t)nslots, 0); turb.nslots = nslots;
    return true;
  }
  bool turb_slot_ok(const char* who, int slot) { return slot_ok(who, "turbulence", !turb.mem.empty(), turb.nslots, slot); }
  TurbArgs turb_args(int slot) {      // inside each_class
    TurbArgs a; a.g = g;
    a.u = ex.sh(d.f("u")); a.v = ex.sh(d.f("v")); a.pt = ex.sh(d.f("pt")); a.delp = ex.sh(d.f("delp"));
    a.nq = d.nq;
    for (int n = 0; n < d.nq; ++n) a.q[n] = ex.sh(d.q[(size_t)n]);
    a.fac = turb.slot[(size_t)slot] + ex.cls_off * g.npz; a.fs = d.n3;
    a.fro = turb.fro + ex.cls_off; a.flag = turb.flag;
    a.ptop = d.opt.ptop; a.akap = d.opt.akap; a.p00k = std::pow(1.0e5, d.opt.akap);
    a.dt = d.bdt; a.grav = d.opt.grav_jedi; a.cp = d.opt.cp; a.zvir = d.opt.zvir;
    return a;
  }
  // VTRILUPERT of the slot's three systems and pk from the resident trajectory delp; a bad pivot is reported here, by one flag
  bool turb_factorise(const char* who, int slot) {
    clear_flags(turb.flag);
    d.each_class([&]() { run_turb_factorise(ex, turb_args(slot)); });
    const int flag = read_flags(turb.flag)[0];
    turb.set[(size_t)slot] = flag ? 0 : 1;
    if (flag) return no(who, "the factorisation of a main diagonal gave a zero or non-finite pivot (slot " + std::to_string(slot) + " is not set)");
    return true;
  }
  bool turb_set_diagonals(int slot, const double* const* diag) {
    const char* who = "fv3lm_turbulence_set_diagonals";
    if (!turb_slot_ok(who, slot)) return false;
    if (!diag) return no(who, "null array");
    for (int n = 0; n < 9; ++n) if (!diag[n]) return no(who, "null array");      // before anything is touched
    turb.set[(size_t)slot] = 0;
    for (int n = 0; n < 9; ++n) d.compact_in(plane(turb.slot[(size_t)slot] + (size_t)n * d.n3, g.npz), 0, diag[n]);
    return turb_factorise(who, slot);
  }
  bool turb_set_simple(int slot, const double* frocean) {
    const char* who = "fv3lm_turbulence_set_simple";
    if (!turb_slot_ok(who, slot)) return false;
    if (d.nq < 3) return no(who, "nq < 3 (BL_simp reads qv, ql, qi = q1, q2, q3)");
    if (!frocean) return no(who, "null array");
    turb.set[(size_t)slot] = 0;
    d.compact_in(plane(turb.fro, 1), 0, frocean);
    d.each_class([&]() { run_turb_simple(ex, turb_args(slot)); });
    return turb_factorise(who, slot);
  }
  // BL_DRIVER on the resident trajectory (bldriver.h): the column's work vectors go through the slot's own planes, the nine diagonals
  // replace them, then the factorisation as after set_diagonals.  Every refusal stands before anything of the slot is touched, except
  // the parcel that never stops, which only the kernel can see: the slot is then left unset like after a zero pivot.
  bool turb_set_driver(int slot, const BlParams* p, double dt, const double* const* sfc, const double* qa, const double* qb, int cloud_mode, double* const* raw_out) {
    const char* who = "fv3lm_turbulence_set_driver";
    if (!turb_slot_ok(who, slot)) return false;
    if (g.npz < 7) return no(who, "npz < 7 (BL_DRIVER smooths the bottom six levels against the seventh)");
    if (d.nq < 1) return no(who, "nq < 1 (BL_DRIVER reads qv = q1)");
    if (!p) return no(who, "null parameters");
    if (p->i[0] < 1 || p->i[0] > g.npz) return no(who, "KPBLMIN = " + std::to_string(p->i[0]) + " outside 1.." + std::to_string(g.npz));
    if (p->i[3] != 0) return no(who, "RADLW_DEP != 0 (the reference reads an uninitialised RADLW there)");
    if (!all_finite(&dt, 1) || dt <= 0.) return no(who, "dt <= 0 or not finite");
    if (cloud_mode < 0 || cloud_mode > 1) return no(who, "cloud_mode outside 0..1");
    if (!sfc) return no(who, "null array");
    for (int n = 0; n < BL_NSFC; ++n) if (!sfc[n]) return no(who, "null array");
    if (raw_out) for (int n = 0; n < 13; ++n) if (!raw_out[n]) return no(who, "null array in raw_out");
    const size_t ss = (size_t)d.ntile_all * g.plane, n3 = d.n3;
    const bool clean = sticky_error().empty();
    if (!turb.bl_tbl) {
      turb.bl_tbl = turb.mem.get<double>((size_t)blc::TABLESIZE * 8);
      if (turb.bl_tbl) { const std::vector<double> x = bl_esinit(); h2d(ex, turb.bl_tbl, x.data(), x.size() * 8); }
    }
    if (!turb.bl_sfc) turb.bl_sfc = turb.mem.get<double>(BL_NSFC * ss * 8);
    if (raw_out && !turb.bl_raw) turb.bl_raw = turb.mem.get<double>(2 * n3 * 8);
    if (!turb.mem.ok()) {      // what was allocated stays with the feature; the next call asks for the rest again
      if (clean) sticky_error().clear();
      return no(who, "allocation failed");
    }
    turb.set[(size_t)slot] = 0;
    double* S = turb.slot[(size_t)slot];
    for (int n = 0; n < BL_NSFC; ++n) d.compact_in(plane(turb.bl_sfc + (size_t)n * ss, 1), 0, sfc[n]);
    const double* cl[2] = {qa, qb};
    for (int n = 0; n < 2; ++n) {
      double* dst = S + (size_t)(BLP_QI + n) * n3;
      if (cl[n]) d.compact_in(plane(dst, g.npz), 0, cl[n]); else dev_zero(ex, dst, n3 * 8);
    }
    clear_flags(turb.flag);
    d.each_class([&]() {
      BlArgs a; a.t = turb_args(slot); a.p = *p; a.dt = dt; a.tbl = turb.bl_tbl; a.sfc = turb.bl_sfc + ex.cls_off; a.ss = ss;
      a.ekv = raw_out ? turb.bl_raw + ex.cls_off * g.npz : nullptr; a.fkv = raw_out ? a.ekv + n3 : nullptr;
      a.cloud_mode = cloud_mode; a.flag = turb.flag + 1;
      run_bl_driver(ex, a);
    });
    if (read_flags(turb.flag)[1]) return no(who, "a column's surface parcel never reaches its level of neutral buoyancy (mpbl_depth leaves ipbl unset; slot " + std::to_string(slot) + " is not set)");
    if (raw_out) {
      for (int n = 0; n < 11; ++n) d.compact_out(plane(n < 9 ? S + (size_t)n * n3 : turb.bl_raw + (size_t)(n - 9) * n3, g.npz), 0, raw_out[n]);
      d.compact_out(plane(turb.bl_sfc + (size_t)BL_ZPBL * ss, 1), 0, raw_out[11]);
      d.compact_out(plane(turb.bl_sfc + (size_t)BL_CT * ss, 1), 0, raw_out[12]);
    }
    return turb_factorise(who, slot);
  }
  bool turb_run(int slot, int mode) {
    const char* who = "fv3lm_turbulence";
    if (!turb_slot_ok(who, slot)) return false;
    if (mode < 0 || mode > 2) return no(who, "bad mode");
    if (!slot_set(who, "slot", turb.set, slot, "fv3lm_turbulence_set_diagonals / _set_simple")) return false;
    d.each_class([&]() { run_turb_solve(ex, mode, turb_args(slot)); });
    return true;
  }
  bool turb_get(int slot, double* const* out) {
    const char* who = "fv3lm_turbulence_get";
    if (!turb_slot_ok(who, slot) || !slot_set(who, "slot", turb.set, slot, nullptr)) return false;
    if (!out) return no(who, "null array");
    for (int n = 0; n < TURB_NARR; ++n) if (!out[n]) return no(who, "null array");
    for (int n = 0; n < TURB_NARR; ++n) d.compact_out(plane(turb.slot[(size_t)slot] + (size_t)n * d.n3, g.npz), 0, out[n]);
    return true;
  }

  // ---- linearised RAS convection (convection.h) ------------------------------------------------------------------------------------------
  size_t conv_slot_doubles() const { return ((size_t)RAS_NS * (g.npz + 1) + RAS_NSC) * ncol(); }
  // fv3lm_convection_create: the slots (what set saw of the trajectory, packed columns), the table, SIGE, the four sources of the
  // perturbation and the work spaces, checkpoints and tape of one batch of columns.  All device memory of the feature is allocated here.
  bool conv_create(int nslots, const RasParams* p, int do_phy_mst) {
    const char* who = "fv3lm_convection_create";
    if (!conv.mem.empty()) return no(who, "already created for this handle");
    if (nslots < 1) return no(who, "nslots < 1");
    if (!p) return no(who, "null parameters");
    if (do_phy_mst < 1 || do_phy_mst > 2) return no(who, "do_phy_mst outside 1..2");
    if (d.ak_host.empty()) return no(who, "the handle has no ak, bk (PREF = ak + bk p00 gives ICMIN and SIGE)");
    if (d.nq < 1) return no(who, "nq < 1 (convection reads and writes qv = q1)");
    if (!all_finite(p->r, 25)) return no(who, "a value that is not finite in the parameters");
    const int lm = g.npz; const size_t nc = ncol();
    std::vector<double> sige((size_t)lm + 1);
    int cnt = 0;
    for (int l = 0; l <= lm; ++l) { sige[(size_t)l] = d.ak_host[(size_t)l] + d.bk_host[(size_t)l] * 100000.0; if (sige[(size_t)l] < 3000.0) ++cnt; }
    const double pb = sige[(size_t)lm];
    for (double& x : sige) x = x / pb;
    Convection& c = conv;
    const size_t kw = (size_t)(lm + 2 < 7 ? 7 : lm + 2), nb = nc < (size_t)RAS_BATCH ? nc : (size_t)RAS_BATCH;
    const size_t b_slot = conv_slot_doubles() * 8, b_gw = RAS_NG * kw * nb * 8, b_tw = 2 * (size_t)RAS_NT * kw * nb * 8, b_ew = ((size_t)RAS_NT + RAS_NE) * kw * nb * 8,
                 b_ck = (5 * (size_t)lm + 1) * kw * nb * 8, b_src = 4 * nc * lm * 8;
    const int cap = RAS_TAPE_PER_LEVEL * (int)kw;
    const size_t b_tape = (size_t)cap * nb * (sizeof(TapePart) + sizeof(TapeIdx) + 8);
    const size_t total = (size_t)nslots * (b_slot + nc * 4) + b_gw + b_tw + b_ew + b_ck + b_src + b_tape + (size_t)blc::TABLESIZE * 8 + sige.size() * 8 + 8;
    if (std::getenv("FV3LM_VERBOSE"))
      std::fprintf(stderr, "fv3lm: convection arena %zu bytes: %d slot(s) x %zu, batch of %d columns: work %zu, checkpoints %zu, tape %zu (%d entries a column); sources %zu\n",
                   total, nslots, b_slot + nc * 4, (int)nb, b_gw + b_tw + b_ew, b_ck, b_tape, cap, b_src);
    const bool clean = sticky_error().empty();
    // the slots and their lists are one block each, so that a request that cannot fit fails in one allocation
    const bool fits = (size_t)nslots <= ((size_t)1 << 62) / (b_slot + nc * 4);
    double* sb = nullptr; int* lb = nullptr;
    if (fits) { sb = c.mem.get<double>((size_t)nslots * b_slot); lb = c.mem.get<int>((size_t)nslots * nc * 4); } else c.mem.refuse();
    c.w = batch_work(c.mem, b_gw, b_tw, b_ew, b_ck, cap, nb);
    c.src = c.mem.get<double>(b_src); c.tbl = c.mem.get<double>((size_t)blc::TABLESIZE * 8); c.sige = c.mem.get<double>(sige.size() * 8);
    if (!allocated(who, c, total, clean)) return false;
    for (int n = 0; n < nslots; ++n) { c.slot.push_back(sb + (size_t)n * (b_slot / 8)); c.list.push_back(lb + (size_t)n * nc); }
    { const std::vector<double> x = bl_esinit(); h2d(ex, c.tbl, x.data(), x.size() * 8); }
    h2d(ex, c.sige, sige.data(), sige.size() * 8);
    c.p = *p; c.mst = do_phy_mst; c.icmin = cnt > 1 ? cnt : 1;
    c.set.assign((size_t)nslots, 0); c.nactive.assign((size_t)nslots, 0); c.nslots = nslots;
    return true;
  }
  bool conv_slot_ok(const char* who, int slot) { return slot_ok(who, "convection", !conv.mem.empty(), conv.nslots, slot); }
  bool conv_slot_set(const char* who, int slot) { return slot_set(who, "slot", conv.set, slot, "fv3lm_convection_set"); }
  RasArgs conv_args(int slot) {
    RasArgs a;
    static_cast<ColView&>(a) = col_view(conv.slot[(size_t)slot], RAS_NS); static_cast<ColWork&>(a) = conv.w;
    a.icmin = conv.icmin; a.mst = conv.mst;
    a.u = ex.sh(d.f("u")); a.v = ex.sh(d.f("v")); a.pt = ex.sh(d.f("pt")); a.delp = ex.sh(d.f("delp")); a.q1 = ex.sh(d.q[0]);
    a.src = conv.src; a.tbl = conv.tbl; a.sige = conv.sige; a.p = conv.p;
    a.dt = d.bdt; a.ptop = d.opt.ptop; a.akap = d.opt.akap; a.p00k = std::pow(1.0e5, d.opt.akap);
    return a;
  }
  // the slot takes the trajectory from the resident u v pt(= T) delp q1 at this call; RASE0, the two filters and the list of DOCONVEC columns
  bool conv_set(int slot, const double* ts, const double* frland, const double* kcbl) {
    const char* who = "fv3lm_convection_set";
    if (!conv_slot_ok(who, slot)) return false;
    if (!ts || !frland || !kcbl) return no(who, "null array");
    const size_t nc = ncol(); const int lm = g.npz;
    for (size_t n = 0; n < nc; ++n) {
      if (!all_finite(ts + n, 1) || !all_finite(frland + n, 1) || !all_finite(kcbl + n, 1)) return no(who, "a value that is not finite in ts, frland or kcbl");
      const long k = std::lround(kcbl[n]);
      if (k < conv.icmin + 1 || k > lm) return no(who, "kcbl = " + std::to_string(k) + " outside ICMIN+1 .. npz = " + std::to_string(conv.icmin + 1) + " .. " + std::to_string(lm));
    }
    conv.set[(size_t)slot] = 0;
    if (!cld.mem.empty()) cld.set[(size_t)slot] = 0;      // the cloud slot reads this one: it has to be set again after it
    std::vector<double> kc(nc);
    for (size_t n = 0; n < nc; ++n) kc[n] = (double)std::lround(kcbl[n]);      // nint
    RasArgs a = conv_args(slot);
    h2d(ex, &a.SC(SC_TS, 0), ts, nc * 8); h2d(ex, &a.SC(SC_FRLAND, 0), frland, nc * 8); h2d(ex, &a.SC(SC_KCBL, 0), kc.data(), nc * 8);
    clear_flags(conv.w.flag);
    a.first = 0; a.n = (int)nc;
    run_ras(ex, -2, a);
    if (read_flags(conv.w.flag)[0]) return no(who, "a value that is not finite in the resident trajectory (slot " + std::to_string(slot) + " is not set)");
    for_batches(nc, (size_t)conv.w.nb, [&](int first, int n) { a.first = first; a.n = n; run_ras(ex, -1, a); });
    std::vector<double> dc(nc);
    d2h(ex, dc.data(), &a.SC(SC_DOCONVEC, 0), nc * 8);
    std::vector<int> list;
    for (size_t n = 0; n < nc; ++n) if (dc[n] == 1.0) list.push_back((int)n);
    if (!list.empty()) h2d(ex, conv.list[(size_t)slot], list.data(), list.size() * 4);
    conv.nactive[(size_t)slot] = (int)list.size();
    if (!sticky_clean()) return false;
    conv.set[(size_t)slot] = 1;
    return true;
  }
  bool conv_get(int slot, double* const* out6, int* doconvec, double* jac2) {
    const char* who = "fv3lm_convection_get";
    if (!conv_slot_ok(who, slot) || !conv_slot_set(who, slot)) return false;
    if (!out6 || !doconvec) return no(who, "null array");
    for (int n = 0; n < 6; ++n) if (!out6[n]) return no(who, "null array");
    const size_t nc = ncol(); const int lm = g.npz;
    const RasArgs a = conv_args(slot);
    std::vector<double> buf((size_t)(lm + 1) * nc);
    for (int n = 0; n < 6; ++n) unpack_columns(&a.S(S_OUT + n, 0, 0), out6[n], buf);
    if (jac2) { unpack_columns(&a.S(S_JAC, 0, 0), jac2, buf); unpack_columns(&a.S(S_JAC + 1, 0, 0), jac2 + (size_t)lm * nc, buf); }
    d2h(ex, buf.data(), &a.SC(SC_DOCONVEC, 0), nc * 8);
    for (size_t n = 0; n < nc; ++n) doconvec[n] = (int)buf[n];
    return true;
  }
  bool conv_sources(int put, double* const* src4) {
    const char* who = "fv3lm_convection_sources";
    if (conv.mem.empty()) return no(who, "call fv3lm_convection_create first");
    if (!src4) return no(who, "null array");
    for (int n = 0; n < 4; ++n) if (!src4[n]) return no(who, "null array");
    const size_t n3c = ncol() * g.npz;
    if (put) for (int n = 0; n < 4; ++n) if (!all_finite(src4[n], n3c)) return no(who, "a value that is not finite");
    for (int n = 0; n < 4; ++n) { if (put) h2d(ex, conv.src + (size_t)n * n3c, src4[n], n3c * 8); else d2h(ex, src4[n], conv.src + (size_t)n * n3c, n3c * 8); }
    return true;
  }
  // the table the kernels look up (ESINIT) as it lies on the device, and the nine constants they use, in the order of the fixture
  bool conv_table(double* table, double* constants) {
    const char* who = "fv3lm_convection_table";
    if (conv.mem.empty()) return no(who, "call fv3lm_convection_create first");
    if (!table || !constants) return no(who, "null array");
    d2h(ex, table, conv.tbl, (size_t)blc::TABLESIZE * 8);
    const double c[9] = {rasc::CP, rasc::ALHL, rasc::GRAV, rasc::RGAS, rasc::H2OMW, rasc::AIRMW, rasc::VIREPS, blc::P00, blc::KAPPA};
    for (int n = 0; n < 9; ++n) constants[n] = c[n];
    return true;
  }
  // DOCONVEC columns only, in dense batches over the slot's list.  Tangent: the sources are cleared, then written in the active columns;
  // adjoint: the sources are the incoming adjoints, consumed and cleared.  The slot is read only.
  bool conv_run(int slot, int mode) {
    const char* who = "fv3lm_convection";
    if (!conv_slot_ok(who, slot)) return false;
    if (mode < 0 || mode > 2) return no(who, "bad mode");
    if (!conv_slot_set(who, slot)) return false;
    RasArgs a = conv_args(slot);
    a.list = conv.list[(size_t)slot];
    const size_t n3c = ncol() * g.npz;
    if (mode == MODE_TL) dev_zero(ex, conv.src, 4 * n3c * 8);
    if (mode == MODE_AD) clear_flags(conv.w.flag);
    for_batches((size_t)conv.nactive[(size_t)slot], (size_t)conv.w.nb, [&](int first, int n) { a.first = first; a.n = n; run_ras(ex, mode, a); });
    if (mode == MODE_AD) {
      dev_zero(ex, conv.src, 4 * n3c * 8);
      if (read_flags(conv.w.flag)[1]) return no(who, "the tape of a cloud type overflowed (RAS_TAPE_PER_LEVEL); the adjoint fields are not valid");
    }
    return sticky_clean();
  }

  // ---- linearised cloud scheme (cloud.h) -----------------------------------------------------------------------------------------------------
  size_t cloud_slot_doubles() const { return ((size_t)CLD_NS * (g.npz + 1) + CLD_NSC) * ncol(); }
  // fv3lm_cloud_create: one slot per convection slot, the perturbation's convective cloud fraction and the work spaces, checkpoints and tape
  // of one batch of columns.  All device memory of the feature is allocated here.
  bool cloud_create(const CldParams* p, int iqi, int iql) {
    const char* who = "fv3lm_cloud_create";
    const int nq = d.nq;
    if (conv.mem.empty()) return no(who, "call fv3lm_convection_create first");
    if (!cld.mem.empty()) return no(who, "already created for this handle");
    if (!p) return no(who, "null parameters");
    if (!all_finite(p->r, 57)) return no(who, "a value that is not finite in the parameters");
    if ((int)p->r[56] != 1) return no(who, "CLOUDPARAMS(57) = PDFFLAG /= 1 (only the top-hat PDF is built)");
    if ((int)(p->r[34] + .001) < 1) return no(who, "CLOUDPARAMS(35) = ICEFRPWR < 1");
    if (iqi < 2 || iqi > nq || iql < 2 || iql > nq) return no(who, "iqi = " + std::to_string(iqi) + ", iql = " + std::to_string(iql) + " outside 2..nq = 2.." + std::to_string(nq));
    if (iqi == iql) return no(who, "iqi = iql = " + std::to_string(iqi) + " (cloud ice and cloud liquid are two tracers)");
    const int lm = g.npz, nslots = conv.nslots; const size_t nc = ncol();
    Cloud& c = cld;
    const size_t kw = (size_t)(lm + 2 < CLD_NSV + 2 ? CLD_NSV + 2 : lm + 2), nb = nc < (size_t)CLD_BATCH ? nc : (size_t)CLD_BATCH;
    const size_t b_slot = cloud_slot_doubles() * 8, b_gw = CLD_NG * kw * nb * 8, b_tw = 2 * (size_t)CLD_NE * kw * nb * 8, b_ew = 2 * (size_t)CLD_NE * kw * nb * 8,
                 b_ck = ((size_t)CLD_NCK + 1) * kw * nb * 8, b_cf = nc * lm * 8;
    const int cap = CLD_TAPE;
    const size_t b_tape = (size_t)cap * nb * (sizeof(TapePart) + sizeof(TapeIdx) + 8);
    const size_t total = (size_t)nslots * b_slot + b_gw + b_tw + b_ew + b_ck + b_cf + b_tape + 8;
    if (std::getenv("FV3LM_VERBOSE"))
      std::fprintf(stderr, "fv3lm: cloud arena %zu bytes: %d slot(s) x %zu, batch of %d columns: work %zu, checkpoints %zu, tape %zu (%d entries a column); cfcn %zu\n",
                   total, nslots, b_slot, (int)nb, b_gw + b_tw + b_ew, b_ck, b_tape, cap, b_cf);
    const bool clean = sticky_error().empty();
    double* sb = c.mem.get<double>((size_t)nslots * b_slot);
    c.w = batch_work(c.mem, b_gw, b_tw, b_ew, b_ck, cap, nb);
    c.cfcn = c.mem.get<double>(b_cf);
    if (!allocated(who, c, total, clean)) return false;
    for (int n = 0; n < nslots; ++n) c.slot.push_back(sb + (size_t)n * (b_slot / 8));
    dev_zero(ex, c.cfcn, b_cf);
    c.p = *p; c.iqi = iqi; c.iql = iql; c.set.assign((size_t)nslots, 0);
    return true;
  }
  bool cloud_slot_ok(const char* who, int slot, bool need_set) {
    if (!slot_ok(who, "cloud", !cld.mem.empty(), conv.nslots, slot)) return false;
    if (!slot_set(who, "the convection slot", conv.set, slot, "fv3lm_convection_set")) return false;
    return !need_set || slot_set(who, "slot", cld.set, slot, "fv3lm_cloud_set");
  }
  // fv3lm_cloud_bind_cfcn: from here on the convective cloud fraction is tracer iqc of the dycore, as the reference's fifth tracer
  // (fv3jedi_lm_dynamics_mod.F90:159-163, :769, :831, :878, :912): the trajectory half is the trajectory cfcn, the perturbation half is
  // cfcn' or its adjoint, and the dynamics carries both.  The feature's own array stays allocated and is no longer read.
  bool cloud_bind_cfcn(int iqc) {
    const char* who = "fv3lm_cloud_bind_cfcn";
    if (cld.mem.empty()) return no(who, "call fv3lm_cloud_create first");
    if (cld.iqc) return no(who, "already bound to tracer " + std::to_string(cld.iqc));
    if (iqc < 2 || iqc > d.nq) return no(who, "iqc = " + std::to_string(iqc) + " outside 2..nq = 2.." + std::to_string(d.nq));
    if (iqc == cld.iqi || iqc == cld.iql)
      return no(who, "iqc = " + std::to_string(iqc) + " is the tracer of cloud " + (iqc == cld.iqi ? "ice (iqi)" : "liquid (iql)") + ": cfcn is a tracer of its own");
    if (cld.was_set) return no(who, "a cloud slot has been set: bind after fv3lm_cloud_create, before the first fv3lm_cloud_set");
    cld.iqc = iqc;
    return true;
  }
  CldArgs cloud_args(int slot) {
    CldArgs a;
    static_cast<ColView&>(a) = col_view(cld.slot[(size_t)slot], CLD_NS); static_cast<ColWork&>(a) = cld.w;
    a.rslot = conv.slot[(size_t)slot]; a.mst = conv.mst;
    a.pt = ex.sh(d.f("pt")); a.delp = ex.sh(d.f("delp")); a.q1 = ex.sh(d.q[0]);
    a.qi = ex.sh(d.q[(size_t)cld.iqi - 1]); a.ql = ex.sh(d.q[(size_t)cld.iql - 1]);
    a.cfcn = cld.cfcn; a.cfcn_t = nullptr; a.cf_fld = 0;
    if (cld.iqc) { const Fld qc = ex.sh(d.q[(size_t)cld.iqc - 1]); a.cfcn = qc.p; a.cfcn_t = qc.t; a.cf_fld = 1; }
    a.src = conv.src; a.tbl = conv.tbl; a.p = cld.p;
    a.dt = d.bdt; a.ptop = d.opt.ptop; a.p00k = std::pow(1.0e5, d.opt.akap);
    return a;
  }
  // the slot takes QLS QCN cfcn khl khu from the host, PLE from the resident delp and everything else from the convection slot of the same
  // number; the split, the fractions, CLOUD_DRIVER in values and (do_phy_mst = 2) the per-cell switch.  With a bound tracer a null cfcn
  // takes the resident trajectory of that tracer (set_ltraj :720)
  bool cloud_set(int slot, const double* qls, const double* qcn, const double* cfcn, const double* khl, const double* khu) {
    const char* who = "fv3lm_cloud_set";
    if (!cloud_slot_ok(who, slot, false)) return false;
    if (!qls || !qcn || (!cfcn && !cld.iqc) || !khl || !khu) return no(who, "null array");
    const size_t nc = ncol(); const int lm = g.npz;
    if (!all_finite(qls, nc * lm) || !all_finite(qcn, nc * lm) || (cfcn && !all_finite(cfcn, nc * lm))) return no(who, "a value that is not finite in QLS, QCN or cfcn");
    for (size_t n = 0; n < nc; ++n) {
      if (!all_finite(khl + n, 1) || !all_finite(khu + n, 1)) return no(who, "a value that is not finite in khl or khu");
      const long l = std::lround(khl[n]), u = std::lround(khu[n]);
      if (l < 1 || l > lm || u < 1 || u > lm) return no(who, "khl = " + std::to_string(l) + ", khu = " + std::to_string(u) + " outside 1..npz = 1.." + std::to_string(lm));
    }
    cld.set[(size_t)slot] = 0;
    CldArgs a = cloud_args(slot);
    std::vector<double> buf((size_t)(lm + 1) * nc, 0.);
    pack_columns(&a.S(CS_QILS, 0, 0), qls, buf); pack_columns(&a.S(CS_QICN, 0, 0), qcn, buf);
    if (cfcn) pack_columns(&a.S(CS_CFCN, 0, 0), cfcn, buf);
    std::vector<double> kh(2 * nc);
    for (size_t n = 0; n < nc; ++n) { kh[n] = (double)std::lround(khl[n]); kh[nc + n] = (double)std::lround(khu[n]); }      // nint
    h2d(ex, &a.SC(CSC_KHL, 0), kh.data(), kh.size() * 8);
    clear_flags(cld.w.flag);
    cld.was_set = true;
    if (!cfcn) for_batches(nc, (size_t)cld.w.nb, [&](int first, int n) { a.first = first; a.n = n; run_cloud(ex, -2, a); });
    for_batches(nc, (size_t)cld.w.nb, [&](int first, int n) { a.first = first; a.n = n; run_cloud(ex, -1, a); });
    if (read_flags(cld.w.flag)[0]) return no(who, "a value that is not finite in the resident trajectory (slot " + std::to_string(slot) + " is not set)");
    if (!sticky_clean()) return false;
    cld.set[(size_t)slot] = 1;
    return true;
  }
  bool cloud_get(int slot, double* const* out8, double* const* frac4, int* pertmod) {
    const char* who = "fv3lm_cloud_get";
    if (!cloud_slot_ok(who, slot, true)) return false;
    if (out8) for (int n = 0; n < 8; ++n) if (!out8[n]) return no(who, "null array");
    if (frac4) for (int n = 0; n < 4; ++n) if (!frac4[n]) return no(who, "null array");
    const CldArgs a = cloud_args(slot);
    std::vector<double> buf((size_t)(g.npz + 1) * ncol());
    if (out8) for (int n = 0; n < 8; ++n) unpack_columns(&a.S(CS_OUT + n, 0, 0), out8[n], buf);
    if (frac4) for (int n = 0; n < 4; ++n) unpack_columns(&a.S(CS_FRAC + n, 0, 0), frac4[n], buf);
    if (pertmod) unpack_columns(&a.S(CS_PMOD, 0, 0), pertmod, buf);
    return true;
  }
  bool cloud_cfcn(int put, double* cfcn) {
    const char* who = "fv3lm_cloud_cfcn";
    if (cld.mem.empty()) return no(who, "call fv3lm_cloud_create first");
    if (!cfcn) return no(who, "null array");
    const size_t n3c = ncol() * g.npz;
    if (put && !all_finite(cfcn, n3c)) return no(who, "a value that is not finite");
    if (cld.iqc) {      // bound: is..ie x js..je of the tracer's perturbation; a put leaves zeros outside, as pert_to_fv3 does
      const Fld& qc = d.q[(size_t)cld.iqc - 1];
      if (put) d.compact_in(qc, 1, cfcn); else d.compact_out(qc, 1, cfcn);
      return sticky_clean();
    }
    if (put) h2d(ex, cld.cfcn, cfcn, n3c * 8); else d2h(ex, cfcn, cld.cfcn, n3c * 8);
    return true;
  }
  // every column, in dense batches.  The slot is read only; mode 0 writes the trajectory tracers iqi, iql and, bound, CF_con to iqc
  bool cloud_run(int slot, int mode) {
    const char* who = "fv3lm_cloud";
    if (!cloud_slot_ok(who, slot, false)) return false;
    if (mode < 0 || mode > 2) return no(who, "bad mode");
    if (!cloud_slot_ok(who, slot, true)) return false;
    CldArgs a = cloud_args(slot);
    if (mode == MODE_AD) clear_flags(cld.w.flag);
    for_batches(ncol(), (size_t)cld.w.nb, [&](int first, int n) { a.first = first; a.n = n; run_cloud(ex, mode, a); });
    if (mode == MODE_NL && cld.iqc) for_batches(ncol(), (size_t)cld.w.nb, [&](int first, int n) { a.first = first; a.n = n; run_cloud(ex, -3, a); });
    if (mode == MODE_AD && read_flags(cld.w.flag)[1]) return no(who, "the tape of a segment overflowed (CLD_TAPE); the adjoint fields are not valid");
    return sticky_clean();
  }
};

}  // namespace fv3
