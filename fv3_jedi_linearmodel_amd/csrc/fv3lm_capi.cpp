// fv3lm-hip: implementation of the C-ABI declared in include/fv3lm.h.
// Built with `hipcc -x hip --offload-arch=gfx950` into libfv3lm_hip.so (the product), and with
// `g++ -DFV3LM_HOST_EMUL` into tests/_emul/libfv3lm_emul.so (test-only host emulation, never
// loaded by the package).
#include "model.h"
#include <array>
#include <string>

using namespace fv3;

struct fv3lm_handle { Dynamics d; Physics p{d}; Model m{d, p}; };

static thread_local std::string g_err;
static int fail(const std::string& m) { g_err = m; return 1; }
static int g_live = 0;      // handles alive in this process (one per GPU / MPI rank in production; tests create several)

extern "C" {

const char* fv3lm_last_error(void) { return g_err.c_str(); }

const char* fv3lm_metric_names(void) {
  return "area,rarea,rarea_c,dx,dy,dxa,dya,dxc,dyc,rdx,rdy,rdxa,rdya,rdxc,rdyc,cosa,sina,rsina,cosa_u,cosa_v,cosa_s,"
         "sina_u,sina_v,rsin_u,rsin_v,rsin2,f0,fC,del6_u,del6_v,divg_u,divg_v,"
         "sin_sg1,sin_sg2,sin_sg3,sin_sg4,sin_sg5,sin_sg6,sin_sg7,sin_sg8,sin_sg9,"
         "cos_sg1,cos_sg2,cos_sg3,cos_sg4,cos_sg5,cos_sg6,cos_sg7,cos_sg8,cos_sg9";
}

int fv3lm_create(fv3lm_handle** out, const fv3lm_dims* dm, const fv3lm_options* opt, const double* const* metrics,
                 double da_min, double da_min_c, const double* phis, const double* ak, const double* bk) {
  if (!out || !dm || !opt || !metrics) return fail("fv3lm_create: null argument");
#ifndef FV3LM_HOST_EMUL
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail("fv3lm_create: no HIP device visible (this library has no CPU fallback)");
#endif
  // The failure record is per process (exec.h sticky_error): a fault of a LIVE handle that no call has reported yet must not be erased by
  // the creation of another one -- that create fails with it instead; with no handle alive there is nobody left to report it to.
  if (!sticky_error().empty()) {
    if (g_live > 0) return fail("fv3lm_create: an earlier failure of a live handle is pending: " + sticky_error());
    sticky_error().clear();
  }
  fv3lm_handle* h = new fv3lm_handle;
  // every failure path releases what was allocated so far (destroy2 / destroy accept a partly built object); the failure is reported here, once
  auto bail = [&](std::string e) { h->m.release(); h->p.release(); h->d.destroy2(); h->d.destroy(); delete h; sticky_error().clear(); return fail("fv3lm_create: " + e); };   // e by value: it may live in *h
  if (!h->d.init(dm->nx, dm->ny, dm->npz, dm->ntile, dm->face, dm->nq, dm->dt, dm->n_split, dm->k_split, *opt, metrics, da_min,
                 da_min_c, phis, dm->nface, dm->tile_ij0)) return bail(h->d.err);
  if (!sticky_error().empty()) return bail(sticky_error());
  if (!h->d.init2(ak, bk)) return bail(h->d.err);
  if (!sticky_error().empty()) return bail(sticky_error());
  *out = h;
  ++g_live;
  return 0;
}

int fv3lm_destroy(fv3lm_handle* h) {
  if (!h) return 0;
  h->m.release(); h->p.release(); h->d.destroy2(); h->d.destroy(); delete h;
  if (--g_live <= 0) { g_live = 0; sticky_error().clear(); }      // the last handle takes its unreported failures with it
  return 0;
}

static bool find(fv3lm_handle* h, const char* name, Fld& f) {
  if (std::string(name) == "phis") { f = Fld{}; f.t = h->d.hs_dev; f.p = h->d.hs_dev; f.nk = 1; return true; }      // surface geopotential, one padded plane per tile (trajectory only)
  auto it = h->d.F.find(name);
  if (it == h->d.F.end()) { g_err = std::string("unknown field ") + name; return false; }
  f = it->second; return true;
}
int fv3lm_field_levels(fv3lm_handle* h, const char* name) { Fld f; return find(h, name, f) ? f.nk : -1; }
int fv3lm_field_put(fv3lm_handle* h, const char* name, int which, const double* host) {
  Fld f; if (!find(h, name, f)) return 1;
  h2d(h->d.ex, which ? f.p : f.t, host, (size_t)h->d.g.ntile * f.nk * h->d.g.plane * 8);
  return sticky_error().empty() ? 0 : fail(sticky_error());
}
int fv3lm_field_get(fv3lm_handle* h, const char* name, int which, double* host) {
  Fld f; if (!find(h, name, f)) return 1;
  d2h(h->d.ex, host, which ? f.p : f.t, (size_t)h->d.g.ntile * f.nk * h->d.g.plane * 8);
  return sticky_error().empty() ? 0 : fail(sticky_error());
}
// sticky conditions a sweep may have run into
static int status(fv3lm_handle* h) {
#ifndef FV3LM_HOST_EMUL
  { const hipError_t e = hipGetLastError();      // launch-time failures (bad configuration, out of resources) of the kernels queued so far
    if (e != hipSuccess) set_sticky(std::string("HIP kernel launch failed: ") + hipGetErrorString(e)); }
  if (const char* dbg = std::getenv("FV3LM_DEBUG_SYNC")) if (dbg[0] == '1') {   // debug runs: execution-time faults surface at the call that caused them
    const hipError_t e = hipStreamSynchronize(h->d.ex.stream);
    if (e != hipSuccess) set_sticky(std::string("HIP stream failed: ") + hipGetErrorString(e));
  }
#endif
  const std::string e = pending_failure(h->d);
  return e.empty() ? 0 : fail(e);
}
int fv3lm_set_face_data(fv3lm_handle* h, const double* edge, const double* ecorner) {
  if (!edge || !ecorner) return fail("fv3lm_set_face_data: null argument");
  return h->d.set_face_data(edge, ecorner) ? 0 : fail(h->d.err);
}
int fv3lm_set_rayleigh(fv3lm_handle* h, double tau, double rf_cutoff, const double* c2l) {
  if (!h) return fail("fv3lm_set_rayleigh: null handle");
  if (!h->d.set_rayleigh(tau, rf_cutoff, c2l)) return fail(h->d.err);
  return status(h);
}
int fv3lm_rayleigh_profile(fv3lm_handle* h, double* rf, int* kmax) {
  if (!h || !rf || !kmax) return fail("fv3lm_rayleigh_profile: null argument");
  for (int k = 0; k < h->d.g.npz; ++k) rf[k] = k < (int)h->d.rf_host.size() ? h->d.rf_host[(size_t)k] : 0.;
  *kmax = h->d.rf_kmax;
  return 0;
}
int fv3lm_set_tracer_damping(fv3lm_handle* h, int nord_tr, double trdm2, int nord_tr_pert, double trdm2_pert, int split_damp_tr) {
  if (!h) return fail("fv3lm_set_tracer_damping: null handle");
  if (!h->d.set_tracer_damping(nord_tr, trdm2, nord_tr_pert, trdm2_pert, split_damp_tr)) return fail(h->d.err);
  return status(h);
}
int fv3lm_tracer_damping(fv3lm_handle* h, int* nord2, double* trdm2) {
  if (!h || !nord2 || !trdm2) return fail("fv3lm_tracer_damping: null argument");
  const LevelParams& l = h->d.lev_host[0];
  nord2[0] = l.nord_tr; nord2[1] = l.nord_tr_p; trdm2[0] = l.trdm2; trdm2[1] = l.trdm2_p;
  return 0;
}
int fv3lm_set_external_damping(fv3lm_handle* h, double d_ext) {
  if (!h) return fail("fv3lm_set_external_damping: null handle");
  if (!h->d.set_external_damping(d_ext)) return fail(h->d.err);
  return status(h);
}
int fv3lm_external_damping(fv3lm_handle* h, double* d_ext) {
  if (!h || !d_ext) return fail("fv3lm_external_damping: null argument");
  *d_ext = h->d.d_ext;
  return 0;
}
int fv3lm_set_trajectory_damping_order(fv3lm_handle* h, int nord) {
  if (!h) return fail("fv3lm_set_trajectory_damping_order: null handle");
  if (!h->d.set_trajectory_damping_order(nord)) return fail(h->d.err);
  return status(h);
}
int fv3lm_trajectory_damping_order(fv3lm_handle* h, int* nord) {
  if (!h || !nord) return fail("fv3lm_trajectory_damping_order: null argument");
  *nord = h->d.opt.nord;
  return 0;
}
int fv3lm_set_exchange(fv3lm_handle* h, int kind, const int* rows, int nrows) {
  if (!rows && nrows > 0) return fail("fv3lm_set_exchange: null table");
  return h->d.set_exchange(kind, rows, nrows) ? 0 : fail(h->d.err);
}
int fv3lm_set_exchange_remote(fv3lm_handle* h, int kind, int npeers, const int* peers, const int* nsend, const int* send_rows, const int* nrecv,
                              const int* recv_rows) {
  return h->d.set_exchange_remote(kind, npeers, peers, nsend, send_rows, nrecv, recv_rows) ? 0 : fail(h->d.err);
}
// Transport between ranks.  Product: RCCL point-to-point on the library stream (library path = the RCCL the process already
// uses, e.g. torch's; the 128-byte unique id comes from rank 0 and is distributed by the host).  Callback: host-emulation tests.
int fv3lm_comm_unique_id(const char* rccl_path, void* id128) {
#ifndef FV3LM_HOST_EMUL
  std::string e; Transport& T = transport();
  if (!T.load(rccl_path, e)) return fail(e);
  ncclUniqueId id;
  if (T.pGetUniqueId(&id) != ncclSuccess) return fail("ncclGetUniqueId failed");
  std::memcpy(id128, &id, sizeof id);
  return 0;
#else
  (void)rccl_path; (void)id128; return fail("host emulation has no RCCL; use fv3lm_set_transport_callback");
#endif
}
int fv3lm_comm_init(const char* rccl_path, const void* id128, int nranks, int rank) {
#ifndef FV3LM_HOST_EMUL
  std::string e; Transport& T = transport();
  if (!T.load(rccl_path, e)) return fail(e);
  ncclUniqueId id; std::memcpy(&id, id128, sizeof id);
  if (T.pCommInitRank(&T.comm, nranks, id, rank) != ncclSuccess) return fail("ncclCommInitRank failed");
  T.rank = rank; T.nranks = nranks;
  return 0;
#else
  (void)rccl_path; (void)id128; (void)nranks; (void)rank; return fail("host emulation has no RCCL; use fv3lm_set_transport_callback");
#endif
}
int fv3lm_comm_destroy(void) {
#ifndef FV3LM_HOST_EMUL
  Transport& T = transport();
  if (T.comm && T.pCommDestroy) T.pCommDestroy(T.comm);
  T.comm = nullptr;
#endif
  return 0;
}
int fv3lm_set_allreduce_callback(fv3lm_allreduce_fn fn, void* user) { allreduce_max_hook().cb = fn; allreduce_max_hook().user = user; return 0; }
int fv3lm_set_transport_callback(fv3lm_transport_fn fn, void* user) { transport().cb = fn; transport().user = user; return 0; }
int fv3lm_halo(fv3lm_handle* h, int kind, const char* name0, const char* name1, int mode) {
  if (mode < 0 || mode > 2 || kind < 0 || kind >= H_NKIND) return fail("bad mode or kind");
  Fld f0, f1{};
  auto it = h->d.F.find(name0);
  if (it == h->d.F.end()) return fail(std::string("unknown field ") + name0);
  f0 = it->second;
  if (name1 && name1[0]) { it = h->d.F.find(name1); if (it == h->d.F.end()) return fail(std::string("unknown field ") + name1); f1 = it->second; }
  h->d.halo(mode, kind, f0, f1);
  return status(h);
}
int fv3lm_run_group(fv3lm_handle* h, const char* group, int mode) {
  if (mode < 0 || mode > 2) return fail("bad mode");
  // one group on its own: every adjoint launch accumulates (the stored-first-write plan of Dycore::plan_adjoint belongs to the whole sweep)
  h->d.ex.no_wmask = group && group[0];
  h->d.run_group(h->d.acoustic, group, mode);
  h->d.ex.no_wmask = false;
  return status(h);
}
int fv3lm_dyn_core(fv3lm_handle* h, int mode) {
  if (mode < 0 || mode > 2) return fail("bad mode");
  h->d.dyn_core(mode);
  return status(h);
}
int fv3lm_pressures(fv3lm_handle* h, int mode) { h->d.pressures(mode); return status(h); }
int fv3lm_tracer_2d(fv3lm_handle* h, int mode) {
  if (mode == MODE_AD) h->d.tracer_ad(); else h->d.tracer_fwd(mode);
  return status(h);
}
int fv3lm_traj_slots(fv3lm_handle* h) { return (int)h->d.traj_slot.size(); }   /* acoustic steps whose intermediates stay resident */
int fv3lm_tracer_nsplt(fv3lm_handle* h) { return h->d.nsplt_max; }   /* largest sub-step count tracer_2d has used so far */
int fv3lm_remap(fv3lm_handle* h, int mode, int last_step) {
  if (mode < 0 || mode > 2) return fail("bad mode");
  if (h->d.nh) h->d.remap_nh_run(mode, last_step != 0);      // w and delz mapped, pt as density temperature through delz
  else h->d.each_class([&]() { run_remap(h->d.ex, mode, h->d.remap_args(last_step != 0)); });
  return status(h);
}
int fv3lm_fv_dynamics(fv3lm_handle* h, int mode) { h->d.fv_dynamics(mode); return status(h); }
int fv3lm_rayleigh(fv3lm_handle* h, int mode) {
  if (mode < 0 || mode > 2) return fail("bad mode");
  h->d.rayleigh(mode);
  return status(h);
}
// an entry point of the column physics (physics.h): the call's own refusal comes back through the handle's error string
extern "C++" {
template <class Fn> static int physics_call(fv3lm_handle* h, const char* name, const Fn& fn) {
  if (!h) return fail(std::string(name) + ": null handle");
  if (!fn(h->p)) return fail(h->d.err);
  return status(h);
}
}
// linearised boundary-layer turbulence (turbulence.h)
int fv3lm_turbulence_create(fv3lm_handle* h, int nslots) {
  return physics_call(h, "fv3lm_turbulence_create", [&](Physics& p_) { return p_.turb_create(nslots); });
}
int fv3lm_turbulence_set_diagonals(fv3lm_handle* h, int slot, const double* const* diag) {
  return physics_call(h, "fv3lm_turbulence_set_diagonals", [&](Physics& p_) { return p_.turb_set_diagonals(slot, diag); });
}
int fv3lm_turbulence_set_simple(fv3lm_handle* h, int slot, const double* frocean) {
  return physics_call(h, "fv3lm_turbulence_set_simple", [&](Physics& p_) { return p_.turb_set_simple(slot, frocean); });
}
void fv3lm_bl_default_params(fv3lm_bl_params* p, int kpblmin) {      // bldriver.F90:100-127
  if (!p) return;
  const double r[22] = {5.0, 160.0, 1.0, 160.0, 1.0, 3000., 3000., 0.1, 0.0030, 2.5101471e-8, 1500., 500., 1.0, 0.75, 0.50, 0.25, 0.85, 0.45, 20.0, 1.5e-3, 0.5, -999.};
  for (int n = 0; n < 22; ++n) p->r[n] = r[n];
  p->i[0] = kpblmin; p->i[1] = 1; p->i[2] = 1; p->i[3] = 0;
}
int fv3lm_turbulence_set_driver(fv3lm_handle* h, int slot, const fv3lm_bl_params* p, double dt, const double* const* sfc, const double* qa,
                                const double* qb, int cloud_mode, double* const* raw_out) {
  static_assert(sizeof(fv3lm_bl_params) == sizeof(BlParams), "fv3lm_bl_params and BlParams must agree");
  return physics_call(h, "fv3lm_turbulence_set_driver", [&](Physics& p_) { return p_.turb_set_driver(slot, reinterpret_cast<const BlParams*>(p), dt, sfc, qa, qb, cloud_mode, raw_out); });
}
int fv3lm_turbulence(fv3lm_handle* h, int slot, int mode) {
  return physics_call(h, "fv3lm_turbulence", [&](Physics& p_) { return p_.turb_run(slot, mode); });
}
int fv3lm_turbulence_get(fv3lm_handle* h, int slot, double* const* out) {
  return physics_call(h, "fv3lm_turbulence_get", [&](Physics& p_) { return p_.turb_get(slot, out); });
}
// linearised RAS convection (convection.h)
void fv3lm_ras_default_params(fv3lm_ras_params* p, int im) {      // fv3jedi_lm_moist_mod.F90:120-148
  if (!p) return;
  const double r[25] = {1.000, 0.05, 0.0, 8.0e-4, 1800., 43200.0, -300., 4.0, 0.0, 200., 7.5e-4, 1.0, -1.0, 1.3, 1.3, 263., 0.5, 1.0, 0.0, 0.1, 0.8, 1.0, 0.0, 0.5, 0.65};
  for (int n = 0; n < 25; ++n) p->r[n] = r[n];
  const long imsize = 4L * im;
  p->r[22] = imsize <= 200 ? 4000.0 : imsize <= 400 ? 2000.0 : imsize <= 800 ? 700.0 : 450.0;
}
int fv3lm_convection_create(fv3lm_handle* h, int nslots, const fv3lm_ras_params* p, int do_phy_mst) {
  static_assert(sizeof(fv3lm_ras_params) == sizeof(RasParams), "fv3lm_ras_params and RasParams must agree");
  return physics_call(h, "fv3lm_convection_create", [&](Physics& p_) { return p_.conv_create(nslots, reinterpret_cast<const RasParams*>(p), do_phy_mst); });
}
int fv3lm_convection_set(fv3lm_handle* h, int slot, const double* ts, const double* frland, const double* kcbl) {
  return physics_call(h, "fv3lm_convection_set", [&](Physics& p_) { return p_.conv_set(slot, ts, frland, kcbl); });
}
int fv3lm_convection_get(fv3lm_handle* h, int slot, double* const* out6, int* doconvec, double* jac2) {
  return physics_call(h, "fv3lm_convection_get", [&](Physics& p_) { return p_.conv_get(slot, out6, doconvec, jac2); });
}
int fv3lm_convection_sources(fv3lm_handle* h, int put, double* const* src4) {
  return physics_call(h, "fv3lm_convection_sources", [&](Physics& p_) { return p_.conv_sources(put, src4); });
}
int fv3lm_convection_table(fv3lm_handle* h, double* table, double* constants) {
  return physics_call(h, "fv3lm_convection_table", [&](Physics& p_) { return p_.conv_table(table, constants); });
}
int fv3lm_convection(fv3lm_handle* h, int slot, int mode) {
  return physics_call(h, "fv3lm_convection", [&](Physics& p_) { return p_.conv_run(slot, mode); });
}
// linearised cloud scheme (cloud.h)
void fv3lm_cloud_default_params(fv3lm_cloud_params* p, int im) {      // fv3jedi_lm_moist_mod.F90:151-211
  if (!p) return;
  const double r[57] = {10.0, 4.0, 4.0, 1.0, 2.0e-3, 8.0e-4, 2.0, 1.0, -1.0, 0.0, 1.3, 1.0e-9, 3.3e-4, 20., 4.8, 4.8, 230., 1.0, 1.0, 230., 14400., 50., 0.01, 0.1, 200., 0., 0., 0.5,
                        0.5, 2000., 0.8, 0.5, -40.0, 1.0, 4.0, 0.0, 0.0, 0.0, 1.0e-3, 8.0e-4, 1.0, 0.80, 1.0, 0.0, 750.0, 0.81, 1.0, 1.0, 0.0, 0.0, 10.e-6, 20.e-6, 21.e-6, 40.e-6,
                        30.e-6, 1.0, 1.0};
  for (int n = 0; n < 57; ++n) p->r[n] = r[n];
  const long imsize = 4L * im;
  p->r[41] = imsize <= 200 ? 0.80 : imsize <= 400 ? 0.90 : imsize <= 800 ? 0.93 : imsize <= 1600 ? 0.95 : 0.97;
  p->r[45] = p->r[41] + 0.01;
}
int fv3lm_cloud_create(fv3lm_handle* h, const fv3lm_cloud_params* p, int iqi, int iql) {
  static_assert(sizeof(fv3lm_cloud_params) == sizeof(CldParams), "fv3lm_cloud_params and CldParams must agree");
  return physics_call(h, "fv3lm_cloud_create", [&](Physics& p_) { return p_.cloud_create(reinterpret_cast<const CldParams*>(p), iqi, iql); });
}
int fv3lm_cloud_bind_cfcn(fv3lm_handle* h, int iqc) {
  return physics_call(h, "fv3lm_cloud_bind_cfcn", [&](Physics& p_) { return p_.cloud_bind_cfcn(iqc); });
}
int fv3lm_cloud_set(fv3lm_handle* h, int slot, const double* qls, const double* qcn, const double* cfcn, const double* khl, const double* khu) {
  return physics_call(h, "fv3lm_cloud_set", [&](Physics& p_) { return p_.cloud_set(slot, qls, qcn, cfcn, khl, khu); });
}
int fv3lm_cloud_get(fv3lm_handle* h, int slot, double* const* out8, double* const* frac4, int* pertmod) {
  return physics_call(h, "fv3lm_cloud_get", [&](Physics& p_) { return p_.cloud_get(slot, out8, frac4, pertmod); });
}
int fv3lm_cloud_cfcn(fv3lm_handle* h, int put, double* cfcn) {
  return physics_call(h, "fv3lm_cloud_cfcn", [&](Physics& p_) { return p_.cloud_cfcn(put, cfcn); });
}
int fv3lm_cloud(fv3lm_handle* h, int slot, int mode) {
  return physics_call(h, "fv3lm_cloud", [&](Physics& p_) { return p_.cloud_run(slot, mode); });
}
// the composed model step (model.h): fv3jedi_lm_mod's step_tl / step_ad over stored trajectory times
extern "C++" {
template <class Fn> static int model_call(fv3lm_handle* h, const char* name, const Fn& fn) {
  if (!h) return fail(std::string(name) + ": null handle");
  if (!fn(h->m)) return fail(h->d.err);
  return status(h);
}
}
int fv3lm_lm_create(fv3lm_handle* h, int nslots, int do_dyn, int do_phy_trb, int do_phy_mst) {
  return model_call(h, "fv3lm_lm_create", [&](Model& m_) { return m_.create(nslots, do_dyn, do_phy_trb, do_phy_mst); });
}
int fv3lm_lm_traj_save(fv3lm_handle* h, int slot) { return model_call(h, "fv3lm_lm_traj_save", [&](Model& m_) { return m_.traj_save(slot); }); }
int fv3lm_lm_traj_load(fv3lm_handle* h, int slot) { return model_call(h, "fv3lm_lm_traj_load", [&](Model& m_) { return m_.traj_load(slot); }); }
int fv3lm_lm_step(fv3lm_handle* h, int slot, int mode) { return model_call(h, "fv3lm_lm_step", [&](Model& m_) { return m_.step(slot, mode); }); }
int fv3lm_step_tl(fv3lm_handle* h) { h->d.step_tl(); return status(h); }
int fv3lm_step_nl(fv3lm_handle* h) { h->d.step_nl(); return status(h); }
int fv3lm_step_ad(fv3lm_handle* h) { h->d.step_ad(); return status(h); }
int fv3lm_traj_to_fv3(fv3lm_handle* h, const double* u, const double* v, const double* t, const double* delp, const double* const* q,
                      const double* w, const double* delz, const double* phis) {
  if (!h->d.traj_to_fv3(u, v, t, delp, q, w, delz, phis)) return fail(h->d.err);
  return status(h);
}
int fv3lm_pert_to_fv3(fv3lm_handle* h, const double* u, const double* v, const double* t, const double* delp, const double* const* q,
                      const double* w, const double* delz) {
  if (!h->d.pert_to_fv3(u, v, t, delp, q, w, delz)) return fail(h->d.err);
  return status(h);
}
int fv3lm_fv3_to_pert(fv3lm_handle* h, double* u, double* v, double* t, double* delp, double* const* q, double* w, double* delz) {
  if (!h->d.fv3_to_pert(u, v, t, delp, q, w, delz)) return fail(h->d.err);
  return status(h);
}
int fv3lm_zero_work_adjoint(fv3lm_handle* h) { h->d.zero_work_adjoint(); return 0; }
int fv3lm_sync(fv3lm_handle* h) { dev_sync(h->d.ex); return status(h); }
long fv3lm_launch_count(fv3lm_handle* h) { return h->d.ex.launches; }
long fv3lm_tp2_launch_count(fv3lm_handle* h) { return h->d.ex.tp2_launches; }
int fv3lm_level_params(fv3lm_handle* h, int k, int* ip, double* rp) {
  if (k < 1 || k > h->d.g.npz) return fail("level out of range");
  const LevelParams& l = h->d.lev_host[k - 1];
  ip[0] = l.hord_mt; ip[1] = l.hord_vt; ip[2] = l.hord_tm; ip[3] = l.hord_dp; ip[4] = l.hord_tr;
  ip[5] = l.nord; ip[6] = l.nord_v; ip[7] = l.nord_w; ip[8] = l.nord_t; ip[9] = l.nord_v_pert;
  rp[0] = l.d2_divg; rp[1] = l.damp_vt; rp[2] = l.damp_w; rp[3] = l.damp_t; rp[4] = l.d_con; rp[5] = l.damp_vt_pert;
  return 0;
}
// Device selection for one-process-per-GPU launches (call before fv3lm_create).
int fv3lm_set_device(int dev) {
#ifndef FV3LM_HOST_EMUL
  if (hipSetDevice(dev) != hipSuccess) return fail("hipSetDevice failed");
#endif
  (void)dev; return 0;
}
// Device-side snapshot / restore of the prognostic state (trajectory and perturbation of u v pt delp q*).
int fv3lm_state_save(fv3lm_handle* h) {
  Dynamics& d = h->d; CkSet& s = d.state_set;
  if (s.items.empty()) {
    for (const Fld& x : d.prognostic()) { s.add("traj", x.t, d.n3); s.add("pert", x.p, d.n3); }
    s.alloc("prognostic state", 1);
  }
  s.save(d.ex, 0);
  return 0;
}
int fv3lm_state_restore(fv3lm_handle* h) {
  Dynamics& d = h->d;
  if (!d.state_set.buf) return fail("fv3lm_state_restore: no snapshot");
  d.state_set.restore(d.ex, 0);
  return 0;
}
// Per-kernel HIP-event profile of everything launched between begin and end (bench.py roofline leg).
// end() writes lines "name count total_ms total_algorithmic_bytes" into buf and returns the length needed.
int fv3lm_profile_begin(fv3lm_handle* h) { h->d.ex.recs.clear(); h->d.ex.profiling = true; return 0; }
int fv3lm_profile_end(fv3lm_handle* h, char* buf, int buflen) {
  Exec& ex = h->d.ex; ex.profiling = false; dev_sync(ex);
  std::map<std::string, std::array<double, 3>> agg;
  for (ProfRec& r : ex.recs) {
    float ms = 0.f;
#ifndef FV3LM_HOST_EMUL
    (void)hipEventElapsedTime(&ms, r.e0, r.e1); (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1);
#endif
    auto& a = agg[r.name]; a[0] += 1.; a[1] += ms; a[2] += r.bytes;
  }
  ex.recs.clear();
  std::string out;
  for (auto& kv : agg) { char line[256]; std::snprintf(line, sizeof line, "%s %.0f %.6f %.0f\n", kv.first.c_str(), kv.second[0], kv.second[1], kv.second[2]); out += line; }
  if (buf && buflen > 0) { std::strncpy(buf, out.c_str(), buflen - 1); buf[buflen - 1] = 0; }
  return (int)out.size() + 1;
}
#ifdef FV3LM_HOST_EMUL
int fv3lm_emul_check_boxes(fv3lm_handle* h, int on) { h->d.ex.check_boxes = on != 0; return 0; }
#endif

}  // extern "C"
