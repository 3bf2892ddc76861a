// fv3lm-hip: the host side of the composed model step -- fv3jedi_lm_mod's step_tl / step_ad (src/fv3jedi_lm_mod.F90:161-187): the dynamics
// and the column physics of one time step in the reference's order, about the trajectory of one stored time -- behind fv3lm_lm_*.
// A Model serves one Dynamics and its Physics: it owns the trajectory slots and nothing of theirs, runs their entry points and reports
// through the handle's one error string.  No kernel of its own: the slots are records of a CkSet (dycore.h), saved and restored by its
// device-to-device copies.
#pragma once
#include "physics.h"

namespace fv3 {

// what a sweep of the dynamics may have run into, as the status of a C-ABI call reports it; empty: nothing
inline std::string pending_failure(Dynamics& d) {
  if (!sticky_error().empty()) return sticky_error();
  if (!d.err.empty() && d.halo_missing) return d.err;
  if (d.halo_missing) return "halo exchange needed before fv3lm_set_exchange provided its table (face mode)";
  if (d.tracer_subcycle_error) return "tracer_2d: accumulated Courant number > 60: trajectory is not usable";
  if (d.nh_overflow()) return "non-hydrostatic column solver: reverse-mode tape overflow (internal sizing error)";
  return std::string();
}

struct Model {
  Dynamics& d; Physics& p; Exec& ex;
  Model(Dynamics& d_, Physics& p_) : d(d_), p(p_), ex(d_.ex) {}
  // nothing allocated until fv3lm_lm_create.  A record of the set is one trajectory time: what fv3lm_traj_to_fv3 leaves resident of the
  // trajectory -- u v pt delp q* (w delz), whole padded planes with their halos and D-grid edge rows, and phis with its halo
  struct Store {
    DevList mem; CkSet set; int nslots = 0; std::vector<char> saved;
    int do_dyn = 0, do_phy_trb = 0, do_phy_mst = 0;      // conf%do_dyn, do_phy_trb, do_phy_mst (/= 0)
  } s;
  void release() { Physics::drop(s); }
  bool created() const { return !s.mem.empty(); }

  // fv3lm_lm_create: every slot in one block, all or nothing
  bool create(int nslots, int do_dyn, int do_phy_trb, int do_phy_mst) {
    const char* who = "fv3lm_lm_create";
    if (created()) return p.no(who, "already created for this handle");
    if (nslots < 1) return p.no(who, "nslots < 1");
    const int flag[3] = {do_dyn, do_phy_trb, do_phy_mst}; const char* name[3] = {"do_dyn", "do_phy_trb", "do_phy_mst"};
    for (int n = 0; n < 3; ++n) if (flag[n] < 0 || flag[n] > 1) return p.no(who, std::string(name[n]) + " = " + std::to_string(flag[n]) + " outside 0..1");
    if (!do_dyn && !do_phy_trb && !do_phy_mst) return p.no(who, "do_dyn = do_phy_trb = do_phy_mst = 0: a step of nothing");
    for (const Fld& x : d.prognostic()) s.set.add("traj", x, d.pl_all());
    s.set.add("phis", d.hs_dev, d.pl_all());
    const size_t b_slot = s.set.stride * 8;
    const bool fits = (size_t)nslots <= ((size_t)1 << 62) / b_slot;
    const size_t total = fits ? (size_t)nslots * b_slot : ~(size_t)0;
    if (std::getenv("FV3LM_VERBOSE")) std::fprintf(stderr, "fv3lm: trajectory store %d slot(s) x %zu bytes\n", nslots, b_slot);
    const bool clean = sticky_error().empty();
    if (fits) s.set.buf = s.mem.get<double>(total); else s.mem.refuse();
    if (!p.allocated(who, s, total, clean)) {
      d.err += " (" + std::to_string(nslots) + " trajectory slot(s) of " + std::to_string(b_slot) + " bytes; fv3lm_create has taken the acoustic-step slots from free memory: cap them with FV3LM_TRAJ_SLOTS)";
      return false;
    }
    s.set.name = "model trajectory"; s.set.nrec = nslots;
    s.saved.assign((size_t)nslots, 0); s.nslots = nslots;
    s.do_dyn = do_dyn; s.do_phy_trb = do_phy_trb; s.do_phy_mst = do_phy_mst;
    return true;
  }
  bool slot_ok(const char* who, int slot) { return p.slot_ok(who, "lm", created(), s.nslots, slot); }
  bool slot_saved(const char* who, int slot) { return p.slot_set(who, "trajectory slot", s.saved, slot, "fv3lm_lm_traj_save"); }
  // resident trajectory -> slot
  bool traj_save(int slot) {
    const char* who = "fv3lm_lm_traj_save";
    if (!slot_ok(who, slot)) return false;
    s.saved[(size_t)slot] = 0;
    s.set.save(ex, slot);
    if (!p.sticky_clean()) return false;
    s.saved[(size_t)slot] = 1;
    return true;
  }
  // slot -> resident trajectory, as fv3lm_traj_to_fv3 of the same host arrays leaves it: the planes come back whole, so the halos, the
  // edge rows and the halo of phis need no exchange; pe peln pk pkz are computed again from the restored delp by the kernel the upload
  // runs (traj_to_fv3, fv3jedi_lm_dynamics_mod.F90:803-805), which gives its bits
  void load(int slot) { s.set.restore(ex, slot); d.pressures(MODE_NL); }
  bool traj_load(int slot) {
    const char* who = "fv3lm_lm_traj_load";
    if (!slot_ok(who, slot) || !slot_saved(who, slot)) return false;
    load(slot);
    return p.sticky_clean();
  }

  // ipert_to_zero (fv3jedi_lm_mod.F90:242-253): of ua, va, cfcn only cfcn lives on the device, with the cloud feature.  Bound to a tracer
  // (fv3lm_cloud_bind_cfcn) it is that tracer's perturbation, cleared on its whole padded planes: the adjoint's halo enters step_ad as
  // zeros, as pert_to_fv3 leaves it (fv3jedi_lm_dynamics_mod.F90:878).  Nothing clears it between the dynamics and the moist half, so the
  // tangent the transport leaves in it reaches CLOUD_DRIVER_D (fv3jedi_lm_moist_mod.F90:438) and the adjoint CLOUD_DRIVER_B leaves in it
  // (:616) reaches FV_DYNAMICS_BWD
  void clear_cfcn() {
    if (p.cld.mem.empty()) return;
    if (p.cld.iqc) dev_zero(ex, d.q[(size_t)p.cld.iqc - 1].p, d.n3 * 8);
    else dev_zero(ex, p.cld.cfcn, p.ncol() * d.g.npz * 8);
  }
  bool dynamics_ok() { const std::string e = pending_failure(d); if (e.empty()) return true; d.err = e; return false; }

  // fv3lm_lm_step: step_tl (fv3jedi_lm_mod.F90:161-172) or step_ad (:176-187) on the resident perturbation.  The physics halves in the
  // order of fv3jedi_lm_physics_mod.F90:121-122 (tangent: moist, then turbulence) and :137-138 (adjoint: turbulence, then moist); every
  // physics run takes its trajectory from its slot, so the dynamics may advance the resident one before them.  Every refusal stands
  // before anything is run or cleared; a part that fails ends the step with its own message.
  bool step(int slot, int mode) {
    const char* who = "fv3lm_lm_step";
    if (!created()) return p.no(who, "call fv3lm_lm_create first");
    if (mode != MODE_TL && mode != MODE_AD)
      return p.no(who, "mode " + std::to_string(mode) + ": 1 (tangent) or 2 (adjoint); the nonlinear step is composed from the parts, because its physics must be set "
                       "from the trajectory the dynamics has just advanced");
    if (!slot_ok(who, slot)) return false;
    if (s.do_dyn && !slot_saved(who, slot)) return false;
    if (s.do_phy_trb && (!p.turb_slot_ok(who, slot) || !p.slot_set(who, "turbulence slot", p.turb.set, slot, "fv3lm_turbulence_set_diagonals / _set_simple"))) return false;
    if (s.do_phy_mst) {
      if (!p.conv_slot_ok(who, slot)) return false;
      if (p.cld.mem.empty()) return p.no(who, "do_phy_mst with the convection created but the cloud scheme not: the reference has no such half (call fv3lm_cloud_create)");
      if (!p.cloud_slot_ok(who, slot, true)) return false;
    }
    if (!dynamics_ok()) return false;
    const bool tl = mode == MODE_TL;
    auto dynamics = [&]() {
      load(slot);
      if (tl) { d.step_tl(); return dynamics_ok(); }
      d.step_nl();                                       // FV_DYNAMICS_FWD: the forward sweep that stores the checkpoints
      if (!dynamics_ok()) return false;
      d.step_ad();
      return dynamics_ok();
    };
    auto moist = [&]() { return tl ? p.conv_run(slot, mode) && p.cloud_run(slot, mode) : p.cloud_run(slot, mode) && p.conv_run(slot, mode); };
    auto turbulence = [&]() { return p.turb_run(slot, mode); };
    clear_cfcn();
    if (tl) {
      if (s.do_dyn && !dynamics()) return false;
      if (s.do_phy_mst && !moist()) return false;
      if (s.do_phy_trb && !turbulence()) return false;
    } else {
      if (s.do_phy_trb && !turbulence()) return false;
      if (s.do_phy_mst && !moist()) return false;
      if (s.do_dyn && !dynamics()) return false;
    }
    clear_cfcn();
    return true;
  }
};

}  // namespace fv3
