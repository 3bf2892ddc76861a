/* fv3lm.h — C-ABI of the MI355X-native FV3 tangent-linear / adjoint dynamical core.
 *
 * Drop-in boundary: the body of fv3jedi_lm_dynamics_type%step_tl / %step_ad between the
 * traj/pert -> FV_Atm copies and the copy back (reference src/dynamics/fv3jedi_lm_dynamics_mod.F90:
 * step_tl :347-456 calls FV_DYNAMICS_TLM at :421-438; step_ad :460-689 calls FV_DYNAMICS_FWD :507 and
 * FV_DYNAMICS_BWD :615).  A Fortran host binds these entry points with ISO_C_BINDING
 * (fortran/fv3lm_hip_mod.F90).
 *
 * Conventions: every pointer is a host pointer to fp64 data unless a function says "device".
 * All functions return 0 on success, nonzero on failure; fv3lm_last_error() gives the message
 * (the reference has no status returns — it calls mpp_error(FATAL)/exit(1),
 * src/fv3jedi_lm_mod.F90:93 — the Fortran shim turns a nonzero status into that).
 *
 * Field layout ("padded plane"): a 3-D field is [ntile][nk][pj][pi] doubles, i fastest,
 *   pi = nx + 2*ng + 1, pj = ny + 2*ng + 1, ng = 3 (TOOLS/fv_mp_nlm_mod.F90:67);
 *   Fortran element (i,j,k), i in isd..ied+1, j in jsd..jed+1 (isd = 1-ng), sits at
 *   ((k-1)*pj + (j-jsd))*pi + (i-isd).  This one index map holds the A-, C-, D- and corner-
 *   staggered arrays of the reference (u(isd:ied,jsd:jed+1), v(isd:ied+1,jsd:jed), ...).
 */
#ifndef FV3LM_H
#define FV3LM_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fv3lm_handle fv3lm_handle;

/* fv_flags_type subset (NLM/fv_arrays_nlm.F90:236-506) and fv_flags_pert_type
 * (TLM/fv_arrays_tlmadm.F90:37-92).  The trajectory-side values are those in force after
 * run_setup_pert (TLM/fv_control_tlmadm.F90:219-252).  Two sets of physical constants are mixed on
 * the path: the JEDI set (utils/fv3jedi_lm_const_mod.F90:17-41, passed at
 * DYN/fv3jedi_lm_dynamics_mod.F90:423-424) and FMS constants_mod — both are runtime inputs. */
typedef struct fv3lm_options {
  int hord_mt, hord_vt, hord_tm, hord_dp, hord_tr;                 /* trajectory advection schemes: 1, 2, 333 (the differentiated ones) or, beside a different
                                                                      perturbation scheme (split_hord), any of the nonlinear routines' 3 .. 13 -- values only */
  int nord, do_vort_damp, n_sponge;
  int hord_mt_pert, hord_vt_pert, hord_tm_pert, hord_dp_pert, hord_tr_pert;      /* perturbation schemes: 1, 2 or 333 (tp_core_tlm.F90:2393-2487) */
  int nord_pert, do_vort_damp_pert, n_sponge_pert, hord_ks_traj, hord_ks_pert;
  int hord_mt_ks_traj, hord_vt_ks_traj, hord_tm_ks_traj, hord_dp_ks_traj, hord_tr_ks_traj;
  int hord_mt_ks_pert, hord_vt_ks_pert, hord_tm_ks_pert, hord_dp_ks_pert, hord_tr_ks_pert;
  int kord_tm, kord_mt, kord_wz, kord_tr;                          /* trajectory remap profiles: |kord| > 16 (linear) or the limited 8 .. 15 of cs_profile / scalar_profile (split_kord) */
  int kord_tm_pert, kord_mt_pert, kord_wz_pert, kord_tr_pert;      /* perturbation remap profiles (fv_flags_pert_type): |kord| > 16, the linear one */
  int hydrostatic;
  int split_damp;   /* fv_flags_pert_type%split_damp (fv_arrays_tlmadm.F90:76; the reference's default is .true.).  1: the perturbation takes its own damping
                       (nord_pert, dddmp_pert, d2_bg_pert, d4_bg_pert, vtdm4_pert ... with the perturbation sponge rules, dyn_core_tlm.F90:835-921), the
                       trajectory values the trajectory's (sw_core_tlm.F90:1664-1682, :1787-1803, :2341-2369); the trajectory's nord may then be 2 or 3
                       (hydrostatic = 0: through fv3lm_set_trajectory_damping_order after create).
                       0: run_setup_pert has copied the perturbation's damping options onto the trajectory (fv_control_tlmadm.F90:220-229): the two sets
                       handed over must then be equal, anything else is refused. */
  double dddmp, d2_bg, d4_bg, vtdm4, d2_bg_k1, d2_bg_k2, d_con, ke_bg;
  double dddmp_pert, d2_bg_pert, d4_bg_pert, vtdm4_pert, d2_bg_k1_pert, d2_bg_k2_pert, d2_bg_ks_pert;
  double akap, cp, zvir, grav_jedi;                          /* JEDI constants */
  double cp_air, rdgas, rvgas, grav, radius, omega, hlv;     /* FMS constants_mod */
  double ptop;
  double a_imp, p_fac, scale_z;                              /* non-hydrostatic solver (hydrostatic = 0): off-centering, pressure floor factor, w damping */
} fv3lm_options;

typedef struct fv3lm_dims {
  int nx, ny, npz;      /* cells per tile edge (npx-1, npy-1), levels */
  int ntile;            /* tiles resident on this GPU */
  int nq;               /* tracers (qv, ql, qi, o3: DYN/fv3jedi_lm_dynamics_mod.F90:158-167) */
  int n_split, k_split; /* acoustic / remap sub-steps (fv_flags_type) */
  int face;             /* 0: one doubly-periodic tile with no cube edge in it (the code path of an MPI rank in the middle of a
                           face: every `is .EQ. 1` / `j .EQ. npy` / sw_corner branch of the reference off); ntile must be 1.
                           1: every resident tile is a whole cube face (is = 1, ie = npx-1; all edge and corner branches on);
                           needs fv3lm_set_face_data and, for anything that exchanges halos, fv3lm_set_exchange. */
  double dt;            /* create(self,dt,...) src/fv3jedi_lm_mod.F90:44 */
  /* Sub-face tiles (fv_flags_type%layout > 1 x 1, NLM/fv_control_nlm.F90:556; rank -> tile map tools/fv_mp_nlm_mod.F90:452-453).  face = 1 only.
     nface: cells per edge of a whole face (npx-1); 0 or nx: every resident tile is a whole face.  tile_ij0: for each resident tile its (is, js)
     in the global indices of its face, 2*ntile ints (NULL: (1, 1) for all).  nx, ny are then the cells of a tile (ie-is+1); all resident
     tiles have the same size.  Exchange tables (fv3lm_set_exchange*) index the padded plane of a TILE. */
  int nface, pad_;
  const int* tile_ij0;
} fv3lm_dims;

/* Number and order of the metric planes handed to fv3lm_create (fv_grid_type,
 * NLM/fv_arrays_nlm.F90:115-234), each [ntile][pj][pi]:
 *  area rarea rarea_c dx dy dxa dya dxc dyc rdx rdy rdxa rdya rdxc rdyc cosa sina rsina cosa_u cosa_v
 *  cosa_s sina_u sina_v rsin_u rsin_v rsin2 f0 fC del6_u del6_v divg_u divg_v sin_sg(1..9) cos_sg(1..9) */
#define FV3LM_NMETRIC 50
const char* fv3lm_metric_names(void);

/* Replaces fv3jedi_lm_dynamics_type%create (DYN/fv3jedi_lm_dynamics_mod.F90:69-264) for the device
 * side: uploads metric terms once, resolves the per-level scheme table, allocates device state. */
int fv3lm_create(fv3lm_handle** h, const fv3lm_dims* dims, const fv3lm_options* opt, const double* const* metrics,
                 double da_min, double da_min_c, const double* phis, const double* ak, const double* bk);
/* Face mode only.  edge: the a2b_ord4 edge weights edge_w, edge_e, edge_s, edge_n of fv_grid_type
 * (NLM/fv_arrays_nlm.F90:150-151) as [ntile][4][pj], entry (j - jsd) / (i - isd) of each; ecorner: the
 * extrap_corner factors x1/(x2-x1) of a2b_ord4's four corners (a2b_edge_tlm.F90:101-139, :1478-1487) as
 * [ntile][4: sw se ne nw][3], in the order the reference evaluates them. */
int fv3lm_set_face_data(fv3lm_handle* h, const double* edge, const double* ecorner);
/* Rayleigh damping of the upper layers (RAYLEIGH_SUPER, fv_dynamics_tlm.F90:1749-1899).  tau: e-folding time in days
 * (flagstruct%tau; 0 switches it off, the default); rf_cutoff: pressure (Pa) above which levels are damped (flagstruct%rf_cutoff);
 * c2l: the cubed-to-lat-lon matrices a11 a12 a21 a22 of fv_grid_type as [ntile][4][pj][pi] (padded plane, like the metrics).
 * Call after fv3lm_create, before the first step; may be called again.  Refused: tau < 0, values that are not finite, and with
 * tau > 0: rf_cutoff <= ptop, c2l == NULL, or a handle created without ak, bk.  Built for conserve = .true., not nested,
 * grid_type < 4 (RAYLEIGH_FRICTION, grid_type >= 4, is not). */
int fv3lm_set_rayleigh(fv3lm_handle* h, double tau, double rf_cutoff, const double* c2l);
/* rf(k) for k = 1..npz (0 below the cutoff) and kmax, as the library computed them (tests, diagnostics). */
int fv3lm_rayleigh_profile(fv3lm_handle* h, double* rf, int* kmax);
/* Tracer damping of tracer_2d: the mass-weighted del-2 (nord 0) or del-4 (nord 1) flux deln_flux adds to every tracer's transport
 * (fv_tracer2d_tlm.F90:1045-1111 tangent, :1390-1417 nonlinear, fv_tracer2d_adm.F90 adjoint; tp_core_tlm.F90:203-206, :1918-2043).
 * nord_tr, trdm2: flagstruct%nord_tr, %trdm2 of the trajectory; nord_tr_pert, trdm2_pert, split_damp_tr: the same of the perturbation
 * (fv_core_pert_nml, fv_arrays_tlmadm.F90:87-90).  As in the reference:
 *   - split_damp_tr = 0: the trajectory's pair is overwritten by the perturbation's (run_setup_pert, fv_control_tlmadm.F90:232-234);
 *   - the damping acts in the first sub-step of a sub-cycled level only, and only where the TRAJECTORY's trdm2 > 1e-4; the
 *     perturbation's coefficient never switches it on;
 *   - hord_tr == hord_tr_pert: one differentiated call with the trajectory's pair -- nord_tr_pert, trdm2_pert are not read, whatever
 *     split_damp_tr says; hord_tr != hord_tr_pert: the tangent / adjoint with the perturbation's pair (no damping where its
 *     trdm2_pert <= 1e-4), the values again with the trajectory's.
 * Call after fv3lm_create, before the first step; may be called again between complete steps.  It rebuilds the tracer program: the
 * damping stages and the mass argument (dp1) exist only while the effective trajectory trdm2 > 1e-4; a handle that never calls it, or
 * whose effective trdm2 <= 1e-4, runs exactly the launches it ran without.  Refused, the handle left as it was: a coefficient that is
 * not finite or negative, split_damp_tr outside 0..1, nord_tr_pert outside 0..1, nord_tr outside 0..2 (nord 3 is not built), an
 * effective nord_tr = 2 with hord_tr == hord_tr_pert (the tangent of a nord-2 deln_flux is not built).  nq = 0: accepted, no effect. */
int fv3lm_set_tracer_damping(fv3lm_handle* h, int nord_tr, double trdm2, int nord_tr_pert, double trdm2_pert, int split_damp_tr);
/* The effective pairs after the first rule above: nord2 = {nord_tr, nord_tr_pert}, trdm2 = {trdm2, trdm2_pert} (tests, diagnostics). */
int fv3lm_tracer_damping(fv3lm_handle* h, int* nord2, double* trdm2);
/* External-mode divergence damping of the acoustic step (dyn_core_nlm.F90:641-644, :678-684, :707-727; dyn_core_tlm.F90:937-943,
 * :999-1007, :1031-1060; consumed by one_grad_p, dyn_core_nlm.F90:1713-1741, :1762-1775).  d_ext: flagstruct%d_ext (the reference's
 * default is 0.02; 0 switches it off, the default HERE -- a host passes its flagstruct%d_ext).  Per acoustic step: the step's input delp at
 * the cell corners (a2b_ord2), the corner divergence d_sw sees before any damping (with split_damp its value from the trajectory's
 * nord, its tangent / adjoint from nord_pert, level by level), their delp-weighted column mean divg2 = d_ext da_min_c sum(wk vt) / sum(wk),
 * and its differences inside the brackets of one_grad_p's wind update -- nonlinear, tangent and adjoint.
 * Call after fv3lm_create, before the first step; may be called again between complete steps.  Going from 0 to > 0 or back rebuilds the
 * acoustic program and with it the plan of the trajectory slots of the backward sweep; a handle that never calls it, or calls it with
 * 0, runs exactly the launches it ran without.  Refused, the handle left as it was: d_ext < 0, a value that is not finite.
 * Non-hydrostatic handle: accepted and remembered, no launch added -- with beta = 0 the pressure gradient is nh_p_grad, which never reads
 * divg2 (dyn_core_nlm.F90:871-880), so d_ext changes no output there.
 * While it is on, fv3lm_field_get knows "divg2" (one level; corners is..ie+1, js..je+1 of the last acoustic step; value and tangent after
 * a tangent-linear sweep). */
int fv3lm_set_external_damping(fv3lm_handle* h, double d_ext);
/* d_ext as set (0 on a handle that never called the setter). */
int fv3lm_external_damping(fv3lm_handle* h, double* d_ext);
/* The trajectory's divergence-damping order (flagstruct%nord) after create.  It sets the trajectory's nord, resolves every level's
 * damping orders and coefficients again (dyn_core_tlm.F90:741-921) and, when the order changed, rebuilds the acoustic program as
 * fv3lm_set_external_damping does: the work arena and the plan of the trajectory slots of the backward sweep are made anew, so a
 * forward sweep stored before the call does not serve an adjoint after it -- call it before the first step or between complete
 * steps (nonlinear sweep + adjoint).  A call with the order the handle already has rebuilds nothing.
 * Hydrostatic handle: the result is the handle fv3lm_create builds with that nord.
 * Non-hydrostatic handle: the only way to orders 2 and 3 (fv3lm_create refuses them).  w in d_sw and the interface heights in
 * update_dz_d are then damped by the differentiated del6_vt_flux of order min(2, nord) -- three Laplacians, tangent and adjoint
 * (sw_core_tlm.F90:1712-1745, nh_utils_tlm.F90:489-520) -- on the levels outside the sponge, as three stage launches per field and
 * mode (FV3LM_DEL6_FUSED=1 in the environment at that time: one LDS-tiled launch).  A host creates with
 * nord = min(flagstruct%nord, nord_pert) and then passes flagstruct%nord here.
 * Refused, the handle left as it was: nord outside 0..3; split_damp = 0 with nord != nord_pert; nord = 0 with nord_pert > 0.
 * A rebuild that fails (device memory) puts the order and the level table back, but leaves the handle's error set: the getter
 * reports the former order and every later call on the handle fails. */
int fv3lm_set_trajectory_damping_order(fv3lm_handle* h, int nord);
/* nord as in force (the value given to fv3lm_create on a handle that never called the setter). */
int fv3lm_trajectory_damping_order(fv3lm_handle* h, int* nord);
/* Halo exchange between the resident faces: replaces the FMS calls mpp_update_domains / mpp_get_boundary that the
 * reference issues from DYN_CORE_TLM (dyn_core_tlm.F90:1744-1790, :1960-1990, :2280-2300, :2418-2434) and
 * FV_DYNAMICS_TLM (fv_dynamics_tlm.F90:646-651, :708-712).  One table per kind of exchange:
 *   0 cell-centred scalar (delp, pt, q)        1 D-grid wind pair (u, v)        2 C-grid wind pair (uc, vc)
 *   3 corner scalar (divg_d)                   4 shared edge rows of (u, v): u(:,npy), v(npx,:)  (mpp_get_boundary)
 * rows[nrows][7] = dst_field(0|1), dst_tile, dst_index, src_field(0|1), src_tile, src_index, sign(+1|-1): plane
 * element dst_index of the halo takes sign * element src_index of the neighbour face (indices into the padded
 * plane, tiles 0-based among the resident ones; field 0/1 = first/second component of a pair). */
int fv3lm_set_exchange(fv3lm_handle* h, int kind, const int* rows, int nrows);
int fv3lm_halo(fv3lm_handle* h, int kind, const char* field0, const char* field1, int mode);   /* one exchange (tests) */
/* Faces held by other ranks (one process per GPU).  The rows of a table whose source face lives on another rank become, per
 * peer, a send list (send_rows[.][3] = field, local tile, index of the source element) and a receive list (recv_rows[.][4] =
 * field, local tile, index of the halo element, sign), concatenated over the peers in peers[] order; both ends must list the
 * rows in the order of the global table (cube.split_table).  nsend[p] / nrecv[p] = rows for peer p. */
int fv3lm_set_exchange_remote(fv3lm_handle* h, int kind, int npeers, const int* peers, const int* nsend, const int* send_rows,
                              const int* nrecv, const int* recv_rows);
/* Transport between ranks: RCCL point-to-point (ncclSend / ncclRecv, grouped per exchange) on the library's own stream.
 * rccl_path: the RCCL shared library the process already uses (e.g. the one bundled with torch), opened with dlopen so that a
 * process never runs two RCCL runtimes; id128: 128-byte ncclUniqueId made by fv3lm_comm_unique_id on rank 0 and distributed by
 * the host (mpp_broadcast / MPI_Bcast / torch.distributed); every rank that holds faces then calls fv3lm_comm_init. */
int fv3lm_comm_unique_id(const char* rccl_path, void* id128);
int fv3lm_comm_init(const char* rccl_path, const void* id128, int nranks, int rank);
int fv3lm_comm_destroy(void);
/* Host hooks.  Transport callback: replaces RCCL (the test-only host-emulation build has no other transport): called once per
 * exchange with one send and one receive buffer per peer, counts in doubles.  All-reduce callback: in-place element-wise max
 * over the ranks that hold faces, for tracer_2d's per-level Courant maxima (mp_reduce_max, fv_tracer2d_tlm.F90:1306). */
typedef void (*fv3lm_transport_fn)(void* user, int npeers, const int* peer_ranks, double* const* sendbufs, const long* send_counts,
                                   double* const* recvbufs, const long* recv_counts);
typedef void (*fv3lm_allreduce_fn)(void* user, double* buf, int n);
int fv3lm_set_transport_callback(fv3lm_transport_fn fn, void* user);
int fv3lm_set_allreduce_callback(fv3lm_allreduce_fn fn, void* user);
int fv3lm_destroy(fv3lm_handle* h);     /* %delete, DYN/fv3jedi_lm_dynamics_mod.F90:693-713 */
const char* fv3lm_last_error(void);

/* Device-resident named fields (padded-plane layout).  which: 0 = trajectory, 1 = perturbation /
 * adjoint.  State fields: u v delp pt (+ q1.. for tracers), diagnostics pe peln pk pkz,
 * accumulators mfx mfy cx cy; every work array of the step is also addressable (tests). */
int fv3lm_field_put(fv3lm_handle* h, const char* name, int which, const double* host);
int fv3lm_field_get(fv3lm_handle* h, const char* name, int which, double* host);
int fv3lm_field_levels(fv3lm_handle* h, const char* name);

/* Execution.  mode: 0 nonlinear, 1 tangent linear, 2 adjoint. */
int fv3lm_run_group(fv3lm_handle* h, const char* group, int mode);  /* one kernel group of the acoustic step:
     "c_sw" (C_SW_TLM sw_core_tlm.F90:87), "geopk_c"/"geopk_d" (GEOPK_TLM dyn_core_tlm.F90:4578),
     "p_grad_c" (:3194), "d_sw" (D_SW_TLM sw_core_tlm.F90:1047), "one_grad_p" (:3867), "halo_*" */
int fv3lm_dyn_core(fv3lm_handle* h, int mode);   /* DYN_CORE_TLM dyn_core_tlm.F90:93 / DYN_CORE_FWD+BWD dyn_core_adm.F90:115,1686 */
/* The operator itself.  State fields u v pt(=temperature) delp q1..qn — and w, delz when hydrostatic = 0 (nh_core_tlm.F90 /
 * nh_utils_tlm.F90 path: RIEM_SOLVER_C, RIEM_SOLVER3 with a_imp in (0.5, 0.999], UPDATE_DZ_C/D) — are device-resident (fv3lm_field_put /
 * _get; compute domain is..ie x js..je, D-grid winds incl. the far edge row/column).
 *  fv3lm_step_tl : replaces compute_fv3_pressures_tlm + FV_DYNAMICS_TLM in %step_tl
 *                  (DYN/fv3jedi_lm_dynamics_mod.F90:404-438).  In: trajectory (which=0) and perturbation
 *                  (which=1) at t; out: both advanced to t+dt.
 *  fv3lm_step_nl : nonlinear sweep that also stores the stage checkpoints (FV_DYNAMICS_FWD role, :507).
 *  fv3lm_step_ad : FV_DYNAMICS_BWD + compute_fv3_pressures_bwd (:615-638); call after fv3lm_step_nl on the
 *                  same trajectory.  In: adjoint of the state at t+dt (which=1); out: adjoint at t.  The forward
 *                  sweep's checkpoints stay valid: further fv3lm_step_ad calls on the same trajectory need no new
 *                  fv3lm_step_nl (the role of cp_iter, utils/tapenade/tapenade_iter.F90). */
int fv3lm_step_tl(fv3lm_handle* h);
int fv3lm_step_nl(fv3lm_handle* h);
int fv3lm_step_ad(fv3lm_handle* h);
/* The host's boundary copies on the device -- traj_to_fv3, pert_to_fv3, fv3_to_pert (DYN/fv3jedi_lm_dynamics_mod.F90:717-807, :846-889,
 * :893-933).  Arrays are the host's own traj% / pert% fields: COMPACT, (isc:iec, jsc:jec, npz) per resident tile in Fortran order
 * (i fastest, tile slowest), no halo; q[n] one array per tracer (qv ql qi o3 ...), w / delz only when hydrostatic = 0, phis
 * (isc:iec, jsc:jec) or NULL to keep the one given at create.
 *   fv3lm_traj_to_fv3: halos zeroed, interiors copied, the D-grid edge rows u(:, jec+1) / v(iec+1, :) filled from the neighbour faces
 *                      (mpp_get_boundary :781-793), halo of phis updated (:798), pe / peln / pk / pkz computed (:803-805).
 *   fv3lm_pert_to_fv3: perturbation (step_tl) or adjoint forcing (step_ad) in, halos zeroed.
 *   fv3lm_fv3_to_pert: compute-domain perturbation / adjoint out; the device copy is cleared as the reference clears FV_AtmP. */
int fv3lm_traj_to_fv3(fv3lm_handle* h, const double* u, const double* v, const double* t, const double* delp, const double* const* q,
                      const double* w, const double* delz, const double* phis);
int fv3lm_pert_to_fv3(fv3lm_handle* h, const double* u, const double* v, const double* t, const double* delp, const double* const* q,
                      const double* w, const double* delz);
int fv3lm_fv3_to_pert(fv3lm_handle* h, double* u, double* v, double* t, double* delp, double* const* q, double* w, double* delz);
/* Sub-operators, same mode argument (tests and kernel-level benchmarks): */
int fv3lm_pressures(fv3lm_handle* h, int mode);                 /* compute_fv3_pressures{,_tlm,_bwd} TLM/fv_pressure.F90 */
int fv3lm_tracer_2d(fv3lm_handle* h, int mode);                 /* TRACER_2D_TLM fv_tracer2d_tlm.F90:757 / _FWD+_BWD */
int fv3lm_traj_slots(fv3lm_handle* h);                          /* acoustic steps (of n_split*k_split) whose intermediates the forward sweep keeps
                                                                   in HBM so that the backward sweep need not recompute them; chosen at create from free memory,
                                                                   FV3LM_TRAJ_SLOTS caps it */
int fv3lm_tracer_nsplt(fv3lm_handle* h);                        /* largest tracer sub-step count (nsplt, fv_tracer2d_tlm.F90:1317) used so far */
int fv3lm_remap(fv3lm_handle* h, int mode, int last_step);      /* LAGRANGIAN_TO_EULERIAN_TLM fv_mapz_tlm.F90:69 / _FWD+_BWD, remap_option 0.
                                                                   Hydrostatic: T_v in log p, tracers, u, v; new pe, peln, pk, pkz, delp.
                                                                   Non-hydrostatic handle: the non-hydrostatic remap of fv_dynamics (density
                                                                   temperature through delz, w with the surface value ws, delz as -delz/delp);
                                                                   last_step as passed */
int fv3lm_fv_dynamics(fv3lm_handle* h, int mode);               /* FV_DYNAMICS_TLM fv_dynamics_tlm.F90:87 / _FWD+_BWD */
int fv3lm_rayleigh(fv3lm_handle* h, int mode);                  /* RAYLEIGH_SUPER_TLM fv_dynamics_tlm.F90:1749 / _FWD+_BWD fv_dynamics_adm.F90:2327-2652
                                                                   on u v pt (w); non-hydrostatic: the heated temperature goes to field "rf_pt",
                                                                   pt keeps the one pt_in takes pkz from.  Adjoint: after a MODE_NL call */
/* Linearised boundary-layer turbulence (physics/turbulence/fv3jedi_lm_turbulence_mod.F90, do_phy_trb): a vertical diffusion of the
 * perturbation with coefficients frozen on the trajectory, seven tridiagonal solves per column -- u, v on the V system, T (as potential
 * temperature p00^kappa T / pk) on S, q1 on Q with ygswitch = 1 and q2 .. q_nq on Q with ygswitch = 0 (step_tl :258-269).  Column-local:
 * only is..ie x js..je of every resident tile is read or written; the far edge rows u(:, je+1), v(ie+1, :), every halo, delp, w and
 * delz are not touched.  Arrays are COMPACT, (isc:iec, jsc:jec, npz) per resident tile, tile slowest, like those of fv3lm_traj_to_fv3.
 *   fv3lm_turbulence_create: nslots = one per trajectory time the host keeps (saveltraj ? conf%nt : 1; ltraj(conf%n) :66-74).
 *       Allocates nslots x 10 x ntile x npz x pj x pi x 8 bytes on the device (FV3LM_VERBOSE=1 prints it); freed by fv3lm_destroy.
 *       Refused: a second create on the handle, nslots < 1, npz < 2, an allocation that fails.
 *   fv3lm_turbulence_set_diagonals: diag[9] = AKV BKV CKV AKS BKS CKS AKQ BKQ CKQ (lower, main, upper) as BL_DRIVER returns them,
 *       BEFORE VTRILUPERT (:510-512): the device factorises (b(1) = 1/b(1); a(l) = a(l) b(l-1), b(l) = 1/(b(l) - c(l-1) a(l))).
 *       Refused with the slot left unset: a pivot that is zero or a factor that is not finite.
 *   fv3lm_turbulence_set_simple: the diagonals from BL_simp (turbulence/blsimp.F90) evaluated on the device from the resident
 *       trajectory (u, v at (i, j), PTT = T / pk, PKT = pk, qv ql qi = q1 q2 q3, JEDI constants of the options) and frocean
 *       (isc:iec, jsc:jec) per tile; needs nq >= 3.
 *   Both take pk (compute_pressures, utils/fv3jedi_lm_utils_mod.F90:359-391) from the RESIDENT TRAJECTORY delp AT THE CALL, and a slot
 *   keeps what its set call saw.  The reference's turbulence uses the trajectory at the start of the step, and fv3lm_step_tl /
 *   fv3lm_step_nl advance the resident trajectory: call set_* after fv3lm_traj_to_fv3 and BEFORE fv3lm_step_tl / fv3lm_step_nl.
 *   fv3lm_turbulence: mode 0 the solves on the trajectory (step_nl :151-214), 1 on the perturbation (step_tl), 2 the adjoint
 *       (step_ad :286-350: the transposed sweeps).  The operator order is the host's, as in fv3jedi_lm_mod.F90:161-187:
 *       tangent  fv3lm_step_tl ; fv3lm_turbulence(h, slot, 1)      adjoint  fv3lm_turbulence(h, slot, 2) ; fv3lm_step_ad.
 *       Refused: before create, slot out of range, a slot never set, a mode outside 0..2.
 *   fv3lm_turbulence_get: out[10] = the LU factors in the order of diag (A the multipliers, B the inverse pivots, C unchanged) and pk. */
int fv3lm_turbulence_create(fv3lm_handle* h, int nslots);
int fv3lm_turbulence_set_diagonals(fv3lm_handle* h, int slot, const double* const* diag);
int fv3lm_turbulence_set_simple(fv3lm_handle* h, int slot, const double* frocean);
int fv3lm_turbulence(fv3lm_handle* h, int slot, int mode);
int fv3lm_turbulence_get(fv3lm_handle* h, int slot, double* const* out);
/* BL_DRIVER (physics/turbulence/bldriver.F90, Louis + Lock) on the device: the nine diagonals set_ltraj
 * (fv3jedi_lm_turbulence_mod.F90:376-540) computes, from the RESIDENT TRAJECTORY at the call -- u, v at (i, j), T, delp, qv = q1, pe
 * accumulated from ptop, pk, theta = p00^kappa T / pk -- written into the slot together with pk and factorised like those of
 * fv3lm_turbulence_set_diagonals; the same rules hold (call after fv3lm_traj_to_fv3 and before the step; the slot keeps what the call saw).
 *   fv3lm_bl_params: TURBPARAMS(22), TURBPARAMSI(4) in the reference's order (LOUIS LAMBDAM LAMBDAM2 LAMBDAH LAMBDAH2 ZKMENV ZKHENV
 *       MINTHICK MINSHEAR C_B LAMBDA_B AKHMMAX PRANDTLSFC PRANDTLRAD BETA_RAD BETA_SURF KHRADFAC KHSFCFAC TPFAC_SURF ENTRATE_SURF PCEFF_SURF
 *       LOUIS_MEMORY; KPBLMIN LOCK_ON PBLHT_OPTION RADLW_DEP).  The reference never assigns them: they are the host's.
 *       fv3lm_bl_default_params fills in the set documented at bldriver.F90:100-127; KPBLMIN = count(PREF < 50000) is the caller's.
 *   sfc[9] = FRLAND FROCEAN VARFLT ZPBL CM CT CQ USTAR BSTAR, compact (isc:iec, jsc:jec) per tile; they are not modified.
 *   cloud_mode 0: qa, qb = QI, QL (compact, npz deep; NULL = zero).  cloud_mode 1: qa, qb = QLS, QCN, split on the device by
 *       IceFraction(T) as set_ltraj:455-464 does.
 *   raw_out: NULL, or 13 compact arrays that receive what BL_DRIVER left BEFORE the factorisation: AKV BKV CKV AKS BKS CKS AKQ BKQ CKQ
 *       (the order of diag), EKV, FKV (npz deep), then ZPBL and CT (2-D) as updated.  Its staging is only allocated when it is given.
 *   LOCK_ON and PBLHT_OPTION are read and never tested by the reference; LOCK_DIFF always runs.  The constants are those of
 *   fv3jedi_lm_const_mod, which the routine uses; pk and theta take akap and ptop of the options.
 *   Refused with a message, the slot left unset: before fv3lm_turbulence_create; slot out of range; npz < 7 (the smooth of the bottom six
 *   levels); nq < 1; KPBLMIN outside 1..npz; RADLW_DEP != 0 (the reference reads an uninitialised array there); dt <= 0; a NULL among
 *   sfc or in a raw_out that is given; cloud_mode outside 0..1; a column with BSTAR > 0 whose surface parcel never reaches its level of
 *   neutral buoyancy (the reference would index with an unset ipbl); a zero or non-finite pivot of the diagonals. */
typedef struct { double r[22]; int i[4]; } fv3lm_bl_params;
void fv3lm_bl_default_params(fv3lm_bl_params* p, int kpblmin);
int fv3lm_turbulence_set_driver(fv3lm_handle* h, int slot, const fv3lm_bl_params* p, double dt, const double* const* sfc, const double* qa,
                                const double* qb, int cloud_mode, double* const* raw_out);
/* Linearised relaxed Arakawa-Schubert convection (physics/moist/convection.F90 RASE, RASE0 with their tangents convection_tl.F90 and
 * adjoint convection_ad.F90, and the part of fv3jedi_lm_moist_mod.F90 that concerns them: create :120-148, :226-238, set_ltraj :700-832 with
 * jacobian_filter_tlm, step_nl / step_tl / step_ad up to the cloud scheme).  Column-local, like the turbulence: compact (isc:iec, jsc:jec
 * [, npz]) arrays per resident tile, tile slowest; nothing outside is..ie x js..je is read or written; delp, w, delz, q2.. are not touched.
 *   fv3lm_ras_params: RASPARAMS(1:25).  fv3lm_ras_default_params fills in create :120-148; entry 23 follows imsize = 4 im.
 *   fv3lm_convection_create: nslots slots (one per trajectory time kept), do_phy_mst 1 | 2 (MAXCONDEP 1 | 10 of the heating-rate filter).
 *       ICMIN and SIGE come from the handle's ak, bk; the table is ESINIT's; the MAPL constants are those of utils/MAPL_Constants.F90 in
 *       double; p00 and kappa of T <-> theta are the options'.  ALL device memory of the feature is allocated here (FV3LM_VERBOSE=1
 *       prints it) and freed by fv3lm_destroy.
 *   fv3lm_convection_set: takes the trajectory from the RESIDENT u v pt(= T) delp q1 at the call (with dt, ptop of the handle) and ts,
 *       frland, kcbl (nint of a real) of the host; runs RASE0 on copies, the heating-rate filter and the Jacobian filter (its loop is
 *       L = 1, 1 in the reference: only the column of PT_pert = e_KCBL exists, thresholds 1e-4 and 1e-7) and lists the DOCONVEC columns.
 *       A slot keeps what set saw and no run modifies it: this is the device's form of "a fresh set_ltraj every step".
 *   fv3lm_convection_get: out6 = PTT_C QVT_C CNV_DQLDT_C CNV_MFD_C CNV_PRC3_C CNV_UPDF_C (npz deep), doconvec (one int a column), jac2
 *       (NULL ok) = H_pert then M_pert of the Jacobian filter, npz deep each, zero where the heating-rate filter had already refused.
 *   fv3lm_convection_sources: the four sources of the PERTURBATION, CNV_DQLDT CNV_MFD CNV_PRC3 CNV_UPDF (npz deep): put = 0 reads them
 *       (after a tangent run), put = 1 writes them (the incoming adjoints, before an adjoint run).
 *   fv3lm_convection: DOCONVEC columns only.  mode 0: RASE on the trajectory, u v T q1 written back (step_nl); 1: RASE_D on the
 *       perturbation of u v pt q1, T -> theta by p00^kappa / pk in and back out, the sources cleared and then written in the active
 *       columns; 2: RASE_B, theta = T pk / p00^kappa in and its inverse out, the sources are consumed and cleared.  Host order, as
 *       fv3jedi_lm_mod.F90:161-187 and fv3jedi_lm_physics_mod.F90:121-122, :137-138 (the moist half before the turbulence in the
 *       tangent, after it in the adjoint):  tangent  fv3lm_step_tl ; fv3lm_convection(1) ; fv3lm_turbulence(1)
 *                                           adjoint  fv3lm_turbulence(2) ; fv3lm_convection(2) ; fv3lm_step_ad.
 *   fv3lm_convection_table: diagnostics -- the 18301 entries of the saturation table as they lie on the device (ESINIT, 150 K .. 333 K in
 *       steps of 0.01 K) and the nine constants of the kernels: CP ALHL GRAV RGAS H2OMW AIRMW VIREPS P00 KAPPA (MAPL_Constants in double).
 *   Refused with a message, the slot left unset: before create or a second create; nslots < 1; do_phy_mst outside 1..2; a handle without
 *   ak, bk; nq < 1; a slot out of range or never set; a mode outside 0..2; a NULL array; kcbl outside ICMIN+1 .. npz; a value that is
 *   not finite; an allocation that fails. */
typedef struct { double r[25]; } fv3lm_ras_params;
void fv3lm_ras_default_params(fv3lm_ras_params* p, int im);
int fv3lm_convection_create(fv3lm_handle* h, int nslots, const fv3lm_ras_params* p, int do_phy_mst);
int fv3lm_convection_set(fv3lm_handle* h, int slot, const double* ts, const double* frland, const double* kcbl);
int fv3lm_convection_get(fv3lm_handle* h, int slot, double* const* out6, int* doconvec, double* jac2);
int fv3lm_convection_sources(fv3lm_handle* h, int put, double* const* src4);
int fv3lm_convection(fv3lm_handle* h, int slot, int mode);
int fv3lm_convection_table(fv3lm_handle* h, double* table, double* constants);
/* Linearised cloud scheme of the moist physics (physics/moist/cloud.F90 CLOUD_DRIVER, its tangent cloud_tl.F90 CLOUD_DRIVER_D and adjoint
 * cloud_ad.F90 CLOUD_DRIVER_B, and the part of fv3jedi_lm_moist_mod.F90 after the rase loops: create :151-211, set_ltraj :834-874, step_nl
 * :365-388, step_tl :429-438 / :495-501, step_ad :542-551 / :607-616).  Column-local; it follows the convection in every column and reads
 * that feature's slot of the same number.  Compact arrays as for the convection.
 *   fv3lm_cloud_params: CLOUDPARAMS(1:57).  fv3lm_cloud_default_params fills in create :151-211; entries 42 and 46 follow imsize = 4 im.
 *   fv3lm_cloud_create: after fv3lm_convection_create, whose do_phy_mst, table, constants and slot count it takes (one cloud slot per
 *       convection slot).  iqi, iql (2..nq, distinct) name the tracers that carry cloud ice and cloud liquid, of the perturbation and of the
 *       trajectory.  ALL device memory of the feature is allocated here (FV3LM_VERBOSE=1 prints it) and freed by fv3lm_destroy.
 *   fv3lm_cloud_set: after fv3lm_convection_set of the same slot, on the same resident trajectory (PLE in Pa is taken from the resident
 *       delp).  QLS, QCN, cfcn (npz deep) and khl, khu (nint of a real) are the host's; PTT_C, QVT_C, the four _C sources, ple, pk and frland
 *       are the convection slot's.  Computes fQi = IceFraction(TEMP) with the GEOS pk, QILST QLLST QICNT QLCNT, the fractions ILSF ICNF
 *       LLSF LCNF, CLOUD_DRIVER in values and, for do_phy_mst = 2, the per-cell switch cloud_pertmod (the eigenvalues of the 8 x 8
 *       Jacobian of LS_CLOUD_D and its four entry thresholds, cloud_tl.F90:405-481).  No later call modifies a slot; a later
 *       fv3lm_convection_set of that slot unsets it.  The reference's cloud_driver_d updates its saved trajectory in place, so a second
 *       call on a saved ltraj sees a trajectory that has been through the cloud scheme already: that is not reproduced.
 *   fv3lm_cloud_get: out8 = theta, q, QI_ls, QL_ls, QI_con, QL_con, CF_ls, CF_con after CLOUD_DRIVER in values; frac4 = ILSF ICNF LLSF
 *       LCNF; pertmod = the switch, one int a cell (all 1 for do_phy_mst = 1).  NULL is allowed for each.
 *   fv3lm_cloud_cfcn: the perturbation's convective cloud fraction (npz deep), which the feature owns on the device: put = 0 reads, 1 writes.
 *   fv3lm_cloud_bind_cfcn: opt-in, after fv3lm_cloud_create and before the first fv3lm_cloud_set.  From then on the convective cloud
 *       fraction of this handle IS tracer iqc of the dycore (1-based, 2..nq, neither iqi nor iql), as the reference's fifth tracer with
 *       do_phy_mst /= 0 (fv3jedi_lm_dynamics_mod.F90:159-163, :769, :831, :878, :912): the trajectory half is the trajectory cfcn, the
 *       perturbation half is cfcn' or its adjoint, and the dynamics transports both.  The tangent and adjoint kernels then read and write
 *       that tracer's perturbation in place of the feature's array.  fv3lm_cloud_set accepts cfcn = NULL and takes the resident trajectory
 *       of tracer iqc (set_ltraj :720; a non-NULL array is used as before); fv3lm_cloud(slot, 0) also writes CF_con to the trajectory of
 *       tracer iqc on is..ie x js..je (step_nl :388); fv3lm_cloud_cfcn moves is..ie x js..je of the tracer's perturbation (a put leaves
 *       zeros outside, as fv3lm_pert_to_fv3 does); fv3lm_lm_step clears the tracer's perturbation, whole padded planes, before and after
 *       a step and nothing clears it in between, so the tangent the transport of the trajectory's cfcn leaves there reaches
 *       CLOUD_DRIVER_D (fv3jedi_lm_moist_mod.F90:438) and the adjoint CLOUD_DRIVER_B leaves there (:616) reaches FV_DYNAMICS_BWD.  A
 *       handle that never binds keeps cfcn out of the dynamics (a host that owns cfcn routes it itself).  Refused with a message, the
 *       handle left as it was: before fv3lm_cloud_create; a second bind; iqc outside 2..nq or equal to iqi or iql; after a cloud slot
 *       has been set.
 *   fv3lm_cloud: every column.  mode 0: CLOUD_DRIVER in values on copies of the slot; qi = QI_ls + QI_con and ql = QL_ls + QL_con go to
 *       the resident trajectory tracers iqi, iql (CF_con is what get returns); T and qv are not touched.  1: T -> theta by p00^kappa / pk,
 *       qi and ql split by the fractions, cflsp = 0, cfcn as put, the four sources as fv3lm_convection(1) left them; after the driver
 *       the parts are summed, theta goes back to T, cfcn is updated.  2: theta = T pk / p00^kappa, both parts of qi and ql receive the
 *       full adjoint; after the driver they are combined with the fractions and the adjoints of the four sources are written where
 *       fv3lm_convection(2) consumes them.  Host order:
 *           tangent  fv3lm_step_tl ; fv3lm_convection(1) ; fv3lm_cloud(1) ; fv3lm_turbulence(1)
 *           adjoint  fv3lm_turbulence(2) ; fv3lm_cloud(2) ; fv3lm_convection(2) ; fv3lm_step_ad
 *       (fv3jedi_lm_physics_mod.F90:121-122, :137-138); fv3lm_lm_step below runs exactly this.
 *   Refused with a message, the slot left unset: before fv3lm_convection_create or a second create; iqi / iql out of range or equal;
 *   CLOUDPARAMS(57) /= 1 (only the top-hat PDF is built); a slot whose convection slot was never set; a slot out of range or never set; a
 *   mode outside 0..2; a NULL array where one is required; khl / khu outside 1..npz; a value that is not finite; an allocation that
 *   fails; a tape that overflows in the adjoint. */
typedef struct { double r[57]; } fv3lm_cloud_params;
void fv3lm_cloud_default_params(fv3lm_cloud_params* p, int im);
int fv3lm_cloud_create(fv3lm_handle* h, const fv3lm_cloud_params* p, int iqi, int iql);
int fv3lm_cloud_bind_cfcn(fv3lm_handle* h, int iqc);
int fv3lm_cloud_set(fv3lm_handle* h, int slot, const double* qls, const double* qcn, const double* cfcn, const double* khl, const double* khu);
int fv3lm_cloud_get(fv3lm_handle* h, int slot, double* const* out8, double* const* frac4, int* pertmod);
int fv3lm_cloud_cfcn(fv3lm_handle* h, int put, double* cfcn);
int fv3lm_cloud(fv3lm_handle* h, int slot, int mode);
/* The composed model step: fv3jedi_lm_mod's step_tl / step_ad (src/fv3jedi_lm_mod.F90:161-187), the dynamics and the column physics of
 * one time step in the reference's order, about the trajectory of a stored time.
 *   fv3lm_lm_create: nslots trajectory slots in one allocation, all or nothing (a refusal names FV3LM_TRAJ_SLOTS: fv3lm_create has by
 *       then taken the acoustic-step slots from free memory).  A slot holds what fv3lm_traj_to_fv3 leaves resident of the trajectory:
 *       u v pt delp q* (w delz on a non-hydrostatic handle) and phis, whole padded planes.  do_dyn, do_phy_trb, do_phy_mst: conf%do_dyn,
 *       conf%do_phy_trb and whether conf%do_phy_mst /= 0, each 0 or 1 (its value 1 or 2 stays with fv3lm_convection_create); a flag may
 *       be set before the feature it names is created, the check is made at the step.
 *   fv3lm_lm_traj_save: the resident trajectory, halos included, into the slot by device-to-device copies; the slot is then set.  The
 *       physics slots carry the same number: the host sets them (fv3lm_convection_set, fv3lm_cloud_set, fv3lm_turbulence_set_*) while
 *       the trajectory of that time is resident, then saves it.
 *   fv3lm_lm_traj_load: the slot back; the handle is then as after fv3lm_traj_to_fv3 of the same host arrays, bit for bit (halos, D-grid
 *       edge rows, halo of phis; pe peln pk pkz computed again from delp as the upload does).  Neither call touches the perturbation.
 *   fv3lm_lm_step: mode 1 tangent, 2 adjoint, on the resident perturbation.  ipert_to_zero (:167, :170, :182, :185, :242-253) clears the
 *       device's cfcn perturbation before and after either (where the cloud feature exists).  Without fv3lm_cloud_bind_cfcn that array is
 *       the cloud feature's own and the dynamics never sees it: the cloud tangent starts from cfcn' = 0 and the cfcn adjoint it leaves is
 *       dropped, which the reference does not do; with it, cfcn is a tracer and the coupling is the reference's.
 *           tangent (:161-172; physics fv3jedi_lm_physics_mod.F90:121-122)
 *               do_dyn: traj_load(slot) ; fv3lm_step_tl      do_phy_mst: convection(slot, 1) ; cloud(slot, 1)      do_phy_trb: turbulence(slot, 1)
 *           adjoint (:176-187; physics :137-138)
 *               do_phy_trb: turbulence(slot, 2)      do_phy_mst: cloud(slot, 2) ; convection(slot, 2)
 *               do_dyn: traj_load(slot) ; fv3lm_step_nl ; fv3lm_step_ad (the dynamics' step_ad is forward sweep + backward sweep)
 *       A part that fails (a tape overflow, a pending device failure) ends the step with its own message; nothing runs after it.
 *   Refused with a message before anything is run or cleared: before create or a second create; nslots < 1; a flag outside 0..1 or all
 *   three 0; a slot out of range; a load, or a step with do_dyn, of a slot never saved; a mode other than 1 or 2 (the nonlinear step is
 *   composed from the parts: its physics must be set from the trajectory the dynamics has just advanced); a physics flag whose feature
 *   was never created or whose slot was never set; do_phy_mst with the convection created and the cloud scheme not. */
int fv3lm_lm_create(fv3lm_handle* h, int nslots, int do_dyn, int do_phy_trb, int do_phy_mst);
int fv3lm_lm_traj_save(fv3lm_handle* h, int slot);   /* resident trajectory -> slot */
int fv3lm_lm_traj_load(fv3lm_handle* h, int slot);   /* slot -> resident trajectory */
int fv3lm_lm_step(fv3lm_handle* h, int slot, int mode);   /* mode 1 tangent, 2 adjoint */
/* Per-kernel HIP-event profile of everything launched between begin and end, on the library's stream:
 * lines "kernel count total_ms algorithmic_bytes".  Returns the buffer length needed. */
int fv3lm_profile_begin(fv3lm_handle* h);
int fv3lm_profile_end(fv3lm_handle* h, char* buf, int buflen);
int fv3lm_set_device(int dev);                 /* one process per GPU: select the device before fv3lm_create */
int fv3lm_state_save(fv3lm_handle* h);         /* device-side snapshot of u v pt delp q* (traj + pert) */
int fv3lm_state_restore(fv3lm_handle* h);
int fv3lm_zero_work_adjoint(fv3lm_handle* h);
int fv3lm_sync(fv3lm_handle* h);
long fv3lm_launch_count(fv3lm_handle* h);
long fv3lm_tp2_launch_count(fv3lm_handle* h);  /* of them, fv_tp_2d launches in the wavefront layout */
int fv3lm_level_params(fv3lm_handle* h, int k, int* iparams10, double* rparams6);

#ifdef __cplusplus
}
#endif
#endif
