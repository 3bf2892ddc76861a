!> fv3lm_hip_mod — ISO_C_BINDING shim between the Fortran host (FV3-JEDI / fv3jedi_lm_dynamics_mod)
!! and the MI355X-native TL/AD dynamical core behind the C-ABI of include/fv3lm.h.
!!
!! The host keeps everything it does today (trajectory management, traj/pert -> FV_Atm copies, the
!! mpp_get_boundary edge fill, fv3_to_pert); only the calls that fv3jedi_lm_dynamics_mod makes into
!! the Tapenade code are replaced (INTEGRATION.md shows the three edited call sites):
!!   create  : call fv3lm_hip_create(...)  after fv_init / fv_init_pert  (fv3jedi_lm_dynamics_mod.F90:155)
!!   step_tl : call fv3lm_hip_step_tl(...) in place of compute_fv3_pressures_tlm + fv_dynamics_tlm (:404-438)
!!   step_ad : call fv3lm_hip_step_ad(...) in place of fv_dynamics_fwd / fv_dynamics_bwd / compute_fv3_pressures_bwd (:507-638)
!!   delete  : call fv3lm_hip_destroy(...) (:693-713)
!! A nonzero status from the library becomes a fatal error, as the reference does with
!! mpp_error(FATAL)/exit(1) (src/fv3jedi_lm_mod.F90:93).
module fv3lm_hip_mod
  use iso_c_binding
  implicit none
  private
  public :: fv3lm_options, fv3lm_dims, fv3lm_hip_type
  public :: fv3lm_hip_create, fv3lm_hip_destroy, fv3lm_hip_put, fv3lm_hip_get
  public :: fv3lm_hip_step_tl, fv3lm_hip_step_ad
  public :: fv3lm_hip_traj_to_fv3, fv3lm_hip_pert_to_fv3, fv3lm_hip_fv3_to_pert
  public :: fv3lm_hip_set_tracer_damping, fv3lm_hip_tracer_damping
  public :: fv3lm_hip_set_external_damping, fv3lm_hip_external_damping
  public :: fv3lm_hip_set_trajectory_damping_order, fv3lm_hip_trajectory_damping_order
  public :: fv3lm_hip_set_rayleigh, fv3lm_hip_rayleigh_profile
  public :: fv3lm_hip_turbulence_create, fv3lm_hip_turbulence_set_diagonals, fv3lm_hip_turbulence_set_simple
  public :: fv3lm_hip_turbulence, fv3lm_hip_turbulence_get
  public :: fv3lm_bl_params, fv3lm_hip_bl_default_params, fv3lm_hip_turbulence_set_driver
  public :: fv3lm_ras_params, fv3lm_hip_ras_default_params, fv3lm_hip_convection_create, fv3lm_hip_convection_set
  public :: fv3lm_hip_convection_get, fv3lm_hip_convection_get_sources, fv3lm_hip_convection_put_sources, fv3lm_hip_convection
  public :: fv3lm_hip_convection_table
  public :: fv3lm_cloud_params, fv3lm_hip_cloud_default_params, fv3lm_hip_cloud_create, fv3lm_hip_cloud_set, fv3lm_hip_cloud_get
  public :: fv3lm_hip_cloud_get_cfcn, fv3lm_hip_cloud_put_cfcn, fv3lm_hip_cloud

  integer, parameter :: ng = 3   ! halo width, tools/fv_mp_nlm_mod.F90:67

  !> mirrors `struct fv3lm_options` (include/fv3lm.h) field for field
  type, bind(C) :: fv3lm_options
    integer(c_int) :: hord_mt, hord_vt, hord_tm, hord_dp, hord_tr
    integer(c_int) :: nord, do_vort_damp, n_sponge
    integer(c_int) :: hord_mt_pert, hord_vt_pert, hord_tm_pert, hord_dp_pert, hord_tr_pert
    integer(c_int) :: nord_pert, do_vort_damp_pert, n_sponge_pert, hord_ks_traj, hord_ks_pert
    integer(c_int) :: hord_mt_ks_traj, hord_vt_ks_traj, hord_tm_ks_traj, hord_dp_ks_traj, hord_tr_ks_traj
    integer(c_int) :: hord_mt_ks_pert, hord_vt_ks_pert, hord_tm_ks_pert, hord_dp_ks_pert, hord_tr_ks_pert
    integer(c_int) :: kord_tm, kord_mt, kord_wz, kord_tr
    integer(c_int) :: kord_tm_pert, kord_mt_pert, kord_wz_pert, kord_tr_pert
    integer(c_int) :: hydrostatic, split_damp
    real(c_double) :: dddmp, d2_bg, d4_bg, vtdm4, d2_bg_k1, d2_bg_k2, d_con, ke_bg
    real(c_double) :: dddmp_pert, d2_bg_pert, d4_bg_pert, vtdm4_pert, d2_bg_k1_pert, d2_bg_k2_pert, d2_bg_ks_pert
    real(c_double) :: akap, cp, zvir, grav_jedi
    real(c_double) :: cp_air, rdgas, rvgas, grav, radius, omega, hlv
    real(c_double) :: ptop
    real(c_double) :: a_imp, p_fac, scale_z
  end type fv3lm_options

  type, bind(C) :: fv3lm_dims
    integer(c_int) :: nx, ny, npz, ntile, nq, n_split, k_split
    integer(c_int) :: face   ! 1: every resident tile is a whole cube face (edge/corner branches on); 0: one edge-free periodic tile
    real(c_double) :: dt
    ! sub-face tiles (layout > 1 x 1): cells per edge of a whole face (0: the tile is the face) and, per resident tile, (is, js) in the global
    ! indices of its face (c_null_ptr: (1, 1)); nx, ny are then the cells of a tile
    integer(c_int) :: nface = 0, pad_ = 0
    type(c_ptr) :: tile_ij0 = c_null_ptr
  end type fv3lm_dims

  !> TURBPARAMS(22), TURBPARAMSI(4) of BL_DRIVER in the reference's order (fv3lm_bl_params of include/fv3lm.h)
  type, bind(C) :: fv3lm_bl_params
    real(c_double) :: r(22)
    integer(c_int) :: i(4)
  end type fv3lm_bl_params

  !> RASPARAMS(1:25) of the moist physics (fv3lm_ras_params of include/fv3lm.h)
  type, bind(C) :: fv3lm_ras_params
    real(c_double) :: r(25)
  end type fv3lm_ras_params
  !> CLOUDPARAMS(1:57) of the moist physics (fv3lm_cloud_params of include/fv3lm.h)
  type, bind(C) :: fv3lm_cloud_params
    real(c_double) :: r(57)
  end type fv3lm_cloud_params

  type :: fv3lm_hip_type
    type(c_ptr) :: handle = c_null_ptr
    integer :: nx = 0, ny = 0, npz = 0
  end type fv3lm_hip_type

  interface
    function c_create(h, dims, opt, metrics, da_min, da_min_c, phis, ak, bk) bind(C, name="fv3lm_create") result(rc)
      import :: c_ptr, c_int, c_double, fv3lm_dims, fv3lm_options
      type(c_ptr), intent(out) :: h
      type(fv3lm_dims), intent(in) :: dims
      type(fv3lm_options), intent(in) :: opt
      type(c_ptr), intent(in) :: metrics(*)
      real(c_double), value :: da_min, da_min_c
      real(c_double), intent(in) :: phis(*), ak(*), bk(*)
      integer(c_int) :: rc
    end function
    function c_set_face_data(h, edge, ecorner) bind(C, name="fv3lm_set_face_data") result(rc)
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(in) :: edge(*), ecorner(*)
      integer(c_int) :: rc
    end function
    function c_set_rayleigh(h, tau, rf_cutoff, c2l) bind(C, name="fv3lm_set_rayleigh") result(rc)
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h, c2l
      real(c_double), value :: tau, rf_cutoff
      integer(c_int) :: rc
    end function
    function c_rayleigh_profile(h, rf, kmax) bind(C, name="fv3lm_rayleigh_profile") result(rc)
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(out) :: rf(*)
      integer(c_int), intent(out) :: kmax
      integer(c_int) :: rc
    end function
    function c_set_tracer_damping(h, nord_tr, trdm2, nord_tr_pert, trdm2_pert, split_damp_tr) &
        bind(C, name="fv3lm_set_tracer_damping") result(rc)
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      integer(c_int), value :: nord_tr, nord_tr_pert, split_damp_tr
      real(c_double), value :: trdm2, trdm2_pert
      integer(c_int) :: rc
    end function
    function c_tracer_damping(h, nord2, trdm2) bind(C, name="fv3lm_tracer_damping") result(rc)
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      integer(c_int), intent(out) :: nord2(2)
      real(c_double), intent(out) :: trdm2(2)
      integer(c_int) :: rc
    end function
    function c_set_external_damping(h, d_ext) bind(C, name="fv3lm_set_external_damping") result(rc)
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), value :: d_ext
      integer(c_int) :: rc
    end function
    function c_external_damping(h, d_ext) bind(C, name="fv3lm_external_damping") result(rc)
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: h
      real(c_double), intent(out) :: d_ext
      integer(c_int) :: rc
    end function
    function c_set_trajectory_damping_order(h, nord) bind(C, name="fv3lm_set_trajectory_damping_order") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: nord
      integer(c_int) :: rc
    end function
    function c_trajectory_damping_order(h, nord) bind(C, name="fv3lm_trajectory_damping_order") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), intent(out) :: nord
      integer(c_int) :: rc
    end function
    function c_set_exchange(h, kind, rows, nrows) bind(C, name="fv3lm_set_exchange") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: kind, nrows
      integer(c_int), intent(in) :: rows(*)
      integer(c_int) :: rc
    end function
    function c_set_exchange_remote(h, kind, npeers, peers, nsend, send_rows, nrecv, recv_rows) &
        bind(C, name="fv3lm_set_exchange_remote") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: kind, npeers
      integer(c_int), intent(in) :: peers(*), nsend(*), send_rows(*), nrecv(*), recv_rows(*)
      integer(c_int) :: rc
    end function
    function c_comm_init(rccl_path, id128, nranks, rank) bind(C, name="fv3lm_comm_init") result(rc)
      import :: c_char, c_int
      character(kind=c_char), intent(in) :: rccl_path(*), id128(*)
      integer(c_int), value :: nranks, rank
      integer(c_int) :: rc
    end function
    function c_comm_unique_id(rccl_path, id128) bind(C, name="fv3lm_comm_unique_id") result(rc)
      import :: c_char, c_int
      character(kind=c_char), intent(in) :: rccl_path(*)
      character(kind=c_char), intent(out) :: id128(*)
      integer(c_int) :: rc
    end function
    function c_destroy(h) bind(C, name="fv3lm_destroy") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int) :: rc
    end function
    function c_put(h, name, which, host) bind(C, name="fv3lm_field_put") result(rc)
      import :: c_ptr, c_int, c_char, c_double
      type(c_ptr), value :: h
      character(kind=c_char), intent(in) :: name(*)
      integer(c_int), value :: which
      real(c_double), intent(in) :: host(*)
      integer(c_int) :: rc
    end function
    function c_get(h, name, which, host) bind(C, name="fv3lm_field_get") result(rc)
      import :: c_ptr, c_int, c_char, c_double
      type(c_ptr), value :: h
      character(kind=c_char), intent(in) :: name(*)
      integer(c_int), value :: which
      real(c_double), intent(out) :: host(*)
      integer(c_int) :: rc
    end function
    function c_step_tl(h) bind(C, name="fv3lm_step_tl") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int) :: rc
    end function
    function c_step_nl(h) bind(C, name="fv3lm_step_nl") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int) :: rc
    end function
    function c_step_ad(h) bind(C, name="fv3lm_step_ad") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int) :: rc
    end function
    function c_traj_to_fv3(h, u, v, t, delp, q, w, delz, phis) bind(C, name="fv3lm_traj_to_fv3") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h, u, v, t, delp, w, delz, phis
      type(c_ptr), intent(in) :: q(*)
      integer(c_int) :: rc
    end function
    function c_pert_to_fv3(h, u, v, t, delp, q, w, delz) bind(C, name="fv3lm_pert_to_fv3") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h, u, v, t, delp, w, delz
      type(c_ptr), intent(in) :: q(*)
      integer(c_int) :: rc
    end function
    function c_fv3_to_pert(h, u, v, t, delp, q, w, delz) bind(C, name="fv3lm_fv3_to_pert") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h, u, v, t, delp, w, delz
      type(c_ptr), intent(in) :: q(*)
      integer(c_int) :: rc
    end function
    function c_turbulence_create(h, nslots) bind(C, name="fv3lm_turbulence_create") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: nslots
      integer(c_int) :: rc
    end function
    function c_turbulence_set_diagonals(h, slot, diag) bind(C, name="fv3lm_turbulence_set_diagonals") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: slot
      type(c_ptr), intent(in) :: diag(*)
      integer(c_int) :: rc
    end function
    function c_turbulence_set_simple(h, slot, frocean) bind(C, name="fv3lm_turbulence_set_simple") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h, frocean
      integer(c_int), value :: slot
      integer(c_int) :: rc
    end function
    function c_turbulence(h, slot, mode) bind(C, name="fv3lm_turbulence") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: slot, mode
      integer(c_int) :: rc
    end function
    function c_turbulence_get(h, slot, out) bind(C, name="fv3lm_turbulence_get") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: slot
      type(c_ptr), intent(in) :: out(*)
      integer(c_int) :: rc
    end function
    subroutine c_bl_default_params(p, kpblmin) bind(C, name="fv3lm_bl_default_params")
      import :: fv3lm_bl_params, c_int
      type(fv3lm_bl_params), intent(out) :: p
      integer(c_int), value :: kpblmin
    end subroutine
    function c_turbulence_set_driver(h, slot, p, dt, sfc, qa, qb, cloud_mode, raw_out) bind(C, name="fv3lm_turbulence_set_driver") result(rc)
      import :: fv3lm_bl_params, c_ptr, c_int, c_double
      type(c_ptr), value :: h, qa, qb, raw_out
      integer(c_int), value :: slot, cloud_mode
      type(fv3lm_bl_params), intent(in) :: p
      real(c_double), value :: dt
      type(c_ptr), intent(in) :: sfc(*)
      integer(c_int) :: rc
    end function
    subroutine c_ras_default_params(p, im) bind(C, name="fv3lm_ras_default_params")
      import :: fv3lm_ras_params, c_int
      type(fv3lm_ras_params), intent(out) :: p
      integer(c_int), value :: im
    end subroutine
    function c_convection_create(h, nslots, p, do_phy_mst) bind(C, name="fv3lm_convection_create") result(rc)
      import :: fv3lm_ras_params, c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: nslots, do_phy_mst
      type(fv3lm_ras_params), intent(in) :: p
      integer(c_int) :: rc
    end function
    function c_convection_set(h, slot, ts, frland, kcbl) bind(C, name="fv3lm_convection_set") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h, ts, frland, kcbl
      integer(c_int), value :: slot
      integer(c_int) :: rc
    end function
    function c_convection_get(h, slot, out6, doconvec, jac2) bind(C, name="fv3lm_convection_get") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h, doconvec, jac2
      integer(c_int), value :: slot
      type(c_ptr), intent(in) :: out6(*)
      integer(c_int) :: rc
    end function
    function c_convection_sources(h, put, src4) bind(C, name="fv3lm_convection_sources") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: put
      type(c_ptr), intent(in) :: src4(*)
      integer(c_int) :: rc
    end function
    function c_convection_table(h, table, constants) bind(C, name="fv3lm_convection_table") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h, table, constants
      integer(c_int) :: rc
    end function
    function c_convection(h, slot, mode) bind(C, name="fv3lm_convection") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: slot, mode
      integer(c_int) :: rc
    end function
    subroutine c_cloud_default_params(p, im) bind(C, name="fv3lm_cloud_default_params")
      import :: fv3lm_cloud_params, c_int
      type(fv3lm_cloud_params), intent(out) :: p
      integer(c_int), value :: im
    end subroutine
    function c_cloud_create(h, p, iqi, iql) bind(C, name="fv3lm_cloud_create") result(rc)
      import :: fv3lm_cloud_params, c_ptr, c_int
      type(c_ptr), value :: h
      type(fv3lm_cloud_params), intent(in) :: p
      integer(c_int), value :: iqi, iql
      integer(c_int) :: rc
    end function
    function c_cloud_set(h, slot, qls, qcn, cfcn, khl, khu) bind(C, name="fv3lm_cloud_set") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h, qls, qcn, cfcn, khl, khu
      integer(c_int), value :: slot
      integer(c_int) :: rc
    end function
    function c_cloud_get(h, slot, out8, frac4, pertmod) bind(C, name="fv3lm_cloud_get") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h, pertmod
      integer(c_int), value :: slot
      type(c_ptr), intent(in) :: out8(*), frac4(*)
      integer(c_int) :: rc
    end function
    function c_cloud_cfcn(h, put, cfcn) bind(C, name="fv3lm_cloud_cfcn") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h, cfcn
      integer(c_int), value :: put
      integer(c_int) :: rc
    end function
    function c_cloud(h, slot, mode) bind(C, name="fv3lm_cloud") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: slot, mode
      integer(c_int) :: rc
    end function
    function c_last_error() bind(C, name="fv3lm_last_error") result(p)
      import :: c_ptr
      type(c_ptr) :: p
    end function
  end interface

contains

  subroutine check(rc, where)
    integer(c_int), intent(in) :: rc
    character(len=*), intent(in) :: where
    character(kind=c_char), pointer :: msg(:)
    integer :: n
    if (rc == 0) return
    call c_f_pointer(c_last_error(), msg, [512])
    n = 1
    do while (n < 512 .and. msg(n) /= c_null_char)
      n = n + 1
    end do
    write(*, '(4a)') 'FATAL fv3lm_hip ', where, ': ', transfer(msg(1:n-1), repeat(' ', n-1))
    call exit(1)      ! the reference's own failure mode, src/fv3jedi_lm_mod.F90:93
  end subroutine check

  !> metrics(:) holds c_loc of the 50 metric planes in the order of fv3lm_metric_names(), each
  !! (isd:ied+1, jsd:jed+1) — the host copies gridstruct%... into padded planes once at create.
  subroutine fv3lm_hip_create(self, dims, opt, metrics, da_min, da_min_c, phis, ak, bk)
    type(fv3lm_hip_type), intent(inout) :: self
    type(fv3lm_dims), intent(in) :: dims
    type(fv3lm_options), intent(in) :: opt
    type(c_ptr), intent(in) :: metrics(:)
    real(c_double), intent(in) :: da_min, da_min_c
    real(c_double), intent(in) :: phis(:, :), ak(:), bk(:)
    call check(c_create(self%handle, dims, opt, metrics, da_min, da_min_c, phis, ak, bk), 'create')
    self%nx = dims%nx; self%ny = dims%ny; self%npz = dims%npz
  end subroutine fv3lm_hip_create

  !> Face mode: a2b_ord4 edge weights gridstruct%edge_w/e/s/n as (pj, 4, ntile) and the extrap_corner factors (3, 4, ntile).
  subroutine fv3lm_hip_set_face_data(self, edge, ecorner)
    type(fv3lm_hip_type), intent(inout) :: self
    real(c_double), intent(in) :: edge(:, :, :), ecorner(:, :, :)
    call check(c_set_face_data(self%handle, edge, ecorner), 'set_face_data')
  end subroutine fv3lm_hip_set_face_data

  !> Rayleigh damping of the upper layers (RAYLEIGH_SUPER): flagstruct%tau (days; 0 = off), flagstruct%rf_cutoff (Pa) and the
  !! cubed-to-lat-lon matrices gridstruct%a11 a12 a21 a22 laid into the padded plane as (pi, pj, 4, ntile); c2l may be left out
  !! when tau = 0.  Call after fv3lm_hip_create, before the first step.
  subroutine fv3lm_hip_set_rayleigh(self, tau, rf_cutoff, c2l)
    type(fv3lm_hip_type), intent(inout) :: self
    real(c_double), intent(in) :: tau, rf_cutoff
    real(c_double), intent(in), target, contiguous, optional :: c2l(:, :, :, :)
    type(c_ptr) :: p
    p = c_null_ptr
    if (present(c2l)) p = c_loc(c2l)
    call check(c_set_rayleigh(self%handle, tau, rf_cutoff, p), 'set_rayleigh')
  end subroutine fv3lm_hip_set_rayleigh

  !> rf(1:npz) (0 below the cutoff) and kmax as the library computed them
  subroutine fv3lm_hip_rayleigh_profile(self, rf, kmax)
    type(fv3lm_hip_type), intent(inout) :: self
    real(c_double), intent(out) :: rf(:)
    integer(c_int), intent(out) :: kmax
    call check(c_rayleigh_profile(self%handle, rf, kmax), 'rayleigh_profile')
  end subroutine fv3lm_hip_rayleigh_profile

  !> Tracer damping of tracer_2d: FV_Atm(1)%flagstruct%nord_tr, %trdm2 and FV_AtmP(1)%flagstruct%nord_tr_pert, %trdm2_pert,
  !! %split_damp_tr (include/fv3lm.h).  Call after fv3lm_hip_create, before the first step or between complete steps.
  subroutine fv3lm_hip_set_tracer_damping(self, nord_tr, trdm2, nord_tr_pert, trdm2_pert, split_damp_tr)
    type(fv3lm_hip_type), intent(inout) :: self
    integer(c_int), intent(in) :: nord_tr, nord_tr_pert
    real(c_double), intent(in) :: trdm2, trdm2_pert
    logical, intent(in) :: split_damp_tr
    call check(c_set_tracer_damping(self%handle, nord_tr, trdm2, nord_tr_pert, trdm2_pert, merge(1_c_int, 0_c_int, split_damp_tr)), &
               'set_tracer_damping')
  end subroutine fv3lm_hip_set_tracer_damping

  !> the effective pairs: nord2 = (nord_tr, nord_tr_pert), trdm2 = (trdm2, trdm2_pert)
  subroutine fv3lm_hip_tracer_damping(self, nord2, trdm2)
    type(fv3lm_hip_type), intent(inout) :: self
    integer(c_int), intent(out) :: nord2(2)
    real(c_double), intent(out) :: trdm2(2)
    call check(c_tracer_damping(self%handle, nord2, trdm2), 'tracer_damping')
  end subroutine fv3lm_hip_tracer_damping

  !> External-mode divergence damping of the acoustic step: FV_Atm(1)%flagstruct%d_ext (include/fv3lm.h; 0 = off, the library's default).
  !! Call after fv3lm_hip_create, before the first step or between complete steps.
  subroutine fv3lm_hip_set_external_damping(self, d_ext)
    type(fv3lm_hip_type), intent(inout) :: self
    real(c_double), intent(in) :: d_ext
    call check(c_set_external_damping(self%handle, d_ext), 'set_external_damping')
  end subroutine fv3lm_hip_set_external_damping

  !> d_ext as set
  subroutine fv3lm_hip_external_damping(self, d_ext)
    type(fv3lm_hip_type), intent(inout) :: self
    real(c_double), intent(out) :: d_ext
    call check(c_external_damping(self%handle, d_ext), 'external_damping')
  end subroutine fv3lm_hip_external_damping

  !> The trajectory's divergence-damping order FV_Atm(1)%flagstruct%nord after create (include/fv3lm.h).  A non-hydrostatic host creates
  !! with nord = min(flagstruct%nord, nord_pert) and passes flagstruct%nord here: orders 2 and 3 are reached only this way.
  !! Call after fv3lm_hip_create, before the first step or between complete steps.
  subroutine fv3lm_hip_set_trajectory_damping_order(self, nord)
    type(fv3lm_hip_type), intent(inout) :: self
    integer(c_int), intent(in) :: nord
    call check(c_set_trajectory_damping_order(self%handle, nord), 'set_trajectory_damping_order')
  end subroutine fv3lm_hip_set_trajectory_damping_order

  !> nord as in force
  subroutine fv3lm_hip_trajectory_damping_order(self, nord)
    type(fv3lm_hip_type), intent(inout) :: self
    integer(c_int), intent(out) :: nord
    call check(c_trajectory_damping_order(self%handle, nord), 'trajectory_damping_order')
  end subroutine fv3lm_hip_trajectory_damping_order

  !> One halo-exchange table (kind 0..4, include/fv3lm.h): rows(7, n) for the faces resident on this GPU, and the
  !! per-peer send/receive lists for faces held by other ranks (replaces mpp_update_domains / mpp_get_boundary).
  subroutine fv3lm_hip_set_exchange(self, kind, rows)
    type(fv3lm_hip_type), intent(inout) :: self
    integer(c_int), intent(in) :: kind, rows(:, :)
    call check(c_set_exchange(self%handle, kind, rows, int(size(rows, 2), c_int)), 'set_exchange')
  end subroutine fv3lm_hip_set_exchange

  subroutine fv3lm_hip_set_exchange_remote(self, kind, peers, nsend, send_rows, nrecv, recv_rows)
    type(fv3lm_hip_type), intent(inout) :: self
    integer(c_int), intent(in) :: kind, peers(:), nsend(:), send_rows(:, :), nrecv(:), recv_rows(:, :)
    call check(c_set_exchange_remote(self%handle, kind, int(size(peers), c_int), peers, nsend, send_rows, nrecv, recv_rows), &
               'set_exchange_remote')
  end subroutine fv3lm_hip_set_exchange_remote

  !> RCCL communicator for the face exchange: rank 0 calls fv3lm_hip_comm_unique_id, the host broadcasts the 128 bytes
  !! (mpp_broadcast / MPI_Bcast), every rank calls fv3lm_hip_comm_init.
  subroutine fv3lm_hip_comm_unique_id(rccl_path, id128)
    character(len=*), intent(in) :: rccl_path
    character(kind=c_char), intent(out) :: id128(128)
    call check(c_comm_unique_id(trim(rccl_path)//c_null_char, id128), 'comm_unique_id')
  end subroutine fv3lm_hip_comm_unique_id

  subroutine fv3lm_hip_comm_init(rccl_path, id128, nranks, rank)
    character(len=*), intent(in) :: rccl_path
    character(kind=c_char), intent(in) :: id128(128)
    integer, intent(in) :: nranks, rank
    call check(c_comm_init(trim(rccl_path)//c_null_char, id128, int(nranks, c_int), int(rank, c_int)), 'comm_init')
  end subroutine fv3lm_hip_comm_init

  subroutine fv3lm_hip_destroy(self)
    type(fv3lm_hip_type), intent(inout) :: self
    if (c_associated(self%handle)) call check(c_destroy(self%handle), 'destroy')
    self%handle = c_null_ptr
  end subroutine fv3lm_hip_destroy

  !> Upload one FV_Atm / FV_AtmP array.  `a` has the reference's own bounds
  !! (ilo:ihi, jlo:jhi, nk), e.g. u(isd:ied, jsd:jed+1, npz) or traj%u(isc:iec, jsc:jec, npz);
  !! it is repacked into the padded plane (isd:ied+1, jsd:jed+1) the device uses.
  subroutine fv3lm_hip_put(self, name, which, a, ilo, jlo)
    type(fv3lm_hip_type), intent(in) :: self
    character(len=*), intent(in) :: name
    integer, intent(in) :: which, ilo, jlo
    real(c_double), intent(in) :: a(ilo:, jlo:, :)
    real(c_double), allocatable :: pad(:, :, :)
    allocate(pad(1-ng:self%nx+ng+1, 1-ng:self%ny+ng+1, size(a, 3)))
    pad = 0.0_c_double
    pad(ilo:ubound(a, 1), jlo:ubound(a, 2), :) = a
    call check(c_put(self%handle, trim(name)//c_null_char, int(which, c_int), pad), 'put '//name)
  end subroutine fv3lm_hip_put

  subroutine fv3lm_hip_get(self, name, which, a, ilo, jlo)
    type(fv3lm_hip_type), intent(in) :: self
    character(len=*), intent(in) :: name
    integer, intent(in) :: which, ilo, jlo
    real(c_double), intent(inout) :: a(ilo:, jlo:, :)
    real(c_double), allocatable :: pad(:, :, :)
    allocate(pad(1-ng:self%nx+ng+1, 1-ng:self%ny+ng+1, size(a, 3)))
    call check(c_get(self%handle, trim(name)//c_null_char, int(which, c_int), pad), 'get '//name)
    a = pad(ilo:ubound(a, 1), jlo:ubound(a, 2), :)
  end subroutine fv3lm_hip_get

  !> traj_to_fv3 / pert_to_fv3 / fv3_to_pert on the device (fv3jedi_lm_dynamics_mod.F90:717-933): the host's own traj% / pert% arrays,
  !! (isc:iec, jsc:jec, npz), no halo -- halos, D-grid edge rows, phis halo and pressures are the library's business.  q(:,:,:,n) in
  !! the reference's tracer order; w, delz only when hydrostatic = .false. (pass any array otherwise: not read).
  subroutine fv3lm_hip_traj_to_fv3(self, u, v, t, delp, q, phis, w, delz)
    type(fv3lm_hip_type), intent(in) :: self
    real(c_double), intent(in), target, contiguous :: u(:, :, :), v(:, :, :), t(:, :, :), delp(:, :, :), q(:, :, :, :), phis(:, :)
    real(c_double), intent(in), target, contiguous, optional :: w(:, :, :), delz(:, :, :)
    type(c_ptr) :: qp(max(1, size(q, 4))), wp, zp
    integer :: n
    do n = 1, size(q, 4)
      qp(n) = c_loc(q(1, 1, 1, n))
    end do
    wp = c_null_ptr; zp = c_null_ptr
    if (present(w)) wp = c_loc(w)
    if (present(delz)) zp = c_loc(delz)
    call check(c_traj_to_fv3(self%handle, c_loc(u), c_loc(v), c_loc(t), c_loc(delp), qp, wp, zp, c_loc(phis)), 'traj_to_fv3')
  end subroutine fv3lm_hip_traj_to_fv3

  subroutine fv3lm_hip_pert_to_fv3(self, u, v, t, delp, q, w, delz)
    type(fv3lm_hip_type), intent(in) :: self
    real(c_double), intent(in), target, contiguous :: u(:, :, :), v(:, :, :), t(:, :, :), delp(:, :, :), q(:, :, :, :)
    real(c_double), intent(in), target, contiguous, optional :: w(:, :, :), delz(:, :, :)
    type(c_ptr) :: qp(max(1, size(q, 4))), wp, zp
    integer :: n
    do n = 1, size(q, 4)
      qp(n) = c_loc(q(1, 1, 1, n))
    end do
    wp = c_null_ptr; zp = c_null_ptr
    if (present(w)) wp = c_loc(w)
    if (present(delz)) zp = c_loc(delz)
    call check(c_pert_to_fv3(self%handle, c_loc(u), c_loc(v), c_loc(t), c_loc(delp), qp, wp, zp), 'pert_to_fv3')
  end subroutine fv3lm_hip_pert_to_fv3

  subroutine fv3lm_hip_fv3_to_pert(self, u, v, t, delp, q, w, delz)
    type(fv3lm_hip_type), intent(in) :: self
    real(c_double), intent(inout), target, contiguous :: u(:, :, :), v(:, :, :), t(:, :, :), delp(:, :, :), q(:, :, :, :)
    real(c_double), intent(inout), target, contiguous, optional :: w(:, :, :), delz(:, :, :)
    type(c_ptr) :: qp(max(1, size(q, 4))), wp, zp
    integer :: n
    do n = 1, size(q, 4)
      qp(n) = c_loc(q(1, 1, 1, n))
    end do
    wp = c_null_ptr; zp = c_null_ptr
    if (present(w)) wp = c_loc(w)
    if (present(delz)) zp = c_loc(delz)
    call check(c_fv3_to_pert(self%handle, c_loc(u), c_loc(v), c_loc(t), c_loc(delp), qp, wp, zp), 'fv3_to_pert')
  end subroutine fv3lm_hip_fv3_to_pert

  !> Linearised boundary-layer turbulence (physics/turbulence/fv3jedi_lm_turbulence_mod.F90).  Slots are numbered from 1 here, like
  !! ltraj(conf%n) (:66-74); nslots = conf%nt with saveltraj, 1 without.  All arrays are the host's own, (isc:iec, jsc:jec, npz).
  subroutine fv3lm_hip_turbulence_create(self, nslots)
    type(fv3lm_hip_type), intent(in) :: self
    integer, intent(in) :: nslots
    call check(c_turbulence_create(self%handle, int(nslots, c_int)), 'turbulence_create')
  end subroutine fv3lm_hip_turbulence_create

  !> In set_ltraj after BL_DRIVER (:482-507), in place of the host's VTRILUPERT (:510-512): the diagonals as BL_DRIVER returns them.
  !! pk comes from the trajectory delp resident on the device: call after fv3lm_hip_traj_to_fv3 and before the dynamics' step.
  subroutine fv3lm_hip_turbulence_set_diagonals(self, slot, akv, bkv, ckv, aks, bks, cks, akq, bkq, ckq)
    type(fv3lm_hip_type), intent(in) :: self
    integer, intent(in) :: slot
    real(c_double), intent(in), target, contiguous :: akv(:, :, :), bkv(:, :, :), ckv(:, :, :), aks(:, :, :), bks(:, :, :), cks(:, :, :)
    real(c_double), intent(in), target, contiguous :: akq(:, :, :), bkq(:, :, :), ckq(:, :, :)
    type(c_ptr) :: d(9)
    d = [c_loc(akv), c_loc(bkv), c_loc(ckv), c_loc(aks), c_loc(bks), c_loc(cks), c_loc(akq), c_loc(bkq), c_loc(ckq)]
    call check(c_turbulence_set_diagonals(self%handle, int(slot - 1, c_int), d), 'turbulence_set_diagonals')
  end subroutine fv3lm_hip_turbulence_set_diagonals

  !> The diagonals from BL_simp (turbulence/blsimp.F90) on the device, from the resident trajectory and traj%frocean(isc:iec, jsc:jec).
  subroutine fv3lm_hip_turbulence_set_simple(self, slot, frocean)
    type(fv3lm_hip_type), intent(in) :: self
    integer, intent(in) :: slot
    real(c_double), intent(in), target, contiguous :: frocean(:, :)
    call check(c_turbulence_set_simple(self%handle, int(slot - 1, c_int), c_loc(frocean)), 'turbulence_set_simple')
  end subroutine fv3lm_hip_turbulence_set_simple

  !> TURBPARAMS / TURBPARAMSI as documented at bldriver.F90:100-127 (the reference never assigns lcnst%TURBPARAMS: they are the host's);
  !! kpblmin = count(PREF < 50000.).
  subroutine fv3lm_hip_bl_default_params(p, kpblmin)
    type(fv3lm_bl_params), intent(out) :: p
    integer, intent(in) :: kpblmin
    call c_bl_default_params(p, int(kpblmin, c_int))
  end subroutine fv3lm_hip_bl_default_params

  !> In set_ltraj in place of compute_pressures, PTT1, the IceFraction split, BL_DRIVER and the three VTRILUPERT (:439-512): the
  !! diagonals from the trajectory resident on the device.  Call after fv3lm_hip_traj_to_fv3 and before the dynamics' step.
  !! qa, qb: traj%QI, traj%QL (cloud_mode 0, do_phy_mst == 0) or traj%QLS, traj%QCN (cloud_mode 1), (isc:iec, jsc:jec, npz).
  subroutine fv3lm_hip_turbulence_set_driver(self, slot, p, dt, frland, frocean, varflt, zpbl, cm, ct, cq, ustar, bstar, qa, qb, cloud_mode)
    type(fv3lm_hip_type), intent(in) :: self
    integer, intent(in) :: slot, cloud_mode
    type(fv3lm_bl_params), intent(in) :: p
    real(c_double), intent(in) :: dt
    real(c_double), intent(in), target, contiguous :: frland(:, :), frocean(:, :), varflt(:, :), zpbl(:, :), cm(:, :), ct(:, :), cq(:, :)
    real(c_double), intent(in), target, contiguous :: ustar(:, :), bstar(:, :), qa(:, :, :), qb(:, :, :)
    type(c_ptr) :: s(9)
    s = [c_loc(frland), c_loc(frocean), c_loc(varflt), c_loc(zpbl), c_loc(cm), c_loc(ct), c_loc(cq), c_loc(ustar), c_loc(bstar)]
    call check(c_turbulence_set_driver(self%handle, int(slot - 1, c_int), p, dt, s, c_loc(qa), c_loc(qb), int(cloud_mode, c_int), c_null_ptr), &
               'turbulence_set_driver')
  end subroutine fv3lm_hip_turbulence_set_driver

  !> mode 0: step_nl (:151-214) on the trajectory; 1: step_tl (:218-282) after fv3lm_hip_step_tl; 2: step_ad (:286-350) before
  !! fv3lm_hip_step_ad.  In place of the seven VTRISOLVEPERT calls and the T <-> theta conversions around them.
  subroutine fv3lm_hip_turbulence(self, slot, mode)
    type(fv3lm_hip_type), intent(in) :: self
    integer, intent(in) :: slot, mode
    call check(c_turbulence(self%handle, int(slot - 1, c_int), int(mode, c_int)), 'turbulence')
  end subroutine fv3lm_hip_turbulence

  !> fac(:, :, :, 1:9) the LU factors in the order of set_diagonals, fac(:, :, :, 10) pk (diagnostics)
  subroutine fv3lm_hip_turbulence_get(self, slot, fac)
    type(fv3lm_hip_type), intent(in) :: self
    integer, intent(in) :: slot
    real(c_double), intent(inout), target, contiguous :: fac(:, :, :, :)
    type(c_ptr) :: d(10)
    integer :: n
    do n = 1, 10
      d(n) = c_loc(fac(1, 1, 1, n))
    end do
    call check(c_turbulence_get(self%handle, int(slot - 1, c_int), d), 'turbulence_get')
  end subroutine fv3lm_hip_turbulence_get

  !> Linearised RAS convection (physics/moist: RASE, RASE_D, RASE_B and the convective part of set_ltraj).  Slots are numbered from 1,
  !! like ltraj(conf%n); arrays are the host's own, (isc:iec, jsc:jec[, npz]).  RASPARAMS as create :120-148 sets them (im = conf%im).
  subroutine fv3lm_hip_ras_default_params(p, im)
    type(fv3lm_ras_params), intent(out) :: p
    integer, intent(in) :: im
    call c_ras_default_params(p, int(im, c_int))
  end subroutine fv3lm_hip_ras_default_params

  subroutine fv3lm_hip_convection_create(self, nslots, p, do_phy_mst)
    type(fv3lm_hip_type), intent(in) :: self
    integer, intent(in) :: nslots, do_phy_mst
    type(fv3lm_ras_params), intent(in) :: p
    call check(c_convection_create(self%handle, int(nslots, c_int), p, int(do_phy_mst, c_int)), 'convection_create')
  end subroutine fv3lm_hip_convection_create

  !> In place of the convective part of set_ltraj (:700-832): call after fv3lm_hip_traj_to_fv3 and before the dynamics' step.
  subroutine fv3lm_hip_convection_set(self, slot, ts, frland, kcbl)
    type(fv3lm_hip_type), intent(in) :: self
    integer, intent(in) :: slot
    real(c_double), intent(in), target, contiguous :: ts(:, :), frland(:, :), kcbl(:, :)
    call check(c_convection_set(self%handle, int(slot - 1, c_int), c_loc(ts), c_loc(frland), c_loc(kcbl)), 'convection_set')
  end subroutine fv3lm_hip_convection_set

  !> out(:, :, :, 1:6) = PTT_C QVT_C CNV_DQLDT_C CNV_MFD_C CNV_PRC3_C CNV_UPDF_C (what the cloud scheme reads), doconvec
  subroutine fv3lm_hip_convection_get(self, slot, out, doconvec)
    type(fv3lm_hip_type), intent(in) :: self
    integer, intent(in) :: slot
    real(c_double), intent(inout), target, contiguous :: out(:, :, :, :)
    integer(c_int), intent(inout), target, contiguous :: doconvec(:, :)
    type(c_ptr) :: d(6)
    integer :: n
    do n = 1, 6
      d(n) = c_loc(out(1, 1, 1, n))
    end do
    call check(c_convection_get(self%handle, int(slot - 1, c_int), d, c_loc(doconvec), c_null_ptr), 'convection_get')
  end subroutine fv3lm_hip_convection_get

  !> src(:, :, :, 1:4) = CNV_DQLDT CNV_MFD CNV_PRC3 CNV_UPDF of the perturbation: read after a tangent run ...
  subroutine fv3lm_hip_convection_get_sources(self, src)
    type(fv3lm_hip_type), intent(in) :: self
    real(c_double), intent(inout), target, contiguous :: src(:, :, :, :)
    type(c_ptr) :: d(4)
    integer :: n
    do n = 1, 4
      d(n) = c_loc(src(1, 1, 1, n))
    end do
    call check(c_convection_sources(self%handle, 0_c_int, d), 'convection_sources (get)')
  end subroutine fv3lm_hip_convection_get_sources

  !> ... and given before an adjoint run (the adjoints the cloud scheme's adjoint left in them)
  subroutine fv3lm_hip_convection_put_sources(self, src)
    type(fv3lm_hip_type), intent(in) :: self
    real(c_double), intent(in), target, contiguous :: src(:, :, :, :)
    type(c_ptr) :: d(4)
    integer :: n
    do n = 1, 4
      d(n) = c_loc(src(1, 1, 1, n))
    end do
    call check(c_convection_sources(self%handle, 1_c_int, d), 'convection_sources (put)')
  end subroutine fv3lm_hip_convection_put_sources

  !> diagnostics: the saturation table on the device (18301 entries) and the kernels' nine constants (CP ALHL GRAV RGAS H2OMW AIRMW VIREPS P00 KAPPA)
  subroutine fv3lm_hip_convection_table(self, table, constants)
    type(fv3lm_hip_type), intent(in) :: self
    real(c_double), intent(inout), target, contiguous :: table(:), constants(:)
    call check(c_convection_table(self%handle, c_loc(table), c_loc(constants)), 'convection_table')
  end subroutine fv3lm_hip_convection_table

  !> mode 0 step_nl, 1 step_tl (after the turbulence), 2 step_ad (before the turbulence's adjoint) of the moist physics, convection only
  subroutine fv3lm_hip_convection(self, slot, mode)
    type(fv3lm_hip_type), intent(in) :: self
    integer, intent(in) :: slot, mode
    call check(c_convection(self%handle, int(slot - 1, c_int), int(mode, c_int)), 'convection')
  end subroutine fv3lm_hip_convection

  !> Linearised cloud scheme (physics/moist: CLOUD_DRIVER, CLOUD_DRIVER_D, CLOUD_DRIVER_B and the cloud part of set_ltraj :834-874).
  !! Slots are those of the convection, numbered from 1; arrays are the host's own, (isc:iec, jsc:jec[, npz]).  CLOUDPARAMS as create
  !! :151-211 sets them (im = conf%im).  iqi, iql: the tracers (2..nq) that carry cloud ice and cloud liquid on the device.
  subroutine fv3lm_hip_cloud_default_params(p, im)
    type(fv3lm_cloud_params), intent(out) :: p
    integer, intent(in) :: im
    call c_cloud_default_params(p, int(im, c_int))
  end subroutine fv3lm_hip_cloud_default_params

  subroutine fv3lm_hip_cloud_create(self, p, iqi, iql)
    type(fv3lm_hip_type), intent(in) :: self
    type(fv3lm_cloud_params), intent(in) :: p
    integer, intent(in) :: iqi, iql
    call check(c_cloud_create(self%handle, p, int(iqi, c_int), int(iql, c_int)), 'cloud_create')
  end subroutine fv3lm_hip_cloud_create

  !> In place of the cloud part of set_ltraj (:834-874): call after fv3lm_hip_convection_set of the same slot.
  subroutine fv3lm_hip_cloud_set(self, slot, qls, qcn, cfcn, khl, khu)
    type(fv3lm_hip_type), intent(in) :: self
    integer, intent(in) :: slot
    real(c_double), intent(in), target, contiguous :: qls(:, :, :), qcn(:, :, :), cfcn(:, :, :), khl(:, :), khu(:, :)
    call check(c_cloud_set(self%handle, int(slot - 1, c_int), c_loc(qls), c_loc(qcn), c_loc(cfcn), c_loc(khl), c_loc(khu)), 'cloud_set')
  end subroutine fv3lm_hip_cloud_set

  !> out(:, :, :, 1:8) = theta q QI_ls QL_ls QI_con QL_con CF_ls CF_con after CLOUD_DRIVER in values, frac(:, :, :, 1:4) = ILSF ICNF LLSF
  !! LCNF, pertmod = the switch cloud_pertmod of every cell
  subroutine fv3lm_hip_cloud_get(self, slot, out, frac, pertmod)
    type(fv3lm_hip_type), intent(in) :: self
    integer, intent(in) :: slot
    real(c_double), intent(inout), target, contiguous :: out(:, :, :, :), frac(:, :, :, :)
    integer(c_int), intent(inout), target, contiguous :: pertmod(:, :, :)
    type(c_ptr) :: d(8), f(4)
    integer :: n
    do n = 1, 8
      d(n) = c_loc(out(1, 1, 1, n))
    end do
    do n = 1, 4
      f(n) = c_loc(frac(1, 1, 1, n))
    end do
    call check(c_cloud_get(self%handle, int(slot - 1, c_int), d, f, c_loc(pertmod)), 'cloud_get')
  end subroutine fv3lm_hip_cloud_get

  !> the perturbation's convective cloud fraction, which lives on the device: read after a run ...
  subroutine fv3lm_hip_cloud_get_cfcn(self, cfcn)
    type(fv3lm_hip_type), intent(in) :: self
    real(c_double), intent(inout), target, contiguous :: cfcn(:, :, :)
    call check(c_cloud_cfcn(self%handle, 0_c_int, c_loc(cfcn)), 'cloud_cfcn (get)')
  end subroutine fv3lm_hip_cloud_get_cfcn

  !> ... and given before one
  subroutine fv3lm_hip_cloud_put_cfcn(self, cfcn)
    type(fv3lm_hip_type), intent(in) :: self
    real(c_double), intent(in), target, contiguous :: cfcn(:, :, :)
    call check(c_cloud_cfcn(self%handle, 1_c_int, c_loc(cfcn)), 'cloud_cfcn (put)')
  end subroutine fv3lm_hip_cloud_put_cfcn

  !> mode 0 step_nl, 1 step_tl (after fv3lm_hip_convection(1)), 2 step_ad (before fv3lm_hip_convection(2)) of the moist physics, cloud scheme
  subroutine fv3lm_hip_cloud(self, slot, mode)
    type(fv3lm_hip_type), intent(in) :: self
    integer, intent(in) :: slot, mode
    call check(c_cloud(self%handle, int(slot - 1, c_int), int(mode, c_int)), 'cloud')
  end subroutine fv3lm_hip_cloud

  !> Replaces compute_fv3_pressures_tlm + fv_dynamics_tlm (fv3jedi_lm_dynamics_mod.F90:404-438).
  subroutine fv3lm_hip_step_tl(self)
    type(fv3lm_hip_type), intent(in) :: self
    call check(c_step_tl(self%handle), 'step_tl')
  end subroutine fv3lm_hip_step_tl

  !> Replaces fv_dynamics_fwd + fv_dynamics_bwd + compute_fv3_pressures_bwd (:507-638).
  subroutine fv3lm_hip_step_ad(self)
    type(fv3lm_hip_type), intent(in) :: self
    call check(c_step_nl(self%handle), 'step_ad (forward sweep)')
    call check(c_step_ad(self%handle), 'step_ad (backward sweep)')
  end subroutine fv3lm_hip_step_ad

end module fv3lm_hip_mod
