!> fv3lm_hip_lm_mod — the composed model step behind fv3lm_lm_* (include/fv3lm.h): fv3jedi_lm_mod's step_tl / step_ad
!! (src/fv3jedi_lm_mod.F90:161-187) in one call, about the trajectory of a stored time.  A host that runs whole steps replaces the
!! per-part calls of fv3lm_hip_mod (step_tl / step_ad, turbulence, convection, cloud, put_cfcn / get_cfcn) by fv3lm_hip_lm_step; the
!! order of the parts and the ipert_to_zero rule (:242-253) are then the library's (INTEGRATION.md section 3d).
!! Slots are numbered from 1, like the physics slots of fv3lm_hip_mod, and carry the same number as those.
module fv3lm_hip_lm_mod
  use iso_c_binding
  use fv3lm_hip_mod
  implicit none
  private
  public :: fv3lm_hip_lm_create, fv3lm_hip_lm_traj_save, fv3lm_hip_lm_traj_load, fv3lm_hip_lm_step, fv3lm_hip_cloud_bind_cfcn

  interface
    function c_lm_create(h, nslots, do_dyn, do_phy_trb, do_phy_mst) bind(C, name="fv3lm_lm_create") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: nslots, do_dyn, do_phy_trb, do_phy_mst
      integer(c_int) :: rc
    end function c_lm_create
    function c_lm_traj_save(h, slot) bind(C, name="fv3lm_lm_traj_save") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: slot
      integer(c_int) :: rc
    end function c_lm_traj_save
    function c_lm_traj_load(h, slot) bind(C, name="fv3lm_lm_traj_load") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: slot
      integer(c_int) :: rc
    end function c_lm_traj_load
    function c_lm_step(h, slot, mode) bind(C, name="fv3lm_lm_step") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: slot, mode
      integer(c_int) :: rc
    end function c_lm_step
    function c_cloud_bind_cfcn(h, iqc) bind(C, name="fv3lm_cloud_bind_cfcn") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: h
      integer(c_int), value :: iqc
      integer(c_int) :: rc
    end function c_cloud_bind_cfcn
    function c_lm_last_error() bind(C, name="fv3lm_last_error") result(p)
      import :: c_ptr
      type(c_ptr) :: p
    end function c_lm_last_error
  end interface

contains

  !> a nonzero status ends the host with the library's message, as fv3lm_hip_mod does (src/fv3jedi_lm_mod.F90:93)
  subroutine check(rc, where)
    integer(c_int), intent(in) :: rc
    character(len=*), intent(in) :: where
    character(kind=c_char), pointer :: msg(:)
    integer :: n
    if (rc == 0) return
    call c_f_pointer(c_lm_last_error(), msg, [512])
    n = 1
    do while (n < 512 .and. msg(n) /= c_null_char)
      n = n + 1
    end do
    write(*, '(4a)') 'FATAL fv3lm_hip ', where, ': ', transfer(msg(1:n-1), repeat(' ', n-1))
    call exit(1)
  end subroutine check

  !> create, once: nslots = conf%nt with saveltraj, 1 without; do_dyn, do_phy_trb as conf% has them, do_phy_mst = merge(1, 0,
  !! conf%do_phy_mst /= 0) (its value 1 or 2 goes to fv3lm_hip_convection_create).  All slots in one allocation.
  subroutine fv3lm_hip_lm_create(self, nslots, do_dyn, do_phy_trb, do_phy_mst)
    type(fv3lm_hip_type), intent(inout) :: self
    integer, intent(in) :: nslots, do_dyn, do_phy_trb, do_phy_mst
    call check(c_lm_create(self%handle, int(nslots, c_int), int(do_dyn, c_int), int(do_phy_trb, c_int), int(do_phy_mst, c_int)), 'lm_create')
  end subroutine fv3lm_hip_lm_create

  !> set_ltraj of time n: after fv3lm_hip_traj_to_fv3 and the physics sets of slot n, the resident trajectory goes into slot n
  subroutine fv3lm_hip_lm_traj_save(self, slot)
    type(fv3lm_hip_type), intent(inout) :: self
    integer, intent(in) :: slot
    call check(c_lm_traj_save(self%handle, int(slot - 1, c_int)), 'lm_traj_save')
  end subroutine fv3lm_hip_lm_traj_save

  !> slot n back as the resident trajectory (as after fv3lm_hip_traj_to_fv3 of the same arrays); fv3lm_hip_lm_step does this itself
  subroutine fv3lm_hip_lm_traj_load(self, slot)
    type(fv3lm_hip_type), intent(inout) :: self
    integer, intent(in) :: slot
    call check(c_lm_traj_load(self%handle, int(slot - 1, c_int)), 'lm_traj_load')
  end subroutine fv3lm_hip_lm_traj_load

  !> mode 1: step_tl (:161-172), 2: step_ad (:176-187) of fv3jedi_lm_mod on the resident perturbation, about the trajectory of slot n
  subroutine fv3lm_hip_lm_step(self, slot, mode)
    type(fv3lm_hip_type), intent(inout) :: self
    integer, intent(in) :: slot, mode
    call check(c_lm_step(self%handle, int(slot - 1, c_int), int(mode, c_int)), 'lm_step')
  end subroutine fv3lm_hip_lm_step

  !> once, after fv3lm_hip_cloud_create and before the first fv3lm_hip_cloud_set: the convective cloud fraction is tracer iqc (1-based,
  !! the reference's q(:,:,:,5) with do_phy_mst /= 0, fv3jedi_lm_dynamics_mod.F90:159-163), trajectory and perturbation, and the dynamics
  !! of fv3lm_hip_lm_step carries it between ipert_to_zero and the cloud scheme as FV_DYNAMICS_TLM / _BWD do
  subroutine fv3lm_hip_cloud_bind_cfcn(self, iqc)
    type(fv3lm_hip_type), intent(inout) :: self
    integer, intent(in) :: iqc
    call check(c_cloud_bind_cfcn(self%handle, int(iqc, c_int)), 'cloud_bind_cfcn')
  end subroutine fv3lm_hip_cloud_bind_cfcn
end module fv3lm_hip_lm_mod
