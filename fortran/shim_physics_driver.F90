!> shim_physics_driver — the second Fortran host in miniature: drives every physics and Rayleigh wrapper of fv3lm_hip_mod (the public
!! list from fv3lm_hip_set_rayleigh to fv3lm_hip_cloud) the way the edited physics modules of the host would, on slots numbered from 1.
!! Inputs and outputs travel through two stream files so that tests/physics_shim_checks.py can hold every array against the same calls
!! made through ctypes (bit for bit): that checks the value attributes, the order of the arguments, slot - 1, the order of the c_ptr
!! arrays (nine diagonals, nine surface fields, out(:,:,:,1:6), src(:,:,:,1:4), out8 / frac4), the three bind(C) parameter types and
!! the integer arrays.  One leg a run: 1 moist (convection + cloud), 2 boundary layer, 3 Rayleigh damping.  With bad = 1 a leg makes a
!! call the library refuses, and the program ends like the host would: FATAL, the library's message, exit status 1.
!! usage: shim_physics_driver <input file> <output file>
program shim_physics_driver
  use iso_c_binding
  use fv3lm_hip_mod
  implicit none
  integer, parameter :: ng = 3
  character(len=512) :: fin, fout
  type(fv3lm_dims) :: dims
  type(fv3lm_options) :: opt
  type(fv3lm_hip_type) :: dyn
  integer(c_int8_t), allocatable :: raw(:)
  integer(c_int) :: leg, bad, nraw
  integer :: nx, ny, npz, nq, nf, n, m, isd, ied, jsd, jed
  real(c_double) :: da_min, da_min_c
  real(c_double), allocatable, target :: metrics(:, :, :)
  type(c_ptr) :: mptr(50)
  real(c_double), allocatable :: phis(:, :), ak(:), bk(:)
  ! the padded planes (isd:ied+1, jsd:jed+1) of u v pt delp q1..: trajectory, perturbation, adjoint forcing
  real(c_double), allocatable :: T(:, :, :, :), P(:, :, :, :), PA(:, :, :, :)
  character(len=8), allocatable :: fname(:)

  call get_command_argument(1, fin); call get_command_argument(2, fout)
  open(11, file=trim(fin), access='stream', form='unformatted', status='old')
  read(11) leg, bad
  read(11) nraw; allocate(raw(nraw)); read(11) raw; dims = transfer(raw, dims); deallocate(raw)
  read(11) nraw; allocate(raw(nraw)); read(11) raw; opt = transfer(raw, opt); deallocate(raw)
  nx = dims%nx; ny = dims%ny; npz = dims%npz; nq = dims%nq; nf = 4 + nq
  isd = 1 - ng; ied = nx + ng; jsd = 1 - ng; jed = ny + ng
  allocate(metrics(isd:ied+1, jsd:jed+1, 50), phis(isd:ied+1, jsd:jed+1), ak(npz+1), bk(npz+1))
  read(11) da_min, da_min_c; read(11) metrics; read(11) phis; read(11) ak; read(11) bk
  allocate(T(isd:ied+1, jsd:jed+1, npz, nf), P(isd:ied+1, jsd:jed+1, npz, nf), PA(isd:ied+1, jsd:jed+1, npz, nf), fname(nf))
  read(11) T, P, PA
  fname(1) = 'u'; fname(2) = 'v'; fname(3) = 'pt'; fname(4) = 'delp'
  do n = 1, nq
    write(fname(4 + n), '(a,i0)') 'q', n
  end do
  do m = 1, 50
    mptr(m) = c_loc(metrics(isd, jsd, m))
  end do
  call fv3lm_hip_create(dyn, dims, opt, mptr, da_min, da_min_c, phis, ak, bk)
  open(12, file=trim(fout), access='stream', form='unformatted', status='replace')
  select case (leg)
  case (1)
    call moist_leg()
  case (2)
    call boundary_layer_leg()
  case (3)
    call rayleigh_leg()
  case default
    write(*, '(a)') 'shim_physics_driver: unknown leg'
    call exit(2)
  end select
  close(11); close(12)
  call fv3lm_hip_destroy(dyn)
  write(*, '(a)') 'shim_physics_driver OK'
contains
  subroutine put_all(which, A)
    integer, intent(in) :: which
    real(c_double), intent(in) :: A(isd:, jsd:, :, :)
    integer :: i
    do i = 1, nf
      call fv3lm_hip_put(dyn, trim(fname(i)), which, A(:, :, :, i), isd, jsd)
    end do
  end subroutine put_all

  subroutine get_all(which)
    integer, intent(in) :: which
    real(c_double), allocatable :: g(:, :, :)
    integer :: i
    allocate(g(isd:ied+1, jsd:jed+1, npz))
    do i = 1, nf
      call fv3lm_hip_get(dyn, trim(fname(i)), which, g, isd, jsd); write(12) g
    end do
  end subroutine get_all

  !> convection and cloud scheme on slot 2 of 2: set, the three gets, the tangent chain, the adjoint chain, both nonlinear runs
  subroutine moist_leg()
    type(fv3lm_ras_params) :: rp
    type(fv3lm_cloud_params) :: cp
    integer(c_int) :: mst, iqi, iql
    integer, parameter :: slot = 2
    real(c_double), allocatable :: ts(:, :), frland(:, :), kcbl(:, :), qls(:, :, :), qcn(:, :, :), cfcn(:, :, :), khl(:, :), khu(:, :)
    real(c_double), allocatable :: cf(:, :, :), cfa(:, :, :), out6(:, :, :, :), src(:, :, :, :), out8(:, :, :, :), frac4(:, :, :, :)
    real(c_double), allocatable :: table(:), constants(:)
    integer(c_int), allocatable :: doconvec(:, :), pertmod(:, :, :)
    allocate(ts(nx, ny), frland(nx, ny), kcbl(nx, ny), qls(nx, ny, npz), qcn(nx, ny, npz), cfcn(nx, ny, npz), khl(nx, ny), khu(nx, ny))
    allocate(cf(nx, ny, npz), cfa(nx, ny, npz), out6(nx, ny, npz, 6), src(nx, ny, npz, 4), out8(nx, ny, npz, 8), frac4(nx, ny, npz, 4))
    allocate(table(18301), constants(9), doconvec(nx, ny), pertmod(nx, ny, npz))
    read(11) mst, iqi, iql
    read(11) ts, frland, kcbl, qls, qcn, cfcn, khl, khu, cf, cfa
    call fv3lm_hip_ras_default_params(rp, 12); write(12) rp%r
    call fv3lm_hip_convection_create(dyn, 2, rp, int(mst))
    call fv3lm_hip_cloud_default_params(cp, 12); write(12) cp%r
    call fv3lm_hip_cloud_create(dyn, cp, int(iqi), int(iql))
    call put_all(0, T)
    if (bad == 1) call fv3lm_hip_convection(dyn, 1, 1)     ! slot 1 was never set: the library refuses, the host ends
    call fv3lm_hip_convection_set(dyn, slot, ts, frland, kcbl)
    call fv3lm_hip_cloud_set(dyn, slot, qls, qcn, cfcn, khl, khu)
    doconvec = -7; pertmod = -7
    call fv3lm_hip_convection_get(dyn, slot, out6, doconvec); write(12) out6, doconvec
    call fv3lm_hip_convection_table(dyn, table, constants); write(12) table, constants
    call fv3lm_hip_cloud_get(dyn, slot, out8, frac4, pertmod); write(12) out8, frac4, pertmod
    ! ---- tangent: convection, its sources read, the cloud scheme with the perturbation's cfcn given and read back
    call put_all(1, P)
    call fv3lm_hip_convection(dyn, slot, 1)
    call fv3lm_hip_convection_get_sources(dyn, src); write(12) src
    call fv3lm_hip_cloud_put_cfcn(dyn, cf)
    call fv3lm_hip_cloud(dyn, slot, 1)
    call fv3lm_hip_cloud_get_cfcn(dyn, cf); write(12) cf
    call get_all(1)
    ! ---- adjoint: the cloud scheme, the source adjoints it leaves read, scaled each by its own factor and given back, convection
    call put_all(1, PA)
    call fv3lm_hip_cloud_put_cfcn(dyn, cfa)
    call fv3lm_hip_cloud(dyn, slot, 2)
    call fv3lm_hip_convection_get_sources(dyn, src); write(12) src
    do n = 1, 4
      src(:, :, :, n) = src(:, :, :, n) * real(n + 1, c_double)
    end do
    call fv3lm_hip_convection_put_sources(dyn, src)
    call fv3lm_hip_convection(dyn, slot, 2)
    call get_all(1)
    call fv3lm_hip_cloud_get_cfcn(dyn, cfa); write(12) cfa
    call fv3lm_hip_convection_get_sources(dyn, src); write(12) src
    ! ---- nonlinear: both write the trajectory
    call fv3lm_hip_convection(dyn, slot, 0)
    call get_all(0)
    call fv3lm_hip_cloud(dyn, slot, 0)
    call get_all(0)
  end subroutine moist_leg

  !> the turbulence: BL_DRIVER on slot 2 of 2, the three solves; slot 1 from diagonals, then from BL_simp
  subroutine boundary_layer_leg()
    type(fv3lm_bl_params) :: bp
    integer(c_int) :: kpblmin
    real(c_double) :: dt
    real(c_double), allocatable :: sfc(:, :, :), qa(:, :, :), qb(:, :, :), frocean(:, :), fac(:, :, :, :), fac1(:, :, :, :)
    integer :: mode
    allocate(sfc(nx, ny, 9), qa(nx, ny, npz), qb(nx, ny, npz), frocean(nx, ny), fac(nx, ny, npz, 10), fac1(nx, ny, npz, 10))
    read(11) kpblmin
    read(11) dt, sfc, qa, qb, frocean
    call fv3lm_hip_turbulence_create(dyn, 2)
    call fv3lm_hip_bl_default_params(bp, int(kpblmin)); write(12) bp%r, bp%i
    call put_all(0, T)
    if (bad == 1) call fv3lm_hip_turbulence(dyn, 1, 1)     ! slot 1 was never set
    call fv3lm_hip_turbulence_set_driver(dyn, 2, bp, dt, sfc(:, :, 1), sfc(:, :, 2), sfc(:, :, 3), sfc(:, :, 4), sfc(:, :, 5), sfc(:, :, 6), &
                                         sfc(:, :, 7), sfc(:, :, 8), sfc(:, :, 9), qa, qb, 0)
    call fv3lm_hip_turbulence_get(dyn, 2, fac); write(12) fac
    do mode = 0, 2
      call put_all(0, T); call put_all(1, P)
      call fv3lm_hip_turbulence(dyn, 2, mode)
      call get_all(min(mode, 1))
    end do
    ! ---- slot 1: the factors just read back taken as diagonals, each scaled by a factor of its own (heat and moisture share their
    ! diffusivity: unscaled, two of the nine arrays are equal and could change places unseen); pk from the resident trajectory
    call put_all(0, T); call put_all(1, P)
    do n = 1, 9
      fac(:, :, :, n) = fac(:, :, :, n) * (1.0_c_double + real(n, c_double) / 32.0_c_double)
    end do
    call fv3lm_hip_turbulence_set_diagonals(dyn, 1, fac(:, :, :, 1), fac(:, :, :, 2), fac(:, :, :, 3), fac(:, :, :, 4), fac(:, :, :, 5), &
                                            fac(:, :, :, 6), fac(:, :, :, 7), fac(:, :, :, 8), fac(:, :, :, 9))
    call fv3lm_hip_turbulence_get(dyn, 1, fac1); write(12) fac1
    call fv3lm_hip_turbulence(dyn, 1, 1)
    call get_all(1)
    call fv3lm_hip_turbulence_set_simple(dyn, 1, frocean)
    call fv3lm_hip_turbulence_get(dyn, 1, fac1); write(12) fac1
  end subroutine boundary_layer_leg

  !> Rayleigh damping switched on through the shim, its profile read back, a tangent and an adjoint step with it
  subroutine rayleigh_leg()
    real(c_double) :: tau, rf_cutoff
    real(c_double), allocatable :: c2l(:, :, :, :), rf(:)
    integer(c_int) :: kmax
    allocate(c2l(isd:ied+1, jsd:jed+1, 4, 1), rf(npz))
    read(11) tau, rf_cutoff, c2l
    if (bad == 1) tau = -1.0_c_double                      ! refused: tau < 0
    call fv3lm_hip_set_rayleigh(dyn, tau, rf_cutoff, c2l)
    kmax = -7
    call fv3lm_hip_rayleigh_profile(dyn, rf, kmax); write(12) rf, kmax
    call put_all(0, T); call put_all(1, P)
    call fv3lm_hip_step_tl(dyn)
    call get_all(0); call get_all(1)
    call put_all(0, T); call put_all(1, PA)
    call fv3lm_hip_step_ad(dyn)
    call get_all(1)
  end subroutine rayleigh_leg
end program shim_physics_driver
