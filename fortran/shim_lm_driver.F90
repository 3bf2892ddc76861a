!> shim_lm_driver — the third Fortran host in miniature: a window of trajectory times driven through the composed model step of
!! fv3lm_hip_lm_mod.  It reads a state file, creates the three physics features and the trajectory store, sets the slots of every time
!! while its trajectory is resident (fv3lm_hip_traj_to_fv3, the physics sets, fv3lm_hip_lm_traj_save), runs tangent steps forward and
!! adjoint steps backward over the times through fv3lm_hip_lm_step only, and writes the perturbation after either sweep.
!! tests/lm_checks.py holds every array against the same window driven through ctypes, bit for bit.  Slots are numbered from 1.
!! With bad = 1 the last time is never saved and the first step at it is refused: FATAL, the library's message, exit status 1.
!! usage: shim_lm_driver <input file> <output file>
program shim_lm_driver
  use iso_c_binding
  use fv3lm_hip_mod
  use fv3lm_hip_lm_mod
  implicit none
  integer, parameter :: ng = 3
  character(len=512) :: fin, fout
  type(fv3lm_dims) :: dims
  type(fv3lm_options) :: opt
  type(fv3lm_hip_type) :: dyn
  type(fv3lm_ras_params) :: rp
  type(fv3lm_cloud_params) :: cp
  integer(c_int8_t), allocatable :: raw(:)
  integer(c_int) :: bad, mst, iqi, iql, ntimes, nraw
  integer :: nx, ny, npz, nq, n, m, isd, ied, jsd, jed
  real(c_double) :: da_min, da_min_c
  real(c_double), allocatable, target :: metrics(:, :, :)
  type(c_ptr) :: mptr(50)
  real(c_double), allocatable :: phis(:, :), ak(:), bk(:)
  ! the host's own arrays (isc:iec, jsc:jec[, npz]), no halo
  real(c_double), allocatable :: u(:, :, :), v(:, :, :), t(:, :, :), delp(:, :, :), q(:, :, :, :), cphis(:, :)
  real(c_double), allocatable :: ts(:, :), frland(:, :), kcbl(:, :), qls(:, :, :), qcn(:, :, :), cfcn(:, :, :), khl(:, :), khu(:, :)
  real(c_double), allocatable :: diag(:, :, :, :)

  call get_command_argument(1, fin); call get_command_argument(2, fout)
  open(11, file=trim(fin), access='stream', form='unformatted', status='old')
  read(11) bad, mst, iqi, iql, ntimes
  read(11) nraw; allocate(raw(nraw)); read(11) raw; dims = transfer(raw, dims); deallocate(raw)
  read(11) nraw; allocate(raw(nraw)); read(11) raw; opt = transfer(raw, opt); deallocate(raw)
  nx = dims%nx; ny = dims%ny; npz = dims%npz; nq = dims%nq
  isd = 1 - ng; ied = nx + ng; jsd = 1 - ng; jed = ny + ng
  allocate(metrics(isd:ied+1, jsd:jed+1, 50), phis(isd:ied+1, jsd:jed+1), ak(npz+1), bk(npz+1))
  read(11) da_min, da_min_c; read(11) metrics; read(11) phis; read(11) ak; read(11) bk
  allocate(u(nx, ny, npz), v(nx, ny, npz), t(nx, ny, npz), delp(nx, ny, npz), q(nx, ny, npz, nq), cphis(nx, ny))
  allocate(ts(nx, ny), frland(nx, ny), kcbl(nx, ny), qls(nx, ny, npz), qcn(nx, ny, npz), cfcn(nx, ny, npz), khl(nx, ny), khu(nx, ny))
  allocate(diag(nx, ny, npz, 9))
  do m = 1, 50
    mptr(m) = c_loc(metrics(isd, jsd, m))
  end do
  call fv3lm_hip_create(dyn, dims, opt, mptr, da_min, da_min_c, phis, ak, bk)
  ! ---- create, once: the features and one slot of each per time; the flags are the reference's conf%do_dyn, do_phy_trb, do_phy_mst /= 0
  call fv3lm_hip_lm_create(dyn, int(ntimes), 1, 1, 1)
  call fv3lm_hip_ras_default_params(rp, 12)
  call fv3lm_hip_convection_create(dyn, int(ntimes), rp, int(mst))
  call fv3lm_hip_cloud_default_params(cp, 12)
  call fv3lm_hip_cloud_create(dyn, cp, int(iqi), int(iql))
  call fv3lm_hip_turbulence_create(dyn, int(ntimes))
  ! ---- set_ltraj of every time: the trajectory goes up once, the physics slots are set from it, the store keeps it
  do n = 1, ntimes
    read(11) u, v, t, delp, q, cphis, ts, frland, kcbl, qls, qcn, cfcn, khl, khu, diag
    call fv3lm_hip_traj_to_fv3(dyn, u, v, t, delp, q, cphis)
    call fv3lm_hip_convection_set(dyn, n, ts, frland, kcbl)
    call fv3lm_hip_cloud_set(dyn, n, qls, qcn, cfcn, khl, khu)
    call fv3lm_hip_turbulence_set_diagonals(dyn, n, diag(:, :, :, 1), diag(:, :, :, 2), diag(:, :, :, 3), diag(:, :, :, 4), diag(:, :, :, 5), &
                                            diag(:, :, :, 6), diag(:, :, :, 7), diag(:, :, :, 8), diag(:, :, :, 9))
    if (bad == 1 .and. n == ntimes) exit      ! the last time is never saved
    call fv3lm_hip_lm_traj_save(dyn, n)
  end do
  call fv3lm_hip_lm_traj_load(dyn, 1)         ! a slot back as the resident trajectory; the steps below do this themselves
  open(12, file=trim(fout), access='stream', form='unformatted', status='replace')
  ! ---- the tangent over the window, first time to last
  read(11) u, v, t, delp, q
  call fv3lm_hip_pert_to_fv3(dyn, u, v, t, delp, q)
  do n = 1, ntimes
    call fv3lm_hip_lm_step(dyn, n, 1)
  end do
  call fv3lm_hip_fv3_to_pert(dyn, u, v, t, delp, q)
  write(12) u, v, t, delp, q
  ! ---- the adjoint over the window, last time to first
  read(11) u, v, t, delp, q
  call fv3lm_hip_pert_to_fv3(dyn, u, v, t, delp, q)
  do n = ntimes, 1, -1
    call fv3lm_hip_lm_step(dyn, n, 2)
  end do
  call fv3lm_hip_fv3_to_pert(dyn, u, v, t, delp, q)
  write(12) u, v, t, delp, q
  close(11); close(12)
  call fv3lm_hip_destroy(dyn)
  write(*, '(a)') 'shim_lm_driver OK'
end program shim_lm_driver
