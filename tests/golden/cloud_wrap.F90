! bind(C) wrapper around the reference's cloud scheme (physics/moist/cloud.F90, cloud_tl.F90, cloud_ad.F90 with qsat_util.F90 and
! utils/MAPL_Constants.F90) and RASE0 of convection.F90, used by make_cloud_golden.py only.  Arrays are (lm, ncol) / (lm + 1, ncol); the
! routines are called one column at a time with im = jm = 1.  The reference's only outside symbol is LAPACK's DGEEV: this file supplies
! it, forwarding the matrix to a callback of the generator (numpy.linalg.eigvals) that returns the real parts in WR.
module cloud_wrap
  use iso_c_binding
  use MAPL_ConstantsMod
  use qsat_util, only: ESINIT
  use CLOUD, only: CLOUD_DRIVER
  use CLOUD_TL, only: CLOUD_DRIVER_D
  use CLOUD_AD, only: CLOUD_DRIVER_B
  implicit none
  integer, parameter :: TABLESIZE = 183 * 100 + 1
  real(8), save :: ESTBLX(TABLESIZE)
  logical, save :: have_table = .false.
  abstract interface
    subroutine eig_cb(a, wr) bind(C)
      import c_double
      real(c_double), intent(in) :: a(8, 8)
      real(c_double), intent(out) :: wr(8)
    end subroutine eig_cb
  end interface
  procedure(eig_cb), pointer, save :: eig => null()
contains

  subroutine table()
    if (.not. have_table) call ESINIT(ESTBLX)
    have_table = .true.
  end subroutine table

  subroutine cloud_set_eig(f) bind(C, name="cloud_set_eig")
    type(c_funptr), value :: f
    call c_f_procpointer(f, eig)
  end subroutine cloud_set_eig

  subroutine cloud_constants(c) bind(C, name="cloud_constants")
    real(c_double), intent(out) :: c(15)
    c(1) = dble(MAPL_RUNIV); c(2) = dble(MAPL_KAPPA); c(3) = dble(MAPL_AIRMW); c(4) = dble(MAPL_H2OMW); c(5) = dble(MAPL_GRAV)
    c(6) = dble(MAPL_ALHL); c(7) = dble(MAPL_ALHF); c(8) = dble(MAPL_PI); c(9) = dble(MAPL_RGAS); c(10) = dble(MAPL_CP)
    c(11) = dble(MAPL_VIREPS); c(12) = dble(MAPL_ALHS); c(13) = dble(MAPL_TICE); c(14) = dble(MAPL_RVAP); c(15) = dble(MAPL_P00)
  end subroutine cloud_constants

  ! which: 0 CLOUD_DRIVER, 1 CLOUD_DRIVER_D, 2 CLOUD_DRIVER_B.  x(lm, ncol, 8): th q qi_ls ql_ls qi_con ql_con cf_ls cf_con (in-out);
  ! xd: their perturbations / adjoints (in-out); s(lm, ncol, 4): cnv_dqldt cnv_mfd cnv_prc3 cnv_updf (in); sd: perturbations (in) /
  ! adjoints (in-out)
  subroutine cloud_run(which, ncol, lm, dt, x, xd, ple, s, sd, frland, khu, khl, params, mst) bind(C, name="cloud_run")
    integer(c_int), value :: which, ncol, lm, mst
    real(c_double), value :: dt
    real(c_double), intent(inout) :: x(lm, ncol, 8), xd(lm, ncol, 8), s(lm, ncol, 4), sd(lm, ncol, 4)
    real(c_double), intent(in) :: ple(lm + 1, ncol), frland(ncol), params(57)
    integer(c_int), intent(in) :: khu(ncol), khl(ncol)
    real(8) :: a(1, 1, lm, 8), ad(1, 1, lm, 8), o(1, 1, lm, 4), od(1, 1, lm, 4), p(1, 1, 0:lm), fr(1, 1)
    integer :: n, m, ku(1, 1), kl(1, 1)
    real(8) :: c(15)
    call table()
    call cloud_constants(c)
    do n = 1, ncol
      do m = 1, 8
        a(1, 1, :, m) = x(:, n, m); ad(1, 1, :, m) = xd(:, n, m)
      end do
      do m = 1, 4
        o(1, 1, :, m) = s(:, n, m); od(1, 1, :, m) = sd(:, n, m)
      end do
      p(1, 1, :) = ple(:, n); fr = frland(n); ku = khu(n); kl = khl(n)
      if (which == 0) then
        call CLOUD_DRIVER(dt, 1, 1, lm, a(:, :, :, 1), a(:, :, :, 2), p, o(:, :, :, 1), o(:, :, :, 2), o(:, :, :, 3), o(:, :, :, 4), &
                          a(:, :, :, 3), a(:, :, :, 4), a(:, :, :, 5), a(:, :, :, 6), a(:, :, :, 7), a(:, :, :, 8), fr, params, ESTBLX, ku, kl, &
                          c(1), c(2), c(3), c(4), c(5), c(6), c(7), c(8), c(9), c(10), c(11), c(12), c(13), c(14), c(15), mst)
      else if (which == 1) then
        call CLOUD_DRIVER_D(dt, 1, 1, lm, a(:, :, :, 1), ad(:, :, :, 1), a(:, :, :, 2), ad(:, :, :, 2), p, o(:, :, :, 1), od(:, :, :, 1), &
                            o(:, :, :, 2), od(:, :, :, 2), o(:, :, :, 3), od(:, :, :, 3), o(:, :, :, 4), od(:, :, :, 4), &
                            a(:, :, :, 3), ad(:, :, :, 3), a(:, :, :, 4), ad(:, :, :, 4), a(:, :, :, 5), ad(:, :, :, 5), a(:, :, :, 6), ad(:, :, :, 6), &
                            a(:, :, :, 7), ad(:, :, :, 7), a(:, :, :, 8), ad(:, :, :, 8), fr, params, ESTBLX, ku, kl, &
                            c(1), c(2), c(3), c(4), c(5), c(6), c(7), c(8), c(9), c(10), c(11), c(12), c(13), c(14), c(15), mst)
      else
        call CLOUD_DRIVER_B(dt, 1, 1, lm, a(:, :, :, 1), ad(:, :, :, 1), a(:, :, :, 2), ad(:, :, :, 2), p, o(:, :, :, 1), od(:, :, :, 1), &
                            o(:, :, :, 2), od(:, :, :, 2), o(:, :, :, 3), od(:, :, :, 3), o(:, :, :, 4), od(:, :, :, 4), &
                            a(:, :, :, 3), ad(:, :, :, 3), a(:, :, :, 4), ad(:, :, :, 4), a(:, :, :, 5), ad(:, :, :, 5), a(:, :, :, 6), ad(:, :, :, 6), &
                            a(:, :, :, 7), ad(:, :, :, 7), a(:, :, :, 8), ad(:, :, :, 8), fr, params, ESTBLX, ku, kl, &
                            c(1), c(2), c(3), c(4), c(5), c(6), c(7), c(8), c(9), c(10), c(11), c(12), c(13), c(14), c(15), mst)
      end if
      do m = 1, 8
        x(:, n, m) = a(1, 1, :, m); xd(:, n, m) = ad(1, 1, :, m)
      end do
      do m = 1, 4
        sd(:, n, m) = od(1, 1, :, m)
      end do
    end do
  end subroutine cloud_run
end module cloud_wrap

! LAPACK's DGEEV as the reference calls it: the workspace query returns a size, the second call the real parts of the eigenvalues
subroutine dgeev(jobvl, jobvr, n, a, lda, wr, wi, vl, ldvl, vr, ldvr, work, lwork, info)
  use cloud_wrap, only: eig
  implicit none
  character(len=*) :: jobvl, jobvr
  integer :: n, lda, ldvl, ldvr, lwork, info
  real(8) :: a(lda, *), wr(*), wi(*), vl(ldvl, *), vr(ldvr, *), work(*)
  real(8) :: m(8, 8), w(8)
  info = 0
  if (lwork == -1) then
    work(1) = 64.0_8
    return
  end if
  m = a(1:8, 1:8)
  call eig(m, w)
  wr(1:8) = w; wi(1:8) = 0.0_8
end subroutine dgeev
