! bind(C) wrapper around the reference's RAS convection routines (physics/moist/convection.F90, convection_tl.F90, convection_ad.F90,
! qsat_util.F90 and utils/MAPL_Constants.F90), used by make_convection_golden.py only.  Arrays are (lm, ncol) / (lm + 1, ncol), one
! column a call as step_tl / step_ad / jacobian_filter_tlm make them; WGT0 = WGT1 = 1 on KCBL..LM and CO_AUTO = 2.5e-3 as set_ltraj.
module convection_wrap
  use iso_c_binding
  use MAPL_ConstantsMod
  use qsat_util, only: ESINIT
  use CONVECTION, only: RASE0
  use CONVECTION_TL, only: RASE_D, RASE0_D
  use CONVECTION_AD, only: RASE_B
  implicit none
  integer, parameter :: TABLESIZE = 183 * 100 + 1
  real(8), save :: ESTBLX(TABLESIZE)
  logical, save :: have_table = .false.
contains

  subroutine table()
    if (.not. have_table) call ESINIT(ESTBLX)
    have_table = .true.
  end subroutine table

  subroutine conv_constants(c, tbl) bind(C, name="conv_constants")
    real(c_double), intent(out) :: c(9), tbl(TABLESIZE)
    call table()
    c(1) = dble(MAPL_CP); c(2) = dble(MAPL_ALHL); c(3) = dble(MAPL_GRAV); c(4) = dble(MAPL_RGAS); c(5) = dble(MAPL_H2OMW)
    c(6) = dble(MAPL_AIRMW); c(7) = dble(MAPL_VIREPS); c(8) = dble(MAPL_P00); c(9) = dble(MAPL_KAPPA)
    tbl = ESTBLX
  end subroutine conv_constants

  subroutine weights(lm, k, w)
    integer, intent(in) :: lm, k
    real(8), intent(out) :: w(1, lm)
    w = 0.0_8
    w(1, k:lm) = 1.0_8
  end subroutine weights

  ! which: 0 RASE0 (tho qho in-out, four sources out), 1 RASE0_D (tho thod qho qhod in-out)
  subroutine conv_rase0(which, ncol, lm, icmin, dt, seedras, sige, kcbl, frland, ts, tho, thod, qho, qhod, ple, clw, flxd, prc3, updf, &
                        rasparams) bind(C, name="conv_rase0")
    integer(c_int), value :: which, ncol, lm, icmin
    real(c_double), value :: dt
    integer(c_int), intent(in) :: seedras(ncol), kcbl(ncol)
    real(c_double), intent(in) :: sige(lm + 1), frland(ncol), ts(ncol), ple(lm + 1, ncol), rasparams(25)
    real(c_double), intent(inout) :: tho(lm, ncol), thod(lm, ncol), qho(lm, ncol), qhod(lm, ncol)
    real(c_double), intent(inout) :: clw(lm, ncol), flxd(lm, ncol), prc3(lm, ncol), updf(lm, ncol)
    real(8) :: w(1, lm), a(1, lm), ad(1, lm), b(1, lm), bd(1, lm), p(1, lm + 1), o1(1, lm), o2(1, lm), o3(1, lm), o4(1, lm)
    real(8) :: co(1), fr(1), t1(1)
    integer :: n, sd(1), kc(1)
    call table()
    do n = 1, ncol
      call weights(lm, kcbl(n), w)
      a(1, :) = tho(:, n); ad(1, :) = thod(:, n); b(1, :) = qho(:, n); bd(1, :) = qhod(:, n); p(1, :) = ple(:, n)
      co = 2.5e-3_8; fr = frland(n); t1 = ts(n); sd = seedras(n); kc = kcbl(n)
      if (which == 0) then
        call RASE0(1, 1, lm, icmin, dt, dble(MAPL_CP), dble(MAPL_ALHL), dble(MAPL_GRAV), dble(MAPL_RGAS), dble(MAPL_H2OMW), &
                   dble(MAPL_AIRMW), dble(MAPL_VIREPS), sd, sige, kc, w, w, fr, t1, a, b, co, p, o1, o2, o3, o4, rasparams, ESTBLX)
        clw(:, n) = o1(1, :); flxd(:, n) = o2(1, :); prc3(:, n) = o3(1, :); updf(:, n) = o4(1, :)
      else
        call RASE0_D(1, 1, lm, icmin, dt, dble(MAPL_CP), dble(MAPL_ALHL), dble(MAPL_GRAV), dble(MAPL_RGAS), dble(MAPL_H2OMW), &
                     dble(MAPL_AIRMW), dble(MAPL_VIREPS), sd, sige, kc, w, w, fr, t1, a, ad, b, bd, co, p, rasparams, ESTBLX)
      end if
      tho(:, n) = a(1, :); thod(:, n) = ad(1, :); qho(:, n) = b(1, :); qhod(:, n) = bd(1, :)
    end do
  end subroutine conv_rase0

  ! which: 1 RASE_D, 2 RASE_B.  x(lm, ncol, 4): tho qho uho vho (in-out); xd: their perturbations / adjoints (in-out);
  ! s(lm, ncol, 4): clw flxd cnv_prc3 cnv_updfrc (out); sd: their perturbations (out) / adjoints (in)
  subroutine conv_rase(which, ncol, lm, icmin, dt, seedras, sige, kcbl, frland, ts, x, xd, ple, s, sd, rasparams) bind(C, name="conv_rase")
    integer(c_int), value :: which, ncol, lm, icmin
    real(c_double), value :: dt
    integer(c_int), intent(in) :: seedras(ncol), kcbl(ncol)
    real(c_double), intent(in) :: sige(lm + 1), frland(ncol), ts(ncol), ple(lm + 1, ncol), rasparams(25)
    real(c_double), intent(inout) :: x(lm, ncol, 4), xd(lm, ncol, 4), s(lm, ncol, 4), sd(lm, ncol, 4)
    real(8) :: w(1, lm), a(1, lm, 4), ad(1, lm, 4), p(1, lm + 1), o(1, lm, 4), od(1, lm, 4)
    real(8) :: co(1), fr(1), t1(1)
    integer :: n, m, se(1), kc(1)
    call table()
    do n = 1, ncol
      call weights(lm, kcbl(n), w)
      do m = 1, 4
        a(1, :, m) = x(:, n, m); ad(1, :, m) = xd(:, n, m); o(1, :, m) = 0.0_8; od(1, :, m) = sd(:, n, m)
      end do
      p(1, :) = ple(:, n)
      co = 2.5e-3_8; fr = frland(n); t1 = ts(n); se = seedras(n); kc = kcbl(n)
      if (which == 1) then
        od = 0.0_8
        call RASE_D(1, 1, lm, icmin, dt, dble(MAPL_CP), dble(MAPL_ALHL), dble(MAPL_GRAV), dble(MAPL_RGAS), dble(MAPL_H2OMW), &
                    dble(MAPL_AIRMW), dble(MAPL_VIREPS), se, sige, kc, w, w, fr, t1, a(:, :, 1), ad(:, :, 1), a(:, :, 2), ad(:, :, 2), &
                    a(:, :, 3), ad(:, :, 3), a(:, :, 4), ad(:, :, 4), co, p, o(:, :, 1), od(:, :, 1), o(:, :, 2), od(:, :, 2), &
                    o(:, :, 3), od(:, :, 3), o(:, :, 4), od(:, :, 4), rasparams, ESTBLX)
      else
        call RASE_B(1, 1, lm, icmin, dt, dble(MAPL_CP), dble(MAPL_ALHL), dble(MAPL_GRAV), dble(MAPL_RGAS), dble(MAPL_H2OMW), &
                    dble(MAPL_AIRMW), dble(MAPL_VIREPS), se, sige, kc, w, w, fr, t1, a(:, :, 1), ad(:, :, 1), a(:, :, 2), ad(:, :, 2), &
                    a(:, :, 3), ad(:, :, 3), a(:, :, 4), ad(:, :, 4), co, p, o(:, :, 1), od(:, :, 1), o(:, :, 2), od(:, :, 2), &
                    o(:, :, 3), od(:, :, 3), o(:, :, 4), od(:, :, 4), rasparams, ESTBLX)
      end if
      do m = 1, 4
        x(:, n, m) = a(1, :, m); xd(:, n, m) = ad(1, :, m); s(:, n, m) = o(1, :, m); sd(:, n, m) = od(1, :, m)
      end do
    end do
  end subroutine conv_rase
end module convection_wrap
