! bind(C) wrapper of the reference's BL_DRIVER (physics/turbulence/bldriver.F90), used by make_bl_driver_golden.py only.
! It calls BL_DRIVER and nothing else: one row of ncol columns (IM = ncol, JM = 1), pe(ncol, 1, 0:lm), every 3-D array (ncol, 1, lm),
! arguments in BL_DRIVER's own order.  ZPBL and CT are updated in place, as in the routine.
subroutine bl_driver_wrap(ncol, lm, dt, u, v, th, q, p, qit, qlt, frland, frocean, varflt, zpbl, cm, ct, cq, turbparams, turbparamsi, &
                          ustar, bstar, aks, bks, cks, akq, bkq, ckq, akv, bkv, ckv, ekv, fkv) bind(C, name="bl_driver_wrap")
  use iso_c_binding
  use bldriver, only: bl_driver
  implicit none
  integer(c_int), value :: ncol, lm
  real(c_double), value :: dt
  real(c_double), intent(in) :: u(ncol, 1, lm), v(ncol, 1, lm), th(ncol, 1, lm), q(ncol, 1, lm), qit(ncol, 1, lm), qlt(ncol, 1, lm)
  real(c_double), intent(in) :: p(ncol, 1, 0:lm)
  real(c_double), intent(in) :: frland(ncol, 1), frocean(ncol, 1), varflt(ncol, 1), cm(ncol, 1), cq(ncol, 1), ustar(ncol, 1), bstar(ncol, 1)
  real(c_double), intent(inout) :: zpbl(ncol, 1), ct(ncol, 1)
  real(c_double), intent(in) :: turbparams(22)
  integer(c_int), intent(in) :: turbparamsi(4)
  real(c_double), intent(out) :: aks(ncol, 1, lm), bks(ncol, 1, lm), cks(ncol, 1, lm), akq(ncol, 1, lm), bkq(ncol, 1, lm), ckq(ncol, 1, lm)
  real(c_double), intent(out) :: akv(ncol, 1, lm), bkv(ncol, 1, lm), ckv(ncol, 1, lm), ekv(ncol, 1, lm), fkv(ncol, 1, lm)
  integer :: im, jm, l_m, ipar(4)
  im = ncol; jm = 1; l_m = lm; ipar = turbparamsi
  call bl_driver(im, jm, l_m, dt, u, v, th, q, p, qit, qlt, frland, frocean, varflt, zpbl, cm, ct, cq, turbparams, ipar, &
                 ustar, bstar, aks, bks, cks, akq, bkq, ckq, akv, bkv, ckv, ekv, fkv)
end subroutine bl_driver_wrap
