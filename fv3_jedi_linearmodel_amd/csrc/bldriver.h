// fv3lm-hip: BL_DRIVER (physics/turbulence/bldriver.F90, Louis + Lock) on the resident trajectory -- the routine that makes the nine
// diagonals set_ltraj (fv3jedi_lm_turbulence_mod.F90:482-512) hands to VTRILUPERT.  Values only: the diagonals are frozen on the
// trajectory, the reference has no tangent and no adjoint of it.  The chain BL_DRIVER :23-297 -> PRELIMINARY :300-369, LOUIS_DIFF
// :373-502, LOCK_DIFF :655-1090 (mpbl_depth :1094, diffusivity_pbl2 :1255, DQSAT_sub_sca :1466 on the table of ESINIT :1304),
// TRIDIAG_SETUP :504-609, ORODRAG :612-652 is column-local; so is what the caller does before it (set_ltraj :439-466): pe from ptop, pk,
// theta = p00^kappa T / pk, and with cloud_mode = 1 the split of QLS + QCN by IceFraction (utils/fv3jedi_lm_utils_mod.F90:295-319).
//
// Kept as the reference has them: QL_tot = QIT, QI_tot = QLT (:337-338); du = min(du, 1e-8) (:1141); CT = FROCEAN CT only where
// FROCEAN == 1 (:170); the running smooth of PV over the bottom six levels (:360-365, hence npz >= 7); the literal formulas in double in
// the routine's order of operations (no contraction into fused multiply-adds: the fixture is the reference's own double result).
// Not built, because dead with RADLW_DEP = 0 (RADLW is an uninitialised local read only under RADLW_DEP == 1, which is refused): the
// radiative / buoyancy-reversal block :894-1075, the kmax / kcldtop / kcldbot searches :854-892, dqs, density, radml_depth; vbulkshr
// (:790, never used) and the diagnostics ALH_X, KMLS_X, KHLS_X, DIFF_T / DIFF_M (LM+1).  LOCK_ON and PBLHT_OPTION are read and never
// tested by the reference: LOCK_DIFF always runs.  mpbl_depth leaves ipbl unset when its loop never exits and the reference then
// indexes with -1: here such a column raises the slot's second flag and the call is refused.
// The constants are those of fv3jedi_lm_const_mod, which the routine uses, evaluated as that module evaluates them; pk and theta -- the
// caller's part -- take akap and ptop of the handle like the rest of the slot.
//
// One thread per column, i fastest: every load and store of a level is one contiguous row piece per wave.  The work vectors of the
// column live in the slot's own planes until the last sweep overwrites them with the diagonals; no array per thread, no workspace:
//   plane 0 pe(l)   1 T = PIf TH   2 QIT   3 QLT   4 ZHALF(l)   5 PV   6 slv   7 RDZ   9 TH          (8 unused)
//   A  down  pe accumulated from ptop, TH, T; cloud_mode 1: the IceFraction split in place
//   B  up    ZHALF, ZFULL, TV, PV, slv, RDZ (TV and ZFULL of the level below are carried); then the smooth of PV
//   C  up    BSTAR > 0 only: the parcel of mpbl_depth (table lookup), the jump search, the entrainment scalars
//   D  down  per level the Louis diffusivities of the interface below, max with the plume's (pointwise in ZHALF, from the scalars of
//            C: k_t_troen is recomputed, not stored), the ZPBL criterion, TRIDIAG_SETUP, ORODRAG; level l's nine diagonals are stored
//            after everything level l of the planes held has been read (the values of level l are carried from the iteration before).
// PFULL, DMI, ZFULL are recomputed where used.  Byte model per point, 8 B words: algorithmic 7 fields read (u v T delp qv qa qb) + 9
// diagonals + pk written = 136 B; this form moves A 5 r + 3 w (+ 2 w cloud_mode 1), B 7 r + 4 w, C <= 6 r up to the parcel's top, D 6 r
// + 9 w (+ 2 w with raw_out), the factorisation that follows 9 r + 6 w + delp r + pk w: about 52 words = 416 B, plus the upload of qa, qb.
#pragma once
#include "turbulence.h"
#include "litcol.h"
#include <vector>

namespace fv3 {

namespace blc {      // utils/fv3jedi_lm_const_mod.F90
constexpr double GRAV = 9.80665, RUNIV = 8314.47, AIRMW = 28.965, H2OMW = 18.015, ALHL = 2.4665e6, ALHF = 3.3370e5, ALHS = ALHL + ALHF;
constexpr double RDRY = RUNIV / AIRMW, CPDRY = 3.5 * RDRY, KAPPA = RDRY / CPDRY, EPSILON = H2OMW / AIRMW, RGAS = RDRY, CP = RGAS / KAPPA;
constexpr double VIREPS = 1.0 / EPSILON - 1.0, P00 = 100000.0, TICE = 273.16, KARMAN = 0.40;
constexpr double TMINTBL = 150.0, TMAXTBL = 333.0;      // bldriver.F90:17-19
constexpr int DEGSUBS = 100, TABLESIZE = 183 * DEGSUBS + 1;
}  // namespace blc

constexpr int BL_NSFC = 9;      // FRLAND FROCEAN VARFLT ZPBL CM CT CQ USTAR BSTAR
enum { BL_FRLAND = 0, BL_FROCEAN, BL_VARFLT, BL_ZPBL, BL_CM, BL_CT, BL_CQ, BL_USTAR, BL_BSTAR };
enum { BLP_PE = 0, BLP_T = 1, BLP_QI = 2, BLP_QL = 3, BLP_ZH = 4, BLP_PV = 5, BLP_SLV = 6, BLP_RDZ = 7, BLP_TH = 9 };

struct BlParams { double r[22]; int i[4]; };      // TURBPARAMS, TURBPARAMSI (fv3lm_bl_params)

struct BlArgs {
  TurbArgs t;                   // geometry, trajectory, the slot, ptop, akap, p00k
  BlParams p;
  double dt;
  const double* tbl;            // ESTBLX
  double* sfc; size_t ss;       // surface field n at sfc + n ss, [ntile][plane]; ZPBL and CT are updated
  double* ekv; double* fkv;     // raw_out only: [ntile][npz][plane], else null
  int cloud_mode;
  int* flag;                    // raised where the parcel of mpbl_depth never stops
};

// ---- host: the table of ESINIT (:1304-1343) with QSATLQU0 (:1346-1389) and QSATICE0 (:1392-1464) --------------------------------------
inline double bl_qsatlqu0(double tl) {
  const double ZEROC = 273.16, TMINLQU = ZEROC - 40.0;
  const double B6 = 6.136820929E-11 * 100.0, B5 = 2.034080948E-8 * 100.0, B4 = 3.031240396E-6 * 100.0, B3 = 2.650648471E-4 * 100.0,
               B2 = 1.428945805E-2 * 100.0, B1 = 4.436518521E-1 * 100.0, B0 = 6.107799961E+0 * 100.0;
  const double ti = tl < TMINLQU ? TMINLQU : tl > blc::TMAXTBL ? blc::TMAXTBL : tl;
  const double tt = ti - ZEROC;
  return (tt * (tt * (tt * (tt * (tt * (tt * B6 + B5) + B4) + B3) + B2) + B1) + B0);
}
inline double bl_qsatice0(double tl) {
  const double ZEROC = 273.16, TMINICE = ZEROC + -95.0, TSTARR1 = -75.0, TSTARR2 = -65.0, TSTARR3 = -50.0, TSTARR4 = -40.0;
  const double BI6 = 1.838826904E-10 * 100.0, BI5 = 4.838803174E-8 * 100.0, BI4 = 5.824720280E-6 * 100.0, BI3 = 4.176223716E-4 * 100.0,
               BI2 = 1.886013408E-2 * 100.0, BI1 = 5.034698970E-1 * 100.0, BI0 = 6.109177956E+0 * 100.0;
  const double S16 = 0.516000335E-11 * 100.0, S15 = 0.276961083E-8 * 100.0, S14 = 0.623439266E-6 * 100.0, S13 = 0.754129933E-4 * 100.0,
               S12 = 0.517609116E-2 * 100.0, S11 = 0.191372282E+0 * 100.0, S10 = 0.298152339E+1 * 100.0;
  const double S26 = 0.314296723E-10 * 100.0, S25 = 0.132243858E-7 * 100.0, S24 = 0.236279781E-5 * 100.0, S23 = 0.230325039E-3 * 100.0,
               S22 = 0.129690326E-1 * 100.0, S21 = 0.401390832E+0 * 100.0, S20 = 0.535098336E+1 * 100.0;
  const double ti = tl < TMINICE ? TMINICE : tl > ZEROC ? ZEROC : tl;
  const double tt = ti - ZEROC;
  const double p1 = (tt * (tt * (tt * (tt * (tt * (tt * S16 + S15) + S14) + S13) + S12) + S11) + S10);
  const double p2 = (tt * (tt * (tt * (tt * (tt * (tt * S26 + S25) + S24) + S23) + S22) + S21) + S20);
  const double pi = (tt * (tt * (tt * (tt * (tt * (tt * BI6 + BI5) + BI4) + BI3) + BI2) + BI1) + BI0);
  if (tt < TSTARR1) return p1;
  if (tt < TSTARR2) { const double w = (TSTARR2 - tt) / (TSTARR2 - TSTARR1); return w * p1 + (1. - w) * p2; }
  if (tt < TSTARR3) return p2;
  if (tt < TSTARR4) { const double w = (TSTARR4 - tt) / (TSTARR4 - TSTARR3); return w * p2 + (1. - w) * pi; }
  return pi;
}
inline std::vector<double> bl_esinit() {
  const double ZEROC = 273.16, TMIX = -20.0, DELTA_T = 1.0 / blc::DEGSUBS;
  std::vector<double> x((size_t)blc::TABLESIZE);
  for (int i = 1; i <= blc::TABLESIZE; ++i) {
    double t = (i - 1) * DELTA_T + blc::TMINTBL;
    const double e = t > ZEROC ? bl_qsatlqu0(t) : bl_qsatice0(t), w = bl_qsatlqu0(t);
    t = t - ZEROC;
    x[(size_t)i - 1] = (t >= TMIX && t < 0.0) ? (t / TMIX) * (e - w) + w : e;
  }
  return x;
}

// ---- device --------------------------------------------------------------------------------------------------------------------------
// DQSAT_sub_sca (:1466-1518): piecewise-linear lookup, clamped at TMAXTBL - .001; the index is kept inside the table whatever TEMP is
HD void bl_dqsat(double& dqsi, double& qssi, double temp, double plo, const double* tbl) {
  FV3LM_LITERAL
  const double ESFAC = blc::H2OMW / blc::AIRMW;
  const double pp = plo * 100.0;
  double ti = temp;
  if (temp <= blc::TMINTBL) ti = blc::TMINTBL; else if (temp >= blc::TMAXTBL - .001) ti = blc::TMAXTBL - .001;
  const double tt = (ti - blc::TMINTBL) * blc::DEGSUBS + 1;
  int it = (int)tt;
  it = it < 1 ? 1 : it > blc::TABLESIZE - 1 ? blc::TABLESIZE - 1 : it;
  const double dqq = tbl[it] - tbl[it - 1];
  const double qq = (tt - it) * dqq + tbl[it - 1];
  if (pp <= qq) { qssi = 1.0; dqsi = 0.0; return; }
  const double dd = 1.0 / (pp - (1.0 - ESFAC) * qq);
  qssi = ESFAC * qq * dd;
  dqsi = (ESFAC * blc::DEGSUBS) * dqq * pp * (dd * dd);
}
// IceFraction (utils/fv3jedi_lm_utils_mod.F90:295-319)
HD double bl_icefraction(double temp) {
  FV3LM_LITERAL
  const double t_ice_all = 233.16, t_ice_max = 273.16;
  double f = 0.0;
  if (temp <= t_ice_all) f = 1.000; else if (temp <= t_ice_max) f = 1.00 - (temp - t_ice_all) / (t_ice_max - t_ice_all);
  f = f < 1.00 ? f : 1.00;
  f = f > 0.00 ? f : 0.00;
  const double f2 = f * f;
  return f2 * f2;
}
// LOUIS_DIFF (:444-498) at one interface: the layer above (zzu pvu uu vu), the layer below (zz pv u v), the interface height ze
HD void bl_louis(const BlParams& p, double pbllocal, double zzu, double zz, double pvu, double pv, double uu, double vu, double u, double v,
                 double ze, double& kh, double& km) {
  FV3LM_LITERAL
  const double LOUIS = p.r[0], LAMBDAM2 = p.r[2], LAMBDAH2 = p.r[4], ZKMENV = p.r[5], ZKHENV = p.r[6], MINTHICK = p.r[7], MINSHEAR = p.r[8], AKHMMAX = p.r[11];
  const double almfac = 1.2, alhfac = 1.2;
  double dz = zzu - zz;
  const double tm = (pvu + pv) * 0.5, dt = pvu - pv;
  double du = (uu - u) * (uu - u) + (vu - v) * (vu - v);
  dz = fmax(dz, MINTHICK);
  du = sqrt(du) / dz;
  const double ms = fmax(du, MINSHEAR);
  const double ri = blc::GRAV * (dt / dz) / (tm * (ms * ms));
  const double em = ze / ZKMENV, eh = ze / ZKHENV;
  const double lamm = fmax(0.1 * pbllocal * exp(-(em * em)), LAMBDAM2), lamh = fmax(0.1 * pbllocal * exp(-(eh * eh)), LAMBDAH2);
  const double bm = blc::KARMAN * ze / (1.0 + blc::KARMAN * (ze / lamm)), bh = blc::KARMAN * ze / (1.0 + blc::KARMAN * (ze / lamh));
  double alm = almfac * (bm * bm), alh = alhfac * (bh * bh);
  if (ri < 0.0) {
    const double c = pow(zzu / zz, 1. / 3.) - 1.0;
    double ps = c * c * c;
    ps = alh * sqrt(ps / (ze * (dz * dz * dz)));
    ps = ri / (1.0 + (3.0 * LOUIS * LOUIS) * ps * sqrt(-ri));
    kh = 1.0 - (LOUIS * 3.0) * ps;
    km = 1.0 - (LOUIS * 2.0) * ps;
  } else {
    const double ps = sqrt(1.0 + LOUIS * ri);
    kh = 1.0 / (1.0 + (LOUIS * 3.0) * ri * ps);
    km = ps / (ps + (LOUIS * 2.0) * ri);
  }
  alm = du * alm; alh = du * alh;
  km = fmin(km * alm, AKHMMAX);
  kh = fmin(kh * alh, AKHMMAX);
}

struct BlDriverFn {
  BlArgs a;
  HD void operator()(int i, int j, int t) const {
    FV3LM_LITERAL
    using namespace blc;
    const TurbArgs& ta = a.t;
    const int lm = ta.g.npz; const size_t pl = ta.g.plane, o = ta.col(t, i, j), os = (size_t)t * pl + ta.g.idx(i, j);
    auto plane = [&](int n) { return ta.fac + (size_t)n * ta.fs + o; };
    double* PE = plane(BLP_PE); double* TB = plane(BLP_T); double* QI = plane(BLP_QI); double* QL = plane(BLP_QL); double* ZH = plane(BLP_ZH);
    double* PV = plane(BLP_PV); double* SLV = plane(BLP_SLV); double* RDZ = plane(BLP_RDZ); double* TH = plane(BLP_TH);
    const double* U = ta.u.t + o; const double* V = ta.v.t + o; const double* T = ta.pt.t + o; const double* DP = ta.delp.t + o; const double* QV = ta.q[0].t + o;
    auto sfc = [&](int n) -> double& { return a.sfc[(size_t)n * a.ss + os]; };
    const double* r = a.p.r;
    const double LAMBDA_B = r[10], C_B = r[9], PRANDTLSFC = r[12], BETA_SURF = r[15], KHSFCFAC = r[17], TPFAC_SURF = r[18], ENTRATE_SURF = r[19], PCEFF_SURF = r[20];
    const int KPBLMIN = a.p.i[0];
    const double dtb = a.dt, ptop = ta.ptop;
    const size_t mb = (size_t)(lm - 1) * pl;      // the lowest level

    // ---- A: what set_ltraj prepares (:439-466) and T = PIf TH (:96-98)
    {
      double pe0 = ptop;
      for (int l = 0; l < lm; ++l) {
        const size_t m = (size_t)l * pl;
        const double pe1 = pe0 + DP[m], tt = T[m];
        const double th = ta.p00k * tt / turb_layer(pe0, pe1, ta.akap).pk;
        const double pf = 0.5 * (pe0 + pe1);
        PE[m] = pe1; TH[m] = th; TB[m] = pow(pf / P00, RGAS / CP) * th;
        if (a.cloud_mode == 1) {
          const double q = QI[m] + QL[m], f = bl_icefraction(tt);
          QI[m] = q * f; QL[m] = q * (1 - f);
        }
        pe0 = pe1;
      }
    }
    // ---- B: PRELIMINARY (:324-365) and the static energy of LOCK_DIFF (:743-768), bottom up
    {
      const double ramp = 20.;
      double zh1 = 0.0, zf1 = 0.0, tv1 = 0.0;
      double pke1 = pow(PE[mb] / P00, KAPPA);
      for (int l = lm - 1; l >= 0; --l) {
        const size_t m = (size_t)l * pl;
        const double pe_up = l > 0 ? PE[m - pl] : ptop;
        const double pke0 = pow(pe_up / P00, KAPPA);
        const double th = TH[m], tb = TB[m], qv = QV[m], qi = QI[m], ql = QL[m];
        const double zh = zh1 + (CP / GRAV) * th * (pke1 - pke0);
        const double zf = 0.5 * (zh + zh1);
        const double tv = tb * (1.0 + VIREPS * qv - qi - ql);      // QL_tot = QIT, QI_tot = QLT
        double hleff;
        if (tb <= TICE - ramp) hleff = ALHS;
        else if (tb < TICE) hleff = ((tb - TICE + ramp) * ALHL + (TICE - tb) * ALHS) / ramp;
        else hleff = ALHL;
        const double qc = qi + ql;
        ZH[m] = zh; PV[m] = tv * (th / tb);
        SLV[m] = CP * tb * (1 + VIREPS * qv - qc) + GRAV * zf - hleff * qc;
        if (l < lm - 1) {
          const double tve = (tv + tv1) * 0.5;
          double rdz = PE[m] / (RGAS * tve);
          rdz = rdz / (zf - zf1);
          RDZ[m] = rdz;
        }
        zh1 = zh; zf1 = zf; tv1 = tv; pke1 = pke0;
      }
      // running 1-2-1 smooth of the bottom levels (:360-365)
      double p0 = PV[mb - 6 * pl], p1 = PV[mb - 5 * pl], p2 = PV[mb - 4 * pl], p3 = PV[mb - 3 * pl], p4 = PV[mb - 2 * pl], p5 = PV[mb - pl], p6 = PV[mb];
      p6 = p5 * 0.25 + p6 * 0.75;
      p5 = p4 * 0.25 + p5 * 0.50 + p6 * 0.25;
      p4 = p3 * 0.25 + p4 * 0.50 + p5 * 0.25;
      p3 = p2 * 0.25 + p3 * 0.50 + p4 * 0.25;
      p2 = p1 * 0.25 + p2 * 0.50 + p3 * 0.25;
      p1 = p0 * 0.25 + p1 * 0.50 + p2 * 0.25;
      PV[mb - 5 * pl] = p1; PV[mb - 4 * pl] = p2; PV[mb - 3 * pl] = p3; PV[mb - 2 * pl] = p4; PV[mb - pl] = p5; PV[mb] = p6;
    }
    auto zfull = [&](int l) { return 0.5 * (ZH[(size_t)l * pl] + (l < lm - 1 ? ZH[(size_t)(l + 1) * pl] : 0.0)); };
    // ---- C: the surface-driven plume of LOCK_DIFF (:775-848).  Levels 0-based; the interface "k" of the reference is the top of level k
    const double bstar = sfc(BL_BSTAR), ustar = sfc(BL_USTAR);
    const int ibot = lm - 1;
    bool conv = false, pbl2 = false;
    int ipbl = -1;
    double k_entr = 0.0, zsml = 0.0, ee = 0.0, kfv = 0.0;
    if (bstar > 0.) {
      {   // mpbl_depth (:1094-1178)
        const double vscale = 0.25 / 100.;
        double tep = TB[mb], qp = QV[mb];
        tep = tep * (1. + TPFAC_SURF * bstar / GRAV);
        double u1 = U[mb], v1 = V[mb], z1 = zfull(ibot);
        zsml = z1;
        for (int k = lm - 2; k >= 1; --k) {
          const size_t m = (size_t)k * pl;
          const double z2 = zfull(k), t2 = TB[m], u2 = U[m], v2 = V[m], pp = 0.5 * (PE[m - pl] + PE[m]);
          double du = sqrt((u2 - u1) * (u2 - u1) + (v2 - v1) * (v2 - v1)) / (z2 - z1);
          du = fmin(du, 1.0e-8);
          const double entrate_x = ENTRATE_SURF * (1.0 + du / vscale);
          const double entfr = fmin(entrate_x * (z2 - z1), 0.99);
          qp = qp + entfr * (QV[m] - qp);
          tep = tep - GRAV * (z2 - z1) / CP;
          tep = tep + entfr * (t2 - tep);
          double dqsp, qsp;
          bl_dqsat(dqsp, qsp, tep, pp * 0.01, a.tbl);
          const double dqp = fmax(qp - qsp, 0.) / (1. + (ALHL / CP) * dqsp);
          qp = qp - dqp;
          tep = tep + PCEFF_SURF * ALHL * dqp / CP;
          if (t2 >= tep || entfr >= 0.9899) { zsml = 0.5 * (z2 + z1); ipbl = k + 1; break; }
          z1 = z2; u1 = u2; v1 = v2;
        }
      }
      if (ipbl < 0) { *a.flag = 1; return; }      // the parcel never stopped: the reference would index with ipbl = -1
      const double Ashear = 25.0, wentrmax = 0.05, akmax = 1.e4, critjump = 2.0;
      const double vsurf3 = ustar * bstar * zsml, vshear3 = Ashear * ustar * ustar * ustar;
      const double vsurf = pow(vsurf3, 1. / 3.);
      if (ipbl < ibot)
        for (int k = ibot; k >= ipbl + 1; --k) {
          const double tmpjump = (SLV[(size_t)(k - 1) * pl] - SLV[(size_t)k * pl]) / CP;
          if (tmpjump > critjump) { ipbl = k; zsml = ZH[(size_t)ipbl * pl]; break; }
        }
      const double s0 = SLV[(size_t)ipbl * pl], sm = SLV[(size_t)(ipbl - 1) * pl];
      const double tmp1 = GRAV * fmax(0.1, (sm - s0) / CP) / (s0 / CP);
      const double tmp2 = pow(vsurf3 + vshear3, 2. / 3.) / zsml;
      double wentr = fmin(wentrmax, fmax(0., (BETA_SURF * (vsurf3 + vshear3) / zsml) / (tmp1 + tmp2)));
      if (zsml < 1600.) wentr = wentr * (zsml / 800.); else wentr = 2. * wentr;
      k_entr = wentr * (zfull(ipbl - 1) - zfull(ipbl));
      k_entr = fmin(k_entr, akmax);
      conv = true;
      if (ipbl < ibot) {      // diffusivity_pbl2 (:1255-1302), hin = 0
        const double kfacx = sfc(BL_FRLAND) < 0.5 ? KHSFCFAC : KHSFCFAC * 2.0;
        if (vsurf * zsml > 0.) {
          ee = 1.0 - sqrt(k_entr / (kfacx * KARMAN * vsurf * zsml));
          ee = fmax(ee, 0.7);
          kfv = kfacx * KARMAN * vsurf;
          pbl2 = true;
        }
      }
    }
    // ---- D: LOUIS_DIFF, the max of LOCK_DIFF :1080-1085, TRIDIAG_SETUP, ORODRAG, top down
    {
      const double fro = sfc(BL_FROCEAN), cu = sfc(BL_CM), cq = sfc(BL_CQ), varflt = sfc(BL_VARFLT);
      double ct = sfc(BL_CT);
      if (fro == 1.0) ct = fro * ct;      // :168-174
      const double zzb = zfull(ibot);
      double pbllocal = sfc(BL_ZPBL);
      if (pbllocal <= zzb) pbllocal = zzb;
      double zpbl = 10.e15, zf_kpblmin = 0.0;
      double zh_c = ZH[0], zh_n = ZH[pl], pv_c = PV[0], u_c = U[0], v_c = V[0], pe_p = ptop, pe_c = PE[0];
      double kh_top = 0.0, aks = 0.0, akv = 0.0;
      for (int l = 0; l < lm; ++l) {
        const size_t m = (size_t)l * pl;
        const bool last = l == lm - 1;
        const double zf = 0.5 * (zh_c + zh_n);
        // everything this level and the next hold in the planes, before level l is overwritten
        double zh_nn = 0.0, pv_n = 0.0, u_n = 0.0, v_n = 0.0, pe_n = 0.0, rdz = 0.0;
        if (!last) {
          zh_nn = l < lm - 2 ? ZH[m + 2 * pl] : 0.0;
          pv_n = PV[m + pl]; u_n = U[m + pl]; v_n = V[m + pl]; pe_n = PE[m + pl]; rdz = RDZ[m];
        }
        double kh_b = 0.0, km_b = 0.0;      // the interface below level l = the top of level l + 1
        if (!last) {
          const double zf_n = 0.5 * (zh_n + zh_nn);
          bl_louis(a.p, pbllocal, zf, zf_n, pv_c, pv_n, u_c, v_c, u_n, v_n, zh_n, kh_b, km_b);
          double kt = 0.0, kmm = 0.0;
          if (conv) {
            if (l + 1 == ipbl) { kt = k_entr; kmm = k_entr; }
            else if (l + 1 > ipbl && pbl2 && zh_n <= zsml && zh_n > 0.0) {
              const double w = 1. - ee * (zh_n / zsml);
              kt = kfv * zh_n * (w * w);
              kmm = kt * PRANDTLSFC;
            }
          }
          kh_b = fmax(kt, kh_b); km_b = fmax(kmm, km_b);
        }
        if (l >= 1 && kh_top < 2. && kh_b >= 2.) zpbl = zf;      // :540-544: the lowest such level wins
        if (l == KPBLMIN - 1) zf_kpblmin = zf;
        const double dmi = (GRAV * dtb) / (pe_c - pe_p);
        double cks, ckq, ckv, ekv, aks_n = 0.0, akv_n = 0.0;
        if (!last) {
          const double dmi_n = (GRAV * dtb) / (pe_n - pe_c);
          cks = -kh_b * rdz; aks_n = cks * dmi_n; cks = cks * dmi; ckq = cks;
          ekv = -km_b * rdz; akv_n = ekv * dmi_n; ckv = ekv * dmi; ekv = -GRAV * ekv;
        } else {
          cks = -ct * dmi; ckq = -cq * dmi; ckv = -cu * dmi; ekv = GRAV * cu;
        }
        const double bks = 1.00 - (aks + cks), bkq = 1.00 - (aks + ckq);
        double bkv = 1.00 - (akv + ckv), fkv = 0.0;
        if (zf < 4.0 * LAMBDA_B) {      // ORODRAG (:636-648)
          double f = zf * (1.0 / LAMBDA_B);
          f = varflt * exp(-f * sqrt(f)) * pow(f, -1.2);
          f = (C_B / LAMBDA_B) * fmin(sqrt(u_c * u_c + v_c * v_c), 5.0) * f;
          bkv = bkv + dtb * f;
          fkv = f * (pe_c - pe_p);
        }
        plane(0)[m] = akv; plane(1)[m] = bkv; plane(2)[m] = ckv;
        plane(3)[m] = aks; plane(4)[m] = bks; plane(5)[m] = cks;
        plane(6)[m] = aks; plane(7)[m] = bkq; plane(8)[m] = ckq;
        if (a.ekv) { a.ekv[o + m] = ekv; a.fkv[o + m] = fkv; }
        kh_top = kh_b; aks = aks_n; akv = akv_n;
        zh_c = zh_n; zh_n = zh_nn; pv_c = pv_n; u_c = u_n; v_c = v_n; pe_p = pe_c; pe_c = pe_n;
        if (last) {
          if (zpbl == 10.e15) zpbl = zf;
          zpbl = fmin(zpbl, zf_kpblmin);
          sfc(BL_ZPBL) = zpbl; sfc(BL_CT) = ct;
        }
      }
    }
  }
};

inline void run_bl_driver(Exec& ex, const BlArgs& a) {
  const Geom& g = a.t.g;
  for_points(ex, Rect{g.is(), g.ie(), g.js(), g.je()}, g.ntile, BlDriverFn{a}, "turbulence_bldriver", 8. * (7. + 10.) * turb_cells(g));
}

}  // namespace fv3
