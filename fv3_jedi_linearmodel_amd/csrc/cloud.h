// fv3lm-hip: the linearised cloud scheme of the moist physics (physics/moist/cloud.F90 CLOUD_DRIVER, its tangent cloud_tl.F90
// CLOUD_DRIVER_D and adjoint cloud_ad.F90 CLOUD_DRIVER_B) and what set_ltraj (fv3jedi_lm_moist_mod.F90:834-874) prepares for it.
// Column-local; it follows the RAS convection of convection.h in every column and reads that feature's slot.
//
// The routine is written ONCE on a generic scalar T and run as values (double), tangent (RD) and adjoint (RV on the Tape of
// coltape.h), the scalars and the contraction rule of litcol.h.  cloud_tl.F90 is NOT everywhere the derivative of cloud.F90; where it
// is not, cloud_tl.F90 rules and the place is marked "TL:" below (DESIGN.md section 3 lists them with their line numbers).  At MIN / MAX /
// IF on a value the branch is taken on the value and the side is Tapenade's, read off cloud_tl.F90.
//
// Three kinds of segment, each a map of the column's state E (CLD_NE vectors of lm levels; the last one holds the carried scalars):
//   pre     theta -> T, QS of DQSAT_BAC, DZET, ZET, QDDF3 / VMIP                                         (cloud_tl.F90:246-302)
//   level   k = KTOP .. LM: cell k of the eight fields, the four sources of cell k, and the 18 carried scalars (:328-841)
//   post    the RH-excess clean-up, the Q < 0 fill with TPW, T -> theta                                  (:844-890)
// Level k touches nothing of another level except through the carried scalars, so the adjoint checkpoints per level the eight cell
// values and the carried scalars in a values sweep and then replays the segments last to first, ONE on the tape at a time; a level's
// leaves are its own cell and the carried scalars only.
// Dead code of the routine is left out: RH, the k = LM normalisation of the area accumulators (:634-672), QVn / TEn of LS_CLOUD, the
// triangular PDF (PDFSHAPE = 2; create refuses CLOUDPARAMS(57) /= 1).
//
// Launch shape: one thread per column, every column, work vectors [vector][level][column of the batch] (convection.h).
#pragma once
#include "convection.h"

namespace fv3 {

constexpr int CLD_BATCH = 2048;
// entries a column.  A segment is one level, or pre / post, never the column: the largest recorded in the host emulation over the mode tests
// is 616 entries at L20, L40 and L72 alike (the device has not been measured), a tenth of the capacity
constexpr int CLD_TAPE = 6144;
constexpr int CLD_KTOP = 30;
// state vectors (units of T); CE_SV holds the carried scalars at "levels" 1..18
enum { CE_T = 0, CE_Q, CE_QILS, CE_QLLS, CE_QICN, CE_QLCN, CE_CFLS, CE_CFCN, CE_DQL, CE_MFD, CE_PRC3, CE_UPDF, CE_QS, CE_DZET, CE_QDDF3, CE_SV, CLD_NE };
// carried scalars: per family (cu, an, ls) PRN PSN EVAP_DD SUBL_DD _above_new, then TOT_PREC and AREA of upd, anv, ls
enum { SV_CU = 1, SV_AN = 5, SV_LS = 9, SV_TOT_UPD = 13, SV_TOT_ANV, SV_TOT_LS, SV_AREA_UPD, SV_AREA_ANV, SV_AREA_LS, CLD_NSV = 18 };
// geometry vectors (double)
enum { CG_PH = 0, CG_PIH, CG_MASS, CG_DPI, CG_DM, CLD_NG };
// slot vectors (lm + 1 levels each), then the per-column scalars
enum { CS_QILS = 0, CS_QLLS, CS_QICN, CS_QLCN, CS_CFCN, CS_FRAC /* 4 */, CS_OUT = CS_FRAC + 4 /* 8 */, CS_PLE = CS_OUT + 8, CS_PMOD, CLD_NS };
enum { CSC_KHL = 0, CSC_KHU, CLD_NSC };
constexpr int CLD_NCK = 8 + CLD_NSV;

struct CldParams { double r[57]; };
namespace cldc {
constexpr double GRAV = blc::GRAV, ALHL = blc::ALHL, ALHF = blc::ALHF, ALHS = blc::ALHS, CP = blc::CP, RGAS = blc::RGAS, H2OMW = blc::H2OMW, AIRMW = blc::AIRMW,
                 TICE = blc::TICE, RVAP = blc::RUNIV / blc::H2OMW, RHO_W = 1.0e3;
constexpr double PI = 3.1415927410125732;      // MAPL_PI is a 4-byte real and fv3jedi_lm_moist_mod.F90:112 hands dble(MAPL_PI) to the scheme
}

// out with the perturbation c out' + (1 - c) in' (the sink and total filters, cloud_tl.F90:797-839): the value is out's
HD double cld_blend(double o, double, double) { FV3LM_LITERAL return o; }
HD RD cld_blend(const RD& o, const RD& i, double c) { FV3LM_LITERAL return RD(o.v, c * o.d + (1.0 - c) * i.d); }
HD RV cld_blend(const RV& o, const RV& i, double c) { FV3LM_LITERAL return rv2(o, i, o.v, c, 1.0 - c); }
// x ** p, p not an integer: Tapenade's derivative is 0 unless x > 0
template <class T> HD T cld_pow(const T& x, double p) { FV3LM_LITERAL
  const double v = rval(x);
  return v > 0.0 ? run1(x, pow(v, p), p * pow(v, p - 1.)) : T(pow(v, p));
}

struct CldCol {
  int lm, mst, khu, khl;
  ColWs g; const double* tbl; const double* r;
  double dt, frland;
  HD double G(int v, int l) const { FV3LM_LITERAL return g.at(v, l); }
};

// GET_ICE_FRACTION (cloud_tl.F90:2350-2393)
template <class T> HD T cld_icefrac(const T& temp, double t_ice_all, double t_ice_max, int pwr) { FV3LM_LITERAL
  const double t = rval(temp);
  T f(0.00);
  if (t <= t_ice_all) f = T(1.000);
  else if (t <= t_ice_max) f = 1.00 - (temp - t_ice_all) / (t_ice_max - t_ice_all);
  if (rval(f) > 1.00) f = T(1.00);
  if (rval(f) < 0.00) f = T(0.00);
  const double x = rval(f);
  double v = 1.0, v1 = 1.0;
  for (int n = 0; n < pwr; ++n) { v1 = v; v = v * x; }
  return x > 0.0 ? run1(f, v, pwr * v1) : T(v);
}
// MELTFREEZE (:991-1055)
template <class T> HD void cld_meltfreeze(double dt, T& te, T& ql, T& qi, double t_ice_all, double t_ice_max, int pwr) { FV3LM_LITERAL
  using namespace cldc;
  const double taufrz = 1000.;
  const T fqi = cld_icefrac(te, t_ice_all, t_ice_max, pwr);
  T dqil(0.0);
  if (rval(te) <= t_ice_max) {
    const T arg1 = -(dt * fqi / taufrz);
    const double e = exp(rval(arg1));
    dqil = ql * (1.0 - run1(arg1, e, e));
  }
  if (!(0. < rval(dqil))) dqil = T(0.);
  qi = qi + dqil; ql = ql - dqil;
  te = te + (ALHS - ALHL) * dqil / CP;
  dqil = T(0.);
  if (rval(te) > t_ice_max) dqil = -qi;
  if (!(0. > rval(dqil))) dqil = T(0.);
  qi = qi + dqil; ql = ql - dqil;
  te = te + (ALHS - ALHL) * dqil / CP;
}
// CLOUD_TIDY (:897-986)
template <class T> HD void cld_tidy(T& qv, T& te, T& qlc, T& qic, T& cf, T& qla, T& qia, T& af) { FV3LM_LITERAL
  using namespace cldc;
  if (rval(af) < 1.e-5) { qv = qv + qla + qia; te = te - ALHL / CP * qla - ALHS / CP * qia; af = T(0.); qla = T(0.); qia = T(0.); }
  if (rval(qlc) < 1.e-8) { qv = qv + qlc; te = te - ALHL / CP * qlc; qlc = T(0.); }
  if (rval(qic) < 1.e-8) { qv = qv + qic; te = te - ALHS / CP * qic; qic = T(0.); }
  if (rval(qla) < 1.e-8) { qv = qv + qla; te = te - ALHL / CP * qla; qla = T(0.); }
  if (rval(qia) < 1.e-8) { qv = qv + qia; te = te - ALHS / CP * qia; qia = T(0.); }
  if (rval(qla) + rval(qia) < 1.e-8) { qv = qv + qla + qia; te = te - ALHL / CP * qla - ALHS / CP * qia; af = T(0.); qla = T(0.); qia = T(0.); }
  if (rval(qlc) + rval(qic) < 1.e-8) { qv = qv + qlc + qic; te = te - ALHL / CP * qlc - ALHS / CP * qic; cf = T(0.); qlc = T(0.); qic = T(0.); }
}
// CONVEC_SRC (:1060-1148)
template <class T> HD void cld_convec_src(double dt, double imass, T& te, T& qv, const T& dcf, const T& dmf, T& qla, T& qia, T& af, const T& qs,
                                          double t_ice_all, double t_ice_max, int pwr) { FV3LM_LITERAL
  using namespace cldc;
  const double minrhx = 0.001;
  T tend = dcf * imass;
  const T fqi = cld_icefrac(te, t_ice_all, t_ice_max, pwr);
  qla = qla + (1.0 - fqi) * tend * dt;
  qia = qia + fqi * tend * dt;
  te = te + (ALHS - ALHL) * fqi * tend * dt / CP;
  tend = dmf * imass;
  af = af + tend * dt;
  if (rval(af) > 0.99) af = T(0.99);
  T qvx;
  if (rval(af) < 1.0) qvx = (qv - qs * af) / (1. - af); else qvx = qs;
  if (rval(qvx) - minrhx * rval(qs) < 0.0 && rval(af) > 0.) af = (qv - minrhx * qs) / (qs * (1.0 - minrhx));
  if (rval(af) < 0.) {
    af = T(0.0);
    qv = qv + qla + qia;
    te = te - (ALHL * qla + ALHS * qia) / CP;
    qla = T(0.0); qia = T(0.0);
  }
}
// the top-hat of PDFFRAC (flag 1, :1484-1502)
template <class T> HD T cld_tophat(const T& qt, const T& s1, const T& qstar) { FV3LM_LITERAL
  if (rval(qt) + rval(s1) < rval(qstar)) return T(0.);
  if (rval(s1) > 0.) {
    T min1;
    if (rval(qt) + rval(s1) - rval(qstar) > 2. * rval(s1)) min1 = 2. * s1; else min1 = qt + s1 - qstar;
    return min1 / (2. * s1);
  }
  return T(1.);
}
// PDFFRAC (:1463-1600), flag 1 and flag 4.  TL: with flag 4 the value is the top-hat and the perturbation the linear ramp in RH between
// 0.9335 and 1.0665 times 0.2 (:1564-1596)
template <class T> HD T cld_pdffrac(int flag, const T& qt, const T& s1, const T& qstar) { FV3LM_LITERAL
  const T top = cld_tophat(qt, s1, qstar);
  if (flag == 1) return top;
  const T rh = qt / qstar;
  const double q1 = 0.9335, q2 = 1.0665, r = rval(rh);
  if (r >= q1 && r < q2) return run1(rh, rval(top), (1. / ((q2 / q1 - 1) * q1)) * 0.2);
  return T(rval(top));
}
// PDFCONDENSATE (:1605-1750), flag 1
template <class T> HD T cld_pdfcond(const T& qt, const T& s1, const T& qstar) { FV3LM_LITERAL
  if (rval(qt) + rval(s1) < rval(qstar)) return T(0.);
  if (rval(qstar) > rval(qt) - rval(s1)) {
    if (rval(s1) > 0.) {
      T min1;
      if (rval(qt) + rval(s1) - rval(qstar) > 2. * rval(s1)) min1 = 2. * s1; else min1 = qt + s1 - qstar;
      return min1 * min1 / (4. * s1);
    }
    return qt - qstar;
  }
  return qt - qstar;
}
// LS_CLOUD (:1153-1457), PDFSHAPE = 1
template <class T> HD void cld_ls_cloud(const CldCol& c, double alpha, double pl, T& te, T& qv, T& qcl, T& qal, T& qci, T& qai, T& cf, T& af,
                                        double t_ice_all, double t_ice_max, int pwr, int pertmod, int dmp) { FV3LM_LITERAL
  using namespace cldc;
  const T qc = qcl + qci, qa = qal + qai;
  T dqsx, qsx;
  ras_dqsat(dqsx, qsx, te, pl, c.tbl);
  T tmparr(0.0);
  if (rval(af) < 1.0) {
    const double v = 1. / (1. - rval(af));
    // TL: below 1 - AF = 0.02 the perturbation of 1 / (1 - AF) is AF' / 0.02 ** 2 (do_moist_physics = 1, :1212-1219); any other dmp: none
    if (dmp == 1) { if (1. - rval(af) > 0.02) tmparr = 1. / (1. - af); else tmparr = run1(af, v, 1. / (0.02 * 0.02)); }
    else if (dmp == 2) tmparr = 1. / (1. - af);
    else tmparr = T(v);
  }
  const T qcx0 = qc * tmparr;
  T qvx = (qv - qsx * af) * tmparr;
  if (rval(af) >= 1.0) qvx = qsx * 1.e-4;
  T qax(0.);
  if (rval(af) > 0.) qax = qa / af;
  const T qt = qcx0 + qvx;
  const T qcp = qcx0, dqs = dqsx, qsn = qsx;
  const T fqi = cld_icefrac(te, t_ice_all, t_ice_max, pwr);
  const T sigmaqt1 = alpha * qsn;
  const T cfn = cld_pdffrac(pertmod == 0 ? 1 : 4, qt, sigmaqt1, qsn);
  T qcn = cld_pdfcond(qt, sigmaqt1, qsn);
  T qao(0.);
  if (rval(af) > 0.) qao = qax;
  const T alhx = (1.0 - fqi) * ALHL + fqi * ALHS;
  qcn = qcp + (qcn - qcp) / (1. - (cfn * (alpha - 1.) - qcn / qsn) * dqs * alhx / CP);
  T qco = qcn;
  if (rval(af) < 1.0) {
    cf = cfn * (1. - af);
    qco = qco * (1. - af);
    qao = qao * af;
  } else {
    cf = T(0.);
    qao = qa + qc;
    qco = T(0.);
    const T qt2 = qao + qv;
    if (rval(qt2) - rval(qsx) < 0.) qao = T(0.); else qao = qt2 - qsx;
  }
  const T qcx = qco - qc;
  T dqcl = (1.0 - fqi) * qcx, dqci = fqi * qcx;
  if (rval(qcl) + rval(dqcl) < 0.) { dqci = dqci + (qcl + dqcl); dqcl = -qcl; }
  if (rval(qci) + rval(dqci) < 0.) { dqcl = dqcl + (qci + dqci); dqci = -qci; }
  const T qax2 = qao - qa;
  T dqal = qax2, dqai(0.);
  if (rval(qal) + rval(dqal) < 0.) { dqai = dqai + (qal + dqal); dqal = -qal; }
  if (rval(qai) + rval(dqai) < 0.) { dqal = dqal + (qai + dqai); dqai = -qai; }
  if (rval(af) < 1.e-5) { dqai = -qai; dqal = -qal; }
  if (rval(cf) < 1.e-5) { dqci = -qci; dqcl = -qcl; }
  qai = qai + dqai; qal = qal + dqal; qci = qci + dqci; qcl = qcl + dqcl;
  qv = qv - (dqai + dqci + dqal + dqcl);
  te = te + (ALHL * (dqai + dqci + dqal + dqcl) + ALHF * (dqai + dqci)) / CP;
  if (rval(qao) <= 0.) {
    qv = qv + qai + qal;
    te = te - ALHS / CP * qai - ALHL / CP * qal;
    qai = T(0.); qal = T(0.); af = T(0.);
  }
}
// EVAP_CNV (:1755-1835) and SUBL_CNV (:1840-1920): ice false / true.  TL: the in-cloud condensate QCm carries no perturbation (:1802, :1887)
template <class T> HD void cld_evap_subl(bool ice, double dt, double rhcr, double pl, T& te, T& qv, T& ql, T& qi, T& f, const T& qs, double cld_evp_eff) { FV3LM_LITERAL
  using namespace cldc;
  const double k_cond = 2.4e-2, diffu = 2.2e-5, nn = ice ? 5. * 1.0e6 : 50. * 1.0e6;
  const double epsilon = H2OMW / AIRMW, a_eff = cld_evp_eff;
  const T es = 100. * pl * qs / (epsilon + (1.0 - epsilon) * qs);
  T rhx;
  if (rval(qv) / rval(qs) > 1.00) rhx = T(1.00); else rhx = qv / qs;
  const T k1 = ALHL * ALHL * RHO_W / (k_cond * RVAP * (te * te));
  const T k2 = RVAP * te * RHO_W / (diffu * (1000. / pl) * es);
  T& qx = ice ? qi : ql;
  double qcm = 0.;
  if (rval(f) > 0. && rval(qx) > 0.) qcm = rval(qx) / rval(f);
  // LDRADIUS (:1925-1950)
  const T pwx1 = qcm * (100. * pl / (RGAS * te)) / (nn * RHO_W * (4. / 3.) * PI);
  const T radius = cld_pow(pwx1, 1. / 3.);
  T teff(0.0);
  if (rval(rhx) < rhcr && rval(radius) > 0.0) teff = (rhcr - rhx) / ((k1 + k2) * (radius * radius));
  T evap = a_eff * qx * dt * teff;
  if (rval(evap) > rval(qx)) evap = qx;
  const T qc = ql + qi;
  if (rval(qc) > 0.) f = f * (qc - evap) / qc;
  qv = qv + evap;
  qx = qx - evap;
  te = te - (ice ? ALHS : ALHL) / CP * evap;
}
// AUTOCONVERSION_LS (:1955-2150) and _CNV (:2155-2345).  TL: the perturbation of F2 is halved (:1992, :2192)
template <class T> HD void cld_autoconv(bool ls, double dt, T& qc, T& qp, const T& te, double pl, T& f, double sundqv2, double sundqv3, double sundqt1,
                                        double c_00, double lwcrit) { FV3LM_LITERAL
  const double tv = rval(te);
  const T f2full = ras_sundq3(te, sundqv2, sundqv3, sundqt1);
  const T f2 = run1(f2full, rval(f2full), 0.5);
  const T c00x = c_00 * f2 * 1.0, iqccrx = f2 * 1.0 / lwcrit;
  T qcm(0.);
  if (rval(f) > 0. && rval(qc) > 0.) qcm = qc / f;
  const T qi = qcm * iqccrx;
  const T arg1 = -(qi * qi);
  const double e1 = exp(rval(arg1));
  T rate = c00x * (1.0 - run1(arg1, e1, e1));
  T f3(1.0);
  if (pl >= 775. && tv <= 275.) f3 = T(0.2);
  if (pl >= 825. && tv <= 282.) f3 = T(0.2);
  if (pl >= 775. && pl < 825. && tv <= 282. && tv > 275.) f3 = T(0.2);
  if (pl >= 825. && tv <= 275.) f3 = T(0.2);
  if (pl <= 775. || tv > 282.) f3 = T(1.);
  if (pl >= 950. && tv >= 285.) { if (0.2 * tv - 56 > 2.) f3 = T(2.); else f3 = 0.2 * te - 56.; }
  if (pl >= 925. && tv >= 290.) { if (0.04 * pl - 36. > 2.) f3 = T(2.); else f3 = T(0.04 * pl - 36.); }
  if (pl >= 925. && pl < 950. && tv > 285. && tv < 290.) {
    T x1;
    if (0.04 * pl + 0.2 * tv - 94. > 2.) x1 = T(2.); else x1 = 0.04 * pl + 0.2 * te - 94.;
    if (rval(x1) < 1.) f3 = T(1.); else f3 = x1;
  }
  if (pl >= 950. && tv >= 290.) f3 = T(2.);
  if (rval(f3) < 0.1) f3 = T(0.1);
  rate = f3 * rate;
  const T a2 = -(rate * dt);
  const double e2 = exp(rval(a2));
  T dqp = qc * (1.0 - run1(a2, e2, e2));
  if (rval(dqp) < 0.0) dqp = T(0.0);
  T dqfac(0.);
  if (pl >= 975. && tv >= 280.) {
    T x2;
    if (0.2 * tv - 56. > 1.) x2 = T(1.); else x2 = 0.2 * te - 56.;
    if (rval(x2) < 0.) dqfac = T(0.); else dqfac = x2;
  }
  if (pl >= 950. && tv >= 285.) {
    double x3;
    if (0.04 * pl - 38. > 1.) x3 = 1.; else x3 = 0.04 * pl - 38.;
    if (x3 < 0.) dqfac = T(0.); else dqfac = T(x3);
  }
  if (pl >= 950. && pl < 975. && tv > 280. && tv < 285.) {
    T x4;
    if (0.04 * pl + 0.2 * tv - 95. > 1.) x4 = T(1.); else x4 = 0.04 * pl + 0.2 * te - 95.;
    if (rval(x4) < 0.) dqfac = T(0.); else dqfac = x4;
  }
  if (pl >= 975. && tv >= 285.) dqfac = T(1.);
  if (rval(dqp) < rval(dqfac) * rval(qc)) dqp = dqfac * qc;
  qc = qc - dqp;
  qp = qp + dqp;
  if (ls && rval(qc) + rval(dqp) > 0.) f = qc * f / (qc + dqp);
}
// ICE_SETTLEFALL_CNV (:2512-2592) and _LS (:2597-2692)
template <class T> HD void cld_settlefall(bool ls, double wxr, T& qi, double pl, const T& te, T& f, int khu, int khl, int k, double dt, const T& dz, T& qp,
                                          double icefall_c) { FV3LM_LITERAL
  using namespace cldc;
  const T rho = 1000. * 100. * pl / (RGAS * te);
  T xim(0.);
  if (rval(f) > 0. && rval(qi) > 0.) xim = qi / f * rho;
  T vf;
  if (ls) vf = rval(xim) > 0.0 ? 109.0 * cld_pow(xim, 0.16) : T(0.0);
  else {
    T lxim(0.0);
    if (rval(xim) > 0.) lxim = run1(xim, log10(rval(xim)), 1. / (rval(xim) * log(10.0)));
    vf = 128.6 + 53.2 * lxim + 5.5 * (lxim * lxim);
  }
  if (wxr > 0.) vf = vf * pow(100. / (pl < 10. ? 10. : pl), wxr);
  vf = vf / 100.;
  if (khu > 0 && khl > 0 && k - 1 >= khu && k - 1 <= khl) vf = 0.01 * vf;
  vf = icefall_c * vf;
  T qixp = qi * (vf * dt / dz);
  if (rval(qixp) > rval(qi)) qixp = qi;
  if (rval(qixp) < 0.0) qixp = T(0.0);
  qp = qp + qixp;
  qi = qi - qixp;
  if (ls && rval(qi) + rval(qixp) > 0.) f = qi * f / (qi + qixp);
}
// MARSHPALM (:3033-3134): diam3, w, ve
template <class T> HD void cld_marshpalm(const T& rain, double pr, T& diam3, T& w, T& ve) { FV3LM_LITERAL
  const double rx[8] = {0., 5., 20., 80., 320., 1280., 5120., 20480.}, d3x[8] = {0.019, 0.032, 0.043, 0.057, 0.076, 0.102, 0.137, 0.183};
  const T rain_day = rain * 3600. * 24.;
  const double rd = rval(rain_day);
  diam3 = T(0.00);
  for (int i = 0; i < 7; ++i)
    if (rd <= rx[i + 1] && rd > rx[i]) { const double slopr = (d3x[i + 1] - d3x[i]) / (rx[i + 1] - rx[i]); diam3 = d3x[i] + (rain_day - rx[i]) * slopr; }
  if (rd >= rx[7]) diam3 = T(d3x[7]);
  diam3 = 0.664 * diam3;
  const double result1 = sqrt(1000. / pr);
  w = (2483.8 * diam3 + 80.) * result1;
  if (0.99 * rval(w) / 100. < 1.000) ve = T(1.000); else ve = 0.99 * w / 100.;
  diam3 = diam3 / 100.;
  w = w / 100.;
}
// PRECIPANDEVAP (:2700-3028).  above: PFL PFI EVAP_DD SUBL_DD, in: what the level above left, out: what this level leaves
template <class T> HD void cld_precipandevap(const CldCol& c, int k, double rhcr3, T& qpl, T& qpi, T& qcl, T& te, T& qv, double mass, double imass, double pl,
                                             const T& dze, const T& qddf3, const T& aa, const T& bb, const T& area, T* above, double envfc, double ddrfc,
                                             double revap_off_p, double c_acc, double c_ev_r, double c_ev_s) { FV3LM_LITERAL
  using namespace cldc;
  const double b_sub = 1.00, envfrac = envfc, ddfract = ddrfc, landseaf = 1.00;
  T ifactor(1.00);
  if (rval(area) > 0.) ifactor = 1. / area;
  if (rval(ifactor) < 1.) ifactor = T(1.);
  T dqs, qs;
  ras_dqsat(dqs, qs, te, pl, c.tbl);
  T pfl, pfi, evap_dd, subl_dd;
  if (k == CLD_KTOP) {
    pfl = qpl * mass; pfi = qpi * mass;
    evap_dd = T(0.); subl_dd = T(0.);
  } else {
    qpl = qpl + above[0] * imass;
    qpi = qpi + above[1] * imass;
    T accr = b_sub * c_acc * (qpl * mass) * qcl;
    if (rval(accr) > rval(qcl)) accr = qcl;
    qpl = qpl + accr; qcl = qcl - accr;
    accr = b_sub * c_acc * (qpi * mass) * qcl;
    if (rval(accr) > rval(qcl)) accr = qcl;
    qpi = qpi + accr; qcl = qcl - accr;
    te = te + ALHF * accr / CP;
    const T rainrat0 = ifactor * qpl * mass / c.dt, snowrat0 = ifactor * qpi * mass / c.dt;
    T diamrn, fallrn, vern, diamsn, fallsn, vesn;
    cld_marshpalm(rainrat0, pl, diamrn, fallrn, vern);
    cld_marshpalm(snowrat0, pl, diamsn, fallsn, vesn);
    const T tinlayerrn = dze / (fallrn + 0.01), tinlayersn = dze / (fallsn + 0.01);
    const double tau_frz = 5000.;
    if (rval(te) > TICE && rval(te) <= TICE + 5.) {
      T mltfrz = tinlayersn * qpi * (te - TICE) / tau_frz;
      if (!(rval(qpi) > rval(mltfrz))) mltfrz = qpi;
      te = te - ALHF * mltfrz / CP;
      qpl = qpl + mltfrz; qpi = qpi - mltfrz;
    }
    if (rval(te) > TICE + 5.) {
      const T mltfrz = qpi;
      te = te - ALHF * mltfrz / CP;
      qpl = qpl + mltfrz; qpi = qpi - mltfrz;
    }
    if (k >= c.lm - 1 && rval(te) > TICE + 0.) {
      const T mltfrz = qpi;
      te = te - ALHF * mltfrz / CP;
      qpl = qpl + mltfrz; qpi = qpi - mltfrz;
    }
    if (rval(te) <= TICE) {
      te = te + ALHF * qpl / CP;
      qpi = qpl + qpi;
      qpl = T(0.);
    }
    const T qko = qv, tko = te;
    const T dqstko = dqs;
    T qstko = qs + dqstko * (tko - te);
    if (rval(qstko) < 1.0e-7) qstko = T(1.0e-7);
    const T rh_box = qko / qstko;
    T efactor(9.99e9);
    if (rval(rh_box) < rhcr3) efactor = RHO_W * (aa + bb) / (rhcr3 - rh_box);
    T evap(0.0), subl(0.0);
    if (rval(rh_box) < rhcr3 && rval(diamrn) > 0.00 && pl > 100. && pl < revap_off_p) {
      const T droprad = 0.5 * diamrn;
      T t_ed = efactor * (droprad * droprad);
      t_ed = t_ed * (1.0 + dqstko * ALHL / CP);
      const T arg1 = -(c_ev_r * vern * landseaf * envfrac * tinlayerrn / t_ed);
      const double e = exp(rval(arg1));
      evap = qpl * (1.0 - run1(arg1, e, e));
    }
    if (rval(rh_box) < rhcr3 && rval(diamsn) > 0.00 && pl > 100. && pl < revap_off_p) {
      const T flakrad = 0.5 * diamsn;
      T t_ed = efactor * (flakrad * flakrad);
      t_ed = t_ed * (1.0 + dqstko * ALHS / CP);
      const T arg1 = -(c_ev_s * vesn * landseaf * envfrac * tinlayersn / t_ed);
      const double e = exp(rval(arg1));
      subl = qpi * (1.0 - run1(arg1, e, e));
    }
    qpi = qpi - subl; qpl = qpl - evap;
    evap_dd = above[2] + ddfract * evap * mass;
    evap = evap - ddfract * evap;
    subl_dd = above[3] + ddfract * subl * mass;
    subl = subl - ddfract * subl;
    qv = qv + evap + subl;
    te = te - evap * ALHL / CP - subl * ALHS / CP;
    pfl = qpl * mass; pfi = qpi * mass;
  }
  const T evap = qddf3 * evap_dd / mass, subl = qddf3 * subl_dd / mass;
  qv = qv + evap + subl;
  te = te - evap * ALHL / CP - subl * ALHS / CP;
  qpi = T(0.); qpl = T(0.);
  above[0] = pfl; above[1] = pfi; above[2] = evap_dd; above[3] = subl_dd;
}
// PDF_WIDTH (cloud.F90:1045-1096)
HD double cld_pdf_width(double pp, double frland, double maxrhcrit, double maxrhcritland, double turnrhcrit, double minrhcrit) { FV3LM_LITERAL
  const double pi_0 = 4. * atan(1.);
  double tempmaxrh = maxrhcrit;
  if (frland > 0.05) tempmaxrh = maxrhcritland;
  double a1;
  if (pp <= turnrhcrit) a1 = minrhcrit;
  else a1 = minrhcrit + (tempmaxrh - minrhcrit) / (19.) * ((atan((2. * (pp - turnrhcrit) / (1020. - turnrhcrit) - 1.) * tan(20. * pi_0 / 21. - 0.5 * pi_0)) + 0.5 * pi_0) * 21. / pi_0 - 1.);
  a1 = a1 < 1. ? a1 : 1.;
  const double alpha = 1. - a1;
  return alpha < 0.25 ? alpha : 0.25;
}

// ---- real parts of the eigenvalues of an 8 x 8 matrix: balancing-free Hessenberg reduction and shifted QR (EISPACK elmhes / hqr) -----------
HD double cld_max_abs_wr(double a[8][8]) { FV3LM_LITERAL
  const int n = 8;
  for (int m = 1; m < n - 1; ++m) {      // elmhes
    double x = 0.; int i = m;
    for (int j = m; j < n; ++j) if (fabs(a[j][m - 1]) > fabs(x)) { x = a[j][m - 1]; i = j; }
    if (i != m) {
      for (int j = m - 1; j < n; ++j) { const double t = a[i][j]; a[i][j] = a[m][j]; a[m][j] = t; }
      for (int j = 0; j < n; ++j) { const double t = a[j][i]; a[j][i] = a[j][m]; a[j][m] = t; }
    }
    if (x != 0.) for (i = m + 1; i < n; ++i) {
      double y = a[i][m - 1];
      if (y != 0.) {
        y /= x; a[i][m - 1] = y;
        for (int j = m; j < n; ++j) a[i][j] -= y * a[m][j];
        for (int j = 0; j < n; ++j) a[j][m] += y * a[j][i];
      }
    }
  }
  for (int i = 2; i < n; ++i) for (int j = 0; j < i - 1; ++j) a[i][j] = 0.;
  double wr[8];
  double anorm = 0.;
  for (int i = 0; i < n; ++i) for (int j = (i - 1 > 0 ? i - 1 : 0); j < n; ++j) anorm += fabs(a[i][j]);
  int nn = n - 1; double t = 0., p = 0., q = 0., r = 0., z = 0., w, x, y;
  while (nn >= 0) {
    int its = 0, l;
    do {
      for (l = nn; l >= 1; --l) {
        double s = fabs(a[l - 1][l - 1]) + fabs(a[l][l]);
        if (s == 0.) s = anorm;
        if (fabs(a[l][l - 1]) + s == s) { a[l][l - 1] = 0.; break; }
      }
      x = a[nn][nn];
      if (l == nn) { wr[nn--] = x + t; }
      else {
        y = a[nn - 1][nn - 1]; w = a[nn][nn - 1] * a[nn - 1][nn];
        if (l == nn - 1) {
          p = 0.5 * (y - x); q = p * p + w; z = sqrt(fabs(q)); x += t;
          if (q >= 0.) { z = p + (p >= 0. ? fabs(z) : -fabs(z)); wr[nn - 1] = wr[nn] = x + z; if (z != 0.) wr[nn] = x - w / z; }
          else { wr[nn - 1] = wr[nn] = x + p; }
          nn -= 2;
        } else {
          if (its == 60) { for (int i = 0; i <= nn; ++i) wr[i] = a[i][i] + t; nn = -1; break; }      // no convergence: the diagonal as it stands
          if (its == 10 || its == 20) {
            t += x;
            for (int i = 0; i <= nn; ++i) a[i][i] -= x;
            const double s = fabs(a[nn][nn - 1]) + fabs(a[nn - 1][nn - 2]);
            y = x = 0.75 * s; w = -0.4375 * s * s;
          }
          ++its;
          int m;
          for (m = nn - 2; m >= l; --m) {
            z = a[m][m]; r = x - z; const double s0 = y - z;
            p = (r * s0 - w) / a[m + 1][m] + a[m][m + 1]; q = a[m + 1][m + 1] - z - r - s0; r = a[m + 2][m + 1];
            const double s = fabs(p) + fabs(q) + fabs(r);
            p /= s; q /= s; r /= s;
            if (m == l) break;
            const double u = fabs(a[m][m - 1]) * (fabs(q) + fabs(r)), v = fabs(p) * (fabs(a[m - 1][m - 1]) + fabs(z) + fabs(a[m + 1][m + 1]));
            if (u + v == v) break;
          }
          for (int i = m + 2; i <= nn; ++i) { a[i][i - 2] = 0.; if (i != m + 2) a[i][i - 3] = 0.; }
          for (int k = m; k <= nn - 1; ++k) {
            if (k != m) {
              p = a[k][k - 1]; q = a[k + 1][k - 1]; r = 0.;
              if (k != nn - 1) r = a[k + 2][k - 1];
              if ((x = fabs(p) + fabs(q) + fabs(r)) != 0.) { p /= x; q /= x; r /= x; }
            }
            const double sq = sqrt(p * p + q * q + r * r), s = p >= 0. ? sq : -sq;
            if (s != 0.) {
              if (k == m) { if (l != m) a[k][k - 1] = -a[k][k - 1]; } else a[k][k - 1] = -s * x;
              p += s; x = p / s; y = q / s; z = r / s; q /= p; r /= p;
              for (int j = k; j <= nn; ++j) {
                p = a[k][j] + q * a[k + 1][j];
                if (k != nn - 1) { p += r * a[k + 2][j]; a[k + 2][j] -= p * z; }
                a[k + 1][j] -= p * y; a[k][j] -= p * x;
              }
              const int mmin = nn < k + 3 ? nn : k + 3;
              for (int i = l; i <= mmin; ++i) {
                p = x * a[i][k] + y * a[i][k + 1];
                if (k != nn - 1) { p += z * a[i][k + 2]; a[i][k + 2] -= p * r; }
                a[i][k + 1] -= p * q; a[i][k] -= p;
              }
            }
          }
        }
      }
    } while (nn >= 0 && l < nn - 1);
  }
  double mx = 0.;
  for (int i = 0; i < n; ++i) mx = mx < fabs(wr[i]) ? fabs(wr[i]) : mx;
  return mx;
}

// ---- pre (:246-302)
template <class T>
HD void cld_pre(const CldCol& c, const LitVecs<T>& V) { FV3LM_LITERAL
  using namespace cldc;
  const int lm = c.lm;
  const RArr<T> TE = V(CE_T), QS = V(CE_QS), DZET = V(CE_DZET), QDDF3 = V(CE_QDDF3);
  for (int l = 1; l <= lm; ++l) {
    const T th = TE(l);
    const T t = th * c.G(CG_PIH, l);
    T dq, qs;
    ras_dqsat(dq, qs, t, c.G(CG_PH, l), c.tbl);
    QS.set(l, qs);
    DZET.set(l, th * c.G(CG_DPI, l) * CP / GRAV);
    TE.set(l, t);
  }
  T zet(0.0), vmip(0.0);
  // VMIP = SUM(QDDF3) runs 1..LM while ZET accumulates LM..1: ZET first into QDDF3's place, then the sum in the reference's order
  for (int l = lm; l >= 1; --l) {
    zet = zet + DZET(l);
    if (rval(zet) < 3000.) QDDF3.set(l, -((zet - 3000.) * zet * c.G(CG_MASS, l))); else QDDF3.set(l, T(0.));
  }
  for (int l = 1; l <= lm; ++l) vmip = vmip + QDDF3(l);
  for (int l = 1; l <= lm; ++l) QDDF3.set(l, QDDF3(l) / vmip);
  for (int n = 1; n <= CLD_NSV; ++n) V(CE_SV).set(n, T(0.));
}

// ---- one level (:328-841).  pertmod: the switch of this cell (do_moist_physics = 1: 1).  jac (values, do_moist_physics = 2): the cell
// computes its own switch from the Jacobian of LS_CLOUD_D (:405-481) and returns it
template <class T>
HD int cld_level(const CldCol& c, const LitVecs<T>& V, int k, int pertmod, bool jac) { FV3LM_LITERAL
  using namespace cldc;
  const double* p = c.r;
  const double cnv_beta = p[0], anv_beta = p[1], ls_beta = p[2], rh00 = p[3], c_00 = p[4], lwcrit = p[5], c_acc = p[6], c_ev_r = p[7], c_ev_s = p[55],
               cld_evp_eff = p[12], ls_sdqv2 = p[14], ls_sdqv3 = p[15], ls_sdqvt1 = p[16], anv_sdqv2 = p[17], anv_sdqv3 = p[18], anv_sdqvt1 = p[19],
               anv_icefall_c = p[27], ls_icefall_c = p[28], revap_off_p = p[29], cnvenvfc = p[30], wrhodep = p[31], t_ice_all = p[32] + TICE,
               cnvddrfc = p[35], anvddrfc = p[36], lsddrfc = p[37], minrhcrit = p[41], maxrhcrit = p[42], turnrhcrit = p[44], maxrhcritland = p[45];
  const int icefrpwr = (int)(p[34] + .001);
  const double t_ice_max = TICE;
  const double ph = c.G(CG_PH, k), mass = c.G(CG_MASS, k), imass = 1 / mass;
  const RArr<T> SV = V(CE_SV);
  T t = V(CE_T)(k), q = V(CE_Q)(k), qi_ls = V(CE_QILS)(k), ql_ls = V(CE_QLLS)(k), qi_con = V(CE_QICN)(k), ql_con = V(CE_QLCN)(k), cf_ls = V(CE_CFLS)(k),
    cf_con = V(CE_CFCN)(k);
  const T qs = V(CE_QS)(k), dzet = V(CE_DZET)(k), qddf3 = V(CE_QDDF3)(k);
  const T t_pre = t, ql_ls_pre = ql_ls, ql_con_pre = ql_con, qi_ls_pre = qi_ls, qi_con_pre = qi_con;
  T tot_prec_upd = SV(SV_TOT_UPD), tot_prec_anv = SV(SV_TOT_ANV), tot_prec_ls = SV(SV_TOT_LS), area_upd_prc = SV(SV_AREA_UPD), area_anv_prc = SV(SV_AREA_ANV),
    area_ls_prc = SV(SV_AREA_LS);
  if (k == CLD_KTOP) { tot_prec_upd = T(0.); tot_prec_anv = T(0.); tot_prec_ls = T(0.); area_upd_prc = T(0.); area_anv_prc = T(0.); area_ls_prc = T(0.); }
  T qrn_ls(0.), qrn_an(0.), qsn_ls(0.), qsn_an(0.), qsn_cu(0.);
  T qrn_cu_1d = V(CE_PRC3)(k);
  cld_tidy(q, t, ql_ls, qi_ls, cf_ls, ql_con, qi_con, cf_con);
  cld_meltfreeze(c.dt, t, ql_ls, qi_ls, t_ice_all, t_ice_max, icefrpwr);
  cld_meltfreeze(c.dt, t, ql_con, qi_con, t_ice_all, t_ice_max, icefrpwr);
  cld_convec_src(c.dt, imass, t, q, V(CE_DQL)(k), V(CE_MFD)(k), ql_con, qi_con, cf_con, qs, t_ice_all, t_ice_max, icefrpwr);
  double alpha = cld_pdf_width(ph, c.frland, maxrhcrit, maxrhcritland, turnrhcrit, minrhcrit);
  if (alpha < 1.0 - rh00) alpha = 1.0 - rh00;
  const double rhcrit = 1.0 - alpha;
  if (jac) {
    pertmod = 0;
    double J[8][8], A[8][8];
    for (int ii = 0; ii < 8; ++ii) {
      RD x[8] = {RD(rval(t)), RD(rval(q)), RD(rval(qi_ls)), RD(rval(qi_con)), RD(rval(ql_ls)), RD(rval(ql_con)), RD(rval(cf_ls)), RD(rval(cf_con))};
      x[ii].d = 1.0;
      cld_ls_cloud<RD>(c, alpha, ph, x[0], x[1], x[4], x[5], x[2], x[3], x[6], x[7], t_ice_all, t_ice_max, icefrpwr, 0, c.mst);
      for (int m = 0; m < 8; ++m) { J[m][ii] = x[m].d; A[m][ii] = x[m].d; }
    }
    if (cld_max_abs_wr(A) > 1.001) pertmod = 1;
    if (J[0][0] < 0.6 || J[1][0] > 0.75e-4 || J[4][0] < -0.75e-4 || J[6][0] < -1.10) pertmod = 1;
  }
  cld_ls_cloud<T>(c, alpha, ph, t, q, ql_ls, ql_con, qi_ls, qi_con, cf_ls, cf_con, t_ice_all, t_ice_max, icefrpwr, pertmod, c.mst);
  const T t_presink = t, q_presink = q, qi_ls_presink = qi_ls, qi_con_presink = qi_con, ql_ls_presink = ql_ls, ql_con_presink = ql_con;
  (void)t_presink;
  T cf_tot = cf_ls + cf_con;
  if (rval(cf_tot) > 1.00) { cf_ls = cf_ls * (1.00 / cf_tot); cf_con = cf_con * (1.00 / cf_tot); }
  cld_evap_subl(false, c.dt, rhcrit, ph, t, q, ql_con, qi_con, cf_con, qs, cld_evp_eff);
  cld_evap_subl(true, c.dt, rhcrit, ph, t, q, ql_con, qi_con, cf_con, qs, cld_evp_eff);
  cld_autoconv(true, c.dt, ql_ls, qrn_ls, t, ph, cf_ls, ls_sdqv2, ls_sdqv3, ls_sdqvt1, c_00, lwcrit);
  cld_autoconv(false, c.dt, ql_con, qrn_an, t, ph, cf_con, anv_sdqv2, anv_sdqv3, anv_sdqvt1, c_00, lwcrit);
  cld_settlefall(false, wrhodep, qi_con, ph, t, cf_con, c.khu, c.khl, k, c.dt, dzet, qsn_an, anv_icefall_c);
  cld_settlefall(true, wrhodep, qi_ls, ph, t, cf_ls, c.khu, c.khl, k, c.dt, dzet, qsn_ls, ls_icefall_c);
  if (rval(t) < TICE) {
    qsn_cu = qrn_cu_1d;
    qrn_cu_1d = T(0.);
    t = t + qsn_cu * (ALHS - ALHL) / CP;
  }
  const T cnv_updf = V(CE_UPDF)(k);
  tot_prec_upd = tot_prec_upd + (qrn_cu_1d + qsn_cu) * mass;
  area_upd_prc = area_upd_prc + cnv_updf * (qrn_cu_1d + qsn_cu) * mass;
  tot_prec_anv = tot_prec_anv + (qrn_an + qsn_an) * mass;
  area_anv_prc = area_anv_prc + cf_con * (qrn_an + qsn_an) * mass;
  tot_prec_ls = tot_prec_ls + (qrn_ls + qsn_ls) * mass;
  area_ls_prc = area_ls_prc + cf_ls * (qrn_ls + qsn_ls) * mass;
  auto area1 = [&](const T& area, const T& tot) {
    T a(0.0);
    if (rval(tot) > 0.0) { if (rval(area) / rval(tot) < 1.e-6) a = T(1.e-6); else a = area / tot; }
    return a;
  };
  const T area_anv_prc1 = anv_beta * area1(area_anv_prc, tot_prec_anv), area_upd_prc1 = cnv_beta * area1(area_upd_prc, tot_prec_upd),
          area_ls_prc1 = ls_beta * area1(area_ls_prc, tot_prec_ls);
  // CONS_ALHX (:2484-2507), CONS_MICROPHYS (:2453-2479)
  T alhx3;
  if (rval(t) < t_ice_all) alhx3 = T(ALHS);
  else if (rval(t) > t_ice_max) alhx3 = T(ALHL);
  else alhx3 = ALHS + (ALHL - ALHS) * (t - t_ice_all) / (t_ice_max - t_ice_all);
  T aa, bb;
  {
    const double k_cond = 2.4e-2, diffu = 2.2e-5, epsi = H2OMW / AIRMW;
    const T e_sat = 100. * ph * qs / (epsi + (1.0 - epsi) * qs);
    aa = alhx3 * alhx3 / (k_cond * RVAP * (t * t));
    bb = RVAP * t / (diffu * (1000. / ph) * e_sat);
  }
  T qlt_tmp = ql_ls + ql_con;
  const T qit_tmp = qi_ls + qi_con;
  T above[4];
  auto family = [&](int base, T& qrn, T& qsn, const T& area, double envfc, double ddrfc) {
    for (int n = 0; n < 4; ++n) above[n] = SV(base + n);
    cld_precipandevap(c, k, rhcrit, qrn, qsn, qlt_tmp, t, q, mass, imass, ph, dzet, qddf3, aa, bb, area, above, envfc, ddrfc, revap_off_p, c_acc, c_ev_r, c_ev_s);
    for (int n = 0; n < 4; ++n) SV.set(base + n, above[n]);
  };
  family(SV_CU, qrn_cu_1d, qsn_cu, area_upd_prc1, cnvenvfc, cnvddrfc);
  family(SV_AN, qrn_an, qsn_an, area_anv_prc1, 1.0, anvddrfc);
  family(SV_LS, qrn_ls, qsn_ls, area_ls_prc1, 1.0, lsddrfc);
  {
    T qt_tmpi_1(0.0);
    if (rval(ql_ls) + rval(ql_con) > 0.00) qt_tmpi_1 = 1. / (ql_ls + ql_con);
    ql_ls = ql_ls * qlt_tmp * qt_tmpi_1;
    ql_con = ql_con * qlt_tmp * qt_tmpi_1;
    T qt_tmpi_2(0.0);
    if (rval(qi_ls) + rval(qi_con) > 0.00) qt_tmpi_2 = 1. / (qi_ls + qi_con);
    qi_ls = qi_ls * qit_tmp * qt_tmpi_2;
    qi_con = qi_con * qit_tmp * qt_tmpi_2;
  }
  // TL: the sink filter and the total filter act on the perturbation only (:797-839)
  const double sink = c.mst == 1 ? 0.65 : 0.9, tot_t = 0.25, tot_ql = c.mst == 1 ? 0.75 : 0.5, tot_qi = 1.0;
  if (k < 50) { qi_ls = cld_blend(qi_ls, qi_ls_presink, sink); qi_con = cld_blend(qi_con, qi_con_presink, sink); q = cld_blend(q, q_presink, sink); }
  if ((k - 62 < 0 ? 62 - k : k - 62) <= 2) { ql_ls = cld_blend(ql_ls, ql_ls_presink, sink); ql_con = cld_blend(ql_con, ql_con_presink, sink); }
  t = cld_blend(t, t_pre, tot_t);
  ql_ls = cld_blend(ql_ls, ql_ls_pre, tot_ql); ql_con = cld_blend(ql_con, ql_con_pre, tot_ql);
  if (tot_qi != 1.0) { qi_ls = cld_blend(qi_ls, qi_ls_pre, tot_qi); qi_con = cld_blend(qi_con, qi_con_pre, tot_qi); }
  V(CE_T).set(k, t); V(CE_Q).set(k, q); V(CE_QILS).set(k, qi_ls); V(CE_QLLS).set(k, ql_ls); V(CE_QICN).set(k, qi_con); V(CE_QLCN).set(k, ql_con);
  V(CE_CFLS).set(k, cf_ls); V(CE_CFCN).set(k, cf_con);
  SV.set(SV_TOT_UPD, tot_prec_upd); SV.set(SV_TOT_ANV, tot_prec_anv); SV.set(SV_TOT_LS, tot_prec_ls);
  SV.set(SV_AREA_UPD, area_upd_prc); SV.set(SV_AREA_ANV, area_anv_prc); SV.set(SV_AREA_LS, area_ls_prc);
  return pertmod;
}

// ---- post (:844-890)
template <class T>
HD void cld_post(const CldCol& c, const LitVecs<T>& V) { FV3LM_LITERAL
  using namespace cldc;
  const int lm = c.lm;
  const double rhexcess = 1.1;
  const RArr<T> TE = V(CE_T), Q = V(CE_Q);
  for (int l = 1; l <= lm; ++l) {
    T t = TE(l), q = Q(l), dqsdt, qs;
    ras_dqsat(dqsdt, qs, t, c.G(CG_PH, l), c.tbl);
    if (rval(q) > rhexcess * rval(qs)) {
      const T dqs = (q - rhexcess * qs) / (1.0 + rhexcess * dqsdt * ALHL / CP);
      q = q - dqs;
      t = t + ALHL / CP * dqs;
      Q.set(l, q); TE.set(l, t);
    }
  }
  T tpw(0.), negtpw(0.);
  for (int l = 1; l <= lm; ++l) tpw = tpw + Q(l) * c.G(CG_DM, l);
  for (int l = 1; l <= lm; ++l) if (rval(Q(l)) < 0.0) { negtpw = negtpw + Q(l) * c.G(CG_DM, l); Q.set(l, T(0.0)); }
  const T fac = 1.0 + negtpw / (tpw - negtpw);
  for (int l = 1; l <= lm; ++l) { Q.set(l, Q(l) * fac); TE.set(l, TE(l) / c.G(CG_PIH, l)); }
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------------------
struct CldArgs : ColView, ColWork {      // the cloud slot's packed columns and the columns of this launch; the work spaces of the batch
  double* rslot;                    // the convection slot of the same number: PTT_C QVT_C, the four _C sources, PLE, PKZ, FRLAND
  int mst;
  Fld pt, delp, q1, qi, ql;
  double* cfcn;                     // perturbation of the convective cloud fraction: the feature's own array, host-compact
                                    // [ntile][lm][ty][tx], or (cf_fld) the perturbation half of the bound tracer, padded planes like pt q1 qi ql
  double* cfcn_t;                   // bound: the trajectory half of that tracer (null otherwise)
  int cf_fld;
  double* src;                      // the four sources' perturbation (convection.h)
  const double* tbl; CldParams p;
  double dt, ptop, p00k;
  HD ColView ras() const { FV3LM_LITERAL ColView r = *this; r.slot = rslot; r.ns = RAS_NS; return r; }
  HD int kw() const { FV3LM_LITERAL return lm + 2 < CLD_NSV + 2 ? CLD_NSV + 2 : lm + 2; }
  HD double& cf(size_t col, int l) const { FV3LM_LITERAL return cfcn[cf_fld ? fld(col, l) : cmp(col, l)]; }      // level l (0-based) of the column's cfcn
  HD CldCol column(int m, size_t col) const { FV3LM_LITERAL
    CldCol c; c.lm = lm; c.mst = mst; c.khl = (int)SC(CSC_KHL, col); c.khu = (int)SC(CSC_KHU, col);
    c.g = ColWs{gw + m, (size_t)nb, kw()}; c.tbl = tbl; c.r = p.r; c.dt = dt; c.frland = ras().SC(SC_FRLAND, col);
    // p = ple 0.01, ph, pi = (p / 1000) ** (rgas / cp), pih, mass, dp, dm (:247-255, :267, :304-305)
    double p0 = S(CS_PLE, 0, col) * 0.01, pi0 = pow(p0 / 1000., cldc::RGAS / cldc::CP);
    for (int l = 1; l <= lm; ++l) {
      const double p1 = S(CS_PLE, l, col) * 0.01, pi1 = pow(p1 / 1000., cldc::RGAS / cldc::CP);
      const double ph = 0.5 * (p0 + p1);
      c.g.at(CG_PH, l) = ph; c.g.at(CG_PIH, l) = pow(ph / 1000., cldc::RGAS / cldc::CP);
      c.g.at(CG_MASS, l) = (p1 - p0) * 100. / cldc::GRAV; c.g.at(CG_DPI, l) = pi1 - pi0;
      c.g.at(CG_DM, l) = (S(CS_PLE, l, col) - S(CS_PLE, l - 1, col)) * (1. / cldc::GRAV);
      p0 = p1; pi0 = pi1;
    }
    return c;
  }
  // the trajectory the driver starts from, as values of the state vectors
  HD void load(const ColWs& w, size_t col) const { FV3LM_LITERAL
    const ColView r = ras();
    for (int l = 1; l <= lm; ++l) {
      w.at(CE_T, l) = r.S(S_OUT, l - 1, col); w.at(CE_Q, l) = r.S(S_OUT + 1, l - 1, col);
      w.at(CE_QILS, l) = S(CS_QILS, l - 1, col); w.at(CE_QLLS, l) = S(CS_QLLS, l - 1, col); w.at(CE_QICN, l) = S(CS_QICN, l - 1, col);
      w.at(CE_QLCN, l) = S(CS_QLCN, l - 1, col); w.at(CE_CFLS, l) = 0.; w.at(CE_CFCN, l) = S(CS_CFCN, l - 1, col);
      for (int v = 0; v < 4; ++v) w.at(CE_DQL + v, l) = r.S(S_OUT + 2 + v, l - 1, col);
    }
  }
};

// set: PLE in Pa from the resident delp, the IceFraction split and the fractions (set_ltraj :834-874), CLOUD_DRIVER in values with the
// per-cell switch; what: 0 set, 1 nonlinear run (the same sweep; the trajectory tracers are written and the slot is left alone)
struct CldSetFn {
  CldArgs a; int what;
  HD void operator()(int m, int, int) const { FV3LM_LITERAL
    const ColView r = a.ras();
    const size_t col = r.col_of(m); const int lm = r.lm;
    if (what == 0) {
      double pe = a.ptop;
      a.S(CS_PLE, 0, col) = pe;
      bool bad = false;
      for (int l = 0; l < lm; ++l) {
        pe = pe + a.delp.t[r.fld(col, l)];
        a.S(CS_PLE, l + 1, col) = pe;
        const double plo = 0.5 * (r.S(S_PLE, l, col) + r.S(S_PLE, l + 1, col));
        const double temp = r.S(S_THO, l, col) * pow(plo / 1000.0, cldc::RGAS / cldc::CP);
        const double fqi = bl_icefraction(temp);
        const double qls = a.S(CS_QILS, l, col), qcn = a.S(CS_QICN, l, col);      // the host's QLS, QCN as uploaded
        const double qils = qls * fqi, qlls = qls * (1 - fqi), qicn = qcn * fqi, qlcn = qcn * (1 - fqi);
        a.S(CS_QILS, l, col) = qils; a.S(CS_QLLS, l, col) = qlls; a.S(CS_QICN, l, col) = qicn; a.S(CS_QLCN, l, col) = qlcn;
        double f4[4] = {0., 0., 0., 0.};
        if (qils + qicn > 0.0) { f4[0] = qils / (qils + qicn); f4[1] = qicn / (qils + qicn); }
        if (qlls + qlcn > 0.0) { f4[2] = qlls / (qlls + qlcn); f4[3] = qlcn / (qlls + qlcn); }
        for (int n = 0; n < 4; ++n) a.S(CS_FRAC + n, l, col) = f4[n];
        bad = bad || turb_stored_nonfinite(&a.S(CS_PLE, l + 1, col)) || turb_stored_nonfinite(&a.S(CS_QILS, l, col)) || turb_stored_nonfinite(&a.S(CS_QICN, l, col));
      }
      if (bad) { *a.flag = 1; return; }
    }
    const CldCol c = a.column(m, col);
    const ColWs tw{a.tw + m, (size_t)a.nb, a.kw()};
    const LitVecs<double> V{tw, nullptr};
    a.load(tw, col);
    cld_pre<double>(c, V);
    for (int k = CLD_KTOP; k <= lm; ++k) {
      if (what == 0) a.S(CS_PMOD, k - 1, col) = (double)cld_level<double>(c, V, k, 1, a.mst == 2);
      else cld_level<double>(c, V, k, 1, false);
    }
    cld_post<double>(c, V);
    if (what == 0) {
      for (int l = 1; l < CLD_KTOP && l <= lm; ++l) a.S(CS_PMOD, l - 1, col) = 1.;
      for (int n = 0; n < 8; ++n) for (int l = 1; l <= lm; ++l) a.S(CS_OUT + n, l - 1, col) = tw.at(CE_T + n, l);
    } else {
      for (int l = 1; l <= lm; ++l) {
        const size_t n = r.fld(col, l - 1);
        a.qi.t[n] = tw.at(CE_QILS, l) + tw.at(CE_QICN, l);
        a.ql.t[n] = tw.at(CE_QLLS, l) + tw.at(CE_QLCN, l);
      }
    }
  }
};

// tangent (:429-438 in, :495-501 out of fv3jedi_lm_moist_mod.F90 around CLOUD_DRIVER_D)
struct CldTlFn {
  CldArgs a;
  HD void operator()(int m, int, int) const { FV3LM_LITERAL
    const ColView r = a.ras();
    const size_t col = r.col_of(m); const int lm = r.lm, kw = a.kw();
    const CldCol c = a.column(m, col);
    const ColWs ew{a.ew + m, (size_t)a.nb, kw}, tw{a.tw + m, (size_t)a.nb, kw};
    const LitVecs<RD> V{tw, nullptr};
    const size_t n3c = (size_t)r.ntile * lm * r.g.tx * r.g.ty;
    a.load(ew, col);
    for (int l = 1; l <= lm; ++l) {
      const size_t n = r.fld(col, l - 1), nc = r.cmp(col, l - 1);
      const double pk = r.S(S_PKZ, l - 1, col), qi = a.qi.p[n], ql = a.ql.p[n];
      const double d[12] = {a.pt.p[n] * a.p00k / pk, a.q1.p[n], qi * a.S(CS_FRAC, l - 1, col), ql * a.S(CS_FRAC + 2, l - 1, col), qi * a.S(CS_FRAC + 1, l - 1, col),
                            ql * a.S(CS_FRAC + 3, l - 1, col), 0., a.cf(col, l - 1), a.src[nc], a.src[n3c + nc], a.src[2 * n3c + nc], a.src[3 * n3c + nc]};
      for (int v = 0; v < 12; ++v) V(v).set(l, RD(ew.at(v, l), d[v]));
    }
    cld_pre<RD>(c, V);
    for (int k = CLD_KTOP; k <= lm; ++k) cld_level<RD>(c, V, k, (int)a.S(CS_PMOD, k - 1, col), false);
    cld_post<RD>(c, V);
    for (int l = 1; l <= lm; ++l) {
      const size_t n = r.fld(col, l - 1);
      const double pk = r.S(S_PKZ, l - 1, col);
      a.pt.p[n] = V(CE_T)(l).d * pk / a.p00k; a.q1.p[n] = V(CE_Q)(l).d;
      a.qi.p[n] = V(CE_QILS)(l).d + V(CE_QICN)(l).d; a.ql.p[n] = V(CE_QLLS)(l).d + V(CE_QLCN)(l).d;
      a.cf(col, l - 1) = V(CE_CFCN)(l).d;
    }
  }
};

// adjoint (:542-551 in, :607-616 out around CLOUD_DRIVER_B): values sweep with the checkpoints, then the segments last to first
struct CldAdFn {
  CldArgs a;
  HD void operator()(int m, int, int) const { FV3LM_LITERAL
    const ColView r = a.ras();
    const size_t col = r.col_of(m); const int lm = r.lm, kw = a.kw();
    const CldCol c = a.column(m, col);
    const ColWs tw{a.tw + m, (size_t)a.nb, kw}, ew{a.ew + m, (size_t)a.nb, kw}, ck{a.ck + m, (size_t)a.nb, kw};
    const ColWs eb{a.ew + (size_t)CLD_NE * kw * a.nb + m, (size_t)a.nb, kw};
    Tape tape; tape.m = a.tape; tape.col = (size_t)m; tape.n = 0;
    const LitVecs<double> EV{ew, nullptr};
    const LitVecs<RV> TV_{tw, &tape};
    const size_t n3c = (size_t)r.ntile * lm * r.g.tx * r.g.ty;
    for (int v = 0; v < CLD_NE; ++v) for (int l = 0; l < kw; ++l) { ew.at(v, l) = 0.; eb.at(v, l) = 0.; }
    a.load(ew, col);
    for (int l = 1; l <= lm; ++l) {
      const size_t n = r.fld(col, l - 1);
      const double pk = r.S(S_PKZ, l - 1, col), qi = a.qi.p[n], ql = a.ql.p[n];
      eb.at(CE_T, l) = a.pt.p[n] * pk / a.p00k; eb.at(CE_Q, l) = a.q1.p[n];
      eb.at(CE_QILS, l) = qi; eb.at(CE_QICN, l) = qi; eb.at(CE_QLLS, l) = ql; eb.at(CE_QLCN, l) = ql;
      eb.at(CE_CFCN, l) = a.cf(col, l - 1);
    }
    // the trajectory before pre is needed again: kept in the checkpoint store's last vectors
    const int T0 = CLD_NCK;
    for (int l = 1; l <= lm; ++l) ck.at(T0, l) = ew.at(CE_T, l);
    cld_pre<double>(c, EV);
    for (int k = CLD_KTOP; k <= lm; ++k) {
      for (int v = 0; v < 8; ++v) ck.at(v, k) = ew.at(v, k);
      for (int n = 1; n <= CLD_NSV; ++n) ck.at(7 + n, k) = ew.at(CE_SV, n);
      cld_level<double>(c, EV, k, (int)a.S(CS_PMOD, k - 1, col), false);
    }
    // one segment on the tape.  which 0 pre, 1 level k, 2 post.  Leaves are what the segment reads of E, and the incoming adjoints move
    // onto what it writes: pre reads theta and writes T QS DZET QDDF3 and the carried scalars; a level reads and writes its own cell of the
    // 15 vectors and the carried scalars; post reads and writes T and Q
    auto leaf = [&](int v, int l) { lit_leaf(tape, tw, ew, kw, v, l); };
    auto seed = [&](int v, int l) { lit_seed(tape, tw, eb, v, l); };
    auto segment = [&](int which, int k) {
      tape.n = 0;
      if (which == 0) { for (int l = 1; l <= lm; ++l) leaf(CE_T, l); cld_pre<RV>(c, TV_); }
      else if (which == 1) {
        for (int v = 0; v < CE_SV; ++v) leaf(v, k);
        for (int n = 1; n <= CLD_NSV; ++n) leaf(CE_SV, n);
        cld_level<RV>(c, TV_, k, (int)a.S(CS_PMOD, k - 1, col), false);
      } else { for (int l = 1; l <= lm; ++l) { leaf(CE_T, l); leaf(CE_Q, l); } cld_post<RV>(c, TV_); }
      if (which == 0) {
        const int o[4] = {CE_T, CE_QS, CE_DZET, CE_QDDF3};
        for (int v = 0; v < 4; ++v) for (int l = 1; l <= lm; ++l) seed(o[v], l);
        for (int n = 1; n <= CLD_NSV; ++n) seed(CE_SV, n);
      } else if (which == 1) {
        for (int v = 0; v < CE_SV; ++v) seed(v, k);
        for (int n = 1; n <= CLD_NSV; ++n) seed(CE_SV, n);
      } else for (int l = 1; l <= lm; ++l) { seed(CE_T, l); seed(CE_Q, l); }
      lit_walk_back(tape, eb, kw);
    };
    segment(2, 0);
    for (int k = lm; k >= CLD_KTOP; --k) {
      for (int v = 0; v < 8; ++v) ew.at(v, k) = ck.at(v, k);
      for (int n = 1; n <= CLD_NSV; ++n) ew.at(CE_SV, n) = ck.at(7 + n, k);
      segment(1, k);
    }
    // pre: the state before it (theta; the other vectors it reads are untouched by the levels' restores except T)
    for (int l = 1; l <= lm; ++l) ew.at(CE_T, l) = ck.at(T0, l);
    segment(0, 0);
    for (int l = 1; l <= lm; ++l) {
      const size_t n = r.fld(col, l - 1), nc = r.cmp(col, l - 1);
      const double pk = r.S(S_PKZ, l - 1, col);
      a.pt.p[n] = eb.at(CE_T, l) * a.p00k / pk; a.q1.p[n] = eb.at(CE_Q, l);
      a.qi.p[n] = eb.at(CE_QILS, l) * a.S(CS_FRAC, l - 1, col) + eb.at(CE_QICN, l) * a.S(CS_FRAC + 1, l - 1, col);
      a.ql.p[n] = eb.at(CE_QLLS, l) * a.S(CS_FRAC + 2, l - 1, col) + eb.at(CE_QLCN, l) * a.S(CS_FRAC + 3, l - 1, col);
      a.cf(col, l - 1) = eb.at(CE_CFCN, l);
      for (int v = 0; v < 4; ++v) a.src[(size_t)v * n3c + nc] = eb.at(CE_DQL + v, l);
    }
  }
};

// a bound tracer's trajectory half and the slot.  what 0: the trajectory cfcn into the slot (set_ltraj :720), gathered as convection_set
// gathers its fields; 1: CF_con as CLOUD_DRIVER in values left it into the trajectory (step_nl :388)
struct CldCfcnFn {
  CldArgs a; int what;
  HD void operator()(int m, int, int) const { FV3LM_LITERAL
    const size_t col = a.col_of(m);
    bool bad = false;
    for (int l = 0; l < a.lm; ++l) {
      const size_t n = a.fld(col, l);
      if (what == 0) { a.S(CS_CFCN, l, col) = a.cfcn_t[n]; bad = bad || turb_stored_nonfinite(&a.S(CS_CFCN, l, col)); }
      else a.cfcn_t[n] = a.S(CS_OUT + 7, l, col);
    }
    if (bad) *a.flag = 1;
  }
};

inline void run_cloud(Exec& ex, int what, const CldArgs& a) {      // what: -3 cfcn scatter, -2 cfcn gather, -1 set, 0 nl, 1 tl, 2 ad
  const Rect R{0, a.n - 1, 0, 0};
  if (a.n <= 0) return;
  if (what == -3) for_points(ex, R, 1, CldCfcnFn{a, 1}, "cloud_cfcn_scatter");
  else if (what == -2) for_points(ex, R, 1, CldCfcnFn{a, 0}, "cloud_cfcn_gather");
  else if (what == -1) for_points(ex, R, 1, CldSetFn{a, 0}, "cloud_set");
  else if (what == MODE_NL) for_points(ex, R, 1, CldSetFn{a, 1}, "cloud.nl");
  else if (what == MODE_TL) for_points(ex, R, 1, CldTlFn{a}, "cloud.tl");
  else for_points(ex, R, 1, CldAdFn{a}, "cloud.ad");
}

}  // namespace fv3
