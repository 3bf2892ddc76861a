// fv3lm-hip: linearised relaxed Arakawa-Schubert convection (physics/moist/convection.F90 RASE :10-638, RASE0 :834-1357 with ACRITN,
// SUNDQ3_ICE, DQSAT_RAS; their tangents convection_tl.F90 RASE_D, RASE0_D and adjoint convection_ad.F90 RASE_B) and what set_ltraj
// (fv3jedi_lm_moist_mod.F90:649-832, jacobian_filter_tlm :897-973) prepares around them.  Column-local.
//
// The routine is written ONCE on a generic scalar T and run as values (double), tangent (RD, a dual number) and adjoint (RV, a taped
// scalar on the Tape of coltape.h): the scalars of litcol.h, compiled like every function of this file with contraction into fused
// multiply-adds off (FV3LM_LITERAL), because the
// fixture is the reference's double result in the routine's order of operations.  At every kink the branch is taken on the VALUE and
// the side is Tapenade's (convection_tl.F90): MIN / MAX keep the first argument's derivative unless the second wins strictly as there,
// a clipped value is a constant, SQRT has derivative 0 at 0, a cloud type that leaves by a CYCLE before its update is the identity.
//
// Three segments, each a map of the column's state E (NE vectors of lm levels) onto itself:
//   pre    THO QHO UHO VHO -> POI QOI QST UOI VOI, DQQ BET GAM GHT GM1, POI_SV.. and TPERT (the strapped sub-cloud layer, DQSAT)
//   cloud  one cloud type IC: reads POI QOI QST UOI VOI and the invariants, updates them and the accumulators CLL RMFD RNS UPDFRC
//   post   de-strapping: THO QHO UHO VHO and the four sources CLW FLXD CNV_PRC3 CNV_UPDFRC
// Dead code of the routine is left out: the sounding before the cloud loop (:302-314, overwritten in every cloud type), BKE, RMFC,
// DLLX, CLLI, CLLX; ZLE / ZLO above the lowest level (only ZLO(K0) is read).
//
// Adjoint memory.  A tape of the whole routine would be (cloud types) x (taped operations of one) entries per column -- about 50 x
// 10^4 x 32 B = 16 MB -- so the adjoint tapes ONE segment at a time: a forward sweep in values stores POI QOI QST UOI VOI before every
// cloud type that fires (5 lm doubles each; the accumulators are additive, their values are not needed), then the segments are
// replayed last to first on the tape, every element of E a leaf whose adjoint is the incoming adjoint of that segment.  Per column in
// flight: checkpoints (5 lm + 1)(lm + 2) 8 B, tape RAS_TAPE_PER_LEVEL (lm + 2) 32 B, workspaces (3 NT + NE + NG)(lm + 2) 8 B
// (DESIGN.md section 3 has the figures); columns run in batches of at most RAS_BATCH, so the arena does not grow with the grid.
//
// Launch shape: one thread per column of a dense list (set: all columns; runs: the DOCONVEC columns, listed at set time), work vectors
// [vector][level][column of the batch] so that the lanes of a wave touch contiguous rows.
#pragma once
#include "litcol.h"
#include "bldriver.h"

namespace fv3 {

constexpr int RAS_BATCH = 2048;
constexpr int RAS_TAPE_PER_LEVEL = 420;
// state vectors (units of T)
enum { E_THO = 0, E_QHO, E_UHO, E_VHO, E_POI, E_QOI, E_QST, E_UOI, E_VOI, E_CLL, E_RMFD, E_RNS, E_UPD, E_DQQ, E_BET, E_GAM, E_GHT, E_GM1,
       E_SV, E_CLW, E_FLXD, E_PRC3, E_UPDF, RAS_NE };
// work vectors of a cloud type (units of T), after the state
enum { L_QOL = RAS_NE, L_SSL, L_HOL, L_HST, L_ZET, L_ZOL, L_SHT, L_QHT, L_ETA, L_HCC, L_EHT, L_CVW, L_RNN, L_GMS, L_GMH, L_UCU, L_VCU, RAS_NT };
// geometry vectors (double)
enum { G_PLE = 0, G_PKE, G_PF, G_PK, G_PRJ, G_PRS, G_PRH, G_PKI, G_DPT, G_DPB, G_PRI, G_POL, G_WGT, G_WG1, RAS_NG };
// slot vectors (lm + 1 levels each), then the per-column scalars
enum { S_THO = 0, S_QHO, S_UHO, S_VHO, S_PLE, S_PKZ, S_OUT /* 6 */, S_JAC = S_OUT + 6 /* 2 */, RAS_NS = S_JAC + 2 };
enum { SC_TS = 0, SC_FRLAND, SC_KCBL, SC_SEED, SC_DOCONVEC, RAS_NSC };

// ---- one column ------------------------------------------------------------------------------------------------------------------------
struct RasParams { double r[25]; };
struct RasCol {
  int lm, k, icmin, momentum;
  ColWs g;                      // geometry vectors
  const double* tbl; const double* sige; const double* r;
  double dt, ts, frland, mxdiam, co_auto;
  HD double G(int v, int l) const { FV3LM_LITERAL return g.at(v, l); }
};
namespace rasc {
constexpr double GRAV = blc::GRAV, ALHL = blc::ALHL, CP = blc::CP, RGAS = blc::RGAS, H2OMW = blc::H2OMW, AIRMW = blc::AIRMW, VIREPS = blc::VIREPS;
constexpr double ONEPKAP = 1. + 2. / 7., DAYLEN = 86400.0, RHMAX = 0.9999;
}

// everything of the routine that depends on the pressures and KCBL only (:185-187, :212-243, :253-256, :595-604)
HD void ras_geom(const RasCol& c) { FV3LM_LITERAL
  using namespace rasc;
  const int lm = c.lm, K = c.k;
  const ColWs& g = c.g;
  for (int l = 1; l <= lm + 1; ++l) g.at(G_PKE, l) = pow(g.at(G_PLE, l) / 1000., RGAS / CP);
  for (int l = 1; l <= lm; ++l) { g.at(G_PF, l) = 0.5 * (g.at(G_PLE, l) + g.at(G_PLE, l + 1)); g.at(G_PK, l) = pow(g.at(G_PF, l) / 1000., RGAS / CP); }
  for (int l = 1; l <= lm + 1; ++l) { g.at(G_PRJ, l) = g.at(G_PKE, l); g.at(G_PRS, l) = g.at(G_PLE, l); }
  double prcbl = g.at(G_PRS, K);
  for (int l = K; l <= lm; ++l) prcbl = prcbl + 1.0 * (g.at(G_PRS, l + 1) - g.at(G_PRS, l));
  g.at(G_PRS, K + 1) = prcbl;
  g.at(G_PRJ, K + 1) = pow(prcbl / 1000., RGAS / CP);
  for (int l = K; l >= c.icmin; --l) {
    const double p0 = g.at(G_PRS, l), p1 = g.at(G_PRS, l + 1), j0 = g.at(G_PRJ, l), j1 = g.at(G_PRJ, l + 1);
    g.at(G_POL, l) = 0.5 * (p0 + p1);
    const double prh = (p1 * j1 - p0 * j0) / (ONEPKAP * (p1 - p0));
    g.at(G_PRH, l) = prh; g.at(G_PKI, l) = 1.0 / prh; g.at(G_DPT, l) = prh - j0; g.at(G_DPB, l) = j1 - prh; g.at(G_PRI, l) = .01 / (p1 - p0);
  }
  double w0 = 0.;
  for (int l = K; l <= lm; ++l) {
    g.at(G_WGT, l) = 1.0 * (g.at(G_PLE, l + 1) - g.at(G_PLE, l)) / (g.at(G_PRS, K + 1) - g.at(G_PRS, K));
    w0 = w0 + 1.0 * (g.at(G_PLE, l + 1) - g.at(G_PLE, l));
  }
  w0 = (g.at(G_PRS, K + 1) - g.at(G_PRS, K)) / w0;
  for (int l = K; l <= lm; ++l) g.at(G_WG1, l) = w0 * 1.0;
}

// DQSAT_RAS / DQSATs_RAS (:705-832) and their tangents (convection_tl.F90:1049-1180)
template <class T>
HD void ras_dqsat(T& dqsi, T& qssi, const T& temp, double plo, const double* tbl) { FV3LM_LITERAL
  const double ESFAC = rasc::H2OMW / rasc::AIRMW;
  const double pp = plo * 100.0, tl = rval(temp);
  T ti = temp;
  if (tl <= blc::TMINTBL) ti = T(blc::TMINTBL); else if (tl >= blc::TMAXTBL - .001) ti = T(blc::TMAXTBL - .001);
  const T tt = (ti - blc::TMINTBL) * (double)blc::DEGSUBS + 1.;
  int it = (int)rval(tt);
  it = it < 1 ? 1 : it > blc::TABLESIZE - 1 ? blc::TABLESIZE - 1 : it;
  const double dqq = tbl[it] - tbl[it - 1];
  const T qq = (tt - (double)it) * dqq + tbl[it - 1];
  if (pp <= rval(qq)) { qssi = T(1.0); dqsi = T(0.0); return; }
  const T dd = 1.0 / (pp - (1.0 - ESFAC) * qq);
  qssi = ESFAC * qq * dd;
  dqsi = (ESFAC * blc::DEGSUBS) * dqq * pp * (dd * dd);
}
// SUNDQ3_ICE (:670-703), F3 = 1
template <class T>
HD T ras_sundq3(const T& temp, double rate2, double rate3, double te1) { FV3LM_LITERAL
  const double te0 = 273., te2 = 200., t = rval(temp);
  const double jump1 = (rate2 - 1.0) / pow(te0 - te1, 0.333);
  T f2;
  if (t >= te0) f2 = T(1.0);
  else if (t >= te1) { const T x = te0 - temp; f2 = 1.0 + jump1 * run1(x, pow(rval(x), 0.3333), 0.3333 * pow(rval(x), -0.6667)); }
  else f2 = rate2 + (rate3 - rate2) * (te1 - temp) / (te1 - te2);
  if (rval(f2) > 27.0) f2 = T(27.0);
  return f2;
}
// ACRITN (:640-668)
HD double ras_acritn(double pl, double plb, double acritfac) { FV3LM_LITERAL
  const double PH[15] = {150.0, 200.0, 250.0, 300.0, 350.0, 400.0, 450.0, 500.0, 550.0, 600.0, 650.0, 700.0, 750.0, 800.0, 850.0};
  const double A[15] = {1.6851, 1.1686, 0.7663, 0.5255, 0.4100, 0.3677, 0.3151, 0.2216, 0.1521, 0.1082, 0.0750, 0.0664, 0.0553, 0.0445, 0.0633};
  const int iwk = (int)(pl * 0.02 - 0.999999999);
  double acr;
  if (iwk > 1 && iwk <= 15) acr = A[iwk - 2] + (pl - PH[iwk - 2]) * .02 * (A[iwk - 1] - A[iwk - 2]);
  else if (iwk > 15) acr = A[14];
  else acr = A[0];
  return acritfac * acr * (plb - pl);
}

// ---- pre (:185-300 without the dead parts)
template <class T>
HD void ras_pre(const RasCol& c, const LitVecs<T>& V) { FV3LM_LITERAL
  using namespace rasc;
  const int lm = c.lm, K = c.k, icmin = c.icmin;
  const double LBCP = ALHL * (1.0 / CP);
  const RArr<T> THO = V(E_THO), QHO = V(E_QHO), UHO = V(E_UHO), VHO = V(E_VHO), POI = V(E_POI), QOI = V(E_QOI), QST = V(E_QST), UOI = V(E_UOI), VOI = V(E_VOI),
                DQQ = V(E_DQQ), BET = V(E_BET), GAM = V(E_GAM), GHT = V(E_GHT), GM1 = V(E_GM1), SV = V(E_SV);
  // TPERT (:194-208): only ZLO(K0) is read, and ZLE(K0 + 1) = 0
  T tpert;
  {
    const T zle = THO(lm) * (1. + VIREPS * QHO(lm));
    const T zlo = 0. + (CP / GRAV) * (c.G(G_PKE, lm + 1) - c.G(G_PK, lm)) * zle;
    const T tempf = THO(lm) * c.G(G_PK, lm);
    tpert = 1.0 * (c.ts - (tempf + GRAV * zlo / CP));
    if (rval(tpert) < 0.0) tpert = T(0.0);
    const double cap = c.frland < 0.1 ? 2.0 : 4.0;
    if (rval(tpert) > cap) tpert = T(cap);
  }
  for (int l = 1; l <= lm; ++l) {
    const bool in = l >= icmin && l <= K;
    T q(0.), d(0.);
    if (in) ras_dqsat(d, q, THO(l) * c.G(G_PK, l), c.G(G_PF, l), c.tbl);
    POI.set(l, in ? THO(l) : T(0.)); QOI.set(l, in ? QHO(l) : T(0.)); UOI.set(l, in ? UHO(l) : T(0.)); VOI.set(l, in ? VHO(l) : T(0.));
    QST.set(l, q); DQQ.set(l, d);
    V(E_CLL).set(l, T(0.)); V(E_RMFD).set(l, T(0.)); V(E_RNS).set(l, T(0.)); V(E_UPD).set(l, T(0.));
    BET.set(l, T(0.)); GAM.set(l, T(0.)); GHT.set(l, T(0.)); GM1.set(l, T(0.));
  }
  {   // the strapped layer (:246-267)
    T p(0.), q(0.), u(0.), v(0.);
    for (int l = K; l <= lm; ++l) {
      const double w = c.G(G_WGT, l);
      p = p + w * THO(l); q = q + w * QHO(l);
      if (c.momentum) { u = u + w * UHO(l); v = v + w * VHO(l); }
    }
    POI.set(K, p); QOI.set(K, q); UOI.set(K, u); VOI.set(K, v);
    T d, s;
    ras_dqsat(d, s, p * c.G(G_PRH, K), c.G(G_POL, K), c.tbl);
    DQQ.set(K, d); QST.set(K, s);
    SV.set(1, p); SV.set(2, q); SV.set(3, u); SV.set(4, v); SV.set(5, tpert);
  }
  for (int l = K; l >= icmin; --l) {
    const T dq = DQQ(l);
    BET.set(l, dq * c.G(G_PKI, l));
    GAM.set(l, c.G(G_PKI, l) / (1.0 + LBCP * dq));
    if (l < K) {
      const T dq1 = DQQ(l + 1);
      GHT.set(l + 1, GAM(l) * c.G(G_DPB, l) + GAM(l + 1) * c.G(G_DPT, l + 1));
      GM1.set(l + 1, 0.5 * LBCP * (dq / (ALHL * (1.0 + LBCP * dq)) + dq1 / (ALHL * (1.0 + LBCP * dq1))));
    }
  }
}

// ---- one cloud type (:316-579).  false: it left by a CYCLE before the update, the state is untouched
template <class T>
HD bool ras_cloud(const RasCol& c, const LitVecs<T>& V, int IC) { FV3LM_LITERAL
  using namespace rasc;
  const int K = c.k;
  const double* r = c.r;
  const double FRICFAC = r[0], CLI_CRIT = r[3], RASAL1 = r[4], RASAL2 = r[5], FRICLAMBDA = r[10], SDQV2 = r[13], SDQV3 = r[14], SDQVT1 = r[15],
               ACRITFAC = r[16], PBLFRAC = r[19], AUTORAMPB = r[20], RHMN = r[23], RHMX = r[24];
  const double CPI = 1.0 / CP, ALHI = 1.0 / ALHL, GRAVI = 1.0 / GRAV, CPBG = CP * GRAVI, DDT = DAYLEN / c.dt, LBCP = ALHL * CPI;
  const RArr<T> POI = V(E_POI), QOI = V(E_QOI), QST = V(E_QST), UOI = V(E_UOI), VOI = V(E_VOI), CLL = V(E_CLL), RMFD = V(E_RMFD), RNS = V(E_RNS), UPD = V(E_UPD),
                DQQ = V(E_DQQ), BET = V(E_BET), GAM = V(E_GAM), GHT = V(E_GHT), GM1 = V(E_GM1),
                QOL = V(L_QOL), SSL = V(L_SSL), HOL = V(L_HOL), HST = V(L_HST), ZET = V(L_ZET), ZOL = V(L_ZOL), SHT = V(L_SHT), QHT = V(L_QHT), ETA = V(L_ETA),
                HCC = V(L_HCC), EHT = V(L_EHT), CVW = V(L_CVW), RNN = V(L_RNN), GMS = V(L_GMS), GMH = V(L_GMH), UCU = V(L_UCU), VCU = V(L_VCU);
  auto PRJ = [&](int l) { return c.G(G_PRJ, l); };
  auto PRS = [&](int l) { return c.G(G_PRS, l); };
  auto PRH = [&](int l) { return c.G(G_PRH, l); };
  auto PKI = [&](int l) { return c.G(G_PKI, l); };
  auto DPT = [&](int l) { return c.G(G_DPT, l); };
  auto DPB = [&](int l) { return c.G(G_DPB, l); };
  auto PRI = [&](int l) { return c.G(G_PRI, l); };
  const T tpert = V(E_SV)(5);

  T trg;
  { const T x = (QOI(K) / QST(K) - RHMN) / (RHMX - RHMN); if (1. > rval(x)) trg = x; else trg = T(1.); }
  double f4 = (AUTORAMPB - c.sige[IC - 1]) / 0.2;
  f4 = 0.0 < f4 ? f4 : 0.0; f4 = 1.0 > f4 ? f4 : 1.0;
  if (rval(trg) <= 1.0e-5) return false;
  // the sounding up to the detrainment level, with the perturbed sub-cloud layer (POI_c, QOI_c; QPERT = 0)
  ZET.set(K + 1, T(0.));
  SHT.set(K + 1, CP * (POI(K) + tpert) * PRJ(K + 1));
  for (int l = K; l >= IC; --l) {
    const T pc = l == K ? POI(K) + tpert : POI(l);
    const T qc = l == K ? QOI(K) + 0.0 : QOI(l);
    const T qs = QST(l), a = qs * RHMAX;
    T qol = rval(a) > rval(qc) ? qc : a;
    if (!(0.000 < rval(qol))) qol = T(0.000);
    const T ssl = CP * PRJ(l + 1) * pc + GRAV * ZET(l + 1);
    QOL.set(l, qol); SSL.set(l, ssl);
    HOL.set(l, ssl + qol * ALHL);
    HST.set(l, ssl + qs * ALHL);
    const T tem = pc * (PRJ(l + 1) - PRJ(l)) * CPBG;
    ZOL.set(l, ZET(l + 1) + (PRJ(l + 1) - PRH(l)) * pc * CPBG);
    ZET.set(l, ZET(l + 1) + tem);
  }
  for (int l = IC + 1; l <= K; ++l) {
    const double tem = (PRJ(l) - PRH(l - 1)) / (PRH(l) - PRH(l - 1));
    SHT.set(l, SSL(l - 1) + tem * (SSL(l) - SSL(l - 1)));
    QHT.set(l, .5 * (QOL(l) + QOL(l - 1)));
  }
  const double LAMBDA_MIN = .2 / c.mxdiam, LAMBDA_MAX = .2 / 200.;
  if (rval(HOL(K)) <= rval(HST(IC))) return false;
  const T hstic = HST(IC);
  T tem = (hstic - HOL(IC)) * (ZOL(IC) - ZET(IC + 1));
  for (int l = IC + 1; l <= K - 1; ++l) tem = tem + (hstic - HOL(l)) * (ZET(l) - ZET(l + 1));
  if (rval(tem) <= 0.0) return false;
  const T alm = (HOL(K) - hstic) / tem;
  if (rval(alm) > LAMBDA_MAX) return false;
  T toki(1.0);
  if (rval(alm) < LAMBDA_MIN) { const T q = alm / LAMBDA_MIN; toki = q * q; }
  const T zetk = ZET(K);
  for (int l = IC + 1; l <= K; ++l) ETA.set(l, 1.0 + alm * (ZET(l) - zetk));
  ETA.set(IC, 1.0 + alm * (ZOL(IC) - zetk));
  // work function (MS-A22)
  T wfn(0.0);
  HCC.set(K, HOL(K));
  for (int l = K - 1; l >= IC + 1; --l) {
    const T hcc = HCC(l + 1) + (ETA(l) - ETA(l + 1)) * HOL(l);
    HCC.set(l, hcc);
    const T tm = HCC(l + 1) * DPB(l) + hcc * DPT(l);
    const T eht = ETA(l + 1) * DPB(l) + ETA(l) * DPT(l);
    EHT.set(l, eht);
    wfn = wfn + (tm - eht * HST(l)) * GAM(l);
  }
  HCC.set(IC, hstic * ETA(IC));
  wfn = wfn + (HCC(IC + 1) - hstic * ETA(IC + 1)) * GAM(IC) * DPB(IC);
  // vertical velocity
  {
    T bk2(0.0), hcld = HOL(K);
    for (int l = K - 1; l >= IC; --l) {
      hcld = (ETA(l + 1) * hcld + (ETA(l) - ETA(l + 1)) * HOL(l)) / ETA(l);
      const T tm = (hcld - HST(l)) * (ZET(l) - ZET(l + 1)) / (1.0 + LBCP * DQQ(l));
      const T max1 = rval(tm) < 0.0 ? T(0.0) : tm;
      bk2 = bk2 + GRAV * max1 / (CP * PRJ(l + 1) * POI(l));
      const T max2 = rval(bk2) < 0.0 ? T(0.0) : bk2;
      const T x = 2.0 * max2;
      const double sq = sqrt(rval(x));
      T cvw = rval(x) == 0.0 ? T(sq) : run1(x, sq, 0.5 / sq);
      if (rval(cvw) < 1.00) cvw = T(1.00);
      CVW.set(l, cvw);
    }
    CVW.set(K, T(1.00));
  }
  T rasal;
  if (rval(ZET(IC)) < 2000.) rasal = T(RASAL1); else rasal = RASAL1 + (RASAL2 - RASAL1) * (ZET(IC) - 2000.) / 8000.;
  if (rval(rasal) > 1.0e5) rasal = T(1.0e5);
  rasal = c.dt / rasal;
  const double acr = ras_acritn(c.G(G_POL, IC), PRS(K), ACRITFAC);
  if (rval(wfn) <= acr) return false;
  T wlq = QOL(K), uht = UOI(K), vht = VOI(K);
  RNN.set(K, T(0.));
  for (int l = K - 1; l >= IC; --l) {
    const T te = ETA(l) - ETA(l + 1);
    wlq = wlq + te * QOL(l);
    if (c.momentum) { uht = uht + te * UOI(l); vht = vht + te * VOI(l); }
    T cll0;
    if (l > IC) {
      const T tx2 = 0.5 * (QST(l) + QST(l - 1)) * ETA(l);
      const T tx3 = 0.5 * (HST(l) + HST(l - 1)) * ETA(l);
      const T qcc = tx2 + GM1(l) * (HCC(l) - tx3);
      cll0 = wlq - qcc;
    } else cll0 = wlq - QST(IC) * ETA(IC);
    if (rval(cll0) < 0.00) cll0 = T(0.00);
    const T cli = cll0 / ETA(l);
    const T te_a = POI(l) * PRH(l);
    const T f2 = ras_sundq3(te_a, SDQV2, SDQV3, SDQVT1);
    const double f3 = 1.0;
    const T c00_x = c.co_auto * f2 * f3 * f4;
    const T cli_crit_x = CLI_CRIT / (f2 * f3);
    const T arg = -((cli * cli) / (cli_crit_x * cli_crit_x));
    const double ea = exp(rval(arg));
    const T rate = c00_x * (1.0 - run1(arg, ea, ea));
    const T cvw_x = CVW(l);      // already >= 1
    const T dt_lyr = (ZET(l) - ZET(l + 1)) / cvw_x;
    T closs = cll0 * rate * dt_lyr;
    if (rval(closs) > rval(cll0)) closs = cll0;
    if (rval(closs) > 0.) { wlq = wlq - closs; RNN.set(l, closs); } else RNN.set(l, T(0.));
  }
  wlq = wlq - QST(IC) * ETA(IC);
  // gammas and kernel
  GMS.set(K, (SHT(K) - SSL(K)) * PRI(K));
  GMH.set(K, GMS(K) + (QHT(K) - QOL(K)) * PRI(K) * ALHL);
  T akm = GMH(K) * GAM(K - 1) * DPB(K - 1);
  T tx2 = GMH(K);
  for (int l = K - 1; l >= IC + 1; --l) {
    const T gms = (ETA(l) * (SHT(l) - SSL(l)) + ETA(l + 1) * (SSL(l) - SHT(l + 1))) * PRI(l);
    const T gmh = gms + (ETA(l) * (QHT(l) - QOL(l)) + ETA(l + 1) * (QOL(l) - QHT(l + 1))) * ALHL * PRI(l);
    GMS.set(l, gms); GMH.set(l, gmh);
    tx2 = tx2 + (ETA(l) - ETA(l + 1)) * gmh;
    akm = akm - gms * EHT(l) * PKI(l) + tx2 * GHT(l);
  }
  {
    const T gms = ETA(IC + 1) * (SSL(IC) - SHT(IC + 1)) * PRI(IC);
    GMS.set(IC, gms);
    akm = akm - gms * ETA(IC + 1) * DPB(IC) * PKI(IC);
    GMH.set(IC, gms + (ETA(IC + 1) * (QOL(IC) - QHT(IC + 1)) * ALHL + ETA(IC) * (hstic - HOL(IC))) * PRI(IC));
  }
  if (rval(akm) >= 0.0 || rval(wlq) < 0.0) return false;
  // cloud-base mass flux
  wfn = -((wfn - acr) / akm);
  {
    const T x1 = (rasal * trg * toki) * wfn;
    const double cap = (PRS(K + 1) - PRS(K)) * (100. * PBLFRAC);
    if (rval(x1) > cap) wfn = T(cap); else wfn = x1;
  }
  const T temf = wfn * GRAVI;
  CLL.set(IC, CLL(IC) + wlq * temf);
  RMFD.set(IC, RMFD(IC) + temf * ETA(IC));
  for (int l = IC + 1; l <= K; ++l) {
    const T rmfp = temf * ETA(l);
    if (rval(CVW(l)) > 0.0) UPD.set(l, UPD(l) + rmfp * (DDT / DAYLEN) * 1000. / (CVW(l) * PRS(l)));
  }
  // momentum is read before theta and q move (the friction block reads UOI, VOI, ETA only)
  for (int l = IC; l <= K; ++l) {
    RNS.set(l, RNS(l) + RNN(l) * temf);
    const T gmh = GMH(l) * wfn, gms = GMS(l) * wfn;
    QOI.set(l, QOI(l) + (gmh - gms) * ALHI);
    POI.set(l, POI(l) + gms * PKI(l) * CPI);
    QST.set(l, QST(l) + gms * BET(l) * CPI);
  }
  wfn = wfn * 0.5 * 1.0;
  if (!c.momentum || FRICFAC <= 0.0) return true;
  // cumulus friction
  {
    const T ax = -alm / FRICLAMBDA;
    const double ex = exp(rval(ax));
    wfn = wfn * FRICFAC * run1(ax, ex, ex);
  }
  T tm = wfn * PRI(K);
  UCU.set(K, 0. + tm * (UOI(K - 1) - UOI(K)));
  VCU.set(K, 0. + tm * (VOI(K - 1) - VOI(K)));
  for (int l = K - 1; l >= IC + 1; --l) {
    tm = wfn * PRI(l);
    UCU.set(l, 0. + tm * ((UOI(l - 1) - UOI(l)) * ETA(l) + (UOI(l) - UOI(l + 1)) * ETA(l + 1)));
    VCU.set(l, 0. + tm * ((VOI(l - 1) - VOI(l)) * ETA(l) + (VOI(l) - VOI(l + 1)) * ETA(l + 1)));
  }
  tm = wfn * PRI(IC);
  UCU.set(IC, 0. + (2. * (uht - UOI(IC) * (ETA(IC) - ETA(IC + 1))) - (UOI(IC) + UOI(IC + 1)) * ETA(IC + 1)) * tm);
  VCU.set(IC, 0. + (2. * (vht - VOI(IC) * (ETA(IC) - ETA(IC + 1))) - (VOI(IC) + VOI(IC + 1)) * ETA(IC + 1)) * tm);
  for (int l = IC; l <= K; ++l) { UOI.set(l, UOI(l) + UCU(l)); VOI.set(l, VOI(l) + VCU(l)); }
  return true;
}

// ---- post (:581-636).  any: a cloud type fired (SUM(RMF) > 0: every contribution to RMF is positive)
template <class T>
HD void ras_post(const RasCol& c, const LitVecs<T>& V, bool any) { FV3LM_LITERAL
  using namespace rasc;
  const int lm = c.lm, K = c.k, icmin = c.icmin;
  const double DDT = DAYLEN / c.dt;
  const RArr<T> CLW = V(E_CLW), FLXD = V(E_FLXD), PRC3 = V(E_PRC3), UPDF = V(E_UPDF), SV = V(E_SV);
  for (int l = 1; l <= lm; ++l) { CLW.set(l, T(0.)); FLXD.set(l, T(0.)); PRC3.set(l, T(0.)); UPDF.set(l, T(0.)); }
  if (!any) return;
  const T dp = V(E_POI)(K) - SV(1), dq = V(E_QOI)(K) - SV(2), du = V(E_UOI)(K) - SV(3), dv = V(E_VOI)(K) - SV(4);
  for (int l = icmin; l <= K; ++l) PRC3.set(l, V(E_RNS)(l) * (c.G(G_PRI, l) * GRAV));
  for (int l = icmin; l <= K - 1; ++l) {
    V(E_THO).set(l, V(E_POI)(l)); V(E_QHO).set(l, V(E_QOI)(l));
    if (c.momentum) { V(E_UHO).set(l, V(E_UOI)(l)); V(E_VHO).set(l, V(E_VOI)(l)); }
    UPDF.set(l, V(E_UPD)(l));
  }
  for (int l = K; l <= lm; ++l) {
    const double w = c.G(G_WG1, l);
    V(E_THO).set(l, V(E_THO)(l) + w * dp); V(E_QHO).set(l, V(E_QHO)(l) + w * dq);
    if (c.momentum) { V(E_UHO).set(l, V(E_UHO)(l) + w * du); V(E_VHO).set(l, V(E_VHO)(l) + w * dv); }
  }
  for (int l = icmin; l <= K; ++l) {
    if (l == K && K < lm) continue;      // FLXD, CLW (K:K0) = 0 when K < K0
    FLXD.set(l, V(E_RMFD)(l) * DDT / DAYLEN); CLW.set(l, V(E_CLL)(l) * DDT / DAYLEN);
  }
}

// the whole routine in one scalar (values, tangent)
template <class T>
HD bool ras_column(const RasCol& c, const LitVecs<T>& V) { FV3LM_LITERAL
  ras_pre<T>(c, V);
  bool any = false;
  for (int ic = c.k; ic >= c.icmin + 1; --ic) any = ras_cloud<T>(c, V, ic) || any;
  ras_post<T>(c, V, any);
  return any;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------------------
struct RasArgs : ColView, ColWork {      // the slot's packed columns and the columns of this launch; the work spaces of the batch
  int icmin, mst;
  Fld u, v, pt, delp, q1;
  double* src;                      // four sources of the perturbation, host-compact [4][ntile][lm][ty][tx]
  const double* tbl; const double* sige; RasParams p;
  double dt, ptop, akap, p00k;
  HD int kw() const { FV3LM_LITERAL return lm + 2 < 7 ? 7 : lm + 2; }
  HD RasCol column(int m, size_t col, int momentum) const { FV3LM_LITERAL
    RasCol c; c.lm = lm; c.icmin = icmin; c.momentum = momentum; c.k = (int)SC(SC_KCBL, col);
    c.g = ColWs{gw + m, (size_t)nb, kw()}; c.tbl = tbl; c.sige = sige; c.r = p.r;
    c.dt = dt; c.ts = SC(SC_TS, col); c.frland = SC(SC_FRLAND, col); c.co_auto = 2.5e-3;
    const double sd = SC(SC_SEED, col) / 1000000.;
    const double rndu = sd < 1e-6 ? 1e-6 : sd;
    c.mxdiam = p.r[22] * pow(rndu, -(1. / 2.));
    for (int l = 1; l <= lm + 1; ++l) c.g.at(G_PLE, l) = S(S_PLE, l - 1, col);
    ras_geom(c);
    return c;
  }
};

// set, part A: the trajectory the slot keeps (set_ltraj :700-743), every column
struct RasGatherFn {
  RasArgs a;
  HD void operator()(int m, int, int) const { FV3LM_LITERAL
    const size_t col = a.col_of(m); const int lm = a.lm;
    double pe0 = a.ptop;
    a.S(S_PLE, 0, col) = 0.01 * pe0;
    bool bad = false;
    double temp_lm = 0.;
    for (int l = 0; l < lm; ++l) {
      const size_t n = a.fld(col, l);
      const double pe1 = pe0 + a.delp.t[n], pk = turb_layer(pe0, pe1, a.akap).pk;
      const double th = a.p00k * a.pt.t[n] / pk;
      a.S(S_THO, l, col) = th; a.S(S_QHO, l, col) = a.q1.t[n]; a.S(S_UHO, l, col) = a.u.t[n]; a.S(S_VHO, l, col) = a.v.t[n];
      a.S(S_PKZ, l, col) = pk; a.S(S_PLE, l + 1, col) = 0.01 * pe1;
      bad = bad || turb_stored_nonfinite(&a.S(S_THO, l, col)) || turb_stored_nonfinite(&a.S(S_QHO, l, col)) || turb_stored_nonfinite(&a.S(S_UHO, l, col)) ||
            turb_stored_nonfinite(&a.S(S_VHO, l, col)) || turb_stored_nonfinite(&a.S(S_PLE, l + 1, col));
      if (l == lm - 1) {
        const double plo = 0.5 * (a.S(S_PLE, l, col) + a.S(S_PLE, l + 1, col));
        temp_lm = th * pow(plo / 1000.0, rasc::RGAS / rasc::CP);
      }
      pe0 = pe1;
    }
    if (bad) { *a.flag = 1; a.SC(SC_SEED, col) = 0.; return; }
    const double x = 100 * temp_lm;
    a.SC(SC_SEED, col) = (double)(int)(1000000 * (x - (double)(int)x));
  }
};

// set, part B: RASE0 on copies, the heating-rate filter (:796-823), the Jacobian filter (:897-973; only its first column exists)
struct RasSetFn {
  RasArgs a;
  HD void operator()(int m, int, int) const { FV3LM_LITERAL
    const size_t col = a.col_of(m); const int lm = a.lm;
    const RasCol c = a.column(m, col, 0);
    const int K = c.k;
    const ColWs tw{a.tw + m, (size_t)a.nb, a.kw()};
    {
      const LitVecs<double> V{tw, nullptr};
      for (int l = 1; l <= lm; ++l) { V(E_THO).set(l, a.S(S_THO, l - 1, col)); V(E_QHO).set(l, a.S(S_QHO, l - 1, col)); V(E_UHO).set(l, 0.); V(E_VHO).set(l, 0.); }
      ras_column<double>(c, V);
      const int src[6] = {E_THO, E_QHO, E_CLW, E_FLXD, E_PRC3, E_UPDF};
      for (int n = 0; n < 6; ++n) for (int l = 1; l <= lm; ++l) a.S(S_OUT + n, l - 1, col) = V(src[n])(l);
    }
    for (int l = 0; l < lm; ++l) { a.S(S_JAC, l, col) = 0.; a.S(S_JAC + 1, l, col) = 0.; }
    int doconvec = 0;
    {
      auto heat = [&](int l) { return fabs((a.S(S_OUT, l - 1, col) - a.S(S_THO, l - 1, col)) / a.dt); };
      double hmax = 0.;
      for (int l = 1; l <= lm; ++l) hmax = hmax < heat(l) ? heat(l) : hmax;
      int ctop = lm;
      for (int l = 1; l <= lm; ++l) if (heat(l) > 0.01 * hmax) { ctop = l; break; }
      double sum = 0.;
      if (ctop != lm && K - ctop > 0) {
        double s = 0., mx = 0.;
        for (int l = ctop; l <= K - 1; ++l) { s += heat(l); mx = mx < heat(l) ? heat(l) : mx; }
        sum = (s - mx) / (K - ctop);
      }
      const int maxcondep = a.mst == 1 ? 1 : 10;
      if (K - ctop >= maxcondep) {
        double mx = 0.;
        for (int l = 1; l <= K - 1; ++l) mx = mx < heat(l) ? heat(l) : mx;
        // sumHEAT / maxval > 0.125; 0 / 0 compares false as in the reference
        if (mx > 0. ? sum / mx > 0.125 : sum > 0.) doconvec = 1;
      }
    }
    if (doconvec) {
      const LitVecs<RD> V{tw, nullptr};
      for (int l = 1; l <= lm; ++l) {
        V(E_THO).set(l, RD(a.S(S_THO, l - 1, col), l == K ? 1. : 0.)); V(E_QHO).set(l, RD(a.S(S_QHO, l - 1, col), 0.));
        V(E_UHO).set(l, RD(0.)); V(E_VHO).set(l, RD(0.));
      }
      ras_column<RD>(c, V);
      double hm = 0., mm = 0.;
      for (int l = 1; l <= lm; ++l) {
        const double h = (V(E_THO)(l).d - (l == K ? 1. : 0.)) / a.dt, q = (V(E_QHO)(l).d - 0.) / a.dt;
        a.S(S_JAC, l - 1, col) = h; a.S(S_JAC + 1, l - 1, col) = q;
        hm = hm < fabs(h) ? fabs(h) : hm; mm = mm < fabs(q) ? fabs(q) : mm;
      }
      if (hm > 0.00010 || mm > 1.0e-07) doconvec = 0;
    }
    a.SC(SC_DOCONVEC, col) = doconvec;
  }
};

// nonlinear (RASE_D with a zero perturbation, the values written back) and tangent run on the DOCONVEC columns
template <class T>
struct RasRunFn {
  RasArgs a;
  HD void operator()(int m, int, int) const { FV3LM_LITERAL
    const size_t col = a.col_of(m); const int lm = a.lm;
    const RasCol c = a.column(m, col, 1);
    const ColWs tw{a.tw + m, (size_t)a.nb, a.kw()};
    const LitVecs<T> V{tw, nullptr};
    const Fld* f[4] = {&a.pt, &a.q1, &a.u, &a.v};
    for (int l = 1; l <= lm; ++l) {
      const size_t n = a.fld(col, l - 1);
      const double pk = a.S(S_PKZ, l - 1, col);
      for (int v = 0; v < 4; ++v) {
        T x(a.S(S_THO + v, l - 1, col));
        if constexpr (!std::is_same<T, double>::value) x.d = v == 0 ? f[0]->p[n] * a.p00k / pk : f[v]->p[n];
        V(E_THO + v).set(l, x);
      }
    }
    ras_column<T>(c, V);
    for (int l = 1; l <= lm; ++l) {
      const size_t n = a.fld(col, l - 1);
      const double pk = a.S(S_PKZ, l - 1, col);
      for (int v = 0; v < 4; ++v) {
        const T x = V(E_THO + v)(l);
        if constexpr (std::is_same<T, double>::value) f[v]->t[n] = v == 0 ? x * pk / a.p00k : x;
        else f[v]->p[n] = v == 0 ? x.d * pk / a.p00k : x.d;
      }
      if constexpr (!std::is_same<T, double>::value)
        for (int v = 0; v < 4; ++v) a.src[(size_t)v * a.ntile * lm * a.g.tx * a.g.ty + a.cmp(col, l - 1)] = V(E_CLW + v)(l).d;
    }
  }
};

// adjoint run: forward sweep in values with the checkpoints, then the segments last to first on the tape
struct RasAdFn {
  RasArgs a;
  HD void operator()(int m, int, int) const { FV3LM_LITERAL
    const size_t col = a.col_of(m); const int lm = a.lm, kw = a.kw();
    const RasCol c = a.column(m, col, 1);
    const int K = c.k, icmin = c.icmin;
    const ColWs tw{a.tw + m, (size_t)a.nb, kw}, ew{a.ew + m, (size_t)a.nb, kw}, ck{a.ck + m, (size_t)a.nb, kw};
    const ColWs eb{a.ew + (size_t)RAS_NT * kw * a.nb + m, (size_t)a.nb, kw};      // after the values' state and work vectors
    Tape tape; tape.m = a.tape; tape.col = (size_t)m; tape.n = 0;
    const LitVecs<double> EV{ew, nullptr};
    const LitVecs<RV> TV_{tw, &tape};
    const Fld* f[4] = {&a.pt, &a.q1, &a.u, &a.v};
    const size_t n3c = (size_t)a.ntile * lm * a.g.tx * a.g.ty;
    // values and incoming adjoints
    for (int v = 0; v < RAS_NE; ++v) for (int l = 0; l < kw; ++l) { ew.at(v, l) = 0.; eb.at(v, l) = 0.; }
    for (int l = 1; l <= lm; ++l) {
      const size_t n = a.fld(col, l - 1);
      const double pk = a.S(S_PKZ, l - 1, col);
      for (int v = 0; v < 4; ++v) {
        ew.at(E_THO + v, l) = a.S(S_THO + v, l - 1, col);
        eb.at(E_THO + v, l) = v == 0 ? f[0]->p[n] * pk / a.p00k : f[v]->p[n];
        eb.at(E_CLW + v, l) = a.src[(size_t)v * n3c + a.cmp(col, l - 1)];
      }
    }
    ras_pre<double>(c, EV);
    int nfired = 0;
    const int mut[5] = {E_POI, E_QOI, E_QST, E_UOI, E_VOI};
    for (int ic = K; ic >= icmin + 1; --ic) {
      for (int v = 0; v < 5; ++v) for (int l = 1; l <= lm; ++l) ck.at(5 * nfired + v, l) = ew.at(mut[v], l);
      if (ras_cloud<double>(c, EV, ic)) { ck.at(5 * lm, nfired) = (double)ic; ++nfired; }
    }
    if (nfired > 0) {      // otherwise the routine is the identity on the four fields and its sources are zero
      // one segment on the tape: every element of E a leaf, run, move the incoming adjoints onto the results, walk back
      auto segment = [&](int which, int ic) {
        tape.n = 0;
        for (int v = 0; v < RAS_NE; ++v) for (int l = 1; l <= lm; ++l) lit_leaf(tape, tw, ew, kw, v, l);
        if (which == 0) ras_pre<RV>(c, TV_); else if (which == 1) ras_cloud<RV>(c, TV_, ic); else ras_post<RV>(c, TV_, true);
        for (int v = 0; v < RAS_NE; ++v) for (int l = 1; l <= lm; ++l) lit_seed(tape, tw, eb, v, l);
        lit_walk_back(tape, eb, kw);
      };
      segment(2, 0);
      for (int s = nfired - 1; s >= 0; --s) {
        for (int v = 0; v < 5; ++v) for (int l = 1; l <= lm; ++l) ew.at(mut[v], l) = ck.at(5 * s + v, l);
        segment(1, (int)ck.at(5 * lm, s));
      }
      segment(0, 0);
    }
    for (int l = 1; l <= lm; ++l) {
      const size_t n = a.fld(col, l - 1);
      const double pk = a.S(S_PKZ, l - 1, col);
      for (int v = 0; v < 4; ++v) f[v]->p[n] = v == 0 ? eb.at(E_THO, l) * a.p00k / pk : eb.at(E_THO + v, l);
    }
  }
};

inline void run_ras(Exec& ex, int what, const RasArgs& a) {      // what: -2 gather, -1 set, 0 nl, 1 tl, 2 ad
  const Rect R{0, a.n - 1, 0, 0};
  if (a.n <= 0) return;
  if (what == -2) for_points(ex, R, 1, RasGatherFn{a}, "convection_gather");
  else if (what == -1) for_points(ex, R, 1, RasSetFn{a}, "convection_set");
  else if (what == MODE_NL) for_points(ex, R, 1, RasRunFn<double>{a}, "convection.nl");
  else if (what == MODE_TL) for_points(ex, R, 1, RasRunFn<RD>{a}, "convection.tl");
  else for_points(ex, R, 1, RasAdFn{a}, "convection.ad");
}

}  // namespace fv3
