// Host program of tests/test_remap_window_host.py (g++ -O2 -std=c++17 -DFV3LM_HOST_EMUL -I <csrc>): the column maps of csrc/remap.h, which keep
// the open source layer in registers and read every source level once per sweep, against the plain form they were derived from (below, kept
// verbatim under other names: every probe of the layer search, the found branch, the m loop and the adjoint's close_to load from the functors
// again).  Same arithmetic, so the comparison is memcmp: the outputs, every workspace vector that survives the call, the three adjoint
// output streams.  On ordered columns the functor calls are counted: that is what the windowed form exists for.
#include "remap.h"
#include <vector>

namespace fv3 {

// ------------------------------------------------------------------------------------------------ the plain form
template <class T, class FP1, class FQ1, class FP2, class FOut>
HD void plain_map_col(int km, const FP1& pe1, const FQ1& q1, const FP2& pe2, const FOut& out, const ColWs& ws, int SG, int SE) {
  typedef WsIO<T> W;
  // edge values by the tridiagonal solve
  T dpa = pe1(2) - pe1(1), dpb = pe1(3) - pe1(2);
  T grat = dpb / dpa;
  T bet = grat * (grat + 0.5);
  T qf = ((grat + grat) * (grat + 1.) * q1(1) + q1(2)) / bet;
  T gam = (1. + grat * (grat + 1.5)) / bet;
  W::set(ws, SE, 1, qf); W::set(ws, SG, 1, gam);
  T d4 = grat, a_prev = q1(1), dp_prev = dpa;
  for (int k = 2; k <= km; ++k) {
    T dpk = pe1(k + 1) - pe1(k);
    T ak_ = q1(k);
    d4 = dp_prev / dpk;
    bet = 2. + d4 + d4 - gam;
    qf = (3. * (a_prev + d4 * ak_) - qf) / bet;
    gam = d4 / bet;
    W::set(ws, SE, k, qf); W::set(ws, SG, k, gam);
    a_prev = ak_; dp_prev = dpk;
  }
  T a_bot = 1. + d4 * (d4 + 1.5);
  T qe = (2. * d4 * (d4 + 1.) * q1(km) + q1(km - 1) - a_bot * qf) / (d4 * (d4 + 0.5) - a_bot * gam);
  W::set(ws, SE, km + 1, qe);
  for (int k = km; k >= 1; --k) {
    qe = W::get(ws, SE, k) - W::get(ws, SG, k) * qe;
    W::set(ws, SE, k, qe);
  }
  // conservative mapping
  int k0 = 1;
  T qsum = T(0.);
  for (int k = 1; k <= km; ++k) {
    const T p2t = pe2(k), p2b = pe2(k + 1);
    int l; bool found = false;
    for (l = k0; l <= km; ++l)
      if (val(p2t) >= val(pe1(l)) && val(p2t) <= val(pe1(l + 1))) { found = true; break; }
    if (found) {
      const T p1l = pe1(l), p1r = pe1(l + 1), dpl = p1r - p1l;
      const T a1 = q1(l), a2 = W::get(ws, SE, l), a3 = W::get(ws, SE, l + 1), a4 = 3. * (2. * a1 - (a2 + a3));
      const T pl = (p2t - p1l) / dpl;
      if (val(p2b) <= val(p1r)) {
        const T pr = (p2b - p1l) / dpl;
        out(k, a2 + 0.5 * (a4 + a3 - a2) * (pr + pl) - a4 * R3 * (pr * (pr + pl) + pl * pl));
        k0 = l;
        continue;
      }
      qsum = (p1r - p2t) * (a2 + 0.5 * (a4 + a3 - a2) * (1. + pl) - a4 * (R3 * (1. + pl * (1. + pl))));
      int m; bool bottom = false;
      for (m = l + 1; m <= km; ++m) {
        if (val(p2b) > val(pe1(m + 1))) qsum = qsum + (pe1(m + 1) - pe1(m)) * q1(m);
        else { bottom = true; break; }
      }
      if (bottom) {
        const T p1m = pe1(m), dpm = pe1(m + 1) - p1m;
        const T b1 = q1(m), b2 = W::get(ws, SE, m), b3 = W::get(ws, SE, m + 1), b4 = 3. * (2. * b1 - (b2 + b3));
        const T dp = p2b - p1m, esl = dp / dpm;
        qsum = qsum + dp * (b2 + 0.5 * esl * (b3 - b2 + b4 * (1. - R23 * esl)));
        k0 = m;
      }
    }
    out(k, qsum / (p2b - p2t));
  }
}

template <class FP1, class FQ1, class FP2, class FE, class FOut>
HD void plain_map_loop_lim(const LimProfile& P, int km, const FP1& pe1, const FQ1& q1, const FP2& pe2, const FE& qe, const FOut& out) {
  int k0 = 1;
  double qsum = 0.;
  for (int k = 1; k <= km; ++k) {
    const double p2t = pe2(k), p2b = pe2(k + 1);
    int l; bool found = false;
    for (l = k0; l <= km; ++l)
      if (p2t >= pe1(l) && p2t <= pe1(l + 1)) { found = true; break; }
    if (found) {
      const double p1l = pe1(l), p1r = pe1(l + 1), dpl = p1r - p1l;
      double a2, a3, a4; lim_layer(P, l, km, q1, qe, a2, a3, a4);
      const double pl = (p2t - p1l) / dpl;
      if (p2b <= p1r) {
        const double pr = (p2b - p1l) / dpl;
        out(k, a2 + 0.5 * (a4 + a3 - a2) * (pr + pl) - a4 * R3 * (pr * (pr + pl) + pl * pl));
        k0 = l;
        continue;
      }
      qsum = (p1r - p2t) * (a2 + 0.5 * (a4 + a3 - a2) * (1. + pl) - a4 * (R3 * (1. + pl * (1. + pl))));
      int m; bool bottom = false;
      for (m = l + 1; m <= km; ++m) {
        if (p2b > pe1(m + 1)) qsum = qsum + (pe1(m + 1) - pe1(m)) * q1(m);
        else { bottom = true; break; }
      }
      if (bottom) {
        const double p1m = pe1(m), dpm = pe1(m + 1) - p1m;
        double b2, b3, b4; lim_layer(P, m, km, q1, qe, b2, b3, b4);
        const double dp = p2b - p1m, esl = dp / dpm;
        qsum = qsum + dp * (b2 + 0.5 * esl * (b3 - b2 + b4 * (1. - R23 * esl)));
        k0 = m;
      }
    }
    out(k, qsum / (p2b - p2t));
  }
}

template <class FP1, class FQ1, class FP2, class FAd, class OQ1, class OP1, class OP2>
HD void plain_map_col_ad_s(int km, const FP1& pe1, const FQ1& q1, const FP2& pe2, const FAd& q2_ad, const ColWs& ws, const MapAdWs& S,
                           const OQ1& q1out, const OP1& p1out, const OP2& p2out) {
  const double dp1_1 = pe1(2) - pe1(1), dp1_2 = pe1(3) - pe1(2);
  const double grat = dp1_2 / dp1_1, bet1 = grat * (grat + 0.5);
  double qbot;
  {   // ---- A
    double qf = ((grat + grat) * (grat + 1.) * q1(1) + q1(2)) / bet1, gam = (1. + grat * (grat + 1.5)) / bet1;
    ws.at(S.SF, 1) = qf; ws.at(S.SG, 1) = gam;
    double d4 = grat, a_prev = q1(1), dp_prev = dp1_1;
    for (int k = 2; k <= km; ++k) {
      const double dpk = pe1(k + 1) - pe1(k), ak_ = q1(k);
      d4 = dp_prev / dpk;
      const double bet = 2. + d4 + d4 - gam;
      qf = (3. * (a_prev + d4 * ak_) - qf) / bet;
      gam = d4 / bet;
      ws.at(S.SF, k) = qf; ws.at(S.SG, k) = gam;
      a_prev = ak_; dp_prev = dpk;
    }
    const double a_bot = 1. + d4 * (d4 + 1.5), den = d4 * (d4 + 0.5) - a_bot * gam;
    qbot = (2. * d4 * (d4 + 1.) * q1(km) + q1(km - 1) - a_bot * qf) / den;
  }
  {   // ---- B
    double qe = qbot;
    ws.at(S.SE, km + 1) = qe;
    for (int k = km; k >= 1; --k) { qe = ws.at(S.SF, k) - ws.at(S.SG, k) * qe; ws.at(S.SE, k) = qe; }
  }
  double fa_bot;
  {   // ---- C
    int b = 1;                                          // the open source level
    double aQ = 0., aD = 0., aP = 0., aPn = 0., aE = 0., aEn = 0.;   // q1_ad(b), dp1_ad(b), pe1_ad(b), pe1_ad(b+1), qe_ad(b), qe_ad(b+1)
    double ecarry = 0., dprev = 0.;                     // back-substitution carry into qe_ad(b); dp1_ad(b-1)
    // close levels b .. nb-1; the levels strictly between lo and hi lie wholly inside the current target (weight qsa)
    auto close_to = [&](int nb, int lo, int hi, double qsa) {
      while (b < nb) {
        const double e = aE + ecarry;
        ws.at(S.SFA, b) = e; ws.at(S.SGA, b) = -ws.at(S.SE, b + 1) * e; ecarry = -ws.at(S.SG, b) * e;
        ws.at(S.SQ, b) = aQ; ws.at(S.SP, b) = aP - aD + dprev; dprev = aD;
        ++b;
        const bool in = b > lo && b < hi;
        aQ = in ? (pe1(b + 1) - pe1(b)) * qsa : 0.; aD = in ? q1(b) * qsa : 0.;
        aP = aPn; aE = aEn; aPn = 0.; aEn = 0.;
      }
    };
    auto addq = [&](double a2_ad, double a3_ad, double a4_ad) {   // a4 = 3 (2 a1 - a2 - a3) of the open level
      aQ += 6. * a4_ad; aE += a2_ad - 3. * a4_ad; aEn += a3_ad - 3. * a4_ad;
    };
    double p2k = 0., p2k1 = 0.;      // pending pe2_ad(k), pe2_ad(k+1)
    for (int k = 1; k <= km; ++k) {
      if (k > 1) p2out(k - 1, p2k);
      p2k = p2k1; p2k1 = 0.;
      const double g = q2_ad(k);
      const double p2t = pe2(k), p2b = pe2(k + 1);
      int l; bool found = false;
      for (l = b; l <= km; ++l)
        if (p2t >= pe1(l) && p2t <= pe1(l + 1)) { found = true; break; }
      if (!found) continue;   // (stale-qsum path of the reference: never taken for ordered pressures)
      close_to(l, 0, 0, 0.);
      const double p1l = pe1(l), p1r = pe1(l + 1), dpl = p1r - p1l;
      const double a1 = q1(l), a2 = ws.at(S.SE, l), a3 = ws.at(S.SE, l + 1), a4 = 3. * (2. * a1 - (a2 + a3)), Sm = a4 + a3 - a2;
      const double pl = (p2t - p1l) / dpl;
      if (p2b <= p1r) {
        const double pr = (p2b - p1l) / dpl, s = pr + pl, w = pr * s + pl * pl;
        addq((1. - 0.5 * s) * g, 0.5 * s * g, (0.5 * s - R3 * w) * g);
        const double pr_ad = (0.5 * Sm - a4 * R3 * (2. * pr + pl)) * g, pl_ad = (0.5 * Sm - a4 * R3 * (pr + 2. * pl)) * g;
        p2k1 += pr_ad / dpl; aP -= pr_ad / dpl; aD -= pr * pr_ad / dpl;
        p2k += pl_ad / dpl; aP -= pl_ad / dpl; aD -= pl * pl_ad / dpl;
        continue;
      }
      const double D = p2b - p2t;
      const double E = a2 + 0.5 * Sm * (1. + pl) - a4 * (R3 * (1. + pl * (1. + pl)));
      double qsum = (p1r - p2t) * E;
      int m; bool bottom = false;
      for (m = l + 1; m <= km; ++m) {
        if (p2b > pe1(m + 1)) qsum += (pe1(m + 1) - pe1(m)) * q1(m);
        else { bottom = true; break; }
      }
      double dp = 0., esl = 0., Fm = 0., b2 = 0., b3 = 0., b4 = 0., dpm = 1.;
      if (bottom) {
        const double p1m = pe1(m); dpm = pe1(m + 1) - p1m;
        const double b1 = q1(m); b2 = ws.at(S.SE, m); b3 = ws.at(S.SE, m + 1); b4 = 3. * (2. * b1 - (b2 + b3));
        dp = p2b - p1m; esl = dp / dpm;
        Fm = b2 + 0.5 * esl * (b3 - b2 + b4 * (1. - R23 * esl));
        qsum += dp * Fm;
      }
      const double q2v = qsum / D, qs_ad = g / D, D_ad = -q2v * g / D;
      p2k1 += D_ad; p2k -= D_ad;
      const double W_ad = E * qs_ad, E_ad = (p1r - p2t) * qs_ad;
      aPn += W_ad; p2k -= W_ad;
      addq((1. - 0.5 * (1. + pl)) * E_ad, 0.5 * (1. + pl) * E_ad, (0.5 * (1. + pl) - R3 * (1. + pl * (1. + pl))) * E_ad);
      const double pl_ad = (0.5 * Sm - a4 * R3 * (1. + 2. * pl)) * E_ad;
      p2k += pl_ad / dpl; aP -= pl_ad / dpl; aD -= pl * pl_ad / dpl;
      if (bottom) {
        close_to(m, l, m, qs_ad);
        double dp_ad = Fm * qs_ad;
        const double F_ad = dp * qs_ad;
        addq((1. - 0.5 * esl) * F_ad, 0.5 * esl * F_ad, 0.5 * esl * (1. - R23 * esl) * F_ad);
        const double esl_ad = (0.5 * (b3 - b2 + b4 * (1. - R23 * esl)) - 0.5 * esl * b4 * R23) * F_ad;
        dp_ad += esl_ad / dpm; aD -= esl * esl_ad / dpm;
        p2k1 += dp_ad; aP -= dp_ad;
      } else {
        close_to(km + 1, l, km + 1, qs_ad);     // the target reaches below the last source layer: nothing further is found
      }
    }
    p2out(km, p2k); p2out(km + 1, p2k1);
    close_to(km + 1, 0, 0, 0.);
    fa_bot = aE + ecarry;                   // adjoint of the bottom edge value
    ws.at(S.SP, km + 1) = aP + dprev;
  }
  {   // ---- D
    double dpk = pe1(km + 1) - pe1(km), dpm1 = pe1(km) - pe1(km - 1);
    double d4 = dpm1 / dpk, gam_k = ws.at(S.SG, km);
    double sfa, sga, sda, qpk, qpkm1, dpend = 0., dnext = 0., q2hold = 0., d2loop = 0.;
    {
      const double d = d4, qfk = ws.at(S.SF, km);
      const double a_bot = 1. + d * (d + 1.5), den = d * (d + 0.5) - a_bot * gam_k;
      const double numb_ad = fa_bot / den, den_ad = -qbot * fa_bot / den;
      double d_ad = 2. * (2. * d + 1.) * q1(km) * numb_ad + (2. * d + 0.5) * den_ad;
      qpk = 2. * d * (d + 1.) * numb_ad; qpkm1 = numb_ad;
      const double abot_ad = -qfk * numb_ad - gam_k * den_ad;
      sfa = ws.at(S.SFA, km) - a_bot * numb_ad;
      sga = ws.at(S.SGA, km) - a_bot * den_ad;
      d_ad += (2. * d + 1.5) * abot_ad;
      sda = d_ad;
    }
    for (int k = km; k >= 2; --k) {
      const double gam = gam_k, gam_km1 = ws.at(S.SG, k - 1), qf = ws.at(S.SF, k);
      const double bet = 2. + d4 + d4 - gam_km1;
      gam_k = gam_km1;
      double d4_ad = sda + sga / bet;
      double bet_ad = -gam * sga / bet;
      const double t = sfa / bet;
      const double qk = ws.at(S.SQ, k) + qpk + 3. * d4 * t;
      if (k > 2) q1out(k, qk); else q2hold = qk;
      qpk = qpkm1 + 3. * t; qpkm1 = 0.;
      d4_ad += 3. * q1(k) * t;
      bet_ad -= qf * t;
      d4_ad += 2. * bet_ad;
      sfa = ws.at(S.SFA, k - 1) - t;
      sga = ws.at(S.SGA, k - 1) - bet_ad;
      sda = 0.;
      const double dk = dpend - d4 * d4_ad / dpk;       // dp1_ad(k) of this sweep
      dpend = d4_ad / dpk;
      if (k > 2) { p1out(k + 1, ws.at(S.SP, k + 1) + dk - dnext); dnext = dk; } else d2loop = dk;
      dpk = dpm1;
      if (k > 2) { dpm1 = pe1(k - 1) - pe1(k - 2); d4 = dpm1 / dpk; }
    }
    {
      const double gam1 = gam_k, qf1 = ws.at(S.SF, 1);
      double grat_ad = (2. * grat + 1.5) / bet1 * sga;
      double bet_ad = -gam1 * sga / bet1;
      const double t = sfa / bet1;
      bet_ad -= qf1 * t;
      grat_ad += 2. * (2. * grat + 1.) * q1(1) * t;
      q1out(2, q2hold + t);
      q1out(1, ws.at(S.SQ, 1) + qpk + 2. * grat * (grat + 1.) * t);
      grat_ad += (2. * grat + 0.5) * bet_ad;
      const double d2 = d2loop + grat_ad / dp1_1, d1 = dpend - grat * grat_ad / dp1_1;
      p1out(3, ws.at(S.SP, 3) + d2 - dnext);
      p1out(2, ws.at(S.SP, 2) + d1 - d2);
      p1out(1, ws.at(S.SP, 1) - d1);
    }
  }
}

}  // namespace fv3

using namespace fv3;

// ------------------------------------------------------------------------------------------------ columns
struct Rng {      // 48-bit linear congruential generator: the columns are the same on every machine
  unsigned long long s;
  double u() { s = (s * 0x5DEECE66DULL + 0xBULL) & ((1ULL << 48) - 1); return double(s >> 16) / double(1ULL << 32); }
  double pm() { return 2. * u() - 1.; }
};
struct Column {
  int km; bool ordered;
  std::vector<double> pe1, pe2, q, pt, pk, ga, pe1d, qd, pe2d;      // 1-based; q: layer means, pt / pk: the T map's factors, ga: output adjoints, *d: tangents
};
enum Kind { SMALL, LARGE, TIES, TOP_ABOVE, BOTTOM_BELOW, NKIND };
static const char* kind_name[] = {"small", "large", "ties", "top_above", "bottom_below"};

static Column make_column(int km, Kind kind, unsigned seed) {
  Column c; c.km = km; c.ordered = kind <= TIES;
  Rng r{seed * 7919ULL + 12345ULL};
  const double ptop = 1., ps = 1.0e5 * (1. + 0.02 * r.pm());
  c.pe1.assign(km + 2, 0.); c.pe2 = c.pe1; c.pe1d = c.pe1; c.pe2d = c.pe1;
  c.q.assign(km + 2, 0.); c.pt = c.q; c.ga = c.q; c.qd = c.q; c.pk.assign(km + 3, 0.);
  for (int k = 1; k <= km + 1; ++k) { const double x = double(k - 1) / km; c.pe2[k] = ptop + (ps - ptop) * x * x * (0.4 + 0.6 * x); }
  c.pe2[km + 1] = ps;
  auto at = [&](double xi) { const int k0 = std::min(int(xi), km - 1); return c.pe2[k0 + 1] + (xi - k0) * (c.pe2[k0 + 2] - c.pe2[k0 + 1]); };   // xi in target layers
  if (kind == LARGE) {      // ten sources in the first target, one source over ten targets (the 'large' warp of tests/remap_checks.py)
    std::vector<double> inc;
    for (int n = 0; n < 10; ++n) inc.push_back(0.1);
    for (int n = 0; n < (km - 11) / 2; ++n) inc.push_back(1.);
    inc.push_back(10.);
    for (int n = 0; n < km - 11 - (km - 11) / 2; ++n) inc.push_back(1.);
    double tot = 0.; for (double x : inc) tot += x;
    double xi = 0.;
    for (int k = 1; k <= km + 1; ++k) { c.pe1[k] = at(xi * km / tot); if (k <= km) xi += inc[k - 1]; }
  } else if (kind == TIES) {      // every second interface is a target interface, bit for bit; the others sit up to 30 % of a layer off
    for (int k = 1; k <= km + 1; ++k) c.pe1[k] = (k % 2 == 1 || k == km + 1) ? c.pe2[k] : at(k - 1 + 0.3 * r.pm());
  } else {      // source layers within 3 % of the target ones
    std::vector<double> d(km + 1, 0.); double tot = 0.;
    for (int k = 1; k <= km; ++k) { d[k] = (c.pe2[k + 1] - c.pe2[k]) * (1. + 0.03 * r.pm()); tot += d[k]; }
    c.pe1[1] = ptop;
    for (int k = 1; k <= km; ++k) c.pe1[k + 1] = c.pe1[k] + d[k] * (ps - ptop) / tot;
  }
  c.pe1[1] = ptop; c.pe1[km + 1] = ps;
  if (kind == TOP_ABOVE) c.pe1[1] = ptop + 0.4 * (c.pe1[2] - ptop);                       // the first target starts above every source layer: not found
  if (kind == BOTTOM_BELOW) c.pe1[km + 1] = ps - 0.4 * (ps - c.pe1[km]);                  // the last target ends below the last source interface: no bottom
  for (int k = 1; k <= km + 1; ++k) { c.pk[k] = std::exp(0.2857 * std::log(c.pe1[k])); c.pe1d[k] = 1e-3 * c.pe1[k] * r.pm(); c.pe2d[k] = 1e-3 * c.pe2[k] * r.pm(); }
  for (int k = 1; k <= km; ++k) { c.q[k] = 1. + 0.5 * r.pm(); c.pt[k] = 200. + 90. * r.u(); c.ga[k] = r.pm(); c.qd[k] = 0.1 * r.pm(); }
  return c;
}

// ------------------------------------------------------------------------------------------------ comparison
static int failures = 0;
static void expect(bool ok, const char* what, const Column& c, int kind, long a = 0, long b = 0) {
  if (ok) return;
  ++failures;
  std::printf("FAIL %s: km = %d, column %s (%ld, %ld)\n", what, c.km, kind_name[kind], a, b);
}
static bool same(const std::vector<double>& a, const std::vector<double>& b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0; }
// slot s of a workspace of kw levels (stride 1)
static std::vector<double> slot(const std::vector<double>& w, int kw, int s) { return std::vector<double>(w.begin() + (size_t)s * kw, w.begin() + (size_t)(s + 1) * kw); }

static const int NSLOT = 12;
struct Work {
  std::vector<double> w; ColWs ws;
  explicit Work(int km) : w((size_t)NSLOT * (km + 2)) { for (size_t n = 0; n < w.size(); ++n) w[n] = -7.25 - double(n); ws = ColWs{w.data(), 1, km + 2}; }
};

static void run(int km, int kind) {
  const Column c = make_column(km, Kind(kind), 100 * kind + km);
  const int kw = km + 2;
  long np = 0, nq = 0;
  auto pe1 = [&](int k) { ++np; return c.pe1[k]; };
  auto q1 = [&](int k) { ++nq; return c.q[k]; };
  auto pe2 = [&](int k) { return c.pe2[k]; };
  {   // forward, double: slots SG 0, SE 1 (, layer means 2)
    Work A(km), B(km), C(km);
    std::vector<double> oa(kw, 0.), ob(kw, 0.), oc(kw, 0.);
    plain_map_col<double>(km, pe1, q1, pe2, [&](int k, double x) { oa[k] = x; }, A.ws, 0, 1);
    np = nq = 0;
    map_col<double>(km, pe1, q1, pe2, [&](int k, double x) { ob[k] = x; }, B.ws, 0, 1, 2);
    const long np_w = np, nq_w = nq;
    map_col<double>(km, pe1, q1, pe2, [&](int k, double x) { oc[k] = x; }, C.ws, 0, 1);
    expect(same(oa, ob) && same(oa, oc), "forward outputs", c, kind);
    for (int s : {0, 1}) expect(same(slot(A.w, kw, s), slot(B.w, kw, s)) && same(slot(A.w, kw, s), slot(C.w, kw, s)), "forward workspace", c, kind, s);
    for (int s = 3; s < NSLOT; ++s) expect(same(slot(A.w, kw, s), slot(B.w, kw, s)), "forward: a slot not its own", c, kind, s);
    for (int k = 1; k <= km; ++k) expect(B.ws.at(2, k) == c.q[k], "forward layer means", c, kind, k);
    if (c.ordered) expect(np_w <= 2 * (km + 1) + 8 && nq_w <= km + 8, "forward functor calls", c, kind, np_w, nq_w);
    if (kind == SMALL) std::printf("km %3d  forward   pe1 %ld  q1 %ld  (one read per level and sweep: %d, %d)\n", km, np_w, nq_w, 2 * (km + 1), km);
  }
  {   // forward, Dual
    auto pe1D = [&](int k) { return Dual(c.pe1[k], c.pe1d[k]); };
    auto q1D = [&](int k) { return Dual(c.q[k], c.qd[k]); };
    auto pe2D = [&](int k) { return Dual(c.pe2[k], c.pe2d[k]); };
    Work A(km), B(km);
    std::vector<double> oa(2 * kw, 0.), ob(2 * kw, 0.);
    plain_map_col<Dual>(km, pe1D, q1D, pe2D, [&](int k, const Dual& x) { oa[2 * k] = x.v; oa[2 * k + 1] = x.d; }, A.ws, 0, 1);
    map_col<Dual>(km, pe1D, q1D, pe2D, [&](int k, const Dual& x) { ob[2 * k] = x.v; ob[2 * k + 1] = x.d; }, B.ws, 0, 1, 2);
    expect(same(oa, ob), "forward Dual outputs", c, kind);
    for (int s = 0; s < 4; ++s) expect(same(slot(A.w, kw, s), slot(B.w, kw, s)), "forward Dual workspace", c, kind, s);
  }
  {   // the T map: T_v from pt, pk and the coordinate, as a plain functor and as the one that builds on the sweep's interfaces
    const double akap = 0.2857;
    std::vector<double> pn(kw, 0.), pn2(kw, 0.);
    for (int k = 1; k <= km + 1; ++k) { pn[k] = std::log(c.pe1[k]); pn2[k] = std::log(c.pe2[k]); }
    auto pn1 = [&](int k) { return pn[k]; };
    auto pn2f = [&](int k) { return pn2[k]; };
    auto tv = [&](int k) { return c.pt[k] * (c.pk[k + 1] - c.pk[k]) / (akap * (pn[k + 1] - pn[k])); };
    long ntv = 0; double pk_hi = c.pk[1];
    auto tvs = [&](int k, const double& p_k, const double& p_k1) { ++ntv; const double pk_lo = c.pk[k + 1]; const double t = c.pt[k] * (pk_lo - pk_hi) / (akap * (p_k1 - p_k)); pk_hi = pk_lo; return t; };
    Work A(km), B(km);
    std::vector<double> oa(kw, 0.), ob(kw, 0.);
    plain_map_col<double>(km, pn1, tv, pn2f, [&](int k, double x) { oa[k] = x; }, A.ws, 0, 1);
    map_col<double>(km, pn1, tvs, pn2f, [&](int k, double x) { ob[k] = x; }, B.ws, 0, 1, 2);
    expect(same(oa, ob), "T map outputs", c, kind);
    for (int s : {0, 1}) expect(same(slot(A.w, kw, s), slot(B.w, kw, s)), "T map workspace", c, kind, s);
    expect(ntv == km, "T map: T_v once per level", c, kind, ntv);
  }
  for (int kord : {9, 10, 11}) for (int iv : {-1, 0, 1}) {   // the limited profiles: the same loop through the window
    const LimProfile P{kord, iv, iv != -1, iv == 1 ? 1.2 : 0.};
    Work A(km), B(km);
    std::vector<double> oa(kw, 0.), ob(kw, 0.);
    auto qc = [&](int k) { return c.q[k]; };
    plain_map_col<double>(km, pe1, q1, pe2, [&](int, double) {}, A.ws, 0, 1);      // the edge values
    auto qe = [&](int k) { return A.ws.at(1, k); };
    plain_map_loop_lim(P, km, pe1, qc, pe2, qe, [&](int k, double x) { oa[k] = x; });
    map_col_lim(P, km, pe1, q1, pe2, [&](int k, double x) { ob[k] = x; }, B.ws, 0, 1, 2);
    expect(same(oa, ob), "limited outputs", c, kind, kord, iv);
    std::fill(ob.begin(), ob.end(), 0.);
    map_col_lim(P, km, pe1, q1, pe2, [&](int k, double x) { ob[k] = x; }, B.ws, 0, 1);
    expect(same(oa, ob), "limited outputs (no slot)", c, kind, kord, iv);
  }
  {   // adjoint: slots SG 0, SF 1, SE 2, SFA 3, SGA 4, SQ 5, SP 6
    const MapAdWs S{0, 1, 2, 3, 4, 5, 6};
    auto ga = [&](int k) { return c.ga[k]; };
    Work A(km), B(km);
    std::vector<double> qa(kw, 0.), pa(kw, 0.), ta(kw, 0.), qb(kw, 0.), pb(kw, 0.), tb(kw, 0.);
    plain_map_col_ad_s(km, pe1, q1, pe2, ga, A.ws, S, [&](int k, double x) { qa[k] = x; }, [&](int k, double x) { pa[k] = x; }, [&](int k, double x) { ta[k] = x; });
    np = nq = 0;
    map_col_ad_s(km, pe1, q1, pe2, ga, B.ws, S, [&](int k, double x) { qb[k] = x; }, [&](int k, double x) { pb[k] = x; }, [&](int k, double x) { tb[k] = x; });
    expect(same(qa, qb), "adjoint q1_ad", c, kind);
    expect(same(pa, pb), "adjoint pe1_ad", c, kind);
    expect(same(ta, tb), "adjoint pe2_ad", c, kind);
    expect(same(A.w, B.w), "adjoint workspace", c, kind);
    if (c.ordered) expect(np <= 3 * (km + 1) + 8 && nq <= 3 * km + 8, "adjoint functor calls", c, kind, np, nq);
    if (kind == SMALL) std::printf("km %3d  adjoint   pe1 %ld  q1 %ld  (one read per level and sweep: %d, %d)\n", km, np, nq, 3 * (km + 1), 3 * km);
  }
}

int main() {
  for (int km : {12, 127})
    for (int kind = 0; kind < NKIND; ++kind) run(km, kind);
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("remap window: all columns bit-identical to the plain form\n");
  return 0;
}
