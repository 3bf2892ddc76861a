// fv3lm-hip: linearised boundary-layer turbulence (physics/turbulence/fv3jedi_lm_turbulence_mod.F90): a vertical diffusion of the
// perturbation with coefficients frozen on the trajectory -- three tridiagonal systems per column, V (u, v), S (potential temperature) and
// Q (q1 .. q_nq), factorised once per trajectory time (VTRILUPERT :583-601) and solved for the seven fields per step (VTRISOLVEPERT
// :605-674; step_nl :151-214 on the trajectory, step_tl :218-282, step_ad :286-350 on the perturbation).  Column-local: only
// is..ie x js..je of a resident tile is read or written (the reference's arrays are compact), delp, w, delz are not touched.
//
// A SLOT (one per trajectory time the host keeps, saveltraj ? nt : 1) is ten arrays [ntile][npz][pj][pi] in the padded-plane layout:
//   0..8  AKV BKV CKV  AKS BKS CKS  AKQ BKQ CKQ   lower / main / upper diagonal; after factorise A holds the multipliers of L, B the
//                                                  INVERSE of the main diagonal of U, C is unchanged
//   9     pk = (pe^kappa(l) - pe^kappa(l-1)) / (kappa (ln pe(l) - ln pe(l-1))), pe(0) = ptop, pe(l) = pe(l-1) + delp(l)
//         (compute_pressures, utils/fv3jedi_lm_utils_mod.F90:359-391), of the trajectory delp resident when the slot was set;
//         evaluated without the cancellation of the two differences (turb_layer).
//
// Kernels: one thread per column, i fastest (every load and store of a level is one contiguous row piece per wave), launched with
// for_points over is..ie x js..je; the independent systems are a launch dimension (z = tile * 3 + system), not a loop in the thread.
//   factorise  z = tile * 4 + s: s < 3 VTRILUPERT of system s, s = 3 pk (pe accumulated in the thread, never stored).  A pivot or
//              factor that is zero or not finite raises one flag, which the host reads (fv3lm_turbulence_set_diagonals refuses).
//   solve      all fields of a system in one pass over its factors.  Two sweeps in place: the first stores its intermediate into the
//              field, the second reads it back; a thread carries only y(l-1) / y(l+1) of each field -- no work array per thread, no
//              global workspace.  T <-> theta (p00^kappa T / pk and back) is folded into the first load and the last store of a level.
//              The last level takes b(lm) (ygswitch = 1: u v T q1) or b(lm-1) / (b(lm-1) - a(lm) (1 + c(lm-1) b(lm-1))) (ygswitch = 0:
//              q2 ..); with that one factor both switches are the same two sweeps, and the adjoint is their transpose written by hand:
//              U' down, the factor, L' up (:644-652; :656-668 is the same matrix).  NL and TL are one code on which = 0 / 1.
//   blsimp     BL_simp (turbulence/blsimp.F90) on the trajectory, written straight into the nine diagonals of the slot.  The routine has
//              no caller in the reference; its arguments are read as PTT = T / pk, PKT = pk -- the reading under which PTT PKT is a
//              temperature and PKH - PKT a difference of like quantities -- UT, VT the D-grid winds at (i, j), QVT QLT QIT = q1 q2 q3,
//              PET = pe(0:lm), and the constants the JEDI set of the options: MAPL_GRAV = grav_jedi, MAPL_KAPPA = akap, MAPL_CP = cp,
//              MAPL_RGAS = cp akap, MAPL_VIREPS = zvir.  Both branches of KH meet at RI = 0: the unit is continuous in its inputs.
//
// Byte model per point (column x level), 8 B words.  Algorithmic (profile lines): the 9 factor arrays and pk read once, each of the
// 3 + nq fields read and written once = (10 + 2 (3 + nq)) 8 B (192 B at nq = 4).  The two-sweep in-place form built here re-reads and
// re-writes the fields between the sweeps and reads pk in both: (3 + 6 + 2 + 4 (3 + nq)) 8 B (312 B at nq = 4).  Holding the column on
// chip between the sweeps instead would need npz x fields x 8 B per THREAD (4 kB for the Q system at L127, 260 kB per wave -- more than
// the 160 kB of LDS of a CU), so it is not built.
#pragma once
#include "column.h"
#include "remap.h"

namespace fv3 {

constexpr int TURB_MAXQ = 8;
constexpr int TURB_NARR = 10;     // arrays of a slot
enum { TURB_V = 0, TURB_S = 1, TURB_Q = 2 };

struct TurbArgs {
  Geom g;
  Fld u, v, pt, delp, q[TURB_MAXQ]; int nq;
  double* fac; size_t fs;         // the slot: array n at fac + n fs, [ntile][npz][plane]
  const double* fro;              // FROCEAN, [ntile][plane] (blsimp)
  int* flag;                      // factorise: raised on a zero or non-finite pivot / factor
  double ptop, akap, p00k;        // p00^kappa
  double dt, grav, cp, zvir;      // blsimp
  HD size_t col(int t, int i, int j) const { return (size_t)t * g.npz * g.plane + g.idx(i, j); }
};

// Inf or NaN (exponent all ones) in a factor as it was STORED: the library is built with -ffinite-math-only, under which the compiler may
// take the result of an arithmetic operation for finite and fold a test of it away; a value read back through a volatile pointer
// carries no such assumption.
HD bool turb_stored_nonfinite(const double* p) {
  const double x = *(const volatile double*)p;
  std::uint64_t b; __builtin_memcpy(&b, &x, 8);
  return ((b >> 52) & 0x7ffu) == 0x7ffu;
}

// One layer between the edge pressures pe0 (top) and pe1: x = kappa ln(pe1 / pe0), g = (e^x - 1) / x - 1, k0 = pe0^kappa.  The
// reference's pk, the quotient (pe1^kappa - pe0^kappa) / (kappa (ln pe1 - ln pe0)), is k0 (1 + g): the same number, evaluated through
// log1p and the series of g so that the two differences do not cancel -- in a thin layer (x ~ 4e-3 at L127) the quotient of
// differences loses 1 / x of the precision of pow and log.  BL_simp differences pk and theta = T / pk of neighbouring layers once
// more (DZ, RI); written with x and g those differences do not cancel either (TurbSimpleFn), where the literal form in double is
// good to 2e-10 of the largest coefficient only (measured against an evaluation in extended precision, 12 x 10 x L127).
struct TurbLayer { double x, g, k0, pk; };
HD double turb_g(double x) {      // x / 2 + x^2 / 6 + x^3 / 24 + ...
  if (fabs(x) >= 0.5) return (expm1(x) - x) / x;
  double s = 1.;
  for (int n = 18; n >= 3; --n) s = 1. + x / n * s;
  return 0.5 * x * s;
}
HD TurbLayer turb_layer(double pe0, double pe1, double akap) {
  TurbLayer y;
  y.x = akap * log1p((pe1 - pe0) / pe0); y.g = turb_g(y.x); y.k0 = pow(pe0, akap); y.pk = y.k0 * (1. + y.g);
  return y;
}

struct TurbFactorFn {
  TurbArgs a;
  HD void operator()(int i, int j, int z) const {
    const int t = z / 4, s = z % 4, lm = a.g.npz; const size_t pl = a.g.plane, o = a.col(t, i, j);
    if (s == 3) {
      double* PK = a.fac + 9 * a.fs + o; const double* dp = a.delp.t + o;
      double pe0 = a.ptop;
      for (int l = 0; l < lm; ++l) { const double pe1 = pe0 + dp[(size_t)l * pl]; PK[(size_t)l * pl] = turb_layer(pe0, pe1, a.akap).pk; pe0 = pe1; }
      return;
    }
    double* A = a.fac + (3 * s) * a.fs + o; double* B = A + a.fs; const double* C = B + a.fs;
    double bi = 1. / B[0];
    B[0] = bi;
    bool bad = turb_stored_nonfinite(B);          // a zero pivot leaves Inf, a NaN anywhere above travels down the column
    for (int l = 1; l < lm; ++l) {
      const size_t m = (size_t)l * pl;
      const double al = A[m] * bi;
      bi = 1. / (B[m] - C[m - pl] * al);
      A[m] = al; B[m] = bi;
      bad = bad || turb_stored_nonfinite(A + m) || turb_stored_nonfinite(B + m);
    }
    if (bad) *a.flag = 1;
  }
};

// The two sweeps of one system over its nf fields f[] (base pointers of the column); yg[n]: ygswitch of field n; theta: the field is a
// temperature (S system); adj: the transpose.
template <int MAXF>
HD void turb_solve_col(const TurbArgs& a, size_t o, int sys, int nf, double* const (&f)[MAXF], const bool (&yg)[MAXF], bool theta, bool adj) {
  const int lm = a.g.npz; const size_t pl = a.g.plane;
  const double* A = a.fac + (3 * sys) * a.fs + o; const double* B = A + a.fs; const double* C = B + a.fs; const double* PK = a.fac + 9 * a.fs + o;
  const double p00k = a.p00k;
  // T -> theta on the way in, theta -> T on the way out (step_tl :258, :269); the adjoint the other way round (step_ad :326, :337)
  auto in = [&](double x, size_t m) { if (!theta) return x; const double pk = PK[m]; return adj ? pk * x / p00k : p00k * x / pk; };
  auto out = [&](double x, size_t m) { if (!theta) return x; const double pk = PK[m]; return adj ? p00k * x / pk : pk * x / p00k; };
  const size_t mb = (size_t)(lm - 1) * pl;        // the last level
  const double bm = B[mb - pl], cm = C[mb - pl], am = A[mb];
  const double last1 = B[mb], last0 = bm / (bm - am * (1. + cm * bm));
  double y[MAXF];
  if (!adj) {
    // sweep down with the multipliers a (:624-626)
#pragma unroll
    for (int n = 0; n < MAXF; ++n) if (n < nf) { y[n] = in(f[n][0], 0); if (theta) f[n][0] = y[n]; }
    for (int l = 1; l < lm; ++l) {
      const size_t m = (size_t)l * pl; const double al = A[m];
#pragma unroll
      for (int n = 0; n < MAXF; ++n) if (n < nf) { y[n] = in(f[n][m], m) - al * y[n]; if (l < lm - 1) f[n][m] = y[n]; }
    }
#pragma unroll
    for (int n = 0; n < MAXF; ++n) if (n < nf) { y[n] = y[n] * (yg[n] ? last1 : last0); f[n][mb] = out(y[n], mb); }      // :629-633
    // sweep up with b (the inverse main diagonal) and c (:635-637)
    for (int l = lm - 2; l >= 0; --l) {
      const size_t m = (size_t)l * pl; const double bl = B[m], cl = C[m];
#pragma unroll
      for (int n = 0; n < MAXF; ++n) if (n < nf) { y[n] = bl * (f[n][m] - cl * y[n]); f[n][m] = out(y[n], m); }
    }
  } else {
    // U' down (:644-647), with the last level's factor in the place of b(lm)
    { const double b0 = B[0];
#pragma unroll
      for (int n = 0; n < MAXF; ++n) if (n < nf) { y[n] = in(f[n][0], 0) * b0; f[n][0] = y[n]; } }
    for (int l = 1; l < lm - 1; ++l) {
      const size_t m = (size_t)l * pl; const double bl = B[m], cl = C[m - pl];
#pragma unroll
      for (int n = 0; n < MAXF; ++n) if (n < nf) { y[n] = bl * (in(f[n][m], m) - cl * y[n]); f[n][m] = y[n]; }
    }
#pragma unroll
    for (int n = 0; n < MAXF; ++n) if (n < nf) { y[n] = (yg[n] ? last1 : last0) * (in(f[n][mb], mb) - cm * y[n]); f[n][mb] = out(y[n], mb); }
    // L' up (:650-652)
    for (int l = lm - 2; l >= 0; --l) {
      const size_t m = (size_t)l * pl; const double an = A[m + pl];
#pragma unroll
      for (int n = 0; n < MAXF; ++n) if (n < nf) { y[n] = f[n][m] - an * y[n]; f[n][m] = out(y[n], m); }
    }
  }
}

struct TurbSolveFn {
  TurbArgs a; int mode;
  HD void operator()(int i, int j, int z) const {
    const int t = z / 3, sys = z % 3; const size_t o = a.col(t, i, j);
    const bool adj = mode == MODE_AD;
    auto p = [&](const Fld& fl) { return (mode == MODE_NL ? fl.t : fl.p) + o; };
    if (sys == TURB_V) {
      double* const f[2] = {p(a.u), p(a.v)}; const bool yg[2] = {true, true};
      turb_solve_col<2>(a, o, TURB_V, 2, f, yg, false, adj);
    } else if (sys == TURB_S) {
      double* const f[1] = {p(a.pt)}; const bool yg[1] = {true};
      turb_solve_col<1>(a, o, TURB_S, 1, f, yg, true, adj);
    } else if (a.nq > 0) {
      double* const f[TURB_MAXQ] = {p(a.q[0]), p(a.q[1]), p(a.q[2]), p(a.q[3]), p(a.q[4]), p(a.q[5]), p(a.q[6]), p(a.q[7])};
      const bool yg[TURB_MAXQ] = {true, false, false, false, false, false, false, false};
      turb_solve_col<TURB_MAXQ>(a, o, TURB_Q, a.nq, f, yg, false, adj);
    }
  }
};

// BL_simp (blsimp.F90:72-133) of one column, z = tile.  Level l (1-based) of the loop below is the reference's L; the values of level
// L-1 are carried.  AKS(1) = 0 and CKS(LM) = 0; the three systems share a, c and b above the surface and differ in b(LM).  The
// formulas are the routine's; its differences of neighbouring pk and theta are written through x and g of the layers (turb_layer).
struct TurbSimpleFn {
  TurbArgs a;
  HD void operator()(int i, int j, int t) const {
    const int lm = a.g.npz; const size_t pl = a.g.plane, o = a.col(t, i, j);
    const double grav = a.grav, kap = a.akap, cp = a.cp, rgas = a.cp * a.akap, eps = a.zvir;
    const double* U = a.u.t + o; const double* V = a.v.t + o; const double* T = a.pt.t + o; const double* DP = a.delp.t + o;
    const double* QV = a.q[0].t + o; const double* QL = a.q[1].t + o; const double* QI = a.q[2].t + o;
    auto put = [&](int which, size_t m, double x) { for (int s = 0; s < 3; ++s) a.fac[(3 * s + which) * a.fs + o + m] = x; };
    const double pe0 = a.ptop;
    double pe1 = pe0 + DP[0];
    TurbLayer lp = turb_layer(pe0, pe1, kap);      // layer l - 1
    double t_p = T[0], u_p = U[0], v_p = V[0];
    double tvt = t_p * (1.0 + eps * QV[0] - QL[0] - QI[0]);      // PTT PKT = T
    double dmi = (grav * a.dt) / (pe1 - pe0);
    double a_prev = 0.;
    put(0, 0, 0.);
    for (int l = 2; l <= lm; ++l) {
      const size_t m = (size_t)(l - 1) * pl;
      const double pe = pe1 + DP[m];
      const TurbLayer lc = turb_layer(pe1, pe, kap);
      const double pk = lc.pk, tc = T[m], ptt_p = t_p / lp.pk, ptt = tc / pk, u = U[m], v = V[m];
      // PKH = PET(L)^kappa = k0(l) e^x(l) = k0(l-1) e^(x(l-1) + x(l)):  PKH - PKT(L-1) and PKT(L) - PKH without their cancellation
      const double dz = cp * (ptt_p * (lp.k0 * (expm1(lp.x + lc.x) - lp.g)) - ptt * (lc.k0 * (expm1(lc.x) - lc.g)));
      const double ws = (u_p - u) * (u_p - u) + (v_p - v) * (v_p - v) + 0.01;
      // PTT(L-1) -+ PTT(L) = (T(L-1) rho -+ T(L)) / pk(L), rho = pk(L) / pk(L-1) = 1 + del
      const double del = expm1(lp.x + log1p(lc.g) - log1p(lp.g));
      const double ri = grav * (((t_p - tc) + t_p * del) / (0.5 * (t_p * (1. + del) + tc))) * dz / ws;
      const double rin = 900. * sqrt(ws) / dz;
      const double kx = ri < 0. ? rin * sqrt(1. - 18. * ri) : rin / (1. + 10. * ri * (1. + 8. * ri));
      const double kh = kx > 0.01 ? kx : 0.01;
      const double tvb = tc * (1.0 + eps * QV[m] - QL[m] - QI[m]);
      const double tve = 0.5 * (tvt + tvb);
      tvt = tvb;
      const double ckx = -kh * pe / (rgas * tve) / dz;
      const double c_up = ckx * dmi;
      dmi = (grav * a.dt) / (pe - pe1);
      const double al = ckx * dmi;
      put(2, m - pl, c_up); put(1, m - pl, 1.0 - (a_prev + c_up)); put(0, m, al);
      if (l == lm) {
        const double wsf = sqrt(u * u + v * v + 1.0);
        const bool sea = a.fro[(size_t)t * pl + a.g.idx(i, j)] == 1.0;
        const double cdrag = sea ? 0.0015 : 0.002, tcoef = sea ? 1. : 0.;
        const double khs = -cdrag * dmi * wsf * pe / (rgas * tvb);
        put(2, m, 0.);
        a.fac[(3 * TURB_V + 1) * a.fs + o + m] = 1.0 - (al + 0. + khs);
        a.fac[(3 * TURB_S + 1) * a.fs + o + m] = 1.0 - (al + 0. + khs * tcoef);
        a.fac[(3 * TURB_Q + 1) * a.fs + o + m] = 1.0 - (al + 0.);
      }
      a_prev = al; pe1 = pe; lp = lc; t_p = tc; u_p = u; v_p = v;
    }
  }
};

// cells of the launch and the byte models above
inline double turb_cells(const Geom& g) { return double(g.tx) * g.ty * g.ntile * g.npz; }
inline void run_turb_factorise(Exec& ex, const TurbArgs& a) {
  const Geom& g = a.g;
  for_points(ex, Rect{g.is(), g.ie(), g.js(), g.je()}, g.ntile * 4, TurbFactorFn{a}, "turbulence_factorise", 8. * (9. + 6. + 2.) * turb_cells(g));
}
inline void run_turb_simple(Exec& ex, const TurbArgs& a) {
  const Geom& g = a.g;
  for_points(ex, Rect{g.is(), g.ie(), g.js(), g.je()}, g.ntile, TurbSimpleFn{a}, "turbulence_blsimp", 8. * (7. + 9.) * turb_cells(g));
}
inline void run_turb_solve(Exec& ex, int mode, const TurbArgs& a) {
  const Geom& g = a.g;
  for_points(ex, Rect{g.is(), g.ie(), g.js(), g.je()}, g.ntile * 3, TurbSolveFn{a, mode},
             mode == MODE_NL ? "turbulence_solve.nl" : mode == MODE_TL ? "turbulence_solve.tl" : "turbulence_solve.ad", 8. * (10. + 2. * (3. + a.nq)) * turb_cells(g));
}

}  // namespace fv3
