// fv3lm-hip: the bulk of c_sw's d2a2c_vect (sw_core_tlm.F90:6505-6803) as ONE LDS-tiled launch per mode.
//
// The staged form (dycore.h build_acoustic) runs the bulk as two launches, CswInterpA (u, v -> utmp, vtmp, ua, va) and CswInterpC
// (utmp, vtmp, u, v -> uc0, utf, vc0, vtf), and utmp, vtmp make a round trip through HBM.  Away from the cube edges both are 4-point
// interpolations with the constant weights A1, A2; within three cells of an edge CswInterpA is the 2-point average (`band`), with no
// metric term, view or corner fix involved.  Here one workgroup owns a 64 x 16 block of points of one level: it loads a u tile (halo
// -2, +1 in i; -1, +2 in j) and a v tile (the transpose) into LDS once (tangent mode: value and tangent planes), forms utmp and vtmp
// in LDS -- the band points among the inputs of CswInterpC included, selected per point from the face's global indices -- and writes
// ua, va on the bulk rectangle of CswInterpA and uc0, utf, vc0, vtf on the rectangles of CswInterpC_<false>.  The arithmetic is that
// of CswInterpAD::eval_e and CswInterpC_::eval in their order, so the host emulation agrees with the staged launches bit for bit.
//
// utmp, vtmp are NOT stored by this launch, anywhere.  Their remaining readers are the strips of CswInterpC next to the cube edges
// (and their corner views), which read them within three cells of an edge only: band territory, written by the strips of CswInterpA
// (which still store utmp, vtmp, ua, va there).  The launch must not read those stored values itself -- the strips run beside it.
//
// The adjoint is the closed-form transpose in the same tile structure: the adjoints of uc0, utf (vc0, vtf) are combined into LDS tiles,
// carried through the A1 / A2 weights to utmp_ad / vtmp_ad in LDS (+ the ua, va part), then through the A1 / A2 weights or the band's
// 0.5 to u_ad, v_ad.  Every output element is owned by exactly one thread: no atomics, fixed order.  The only trajectory dependence is
// the sign of ut / vt that picks the sin_sg factor of utf / vtf; it is read off the stored trajectory of utf / vtf (dt2 dy sin_sg > 0
// times ut, the same two fields of traffic as a recompute from u, v and a third of the LDS).  What reaches band points of utmp / vtmp
// through the fused outputs goes straight on to u_ad / v_ad here; what reaches them through the stored band values (the adjoint of the
// CswInterpC strips) keeps travelling through utmp_ad / vtmp_ad in memory to the adjoint of the CswInterpA strips -- the routine is
// linear in the perturbation, the two paths add.  The launch is the first of the routine in the backward sweep and stores the zeros
// those strips accumulate onto (Op::ad_store), on the band points of its launch rectangle.
#pragma once
#include <algorithm>
#include "stages.h"
#include "tiled.h"

namespace fv3 {

struct D2a2cArgs {
  Fld u, v;                        // inputs (D grid)
  Fld ua, va, uc0, utf, vc0, vtf;  // outputs
  Fld utmp, vtmp;                  // the staged intermediates: never written; adjoint on a face: zeros stored on the bands (clear_tmp)
  Rect ru, rv, ra;                 // where uc0, utf / vc0, vtf / ua, va are formed (CswInterpC_<false>'s and CswInterpA's bulk rectangles)
  Rect rtmp{1, 0, 1, 0};           // face: where utmp_ad, vtmp_ad must hold defined values (the rectangles of the CswInterpA strips)
  double dt2 = 0.;
  int nk = 0;
  int face = 0;                    // cube faces: the 2-point band within three cells of an edge
  int clear_tmp = 0;
  unsigned wmask = 0;              // adjoint: u_ad (bit 0), v_ad (bit 1) stored instead of accumulated (dycore.h plan_adjoint) ...
  Rect wrect{1, 0, 1, 0};          // ... over the launch rectangle widened to this one
  // utmp is formed where uc0 reads it (ru widened by -2, +1 in i) and on ra; vtmp the transpose
  HD bool has_ut(int i, int j) const { return (i >= ru.i0 - 2 && i <= ru.i1 + 1 && j >= ru.j0 && j <= ru.j1) || ra.has(i, j); }
  HD bool has_vt(int i, int j) const { return (i >= rv.i0 && i <= rv.i1 && j >= rv.j0 - 2 && j <= rv.j1 + 1) || ra.has(i, j); }
  Rect all() const {               // the rectangle the forward launch is laid over
    return rect_join(rect_join(ru, rv), ra);
  }
};
// nonlinear / tangent / adjoint launch of the bulk
FV3LM_LINK void run_d2a2c(Exec& ex, int mode, const D2a2cArgs& a0, const Ctx& c);

// algorithmic bytes of one launch in the convention of stage_bytes: u, v read, six outputs written (x2 in the tangent mode; adjoint: six
// output adjoints and the trajectory of utf, vtf read, u_ad, v_ad read-modify-written)
inline double d2a2c_bytes(const D2a2cArgs& a, const Geom& g, int mode) {
  const Rect q = a.all();
  const double cells = double(q.i1 - q.i0 + 1) * double(q.j1 - q.j0 + 1) * g.ntile * a.nk;
  return 8. * cells * (mode == MODE_NL ? 8. : mode == MODE_TL ? 16. : 12.);
}
}  // namespace fv3

#if !defined(FV3LM_SPLIT_BUILD) || defined(FV3LM_IMPL_D2A2C)
namespace fv3 {
#ifndef FV3LM_D2A2C_THREADS_NL
#define FV3LM_D2A2C_THREADS_NL 256
#endif
#ifndef FV3LM_D2A2C_THREADS_TL
#define FV3LM_D2A2C_THREADS_TL 512
#endif
#ifndef FV3LM_D2A2C_THREADS_AD
#define FV3LM_D2A2C_THREADS_AD 512
#endif
constexpr int D2C_W = 64, D2C_H = 16;                          // points per block
constexpr int D2C_QW = D2C_W + 3, D2C_QH = D2C_H + 3;          // a halo'd extent
// LDS of the forward modes, doubles per component: u tile | v tile | utmp (halo'd in i) | vtmp (halo'd in j)
constexpr int D2C_NQ = D2C_QW * D2C_QH, D2C_NUT = D2C_QW * D2C_H, D2C_NVT = D2C_W * D2C_QH, D2C_NT = 2 * D2C_NQ + D2C_NUT + D2C_NVT;
// LDS of the adjoint: uc_ad | vc_ad (halo'd both ways) | the utf / vtf part of the block | utmp_ad (halo'd in j) | vtmp_ad (halo'd in i)
constexpr int D2C_NB = D2C_W * D2C_H, D2C_NT_AD = 2 * D2C_NQ + 2 * D2C_NB + D2C_NVT + D2C_NUT;
// the 2-point band of CswInterpAD::eval_e (global face indices)
HD bool d2c_band(const D2a2cArgs& a, const Geom& g, int i, int j) { return a.face && (i <= 3 || i >= g.nx - 2 || j <= 3 || j >= g.ny - 2); }
#ifdef FV3LM_HOST_EMUL
#define D2C_UNROLL
#else
#define D2C_UNROLL _Pragma("unroll")
#endif
// the metric terms of point (i, j): cosa_s rsin2 | cosa_u rsin_u dy sin_sg3(i-1) sin_sg1 | cosa_v rsin_v dx sin_sg4(j-1) sin_sg2
enum { M_CS, M_R2, M_CU, M_RU, M_DY, M_S3, M_S1, M_CV, M_RV, M_DX, M_S4, M_S2, M_N };
DEV void d2c_metrics(const Ctx& c, int tile, int i, int j, double* m) {
  const int m0 = c.mi(tile, i, j), mw = c.mi(tile, i - 1, j), ms = c.mi(tile, i, j - 1);
  m[M_CS] = c.m.cosa_s[m0]; m[M_R2] = c.m.rsin2[m0];
  m[M_CU] = c.m.cosa_u[m0]; m[M_RU] = c.m.rsin_u[m0]; m[M_DY] = c.m.dy[m0]; m[M_S3] = c.m.sin_sg[3][mw]; m[M_S1] = c.m.sin_sg[1][m0];
  m[M_CV] = c.m.cosa_v[m0]; m[M_RV] = c.m.rsin_v[m0]; m[M_DX] = c.m.dx[m0]; m[M_S4] = c.m.sin_sg[4][ms]; m[M_S2] = c.m.sin_sg[2][m0];
}
// an index clamped to where (m, m - 1) both lie in the padded plane
HD int d2c_clamp(int m, int lo, int hi) { return m <= lo ? lo + 1 : m > hi ? hi : m; }

// One block of the forward modes: the points I0..I1 x J0..J1 of level k of one tile, blocks laid over Qr = a.all().
template <class T, int NTH>
DEV void d2a2c_block(const D2a2cArgs& a, const Ctx& c, const Rect& Qr, int tile, int k, int bx, int by, double* lds, int tid) {
  typedef TpfIO<T> IO;
  const Geom& g = c.g;
  const TileBlk B = tile_blk(Qr, bx, by, D2C_W, D2C_H);
  const int I0 = B.I0, I1 = B.I1, J0 = B.J0, J1 = B.J1;
  double* const U = lds; double* const V = U + D2C_NQ; double* const UT = V + D2C_NQ; double* const VT = UT + D2C_NUT;
  // ---- u on [I0-2, I1+1] x [J0-1, J1+2], v on [I0-1, I1+2] x [J0-2, J1+1].  Every element of a tile is loaded, from its index clamped
  // into the plane and the block's reach (more than is read below; a clamped element is never read): loads without a branch around
  // them, all of a thread's elements in flight at once -- a load per branch, each waited for, cost ten memory latencies per block
  {
    constexpr int E = (D2C_NQ + NTH - 1) / NTH;
    const int ihi = (I1 + 2 < g.ied() + 1) ? I1 + 2 : g.ied() + 1, jhi = (J1 + 2 < g.jed() + 1) ? J1 + 2 : g.jed() + 1;
    auto ci = [&](int i) { return i < g.isd() ? g.isd() : i > ihi ? ihi : i; };
    auto cj = [&](int j) { return j < g.jsd() ? g.jsd() : j > jhi ? jhi : j; };
    T ru[E], rv[E];
    D2C_UNROLL
    for (int s = 0; s < E; ++s) {
      const int e = (tid + s * NTH < D2C_NQ) ? tid + s * NTH : D2C_NQ - 1, x = e % D2C_QW, r = e / D2C_QW;
      ru[s] = IO::ld(a.u, fld_at(g, a.u, tile, k, ci(I0 - 2 + x), cj(J0 - 1 + r)));
      rv[s] = IO::ld(a.v, fld_at(g, a.v, tile, k, ci(I0 - 1 + x), cj(J0 - 2 + r)));
    }
    D2C_UNROLL
    for (int s = 0; s < E; ++s) {
      const int e = tid + s * NTH;
      if (e < D2C_NQ) { IO::lset(U, D2C_NT, e, ru[s]); IO::lset(V, D2C_NT, e, rv[s]); }
    }
  }
  TPF_SYNC();
  // ---- utmp on [I0-2, I1+1] x [J0, J1], vtmp on [I0, I1] x [J0-2, J1+1] (CswInterpAD::eval_e, the band select per point)
  TPF_LOOP(e, D2C_NUT) {
    const int x = e % D2C_QW, r = e / D2C_QW, i = I0 - 2 + x, j = J0 + r;
    if (i > I1 + 1 || j > J1 || !a.has_ut(i, j)) continue;
    auto u = [&](int jj) -> T { return IO::lget(U, D2C_NT, (jj - (J0 - 1)) * D2C_QW + x); };
    const T ut = d2c_band(a, g, i, j) ? 0.5 * (u(j) + u(j + 1)) : A2 * (u(j - 1) + u(j + 2)) + A1 * (u(j) + u(j + 1));
    IO::lset(UT, D2C_NT, e, ut);
  }
  TPF_LOOP(e, D2C_NVT) {
    const int x = e % D2C_W, r = e / D2C_W, i = I0 + x, j = J0 - 2 + r;
    if (i > I1 || j > J1 + 1 || !a.has_vt(i, j)) continue;
    auto v = [&](int ii) -> T { return IO::lget(V, D2C_NT, r * D2C_QW + (ii - (I0 - 1))); };
    const T vt = d2c_band(a, g, i, j) ? 0.5 * (v(i) + v(i + 1)) : A2 * (v(i - 1) + v(i + 2)) + A1 * (v(i) + v(i + 1));
    IO::lset(VT, D2C_NT, e, vt);
  }
  TPF_SYNC();
  // ---- ua, va (CswInterpAD::eval_e); uc0, utf, vc0, vtf (CswInterpC_<false>::eval)
  // the metric terms of a thread's points first, all loads in flight at once (indices clamped into the plane: no branch around a load)
  constexpr int E3 = (D2C_NB + NTH - 1) / NTH;
  double mt[E3][M_N];
  D2C_UNROLL
  for (int s = 0; s < E3; ++s) {
    const int e = (tid + s * NTH < D2C_NB) ? tid + s * NTH : D2C_NB - 1;
    d2c_metrics(c, tile, d2c_clamp(I0 + e % D2C_W, g.isd(), g.ied() + 1), d2c_clamp(J0 + e / D2C_W, g.jsd(), g.jed() + 1), mt[s]);
  }
  D2C_UNROLL
  for (int s = 0; s < E3; ++s) {
    const int e = tid + s * NTH;
    if (e >= D2C_NB) continue;
    const int x = e % D2C_W, r = e / D2C_W, i = I0 + x, j = J0 + r;
    if (i > I1 || j > J1) continue;
    const double* const mm = mt[s];
    auto utmp = [&](int ii) -> T { return IO::lget(UT, D2C_NT, r * D2C_QW + (ii - (I0 - 2))); };
    auto vtmp = [&](int jj) -> T { return IO::lget(VT, D2C_NT, (jj - (J0 - 2)) * D2C_W + x); };
    if (a.ra.has(i, j)) {
      const T ut = utmp(i), vt = vtmp(j);
      const double cs = mm[M_CS], r2 = mm[M_R2];
      IO::st(a.ua, fld_at(g, a.ua, tile, k, i, j), (ut - vt * cs) * r2);
      IO::st(a.va, fld_at(g, a.va, tile, k, i, j), (vt - ut * cs) * r2);
    }
    if (a.ru.has(i, j)) {
      const T uc = A2 * (utmp(i - 2) + utmp(i + 1)) + A1 * (utmp(i - 1) + utmp(i));
      const T ut = (uc - IO::lget(V, D2C_NT, (r + 2) * D2C_QW + (x + 1)) * mm[M_CU]) * mm[M_RU];
      IO::st(a.uc0, fld_at(g, a.uc0, tile, k, i, j), uc);
      IO::st(a.utf, fld_at(g, a.utf, tile, k, i, j), (val(ut) > 0.) ? a.dt2 * ut * mm[M_DY] * mm[M_S3] : a.dt2 * ut * mm[M_DY] * mm[M_S1]);
    }
    if (a.rv.has(i, j)) {
      const T vc = A2 * (vtmp(j - 2) + vtmp(j + 1)) + A1 * (vtmp(j - 1) + vtmp(j));
      const T vt = (vc - IO::lget(U, D2C_NT, (r + 1) * D2C_QW + (x + 2)) * mm[M_CV]) * mm[M_RV];
      IO::st(a.vc0, fld_at(g, a.vc0, tile, k, i, j), vc);
      IO::st(a.vtf, fld_at(g, a.vtf, tile, k, i, j), (val(vt) > 0.) ? a.dt2 * vt * mm[M_DX] * mm[M_S4] : a.dt2 * vt * mm[M_DX] * mm[M_S2]);
    }
  }
}

// One block of the adjoint: the points I0..I1 x J0..J1 of u_ad, v_ad, blocks laid over Qr (run_d2a2c).
template <int NTH>
DEV void d2a2c_ad_block(const D2a2cArgs& a, const Ctx& c, const Rect& Qr, int tile, int k, int bx, int by, double* lds, int tid) {
  const Geom& g = c.g;
  const TileBlk B = tile_blk(Qr, bx, by, D2C_W, D2C_H);
  const int I0 = B.I0, I1 = B.I1, J0 = B.J0, J1 = B.J1;
  double* const UC = lds; double* const VC = UC + D2C_NQ; double* const GU = VC + D2C_NQ; double* const GV = GU + D2C_NB;
  double* const UTA = GV + D2C_NB; double* const VTA = UTA + D2C_NVT;
  // ---- uc_ad on [I0-1, I0+W+1] x [J0-2, J0+H], vc_ad on [I0-2, I0+W] x [J0-1, J0+H+1]: the adjoint of uc0 + the one of utf through ut (the
  // formulas of CswInterpC_::hand_ad), zero outside ru / rv; the utf / vtf part of the block's own points is kept for v_ad / u_ad
  // Every phase loads what its elements need first, from indices clamped into the plane (no branch around a load: all of a thread's
  // loads in flight at once), then selects.
  const int ilo = g.isd(), ihi = g.ied() + 1, jlo = g.jsd(), jhi = g.jed() + 1;
  constexpr int E1 = (D2C_NQ + NTH - 1) / NTH;
  {
    double q[E1][7];      // utf (trajectory), utf_ad, uc0_ad, dy, sin_sg3(i-1), sin_sg1, rsin_u
    D2C_UNROLL
    for (int s = 0; s < E1; ++s) {
      const int e = (tid + s * NTH < D2C_NQ) ? tid + s * NTH : D2C_NQ - 1;
      const int i = d2c_clamp(I0 - 1 + e % D2C_QW, ilo, ihi), j = d2c_clamp(J0 - 2 + e / D2C_QW, jlo, jhi);
      const size_t m = fld_at(g, a.utf, tile, k, i, j);
      q[s][0] = a.utf.t[m]; q[s][1] = a.utf.p[m]; q[s][2] = a.uc0.p[m];
      q[s][3] = MET(dy, i, j); q[s][4] = SSG(3, i - 1, j); q[s][5] = SSG(1, i, j); q[s][6] = MET(rsin_u, i, j);
    }
    D2C_UNROLL
    for (int s = 0; s < E1; ++s) {
      const int e = tid + s * NTH;
      if (e >= D2C_NQ) continue;
      const int x = e % D2C_QW, r = e / D2C_QW, i = I0 - 1 + x, j = J0 - 2 + r;
      double v = 0., gu = 0.;
      if (a.ru.has(i, j)) {
        const double f = a.dt2 * q[s][3] * ((q[s][0] * a.dt2 > 0.) ? q[s][4] : q[s][5]) * q[s][1];
        gu = q[s][6] * f;
        v = q[s][2] + gu;
      }
      UC[e] = v;
      if (x >= 1 && x <= D2C_W && r >= 2 && r < 2 + D2C_H) GU[(r - 2) * D2C_W + (x - 1)] = gu;
    }
  }
  {
    double q[E1][7];      // vtf (trajectory), vtf_ad, vc0_ad, dx, sin_sg4(j-1), sin_sg2, rsin_v
    D2C_UNROLL
    for (int s = 0; s < E1; ++s) {
      const int e = (tid + s * NTH < D2C_NQ) ? tid + s * NTH : D2C_NQ - 1;
      const int i = d2c_clamp(I0 - 2 + e % D2C_QW, ilo, ihi), j = d2c_clamp(J0 - 1 + e / D2C_QW, jlo, jhi);
      const size_t m = fld_at(g, a.vtf, tile, k, i, j);
      q[s][0] = a.vtf.t[m]; q[s][1] = a.vtf.p[m]; q[s][2] = a.vc0.p[m];
      q[s][3] = MET(dx, i, j); q[s][4] = SSG(4, i, j - 1); q[s][5] = SSG(2, i, j); q[s][6] = MET(rsin_v, i, j);
    }
    D2C_UNROLL
    for (int s = 0; s < E1; ++s) {
      const int e = tid + s * NTH;
      if (e >= D2C_NQ) continue;
      const int x = e % D2C_QW, r = e / D2C_QW, i = I0 - 2 + x, j = J0 - 1 + r;
      double v = 0., gv = 0.;
      if (a.rv.has(i, j)) {
        const double f = a.dt2 * q[s][3] * ((q[s][0] * a.dt2 > 0.) ? q[s][4] : q[s][5]) * q[s][1];
        gv = q[s][6] * f;
        v = q[s][2] + gv;
      }
      VC[e] = v;
      if (x >= 2 && x < 2 + D2C_W && r >= 1 && r <= D2C_H) GV[(r - 1) * D2C_W + (x - 2)] = gv;
    }
  }
  TPF_SYNC();
  // ---- utmp_ad on [I0, I0+W-1] x [J0-2, J0+H], vtmp_ad on [I0-2, I0+W] x [J0, J0+H-1]: the transposed A1 / A2 sums + the ua, va part
  {
    constexpr int E2 = (D2C_NVT + NTH - 1) / NTH;
    double q[E2][4];      // ua_ad, va_ad, rsin2, cosa_s
    D2C_UNROLL
    for (int s = 0; s < E2; ++s) {
      const int e = (tid + s * NTH < D2C_NVT) ? tid + s * NTH : D2C_NVT - 1;
      const int i = d2c_clamp(I0 + e % D2C_W, ilo, ihi), j = d2c_clamp(J0 - 2 + e / D2C_W, jlo, jhi);
      const size_t m = fld_at(g, a.ua, tile, k, i, j);
      q[s][0] = a.ua.p[m]; q[s][1] = a.va.p[m]; q[s][2] = MET(rsin2, i, j); q[s][3] = MET(cosa_s, i, j);
    }
    D2C_UNROLL
    for (int s = 0; s < E2; ++s) {
      const int e = tid + s * NTH;
      if (e >= D2C_NVT) continue;
      const int x = e % D2C_W, r = e / D2C_W, i = I0 + x, j = J0 - 2 + r;
      double v = 0.;
      if (a.has_ut(i, j)) {
        const double* p = UC + r * D2C_QW + x;         // uc_ad(i-1, j)
        v = A2 * (p[0] + p[3]) + A1 * (p[1] + p[2]);
        if (a.ra.has(i, j)) v += q[s][2] * (q[s][0] - q[s][3] * q[s][1]);
      }
      UTA[e] = v;
    }
  }
  {
    constexpr int E2 = (D2C_NUT + NTH - 1) / NTH;
    double q[E2][4];      // ua_ad, va_ad, rsin2, cosa_s
    D2C_UNROLL
    for (int s = 0; s < E2; ++s) {
      const int e = (tid + s * NTH < D2C_NUT) ? tid + s * NTH : D2C_NUT - 1;
      const int i = d2c_clamp(I0 - 2 + e % D2C_QW, ilo, ihi), j = d2c_clamp(J0 + e / D2C_QW, jlo, jhi);
      const size_t m = fld_at(g, a.ua, tile, k, i, j);
      q[s][0] = a.ua.p[m]; q[s][1] = a.va.p[m]; q[s][2] = MET(rsin2, i, j); q[s][3] = MET(cosa_s, i, j);
    }
    D2C_UNROLL
    for (int s = 0; s < E2; ++s) {
      const int e = tid + s * NTH;
      if (e >= D2C_NUT) continue;
      const int x = e % D2C_QW, r = e / D2C_QW, i = I0 - 2 + x, j = J0 + r;
      double v = 0.;
      if (a.has_vt(i, j)) {
        const double* p = VC + r * D2C_QW + x;         // vc_ad(i, j-1)
        v = A2 * (p[0] + p[3 * D2C_QW]) + A1 * (p[D2C_QW] + p[2 * D2C_QW]);
        if (a.ra.has(i, j)) v += q[s][2] * (q[s][1] - q[s][3] * q[s][0]);
      }
      VTA[e] = v;
    }
  }
  TPF_SYNC();
  // ---- u_ad, v_ad: utmp(i, j') reads u(i, j'-1 .. j'+2) with A2 A1 A1 A2, on the band u(i, j'), u(i, j'+1) with 0.5; vtmp the transpose
  // (store rules of exec.h body_ad_joint: the whole launch rectangle is stored in write mode, zeros where nothing arrives)
  constexpr int E3 = (D2C_NB + NTH - 1) / NTH;
  const bool acc_u = a.u.p && !(a.wmask & 1u), acc_v = a.v.p && !(a.wmask & 2u);
  double q[E3][4];        // u_ad, v_ad as they stand (accumulate mode), cosa_v, cosa_u
  D2C_UNROLL
  for (int s = 0; s < E3; ++s) {
    const int e = (tid + s * NTH < D2C_NB) ? tid + s * NTH : D2C_NB - 1;
    const int i = (I0 + e % D2C_W < I1) ? I0 + e % D2C_W : I1, j = (J0 + e / D2C_W < J1) ? J0 + e / D2C_W : J1;      // the block's own points: in the plane
    const size_t m = fld_at(g, a.u, tile, k, i, j);
    q[s][0] = acc_u ? a.u.p[m] : 0.; q[s][1] = acc_v ? a.v.p[m] : 0.; q[s][2] = MET(cosa_v, i, j); q[s][3] = MET(cosa_u, i, j);
  }
  D2C_UNROLL
  for (int s = 0; s < E3; ++s) {
    const int e = tid + s * NTH;
    if (e >= D2C_NB) continue;
    const int x = e % D2C_W, r = e / D2C_W, i = I0 + x, j = J0 + r;
    if (i > I1 || j > J1) continue;
    double au = 0., av = 0.;
    D2C_UNROLL
    for (int d = 0; d < 4; ++d) {                    // utmp_ad(i, j-2+d), vtmp_ad(i-2+d, j)
      const bool mid = d == 1 || d == 2;
      au += (d2c_band(a, g, i, j - 2 + d) ? (mid ? 0.5 : 0.) : (mid ? A1 : A2)) * UTA[(r + d) * D2C_W + x];
      av += (d2c_band(a, g, i - 2 + d, j) ? (mid ? 0.5 : 0.) : (mid ? A1 : A2)) * VTA[r * D2C_QW + x + d];
    }
    if (a.rv.has(i, j)) au -= q[s][2] * GV[e];
    if (a.ru.has(i, j)) av -= q[s][3] * GU[e];
    const size_t m = fld_at(g, a.u, tile, k, i, j);
    if (a.u.p) a.u.p[m] = q[s][0] + au;
    if (a.v.p) a.v.p[m] = q[s][1] + av;
    if (a.clear_tmp && a.rtmp.has(i, j) && d2c_band(a, g, i, j)) { a.utmp.p[m] = 0.; a.vtmp.p[m] = 0.; }
  }
}

// the block descriptors (tiled.h)
template <class T, int N> struct D2a2cFwd {
  typedef D2a2cArgs Args; static constexpr int NTH = N; static constexpr size_t LDS_BYTES = (size_t)D2C_NT * 8 * TpfIO<T>::NC;
  DEV static void block(const Args& a, const Ctx& c, const Rect& Qr, int tile, int k, int bx, int by, double* lds, int tid) { d2a2c_block<T, N>(a, c, Qr, tile, k, bx, by, lds, tid); }
};
template <int N> struct D2a2cAd {
  typedef D2a2cArgs Args; static constexpr int NTH = N; static constexpr size_t LDS_BYTES = (size_t)D2C_NT_AD * 8;
  DEV static void block(const Args& a, const Ctx& c, const Rect& Qr, int tile, int k, int bx, int by, double* lds, int tid) { d2a2c_ad_block<N>(a, c, Qr, tile, k, bx, by, lds, tid); }
};

FV3LM_LINK void run_d2a2c(Exec& ex, int mode, const D2a2cArgs& a0, const Ctx& c) {
  D2a2cArgs a = a0;
  for (Fld* f : {&a.u, &a.v, &a.ua, &a.va, &a.uc0, &a.utf, &a.vc0, &a.vtf, &a.utmp, &a.vtmp}) *f = ex.sh(*f);
  if (ex.no_wmask) a.wmask = 0;
  if (!a.utmp.p || !a.vtmp.p) a.clear_tmp = 0;
  if (mode == MODE_AD && !a.u.p && !a.v.p && !a.clear_tmp) return;
  Rect Qr = a.all();
  if (mode == MODE_AD) {
    // three points around everything the bulk forms (the reach of the two interpolations), where the zeros of utmp_ad / vtmp_ad go, and
    // in store mode where the stored adjoint is read later
    Qr.i0 -= 3; Qr.i1 += 3; Qr.j0 -= 3; Qr.j1 += 3;
    if (a.clear_tmp) Qr = rect_join(Qr, a.rtmp);
    Qr = ad_launch_rect(Qr, a.wmask != 0, a.wrect, c.g);
  }
  const int nbx = tiled_blocks(Qr.i0, Qr.i1, D2C_W), nby = tiled_blocks(Qr.j0, Qr.j1, D2C_H);
  const double bytes = d2a2c_bytes(a, c.g, mode);
  if (mode == MODE_TL) run_tiled<D2a2cFwd<Dual, tiled_nth(FV3LM_D2A2C_THREADS_TL)>>(ex, "D2a2c", mode_tag(mode), bytes, Qr, nbx, nby, a, c);
  else if (mode == MODE_NL) run_tiled<D2a2cFwd<double, tiled_nth(FV3LM_D2A2C_THREADS_NL)>>(ex, "D2a2c", mode_tag(mode), bytes, Qr, nbx, nby, a, c);
  else run_tiled<D2a2cAd<tiled_nth(FV3LM_D2A2C_THREADS_AD)>>(ex, "D2a2c", mode_tag(mode), bytes, Qr, nbx, nby, a, c);
}

}  // namespace fv3
#endif
