// fv3lm-hip: Rayleigh damping of the upper layers, RAYLEIGH_SUPER (fv_dynamics_tlm.F90:1749-1899; adjoint RAYLEIGH_SUPER_FWD / _BWD,
// fv_dynamics_adm.F90:2327-2652) with conserve = .true., not nested, grid_type < 4: on the levels k = 1..kmax whose reference pressure is
// below rf_cutoff, the D-grid winds go to cell-centre lat-lon winds (C2L_ORD2, fv_grid_utils_tlm.F90:349-450, do_halo = .false.), the
// kinetic energy the damping removes heats pt (temperature here), and u, v (and w) are multiplied by u2f = 1 / (1 + rf(k)).  u2f is one
// constant per level, so the reference's halo update of it (:1837) carries nothing: the unit is local to a tile.
//
// Three point launches over the cells and edges of a tile (is..ie+1 x js..je+1, one thread per point, i fastest) and levels 1..kmax:
//   forward (nonlinear T = double, tangent T = Dual): heat (cells; reads the winds before the damping and, in MODE_NL, checkpoints them
//   for the adjoint), then damp (edges, cells) -- two launches, because a cell reads the edges the damping rewrites;
//   adjoint, gather form: the thread of an edge collects from the (up to) two cells that read it, the thread of a cell its w; no atomics.
// Non-hydrostatic: the heated temperature goes to its own field (pth, levels 1..kmax), because pt_in takes pkz from the temperature
// BEFORE the heating (fv_dynamics_tlm.F90:436-470 run before :535) and divides the heated one by it (:564-590); stages.h DynPtInNhRf.
#pragma once
#include "column.h"
#include "remap.h"

namespace fv3 {

struct RfArgs {
  Geom g;
  Fld u, v, w, pt, pth;            // pth: non-hydrostatic heated temperature (hydrostatic: pt itself)
  const double *dx, *dy;           // metrics of the class's tiles
  const double* c2l;               // [ntile][4: a11 a12 a21 a22][plane]
  const double* lv;                // per level k = 1..kmax: rf(k), cp_air - rdgas ptop / pm(k)
  double rcv;                      // 1 / (cp_air - rdgas)  (non-hydrostatic heating)
  int kmax, nh;
  double *cu, *cv, *cw;            // winds before the damping, [ntile][kmax][plane] (written in MODE_NL, read by the adjoint)
  HD size_t ck(int t, int k, int i, int j) const { return ((size_t)t * kmax + k - 1) * g.plane + g.idx(i, j); }
  HD double met(const double* p, int t, int i, int j) const { return p[(size_t)t * g.plane + g.idx(i, j)]; }
  HD double a(int t, int n, int i, int j) const { return c2l[((size_t)t * 4 + n) * g.plane + g.idx(i, j)]; }
  HD double u2f(int k) const { return 1. / (1. + lv[2 * (k - 1)]); }
};

// C2L_ORD2 at cell (i, j) from its four D-grid edges (fv_grid_utils_tlm.F90:408-431)
template <class T>
HD void rf_c2l(const RfArgs& a, int t, int i, int j, T us, T un, T vw, T ve, T& ua, T& va) {
  const double dx0 = a.met(a.dx, t, i, j), dx1 = a.met(a.dx, t, i, j + 1), dy0 = a.met(a.dy, t, i, j), dy1 = a.met(a.dy, t, i + 1, j);
  T u1 = 2. * (us * dx0 + un * dx1) / (dx0 + dx1);
  T v1 = 2. * (vw * dy0 + ve * dy1) / (dy0 + dy1);
  ua = a.a(t, 0, i, j) * u1 + a.a(t, 1, i, j) * v1;
  va = a.a(t, 2, i, j) * u1 + a.a(t, 3, i, j) * v1;
}

// heating of one cell, conserve = .true. (fv_dynamics_tlm.F90:1845-1866)
template <class T>
HD void rf_heat_cell(const RfArgs& a, int t, int k, int i, int j) {
  typedef FIO<T> IO; const Geom& g = a.g;
  T ua, va;
  rf_c2l<T>(a, t, i, j, IO::ld(a.u, fidx(g, a.u, t, i, j, k)), IO::ld(a.u, fidx(g, a.u, t, i, j + 1, k)),
            IO::ld(a.v, fidx(g, a.v, t, i, j, k)), IO::ld(a.v, fidx(g, a.v, t, i + 1, j, k)), ua, va);
  const double u2f = a.u2f(k);
  const size_t n = fidx(g, a.pt, t, i, j, k);
  const T pt = IO::ld(a.pt, n);
  if (!a.nh) { IO::st(a.pt, n, pt + 0.5 * (ua * ua + va * va) * (1. - u2f * u2f) / a.lv[2 * (k - 1) + 1]); return; }
  const T w = IO::ld(a.w, fidx(g, a.w, t, i, j, k));
  IO::st(a.pth, fidx(g, a.pth, t, i, j, k), pt + 0.5 * (ua * ua + va * va + w * w) * (1. - u2f * u2f) * a.rcv);
}

struct RfHeatFn {   // MODE_NL / MODE_TL
  RfArgs a; int mode;
  HD void operator()(int i, int j, int z) const {
    const Geom& g = a.g; const int t = z / a.kmax, k = 1 + z % a.kmax;
    const bool cell = i <= g.ie() && j <= g.je();
    if (mode == MODE_NL) {
      const size_t c = a.ck(t, k, i, j);
      if (i <= g.ie()) a.cu[c] = a.u.t[fidx(g, a.u, t, i, j, k)];
      if (j <= g.je()) a.cv[c] = a.v.t[fidx(g, a.v, t, i, j, k)];
      if (a.nh && cell) a.cw[c] = a.w.t[fidx(g, a.w, t, i, j, k)];
    }
    if (!cell) return;
    if (mode == MODE_NL) rf_heat_cell<double>(a, t, k, i, j); else rf_heat_cell<Dual>(a, t, k, i, j);
  }
};

// u(is:ie, js:je+1), v(is:ie+1, js:je), w(is:ie, js:je) times u2f (fv_dynamics_tlm.F90:1868-1896)
struct RfDampFn {
  RfArgs a; int mode;
  HD void operator()(int i, int j, int z) const {
    const Geom& g = a.g; const int t = z / a.kmax, k = 1 + z % a.kmax;
    const double u2f = a.u2f(k);
    auto damp = [&](const Fld& f) { const size_t n = fidx(g, f, t, i, j, k); f.t[n] = u2f * f.t[n]; if (mode == MODE_TL) f.p[n] = u2f * f.p[n]; };
    if (i <= g.ie()) damp(a.u);
    if (j <= g.je()) damp(a.v);
    if (a.nh && i <= g.ie() && j <= g.je()) damp(a.w);
  }
};

// Adjoint.  With ptb the adjoint of the heated temperature of a cell and f = (1 - u2f^2) / den (hydrostatic) or (1 - u2f^2) rcv:
// ua_b = f ua ptb, va_b = f va ptb, w_b += f w ptb; u1_b = a11 ua_b + a21 va_b, v1_b = a12 ua_b + a22 va_b; an edge receives
// 2 dx(edge) / (dx(i,j) + dx(i,j+1)) u1_b from each cell it borders (v likewise with dy), on top of u2f times its own adjoint.
struct RfAdFn {
  RfArgs a;
  HD void cell_bar(int t, int k, int i, int j, double& u1b, double& v1b) const {
    double ua, va;
    rf_c2l<double>(a, t, i, j, a.cu[a.ck(t, k, i, j)], a.cu[a.ck(t, k, i, j + 1)], a.cv[a.ck(t, k, i, j)], a.cv[a.ck(t, k, i + 1, j)], ua, va);
    const Fld& h = a.nh ? a.pth : a.pt;
    const double u2f = a.u2f(k), fac = a.nh ? (1. - u2f * u2f) * a.rcv : (1. - u2f * u2f) / a.lv[2 * (k - 1) + 1];
    const double ptb = h.p[fidx(a.g, h, t, i, j, k)];
    const double uab = fac * ua * ptb, vab = fac * va * ptb;
    u1b = a.a(t, 0, i, j) * uab + a.a(t, 2, i, j) * vab;
    v1b = a.a(t, 1, i, j) * uab + a.a(t, 3, i, j) * vab;
  }
  HD void operator()(int i, int j, int z) const {
    const Geom& g = a.g; const int t = z / a.kmax, k = 1 + z % a.kmax;
    const double u2f = a.u2f(k);
    double u1b, v1b;
    if (i <= g.ie()) {           // u(i, j): south edge of cell (i, j), north edge of cell (i, j-1)
      const size_t n = fidx(g, a.u, t, i, j, k);
      const double dxe = a.met(a.dx, t, i, j);
      double acc = u2f * a.u.p[n];
      if (j <= g.je()) { cell_bar(t, k, i, j, u1b, v1b); acc += 2. * dxe * u1b / (dxe + a.met(a.dx, t, i, j + 1)); }
      if (j > g.js()) { cell_bar(t, k, i, j - 1, u1b, v1b); acc += 2. * dxe * u1b / (a.met(a.dx, t, i, j - 1) + dxe); }
      a.u.p[n] = acc;
    }
    if (j <= g.je()) {           // v(i, j): west edge of cell (i, j), east edge of cell (i-1, j)
      const size_t n = fidx(g, a.v, t, i, j, k);
      const double dye = a.met(a.dy, t, i, j);
      double acc = u2f * a.v.p[n];
      if (i <= g.ie()) { cell_bar(t, k, i, j, u1b, v1b); acc += 2. * dye * v1b / (dye + a.met(a.dy, t, i + 1, j)); }
      if (i > g.is()) { cell_bar(t, k, i - 1, j, u1b, v1b); acc += 2. * dye * v1b / (a.met(a.dy, t, i - 1, j) + dye); }
      a.v.p[n] = acc;
    }
    if (a.nh && i <= g.ie() && j <= g.je()) {     // w and the temperature itself (the heated copy is pt plus the heating)
      const size_t n = fidx(g, a.w, t, i, j, k), m = fidx(g, a.pt, t, i, j, k), h = fidx(g, a.pth, t, i, j, k);
      const double ptb = a.pth.p[h];
      a.w.p[n] = u2f * a.w.p[n] + (1. - u2f * u2f) * a.rcv * a.cw[a.ck(t, k, i, j)] * ptb;
      a.pt.p[m] += ptb;
    }
  }
};

}  // namespace fv3
