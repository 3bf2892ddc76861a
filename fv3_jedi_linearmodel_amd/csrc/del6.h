// fv3lm-hip: the damping increment of a cell scalar by del6_vt_flux up to order 2 (sw_core_tlm.F90:3719-3801 + the divergence of its
// fluxes) as ONE LDS-tiled launch per mode: dw of w in d_sw (sw_core_tlm.F90:1712-1745) and the damping term of the interface heights in
// update_dz_d (nh_utils_tlm.F90:489-520, :655-700), in programs that have a level of order 2 and are built with FV3LM_DEL6_FUSED=1 (the
// staged chain is the default: dycore.h del6_tiled_modes).
//
// The staged form (dycore.h) runs Del6A (A = L q on is-2..ie+2), Del6B (B = -L A on is-1..ie+1) and the consumer's del6_increment, and A
// and B make a round trip through HBM.  Here one workgroup owns a 64 x 16 block of cells of one level of one tile: it loads q with a halo
// of 3 into LDS (70 x 22 doubles; tangent mode: a value and a tangent plane), forms A and B in LDS on the shrinking rectangles -- two
// planes in turn, B over q -- and writes the increment alone.  The order is a scalar of the block (c.lev[k-1]): a level of order 0 or 1
// runs the shorter chain in the same launch.  The arithmetic is lap_corner's, Del6BD's and del6_increment's in their order, so the host
// emulation agrees with the staged launches bit for bit.  Corner halo: every difference reads its operand through copy_corners' x-view
// (x-differences) or y-view (y-differences), edges.h corner_map on the cell's face indices; the source of a view lies within three cells
// of the corner on the inner side, i.e. inside the tile of every block that holds a corner-halo cell it needs (a view that falls outside
// the tile belongs to a value no output of the block depends on and reads as zero).  del6_u, del6_v and rarea come from memory, from
// indices clamped into the plane.
//
// The adjoint is the closed-form transpose in the same tiles.  With R = diag(rarea) and S the symmetric face-weighted difference
// (S t)(c) = sum over the four faces f of c of del6(f) (t(neighbour) - t(c)), L = R S and the increment is damp R S q, -damp R S R S q,
// damp R S R S R S q for order 0, 1, 2 (every neighbour a pass reads lies inside the ring the pass before it was formed on, so no
// restriction enters but the one onto is..ie, js..je at the end).  Transposed: q_ad = S R S R S R (damp y_ad), passes in reverse order,
// y_ad zero outside is..ie, js..je; a block owns 64 x 16 cells of q_ad over is-3..ie+3, js-3..je+3 and loads R damp y_ad with a halo of 3.
// Every element has one owner, no atomics; in store mode (dycore.h plan_adjoint) it stores, zeros outside its reach.  The transposition
// holds where no corner view acts: the adjoint launch serves the periodic tile and the sub-face tiles without a cube corner; on tiles
// with one the staged adjoint runs (Op::modes, dycore.h).
#pragma once
#include "stages.h"
#include "tiled.h"

namespace fv3 {

struct Del6Args {
  Fld q, out;           // the damped field (w, zh), the increment (dw, the damping term of update_dz_d)
  Rect ro;              // is..ie, js..je
  int nk = 0;
  int sel = 0;          // 0: w (nord_w, (damp_w da_min_c)^(nord_w+1)), 1: heights (nord_v, damp_vt raw)
  unsigned wmask = 0;   // adjoint: q_ad is stored instead of accumulated (dycore.h plan_adjoint) ...
  Rect wrect{1, 0, 1, 0};   // ... over its reach and this rectangle
  HD Rect reach() const { return Rect{ro.i0 - 3, ro.i1 + 3, ro.j0 - 3, ro.j1 + 3}; }
};
FV3LM_LINK void run_del6(Exec& ex, int mode, const Del6Args& a0, const Ctx& c);

// order and coefficient of a level (DswDwT / UpdateDzDT of stages.h); false: the level is not damped
HD bool del6_level(const LevelParams& l, int sel, double da_min_c, int& nord, double& damp) {
  if (sel == 0) {
    if (!(l.damp_w > 1.e-5)) return false;
    nord = l.nord_w;
    double d4 = l.damp_w * da_min_c;
    if (nord == 1) d4 = d4 * d4;
    if (nord == 2) d4 = d4 * d4 * d4;
    damp = d4;
    return true;
  }
  if (!(l.damp_vt > 1.e-5)) return false;
  nord = l.nord_v; damp = l.damp_vt;
  return true;
}
// q read, increment written (x2 in the tangent mode; adjoint: y_ad read, q_ad read-modify-written)
inline double del6_bytes(const Del6Args& a, const Geom& g, int mode) {
  const double cells = double(a.ro.i1 - a.ro.i0 + 1) * double(a.ro.j1 - a.ro.j0 + 1) * g.ntile * a.nk;
  return 8. * cells * (mode == MODE_NL ? 2. : mode == MODE_TL ? 4. : 3.);
}
}  // namespace fv3

#if !defined(FV3LM_SPLIT_BUILD) || defined(FV3LM_IMPL_DEL6)
namespace fv3 {
#ifndef FV3LM_DEL6_THREADS
#define FV3LM_DEL6_THREADS 256
#endif
constexpr int D6_W = 64, D6_H = 16, D6_HALO = 3;
constexpr int D6_QW = D6_W + 2 * D6_HALO, D6_QH = D6_H + 2 * D6_HALO, D6_NQ = D6_QW * D6_QH;      // 70 x 22
constexpr int D6_NT = 2 * D6_NQ;                                                                  // two planes per component

// metric of cell / face (i, j), the index clamped into the padded plane
DEV double d6_met(const double* p, const Ctx& c, int tile, int i, int j) {
  const Geom& g = c.g;
  i = i < g.isd() ? g.isd() : i > g.ied() + 1 ? g.ied() + 1 : i;
  j = j < g.jsd() ? g.jsd() : j > g.jed() + 1 ? g.jed() + 1 : j;
  return p[c.mi(tile, i, j)];
}

// One block of the forward modes: cells I0..I1 x J0..J1 of level k of one tile, blocks laid over Qr = a.ro.
template <class T, int NTH>
DEV void del6_block(const Del6Args& a, const Ctx& c, const Rect& Qr, int tile, int k, int bx, int by, double* lds, int tid) {
  typedef TpfIO<T> IO;
  const Geom& g = c.g;
  const TileBlk B = tile_blk(Qr, bx, by, D6_W, D6_H);
  const int I0 = B.I0, I1 = B.I1, J0 = B.J0, J1 = B.J1, X0 = I0 - D6_HALO, Y0 = J0 - D6_HALO;
  double* const P0 = lds; double* const P1 = lds + D6_NQ;
  int nord = 0; double damp = 0.;
  const bool on = del6_level(c.lev[k - 1], a.sel, c.m.da_min_c, nord, damp);
  if (!on) {
    TPF_LOOP(e, D6_W * D6_H) {
      const int i = I0 + e % D6_W, j = J0 + e / D6_W;
      if (i <= I1 && j <= J1) IO::st(a.out, fld_at(g, a.out, tile, k, i, j), T(0.));
    }
    return;
  }
  // element of a plane through the view of the difference's direction (dir = 0: as stored)
  auto rd = [&](const double* P, int dir, int i, int j) -> T {
    if (dir) corner_map(g, dir, i, j);
    const int x = i - X0, y = j - Y0;
    if (x < 0 || x >= D6_QW || y < 0 || y >= D6_QH) return T(0.);
    return IO::lget(P, D6_NT, y * D6_QW + x);
  };
  auto lap = [&](const double* P, int i, int j) -> T {      // stages.h lap_corner
    T fxa = d6_met(c.m.del6_v, c, tile, i, j) * (rd(P, 1, i - 1, j) - rd(P, 1, i, j));
    T fxb = d6_met(c.m.del6_v, c, tile, i + 1, j) * (rd(P, 1, i, j) - rd(P, 1, i + 1, j));
    T fya = d6_met(c.m.del6_u, c, tile, i, j) * (rd(P, 2, i, j - 1) - rd(P, 2, i, j));
    T fyb = d6_met(c.m.del6_u, c, tile, i, j + 1) * (rd(P, 2, i, j) - rd(P, 2, i, j + 1));
    return (fxa - fxb + (fya - fyb)) * d6_met(c.m.rarea, c, tile, i, j);
  };
  // ---- q on [I0-3, I1+3] x [J0-3, J1+3]
  TPF_LOOP(e, D6_NQ) {
    const int i = X0 + e % D6_QW, j = Y0 + e / D6_QW;
    if (i <= I1 + D6_HALO && j <= J1 + D6_HALO) IO::lset(P0, D6_NT, e, IO::ld(a.q, fld_at(g, a.q, tile, k, i, j)));
  }
  TPF_SYNC();
  const double* src = P0;
  if (nord >= 1) {      // ---- A = L q on the ring of 2 (Del6A)
    TPF_LOOP(e, D6_NQ) {
      const int i = X0 + e % D6_QW, j = Y0 + e / D6_QW;
      if (i >= I0 - 2 && i <= I1 + 2 && j >= J0 - 2 && j <= J1 + 2) IO::lset(P1, D6_NT, e, lap(P0, i, j));
    }
    TPF_SYNC();
    src = P1;
  }
  if (nord == 2) {      // ---- B = -L A on the ring of 1 (Del6B), over q
    TPF_LOOP(e, D6_NQ) {
      const int i = X0 + e % D6_QW, j = Y0 + e / D6_QW;
      if (i >= I0 - 1 && i <= I1 + 1 && j >= J0 - 1 && j <= J1 + 1) IO::lset(P0, D6_NT, e, -1.0 * lap(P1, i, j));
    }
    TPF_SYNC();
    src = P0;
  }
  // ---- the increment (stages.h del6_increment)
  TPF_LOOP(e, D6_W * D6_H) {
    const int i = I0 + e % D6_W, j = J0 + e / D6_W;
    if (i > I1 || j > J1) continue;
    const double dv0 = d6_met(c.m.del6_v, c, tile, i, j), dv1 = d6_met(c.m.del6_v, c, tile, i + 1, j);
    const double du0 = d6_met(c.m.del6_u, c, tile, i, j), du1 = d6_met(c.m.del6_u, c, tile, i, j + 1);
    T fxa, fxb, fya, fyb;
    if (nord == 0) {
      fxa = dv0 * (rd(src, 0, i - 1, j) - rd(src, 0, i, j)); fxb = dv1 * (rd(src, 0, i, j) - rd(src, 0, i + 1, j));
      fya = du0 * (rd(src, 0, i, j - 1) - rd(src, 0, i, j)); fyb = du1 * (rd(src, 0, i, j) - rd(src, 0, i, j + 1));
    } else {
      fxa = dv0 * (rd(src, 0, i, j) - rd(src, 0, i - 1, j)); fxb = dv1 * (rd(src, 0, i + 1, j) - rd(src, 0, i, j));
      fya = du0 * (rd(src, 0, i, j) - rd(src, 0, i, j - 1)); fyb = du1 * (rd(src, 0, i, j + 1) - rd(src, 0, i, j));
    }
    IO::st(a.out, fld_at(g, a.out, tile, k, i, j), damp * ((fxa - fxb + (fya - fyb)) * d6_met(c.m.rarea, c, tile, i, j)));
  }
}

// One block of the adjoint: the cells I0..I1 x J0..J1 of q_ad, blocks laid over Qr (the reach, widened in store mode).
template <int NTH>
DEV void del6_ad_block(const Del6Args& a, const Ctx& c, const Rect& Qr, int tile, int k, int bx, int by, double* lds, int tid) {
  const Geom& g = c.g;
  const TileBlk B = tile_blk(Qr, bx, by, D6_W, D6_H);
  const int I0 = B.I0, I1 = B.I1, J0 = B.J0, J1 = B.J1, X0 = I0 - D6_HALO, Y0 = J0 - D6_HALO;
  const Rect rq = a.reach();
  double* P0 = lds; double* P1 = lds + D6_NQ;
  int nord = 0; double damp = 0.;
  const bool on = del6_level(c.lev[k - 1], a.sel, c.m.da_min_c, nord, damp);
  if (!on) {
    if (a.wmask & 1u) {
      TPF_LOOP(e, D6_W * D6_H) {
        const int i = I0 + e % D6_W, j = J0 + e / D6_W;
        if (i <= I1 && j <= J1) a.q.p[fld_at(g, a.q, tile, k, i, j)] = 0.;
      }
    }
    return;
  }
  const double cf = nord == 1 ? -damp : damp;
  // S t at an element whose four neighbours lie inside the plane of 70 x 22
  auto sdiff = [&](const double* P, int e, int i, int j) -> double {
    const double t0 = P[e];
    return d6_met(c.m.del6_v, c, tile, i, j) * (P[e - 1] - t0) + d6_met(c.m.del6_v, c, tile, i + 1, j) * (P[e + 1] - t0) +
           (d6_met(c.m.del6_u, c, tile, i, j) * (P[e - D6_QW] - t0) + d6_met(c.m.del6_u, c, tile, i, j + 1) * (P[e + D6_QW] - t0));
  };
  // ---- t = R (damp y_ad) on the block with a halo of 3, zero outside is..ie, js..je
  TPF_LOOP(e, D6_NQ) {
    const int i = X0 + e % D6_QW, j = Y0 + e / D6_QW;
    P0[e] = a.ro.has(i, j) ? d6_met(c.m.rarea, c, tile, i, j) * (cf * a.out.p[fld_at(g, a.out, tile, k, i, j)]) : 0.;
  }
  TPF_SYNC();
  // ---- nord times t <- R S t, valid on a halo one narrower each time
  for (int n = 1; n <= nord; ++n) {
    TPF_LOOP(e, D6_NQ) {
      const int x = e % D6_QW, y = e / D6_QW;
      P1[e] = (x >= n && x < D6_QW - n && y >= n && y < D6_QH - n) ? d6_met(c.m.rarea, c, tile, X0 + x, Y0 + y) * sdiff(P0, e, X0 + x, Y0 + y) : 0.;
    }
    TPF_SYNC();
    double* t_ = P0; P0 = P1; P1 = t_;
  }
  // ---- q_ad = S t (store rules of exec.h body_ad_joint)
  TPF_LOOP(e, D6_W * D6_H) {
    const int x = e % D6_W, r = e / D6_W, i = I0 + x, j = J0 + r;
    if (i > I1 || j > J1) continue;
    const bool in = rq.has(i, j);
    if (!in && !(a.wmask & 1u)) continue;
    const double acc = sdiff(P0, (r + D6_HALO) * D6_QW + x + D6_HALO, i, j);
    double* q = &a.q.p[fld_at(g, a.q, tile, k, i, j)];
    if (a.wmask & 1u) *q = in ? acc : 0.; else *q += acc;
  }
}
// the block descriptors (tiled.h)
template <class T, int N> struct Del6Fwd {
  typedef Del6Args Args; static constexpr int NTH = N; static constexpr size_t LDS_BYTES = (size_t)D6_NT * 8 * TpfIO<T>::NC;      // 24.6 KB, tangent 49.3 KB
  DEV static void block(const Args& a, const Ctx& c, const Rect& Qr, int tile, int k, int bx, int by, double* lds, int tid) { del6_block<T, N>(a, c, Qr, tile, k, bx, by, lds, tid); }
};
template <int N> struct Del6Ad {
  typedef Del6Args Args; static constexpr int NTH = N; static constexpr size_t LDS_BYTES = (size_t)D6_NT * 8;
  DEV static void block(const Args& a, const Ctx& c, const Rect& Qr, int tile, int k, int bx, int by, double* lds, int tid) { del6_ad_block<N>(a, c, Qr, tile, k, bx, by, lds, tid); }
};

FV3LM_LINK void run_del6(Exec& ex, int mode, const Del6Args& a0, const Ctx& c) {
  Del6Args a = a0;
  for (Fld* f : {&a.q, &a.out}) *f = ex.sh(*f);
  if (ex.no_wmask) a.wmask = 0;
  if (mode == MODE_AD && !a.q.p) return;
  const Rect Qr = mode == MODE_AD ? ad_launch_rect(a.reach(), a.wmask & 1u, a.wrect, c.g) : a.ro;
  const int nbx = tiled_blocks(Qr.i0, Qr.i1, D6_W), nby = tiled_blocks(Qr.j0, Qr.j1, D6_H);
  const double bytes = del6_bytes(a, c.g, mode);
  constexpr int NTH = tiled_nth(FV3LM_DEL6_THREADS);
  if (mode == MODE_TL) run_tiled<Del6Fwd<Dual, NTH>>(ex, "Del6", mode_tag(mode), bytes, Qr, nbx, nby, a, c);
  else if (mode == MODE_NL) run_tiled<Del6Fwd<double, NTH>>(ex, "Del6", mode_tag(mode), bytes, Qr, nbx, nby, a, c);
  else run_tiled<Del6Ad<NTH>>(ex, "Del6", mode_tag(mode), bytes, Qr, nbx, nby, a, c);
}

}  // namespace fv3
#endif
