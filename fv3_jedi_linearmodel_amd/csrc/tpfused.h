// fv3lm-hip: what the LDS-tiled forms of fv_tp_2d (tp_core_tlm.F90:83-236, _TLM :2123-2324) share -- the arguments of a launch, the
// rectangle its blocks are laid over, its algorithmic bytes -- and the values-only TRAJECTORY pass of the levels with split schemes.
//
// The staged form (dycore.h build_tp, FV3LM_TP_FUSED=0) runs the routine as seven launches + edge strips -- inner y-sweep, q_i, outer
// x-sweep, inner x-sweep, q_j, outer y-sweep, flux assembly -- with every intermediate (fy2, q_i, fxo, fx2, q_j, fyo) making a round trip
// through HBM.  In the tiled form one workgroup owns a block of cells of one level: it loads the block of q plus a 3-cell halo into LDS
// once, runs the four 1-D PPM sweeps and the two intermediate updates against LDS, and writes only the two fluxes.  Cube-face edges are
// the same four-cell edge values with other weights (edges.h ppm_w), the corner halo of the inner sweeps is read through the
// copy_corners view of the sweep direction (corner_map) inside the tile -- no strip launches.  The arithmetic is the staged stages' own
// (ppm_flux, the TpQi/TpQj/TpFlux formulas in their order), so both forms agree bit for bit.  Nonlinear and tangent launches: tp2.h;
// adjoint: tpad.h; here the trajectory pass, in the flattened-element layout of the first tiled kernel.
#pragma once
#include "stages.h"
#include "tiled.h"

namespace fv3 {

struct TpFusedArgs {
  Fld q, crx, cry, xfx, yfx, rax, ray, mx, my;   // inputs
  Fld mass, d2b;                                 // damping inputs (t == nullptr when unused)
  Fld d2b_t;                                     // the damping Laplacian of the trajectory pass of split levels (TpD2 with traj = 1)
  Fld fx, fy;                                    // outputs
  int hsel, dsel, use_mass, nk;
  // flux capacitors of d_sw (sw_core_tlm.F90:3000-3016): cx += crx, cy += cry, mfx += fx, mfy += fy folded into this launch
  // (t == nullptr: none).  do_acc is cleared for the adjoint's trajectory recompute, which must leave the accumulators alone.
  Fld acx, acy, amfx, amfy; int do_acc;
};
// the values-only trajectory pass of the levels with split schemes, in the nonlinear and the tangent mode alike
FV3LM_LINK void run_tp_traj(Exec& ex, const TpFusedArgs& a0, const Ctx& c);
// the rectangle the blocks of the fv_tp_2d launches are laid over: the tile's window of the face
inline Rect tp_window(const Geom& g) { return Rect{g.is(), g.ie(), g.js(), g.je()}; }
// algorithmic bytes of one nonlinear / tangent launch: 9 inputs (+ d2b, mass) read and 2 outputs written per cell (x2 in the tangent mode)
inline double tpf_bytes(const TpFusedArgs& a, const Geom& g, int mode) {
  const double cells = double(g.tx) * g.ty * g.ntile * a.nk, nin = 9. + (a.d2b.t ? 1. : 0.) + (a.mass.t ? 1. : 0.);
  return 8. * cells * (mode == MODE_TL ? 2. : 1.) * (nin + 2.);
}

}  // namespace fv3

#if !defined(FV3LM_SPLIT_BUILD) || defined(FV3LM_IMPL_TPFUSED)
namespace fv3 {
#ifndef FV3LM_TPF_H
#define FV3LM_TPF_H 16
#endif
// threads per block (measured on MI355X, C192L127 six faces, ms per nonlinear launch of this layout): 512: 1.43, 1024: 1.85; 64 x 8
// blocks were slower
#ifndef FV3LM_TPF_THREADS_NL
#define FV3LM_TPF_THREADS_NL 512
#endif
constexpr int TPF_W = 64, TPF_H = FV3LM_TPF_H;   // cells per block
constexpr int TPF_QW = TPF_W + 6, TPF_QH = TPF_H + 6;
constexpr int TPF_NQ = TPF_QW * TPF_QH, TPF_NFY2 = TPF_QW * (TPF_H + 1), TPF_NQI = TPF_QW * TPF_H, TPF_NFX2 = (TPF_W + 1) * TPF_QH,
              TPF_NQJ = TPF_W * TPF_QH, TPF_NT = TPF_NQ + TPF_NFY2 + TPF_NQI + TPF_NFX2 + TPF_NQJ;   // doubles of LDS
constexpr int TPF_THREADS_NL = FV3LM_TPF_THREADS_NL;

// an LDS array over the rectangle [i0, i0+w) x [j0, ...)
struct TpfTile {
  double* v; int i0, j0, w;
  DEV double get(int i, int j) const { return v[(j - j0) * w + (i - i0)]; }
  DEV void set(int i, int j, double x) const { v[(j - j0) * w + (i - i0)] = x; }
};

// One block: cells I0..I1 x J0..J1 of level k of one tile, blocks laid over the tile's window.
// The values-only second pass of a level whose trajectory scheme differs from the scheme the tangent / adjoint is taken of
// (split_hord, sw_core_tlm.F90:1664-1682): the whole chain again with the trajectory scheme (inner sweeps: 8 where it is 10,
// tp_core_tlm.F90:135-136) and the trajectory damping, fx.t / fy.t overwritten; levels without a split return at once.
template <int NTH>
DEV void tp_traj_block(const TpFusedArgs& a, const Ctx& c, int tile, int k, int bx, int by, double* lds, int tid) {
  if (!level_split(c.lev[k - 1], a.hsel, a.dsel)) return;
  const Geom& g = c.g;
  const int nx = g.nx, ny = g.ny;
  const bool face = g.face != 0;
  const int is = g.is(), ie = g.ie(), js = g.js(), je = g.je();      // the tile's window of the face (nx, ny: the FACE, for the edge formulas)
  const TileBlk B = tile_blk(Rect{is, ie, js, je}, bx, by, TPF_W, TPF_H);
  const int I0 = B.I0, I1 = B.I1, J0 = B.J0, J1 = B.J1;
  const bool lastx = I1 == ie, lasty = J1 == je;
  const size_t base = (size_t)(tile * a.nk + k - 1) * g.plane;
  auto at = [&](int i, int j) -> size_t { return base + g.idx(i, j); };
  // constant row pitches (the full block's), whatever the block's own width: index arithmetic by compile-time constants
  const TpfTile q{lds, I0 - 3, J0 - 3, TPF_QW}, fy2{lds + TPF_NQ, I0 - 3, J0, TPF_QW}, qi{lds + TPF_NQ + TPF_NFY2, I0 - 3, J0, TPF_QW},
      fx2{lds + TPF_NQ + TPF_NFY2 + TPF_NQI, I0, J0 - 3, TPF_W + 1}, qj{lds + TPF_NQ + TPF_NFY2 + TPF_NQI + TPF_NFX2, I0, J0 - 3, TPF_W};
  auto acc_flux = [&](const Fld& acc, size_t n, const double& f) { acc.t[n] += f; };
  const int iord = hord_traj_of(c.lev[k - 1], a.hsel), iord_in = iord == 10 ? 8 : iord;
  auto flux1d = [&](int io, bool ydir, int m, int n1, const auto& line, const auto& da, const double& cc) -> double { return ppm_flux_traj(io, face, ydir, m, n1, line, da, cc); };
  // ---- the block of q and its halo
  { constexpr int w = TPF_QW, n = w * TPF_QH;
    TPF_LOOP(e, n) { const int i = I0 - 3 + e % w, j = J0 - 3 + e / w; if (i <= I1 + 3 && j <= J1 + 3) q.set(i, j, a.q.t[at(i, j)]); } }
  TPF_SYNC();
  // ---- inner sweeps: fy2 = yppm(q) on the halo'd columns (copy_corners view 2), fx2 = xppm(q) on the halo'd rows (view 1)
  { constexpr int w = TPF_QW, n = w * (TPF_H + 1);
    TPF_LOOP(e, n) {
      const int i = I0 - 3 + e % w, j = J0 + e / w;
      if (i > I1 + 3 || j > J1 + 1) continue;
      auto line = [&](int jj) -> double { int ii = i, j2 = jj; if (face) corner_map(g, 2, ii, j2); return q.get(ii, j2); };
      const MetY da{c.m.dya, c, tile, i};
      const double cc = a.cry.t[at(i, j)];
      const double f = flux1d(iord_in, true, j, ny + 1, line, da, cc);
      fy2.set(i, j, f);
    } }
  { constexpr int w = TPF_W + 1, n = w * TPF_QH;
    TPF_LOOP(e, n) {
      const int i = I0 + e % w, j = J0 - 3 + e / w;
      if (i > I1 + 1 || j > J1 + 3) continue;
      auto line = [&](int ii) -> double { int i2 = ii, jj = j; if (face) corner_map(g, 1, i2, jj); return q.get(i2, jj); };
      const MetX da{c.m.dxa, c, tile, j};
      const double cc = a.crx.t[at(i, j)];
      const double f = flux1d(iord_in, false, i, nx + 1, line, da, cc);
      fx2.set(i, j, f);
    } }
  TPF_SYNC();
  // ---- q_i, q_j: the field advanced by the inner fluxes (tp_core_tlm.F90:149-159, :173-181)
  { constexpr int w = TPF_QW, n = w * TPF_H;
    TPF_LOOP(e, n) {
      const int i = I0 - 3 + e % w, j = J0 + e / w;
      if (i > I1 + 3 || j > J1) continue;
      const double f0 = a.yfx.t[at(i, j)] * fy2.get(i, j), f1 = a.yfx.t[at(i, j + 1)] * fy2.get(i, j + 1);
      const double x = (q.get(i, j) * MET(area, i, j) + f0 - f1) / a.ray.t[at(i, j)];
      qi.set(i, j, x);
    } }
  { constexpr int w = TPF_W, n = w * TPF_QH;
    TPF_LOOP(e, n) {
      const int i = I0 + e % w, j = J0 - 3 + e / w;
      if (i > I1 || j > J1 + 3) continue;
      const double f0 = a.xfx.t[at(i, j)] * fx2.get(i, j), f1 = a.xfx.t[at(i + 1, j)] * fx2.get(i + 1, j);
      const double x = (q.get(i, j) * MET(area, i, j) + f0 - f1) / a.rax.t[at(i, j)];
      qj.set(i, j, x);
    } }
  TPF_SYNC();
  // ---- outer sweeps and flux assembly (tp_core_tlm.F90:187-234; deln_flux :1918-2043 as in stages.h TpFlux)
  int nord; double dc; damp_of(c.lev[k - 1], a.dsel, nord, dc, false);
  const bool dmp = (a.dsel != DAMP_NONE) && (dc > 1.e-4) && damp_gate(c, c.lev[k - 1], a.dsel);
  double damp = 0.;
  if (dmp) damp = damp_pow(dc * c.m.da_min, nord);
  const Fld& d2 = a.d2b_t;
  { constexpr int w = TPF_W + 1, n = w * (TPF_H + 1);
    TPF_LOOP(e, n) {
      const int i = I0 + e % w, j = J0 + e / w;
      if (i > I1 + 1 || j > J1 + 1) continue;
      if (j <= J1 && (i <= I1 || lastx)) {          // fx(i,j)
        auto line = [&](int ii) -> double { return qi.get(ii, j); };
        const MetX da{c.m.dxa, c, tile, j};
        const double fo = flux1d(iord, false, i, nx + 1, line, da, a.crx.t[at(i, j)]);
        double f = 0.5 * (fo + fx2.get(i, j)) * a.mx.t[at(i, j)];
        if (dmp) {
          double f2;
          if (nord == 0) { f2 = MET(del6_v, i, j) * (q.get(i - 1, j) - q.get(i, j)); if (!a.use_mass) f2 = damp * f2; }
          else f2 = MET(del6_v, i, j) * (d2.t[at(i, j)] - d2.t[at(i - 1, j)]);
          if (a.use_mass) f = f + (0.5 * damp) * (a.mass.t[at(i - 1, j)] + a.mass.t[at(i, j)]) * f2;
          else f = f + f2;
        }
        a.fx.t[at(i, j)] = f;
        if (a.do_acc) acc_flux(a.amfx, at(i, j), f);      // flux capacitors on a split level: the first pass adds the tangents, this pass the values
      }
      if (i <= I1 && (j <= J1 || lasty)) {          // fy(i,j)
        auto line = [&](int jj) -> double { return qj.get(i, jj); };
        const MetY da{c.m.dya, c, tile, i};
        const double fo = flux1d(iord, true, j, ny + 1, line, da, a.cry.t[at(i, j)]);
        double f = 0.5 * (fo + fy2.get(i, j)) * a.my.t[at(i, j)];
        if (dmp) {
          double f2;
          if (nord == 0) { f2 = MET(del6_u, i, j) * (q.get(i, j - 1) - q.get(i, j)); if (!a.use_mass) f2 = damp * f2; }
          else f2 = MET(del6_u, i, j) * (d2.t[at(i, j)] - d2.t[at(i, j - 1)]);
          if (a.use_mass) f = f + (0.5 * damp) * (a.mass.t[at(i, j - 1)] + a.mass.t[at(i, j)]) * f2;
          else f = f + f2;
        }
        a.fy.t[at(i, j)] = f;
        if (a.do_acc) acc_flux(a.amfy, at(i, j), f);
      }
    } }
}

// the block descriptor (tiled.h); the block function takes the launch rectangle, the tile's window, from the geometry
template <int N> struct TpTrajBlk {
  typedef TpFusedArgs Args; static constexpr int NTH = N; static constexpr size_t LDS_BYTES = (size_t)TPF_NT * 8;
  DEV static void block(const Args& a, const Ctx& c, const Rect&, int tile, int k, int bx, int by, double* lds, int tid) { tp_traj_block<N>(a, c, tile, k, bx, by, lds, tid); }
};

FV3LM_LINK void run_tp_traj(Exec& ex, const TpFusedArgs& a0, const Ctx& c) {
  TpFusedArgs a = a0;
  for (Fld* f : {&a.q, &a.crx, &a.cry, &a.xfx, &a.yfx, &a.rax, &a.ray, &a.mx, &a.my, &a.mass, &a.d2b, &a.d2b_t, &a.fx, &a.fy, &a.acx, &a.acy, &a.amfx, &a.amfy}) *f = ex.sh(*f);
  a.do_acc = (a.acx.t && !ex.skip_accum) ? 1 : 0;
  const Rect Qr = tp_window(c.g);
  run_tiled<TpTrajBlk<tiled_nth(TPF_THREADS_NL)>>(ex, "TpFusedTraj", ".nl", 0., Qr, tiled_blocks(Qr.i0, Qr.i1, TPF_W), tiled_blocks(Qr.j0, Qr.j1, TPF_H), a, c);
}

}  // namespace fv3
#endif
