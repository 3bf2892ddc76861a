// fv3lm-hip: external-mode divergence damping of the hydrostatic acoustic step, flagstruct%d_ext > 0 (fv3lm_set_external_damping).
//
// Per acoustic step the reference (dyn_core_nlm.F90:641-644, :678-684, :707-727; tangent dyn_core_tlm.F90:937-943, :999-1007,
// :1031-1060) averages the step's input delp to the cell corners with a2b_ord2, takes from d_sw the corner divergence BEFORE any damping
// (sw_core_nlm.F90:1264-1340 on a level with nord_k = 0, the copy of c_sw's divg_d of :1350-1355 otherwise), forms the delp-weighted
// column mean
//     divg2 = d_ext da_min_c  (sum_k wk_k vt_k) / (sum_k wk_k)
// and hands it to one_grad_p, where wk2 = divg2(i,j) - divg2(i+1,j) and wk1 = divg2(i,j) - divg2(i,j+1) enter the brackets of the u and
// v updates (dyn_core_nlm.F90:1713-1741, :1762-1775).
//
// Here: a2b_ord2 is a stage (A2bOrd2D below: nonlinear, tangent and gather adjoint from exec.h, face-edge strips from add_face), the
// column mean is one thread per corner column with the lanes along i (DextColFn), its adjoint a gather over (i, j, k) that STORES the
// adjoints of the corner delp and of the divergence over whole padded planes (DextColAdFn; no atomics, nothing to clear beforehand),
// and the adjoint of divg2 itself is gathered per corner column from the adjoints of the step's winds (DextGradAdFn).  one_grad_p
// reads divg2 as a one-level operand beside its stage inputs (stages.h OneGradPT<true>).
//
// split_damp: the VALUE of the divergence is the trajectory pass's (nord_k; dampt.h DampTFinal leaves its nord_k = 0 divergence in
// `dvt`), the TANGENT the perturbation pass's (nord_k_pert; DdB / divg_d), sw_core_tlm.F90:2341-2369 -- the two may take different
// branches on one level.
#pragma once
#include "stages.h"

namespace fv3 {

// a2b_ord2 (a2b_edge_nlm.F90:677-798, replace = .false.): the 4-point mean; on a cube edge the edge_w/e/s/n-weighted mean of the two
// 2-point averages across the edge (:735-773); r3 x the three cells around a cube corner (:729-733)
struct A2bOrd2D {
  STAGE_COMMON("A2bOrd2", 1, 1)   // in: q (cell centres, halo ring of 1)   out: q at the corners
  HD static constexpr Box box(int) { return Box{-1, 0, -1, 0, 0, 0}; }
  template <bool EDGE, class T, class A>
  HD void eval_e(const A& a, const Ctx& c, int tile, int i, int j, int k, T* o) const {
    constexpr bool F = EDGE; const int npx = c.g.nx + 1, npy = c.g.ny + 1;
    const bool ex = F && (i == 1 || i == npx), ey = F && (j == 1 || j == npy);
    if (ex && ey) {
      const int ci = (i == 1) ? i : i - 1, oi = (i == 1) ? i - 1 : i, cj = (j == 1) ? j : j - 1, oj = (j == 1) ? j - 1 : j;
      o[0] = (1. / 3.) * (IN(0, ci, cj) + IN(0, ci, oj) + IN(0, oi, cj));
      return;
    }
    if (ex) {
      const double w = c.m.edge[((size_t)tile * 4 + (i == 1 ? 0 : 1)) * c.g.pj + (j - c.g.j0 + c.g.ng)];
      o[0] = w * (0.5 * (IN(0, i - 1, j - 1) + IN(0, i, j - 1))) + (1. - w) * (0.5 * (IN(0, i - 1, j) + IN(0, i, j)));
      return;
    }
    if (ey) {
      const double w = c.m.edge[((size_t)tile * 4 + (j == 1 ? 2 : 3)) * c.g.pj + (i - c.g.i0 + c.g.ng)];
      o[0] = w * (0.5 * (IN(0, i - 1, j - 1) + IN(0, i - 1, j))) + (1. - w) * (0.5 * (IN(0, i, j - 1) + IN(0, i, j)));
      return;
    }
    o[0] = 0.25 * (IN(0, i - 1, j - 1) + IN(0, i, j - 1) + IN(0, i - 1, j) + IN(0, i, j));
  }
};

struct DextArgs {
  Geom g; const LevelParams* lev; double cfac;   // d_ext * da_min_c
  Fld wk;                  // corner delp (A2bOrd2D)
  Fld dc, dg;              // the nord = 0 divergence (DdB) and c_sw's divg_d (null while no level has nord > 0)
  const double* dvt;       // split_damp with differing passes: the trajectory's nord_k = 0 divergence (dampt.h), else null
  Fld d2, ws;              // one level: divg2 and the column sum of the corner delp
  Fld uo, vo;              // the step's wind outputs (adjoint of divg2)
  const double *rdx, *rdy;
  int tl, store;
  // the divergence of level k: where its value and where its tangent / adjoint live
  HD const double* val_of(int k) const {
    const LevelParams& l = lev[k - 1];
    if (dvt) return l.nord == 0 ? dvt : dg.t;
    return l.nord_p == 0 ? dc.t : dg.t;
  }
  HD bool pert_dc(int k) const { return lev[k - 1].nord_p == 0; }
  HD Rect corners() const { return Rect{g.is(), g.ie() + 1, g.js(), g.je() + 1}; }
};

// divg2 and W = sum_k wk of one corner column (dyn_core_nlm.F90:707-727), tangent by the quotient rule (dyn_core_tlm.F90:1031-1056).
// z = tile.  Every level's plane is read along i by consecutive lanes.
struct DextColFn {
  DextArgs a;
  HD void operator()(int i, int j, int tile) const {
    const Geom& g = a.g;
    const size_t pt = g.idx(i, j), p2 = (size_t)tile * g.plane + pt;
    double W = 0., S = 0., dW = 0., dS = 0.;
    for (int k = 1; k <= g.npz; ++k) {
      const size_t n = (size_t)(tile * g.npz + k - 1) * g.plane + pt;
      const double wk = a.wk.t[n], vt = a.val_of(k)[n];
      W += wk; S += wk * vt;
      if (a.tl) { const double dwk = a.wk.p[n], dvt_ = (a.pert_dc(k) ? a.dc.p : a.dg.p)[n]; dW += dwk; dS += dwk * vt + wk * dvt_; }
    }
    const double m = S / W;
    a.d2.t[p2] = a.cfac * m; a.ws.t[p2] = W;
    if (a.tl) a.d2.p[p2] = a.cfac * (dS - m * dW) / W;
  }
};

// Adjoint of the column mean as a gather: point (i, j, k) of the corner delp and of the divergence reads the 2-D adjoint of divg2 and the
// stored divg2, W.  store: whole padded planes are written (zeros outside the corners, zeros in the divergence array the level does not
// use), so nothing is cleared beforehand and every adjoint is written once (dycore.h plan_adjoint, Op::ad_store); otherwise (a kernel
// group run on its own) the contributions are added.
struct DextColAdFn {
  DextArgs a;
  HD void operator()(int i, int j, int z) const {
    const Geom& g = a.g;
    const int tile = z / g.npz, k = 1 + z % g.npz;
    const size_t pt = g.idx(i, j), n = (size_t)z * g.plane + pt;
    const bool in = a.corners().has(i, j);
    double wad = 0., vad = 0.;
    if (in) {
      const size_t p2 = (size_t)tile * g.plane + pt;
      const double coef = a.cfac / a.ws.t[p2] * a.d2.p[p2];
      wad = coef * (a.val_of(k)[n] - a.d2.t[p2] / a.cfac);
      vad = coef * a.wk.t[n];
    }
    double* tgt = a.pert_dc(k) ? a.dc.p : a.dg.p;
    double* oth = a.pert_dc(k) ? a.dg.p : a.dc.p;
    if (a.store) { a.wk.p[n] = wad; tgt[n] = vad; if (oth) oth[n] = 0.; }
    else if (in) { a.wk.p[n] += wad; tgt[n] += vad; }
  }
};

// Adjoint of divg2 from the adjoints of the step's winds: u = rdx (wk2 + ...), wk2 = divg2(i,j) - divg2(i+1,j) on (is:ie, js:je+1);
// v = rdy (wk1 + ...), wk1 = divg2(i,j) - divg2(i,j+1) on (is:ie+1, js:je).  One thread per corner column, stored.
struct DextGradAdFn {
  DextArgs a;
  HD void operator()(int i, int j, int tile) const {
    const Geom& g = a.g;
    const size_t mb = (size_t)tile * g.plane;
    const bool u0 = i <= g.ie(), u1 = i - 1 >= g.is(), v0 = j <= g.je(), v1 = j - 1 >= g.js();
    const size_t p00 = g.idx(i, j), pw = u1 ? g.idx(i - 1, j) : p00, ps = v1 ? g.idx(i, j - 1) : p00;
    const double rx0 = u0 ? a.rdx[mb + p00] : 0., rx1 = u1 ? a.rdx[mb + pw] : 0., ry0 = v0 ? a.rdy[mb + p00] : 0., ry1 = v1 ? a.rdy[mb + ps] : 0.;
    double acc = 0.;
    for (int k = 1; k <= g.npz; ++k) {
      const size_t b = (size_t)(tile * g.npz + k - 1) * g.plane;
      acc += rx0 * a.uo.p[b + p00] - rx1 * a.uo.p[b + pw] + (ry0 * a.vo.p[b + p00] - ry1 * a.vo.p[b + ps]);
    }
    a.d2.p[mb + p00] = acc;
  }
};

inline void run_dext_col(Exec& ex, int mode, const DextArgs& a0) {
  DextArgs a = a0;
  const Geom& g = a.g;
  const double fld = 8. * double(g.ie() - g.is() + 2) * double(g.je() - g.js() + 2) * g.ntile * g.npz;      // one field over the corners
  if (mode == MODE_AD) {
    a.store = ex.no_wmask ? 0 : 1;
    // reads vt, the corner delp (and, per level, the planes of divg2, W and the 2-D adjoint: 3 / npz of a field); writes the two adjoints
    // and zeros in the divergence array the level does not use, over whole padded planes
    const double pad = 8. * double(g.plane) * g.ntile * g.npz;
    for_points(ex, Rect{g.isd(), g.ied() + 1, g.jsd(), g.jed() + 1}, g.ntile * g.npz, DextColAdFn{a}, "dext_col.ad", (2. + 3. / g.npz) * fld + (a.dg.p ? 3. : 2.) * pad);
    return;
  }
  a.tl = mode == MODE_TL;
  for_points(ex, a.corners(), g.ntile, DextColFn{a}, mode == MODE_NL ? "dext_col.nl" : "dext_col.tl", (a.tl ? 4. : 2.) * fld);
}
inline void run_dext_grad_ad(Exec& ex, const DextArgs& a) {
  const Geom& g = a.g;
  for_points(ex, a.corners(), g.ntile, DextGradAdFn{a}, "dext_grad.ad", 16. * double(g.tx + 1) * double(g.ty + 1) * g.ntile * g.npz);
}

}  // namespace fv3
