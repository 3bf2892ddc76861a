// fv3lm-hip: what the column schemes that follow the reference's double results literally share (bldriver.h, convection.h, cloud.h).
//
// FV3LM_LITERAL switches contraction into fused multiply-adds off for the function whose body it opens: the fixtures of these schemes
// are the reference's double results in the routine's order of operations.  It is scoped to the function, so nothing outlives a header.
//
// The routines of convection.h and cloud.h are written ONCE on a generic scalar T and run as values (double), tangent (RD, a dual
// number) and adjoint (RV, a taped scalar on the Tape of coltape.h).  Both scalars are this file's own because their operators must be
// compiled with contraction off (the pragma acts where an operator is defined, and Dual / TV of core.h / coltape.h serve kernels that
// are built with it on).  Also here: the work vectors of a column in the three scalars (RW, RArr, LitVecs), the packed columns of a
// slot (ColView), the work memory of a batch of columns (ColWork) and the walk back over the tape of one segment of the adjoint.
#pragma once
#include "coltape.h"

#if defined(__clang__)
#define FV3LM_LITERAL _Pragma("clang fp contract(off)")
#else
#define FV3LM_LITERAL
#endif

namespace fv3 {

// ---- the two scalars ---------------------------------------------------------------------------------------------------------------
struct RD {
  double v, d;
  HD RD() : v(0.), d(0.) {}
  HD RD(double v_) : v(v_), d(0.) {}
  HD RD(double v_, double d_) : v(v_), d(d_) {}
};
HD RD operator+(RD a, RD b) { FV3LM_LITERAL return RD(a.v + b.v, a.d + b.d); }
HD RD operator-(RD a, RD b) { FV3LM_LITERAL return RD(a.v - b.v, a.d - b.d); }
HD RD operator*(RD a, RD b) { FV3LM_LITERAL return RD(a.v * b.v, a.d * b.v + a.v * b.d); }
HD RD operator/(RD a, RD b) { FV3LM_LITERAL const double q = a.v / b.v; return RD(q, (a.d - q * b.d) / b.v); }
HD RD operator-(RD a) { FV3LM_LITERAL return RD(-a.v, -a.d); }
HD RD operator+(RD a, double b) { FV3LM_LITERAL return RD(a.v + b, a.d); }
HD RD operator+(double a, RD b) { FV3LM_LITERAL return RD(a + b.v, b.d); }
HD RD operator-(RD a, double b) { FV3LM_LITERAL return RD(a.v - b, a.d); }
HD RD operator-(double a, RD b) { FV3LM_LITERAL return RD(a - b.v, -b.d); }
HD RD operator*(RD a, double b) { FV3LM_LITERAL return RD(a.v * b, a.d * b); }
HD RD operator*(double a, RD b) { FV3LM_LITERAL return RD(a * b.v, a * b.d); }
HD RD operator/(RD a, double b) { FV3LM_LITERAL return RD(a.v / b, a.d / b); }
HD RD operator/(double a, RD b) { FV3LM_LITERAL const double q = a / b.v; return RD(q, -q * b.d / b.v); }

// taped value (value, scale, id): its derivative with respect to tape variable id is scale (as TV of coltape.h)
struct RV {
  double v, s; int id; Tape* t;
  HD RV() : v(0.), s(1.), id(-1), t(nullptr) {}
  HD RV(double v_) : v(v_), s(1.), id(-1), t(nullptr) {}
  HD RV(double v_, double s_, int id_, Tape* t_) : v(v_), s(s_), id(id_), t(t_) {}
};
HD RV rv2(const RV& a, const RV& b, double v, double pa, double pb) { FV3LM_LITERAL
  if (a.id >= 0 && b.id >= 0) return RV(v, 1., a.t->push(a.id, b.id, pa * a.s, pb * b.s), a.t);
  if (a.id >= 0) return RV(v, pa * a.s, a.id, a.t);
  if (b.id >= 0) return RV(v, pb * b.s, b.id, b.t);
  return RV(v);
}
HD RV rv1n(const RV& a, double v, double pa) { FV3LM_LITERAL return a.id < 0 ? RV(v) : RV(v, 1., a.t->push(a.id, -1, pa * a.s, 0.), a.t); }
HD RV rv1l(const RV& a, double v, double pa) { FV3LM_LITERAL return a.id < 0 ? RV(v) : RV(v, pa * a.s, a.id, a.t); }
HD RV operator+(const RV& a, const RV& b) { FV3LM_LITERAL return rv2(a, b, a.v + b.v, 1., 1.); }
HD RV operator-(const RV& a, const RV& b) { FV3LM_LITERAL return rv2(a, b, a.v - b.v, 1., -1.); }
HD RV operator*(const RV& a, const RV& b) { FV3LM_LITERAL return rv2(a, b, a.v * b.v, b.v, a.v); }
HD RV operator/(const RV& a, const RV& b) { FV3LM_LITERAL
  const double q = a.v / b.v;
  if (b.id < 0) return rv1l(a, q, 1. / b.v);
  if (a.id < 0) return rv1n(b, q, -q / b.v);
  return rv2(a, b, q, 1. / b.v, -q / b.v);
}
HD RV operator-(const RV& a) { FV3LM_LITERAL return rv1l(a, -a.v, -1.); }
HD RV operator+(const RV& a, double b) { FV3LM_LITERAL return rv1l(a, a.v + b, 1.); }
HD RV operator+(double a, const RV& b) { FV3LM_LITERAL return rv1l(b, a + b.v, 1.); }
HD RV operator-(const RV& a, double b) { FV3LM_LITERAL return rv1l(a, a.v - b, 1.); }
HD RV operator-(double a, const RV& b) { FV3LM_LITERAL return rv1l(b, a - b.v, -1.); }
HD RV operator*(const RV& a, double b) { FV3LM_LITERAL return rv1l(a, a.v * b, b); }
HD RV operator*(double a, const RV& b) { FV3LM_LITERAL return rv1l(b, a * b.v, a); }
HD RV operator/(const RV& a, double b) { FV3LM_LITERAL return rv1l(a, a.v / b, 1. / b); }
HD RV operator/(double a, const RV& b) { FV3LM_LITERAL const double q = a / b.v; return rv1n(b, q, -q / b.v); }

HD double rval(double a) { FV3LM_LITERAL return a; }
HD double rval(const RD& a) { FV3LM_LITERAL return a.v; }
HD double rval(const RV& a) { FV3LM_LITERAL return a.v; }
// a nonlinear function of one argument: its value and its derivative at the argument
HD double run1(double, double v, double) { FV3LM_LITERAL return v; }
HD RD run1(const RD& a, double v, double p) { FV3LM_LITERAL return RD(v, p * a.d); }
HD RV run1(const RV& a, double v, double p) { FV3LM_LITERAL return rv1n(a, v, p); }

template <class T> struct RW;
template <> struct RW<double> {
  static constexpr int W = 1;
  HD static double get(const ColWs& w, int s, int k, Tape*) { FV3LM_LITERAL return w.at(s, k); }
  HD static void set(const ColWs& w, int s, int k, double x) { FV3LM_LITERAL w.at(s, k) = x; }
};
template <> struct RW<RD> {
  static constexpr int W = 2;
  HD static RD get(const ColWs& w, int s, int k, Tape*) { FV3LM_LITERAL return RD(w.at(2 * s, k), w.at(2 * s + 1, k)); }
  HD static void set(const ColWs& w, int s, int k, const RD& x) { FV3LM_LITERAL w.at(2 * s, k) = x.v; w.at(2 * s + 1, k) = x.d; }
};
template <> struct RW<RV> {
  static constexpr int W = 2;
  HD static RV get(const ColWs& w, int s, int k, Tape* t) { FV3LM_LITERAL return RV(w.at(2 * s, k), 1., (int)w.at(2 * s + 1, k), t); }
  HD static void set(const ColWs& w, int s, int k, const RV& x) { FV3LM_LITERAL
    const int id = (x.id < 0 || x.s == 1.) ? x.id : x.t->push(x.id, -1, x.s, 0.);
    w.at(2 * s, k) = x.v; w.at(2 * s + 1, k) = (double)id;
  }
};
// vector s of the work space, level 1 .. lm + 1
template <class T> struct RArr {
  ColWs w; int s; Tape* t;
  HD T operator()(int k) const { FV3LM_LITERAL return RW<T>::get(w, s, k, t); }
  HD void set(int k, const T& x) const { FV3LM_LITERAL RW<T>::set(w, s, k, x); }
};
template <class T> struct LitVecs {
  ColWs w; Tape* t;
  HD RArr<T> operator()(int s) const { FV3LM_LITERAL return RArr<T>{w, s, t}; }
};

// ---- the packed columns of a slot and the columns of one launch -----------------------------------------------------------------
// A slot is ns vectors of lm + 1 levels, then per-column scalars, each [level][column] over all resident tiles at once: a column does
// not know where it lies, col = (tile ty + j) tx + i.
struct ColView {
  Geom g; int ntile, lm, ns;
  double* slot; size_t nc;
  const int* list; int first, n;    // the columns of this launch: list[first + m] (list null: first + m)
  HD double& S(int v, int l, size_t col) const { FV3LM_LITERAL return slot[((size_t)v * (lm + 1) + l) * nc + col]; }
  HD double& SC(int s, size_t col) const { FV3LM_LITERAL return slot[((size_t)ns * (lm + 1) + s) * nc + col]; }
  HD size_t fld(size_t col, int l) const { FV3LM_LITERAL      // level l (0-based) of the column in a padded field
    const size_t pc = (size_t)g.tx * g.ty, t = col / pc, r = col % pc;
    return (t * lm + l) * g.plane + g.idx(g.i0 + (int)(r % g.tx), g.j0 + (int)(r / g.tx));
  }
  HD size_t cmp(size_t col, int l) const { FV3LM_LITERAL const size_t pc = (size_t)g.tx * g.ty; return ((col / pc) * lm + l) * pc + col % pc; }      // host-compact
  HD size_t col_of(int m) const { FV3LM_LITERAL return list ? (size_t)list[first + m] : (size_t)(first + m); }
};
// work spaces, checkpoints and tape of one batch of columns, [vector][level][column of the batch] (stride nb), and the feature's two flags
struct ColWork { double *gw, *tw, *ew, *ck; TapeMem tape; int nb; int* flag; };

// ---- one segment of the adjoint on the tape ------------------------------------------------------------------------------------------
// element (v, l) of the state E becomes a leaf of the tape, read from the values ew into the taped work space tw
HD void lit_leaf(Tape& tape, const ColWs& tw, const ColWs& ew, int kw, int v, int l) { FV3LM_LITERAL
  RW<RV>::set(tw, v, l, RV(ew.at(v, l), 1., tape.push(-2 - (v * kw + l), -1, 0., 0.), &tape));
}
// the incoming adjoint of element (v, l) moves onto what the segment left there
HD void lit_seed(const Tape& tape, const ColWs& tw, const ColWs& eb, int v, int l) { FV3LM_LITERAL
  const double gb = eb.at(v, l);
  eb.at(v, l) = 0.;
  const int id = (int)tw.at(2 * v + 1, l);
  if (id >= 0 && gb != 0.) tape.ad(id) += gb;
}
// walk back: the leaves hand their adjoints to eb
HD void lit_walk_back(const Tape& tape, const ColWs& eb, int kw) { FV3LM_LITERAL
  for (int id = tape.n - 1; id >= 0; --id) {
    const size_t e = (size_t)id * tape.m.stride + tape.col;
    const double ad = tape.m.adj[e];
    if (ad == 0.) continue;
    const TapeIdx ix = tape.m.idx[e];
    if (ix.a <= -2) { const int q = -2 - ix.a; eb.at(q / kw, q % kw) += ad; continue; }
    const TapePart pt = tape.m.part[e];
    if (ix.a >= 0) tape.ad(ix.a) += pt.a * ad;
    if (ix.b >= 0) tape.ad(ix.b) += pt.b * ad;
  }
}

}  // namespace fv3
