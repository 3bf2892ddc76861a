// fv3lm-hip: the bulk of a2b_ord4 (a2b_edge_tlm.F90:48-542) as ONE LDS-tiled launch per mode.
//
// The staged form (dycore.h build_a2b) runs the bulk as two launches, A2bA (q -> qx, qy) and A2bB (qx, qy -> qb), and the two
// intermediates make a round trip through HBM.  Away from the cube edges the routine is linear with constant weights:
//   qx(i,j) = B2 (q(i-2,j) + q(i+1,j)) + B1 (q(i-1,j) + q(i,j)),   qy the same along j,
//   qb(i,j) = 0.5 (qxx + qyy),   qxx = A2 (qx(i,j-2) + qx(i,j+1)) + A1 (qx(i,j-1) + qx(i,j)),   qyy the same of qy along i,
// and the bulk A2bB rectangle reads only qx, qy of the bulk A2bA rectangles.  Here one workgroup owns a 64 x 16 block of corner points of
// one level: it loads q with a halo of (-2, +1) in both directions into LDS once (tangent mode: value and tangent planes), forms qx and
// qy in LDS and writes qb.  The arithmetic is that of A2bA_::line's std4 and of A2bB_::qxx / qyy / eval in their order, so the host
// emulation agrees with the staged launches bit for bit.
//
// The rim.  The strip launches next to the cube edges (A2bBe) read bulk qx on the rows within four of an edge and bulk qy on the columns
// within four (A2bB_<true>::box with qxx / qyy): the forward launch stores qx / qy there and nowhere else.
//
// The adjoint is the closed-form transpose in the same tile structure: qb_ad (block + halo of (-1, +2)) into LDS, qx_ad / qy_ad through
// the A1 / A2 weights into LDS, q_ad through the B1 / B2 weights.  Every output element is owned by exactly one thread: no atomics,
// fixed order.  The launch runs AFTER the strips' adjoint in the backward sweep and reads what they left in qx_ad / qy_ad on the rim from
// memory (one thin launch, run_a2b_rim_clear, stores the zeros the strips accumulate onto; the alternative -- a thin A2bA adjoint over
// the rim, which is four bands -- costs two to four launches and a second pass over q_ad there).
#pragma once
#include <algorithm>
#include "stages.h"
#include "tiled.h"

namespace fv3 {

struct A2bArgs {
  Fld q, qb;            // input (A grid), output (corners)
  Fld qx, qy;           // the staged intermediates: only their rim is stored / read (face mode)
  Rect rb;              // the bulk corner rectangle (A2bB's orect); qx lives on rb widened by (-2, +1) in j, qy by (-2, +1) in i
  int nk = 0;
  int rim = 0;          // cube faces: the strips next to the edges read / accumulate qx, qy on the rim
  unsigned wmask = 0;   // adjoint: q_ad is stored instead of accumulated (dycore.h plan_adjoint) ...
  Rect wrect{1, 0, 1, 0};   // ... over its reach and this rectangle
  HD Rect rx() const { return Rect{rb.i0, rb.i1, rb.j0 - 2, rb.j1 + 1}; }
  HD Rect ry() const { return Rect{rb.i0 - 2, rb.i1 + 1, rb.j0, rb.j1}; }
  HD Rect reach() const { return Rect{rb.i0 - 2, rb.i1 + 1, rb.j0 - 2, rb.j1 + 1}; }      // the q the bulk reads = the q_ad its adjoint touches
};
// nonlinear / tangent / adjoint launch of the bulk
FV3LM_LINK void run_a2b(Exec& ex, int mode, const A2bArgs& a0, const Ctx& c);
// adjoint only: zeros in qx_ad, qy_ad on the bands within four of a cube edge (the rim and the outputs of the A2bAe strips), over `frame`
FV3LM_LINK void run_a2b_rim_clear(Exec& ex, const A2bArgs& a0, const Rect& frame, const Ctx& c);

// algorithmic bytes of one launch in the convention of stage_bytes: q read, qb written (x2 in the tangent mode; adjoint: qb_ad read,
// q_ad read-modify-written -- the routine is linear, no trajectory)
inline double a2b_bytes(const A2bArgs& a, const Geom& g, int mode) {
  const double cells = double(a.rb.i1 - a.rb.i0 + 1) * double(a.rb.j1 - a.rb.j0 + 1) * g.ntile * a.nk;
  return 8. * cells * (mode == MODE_NL ? 2. : mode == MODE_TL ? 4. : 3.);
}
}  // namespace fv3

#if !defined(FV3LM_SPLIT_BUILD) || defined(FV3LM_IMPL_A2B)
namespace fv3 {
#ifndef FV3LM_A2B_H
#define FV3LM_A2B_H 16
#endif
#ifndef FV3LM_A2B_THREADS_NL
#define FV3LM_A2B_THREADS_NL 256
#endif
#ifndef FV3LM_A2B_THREADS_TL
#define FV3LM_A2B_THREADS_TL 512
#endif
#ifndef FV3LM_A2B_THREADS_AD
#define FV3LM_A2B_THREADS_AD 256
#endif
constexpr int A2B_W = 64, A2B_H = FV3LM_A2B_H;                  // points per block
constexpr int A2B_QW = A2B_W + 3, A2B_QH = A2B_H + 3;           // the halo'd tile
// LDS, doubles per component: the halo'd tile (q / qb_ad) | the x-interpolated one, halo'd in j (forward) or i (adjoint) | the other
constexpr int A2B_NQ = A2B_QW * A2B_QH, A2B_NA = A2B_W * A2B_QH, A2B_NB = A2B_QW * A2B_H, A2B_NT = A2B_NQ + A2B_NA + A2B_NB;
// the rim: rows / columns of bulk qx / qy that the edge strips read (n1 = npx or npy)
HD bool a2b_rim(int m, int n1) { return m <= 4 || m >= n1 - 4; }

// One block of the forward modes: corner points I0..I1 x J0..J1 of level k of one tile, blocks laid over Qr = a.rb.
template <class T, int NTH>
DEV void a2b_block(const A2bArgs& a, const Ctx& c, const Rect& Qr, int tile, int k, int bx, int by, double* lds, int tid) {
  typedef TpfIO<T> IO;
  const Geom& g = c.g;
  const int npx = g.nx + 1, npy = g.ny + 1;
  const TileBlk B = tile_blk(Qr, bx, by, A2B_W, A2B_H);
  const int I0 = B.I0, I1 = B.I1, J0 = B.J0, J1 = B.J1;
  const bool firstx = bx == 0, lastx = I1 == Qr.i1, firsty = by == 0, lasty = J1 == Qr.j1;
  double* const Q = lds; double* const QX = lds + A2B_NQ; double* const QY = QX + A2B_NA;
  // ---- q on [I0-2, I1+1] x [J0-2, J1+1]
  TPF_LOOP(e, A2B_NQ) {
    const int i = I0 - 2 + e % A2B_QW, j = J0 - 2 + e / A2B_QW;
    if (i <= I1 + 1 && j <= J1 + 1) IO::lset(Q, A2B_NT, e, IO::ld(a.q, fld_at(g, a.q, tile, k, i, j)));
  }
  TPF_SYNC();
  // ---- qx on [I0, I1] x [J0-2, J1+1], qy on [I0-2, I1+1] x [J0, J1] (A2bA_::line std4); the rim goes to memory, each element by the block
  // that owns its row / column
  TPF_LOOP(e, A2B_NA) {
    const int x = e % A2B_W, r = e / A2B_W, i = I0 + x, j = J0 - 2 + r;
    if (i > I1 || j > J1 + 1) continue;
    auto q = [&](int ii) -> T { return IO::lget(Q, A2B_NT, r * A2B_QW + (ii - (I0 - 2))); };
    const T v = B2 * (q(i - 2) + q(i + 1)) + B1 * (q(i - 1) + q(i));
    IO::lset(QX, A2B_NT, e, v);
    if (a.rim && a2b_rim(j, npy) && ((j >= J0 && j <= J1) || (firsty && j < J0) || (lasty && j > J1))) IO::st(a.qx, fld_at(g, a.qx, tile, k, i, j), v);
  }
  TPF_LOOP(e, A2B_NB) {
    const int x = e % A2B_QW, r = e / A2B_QW, i = I0 - 2 + x, j = J0 + r;
    if (i > I1 + 1 || j > J1) continue;
    auto q = [&](int jj) -> T { return IO::lget(Q, A2B_NT, (jj - (J0 - 2)) * A2B_QW + x); };
    const T v = B2 * (q(j - 2) + q(j + 1)) + B1 * (q(j - 1) + q(j));
    IO::lset(QY, A2B_NT, e, v);
    if (a.rim && a2b_rim(i, npx) && ((i >= I0 && i <= I1) || (firstx && i < I0) || (lastx && i > I1))) IO::st(a.qy, fld_at(g, a.qy, tile, k, i, j), v);
  }
  TPF_SYNC();
  // ---- qb (A2bB_::qxx, qyy, eval)
  TPF_LOOP(e, A2B_W * A2B_H) {
    const int x = e % A2B_W, r = e / A2B_W, i = I0 + x, j = J0 + r;
    if (i > I1 || j > J1) continue;
    auto qx = [&](int jj) -> T { return IO::lget(QX, A2B_NT, (jj - (J0 - 2)) * A2B_W + x); };
    auto qy = [&](int ii) -> T { return IO::lget(QY, A2B_NT, r * A2B_QW + (ii - (I0 - 2))); };
    const T qxx = A2 * (qx(j - 2) + qx(j + 1)) + A1 * (qx(j - 1) + qx(j));
    const T qyy = A2 * (qy(i - 2) + qy(i + 1)) + A1 * (qy(i - 1) + qy(i));
    IO::st(a.qb, fld_at(g, a.qb, tile, k, i, j), 0.5 * (qxx + qyy));
  }
}

// One block of the adjoint: the points I0..I1 x J0..J1 of q_ad, blocks laid over Qr (the reach of the bulk, widened in store mode).
template <int NTH>
DEV void a2b_ad_block(const A2bArgs& a, const Ctx& c, const Rect& Qr, int tile, int k, int bx, int by, double* lds, int tid) {
  const Geom& g = c.g;
  const int npx = g.nx + 1, npy = g.ny + 1;
  const TileBlk B = tile_blk(Qr, bx, by, A2B_W, A2B_H);
  const int I0 = B.I0, I1 = B.I1, J0 = B.J0, J1 = B.J1;
  const Rect rx = a.rx(), ry = a.ry(), rq = a.reach();
  double* const QB = lds; double* const QX = lds + A2B_NQ; double* const QY = QX + A2B_NB;
  // ---- qb_ad on [I0-1, I0+W+1] x [J0-1, J0+H+1], zero outside the bulk rectangle
  TPF_LOOP(e, A2B_NQ) {
    const int i = I0 - 1 + e % A2B_QW, j = J0 - 1 + e / A2B_QW;
    QB[e] = a.rb.has(i, j) ? a.qb.p[fld_at(g, a.qb, tile, k, i, j)] : 0.;
  }
  TPF_SYNC();
  // ---- qx_ad on [I0-1, I0+W+1] x [J0, J0+H-1], qy_ad on [I0, I0+W-1] x [J0-1, J0+H+1]: the transposed A1 / A2 sums, + on the rim what the
  // strips' adjoint left in memory
  TPF_LOOP(e, A2B_NB) {
    const int x = e % A2B_QW, r = e / A2B_QW, i = I0 - 1 + x, j = J0 + r;
    double v = 0.;
    if (rx.has(i, j)) {
      const double* b = QB + r * A2B_QW + x;       // qb_ad(i, j-1)
      v = 0.5 * (A2 * (b[0] + b[3 * A2B_QW]) + A1 * (b[A2B_QW] + b[2 * A2B_QW]));
      if (a.rim && a2b_rim(j, npy)) v += a.qx.p[fld_at(g, a.qx, tile, k, i, j)];
    }
    QX[e] = v;
  }
  TPF_LOOP(e, A2B_NA) {
    const int x = e % A2B_W, r = e / A2B_W, i = I0 + x, j = J0 - 1 + r;
    double v = 0.;
    if (ry.has(i, j)) {
      const double* b = QB + r * A2B_QW + x;       // qb_ad(i-1, j)
      v = 0.5 * (A2 * (b[0] + b[3]) + A1 * (b[1] + b[2]));
      if (a.rim && a2b_rim(i, npx)) v += a.qy.p[fld_at(g, a.qy, tile, k, i, j)];
    }
    QY[e] = v;
  }
  TPF_SYNC();
  // ---- q_ad: the transposed B1 / B2 sums (store rules of exec.h body_ad_joint)
  TPF_LOOP(e, A2B_W * A2B_H) {
    const int x = e % A2B_W, r = e / A2B_W, i = I0 + x, j = J0 + r;
    if (i > I1 || j > J1) continue;
    const bool in = rq.has(i, j);
    if (!in && !(a.wmask & 1u)) continue;
    const double* px = QX + r * A2B_QW + x;        // qx_ad(i-1, j)
    const double* py = QY + r * A2B_W + x;         // qy_ad(i, j-1)
    const double acc = (B2 * (px[0] + px[3]) + B1 * (px[1] + px[2])) + (B2 * (py[0] + py[3 * A2B_W]) + B1 * (py[A2B_W] + py[2 * A2B_W]));
    double* q = &a.q.p[fld_at(g, a.q, tile, k, i, j)];
    if (a.wmask & 1u) *q = in ? acc : 0.; else *q += acc;
  }
}
// the block descriptors (tiled.h)
template <class T, int N> struct A2bFwd {
  typedef A2bArgs Args; static constexpr int NTH = N; static constexpr size_t LDS_BYTES = (size_t)A2B_NT * 8 * TpfIO<T>::NC;
  DEV static void block(const Args& a, const Ctx& c, const Rect& Qr, int tile, int k, int bx, int by, double* lds, int tid) { a2b_block<T, N>(a, c, Qr, tile, k, bx, by, lds, tid); }
};
template <int N> struct A2bAd {
  typedef A2bArgs Args; static constexpr int NTH = N; static constexpr size_t LDS_BYTES = (size_t)A2B_NT * 8;
  DEV static void block(const Args& a, const Ctx& c, const Rect& Qr, int tile, int k, int bx, int by, double* lds, int tid) { a2b_ad_block<N>(a, c, Qr, tile, k, bx, by, lds, tid); }
};

// The bands of `frame` within four of a cube edge, as up to four rectangles (south, north, west, east; disjoint).
struct A2bBands { Rect r[4]; int off[5]; };
inline A2bBands a2b_bands(const Rect& f, int npx, int npy) {
  A2bBands b;
  const int jn = std::max(npy - 4, 5), ie_ = std::max(npx - 4, 5);
  b.r[0] = Rect{f.i0, f.i1, f.j0, std::min(4, f.j1)};
  b.r[1] = Rect{f.i0, f.i1, std::max(jn, f.j0), f.j1};
  const int m0 = std::max(f.j0, 5), m1 = std::min(f.j1, jn - 1);      // the rows between the two
  b.r[2] = Rect{f.i0, std::min(4, f.i1), m0, m1};
  b.r[3] = Rect{std::max(ie_, f.i0), f.i1, m0, m1};
  b.off[0] = 0;
  for (int n = 0; n < 4; ++n) {
    const int w = b.r[n].i1 - b.r[n].i0 + 1, h = b.r[n].j1 - b.r[n].j0 + 1;
    b.off[n + 1] = b.off[n] + ((w > 0 && h > 0) ? w * h : 0);
  }
  return b;
}
HD void a2b_rim_clear_point(const A2bArgs& a, const Ctx& c, const A2bBands& b, int e, int z) {
  int n = 0;
  while (n < 3 && e >= b.off[n + 1]) ++n;
  e -= b.off[n];
  const int w = b.r[n].i1 - b.r[n].i0 + 1, i = b.r[n].i0 + e % w, j = b.r[n].j0 + e / w;
  const size_t m = (size_t)z * c.g.plane + (size_t)c.g.idx(i, j);
  a.qx.p[m] = 0.; a.qy.p[m] = 0.;
}

#ifndef FV3LM_HOST_EMUL
__global__ void __launch_bounds__(256) k_a2b_rim_clear(A2bArgs a, Ctx c, A2bBands b) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < b.off[4]) a2b_rim_clear_point(a, c, b, e, blockIdx.y);
}
#endif

FV3LM_LINK void run_a2b(Exec& ex, int mode, const A2bArgs& a0, const Ctx& c) {
  A2bArgs a = a0;
  for (Fld* f : {&a.q, &a.qb, &a.qx, &a.qy}) *f = ex.sh(*f);
  if (ex.no_wmask) a.wmask = 0;
  if (mode == MODE_AD && !a.q.p) return;
  // adjoint: the blocks are laid over the reach of the bulk; store mode: also over where the stored adjoint is read later
  const Rect Qr = mode == MODE_AD ? ad_launch_rect(a.reach(), a.wmask & 1u, a.wrect, c.g) : a.rb;
  const int nbx = tiled_blocks(Qr.i0, Qr.i1, A2B_W), nby = tiled_blocks(Qr.j0, Qr.j1, A2B_H);
  const double bytes = a2b_bytes(a, c.g, mode);
  if (mode == MODE_TL) run_tiled<A2bFwd<Dual, tiled_nth(FV3LM_A2B_THREADS_TL)>>(ex, "A2b", mode_tag(mode), bytes, Qr, nbx, nby, a, c);
  else if (mode == MODE_NL) run_tiled<A2bFwd<double, tiled_nth(FV3LM_A2B_THREADS_NL)>>(ex, "A2b", mode_tag(mode), bytes, Qr, nbx, nby, a, c);
  else run_tiled<A2bAd<tiled_nth(FV3LM_A2B_THREADS_AD)>>(ex, "A2b", mode_tag(mode), bytes, Qr, nbx, nby, a, c);
}

FV3LM_LINK void run_a2b_rim_clear(Exec& ex, const A2bArgs& a0, const Rect& frame, const Ctx& c) {
  A2bArgs a = a0;
  for (Fld* f : {&a.qx, &a.qy}) *f = ex.sh(*f);
  if (!a.qx.p || !a.qy.p) return;
  const A2bBands b = a2b_bands(frame, c.g.nx + 1, c.g.ny + 1);
  const int nz = c.g.ntile * a.nk;
  if (b.off[4] <= 0) return;
  ex.mark_begin("A2bRim", ".ad", 8. * 2. * double(b.off[4]) * nz);
#ifdef FV3LM_HOST_EMUL
  for (int z = 0; z < nz; ++z)
    for (int e = 0; e < b.off[4]; ++e) a2b_rim_clear_point(a, c, b, e, z);
#else
  hipLaunchKernelGGL(k_a2b_rim_clear, dim3((b.off[4] + 255) / 256, nz), dim3(256), 0, ex.stream, a, c, b);
#endif
  ex.mark_end();
  ex.launches++;
}

}  // namespace fv3
#endif
