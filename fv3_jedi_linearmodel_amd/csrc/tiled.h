// fv3lm-hip: what the hand-written LDS-tiled launches share (a2b.h, d2a2c.h, tpfused.h, tp2.h, tpad.h): one workgroup owns a W x H block
// of points of one level of one tile, the blocks are laid over a launch rectangle Qr, grid.z = tiles x levels.
//
// A launch is described by a block descriptor B:
//   typedef ... Args;                     the launch's arguments (by value to the kernel; Args::nk = levels)
//   static constexpr int NTH;             threads per block (host emulation: one "thread" runs every element, see tiled_nth)
//   static constexpr size_t LDS_BYTES;    dynamic LDS of a block
//   DEV static void block(const Args&, const Ctx&, const Rect& Qr, int tile, int k, int bx, int by, double* lds, int tid);
// and run by run_tiled<B>: profile markers, the launch count, the LDS limit of the kernel where a block needs more than the 64 KB a
// launch may ask for by default, and in the host emulation the loop over the blocks with a guarded LDS buffer.
#pragma once
#include "exec.h"

#ifdef FV3LM_HOST_EMUL
#define TPF_SYNC() ((void)0)
#define TPF_LOOP(e, n) for (int e = tid; e < (n); e += NTH)
#define TPF_LOOPU(e, u, n, E) for (int u = 0, e = 0; e < (n); ++e, ++u)      /* one "thread": slot u of a per-thread array is element e */
#else
#define TPF_SYNC() __syncthreads()
// constant trip count, unrolled: the global loads of a thread's elements of a phase are issued together
#define TPF_LOOP(e, n) _Pragma("unroll") for (int e = tid; e < (n); e += NTH)
// the same with the slot index u of a per-thread register array (constant trip count E = ceil(n / NTH): static indices after unrolling)
#define TPF_LOOPU(e, u, n, E) _Pragma("unroll") for (int u = 0; u < (E); ++u) if (const int e = tid + u * NTH; e < (n))
#endif

namespace fv3 {
// global and LDS access of a value (nonlinear) or a value + tangent pair; an LDS array of Dual is two planes nt doubles apart
template <class T> struct TpfIO;
template <> struct TpfIO<double> {
  static constexpr int NC = 1;
  DEV static double ld(const Fld& f, size_t n) { return f.t[n]; }
  DEV static void st(const Fld& f, size_t n, double x) { f.t[n] = x; }
  DEV static double lget(const double* v, int, int e) { return v[e]; }
  DEV static void lset(double* v, int, int e, double x) { v[e] = x; }
};
template <> struct TpfIO<Dual> {
  static constexpr int NC = 2;
  DEV static Dual ld(const Fld& f, size_t n) { return Dual(f.t[n], f.p ? f.p[n] : 0.0); }
  DEV static void st(const Fld& f, size_t n, const Dual& x) { f.t[n] = x.v; f.p[n] = x.d; }
  DEV static Dual lget(const double* v, int nt, int e) { return Dual(v[e], v[nt + e]); }
  DEV static void lset(double* v, int nt, int e, const Dual& x) { v[e] = x.v; v[nt + e] = x.d; }
};

// block (bx, by) of W x H points of the launch rectangle Q, the last row / column of blocks cut at the rectangle
struct TileBlk { int I0, I1, J0, J1; };
HD TileBlk tile_blk(const Rect& Q, int bx, int by, int W, int H) {
  const int I0 = Q.i0 + bx * W, J0 = Q.j0 + by * H;
  return TileBlk{I0, (I0 + W - 1 < Q.i1) ? I0 + W - 1 : Q.i1, J0, (J0 + H - 1 < Q.j1) ? J0 + H - 1 : Q.j1};
}
// element (i, j) of level k of a tile of field f
HD size_t fld_at(const Geom& g, const Fld& f, int tile, int k, int i, int j) { return (size_t)(tile * f.nk + k - 1) * g.plane + (size_t)g.idx(i, j); }
inline int tiled_blocks(int lo, int hi, int n) { return (hi - lo + n) / n; }      // blocks of n points over lo..hi
inline const char* mode_tag(int mode) { return mode == MODE_NL ? ".nl" : mode == MODE_TL ? ".tl" : ".ad"; }
// threads per block of a descriptor: n on the device, one in the host emulation
constexpr int tiled_nth(int n) {
#ifdef FV3LM_HOST_EMUL
  return (void)n, 1;
#else
  return n;
#endif
}

#ifndef FV3LM_HOST_EMUL
// 16-byte alignment: tp2.h holds Dual elements in LDS
template <class B>
__global__ void __launch_bounds__(B::NTH) k_tiled(typename B::Args a, Ctx c, Rect Qr) {
  extern __shared__ __attribute__((aligned(16))) double tiled_lds[];
  int bx = blockIdx.x, by = blockIdx.y; xcd_block(gridDim.x, gridDim.y, bx, by);
  B::block(a, c, Qr, blockIdx.z / a.nk, 1 + blockIdx.z % a.nk, bx, by, tiled_lds, threadIdx.x);
}
#endif

// One launch of nbx x nby blocks per level and tile over Qr; profile name `name` + `tag`, `bytes` the algorithmic traffic.
template <class B>
inline void run_tiled(Exec& ex, const char* name, const char* tag, double bytes, const Rect& Qr, int nbx, int nby, const typename B::Args& a, const Ctx& c) {
  const int nz = c.g.ntile * a.nk;
  ex.mark_begin(name, tag, bytes);
#ifdef FV3LM_HOST_EMUL
  // the LDS of a block is exactly what the descriptor declares, with guard words behind it: a block that writes past its declared LDS
  // (which the device launch would not have been given) fails the call
  constexpr size_t N = (B::LDS_BYTES + 7) / 8, NG = 8;
  constexpr double GUARD = -6.02214076e23;
  std::vector<double> lds(N + NG, 0.);
  for (size_t n = N; n < N + NG; ++n) lds[n] = GUARD;
  for (int z = 0; z < nz; ++z)
    for (int by = 0; by < nby; ++by)
      for (int bx = 0; bx < nbx; ++bx) B::block(a, c, Qr, z / a.nk, 1 + z % a.nk, bx, by, lds.data(), 0);
  for (size_t n = N; n < N + NG; ++n)
    if (lds[n] != GUARD) { set_sticky(std::string("internal error: ") + name + tag + " wrote past the " + std::to_string(B::LDS_BYTES) + " bytes of LDS it declares"); break; }
#else
  if (B::LDS_BYTES > 64 * 1024) {      // above the default limit of a launch
    static bool attr = false;
    if (!attr) { if (hipFuncSetAttribute((const void*)k_tiled<B>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)B::LDS_BYTES) != hipSuccess) set_sticky(std::string("hipFuncSetAttribute(") + name + tag + ") failed"); attr = true; }
  }
  hipLaunchKernelGGL((k_tiled<B>), dim3(nbx, nby, nz), dim3(B::NTH), B::LDS_BYTES, ex.stream, a, c, Qr);
#endif
  ex.mark_end();
  ex.launches++;
}

}  // namespace fv3
