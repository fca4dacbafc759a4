// Host side of the depthwise sources (dwconv.hip: tile kernels and the C entries; dwconv_cw.hip, dwconv_mm.hip, dwconv_mm2.hip, dwconv_big.hip;
// csrc/experimental/xdw_cw_bwd.hip for the geometry): the argument structs behind the C entries, the run-time switches, one plan per
// launch (family order, accept / reject, launch sizing), the tile geometry of the channel-pair kernels and the dispatch helpers.
// The device side they share is dwconv_cw.h.
#pragma once
#include "dwconv_cw.h"
#include <cstdlib>
#include <type_traits>

namespace atomnas {

// What the C entries (dwconv.hip) hand down after validation; everything below them takes these by const&.
// `slab`: every activation operand is slab-major and the tap table is padded to whole 8-channel groups (ldw >= pad8(C)) -- what the
// cw / mm / mm2 families need; the tile kernels of dwconv.hip take any layout.
struct DwShape { int N, H, W, C, k, stride, dtype; bool slab; };
struct DwFwdArgs {
  DwShape s;
  const void* x; int ldx; long xss;
  const float *sc, *sh; int relu;
  const float* w; int ldw;
  void* y; int ldy; long yss;
  float* stats; int stat_ld, stat_rows;
  hipStream_t st;
};
struct DwBwdArgs {
  DwShape s;
  const void* gup; int ldg; long gss;
  const void* yraw; int ldyr; long yrss;
  const float *c1, *c2, *c3;
  const void* x; int ldx; long xss;
  const float *sc, *sh; int relu;
  const float* w; int ldw;
  void* h; int ldh; long hss;
  float *dw, *stats; int stat_ld, part_rows;
  float* dw_ws;
  hipStream_t st;
};

// The run-time switches of the depthwise host code, each read once per process.
//   ATOMNAS_DW_MM, default 166 = 2 + 4 + 32 + 128 (which shapes run on the matrix cores, bf16 slab-major tensors):
//     bits 0-2 (1, 2, 4)    stride-1 forward k = 3 / 5 / 7          (dwconv_mm.hip)
//     bits 3-5 (8, 16, 32)  stride-1 backward k = 3 / 5 / 7
//     bit 6 (64)            the backward also on whole-image tiles (14 x 14, 7 x 7 maps)
//     bit 7 (128)           stride-2 forward, every k               (dwconv_mm2.hip)
//   Default (profiles/r05_dw_mm_per_shape.txt, batch 256): forward k = 5, 7 everywhere (k = 3 is as fast on the packed-FMA rows);
//   backward k = 7 on row-ring tiles (56 x 56: 0.42 -> 0.34 ms, 28 x 28: 0.20 -> 0.16 ms) -- a tile of the backward kernel costs about
//   the same for every k (commit + two operand copies + epilogue, ~1000 instructions per wave), which beats the packed-FMA rows only
//   at k = 7 and only where a worker walks many tiles; the stride-2 forward: profiles/r05_dw_mm2_per_shape.txt.
//   ATOMNAS_DW_CW, default 7 (dwconv_cw.hip): bit 0 backward, bit 1 stride-1 forward, bit 2 stride-2 backward (needs bit 0 as well).
//   ATOMNAS_DW_MAX_WORKERS, default 0 = no limit (tests: few workers walk long columns of tiles).
struct DwEnv { int mm, cw; long max_workers; };
inline const DwEnv& dw_env() {
  static const DwEnv e = {
      getenv("ATOMNAS_DW_MM") ? atoi(getenv("ATOMNAS_DW_MM")) : 166,
      getenv("ATOMNAS_DW_CW") ? atoi(getenv("ATOMNAS_DW_CW")) : 7,
      getenv("ATOMNAS_DW_MAX_WORKERS") ? atol(getenv("ATOMNAS_DW_MAX_WORKERS")) : 0,
  };
  return e;
}

// One plan per launch.  <family>_plan is the COMPLETE accept / reject decision for a shape and direction (dir 0 forward, 1 backward:
// switch bits, layout, geometry, LDS limit) and leaves the geometry and the LDS size in the plan; <family>_launch_* runs an accepted
// plan and cannot decline.  dw_pick (dwconv.hip) states the order of the families; the C entries and the *_supported queries share it.
enum DwFamily { DW_TILE, DW_CW, DW_MM, DW_MM2, DW_BIG };
// geometry of the k = 9 / 11 kernels (dwconv_big.hip): 16-channel slabs, tiles of TH x TW pixels, haloed LDS window
struct BigGeom {
  int N, H, W, C, Ho, Wo;
  int TH, TW;             // tile: output pixels (forward) / input pixels (backward); TW a multiple of 4, backward TH even
  int tiles_y, tiles_x;   // tiles per image
  int LH, LW, RP;         // LDS window: rows, columns, row pitch (floats)
  int nworkers, nslabs;
};
struct DwPlan {
  CwGeom g;
  MmGeom mg;     // DW_MM
  Mm2Geom mg2;   // DW_MM2
  BigGeom bg;    // DW_BIG
  size_t lds;
};
bool cw_plan(const DwShape& s, int dir, DwPlan& p);     // dwconv_cw.hip: packed-FMA tap rows, stride 1 both ways, stride 2 backward
int cw_launch_fwd(const DwPlan& p, const DwFwdArgs& a);
int cw_launch_bwd(const DwPlan& p, const DwBwdArgs& a);
bool mm_plan(const DwShape& s, int dir, DwPlan& p);     // dwconv_mm.hip: tap rows on the matrix cores, bf16, stride 1
int mm_launch_fwd(const DwPlan& p, const DwFwdArgs& a);
int mm_launch_bwd(const DwPlan& p, const DwBwdArgs& a);
bool mm2_plan(const DwShape& s, int dir, DwPlan& p);    // dwconv_mm2.hip: the stride-2 forward on the matrix cores, bf16
int mm2_launch_fwd(const DwPlan& p, const DwFwdArgs& a);
bool big_plan(const DwShape& s, int dir, DwPlan& p);    // dwconv_big.hip: k = 9 / 11, every stride, storage type and layout
int big_launch_fwd(const DwPlan& p, const DwFwdArgs& a);
int big_launch_bwd(const DwPlan& p, const DwBwdArgs& a);
DwFamily dw_pick(const DwShape& s, int dir, DwPlan& p);

static bool cw_geometry(CwGeom& g, int N, int H, int W, int C, int K) {
  if (W % 7 != 0 || W < 7) return false;
  g.N = N; g.H = H; g.W = W; g.C = C;
  g.ns = W / 7;
  if (g.ns > 16) return false;
  if (H * g.ns <= 64) {   // whole images
    g.TH = H; g.tiles_y = 1; g.NI = 64 / (H * g.ns); g.ring = 0;
    if (g.NI > N) g.NI = N;
  } else {
    const int cap = 64 / g.ns;
    const int nty = (H + cap - 1) / cap;
    g.TH = (H + nty - 1) / nty;
    g.tiles_y = (H + g.TH - 1) / g.TH;
    g.NI = 1; g.ring = 1;
  }
  g.LH = g.TH + K - 1;
  // row pitch: the 32 lanes of an LDS group are (rows x strips); their first elements r * LWp + 7 * j must differ mod 32 (8-byte
  // bank pairs): LWp = ns (mod 2 ns) for ns a power of two does it (7 is invertible mod 32), an odd pitch otherwise
  const int lw = W + K - 1;
  const bool pow2 = (g.ns & (g.ns - 1)) == 0;
  int lwp = lw;
  if (pow2) { while (lwp % (2 * g.ns) != g.ns) ++lwp; } else if (lwp % 2 == 0) ++lwp;
  g.LWp = lwp;
  g.RH = g.LH;
  int plane = g.NI * g.RH * g.LWp;
  if (plane < 512) plane = 512;      // the weight-gradient flush transposes 64 x 15 + 56 floats through a wave's own plane
  while (plane % 4 != 2) ++plane;     // staging writes of the two channel groups land in different bank halves
  g.plane = plane;
  g.TPIX = g.NI * g.TH * W;
  int tp = g.TPIX;
  while (tp % 8 != 4) ++tp;
  g.TPIXp = tp;
  g.ntiles = ((N + g.NI - 1) / g.NI) * g.tiles_y;
  g.nslabs = (C + 15) / 16;
  return true;
}

// stride 2: the lane grid is the output grid; K decides the halo rows / columns of the window
static bool cw2_geometry(CwGeom& g, int N, int H, int W, int C, int K) {
  if (H % 2 || W % 14 != 0 || W < 14) return false;
  const int P = (K - 1) / 2;
  const int RELMIN = cw_fdiv(-P, 2), RELMAX = cw_fdiv(13 + P, 2), CL = -RELMIN, CR = RELMAX - 6;
  const int HL = P / 2 + cw_fdiv(P - 1, 2) + 1;
  g.N = N; g.H = H; g.W = W; g.C = C;
  g.Ho = H / 2; g.Wo = W / 2;
  g.ns = g.Wo / 7;
  if (g.ns > 16) return false;
  if (g.Ho * g.ns <= 64) {   // whole images
    g.THd = g.Ho; g.tiles_y = 1; g.NI = 64 / (g.Ho * g.ns); g.ring = 0;
    if (g.NI > N) g.NI = N;
  } else {
    const int cap = 64 / g.ns;
    const int nty = (g.Ho + cap - 1) / cap;
    g.THd = (g.Ho + nty - 1) / nty;
    g.tiles_y = (g.Ho + g.THd - 1) / g.THd;
    g.NI = 1; g.ring = 1;
  }
  g.TH = 2 * g.THd;
  g.LH = g.THd + HL;
  const int lw = g.Wo + CL + CR;
  const bool pow2 = (g.ns & (g.ns - 1)) == 0;
  int lwp = lw;
  if (pow2) { while (lwp % (2 * g.ns) != g.ns) ++lwp; } else if (lwp % 2 == 0) ++lwp;
  g.LWp = lwp;
  g.RH = g.LH;
  int plane = g.NI * g.RH * g.LWp + 4;   // + slack: a half strip reads a fixed number of operand pairs, up to 2 past its last one
  if (plane < 512) plane = 512;
  while (plane % 4 != 2) ++plane;
  g.plane = plane;
  g.TPIX = g.NI * g.TH * W;
  g.TPIXD = g.NI * g.THd * g.Wo;
  int tp = g.TPIX;
  while (tp % 8 != 4) ++tp;
  g.TPIXp = tp;
  g.ntiles = ((N + g.NI - 1) / g.NI) * g.tiles_y;
  g.nslabs = (C + 15) / 16;
  return true;
}

// every family but the tile kernels runs half-slab workgroups of 4 waves (cw_block<4>): two workgroups per (slab, worker)
static void cw_workers(CwGeom& g, int per_cu, int max_rows) {
  if (per_cu < 1) per_cu = 1;
  long want = ((long)num_cus() * per_cu) / (g.nslabs * 2);
  const long max_env = dw_env().max_workers;
  if (max_env > 0 && want > max_env) want = max_env;
  if (max_rows > 0 && want > max_rows) want = max_rows;   // every worker owns one partial row
  if (want > g.ntiles) want = g.ntiles;
  if (want < 1) want = 1;
  g.nworkers = (int)want;
}
static unsigned cw_grid(const CwGeom& g) {
  return ((unsigned)g.nworkers * g.nslabs + 7) / 8 * 16;   // 8 (slab, worker) units -> 16 blocks, see cw_block
}

// ---- one copy of each dispatch idiom: f receives the choice as a compile-time constant
template <int V> using IC = std::integral_constant<int, V>;
template <typename T> struct DwType { typedef T type; };
template <typename F> static auto dw_for_k(int k, F&& f) {   // the tile kernels' k; k > 7 never comes here (DW_BIG)
  if (k == 3) return f(IC<3>{});
  if (k == 5) return f(IC<5>{});
  return f(IC<7>{});
}
template <typename F> static auto dw_for_type(int dtype, F&& f) {
  if (dtype == DT_F32) return f(DwType<float>{});
  return f(DwType<bf16_t>{});
}
// LDS bytes of a channel-pair workgroup: per wave one operand plane (f32 pairs) and one pixel plane in the storage type's pair_t
static size_t cw_lds(const CwGeom& g, int dtype) {
  const size_t pair_bytes = dw_for_type(dtype, [](auto t) { return sizeof(typename Cw<typename decltype(t)::type>::pair_t); });
  return (size_t)4 * g.plane * sizeof(f32x2) + (size_t)4 * g.TPIXp * pair_bytes + 48 * sizeof(float);
}
// The activation instance AM of a kernel.  ReLU6 and Swish always have their own; plain ReLU has one only in the matrix-core families
// (RELU_INSTANCE) and only behind a fused input BatchNorm (`fused`: in_scale is given).  Everything else runs instance 0, which
// reads the run-time flag.
template <bool RELU_INSTANCE, typename F> static auto dw_for_act(int relu, bool fused, F&& f) {
  if (relu == ACT_RELU6) return f(IC<ACT_RELU6>{});
  if (relu == ACT_SWISH) return f(IC<ACT_SWISH>{});
  if constexpr (RELU_INSTANCE) {
    if (relu == ACT_RELU && fused) return f(IC<ACT_RELU>{});
  }
  return f(IC<0>{});
}
// tail of every backward launch: dw[c][t] += sum over workers of the weight-gradient partials, in worker order
static int dw_finish_bwd(const char* what, const DwBwdArgs& a, int nworkers) {
  if (int rc = check_launch(what)) return rc;
  const long n = (long)a.s.C * a.s.k * a.s.k;
  return a.dw ? reduce_parts(a.dw_ws, n, nworkers, n, a.dw, (int)n, 0, 1, a.st) : 0;
}

}  // namespace atomnas
