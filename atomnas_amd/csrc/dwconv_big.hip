// Depthwise k x k convolution for the MixConv-size atoms, k in {9, 11} (stride in {1,2}, pad (k-1)/2): the DW_BIG family of dw_pick.
//
// Same contract as the kernels of dwconv.hip (include/atomnas_hip.h), plain kernels: no matrix cores, no channel-pair-per-wave form, no
// software pipeline.  Any layout (plain [M][ld] or slab-major), fp32 or bf16 storage; operands are the stored values, products and sums
// are fp32, one rounding at the store.
//
// Structure (both directions): a 256-thread workgroup owns one slab of 16 channels and a contiguous range of spatial tiles ("worker").
// Per tile the haloed operand window is staged once through LDS as fp32 after its prologue; a thread owns one channel pair
// (tid % 8) and walks work items (row, strip of 4 pixels), one tap row at a time (an LDS row segment in registers, k x 4 packed FMAs).
//   forward : window = act(x*in_scale+in_shift) over the input pixels an output tile touches
//   backward: window = dYraw = c1*g + c2*yraw + c3 over the output pixels an INPUT tile touches, plus the tile's own pixels (raw and
//             activated).  The tile is walked twice over the same LDS contents:
//               1. input gradient: work items as in the forward, epilogue act' / rounding / statistics / store of h;
//               2. weight gradient: 81 / 121 accumulators per channel do not fit a thread, so here a thread owns a channel pair and ONE
//                  HALF TAP ROW (ky, kx0 .. kx0 + (k+1)/2 - 1): 2k of the 32 pair-groups work, each sums its (k+1)/2 taps over every
//                  pixel of every tile of the worker.  No two threads share a tap, so there is nothing to reduce inside the workgroup:
//                  the thread stores its sums to row `worker` of dw_ws, and dw_finish_bwd adds the rows in worker order.
// Statistics: per-thread sums, butterfly over the lanes of a wave that hold the same pair, the four waves added in order, row `worker`
// of the partial-row buffer written with plain stores and the rows of absent workers zero-filled -- no atomics anywhere.
#include "dwconv_host.h"

namespace atomnas {

constexpr __host__ __device__ int bfdiv(int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }
constexpr __host__ __device__ int bcdiv(int a, int b) { return -bfdiv(-a, b); }
constexpr __host__ __device__ int bpmod(int a, int b) { return ((a % b) + b) % b; }
constexpr __host__ __device__ int bmin(int a, int b) { return a < b ? a : b; }

constexpr int BIG_CB = 16;   // channels per slab
constexpr int BIG_SW = 4;    // pixels per strip (a multiple of the stride: strip origins keep the parity of the tile origin)

__device__ __forceinline__ long big_chan_base(int c, long ss) { return ss ? (long)(c >> 4) * ss + (c & 15) : (long)c; }
__device__ __forceinline__ long big_pix_stride(int ld, long ss) { return ss ? 16 : (long)ld; }

// statistics of one workgroup -> row `worker`, rows of absent workers zeroed.  s_st: [4 waves][2][16]
__device__ __forceinline__ void big_flush_stats(float (&a)[2], float (&b)[2], float* s_st, float* __restrict__ stats, int stat_ld, int stat_rows,
                                                int worker, int nworkers, int c_base, int C) {
  const int tid = threadIdx.x, c2 = tid & 7;
#pragma unroll
  for (int o = 32; o >= 8; o >>= 1) {
    a[0] += __shfl_xor(a[0], o, 64); a[1] += __shfl_xor(a[1], o, 64);
    b[0] += __shfl_xor(b[0], o, 64); b[1] += __shfl_xor(b[1], o, 64);
  }
  __syncthreads();
  if ((tid & 63) < 8) {
    float* sw = s_st + (tid >> 6) * 2 * BIG_CB;
    sw[2 * c2] = a[0]; sw[2 * c2 + 1] = a[1];
    sw[BIG_CB + 2 * c2] = b[0]; sw[BIG_CB + 2 * c2 + 1] = b[1];
  }
  __syncthreads();
  if (tid < 2 * BIG_CB) {
    const int pl = tid / BIG_CB, c = c_base + tid % BIG_CB;
    if (c < C) {
      const float v = ((s_st[tid] + s_st[2 * BIG_CB + tid]) + s_st[4 * BIG_CB + tid]) + s_st[6 * BIG_CB + tid];
      const long elem = (long)pl * stat_ld + c;
      stats[(long)worker * 2 * stat_ld + elem] = v;
      stat_zero_tail(stats, 2L * stat_ld, worker + nworkers, nworkers, stat_rows, elem);
    }
  }
}

// ------------------------------------------------------------------------------------------------ forward
template <typename T, int K, int S>
__global__ __launch_bounds__(256) void k_dwbig_fwd(const T* __restrict__ x, int ldx, long xss, const float* __restrict__ in_scale,
                                                   const float* __restrict__ in_shift, int in_act, const float* __restrict__ w, int ldw,
                                                   T* __restrict__ y, int ldy, long yss, float* __restrict__ stats, int stat_ld, int stat_rows,
                                                   BigGeom g) {
  constexpr int P = (K - 1) / 2, KK = K * K;
  constexpr int IWS = (BIG_SW - 1) * S + K;   // input columns one strip needs
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* s_in = smem;                   // [LH][RP]
  float* s_w = s_in + g.LH * g.RP;      // [KK][16]
  float* s_st = s_w + KK * BIG_CB;      // [4][2][16]

  const int tid = threadIdx.x;
  const int slab = (int)(blockIdx.x % g.nslabs), worker = (int)(blockIdx.x / g.nslabs);
  const int c_base = slab * BIG_CB;
  const int cpad = (g.C + 7) & ~7;
  const Act am = act_of(in_act);

  for (int i = tid; i < KK * BIG_CB; i += 256) {
    const int t = i / BIG_CB, c = i % BIG_CB;
    s_w[i] = (c_base + c < g.C) ? w[(long)t * ldw + c_base + c] : 0.f;
  }

  // staging role: one 8-channel group per thread (piece index parity = tid parity)
  const int cg = tid & 1;
  const int cgc = c_base + cg * 8;
  const bool cg_ok = cgc < cpad;
  float sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { sc[e] = 1.f; sh[e] = 0.f; }
  if (in_scale && cg_ok) { VecIO<float, 8>::load(in_scale + cgc, sc); VecIO<float, 8>::load(in_shift + cgc, sh); }

  // compute role: one channel pair per thread
  const int c2 = tid & 7;
  const int ch = c_base + 2 * c2;
  const int nstrips = g.TW / BIG_SW;
  const int nitems = 8 * g.TH * nstrips;
  float ssum[2] = {0.f, 0.f}, ssq[2] = {0.f, 0.f};
  const long xps = big_pix_stride(ldx, xss), yps = big_pix_stride(ldy, yss);

  const int per_img = g.tiles_y * g.tiles_x;
  const int ntiles = g.N * per_img;
  const int t_beg = (int)((long)worker * ntiles / g.nworkers), t_end = (int)((long)(worker + 1) * ntiles / g.nworkers);
  for (int tile = t_beg; tile < t_end; ++tile) {
    const int n = tile / per_img, tr = tile % per_img;
    const int ty = tr % g.tiles_y, tx = tr / g.tiles_y;
    const int ho0 = ty * g.TH, wo0 = tx * g.TW;
    const int hi0 = ho0 * S - P, wi0 = wo0 * S - P;
    __syncthreads();   // the previous tile is consumed (also orders the s_w initialisation)
    for (int i = tid; i < g.LH * g.LW * 2; i += 256) {
      const int pix = i >> 1;
      const int iy = pix / g.LW, ix = pix % g.LW;
      const int hi = hi0 + iy, wi = wi0 + ix;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.f;
      if (cg_ok && hi >= 0 && hi < g.H && wi >= 0 && wi < g.W) {
        VecIO<T, 8>::load(x + (((long)n * g.H + hi) * g.W + wi) * xps + big_chan_base(cgc, xss), v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = v[e] * sc[e] + sh[e];
        act_apply_v(v, am);
      }
      float* d = s_in + iy * g.RP + ix * BIG_CB + cg * 8;
      *reinterpret_cast<f32x4*>(d) = f32x4{v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4*>(d + 4) = f32x4{v[4], v[5], v[6], v[7]};
    }
    __syncthreads();

    for (int it = tid; it < nitems; it += 256) {
      const int rs = it >> 3;
      const int r = rs % g.TH, j = rs / g.TH;   // rows fastest: the lanes of a wave read 8 different LDS rows
      const int ho = ho0 + r, wos = wo0 + j * BIG_SW;
      if (ho >= g.Ho || wos >= g.Wo || ch >= cpad) continue;
      f32x2 acc[BIG_SW];
#pragma unroll
      for (int t = 0; t < BIG_SW; ++t) acc[t] = f32x2{0.f, 0.f};
#pragma unroll 1
      for (int ky = 0; ky < K; ++ky) {   // one tap row at a time: IWS pairs live
        const float* row = s_in + (r * S + ky) * g.RP + (j * BIG_SW * S) * BIG_CB + 2 * c2;
        f32x2 in[IWS];
#pragma unroll
        for (int i = 0; i < IWS; ++i) in[i] = *reinterpret_cast<const f32x2*>(row + i * BIG_CB);
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const f32x2 wv = *reinterpret_cast<const f32x2*>(s_w + (ky * K + kx) * BIG_CB + 2 * c2);
#pragma unroll
          for (int t = 0; t < BIG_SW; ++t) acc[t] += in[t * S + kx] * wv;
        }
      }
      T* yr = y + (((long)n * g.Ho + ho) * g.Wo) * yps + big_chan_base(ch & ~7, yss) + (ch & 7);
#pragma unroll
      for (int t = 0; t < BIG_SW; ++t) {
        const int wo = wos + t;
        if (wo < g.Wo) {
          float o[2];
          o[0] = (ch < g.C) ? to_f32(from_f32<T>(acc[t][0])) : 0.f;   // pad channels are written as zeros
          o[1] = (ch + 1 < g.C) ? to_f32(from_f32<T>(acc[t][1])) : 0.f;
          VecIO<T, 2>::store(yr + (long)wo * yps, o);
          ssum[0] += o[0]; ssq[0] += o[0] * o[0];   // statistics of the values as stored
          ssum[1] += o[1]; ssq[1] += o[1] * o[1];
        }
      }
    }
  }
  if (stats) big_flush_stats(ssum, ssq, s_st, stats, stat_ld, stat_rows, worker, g.nworkers, c_base, g.C);
}

// ------------------------------------------------------------------------------------------------ backward
// Tiles are in INPUT space; the LDS window holds dYraw over the output pixels the tile touches: rows from
// hob = ceil((hi0 + P - (K-1)) / S), columns from wob = wi0 / S + floor(-P / S)  (hi0, wi0 multiples of S).
template <typename T, int K, int S>
__global__ __launch_bounds__(256) void k_dwbig_bwd(const T* __restrict__ gup, int ldg, long gss, const T* __restrict__ yraw, int ldyr, long yrss,
                                                   const float* __restrict__ c1, const float* __restrict__ c2p, const float* __restrict__ c3,
                                                   const T* __restrict__ x, int ldx, long xss, const float* __restrict__ in_scale,
                                                   const float* __restrict__ in_shift, int in_act, const float* __restrict__ w, int ldw,
                                                   T* __restrict__ h, int ldh, long hss, float* __restrict__ dwp /*[nworkers][C][K*K]*/,
                                                   float* __restrict__ stats, int stat_ld, int stat_rows, BigGeom g) {
  constexpr int P = (K - 1) / 2, KK = K * K;
  constexpr int RELMIN = bfdiv(-P, S);                         // first dY column a strip touches, relative to strip origin / S
  constexpr int DWN = bfdiv(BIG_SW - 1 + P, S) - RELMIN + 1;   // dY columns per strip
  constexpr int TG = (K + 1) / 2;                              // taps of a half tap row
  static_assert(BIG_SW % S == 0, "strip origins must stay multiples of the stride");
  static_assert(2 * K <= 32, "one pair-group of the workgroup per half tap row");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* s_dy = smem;                              // [LH][RP]
  float* s_w = s_dy + g.LH * g.RP;                 // [KK][16]
  float* s_x = s_w + KK * BIG_CB;                  // [TH*TW][16] the tile's pixels as stored
  float* s_xa = s_x + g.TH * g.TW * BIG_CB;        // [TH*TW][16] ... activated (zero outside the image)
  float* s_cf = s_xa + g.TH * g.TW * BIG_CB;       // [5][16] c1, c2, c3, in_scale, in_shift of the slab
  float* s_st = s_cf + 5 * BIG_CB;                 // [4][2][16]

  const int tid = threadIdx.x;
  const int slab = (int)(blockIdx.x % g.nslabs), worker = (int)(blockIdx.x / g.nslabs);
  const int c_base = slab * BIG_CB;
  const int cpad = (g.C + 7) & ~7;
  const Act am = act_of(in_act);

  for (int i = tid; i < KK * BIG_CB; i += 256) {
    const int t = i / BIG_CB, c = i % BIG_CB;
    s_w[i] = (c_base + c < g.C) ? w[(long)t * ldw + c_base + c] : 0.f;
  }
  if (tid < 5 * BIG_CB) {
    const int v = tid / BIG_CB, c = c_base + tid % BIG_CB;
    const float* src = (v == 0) ? c1 : (v == 1 ? c2p : (v == 2 ? c3 : (v == 3 ? in_scale : in_shift)));
    const bool coef = v < 3;
    const float dflt = (v == 0 || v == 3) ? 1.f : 0.f;
    s_cf[tid] = (src && c < cpad && (!coef || c1)) ? src[c] : dflt;
  }
  __syncthreads();

  const int cg = tid & 1;
  const int cgc = c_base + cg * 8;
  const bool cg_ok = cgc < cpad;
  const int c2 = tid & 7;
  const int ch = c_base + 2 * c2;
  const bool ch_ok = ch < cpad;
  const float sc2[2] = {s_cf[3 * BIG_CB + 2 * c2], s_cf[3 * BIG_CB + 2 * c2 + 1]};
  const float sh2[2] = {s_cf[4 * BIG_CB + 2 * c2], s_cf[4 * BIG_CB + 2 * c2 + 1]};
  const int nstrips = g.TW / BIG_SW;
  const int nitems = 8 * g.TH * nstrips;
  const long gps = big_pix_stride(ldg, gss), yps = big_pix_stride(ldyr, yrss), xps = big_pix_stride(ldx, xss), hps = big_pix_stride(ldh, hss);

  // weight-gradient role: pair-group q owns the half tap row (ky = q % K, half = q / K)
  const int wq = tid >> 3;
  const int wky = wq % K, whalf = wq / K;
  f32x2 dacc[TG];
#pragma unroll
  for (int i = 0; i < TG; ++i) dacc[i] = f32x2{0.f, 0.f};
  float s0[2] = {0.f, 0.f}, s1[2] = {0.f, 0.f};

  const int per_img = g.tiles_y * g.tiles_x;
  const int ntiles = g.N * per_img;
  const int t_beg = (int)((long)worker * ntiles / g.nworkers), t_end = (int)((long)(worker + 1) * ntiles / g.nworkers);
  for (int tile = t_beg; tile < t_end; ++tile) {
    const int n = tile / per_img, tr = tile % per_img;
    const int ty = tr % g.tiles_y, tx = tr / g.tiles_y;
    const int hi0 = ty * g.TH, wi0 = tx * g.TW;   // multiples of S
    const int hob = bcdiv(hi0 + P - (K - 1), S), wob = wi0 / S + RELMIN;
    __syncthreads();   // the previous tile is consumed
    // dYraw window
    for (int i = tid; i < g.LH * g.LW * 2; i += 256) {
      const int pix = i >> 1;
      const int iy = pix / g.LW, ix = pix % g.LW;
      const int ho = hob + iy, wo = wob + ix;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.f;
      if (cg_ok && ho >= 0 && ho < g.Ho && wo >= 0 && wo < g.Wo) {
        const long opix = ((long)n * g.Ho + ho) * g.Wo + wo;
        float q1[8];
        VecIO<T, 8>::load(gup + opix * gps + big_chan_base(cgc, gss), v);
        VecIO<float, 8>::load(s_cf + cg * 8, q1);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= q1[e];
        if (yraw) {
          float yr[8], q2[8], q3[8];
          VecIO<T, 8>::load(yraw + opix * yps + big_chan_base(cgc, yrss), yr);
          VecIO<float, 8>::load(s_cf + BIG_CB + cg * 8, q2);
          VecIO<float, 8>::load(s_cf + 2 * BIG_CB + cg * 8, q3);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += q2[e] * yr[e] + q3[e];
        }
      }
      float* d = s_dy + iy * g.RP + ix * BIG_CB + cg * 8;
      *reinterpret_cast<f32x4*>(d) = f32x4{v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4*>(d + 4) = f32x4{v[4], v[5], v[6], v[7]};
    }
    // the tile's own pixels: as stored, and activated
    for (int i = tid; i < g.TH * g.TW * 2; i += 256) {
      const int pix = i >> 1;
      const int hi = hi0 + pix / g.TW, wi = wi0 + pix % g.TW;
      float v[8], a[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { v[e] = 0.f; a[e] = 0.f; }
      if (cg_ok && hi < g.H && wi < g.W) {
        float qs[8], qh[8];
        VecIO<T, 8>::load(x + (((long)n * g.H + hi) * g.W + wi) * xps + big_chan_base(cgc, xss), v);
        VecIO<float, 8>::load(s_cf + 3 * BIG_CB + cg * 8, qs);
        VecIO<float, 8>::load(s_cf + 4 * BIG_CB + cg * 8, qh);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = v[e] * qs[e] + qh[e];
        act_apply_v(a, am);
      }
      float* d = s_x + pix * BIG_CB + cg * 8;
      *reinterpret_cast<f32x4*>(d) = f32x4{v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4*>(d + 4) = f32x4{v[4], v[5], v[6], v[7]};
      float* da = s_xa + pix * BIG_CB + cg * 8;
      *reinterpret_cast<f32x4*>(da) = f32x4{a[0], a[1], a[2], a[3]};
      *reinterpret_cast<f32x4*>(da + 4) = f32x4{a[4], a[5], a[6], a[7]};
    }
    __syncthreads();

    // ---- pass 1: input gradient
    for (int it = tid; it < nitems; it += 256) {
      const int rs = it >> 3;
      const int r = rs % g.TH, j = rs / g.TH;
      const int hi = hi0 + r, wis = wi0 + j * BIG_SW;
      if (hi >= g.H || wis >= g.W || !ch_ok) continue;
      f32x2 dx[BIG_SW];
#pragma unroll
      for (int t = 0; t < BIG_SW; ++t) dx[t] = f32x2{0.f, 0.f};
#pragma unroll 1
      for (int ky = 0; ky < K; ++ky) {
        const int numr = hi + P - ky;
        if (S > 1 && bpmod(numr, S) != 0) continue;
        const int ho = bfdiv(numr, S);
        if (ho < 0 || ho >= g.Ho) continue;   // rows outside the image hold zeros anyway
        const float* row = s_dy + (ho - hob) * g.RP + ((wis - wi0) / S) * BIG_CB + 2 * c2;
        f32x2 dy[DWN];
#pragma unroll
        for (int i = 0; i < DWN; ++i) dy[i] = *reinterpret_cast<const f32x2*>(row + i * BIG_CB);
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const f32x2 wv = *reinterpret_cast<const f32x2*>(s_w + (ky * K + kx) * BIG_CB + 2 * c2);
#pragma unroll
          for (int t = 0; t < BIG_SW; ++t) {
            const int num = t + P - kx;   // compile-time after unrolling
            if (bpmod(num, S) != 0) continue;
            dx[t] += dy[bfdiv(num, S) - RELMIN] * wv;
          }
        }
      }
      // epilogue: derivative of the producer's activation, rounding, statistics, store
      const int pix0 = r * g.TW + j * BIG_SW;
      T* hr = h + (((long)n * g.H + hi) * g.W) * hps + big_chan_base(ch & ~7, hss) + (ch & 7);
#pragma unroll
      for (int t = 0; t < BIG_SW; ++t) {
        const int wi = wis + t;
        if (wi < g.W) {
          const f32x2 xv = *reinterpret_cast<const f32x2*>(s_x + (pix0 + t) * BIG_CB + 2 * c2);
          const float pre[2] = {xv[0] * sc2[0] + sh2[0], xv[1] * sc2[1] + sh2[1]};
          float o[2] = {dx[t][0], dx[t][1]};
          act_bwd_v(o, pre, am);
          o[0] = (ch < g.C) ? to_f32(from_f32<T>(o[0])) : 0.f;
          o[1] = (ch + 1 < g.C) ? to_f32(from_f32<T>(o[1])) : 0.f;
          VecIO<T, 2>::store(hr + (long)wi * hps, o);
          s0[0] += o[0]; s1[0] += o[0] * xv[0];
          s0[1] += o[1]; s1[1] += o[1] * xv[1];
        }
      }
    }

    // ---- pass 2: weight gradient, dw[ky][kx] += sum over the tile's pixels of xa[hi][wi] * dYraw[(hi+P-ky)/S][(wi+P-kx)/S]
    if (dwp && ch_ok && wq < 2 * K) {
      auto half_row = [&](auto half) {
        constexpr int KX0 = decltype(half)::value * TG;
        constexpr int NT = bmin(TG, K - KX0);
        constexpr int JMIN = bfdiv(P - (KX0 + NT - 1), S), JMAX = bfdiv(BIG_SW - 1 + P - KX0, S);
        constexpr int NDY = JMAX - JMIN + 1;
        for (int r = 0; r < g.TH; ++r) {
          const int hi = hi0 + r;
          if (hi >= g.H) break;
          const int numr = hi + P - wky;
          if (S > 1 && bpmod(numr, S) != 0) continue;
          const int ho = bfdiv(numr, S);
          if (ho < 0 || ho >= g.Ho) continue;
          for (int j = 0; j < nstrips; ++j) {
            if (wi0 + j * BIG_SW >= g.W) break;
            const float* row = s_dy + (ho - hob) * g.RP + (j * BIG_SW / S + JMIN - RELMIN) * BIG_CB + 2 * c2;
            const float* xrow = s_xa + (r * g.TW + j * BIG_SW) * BIG_CB + 2 * c2;
            f32x2 dy[NDY], xa[BIG_SW];
#pragma unroll
            for (int i = 0; i < NDY; ++i) dy[i] = *reinterpret_cast<const f32x2*>(row + i * BIG_CB);
#pragma unroll
            for (int t = 0; t < BIG_SW; ++t) xa[t] = *reinterpret_cast<const f32x2*>(xrow + t * BIG_CB);   // zero beyond the image
#pragma unroll
            for (int i = 0; i < NT; ++i) {
#pragma unroll
              for (int t = 0; t < BIG_SW; ++t) {
                const int num = t + P - (KX0 + i);
                if (bpmod(num, S) != 0) continue;
                dacc[i] += xa[t] * dy[bfdiv(num, S) - JMIN];
              }
            }
          }
        }
      };
      if (whalf == 0) half_row(IC<0>{}); else half_row(IC<1>{});
    }
  }

  if (dwp && ch_ok && wq < 2 * K) {
    const int kx0 = whalf * TG;
#pragma unroll
    for (int i = 0; i < TG; ++i) {
      if (kx0 + i < K) {
        const int t = wky * K + kx0 + i;
        if (ch < g.C) dwp[((long)worker * g.C + ch) * KK + t] = dacc[i][0];
        if (ch + 1 < g.C) dwp[((long)worker * g.C + ch + 1) * KK + t] = dacc[i][1];
      }
    }
  }
  if (stats) big_flush_stats(s0, s1, s_st, stats, stat_ld, stat_rows, worker, g.nworkers, c_base, g.C);
}

// ------------------------------------------------------------------------------------------------ host side
// row pitch of an LDS window: the 8 rows a wave's lanes read (r, r + 1, ...; S window rows apart in the forward) start 16 banks apart
static int big_pitch(int lw, int step) {
  int rp = lw * BIG_CB;
  while ((rp * step) % 64 != 16) rp += 8;
  return rp;
}

static size_t big_lds_fwd(const BigGeom& g, int K) {
  return ((size_t)g.LH * g.RP + (size_t)K * K * BIG_CB + 8 * BIG_CB) * sizeof(float);
}
static size_t big_lds_bwd(const BigGeom& g, int K) {
  return ((size_t)g.LH * g.RP + (size_t)K * K * BIG_CB + (size_t)2 * g.TH * g.TW * BIG_CB + 5 * BIG_CB + 8 * BIG_CB) * sizeof(float);
}

static void big_window(BigGeom& g, int K, int S, int dir) {
  const int P = (K - 1) / 2;
  if (dir == 0) {
    g.LH = (g.TH - 1) * S + K;
    g.LW = (g.TW - 1) * S + K;
    g.RP = big_pitch(g.LW, S);
  } else {
    g.LH = bfdiv(g.TH - 1 + P, S) - bcdiv(P - (K - 1), S) + 1;
    g.LW = bfdiv(g.TW - 1 + P, S) - bfdiv(-P, S) + 1;
    g.RP = big_pitch(g.LW, 1);
  }
}

// The plan of the family: tile and LDS window for a shape and direction.  Tiles start at 16 x 16 pixels (forward stride 2: 8 x 16, the
// input window doubles) clipped to the map and are SHRUNK until the window fits the device's LDS limit: rows are halved first, then
// strips are dropped.  The smallest tile (2 x 4 pixels) needs under 30 KiB for k = 11, so every valid shape has a plan.
bool big_plan(const DwShape& s, int dir, DwPlan& p) {
  if (s.k != 9 && s.k != 11) return false;
  const int K = s.k, S = s.stride, P = (K - 1) / 2;
  BigGeom& g = p.bg;
  g.N = s.N; g.H = s.H; g.W = s.W; g.C = s.C;
  g.Ho = (s.H + 2 * P - K) / S + 1; g.Wo = (s.W + 2 * P - K) / S + 1;
  const int rows = dir ? s.H : g.Ho, cols = dir ? s.W : g.Wo;
  const int th_max = (dir == 0 && S == 2) ? 8 : 16;
  g.TH = rows < th_max ? rows : th_max;
  if (dir && (g.TH % 2)) g.TH += 1;   // input tiles start on even rows (stride 2)
  g.TW = cols < 16 ? (cols + BIG_SW - 1) / BIG_SW * BIG_SW : 16;
  const size_t cap = max_lds_bytes();
  for (;;) {
    big_window(g, K, S, dir);
    p.lds = dir ? big_lds_bwd(g, K) : big_lds_fwd(g, K);
    if (p.lds <= cap) break;
    if (g.TH > 2) g.TH = ((g.TH / 2) + 1) / 2 * 2;
    else if (g.TW > BIG_SW) g.TW -= BIG_SW;
    else return false;   // (a device with less than 30 KiB of LDS)
  }
  g.tiles_y = (rows + g.TH - 1) / g.TH;
  g.tiles_x = (cols + g.TW - 1) / g.TW;
  g.nslabs = (s.C + BIG_CB - 1) / BIG_CB;
  g.nworkers = 1;
  return true;
}

// persistent grid: as many workgroups as are resident at once, one partial row per worker (max_rows > 0), at most one worker per tile
static void big_workers(BigGeom& g, int per_cu, int max_rows) {
  if (per_cu < 1) per_cu = 1;
  long want = ((long)num_cus() * per_cu) / g.nslabs;
  const long max_env = dw_env().max_workers;
  const long ntiles = (long)g.N * g.tiles_y * g.tiles_x;
  if (max_env > 0 && want > max_env) want = max_env;
  if (max_rows > 0 && want > max_rows) want = max_rows;
  if (want > ntiles) want = ntiles;
  if (want < 1) want = 1;
  g.nworkers = (int)want;
}

template <typename F> static int big_dispatch(const DwShape& s, F&& f) {
  return dw_for_type(s.dtype, [&](auto tt) {
    if (s.k == 9) return s.stride == 1 ? f(tt, IC<9>{}, IC<1>{}) : f(tt, IC<9>{}, IC<2>{});
    return s.stride == 1 ? f(tt, IC<11>{}, IC<1>{}) : f(tt, IC<11>{}, IC<2>{});
  });
}

int big_launch_fwd(const DwPlan& p, const DwFwdArgs& a) {
  BigGeom g = p.bg;
  return big_dispatch(a.s, [&](auto tt, auto kc, auto sc) {
    typedef typename decltype(tt)::type T;
    auto kern = k_dwbig_fwd<T, decltype(kc)::value, decltype(sc)::value>;
    big_workers(g, resident_per_cu(kern, 256, p.lds), a.stats ? a.stat_rows : 0);
    hipLaunchKernelGGL(kern, dim3((unsigned)g.nworkers * g.nslabs), dim3(256), p.lds, a.st, (const T*)a.x, a.ldx, a.xss, a.sc, a.sh, a.relu, a.w,
                       a.ldw, (T*)a.y, a.ldy, a.yss, a.stats, a.stat_ld, a.stat_rows, g);
    return check_launch("dwconv_fwd");
  });
}

int big_launch_bwd(const DwPlan& p, const DwBwdArgs& a) {
  BigGeom g = p.bg;
  return big_dispatch(a.s, [&](auto tt, auto kc, auto sc) {
    typedef typename decltype(tt)::type T;
    auto kern = k_dwbig_bwd<T, decltype(kc)::value, decltype(sc)::value>;
    big_workers(g, resident_per_cu(kern, 256, p.lds), (a.stats || a.dw) ? a.part_rows : 0);
    hipLaunchKernelGGL(kern, dim3((unsigned)g.nworkers * g.nslabs), dim3(256), p.lds, a.st, (const T*)a.gup, a.ldg, a.gss, (const T*)a.yraw, a.ldyr,
                       a.yrss, a.c1, a.c2, a.c3, (const T*)a.x, a.ldx, a.xss, a.sc, a.sh, a.relu, a.w, a.ldw, (T*)a.h, a.ldh, a.hss,
                       a.dw ? a.dw_ws : nullptr, a.stats, a.stat_ld, a.part_rows, g);
    return dw_finish_bwd("dwconv_bwd", a, g.nworkers);
  });
}

}  // namespace atomnas
