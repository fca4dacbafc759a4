// Inference path: one launch per atomic block (InvertedResidualChannels / InvertedResidualChannelsFused, eval mode; with SE: below)
//
//     out = [x +] bn_p( Wp . act(bn_d( dw_k( act(bn_e( We . x )) ) )) )
//
// The 6x-wide hidden maps E (expand output) and D (depthwise output) never reach global memory.  A workgroup of 8 waves owns
// (image, output tile): it stages the x window of the tile (tile + halo of the block's largest k, clipped to the image: the halo
// outside the image is zeros of the ACTIVATED map, which no expand has to compute) in LDS once, then walks the hidden channels in
// chunks of CH channels inside one branch segment.  Per chunk:
//   1. expand on the matrix cores (mfma_f32_16x16x32_bf16, the weight rows as the A operand so that a lane ends up with 4 consecutive
//      channels of one window pixel), K = inp rounded up to 32;
//   2. raw value rounded to bf16, bn_e + activation in fp32, fp32 into LDS [window pixel][CH]; window positions outside the image are
//      zeroed once and never written: EXACT ZERO, not act(shift) (the depthwise convolution pads the activated map);
//   3. k x k taps from LDS on the VALU in fp32: a lane owns 4 channels x 4 consecutive output pixels of one row;
//   4. raw value rounded to bf16, bn_d + activation, rounded to bf16 into LDS [tile pixel][CH]: the projection's operand;
//   5. projection MFMAs into fp32 accumulators [tile pixels x oup] that stay in registers over the whole hidden loop.
// The epilogue rounds the raw projection sum to bf16, applies bn_p, adds the residual and stores once.  These are the rounding
// points of the plain bf16 storage model, so a network scores the same through this path and through the training decomposition up
// to accumulation order.  No atomics; a workgroup depends on its own image only: bit-reproducible and batch invariant.
//
// Squeeze-and-Excitation (InvertedResidualChannelsFused with se_ratio, the "+" networks; template parameter SE, atomnas_block_infer_se):
//     A = act(bn_d(bf16(dw)))  fp32, not rounded;   s[c] = mean_hw A[:, c];   gate = sigmoid(W2 . act(W1 . s + b1) + b2);   out = [x +] bn_p(bf16(Wp . bf16(gate * A)))
// The gate of one channel needs the squeeze of ALL hidden channels, so the kernel serves SE only where ONE workgroup owns the whole map
// (stride 1, at most 256 pixels) and runs the chunk loop TWICE (the same code, so the recomputed A is bit-identical):
//   pass 0  steps 1-3, bn_d + activation in fp32; every depthwise work item adds its own 4 pixels and writes one fp32 partial per
//           (row, strip) into the Ds / Wps region (idle in this pass); after the barrier one thread per channel adds the partials in
//           row-major order into pooled[HT].  Only tile pixels are ever summed: the padding rows of the MFMA tiles do not exist here.
//   gate    hpre: a wave per hidden unit, butterfly sum over the channels; gate: a thread per channel, the hidden units in sequence
//           (the scheme and the packed fp32 operands of csrc/se.hip k_se_mlp).  pooled, gate and act(hpre) live in LDS.
//   pass 1  steps 1-5 with bf16(gate * A) as the projection's operand.
// The expand and tap work is done twice (recompute factor 2); every sum has a fixed order that depends on the shape alone.
//
// The three BatchNorms arrive as per-channel fp32 scale / shift (atomnas_bn_eval_coeffs), the weights in the pointwise GEMMs' packed
// layouts (atomnas_pack_weights), the taps tap-major [k*k][channels] per segment.
#include "common.h"

namespace atomnas {
namespace {

constexpr int BI_THREADS = 512, BI_WAVES = BI_THREADS / 64, BI_MAXSEG = 8;
constexpr int BI_R = 4;                                  // output pixels of one row per depthwise work item
constexpr int BI_B = 8;                                  // 16-byte staging copies in flight per lane
constexpr size_t BI_LDS_BUDGET = 160 * 1024 - 512;       // gfx950: 160 KiB per CU (the predicate must answer without a device)
constexpr int BI_MAX_ACC_TILES = 24;                     // 16x16 accumulator tiles per wave: 96 registers of the 256 a lane has at 8 waves

struct BiSeg {
  const float* taps;   // fp32 [k*k][ldw]
  int off, ch, k, ldw;
};

struct BiArgs {
  const bf16_t* x; bf16_t* out;
  const bf16_t* we; const bf16_t* wp;
  const float *es, *eb, *ds, *db, *ps, *pb;
  int ldx, ldo, ldwe, ldwp;
  int N, H, W, Ho, Wo, inp, oup, stride, act, expand, res, nseg;
  BiSeg seg[BI_MAXSEG];
  // tiling (bi_plan)
  int toh, tow, tiles_x, ih, iw, ipix, erows, xr16, kp, ch, kmax, tpix, tp16, nt;
  int xstr, estr, dstr;            // LDS row pitches in elements: x window / weights (bf16), E (fp32), D / projection weights (bf16)
  unsigned o_xs, o_es, o_ds, o_wes, o_wps, o_ts, o_cs;   // byte offsets of the LDS arrays
};

// the SE instances' arguments: BiArgs (so that the plain instances keep theirs, and their code) + the gate's operands
struct BiArgsSe : BiArgs {
  const float *w1p, *w2t, *b1, *b2p;   // fp32 [se_hid][ldse] x 2 (channels contiguous, zeros in padding columns), [se_hid], [HT]
  int se_hid, ldse, ht;
  float inv_hw;
  unsigned o_pool, o_gate, o_hs;       // byte offsets of pooled[HT], gate[HT], act(hpre)[se_hid]
};
template <bool SE> struct BiArgsOf { typedef BiArgs type; };
template <> struct BiArgsOf<true> { typedef BiArgsSe type; };

struct BiShape {
  int N, H, W, inp, oup, nseg, off[BI_MAXSEG], ch[BI_MAXSEG], k[BI_MAXSEG], stride, act, expand, res, se, dtype, se_hid;
};

struct BiPlan {
  int toh, tow, ch, mt, ntmax, kmax, kp;
  size_t lds;
};

__device__ __forceinline__ float bf16_round(float v) { return (float)(bf16_t)v; }

// K x K taps of 4 channels for BI_R consecutive output pixels of one row.  e: the activated expand map at the strip's first input
// position (+ the lane's channel quad), t: the chunk's taps at the quad.  Each input value is read once per tap row and feeds every
// output pixel it belongs to.
template <int K, int S>
__device__ __forceinline__ void dw_strip(const float* __restrict__ e, int rowstride, int estr, const float* __restrict__ t, int tstr,
                                         f32x4 (&acc)[BI_R]) {
  constexpr int NX = (BI_R - 1) * S + K;
#pragma unroll 1
  for (int ky = 0; ky < K; ++ky) {
    f32x4 tp[K];
#pragma unroll
    for (int kx = 0; kx < K; ++kx) tp[kx] = *reinterpret_cast<const f32x4*>(t + (ky * K + kx) * tstr);
    const float* er = e + ky * rowstride;
#pragma unroll
    for (int ix = 0; ix < NX; ++ix) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(er + ix * estr);
#pragma unroll
      for (int r = 0; r < BI_R; ++r) {
        const int kx = ix - r * S;
        if (kx >= 0 && kx < K) acc[r] += v * tp[kx];
      }
    }
  }
}

template <int MT, int NTMAX, bool SE>
__global__ __launch_bounds__(BI_THREADS) void k_block_infer(const typename BiArgsOf<SE>::type a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bi_smem[];
  bf16_t* Xs = reinterpret_cast<bf16_t*>(bi_smem + a.o_xs);     // [xr16][xstr]   x window clipped to the image, zeros beyond inp
  float* Es = reinterpret_cast<float*>(bi_smem + a.o_es);       // [erows][estr]  activated expand chunk over the whole window
  bf16_t* Ds = reinterpret_cast<bf16_t*>(bi_smem + a.o_ds);     // [tp16][dstr]   activated depthwise chunk
  bf16_t* Wes = reinterpret_cast<bf16_t*>(bi_smem + a.o_wes);   // [ch][xstr]     expand weights of the chunk
  bf16_t* Wps = reinterpret_cast<bf16_t*>(bi_smem + a.o_wps);   // [nt*16][dstr]  projection weights of the chunk
  float* Ts = reinterpret_cast<float*>(bi_smem + a.o_ts);       // [k*k][ch]      taps of the chunk
  float* Cs = reinterpret_cast<float*>(bi_smem + a.o_cs);       // [4][ch]        bn_d scale, shift, bn_e scale, shift of the chunk

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int n = blockIdx.y, ty = blockIdx.x / a.tiles_x, tx = blockIdx.x % a.tiles_x;
  const int oy0 = ty * a.toh, ox0 = tx * a.tow;
  const int S = a.stride, pmax = (a.kmax - 1) / 2;
  const int gy0 = oy0 * S - pmax, gx0 = ox0 * S - pmax;   // the window's origin in the input map
  const int H = a.H, W = a.W, iw = a.iw, ipix = a.ipix;
  const int xstr = a.xstr, estr = a.estr, dstr = a.dstr, CH = a.ch;
  const Act act = act_of(a.act);
  const long img = (long)n * H * W;
  const bf16x8 zero8 = {};
  // the window clipped to the image: rows [cy0, cy1) x columns [cx0, cx1) of the input map, cpix pixels in row-major order
  const int cy0 = max(gy0, 0), cy1 = min(gy0 + a.ih, H), cx0 = max(gx0, 0), cx1 = min(gx0 + iw, W);
  const int cw = max(cx1 - cx0, 0), cpix = cw * max(cy1 - cy0, 0), cp16 = (cpix + 15) / 16 * 16;

  // Staging copies are 16 bytes per lane and BI_B of them in flight: every copy loop issues its loads first and stores afterwards (one
  // load round trip per BI_B copies; a workgroup alone on its CU has nothing else to hide the latency of a dependent copy behind).
  if (a.expand) {
    const int k8 = a.kp / 8;
    for (int base = tid; base < cp16 * k8; base += BI_THREADS * BI_B) {
      bf16x8 v[BI_B];
#pragma unroll
      for (int j = 0; j < BI_B; ++j) {
        const int u = base + j * BI_THREADS, p = u / k8, c = (u % k8) * 8;
        v[j] = zero8;
        if (p < cpix && c < a.inp) v[j] = *reinterpret_cast<const bf16x8*>(a.x + (img + (long)(cy0 + p / cw) * W + cx0 + p % cw) * a.ldx + c);
      }
#pragma unroll
      for (int j = 0; j < BI_B; ++j) {
        const int u = base + j * BI_THREADS, p = u / k8, c = (u % k8) * 8;
        if (p < cp16) *reinterpret_cast<bf16x8*>(Xs + p * xstr + c) = v[j];
      }
    }
    for (int u = tid; u < a.erows * (estr / 4); u += BI_THREADS) *reinterpret_cast<f32x4*>(Es + u * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int u = tid; u < a.tp16 * (dstr / 8); u += BI_THREADS) *reinterpret_cast<bf16x8*>(Ds + u * 8) = zero8;
  if constexpr (SE)   // channels between two segments belong to no chunk: their squeeze is zero (and their gate columns hold zeros)
    for (int c = tid; c < a.ht; c += BI_THREADS) reinterpret_cast<float*>(bi_smem + a.o_pool)[c] = 0.f;

  f32x4 acc[MT][NTMAX];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < NTMAX; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  int pass = 0;   // SE: the chunk loop runs twice, 0 squeeze, 1 project
  do {
  for (int si = 0; si < a.nseg; ++si) {
    const BiSeg sg = a.seg[si];
    const int K = sg.k, off = pmax - (K - 1) / 2;   // the segment's own padding inside the window of the largest k
    for (int c0 = sg.off; c0 < sg.off + sg.ch; c0 += CH) {
      const int cv = min(CH, sg.off + sg.ch - c0);   // channels of this chunk (a multiple of 8; of 16 in an expanding block)
      const int cv32 = (cv + 31) / 32 * 32;
      // ---- stage the chunk's expand weights, projection weights, taps and BatchNorm coefficients: ONE index space of 16-byte copies, so
      // that the chunk pays one load round trip (a coefficient load from global memory inside a phase stalls the whole workgroup)
      {
        const int k8 = a.kp / 8, c8 = cv32 / 8, c4 = cv / 4;
        const int nwe = a.expand ? cv * k8 : 0, nwp = SE && pass == 0 ? 0 : a.nt * 16 * c8, nts = K * K * c4, total = nwe + nwp + nts + (a.expand ? 4 : 2) * c4;
        for (int base = tid; base < total; base += BI_THREADS * BI_B) {
          f32x4 v[BI_B];
          unsigned dst[BI_B];   // byte offset in LDS; ~0u: nothing to store
#pragma unroll
          for (int j = 0; j < BI_B; ++j) {
            int u = base + j * BI_THREADS;
            v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            dst[j] = ~0u;
            if (u < nwe) {
              const int r = u / k8, c = (u % k8) * 8;
              v[j] = *reinterpret_cast<const f32x4*>(a.we + (long)(c0 + r) * a.ldwe + c);
              dst[j] = a.o_wes + (unsigned)(r * xstr + c) * 2;
            } else if (u < nwe + nwp) {
              u -= nwe;
              const int o = u / c8, c = (u % c8) * 8;
              if (c < cv) v[j] = *reinterpret_cast<const f32x4*>(a.wp + (long)o * a.ldwp + c0 + c);
              dst[j] = a.o_wps + (unsigned)(o * dstr + c) * 2;
            } else if (u < nwe + nwp + nts) {
              u -= nwe + nwp;
              const int t = u / c4, c = (u % c4) * 4;
              v[j] = *reinterpret_cast<const f32x4*>(sg.taps + (long)t * sg.ldw + (c0 - sg.off) + c);
              dst[j] = a.o_ts + (unsigned)(t * CH + c) * 4;
            } else if (u < total) {
              u -= nwe + nwp + nts;
              const int w = u / c4, c = (u % c4) * 4;
              const float* src = w == 0 ? a.ds : w == 1 ? a.db : w == 2 ? a.es : a.eb;
              v[j] = *reinterpret_cast<const f32x4*>(src + c0 + c);
              dst[j] = a.o_cs + (unsigned)(w * CH + c) * 4;
            }
          }
#pragma unroll
          for (int j = 0; j < BI_B; ++j)
            if (dst[j] != ~0u) *reinterpret_cast<f32x4*>(bi_smem + dst[j]) = v[j];
        }
      }
      __syncthreads();
      // ---- E chunk: expand MFMAs + bn_e + activation over the pixels inside the image
      if (a.expand) {
        const int ntile = cv / 16, ksteps = a.kp / 32;
        for (int mt = wave; mt < cp16 / 16; mt += BI_WAVES) {
          const int p = mt * 16 + l15;
          const bool inside = p < cpix;
          const int wp = inside ? (cy0 + p / cw - gy0) * iw + (cx0 + p % cw - gx0) : 0;   // the pixel's place in the window
          const bf16_t* xb = Xs + p * xstr + 8 * lq;
          for (int t0 = 0; t0 < ntile; t0 += 2) {
            const bool two = t0 + 1 < ntile;
            f32x4 e0 = {0.f, 0.f, 0.f, 0.f}, e1 = {0.f, 0.f, 0.f, 0.f};
            const bf16_t* w0 = Wes + (t0 * 16 + l15) * xstr + 8 * lq;
            const bf16_t* w1 = w0 + (two ? 16 * xstr : 0);
            for (int ks = 0; ks < ksteps; ++ks) {
              const bf16x8 b = *reinterpret_cast<const bf16x8*>(xb + ks * 32);
              e0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(w0 + ks * 32), b, e0, 0, 0, 0);
              e1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(w1 + ks * 32), b, e1, 0, 0, 0);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              if (h == 1 && !two) break;
              const f32x4 e = h ? e1 : e0;
              const int c = (t0 + h) * 16 + lq * 4;
              const f32x4 sc = *reinterpret_cast<const f32x4*>(Cs + 2 * CH + c), sh = *reinterpret_cast<const f32x4*>(Cs + 3 * CH + c);
              float v[4];
#pragma unroll
              for (int r = 0; r < 4; ++r) v[r] = bf16_round(e[r]) * sc[r] + sh[r];
              act_apply_v(v, act);
              if (inside) *reinterpret_cast<f32x4*>(Es + wp * estr + c) = f32x4{v[0], v[1], v[2], v[3]};
            }
          }
        }
      } else {   // the first block of a network: the depthwise stage reads x itself
        const int c8 = cv / 8;
        for (int base = tid; base < ipix * c8; base += BI_THREADS * BI_B) {
          bf16x8 v[BI_B];
#pragma unroll
          for (int j = 0; j < BI_B; ++j) {
            const int u = base + j * BI_THREADS, p = u / c8, c = (u % c8) * 8;
            const int gy = gy0 + p / iw, gx = gx0 + p % iw;
            v[j] = zero8;
            if (p < ipix && gy >= 0 && gy < H && gx >= 0 && gx < W) v[j] = *reinterpret_cast<const bf16x8*>(a.x + (img + (long)gy * W + gx) * a.ldx + c0 + c);
          }
#pragma unroll
          for (int j = 0; j < BI_B; ++j) {
            const int u = base + j * BI_THREADS, p = u / c8, c = (u % c8) * 8;
            if (p < ipix) {
              *reinterpret_cast<f32x4*>(Es + p * estr + c) = f32x4{(float)v[j][0], (float)v[j][1], (float)v[j][2], (float)v[j][3]};
              *reinterpret_cast<f32x4*>(Es + p * estr + c + 4) = f32x4{(float)v[j][4], (float)v[j][5], (float)v[j][6], (float)v[j][7]};
            }
          }
        }
      }
      __syncthreads();
      // ---- D chunk: taps on the VALU + bn_d + activation -> bf16 operand
      {
        const int nq = cv32 / 4, strips = (a.tow + BI_R - 1) / BI_R;
        for (int it = tid; it < nq * strips * a.toh; it += BI_THREADS) {
          const int q = it % nq, rest = it / nq;
          const int ox = (rest % strips) * BI_R, oy = rest / strips;
          f32x4 d[BI_R];
#pragma unroll
          for (int r = 0; r < BI_R; ++r) d[r] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (q * 4 < cv) {   // (else: the zero columns that fill the projection's last k-step)
            const float* e = Es + ((oy * S + off) * iw + ox * S + off) * estr + q * 4;
            const float* t = Ts + q * 4;
            const int rs = iw * estr;
            switch (K * 2 + S) {
              case 3 * 2 + 1: dw_strip<3, 1>(e, rs, estr, t, CH, d); break;
              case 3 * 2 + 2: dw_strip<3, 2>(e, rs, estr, t, CH, d); break;
              case 5 * 2 + 1: dw_strip<5, 1>(e, rs, estr, t, CH, d); break;
              case 5 * 2 + 2: dw_strip<5, 2>(e, rs, estr, t, CH, d); break;
              case 7 * 2 + 1: dw_strip<7, 1>(e, rs, estr, t, CH, d); break;
              case 7 * 2 + 2: dw_strip<7, 2>(e, rs, estr, t, CH, d); break;
              case 9 * 2 + 1: dw_strip<9, 1>(e, rs, estr, t, CH, d); break;
              case 9 * 2 + 2: dw_strip<9, 2>(e, rs, estr, t, CH, d); break;
              case 11 * 2 + 1: dw_strip<11, 1>(e, rs, estr, t, CH, d); break;
              default: dw_strip<11, 2>(e, rs, estr, t, CH, d); break;
            }
            const f32x4 sc = *reinterpret_cast<const f32x4*>(Cs + q * 4), sh = *reinterpret_cast<const f32x4*>(Cs + CH + q * 4);
#pragma unroll
            for (int r = 0; r < BI_R; ++r) {
              float v[4];
#pragma unroll
              for (int j = 0; j < 4; ++j) v[j] = bf16_round(d[r][j]) * sc[j] + sh[j];
              act_apply_v(v, act);
              d[r] = f32x4{v[0], v[1], v[2], v[3]};
            }
            if constexpr (SE) {
              if (pass == 0) {   // the work item's own pixels, left to right: one partial per (row, strip) and channel
                f32x4 s = d[0];
#pragma unroll
                for (int r = 1; r < BI_R; ++r)
                  if (ox + r < a.tow) s += d[r];
                *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(Ds) + rest * CH + q * 4) = s;
              } else {
                const f32x4 g = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(bi_smem + a.o_gate) + c0 + q * 4);
#pragma unroll
                for (int r = 0; r < BI_R; ++r) d[r] *= g;
              }
            }
          }
          if (SE && pass == 0) continue;
#pragma unroll
          for (int r = 0; r < BI_R; ++r)
            if (ox + r < a.tow) {
              const float v[4] = {d[r][0], d[r][1], d[r][2], d[r][3]};
              VecIO<bf16_t, 4>::store(Ds + (oy * a.tow + ox + r) * dstr + q * 4, v);
            }
        }
      }
      __syncthreads();
      if constexpr (SE) {
        if (pass == 0) {   // ---- squeeze: the chunk's partials in row-major order, one thread per channel
          const float* ps = reinterpret_cast<const float*>(Ds);
          float* pooled = reinterpret_cast<float*>(bi_smem + a.o_pool);
          const int rows = (a.tow + BI_R - 1) / BI_R * a.toh;
          for (int c = tid; c < cv; c += BI_THREADS) {
            float s = 0.f;
#pragma unroll 8
            for (int r = 0; r < rows; ++r) s += ps[r * CH + c];
            pooled[c0 + c] = s;
          }
        }
      }
      // ---- projection: accumulate the chunk
      for (int ks = 0; ks < (SE && pass == 0 ? 0 : cv32 / 32); ++ks) {
        bf16x8 b[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const int mt = min(wave + BI_WAVES * m, a.tp16 / 16 - 1);
          b[m] = *reinterpret_cast<const bf16x8*>(Ds + (mt * 16 + l15) * dstr + ks * 32 + 8 * lq);
        }
#pragma unroll
        for (int t = 0; t < NTMAX; ++t) {
          if (t < a.nt) {
            const bf16x8 w = *reinterpret_cast<const bf16x8*>(Wps + (t * 16 + l15) * dstr + ks * 32 + 8 * lq);
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, b[m], acc[m][t], 0, 0, 0);
          }
        }
      }
      __syncthreads();
    }
  }
  if constexpr (SE) {
    if (pass == 0) {   // ---- gate (csrc/se.hip k_se_mlp): the trailing barrier of the chunk loop has completed pooled
      const float* pooled = reinterpret_cast<const float*>(bi_smem + a.o_pool);
      float* gate = reinterpret_cast<float*>(bi_smem + a.o_gate);
      float* hs = reinterpret_cast<float*>(bi_smem + a.o_hs);
      // the partials have overwritten Ds: its padding rows are zeros again for the projection
      for (int u = tid; u < a.tp16 * (dstr / 8); u += BI_THREADS) *reinterpret_cast<bf16x8*>(Ds + u * 8) = zero8;
      for (int j = wave; j < a.se_hid; j += BI_WAVES) {
        const float* w = a.w1p + (long)j * a.ldse;
        float s = 0.f;
#pragma unroll 4
        for (int c = lane; c < a.ht; c += 64) s += w[c] * (pooled[c] * a.inv_hw);
        s = wave_sum(s);
        if (lane == 0) hs[j] = act_apply(s + a.b1[j], act);
      }
      __syncthreads();
      for (int c = tid; c < a.ht; c += BI_THREADS) {
        float s = a.b2p[c];
#pragma unroll 8
        for (int j = 0; j < a.se_hid; ++j) s += a.w2t[(long)j * a.ldse + c] * hs[j];
        gate[c] = 1.f / (1.f + __expf(-s));
      }
      __syncthreads();
    }
  }
  } while (SE && ++pass < 2);

  // ---- epilogue: raw sum rounded to bf16, bn_p, residual, one store
  const long oimg = (long)n * a.Ho * a.Wo;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int mt = wave + BI_WAVES * m;
    const int p = mt * 16 + l15;
    const int oy = oy0 + p / a.tow, ox = ox0 + p % a.tow;
    if (mt * 16 >= a.tp16 || p >= a.tpix || oy >= a.Ho || ox >= a.Wo) continue;
#pragma unroll
    for (int t = 0; t < NTMAX; ++t) {
      const int o = t * 16 + lq * 4;
      if (t < a.nt && o < a.oup) {
        const f32x4 sc = *reinterpret_cast<const f32x4*>(a.ps + o), sh = *reinterpret_cast<const f32x4*>(a.pb + o);
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = bf16_round(acc[m][t][r]) * sc[r] + sh[r];
        if (a.res) {
          float xr[4];
          VecIO<bf16_t, 4>::load(a.x + (img + (long)oy * W + ox) * a.ldx + o, xr);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += xr[r];
        }
        VecIO<bf16_t, 4>::store(a.out + (oimg + (long)oy * a.Wo + ox) * a.ldo + o, v);
      }
    }
  }
}

inline int pad_to(int v, int m) { return (v + m - 1) / m * m; }

// the shape arguments of the C entries as they arrive
struct BiDims { int N, H, W, inp, oup, nseg; const int *seg_off, *seg_ch, *seg_k; int stride, act, expand, residual, dtype; };

// -> s; false where the segment lists cannot even be read (the one guard of the predicates and of the launch)
bool bi_shape(BiShape& s, const BiDims& d, bool se, int se_hid) {
  if (d.nseg < 1 || d.nseg > BI_MAXSEG || !d.seg_off || !d.seg_ch || !d.seg_k) return false;
  s.N = d.N, s.H = d.H, s.W = d.W, s.inp = d.inp, s.oup = d.oup, s.nseg = d.nseg, s.stride = d.stride, s.act = d.act, s.expand = d.expand != 0,
  s.res = d.residual != 0, s.se = se, s.dtype = d.dtype, s.se_hid = se_hid;
  for (int i = 0; i < d.nseg; ++i) s.off[i] = d.seg_off[i], s.ch[i] = d.seg_ch[i], s.k[i] = d.seg_k[i];
  return true;
}

// What one workgroup works on and where it keeps it: the tile geometry and the byte offset of every LDS array of k_block_infer, for a
// tile of toh x tow output pixels and chunks of ch hidden channels.  The ONLY place either is computed: bi_plan takes `total` to the
// budget, bi_launch copies the rest into BiArgs.
struct BiLayout {
  int ih, iw, ipix, erows, xr16, tpix, tp16, nt, ht;   // ht: the padded hidden width, where the last segment ends
  int xstr, estr, dstr;
  unsigned o_xs, o_wes, o_es, o_ds, o_wps, o_ts, o_cs, o_pool, o_gate, o_hs;
  size_t total;
};

BiLayout bi_layout(const BiShape& s, int kmax, int kp, int toh, int tow, int ch) {
  BiLayout l = {};
  l.ih = (toh - 1) * s.stride + kmax, l.iw = (tow - 1) * s.stride + kmax, l.ipix = l.ih * l.iw;
  l.erows = l.ipix + 8;   // slack: the last strip of a row reads up to 3 * stride pixels past it
  l.xr16 = pad_to((l.ih < s.H ? l.ih : s.H) * (l.iw < s.W ? l.iw : s.W), 16);   // the window clipped to the image
  l.tpix = toh * tow, l.tp16 = pad_to(l.tpix, 16), l.nt = (s.oup + 15) / 16;
  l.xstr = kp + 8, l.estr = ch + 4, l.dstr = ch + 8;
  l.ht = s.off[s.nseg - 1] + s.ch[s.nseg - 1];
  // the Ds + Wps region; with SE it also holds pass 0's fp32 partials, one [ch] row per (map row, strip)
  const size_t ds = (size_t)l.tp16 * l.dstr * 2, dw = ds + (size_t)l.nt * 16 * l.dstr * 2;
  const size_t parts = s.se ? (size_t)((tow + BI_R - 1) / BI_R) * toh * ch * 4 : 0;
  size_t o = 0;
  l.o_xs = (unsigned)o, o += s.expand ? (size_t)l.xr16 * l.xstr * 2 : 0;
  l.o_wes = (unsigned)o, o += s.expand ? (size_t)ch * l.xstr * 2 : 0;
  l.o_es = (unsigned)o, o += (size_t)l.erows * l.estr * 4;
  l.o_ds = (unsigned)o, l.o_wps = (unsigned)(o + ds), o += dw > parts ? dw : parts;
  l.o_ts = (unsigned)o, o += (size_t)kmax * kmax * ch * 4;
  l.o_cs = (unsigned)o, o += (size_t)4 * ch * 4;
  if (s.se) {
    l.o_pool = (unsigned)o, o += (size_t)l.ht * 4;
    l.o_gate = (unsigned)o, o += (size_t)l.ht * 4;
    l.o_hs = (unsigned)o, o += (size_t)pad_to(s.se_hid, 4) * 4;
  }
  l.total = o;
  return l;
}

// The COMPLETE accept / reject decision and the tiling, pure host arithmetic (no device query): the entry point and the predicate share it.
// SE (atomnas_block_infer_se only): stride 1, expanding, the whole map in one workgroup, HT <= 4096, 1 <= se_hid <= 512.
bool bi_plan(const BiShape& s, BiPlan& p, BiLayout& l) {
  if (s.dtype != DT_BF16) return false;
  if (s.se && (s.stride != 1 || !s.expand || s.se_hid < 1 || s.se_hid > 512)) return false;
  if (s.N < 1 || s.N > 65535 || s.H < 1 || s.W < 1 || (long)s.H * s.W > (1L << 24)) return false;
  if (s.stride != 1 && s.stride != 2) return false;
  if (s.act < ACT_NONE || s.act > ACT_SWISH) return false;
  if (s.nseg < 1 || s.nseg > BI_MAXSEG) return false;
  if (s.inp < 8 || s.inp % 8 || s.inp > 1024 || s.oup < 8 || s.oup % 8 || s.oup > 320) return false;
  if (s.res && (s.stride != 1 || s.inp != s.oup)) return false;
  int kmax = 0, chmax = 0, end = 0;
  for (int i = 0; i < s.nseg; ++i) {
    const int k = s.k[i];
    if (k != 3 && k != 5 && k != 7 && k != 9 && k != 11) return false;
    if (s.ch[i] < 8 || s.ch[i] % (s.expand ? 16 : 8) || s.off[i] < end || s.off[i] % 8) return false;
    end = s.off[i] + s.ch[i];
    kmax = k > kmax ? k : kmax;
    chmax = s.ch[i] > chmax ? s.ch[i] : chmax;
  }
  if (end > 8192 || (!s.expand && end > s.inp) || (s.se && end > 4096)) return false;
  const int nt = (s.oup + 15) / 16;
  const int ntmax = nt <= 2 ? 2 : nt <= 4 ? 4 : nt <= 8 ? 8 : nt <= 12 ? 12 : 20;
  const int Ho = (s.H - 1) / s.stride + 1, Wo = (s.W - 1) / s.stride + 1;
  const int kp = s.expand ? pad_to(s.inp, 32) : 0;
  // tiles: a whole map of up to 16 MFMA row tiles per workgroup (no expand recompute), else from the largest tile down
  const int cand[6][2] = {{Ho, Wo}, {16, 16}, {8, 16}, {8, 8}, {4, 8}, {4, 4}};
  for (int ci = 0; ci < 6; ++ci) {
    if (ci == 0 && (long)Ho * Wo > 256) continue;
    if (s.se && ci) break;   // the squeeze is a reduction inside the workgroup: whole maps only
    const int toh = cand[ci][0] < Ho ? cand[ci][0] : Ho, tow = cand[ci][1] < Wo ? cand[ci][1] : Wo;
    const int mt = (toh * tow + 16 * BI_WAVES - 1) / (16 * BI_WAVES);   // 16-pixel MFMA row tiles per wave
    if (mt > 2 || mt * ntmax > BI_MAX_ACC_TILES) continue;
    for (int ch = pad_to(chmax, 32) < 128 ? pad_to(chmax, 32) : 128; ch >= 32; ch -= 32) {
      l = bi_layout(s, kmax, kp, toh, tow, ch);
      if (l.total <= BI_LDS_BUDGET) {
        p.toh = toh, p.tow = tow, p.ch = ch, p.mt = mt, p.ntmax = ntmax, p.kmax = kmax, p.kp = kp, p.lds = l.total;
        return true;
      }
    }
  }
  return false;
}

// padded hidden channels; x the window's pixels (BiLayout::ipix): the hidden work of one workgroup, which both rules below are stated in
long bi_hidden(const BiShape& s) {
  long hidden = 0;
  for (int i = 0; i < s.nseg; ++i) hidden += s.ch[i];
  return hidden;
}

// Where the kernel is FASTER than the launch-per-stage decomposition (functional.block_forward in eval mode), measured block by block
// on an MI355X at batch 256 (profiles/infer_bench.txt; the table is in DESIGN.md): expanding blocks whose whole map sits in one
// workgroup (stride 1, no expand recompute) with little hidden work -- padded hidden channels x window pixels <= 140,000, the searched
// networks' 14x14 and 7x7 stages -- and an output of at most 192 channels.  Everything else measured slower (the chunk loop of one
// workgroup per CU does not hide its phases behind each other) and is reported as unsupported, so that it takes the existing path.
bool bi_profitable(const BiShape& s, const BiPlan& p, const BiLayout& l) {
  const int Ho = (s.H - 1) / s.stride + 1, Wo = (s.W - 1) / s.stride + 1;
  if (!s.expand || s.stride != 1 || p.toh != Ho || p.tow != Wo || s.oup > 192) return false;
  return bi_hidden(s) * l.ipix <= 140000;
}

// The same question for the SE instances (atomnas_block_infer_se_supported).  The two passes double the expand and tap work and every
// image's workgroup reads both gate matrices, so the plain rule does not carry over.  Measured block by block on an MI355X for
// AtomNAS-C+ at batches 1, 8 and 256, two runs (profiles/infer_bench_se.txt; the table is in DESIGN.md): the existing path costs
// 0.17-0.19 ms per block at all three batches (its eight launches), the fused launch 0.10-0.14 ms on the 14x14 blocks of up to 192
// padded hidden channels -- 1.22-1.85x, the two runs within 0.17x of each other -- and 0.23-1.31 ms on everything wider (7x7 with
// 656-2336 channels 0.16-0.81x, 14x14 with 928 channels 0.31-0.53x): one workgroup per image walks the chunks twice, one after the
// other.  The rule is the largest measured winner (192 channels x 400 window pixels, 96 outputs); nothing was measured between it
// and the smallest loser (656 x 169), so that range stays on the existing path.  Batches: the per-block loop is bound by ISSUING the
// existing path's launches, which a whole forward is only while the GPU keeps up: AtomNAS-C+ with these six blocks fused runs 1.29x
// faster (eager; 1.29-1.59x as a graph) at batches 1-32 and 1.09x at 64, and 0.96-0.98x at 128 and 256 in both runs -- so N <= 64.
bool bi_profitable_se(const BiShape& s, const BiLayout& l) {
  const long hidden = bi_hidden(s);
  return s.N <= 64 && s.oup <= 96 && hidden <= 192 && hidden * l.ipix <= 77000;
}

// The body of all four predicates: the shape, its plan and, where asked, whether the kernel measured faster
int bi_answer(const BiDims& d, bool se, int se_hid, bool profitable) {
  BiShape s; BiPlan p; BiLayout l;
  if (!bi_shape(s, d, se, se_hid) || !bi_plan(s, p, l)) return 0;
  return !profitable || (se ? bi_profitable_se(s, l) : bi_profitable(s, p, l)) ? 1 : 0;
}

template <int MT, int NTMAX, bool SE>
int bi_run(const typename BiArgsOf<SE>::type& a, dim3 grid, size_t lds, hipStream_t st) {
  (void)resident_per_cu(k_block_infer<MT, NTMAX, SE>, BI_THREADS, lds);   // opts the kernel into its dynamic LDS size (cached)
  hipLaunchKernelGGL((k_block_infer<MT, NTMAX, SE>), grid, dim3(BI_THREADS), lds, st, a);
  return check_launch(SE ? "block_infer_se" : "block_infer");
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the operands of atomnas_block_infer in the order of its arguments, and those atomnas_block_infer_se adds
struct BiOperands {
  const void* x; int ldx; void* out; int ldo; const void* we; int ldwe; const void* wp; int ldwp;
  const float* const* taps;
  const float *e_scale, *e_shift, *d_scale, *d_shift, *p_scale, *p_shift;
};
struct BiGate { const float *w1p, *w2t, *b1, *b2p; int se_hid, ldse; };

// SE == false: atomnas_block_infer (g is unused); SE == true: atomnas_block_infer_se
template <bool SE>
int bi_launch(const BiDims& d, const BiOperands& o, const BiGate& g, void* stream) {
  BiShape s; BiPlan p; BiLayout l;
  ATOMNAS_REQUIRE(bi_shape(s, d, SE, g.se_hid) && o.taps, "block_infer: 1..%d segments with offsets, channels, kernel sizes and taps", BI_MAXSEG);
  ATOMNAS_REQUIRE(bi_plan(s, p, l), "block_infer: shape outside the fused kernel's envelope (ask atomnas_block_infer%s_runs first): N=%d %dx%d inp=%d oup=%d stride=%d dtype=%d",
                  SE ? "_se" : "", s.N, s.H, s.W, s.inp, s.oup, s.stride, s.dtype);
  ATOMNAS_REQUIRE(p.lds <= max_lds_bytes(), "block_infer: needs %zu bytes of LDS, the device grants %zu", p.lds, max_lds_bytes());
  ATOMNAS_REQUIRE(o.x && o.out && o.wp && o.d_scale && o.d_shift && o.p_scale && o.p_shift && (!s.expand || (o.we && o.e_scale && o.e_shift)), "block_infer: null operand");
  ATOMNAS_REQUIRE(o.ldx >= s.inp && o.ldx % 8 == 0 && o.ldo >= s.oup && o.ldo % 4 == 0 && aligned16(o.x) && ((uintptr_t)o.out & 7) == 0, "block_infer: activation pitch / alignment");
  ATOMNAS_REQUIRE(o.ldwp >= l.ht && o.ldwp % 8 == 0 && aligned16(o.wp) && (!s.expand || (o.ldwe >= p.kp && o.ldwe % 8 == 0 && aligned16(o.we))), "block_infer: packed weight pitch / alignment");
  ATOMNAS_REQUIRE(aligned16(o.d_scale) && aligned16(o.d_shift) && aligned16(o.p_scale) && aligned16(o.p_shift) && aligned16(o.e_scale) && aligned16(o.e_shift), "block_infer: coefficient vectors must be 16-byte aligned");
  if (SE) {
    ATOMNAS_REQUIRE(g.w1p && g.w2t && g.b1 && g.b2p, "block_infer_se: null squeeze-and-excitation operand");
    ATOMNAS_REQUIRE(aligned16(g.w1p) && aligned16(g.w2t) && aligned16(g.b1) && aligned16(g.b2p), "block_infer_se: the squeeze-and-excitation tensors must be 16-byte aligned");
    ATOMNAS_REQUIRE(g.ldse >= l.ht, "block_infer_se: ldse = %d is below the %d padded hidden channels", g.ldse, l.ht);
  }
  typename BiArgsOf<SE>::type a = {};
  a.x = (const bf16_t*)o.x, a.out = (bf16_t*)o.out, a.we = (const bf16_t*)o.we, a.wp = (const bf16_t*)o.wp;
  a.es = o.e_scale, a.eb = o.e_shift, a.ds = o.d_scale, a.db = o.d_shift, a.ps = o.p_scale, a.pb = o.p_shift;
  a.ldx = o.ldx, a.ldo = o.ldo, a.ldwe = o.ldwe, a.ldwp = o.ldwp;
  a.N = s.N, a.H = s.H, a.W = s.W, a.Ho = (s.H - 1) / s.stride + 1, a.Wo = (s.W - 1) / s.stride + 1, a.inp = s.inp, a.oup = s.oup, a.stride = s.stride,
  a.act = s.act, a.expand = s.expand, a.res = s.res, a.nseg = s.nseg;
  for (int i = 0; i < s.nseg; ++i) {
    ATOMNAS_REQUIRE(o.taps[i] && aligned16(o.taps[i]), "block_infer: taps of segment %d missing or not 16-byte aligned", i);
    a.seg[i] = BiSeg{o.taps[i], s.off[i], s.ch[i], s.k[i], s.ch[i]};
  }
  a.toh = p.toh, a.tow = p.tow, a.kmax = p.kmax, a.kp = p.kp, a.ch = p.ch;
  a.tiles_x = (a.Wo + p.tow - 1) / p.tow;
  const int tiles_y = (a.Ho + p.toh - 1) / p.toh;
  a.ih = l.ih, a.iw = l.iw, a.ipix = l.ipix, a.erows = l.erows, a.xr16 = l.xr16, a.tpix = l.tpix, a.tp16 = l.tp16, a.nt = l.nt;
  a.xstr = l.xstr, a.estr = l.estr, a.dstr = l.dstr;
  a.o_xs = l.o_xs, a.o_wes = l.o_wes, a.o_es = l.o_es, a.o_ds = l.o_ds, a.o_wps = l.o_wps, a.o_ts = l.o_ts, a.o_cs = l.o_cs;
  if constexpr (SE) {
    a.w1p = g.w1p, a.w2t = g.w2t, a.b1 = g.b1, a.b2p = g.b2p, a.se_hid = g.se_hid, a.ldse = g.ldse, a.ht = l.ht, a.inv_hw = 1.0f / (float)(s.H * s.W);
    a.o_pool = l.o_pool, a.o_gate = l.o_gate, a.o_hs = l.o_hs;
  }
  const dim3 grid((unsigned)(a.tiles_x * tiles_y), (unsigned)s.N);
  hipStream_t st = (hipStream_t)stream;
#define X(MT, NT) if (p.mt == MT && p.ntmax == NT) return bi_run<MT, NT, SE>(a, grid, p.lds, st);
  X(1, 2) X(1, 4) X(1, 8) X(1, 12) X(1, 20) X(2, 2) X(2, 4) X(2, 8) X(2, 12)
#undef X
  ATOMNAS_REQUIRE(false, "block_infer: no instance for %d x %d accumulator tiles", p.mt, p.ntmax);
}

}  // namespace
}  // namespace atomnas

using namespace atomnas;

// The shape arguments of an entry as BiDims, the operands as BiOperands: both in the order of the entry's own arguments
#define BI_DIMS BiDims{N, H, W, inp, oup, nseg, seg_off, seg_ch, seg_k, stride, act, expand, residual, dtype}
#define BI_OPERANDS BiOperands{x, ldx, out, ldo, we, ldwe, wp, ldwp, taps, e_scale, e_shift, d_scale, d_shift, p_scale, p_shift}

// The two predicates of atomnas_block_infer, which has no SE operands: se != 0 is outside, whatever atomnas_block_infer_se can do.
extern "C" int atomnas_block_infer_runs(int N, int H, int W, int inp, int oup, int nseg, const int* seg_off, const int* seg_ch,
                                        const int* seg_k, int stride, int act, int expand, int residual, int se, int dtype) {
  return se ? 0 : bi_answer(BI_DIMS, false, 0, false);
}

extern "C" int atomnas_block_infer_supported(int N, int H, int W, int inp, int oup, int nseg, const int* seg_off, const int* seg_ch,
                                             const int* seg_k, int stride, int act, int expand, int residual, int se, int dtype) {
  return se ? 0 : bi_answer(BI_DIMS, false, 0, true);
}

extern "C" int atomnas_block_infer_se_runs(int N, int H, int W, int inp, int oup, int nseg, const int* seg_off, const int* seg_ch,
                                           const int* seg_k, int stride, int act, int expand, int residual, int se_hid, int dtype) {
  return bi_answer(BI_DIMS, true, se_hid, false);
}

extern "C" int atomnas_block_infer_se_supported(int N, int H, int W, int inp, int oup, int nseg, const int* seg_off, const int* seg_ch,
                                                const int* seg_k, int stride, int act, int expand, int residual, int se_hid, int dtype) {
  return bi_answer(BI_DIMS, true, se_hid, true);
}

extern "C" int atomnas_block_infer(const void* x, int ldx, void* out, int ldo, const void* we, int ldwe, const void* wp, int ldwp,
                                   const float* const* taps, const float* e_scale, const float* e_shift, const float* d_scale,
                                   const float* d_shift, const float* p_scale, const float* p_shift, int N, int H, int W, int inp, int oup,
                                   int nseg, const int* seg_off, const int* seg_ch, const int* seg_k, int stride, int act, int expand,
                                   int residual, int dtype, void* stream) {
  return bi_launch<false>(BI_DIMS, BI_OPERANDS, BiGate{}, stream);
}

extern "C" int atomnas_block_infer_se(const void* x, int ldx, void* out, int ldo, const void* we, int ldwe, const void* wp, int ldwp,
                                      const float* const* taps, const float* e_scale, const float* e_shift, const float* d_scale,
                                      const float* d_shift, const float* p_scale, const float* p_shift, int N, int H, int W, int inp, int oup,
                                      int nseg, const int* seg_off, const int* seg_ch, const int* seg_k, int stride, int act, int expand,
                                      int residual, int dtype, const float* se_w1p, const float* se_w2t, const float* se_b1,
                                      const float* se_b2p, int se_hid, int ldse, void* stream) {
  return bi_launch<true>(BI_DIMS, BI_OPERANDS, BiGate{se_w1p, se_w2t, se_b1, se_b2p, se_hid, ldse}, stream);
}
