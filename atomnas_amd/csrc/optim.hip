// Optimizer tail of the training step on flat fp32 arenas: one launch replaces the ~12k tiny ATen dispatches of
//   cal_l2_loss 'mnas'        (utils/optim.py:226-243,249)   grad += wd * p on conv/fc weights and the classifier bias
//   RMSprop.step              (utils/rmsprop.py:70-132)      TF-style, eps inside the sqrt, momentum buffer, lr outside
//   ExponentialMovingAverage  (utils/optim.py:54-65)         shadow = d*shadow + (1-d)*p, d = min(decay, (1+n)/(10+n))
// plus the re-packing of the updated weights into the layouts the convolution kernels consume.
// Scalars that change every iteration (lr, EMA decay, 1/world) are read from device memory so that the launch can sit
// inside a replayed hipGraph.
#include "common.h"

namespace atomnas {

enum { HYP_LR = 0, HYP_RHO = 1, HYP_EMA_DECAY = 2, HYP_GRAD_SCALE = 3 };

// The guard vector of a guarded step (atomnas_grad_guard writes it, the *_guarded entries read it): 8 fp32 words owned by the caller.
//   GUARD_OK       1.0: apply the step; 0.0: the gradients are not finite and the step is dropped
//   GUARD_SCALE    hyper[HYP_GRAD_SCALE] * coef, one fp32 product: what the guarded optimizer kernels multiply g by
//   GUARD_NORM     sqrt(sum g^2) * hyper[HYP_GRAD_SCALE]: the L2 norm of the averaged gradient the optimizer consumes (may be Inf / NaN)
//   GUARD_COEF     min(1, max_norm / (norm + 1e-6)), torch's clip_grad_norm_ coefficient; 1 without clipping or with a non-finite norm
//   GUARD_SKIPPED  int32 bits: steps dropped so far       } cumulative: the kernel increments them and never clears them
//   GUARD_CLIPPED  int32 bits: steps with coef < 1 so far }
enum { GUARD_OK = 0, GUARD_SCALE = 1, GUARD_NORM = 2, GUARD_COEF = 3, GUARD_SKIPPED = 4, GUARD_CLIPPED = 5 };

// arithmetic order follows the reference: sq.mul_(alpha).addcmul_(1-alpha, g, g); avg = sqrt(sq+eps);
// buf.mul_(mom).addcdiv_(g, avg); p.add_(-lr, buf)
// GUARDED: the gradient scale comes from guard[GUARD_SCALE], and with guard[GUARD_OK] == 0 nothing is written to p, sq, buf or ema (the L2
// value, which only reads p, is still produced).  The plain instance never looks at `guard` and keeps its arithmetic and rounding order.
template <bool GUARDED>
__global__ __launch_bounds__(256) void k_rmsprop_ema(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ sq,
                                                     float* __restrict__ buf, float* __restrict__ ema,
                                                     const float* __restrict__ wd_chunk, long n, const float* __restrict__ hyper,
                                                     float alpha, float one_minus_alpha, float eps, int eps_inside_sqrt,
                                                     float momentum, float* __restrict__ l2_part, const float* __restrict__ guard) {
#pragma clang fp contract(off)  // keep the reference's separate roundings (no fused multiply-add)
  __shared__ float s_part[4];
  const float lr = hyper[HYP_LR], d = hyper[HYP_EMA_DECAY], gs = GUARDED ? guard[GUARD_SCALE] : hyper[HYP_GRAD_SCALE];
  const bool dropped = GUARDED && guard[GUARD_OK] == 0.f;
  const long nchunks = (n + 255) / 256;
  float l2acc = 0.f;
  for (long ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const long i = ch * 256 + threadIdx.x;
    if (i >= n) continue;
    const float wd = wd_chunk ? wd_chunk[ch] : 0.f;
    float pv = p[i];
    l2acc += (wd * pv) * pv;   // value of the L2 regulariser at the weights this step's loss saw (before the update)
    if (dropped) continue;
    float gv = g[i] * gs;
    gv = gv + wd * pv;
    float s = sq[i] * alpha;
    s = s + (one_minus_alpha * gv) * gv;
    sq[i] = s;
    const float avg = eps_inside_sqrt ? sqrtf(s + eps) : (sqrtf(s) + eps);
    if (buf) {
      float b = buf[i] * momentum;
      b = b + gv / avg;
      buf[i] = b;
      pv = pv - lr * b;
    } else {
      pv = pv - lr * (gv / avg);
    }
    p[i] = pv;
    if (ema && d >= 0.f) ema[i] = ema[i] * d + (1.0f - d) * pv;
  }
  if (l2_part) {   // per-workgroup partial, fixed order inside the workgroup; summed by k_sum_partials
    l2acc = wave_sum(l2acc);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = l2acc;
    __syncthreads();
    if (threadIdx.x == 0) l2_part[blockIdx.x] = 0.5f * (((s_part[0] + s_part[1]) + s_part[2]) + s_part[3]);
  }
}

// SGD with momentum / Nesterov on the same arenas (torch.optim.SGD with dampening 0: buf.mul_(momentum).add_(g');
// d = nesterov ? g'.add(buf, alpha=momentum) : buf; p.add_(d, alpha=-lr)), with the L2 term, the 1/world scale, the EMA and the L2 value
// exactly as in k_rmsprop_ema (same launch geometry, same summation order: the L2 value of a given arena is the same bits).
// buf starts at zero, so the first step gives momentum * 0 + g' = g', torch's first-step `buf = g'`.
template <bool GUARDED>   // as in k_rmsprop_ema
__global__ __launch_bounds__(256) void k_sgd_ema(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                 float* __restrict__ ema, const float* __restrict__ wd_chunk, long n,
                                                 const float* __restrict__ hyper, float momentum, int nesterov,
                                                 float* __restrict__ l2_part, const float* __restrict__ guard) {
#pragma clang fp contract(off)  // keep torch's separate roundings (no fused multiply-add)
  __shared__ float s_part[4];
  const float lr = hyper[HYP_LR], d = hyper[HYP_EMA_DECAY], gs = GUARDED ? guard[GUARD_SCALE] : hyper[HYP_GRAD_SCALE];
  const bool dropped = GUARDED && guard[GUARD_OK] == 0.f;
  const long nchunks = (n + 255) / 256;
  float l2acc = 0.f;
  for (long ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const long i = ch * 256 + threadIdx.x;
    if (i >= n) continue;
    const float wd = wd_chunk ? wd_chunk[ch] : 0.f;
    float pv = p[i];
    l2acc += (wd * pv) * pv;   // value of the L2 regulariser at the weights this step's loss saw (before the update)
    if (dropped) continue;
    float gv = g[i] * gs;
    gv = gv + wd * pv;
    float dv = gv;
    if (buf) {
      float b = buf[i] * momentum;
      b = b + gv;
      buf[i] = b;
      dv = nesterov ? gv + momentum * b : b;
    }
    pv = pv - lr * dv;
    p[i] = pv;
    if (ema && d >= 0.f) ema[i] = ema[i] * d + (1.0f - d) * pv;
  }
  if (l2_part) {   // per-workgroup partial, fixed order inside the workgroup; summed by k_sum_partials
    l2acc = wave_sum(l2acc);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = l2acc;
    __syncthreads();
    if (threadIdx.x == 0) l2_part[blockIdx.x] = 0.5f * (((s_part[0] + s_part[1]) + s_part[2]) + s_part[3]);
  }
}

// one workgroup: out[0] (+)= scale * sum of n values in a fixed order (thread t adds t, t+256, ...; then a fixed tree)
__global__ __launch_bounds__(256) void k_sum_partials(const float* __restrict__ ws, int n, float scale, int accumulate,
                                                      float* __restrict__ out) {
  __shared__ float s_t[256];
  float a = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) a += ws[i];
  s_t[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_t[threadIdx.x] += s_t[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (accumulate ? out[0] : 0.f) + scale * s_t[0];
}

template <bool GUARDED>   // GUARDED: a no-op when guard[GUARD_OK] == 0
__global__ __launch_bounds__(256) void k_ema(float* __restrict__ shadow, const float* __restrict__ x, long n,
                                             const float* __restrict__ hyper, const float* __restrict__ guard) {
#pragma clang fp contract(off)
  if (GUARDED && guard[GUARD_OK] == 0.f) return;
  const float d = hyper[HYP_EMA_DECAY];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) shadow[i] = shadow[i] * d + (1.0f - d) * x[i];
}

// x *= hyper[idx]  (the BN running statistics summed over the ranks -> their average: hyper[HYP_GRAD_SCALE] = 1 / world)
__global__ __launch_bounds__(256) void k_scale_by(float* __restrict__ x, long n, const float* __restrict__ hyper, int idx) {
  const float f = hyper[idx];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) x[i] *= f;
}

// Fold of one micro-batch into a running sum (gradient accumulation, engine.TrainStep with accum_steps > 1):
//   acc = (first ? 0 : acc) + cur;   then   cur = acc * inv_count (last)   or   cur = base (not last; base null: cur stays)
// One thread owns an element from the read to both writes, 16-byte pieces plus a ragged tail of up to 3 floats: no atomics, no order
// between threads to depend on.  The BN running statistics use it with base = their values at the start of the step (every
// micro-batch updates from the same start, the step leaves the mean); the gradient arena with base = null and inv_count = 1.
__global__ __launch_bounds__(256) void k_accum_fold(float* __restrict__ acc, float* __restrict__ cur, const float* __restrict__ base,
                                                    long n, int first, int last, float inv_count) {
#pragma clang fp contract(off)
  const long n4 = n >> 2;
  f32x4* __restrict__ a4 = reinterpret_cast<f32x4*>(acc);
  f32x4* __restrict__ c4 = reinterpret_cast<f32x4*>(cur);
  const f32x4* __restrict__ b4 = reinterpret_cast<const f32x4*>(base);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    f32x4 a = first ? f32x4{0.f, 0.f, 0.f, 0.f} : a4[i];
    a = a + c4[i];
    a4[i] = a;
    if (last) c4[i] = a * inv_count;
    else if (base) c4[i] = b4[i];
  }
  const long t = n4 * 4 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 3 && t < n) {
    float a = first ? 0.f : acc[t];
    a = a + cur[t];
    acc[t] = a;
    if (last) cur[t] = a * inv_count;
    else if (base) cur[t] = base[t];
  }
}

// zero-fill with 16-byte stores (n16 pieces) plus a 4-byte tail.  A kernel rather than hipMemsetAsync: as a captured memset node
// the 44 MB gradient arena was not cleared on replay (bs 256 supernet, ROCm 7.2: the replayed step trained on accumulated
// gradients), while kernel nodes replay faithfully.
__global__ __launch_bounds__(256) void k_zero(f32x4* __restrict__ p16, long n16, float* __restrict__ tail, int ntail) {
  const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long)gridDim.x * 256) p16[i] = z;
  if (blockIdx.x == 0 && (int)threadIdx.x < ntail) tail[threadIdx.x] = 0.f;
}

// ---- guarded step: global L2 norm of the gradient arena -> verdict (skip on non-finite gradients, clip_grad_norm_ coefficient)
// Stage 1, a capped grid over the 16-byte pieces of g.  One sweep of the grid covers gridDim.x * GUARD_SWEEP pieces; in a sweep a thread
// loads GUARD_UNROLL pieces 256 apart (all loads issued before the first use) and adds each piece's sum of squares
// (x0^2 + x1^2) + (x2^2 + x3^2) to an accumulator of its own, so a value passes through: its square, 2 additions inside the piece, one
// addition per sweep, 2 to join the four accumulators, [the ragged tail: 1], 6 wave levels, 3 wave partials; then stage 2.  Plain stores
// of one partial per workgroup, no atomics: the sum does not depend on arrival order and is the same bits on every run and every rank.
constexpr int GUARD_UNROLL = 4;
constexpr int GUARD_SWEEP = 256 * GUARD_UNROLL;   // 16-byte pieces per workgroup and sweep
constexpr int GUARD_MAX_BLOCKS = 1024;            // 4 workgroups per CU: 16 waves per CU with 4 KiB in flight each

__global__ __launch_bounds__(256) void k_grad_sumsq(const float* __restrict__ g, long n, float* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ float s_part[4];
  const long n4 = n >> 2;
  const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g);
  float a[GUARD_UNROLL] = {0.f, 0.f, 0.f, 0.f};
  for (long base = (long)blockIdx.x * GUARD_SWEEP + threadIdx.x; base < n4; base += (long)gridDim.x * GUARD_SWEEP) {
    f32x4 v[GUARD_UNROLL];
#pragma unroll
    for (int u = 0; u < GUARD_UNROLL; ++u) {
      const long i = base + u * 256;
      v[u] = i < n4 ? g4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < GUARD_UNROLL; ++u) a[u] = a[u] + ((v[u][0] * v[u][0] + v[u][1] * v[u][1]) + (v[u][2] * v[u][2] + v[u][3] * v[u][3]));
  }
  float acc = (a[0] + a[1]) + (a[2] + a[3]);
  const long t = n4 * 4 + threadIdx.x;   // ragged tail of up to 3 floats
  if (blockIdx.x == 0 && threadIdx.x < 3 && t < n) acc = acc + g[t] * g[t];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

// Stage 2, one workgroup: the partials in the order of k_sum_partials, then the verdict (thread 0, plain stores).
__global__ __launch_bounds__(256) void k_guard_verdict(const float* __restrict__ part, int nparts, const float* __restrict__ hyper,
                                                       float max_norm, int skip_nonfinite, float* __restrict__ guard) {
#pragma clang fp contract(off)
  __shared__ float s_t[256];
  float a = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 256) a += part[i];
  s_t[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_t[threadIdx.x] += s_t[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float sumsq = s_t[0], gs = hyper[HYP_GRAD_SCALE];
    const float norm = sqrtf(sumsq) * gs;
    const bool finite = isfinite(sumsq);   // an fp32 overflow of the sum for huge finite gradients counts as non-finite
    float coef = 1.f;
    if (max_norm > 0.f && isfinite(max_norm) && isfinite(norm)) {   // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1)
      const float c = max_norm / (norm + 1e-6f);
      coef = c < 1.f ? c : 1.f;
    }
    const bool ok = finite || !skip_nonfinite;
    guard[GUARD_OK] = ok ? 1.f : 0.f;
    guard[GUARD_SCALE] = gs * coef;
    guard[GUARD_NORM] = norm;
    guard[GUARD_COEF] = coef;
    int* cnt = reinterpret_cast<int*>(guard);
    if (!ok) cnt[GUARD_SKIPPED] = cnt[GUARD_SKIPPED] + 1;
    if (coef < 1.f) cnt[GUARD_CLIPPED] = cnt[GUARD_CLIPPED] + 1;
  }
}

// dst = src over n floats when `unconditional` or guard[GUARD_OK] == 0 (the BN running statistics: their snapshot at the start of a
// guarded step, and their way back after a dropped one).  One thread owns an element, 16-byte pieces plus a tail of up to 3 floats.
__global__ __launch_bounds__(256) void k_guard_restore(float* __restrict__ dst, const float* __restrict__ src, long n,
                                                       const float* __restrict__ guard, int unconditional) {
  if (!unconditional && guard[GUARD_OK] != 0.f) return;
  const long n4 = n >> 2;
  f32x4* __restrict__ d4 = reinterpret_cast<f32x4*>(dst);
  const f32x4* __restrict__ s4 = reinterpret_cast<const f32x4*>(src);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) d4[i] = s4[i];
  const long t = n4 * 4 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 3 && t < n) dst[t] = src[t];
}

__global__ __launch_bounds__(256) void k_add_i64(long* __restrict__ p, long n, long v) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) p[i] += v;
}

// Weight packing jobs.  src is fp32 in the parameter arena with logical shape [rows][cols] (row pitch src_ld).
//   mode 0 (PW):   dst[r*dst_ld + c_off + c] = src[r][c]            (storage T)   -> gemm_nt weight  [N][K]
//   mode 1 (PW_T): dst[(c_off + c)*dst_ld + r] = src[r][c]          (storage T)   -> gemm_nt weight of the transposed product
//   mode 2 (DW):   dst[c*dst_ld + c_off + r] = src[r][c]            (fp32)        -> depthwise taps [k*k][C]
struct PackJob {
  long src_off, dst_off;
  int rows, cols, src_ld, dst_ld, c_off, mode;
};

// A workgroup walks [PACK_TILE x PACK_TILE] tiles of its job (grid = (PACK_GRID_X, job)); a thread moves 4 consecutive elements: one
// 16-byte load of the source row where the address allows it, one store of 4 storage elements (8 bytes bf16, 16 bytes fp32) into the
// destination row, element by element at ragged edges and odd offsets.  Modes 1 and 2 turn the tile through LDS, so that both sides of
// the transpose are walked along their rows (written straight, every lane of a wave store hit another destination row).  Only elements
// of the job are written: the padding of the pack buffers is zeroed once and never touched.
constexpr int PACK_TILE = 64;
constexpr int PACK_GRID_X = 64;

template <typename D>
__device__ __forceinline__ void pack_store4(D* __restrict__ d, const float (&v)[4], int cnt) {
  if (cnt == 4 && (reinterpret_cast<uintptr_t>(d) & (4 * sizeof(D) - 1)) == 0) {
    VecIO<D, 4>::store(d, v);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) d[k] = from_f32<D>(v[k]);
  }
}

__device__ __forceinline__ void pack_load4(const float* __restrict__ s, float (&v)[4], int cnt) {
  if (cnt == 4 && (reinterpret_cast<uintptr_t>(s) & 15) == 0) {
    VecIO<float, 4>::load(s, v);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = k < cnt ? s[k] : 0.f;
  }
}

// transposed store of one tile out of LDS: destination row c (tile column), 4 consecutive source rows r per thread
template <typename D>
__device__ __forceinline__ void pack_store_t(D* __restrict__ dst, long dst_ld, const float (*tile)[PACK_TILE + 1], int r0, int c0, int rows,
                                             int cols) {
  const int rq = (threadIdx.x & 15) * 4;
#pragma unroll
  for (int pass = 0; pass < PACK_TILE / 16; ++pass) {
    const int cl = pass * 16 + (threadIdx.x >> 4);
    const int cnt = min(4, rows - (r0 + rq));
    if (c0 + cl < cols && cnt > 0) {
      const float v[4] = {tile[rq][cl], tile[rq + 1][cl], tile[rq + 2][cl], tile[rq + 3][cl]};
      pack_store4<D>(dst + (long)(c0 + cl) * dst_ld + r0 + rq, v, cnt);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_pack(const float* __restrict__ arena, void* __restrict__ packbuf, const PackJob* __restrict__ jobs) {
  __shared__ float tile[PACK_TILE][PACK_TILE + 1];
  const PackJob jb = jobs[blockIdx.y];
  const float* __restrict__ src = arena + jb.src_off;
  const int tc = (jb.cols + PACK_TILE - 1) / PACK_TILE;
  const int ntiles = ((jb.rows + PACK_TILE - 1) / PACK_TILE) * tc;
  const int cq = (threadIdx.x & 15) * 4, rl = threadIdx.x >> 4;   // a pass covers 16 rows x 64 columns
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int r0 = (t / tc) * PACK_TILE, c0 = (t % tc) * PACK_TILE;
    const int cnt = min(4, jb.cols - (c0 + cq));
    if (jb.mode == 0) {
      T* __restrict__ dst = reinterpret_cast<T*>(packbuf) + jb.dst_off + jb.c_off;
#pragma unroll
      for (int pass = 0; pass < PACK_TILE / 16; ++pass) {
        const int r = r0 + pass * 16 + rl;
        if (r < jb.rows && cnt > 0) {
          float v[4];
          pack_load4(src + (long)r * jb.src_ld + c0 + cq, v, cnt);
          pack_store4<T>(dst + (long)r * jb.dst_ld + c0 + cq, v, cnt);
        }
      }
      continue;
    }
    __syncthreads();   // the previous tile has been read out
#pragma unroll
    for (int pass = 0; pass < PACK_TILE / 16; ++pass) {
      const int rt = pass * 16 + rl;
      if (r0 + rt < jb.rows && cnt > 0) {
        float v[4];
        pack_load4(src + (long)(r0 + rt) * jb.src_ld + c0 + cq, v, cnt);
#pragma unroll
        for (int k = 0; k < 4; ++k) tile[rt][cq + k] = v[k];
      }
    }
    __syncthreads();
    if (jb.mode == 1)
      pack_store_t<T>(reinterpret_cast<T*>(packbuf) + jb.dst_off + (long)jb.c_off * jb.dst_ld, jb.dst_ld, tile, r0, c0, jb.rows, jb.cols);
    else
      pack_store_t<float>(reinterpret_cast<float*>(packbuf) + jb.dst_off + jb.c_off, jb.dst_ld, tile, r0, c0, jb.rows, jb.cols);
  }
}

}  // namespace atomnas

using namespace atomnas;

// the two forms of each fused optimizer entry share their checks and launch geometry; `guard` selects the kernel instance
static int launch_rmsprop(const char* what, float* p, const float* g, float* sq, float* buf, float* ema, const float* wd_chunk, long n,
                          const float* hyper, double alpha, double eps, int eps_inside_sqrt, double momentum, float* l2_value, float* ws,
                          const float* guard, void* stream) {
  ATOMNAS_REQUIRE(p && g && sq && hyper && n > 0, "%s: bad arguments", what);
  ATOMNAS_REQUIRE(!l2_value || (ws && wd_chunk), "%s: the L2 value needs wd_chunk and a 4096-float workspace", what);
  ATOMNAS_REQUIRE(momentum >= 0.0 && alpha >= 0.0 && eps >= 0.0, "%s: bad hyper-parameters", what);
  ATOMNAS_REQUIRE((momentum > 0.0) == (buf != nullptr), "%s: momentum buffer must be given iff momentum > 0", what);
  long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(guard ? k_rmsprop_ema<true> : k_rmsprop_ema<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, sq,
                     buf, ema, wd_chunk, n, hyper, (float)alpha, (float)(1.0 - alpha), (float)eps, eps_inside_sqrt, (float)momentum,
                     l2_value ? ws : nullptr, guard);
  if (l2_value)
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, (hipStream_t)stream, ws, (int)blocks, 1.f, 0, l2_value);
  return check_launch(what);
}

extern "C" int atomnas_fused_rmsprop_ema(float* p, const float* g, float* sq, float* buf, float* ema, const float* wd_chunk, long n,
                                         const float* hyper, double alpha, double eps, int eps_inside_sqrt, double momentum,
                                         float* l2_value, float* ws, void* stream) {
  return launch_rmsprop("fused_rmsprop_ema", p, g, sq, buf, ema, wd_chunk, n, hyper, alpha, eps, eps_inside_sqrt, momentum, l2_value, ws,
                        nullptr, stream);
}

extern "C" int atomnas_fused_rmsprop_ema_guarded(float* p, const float* g, float* sq, float* buf, float* ema, const float* wd_chunk, long n,
                                                 const float* hyper, double alpha, double eps, int eps_inside_sqrt, double momentum,
                                                 float* l2_value, float* ws, const float* guard, void* stream) {
  ATOMNAS_REQUIRE(guard, "fused_rmsprop_ema_guarded: needs the guard vector");
  return launch_rmsprop("fused_rmsprop_ema_guarded", p, g, sq, buf, ema, wd_chunk, n, hyper, alpha, eps, eps_inside_sqrt, momentum, l2_value,
                        ws, guard, stream);
}

static int launch_sgd(const char* what, float* p, const float* g, float* buf, float* ema, const float* wd_chunk, long n, const float* hyper,
                      double momentum, int nesterov, float* l2_value, float* ws, const float* guard, void* stream) {
  ATOMNAS_REQUIRE(p && g && hyper && n > 0, "%s: bad arguments", what);
  ATOMNAS_REQUIRE(!l2_value || (ws && wd_chunk), "%s: the L2 value needs wd_chunk and a 4096-float workspace", what);
  ATOMNAS_REQUIRE(momentum >= 0.0, "%s: bad hyper-parameters", what);
  ATOMNAS_REQUIRE((momentum > 0.0) == (buf != nullptr), "%s: momentum buffer must be given iff momentum > 0", what);
  ATOMNAS_REQUIRE(!nesterov || momentum > 0.0, "%s: Nesterov momentum needs momentum > 0", what);
  long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(guard ? k_sgd_ema<true> : k_sgd_ema<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, buf, ema,
                     wd_chunk, n, hyper, (float)momentum, nesterov, l2_value ? ws : nullptr, guard);
  if (l2_value)
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, (hipStream_t)stream, ws, (int)blocks, 1.f, 0, l2_value);
  return check_launch(what);
}

extern "C" int atomnas_fused_sgd_ema(float* p, const float* g, float* buf, float* ema, const float* wd_chunk, long n, const float* hyper,
                                     double momentum, int nesterov, float* l2_value, float* ws, void* stream) {
  return launch_sgd("fused_sgd_ema", p, g, buf, ema, wd_chunk, n, hyper, momentum, nesterov, l2_value, ws, nullptr, stream);
}

extern "C" int atomnas_fused_sgd_ema_guarded(float* p, const float* g, float* buf, float* ema, const float* wd_chunk, long n,
                                             const float* hyper, double momentum, int nesterov, float* l2_value, float* ws,
                                             const float* guard, void* stream) {
  ATOMNAS_REQUIRE(guard, "fused_sgd_ema_guarded: needs the guard vector");
  return launch_sgd("fused_sgd_ema_guarded", p, g, buf, ema, wd_chunk, n, hyper, momentum, nesterov, l2_value, ws, guard, stream);
}

// Verdict of a guarded step from the n floats of g (16-byte aligned): guard[] as laid out next to the HYP_* enum.  ws: caller-owned
// scratch of atomnas_grad_guard_ws_floats() floats.  Two launches, capturable, no atomics: bit-reproducible.
extern "C" int atomnas_grad_guard_ws_floats() { return GUARD_MAX_BLOCKS; }

extern "C" int atomnas_grad_guard(const float* g, long n, const float* hyper, float max_norm, int skip_nonfinite, float* ws, float* guard,
                                  void* stream) {
  ATOMNAS_REQUIRE(g && hyper && ws && guard && n > 0, "grad_guard: bad arguments");
  ATOMNAS_REQUIRE(((unsigned long long)g & 15ull) == 0, "grad_guard: needs a 16-byte aligned gradient arena");
  ATOMNAS_REQUIRE(!(max_norm != max_norm), "grad_guard: max_norm is NaN");
  long blocks = (n / 4 + GUARD_SWEEP - 1) / GUARD_SWEEP;
  if (blocks > GUARD_MAX_BLOCKS) blocks = GUARD_MAX_BLOCKS;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_grad_sumsq, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g, n, ws);
  hipLaunchKernelGGL(k_guard_verdict, dim3(1), dim3(256), 0, (hipStream_t)stream, ws, (int)blocks, hyper, max_norm, skip_nonfinite, guard);
  return check_launch("grad_guard");
}

extern "C" int atomnas_guard_restore(float* dst, const float* src, long n, const float* guard, int unconditional, void* stream) {
  ATOMNAS_REQUIRE(dst && src && n > 0 && (guard || unconditional), "guard_restore: bad arguments");
  ATOMNAS_REQUIRE((((unsigned long long)dst | (unsigned long long)src) & 15ull) == 0, "guard_restore: needs 16-byte aligned pointers");
  long blocks = (n / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_guard_restore, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dst, src, n, guard, unconditional);
  return check_launch("guard_restore");
}

// out[0] = scale * sum_i x[i] in a fixed order (mean of the per-sample losses, train.py:178-180 `loss = torch.mean(loss)`)
extern "C" int atomnas_vec_sum(const float* x, int n, float scale, float* out, void* stream) {
  ATOMNAS_REQUIRE(x && out && n > 0, "vec_sum: bad arguments");
  hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, (hipStream_t)stream, x, n, scale, 0, out);
  return check_launch("vec_sum");
}

extern "C" int atomnas_ema_update(float* shadow, const float* x, long n, const float* hyper, void* stream) {
  ATOMNAS_REQUIRE(shadow && x && hyper && n > 0, "ema_update: bad arguments");
  long blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_ema<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, shadow, x, n, hyper, (const float*)nullptr);
  return check_launch("ema_update");
}

extern "C" int atomnas_ema_update_guarded(float* shadow, const float* x, long n, const float* hyper, const float* guard, void* stream) {
  ATOMNAS_REQUIRE(shadow && x && hyper && guard && n > 0, "ema_update_guarded: bad arguments");
  long blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_ema<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, shadow, x, n, hyper, guard);
  return check_launch("ema_update_guarded");
}

extern "C" int atomnas_scale_by(float* x, long n, const float* hyper, int idx, void* stream) {
  ATOMNAS_REQUIRE(x && hyper && n > 0 && idx >= 0 && idx < 4, "scale_by: bad arguments");
  long blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_scale_by, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, n, hyper, idx);
  return check_launch("scale_by");
}

// acc = (first ? 0 : acc) + cur over n floats, then cur = acc * inv_count (last) or cur = base (not last; base may be null: cur is left
// as it is).  acc, cur and base are 16-byte aligned and do not overlap.  One launch, capturable.
extern "C" int atomnas_accum_fold(float* acc, float* cur, const float* base, long n, int first, int last, float inv_count, void* stream) {
  ATOMNAS_REQUIRE(acc && cur && n > 0, "accum_fold: bad arguments");
  ATOMNAS_REQUIRE((((unsigned long long)acc | (unsigned long long)cur | (unsigned long long)base) & 15ull) == 0,
                  "accum_fold: needs 16-byte aligned pointers");
  long blocks = (n / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_accum_fold, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, acc, cur, base, n, first, last, inv_count);
  return check_launch("accum_fold");
}

// p[0 .. bytes) = 0 (gradient arena, per-step scalars, accumulated outputs); p 16-byte aligned, bytes a multiple of 4
extern "C" int atomnas_zero(void* p, long bytes, void* stream) {
  ATOMNAS_REQUIRE(p && bytes > 0 && bytes % 4 == 0 && ((unsigned long long)p & 15ull) == 0, "zero: needs a 16-byte aligned pointer and whole words");
  const long n16 = bytes / 16;
  const int ntail = (int)((bytes % 16) / 4);
  long blocks = (n16 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_zero, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (f32x4*)p, n16, (float*)p + n16 * 4, ntail);
  return check_launch("zero");
}

// p[i] += v for the int64 counters (num_batches_tracked of every BatchNorm, models/mobilenet_base.py:142; the dropout step counter)
extern "C" int atomnas_add_i64(long* p, long n, long v, void* stream) {
  ATOMNAS_REQUIRE(p && n > 0, "add_i64: bad arguments");
  long blocks = (n + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(k_add_i64, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, n, v);
  return check_launch("add_i64");
}

extern "C" int atomnas_pack_weights(const float* arena, void* packbuf, const void* jobs_dev, int njobs, int dtype, void* stream) {
  ATOMNAS_REQUIRE(arena && packbuf && jobs_dev && njobs > 0, "pack_weights: bad arguments");
  dim3 grid(PACK_GRID_X, njobs);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DT_F32) hipLaunchKernelGGL(k_pack<float>, grid, dim3(256), 0, st, arena, packbuf, (const PackJob*)jobs_dev);
  else hipLaunchKernelGGL(k_pack<bf16_t>, grid, dim3(256), 0, st, arena, packbuf, (const PackJob*)jobs_dev);
  return check_launch("pack_weights");
}

// ---- regularisers as gradient contributions (so that p.grad after backward() is what the reference's autograd leaves
// there): cal_l2_loss (utils/optim.py:210-249) contributes wd*p, cal_bn_l1_loss (utils/prune.py:161-167) contributes
// rho*penalty*sign(gamma).  One launch over a job table instead of ~2.2k ATen dispatches forward and ~3.3k backward.
namespace atomnas {
struct RegJob {
  long off;
  int count;
  float coef;
};

__global__ __launch_bounds__(256) void k_reg_grad(const float* __restrict__ p, float* __restrict__ g, const RegJob* __restrict__ jobs,
                                                  int use_sign, const float* __restrict__ mult_ptr, const float* __restrict__ go_ptr) {
  const RegJob jb = jobs[blockIdx.y];
  float m = jb.coef;
  if (mult_ptr) m *= mult_ptr[0];
  if (go_ptr) m *= go_ptr[0];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < jb.count; i += gridDim.x * 256) {
    const float v = p[jb.off + i];
    const float d = use_sign ? ((v > 0.f) ? 1.f : ((v < 0.f) ? -1.f : 0.f)) : v;
    g[jb.off + i] += m * d;
  }
}

// stage 1: ws[job * 64 + block] = coef * post_scale * mult * (block's share of the job's sum), fixed order inside the block
__global__ __launch_bounds__(256) void k_reg_value(const float* __restrict__ p, const RegJob* __restrict__ jobs, int use_abs,
                                                   const float* __restrict__ mult_ptr, float post_scale, float* __restrict__ ws) {
  __shared__ float s_part[4];
  const RegJob jb = jobs[blockIdx.y];
  float acc = 0.f;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < jb.count; i += gridDim.x * 256) {
    const float v = p[jb.off + i];
    acc += use_abs ? fabsf(v) : v * v;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = jb.coef * post_scale;
    if (mult_ptr) m *= mult_ptr[0];
    ws[blockIdx.y * gridDim.x + blockIdx.x] = m * (((s_part[0] + s_part[1]) + s_part[2]) + s_part[3]);
  }
}

}  // namespace atomnas

// g[off+i] += coef * mult * go * (use_sign ? sign(p) : p) for every job {long off; int count; float coef;}
extern "C" int atomnas_reg_grad(const float* p, float* g, const void* jobs_dev, int njobs, int use_sign, const float* mult_ptr,
                                const float* grad_out_ptr, void* stream) {
  ATOMNAS_REQUIRE(p && g && jobs_dev && njobs > 0, "reg_grad: bad arguments");
  hipLaunchKernelGGL(atomnas::k_reg_grad, dim3(64, njobs), dim3(256), 0, (hipStream_t)stream, p, g, (const atomnas::RegJob*)jobs_dev,
                     use_sign, mult_ptr, grad_out_ptr);
  return atomnas::check_launch("reg_grad");
}

// out += post_scale * mult * sum_jobs coef * sum_i (use_abs ? |p_i| : p_i^2);  ws: caller-owned scratch of 64 * njobs floats
// (per-workgroup partials, summed in a fixed order: the logged regulariser values are bit-reproducible)
extern "C" int atomnas_reg_value(const float* p, const void* jobs_dev, int njobs, int use_abs, const float* mult_ptr,
                                 float post_scale, float* out, float* ws, void* stream) {
  ATOMNAS_REQUIRE(p && out && ws && jobs_dev && njobs > 0, "reg_value: bad arguments");
  hipLaunchKernelGGL(atomnas::k_reg_value, dim3(64, njobs), dim3(256), 0, (hipStream_t)stream, p, (const atomnas::RegJob*)jobs_dev,
                     use_abs, mult_ptr, post_scale, ws);
  hipLaunchKernelGGL(atomnas::k_sum_partials, dim3(1), dim3(256), 0, (hipStream_t)stream, ws, 64 * njobs, 1.f, 1, out);
  return atomnas::check_launch("reg_value");
}
