// Sequence loss and flow metrics, forward and backward (include/dexiraft_loss.h;
// reference train.py:48-73): the masked L1 term of each of P predictions, their
// gamma-weighted sum, and the end-point-error statistics of the last one.
//
// Mapping (all kernels).  Pixels are numbered flat over [B, H, W]; a thread owns
// groups of 4 consecutive pixels, lanes run along the groups, so a wave's loads
// of one plane are 1 KiB contiguous.  A pixel n of item b sits at element
// n + b*H*W of channel x of a [B, 2, H, W] tensor (channel y: + H*W) and at
// element n of `valid`.  With `vec` (H*W a multiple of 4, every pointer 16-byte
// aligned) a group is one 16-byte access per plane; otherwise four 4-byte ones
// of the same pixels, so both paths add the same numbers in the same order.
//
// Forward, first launch: a thread keeps flow_gt and v of its 2 groups in
// registers and walks the predictions; each prediction's 16 summands are added
// in the thread, then over the wave (a shuffle tree) at once, so there is one
// accumulator and not P of them, and flow_gt / valid are read once.  The waves'
// sums meet in LDS and are added in float64, wave ascending, into one partial
// per workgroup and term.  Second launch: one workgroup adds the partials,
// workgroup ascending, in float64.  Counts are integers throughout.
//
// Backward: one launch, 1 group per thread; v and sgn(d_i) are recomputed.
#include "dexiraft_loss.h"
#include "dxr_common.h"

#include <cmath>

namespace {

constexpr int SL_MAX_P = 32;
constexpr int SL_THREADS = 256;
constexpr int SL_WAVES = SL_THREADS / 64;
constexpr int SL_GROUPS = 2;                                   // forward: 4-pixel groups per thread
constexpr int64_t SL_WG_PIXELS = 4LL * SL_GROUPS * SL_THREADS;  // forward: pixels per workgroup
constexpr int64_t SL_MAX_PIXELS = 1LL << 31;
constexpr int SL_COUNTS = 5;                                   // count(v), epe < 1, < 3, < 5, outliers
constexpr int FIN_THREADS = 1024;                              // the final kernel's one workgroup
constexpr int FIN_DOUBLES = 7936;                              // partials it stages in LDS at a time (62 KiB)

struct Preds { const float* p[SL_MAX_P]; };
struct Weights { double w[SL_MAX_P]; };
struct BackwardArgs {
  const float* pred[SL_MAX_P];
  float* grad[SL_MAX_P];
  float c[SL_MAX_P];
};

// The 4 pixels n0 .. n0 + 3 of a thread: `left` of them exist (0 .. 4); off[j] is
// the element of channel x in a [B, 2, H, W] tensor, n0 + j the element of `valid`.
struct Group {
  int64_t n0;
  int64_t off[4];
  int left;
};

__device__ __forceinline__ Group make_group(int64_t grp, int64_t npix, int64_t hw) {
  Group g;
  g.n0 = 4 * grp;
  const int64_t rem = npix - g.n0;
  g.left = rem <= 0 ? 0 : rem >= 4 ? 4 : (int)rem;
  // n0 < npix <= 2^31 and hw <= 2^31: the division fits 32 bits
  uint32_t b = g.left ? (uint32_t)g.n0 / (uint32_t)hw : 0u;
  int64_t p = g.left ? g.n0 - (int64_t)b * hw : 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    g.off[j] = g.left ? g.n0 + j + (int64_t)b * hw : 0;
    if (++p == hw) {
      p = 0;
      ++b;
    }
  }
  return g;
}

// plane[first + 0..3]; pixels that do not exist read as 0.
__device__ __forceinline__ void load4(const float* __restrict__ plane, int64_t first,
                                      const int64_t (&off)[4], int left, bool vec, float (&v)[4]) {
  if (vec) {
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (left) a = *reinterpret_cast<const float4*>(plane + first);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < left ? plane[off[j]] : 0.0f;
  }
}

__device__ __forceinline__ void store4(float* __restrict__ plane, const int64_t (&off)[4], int left,
                                       bool vec, const float (&v)[4]) {
  if (vec) {
    if (left) *reinterpret_cast<float4*>(plane + off[0]) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < left) plane[off[j]] = v[j];
  }
}

// flow_gt and v (1.0 / 0.0) of a group.
__device__ __forceinline__ void load_target(const Group& g, const float* __restrict__ gt,
                                            const float* __restrict__ valid, int64_t hw,
                                            float max_flow, bool vec, float (&gx)[4], float (&gy)[4],
                                            float (&mag)[4], float (&vf)[4]) {
#pragma clang fp contract(off)
  const int64_t flat[4] = {g.n0, g.n0 + 1, g.n0 + 2, g.n0 + 3};
  float va[4] = {1.0f, 1.0f, 1.0f, 1.0f};
  load4(gt, g.off[0], g.off, g.left, vec, gx);
  load4(gt + hw, g.off[0], g.off, g.left, vec, gy);
  if (valid) load4(valid, g.n0, flat, g.left, vec, va);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    mag[j] = sqrtf(gx[j] * gx[j] + gy[j] * gy[j]);
    vf[j] = (j < g.left && va[j] >= 0.5f && mag[j] < max_flow) ? 1.0f : 0.0f;
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma clang fp contract(off)
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_down(v, s, 64);
  return v;   // lane 0
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += (uint32_t)__shfl_down((int)v, s, 64);
  return v;   // lane 0
}

// The forward's SL_GROUPS groups of one prediction.
__device__ __forceinline__ void load_pred(const float* __restrict__ pr, const Group (&g)[SL_GROUPS],
                                          int64_t hw, bool vec, float (&x)[SL_GROUPS][4],
                                          float (&y)[SL_GROUPS][4]) {
#pragma unroll
  for (int k = 0; k < SL_GROUPS; ++k) {
    load4(pr, g[k].off[0], g[k].off, g[k].left, vec, x[k]);
    load4(pr + hw, g[k].off[0], g[k].off, g[k].left, vec, y[k]);
  }
}

// sum v * |d| over a thread's pixels: group, pixel, channel ascending.
__device__ __forceinline__ float thread_term(const float (&x)[SL_GROUPS][4],
                                             const float (&y)[SL_GROUPS][4],
                                             const float (&gx)[SL_GROUPS][4],
                                             const float (&gy)[SL_GROUPS][4],
                                             const float (&vf)[SL_GROUPS][4]) {
#pragma clang fp contract(off)
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < SL_GROUPS; ++k) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s = s + vf[k][j] * fabsf(x[k][j] - gx[k][j]);
      s = s + vf[k][j] * fabsf(y[k][j] - gy[k][j]);
    }
  }
  return s;
}

// Workspace: double sums[P + 1][nwg] (the terms, then sum_v epe), then
// uint32 counts[SL_COUNTS][nwg].
__global__ __launch_bounds__(SL_THREADS) void sequence_loss_partial_kernel(
    Preds preds, int P, const float* __restrict__ gt, const float* __restrict__ valid, int64_t npix,
    int64_t hw, float max_flow, double* __restrict__ sums, uint32_t* __restrict__ counts, bool vec) {
#pragma clang fp contract(off)
  __shared__ float red[SL_MAX_P + 1][SL_WAVES];
  __shared__ uint32_t redc[SL_COUNTS][SL_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  Group g[SL_GROUPS];
  float gx[SL_GROUPS][4], gy[SL_GROUPS][4], mag[SL_GROUPS][4], vf[SL_GROUPS][4];
#pragma unroll
  for (int k = 0; k < SL_GROUPS; ++k) {
    g[k] = make_group(((int64_t)blockIdx.x * SL_GROUPS + k) * SL_THREADS + tid, npix, hw);
    load_target(g[k], gt, valid, hw, max_flow, vec, gx[k], gy[k], mag[k], vf[k]);
  }
  // two predictions at a time: eight 16-byte loads of a thread in flight
  int i = 0;
  for (; i + 1 < P - 1; i += 2) {
    float xa[SL_GROUPS][4], ya[SL_GROUPS][4], xb[SL_GROUPS][4], yb[SL_GROUPS][4];
    load_pred(preds.p[i], g, hw, vec, xa, ya);
    load_pred(preds.p[i + 1], g, hw, vec, xb, yb);
    const float sa = wave_sum(thread_term(xa, ya, gx, gy, vf));
    const float sb = wave_sum(thread_term(xb, yb, gx, gy, vf));
    if (lane == 0) {
      red[i][wave] = sa;
      red[i + 1][wave] = sb;
    }
  }
  if (i < P - 1) {
    float x[SL_GROUPS][4], y[SL_GROUPS][4];
    load_pred(preds.p[i], g, hw, vec, x, y);
    const float s = wave_sum(thread_term(x, y, gx, gy, vf));
    if (lane == 0) red[i][wave] = s;
  }
  {   // the last prediction: its term and the statistics
    const float* __restrict__ pr = preds.p[P - 1];
    float s = 0.0f, se = 0.0f;
    uint32_t c[SL_COUNTS] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < SL_GROUPS; ++k) {
      float x[4], y[4];
      load4(pr, g[k].off[0], g[k].off, g[k].left, vec, x);
      load4(pr + hw, g[k].off[0], g[k].off, g[k].left, vec, y);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float dx = x[j] - gx[k][j], dy = y[j] - gy[k][j];
        s = s + vf[k][j] * fabsf(dx);
        s = s + vf[k][j] * fabsf(dy);
        const float epe = sqrtf(dx * dx + dy * dy);
        const bool v = vf[k][j] != 0.0f;
        se = se + (v ? epe : 0.0f);
        c[0] += v;
        c[1] += v && epe < 1.0f;
        c[2] += v && epe < 3.0f;
        c[3] += v && epe < 5.0f;
        c[4] += v && epe > 3.0f && epe / mag[k][j] > 0.05f;
      }
    }
    s = wave_sum(s);
    se = wave_sum(se);
#pragma unroll
    for (int q = 0; q < SL_COUNTS; ++q) c[q] = wave_sum(c[q]);
    if (lane == 0) {
      red[P - 1][wave] = s;
      red[P][wave] = se;
#pragma unroll
      for (int q = 0; q < SL_COUNTS; ++q) redc[q][wave] = c[q];
    }
  }
  __syncthreads();
  const int64_t nwg = gridDim.x;
  if (tid <= P) {
    double d = 0.0;
#pragma unroll
    for (int w = 0; w < SL_WAVES; ++w) d = d + (double)red[tid][w];
    sums[tid * nwg + blockIdx.x] = d;
  } else if (tid >= 64 && tid < 64 + SL_COUNTS) {
    const int q = tid - 64;
    uint32_t n = 0;
#pragma unroll
    for (int w = 0; w < SL_WAVES; ++w) n += redc[q][w];
    counts[q * nwg + blockIdx.x] = n;
  }
}

// One workgroup.  A dependent chain of loads from the workspace would pay a memory
// latency per partial, so all threads stage a chunk of partials in LDS with
// independent coalesced loads, and thread q then adds row q, workgroup ascending.
// The row stride is 1 mod 32 doubles: the P + 1 adding threads hit distinct banks.
// The counts are integers, so any order is exact: one wave per count, lanes strided.
__global__ __launch_bounds__(FIN_THREADS) void sequence_loss_final_kernel(
    Weights weights, int P, const double* __restrict__ sums, const uint32_t* __restrict__ counts,
    int64_t nwg, double M, float* __restrict__ loss, float* __restrict__ terms,
    double* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ double stage[FIN_DOUBLES];
  __shared__ double tot[SL_MAX_P + 1 + SL_COUNTS];
  const int t = threadIdx.x, rows = P + 1;
  const int stride = (FIN_DOUBLES / rows - 1) / 32 * 32 + 1;
  double d = 0.0;
  for (int64_t w0 = 0; w0 < nwg; w0 += stride) {
    const int cw = nwg - w0 < stride ? (int)(nwg - w0) : stride;
#pragma unroll 8
    for (int e = t; e < rows * cw; e += FIN_THREADS) {
      const int q = e / cw, w = e - q * cw;
      stage[q * stride + w] = sums[q * nwg + w0 + w];
    }
    __syncthreads();
    if (t < rows) {
      const double* row = stage + t * stride;
#pragma unroll 16
      for (int w = 0; w < cw; ++w) d = d + row[w];
    }
    __syncthreads();
  }
  if (t < rows) tot[t] = d;
  const int q = (t >> 6) - 1;   // waves 1 .. SL_COUNTS
  if (q >= 0 && q < SL_COUNTS) {
    uint32_t n = 0;             // at most 2^31 in all
    for (int64_t w = t & 63; w < nwg; w += 64) n += counts[q * nwg + w];
    n = wave_sum(n);
    if ((t & 63) == 0) tot[P + 1 + q] = (double)n;
  }
  __syncthreads();
  if (t == 0) {
    double l = 0.0;
    for (int i = 0; i < P; ++i) {
      const double term = tot[i] / M;
      if (terms) terms[i] = (float)term;
      l = l + weights.w[i] * term;
    }
    if (loss) *loss = (float)l;
  } else if (t == 1 && stats) {
    stats[0] = tot[P + 1];
    stats[1] = tot[P];
#pragma unroll
    for (int q = 1; q < SL_COUNTS; ++q) stats[1 + q] = tot[P + 1 + q];
  }
}

__global__ __launch_bounds__(SL_THREADS) void sequence_loss_backward_kernel(
    BackwardArgs a, int n, const float* __restrict__ grad_loss, const float* __restrict__ gt,
    const float* __restrict__ valid, int64_t npix, int64_t hw, float max_flow, bool vec) {
#pragma clang fp contract(off)
  const Group g = make_group((int64_t)blockIdx.x * SL_THREADS + threadIdx.x, npix, hw);
  if (!g.left) return;
  float gx[4], gy[4], mag[4], vf[4];
  load_target(g, gt, valid, hw, max_flow, vec, gx, gy, mag, vf);
  const float gl = *grad_loss;
#pragma unroll 2
  for (int k = 0; k < n; ++k) {
    const float* __restrict__ pr = a.pred[k];
    float* __restrict__ out = a.grad[k];
    const float q = a.c[k] * gl;
    float x[4], y[4];
    load4(pr, g.off[0], g.off, g.left, vec, x);
    load4(pr + hw, g.off[0], g.off, g.left, vec, y);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float dx = x[j] - gx[j], dy = y[j] - gy[j];
      const bool v = vf[j] != 0.0f;
      x[j] = (v && dx > 0.0f) ? q : (v && dx < 0.0f) ? -q : 0.0f;
      y[j] = (v && dy > 0.0f) ? q : (v && dy < 0.0f) ? -q : 0.0f;
    }
    store4(out, g.off, g.left, vec, x);
    store4(out + hw, g.off, g.left, vec, y);
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// DXR_OK with *npix = B*H*W, or DXR_EINVAL.
inline int geometry(int64_t P, int64_t B, int64_t H, int64_t W, int64_t* npix) {
  if (P < 1 || P > SL_MAX_P) return DXR_EINVAL;
  if (B < 0 || H < 1 || W < 1) return DXR_EINVAL;
  if (B > SL_MAX_PIXELS || H > SL_MAX_PIXELS || W > SL_MAX_PIXELS) return DXR_EINVAL;
  if (H * W > SL_MAX_PIXELS) return DXR_EINVAL;
  if (B * (H * W) > SL_MAX_PIXELS) return DXR_EINVAL;
  *npix = B * H * W;
  return DXR_OK;
}

inline int64_t workgroups(int64_t npix) { return (npix + SL_WG_PIXELS - 1) / SL_WG_PIXELS; }

inline bool scalars_ok(double gamma, float max_flow) {
  return !std::isnan(gamma) && gamma >= 0.0 && !std::isnan(max_flow);
}

}  // namespace

extern "C" int dxl_abi_version(void) { return DXL_ABI_VERSION; }

extern "C" int64_t dxl_sequence_loss_workspace_bytes(int64_t P, int64_t B, int64_t H, int64_t W) {
  int64_t npix;
  if (geometry(P, B, H, W, &npix) != DXR_OK) return -1;
  const int64_t nwg = workgroups(npix);
  return (nwg * ((P + 1) * 8 + SL_COUNTS * 4) + 15) / 16 * 16;
}

extern "C" int dxl_sequence_loss(const float* const* preds, int64_t P, const float* flow_gt,
                                 const float* valid, int64_t B, int64_t H, int64_t W, double gamma,
                                 float max_flow, float* loss, float* terms, double* stats,
                                 void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  int64_t npix;
  if (geometry(P, B, H, W, &npix) != DXR_OK) return DXR_EINVAL;
  if (B == 0) return DXR_OK;
  if (!scalars_ok(gamma, max_flow)) return DXR_EINVAL;
  if (!preds || !flow_gt) return DXR_EINVAL;
  if (!loss && !terms && !stats) return DXR_EINVAL;
  if (!workspace || !aligned16(workspace)) return DXR_EINVAL;
  if (workspace_bytes < dxl_sequence_loss_workspace_bytes(P, B, H, W)) return DXR_EINVAL;
  const int64_t hw = H * W;
  Preds pa = {};
  Weights wa = {};
  bool vec = hw % 4 == 0 && aligned16(flow_gt) && aligned16(valid);
  for (int64_t i = 0; i < P; ++i) {
    if (!preds[i]) return DXR_EINVAL;
    pa.p[i] = preds[i];
    wa.w[i] = std::pow(gamma, (double)(P - 1 - i));
    vec = vec && aligned16(preds[i]);
  }
  const int64_t nwg = workgroups(npix);
  double* sums = static_cast<double*>(workspace);
  uint32_t* counts = reinterpret_cast<uint32_t*>(sums + (P + 1) * nwg);
  sequence_loss_partial_kernel<<<dim3((unsigned)nwg), dim3(SL_THREADS), 0, stream>>>(
      pa, (int)P, flow_gt, valid, npix, hw, max_flow, sums, counts, vec);
  const int st = dxr::launch_status();
  if (st != DXR_OK) return st;
  sequence_loss_final_kernel<<<dim3(1), dim3(FIN_THREADS), 0, stream>>>(
      wa, (int)P, sums, counts, nwg, 2.0 * (double)npix, loss, terms, stats);
  return dxr::launch_status();
}

extern "C" int dxl_sequence_loss_backward(const float* grad_loss, const float* const* preds,
                                          float* const* grad_preds, int64_t P,
                                          const float* flow_gt, const float* valid, int64_t B,
                                          int64_t H, int64_t W, double gamma, float max_flow,
                                          hipStream_t stream) {
  int64_t npix;
  if (geometry(P, B, H, W, &npix) != DXR_OK) return DXR_EINVAL;
  if (B == 0) return DXR_OK;
  if (!scalars_ok(gamma, max_flow)) return DXR_EINVAL;
  if (!grad_loss || !preds || !grad_preds || !flow_gt) return DXR_EINVAL;
  const int64_t hw = H * W;
  const double M = 2.0 * (double)npix;
  BackwardArgs a = {};
  int n = 0;
  bool vec = hw % 4 == 0 && aligned16(flow_gt) && aligned16(valid);
  for (int64_t i = 0; i < P; ++i) {
    if (!preds[i]) return DXR_EINVAL;
    if (!grad_preds[i]) continue;
    a.pred[n] = preds[i];
    a.grad[n] = grad_preds[i];
    a.c[n] = (float)(std::pow(gamma, (double)(P - 1 - i)) / M);
    vec = vec && aligned16(preds[i]) && aligned16(grad_preds[i]);
    ++n;
  }
  if (n == 0) return DXR_EINVAL;
  const int64_t groups = (npix + 3) / 4;
  const int64_t nwg = (groups + SL_THREADS - 1) / SL_THREADS;
  sequence_loss_backward_kernel<<<dim3((unsigned)nwg), dim3(SL_THREADS), 0, stream>>>(
      a, n, grad_loss, flow_gt, valid, npix, hw, max_flow, vec);
  return dxr::launch_status();
}
