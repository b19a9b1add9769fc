// Stage (d) backward on the matrix cores: dxr_alt_corr_backward with
// DXR_ALT_BWD_ACCUMULATE.  The gradients of the on-the-fly
// lookup (alt_cuda_corr/correlation_kernel.cu:122-256) are ADDED into fmap1_grad
// and fmap2_grad; the caller zero-fills.
//
// The per-query kernel (alt_corr.hip, alt_corr_backward_kernel) issues one float
// atomic per (query, window cell, channel) and is bound by them.  Here a
// workgroup owns a 4 x 8 tile of query pixels of one (pair, coordinate set), as
// the forward's box GEMM does (alt_corr.hip, alt_corr_mfma_kernel), and works on
// the union bounding box of its live queries' (2r+2)^2 windows, clipped to the
// map, in chunks of 32 cells (row-major in the box):
//   Wt[cell, q] = the <= 4 corr_grad taps that window cell feeds, weighted
//                 dy dx, dy (1-dx), (1-dy) dx, (1-dy)(1-dx) (:197-216; the `g`
//                 of the per-query kernel), 0 outside q's window
//   dF2[cell, :]  = sum_q    Wt[cell, q] fmap1[q, :]    GEMM 1, K = 32 queries
//   dF1[q, :]    += sum_cell Wt[cell, q] fmap2[cell, :]  GEMM 2, K = 32 cells
// both on v_mfma_f32_32x32x2_f32 (exact f32 products, f32 accumulation: no
// magnitude bound on corr_grad).  GEMM 1's tile goes to fmap2_grad with one
// float atomic per (box cell, channel) per workgroup — the (2r+2)^2 per-query
// atomics of a cell's up to 32 queries folded into one; GEMM 2 accumulates in
// registers across the chunks and the owning workgroup adds it to fmap1_grad
// once (a plain read-add-write: a (query, coordinate set) belongs to exactly one
// workgroup and calls are stream-ordered; atomics when Nc > 1 puts the sets of
// one query in different workgroups).  A wave owns 32-channel column blocks
// (wave, wave + 4) of both GEMMs.
//
// A query with a NaN / infinite / far coordinate, or whose window lies off the
// map, is not live: it takes no part in the box and its Wt column is exactly 0
// (its corr_grad taps are never read into a weight).  Zero weights multiply
// fmap1 rows and fmap2 cells the per-query form never reads, so fmaps and
// corr_grad must be finite (0 * inf is NaN): the contract of the flagged call.
// A chunk no window touches is skipped, and GEMM 1 skips the query pairs whose
// windows miss the chunk.
#include <cstdint>

#include "dxr_common.h"
#include "mfma_operands.h"

namespace {

using dxr::f32x16_t;


constexpr int BQY = 4, BQX = 8, BQ = BQY * BQX;   // query tile (32 pixels)
constexpr int BCH = 32;                           // box cells per chunk
constexpr int BWP = BCH + 1;                      // Wt row pitch (odd: GEMM 1 reads columns)
constexpr int BCMAX = 256;                        // channels served
constexpr int BNS = BCMAX / 32 / 4;               // 32-channel column blocks per wave

template <int R>
__global__ __launch_bounds__(256) void alt_corr_bwd_mfma_kernel(
    const float* __restrict__ f1, const float* __restrict__ f2, const float* __restrict__ coords,
    const float* __restrict__ cgrad, float* __restrict__ f1g, float* __restrict__ f2g, int N,
    int W1, int H2, int W2, int C, int Nc, int tiles_x) {
  constexpr int RD = 2 * R + 1, RD1 = RD + 1, RR = RD * RD;   // RR is odd: a conflict-free pitch
  __shared__ __attribute__((aligned(16))) float F1s[BQ * BCMAX];   // [q][c], pitch C
  __shared__ float Gs[BQ * RR];                                    // [q][oy + RD ox]
  __shared__ float Wt[BCH * BWP];                                  // [cell][q]
  __shared__ int4 qinfo[BQ];                                       // {x0, y0, live, query or -1}
  __shared__ float2 qfrac[BQ];                                     // {dx, dy}
  __shared__ int box[4];                                           // bx0, by0, bw, bh
  __shared__ int cellofs[BCH];                                     // cell index on the map or -1
  __shared__ unsigned qmask[2];                                    // queries touching the chunk

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // XCD k takes the k-th contiguous band of tiles (alt_corr_mfma_kernel): neighbouring
  // tiles, whose boxes overlap, then share one L2
  int tile = blockIdx.x;
  {
    const int n = gridDim.x, q8 = n / 8, r8 = n % 8, xcd = tile % 8;
    tile = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + tile / 8;
  }
  const int tx = tile % tiles_x, ty = tile / tiles_x;
  const int z = blockIdx.z, b = z / Nc;
  const int H1 = N / W1;
  const float* cz = coords + (long long)z * N * 2;
  const float* f1b = f1 + (long long)b * N * C;
  const float* f2b = f2 + (long long)b * H2 * W2 * C;
  float* f2gb = f2g + (long long)b * H2 * W2 * C;
  // slot qq of the tile -> query pixel, -1 past the image
  auto query_of = [&](int qq) -> int {
    const int qy = ty * BQY + qq / BQX, qx = tx * BQX + qq % BQX;
    return (qy < H1 && qx < W1) ? qy * W1 + qx : -1;
  };

  // ---- coordinates, window origins, the live windows' union box
  if (tid < BQ) {
    const int q = query_of(tid);
    int x0 = 0, y0 = 0, live = 0;
    float dx = 0.f, dy = 0.f;
    if (q >= 0) {
      const float x = cz[(long long)q * 2], y = cz[(long long)q * 2 + 1];
      const float xf = floorf(x), yf = floorf(y);
      if (fabsf(xf) < 1.0e8f && fabsf(yf) < 1.0e8f) {   // false for NaN and +-inf
        x0 = (int)xf - R;
        y0 = (int)yf - R;
        live = (x0 + RD1 > 0 && x0 < W2 && y0 + RD1 > 0 && y0 < H2) ? 1 : 0;
        if (live) {
          dx = x - xf;
          dy = y - yf;
        }
      }
    }
    qinfo[tid] = make_int4(x0, y0, live, q);
    qfrac[tid] = make_float2(dx, dy);
    int lx0 = live ? max(x0, 0) : 0x7fffffff, ly0 = live ? max(y0, 0) : 0x7fffffff;
    int lx1 = live ? min(x0 + RD1, W2) : -1, ly1 = live ? min(y0 + RD1, H2) : -1;
#pragma unroll
    for (int o = 1; o < BQ; o <<= 1) {
      lx0 = min(lx0, __shfl_xor(lx0, o));
      ly0 = min(ly0, __shfl_xor(ly0, o));
      lx1 = max(lx1, __shfl_xor(lx1, o));
      ly1 = max(ly1, __shfl_xor(ly1, o));
    }
    if (tid == 0) {
      const bool any = lx1 > lx0;
      box[0] = any ? lx0 : 0;
      box[1] = any ? ly0 : 0;
      box[2] = any ? lx1 - lx0 : 0;
      box[3] = any ? ly1 - ly0 : 0;
      qmask[0] = 0u;
      qmask[1] = 0u;
    }
  }
  // ---- the tile's fmap1 rows (zero past the image) and corr_grad taps
  const int c4n = C / 4;
  for (int u = tid; u < BQ * c4n; u += 256) {
    const int qq = u / c4n, c4 = u - qq * c4n;
    const int q = query_of(qq);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q >= 0) v = *reinterpret_cast<const float4*>(f1b + (long long)q * C + 4 * c4);
    *reinterpret_cast<float4*>(&F1s[qq * C + 4 * c4]) = v;
  }
  for (int u = tid; u < BQ * RR; u += 256) {
    const int qq = u & (BQ - 1), i = u / BQ;
    const int q = query_of(qq);
    Gs[qq * RR + i] = q >= 0 ? cgrad[((long long)z * RR + i) * N + q] : 0.f;
  }
  __syncthreads();

  const int bx0 = box[0], by0 = box[1], bw = box[2], bh = box[3];
  const int ncells = bw * bh;
  if (ncells == 0) return;   // no live query (the whole workgroup: box is shared)
  const int j = lane & 31, kh = lane >> 5;
  const int ncb = (C + 31) / 32;
  // build role: query bq, cells (tid >> 5) + 8 i of the chunk
  const int bq = tid & (BQ - 1);
  const int4 qi = qinfo[bq];
  const float2 qd = qfrac[bq];
  const float* gq = Gs + bq * RR;

  f32x16_t acc2[BNS];
#pragma unroll
  for (int s = 0; s < BNS; ++s)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[s][r] = 0.f;

  int par = 0;
  for (int c0 = 0; c0 < ncells; c0 += BCH, par ^= 1) {
    // ---- Wt of this chunk
    if (tid < BCH) {
      const int c = c0 + tid;
      int co = -1;
      if (c < ncells) {
        const int cy = c / bw, cx = c - cy * bw;
        co = (by0 + cy) * W2 + bx0 + cx;
      }
      cellofs[tid] = co;
    }
    if (tid == 0) qmask[par ^ 1] = 0u;   // the next chunk's (read last before the barrier below)
    bool touch = false;
#pragma unroll
    for (int i = 0; i < BCH / 8; ++i) {
      const int cl = (tid >> 5) + 8 * i, c = c0 + cl;
      float w = 0.f;
      if (qi.z && c < ncells) {
        const int cy = c / bw, cx = c - cy * bw;
        const int iy = by0 + cy - qi.y, ix = bx0 + cx - qi.x;
        if (iy >= 0 && iy <= RD && ix >= 0 && ix <= RD) {
          touch = true;
          const float dx = qd.x, dy = qd.y;
          if (iy > 0 && ix > 0) w += gq[(iy - 1) + RD * (ix - 1)] * dy * dx;
          if (iy > 0 && ix < RD) w += gq[(iy - 1) + RD * ix] * dy * (1.f - dx);
          if (iy < RD && ix > 0) w += gq[iy + RD * (ix - 1)] * (1.f - dy) * dx;
          if (iy < RD && ix < RD) w += gq[iy + RD * ix] * (1.f - dy) * (1.f - dx);
        }
      }
      Wt[cl * BWP + bq] = w;
    }
    {
      const unsigned long long bal = __ballot(touch);
      const unsigned m = (unsigned)bal | (unsigned)(bal >> 32);
      if (lane == 0 && m) atomicOr(&qmask[par], m);
    }
    __syncthreads();
    const unsigned qm = (unsigned)__builtin_amdgcn_readfirstlane((int)qmask[par]);
    if (qm != 0u) {
      // ---- GEMM 1: dF2[cell, c] = sum_q Wt[cell, q] fmap1[q, c]  (rows = cells)
#pragma unroll
      for (int s = 0; s < BNS; ++s) {
        const int cb = wave + 4 * s;
        if (cb >= ncb) break;
        const int c = cb * 32 + j;
        const bool cok = c < C;
        const int cc = cok ? c : 0;
        f32x16_t acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc1[r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < BQ / 2; ++kk) {
          if (((qm >> (2 * kk)) & 3u) == 0u) continue;   // wave-uniform: both queries miss the chunk
          const float a = Wt[j * BWP + 2 * kk + kh];
          const float v = F1s[(2 * kk + kh) * C + cc];
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, cok ? v : 0.f, acc1, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = (r & 3) + 8 * (r >> 2) + 4 * kh;
          const int co = cellofs[row];
          const float v = acc1[r];
          if (co >= 0 && cok && v != 0.f) unsafeAtomicAdd(f2gb + (long long)co * C + c, v);
        }
      }
      // ---- GEMM 2: dF1[q, c] += sum_cell Wt[cell, q] fmap2[cell, c]  (rows = queries)
#pragma unroll
      for (int kk = 0; kk < BCH / 2; ++kk) {
        const int cl = 2 * kk + kh;
        const float a = Wt[cl * BWP + j];
        const int co = cellofs[cl];
#pragma unroll
        for (int s = 0; s < BNS; ++s) {
          const int cb = wave + 4 * s;
          if (cb >= ncb) break;
          const int c = cb * 32 + j;
          const float v = (co >= 0 && c < C) ? f2b[(long long)co * C + c] : 0.f;
          acc2[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, v, acc2[s], 0, 0, 0);
        }
      }
    }
    __syncthreads();   // Wt, cellofs and qmask[par] are rebuilt / cleared from here on
  }

  // ---- fmap1_grad: this workgroup owns its queries' rows for this coordinate set
#pragma unroll
  for (int s = 0; s < BNS; ++s) {
    const int cb = wave + 4 * s;
    if (cb >= ncb) break;
    const int c = cb * 32 + j;
    if (c >= C) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * kh;
      const int q = qinfo[row].w;
      const float v = acc2[s][r];
      if (q < 0 || v == 0.f) continue;
      float* p = f1g + ((long long)b * N + q) * C + c;
      if (Nc > 1) unsafeAtomicAdd(p, v);
      else *p += v;
    }
  }
}

template <int R>
int launch_bwd_mfma(const float* f1, const float* f2, const float* coords, const float* cgrad,
                    float* f1g, float* f2g, int B, int H1, int W1, int H2, int W2, int C, int Nc,
                    hipStream_t stream) {
  const int tiles_x = (W1 + BQX - 1) / BQX, tiles_y = (H1 + BQY - 1) / BQY;
  const dim3 grid((unsigned)(tiles_x * tiles_y), 1u, (unsigned)(B * Nc));
  hipLaunchKernelGGL((alt_corr_bwd_mfma_kernel<R>), grid, dim3(256), 0, stream, f1, f2, coords,
                     cgrad, f1g, f2g, H1 * W1, W1, H2, W2, C, Nc, tiles_x);
  return dxr::launch_status();
}

bool bwd_aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace

namespace dxr {

// dxr_alt_corr_backward with DXR_ALT_BWD_ACCUMULATE on `radius` (passed whole;
// the geometry is already known to be positive and radius >= 0).  Everything
// is answered here, on the host, before the one launch.
int alt_backward_accumulate(const float* fmap1, const float* fmap2, const float* coords,
                            const float* corr_grad, float* fmap1_grad, float* fmap2_grad,
                            int64_t B, int64_t H1, int64_t W1, int64_t H2, int64_t W2, int64_t C,
                            int64_t Nc, int radius, hipStream_t stream) {
  if (radius & ~(DXR_ALT_BWD_ACCUMULATE | 0xff)) return DXR_EINVAL;
  const int r = radius & 0xff;
  if (r > 6) return DXR_EUNSUPPORTED;
  if (H1 * W1 > (1LL << 30) || H2 * W2 > (1LL << 30) || B > 65535 || C > (1 << 20))
    return DXR_EINVAL;
  if (B == 0) return DXR_OK;
  if (!fmap1 || !fmap2 || !fmap1_grad || !fmap2_grad) return DXR_EINVAL;
  if (Nc > 0 && (!coords || !corr_grad)) return DXR_EINVAL;
  if (C % 16 != 0 || C > BCMAX || B * Nc > 65535 || !bwd_aligned16(fmap1) ||
      !bwd_aligned16(fmap2) || !bwd_aligned16(fmap1_grad) || !bwd_aligned16(fmap2_grad))
    return DXR_EUNSUPPORTED;
  if (Nc == 0) return DXR_OK;   // nothing to add
  const int b = (int)B, h1 = (int)H1, w1 = (int)W1, h2 = (int)H2, w2 = (int)W2, c = (int)C,
            nc = (int)Nc;
  return dispatch_radius<6>(r, [&](auto rr) {
    return launch_bwd_mfma<decltype(rr)::value>(fmap1, fmap2, coords, corr_grad, fmap1_grad,
                                                fmap2_grad, b, h1, w1, h2, w2, c, nc, stream);
  });
}

}  // namespace dxr
