// forward_interpolate on the GPU (include/dexiraft_flow.h; reference
// core/utils/utils.py:26-54): every grid point takes the flow of the nearest
// forward-warped source, by an exhaustive float64 search with a specified tie
// rule (lowest flat source index).
//
// Three launches per call, all on the caller's stream, no atomics:
//   flow_interp_land_kernel    (x1, y1) of every source as a double pair; an
//                              invalid source is written as (+inf, +inf): its
//                              d2 is +inf, which never passes the strict `<`.
//   flow_interp_search_kernel  grid = (grid-point tiles, source slices, items).
//                              A workgroup stages its slice through LDS in
//                              chunks; every lane reads the same source (a
//                              broadcast read), keeps its own (best d2, best
//                              index) and writes one partial per slice.
//   flow_interp_reduce_kernel  folds the slices in ascending order with the
//                              same strict `<` and copies the winner's flow.
// Sources are visited in ascending index order everywhere and a later candidate
// replaces the best only when strictly nearer, so among equal d2 the lowest
// index wins whatever the split.
#include "dexiraft_flow.h"
#include "dxr_common.h"

namespace {

constexpr int FI_TILE = 256;    // grid points per workgroup = threads per workgroup
constexpr int FI_CHUNK = 256;   // sources staged in LDS at a time (one per thread)
constexpr int64_t FI_TARGET_WG = 1024;      // workgroups the split aims at (4 per CU)
constexpr int64_t FI_MAX_N = 1LL << 22;
constexpr int64_t FI_MAX_B = 65535;         // grid.z / grid.y limit

struct Plan {
  int64_t n;           // sources = grid points per item
  int tiles;           // grid-point tiles per item
  int slices;          // source slices per item
  int slice_len;       // sources per slice, a multiple of FI_CHUNK
  int64_t item_bytes;  // workspace per item (an upper bound that does not depend on B)
};

// Partial slots per item are bounded by min(ceil(n / CHUNK) * n, TARGET * TILE + n):
// slices <= ceil(n / CHUNK), and slices > 1 only while slices * tiles <= TARGET.
// Both terms grow with n, so the workspace size is monotone.
inline bool make_plan(int64_t B, int64_t H, int64_t W, Plan* p) {
  if (B < 0 || B > FI_MAX_B || H < 1 || W < 1 || H > FI_MAX_N || W > FI_MAX_N || H * W > FI_MAX_N)
    return false;
  const int64_t n = H * W;
  const int64_t tiles = (n + FI_TILE - 1) / FI_TILE, chunks = (n + FI_CHUNK - 1) / FI_CHUNK;
  int64_t want = FI_TARGET_WG / (tiles * (B > 0 ? B : 1));
  want = want < 1 ? 1 : (want > chunks ? chunks : want);
  const int64_t per = (n + want - 1) / want;
  const int64_t slice_len = (per + FI_CHUNK - 1) / FI_CHUNK * FI_CHUNK;
  p->n = n;
  p->tiles = (int)tiles;
  p->slice_len = (int)slice_len;
  p->slices = (int)((n + slice_len - 1) / slice_len);
  const int64_t a = chunks * n, b = FI_TARGET_WG * FI_TILE + n;
  const int64_t slots = a < b ? a : b;
  p->item_bytes = (16 * n + 12 * slots + 15) / 16 * 16;
  return true;
}

// Workspace of one item: double2 land[n]; double part_d2[slices][n]; int part_idx[slices][n].
__device__ __forceinline__ double2* ws_land(char* ws, int64_t item_bytes, int b) {
  return reinterpret_cast<double2*>(ws + (int64_t)b * item_bytes);
}
__device__ __forceinline__ double* ws_d2(char* ws, int64_t item_bytes, int b, int n) {
  return reinterpret_cast<double*>(ws + (int64_t)b * item_bytes + 16LL * n);
}
__device__ __forceinline__ int* ws_idx(char* ws, int64_t item_bytes, int b, int n, int slices) {
  return reinterpret_cast<int*>(ws + (int64_t)b * item_bytes + 16LL * n + 8LL * slices * n);
}

__global__ __launch_bounds__(FI_TILE) void flow_interp_land_kernel(
    const float* __restrict__ flow, char* __restrict__ ws, int64_t item_bytes, int n, int H, int W) {
  const int i = blockIdx.x * FI_TILE + threadIdx.x, b = blockIdx.y;
  if (i >= n) return;
  const float* f = flow + (int64_t)b * 2 * n;
  const double x1 = (double)(i % W) + (double)f[i];
  const double y1 = (double)(i / W) + (double)f[n + i];
  const bool valid = x1 > 0.0 && x1 < (double)W && y1 > 0.0 && y1 < (double)H;   // NaN: false
  const double inf = __builtin_huge_val();
  ws_land(ws, item_bytes, b)[i] = valid ? make_double2(x1, y1) : make_double2(inf, inf);
}

__global__ __launch_bounds__(FI_TILE) void flow_interp_search_kernel(
    char* __restrict__ ws, int64_t item_bytes, int n, int W, int slice_len, int slices) {
  __shared__ double2 land[FI_CHUNK];
  const int tid = threadIdx.x, s = blockIdx.y, b = blockIdx.z;
  const int g = blockIdx.x * FI_TILE + tid;
  const double2* src = ws_land(ws, item_bytes, b);
  const double gx = (double)(g % W), gy = (double)(g / W);
  const double inf = __builtin_huge_val();
  double best = inf;
  int best_i = -1;
  const int s0 = s * slice_len, s1 = min(n, s0 + slice_len);
  for (int c = s0; c < s1; c += FI_CHUNK) {
    __syncthreads();
    const int i = c + tid;
    land[tid] = i < s1 ? src[i] : make_double2(inf, inf);
    __syncthreads();
#pragma unroll 8
    for (int j = 0; j < FI_CHUNK; ++j) {
      // each operation rounded on its own: hipcc contracts a*b + c into an FMA by default
      // (through __dmul_rn / __dadd_rn too, which are plain operators here)
#pragma clang fp contract(off)
      const double2 p = land[j];
      const double ex = gx - p.x, ey = gy - p.y;
      const double xx = ex * ex, yy = ey * ey;
      const double d2 = xx + yy;
      if (d2 < best) {
        best = d2;
        best_i = c + j;
      }
    }
  }
  if (g < n) {
    ws_d2(ws, item_bytes, b, n)[(int64_t)s * n + g] = best;
    ws_idx(ws, item_bytes, b, n, slices)[(int64_t)s * n + g] = best_i;
  }
}

__global__ __launch_bounds__(FI_TILE) void flow_interp_reduce_kernel(
    const uint32_t* __restrict__ flow, uint32_t* __restrict__ out, char* __restrict__ ws,
    int64_t item_bytes, int n, int slices) {
  const int g = blockIdx.x * FI_TILE + threadIdx.x, b = blockIdx.y;
  if (g >= n) return;
  const double* __restrict__ d2 = ws_d2(ws, item_bytes, b, n);
  const int* __restrict__ idx = ws_idx(ws, item_bytes, b, n, slices);
  double best = __builtin_huge_val();
  int best_i = -1;
  for (int s = 0; s < slices; ++s) {   // ascending slices = ascending source indices
    const double d = d2[(int64_t)s * n + g];
    const int i = idx[(int64_t)s * n + g];
    if (d < best) {
      best = d;
      best_i = i;
    }
  }
  const uint32_t* f = flow + (int64_t)b * 2 * n;
  uint32_t* o = out + (int64_t)b * 2 * n;
  o[g] = best_i >= 0 ? f[best_i] : 0u;           // the bits, copied
  o[n + g] = best_i >= 0 ? f[n + best_i] : 0u;
}

}  // namespace

extern "C" int dxf_abi_version(void) { return DXF_ABI_VERSION; }

extern "C" int64_t dxf_forward_interpolate_workspace_bytes(int64_t B, int64_t H, int64_t W) {
  Plan p;
  if (!make_plan(B, H, W, &p)) return -1;
  return B * p.item_bytes;
}

extern "C" int dxf_forward_interpolate(const float* flow, int64_t B, int64_t H, int64_t W,
                                       float* out, void* workspace, int64_t workspace_bytes,
                                       hipStream_t stream) {
  if (B == 0) return DXR_OK;
  Plan p;
  if (!make_plan(B, H, W, &p)) return DXR_EINVAL;
  if (!flow || !out || !workspace) return DXR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return DXR_EINVAL;
  if (workspace_bytes < B * p.item_bytes) return DXR_EINVAL;
  char* ws = static_cast<char*>(workspace);
  const int n = (int)p.n;
  const dim3 block(FI_TILE);
  flow_interp_land_kernel<<<dim3(p.tiles, (unsigned)B), block, 0, stream>>>(
      flow, ws, p.item_bytes, n, (int)H, (int)W);
  int st = dxr::launch_status();
  if (st != DXR_OK) return st;
  flow_interp_search_kernel<<<dim3(p.tiles, p.slices, (unsigned)B), block, 0, stream>>>(
      ws, p.item_bytes, n, (int)W, p.slice_len, p.slices);
  st = dxr::launch_status();
  if (st != DXR_OK) return st;
  flow_interp_reduce_kernel<<<dim3(p.tiles, (unsigned)B), block, 0, stream>>>(
      reinterpret_cast<const uint32_t*>(flow), reinterpret_cast<uint32_t*>(out), ws, p.item_bytes,
      n, p.slices);
  return dxr::launch_status();
}
