// Which kernel serves a pyramid build request: the host-only planner behind
// dxr_corr_pyramid_build / _build_ws (include/dexiraft_corr.h, "Kernels by
// request").  Plain C++, no HIP: pyramid_build (corr_build.hip) calls plan_build
// and switches on its result, and tests/test_build_plan.py runs the same
// function on a CPU, row by row of that table.  Every refusal is answered here,
// so the launchers validate nothing.
#pragma once

#include <stdint.h>

#include "dexiraft_corr.h"
#include "pyramid_layout.h"

namespace dxr {

// One value per row of the header's table.
enum BuildPath {
  BUILD_NONE = 0,          // B == 0, or a refused request: nothing to launch
  BUILD_DMA_F32_NCHW,      // pre-split f16 pairs + LDS-DMA build (workspace)
  BUILD_DMA_F32_NHWC,
  BUILD_SPLIT_F4,          // register split build, float4 target units
  BUILD_SPLIT_F2,          //   float2 units (even W)
  BUILD_SPLIT_NHWC,        //   channels-last operands
  BUILD_EXACT_VEC,         // exact-f32 MFMA build, float4 staging
  BUILD_EXACT_SCALAR,
  BUILD_PACK_DMA16,        // 16-bit pack pass + LDS-DMA build (NCHW, workspace)
  BUILD_DMA16_NHWC,        // 16-bit LDS-DMA build on channels-last rows in place
  BUILD_BF16_Q2,           // two query blocks per workgroup
  BUILD_BF16               // one query block, scalar staging
};

inline const char* build_path_name(int path) {
  switch (path) {
    case BUILD_DMA_F32_NCHW: return "split_pairs_kernel<NCHW> + corr_build_dma_kernel";
    case BUILD_DMA_F32_NHWC: return "split_pairs_kernel<NHWC> + corr_build_dma_kernel";
    case BUILD_SPLIT_F4: return "corr_build_split_kernel<float4>";
    case BUILD_SPLIT_F2: return "corr_build_split_kernel<float2>";
    case BUILD_SPLIT_NHWC: return "corr_build_split_kernel<NHWC>";
    case BUILD_EXACT_VEC: return "corr_build_f32_kernel<vec>";
    case BUILD_EXACT_SCALAR: return "corr_build_f32_kernel<scalar>";
    case BUILD_PACK_DMA16: return "pack_bf16_kernel + corr_build_dma_kernel";
    case BUILD_DMA16_NHWC: return "corr_build_dma_kernel";
    case BUILD_BF16_Q2: return "corr_build_bf16_q2_kernel";
    case BUILD_BF16: return "corr_build_bf16_kernel";
    default: return "none";
  }
}

// Everything pyramid_build receives, pointers as integers.
struct BuildRequest {
  int in_dtype, fmap_layout;
  int64_t B, D, H, W;
  int num_levels;
  float divisor;
  int pyr_dtype, algo;
  uintptr_t fmap1, fmap2, pyramid, workspace;
  int64_t workspace_bytes;
};

struct BuildPlan {
  int path;         // BuildPath
  int operand;      // in_dtype: the 16-bit paths' record kind (DXR_BF16 or DXR_F16)
  int cells;        // pyr_dtype: the pyramid's cell type
  bool pool_extra;  // f32 pooling passes for the levels beyond the fused four follow
};

// Sizes that answer -1 instead of overflowing int64; a negative operand (an
// earlier overflow) stays -1.
inline long long size_mul(long long a, long long b) {
  long long r;
  return a < 0 || b < 0 || __builtin_mul_overflow(a, b, &r) ? -1 : r;
}
inline long long size_add(long long a, long long b) {
  long long r;
  return a < 0 || b < 0 || __builtin_add_overflow(a, b, &r) ? -1 : r;
}
inline long long align256(long long x) { return size_add(x, 255) < 0 ? -1 : (x + 255) & ~255LL; }

// Pre-split + LDS-DMA f32 build (round 3): workspace = SP1 | SP2 | E1 | E2.
inline long long dma_workspace_bytes(long long B, long long D, long long H, long long W) {
  const long long px = size_mul(B, size_mul(H, W));
  return size_add(size_mul(2, align256(size_mul(size_mul(px, D), 4))),
                  size_mul(2, align256(size_mul(px, 4))));
}
// The 16-bit pack pass's blocked copies of both NCHW fmaps.
inline long long bf16_pack_bytes(long long B, long long D, long long H, long long W) {
  return size_mul(2, align256(size_mul(size_mul(size_mul(B, D), size_mul(H, W)), 2)));
}

// dxr_build_workspace_bytes.
inline int64_t build_workspace_bytes(int in_dtype, int64_t B, int64_t D, int64_t H, int64_t W) {
  if (B < 0 || D < 1 || H < 1 || W < 1 || !pixels_ok(H, W)) return -1;
  if (in_dtype == DXR_BF16 || in_dtype == DXR_F16)   // the 16-bit pack pass of NCHW fmaps
    return D % 32 == 0 ? bf16_pack_bytes(B, D, H, W) : 0;
  if (in_dtype != DXR_F32 || D % 16 != 0) return 0;
  return dma_workspace_bytes(B, D, H, W);
}

// The pyramid's geometry exists (dxr::make_levels, pyramid_layout.h): every level
// at least 1 x 1, at most 8 levels, H * W <= 2^30.
inline bool levels_ok(int64_t B, int64_t H, int64_t W, int num_levels) {
  Levels L;
  return make_levels(B, H, W, num_levels, &L);
}

// Argument checks shared by the pyramid builds and dxr_corr_volume; DXR_OK:
// go on (with B == 0: nothing to do, whatever the pointers).
inline int check_build_args(int in_dtype, int64_t B, int64_t D, float divisor, int out_dtype) {
  if (D < 1 || D > (1 << 20) || !(divisor == divisor) || divisor == 0.f) return DXR_EINVAL;
  if (B > 65535) return DXR_EINVAL;
  if ((in_dtype != DXR_F32 && in_dtype != DXR_BF16 && in_dtype != DXR_F16) ||
      (out_dtype != DXR_F32 && out_dtype != DXR_BF16 && out_dtype != DXR_PYR_F16))
    return DXR_EINVAL;
  return DXR_OK;
}

// The 3-D build grid (tiles, query blocks, pairs) has ceil(N / 128) <= 65535 rows.
inline bool grid_rows_ok(int64_t H, int64_t W) { return (H * W + 127) / 128 <= 65535; }

// Status of a build request and, for DXR_OK, its plan.  The order of the checks
// is the contract: a request that is both invalid and unsupported answers what
// comes first here.
inline int plan_build(const BuildRequest& r, BuildPlan* plan) {
  *plan = BuildPlan{BUILD_NONE, r.in_dtype, r.pyr_dtype, false};
  if (!levels_ok(r.B, r.H, r.W, r.num_levels)) return DXR_EINVAL;
  if (r.fmap_layout != DXR_NCHW && r.fmap_layout != DXR_NHWC) return DXR_EINVAL;
  if (r.algo != DXR_BUILD_AUTO && r.algo != DXR_BUILD_EXACT_F32) return DXR_EINVAL;
  const int chk = check_build_args(r.in_dtype, r.B, r.D, r.divisor, r.pyr_dtype);
  if (chk != DXR_OK || r.B == 0) return chk;
  if (!r.fmap1 || !r.fmap2 || !r.pyramid) return DXR_EINVAL;
  // Levels beyond the fused four are pooled by f32 passes: f32 pyramids only.
  plan->pool_extra = r.num_levels > 4;
  if (plan->pool_extra && r.pyr_dtype != DXR_F32) return DXR_EUNSUPPORTED;
  if (r.algo == DXR_BUILD_EXACT_F32 && r.in_dtype != DXR_F32) return DXR_EUNSUPPORTED;

  const bool f32 = r.in_dtype == DXR_F32, nhwc = r.fmap_layout == DXR_NHWC;
  const bool automatic = r.algo == DXR_BUILD_AUTO;
  const long long dhw = r.D * r.H * r.W;   // < 2^50
  const auto al = [](uintptr_t p, unsigned n) { return p % n == 0; };
  const bool fmaps16 = al(r.fmap1, 16) && al(r.fmap2, 16), fmaps8 = al(r.fmap1, 8) && al(r.fmap2, 8);
  const bool pyr16 = al(r.pyramid, 16);
  const auto ws_holds = [&](long long bytes) {
    return r.workspace != 0 && al(r.workspace, 16) && r.workspace_bytes >= bytes;
  };
  // The 16-bit LDS-DMA forms: whole 32-channel stages, D * N * 2 < 2^31 per pair.
  const bool dma16 = r.D % 32 == 0 && dhw < (1LL << 30) && pyr16;
  const bool pack16 = dma16 && !nhwc && ws_holds(bf16_pack_bytes(r.B, r.D, r.H, r.W));
  // The f32 split forms: whole 16-channel stages; and the pre-split LDS-DMA
  // build on top of them, with a workspace (any W).
  const bool split = f32 && automatic && r.D % 16 == 0 && dhw < (1LL << 29);
  const bool dma32 = split && pyr16 && ws_holds(dma_workspace_bytes(r.B, r.D, r.H, r.W));

  int path;
  if (r.in_dtype == DXR_F16) {
    // float16 fmaps: the 16-bit DMA build on f16 records, or nothing (callers
    // widen to f32); into an f32 or a float16 pyramid.
    if (r.pyr_dtype == DXR_BF16 || !dma16) return DXR_EUNSUPPORTED;
    if (nhwc ? !fmaps16 : !pack16) return DXR_EUNSUPPORTED;
    path = nhwc ? BUILD_DMA16_NHWC : BUILD_PACK_DMA16;
  } else if (r.pyr_dtype == DXR_PYR_F16) {
    // a float16 pyramid from f32 fmaps: the pre-split DMA build alone stores it
    if (!dma32 || (nhwc && !fmaps16)) return DXR_EUNSUPPORTED;
    path = nhwc ? BUILD_DMA_F32_NHWC : BUILD_DMA_F32_NCHW;
  } else if (dma32 && (!nhwc || fmaps16)) {
    path = nhwc ? BUILD_DMA_F32_NHWC : BUILD_DMA_F32_NCHW;
  } else if (!f32 && pack16 && !plan->pool_extra) {
    path = BUILD_PACK_DMA16;
  } else if (nhwc && !f32) {
    // channels-last bf16 rows are read in place; callers transpose the rest
    if (!dma16 || !fmaps16) return DXR_EUNSUPPORTED;
    path = BUILD_DMA16_NHWC;
  } else if (nhwc) {
    // channels-last f32 without the DMA build: where the NCHW build would also
    // be the split build (even W: same bits), with 16-byte aligned rows
    if (!split || r.W % 2 != 0 || !fmaps16 || !pyr16) return DXR_EUNSUPPORTED;
    path = BUILD_SPLIT_NHWC;
  } else if (f32) {
    const bool vec = r.W % 4 == 0 && fmaps16 && pyr16;
    if (split && vec) path = BUILD_SPLIT_F4;
    else if (split && r.W % 2 == 0 && fmaps8 && pyr16) path = BUILD_SPLIT_F2;
    else path = vec ? BUILD_EXACT_VEC : BUILD_EXACT_SCALAR;
  } else {
    path = r.W % 4 == 0 && fmaps8 && pyr16 && dhw < (1LL << 30) ? BUILD_BF16_Q2 : BUILD_BF16;
  }
  // the 16-bit DMA builds run on a 1-D grid; every other path on the 3-D one
  if (path != BUILD_PACK_DMA16 && path != BUILD_DMA16_NHWC && !grid_rows_ok(r.H, r.W))
    return DXR_EINVAL;
  plan->path = path;
  return DXR_OK;
}

}  // namespace dxr
