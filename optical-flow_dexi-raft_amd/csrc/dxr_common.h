// Internal helpers shared by the HIP translation units of libdexiraft_corr.so.
// Not part of the public ABI (that is include/dexiraft_corr.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dexiraft_corr.h"
#include "mfma_operands.h"

namespace dxr {

// Thread-local record of the last failed HIP launch (dxr_last_hip_error()).
void set_last_hip_error(hipError_t e);

// Check the launch that was just issued; map a HIP error to DXR_EHIP.
inline int launch_status() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_last_hip_error(e);
    return DXR_EHIP;
  }
  return DXR_OK;
}

// A run-time radius in [MIN, MAX] as a std::integral_constant handed to `f`
// (which returns a status); any other radius is DXR_EUNSUPPORTED.  `f` is
// instantiated for exactly those radii.
template <int MAX, int MIN = 0, typename F>
int dispatch_radius(int radius, F&& f) {
  if constexpr (MIN <= MAX) {
    if (radius == MIN) return f(std::integral_constant<int, MIN>{});
    return dispatch_radius<MAX, MIN + 1>(radius, f);
  }
  return DXR_EUNSUPPORTED;
}

// ---------------------------------------------------------------------------
// The lookups' variant units.  A lookup's kernel forms are spread over several
// translation units; the entry point splits and validates the
// flags, fills one of the argument structs below and hands it to the unit that
// instantiates the form.  out_flag: 0 (float32 `out`), DXR_OUT_F16 or
// DXR_OUT_BF16; nhwc: DXR_OUT_NHWC (`out` is [B, H, W, C]).
// ---------------------------------------------------------------------------

// dxr_corr_lookup, and with `conv1x1` dxr_corr_lookup_conv1x1 (weight_packed,
// bias, cout, relu).  pyr_dtype: DXR_F32 / DXR_BF16 / DXR_PYR_F16, flags off.
struct LookupArgs {
  const void* pyramid;
  int pyr_dtype, out_flag;
  bool nhwc;
  int64_t B, H, W;
  int num_levels, radius;
  const float* coords;
  bool conv1x1;
  const void* weight_packed;
  const float* bias;
  int64_t cout;
  int relu;
  void* out;
  hipStream_t stream;
};
// 16-bit NCHW outputs of float32 / bfloat16 pyramids: corr_lookup_out16.hip.
int lookup_out16(const LookupArgs& a);
// float16 pyramids (DXR_PYR_F16), every NCHW output type: corr_lookup_pyr16.hip,
// the only unit that instantiates the lookup kernels with the float16 cell type.
int lookup_pyr16(const LookupArgs& a);
// Channels-last outputs, every cell and output type: corr_lookup_nhwc.hip.
int lookup_nhwc(const LookupArgs& a);

// dxr_alt_corr_lookup, _ws and _levels_ws (n_levels < 0: every level) with the
// flags off `radius`.  fmap1 and fmap2_levels[0] point at what the unit reads
// (float32, float16 or bfloat16), the further levels at float32.
struct AltLookupArgs {
  const float* fmap1;
  const float* const* fmap2_levels;
  const float* coords;
  void* out;
  int out_flag;
  bool nhwc;
  int64_t B, H, W, C;
  int num_levels, radius;
  float divisor;
  void* workspace;
  int64_t workspace_bytes;
  hipStream_t stream;
  int n_levels;
};
// float32 fmaps with an output flag (at least one set): alt_corr_out.hip.
int alt_lookup_out(const AltLookupArgs& a);
// DXR_ALT_IN_F16, with or without output flags: alt_corr_in16.hip.
int alt_lookup_in16(const AltLookupArgs& a);
// DXR_ALT_IN_BF16, likewise: alt_corr_inbf16.hip.
int alt_lookup_inbf16(const AltLookupArgs& a);

// dxr_alt_volume_lookup with the flags off `radius`; `volumes` holds float32 or
// (DXR_ALT_VOL_F16) float16 cells.
struct AltVolumeArgs {
  const void* volumes;
  const float* coords;
  void* out;
  int out_flag;
  bool nhwc;
  int64_t B, H, W;
  int num_levels, first_level, radius;
  float divisor;
  hipStream_t stream;
};
// float32 volumes with an output flag (at least one set): corr_lookup_alt_out.hip.
int alt_volume_lookup_out(const AltVolumeArgs& a);
// float16 volumes, every output form: corr_lookup_alt_vol16.hip, the only unit
// that instantiates the volume lookup with the float16 cell type.
int alt_volume_lookup_vol16(const AltVolumeArgs& a);

// dxr_alt_corr_backward with DXR_ALT_BWD_ACCUMULATE on `radius` (passed whole; B,
// the map sizes and C already checked positive, radius >= 0): validation and
// the MFMA kernel that adds into both gradients.  Defined in alt_corr_bwd.hip.
int alt_backward_accumulate(const float* fmap1, const float* fmap2, const float* coords,
                            const float* corr_grad, float* fmap1_grad, float* fmap2_grad,
                            int64_t B, int64_t H1, int64_t W1, int64_t H2, int64_t W2, int64_t C,
                            int64_t Nc, int radius, hipStream_t stream);

// ---------------------------------------------------------------------------
// Pyramid layout ("paged" correlation volume).
//
// Level sizes follow F.avg_pool2d(2, stride=2) floor mode: H_l = floor(H_{l-1}/2).
// Storage is tiled so that each build workgroup owns one contiguous block:
// a PAGE = (QB query pixels) x (one TH x TW tile of image-2 cells).  Levels 0..3
// use QB = 128 and a level-0 tile of 8 x 16 cells, pooled to 4x8, 2x4, 1x2 at
// levels 1..3 (so one page's pooled cells come from the same workgroup).  Pages
// are padded: queries to a multiple of 128, image-2 to whole tiles.  Levels >= 4
// are plain row-major images (QB = 1, one tile = the whole level).  The element
// index of (pair b, query q, cell y, x) at a level is
//   ((((b*QT + q/QB)*TY + y/TH)*TX + x/TW)*QB + q%QB)*(TH*TW) + (y%TH)*TW + x%TW
// ---------------------------------------------------------------------------
constexpr int PAGE_Q = 128;    // queries per page (levels 0..3)
constexpr int PAGE_H = 8;      // level-0 tile rows
constexpr int PAGE_W = 16;     // level-0 tile cols
constexpr int TILED_LEVELS = 4;

struct LevelLayout {
  int h, w;          // true level size (floor-mode pooling)
  int th, tw;        // tile rows / cols at this level
  int ty, tx;        // tiles per image along y / x
  int qb, qt;        // queries per page, query blocks per pair
  long long off;     // element offset of the level in the pyramid buffer
};

struct Levels {
  int n;
  int h[8];
  int w[8];
  int64_t off[8];  // element offset of each level in the pyramid buffer
  int64_t numel;
  LevelLayout lay[8];
};

inline bool make_levels(int64_t B, int64_t H, int64_t W, int num_levels, Levels* L) {
  if (B < 0 || H < 1 || W < 1 || num_levels < 1 || num_levels > 8) return false;
  if (H * W > (1LL << 30)) return false;
  const int64_t N = H * W;
  const int64_t qt = (N + PAGE_Q - 1) / PAGE_Q;
  const int64_t ty = (H + PAGE_H - 1) / PAGE_H, tx = (W + PAGE_W - 1) / PAGE_W;
  int64_t off = 0, h = H, w = W;
  L->n = num_levels;
  for (int l = 0; l < num_levels; ++l) {
    if (l > 0) { h /= 2; w /= 2; }
    if (h < 1 || w < 1) return false;
    LevelLayout& y = L->lay[l];
    y.h = (int)h;
    y.w = (int)w;
    y.off = off;
    if (l < TILED_LEVELS) {
      y.th = PAGE_H >> l; y.tw = PAGE_W >> l;
      y.ty = (int)ty; y.tx = (int)tx;
      y.qb = PAGE_Q; y.qt = (int)qt;
      off += B * qt * PAGE_Q * ty * tx * (int64_t)y.th * y.tw;
    } else {
      y.th = (int)h; y.tw = (int)w; y.ty = 1; y.tx = 1; y.qb = 1; y.qt = (int)N;
      off += B * N * h * w;
    }
    L->h[l] = (int)h;
    L->w[l] = (int)w;
    L->off[l] = y.off;
  }
  L->numel = off;
  return true;
}

// Element index of (pair b, query q, cell y, x) inside one level (see above).
__host__ __device__ __forceinline__ long long cell_index(const LevelLayout& y, int b, int q, int cy,
                                                        int cx) {
  const long long page = (((long long)b * y.qt + q / y.qb) * y.ty + cy / y.th) * y.tx + cx / y.tw;
  return y.off + (page * y.qb + q % y.qb) * (y.th * y.tw) + (cy % y.th) * y.tw + cx % y.tw;
}

}  // namespace dxr
