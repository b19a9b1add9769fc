// Internal helpers shared by the HIP translation units of libdexiraft_corr.so.
// Not part of the public ABI (that is include/dexiraft_corr.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dexiraft_corr.h"
#include "lookup_plan.h"
#include "mfma_operands.h"
#include "pyramid_layout.h"

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
// translation units; the entry point plans the request
// (lookup_plan.h: the flags, every check, the unit, the shape), fills one of the
// argument structs below and hands it to the unit its plan names.  The units
// only pick the template instantiation: they do not plan again.
// ---------------------------------------------------------------------------

// dxr_corr_lookup, and with plan->conv1x1 dxr_corr_lookup_conv1x1 (weight_packed,
// bias, cout, relu).
struct LookupArgs {
  const LookupPlan* plan;
  const void* pyramid;
  const float* coords;
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

// dxr_alt_corr_lookup, _ws and _levels_ws.  fmap1 and fmap2_levels[0] point at
// what the unit reads (float32, float16 or bfloat16), the further levels at
// float32; plan->levels of them are read.
struct AltLookupArgs {
  const AltLookupPlan* plan;
  const float* fmap1;
  const float* const* fmap2_levels;
  const float* coords;
  void* out;
  int64_t B, H, W, C;
  int num_levels;
  float divisor;
  void* workspace;
  hipStream_t stream;
};
// float32 fmaps with an output flag (at least one set): alt_corr_out.hip.
int alt_lookup_out(const AltLookupArgs& a);
// DXR_ALT_IN_F16, with or without output flags: alt_corr_in16.hip.
int alt_lookup_in16(const AltLookupArgs& a);
// DXR_ALT_IN_BF16, likewise: alt_corr_inbf16.hip.
int alt_lookup_inbf16(const AltLookupArgs& a);

// dxr_alt_volume_lookup; `volumes` holds float32 or (DXR_ALT_VOL_F16) float16 cells.
struct AltVolumeArgs {
  const VolumeLookupPlan* plan;
  const void* volumes;
  const float* coords;
  void* out;
  int num_levels, first_level;
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

// Element index of (pair b, query q, cell y, x) inside one level (pyramid_layout.h).
__host__ __device__ __forceinline__ long long cell_index(const LevelLayout& y, int b, int q, int cy,
                                                        int cx) {
  const long long page = (((long long)b * y.qt + q / y.qb) * y.ty + cy / y.th) * y.tx + cx / y.tw;
  return y.off + (page * y.qb + q % y.qb) * (y.th * y.tw) + (cy % y.th) * y.tw + cx % y.tw;
}

}  // namespace dxr
