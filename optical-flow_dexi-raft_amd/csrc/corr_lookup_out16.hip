// The lookup's 16-bit output instantiations (float16 / bfloat16 stores:
// DXR_OUT_F16 / DXR_OUT_BF16 of dxr_corr_lookup and dxr_corr_lookup_conv1x1).
// The kernels are corr_lookup.hip's templates; they are instantiated in this
// translation unit so that the float32-output kernels of corr_lookup.hip compile
// exactly as they did without them (co-compiled, six of them
// were allocated two more VGPRs).
#define DXR_TEMPLATES_ONLY
#include "corr_lookup.hip"

int dxr::lookup_out16(const LookupArgs& a) {
  return pyramid_lookup_forms<CELLS_F32_BF16, FORMS_NCHW16>(a);
}
