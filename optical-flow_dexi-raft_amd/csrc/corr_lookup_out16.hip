// The lookup's 16-bit output instantiations (float16 / bfloat16 stores:
// DXR_OUT_F16 / DXR_OUT_BF16 of dxr_corr_lookup and dxr_corr_lookup_conv1x1).
// The kernels are corr_lookup.hip's templates; they are instantiated in this
// translation unit so that the float32-output kernels of corr_lookup.hip compile
// exactly as they did without them (co-compiled, six of them
// were allocated two more VGPRs).  Defines dxr::lookup_out16 and
// dxr::lookup_conv1x1_out16 (dxr_common.h), which the entry points call.
#define DXR_LOOKUP_OUT16_TU
#include "corr_lookup.hip"
