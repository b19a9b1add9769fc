// The lookup's float16-pyramid instantiations (pyr_dtype DXR_PYR_F16 of
// dxr_corr_lookup and dxr_corr_lookup_conv1x1, with float32, float16 and bfloat16
// outputs).  The kernels are corr_lookup.hip's templates with the cell type
// _Float16: cells are widened to float32 on load (v_cvt_f32_f16, exact) and the
// float32 arithmetic after that is shared.  They are instantiated in this
// translation unit so that the float32 / bfloat16 pyramid kernels of
// corr_lookup.hip and corr_lookup_out16.hip compile exactly as they did without
// them.
#define DXR_TEMPLATES_ONLY
#include "corr_lookup.hip"

int dxr::lookup_pyr16(const LookupArgs& a) {
  return pyramid_lookup_forms<CELLS_F16, FORMS_NCHW>(a);
}
