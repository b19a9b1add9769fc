// The on-the-fly lookup on float16 feature maps (DXR_ALT_IN_F16 on the `radius`
// of dxr_alt_corr_lookup, dxr_alt_corr_lookup_ws and
// dxr_alt_corr_lookup_levels_ws): alt_corr.hip's alt_corr_mfma_kernel with
// IN16 = true — fmap1 and fmap2 level 0 read as the float16 they are (one f16
// MFMA product per k step, one query plane in LDS, no split), the pooled float32
// levels with two products instead of three — tile order and ordered, radius
// 0..6, with and without the output flags (OUTX).  Instantiated in this
// translation unit so that the float32-operand kernels of alt_corr.hip and
// alt_corr_out.hip compile as they did without them.
#define DXR_TEMPLATES_ONLY
#include "alt_corr.hip"

int dxr::alt_lookup_in16(const AltLookupArgs& a) {
  return alt_lookup_forms<FORMS_ALL, true>(a);
}
