// The on-the-fly lookup's flagged output forms (DXR_OUT_F16 / DXR_OUT_BF16 /
// DXR_OUT_NHWC on the `radius` of dxr_alt_corr_lookup, dxr_alt_corr_lookup_ws and
// dxr_alt_corr_lookup_levels_ws): alt_corr.hip's alt_corr_mfma_kernel with
// OUTX = true, tile order and ordered, radius 0..6; the output dtype and layout
// are a run-time switch in its last phase.  Instantiated in this translation
// unit so that the float32 NCHW kernels of alt_corr.hip compile exactly as they
// did without them.
#define DXR_TEMPLATES_ONLY
#include "alt_corr.hip"

int dxr::alt_lookup_out(const AltLookupArgs& a) {
  return alt_lookup_forms<FORMS_FLAGGED>(a);   // unflagged: alt_corr.hip's
}
