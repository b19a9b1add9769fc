// The alternate block's volume lookup with flagged outputs (DXR_OUT_F16 /
// DXR_OUT_BF16 / DXR_OUT_NHWC on the `radius` of dxr_alt_volume_lookup): the ALT
// form of corr_lookup.hip's corr_lookup_qm_kernel with the 16-bit and channels-
// last stores of the product lookup.  Instantiated in this translation unit so
// that every other kernel of corr_lookup.hip compiles exactly as it did without
// them.
#define DXR_TEMPLATES_ONLY
#include "corr_lookup.hip"

int dxr::alt_volume_lookup_out(const AltVolumeArgs& a) {
  return alt_volume_lookup_forms<float, FORMS_FLAGGED>(a);   // unflagged: corr_lookup.hip's
}
