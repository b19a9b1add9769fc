// The alternate block's volume lookup on float16 volumes (DXR_ALT_VOL_F16 on the
// `radius` of dxr_alt_volume_lookup, alone or with DXR_OUT_F16 / DXR_OUT_BF16 /
// DXR_OUT_NHWC): the ALT form of corr_lookup.hip's corr_lookup_qm_kernel with the
// cell type _Float16.  Cells are widened to float32 on load (v_cvt_f32_f16, exact;
// the float16 pyramid's loaders) and the float32 arithmetic after that is the
// flagged forms' pinned one, so every output is the float32-volume lookup of the
// widened buffer bit for bit.  Instantiated in this translation unit so that
// every other kernel of corr_lookup.hip compiles exactly as it did without them
// (DESIGN.md §3.11, §3.19).
#define DXR_TEMPLATES_ONLY
#include "corr_lookup.hip"

int dxr::alt_volume_lookup_vol16(const AltVolumeArgs& a) {
  return alt_volume_lookup_forms<_Float16, FORMS_ALL>(a);
}
