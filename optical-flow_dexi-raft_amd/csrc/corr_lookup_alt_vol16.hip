// The alternate block's volume lookup on float16 volumes (DXR_ALT_VOL_F16 on the
// `radius` of dxr_alt_volume_lookup, alone or with DXR_OUT_F16 / DXR_OUT_BF16 /
// DXR_OUT_NHWC): the ALT form of corr_lookup.hip's corr_lookup_qm_kernel with the
// cell type _Float16.  Cells are widened to float32 on load (v_cvt_f32_f16, exact;
// the float16 pyramid's loaders) and the float32 arithmetic after that is the
// flagged forms' pinned one, so every output is the float32-volume lookup of the
// widened buffer bit for bit.  Instantiated in this translation unit so that
// every other kernel of corr_lookup.hip compiles exactly as it did without them
// (DESIGN.md §3.11, §3.19).  Defines dxr::alt_volume_lookup_vol16 (dxr_common.h),
// which the entry point calls.
#define DXR_LOOKUP_ALT_VOL16_TU
#include "corr_lookup.hip"
