// The on-the-fly lookup on bfloat16 feature maps (DXR_ALT_IN_BF16 on the `radius`
// of dxr_alt_corr_lookup, dxr_alt_corr_lookup_ws and
// dxr_alt_corr_lookup_levels_ws): alt_corr.hip's alt_corr_mfma_kernel with
// IN16 = INBF = true — fmap1 and fmap2 level 0 read as the bfloat16 they are (one
// bf16 MFMA product per k step, one query plane in LDS, no split, no fallback),
// the pooled float32 levels with three exact bf16 products (the cell split three
// ways, times the raw query) — tile order and ordered, radius 0..6, with and
// without the output flags (OUTX).  Instantiated in this translation unit so that
// the float32- and float16-operand kernels of alt_corr.hip, alt_corr_out.hip and
// alt_corr_in16.hip compile as they did without them.
#define DXR_TEMPLATES_ONLY
#include "alt_corr.hip"

int dxr::alt_lookup_inbf16(const AltLookupArgs& a) {
  return alt_lookup_forms<FORMS_ALL, true, true>(a);
}
