// The lookup's channels-last output instantiations (DXR_OUT_NHWC of
// dxr_corr_lookup and dxr_corr_lookup_conv1x1: `out` is [B, H, W, C], for every
// pyramid cell type and every output type).  The kernels are corr_lookup.hip's
// templates with NHWC = true: the same sums, stored along channels.  They are
// instantiated in this translation unit so that the NCHW kernels of
// corr_lookup.hip, corr_lookup_out16.hip and corr_lookup_pyr16.hip compile
// exactly as they did without them.
#define DXR_TEMPLATES_ONLY
#include "corr_lookup.hip"

int dxr::lookup_nhwc(const LookupArgs& a) {
  return pyramid_lookup_forms<CELLS_ALL, FORMS_NHWC>(a);
}
