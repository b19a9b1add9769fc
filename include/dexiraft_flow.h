/*
 * dexiraft_flow.h — C-ABI of the flow helpers around the correlation subsystem.
 *
 * Separate from dexiraft_corr.h (whose symbol set and DXR_ABI_VERSION are
 * unchanged): prefix dxf_, its own version.  Same conventions: every entry
 * point takes plain device pointers, int64 sizes and a hipStream_t; none
 * allocates, none throws, none synchronises, and each validates its arguments
 * on the host before any launch and returns a dxr_status code of
 * dexiraft_corr.h (DXR_OK, DXR_EINVAL, DXR_EHIP; dxr_last_hip_error() holds the
 * HIP error of a failed launch).  Outputs and workspaces are allocated by the
 * caller.  Functions are reentrant and thread-safe per stream.
 *
 * Reference interfaces replaced (paths relative to the reference repository):
 *   dxf_forward_interpolate  core/utils/utils.py:26-54 forward_interpolate
 *                            (device-to-host copy, two scipy
 *                            interpolate.griddata(method='nearest') calls, copy
 *                            back), as the warm start of evaluate.py:33-50 uses
 *                            it for flow_init (core/raft.py:165-166)
 */
#ifndef DEXIRAFT_FLOW_H
#define DEXIRAFT_FLOW_H

#include <stdint.h>

#include "dexiraft_corr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DXF_ABI_VERSION 1

/* DXF_ABI_VERSION of the library that was loaded. */
int dxf_abi_version(void);

/*
 * dxf_forward_interpolate — core/utils/utils.py:26-54.
 *
 * flow, out: [B, 2, H, W] float32, C-contiguous; channel 0 = dx, 1 = dy.  Each
 * of the B items is answered on its own:
 *
 *   Source position.  Source pixel i = y0*W + x0 lands at
 *     x1 = (double)x0 + (double)dx[i],  y1 = (double)y0 + (double)dy[i]
 *   (one float64 addition each: numpy's int64 + float32 promotion, utils.py:33-34).
 *   Validity.  A source is valid iff x1 > 0 && x1 < W && y1 > 0 && y1 < H, all
 *   strict (utils.py:41).  NaN and +-inf flows fail the comparisons and drop out.
 *   Nearest source.  Grid point (gx, gy) takes the (dx, dy) of the valid source
 *   that minimises
 *     d2 = fl(fl(ex*ex) + fl(ey*ey)),  ex = gx - x1,  ey = gy - y1
 *   in float64, every operation rounded on its own (no fused multiply-add), so a
 *   float64 oracle without contraction reproduces d2 bit for bit.
 *   Ties.  Among equal d2 the lowest flat source index i wins.  (scipy's KD-tree
 *   leaves ties unspecified; this rule makes the result deterministic.)
 *   Output bits.  The two float32 values are copied, not recomputed: -0.0 stays
 *   -0.0.
 *   No valid source.  The item's output is all zeros.  This is the one deliberate
 *   difference: the reference raises inside scipy here.
 *
 * The search is exhaustive (H*W sources for each of the H*W grid points), spread
 * over grid-point tiles x source slices x items; `workspace` holds the landing
 * positions and one (d2, index) partial per grid point and slice.  It must be
 * 16-byte aligned and at least dxf_forward_interpolate_workspace_bytes(B, H, W)
 * bytes; its contents on return are unspecified.
 *
 * B == 0 is DXR_OK before the pointers are looked at.  DXR_EINVAL: B < 0,
 * B > 65535, H < 1, W < 1, H*W > 2^22, a null flow / out, a workspace that is
 * null, not 16-byte aligned or shorter than required.
 *
 * dxf_forward_interpolate_workspace_bytes returns -1 for the geometry errors
 * above, 0 for B == 0; it is non-decreasing in each of B, H and W.
 */
int64_t dxf_forward_interpolate_workspace_bytes(int64_t B, int64_t H, int64_t W);
int dxf_forward_interpolate(const float* flow, int64_t B, int64_t H, int64_t W, float* out,
                            void* workspace, int64_t workspace_bytes, hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DEXIRAFT_FLOW_H */
