/*
 * dexiraft_upsample.h — C-ABI of the convex 8x flow upsampling.
 *
 * Separate from dexiraft_corr.h and dexiraft_flow.h (whose symbol sets and
 * versions are unchanged): prefix dxu_, its own version.  Same conventions:
 * every entry point takes plain device pointers, int64 sizes and a hipStream_t;
 * none allocates, none throws, none synchronises, and each validates its
 * arguments on the host before any launch and returns a dxr_status code of
 * dexiraft_corr.h (DXR_OK, DXR_EINVAL, DXR_EHIP; dxr_last_hip_error() holds the
 * HIP error of a failed launch).  Outputs and workspaces are allocated by the
 * caller.  Functions are reentrant and thread-safe per stream.
 *
 * Reference interfaces replaced (paths relative to the reference repository):
 *   dxu_convex_upsample           core/raft.py:87-98 RAFT.upsample_flow (view,
 *                                 softmax over the 9 taps, F.unfold of 8 * flow,
 *                                 multiply, sum, permute, reshape), called once
 *                                 per iteration at core/raft.py:190
 *   dxu_convex_upsample_backward  what autograd records for those lines
 */
#ifndef DEXIRAFT_UPSAMPLE_H
#define DEXIRAFT_UPSAMPLE_H

#include <stdint.h>

#include "dexiraft_corr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DXU_ABI_VERSION 1

/* Storage type of `mask` (and of `grad_mask`); every other tensor is float32. */
enum dxu_mask_dtype {
  DXU_MASK_F32 = 0,
  DXU_MASK_F16 = 1,
  DXU_MASK_BF16 = 2
};

/* DXU_ABI_VERSION of the library that was loaded. */
int dxu_abi_version(void);

/*
 * dxu_convex_upsample — core/raft.py:87-98.
 *
 * mask: [N, 576, H, W] of mask_dtype, flow: [N, 2, H, W] float32,
 * out: [N, 2, 8H, 8W] float32, all C-contiguous.  Fine pixel (8h+i, 8w+j) of
 * item n and channel c uses x_k = mask[n, 64k + 8i + j, h, w], k = 0..8; tap k
 * points at coarse pixel (h + k/3 - 1, w + k%3 - 1), and a tap outside the map
 * contributes f = 0 (the zero padding of F.unfold):
 *
 *   m = max_k x_k,  e_k = exp(x_k - m),  s = sum_k e_k  (k ascending)
 *   out = (sum_k e_k * (8 * f_{c,k})) * (1 / s)         (k ascending, fused
 *                                                        multiply-adds)
 *
 * in float32 whatever mask_dtype is (16-bit masks are widened on load, which is
 * exact).  A -inf tap among finite ones has weight exactly 0; other non-finite
 * inputs follow IEEE arithmetic.  One launch, no workspace.
 */
int dxu_convex_upsample(const void* mask, int mask_dtype, const float* flow, int64_t N, int64_t H,
                        int64_t W, float* out, hipStream_t stream);

/*
 * dxu_convex_upsample_backward — the gradients of the above.
 *
 * grad_out: [N, 2, 8H, 8W] float32.  grad_mask ([N, 576, H, W] of mask_dtype)
 * and grad_flow ([N, 2, H, W] float32) may each be null (that gradient is then
 * not computed), but not both.  Nothing of the forward is kept: the softmax is
 * recomputed from `mask` exactly as the forward computes it.  With
 * w_k = e_k * (1 / s), g_c = grad_out[n, c, 8h+i, 8w+j] and
 * a_k = g_0 * 8 f_{0,k} + g_1 * 8 f_{1,k}:
 *
 *   grad_mask[n, 64k + 8i + j, h, w] = w_k * (a_k - sum_m w_m a_m)
 *   grad_flow[n, c, h', w'] = 8 * sum w_k g_c over every (h, w, k, i, j) whose
 *                             tap k lands on (h', w')
 *
 * grad_mask is the float32 value rounded once to nearest even in the store.
 * The result is deterministic (no floating-point atomics): the main kernel
 * sums T[n, c, k, h, w] = sum_{i,j} w_k g_c in a fixed order (j within a
 * thread, then i across the workgroup's waves) into `workspace`, and a second
 * launch adds the 9 shifted T planes (k ascending) into grad_flow.  grad_flow
 * does not depend on whether grad_mask is requested.
 *
 * `workspace` is needed only when grad_flow is requested: 16-byte aligned and
 * at least dxu_convex_upsample_backward_workspace_bytes(N, H, W) bytes
 * (18 * N * H * W floats, rounded up to 16); its contents on return are
 * unspecified.
 *
 * Both calls: N == 0 is DXR_OK before the pointers are looked at.  DXR_EINVAL:
 * N < 0, N > 65535, H < 1, W < 1, H*W > 2^22, an unknown mask_dtype, a null
 * required pointer, both gradient pointers null, and, when grad_flow is
 * requested, a workspace that is null, not 16-byte aligned or too short.
 *
 * dxu_convex_upsample_backward_workspace_bytes returns -1 for the geometry
 * errors above, 0 for N == 0; it is a multiple of 16 and non-decreasing in
 * each of N, H and W.
 */
int64_t dxu_convex_upsample_backward_workspace_bytes(int64_t N, int64_t H, int64_t W);
int dxu_convex_upsample_backward(const float* grad_out, const void* mask, int mask_dtype,
                                 const float* flow, int64_t N, int64_t H, int64_t W,
                                 void* grad_mask, float* grad_flow, void* workspace,
                                 int64_t workspace_bytes, hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DEXIRAFT_UPSAMPLE_H */
