/*
 * dexiraft_loss.h — C-ABI of the fused sequence loss and flow metrics.
 *
 * Separate from dexiraft_corr.h, dexiraft_flow.h and dexiraft_upsample.h (whose
 * symbol sets and versions are unchanged): prefix dxl_, its own version.  Same
 * conventions: every entry point takes plain device pointers, int64 sizes and a
 * hipStream_t; none allocates, none throws, none synchronises, and each
 * validates its arguments on the host before any launch and returns a
 * dxr_status code of dexiraft_corr.h (DXR_OK, DXR_EINVAL, DXR_EHIP;
 * dxr_last_hip_error() holds the HIP error of a failed launch).  Outputs and
 * workspaces are allocated by the caller.  Functions are reentrant and
 * thread-safe per stream.
 *
 * Reference interfaces replaced (paths relative to the reference repository):
 *   dxl_sequence_loss           train.py:48-73 sequence_loss (the masked L1 terms
 *                               of every prediction, their gamma-weighted sum and
 *                               the end-point-error statistics of the last one),
 *                               and the EPE reductions of evaluate.py:93, 121-128,
 *                               154-169 through `stats`
 *   dxl_sequence_loss_backward  what autograd records for the loss
 */
#ifndef DEXIRAFT_LOSS_H
#define DEXIRAFT_LOSS_H

#include <stdint.h>

#include "dexiraft_corr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DXL_ABI_VERSION 1

/* DXL_ABI_VERSION of the library that was loaded. */
int dxl_abi_version(void);

/*
 * dxl_sequence_loss — train.py:48-73.
 *
 * preds: a host array of P device pointers p_i, each [B, 2, H, W] float32;
 * flow_gt g: [B, 2, H, W] float32; valid: [B, H, W] float32 or null (all valid);
 * all C-contiguous.  Predictions may alias each other.  With M = 2*B*H*W, per
 * pixel in float32, every operation rounded on its own (no fused multiply-add;
 * square root and division correctly rounded):
 *
 *   mag    = sqrt(gx*gx + gy*gy)
 *   v      = (valid >= 0.5) && (mag < max_flow)      max_flow = +inf allowed
 *   d_i    = p_i - g
 *   term_i = (1/M) * sum_{b,c,y,x} v * |d_i|         v multiplied in as 0.0 / 1.0
 *   w_i    = gamma^(P-1-i)                           pow() on the host, double
 *   loss   = sum_i w_i * term_i                      i ascending, float64, rounded
 *                                                    once to float32
 *
 * so a non-finite prediction makes its term and the loss NaN even at an invalid
 * pixel (0 * inf, as the reference's multiplication by the mask does).  The
 * statistics use the last prediction only and select by v:
 *
 *   epe   = sqrt(dx*dx + dy*dy)
 *   stats = [ count(v), sum_v epe, #(epe < 1), #(epe < 3), #(epe < 5),
 *             #(epe > 3 && epe / mag > 0.05) ]       float64[6], counts exact
 *
 * loss: one float32, terms: [P] float32, stats: [6] float64; each may be null,
 * not all three.
 *
 * Two launches.  The first reads every prediction once and flow_gt and valid
 * once per pixel; a thread owns 8 pixels, so a float32 sum is at most 16
 * additions long before it is combined over the wave as a tree and over the
 * workgroup's waves in float64; counts are integers.  Each workgroup writes
 * one float64 partial per term (and the statistics) into `workspace`; the second
 * launch, one workgroup, adds the partials in ascending order in float64.  No
 * atomics: the result is deterministic.  16-byte loads are used when H*W is a
 * multiple of 4 and flow_gt, valid and every prediction are 16-byte aligned,
 * 4-byte loads otherwise, with the same result.
 *
 * `workspace`: 16-byte aligned and at least
 * dxl_sequence_loss_workspace_bytes(P, B, H, W) bytes; its contents on return
 * are unspecified.
 */
int64_t dxl_sequence_loss_workspace_bytes(int64_t P, int64_t B, int64_t H, int64_t W);
int dxl_sequence_loss(const float* const* preds, int64_t P, const float* flow_gt,
                      const float* valid, int64_t B, int64_t H, int64_t W, double gamma,
                      float max_flow, float* loss, float* terms, double* stats, void* workspace,
                      int64_t workspace_bytes, hipStream_t stream);

/*
 * dxl_sequence_loss_backward — the gradients of `loss` in the predictions.
 *
 * grad_loss: one float32 on the device (read by the kernel: no synchronisation).
 * grad_preds: a host array of P device pointers, [B, 2, H, W] float32 each;
 * entries may be null (that gradient is not computed and nothing is written for
 * it), but not all.  Nothing of the forward is kept: v and the sign of d_i are
 * recomputed from preds, flow_gt and valid exactly as the forward computes them.
 *
 *   c_i         = float32(w_i / M)                   host double, rounded once
 *   grad_pred_i = (c_i * grad_loss) * v * sgn(d_i)   float32, sgn(0) = 0
 *
 * so every element is +q_i, -q_i or 0 with q_i = fl(c_i * grad_loss).  No
 * gradient is computed for flow_gt or valid.  Where d_i is not finite the value
 * is unspecified.  No address depends on data.  One launch, no workspace;
 * 16-byte accesses under the rule above (the requested grad_preds included).
 *
 * Both calls.  DXR_EINVAL, answered on the host before any launch: P < 1 or
 * P > 32; B < 0, H < 1 or W < 1; B*H*W > 2^31; then B == 0 is DXR_OK before the
 * pointers are looked at; a NaN or negative gamma, a NaN max_flow; a null
 * required pointer or a null entry of preds; all grad_preds null; loss, terms and
 * stats all null; a workspace that is null, not 16-byte aligned or too short.
 *
 * dxl_sequence_loss_workspace_bytes returns -1 for the P and geometry errors
 * above and 0 for B == 0; it is a multiple of 16 and non-decreasing in each
 * argument.
 */
int dxl_sequence_loss_backward(const float* grad_loss, const float* const* preds,
                               float* const* grad_preds, int64_t P, const float* flow_gt,
                               const float* valid, int64_t B, int64_t H, int64_t W, double gamma,
                               float max_flow, hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DEXIRAFT_LOSS_H */
