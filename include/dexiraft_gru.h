/*
 * dexiraft_gru.h — C-ABI of the fused SepConvGRU inference forward.
 *
 * Separate from dexiraft_corr.h, dexiraft_flow.h, dexiraft_upsample.h and
 * dexiraft_loss.h (whose symbol sets and versions are unchanged): prefix dxg_,
 * its own version, and its own shared object, libdexiraft_gru.so, so that the
 * export list of libdexiraft_corr.so stays what it was.  Same conventions: every
 * entry point takes plain device pointers, int64 sizes and a hipStream_t; none
 * allocates, none throws, none synchronises, and each validates its arguments on
 * the host before any launch and returns a dxr_status code of dexiraft_corr.h
 * (DXR_OK, DXR_EINVAL, DXR_EUNSUPPORTED, DXR_EHIP; dxr_last_hip_error() holds the
 * HIP error of a failed launch).  Outputs and workspaces are allocated by the
 * caller.  Functions are reentrant and thread-safe per stream.
 *
 * Reference interfaces replaced (paths relative to the reference repository):
 *   dxg_sepconv_pack_weights  the six nn.Conv2d parameters of
 *                             core/update.py:36-42, rearranged once
 *   dxg_sepconv_pack_inputs   the torch.cat([h, x]) of core/update.py:47 (and, under
 *                             autocast, the casts in front of each convolution)
 *   dxg_sepconv_gate_zr       core/update.py:47-49 (axis 0) and :54-56 (axis 1):
 *                             cat, convz, convr, the two sigmoids, and the r*h of
 *                             :50 / :57
 *   dxg_sepconv_gate_qh       core/update.py:50-51 (axis 0) and :57-58 (axis 1):
 *                             cat, convq, tanh and the blend
 *   dxg_sepconv_gru           core/update.py:45-60, SepConvGRU.forward, called at
 *                             core/update.py:131 once per stream and iteration
 *
 * Numerical definition.  c is the compute dtype (float16 or bfloat16), rne_c
 * rounding to nearest even into c.  The state h is float32 between the stages.
 * For axis 0 (taps along W, convz1 / convr1 / convq1), then axis 1 (taps along H,
 * convz2 / convr2 / convq2):
 *   1. hc = rne_c(h), xc = rne_c(x) (once per call), Wc = rne_c(W); biases float32.
 *   2. Pz, Pr = b + sum_{t=0..4} sum_ci Wc[co, ci, t] * [hc | xc][ci, p + t - 2]:
 *      exact products, float32 accumulation in a fixed order (tap-major, then
 *      channels in steps of 16: one MFMA per step, the bias added last).  Taps past
 *      the ends of the row (axis 0) or of the image column (axis 1) read zero.
 *   3. z = sigmoid(Pz), r = sigmoid(Pr) in float32; rh = rne_c(r * h).
 *   4. Pq as 2. on [rh | xc]; q = tanh(Pq); h <- (1 - z) * h + z * q in float32.
 * The output is the final h rounded once to out_dtype, in NCHW.  Non-finite
 * inputs do not fault; the values they produce are unspecified.
 *
 * Geometry: N >= 0, H >= 1, W >= 1, Ch >= 1, Cx >= 1, else DXR_EINVAL.  Supported:
 * Ch % 16 == 0 with 16 <= Ch <= 128, Cx % 16 == 0 with 16 <= Cx <= 256,
 * N <= 65535 and H * W <= 2^22; anything else is DXR_EUNSUPPORTED (there is no
 * fallback).  The byte-size functions return -1 for either kind.
 *
 * Workspace layout (part of this ABI: the stage entry points communicate through
 * it).  With P = N * H * W, in this order and with no padding (every size is a
 * multiple of 32 bytes), all channels-last [N, H, W, C]:
 *   h32  float32 [P, Ch]   the state
 *   hc   c       [P, Ch]   rne_c(h32)
 *   xc   c       [P, Cx]   rne_c(x)
 *   z    float32 [P, Ch]   the update gate of the current axis
 *   rh   c       [P, Ch]   rne_c(r * h32) of the current axis
 * dxg_sepconv_workspace_bytes = P * (12 * Ch + 2 * Cx).  The workspace must be
 * 16-byte aligned.
 */
#ifndef DEXIRAFT_GRU_H
#define DEXIRAFT_GRU_H

#include <stdint.h>

#include "dexiraft_corr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DXG_ABI_VERSION 1

/* Storage types: of h, x and out (any of the three) and the compute dtype c
 * (DXG_F16 or DXG_BF16 only). */
enum dxg_dtype {
  DXG_F32 = 0,
  DXG_F16 = 1,
  DXG_BF16 = 2
};

/* DXG_ABI_VERSION of the library that was loaded. */
int dxg_abi_version(void);

/*
 * dxg_sepconv_pack_weights — the parameters of one axis (core/update.py:36-38 or
 * :40-42) in MFMA operand order.
 *
 * wz, wr, wq: [Ch, Ch + Cx, 5] float32 (nn.Conv2d's [Ch, Ch + Cx, 1, 5] and
 * [Ch, Ch + Cx, 5, 1] are both this, contiguous); bz, br, bq: [Ch] float32; all on
 * the device.  `packed` (16-byte aligned, at least
 * dxg_sepconv_packed_weight_bytes(Ch, Cx) bytes) receives rne_c of the weights,
 * [tap][channel / 16][channel / 8 % 2][output row][8], the z rows then the r rows
 * for the ZR stage and the q rows (zero rows up to a multiple of 32) for the QH
 * stage, then the biases in float32.  One launch.  Pack once per (weights,
 * compute dtype) and reuse.
 */
int64_t dxg_sepconv_packed_weight_bytes(int64_t Ch, int64_t Cx);
int dxg_sepconv_pack_weights(const float* wz, const float* wr, const float* wq, const float* bz,
                             const float* br, const float* bq, int64_t Ch, int64_t Cx,
                             int compute_dtype, void* packed, int64_t packed_bytes,
                             hipStream_t stream);

int64_t dxg_sepconv_workspace_bytes(int64_t N, int64_t H, int64_t W, int64_t Ch, int64_t Cx);

/*
 * dxg_sepconv_pack_inputs — core/update.py:47's cat, as a layout change.
 *
 * h: [N, Ch, H, W] of h_dtype, x: [N, Cx, H, W] of x_dtype, C-contiguous, read in
 * place.  Writes h32 (the widened h, exact), hc = rne_c(h) and xc = rne_c(x) of the
 * workspace.  One launch.
 */
int dxg_sepconv_pack_inputs(const void* h, int h_dtype, const void* x, int x_dtype, int64_t N,
                            int64_t H, int64_t W, int64_t Ch, int64_t Cx, int compute_dtype,
                            void* workspace, int64_t workspace_bytes, hipStream_t stream);

/*
 * dxg_sepconv_gate_zr — core/update.py:47-49 (axis 0), :54-56 (axis 1), and r * h.
 *
 * Reads hc, xc and h32; writes z and rh (steps 2 and 3 above).  `packed` is the
 * packed buffer of that axis.  One launch.
 */
int dxg_sepconv_gate_zr(const void* packed, int axis, int64_t N, int64_t H, int64_t W, int64_t Ch,
                        int64_t Cx, int compute_dtype, void* workspace, int64_t workspace_bytes,
                        hipStream_t stream);

/*
 * dxg_sepconv_gate_qh — core/update.py:50-51 (axis 0), :57-58 (axis 1).
 *
 * Reads rh, xc, z and h32 (step 4 above).  With `out` null it writes the new
 * state to h32 and its rne_c to hc (what axis 1's ZR stage reads); with `out`
 * ([N, Ch, H, W] of out_dtype) it writes the new state there, rounded once, and
 * leaves h32 and hc as they were.  One launch.
 */
int dxg_sepconv_gate_qh(const void* packed, int axis, int64_t N, int64_t H, int64_t W, int64_t Ch,
                        int64_t Cx, int compute_dtype, void* out, int out_dtype, void* workspace,
                        int64_t workspace_bytes, hipStream_t stream);

/*
 * dxg_sepconv_gru — core/update.py:45-60 in five launches: pack_inputs,
 * gate_zr(0), gate_qh(0, out = null), gate_zr(1), gate_qh(1, out).  The result
 * equals those five calls bit for bit.  packed_h / packed_v: the packed buffers of
 * axis 0 (convz1, convr1, convq1) and axis 1 (convz2, convr2, convq2).
 *
 * All calls: N == 0 is DXR_OK before the pointers are looked at.  DXR_EINVAL: the
 * geometry errors above, an unknown dtype, a compute dtype other than DXG_F16 /
 * DXG_BF16, an axis other than 0 / 1, a null required pointer, and a workspace (or
 * `packed` of dxg_sepconv_pack_weights) that is null, not 16-byte aligned or too
 * short.
 */
int dxg_sepconv_gru(const void* h, int h_dtype, const void* x, int x_dtype, const void* packed_h,
                    const void* packed_v, int64_t N, int64_t H, int64_t W, int64_t Ch, int64_t Cx,
                    int compute_dtype, void* out, int out_dtype, void* workspace,
                    int64_t workspace_bytes, hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DEXIRAFT_GRU_H */
