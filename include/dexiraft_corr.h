/*
 * dexiraft_corr.h — C-ABI of the MI355X-native RAFT correlation subsystem.
 *
 * This is the drop-in boundary for the hot path named in BASELINE.json
 * (`north_star`): RAFT's correlation block as used by Dexi+RAFT.  Every entry
 * point takes plain device pointers, int64 sizes and a hipStream_t; none
 * allocates, none throws, and each returns a status code (0 = ok, >0 = invalid
 * argument / unsupported, <0 = HIP launch error).  Outputs and workspaces are
 * allocated by the caller (the Python shell allocates them from torch's caching
 * allocator).  Functions are reentrant and thread-safe per stream.
 *
 * Reference interfaces replaced (paths relative to the reference repository):
 *   dxr_corr_pyramid_build   core/corr.py:13-27  CorrBlock.__init__ (matmul,
 *                            / sqrt(D), 3x F.avg_pool2d); NCHW or channels-last
 *                            fmaps (core/extractor.py:166-192 -> core/raft.py:139-148)
 *   dxr_corr_volume          core/corr.py:52-60  CorrBlock.corr (static)
 *   dxr_pyramid_unpack/pack  core/corr.py:16,24,27 the corr_pyramid attribute
 *                            (reference layout <-> paged storage)
 *   dxr_corr_lookup          core/corr.py:29-50  CorrBlock.__call__ together with
 *                            core/utils/utils.py:57-71 bilinear_sampler
 *                            (F.grid_sample, align_corners=True, zero padding)
 *   dxr_corr_lookup_backward core/utils/utils.py:65 grid_sample backward
 *                            (autograd of CorrBlock.__call__, train.py:175-178);
 *                            _multi: several lookups' backwards in one launch
 *   dxr_pyramid_backward     core/corr.py:25-27,58-60 avg_pool2d + division
 *                            backward (autograd of CorrBlock.__init__)
 *   dxr_fmap_grads           core/corr.py:13-27,52-60 the whole CorrBlock.__init__
 *                            backward (pooling + division + matmul) to d fmap1/2
 *   dxr_avg_pool2x2          core/corr.py:69-71  F.avg_pool2d(fmap, 2, stride=2)
 *                            in AlternateCorrBlock.__init__
 *   dxr_avg_pool2x2_nhwc     core/corr.py:70-71 the same pool on channels-last fmaps
 *   dxr_transpose            core/corr.py:82-83 fmap.permute(0, 2, 3, 1).contiguous()
 *                            (NCHW <-> NHWC)
 *   dxr_alt_corr_forward     alt_cuda_corr/correlation.cpp:23-33 `forward`
 *                            (alt_cuda_corr/correlation_kernel.cu:260-286)
 *   dxr_alt_corr_backward    alt_cuda_corr/correlation.cpp:36-48 `backward`
 *                            (alt_cuda_corr/correlation_kernel.cu:288-320)
 *   dxr_alt_corr_lookup      core/corr.py:74-91  AlternateCorrBlock.__call__
 *   dxr_alt_corr_lookup_ws   the same, queries ordered by window position first
 *                            (all levels in one launch, / sqrt(D) fused)
 *   dxr_corr_lookup_conv1x1  core/corr.py:29-50 CorrBlock.__call__ followed by
 *                            core/update.py:90 F.relu(self.convc1(corr))
 *                            (BasicMotionEncoder; :71 SmallMotionEncoder)
 *   dxr_conv1x1_pack_weight  core/update.py:83 / :66 the convc1 weight,
 *                            rearranged once into the fused kernel's operand layout
 *
 * Layouts (all row-major, C-contiguous):
 *   fmap (CorrBlock)        [B, D, H, W]               (NCHW, as core/raft.py:139-142)
 *                           or [B, H, W, D] (DXR_NHWC)
 *   pyramid                 PAGED storage (opaque to callers; sizes and level
 *                           offsets from dxr_pyramid_numel/_level_offset).  Level l
 *                           has H_l = floor(H_{l-1}/2) rows, as F.avg_pool2d.  Levels
 *                           0..3 are split into pages of 128 query pixels x one
 *                           (8x16 >> l) tile of image-2 cells, each page contiguous
 *                           and written by one build workgroup; levels >= 4 are
 *                           row-major.  dxr_pyramid_unpack converts a level to the
 *                           reference's corr_pyramid[l] layout [B*H*W, H_l, W_l].
 *   coords                  [B, 2, H, W] float32       channel 0 = x, 1 = y
 *                           (core/utils/utils.py:74-77)
 *   lookup output           [B, L*(2r+1)^2, H, W] float32, channel
 *                           l*(2r+1)^2 + ix*(2r+1) + iy, x offset = ix - r
 *                           (x-major, core/corr.py:37-46)
 *   alt fmaps               [B, H, W, C]               (NHWC, core/corr.py:82-83)
 *   alt coords              [B, Nc, H1, W1, 2]
 *   alt output              [B, Nc, (2r+1)^2, H1, W1]  channel iy + (2r+1)*ix
 *                           (alt_cuda_corr/correlation_kernel.cu:92-95)
 */
#ifndef DEXIRAFT_CORR_H
#define DEXIRAFT_CORR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* HIP's own definition; repeating an identical typedef is legal in C11/C++. */
typedef struct ihipStream_t* hipStream_t;

#define DXR_ABI_VERSION 10

enum dxr_status {
  DXR_OK = 0,
  DXR_EINVAL = 1,        /* bad pointer / shape / radius / level count   */
  DXR_EUNSUPPORTED = 2,  /* valid request this build does not implement  */
  DXR_EHIP = -1          /* a HIP launch failed; see dxr_last_hip_error() */
};

enum dxr_dtype {
  DXR_F32 = 0,
  DXR_BF16 = 1,         /* storage as IEEE bfloat16 bit patterns (uint16) */
  DXR_F16 = 2,          /* IEEE float16 fmaps: an in_dtype of the pyramid builds only */
  /*
   * IEEE float16 pyramid storage: a pyr_dtype only (never an in_dtype), of
   * dxr_corr_pyramid_build / _build_ws, dxr_pyramid_unpack / _pack,
   * dxr_corr_lookup and dxr_corr_lookup_conv1x1.  Every stored cell of every
   * level is the DXR_F32 pyramid's cell for the same fmaps, rounded once to
   * float16 with round-to-nearest-even (overflow to +-inf, subnormals kept, NaN
   * stays NaN): torch's .half() of the float32 pyramid, bit for bit.  Pooled
   * levels are computed from the float32 values of the level above and rounded
   * once.  Lookups widen the cells on load (exact) and run the float32
   * arithmetic unchanged.  Every other entry point that takes a dtype rejects it
   * as it rejects an unknown one.
   */
  DXR_PYR_F16 = 4
};

/*
 * Output dtype flags of dxr_corr_lookup and dxr_corr_lookup_conv1x1: or-ed
 * onto their pyr_dtype argument (DXR_F32, DXR_BF16 or DXR_PYR_F16), they make the
 * call store `out` as IEEE float16 / bfloat16 elements instead of float32 (same
 * ABI, no new entry point).  Both flags together, any other bit above the low
 * byte, a flag on any other low value (DXR_F16 included) and a flag passed to any
 * other entry point are DXR_EINVAL, answered on the host before any launch.
 * The alternate block's lookups (dxr_alt_corr_lookup, dxr_alt_corr_lookup_ws,
 * dxr_alt_corr_lookup_levels_ws, dxr_alt_volume_lookup) have no pyr_dtype and
 * take the same flags, with the same meaning, on their `radius` argument: see
 * "Output flags on radius" at dxr_alt_corr_lookup.
 */
#define DXR_OUT_F16 0x100
#define DXR_OUT_BF16 0x200

/*
 * Output layout flag of the same two entry points, or-ed onto pyr_dtype alone or
 * together with exactly one of the dtype flags above (low byte DXR_F32, DXR_BF16
 * or DXR_PYR_F16): `out` is channels-last, [B, H, W, C] instead of [B, C, H, W]
 * (C = num_levels*(2r+1)^2 for dxr_corr_lookup, cout for
 * dxr_corr_lookup_conv1x1).  Element (b, c, h, w) of the unflagged call lands at
 * ((b*H + h)*W + w)*C + c and is that call's element with the same dtype flag,
 * bit for bit (NaN levels, far and non-finite coordinates, float16 overflow to
 * +-inf included): only the address changes.  `out` needs the element's own
 * alignment (4 bytes for float32, 2 for the 16-bit types) and no byte outside
 * the B*H*W*C elements is written.  The flag with both dtype flags, with any
 * other bit above the low byte, on any other low value (DXR_F16 included) or on
 * any other entry point is DXR_EINVAL, answered on the host before any launch.
 * (The fmap layout DXR_NHWC of enum dxr_layout below is an input layout of the
 * builds and unrelated to this flag.)  The alternate block's four lookups take it
 * on `radius` ("Output flags on radius" at dxr_alt_corr_lookup).
 */
#define DXR_OUT_NHWC 0x1000

/*
 * Accumulate flag of dxr_alt_corr_backward, or-ed onto its `radius` argument
 * (the low byte is the radius): the gradients are added into fmap1_grad and
 * fmap2_grad by the matrix-core kernel instead of overwriting them.  Semantics,
 * served shapes and validation: at dxr_alt_corr_backward.  On any other entry
 * point the bit is an unknown flag.
 */
#define DXR_ALT_BWD_ACCUMULATE 0x2000

/*
 * Input dtype flag of dxr_alt_corr_lookup, dxr_alt_corr_lookup_ws and
 * dxr_alt_corr_lookup_levels_ws, or-ed onto their `radius` argument (the low
 * byte is the radius), alone or with the output flags: fmap1 and fmap2 level 0
 * are read as the float16 maps a mixed-precision encoder emits
 * (core/raft.py:139-142 widens them first), without a float32 copy.  Semantics,
 * served shapes and validation: "Float16 fmaps on radius" at
 * dxr_alt_corr_lookup.  On any other entry point the bit is an unknown flag.
 */
#define DXR_ALT_IN_F16 0x8000

/*
 * The same for bfloat16 maps, the usual autocast dtype: fmap1 and fmap2 level 0
 * are read as bfloat16, without a float32 copy.  One input flag at a time: both
 * together are DXR_EINVAL.  Semantics, served shapes and validation: "Bfloat16
 * fmaps on radius" at dxr_alt_corr_lookup.  On any other entry point the bit is
 * an unknown flag.
 */
#define DXR_ALT_IN_BF16 0x20000

/*
 * Cell type flag of the alternate block's coarse volumes: or-ed onto the
 * `first_level` argument of dxr_alt_coarse_volumes / dxr_alt_coarse_volumes_ws
 * (the low byte is the level), `volumes` holds IEEE float16 cells, stored by the
 * volume GEMM itself; or-ed onto the `radius` of dxr_alt_volume_lookup, alone or
 * with the output flags, the lookup reads such cells.  Semantics, served shapes
 * and validation: "Float16 volumes" at dxr_alt_volume_numel.  On any other entry
 * point the bit is an unknown flag.
 */
#define DXR_ALT_VOL_F16 0x40000

enum dxr_layout {
  DXR_NCHW = 0,         /* fmaps [B, D, H, W] (core/raft.py:139-142)              */
  DXR_NHWC = 1          /* fmaps [B, H, W, D] (channels-last encoders, §8(f) row 4) */
};

enum dxr_build_algo {
  DXR_BUILD_AUTO = 0,       /* f32 fmaps: split build where its layout allows  */
  DXR_BUILD_EXACT_F32 = 1   /* f32 fmaps: exact-f32 MFMA build (v_mfma_f32_32x32x2_f32) */
};

/* ABI version of the loaded library (== DXR_ABI_VERSION it was built with). */
int dxr_abi_version(void);

/* Human-readable name of a dxr_status value. */
const char* dxr_status_string(int status);

/* hipError_t of the most recent failed launch on the calling thread. */
int dxr_last_hip_error(void);

/* Elements (not bytes) of a num_levels pyramid for B pairs of H x W fmaps. */
int64_t dxr_pyramid_numel(int64_t B, int64_t H, int64_t W, int num_levels);

/* Element offset of level `level` inside that pyramid buffer. */
int64_t dxr_pyramid_level_offset(int64_t B, int64_t H, int64_t W, int level);

/*
 * Stage (a)+(b): all-pairs correlation fmap1^T . fmap2 / divisor and its
 * avg-pool pyramid, written in one pass (pooling fused into the MFMA epilogue).
 *   fmap1, fmap2 : [B, D, H, W] (fmap_layout DXR_NCHW) or [B, H, W, D]
 *                  (DXR_NHWC), dtype in_dtype (DXR_F32, DXR_BF16 or DXR_F16)
 *   divisor      : the reference divides by sqrt(D) (core/corr.py:60)
 *   pyramid      : dxr_pyramid_numel(B,H,W,num_levels) elements of pyr_dtype
 *                  (levels beyond 4 need pyr_dtype DXR_F32)
 *   num_levels   : >= 1; every level must be at least 1 x 1
 *   algo         : DXR_BUILD_AUTO, or DXR_BUILD_EXACT_F32 (f32 fmaps only)
 * DXR_F32 inputs compute in f32 class: every f32 operand is split into an f16
 * pair x = hi + 2^-11 lo and three f16 x f16 MFMA products per f32 product are
 * accumulated in two f32 accumulators (the lo*lo term, <= 2^-22 |x y|, dropped);
 * a page whose sums are not finite (an operand beyond the f16 range, or inf/NaN)
 * is recomputed on an exact three-way bf16 split (six products).  The pair is
 * unscaled here: where |x| < 2^-14, hi falls on f16's subnormal grid and the
 * pair's error stays ~2^-36 absolute, so relative accuracy drops for tiny fmaps
 * (~1e-4 at |x| ~ 1e-7); dxr_corr_pyramid_build_ws (per-pixel power-of-two
 * scaling, what CorrBlock calls) has no such bound.  With
 * D % 16 != 0, odd W or DXR_BUILD_EXACT_F32 the exact-f32 MFMA
 * v_mfma_f32_32x32x2_f32 is used.  Pyramid stores are write-through (sc1).
 * DXR_BF16 inputs use bf16 MFMA with f32 accumulation.  NHWC and NCHW inputs
 * of the same values give bit-identical pyramids.
 * DXR_F16 inputs (float16 fmaps, what autocast encoders emit under
 * --mixed_precision) run the LDS-DMA build on f16 records: one
 * v_mfma_f32_32x32x16_f16 product per channel pair, f32 accumulation, no
 * scales, into a DXR_F32 pyramid.  Every f16 is an f32 and f16 x f16 products
 * are exact in f32, so the result is the f32 matmul of the widened fmaps to
 * accumulation rounding (f32 class; inf/NaN propagate through the MFMA).  It
 * needs D % 32 == 0, D * H * W < 2^30, a 16-byte aligned pyramid and either
 * channels-last fmaps with 16-byte aligned pixel rows or, for NCHW fmaps, the
 * workspace of dxr_corr_pyramid_build_ws; every other valid DXR_F16 request
 * (also a DXR_BF16 pyramid and DXR_BUILD_EXACT_F32) returns DXR_EUNSUPPORTED
 * and the caller widens the fmaps to f32.  DXR_F16 is no pyr_dtype, and no
 * dtype of any other entry point (dxr_corr_volume: DXR_EUNSUPPORTED;
 * dxr_transpose moves f16 fmaps as DXR_BF16, any 16-bit pattern).
 * pyr_dtype DXR_PYR_F16 (a float16 pyramid: the DXR_F32 pyramid of the same
 * request, each cell rounded once to float16, RNE, in the epilogue's own 16-byte
 * stores) is built by the two LDS-DMA builds only: DXR_F16 fmaps under the
 * conditions above, and DXR_F32 fmaps with a workspace, DXR_BUILD_AUTO and
 * D % 16 == 0 (the pre-split build of dxr_corr_pyramid_build_ws).  Every other
 * valid request for it (DXR_BF16 fmaps, no or a short workspace for f32 / NCHW
 * f16 fmaps, DXR_BUILD_EXACT_F32, D % 16 != 0, more than 4 levels) returns
 * DXR_EUNSUPPORTED before any launch; such a pyramid can be made from a DXR_F32
 * one, level by level, with dxr_pyramid_unpack + dxr_pyramid_pack.
 *
 * Kernels by request (both build entry points).  csrc/build_plan.h is this
 * table's implementation: its plan_build() answers every refusal and names the
 * kernel before anything is launched, and tests/test_build_plan.py checks it
 * against these rows one by one on a CPU (tests/test_gpu_parity.py
 * test_build_kernel_by_request runs the kernels against the oracle).
 * First, for every request: invalid arguments are DXR_EINVAL (B == 0 is DXR_OK
 * before the pointers are looked at); more than 4 levels with a pyramid that is
 * not DXR_F32, and DXR_BUILD_EXACT_F32 with fmaps that are not f32, are
 * DXR_EUNSUPPORTED.  Then the first row that matches, top to bottom.
 * "workspace": non-null, 16-byte aligned and at least dxr_build_workspace_bytes
 * (anything less counts as none); "aligned": 16-byte aligned.
 *   f16 fmaps, f32 or float16 pyramid, D % 32 == 0, D*H*W < 2^30, pyramid aligned:
 *     NHWC, fmaps aligned               corr_build_dma_kernel (rows read in place)
 *     NCHW, workspace                   pack_bf16_kernel + corr_build_dma_kernel
 *   f16 fmaps otherwise                 none: DXR_EUNSUPPORTED
 *   f32, workspace, AUTO, D % 16 == 0, D*H*W < 2^29, pyramid aligned (CorrBlock's path):
 *     NCHW                              split_pairs_kernel<NCHW> + corr_build_dma_kernel
 *     NHWC, fmaps aligned               split_pairs_kernel<NHWC> + corr_build_dma_kernel
 *   float16 pyramid otherwise           none: DXR_EUNSUPPORTED
 *   bf16 NCHW, workspace, D % 32 == 0, D*H*W < 2^30, pyramid aligned, <= 4 levels
 *                                       pack_bf16_kernel + corr_build_dma_kernel
 *   bf16 NHWC, D % 32 == 0, D*H*W < 2^30, fmaps and pyramid aligned
 *                                       corr_build_dma_kernel (rows read in place)
 *   bf16 NHWC otherwise                 none: DXR_EUNSUPPORTED
 *   f32 NHWC, AUTO, D % 16 == 0, D*H*W < 2^29, even W, fmaps and pyramid aligned
 *                                       corr_build_split_kernel<NHWC>
 *   f32 NHWC otherwise                  none: DXR_EUNSUPPORTED
 *   f32 NCHW, AUTO, D % 16 == 0, D*H*W < 2^29 (round-2 register split; the
 *   documented fallback for callers that cannot provide a workspace):
 *     W % 4 == 0, fmaps and pyramid aligned
 *                                       corr_build_split_kernel<float4>
 *     even W, fmaps 8-byte aligned, pyramid aligned
 *                                       corr_build_split_kernel<float2>
 *   f32 NCHW otherwise (EXACT_F32, D % 16 != 0, odd W, alignment; exact-f32 MFMA):
 *     W % 4 == 0, fmaps and pyramid aligned
 *                                       corr_build_f32_kernel<vec>
 *     else                              corr_build_f32_kernel<scalar>
 *   bf16 NCHW, W % 4 == 0, fmaps 8-byte aligned, pyramid aligned, D*H*W < 2^30
 *                                       corr_build_bf16_q2_kernel
 *   bf16 NCHW otherwise                 corr_build_bf16_kernel (one query block)
 * Last: every kernel but the two 16-bit corr_build_dma_kernel rows (1-D grids)
 * runs on a grid with ceil(H*W / 128) rows; more than 65535 are DXR_EINVAL.
 * Levels beyond 4 follow as f32 pooling passes.
 */
int dxr_corr_pyramid_build(const void* fmap1, const void* fmap2, int in_dtype,
                           int fmap_layout, int64_t B, int64_t D, int64_t H,
                           int64_t W, int num_levels, float divisor,
                           void* pyramid, int pyr_dtype, int algo,
                           hipStream_t stream);

/*
 * Bytes of device workspace dxr_corr_pyramid_build_ws uses for B pairs of
 * D x H x W fmaps of in_dtype (0: that request needs none; -1: bad geometry):
 * f32 with D % 16 == 0 the pre-split operands, bf16 with D % 32 == 0 the pack
 * pass's blocked copies of NCHW fmaps (channels-last bf16 fmaps need none);
 * f16 as bf16 (the same 16-bit pack pass).  A size beyond int64 is -1 too
 * (only with B > 65535 or D*H*W >= 2^30, where no build takes a workspace).
 * ABI 6.
 */
int64_t dxr_build_workspace_bytes(int in_dtype, int64_t B, int64_t D, int64_t H,
                                  int64_t W);

/*
 * dxr_corr_pyramid_build with a caller-owned workspace (16-byte aligned, at
 * least dxr_build_workspace_bytes; contents need no initialisation and are
 * dead after the build).  Same arguments, same result contract; with DXR_F32
 * fmaps, algo DXR_BUILD_AUTO and D % 16 == 0 it runs the pre-split build:
 * one pass scales every pixel's channel vector by a power of two 2^s
 * (|x 2^s| < 2^14) and splits it into an f16 pair x 2^s = hi + lo
 * (lo = RNE_f16(x 2^s - hi)) in the workspace, then the build's K loop moves
 * those pairs by LDS-DMA and runs three f16 MFMA products per f32 product
 * (lo.hi + hi.lo + hi.hi into one f32 accumulator), undoing both scales
 * exactly in its epilogue — f32-class error (the pair holds each element to
 * <= 2^-23 |x| unless it is more than 2^16 below its pixel's max) at any fmap
 * scale, bit-identical for NCHW and NHWC fmaps and exactly linear in
 * power-of-two scalings of either fmap.  A workgroup whose sums are not
 * finite (an inf/NaN operand) rewrites its pages from the f32 operands on the
 * exact-f32 MFMA (IEEE inf/NaN semantics).  NHWC fmaps need 16-byte aligned
 * pixel rows.  With DXR_BF16 NCHW fmaps (D % 32 == 0) a pack pass copies the
 * operands into 64-byte records of 32 channels per pixel and the bf16 build
 * runs the same LDS-DMA K loop on them — the workspace-less bf16 build's
 * pyramid bit for bit; DXR_F16 NCHW fmaps take the same pack pass and the f16
 * record build (above).  A NULL or short workspace runs dxr_corr_pyramid_build.
 * Replaces the same reference lines: core/corr.py:52-60 + :21-27.  ABI 6.
 */
int dxr_corr_pyramid_build_ws(const void* fmap1, const void* fmap2, int in_dtype,
                              int fmap_layout, int64_t B, int64_t D, int64_t H,
                              int64_t W, int num_levels, float divisor,
                              void* pyramid, int pyr_dtype, int algo,
                              void* workspace, int64_t workspace_bytes,
                              hipStream_t stream);

/*
 * CorrBlock.corr: the level-0 volume alone, row-major [B, H, W, 1, H, W]
 * (= [B*H*W, H, W]) float32, divided by `divisor`.
 */
int dxr_corr_volume(const void* fmap1, const void* fmap2, int in_dtype,
                    int64_t B, int64_t D, int64_t H, int64_t W, float divisor,
                    float* out, hipStream_t stream);

/*
 * Convert one level between the paged pyramid and the reference layout
 * [B*H*W, H_l, W_l] float32 (core/corr.py:22-27).  Padding cells of the paged
 * storage are neither read nor written.  pyr_dtype DXR_F32, DXR_BF16 or
 * DXR_PYR_F16: unpack widens 16-bit cells exactly, pack rounds float32 to the
 * pyramid's type to nearest even (float16: overflow to +-inf, subnormals kept).
 */
int dxr_pyramid_unpack(const void* pyramid, int pyr_dtype, int64_t B, int64_t H,
                       int64_t W, int num_levels, int level, float* out,
                       hipStream_t stream);
int dxr_pyramid_pack(const float* level_data, int64_t B, int64_t H, int64_t W,
                     int num_levels, int level, void* pyramid, int pyr_dtype,
                     hipStream_t stream);

/*
 * Stage (c): radius-r bilinear lookup of every level around coords / 2^l.
 *   pyramid : as produced by dxr_corr_pyramid_build
 *   coords  : [B, 2, H, W] float32
 *   out     : [B, num_levels*(2r+1)^2, H, W] float32
 * A level with H_l == 1 or W_l == 1 yields NaN, as the reference does
 * (bilinear_sampler divides by H_l-1 / W_l-1, core/utils/utils.py:61-62).
 * A DXR_PYR_F16 pyramid's cells are widened to float32 on load (exact), so the
 * result is the float32 lookup of the widened pyramid bit for bit; a cell that
 * overflowed to +-inf in the pyramid gives inf / NaN in the outputs that tap it.
 * pyr_dtype | DXR_OUT_F16 or pyr_dtype | DXR_OUT_BF16: `out` points to
 * [B, num_levels*(2r+1)^2, H, W] float16 / bfloat16 elements (passed through the
 * float* parameter) and needs 2-byte alignment only.  Every element is the
 * float32 call's, converted round-to-nearest-even in the store (float16: overflow
 * to +-inf, subnormals kept; NaN stays NaN): torch's out.to(dtype) bit for bit.
 * No byte outside the elements is written.
 * pyr_dtype | DXR_OUT_NHWC (alone or with one dtype flag): `out` is
 * [B, H, W, num_levels*(2r+1)^2], the same elements bit for bit at
 * ((b*H + h)*W + w)*C + c (see DXR_OUT_NHWC), all radii and level counts.
 *
 * Lookup kernels by request (the forward lookups: dxr_corr_lookup,
 * dxr_corr_lookup_conv1x1, dxr_alt_volume_lookup, dxr_alt_corr_lookup / _ws /
 * _levels_ws).  csrc/lookup_plan.h is this table's implementation: its
 * plan_lookup(), plan_volume_lookup() and plan_alt_lookup() answer every refusal
 * and name the translation unit, the kernel, its grid and its store policy
 * before anything is launched, and tests/test_lookup_plan.py checks them against
 * these rows one by one on a CPU.  For every request the checks run in the
 * order written below (a request that is wrong in two ways answers the first),
 * and B == 0 is DXR_OK before the pointers are looked at.  N = H*W;
 * "flagged": any of DXR_OUT_F16 / DXR_OUT_BF16 / DXR_OUT_NHWC.
 *
 * Pyramid lookup (dxr_corr_lookup; dxr_corr_lookup_conv1x1 below).  Checks: the
 * flags on pyr_dtype (both dtype flags, another high bit, a flag on a low value
 * that is no cell type, a 16-bit `out` at an odd address: DXR_EINVAL); levels
 * (1..8, every level >= 1 x 1, H*W <= 2^30), radius >= 0 and cout >= 1:
 * DXR_EINVAL; radius > 8 (fused: radius not 3 or 4, more than 4 levels, cout
 * % 32 != 0, cout > 4096): DXR_EUNSUPPORTED; B > 65535: DXR_EINVAL; B == 0:
 * DXR_OK; a null pointer, then an unknown unflagged cell type: DXR_EINVAL.
 *   unit, by the first that matches:
 *     DXR_OUT_NHWC                      corr_lookup_nhwc.hip
 *     DXR_PYR_F16 cells                 corr_lookup_pyr16.hip
 *     DXR_OUT_F16 / DXR_OUT_BF16        corr_lookup_out16.hip
 *     else                              corr_lookup.hip
 *   kernel, grid (x, y, z) and NCHW store policy, in every unit.  wg32 =
 *   ceil(N / QB) * levels * B with QB = 32 (r <= 4) or 16 (r > 4); "large
 *   misaligned": N % 32 != 0 and B * (level-0 cells per pair, pages padded) *
 *   cell bytes * 4/3 >= 128 MiB:
 *     r <= 4, wg32 <= 1024, not large misaligned (one round):
 *                                       corr_lookup_qm_kernel<256 x 16>
 *                                       (ceil(N/16), levels, B); non-temporal
 *                                       stores if N % 32 == 0, else write-through
 *     else, r <= 4                      corr_lookup_qm_kernel<512 x 32>
 *                                       (ceil(N/32), levels, B); non-temporal
 *     else, r > 4                       corr_lookup_qm_kernel<512 x 16>
 *                                       (ceil(N/16), levels, B); non-temporal
 *     (channels-last outputs: non-temporal stores in every shape, at compile time)
 *   dxr_corr_lookup_conv1x1, grid (ceil(N/32), B):
 *     ceil(N/32) * B <= 256             corr_lookup_conv1x1_h2_kernel<1024>
 *     else                              corr_lookup_conv1x1_h2_kernel<512>
 *
 * Volume lookup (dxr_alt_volume_lookup).  Checks: a negative radius, the flags
 * on radius (DXR_ALT_VOL_F16 taken off first; then as above, the odd `out`
 * included): DXR_EINVAL; levels, 0 <= first_level < num_levels, divisor (not 0,
 * not NaN): DXR_EINVAL; radius > 8: DXR_EUNSUPPORTED; B > 65535: DXR_EINVAL;
 * B == 0: DXR_OK; a null pointer: DXR_EINVAL.
 *   unit: DXR_ALT_VOL_F16               corr_lookup_alt_vol16.hip
 *         else flagged                  corr_lookup_alt_out.hip
 *         else                          corr_lookup.hip
 *   kernel: the pyramid lookup's rule over num_levels - first_level levels,
 *   without the large misaligned exception:
 *     r <= 4, wg32 <= 1024              corr_lookup_qm_kernel<ALT, 256 x 16>
 *     else, r <= 4                      corr_lookup_qm_kernel<ALT, 512 x 32>
 *     else, r > 4                       corr_lookup_qm_kernel<ALT, 512 x 16>
 *
 * On-the-fly lookup (dxr_alt_corr_lookup, _ws, _levels_ws).  Checks: a negative
 * radius, both input flags, the output flags on radius, then n_levels < 1
 * (_levels_ws), the odd `out`: DXR_EINVAL; levels, n_levels > num_levels, C < 1,
 * divisor: DXR_EINVAL; radius > 6: DXR_EUNSUPPORTED; B > 65535, C > 2^20:
 * DXR_EINVAL; B == 0: DXR_OK; a null pointer, then a null level pointer among
 * the levels computed: DXR_EINVAL.
 *   unit: DXR_ALT_IN_BF16               alt_corr_inbf16.hip
 *         DXR_ALT_IN_F16                alt_corr_in16.hip
 *         else flagged                  alt_corr_out.hip
 *         else                          alt_corr.hip
 *   kernel.  "aligned": C % 4 == 0 and fmap1 and every level computed 16-byte
 *   aligned; "workspace": non-null, 16-byte aligned and at least
 *   dxr_alt_workspace_bytes for the levels computed (anything less counts as none):
 *     aligned, C % 16 == 0, C <= 256 (the matrix-core forms, every unit):
 *       workspace                       alt_bin_*_kernel + alt_corr_mfma_kernel<ordered>
 *       else                            alt_corr_mfma_kernel<tile order>
 *     else, with an input or output flag
 *                                       none: DXR_EUNSUPPORTED
 *     else, aligned                     alt_corr_kernel<vec>
 *     else                              alt_corr_kernel<scalar>
 */
int dxr_corr_lookup(const void* pyramid, int pyr_dtype,
                    int64_t B, int64_t H, int64_t W, int num_levels, int radius,
                    const float* coords, float* out, hipStream_t stream);

/*
 * Backward of stage (c) (training: core/utils/utils.py:65 grid_sample under
 * autograd, train.py:175-178): ADDS d loss / d pyramid of one lookup to
 * grad_pyramid, a float32 buffer with the pyramid's paged layout and size
 * (dxr_pyramid_numel; the caller zero-fills it once and may accumulate several
 * lookups into it).  grad_out: [B, num_levels*(2r+1)^2, H, W] float32.  No
 * coordinate gradient (the reference detaches coords, core/raft.py:170).
 * Cells the lookup does not tap keep their bits, and far / non-finite queries
 * add nothing, as grid_sample's backward does (tests/test_gpu_lookup_backward.py).
 */
int dxr_corr_lookup_backward(const float* coords, const float* grad_out,
                             int64_t B, int64_t H, int64_t W, int num_levels,
                             int radius, void* grad_pyramid, int grad_dtype,
                             hipStream_t stream);

/*
 * The same for n_sets lookups of one block at once (coords[i], grad_out[i]),
 * added in the order given — the result equals n_sets single calls in that
 * order bit for bit — in one launch, so each workgroup's window lines stay in
 * L2 across the sets.  n_sets <= 16 (more: DXR_EUNSUPPORTED).  ABI 7.
 */
int dxr_corr_lookup_backward_multi(const float* const* coords, const float* const* grad_out,
                                   int n_sets, int64_t B, int64_t H, int64_t W,
                                   int num_levels, int radius, void* grad_pyramid,
                                   int grad_dtype, hipStream_t stream);

/*
 * dxr_corr_lookup_backward_multi that also records a magnitude bound of the
 * gradient pyramid for dxr_fmap_grads_bounded: every workgroup adds to its own
 * element of bound_slots (a float32 array of dxr_lookup_backward_bound_slots(B,
 * H, W, num_levels, radius) elements that the caller zero-fills with the
 * gradient pyramid) 9 x the largest |grad_out| it reads per set (a cell hears
 * from at most 3 x 3 samples, tap weights <= 1; non-finite values count as
 * +inf), so after any number of calls max(bound_slots) >= max |grad_pyramid|.
 * The gradient pyramid is the one dxr_corr_lookup_backward_multi writes, bit
 * for bit.  ABI 8.
 */
int64_t dxr_lookup_backward_bound_slots(int64_t B, int64_t H, int64_t W, int num_levels,
                                        int radius);
int dxr_corr_lookup_backward_multi_bound(const float* const* coords,
                                         const float* const* grad_out, int n_sets,
                                         int64_t B, int64_t H, int64_t W, int num_levels,
                                         int radius, void* grad_pyramid, int grad_dtype,
                                         float* bound_slots, hipStream_t stream);

/*
 * Stage (c) fused with the motion encoder's 1x1 convolution (SURVEY.md §8(f)
 * row 2; inference):
 *   out[b,o,h,w] = act(bias[o] + sum_c weight[o,c] * lookup(coords)[b,c,h,w])
 * lookup() is dxr_corr_lookup (bit-identical samples), the contraction runs in
 * f32 class (f16 pair split of both operands, x = hi + 2^-11 lo, three MFMA
 * products, f32 accumulation; workgroups whose sums are not finite re-run it on
 * the exact three-way bf16 split).
 * Range: the split carries no power-of-two prescale.  hi = f16(x) and
 * lo = f16((x - hi) * 2048) represent an operand (weight or sample) to 2^-22 |x|
 * while |x| >= 2^-13, and to an absolute 2^-36 below that (f16's subnormal
 * grid): the contraction is f32 class while operand magnitudes are at least
 * 2^-13; a smaller operand contributes up to 2^-36 times the other operand's
 * magnitude per product.  Magnitudes of 65520 and above round to inf in f16, make
 * the sums non-finite and take the workgroup (32 consecutive queries of one batch
 * item) to the bf16 split, which has float32's range.  Per output element,
 * |out - exact| <= sum_c [d(|w|) d(|x|) + e(|w|) |x| + |w| e(|x|)]
 *                  + (cin + 4) 2^-24 (|bias| + sum_c |w| |x|),
 * d(a) = 2^-11 a (2^-25 below 2^-14), e(a) = 2^-11 d(a)
 * (tests/motion_oracle.py, tests/test_gpu_motion_per_element.py).
 *   weight_packed : dxr_conv1x1_pack_weight of the [cout, cin] float32 weight,
 *                   cin = num_levels*(2r+1)^2 (dxr_conv1x1_packed_bytes bytes:
 *                   float32 [ceil(cin/16)*2][cout][8], zero padded, followed by
 *                   the same layout as f16 pairs, 8 hi then 8 lo per 32 bytes)
 *   bias          : [cout] float32 or NULL;  relu: 1 = F.relu, 0 = none
 *   out           : [B, cout, H, W] float32; with pyr_dtype | DXR_OUT_F16 or
 *                   | DXR_OUT_BF16 float16 / bfloat16 elements (2-byte aligned),
 *                   as dxr_corr_lookup: the same float32 accumulation, bias and
 *                   ReLU, converted round-to-nearest-even in the store; with
 *                   | DXR_OUT_NHWC [B, H, W, cout] (channels-last), the same
 *                   elements bit for bit
 * Supported: radius 3 or 4, num_levels <= 4, cout a multiple of 32 (<= 4096);
 * other valid requests return DXR_EUNSUPPORTED.
 */
int64_t dxr_conv1x1_packed_bytes(int64_t cout, int64_t cin);
int dxr_conv1x1_pack_weight(const float* weight, int64_t cout, int64_t cin,
                            void* packed, hipStream_t stream);
int dxr_corr_lookup_conv1x1(const void* pyramid, int pyr_dtype,
                            int64_t B, int64_t H, int64_t W, int num_levels,
                            int radius, const float* coords,
                            const void* weight_packed, const float* bias,
                            int64_t cout, int relu, float* out,
                            hipStream_t stream);

/*
 * Backward of stages (a)+(b) down to the volume: folds the gradient of every
 * level down the avg-pool chain (core/corr.py:25-27) and divides by `divisor`
 * (core/corr.py:60), writing d loss / d (fmap1^T fmap2) as row-major
 * [B*H*W, H, W] float32.  The fmap gradients are then two plain GEMMs:
 * dfmap1 = fmap2 . dV^T, dfmap2 = fmap1 . dV (per pair, [D, H*W]).
 */
int dxr_pyramid_backward(const void* grad_pyramid, int grad_dtype,
                         int64_t B, int64_t H, int64_t W, int num_levels,
                         float divisor, float* grad_volume, hipStream_t stream);

/*
 * Backward of stages (a)+(b) straight to the fmap gradients, without the
 * [B, H*W, H*W] volume gradient (core/corr.py:13-27,52-60 under autograd,
 * train.py:175-178): the gradient pyramid is folded down the pooling chain
 * inside the two GEMMs' operand loads,
 *   grad_fmap1 = fmap2 . dV^T,  grad_fmap2 = fmap1 . dV   (dV as above),
 * on MFMA with a three-way bf16 split of both operands (six products, f32
 * accumulation: f32-class).  Deterministic (fixed summation order).
 * Range: every finite operand stays finite in the split (one beyond
 * bfloat16's largest finite value, |x| > 3.3895e38, keeps its truncation as the
 * high part instead of rounding it to +-inf); inf and NaN operands propagate as
 * in an f32 GEMM.
 *   grad_pyramid : float32, the paged layout of dxr_corr_pyramid_build
 *   fmap1, fmap2 : [B, D, H, W] float32, NCHW contiguous
 *   grad_fmap1/2 : [B, D, H, W] float32 outputs, either may be NULL (skipped)
 *   workspace    : >= dxr_fmap_grads_workspace_bytes(B, D, H, W, num_levels)
 * Supported: D a multiple of 32, num_levels <= 4 (other valid requests return
 * DXR_EUNSUPPORTED; dxr_pyramid_backward + two GEMMs covers them).
 * dxr_fmap_grads_workspace_bytes returns -1 for unsupported shapes.  ABI 7.
 */
int64_t dxr_fmap_grads_workspace_bytes(int64_t B, int64_t D, int64_t H, int64_t W,
                                       int num_levels);
int dxr_fmap_grads(const void* grad_pyramid, int grad_dtype, const float* fmap1,
                   const float* fmap2, int64_t B, int64_t D, int64_t H, int64_t W,
                   int num_levels, float divisor, float* grad_fmap1, float* grad_fmap2,
                   void* workspace, int64_t workspace_bytes, hipStream_t stream);

/*
 * dxr_fmap_grads given a bound on the gradient pyramid: bound_slots[0..n_slots)
 * (device float32, e.g. dxr_corr_lookup_backward_multi_bound's slots) hold
 * values whose maximum is >= max |grad_pyramid|.  Both operands then run as
 * power-of-two-scaled f16 pairs (x 2^s = hi + lo, |x 2^s| < 2^14; one scale per
 * fmap channel, one for the folded dV) with three f16 MFMA products and f32
 * accumulation — half the MFMA work of the six-product split, f32-class:
 * per-operand error <= 2^-22 |x| + 2^-39 of its scale's bound.  A pair whose
 * fmap holds inf/NaN, or a non-finite bound, runs the six-product arithmetic of
 * dxr_fmap_grads (same IEEE propagation).  A bound below the true maximum gives
 * wrong (overflowed) results.  workspace: >= dxr_fmap_grads_bounded_workspace_bytes
 * (<= dxr_fmap_grads_workspace_bytes, which covers both forms).  Same outputs'
 * layout, deterministic.  ABI 8.
 */
int64_t dxr_fmap_grads_bounded_workspace_bytes(int64_t B, int64_t D, int64_t H, int64_t W,
                                               int num_levels);
int dxr_fmap_grads_bounded(const void* grad_pyramid, int grad_dtype, const float* fmap1,
                           const float* fmap2, int64_t B, int64_t D, int64_t H, int64_t W,
                           int num_levels, float divisor, const float* bound_slots,
                           int64_t n_slots, float* grad_fmap1, float* grad_fmap2,
                           void* workspace, int64_t workspace_bytes, hipStream_t stream);

/*
 * 2x2 / stride-2 average pool, floor mode, of [planes, H, W] float32 into
 * [planes, H/2, W/2] (F.avg_pool2d(x, 2, stride=2), core/corr.py:26,70-71).
 */
int dxr_avg_pool2x2(const float* in, float* out, int64_t planes,
                    int64_t H, int64_t W, hipStream_t stream);

/*
 * Channels-last fmaps.
 *
 * dxr_transpose: batched [B, rows, cols] -> [B, cols, rows] of float32
 * (dtype DXR_F32) or bfloat16 (DXR_BF16) elements; NCHW -> NHWC is rows = C,
 * cols = H*W (core/corr.py:82-83 `permute(0, 2, 3, 1).contiguous()`), NHWC ->
 * NCHW the reverse.  Bit-exact.
 *
 * dxr_avg_pool2x2_nhwc: F.avg_pool2d(x, 2, stride=2) (core/corr.py:70-71) of a
 * channels-last [B, H, W, C] float32 tensor into [B, H/2, W/2, C]; bit-identical
 * to dxr_avg_pool2x2 on the NCHW tensor (same four values, same summation order).
 */
int dxr_transpose(const void* in, void* out, int dtype, int64_t B, int64_t rows,
                  int64_t cols, hipStream_t stream);
int dxr_avg_pool2x2_nhwc(const float* in, float* out, int64_t B, int64_t H,
                         int64_t W, int64_t C, hipStream_t stream);

/*
 * Stage (d), reference-FFI form: alt_cuda_corr.forward(fmap1, fmap2, coords,
 * radius) with the reference's layouts (see the header comment).  `corr` is
 * fully overwritten (the reference zero-fills then accumulates).
 */
int dxr_alt_corr_forward(const float* fmap1, const float* fmap2,
                         const float* coords, float* corr,
                         int64_t B, int64_t H1, int64_t W1, int64_t H2,
                         int64_t W2, int64_t C, int64_t Nc, int radius,
                         hipStream_t stream);

/*
 * Stage (d), reference-FFI backward: alt_cuda_corr.backward(fmap1, fmap2, coords,
 * corr_grad, radius) (correlation.cpp:36-48, correlation_kernel.cu:122-256,288-320).
 *   corr_grad  : [B, Nc, (2r+1)^2, H1, W1] float32 (the forward's output layout)
 *   fmap1_grad : [B, H1, W1, C]  fully overwritten
 *   fmap2_grad : [B, H2, W2, C]  zero-filled on `stream`, then accumulated with
 *                atomics (summation order, hence the last bits, is not fixed —
 *                as in the reference)
 * The reference's third output, coords_grad, is identically zero; the caller
 * allocates it.  Radius 0..6.
 *
 * DXR_ALT_BWD_ACCUMULATE or-ed onto `radius` (low byte: the radius, 0..6): the
 * values the unflagged call would write — same mathematics, layouts and channel
 * order iy + (2r+1)*ix, no 1/sqrt(C) — are ADDED INTO fmap1_grad and fmap2_grad.
 * No memset is issued: the caller zero-fills (or keeps accumulating into) both.
 * The call runs one exact-f32 MFMA kernel (v_mfma_f32_32x32x2_f32): a workgroup
 * takes a 4 x 8 tile of queries, walks the union box of their windows and adds
 * one float atomic per (box cell, channel) into fmap2_grad instead of one per
 * (query, cell, channel); fmap1_grad is added by the tile's own workgroup
 * (atomically when Nc > 1).  Served when C % 16 == 0, C <= 256, B * Nc <= 65535
 * and the four fmap pointers are 16-byte aligned; other shapes and radius > 6
 * are DXR_EUNSUPPORTED (callers then use the unflagged call and add).  With the
 * flag any other bit above the low byte is DXR_EINVAL, null pointers are
 * DXR_EINVAL and B == 0 is DXR_OK; everything is answered on the host before any
 * launch, and every `radius` without the bit is answered as it always was.
 * Contract: finite fmaps and finite corr_grad (the box GEMM multiplies a zero
 * weight with cells and queries the per-query form never reads, and 0 * inf is
 * NaN).  Coordinates may be anything: a query with a NaN, infinite or far
 * (|floor| >= 1e8) coordinate, or whose window lies off the map, has weights
 * exactly 0 and contributes exactly nothing (the unflagged kernel returns NaN
 * rows for non-finite coordinates).  fmap2_grad's last bits depend on the
 * order of the atomics, as above.
 */
int dxr_alt_corr_backward(const float* fmap1, const float* fmap2,
                          const float* coords, const float* corr_grad,
                          float* fmap1_grad, float* fmap2_grad,
                          int64_t B, int64_t H1, int64_t W1, int64_t H2,
                          int64_t W2, int64_t C, int64_t Nc, int radius,
                          hipStream_t stream);

/*
 * Stage (d), fused form used by AlternateCorrBlock.__call__: every level in one
 * launch, output already divided by `divisor`, written in CorrBlock's layout.
 *   fmap1        : [B, H, W, C] full resolution (NHWC)
 *   fmap2_levels : num_levels pointers; level l is [B, H_l, W_l, C] (NHWC),
 *                  H_l = floor(H_{l-1}/2)
 *   coords       : [B, 2, H, W] float32 (CorrBlock convention)
 *   out          : [B, num_levels*(2r+1)^2, H, W] float32
 *
 * Output flags on radius.  DXR_OUT_F16, DXR_OUT_BF16 and DXR_OUT_NHWC may be
 * or-ed onto the `radius` argument of dxr_alt_corr_lookup, dxr_alt_corr_lookup_ws,
 * dxr_alt_corr_lookup_levels_ws and dxr_alt_volume_lookup (not of
 * dxr_alt_corr_forward / _backward); the low byte is the radius.  Semantics are
 * dxr_corr_lookup's:
 *   DXR_OUT_F16 / DXR_OUT_BF16  `out` holds float16 / bfloat16 elements (passed
 *       through the float* parameter, 2-byte aligned; an odd address is
 *       DXR_EINVAL): each is the unflagged call's float32 element rounded to
 *       nearest even in the store (float16 overflows to +-inf, subnormals are
 *       kept, NaN stays NaN), i.e. out.to(dtype) bit for bit, a NaN's bits
 *       included (float16 keeps its sign and payload; bfloat16 is 0x7FC0 for
 *       every NaN, as torch converts);
 *   DXR_OUT_NHWC (alone or with one dtype flag)  `out` is [B, H, W, C],
 *       C = num_levels*(2r+1)^2: element (b, c, h, w) of the NCHW call lands at
 *       ((b*H + h)*W + w)*C + c with the same bits.
 * No byte outside the call's own elements is written under either flag: a partial
 * call (_levels_ws with n_levels < num_levels, dxr_alt_volume_lookup from
 * first_level) writes only its levels' channels of each pixel's run of C, so the
 * two partial calls fill one tensor when given the same flags.  Both dtype flags
 * together, or any other bit above the low byte, is DXR_EINVAL, answered on the
 * host before every other check (the B == 0 return and the pointer checks
 * included) and before any launch.
 * Which forms implement the flags: the MFMA forms of the three on-the-fly calls
 * (C % 16 == 0, C <= 256, 16-byte aligned operands; tile order, ordered and
 * _levels_ws, radius 0..6) and dxr_alt_volume_lookup (radius 0..8) implement
 * every combination natively.  The per-query VALU forms (any other C, or
 * misaligned operands) decline a flagged request with DXR_EUNSUPPORTED and
 * launch nothing; the caller runs the unflagged call and converts.
 *
 * Float16 fmaps on radius.  DXR_ALT_IN_F16, or-ed onto the `radius` of
 * dxr_alt_corr_lookup, dxr_alt_corr_lookup_ws and dxr_alt_corr_lookup_levels_ws,
 * alone or with any valid combination of the output flags above: fmap1 and
 * fmap2_levels[0] point at [B, H, W, C] IEEE float16 (through the float*
 * parameters) — the feature maps a mixed-precision encoder emits, which the
 * reference widens first (core/raft.py:139-142) — and fmap2_levels[l >= 1] at
 * float32 as ever: the 2x2 means of the level above, pooled from the widened
 * level 0, which are not float16 numbers.  The call returns what the unflagged
 * call returns on the widened float32 copies of the two maps: with finite fmaps
 * every output is equal as a value (+0 and -0 compare equal) under every output
 * flag.  Level 0 is one f16 matrix-core product per k step on the raw values and
 * needs no overflow fallback; the pooled levels issue two products instead of
 * three.  With inf / NaN in the fmaps the outputs are non-finite exactly where
 * exact arithmetic's are; the finite outputs of a chunk that the widened call
 * recomputes on its bf16 split may differ from it in the last bits.
 * Served when C % 16 == 0, C <= 256, radius <= 6 and fmap1 and every level are
 * 16-byte aligned; any other C or alignment (the per-query VALU forms have no
 * float16 variant) and radius > 6 are DXR_EUNSUPPORTED, null pointers DXR_EINVAL,
 * B == 0 DXR_OK, all answered on the host before any launch; the caller widens
 * and runs the unflagged call.  dxr_alt_volume_lookup (no fmaps),
 * dxr_alt_corr_forward / _backward and dxr_alt_coarse_volumes* do not take the
 * bit: there it is an unknown flag.
 *
 * Bfloat16 fmaps on radius.  DXR_ALT_IN_BF16, or-ed onto the `radius` of
 * dxr_alt_corr_lookup, dxr_alt_corr_lookup_ws and dxr_alt_corr_lookup_levels_ws,
 * alone or with any valid combination of the output flags above: fmap1 and
 * fmap2_levels[0] point at [B, H, W, C] bfloat16 (through the float*
 * parameters) — the maps an encoder emits under bfloat16 autocast, which the
 * reference widens first (core/raft.py:139-142) — and fmap2_levels[l >= 1] at
 * float32: the 2x2 means pooled from the widened level 0.  Level 0 is one bf16
 * matrix-core product per k step on the raw values: 8-bit significands multiply
 * exactly into the float32 accumulator and bfloat16 has float32's exponent
 * range, so there is no split, no scaling and no overflow fallback.  A pooled
 * level's float32 cells are split exactly into three bfloat16 parts, each
 * multiplied with the raw query: three exact products per k step.  Every output
 * is the float32 sum of exact products, within 1e-5 of sum |fmap1| |fmap2|
 * (combined as the output is) of the exact result; it is not claimed bit-equal
 * to the unflagged call on the widened maps, which accumulates the same
 * products through another instruction and in its own fallback where a value
 * lies outside float16's range.  inf / NaN propagate by IEEE arithmetic.  The
 * ordered and tile-order forms agree bit for bit, and a flagged output is the
 * float32 NCHW output converted.  DXR_ALT_IN_F16 | DXR_ALT_IN_BF16 is
 * DXR_EINVAL.  Served when C % 16 == 0, C <= 256, radius <= 6 and fmap1 and
 * every level are 16-byte aligned; any other C or alignment and radius > 6 are
 * DXR_EUNSUPPORTED, null pointers DXR_EINVAL, B == 0 DXR_OK, all answered on the
 * host before any launch; the caller widens and runs the unflagged call.
 * dxr_alt_volume_lookup, dxr_alt_corr_forward / _backward and
 * dxr_alt_coarse_volumes* do not take the bit, as they do not take
 * DXR_ALT_IN_F16.
 */
int dxr_alt_corr_lookup(const float* fmap1, const float* const* fmap2_levels,
                        const float* coords, float* out,
                        int64_t B, int64_t H, int64_t W, int64_t C,
                        int num_levels, int radius, float divisor,
                        hipStream_t stream);

/*
 * Bytes of device workspace dxr_alt_corr_lookup_ws uses for B coordinate sets
 * of H x W queries over num_levels levels (per level and set: the ordered list,
 * 16 B per query slot of every 4 x 8 query tile, 4-B bin ids, 64 blocks'
 * histograms of up to 4097 bins; -1: bad geometry).  ABI 6.
 */
int64_t dxr_alt_workspace_bytes(int64_t B, int64_t H, int64_t W, int num_levels);

/*
 * dxr_alt_corr_lookup with a caller-owned workspace (16-byte aligned, at least
 * dxr_alt_workspace_bytes; no initialisation needed).  Three small launches
 * (count, scan, scatter) order each level's queries before the lookup: grouped
 * by window position (bins of ~32 queries) when the 4 x 8 query tiles' union
 * boxes would be larger than 1.5x a bin group's (flows that vary pixel to
 * pixel), else in tile order.  The scan always walks the fixed 64 x 4097-bin
 * histogram, so the three launches cost a few microseconds even for small
 * maps.  The outputs are the workspace-less call's, bit for bit.  Falls back to
 * dxr_alt_corr_lookup when the workspace is NULL or short.  Replaces
 * core/corr.py:74-91 as above.  ABI 6.
 */
int dxr_alt_corr_lookup_ws(const float* fmap1, const float* const* fmap2_levels,
                           const float* coords, float* out,
                           int64_t B, int64_t H, int64_t W, int64_t C,
                           int num_levels, int radius, float divisor,
                           void* workspace, int64_t workspace_bytes,
                           hipStream_t stream);

/*
 * dxr_alt_corr_lookup_ws for levels [0, n_levels) only of a num_levels-level
 * output (channels of the other levels untouched): the alternate block's
 * on-the-fly part when its coarse levels come from dxr_alt_volume_lookup.
 * Workspace: dxr_alt_workspace_bytes(B, H, W, n_levels).  Replaces
 * core/corr.py:74-91 for those levels.  ABI 9.
 */
int dxr_alt_corr_lookup_levels_ws(const float* fmap1, const float* const* fmap2_levels,
                                  const float* coords, float* out,
                                  int64_t B, int64_t H, int64_t W, int64_t C,
                                  int num_levels, int n_levels, int radius, float divisor,
                                  void* workspace, int64_t workspace_bytes,
                                  hipStream_t stream);

/*
 * Coarse-level volumes of the alternate block (round 6).  An on-the-fly
 * lookup recomputes each level's window dot products on every call; for a
 * coarse level the whole volume (every fmap1 pixel against every cell of the
 * pooled fmap2 level) costs less than one lookup, once per block.
 *   dxr_alt_volume_numel    floats of the volumes of levels
 *                           [first_level, num_levels) (-1: bad geometry);
 *   dxr_alt_coarse_volumes  computes them: raw dot products <fmap1[q],
 *                           fmap2_levels[l][cell]> (not divided), the same
 *                           f16-pair MFMA products as dxr_alt_corr_lookup's,
 *                           stored in the paged layout of those pyramid levels
 *                           (the tail of a num_levels-level pyramid buffer);
 *                           fmap1 / fmap2_levels as dxr_alt_corr_lookup
 *                           (NHWC, 16-byte aligned), C % 16 == 0, C <= 256;
 *   dxr_alt_volume_lookup   reads the windows of levels [first_level,
 *                           num_levels) from them with correlation_kernel.cu's
 *                           arithmetic (origin floor(c / 2^l) - r, bilinear
 *                           weights of the fraction, :92-114's order, divided
 *                           by divisor) into those levels' channels of `out`
 *                           ([B, num_levels*(2r+1)^2, H, W]); r <= 8.  Takes
 *                           the output flags on `radius` (dxr_alt_corr_lookup),
 *                           every combination at every radius.
 * With finite operands inside the f16 pair's range the outputs are
 * dxr_alt_corr_lookup's bit for bit.  Replaces core/corr.py:74-91 (levels
 * >= first_level) with the reference's alt_cuda_corr semantics.  ABI 9.
 *   dxr_alt_coarse_volumes_ws_bytes / dxr_alt_coarse_volumes_ws (ABI 10): the
 *                           same volumes, bit for bit, with a caller workspace
 *                           for the f16 pair planes of fmap1 and of the levels
 *                           (C % 32 == 0, levels 0-3), which the volume GEMM
 *                           then stages by LDS-DMA; a null or short workspace
 *                           falls back to dxr_alt_coarse_volumes.  0 bytes when
 *                           no level takes the GEMM; -1: bad geometry.
 *
 * Float16 volumes.  DXR_ALT_VOL_F16 halves the volumes' memory (about 333 MB of
 * float32 per 1080p pair, levels 2-3).  No new tolerance is involved:
 *   dxr_alt_coarse_volumes / dxr_alt_coarse_volumes_ws with the flag or-ed onto
 *       `first_level` (the low byte is the level): `volumes` points at
 *       dxr_alt_volume_numel(...) float16 elements (the count is in elements and
 *       does not change; passed through the float* parameter) and must be 16-byte
 *       aligned, else DXR_EINVAL.  Every stored cell is the unflagged call's
 *       float32 cell for the same operands rounded once to float16 in the GEMM's
 *       own stores: to nearest even, beyond 65504 to +-inf, subnormals kept, still
 *       the raw dot product.  The layout is counted in elements, so the buffer is
 *       the float32 buffer's .half() element for element over every written page.
 *       A 32 x 32 tile goes to the bf16-split fallback on its float32 sums, as
 *       unflagged: a finite sum that rounds to +-inf is stored as +-inf.
 *   dxr_alt_volume_lookup with the flag or-ed onto `radius`, alone or with any
 *       valid combination of DXR_OUT_F16 / DXR_OUT_BF16 / DXR_OUT_NHWC: `volumes`
 *       holds float16 cells, which are widened on load (exact) before the float32
 *       arithmetic.  The output is that of the unflagged call with the same output
 *       flags on the widened float32 copy of the buffer, bit for bit, for radius
 *       0..8 and NaN / inf / far coordinates.  The flag beside
 *       DXR_ALT_IN_F16 / DXR_ALT_IN_BF16 or any other unknown bit is DXR_EINVAL.
 * Served natively: C % 32 == 0 and every requested level a tiled level (num_levels
 * <= 4: the volume GEMM's levels).  Any other valid request — C % 32 != 0, whose
 * levels take the FULL box form, or a row-major level 4 and beyond — is
 * DXR_EUNSUPPORTED, answered on the host before any launch; the caller builds the
 * float32 volumes and rounds them, which is the same buffer by definition.
 * dxr_alt_volume_numel and dxr_alt_coarse_volumes_ws_bytes do not take the bit
 * (-1), every other entry point rejects it as an unknown bit (DXR_EINVAL;
 * dxr_alt_corr_forward / _backward: DXR_EUNSUPPORTED, as for the other high bits).
 */
int64_t dxr_alt_volume_numel(int64_t B, int64_t H, int64_t W, int num_levels, int first_level);
int dxr_alt_coarse_volumes(const float* fmap1, const float* const* fmap2_levels,
                           int64_t B, int64_t H, int64_t W, int64_t C,
                           int num_levels, int first_level, float* volumes,
                           hipStream_t stream);
int64_t dxr_alt_coarse_volumes_ws_bytes(int64_t B, int64_t H, int64_t W, int64_t C,
                                        int num_levels, int first_level);
int dxr_alt_coarse_volumes_ws(const float* fmap1, const float* const* fmap2_levels,
                              int64_t B, int64_t H, int64_t W, int64_t C,
                              int num_levels, int first_level, float* volumes,
                              void* workspace, int64_t workspace_bytes, hipStream_t stream);
int dxr_alt_volume_lookup(const float* volumes, const float* coords, float* out,
                          int64_t B, int64_t H, int64_t W, int num_levels, int first_level,
                          int radius, float divisor, hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DEXIRAFT_CORR_H */
