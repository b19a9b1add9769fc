// Which unit, kernel shape and store policy serve a forward lookup request: the
// host-only planner behind dxr_corr_lookup / dxr_corr_lookup_conv1x1 (the
// pyramid lookup), dxr_alt_volume_lookup (the volume lookup) and
// dxr_alt_corr_lookup / _ws / _levels_ws (the on-the-fly lookup);
// include/dexiraft_corr.h, "Lookup kernels by request".  Plain C++, no HIP: the
// entry points (corr_lookup.hip, alt_corr.hip) call a plan_* function once and
// switch on its result, and tests/test_lookup_plan.py runs the same functions on
// a CPU, row by row of that table.  Every refusal is answered here, in the order
// the checks stand in, and every rule (flag split, workgroup shape, store policy,
// kernel form) is written here once, so the launchers validate nothing and
// compute no rule.  Nothing here allocates: plain structs on the caller's stack.
#pragma once

#include <stdint.h>

#include "dexiraft_corr.h"
#include "pyramid_layout.h"

namespace dxr {

// ---------------------------------------------------------------------------
// Shared pieces
// ---------------------------------------------------------------------------

// The output flags of the lookups (DXR_OUT_F16 / DXR_OUT_BF16 / DXR_OUT_NHWC) or-ed
// onto an argument whose low byte is the value proper: splits them off.  False
// for both dtype flags together or any other bit above the low byte (every
// negative value has some).
inline bool split_out_flags(int* value, int* out_flag, bool* nhwc) {
  const int hi = *value & ~0xff;
  const int dt = hi & ~DXR_OUT_NHWC;
  *out_flag = dt;
  *nhwc = (hi & DXR_OUT_NHWC) != 0;
  *value &= 0xff;
  return dt == 0 || dt == DXR_OUT_F16 || dt == DXR_OUT_BF16;
}

// A 16-bit `out` is 2-byte aligned.
inline bool out_aligned(int out_flag, uintptr_t out) { return out_flag == 0 || (out & 1) == 0; }

inline bool aligned16(uintptr_t p) { return p % 16 == 0; }

inline bool divisor_ok(float d) { return d == d && d != 0.f; }

// 1 / d when d is a (normal) power of two, 2^-125 ... 2^124 — then x * (1 / d) ==
// x / d exactly — else 0: the volume and the on-the-fly lookups' div_recip.
inline float pow2_recip(float d) {
  uint32_t u;
  __builtin_memcpy(&u, &d, sizeof u);
  const uint32_t se = u >> 23;   // sign and biased exponent
  return (u & 0x7fffffu) == 0 && se >= 2 && se <= 251 ? 1.f / d : 0.f;
}

// The workgroup shapes of the lookup kernels.
enum LookupShape {
  SHAPE_NONE = 0,       // B == 0, or a refused request: nothing to launch
  SHAPE_ONE_ROUND,      // corr_lookup_qm_kernel, 256 threads x 16 queries, plain loads
  SHAPE_MULTI_ROUND,    //   512 threads x QB queries (32; 16 for r > 4), buffer loads
  SHAPE_CONV_1024,      // corr_lookup_conv1x1_h2_kernel, 1024 threads x 32 queries
  SHAPE_CONV_512        //   512 threads x 32 queries
};

// What a launcher takes: the shape, its grid and the NCHW forms' store policy
// (LookupGeom::out_nt; 1: non-temporal output stores, 0: write-through).
struct LookupLaunch {
  int shape;
  unsigned gx, gy, gz;
  int out_nt;
};

constexpr int LOOKUP_ONE_QB = 16;                                   // queries per one-round workgroup
constexpr int lookup_multi_qb(int radius) { return radius <= 4 ? 32 : 16; }   // WideCfg<R>::QB

// Cells of one pair's level 0 as stored: whole pages (queries padded to 128,
// image 2 to whole tiles).
inline int64_t level0_cells(const LevelLayout& y) {
  return (int64_t)y.qt * y.qb * y.ty * y.tx * y.th * y.tw;
}

// The product's workgroup shape: true = the one-round 256 x 16 shape, false =
// 512 x 32 (512 x 16 for r > 4).  Shared by the NCHW and the channels-last
// launchers.
// Workgroup shape: 512 threads x 32 queries (4 resident per CU), or — when that
// grid fits in one dispatch round (<= 1024 workgroups: Sintel / Chairs B=1) —
// 256 threads x 16 queries, the same 16 threads per query in twice the
// workgroups, so the per-CU load evens out (3.44 -> 6.9 workgroups per CU at
// Sintel B=1: one CU in four no longer runs a fourth workgroup after the rest).
// Round 3, same-process A/B (bit-identical): Sintel B=1 8.0 -> 7.4 us, Chairs
// 5.6 -> 5.2 us; multi-round grids keep 512 x 32 (Sintel B=8 50.4 vs 53.3 us).
// Output store policy (round 5, same-process A/Bs in the step, scripts/ab_step.py,
// profiles/r05/experiments/r6e_lookup_output_nt.jsonl): non-temporal stores
// gained 2-9 % per step wherever a wave stores whole lines (the 512 x 32 shape: 32
// consecutive queries of a channel = 128 B; Sintel B=8 -2.3 %, KITTI B=8 bf16
// -5.6 %, Chairs B=4 -8.9 %, Sintel B=2 -2.3 %) and with the 256 x 16 shape
// (64-B segments) when those are half-line aligned (N % 32 == 0: Sintel B=1 f32
// -4.0 %, bf16 -4.4 %); with misaligned 64-B segments (KITTI, Chairs at B=1)
// write-through stores, which L2 merges, were 2-12 % faster — except with a large
// pyramid (>= 128 MB: KITTI B=1, 286 MB f32 / 143 MB bf16), where the 512 x 32 shape
// with non-temporal stores beat both (-6.3 % / -3.9 %, r6k); a small one (Chairs
// B=1, 43 MB, resident anyway) keeps 256 x 16 with write-through (+13 % otherwise).
// `levels`: the levels the grid covers; `cell_bytes`: the size of a pyramid cell;
// `lv0_cells`: level0_cells of the pyramid (the pyramid's bytes as the build's
// store rule counts them: padded level-0 pages, x 4/3 for levels 1-3).
// lv0_cells == 0: no large-pyramid exception — the volume lookup, whose rule
// was written without it and stays so.
inline bool lookup_one_round(int radius, int64_t N, int levels, int64_t B, int cell_bytes,
                             int64_t lv0_cells) {
  const int qb = lookup_multi_qb(radius);
  const long long wg32 = (long long)((N + qb - 1) / qb) * levels * B;
  const double pyr_bytes = (double)B * (double)lv0_cells * cell_bytes * (4.0 / 3.0);
  const bool big_misaligned = N % 32 != 0 && pyr_bytes >= 128.0 * (1 << 20);
  return radius <= 4 && wg32 <= 1024 && !big_misaligned;
}

// The shape, grid and store policy of corr_lookup_qm_kernel by that rule.
// Channels-last outputs (`nhwc`) take their store policy at compile time and do
// not read out_nt: it stays 0.  Their rule (same-process A/B in the step,
// scripts/ab_nhwc_out.py, profiles/r11/nhwc_out/): the NCHW rule above was derived
// for whole or half lines along queries and does not carry over — there a wave
// instruction covers 256 consecutive bytes (128 with 16-bit outputs) of a query's
// run of K channels, which starts wherever l * K elements into the query's row
// falls — so non-temporal stores in both shapes.  Per step (build + 12 lookups),
// non-temporal / write-through / plain: Sintel B=1 213.4 / 231.2 / 229.1 us,
// Sintel B=8 1,357 / 1,431 / 1,398, KITTI B=8 bf16 939 / 1,019 / 1,018, Sintel B=8
// float16 outputs 1,328 / 1,383 / 1,354 (A/A spread 1-8 us): as in the NCHW form,
// outputs that leave the caches keep the pyramid lines of the next lookups
// resident.
inline LookupLaunch lookup_launch(int radius, int64_t N, int levels, int64_t B, int cell_bytes,
                                  int64_t lv0_cells, bool nhwc) {
  const bool one = lookup_one_round(radius, N, levels, B, cell_bytes, lv0_cells);
  const int qb = one ? LOOKUP_ONE_QB : lookup_multi_qb(radius);
  LookupLaunch s;
  s.shape = one ? SHAPE_ONE_ROUND : SHAPE_MULTI_ROUND;
  s.gx = (unsigned)((N + qb - 1) / qb);
  s.gy = (unsigned)levels;
  s.gz = (unsigned)B;
  s.out_nt = nhwc ? 0 : one ? (N % 32 == 0 ? 1 : 0) : 1;
  return s;
}

// The fused lookup + 1x1 convolution: one workgroup per 32 queries and pair.
// Grids up to one workgroup per CU (Sintel B=1: 220) run the 1024-thread form
// (more waves per workgroup: 24 vs 26 us); larger grids the 512-thread form,
// ~76 KB LDS and 128 VGPRs, two workgroups per CU (Sintel B=2: 35 vs 47 us,
// KITTI-shape B=8: 136 vs 190 us; r01 kernel 52 / 214 us).
inline LookupLaunch conv1x1_launch(int64_t N, int64_t B) {
  LookupLaunch s;
  s.gx = (unsigned)((N + 31) / 32);
  s.gy = (unsigned)B;
  s.gz = 1;
  s.shape = (long long)s.gx * s.gy <= 256 ? SHAPE_CONV_1024 : SHAPE_CONV_512;
  s.out_nt = 0;
  return s;
}

inline int cell_bytes(int cells) { return cells == DXR_F32 ? 4 : 2; }

// ---------------------------------------------------------------------------
// Pyramid lookup: dxr_corr_lookup and (conv1x1) dxr_corr_lookup_conv1x1
// ---------------------------------------------------------------------------

// The translation unit that instantiates a request's form.
enum LookupUnit {
  LOOKUP_UNIT_NONE = 0,
  LOOKUP_UNIT_MAIN,     // corr_lookup.hip: f32 / bf16 cells, float32 NCHW out
  LOOKUP_UNIT_OUT16,    // corr_lookup_out16.hip: f32 / bf16 cells, 16-bit NCHW out
  LOOKUP_UNIT_PYR16,    // corr_lookup_pyr16.hip: float16 cells, every NCHW out
  LOOKUP_UNIT_NHWC      // corr_lookup_nhwc.hip: channels-last out, every cell and type
};

struct LookupRequest {
  int pyr_dtype;            // the flags still on
  int64_t B, H, W;
  int num_levels, radius;
  bool conv1x1;
  int64_t cout;             // conv1x1: the convolution's output channels
  uintptr_t pyramid, coords, weight_packed, out;   // weight_packed: conv1x1 only
};

struct LookupPlan {
  int unit;                 // LookupUnit
  int cells;                // DXR_F32 / DXR_BF16 / DXR_PYR_F16
  int out_flag;             // 0, DXR_OUT_F16 or DXR_OUT_BF16
  bool nhwc;                // DXR_OUT_NHWC
  bool conv1x1;
  int radius;
  LookupLaunch launch;
  Levels L;                 // the pyramid's layout
};

// Status of a pyramid lookup request and, for DXR_OK, its plan.  The order of
// the checks is the contract: a request that is both invalid and unsupported
// answers what comes first here.
inline int plan_lookup(const LookupRequest& r, LookupPlan* p) {
  p->unit = LOOKUP_UNIT_NONE;
  p->cells = r.pyr_dtype;
  p->out_flag = 0;
  p->nhwc = false;
  p->conv1x1 = r.conv1x1;
  p->radius = r.radius;
  p->launch = LookupLaunch{SHAPE_NONE, 0, 0, 0, 0};
  // The flags on pyr_dtype.  A flagged value must carry a cell type in its low
  // byte and a 16-bit `out` must be 2-byte aligned; an unflagged value passes
  // through to the cell type check, the last one.
  if ((r.pyr_dtype & ~0xff) != 0) {
    if (!split_out_flags(&p->cells, &p->out_flag, &p->nhwc)) return DXR_EINVAL;
    if (p->cells != DXR_F32 && p->cells != DXR_BF16 && p->cells != DXR_PYR_F16) return DXR_EINVAL;
    if (!out_aligned(p->out_flag, r.out)) return DXR_EINVAL;
  }
  if (!make_levels(r.B, r.H, r.W, r.num_levels, &p->L)) return DXR_EINVAL;
  if (r.radius < 0 || (r.conv1x1 && r.cout < 1)) return DXR_EINVAL;
  if (r.conv1x1) {
    // radius 3 or 4 and at most 4 levels: then the lookup's num_levels * (2r+1)^2
    // channels fit the kernel's staged MotionCfg<R>::KP (4 levels, padded to 16)
    if (r.radius != 3 && r.radius != 4) return DXR_EUNSUPPORTED;
    if (r.num_levels > 4 || r.cout % 32 != 0 || r.cout > 4096) return DXR_EUNSUPPORTED;
  } else if (r.radius > 8) {
    return DXR_EUNSUPPORTED;
  }
  if (r.B > 65535) return DXR_EINVAL;
  if (r.B == 0) return DXR_OK;
  if (!r.pyramid || !r.coords || !r.out || (r.conv1x1 && !r.weight_packed)) return DXR_EINVAL;
  if (p->cells != DXR_F32 && p->cells != DXR_BF16 && p->cells != DXR_PYR_F16) return DXR_EINVAL;

  const int64_t N = r.H * r.W;
  p->launch = r.conv1x1 ? conv1x1_launch(N, r.B)
                        : lookup_launch(r.radius, N, r.num_levels, r.B, cell_bytes(p->cells),
                                        level0_cells(p->L.lay[0]), p->nhwc);
  p->unit = p->nhwc                   ? LOOKUP_UNIT_NHWC
            : p->cells == DXR_PYR_F16 ? LOOKUP_UNIT_PYR16
            : p->out_flag != 0        ? LOOKUP_UNIT_OUT16
                                      : LOOKUP_UNIT_MAIN;
  return DXR_OK;
}

inline const char* lookup_unit_name(int unit) {
  switch (unit) {
    case LOOKUP_UNIT_MAIN: return "corr_lookup.hip";
    case LOOKUP_UNIT_OUT16: return "corr_lookup_out16.hip";
    case LOOKUP_UNIT_PYR16: return "corr_lookup_pyr16.hip";
    case LOOKUP_UNIT_NHWC: return "corr_lookup_nhwc.hip";
    default: return "none";
  }
}

// The kernel as the header's table spells it.
inline const char* lookup_name(const LookupPlan& p) {
  switch (p.launch.shape) {
    case SHAPE_ONE_ROUND: return "corr_lookup_qm_kernel<256 x 16>";
    case SHAPE_MULTI_ROUND:
      return p.radius <= 4 ? "corr_lookup_qm_kernel<512 x 32>" : "corr_lookup_qm_kernel<512 x 16>";
    case SHAPE_CONV_1024: return "corr_lookup_conv1x1_h2_kernel<1024>";
    case SHAPE_CONV_512: return "corr_lookup_conv1x1_h2_kernel<512>";
    default: return "none";
  }
}

// ---------------------------------------------------------------------------
// Volume lookup: dxr_alt_volume_lookup
// ---------------------------------------------------------------------------

enum VolumeUnit {
  VOLUME_UNIT_NONE = 0,
  VOLUME_UNIT_MAIN,     // corr_lookup.hip: float32 volumes, float32 NCHW out
  VOLUME_UNIT_OUT,      // corr_lookup_alt_out.hip: float32 volumes, a flagged out
  VOLUME_UNIT_VOL16     // corr_lookup_alt_vol16.hip: float16 volumes, every out
};

struct VolumeLookupRequest {
  int64_t B, H, W;
  int num_levels, first_level;
  int radius;               // DXR_ALT_VOL_F16 and the output flags still on
  float divisor;
  uintptr_t volumes, coords, out;
};

struct VolumeLookupPlan {
  int unit;                 // VolumeUnit
  int cells;                // DXR_F32, or DXR_PYR_F16 with DXR_ALT_VOL_F16
  int out_flag;
  bool nhwc;
  int radius;
  float div_recip;          // pow2_recip(divisor)
  LookupLaunch launch;
  Levels L;                 // the layout of all num_levels levels
};

inline int plan_volume_lookup(const VolumeLookupRequest& r, VolumeLookupPlan* p) {
  p->unit = VOLUME_UNIT_NONE;
  p->cells = DXR_F32;
  p->out_flag = 0;
  p->nhwc = false;
  p->radius = r.radius;
  p->div_recip = 0.f;
  p->launch = LookupLaunch{SHAPE_NONE, 0, 0, 0, 0};
  // the flags on `radius` first: DXR_ALT_VOL_F16 (float16 volume cells), then the
  // output flags; a negative radius carries none and is invalid
  if (r.radius < 0) return DXR_EINVAL;
  if (r.radius & DXR_ALT_VOL_F16) p->cells = DXR_PYR_F16;
  p->radius &= ~DXR_ALT_VOL_F16;
  if (!split_out_flags(&p->radius, &p->out_flag, &p->nhwc)) return DXR_EINVAL;
  if (!out_aligned(p->out_flag, r.out)) return DXR_EINVAL;
  if (!make_levels(r.B, r.H, r.W, r.num_levels, &p->L) || r.first_level < 0 ||
      r.first_level >= r.num_levels)
    return DXR_EINVAL;
  if (!divisor_ok(r.divisor)) return DXR_EINVAL;
  if (p->radius > 8) return DXR_EUNSUPPORTED;
  if (r.B > 65535) return DXR_EINVAL;
  if (r.B == 0) return DXR_OK;
  if (!r.volumes || !r.coords || !r.out) return DXR_EINVAL;

  p->div_recip = pow2_recip(r.divisor);
  // the pyramid lookup's shapes over the levels [first_level, num_levels),
  // without the large-pyramid exception (lookup_one_round)
  p->launch = lookup_launch(p->radius, r.H * r.W, r.num_levels - r.first_level, r.B,
                            cell_bytes(p->cells), 0, p->nhwc);
  p->unit = p->cells == DXR_PYR_F16          ? VOLUME_UNIT_VOL16
            : (p->out_flag != 0 || p->nhwc) ? VOLUME_UNIT_OUT
                                             : VOLUME_UNIT_MAIN;
  return DXR_OK;
}

inline const char* volume_unit_name(int unit) {
  switch (unit) {
    case VOLUME_UNIT_MAIN: return "corr_lookup.hip";
    case VOLUME_UNIT_OUT: return "corr_lookup_alt_out.hip";
    case VOLUME_UNIT_VOL16: return "corr_lookup_alt_vol16.hip";
    default: return "none";
  }
}

inline const char* volume_lookup_name(const VolumeLookupPlan& p) {
  switch (p.launch.shape) {
    case SHAPE_ONE_ROUND: return "corr_lookup_qm_kernel<ALT, 256 x 16>";
    case SHAPE_MULTI_ROUND:
      return p.radius <= 4 ? "corr_lookup_qm_kernel<ALT, 512 x 32>"
                           : "corr_lookup_qm_kernel<ALT, 512 x 16>";
    default: return "none";
  }
}

// ---------------------------------------------------------------------------
// On-the-fly lookup: dxr_alt_corr_lookup, _ws and _levels_ws
// ---------------------------------------------------------------------------

constexpr int TQY = 4, TQX = 8, TQ = TQY * TQX;    // the MFMA forms' query tile (32 pixels)
constexpr int ALT_MFMA_C = 256;                    // channels the query planes hold (C <= 256)
constexpr int BIN_MAX = 4096;                      // the ordered form: bins per list
constexpr int OB = 64;                             //   blocks per list

// Workspace of one list (coordinate set, level) of the ordered form: entries
// int4[NP] | bin ids int[NP] | cnt int[OB][BIN_MAX + 1] | tot int[BIN_MAX + 1] |
// cost float[OB] (16-B aligned).
struct OrderWs {
  long long np, ents, ids, cnt, tot, cost, bytes;   // byte offsets within a list
};
constexpr OrderWs order_ws(long long np) {
  OrderWs w{};
  w.np = np;
  w.ents = 0;
  w.ids = w.ents + 16 * np;
  w.cnt = w.ids + 4 * np;
  w.tot = w.cnt + 4LL * OB * (BIN_MAX + 1);
  w.cost = w.tot + 4LL * (BIN_MAX + 1);
  w.bytes = (w.cost + 4LL * OB + 15) & ~15LL;
  return w;
}

inline long long alt_order_entries(long long H, long long W) {
  return ((W + TQX - 1) / TQX) * ((H + TQY - 1) / TQY) * (long long)TQ;
}
inline long long alt_order_bytes(long long H, long long W) {
  return order_ws(alt_order_entries(H, W)).bytes;
}

// dxr_alt_workspace_bytes: the ordered form's lists for `levels` levels.
inline int64_t alt_workspace_bytes(int64_t B, int64_t H, int64_t W, int levels) {
  if (B < 0 || H < 1 || W < 1 || levels < 1 || levels > 8 || !pixels_ok(H, W)) return -1;
  return B * levels * alt_order_bytes(H, W);
}

enum AltUnit {
  ALT_UNIT_NONE = 0,
  ALT_UNIT_MAIN,        // alt_corr.hip: float32 fmaps, float32 NCHW out
  ALT_UNIT_OUT,         // alt_corr_out.hip: float32 fmaps, a flagged out
  ALT_UNIT_IN16,        // alt_corr_in16.hip: DXR_ALT_IN_F16, every out
  ALT_UNIT_INBF16       // alt_corr_inbf16.hip: DXR_ALT_IN_BF16, every out
};

enum AltForm {
  ALT_FORM_NONE = 0,
  ALT_MFMA_ORDERED,     // alt_bin_*_kernel + alt_corr_mfma_kernel on the ordered lists
  ALT_MFMA_TILE,        // alt_corr_mfma_kernel in tile order
  ALT_VALU_VEC,         // alt_corr_kernel, float4 loads
  ALT_VALU_SCALAR
};

// The kernel form.  MFMA: C a multiple of 16 (k16 steps) up to 256, 16-byte
// aligned rows (`aligned`: C % 4 == 0, fmap1 and every level 16-byte aligned), on
// the ordered lists when there is a workspace; the per-query VALU form
// otherwise, with float4 loads when aligned.  Also the rule of the reference FFI
// dxr_alt_corr_forward (no workspace).
inline int alt_form(bool aligned, int64_t C, bool workspace) {
  if (aligned && C % 16 == 0 && C <= ALT_MFMA_C) return workspace ? ALT_MFMA_ORDERED : ALT_MFMA_TILE;
  return aligned ? ALT_VALU_VEC : ALT_VALU_SCALAR;
}
inline bool alt_form_is_mfma(int form) { return form == ALT_MFMA_ORDERED || form == ALT_MFMA_TILE; }

struct AltLookupRequest {
  int64_t B, H, W, C;
  int num_levels;
  int n_levels;             // < 0: every level; else the levels [0, n_levels)
  bool levels_call;         // dxr_alt_corr_lookup_levels_ws: n_levels < 1 is invalid
  int radius;               // the input and output flags still on
  float divisor;
  uintptr_t fmap1, fmap2_levels, coords, out;
  uintptr_t level[8];       // fmap2_levels[l], read by plan_alt_form only
  uintptr_t workspace;
  int64_t workspace_bytes;
};

struct AltLookupPlan {
  int unit;                 // AltUnit
  int form;                 // AltForm
  int out_flag;
  bool nhwc;
  int radius;
  int levels;               // levels the call computes
  bool use_workspace;       // the ordered form runs on `workspace`
  float div_recip;          // pow2_recip(divisor)
  Levels L;
};

// First half: every check before the level pointers are looked at.  DXR_OK with
// r.B > 0: go on with plan_alt_form, once level[0 .. p->levels) are filled in
// (the array itself is non-null then).
inline int plan_alt_args(const AltLookupRequest& r, AltLookupPlan* p) {
  p->unit = ALT_UNIT_NONE;
  p->form = ALT_FORM_NONE;
  p->out_flag = 0;
  p->nhwc = false;
  p->radius = r.radius;
  p->levels = 0;
  p->use_workspace = false;
  p->div_recip = 0.f;
  // the flags on `radius` first — an invalid combination is DXR_EINVAL before
  // anything else, n_levels < 1 included; a negative radius carries none and is invalid
  if (r.radius < 0) return DXR_EINVAL;
  const bool in16 = (r.radius & DXR_ALT_IN_F16) != 0, inbf = (r.radius & DXR_ALT_IN_BF16) != 0;
  if (in16 && inbf) return DXR_EINVAL;   // one input dtype
  p->radius &= ~(DXR_ALT_IN_F16 | DXR_ALT_IN_BF16);
  if (!split_out_flags(&p->radius, &p->out_flag, &p->nhwc)) return DXR_EINVAL;
  if (r.levels_call && r.n_levels < 1) return DXR_EINVAL;
  if (!out_aligned(p->out_flag, r.out)) return DXR_EINVAL;
  if (!make_levels(r.B, r.H, r.W, r.num_levels, &p->L)) return DXR_EINVAL;
  if (r.n_levels > r.num_levels || r.n_levels == 0) return DXR_EINVAL;
  if (r.C < 1 || !divisor_ok(r.divisor)) return DXR_EINVAL;
  if (p->radius > 6) return DXR_EUNSUPPORTED;
  if (r.B > 65535 || r.C > (1 << 20)) return DXR_EINVAL;
  if (r.B == 0) return DXR_OK;
  if (!r.fmap1 || !r.fmap2_levels || !r.coords || !r.out) return DXR_EINVAL;
  p->levels = r.n_levels < 0 ? r.num_levels : r.n_levels;
  p->unit = inbf                             ? ALT_UNIT_INBF16
            : in16                           ? ALT_UNIT_IN16
            : (p->out_flag != 0 || p->nhwc) ? ALT_UNIT_OUT
                                             : ALT_UNIT_MAIN;
  return DXR_OK;
}

// Second half: the level pointers, the kernel form and the workspace.
inline int plan_alt_form(const AltLookupRequest& r, AltLookupPlan* p) {
  const int unit = p->unit;
  p->unit = ALT_UNIT_NONE;
  bool vec = r.C % 4 == 0 && aligned16(r.fmap1);
  for (int l = 0; l < p->levels; ++l) {
    if (!r.level[l]) return DXR_EINVAL;
    vec = vec && aligned16(r.level[l]);
  }
  // With a workspace the queries are ordered first (alt_bin_*_kernel): non-null,
  // 16-byte aligned and at least dxr_alt_workspace_bytes for the levels computed
  // (anything less counts as none).
  const bool ws = r.workspace != 0 && aligned16(r.workspace) &&
                  r.workspace_bytes >= alt_workspace_bytes(r.B, r.H, r.W, p->levels);
  const int form = alt_form(vec, r.C, ws);
  // The MFMA forms implement every flag combination; the VALU forms decline a
  // flagged request (input or output flag; nothing launched): a caller runs the
  // unflagged call and converts.
  if (!alt_form_is_mfma(form) && unit != ALT_UNIT_MAIN) return DXR_EUNSUPPORTED;
  p->form = form;
  p->use_workspace = form == ALT_MFMA_ORDERED;
  p->div_recip = pow2_recip(r.divisor);
  p->unit = unit;
  return DXR_OK;
}

// Both halves, for a caller that holds the level pointers already.
inline int plan_alt_lookup(const AltLookupRequest& r, AltLookupPlan* p) {
  const int st = plan_alt_args(r, p);
  return st != DXR_OK || r.B == 0 ? st : plan_alt_form(r, p);
}

inline const char* alt_unit_name(int unit) {
  switch (unit) {
    case ALT_UNIT_MAIN: return "alt_corr.hip";
    case ALT_UNIT_OUT: return "alt_corr_out.hip";
    case ALT_UNIT_IN16: return "alt_corr_in16.hip";
    case ALT_UNIT_INBF16: return "alt_corr_inbf16.hip";
    default: return "none";
  }
}

inline const char* alt_lookup_name(const AltLookupPlan& p) {
  switch (p.form) {
    case ALT_MFMA_ORDERED: return "alt_bin_*_kernel + alt_corr_mfma_kernel<ordered>";
    case ALT_MFMA_TILE: return "alt_corr_mfma_kernel<tile order>";
    case ALT_VALU_VEC: return "alt_corr_kernel<vec>";
    case ALT_VALU_SCALAR: return "alt_corr_kernel<scalar>";
    default: return "none";
  }
}

}  // namespace dxr
