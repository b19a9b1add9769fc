// Stage (d): on-the-fly ("alternate") correlation lookup — no O((HW)^2) volume.
//
// Replaces alt_cuda_corr/correlation_kernel.cu:18-119 (corr_forward_kernel) +
// :260-286 (corr_cuda_forward), reached through alt_cuda_corr/correlation.cpp:23-33,
// and the Python loop around it, core/corr.py:74-91 (AlternateCorrBlock.__call__).
//
// Semantics (restated from correlation_kernel.cu:59-114): for a query pixel with
// level coordinate (x, y), x0 = floor(x), dx = x - x0 (same for y), the (2r+2)^2
// integer cells (h2, w2) = (y0 - r + iy, x0 - r + ix), iy, ix in [0, 2r+1], each
// get s = <fmap1[q], fmap2[h2, w2]> (0 outside the map), and output channel
// oy + (2r+1)*ox receives the bilinear combination of cells (oy..oy+1, ox..ox+1):
//   s(oy,ox)(1-dy)(1-dx) + s(oy,ox+1)(1-dy)dx + s(oy+1,ox)dy(1-dx) + s(oy+1,ox+1)dy dx
// i.e. bilinear sampling at (x - r + ox, y - r + oy) of the implicit correlation.
//
// MI355X mapping.  A workgroup owns 64 consecutive query pixels of one
// (pair, level).  Each wave takes one query at a time: lane L holds channels
// [4L, 4L+4) (+256 m) of fmap1[q] in registers and reads, per cell, the 16-byte
// slice of fmap2[cell] — one fully coalesced 1 KiB wave load per cell vector.
// Partial dot products of 16 cells are reduced across the wave by a 17-shuffle
// butterfly transpose (each lane ends with one cell's sum), cell sums go to LDS,
// and after one barrier every thread emits outputs for one query with coalesced
// 256-byte wave stores along the query dimension.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include <type_traits>

#include "dxr_common.h"
#include "mfma_operands.h"
#include "out_store.h"

namespace {

using dxr::f32x16_t;
using dxr::bf16x8_t;
using dxr::f16x8_t;
using dxr::f16x2_t;
using dxr::cvt_pk_f16;
using dxr::lds_void_t;
using dxr::Bf16Split;
using dxr::Split2;
using dxr::split2_f16;
using dxr::split8_f16;
using dxr::split8_bf16;

struct AltLevel {
  const float* f2;        // [Bf, H2, W2, C]
  int H2, W2;
  float inv;              // coordinate scale (1 / 2^l)
  int ch_off;             // first output channel of this level
};

struct AltGeom {
  int N;                  // query pixels per coordinate set (H1 * W1)
  int C;
  int Nc;                 // coordinate sets per pair (reference FFI); 1 for the fused form
  int cout;               // channels per output image
  float divisor;
  float div_recip = 0.f;  // 1 / divisor when divisor is a power of two (exact), else 0
  long long f1_bstride;   // H1 * W1 * C
  long long coord_zstride, coord_cstride, coord_qstride;
  AltLevel lv[8];
  dxr::LevelLayout vlay{};  // FULL: the volume's paged level layout (offset from the volume buffer)
  unsigned f16_levels = 0;  // IN16: bit l set: lv[l].f2 points at float16 (INBF: bfloat16) cells
};

template <int R>
struct Cells {
  static constexpr int RD = 2 * R + 1;
  static constexpr int RD1 = RD + 1;
  static constexpr int NCELL = RD1 * RD1;
  static constexpr int NB = (NCELL + 15) / 16;   // 16-cell batches
  static constexpr int LD = NCELL + 1;           // LDS row pitch (odd: no bank aliasing)
};

template <int R, bool VEC>
__global__ __launch_bounds__(256) void alt_corr_kernel(const float* __restrict__ f1,
                                                       const float* __restrict__ coords,
                                                       float* __restrict__ out, AltGeom g) {
  using CL = Cells<R>;
  constexpr int RD = CL::RD, RD1 = CL::RD1, NCELL = CL::NCELL;
  __shared__ float cells[64 * CL::LD];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.x * 64;
  const AltLevel lv = g.lv[blockIdx.y];
  const int z = blockIdx.z;           // coordinate-set index (b * Nc + n)
  const int bf = z / g.Nc;            // fmap batch index
  const float* cz = coords + (long long)z * g.coord_zstride;
  const float* f1b = f1 + (long long)bf * g.f1_bstride;
  const float* f2b = lv.f2 + (long long)bf * lv.H2 * lv.W2 * g.C;
  const int nslab = VEC ? (g.C + 255) / 256 : (g.C + 63) / 64;

  for (int qq = wave; qq < 64; qq += 4) {
    const int q = q0 + qq;
    if (q >= g.N) break;  // wave-uniform
    const float x = cz[(long long)q * g.coord_qstride] * lv.inv;
    const float y = cz[(long long)q * g.coord_qstride + g.coord_cstride] * lv.inv;
    const float xf = floorf(x), yf = floorf(y);
    const bool near = fabsf(xf) < 1.0e8f && fabsf(yf) < 1.0e8f;
    const int xb = near ? (int)xf - R : -(1 << 28);
    const int yb = near ? (int)yf - R : -(1 << 28);

    for (int cb = 0; cb < CL::NB; ++cb) {
      float p[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) p[i] = 0.f;
      for (int m = 0; m < nslab; ++m) {
        if constexpr (VEC) {
          const int c = 4 * lane + 256 * m;
          if (c < g.C) {
            const float4 a = *reinterpret_cast<const float4*>(f1b + (long long)q * g.C + c);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              const int cell = cb * 16 + i;
              if (cell < NCELL) {
                const int hh = yb + cell / RD1, ww = xb + cell % RD1;
                if ((unsigned)hh < (unsigned)lv.H2 && (unsigned)ww < (unsigned)lv.W2) {
                  const float4 v = *reinterpret_cast<const float4*>(
                      f2b + ((long long)hh * lv.W2 + ww) * g.C + c);
                  p[i] += a.x * v.x + a.y * v.y + a.z * v.z + a.w * v.w;
                }
              }
            }
          }
        } else {
          const int c = lane + 64 * m;
          if (c < g.C) {
            const float a = f1b[(long long)q * g.C + c];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              const int cell = cb * 16 + i;
              if (cell < NCELL) {
                const int hh = yb + cell / RD1, ww = xb + cell % RD1;
                if ((unsigned)hh < (unsigned)lv.H2 && (unsigned)ww < (unsigned)lv.W2)
                  p[i] += a * f2b[((long long)hh * lv.W2 + ww) * g.C + c];
              }
            }
          }
        }
      }
      // Butterfly transpose-reduce: 16 partials x 64 lanes -> one cell per lane.
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const bool hi = lane & 32;
        const float send = hi ? p[i] : p[i + 8], keep = hi ? p[i + 8] : p[i];
        p[i] = keep + __shfl_xor(send, 32);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool hi = lane & 16;
        const float send = hi ? p[i] : p[i + 4], keep = hi ? p[i + 4] : p[i];
        p[i] = keep + __shfl_xor(send, 16);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const bool hi = lane & 8;
        const float send = hi ? p[i] : p[i + 2], keep = hi ? p[i + 2] : p[i];
        p[i] = keep + __shfl_xor(send, 8);
      }
      {
        const bool hi = lane & 4;
        const float send = hi ? p[0] : p[1], keep = hi ? p[1] : p[0];
        p[0] = keep + __shfl_xor(send, 4);
      }
      p[0] += __shfl_xor(p[0], 2);
      p[0] += __shfl_xor(p[0], 1);
      const int cell = cb * 16 + ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 +
                       ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1);
      if ((lane & 3) == 0 && cell < NCELL) cells[qq * CL::LD + cell] = p[0];
    }
  }
  __syncthreads();

  // Output phase: thread -> (query = tid % 64, x-offset class = tid / 64).
  const int qq = tid & 63;
  const int q = q0 + qq;
  if (q >= g.N) return;
  const float x = cz[(long long)q * g.coord_qstride] * lv.inv;
  const float y = cz[(long long)q * g.coord_qstride + g.coord_cstride] * lv.inv;
  const float dx = x - floorf(x), dy = y - floorf(y);
  const float* s = cells + qq * CL::LD;
  float* o = out + (long long)z * g.cout * g.N + (long long)lv.ch_off * g.N + q;
  for (int ox = wave; ox < RD; ox += 4) {
#pragma unroll
    for (int oy = 0; oy < RD; ++oy) {
      // Reference accumulation order: se, sw, ne, nw (cell loop iy-major, ix-minor).
      const float s00 = s[oy * RD1 + ox], s01 = s[oy * RD1 + ox + 1];
      const float s10 = s[(oy + 1) * RD1 + ox], s11 = s[(oy + 1) * RD1 + ox + 1];
      float v = __fmul_rn(__fmul_rn(s00, 1.f - dy), 1.f - dx);
      v = __fadd_rn(v, __fmul_rn(__fmul_rn(s01, 1.f - dy), dx));
      v = __fadd_rn(v, __fmul_rn(__fmul_rn(s10, dy), 1.f - dx));
      v = __fadd_rn(v, __fmul_rn(__fmul_rn(s11, dy), dx));
      o[(long long)(oy + RD * ox) * g.N] = v / g.divisor;
    }
  }
}

// ---------------------------------------------------------------------------
// MFMA form (default when C % 16 == 0, C <= 256).  A workgroup owns a 4 x 8
// tile of query pixels and one level.  The queries' (2r+2)^2 windows overlap,
// so it computes the dot products of its 32 queries with every cell of the
// windows' union bounding box (clipped to the level) as a small GEMM on the
// matrix cores, cells x queries x C, and keeps the entries that fall in each
// query's own window.  Every fmap2 cell vector is then read once per workgroup
// instead of once per query (the per-query form above re-reads 100 cell vectors
// per query: 6.7 GB per 1080p lookup, 1.37 ms).  f32 class: both operands are
// split into f16 pairs (as the split build, csrc/corr_build.hip; r01: a 3-way
// bf16 split with six products, still the overflow fallback) and accumulated in
// f32; the query planes are split once into LDS, cell vectors in registers as
// they arrive (one k step ahead).  Box
// cells are walked in chunks of 4 waves x 32*NRB.  The bilinear combination and
// the output follow the per-query form exactly.
// ---------------------------------------------------------------------------
// query tile (TQY x TQX = TQ = 32 pixels) and the channels the query planes hold
// (C <= ALT_MFMA_C): lookup_plan.h, with the rule that picks the MFMA forms
using dxr::TQY;
using dxr::TQX;
using dxr::TQ;
using dxr::ALT_MFMA_C;

// The f16 pair split (3 f16 products, cross terms in a second accumulator), as
// the split build; a chunk whose sums are not finite (an operand beyond f16
// range, or inf/NaN) is recomputed by its wave on the 3-way bf16 split, with
// the query operand split from fmap1 in registers.
// BIN: the workgroup's 32 queries are not a 4 x 8 pixel tile but 32 consecutive
// entries of `ord` — this coordinate set's and level's query list in the order
// alt_bin_*_kernel chose (grouped by window position, or the tile order), each
// entry {query, x, y, -} carrying the query's coordinates, so a workgroup's
// first global read gives it both.
// PF: k steps of cell-vector loads kept in flight (a ring of PF register stages).
// XP (experiments only; 0 in the product): bit 0 feeds the cell vectors' raw
// bits to the f16 MFMAs instead of splitting them (and skips the non-finite
// fallback) — a timing ablation of the split's VALU work, results meaningless;
// bit 1 stores only outputs that are exactly 12345.0 (none: an ablation of the
// output stores).
// FULL (round 6, the coarse-level volumes of dxr_alt_coarse_volumes): the box is
// the whole level and every (cell, query) sum is stored, raw (not divided), into
// `out` in the pyramid's paged layout of that level (g.vlay, dxr_common.h
// cell_index): the same products in the same order as the windowed form, so a
// lookup that reads its windows from the volume reproduces the on-the-fly
// outputs bit for bit (finite operands inside the f16 pair's range; a chunk with
// a non-finite sum is recomputed on the bf16 split in either form, and chunks
// group different cells in the two forms).  Tile order only (BIN = false);
// coordinates are not read.
// OUTX (alt_corr_out.hip only): the flagged output forms of the lookup — `okind`
// bit 0: float16 elements, bit 1: bfloat16 (DXR_OUT_F16 / DXR_OUT_BF16: the
// float32 result converted in the store, out_store.h), bit 2: channels-last
// (DXR_OUT_NHWC: element (z, ch, q) at (z N + q) cout + ch).  Everything up to
// the bilinear combination is the float32 NCHW form's code; without OUTX `okind`
// is not read and the kernel is the one it was.
// IN16 (alt_corr_in16.hip only; DXR_ALT_IN_F16): `f1` points at float16 rows and
// so do the levels of g.f16_levels (level 0: the encoder's own map; the pooled
// levels are means of four values, not float16 numbers, and stay float32).  A
// float16 value's f16 pair is (its own bits, 0), so the query rows are copied
// raw into one LDS plane (no split, NPL = 1) and
//   - a float16 level's 16-byte cell load is the A operand itself: one product
//     per k step (th qh), no fallback (IEEE arithmetic on the raw values);
//   - a float32 level splits its cells as ever and issues two (tl qh, th qh);
//     th ql multiplied by zero.  Its fallback widens the query row in registers.
// The products kept are issued in the float32 form's k order, so with finite
// fmaps every sum is the one the float32 form gives on the widened values
// (dropped MFMAs added exact zeros; only a zero's sign can differ).  The level is
// blockIdx.y: the branch is uniform per workgroup.  Without IN16 the kernel is
// the one it was.
// INBF (alt_corr_inbf16.hip only; DXR_ALT_IN_BF16; with IN16, whose 16-bit
// plumbing it shares: the raw query plane, the 16-byte cell loads, the ring):
// the 16-bit values are bfloat16.  8-bit significands multiply exactly into the
// f32 accumulator and bfloat16 has float32's exponent range, so nothing is split,
// scaled or recomputed:
//   - a bfloat16 level: one v_mfma_f32_32x32x16_bf16 per k step on the raw
//     cell vector and the raw query;
//   - a float32 level: its cells split three ways by split8_bf16<GUARD_INF> (exact: 3 x 8
//     bits), each part times the raw bfloat16 query — three exact products
//     (tl q, tm q, th q: small terms first), no query parts; inf and NaN go
//     through the split as in the float32 form's fallback, so no second pass.
// Without INBF no statement of it is compiled.
template <int R, int MINW = 2, bool BIN = false, int PF = 1, int DMA = 0, int XP = 0,
          bool FULL = false, bool OUTX = false, bool IN16 = false, bool INBF = false>
__global__ __launch_bounds__(256, MINW) void alt_corr_mfma_kernel(const float* __restrict__ f1,
                                                               const float* __restrict__ coords,
                                                               float* __restrict__ out,
                                                               AltGeom g, int W1, int tiles_x,
                                                               const int4* __restrict__ ord,
                                                               long long ord_stride, int XL,
                                                               int okind) {
  static_assert(!OUTX || (!FULL && XP == 0), "flagged outputs: the product lookup only");
  static_assert(!IN16 || (!FULL && XP == 0 && DMA == 0), "float16 fmaps: the product lookup only");
  static_assert(!INBF || IN16, "bfloat16 fmaps: a kind of the 16-bit operand form");
  constexpr int RD = 2 * R + 1, RD1 = RD + 1, NCELL = RD1 * RD1;
  // 32-cell blocks per wave and chunk.  Always 1 (the DMA forms stage one block
  // per wave); the [NRB] arrays and rb loops below stay as they are because
  // flattening them changes the register allocation of every instantiation.
  constexpr int NRB = 1;
  constexpr int CHUNK = 4 * 32 * NRB;                       // box cells per chunk
  constexpr int KB = ALT_MFMA_C / 8;                        // 8-channel blocks
  constexpr int NPL = IN16 ? 1 : 2;                         // query operand planes
  // (IN16 with OUTX: at least the channels-last stage of the last phase, which one
  // plane does not hold from r = 6)
  constexpr int QPU = (IN16 && OUTX && TQ * (RD * RD | 1) * 4 > NPL * KB * TQ * 16)
                          ? (TQ * (RD * RD | 1) * 4 + 15) / 16 : NPL * KB * TQ;
  __shared__ __attribute__((aligned(16))) uint4 qplanes[QPU];           // [plane][kb][q]
  // window dot products, row pitch SP: odd (round 6), so the 32 lanes of a
  // half-wave reading S[q * SP + cell] for 32 queries hit 32 banks (pitch 100:
  // 4 q mod 32, a 4-way conflict on every phase-2 read).  XP bit 4: the old pitch.
  constexpr int SP = (XP & 16) ? NCELL : NCELL + 1;
  __shared__ float S[TQ * SP];
  __shared__ int4 qinfo[TQ];                                // {x0, y0, live, -}
  __shared__ int box[4];                                    // bx0, by0, bw, bh
  __shared__ int qlist[TQ];                                 // BIN: query index or -1
  __shared__ float2 qxy[TQ];                                // BIN: its coordinates
  // DMA 1: per wave two 4 KB buffers of 32 cells x 128 B (two k steps), swizzled 16-B slots;
  // DMA 2: per wave a ring of 4 one-k-step stages of 32 cells x 64 B (round 6)
  __shared__ __attribute__((aligned(16))) unsigned char cbuf[DMA ? 4 * 2 * 4096 : 16];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // Workgroups are dealt round-robin to the 8 XCDs; XCD k takes the k-th
  // contiguous band of tiles instead, so neighbouring tiles (whose boxes overlap)
  // share one L2 (the bijection of csrc/corr_build.hip's banded_coord; r01 1080p:
  // FETCH 424 -> 162 MB per lookup).  XL (levels dividing 8, levels x tiles a
  // multiple of 8): the XCDs are shared out by level too — 8 / levels XCDs per
  // level, each taking a contiguous band of that level's list — so one output
  // line (32 pixels of one channel, written by the workgroups holding those
  // pixels' queries) is written from one or two XCDs' L2s: with queries ordered
  // by window position a line's 32 queries sit in bins of several bands, and
  // partial dirty lines written back from several L2s multiplied the output's
  // write traffic (r03 1080p: WRITE 137 MB per lookup for a 42 MB output).
  // Measured slower (the levels cost different amounts): experiments only.
  int tile = blockIdx.x, lvl = blockIdx.y;
  if (XL) {
    const int T = gridDim.x, L = gridDim.y;
    const int lin = blockIdx.x + T * blockIdx.y, xcd = lin % 8, k = lin / 8;
    const int xpl = 8 / L;
    lvl = xcd / xpl;
    tile = (xcd % xpl) * (T / xpl) + k;
  } else {
    const int n = gridDim.x, q8 = n / 8, r8 = n % 8, xcd = tile % 8;
    tile = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + tile / 8;
  }
  const int tx = tile % tiles_x, ty = tile / tiles_x;
  const AltLevel lv = g.lv[lvl];
  const int z = blockIdx.z, bf = z / g.Nc;
  const float* cz = coords + (long long)z * g.coord_zstride;
  const float* f1b = f1 + (long long)bf * g.f1_bstride;
  const float* f2b = lv.f2 + (long long)bf * lv.H2 * lv.W2 * g.C;
  // IN16: the float16 views of the same operands; lvh: this level's cells are float16
  const _Float16* f1h = reinterpret_cast<const _Float16*>(f1) + (long long)bf * g.f1_bstride;
  const _Float16* f2h = reinterpret_cast<const _Float16*>(lv.f2) + (long long)bf * lv.H2 * lv.W2 * g.C;
  const bool lvh = IN16 && ((g.f16_levels >> lvl) & 1u) != 0;
  const int H1 = g.N / W1;
  const int nkb = g.C / 8;
  // query of lane/slot qq: a pixel of the 4 x 8 tile, or (BIN) entry tile*32 + qq of
  // the sorted list; -1 past the image / the list
  auto query_of = [&](int qq) -> int {
    if constexpr (BIN) {
      return qlist[qq];
    } else {
      const int qy = ty * TQY + qq / TQX, qx = tx * TQX + qq % TQX;
      return (qy < H1 && qx < W1) ? qy * W1 + qx : -1;
    }
  };
  if constexpr (BIN) {
    if (tid < TQ) {
      // per (coordinate set, level) gridDim.x * 32 entries, query -1 = padding
      const int4 e = ord[((long long)z * gridDim.y + lvl) * ord_stride + tile * TQ + tid];
      qlist[tid] = e.x;
      qxy[tid] = make_float2(__int_as_float(e.y), __int_as_float(e.z));
    }
    __syncthreads();
  }

  // ---- query coordinates, window origins, the windows' union box
  if constexpr (FULL) {
    static_assert(!BIN, "the full-level box runs in tile order");
    if (tid < TQ) qinfo[tid] = make_int4(0, 0, 0, 0);
    if (tid == 0) {
      box[0] = 0;
      box[1] = 0;
      box[2] = lv.W2;
      box[3] = lv.H2;
    }
  } else if (tid < TQ) {
    const int qsel = query_of(tid);
    int x0 = 0, y0 = 0, live = 0;
    if (qsel >= 0) {
      const int q = qsel;
      float x, y;
      if constexpr (BIN) {
        x = qxy[tid].x * lv.inv;
        y = qxy[tid].y * lv.inv;
      } else {
        x = cz[(long long)q * g.coord_qstride] * lv.inv;
        y = cz[(long long)q * g.coord_qstride + g.coord_cstride] * lv.inv;
      }
      const float xf = floorf(x), yf = floorf(y);
      if (fabsf(xf) < 1.0e8f && fabsf(yf) < 1.0e8f) {
        x0 = (int)xf - R;
        y0 = (int)yf - R;
        // windows entirely off the level need no dot products
        live = (x0 + RD1 > 0 && x0 < lv.W2 && y0 + RD1 > 0 && y0 < lv.H2) ? 1 : 0;
      }
    }
    qinfo[tid] = make_int4(x0, y0, live, 0);
    int lx0 = live ? max(x0, 0) : 0x7fffffff, ly0 = live ? max(y0, 0) : 0x7fffffff;
    int lx1 = live ? min(x0 + RD1, lv.W2) : -1, ly1 = live ? min(y0 + RD1, lv.H2) : -1;
#pragma unroll
    for (int o = 1; o < TQ; o <<= 1) {
      lx0 = min(lx0, __shfl_xor(lx0, o));
      ly0 = min(ly0, __shfl_xor(ly0, o));
      lx1 = max(lx1, __shfl_xor(lx1, o));
      ly1 = max(ly1, __shfl_xor(ly1, o));
    }
    if (tid == 0) {
      const bool any = lx1 > lx0;
      box[0] = any ? lx0 : 0;
      box[1] = any ? ly0 : 0;
      box[2] = any ? lx1 - lx0 : 0;
      box[3] = any ? ly1 - ly0 : 0;
    }
  }
  if constexpr (!FULL)
    for (int i = tid; i < TQ * SP; i += 256) S[i] = 0.f;
  // query operand planes: unit (kb, q) -> f1[q][8 kb .. 8 kb + 8), split once
  for (int u = tid; u < nkb * TQ; u += 256) {
    const int kb = u / TQ, qq = u - kb * TQ;
    int qsrc0;   // padding slots read a valid query (their outputs are not stored)
    if constexpr (BIN) {
      qsrc0 = max(query_of(qq), 0);
    } else {
      const int qy = min(ty * TQY + qq / TQX, H1 - 1), qx = min(tx * TQX + qq % TQX, W1 - 1);
      qsrc0 = qy * W1 + qx;
    }
    if constexpr (IN16) {   // the float16 row is the operand
      qplanes[kb * TQ + qq] = *reinterpret_cast<const uint4*>(f1h + (long long)qsrc0 * g.C + kb * 8);
      continue;
    }
    const float* src = f1b + (long long)qsrc0 * g.C + kb * 8;
    const float4 a = *reinterpret_cast<const float4*>(src);
    const float4 c = *reinterpret_cast<const float4*>(src + 4);
    const float x[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
    uint4 h, l;
    split8_f16(x, h, l);
    qplanes[(0 * KB + kb) * TQ + qq] = h;
    qplanes[(1 * KB + kb) * TQ + qq] = l;
  }
  __syncthreads();

  const int bx0 = box[0], by0 = box[1], bw = box[2], bh = box[3];
  // c / bw for box cells (c < 2^24): a float estimate corrected to the exact quotient
  const float rbw = 1.f / (float)max(bw, 1);
  auto divbw = [&](int c) -> int {
    int q = (int)((float)c * rbw);
    q -= (q * bw > c) ? 1 : 0;
    q += ((q + 1) * bw <= c) ? 1 : 0;
    return q;
  };
  const int ncells = bw * bh;
  const int j = lane & 31, kh = lane >> 5;
  const int4 qi = qinfo[j];                   // this lane's accumulator column (query j)
  for (int c0 = 0; c0 < ncells; c0 += CHUNK) {
    f32x16_t acc[NRB];
    const float* src[NRB];
    const _Float16* srch[NRB];   // IN16, a float16 level
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) {
      // A operand lane -> cell c0 + 32 (wave NRB + rb) + j, channels 8 kh .. + 8 per k16
      const int c = min(c0 + (wave * NRB + rb) * 32 + j, ncells - 1);
      const int cy = divbw(c), cx = c - cy * bw;
      src[rb] = f2b + ((long long)(by0 + cy) * lv.W2 + bx0 + cx) * g.C + 8 * kh;
      if constexpr (IN16) srch[rb] = f2h + ((long long)(by0 + cy) * lv.W2 + bx0 + cx) * g.C + 8 * kh;
      if constexpr ((XP & 4) != 0) src[rb] = f2b + (long long)(j & 7) * g.C + 8 * kh;   // ablation: 8 hot cells
    }
    // DMA (f16 pair form): the wave's 32 cell vectors move by LDS-DMA, two k steps (128 B per cell)
    // per batch into a double-buffered wave region: an instruction covers 8 cells x 128 B (8 lanes
    // per cell: 8 line segments instead of the 32 cells x 32 B of a register load), and slot
    // s of cell row r holds logical 16-B piece s ^ ((r >> 1) & 7), so the operand reads below
    // (row j, pieces 4 step + 2 kh, + 1) are conflict-free ds_read_b128.  Same operands, same
    // split, same products in the same order: bit-identical to the register form.
    auto kloop_dma = [&]() {
      f32x16_t acc2 = {};
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][r] = 0.f;
      const __amdgpu_buffer_rsrc_t rf = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(f2b), (short)0, lv.H2 * lv.W2 * g.C * 4, 0x00020000);
      uint32_t voff[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = 8 * i + (lane >> 3), slot = lane & 7;
        const int c = min(c0 + wave * 32 + row, ncells - 1);
        const int cy = divbw(c), cx = c - cy * bw;
        const int piece = slot ^ ((row >> 1) & 7);
        voff[i] = (uint32_t)(((by0 + cy) * lv.W2 + bx0 + cx) * g.C) * 4u + 16u * piece;
      }
      // readfirstlane: the DMA's LDS destination must be wave-uniform (an SGPR)
      unsigned char* wreg = cbuf + __builtin_amdgcn_readfirstlane(wave) * 8192;
      auto issue = [&](int bt) {
        unsigned char* dst = wreg + (bt & 1) * 4096;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rf, (lds_void_t*)(dst + i * 1024), 16, voff[i],
                                                   bt * 128, 0, 0);
      };
      const int nbt = nkb / 4;                     // batches of two k16 steps
      const int sw = (j >> 1) & 7;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      issue(0);
      for (int bt = 0; bt < nbt; ++bt) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // reads of the buffer refilled next
        if (bt + 1 < nbt) {
          issue(bt + 1);
          asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        const unsigned char* rb0 = wreg + (bt & 1) * 4096 + j * 128;
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          const int ks = 2 * bt + st;
          const int p0 = 4 * st + 2 * kh;
          const float4 a = *reinterpret_cast<const float4*>(rb0 + 16 * (p0 ^ sw));
          const float4 b = *reinterpret_cast<const float4*>(rb0 + 16 * ((p0 + 1) ^ sw));
          const f16x8_t qh = __builtin_bit_cast(f16x8_t, qplanes[(0 * KB + 2 * ks + kh) * TQ + j]);
          const f16x8_t ql = __builtin_bit_cast(f16x8_t, qplanes[(1 * KB + 2 * ks + kh) * TQ + j]);
          const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
          uint4 h, l;
          split8_f16(x, h, l);
          const f16x8_t th = __builtin_bit_cast(f16x8_t, h), tl = __builtin_bit_cast(f16x8_t, l);
          acc2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(tl, qh, acc2, 0, 0, 0);
          acc2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, ql, acc2, 0, 0, 0);
          acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, qh, acc[0], 0, 0, 0);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][r] = __builtin_fmaf(acc2[r], 0x1p-11f, acc[0][r]);
    };
    // DMA 2 (round 6, experiments): one k step (32 cells x 64 B) per stage, a ring of
    // NS = 4 stages per wave, so three k steps of cell data are in flight (DMA 1 keeps
    // one two-step batch ahead).  An instruction covers 16 cells x 64 B (4 lanes per
    // cell); physical slot p of cell row r holds logical 16-B piece p ^ ((r >> 2) & 3),
    // so the fragment reads (row j, pieces 2 kh, 2 kh + 1) are conflict-free
    // ds_read_b128.  Same operands, split and products: bit-identical.
    auto kloop_dma2 = [&]() {
      constexpr int NS = 4;
      f32x16_t acc2 = {};
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][r] = 0.f;
      const __amdgpu_buffer_rsrc_t rf = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(f2b), (short)0, lv.H2 * lv.W2 * g.C * 4, 0x00020000);
      uint32_t voff[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = 16 * i + (lane >> 2), slot = lane & 3;
        const int c = min(c0 + wave * 32 + row, ncells - 1);
        const int cy = divbw(c), cx = c - cy * bw;
        const int piece = slot ^ ((row >> 2) & 3);
        voff[i] = (uint32_t)(((by0 + cy) * lv.W2 + bx0 + cx) * g.C) * 4u + 16u * piece;
      }
      unsigned char* wreg = cbuf + __builtin_amdgcn_readfirstlane(wave) * (NS * 2048);
      auto issue = [&](int ks) {
        unsigned char* dst = wreg + (ks % NS) * 2048;
#pragma unroll
        for (int i = 0; i < 2; ++i)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rf, (lds_void_t*)(dst + i * 1024), 16, voff[i],
                                                   ks * 64, 0, 0);
      };
      const int nst = nkb / 2;
      const int sw = (j >> 2) & 3;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
      for (int u = 0; u < NS - 1; ++u)
        if (u < nst) issue(u);
      for (int ks = 0; ks < nst; ++ks) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // reads of the slot refilled next
        if (ks + NS - 1 < nst) {
          issue(ks + NS - 1);
          asm volatile("s_waitcnt vmcnt(6)" ::: "memory");   // stage ks landed (3 stages behind it)
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        const unsigned char* rb0 = wreg + (ks % NS) * 2048 + j * 64;
        const float4 a = *reinterpret_cast<const float4*>(rb0 + 16 * ((2 * kh) ^ sw));
        const float4 b = *reinterpret_cast<const float4*>(rb0 + 16 * ((2 * kh + 1) ^ sw));
        const f16x8_t qh = __builtin_bit_cast(f16x8_t, qplanes[(0 * KB + 2 * ks + kh) * TQ + j]);
        const f16x8_t ql = __builtin_bit_cast(f16x8_t, qplanes[(1 * KB + 2 * ks + kh) * TQ + j]);
        const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        uint4 h, l;
        split8_f16(x, h, l);
        const f16x8_t th = __builtin_bit_cast(f16x8_t, h), tl = __builtin_bit_cast(f16x8_t, l);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(tl, qh, acc2, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, ql, acc2, 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, qh, acc[0], 0, 0, 0);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][r] = __builtin_fmaf(acc2[r], 0x1p-11f, acc[0][r]);
    };
    // cell vectors one k step ahead in registers
    auto kloop = [&](auto h2tag) {
      constexpr bool M2 = decltype(h2tag)::value;
      f32x16_t acc2[NRB];
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[rb][r] = acc2[rb][r] = 0.f;
      const int nst = nkb / 2;
      float4 ra[PF][NRB], rv[PF][NRB];   // ring of in-flight k steps
#pragma unroll
      for (int u = 0; u < PF; ++u)
        if (u < nst) {
#pragma unroll
          for (int rb = 0; rb < NRB; ++rb) {
            ra[u][rb] = *reinterpret_cast<const float4*>(src[rb] + u * 16);
            rv[u][rb] = *reinterpret_cast<const float4*>(src[rb] + u * 16 + 4);
          }
        }
      // fallback form: this lane's query operand straight from fmap1
      int fq;
      if constexpr (BIN) {
        fq = max(query_of(j), 0);
      } else {
        const int fqy = min(ty * TQY + j / TQX, H1 - 1), fqx = min(tx * TQX + j % TQX, W1 - 1);
        fq = fqy * W1 + fqx;
      }
      const float* qsrc = f1b + (long long)fq * g.C + 8 * kh;
      const _Float16* qsrch = f1h + (long long)fq * g.C + 8 * kh;
      for (int ks0 = 0; ks0 < nst; ks0 += PF)
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const int ks = ks0 + u;
        if (ks >= nst) break;
        float4 ca[NRB], cb[NRB];
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) {
          ca[rb] = ra[u][rb];
          cb[rb] = rv[u][rb];
        }
        if (ks + PF < nst) {
#pragma unroll
          for (int rb = 0; rb < NRB; ++rb) {
            ra[u][rb] = *reinterpret_cast<const float4*>(src[rb] + (ks + PF) * 16);
            rv[u][rb] = *reinterpret_cast<const float4*>(src[rb] + (ks + PF) * 16 + 4);
          }
        }
        if constexpr (M2) {
          const f16x8_t qh = __builtin_bit_cast(f16x8_t, qplanes[(0 * KB + 2 * ks + kh) * TQ + j]);
          // (IN16: no low plane — it would be zero — and no th ql product)
          const f16x8_t ql = __builtin_bit_cast(f16x8_t, qplanes[((IN16 ? 0 : 1) * KB + 2 * ks + kh) * TQ + j]);
#pragma unroll
          for (int rb = 0; rb < NRB; ++rb) {
            const float4 a = ca[rb], b = cb[rb];
            uint4 h, l;
            if constexpr ((XP & 1) != 0) {
              h = __builtin_bit_cast(uint4, a);
              l = __builtin_bit_cast(uint4, b);
            } else {
              const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
              split8_f16(x, h, l);
            }
            const f16x8_t th = __builtin_bit_cast(f16x8_t, h), tl = __builtin_bit_cast(f16x8_t, l);
            if constexpr ((XP & 8) != 0) {   // ablation: no MFMAs (results meaningless)
              acc[rb][0] += __uint_as_float(h.x ^ l.y) + (float)qh[0] + (float)ql[1];
            } else {
            acc2[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(tl, qh, acc2[rb], 0, 0, 0);
            if constexpr (!IN16)
              acc2[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, ql, acc2[rb], 0, 0, 0);
            acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(th, qh, acc[rb], 0, 0, 0);
            }
          }
        } else {
          bf16x8_t qh, qm, ql;
          if constexpr (INBF) {   // the raw bfloat16 query row is the B operand of all three
            qh = __builtin_bit_cast(bf16x8_t, qplanes[(2 * ks + kh) * TQ + j]);
          } else if constexpr (IN16) {   // fallback: the float16 query row, widened here
            const f16x8_t u = *reinterpret_cast<const f16x8_t*>(qsrch + ks * 16);
            const float x[8] = {(float)u[0], (float)u[1], (float)u[2], (float)u[3],
                                (float)u[4], (float)u[5], (float)u[6], (float)u[7]};
            uint4 h, m, l;
            split8_bf16<Bf16Split::GUARD_INF>(x, h, m, l);
            qh = __builtin_bit_cast(bf16x8_t, h);
            qm = __builtin_bit_cast(bf16x8_t, m);
            ql = __builtin_bit_cast(bf16x8_t, l);
          } else {     // fallback: split the query operand here
            const float4 u = *reinterpret_cast<const float4*>(qsrc + ks * 16);
            const float4 w = *reinterpret_cast<const float4*>(qsrc + ks * 16 + 4);
            const float x[8] = {u.x, u.y, u.z, u.w, w.x, w.y, w.z, w.w};
            uint4 h, m, l;
            split8_bf16<Bf16Split::GUARD_INF>(x, h, m, l);
            qh = __builtin_bit_cast(bf16x8_t, h);
            qm = __builtin_bit_cast(bf16x8_t, m);
            ql = __builtin_bit_cast(bf16x8_t, l);
          }
#pragma unroll
          for (int rb = 0; rb < NRB; ++rb) {
            const float4 a = ca[rb], b = cb[rb];
            const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            uint4 h, m, l;
            split8_bf16<Bf16Split::GUARD_INF>(x, h, m, l);
            const bf16x8_t th = __builtin_bit_cast(bf16x8_t, h), tm = __builtin_bit_cast(bf16x8_t, m),
                       tl = __builtin_bit_cast(bf16x8_t, l);
            if constexpr (INBF) {   // (q has no middle or low part)
              acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tl, qh, acc[rb], 0, 0, 0);
              acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tm, qh, acc[rb], 0, 0, 0);
              acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(th, qh, acc[rb], 0, 0, 0);
              continue;
            }
            // small terms first
            acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tm, qm, acc[rb], 0, 0, 0);
            acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tl, qh, acc[rb], 0, 0, 0);
            acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(th, ql, acc[rb], 0, 0, 0);
            acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tm, qh, acc[rb], 0, 0, 0);
            acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(th, qm, acc[rb], 0, 0, 0);
            acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(th, qh, acc[rb], 0, 0, 0);
          }
        }
      }
      if constexpr (M2) {
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[rb][r] = __builtin_fmaf(acc2[rb][r], 0x1p-11f, acc[rb][r]);
      }
    };
    // IN16, a float16 level: the cell vector's 16 bytes are the A operand; PF k
    // steps in flight, one product per step, nothing to fall back to
    auto kloop_h = [&]() {
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[rb][r] = 0.f;
      const int nst = nkb / 2;
      uint4 rh[PF][NRB];
#pragma unroll
      for (int u = 0; u < PF; ++u)
        if (u < nst) {
#pragma unroll
          for (int rb = 0; rb < NRB; ++rb)
            rh[u][rb] = *reinterpret_cast<const uint4*>(srch[rb] + u * 16);
        }
      for (int ks0 = 0; ks0 < nst; ks0 += PF)
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const int ks = ks0 + u;
        if (ks >= nst) break;
        uint4 ch[NRB];
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) ch[rb] = rh[u][rb];
        if (ks + PF < nst) {
#pragma unroll
          for (int rb = 0; rb < NRB; ++rb)
            rh[u][rb] = *reinterpret_cast<const uint4*>(srch[rb] + (ks + PF) * 16);
        }
        if constexpr (INBF) {
          const bf16x8_t qb = __builtin_bit_cast(bf16x8_t, qplanes[(2 * ks + kh) * TQ + j]);
#pragma unroll
          for (int rb = 0; rb < NRB; ++rb)
            acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, ch[rb]), qb,
                                                              acc[rb], 0, 0, 0);
          continue;
        }
        const f16x8_t qh = __builtin_bit_cast(f16x8_t, qplanes[(2 * ks + kh) * TQ + j]);
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb)
          acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, ch[rb]), qh,
                                                           acc[rb], 0, 0, 0);
      }
    };
    if constexpr (IN16) {
      if (lvh) {   // workgroup-uniform
        kloop_h();
      } else if constexpr (INBF) {   // three exact bf16 products, one pass
        kloop(std::integral_constant<bool, false>{});
      } else {
        kloop(std::integral_constant<bool, true>{});
        bool bad = false;
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
          for (int r = 0; r < 16; ++r) bad |= !(__builtin_fabsf(acc[rb][r]) <= 3.40282347e38f);
        if (__ballot(bad) != 0) kloop(std::integral_constant<bool, false>{});   // wave-uniform
      }
    } else {
      if constexpr (DMA == 2) {
        if (nkb % 2 == 0) kloop_dma2();
        else kloop(std::integral_constant<bool, true>{});
      } else if constexpr (DMA == 1) {
        if (nkb % 4 == 0) kloop_dma();
        else kloop(std::integral_constant<bool, true>{});
      } else {
        kloop(std::integral_constant<bool, true>{});
      }
      bool bad = false;
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r) bad |= !(__builtin_fabsf(acc[rb][r]) <= 3.40282347e38f);
      if ((XP & 13) == 0 && __ballot(bad) != 0)
        kloop(std::integral_constant<bool, false>{});   // wave-uniform
    }
    if constexpr (FULL) {
      // every sum of query j to its row of the volume: D rows (r & 3) + 8 (r >> 2)
      // + 4 kh, i.e. four runs of four consecutive cells per lane
      const int qv = query_of(j);
      if (qv >= 0) {
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int c = c0 + (wave * NRB + rb) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (c < ncells) {
              const int cy = divbw(c), cx = c - cy * bw;
              out[dxr::cell_index(g.vlay, bf, qv, cy, cx)] = acc[rb][r];
            }
          }
      }
      continue;
    }
    // keep the entries inside query j's window: D row = (r & 3) + 8 (r >> 2) + 4 kh
    if (qi.z) {
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = c0 + (wave * NRB + rb) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
          if (c < ncells) {
            const int cy = divbw(c), cx = c - cy * bw;
            const int iy = by0 + cy - qi.y, ix = bx0 + cx - qi.x;
            if ((unsigned)iy < (unsigned)RD1 && (unsigned)ix < (unsigned)RD1)
              S[j * SP + iy * RD1 + ix] = acc[rb][r];
          }
        }
    }
  }
  if constexpr (FULL) return;
  __syncthreads();

  if constexpr (OUTX) {
    // ---- the flagged forms: the combination below, stored as `okind` says
    const int qq = tid & (TQ - 1), cls = tid / TQ;
    const int q = query_of(qq);
    // (channels-last: padding slots stay for the barrier below, on query 0's coordinates)
    if ((okind & 4) == 0) {
      if (q < 0) return;
    }
    const int qs = max(q, 0);
    float cx, cy;
    if constexpr (BIN) {
      cx = qxy[qq].x;
      cy = qxy[qq].y;
    } else {
      cx = cz[(long long)qs * g.coord_qstride];
      cy = cz[(long long)qs * g.coord_qstride + g.coord_cstride];
    }
    // the float32 NCHW form's arithmetic (below) as the compiler issues it there,
    // instruction by instruction (out_store.h, "Pinned float32 arithmetic"): the
    // fractions c * inv - floor(c * inv) fused, 1 - d, then the combination
    const float dx = dxr::pin_fma_neg(lv.inv, cx, floorf(lv.inv * cx));
    const float dy = dxr::pin_fma_neg(lv.inv, cy, floorf(lv.inv * cy));
    const float gx = dxr::pin_sub(1.f, dx), gy = dxr::pin_sub(1.f, dy);
    const float* s = S + qq * SP;
    // `put` stores output (oy, ox) of query q
    auto combine = [&](auto&& put) {
      for (int ox = cls; ox < RD; ox += 256 / TQ) {
#pragma unroll
        for (int oy = 0; oy < RD; ++oy) {
          const float s00 = s[oy * RD1 + ox], s01 = s[oy * RD1 + ox + 1];
          const float s10 = s[(oy + 1) * RD1 + ox], s11 = s[(oy + 1) * RD1 + ox + 1];
          const float v = R == 0
              ? dxr::alt_combine_pinned_r0(s00, s01, s10, s11, dx, dy, gx, gy)
              : dxr::alt_combine_pinned<false>(s00, s01, s10, s11, dx, dy, gx, gy);
          // v / divisor; a power-of-two divisor (sqrt(256) = 16) scales exactly by its reciprocal
          const float res = g.div_recip != 0.f ? v * g.div_recip : v / g.divisor;
          put(oy, ox, res);
        }
      }
    };
    const bool f16 = (okind & 1) != 0, is16 = (okind & 3) != 0;
    auto bits16 = [&](float r) -> uint32_t {
      return f16 ? dxr::out16_bits<_Float16>(r) : dxr::out16_bits<__bf16>(dxr::bf16_nan_as_torch(r));
    };
    uint16_t* o16 = reinterpret_cast<uint16_t*>(out);
    const int bpar = dxr::out16_base_parity(o16);
    if ((okind & 4) == 0) {
      // NCHW, 16-bit elements: element (ch, q) of this set at e = (z cout + ch) N + q.
      // Lanes 2i, 2i + 1 swap their 16 bits by DPP, and where they hold queries
      // q, q + 1 (a tile row's neighbours; seldom in bin order) and the even
      // lane's element sits on a 4-byte boundary, the even lane stores one word
      // for both; every other lane stores its own 2 bytes.  No store touches a
      // byte outside its element(s).  A lane whose partner has left (padding)
      // reads its own q back and stores alone.
      const int qn = __builtin_amdgcn_update_dpp(q, q, 0xB1, 0xF, 0xF, false);
      const bool even = (lane & 1) == 0;
      const bool pair = even ? qn == q + 1 : qn == q - 1;
      const long long e0 = ((long long)z * g.cout + lv.ch_off) * g.N + q;
      combine([&](int oy, int ox, float res) {
        const long long e = e0 + (long long)(oy + RD * ox) * g.N;
        const uint32_t h = bits16(res);
        const uint32_t nb = (uint32_t)__builtin_amdgcn_update_dpp((int)h, (int)h, 0xB1, 0xF, 0xF, false);
        const long long ee = even ? e : e - 1;     // the pair's even lane's element
        const bool word = pair && (((int)(ee & 1) + bpar) & 1) == 0;
        if (!(word && !even)) dxr::store_out16_one<uint16_t, 0>(o16 + e, h, h | (nb << 16), word);
      });
      return;
    }
    // Channels-last: query q's K = (2r+1)^2 values of this level are one run at
    // (z N + q) cout + ch_off.  They are staged in LDS (the query operand planes,
    // dead after the k loops; odd pitch KP) and written with lanes along the run:
    // a wave store covers 256 consecutive bytes of a run (128 at 16 bits) and
    // goes on in the next query's.  16-bit: a lane takes one 4-byte aligned word
    // of the run (the run starts at an odd element when ch_off, cout or the base
    // make it so) and the run's first / last lone element 2 bytes.
    constexpr int K = RD * RD, KP = K | 1;
    static_assert(TQ * KP * 4 <= (int)sizeof(qplanes), "the staged runs fit the operand planes");
    float* stage = reinterpret_cast<float*>(qplanes);
    combine([&](int oy, int ox, float res) {
      if (q >= 0) stage[qq * KP + oy + RD * ox] = res;
    });
    __syncthreads();
    const long long pix0 = (long long)z * g.N;
    if (!is16) {
      for (int i = tid; i < TQ * K; i += 256) {
        const int rq = i / K, kk = i - rq * K;
        const int qr = query_of(rq);
        if (qr >= 0) out[(pix0 + qr) * g.cout + lv.ch_off + kk] = stage[rq * KP + kk];
      }
    } else {
      constexpr int NS = K / 2 + 1;   // word slots per run, either parity
      for (int i = tid; i < TQ * NS; i += 256) {
        const int rq = i / NS, sl = i - rq * NS;
        const int qr = query_of(rq);
        if (qr < 0) continue;
        const long long e = (pix0 + qr) * g.cout + lv.ch_off;   // the run's first element
        const int par = ((int)(e & 1) + bpar) & 1;
        const int k0 = 2 * sl - par, k1 = k0 + 1;
        const bool in0 = k0 >= 0 && k0 < K, in1 = k1 < K;       // k1 >= 0 always
        if (!in0 && !in1) continue;
        const float* rr = stage + rq * KP;
        const uint32_t h0 = bits16(rr[in0 ? k0 : k1]), h1 = bits16(rr[in1 ? k1 : k0]);
        if (in0 && in1) *reinterpret_cast<uint32_t*>(o16 + e + k0) = h0 | (h1 << 16);
        else if (in0) o16[e + k0] = (uint16_t)h0;
        else o16[e + k1] = (uint16_t)h1;
      }
    }
    return;
  }
  // ---- bilinear combination, as the per-query form (reference order)
  const int qq = tid & (TQ - 1), cls = tid / TQ;
  const int q = query_of(qq);
  if (q < 0) return;
  float x, y;
  if constexpr (BIN) {
    x = qxy[qq].x * lv.inv;
    y = qxy[qq].y * lv.inv;
  } else {
    x = cz[(long long)q * g.coord_qstride] * lv.inv;
    y = cz[(long long)q * g.coord_qstride + g.coord_cstride] * lv.inv;
  }
  const float dx = x - floorf(x), dy = y - floorf(y);
  const float* s = S + qq * SP;
  float* o = out + (long long)z * g.cout * g.N + (long long)lv.ch_off * g.N + q;
  for (int ox = cls; ox < RD; ox += 256 / TQ) {
#pragma unroll
    for (int oy = 0; oy < RD; ++oy) {
      const float s00 = s[oy * RD1 + ox], s01 = s[oy * RD1 + ox + 1];
      const float s10 = s[(oy + 1) * RD1 + ox], s11 = s[(oy + 1) * RD1 + ox + 1];
      float v = __fmul_rn(__fmul_rn(s00, 1.f - dy), 1.f - dx);
      v = __fadd_rn(v, __fmul_rn(__fmul_rn(s01, 1.f - dy), dx));
      v = __fadd_rn(v, __fmul_rn(__fmul_rn(s10, dy), 1.f - dx));
      v = __fadd_rn(v, __fmul_rn(__fmul_rn(s11, dy), dx));
      // v / divisor; a power-of-two divisor (sqrt(256) = 16) scales exactly by its reciprocal
      const float res = g.div_recip != 0.f ? v * g.div_recip : v / g.divisor;
      if ((XP & 2) == 0 || res == 12345.0f) o[(long long)(oy + RD * ox) * g.N] = res;
    }
  }
}

// ---------------------------------------------------------------------------
// Query order of the on-the-fly lookup (round 3).  The union box of a 4 x 8
// query tile is compact for smooth flow fields but ~10x its windows' cells at
// level 0 for flows that vary pixel to pixel (the bench's i.i.d. N(0, 4^2)
// model): neighbouring queries' windows are unrelated.  Grouping the queries by
// window position instead keeps every box near one window whatever the flow.
// Three launches over OB blocks of whole tiles per (coordinate set, level):
//   K1 alt_bin_count_kernel   thread = query (tile-major): bin by window origin
//      (bins of ~32 queries: 2^by x 2^bx origin cells, snake order over bin
//      rows; non-finite coordinates in a last bin), bin ids to the workspace,
//      the block's histogram (LDS) to cnt[block][bin], and the block's tiles'
//      union box areas (the cells the tile order would multiply) to cost[block];
//   K2 alt_bin_scan_kernel    thread = bin: its exclusive prefix over the
//      blocks (in place) and its total;
//   K3 alt_bin_scatter_kernel chooses the bin order when the tiles' boxes
//      average more than 1.5x a bin group's estimated box ((2^by + 2r + 1) x
//      (2^bx + 2r + 1)), else the tile order (then the lookup multiplies exactly
//      the spatial form's boxes); in bin order each block scans the bins' totals
//      itself and writes its queries' entries {query, x, y, 0} at bin base +
//      block prefix + an LDS rank, in tile order at their tile slots.
// Queries of a bin land in any order: the box GEMM's per-(cell, query) sums do
// not depend on which queries share a workgroup, so the lookup's outputs are
// bit-identical to the tile order's.  (A one-workgroup-per-list form ran the
// whole job on 4 CUs: 76 us per 1080p lookup.)
// ---------------------------------------------------------------------------
using dxr::BIN_MAX;   // lookup_plan.h, with the workspace's size
using dxr::OB;        // blocks per list

struct BinGeom {
  int bsx[8], bsy[8], nbx[8], nby[8];
};

BinGeom make_bins(int N, const AltGeom& g, int levels) {
  BinGeom b{};
  for (int l = 0; l < levels; ++l) {
    const int h2 = g.lv[l].H2, w2 = g.lv[l].W2;
    const double dens = (double)N / ((double)h2 * w2);
    int lg = 0;
    while ((1 << lg) * dens < 32.0 && lg < 12) ++lg;   // bin area 2^lg ~ 32 queries
    int by = lg / 2, bx = lg - by;
    while (((w2 + (1 << bx) - 1) >> bx) * ((h2 + (1 << by) - 1) >> by) > BIN_MAX) {
      if (bx <= by) ++bx; else ++by;
    }
    b.bsx[l] = bx;
    b.bsy[l] = by;
    b.nbx[l] = (w2 + (1 << bx) - 1) >> bx;
    b.nby[l] = (h2 + (1 << by) - 1) >> by;
  }
  return b;
}

// Workspace of one list (coordinate set, level): dxr::OrderWs (lookup_plan.h).
using dxr::OrderWs;
using dxr::order_ws;

struct OrderArgs {
  unsigned char* ws;   // lists [Z][L] of OrderWs.bytes each
  long long list_bytes, np;
  int W1, tiles_x, ntiles, tpb;   // tiles per block
};

// slot i of a block -> (tile, slot within the 4 x 8 tile) -> query (or -1)
__device__ __forceinline__ int order_query(int blk, int i, const OrderArgs& o, int H1, int& tile,
                                           int& slot) {
  tile = blk * o.tpb + i / TQ;
  slot = i % TQ;
  const int qy = (tile / o.tiles_x) * TQY + slot / TQX, qx = (tile % o.tiles_x) * TQX + slot % TQX;
  return (tile < o.ntiles && qy < H1 && qx < o.W1) ? qy * o.W1 + qx : -1;
}

template <int R>
__global__ __launch_bounds__(256) void alt_bin_count_kernel(const float* __restrict__ coords,
                                                            AltGeom g, BinGeom bg, OrderArgs o) {
  constexpr int RD1 = 2 * R + 2;
  __shared__ int hist[BIN_MAX + 1];
  __shared__ float wcost[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blk = blockIdx.x, l = blockIdx.y, z = blockIdx.z;
  const AltLevel lv = g.lv[l];
  const int nbx = bg.nbx[l], nb = nbx * bg.nby[l], bsx = bg.bsx[l], bsy = bg.bsy[l];
  const float* cz = coords + (long long)z * g.coord_zstride;
  const int H1 = g.N / o.W1;
  unsigned char* lw = o.ws + ((long long)z * gridDim.y + l) * o.list_bytes;
  const OrderWs w = order_ws(o.np);
  int* ids = reinterpret_cast<int*>(lw + w.ids);
  for (int i = tid; i <= nb; i += 256) hist[i] = 0;
  __syncthreads();
  float cost = 0.f;
  // 32 consecutive lanes = one tile: its union box by a 32-lane reduction
  for (int i = tid; i < o.tpb * TQ; i += 256) {
    int tile, slot;
    const int q = order_query(blk, i, o, H1, tile, slot);
    const int qc = max(q, 0);
    const float x = cz[(long long)qc * g.coord_qstride] * lv.inv;
    const float y = cz[(long long)qc * g.coord_qstride + g.coord_cstride] * lv.inv;
    const float xf = floorf(x), yf = floorf(y);
    int bin = nb;
    int lx0 = 0x7fffffff, ly0 = 0x7fffffff, lx1 = -1, ly1 = -1;
    if (q >= 0 && fabsf(xf) < 1.0e8f && fabsf(yf) < 1.0e8f) {
      const int cx = min(max((int)xf, 0), lv.W2 - 1), cy = min(max((int)yf, 0), lv.H2 - 1);
      const int byi = cy >> bsy;
      int bxi = cx >> bsx;
      if (byi & 1) bxi = nbx - 1 - bxi;
      bin = byi * nbx + bxi;
      const int x0 = (int)xf - R, y0 = (int)yf - R;
      if (x0 + RD1 > 0 && x0 < lv.W2 && y0 + RD1 > 0 && y0 < lv.H2) {   // live window
        lx0 = max(x0, 0);
        ly0 = max(y0, 0);
        lx1 = min(x0 + RD1, lv.W2);
        ly1 = min(y0 + RD1, lv.H2);
      }
    }
    if (q >= 0) {
      atomicAdd(&hist[bin], 1);
      ids[(long long)blk * o.tpb * TQ + i] = bin;
    }
#pragma unroll
    for (int d = 1; d < TQ; d <<= 1) {
      lx0 = min(lx0, __shfl_xor(lx0, d));
      ly0 = min(ly0, __shfl_xor(ly0, d));
      lx1 = max(lx1, __shfl_xor(lx1, d));
      ly1 = max(ly1, __shfl_xor(ly1, d));
    }
    if ((lane & 31) == 0 && lx1 > lx0) cost += (float)(lx1 - lx0) * (float)(ly1 - ly0);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) cost += __shfl_xor(cost, d);
  if (lane == 0) wcost[wave] = cost;
  __syncthreads();
  int* cnt = reinterpret_cast<int*>(lw + w.cnt) + (long long)blk * (BIN_MAX + 1);
  for (int i = tid; i <= nb; i += 256) cnt[i] = hist[i];
  if (tid == 0)
    reinterpret_cast<float*>(lw + w.cost)[blk] = wcost[0] + wcost[1] + wcost[2] + wcost[3];
}

// K2: thread = bin: exclusive prefix of its count over the OB blocks, in place
// (64 loads in flight), and the bin's total.  Grid (ceil(bins / 256), L, Z).
__global__ __launch_bounds__(256) void alt_bin_scan_kernel(BinGeom bg, OrderArgs o) {
  const int l = blockIdx.y, z = blockIdx.z;
  const int bin = blockIdx.x * 256 + threadIdx.x;
  const int nb = bg.nbx[l] * bg.nby[l];
  if (bin > nb) return;
  unsigned char* lw = o.ws + ((long long)z * gridDim.y + l) * o.list_bytes;
  const OrderWs w = order_ws(o.np);
  int* cnt = reinterpret_cast<int*>(lw + w.cnt) + bin;
  int c[OB];
#pragma unroll
  for (int b = 0; b < OB; ++b) c[b] = cnt[(long long)b * (BIN_MAX + 1)];
  int run = 0;
#pragma unroll
  for (int b = 0; b < OB; ++b) {
    const int t = c[b];
    cnt[(long long)b * (BIN_MAX + 1)] = run;
    run += t;
  }
  reinterpret_cast<int*>(lw + w.tot)[bin] = run;
}

// K3: every block scans the bins' totals itself (<= 4097 values from L2) into
// LDS bases, decides the order from the blocks' box costs (the same decision in
// every block), then writes its queries' entries: at base[bin] + its block
// prefix + an LDS rank (bin order), or at their tile slots (tile order).
template <int R>
__global__ __launch_bounds__(256) void alt_bin_scatter_kernel(const float* __restrict__ coords,
                                                              AltGeom g, BinGeom bg, OrderArgs o) {
  constexpr int RD1 = 2 * R + 2;
  __shared__ int off[BIN_MAX + 1];
  __shared__ int wsum[4];
  __shared__ int binned_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blk = blockIdx.x, l = blockIdx.y, z = blockIdx.z;
  const int nb = bg.nbx[l] * bg.nby[l];
  const float* cz = coords + (long long)z * g.coord_zstride;
  const int H1 = g.N / o.W1;
  unsigned char* lw = o.ws + ((long long)z * gridDim.y + l) * o.list_bytes;
  const OrderWs w = order_ws(o.np);
  int4* ents = reinterpret_cast<int4*>(lw + w.ents);
  const int* ids = reinterpret_cast<const int*>(lw + w.ids);
  if (tid == 0) {
    float c = 0.f;
    const float* cost = reinterpret_cast<const float*>(lw + w.cost);
    for (int b = 0; b < OB; ++b) c += cost[b];
    const float chunk = (float)((1 << bg.bsy[l]) + RD1 - 1) * (float)((1 << bg.bsx[l]) + RD1 - 1);
    binned_s = c > 1.5f * chunk * (float)o.ntiles ? 1 : 0;
  }
  __syncthreads();
  const bool binned = binned_s != 0;
  if (binned) {
    // exclusive scan of the totals: thread t owns bins [t * per, t * per + per)
    const int* tot = reinterpret_cast<const int*>(lw + w.tot);
    const int per = (nb + 1 + 255) / 256;    // <= 17
    int loc = 0;
    for (int k = 0; k < per; ++k) {
      const int b = tid * per + k;
      if (b <= nb) loc += tot[b];
    }
    int v = loc;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(v, d);
      if (lane >= d) v += t;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    int base = v - loc;
    for (int i = 0; i < wave; ++i) base += wsum[i];
    const int* cnt = reinterpret_cast<const int*>(lw + w.cnt) + (long long)blk * (BIN_MAX + 1);
    for (int k = 0; k < per; ++k) {
      const int b = tid * per + k;
      if (b <= nb) {
        off[b] = base + cnt[b];
        base += tot[b];
      }
    }
    __syncthreads();
  }
  for (int i = tid; i < o.tpb * TQ; i += 256) {
    int tile, slot;
    const int q = order_query(blk, i, o, H1, tile, slot);
    if (tile >= o.ntiles) break;
    int4 e = make_int4(-1, 0, 0, 0);
    if (q >= 0)
      e = make_int4(q, __float_as_int(cz[(long long)q * g.coord_qstride]),
                    __float_as_int(cz[(long long)q * g.coord_qstride + g.coord_cstride]), 0);
    if (!binned)
      ents[(long long)tile * TQ + slot] = e;
    else if (q >= 0)
      ents[atomicAdd(&off[ids[(long long)blk * o.tpb * TQ + i]], 1)] = e;
  }
  if (binned && blk == 0)   // entries past the queries: padding
    for (long long i = g.N + tid; i < o.np; i += 256) ents[i] = make_int4(-1, 0, 0, 0);
}

// PF: cell loads of the ordered form kept 4 k steps ahead (round 3: with compact boxes the
// waves wait on L2 latency, 62 % of wave cycles at PF = 1; 1080p 12 lookups 2,033 -> 1,972 us,
// Sintel 626 -> 612 us in the step).  The tile-order form stays at 1 (its boxes are L1/TA-bound).
// Occupancy bound of the f16-pair form: 3 workgroups per CU (the 1080p r02
// A/B); from r = 6 the window buffers and index registers do not fit that bound
// (hipcc: "desired occupancy 3, final 2"), so those radii ask for 2.
constexpr int alt_minw(int r) { return r >= 6 ? 2 : 3; }
// The float16-operand form (IN16): one query plane, 16 KB of LDS less per
// workgroup, so one workgroup more per CU fits (hipcc, ordered form: r <= 5 128
// VGPRs, 18-36 KB LDS, occupancy 4; r = 6 138 VGPRs, 42.5 KB, occupancy 3; no
// scratch, no spills.  Asking for 5 spills 24-25 VGPRs.  DESIGN.md §3.17).
constexpr int alt_minw16(int r) { return r >= 6 ? 3 : 4; }
// The bfloat16-operand form (INBF) asks for the same bound (DESIGN.md §3.18 has
// hipcc's figures per radius).
constexpr int alt_minwbf(int r) { return r >= 6 ? 3 : 4; }

// OUTX / okind: the flagged output forms (alt_corr_mfma_kernel), tile order and ordered.
// IN16: float16 fmap1 and the float16 levels of g.f16_levels (alt_corr_in16.hip).
// INBF (with IN16): they are bfloat16 (alt_corr_inbf16.hip).
template <int R, int DMA = 0, int PF = 4, int XP = 0, bool OUTX = false, bool IN16 = false,
          bool INBF = false>
int launch_alt_mfma_r(const float* f1, const float* coords, float* out, const AltGeom& g,
                      int levels, int Z, int W1, hipStream_t stream, void* ws = nullptr,
                      int xl = -1, int okind = 0) {
  const int H1 = g.N / W1;
  const int tiles_x = (W1 + TQX - 1) / TQX, tiles_y = (H1 + TQY - 1) / TQY;
  const int ntiles = tiles_x * tiles_y;
  // XCDs shared out by level (alt_corr_mfma_kernel XL) where the split is exact:
  // experiments only — round 4, 1080p i.i.d. flows, 12 ordered lookups in the
  // step: 2,567 us with it against 1,990 us without (the levels' lists cost
  // different amounts, so the XCDs of the cheap levels idle)
  const int xl_ok = (8 % levels == 0 && ((long long)levels * ntiles) % 8 == 0) ? 1 : 0;
  const int XL = xl < 0 ? 0 : (xl & xl_ok);
  const dim3 grid((unsigned)ntiles, (unsigned)levels, (unsigned)Z);
  // f16 pair split (r02, 1080p: 227 vs 275 us for the 3-way bf16 split), 3 workgroups/CU
  if (ws != nullptr) {
    OrderArgs o;
    o.ws = static_cast<unsigned char*>(ws);
    o.np = (long long)ntiles * TQ;
    o.list_bytes = order_ws(o.np).bytes;
    o.W1 = W1;
    o.tiles_x = tiles_x;
    o.ntiles = ntiles;
    o.tpb = (ntiles + OB - 1) / OB;
    const BinGeom bg = make_bins(g.N, g, levels);
    const dim3 bgrid(OB, (unsigned)levels, (unsigned)Z);
    hipLaunchKernelGGL((alt_bin_count_kernel<R>), bgrid, dim3(256), 0, stream, coords, g, bg, o);
    int st = dxr::launch_status();
    if (st != DXR_OK) return st;
    int nbmax = 0;
    for (int l = 0; l < levels; ++l) nbmax = std::max(nbmax, bg.nbx[l] * bg.nby[l]);
    hipLaunchKernelGGL(alt_bin_scan_kernel, dim3((unsigned)((nbmax + 1 + 255) / 256),
                       (unsigned)levels, (unsigned)Z), dim3(256), 0, stream, bg, o);
    st = dxr::launch_status();
    if (st != DXR_OK) return st;
    hipLaunchKernelGGL((alt_bin_scatter_kernel<R>), bgrid, dim3(256), 0, stream, coords, g, bg, o);
    st = dxr::launch_status();
    if (st != DXR_OK) return st;
    // entries of list (z, l) start at list (z * levels + l) * list_bytes: the kernel
    // indexes int4 entries by ((z * levels + l) * np + i), so lists are laid out
    // with a stride of list_bytes / 16 entries
    if constexpr (DMA != 0)
      hipLaunchKernelGGL((alt_corr_mfma_kernel<R, 2, true, 1, DMA>), grid,
                         dim3(256), 0, stream, f1, coords, out, g, W1, tiles_x,
                         reinterpret_cast<const int4*>(ws), o.list_bytes / 16, XL, 0);
    else if constexpr (INBF)
      hipLaunchKernelGGL((alt_corr_mfma_kernel<R, alt_minwbf(R), true, PF, 0, 0, false, OUTX, true, true>),
                         grid, dim3(256), 0, stream, f1, coords, out, g, W1, tiles_x,
                         reinterpret_cast<const int4*>(ws), o.list_bytes / 16, XL, okind);
    else if constexpr (IN16)
      hipLaunchKernelGGL((alt_corr_mfma_kernel<R, alt_minw16(R), true, PF, 0, 0, false, OUTX, true>),
                         grid, dim3(256), 0, stream, f1, coords, out, g, W1, tiles_x,
                         reinterpret_cast<const int4*>(ws), o.list_bytes / 16, XL, okind);
    else
      hipLaunchKernelGGL((alt_corr_mfma_kernel<R, alt_minw(R), true, PF, 0, XP, false, OUTX>),
                         grid, dim3(256), 0, stream, f1, coords, out, g, W1, tiles_x,
                         reinterpret_cast<const int4*>(ws), o.list_bytes / 16, XL, okind);
    return dxr::launch_status();
  }
  if constexpr (INBF)
    hipLaunchKernelGGL((alt_corr_mfma_kernel<R, alt_minwbf(R), false, 1, 0, 0, false, OUTX, true, true>), grid,
                       dim3(256), 0, stream, f1, coords, out, g, W1, tiles_x, nullptr, 0, 0, okind);
  else if constexpr (IN16)
    hipLaunchKernelGGL((alt_corr_mfma_kernel<R, alt_minw16(R), false, 1, 0, 0, false, OUTX, true>), grid,
                       dim3(256), 0, stream, f1, coords, out, g, W1, tiles_x, nullptr, 0, 0, okind);
  else
    hipLaunchKernelGGL((alt_corr_mfma_kernel<R, alt_minw(R), false, 1, 0, 0, false, OUTX>), grid,
                       dim3(256), 0, stream, f1, coords, out, g, W1, tiles_x, nullptr, 0, 0, okind);
  return dxr::launch_status();
}

template <int R>
int launch_alt_r(const float* f1, const float* coords, float* out, const AltGeom& g, int levels,
                 int Z, bool vec, hipStream_t stream) {
  const dim3 grid((unsigned)((g.N + 63) / 64), (unsigned)levels, (unsigned)Z);
  if (vec)
    hipLaunchKernelGGL((alt_corr_kernel<R, true>), grid, dim3(256), 0, stream, f1, coords, out, g);
  else
    hipLaunchKernelGGL((alt_corr_kernel<R, false>), grid, dim3(256), 0, stream, f1, coords, out, g);
  return dxr::launch_status();
}

// The form the plan names (dxr::plan_alt_form: MFMA ordered on the workspace, MFMA
// in tile order, or the per-query VALU form, float4 or scalar loads).
// OUTX / okind: a flagged request (alt_corr_out.hip); IN16: float16 operands
// (alt_corr_in16.hip); INBF (with IN16): bfloat16 operands (alt_corr_inbf16.hip).
// The plan sends those to the MFMA forms only.
template <bool OUTX = false, bool IN16 = false, bool INBF = false>
int launch_alt(const float* f1, const float* coords, float* out, const AltGeom& g,
               const dxr::AltLookupPlan& p, int Z, hipStream_t stream, int W1, void* ws, int okind) {
  if (dxr::alt_form_is_mfma(p.form))
    return dxr::dispatch_radius<6>(p.radius, [&](auto r) {
      return launch_alt_mfma_r<decltype(r)::value, 0, 4, 0, OUTX, IN16, INBF>(
          f1, coords, out, g, p.levels, Z, W1, stream, p.use_workspace ? ws : nullptr, -1, okind);
    });
  // (the flagged units instantiate the VALU forms too, as they always have)
  return dxr::dispatch_radius<6>(p.radius, [&](auto r) {
    return launch_alt_r<decltype(r)::value>(f1, coords, out, g, p.levels, Z, p.form == dxr::ALT_VALU_VEC,
                                            stream);
  });
}

// A planned on-the-fly lookup (a.plan: lookup_plan.h): the geometry and the launch.
// plan->levels < num_levels: only those levels of a num_levels-level output (the
// rest come from dxr_alt_volume_lookup).
// OUTX / okind: a flagged request (launch_alt); `out` then holds what okind says.
// IN16: DXR_ALT_IN_F16 — fmap1 and fmap2_levels[0] point at float16.
// INBF (with IN16): DXR_ALT_IN_BF16 — they point at bfloat16.
template <bool OUTX = false, bool IN16 = false, bool INBF = false>
int alt_lookup(const dxr::AltLookupArgs& a, int okind) {
  const dxr::AltLookupPlan& p = *a.plan;
  const int rd = 2 * p.radius + 1;
  AltGeom g;
  g.N = (int)(a.H * a.W);
  g.C = (int)a.C;
  g.Nc = 1;
  g.cout = a.num_levels * rd * rd;
  g.divisor = a.divisor;
  g.div_recip = p.div_recip;
  g.f1_bstride = a.H * a.W * a.C;
  g.coord_zstride = 2 * a.H * a.W;
  g.coord_cstride = a.H * a.W;
  g.coord_qstride = 1;
  for (int l = 0; l < p.levels; ++l)
    g.lv[l] = AltLevel{a.fmap2_levels[l], p.L.h[l], p.L.w[l], 1.f / (float)(1 << l), l * rd * rd};
  if constexpr (IN16) g.f16_levels = 1u;
  return launch_alt<OUTX, IN16, INBF>(a.fmap1, a.coords, static_cast<float*>(a.out), g, p, (int)a.B,
                                      a.stream, (int)a.W, a.workspace, okind);
}

// A unit's whole shim: alt_lookup on its operand type for the request's output
// form, FORMS being the forms the unit answers (out_store.h); OUTX and okind
// follow from the form.
template <unsigned FORMS, bool IN16 = false, bool INBF = false>
int alt_lookup_forms(const dxr::AltLookupArgs& a) {
  return dxr::dispatch_out_form<FORMS>(a.plan->out_flag, a.plan->nhwc, a.out, [&](auto* out, auto nhwc) {
    constexpr int okind = dxr::out_kind<std::remove_pointer_t<decltype(out)>, decltype(nhwc)::value>();
    return alt_lookup<okind != 0, IN16, INBF>(a, okind);
  });
}

}  // namespace

// Everything above is the lookup's templates.  The variant units (alt_corr_out.hip,
// alt_corr_in16.hip, alt_corr_inbf16.hip) define DXR_TEMPLATES_ONLY and include this
// file for them; what follows (the reference-FFI backward, the layout helpers, the
// volume GEMM and every entry point) is this unit's alone.
#ifndef DXR_TEMPLATES_ONLY

namespace {

bool aligned16(const void* p) { return dxr::aligned16((uintptr_t)p); }

// ---------------------------------------------------------------------------
// alt_cuda_corr.backward, reference-FFI form (correlation_kernel.cu:122-256,
// launched by :288-320).  For query q of pair b and coordinate set n, cell
// (iy, ix) in [0, 2r+1]^2 — (h2, w2) = (floor(y) - r + iy, floor(x) - r + ix) —
// receives the transpose of the forward's bilinear scatter (:197-216):
//   g = [iy>0, ix>0]  G(iy-1, ix-1) dy dx   + [iy>0, ix<rd]  G(iy-1, ix) dy (1-dx)
//     + [iy<rd, ix>0] G(iy, ix-1) (1-dy) dx + [iy<rd, ix<rd] G(iy, ix) (1-dy)(1-dx)
// with G(oy, ox) = corr_grad[b][n][oy + rd*ox][q]; every in-bounds cell then adds
// g * fmap2[cell] to fmap1_grad[q] and g * fmap1[q] to fmap2_grad[cell]
// (:218-233; atomics there too).  coords_grad is zero (:307).
//
// MI355X mapping: one wave per query pixel.  Lane L owns channels c0 + L + 64j
// (j < 4) of a 256-channel slab, so each fmap2[cell] read is four 256-byte
// coalesced dword loads and each fmap2_grad update four 256-byte hardware
// global_atomic_add_f32 (full rate on contiguous lines).  The (2r+1)^2 weights of
// the query are loaded once across the lanes and broadcast per cell with
// v_readlane (the cell loops are unrolled, so the lane index is a constant).
// fmap1_grad[q] is owned by the wave: written once per slab, no atomics.
template <int R>
__global__ __launch_bounds__(256) void alt_corr_backward_kernel(
    const float* __restrict__ f1, const float* __restrict__ f2, const float* __restrict__ coords,
    const float* __restrict__ cgrad, float* __restrict__ f1g, float* __restrict__ f2g, int N,
    int H2, int W2, int C, int Nc) {
  constexpr int RD = 2 * R + 1, RR = RD * RD, NG = (RR + 63) / 64;
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  const int b = blockIdx.y;
  if (q >= N) return;  // whole wave; the kernel has no block barrier
  const float* f1q = f1 + ((long long)b * N + q) * C;
  float* f1gq = f1g + ((long long)b * N + q) * C;
  const float* f2b = f2 + (long long)b * H2 * W2 * C;
  float* f2gb = f2g + (long long)b * H2 * W2 * C;
  for (int c0 = 0; c0 < C; c0 += 256) {
    float a[4], acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + lane + 64 * j;
      a[j] = c < C ? f1q[c] : 0.f;
      acc[j] = 0.f;
    }
    for (int n = 0; n < Nc; ++n) {
      const long long z = (long long)b * Nc + n;
      const float x = coords[(z * N + q) * 2], y = coords[(z * N + q) * 2 + 1];
      const float fx = floorf(x), fy = floorf(y);
      const float dx = x - fx, dy = y - fy;
      const int x0 = (int)fx - R, y0 = (int)fy - R;
      int gv[NG];
#pragma unroll
      for (int k = 0; k < NG; ++k) {
        const int i = lane + 64 * k;
        gv[k] = i < RR ? __float_as_int(cgrad[(z * RR + i) * N + q]) : 0;
      }
      auto G = [&](int oy, int ox) {
        const int i = oy + RD * ox;
        return __int_as_float(__builtin_amdgcn_readlane(gv[i / 64], i % 64));
      };
#pragma unroll
      for (int iy = 0; iy <= RD; ++iy) {
        const int h2 = y0 + iy;
        if (h2 < 0 || h2 >= H2) continue;
#pragma unroll
        for (int ix = 0; ix <= RD; ++ix) {
          const int w2 = x0 + ix;
          if (w2 < 0 || w2 >= W2) continue;
          float g = 0.f;
          if (iy > 0 && ix > 0) g += G(iy - 1, ix - 1) * dy * dx;
          if (iy > 0 && ix < RD) g += G(iy - 1, ix) * dy * (1.f - dx);
          if (iy < RD && ix > 0) g += G(iy, ix - 1) * (1.f - dy) * dx;
          if (iy < RD && ix < RD) g += G(iy, ix) * (1.f - dy) * (1.f - dx);
          const long long cell = ((long long)h2 * W2 + w2) * C;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c = c0 + lane + 64 * j;
            if (c < C) {
              acc[j] += g * f2b[cell + c];
              unsafeAtomicAdd(f2gb + cell + c, g * a[j]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + lane + 64 * j;
      if (c < C) f1gq[c] = acc[j];
    }
  }
}

struct AltBwd {
  const float *f1, *f2, *coords, *cgrad;
  float *f1g, *f2g;
  int B, N, H2, W2, C, Nc;
};

template <int R>
int launch_alt_backward_r(const AltBwd& a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.N + 3) / 4), (unsigned)a.B);
  hipLaunchKernelGGL((alt_corr_backward_kernel<R>), grid, dim3(256), 0, stream, a.f1, a.f2,
                     a.coords, a.cgrad, a.f1g, a.f2g, a.N, a.H2, a.W2, a.C, a.Nc);
  return dxr::launch_status();
}

// ---------------------------------------------------------------------------
// Layout kernels for channels-last (NHWC) fmaps.
//
// Batched transpose [B, rows, cols] -> [B, cols, rows] (NCHW -> NHWC is rows = C,
// cols = H*W; NHWC -> NCHW the reverse).  One workgroup moves a 64x64 tile
// through LDS (row pitch 65 elements: the column reads are conflict-free); a
// wave reads one 64-element row segment and writes one 64-element column
// segment, so both HBM streams are contiguous.  Pure data movement: bit-exact.
template <typename T>
__global__ __launch_bounds__(256) void transpose_tile_kernel(const T* __restrict__ in,
                                                             T* __restrict__ out, int rows,
                                                             int cols) {
  __shared__ T tile[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
  const long long base = (long long)blockIdx.z * rows * cols;
  const T* src = in + base;
  T* dst = out + base;
  const int c = c0 + tx;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = r0 + ty + 4 * i;
    if (r < rows && c < cols) tile[ty + 4 * i][tx] = src[(long long)r * cols + c];
  }
  __syncthreads();
  const int r = r0 + tx;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int cc = c0 + ty + 4 * i;
    if (cc < cols && r < rows) dst[(long long)cc * rows + r] = tile[tx][ty + 4 * i];
  }
}

// float32 form for rows % 4 == 0 and cols % 4 == 0 (fmaps: C and H*W): 16-byte
// loads along cols and 16-byte stores along rows, 16 lanes per 256-byte row
// segment.  The scalar kernel moved 1080p fmaps at 3.8 TB/s.
__global__ __launch_bounds__(256) void transpose_tile_v4_kernel(const float* __restrict__ in,
                                                                float* __restrict__ out, int rows,
                                                                int cols) {
  __shared__ float tile[64][65];
  const int tq = threadIdx.x & 15, tr = threadIdx.x >> 4;   // float4 slot, row in pass
  const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
  const long long base = (long long)blockIdx.z * rows * cols;
  const float* src = in + base;
  float* dst = out + base;
  const int c = c0 + 4 * tq;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lr = tr + 16 * i, r = r0 + lr;
    if (r < rows && c < cols) {
      const float4 v = *reinterpret_cast<const float4*>(src + (long long)r * cols + c);
      tile[lr][4 * tq] = v.x;
      tile[lr][4 * tq + 1] = v.y;
      tile[lr][4 * tq + 2] = v.z;
      tile[lr][4 * tq + 3] = v.w;
    }
  }
  __syncthreads();
  const int r = r0 + 4 * tq;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lc = tr + 16 * i, cc = c0 + lc;
    if (cc < cols && r < rows) {
      const float4 v = make_float4(tile[4 * tq][lc], tile[4 * tq + 1][lc], tile[4 * tq + 2][lc],
                                   tile[4 * tq + 3][lc]);
      *reinterpret_cast<float4*>(dst + (long long)cc * rows + r) = v;
    }
  }
}

// 2x2 / stride-2 floor-mode average pool of [B, H, W, C] into [B, H/2, W/2, C]:
// F.avg_pool2d on a channels-last tensor (core/corr.py:70-71), the same four
// values summed in the same order as avg_pool2x2_kernel (corr_build.hip), so
// the result is bit-identical to pooling the NCHW tensor.  Four channels per
// thread (float4) when C % 4 == 0.
template <int V>
__global__ __launch_bounds__(256) void avg_pool2x2_nhwc_kernel(const float* __restrict__ in,
                                                               float* __restrict__ out,
                                                               int B, int H, int W, int C) {
  const int Ho = H / 2, Wo = W / 2, Cv = C / V;
  const long long total = (long long)B * Ho * Wo * Cv;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int cv = (int)(idx % Cv);
    long long r = idx / Cv;
    const int x = (int)(r % Wo);
    r /= Wo;
    const int y = (int)(r % Ho);
    const long long b = r / Ho;
    const long long row = (b * H + 2 * y) * W + 2 * x;
    if constexpr (V == 4) {
      const float4* s = reinterpret_cast<const float4*>(in);
      const long long cs = C / 4;
      const float4 a = s[row * cs + cv], bb = s[(row + 1) * cs + cv];
      const float4 cc = s[(row + W) * cs + cv], d = s[(row + W + 1) * cs + cv];
      float4 o;
      o.x = (((a.x + bb.x) + cc.x) + d.x) * 0.25f;
      o.y = (((a.y + bb.y) + cc.y) + d.y) * 0.25f;
      o.z = (((a.z + bb.z) + cc.z) + d.z) * 0.25f;
      o.w = (((a.w + bb.w) + cc.w) + d.w) * 0.25f;
      reinterpret_cast<float4*>(out)[idx] = o;
    } else {
      const float* s = in + row * C + cv;
      out[idx] = (((s[0] + s[C]) + s[(long long)W * C]) + s[(long long)(W + 1) * C]) * 0.25f;
    }
  }
}

}  // namespace

extern "C" int dxr_alt_corr_forward(const float* fmap1, const float* fmap2, const float* coords,
                                    float* corr, int64_t B, int64_t H1, int64_t W1, int64_t H2,
                                    int64_t W2, int64_t C, int64_t Nc, int radius,
                                    hipStream_t stream) {
  if (B < 0 || H1 < 1 || W1 < 1 || H2 < 1 || W2 < 1 || C < 1 || Nc < 0 || radius < 0)
    return DXR_EINVAL;
  if (radius > 6) return DXR_EUNSUPPORTED;
  if (H1 * W1 > (1LL << 30) || H2 * W2 > (1LL << 30) || B * Nc > 65535 || C > (1 << 20))
    return DXR_EINVAL;
  if (B == 0 || Nc == 0) return DXR_OK;
  if (!fmap1 || !fmap2 || !coords || !corr) return DXR_EINVAL;
  const int rd = 2 * radius + 1;
  AltGeom g;
  g.N = (int)(H1 * W1);
  g.C = (int)C;
  g.Nc = (int)Nc;
  g.cout = rd * rd;
  g.divisor = 1.f;
  g.div_recip = 1.f;
  g.f1_bstride = H1 * W1 * C;
  g.coord_zstride = H1 * W1 * 2;
  g.coord_cstride = 1;
  g.coord_qstride = 2;
  g.lv[0] = AltLevel{fmap2, (int)H2, (int)W2, 1.f, 0};
  const bool vec = (C % 4 == 0) && aligned16(fmap1) && aligned16(fmap2);
  dxr::AltLookupPlan p{};   // one level, no flags, no workspace: the lookups' form rule
  p.radius = radius;
  p.levels = 1;
  p.form = dxr::alt_form(vec, C, false);
  return launch_alt(fmap1, coords, corr, g, p, (int)(B * Nc), stream, (int)W1, nullptr, 0);
}

extern "C" int dxr_alt_corr_backward(const float* fmap1, const float* fmap2, const float* coords,
                                     const float* corr_grad, float* fmap1_grad,
                                     float* fmap2_grad, int64_t B, int64_t H1, int64_t W1,
                                     int64_t H2, int64_t W2, int64_t C, int64_t Nc, int radius,
                                     hipStream_t stream) {
  if (B < 0 || H1 < 1 || W1 < 1 || H2 < 1 || W2 < 1 || C < 1 || Nc < 0 || radius < 0)
    return DXR_EINVAL;
  // the accumulating MFMA form (alt_corr_bwd.hip); every other radius as it always was
  if (radius & DXR_ALT_BWD_ACCUMULATE)
    return dxr::alt_backward_accumulate(fmap1, fmap2, coords, corr_grad, fmap1_grad, fmap2_grad,
                                        B, H1, W1, H2, W2, C, Nc, radius, stream);
  if (radius > 6) return DXR_EUNSUPPORTED;
  if (H1 * W1 > (1LL << 30) || H2 * W2 > (1LL << 30) || B > 65535 || C > (1 << 20))
    return DXR_EINVAL;
  if (B == 0) return DXR_OK;
  if (!fmap1 || !fmap2 || !fmap1_grad || !fmap2_grad) return DXR_EINVAL;
  if (Nc > 0 && (!coords || !corr_grad)) return DXR_EINVAL;
  // fmap2_grad accumulates atomically from zero, as the reference's torch::zeros output.
  hipError_t e = hipMemsetAsync(fmap2_grad, 0, (size_t)(B * H2 * W2 * C) * sizeof(float), stream);
  if (e != hipSuccess) {
    dxr::set_last_hip_error(e);
    return DXR_EHIP;
  }
  const AltBwd a{fmap1, fmap2, coords, corr_grad, fmap1_grad, fmap2_grad, (int)B,
                 (int)(H1 * W1), (int)H2, (int)W2, (int)C, (int)Nc};
  return dxr::dispatch_radius<6>(radius, [&](auto r) {
    return launch_alt_backward_r<decltype(r)::value>(a, stream);
  });
}

extern "C" int dxr_transpose(const void* in, void* out, int dtype, int64_t B, int64_t rows,
                             int64_t cols, hipStream_t stream) {
  if (B < 0 || rows < 0 || cols < 0 || (dtype != DXR_F32 && dtype != DXR_BF16)) return DXR_EINVAL;
  if (rows * cols > (1LL << 40) || B > 65535 || (rows + 63) / 64 > 65535 ||
      (cols + 63) / 64 > (1LL << 31) - 1)
    return DXR_EINVAL;
  if (B == 0 || rows == 0 || cols == 0) return DXR_OK;
  if (!in || !out || rows > INT32_MAX || cols > INT32_MAX) return DXR_EINVAL;
  const dim3 grid((unsigned)((cols + 63) / 64), (unsigned)((rows + 63) / 64), (unsigned)B);
  if (dtype == DXR_F32 && rows % 4 == 0 && cols % 4 == 0 && aligned16(in) && aligned16(out))
    hipLaunchKernelGGL(transpose_tile_v4_kernel, grid, dim3(256), 0, stream,
                       static_cast<const float*>(in), static_cast<float*>(out), (int)rows,
                       (int)cols);
  else if (dtype == DXR_F32)
    hipLaunchKernelGGL((transpose_tile_kernel<float>), grid, dim3(256), 0, stream,
                       static_cast<const float*>(in), static_cast<float*>(out), (int)rows,
                       (int)cols);
  else
    hipLaunchKernelGGL((transpose_tile_kernel<uint16_t>), grid, dim3(256), 0, stream,
                       static_cast<const uint16_t*>(in), static_cast<uint16_t*>(out), (int)rows,
                       (int)cols);
  return dxr::launch_status();
}

extern "C" int dxr_avg_pool2x2_nhwc(const float* in, float* out, int64_t B, int64_t H, int64_t W,
                                    int64_t C, hipStream_t stream) {
  if (B < 0 || H < 0 || W < 0 || C < 1 || B > INT32_MAX || H > INT32_MAX || W > INT32_MAX ||
      C > INT32_MAX)
    return DXR_EINVAL;
  const long long total = B * (H / 2) * (W / 2) * C;
  if (total == 0) return DXR_OK;
  if (!in || !out) return DXR_EINVAL;
  const bool vec = (C % 4 == 0) && aligned16(in) && aligned16(out);
  long long blocks = (total / (vec ? 4 : 1) + 255) / 256;
  if (blocks > 2048 * 8) blocks = 2048 * 8;
  if (vec)
    hipLaunchKernelGGL((avg_pool2x2_nhwc_kernel<4>), dim3((unsigned)blocks), dim3(256), 0, stream,
                       in, out, (int)B, (int)H, (int)W, (int)C);
  else
    hipLaunchKernelGGL((avg_pool2x2_nhwc_kernel<1>), dim3((unsigned)blocks), dim3(256), 0, stream,
                       in, out, (int)B, (int)H, (int)W, (int)C);
  return dxr::launch_status();
}

namespace {
// ---------------------------------------------------------------------------
// A coarse level's whole volume as one tiled GEMM (round 6): every (query, cell)
// sum of the level, raw, into that level's pages of the volume buffer — the FULL
// form's output (and so the on-the-fly lookup's dot products) bit for bit, since
// each sum is the same three f16 products per k step (split8_f16 operands, cell
// vectors as the A rows, queries as the B columns of v_mfma_f32_32x32x16_f16,
// cross terms in a second accumulator folded by 2^-11 at the end) in the same k
// order; only the tiling differs.  The FULL form streams every cell of the level
// through each 32-query workgroup (1080p level 2: 337 us per block); here one
// workgroup = one page's 128 queries x 128 cells (128 / T whole tiles of the
// level, T = th * tw cells per tile, i.e. 128 / T consecutive pages), four waves
// of 64 cells x 64 queries (2 x 2 MFMA tiles), so each loaded operand feeds 64
// MFMA columns instead of 32 and the split is paid once per workgroup.
// K runs in stages of 32 channels: every thread loads 8 float4 (4 of cells, 4 of
// queries) one stage ahead, splits them and writes hi / lo to a double-buffered
// LDS stage laid out [operand][plane][k step][row][kh] x 16 B, so every MFMA
// fragment read is a conflict-free ds_read_b128 over 1 KB contiguous per wave
// (blocks padded by 128 B so the split's 8-B writes of the two k steps of a row
// land in different banks).  A 32 x 32 tile whose sums are not finite is redone
// from fmap1 / fmap2 on the 3-way bf16 split (six products, the windowed form's
// fallback arithmetic).  Rows past the level or the query count compute zeros;
// pages past the level's last tile are not written.  C % 32 == 0.
constexpr int VG_BLK = 4096 + 128;            // one [row][kh] block of 128 rows x 32 B
constexpr int VG_STAGE = 8 * VG_BLK;          // [operand][plane][k step] blocks

// XA (experiments only; 0 in the product): bit 0 stores only sums equal to
// 12345.0 (none: an ablation of the stores), bit 1 writes the raw f32 bits as the
// hi / lo planes (no split VALU; results meaningless), bit 2 skips the MFMAs.
// CT: the stored cell type.  float: the sums as they are.  _Float16 (DXR_ALT_VOL_F16):
// each float32 sum rounded once to nearest even in the store (v_cvt_f16_f32: overflow to
// +-inf, subnormals kept), so the buffer is the float32 buffer's .half() element for
// element; the non-finite test below looks at the float32 sums, before the rounding.
template <int T, bool DMA, int XA = 0, typename CT = float>
__global__ __launch_bounds__(256, 2) void alt_volume_gemm_kernel(
    const float* __restrict__ f1, const float* __restrict__ f2, CT* __restrict__ out,
    dxr::LevelLayout vl, int N, int C, int ngroups, const _Float16* __restrict__ p1,
    const _Float16* __restrict__ p2) {
  static_assert(T == 2 || T == 8 || T == 32 || T == 128, "tiled levels 0-3 only");
  constexpr int TPG = 128 / T;                 // level tiles (pages) per workgroup
  __shared__ __attribute__((aligned(16))) unsigned char lds[DMA ? 4 * 16384 : 2 * VG_STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, kh = lane >> 5;
  const int wc = wave & 1, wq = wave >> 1;     // the wave's 64-cell / 64-query half
  // contiguous bands of (query block, cell group) per XCD (csrc/corr_build.hip's
  // banded_coord bijection): one XCD's workgroups share their query block's operand in L2
  const int n = gridDim.x, q8 = n / 8, r8 = n % 8, xcd = (int)blockIdx.x % 8;
  const int idx = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) +
                  (int)blockIdx.x / 8;
  const int qblk = idx / ngroups, grp = idx - qblk * ngroups;
  const int b = blockIdx.z;
  const int ntiles = vl.ty * vl.tx;
  const float* f1b = f1 + (long long)b * N * C;
  const float* f2b = f2 + (long long)b * vl.h * vl.w * C;
  // element offset of cell row i (0..127) of this workgroup's group, -1 past the level
  auto cell_off = [&](int i) -> int {
    const int tile = grp * TPG + i / T, c = i % T;
    if (tile >= ntiles) return -1;
    const int ty = tile / vl.tx, tx = tile - ty * vl.tx;
    const int cy = ty * vl.th + c / vl.tw, cx = tx * vl.tw + c % vl.tw;
    return (cy < vl.h && cx < vl.w) ? (cy * vl.w + cx) * C : -1;
  };
  auto query_off = [&](int i) -> int {
    const int q = qblk * 128 + i;
    return q < N ? q * C : -1;
  };
  f32x16_t acc[2][2], acc2[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][q][r] = acc2[a][q][r] = 0.f;
  // one k step of the wave's 2 x 2 tiles: the windowed form's three products
  auto mfma_step = [&](const f16x8_t (&th)[2], const f16x8_t (&tl)[2], const f16x8_t (&qh)[2],
                       const f16x8_t (&ql)[2]) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if constexpr ((XA & 4) != 0) {
          acc[a][q][0] += (float)th[a][0] * (float)qh[q][1] + (float)tl[a][2] * (float)ql[q][3];
          continue;
        }
        acc2[a][q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(tl[a], qh[q], acc2[a][q], 0, 0, 0);
        acc2[a][q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(th[a], ql[q], acc2[a][q], 0, 0, 0);
        acc[a][q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(th[a], qh[q], acc[a][q], 0, 0, 0);
      }
  };
  if constexpr (DMA) {
    // operands pre-split (alt_split_planes_kernel: [pair][hi | lo][k step][row][16]
    // f16) and staged by LDS-DMA, one k step (16 channels) per ring slot, NS slots: no
    // staging VGPRs and no split VALU in the loop, NS - 1 k steps of loads in flight.
    // Slot layout [operand][plane][row block of 32][row][kh] x 16 B: one DMA
    // instruction (lane l -> row 32 rb + l / 2, kh = l % 2, 16 B) fills one 1 KB row
    // block — from 32 consecutive 32-B records of one k step, so queries read whole
    // lines — and every fragment read is a conflict-free ds_read_b128 of 1 KB per
    // wave.  Wave w moves operand w / 2 (0 cells, 1 queries), plane w % 2; rows past
    // the level or the query count read out of the buffer's range, i.e. zeros.
    constexpr int NS = 4, SLOT = 16384;
    const int o = wave >> 1, pl = wave & 1;
    const int rows_o = o == 0 ? vl.h * vl.w : N;
    const _Float16* pbase = (o == 0 ? p2 : p1) + ((long long)b * 2 + pl) * rows_o * C;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<_Float16*>(pbase), (short)0, rows_o * C * 2, 0x00020000);
    uint32_t voff[4];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
      const int row = rb * 32 + (lane >> 1);
      const int e = o == 0 ? cell_off(row) : query_off(row);   // row * C, or -1
      voff[rb] = e >= 0 ? (uint32_t)(e / C) * 32u + (uint32_t)(lane & 1) * 16u : 0x80000000u;
    }
    const int kstride = rows_o * 32;               // bytes per k step of a plane
    const int wslot = __builtin_amdgcn_readfirstlane((o * 2 + pl) * 4096);
    auto issue = [&](int ks) {
      unsigned char* dst = lds + (ks % NS) * SLOT + wslot;
#pragma unroll
      for (int rb = 0; rb < 4; ++rb)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(dst + rb * 1024), 16, voff[rb],
                                                 ks * kstride, 0, 0);
    };
    const int nks = C / 16;
#pragma unroll
    for (int u = 0; u < NS - 1; ++u)
      if (u < nks) issue(u);
    for (int ks = 0; ks < nks; ++ks) {
      // this wave's DMAs of step ks done (those of the younger steps may fly), then
      // everyone's: the barrier also retires the reads of the slot refilled below
      const int younger = min(NS - 2, nks - 1 - ks);
      if (younger >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else if (younger == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (ks + NS - 1 < nks) issue(ks + NS - 1);
      const unsigned char* st = lds + (ks % NS) * SLOT;
      f16x8_t th[2], tl[2], qh[2], ql[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int rc = (wc * 2 + a) * 1024 + j * 32 + kh * 16;
        const int rq = (wq * 2 + a) * 1024 + j * 32 + kh * 16;
        th[a] = __builtin_bit_cast(f16x8_t, *reinterpret_cast<const uint4*>(st + 0 * 4096 + rc));
        tl[a] = __builtin_bit_cast(f16x8_t, *reinterpret_cast<const uint4*>(st + 1 * 4096 + rc));
        qh[a] = __builtin_bit_cast(f16x8_t, *reinterpret_cast<const uint4*>(st + 2 * 4096 + rq));
        ql[a] = __builtin_bit_cast(f16x8_t, *reinterpret_cast<const uint4*>(st + 3 * 4096 + rq));
      }
      mfma_step(th, tl, qh, ql);
    }
  } else {
    // this thread's 8 load slots: slot i < 4 cells, else queries; piece t + 256 (i % 4)
    // -> row piece / 8, channels 4 (piece % 8) .. + 4 of the stage
    int off[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int piece = tid + 256 * (i & 3), row = piece >> 3;
      off[i] = i < 4 ? cell_off(row) : query_off(row);
    }
    const int f4 = tid & 7;
    const int ch = 4 * f4;
    // LDS byte offset of this thread's 8-B hi write for slot i (lo: + 2 VG_BLK)
    auto wr_addr = [&](int i) -> int {
      const int row = (tid + 256 * (i & 3)) >> 3, o = i >> 2;
      return ((o * 2 + 0) * 2 + (f4 >> 2)) * VG_BLK + row * 32 + ((f4 >> 1) & 1) * 16 + (f4 & 1) * 8;
    };
    float4 pre[8];
    auto load_stage = [&](int s) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float* base = i < 4 ? f2b : f1b;
        pre[i] = off[i] >= 0 ? *reinterpret_cast<const float4*>(base + off[i] + 32 * s + ch)
                             : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    };
    auto write_stage = [&](int buf) {
      unsigned char* st = lds + buf * VG_STAGE;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float4 v = pre[i];
        uint32_t h0, h1, l0, l1;
        if constexpr ((XA & 2) != 0) {
          h0 = __float_as_uint(v.x); h1 = __float_as_uint(v.y);
          l0 = __float_as_uint(v.z); l1 = __float_as_uint(v.w);
        } else {
          // split2_f16 of (x, y) and (z, w), both hi words first: through the
          // pair function this kernel's instructions come out in another order
          h0 = cvt_pk_f16(v.x, v.y);
          h1 = cvt_pk_f16(v.z, v.w);
          const f16x2_t a0 = __builtin_bit_cast(f16x2_t, h0), a1 = __builtin_bit_cast(f16x2_t, h1);
          l0 = cvt_pk_f16((v.x - (float)a0[0]) * 2048.f, (v.y - (float)a0[1]) * 2048.f);
          l1 = cvt_pk_f16((v.z - (float)a1[0]) * 2048.f, (v.w - (float)a1[1]) * 2048.f);
        }
        const int a = wr_addr(i);
        *reinterpret_cast<uint2*>(st + a) = make_uint2(h0, h1);
        *reinterpret_cast<uint2*>(st + a + 2 * VG_BLK) = make_uint2(l0, l1);
      }
    };
    const int nst = C / 32;
    load_stage(0);
    write_stage(0);
    __syncthreads();
    for (int s = 0; s < nst; ++s) {
      if (s + 1 < nst) load_stage(s + 1);
      const unsigned char* st = lds + (s & 1) * VG_STAGE;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        f16x8_t th[2], tl[2], qh[2], ql[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          const int rc = (wc * 64 + a * 32 + j) * 32 + kh * 16;
          const int rq = (wq * 64 + a * 32 + j) * 32 + kh * 16;
          th[a] = __builtin_bit_cast(f16x8_t, *reinterpret_cast<const uint4*>(st + (0 + ks) * VG_BLK + rc));
          tl[a] = __builtin_bit_cast(f16x8_t, *reinterpret_cast<const uint4*>(st + (2 + ks) * VG_BLK + rc));
          qh[a] = __builtin_bit_cast(f16x8_t, *reinterpret_cast<const uint4*>(st + (4 + ks) * VG_BLK + rq));
          ql[a] = __builtin_bit_cast(f16x8_t, *reinterpret_cast<const uint4*>(st + (6 + ks) * VG_BLK + rq));
        }
        mfma_step(th, tl, qh, ql);
      }
      if (s + 1 < nst) write_stage((s + 1) & 1);
      __syncthreads();
    }
  }
  const long long page0 = ((long long)b * vl.qt + qblk) * ntiles + (long long)grp * TPG;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      bool bad = false;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        acc[a][q][r] = __builtin_fmaf(acc2[a][q][r], 0x1p-11f, acc[a][q][r]);
        bad |= !(__builtin_fabsf(acc[a][q][r]) <= 3.40282347e38f);
      }
      if ((XA & 6) == 0 && __ballot(bad) != 0) {   // wave-uniform: the tile on the 3-way bf16 split
        const int co = cell_off(wc * 64 + a * 32 + j), qo = query_off(wq * 64 + q * 32 + j);
        f32x16_t f = {};
        for (int ks = 0; ks < C / 16; ++ks) {
          float x[8], y[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            x[e] = co >= 0 ? f2b[co + 16 * ks + 8 * kh + e] : 0.f;
            y[e] = qo >= 0 ? f1b[qo + 16 * ks + 8 * kh + e] : 0.f;
          }
          uint4 h, m, l, uh, um, ul;
          split8_bf16<Bf16Split::GUARD_INF>(x, h, m, l);
          split8_bf16<Bf16Split::GUARD_INF>(y, uh, um, ul);
          const bf16x8_t th = __builtin_bit_cast(bf16x8_t, h), tm = __builtin_bit_cast(bf16x8_t, m),
                     tl = __builtin_bit_cast(bf16x8_t, l);
          const bf16x8_t qh = __builtin_bit_cast(bf16x8_t, uh), qm = __builtin_bit_cast(bf16x8_t, um),
                     ql = __builtin_bit_cast(bf16x8_t, ul);
          f = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tm, qm, f, 0, 0, 0);
          f = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tl, qh, f, 0, 0, 0);
          f = __builtin_amdgcn_mfma_f32_32x32x16_bf16(th, ql, f, 0, 0, 0);
          f = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tm, qh, f, 0, 0, 0);
          f = __builtin_amdgcn_mfma_f32_32x32x16_bf16(th, qm, f, 0, 0, 0);
          f = __builtin_amdgcn_mfma_f32_32x32x16_bf16(th, qh, f, 0, 0, 0);
        }
        acc[a][q] = f;
      }
      // lane (j, kh) holds rows (r & 3) + 8 (r >> 2) + 4 kh of column j: runs of four
      // consecutive cells, i.e. one 16-B store into one page (T >= 4) or two 8-B
      // stores into two (T = 2)
      const int ql_ = wq * 64 + q * 32 + j;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int row = wc * 64 + a * 32 + 8 * g4 + 4 * kh;
        const float4 v = make_float4(acc[a][q][4 * g4], acc[a][q][4 * g4 + 1],
                                     acc[a][q][4 * g4 + 2], acc[a][q][4 * g4 + 3]);
        if constexpr ((XA & 1) != 0)
          if (v.x != 12345.f) continue;
        if constexpr (std::is_same_v<CT, _Float16>) {
          // float16 cells: the same runs as one 8-B store, or two 4-B stores (T = 2)
          const uint32_t h01 = dxr::out16_bits<_Float16>(v.x) | (dxr::out16_bits<_Float16>(v.y) << 16);
          const uint32_t h23 = dxr::out16_bits<_Float16>(v.z) | (dxr::out16_bits<_Float16>(v.w) << 16);
          if constexpr (T >= 4) {
            const int t = row / T;
            if (grp * TPG + t < ntiles)
              *reinterpret_cast<uint2*>(out + vl.off + ((page0 + t) * 128 + ql_) * T + row % T) =
                  make_uint2(h01, h23);
          } else {
            const int t = row / 2;
            if (grp * TPG + t < ntiles)
              *reinterpret_cast<uint32_t*>(out + vl.off + ((page0 + t) * 128 + ql_) * 2) = h01;
            if (grp * TPG + t + 1 < ntiles)
              *reinterpret_cast<uint32_t*>(out + vl.off + ((page0 + t + 1) * 128 + ql_) * 2) = h23;
          }
        } else if constexpr (T >= 4) {
          const int t = row / T;
          if (grp * TPG + t < ntiles)
            *reinterpret_cast<float4*>(out + vl.off + ((page0 + t) * 128 + ql_) * T + row % T) = v;
        } else {
          const int t = row / 2;
          if (grp * TPG + t < ntiles)
            *reinterpret_cast<float2*>(out + vl.off + ((page0 + t) * 128 + ql_) * 2) =
                make_float2(v.x, v.y);
          if (grp * TPG + t + 1 < ntiles)
            *reinterpret_cast<float2*>(out + vl.off + ((page0 + t + 1) * 128 + ql_) * 2) =
                make_float2(v.z, v.w);
        }
      }
    }
}

// f16 pair planes of `rows` f32 rows of C channels per pair, k-step-major so one
// k step (16 channels) of consecutive rows is contiguous: out[pair][plane][ks][row][16]
// with plane 0 = RNE_f16(x), plane 1 = RNE_f16((x - hi) * 2^11) — split8_f16 per
// element, so the DMA form's products are the register form's.  Thread = 4
// channels of a row, row-major (a wave reads 1 KB contiguous; its 8-B writes form
// 32-B runs whose neighbours — the next rows' — the next waves write).
__global__ __launch_bounds__(256) void alt_split_planes_kernel(const float* __restrict__ in,
                                                               _Float16* __restrict__ out,
                                                               long long rows, int C,
                                                               long long n4) {
  const int c4n = C / 4;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n4;
       t += (long long)gridDim.x * 256) {
    const long long prow = t / c4n;
    const int c = (int)(t - prow * c4n) * 4;
    const long long pair = prow / rows, row = prow - pair * rows;
    const float4 v = *reinterpret_cast<const float4*>(in + 4 * t);
    const Split2 s0 = split2_f16(v.x, v.y), s1 = split2_f16(v.z, v.w);
    _Float16* o = out + pair * 2 * rows * C + ((long long)(c >> 4) * rows + row) * 16 + (c & 15);
    *reinterpret_cast<uint2*>(o) = make_uint2(s0.h, s1.h);
    *reinterpret_cast<uint2*>(o + rows * C) = make_uint2(s0.l, s1.l);
  }
}

int launch_split_planes(const float* in, _Float16* out, long long B, long long rows, int C,
                        hipStream_t stream) {
  const long long n4 = B * rows * C / 4;
  const long long blocks = std::min<long long>((n4 + 255) / 256, 16384);
  hipLaunchKernelGGL(alt_split_planes_kernel, dim3((unsigned)std::max<long long>(blocks, 1)),
                     dim3(256), 0, stream, in, out, rows, C, n4);
  return dxr::launch_status();
}

// one level's volume by alt_volume_gemm_kernel (tiled levels 0-3, C % 32 == 0);
// with f16 pair planes of both operands (p1, p2) the LDS-DMA form; CT: the cell type
template <int XA = 0, typename CT = float>
int launch_alt_volume_gemm(const float* f1, const float* f2, CT* vol, const dxr::LevelLayout& vl,
                           int B, int N, int C, hipStream_t stream,
                           const _Float16* p1 = nullptr, const _Float16* p2 = nullptr) {
  const int T = vl.th * vl.tw;
  const int ngroups = (vl.ty * vl.tx + 128 / T - 1) / (128 / T);
  const long long nwg = (long long)vl.qt * ngroups;
  if (nwg > 0x7fffffffLL || (long long)N * C > 0x3fffffffLL ||
      (long long)vl.h * vl.w * C > 0x3fffffffLL)
    return DXR_EUNSUPPORTED;
  const dim3 grid((unsigned)nwg, 1u, (unsigned)B);
  const bool dma = p1 != nullptr && p2 != nullptr;
#define DXR_VG(TT)                                                                              \
  if (dma)                                                                                      \
    hipLaunchKernelGGL((alt_volume_gemm_kernel<TT, true, XA, CT>), grid, dim3(256), 0, stream, \
                       f1, f2, vol, vl, N, C, ngroups, p1, p2);                                 \
  else                                                                                          \
    hipLaunchKernelGGL((alt_volume_gemm_kernel<TT, false, XA, CT>), grid, dim3(256), 0, stream, \
                       f1, f2, vol, vl, N, C, ngroups, p1, p2);
  switch (T) {
    case 2: DXR_VG(2) break;
    case 8: DXR_VG(8) break;
    case 32: DXR_VG(32) break;
    case 128: DXR_VG(128) break;
    default: return DXR_EUNSUPPORTED;
  }
#undef DXR_VG
  return dxr::launch_status();
}
}  // namespace

// ---------------------------------------------------------------------------
// Coarse-level volumes (round 6).  An on-the-fly lookup pays each level's box
// GEMMs again on every call, ~26 us per level and 1080p lookup whatever the
// level's size; a coarse level's whole correlation volume costs less than one
// such lookup to compute once per block.  dxr_alt_coarse_volumes computes levels
// [first_level, num_levels) of fmap1 against the pooled fmap2 levels (the
// alternate block's own operands) — the tiled levels (0-3) by
// alt_volume_gemm_kernel when C % 32 == 0, others by the FULL form of the box
// kernel, the same sums either way — and
// stores them, raw, in the paged layout of those pyramid levels, one buffer of
// dxr_alt_volume_numel floats; dxr_alt_volume_lookup (csrc/corr_lookup.hip)
// reads its windows from there with the alternate block's arithmetic.
extern "C" int64_t dxr_alt_volume_numel(int64_t B, int64_t H, int64_t W, int num_levels,
                                        int first_level) {
  dxr::Levels L;
  if (!dxr::make_levels(B, H, W, num_levels, &L) || first_level < 0 || first_level >= num_levels)
    return -1;
  return L.numel - L.off[first_level];
}

namespace {
// Bytes of the f16 pair planes the DMA form of the volume GEMM reads (fmap1 and
// each tiled level >= first_level of fmap2, 2 x 2 B per element, 256-B aligned
// regions); 0 when no level takes the GEMM.
long long alt_volume_planes_bytes(const dxr::Levels& L, int64_t B, int64_t H, int64_t W, int64_t C,
                                  int num_levels, int first_level, long long* level_off) {
  if (C % 32 != 0 || first_level >= dxr::TILED_LEVELS) return 0;
  auto up = [](long long x) { return (x + 255) / 256 * 256; };
  long long off = up(B * H * W * C * 4);
  for (int l = first_level; l < num_levels && l < dxr::TILED_LEVELS; ++l) {
    if (level_off) level_off[l] = off;
    off += up(B * (long long)L.h[l] * L.w[l] * C * 4);
  }
  return off;
}

// full_form: every level by the FULL box kernel (experiments: the round-6 first form);
// ws (>= alt_volume_planes_bytes): the GEMM's LDS-DMA form on pre-split planes.
// DXR_ALT_VOL_F16 on first_level (the low byte is the level): `volumes` holds float16
// cells, stored by the volume GEMM itself, so every level must take that GEMM.
int alt_coarse_volumes(const float* fmap1, const float* const* fmap2_levels, int64_t B, int64_t H,
                       int64_t W, int64_t C, int num_levels, int first_level, float* volumes,
                       hipStream_t stream, bool full_form, void* ws = nullptr,
                       int64_t ws_bytes = 0) {
  // (any other bit above the low byte leaves first_level >= num_levels: DXR_EINVAL below)
  const bool vol16 = first_level >= 0 && (first_level & ~0xff) == DXR_ALT_VOL_F16;
  if (vol16) first_level &= 0xff;
  dxr::Levels L;
  if (!dxr::make_levels(B, H, W, num_levels, &L) || first_level < 0 || first_level >= num_levels)
    return DXR_EINVAL;
  if (C < 1 || B > 65535 || H * W > (1LL << 30)) return DXR_EINVAL;
  if (C % 16 != 0 || C > 256) return DXR_EUNSUPPORTED;
  // float16 cells: the tiled GEMM's stores only (the FULL form and a row-major level store
  // float32); the caller builds float32 volumes and rounds them: the same buffer
  if (vol16 && (C % 32 != 0 || num_levels > dxr::TILED_LEVELS || full_form))
    return DXR_EUNSUPPORTED;
  if (B == 0) return DXR_OK;
  if (!fmap1 || !fmap2_levels || !volumes || !aligned16(fmap1)) return DXR_EINVAL;
  if (vol16 && !aligned16(volumes)) return DXR_EINVAL;
  AltGeom g;
  g.N = (int)(H * W);
  g.C = (int)C;
  g.Nc = 1;
  g.cout = 0;
  g.divisor = 1.f;
  g.f1_bstride = H * W * C;
  g.coord_zstride = g.coord_cstride = 0;
  g.coord_qstride = 0;
  const int tiles_x = (int)((W + TQX - 1) / TQX);
  const int ntiles = tiles_x * (int)((H + TQY - 1) / TQY);
  long long loff[8] = {};
  const long long pbytes = alt_volume_planes_bytes(L, B, H, W, C, num_levels, first_level, loff);
  _Float16* planes = nullptr;
  if (!full_form && pbytes > 0 && ws != nullptr && ws_bytes >= pbytes && aligned16(ws)) {
    planes = static_cast<_Float16*>(ws);
    int st = launch_split_planes(fmap1, planes, B, H * W, (int)C, stream);
    if (st != DXR_OK) return st;
  }
  for (int l = first_level; l < num_levels; ++l) {
    if (!fmap2_levels[l] || !aligned16(fmap2_levels[l])) return DXR_EINVAL;
    g.lv[0] = AltLevel{fmap2_levels[l], L.h[l], L.w[l], 1.f, 0};
    g.vlay = L.lay[l];
    g.vlay.off -= L.off[first_level];
    if (l < dxr::TILED_LEVELS && C % 32 == 0 && !full_form) {
      _Float16* p2 = nullptr;
      if (planes) {
        p2 = reinterpret_cast<_Float16*>(static_cast<unsigned char*>(ws) + loff[l]);
        const int st = launch_split_planes(fmap2_levels[l], p2, B, (long long)L.h[l] * L.w[l],
                                           (int)C, stream);
        if (st != DXR_OK) return st;
      }
      const int st =
          vol16 ? launch_alt_volume_gemm<0, _Float16>(fmap1, fmap2_levels[l],
                                                      reinterpret_cast<_Float16*>(volumes), g.vlay,
                                                      (int)B, g.N, (int)C, stream, planes, p2)
                : launch_alt_volume_gemm(fmap1, fmap2_levels[l], volumes, g.vlay, (int)B, g.N,
                                         (int)C, stream, planes, p2);
      if (st != DXR_OK) return st;
      continue;
    }
    hipLaunchKernelGGL((alt_corr_mfma_kernel<0, 3, false, 4, 0, 0, true>),
                       dim3((unsigned)ntiles, 1u, (unsigned)B), dim3(256), 0, stream, fmap1,
                       (const float*)nullptr, volumes, g, (int)W, tiles_x, (const int4*)nullptr,
                       0LL, 0, 0);
    const int st = dxr::launch_status();
    if (st != DXR_OK) return st;
  }
  return DXR_OK;
}
}  // namespace

extern "C" int dxr_alt_coarse_volumes(const float* fmap1, const float* const* fmap2_levels,
                                      int64_t B, int64_t H, int64_t W, int64_t C, int num_levels,
                                      int first_level, float* volumes, hipStream_t stream) {
  return alt_coarse_volumes(fmap1, fmap2_levels, B, H, W, C, num_levels, first_level, volumes,
                            stream, false);
}

extern "C" int64_t dxr_alt_coarse_volumes_ws_bytes(int64_t B, int64_t H, int64_t W, int64_t C,
                                                   int num_levels, int first_level) {
  dxr::Levels L;
  if (!dxr::make_levels(B, H, W, num_levels, &L) || first_level < 0 ||
      first_level >= num_levels || C < 1)
    return -1;
  return alt_volume_planes_bytes(L, B, H, W, C, num_levels, first_level, nullptr);
}

extern "C" int dxr_alt_coarse_volumes_ws(const float* fmap1, const float* const* fmap2_levels,
                                         int64_t B, int64_t H, int64_t W, int64_t C,
                                         int num_levels, int first_level, float* volumes,
                                         void* workspace, int64_t workspace_bytes,
                                         hipStream_t stream) {
  return alt_coarse_volumes(fmap1, fmap2_levels, B, H, W, C, num_levels, first_level, volumes,
                            stream, false, workspace, workspace_bytes);
}

namespace {
// The three lookup entry points: planned once (lookup_plan.h: every check in its
// order, the unit, the form, whether the workspace is used), then to the unit the
// plan names.  The level pointers are read between the planner's two halves, once
// the array is known to hold them.
int alt_lookup_entry(const float* fmap1, const float* const* fmap2_levels, const float* coords,
                     float* out, int64_t B, int64_t H, int64_t W, int64_t C, int num_levels,
                     int radius, float divisor, void* workspace, int64_t workspace_bytes,
                     hipStream_t stream, int n_levels, bool levels_call) {
  dxr::AltLookupRequest r{B, H, W, C, num_levels, n_levels, levels_call, radius, divisor,
                          (uintptr_t)fmap1, (uintptr_t)fmap2_levels, (uintptr_t)coords,
                          (uintptr_t)out, {}, (uintptr_t)workspace, workspace_bytes};
  dxr::AltLookupPlan plan;
  int st = dxr::plan_alt_args(r, &plan);
  if (st != DXR_OK || B == 0) return st;
  for (int l = 0; l < plan.levels; ++l) r.level[l] = (uintptr_t)fmap2_levels[l];
  st = dxr::plan_alt_form(r, &plan);
  if (st != DXR_OK) return st;
  const dxr::AltLookupArgs a{&plan, fmap1, fmap2_levels, coords, out, B, H, W, C, num_levels, divisor,
                             workspace, stream};
  switch (plan.unit) {
    // 16-bit fmap1 and level 0, with or without output flags
    case dxr::ALT_UNIT_INBF16: return dxr::alt_lookup_inbf16(a);
    case dxr::ALT_UNIT_IN16: return dxr::alt_lookup_in16(a);
    case dxr::ALT_UNIT_OUT: return dxr::alt_lookup_out(a);
    default: return alt_lookup_forms<dxr::FORM_F32>(a);
  }
}
}  // namespace

extern "C" int dxr_alt_corr_lookup(const float* fmap1, const float* const* fmap2_levels,
                                   const float* coords, float* out, int64_t B, int64_t H,
                                   int64_t W, int64_t C, int num_levels, int radius,
                                   float divisor, hipStream_t stream) {
  return alt_lookup_entry(fmap1, fmap2_levels, coords, out, B, H, W, C, num_levels, radius, divisor,
                          nullptr, 0, stream, -1, false);
}

extern "C" int64_t dxr_alt_workspace_bytes(int64_t B, int64_t H, int64_t W, int num_levels) {
  return dxr::alt_workspace_bytes(B, H, W, num_levels);
}

extern "C" int dxr_alt_corr_lookup_ws(const float* fmap1, const float* const* fmap2_levels,
                                      const float* coords, float* out, int64_t B, int64_t H,
                                      int64_t W, int64_t C, int num_levels, int radius,
                                      float divisor, void* workspace, int64_t workspace_bytes,
                                      hipStream_t stream) {
  return alt_lookup_entry(fmap1, fmap2_levels, coords, out, B, H, W, C, num_levels, radius, divisor,
                          workspace, workspace_bytes, stream, -1, false);
}

extern "C" int dxr_alt_corr_lookup_levels_ws(const float* fmap1, const float* const* fmap2_levels,
                                             const float* coords, float* out, int64_t B, int64_t H,
                                             int64_t W, int64_t C, int num_levels, int n_levels,
                                             int radius, float divisor, void* workspace,
                                             int64_t workspace_bytes, hipStream_t stream) {
  return alt_lookup_entry(fmap1, fmap2_levels, coords, out, B, H, W, C, num_levels, radius, divisor,
                          workspace, workspace_bytes, stream, n_levels, true);
}

#endif  // DXR_TEMPLATES_ONLY
