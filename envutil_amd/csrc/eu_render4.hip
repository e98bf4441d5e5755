// Packed render kernel with PER-WAVE LDS staging of the b-spline footprint.
//
// A wavefront (a workgroup of its own: no barrier, no tail behind a slower sibling) owns a
// 16x8 output tile (two horizontally adjacent pixels per lane) and a slice of LDS. It
//   1. computes the source coordinates of its 128 pixels (eu_packed_dev.h: the same float2
//      arithmetic as eu_render2_kernel, the reference's operations in the reference's
//      order, without the scalar fallbacks); where the stepper's row constants make the
//      source COLUMN a function of the target column alone (an upright cubemap /
//      rectilinear / cylindrical target of a lat/lon source: stepper.h hoists the same
//      invariants per segment), that half of the chain - the longitude atan2f, the square
//      root, the x gate, split and weights - comes from a per-column table that a small
//      pre-pass kernel fills with the very same device functions (eu_render5_kernel, the
//      form for lat/lon sources; eu_render4s_kernel serves cubemap and biatan6 sources),
//   2. reduces the integer base positions to the tile's bounding box (DPP row shifts +
//      row broadcasts, no LDS traffic, no barrier),
//   3. copies the box from the braced container straight into LDS with LDS-DMA
//      (global_load_lds_dwordx4, one instruction per box row: every lane fetches ONE
//      texel, 16 bytes from its own 4-byte-aligned source address - an RGB texel plus one
//      float that is never read - so the LDS image is made of aligned 16-byte texels, rows
//      back to back, without a single VGPR or ds_write),
//   4. evaluates the (d+1)^2 taps of both pixels with ds_read_b128 and the reference's
//      weighted sum (zimt/eval.h:904-1059), and
//   5. stores 24 contiguous bytes per lane (192 per row and wave).
// Every source texel of the box passes the vector memory pipe once per tile instead of
// once per tap and lane quad: the L1 (TCP) tag rate that bounds eu_render2_kernel (7.0
// line accesses per output pixel) drops to the staging traffic (1.8).
//
// Tiles whose box exceeds the LDS slice (the poles of a lat/lon source, the +-180 degree
// seam, strong minification) and tiles with a lane that needs one of the scalar fallbacks
// of the coordinate arithmetic go to a work list and are rendered by the direct-gather
// kernel behind this one.
//
// Stands in for: zimt::process' get/act/put loop (wielding.h:151-463) with the
// evaluator's gathers (zimt/eval.h:838-889) replaced by LDS reads.
#include <cstdio>
#include <cstring>
#include <vector>
#include <algorithm>
#include "eu_packed_dev.h"
#include "eu_quad_gather.h"
#include "eu_launch.h"
#include "eu_polar_groups.h"

#define EU4_TW 16          // wave tile, pixels
#define EU4_TH 8
#define EU4_WAVES 4        // waves per workgroup of the direct-gather kernel
#ifndef EU4_WAVES0
#define EU4_WAVES0 1       // waves per workgroup of the staged kernel
#define EU4_TEXELS 384     // LDS texels (16 bytes) per wave of the staged kernel: 6 KB + the atanf table (3 KB);
                           // 16 single-wave workgroups per CU (the hardware's limit) use 144 of 160 KB
#define EU4_OCC0 4         // waves per SIMD the registers are capped for
#endif
// the work list of the direct-gather kernel - EU4_SHARDS lists, a tile goes to list eu4_shard_of(id) - and the layout
// of eu_render_params::wl (EU4_WL_*): eu_worklist.h, through eu_launch.h
#define EU4_UNIT_ROWS 4    // tile rows per XCD unit (32 pixel rows)
#define EU4_COL_FLOATS 8   // per-column table: ix, tx, wx[0..3], sqrt(rx^2 + rz^2), longitude
#define EU4_MAX_PLANS 16

// Bounding-box reduction over the wavefront: min of two and max of two registers, all four
// interleaved (a DPP operand written by the preceding VALU instruction needs two wait states;
// three independent instructions sit between dependent ones). Log-step row shifts inside the
// rows of 16 lanes, then the two row broadcasts; lanes without a valid source keep their
// value (the destination is the second operand). Results are valid in lane 63. EXEC must be
// all ones.
__device__ __forceinline__ void eu4_box_reduce(int &mn0, int &mn1, int &mx0, int &mx1)
{
#define EU4_RED(ctrl)                                        \
  "v_min_i32_dpp %0, %0, %0 " ctrl "\n\t"                    \
  "v_min_i32_dpp %1, %1, %1 " ctrl "\n\t"                    \
  "v_max_i32_dpp %2, %2, %2 " ctrl "\n\t"                    \
  "v_max_i32_dpp %3, %3, %3 " ctrl "\n\t"
  asm("s_nop 1\n\t"
      EU4_RED("row_shr:1 row_mask:0xf bank_mask:0xf")
      EU4_RED("row_shr:2 row_mask:0xf bank_mask:0xf")
      EU4_RED("row_shr:4 row_mask:0xf bank_mask:0xf")
      EU4_RED("row_shr:8 row_mask:0xf bank_mask:0xf")
      EU4_RED("row_bcast:15 row_mask:0xa bank_mask:0xf")
      EU4_RED("row_bcast:31 row_mask:0xc bank_mask:0xf")
      "s_nop 0"
      : "+v"(mn0), "+v"(mn1), "+v"(mx0), "+v"(mx1));
#undef EU4_RED
  mn0 = __builtin_amdgcn_readlane(mn0, 63); mn1 = __builtin_amdgcn_readlane(mn1, 63);
  mx0 = __builtin_amdgcn_readlane(mx0, 63); mx1 = __builtin_amdgcn_readlane(mx1, 63);
}

typedef __attribute__((address_space(3))) void *eu4_lds_void;
typedef const __attribute__((address_space(1))) void *eu4_gbl_void;

typedef float eu4_f4 __attribute__((ext_vector_type(4)));   // one 16-byte LDS texel

// one LDS-DMA row: lane c fetches 16 bytes at sb + voff into LDS dst + 16 c (M0 = dst is written
// in the statement that uses it and restored for the compiler)
__device__ __forceinline__ void eu4_dma_row(unsigned dst, unsigned voff, const char *sb)
{
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\t"
               "s_mov_b32 m0, %1\n\t"
               "s_nop 0\n\t"
               "global_load_lds_dwordx4 %2, %3\n\t"
               "s_mov_b32 m0, %0"
               : "=&s"(keep) : "s"(dst), "v"(voff), "s"(sb) : "memory");
}

// what the staged kernel needs besides eu_render_params
struct eu4_plan {
  const float *atab_g;    // the atanf range table (eu_math2.h) in global memory, 768 floats
  const int *tileplan;    // per tile row of the launch: column table to use, -1: none
  const float *coltab;    // [plan][width][EU4_COL_FLOATS]
  int tiles16;            // wave tiles per tile row
  // eu_render5_kernel's second loop (the tile rows without a common column plan), dealt out dynamically: the tile
  // rows XCD x owns in that loop are l2_rows[l2_off[x] .. l2_off[x + 1]) (raster order), a dequeue is one BATCH of
  // two neighbouring tiles of a row; l2_half = ceil(tiles16 / 2) batches per row, l2_magic = floor(2^40 / l2_half) + 1
  const int *l2_rows;
  int l2_off[9];
  int l2_half;
  unsigned long long l2_magic;
  // the first loop's list: entries of EU_SHARE_ENTRY_INTS ints (eu_share_groups.h: a leader double row and the
  // members rendered from its coordinates), those of XCD x at l1_ent[EU_SHARE_ENTRY_INTS * l1_off[x] ...]; an entry
  // covers l1_ecols tile columns; walked with a fixed stride (no queue); l1_magic = floor(2^40 / l1_ecols) + 1
  const int *l1_ent;
  int l1_off[9];
  int l1_ecols;
  unsigned long long l1_magic;
  const int *xtab;        // [plan][tiles16] { min, max } of the column entries' base position ix; min = INT_MAX: not fast
  const int *boxtab;      // the second loop's tile boxes (eu_render5.h: EU5_BT_RECS records per tile of the rows in l2_rows); null: none
  // the second loop's list where it reads the box table: entries of EU_POLAR_ENTRY_INTS ints (eu_polar_groups.h: a leader
  // tile row and the rows rendered from its angles), those of XCD x at l2p_ent[EU_POLAR_ENTRY_INTS * l2p_off[x] ...]; an
  // entry covers l2p_ecols tile columns in l2p_bpe batches of l2p_bcols; l2p_magic = floor(2^40 / l2p_bpe) + 1
  const int *l2p_ent;
  int l2p_off[9];
  int l2p_ecols, l2p_bcols, l2p_bpe;
  unsigned long long l2p_magic;
#ifdef EU5_STAMPS
  unsigned long long *stamps;   // diagnostic build: 8 s_memtime stamps per tile of eu_render5_kernel
#endif
};

#ifdef EU5_STAMPS
#define EU5_STAMP(k) do { asm volatile("" ::: "memory"); st_[k] = __builtin_amdgcn_s_memtime(); asm volatile("" ::: "memory"); } while (0)
#define EU5_STAMP32(k) do { asm volatile("" ::: "memory"); st_[k] = (unsigned)__builtin_amdgcn_s_memtime(); asm volatile("" ::: "memory"); } while (0)
#else
#define EU5_STAMP(k) do { } while (0)
#define EU5_STAMP32(k) do { } while (0)
#endif

// ---------------------------------------------------------------------------
// one tile of the staged kernel
// ---------------------------------------------------------------------------
template <int NCH, int DEG, int PRJ>
__device__ __forceinline__ void eu4_tile(const eu_render_params &p, const eu4_plan &w, const float *atab,
                                         float *wtile, int tile_y, int x0, int lane)
{
  constexpr int TEX = 4;                              // floats per LDS texel
  constexpr int order = DEG + 1;
  const eu_src_dev &s = p.src;
  const int lx = lane & 7, ly = lane >> 3;
  const int y = p.row_begin + tile_y * EU4_TH + ly;
  const bool yin = y < p.row_end;
  const int yc = yin ? y : p.row_end - 1;
  // the stepper's row constants of this lane's row (stepper.h: per-segment invariants)
  const float *rt = p.row + (long long)eu_frame_row(yc, p.band_shift, p.band_count, p.band_index) * EU_ROW_FLOATS;
  const int xa = x0 + 2 * lx, xb = xa + 1;
  const bool va = yin && xa < p.width, vb = yin && xb < p.width;
  const int xac = xa < p.width ? xa : p.width - 1, xbc = xb < p.width ? xb : p.width - 1;

  eu_f2 tx, ty, gy;
  eu_i2 hit, ok = { -1, -1 };
  int ixa, ixb;
  float wxa[order], wxb[order];
  // rays of both pixels (stepper.h: ray = B * c0 (+ C * c1) + A)
  eu_ray2 r;
  {
    const float A0 = rt[0], A1 = rt[1], A2 = rt[2], B0 = rt[3], B1 = rt[4], B2 = rt[5];
    const eu_f2 c0 = { p.col[xac], p.col[xbc] };
    if (p.form == EU_FORM_BCA) {
      const float C0 = rt[6], C1 = rt[7], C2 = rt[8];
      const float *colB = p.col + p.width;
      const eu_f2 c1 = { colB[xac], colB[xbc] };
      r.x = B0 * c0 + C0 * c1 + A0;
      r.y = B1 * c0 + C1 * c1 + A1;
      r.z = B2 * c0 + C2 * c1 + A2;
    } else {
      r.x = B0 * c0 + A0;
      r.y = B1 * c0 + A1;
      r.z = B2 * c0 + A2;
    }
    if (p.norm_mode == EU_NORM_DIV) {
      eu_f2 sqn = r.x * r.x; sqn = sqn + r.y * r.y; sqn = sqn + r.z * r.z;
      const eu_f2 n = { sqrtf(sqn.x), sqrtf(sqn.y) };
      r.x = r.x / n; r.y = r.y / n; r.z = r.z / n;
    }
  }
  // the atanf table is complete behind this wait (LDS-DMA, issued at kernel entry)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  eu_f2 sx, sy;
  hit = eu_coord2_ok<PRJ>(s, r, sx, sy, atab, ok);
  const eu_f2 gx = eu_gate2_ok(sx, s.gate0, s.lower0, s.upper0, ok);
  gy = eu_gate2_ok(sy, s.gate1, s.lower1, s.upper1, ok);
  eu_f2 fx;
  if constexpr (DEG & 1) fx = (eu_f2){ floorf(gx.x), floorf(gx.y) };
  else fx = (eu_f2){ roundf(gx.x), roundf(gx.y) };
  tx = gx - fx;
  ixa = (int)fx.x; ixb = (int)fx.y;
  hit = hit & (eu_i2){ va ? -1 : 0, vb ? -1 : 0 };
  eu_f2 fy;
  if constexpr (DEG & 1) fy = (eu_f2){ floorf(gy.x), floorf(gy.y) };
  else fy = (eu_f2){ roundf(gy.x), roundf(gy.y) };
  ty = gy - fy;
  const int iya = (int)fy.x, iyb = (int)fy.y;

  // bounding box of the base positions of the tile's hitting pixels
  int mnx = INT_MAX, mny = INT_MAX, mxx = INT_MIN, mxy = INT_MIN;
  if (hit.x) { mnx = ixa; mxx = ixa; mny = iya; mxy = iya; }
  if (hit.y) { mnx = min(mnx, ixb); mxx = max(mxx, ixb); mny = min(mny, iyb); mxy = max(mxy, iyb); }
  eu4_box_reduce(mnx, mny, mxx, mxy);
  const bool any = mnx != INT_MAX;
  const long long bw = (long long)mxx - mnx + order, bh = (long long)mxy - mny + order;
  // the LDS image is the box itself, rows of bw texels back to back (pitch = bw: no padding;
  // rows an odd number of 16-byte texels apart spread over the banks)
  const bool fits = bw <= 64 && bh <= EU4_TEXELS && bw * bh <= EU4_TEXELS;
  // a hitting pixel that left the fast path of the coordinate arithmetic?
  const bool clean = __ballot((hit.x && !ok.x) || (hit.y && !ok.y)) == 0ull;
  float *const orow = p.out + (long long)(yc - p.row_begin) * p.out_stride;
  if (any && !(fits && clean)) {
    // left to the direct-gather kernel: one of EU4_SHARDS lists (a single counter serialises:
    // ~88 returning atomics per microsecond on one word)
    if (lane == 0) {
      const int id = tile_y * w.tiles16 + x0 / EU4_TW;
      const int sh = eu4_shard_of(id);
      const int slot = atomicAdd(p.wl + EU4_WL_SHARD(sh), 1);
      p.wl[EU4_WL_ENTRIES + (size_t)slot * EU4_SHARDS + sh] = id;
    }
    return;
  }
  float qa[NCH], qb[NCH];
  if (any) {
    // stage: one LDS-DMA instruction per box row, lane c fetches the texel of box column c;
    // the address arithmetic is scalar
    const int ibw = (int)bw, ibh = (int)bh;
    const unsigned lds_tile = (unsigned)(unsigned long long)(eu4_lds_void)wtile;
    if (lane < ibw) {
      const int bx0 = mnx - DEG / 2, by0 = mny - DEG / 2;
      const unsigned voff = (unsigned)(lane * NCH) * 4u;
      const char *sb = (const char *)(s.base + ((long long)by0 * s.es1 + (long long)bx0 * NCH));
      const long long step = s.es1 * 4;
      unsigned dst = lds_tile;
      const unsigned dstep = (unsigned)ibw * (TEX * 4u);
#pragma unroll 1
      for (int it = 0; it < ibh; it++) { eu4_dma_row(dst, voff, sb); sb += step; dst += dstep; }
    }
    // the weights, behind the DMA issue
    eu_f2 wx[order], wy[order];
    float wya[order], wyb[order];
    if constexpr (DEG >= 2) {
      eu_weights2<DEG>(s.wm, ty, wy);
      eu_weights2<DEG>(s.wm, tx, wx);
    }
#pragma unroll
    for (int i = 0; i < order; i++) {
      if constexpr (DEG >= 2) {
        wya[i] = wy[i].x; wyb[i] = wy[i].y;
        wxa[i] = wx[i].x; wxb[i] = wx[i].y;
      } else {
        wya[i] = wyb[i] = 0.0f;
        wxa[i] = wxb[i] = 0.0f;
      }
    }
    // lanes without a hit read the box origin
    const int oa = hit.x ? ((iya - mny) * ibw + (ixa - mnx)) * TEX : 0;
    const int ob = hit.y ? ((iyb - mny) * ibw + (ixb - mnx)) * TEX : 0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    eu_lptr lt = (eu_lptr)wtile;
    eu_accumulate1<NCH, DEG, TEX, int, eu_lptr>(lt + oa, ibw * TEX, wxa, wya, tx.x, ty.x, qa);
    eu_accumulate1<NCH, DEG, TEX, int, eu_lptr>(lt + ob, ibw * TEX, wxb, wyb, tx.y, ty.y, qb);
  } else {
#pragma unroll
    for (int c = 0; c < NCH; c++) { qa[c] = 0.0f; qb[c] = 0.0f; }
  }
  // environment::eval brighten (environment.h:1821-1842), zero on a miss; storer
  constexpr int ncol = (NCH == 2 || NCH == 4) ? NCH - 1 : NCH;
  const bool bright = s.brighten != 1.0f;
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    float a = qa[c], bb = qb[c];
    if (bright && c < ncol) { a = a * s.brighten; bb = bb * s.brighten; }
    qa[c] = hit.x ? a : 0.0f;
    qb[c] = hit.y ? bb : 0.0f;
  }
  if (va) eu_put<NCH>(orow, xa, qa);
  if (vb) eu_put<NCH>(orow, xb, qb);
}

// the staged kernel of cubemap and biatan6 sources: one 16x8 tile per wave, EU4_WAVES0 waves
// (neighbouring tiles of one tile row) per workgroup; they share nothing but the atanf table
template <int NCH, int DEG, int PRJ>
__global__ __launch_bounds__(64 * EU4_WAVES0, EU4_OCC0) void eu_render4s_kernel(const eu_render_params p, const eu4_plan w)
{
  __shared__ __attribute__((aligned(16))) float tile_all[EU4_WAVES0 * EU4_TEXELS * 4];
  __shared__ __attribute__((aligned(16))) float atab[768];   // EU_ATAN_TAB_FLOATS, rounded up to three DMA pieces
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float *const tile = tile_all + wave * (EU4_TEXELS * 4);
  if (PRJ != EU_CUBEMAP && wave == 0) {
    // the table comes from its copy in global memory by LDS-DMA: 3 instructions of 64 x 16
    // bytes cover its 2592 bytes (a workgroup of one wave would spend ~70 VALU instructions
    // computing it)
    static_assert(EU_ATAN_TAB_FLOATS * 4 <= 3 * 1024, "three pieces");
#pragma unroll
    for (int i = 0; i < 3; i++)
      __builtin_amdgcn_global_load_lds((eu4_gbl_void)(w.atab_g + i * 256 + lane * 4),
                                       (eu4_lds_void)(atab + i * 256), 16, 0, 0);
  }
  // XCD-aware tile order without a division: grid = (8 * tiles16, unit rows, rounds).
  // Workgroups are dispatched x fastest and dealt round-robin to the 8 XCDs, so
  // blockIdx.x & 7 is the XCD (up to a rotation); an XCD walks the tiles of its unit
  // (EU4_UNIT_ROWS tile rows) in raster order and gets every 8th unit of the frame.
  const int tile_x = (int)(blockIdx.x >> 3) * EU4_WAVES0 + wave;
  const int tile_y = ((int)blockIdx.z * 8 + (int)(blockIdx.x & 7)) * EU4_UNIT_ROWS + (int)blockIdx.y;
  if (tile_y >= p.tiles_y) return;                    // the whole workgroup
  if constexpr (EU4_WAVES0 > 1) {
    // wave 0's table has to be in LDS before the others use it
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (tile_x >= w.tiles16) return;
  eu4_tile<NCH, DEG, PRJ>(p, w, atab, tile, tile_y, tile_x * EU4_TW, lane);
}

// one 16x8 tile by direct gathers: (d+1)^2 taps from global memory, every scalar fallback of the
// coordinate arithmetic (the work-list kernel's tile)
// qrec: the wave's area for the pixel records of eu_quad_gather.h (degrees 2 and 3)
template <int NCH, int DEG, int PRJ>
__device__ __forceinline__ void eu4_direct_tile(const eu_render_params &p, const float *atab, float *qrec, int tile_y, int x0, int lane)
{
  const eu_src_dev &s = p.src;
  const int lx = lane & 7, ly = lane >> 3;
  const int y = p.row_begin + tile_y * EU4_TH + ly;
  const bool yin = y < p.row_end;
  const int yc = yin ? y : p.row_end - 1;
  const float *rt = p.row + (long long)eu_frame_row(yc, p.band_shift, p.band_count, p.band_index) * EU_ROW_FLOATS;
  const int xa = x0 + 2 * lx, xb = xa + 1;
  const bool va = yin && xa < p.width, vb = yin && xb < p.width;
  const int xac = xa < p.width ? xa : p.width - 1, xbc = xb < p.width ? xb : p.width - 1;
  eu_ray2 ry;
  {
    const float A0 = rt[0], A1 = rt[1], A2 = rt[2], B0 = rt[3], B1 = rt[4], B2 = rt[5];
    const eu_f2 c0 = { p.col[xac], p.col[xbc] };
    if (p.form == EU_FORM_BCA) {
      const float C0 = rt[6], C1 = rt[7], C2 = rt[8];
      const float *colB = p.col + p.width;
      const eu_f2 c1 = { colB[xac], colB[xbc] };
      ry.x = B0 * c0 + C0 * c1 + A0;
      ry.y = B1 * c0 + C1 * c1 + A1;
      ry.z = B2 * c0 + C2 * c1 + A2;
    } else {
      ry.x = B0 * c0 + A0;
      ry.y = B1 * c0 + A1;
      ry.z = B2 * c0 + A2;
    }
    if (p.norm_mode == EU_NORM_DIV) {
      eu_f2 sqn = ry.x * ry.x; sqn = sqn + ry.y * ry.y; sqn = sqn + ry.z * ry.z;
      const eu_f2 n = { sqrtf(sqn.x), sqrtf(sqn.y) };
      ry.x = ry.x / n; ry.y = ry.y / n; ry.z = ry.z / n;
    }
  }
  eu_f2 sx, sy;
  eu_i2 hit = eu_coord2<PRJ>(s, ry, sx, sy, atab);
  hit = hit & (eu_i2){ va ? -1 : 0, vb ? -1 : 0 };
  if constexpr (DEG >= 2) {
    // the windows' rows fetched by lane quads: records of the lane's two pixels, then 16 pixels - one tile row - per
    // step with four lanes each. The wave reads what it wrote itself: its LDS operations complete in order
    eu_qg_records<NCH, DEG>(s, sx, sy, hit, va, vb, qrec, lane);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int rows = min(EU4_TH, p.row_end - (p.row_begin + tile_y * EU4_TH));
    const int i = lane & 3, xq = x0 + (lane >> 2);
    float *orow = p.out + (long long)(tile_y * EU4_TH) * p.out_stride;
    // two steps per turn: both steps' loads are in flight before the first sum
    auto finish = [&](const eu_qg_taps<NCH, DEG> &w) {
      float px[NCH];
      eu_qg_sum<NCH, DEG>(s, w, px);
      if (i == DEG && (w.flags & EU_QG_VALID)) eu_put<NCH>(orow, xq, px);
      orow += p.out_stride;
    };
#pragma unroll 1
    for (int k = 0; k < rows; k += 2) {
      eu_qg_taps<NCH, DEG> wa, wb;
      const bool two = k + 1 < rows;
      eu_qg_fetch<NCH, DEG>(s, qrec, k * EU4_TW + (lane >> 2), i, wa);
      if (two) eu_qg_fetch<NCH, DEG>(s, qrec, (k + 1) * EU4_TW + (lane >> 2), i, wb);
      finish(wa);
      if (two) finish(wb);
    }
    __builtin_amdgcn_wave_barrier();
  } else {
    float pxa[NCH], pxb[NCH];
    eu_eval2<NCH, DEG>(s, sx, sy, hit, pxa, pxb);
    float *const orow = p.out + (long long)(yc - p.row_begin) * p.out_stride;
    if (va) eu_put<NCH>(orow, xa, pxa);
    if (vb) eu_put<NCH>(orow, xb, pxb);
  }
}

#include "eu_share_groups.h"
#include "eu_render5.h"

// ---------------------------------------------------------------------------
// pre-pass: the column table of one plan. Thread t fills columns 2t and 2t + 1 with the
// operations the staged kernel performs on the x coordinate (eu_coord2_ok for a lat/lon
// source, the x gate, split and weights), on the same float2 functions: same bits.
// ---------------------------------------------------------------------------
template <int DEG>
__global__ __launch_bounds__(256) void eu_colplan_kernel(const eu_render_params p, float *ct,
                                                         float A0, float A2, float B0, float B2)
{
  __shared__ __attribute__((aligned(16))) float atab[EU_ATAN_TAB_FLOATS];
  if (threadIdx.x < EU_ATAN_TAB_ENTRIES) eu_atan_tab_entry(threadIdx.x, atab + 8 * threadIdx.x);
  __syncthreads();
  constexpr int order = DEG + 1;
  const eu_src_dev &s = p.src;
  const int xa = 2 * (blockIdx.x * 256 + threadIdx.x), xb = xa + 1;
  if (xa >= p.width) return;
  const int xbc = xb < p.width ? xb : p.width - 1;
  const eu_f2 c0 = { p.col[xa], p.col[xbc] };
  const eu_f2 rx = B0 * c0 + A0, rz = B2 * c0 + A2;
  eu_i2 ok = { -1, -1 };
  const eu_f2 q2 = rx * rx + rz * rz;
  const eu_f2 qs = eu_sqrt2_ok(q2, ok);
  const eu_f2 lon = eu_atan2f_2_tab_ok(rx, rz, atab, 0, ok);
  eu_f2 i0 = { (float)((double)lon.x - s.tex_x0), (float)((double)lon.y - s.tex_x0) };
  if (s.cdiv_ok) i0 = eu_div2_const(i0, s.ext_w, s.rcp_ext_w);
  else i0 = i0 / s.ext_w;
  i0 = i0 * s.total_w; i0 = i0 - .5f;
  const eu_f2 sx = i0 - s.win_x_off;
  const eu_f2 gx = eu_gate2_ok(sx, s.gate0, s.lower0, s.upper0, ok);
  eu_f2 fx;
  if constexpr (DEG & 1) fx = (eu_f2){ floorf(gx.x), floorf(gx.y) };
  else fx = (eu_f2){ roundf(gx.x), roundf(gx.y) };
  const eu_f2 tx = gx - fx;
  eu_f2 wx[4];
#pragma unroll
  for (int i = 0; i < 4; i++) wx[i] = (eu_f2){ 0.0f, 0.0f };
  if constexpr (DEG >= 2) eu_weights2<DEG>(s.wm, tx, wx);
  float e[2][EU4_COL_FLOATS];
  e[0][0] = __int_as_float(ok.x ? (int)fx.x : INT_MIN);
  e[1][0] = __int_as_float(ok.y ? (int)fx.y : INT_MIN);
  e[0][1] = tx.x; e[1][1] = tx.y;
#pragma unroll
  for (int i = 0; i < 4; i++) { e[0][2 + i] = i < order ? wx[i].x : 0.0f; e[1][2 + i] = i < order ? wx[i].y : 0.0f; }
  e[0][6] = qs.x; e[1][6] = qs.y;
  e[0][7] = lon.x; e[1][7] = lon.y;
  float *o = ct + (size_t)xa * EU4_COL_FLOATS;
#pragma unroll
  for (int i = 0; i < EU4_COL_FLOATS; i++) o[i] = e[0][i];
  if (xb < p.width) {
#pragma unroll
    for (int i = 0; i < EU4_COL_FLOATS; i++) o[EU4_COL_FLOATS + i] = e[1][i];
  }
}

// ---------------------------------------------------------------------------
// the direct-gather kernel: the tiles of the work list, (d+1)^2 taps from global memory,
// every scalar fallback of the coordinate arithmetic. The lists it reads stay as they are
// (eu_hip_listed_tiles adds them up); the launch empties the OTHER set of counters, `wl_next`,
// for the pair behind it (eu_worklist.h): plain stores, nobody waits for anybody
// ---------------------------------------------------------------------------
template <int NCH, int DEG, int PRJ>
__global__ __launch_bounds__(256, 4) void eu_render4d_kernel(const eu_render_params p, const eu4_plan w, int *wl_next)
{
  __shared__ __attribute__((aligned(16))) float atab[EU_ATAN_TAB_FLOATS];
  if constexpr (PRJ != EU_CUBEMAP) {
    if (threadIdx.x < EU_ATAN_TAB_ENTRIES) eu_atan_tab_entry(threadIdx.x, atab + 8 * threadIdx.x);
  }
  for (int i = blockIdx.x * 256 + threadIdx.x; i < EU4_WL_COUNTERS; i += (int)gridDim.x * 256)
    __hip_atomic_store(wl_next + 16 * i, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // the pixel records of a wave's tile (eu_quad_gather.h): 6 KB per wave
  __shared__ __attribute__((aligned(16))) float qrec_all[DEG >= 2 ? EU4_WAVES * EU4_TW * EU4_TH * EU_QG_REC : 4];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // this wave's list: waves gid, gid + EU4_SHARDS, ... share list gid % EU4_SHARDS
  float *const qrec = qrec_all + (DEG >= 2 ? wave * (EU4_TW * EU4_TH * EU_QG_REC) : 0);
  const int gid = blockIdx.x * EU4_WAVES + wave;
  const int sh = gid & (EU4_SHARDS - 1);
  const int nwork = __builtin_amdgcn_readfirstlane(
    __hip_atomic_load(p.wl + EU4_WL_SHARD(sh), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  __syncthreads();
#pragma unroll 1
  for (int k = gid / EU4_SHARDS; k < nwork; k += (int)(gridDim.x * EU4_WAVES / EU4_SHARDS)) {
    const int id = __builtin_amdgcn_readfirstlane(p.wl[EU4_WL_ENTRIES + (size_t)k * EU4_SHARDS + sh]);
    const int tile_y = id / w.tiles16;
    const int x0 = (id - tile_y * w.tiles16) * EU4_TW;
    eu4_direct_tile<NCH, DEG, PRJ>(p, atab, qrec, tile_y, x0, lane);
  }
}

// follower tiles (eu_share_groups.h) of the plan about to be launched / of the last launch of eu_render5_kernel's FAST form
static long long eu4_followers_plan = 0, eu4_followers_last = 0;
extern "C" unsigned long long eu_hip_share_follower_tiles(void) { return (unsigned long long)eu4_followers_last; }
// ... and the same for the second loop's groups (eu_polar_groups.h): counted where the launch read the box table
static long long eu4_polar_plan = 0, eu4_polar_last = 0;
extern "C" unsigned long long eu_hip_polar_follower_tiles(void) { return (unsigned long long)eu4_polar_last; }
// whether the last launch of eu_render5_kernel's FAST form read a box table (1, also for one of zero tiles) or not (0),
// and the tiles that table holds
static int eu4_boxtab_last = 0;
static long long eu4_boxtab_tiles_last = 0;
extern "C" int eu_hip_boxtab_used(void) { return eu4_boxtab_last; }
extern "C" unsigned long long eu_hip_boxtab_tiles(void) { return (unsigned long long)eu4_boxtab_tiles_last; }

#ifndef EU4_DIRECT_WGS
#define EU4_DIRECT_WGS 2048
#endif

template <int NCH, int DEG, int PRJ>
static int launch4_ndp(const eu_render_params &p, const eu4_plan &w, int *wl_next, hipStream_t st)
{
  // lat/lon sources: the persistent staged kernel (headline 1.13 vs 1.22 ms for the launch-level hybrid of the
  // direct-gather kernels); cubemap / biatan6 sources: one tile per workgroup (config 3 1.00 vs 1.22 ms)
  if constexpr (PRJ == EU_SPHERICAL) {
    // as many workgroups as are resident at once (a persistent kernel must not queue a second round)
    static const int cus = [] {
      int dev = 0, n = 0;
      if (hipGetDevice(&dev) != hipSuccess) return 0;
      if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
      return n;
    }();
    const bool fast = eu_staged_fast_profile(p);
    // (eu5_tile_bt stores through 32-bit buffer offsets: eight rows of the output below 2^31 bytes)
    const bool bt = fast && w.boxtab != nullptr && p.out_stride < (1ll << 25);
    int per_cu = 0;
    if (bt) {
      static const int occ = [] { int n = 0; return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, eu_render5_kernel<NCH, DEG, PRJ, true, true>, 64 * EU5_WAVES, 0) == hipSuccess ? n : 0; }();
      per_cu = occ;
    } else if (fast) {
      static const int occ = [] { int n = 0; return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, eu_render5_kernel<NCH, DEG, PRJ, true>, 64 * EU5_WAVES, 0) == hipSuccess ? n : 0; }();
      per_cu = occ;
    } else {
      static const int occ = [] { int n = 0; return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, eu_render5_kernel<NCH, DEG, PRJ, false>, 64 * EU5_WAVES, 0) == hipSuccess ? n : 0; }();
      per_cu = occ;
    }
    const int wgs = (cus / 8) * 8 * per_cu;
    if (wgs <= 0) return -1;
    if (fast) eu4_followers_last = eu4_followers_plan;
    eu4_boxtab_last = bt;
    if (bt) eu4_polar_last = eu4_polar_plan;
    if (bt) hipLaunchKernelGGL((eu_render5_kernel<NCH, DEG, PRJ, true, true>), dim3((unsigned)wgs), dim3(64 * EU5_WAVES), 0, st, p, w);
    else if (fast) hipLaunchKernelGGL((eu_render5_kernel<NCH, DEG, PRJ, true>), dim3((unsigned)wgs), dim3(64 * EU5_WAVES), 0, st, p, w);
    else hipLaunchKernelGGL((eu_render5_kernel<NCH, DEG, PRJ, false>), dim3((unsigned)wgs), dim3(64 * EU5_WAVES), 0, st, p, w);
  } else {
    const int units = (p.tiles_y + EU4_UNIT_ROWS - 1) / EU4_UNIT_ROWS;
    dim3 grid((unsigned)(8 * ((w.tiles16 + EU4_WAVES0 - 1) / EU4_WAVES0)), (unsigned)EU4_UNIT_ROWS, (unsigned)((units + 7) / 8));
    hipLaunchKernelGGL((eu_render4s_kernel<NCH, DEG, PRJ>), grid, dim3(64 * EU4_WAVES0), 0, st, p, w);
  }
  if (hipGetLastError() != hipSuccess) return -1;
  hipLaunchKernelGGL((eu_render4d_kernel<NCH, DEG, PRJ>), dim3(EU4_DIRECT_WGS), dim3(256), 0, st, p, w, wl_next);
  if (hipGetLastError() != hipSuccess) {
    // the staged kernel has filled this set's lists and nobody has emptied the other's: the next job must not append to
    // either (the caller does not advance the parity, so it is this set again)
    (void)hipMemsetAsync(std::min(p.wl, wl_next), 0, eu_render4_worklist_clear_ints() * sizeof(int), st);
    return -1;
  }
  return 0;
}

template <int NCH, int DEG>
static int launch4_nd(const eu_render_params &p, const eu4_plan &w, int *wl_next, hipStream_t st)
{
  switch (p.src.prj) {
    case EU_SPHERICAL: return launch4_ndp<NCH, DEG, EU_SPHERICAL>(p, w, wl_next, st);
    case EU_CUBEMAP: return launch4_ndp<NCH, DEG, EU_CUBEMAP>(p, w, wl_next, st);
    case EU_BIATAN6: return launch4_ndp<NCH, DEG, EU_BIATAN6>(p, w, wl_next, st);
  }
  return -2;
}

template <int NCH>
static int launch4_n(const eu_render_params &p, const eu4_plan &w, int *wl_next, hipStream_t st)
{
  switch (p.src.degree) {
    case 1: return launch4_nd<NCH, 1>(p, w, wl_next, st);
    case 2: return launch4_nd<NCH, 2>(p, w, wl_next, st);
    case 3: return launch4_nd<NCH, 3>(p, w, wl_next, st);
  }
  return -2;
}

// ---------------------------------------------------------------------------
// host: the column plans of a launch. A tile row can take the x half of its coordinates
// from a per-column table when the job is 'ray = B * c0 + A' without normalisation on a
// lat/lon source and the x and z components of A and B are the same for its 8 rows (then
// rx, rz and everything derived from them alone are functions of the column). Tile rows
// with the same four constants share a table.
// ---------------------------------------------------------------------------
static_assert(EU_STAGED_TILE_ROWS == EU4_TH && EU_STAGED_MAX_TILES_Y == 65535 * 8 * EU4_UNIT_ROWS, "eu_select.h: eu_staged_covers");
namespace {
struct plan_cache {
  std::vector<unsigned char> key;
  eu_dev_buf<int> tileplan, l2_rows, l1_ent, xtab, boxtab, l2p_ent;
  bool has_boxtab = false;   // the second loop's box table exists (it may hold no tile)
  long long boxtab_tiles = 0;
  eu_dev_buf<float> coltab;
  float *atab = nullptr;
  int planned_rows = 0;      // tile rows with a column plan
  int l2_off[9] = {};
  int l1_off[9] = {};
  int l1_ecols = 1;
  long long follower_tiles = 0;
  int l2p_off[9] = {};
  int l2p_ecols = 1, l2p_bcols = 2;
  long long polar_follower_tiles = 0;
} g4s[EU_MAX_SLOTS];
// one cache per device slot (eu_api_devices.hip: eu_hip_init_devices)
#define g4 (g4s[eu_current_slot()])

bool ensure_atab()
{
  if (g4.atab) return true;
  std::vector<float> tab(768, 0.0f);
  for (int i = 0; i < EU_ATAN_TAB_ENTRIES; i++) eu_atan_tab_entry(i, tab.data() + 8 * i);
  if (hipMalloc((void **)&g4.atab, tab.size() * sizeof(float)) != hipSuccess) return false;
  return hipMemcpy(g4.atab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
}

template <int DEG>
void launch_colplan(const eu_render_params &p, float *ct, const float *k, hipStream_t st)
{
  hipLaunchKernelGGL((eu_colplan_kernel<DEG>), dim3((unsigned)((p.width + 511) / 512)), dim3(256), 0, st, p, ct,
                     k[0], k[1], k[2], k[3]);
}

// everything the cached plans depend on
std::vector<unsigned char> eu4_plan_key(const eu_render_params &p, unsigned long long plan_gen, const eu_switches &sw)
{
  std::vector<unsigned char> key(sizeof(unsigned long long) + sizeof(eu_src_dev) + 12 * sizeof(int));
  unsigned char *q = key.data();
  memcpy(q, &plan_gen, sizeof plan_gen); q += sizeof plan_gen;
  eu_src_dev sd = p.src; sd.base = nullptr;
  memcpy(q, &sd, sizeof sd); q += sizeof sd;
  const int v[12] = { p.width, p.row_begin, p.row_end, p.band_shift, p.band_count, p.band_index, p.form, p.norm_mode, sw.share,
                      sw.boxtab, sw.boxtab_max_kb, sw.polar_share };
  memcpy(q, v, sizeof v);
  return key;
}

bool upload(eu_dev_buf<int> &buf, const std::vector<int> &v, size_t spare)
{
  if (buf.reserve(v.size() + spare) != hipSuccess) return false;
  return v.empty() || hipMemcpy(buf.p, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
}

template <int DEG>
void launch_boxplan(const eu_render_params &p, const float *atab_g, const int *l2_rows, int tiles16, int ntiles, int *tab, hipStream_t st)
{
  hipLaunchKernelGGL((eu5_boxplan_kernel<DEG>), dim3((unsigned)((ntiles + 3) / 4)), dim3(256), 0, st, p, atab_g, l2_rows, tiles16,
                     ntiles, tab);
}

// the plans of a lat/lon job into the slot's cache: the tile rows' plan ids, the second loop's rows, the column
// tables (one kernel launch per plan) and, from their bits, the first loop's entries (eu_share_groups.h)
int eu4_build_plans(const eu_render_params &p, int tiles16, const eu_switches &sw, const float *h_row,
                    size_t h_row_floats, const float *h_col, size_t h_col_floats, hipStream_t st)
{
  static_assert(EU_TILE_ROWS == EU4_TH && EU_PLAN_MAX == EU4_MAX_PLANS && EU_SECOND_LOOP_UNIT_ROWS == EU5_UNIT_ROWS,
                "eu_polar_groups.h: what a host program takes for the launcher's constants");
  std::vector<int> tp((size_t)p.tiles_y, -1);
  std::vector<float> plans;          // 4 floats per plan: A0, A2, B0, B2
  const bool can = p.form == EU_FORM_BA && p.norm_mode == EU_NORM_NONE && h_row;
  if (can && sw.colplan)
    eu_tile_row_plans(h_row, h_row_floats, EU_ROW_FLOATS, p.row_begin, p.row_end,
                      [&](int y) { return eu_frame_row(y, p.band_shift, p.band_count, p.band_index); }, tp, plans);
  const int nplans = (int)(plans.size() / 4);
  // the previous launch pair may still read the old plans, on this stream or on another: `st` is ordered behind it
  // (eu_launch.h), so when `st` is through, that pair is
  if (hipStreamSynchronize(st) != hipSuccess) return -1;
  if (g4.tileplan.reserve(tp.size()) != hipSuccess) return -1;
  if (g4.coltab.reserve(std::max<size_t>(1, nplans) * (size_t)p.width * EU4_COL_FLOATS) != hipSuccess) return -1;
  if (hipMemcpy(g4.tileplan.p, tp.data(), tp.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return -1;
  g4.planned_rows = 0;
  for (int v : tp) g4.planned_rows += v >= 0;
  auto paired = [&](int m) { return 2 * m + 1 < p.tiles_y && tp[(size_t)2 * m] >= 0 && tp[(size_t)2 * m] == tp[(size_t)2 * m + 1]; };
  {
    // the second loop's rows per XCD: units of EU5_UNIT_ROWS tile rows dealt round-robin, as in the first loop
    std::vector<int> all;
    eu_second_loop_rows(tp, EU5_UNIT_ROWS, all, g4.l2_off);
    if (!upload(g4.l2_rows, all, 1)) return -1;
    // ... and who may follow whom there, from the bits of the tables the kernel reads (eu_polar_groups.h): the list
    // of the loop's form that reads the box table
    eu_polar_input pin;
    pin.width = p.width; pin.tiles16 = tiles16; pin.row_begin = p.row_begin; pin.row_end = p.row_end;
    pin.band_mode = p.band_count > 1;
    pin.nrows = (int)all.size(); pin.rows = all.data();
    pin.h_row = h_row; pin.h_row_floats = h_row_floats; pin.row_floats = EU_ROW_FLOATS;
    pin.h_col = h_col; pin.h_col_floats = h_col_floats;
    pin.mode = can ? sw.polar_share : 0; pin.unit_rows = EU5_UNIT_ROWS;
    eu_polar_result pr;
    eu_polar_build(pin, pr);
    if (!upload(g4.l2p_ent, pr.entries, EU_POLAR_ENTRY_INTS)) return -1;
    for (int x = 0; x < 9; x++) g4.l2p_off[x] = pr.off[x];
    g4.l2p_ecols = pr.ecols; g4.l2p_bcols = pr.bcols;
    g4.polar_follower_tiles = pr.follower_tiles;
  }
  // the second loop's box table (eu_render5.h), for the FAST form - the only reader: one wave per tile of those rows,
  // on the stream the plans are built on. A table beyond sw.boxtab_max_kb is not built: the job takes the loop that
  // reduces its boxes per frame.
  g4.has_boxtab = false; g4.boxtab_tiles = 0;
  if (sw.boxtab && eu_staged_fast_profile(p)) {
    const long long ntiles = (long long)g4.l2_off[8] * tiles16;
    const long long bytes = ntiles * (EU5_BT_RECS * 16);
    if (bytes <= (long long)sw.boxtab_max_kb * 1024) {
      if (g4.boxtab.reserve((size_t)std::max<long long>(1, ntiles) * (EU5_BT_RECS * 4)) != hipSuccess) return -1;
      if (ntiles > 0) {
        switch (p.src.degree) {
          case 1: launch_boxplan<1>(p, g4.atab, g4.l2_rows.p, tiles16, (int)ntiles, g4.boxtab.p, st); break;
          case 2: launch_boxplan<2>(p, g4.atab, g4.l2_rows.p, tiles16, (int)ntiles, g4.boxtab.p, st); break;
          default: launch_boxplan<3>(p, g4.atab, g4.l2_rows.p, tiles16, (int)ntiles, g4.boxtab.p, st); break;
        }
        if (hipGetLastError() != hipSuccess) return -1;
      }
      g4.has_boxtab = true; g4.boxtab_tiles = ntiles;
    }
  }
  for (int j = 0; j < nplans; j++) {
    float *ct = g4.coltab.p + j * (size_t)p.width * EU4_COL_FLOATS;
    switch (p.src.degree) {
      case 1: launch_colplan<1>(p, ct, &plans[4 * j], st); break;
      case 2: launch_colplan<2>(p, ct, &plans[4 * j], st); break;
      default: launch_colplan<3>(p, ct, &plans[4 * j], st); break;
    }
    if (hipGetLastError() != hipSuccess) return -1;
  }
  // the first loop's entries per XCD and the boxes' x extents, from the bits of the tables the kernel reads
  // (eu_share_groups.h): the column plans come back to the host once per plan build
  std::vector<float> h_ct((size_t)nplans * p.width * EU4_COL_FLOATS);
  if (nplans) {
    if (hipStreamSynchronize(st) != hipSuccess) return -1;
    if (hipMemcpy(h_ct.data(), g4.coltab.p, h_ct.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  }
  std::vector<int> cm, cp;
  for (int m = 0; 2 * m + 1 < p.tiles_y; m++)
    if (paired(m)) { cm.push_back(m); cp.push_back(tp[(size_t)2 * m]); }
  eu_share_input in;
  in.width = p.width; in.tiles16 = tiles16; in.row_begin = p.row_begin; in.row_end = p.row_end;
  in.band_mode = p.band_count > 1;
  in.ncand = (int)cm.size(); in.cand_m = cm.data(); in.cand_plan = cp.data();
  in.h_row = h_row; in.h_row_floats = h_row_floats; in.row_floats = EU_ROW_FLOATS;
  in.coltab = nplans ? h_ct.data() : nullptr; in.col_floats = EU4_COL_FLOATS; in.nplans = nplans;
  in.mode = sw.share; in.unit_drows = EU5_UNIT_ROWS / 2;
  eu_share_result gr;
  eu_share_build(in, gr);
  if (!upload(g4.l1_ent, gr.entries, 2)) return -1;
  if (g4.xtab.reserve(gr.xtab.size()) != hipSuccess) return -1;
  if (hipMemcpy(g4.xtab.p, gr.xtab.data(), gr.xtab.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return -1;
  for (int x = 0; x < 9; x++) g4.l1_off[x] = gr.off[x];
  g4.l1_ecols = gr.ecols;
  g4.follower_tiles = gr.follower_tiles;
  return 0;
}

// the launch's view of the slot's cache (w.tiles16 and w.atab_g are set)
void eu4_fill_plan(eu4_plan &w)
{
  w.tileplan = g4.tileplan.p;
  w.coltab = g4.coltab.p;
  w.l2_rows = g4.l2_rows.p;
  for (int x = 0; x < 9; x++) w.l2_off[x] = g4.l2_off[x];
  w.l2_half = (w.tiles16 + 1) / 2;
  w.l2_magic = (1ull << 40) / (unsigned long long)w.l2_half + 1;
  w.l1_ent = g4.l1_ent.p;
  for (int x = 0; x < 9; x++) w.l1_off[x] = g4.l1_off[x];
  w.l1_ecols = g4.l1_ecols;
  w.l1_magic = (1ull << 40) / (unsigned long long)w.l1_ecols + 1;
  w.xtab = g4.xtab.p;
  w.boxtab = g4.has_boxtab ? g4.boxtab.p : nullptr;
  w.l2p_ent = g4.l2p_ent.p;
  for (int x = 0; x < 9; x++) w.l2p_off[x] = g4.l2p_off[x];
  w.l2p_ecols = g4.l2p_ecols; w.l2p_bcols = g4.l2p_bcols;
  w.l2p_bpe = std::max(1, (w.l2p_ecols + w.l2p_bcols - 1) / w.l2p_bcols);
  w.l2p_magic = (1ull << 40) / (unsigned long long)w.l2p_bpe + 1;
}

int launch4(const eu_render_params &p, const eu4_plan &w, int *wl_next, hipStream_t st)
{
  switch (p.nch) {
    case 3: return launch4_n<3>(p, w, wl_next, st);
    case 4: return launch4_n<4>(p, w, wl_next, st);
  }
  return -2;
}

#ifdef EU5_STAMPS
// diagnostic build: stamps of every tile, averaged per pass count / plan kind after the launch
int launch4_stamped(const eu_render_params &p, eu4_plan &w, int *wl_next, hipStream_t st)
{
  static unsigned long long *d_st = nullptr; static size_t st_cap = 0; static int dumps = 0;
  const size_t ntile_st = (size_t)w.tiles16 * p.tiles_y * 8;
  const size_t nst = ntile_st + 8192 * 4;      // + per-wave totals (eu_render5_kernel)
  if (st_cap < nst) { if (d_st) (void)hipFree(d_st); if (hipMalloc((void **)&d_st, nst * 8) != hipSuccess) return -1; st_cap = nst; }
  (void)hipMemsetAsync(d_st, 0, nst * 8, st);
  w.stamps = d_st;
  const int rc_ = launch4(p, w, wl_next, st);
  if (rc_ == 0 && dumps < 2 && nst >= 8 * 4096) {
    dumps++;
    std::vector<unsigned long long> h(nst);
    (void)hipStreamSynchronize(st);
    (void)hipMemcpy(h.data(), d_st, nst * 8, hipMemcpyDeviceToHost);
    double acc[32][8] = {}; size_t cnt[32] = {};
    for (size_t t = 0; t < ntile_st / 8; t++) {
      const unsigned long long *q = &h[t * 8];
      if (!q[0] || !q[7]) continue;
      const int cls = (int)(q[1] & 31);
      cnt[cls]++;
      acc[cls][0] += (double)(q[2] - q[0]); acc[cls][1] += (double)(q[3] - q[2]);
      if (q[4]) { acc[cls][2] += (double)(q[4] - q[3]); acc[cls][3] += (double)(q[5] - q[4]); acc[cls][4] += (double)(q[6] - q[5]); }
      acc[cls][5] += (double)(q[7] - q[6]); acc[cls][6] += (double)(q[7] - q[0]);
    }
    {
      double mn = 1e30, mx = 0, sum = 0, l1 = 0, first = 1e30, last = 0; size_t nw = 0;
      for (size_t k = 0; k < 8192; k++) {
        const unsigned long long *q = &h[ntile_st + k * 4];
        if (!q[3]) continue;
        const double d = (double)(q[2] - q[0]);
        mn = std::min(mn, d); mx = std::max(mx, d); sum += d; l1 += (double)(q[1] - q[0]); nw++;
        first = std::min(first, (double)q[0]); last = std::max(last, (double)q[2]);
      }
      if (nw) fprintf(stderr, "eu5 waves: %zu, cycles per wave min %.0f avg %.0f max %.0f, first loop avg %.0f, first start .. last end %.0f\n",
                      nw, mn, sum / nw, mx, l1 / nw, last - first);
    }
    for (int c = 0; c < 32; c++) if (cnt[c])
      fprintf(stderr, "eu5 stamps: hoist %d npass %2d tiles %8zu | coords %7.0f box %6.0f dma-issue+weights %6.0f dma-wait %6.0f taps(all passes) %6.0f store %5.0f | tile %7.0f (100 MHz ticks? s_memtime)\n",
              c >> 4, (c & 15) - 1, cnt[c], acc[c][0] / cnt[c], acc[c][1] / cnt[c], acc[c][2] / cnt[c], acc[c][3] / cnt[c], acc[c][4] / cnt[c], acc[c][5] / cnt[c], acc[c][6] / cnt[c]);
  }
  return rc_;
}
#endif
}  // namespace

extern "C" int eu_launch_render4(const eu_render_params *pp, int *wl_next, const eu_switches *sw, const float *h_row, size_t h_row_floats,
                                 const float *h_col, size_t h_col_floats, unsigned long long plan_gen, void *stream, int *launches)
{
  eu_render_params p = *pp;
  eu4_followers_last = 0; eu4_polar_last = 0;
  eu4_boxtab_last = 0; eu4_boxtab_tiles_last = 0;
  *launches = 2;
  if (!eu_staged_covers(p) || !p.wl || !wl_next) return -2;
  p.tiles_y = (p.row_end - p.row_begin + EU4_TH - 1) / EU4_TH;
  eu4_plan w;
  w.tiles16 = (p.width + EU4_TW - 1) / EU4_TW;
  if (w.tiles16 <= 0 || p.tiles_y <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (!ensure_atab()) return -1;
  w.atab_g = g4.atab;
  // the plans are cached while nothing they depend on changes (cubemap / biatan6 sources never read the
  // tile plan: no plans, no upload, no synchronisation for them)
  if (p.src.prj == EU_SPHERICAL) {
    std::vector<unsigned char> key = eu4_plan_key(p, plan_gen, *sw);
    if (key != g4.key) {
      if (eu4_build_plans(p, w.tiles16, *sw, h_row, h_row_floats, h_col, h_col_floats, st)) return -1;
      g4.key.swap(key);
    }
    if (sw->r4 != 1 && !eu_staged_worth(p.src.degree, g4.planned_rows, p.tiles_y)) { *launches = 0; return 0; }
  }
  eu4_fill_plan(w);
  eu4_followers_plan = g4.follower_tiles;
  eu4_polar_plan = g4.polar_follower_tiles;
  eu4_boxtab_tiles_last = w.boxtab ? g4.boxtab_tiles : 0;
#ifdef EU5_STAMPS
  return launch4_stamped(p, w, wl_next, st);
#else
  return launch4(p, w, wl_next, st);
#endif
}
