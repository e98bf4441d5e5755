// Packed render kernel: TWO output pixels per lane (x and x+64 of one row),
// all coordinate arithmetic on float2 so that it issues as v_pk_* instructions
// (see eu_math2.h), divisions/square roots by the range-checked FMA sequences,
// b-spline weights with the structural zeros of the weight matrix skipped.
// Same operations, same order, same bits as eu_render_kernel - only how they
// are issued changes. Covers the jobs without twining whose source is a
// lat/lon image; everything else stays on eu_render_kernel.
#include "eu_packed_dev.h"
#include "eu_launch.h"

#define EU2_TILE_W 128   // pixels of one row per wave and pass (2 per lane)
#define EU2_TILE_H 4   // default waves (rows) per workgroup
#define EU2_UNIT_ROWS 8  // tile rows per XCD unit

// ---------------------------------------------------------------------------
// the kernel
// ---------------------------------------------------------------------------

// EU2_WAVES (build-time experiment): cap the registers for that many waves per SIMD
#ifdef EU2_WAVES
#define EU2_OCC __attribute__((amdgpu_waves_per_eu(EU2_WAVES, EU2_WAVES)))
#else
#define EU2_OCC
#endif

template <int NCH, int DEG, int PRJ, bool TWINE>
__global__ __launch_bounds__(256) EU2_OCC void eu_render2_kernel(const eu_render_params p)
{
  // atanf range table in LDS (eu_math2.h): filled before any thread leaves
  __shared__ __attribute__((aligned(16))) float atab[EU_ATAN_TAB_FLOATS];
  if constexpr (PRJ != EU_CUBEMAP) {
    if (threadIdx.x < EU_ATAN_TAB_ENTRIES) eu_atan_tab_entry(threadIdx.x, atab + 8 * threadIdx.x);
    __syncthreads();
  }
  const int b = eu_xcd_tile(blockIdx.x, p.tiles_x, p.tiles_y, p.unit_rows);
  if (b < 0) return;
  const int tile_y = b / p.tiles_x, tile_x = b - tile_y * p.tiles_x;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int y = p.row_begin + tile_y * EU2_TILE_H + wave;
  if (y >= p.row_end) return;
  const int xa = tile_x * EU2_TILE_W + lane, xb = xa + 64;
  if (xa >= p.width) return;
  const bool vb = xb < p.width;
  const int xbc = vb ? xb : xa;

  eu_cptr rowt = (eu_cptr)(p.row + (long long)eu_frame_row(y, p.band_shift, p.band_count, p.band_index) * EU_ROW_FLOATS);
  const eu_ray2 r00 = eu_rays2(p.form, p.norm_mode, rowt, p.col, p.col + p.width, xa, xbc);

  float pxa[NCH], pxb[NCH];
  eu_pixels2<NCH, DEG, PRJ, TWINE>(p, r00,
      [&](eu_ray2 &r10, eu_ray2 &r01) __attribute__((always_inline)) {
        r10 = eu_rays2(p.form, p.norm_mode, rowt, p.col + 2 * p.width, p.col + 3 * p.width, xa, xbc);
        r01 = eu_rays2(p.form, p.norm_mode, rowt + EU_ROW_VARIANT, p.col, p.col + p.width, xa, xbc);
      },
      [](eu_i2 &, eu_f2, eu_f2) __attribute__((always_inline)) {}, atab, pxa, pxb);

  float *o = p.out + (long long)(y - p.row_begin) * p.out_stride;
  eu_put<NCH>(o, xa, pxa);
  if (vb) eu_put<NCH>(o, xb, pxb);
}

// ---------------------------------------------------------------------------
// 32x16 output tiles (no twining), still two pixels per lane (rows y and y+8 of one
// column): the hybrid's tile layout (eu_render_params::layout == 2). The four lanes the
// memory pipe serves together (a quad) form a 2x2 pixel block, which touches about the
// same number of cache lines for every orientation of the mapping (polar cube faces,
// rotated targets); a wave covers 32x2 pixels.
// ---------------------------------------------------------------------------

#define EU3_TW 32
#define EU3_TH 16

template <int NCH, int DEG, int PRJ>
__global__ __launch_bounds__(256, 4) void eu_render3_kernel(const eu_render_params p)
{
  __shared__ __attribute__((aligned(16))) float atab[EU_ATAN_TAB_FLOATS];
  if constexpr (PRJ != EU_CUBEMAP) {
    if (threadIdx.x < EU_ATAN_TAB_ENTRIES) eu_atan_tab_entry(threadIdx.x, atab + 8 * threadIdx.x);
  }
  const int b = eu_xcd_tile(blockIdx.x, p.tiles_x, p.tiles_y, p.unit_rows);
  if (b < 0) return;                                   // whole workgroup
  __syncthreads();
  const int tile_y = b / p.tiles_x, tile_x = b - tile_y * p.tiles_x;
  const int l = threadIdx.x & 63;
  const int lx = ((l >> 2) << 1) | (l & 1);
  const int ly = ((threadIdx.x >> 6) << 1) | ((l >> 1) & 1);
  const int x = tile_x * EU3_TW + lx;
  const int ya = p.row_begin + tile_y * EU3_TH + ly, yb = ya + 8;
  const bool la = x < p.width && ya < p.row_end, lb = x < p.width && yb < p.row_end;
  const int xc = x < p.width ? x : p.width - 1;
  const int yac = ya < p.row_end ? ya : p.row_end - 1, ybc = yb < p.row_end ? yb : p.row_end - 1;
  const eu_src_dev &s = p.src;

  // rays: the two pixels share the column value and differ in the row constants
  eu_ray2 r;
  {
    const float *ra = p.row + (long long)eu_frame_row(yac, p.band_shift, p.band_count, p.band_index) * EU_ROW_FLOATS;
    const float *rb = p.row + (long long)eu_frame_row(ybc, p.band_shift, p.band_count, p.band_index) * EU_ROW_FLOATS;
    const float c0 = p.col[xc];
    const eu_f2 A0 = { ra[0], rb[0] }, A1 = { ra[1], rb[1] }, A2 = { ra[2], rb[2] };
    const eu_f2 B0 = { ra[3], rb[3] }, B1 = { ra[4], rb[4] }, B2 = { ra[5], rb[5] };
    if (p.form == EU_FORM_BCA) {
      const float c1 = p.col[p.width + xc];
      const eu_f2 C0 = { ra[6], rb[6] }, C1 = { ra[7], rb[7] }, C2 = { ra[8], rb[8] };
      r.x = B0 * c0 + C0 * c1 + A0;
      r.y = B1 * c0 + C1 * c1 + A1;
      r.z = B2 * c0 + C2 * c1 + A2;
    } else {
      r.x = B0 * c0 + A0;
      r.y = B1 * c0 + A1;
      r.z = B2 * c0 + A2;
    }
  }
  eu_f2 sx, sy;
  eu_i2 hit = eu_coord2<PRJ>(s, r, sx, sy, atab);
  hit = hit & (eu_i2){ la ? -1 : 0, lb ? -1 : 0 };

  // gate + split
  eu_f2 gx = eu_gate2(sx, s.gate0, s.lower0, s.upper0);
  eu_f2 gy = eu_gate2(sy, s.gate1, s.lower1, s.upper1);
  eu_f2 fx, fy;
  if constexpr (DEG & 1) {
    fx = (eu_f2){ floorf(gx.x), floorf(gx.y) }; fy = (eu_f2){ floorf(gy.x), floorf(gy.y) };
  } else {
    fx = (eu_f2){ roundf(gx.x), roundf(gx.y) }; fy = (eu_f2){ roundf(gy.x), roundf(gy.y) };
  }
  const eu_f2 tx = gx - fx, ty = gy - fy;
  // lanes without a hit (misses, pixels outside the frame) use the window at
  // the core origin: inside every container, framed or not
  const int ixa = hit.x ? (int)fx.x : DEG / 2, iya = hit.x ? (int)fy.x : DEG / 2;
  const int ixb = hit.y ? (int)fx.y : DEG / 2, iyb = hit.y ? (int)fy.y : DEG / 2;

  constexpr int order = DEG + 1;
  eu_f2 wx[order], wy[order];
  if constexpr (DEG >= 2) {
    eu_weights2<DEG>(s.wm, tx, wx);
    eu_weights2<DEG>(s.wm, ty, wy);
  }
  float wxa[order], wxb[order], wya[order], wyb[order];
#pragma unroll
  for (int i = 0; i < order; i++) {
    if constexpr (DEG >= 2) { wxa[i] = wx[i].x; wxb[i] = wx[i].y; wya[i] = wy[i].x; wyb[i] = wy[i].y; }
    else { wxa[i] = wxb[i] = wya[i] = wyb[i] = 0.0f; }
  }

  float pxa[NCH], pxb[NCH];
  const float *pa = s.base + (long long)(ixa - DEG / 2) * NCH + (long long)(iya - DEG / 2) * s.es1;
  const float *pb = s.base + (long long)(ixb - DEG / 2) * NCH + (long long)(iyb - DEG / 2) * s.es1;
  eu_accumulate1<NCH, DEG>(pa, s.es1, wxa, wya, tx.x, ty.x, pxa);
  eu_accumulate1<NCH, DEG>(pb, s.es1, wxb, wyb, tx.y, ty.y, pxb);
  constexpr int ncol = (NCH == 2 || NCH == 4) ? NCH - 1 : NCH;
  const bool bright = s.brighten != 1.0f;
  if (la) {
    float *o = p.out + (long long)(ya - p.row_begin) * p.out_stride + (long long)x * NCH;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      float v = pxa[c];
      if (bright && c < ncol) v = v * s.brighten;
      o[c] = hit.x ? v : 0.0f;
    }
  }
  if (lb) {
    float *o = p.out + (long long)(yb - p.row_begin) * p.out_stride + (long long)x * NCH;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      float v = pxb[c];
      if (bright && c < ncol) v = v * s.brighten;
      o[c] = hit.y ? v : 0.0f;
    }
  }
}


template <int NCH, int DEG, int PRJ>
static int launch2_ndp(const eu_render_params &p, hipStream_t st)
{
  if (p.layout == 2 && !p.twine && p.norm_mode == EU_NORM_NONE) {
    eu_render_params q = p;
    q.tiles_x = (p.width + EU3_TW - 1) / EU3_TW;
    q.tiles_y = (p.row_end - p.row_begin + EU3_TH - 1) / EU3_TH;
    q.unit_rows = 2;
    dim3 grid3((unsigned)eu_xcd_grid(q.tiles_x, q.tiles_y, q.unit_rows)), block3(256);
    hipLaunchKernelGGL((eu_render3_kernel<NCH, DEG, PRJ>), grid3, block3, 0, st, q);
    return hipGetLastError() == hipSuccess ? 0 : -1;
  }
  dim3 grid((unsigned)eu_xcd_grid(p.tiles_x, p.tiles_y, p.unit_rows)), block(256);
  if (p.twine) hipLaunchKernelGGL((eu_render2_kernel<NCH, DEG, PRJ, true>), grid, block, 0, st, p);
  else hipLaunchKernelGGL((eu_render2_kernel<NCH, DEG, PRJ, false>), grid, block, 0, st, p);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int NCH, int DEG>
static int launch2_nd(const eu_render_params &p, hipStream_t st)
{
  switch (p.src.prj) {
    case EU_SPHERICAL: return launch2_ndp<NCH, DEG, EU_SPHERICAL>(p, st);
    case EU_CUBEMAP: return launch2_ndp<NCH, DEG, EU_CUBEMAP>(p, st);
    case EU_BIATAN6: return launch2_ndp<NCH, DEG, EU_BIATAN6>(p, st);
  }
  return -2;
}

template <int NCH>
static int launch2_n(const eu_render_params &p, hipStream_t st)
{
  switch (p.src.degree) {
    case 1: return launch2_nd<NCH, 1>(p, st);
    case 2: return launch2_nd<NCH, 2>(p, st);
    case 3: return launch2_nd<NCH, 3>(p, st);
  }
  return -2;
}

extern "C" int eu_launch_render2(const eu_render_params *pp, const eu_switches *sw, void *stream)
{
  eu_render_params p = *pp;
  if (!eu_packed_covers(p)) return -2;
  p.unit_rows = EU2_UNIT_ROWS;
  // rotated targets and twined jobs walk their units column by column (eu_xcd_tile): their source lines are
  // shared between vertically neighbouring tiles. EU_HIP_COLMAJOR=0 / 1 forces one walk (A/B runs).
  const bool cm = sw->colmajor >= 0 ? sw->colmajor != 0 : (p.form != EU_FORM_BA || p.twine);
  if (cm) p.unit_rows = -p.unit_rows;
  p.tiles_x = (p.width + EU2_TILE_W - 1) / EU2_TILE_W;
  p.tiles_y = (p.row_end - p.row_begin + EU2_TILE_H - 1) / EU2_TILE_H;
  if (p.tiles_x <= 0 || p.tiles_y <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  switch (p.nch) {
    case 1: return launch2_n<1>(p, st);
    case 2: return launch2_n<2>(p, st);
    case 3: return launch2_n<3>(p, st);
    case 4: return launch2_n<4>(p, st);
  }
  return -2;
}
