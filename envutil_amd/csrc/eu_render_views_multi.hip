// Many views of a multi-facet job in one call (eu_hip_render_views_multi): what eu_render_views.hip is to
// eu_render_kernel, this file is to eu_render_multi_kernel. The views share the target's projection, size,
// channels and tap table and the facets; they differ in orientation and extent, so everything a view changes is
// a stepper table: col [6][W] of the view, row [nfct][H][EU_ROW_FLOATS] of its facets. eu_view_tables_kernel
// (eu_render_views.hip) builds them from one scalar block per (view, facet); the kernel below has the view on
// blockIdx.y and offsets col, row and out by it.
//
//   eu_views_multi_kernel<NCH, DEG, PLUS, SYN, BIG>   eu_render_multi_kernel's body on the tables of view blockIdx.y
//
// It calls the device functions of eu_multi_dev.h with GEN = false (a facet with translation is refused: it is
// stepped by the generic stepper, whose tf3d_t is host work per view) and without early-miss tables. The
// strides are kernel arguments and blockIdx.y is wave-uniform, so the three offsets are scalar arithmetic.
// The instantiation of a job is chosen by eu_multi_ladder (eu_multi_dev.h), as for eu_render_multi_kernel.
//
// Why the body is written out here and in eu_render_multi.hip, and not one device function called by both: every
// kernel of the two families is held at 96 registers by EU_MULTI_OCC and spills, and where the allocator puts
// the spills moved with the body in a function. With the parameter block taken by reference, three
// instantiations of eu_render_multi_kernel and four of this kernel had 16-32 bytes more scratch per lane; by
// value eu_views_multi_kernel<3, 2, hdr> had 260 bytes for 244, and the 64-view jobs of tools/views_multi_time.py
// ran 2 % (RGB) and 1 % (RGBA) slower in each of three runs. A change to the body is made in both files.
// gridDim.x is eu_xcd_grid(), a multiple of 8: workgroup (x, y) still runs on XCD x % 8.
// The Makefile compiles this file once per channel count (EU_MULTI_NCH), like eu_render_multi.hip, and once
// without for the dispatcher. Compiled with -ffp-contract=off like every kernel file.
#include <cstring>
#undef EU_MULTI_STAMPS       // the stamps of the diagnostic build belong to eu_render_multi.hip
#include "eu_multi_dev.h"

#define EU_CAT2(a, b) a##b
#define EU_CAT(a, b) EU_CAT2(a, b)

#ifdef EU_MULTI_NCH

template <int NCH, int DEG, bool PLUS, int SYN, bool BIG>
__global__ __launch_bounds__(256) EU_MULTI_OCC void eu_views_multi_kernel(const eu_multi_params p0, const eu_view_strides vs)
{
  extern __shared__ float eu_dyn_lds[];
  const int b = eu_xcd_tile(blockIdx.x, p0.tiles_x, p0.tiles_y, -EU_UNIT_ROWS);
  if (b < 0) return;
  // this view's tables and frame
  eu_multi_params p = p0;
  const long long view = blockIdx.y;
  p.col = p0.col + view * vs.col;
  p.row = p0.row + view * vs.row;
  p.out = p0.out + view * vs.out;
  const int tile_y = b / p.tiles_x, tile_x = b - tile_y * p.tiles_x;
  const int lane = threadIdx.x & 63;
  const int wrow = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  eu_pix px;
  px.x = tile_x * EU_TILE_W + lane;
  px.y = p.row_begin + tile_y * EU_TILE_H + wrow;
  if (px.y >= p.row_end) return;              // wave-uniform
  const bool live = px.x < p.width;
  if (!live) px.x = p.width - 1;              // keeps table reads in range; no store
  eu_slots sl;
  sl.keep = p.nfct <= EU_MULTI_KEEP;
  sl.z = eu_dyn_lds + threadIdx.x;
  sl.sx = sl.z + p.nfct * 256;
  sl.sy = sl.sx + p.nfct * 256;
  float out[NCH];
  if (!p.twine) {
    if constexpr (eu_mode_feather(SYN)) eu_synopsis_feather<NCH, DEG, false, SYN == EU_MODE_FEATHER_EDGES>(p, px, false, 0.0f, 0.0f, out);
    else if constexpr (SYN == EU_MODE_HDR) eu_synopsis_hdr<NCH, DEG, false>(p, px, live, false, 0.0f, 0.0f, out);
    else if constexpr (BIG) eu_synopsis_big<NCH, DEG, false>(p, px, live, false, 0.0f, 0.0f, sl, out);
    else eu_synopsis<NCH, DEG, PLUS, false>(p, px, live, false, 0.0f, 0.0f, sl, out);
  } else {
#pragma unroll
    for (int c = 0; c < NCH; c++) out[c] = 0.0f;
    for (int k = 0; k < p.ntaps; k++) {
      const float cx = p.taps[3 * k], cy = p.taps[3 * k + 1], cw = p.taps[3 * k + 2];
      float help[NCH];
      if constexpr (eu_mode_feather(SYN)) eu_synopsis_feather<NCH, DEG, false, SYN == EU_MODE_FEATHER_EDGES>(p, px, true, cx, cy, help);
      else if constexpr (SYN == EU_MODE_HDR) eu_synopsis_hdr<NCH, DEG, false>(p, px, live, true, cx, cy, help);
      else if constexpr (BIG) eu_synopsis_big<NCH, DEG, false>(p, px, live, true, cx, cy, sl, help);
      else eu_synopsis<NCH, DEG, PLUS, false>(p, px, live, true, cx, cy, sl, help);
#pragma unroll
      for (int c = 0; c < NCH; c++) out[c] = out[c] + cw * help[c];
    }
  }
  if (!live) return;
  eu_put<NCH>(p.out + (long long)(px.y - p.row_begin) * p.out_stride, px.x, out);
}

// GEN falls away: the one kernel of each (DEG, SYN, BIG)
template <int NCH, bool PLUS>
struct launch_views_multi {
  static constexpr bool layers = false;         // no EU_MODE_LAYERS: eu_hip_render_views_multi refuses the multi-band synopsis
  const eu_multi_params &p;
  const eu_view_strides &vs;
  int nviews;
  hipStream_t st;
  template <int DEG, int SYN, bool GEN, bool BIG>
  void go(size_t lds) const
  {
    dim3 grid((unsigned)eu_xcd_grid(p.tiles_x, p.tiles_y, EU_UNIT_ROWS), (unsigned)nviews), block(256);
    hipLaunchKernelGGL((eu_views_multi_kernel<NCH, DEG, PLUS, SYN, BIG>), grid, block, lds, st, p, vs);
  }
};

// this translation unit carries the kernels of ONE channel count
extern "C" int EU_CAT(eu_launch_render_views_multi_nch, EU_MULTI_NCH)(const eu_multi_params *p, const eu_view_strides *vs,
                                                                     int nviews, int degree, void *stream)
{
  constexpr bool plus = EU_MULTI_NCH == 2 || EU_MULTI_NCH == 4;
  return eu_multi_ladder<plus>(*p, degree, launch_views_multi<EU_MULTI_NCH, plus>{ *p, *vs, nviews, (hipStream_t)stream });
}

#else

// p describes view 0 of the launch: whole frames, no row bands, no generic stepper, no early-miss tables
extern "C" int eu_launch_render_views_multi(const eu_multi_params *pp, const eu_view_strides *vs, int nviews, int degree,
                                            void *stream)
{
  eu_multi_params p = *pp;
  if (nviews <= 0) return 0;
  if (nviews > EU_VIEWS_MAX_GRID_Y || p.nfct < 1 || p.row_begin != 0 || p.row_end != p.height || p.band_count > 1 ||
      p.gen || p.rej || p.form == EU_FORM_GENERIC)
    return -2;
  p.tiles_x = (p.width + EU_TILE_W - 1) / EU_TILE_W;
  p.tiles_y = (p.height + EU_TILE_H - 1) / EU_TILE_H;
  if (p.tiles_x <= 0 || p.tiles_y <= 0) return 0;
  switch (p.nch) {
    case 1: return eu_launch_render_views_multi_nch1(&p, vs, nviews, degree, stream);
    case 2: return eu_launch_render_views_multi_nch2(&p, vs, nviews, degree, stream);
    case 3: return eu_launch_render_views_multi_nch3(&p, vs, nviews, degree, stream);
    case 4: return eu_launch_render_views_multi_nch4(&p, vs, nviews, degree, stream);
  }
  return -2;
}

#endif
