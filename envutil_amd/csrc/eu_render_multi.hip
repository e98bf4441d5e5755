// Multi-facet rendering: N steppers (one per source facet, each with that
// facet's composed rotation) feed a synopsis that picks / composites the facets
// per pixel.
//   fusion_t                zimt/get.h:1181-1242
//   synopsis_t (twining)    envutil_payload.cc:587-691
//   _voronoi_syn            envutil_payload.cc:762-957   (1 or 3 channels)
//   _voronoi_syn_plus       envutil_payload.cc:964-1233  (alpha: 2 or 4 channels)
//   _hdr_merge_syn          envutil_payload.cc:1325-1626 (args.synopsis == "hdr_merge")
//
// One thread per output pixel, 64x4 tiles like eu_render_kernel. The reference
// takes three decisions per 16-lane VECTOR (which facets enter the layer list,
// "one facet on top everywhere", "fully opaque"); a wavefront holds four such
// vectors (its 64 pixels start at a multiple of 64 inside a 512-pixel segment),
// so those decisions are wavefront ballots masked to 16-lane groups - the
// reference's any_of/all_of, bit for bit.
//
// The facets are walked by run-time loops (any count up to 64): the facet index
// is wave-uniform, its parameters come through the scalar cache. The mask pass
// computes every facet's source coordinate once; the coordinates (and, with
// alpha, the z scores the layers are sorted by) of up to 16 facets stay in LDS,
// one slot per thread, and the evaluation of the winning facet(s) starts from
// them. Facets whose evaluation differs between lanes are handled by a waterfall
// loop (readlane makes the index uniform, the lanes that want it go together).
#include <cstring>
#include "eu_render_dev.h"
#if defined(EU_MULTI_NCH) && defined(EU_MULTI_STAMPS)
// diagnostic build (tools/multi_stamps.py): shader-clock cycles per phase of eu_synopsis's alpha path, summed
// over the waves of a launch: [0] mask pass, [1] the top facet / all-top evaluation, [2] compositing, [3] waves
__device__ unsigned long long eu_multi_stamp_acc[1024 * 4];      // sharded by workgroup: one hot address serialises the launch
#endif
#include "eu_multi_dev.h"

#ifdef EU_MULTI_NCH
// GEN: some facet of the job is stepped by generic_stepper (translation, --single); only the run-time-degree
// variants are instantiated with it
// BIG: alpha compositing of more than 64 facets (eu_synopsis_big)
template <int NCH, int DEG, bool PLUS, int SYN, bool GEN, bool BIG>
__global__ __launch_bounds__(256) EU_MULTI_OCC void eu_render_multi_kernel(const eu_multi_params p)
{
  extern __shared__ float eu_dyn_lds[];
  const int b = eu_xcd_tile(blockIdx.x, p.tiles_x, p.tiles_y, -EU_UNIT_ROWS);
  if (b < 0) return;
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
  if constexpr (eu_mode_layers(SYN)) {
    // stage A of the multi-band synopsis: the layers go to their planes, no frame is written
    eu_synopsis_layers<NCH, DEG, GEN, SYN == EU_MODE_LAYERS_EDGES>(p, px, live);
    return;
  }
  float out[NCH];
  if (!p.twine) {
    if constexpr (eu_mode_feather(SYN)) eu_synopsis_feather<NCH, DEG, GEN, SYN == EU_MODE_FEATHER_EDGES>(p, px, false, 0.0f, 0.0f, out);
    else if constexpr (SYN == EU_MODE_HDR) eu_synopsis_hdr<NCH, DEG, GEN>(p, px, live, false, 0.0f, 0.0f, out);
    else if constexpr (BIG) eu_synopsis_big<NCH, DEG, GEN>(p, px, live, false, 0.0f, 0.0f, sl, out);
    else eu_synopsis<NCH, DEG, PLUS, GEN>(p, px, live, false, 0.0f, 0.0f, sl, out);
  } else {
#pragma unroll
    for (int c = 0; c < NCH; c++) out[c] = 0.0f;
    for (int k = 0; k < p.ntaps; k++) {
      const float cx = p.taps[3 * k], cy = p.taps[3 * k + 1], cw = p.taps[3 * k + 2];
      float help[NCH];
      if constexpr (eu_mode_feather(SYN)) eu_synopsis_feather<NCH, DEG, GEN, SYN == EU_MODE_FEATHER_EDGES>(p, px, true, cx, cy, help);
      else if constexpr (SYN == EU_MODE_HDR) eu_synopsis_hdr<NCH, DEG, GEN>(p, px, live, true, cx, cy, help);
      else if constexpr (BIG) eu_synopsis_big<NCH, DEG, GEN>(p, px, live, true, cx, cy, sl, help);
      else eu_synopsis<NCH, DEG, PLUS, GEN>(p, px, live, true, cx, cy, sl, help);
#pragma unroll
      for (int c = 0; c < NCH; c++) out[c] = out[c] + cw * help[c];
    }
  }
  if (!live) return;
  eu_put<NCH>(p.out + (long long)(px.y - p.row_begin) * p.out_stride, px.x, out);
}

template <int NCH, bool PLUS>
struct launch_multi {
  static constexpr bool layers = true;          // EU_MODE_LAYERS is instantiated here
  const eu_multi_params &p;
  hipStream_t st;
  template <int DEG, int SYN, bool GEN, bool BIG>
  void go(size_t lds) const
  {
    dim3 grid((unsigned)eu_xcd_grid(p.tiles_x, p.tiles_y, EU_UNIT_ROWS)), block(256);
    hipLaunchKernelGGL((eu_render_multi_kernel<NCH, DEG, PLUS, SYN, GEN, BIG>), grid, block, lds, st, p);
  }
};

#endif  // EU_MULTI_NCH

#define EU_CAT2(a, b) a##b
#define EU_CAT(a, b) EU_CAT2(a, b)

#if defined(EU_MULTI_NCH) && defined(EU_MULTI_STAMPS)
extern "C" int eu_multi_stamps_read(unsigned long long *out4)
{
  static unsigned long long h[1024 * 4];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(eu_multi_stamp_acc), sizeof h) != hipSuccess) return -1;
  for (int k = 0; k < 4; k++) { out4[k] = 0; for (int i = 0; i < 1024; i++) out4[k] += h[4 * i + k]; }
  memset(h, 0, sizeof h);
  return hipMemcpyToSymbol(HIP_SYMBOL(eu_multi_stamp_acc), h, sizeof h) == hipSuccess ? 0 : -1;
}
#endif
#ifdef EU_MULTI_NCH
// this translation unit carries the kernels of ONE channel count (the Makefile
// compiles the file four times, so that the four compile in parallel)
extern "C" int EU_CAT(eu_launch_render_multi_nch, EU_MULTI_NCH)(const eu_multi_params *p, int degree,
                                                               void *stream)
{
  constexpr bool plus = EU_MULTI_NCH == 2 || EU_MULTI_NCH == 4;
  return eu_multi_ladder<plus>(*p, degree, launch_multi<EU_MULTI_NCH, plus>{ *p, (hipStream_t)stream });
}
#else
extern "C" int eu_launch_render_multi(const eu_multi_params *pp, int degree, void *stream)
{
  eu_multi_params p = *pp;
  // voronoi_syn and hdr_merge keep no per-facet state; alpha compositing beyond 64 facets: eu_synopsis_big
  p.tiles_x = (p.width + EU_TILE_W - 1) / EU_TILE_W;
  p.tiles_y = (p.row_end - p.row_begin + EU_TILE_H - 1) / EU_TILE_H;
  if (p.tiles_x <= 0 || p.tiles_y <= 0) return 0;
  switch (p.nch) {
    case 1: return eu_launch_render_multi_nch1(&p, degree, stream);
    case 2: return eu_launch_render_multi_nch2(&p, degree, stream);
    case 3: return eu_launch_render_multi_nch3(&p, degree, stream);
    case 4: return eu_launch_render_multi_nch4(&p, degree, stream);
  }
  return -2;
}
#endif
