// `act` and `put` without a stepper: the source is evaluated at rays the caller supplies
// (eu_hip_render_rays). What the render kernels obtain from the stepper tables is here a coalesced read
// of an array; everything behind it - coordinate stage, gates, b-spline, brighten, channel adaption, the
// twining loop - is the render kernels' own device code in the render kernels' order (eu_pixel in
// eu_render_dev.h, eu_pixels2 in eu_packed_dev.h: the one copy of each pixel path), so the rays of a job
// give that job's frame bit for bit. Compiled with -ffp-contract=off like them.
//
//   eu_rays_kernel<NCH, DEG, TWINE>        one ray or ninepack per lane; every mount and degree (DEG -1:
//                                          run-time degree), channel adaption, --mask_for sources
//   eu_rays2_kernel<NCH, DEG, PRJ, TWINE>  two per lane (k and k + 64 of a row, as eu_render2_kernel lays
//                                          pixels out) through eu_coord2 / eu_eval2: lat/lon, cubemap and
//                                          biatan6 sources at degrees 1-3
//
// Ray reads. The 64 rays of a wave are 768 contiguous bytes and are read 12 bytes per lane in one
// instruction (global_load_dwordx3; rows are 4-byte aligned, which is all that instruction asks). A
// ninepack is 36 bytes: the wave's ninepacks are read the same way - contiguous 12-byte pieces, lane after
// lane - and every lane picks its own nine floats out of the wave's slice of LDS (strides of 3 and 9 dwords
// are free of bank conflicts). Three stride-12 dword loads per lane, or stride-36 loads, would be the
// quad-granular pattern DESIGN.md 5 measured at 7 L1 accesses per pixel.
//
// Rays are arbitrary bit patterns: eu_ray_guard.h says which of them are misses, and why nothing else can
// make a gather leave the container.
#include <hip/hip_runtime.h>
#include "eu_packed_dev.h"
#include "eu_ray_guard.h"
#include "eu_launch.h"

#define EUR_TILE_H 4        // waves of a workgroup: four rows of the grid, or four pieces of a flat list
#define EUR_FLAT_TILES 32   // flat list: tiles per row of the virtual grid eu_xcd_tile deals out to the XCDs

typedef float eu_f3 __attribute__((ext_vector_type(3)));

__device__ __forceinline__ eu_f3 eu_load3(const float *q)
{
  eu_f3 v;
  __builtin_memcpy(&v, q, 12);
  return v;
}

// the wave's piece of the grid: row y and first column x0, both wave-uniform; false: none
template <int TILE_W>
__device__ __forceinline__ bool eu_rays_tile(const eu_rays_params &p, int wave, int &x0, int &y)
{
  const int b = eu_xcd_tile(blockIdx.x, p.tiles_x, p.tiles_y, p.unit_rows);
  if (b < 0) return false;
  if (p.flat) {
    const long long first = ((long long)b * EUR_TILE_H + wave) * TILE_W;
    if (first >= p.width) return false;
    x0 = (int)first; y = 0;
    return true;
  }
  const int tile_y = b / p.tiles_x, tile_x = b - tile_y * p.tiles_x;
  x0 = tile_x * TILE_W;
  y = tile_y * EUR_TILE_H + wave;
  return y < p.height;
}

// the n ninepacks of a wave (n <= PIX), 9 * n contiguous floats at src, into the wave's slice of LDS
template <int PIX>
__device__ __forceinline__ void eu_ninepacks(const float *src, int n, float *slice, int lane)
{
#pragma unroll
  for (int j = 0; j < PIX * 3 / 64; j++) {
    const int v = j * 64 + lane;             // 12-byte piece v of the wave's 3 * n
    if (v < 3 * n) {
      const eu_f3 t = eu_load3(src + 3 * v);
      slice[3 * v] = t.x; slice[3 * v + 1] = t.y; slice[3 * v + 2] = t.z;
    }
  }
  // the slice belongs to this wave alone, and a wave's LDS accesses complete in order: only the
  // compiler has to keep the reads below behind the writes above
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a missed ray or ninepack goes through the arithmetic as the forward ray (finite coordinates on every
// mount, no slow paths) and counts as no hit where the source is evaluated. (Selecting zeros behind the
// evaluation instead cost the cubic RGB lat/lon instantiation of the packed form 121 registers for 79, and
// a vector of lane masks kept across the coordinate stage 81.)
template <int NIN>
__device__ __forceinline__ void eu_forward_if(bool miss, float *in)
{
#pragma unroll
  for (int k = 0; k < NIN; k++) in[k] = miss ? (k % 3 == 2 ? 1.0f : 0.0f) : in[k];
}

// environment::eval (eu_environment / eu_environment_repix) with the coordinate guard of eu_ray_guard.h
// between its two halves: the act eu_pixel (eu_render_dev.h) takes for the ray form. A missed lane counts
// as no hit in eval; repix evaluates it as the forward ray, and eu_pixel stores zeros for it
struct eu_rays_act {
  bool miss;
  template <int NCH, int DEG>
  __device__ __forceinline__ void eval(const eu_src_dev &s, float rx, float ry, float rz, float *px) const
  {
    float sx, sy;
    int face;
    bool hit = eu_source_coordinate(s, rx, ry, rz, sx, sy, face);
    hit = hit && eu_coord_finite(sx, sy) && !miss;
    eu_environment_at<NCH, DEG>(s, hit, sx, sy, px);
  }
  template <int NCH, int DEG>
  __device__ __forceinline__ void repix(const eu_src_dev &s, int out_n, float rx, float ry, float rz, float *px) const
  {
    float sx, sy;
    int face;
    bool hit = eu_source_coordinate(s, rx, ry, rz, sx, sy, face);
    hit = hit && eu_coord_finite(sx, sy);
    eu_environment_repix_at<NCH, DEG>(s, out_n, hit, sx, sy, px);
  }
};

// ---------------------------------------------------------------------------
// general form
// ---------------------------------------------------------------------------

template <int NCH, int DEG, bool TWINE>
__global__ __launch_bounds__(256) void eu_rays_kernel(const eu_rays_params p)
{
  constexpr int NIN = TWINE ? 9 : 3;
  __shared__ float pack[TWINE ? EUR_TILE_H * 64 * 9 : 1];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int x0, y;
  if (!eu_rays_tile<64>(p, wave, x0, y)) return;
  const int n = min(64, p.width - x0);
  const float *src = p.rays + (long long)y * p.ray_stride + (long long)x0 * NIN;
  float in[NIN];
  if constexpr (TWINE) {
    float *slice = pack + wave * 64 * 9;
    eu_ninepacks<64>(src, n, slice, lane);
    if (lane >= n) return;
#pragma unroll
    for (int k = 0; k < 9; k++) in[k] = slice[9 * lane + k];
  } else {
    if (lane >= n) return;
    const eu_f3 t = eu_load3(src + 3 * lane);
    in[0] = t.x; in[1] = t.y; in[2] = t.z;
  }
  bool miss;
  if constexpr (TWINE) miss = eu_ninepack_miss(in); else miss = eu_ray_miss(in[0], in[1], in[2]);
  eu_forward_if<NIN>(miss, in);
  const float rx = in[0], ry = in[1], rz = in[2];
  const int x = x0 + lane;
  float *dst = p.out + (long long)y * p.out_stride;

  eu_pixel<NCH, DEG, TWINE>(p, eu_rays_act{ miss }, rx, ry, rz,
      [&](float &ax, float &ay, float &az, float &bx, float &by, float &bz) __attribute__((always_inline)) {
        if constexpr (TWINE) {      // the ninepack's r10 and r01
          ax = in[3]; ay = in[4]; az = in[5];
          bx = in[6]; by = in[7]; bz = in[8];
        }
      }, dst, x);
}

// ---------------------------------------------------------------------------
// packed form
// ---------------------------------------------------------------------------

__device__ __forceinline__ eu_i2 eu_coord_finite2(eu_f2 sx, eu_f2 sy)
{
  return ((eu_bits2(sx) & 0x7f800000u) != 0x7f800000u) & ((eu_bits2(sy) & 0x7f800000u) != 0x7f800000u);
}

template <int NCH, int DEG, int PRJ, bool TWINE>
__global__ __launch_bounds__(256) void eu_rays2_kernel(const eu_rays_params p)
{
  constexpr int NIN = TWINE ? 9 : 3;
  // atanf range table in LDS (eu_math2.h): filled before any thread leaves
  __shared__ __attribute__((aligned(16))) float atab[EU_ATAN_TAB_FLOATS];
  __shared__ float pack[TWINE ? EUR_TILE_H * 128 * 9 : 1];
  if constexpr (PRJ != EU_CUBEMAP) {
    if (threadIdx.x < EU_ATAN_TAB_ENTRIES) eu_atan_tab_entry(threadIdx.x, atab + 8 * threadIdx.x);
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int x0, y;
  if (!eu_rays_tile<128>(p, wave, x0, y)) return;
  const int n = min(128, p.width - x0);
  const bool vb = lane + 64 < n;
  const int kb = vb ? lane + 64 : lane;       // a lane without a second ray evaluates its first twice
  const float *src = p.rays + (long long)y * p.ray_stride + (long long)x0 * NIN;
  float a[NIN], b[NIN];
  if constexpr (TWINE) {
    float *slice = pack + wave * 128 * 9;
    eu_ninepacks<128>(src, n, slice, lane);
    if (lane >= n) return;
#pragma unroll
    for (int k = 0; k < 9; k++) { a[k] = slice[9 * lane + k]; b[k] = slice[9 * kb + k]; }
  } else {
    if (lane >= n) return;
    const eu_f3 ta = eu_load3(src + 3 * lane), tb = eu_load3(src + 3 * kb);
    a[0] = ta.x; a[1] = ta.y; a[2] = ta.z;
    b[0] = tb.x; b[1] = tb.y; b[2] = tb.z;
  }
  bool miss_a, miss_b;
  if constexpr (TWINE) { miss_a = eu_ninepack_miss(a); miss_b = eu_ninepack_miss(b); }
  else { miss_a = eu_ray_miss(a[0], a[1], a[2]); miss_b = eu_ray_miss(b[0], b[1], b[2]); }
  eu_forward_if<NIN>(miss_a, a);
  eu_forward_if<NIN>(miss_b, b);
  eu_ray2 r00;
  r00.x = (eu_f2){ a[0], b[0] }; r00.y = (eu_f2){ a[1], b[1] }; r00.z = (eu_f2){ a[2], b[2] };

  float pxa[NCH], pxb[NCH];
  eu_pixels2<NCH, DEG, PRJ, TWINE>(p, r00,
      [&](eu_ray2 &r10, eu_ray2 &r01) __attribute__((always_inline)) {
        if constexpr (TWINE) {      // the ninepacks' r10 and r01
          r10.x = (eu_f2){ a[3], b[3] }; r10.y = (eu_f2){ a[4], b[4] }; r10.z = (eu_f2){ a[5], b[5] };
          r01.x = (eu_f2){ a[6], b[6] }; r01.y = (eu_f2){ a[7], b[7] }; r01.z = (eu_f2){ a[8], b[8] };
        }
      },
      // a missed lane is no hit BEFORE the evaluation (the register notes above eu_forward_if)
      [&](eu_i2 &hit, eu_f2 sx, eu_f2 sy) __attribute__((always_inline)) {
        hit = hit & eu_coord_finite2(sx, sy);
        hit.x = miss_a ? 0 : hit.x; hit.y = miss_b ? 0 : hit.y;
      }, atab, pxa, pxb);
  if constexpr (TWINE) {          // the sum of the taps' zeros, whatever the weights
#pragma unroll
    for (int c = 0; c < NCH; c++) { pxa[c] = miss_a ? 0.0f : pxa[c]; pxb[c] = miss_b ? 0.0f : pxb[c]; }
  }

  float *o = p.out + (long long)y * p.out_stride;
  const int xa = x0 + lane;
  eu_put<NCH>(o, xa, pxa);
  if (vb) eu_put<NCH>(o, xa + 64, pxb);
}

// ---------------------------------------------------------------------------
// launch
// ---------------------------------------------------------------------------

// tiles of tile_w x 4; a flat list (height 1) is dealt out as a virtual grid of EUR_FLAT_TILES tiles per row,
// every tile four consecutive pieces of tile_w, so that all XCDs and all four waves of a workgroup take part
static bool rays_grid(eu_rays_params &p, int tile_w)
{
  p.flat = p.height == 1;
  if (p.flat) {
    const long long pieces = ((long long)p.width + tile_w - 1) / tile_w;
    const long long tiles = (pieces + EUR_TILE_H - 1) / EUR_TILE_H;
    p.tiles_x = (int)std::min<long long>(tiles, EUR_FLAT_TILES);
    p.tiles_y = (int)((tiles + p.tiles_x - 1) / p.tiles_x);
    p.unit_rows = 1;
  } else {
    p.tiles_x = (p.width + tile_w - 1) / tile_w;
    p.tiles_y = (p.height + EUR_TILE_H - 1) / EUR_TILE_H;
    // neighbouring rows share an XCD's L2; a short grid still reaches every XCD
    p.unit_rows = std::max(1, std::min(EU_UNIT_ROWS, p.tiles_y / 8));
  }
  return p.tiles_x > 0 && p.tiles_y > 0;
}

template <int NCH, int DEG>
static void launch_rays_nd(const eu_rays_params &p, dim3 grid, hipStream_t st)
{
  if (p.ninputs == 9) hipLaunchKernelGGL((eu_rays_kernel<NCH, DEG, true>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((eu_rays_kernel<NCH, DEG, false>), grid, dim3(256), 0, st, p);
}

template <int NCH>
static void launch_rays_n(const eu_rays_params &p, dim3 grid, hipStream_t st)
{
  switch (p.src.degree) {
    case 0: return launch_rays_nd<NCH, 0>(p, grid, st);
    case 1: return launch_rays_nd<NCH, 1>(p, grid, st);
    case 2: return launch_rays_nd<NCH, 2>(p, grid, st);
    case 3: return launch_rays_nd<NCH, 3>(p, grid, st);
    default: return launch_rays_nd<NCH, -1>(p, grid, st);
  }
}

template <int NCH, int DEG, int PRJ>
static void launch_rays2_ndp(const eu_rays_params &p, dim3 grid, hipStream_t st)
{
  if (p.ninputs == 9) hipLaunchKernelGGL((eu_rays2_kernel<NCH, DEG, PRJ, true>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((eu_rays2_kernel<NCH, DEG, PRJ, false>), grid, dim3(256), 0, st, p);
}

template <int NCH, int DEG>
static int launch_rays2_nd(const eu_rays_params &p, dim3 grid, hipStream_t st)
{
  switch (p.src.prj) {
    case EU_SPHERICAL: launch_rays2_ndp<NCH, DEG, EU_SPHERICAL>(p, grid, st); return 0;
    case EU_CUBEMAP: launch_rays2_ndp<NCH, DEG, EU_CUBEMAP>(p, grid, st); return 0;
    case EU_BIATAN6: launch_rays2_ndp<NCH, DEG, EU_BIATAN6>(p, grid, st); return 0;
  }
  return -2;
}

template <int NCH>
static int launch_rays2_n(const eu_rays_params &p, dim3 grid, hipStream_t st)
{
  switch (p.src.degree) {
    case 1: return launch_rays2_nd<NCH, 1>(p, grid, st);
    case 2: return launch_rays2_nd<NCH, 2>(p, grid, st);
    case 3: return launch_rays2_nd<NCH, 3>(p, grid, st);
  }
  return -2;
}

// path: an eu_ray_path (eu_select.h: eu_select_ray_path decides before the call)
extern "C" int eu_launch_render_rays(const eu_rays_params *pp, int path, void *stream)
{
  eu_rays_params p = *pp;
  if (p.ninputs != 3 && p.ninputs != 9) return -2;
  const bool packed = path == EU_RAYS_PACKED;
  if (packed && !eu_packed_covers_source(p.src, p.nch, p.nch_out)) return -2;
  if (!rays_grid(p, packed ? 128 : 64)) return 0;
  const dim3 grid((unsigned)eu_xcd_grid(p.tiles_x, p.tiles_y, p.unit_rows));
  hipStream_t st = (hipStream_t)stream;
  int rc = 0;
  switch (p.nch) {
    case 1: if (packed) rc = launch_rays2_n<1>(p, grid, st); else launch_rays_n<1>(p, grid, st); break;
    case 2: if (packed) rc = launch_rays2_n<2>(p, grid, st); else launch_rays_n<2>(p, grid, st); break;
    case 3: if (packed) rc = launch_rays2_n<3>(p, grid, st); else launch_rays_n<3>(p, grid, st); break;
    case 4: if (packed) rc = launch_rays2_n<4>(p, grid, st); else launch_rays_n<4>(p, grid, st); break;
    default: return -2;
  }
  if (rc) return rc;
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
