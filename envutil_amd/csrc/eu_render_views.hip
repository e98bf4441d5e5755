// Many views of one resident source in one call (eu_hip_render_views): the camera of a tethered viewer, a
// camera path, a batch of crops from one panorama. Views share the target's projection, size, channels and tap
// table and differ in orientation and extent, so a launch has the view on blockIdx.y and nothing per view is
// done on the host beyond a block of scalars (eu::view_scalars, eu_view_dev).
//
//   eu_view_tables_kernel                   the stepper tables of every view of a chunk, col [6][W] and row
//                                           [H][EU_ROW_FLOATS]: the loops of eu::build_stepper_tables
//                                           (eu_setup_math.h), same operations in the same order, sinf / cosf /
//                                           tanf through eu_sinf / eu_cosf / eu_tanf (eu_math.h: glibc's bits)
//   eu_views_kernel<NCH, DEG, TWINE>        one pixel per lane: eu_pixel (eu_render_dev.h), the pixel path
//                                           eu_render_kernel and eu_rays_kernel run too
//   eu_views2_kernel<NCH, DEG, PRJ, TWINE>  two per lane in row strips: eu_pixels2 (eu_packed_dev.h), the pixel path
//                                           of eu_render2_kernel and eu_rays2_kernel
//
// What the render kernels have of their own is where a view's tables and frame are: every workgroup offsets col,
// row and out by its view and walks its view's tiles with eu_xcd_tile: gridDim.x is eu_xcd_grid(), a multiple of
// 8, so workgroup (x, y) still runs on XCD x % 8.
// Compiled with -ffp-contract=off like every kernel file.
#include <hip/hip_runtime.h>
#include "eu_packed_dev.h"
#include "eu_launch.h"

#define EUV2_TILE_W 128  // eu_render2.hip: pixels of one row per wave (2 per lane)
#define EUV2_TILE_H 4    // waves (rows) per workgroup
#define EUV2_UNIT_ROWS 8 // tile rows per XCD unit

// ---------------------------------------------------------------------------
// the table kernel
// ---------------------------------------------------------------------------

// eu::planar_columns for one column: the segment-start value of the column's lane, then one addition of delta
// per step the lane has made inside its segment of 512 (at most 31). Not a closed form: the sum rounds at every step.
__device__ __forceinline__ float eu_view_planar_x(const eu_view_dev &v, int W, int x, int biased)
{
  const int seg = (x / EU_SEGMENT) * EU_SEGMENT;
  const int lane = (x - seg) % EU_LANES, steps = (x - seg) / EU_LANES;
  const float ll0 = (float)(2 * lane) + (float)(seg * 2 + 1);
  float p = v.bias_x[biased] + ll0 * v.fx1 + ((float)(2 * W) - ll0) * v.fx0;
  for (int k = 0; k < steps; k++) p += v.delta;
  return p;
}

// eu::planar_row
__device__ __forceinline__ float eu_view_planar_y(const eu_view_dev &v, int H, int y, int biased)
{
  const int ll1 = y * 2 + 1;
  return v.bias_y[biased] + ll1 * v.fy1 + (float)(2 * H - ll1) * v.fy0;
}

// one variant (unbiased / y-biased) of a row-table entry: A, B, C, planar y; r has EU_ROW_VARIANT floats
__device__ __forceinline__ void eu_view_row(const eu_view_dev &v, int prj, int W, int H, int y, int biased, float *r)
{
  const float q = (float)(M_PI / 4.0);
  const float p1 = eu_view_planar_y(v, H, y, biased);
#pragma unroll
  for (int i = 0; i < EU_ROW_VARIANT; i++) r[i] = 0.0f;
  r[9] = p1;
  switch (prj) {
    case EU_SPHERICAL: {
      const float sy = eu_sinf(p1), rr = eu_cosf(p1);
      for (int i = 0; i < 3; i++) { r[3 + i] = v.xx[i] * rr; r[i] = v.yy[i] * sy; r[6 + i] = v.zz[i] * rr; }
      break;
    }
    case EU_CYLINDRICAL:
      for (int i = 0; i < 3; i++) { r[3 + i] = v.xx[i]; r[i] = v.yy[i] * p1; r[6 + i] = v.zz[i]; }
      break;
    case EU_RECTILINEAR:
      for (int i = 0; i < 3; i++) { r[3 + i] = v.xx[i]; r[i] = v.yy[i] * p1 + v.zz[i]; }
      break;
    case EU_FISHEYE:
    case EU_STEREOGRAPHIC:
      for (int i = 0; i < 3; i++) { r[i] = v.xx[i]; r[3 + i] = v.yy[i]; r[6 + i] = v.zz[i]; }
      break;
    default: {               // cubemap, biatan6
      const int face = y / W;
      float pp = p1 + (float)(3 - face) * v.section_md - v.refc_md;
      if (prj == EU_BIATAN6) pp = eu_tanf(pp * q);
      for (int i = 0; i < 3; i++) {
        const float xx = v.xx[i], yy = v.yy[i], zz = v.zz[i];
        float ccc, vvv;
        switch (face) {
          case 0: ccc = (float)(-1.0 * (double)xx + (double)(pp * yy)); vvv = zz; break;
          case 1: ccc = (float)(1.0 * (double)xx + (double)(pp * yy)); vvv = -zz; break;
          case 2: ccc = (float)(-1.0 * (double)yy - (double)(pp * zz)); vvv = -xx; break;
          case 3: ccc = (float)(1.0 * (double)yy + (double)(pp * zz)); vvv = -xx; break;
          case 4: ccc = (float)((double)(pp * yy) + 1.0 * (double)zz); vvv = xx; break;
          default: ccc = (float)((double)(pp * yy) - 1.0 * (double)zz); vvv = -xx; break;
        }
        r[i] = ccc;
        r[3 + i] = vvv;
      }
    }
  }
}

// thread t of view blockIdx.y: column t for t < W, row t - W behind that. Every float of both tables is written
// (the host function zero-fills what a projection or an untwined job leaves out), so the buffer needs no clearing.
__global__ __launch_bounds__(256) void eu_view_tables_kernel(const eu_view_dev *__restrict__ views, int prj, int W,
                                                             int H, int twine, float *__restrict__ col,
                                                             float *__restrict__ row)
{
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)W + H) return;
  const eu_view_dev v = views[blockIdx.y];
  const float q = (float)(M_PI / 4.0);
  if (t < W) {
    const int x = (int)t;
    float *c = col + (long long)blockIdx.y * 6 * W + x;
    const float p0 = eu_view_planar_x(v, W, x, 0);
    const float p0b = twine ? eu_view_planar_x(v, W, x, 1) : 0.0f;
    float c0 = p0, c1 = 0.0f, c0b = p0b, c1b = 0.0f;
    if (prj == EU_SPHERICAL || prj == EU_CYLINDRICAL) {
      c0 = eu_sinf(p0); c1 = eu_cosf(p0);
      if (twine) { c0b = eu_sinf(p0b); c1b = eu_cosf(p0b); }
    } else if (prj == EU_BIATAN6) {
      c0 = eu_tanf(p0 * q);
      if (twine) c0b = eu_tanf(p0b * q);
    }
    c[0] = c0;
    c[(long long)W] = c1;
    c[(long long)2 * W] = c0b;
    c[(long long)3 * W] = c1b;
    c[(long long)4 * W] = p0;
    c[(long long)5 * W] = p0b;
    return;
  }
  const int y = (int)(t - W);
  float r[EU_ROW_FLOATS];
  eu_view_row(v, prj, W, H, y, 0, r);
  if (twine) eu_view_row(v, prj, W, H, y, 1, r + EU_ROW_VARIANT);
  else {
#pragma unroll
    for (int i = 0; i < EU_ROW_VARIANT; i++) r[EU_ROW_VARIANT + i] = 0.0f;
  }
  float4 *dst = reinterpret_cast<float4 *>(row + ((long long)blockIdx.y * H + y) * EU_ROW_FLOATS);
#pragma unroll
  for (int i = 0; i < EU_ROW_FLOATS / 4; i++) dst[i] = make_float4(r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]);
}

extern "C" int eu_launch_view_tables(const eu_view_dev *views, int nviews, int prj, int width, int height, int twine,
                                     float *col, float *row, void *stream)
{
  if (nviews <= 0) return 0;
  if (nviews > EU_VIEWS_MAX_GRID_Y || width <= 0 || height <= 0 || prj < 0 || prj > EU_BIATAN6) return -2;
  const long long threads = (long long)width + height;
  dim3 grid((unsigned)((threads + 255) / 256), (unsigned)nviews);
  hipLaunchKernelGGL(eu_view_tables_kernel, grid, dim3(256), 0, (hipStream_t)stream, views, prj, width, height, twine,
                     col, row);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------
// general form (whole frames: no stages, no row bands)
// ---------------------------------------------------------------------------

template <int NCH, int DEG, bool TWINE>
__global__ __launch_bounds__(256) void eu_views_kernel(const eu_render_params p, const eu_view_strides vs)
{
  const int b = eu_xcd_tile(blockIdx.x, p.tiles_x, p.tiles_y, -EU_UNIT_ROWS);
  if (b < 0) return;
  const int tile_y = b / p.tiles_x, tile_x = b - tile_y * p.tiles_x;
  const int lane = threadIdx.x & 63;
  const int wrow = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int x = tile_x * EU_TILE_W + lane;
  const int y = tile_y * EU_TILE_H + wrow;   // wave-uniform
  if (y >= p.height || x >= p.width) return;

  const long long view = blockIdx.y;
  const float *col0 = p.col + view * vs.col, *col1 = col0 + p.width;
  const float *rowt = p.row + view * vs.row + (long long)y * EU_ROW_FLOATS;
  float rx, ry, rz;
  eu_stepper<false>(p.form, p.norm_mode, col0, col1, rowt, x, rx, ry, rz);

  float *dst = p.out + view * vs.out + (long long)y * p.out_stride;
  eu_pixel<NCH, DEG, TWINE>(p, eu_env_act(), rx, ry, rz,
      [&](float &ax, float &ay, float &az, float &bx, float &by, float &bz) __attribute__((always_inline)) {
        eu_stepper<false>(p.form, p.norm_mode, col0 + 2 * p.width, col0 + 3 * p.width, rowt, x, ax, ay, az);
        eu_stepper<false>(p.form, p.norm_mode, col0, col1, rowt + EU_ROW_VARIANT, x, bx, by, bz);
      }, dst, x);
}

// ---------------------------------------------------------------------------
// packed form
// ---------------------------------------------------------------------------

template <int NCH, int DEG, int PRJ, bool TWINE>
__global__ __launch_bounds__(256) void eu_views2_kernel(const eu_render_params p, const eu_view_strides vs)
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
  const int y = tile_y * EUV2_TILE_H + wave;
  if (y >= p.height) return;
  const int xa = tile_x * EUV2_TILE_W + lane, xb = xa + 64;
  if (xa >= p.width) return;
  const bool vb = xb < p.width;
  const int xbc = vb ? xb : xa;

  const long long view = blockIdx.y;
  const float *col = p.col + view * vs.col;
  eu_cptr rowt = (eu_cptr)(p.row + view * vs.row + (long long)y * EU_ROW_FLOATS);
  const eu_ray2 r00 = eu_rays2(p.form, p.norm_mode, rowt, col, col + p.width, xa, xbc);

  float pxa[NCH], pxb[NCH];
  eu_pixels2<NCH, DEG, PRJ, TWINE>(p, r00,
      [&](eu_ray2 &r10, eu_ray2 &r01) __attribute__((always_inline)) {
        r10 = eu_rays2(p.form, p.norm_mode, rowt, col + 2 * p.width, col + 3 * p.width, xa, xbc);
        r01 = eu_rays2(p.form, p.norm_mode, rowt + EU_ROW_VARIANT, col, col + p.width, xa, xbc);
      },
      [](eu_i2 &, eu_f2, eu_f2) __attribute__((always_inline)) {}, atab, pxa, pxb);

  float *o = p.out + view * vs.out + (long long)y * p.out_stride;
  eu_put<NCH>(o, xa, pxa);
  if (vb) eu_put<NCH>(o, xb, pxb);
}

// ---------------------------------------------------------------------------
// launch
// ---------------------------------------------------------------------------

template <int NCH, int DEG>
static void launch_views_nd(const eu_render_params &p, const eu_view_strides &vs, dim3 grid, hipStream_t st)
{
  if (p.twine) hipLaunchKernelGGL((eu_views_kernel<NCH, DEG, true>), grid, dim3(256), 0, st, p, vs);
  else hipLaunchKernelGGL((eu_views_kernel<NCH, DEG, false>), grid, dim3(256), 0, st, p, vs);
}

template <int NCH>
static void launch_views_n(const eu_render_params &p, const eu_view_strides &vs, dim3 grid, hipStream_t st)
{
  switch (p.src.degree) {
    case 0: return launch_views_nd<NCH, 0>(p, vs, grid, st);
    case 1: return launch_views_nd<NCH, 1>(p, vs, grid, st);
    case 2: return launch_views_nd<NCH, 2>(p, vs, grid, st);
    case 3: return launch_views_nd<NCH, 3>(p, vs, grid, st);
    default: return launch_views_nd<NCH, -1>(p, vs, grid, st);
  }
}

template <int NCH, int DEG, int PRJ>
static void launch_views2_ndp(const eu_render_params &p, const eu_view_strides &vs, dim3 grid, hipStream_t st)
{
  if (p.twine) hipLaunchKernelGGL((eu_views2_kernel<NCH, DEG, PRJ, true>), grid, dim3(256), 0, st, p, vs);
  else hipLaunchKernelGGL((eu_views2_kernel<NCH, DEG, PRJ, false>), grid, dim3(256), 0, st, p, vs);
}

template <int NCH, int DEG>
static int launch_views2_nd(const eu_render_params &p, const eu_view_strides &vs, dim3 grid, hipStream_t st)
{
  switch (p.src.prj) {
    case EU_SPHERICAL: launch_views2_ndp<NCH, DEG, EU_SPHERICAL>(p, vs, grid, st); return 0;
    case EU_CUBEMAP: launch_views2_ndp<NCH, DEG, EU_CUBEMAP>(p, vs, grid, st); return 0;
    case EU_BIATAN6: launch_views2_ndp<NCH, DEG, EU_BIATAN6>(p, vs, grid, st); return 0;
  }
  return -2;
}

template <int NCH>
static int launch_views2_n(const eu_render_params &p, const eu_view_strides &vs, dim3 grid, hipStream_t st)
{
  switch (p.src.degree) {
    case 1: return launch_views2_nd<NCH, 1>(p, vs, grid, st);
    case 2: return launch_views2_nd<NCH, 2>(p, vs, grid, st);
    case 3: return launch_views2_nd<NCH, 3>(p, vs, grid, st);
  }
  return -2;
}

// path: an eu_view_path (eu_select.h: eu_select_view_path decides before the call)
extern "C" int eu_launch_render_views(const eu_render_params *pp, const eu_view_strides *vs, int nviews, int path,
                                      const eu_switches *sw, void *stream)
{
  eu_render_params p = *pp;
  if (nviews <= 0) return 0;
  if (nviews > EU_VIEWS_MAX_GRID_Y || p.stage != 0 || p.band_count > 1 || p.row_begin != 0 || p.row_end != p.height ||
      p.form == EU_FORM_GENERIC)
    return -2;
  const bool packed = path == EU_VIEWS_PACKED;
  if (packed && !eu_packed_covers(p)) return -2;
  if (packed) {
    // as eu_launch_render2: rotated targets and twined jobs walk their units column by column
    const bool cm = sw->colmajor >= 0 ? sw->colmajor != 0 : (p.form != EU_FORM_BA || p.twine);
    p.unit_rows = cm ? -EUV2_UNIT_ROWS : EUV2_UNIT_ROWS;
    p.tiles_x = (p.width + EUV2_TILE_W - 1) / EUV2_TILE_W;
    p.tiles_y = (p.height + EUV2_TILE_H - 1) / EUV2_TILE_H;
  } else {
    p.unit_rows = -EU_UNIT_ROWS;
    p.tiles_x = (p.width + EU_TILE_W - 1) / EU_TILE_W;
    p.tiles_y = (p.height + EU_TILE_H - 1) / EU_TILE_H;
  }
  if (p.tiles_x <= 0 || p.tiles_y <= 0) return 0;
  const dim3 grid((unsigned)eu_xcd_grid(p.tiles_x, p.tiles_y, p.unit_rows), (unsigned)nviews);
  hipStream_t st = (hipStream_t)stream;
  int rc = 0;
  switch (p.nch) {
    case 1: if (packed) rc = launch_views2_n<1>(p, *vs, grid, st); else launch_views_n<1>(p, *vs, grid, st); break;
    case 2: if (packed) rc = launch_views2_n<2>(p, *vs, grid, st); else launch_views_n<2>(p, *vs, grid, st); break;
    case 3: if (packed) rc = launch_views2_n<3>(p, *vs, grid, st); else launch_views_n<3>(p, *vs, grid, st); break;
    case 4: if (packed) rc = launch_views2_n<4>(p, *vs, grid, st); else launch_views_n<4>(p, *vs, grid, st); break;
    default: return -2;
  }
  if (rc) return rc;
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
