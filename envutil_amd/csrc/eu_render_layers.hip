// Many pictures of one geometry in one call (eu_hip_render_layers): the eyes of a stereo pair, the exposures of a
// bracket, the passes of a rendered panorama, frames of a video. The layers share projection, size, field of view,
// orientation, lens, degree and container layout (the entry point checks it), so everything of a pixel that does
// not depend on the picture is computed ONCE - stepper -> ray, ray -> source coordinate, gate, split, b-spline
// weights, texel offsets; for a twined job once per tap - and only the taps, the weighted sum, brighten and the
// store are done per layer. Layer k is bit for bit what the single-picture kernels give for source k: the same
// operations in the same order, only no longer repeated.
//
//   eu_layers2_kernel<NCH, DEG, PRJ, TWINE>  two pixels per lane in row strips, as eu_render2_kernel: eu_rays2 and
//                                            eu_coord2 as there; eu_eval2 in two halves, eu_layers_front2 (once)
//                                            and eu_layers_back2 (per layer)
//   eu_layers_kernel<NCH, DEG, TWINE>        one pixel per lane, as eu_render_kernel: eu_source_coordinate and
//                                            eu_split once, then per layer what eu_environment_at /
//                                            eu_environment_repix_at do behind them
//
// The halves are written here, beside eu_eval2 and eu_environment_at, which stay as they are for their callers.
// What differs between layers is an eu_layer_dev {base, brighten}: a table in device memory, indexed wave-uniformly
// and so read through the scalar cache. Offsets are 64-bit; es1 is shared by the agreement rule.
//
// A twined job needs one sum per layer across the tap loop: layers are taken in groups of EU_LAYERS_GROUP, a group
// runs the tap loop once (coordinates once per tap and group) and carries EU_LAYERS_GROUP x NCH sums (x 2 in the
// packed form). The sum of a layer adds the taps in the table's order from zero, acc = acc + cw * q, as eu_pixels2
// and eu_pixel do.
// Compiled with -ffp-contract=off like every kernel file.
#include <hip/hip_runtime.h>
#include "eu_packed_dev.h"
#include "eu_launch.h"

#define EUL2_TILE_W 128  // eu_render2.hip: pixels of one row per wave (2 per lane)
#define EUL2_TILE_H 4    // waves (rows) per workgroup
#define EUL2_UNIT_ROWS 8 // tile rows per XCD unit

typedef const __attribute__((address_space(4))) eu_layer_dev *eu_layer_cptr;   // scalar-cache loads

// ---------------------------------------------------------------------------
// packed form: eu_eval2 in two halves
// ---------------------------------------------------------------------------

// what eu_eval2 computes in front of its first texel read
template <int DEG>
struct eu_front2 {
  float wxa[DEG + 1], wxb[DEG + 1], wya[DEG + 1], wyb[DEG + 1];
  eu_f2 tx, ty;
  long long offa, offb;      // floats from a layer's base to the window's first texel
  eu_i2 hit;
};

template <int NCH, int DEG>
__device__ __forceinline__ void eu_layers_front2(const eu_src_dev &s, eu_f2 sx, eu_f2 sy, eu_i2 hit, eu_front2<DEG> &f)
{
  // gate + split (map.h, basis.h:102-146)
  eu_f2 gx = eu_gate2(sx, s.gate0, s.lower0, s.upper0);
  eu_f2 gy = eu_gate2(sy, s.gate1, s.lower1, s.upper1);
  eu_f2 fx, fy;
  if constexpr (DEG & 1) {
    fx = (eu_f2){ floorf(gx.x), floorf(gx.y) }; fy = (eu_f2){ floorf(gy.x), floorf(gy.y) };
  } else {
    fx = (eu_f2){ roundf(gx.x), roundf(gx.y) }; fy = (eu_f2){ roundf(gy.x), roundf(gy.y) };
  }
  f.tx = gx - fx; f.ty = gy - fy;
  constexpr int order = DEG + 1;
  eu_f2 wx[order], wy[order];
  if constexpr (DEG >= 2) {
    eu_weights2<DEG>(s.wm, f.tx, wx);
    eu_weights2<DEG>(s.wm, f.ty, wy);
  }
#pragma unroll
  for (int i = 0; i < order; i++) {
    if constexpr (DEG >= 2) { f.wxa[i] = wx[i].x; f.wxb[i] = wx[i].y; f.wya[i] = wy[i].x; f.wyb[i] = wy[i].y; }
    else { f.wxa[i] = f.wxb[i] = f.wya[i] = f.wyb[i] = 0.0f; }
  }
  // a lane without a hit reads every layer's window at the core origin (always inside the container, framed or
  // not); its result is discarded
  const int ixa = hit.x ? (int)fx.x : DEG / 2, iya = hit.x ? (int)fy.x : DEG / 2;
  const int ixb = hit.y ? (int)fx.y : DEG / 2, iyb = hit.y ? (int)fy.y : DEG / 2;
  f.offa = (long long)(ixa - DEG / 2) * NCH + (long long)(iya - DEG / 2) * s.es1;
  f.offb = (long long)(ixb - DEG / 2) * NCH + (long long)(iyb - DEG / 2) * s.es1;
  f.hit = hit;
}

// ... and behind it, for one layer: the weighted sum, environment::eval's brighten, zero on a miss
template <int NCH, int DEG>
__device__ __forceinline__ void eu_layers_back2(const eu_front2<DEG> &f, long long es1, const float *base,
                                                float brighten, float *pxa, float *pxb)
{
  eu_accumulate1<NCH, DEG>(base + f.offa, es1, f.wxa, f.wya, f.tx.x, f.ty.x, pxa);
  eu_accumulate1<NCH, DEG>(base + f.offb, es1, f.wxb, f.wyb, f.tx.y, f.ty.y, pxb);
  constexpr int ncol = (NCH == 2 || NCH == 4) ? NCH - 1 : NCH;
  const bool bright = brighten != 1.0f;
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    float va = pxa[c], vb = pxb[c];
    if (bright && c < ncol) { va = va * brighten; vb = vb * brighten; }
    pxa[c] = f.hit.x ? va : 0.0f;
    pxb[c] = f.hit.y ? vb : 0.0f;
  }
}

template <int NCH, int DEG, int PRJ, bool TWINE>
__global__ __launch_bounds__(256) void eu_layers2_kernel(const eu_render_params p, const eu_layers_params lp)
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
  const int y = tile_y * EUL2_TILE_H + wave;
  if (y >= p.height) return;
  const int xa = tile_x * EUL2_TILE_W + lane, xb = xa + 64;
  if (xa >= p.width) return;
  const bool vb = xb < p.width;
  const int xbc = vb ? xb : xa;

  const eu_src_dev &s = p.src;
  const eu_layer_cptr layers = (eu_layer_cptr)lp.layers;
  eu_cptr rowt = (eu_cptr)(p.row + (long long)y * EU_ROW_FLOATS);
  const eu_ray2 r00 = eu_rays2(p.form, p.norm_mode, rowt, p.col, p.col + p.width, xa, xbc);
  float *o = p.out + (long long)y * p.out_stride;

  if constexpr (!TWINE) {
    eu_f2 sx, sy;
    const eu_i2 hit = eu_coord2<PRJ>(s, r00, sx, sy, atab);
    eu_front2<DEG> f;
    eu_layers_front2<NCH, DEG>(s, sx, sy, hit, f);
    for (int k = 0; k < lp.nlayers; k++) {
      const float *base = layers[k].base;
      const float brighten = layers[k].brighten;
      float pxa[NCH], pxb[NCH];
      eu_layers_back2<NCH, DEG>(f, s.es1, base, brighten, pxa, pxb);
      float *ok = o + (long long)k * lp.out_layer;
      eu_put<NCH>(ok, xa, pxa);
      if (vb) eu_put<NCH>(ok, xb, pxb);
    }
  } else {
    // twine_t::eval (twining.h:128-263), differencing branch, as eu_pixels2
    const eu_ray2 r10 = eu_rays2(p.form, p.norm_mode, rowt, p.col + 2 * p.width, p.col + 3 * p.width, xa, xbc);
    const eu_ray2 r01 = eu_rays2(p.form, p.norm_mode, rowt + EU_ROW_VARIANT, p.col, p.col + p.width, xa, xbc);
    const eu_f2 dxx = r10.x - r00.x, dxy = r10.y - r00.y, dxz = r10.z - r00.z;
    const eu_f2 dyx = r01.x - r00.x, dyy = r01.y - r00.y, dyz = r01.z - r00.z;
    eu_cptr taps = (eu_cptr)p.taps;
    for (int g = 0; g < eu_layers_groups(lp.nlayers); g++) {
      const int g0 = g * EU_LAYERS_GROUP, ng = eu_layers_in_group(lp.nlayers, g);      // wave-uniform
      float acca[EU_LAYERS_GROUP][NCH], accb[EU_LAYERS_GROUP][NCH];
#pragma unroll
      for (int j = 0; j < EU_LAYERS_GROUP; j++)
#pragma unroll
        for (int c = 0; c < NCH; c++) { acca[j][c] = 0.0f; accb[j][c] = 0.0f; }
      for (int k = 0; k < p.ntaps; k++) {
        const float cx = taps[3 * k], cy = taps[3 * k + 1], cw = taps[3 * k + 2];
        eu_ray2 rk;
        rk.x = r00.x + cx * dxx + cy * dyx;
        rk.y = r00.y + cx * dxy + cy * dyy;
        rk.z = r00.z + cx * dxz + cy * dyz;
        eu_f2 sx, sy;
        const eu_i2 hit = eu_coord2<PRJ>(s, rk, sx, sy, atab);
        eu_front2<DEG> f;
        eu_layers_front2<NCH, DEG>(s, sx, sy, hit, f);
#pragma unroll
        for (int j = 0; j < EU_LAYERS_GROUP; j++) {
          if (j < ng) {
            float qa[NCH], qb[NCH];
            eu_layers_back2<NCH, DEG>(f, s.es1, layers[g0 + j].base, layers[g0 + j].brighten, qa, qb);
#pragma unroll
            for (int c = 0; c < NCH; c++) { acca[j][c] = acca[j][c] + cw * qa[c]; accb[j][c] = accb[j][c] + cw * qb[c]; }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < EU_LAYERS_GROUP; j++) {
        if (j < ng) {
          float *ok = o + (long long)(g0 + j) * lp.out_layer;
          eu_put<NCH>(ok, xa, acca[j]);
          if (vb) eu_put<NCH>(ok, xb, accb[j]);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// general form (whole frames: no stages, no row bands, no --mask_for paint)
// ---------------------------------------------------------------------------

// what eu_split and the window's position give, once per coordinate
struct eu_front1 {
  float sx, sy, tx, ty;
  long long off;             // DEG >= 0: floats from a layer's base to the window's first texel
  bool hit;
};

template <int DEG>
__device__ __forceinline__ void eu_layers_front1(const eu_src_dev &s, bool hit, float sx, float sy, eu_front1 &f)
{
  f.hit = hit; f.sx = sx; f.sy = sy; f.tx = 0.0f; f.ty = 0.0f; f.off = 0;
  if constexpr (DEG >= 0) {
    if (hit) {
      int ix, iy;
      eu_split<DEG>(s, sx, sy, ix, iy, f.tx, f.ty);
      f.off = (long long)(ix - DEG / 2) * s.es0 + (long long)(iy - DEG / 2) * s.es1;
    }
  }
}

// eu_bspline_generic (eu_render_dev.h) on a layer's container: the runtime-degree evaluator for degrees above the
// specialised ones. A COPY, line for line, with `base` for s.base: whoever changes one changes the other
// (tests/test_gpu_layers.py holds "latlon d5" layers to eu_hip_render's bits)
template <int NCH>
__device__ void eu_layers_bspline_generic(const eu_src_dev &s, const float *base, float cx, float cy, float *out)
{
  const int d = s.degree, order = d + 1;
  float gx = eu_gate(cx, s.gate0, s.lower0, s.upper0);
  float gy = eu_gate(cy, s.gate1, s.lower1, s.upper1);
  float fx = (d & 1) ? floorf(gx) : roundf(gx);
  float fy = (d & 1) ? floorf(gy) : roundf(gy);
  float tx = gx - fx, ty = gy - fy;
  const float *p = base + (long long)(int)fx * s.es0 + (long long)(int)fy * s.es1;
  float wx[EU_MAX_DEGREE + 1], wy[EU_MAX_DEGREE + 1];
  for (int c = 0; c <= d; c++) { wx[c] = s.wm[c * order]; wy[c] = wx[c]; }
  float px = tx, py = ty;
  for (int row = 1; row <= d; row++) {
    for (int c = 0; c <= d; c++) {
      wx[c] = wx[c] + px * s.wm[c * order + row];
      wy[c] = wy[c] + py * s.wm[c * order + row];
    }
    if (row < d) { px = px * tx; py = py * ty; }
  }
  const float *p0 = p - (d / 2) * s.es1 - (d / 2) * s.es0;
  float sum[NCH];
  for (int j = 0; j < order; j++) {
    const float *rowp = p0 + j * s.es1;
    for (int c = 0; c < NCH; c++) {
      float r = rowp[c] * wx[0];
      for (int i = 1; i < order; i++) r = r + wx[i] * rowp[i * s.es0 + c];
      if (j == 0) sum[c] = r * wy[0];
      else sum[c] = sum[c] + r * wy[j];
    }
  }
  for (int c = 0; c < NCH; c++) out[c] = sum[c];
}

// the inner evaluation of a hit on one layer (eu_bspline / eu_bspline_generic behind the split)
template <int NCH, int DEG>
__device__ __forceinline__ void eu_layers_inner(const eu_src_dev &s, const eu_front1 &f, const float *base, float *raw)
{
  if constexpr (DEG >= 0) {
    eu_global_taps<NCH> g;
    g.es0 = s.es0; g.es1 = s.es1;
    g.p0 = base + f.off;
    eu_accumulate<NCH, DEG>(s.wm, f.tx, f.ty, g, raw);
  } else {
    eu_layers_bspline_generic<NCH>(s, base, f.sx, f.sy, raw);
  }
}

// One layer behind the coordinate. ADAPT false: eu_environment_at, px has NCH floats. ADAPT true: the target's
// channel count differs (repix_t), eu_environment_repix_at, px has room for 4 floats.
template <int NCH, int DEG, bool ADAPT>
__device__ __forceinline__ void eu_layers_back1(const eu_src_dev &s, int out_n, const eu_front1 &f, const float *base,
                                                float brighten, float *px)
{
  if constexpr (!ADAPT) {
    if (f.hit) {
      eu_layers_inner<NCH, DEG>(s, f, base, px);
      // environment::eval, environment.h:1821-1842
      if (brighten != 1.0f) {
        constexpr int ncol = (NCH == 2 || NCH == 4) ? NCH - 1 : NCH;
#pragma unroll
        for (int c = 0; c < ncol; c++) px[c] = px[c] * brighten;
      }
    } else {
#pragma unroll
      for (int c = 0; c < NCH; c++) px[c] = 0.0f;
    }
  } else {
    float raw[NCH];
    if (f.hit) eu_layers_inner<NCH, DEG>(s, f, base, raw);
    else {
#pragma unroll
      for (int c = 0; c < NCH; c++) raw[c] = 0.0f;
    }
    eu_repix<NCH>(out_n, raw, px);
    if (brighten != 1.0f) {
      const int ncol = (out_n == 2 || out_n == 4) ? out_n - 1 : out_n;
      for (int c = 0; c < ncol; c++) px[c] = px[c] * brighten;
    }
  }
}

// the pixel of every layer of the launch, as eu_pixel forms the pixel of one: CH channels are carried (NCH, or 4
// under channel adaption, of which the first p.nch_out are stored)
template <int NCH, int DEG, bool TWINE, bool ADAPT>
__device__ __forceinline__ void eu_layers_pixel(const eu_render_params &p, const eu_layers_params &lp,
                                                const float *rowt, int x, float rx, float ry, float rz, float *dst)
{
  constexpr int CH = ADAPT ? 4 : NCH;
  const int on = ADAPT ? p.nch_out : NCH;
  const eu_src_dev &s = p.src;
  const eu_layer_cptr layers = (eu_layer_cptr)lp.layers;
  float *o = dst + (long long)x * on;
  if constexpr (!TWINE) {
    float sx, sy;
    int face;
    const bool hit = eu_source_coordinate(s, rx, ry, rz, sx, sy, face);
    eu_front1 f;
    eu_layers_front1<DEG>(s, hit, sx, sy, f);
    for (int k = 0; k < lp.nlayers; k++) {
      float px[CH];
#pragma unroll
      for (int c = 0; c < CH; c++) px[c] = 0.0f;
      eu_layers_back1<NCH, DEG, ADAPT>(s, on, f, layers[k].base, layers[k].brighten, px);
      float *ok = o + (long long)k * lp.out_layer;
      if constexpr (ADAPT) { for (int c = 0; c < on; c++) ok[c] = px[c]; }
      else {
#pragma unroll
        for (int c = 0; c < NCH; c++) ok[c] = px[c];
      }
    }
  } else {
    // twine_t::eval (twining.h:128-263), differencing branch
    float ax, ay, az, bx, by, bz;
    eu_stepper<false>(p.form, p.norm_mode, p.col + 2 * p.width, p.col + 3 * p.width, rowt, x, ax, ay, az);   // r10
    eu_stepper<false>(p.form, p.norm_mode, p.col, p.col + p.width, rowt + EU_ROW_VARIANT, x, bx, by, bz);    // r01
    const float dxx = ax - rx, dxy = ay - ry, dxz = az - rz;
    const float dyx = bx - rx, dyy = by - ry, dyz = bz - rz;
    for (int g = 0; g < eu_layers_groups(lp.nlayers); g++) {
      const int g0 = g * EU_LAYERS_GROUP, ng = eu_layers_in_group(lp.nlayers, g);      // wave-uniform
      float acc[EU_LAYERS_GROUP][CH];
#pragma unroll
      for (int j = 0; j < EU_LAYERS_GROUP; j++)
#pragma unroll
        for (int c = 0; c < CH; c++) acc[j][c] = 0.0f;
      for (int k = 0; k < p.ntaps; k++) {
        const float cx = p.taps[3 * k], cy = p.taps[3 * k + 1], cw = p.taps[3 * k + 2];
        const float kx = rx + cx * dxx + cy * dyx;
        const float ky = ry + cx * dxy + cy * dyy;
        const float kz = rz + cx * dxz + cy * dyz;
        float sx, sy;
        int face;
        const bool hit = eu_source_coordinate(s, kx, ky, kz, sx, sy, face);
        eu_front1 f;
        eu_layers_front1<DEG>(s, hit, sx, sy, f);
#pragma unroll
        for (int j = 0; j < EU_LAYERS_GROUP; j++) {
          if (j < ng) {
            float q[CH];
#pragma unroll
            for (int c = 0; c < CH; c++) q[c] = 0.0f;
            eu_layers_back1<NCH, DEG, ADAPT>(s, on, f, layers[g0 + j].base, layers[g0 + j].brighten, q);
            if constexpr (ADAPT) { for (int c = 0; c < on; c++) acc[j][c] = acc[j][c] + cw * q[c]; }
            else {
#pragma unroll
              for (int c = 0; c < NCH; c++) acc[j][c] = acc[j][c] + cw * q[c];
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < EU_LAYERS_GROUP; j++) {
        if (j < ng) {
          float *ok = o + (long long)(g0 + j) * lp.out_layer;
          if constexpr (ADAPT) { for (int c = 0; c < on; c++) ok[c] = acc[j][c]; }
          else {
#pragma unroll
            for (int c = 0; c < NCH; c++) ok[c] = acc[j][c];
          }
        }
      }
    }
  }
}

template <int NCH, int DEG, bool TWINE>
__global__ __launch_bounds__(256) void eu_layers_kernel(const eu_render_params p, const eu_layers_params lp)
{
  const int b = eu_xcd_tile(blockIdx.x, p.tiles_x, p.tiles_y, -EU_UNIT_ROWS);
  if (b < 0) return;
  const int tile_y = b / p.tiles_x, tile_x = b - tile_y * p.tiles_x;
  const int lane = threadIdx.x & 63;
  const int wrow = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int x = tile_x * EU_TILE_W + lane;
  const int y = tile_y * EU_TILE_H + wrow;   // wave-uniform
  if (y >= p.height || x >= p.width) return;

  const float *rowt = p.row + (long long)y * EU_ROW_FLOATS;
  float rx, ry, rz;
  eu_stepper<false>(p.form, p.norm_mode, p.col, p.col + p.width, rowt, x, rx, ry, rz);
  float *dst = p.out + (long long)y * p.out_stride;
  if (p.nch_out != NCH) eu_layers_pixel<NCH, DEG, TWINE, true>(p, lp, rowt, x, rx, ry, rz, dst);
  else eu_layers_pixel<NCH, DEG, TWINE, false>(p, lp, rowt, x, rx, ry, rz, dst);
}

// ---------------------------------------------------------------------------
// launch
// ---------------------------------------------------------------------------

template <int NCH, int DEG>
static void launch_layers_nd(const eu_render_params &p, const eu_layers_params &lp, dim3 grid, hipStream_t st)
{
  if (p.twine) hipLaunchKernelGGL((eu_layers_kernel<NCH, DEG, true>), grid, dim3(256), 0, st, p, lp);
  else hipLaunchKernelGGL((eu_layers_kernel<NCH, DEG, false>), grid, dim3(256), 0, st, p, lp);
}

template <int NCH>
static void launch_layers_n(const eu_render_params &p, const eu_layers_params &lp, dim3 grid, hipStream_t st)
{
  switch (p.src.degree) {
    case 0: return launch_layers_nd<NCH, 0>(p, lp, grid, st);
    case 1: return launch_layers_nd<NCH, 1>(p, lp, grid, st);
    case 2: return launch_layers_nd<NCH, 2>(p, lp, grid, st);
    case 3: return launch_layers_nd<NCH, 3>(p, lp, grid, st);
    default: return launch_layers_nd<NCH, -1>(p, lp, grid, st);
  }
}

template <int NCH, int DEG, int PRJ>
static void launch_layers2_ndp(const eu_render_params &p, const eu_layers_params &lp, dim3 grid, hipStream_t st)
{
  if (p.twine) hipLaunchKernelGGL((eu_layers2_kernel<NCH, DEG, PRJ, true>), grid, dim3(256), 0, st, p, lp);
  else hipLaunchKernelGGL((eu_layers2_kernel<NCH, DEG, PRJ, false>), grid, dim3(256), 0, st, p, lp);
}

template <int NCH, int DEG>
static int launch_layers2_nd(const eu_render_params &p, const eu_layers_params &lp, dim3 grid, hipStream_t st)
{
  switch (p.src.prj) {
    case EU_SPHERICAL: launch_layers2_ndp<NCH, DEG, EU_SPHERICAL>(p, lp, grid, st); return 0;
    case EU_CUBEMAP: launch_layers2_ndp<NCH, DEG, EU_CUBEMAP>(p, lp, grid, st); return 0;
    case EU_BIATAN6: launch_layers2_ndp<NCH, DEG, EU_BIATAN6>(p, lp, grid, st); return 0;
  }
  return -2;
}

template <int NCH>
static int launch_layers2_n(const eu_render_params &p, const eu_layers_params &lp, dim3 grid, hipStream_t st)
{
  switch (p.src.degree) {
    case 1: return launch_layers2_nd<NCH, 1>(p, lp, grid, st);
    case 2: return launch_layers2_nd<NCH, 2>(p, lp, grid, st);
    case 3: return launch_layers2_nd<NCH, 3>(p, lp, grid, st);
  }
  return -2;
}

// For tests and tools (eu_hip.h): the group size THIS file's twined kernels were compiled with - here and not in the
// host glue, so that a library whose kernel file was built with another -DEU_LAYERS_GROUP says so
extern "C" int eu_hip_layers_group(void) { return EU_LAYERS_GROUP; }

// path: an eu_layer_path (eu_select.h: eu_select_layer_path decides before the call)
extern "C" int eu_launch_render_layers(const eu_render_params *pp, const eu_layers_params *lp, int path,
                                       const eu_switches *sw, void *stream)
{
  eu_render_params p = *pp;
  if (lp->nlayers <= 0) return 0;
  if (!lp->layers || p.stage != 0 || p.band_count > 1 || p.row_begin != 0 || p.row_end != p.height ||
      p.form == EU_FORM_GENERIC || p.src.mask_paint)
    return -2;
  const bool packed = path == EU_LAYERS_PACKED;
  if (packed && !eu_packed_covers(p)) return -2;
  if (packed) {
    // as eu_launch_render2: rotated targets and twined jobs walk their units column by column
    const bool cm = sw->colmajor >= 0 ? sw->colmajor != 0 : (p.form != EU_FORM_BA || p.twine);
    p.unit_rows = cm ? -EUL2_UNIT_ROWS : EUL2_UNIT_ROWS;
    p.tiles_x = (p.width + EUL2_TILE_W - 1) / EUL2_TILE_W;
    p.tiles_y = (p.height + EUL2_TILE_H - 1) / EUL2_TILE_H;
  } else {
    p.unit_rows = -EU_UNIT_ROWS;
    p.tiles_x = (p.width + EU_TILE_W - 1) / EU_TILE_W;
    p.tiles_y = (p.height + EU_TILE_H - 1) / EU_TILE_H;
  }
  if (p.tiles_x <= 0 || p.tiles_y <= 0) return 0;
  const dim3 grid((unsigned)eu_xcd_grid(p.tiles_x, p.tiles_y, p.unit_rows));
  hipStream_t st = (hipStream_t)stream;
  int rc = 0;
  switch (p.nch) {
    case 1: if (packed) rc = launch_layers2_n<1>(p, *lp, grid, st); else launch_layers_n<1>(p, *lp, grid, st); break;
    case 2: if (packed) rc = launch_layers2_n<2>(p, *lp, grid, st); else launch_layers_n<2>(p, *lp, grid, st); break;
    case 3: if (packed) rc = launch_layers2_n<3>(p, *lp, grid, st); else launch_layers_n<3>(p, *lp, grid, st); break;
    case 4: if (packed) rc = launch_layers2_n<4>(p, *lp, grid, st); else launch_layers_n<4>(p, *lp, grid, st); break;
    default: return -2;
  }
  if (rc) return rc;
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
