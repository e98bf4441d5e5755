// Multi-band blending (Burt-Adelson) behind stage A: the streaming kernels of EU_SYN_MULTIBAND and of
// eu_hip_blend_layers. No counterpart in the reference; the definition is this project's own (include/eu_hip.h,
// eu_target::bands) and tests/multiband_model.py restates it in numpy float32. Every operation is one of its own
// (-ffp-contract=off), in the order the definition writes it, so the device and the model agree bit for bit.
//
//   mb_prep_kernel        the caller's pictures (eu_hip_blend_layers) into layer planes: X_f, Q_f, qsum
//   mb_normalise_kernel   M_f^0 = Q_f > 0, W_f^0 = Q_f / qsum
//   mb_reduce_kernel      one level down, 5 x 5 fused through an LDS tile: rows first, then columns - the bits
//                         of the separable order. One plane per blockIdx.z
//   mb_band_kernel        one facet's band of one level into num / den; level l + 1 is expanded on the fly
//   mb_collapse_kernel    O^l = num / den + E(O^{l+1}) on levels L .. 1, in place in num
//   mb_finish_kernel      level 0 of the collapse and the pixel: interleaved, alpha and count applied
//
// All planes are dense floats of their level's size (eu_multiband.h). Every index clamps to the plane, columns
// wrap where the job says so; a thread or a workgroup past the plane does nothing. They are memory-bound sweeps.
#include "eu_multiband.h"
#include <vector>

#define MB_TW 32
#define MB_TH 8
#define MB_RAW_W (2 * MB_TW + 3)
#define MB_RAW_H (2 * MB_TH + 3)
#define MB_PLANES (EU_MB_MAXCOL + 2)

__device__ __forceinline__ int mb_col(int k, int n, int wrap)
{
  if (wrap) { k %= n; return k < 0 ? k + n : k; }
  return k < 0 ? 0 : (k >= n ? n - 1 : k);
}
__device__ __forceinline__ int mb_row(int k, int n) { return k < 0 ? 0 : (k >= n ? n - 1 : k); }

struct mb_prep_args {
  eu_mb_in in;
  float *X[EU_MB_MAXCOL], *Q;     // layer 0's planes; layer f lies f * lay floats behind
  float *qsum;
  long long lay;
  int ncol, nlay, w, h;
};

__global__ __launch_bounds__(256) void mb_prep_kernel(const mb_prep_args a)
{
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= a.w || y >= a.h) return;
  const long long at = (long long)y * a.w + x;
  float qsum = 0.0f;
  for (int f = 0; f < a.nlay; f++) {
    const float wt = a.in.weight[f * a.in.w_layer + y * a.in.w_row + x];
    const float q = wt > 0.0f ? wt : 0.0f;
    const float *c = a.in.colour + f * a.in.c_layer + y * a.in.c_row + (long long)x * a.ncol;
    for (int k = 0; k < a.ncol; k++) a.X[k][f * a.lay + at] = q > 0.0f ? c[k] : 0.0f;
    a.Q[f * a.lay + at] = q;
    qsum = qsum + q;
  }
  a.qsum[at] = qsum;
}

__global__ __launch_bounds__(256) void mb_normalise_kernel(const float *Q, const float *qsum, float *M, float *W, long long n)
{
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const float q = Q[k], s = qsum[k];
  M[k] = q > 0.0f ? 1.0f : 0.0f;
  float t = q / s;
  if (!(s > 0.0f)) t = 0.0f;
  W[k] = t;
}

struct mb_planes { const float *src[MB_PLANES]; float *dst[MB_PLANES]; };

// R: h[r, i] = (((A[r, 2i-2] + A[r, 2i+2]) + 4 (A[r, 2i-1] + A[r, 2i+1])) + 6 A[r, 2i]) / 16, then the same down
// the rows 2j-2 .. 2j+2 of h. A workgroup makes MB_TW x MB_TH values: the (2 MB_TW + 3) x (2 MB_TH + 3) source
// values under them go to LDS with their indices clamped or wrapped, the row pass fills a second tile.
__global__ __launch_bounds__(256) void mb_reduce_kernel(const mb_planes pl, int w, int h, int w2, int h2, int wrap)
{
  __shared__ float raw[MB_RAW_H][MB_RAW_W + 1];
  __shared__ float hz[MB_RAW_H][MB_TW + 1];
  const int i0 = blockIdx.x * MB_TW, j0 = blockIdx.y * MB_TH;
  if (i0 >= w2 || j0 >= h2) return;
  const float *A = pl.src[blockIdx.z];
  float *D = pl.dst[blockIdx.z];
  for (int k = threadIdx.x; k < MB_RAW_H * MB_RAW_W; k += 256) {
    const int r = k / MB_RAW_W, c = k - r * MB_RAW_W;
    raw[r][c] = A[(long long)mb_row(2 * j0 - 2 + r, h) * w + mb_col(2 * i0 - 2 + c, w, wrap)];
  }
  __syncthreads();
  for (int k = threadIdx.x; k < MB_RAW_H * MB_TW; k += 256) {
    const int r = k / MB_TW, i = k - r * MB_TW;
    const float *q = &raw[r][2 * i];
    hz[r][i] = (((q[0] + q[4]) + 4.0f * (q[1] + q[3])) + 6.0f * q[2]) * 0.0625f;
  }
  __syncthreads();
  const int i = threadIdx.x % MB_TW, j = threadIdx.x / MB_TW;
  if (i0 + i >= w2 || j0 + j >= h2) return;
  const float v = (((hz[2 * j][i] + hz[2 * j + 4][i]) + 4.0f * (hz[2 * j + 1][i] + hz[2 * j + 3][i])) + 6.0f * hz[2 * j + 2][i]) * 0.0625f;
  D[(long long)(j0 + j) * w2 + i0 + i] = v;
}

// E at (x, y) of the finer level from the wc x hc plane A: along the row first - even 2i: ((A[i-1] + A[i+1]) +
// 6 A[i]) / 8, odd 2i+1: (A[i] + A[i+1]) / 2 -, then the same down the columns of that
__device__ __forceinline__ float mb_expand_row(const float *q, int x, int wc, int wrap)
{
  const int i = x >> 1;
  if (x & 1) return (q[mb_col(i, wc, wrap)] + q[mb_col(i + 1, wc, wrap)]) * 0.5f;
  return ((q[mb_col(i - 1, wc, wrap)] + q[mb_col(i + 1, wc, wrap)]) + 6.0f * q[mb_col(i, wc, wrap)]) * 0.125f;
}
__device__ __forceinline__ float mb_expand(const float *A, int x, int y, int wc, int hc, int wrap)
{
  const int j = y >> 1;
  if (y & 1)
    return (mb_expand_row(A + (long long)mb_row(j, hc) * wc, x, wc, wrap) +
            mb_expand_row(A + (long long)mb_row(j + 1, hc) * wc, x, wc, wrap)) * 0.5f;
  return ((mb_expand_row(A + (long long)mb_row(j - 1, hc) * wc, x, wc, wrap) +
           mb_expand_row(A + (long long)mb_row(j + 1, hc) * wc, x, wc, wrap)) +
          6.0f * mb_expand_row(A + (long long)mb_row(j, hc) * wc, x, wc, wrap)) * 0.125f;
}

struct mb_band_args {
  const float *X[EU_MB_MAXCOL], *M, *W;       // this facet's level l
  const float *Xc[EU_MB_MAXCOL], *Mc;         // its level l + 1 (not read at the top)
  float *num[EU_MB_MAXCOL], *den;
  int ncol, w, h, wc, hc, wrap, top;
};

// B = X^l / M^l - E(X^{l+1}) / E(M^{l+1}) (the second term 0 unless E(M^{l+1}) > 0; at the top none), where
// M^l > 0: num += W^l * B, den += W^l
__global__ __launch_bounds__(256) void mb_band_kernel(const mb_band_args a)
{
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= a.w || y >= a.h) return;
  const long long at = (long long)y * a.w + x;
  const float m = a.M[at];
  if (!(m > 0.0f)) return;
  const float wt = a.W[at];
  float em = 0.0f;
  if (!a.top) em = mb_expand(a.Mc, x, y, a.wc, a.hc, a.wrap);
#pragma unroll
  for (int c = 0; c < EU_MB_MAXCOL; c++) {
    if (c >= a.ncol) break;
    float b = a.X[c][at] / m;
    if (!a.top) {
      float low = 0.0f;
      if (em > 0.0f) low = mb_expand(a.Xc[c], x, y, a.wc, a.hc, a.wrap) / em;
      b = b - low;
    }
    a.num[c][at] = a.num[c][at] + wt * b;
  }
  a.den[at] = a.den[at] + wt;
}

struct mb_collapse_args {
  float *num[EU_MB_MAXCOL];                   // level l; receives O^l
  const float *den;
  const float *Oc[EU_MB_MAXCOL];              // O^{l+1} (not read at the top)
  int w, h, wc, hc, wrap, top;
};

__global__ __launch_bounds__(256) void mb_collapse_kernel(const mb_collapse_args a)
{
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= a.w || y >= a.h) return;
  const long long at = (long long)y * a.w + x;
  const int c = blockIdx.z;
  const float d = a.den[at];
  float o = 0.0f;
  if (d > 0.0f) o = a.num[c][at] / d;
  if (!a.top) o = o + mb_expand(a.Oc[c], x, y, a.wc, a.hc, a.wrap);
  a.num[c][at] = o;
}

struct mb_finish_args {
  const float *num[EU_MB_MAXCOL], *den, *Oc[EU_MB_MAXCOL];
  const float *amax, *count;
  eu_mb_out o;
  int ncol, w, h, wc, hc, wrap, top;
};

__global__ __launch_bounds__(256) void mb_finish_kernel(const mb_finish_args a)
{
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= a.w || y >= a.h) return;
  const long long at = (long long)y * a.w + x;
  float *px = a.o.out + y * a.o.stride + (long long)x * a.o.nch;
  const bool none = a.o.count && a.count[at] == 0.0f;
  const float am = a.o.alpha ? a.amax[at] : 1.0f;
  const float d = a.den[at];
#pragma unroll
  for (int c = 0; c < EU_MB_MAXCOL; c++) {
    if (c >= a.ncol) break;
    float o = 0.0f;
    if (d > 0.0f) o = a.num[c][at] / d;
    if (!a.top) o = o + mb_expand(a.Oc[c], x, y, a.wc, a.hc, a.wrap);
    if (a.o.alpha) o = o * am;
    px[c] = none ? 0.0f : o;
  }
  if (a.o.alpha) px[a.ncol] = none ? 0.0f : am;
}

static inline dim3 mb_grid(int w, int h, int z = 1) { return dim3((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4), (unsigned)z); }

extern "C" int eu_launch_mb_prep(float *s, const eu_mb_geom *g, int ncol, int nlay, const eu_mb_in *in, void *stream)
{
  if (ncol < 1 || ncol > EU_MB_MAXCOL || nlay < 1) return -2;
  mb_prep_args a {};
  a.in = *in;
  for (int c = 0; c < ncol; c++) a.X[c] = eu_mb_layer(s, *g, ncol, 0, c);
  a.Q = eu_mb_layer(s, *g, ncol, 0, ncol);
  a.qsum = eu_mb_pixel(s, *g, ncol, nlay, 0);
  a.lay = (long long)(ncol + 1) * (long long)g->off[1];
  a.ncol = ncol; a.nlay = nlay; a.w = g->w[0]; a.h = g->h[0];
  hipLaunchKernelGGL(mb_prep_kernel, mb_grid(a.w, a.h), dim3(256), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// the diagnostic's events: one pair per launch, read and destroyed behind the job
struct mb_stamps {
  eu_mb_times *t;
  hipStream_t st;
  struct pair { hipEvent_t a, b; int stage; };
  std::vector<pair> ev;
  void before(int stage, double bytes)
  {
    if (!t) return;
    pair p { nullptr, nullptr, stage };
    if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) return;
    (void)hipEventRecord(p.a, st);
    ev.push_back(p);
    t->bytes[stage] += bytes;
  }
  void after() { if (t && !ev.empty()) (void)hipEventRecord(ev.back().b, st); }
  ~mb_stamps()
  {
    if (!t) return;
    (void)hipStreamSynchronize(st);
    for (pair &p : ev) {
      float ms = 0.0f;
      if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) t->ms[p.stage] += ms;
      (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b);
    }
  }
};

extern "C" int eu_launch_mb_blend(float *s, const eu_mb_geom *gp, int ncol, int nlay, const eu_mb_out *o, void *stream,
                                  eu_mb_times *times)
{
  const eu_mb_geom &g = *gp;
  hipStream_t st = (hipStream_t)stream;
  mb_stamps stamp { times, st, {} };
  if (ncol < 1 || ncol > EU_MB_MAXCOL || nlay < 1 || g.L < 0 || g.L > EU_MB_MAXL) return -2;
  if (o->nch != ncol + (o->alpha ? 1 : 0)) return -2;
  const int L = g.L;
  const size_t S0 = g.off[1], T = g.off[L + 1];
  auto S = [&](int l) { return g.off[l + 1] - g.off[l]; };
  float *pix = eu_mb_pixel(s, g, ncol, nlay, 0);
  float *fx = pix + 3 * S0;                               // X, levels 1 .. L
  float *fm = fx + (size_t)ncol * (T - S0), *fw = fm + T; // M and W, levels 0 .. L
  float *num = fw + T, *den = num + (size_t)ncol * T;
  auto X_at = [&](int f, int l, int c) { return l == 0 ? eu_mb_layer(s, g, ncol, f, c) : fx + (size_t)ncol * (g.off[l] - S0) + (size_t)c * S(l); };
  auto num_at = [&](int l, int c) { return num + (size_t)ncol * g.off[l] + (size_t)c * S(l); };
  if (hipMemsetAsync(num, 0, (size_t)(ncol + 1) * T * sizeof(float), st) != hipSuccess) return -1;
  for (int f = 0; f < nlay; f++) {
    const long long n0 = (long long)S0;
    stamp.before(EU_MB_T_NORMALISE, 16.0 * (double)S0);                         // Q, qsum in; M, W out
    hipLaunchKernelGGL(mb_normalise_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, st,
                       eu_mb_layer(s, g, ncol, f, ncol), pix, fm, fw, n0);
    stamp.after();
    for (int l = 0; l < L; l++) {
      mb_planes pl {};
      for (int c = 0; c < ncol; c++) { pl.src[c] = X_at(f, l, c); pl.dst[c] = X_at(f, l + 1, c); }
      pl.src[ncol] = fm + g.off[l]; pl.dst[ncol] = fm + g.off[l + 1];
      pl.src[ncol + 1] = fw + g.off[l]; pl.dst[ncol + 1] = fw + g.off[l + 1];
      const dim3 grid((unsigned)((g.w[l + 1] + MB_TW - 1) / MB_TW), (unsigned)((g.h[l + 1] + MB_TH - 1) / MB_TH), (unsigned)(ncol + 2));
      stamp.before(EU_MB_T_REDUCE, 4.0 * (ncol + 2) * (double)(S(l) + S(l + 1)));  // every plane in, its next level out
      hipLaunchKernelGGL(mb_reduce_kernel, grid, dim3(256), 0, st, pl, g.w[l], g.h[l], g.w[l + 1], g.h[l + 1], g.wrap);
      stamp.after();
    }
    for (int l = 0; l <= L; l++) {
      mb_band_args a {};
      a.ncol = ncol; a.w = g.w[l]; a.h = g.h[l]; a.wrap = g.wrap; a.top = l == L;
      a.M = fm + g.off[l]; a.W = fw + g.off[l]; a.den = den + g.off[l];
      for (int c = 0; c < ncol; c++) { a.X[c] = X_at(f, l, c); a.num[c] = num_at(l, c); }
      if (!a.top) {
        a.wc = g.w[l + 1]; a.hc = g.h[l + 1]; a.Mc = fm + g.off[l + 1];
        for (int c = 0; c < ncol; c++) a.Xc[c] = X_at(f, l + 1, c);
      }
      // X, M, W in, num and den in and out, and below the top the next level's X and M in (where M > 0: nominal)
      stamp.before(EU_MB_T_BAND, 4.0 * ((ncol + 2 + 2 * (ncol + 1)) * (double)S(l) + (a.top ? 0.0 : (ncol + 1) * (double)S(l + 1))));
      hipLaunchKernelGGL(mb_band_kernel, mb_grid(a.w, a.h), dim3(256), 0, st, a);
      stamp.after();
    }
  }
  for (int l = L; l >= 1; l--) {
    mb_collapse_args a {};
    a.w = g.w[l]; a.h = g.h[l]; a.wrap = g.wrap; a.top = l == L;
    a.den = den + g.off[l];
    for (int c = 0; c < ncol; c++) a.num[c] = num_at(l, c);
    if (!a.top) {
      a.wc = g.w[l + 1]; a.hc = g.h[l + 1];
      for (int c = 0; c < ncol; c++) a.Oc[c] = num_at(l + 1, c);
    }
    // num in and out, den in per channel, the next level's O in
    stamp.before(EU_MB_T_COLLAPSE, 4.0 * (3.0 * ncol * (double)S(l) + (a.top ? 0.0 : ncol * (double)S(l + 1))));
    hipLaunchKernelGGL(mb_collapse_kernel, mb_grid(a.w, a.h, ncol), dim3(256), 0, st, a);
    stamp.after();
  }
  mb_finish_args a {};
  a.ncol = ncol; a.w = g.w[0]; a.h = g.h[0]; a.wrap = g.wrap; a.top = L == 0;
  a.den = den; a.amax = pix + S0; a.count = pix + 2 * S0; a.o = *o;
  for (int c = 0; c < ncol; c++) a.num[c] = num_at(0, c);
  if (!a.top) {
    a.wc = g.w[1]; a.hc = g.h[1];
    for (int c = 0; c < ncol; c++) a.Oc[c] = num_at(1, c);
  }
  // num, den, amax, count in, the next level's O in, the pixel out
  stamp.before(EU_MB_T_COLLAPSE, 4.0 * ((ncol + 3 + o->nch) * (double)S0 + (a.top ? 0.0 : ncol * (double)S(1))));
  hipLaunchKernelGGL(mb_finish_kernel, mb_grid(a.w, a.h), dim3(256), 0, st, a);
  stamp.after();
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
