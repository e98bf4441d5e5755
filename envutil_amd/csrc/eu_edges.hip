// The distance plane of a source loaded with EU_LOAD_EDGES (include/eu_hip.h, "Feathering to alpha edges"): per
// window pixel the Euclidean distance, in source pixels, to the nearest pixel whose alpha is not positive. An exact
// Euclidean distance transform in two passes (Meijster, Roerdink, Hesselink 2000); everything up to the root is
// integer arithmetic, so the plane does not depend on the order anything runs in. Load-time work, queued by
// fill_source (eu_api_source.hip) between the alpha edit and the prefilter.
//
//   eu_edges_rows_kernel   pass 1: a workgroup per row. The row's outside pixels become one bit each in LDS (a ballot
//                          per 64 columns: the state a row longer than the workgroup carries from chunk to chunk is
//                          these words), one thread walks the words once in each direction for "last outside column
//                          in front of this word" / "first behind it" - seeded from the row's other end where the rows
//                          close -, and every lane finds its own nearest bit on either side with a count of leading /
//                          trailing zeros. Reads and stores are coalesced: lanes take adjacent columns.
//   eu_edges_cols_kernel   pass 2: a thread per column, a wave per workgroup, so a wave reads 64 adjacent columns of a
//                          row at once and 64 columns already make a workgroup of their own. The lower envelope of the
//                          parabolas g(x, v)^2 + (y - v)^2 is a stack of (row, first row it rules); the stack of
//                          column x lives in column x of the two planes - row and start packed into a word of the
//                          distance plane, the row's g in the scratch plane, whose rows the sweep has read by then
//                          (entry q is written at row u >= q). The sweep back up turns the envelope into D and
//                          overwrites the stack from the far end: row u is written when entry q <= u is in registers.
//                          An 8192-column image is 128 waves: latency-bound, and accepted for load-time work.
#include <hip/hip_runtime.h>
#include "eu_edges.h"

#define EU_EDGES_NO_LEFT (-(1 << 20))    // "no outside column on this side": further than any column of a row
#define EU_EDGES_NO_RIGHT (1 << 21)
#define EU_EDGES_NONE (1 << 20)          // g of a row without an outside pixel is at least this

__global__ __launch_bounds__(256) void eu_edges_rows_kernel(const eu_edges_params p)
{
  __shared__ unsigned long long bits[EU_EDGES_MAX_SIDE / 64];
  __shared__ int lw[EU_EDGES_MAX_SIDE / 64], rw[EU_EDGES_MAX_SIDE / 64];
  const int y = blockIdx.x, w = p.w;
  const float *row = p.plane + ((size_t)y * p.pitch) * p.nch + (p.nch - 1);
  const int nwords = (w + 63) >> 6;
  for (int x0 = 0; x0 < nwords * 64; x0 += 256) {
    const int x = x0 + (int)threadIdx.x;
    bool outside = false;
    if (x < w) outside = !(row[(size_t)x * p.nch] > 0.0f);     // NaN, negative and zero alpha are outside
    const unsigned long long m = __ballot(outside);
    if ((threadIdx.x & 63) == 0 && x < nwords * 64) bits[x >> 6] = m;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    // per word: the last outside column in the words in front of it, the first in the words behind it
    for (int pass = 0, seed = EU_EDGES_NO_LEFT; pass < 2; pass++) {
      int carry = seed;
      for (int k = 0; k < nwords; k++) {
        lw[k] = carry;
        if (bits[k]) carry = k * 64 + 63 - __clzll((long long)bits[k]);
      }
      if (!p.cyclic || carry == seed) break;                   // (a row without an outside pixel: nothing to wrap)
      seed = carry - w;                                        // the row's last outside column, one turn back
    }
    for (int pass = 0, seed = EU_EDGES_NO_RIGHT; pass < 2; pass++) {
      int carry = seed;
      for (int k = nwords - 1; k >= 0; k--) {
        rw[k] = carry;
        if (bits[k]) carry = k * 64 + __ffsll((long long)bits[k]) - 1;
      }
      if (!p.cyclic || carry == seed) break;
      seed = carry + w;
    }
  }
  __syncthreads();
  int32_t *g = p.scratch + (size_t)y * w;
  for (int x = threadIdx.x; x < w; x += 256) {
    const int k = x >> 6, b = x & 63;
    const unsigned long long m = bits[k];
    const unsigned long long lo = m & (~0ull >> (63 - b)), hi = m & (~0ull << b);
    const int left = lo ? k * 64 + 63 - __clzll((long long)lo) : lw[k];
    const int right = hi ? k * 64 + __ffsll((long long)hi) - 1 : rw[k];
    g[x] = min(x - left, right - x);
  }
}

__global__ __launch_bounds__(64) void eu_edges_cols_kernel(const eu_edges_params p)
{
  const int x = blockIdx.x * 64 + threadIdx.x;
  if (x >= p.w) return;
  const size_t w = (size_t)p.w;
  const int h = p.h;
  int32_t *G = p.scratch + x;                                  // this column: rows w words apart
  uint32_t *S = reinterpret_cast<uint32_t *>(p.dist) + x;
  float *D = p.dist + x;
  // the top of the stack: its row, the first row it rules, its g^2
  int q = -1, ts = 0, tt = 0, tg2 = 0;
  int gn = G[0];
  for (int u = 0; u < h; u++) {
    const int gu = gn;
    if (u + 1 < h) gn = G[(size_t)(u + 1) * w];                // ahead of the stores below, which go to rows <= u
    if (gu >= EU_EDGES_NONE) continue;                         // no parabola in this row
    const int fu = gu * gu;
    while (q >= 0) {
      const int a = tt - ts, b = tt - u;
      if (!(a * a + tg2 > b * b + fu)) break;                  // (each sum is a squared distance: below 2^31)
      if (--q >= 0) {
        const uint32_t e = S[(size_t)q * w];
        const int gs = G[(size_t)q * w];
        ts = (int)(e & 0xffffu); tt = (int)(e >> 16); tg2 = gs * gs;
      }
    }
    if (q < 0) {
      q = 0; ts = u; tt = 0; tg2 = fu;
      S[0] = (uint32_t)u; G[0] = gu;
    } else {
      // the last row at which the top's parabola is not above u's: floor of the intersection
      const int num = (u * u - ts * ts) + (fu - tg2), den = 2 * (u - ts);
      int sep = num / den;
      if (num % den != 0 && num < 0) sep--;
      const int start = sep + 1;                               // > tt: the loop above left the top in rule at tt
      if (start < h) {
        q++; ts = u; tt = start; tg2 = fu;
        S[(size_t)q * w] = (uint32_t)u | ((uint32_t)start << 16);
        G[(size_t)q * w] = gu;
      }
    }
  }
  if (q < 0) {
    const float far = __builtin_sqrtf((float)EU_EDGES_FAR);
    for (int u = 0; u < h; u++) D[(size_t)u * w] = far;
    return;
  }
  for (int u = h - 1; u >= 0; u--) {
    const int d = u - ts;
    const int d2 = d * d + tg2;
    if (u == tt && q > 0) {                                    // the entry below rules from here: q - 1 < u, not yet overwritten
      q--;
      const uint32_t e = S[(size_t)q * w];
      const int gs = G[(size_t)q * w];
      ts = (int)(e & 0xffffu); tt = (int)(e >> 16); tg2 = gs * gs;
    }
    D[(size_t)u * w] = __builtin_sqrtf((float)d2);
  }
}

extern "C" int eu_launch_edges(const eu_edges_params *p, void *stream)
{
  if (!p->plane || !p->scratch || !p->dist || p->w < 1 || p->h < 1 || p->w > EU_EDGES_MAX_SIDE || p->h > EU_EDGES_MAX_SIDE ||
      p->nch < 1 || p->pitch < (size_t)p->w)
    return -2;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(eu_edges_rows_kernel, dim3((unsigned)p->h), dim3(256), 0, st, *p);
  hipLaunchKernelGGL(eu_edges_cols_kernel, dim3((unsigned)((p->w + 63) / 64)), dim3(64), 0, st, *p);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
