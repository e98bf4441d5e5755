// Multi-band blending (EU_SYN_MULTIBAND, eu_hip_blend_layers): the levels of a job, the layout of its scratch and
// the launchers of eu_multiband.hip. The definition is in include/eu_hip.h (eu_target::bands); tests/multiband_model.py
// restates it in numpy. Host only.
//
// Everything is a dense float PLANE of its level's size. The scratch of a job of `nlay` layers with `ncol` colour
// channels on levels 0 .. L (S_l = w_l * h_l floats, T = S_0 + .. + S_L), in this order:
//   layers   nlay * (ncol + 1) * S_0    X_f per channel and Q_f, what stage A (or the prep kernel) writes
//   pixel    3 * S_0                    qsum, amax, count
//   facet    ncol * (T - S_0) + 2 * T   ONE facet's pyramids: X on levels 1 .. L, M and W on levels 0 .. L
//   sums     (ncol + 1) * T             num per channel and den, shared by the facets; the collapse runs in num
// The facets go through `facet` one after the other, in job order, so the scratch grows with the layers only by
// their level-0 planes.
#ifndef EU_MULTIBAND_H
#define EU_MULTIBAND_H
#include <hip/hip_runtime.h>
#include <cstddef>

#define EU_MB_MAXL 28          // more levels than any frame the library takes can have
#define EU_MB_DEFAULT 8        // bands = 0: min(L_max, 8)
#define EU_MB_MAXCOL 4         // colour channels of a plane set

struct eu_mb_geom {
  int L, wrap;
  int w[EU_MB_MAXL + 1], h[EU_MB_MAXL + 1];
  size_t off[EU_MB_MAXL + 2];  // off[l]: floats of the levels below l; off[L + 1] = T
};

// the levels of a w x h frame: L = bands clamped to L_max (the largest L with min(w_L, h_L) >= 4, and with wrap
// w % 2^L == 0), bands == 0: min(L_max, EU_MB_DEFAULT)
inline void eu_mb_levels(int w, int h, int bands, int wrap, eu_mb_geom *g)
{
  g->wrap = wrap;
  g->w[0] = w; g->h[0] = h; g->off[0] = 0;
  const int want = bands > 0 ? (bands < EU_MB_MAXL ? bands : EU_MB_MAXL) : EU_MB_DEFAULT;
  int L = 0;
  while (L < want) {
    const int w1 = (g->w[L] + 1) >> 1, h1 = (g->h[L] + 1) >> 1;
    if ((w1 < h1 ? w1 : h1) < 4) break;
    if (wrap && (w & ((1 << (L + 1)) - 1))) break;
    g->w[L + 1] = w1; g->h[L + 1] = h1;
    L++;
  }
  g->L = L;
  for (int l = 0; l <= L; l++) g->off[l + 1] = g->off[l] + (size_t)g->w[l] * g->h[l];
}

inline size_t eu_mb_scratch_floats(const eu_mb_geom &g, int ncol, int nlay)
{
  const size_t S0 = g.off[1], T = g.off[g.L + 1];
  return S0 * ((size_t)nlay * (ncol + 1) + 3) + (size_t)ncol * (T - S0) + 2 * T + (size_t)(ncol + 1) * T;
}

// plane c (c == ncol: Q) of layer f, and the three planes per pixel
inline float *eu_mb_layer(float *s, const eu_mb_geom &g, int ncol, int f, int c)
{
  return s + ((size_t)f * (ncol + 1) + c) * g.off[1];
}
inline float *eu_mb_pixel(float *s, const eu_mb_geom &g, int ncol, int nlay, int k)
{
  return s + ((size_t)nlay * (ncol + 1) + k) * g.off[1];
}

// where the frame goes: rows of `nch` interleaved floats, `stride` floats apart. alpha: nch == ncol + 1, the colour
// is multiplied by amax and the last channel is amax. count: pixels whose count is 0 are zeros (the render path).
struct eu_mb_out {
  float *out;
  long long stride;
  int nch, alpha, count;
};

// the caller's pictures into the layer planes: colour (N, H, W, C) and weight (N, H, W) with strides in floats
struct eu_mb_in {
  const float *colour, *weight;
  long long c_layer, c_row, w_layer, w_row;
};

// DIAGNOSTIC (tools/multiband_time.py): kernel time and nominal bytes moved per stage, summed over the launches of
// the jobs run while it is set - stage A, normalise, reduce, band, collapse (with the pixel kernel)
enum { EU_MB_T_STAGE_A = 0, EU_MB_T_NORMALISE = 1, EU_MB_T_REDUCE = 2, EU_MB_T_BAND = 3, EU_MB_T_COLLAPSE = 4, EU_MB_T_N = 5 };
struct eu_mb_times { double ms[EU_MB_T_N], bytes[EU_MB_T_N]; };

extern "C" {
// eu_hip_blend_layers' stage A: X_f = M_f ? colour : 0, Q_f = weight > 0 ? weight : 0, qsum in layer order
int eu_launch_mb_prep(float *scratch, const eu_mb_geom *g, int ncol, int nlay, const eu_mb_in *in, void *stream);
// everything behind stage A: per facet normalise, reduce, band; then the collapse into `o`
// times != nullptr: HIP events around every launch, and the stream is synchronised before the call returns
int eu_launch_mb_blend(float *scratch, const eu_mb_geom *g, int ncol, int nlay, const eu_mb_out *o, void *stream,
                       eu_mb_times *times);
}

#endif
