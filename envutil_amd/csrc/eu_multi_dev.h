// Device functions of the multi-facet kernels, shared by eu_render_multi.hip (one job, eu_hip_render) and
// eu_render_views_multi.hip (many views of one job, eu_hip_render_views_multi): the steppers' rays per facet, the
// early-miss test, the three synopses and the register cap. A translation unit defines EU_MULTI_NCH before it
// includes this file to get the part its kernels are made of; the -DEU_MULTI_STAMPS build reads
// eu_multi_stamp_acc, which eu_render_multi.hip defines in front of its include.
#ifndef EU_MULTI_DEV_H
#define EU_MULTI_DEV_H
#include "eu_render_dev.h"
#include "eu_launch.h"

#define EU_MULTI_MAXF 64     // facets per job the mask-based alpha compositing takes (one bit each); beyond: eu_synopsis_big
#define EU_MULTI_KEEP 16     // facets whose coordinates are kept in LDS (3 KB each per workgroup)

// Early miss, second stage (round 3). The exact hit test of a facet costs ~300 vector instructions (two atan2f,
// sincosf in double, the lens polynomial, md_to_spline) and config 5 ran it 3.1 times per pixel: for every
// facet whose CORNER cone (rej_cos) holds the ray. The window is a square, two thirds of that cone. For a
// fisheye facet the planar coordinate is c = R(theta) * (rx, ry) / |(rx, ry)| + shift with R = theta * lens
// polynomial, and theta is a function of u = rz / |ray|: a table of a LOWER bound of R over bins of u (built
// on the host in double, 0.2 % below the smallest value of the bin and its neighbours) turns "c.x beyond the
// right edge" into a few approximate operations (rsq, one table read). Conservative by construction: a ray is
// dropped only when its coordinate lies beyond an edge moved OUT by 0.1 % of the window, far more than float
// rounding moves it; everything else takes the exact test as before. Header of a facet's table:
// [0] u0, [1] bins per unit of u, [2] 0 = no table, [4] [5] shift, [6]..[9] the edges x0 x1 y0 y1 moved out.
__device__ __forceinline__ bool eu_multi_maybe(const eu_multi_params &p, int f, const eu_src_dev &s, float rx, float ry, float rz)
{
  const float n2 = rx * rx + ry * ry, n3 = n2 + rz * rz;
  // stage one: the whole window lies inside a cone around the facet's axis
  bool maybe = !(rz < s.rej_cos * __builtin_amdgcn_sqrtf(n3));
  if (p.rej) {
    const float *tb = p.rej + (size_t)f * EU_REJ_STRIDE;         // f is wave-uniform: scalar loads
    if (tb[2] == 2.0f) {
      // no table: theta = acos(u) >= sqrt(2 t) (1 + t / 12 + 3 t^2 / 160), t = 1 - u (the series of acos in
      // sqrt(2 t), every term positive: cut off it is a lower bound, 0.13 % low at 65 degrees, 0.9 % at 92), and R is
      // increasing in theta (checked on the host), so R(bound) <= R(theta). Nothing is read per lane.
      const float t = 1.0f - rz * __builtin_amdgcn_rsqf(n3);
      const float th = __builtin_amdgcn_sqrtf(2.0f * t) * (1.0f + t * (0.083333f + t * 0.01875f));
      const float x = th * tb[10];
      const float lo = th * (tb[11] + x * (tb[12] + x * (tb[13] + x * tb[14])));          // 0.2 % folded into tb[11..14]
      const float ir = __builtin_amdgcn_rsqf(n2);
      const float a0 = lo * (rx * ir) + tb[4], a1 = lo * (ry * ir) + tb[5];
      const bool out = (rx >= 0.0f ? a0 > tb[7] : a0 < tb[6]) || (ry >= 0.0f ? a1 > tb[9] : a1 < tb[8]);
      maybe = maybe && !(out && t > 0.0f);
    } else if (tb[2] != 0.0f) {
      const float u = rz * __builtin_amdgcn_rsqf(n3);
      int k = (int)((u - tb[0]) * tb[1]);
      k = min(max(k, 0), EU_REJ_N - 1);
      const float lo = tb[EU_REJ_HDR + k];
      const float ir = __builtin_amdgcn_rsqf(n2);                 // (a ray on the axis: NaN below, no early miss)
      const float a0 = lo * (rx * ir) + tb[4], a1 = lo * (ry * ir) + tb[5];
      const bool out = (rx >= 0.0f ? a0 > tb[7] : a0 < tb[6]) || (ry >= 0.0f ? a1 > tb[9] : a1 < tb[8]);
      maybe = maybe && !out;
    }
  }
  return maybe;
}

struct eu_pix { int x, y; };

// ray of facet f for this pixel; variant 0: r00, 1: x-biased, 2: y-biased
template <bool GEN>
__device__ __forceinline__ void eu_multi_ray(const eu_multi_params &p, int f, int variant,
                                             const eu_pix &px, float &rx, float &ry, float &rz)
{
  const float *rowt = p.row + ((long long)f * p.height + eu_frame_row(px.y, p.band_shift, p.band_count, p.band_index)) * EU_ROW_FLOATS
                      + (variant == 2 ? EU_ROW_VARIANT : 0);
  const float *ca = variant == 1 ? p.col + 2 * p.width : p.col;
  if constexpr (GEN) {
    if (p.gen && p.gen[f].on) {             // f is wave-uniform
      // generic_stepper<float, LANES, true>: the ray is normalised (stepper.h:431-434)
      eu_stepper<true>(EU_FORM_GENERIC, EU_NORM_DIV, ca, ca, rowt, px.x, rx, ry, rz, &p.gen[f],
                       p.col + (variant == 1 ? 5 : 4) * (long long)p.width,
                       (p.inv.shear | p.inv.shift | p.inv.lcp) ? &p.inv : nullptr);
      return;
    }
  }
  eu_stepper<false>(p.form, p.norm_mode, ca, ca + p.width, rowt, px.x, rx, ry, rz);
}

// the ray the synopsis sees for facet f: the stepper's, or the twining tap's
// p0 + cx * du + cy * dv (payload.cc:669-675)
template <bool GEN>
__device__ __forceinline__ void eu_syn_ray(const eu_multi_params &p, int f, const eu_pix &px,
                                           bool tap, float cx, float cy, float &rx, float &ry,
                                           float &rz)
{
  eu_multi_ray<GEN>(p, f, 0, px, rx, ry, rz);
  if (tap) {
    float ax, ay, az, bx, by, bz;
    eu_multi_ray<GEN>(p, f, 1, px, ax, ay, az);
    eu_multi_ray<GEN>(p, f, 2, px, bx, by, bz);
    float dux = ax - rx, duy = ay - ry, duz = az - rz;
    float dvx = bx - rx, dvy = by - ry, dvz = bz - rz;
    rx = rx + cx * dux + cy * dvx;
    ry = ry + cx * duy + cy * dvy;
    rz = rz + cx * duz + cy * dvz;
  }
}

#ifdef EU_MULTI_NCH
#ifdef EU_MULTI_STAMPS
#define EU_MST(k) do { asm volatile("" ::: "memory"); mst_[k] = __builtin_amdgcn_s_memtime(); asm volatile("" ::: "memory"); } while (0)
#else
#define EU_MST(k) do { } while (0)
#endif
// per-thread slots in dynamic LDS: [z | sx | sy][facet][256 threads]
struct eu_slots {
  float *z, *sx, *sy;        // this thread's slot of facet 0; facets are 256 floats apart
  bool keep;                 // coordinates are stored (nfct <= EU_MULTI_KEEP)
};

// the facet's environment with channel adaption; a real call (one body per
// source channel count and degree, shared by all kernels of this file)
template <int SN, int DEG>
__device__ __noinline__ float4 eu_env_adapted(const eu_src_dev *s, int out_n, bool hit, float sx,
                                              float sy)
{
  float t[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
  eu_environment_repix_at<SN, DEG>(*s, out_n, hit, sx, sy, t);
  return make_float4(t[0], t[1], t[2], t[3]);
}

// facet f (wave-uniform) at this lane's source coordinate
template <int NCH, int DEG>
__device__ __forceinline__ void eu_env_facet(const eu_src_dev &s, bool hit, float sx, float sy,
                                             float *out)
{
  if (s.nch == NCH) {
    eu_environment_at<NCH, DEG>(s, hit, sx, sy, out);
  } else {
    // a facet with another channel count: repix_t inside its environment
    // object (environment.h:1846-1900); f is wave-uniform, so is this switch
    float4 t;
    switch (s.nch) {
      case 1: t = eu_env_adapted<1, DEG>(&s, NCH, hit, sx, sy); break;
      case 2: t = eu_env_adapted<2, DEG>(&s, NCH, hit, sx, sy); break;
      case 3: t = eu_env_adapted<3, DEG>(&s, NCH, hit, sx, sy); break;
      default: t = eu_env_adapted<4, DEG>(&s, NCH, hit, sx, sy); break;
    }
    const float tt[4] = { t.x, t.y, t.z, t.w };
#pragma unroll
    for (int c = 0; c < NCH; c++) out[c] = tt[c];
  }
}

// evaluate facet `want` (wave-divergent, -1: none) for this lane; hitm: the
// facets this lane's ray hits (bit per facet)
template <int NCH, int DEG, bool GEN>
__device__ __forceinline__ void eu_eval_facet(const eu_multi_params &p, int want, const eu_pix &px,
                                              bool tap, float cx, float cy, const eu_slots &sl,
                                              unsigned long long hitm, float *out)
{
#pragma unroll
  for (int c = 0; c < NCH; c++) out[c] = 0.0f;
  int pending = want;
  while (true) {
    unsigned long long m = __ballot(pending >= 0);
    if (!m) break;
    int first = __ffsll((long long)m) - 1;
    int f = __builtin_amdgcn_readlane(pending, first);
    if (pending == f) {
      const eu_src_dev &s = p.srcs[f];
      float sx, sy;
      bool hit;
      if (sl.keep && !s.mask_all) {
        sx = sl.sx[f * 256]; sy = sl.sy[f * 256];
        hit = (hitm >> f) & 1ull;
      } else {
        float rx, ry, rz;
        int face;
        eu_syn_ray<GEN>(p, f, px, tap, cx, cy, rx, ry, rz);
        hit = eu_source_coordinate(s, rx, ry, rz, sx, sy, face);
      }
      eu_env_facet<NCH, DEG>(s, hit, sx, sy, out);
      pending = -1;
    }
  }
}

// one synopsis evaluation for this lane
template <int NCH, int DEG, bool PLUS, bool GEN>
__device__ __forceinline__ void eu_synopsis(const eu_multi_params &p, const eu_pix &px,
                                            bool live, bool tap, float cx, float cy,
                                            const eu_slots &sl, float *out)
{
  const int nf = p.nfct;
  if constexpr (!PLUS) {
    // _voronoi_syn: get_mask + z score of every facet; the largest z wins,
    // strict '>' keeps the earlier facet. The champion's coordinate is kept.
    int champ = -1;
    float max_z = -3.402823466e+38f;          // numeric_limits<float>::lowest()
    float csx = 0.0f, csy = 0.0f;
    bool have = false;
#pragma unroll 1
    for (int f = 0; f < nf; f++) {
      float rx, ry, rz, sx = 0.0f, sy = 0.0f;
      int face;
      eu_syn_ray<GEN>(p, f, px, tap, cx, cy, rx, ry, rz);
      const eu_src_dev &s = p.srcs[f];
      const bool masked = !s.mask_all;        // wave-uniform
      bool hit = true;
      if (masked) {
        // whole wavefront provably outside the facet's window: skip the exact test
        const bool maybe = eu_multi_maybe(p, f, s, rx, ry, rz);
        hit = false;
        if (__ballot(maybe)) hit = eu_source_coordinate(s, rx, ry, rz, sx, sy, face);
      }
      const float z = rz * s.recip_step;
      if (hit && live && (f == 0 || z > max_z)) {
        // f == 0: the reference seeds champion and max_z with facet 0 where it is valid
        champ = f; max_z = z; csx = sx; csy = sy; have = masked;
      }
    }
    // evaluate the champion: waterfall over the facets the lanes chose
#pragma unroll
    for (int c = 0; c < NCH; c++) out[c] = 0.0f;
    int pending = champ;
    while (true) {
      unsigned long long m = __ballot(pending >= 0);
      if (!m) break;
      int first = __ffsll((long long)m) - 1;
      int f = __builtin_amdgcn_readlane(pending, first);
      if (pending == f) {
        const eu_src_dev &s = p.srcs[f];
        float sx = csx, sy = csy;
        bool hit = true;
        if (!have) {
          float rx, ry, rz;
          int face;
          eu_syn_ray<GEN>(p, f, px, tap, cx, cy, rx, ry, rz);
          hit = eu_source_coordinate(s, rx, ry, rz, sx, sy, face);
        }
        eu_env_facet<NCH, DEG>(s, hit, sx, sy, out);
        pending = -1;
      }
    }
    return;
  } else {
    const int lane = threadIdx.x & 63;
    const int grp = lane >> 4;
#ifdef EU_MULTI_STAMPS
    unsigned long long mst_[4];
    int nexact_ = 0;
#endif
    EU_MST(0);
    const unsigned long long live_m = __ballot(live);
    const unsigned live_g = (unsigned)(live_m >> (16 * grp)) & 0xffffu;
    unsigned long long valid = 0, hitm = 0;
    // next_best of this lane's vector: the last facet valid for any of its lanes
    int next_best = -1;
#pragma unroll 1
    for (int f = 0; f < nf; f++) {
      float rx, ry, rz, sx = 0.0f, sy = 0.0f;
      int face;
      eu_syn_ray<GEN>(p, f, px, tap, cx, cy, rx, ry, rz);
      const eu_src_dev &s = p.srcs[f];
      bool hit = true;
      if (!s.mask_all) {
        // whole wavefront provably outside the facet's window: skip the exact test
        const bool maybe = eu_multi_maybe(p, f, s, rx, ry, rz);
        hit = false;
        if (__ballot(maybe)) {
          hit = eu_source_coordinate(s, rx, ry, rz, sx, sy, face);
#ifdef EU_MULTI_STAMPS
          nexact_++;
#endif
        }
      }
      sl.z[f * 256] = rz * s.recip_step;
      if (sl.keep) { sl.sx[f * 256] = sx; sl.sy[f * 256] = sy; }
      if (hit) hitm |= 1ull << f;
      const bool v = hit && live;
      if (v) valid |= 1ull << f;
      const unsigned long long bm = __ballot(v);
      if ((unsigned)(bm >> (16 * grp)) & 0xffffu) next_best = f;
    }
    // the lane's nearest valid facet that is not used yet
    auto pick = [&](unsigned long long used) {
      int best = -1;
      float bz = 0.0f;
      unsigned long long todo = valid & ~used;
      while (todo) {
        const int f = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const float z = sl.z[f * 256];
        if (best < 0 || z > bz) { best = f; bz = z; }
      }
      return best;
    };
    EU_MST(1);
    const int top = pick(0ull);
#pragma unroll
    for (int c = 0; c < NCH; c++) out[c] = 0.0f;
    bool done = !live;
    if (next_best < 0) done = true;           // layers == 0 for this vector
    // "one facet on top of the whole vector" + "opaque everywhere": take it as is
    {
      unsigned long long tm = __ballot(live && top == next_best);
      bool all_top = !done && ((unsigned)(tm >> (16 * grp)) & 0xffffu) == live_g;
      float help[NCH];
      eu_eval_facet<NCH, DEG, GEN>(p, all_top ? next_best : -1, px, tap, cx, cy, sl, hitm, help);
      unsigned long long om = __ballot(all_top && help[NCH - 1] >= 1.0f);
      bool opaque = all_top && ((unsigned)(om >> (16 * grp)) & 0xffffu) == live_g;
      if (opaque) {
#pragma unroll
        for (int c = 0; c < NCH; c++) out[c] = help[c];
        done = true;
      }
    }
    EU_MST(2);
    // general path: composite the lane's valid facets, nearest first
    unsigned long long used = 0;
    int layer = 0;
    while (true) {
      int f = done ? -1 : pick(used);
      if (!__ballot(f >= 0)) break;
      float help[NCH];
      eu_eval_facet<NCH, DEG, GEN>(p, f, px, tap, cx, cy, sl, hitm, help);
      if (f >= 0) {
        used |= 1ull << f;
        if (layer == 0) {
#pragma unroll
          for (int c = 0; c < NCH; c++) out[c] = help[c];
        } else {
          const float a = out[NCH - 1];
#pragma unroll
          for (int c = 0; c < NCH; c++) out[c] = out[c] + (1.0f - a) * help[c];
        }
        layer++;
      }
    }
#ifdef EU_MULTI_STAMPS
    EU_MST(3);
    if (lane == 0) {
      unsigned long long *acc = eu_multi_stamp_acc + 4 * (blockIdx.x & 1023);
      atomicAdd(&acc[0], mst_[1] - mst_[0]);
      atomicAdd(&acc[1], mst_[2] - mst_[1]);
      atomicAdd(&acc[2], mst_[3] - mst_[2]);
      atomicAdd(&acc[3], 1ull + ((unsigned long long)nexact_ << 32));      // waves, exact hit tests (wave-level) above bit 32
    }
#endif
  }
}

// _voronoi_syn_plus for MORE facets than there are mask bits: nothing is kept per facet. A pass over all
// facets finds this lane's nearest valid facet BEHIND the layer composited last - (z, facet) smaller in
// the order the reference's layer list has (z descending, the earlier facet first among equals) - by
// recomputing every facet's ray, hit test and z score; one such pass per layer. Slow (facets x layers)
// and without limit; jobs of up to 64 facets use eu_synopsis.
template <int NCH, int DEG, bool GEN>
__device__ __forceinline__ void eu_synopsis_big(const eu_multi_params &p, const eu_pix &px, bool live,
                                                bool tap, float cx, float cy, const eu_slots &sl, float *out)
{
  const int nf = p.nfct;
  const int grp = (threadIdx.x & 63) >> 4;
  const unsigned live_g = (unsigned)(__ballot(live) >> (16 * grp)) & 0xffffu;
  // the nearest valid facet behind (lz, lf); first = true: the nearest of all. Also next_best of the
  // lane's vector: the last facet valid for any of its lanes
  int next_best = -1;
  auto pick = [&](bool first, float lz, int lf, float &bz) {
    int best = -1;
    bz = 0.0f;
#pragma unroll 1
    for (int f = 0; f < nf; f++) {
      float rx, ry, rz, sx = 0.0f, sy = 0.0f;
      int face;
      eu_syn_ray<GEN>(p, f, px, tap, cx, cy, rx, ry, rz);
      const eu_src_dev &s = p.srcs[f];
      bool hit = true;
      if (!s.mask_all) {
        const bool maybe = eu_multi_maybe(p, f, s, rx, ry, rz);
        hit = false;
        if (__ballot(maybe)) hit = eu_source_coordinate(s, rx, ry, rz, sx, sy, face);
      }
      const bool v = hit && live;
      if (first) {
        const unsigned long long bm = __ballot(v);
        if ((unsigned)(bm >> (16 * grp)) & 0xffffu) next_best = f;
      }
      const float z = rz * s.recip_step;
      const bool behind = first || z < lz || (z == lz && f > lf);
      if (v && behind && (best < 0 || z > bz)) { best = f; bz = z; }
    }
    return best;
  };
  float tz;
  const int top = pick(true, 0.0f, -1, tz);
#pragma unroll
  for (int c = 0; c < NCH; c++) out[c] = 0.0f;
  bool done = !live;
  if (next_best < 0) done = true;
  {
    unsigned long long tm = __ballot(live && top == next_best);
    bool all_top = !done && ((unsigned)(tm >> (16 * grp)) & 0xffffu) == live_g;
    float help[NCH];
    eu_eval_facet<NCH, DEG, GEN>(p, all_top ? next_best : -1, px, tap, cx, cy, sl, 0ull, help);
    unsigned long long om = __ballot(all_top && help[NCH - 1] >= 1.0f);
    bool opaque = all_top && ((unsigned)(om >> (16 * grp)) & 0xffffu) == live_g;
    if (opaque) {
#pragma unroll
      for (int c = 0; c < NCH; c++) out[c] = help[c];
      done = true;
    }
  }
  int f = done ? -1 : top;
  float fz = tz;
  int layer = 0;
  while (true) {
    if (!__ballot(f >= 0)) break;
    float help[NCH];
    eu_eval_facet<NCH, DEG, GEN>(p, f, px, tap, cx, cy, sl, 0ull, help);
    if (f >= 0) {
      if (layer == 0) {
#pragma unroll
        for (int c = 0; c < NCH; c++) out[c] = help[c];
      } else {
        const float a = out[NCH - 1];
#pragma unroll
        for (int c = 0; c < NCH; c++) out[c] = out[c] + (1.0f - a) * help[c];
      }
      layer++;
    }
    float nz;
    const int nxt = pick(false, fz, f >= 0 ? f : 0x7fffffff, nz);     // uniform control flow: every lane runs the pass
    if (f >= 0) { f = nxt; fz = nz; }
  }
}

// _hdr_merge_syn::get_quality for a grey value (envutil_payload.cc:1388-1446); kind 0 LOW, 1 MIDDLE, 2 HIGH
__device__ __forceinline__ float eu_hdr_quality(float grey, float optimum, int kind)
{
  const bool large = grey > optimum;
  float distance = fabsf(optimum - grey);
  if (kind == 0 && !large) distance = 0.0f;
  if (kind == 2 && large) distance = 0.0f;
  const float proximity = optimum - distance;
  return proximity / (optimum * optimum);
}
__device__ __forceinline__ float eu_std_max(float a, float b) { return a < b ? b : a; }

// _hdr_merge_syn::operator() (envutil_payload.cc:1500-1622): EVERY facet is evaluated - a miss is a
// zero pixel and takes part with the quality a zero pixel has -, quality-weighted sum, normalised.
// The one per-VECTOR decision (all_of(alpha == 0) -> quality 0) is a ballot over the lane's group of 16.
template <int NCH, int DEG, bool GEN>
__device__ __forceinline__ void eu_synopsis_hdr(const eu_multi_params &p, const eu_pix &px, bool live,
                                                bool tap, float cx, float cy, float *out)
{
  constexpr bool alpha = NCH == 2 || NCH == 4;
  constexpr int ncol = alpha ? NCH - 1 : NCH;
  const int grp = (threadIdx.x & 63) >> 4;
  const unsigned live_g = (unsigned)(__ballot(live) >> (16 * grp)) & 0xffffu;
  float qsum = 0.0f;
#pragma unroll
  for (int c = 0; c < NCH; c++) out[c] = 0.0f;
#pragma unroll 1
  for (int f = 0; f < p.nfct; f++) {
    float rx, ry, rz, sx = 0.0f, sy = 0.0f;
    int face;
    eu_syn_ray<GEN>(p, f, px, tap, cx, cy, rx, ry, rz);
    const eu_src_dev &s = p.srcs[f];
    bool hit = true, any = true;
    if (!s.mask_all) {
      // whole wavefront provably outside the facet's window: its pixel is zero without the exact test
      const bool maybe = eu_multi_maybe(p, f, s, rx, ry, rz);
      hit = false;
      any = __ballot(maybe) != 0;
      if (any) hit = eu_source_coordinate(s, rx, ry, rz, sx, sy, face);
    } else {
      hit = eu_source_coordinate(s, rx, ry, rz, sx, sy, face);
    }
    float v[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) v[c] = 0.0f;
    // a wavefront without a hit needs no gathers - unless the facet has another channel count: a miss
    // is then the ADAPTED zero pixel (repix_t gives it alpha 1)
    if (s.nch != NCH || (any && __ballot(hit))) eu_env_facet<NCH, DEG>(s, hit, sx, sy, v);
    const int kind = f == p.hdr_low ? 0 : (f == p.hdr_high ? 2 : 1);
    const float optimum = 0.5f * s.brighten;
    float grey;
    if constexpr (ncol == 1) grey = v[0];
    else grey = eu_std_max(v[0], eu_std_max(v[1], v[2]));
    float q = eu_hdr_quality(grey, optimum, kind);
    if constexpr (alpha) {
      const float a = v[NCH - 1];
      const unsigned zero_g = (unsigned)(__ballot(live && a == 0.0f) >> (16 * grp)) & 0xffffu;
      q = zero_g == live_g ? 0.0f : a * q;
    }
    qsum = qsum + q;
    if constexpr (!alpha) {
#pragma unroll
      for (int c = 0; c < NCH; c++) out[c] = out[c] + v[c] * q;
    } else {
      const float a = v[NCH - 1];
#pragma unroll
      for (int c = 0; c < ncol; c++) {
        float d = 0.0f;
        if (a > 0.000001f) d = v[c] / a;
        out[c] = out[c] + d * q;
      }
      out[NCH - 1] = eu_std_max(out[NCH - 1], a);
    }
  }
#pragma unroll
  for (int c = 0; c < ncol; c++) {
    float t = out[c] / qsum;
    if (!(qsum > 0.0f)) t = 0.0f;
    if constexpr (alpha) t = t * out[NCH - 1];
    out[c] = t;
  }
}

__device__ __forceinline__ float eu_std_min(float a, float b) { return b < a ? b : a; }

#define EU_FEATHER_FLOOR 0x1p-16f

// The edge weight e of a facet at a source coordinate, for eu_synopsis_feather and eu_synopsis_layers alike: the ramp
// towards the window's borders and - EDGES, for a facet that keeps a distance plane (EU_LOAD_EDGES; eu_hip.h has the
// definition) - towards the nearest pixel without alpha, a bilinear sample of the plane. The four loads happen under
// `hit` alone; a lane that misses gets a weight nobody reads. Without EDGES this is the code both loops had.
template <bool EDGES>
__device__ __forceinline__ float eu_feather_weight(const eu_feather_dev &w, bool hit, float sx, float sy)
{
  float e = 1.0f;
  if constexpr (!EDGES) {
    if (w.border) {
      const float dx = eu_std_min(sx + 0.5f, w.lim_x - sx), dy = eu_std_min(sy + 0.5f, w.lim_y - sy);
      const float d = w.border == 1 ? dx : (w.border == 2 ? dy : eu_std_min(dx, dy));
      e = d * w.rcp;
      e = e < EU_FEATHER_FLOOR ? EU_FEATHER_FLOOR : e;
      e = e > 1.0f ? 1.0f : e;
    }
  } else {
    const float *dist = w.dist;                 // wave-uniform, like everything in w
    if (w.border || dist) {
      float d = 0.0f;
      if (w.border) {
        const float dx = eu_std_min(sx + 0.5f, w.lim_x - sx), dy = eu_std_min(sy + 0.5f, w.lim_y - sy);
        d = w.border == 1 ? dx : (w.border == 2 ? dy : eu_std_min(dx, dy));
      }
      if (dist) {
        float dm = 0.0f;
        if (hit) {
          const float flx = floorf(sx), fly = floorf(sy);
          const float fx = sx - flx, fy = sy - fly;
          const int ix = (int)flx, iy = (int)fly;
          const int dw = w.dist_w, dh = w.dist_h;
          int x0, x1;
          if (w.cyclic) {
            x0 = ix % dw; x0 = x0 < 0 ? x0 + dw : x0;
            x1 = x0 + 1 == dw ? 0 : x0 + 1;
          } else {
            x0 = min(max(ix, 0), dw - 1);
            x1 = min(max(ix + 1, 0), dw - 1);
          }
          const int y0 = min(max(iy, 0), dh - 1), y1 = min(max(iy + 1, 0), dh - 1);
          const float *r0 = dist + (long long)y0 * dw, *r1 = dist + (long long)y1 * dw;
          const float d00 = r0[x0], d10 = r0[x1], d01 = r1[x0], d11 = r1[x1];
          const float top = d00 + (d10 - d00) * fx, bot = d01 + (d11 - d01) * fx;
          dm = (top + (bot - top) * fy) - 0.5f;
        }
        d = w.border ? eu_std_min(dm, d) : dm;
      }
      e = d * w.rcp;
      e = e < EU_FEATHER_FLOOR ? EU_FEATHER_FLOOR : e;
      e = e > 1.0f ? 1.0f : e;
    }
  }
  return e;
}

// Feathered seams. No counterpart in the reference: the definition is this project's own (DESIGN.md 1,
// tests/feather_model.py restates it in numpy). Every facet the ray HITS is weighted by its distance to the
// nearest border of the facet's window, a ramp of the job's width clamped to [2^-16, 1]; a miss contributes nothing
// at all (unlike eu_synopsis_hdr, where it is a zero pixel) - also for a facet of another channel count. With
// alpha the weight is alpha * ramp on the de-associated colour, as _hdr_merge_syn treats alpha. A pixel that one
// facet alone covers is that facet's pixel as it is, so where facets do not overlap the frame is eu_synopsis's.
// Per pixel, nothing per vector, nothing kept per facet: no limit on the facets, no dynamic LDS.
// Every operation is one of its own (-ffp-contract=off); the facets are walked in job order.
// EDGES: the job has a facet with a distance plane (eu_feather_weight); other jobs run the instantiation without.
template <int NCH, int DEG, bool GEN, bool EDGES>
__device__ __forceinline__ void eu_synopsis_feather(const eu_multi_params &p, const eu_pix &px,
                                                    bool tap, float cx, float cy, float *out)
{
  constexpr bool alpha = NCH == 2 || NCH == 4;
  constexpr int ncol = alpha ? NCH - 1 : NCH;
  float qsum = 0.0f, amax = 0.0f;
  float acc[ncol], one[NCH];
  int count = 0;
#pragma unroll
  for (int c = 0; c < ncol; c++) acc[c] = 0.0f;
#pragma unroll
  for (int c = 0; c < NCH; c++) one[c] = 0.0f;
#pragma unroll 1
  for (int f = 0; f < p.nfct; f++) {
    float rx, ry, rz, sx = 0.0f, sy = 0.0f;
    int face;
    eu_syn_ray<GEN>(p, f, px, tap, cx, cy, rx, ry, rz);
    const eu_src_dev &s = p.srcs[f];
    bool hit = false;
    if (!s.mask_all) {
      // whole wavefront provably outside the facet's window: no exact test
      if (__ballot(eu_multi_maybe(p, f, s, rx, ry, rz))) hit = eu_source_coordinate(s, rx, ry, rz, sx, sy, face);
    } else {
      hit = eu_source_coordinate(s, rx, ry, rz, sx, sy, face);
    }
    if (!__ballot(hit)) continue;               // a wavefront without a hit: no gathers
    float v[NCH];
    eu_env_facet<NCH, DEG>(s, hit, sx, sy, v);
    const float e = eu_feather_weight<EDGES>(p.fth[f], hit, sx, sy);        // f is wave-uniform: scalar loads
    if (hit) {
      float q = e;
      if constexpr (!alpha) {
#pragma unroll
        for (int c = 0; c < NCH; c++) acc[c] = acc[c] + v[c] * q;
      } else {
        const float a = v[NCH - 1];
        q = a * e;
#pragma unroll
        for (int c = 0; c < ncol; c++) {
          float dc = 0.0f;
          if (a > 0.000001f) dc = v[c] / a;
          acc[c] = acc[c] + dc * q;
        }
        amax = eu_std_max(amax, a);
      }
      qsum = qsum + q;
      if (count == 0) {
#pragma unroll
        for (int c = 0; c < NCH; c++) one[c] = v[c];
      }
      count++;
    }
  }
#pragma unroll
  for (int c = 0; c < ncol; c++) {
    float t = acc[c] / qsum;
    if (!(qsum > 0.0f)) t = 0.0f;
    if constexpr (alpha) t = t * amax;
    out[c] = count == 1 ? one[c] : t;           // (no facet: acc, qsum and `one` are zero)
  }
  if constexpr (alpha) out[NCH - 1] = count == 1 ? one[NCH - 1] : amax;
}

// The layer form of eu_synopsis_feather, stage A of the multi-band synopsis (EU_SYN_MULTIBAND, eu_multiband.hip):
// the same loop - ray, early miss, exact hit, eu_env_facet, ramp - but nothing is summed over the facets except
// qsum: per facet the colour X_f (de-associated with alpha; 0 where the weight is not positive) and the weight
// Q_f (0 on a miss) go to planes of the frame's size, p.lay_plane floats apart - facet f's ncol colour planes, then
// its Q - and behind all facets' the pixel's qsum, amax and count (as a float). Every plane is written for every
// live pixel, so the scratch needs no clearing. Whole frames only (no twining: the entry points refuse it).
template <int NCH, int DEG, bool GEN, bool EDGES>
__device__ __forceinline__ void eu_synopsis_layers(const eu_multi_params &p, const eu_pix &px, bool live)
{
  constexpr bool alpha = NCH == 2 || NCH == 4;
  constexpr int ncol = alpha ? NCH - 1 : NCH;
  float qsum = 0.0f, amax = 0.0f;
  int count = 0;
  const long long at = (long long)(px.y - p.row_begin) * p.width + px.x;
#pragma unroll 1
  for (int f = 0; f < p.nfct; f++) {
    float *lay = p.lay + (long long)f * (ncol + 1) * p.lay_plane + at;
    float rx, ry, rz, sx = 0.0f, sy = 0.0f;
    int face;
    eu_syn_ray<GEN>(p, f, px, false, 0.0f, 0.0f, rx, ry, rz);
    const eu_src_dev &s = p.srcs[f];
    bool hit = false;
    if (!s.mask_all) {
      if (__ballot(eu_multi_maybe(p, f, s, rx, ry, rz))) hit = eu_source_coordinate(s, rx, ry, rz, sx, sy, face);
    } else {
      hit = eu_source_coordinate(s, rx, ry, rz, sx, sy, face);
    }
    if (!__ballot(hit)) {                       // a wavefront without a hit: no gathers, empty layers
      if (live) {
#pragma unroll
        for (int c = 0; c <= ncol; c++) lay[c * p.lay_plane] = 0.0f;
      }
      continue;
    }
    float v[NCH];
    eu_env_facet<NCH, DEG>(s, hit, sx, sy, v);
    const float e = eu_feather_weight<EDGES>(p.fth[f], hit, sx, sy);        // f is wave-uniform: scalar loads
    float q = 0.0f, col[ncol];
#pragma unroll
    for (int c = 0; c < ncol; c++) col[c] = 0.0f;
    if (hit) {
      q = e;
      if constexpr (!alpha) {
#pragma unroll
        for (int c = 0; c < NCH; c++) col[c] = v[c];
      } else {
        const float a = v[NCH - 1];
        q = a * e;
#pragma unroll
        for (int c = 0; c < ncol; c++)
          if (a > 0.000001f) col[c] = v[c] / a;
        amax = eu_std_max(amax, a);
      }
      qsum = qsum + q;
      count++;
    }
    if (live) {
      const bool m = q > 0.0f;
#pragma unroll
      for (int c = 0; c < ncol; c++) lay[c * p.lay_plane] = m ? col[c] : 0.0f;
      lay[ncol * p.lay_plane] = q;
    }
  }
  if (live) {
    float *pix = p.lay + (long long)p.nfct * (ncol + 1) * p.lay_plane + at;
    pix[0] = qsum;
    pix[p.lay_plane] = amax;
    pix[2 * p.lay_plane] = (float)count;
  }
}

// The synopsis kernels are bound by the latency of their gathers (six 1-GB sources,
// little locality) more than by anything else: capping the registers for 5 waves per
// SIMD (a few spills) beats the 2-3 waves the allocator settles on by itself - config 5:
// 9.2 ms free, 8.0 at 4, 7.7 at 5, 8.8 at 6, 11.7 at 8 waves.
#ifndef EU_MULTI_WAVES
#define EU_MULTI_WAVES 5
#endif
#define EU_MULTI_OCC __attribute__((amdgpu_waves_per_eu(EU_MULTI_WAVES, EU_MULTI_WAVES)))

// The instantiation of a job, for both launchers: launch.go<DEG, SYN, GEN, BIG>(bytes of dynamic LDS) starts
// the launcher's own kernel (the view form has no generic stepper and maps GEN onto the one it has). SYN is the
// job's EU_MODE_*; hdr_merge and feather have the same set: degrees 0 to 3, the run-time degree, GEN.
template <bool PLUS, class L>
static int eu_multi_ladder(const eu_multi_params &p, int degree, const L &launch)
{
  const bool pano = p.mode == EU_MODE_PANORAMA;
  if (PLUS && pano && p.nfct > EU_MULTI_MAXF) {
    // the one instantiation serves jobs with and without generic-stepper facets
    if constexpr (PLUS) launch.template go<-1, EU_MODE_PANORAMA, true, true>(0);
    return hipGetLastError() == hipSuccess ? 0 : -1;
  }
  // alpha compositing keeps z (and, for up to EU_MULTI_KEEP facets, the source coordinate) of every facet per
  // thread in LDS
  const size_t lds = PLUS && pano ? (size_t)(p.nfct <= EU_MULTI_KEEP ? 3 : 1) * p.nfct * 256 * sizeof(float) : 0;
#define EU_LADDER_MODE(M)                                                            \
  if (p.gen) launch.template go<-1, M, true, false>(lds);                            \
  else switch (degree) {                                                             \
    case 0: launch.template go<0, M, false, false>(lds); break;                      \
    case 1: launch.template go<1, M, false, false>(lds); break;                      \
    case 2: launch.template go<2, M, false, false>(lds); break;                      \
    case 3: launch.template go<3, M, false, false>(lds); break;                      \
    default: launch.template go<-1, M, false, false>(lds); break;                    \
  }
  if (eu_mode_layers(p.mode)) {
    // stage A of the multi-band synopsis: the one-job launcher alone has it
    if (!L::layers || !p.fth || !p.lay || p.twine) return -2;
    if constexpr (L::layers) {
      if (p.mode == EU_MODE_LAYERS) { EU_LADDER_MODE(EU_MODE_LAYERS) }
      else { EU_LADDER_MODE(EU_MODE_LAYERS_EDGES) }
    }
  } else if (p.mode == EU_MODE_FEATHER) {
    if (!p.fth) return -2;
    EU_LADDER_MODE(EU_MODE_FEATHER)
  } else if (p.mode == EU_MODE_FEATHER_EDGES) {
    if (!p.fth) return -2;
    EU_LADDER_MODE(EU_MODE_FEATHER_EDGES)
  } else if (p.mode == EU_MODE_HDR) {
    EU_LADDER_MODE(EU_MODE_HDR)
  } else {
    EU_LADDER_MODE(EU_MODE_PANORAMA)
  }
#undef EU_LADDER_MODE
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

#endif  // EU_MULTI_NCH
#endif
