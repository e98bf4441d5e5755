// The direct-gather tile with its window rows fetched by lane quads (eu_render4.hip: eu4_direct_tile, degrees 2
// and 3). eu_eval2 lets a lane fetch its two pixels' windows itself - per pixel four rows of 48 contiguous bytes as
// three or four loads each, every one an L1 access of its own because the neighbouring lanes' windows lie elsewhere
// (around a pole tens of texels apart). Here the work is dealt twice:
//   phase 1  two pixels per lane, as in eu_eval2: gates (with their scalar fallbacks), split, weights, the window's
//            origin. What the taps need goes to a record of EU_QG_REC dwords per pixel in the wave's LDS area.
//   phase 2  four lanes per pixel, lane = (pixel | tap column i): one load instruction fetches a window row of 16
//            pixels, the texels of a row in adjacent lanes - 48 (64 with four channels) contiguous bytes per quad.
// The sums take the reference's terms in the reference's order (zimt/eval.h:904-1059, as eu_accumulate1 has them):
// per row and channel r = t0 * wx0; r = wx_i * t_i + r - the products formed in the lanes, the sum walked up the
// quad by row_shr:1 DPP operands - then sum = r0 * wy0; sum = r_j * wy_j + sum in the quad's last active lane.
// Addition commutes bit for bit, the order of the terms is kept. For order 3 the quad's fourth lane repeats the
// third lane's load and its products are never read.
#ifndef EU_QUAD_GATHER_H
#define EU_QUAD_GATHER_H

#include "eu_packed_dev.h"

#define EU_QG_REC 12        // dwords per pixel record: offset (2), flags, spare, wx[4], wy[4]
#define EU_QG_HIT 1         // flags: the pixel hits the source
#define EU_QG_VALID 2       //        the pixel lies in the frame

typedef float eu_qg_f4 __attribute__((ext_vector_type(4)));

// phase 1 for the lane's two pixels: the first half of eu_eval2, the records of pixels 2 * lane and 2 * lane + 1
template <int NCH, int DEG>
__device__ __forceinline__ void eu_qg_records(const eu_src_dev &s, eu_f2 sx, eu_f2 sy, eu_i2 hit, bool va, bool vb,
                                              float *rec, int lane)
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
  const eu_f2 tx = gx - fx, ty = gy - fy;
  constexpr int order = DEG + 1;
  eu_f2 wx[4], wy[4];
  wx[3] = wy[3] = (eu_f2){ 0.0f, 0.0f };
  eu_weights2<DEG>(s.wm, tx, wx);
  eu_weights2<DEG>(s.wm, ty, wy);
  static_assert(order == 3 || order == 4, "degrees 2 and 3");
  // a lane without a hit reads the window at the core origin (always inside the container, framed or not); its
  // result is discarded
  const int ixa = hit.x ? (int)fx.x : DEG / 2, iya = hit.x ? (int)fy.x : DEG / 2;
  const int ixb = hit.y ? (int)fx.y : DEG / 2, iyb = hit.y ? (int)fy.y : DEG / 2;
  const long long oa = (long long)(ixa - DEG / 2) * NCH + (long long)(iya - DEG / 2) * s.es1;
  const long long ob = (long long)(ixb - DEG / 2) * NCH + (long long)(iyb - DEG / 2) * s.es1;
  const int fa = (hit.x ? EU_QG_HIT : 0) | (va ? EU_QG_VALID : 0), fb = (hit.y ? EU_QG_HIT : 0) | (vb ? EU_QG_VALID : 0);
  eu_qg_f4 *r = (eu_qg_f4 *)(rec + 2 * lane * EU_QG_REC);
  r[0] = (eu_qg_f4){ __int_as_float((int)(unsigned)oa), __int_as_float((int)(oa >> 32)), __int_as_float(fa), 0.0f };
  r[1] = (eu_qg_f4){ wx[0].x, wx[1].x, wx[2].x, wx[3].x };
  r[2] = (eu_qg_f4){ wy[0].x, wy[1].x, wy[2].x, wy[3].x };
  r[3] = (eu_qg_f4){ __int_as_float((int)(unsigned)ob), __int_as_float((int)(ob >> 32)), __int_as_float(fb), 0.0f };
  r[4] = (eu_qg_f4){ wx[0].y, wx[1].y, wx[2].y, wx[3].y };
  r[5] = (eu_qg_f4){ wy[0].y, wy[1].y, wy[2].y, wy[3].y };
}

// the value of the lane one below in its row of 16 lanes (row_shr:1); the first lane of a row reads 0
__device__ __forceinline__ float eu_qg_below(float v)
{
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, false));
}

// phase 2 for pixel `pid` of the tile, in the four lanes that share it (i = lane & 3), in two halves so that the
// next pixel's loads can be issued in front of this pixel's sums: the record and the lane's column of the window ...
template <int NCH, int DEG>
struct eu_qg_taps {
  float t[DEG + 1][NCH];
  eu_qg_f4 wy;
  float wxi;
  int flags;
};

template <int NCH, int DEG>
__device__ __forceinline__ void eu_qg_fetch(const eu_src_dev &s, const float *rec, int pid, int i, eu_qg_taps<NCH, DEG> &w)
{
  constexpr int order = DEG + 1;
  const float *r = rec + pid * EU_QG_REC;
  const eu_qg_f4 head = *(const eu_qg_f4 *)r;
  w.wy = *(const eu_qg_f4 *)(r + 8);
  const int ic = i < order ? i : order - 1;
  w.wxi = r[4 + ic];
  const long long off = (long long)(((unsigned long long)(unsigned)__float_as_int(head.y) << 32) | (unsigned)__float_as_int(head.x));
  w.flags = __float_as_int(head.z);
  const float *p0 = s.base + off + ic * NCH;
#pragma unroll
  for (int j = 0; j < order; j++) {
    const float *q = p0 + j * s.es1;
#pragma unroll
    for (int c = 0; c < NCH; c++) w.t[j][c] = q[c];
  }
}

// ... and the sums. EXEC must be all ones. The pixel's value - brightened, zero on a miss - is valid in the lane
// with i == order - 1
template <int NCH, int DEG>
__device__ __forceinline__ void eu_qg_sum(const eu_src_dev &s, const eu_qg_taps<NCH, DEG> &w, float *px)
{
  constexpr int order = DEG + 1;
  const float (&t)[order][NCH] = w.t;
  const eu_qg_f4 wy = w.wy;
  const float wxi = w.wxi;
  const int flags = w.flags;
  float sum[NCH];
#pragma unroll
  for (int j = 0; j < order; j++) {
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      // lane i holds wx_i * t_i; lane k then t0 * wx0 + ... + wx_k * t_k, the terms added in that order
      const float p = wxi * t[j][c];
      float rsum = p;
#pragma unroll
      for (int k = 1; k < order; k++) rsum = p + eu_qg_below(rsum);
      if (j == 0) sum[c] = rsum * wy[0];
      else sum[c] = EU_MAD1(rsum, wy[j], sum[c]);
    }
  }
  // environment::eval brighten (environment.h:1821-1842), zero on a miss
  constexpr int ncol = (NCH == 2 || NCH == 4) ? NCH - 1 : NCH;
  const bool bright = s.brighten != 1.0f;
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    float v = sum[c];
    if (bright && c < ncol) v = v * s.brighten;
    px[c] = (flags & EU_QG_HIT) ? v : 0.0f;
  }
}

#endif
