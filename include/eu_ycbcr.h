/* eu_ycbcr.h - the pixel functions of a Y'CbCr frame, in (here) and out (further down: eu_ycbcr_forward_pixel, the box
 * mean of the chroma, the step tables and the host loop eu_ycbcr_planes_rows). In: three floats Y, U, V (what the
 * caller's tables make of a luma and two chroma samples) to R, G, B through the four coefficients of the matrix. ONE
 * statement of it, for the host route (eu_hip_ycbcr_floats, the command line) and for the device route
 * (envutil_amd/csrc/eu_ycbcr.hip), so that the two cannot drift apart. Plain C and C++, host and device.
 *
 *   R = Y + m_rv * V        G = (Y + m_gu * U) + m_gv * V        B = Y + m_bu * U
 *
 * Every product and every sum is a float32 operation rounded on its own, in this order; a translation unit that
 * includes this header is built without contraction of a product and a sum into one operation (-ffp-contract=off).
 * Range, bit depth, bit alignment and the chroma offset are the tables' business; chroma is replicated: pixel (x, y)
 * takes chroma sample (x / sub_x, y / sub_y).
 *
 * eu_ycbcr_rows is the host loop over planes as a decoder lays them out - planar (c_step 1) or interleaved chroma
 * (c_step 2: NV12 with cr == cb + 1 sample, NV21 with cb == cr + 1 sample), 8-bit or 16-bit samples in host order,
 * rows `pitch` BYTES apart - into dense rows of nch floats (nch 4: alpha 1.0f). It reads the ceil(w / sub_x) x
 * ceil(h / sub_y) chroma samples of each plane and nothing else.
 */
#ifndef EU_YCBCR_H
#define EU_YCBCR_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define EU_YCBCR_FN __host__ __device__ __forceinline__
#else
#define EU_YCBCR_FN static inline
#endif

EU_YCBCR_FN void eu_ycbcr_pixel(float Y, float U, float V, float m_rv, float m_gu, float m_gv, float m_bu,
                                float *r, float *g, float *b)
{
  const float rv = m_rv * V, gu = m_gu * U, gv = m_gv * V, bu = m_bu * U;
  const float yg = Y + gu;
  *r = Y + rv;
  *g = yg + gv;
  *b = Y + bu;
}

/* sample number i of a row of 8- or 16-bit samples that starts at `row` (16 bit: an even address) */
static inline uint32_t eu_ycbcr_sample(const unsigned char *row, size_t i, int bits)
{
  if (bits == 8) return row[i];
  uint16_t v;
  memcpy(&v, row + 2 * i, sizeof v);
  return v;
}

static inline void eu_ycbcr_rows(const void *y, const void *cb, const void *cr, size_t y_pitch, size_t c_pitch,
                                 int c_step, int sub_x, int sub_y, int bits, const float *y_table,
                                 const float *c_table, float m_rv, float m_gu, float m_gv, float m_bu, int w, int h,
                                 int nch, float *out)
{
  for (int j = 0; j < h; j++) {
    const unsigned char *yr = (const unsigned char *)y + (size_t)j * y_pitch;
    const unsigned char *br = (const unsigned char *)cb + (size_t)(j / sub_y) * c_pitch;
    const unsigned char *rr = (const unsigned char *)cr + (size_t)(j / sub_y) * c_pitch;
    float *o = out + (size_t)j * (size_t)w * (size_t)nch;
    for (int i = 0; i < w; i++, o += nch) {
      const size_t ci = (size_t)(i / sub_x) * (size_t)c_step;
      const float Y = y_table[eu_ycbcr_sample(yr, (size_t)i, bits)];
      const float U = c_table[eu_ycbcr_sample(br, ci, bits)];
      const float V = c_table[eu_ycbcr_sample(rr, ci, bits)];
      eu_ycbcr_pixel(Y, U, V, m_rv, m_gu, m_gv, m_bu, &o[0], &o[1], &o[2]);
      if (nch == 4) o[3] = 1.0f;
    }
  }
}

/* ---- the way out: R, G, B to Y, U, V and on to the samples of the planes ------------------------------------------
 *
 *   Y = (k_r * R + k_g * G) + k_b * B        U = (B - Y) * c_u        V = (R - Y) * c_v
 *
 * Again every product and every sum is a float32 operation rounded on its own, in this order. The five coefficients
 * are the caller's (k_r, k_g, k_b the luma weights, c_u = 1 / (2 (1 - k_b)), c_v = 1 / (2 (1 - k_r))).
 *
 * Chroma subsampling is a box mean with the edge replicated: chroma sample (i, j) is made of the U (V) of the pixels
 * (min(sub_x i + a, w - 1), min(sub_y j + b, h - 1)), a < sub_x, b < sub_y, summed in this order (first index x):
 *   2 x 2: ((U00 + U10) + (U01 + U11)) * 0.25f     2 x 1: (U00 + U10) * 0.5f     1 x 2: (U00 + U01) * 0.5f     1 x 1: U
 *
 * A float becomes a code through a step table of 1 << bits floats with eu_encode's semantics (eu_hip.h): code(v) = the
 * number of k in 1 .. (1 << bits) - 1 with v >= steps[k]; a valid table has steps[1 .. m] free of NaN and
 * non-decreasing and NaN behind m, so a NaN is code 0 and +inf code m. The stored sample is the low `bits` bits of
 * code << shift (shift 0, or bits - depth for surfaces with the code in the high bits: P010 has 6). Range, depth and
 * the chroma offset are the tables' business.
 *
 * eu_ycbcr_planes_rows is the host loop into planes laid out as eu_ycbcr_rows reads them: planar (c_step 1) or
 * interleaved chroma (c_step 2, cr one sample before or behind cb), samples in host order, rows `pitch` BYTES apart.
 * It writes the w x h luma samples and the ceil(w / sub_x) x ceil(h / sub_y) samples of each chroma plane and no
 * other byte. `frame` holds rows of nch (3 or 4; alpha is ignored) floats, frame_stride BYTES apart.
 */
EU_YCBCR_FN void eu_ycbcr_forward_pixel(float R, float G, float B, float k_r, float k_g, float k_b, float c_u, float c_v,
                                        float *y, float *u, float *v)
{
  const float yr = k_r * R, yg = k_g * G, yb = k_b * B;
  const float yrg = yr + yg;
  const float Y = yrg + yb;
  const float bu = B - Y, rv = R - Y;
  *y = Y;
  *u = bu * c_u;
  *v = rv * c_v;
}

/* the number of k in 1 .. (1 << bits) - 1 with v >= steps[k], for a valid table */
static inline uint32_t eu_ycbcr_code(const float *steps, int bits, float v)
{
  uint32_t pos = 0;
  for (uint32_t step = (uint32_t)1 << (bits - 1); step > 0; step >>= 1)
    if (v >= steps[pos + step]) pos += step;
  return pos;
}

static inline void eu_ycbcr_store(unsigned char *row, size_t i, int bits, int shift, uint32_t code)
{
  if (bits == 8) row[i] = (unsigned char)(code << shift);
  else {
    const uint16_t v = (uint16_t)(code << shift);
    memcpy(row + 2 * i, &v, sizeof v);
  }
}

static inline void eu_ycbcr_planes_rows(const float *frame, size_t frame_stride, int w, int h, int nch, void *y,
                                        void *cb, void *cr, size_t y_pitch, size_t c_pitch, int c_step, int sub_x,
                                        int sub_y, int bits, int shift, const float *y_steps, const float *c_steps,
                                        float k_r, float k_g, float k_b, float c_u, float c_v)
{
  const int cw = (w + sub_x - 1) / sub_x, ch = (h + sub_y - 1) / sub_y;
  for (int j = 0; j < ch; j++) {
    unsigned char *br = (unsigned char *)cb + (size_t)j * c_pitch;
    unsigned char *rr = (unsigned char *)cr + (size_t)j * c_pitch;
    for (int i = 0; i < cw; i++) {
      float U[2][2], V[2][2];                                        /* [b][a]: row, column */
      for (int b = 0; b < sub_y; b++)
        for (int a = 0; a < sub_x; a++) {
          const int px = sub_x * i + a, py = sub_y * j + b;
          const int x = px < w ? px : w - 1, yy = py < h ? py : h - 1;
          const float *p = (const float *)((const char *)frame + (size_t)yy * frame_stride) + (size_t)x * (size_t)nch;
          float Y;
          eu_ycbcr_forward_pixel(p[0], p[1], p[2], k_r, k_g, k_b, c_u, c_v, &Y, &U[b][a], &V[b][a]);
          if (px < w && py < h)
            eu_ycbcr_store((unsigned char *)y + (size_t)py * y_pitch, (size_t)px, bits, shift, eu_ycbcr_code(y_steps, bits, Y));
        }
      float u = U[0][0], v = V[0][0];
      if (sub_x == 2 && sub_y == 2) {
        const float u0 = U[0][0] + U[0][1], u1 = U[1][0] + U[1][1], v0 = V[0][0] + V[0][1], v1 = V[1][0] + V[1][1];
        const float us = u0 + u1, vs = v0 + v1;
        u = us * 0.25f; v = vs * 0.25f;
      } else if (sub_x == 2) {
        const float us = U[0][0] + U[0][1], vs = V[0][0] + V[0][1];
        u = us * 0.5f; v = vs * 0.5f;
      } else if (sub_y == 2) {
        const float us = U[0][0] + U[1][0], vs = V[0][0] + V[1][0];
        u = us * 0.5f; v = vs * 0.5f;
      }
      eu_ycbcr_store(br, (size_t)i * (size_t)c_step, bits, shift, eu_ycbcr_code(c_steps, bits, u));
      eu_ycbcr_store(rr, (size_t)i * (size_t)c_step, bits, shift, eu_ycbcr_code(c_steps, bits, v));
    }
  }
}

#endif
