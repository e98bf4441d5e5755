/* eu_ycbcr.h - the pixel function of a Y'CbCr frame: three floats Y, U, V (what the caller's tables make of a luma
 * and two chroma samples) to R, G, B through the four coefficients of the matrix. ONE statement of it, for the host
 * route (eu_hip_ycbcr_floats, the command line) and for the device route (envutil_amd/csrc/eu_ycbcr.hip), so that
 * the two cannot drift apart. Plain C and C++, host and device.
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

#endif
