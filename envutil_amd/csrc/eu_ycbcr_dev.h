// Launch interface of eu_ycbcr.hip: the planes of a Y'CbCr frame to float pixels (include/eu_ycbcr.h).
#ifndef EU_YCBCR_DEV_H
#define EU_YCBCR_DEV_H

#include <stddef.h>
#include <stdint.h>

// All pointers are device memory.
struct eu_ycbcr_decode_params {
  const void *y, *cb, *cr;   // first sample of each plane; 16 bit: even addresses
  size_t y_pitch, c_pitch;   // BYTES between rows of the luma plane / of both chroma planes; 16 bit: even
  const float *tables;       // 1 << bits floats for luma, then 1 << bits floats for chroma
  float *dst;                // w x h pixels of nch floats, rows dst_pitch PIXELS apart
  size_t dst_pitch;
  int w, h;
  int nch;                   // 3, or 4: the new last channel is 1.0f
  int bits;                  // 8 or 16 (the device's byte order)
  int c_step;                // samples from one chroma sample to the next in a row: 1 or 2
  int sub_x, sub_y;          // 1 or 2 each: pixel (x, y) takes chroma sample (x / sub_x, y / sub_y)
  float m_rv, m_gu, m_gv, m_bu;
};

extern "C" int eu_launch_ycbcr_decode(const eu_ycbcr_decode_params *p, void *stream);

#endif
