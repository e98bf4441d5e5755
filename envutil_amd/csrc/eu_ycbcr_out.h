// Launch interface of eu_ycbcr_out.hip: float pixels to the planes of a Y'CbCr frame through two step tables.
#ifndef EU_YCBCR_OUT_H
#define EU_YCBCR_OUT_H

#include <stddef.h>
#include <stdint.h>

// All pointers are device memory.
struct eu_ycbcr_encode_params {
  const float *src;          // w x h pixels of nch floats, rows src_stride_bytes apart (a multiple of 4)
  void *y, *cb, *cr;         // first sample of each plane; any byte address (16 bit: even)
  const float *tables;       // 2 << bits floats: the luma steps, then the chroma steps
  size_t src_stride_bytes, y_pitch, c_pitch;
  int w, h;
  int nch;                   // 3 or 4 (alpha is not read)
  int bits;                  // 8 or 16
  int shift;                 // the stored sample is the low `bits` bits of code << shift
  int sub_x, sub_y;          // 1 or 2 each
  int c_step;                // 1: planar; 2: interleaved, cr == cb + 1 sample or cb == cr + 1 sample
  float k_r, k_g, k_b, c_u, c_v;
};

extern "C" int eu_launch_ycbcr_encode(const eu_ycbcr_encode_params *p, void *stream);

#endif
