// Launch interface of eu_encode.hip: float pixels to 8- and 16-bit integer samples through step tables.
#ifndef EU_ENCODE_H
#define EU_ENCODE_H

#include <stddef.h>
#include <stdint.h>

// All pointers are device memory.
struct eu_encode_params {
  const float *src;          // w x h pixels of nch floats, rows src_stride_bytes apart (a multiple of 4)
  void *dst;                 // w x h pixels of nch samples, rows dst_stride_bytes apart; any byte address (16 bit: even)
  const float *tables;       // 2 << bits floats: the colour steps, then the steps of the alpha channel
  size_t src_stride_bytes, dst_stride_bytes;
  int w, h;
  int bits;                  // 8 or 16
  int big_endian;            // 16 bit: the high byte goes first
  int nch;                   // 1..4; the last of 2 or 4 reads the second table
};

extern "C" int eu_launch_encode(const eu_encode_params *p, void *stream);

#endif
