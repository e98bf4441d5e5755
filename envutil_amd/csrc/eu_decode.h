// Launch interface of eu_decode.hip: 8- and 16-bit integer samples to float pixels through look-up tables.
#ifndef EU_DECODE_H
#define EU_DECODE_H

#include <stddef.h>
#include <stdint.h>

// All pointers are device memory.
struct eu_decode_params {
  const void *src;           // w x h pixels of src_ch samples, rows dense; any byte address (16 bit: even)
  float *dst;                // w x h pixels of nch floats, rows dst_pitch PIXELS apart
  const float *tables;       // 2 << bits floats: the colour table, then the table of the alpha channel
  size_t dst_pitch;
  int w, h;
  int bits;                  // 8 or 16
  int big_endian;            // 16 bit: the high byte comes first
  int nch, src_ch;           // src_ch == nch, or nch - 1 with nch 2 or 4 (the new last channel is 1.0f)
};

extern "C" int eu_launch_decode(const eu_decode_params *p, void *stream);

#endif
