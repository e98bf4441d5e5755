// Launch interface of eu_rgbe.hip: Radiance RGBE quads to float pixels and back (include/eu_rgbe.h).
#ifndef EU_RGBE_DEV_H
#define EU_RGBE_DEV_H

#include <stddef.h>
#include <stdint.h>

// All pointers are device memory.
struct eu_rgbe_decode_params {
  const uint32_t *src;       // w x h quads, rows dense; a 4-byte boundary
  float *dst;                // w x h pixels of nch floats, rows dst_pitch PIXELS apart
  const float *table;        // 65536 floats indexed (E << 8) | mantissa; nullptr: eu_rgbe_decode
  size_t dst_pitch;
  int w, h;
  int nch;                   // 3, or 4: the new last channel is 1.0f
};

struct eu_rgbe_encode_params {
  const float *src;          // w x h pixels of 3 floats, rows src_stride_bytes apart (a multiple of 4)
  uint32_t *dst;             // w x h quads, rows dst_stride_bytes apart (a multiple of 4); a 4-byte boundary
  size_t src_stride_bytes, dst_stride_bytes;
  int w, h;
};

extern "C" int eu_launch_rgbe_decode(const eu_rgbe_decode_params *p, void *stream);
extern "C" int eu_launch_rgbe_encode(const eu_rgbe_encode_params *p, void *stream);

#endif
