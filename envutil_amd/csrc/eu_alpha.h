// Launch interface of eu_alpha.hip: the device form of facet_alpha (PTO exclude masks and lens crops).
#ifndef EU_ALPHA_H
#define EU_ALPHA_H

#include <stddef.h>
#include <stdint.h>

// All pointers are device memory. The row plan is eu::facet_alpha_rows' (eu_imageprep.h).
struct eu_alpha_params {
  const float *src;          // w x h pixels of src_ch channels, rows src_pitch PIXELS apart; may be dst
  float *dst;                // w x h pixels of nch channels, rows dst_pitch pixels apart; NULL: the plane only
  float *alpha_out;          // w x h floats, dense; NULL: not wanted
  size_t src_pitch, dst_pitch;
  int w, h;
  int nch, src_ch;           // nch 2 or 4; src_ch == nch or nch - 1 (the new last channel is 1.0f * alpha)
  const int32_t *keep;       // 2 h: per row the columns [k0, k1) the crop keeps
  const int32_t *row_start;  // h + 1 offsets into spans
  const int32_t *spans;      // pairs [x0, x1) the polygons clear
};

#endif
