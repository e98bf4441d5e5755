// Launch interface of eu_edges.hip: the distance plane of a source loaded with EU_LOAD_EDGES (include/eu_hip.h has the
// definition) - per window pixel the Euclidean distance to the nearest pixel whose alpha is not positive.
#ifndef EU_EDGES_H
#define EU_EDGES_H

#include <stddef.h>
#include <stdint.h>

#define EU_EDGES_MAX_SIDE 32768          // 2 * 32767^2 < 2^31: the squared distance is an exact int32
#define EU_EDGES_FAR 0x7fffffff          // D2 of a plane without an outside pixel

// All pointers are device memory.
struct eu_edges_params {
  const float *plane;        // w x h pixels of nch floats, alpha last, rows pitch PIXELS apart
  size_t pitch;
  int w, h, nch;
  int cyclic;                // the rows close: column w - 1 is column 0's neighbour
  int32_t *scratch;          // w x h: the row distances, then the columns' envelopes
  float *dist;               // w x h floats, dense: D
};

extern "C" int eu_launch_edges(const eu_edges_params *p, void *stream);

#endif
