// Float pixels to integer samples: the encode of a rendered frame on its way out (eu_hip_encode_samples,
// eu_hip_render_samples), the mirror of eu_decode.hip. The code a float becomes is a non-decreasing step function
// of the float, so the host hands over the steps as a table of 1 << bits floats - found by bisection over the very
// expression its float route applies - and the device only compares: code(v) = the number of k in 1 .. (1 << bits)
// - 1 with v >= steps[k]. A valid table (the host checks it) has steps[1 .. m] free of NaN and non-decreasing and
// NaN behind m, so the predicate is true on a prefix of k and a branch-free binary search that adds a step whenever
// v >= steps[pos + step] gives exactly that count: a NaN pixel fails every compare and is code 0, no code above m is
// produced. No transcendental, no multiply, no rounding of the device's own.
// Two tables: one for the colour channels, one for the last of 2 or 4 channels (alpha takes no transfer curve).
//
// One streaming pass. A thread owns one ALIGNED DWORD of a destination row - four 8-bit or two 16-bit samples; with
// the channel count a template parameter the channel of each sample costs a constant division - and writes it with
// one store. Rows of the destination start at any byte (16 bit: any even byte) and may be padded, so per row thread 0
// takes the bytes in front of the row's first dword boundary, and the last thread of a row its ragged end, with byte
// or short stores: no store touches a byte outside the w * nch * bits / 8 bytes of a row. The floats that feed a
// dword are consecutive in the source row; they are read with one 16- (8-) byte load where that address is so
// aligned - the same for every dword of a row - and with dword loads otherwise.
//   8 bit:  both tables (2 x 1 KB) are copied to LDS once per workgroup, which then walks ROWS rows at a time;
//           eight compares per sample.
//   16 bit: the tables (2 x 256 KB) stay in global memory; every 16th entry of each (2 x 16 KB) goes to LDS and
//           serves the first twelve of the sixteen levels, the last four are per-lane gathers within one 64-byte
//           line. A launch has at most MAX_GROUPS workgroups, which walk the rows in strides, so that filling
//           the LDS stays a small part of the work.
// The device is little endian; big_endian swaps the bytes of a 16-bit code.

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "eu_encode.h"

namespace {

constexpr int NT = 256, ROWS = 8;
constexpr int TOP_SHIFT = 4, TOP = 65536 >> TOP_SHIFT;             // 16 bit: steps[k << TOP_SHIFT], k < TOP, in LDS
constexpr unsigned MAX_GROUPS = 4096;                              // workgroups of a launch: each fills its LDS once

template <int BITS, int NCH>
__global__ __launch_bounds__(NT) void encode_kernel(eu_encode_params p)
{
  constexpr int NTAB = 1 << BITS, BYTES = BITS / 8, SPT = 4 / BYTES;   // samples per dword
  constexpr bool ALPHA = NCH == 2 || NCH == 4;                     // the last channel reads the second table
  constexpr int NLDS = BITS == 8 ? NTAB : TOP;
  __shared__ float lut[2 * NLDS];
  for (int i = threadIdx.x; i < 2 * NLDS; i += NT)
    lut[i] = BITS == 8 ? p.tables[i] : p.tables[(i / TOP) * NTAB + ((i % TOP) << TOP_SHIFT)];
  __syncthreads();

  const int rb = p.w * NCH * BYTES;                                // bytes of a destination row
  const int t = blockIdx.x * NT + threadIdx.x;
  const bool swap = BITS == 16 && p.big_endian;

  for (int yb = blockIdx.y * ROWS; yb < p.h; yb += gridDim.y * ROWS) {
    const int y1 = min(yb + ROWS, p.h);
    for (int y = yb; y < y1; y++) {
      char *drow = static_cast<char *>(p.dst) + size_t(y) * p.dst_stride_bytes;
      const float *srow = reinterpret_cast<const float *>(reinterpret_cast<const char *>(p.src) + size_t(y) * p.src_stride_bytes);
      // bytes in front of the row's first dword boundary: thread 0's; thread t > 0 takes the t-th aligned dword
      const int head = int((0 - reinterpret_cast<uintptr_t>(drow)) & 3);
      const int b0 = t == 0 ? 0 : head + 4 * (t - 1);
      const int cnt = t == 0 ? min(head, rb) : min(4, rb - b0);
      if (cnt <= 0) continue;
      const int s0 = b0 / BYTES, ns = cnt / BYTES;                 // the samples [s0, s0 + ns) of the row

      float v[SPT];
      const float *f = srow + s0;
      if (ns == SPT && (reinterpret_cast<uintptr_t>(f) & (SPT * 4 - 1)) == 0) {
        if (BITS == 8) {
          const float4 q = *reinterpret_cast<const float4 *>(f);
          v[0] = q.x; v[1] = q.y; v[2 % SPT] = q.z; v[3 % SPT] = q.w;
        } else {
          const float2 q = *reinterpret_cast<const float2 *>(f);
          v[0] = q.x; v[1] = q.y;
        }
      } else {
#pragma unroll
        for (int k = 0; k < SPT; k++) v[k] = k < ns ? f[k] : 0.0f;
      }

      const int c0 = s0 % NCH;
      uint32_t c[SPT];
#pragma unroll
      for (int k = 0; k < SPT; k++) {
        const bool alpha = ALPHA && (c0 + k) % NCH == NCH - 1;
        const float *lt = lut + (alpha ? NLDS : 0);
        uint32_t pos = 0;
        if (BITS == 8) {
#pragma unroll
          for (int step = NTAB / 2; step > 0; step >>= 1) pos += v[k] >= lt[pos + step] ? step : 0;
        } else {
#pragma unroll
          for (int step = NTAB / 2; step >= 1 << TOP_SHIFT; step >>= 1) pos += v[k] >= lt[(pos + step) >> TOP_SHIFT] ? step : 0;
          const float *gt = p.tables + (alpha ? NTAB : 0);
#pragma unroll
          for (int step = (1 << TOP_SHIFT) / 2; step > 0; step >>= 1) pos += v[k] >= gt[pos + step] ? step : 0;
          if (swap) pos = ((pos & 0xffu) << 8) | (pos >> 8);
        }
        c[k] = pos;
      }

      char *d = drow + b0;
      if (t > 0 && cnt == 4) {
        uint32_t word;
        if (BITS == 8) word = c[0] | (c[1] << 8) | (c[2 % SPT] << 16) | (c[3 % SPT] << 24);
        else word = c[0] | (c[1] << 16);
        *reinterpret_cast<uint32_t *>(d) = word;
      } else if (BITS == 8) {
#pragma unroll
        for (int k = 0; k < 3; k++) if (k < cnt) reinterpret_cast<uint8_t *>(d)[k] = uint8_t(c[k % SPT]);
      } else {
        *reinterpret_cast<uint16_t *>(d) = uint16_t(c[0]);         // cnt == 2: the head or the end of a row of shorts
      }
    }
  }
}

template <int BITS>
void launch_bits(const eu_encode_params &p, dim3 grid, hipStream_t st)
{
  switch (p.nch) {
    case 1: hipLaunchKernelGGL((encode_kernel<BITS, 1>), grid, dim3(NT), 0, st, p); break;
    case 2: hipLaunchKernelGGL((encode_kernel<BITS, 2>), grid, dim3(NT), 0, st, p); break;
    case 3: hipLaunchKernelGGL((encode_kernel<BITS, 3>), grid, dim3(NT), 0, st, p); break;
    case 4: hipLaunchKernelGGL((encode_kernel<BITS, 4>), grid, dim3(NT), 0, st, p); break;
  }
}

}  // namespace

extern "C" int eu_launch_encode(const eu_encode_params *pp, void *stream)
{
  const eu_encode_params &p = *pp;
  if (p.w <= 0 || p.h <= 0 || !p.src || !p.dst || !p.tables || (p.bits != 8 && p.bits != 16)) return -1;
  if (p.nch < 1 || p.nch > 4) return -1;
  // the kernel counts the bytes of a row in an int, with room for the threads behind the row's end
  const size_t rf = size_t(p.w) * size_t(p.nch);
  if (rf > size_t(1) << 28) return -1;
  const size_t rb = rf * size_t(p.bits / 8);
  if (p.src_stride_bytes < rf * sizeof(float) || p.src_stride_bytes % sizeof(float) || reinterpret_cast<uintptr_t>(p.src) % sizeof(float)) return -1;
  if (p.dst_stride_bytes < rb) return -1;
  if (p.bits == 16 && (reinterpret_cast<uintptr_t>(p.dst) % 2 || p.dst_stride_bytes % 2)) return -1;
  // a row has at most one head thread and rb / 4 + 1 more (the dwords a row of rb bytes can touch behind its head)
  const size_t units = rb / 4 + 2;
  const size_t gx = (units + NT - 1) / NT, gy = (size_t(p.h) + ROWS - 1) / ROWS;
  const size_t gy_max = gx >= MAX_GROUPS ? 1 : MAX_GROUPS / gx;
  const dim3 grid((unsigned)gx, (unsigned)(gy < gy_max ? gy : gy_max));
  hipStream_t st = (hipStream_t)stream;
  if (p.bits == 8) launch_bits<8>(p, grid, st);
  else launch_bits<16>(p, grid, st);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
