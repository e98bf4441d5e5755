// Integer samples to float pixels: the decode of an 8- or 16-bit image on its way into a container
// (eu_hip_source_load_samples). The float a sample becomes is a function of its integer value alone, so
// the host hands over that function as a table of 1 << bits floats - made by the very expression its
// float route uses - and the device only looks it up: no arithmetic, the same bits by construction.
// Two tables: one for the colour channels, one for the last of 2 or 4 source channels (alpha takes no
// transfer curve). A facet that gains its alpha channel here (1 -> 2, 3 -> 4) gets 1.0f in it.
//
// One streaming pass. A thread owns four consecutive FLOATS of a destination row - not pixels: with the
// channel count a template parameter the channel and pixel of each float cost a constant division - and
// writes them with one 16-byte store. Rows of the destination start at any float (the core of a braced
// container is offset by its frame, its pitch is not the image's width), so per row thread 0 takes the
// 0..3 floats in front of the first 16-byte boundary with narrow stores, and the last thread of a row
// its ragged end. The up to four samples a thread needs are consecutive in the source row (the gained
// channel has no sample). Source rows are dense and start at every byte alignment (odd widths, three
// channels, views into a decoder's buffer), so the window of samples is fetched as the one to three
// ALIGNED dwords that hold it and shifted into place (v_alignbyte); a dword is loaded only if it holds a
// byte the thread needs, so no access touches a dword without a byte of the image. Neighbouring lanes
// load overlapping dwords; they come from the same cache line.
//   8 bit:  both tables (2 x 1 KB) are copied to LDS once per workgroup, which then walks ROWS rows.
//   16 bit: the tables (2 x 256 KB) stay in global memory, per-lane gathers that the L2 serves.
// The device is little endian; big_endian swaps the bytes of a 16-bit sample.

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "eu_decode.h"

namespace {

constexpr int NT = 256, ROWS = 8;

template <int BITS, int NCH, int SRC>
__global__ __launch_bounds__(NT) void decode_kernel(eu_decode_params p)
{
  constexpr int NTAB = 1 << BITS, BYTES = BITS / 8;
  constexpr bool ALPHA = SRC == NCH && (NCH == 2 || NCH == 4);   // the last source channel reads the second table
  __shared__ float lut[BITS == 8 ? 2 * NTAB : 1];
  if (BITS == 8) {
    for (int i = threadIdx.x; i < 2 * NTAB; i += NT) lut[i] = p.tables[i];
    __syncthreads();
  }
  const int rf = p.w * NCH;                                      // floats of a destination row
  const int t = blockIdx.x * NT + threadIdx.x;
  const size_t src_row_bytes = size_t(p.w) * SRC * BYTES;
  const bool swap = BITS == 16 && p.big_endian;

  for (int yb = blockIdx.y * ROWS; yb < p.h; yb += gridDim.y * ROWS) {
    const int y1 = min(yb + ROWS, p.h);
    for (int y = yb; y < y1; y++) {
      float *drow = p.dst + size_t(y) * p.dst_pitch * NCH;
      // floats in front of the row's first 16-byte boundary: thread 0's; thread t > 0 takes the t-th aligned four
      const int head = (4 - int((reinterpret_cast<uintptr_t>(drow) >> 2) & 3)) & 3;
      const int j0 = t == 0 ? 0 : head + 4 * (t - 1);
      const int cnt = t == 0 ? min(head, rf) : min(4, rf - j0);
      if (cnt <= 0) continue;

      // float j0 + k is channel c of pixel q; its sample, if it has one, is number q * SRC + c of the row
      const int q0 = j0 / NCH, c0 = j0 - q0 * NCH, base = q0 * SRC + c0;
      int delta[4], need = 0;
      bool has[4], alpha[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int j = j0 + k, q = j / NCH, c = j - q * NCH;
        has[k] = k < cnt && c < SRC;
        alpha[k] = ALPHA && c == NCH - 1;
        delta[k] = q * SRC + c - base;                           // 0..3 where has[k]
        if (has[k]) need = delta[k] + 1;
      }

      // the window of `need` samples from sample `base` on, out of the aligned dwords that hold it
      const uintptr_t b0 = reinterpret_cast<uintptr_t>(p.src) + size_t(y) * src_row_bytes + size_t(base) * BYTES;
      const uint32_t *a = reinterpret_cast<const uint32_t *>(b0 & ~uintptr_t(3));
      const int sh = int(b0 & 3), last = sh + need * BYTES;      // bytes [sh, last) of the dwords at a
      uint32_t d0 = 0, d1 = 0, d2 = 0;
      if (need > 0) d0 = a[0];
      if (last > 4) d1 = a[1];
      if (BITS == 16 && last > 8) d2 = a[2];
      const uint32_t w0 = __builtin_amdgcn_alignbyte(d1, d0, sh);
      const uint32_t w1 = BITS == 16 ? __builtin_amdgcn_alignbyte(d2, d1, sh) : 0u;

      float v[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        uint32_t s;
        if (BITS == 8) s = (w0 >> (8 * (delta[k] & 3))) & 0xffu;
        else {
          s = ((delta[k] & 2 ? w1 : w0) >> (16 * (delta[k] & 1))) & 0xffffu;
          if (swap) s = ((s & 0xffu) << 8) | (s >> 8);
        }
        const uint32_t i = s + (alpha[k] ? NTAB : 0);
        v[k] = 1.0f;                                             // the channel a facet gains
        if (has[k]) v[k] = BITS == 8 ? lut[i] : p.tables[i];
      }

      float *d = drow + j0;
      if (t > 0 && cnt == 4) *reinterpret_cast<float4 *>(d) = make_float4(v[0], v[1], v[2], v[3]);
      else {
#pragma unroll
        for (int k = 0; k < 3; k++) if (k < cnt) d[k] = v[k];
      }
    }
  }
}

template <int BITS, int NCH, int SRC>
void launch(const eu_decode_params &p, dim3 grid, hipStream_t st)
{
  hipLaunchKernelGGL((decode_kernel<BITS, NCH, SRC>), grid, dim3(NT), 0, st, p);
}

template <int BITS>
void launch_bits(const eu_decode_params &p, dim3 grid, hipStream_t st)
{
  switch (p.nch * 8 + p.src_ch) {
    case 1 * 8 + 1: launch<BITS, 1, 1>(p, grid, st); break;
    case 2 * 8 + 2: launch<BITS, 2, 2>(p, grid, st); break;
    case 3 * 8 + 3: launch<BITS, 3, 3>(p, grid, st); break;
    case 4 * 8 + 4: launch<BITS, 4, 4>(p, grid, st); break;
    case 2 * 8 + 1: launch<BITS, 2, 1>(p, grid, st); break;
    case 4 * 8 + 3: launch<BITS, 4, 3>(p, grid, st); break;
  }
}

}  // namespace

extern "C" int eu_launch_decode(const eu_decode_params *pp, void *stream)
{
  const eu_decode_params &p = *pp;
  if (p.w <= 0 || p.h <= 0 || !p.src || !p.dst || !p.tables || (p.bits != 8 && p.bits != 16)) return -1;
  if (p.nch < 1 || p.nch > 4 || p.src_ch < 1) return -1;
  if (p.src_ch != p.nch && !(p.src_ch == p.nch - 1 && (p.nch == 2 || p.nch == 4))) return -1;
  if (p.dst_pitch < size_t(p.w) || reinterpret_cast<uintptr_t>(p.dst) % 4) return -1;
  if (p.bits == 16 && reinterpret_cast<uintptr_t>(p.src) % 2) return -1;
  // the kernel counts the floats of a row in an int
  const size_t rf = size_t(p.w) * size_t(p.nch);
  if (rf > size_t(1) << 30) return -1;
  // a row has at most one head thread and ceil(rf / 4) more
  const size_t units = (rf + 3) / 4 + 1;
  const size_t gx = (units + NT - 1) / NT, gy = (size_t(p.h) + ROWS - 1) / ROWS;
  const dim3 grid((unsigned)gx, (unsigned)(gy < 65535u ? gy : 65535u));
  hipStream_t st = (hipStream_t)stream;
  if (p.bits == 8) launch_bits<8>(p, grid, st);
  else launch_bits<16>(p, grid, st);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
