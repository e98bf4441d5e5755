// The planes of a Y'CbCr frame to float pixels on the way into a container (eu_hip_source_load_ycbcr,
// eu_hip_source_reload): a video decoder's surface - NV12 / P010 from the hardware decoder, I420 / I422 / I444 from
// software - read where it lies. The pixel function is eu_ycbcr_pixel of include/eu_ycbcr.h, the very one the host
// route (eu_hip_ycbcr_floats) calls: two tables say what a luma and a chroma sample become, four coefficients make
// R, G and B of them, every product and sum rounded on its own - the same bits by construction.
//
// ycbcr_decode_kernel follows decode_kernel (eu_decode.hip): one streaming pass in which a thread owns four
// consecutive FLOATS of a destination row and writes them with one 16-byte store; rows of the destination start at
// any float (the core of a braced container is offset by its frame), so per row thread 0 takes the 0..3 floats in
// front of the first 16-byte boundary with narrow stores, and the last thread of a row its ragged end. Four floats
// of 3 or 4 channels span at most two pixels, q0 and q0 + 1; the second is fetched and computed only where a float of
// the thread lies in it (never for an aligned four of 4 channels). Per plane the thread fetches the sample of q0 and,
// only where the sample of q0 + 1 is not in the same dword, that of q0 + 1: a luma
// sample is read once for all floats of its pixel, and the two pixels share their chroma fetch whenever they share
// the chroma sample (sub_x 2) or its dword. A fetch is the ALIGNED dword that holds the sample - planes are packed
// back to back and views into a decoder's buffer end where they end, so no access touches a dword without a byte
// of the plane's row. Neighbouring lanes load the same or adjacent dwords; they come from the same cache line.
//   8 bit:  both tables (2 x 1 KB) are copied to LDS once per workgroup, which then walks ROWS rows. A wave's
//           look-ups are ds_read_b32 at data-dependent addresses: equal samples broadcast, different ones on one
//           bank serialise - a quarter of the LDS reads of a kernel whose time is its stores.
//   16 bit: the tables (2 x 256 KB) stay in global memory, per-lane gathers that the L2 serves.
// Channel count and chroma layout (c_step) are template parameters; sub_x and sub_y are shifts.

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "../../include/eu_ycbcr.h"
#include "eu_ycbcr_dev.h"

namespace {

constexpr int NT = 256, ROWS = 8;

// the sample at `at` out of the aligned dword that holds it. `have` / `d`: the dword loaded last from this plane and
// its address - the next pixel's sample mostly lies in it, and then costs no load
template <int BITS>
__device__ __forceinline__ uint32_t fetch(const char *at, const uint32_t *&have, uint32_t &d)
{
  const uint32_t sh = uint32_t(reinterpret_cast<uintptr_t>(at) & 3);
  const uint32_t *a = reinterpret_cast<const uint32_t *>(at - sh);
  if (a != have) { d = *a; have = a; }
  return (d >> (8 * sh)) & ((1u << BITS) - 1u);
}

template <int BITS, int NCH, int CSTEP>
__global__ __launch_bounds__(NT) void ycbcr_decode_kernel(eu_ycbcr_decode_params p)
{
  constexpr int NTAB = 1 << BITS, BYTES = BITS / 8;
  __shared__ float lut[BITS == 8 ? 2 * NTAB : 1];
  if (BITS == 8) {
    for (int i = threadIdx.x; i < 2 * NTAB; i += NT) lut[i] = p.tables[i];
    __syncthreads();
  }
  const int rf = p.w * NCH;                                      // floats of a destination row
  const int t = blockIdx.x * NT + threadIdx.x;
  const int sx = p.sub_x - 1, sy = p.sub_y - 1;                  // 1 or 2: a shift by 0 or 1

  for (int yb = blockIdx.y * ROWS; yb < p.h; yb += gridDim.y * ROWS) {
    const int y1 = min(yb + ROWS, p.h);
    for (int y = yb; y < y1; y++) {
      float *drow = p.dst + size_t(y) * p.dst_pitch * NCH;
      // floats in front of the row's first 16-byte boundary: thread 0's; thread t > 0 takes the t-th aligned four
      const int head = (4 - int((reinterpret_cast<uintptr_t>(drow) >> 2) & 3)) & 3;
      const int j0 = t == 0 ? 0 : head + 4 * (t - 1);
      const int cnt = t == 0 ? min(head, rf) : min(4, rf - j0);
      if (cnt <= 0) continue;

      // float j0 + k is channel c of pixel q; pixels q0 and, where a float of the thread lies in it, q0 + 1
      const int q0 = j0 / NCH, c0 = j0 - q0 * NCH;
      const int q1 = (j0 + cnt - 1) / NCH > q0 ? q0 + 1 : q0;
      const char *yrow = static_cast<const char *>(p.y) + size_t(y) * p.y_pitch;
      const size_t coff = size_t(y >> sy) * p.c_pitch;
      const char *urow = static_cast<const char *>(p.cb) + coff, *vrow = static_cast<const char *>(p.cr) + coff;
      const float *tab = BITS == 8 ? lut : p.tables;
      const uint32_t *hy = nullptr, *hu = nullptr, *hv = nullptr;
      uint32_t dy = 0, du = 0, dv = 0;
      float ra, ga, ba;
      {
        const size_t co = size_t(q0 >> sx) * (CSTEP * BYTES);
        const uint32_t sy0 = fetch<BITS>(yrow + size_t(q0) * BYTES, hy, dy);
        const uint32_t su0 = fetch<BITS>(urow + co, hu, du), sv0 = fetch<BITS>(vrow + co, hv, dv);
        eu_ycbcr_pixel(tab[sy0], tab[NTAB + su0], tab[NTAB + sv0], p.m_rv, p.m_gu, p.m_gv, p.m_bu, &ra, &ga, &ba);
      }
      float rb = ra, gb = ga, bb = ba;
      if (q1 != q0) {                                            // a second pixel only where a float of the thread lies in it
        const size_t co = size_t(q1 >> sx) * (CSTEP * BYTES);
        const uint32_t sy1 = fetch<BITS>(yrow + size_t(q1) * BYTES, hy, dy);
        const uint32_t su1 = fetch<BITS>(urow + co, hu, du), sv1 = fetch<BITS>(vrow + co, hv, dv);
        eu_ycbcr_pixel(tab[sy1], tab[NTAB + su1], tab[NTAB + sv1], p.m_rv, p.m_gu, p.m_gv, p.m_bu, &rb, &gb, &bb);
      }

      float v[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const bool first = c0 + k < NCH;
        const int c = first ? c0 + k : c0 + k - NCH;
        const float r = first ? ra : rb, g = first ? ga : gb, b = first ? ba : bb;
        v[k] = c == 0 ? r : c == 1 ? g : c == 2 ? b : 1.0f;      // channel 3: the channel a facet gains
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

template <int BITS, int NCH>
void launch_step(const eu_ycbcr_decode_params &p, dim3 grid, hipStream_t st)
{
  if (p.c_step == 1) hipLaunchKernelGGL((ycbcr_decode_kernel<BITS, NCH, 1>), grid, dim3(NT), 0, st, p);
  else hipLaunchKernelGGL((ycbcr_decode_kernel<BITS, NCH, 2>), grid, dim3(NT), 0, st, p);
}

}  // namespace

extern "C" int eu_launch_ycbcr_decode(const eu_ycbcr_decode_params *pp, void *stream)
{
  const eu_ycbcr_decode_params &p = *pp;
  if (p.w <= 0 || p.h <= 0 || !p.y || !p.cb || !p.cr || !p.dst || !p.tables) return -1;
  if ((p.bits != 8 && p.bits != 16) || (p.nch != 3 && p.nch != 4)) return -1;
  if (p.c_step < 1 || p.c_step > 2 || p.sub_x < 1 || p.sub_x > 2 || p.sub_y < 1 || p.sub_y > 2) return -1;
  const size_t bytes = size_t(p.bits / 8), cw = (size_t(p.w) + p.sub_x - 1) / p.sub_x;
  if (p.y_pitch < size_t(p.w) * bytes || p.c_pitch < ((cw - 1) * p.c_step + 1) * bytes) return -1;
  if (p.bits == 16 && ((reinterpret_cast<uintptr_t>(p.y) | reinterpret_cast<uintptr_t>(p.cb) |
                        reinterpret_cast<uintptr_t>(p.cr) | p.y_pitch | p.c_pitch) & 1)) return -1;
  if (p.dst_pitch < size_t(p.w) || reinterpret_cast<uintptr_t>(p.dst) % 4) return -1;
  // the kernel counts the floats of a row in an int
  const size_t rf = size_t(p.w) * size_t(p.nch);
  if (rf > size_t(1) << 30) return -1;
  // a row has at most one head thread and ceil(rf / 4) more
  const size_t units = (rf + 3) / 4 + 1;
  const size_t gx = (units + NT - 1) / NT, gy = (size_t(p.h) + ROWS - 1) / ROWS;
  const dim3 grid((unsigned)gx, (unsigned)(gy < 65535u ? gy : 65535u));
  hipStream_t st = (hipStream_t)stream;
  if (p.bits == 8) { if (p.nch == 3) launch_step<8, 3>(p, grid, st); else launch_step<8, 4>(p, grid, st); }
  else { if (p.nch == 3) launch_step<16, 3>(p, grid, st); else launch_step<16, 4>(p, grid, st); }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
