// Radiance RGBE quads to float pixels on the way into a container (eu_hip_source_load_rgbe) and float pixels to
// quads on the way out (eu_hip_encode_rgbe, eu_hip_render_rgbe). The pixel functions are those of
// include/eu_rgbe.h, the very ones the file route calls on the host: built from bits, three exact multiplications
// each, no libm call and no division - the same bytes by construction. Neither pass touches a render kernel.
//
// rgbe_decode_kernel follows decode_kernel (eu_decode.hip): a thread owns four consecutive FLOATS of a destination
// row and writes them with one 16-byte store; rows of the destination start at any float (the core of a braced
// container is offset by its frame), so per row thread 0 takes the 0..3 floats in front of the first 16-byte
// boundary with narrow stores, and the last thread of a row its ragged end. A quad is one aligned dword and four
// floats span at most two pixels of 3 or 4 channels, so the source side is one or two dword loads; the second is
// made only when a float of the thread needs it, so no access leaves the image. A facet that gains its alpha
// channel here (3 -> 4) gets 1.0f in it. With a table (65536 floats indexed (E << 8) | mantissa, a facet whose
// colour space is not the working one) the float of a channel is a per-lane gather that the L2 serves, as for
// 16-bit samples; without one it is eu_rgbe_decode.
//
// rgbe_encode_kernel: a lane owns one pixel. It reads its three floats as ONE 12-byte load (global_load_dwordx3;
// rows are 4-byte aligned, which is all that instruction asks) - a wave's 64 pixels are 768 contiguous bytes, the
// read eu_rays2_kernel uses - and stores one dword: 16 bytes per pixel. There is no table.

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "../../include/eu_rgbe.h"
#include "eu_rgbe_dev.h"

namespace {

constexpr int NT = 256, ROWS = 8;

template <int NCH, bool TABLE>
__global__ __launch_bounds__(NT) void rgbe_decode_kernel(eu_rgbe_decode_params p)
{
  const int rf = p.w * NCH;                                      // floats of a destination row
  const int t = blockIdx.x * NT + threadIdx.x;

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
      const uint32_t *srow = p.src + size_t(y) * p.w;
      const uint32_t qa = srow[q0];
      uint32_t qb = 0;
      if ((j0 + cnt - 1) / NCH > q0) qb = srow[q0 + 1];

      float v[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int c = c0 + k < NCH ? c0 + k : c0 + k - NCH;
        const uint32_t quad = c0 + k < NCH ? qa : qb;
        v[k] = 1.0f;                                             // the channel a facet gains
        if (c < 3) {
          if (TABLE) {
            const uint32_t i = ((quad >> 24) << 8) | ((quad >> (8 * c)) & 0xffu);
            v[k] = k < cnt ? p.table[i] : 0.0f;
          } else {
            float f[3];
            eu_rgbe_decode(quad, &f[0], &f[1], &f[2]);
            v[k] = f[c];
          }
        }
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

typedef float eu_f3 __attribute__((ext_vector_type(3)));

__global__ __launch_bounds__(NT) void rgbe_encode_kernel(eu_rgbe_encode_params p)
{
  const int x = blockIdx.x * NT + threadIdx.x;
  if (x >= p.w) return;
  for (int yb = blockIdx.y * ROWS; yb < p.h; yb += gridDim.y * ROWS) {
    const int y1 = min(yb + ROWS, p.h);
    for (int y = yb; y < y1; y++) {
      const float *srow = reinterpret_cast<const float *>(reinterpret_cast<const char *>(p.src) + size_t(y) * p.src_stride_bytes);
      uint32_t *drow = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(p.dst) + size_t(y) * p.dst_stride_bytes);
      eu_f3 px;
      __builtin_memcpy(&px, srow + 3 * size_t(x), 12);
      drow[x] = eu_rgbe_encode(px.x, px.y, px.z);
    }
  }
}

}  // namespace

extern "C" int eu_launch_rgbe_decode(const eu_rgbe_decode_params *pp, void *stream)
{
  const eu_rgbe_decode_params &p = *pp;
  if (p.w <= 0 || p.h <= 0 || !p.src || !p.dst || (p.nch != 3 && p.nch != 4)) return -1;
  if (p.dst_pitch < size_t(p.w) || reinterpret_cast<uintptr_t>(p.dst) % 4 || reinterpret_cast<uintptr_t>(p.src) % 4) return -1;
  // the kernel counts the floats of a row in an int
  const size_t rf = size_t(p.w) * size_t(p.nch);
  if (rf > size_t(1) << 30) return -1;
  // a row has at most one head thread and ceil(rf / 4) more
  const size_t units = (rf + 3) / 4 + 1;
  const size_t gx = (units + NT - 1) / NT, gy = (size_t(p.h) + ROWS - 1) / ROWS;
  const dim3 grid((unsigned)gx, (unsigned)(gy < 65535u ? gy : 65535u));
  hipStream_t st = (hipStream_t)stream;
  if (p.nch == 3) {
    if (p.table) hipLaunchKernelGGL((rgbe_decode_kernel<3, true>), grid, dim3(NT), 0, st, p);
    else hipLaunchKernelGGL((rgbe_decode_kernel<3, false>), grid, dim3(NT), 0, st, p);
  } else {
    if (p.table) hipLaunchKernelGGL((rgbe_decode_kernel<4, true>), grid, dim3(NT), 0, st, p);
    else hipLaunchKernelGGL((rgbe_decode_kernel<4, false>), grid, dim3(NT), 0, st, p);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int eu_launch_rgbe_encode(const eu_rgbe_encode_params *pp, void *stream)
{
  const eu_rgbe_encode_params &p = *pp;
  if (p.w <= 0 || p.h <= 0 || !p.src || !p.dst) return -1;
  if (size_t(p.w) > size_t(1) << 28) return -1;
  if (p.src_stride_bytes < size_t(p.w) * 3 * sizeof(float) || p.src_stride_bytes % sizeof(float) || reinterpret_cast<uintptr_t>(p.src) % sizeof(float)) return -1;
  if (p.dst_stride_bytes < size_t(p.w) * 4 || p.dst_stride_bytes % 4 || reinterpret_cast<uintptr_t>(p.dst) % 4) return -1;
  const size_t gx = (size_t(p.w) + NT - 1) / NT, gy = (size_t(p.h) + ROWS - 1) / ROWS;
  const dim3 grid((unsigned)gx, (unsigned)(gy < 65535u ? gy : 65535u));
  hipLaunchKernelGGL(rgbe_encode_kernel, grid, dim3(NT), 0, (hipStream_t)stream, p);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
