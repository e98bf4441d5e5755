// Device form of facet_alpha (eu_imageprep.h; environment.h:700-890): the alpha plane of a masked or
// cropped facet - 1, cleared by the PTO exclude polygons and outside the lens crop, softened by the
// binomial (1 4 6 4 1) / 16 along both axes with REFLECT - multiplied into every channel of the image.
// One pass: every pixel is read once and written once.
//
// The host hands over the row plan (eu::facet_alpha_rows): per row the interval the crop keeps and the
// runs the polygons clear, integers only. A workgroup of 256 threads owns a tile of 64 x 16 pixels. It
//   0. fetches the tile's pixels into registers (their latency is covered by what follows);
//   1. builds the stage-0 alpha (0 / 1) of the tile and a halo of two from the plan into LDS; the
//      halo's indices are reflected as eu::reflect_index does, whatever the image's size;
//   2. runs the axis-0 binomial over the 20 rows the axis-1 pass needs, into a second LDS plane;
//   3. runs the axis-1 binomial from that plane, back into the first;
//   4. multiplies the pixels' channels by the result and stores them (and the plane, when asked).
// The order of the five products is zimt's circular buffer (eu::binomial_line / binomial_rows): at
// position t the first term is k = (-t) mod 5, then k + 1 ... cyclically, each sample * kf[k], summed
// left to right. Compiled with -ffp-contract=off. Samples are 0 or 1 and the weights k / 16, so every
// partial sum is a multiple of 1 / 256 and exact: the only rounding is the final pixel * alpha.

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "eu_alpha.h"
#include "eu_launch.h"

namespace {

constexpr int TW = 64, TH = 16, HALO = 2, NT = 256;
constexpr int AW = TW + 2 * HALO, AH = TH + 2 * HALO;

// zimt's REFLECT extrapolation (zimt/extrapolate.h:141-155), as eu::reflect_index
__device__ __forceinline__ int reflect_index(int i, int w)
{
  if (i < 0) i = -1 - i;
  if (i >= w) {
    i %= 2 * w;
    if (i >= w) i = 2 * w - 1 - i;
  }
  return i;
}

__device__ __forceinline__ float binomial5(const float *s, int stride, int t)
{
  const float kf[5] = { float(1.0 / 16.0), float(4.0 / 16.0), float(6.0 / 16.0), float(4.0 / 16.0),
                        float(1.0 / 16.0) };
  int k = (5 - t % 5) % 5;
  float r = s[k * stride] * kf[k];
#pragma unroll
  for (int j = 1; j < 5; j++) {
    k = k == 4 ? 0 : k + 1;
    r += s[k * stride] * kf[k];
  }
  return r;
}

// NCH: channels of the destination; SRC: of the source (NCH or NCH - 1, the new last channel is
// 1.0f * alpha); VEC: rows of both are 16-byte aligned for the wide accesses used below
template <int NCH, int SRC, bool VEC>
__global__ __launch_bounds__(NT) void facet_alpha_kernel(eu_alpha_params p)
{
  __shared__ float a0[AH * AW];     // stage 0 with halo; later the finished tile (TH x TW, stride TW)
  __shared__ float a1[AH * TW];     // after axis 0
  const int tid = threadIdx.x;
  const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
  const int w = p.w, h = p.h;

  // The thread's pixels are fetched first, so that their way from memory overlaps the work on the plane.
  // Two layouts: one pixel per lane and access (a wave reads a row of 64 pixels), or - two channels, aligned
  // rows - two pixels per lane, one 16-byte access. Either way a lane stores the pixels it loaded: in place is safe.
  constexpr bool PAIR = NCH == 2 && VEC;
  constexpr int LW = PAIR ? TW / 2 : TW;            // lanes across the tile
  constexpr int NP = TH * LW / NT;                  // accesses per thread
  constexpr int NV = PAIR ? 4 : NCH;                // floats per access
  float c[NP][NV];
  if (p.dst) {
#pragma unroll
    for (int j = 0; j < NP; j++) {
      const int i = tid + j * NT, ly = i / LW, lx = (PAIR ? 2 : 1) * (i - ly * LW);
      const int x = tx0 + lx, y = ty0 + ly;
#pragma unroll
      for (int k = 0; k < NV; k++) c[j][k] = 1.0f;  // the channel a facet gains is 1 before the edit
      if (x >= w || y >= h) continue;
      const float *s = p.src + (size_t(y) * p.src_pitch + size_t(x)) * SRC;
      if (PAIR) {
        if (SRC == 2 && x + 1 < w) {
          const float4 v = *reinterpret_cast<const float4 *>(s);
          c[j][0] = v.x; c[j][1] = v.y; c[j][2] = v.z; c[j][3] = v.w;
        } else {
          c[j][0] = s[0];
          if (SRC == 2) c[j][1] = s[1];
          else if (x + 1 < w) c[j][2] = s[1];
        }
      } else if (NCH == 4 && SRC == 4 && VEC) {
        const float4 v = *reinterpret_cast<const float4 *>(s);
        c[j][0] = v.x; c[j][1] = v.y; c[j][2] = v.z; c[j][3] = v.w;
      } else {
#pragma unroll
        for (int k = 0; k < SRC; k++) c[j][k] = s[k];
      }
    }
  }

  for (int i = tid; i < AH * AW; i += NT) {
    const int ly = i / AW, lx = i - ly * AW;
    const int gy = reflect_index(ty0 + ly - HALO, h), gx = reflect_index(tx0 + lx - HALO, w);
    float v = (gx >= p.keep[2 * gy] && gx < p.keep[2 * gy + 1]) ? 1.0f : 0.0f;
    const int s1 = p.row_start[gy + 1];
    for (int s = p.row_start[gy]; s < s1; s++)
      if (gx >= p.spans[2 * s] && gx < p.spans[2 * s + 1]) v = 0.0f;
    a0[i] = v;
  }
  __syncthreads();
  // axis 0: position t = x along the row; sample t - 2 + k sits at column lx + k of a0
  for (int i = tid; i < AH * TW; i += NT) {
    const int ly = i / TW, lx = i - ly * TW;
    a1[i] = binomial5(a0 + ly * AW + lx, 1, tx0 + lx);
  }
  __syncthreads();
  // axis 1: position t = y; the row t - 2 + k (reflected when a0 was built) is row ly + k of a1
  for (int i = tid; i < TH * TW; i += NT) {
    const int ly = i / TW, lx = i - ly * TW;
    a0[i] = binomial5(a1 + ly * TW + lx, TW, ty0 + ly);
  }
  __syncthreads();

  if (p.alpha_out)
    for (int i = tid; i < TH * TW; i += NT) {
      const int ly = i / TW, lx = i - ly * TW;
      const int x = tx0 + lx, y = ty0 + ly;
      if (x < w && y < h) p.alpha_out[size_t(y) * size_t(w) + size_t(x)] = a0[i];
    }
  if (!p.dst) return;

#pragma unroll
  for (int j = 0; j < NP; j++) {
    const int i = tid + j * NT, ly = i / LW, lx = (PAIR ? 2 : 1) * (i - ly * LW);
    const int x = tx0 + lx, y = ty0 + ly;
    if (x >= w || y >= h) continue;
    float *d = p.dst + (size_t(y) * p.dst_pitch + size_t(x)) * NCH;
    if (PAIR) {
      const float al0 = a0[ly * TW + lx], al1 = a0[ly * TW + lx + 1];
      const float r0 = c[j][0] * al0, r1 = c[j][1] * al0, r2 = c[j][2] * al1, r3 = c[j][3] * al1;
      if (x + 1 < w) *reinterpret_cast<float4 *>(d) = make_float4(r0, r1, r2, r3);
      else { d[0] = r0; d[1] = r1; }
    } else {
      const float al = a0[ly * TW + lx];
      float r[NV];
#pragma unroll
      for (int k = 0; k < NV; k++) r[k] = c[j][k] * al;
      if (NCH == 4 && VEC) {
        *reinterpret_cast<float4 *>(d) = make_float4(r[0], r[1], r[2], r[3]);
      } else {
#pragma unroll
        for (int k = 0; k < NV; k++) d[k] = r[k];
      }
    }
  }
}

template <int NCH, int SRC>
void launch(const eu_alpha_params &p, bool vec, dim3 grid, hipStream_t st)
{
  if (vec) hipLaunchKernelGGL((facet_alpha_kernel<NCH, SRC, true>), grid, dim3(NT), 0, st, p);
  else hipLaunchKernelGGL((facet_alpha_kernel<NCH, SRC, false>), grid, dim3(NT), 0, st, p);
}

}  // namespace

extern "C" int eu_launch_facet_alpha(const eu_alpha_params *pp, void *stream)
{
  const eu_alpha_params &p = *pp;
  if (p.w <= 0 || p.h <= 0 || (p.nch != 2 && p.nch != 4) || (p.src_ch != p.nch && p.src_ch != p.nch - 1)) return -1;
  if (!p.keep || !p.row_start || (!p.dst && !p.alpha_out) || (p.dst && !p.src)) return -1;
  if (p.dst && (p.src_pitch < size_t(p.w) || p.dst_pitch < size_t(p.w))) return -1;
  const size_t gx = (size_t(p.w) + TW - 1) / TW, gy = (size_t(p.h) + TH - 1) / TH;
  if (gy > 65535u) return -1;
  // the wide accesses need 16-byte aligned rows: the base and, in floats, pitch * channels a multiple of 4
  // (the source only where it is read wide, that is with as many channels as the destination)
  bool vec = p.dst && reinterpret_cast<uintptr_t>(p.dst) % 16 == 0 && (p.dst_pitch * size_t(p.nch)) % 4 == 0;
  if (vec && p.src_ch == p.nch)
    vec = reinterpret_cast<uintptr_t>(p.src) % 16 == 0 && (p.src_pitch * size_t(p.src_ch)) % 4 == 0;
  const dim3 grid((unsigned)gx, (unsigned)gy);
  hipStream_t st = (hipStream_t)stream;
  if (p.nch == 4 && p.src_ch == 4) launch<4, 4>(p, vec, grid, st);
  else if (p.nch == 4) launch<4, 3>(p, vec, grid, st);
  else if (p.src_ch == 2) launch<2, 2>(p, vec, grid, st);
  else launch<2, 1>(p, vec, grid, st);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
