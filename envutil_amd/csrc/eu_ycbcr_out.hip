// Float pixels to the planes of a Y'CbCr frame: the way out of a rendered frame towards a video encoder
// (eu_hip_encode_ycbcr, eu_hip_render_ycbcr), the mirror of eu_ycbcr.hip. The pixel function, the box mean of the
// chroma and the meaning of the step tables are those of include/eu_ycbcr.h (eu_ycbcr_forward_pixel and the comment
// above it); the host loop there and this kernel give the same bytes. The search is eu_encode.hip's, restated: a
// branch-free binary search that adds a step whenever v >= steps[pos + step], so a NaN is code 0.
//
// One streaming pass, shaped as encode_kernel is. A thread owns the pixels under one ALIGNED DWORD of a luma row -
// four 8-bit or two 16-bit samples - times SUB_Y rows. The dword boundaries are those of the first of the SUB_Y rows;
// thread 0 takes the bytes in front of that row's first boundary, the last thread of a row its ragged end. The
// thread reads its pixels' floats once (vector loads where the address allows), makes their luma codes and stores
// them - one dword per row where the row's own address is aligned, which with a pitch that is a multiple of 4 is every
// row, shorts or bytes otherwise - and keeps U and V for the chroma.
// A chroma sample belongs to the thread that owns its FIRST pixel (sub_x * i). With SUB_X 2 and a luma row that
// starts at an even pixel of a dword - every surface whose luma rows start on a 4-byte boundary - both pixels of a
// pair are the thread's own. Where a row starts at an odd byte the pairs straddle the dwords, and the thread reads
// the one pixel behind its own a second time (the same cache line); the last column of an odd width is its own
// partner (the edge is replicated), and so is the last row of an odd height.
// Chroma rows align on their own: the samples of a thread (2 or 4 bytes per plane, 4 or 8 interleaved) leave in
// dwords where their address is a multiple of 4, in shorts where it is even, in bytes otherwise. No store touches a
// byte outside the samples of a row of a plane.
//   8 bit:  both tables (2 x 1 KB) in LDS; eight compares per sample.
//   16 bit: every 16th entry of each table (2 x 16 KB) in LDS for twelve levels, the last four are per-lane gathers
//           within one 64-byte line of the table in global memory.
// A launch has at most MAX_GROUPS workgroups, which walk the rows in strides.

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "eu_ycbcr_out.h"
#include "../../include/eu_ycbcr.h"

namespace {

constexpr int NT = 256, ROWS = 8;
constexpr int TOP_SHIFT = 4, TOP = 65536 >> TOP_SHIFT;             // 16 bit: steps[k << TOP_SHIFT], k < TOP, in LDS
constexpr unsigned MAX_GROUPS = 4096;                              // workgroups of a launch: each fills its LDS once

// code(v): lt is the table's part in LDS, gt the whole table in global memory (16 bit only)
template <int BITS>
__device__ __forceinline__ uint32_t code_of(float v, const float *lt, const float *gt)
{
  constexpr int NTAB = 1 << BITS;
  uint32_t pos = 0;
  if (BITS == 8) {
#pragma unroll
    for (int step = NTAB / 2; step > 0; step >>= 1) pos += v >= lt[pos + step] ? step : 0;
  } else {
#pragma unroll
    for (int step = NTAB / 2; step >= 1 << TOP_SHIFT; step >>= 1) pos += v >= lt[(pos + step) >> TOP_SHIFT] ? step : 0;
#pragma unroll
    for (int step = (1 << TOP_SHIFT) / 2; step > 0; step >>= 1) pos += v >= gt[pos + step] ? step : 0;
  }
  return pos;
}

// the n <= MAXB bytes of `bits` (low byte first) to d .. d + n: dwords where d is a multiple of 4, shorts where it is
// even, bytes for the rest - and no byte outside [d, d + n)
template <int MAXB, bool BYTES_TOO>
__device__ __forceinline__ void store_run(char *d, uint64_t bits, int n)
{
  const uintptr_t a = reinterpret_cast<uintptr_t>(d);
  const bool w4 = (a & 3) == 0, w2 = (a & 1) == 0;
#pragma unroll
  for (int k = 0; k + 4 <= MAXB; k += 4)
    if (w4 && k + 4 <= n) *reinterpret_cast<uint32_t *>(d + k) = uint32_t(bits >> (8 * k));
  const int o4 = w4 ? (n & ~3) : 0;
#pragma unroll
  for (int k = 0; k + 2 <= MAXB; k += 2)
    if (w2 && k >= o4 && k + 2 <= n) *reinterpret_cast<uint16_t *>(d + k) = uint16_t(bits >> (8 * k));
  if (BYTES_TOO) {
    const int o2 = w2 ? (n & ~1) : 0;
#pragma unroll
    for (int k = 0; k < MAXB; k++)
      if (k >= o2 && k < n) *reinterpret_cast<uint8_t *>(d + k) = uint8_t(bits >> (8 * k));
  }
}

// One row of a thread: the pixels [x0, x0 + n) of the row at srow, n <= PPT, and with `extra` the pixel behind them.
// Slot k stands for pixel min(x0 + k, w - 1). Stores the luma samples at drow + x0 samples when drow is not null;
// hu / hv receive, per chroma sample of the thread, the sum over the sample's pixels of this row.
template <int BITS, int NCH, int SUB_X>
__device__ __forceinline__ void row_of(const eu_ycbcr_encode_params &p, const float *srow, char *drow, int x0, int n,
                                       bool extra, const float *lt, float *hu, float *hv)
{
  constexpr int BYTES = BITS / 8, PPT = 4 / BYTES, NF = PPT * NCH, NC = SUB_X == 2 ? PPT / 2 : PPT;
  float f[(PPT + 1) * NCH];
  const float *src = srow + size_t(x0) * NCH;
  const uintptr_t sa = reinterpret_cast<uintptr_t>(src);
  if (n == PPT && NF % 4 == 0 && (sa & 15) == 0) {
#pragma unroll
    for (int k = 0; k < NF / 4; k++) {
      const float4 q = reinterpret_cast<const float4 *>(src)[k];
      f[4 * k] = q.x; f[4 * k + 1] = q.y; f[4 * k + 2] = q.z; f[4 * k + 3] = q.w;
    }
  } else if (n == PPT && (sa & 7) == 0) {
#pragma unroll
    for (int k = 0; k < NF / 2; k++) {
      const float2 q = reinterpret_cast<const float2 *>(src)[k];
      f[2 * k] = q.x; f[2 * k + 1] = q.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < PPT; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) f[k * NCH + c] = k < n ? src[k * NCH + c] : 0.0f;
  }
  if (SUB_X == 2) {
    // the partner of the thread's last pixel: slot n, the pixel itself at the end of an odd row
#pragma unroll
    for (int k = 1; k <= PPT; k++) {
      if (k == n && extra) {
        const float *e = srow + size_t(min(x0 + k, p.w - 1)) * NCH;
#pragma unroll
        for (int c = 0; c < 3; c++) f[k * NCH + c] = e[c];
      } else if (k == PPT) {
#pragma unroll
        for (int c = 0; c < 3; c++) f[k * NCH + c] = 0.0f;
      }
    }
  }

  float Y[PPT + 1], U[PPT + 1], V[PPT + 1];
#pragma unroll
  for (int k = 0; k < (SUB_X == 2 ? PPT + 1 : PPT); k++)
    eu_ycbcr_forward_pixel(f[k * NCH], f[k * NCH + 1], f[k * NCH + 2], p.k_r, p.k_g, p.k_b, p.c_u, p.c_v, &Y[k], &U[k], &V[k]);

  if (drow) {
    uint64_t bits = 0;
#pragma unroll
    for (int k = 0; k < PPT; k++) {
      const uint32_t c = (code_of<BITS>(Y[k], lt, p.tables) << p.shift) & ((1u << BITS) - 1u);
      bits |= uint64_t(c) << (k * BITS);
    }
    store_run<4, BITS == 8>(drow + size_t(x0) * BYTES, bits, n * BYTES);
  }

  if (SUB_X == 2) {
    const bool odd = x0 & 1;                                       // the thread's pairs start at slots odd, odd + 2
#pragma unroll
    for (int s = 0; s < NC; s++) {
      const float ua = odd ? U[2 * s + 1] : U[2 * s], ub = odd ? U[2 * s + 2] : U[2 * s + 1];
      const float va = odd ? V[2 * s + 1] : V[2 * s], vb = odd ? V[2 * s + 2] : V[2 * s + 1];
      hu[s] = ua + ub;
      hv[s] = va + vb;
    }
  } else {
#pragma unroll
    for (int s = 0; s < NC; s++) { hu[s] = U[s]; hv[s] = V[s]; }
  }
}

template <int BITS, int NCH, int SUB_X, int SUB_Y, bool INTERLEAVED>
__global__ __launch_bounds__(NT) void ycbcr_encode_kernel(eu_ycbcr_encode_params p)
{
  constexpr int NTAB = 1 << BITS, BYTES = BITS / 8, PPT = 4 / BYTES, NC = SUB_X == 2 ? PPT / 2 : PPT;
  constexpr int NLDS = BITS == 8 ? NTAB : TOP;
  __shared__ float lut[2 * NLDS];
  for (int i = threadIdx.x; i < 2 * NLDS; i += NT)
    lut[i] = BITS == 8 ? p.tables[i] : p.tables[(i / TOP) * NTAB + ((i % TOP) << TOP_SHIFT)];
  __syncthreads();

  const int rb = p.w * BYTES;                                      // bytes of a luma row
  const int t = blockIdx.x * NT + threadIdx.x;
  const int ng = (p.h + SUB_Y - 1) / SUB_Y;                        // groups of SUB_Y rows = chroma rows
  // interleaved chroma: one plane of pairs that starts at the lower of cb and cr
  const bool v_first = INTERLEAVED && reinterpret_cast<uintptr_t>(p.cr) < reinterpret_cast<uintptr_t>(p.cb);

  for (int gb = blockIdx.y * ROWS; gb < ng; gb += gridDim.y * ROWS) {
    const int g1 = min(gb + ROWS, ng);
    for (int g = gb; g < g1; g++) {
      const int r0 = g * SUB_Y;
      char *drow = static_cast<char *>(p.y) + size_t(r0) * p.y_pitch;
      const float *srow = reinterpret_cast<const float *>(reinterpret_cast<const char *>(p.src) + size_t(r0) * p.src_stride_bytes);
      // bytes in front of the row's first dword boundary: thread 0's; thread t > 0 takes the t-th aligned dword
      const int head = int((0 - reinterpret_cast<uintptr_t>(drow)) & 3);
      const int b0 = t == 0 ? 0 : head + 4 * (t - 1);
      const int cnt = t == 0 ? min(head, rb) : min(4, rb - b0);
      if (cnt <= 0) continue;
      const int x0 = b0 / BYTES, n = cnt / BYTES;                  // the pixels [x0, x0 + n) of the row
      const bool extra = SUB_X == 2 && ((x0 + n) & 1);             // the last of them starts a pair

      float hu[NC], hv[NC];
      row_of<BITS, NCH, SUB_X>(p, srow, drow, x0, n, extra, lut, hu, hv);
      if (SUB_Y == 2) {
        float hu1[NC], hv1[NC];
        if (r0 + 1 < p.h) {
          const float *srow1 = reinterpret_cast<const float *>(reinterpret_cast<const char *>(srow) + p.src_stride_bytes);
          row_of<BITS, NCH, SUB_X>(p, srow1, drow + p.y_pitch, x0, n, extra, lut, hu1, hv1);
        } else {
#pragma unroll
          for (int s = 0; s < NC; s++) { hu1[s] = hu[s]; hv1[s] = hv[s]; }
        }
#pragma unroll
        for (int s = 0; s < NC; s++) { hu[s] = hu[s] + hu1[s]; hv[s] = hv[s] + hv1[s]; }
      }
      constexpr float MEAN = 1.0f / float(SUB_X * SUB_Y);

      // the chroma samples [ci0, ci0 + nc) of row g: those whose first pixel is the thread's
      const int ci0 = SUB_X == 2 ? (x0 + 1) >> 1 : x0;
      const int nc = SUB_X == 2 ? ((x0 + n + 1) >> 1) - ci0 : n;
      if (nc <= 0) continue;
      uint32_t cu[NC], cv[NC];
#pragma unroll
      for (int s = 0; s < NC; s++) {
        const float u = SUB_X * SUB_Y == 1 ? hu[s] : hu[s] * MEAN, v = SUB_X * SUB_Y == 1 ? hv[s] : hv[s] * MEAN;
        cu[s] = (code_of<BITS>(u, lut + NLDS, p.tables + NTAB) << p.shift) & ((1u << BITS) - 1u);
        cv[s] = (code_of<BITS>(v, lut + NLDS, p.tables + NTAB) << p.shift) & ((1u << BITS) - 1u);
      }
      if (INTERLEAVED) {
        char *crow = static_cast<char *>(v_first ? p.cr : p.cb) + size_t(g) * p.c_pitch + size_t(ci0) * (2 * BYTES);
        uint64_t bits = 0;
#pragma unroll
        for (int s = 0; s < NC; s++) {
          const uint32_t a = v_first ? cv[s] : cu[s], b = v_first ? cu[s] : cv[s];
          bits |= (uint64_t(a) << (2 * s * BITS)) | (uint64_t(b) << ((2 * s + 1) * BITS));
        }
        store_run<2 * NC * BYTES, BITS == 8>(crow, bits, 2 * nc * BYTES);
      } else {
        uint64_t ub = 0, vb = 0;
#pragma unroll
        for (int s = 0; s < NC; s++) { ub |= uint64_t(cu[s]) << (s * BITS); vb |= uint64_t(cv[s]) << (s * BITS); }
        const size_t off = size_t(g) * p.c_pitch + size_t(ci0) * BYTES;
        store_run<NC * BYTES, BITS == 8>(static_cast<char *>(p.cb) + off, ub, nc * BYTES);
        store_run<NC * BYTES, BITS == 8>(static_cast<char *>(p.cr) + off, vb, nc * BYTES);
      }
    }
  }
}

template <int BITS, int NCH, int SUB_X, int SUB_Y>
void launch_layout(const eu_ycbcr_encode_params &p, dim3 grid, hipStream_t st)
{
  if (p.c_step == 2) hipLaunchKernelGGL((ycbcr_encode_kernel<BITS, NCH, SUB_X, SUB_Y, true>), grid, dim3(NT), 0, st, p);
  else hipLaunchKernelGGL((ycbcr_encode_kernel<BITS, NCH, SUB_X, SUB_Y, false>), grid, dim3(NT), 0, st, p);
}

template <int BITS, int NCH>
void launch_sub(const eu_ycbcr_encode_params &p, dim3 grid, hipStream_t st)
{
  if (p.sub_x == 2 && p.sub_y == 2) launch_layout<BITS, NCH, 2, 2>(p, grid, st);
  else if (p.sub_x == 2) launch_layout<BITS, NCH, 2, 1>(p, grid, st);
  else if (p.sub_y == 2) launch_layout<BITS, NCH, 1, 2>(p, grid, st);
  else launch_layout<BITS, NCH, 1, 1>(p, grid, st);
}

}  // namespace

extern "C" int eu_launch_ycbcr_encode(const eu_ycbcr_encode_params *pp, void *stream)
{
  const eu_ycbcr_encode_params &p = *pp;
  if (p.w <= 0 || p.h <= 0 || !p.src || !p.y || !p.cb || !p.cr || !p.tables || (p.bits != 8 && p.bits != 16)) return -1;
  if (p.nch != 3 && p.nch != 4) return -1;
  if ((p.sub_x != 1 && p.sub_x != 2) || (p.sub_y != 1 && p.sub_y != 2) || (p.c_step != 1 && p.c_step != 2)) return -1;
  if (p.shift < 0 || p.shift >= p.bits) return -1;
  const size_t sb = size_t(p.bits / 8);
  if (p.c_step == 2) {             // the pair: one sample apart, either way round
    const uintptr_t b = reinterpret_cast<uintptr_t>(p.cb), r = reinterpret_cast<uintptr_t>(p.cr);
    if (r != b + sb && b != r + sb) return -1;
  }
  // the kernel counts the bytes of a row in an int, with room for the threads behind the row's end
  const size_t rf = size_t(p.w) * size_t(p.nch);
  if (rf > size_t(1) << 28) return -1;
  const size_t rb = size_t(p.w) * sb, cw = (size_t(p.w) + p.sub_x - 1) / p.sub_x;
  if (p.src_stride_bytes < rf * sizeof(float) || p.src_stride_bytes % sizeof(float) || reinterpret_cast<uintptr_t>(p.src) % sizeof(float)) return -1;
  if (p.y_pitch < rb || p.c_pitch < ((cw - 1) * p.c_step + 1) * sb) return -1;
  if (p.bits == 16 && ((reinterpret_cast<uintptr_t>(p.y) | reinterpret_cast<uintptr_t>(p.cb) | reinterpret_cast<uintptr_t>(p.cr) |
                        p.y_pitch | p.c_pitch) & 1)) return -1;
  // a row has at most one head thread and rb / 4 + 1 more (the dwords a row of rb bytes can touch behind its head)
  const size_t units = rb / 4 + 2;
  const size_t ng = (size_t(p.h) + p.sub_y - 1) / p.sub_y;
  const size_t gx = (units + NT - 1) / NT, gy = (ng + ROWS - 1) / ROWS;
  const size_t gy_max = gx >= MAX_GROUPS ? 1 : MAX_GROUPS / gx;
  const dim3 grid((unsigned)gx, (unsigned)(gy < gy_max ? gy : gy_max));
  hipStream_t st = (hipStream_t)stream;
  if (p.bits == 8) { if (p.nch == 3) launch_sub<8, 3>(p, grid, st); else launch_sub<8, 4>(p, grid, st); }
  else { if (p.nch == 3) launch_sub<16, 3>(p, grid, st); else launch_sub<16, 4>(p, grid, st); }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
