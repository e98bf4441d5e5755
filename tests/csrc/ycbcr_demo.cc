// Host program for include/eu_ycbcr.h: eu_ycbcr_rows over planes of odd sizes with MINIMAL pitches, every plane a heap
// block of exactly the bytes the frame has - so that a build with -fsanitize=address,undefined reports any byte read
// outside a plane - against a second, index-by-index statement of the three formulas. 8- and 16-bit samples, every
// subsampling, planar and interleaved chroma in both orders, 3 and 4 channels. Prints one line per case and "all ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/eu_ycbcr.h"

static uint32_t lcg_state = 12345u;
static uint32_t lcg() { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state >> 8; }

struct block {                      // exactly n bytes on the heap
  unsigned char *p; size_t n;
  explicit block(size_t bytes) : p((unsigned char *)std::malloc(bytes ? bytes : 1)), n(bytes) { for (size_t i = 0; i < n; i++) p[i] = (unsigned char)lcg(); }
  ~block() { std::free(p); }
  block(const block &) = delete;
};

static uint32_t sample_at(const unsigned char *plane, size_t pitch, int row, size_t index, int bits)
{
  const unsigned char *q = plane + (size_t)row * pitch + index * (size_t)(bits / 8);
  if (bits == 8) return q[0];
  uint16_t v; std::memcpy(&v, q, 2); return v;
}

int main()
{
  int failed = 0, cases = 0;
  const float m[4] = { 1.5748f, -0.18732427f, -0.46812427f, 1.8556f };
  for (int bits : { 8, 16 }) {
    const size_t sb = (size_t)bits / 8, ntab = (size_t)1 << bits;
    std::vector<float> yt(ntab), ct(ntab);
    for (size_t i = 0; i < ntab; i++) { yt[i] = (float)(lcg() % 4096) / 4000.0f - 0.01f; ct[i] = (float)(lcg() % 4096) / 4096.0f - 0.5f; }
    const int sizes[][2] = { {1, 1}, {2, 1}, {1, 2}, {3, 3}, {5, 3}, {3, 5}, {7, 5}, {64, 7}, {65, 9} };
    for (const auto &wh : sizes)
      for (int sub_x = 1; sub_x <= 2; sub_x++)
        for (int sub_y = 1; sub_y <= 2; sub_y++)
          for (int layout = 0; layout < 3; layout++)          // 0 planar, 1 cr behind cb (NV12), 2 cb behind cr (NV21)
            for (int nch = 3; nch <= 4; nch++) {
              const int w = wh[0], h = wh[1];
              const size_t cw = (size_t)(w + sub_x - 1) / sub_x, ch = (size_t)(h + sub_y - 1) / sub_y;
              const int c_step = layout ? 2 : 1;
              const size_t y_pitch = (size_t)w * sb;
              const size_t c_pitch = layout ? 2 * cw * sb : cw * sb;      // the smallest a plane of whole rows has
              block Y(y_pitch * h), C0(c_pitch * ch), C1(layout ? 0 : c_pitch * ch);
              const unsigned char *cb = layout == 2 ? C0.p + sb : C0.p;
              const unsigned char *cr = layout == 0 ? C1.p : layout == 1 ? C0.p + sb : C0.p;
              std::vector<float> out((size_t)w * h * nch, -7.0f);
              eu_ycbcr_rows(Y.p, cb, cr, y_pitch, c_pitch, c_step, sub_x, sub_y, bits, yt.data(), ct.data(), m[0], m[1], m[2],
                            m[3], w, h, nch, out.data());
              int bad = 0;
              for (int j = 0; j < h; j++)
                for (int i = 0; i < w; i++) {
                  const float yy = yt[sample_at(Y.p, y_pitch, j, (size_t)i, bits)];
                  const float u = ct[sample_at(cb, c_pitch, j / sub_y, (size_t)(i / sub_x) * c_step, bits)];
                  const float v = ct[sample_at(cr, c_pitch, j / sub_y, (size_t)(i / sub_x) * c_step, bits)];
                  volatile float rv = m[0] * v, gu = m[1] * u, gv = m[2] * v, bu = m[3] * u;
                  volatile float yg = yy + gu;
                  const float want[4] = { yy + rv, yg + gv, yy + bu, 1.0f };
                  if (std::memcmp(&out[((size_t)j * w + i) * nch], want, sizeof(float) * nch)) bad++;
                }
              cases++;
              if (bad) { failed++; std::printf("FAILED bits %d %dx%d sub %d%d layout %d nch %d: %d pixels\n", bits, w, h, sub_x, sub_y, layout, nch, bad); }
            }
  }
  std::printf("%d cases, %d failed\n", cases, failed);
  if (!failed) std::printf("all ok\n");
  return failed ? 1 : 0;
}
