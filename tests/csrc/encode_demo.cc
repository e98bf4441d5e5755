// encode_demo - io::encode_steps (include/eu_image_io.hpp) against the host route it stands in for,
// io::convert_colour + the quantiser as io::write_one calls it. Host code only, a program of its own.
//
//   encode_demo sweep NTHREADS
//     All 2^32 float bit patterns, every pair of Linear / sRGB / Rec709, maxval 255 (8 bit) and 65535 (16 bit):
//     18 tables. Per float the pair's curve is evaluated once (convert_colour) and quantised for both maxvals;
//     the count over the table - the number of k >= 1 with v >= steps[k], what the device evaluates - has to be
//     that code. The floats are walked in the order of their values, so the count is a cursor that only moves up.
//     One line per table, then "failures: N"; a failure is a difference in a table the builder accepted, a refused
//     table without a difference, one of the two Rec709 tables at 65535 accepted, or more than two refused.
//   encode_demo host IN.pfm OUT FROM TO [cube]
//     the host route to a file: read_image, convert_colour FROM -> TO, write_image (cube: six faces for a %s name)
//   encode_demo steps BITS MAXVAL FROM TO OUT
//     the step tables as raw floats, colour then alpha; exit status 3 (the file is written all the same) when the
//     builder refuses the table
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "eu_image_io.hpp"

using namespace project;

namespace {

const char *const space[3] = { "Linear", "sRGB", "Rec709" };
const int depth[2][2] = { { 8, 255 }, { 16, 65535 } };

struct table {
  std::vector<float> colour, alpha;
  bool accepted = false;
  std::string why;
  std::atomic<unsigned long long> diffs { 0 };
  std::mutex lock;
  uint32_t first_key = 0xffffffffu;       // the smallest key with a difference
};

table tables[3][3][2];                    // [from][to][depth]

constexpr uint32_t CHUNK_BITS = 20, BLOCK = 4096;
std::atomic<uint32_t> next_chunk { 0 };

// the count over a table for v, given that it is at least *pos: steps[1 .. m] are numbers, v is not NaN
inline unsigned count_from(const float *steps, unsigned m, unsigned *pos, float v)
{
  unsigned p = *pos;
  while (p < m && v >= steps[p + 1]) p++;
  return *pos = p;
}

void sweep_worker()
{
  std::vector<float> src(BLOCK), buf(BLOCK);
  std::string err;
  for (;;) {
    const uint32_t c = next_chunk.fetch_add(1);
    if (c >= (1u << (32 - CHUNK_BITS))) return;
    const uint32_t k0 = c << CHUNK_BITS;
    const float v_first = io::key_float(k0);
    unsigned pos[3][3][2];
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++)
        for (int d = 0; d < 2; d++) {
          // the cursor starts below the chunk's first float (0 for a NaN: every compare fails)
          const float *s = tables[a][b][d].colour.data();
          const unsigned m = unsigned(depth[d][1]);
          unsigned p = 0;
          if (v_first == v_first) p = unsigned(std::upper_bound(s + 1, s + 1 + m, v_first) - (s + 1));
          pos[a][b][d] = p ? p - 1 : 0;
        }
    for (uint32_t off = 0; off < (1u << CHUNK_BITS); off += BLOCK) {
      for (uint32_t i = 0; i < BLOCK; i++) src[i] = io::key_float(k0 + off + i);
      for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
          buf = src;
          if (!io::convert_colour(buf.data(), BLOCK, 1, space[a], space[b], err)) { std::fprintf(stderr, "%s\n", err.c_str()); std::exit(2); }
          for (int d = 0; d < 2; d++) {
            table &t = tables[a][b][d];
            const float *s = t.colour.data();
            const unsigned m = unsigned(depth[d][1]);
            unsigned p = pos[a][b][d];
            unsigned long long bad = 0;
            uint32_t first = 0xffffffffu;
            for (uint32_t i = 0; i < BLOCK; i++) {
              const float v = src[i];
              const unsigned want = io::quantise_sample(buf[i], depth[d][1]);
              const unsigned got = v == v ? count_from(s, m, &p, v) : 0u;
              if (got != want) { if (!bad) first = k0 + off + i; bad++; }
            }
            pos[a][b][d] = p;
            if (bad) {
              t.diffs += bad;
              std::lock_guard<std::mutex> hold(t.lock);
              t.first_key = std::min(t.first_key, first);
            }
          }
        }
    }
  }
}

int sweep(int nthreads)
{
  int failures = 0, refused = 0;
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++)
      for (int d = 0; d < 2; d++) {
        table &t = tables[a][b][d];
        t.accepted = io::encode_steps(depth[d][0], depth[d][1], space[a], space[b], t.colour, t.alpha, t.why);
        if (t.colour.size() != size_t(1) << depth[d][0]) { std::printf("FAILED: %s -> %s: no table: %s\n", space[a], space[b], t.why.c_str()); return 1; }
        refused += !t.accepted;
      }
  // alpha has no curve: its table is the quantiser's alone, the colour table of equal spaces
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++)
      for (int d = 0; d < 2; d++)
        if (std::memcmp(tables[a][b][d].alpha.data(), tables[0][0][d].colour.data(), tables[0][0][d].colour.size() * 4)) {
          failures++;
          std::printf("FAILED: %s -> %s at %d: the alpha table is not the quantiser's\n", space[a], space[b], depth[d][1]);
        }
  std::vector<std::thread> pool;
  for (int i = 0; i < nthreads; i++) pool.emplace_back(sweep_worker);
  for (auto &th : pool) th.join();
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++)
      for (int d = 0; d < 2; d++) {
        table &t = tables[a][b][d];
        const unsigned long long diffs = t.diffs.load();
        std::printf("%s -> %s at %d: %s, %llu differences", space[a], space[b], depth[d][1], t.accepted ? "accepted" : "refused", diffs);
        if (diffs) std::printf(", the first at %.9g", double(io::key_float(t.first_key)));
        if (!t.accepted) std::printf(" (%s)", t.why.c_str());
        std::printf("\n");
        if (t.accepted && diffs) { failures++; std::printf("FAILED: an accepted table differs from the host route\n"); }
        if (!t.accepted && !diffs) { failures++; std::printf("FAILED: refused, but the table tells every float's code\n"); }
        if (a == 2 && b != 2 && d == 1 && t.accepted) { failures++; std::printf("FAILED: Rec709's drop at its joint went unnoticed\n"); }
      }
  if (refused > 2) { failures++; std::printf("FAILED: %d of 18 tables refused\n", refused); }
  std::printf("failures: %d\n", failures);
  return failures ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv)
{
  const std::string mode = argc > 1 ? argv[1] : "";
  std::string err;
  if (mode == "sweep" && argc == 3) return sweep(std::max(1, std::atoi(argv[2])));
  if (mode == "host" && (argc == 6 || argc == 7)) {
    std::vector<float> px;
    int w = 0, h = 0, nch = 0;
    if (!io::read_image(argv[2], px, w, h, nch, err)) { std::fprintf(stderr, "encode_demo: %s\n", err.c_str()); return 1; }
    if (!io::convert_colour(px.data(), size_t(w) * h, nch, argv[4], argv[5], err)) { std::fprintf(stderr, "encode_demo: %s\n", err.c_str()); return 1; }
    const bool cube = argc == 7 && std::string(argv[6]) == "cube";
    if (!io::write_image(argv[3], px.data(), w, h, nch, cube, err)) { std::fprintf(stderr, "encode_demo: %s\n", err.c_str()); return 1; }
    return 0;
  }
  if (mode == "steps" && argc == 7) {
    std::vector<float> colour, alpha;
    const bool ok = io::encode_steps(std::atoi(argv[2]), std::atoi(argv[3]), argv[4], argv[5], colour, alpha, err);
    if (!ok) std::fprintf(stderr, "encode_demo: %s\n", err.c_str());
    if (colour.empty() || alpha.size() != colour.size()) return 1;
    FILE *f = std::fopen(argv[6], "wb");
    if (!f) return 1;
    const bool wrote = std::fwrite(colour.data(), 4, colour.size(), f) == colour.size() && std::fwrite(alpha.data(), 4, alpha.size(), f) == alpha.size();
    if (std::fclose(f) != 0 || !wrote) return 1;
    return ok ? 0 : 3;
  }
  std::fprintf(stderr, "usage: encode_demo sweep NTHREADS | host IN.pfm OUT FROM TO [cube] | steps BITS MAXVAL FROM TO OUT\n");
  return 2;
}
