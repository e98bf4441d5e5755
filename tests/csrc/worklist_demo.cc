// Host test of envutil_amd/csrc/eu_worklist.h: the staged kernels' appends to the work list, replayed on
// simulated list counters exactly as the writers perform them
//   sh = eu4_shard_of(id); slot = count[sh]++; index = EU4_WL_ENTRIES + slot * EU4_SHARDS + sh
// for the ids 0 .. ntiles - 1 (every tile listed - no subset reaches further) and for every third and every
// seventh of them. Every index must lie inside the entries region of a buffer of eu_render4_worklist_ints(ntiles)
// ints. Checked at every ntiles from 1 to 16384 (one incremental pass), at 98304, 786432 (the headline), 2^20
// and at the largest launch the staged path accepts. Prints one line per sweep, the first failure of a sweep,
// the slack of some sizes for tests/test_worklist.py; exit status 0 when all hold.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../envutil_amd/csrc/eu_select.h"
#include "../../envutil_amd/csrc/eu_worklist.h"

namespace {
int failures = 0;

// the counters of the lists and the range of the indices written so far
struct replay {
  std::vector<unsigned> count = std::vector<unsigned>(EU4_SHARDS, 0u);
  size_t lowest = (size_t)-1, highest = 0, listed = 0;
  void append(int id)
  {
    const int sh = eu4_shard_of(id);
    const int slot = (int)count[(size_t)sh]++;
    const size_t index = EU4_WL_ENTRIES + (size_t)slot * EU4_SHARDS + sh;
    lowest = std::min(lowest, index);
    highest = std::max(highest, index);
    listed++;
  }
  unsigned fullest() const { return *std::max_element(count.begin(), count.end()); }
};

// lists every stride-th id below `upto` and checks the indices at every ntiles <= dense and at the sizes in
// `marks` (ascending, the last one is `upto`); slack_at: sizes whose slack is printed
void sweep(const char *what, size_t stride, size_t dense, const std::vector<size_t> &marks, const std::vector<size_t> &slack_at = {})
{
  replay r;
  size_t next = 0, checked = 0, first_bad = 0, due = 0;
  const size_t upto = marks.back();
  for (size_t ntiles = 1; ntiles <= upto;) {
    for (; due < ntiles; due += stride) r.append((int)due);      // the ids below ntiles
    const size_t cap = eu_render4_worklist_ints(ntiles);
    checked++;
    const bool ok = r.lowest >= (size_t)EU4_WL_ENTRIES && r.highest < cap;
    if (!ok && !first_bad) {
      first_bad = ntiles;
      printf("FAILED: %s: ntiles = %zu: fullest list %u, highest index %zu, capacity %zu ints: %zu ints past the end\n",
             what, ntiles, r.fullest(), r.highest, cap, r.highest + 1 - cap);
    }
    for (size_t s : slack_at)
      if (s == ntiles) {
        printf("size %zu: fullest list %u, highest index %zu, capacity %zu\n", ntiles, r.fullest(), r.highest, cap);
        printf("slack %zu %lld\n", ntiles, (long long)cap - (long long)r.highest - 1);
      }
    // the next size: every one up to `dense`, then the marks
    if (ntiles < dense) { ntiles++; continue; }
    while (next < marks.size() && marks[next] <= ntiles) next++;
    if (next == marks.size()) break;
    ntiles = marks[next];
  }
  if (first_bad) failures++;
  printf("%s: %s, %zu ids listed, %zu sizes checked up to ntiles = %zu\n", first_bad ? "FAILED" : "ok", what, r.listed, checked, upto);
}
}  // namespace

int main()
{
  printf("shards %d\n", EU4_SHARDS);
  // the largest launch: a strip of EU_STAGED_MAX_TILES_Y tile rows of the widest frame an int holds, or what a tile id holds
  const unsigned long long widest = ((unsigned long long)INT_MAX + 15) / 16 * (unsigned long long)EU_STAGED_MAX_TILES_Y;
  const size_t largest = (size_t)std::min<unsigned long long>(widest, EU4_WL_MAX_TILES);
  printf("largest launch %zu tiles\n", largest);
  {
    // what the first frame of a new size pays on the host: a census of its own, not the cached one
    eu4_wl_census c;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t m = c.fullest(786432);
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    printf("census of 786432 ids: fullest list %zu, %.0f microseconds\n", m, us);
  }
  // a smaller launch behind a larger one is answered from the same census
  {
    const size_t big = eu_render4_worklist_ints(786432), small = eu_render4_worklist_ints(600), again = eu_render4_worklist_ints(786432);
    const bool ok = small == (size_t)EU4_WL_ENTRIES + EU4_SHARDS && big == again && eu_render4_worklist_ints(0) == (size_t)EU4_WL_ENTRIES &&
                    eu_render4_worklist_header_ints() == (size_t)EU4_WL_ENTRIES && eu_render4_worklist_ints(EU4_WL_MAX_TILES + 1) == 0;
    printf("%s: sizes asked for in any order; no entries for no tiles; no buffer beyond the ids\n", ok ? "ok" : "FAILED");
    if (!ok) failures++;
  }
  const std::vector<size_t> sizes = { 98304, 786432, (size_t)1 << 20 };
  std::vector<size_t> all = sizes;
  all.push_back(largest);
  sweep("every tile listed", 1, 16384, all, { 1024, 4096, 786432 });
  sweep("every third tile listed", 3, 16384, sizes);
  sweep("every seventh tile listed", 7, 16384, sizes);
  printf(failures ? "%d checks FAILED\n" : "all ok\n", failures);
  return failures ? 1 : 0;
}
