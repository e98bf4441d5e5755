// The work list between the staged render kernels and the direct-gather kernel behind them
// (eu_render4.hip, eu_render5.h; the buffer is eu_render_params::wl, allocated in eu_api_render.hip): its layout,
// the list a tile goes to, and how many ints a launch needs - defined once, for the kernels that write
// and read it, for the host that sizes it and for a host test program (tests/csrc/worklist_demo.cc).
// Plain C++ with the functions the kernels call marked for both sides under hipcc.
#ifndef EU_WORKLIST_H
#define EU_WORKLIST_H
#include <algorithm>
#include <climits>
#include <cstddef>
#include <vector>

#if defined(__HIPCC__)
#define EU_WL_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define EU_WL_FN inline
#endif

// EU4_SHARDS lists, so that the staged kernels' appends do not queue on one counter (~88 returning
// atomics per microsecond on one word); a tile goes to list eu4_shard_of(id)
#define EU4_SHARDS 1024
// layout (ints); every counter on a 64-byte line of its own
#define EU4_WL_SHARD(s) (16 * (s))                       // entries in list s
#define EU4_WL_DYN(x) (16 * (EU4_SHARDS + 1 + (x)))       // eu_render5_kernel: next batch of XCD x's second loop, x = 0 .. 7
#define EU4_WL_COUNTERS (EU4_SHARDS + 9)                 // the lines that hold a counter: the lists, one spare, the queues
#define EU4_WL_ENTRIES (16 * (EU4_SHARDS + 16))          // entry k of list s at + k * EU4_SHARDS + s
// The buffer holds TWO sets of this layout, the second EU4_WL_SET_INTS ints behind the first: its counters are the
// words 8 of the lines whose words 0 are the first set's (a line still serves one list or one queue), its entries
// lie over the first set's, shifted. Launch pair n appends to and reads set n % 2, and its direct-gather kernel
// stores zeros to the counters of the other set - pair n - 1's, which is through, and pair n + 1's, which starts
// behind this kernel - so nobody counts finished workgroups to find the one that may empty the lists (2048 returning
// atomics on one word, ~88 per microsecond, with every workgroup waiting for its own). The entries need no set of
// their own: a pair's entries are dead when its second kernel ends, the counters are what eu_hip_listed_tiles() adds up.
#define EU4_WL_SET_INTS 8
#define EU4_WL_SET(buf, parity) ((buf) + ((parity) & 1) * EU4_WL_SET_INTS)

// A tile id is an int: a launch has at most this many wave tiles (eu_select.h: eu_staged_covers)
#define EU4_WL_MAX_TILES ((size_t)INT_MAX)

// the work list a tile goes to: a multiplicative hash of the tile id. (id % EU4_SHARDS keeps the
// tile COLUMN: the tiles around a pole then land in a sixth of the lists, and the direct-gather
// kernel's waves on those lists work through ~10 tiles each while the others idle: 0.23 ms for
// 1.6 % of the headline's tiles.)
EU_WL_FN int eu4_shard_of(int id)
{
  return (int)(((unsigned)id * 0x9E3779B1u) >> 22) & (EU4_SHARDS - 1);
}

// The hash does not fill the lists evenly (of 4096 ids one list takes 5, of 786432 one takes 771), and
// list s holding m entries reaches index EU4_WL_ENTRIES + (m - 1) * EU4_SHARDS + s. A launch lists a
// subset of the ids 0 .. ntiles - 1, and a subset fills no list further than the whole set does: the
// entries region is M(ntiles) * EU4_SHARDS ints, M the population of the fullest list when every id is
// listed. M is counted, not estimated: the ids are hashed once, in order, up to the largest ntiles asked
// for so far, and the values of ntiles at which M grows are kept (M is monotone, so they answer every
// smaller ntiles as well). 786432 ids - the headline - are counted in about 2 ms (1.6 - 2.7 in five runs of
// tests/csrc/worklist_demo.cc, g++ -O2, one core of the Xeon host of the build machine; DESIGN.md 5 has the same
// figure); the cost is linear, so a launch near EU4_WL_MAX_TILES would hash 2^31 ids, about 3 s, once.
// The one census of the process is the function-local static of eu_render4_worklist_ints() below (an inline
// function: one instance across translation units). Not for concurrent callers (like the launchers that ask).
class eu4_wl_census {
  std::vector<unsigned> count_;
  std::vector<size_t> grows_;      // grows_[k]: the smallest ntiles whose fullest list holds k + 1 ids
  size_t n_ = 0;
  unsigned fullest_ = 0;

public:
  eu4_wl_census() : count_(EU4_SHARDS, 0u) {}
  // M(ntiles), ntiles <= EU4_WL_MAX_TILES
  size_t fullest(size_t ntiles)
  {
    for (; n_ < ntiles; n_++) {
      const unsigned c = ++count_[(size_t)eu4_shard_of((int)n_)];
      if (c > fullest_) { fullest_ = c; grows_.push_back(n_ + 1); }
    }
    return (size_t)(std::upper_bound(grows_.begin(), grows_.end(), ntiles) - grows_.begin());
  }
};

// ints of the counters and queues in front of the entries
inline size_t eu_render4_worklist_header_ints(void) { return EU4_WL_ENTRIES; }

// ints the work list buffer needs for a launch of `ntiles` wave tiles, whichever of them are listed and in
// whatever order; 0 for more tiles than ids (no such launch reaches the staged kernels)
inline size_t eu_render4_worklist_ints(size_t ntiles)
{
  static eu4_wl_census census;
  if (ntiles > EU4_WL_MAX_TILES) return 0;
  return EU4_WL_ENTRIES + census.fullest(ntiles) * EU4_SHARDS;
}

// ints of the buffer that holds both sets for such a launch (0 as above), and of what a host clears to empty both
inline size_t eu_render4_worklist_buffer_ints(size_t ntiles)
{
  const size_t one = eu_render4_worklist_ints(ntiles);
  return one ? one + EU4_WL_SET_INTS : 0;
}
inline size_t eu_render4_worklist_clear_ints(void) { return eu_render4_worklist_header_ints() + EU4_WL_SET_INTS; }

#endif
