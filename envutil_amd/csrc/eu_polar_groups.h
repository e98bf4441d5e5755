// Host side of eu_render5_kernel's second loop with the box table: which 16x8 tiles may be rendered from ONE run
// of the ray, the root and the two atan2 chains. Plain C++ (no HIP): eu_render4.hip includes it, and so does a host
// test program (tests/csrc/polar_groups_demo.cc).
//
// A second-loop tile computes 'ray = B * c0 + A', lat = atan2(ry, sqrt(rx^2 + rz^2)), lon = atan2(rx, rz), and
// eu_atan2f_2_lean takes the atanf of the absolute quotient and puts the sign bit of its first argument on last.
//   Twins: where A0, B1, B2 are +-0 a ray is (B0 * c0, A1, A2). Two tile rows whose A2 and B0 agree bit for bit and
//     whose A1 differ in the sign bit alone - lane row k of the one against lane row 7 - k of the other - have the same
//     longitude and the latitude with the sign bit flipped (the top and the bottom face of an upright cubemap).
//   Mirrors: where the column table holds col[W-1-x] = -col[x] bit for bit, column W-1-x of such a row has rx
//     negated and ry, rz unchanged: the same latitude, the longitude with the sign bit flipped.
// Nothing of this is assumed from the job: it is decided from the bits of the tables the kernel reads. The affine
// halves of md_to_spline, the box, the staging, the taps and the stores stay every tile's own.
#ifndef EU_POLAR_GROUPS_H
#define EU_POLAR_GROUPS_H
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <map>
#include <utility>
#include <vector>
#include "eu_share_groups.h"    // the mode bits EU_POLAR_TWINS, EU_POLAR_MIRRORS (beside the first loop's)

#define EU_POLAR_MAX_MEMBERS 4
// one list entry: { members n, first tile column, n x { tile row | flags, slot of the row in the second loop's rows } }
#define EU_POLAR_ENTRY_INTS 12
#define EU_POLAR_FLIP (1 << 29)      // the member's lane rows run the other way (a twin)
#define EU_POLAR_MIRROR (1 << 30)    // the member's columns do (tile column tiles16 - 1 - c, columns W-1-x)
// what the launcher and the kernel fix and a host program has to use as well (eu_render4.hip asserts that they agree)
#define EU_TILE_ROWS 8               // frame rows per tile row
#define EU_PLAN_MAX 16               // column plans of a launch at the most
#define EU_SECOND_LOOP_UNIT_ROWS 4   // tile rows per XCD unit

struct eu_polar_input {
  int width, tiles16;           // frame width, 16-pixel tile columns
  int row_begin, row_end;       // the launch's rows; tile row r covers row_begin + 8 r .. + 7
  int band_mode;                // non-zero: rows are not frame rows in sequence - nothing is shared
  int nrows;                    // the second loop's tile rows, in slot order (the box table's order)
  const int *rows;
  const float *h_row;           // host copy of the stepper's row table, row_floats per frame row
  size_t h_row_floats;
  int row_floats;
  const float *h_col;           // host copy of the stepper's column table c0, one float per column
  size_t h_col_floats;
  int mode;                     // EU_POLAR_* bits; 0: every entry is a single
  int unit_rows;                // tile rows per XCD unit: the leader's unit names the XCD
};

struct eu_polar_result {
  std::vector<int> entries;     // the lists of the 8 XCDs back to back, EU_POLAR_ENTRY_INTS per entry
  int off[9];                   // XCD x owns entries off[x] .. off[x + 1]
  int ecols;                    // tile columns one entry covers (tiles16, or tiles16 / 2 where the columns mirror)
  int bcols;                    // tile columns one dequeue hands out: 1 where every entry has a follower, else 2
  long long follower_tiles;     // 16x8 tiles that are rendered from another tile's angles
};

namespace eu_polar_detail {
inline unsigned bits_of(float v) { unsigned u; memcpy(&u, &v, 4); return u; }
inline bool is_zero_bits(float v) { return (bits_of(v) & 0x7fffffffu) == 0; }
}  // namespace eu_polar_detail

// The column plans of a launch's tile rows: a tile row can take the x half of its coordinates from a per-column
// table when A0, A2, B0, B2 are the same bits in its 8 rows; tile rows with the same four constants share a plan, and
// there are EU_PLAN_MAX plans at the most. frame_row(y): the row of h_row that launch row y reads (a row beyond
// row_end - 1 counts as that row). tileplan: per tile row the plan id, -1: none; plans: 4 floats per plan.
template <class FrameRow>
inline void eu_tile_row_plans(const float *h_row, size_t h_row_floats, int row_floats, int row_begin, int row_end,
                              FrameRow frame_row, std::vector<int> &tileplan, std::vector<float> &plans)
{
  const int tiles_y = (row_end - row_begin + EU_TILE_ROWS - 1) / EU_TILE_ROWS;
  tileplan.assign((size_t)(tiles_y > 0 ? tiles_y : 0), -1);
  plans.clear();
  for (int ty = 0; h_row && ty < tiles_y; ty++) {
    float k[4] = { 0, 0, 0, 0 };
    bool same = true;
    for (int ly = 0; ly < EU_TILE_ROWS && same; ly++) {
      const int y = std::min(row_begin + ty * EU_TILE_ROWS + ly, row_end - 1);
      const size_t fr = (size_t)frame_row(y) * row_floats;
      if (fr + 6 > h_row_floats) { same = false; break; }
      const float c[4] = { h_row[fr + 0], h_row[fr + 2], h_row[fr + 3], h_row[fr + 5] };
      if (ly == 0) memcpy(k, c, sizeof k);
      else same = memcmp(k, c, sizeof k) == 0;
    }
    if (!same) continue;
    int id = -1;
    for (size_t j = 0; j < plans.size() / 4 && id < 0; j++)
      if (memcmp(&plans[4 * j], k, sizeof k) == 0) id = (int)j;
    if (id < 0 && plans.size() / 4 < EU_PLAN_MAX) {
      id = (int)(plans.size() / 4);
      plans.insert(plans.end(), k, k + 4);
    }
    tileplan[(size_t)ty] = id;
  }
}

// The second loop's tile rows - those of a launch's tile rows that have no column plan in common with their
// partner (tileplan: the plan id per tile row, -1: none; rows 2m and 2m + 1 are partners) - in slot order: the rows
// of XCD x are rows[off[x] .. off[x + 1]) in raster order, units of unit_rows tile rows dealt round-robin
inline void eu_second_loop_rows(const std::vector<int> &tileplan, int unit_rows, std::vector<int> &rows, int off[9])
{
  const int ty = (int)tileplan.size();
  auto paired = [&](int m) { return 2 * m + 1 < ty && tileplan[(size_t)2 * m] >= 0 && tileplan[(size_t)2 * m] == tileplan[(size_t)2 * m + 1]; };
  std::vector<int> per[8];
  for (int r = 0; r < ty; r++)
    if (!paired(r >> 1)) per[(r / unit_rows) & 7].push_back(r);
  rows.clear();
  for (int x = 0; x < 8; x++) { off[x] = (int)rows.size(); rows.insert(rows.end(), per[x].begin(), per[x].end()); }
  off[8] = (int)rows.size();
}

inline void eu_polar_build(const eu_polar_input &in, eu_polar_result &out)
{
  using namespace eu_polar_detail;
  const int W = in.width, T = in.tiles16, n = in.nrows, rf = in.row_floats;
  const bool share_ok = in.mode != 0 && !in.band_mode && in.h_row && in.h_col;
  // ---- the column mirror: a property of the whole column table
  bool colmirror = share_ok && (in.mode & EU_POLAR_MIRRORS) && W > 0 && W % 16 == 0 && T % 2 == 0 && in.h_col_floats >= (size_t)W;
  for (int x = 0; colmirror && x < W; x++)
    colmirror = !is_zero_bits(in.h_col[x]) && bits_of(in.h_col[W - 1 - x]) == (bits_of(in.h_col[x]) ^ 0x80000000u);
  out.ecols = colmirror ? T / 2 : T;
  out.follower_tiles = 0;
  // ---- per row: all 8 frame rows inside the launch and the table, and A0, B1, B2 +-0 in every one of them
  std::vector<char> plain((size_t)n, 0), done((size_t)n, 0);
  auto frame_row = [&](int i, int k) { return in.h_row + (size_t)(in.row_begin + 8 * in.rows[i] + k) * rf; };
  for (int i = 0; share_ok && i < n; i++) {
    const long long y0 = (long long)in.row_begin + 8ll * in.rows[i];
    if (y0 < 0 || y0 + 8 > in.row_end || (size_t)(y0 + 8) * rf > in.h_row_floats) continue;
    bool ok = true;
    for (int k = 0; k < 8 && ok; k++) {
      const float *r = frame_row(i, k);
      ok = is_zero_bits(r[0]) && is_zero_bits(r[4]) && is_zero_bits(r[5]);
    }
    plain[(size_t)i] = ok;
  }
  // ---- twins: rows by (A2, |A1|) of their LAST lane row, looked up with a leader's first
  std::map<std::pair<unsigned, unsigned>, std::vector<int>> by_last;
  const bool twins = share_ok && (in.mode & EU_POLAR_TWINS);
  for (int i = 0; twins && i < n; i++)
    if (plain[(size_t)i]) {
      const float *r = frame_row(i, 7);
      by_last[std::make_pair(bits_of(r[2]), bits_of(r[1]) & 0x7fffffffu)].push_back(i);
    }
  auto twin_of = [&](int i) -> int {
    if (!twins || !plain[(size_t)i]) return -1;
    const float *r0 = frame_row(i, 0);
    auto it = by_last.find(std::make_pair(bits_of(r0[2]), bits_of(r0[1]) & 0x7fffffffu));
    if (it == by_last.end()) return -1;
    for (int j : it->second) {
      if (j == i || done[(size_t)j]) continue;
      bool ok = true;
      for (int k = 0; k < 8 && ok; k++) {
        const float *a = frame_row(i, k), *b = frame_row(j, 7 - k);
        ok = bits_of(a[2]) == bits_of(b[2]) && bits_of(a[3]) == bits_of(b[3]) && !is_zero_bits(a[1]) &&
             bits_of(a[1]) == (bits_of(b[1]) ^ 0x80000000u);
      }
      if (ok) return j;
    }
    return -1;
  };
  // leaders in raster order, whatever the order of the slots
  std::vector<int> order((size_t)n);
  for (int i = 0; i < n; i++) order[(size_t)i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return in.rows[a] < in.rows[b]; });
  std::vector<int> lists[8];
  bool all_followed = n > 0;
  for (int oi = 0; oi < n; oi++) {
    const int i = order[(size_t)oi];
    if (done[(size_t)i]) continue;
    done[(size_t)i] = 1;
    const int j = twin_of(i);
    if (j >= 0) done[(size_t)j] = 1;
    const bool mirrored = colmirror && plain[(size_t)i];
    int mem[2 * EU_POLAR_MAX_MEMBERS], nm = 0;
    auto add = [&](int slot, int flags) { mem[2 * nm] = in.rows[slot] | flags; mem[2 * nm + 1] = slot; nm++; };
    add(i, 0);
    if (mirrored) add(i, EU_POLAR_MIRROR);
    if (j >= 0) {
      add(j, EU_POLAR_FLIP);
      if (mirrored) add(j, EU_POLAR_FLIP | EU_POLAR_MIRROR);
    }
    if (nm < 2) all_followed = false;
    const int xcd = (in.rows[i] / (in.unit_rows > 0 ? in.unit_rows : 1)) & 7;
    auto emit = [&](int colbase) {
      std::vector<int> &l = lists[xcd];
      const size_t at = l.size();
      l.resize(at + EU_POLAR_ENTRY_INTS, 0);
      l[at] = nm; l[at + 1] = colbase;
      for (int k = 0; k < 2 * nm; k++) l[at + 2 + k] = mem[k];
      out.follower_tiles += (long long)(nm - 1) * out.ecols;
    };
    emit(0);
    if (colmirror && !mirrored) emit(T / 2);
  }
  out.bcols = all_followed ? 1 : 2;
  out.entries.clear();
  for (int x = 0; x < 8; x++) {
    out.off[x] = (int)(out.entries.size() / EU_POLAR_ENTRY_INTS);
    out.entries.insert(out.entries.end(), lists[x].begin(), lists[x].end());
  }
  out.off[8] = (int)(out.entries.size() / EU_POLAR_ENTRY_INTS);
}
#endif
