// Host side of eu_render5_kernel's first loop: which 16x16 tiles may be rendered from ONE run of the
// coordinate stage. Plain C++ (no HIP): eu_render4.hip includes it, and so does a host test program.
//
// A double row (16 frame rows with a common column plan) of an upright target gets its source row and
// fraction per pixel from 'ry = B1 * c0 + A1' and sqrt(rx^2 + rz^2) of the column. Where B1 is +-0, ry is
// the row's A1 in every column, and then two double rows whose A1 agree in all 16 rows and whose column
// plans hold the same sqrt(rx^2 + rz^2) column for column - or column x against column W-1-x: a mirror -
// have the same iy, ty per lane. Nothing of this is assumed from the job: it is decided from the bits
// of the tables the kernel reads (a cubemap face of 96 pixels shares nothing: its stepper does not step
// in exact binary fractions).
#ifndef EU_SHARE_GROUPS_H
#define EU_SHARE_GROUPS_H
#include <climits>
#include <cstddef>
#include <cstring>
#include <vector>

#define EU_SHARE_MAX_MEMBERS 8
// one list entry: { members n, first tile column, n x { double row, plan | EU_SHARE_MIRROR } }
#define EU_SHARE_ENTRY_INTS (2 + 2 * EU_SHARE_MAX_MEMBERS)
#define EU_SHARE_MIRROR (1 << 30)
#define EU_SHARE_FACES 1        // mode bits: double rows of other faces may follow a leader
#define EU_SHARE_MIRRORS 2      //            a double row mirrored column for column may
// ... and those of the second loop's groups (eu_polar_groups.h), here for eu_select.h's sake
#define EU_POLAR_TWINS 1        //            a tile row of the opposite polar face may follow a leader
#define EU_POLAR_MIRRORS 2      //            a tile row mirrored column for column may

struct eu_share_input {
  int width, tiles16;           // frame width, 16-pixel tile columns
  int row_begin, row_end;       // the launch's rows; double row m covers row_begin + 16 m .. + 15
  int band_mode;                // non-zero: rows are not frame rows in sequence - nothing is shared
  int ncand;                    // candidates: the double rows with a common column plan, ascending
  const int *cand_m, *cand_plan;
  const float *h_row;           // host copy of the stepper's row table, row_floats per frame row
  size_t h_row_floats;
  int row_floats;
  const float *coltab;          // host copy of the column plans: [plan][width][col_floats]
  int col_floats, nplans;
  int mode;                     // EU_SHARE_* bits; 0: every entry is a single
  int unit_drows;               // double rows per XCD unit: the leader's unit names the XCD
};

struct eu_share_result {
  std::vector<int> entries;     // the lists of the 8 XCDs back to back, EU_SHARE_ENTRY_INTS per entry
  int off[9];                   // XCD x owns entries off[x] .. off[x + 1]
  int ecols;                    // tile columns one entry covers (tiles16, or tiles16 / 2 where mirrors are possible)
  long long follower_tiles;     // 16x16 tiles that are rendered from another tile's coordinates
  std::vector<int> xtab;        // [plan][tiles16] { min, max } of the base column ix over the tile's columns
                                // inside the frame; min = INT_MAX: a column is off the fast path
};

namespace eu_share_detail {
inline bool is_zero_bits(float v) { unsigned u; memcpy(&u, &v, 4); return (u & 0x7fffffffu) == 0; }
inline int ix_of(const eu_share_input &in, int plan, int x)
{
  int v; memcpy(&v, in.coltab + ((size_t)plan * in.width + x) * in.col_floats, 4); return v;
}
inline unsigned qs_of(const eu_share_input &in, int plan, int x)
{
  unsigned v; memcpy(&v, in.coltab + ((size_t)plan * in.width + x) * in.col_floats + 6, 4); return v;
}
}  // namespace eu_share_detail

inline void eu_share_build(const eu_share_input &in, eu_share_result &out)
{
  using namespace eu_share_detail;
  const int W = in.width, T = in.tiles16, np = in.nplans;
  // ---- the box x extent per (plan, tile column)
  out.xtab.assign((size_t)(np > 0 ? np : 1) * T * 2, 0);
  std::vector<char> plan_clean((size_t)(np > 0 ? np : 1), 1);     // no column off the fast path
  for (int pl = 0; pl < np; pl++)
    for (int t = 0; t < T; t++) {
      int mn = INT_MAX, mx = INT_MIN;
      bool okc = true;
      for (int x = 16 * t; x < 16 * t + 16 && x < W; x++) {
        const int ix = ix_of(in, pl, x);
        if (ix == INT_MIN) okc = false;
        mn = ix < mn ? ix : mn; mx = ix > mx ? ix : mx;
      }
      if (!okc) { mn = INT_MAX; mx = INT_MIN; plan_clean[(size_t)pl] = 0; }
      out.xtab[((size_t)pl * T + t) * 2] = mn; out.xtab[((size_t)pl * T + t) * 2 + 1] = mx;
    }
  const bool share_ok = in.mode != 0 && !in.band_mode && in.h_row && in.coltab;
  const bool half = share_ok && (in.mode & EU_SHARE_MIRRORS) && W % 16 == 0 && T % 2 == 0;
  out.ecols = half ? T / 2 : T;
  out.follower_tiles = 0;
  // ---- which candidates can share at all: all 16 rows inside the launch, B1 +-0 and A1 not (with A1 = +-0 the
  // sign of ry would be the sign of B1 * c0, which a mirror flips), no column of the plan off the fast path
  const int n = in.ncand;
  std::vector<char> can((size_t)n, 0), done((size_t)n, 0);
  std::vector<float> a1((size_t)n * 16, 0.0f);
  for (int i = 0; share_ok && i < n; i++) {
    const int y0 = in.row_begin + 16 * in.cand_m[i];
    const int pl = in.cand_plan[i];
    if (y0 + 16 > in.row_end || pl < 0 || pl >= np || !plan_clean[(size_t)pl]) continue;
    bool ok = true;
    for (int r = 0; r < 16 && ok; r++) {
      const size_t fr = (size_t)(y0 + r) * in.row_floats;
      if (fr + 6 > in.h_row_floats) { ok = false; break; }
      const float A1 = in.h_row[fr + 1], B1 = in.h_row[fr + 4];
      ok = is_zero_bits(B1) && !is_zero_bits(A1);
      a1[(size_t)i * 16 + r] = A1;
    }
    can[(size_t)i] = ok;
  }
  // sqrt(rx^2 + rz^2) of two plans, column for column (memo: 0 unknown, 1 equal, 2 not)
  std::vector<char> memo((size_t)(np > 0 ? np : 1) * (np > 0 ? np : 1) * 2, 0);
  auto qs_eq = [&](int pa, int pb, int mirror) -> bool {
    char &m = memo[((size_t)pa * np + pb) * 2 + mirror];
    if (!m) {
      m = 1;
      for (int x = 0; x < W; x++)
        if (qs_of(in, pa, x) != qs_of(in, pb, mirror ? W - 1 - x : x)) { m = 2; break; }
    }
    return m == 1;
  };
  std::vector<int> lists[8];
  auto emit = [&](int xcd, int colbase, const std::vector<int> &mem) {
    std::vector<int> &l = lists[xcd];
    const size_t at = l.size();
    l.resize(at + EU_SHARE_ENTRY_INTS, 0);
    l[at] = (int)mem.size() / 2; l[at + 1] = colbase;
    for (size_t k = 0; k < mem.size(); k++) l[at + 2 + k] = mem[k];
    out.follower_tiles += (long long)(mem.size() / 2 - 1) * out.ecols;
  };
  for (int i = 0; i < n; i++) {
    if (done[(size_t)i]) continue;
    done[(size_t)i] = 1;
    const int pi = in.cand_plan[i];
    const bool mirrored = half && can[(size_t)i] && qs_eq(pi, pi, 1);
    std::vector<int> faces(1, i);
    const int max_faces = mirrored ? EU_SHARE_MAX_MEMBERS / 2 : EU_SHARE_MAX_MEMBERS;
    if (can[(size_t)i] && (in.mode & EU_SHARE_FACES))
      for (int j = i + 1; j < n && (int)faces.size() < max_faces; j++) {
        if (done[(size_t)j] || !can[(size_t)j]) continue;
        if (memcmp(&a1[(size_t)i * 16], &a1[(size_t)j * 16], 16 * sizeof(float)) != 0) continue;
        const int pj = in.cand_plan[j];
        if (!qs_eq(pi, pj, 0)) continue;
        // in a mirrored group every face brings its mirror along: the entry covers the left half of the columns only
        if (mirrored && !qs_eq(pi, pj, 1)) continue;
        done[(size_t)j] = 1;
        faces.push_back(j);
      }
    std::vector<int> mem;
    for (int f : faces) {
      mem.push_back(in.cand_m[f]); mem.push_back(in.cand_plan[f]);
      if (mirrored) { mem.push_back(in.cand_m[f]); mem.push_back(in.cand_plan[f] | EU_SHARE_MIRROR); }
    }
    const int xcd = (in.cand_m[i] / (in.unit_drows > 0 ? in.unit_drows : 1)) & 7;
    emit(xcd, 0, mem);
    if (half && !mirrored) emit(xcd, T / 2, mem);
  }
  out.entries.clear();
  for (int x = 0; x < 8; x++) {
    out.off[x] = (int)(out.entries.size() / EU_SHARE_ENTRY_INTS);
    out.entries.insert(out.entries.end(), lists[x].begin(), lists[x].end());
  }
  out.off[8] = (int)(out.entries.size() / EU_SHARE_ENTRY_INTS);
}
#endif
