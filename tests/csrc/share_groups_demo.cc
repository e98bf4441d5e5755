// Host test of envutil_amd/csrc/eu_share_groups.h: synthetic row and column tables in, the first loop's
// group list out. Prints one line per check; exit status 0 when all hold.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "../../envutil_amd/csrc/eu_share_groups.h"

namespace {
constexpr int ROWF = 24, COLF = 8;
int failures = 0;
void check(bool ok, const char *what)
{
  printf("%s: %s\n", ok ? "ok" : "FAILED", what);
  if (!ok) failures++;
}

// an "upright cubemap" of four equatorial faces of F rows and W columns: face f has plan f, the rows of all
// faces the same A1, B1 = +0 or -0, and every plan the same, mirror-symmetric sqrt(rx^2 + rz^2) column
struct job {
  int W, F, row_begin, row_end, band = 0, mode = EU_SHARE_FACES | EU_SHARE_MIRRORS;
  std::vector<float> row, col;
  std::vector<int> m, plan;
  job(int W_, int F_) : W(W_), F(F_), row_begin(0), row_end(4 * F_)
  {
    row.assign((size_t)4 * F * ROWF, 0.0f);
    col.assign((size_t)4 * W * COLF, 0.0f);
    for (int f = 0; f < 4; f++) {
      for (int y = 0; y < F; y++) {
        float *r = &row[((size_t)f * F + y) * ROWF];
        r[1] = (float)(2 * y + 1 - F) / (float)F;
        r[4] = (f & 1) ? -0.0f : 0.0f;
        r[0] = (float)f; r[2] = 1.0f - (float)f;
      }
      for (int x = 0; x < W; x++) {
        float *c = &col[((size_t)f * W + x) * COLF];
        const int ix = 100 * f + x;
        memcpy(&c[0], &ix, 4);
        const float u = (float)(2 * x + 1 - W) / (float)W;
        c[6] = 1.0f + u * u;
      }
    }
  }
  void candidates()
  {
    m.clear(); plan.clear();
    const int tiles_y = (row_end - row_begin + 7) / 8;
    for (int k = 0; 2 * k + 1 < tiles_y; k++) {
      // as the launcher does: both tile rows inside one face
      const int y0 = row_begin + 16 * k, y1 = std::min(row_begin + 16 * k + 15, row_end - 1);
      if (y0 / F == y1 / F) { m.push_back(k); plan.push_back(y0 / F); }
    }
  }
  eu_share_result build()
  {
    candidates();
    eu_share_input in;
    in.width = W; in.tiles16 = (W + 15) / 16; in.row_begin = row_begin; in.row_end = row_end; in.band_mode = band;
    in.ncand = (int)m.size(); in.cand_m = m.data(); in.cand_plan = plan.data();
    in.h_row = row.data(); in.h_row_floats = row.size(); in.row_floats = ROWF;
    in.coltab = col.data(); in.col_floats = COLF; in.nplans = 4;
    in.mode = mode; in.unit_drows = 2;
    eu_share_result r;
    eu_share_build(in, r);
    return r;
  }
  // every 16x16 tile of every candidate exactly once?
  bool exact_cover(const eu_share_result &r) const
  {
    const int T = (W + 15) / 16;
    std::map<std::pair<int, int>, int> seen;
    for (size_t e = 0; e < r.entries.size(); e += EU_SHARE_ENTRY_INTS) {
      const int *q = &r.entries[e];
      if (q[0] < 1 || q[0] > EU_SHARE_MAX_MEMBERS) return false;
      if ((q[3] & EU_SHARE_MIRROR) != 0) return false;                   // a leader is never a mirror
      for (int k = 0; k < q[0]; k++)
        for (int c = q[1]; c < q[1] + r.ecols; c++)
          seen[{ q[2 + 2 * k], (q[3 + 2 * k] & EU_SHARE_MIRROR) ? T - 1 - c : c }]++;
    }
    if (seen.size() != m.size() * (size_t)T) return false;
    for (auto &kv : seen) if (kv.second != 1) return false;
    for (int k : m) for (int c = 0; c < T; c++) if (!seen.count({ k, c })) return false;
    if (r.off[0] != 0 || r.off[8] != (int)(r.entries.size() / EU_SHARE_ENTRY_INTS)) return false;
    for (int x = 0; x < 8; x++) if (r.off[x] > r.off[x + 1]) return false;
    return true;
  }
};

// members per entry -> number of entries
std::map<int, int> sizes(const eu_share_result &r)
{
  std::map<int, int> h;
  for (size_t e = 0; e < r.entries.size(); e += EU_SHARE_ENTRY_INTS) h[r.entries[e]]++;
  return h;
}
// is double row m (mirror or not) a follower or leader of an entry with more than one member?
bool shared(const eu_share_result &r, int m, bool mirror)
{
  for (size_t e = 0; e < r.entries.size(); e += EU_SHARE_ENTRY_INTS)
    for (int k = 0; k < r.entries[e]; k++)
      if (r.entries[e + 2 + 2 * k] == m && ((r.entries[e + 3 + 2 * k] & EU_SHARE_MIRROR) != 0) == mirror && r.entries[e] > 1) return true;
  return false;
}
void flip(float &v) { unsigned u; memcpy(&u, &v, 4); u ^= 1u; memcpy(&v, &u, 4); }
}  // namespace

int main()
{
  const int W = 64, F = 64, D = F / 16;      // D double rows per face
  {
    job j(W, F);
    const eu_share_result r = j.build();
    const auto h = sizes(r);
    check(h.size() == 1 && h.count(8) && h.at(8) == D && r.ecols == 2, "identical tables: groups of 8, half the columns each");
    check(r.follower_tiles == (long long)7 * D * 2, "identical tables: 7 of 8 tiles are followers");
    check(j.exact_cover(r), "identical tables: every tile in exactly one group");
    bool xt = r.xtab.size() == (size_t)4 * 4 * 2;
    for (int p = 0; xt && p < 4; p++) for (int t = 0; t < 4; t++)
      xt = xt && r.xtab[(p * 4 + t) * 2] == 100 * p + 16 * t && r.xtab[(p * 4 + t) * 2 + 1] == 100 * p + 16 * t + 15;
    check(xt, "x extent per plan and tile column");
  }
  {
    job j(W, F);
    flip(j.row[((size_t)2 * F + 16 + 5) * ROWF + 1]);       // A1 of one row of face 2, double row 1
    const eu_share_result r = j.build();
    const auto h = sizes(r);
    check(h.size() == 3 && h.at(8) == D - 1 && h.at(6) == 1 && h.at(2) == 1, "one bit of A1: that double row leaves its group (with its mirror)");
    check(j.exact_cover(r), "one bit of A1: every tile in exactly one group");
    bool only = true;
    for (size_t e = 0; e < r.entries.size(); e += EU_SHARE_ENTRY_INTS)
      if (r.entries[e] == 2) only = only && r.entries[e + 2] == 2 * D + 1 && r.entries[e + 4] == 2 * D + 1;
    check(only, "one bit of A1: exactly that member");
  }
  {
    job j(W, F);
    flip(j.col[((size_t)3 * W + 10) * COLF + 6]);           // sqrt(rx^2 + rz^2) of one column of plan 3
    const eu_share_result r = j.build();
    const auto h = sizes(r);
    // face 3 equals neither the others nor its own mirror: singles over both halves of the columns
    check(h.size() == 2 && h.at(6) == D && h.at(1) == 2 * D, "one bit of qs: the face with that plan leaves every group");
    check(j.exact_cover(r), "one bit of qs: every tile in exactly one group");
    bool none = true;
    for (int k = 0; k < D; k++) none = none && !shared(r, 3 * D + k, false) && !shared(r, 3 * D + k, true);
    check(none, "one bit of qs: exactly that member");
  }
  {
    job j(W, F);
    const int imin = (-2147483647 - 1);
    memcpy(&j.col[((size_t)1 * W + 40) * COLF], &imin, 4);  // a column of plan 1 off the fast path
    const eu_share_result r = j.build();
    const auto h = sizes(r);
    check(h.at(6) == D && h.at(1) == 2 * D && j.exact_cover(r), "a column off the fast path: its plan shares nothing");
    check(r.xtab[(1 * 4 + 2) * 2] == INT_MAX && r.xtab[(1 * 4 + 1) * 2] == 116, "a column off the fast path: sentinel in the x extent of its tile only");
  }
  {
    job j(48, F);                                           // three tile columns: no mirrors
    const eu_share_result r = j.build();
    const auto h = sizes(r);
    check(h.size() == 1 && h.at(4) == D && r.ecols == 3 && j.exact_cover(r), "odd tile count: faces only");
  }
  {
    job j(56, F);                                           // width not a multiple of 16: no mirrors
    const eu_share_result r = j.build();
    const auto h = sizes(r);
    check(h.size() == 1 && h.at(4) == D && r.ecols == 4 && j.exact_cover(r), "width not a multiple of 16: faces only");
  }
  {
    job j(W, F);
    j.row_end = 4 * F - 6;                                  // the last double row of face 3 is cut
    const eu_share_result r = j.build();
    const auto h = sizes(r);
    check(h.at(8) == D - 1 && h.at(6) == 1 && h.at(1) == 2 && j.exact_cover(r), "row range: the cut double row is a single, the rest of its group stays");
  }
  {
    job j(W, F);
    j.row_begin = 16; j.row_end = 3 * F + 16;               // faces 0 and 3 lose rows; still aligned
    const eu_share_result r = j.build();
    check(j.exact_cover(r) && r.follower_tiles > 0, "row range from row 16: every tile in exactly one group");
  }
  {
    job j(W, F);
    j.row_begin = 5;                                        // double rows straddle different A1: rows shift by 5 in every face alike
    const eu_share_result r = j.build();
    check(j.exact_cover(r), "row range from row 5: every tile in exactly one group");
  }
  {
    job j(W, F);
    j.band = 1;
    const eu_share_result r = j.build();
    const auto h = sizes(r);
    check(h.size() == 1 && h.count(1) && r.follower_tiles == 0 && j.exact_cover(r), "band mode: singles");
  }
  {
    job j(W, F);
    j.mode = 0;
    eu_share_result r = j.build();
    auto h = sizes(r);
    check(h.size() == 1 && h.count(1) && r.follower_tiles == 0 && r.ecols == 4 && j.exact_cover(r), "mode 0: singles");
    j.mode = EU_SHARE_MIRRORS; r = j.build(); h = sizes(r);
    check(h.size() == 1 && h.at(2) == 4 * D && j.exact_cover(r), "mirrors only: groups of 2");
    j.mode = EU_SHARE_FACES; r = j.build(); h = sizes(r);
    check(h.size() == 1 && h.at(4) == D && r.ecols == 4 && j.exact_cover(r), "faces only: groups of 4");
  }
  {
    job j(W, F);
    for (int y = 0; y < F; y++) j.row[((size_t)1 * F + y) * ROWF + 4] = 1e-30f;     // B1 of face 1 not zero
    const eu_share_result r = j.build();
    const auto h = sizes(r);
    check(h.at(6) == D && h.at(1) == 2 * D && j.exact_cover(r), "B1 not +-0: that face shares nothing");
  }
  printf("%s\n", failures ? "FAILED" : "all ok");
  return failures ? 1 : 0;
}
