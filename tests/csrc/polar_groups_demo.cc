// Host test of envutil_amd/csrc/eu_polar_groups.h: the stepper tables of cubemap targets (eu::build_stepper_tables)
// in, the second loop's list of positions out. Without arguments it prints one line per check, exit status 0 when
// all hold; with 'face yaw_degrees row_begin row_end mode' it prints the follower tiles of that launch
// ('followers N'), which tests/test_gpu_polar_share.py holds the library's own count to.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "../../envutil_amd/csrc/eu_setup_math.h"
#include "../../envutil_amd/csrc/eu_polar_groups.h"

namespace {
int failures = 0;
void check(bool ok, const char *what)
{
  printf("%s: %s\n", ok ? "ok" : "FAILED", what);
  if (!ok) failures++;
}

struct job {
  int W, r0, r1, tiles16, band = 0;
  eu::stepper_tables tb;
  std::vector<int> rows;
  int off[9];
  job(int face, double yaw_deg, int row_begin, int row_end) : W(face), r0(row_begin), r1(row_end), tiles16((face + 15) / 16)
  {
    eu_target t;
    memset(&t, 0, sizeof t);
    t.projection = EU_CUBEMAP; t.width = face; t.height = 6 * face;
    double e[4];
    eu::get_extent(EU_CUBEMAP, face, 6 * face, M_PI / 2.0, e);
    t.x0 = e[0]; t.x1 = e[1]; t.y0 = e[2]; t.y1 = e[3];
    t.yaw = yaw_deg * M_PI / 180.0;
    const eu::mat3 basis = eu::rotate(eu::make_r3(t.roll, t.pitch, t.yaw, false), eu::make_r3(0, 0, 0, true));
    if (!eu::build_stepper_tables(t, basis, false, false, tb)) { printf("FAILED: no tables\n"); exit(1); }
    // the tile rows' column plans and the second loop's rows, by the functions the launcher calls
    std::vector<int> tp;
    std::vector<float> plans;
    eu_tile_row_plans(tb.row.data(), tb.row.size(), EU_ROW_FLOATS, r0, r1, [](int y) { return y; }, tp, plans);
    eu_second_loop_rows(tp, EU_SECOND_LOOP_UNIT_ROWS, rows, off);
  }
  eu_polar_result build(int mode)
  {
    eu_polar_input in;
    in.width = W; in.tiles16 = tiles16; in.row_begin = r0; in.row_end = r1; in.band_mode = band;
    in.nrows = (int)rows.size(); in.rows = rows.data();
    in.h_row = tb.row.data(); in.h_row_floats = tb.row.size(); in.row_floats = EU_ROW_FLOATS;
    in.h_col = tb.col.data(); in.h_col_floats = tb.col.size();
    in.mode = mode; in.unit_rows = EU_SECOND_LOOP_UNIT_ROWS;
    eu_polar_result r;
    eu_polar_build(in, r);
    return r;
  }
};

struct summary {
  int entries = 0, n[5] = { 0, 0, 0, 0, 0 }, flips = 0, mirrors = 0;
  int polar = 0, polar_n[5] = { 0, 0, 0, 0, 0 };     // entries whose leader lies in the top or the bottom face
  bool once = true, xcd_ok = true, leaders_plain = true;
};

// every second-loop tile in exactly one position, the leader's unit names the XCD, the counters add up
summary walk(const job &j, const eu_polar_result &r)
{
  summary s;
  std::map<std::pair<int, int>, int> seen;
  long long followers = 0;
  for (int x = 0; x < 8; x++)
    for (int e = r.off[x]; e < r.off[x + 1]; e++) {
      const int *q = &r.entries[(size_t)e * EU_POLAR_ENTRY_INTS];
      const int n = q[0], colbase = q[1];
      s.entries++;
      if (n < 1 || n > EU_POLAR_MAX_MEMBERS) { s.once = false; continue; }
      s.n[n]++;
      {
        const int y0 = j.r0 + 8 * (q[2] & (EU_POLAR_FLIP - 1));
        if (y0 >= 2 * j.W && y0 + 8 <= 4 * j.W) { s.polar++; s.polar_n[n]++; }
      }
      if (q[2] & (EU_POLAR_FLIP | EU_POLAR_MIRROR)) s.leaders_plain = false;
      if (((q[2] / 4) & 7) != x) s.xcd_ok = false;
      followers += (long long)(n - 1) * r.ecols;
      for (int k = 0; k < n; k++) {
        const int m = q[2 + 2 * k], slot = q[3 + 2 * k];
        const int row = m & (EU_POLAR_FLIP - 1);
        if (slot < 0 || slot >= (int)j.rows.size() || j.rows[(size_t)slot] != row) s.once = false;
        if (k > 0) { s.flips += (m & EU_POLAR_FLIP) != 0; s.mirrors += (m & EU_POLAR_MIRROR) != 0; }
        for (int c = colbase; c < colbase + r.ecols; c++)
          seen[std::make_pair(row, (m & EU_POLAR_MIRROR) ? j.tiles16 - 1 - c : c)]++;
      }
    }
  if (seen.size() != j.rows.size() * (size_t)j.tiles16) s.once = false;
  for (auto &kv : seen)
    if (kv.second != 1 || kv.first.second < 0 || kv.first.second >= j.tiles16) s.once = false;
  if (followers != r.follower_tiles) s.once = false;
  return s;
}

constexpr int BOTH = EU_POLAR_TWINS | EU_POLAR_MIRRORS;
}  // namespace

int main(int argc, char **argv)
{
  if (argc == 6) {
    job j(atoi(argv[1]), atof(argv[2]), atoi(argv[3]), atoi(argv[4]));
    const char m = argv[5][0];
    const eu_polar_result r = j.build(m == '0' ? 0 : m == 't' ? EU_POLAR_TWINS : m == 'm' ? EU_POLAR_MIRRORS : BOTH);
    printf("followers %lld\n", r.follower_tiles);
    return 0;
  }
  {
    job j(64, 0.0, 0, 384);
    const eu_polar_result r = j.build(BOTH);
    const summary s = walk(j, r);
    check(j.rows.size() == 16, "face 64: the second loop has the 16 tile rows of the two polar faces");
    check(s.entries == 8 && s.n[4] == 8, "face 64: every polar position has four members");
    check(s.once && s.xcd_ok && s.leaders_plain, "face 64: every second-loop tile exactly once");
    check(r.ecols == 2 && r.bcols == 1 && r.follower_tiles == 48, "face 64: half the columns per entry, one per dequeue, 48 followers");
    const eu_polar_result t = j.build(EU_POLAR_TWINS), m = j.build(EU_POLAR_MIRRORS), z = j.build(0);
    const summary st = walk(j, t), sm = walk(j, m), sz = walk(j, z);
    check(st.once && st.n[2] == 8 && st.entries == 8 && st.mirrors == 0 && t.ecols == 4 && t.follower_tiles == 32, "face 64, mode t: twins only");
    check(sm.once && sm.n[2] == 16 && sm.entries == 16 && sm.flips == 0 && m.ecols == 2 && m.follower_tiles == 32, "face 64, mode m: mirrors only");
    check(sz.once && sz.n[1] == 16 && sz.entries == 16 && z.ecols == 4 && z.bcols == 2 && z.follower_tiles == 0, "face 64, mode 0: entries of one");
  }
  for (int face : { 96, 80, 48 }) {
    job j(face, 0.0, 0, 6 * face);
    const eu_polar_result r = j.build(BOTH);
    const summary s = walk(j, r);
    char what[96];
    // (faces of 80 and 48 leave the two tile rows at the middle of every equatorial face to this loop as well - their
    // plans differ in the sign of a zero - and those follow nobody)
    snprintf(what, sizeof what, "face %d: twins only in the polar faces, singles elsewhere, every tile once", face);
    check(s.once && s.xcd_ok && s.polar == face / 8 && s.polar_n[2] == s.polar && s.n[2] == s.polar && s.n[1] == s.entries - s.polar &&
          s.mirrors == 0 && s.flips == s.polar && r.ecols == j.tiles16 && r.bcols == (s.n[1] ? 2 : 1), what);
  }
  for (int face : { 41, 33 }) {
    job j(face, 0.0, 0, 6 * face);
    const eu_polar_result r = j.build(BOTH);
    const summary s = walk(j, r);
    char what[96];
    snprintf(what, sizeof what, "face %d: entries of one", face);
    check(s.once && s.entries == (int)j.rows.size() && s.n[1] == s.entries && r.follower_tiles == 0 && r.bcols == 2, what);
  }
  {
    job j(64, 30.0, 0, 384);
    const eu_polar_result r = j.build(BOTH);
    const summary s = walk(j, r);
    check(s.once && s.entries > 0 && s.n[1] == s.entries && r.follower_tiles == 0, "face 64, yaw 30: entries of one");
  }
  {
    job j(64, 0.0, 128, 192);
    const eu_polar_result r = j.build(BOTH);
    const summary s = walk(j, r);
    check(s.once && s.entries == 8 && s.n[2] == 8 && s.flips == 0 && s.mirrors == 8, "face 64, rows 128-192: mirrors only");
  }
  {
    job j(64, 0.0, 136, 248);
    const eu_polar_result r = j.build(BOTH);
    const summary s = walk(j, r);
    check(s.once && j.rows.size() == 14 && s.entries == 7 && s.n[4] == 7, "face 64, rows 136-248: the twins whose rows are inside");
  }
  {
    job j(64, 0.0, 3, 381);
    const eu_polar_result r = j.build(BOTH);
    const summary s = walk(j, r);
    check(s.once && s.xcd_ok && s.entries > 0, "face 64, rows 3-381: every tile exactly once");
    printf("   (rows 3-381: %d entries, of 1 / 2 / 3 / 4 members: %d / %d / %d / %d)\n", s.entries, s.n[1], s.n[2], s.n[3], s.n[4]);
  }
  {
    job j(64, 0.0, 0, 384);
    j.band = 1;
    const eu_polar_result r = j.build(BOTH);
    const summary s = walk(j, r);
    check(s.once && s.n[1] == s.entries && r.follower_tiles == 0, "bands: nothing shared");
  }
  // one flipped bit takes the premise away from exactly the rows it touches
  {
    job j(64, 0.0, 0, 384);
    unsigned u;
    float *a2 = &j.tb.row[(size_t)(128 + 11) * EU_ROW_FLOATS + 2];       // top face, tile row 17, lane row 3
    memcpy(&u, a2, 4); u ^= 1u; memcpy(a2, &u, 4);
    const eu_polar_result r = j.build(BOTH);
    const summary s = walk(j, r);
    check(s.once && s.n[4] == 7 && s.n[2] == 2 && s.flips == 14, "a bit of A2 in one row: that row and its twin keep their mirrors only");
    job c(64, 0.0, 0, 384);
    float *cx = &c.tb.col[5];
    memcpy(&u, cx, 4); u ^= 1u; memcpy(cx, &u, 4);
    const eu_polar_result rc = c.build(BOTH);
    const summary sc = walk(c, rc);
    check(sc.once && sc.n[2] == 8 && sc.mirrors == 0 && rc.ecols == 4, "a bit of one column: no mirrors, the twins stay");
  }
  printf(failures ? "%d checks FAILED\n" : "all ok\n", failures);
  return failures ? 1 : 0;
}
