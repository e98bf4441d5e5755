// Host test of eu_views_per_chunk() with a facet count (envutil_amd/csrc/eu_select.h), plain C++: the views of
// one chunk of eu_hip_render_views_multi, whose tables take one block per (view, facet).
// Prints one line per check; exit status 0 when all hold.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "../../envutil_amd/csrc/eu_select.h"

namespace {
int failures = 0;
void check(bool ok, const char *what)
{
  printf("%s: %s\n", ok ? "ok" : "FAILED", what);
  if (!ok) failures++;
}

// the rule for one source as eu_hip_render_views has used it: restated here, not read from the header
int one_source(int width, int height, int max_kb)
{
  const unsigned long long per = (6ull * width + 24ull * height) * 4ull;
  const unsigned long long n = (unsigned long long)max_kb * 1024ull / per;
  return (int)std::max<unsigned long long>(1, std::min<unsigned long long>(n, 65535));
}
}  // namespace

int main()
{
  const int sizes[][2] = { { 1, 1 }, { 10, 4 }, { 129, 97 }, { 256, 256 }, { 1920, 1080 }, { 1 << 30, 1 << 30 } };
  const int bounds[] = { 0, 1, 25, 29, 30, 60, 65536, 16 * 1024 * 1024 };
  const int facets[] = { 1, 2, 6, 17, 72, 1000, 32767, 32768, 65535 };
  bool same = true, same_default = true, grid = true, least = true, bound = true;
  for (auto &s : sizes)
    for (int kb : bounds) {
      same = same && eu_views_per_chunk(s[0], s[1], kb, 1) == one_source(s[0], s[1], kb);
      same_default = same_default && eu_views_per_chunk(s[0], s[1], kb) == one_source(s[0], s[1], kb);
      for (int nf : facets) {
        const long long n = eu_views_per_chunk(s[0], s[1], kb, nf);
        grid = grid && n * nf <= 65535;
        least = least && n >= 1;
        // more than one view only where the bound holds them all
        const unsigned long long per = (unsigned long long)nf * (6ull * s[0] + 24ull * s[1]) * 4ull;
        bound = bound && (n == 1 || (unsigned long long)n * per <= (unsigned long long)kb * 1024ull);
      }
    }
  check(same, "one facet: the values of the single-source rule");
  check(same_default, "no facet count: the values of the single-source rule");
  check(grid, "views * nfct <= 65535");
  check(least, "at least one view");
  check(bound, "several views only within EU_HIP_VIEWS_MAX_KB");
  // a 256 x 256 view of six facets: 6 * (6 * 256 + 24 * 256) * 4 = 184320 bytes of tables
  check(eu_views_per_chunk(256, 256, 65536, 6) == 364, "64 MiB hold 364 views of 256 x 256 with six facets");
  check(eu_views_per_chunk(256, 256, 360, 6) == 2, "360 KiB hold two");
  check(eu_views_per_chunk(256, 256, 359, 6) == 1, "359 KiB hold one");
  check(eu_views_per_chunk(256, 256, 100, 6) == 1, "a view larger than the bound still goes through, alone");
  check(eu_views_per_chunk(1, 1, 65536, 6) == 10922, "six facets: 10922 views fill a grid's y extent");
  check(eu_views_per_chunk(1, 1, 65536, 65535) == 1, "65535 facets: one view");
  printf(failures ? "%d checks FAILED\n" : "all ok\n", failures);
  return failures ? 1 : 0;
}
