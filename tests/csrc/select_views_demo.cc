// Host test of eu_select_view_path(), eu_views_per_chunk() and the EU_HIP_VIEWS_MAX_KB switch
// (envutil_amd/csrc/eu_select.h), all plain C++.
// Prints one line per check; exit status 0 when all hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../envutil_amd/csrc/eu_select.h"

namespace {
int failures = 0;
void check(bool ok, const char *what)
{
  printf("%s: %s\n", ok ? "ok" : "FAILED", what);
  if (!ok) failures++;
}

eu_switches defaults()
{
  eu_switches s;
  memset(&s, 0, sizeof s);
  s.hybrid = 1; s.r4 = -1; s.colmajor = -1; s.colplan = 1;
  s.share = EU_SHARE_FACES | EU_SHARE_MIRRORS; s.iir_stream = 7; s.boxtab = 1; s.boxtab_max_kb = EU_BOXTAB_MAX_KB;
  s.views_max_kb = EU_VIEWS_MAX_KB;
  return s;
}

eu_render_params job(int form, int prj, int degree, int nch, int nch_out, int twine)
{
  eu_render_params p;
  memset(&p, 0, sizeof p);
  p.width = 256; p.height = 256; p.row_end = 256;
  p.form = form; p.norm_mode = twine && form == EU_FORM_BA ? EU_NORM_DIV : EU_NORM_NONE;
  p.twine = twine; p.ntaps = twine ? 4 : 0;
  p.nch = nch; p.nch_out = nch_out;
  p.src.prj = prj; p.src.nch = nch; p.src.degree = degree; p.src.es0 = nch; p.src.es1 = 1024 * nch;
  p.src.brighten = 1.0f; p.src.always_hit = 1;
  return p;
}

void expect(const char *what, const eu_render_params &p, const eu_switches &sw, eu_view_path want)
{
  const eu_view_path got = eu_select_view_path(p, sw);
  printf("%s: %s -> %s\n", got == want ? "ok" : "FAILED", what, got == EU_VIEWS_PACKED ? "packed" : "general");
  if (got != want) failures++;
}

void test_paths()
{
  const eu_switches d = defaults();
  const int prjs[3] = { EU_SPHERICAL, EU_CUBEMAP, EU_BIATAN6 };
  const int forms[2] = { EU_FORM_BCA, EU_FORM_BA };
  for (int prj : prjs)
    for (int form : forms)
      for (int deg = 1; deg <= 3; deg++)
        for (int nch = 1; nch <= 4; nch++)
          for (int twine = 0; twine < 2; twine++) {
            char what[112];
            snprintf(what, sizeof what, "packed: source %d form %d degree %d nch %d twine %d", prj, form, deg, nch, twine);
            expect(what, job(form, prj, deg, nch, nch, twine), d, EU_VIEWS_PACKED);
          }
  // switches that have no say: there is no plan, so neither the staged kernels nor the runs exist here
  { eu_switches s = d; s.r4 = 1; expect("R4=1 has no say", job(EU_FORM_BA, EU_SPHERICAL, 3, 3, 3, 0), s, EU_VIEWS_PACKED); }
  { eu_switches s = d; s.hybrid = 2; expect("HYBRID=2 has no say", job(EU_FORM_BA, EU_SPHERICAL, 3, 3, 3, 0), s, EU_VIEWS_PACKED); }
  { eu_switches s = d; s.direct = 1; expect("DIRECT=1 has no say", job(EU_FORM_BA, EU_CUBEMAP, 2, 4, 4, 1), s, EU_VIEWS_PACKED); }
  // one job per reason for the general form
  { eu_render_params p = job(EU_FORM_BA, EU_SPHERICAL, 3, 3, 3, 0); p.src.mask_paint = 1; expect("mask_paint", p, d, EU_VIEWS_GENERAL); }
  { eu_switches s = d; s.force_general = 1; expect("EU_HIP_KERNEL=1", job(EU_FORM_BA, EU_SPHERICAL, 3, 3, 3, 0), s, EU_VIEWS_GENERAL); }
  { eu_switches s = d; s.force_general = 1; expect("EU_HIP_KERNEL=1, twined", job(EU_FORM_BCA, EU_CUBEMAP, 1, 3, 3, 1), s, EU_VIEWS_GENERAL); }
  { eu_render_params p = job(EU_FORM_BA, EU_SPHERICAL, 3, 3, 3, 0); p.src.has_lcp = 1; expect("has_lcp", p, d, EU_VIEWS_GENERAL); }
  expect("nch_out != nch (3 -> 4)", job(EU_FORM_BA, EU_SPHERICAL, 1, 3, 4, 0), d, EU_VIEWS_GENERAL);
  expect("nch_out != nch (4 -> 1), twined", job(EU_FORM_BA, EU_CUBEMAP, 1, 4, 1, 1), d, EU_VIEWS_GENERAL);
  expect("degree 0", job(EU_FORM_BA, EU_SPHERICAL, 0, 3, 3, 0), d, EU_VIEWS_GENERAL);
  expect("degree 4", job(EU_FORM_BA, EU_SPHERICAL, 4, 3, 3, 0), d, EU_VIEWS_GENERAL);
  expect("degree 9", job(EU_FORM_BCA, EU_BIATAN6, 9, 3, 3, 0), d, EU_VIEWS_GENERAL);
  expect("fisheye target", job(EU_FORM_FISH, EU_SPHERICAL, 3, 3, 3, 0), d, EU_VIEWS_GENERAL);
  expect("stereographic target", job(EU_FORM_STER, EU_SPHERICAL, 1, 3, 3, 1), d, EU_VIEWS_GENERAL);
  expect("rectilinear source", job(EU_FORM_BA, EU_RECTILINEAR, 1, 3, 3, 0), d, EU_VIEWS_GENERAL);
  expect("fisheye source", job(EU_FORM_BA, EU_FISHEYE, 1, 4, 4, 1), d, EU_VIEWS_GENERAL);
  { eu_render_params p = job(EU_FORM_BA, EU_SPHERICAL, 3, 3, 3, 0); p.src.es0 = 4; expect("texels not dense", p, d, EU_VIEWS_GENERAL); }
}

// degrees 0 and 4 to 9: never the packed form, whatever the switches say
void test_high_degrees()
{
  const int prjs[3] = { EU_SPHERICAL, EU_CUBEMAP, EU_BIATAN6 };
  const int forms[2] = { EU_FORM_BCA, EU_FORM_BA };
  const int degrees[7] = { 0, 4, 5, 6, 7, 8, 9 };
  int n = 0, bad = 0;
  for (int prj : prjs)
    for (int form : forms)
      for (int deg : degrees)
        for (int nch = 1; nch <= 4; nch++)
          for (int twine = 0; twine < 2; twine++)
            for (int r4 = -1; r4 <= 2; r4++)
              for (int hybrid = 0; hybrid <= 2; hybrid++)
                for (int kernel = 0; kernel <= 1; kernel++)
                  for (int direct = 0; direct <= 1; direct++) {
                    eu_switches s = defaults();
                    s.r4 = r4; s.hybrid = hybrid; s.force_general = kernel; s.direct = direct;
                    n++;
                    if (eu_select_view_path(job(form, prj, deg, nch, nch, twine), s) != EU_VIEWS_GENERAL) {
                      bad++;
                      printf("FAILED: source %d form %d degree %d nch %d twine %d R4=%d HYBRID=%d KERNEL=%d DIRECT=%d -> packed\n", prj,
                             form, deg, nch, twine, r4, hybrid, kernel, direct);
                    }
                  }
  char what[96];
  snprintf(what, sizeof what, "high degrees: %d combinations, all general", n);
  check(bad == 0 && n == 3 * 2 * 7 * 4 * 2 * 4 * 3 * 2 * 2, what);
}

void test_switch()
{
  unsetenv("EU_HIP_VIEWS_MAX_KB");
  check(eu_read_switches().views_max_kb == EU_VIEWS_MAX_KB && EU_VIEWS_MAX_KB == 65536, "EU_HIP_VIEWS_MAX_KB unset: 65536");
  setenv("EU_HIP_VIEWS_MAX_KB", "", 1);
  check(eu_read_switches().views_max_kb == EU_VIEWS_MAX_KB, "EU_HIP_VIEWS_MAX_KB empty: the default");
  setenv("EU_HIP_VIEWS_MAX_KB", "300", 1);
  check(eu_read_switches().views_max_kb == 300, "EU_HIP_VIEWS_MAX_KB=300");
  setenv("EU_HIP_VIEWS_MAX_KB", "0", 1);
  check(eu_read_switches().views_max_kb == 0, "EU_HIP_VIEWS_MAX_KB=0");
  setenv("EU_HIP_VIEWS_MAX_KB", "-5", 1);
  check(eu_read_switches().views_max_kb == 0, "EU_HIP_VIEWS_MAX_KB=-5 is 0");
  setenv("EU_HIP_VIEWS_MAX_KB", "2000000000", 1);
  check(eu_read_switches().views_max_kb == 16 * 1024 * 1024, "EU_HIP_VIEWS_MAX_KB is capped at 16 GiB");
  // the other switches are read as before
  setenv("EU_HIP_KERNEL", "1", 1);
  check(eu_read_switches().force_general == 1 && eu_read_switches().boxtab_max_kb == EU_BOXTAB_MAX_KB, "the other switches");
  unsetenv("EU_HIP_KERNEL");
  unsetenv("EU_HIP_VIEWS_MAX_KB");
}

void test_chunks()
{
  // a 256 x 256 view: (6 * 256 + 24 * 256) * 4 = 30720 bytes of tables
  check(eu_views_per_chunk(256, 256, 65536) == 2184, "64 MiB hold 2184 views of 256 x 256");
  check(eu_views_per_chunk(256, 256, 30) == 1, "30 KiB hold one");
  check(eu_views_per_chunk(256, 256, 60) == 2, "60 KiB hold two");
  check(eu_views_per_chunk(256, 256, 29) == 1, "a view larger than the bound still goes through, alone");
  check(eu_views_per_chunk(256, 256, 0) == 1, "... and with a bound of 0");
  check(eu_views_per_chunk(1, 1, 65536) == 65535, "never more views than a grid's y extent");
  check(eu_views_per_chunk(1 << 30, 1 << 30, 16 * 1024 * 1024) == 1, "no overflow for huge views");
}
}  // namespace

int main()
{
  test_paths();
  test_high_degrees();
  test_switch();
  test_chunks();
  printf(failures ? "%d checks FAILED\n" : "all ok\n", failures);
  return failures ? 1 : 0;
}
