// Host test of eu_select_layer_path(), the chunking arithmetic of eu_hip_render_layers (eu_layers_per_launch,
// eu_layers_launches, eu_layers_groups, eu_layers_in_group) and the EU_HIP_LAYERS_MAX switch
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
  s.views_max_kb = EU_VIEWS_MAX_KB; s.layers_max = EU_LAYERS_MAX;
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

void expect(const char *what, const eu_render_params &p, const eu_switches &sw, eu_layer_path want)
{
  const eu_layer_path got = eu_select_layer_path(p, sw);
  // the rules are those of the view calls: the two must never part
  const bool as_views = (got == EU_LAYERS_PACKED) == (eu_select_view_path(p, sw) == EU_VIEWS_PACKED);
  const bool ok = got == want && as_views;
  printf("%s: %s -> %s\n", ok ? "ok" : "FAILED", what, got == EU_LAYERS_PACKED ? "packed" : "general");
  if (!ok) failures++;
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
            expect(what, job(form, prj, deg, nch, nch, twine), d, EU_LAYERS_PACKED);
          }
  // switches that have no say: there is no plan, so neither the staged kernels nor the runs exist here
  { eu_switches s = d; s.r4 = 1; expect("R4=1 has no say", job(EU_FORM_BA, EU_SPHERICAL, 3, 3, 3, 0), s, EU_LAYERS_PACKED); }
  { eu_switches s = d; s.hybrid = 2; expect("HYBRID=2 has no say", job(EU_FORM_BA, EU_SPHERICAL, 3, 3, 3, 0), s, EU_LAYERS_PACKED); }
  { eu_switches s = d; s.direct = 1; expect("DIRECT=1 has no say", job(EU_FORM_BA, EU_CUBEMAP, 2, 4, 4, 1), s, EU_LAYERS_PACKED); }
  { eu_switches s = d; s.layers_max = 1; expect("LAYERS_MAX=1 has no say", job(EU_FORM_BA, EU_CUBEMAP, 2, 4, 4, 1), s, EU_LAYERS_PACKED); }
  // one job per reason for the general form
  { eu_render_params p = job(EU_FORM_BA, EU_SPHERICAL, 3, 3, 3, 0); p.src.mask_paint = 1; expect("mask_paint", p, d, EU_LAYERS_GENERAL); }
  { eu_switches s = d; s.force_general = 1; expect("EU_HIP_KERNEL=1", job(EU_FORM_BA, EU_SPHERICAL, 3, 3, 3, 0), s, EU_LAYERS_GENERAL); }
  { eu_switches s = d; s.force_general = 1; expect("EU_HIP_KERNEL=1, twined", job(EU_FORM_BCA, EU_CUBEMAP, 1, 3, 3, 1), s, EU_LAYERS_GENERAL); }
  { eu_render_params p = job(EU_FORM_BA, EU_SPHERICAL, 3, 3, 3, 0); p.src.has_lcp = 1; expect("has_lcp", p, d, EU_LAYERS_GENERAL); }
  expect("nch_out != nch (3 -> 4)", job(EU_FORM_BA, EU_SPHERICAL, 1, 3, 4, 0), d, EU_LAYERS_GENERAL);
  expect("nch_out != nch (4 -> 1), twined", job(EU_FORM_BA, EU_CUBEMAP, 1, 4, 1, 1), d, EU_LAYERS_GENERAL);
  expect("degree 0", job(EU_FORM_BA, EU_SPHERICAL, 0, 3, 3, 0), d, EU_LAYERS_GENERAL);
  expect("degree 4", job(EU_FORM_BA, EU_SPHERICAL, 4, 3, 3, 0), d, EU_LAYERS_GENERAL);
  expect("degree 9", job(EU_FORM_BCA, EU_BIATAN6, 9, 3, 3, 0), d, EU_LAYERS_GENERAL);
  expect("fisheye target", job(EU_FORM_FISH, EU_SPHERICAL, 3, 3, 3, 0), d, EU_LAYERS_GENERAL);
  expect("stereographic target", job(EU_FORM_STER, EU_SPHERICAL, 1, 3, 3, 1), d, EU_LAYERS_GENERAL);
  expect("rectilinear source", job(EU_FORM_BA, EU_RECTILINEAR, 1, 3, 3, 0), d, EU_LAYERS_GENERAL);
  expect("fisheye source", job(EU_FORM_BA, EU_FISHEYE, 1, 4, 4, 1), d, EU_LAYERS_GENERAL);
  { eu_render_params p = job(EU_FORM_BA, EU_SPHERICAL, 3, 3, 3, 0); p.src.es0 = 4; expect("texels not dense", p, d, EU_LAYERS_GENERAL); }
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
                    if (eu_select_layer_path(job(form, prj, deg, nch, nch, twine), s) != EU_LAYERS_GENERAL) {
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
  unsetenv("EU_HIP_LAYERS_MAX");
  check(eu_read_switches().layers_max == EU_LAYERS_MAX && EU_LAYERS_MAX == 4, "EU_HIP_LAYERS_MAX unset: 4");
  setenv("EU_HIP_LAYERS_MAX", "", 1);
  check(eu_read_switches().layers_max == EU_LAYERS_MAX, "EU_HIP_LAYERS_MAX empty: the default");
  setenv("EU_HIP_LAYERS_MAX", "16", 1);
  check(eu_read_switches().layers_max == 16, "EU_HIP_LAYERS_MAX=16");
  setenv("EU_HIP_LAYERS_MAX", "0", 1);
  check(eu_read_switches().layers_max == 0, "EU_HIP_LAYERS_MAX=0 is all");
  setenv("EU_HIP_LAYERS_MAX", "-3", 1);
  check(eu_read_switches().layers_max == 0, "EU_HIP_LAYERS_MAX=-3 is all");
  // the other switches are read as before
  setenv("EU_HIP_KERNEL", "1", 1);
  check(eu_read_switches().force_general == 1 && eu_read_switches().views_max_kb == EU_VIEWS_MAX_KB, "the other switches");
  unsetenv("EU_HIP_KERNEL");
  unsetenv("EU_HIP_LAYERS_MAX");
}

// every layer of a list of L is walked exactly once, in order: launches of `max` layers (0: all), and inside a
// twined launch groups of G
void walk(int L, int max, int G)
{
  const int per = eu_layers_per_launch(L, max), launches = eu_layers_launches(L, max);
  int next = 0, seen_launches = 0, ok = 1;
  for (int c0 = 0; c0 < L; c0 += per) {
    const int nl = L - c0 < per ? L - c0 : per;
    seen_launches++;
    ok = ok && nl >= 1 && (max <= 0 || nl <= max);
    const int groups = eu_layers_groups(nl, G);
    int in_launch = 0;
    for (int g = 0; g < groups; g++) {
      const int n = eu_layers_in_group(nl, g, G);
      ok = ok && n >= 1 && n <= G && (g + 1 == groups || n == G);
      for (int j = 0; j < n; j++) { ok = ok && c0 + g * G + j == next; next++; in_launch++; }
    }
    ok = ok && in_launch == nl && eu_layers_in_group(nl, groups, G) == 0;
  }
  ok = ok && next == L && seen_launches == launches;
  char what[96];
  snprintf(what, sizeof what, "EU_HIP_LAYERS_MAX %d, groups of %d, %d layers: %d launches", max, G, L, launches);
  check(ok, what);
}

void test_chunks()
{
  const int G = EU_LAYERS_GROUP;
  check(G == 1 || G == 2 || G == 4, "EU_LAYERS_GROUP is 1, 2 or 4");
  printf("EU_LAYERS_GROUP %d\n", G);
  const int maxes[6] = { 0, 1, 2, 3, 4, 8 };
  const int groups[4] = { G, 1, 2, 4 };
  for (int max : maxes)
    for (int g : groups) {
      const int counts[9] = { 0, 1, g, g + 1, 2 * g + 1, max, max + 1, 2 * max + 1, 17 };
      for (int L : counts) walk(L, max, g);
    }
  check(eu_layers_launches(0, 0) == 0 && eu_layers_launches(0, 4) == 0, "no layer, no launch");
  check(eu_layers_launches(9, 0) == 1 && eu_layers_per_launch(9, 0) == 9, "EU_HIP_LAYERS_MAX 0: all layers in one launch");
  check(eu_layers_launches(9, EU_LAYERS_MAX) == 3 && eu_layers_launches(4, EU_LAYERS_MAX) == 1, "EU_HIP_LAYERS_MAX by default: four at a time");
  check(eu_layers_launches(9, 4) == 3 && eu_layers_per_launch(9, 4) == 4, "nine layers, four at a time: three launches");
  check(eu_layers_launches(8, 8) == 1 && eu_layers_launches(9, 8) == 2, "max and max + 1");
  check(eu_layers_groups(0, 2) == 0 && eu_layers_groups(1, 2) == 1 && eu_layers_groups(2, 2) == 1 &&
        eu_layers_groups(3, 2) == 2 && eu_layers_groups(5, 2) == 3, "groups of two: 0, 1, G, G + 1, 2 G + 1 layers");
  check(eu_layers_in_group(5, 0, 2) == 2 && eu_layers_in_group(5, 2, 2) == 1 && eu_layers_in_group(5, 3, 2) == 0,
        "the last group is partial, the one behind it empty");
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
