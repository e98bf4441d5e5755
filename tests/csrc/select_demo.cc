// Host test of envutil_amd/csrc/eu_select.h: hand-made jobs and switch values in, the chosen path out; the
// run splitter on hand-made segment flags. The expected values were read off the launchers as they were
// before the choice moved into eu_select.h (launch_render's cascade of eu_launch_render4 / eu_launch_render2
// refusals). Prints one line per check; exit status 0 when all hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../envutil_amd/csrc/eu_select.h"

namespace {
int failures = 0;
void check(bool ok, const char *what)
{
  printf("%s: %s\n", ok ? "ok" : "FAILED", what);
  if (!ok) failures++;
}

const char *name(eu_path p)
{
  switch (p) {
    case EU_PATH_GENERAL: return "general";
    case EU_PATH_GENERAL_DIRECT: return "general-direct";
    case EU_PATH_PACKED: return "packed";
    case EU_PATH_PACKED_RUNS: return "packed-runs";
    case EU_PATH_STAGED: return "staged";
  }
  return "?";
}

void expect(const char *what, const eu_render_params &p, const eu_switches &sw, eu_path want, bool staged_allowed = true)
{
  const eu_path got = eu_select_path(p, sw, staged_allowed);
  printf("%s: %s -> %s (expected %s)\n", got == want ? "ok" : "FAILED", what, name(got), name(want));
  if (got != want) failures++;
}

// the library's behaviour with no EU_HIP_* variable set
eu_switches defaults()
{
  eu_switches s;
  s.force_general = 0; s.hybrid = 1; s.r4 = -1; s.colmajor = -1; s.rej = 0; s.colplan = 1;
  s.share = EU_SHARE_FACES | EU_SHARE_MIRRORS; s.direct = 0; s.iir_stream = 7;
  return s;
}
eu_switches with_r4(int v) { eu_switches s = defaults(); s.r4 = v; return s; }
eu_switches with_hybrid(int v) { eu_switches s = defaults(); s.hybrid = v; return s; }
eu_switches with_kernel1() { eu_switches s = defaults(); s.force_general = 1; return s; }

// one source of src_w texels per row (plus a frame of 8) rendered into a W x H target
eu_render_params job(int src_prj, int src_w, int degree, int nch, int form, int norm, int W, int H)
{
  eu_render_params p;
  memset(&p, 0, sizeof p);
  p.width = W; p.height = H; p.row_begin = 0; p.row_end = H;
  p.form = form; p.norm_mode = norm; p.nch = p.nch_out = nch;
  p.tab_finite = 1;
  p.src.prj = src_prj; p.src.nch = nch; p.src.degree = degree;
  p.src.es0 = nch; p.src.es1 = (long long)nch * (src_w + 8);
  p.src.brighten = 1.0f;
  if (src_prj == EU_SPHERICAL) {                 // a full sphere
    p.src.always_hit = 1;
    p.src.tex_x0 = -3.141592653589793; p.src.tex_y0 = -1.5707963267948966;
    p.src.ext_w = 6.2831855f; p.src.ext_h = 3.1415927f;
  }
  return p;
}
eu_render_params twined(eu_render_params p, int norm) { p.twine = 1; p.ntaps = 9; p.norm_mode = norm; return p; }

// BASELINE's jobs (bench.py WORKLOADS), one facet each
eu_render_params headline() { return job(EU_SPHERICAL, 16384, 3, 3, EU_FORM_BA, EU_NORM_NONE, 4096, 24576); }
eu_render_params config1() { return job(EU_SPHERICAL, 2048, 1, 3, EU_FORM_BA, EU_NORM_NONE, 1024, 1024); }
eu_render_params config2() { return job(EU_SPHERICAL, 8192, 1, 3, EU_FORM_BA, EU_NORM_NONE, 2048, 12288); }
eu_render_params config3() { return job(EU_CUBEMAP, 2048, 3, 3, EU_FORM_BCA, EU_NORM_NONE, 16384, 8192); }
eu_render_params config4() { return twined(job(EU_SPHERICAL, 32768, 1, 3, EU_FORM_BCA, EU_NORM_NONE, 32768, 16384), EU_NORM_NONE); }
eu_render_params config5_facet()
{
  eu_render_params p = job(EU_FISHEYE, 8192, 1, 4, EU_FORM_BCA, EU_NORM_NONE, 16384, 8192);
  p.src.has_lcp = 1;
  return p;
}

void test_paths()
{
  const eu_switches d = defaults();
  // ---- the headline: lat/lon, cubic, upright cubemap target ----
  expect("headline", headline(), d, EU_PATH_STAGED);
  expect("headline, plan not worth staging", headline(), d, EU_PATH_PACKED_RUNS, false);
  expect("headline R4=0", headline(), with_r4(0), EU_PATH_PACKED_RUNS);
  expect("headline R4=1", headline(), with_r4(1), EU_PATH_STAGED);
  expect("headline R4=2", headline(), with_r4(2), EU_PATH_STAGED);
  expect("headline KERNEL=1", headline(), with_kernel1(), EU_PATH_GENERAL);
  expect("headline HYBRID=0", headline(), with_hybrid(0), EU_PATH_STAGED);
  expect("headline HYBRID=2", headline(), with_hybrid(2), EU_PATH_STAGED);
  { eu_switches s = with_hybrid(0); s.r4 = 0; expect("headline HYBRID=0 R4=0", headline(), s, EU_PATH_PACKED); }
  { eu_switches s = with_kernel1(); s.r4 = 1; expect("headline KERNEL=1 R4=1", headline(), s, EU_PATH_GENERAL); }
  // the switches that do not take part in the choice
  { eu_switches s = d; s.colmajor = 0; expect("headline COLMAJOR=0", headline(), s, EU_PATH_STAGED); }
  { eu_switches s = d; s.colmajor = 1; expect("headline COLMAJOR=1", headline(), s, EU_PATH_STAGED); }
  { eu_switches s = d; s.rej = 1; expect("headline REJ=1", headline(), s, EU_PATH_STAGED); }
  { eu_switches s = d; s.rej = 2; expect("headline REJ=2", headline(), s, EU_PATH_STAGED); }
  { eu_switches s = d; s.colplan = 0; expect("headline COLPLAN=0", headline(), s, EU_PATH_STAGED); }
  { eu_switches s = d; s.share = 0; expect("headline SHARE=0", headline(), s, EU_PATH_STAGED); }
  { eu_switches s = d; s.share = EU_SHARE_MIRRORS; expect("headline SHARE=m", headline(), s, EU_PATH_STAGED); }
  { eu_switches s = d; s.share = EU_SHARE_FACES; expect("headline SHARE=f", headline(), s, EU_PATH_STAGED); }
  { eu_switches s = d; s.direct = 1; expect("headline DIRECT=1", headline(), s, EU_PATH_STAGED); }
  { eu_switches s = d; s.iir_stream = 0; expect("headline IIR_STREAM=0", headline(), s, EU_PATH_STAGED); }
  // ---- configs 1 and 2: lat/lon, bilinear ----
  expect("config1", config1(), d, EU_PATH_PACKED);
  expect("config1 R4=0", config1(), with_r4(0), EU_PATH_PACKED);
  expect("config1 R4=1", config1(), with_r4(1), EU_PATH_STAGED);
  expect("config1 HYBRID=2", config1(), with_hybrid(2), EU_PATH_PACKED_RUNS);
  expect("config1 HYBRID=0", config1(), with_hybrid(0), EU_PATH_PACKED);
  expect("config1 KERNEL=1", config1(), with_kernel1(), EU_PATH_GENERAL);
  expect("config2", config2(), d, EU_PATH_PACKED);
  expect("config2 R4=1", config2(), with_r4(1), EU_PATH_STAGED);
  // ---- config 3: cube source, cubic ----
  expect("config3", config3(), d, EU_PATH_STAGED);
  expect("config3 R4=0", config3(), with_r4(0), EU_PATH_PACKED);
  expect("config3 R4=1", config3(), with_r4(1), EU_PATH_STAGED);
  expect("config3 HYBRID=2 R4=0", config3(), [] { eu_switches s = with_hybrid(2); s.r4 = 0; return s; }(), EU_PATH_PACKED);
  expect("config3 KERNEL=1", config3(), with_kernel1(), EU_PATH_GENERAL);
  { eu_render_params p = config3(); p.src.prj = EU_BIATAN6; expect("config3 from a biatan6 source", p, d, EU_PATH_STAGED); }
  { eu_render_params p = config3(); p.src.degree = 2; expect("config3 quadratic", p, d, EU_PATH_STAGED); }
  { eu_render_params p = config3(); p.src.degree = 1; expect("config3 bilinear", p, d, EU_PATH_PACKED); }
  { eu_render_params p = config3(); p.norm_mode = EU_NORM_DIV; p.form = EU_FORM_BA; expect("cube source, normalised BA target", p, d, EU_PATH_STAGED); }
  { eu_render_params p = config3(); p.norm_mode = EU_NORM_CYL; expect("cube source, cylindrical normalisation", p, d, EU_PATH_PACKED); }
  // a downscaling job of 1024 wave tiles, every one of them for the work list (tests/test_gpu_worklist.py): staged without a switch
  expect("cube source 1024, cubic, spherical 512 x 256", job(EU_CUBEMAP, 1024, 3, 3, EU_FORM_BCA, EU_NORM_NONE, 512, 256), d, EU_PATH_STAGED);
  // ---- config 4: twining ----
  expect("config4", config4(), d, EU_PATH_PACKED);
  expect("config4 R4=1", config4(), with_r4(1), EU_PATH_PACKED);
  expect("config4 HYBRID=2", config4(), with_hybrid(2), EU_PATH_PACKED);
  expect("headline twined", twined(headline(), EU_NORM_DIV), d, EU_PATH_PACKED);
  expect("headline twined R4=1", twined(headline(), EU_NORM_DIV), with_r4(1), EU_PATH_PACKED);
  expect("config3 twined", twined(config3(), EU_NORM_NONE), d, EU_PATH_PACKED);
  // ---- config 5's facets: fisheye with a lens polynomial ----
  expect("config5 facet", config5_facet(), d, EU_PATH_GENERAL);
  expect("config5 facet R4=1", config5_facet(), with_r4(1), EU_PATH_GENERAL);
  expect("config5 facet HYBRID=2", config5_facet(), with_hybrid(2), EU_PATH_GENERAL);
  // ---- --mask_for: the general kernel's inline evaluation, whatever the switches say ----
  for (int paint = 1; paint <= 2; paint++) {
    eu_render_params p = headline();
    p.src.mask_paint = paint;
    expect("mask_paint", p, d, EU_PATH_GENERAL_DIRECT);
    expect("mask_paint R4=1", p, with_r4(1), EU_PATH_GENERAL_DIRECT);
    expect("mask_paint KERNEL=1", p, with_kernel1(), EU_PATH_GENERAL_DIRECT);
    eu_render_params c = config3();
    c.src.mask_paint = paint;
    expect("mask_paint, cube source", c, d, EU_PATH_GENERAL_DIRECT);
  }
  // ---- outside the packed kernels' coverage: the general kernel ----
  for (int r4 = -1; r4 <= 1; r4++) {
    const eu_switches s = with_r4(r4);
    { eu_render_params p = headline(); p.stage = 1; expect("stage 1", p, s, EU_PATH_GENERAL); }
    { eu_render_params p = config3(); p.stage = 2; expect("stage 2, cube source", p, s, EU_PATH_GENERAL); }
    { eu_render_params p = headline(); p.nch_out = 1; expect("nch_out != nch", p, s, EU_PATH_GENERAL); }
    { eu_render_params p = headline(); p.src.has_lcp = 1; expect("has_lcp", p, s, EU_PATH_GENERAL); }
    { eu_render_params p = headline(); p.src.degree = 0; expect("degree 0", p, s, EU_PATH_GENERAL); }
    { eu_render_params p = headline(); p.src.degree = 4; expect("degree 4", p, s, EU_PATH_GENERAL); }
    { eu_render_params p = config3(); p.src.degree = 4; expect("degree 4, cube source", p, s, EU_PATH_GENERAL); }
    { eu_render_params p = headline(); p.form = EU_FORM_FISH; expect("fisheye target", p, s, EU_PATH_GENERAL); }
    { eu_render_params p = headline(); p.form = EU_FORM_STER; expect("stereographic target", p, s, EU_PATH_GENERAL); }
    { eu_render_params p = config3(); p.form = EU_FORM_FISH; expect("fisheye target, cube source", p, s, EU_PATH_GENERAL); }
    { eu_render_params p = headline(); p.form = EU_FORM_GENERIC; expect("generic stepper", p, s, EU_PATH_GENERAL); }
    { eu_render_params p = headline(); p.src.es0 = 4; expect("es0 != nch", p, s, EU_PATH_GENERAL); }
    { eu_render_params p = headline(); p.src.prj = EU_RECTILINEAR; p.src.always_hit = 0; expect("rectilinear source", p, s, EU_PATH_GENERAL); }
    { eu_render_params p = headline(); p.src.prj = EU_FISHEYE; p.src.always_hit = 0; expect("fisheye source", p, s, EU_PATH_GENERAL); }
  }
  expect("fisheye target HYBRID=2", [] { eu_render_params p = headline(); p.form = EU_FORM_FISH; return p; }(), with_hybrid(2), EU_PATH_GENERAL);
  // ---- inside the packed kernels' coverage, outside the staged kernels' ----
  for (int nch = 1; nch <= 2; nch++) {
    eu_render_params p = headline();
    p.nch = p.nch_out = p.src.nch = nch; p.src.es0 = nch;
    expect("nch 1 / 2", p, d, EU_PATH_PACKED_RUNS);
    expect("nch 1 / 2 R4=1", p, with_r4(1), EU_PATH_PACKED_RUNS);
    eu_render_params c = config3();
    c.nch = c.nch_out = c.src.nch = nch; c.src.es0 = nch;
    expect("nch 1 / 2, cube source R4=1", c, with_r4(1), EU_PATH_PACKED);
    eu_render_params b = config1();
    b.nch = b.nch_out = b.src.nch = nch; b.src.es0 = nch;
    expect("nch 1 / 2, bilinear R4=1", b, with_r4(1), EU_PATH_PACKED);
  }
  { eu_render_params p = headline(); p.nch = p.nch_out = p.src.nch = 4; p.src.es0 = 4; expect("nch 4", p, d, EU_PATH_STAGED); }
  { eu_render_params p = headline(); p.nch = p.nch_out = p.src.nch = 5; p.src.es0 = 5; expect("nch 5", p, with_r4(1), EU_PATH_GENERAL); }
  {
    eu_render_params p = headline();
    p.src.es1 = 1ll << 29;                       // es1 * 4 == 2^31
    expect("es1 * 4 >= 2^31", p, d, EU_PATH_PACKED_RUNS);
    expect("es1 * 4 >= 2^31 R4=1", p, with_r4(1), EU_PATH_PACKED_RUNS);
    p.src.es1 = (1ll << 29) - 1;
    expect("es1 * 4 < 2^31", p, d, EU_PATH_STAGED);
    eu_render_params c = config3();
    c.src.es1 = 1ll << 29;
    expect("es1 * 4 >= 2^31, cube source", c, d, EU_PATH_PACKED);
  }
  {
    eu_render_params c = config3();
    c.row_end = c.height = 65535 * 8 * 4 * 8;    // as many tile rows as the staged grid takes
    expect("65535 * 8 units of tile rows", c, d, EU_PATH_STAGED);
    c.row_end = c.height = 65535 * 8 * 4 * 8 + 1;
    expect("one tile row more", c, d, EU_PATH_PACKED);
  }
  // ---- a band-interleaved share of the headline: not the default staged profile, split only if the runs are long ----
  {
    eu_render_params p = headline();
    p.band_shift = 6; p.band_count = 8; p.band_index = 1; p.row_end = 3072;
    expect("band-interleaved share", p, d, EU_PATH_PACKED_RUNS);
    expect("band-interleaved share R4=1", p, with_r4(1), EU_PATH_STAGED);
    expect("band-interleaved share R4=0 HYBRID=0", p, [] { eu_switches s = with_hybrid(0); s.r4 = 0; return s; }(), EU_PATH_PACKED);
    check(!eu_staged_default(p) && !eu_staged_fast_profile(p), "band-interleaved share: neither staged profile");
  }
  // ---- lat/lon jobs that are not the default staged profile ----
  { eu_render_params p = headline(); p.src.brighten = 2.0f; expect("brighten != 1", p, d, EU_PATH_PACKED_RUNS); expect("brighten != 1 R4=1", p, with_r4(1), EU_PATH_STAGED); }
  { eu_render_params p = headline(); p.src.always_hit = 0; expect("a partial sphere", p, d, EU_PATH_PACKED_RUNS); }
  { eu_render_params p = headline(); p.norm_mode = EU_NORM_DIV; expect("normalised BA target", p, d, EU_PATH_PACKED); expect("normalised BA target R4=1", p, with_r4(1), EU_PATH_STAGED); }
  { eu_render_params p = headline(); p.form = EU_FORM_BCA; expect("lat/lon to lat/lon, cubic", p, d, EU_PATH_PACKED_RUNS); expect("lat/lon to lat/lon, cubic R4=1", p, with_r4(1), EU_PATH_STAGED); }
  { eu_render_params p = headline(); p.src.degree = 2; expect("headline quadratic", p, d, EU_PATH_STAGED); }
}

// degrees 0 and 4 to 9 have no packed and no staged kernel (eu_packed_covers_source): whatever EU_HIP_R4, EU_HIP_HYBRID,
// EU_HIP_KERNEL and EU_HIP_DIRECT say, and whatever the plan said, BASELINE's jobs at those degrees are the general kernel's
void test_high_degrees()
{
  const eu_render_params base[6] = { headline(), config1(), config3(), config4(), twined(headline(), EU_NORM_DIV),
                                     [] { eu_render_params p = config3(); p.src.prj = EU_BIATAN6; return p; }() };
  const int degrees[7] = { 0, 4, 5, 6, 7, 8, 9 };
  int n = 0, bad = 0;
  for (const eu_render_params &b : base)
    for (int deg : degrees)
      for (int nch = 1; nch <= 4; nch++)
        for (int r4 = -1; r4 <= 2; r4++)
          for (int hybrid = 0; hybrid <= 2; hybrid++)
            for (int kernel = 0; kernel <= 1; kernel++)
              for (int direct = 0; direct <= 1; direct++)
                for (int allowed = 0; allowed <= 1; allowed++) {
                  eu_render_params p = b;
                  p.src.degree = deg;
                  p.nch = p.nch_out = p.src.nch = nch; p.src.es0 = nch;
                  eu_switches s = defaults();
                  s.r4 = r4; s.hybrid = hybrid; s.force_general = kernel; s.direct = direct;
                  n++;
                  if (eu_select_path(p, s, allowed != 0) != EU_PATH_GENERAL || eu_packed_covers(p) || eu_staged_covers(p) ||
                      eu_packed_covers_source(p.src, p.nch, p.nch_out)) {
                    bad++;
                    printf("FAILED: degree %d nch %d R4=%d HYBRID=%d KERNEL=%d DIRECT=%d staged_allowed %d -> %s\n", deg, nch, r4,
                           hybrid, kernel, direct, allowed, name(eu_select_path(p, s, allowed != 0)));
                  }
                }
  char what[96];
  snprintf(what, sizeof what, "high degrees: %d combinations, all general", n);
  check(bad == 0 && n == 6 * 7 * 4 * 4 * 3 * 2 * 2 * 2, what);
}

void test_profiles()
{
  check(eu_staged_default(headline()) && eu_staged_fast_profile(headline()), "headline: default staged job, FAST profile");
  check(!eu_staged_default(config1()) && eu_staged_fast_profile(config1()), "config1: FAST profile, not a default staged job (bilinear)");
  check(!eu_staged_default(config3()) && !eu_staged_fast_profile(config3()), "config3: neither (BCA form)");
  { eu_render_params p = headline(); p.tab_finite = 0; check(eu_staged_default(p) && !eu_staged_fast_profile(p), "tables with a non-finite entry: not FAST"); }
  { eu_render_params p = headline(); p.src.tex_x0 = 1e-7; check(!eu_staged_fast_profile(p), "extent origin below 2^-20: not FAST"); }
  { eu_render_params p = headline(); p.src.tex_y0 = -2e6; check(!eu_staged_fast_profile(p), "extent origin above 2^20: not FAST"); }
  { eu_render_params p = headline(); p.src.tex_x0 = 0.0; p.src.tex_y0 = -0.0; check(eu_staged_fast_profile(p), "extent origin 0: FAST"); }
  { eu_render_params p = headline(); p.src.ext_w = 0x1p21f; check(!eu_staged_fast_profile(p), "extent above 2^20: not FAST"); }
  { eu_render_params p = headline(); p.src.ext_h = 0x1p-21f; check(!eu_staged_fast_profile(p), "extent below 2^-20: not FAST"); }
  { eu_render_params p = headline(); p.src.ext_w = 0x1p20f; p.src.ext_h = 0x1p-20f; check(eu_staged_fast_profile(p), "extents at the limits: FAST"); }
  { eu_render_params p = headline(); p.src.brighten = 0.5f; check(!eu_staged_default(p) && !eu_staged_fast_profile(p), "brighten: neither"); }
  { eu_render_params p = headline(); p.src.always_hit = 0; check(!eu_staged_default(p) && !eu_staged_fast_profile(p), "partial sphere: neither"); }
  { eu_render_params p = twined(headline(), EU_NORM_DIV); check(!eu_staged_default(p) && !eu_staged_fast_profile(p), "twined: neither"); }
  check(eu_staged_covers(headline()) && eu_packed_covers(headline()), "headline: both kernels cover it");
  check(!eu_staged_covers(config4()) && eu_packed_covers(config4()), "config4: packed only");
  check(!eu_staged_covers(config5_facet()) && !eu_packed_covers(config5_facet()), "config5 facet: neither");
  // a tile id of the work list is an int: the tallest strip the staged kernels take (EU_STAGED_MAX_TILES_Y tile rows)
  // at 1024 tile columns has 2147450880 tiles, at 1025 columns more than INT_MAX
  {
    eu_render_params p = headline();
    p.height = p.row_end = EU_STAGED_MAX_TILES_Y * EU_STAGED_TILE_ROWS;
    p.width = 1024 * 16;
    check(eu_staged_tiles(p.width, p.row_begin, p.row_end) == 2147450880ull && eu_staged_covers(p), "2147450880 tiles: staged");
    p.width = 1024 * 16 + 1;
    check(eu_staged_tiles(p.width, p.row_begin, p.row_end) > (unsigned long long)INT_MAX && !eu_staged_covers(p) && eu_packed_covers(p),
          "more tiles than an int holds: not staged");
    expect("more tiles than an int holds", p, defaults(), EU_PATH_PACKED_RUNS);
    expect("more tiles than an int holds, R4=1", p, with_r4(1), EU_PATH_PACKED_RUNS);
    p.row_end = p.height = p.height + 1;
    p.width = 16;
    check(!eu_staged_covers(p), "one tile row more than the grid has: not staged");
  }
  // the post-plan test: cubic / quadratic and column plans on at least half of the tile rows
  check(eu_staged_worth(3, 3072, 3072), "worth: every tile row planned");
  check(eu_staged_worth(3, 1536, 3072) && eu_staged_worth(2, 1536, 3072), "worth: half of the tile rows planned");
  check(!eu_staged_worth(3, 1535, 3072), "not worth: less than half");
  check(!eu_staged_worth(3, 0, 1024), "not worth: no column plans (a rotated target)");
  check(!eu_staged_worth(1, 3072, 3072), "not worth: bilinear");
}

bool same(const std::vector<eu_run> &got, const std::vector<eu_run> &want)
{
  if (got.size() != want.size()) return false;
  for (size_t i = 0; i < got.size(); i++)
    if (got[i].row_begin != want[i].row_begin || got[i].row_end != want[i].row_end || got[i].layout != want[i].layout) return false;
  return true;
}

void test_runs()
{
  // the headline's frame: 48 segments of 512 rows, the inner halves of the two polar faces (rows 8192 .. 16383)
  // want tiles
  std::vector<unsigned char> fl(48, 0);
  for (int k = 18; k < 22; k++) fl[(size_t)k] = fl[(size_t)k + 8] = 1;
  const int n = (int)fl.size();
  eu_render_params p = headline();
  check(same(eu_split_runs(fl.data(), n, p, false),
             { { 0, 9216, 1 }, { 9216, 11264, 2 }, { 11264, 13312, 1 }, { 13312, 15360, 2 }, { 15360, 24576, 1 } }),
        "whole frame: 5 runs");
  check(same(eu_split_runs(fl.data(), n, p, true),
             { { 0, 9216, 1 }, { 9216, 11264, 2 }, { 11264, 13312, 1 }, { 13312, 15360, 2 }, { 15360, 24576, 1 } }),
        "whole frame, HYBRID=2: the same 5 runs");
  // contiguous strips (one device's or one chunk's rows)
  p.row_begin = 8192; p.row_end = 12288;
  check(same(eu_split_runs(fl.data(), n, p, false), { { 8192, 9216, 1 }, { 9216, 11264, 2 }, { 11264, 12288, 1 } }), "a polar face: 3 runs");
  p.row_begin = 9000; p.row_end = 12000;
  check(same(eu_split_runs(fl.data(), n, p, false), { { 9000, 9216, 1 }, { 9216, 11264, 2 }, { 11264, 12000, 1 } }),
        "a strip that starts and ends inside a 64-row chunk: 3 runs");
  p.row_begin = 9216; p.row_end = 11264;
  check(same(eu_split_runs(fl.data(), n, p, false), { { 9216, 11264, 2 } }), "a strip of tile rows only: 1 run, tiles");
  p.row_begin = 10000; p.row_end = 14000;
  check(same(eu_split_runs(fl.data(), n, p, false), { { 10000, 11264, 2 }, { 11264, 13312, 1 }, { 13312, 14000, 2 } }), "across both inner halves: 3 runs");
  p.row_begin = 0; p.row_end = 8192;
  check(eu_split_runs(fl.data(), n, p, false).empty() && eu_split_runs(fl.data(), n, p, true).empty(), "a strip without tile rows: one launch");
  p.row_begin = 9000; p.row_end = 15500;
  check(eu_split_runs(fl.data(), n, p, false).empty(), "5 runs, the shortest below a segment: one launch");
  check(same(eu_split_runs(fl.data(), n, p, true),
             { { 9000, 9216, 1 }, { 9216, 11264, 2 }, { 11264, 13312, 1 }, { 13312, 15360, 2 }, { 15360, 15500, 1 } }),
        "the same, HYBRID=2: 5 runs");
  // a band-interleaved share: bands of 64 rows dealt to 8 parts - local chunk k lies in segment k
  p = headline();
  p.band_shift = 6; p.band_count = 8; p.band_index = 1; p.row_begin = 0; p.row_end = 3072;
  check(eu_split_runs(fl.data(), n, p, false).empty(), "band-interleaved share: 5 short runs, one launch");
  check(same(eu_split_runs(fl.data(), n, p, true),
             { { 0, 1152, 1 }, { 1152, 1408, 2 }, { 1408, 1664, 1 }, { 1664, 1920, 2 }, { 1920, 3072, 1 } }),
        "band-interleaved share, HYBRID=2: 5 runs of local rows");
  // many short runs: the layout changes with every segment
  std::vector<unsigned char> alt(48, 0);
  for (int k = 1; k < 48; k += 2) alt[(size_t)k] = 1;
  p = headline();
  check(eu_split_runs(alt.data(), n, p, false).empty(), "48 runs: one launch");
  {
    const std::vector<eu_run> r = eu_split_runs(alt.data(), n, p, true);
    bool ok = r.size() == 48;
    for (size_t k = 0; ok && k < r.size(); k++)
      ok = r[k].row_begin == (int)k * 512 && r[k].row_end == (int)(k + 1) * 512 && r[k].layout == ((k & 1) ? 2 : 1);
    check(ok, "48 runs, HYBRID=2: a launch per segment");
  }
  p.row_begin = 0; p.row_end = 2048;
  check(same(eu_split_runs(alt.data(), n, p, false), { { 0, 512, 1 }, { 512, 1024, 2 }, { 1024, 1536, 1 }, { 1536, 2048, 2 } }),
        "4 runs of a whole segment each: split");
  p.row_begin = 0; p.row_end = 3072;
  check(eu_split_runs(alt.data(), n, p, false).empty(), "6 runs of a whole segment each: one launch");
  // no segment wants tiles, or no flags at all
  std::vector<unsigned char> none(48, 0);
  p = headline();
  check(eu_split_runs(none.data(), n, p, false).empty() && eu_split_runs(none.data(), n, p, true).empty(), "no tile segment: one launch");
  check(eu_split_runs(nullptr, 0, p, true).empty(), "no flags: one launch");
  // rows beyond the last flag use the last flag
  std::vector<unsigned char> few(20, 0);
  few[19] = 1;
  p.row_begin = 0; p.row_end = 24576;
  check(same(eu_split_runs(few.data(), 20, p, false), { { 0, 9728, 1 }, { 9728, 24576, 2 } }), "rows beyond the flags take the last one");
}

void set(const char *k, const char *v) { if (v) setenv(k, v, 1); else unsetenv(k); }

void test_read()
{
  static const char *names[] = { "EU_HIP_KERNEL", "EU_HIP_HYBRID", "EU_HIP_R4", "EU_HIP_COLMAJOR", "EU_HIP_REJ", "EU_HIP_COLPLAN",
                                 "EU_HIP_SHARE", "EU_HIP_DIRECT", "EU_HIP_IIR_STREAM" };
  for (const char *k : names) unsetenv(k);
  {
    const eu_switches s = eu_read_switches(), d = defaults();
    check(s.force_general == d.force_general && s.hybrid == d.hybrid && s.r4 == d.r4 && s.colmajor == d.colmajor && s.rej == d.rej &&
          s.colplan == d.colplan && s.share == d.share && s.direct == d.direct && s.iir_stream == d.iir_stream, "nothing set: the defaults");
  }
  set("EU_HIP_KERNEL", "1"); check(eu_read_switches().force_general == 1, "KERNEL=1");
  set("EU_HIP_KERNEL", "2"); check(eu_read_switches().force_general == 0, "KERNEL=2: not forced");
  set("EU_HIP_KERNEL", "");  check(eu_read_switches().force_general == 0, "KERNEL empty: not forced");
  set("EU_HIP_KERNEL", nullptr); check(eu_read_switches().force_general == 0, "KERNEL unset again: re-read on every call");
  set("EU_HIP_HYBRID", "0"); check(eu_read_switches().hybrid == 0, "HYBRID=0");
  set("EU_HIP_HYBRID", "2"); check(eu_read_switches().hybrid == 2, "HYBRID=2");
  set("EU_HIP_HYBRID", "1"); check(eu_read_switches().hybrid == 1, "HYBRID=1");
  set("EU_HIP_HYBRID", "x"); check(eu_read_switches().hybrid == 1, "HYBRID=x: the default");
  set("EU_HIP_R4", "0"); check(eu_read_switches().r4 == 0, "R4=0");
  set("EU_HIP_R4", "1"); check(eu_read_switches().r4 == 1, "R4=1");
  set("EU_HIP_R4", "");  check(eu_read_switches().r4 == 0, "R4 empty: atoi gives 0, never staged");
  set("EU_HIP_R4", "10"); check(eu_read_switches().r4 == 10, "R4=10: atoi, not the first character");
  set("EU_HIP_R4", nullptr); check(eu_read_switches().r4 == -1, "R4 unset");
  set("EU_HIP_COLMAJOR", "0"); check(eu_read_switches().colmajor == 0, "COLMAJOR=0");
  set("EU_HIP_COLMAJOR", "1"); check(eu_read_switches().colmajor == 1, "COLMAJOR=1");
  set("EU_HIP_COLMAJOR", "");  check(eu_read_switches().colmajor == -1, "COLMAJOR empty: as unset");
  set("EU_HIP_COLMAJOR", "-3"); check(eu_read_switches().colmajor == -3, "COLMAJOR=-3: negative, the job's own walk");
  set("EU_HIP_REJ", "1"); check(eu_read_switches().rej == 1, "REJ=1");
  set("EU_HIP_REJ", "2"); check(eu_read_switches().rej == 2, "REJ=2");
  set("EU_HIP_REJ", "0"); check(eu_read_switches().rej == 0, "REJ=0");
  set("EU_HIP_REJ", "3"); check(eu_read_switches().rej == 0, "REJ=3: off");
  set("EU_HIP_COLPLAN", "0"); check(eu_read_switches().colplan == 0, "COLPLAN=0");
  set("EU_HIP_COLPLAN", "1"); check(eu_read_switches().colplan == 1, "COLPLAN=1");
  set("EU_HIP_SHARE", "0"); check(eu_read_switches().share == 0, "SHARE=0");
  set("EU_HIP_SHARE", "m"); check(eu_read_switches().share == EU_SHARE_MIRRORS, "SHARE=m");
  set("EU_HIP_SHARE", "f"); check(eu_read_switches().share == EU_SHARE_FACES, "SHARE=f");
  set("EU_HIP_SHARE", "1"); check(eu_read_switches().share == (EU_SHARE_FACES | EU_SHARE_MIRRORS), "SHARE=1: both");
  set("EU_HIP_DIRECT", "1"); check(eu_read_switches().direct == 1, "DIRECT=1");
  set("EU_HIP_DIRECT", "0"); check(eu_read_switches().direct == 0, "DIRECT=0");
  set("EU_HIP_IIR_STREAM", "0"); check(eu_read_switches().iir_stream == 0, "IIR_STREAM=0");
  set("EU_HIP_IIR_STREAM", "3"); check(eu_read_switches().iir_stream == 3, "IIR_STREAM=3");
  set("EU_HIP_IIR_STREAM", "");  check(eu_read_switches().iir_stream == 0, "IIR_STREAM empty: atoi gives 0");
  for (const char *k : names) unsetenv(k);
}
}  // namespace

int main()
{
  test_paths();
  test_high_degrees();
  test_profiles();
  test_runs();
  test_read();
  printf(failures ? "%d checks FAILED\n" : "all ok\n", failures);
  return failures ? 1 : 0;
}
