// Host test of eu_select_ray_path() (envutil_amd/csrc/eu_select.h) and of the miss predicate of the ray path
// (envutil_amd/csrc/eu_ray_guard.h), both plain C++.
//   select_rays_demo            one job per reason for the general form, plus the packed cases, and the
//                               predicate over every exponent class in every component
//   select_rays_demo miss 3|9 HEX...  the predicate on groups of three or nine float bit patterns: a line
//                               of 0 or 1 per group
// Prints one line per check; exit status 0 when all hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../envutil_amd/csrc/eu_select.h"
#include "../../envutil_amd/csrc/eu_ray_guard.h"

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
  return s;
}

eu_rays_params job(int prj, int degree, int nch, int nch_out, int ninputs)
{
  eu_rays_params p;
  memset(&p, 0, sizeof p);
  p.width = 1000; p.height = 10; p.ninputs = ninputs; p.ntaps = ninputs == 9 ? 9 : 0;
  p.nch = nch; p.nch_out = nch_out;
  p.src.prj = prj; p.src.nch = nch; p.src.degree = degree; p.src.es0 = nch; p.src.es1 = 1024 * nch;
  p.src.brighten = 1.0f;
  return p;
}

void expect(const char *what, const eu_rays_params &p, const eu_switches &sw, eu_ray_path want)
{
  const eu_ray_path got = eu_select_ray_path(p, sw);
  printf("%s: %s -> %s\n", got == want ? "ok" : "FAILED", what, got == EU_RAYS_PACKED ? "packed" : "general");
  if (got != want) failures++;
}

void test_paths()
{
  const eu_switches d = defaults();
  // the packed form: lat/lon, cubemap and biatan6 sources, degrees 1-3, 1-4 channels, rays and ninepacks
  const int prjs[3] = { EU_SPHERICAL, EU_CUBEMAP, EU_BIATAN6 };
  for (int prj : prjs)
    for (int deg = 1; deg <= 3; deg++)
      for (int nch = 1; nch <= 4; nch++)
        for (int nin : { 3, 9 }) {
          char what[96];
          snprintf(what, sizeof what, "packed: prj %d degree %d nch %d ninputs %d", prj, deg, nch, nin);
          expect(what, job(prj, deg, nch, nch, nin), d, EU_RAYS_PACKED);
        }
  // switches that have no say
  { eu_switches s = d; s.r4 = 1; expect("R4=1 has no say", job(EU_SPHERICAL, 3, 3, 3, 3), s, EU_RAYS_PACKED); }
  { eu_switches s = d; s.r4 = 0; s.hybrid = 0; expect("R4=0 HYBRID=0 have no say", job(EU_SPHERICAL, 3, 3, 3, 3), s, EU_RAYS_PACKED); }
  { eu_switches s = d; s.direct = 1; expect("DIRECT=1 has no say", job(EU_CUBEMAP, 2, 4, 4, 9), s, EU_RAYS_PACKED); }
  // one job per reason for the general form
  { eu_rays_params p = job(EU_SPHERICAL, 3, 3, 3, 3); p.src.mask_paint = 1; expect("mask_paint", p, d, EU_RAYS_GENERAL); }
  { eu_switches s = d; s.force_general = 1; expect("EU_HIP_KERNEL=1", job(EU_SPHERICAL, 3, 3, 3, 3), s, EU_RAYS_GENERAL); }
  { eu_switches s = d; s.force_general = 1; expect("EU_HIP_KERNEL=1, ninepacks", job(EU_CUBEMAP, 1, 3, 3, 9), s, EU_RAYS_GENERAL); }
  { eu_rays_params p = job(EU_SPHERICAL, 3, 3, 3, 3); p.src.has_lcp = 1; expect("has_lcp", p, d, EU_RAYS_GENERAL); }
  expect("nch_out != nch (3 -> 4)", job(EU_SPHERICAL, 1, 3, 4, 3), d, EU_RAYS_GENERAL);
  expect("nch_out != nch (4 -> 1), ninepacks", job(EU_CUBEMAP, 1, 4, 1, 9), d, EU_RAYS_GENERAL);
  expect("degree 0", job(EU_SPHERICAL, 0, 3, 3, 3), d, EU_RAYS_GENERAL);
  expect("degree 4", job(EU_SPHERICAL, 4, 3, 3, 3), d, EU_RAYS_GENERAL);
  expect("degree 5", job(EU_BIATAN6, 5, 3, 3, 3), d, EU_RAYS_GENERAL);
  expect("rectilinear source", job(EU_RECTILINEAR, 1, 3, 3, 3), d, EU_RAYS_GENERAL);
  expect("cylindrical source", job(EU_CYLINDRICAL, 3, 3, 3, 3), d, EU_RAYS_GENERAL);
  expect("stereographic source", job(EU_STEREOGRAPHIC, 2, 3, 3, 3), d, EU_RAYS_GENERAL);
  expect("fisheye source", job(EU_FISHEYE, 1, 4, 4, 9), d, EU_RAYS_GENERAL);
  { eu_rays_params p = job(EU_SPHERICAL, 3, 3, 3, 3); p.src.es0 = 4; expect("texels not dense", p, d, EU_RAYS_GENERAL); }
  // eu_packed_covers() still asks the same of the source
  {
    eu_render_params r;
    memset(&r, 0, sizeof r);
    r.form = EU_FORM_BA; r.nch = r.nch_out = 3;
    r.src = job(EU_SPHERICAL, 3, 3, 3, 3).src;
    check(eu_packed_covers(r), "eu_packed_covers: a lat/lon cubic RGB job");
    r.stage = 1; check(!eu_packed_covers(r), "eu_packed_covers: not a stage output"); r.stage = 0;
    r.form = EU_FORM_FISH; check(!eu_packed_covers(r), "eu_packed_covers: not a fisheye target"); r.form = EU_FORM_BA;
    r.src.has_lcp = 1; check(!eu_packed_covers(r), "eu_packed_covers: not with a lens polynomial");
  }
}

// degrees 0 and 4 to 9: never the packed form, whatever the switches say
void test_high_degrees()
{
  const int prjs[3] = { EU_SPHERICAL, EU_CUBEMAP, EU_BIATAN6 };
  const int degrees[7] = { 0, 4, 5, 6, 7, 8, 9 };
  int n = 0, bad = 0;
  for (int prj : prjs)
    for (int deg : degrees)
      for (int nch = 1; nch <= 4; nch++)
        for (int nin : { 3, 9 })
          for (int r4 = -1; r4 <= 2; r4++)
            for (int hybrid = 0; hybrid <= 2; hybrid++)
              for (int kernel = 0; kernel <= 1; kernel++)
                for (int direct = 0; direct <= 1; direct++) {
                  eu_switches s = defaults();
                  s.r4 = r4; s.hybrid = hybrid; s.force_general = kernel; s.direct = direct;
                  n++;
                  if (eu_select_ray_path(job(prj, deg, nch, nch, nin), s) != EU_RAYS_GENERAL) {
                    bad++;
                    printf("FAILED: prj %d degree %d nch %d ninputs %d R4=%d HYBRID=%d KERNEL=%d DIRECT=%d -> packed\n", prj, deg, nch,
                           nin, r4, hybrid, kernel, direct);
                  }
                }
  char what[96];
  snprintf(what, sizeof what, "high degrees: %d combinations, all general", n);
  check(bad == 0 && n == 3 * 7 * 4 * 2 * 4 * 3 * 2 * 2, what);
}

float from_bits(uint32_t u) { float f; memcpy(&f, &u, sizeof f); return f; }

// every exponent class, both signs; `finite`: the class is a finite number, `zero`: +-0
struct cls { const char *name; uint32_t bits; bool finite, zero; };
const cls classes[] = {
  { "+0", 0x00000000u, true, true }, { "-0", 0x80000000u, true, true },
  { "+denormal min", 0x00000001u, true, false }, { "-denormal min", 0x80000001u, true, false },
  { "+denormal max", 0x007fffffu, true, false }, { "-denormal max", 0x807fffffu, true, false },
  { "+normal min", 0x00800000u, true, false }, { "-normal min", 0x80800000u, true, false },
  { "+1", 0x3f800000u, true, false }, { "-1", 0xbf800000u, true, false },
  { "+normal max", 0x7f7fffffu, true, false }, { "-normal max", 0xff7fffffu, true, false },
  { "+inf", 0x7f800000u, false, false }, { "-inf", 0xff800000u, false, false },
  { "+quiet NaN", 0x7fc00000u, false, false }, { "-quiet NaN", 0xffc00000u, false, false },
  { "+quiet NaN, payload", 0x7fffffffu, false, false }, { "-quiet NaN, payload", 0xffffffffu, false, false },
  { "+signalling NaN", 0x7f800001u, false, false }, { "-signalling NaN", 0xff800001u, false, false },
  { "+signalling NaN, payload", 0x7fbfffffu, false, false }, { "-signalling NaN, payload", 0xffbfffffu, false, false },
};

void test_predicate()
{
  int bad3 = 0, bad9 = 0, n3 = 0, n9 = 0;
  // a ray: every class in one component, the other two zero / ordinary
  for (int comp = 0; comp < 3; comp++)
    for (const cls &c : classes)
      for (int others = 0; others < 3; others++) {        // the other components: +0, -0, 0.5
        float r[3];
        const uint32_t ob = others == 0 ? 0u : others == 1 ? 0x80000000u : 0x3f000000u;
        for (int k = 0; k < 3; k++) r[k] = from_bits(k == comp ? c.bits : ob);
        const bool want = !c.finite || (c.zero && others < 2);
        n3++;
        if ((eu_ray_miss(r[0], r[1], r[2]) != 0) != want) {
          bad3++;
          printf("FAILED: ray, %s in component %d, others %d\n", c.name, comp, others);
        }
      }
  // a ninepack: every class in one of the nine, the rest an ordinary ninepack
  for (int comp = 0; comp < 9; comp++)
    for (const cls &c : classes) {
      float in[9] = { 0.25f, -0.5f, 1.0f, 0.26f, -0.5f, 1.0f, 0.25f, -0.49f, 1.0f };
      in[comp] = from_bits(c.bits);
      n9++;
      if ((eu_ninepack_miss(in) != 0) != !c.finite) {       // a zero among the nine leaves a ray that is not null
        bad9++;
        printf("FAILED: ninepack, %s in component %d\n", c.name, comp);
      }
    }
  // the null centre ray, with any neighbours
  for (uint32_t z : { 0u, 0x80000000u }) {
    float in[9] = { from_bits(z), from_bits(z ^ 0x80000000u), from_bits(z), 0.26f, -0.5f, 1.0f, 0.25f, -0.49f, 1.0f };
    n9++;
    if (!eu_ninepack_miss(in)) { bad9++; printf("FAILED: ninepack with a null centre ray\n"); }
    float nb[9] = { 0.25f, -0.5f, 1.0f, from_bits(z), from_bits(z), from_bits(z), 0.25f, -0.49f, 1.0f };
    n9++;
    if (eu_ninepack_miss(nb)) { bad9++; printf("FAILED: a null NEIGHBOUR is an ordinary ninepack\n"); }
  }
  char what[96];
  snprintf(what, sizeof what, "eu_ray_miss over %d patterns", n3);
  check(bad3 == 0, what);
  snprintf(what, sizeof what, "eu_ninepack_miss over %d patterns", n9);
  check(bad9 == 0, what);
  check(eu_coord_finite(0.0f, -3.5f) && !eu_coord_finite(from_bits(0x7f800000u), 0.0f) &&
        !eu_coord_finite(1.0f, from_bits(0xffc00000u)), "eu_coord_finite");
}
}  // namespace

int main(int argc, char **argv)
{
  if (argc >= 3 && !strcmp(argv[1], "miss")) {
    const int n = atoi(argv[2]), count = argc - 3;
    if ((n != 3 && n != 9) || count % n) { fprintf(stderr, "miss 3|9 HEX...: groups of three or nine bit patterns\n"); return 2; }
    for (int g0 = 0; g0 < count; g0 += n) {
      float in[9];
      for (int k = 0; k < n; k++) in[k] = from_bits((uint32_t)strtoul(argv[3 + g0 + k], nullptr, 16));
      printf("%d\n", n == 3 ? eu_ray_miss(in[0], in[1], in[2]) : eu_ninepack_miss(in));
    }
    return 0;
  }
  test_paths();
  test_high_degrees();
  test_predicate();
  printf(failures ? "%d FAILED\n" : "all ok\n", failures);
  return failures ? 1 : 0;
}
