// --synopsis feather / --feather WIDTH through include/eu_frontend.hpp and include/eu_dispatch.hpp, and the refusals
// of the C ABI (TEST CODE).
//   feather_demo ARGS...    parses an envutil command line and prints synopsis and width as JSON; image sizes come from
//                           EU_TEST_IMAGES="a.tif=200x150x3;b.tif=200x150x3" as for frontend_demo. With EU_TEST_PAYLOAD
//                           set, payload() is called on synthetic pixels and its result printed ("rc N").
//   feather_demo selftest   needs no device and asks for none (HIP_VISIBLE_DEVICES=-1): command lines and their
//                           refusals, then eu_hip_render, eu_hip_render_devices and eu_hip_render_views_multi with
//                           a synopsis outside the three and with negative and non-finite widths. One line per
//                           check, "all ok" and exit status 0 when every one holds. The program to build with
//                           -fsanitize=address,undefined when a sanitizer run is wanted.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <vector>
#include "eu_frontend.hpp"

extern "C" int eu_hip_diag_host_source(const eu_facet *fct, int spline_degree, eu_source **out);

using namespace project;

static std::map<std::string, image_info> table;
static bool probe_table(const std::string &name, image_info &info)
{
  auto it = table.find(name);
  if (it == table.end()) return false;
  info = it->second;
  return true;
}

static int failures = 0;
static void check(bool ok, const std::string &what)
{
  std::printf("%s: %s\n", ok ? "ok" : "FAILED", what.c_str());
  if (!ok) failures++;
}

static bool parse(std::vector<const char *> argv, std::string &err)
{
  argv.insert(argv.begin(), "feather_demo");
  return init_arguments(int(argv.size()), argv.data(), probe_table, err);
}

static int selftest()
{
  setenv("HIP_VISIBLE_DEVICES", "-1", 1);
  image_info im; im.width = 48; im.height = 32; im.nchannels = 3;
  table["a.pfm"] = im; table["b.pfm"] = im;
  std::string err;
#define TWO "--facet", "a.pfm", "rectilinear", "50", "-14", "0", "0", "--facet", "b.pfm", "rectilinear", "50", "15", "0", "0", "--output", "o.pfm"
  check(parse({ TWO }, err) && args.synopsis == "panorama" && args.feather == 0.0, "default: panorama, width 0");
  check(parse({ TWO, "--synopsis", "feather" }, err) && args.synopsis == "feather" && args.feather == 0.0 && args.nfacets == 2,
        "--synopsis feather, default width");
  check(parse({ TWO, "--synopsis", "feather", "--feather", "6.5" }, err) && args.feather == 6.5, "--feather 6.5");
  check(parse({ TWO, "--feather", "0", "--synopsis", "feather" }, err) && args.feather == 0.0, "--feather 0 is the default, said aloud");
  check(!parse({ TWO, "--synopsis", "feather", "--feather", "-1" }, err) && err.find("--feather -1") != std::string::npos,
        "a negative width is refused: " + err);
  check(!parse({ TWO, "--synopsis", "feather", "--feather", "nan" }, err) && err.find("--feather") != std::string::npos,
        "a width that is no number is refused: " + err);
  check(!parse({ TWO, "--synopsis", "feather", "--feather", "inf" }, err) && err.find("--feather") != std::string::npos,
        "an infinite width is refused: " + err);
  check(!parse({ TWO, "--synopsis", "feather", "--feather", "wide" }, err) && err.find("--feather") != std::string::npos,
        "a width that is a word is refused: " + err);
  check(!parse({ TWO, "--feather", "4" }, err) && err.find("--synopsis feather") != std::string::npos,
        "--feather without --synopsis feather is refused: " + err);
  check(!parse({ TWO, "--synopsis", "hdr_merge", "--feather", "4" }, err) && err.find("--synopsis feather") != std::string::npos,
        "--feather with --synopsis hdr_merge is refused: " + err);
  check(!parse({ TWO, "--synopsis", "feather", "--feather" }, err), "--feather needs a value: " + err);
  // payload(): "feather" passes the synopsis test (and then finds no device), another word does not
  {
    std::vector<float> px(48 * 32 * 3, 0.5f), out(size_t(96) * 48 * 3);
    const char *base[] = { "--projection", "spherical", "--hfov", "360", "--width", "96", "--twine", "0" };
    for (const char *syn : { "feather", "median" }) {
      std::vector<const char *> av = { TWO, "--synopsis", syn };
      av.insert(av.end(), base, base + 8);
      const bool ok = parse(av, err);
      for (auto &f : args.facet_spec_v) f.pixels = px.data();
      args.p_output = out.data();
      args.twine_setup();
      const int rc = ok ? get_dispatch()->payload(args.nchannels, 3, args.projection) : -99;
      if (std::string(syn) == "feather") check(rc == EU_ERR_NO_DEVICE || rc == EU_OK, "payload takes --synopsis feather as far as the device: rc " + std::to_string(rc));
      else check(rc == EU_ERR_ARGUMENT, "payload refuses --synopsis median: rc " + std::to_string(rc));
    }
  }
  // the C ABI
  eu_facet fc {};
  fc.projection = EU_RECTILINEAR; fc.nchannels = 3; fc.hfov = 0.9; fc.width = 48; fc.height = 32;
  fc.window_width = 48; fc.window_height = 32; fc.brighten = 1.0;
  fc.step = eu_hip_get_step(fc.projection, fc.width, fc.height, fc.hfov);
  eu_source *s[2] = { nullptr, nullptr };
  check(eu_hip_diag_host_source(&fc, 1, &s[0]) == EU_OK && eu_hip_diag_host_source(&fc, 1, &s[1]) == EU_OK, "two host handles");
  eu_target t {};
  t.projection = EU_SPHERICAL; t.width = 10; t.height = 4; t.nchannels = 3; t.row_end = 4;
  double e[4];
  eu_hip_get_extent(t.projection, t.width, t.height, 2.0, e);
  t.x0 = e[0]; t.x1 = e[1]; t.y0 = e[2]; t.y1 = e[3];
  std::vector<float> out(size_t(10) * 4 * 3);
  eu_view view {};
  view.x0 = t.x0; view.x1 = t.x1; view.y0 = t.y0; view.y1 = t.y1;
  const size_t row = 10 * 3 * sizeof(float);
  auto calls = [&](const eu_target &tt, int rcs[3], std::string msg[3]) {
    rcs[0] = eu_hip_render(&tt, s, 2, out.data(), row, 0, nullptr); msg[0] = eu_hip_last_error();
    rcs[1] = eu_hip_render_devices(&tt, s, 2, out.data(), row, 0); msg[1] = eu_hip_last_error();
    rcs[2] = eu_hip_render_views_multi(&tt, &view, 1, s, 2, out.data(), row, 4 * row, 0, nullptr); msg[2] = eu_hip_last_error();
  };
  const char *entry[3] = { "eu_hip_render", "eu_hip_render_devices", "eu_hip_render_views_multi" };
  struct bad_case { const char *what; int synopsis; double feather; const char *word; };
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const bad_case bad[] = { { "synopsis 3", 3, 0.0, "synopsis" }, { "synopsis -1", -1, 0.0, "synopsis" },
                           { "feather -1", EU_SYN_FEATHER, -1.0, "feather" }, { "feather -1e-300", EU_SYN_FEATHER, -1e-300, "feather" },
                           { "feather nan", EU_SYN_FEATHER, nan, "feather" }, { "feather inf", EU_SYN_FEATHER, inf, "feather" },
                           { "feather -inf", EU_SYN_FEATHER, -inf, "feather" },
                           { "a negative width under panorama", EU_SYN_PANORAMA, -2.0, "feather" } };
  for (const bad_case &b : bad) {
    eu_target tt = t;
    tt.synopsis = b.synopsis; tt.feather = b.feather;
    int rcs[3]; std::string msg[3];
    calls(tt, rcs, msg);
    for (int k = 0; k < 3; k++)
      check(rcs[k] == EU_ERR_ARGUMENT && msg[k].find(b.word) != std::string::npos && msg[k].find("no HIP device") == std::string::npos,
            std::string(entry[k]) + ", " + b.what + ": " + std::to_string(rcs[k]) + " " + msg[k]);
  }
  for (double w : { 0.0, 6.5, 1e6 }) {
    eu_target tt = t;
    tt.synopsis = EU_SYN_FEATHER; tt.feather = w;
    int rcs[3]; std::string msg[3];
    calls(tt, rcs, msg);
    for (int k = 0; k < 3; k++)
      // (a device that shows in spite of HIP_VISIBLE_DEVICES: the call gets as far as the handles, which have no container)
      check(rcs[k] == EU_ERR_NO_DEVICE || rcs[k] == EU_ERR_HANDLE, std::string(entry[k]) + ", feather " + std::to_string(w) + " goes as far as the device: " +
                                        std::to_string(rcs[k]) + " " + msg[k]);
  }
  eu_hip_source_release(s[0]);
  eu_hip_source_release(s[1]);
  std::printf(failures ? "%d FAILED\n" : "all ok\n", failures);
  return failures ? 1 : 0;
}

int main(int argc, char **argv)
{
  if (argc == 2 && std::string(argv[1]) == "selftest") return selftest();
  if (const char *e = std::getenv("EU_TEST_IMAGES")) {
    std::string s(e);
    size_t p = 0;
    while (p < s.size()) {
      size_t q = s.find(';', p);
      if (q == std::string::npos) q = s.size();
      const std::string item = s.substr(p, q - p);
      const size_t eq = item.find('=');
      image_info info;
      if (eq != std::string::npos &&
          std::sscanf(item.c_str() + eq + 1, "%dx%dx%d", &info.width, &info.height, &info.nchannels) == 3)
        table[item.substr(0, eq)] = info;
      p = q + 1;
    }
  }
  std::string err;
  if (!init_arguments(argc, argv, probe_table, err)) {
    std::printf("{\"ok\": false, \"error\": \"%s\"}\n", err.c_str());
    return 2;
  }
  args.twine_setup();
  std::printf("{\"ok\": true, \"synopsis\": \"%s\", \"feather\": %.17g, \"nfacets\": %d, \"projection\": %d, \"width\": %d, "
              "\"height\": %d}\n", args.synopsis.c_str(), args.feather, args.nfacets, int(args.projection), args.width, args.height);
  if (std::getenv("EU_TEST_PAYLOAD")) {
    std::vector<std::vector<float>> px(args.facet_spec_v.size());
    for (size_t k = 0; k < args.facet_spec_v.size(); k++) {
      facet_spec &f = args.facet_spec_v[k];
      px[k].assign(size_t(f.window_width) * f.window_height * f.nchannels, 0.25f + 0.125f * float(k));
      f.pixels = px[k].data();
    }
    std::vector<float> out(size_t(args.width) * args.height * args.nchannels);
    args.p_output = out.data();
    const int rc = get_dispatch()->payload(args.nchannels, args.twine ? 9 : 3, args.projection);
    std::printf("rc %d\n", rc);
  }
  return 0;
}
