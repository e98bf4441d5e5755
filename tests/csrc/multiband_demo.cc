// --synopsis multiband / --bands N through include/eu_frontend.hpp and include/eu_dispatch.hpp, and the refusals of
// the C ABI (TEST CODE).
//   multiband_demo ARGS...    parses an envutil command line and prints synopsis, width and bands as JSON; image sizes
//                             come from EU_TEST_IMAGES="a.tif=200x150x3;b.tif=200x150x3" as for feather_demo. With
//                             EU_TEST_PAYLOAD set, payload() is called on synthetic pixels and its result printed ("rc N").
//   multiband_demo selftest   needs no device and asks for none (HIP_VISIBLE_DEVICES=-1): command lines and their
//                             refusals, the levels of a table of sizes, the scratch bytes, then what eu_hip_render,
//                             eu_hip_render_samples, eu_hip_render_rgbe, eu_hip_render_views_multi and
//                             eu_hip_blend_layers refuse of a multiband job before they look for a device. One line
//                             per check, "all ok" and exit status 0 when every one holds. The program to build with
//                             -fsanitize=address,undefined when a sanitizer run is wanted.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
  argv.insert(argv.begin(), "multiband_demo");
  return init_arguments(int(argv.size()), argv.data(), probe_table, err);
}

static bool has(const std::string &s, const char *word) { return s.find(word) != std::string::npos; }

static int selftest()
{
  setenv("HIP_VISIBLE_DEVICES", "-1", 1);
  image_info im; im.width = 48; im.height = 32; im.nchannels = 3;
  table["a.pfm"] = im; table["b.pfm"] = im;
  std::string err;
#define TWO "--facet", "a.pfm", "rectilinear", "50", "-14", "0", "0", "--facet", "b.pfm", "rectilinear", "50", "15", "0", "0", "--output", "o.pfm"
  check(parse({ TWO }, err) && args.synopsis == "panorama" && args.bands == 0, "default: panorama, bands 0");
  check(parse({ TWO, "--synopsis", "multiband" }, err) && args.synopsis == "multiband" && args.bands == 0 && args.feather == 0.0 && args.nfacets == 2,
        "--synopsis multiband, default bands and width");
  check(parse({ TWO, "--synopsis", "multiband", "--bands", "5" }, err) && args.bands == 5, "--bands 5");
  check(parse({ TWO, "--bands", "0", "--synopsis", "multiband" }, err) && args.bands == 0, "--bands 0 is the default, said aloud");
  check(parse({ TWO, "--synopsis", "multiband", "--feather", "6.5", "--bands", "2" }, err) && args.feather == 6.5 && args.bands == 2,
        "--feather goes with multiband too");
  check(!parse({ TWO, "--synopsis", "multiband", "--bands", "-1" }, err) && has(err, "--bands -1"), "negative bands are refused: " + err);
  check(!parse({ TWO, "--synopsis", "multiband", "--bands", "many" }, err) && has(err, "--bands"), "bands that are a word are refused: " + err);
  check(!parse({ TWO, "--bands", "4" }, err) && has(err, "--bands goes with --synopsis multiband"), "--bands without the synopsis is refused: " + err);
  check(!parse({ TWO, "--synopsis", "feather", "--bands", "4" }, err) && has(err, "--synopsis multiband"), "--bands with --synopsis feather is refused: " + err);
  check(!parse({ TWO, "--synopsis", "hdr_merge", "--feather", "4" }, err) && has(err, "--feather goes with --synopsis feather"),
        "--feather with hdr_merge keeps its wording: " + err);
  check(!parse({ TWO, "--synopsis", "multiband", "--bands" }, err), "--bands needs a value: " + err);
  // twining: none is applied by default to a multiband job of several facets, and none can be asked for
#define SPH "--projection", "spherical", "--hfov", "360", "--width", "96"
  check(parse({ TWO, SPH, "--synopsis", "multiband" }, err) && args.twine_setup() && args.twine == 0 && args.twine_spread.empty(),
        "multiband without --twine: no automatic twining, twine " + std::to_string(args.twine));
  check(parse({ TWO, SPH, "--synopsis", "feather" }, err) && args.twine_setup() && args.twine > 1 && !args.twine_spread.empty(),
        "feather without --twine: automatic twining as ever, twine " + std::to_string(args.twine));
  check(parse({ TWO, SPH, "--synopsis", "multiband", "--twine", "1" }, err) && args.twine_setup() && args.twine == 0, "multiband --twine 1 is no twining");
  check(!parse({ TWO, SPH, "--synopsis", "multiband", "--twine", "3" }, err) && has(err, "--synopsis multiband blends whole frames"),
        "multiband --twine 3 is refused: " + err);
  check(!parse({ TWO, SPH, "--synopsis", "multiband", "--twf_file", "taps.twf" }, err) && has(err, "no --twf_file"),
        "multiband --twf_file is refused: " + err);
  check(parse({ TWO, SPH, "--synopsis", "multiband", "--solo", "1" }, err) && args.twine_setup() && args.twine > 1,
        "multiband --solo 1 is a job of one facet: it twines, twine " + std::to_string(args.twine));
  // payload(): "multiband" passes the synopsis test (and then finds no device)
  {
    std::vector<float> px(48 * 32 * 3, 0.5f), out(size_t(96) * 48 * 3);
    const bool ok = parse({ TWO, "--synopsis", "multiband", "--bands", "2", "--projection", "spherical", "--hfov", "360", "--width", "96", "--twine", "0" }, err);
    for (auto &f : args.facet_spec_v) f.pixels = px.data();
    args.p_output = out.data();
    args.twine_setup();
    const int rc = ok ? get_dispatch()->payload(args.nchannels, 3, args.projection) : -99;
    check(rc == EU_ERR_NO_DEVICE || rc == EU_OK, "payload takes --synopsis multiband as far as the device: rc " + std::to_string(rc));
  }
  // levels
  struct lv { int w, h, bands, wrap, want; };
  for (const lv &c : { lv{ 4, 4, 0, 0, 0 }, lv{ 5, 3, 0, 0, 0 }, lv{ 9, 7, 0, 0, 1 }, lv{ 33, 17, 0, 0, 2 }, lv{ 130, 70, 0, 0, 4 },
                       lv{ 130, 70, 3, 0, 3 }, lv{ 64, 6, 3, 1, 0 }, lv{ 64, 16, 3, 1, 2 }, lv{ 36, 32, 0, 1, 2 }, lv{ 36, 32, 0, 0, 3 },
                       lv{ 16384, 8192, 0, 0, 8 }, lv{ 16384, 8192, 64, 0, 11 }, lv{ 1, 1, 0, 0, 0 } })
    check(eu_hip_multiband_levels(c.w, c.h, c.bands, c.wrap) == c.want,
          "levels of " + std::to_string(c.w) + " x " + std::to_string(c.h) + ", bands " + std::to_string(c.bands) + (c.wrap ? ", wrap" : "") + ": " +
          std::to_string(eu_hip_multiband_levels(c.w, c.h, c.bands, c.wrap)));
  check(eu_hip_multiband_levels(8, 8, -1, 0) == EU_ERR_ARGUMENT && eu_hip_multiband_levels(0, 8, 0, 0) == EU_ERR_ARGUMENT, "levels: bad arguments");
  // the C ABI
  eu_facet fc {};
  fc.projection = EU_RECTILINEAR; fc.nchannels = 3; fc.hfov = 0.9; fc.width = 48; fc.height = 32;
  fc.window_width = 48; fc.window_height = 32; fc.brighten = 1.0;
  fc.step = eu_hip_get_step(fc.projection, fc.width, fc.height, fc.hfov);
  eu_source *s[2] = { nullptr, nullptr }, *painted[2] = { nullptr, nullptr };
  check(eu_hip_diag_host_source(&fc, 1, &s[0]) == EU_OK && eu_hip_diag_host_source(&fc, 1, &s[1]) == EU_OK, "two host handles");
  fc.mask_paint = 1;
  check(eu_hip_diag_host_source(&fc, 1, &painted[1]) == EU_OK, "a painted host handle");
  painted[0] = s[0];
  eu_target t {};
  t.projection = EU_SPHERICAL; t.width = 20; t.height = 10; t.nchannels = 3; t.row_end = 10; t.synopsis = EU_SYN_MULTIBAND;
  double e[4];
  eu_hip_get_extent(t.projection, t.width, t.height, 2.0, e);
  t.x0 = e[0]; t.x1 = e[1]; t.y0 = e[2]; t.y1 = e[3];
  {
    // 20 x 10 -> 10 x 5: L = 1; ncol 3, two facets
    const size_t S0 = 200, T = 250, want = 4 * (S0 * (2 * 4 + 3) + 3 * (T - S0) + 2 * T + 4 * T);
    check(eu_hip_multiband_scratch_bytes(&t, 2) == want && eu_hip_multiband_scratch_bytes(&t, 1) == 0,
          "scratch bytes: " + std::to_string(eu_hip_multiband_scratch_bytes(&t, 2)) + ", formula " + std::to_string(want));
  }
  std::vector<float> out(size_t(20) * 10 * 4);
  const float taps[6] = { -0.25f, 0.0f, 0.5f, 0.25f, 0.0f, 0.5f };
  std::vector<float> steps(256, NAN);
  steps[1] = 0.5f;
  eu_encode enc {};
  enc.bits = 8; enc.colour_steps = steps.data();
  eu_view view {};
  view.x0 = t.x0; view.x1 = t.x1; view.y0 = t.y0; view.y1 = t.y1;
  const size_t row = 20 * 3 * sizeof(float);
  struct bad_case { const char *what; eu_target tt; eu_source **srcs; const char *word; };
  std::vector<bad_case> bad;
  { eu_target tt = t; tt.ntaps = 2; tt.taps = taps; bad.push_back({ "twining", tt, s, "multiband: no twining" }); }
  { eu_target tt = t; tt.row_begin = 2; bad.push_back({ "rows 2..10", tt, s, "multiband: the row range" }); }
  { eu_target tt = t; tt.row_end = 6; bad.push_back({ "rows 0..6", tt, s, "multiband: the row range" }); }
  { eu_target tt = t; tt.band_rows = 4; tt.band_count = 2; tt.row_end = 6; bad.push_back({ "row bands", tt, s, "multiband: no row bands" }); }
  { eu_target tt = t; tt.crop_w = 10; tt.crop_h = 10; bad.push_back({ "a crop window", tt, s, "multiband: no crop window" }); }
  { eu_target tt = t; tt.bands = -1; bad.push_back({ "bands -1", tt, s, "bands must be 0" }); }
  { eu_target tt = t; bad.push_back({ "--mask_for", tt, painted, "multiband: --mask_for" }); }
  for (const bad_case &b : bad) {
    int rcs[3]; std::string msg[3];
    rcs[0] = eu_hip_render(&b.tt, b.srcs, 2, out.data(), row, 0, nullptr); msg[0] = eu_hip_last_error();
    rcs[1] = eu_hip_render_samples(&b.tt, b.srcs, 2, &enc, out.data(), 20 * 3, 0, nullptr); msg[1] = eu_hip_last_error();
    rcs[2] = eu_hip_render_rgbe(&b.tt, b.srcs, 2, out.data(), 20 * 4, 0, nullptr); msg[2] = eu_hip_last_error();
    const char *entry[3] = { "eu_hip_render", "eu_hip_render_samples", "eu_hip_render_rgbe" };
    for (int k = 0; k < 3; k++)
      check(rcs[k] == EU_ERR_ARGUMENT && has(msg[k], b.word) && !has(msg[k], "no HIP device"),
            std::string(entry[k]) + ", " + b.what + ": " + std::to_string(rcs[k]) + " " + msg[k]);
  }
  {
    eu_target tt = t; tt.out_format = EU_OUT_SRGBA8;
    const int rc = eu_hip_render(&tt, s, 2, out.data(), 20 * 4, 0, nullptr);
    check(rc == EU_ERR_ARGUMENT && has(eu_hip_last_error(), "multiband: EU_OUT_SRGBA8"), std::string("eu_hip_render, EU_OUT_SRGBA8: ") + eu_hip_last_error());
    const int rv = eu_hip_render_views_multi(&t, &view, 1, s, 2, out.data(), row, 10 * row, 0, nullptr);
    check(rv == EU_ERR_ARGUMENT && has(eu_hip_last_error(), "render_views_multi: no multiband synopsis"), std::string("eu_hip_render_views_multi: ") + eu_hip_last_error());
    // one slot: eu_hip_render_devices is eu_hip_render, and a single facet ignores the synopsis
    const int rd = eu_hip_render_devices(&t, s, 2, out.data(), row, 0);
    check(rd == EU_ERR_NO_DEVICE || rd == EU_ERR_HANDLE, "eu_hip_render_devices with one slot goes as far as the device: " + std::to_string(rd));
    eu_target t1 = t; t1.row_end = 6;
    const int r1 = eu_hip_render(&t1, s, 1, out.data(), row, 0, nullptr);
    check(r1 == EU_ERR_NO_DEVICE || r1 == EU_ERR_HANDLE, "one facet ignores the synopsis: " + std::to_string(r1));
    const int ok = eu_hip_render(&t, s, 2, out.data(), row, 0, nullptr);
    check(ok == EU_ERR_NO_DEVICE || ok == EU_ERR_HANDLE, std::string("a whole multiband job goes as far as the device: ") + std::to_string(ok) + " " + eu_hip_last_error());
  }
  // eu_hip_blend_layers
  {
    std::vector<float> colour(2 * 7 * 9 * 3, 0.5f), weight(2 * 7 * 9, 1.0f), frame(7 * 9 * 3);
    const size_t cr = 9 * 3 * 4, wr = 9 * 4;
    auto call = [&](const float *c, const float *w, float *o, int n, int width, int height, int nch, int bands, size_t crow, size_t wrow, size_t orow) {
      return eu_hip_blend_layers(c, crow, crow * 7, w, wrow, wrow * 7, 0, n, width, height, nch, bands, 0, o, orow, 0, nullptr);
    };
    struct bl { const char *what; int rc; const char *word; };
    const bl cases[] = {
      { "null colour", call(nullptr, weight.data(), frame.data(), 2, 9, 7, 3, 0, cr, wr, cr), "null argument" },
      { "no layer", call(colour.data(), weight.data(), frame.data(), 0, 9, 7, 3, 0, cr, wr, cr), "at least one layer" },
      { "5 channels", call(colour.data(), weight.data(), frame.data(), 2, 9, 7, 5, 0, cr, wr, cr), "channels must be 1..4" },
      { "no width", call(colour.data(), weight.data(), frame.data(), 2, 0, 7, 3, 0, cr, wr, cr), "empty pictures" },
      { "bands -1", call(colour.data(), weight.data(), frame.data(), 2, 9, 7, 3, -1, cr, wr, cr), "blend_layers: bands" },
      { "a short row", call(colour.data(), weight.data(), frame.data(), 2, 9, 7, 3, 0, cr - 4, wr, cr), "row stride smaller than a row" },
      { "a short out row", call(colour.data(), weight.data(), frame.data(), 2, 9, 7, 3, 0, cr, wr, cr - 4), "row stride smaller than a row" },
      { "an odd stride", call(colour.data(), weight.data(), frame.data(), 2, 9, 7, 3, 0, cr + 2, wr, cr), "multiples of 4" },
    };
    for (const bl &c : cases) check(c.rc == EU_ERR_ARGUMENT, std::string("eu_hip_blend_layers, ") + c.what + ": " + std::to_string(c.rc));
    const int rc = eu_hip_blend_layers(colour.data(), cr, cr * 6, weight.data(), wr, wr * 7, 0, 2, 9, 7, 3, 0, 0, frame.data(), cr, 0, nullptr);
    check(rc == EU_ERR_ARGUMENT && has(eu_hip_last_error(), "layer stride smaller than a picture"), std::string("eu_hip_blend_layers, a short layer stride: ") + eu_hip_last_error());
    const int ok = call(colour.data(), weight.data(), frame.data(), 2, 9, 7, 3, 0, cr, wr, cr);
    check(ok == EU_ERR_NO_DEVICE || ok == EU_OK, "eu_hip_blend_layers goes as far as the device: " + std::to_string(ok));
  }
  check(eu_hip_multiband_scratch_release() == EU_OK, "scratch release without a device");
  eu_hip_source_release(s[0]);
  eu_hip_source_release(s[1]);
  eu_hip_source_release(painted[1]);
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
  std::printf("{\"ok\": true, \"synopsis\": \"%s\", \"feather\": %.17g, \"bands\": %d, \"twine\": %d, \"nfacets\": %d, \"projection\": %d, \"width\": %d, "
              "\"height\": %d}\n", args.synopsis.c_str(), args.feather, args.bands, args.twine, args.nfacets, int(args.projection), args.width, args.height);
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
