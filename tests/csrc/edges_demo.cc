// Host program for --feather_edges in include/eu_frontend.hpp (TEST CODE): the option's parse, what it is refused with,
// and which facets it reaches as facet_spec::edges. No device is needed: init_arguments runs on the host.
//   edges_demo parse ARGS...   -> "ok feather_edges E | NAME nchannels N edges B key KEY | ..." | "refused: ..."
//        image sizes from the environment, as frontend_demo: EU_TEST_IMAGES="a.pam=40x30x4;b.ppm=40x30x3"
//   edges_demo selftest        -> a fixed set of command lines and PTO scripts, parsed in this process one after the
//        other; the program to build with -fsanitize=address,undefined
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>
#include "eu_frontend.hpp"

using namespace project;

static std::map<std::string, image_info> table;

static bool probe_table(const std::string &name, image_info &info)
{
  auto it = table.find(name);
  if (it == table.end()) return false;
  info = it->second;
  return true;
}

static bool parse(const std::vector<std::string> &argv, std::string &err)
{
  std::vector<const char *> v { "edges_demo" };
  for (const auto &s : argv) v.push_back(s.c_str());
  image_probe probe = probe_table;
  return init_arguments(int(v.size()), v.data(), probe, err);
}

static void add_image(const std::string &name, int w, int h, int c)
{
  image_info info;
  info.width = w; info.height = h; info.nchannels = c;
  table[name] = info;
}

static int selftest()
{
  int failed = 0, cases = 0;
  auto expect = [&](bool ok, const std::string &what) { cases++; if (!ok) { failed++; std::printf("FAILED %s\n", what.c_str()); } };
  add_image("rgba.pam", 40, 30, 4);
  add_image("rgb.ppm", 40, 30, 3);
  add_image("grey.pgm", 40, 30, 1);
  add_image("ga.pam", 40, 30, 2);
  add_image("cube.pam", 16, 96, 4);
  std::string err;
  const std::vector<std::string> two = { "--facet", "rgba.pam", "rectilinear", "50", "-10", "0", "0", "--facet", "rgb.ppm", "rectilinear", "50", "12", "0", "0",
                                         "--projection", "spherical", "--hfov", "120", "--width", "96", "--height", "48", "--output", "o.pfm" };
  auto with = [&](std::vector<std::string> more) { std::vector<std::string> v = two; v.insert(v.end(), more.begin(), more.end()); return v; };
  expect(parse(with({ "--synopsis", "feather", "--feather_edges" }), err) && args.feather_edges && args.facet_spec_v.size() == 2 &&
         args.facet_spec_v[0].edges && !args.facet_spec_v[1].edges, "feather: the facet with alpha alone: " + err);
  expect(args.facet_spec_v[0].asset_key != "rgba.pam" && args.facet_spec_v[1].asset_key == "rgb.ppm", "the asset key says so");
  expect(parse(with({ "--synopsis", "multiband", "--feather_edges", "--bands", "2" }), err) && args.facet_spec_v[0].edges, "multiband: " + err);
  expect(parse(with({ "--synopsis", "feather" }), err) && !args.feather_edges && !args.facet_spec_v[0].edges &&
         args.facet_spec_v[0].asset_key == "rgba.pam", "without the option: " + err);
  for (const char *syn : { "panorama", "hdr_merge" })
    expect(!parse(with({ "--synopsis", syn, "--feather_edges" }), err) && err.find("--feather_edges goes with") != std::string::npos,
           std::string("refused under ") + syn + ": " + err);
  expect(!parse(with({ "--feather_edges" }), err) && err.find("--feather_edges goes with") != std::string::npos, "refused without a synopsis: " + err);
  expect(!parse(with({ "--synopsis", "feather", "--feather_edges", "1" }), err), "the option takes no value");
  // grey + alpha, plain grey, a cubemap with alpha
  expect(parse({ "--facet", "ga.pam", "rectilinear", "50", "-10", "0", "0", "--facet", "grey.pgm", "rectilinear", "50", "12", "0", "0",
                 "--facet", "cube.pam", "cubemap", "90", "0", "0", "0", "--projection", "spherical", "--hfov", "360", "--width", "96",
                 "--height", "48", "--output", "o.pfm", "--synopsis", "feather", "--feather_edges" }, err) &&
         args.facet_spec_v[0].edges && !args.facet_spec_v[1].edges && !args.facet_spec_v[2].edges, "2 channels, 1 channel, a cubemap: " + err);
  std::printf("%d checks, %d failed\n", cases, failed);
  if (!failed) std::printf("all ok\n");
  return failed ? 1 : 0;
}

int main(int argc, char **argv)
{
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "selftest" && argc == 2) return selftest();
  if (mode == "parse") {
    if (const char *e = std::getenv("EU_TEST_IMAGES")) {
      std::string s(e);
      size_t p = 0;
      while (p < s.size()) {
        size_t q = s.find(';', p);
        if (q == std::string::npos) q = s.size();
        const std::string item = s.substr(p, q - p);
        const size_t eq = item.find('=');
        int w = 0, h = 0, c = 0;
        if (eq != std::string::npos && std::sscanf(item.c_str() + eq + 1, "%dx%dx%d", &w, &h, &c) == 3) add_image(item.substr(0, eq), w, h, c);
        p = q + 1;
      }
    }
    std::string err;
    if (!parse(std::vector<std::string>(argv + 2, argv + argc), err)) { std::printf("refused: %s\n", err.c_str()); return 0; }
    std::printf("ok feather_edges %d", int(args.feather_edges));
    for (const auto &f : args.facet_spec_v)
      std::printf(" | %s nchannels %d edges %d key %s", f.filename.c_str(), f.nchannels, int(f.edges), f.asset_key.c_str());
    std::printf("\n");
    return 0;
  }
  std::fprintf(stderr, "usage: edges_demo parse ARGS... | selftest\n");
  return 2;
}
