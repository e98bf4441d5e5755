// A PTO-style job with an exclude mask on one image and a lens crop on a fisheye image, through
// include/eu_dispatch.hpp: the facets carry their pixels as read (three channels) and payload() makes
// source_t's alpha edit while it loads them - on the device. With the argument "host" the pixels are
// prepared by prepare_facet_pixels (the library's HOST function) first, as a host that keeps its own
// set-up stage would; both runs must print the same checksum.
// Prints "rc <code>" and, on success, a checksum of the output.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "eu_dispatch.hpp"
#include "eu_imageprep.hpp"

static std::vector<float> synth(int w, int h, int nch, int seed)
{
  std::vector<float> img(size_t(w) * h * nch);
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++)
      for (int c = 0; c < nch; c++)
        img[(size_t(y) * w + x) * nch + c] = 0.25f + 0.5f * float((x * 7 + y * 13 + c * 29 + seed * 31) % 97) / 97.0f;
  return img;
}

int main(int argc, char **argv)
{
  using namespace project;
  const bool host = argc > 1 && !std::strcmp(argv[1], "host");
  std::vector<float> pa = synth(200, 150, 3, 1), pb = synth(160, 160, 3, 2);
  facet_spec a, b;
  a.projection = RECTILINEAR; a.width = 200; a.height = 150; a.hfov = 70.0 * M_PI / 180.0;
  a.yaw = 10.0 * M_PI / 180.0; a.pitch = 5.0 * M_PI / 180.0; a.roll = 2.0 * M_PI / 180.0;
  a.nchannels = 4; a.asset_key = "a"; a.facet_no = 0;
  a.has_pto_mask = true;
  pto_mask_type m;
  m.image = 0; m.variant = 0; m.vx = { 30, 120, 140, 40 }; m.vy = { 20, 25, 110, 100 };
  a.pto_mask_v.push_back(m);
  m.variant = 1;                                   // other variants are ignored, as in the reference
  m.vx = { 0, 200, 200, 0 }; m.vy = { 0, 0, 150, 150 };
  a.pto_mask_v.push_back(m);
  a.process_geometry();
  b.projection = FISHEYE; b.width = 160; b.height = 160; b.hfov = 170.0 * M_PI / 180.0;
  b.yaw = -100.0 * M_PI / 180.0; b.pitch = -20.0 * M_PI / 180.0;
  b.nchannels = 4; b.asset_key = "b"; b.facet_no = 1;
  b.has_lens_crop = true; b.crop_x0 = 10; b.crop_x1 = 150; b.crop_y0 = 10; b.crop_y1 = 150;
  b.process_geometry();
  std::string err;
  if (host) {
    if (!prepare_facet_pixels(a, pa, 3, err) || !prepare_facet_pixels(b, pb, 3, err)) {
      std::printf("rc -2\nerror: %s\n", err.c_str());
      return 1;
    }
  } else {
    a.pixel_channels = b.pixel_channels = 3;
  }
  a.pixels = pa.data(); b.pixels = pb.data();
  args.projection = SPHERICAL; args.width = 300; args.height = 150; args.hfov = 2.0 * M_PI;
  args.spline_degree = 3; args.twine = 0; args.nchannels = 4;
  args.facet_spec_v = { a, b };
  args.target_setup();
  args.twine_setup();
  std::vector<float> out(size_t(args.width) * args.height * 4);
  args.p_output = out.data();
  int rc = get_dispatch()->payload(4, 3, args.projection);
  std::printf("rc %d\n", rc);
  if (rc != 0) { std::printf("error: %s\n", eu_hip_last_error()); return rc == EU_ERR_NO_DEVICE ? 3 : 1; }
  uint64_t hsum = 1469598103934665603ull;
  size_t clear = 0, opaque = 0;
  for (size_t i = 0; i < out.size(); i++) {
    uint32_t u; std::memcpy(&u, &out[i], 4); hsum = (hsum ^ u) * 1099511628211ull;
    if (i % 4 == 3) { clear += out[i] == 0.0f; opaque += out[i] == 1.0f; }
  }
  std::printf("alpha clear %zu opaque %zu\n", clear, opaque);
  std::printf("fnv1a %016llx\n", (unsigned long long)hsum);
  return 0;
}
