// envutil_hip - envutil's command line on the MI355X path.
//
//   envutil_hip --facet pano.pfm spherical 360 0 0 0 --projection cubemap --hfov 90
//               --width 1024 --degree 3 --output cube.pfm
//   envutil_hip --pto project.pto --output pano.pfm
//   envutil_hip --facet pano.pfm spherical 360 0 0 0 --degree 3 --ray_map rays.pfm --output looked_up.pfm
//   envutil_hip --facet left.pfm spherical 360 0 0 0 --projection cubemap --width 1024 --degree 3
//               --output left_cube.pfm --layer right.pfm right_cube.pfm        (two pictures, one geometry, one call)
//   envutil_hip <fixed options> -          (pipe mode: one job per line of stdin)
//
// The same options, defaults and PTO handling as the reference's main() / core()
// (envutil_main.cc:1634-1727, :1948-1982): include/eu_frontend.hpp fills project::args,
// get_dispatch()->payload() renders (include/eu_dispatch.hpp -> libeu_hip.so), and the images
// go through include/eu_image_io.hpp (PFM / PNM / PAM / Radiance instead of OpenImageIO; the sRGB / Rec709 /
// linear transfer pairs of OpenImageIO's built-in colour configuration, --input / --working / --output_colour_space
// and the PTO's Csp clause honoured, any other colour space an error message). Sources stay resident in HBM between the jobs of a pipe-mode session, as the
// reference's asset_handler keeps them in RAM. There is no CPU rendering path: without an
// MI355X every job fails with the library's error.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "eu_frontend.hpp"
#include "eu_image_io.hpp"
#include "eu_imageprep.hpp"

using namespace project;

// tokenize (envutil_basic.cc:323-420): blanks separate, single or double quotes group, a
// backslash inside quotes carries the quote sign
static std::vector<std::string> tokenize(const std::string &s)
{
  std::vector<std::string> out;
  std::string tok;
  char quote = 0;
  bool in_tok = false;
  for (size_t i = 0; i < s.size(); i++) {
    const char c = s[i];
    if (quote) {
      if (c == '\\' && i + 1 < s.size() && s[i + 1] == quote) { tok += quote; i++; }
      else if (c == quote) { out.push_back(tok); tok.clear(); quote = 0; in_tok = false; }
      else tok += c;
    } else if (c == ' ' || c == '\t' || c == '\n' || c == '\r') {
      if (in_tok) { out.push_back(tok); tok.clear(); in_tok = false; }
    } else if (!in_tok && (c == '"' || c == '\'')) { quote = c; in_tok = true; }
    else { tok += c; in_tok = true; }
  }
  if (in_tok) out.push_back(tok);
  return out;
}

// image_series (envutil_basic.h:207-262): a format string with one %-sequence taking an integer
// The reference formats whenever the string holds exactly one '%' and returns it verbatim otherwise; a
// conversion other than an integer one ("%s", "%n") is undefined behaviour there. Here the one '%' has to
// introduce "%[flags][width]d" (or i / u / x / X / o) - anything else is returned verbatim, never handed to printf
// (the string arrives from the command line and, in pipe mode, from stdin).
static std::string series_name(const std::string &fmt, int index)
{
  size_t npct = 0, pos = 0;
  for (size_t i = 0; i < fmt.size(); i++) if (fmt[i] == '%') { npct++; pos = i; }
  if (npct != 1) return fmt;
  size_t k = pos + 1;
  while (k < fmt.size() && (fmt[k] == '0' || fmt[k] == '-' || fmt[k] == '+' || fmt[k] == ' ')) k++;
  while (k < fmt.size() && fmt[k] >= '0' && fmt[k] <= '9') k++;
  if (k >= fmt.size() || !std::strchr("diuxXo", fmt[k]) || k - pos > 8) return fmt;
  std::vector<char> buf(fmt.size() + 32);
  std::snprintf(buf.data(), buf.size(), fmt.c_str(), index);
  return buf.data();
}

// A .y4m --output: one stream for all frames of a run, opened by the first frame that is written (its size is the
// frame's), closed by core()
static std::unique_ptr<io::y4m_writer> y4m_sink;

// One frame as the planes of the stream's format: rendered and encoded on the device (eu_hip_render_ycbcr), the bytes
// of the file come down as they are. No colour conversion: the floats are encoded as they are, as a .y4m facet is
// loaded as it is.
static int run_payload_y4m(const std::string &output, int ow, int oh)
{
  std::string err;
  const bool full = args.ycbcr_range == "full";
  const std::string matrix = !args.ycbcr_matrix.empty() ? args.ycbcr_matrix : oh >= 720 ? "709" : "601";
  if (!y4m_sink) {
    y4m_sink.reset(new io::y4m_writer);
    if (!y4m_sink->open(output, ow, oh, args.y4m_format, args.y4m_depth, full, args.fps_num, args.fps_den, err)) {
      std::fprintf(stderr, "envutil_hip: %s\n", err.c_str());
      return 1;
    }
  }
  io::y4m_writer &sink = *y4m_sink;
  const io::y4m_info &yi = sink.info;
  if (yi.width != ow || yi.height != oh) {
    std::fprintf(stderr, "envutil_hip: %s holds frames of %d x %d, this one has %d x %d\n", output.c_str(), yi.width, yi.height, ow, oh);
    return 1;
  }
  // (the tables of a depth and a range are kept: the frames of a sequence share them)
  static std::map<std::string, std::pair<std::vector<float>, std::vector<float>>> kept;
  const std::string key = std::to_string(yi.depth) + (full ? "f" : "l");
  auto it = kept.find(key);
  if (it == kept.end()) {
    std::pair<std::vector<float>, std::vector<float>> t;
    io::ycbcr_steps(yi.bits, yi.depth, full, t.first, t.second);
    it = kept.emplace(key, std::move(t)).first;
  }
  float k[5];
  if (!io::ycbcr_forward(matrix, k, err)) { std::fprintf(stderr, "envutil_hip: %s\n", err.c_str()); return 1; }
  std::vector<uint8_t> planes(yi.frame_bytes());
  const size_t sb = size_t(yi.bits / 8), cw = (size_t(ow) + yi.sub_x - 1) / yi.sub_x;
  eu_ycbcr_out o {};
  o.y = planes.data(); o.cb = planes.data() + yi.y_bytes; o.cr = planes.data() + yi.y_bytes + yi.c_bytes;
  o.y_pitch = size_t(ow) * sb; o.c_pitch = cw * sb;
  o.c_step = 1; o.sub_x = yi.sub_x; o.sub_y = yi.sub_y; o.bits = yi.bits; o.shift = 0; o.on_device = 0;
  o.y_steps = it->second.first.data(); o.c_steps = it->second.second.data();
  o.k_r = k[0]; o.k_g = k[1]; o.k_b = k[2]; o.c_u = k[3]; o.c_v = k[4];
  args.p_output_ycbcr = &o;
  const int rc = get_dispatch()->payload(args.nchannels, args.twine ? 9 : 3, args.projection);
  args.p_output_ycbcr = nullptr;
  if (rc != 0) {
    std::fprintf(stderr, "envutil_hip: render failed (%d): %s\n", rc, eu_hip_last_error());
    return 1;
  }
  if (!sink.frame(planes.data(), err)) {
    std::fprintf(stderr, "envutil_hip: %s\n", err.c_str());
    return 1;
  }
  if (args.verbose)
    std::printf("saved frame %d of %s (%d x %d, C%s, BT.%s %s range): Y'CbCr planes, encoded on the device\n", sink.frames - 1,
                output.c_str(), ow, oh, sink.tag.c_str(), matrix.c_str(), full ? "full" : "limited");
  return 0;
}

static int run_payload(const std::string &output)
{
  int ow = args.width, oh = args.height;
  if (args.store_cropped) { ow = args.p_crop_x1 - args.p_crop_x0; oh = args.p_crop_y1 - args.p_crop_y0; }
  const bool ray_map = args.p_ray_map != nullptr;            // --ray_map: the output has the map's size
  if (ray_map) { ow = args.ray_map_width; oh = args.ray_map_height; }
  std::string err;
  if (io::lower_ext(output) == "y4m") return run_payload_y4m(output, ow, oh);    // (core() has refused what does not go with it)
  const bool cube = (args.projection == CUBEMAP || args.projection == BIATAN6) && !args.store_cropped && !ray_map;
  // save_array attaches the target's projection and hfov (degrees) to the file (envutil_basic.h:770-772)
  io::metadata meta;
  meta.projection = projection_name[args.projection];
  meta.hfov = (180.0 / M_PI) * args.hfov;

  // A PNM / PAM output leaves the device as the file's samples (eu_hip_render_samples): the step tables say, for
  // the way from the working colour space to the output's and the file's maxval, which sample a float becomes by
  // convert_colour + write_one below - the same bytes, without the float download and the host's pass over them.
  // A table the builder refuses (a curve whose code drops at a joint), --ray_map and several devices keep that route.
  const size_t nlayers = args.layer_spec_v.size();          // --layer: every picture leaves by the float route
  int bits = 0, maxval = 0;
  if (!nlayers && io::sample_format(output, bits, maxval) && !ray_map && !args.tethered && hip_dispatch::device_slots() == 1) {
    // (the tables of a pair of colour spaces are kept: the jobs of a pipe-mode session share them)
    struct step_tables { bool ok; std::string why; std::vector<float> colour, alpha; };
    static std::map<std::string, step_tables> kept;
    const std::string key = std::to_string(bits) + "/" + args.working_colour_space + "/" + args.colour_space;
    auto it = kept.find(key);
    if (it == kept.end()) {
      step_tables t;
      t.ok = io::encode_steps(bits, maxval, args.working_colour_space, args.colour_space, t.colour, t.alpha, t.why);
      it = kept.emplace(key, std::move(t)).first;
    }
    const std::vector<float> &colour_steps = it->second.colour, &alpha_steps = it->second.alpha;
    const std::string &why = it->second.why;
    if (it->second.ok) {
      std::vector<uint8_t> samples(size_t(ow) * oh * args.nchannels * size_t(bits / 8));
      args.output_encode.bits = bits;
      args.output_encode.big_endian = 1;                     // as PNM / PAM store 16-bit samples
      args.output_encode.colour_steps = colour_steps.data();
      args.output_encode.alpha_steps = alpha_steps.data();
      args.p_output_samples = samples.data();
      const int rc = get_dispatch()->payload(args.nchannels, args.twine ? 9 : 3, args.projection);
      args.p_output_samples = nullptr;
      args.output_encode = eu_encode {};
      if (rc != 0) {
        std::fprintf(stderr, "envutil_hip: render failed (%d): %s\n", rc, eu_hip_last_error());
        return 1;
      }
      if (!io::write_samples(output, samples.data(), ow, oh, args.nchannels, cube, err, &meta)) {
        std::fprintf(stderr, "envutil_hip: %s\n", err.c_str());
        return 1;
      }
      if (args.verbose)
        std::printf("saved %s (%d x %d x %d): %d-bit samples, encoded on the device\n", output.c_str(), ow, oh, args.nchannels, bits);
      return 0;
    }
    if (args.verbose) std::printf("%s: float pixels, encoded on the host (%s)\n", output.c_str(), why.c_str());
  }

  // A Radiance output leaves the device as the file's quads (eu_hip_render_rgbe): eu_rgbe_encode is the function
  // write_one calls below - the same bytes, without the float download and the host's pass over them. A colour
  // conversion on the way out, a target of another channel count (write_one's error message), --ray_map and several
  // devices keep the float route.
  const std::string oext = io::lower_ext(output);
  if ((oext == "hdr" || oext == "pic") && !args.tethered && !nlayers) {
    io::colour_class ca, cb;
    bool same = false;
    std::string cerr;
    const char *why = nullptr;
    if (ray_map) why = "a ray map's output";
    else if (hip_dispatch::device_slots() != 1) why = "several devices";
    else if (args.nchannels != 3) why = "not 3 channels";
    else if (!io::colour_pair(args.working_colour_space, args.colour_space, ca, cb, same, cerr) || !same) why = "the output's colour space is not the working one";
    if (!why) {
      std::vector<uint8_t> quads(size_t(ow) * oh * 4);
      args.p_output_rgbe = quads.data();
      const int rc = get_dispatch()->payload(args.nchannels, args.twine ? 9 : 3, args.projection);
      args.p_output_rgbe = nullptr;
      if (rc != 0) {
        std::fprintf(stderr, "envutil_hip: render failed (%d): %s\n", rc, eu_hip_last_error());
        return 1;
      }
      if (!io::write_rgbe(output, quads.data(), ow, oh, cube, err, &meta)) {
        std::fprintf(stderr, "envutil_hip: %s\n", err.c_str());
        return 1;
      }
      if (args.verbose)
        std::printf("saved %s (%d x %d x %d): RGBE pixels, encoded on the device\n", output.c_str(), ow, oh, args.nchannels);
      return 0;
    }
    if (args.verbose) std::printf("%s: float pixels, encoded on the host (%s)\n", output.c_str(), why);
  }

  // the facet's frame, and behind it one frame per --layer: one eu_hip_render_layers call renders them all
  const size_t frame = size_t(ow) * oh * args.nchannels;
  std::vector<float> out(frame * (1 + nlayers));
  args.p_output = out.data();
  const int rc = get_dispatch()->payload(args.nchannels, args.twine ? 9 : 3, args.projection);
  args.p_output = nullptr;
  if (rc != 0) {
    std::fprintf(stderr, "envutil_hip: render failed (%d): %s\n", rc, eu_hip_last_error());
    return 1;
  }
  if (nlayers && args.verbose)
    std::printf("rendered %zu pictures of one geometry in one eu_hip_render_layers call\n", 1 + nlayers);
  for (size_t k = 0; k <= nlayers; k++) {
    const std::string &name = k ? args.layer_output_v[k - 1] : output;
    float *px = out.data() + k * frame;
    // save_array: from the working colour space to the output's where they differ (envutil_basic.h:786-812)
    if (!io::convert_colour(px, size_t(ow) * oh, args.nchannels, args.working_colour_space, args.colour_space, err)) {
      std::fprintf(stderr, "envutil_hip: %s\n", err.c_str());
      return 1;
    }
    // (a ray map's output has no projection of its own to record)
    if (!io::write_image(name, px, ow, oh, args.nchannels, cube, err, ray_map ? nullptr : &meta)) {
      std::fprintf(stderr, "envutil_hip: %s\n", err.c_str());
      return 1;
    }
    if (args.verbose) std::printf("saved %s (%d x %d x %d)\n", name.c_str(), ow, oh, args.nchannels);
  }
  return 0;
}

// core(), envutil_main.cc:1634-1727
static int core(int argc, const char *const *argv, bool pipe_mode = false)
{
  std::string err;
  // with --frames a numbered name stands for its first frame (init_arguments checks name and numbers before it probes)
  int probe_frame = -1;
  for (int i = 1; i + 1 < argc; i++)
    if (std::string(argv[i]) == "--frames" && !io::frame_number(argv[i + 1], probe_frame)) probe_frame = -1;
  image_probe probe = [&](const std::string &given, image_info &info) {
    std::string e, name = given;
    io::metadata m;
    if (probe_frame >= 0 && io::lower_ext(given) != "y4m" && !io::frame_name(given, probe_frame, name, e)) return false;
    if (!io::probe(name, info.width, info.height, info.nchannels, e, &m)) return false;
    info.projection = m.projection; info.hfov = m.hfov;
    return true;
  };
  if (!init_arguments(argc, argv, probe, err)) {
    std::fprintf(stderr, "envutil_hip: %s\n", err.c_str());
    return 2;
  }
  if (!args.layer_spec_v.empty()) {
    if (pipe_mode) {
      std::fprintf(stderr, "envutil_hip: --layer does not go with pipe mode: one call renders the layers, then the program ends\n");
      return 2;
    }
    if (args.store_cropped) {
      std::fprintf(stderr, "envutil_hip: --layer renders whole frames: the p-line's crop (S clause) does not go with it\n");
      return 2;
    }
    if (hip_dispatch::device_slots() > 1) {
      std::fprintf(stderr, "envutil_hip: --layer renders on one device: set EU_HIP_DEVICES=1 on a host with several\n");
      return 2;
    }
  }
  // A .y4m --output is written through eu_hip_render_ycbcr. What that route does not do is refused here, each with
  // its own message.
  const bool y4m_out = io::lower_ext(args.output) == "y4m";
  y4m_sink.reset();
  for (const std::string &name : args.layer_output_v)
    if (io::lower_ext(name) == "y4m") {
      std::fprintf(stderr, "envutil_hip: --layer %s: the pictures of --layer leave by the float route, a .y4m stream is the --output's alone\n", name.c_str());
      return 2;
    }
  if (io::lower_ext(args.split) == "y4m" || (y4m_out && !args.split.empty())) {
    std::fprintf(stderr, "envutil_hip: --split does not go with a .y4m output: its jobs differ in size, a stream holds frames of one size\n");
    return 2;
  }
  if (y4m_out) {
    if (pipe_mode) {
      std::fprintf(stderr, "envutil_hip: a .y4m output does not go with pipe mode: one call writes the stream, then the program ends\n");
      return 2;
    }
    if (!args.ray_map.empty()) {
      std::fprintf(stderr, "envutil_hip: a .y4m output does not go with --ray_map: a ray map's output is a float image\n");
      return 2;
    }
    if (args.nchannels != 3) {
      std::fprintf(stderr, "envutil_hip: a .y4m output holds 3 channels, the target has %d (--nchannels 3)\n", args.nchannels);
      return 2;
    }
    if (hip_dispatch::device_slots() > 1) {
      std::fprintf(stderr, "envutil_hip: a .y4m output is encoded on one device: set EU_HIP_DEVICES=1 on a host with several\n");
      return 2;
    }
  }
  struct close_sink {
    ~close_sink()
    {
      std::string e;
      if (y4m_sink && !y4m_sink->close(e)) std::fprintf(stderr, "envutil_hip: %s\n", e.c_str());
      if (y4m_sink && !y4m_sink->frames && !y4m_sink->name.empty()) std::remove(y4m_sink->name.c_str());   // no frame: no stream
      y4m_sink.reset();
    }
  } close_sink_on_exit;
  const bool sequence = args.frames_first >= 0;
  if (sequence) {
    if (pipe_mode) {
      std::fprintf(stderr, "envutil_hip: --frames does not go with pipe mode: one call renders the sequence, then the program ends\n");
      return 2;
    }
    if (hip_dispatch::device_slots() > 1) {
      std::fprintf(stderr, "envutil_hip: --frames renders on one device: set EU_HIP_DEVICES=1 on a host with several\n");
      return 2;
    }
  }
  const auto *dp = static_cast<const hip_dispatch *>(get_dispatch());
  if (args.verbose) std::printf("using %s (%s)\n", dp->hwy_target_name.c_str(), dp->hwy_target_str.c_str());
  if (args.verbose && args.facet_spec_v.size() > 1) {
    // how the facets are composed; feather: the ramp's width in source pixels
    if (args.synopsis == "multiband") {
      // the levels the frame gets: columns wrap on a spherical or cylindrical target of 360 degrees
      const bool wrap = (args.projection == SPHERICAL || args.projection == CYLINDRICAL) && std::fabs(args.hfov - 2.0 * M_PI) < .000001;
      std::printf("synopsis multiband, %d levels above level 0%s", eu_hip_multiband_levels(args.width, args.height, args.bands, wrap),
                  wrap ? ", columns wrap" : "");
      if (args.feather > 0.0) std::printf(", width %g source pixels\n", args.feather);
      else std::printf(", width: half of each facet's shorter side\n");
    }
    else if (args.synopsis != "feather") std::printf("synopsis %s\n", args.synopsis.c_str());
    else if (args.feather > 0.0) std::printf("synopsis feather, width %g source pixels\n", args.feather);
    else std::printf("synopsis feather, width: half of each facet's shorter side\n");
  }
  if (!args.twine_setup()) {
    std::fprintf(stderr, "envutil_hip: cannot read the tap table %s\n", args.twf_file.c_str());
    return 2;
  }

  // pixels of the facets that are not resident yet (asset_handler, environment.h:84-227): floats, or - PNM / PAM
  // files - the file's integer samples with the tables that say which float each value becomes, or - Radiance
  // pictures - the file's quads, with such a table where the file's colour space is not the working one
  // (the pictures of --layer come behind the facets: each by the route its own file type takes)
  const size_t nfct = args.facet_spec_v.size(), nimg = nfct + args.layer_spec_v.size();
  std::vector<std::vector<float>> pixels(nimg), colour_tab(nimg), alpha_tab(nimg);
  std::vector<std::vector<uint8_t>> samples(nimg);
  // ... or - a .y4m stream - the planes of one of its frames, with the tables and the matrix of the Y'CbCr feed
  std::vector<std::unique_ptr<io::y4m_reader>> streams(nimg);
  std::vector<eu_ycbcr> ycc(nimg);
  enum { KIND_FLOATS, KIND_SAMPLES_8, KIND_SAMPLES_16, KIND_RGBE, KIND_YCBCR };
  static const char *const kind_name[] = { "float pixels", "8-bit samples, decoded on the device", "16-bit samples, decoded on the device",
                                           "RGBE pixels, decoded on the device", "YCbCr planes, decoded on the device" };
  // image k's pixels out of `file` (a .y4m stream: its frame `frame`) into the buffers above and into f's feed
  auto read_pixels = [&](size_t k, facet_spec &f, const std::string &file, int frame, int &kind, int &nch) -> bool {
    f.pixels = nullptr; f.samples = nullptr; f.rgbe = nullptr; f.rgbe_table = nullptr; f.ycbcr = nullptr;
    int w = 0, h = 0, maxval = 0, sbits = 0;
    nch = 0;
    std::string serr;
    const bool as_ycbcr = io::lower_ext(file) == "y4m";
    if (as_ycbcr) {
      if (!streams[k]) {
        streams[k].reset(new io::y4m_reader);
        if (!streams[k]->open(file, err)) { std::fprintf(stderr, "envutil_hip: %s\n", err.c_str()); return false; }
      }
      io::y4m_reader &r = *streams[k];
      if (!r.frame(frame, samples[k], err)) { std::fprintf(stderr, "envutil_hip: %s\n", err.c_str()); return false; }
      const io::y4m_info &yi = r.info;
      w = yi.width; h = yi.height; nch = 3;
      if (yi.bits == 16) {                          // the file's words are little-endian, the feed takes host order
        const uint16_t one = 1;
        if (!*reinterpret_cast<const uint8_t *>(&one))
          for (size_t i = 0; i + 1 < samples[k].size(); i += 2) std::swap(samples[k][i], samples[k][i + 1]);
      }
      eu_ycbcr &y = ycc[k];
      if (colour_tab[k].empty()) {
        const bool full = args.ycbcr_range.empty() ? yi.full_range : args.ycbcr_range == "full";
        const std::string matrix = !args.ycbcr_matrix.empty() ? args.ycbcr_matrix : h >= 720 ? "709" : "601";
        io::ycbcr_tables(yi.bits, yi.depth, full, colour_tab[k], alpha_tab[k]);
        float m[4];
        if (!io::ycbcr_matrix(matrix, m, err)) { std::fprintf(stderr, "envutil_hip: %s\n", err.c_str()); return false; }
        y = eu_ycbcr {};
        y.m_rv = m[0]; y.m_gu = m[1]; y.m_gv = m[2]; y.m_bu = m[3];
        if (args.verbose)
          std::printf("%s: %d x %d, %d-bit 4:%s, matrix %s, %s range\n", file.c_str(), w, h, yi.depth,
                      yi.sub_x == 1 ? "4:4" : yi.sub_y == 1 ? "2:2" : "2:0", matrix.c_str(), full ? "full" : "limited");
      }
      const size_t sb = size_t(yi.bits / 8), cw = (size_t(w) + yi.sub_x - 1) / yi.sub_x;
      y.y = samples[k].data(); y.cb = samples[k].data() + yi.y_bytes; y.cr = samples[k].data() + yi.y_bytes + yi.c_bytes;
      y.y_pitch = size_t(w) * sb; y.c_pitch = cw * sb;
      y.c_step = 1; y.sub_x = yi.sub_x; y.sub_y = yi.sub_y; y.bits = yi.bits; y.on_device = 0;
      y.y_table = colour_tab[k].data(); y.c_table = alpha_tab[k].data();
    }
    // an integer file goes up as it is and is widened and linearised on the device; whatever read_samples refuses
    // is left to the float route and to its messages
    const bool as_samples = !as_ycbcr && io::read_samples(file, samples[k], w, h, nch, maxval, sbits, serr);
    // ... and so does a Radiance picture, as its quads (they share the byte buffer: a file is one or the other)
    const bool as_rgbe = !as_ycbcr && !as_samples && io::read_rgbe(file, samples[k], w, h, serr);
    if (as_rgbe) nch = 3;
    if (!as_ycbcr && !as_samples && !as_rgbe && !io::read_image(file, pixels[k], w, h, nch, err)) {
      std::fprintf(stderr, "envutil_hip: %s\n", err.c_str());
      return false;
    }
    kind = as_ycbcr ? KIND_YCBCR : as_samples ? (sbits == 8 ? KIND_SAMPLES_8 : KIND_SAMPLES_16) : as_rgbe ? KIND_RGBE : KIND_FLOATS;
    if (args.verbose) std::printf("%s: %s\n", file.c_str(), kind_name[kind]);
    if (args.verbose && f.edges)
      std::printf("%s: a distance plane of its alpha channel is built on the device (--feather_edges), %d x %d\n", file.c_str(),
                  f.window_width, f.window_height);
    // read_image_data: from the facet's colour space - Csp clause / --input_colour_space, else what the file's
    // format says - to the working one (envutil_basic.h:950-977). A video frame stays in its own non-linear space,
    // as its tables leave it
    if (!as_ycbcr) {
      const std::string csp = f.colour_space.empty() ? io::file_colour_space(file) : f.colour_space;
      if (args.verbose && csp != args.working_colour_space)
        std::printf("converting %s from %s to %s\n", file.c_str(), csp.c_str(), args.working_colour_space.c_str());
      io::colour_class ca, cb;
      bool same = false;
      const bool ok = as_samples ? io::sample_tables(sbits, maxval, csp, args.working_colour_space, colour_tab[k], alpha_tab[k], err)
                    // (no table where the colour spaces agree: the device's decode is the file route's)
                    : as_rgbe ? io::colour_pair(csp, args.working_colour_space, ca, cb, same, err) &&
                                (same || io::rgbe_table(csp, args.working_colour_space, colour_tab[k], err))
                                 : io::convert_colour(pixels[k].data(), size_t(w) * h, nch, csp, args.working_colour_space, err);
      if (!ok) {
        std::fprintf(stderr, "envutil_hip: %s: %s\n", file.c_str(), err.c_str());
        return false;
      }
    }
    const bool cube = f.projection == CUBEMAP || f.projection == BIATAN6;
    if (w != f.window_width || (cube ? h != 6 * w : h != f.window_height)) {
      std::fprintf(stderr, "envutil_hip: %s is %d x %d, expected %d x %d\n", file.c_str(), w, h,
                   f.window_width, cube ? 6 * f.window_width : f.window_height);
      return false;
    }
    // PTO masks and lens crops edit the loaded pixels (environment.h:700-890): the dispatch does that on the
    // device when it loads the facet, from the pixels at the file's own channel count
    const size_t count = as_ycbcr ? size_t(w) * h * 3 : as_samples ? samples[k].size() / size_t(sbits / 8) : as_rgbe ? samples[k].size() / 4 * 3 : pixels[k].size();
    if (!check_facet_pixels(f, count, nch, err)) {
      std::fprintf(stderr, "envutil_hip: %s: %s\n", file.c_str(), err.c_str());
      return false;
    }
    if (as_ycbcr) f.ycbcr = &ycc[k];
    else if (as_samples) {
      f.samples = samples[k].data(); f.sample_bits = sbits; f.samples_big_endian = true;
      f.colour_table = colour_tab[k].data(); f.alpha_table = alpha_tab[k].data();
    } else if (as_rgbe) {
      f.rgbe = samples[k].data();
      f.rgbe_table = colour_tab[k].empty() ? nullptr : colour_tab[k].data();
    } else f.pixels = pixels[k].data();
    return true;
  };
  int first_kind = 0, first_nch = 0;
  for (size_t k = 0; k < nimg; k++) {
    facet_spec &f = k < nfct ? args.facet_spec_v[k] : args.layer_spec_v[k - nfct];
    if (k < nfct && args.solo >= 0 && int(k) != args.solo) continue;
    if (dp->resident.count(f.asset_key)) {
      if (args.verbose) std::printf("asset %s is already resident\n", f.asset_key.c_str());
      continue;
    }
    // a sequence begins with its first frame; a .y4m facet without --frames is its frame 0
    std::string file = f.filename;
    if (sequence && io::lower_ext(file) != "y4m" && !io::frame_name(f.filename, args.frames_first, file, err)) {
      std::fprintf(stderr, "envutil_hip: %s\n", err.c_str());
      return 2;
    }
    if (!read_pixels(k, f, file, sequence ? args.frames_first : 0, first_kind, first_nch)) return 2;
  }

  // --frames FIRST LAST: the first frame is a load, every later one new pixels into the resident container
  // (eu_hip_source_reload, through the feed the file's type takes); each frame is rendered and written by the route
  // the output's type takes - the files of one run per frame
  if (sequence) {
    facet_spec &f = args.facet_spec_v[0];
    const std::string out_format = args.output;
    for (int k = args.frames_first; k <= args.frames_last; k++) {
      std::string file = f.filename, out;
      const bool stream = io::lower_ext(file) == "y4m";
      if (!stream && !io::frame_name(f.filename, k, file, err)) { std::fprintf(stderr, "envutil_hip: %s\n", err.c_str()); return 2; }
      if (y4m_out) out = out_format;              // one stream holds all frames
      else if (!io::frame_name(out_format, k, out, err)) { std::fprintf(stderr, "envutil_hip: %s\n", err.c_str()); return 2; }
      if (k > args.frames_first) {
        int kind = 0, nch = 0;
        if (!read_pixels(0, f, file, k, kind, nch)) { std::fprintf(stderr, "envutil_hip: frame %d could not be read\n", k); return 2; }
        if (kind != first_kind || nch != first_nch) {
          std::fprintf(stderr, "envutil_hip: frame %d (%s) holds %s at %d channels, frame %d %s at %d: the frames of a sequence share size, channels and file type\n",
                       k, file.c_str(), kind_name[kind], nch, args.frames_first, kind_name[first_kind], first_nch);
          return 2;
        }
        f.refill = true;
      }
      if (args.verbose)
        std::printf("frame %d: %s, %s\n", k, file.c_str(), f.refill ? "eu_hip_source_reload into the resident source" : "loaded as a new source");
      args.output = out;
      const int rc = run_payload(out);
      if (rc) return rc;
    }
    f.refill = false;
    args.output = out_format;
    return 0;
  }

  // --ray_map FILE: a 3-channel PFM of rays in the facet's frame
  std::vector<float> ray_map;
  args.p_ray_map = nullptr;
  if (!args.ray_map.empty()) {
    int w = 0, h = 0, nch = 0;
    if (!io::read_image(args.ray_map, ray_map, w, h, nch, err)) {
      std::fprintf(stderr, "envutil_hip: %s\n", err.c_str());
      return 2;
    }
    const std::string &n = args.ray_map;
    if (nch != 3 || n.size() < 4 || n.compare(n.size() - 4, 4, ".pfm") != 0) {
      std::fprintf(stderr, "envutil_hip: --ray_map %s: a ray map is a 3-channel PFM (x, y, z per pixel)\n", n.c_str());
      return 2;
    }
    args.p_ray_map = ray_map.data(); args.ray_map_width = w; args.ray_map_height = h;
    const int rc = run_payload(args.output);
    args.p_ray_map = nullptr;
    return rc;
  }

  if (!args.split.empty()) {
    int rc = 0;
    const int nfacets = args.nfacets;
    for (int i = 0; i < nfacets && rc == 0; i++) {
      if (i == args.solo) continue;
      static_cast<facet_base &>(args) = args.facet_spec_v[size_t(i)];
      args.single = i;
      args.store_cropped = false;
      args.output = series_name(args.split, i);
      rc = run_payload(args.output);
    }
    return rc;
  }
  if (args.single != -1) args.store_cropped = false;
  return run_payload(args.output);
}

int main(int argc, const char **argv)
{
  if (argc < 2) {
    std::fprintf(stderr, "usage: envutil_hip <envutil options> (see README.md); a trailing '-' reads jobs from stdin\n");
    return 2;
  }
  for (int i = 1; i < argc; i++)
    if (std::string(argv[i]) == "--help" || std::string(argv[i]) == "-h") {
      std::puts(
        "envutil_hip - envutil's reprojection on an MI355X (options as in envutil, envutil_main.cc:190-372)\n"
        "  source:   --facet IMAGE PROJECTION HFOV YAW PITCH ROLL (repeatable) | --photo IMAGE | --pto FILE [--pto_line LINE]\n"
        "            projections: spherical cylindrical rectilinear stereographic fisheye cubemap biatan6\n"
        "            --solo N  --single N  --split FORMAT(%d)  --mask_for N  --synopsis panorama|hdr_merge|feather|multiband\n"
        "            --feather WIDTH  with --synopsis feather or multiband: the blending ramp in source pixels (0: half the shorter side)\n"
        "            --feather_edges  with either: the ramp also falls towards mask, crop and alpha edges (a distance plane\n"
        "            per facet with alpha, 4 bytes per pixel)\n"
        "            --bands N  with --synopsis multiband: pyramid levels above level 0 (0: what the frame allows, 8 at the most);\n"
        "                       a multiband job of several facets is not twined: no automatic twining, --twine above 1 is refused\n"
        "  rays:     --ray_map FILE.pfm  the single facet's image at the rays x y z of a 3-channel PFM, in the facet's\n"
        "            frame (no yaw / pitch / roll, no twining); the output has the map's size\n"
        "  layers:   --layer IMAGE OUTPUT (repeatable)  a further picture of the single facet's geometry - same size and\n"
        "            channels - with an output of its own; all of them are rendered in one call, float route\n"
        "  target:   --output FILE  --projection P  --hfov DEG  --width W  --height H  --yaw --pitch --roll DEG\n"
        "            --x0 --x1 --y0 --y1 (extent instead of hfov)  --nchannels N  --brighten F\n"
        "  spline:   --degree D  --prefilter D  --support_min PX  --tile_size PX (cubemap sources)\n"
        "  twining:  --twine N (-1: automatic)  --twine_width F  --twine_density F  --twine_max N\n"
        "            --twine_sigma F  --twine_threshold F  --twine_normalize  --twine_precise  --twf_file FILE\n"
        "  frames:   --frames FIRST LAST  a sequence through ONE resident source: the single facet's image and --output hold\n"
        "            one integer conversion each (%d, %04d, ...), or the image is a .y4m stream (YUV4MPEG2; read forward);\n"
        "            the first frame is loaded, every later one refills the source in place\n"
        "            --ycbcr_matrix 601|709|2020 (default: 709 from 720 rows on, else 601)  --ycbcr_range limited|full\n"
        "  video out: an --output ending in .y4m is a YUV4MPEG2 stream, encoded on the device; with --frames one stream\n"
        "            holds all frames. --y4m_format 420|422|444  --y4m_depth 8|10|12|16  --fps N[:D] (default 25:1);\n"
        "            --ycbcr_matrix / --ycbcr_range say matrix and range (default: by the output's rows, limited)\n"
        "  images:   .pfm .hdr (float), .pgm .ppm .pnm (8 / 16 bit), .pam (8 / 16 bit, alpha), .y4m (frame 0 without --frames); a name with one %s\n"
        "            stands for six cube faces: left right top bottom front back\n"
        "            .hdr / .pic and the integer formats go to and from the device as the file's own pixels\n"
        "  -v verbose; a trailing '-' reads one job per line from stdin (sources stay resident in HBM)");
      return 0;
    }
  if (std::string(argv[argc - 1]) != "-") return core(argc, argv);
  argc--;
  int rc = 0;
  std::string line;
  while (std::getline(std::cin, line)) {
    const std::vector<std::string> sv = tokenize(line);
    if (sv.empty()) continue;
    std::vector<const char *> av(argv, argv + argc);
    for (const auto &t : sv) av.push_back(t.c_str());
    const int r = core(int(av.size()), av.data(), true);
    if (r) rc = r;
  }
  return rc;
}
