// Stand-alone host program over the host side of the Y'CbCr way out: io::y4m_writer, io::ycbcr_steps,
// io::ycbcr_forward (include/eu_image_io.hpp) and the host loop of include/eu_ycbcr.h. No device, no library.
//   ycbcr_out_demo selftest DIR                       every format and depth at odd sizes, written and read back
//   ycbcr_out_demo steps BITS DEPTH FULL OUT          y_steps then c_steps as raw floats
//   ycbcr_out_demo encode FRAME.f32 W H FORMAT DEPTH MATRIX OUT.y4m
//                                                     a 3-channel float frame through eu_ycbcr_planes_rows into a stream
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "eu_image_io.hpp"
#include "eu_ycbcr.h"

using namespace project;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static int selftest(const std::string &dir)
{
  std::string err;
  const char *formats[] = { "420", "422", "444" };
  const int depths[] = { 8, 10, 12, 16 };
  const int sizes[][2] = { { 1, 1 }, { 3, 5 }, { 7, 2 }, { 17, 9 } };
  int n = 0;
  for (const char *fmt : formats)
    for (int depth : depths)
      for (const auto &sz : sizes) {
        const bool full = (n++ & 1) != 0;
        const std::string file = dir + "/t" + std::to_string(n) + ".y4m";
        io::y4m_writer w;
        CHECK(w.open(file, sz[0], sz[1], fmt, depth, full, 30000, 1001, err), "%s", err.c_str());
        const std::string tag = depth == 8 ? (std::string(fmt) == "420" ? "420jpeg" : fmt) : std::string(fmt) + "p" + std::to_string(depth);
        const std::string want = "YUV4MPEG2 W" + std::to_string(sz[0]) + " H" + std::to_string(sz[1]) + " F30000:1001 Ip A1:1 C" + tag +
                                 (full ? " XCOLORRANGE=FULL" : "");
        CHECK(io::y4m_writer::header(w.info, w.tag, 30000, 1001) == want, "header '%s'", io::y4m_writer::header(w.info, w.tag, 30000, 1001).c_str());
        const int sx = std::string(fmt) == "444" ? 1 : 2, sy = std::string(fmt) == "420" ? 2 : 1, sb = depth == 8 ? 1 : 2;
        CHECK(w.info.sub_x == sx && w.info.sub_y == sy && w.info.bits == 8 * sb && w.info.depth == depth, "layout of C%s", tag.c_str());
        const size_t cw = (sz[0] + sx - 1) / sx, ch = (sz[1] + sy - 1) / sy;
        CHECK(w.info.frame_bytes() == (size_t(sz[0]) * sz[1] + 2 * cw * ch) * sb, "frame bytes of C%s", tag.c_str());
        std::vector<std::vector<uint8_t>> frames(3, std::vector<uint8_t>(w.info.frame_bytes()));
        for (size_t k = 0; k < frames.size(); k++) {
          if (sb == 1) for (size_t i = 0; i < frames[k].size(); i++) frames[k][i] = uint8_t(i * 7 + k * 31 + n);
          else for (size_t i = 0; i + 1 < frames[k].size(); i += 2) {
            const uint16_t v = uint16_t((i * 77 + k * 311 + n) & ((1u << depth) - 1));
            std::memcpy(&frames[k][i], &v, 2);
          }
          CHECK(w.frame(frames[k].data(), err), "%s", err.c_str());
        }
        CHECK(w.frames == 3 && w.close(err), "close");
        // the stream's first line is the header; the reader finds the same layout and the same planes
        io::y4m_reader r;
        CHECK(r.open(file, err), "%s", err.c_str());
        CHECK(r.info.width == sz[0] && r.info.height == sz[1] && r.info.sub_x == sx && r.info.sub_y == sy && r.info.bits == 8 * sb &&
              r.info.depth == depth && r.info.full_range == full, "reader's layout of C%s", tag.c_str());
        std::vector<uint8_t> back;
        for (int k : { 0, 2 }) {
          CHECK(r.frame(k, back, err), "%s", err.c_str());
          CHECK(back == frames[size_t(k)], "frame %d of %s differs", k, file.c_str());
        }
        CHECK(!r.frame(3, back, err), "a fourth frame");
        // 16-bit samples are little-endian words in the file
        if (sb == 2) {
          FILE *f = std::fopen(file.c_str(), "rb");
          std::string line;
          io::y4m_reader::line(f, line); io::y4m_reader::line(f, line);
          const int lo = std::fgetc(f), hi = std::fgetc(f);
          uint16_t v;
          std::memcpy(&v, &frames[0][0], 2);
          CHECK(lo == (v & 255) && hi == (v >> 8), "byte order");
          std::fclose(f);
        }
      }
  io::y4m_writer w;
  CHECK(!w.open(dir + "/bad.y4m", 4, 4, "411", 8, false, 25, 1, err) && err.find("--y4m_format") != std::string::npos, "format 411");
  CHECK(!w.open(dir + "/bad.y4m", 4, 4, "420", 9, false, 25, 1, err) && err.find("--y4m_depth") != std::string::npos, "depth 9");
  CHECK(!w.open(dir + "/bad.y4m", 4, 4, "420", 8, false, 0, 1, err) && err.find("--fps") != std::string::npos, "fps 0");
  CHECK(!w.open(dir + "/bad.y4m", 0, 4, "420", 8, false, 25, 1, err), "width 0");
  CHECK(!w.open(dir + "/no/such/dir/x.y4m", 4, 4, "420", 8, false, 25, 1, err) && err.find("cannot write") != std::string::npos, "no directory");
  std::vector<uint8_t> none(64);
  CHECK(!w.frame(none.data(), err), "frame without a file");
  int a = 0, b = 0;
  CHECK(io::parse_fps("25", a, b) && a == 25 && b == 1, "fps 25");
  CHECK(io::parse_fps("30000:1001", a, b) && a == 30000 && b == 1001, "fps 30000:1001");
  CHECK(!io::parse_fps("", a, b) && !io::parse_fps("25:", a, b) && !io::parse_fps("25:0", a, b) && !io::parse_fps("x", a, b) &&
        !io::parse_fps("-3", a, b) && !io::parse_fps("2.5", a, b), "bad fps");
  // check_frames: a .y4m output needs no conversion, every other extension still does
  int first = 0, last = 0;
  CHECK(io::check_frames("0", "3", "clip.y4m", "out.y4m", first, last, err) && first == 0 && last == 3, "%s", err.c_str());
  CHECK(io::check_frames("0", "3", "in%03d.ppm", "out.Y4M", first, last, err), "%s", err.c_str());
  CHECK(!io::check_frames("0", "3", "clip.y4m", "out.ppm", first, last, err) && err.find("--output") != std::string::npos, "out.ppm");
  // the steps: a few by hand. Limited range 8 bit: code 16 from -0.5 / 219 on, code 235 at 1.0; chroma 128 at 0
  std::vector<float> ys, cs;
  CHECK(io::ycbcr_steps(8, 8, false, ys, cs) && ys.size() == 256 && cs.size() == 256, "steps 8");
  CHECK(eu_ycbcr_code(ys.data(), 8, 0.0f) == 16 && eu_ycbcr_code(ys.data(), 8, 1.0f) == 235 && eu_ycbcr_code(ys.data(), 8, 2.0f) == 255 &&
        eu_ycbcr_code(ys.data(), 8, -1.0f) == 0, "luma codes");
  CHECK(eu_ycbcr_code(cs.data(), 8, 0.0f) == 128 && eu_ycbcr_code(cs.data(), 8, 0.5f) == 240 && eu_ycbcr_code(cs.data(), 8, -0.5f) == 16, "chroma codes");
  CHECK(io::ycbcr_steps(16, 10, true, ys, cs) && ys.size() == 65536, "steps 10");
  CHECK(eu_ycbcr_code(ys.data(), 16, 1.0f) == 1023 && eu_ycbcr_code(ys.data(), 16, 1e30f) == 1023 && ys[1024] != ys[1024] && ys[65535] != ys[65535], "10-bit codes end at 1023");
  CHECK(eu_ycbcr_code(cs.data(), 16, 0.0f) == 512, "10-bit chroma zero");
  CHECK(!io::ycbcr_steps(8, 10, false, ys, cs) && !io::ycbcr_steps(12, 12, false, ys, cs), "bad bits / depth");
  float k[5];
  CHECK(io::ycbcr_forward("709", k, err) && k[0] == 0.2126f && k[2] == 0.0722f && k[1] == float(1.0 - 0.2126 - 0.0722), "forward 709");
  CHECK(!io::ycbcr_forward("240", k, err), "forward 240");
  std::printf("failures: %d\n", failures);
  return failures ? 1 : 0;
}

int main(int argc, char **argv)
{
  const std::string cmd = argc > 1 ? argv[1] : "";
  std::string err;
  if (cmd == "selftest" && argc == 3) return selftest(argv[2]);
  if (cmd == "steps" && argc == 6) {
    std::vector<float> ys, cs;
    if (!io::ycbcr_steps(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]) != 0, ys, cs)) return 2;
    FILE *f = std::fopen(argv[5], "wb");
    if (!f) return 2;
    const bool ok = std::fwrite(ys.data(), 4, ys.size(), f) == ys.size() && std::fwrite(cs.data(), 4, cs.size(), f) == cs.size();
    return std::fclose(f) == 0 && ok ? 0 : 2;
  }
  if (cmd == "encode" && argc == 9) {
    const int w = std::atoi(argv[3]), h = std::atoi(argv[4]), depth = std::atoi(argv[6]);
    if (w < 1 || h < 1) return 2;
    std::vector<float> frame(size_t(w) * h * 3);
    FILE *f = std::fopen(argv[2], "rb");
    if (!f || std::fread(frame.data(), 4, frame.size(), f) != frame.size()) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    std::fclose(f);
    io::y4m_writer wr;
    if (!wr.open(argv[8], w, h, argv[5], depth, false, 25, 1, err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 2; }
    std::vector<float> ys, cs;
    float k[5];
    if (!io::ycbcr_steps(wr.info.bits, wr.info.depth, false, ys, cs) || !io::ycbcr_forward(argv[7], k, err)) return 2;
    std::vector<uint8_t> planes(wr.info.frame_bytes());
    const size_t sb = size_t(wr.info.bits / 8), cw = (size_t(w) + wr.info.sub_x - 1) / wr.info.sub_x;
    eu_ycbcr_planes_rows(frame.data(), size_t(w) * 12, w, h, 3, planes.data(), planes.data() + wr.info.y_bytes,
                         planes.data() + wr.info.y_bytes + wr.info.c_bytes, size_t(w) * sb, cw * sb, 1, wr.info.sub_x, wr.info.sub_y,
                         wr.info.bits, 0, ys.data(), cs.data(), k[0], k[1], k[2], k[3], k[4]);
    if (!wr.frame(planes.data(), err) || !wr.close(err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 2; }
    return 0;
  }
  std::fprintf(stderr, "usage: ycbcr_out_demo selftest DIR | steps BITS DEPTH FULL OUT | encode FRAME.f32 W H FORMAT DEPTH MATRIX OUT.y4m\n");
  return 2;
}
