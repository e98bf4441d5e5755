// Host program for the frame-sequence parts of include/eu_image_io.hpp (TEST CODE): the YUV4MPEG2 header parser and
// reader, the names of a numbered sequence and the argument checks of --frames. No HIP library is needed.
//   frames_demo header "YUV4MPEG2 W.. H.. C.."     -> "ok W H sub_x sub_y bits depth full y_bytes c_bytes" | "refused: ..."
//   frames_demo check FIRST LAST IMAGE OUTPUT      -> "ok FIRST LAST" | "refused: ..."
//   frames_demo name FORMAT K                      -> "ok NAME" | "refused: ..."
//   frames_demo read FILE K [K ...]                -> per K "frame K: BYTES bytes, sum S" | "refused: ..."
//   frames_demo selftest DIR                       -> writes small streams of every accepted colour tag at odd sizes into
//        DIR, reads them back frame by frame, a truncated one too; the program to build with -fsanitize=address,undefined
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "eu_image_io.hpp"

using namespace project;

static uint8_t byte_of(int frame, size_t i) { return uint8_t((frame * 131 + int(i) * 7 + 3) & 0xff); }

static bool write_stream(const std::string &name, const std::string &header, size_t frame_bytes, int nframes, size_t cut)
{
  FILE *f = std::fopen(name.c_str(), "wb");
  if (!f) return false;
  std::fprintf(f, "%s\n", header.c_str());
  for (int k = 0; k < nframes; k++) {
    std::fprintf(f, k == 1 ? "FRAME Ip\n" : "FRAME\n");
    std::vector<uint8_t> b(frame_bytes);
    for (size_t i = 0; i < b.size(); i++) b[i] = byte_of(k, i);
    const size_t n = k == nframes - 1 ? b.size() - cut : b.size();
    std::fwrite(b.data(), 1, n, f);
  }
  std::fclose(f);
  return true;
}

static int selftest(const std::string &dir)
{
  int failed = 0, cases = 0;
  auto expect = [&](bool ok, const std::string &what) { cases++; if (!ok) { failed++; std::printf("FAILED %s\n", what.c_str()); } };
  struct tag_case { const char *tag; int sub_x, sub_y, bits, depth; };
  const tag_case good[] = { { "", 2, 2, 8, 8 }, { "C420", 2, 2, 8, 8 }, { "C420jpeg", 2, 2, 8, 8 }, { "C420mpeg2", 2, 2, 8, 8 }, { "C420paldv", 2, 2, 8, 8 },
                            { "C422", 2, 1, 8, 8 }, { "C444", 1, 1, 8, 8 }, { "C420p10", 2, 2, 16, 10 }, { "C420p12", 2, 2, 16, 12 }, { "C420p16", 2, 2, 16, 16 },
                            { "C422p10", 2, 1, 16, 10 }, { "C422p12", 2, 1, 16, 12 }, { "C422p16", 2, 1, 16, 16 }, { "C444p10", 1, 1, 16, 10 },
                            { "C444p12", 1, 1, 16, 12 }, { "C444p16", 1, 1, 16, 16 } };
  const int sizes[][2] = { { 1, 1 }, { 5, 3 }, { 3, 5 }, { 8, 2 } };
  for (const auto &t : good)
    for (const auto &wh : sizes) {
      const int w = wh[0], h = wh[1];
      const std::string header = "YUV4MPEG2 W" + std::to_string(w) + " H" + std::to_string(h) + " F25:1 Ip A1:1" + (t.tag[0] ? std::string(" ") + t.tag : "") + " XYSCSS=TEST";
      io::y4m_info info;
      std::string err;
      expect(io::y4m_parse_header(header, info, err), header + ": " + err);
      const size_t sb = size_t(t.bits / 8), cw = size_t(w + t.sub_x - 1) / t.sub_x, ch = size_t(h + t.sub_y - 1) / t.sub_y;
      expect(info.sub_x == t.sub_x && info.sub_y == t.sub_y && info.bits == t.bits && info.depth == t.depth && !info.full_range &&
             info.y_bytes == size_t(w) * h * sb && info.c_bytes == cw * ch * sb, header + ": what the header says");
      const std::string name = dir + "/t.y4m";
      expect(write_stream(name, header, info.frame_bytes(), 3, 0), "writing " + name);
      io::y4m_reader r;
      std::vector<uint8_t> planes;
      expect(r.open(name, err), err);
      for (int k : { 0, 2 }) {
        bool ok = r.frame(k, planes, err) && planes.size() == info.frame_bytes();
        for (size_t i = 0; ok && i < planes.size(); i++) ok = planes[i] == byte_of(k, i);
        expect(ok, header + ": frame " + std::to_string(k) + " " + err);
      }
      expect(!r.frame(1, planes, err) && err.find("forward") != std::string::npos, "a frame behind the position");
      expect(!r.frame(3, planes, err) && err.find("ends") != std::string::npos, "a frame behind the last: " + err);
      // the last frame one byte short
      expect(write_stream(name, header, info.frame_bytes(), 2, 1), "writing " + name);
      io::y4m_reader cut;
      expect(cut.open(name, err) && cut.frame(0, planes, err), "the whole frame of a cut stream: " + err);
      expect(!cut.frame(1, planes, err) && err.find("truncated") != std::string::npos, "a truncated frame: " + err);
    }
  for (const char *bad : { "Cmono", "Cmono16", "C444alpha", "C420jpegp10", "C411", "C420p9", "C", "C420p" }) {
    io::y4m_info info;
    std::string err;
    expect(!io::y4m_parse_header(std::string("YUV4MPEG2 W4 H4 ") + bad, info, err) && err.find("colour tag") != std::string::npos, std::string("refusing ") + bad);
  }
  {
    io::y4m_info info;
    std::string err;
    expect(io::y4m_parse_header("YUV4MPEG2 W4 H4 C444 XCOLORRANGE=FULL", info, err) && info.full_range, "XCOLORRANGE=FULL");
    expect(!io::y4m_parse_header("YUV4MPEG W4 H4", info, err), "another magic");
    expect(!io::y4m_parse_header("YUV4MPEG2 H4", info, err), "no width");
    expect(!io::y4m_parse_header("YUV4MPEG2 W-3 H4", info, err), "a negative width");
    expect(!io::y4m_parse_header("", info, err), "an empty header");
  }
  {
    std::string out, err;
    int a = 0, b = 0;
    expect(io::frame_name("f%04d.ppm", 7, out, err) && out == "f0007.ppm", "f%04d.ppm");
    expect(io::frame_name("%d", 12, out, err) && out == "12", "%d");
    expect(!io::frame_name("f.ppm", 7, out, err) && err.find("no conversion") != std::string::npos, "no conversion");
    expect(!io::frame_name("f%d_%d.ppm", 7, out, err), "two conversions");
    expect(!io::frame_name("f%s.ppm", 7, out, err), "%s");
    expect(!io::frame_name("f%d%%.ppm", 7, out, err), "a second percent sign");
    expect(!io::frame_name("f%", 7, out, err), "a percent sign at the end");
    expect(io::check_frames("0", "9", "in%d.pfm", "out%03d.pfm", a, b, err) && a == 0 && b == 9, "0 9");
    expect(io::check_frames("3", "3", "in.y4m", "out%d.ppm", a, b, err), "a stream");
    expect(!io::check_frames("5", "4", "in%d.pfm", "out%d.pfm", a, b, err) && err.find("beyond") != std::string::npos, "FIRST > LAST");
    expect(!io::check_frames("-1", "4", "in%d.pfm", "out%d.pfm", a, b, err), "a negative number");
    expect(!io::check_frames("1", "x", "in%d.pfm", "out%d.pfm", a, b, err), "not a number");
    expect(!io::check_frames("1", "2", "in.pfm", "out%d.pfm", a, b, err) && err.find("image") != std::string::npos, "an image without a conversion");
    expect(!io::check_frames("1", "2", "in%d_%d.pfm", "out%d.pfm", a, b, err), "an image with two conversions");
    expect(!io::check_frames("1", "2", "face_%s.pfm", "out%d.pfm", a, b, err) && err.find("cubemap") != std::string::npos, "a six-file cubemap name");
    expect(!io::check_frames("1", "2", "in%d.pfm", "out.pfm", a, b, err) && err.find("--output") != std::string::npos, "an output without a conversion");
    expect(!io::check_frames("1", "2", "in.y4m", "out%d%d.pfm", a, b, err), "an output with two conversions");
  }
  std::printf("%d checks, %d failed\n", cases, failed);
  if (!failed) std::printf("all ok\n");
  return failed ? 1 : 0;
}

int main(int argc, char **argv)
{
  const std::string mode = argc > 1 ? argv[1] : "";
  std::string err;
  if (mode == "selftest" && argc == 3) return selftest(argv[2]);
  if (mode == "header" && argc == 3) {
    io::y4m_info i;
    if (!io::y4m_parse_header(argv[2], i, err)) { std::printf("refused: %s\n", err.c_str()); return 0; }
    std::printf("ok %d %d %d %d %d %d %d %zu %zu\n", i.width, i.height, i.sub_x, i.sub_y, i.bits, i.depth, int(i.full_range), i.y_bytes, i.c_bytes);
    return 0;
  }
  if (mode == "check" && argc == 6) {
    int a = 0, b = 0;
    if (!io::check_frames(argv[2], argv[3], argv[4], argv[5], a, b, err)) { std::printf("refused: %s\n", err.c_str()); return 0; }
    std::printf("ok %d %d\n", a, b);
    return 0;
  }
  if (mode == "name" && argc == 4) {
    std::string out;
    if (!io::frame_name(argv[2], std::atoi(argv[3]), out, err)) { std::printf("refused: %s\n", err.c_str()); return 0; }
    std::printf("ok %s\n", out.c_str());
    return 0;
  }
  if (mode == "read" && argc >= 4) {
    io::y4m_reader r;
    if (!r.open(argv[2], err)) { std::printf("refused: %s\n", err.c_str()); return 0; }
    std::vector<uint8_t> planes;
    for (int a = 3; a < argc; a++) {
      const int k = std::atoi(argv[a]);
      if (!r.frame(k, planes, err)) { std::printf("refused: %s\n", err.c_str()); continue; }
      unsigned long sum = 0;
      for (uint8_t v : planes) sum += v;
      std::printf("frame %d: %zu bytes, sum %lu\n", k, planes.size(), sum);
    }
    return 0;
  }
  std::fprintf(stderr, "usage: frames_demo header|check|name|read|selftest ...\n");
  return 2;
}
