// samples_demo DIR - checks of io::sample_tables and io::read_samples (include/eu_image_io.hpp) against the float
// route they stand in for, io::read_image + io::convert_colour; files are written into DIR. Prints one line
// per failed check and "failures: N" at the end; the exit status is 0 when N is 0. Host code only.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "eu_image_io.hpp"

using namespace project;

static int failures = 0;
static void check(bool ok, const std::string &what)
{
  if (!ok) { failures++; std::printf("FAILED: %s\n", what.c_str()); }
}

static bool write_file(const std::string &name, const std::string &head, const std::vector<uint8_t> &body)
{
  FILE *f = std::fopen(name.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(head.data(), 1, head.size(), f) == head.size() &&
                  (body.empty() || std::fwrite(body.data(), 1, body.size(), f) == body.size());
  return std::fclose(f) == 0 && ok;
}

// every value of `bits` bits once, in order, as a PNM / PAM body (16 bit: big endian)
static std::vector<uint8_t> all_values(int bits)
{
  std::vector<uint8_t> b;
  for (unsigned v = 0; v < (1u << bits); v++) {
    if (bits == 16) b.push_back(uint8_t(v >> 8));
    b.push_back(uint8_t(v & 255u));
  }
  return b;
}

int main(int argc, char **argv)
{
  if (argc != 2) { std::fprintf(stderr, "usage: samples_demo DIR\n"); return 2; }
  const std::string dir = std::string(argv[1]) + "/";
  std::string err;

  // ---- the tables hold the bits of read_image + convert_colour, for every value a file can hold
  const int depth[4][2] = { { 8, 255 }, { 8, 100 }, { 16, 65535 }, { 16, 1000 } };
  const char *const space[3] = { "Linear", "sRGB", "Rec709" };
  for (const auto &d : depth) {
    const int bits = d[0], maxval = d[1], n = 1 << bits;
    const std::string name = dir + "all_" + std::to_string(bits) + "_" + std::to_string(maxval) + ".pgm";
    check(write_file(name, "P5\n256 " + std::to_string(n / 256) + "\n" + std::to_string(maxval) + "\n", all_values(bits)), "write " + name);
    for (const char *from : space)
      for (const char *to : space) {
        const std::string what = std::to_string(bits) + " bit, maxval " + std::to_string(maxval) + ", " + from + " -> " + to;
        std::vector<float> px, colour, alpha;
        int w = 0, h = 0, nch = 0;
        if (!io::read_image(name, px, w, h, nch, err)) { check(false, what + ": read_image: " + err); continue; }
        check(w * h == n && nch == 1, what + ": size");
        if (!io::sample_tables(bits, maxval, from, to, colour, alpha, err)) { check(false, what + ": sample_tables: " + err); continue; }
        check(colour.size() == size_t(n) && alpha.size() == size_t(n), what + ": table size");
        check(std::memcmp(alpha.data(), px.data(), size_t(n) * 4) == 0, what + ": alpha table");     // the unconverted floats
        if (!io::convert_colour(px.data(), size_t(n), 1, from, to, err)) { check(false, what + ": convert_colour: " + err); continue; }
        check(std::memcmp(colour.data(), px.data(), size_t(n) * 4) == 0, what + ": colour table");
      }
  }
  {
    // an unknown name: convert_colour's message, either side
    std::vector<float> colour, alpha, one(1, 0.5f);
    std::string e1, e2;
    check(!io::sample_tables(8, 255, "ACEScg", "Linear", colour, alpha, e1) && !io::convert_colour(one.data(), 1, 1, "ACEScg", "Linear", e2) && e1 == e2 && !e1.empty(),
          "unknown source colour space: " + e1);
    check(!io::sample_tables(16, 65535, "sRGB", "nope", colour, alpha, e1) && !io::convert_colour(one.data(), 1, 1, "sRGB", "nope", e2) && e1 == e2,
          "unknown working colour space: " + e1);
    // equal names need not be known ones (convert_colour's first early return)
    check(io::sample_tables(8, 255, "whatever", "whatever", colour, alpha, e1) && std::memcmp(colour.data(), alpha.data(), 256 * 4) == 0, "equal names");
    check(!io::sample_tables(12, 4095, "sRGB", "Linear", colour, alpha, e1), "12 bits refused");
  }

  // ---- read_samples returns the file's bytes
  struct file_case { const char *name; std::string head; int w, h, nch, maxval, bits; };
  const file_case files[] = {
    { "a.pgm", "P5\n# a comment\n7 5\n255\n", 7, 5, 1, 255, 8 },
    { "b.ppm", "P6\n7 5\n255\n", 7, 5, 3, 255, 8 },
    { "c.ppm", "P6\n5 3\n1000\n", 5, 3, 3, 1000, 16 },
    { "d.pam", "P7\nWIDTH 7\nHEIGHT 5\nDEPTH 2\nMAXVAL 200\nTUPLTYPE GRAYSCALE_ALPHA\nENDHDR\n", 7, 5, 2, 200, 8 },
    { "e.pam", "P7\nWIDTH 3\nHEIGHT 5\nDEPTH 4\nMAXVAL 65535\nTUPLTYPE RGB_ALPHA\nENDHDR\n", 3, 5, 4, 65535, 16 },
    { "f.pam", "P7\nWIDTH 3\nHEIGHT 2\nDEPTH 2\nMAXVAL 65535\nTUPLTYPE GRAYSCALE_ALPHA\nENDHDR\n", 3, 2, 2, 65535, 16 },
  };
  for (const auto &fc : files) {
    const std::string name = dir + fc.name;
    std::vector<uint8_t> body(size_t(fc.w) * fc.h * fc.nch * (fc.bits / 8));
    for (size_t i = 0; i < body.size(); i++) body[i] = uint8_t((i * 37u + 11u) ^ (i >> 3));
    check(write_file(name, fc.head, body), "write " + name);
    std::vector<uint8_t> got;
    int w = 0, h = 0, nch = 0, maxval = 0, bits = 0;
    if (!io::read_samples(name, got, w, h, nch, maxval, bits, err)) { check(false, std::string(fc.name) + ": read_samples: " + err); continue; }
    check(w == fc.w && h == fc.h && nch == fc.nch && maxval == fc.maxval && bits == fc.bits, std::string(fc.name) + ": header");
    check(got == body, std::string(fc.name) + ": bytes");
  }
  {
    // six cube faces by a format string: stacked in cubeface order
    static const char *const face[6] = { "left", "right", "top", "bottom", "front", "back" };
    std::vector<uint8_t> all;
    for (int i = 0; i < 6; i++) {
      std::vector<uint8_t> body(4 * 4 * 3);
      for (size_t k = 0; k < body.size(); k++) body[k] = uint8_t(40 * i + k);
      check(write_file(dir + "cube_" + face[i] + ".ppm", "P6\n4 4\n255\n", body), "write cube face");
      all.insert(all.end(), body.begin(), body.end());
    }
    std::vector<uint8_t> got;
    int w = 0, h = 0, nch = 0, maxval = 0, bits = 0;
    check(io::read_samples(dir + "cube_%s.ppm", got, w, h, nch, maxval, bits, err) && w == 4 && h == 24 && nch == 3 && bits == 8 && got == all,
          "six cube faces: " + err);
  }
  {
    // a float format is refused; a truncated file gives read_one's message
    std::vector<uint8_t> got, body(4 * 3 * 2 * 4, 0);
    int w = 0, h = 0, nch = 0, maxval = 0, bits = 0;
    check(write_file(dir + "x.pfm", "PF\n4 2\n-1.0\n", body), "write x.pfm");
    err.clear();
    check(!io::read_samples(dir + "x.pfm", got, w, h, nch, maxval, bits, err) && err.find("not an integer format") != std::string::npos,
          "a .pfm is refused: " + err);
    body.resize(10);
    check(write_file(dir + "cut.ppm", "P6\n7 5\n255\n", body), "write cut.ppm");
    std::vector<float> px;
    std::string e1, e2;
    check(!io::read_samples(dir + "cut.ppm", got, w, h, nch, maxval, bits, e1) && !io::read_image(dir + "cut.ppm", px, w, h, nch, e2) && e1 == e2 &&
            e1.find("truncated pixel data") != std::string::npos, "truncated file: '" + e1 + "' / '" + e2 + "'");
    check(write_file(dir + "head.ppm", "P6\n7", std::vector<uint8_t>()), "write head.ppm");
    check(!io::read_samples(dir + "head.ppm", got, w, h, nch, maxval, bits, e1) && !io::read_image(dir + "head.ppm", px, w, h, nch, e2) && e1 == e2 && !e1.empty(),
          "truncated header: '" + e1 + "' / '" + e2 + "'");
    check(!io::read_samples(dir + "none.ppm", got, w, h, nch, maxval, bits, e1) && !io::read_image(dir + "none.ppm", px, w, h, nch, e2) && e1 == e2,
          "missing file: '" + e1 + "' / '" + e2 + "'");
  }
  std::printf("failures: %d\n", failures);
  return failures ? 1 : 0;
}
