// Radiance RGBE pixels, host side (tests/test_rgbe_host.py): the two pixel functions of include/eu_rgbe.h against
// the expressions the file route used before them - kept here verbatim, they are the yardstick - and the readers,
// the table and the writers of include/eu_image_io.hpp.
//   rgbe_demo check DIR        every check below, files in DIR; prints "failures: N"
//   rgbe_demo encode IN OUT    IN: n x 3 float32, OUT: n quads of eu_rgbe_encode
//   rgbe_demo decode IN OUT    IN: n quads, OUT: n x 3 float32 of eu_rgbe_decode
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "eu_image_io.hpp"

using namespace project;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// write_one's pixel expression as it stood before eu_rgbe.h, verbatim. Defined for a largest channel below 2^127.
static void old_encode(float r, float g, float b, uint8_t *p)
{
  float v = r > g ? r : g;
  v = b > v ? b : v;
  if (!(v >= 1e-32f)) { p[0] = p[1] = p[2] = p[3] = 0; return; }     // also NaN and negatives
  int e;
  const float m = std::frexp(v, &e) * 256.0f / v;
  p[0] = uint8_t(r > 0.0f ? r * m : 0.0f); p[1] = uint8_t(g > 0.0f ? g * m : 0.0f);
  p[2] = uint8_t(b > 0.0f ? b * m : 0.0f); p[3] = uint8_t(e + 128);
}

// read_one's pixel expression as it stood, verbatim
static void old_decode(const uint8_t *p, float *d)
{
  if (p[3]) {
    const float fexp = std::ldexp(1.0f, int(p[3]) - (128 + 8));
    d[0] = p[0] * fexp; d[1] = p[1] * fexp; d[2] = p[2] * fexp;
  } else d[0] = d[1] = d[2] = 0.0f;
}

static uint32_t bits_of(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }
static float float_of(uint32_t u) { float v; std::memcpy(&v, &u, 4); return v; }
static uint32_t quad_of(const uint8_t *p) { return io::rgbe_quad(p); }

static void same_as_old(float r, float g, float b)
{
  uint8_t p[4];
  old_encode(r, g, b, p);
  const uint32_t got = eu_rgbe_encode(r, g, b);
  CHECK(got == quad_of(p), "encode(%a, %a, %a) = %08x, the old expression gives %08x", r, g, b, got, quad_of(p));
}

static void check_encode()
{
  std::mt19937 rng(20251);
  const uint32_t e_lo = bits_of(1e-32f) >> 23;
  const float nan = std::nanf(""), specials[] = { -1.0f, -0.0f, 0.0f, nan, -HUGE_VALF, -1e-40f, 1e-40f };
  for (uint32_t e = e_lo; e <= 253; e++)
    for (int rep = 0; rep < 400; rep++) {
      const float v = float_of((e << 23) | (rng() & 0x7fffffu));
      // the other channels: a random fraction of v, a random float below it, a tie
      const float frac = v * (float(rng() >> 8) / 16777216.0f);
      const float lower = float_of(rng() % (bits_of(v) + 1u));
      const float others[] = { frac, lower, v, 0.5f * v, float_of(bits_of(v) - 1u) };
      const float a = others[rng() % 5], b = others[rng() % 5];
      // the largest channel in each position
      same_as_old(v, a, b); same_as_old(a, v, b); same_as_old(a, b, v);
      // negative, zero of both signs, NaN, denormals in each position
      for (float s : specials) {
        same_as_old(s, v, a); same_as_old(v, s, a); same_as_old(v, a, s);
        same_as_old(s, s, v); same_as_old(s, v, s); same_as_old(v, s, s);
      }
    }
  // nothing to encode
  for (float s : specials) for (float t : specials) { same_as_old(s, t, s); same_as_old(t, s, s); same_as_old(s, s, t); }
  // 1e-32f and its two neighbours
  for (int d = -1; d <= 1; d++) {
    const float v = float_of(bits_of(1e-32f) + d);
    same_as_old(v, 0.0f, 0.0f); same_as_old(0.5f * v, v, -v); same_as_old(nan, 0.0f, v); same_as_old(v, v, v);
  }
  CHECK(eu_rgbe_encode(float_of(bits_of(1e-32f) - 1u), 0.0f, 0.0f) == 0u, "below 1e-32f: four zero bytes");
  CHECK(eu_rgbe_encode(1e-32f, 0.0f, 0.0f) != 0u, "1e-32f is encoded");

  // at and above 2^127: every channel clamped from above to 255 * 2^119, then the old expression
  const float top = EU_RGBE_MAX, tops[] = { 0x1p127f, FLT_MAX, HUGE_VALF, top, float_of(bits_of(top) + 1u), 3e38f };
  CHECK(top == 255.0f * 0x1p119f, "EU_RGBE_MAX");
  for (float v : tops) {
    const float others[] = { 0.0f, -1.0f, nan, 1.0f, 0.5f * top, 0x1p126f, top, v, FLT_MAX, HUGE_VALF };
    for (float a : others) for (float b : others) {
      const float in[3][3] = { { v, a, b }, { a, v, b }, { a, b, v } };
      for (const auto &c : in) {
        uint8_t p[4];
        old_encode(c[0] > top ? top : c[0], c[1] > top ? top : c[1], c[2] > top ? top : c[2], p);
        const uint32_t got = eu_rgbe_encode(c[0], c[1], c[2]);
        CHECK(got == quad_of(p), "encode(%a, %a, %a) = %08x, the clamped definition gives %08x", c[0], c[1], c[2], got, quad_of(p));
        // the largest channel as the two compares choose it: a NaN in the second place hides the first, as ever
        float m = c[0] > c[1] ? c[0] : c[1];
        m = c[2] > m ? c[2] : m;
        CHECK((got >> 24) == (m >= top ? 255u : m >= 1e-32f ? uint32_t(p[3]) : 0u), "encode(%a, %a, %a): exponent byte %u", c[0], c[1], c[2], got >> 24);
      }
    }
    if (v >= top) CHECK(eu_rgbe_encode(v, 0.0f, 0.0f) == 0xff0000ffu, "encode(%a, 0, 0) = %08x", v, eu_rgbe_encode(v, 0.0f, 0.0f));
  }
  CHECK(eu_rgbe_encode(0x1p127f, 0x1p126f, -1.0f) == 0xff0080ffu, "2^127, 2^126, -1: %08x", eu_rgbe_encode(0x1p127f, 0x1p126f, -1.0f));
  CHECK(eu_rgbe_encode(HUGE_VALF, HUGE_VALF, nan) == 0xff00ffffu, "inf, inf, NaN: %08x", eu_rgbe_encode(HUGE_VALF, HUGE_VALF, nan));
  // the largest value below the bound that has a mantissa of its own
  CHECK(eu_rgbe_encode(254.0f * 0x1p119f, 0.0f, 0.0f) == 0xff0000feu, "254 * 2^119");
}

static void check_decode()
{
  for (uint32_t e = 0; e < 256; e++)
    for (uint32_t m = 0; m < 256; m++) {
      const uint8_t p[4] = { uint8_t(m), uint8_t(255u - m), uint8_t(m ^ 0x55u), uint8_t(e) };
      float want[3], got[3];
      old_decode(p, want);
      eu_rgbe_decode(quad_of(p), &got[0], &got[1], &got[2]);
      for (int c = 0; c < 3; c++) {
        CHECK(bits_of(got[c]) == bits_of(want[c]), "decode: mantissa %u, exponent %u: %a, the old expression gives %a", p[c], e, got[c], want[c]);
        const float def = e ? float(p[c]) * std::ldexp(1.0f, int(e) - 136) : 0.0f;
        CHECK(bits_of(got[c]) == bits_of(def), "decode: mantissa %u, exponent %u: %a, the definition gives %a", p[c], e, got[c], def);
      }
    }
}

// decode, then encode: the same quad - for the quads an encoder emits, whose largest mantissa is at least 128 and
// whose largest channel is not below 1e-32f (smaller ones encode as four zero bytes)
static void check_round_trip()
{
  std::mt19937 rng(7);
  long n = 0;
  for (uint32_t e = 1; e < 256; e++)
    for (uint32_t top = 128; top < 256; top++)
      for (int pos = 0; pos < 3; pos++)
        for (int rep = 0; rep < 8; rep++) {
          uint8_t p[4] = { uint8_t(rng() % (top + 1)), uint8_t(rng() % (top + 1)), uint8_t(rng() % (top + 1)), uint8_t(e) };
          if (rep == 0) p[0] = p[1] = p[2] = 0;
          if (rep == 1) p[0] = p[1] = p[2] = uint8_t(top);
          p[pos] = uint8_t(top);
          float f[3];
          eu_rgbe_decode(quad_of(p), &f[0], &f[1], &f[2]);
          if (!(f[pos] >= 1e-32f)) continue;
          n++;
          const uint32_t back = eu_rgbe_encode(f[0], f[1], f[2]);
          CHECK(back == quad_of(p), "round trip: %08x became %08x", quad_of(p), back);
        }
  CHECK(n > 600000, "round trip: only %ld quads were tried", n);
}

static std::string header_text(int w, int h) { return "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y " + std::to_string(h) + " +X " + std::to_string(w) + "\n"; }

static bool put(const std::string &name, const std::string &head, const std::vector<uint8_t> &body)
{
  FILE *f = std::fopen(name.c_str(), "wb");
  if (!f) return false;
  bool ok = std::fwrite(head.data(), 1, head.size(), f) == head.size() && (body.empty() || std::fwrite(body.data(), 1, body.size(), f) == body.size());
  return std::fclose(f) == 0 && ok;
}

static std::vector<uint8_t> get(const std::string &name)
{
  std::vector<uint8_t> b;
  FILE *f = std::fopen(name.c_str(), "rb");
  if (!f) return b;
  int c;
  while ((c = std::fgetc(f)) != EOF) b.push_back(uint8_t(c));
  std::fclose(f);
  return b;
}

// the new run-length encoding of the quads, scanline by scanline: runs of 2 .. 127 equal bytes, literals between
static std::vector<uint8_t> rle(const std::vector<uint8_t> &quads, int w, int h)
{
  std::vector<uint8_t> out;
  for (int y = 0; y < h; y++) {
    out.insert(out.end(), { 2, 2, uint8_t(w >> 8), uint8_t(w & 255) });
    for (int c = 0; c < 4; c++) {
      std::vector<uint8_t> line(size_t(w), 0);
      for (int x = 0; x < w; x++) line[size_t(x)] = quads[(size_t(y) * w + x) * 4 + c];
      int x = 0;
      while (x < w) {
        int run = 1;
        while (x + run < w && run < 127 && line[size_t(x + run)] == line[size_t(x)]) run++;
        if (run >= 2) { out.push_back(uint8_t(128 + run)); out.push_back(line[size_t(x)]); x += run; continue; }
        int lit = 1;
        while (x + lit < w && lit < 128 && !(x + lit + 1 < w && line[size_t(x + lit)] == line[size_t(x + lit + 1)])) lit++;
        out.push_back(uint8_t(lit));
        for (int i = 0; i < lit; i++) out.push_back(line[size_t(x + i)]);
        x += lit;
      }
    }
  }
  return out;
}

static void check_files(const std::string &dir)
{
  std::mt19937 rng(99);
  const int w = 37, h = 11;
  std::vector<uint8_t> quads(size_t(w) * h * 4);
  for (size_t i = 0; i < quads.size(); i++) quads[i] = uint8_t(rng());
  // runs, so that the run-length form holds both kinds of packet
  for (int y = 0; y < h; y += 2) for (int x = 5; x < 30; x++) for (int c = 0; c < 4; c++) quads[(size_t(y) * w + x) * 4 + c] = uint8_t(17 * c + y);
  for (int x = 0; x < w; x++) quads[(size_t(3) * w + x) * 4 + 3] = 0;                       // a row of zero exponents
  const std::string flat = dir + "/flat.hdr", packed = dir + "/packed.hdr";
  const std::vector<uint8_t> body = rle(quads, w, h);
  CHECK(put(flat, header_text(w, h), quads) && put(packed, header_text(w, h), body), "cannot write into %s", dir.c_str());
  CHECK(body.size() < quads.size(), "the run-length form is smaller here");

  std::string err;
  for (const std::string &name : { flat, packed }) {
    std::vector<uint8_t> got;
    int gw = 0, gh = 0;
    CHECK(io::read_rgbe(name, got, gw, gh, err), "%s", err.c_str());
    CHECK(gw == w && gh == h && got == quads, "%s: read_rgbe returns other quads", name.c_str());
    // ... and read_image their decode
    std::vector<float> px;
    int nch = 0;
    CHECK(io::read_image(name, px, gw, gh, nch, err) && nch == 3 && px.size() == size_t(w) * h * 3, "%s", err.c_str());
    size_t bad = 0;
    for (size_t i = 0; i < size_t(w) * h && px.size() == size_t(w) * h * 3; i++) {
      float want[3];
      old_decode(&quads[i * 4], want);
      for (int c = 0; c < 3; c++) bad += bits_of(px[i * 3 + c]) != bits_of(want[c]);
    }
    CHECK(bad == 0, "%s: %zu floats of read_image differ from the old decode", name.c_str(), bad);
  }
  // truncated files: in the pixels of a flat file, in a packet of a packed one, in the header
  std::vector<uint8_t> got;
  int gw = 0, gh = 0;
  std::vector<uint8_t> cut(quads.begin(), quads.end() - 5);
  put(dir + "/cut.hdr", header_text(w, h), cut);
  CHECK(!io::read_rgbe(dir + "/cut.hdr", got, gw, gh, err) && err.find("truncated") != std::string::npos, "a cut flat file: %s", err.c_str());
  cut.assign(body.begin(), body.begin() + long(body.size() / 2));
  put(dir + "/cut2.hdr", header_text(w, h), cut);
  CHECK(!io::read_rgbe(dir + "/cut2.hdr", got, gw, gh, err) && err.find("truncated") != std::string::npos, "a cut packed file: %s", err.c_str());
  put(dir + "/cut3.hdr", "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n", {});
  CHECK(!io::read_rgbe(dir + "/cut3.hdr", got, gw, gh, err), "a cut header");
  CHECK(!io::read_rgbe(dir + "/missing.hdr", got, gw, gh, err), "a missing file");
  put(dir + "/float.pfm", "PF\n1 1\n-1.0\n", std::vector<uint8_t>(12, 0));
  CHECK(!io::read_rgbe(dir + "/float.pfm", got, gw, gh, err) && err.find("not a Radiance picture") != std::string::npos, "a PFM: %s", err.c_str());

  // the table of equal colour spaces is the decode; another pair is the decode followed by convert_colour's expression
  std::vector<float> table, curve;
  CHECK(io::rgbe_table("Linear", "Linear", table, err) && table.size() == 65536, "%s", err.c_str());
  CHECK(io::rgbe_table("sRGB", "Linear", curve, err) && curve.size() == 65536, "%s", err.c_str());
  CHECK(!io::rgbe_table("ACEScg", "Linear", curve, err), "an unknown colour space");
  io::rgbe_table("sRGB", "Linear", curve, err);
  size_t bad = 0, bad_curve = 0;
  for (uint32_t e = 0; e < 256 && table.size() == 65536 && curve.size() == 65536; e++)
    for (uint32_t m = 0; m < 256; m++) {
      const uint8_t p[4] = { uint8_t(m), 0, 0, uint8_t(e) };
      float want[3];
      old_decode(p, want);
      bad += bits_of(table[(e << 8) | m]) != bits_of(want[0]);
      float one = want[0];
      io::convert_colour(&one, 1, 1, "sRGB", "Linear", err);
      bad_curve += bits_of(curve[(e << 8) | m]) != bits_of(one);
    }
  CHECK(bad == 0 && bad_curve == 0, "rgbe_table: %zu / %zu entries differ", bad, bad_curve);

  // write_one writes the file it has always written, and write_rgbe the same file from the quads
  std::vector<float> img(size_t(w) * h * 3);
  for (size_t i = 0; i < img.size(); i++) img[i] = std::ldexp(float(rng() % 2000) - 200.0f, int(rng() % 60) - 40);
  std::vector<uint8_t> want_body(size_t(w) * h * 4);
  for (size_t i = 0; i < size_t(w) * h; i++) old_encode(img[3 * i], img[3 * i + 1], img[3 * i + 2], &want_body[4 * i]);
  io::metadata meta;
  meta.projection = "spherical"; meta.hfov = 360.0;
  CHECK(io::write_one(dir + "/out.hdr", img.data(), w, h, 3, err, &meta), "%s", err.c_str());
  CHECK(io::write_rgbe(dir + "/out2.hdr", want_body.data(), w, h, false, err, &meta), "%s", err.c_str());
  const std::string head = "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\nProjection=spherical\nHfov=360\n\n-Y 11 +X 37\n";
  std::vector<uint8_t> whole(head.begin(), head.end());
  whole.insert(whole.end(), want_body.begin(), want_body.end());
  CHECK(get(dir + "/out.hdr") == whole, "write_one: the file changed");
  CHECK(get(dir + "/out2.hdr") == whole, "write_rgbe: not write_one's file");
  CHECK(!io::write_rgbe(dir + "/out.pfm", want_body.data(), w, h, false, err), "quads into a .pfm");
}

int main(int argc, char **argv)
{
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "check" && argc == 3) {
    check_encode();
    check_decode();
    check_round_trip();
    check_files(argv[2]);
    std::printf("failures: %d\n", failures);
    return failures ? 1 : 0;
  }
  if ((mode == "encode" || mode == "decode") && argc == 4) {
    const std::vector<uint8_t> in = get(argv[2]);
    std::vector<uint8_t> out;
    if (mode == "encode") {
      const size_t n = in.size() / 12;
      out.resize(n * 4);
      for (size_t i = 0; i < n; i++) {
        float f[3];
        std::memcpy(f, &in[i * 12], 12);
        const uint32_t q = eu_rgbe_encode(f[0], f[1], f[2]);
        out[4 * i] = uint8_t(q); out[4 * i + 1] = uint8_t(q >> 8); out[4 * i + 2] = uint8_t(q >> 16); out[4 * i + 3] = uint8_t(q >> 24);
      }
    } else {
      const size_t n = in.size() / 4;
      out.resize(n * 12);
      for (size_t i = 0; i < n; i++) {
        float f[3];
        eu_rgbe_decode(io::rgbe_quad(&in[i * 4]), &f[0], &f[1], &f[2]);
        std::memcpy(&out[i * 12], f, 12);
      }
    }
    return put(argv[3], "", out) ? 0 : 1;
  }
  std::fprintf(stderr, "usage: rgbe_demo check DIR | encode IN OUT | decode IN OUT\n");
  return 2;
}
