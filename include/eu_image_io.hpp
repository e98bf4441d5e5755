// eu_image_io.hpp - image files for the stand-alone command line (tools/envutil_hip.cc).
//
// The reference reads and writes every format through OpenImageIO (read_image_data /
// save_array, envutil_basic.h:710-986), which this image does not have. What the path needs
// from a file is what those two functions hand over: interleaved float pixels, x fastest, the
// file's own channel count - and the colour space the samples are in, because the reference converts
// every image whose colour space differs from the working one (envutil_basic.h:950-977) and the output
// when the output's differs (:786-812). OpenImageIO labels a file by its format (oiio:ColorSpace):
// float formats (PFM, Radiance) are linear, 8/16-bit integer formats are display-referred. Here:
// file_colour_space() says "Linear" for .pfm / .hdr / .pic and "sRGB" for PNM / PAM, and convert_colour()
// knows the transfer pairs of OpenImageIO's built-in configuration (no OpenColorIO): sRGB <-> linear (IEC
// 61966-2-1 piecewise curve), Rec709 <-> linear (BT.709 OETF) - the alpha channel is not touched - and the
// names "Linear" / "linear" / "scene_linear" / "lin_srgb" / "lin_rec709", "sRGB" / "srgb" / "sRGB - Texture" /
// "srgb_tx", "Rec709" / "rec709". Any other name is an error message, not silence. DIFFERENCE from the
// reference, stated in INTEGRATION.md: which label OpenImageIO gives a PNM file (sRGB or Rec709, by version)
// cannot be checked here; --input_colour_space / the PTO's Csp clause override it as in the reference.
// Formats, chosen because they need no library and hold linear float or plain integer samples:
//   .pfm            Portable Float Map: "Pf" 1 channel, "PF" 3 channels, "PF4" 4 channels (the
//                   extension several tools use for RGBA); float32, either byte order, rows
//                   bottom to top
//   .pgm .ppm .pnm  binary PNM (P5 / P6), 8 or 16 bit: value / maxval
//   .pam            P7 (GRAYSCALE, GRAYSCALE_ALPHA, RGB, RGB_ALPHA), 8 or 16 bit: the integer
//                   format with an alpha channel
//   .hdr .pic       Radiance RGBE pictures (32-bit_rle_rgbe, -Y h +X w; flat or run-length encoded
//                   scanlines on input, flat on output), the usual container of lat/lon environment maps;
//                   mantissa * 2^(exponent - 136) as in the widely used rgbe.c that OpenImageIO follows
// Writing integer formats follows OpenImageIO's float -> unsigned conversion: clamp to [0, 1],
// scale by maxval, add 0.5, truncate. Cubemaps: one image of aspect 1:6, or six files named by a
// format string with one %s, filled with left, right, top, bottom, front, back (cubeface_series,
// envutil_basic.h:267-340).
//
// Integer files can also be handed on as they are: read_samples() returns the file's sample bytes and
// sample_tables() the float each sample value becomes on the way read_image() + convert_colour() take it -
// what eu_hip_source_load_samples wants, which widens and linearises on the device.
//
// The way out mirrors it: encode_steps() returns the step tables that tell which sample a float becomes on the way
// convert_colour() + write_one() take it - what eu_hip_render_samples wants - and write_samples() writes samples
// that were encoded on the device into the file write_one writes.
//
// Radiance pictures go the same two ways: read_rgbe() returns the file's quads with their scanlines expanded,
// rgbe_table() the float every (exponent, mantissa) pair becomes - what eu_hip_source_load_rgbe wants - and
// write_rgbe() writes quads that eu_hip_render_rgbe encoded. The two pixel functions are those of eu_rgbe.h, for
// read_one and write_one and for the device alike.
//
// Frames of a video: y4m_reader reads the FRAMEs of a YUV4MPEG2 stream (.y4m) forward, as the planes Y, Cb, Cr that
// eu_hip_source_load_ycbcr / eu_hip_source_reload take; ycbcr_tables() and ycbcr_matrix() are the float64 expressions
// of the Python binding's functions of the same names; frame_name() formats a name with exactly one integer
// conversion, check_frames() is what --frames FIRST LAST asks of its arguments.
//
// Header-only, host code, no dependency on the HIP library.
#ifndef EU_IMAGE_IO_HPP
#define EU_IMAGE_IO_HPP

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <vector>
#include "eu_rgbe.h"

namespace project {
namespace io {

struct header
{
  int width = 0, height = 0, nchannels = 0;
  int maxval = 0;          // 0: float samples
  bool little_endian = true;   // PFM
  bool bottom_up = false;
  bool rgbe = false;           // Radiance picture: 4-byte RGBE pixels, flat or run-length encoded scanlines
  long data_offset = 0;
  // "Projection" / "Hfov" (degrees) as envutil's save_array attaches them to its output
  // (envutil_basic.h:770-772): header lines Projection=... / Hfov=... of a Radiance picture, comment
  // lines "# Projection: ..." / "# Hfov: ..." of a PNM / PAM header; PFM has no room for them
  std::string projection;
  double hfov = -1.0;
};

struct metadata { std::string projection; double hfov = -1.0; };

inline std::string lower_ext(const std::string &name)
{
  const size_t dot = name.find_last_of('.');
  if (dot == std::string::npos) return std::string();
  std::string e = name.substr(dot + 1);
  for (auto &c : e) c = char(c >= 'A' && c <= 'Z' ? c - 'A' + 'a' : c);
  return e;
}

// next whitespace-separated token of a PNM header; '#' starts a comment up to the line's end
inline void note_metadata(const std::string &line, char sep, header &h)
{
  const size_t p = line.find(sep);
  if (p == std::string::npos) return;
  std::string key = line.substr(0, p), val = line.substr(p + 1);
  while (!key.empty() && (key[0] == ' ' || key[0] == '#')) key.erase(0, 1);
  while (!val.empty() && (val[0] == ' ')) val.erase(0, 1);
  while (!val.empty() && (val.back() == '\n' || val.back() == '\r' || val.back() == ' ')) val.pop_back();
  if (key == "Projection") h.projection = val;
  else if (key == "Hfov") { try { h.hfov = std::stod(val); } catch (...) {} }
}

inline bool token(FILE *f, std::string &t, header *meta = nullptr)
{
  t.clear();
  int c;
  for (;;) {
    c = std::fgetc(f);
    if (c == EOF) return false;
    if (c == '#') {
      std::string line;
      while ((c = std::fgetc(f)) != EOF && c != '\n') line += char(c);
      if (meta) note_metadata(line, ':', *meta);
      continue;
    }
    if (c != ' ' && c != '\t' && c != '\n' && c != '\r') break;
  }
  while (c != EOF && c != ' ' && c != '\t' && c != '\n' && c != '\r') { t += char(c); c = std::fgetc(f); }
  return true;   // exactly one whitespace character behind the token has been consumed
}

// Radiance header: "#?RADIANCE" (or "#?RGBE"), lines of NAME=value, an empty line, then "-Y h +X w"
inline bool read_rgbe_header(FILE *f, header &h, std::string &err)
{
  char line[512];
  bool format_ok = false;
  for (;;) {
    if (!std::fgets(line, sizeof line, f)) { err = "truncated Radiance header"; return false; }
    if (line[0] == '\n' || (line[0] == '\r' && line[1] == '\n')) break;
    if (!std::strncmp(line, "FORMAT=", 7)) format_ok = !std::strncmp(line + 7, "32-bit_rle_rgbe", 15);
    else note_metadata(line, '=', h);
  }
  if (!format_ok) { err = "Radiance picture without FORMAT=32-bit_rle_rgbe"; return false; }
  if (!std::fgets(line, sizeof line, f)) { err = "truncated Radiance header"; return false; }
  if (std::sscanf(line, "-Y %d +X %d", &h.height, &h.width) != 2) { err = "only the standard orientation -Y h +X w is read"; return false; }
  h.nchannels = 3; h.maxval = 0; h.rgbe = true;
  if (h.width <= 0 || h.height <= 0) { err = "unsupported image geometry"; return false; }
  h.data_offset = std::ftell(f);
  return true;
}

inline bool read_header(FILE *f, header &h, std::string &err)
{
  std::string magic, t;
  {
    const int c0 = std::fgetc(f), c1 = std::fgetc(f);
    if (c0 == '#' && c1 == '?') return read_rgbe_header(f, h, err);
    std::rewind(f);
  }
  if (!token(f, magic, &h)) { err = "empty file"; return false; }
  try {
    if (magic == "PF" || magic == "Pf" || magic == "PF4") {
      h.nchannels = magic == "Pf" ? 1 : magic == "PF" ? 3 : 4;
      if (!token(f, t, &h)) { err = "truncated header"; return false; }
      h.width = std::stoi(t);
      if (!token(f, t, &h)) { err = "truncated header"; return false; }
      h.height = std::stoi(t);
      if (!token(f, t, &h)) { err = "truncated header"; return false; }
      h.little_endian = std::stod(t) < 0.0;
      h.maxval = 0;
      h.bottom_up = true;
    } else if (magic == "P5" || magic == "P6") {
      h.nchannels = magic == "P5" ? 1 : 3;
      if (!token(f, t, &h)) { err = "truncated header"; return false; }
      h.width = std::stoi(t);
      if (!token(f, t, &h)) { err = "truncated header"; return false; }
      h.height = std::stoi(t);
      if (!token(f, t, &h)) { err = "truncated header"; return false; }
      h.maxval = std::stoi(t);
    } else if (magic == "P7") {
      for (;;) {
        if (!token(f, t, &h)) { err = "truncated header"; return false; }
        if (t == "ENDHDR") break;
        std::string v;
        if (!token(f, v, &h)) { err = "truncated header"; return false; }
        if (t == "WIDTH") h.width = std::stoi(v);
        else if (t == "HEIGHT") h.height = std::stoi(v);
        else if (t == "DEPTH") h.nchannels = std::stoi(v);
        else if (t == "MAXVAL") h.maxval = std::stoi(v);
      }
    } else {
      err = "not a PFM / PNM / PAM / Radiance file (magic '" + magic + "')";
      return false;
    }
  } catch (...) { err = "malformed header"; return false; }
  if (h.width <= 0 || h.height <= 0 || h.nchannels < 1 || h.nchannels > 4 || h.maxval < 0 || h.maxval > 65535) {
    err = "unsupported image geometry";
    return false;
  }
  // integer formats carry their MAXVAL (1 .. 65535); without one the samples would be read as raw floats
  if (magic[0] == 'P' && magic[1] >= '5' && magic[1] <= '7' && magic.size() == 2 && h.maxval < 1) {
    err = "PNM / PAM header without a MAXVAL between 1 and 65535";
    return false;
  }
  h.data_offset = std::ftell(f);
  return true;
}

inline bool probe_one(const std::string &name, header &h, std::string &err)
{
  FILE *f = std::fopen(name.c_str(), "rb");
  if (!f) { err = "cannot open " + name; return false; }
  const bool ok = read_header(f, h, err);
  std::fclose(f);
  if (!ok) err = name + ": " + err;
  return ok;
}

// cubeface_series (envutil_basic.h:267-340): six names from a format string with ONE percent sign
inline bool cubeface_names(const std::string &fmt, std::vector<std::string> &names)
{
  size_t count = 0;
  for (char c : fmt) count += c == '%';
  const size_t p = fmt.find("%s");
  if (count != 1 || p == std::string::npos) return false;
  static const char *const face[6] = { "left", "right", "top", "bottom", "front", "back" };
  names.clear();
  for (int i = 0; i < 6; i++) names.push_back(fmt.substr(0, p) + face[i] + fmt.substr(p + 2));
  return true;
}

inline bool probe_y4m(const std::string &name, int &width, int &height, int &nchannels, std::string &err);   // below

// facet_base::get_image_metrics (envutil_basic.h:546-589): a name with a percent sign is a set
// of six cube faces and reports the metrics of the first
inline bool probe(const std::string &name, int &width, int &height, int &nchannels, std::string &err,
                  metadata *meta = nullptr)
{
  if (lower_ext(name) == "y4m") return probe_y4m(name, width, height, nchannels, err);
  header h;
  std::vector<std::string> faces;
  const bool series = name.find('%') != std::string::npos;
  if (series && !cubeface_names(name, faces)) { err = "a format string needs exactly one %s: " + name; return false; }
  if (!probe_one(series ? faces[0] : name, h, err)) return false;
  width = h.width; height = h.height; nchannels = h.nchannels;
  if (meta) { meta->projection = h.projection; meta->hfov = h.hfov; }
  return true;
}

// one scanline of a Radiance picture, flat or run-length encoded, as width quads R G B E
inline bool read_rgbe_scanline(FILE *f, int width, uint8_t *sl)
{
  uint8_t b4[4];
  if (std::fread(b4, 1, 4, f) != 4) return false;
  if (b4[0] == 2 && b4[1] == 2 && !(b4[2] & 0x80) && ((int(b4[2]) << 8) | b4[3]) == width && width >= 8 && width < 32768) {
    // new run-length encoding: the four components one after the other
    for (int c = 0; c < 4; c++) {
      int x = 0;
      while (x < width) {
        int n = std::fgetc(f);
        if (n == EOF) return false;
        if (n > 128) {
          n -= 128;
          const int v = std::fgetc(f);
          if (v == EOF || x + n > width) return false;
          for (int i = 0; i < n; i++) sl[size_t(x++) * 4 + c] = uint8_t(v);
        } else {
          if (n == 0 || x + n > width) return false;
          for (int i = 0; i < n; i++) {
            const int v = std::fgetc(f);
            if (v == EOF) return false;
            sl[size_t(x++) * 4 + c] = uint8_t(v);
          }
        }
      }
    }
    return true;
  }
  // flat scanline (the first pixel is already read)
  std::memcpy(sl, b4, 4);
  const size_t rest = size_t(width) * 4 - 4;
  return std::fread(sl + 4, 1, rest, f) == rest;
}

// the four bytes of a quad as eu_rgbe.h takes them, whatever the host's byte order
inline uint32_t rgbe_quad(const uint8_t *p) { return uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24); }

// rows top to bottom, interleaved, the file's own channel count
inline bool read_one(const std::string &name, header &h, float *dst, std::string &err)
{
  FILE *f = std::fopen(name.c_str(), "rb");
  if (!f) { err = "cannot open " + name; return false; }
  header g;
  if (!read_header(f, g, err)) { std::fclose(f); err = name + ": " + err; return false; }
  if (h.width && (g.width != h.width || g.height != h.height || g.nchannels != h.nchannels)) {
    std::fclose(f);
    err = name + ": size differs from the first image of the set";
    return false;
  }
  h = g;
  const size_t row = size_t(h.width) * h.nchannels;
  bool ok = true;
  if (h.rgbe) {
    std::vector<uint8_t> sl(size_t(h.width) * 4);
    for (int y = 0; y < h.height && ok; y++) {
      ok = read_rgbe_scanline(f, h.width, sl.data());
      if (!ok) break;
      float *d = dst + size_t(y) * row;
      for (int x = 0; x < h.width; x++) eu_rgbe_decode(rgbe_quad(sl.data() + size_t(x) * 4), d + 3 * x, d + 3 * x + 1, d + 3 * x + 2);
    }
  } else if (h.maxval == 0) {
    const uint16_t one = 1;
    const bool host_little = *reinterpret_cast<const uint8_t *>(&one) == 1;
    for (int y = 0; y < h.height && ok; y++) {
      float *d = dst + size_t(h.bottom_up ? h.height - 1 - y : y) * row;
      ok = std::fread(d, 4, row, f) == row;
      if (ok && host_little != h.little_endian)
        for (size_t i = 0; i < row; i++) {
          uint32_t u;
          std::memcpy(&u, d + i, 4);
          u = (u >> 24) | ((u >> 8) & 0xff00u) | ((u << 8) & 0xff0000u) | (u << 24);
          std::memcpy(d + i, &u, 4);
        }
    }
  } else {
    const int bytes = h.maxval > 255 ? 2 : 1;
    std::vector<uint8_t> buf(row * bytes);
    const float mv = float(h.maxval);
    for (int y = 0; y < h.height && ok; y++) {
      ok = std::fread(buf.data(), 1, buf.size(), f) == buf.size();
      float *d = dst + size_t(y) * row;
      if (bytes == 1) for (size_t i = 0; i < row; i++) d[i] = float(buf[i]) / mv;
      else for (size_t i = 0; i < row; i++) d[i] = float((unsigned(buf[2 * i]) << 8) | buf[2 * i + 1]) / mv;   // big endian
    }
  }
  std::fclose(f);
  if (!ok) err = name + ": truncated pixel data";
  return ok;
}

// a facet's pixels: a single image, or six cube faces stacked to the 1:6 image
// ---- colour spaces (envutil_basic.h:786-812, :950-977; OpenImageIO's built-in ColorConfig) -----------------
enum colour_class { CSP_UNKNOWN = 0, CSP_LINEAR = 1, CSP_SRGB = 2, CSP_REC709 = 3 };
inline colour_class classify_colour_space(const std::string &name)
{
  std::string n;
  for (char c : name) n += char(c >= 'A' && c <= 'Z' ? c - 'A' + 'a' : c);
  if (n == "linear" || n == "scene_linear" || n == "lin_srgb" || n == "lin_rec709" || n == "linear rec.709 (srgb)") return CSP_LINEAR;
  if (n == "srgb" || n == "srgb - texture" || n == "srgb_tx" || n == "srgb_texture" || n == "srgb encoded rec.709 (srgb)") return CSP_SRGB;
  if (n == "rec709" || n == "rec.709") return CSP_REC709;
  return CSP_UNKNOWN;
}
// what the format says about its samples (OpenImageIO: oiio:ColorSpace)
inline std::string file_colour_space(const std::string &name)
{
  const std::string e = lower_ext(name);
  return (e == "pfm" || e == "hdr" || e == "pic") ? "Linear" : "sRGB";
}
inline float to_linear(colour_class c, float v)
{
  if (c == CSP_SRGB) return v <= 0.04045f ? v / 12.92f : std::pow((v + 0.055f) / 1.055f, 2.4f);
  if (c == CSP_REC709) return v < 0.081f ? v / 4.5f : std::pow((v + 0.099f) / 1.099f, 1.0f / 0.45f);
  return v;
}
inline float from_linear(colour_class c, float v)
{
  if (c == CSP_SRGB) return v <= 0.0031308f ? 12.92f * v : 1.055f * std::pow(v, 1.0f / 2.4f) - 0.055f;
  if (c == CSP_REC709) return v < 0.018f ? 4.5f * v : 1.099f * std::pow(v, 0.45f) - 0.099f;
  return v;
}
// the classes of a conversion `from` -> `to`; *same: nothing to do (equal names, equal classes). False with a
// message for a name this table does not know.
inline bool colour_pair(const std::string &from, const std::string &to, colour_class &a, colour_class &b, bool &same, std::string &err)
{
  a = b = CSP_UNKNOWN;
  same = true;
  if (from == to) return true;
  a = classify_colour_space(from); b = classify_colour_space(to);
  if (a == CSP_UNKNOWN || b == CSP_UNKNOWN) {
    err = "colour space '" + (a == CSP_UNKNOWN ? from : to) + "' is not known here (known: Linear / scene_linear / lin_srgb, sRGB, Rec709; OpenColorIO configurations are not read)";
    return false;
  }
  same = a == b;
  return true;
}
// one colour sample from class a to class b: the ONE statement of the curve, for convert_colour and sample_tables
inline float convert_sample(colour_class a, colour_class b, float v) { return from_linear(b, to_linear(a, v)); }
// npix pixels of nch interleaved channels from colour space `from` to `to`, in place; the alpha channel (the
// last of 2 or 4) stays. False with a message for a name this table does not know.
inline bool convert_colour(float *px, size_t npix, int nch, const std::string &from, const std::string &to, std::string &err)
{
  colour_class a, b;
  bool same;
  if (!colour_pair(from, to, a, b, same, err)) return false;
  if (same) return true;
  const int ncol = (nch == 2 || nch == 4) ? nch - 1 : nch;
  for (size_t i = 0; i < npix; i++)
    for (int c = 0; c < ncol; c++) {
      float &v = px[i * size_t(nch) + c];
      v = convert_sample(a, b, v);
    }
  return true;
}

// The floats the samples of an integer image become, as tables over EVERY value of `bits` bits (8 or 16; values
// above maxval included - a file may hold them): alpha[v] is read_one's float(v) / float(maxval), colour[v] what
// convert_colour makes of that float on the way from `from` to `to`. A sample's float depends on its value alone,
// so a look-up in these tables gives the bits of read_image + convert_colour (eu_hip_source_load_samples).
inline bool sample_tables(int bits, int maxval, const std::string &from, const std::string &to, std::vector<float> &colour,
                          std::vector<float> &alpha, std::string &err)
{
  if ((bits != 8 && bits != 16) || maxval < 1 || maxval >= (1 << bits)) { err = "sample tables: 8 or 16 bits, maxval within them"; return false; }
  colour_class a, b;
  bool same;
  if (!colour_pair(from, to, a, b, same, err)) return false;
  const size_t n = size_t(1) << bits;
  const float mv = float(maxval);
  colour.resize(n); alpha.resize(n);
  for (size_t v = 0; v < n; v++) {
    alpha[v] = float(v) / mv;
    colour[v] = same ? alpha[v] : convert_sample(a, b, alpha[v]);
  }
  return true;
}

// The code a float becomes in an integer file (OpenImageIO's float -> unsigned conversion): clamp to [0, 1], scale
// by maxval, add 0.5, truncate; NaN fails both tests of the clamp and is written as 0. The ONE statement of the
// quantiser, for write_one and encode_steps.
inline unsigned quantise_sample(float v, int maxval)
{
  v = v < 0.0f ? 0.0f : v > 1.0f ? 1.0f : v;
  return v == v ? unsigned(v * float(maxval) + 0.5f) : 0u;
}

// float bit patterns in the order of their values: key(-inf) < ... < key(-0) < key(+0) < ... < key(+inf)
inline uint32_t float_key(float v)
{
  uint32_t u;
  std::memcpy(&u, &v, 4);
  return u & 0x80000000u ? ~u : u | 0x80000000u;
}
inline float key_float(uint32_t k)
{
  const uint32_t u = k & 0x80000000u ? k & 0x7fffffffu : ~k;
  float v;
  std::memcpy(&v, &u, 4);
  return v;
}

// The way out as tables, the mirror of sample_tables: the code Q(v) that convert_colour (`from` -> `to`) followed by
// write_one's quantiser gives a float is a non-decreasing step function of v, so it is told by its steps - steps[k]
// is the smallest float with Q >= k, found by bisection over the float keys from -inf to +inf with the very
// expressions the float route applies (convert_sample, quantise_sample); steps[0] = -inf, and every k > maxval is NaN
// (eu_hip.h: eu_encode). Q(v) is then the number of k >= 1 with v >= steps[k], which is all eu_hip_encode_samples
// evaluates. alpha: the same without a curve.
// Each branch of a transfer curve is monotone if powf is; where two branches meet the code may DROP (to_linear of
// Rec709 falls from 0.018 to about 0.01794 at 0.081: four codes at maxval 65535, none at 255), and no table can
// tell such a function. So the builder evaluates Q on the floats either side of every joint - 0.04045f, 0.081f and
// the smallest v whose to_linear reaches 0.0031308f / 0.018f - and returns false, with a message naming the pair of
// floats, if the code drops there: the caller then keeps the float route. The tables are filled in either case.
inline bool encode_steps(int bits, int maxval, const std::string &from, const std::string &to, std::vector<float> &colour,
                         std::vector<float> &alpha, std::string &err)
{
  if ((bits != 8 && bits != 16) || maxval < 1 || maxval >= (1 << bits)) { err = "encode steps: 8 or 16 bits, maxval within them"; return false; }
  colour_class a, b;
  bool same;
  if (!colour_pair(from, to, a, b, same, err)) return false;
  const size_t n = size_t(1) << bits;
  const float nan = std::nanf("");
  const uint32_t lo_key = float_key(-HUGE_VALF), hi_key = float_key(HUGE_VALF);
  auto q_colour = [&](float v) { return quantise_sample(same ? v : convert_sample(a, b, v), maxval); };
  auto q_alpha = [&](float v) { return quantise_sample(v, maxval); };
  auto build = [&](std::vector<float> &steps, auto q) {
    steps.assign(n, nan);
    steps[0] = -HUGE_VALF;
    uint32_t lo = lo_key;
    for (unsigned k = 1; k <= unsigned(maxval); k++) {
      // the smallest key in [lo, hi] whose code is >= k; it is not below the step before it
      uint32_t l = lo, h = hi_key;
      if (q(key_float(h)) < k) return false;
      while (l < h) {
        const uint32_t m = l + (h - l) / 2;
        if (q(key_float(m)) >= k) h = m; else l = m + 1;
      }
      steps[k] = key_float(l);
      lo = l;
    }
    return true;
  };
  if (!build(colour, q_colour) || !build(alpha, q_alpha)) { err = "encode steps: " + from + " -> " + to + " does not reach code " + std::to_string(maxval); return false; }
  if (same) return true;
  // the joints: of `from`'s curve in v, of `to`'s curve where to_linear(from, v) reaches its threshold
  std::vector<float> joints;
  if (a == CSP_SRGB) joints.push_back(0.04045f);
  if (a == CSP_REC709) joints.push_back(0.081f);
  if (b == CSP_SRGB || b == CSP_REC709) {
    const float reach = b == CSP_SRGB ? 0.0031308f : 0.018f;
    uint32_t l = float_key(0.0f), h = float_key(1.0f);
    while (l < h) {
      const uint32_t m = l + (h - l) / 2;
      if (to_linear(a, key_float(m)) >= reach) h = m; else l = m + 1;
    }
    joints.push_back(key_float(l));
  }
  for (float j : joints) {
    const uint32_t kj = float_key(j);
    for (uint32_t k = kj - 4; k < kj + 4; k++) {
      const float v0 = key_float(k), v1 = key_float(k + 1);
      const unsigned c0 = q_colour(v0), c1 = q_colour(v1);
      if (c1 < c0) {
        char msg[256];
        std::snprintf(msg, sizeof msg, "encode steps: %s -> %s at maxval %d is no step function: %.9g has code %u, %.9g code %u",
                      from.c_str(), to.c_str(), maxval, double(v0), c0, double(v1), c1);
        err = msg;
        return false;
      }
    }
  }
  return true;
}

inline bool read_image(const std::string &name, std::vector<float> &pixels, int &width, int &height,
                       int &nchannels, std::string &err)
{
  std::vector<std::string> faces;
  if (name.find('%') != std::string::npos) {
    if (!cubeface_names(name, faces)) { err = "a format string needs exactly one %s: " + name; return false; }
  } else faces.push_back(name);
  header h;
  if (!probe_one(faces[0], h, err)) return false;
  const size_t per = size_t(h.width) * h.height * h.nchannels;
  try { pixels.resize(per * faces.size()); }
  catch (const std::exception &) { err = name + ": not enough host memory for " + std::to_string(h.width) + " x " + std::to_string(h.height) + " pixels"; return false; }
  for (size_t i = 0; i < faces.size(); i++)
    if (!read_one(faces[i], h, pixels.data() + i * per, err)) return false;
  width = h.width; height = h.height * int(faces.size()); nchannels = h.nchannels;
  return true;
}

// the raw samples of a PNM / PAM file: `bytes` per sample, big endian as stored; the header checks and messages
// are read_one's
inline bool read_samples_one(const std::string &name, header &h, uint8_t *dst, std::string &err)
{
  FILE *f = std::fopen(name.c_str(), "rb");
  if (!f) { err = "cannot open " + name; return false; }
  header g;
  if (!read_header(f, g, err)) { std::fclose(f); err = name + ": " + err; return false; }
  if (h.width && (g.width != h.width || g.height != h.height || g.nchannels != h.nchannels)) {
    std::fclose(f);
    err = name + ": size differs from the first image of the set";
    return false;
  }
  // (one pair of tables serves the whole set)
  if (h.width && g.maxval != h.maxval) { std::fclose(f); err = name + ": MAXVAL differs from the first image of the set"; return false; }
  if (g.maxval == 0) { std::fclose(f); err = name + ": not an integer format"; return false; }
  h = g;
  const size_t n = size_t(h.width) * h.height * h.nchannels * (h.maxval > 255 ? 2 : 1);
  const bool ok = std::fread(dst, 1, n, f) == n;
  std::fclose(f);
  if (!ok) err = name + ": truncated pixel data";
  return ok;
}

// read_image for the integer formats, without the step to float: the file's sample bytes (16 bit: big endian, as
// PNM / PAM store them), rows top to bottom, six cube faces stacked. `bits` is 8 for maxval <= 255, else 16.
// .pfm / .hdr / .pic: false, "not an integer format".
inline bool read_samples(const std::string &name, std::vector<uint8_t> &samples, int &width, int &height, int &nchannels,
                         int &maxval, int &bits, std::string &err)
{
  std::vector<std::string> faces;
  if (name.find('%') != std::string::npos) {
    if (!cubeface_names(name, faces)) { err = "a format string needs exactly one %s: " + name; return false; }
  } else faces.push_back(name);
  header h;
  if (!probe_one(faces[0], h, err)) return false;
  if (h.maxval == 0) { err = faces[0] + ": not an integer format"; return false; }
  const size_t per = size_t(h.width) * h.height * h.nchannels * (h.maxval > 255 ? 2 : 1);
  try { samples.resize(per * faces.size()); }
  catch (const std::exception &) { err = name + ": not enough host memory for " + std::to_string(h.width) + " x " + std::to_string(h.height) + " pixels"; return false; }
  for (size_t i = 0; i < faces.size(); i++)
    if (!read_samples_one(faces[i], h, samples.data() + i * per, err)) return false;
  width = h.width; height = h.height * int(faces.size()); nchannels = h.nchannels;
  maxval = h.maxval; bits = h.maxval > 255 ? 8 * 2 : 8;
  return true;
}

// the header of a PNM (P5 / P6) or PAM (P7) file, the metadata as comment lines: for write_one and write_samples
inline void write_pnm_header(FILE *f, bool pam, int width, int height, int nch, int maxval, const metadata *meta)
{
  if (pam) {
    static const char *const tt[5] = { "", "GRAYSCALE", "GRAYSCALE_ALPHA", "RGB", "RGB_ALPHA" };
    std::fprintf(f, "P7\n");
    if (meta && !meta->projection.empty()) std::fprintf(f, "# Projection: %s\n# Hfov: %.9g\n", meta->projection.c_str(), meta->hfov);
    std::fprintf(f, "WIDTH %d\nHEIGHT %d\nDEPTH %d\nMAXVAL %d\nTUPLTYPE %s\nENDHDR\n", width, height, nch, maxval, tt[nch]);
  } else {
    std::fprintf(f, "%s\n", nch == 1 ? "P5" : "P6");
    if (meta && !meta->projection.empty()) std::fprintf(f, "# Projection: %s\n# Hfov: %.9g\n", meta->projection.c_str(), meta->hfov);
    std::fprintf(f, "%d %d\n%d\n", width, height, maxval);
  }
}

// What write_one makes of a PNM / PAM name, as (bits, maxval): .pgm / .ppm / .pnm hold 8-bit samples, .pam 16-bit
// ones, big endian. False for every other name - those files take floats.
inline bool sample_format(const std::string &name, int &bits, int &maxval)
{
  const std::string ext = lower_ext(name);
  if (ext == "pam") { bits = 16; maxval = 65535; return true; }
  if (ext == "pgm" || ext == "ppm" || ext == "pnm") { bits = 8; maxval = 255; return true; }
  return false;
}

// the header of a Radiance picture with flat scanlines, the metadata as header lines: for write_one and write_rgbe
inline void write_rgbe_header(FILE *f, int width, int height, const metadata *meta)
{
  std::fprintf(f, "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n");
  if (meta && !meta->projection.empty()) std::fprintf(f, "Projection=%s\nHfov=%.9g\n", meta->projection.c_str(), meta->hfov);
  std::fprintf(f, "\n-Y %d +X %d\n", height, width);
}

inline bool write_one(const std::string &name, const float *src, int width, int height, int nch, std::string &err,
                      const metadata *meta = nullptr)
{
  const std::string ext = lower_ext(name);
  FILE *f = std::fopen(name.c_str(), "wb");
  if (!f) { err = "cannot create " + name; return false; }
  const size_t row = size_t(width) * nch;
  bool ok = true;
  if (ext == "pfm") {
    if (nch == 2) { std::fclose(f); err = name + ": PFM holds 1, 3 or 4 channels; use .pam for 2"; return false; }
    const uint16_t one = 1;
    const bool host_little = *reinterpret_cast<const uint8_t *>(&one) == 1;
    std::fprintf(f, "%s\n%d %d\n%s\n", nch == 1 ? "Pf" : nch == 3 ? "PF" : "PF4", width, height, host_little ? "-1.0" : "1.0");
    for (int y = height - 1; y >= 0 && ok; y--) ok = std::fwrite(src + size_t(y) * row, 4, row, f) == row;
  } else if (ext == "hdr" || ext == "pic") {
    if (nch != 3) { std::fclose(f); err = name + ": a Radiance picture holds 3 channels"; return false; }
    write_rgbe_header(f, width, height, meta);
    std::vector<uint8_t> sl(size_t(width) * 4);
    for (int y = 0; y < height && ok; y++) {
      const float *sp = src + size_t(y) * row;
      for (int x = 0; x < width; x++) {
        const uint32_t q = eu_rgbe_encode(sp[3 * x], sp[3 * x + 1], sp[3 * x + 2]);
        uint8_t *p = sl.data() + size_t(x) * 4;
        p[0] = uint8_t(q); p[1] = uint8_t(q >> 8); p[2] = uint8_t(q >> 16); p[3] = uint8_t(q >> 24);
      }
      ok = std::fwrite(sl.data(), 1, sl.size(), f) == sl.size();
    }
  } else if (ext == "pgm" || ext == "ppm" || ext == "pnm" || ext == "pam") {
    const bool pam = ext == "pam";
    if (!pam && nch != 1 && nch != 3) { std::fclose(f); err = name + ": PNM holds 1 or 3 channels; use .pam or .pfm"; return false; }
    const int maxval = pam ? 65535 : 255;
    write_pnm_header(f, pam, width, height, nch, maxval, meta);
    std::vector<uint8_t> buf(row * (pam ? 2 : 1));
    for (int y = 0; y < height && ok; y++) {
      const float *s = src + size_t(y) * row;
      for (size_t i = 0; i < row; i++) {
        const unsigned q = quantise_sample(s[i], maxval);
        if (pam) { buf[2 * i] = uint8_t(q >> 8); buf[2 * i + 1] = uint8_t(q & 255u); }
        else buf[i] = uint8_t(q);
      }
      ok = std::fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    }
  } else {
    std::fclose(f);
    err = name + ": output formats are .pfm, .hdr, .pgm, .ppm, .pnm, .pam";
    return false;
  }
  ok = std::fclose(f) == 0 && ok;
  if (!ok) err = name + ": write failed";
  return ok;
}

// save_array (envutil_basic.h:710-815): a cubemap target whose output name is a format string
// goes to six face images, everything else to one file
inline bool write_image(const std::string &name, const float *src, int width, int height, int nch,
                        bool cubemap, std::string &err, const metadata *meta = nullptr)
{
  std::vector<std::string> faces;
  if (cubemap && name.find('%') != std::string::npos && cubeface_names(name, faces)) {
    if (height != 6 * width) { err = "a cubemap is 1:6"; return false; }
    // save_array writes the six faces as rectilinear images (envutil_basic.h:741-757)
    metadata face_meta;
    if (meta) { face_meta.projection = "rectilinear"; face_meta.hfov = meta->hfov; }
    for (int i = 0; i < 6; i++)
      if (!write_one(faces[size_t(i)], src + size_t(i) * width * width * nch, width, width, nch, err, meta ? &face_meta : nullptr)) return false;
    return true;
  }
  return write_one(name, src, width, height, nch, err, meta);
}

// write_one for samples that are already encoded (eu_hip_render_samples): `src` holds width * nch samples per row
// in the file's own form - bytes for PNM, big-endian shorts for PAM (sample_format) - and the file is, header and
// metadata included, the one write_one writes from the floats those samples were made of.
inline bool write_samples_one(const std::string &name, const uint8_t *src, int width, int height, int nch, std::string &err,
                              const metadata *meta = nullptr)
{
  int bits = 0, maxval = 0;
  if (!sample_format(name, bits, maxval)) { err = name + ": samples go to .pgm, .ppm, .pnm or .pam"; return false; }
  const bool pam = bits == 16;
  if (!pam && nch != 1 && nch != 3) { err = name + ": PNM holds 1 or 3 channels; use .pam or .pfm"; return false; }
  FILE *f = std::fopen(name.c_str(), "wb");
  if (!f) { err = "cannot create " + name; return false; }
  write_pnm_header(f, pam, width, height, nch, maxval, meta);
  const size_t n = size_t(width) * height * nch * size_t(bits / 8);
  bool ok = std::fwrite(src, 1, n, f) == n;
  ok = std::fclose(f) == 0 && ok;
  if (!ok) err = name + ": write failed";
  return ok;
}

// write_image for samples: six face files for a cubemap target and a format string, else one file
inline bool write_samples(const std::string &name, const uint8_t *src, int width, int height, int nch,
                          bool cubemap, std::string &err, const metadata *meta = nullptr)
{
  std::vector<std::string> faces;
  if (cubemap && name.find('%') != std::string::npos && cubeface_names(name, faces)) {
    if (height != 6 * width) { err = "a cubemap is 1:6"; return false; }
    int bits = 0, maxval = 0;
    if (!sample_format(name, bits, maxval)) { err = name + ": samples go to .pgm, .ppm, .pnm or .pam"; return false; }
    metadata face_meta;
    if (meta) { face_meta.projection = "rectilinear"; face_meta.hfov = meta->hfov; }
    for (int i = 0; i < 6; i++)
      if (!write_samples_one(faces[size_t(i)], src + size_t(i) * width * width * nch * size_t(bits / 8), width, width, nch, err,
                             meta ? &face_meta : nullptr)) return false;
    return true;
  }
  return write_samples_one(name, src, width, height, nch, err, meta);
}

// ---- Radiance pictures handed on as they are (eu_hip_source_load_rgbe, eu_hip_render_rgbe) -----------------------

// read_image for .hdr / .pic without the step to float: the file's quads R G B E, rows top to bottom, scanlines
// expanded as read_one expands them, six cube faces stacked. Every other format: false, "not a Radiance picture".
inline bool read_rgbe(const std::string &name, std::vector<uint8_t> &quads, int &width, int &height, std::string &err)
{
  std::vector<std::string> faces;
  if (name.find('%') != std::string::npos) {
    if (!cubeface_names(name, faces)) { err = "a format string needs exactly one %s: " + name; return false; }
  } else faces.push_back(name);
  header h;
  if (!probe_one(faces[0], h, err)) return false;
  if (!h.rgbe) { err = faces[0] + ": not a Radiance picture"; return false; }
  const size_t per = size_t(h.width) * h.height * 4;
  try { quads.resize(per * faces.size()); }
  catch (const std::exception &) { err = name + ": not enough host memory for " + std::to_string(h.width) + " x " + std::to_string(h.height) + " pixels"; return false; }
  for (size_t i = 0; i < faces.size(); i++) {
    FILE *f = std::fopen(faces[i].c_str(), "rb");
    if (!f) { err = "cannot open " + faces[i]; return false; }
    header g;
    if (!read_header(f, g, err)) { std::fclose(f); err = faces[i] + ": " + err; return false; }
    if (!g.rgbe || g.width != h.width || g.height != h.height) {
      std::fclose(f);
      err = faces[i] + ": size differs from the first image of the set";
      return false;
    }
    bool ok = true;
    for (int y = 0; y < h.height && ok; y++) ok = read_rgbe_scanline(f, h.width, quads.data() + i * per + size_t(y) * h.width * 4);
    std::fclose(f);
    if (!ok) { err = faces[i] + ": truncated pixel data"; return false; }
  }
  width = h.width; height = h.height * int(faces.size());
  return true;
}

// The float a channel of a quad becomes, as a table over EVERY (E, mantissa) pair, indexed (E << 8) | mantissa:
// read_one's decode followed by what convert_colour makes of that float on the way from `from` to `to`. A channel's
// float depends on its pair alone, so a look-up gives the bits of read_image + convert_colour.
inline bool rgbe_table(const std::string &from, const std::string &to, std::vector<float> &table, std::string &err)
{
  colour_class a, b;
  bool same;
  if (!colour_pair(from, to, a, b, same, err)) return false;
  table.resize(65536);
  for (uint32_t e = 0; e < 256; e++)
    for (uint32_t m = 0; m < 256; m++) {
      float v, g, bl;
      eu_rgbe_decode(m | (e << 24), &v, &g, &bl);
      table[(e << 8) | m] = same ? v : convert_sample(a, b, v);
    }
  return true;
}

// write_one for pixels that are already encoded (eu_hip_render_rgbe): `src` holds width quads per row, and the file
// is, header and metadata included, the one write_one writes from the floats those quads were made of.
inline bool write_rgbe_one(const std::string &name, const uint8_t *src, int width, int height, std::string &err,
                           const metadata *meta = nullptr)
{
  const std::string ext = lower_ext(name);
  if (ext != "hdr" && ext != "pic") { err = name + ": quads go to .hdr or .pic"; return false; }
  FILE *f = std::fopen(name.c_str(), "wb");
  if (!f) { err = "cannot create " + name; return false; }
  write_rgbe_header(f, width, height, meta);
  const size_t n = size_t(width) * height * 4;
  bool ok = std::fwrite(src, 1, n, f) == n;
  ok = std::fclose(f) == 0 && ok;
  if (!ok) err = name + ": write failed";
  return ok;
}

// write_image for quads: six face files for a cubemap target and a format string, else one file
inline bool write_rgbe(const std::string &name, const uint8_t *src, int width, int height, bool cubemap, std::string &err,
                       const metadata *meta = nullptr)
{
  std::vector<std::string> faces;
  if (cubemap && name.find('%') != std::string::npos && cubeface_names(name, faces)) {
    if (height != 6 * width) { err = "a cubemap is 1:6"; return false; }
    metadata face_meta;
    if (meta) { face_meta.projection = "rectilinear"; face_meta.hfov = meta->hfov; }
    for (int i = 0; i < 6; i++)
      if (!write_rgbe_one(faces[size_t(i)], src + size_t(i) * width * width * 4, width, width, err, meta ? &face_meta : nullptr)) return false;
    return true;
  }
  return write_rgbe_one(name, src, width, height, err, meta);
}

// ---- frame sequences: numbered names and YUV4MPEG2 streams ---------------------------------------------------------

// the conversions of a name: `ints` counts %[flags][width]d (or i, u), `others` every other '%'
inline void count_conversions(const std::string &fmt, int &ints, int &others)
{
  ints = others = 0;
  for (size_t i = 0; i < fmt.size(); i++) {
    if (fmt[i] != '%') continue;
    size_t k = i + 1;
    while (k < fmt.size() && (fmt[k] == '0' || fmt[k] == '-' || fmt[k] == '+' || fmt[k] == ' ')) k++;
    while (k < fmt.size() && fmt[k] >= '0' && fmt[k] <= '9') k++;
    if (k < fmt.size() && std::strchr("diu", fmt[k]) && k - i <= 8) { ints++; i = k; }
    else others++;
  }
}

// the name of frame k: fmt holds exactly one integer conversion (%d, %04d, ...) and no other '%'
inline bool frame_name(const std::string &fmt, int k, std::string &out, std::string &err)
{
  int ints = 0, others = 0;
  count_conversions(fmt, ints, others);
  if (ints != 1 || others != 0) {
    err = "'" + fmt + "' holds " + (ints == 0 && others == 0 ? std::string("no conversion") : std::to_string(ints + others) + " conversions, " + std::to_string(ints) + " of them for an integer") +
          ": the name of a frame sequence holds exactly one integer conversion (%d, %04d, ...)";
    return false;
  }
  std::vector<char> buf(fmt.size() + 32);
  std::snprintf(buf.data(), buf.size(), fmt.c_str(), k);
  out = buf.data();
  return true;
}

// a whole non-negative decimal number
inline bool frame_number(const std::string &s, int &v)
{
  if (s.empty() || s.size() > 9) return false;
  v = 0;
  for (char c : s) { if (c < '0' || c > '9') return false; v = v * 10 + (c - '0'); }
  return true;
}

// --frames FIRST LAST on the single facet's image `image` with the output `output`: both numbers at least 0 and
// FIRST <= LAST; the image a .y4m stream or a name with one integer conversion (not the six-file cubemap name, %s);
// the output a name with one integer conversion, or a .y4m stream
inline bool check_frames(const std::string &first_s, const std::string &last_s, const std::string &image,
                         const std::string &output, int &first, int &last, std::string &err)
{
  if (!frame_number(first_s, first) || !frame_number(last_s, last)) {
    err = "--frames FIRST LAST: two whole numbers, both at least 0 ('" + first_s + "', '" + last_s + "')";
    return false;
  }
  if (first > last) { err = "--frames " + first_s + " " + last_s + ": FIRST is beyond LAST"; return false; }
  std::string name;
  if (lower_ext(image) != "y4m") {
    if (image.find("%s") != std::string::npos) { err = "--frames: '" + image + "' names the six files of a cubemap (%s): a frame sequence is one file per frame"; return false; }
    if (!frame_name(image, first, name, err)) { err = "--frames: the facet's image " + err; return false; }
  }
  // (a .y4m output is one stream that holds all frames: its name needs no conversion)
  if (lower_ext(output) != "y4m" && !frame_name(output, first, name, err)) { err = "--frames: --output " + err; return false; }
  return true;
}

// What a YUV4MPEG2 header says of its frames. Colour tags: C420, C420jpeg, C420mpeg2, C420paldv (4:2:0; the tags differ
// in chroma siting, which replication does not read), C422, C444 - 8 bit - and C420p10 / p12 / p16, C422p10 / ..,
// C444p10 / ..: 16-bit little-endian words with the code in the low bits. No tag: C420jpeg, as the format's tools
// assume. Cmono, the alpha variants and everything else are refused. XCOLORRANGE=FULL: full range.
struct y4m_info
{
  int width = 0, height = 0;
  int sub_x = 2, sub_y = 2;
  int bits = 8, depth = 8;         // bits of a stored sample (8 or 16), significant bits
  bool full_range = false;
  size_t y_bytes = 0, c_bytes = 0; // of the luma plane, of ONE chroma plane
  size_t frame_bytes() const { return y_bytes + 2 * c_bytes; }
};

inline bool y4m_colour_tag(const std::string &tag, y4m_info &info, std::string &err)
{
  std::string base = tag;
  int depth = 8;
  const size_t p = tag.rfind('p');
  if (p != std::string::npos && p > 0 && (tag.substr(p) == "p10" || tag.substr(p) == "p12" || tag.substr(p) == "p16")) {
    base = tag.substr(0, p);
    depth = std::atoi(tag.c_str() + p + 1);
    if (base != "420" && base != "422" && base != "444") base = "?";     // C420jpegp10 and the like do not exist
  }
  if (base == "420" || (depth == 8 && (base == "420jpeg" || base == "420mpeg2" || base == "420paldv"))) { info.sub_x = 2; info.sub_y = 2; }
  else if (base == "422") { info.sub_x = 2; info.sub_y = 1; }
  else if (base == "444") { info.sub_x = 1; info.sub_y = 1; }
  else {
    err = "colour tag C" + tag + ": C420, C420jpeg, C420mpeg2, C420paldv, C422, C444 and the p10, p12, p16 forms of C420, C422, C444 are read" +
          (tag.compare(0, 4, "mono") == 0 ? " (no chroma planes)" : tag.find("alpha") != std::string::npos ? " (no alpha plane)" : "");
    return false;
  }
  info.depth = depth;
  info.bits = depth == 8 ? 8 : 16;
  return true;
}

// the stream header, one line without its newline: "YUV4MPEG2 W.. H.. [F.. I.. A..] [C..] [X..]"
inline bool y4m_parse_header(const std::string &line, y4m_info &info, std::string &err)
{
  info = y4m_info();
  if (line.compare(0, 9, "YUV4MPEG2") != 0 || (line.size() > 9 && line[9] != ' ')) { err = "not a YUV4MPEG2 stream"; return false; }
  std::string tag = "420jpeg";
  size_t p = 9;
  while (p < line.size()) {
    while (p < line.size() && line[p] == ' ') p++;
    size_t q = line.find(' ', p);
    if (q == std::string::npos) q = line.size();
    if (q == p) break;
    const std::string t = line.substr(p, q - p);
    p = q;
    const std::string v = t.substr(1);
    if (t[0] == 'W' || t[0] == 'H') {
      int n = 0;
      if (!frame_number(v, n) || n < 1) { err = "bad frame size '" + t + "'"; return false; }
      (t[0] == 'W' ? info.width : info.height) = n;
    } else if (t[0] == 'C') tag = v;
    else if (t == "XCOLORRANGE=FULL") info.full_range = true;
  }
  if (info.width < 1 || info.height < 1) { err = "the stream header gives no frame size (W, H)"; return false; }
  if (!y4m_colour_tag(tag, info, err)) return false;
  const size_t sb = size_t(info.bits / 8);
  const size_t cw = (size_t(info.width) + info.sub_x - 1) / info.sub_x, ch = (size_t(info.height) + info.sub_y - 1) / info.sub_y;
  info.y_bytes = size_t(info.width) * info.height * sb;
  info.c_bytes = cw * ch * sb;
  return true;
}

// A stream can only be read forward: frame(k) skips the frames in front of frame k and fails for one behind it.
struct y4m_reader
{
  FILE *f = nullptr;
  y4m_info info;
  int next = 0;                    // the frame the file position stands in front of
  std::string name;
  y4m_reader() = default;
  y4m_reader(const y4m_reader &) = delete;
  y4m_reader &operator=(const y4m_reader &) = delete;
  ~y4m_reader() { if (f) std::fclose(f); }

  static bool line(FILE *f, std::string &s, size_t limit = 4096)
  {
    s.clear();
    int c;
    while ((c = std::fgetc(f)) != EOF && c != '\n') { if (s.size() >= limit) return false; s += char(c); }
    return c == '\n';
  }
  bool open(const std::string &file, std::string &err)
  {
    if (f) { std::fclose(f); f = nullptr; }
    name = file; next = 0;
    f = std::fopen(file.c_str(), "rb");
    if (!f) { err = "cannot open " + file; return false; }
    std::string h;
    if (!line(f, h)) { err = file + ": no stream header"; return false; }
    if (!y4m_parse_header(h, info, err)) { err = file + ": " + err; return false; }
    return true;
  }
  // the planes of frame k - Y, then Cb, then Cr, rows dense - into `planes` (resized to info.frame_bytes())
  bool frame(int k, std::vector<uint8_t> &planes, std::string &err)
  {
    if (!f) { err = name + ": not open"; return false; }
    if (k < next) { err = name + ": frame " + std::to_string(k) + " lies behind frame " + std::to_string(next) + ": a stream is read forward"; return false; }
    try { planes.resize(info.frame_bytes()); } catch (const std::exception &) { err = name + ": out of memory"; return false; }
    for (; next <= k; next++) {
      std::string h;
      if (!line(f, h) || h.compare(0, 5, "FRAME") != 0 || (h.size() > 5 && h[5] != ' ')) {
        err = name + ": frame " + std::to_string(next) + ": " + (h.empty() && std::feof(f) ? "the stream ends in front of it" : "no FRAME header");
        return false;
      }
      if (next < k) {
        if (std::fseek(f, long(info.frame_bytes()), SEEK_CUR) != 0) { err = name + ": cannot skip frame " + std::to_string(next); return false; }
      } else if (std::fread(planes.data(), 1, planes.size(), f) != planes.size()) {
        err = name + ": frame " + std::to_string(k) + " is truncated";
        return false;
      }
    }
    return true;
  }
};

// ycbcr_tables of the Python binding: float32 of a float64 expression of the code c = v. With s = 2^(depth - 8):
// limited range (c - 16 s) / (219 s) and (c - 128 s) / (224 s), full range c / (2^depth - 1) and (c - 128 s) / (2^depth - 1)
inline void ycbcr_tables(int bits, int depth, bool full_range, std::vector<float> &y_table, std::vector<float> &c_table)
{
  const size_t n = size_t(1) << bits;
  y_table.resize(n); c_table.resize(n);
  const double s = std::ldexp(1.0, depth - 8), top = std::ldexp(1.0, depth) - 1.0;
  for (size_t v = 0; v < n; v++) {
    const double c = double(v);
    y_table[v] = float(full_range ? c / top : (c - 16.0 * s) / (219.0 * s));
    c_table[v] = float(full_range ? (c - 128.0 * s) / top : (c - 128.0 * s) / (224.0 * s));
  }
}

// ycbcr_matrix of the Python binding: "601", "709", "2020" -> m_rv, m_gu, m_gv, m_bu
inline bool ycbcr_matrix(const std::string &name, float m[4], std::string &err)
{
  double kr, kb;
  if (name == "601") { kr = 0.299; kb = 0.114; }
  else if (name == "709") { kr = 0.2126; kb = 0.0722; }
  else if (name == "2020") { kr = 0.2627; kb = 0.0593; }
  else { err = "--ycbcr_matrix " + name + ": 601, 709 or 2020"; return false; }
  const double kg = 1.0 - kr - kb;
  m[0] = float(2.0 * (1.0 - kr));
  m[1] = float(-2.0 * kb * (1.0 - kb) / kg);
  m[2] = float(-2.0 * kr * (1.0 - kr) / kg);
  m[3] = float(2.0 * (1.0 - kb));
  return true;
}

// ycbcr_forward of the Python binding: "601", "709", "2020" -> k_r, k_g, k_b, c_u, c_v (eu_hip.h: eu_ycbcr_out)
inline bool ycbcr_forward(const std::string &name, float k[5], std::string &err)
{
  double kr, kb;
  if (name == "601") { kr = 0.299; kb = 0.114; }
  else if (name == "709") { kr = 0.2126; kb = 0.0722; }
  else if (name == "2020") { kr = 0.2627; kb = 0.0593; }
  else { err = "--ycbcr_matrix " + name + ": 601, 709 or 2020"; return false; }
  k[0] = float(kr);
  k[1] = float(1.0 - kr - kb);
  k[2] = float(kb);
  k[3] = float(1.0 / (2.0 * (1.0 - kb)));
  k[4] = float(1.0 / (2.0 * (1.0 - kr)));
  return true;
}

// ycbcr_steps of the Python binding, the inverse of ycbcr_tables: the step tables (eu_hip.h: eu_ycbcr_out) of the
// quantiser code(v) = clip(floor(double(v) * a + b + 0.5), 0, 2^depth - 1), NaN -> 0, bisected over the float keys as
// encode_steps bisects. With s = 2^(depth - 8): limited range a, b = 219 s, 16 s (luma) and 224 s, 128 s (chroma);
// full range 2^depth - 1, 0 and 2^depth - 1, 128 s. steps[0] = -inf, NaN behind 2^depth - 1; codes in the low bits.
inline bool ycbcr_steps(int bits, int depth, bool full_range, std::vector<float> &y_steps, std::vector<float> &c_steps)
{
  if ((bits != 8 && bits != 16) || depth < 8 || depth > bits) return false;
  const size_t n = size_t(1) << bits;
  const double s = std::ldexp(1.0, depth - 8), top = std::ldexp(1.0, depth) - 1.0;
  const uint32_t lo_key = float_key(-HUGE_VALF), hi_key = float_key(HUGE_VALF);
  auto build = [&](std::vector<float> &steps, double a, double b) {
    auto q = [&](float v) -> double {
      if (v != v) return 0.0;
      const double c = std::floor(double(v) * a + b + 0.5);
      return c < 0.0 ? 0.0 : c > top ? top : c;
    };
    steps.assign(n, std::nanf(""));
    steps[0] = -HUGE_VALF;
    uint32_t lo = lo_key;
    for (unsigned k = 1; k <= unsigned(top); k++) {
      uint32_t l = lo, h = hi_key;
      while (l < h) {
        const uint32_t m = l + (h - l) / 2;
        if (q(key_float(m)) >= double(k)) h = m; else l = m + 1;
      }
      steps[k] = key_float(l);
      lo = l;
    }
  };
  build(y_steps, full_range ? top : 219.0 * s, full_range ? 0.0 : 16.0 * s);
  build(c_steps, full_range ? top : 224.0 * s, 128.0 * s);
  return true;
}

// "N" or "N:D", both whole and at least 1
inline bool parse_fps(const std::string &s, int &num, int &den)
{
  const size_t c = s.find(':');
  den = 1;
  if (!frame_number(s.substr(0, c), num) || num < 1) return false;
  return c == std::string::npos || (frame_number(s.substr(c + 1), den) && den >= 1);
}

// The counterpart of y4m_reader: a YUV4MPEG2 stream written frame by frame. format "420" | "422" | "444", depth 8, 10,
// 12 or 16 - above 8 the samples are 16-bit little-endian words with the code in the low bits, the tags C420p10 and
// so on that the reader accepts. 8-bit 4:2:0 is tagged C420jpeg: a box mean of the chroma is centre siting.
struct y4m_writer
{
  FILE *f = nullptr;
  y4m_info info;
  int frames = 0;
  std::string name, tag;
  y4m_writer() = default;
  y4m_writer(const y4m_writer &) = delete;
  y4m_writer &operator=(const y4m_writer &) = delete;
  ~y4m_writer() { if (f) std::fclose(f); }

  // the frames' layout for a format and a depth, without a file: what open() writes planes of
  static bool layout(int width, int height, const std::string &format, int depth, bool full_range, y4m_info &info,
                     std::string &tag, std::string &err)
  {
    if (width < 1 || height < 1) { err = "a .y4m frame has at least one pixel"; return false; }
    if (format != "420" && format != "422" && format != "444") { err = "--y4m_format " + format + ": 420, 422 or 444"; return false; }
    if (depth != 8 && depth != 10 && depth != 12 && depth != 16) { err = "--y4m_depth " + std::to_string(depth) + ": 8, 10, 12 or 16"; return false; }
    tag = depth == 8 ? (format == "420" ? "420jpeg" : format) : format + "p" + std::to_string(depth);
    info = y4m_info();
    info.width = width; info.height = height;
    if (!y4m_colour_tag(tag, info, err)) return false;
    info.full_range = full_range;
    const size_t sb = size_t(info.bits / 8);
    const size_t cw = (size_t(width) + info.sub_x - 1) / info.sub_x, ch = (size_t(height) + info.sub_y - 1) / info.sub_y;
    info.y_bytes = size_t(width) * height * sb;
    info.c_bytes = cw * ch * sb;
    return true;
  }
  // the stream header, one line without its newline
  static std::string header(const y4m_info &info, const std::string &tag, int fps_num, int fps_den)
  {
    return "YUV4MPEG2 W" + std::to_string(info.width) + " H" + std::to_string(info.height) + " F" + std::to_string(fps_num) +
           ":" + std::to_string(fps_den) + " Ip A1:1 C" + tag + (info.full_range ? " XCOLORRANGE=FULL" : "");
  }
  bool open(const std::string &file, int width, int height, const std::string &format, int depth, bool full_range,
            int fps_num, int fps_den, std::string &err)
  {
    if (f) { std::fclose(f); f = nullptr; }
    name = file; frames = 0;
    if (fps_num < 1 || fps_den < 1) { err = "--fps N[:D]: whole numbers, at least 1"; return false; }
    if (!layout(width, height, format, depth, full_range, info, tag, err)) return false;
    f = std::fopen(file.c_str(), "wb");
    if (!f) { err = "cannot write " + file; return false; }
    const std::string h = header(info, tag, fps_num, fps_den) + "\n";
    if (std::fwrite(h.data(), 1, h.size(), f) != h.size()) { err = "cannot write " + file; return false; }
    return true;
  }
  // one frame: the planes Y, Cb, Cr behind one another, rows dense, samples in HOST order (info.frame_bytes() bytes)
  bool frame(const uint8_t *planes, std::string &err)
  {
    if (!f) { err = name + ": not open"; return false; }
    bool ok = std::fwrite("FRAME\n", 1, 6, f) == 6;
    const size_t nb = info.frame_bytes();
    const uint16_t one = 1;
    if (info.bits == 8 || *reinterpret_cast<const uint8_t *>(&one) == 1) ok = ok && std::fwrite(planes, 1, nb, f) == nb;
    else {                                       // a big-endian host: low byte first
      std::vector<uint8_t> le(nb);
      for (size_t i = 0; i + 1 < nb; i += 2) { le[i] = planes[i + 1]; le[i + 1] = planes[i]; }
      ok = ok && std::fwrite(le.data(), 1, nb, f) == nb;
    }
    if (!ok) { err = "cannot write " + name; return false; }
    frames++;
    return true;
  }
  bool close(std::string &err)
  {
    if (!f) return true;
    const bool ok = std::fclose(f) == 0;
    f = nullptr;
    if (!ok) err = "cannot write " + name;
    return ok;
  }
};

inline bool probe_y4m(const std::string &name, int &width, int &height, int &nchannels, std::string &err)
{
  y4m_reader r;
  if (!r.open(name, err)) return false;
  width = r.info.width; height = r.info.height; nchannels = 3;
  return true;
}

}  // namespace io
}  // namespace project
#endif
