/* eu_rgbe.h - the two pixel functions of the Radiance RGBE format: a quad R G B E to three floats and back.
 * ONE statement of each, for the file route (include/eu_image_io.hpp: read_one, write_one) and for the device
 * route (envutil_amd/csrc/eu_rgbe.hip), so that the two cannot drift apart. Plain C and C++, host and device.
 * Both functions are built from bits: no libm call, no division.
 *
 * Decode: channel = mantissa * 2^(E - 136), E == 0: zero in all three channels (the widely used rgbe.c). The
 * product is exact for every one of the 255 x 256 pairs - the smallest scale, 2^-135, is a denormal.
 *
 * Encode, as write_one has always done it: v is the largest channel by two ordered compares (a NaN channel
 * loses them), !(v >= 1e-32f) gives four zero bytes, and with frexp(v) = (mant, e) the factor is
 * mant * 256.0f / v. Numerator and denominator share `mant`, so the correctly rounded quotient is exactly
 * 2^(8 - e): the factor is built from v's exponent field, and E = e + 128. v >= 1e-32f is a normal number. A
 * channel that fails `> 0.0f` has mantissa 0; the others are truncated products below 256.
 * A largest channel at or above 2^127 has e = 128 and no exponent byte (it used to wrap to 0, which readers take
 * for black; +inf made the factor NaN). So every channel is first clamped from above to RGBE's largest value,
 * 255 * 2^119, which alone encodes as 255 . . 255. The clamp changes no byte of a pixel whose largest channel is
 * below 2^127: a channel it touches lies in (255 * 2^119, 2^127), its exponent field is that of the bound and its
 * product truncates to 255 either way.
 */
#ifndef EU_RGBE_H
#define EU_RGBE_H
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define EU_RGBE_FN __host__ __device__ __forceinline__
#else
#define EU_RGBE_FN static inline
#endif

#define EU_RGBE_MAX 0x1.fep+126f   /* 255 * 2^119 */

EU_RGBE_FN float eu_rgbe_bits_float(uint32_t u)
{
  float v;
  memcpy(&v, &u, sizeof v);
  return v;
}

/* 2^(E - 136) for E in 1 .. 255: normal from E = 10 on (biased exponent E - 9), below that the denormal with
 * the one bit E + 13 */
EU_RGBE_FN float eu_rgbe_scale(uint32_t e)
{
  return eu_rgbe_bits_float(e >= 10u ? (e - 9u) << 23 : 1u << (e + 13u));
}

/* quad: R | G << 8 | B << 16 | E << 24, the four bytes in memory order read as a little-endian word */
EU_RGBE_FN void eu_rgbe_decode(uint32_t quad, float *r, float *g, float *b)
{
  const uint32_t e = quad >> 24;
  const float s = e ? eu_rgbe_scale(e) : 0.0f;
  *r = (float)(quad & 0xffu) * s;
  *g = (float)((quad >> 8) & 0xffu) * s;
  *b = (float)((quad >> 16) & 0xffu) * s;
}

EU_RGBE_FN uint32_t eu_rgbe_encode(float r, float g, float b)
{
  float v = r > g ? r : g;
  v = b > v ? b : v;
  if (!(v >= 1e-32f)) return 0u;                                   /* also NaN and negatives */
  v = v > EU_RGBE_MAX ? EU_RGBE_MAX : v;
  r = r > EU_RGBE_MAX ? EU_RGBE_MAX : r;
  g = g > EU_RGBE_MAX ? EU_RGBE_MAX : g;
  b = b > EU_RGBE_MAX ? EU_RGBE_MAX : b;
  uint32_t u;
  memcpy(&u, &v, sizeof u);
  const uint32_t fe = u >> 23;                                     /* v = mant * 2^(fe - 126), mant in [0.5, 1); 20 <= fe <= 253 */
  const float m = eu_rgbe_bits_float((261u - fe) << 23);           /* 2^(8 - (fe - 126)) */
  const uint32_t qr = (uint8_t)(int)(r > 0.0f ? r * m : 0.0f);
  const uint32_t qg = (uint8_t)(int)(g > 0.0f ? g * m : 0.0f);
  const uint32_t qb = (uint8_t)(int)(b > 0.0f ? b * m : 0.0f);
  return qr | (qg << 8) | (qb << 16) | ((fe + 2u) << 24);
}

#endif
