// Which caller-supplied rays the ray path (eu_render_rays.hip, eu_hip_render_rays) evaluates at all.
// The steppers only ever hand `act` finite, non-null rays; a caller's array holds arbitrary bit patterns.
// A ray with a non-finite component, or with all three components zero, is a MISS - zeros in every
// channel - decided on the bit patterns before any arithmetic; a ninepack is a miss when any of its nine
// floats is non-finite or its centre ray is null. Plain C and C++, host and device: tests/test_rays_host.py
// compiles it for the host.
#ifndef EU_RAY_GUARD_H
#define EU_RAY_GUARD_H
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define EU_GUARD_FN __host__ __device__ __forceinline__
#else
#define EU_GUARD_FN static inline
#endif

EU_GUARD_FN uint32_t eu_float_bits(float v)
{
  uint32_t u;
  memcpy(&u, &v, sizeof u);
  return u;
}

// inf or NaN (quiet or signalling, either sign): the exponent field is all ones
EU_GUARD_FN int eu_nonfinite_bits(uint32_t u) { return (u & 0x7f800000u) == 0x7f800000u; }

EU_GUARD_FN int eu_ray_miss(float x, float y, float z)
{
  const uint32_t a = eu_float_bits(x), b = eu_float_bits(y), c = eu_float_bits(z);
  const int null_ray = ((a | b | c) & 0x7fffffffu) == 0u;          // +-0 in all three; a denormal is not zero
  return eu_nonfinite_bits(a) | eu_nonfinite_bits(b) | eu_nonfinite_bits(c) | null_ray;
}

// in: {ray, x-neighbour, y-neighbour} as twine_t::eval reads them (twining.h:128-263)
EU_GUARD_FN int eu_ninepack_miss(const float *in)
{
  int bad = eu_ray_miss(in[0], in[1], in[2]);
  for (int k = 3; k < 9; k++) bad |= eu_nonfinite_bits(eu_float_bits(in[k]));
  return bad;
}

// The second line of defence, behind the coordinate stage: a tap ray of a ninepack (ray + cx * dx + cy * dy)
// may overflow or cancel to the null ray although the nine floats passed; the gates (eu_gate, eu_gate2) fold
// every FINITE coordinate into [lower, upper] and nothing else, so a lane whose source coordinate is not
// finite does not gather ("rays from the caller").
EU_GUARD_FN int eu_coord_finite(float sx, float sy)
{
  return !(eu_nonfinite_bits(eu_float_bits(sx)) | eu_nonfinite_bits(eu_float_bits(sy)));
}

#endif
