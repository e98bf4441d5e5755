// C ABI (include/eu_hip.h): host glue between the reference-shaped job
// description and the HIP kernels. No CPU rendering path exists in this
// library: without a HIP device every render/load call fails with
// EU_ERR_NO_DEVICE.

#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>
#include <new>
#include "eu_device.h"
#include "eu_setup_math.h"
#include "eu_imageprep.h"
#include "eu_alpha.h"
#include "eu_decode.h"
#include "eu_encode.h"
#include "eu_math2.h"
#include "eu_launch.h"
#include "eu_ray_guard.h"

struct eu_source {
  eu_facet fct;
  eu_container geom;
  int bc[2];
  int degree;
  int nch;
  float *dev;            // braced container in HBM
  size_t nfloats;
  eu_src_dev sd;
  // several devices in one process (eu_hip_init_devices): the device slot this container lives on and its
  // copies on the other slots (made on first use by eu_hip_render_devices, freed with the source)
  int slot = 0;
  eu_source *replica[EU_MAX_SLOTS] = {};
  bool is_replica = false;
};

namespace {

thread_local std::string g_err;
int fail(int code, const std::string &msg) { g_err = msg; return code; }

// A temporary device allocation of n elements: freed when it goes out of scope (eu_dev_buf, eu_launch.h, is the
// buffer that stays). Whoever queues work on it synchronises before that.
template <class T> struct eu_dev_tmp {
  T *p = nullptr;
  eu_dev_tmp() = default;
  eu_dev_tmp(const eu_dev_tmp &) = delete;
  eu_dev_tmp &operator=(const eu_dev_tmp &) = delete;
  ~eu_dev_tmp() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t n)
  {
    const hipError_t e = hipMalloc((void **)&p, n * sizeof(T));
    if (e != hipSuccess) p = nullptr;
    return e;
  }
};

struct context {
  int device = -1;
  hipStream_t stream = nullptr;
  eu_dev_buf<float> col, row, taps;
  float *lut = nullptr;        // to_screen_t's sRGB LUT, 257 floats
  eu_dev_buf<float> scr;                          // float frame of a tethered job
  // host copies of the plan's stepper tables and, from them, the layout the packed
  // kernel should use per segment of EU_SEG_ROWS frame rows (launch-level hybrid)
  std::vector<float> h_col, h_row;
  std::vector<unsigned char> seg_flags;
  bool seg_valid = false;
  unsigned long long plan_gen = 0;                // bumped whenever the stepper tables change
  int tab_finite = 0;                             // every entry of the plan's stepper tables is finite
  unsigned long long launches = 0;                // render kernel launches so far
  eu_src_dev seg_sd;
  eu_dev_buf<float> stage;                        // host-output staging
  eu_dev_buf<eu_generic> mgen;                    // multi-facet jobs: the translated facets' transformations
  float *inv_coef = nullptr;                      // --single: the inverse lens model's coefficients (eu_inv_planar)
  // who may still read the buffers that outlive a call, on a caller's stream ("Buffers that outlive a call")
  eu_readers tables;                              // col/row/taps, mcol/mrow/mtaps/msrc/mrej/mgen, inv_coef, scr
  eu_readers wl_pair;                             // wl and the staged kernels' cached plans: behind EVERY launch pair
  eu_readers rays, views, encode, alpha;          // rtaps | vscal/vcol/vrow/vtaps/vsrc | esteps | aplan
  bool encode_own = false;                        // the library's own stream has used scr or esteps since a caller's
                                                  // stream last waited for it (it leaves no event: order_encoders)
  hipStream_t copy = nullptr;                     // D2H of a host-output frame, chunk by chunk
  hipEvent_t chunk_done[4] = { nullptr, nullptr, nullptr, nullptr };
  eu_dev_buf<int> wl;                             // eu_render4.hip work list (count, done, tile ids)
  // the tables of the last target stay valid while (target geometry,
  // orientation, taps) repeat: streaming / tethered jobs re-render the same
  // target many times (envutil_main.cc:1948-1982)
  std::vector<unsigned char> plan_key;
  int plan_form = 0, plan_norm = 0;
  // multi-facet jobs keep their own tables
  eu_dev_buf<float> mcol, mrow, mtaps;
  eu_dev_buf<eu_src_dev> msrc;
  eu_dev_buf<float> mrej;                         // early-miss tables of a multi-facet job
  std::vector<unsigned char> mplan_key;
  int mplan_form = 0, mplan_norm = 0;
  eu_dev_buf<float> strip;                        // eu_hip_render_devices: this slot's rows before they are gathered
  // eu_hip_render_rays keeps its own tap table (the plan's, `taps`, is part of the cached plan of eu_hip_render)
  // and its own staging of host rays
  eu_dev_buf<float> rtaps, rstage;
  std::vector<float> rtaps_host;                  // what rtaps holds
  // eu_hip_render_views: the views' scalar blocks, the stepper tables the table kernel makes from them (one chunk
  // of views), its tap table and the staging of a host output - all its own, like eu_hip_render_rays' buffers
  eu_dev_buf<eu_view_dev> vscal;
  eu_dev_buf<float> vcol, vrow, vtaps, vstage;
  eu_dev_buf<eu_src_dev> vsrc;                    // eu_hip_render_views_multi: the facets' evaluator parameters
  std::vector<float> vtaps_host;                  // what vtaps holds
  // eu_hip_encode_samples / eu_hip_render_samples: the step tables on the device (colour, then alpha), the host copy
  // they were uploaded from - it stays, so that an upload queued on a stream never reads a caller's memory after the
  // call, and equal tables are not sent again - and the staging of a host frame and of a host output
  eu_dev_buf<float> esteps, eframe;
  eu_dev_buf<uint32_t> eout;
  std::vector<float> esteps_host;
  eu_dev_buf<int32_t> aplan;                      // row plan of the last device alpha edit
};
// One context per device SLOT. A process that never calls eu_hip_init_devices has one slot (one process per
// GPU, the set-up bench.py's multi-rank runs use); eu_hip_init_devices makes a slot per listed device, and every
// entry point works on the current one (`g`).
context ctx_[EU_MAX_SLOTS];
int nslots_ = 1, cur_slot_ = 0;
#define g (ctx_[cur_slot_])

#define HIPCHK(call)                                                          \
  do {                                                                        \
    hipError_t e_ = (call);                                                   \
    if (e_ != hipSuccess)                                                     \
      return fail(EU_ERR_NO_DEVICE, std::string(#call ": ") + hipGetErrorString(e_)); \
  } while (0)

// the end of a call with result `rc` that may have left work on a caller's stream (null: the library's own, no event)
int note_caller(eu_readers &r, void *stream, int rc)
{
  const hipError_t e = stream ? r.note((hipStream_t)stream) : hipSuccess;
  return rc || e == hipSuccess ? rc : fail(EU_ERR_NO_DEVICE, std::string("stream order: ") + hipGetErrorString(e));
}

// whatever happens after this, nothing of the call may still use the caller's host memory or a staging buffer when it returns
struct drain {
  hipStream_t a, b; bool on = true;
  ~drain() { if (on) { (void)hipStreamSynchronize(a); if (b != a) (void)hipStreamSynchronize(b); } }
};

int set_slot(int k)
{
  cur_slot_ = k;
  if (ctx_[k].device >= 0) HIPCHK(hipSetDevice(ctx_[k].device));
  return EU_OK;
}

// per-device state: the library's stream and to_screen_t's sRGB LUT. Used by the implicit
// initialisation and by eu_hip_init; switching devices while sources or tables of the old
// device are alive is refused by eu_hip_init.
int init_device(int dev)
{
  HIPCHK(hipSetDevice(dev));
  if (!g.stream) HIPCHK(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
  if (!g.lut) {
    float lut[257];
    eu::screen_lut(lut);
    HIPCHK(hipMalloc((void **)&g.lut, sizeof lut));
    HIPCHK(hipMemcpy(g.lut, lut, sizeof lut, hipMemcpyHostToDevice));
  }
  g.device = dev;
  return EU_OK;
}

int ensure_init()
{
  if (g.device >= 0) return EU_OK;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(EU_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
  int dev = 0;
  const char *lr = getenv("LOCAL_RANK");
  if (lr) dev = atoi(lr) % n;
  return init_device(dev);
}

// evaluator + mount parameters (eval.h:2039-2164, environment.h:594-633)
void fill_src_dev(eu_source *s)
{
  eu_src_dev &d = s->sd;
  const eu_facet &f = s->fct;
  memset(&d, 0, sizeof d);
  const eu_container &g0 = s->geom;
  d.base = s->dev + ((size_t)g0.left[1] * g0.shape[0] + g0.left[0]) * s->nch;
  d.es0 = s->nch;
  d.es1 = (long long)s->nch * g0.shape[0];
  d.prj = f.projection; d.nch = s->nch; d.degree = s->degree;
  float lo[2], up[2]; int gt[2];
  for (int a = 0; a < 2; a++) {
    int bc = s->bc[a];
    long double l = 0.0L, u = (long double)(g0.core[a] - 1);
    if (bc == EU_BC_REFLECT || bc == EU_BC_PERIODIC) { l = -0.5L; u += 0.5L; }
    lo[a] = (float)l; up[a] = (float)u;
    if (g0.core[a] == 1) { bc = EU_BC_CONSTANT; lo[a] = up[a] = 0.0f; }
    gt[a] = bc == EU_BC_PERIODIC ? 2 : (bc == EU_BC_MIRROR || bc == EU_BC_REFLECT) ? 1 : 0;
  }
  d.gate0 = gt[0]; d.gate1 = gt[1];
  d.lower0 = lo[0]; d.upper0 = up[0]; d.lower1 = lo[1]; d.upper1 = up[1];
  d.brighten = (float)f.brighten;
  d.mask_paint = f.mask_paint;
  d.recip_step = (float)(1.0 / f.step);
  d.mask_all = eu_cube_source(f.projection) || (f.projection == EU_FISHEYE && f.hfov >= M_PI * 2.0);
  eu::weight_matrix(s->degree, d.wm);
  if (eu_cube_source(f.projection)) return;
  double te[4], we[4];
  eu::get_extent(f.projection, f.width, f.height, f.hfov, te);
  double wx = te[1] - te[0], wy = te[3] - te[2];
  // environment.h:617-633, including its use of total_width / window_width
  // in the y terms
  double px = double(f.window_x_offset) / f.width;
  double py = double(f.window_y_offset) / f.width;
  we[0] = te[0] + px * wx; we[2] = te[2] + py * wy;
  px = double(f.window_x_offset + f.window_width) / f.width;
  py = double(f.window_y_offset + f.window_width) / f.width;
  we[1] = te[0] + px * wx; we[3] = te[2] + py * wy;
  {
    // process_geometry, envutil_basic.h:499-521; the planar functor is only
    // installed when the radial polynomial is present (environment.h:1692-1695)
    double dv = std::fabs(te[3] - te[2]) / 2.0, dh = std::fabs(te[1] - te[0]) / 2.0;
    d.has_lcp = (f.a != 0.0 || f.b != 0.0 || f.c != 0.0);
    d.has_shift = d.has_lcp && (f.h != 0.0 || f.v != 0.0);
    d.has_shear = d.has_lcp && (f.shear_g != 0.0 || f.shear_t != 0.0);
    d.lens_a = (float)f.a; d.lens_b = (float)f.b; d.lens_c = (float)f.c;
    d.lens_d = 1.0f - (d.lens_a + d.lens_b + d.lens_c);
    d.lens_s = (float)((dh < dv) ? dh : dv);
    d.lens_h = (float)f.h; d.lens_v = (float)f.v;
    d.shear_g = f.shear_g; d.shear_t = f.shear_t;
  }
  d.rej_cos = -2.0f;
  if (f.projection == EU_RECTILINEAR) {
    d.rej_cos = 0.0f;                      // the mask includes rz > 0 (environment.h:1135-1137)
  } else if (f.projection == EU_FISHEYE && !d.has_shear) {
    // radius after the lens polynomial: |c'| >= r * |sum(r / s)| - |shift|; outside the
    // window for sure when its larger component (>= |c'| / sqrt 2) exceeds every edge
    const double W = 1.001 * std::max(std::max(std::fabs(we[0]), std::fabs(we[1])),
                                      std::max(std::fabs(we[2]), std::fabs(we[3])));
    const double shift = d.has_shift ? std::hypot((double)d.lens_h, (double)d.lens_v) : 0.0;
    auto outside = [&](double r) {
      double sum = 1.0;
      if (d.has_lcp) {
        const double x = r / d.lens_s;
        sum = d.lens_d + d.lens_c * x + d.lens_b * x * x + d.lens_a * x * x * x;
      }
      return (r * std::fabs(sum) - shift) / std::sqrt(2.0) > W;
    };
    // the smallest angle from which EVERY larger angle is outside
    double r0 = -1.0;
    for (double r = M_PI; r >= 0.0; r -= 1e-4) {
      if (!outside(r)) break;
      r0 = r;
    }
    if (r0 >= 0.0) d.rej_cos = (float)(std::cos(r0) - 1e-4);
  }
  d.tex_x0 = te[0]; d.tex_y0 = te[2];
  d.ext_w = (float)(te[1] - te[0]); d.ext_h = (float)(te[3] - te[2]);
  d.total_w = (float)f.width; d.total_h = (float)f.height;
  d.win_x_off = (float)f.window_x_offset; d.win_y_off = (float)f.window_y_offset;
  d.wex0 = (float)we[0]; d.wex1 = (float)we[1]; d.wex2 = (float)we[2]; d.wex3 = (float)we[3];
  // hits have 0 <= coordinate - extent.x0 <= extent width: verify the cheap
  // constant division over that whole range (twice the width for slack)
  // atan2f returns values in [-0x1.921fb6p+1, 0x1.921fb6p+1]; lat = atan2f(d, s >= 0) in
  // [-0x1.921fb6p+0, 0x1.921fb6p+0]
  d.always_hit = f.projection == EU_SPHERICAL && d.wex0 <= -0x1.921fb6p+1f && d.wex1 >= 0x1.921fb6p+1f
              && d.wex2 <= -0x1.921fb6p+0f && d.wex3 >= 0x1.921fb6p+0f;
  d.rcp_ext_w = 1.0f / d.ext_w; d.rcp_ext_h = 1.0f / d.ext_h;
  d.cdiv_ok = eu_verify_const_div(d.ext_w, 2.0f * d.ext_w, g.stream)
           && eu_verify_const_div(d.ext_h, 2.0f * d.ext_h, g.stream);
}

int check_facet(const eu_facet *f)
{
  if (!f) return fail(EU_ERR_ARGUMENT, "null facet");
  if (f->nchannels < 1 || f->nchannels > 4) return fail(EU_ERR_ARGUMENT, "nchannels must be 1..4");
  if (f->mask_paint < 0 || f->mask_paint > 2) return fail(EU_ERR_ARGUMENT, "mask_paint must be 0, 1 or 2");
  if (f->projection < 0 || f->projection > EU_BIATAN6) return fail(EU_ERR_ARGUMENT, "unknown source projection");
  if (f->width <= 0 || f->height <= 0) return fail(EU_ERR_ARGUMENT, "empty source image");
  return EU_OK;
}

// a handle without a container: the facet, the degree and the channel count; nullptr: no host memory
eu_source *bare_source(const eu_facet *fct, int spline_degree)
{
  eu_source *s = new (std::nothrow) eu_source;
  if (!s) return nullptr;
  memset(s, 0, sizeof *s);
  s->fct = *fct;
  s->degree = spline_degree;
  s->nch = fct->nchannels;
  return s;
}

// the handle and its container (not the copies on other device slots: eu_hip_source_release)
void destroy_source(eu_source *s)
{
  if (!s) return;
  if (s->dev) (void)hipFree(s->dev);
  delete s;
}

// allocates the eu_source and its container for the facet
int new_source(const eu_facet *fct, int spline_degree, int bc0, int bc1, int support_min,
               int tile_size, eu_source **out)
{
  if (spline_degree < 0 || spline_degree > EU_MAX_DEGREE)
    return fail(EU_ERR_ARGUMENT, "spline degree out of range");
  eu_source *s = bare_source(fct, spline_degree);
  if (!s) return fail(EU_ERR_MEMORY, "host allocation failed");
  const bool cube = eu_cube_source(fct->projection);
  eu::metrics m {};
  if (cube) {
    // IR image: container == core, REFLECT x REFLECT (cubemap.h:576-583)
    m = eu::make_metrics(fct->width, fct->hfov, support_min, tile_size);
    // The support frame is all the margin the IR has: a ray at a face's edge picks up at left_frame - 0.5, and a
    // spline of degree d reaches d / 2 + 1 texels beyond that. With less frame than that (--support_min below its
    // default of 8 AND a small --tile_size) the reference reads outside its IR array (README.md:1553: the frame
    // is there "so that interpolators needing support can operate without special-casing"); here the job is refused.
    // Found by the randomised set-up test at seed 1033: biatan6, 45-pixel faces, degree 4, support 1, tile 16 - frame
    // 1 / 2 - where the oracle and the device each read their own memory in front of the array.
    const long need = spline_degree / 2 + 1;
    if (m.left_frame_px + m.inherent_px < need || m.right_frame_px + m.inherent_px < need) {
      destroy_source(s);
      return fail(EU_ERR_ARGUMENT, "cubemap support frame (--support_min / --tile_size) too small for the spline degree");
    }
    s->geom.shape[0] = s->geom.core[0] = m.section_px;
    s->geom.shape[1] = s->geom.core[1] = 6 * m.section_px;
    s->geom.left[0] = s->geom.left[1] = s->geom.right[0] = s->geom.right[1] = 0;
    s->bc[0] = s->bc[1] = EU_BC_REFLECT;
  } else {
    eu::container_geometry(spline_degree, bc0, bc1, fct->window_width, fct->window_height, &s->geom);
    s->bc[0] = bc0; s->bc[1] = bc1;
  }
  s->nfloats = (size_t)s->geom.shape[0] * s->geom.shape[1] * s->nch;
  // slack behind the container: the LDS-staging kernel (eu_render4.hip) fetches whole
  // 64-texel instructions, up to 3 rows and 63 texels past a tile's box (never evaluated)
  const size_t slack = (size_t)4 * s->geom.shape[0] * s->nch + 64 * 4;
  hipError_t e = hipMalloc((void **)&s->dev, (s->nfloats + slack) * sizeof(float));
  if (e != hipSuccess) s->dev = nullptr;
  else e = hipMemset(s->dev + s->nfloats, 0, slack * sizeof(float));
  if (e != hipSuccess) { destroy_source(s); return fail(EU_ERR_MEMORY, std::string("hipMalloc: ") + hipGetErrorString(e)); }
  fill_src_dev(s);
  if (cube) {
    s->sd.refc_md = (float)m.refc_md;
    s->sd.model_to_px = (float)m.model_to_px;
    s->sd.section_px = (int)m.section_px;
  }
  *out = s;
  return EU_OK;
}

// boundary conditions source_t picks (environment.h:638-644)
void source_bcs(const eu_facet *f, int *bc0, int *bc1)
{
  *bc0 = EU_BC_REFLECT; *bc1 = EU_BC_REFLECT;
  if ((f->projection == EU_SPHERICAL || f->projection == EU_CYLINDRICAL)
      && std::fabs(f->hfov - 2.0 * M_PI) < .000001)
    *bc0 = EU_BC_PERIODIC;
}

// the prefilter source_t picks (environment.h:905-936): a full spherical image gets the two-axis periodic
// scheme, everything else bspline::prefilter(). A stronger test than source_bcs', and a separate one.
// (a full-sphere image smaller than its frame - 2 x 1, 4 x 2, 6 x 3 for degree 3 - takes the sequential forms of
// the pole rows and of the horizontal bracing: eu_setup.hip, pole_rows_seq_kernel / brace_seq_kernel)
bool full_sphere(const eu_facet *f)
{
  return f->projection == EU_SPHERICAL && std::fabs(f->hfov - 2.0 * M_PI) < .000001 && f->width == 2 * f->height;
}

// the processed frame: the whole target or its crop window (store_cropped)
inline int frame_w(const eu_target *t) { return t->crop_w > 0 ? t->crop_w : t->width; }
inline int frame_h(const eu_target *t) { return t->crop_w > 0 ? t->crop_h : t->height; }

// rows of the processed frame that belong to this call (interleaved bands)
int local_rows(int height, int band_rows, int band_count, int band_index)
{
  if (band_count <= 1) return height;
  const int nb = (height + band_rows - 1) / band_rows;       // bands of the frame
  int rows = 0;
  for (int b = band_index; b < nb; b += band_count)
    rows += std::min(band_rows, height - b * band_rows);
  return rows;
}

int band_shift_of(int band_rows)
{
  int sh = 0;
  while ((1 << sh) < band_rows) sh++;
  return sh;
}

int check_target(const eu_target *t)
{
  if (t->nchannels < 1 || t->nchannels > 4) return fail(EU_ERR_ARGUMENT, "target channels must be 1..4");
  if (t->width <= 0 || t->height <= 0) return fail(EU_ERR_ARGUMENT, "empty target");
  if (t->crop_w < 0 || (t->crop_w > 0 && (t->crop_h <= 0 || t->crop_x0 < 0 || t->crop_y0 < 0 ||
                        (long long)t->crop_x0 + t->crop_w > t->width ||
                        (long long)t->crop_y0 + t->crop_h > t->height)))
    return fail(EU_ERR_ARGUMENT, "crop window outside the target");
  if (t->band_count > 1) {
    if (t->band_rows < 4 || (t->band_rows & (t->band_rows - 1)))
      return fail(EU_ERR_ARGUMENT, "band_rows must be a power of two >= 4");
    if (t->band_index < 0 || t->band_index >= t->band_count)
      return fail(EU_ERR_ARGUMENT, "band_index outside [0, band_count)");
  }
  if (t->row_begin < 0 || t->row_begin > t->row_end ||
      t->row_end > local_rows(frame_h(t), t->band_rows, t->band_count, t->band_index))
    return fail(EU_ERR_ARGUMENT, "row range outside the target");
  if (t->ntaps < 0 || t->ntaps > EU_MAX_TAPS || (t->ntaps > 0 && !t->taps))
    return fail(EU_ERR_ARGUMENT, "bad twining tap table");
  if ((t->projection == EU_CUBEMAP || t->projection == EU_BIATAN6) && t->height != 6 * t->width)
    return fail(EU_ERR_ARGUMENT, "cubemap targets are 1:6");
  if (t->synopsis != EU_SYN_PANORAMA && t->synopsis != EU_SYN_HDR_MERGE)
    return fail(EU_ERR_ARGUMENT, "unknown synopsis");
  if (t->out_format != EU_OUT_FLOAT && t->out_format != EU_OUT_SRGBA8)
    return fail(EU_ERR_ARGUMENT, "unknown output format");
  if (t->out_format == EU_OUT_SRGBA8 && t->stage)
    return fail(EU_ERR_ARGUMENT, "stage outputs are float only");
  if ((t->stage == 3 || t->stage == 4) && t->ntaps == 0)
    return fail(EU_ERR_ARGUMENT, "stages 3 and 4 are the neighbour rays of a twined job: they need a tap table");
  return EU_OK;
}

// tf22 of a --single job: the inverse planar transformation of the facet the target recreates
// (environment.h:285-307); the inverse lens model goes to device memory (g.inv_coef)
int build_inv_planar(const eu_target *t, eu_inv_planar *q)
{
  memset(q, 0, sizeof *q);
  const eu_facet *f = t->single;
  if (!f || !eu::has_2d_tf(*f)) return EU_OK;
  q->shear = f->shear_g != 0.0 || f->shear_t != 0.0;
  q->shift = f->h != 0.0 || f->v != 0.0;
  q->lcp = f->a != 0.0 || f->b != 0.0 || f->c != 0.0;
  q->shear_g = f->shear_g; q->shear_t = f->shear_t;
  { // the reference radius: half the smaller edge of the facet's extent (envutil_basic.h:508-513)
    const double dv0 = std::fabs(t->y1 - t->y0) / 2.0, dh0 = std::fabs(t->x1 - t->x0) / 2.0;
    q->s = (dh0 < dv0) ? dh0 : dv0; }
  q->h = (float)f->h; q->v = (float)f->v;
  if (q->lcp) {
    // r_max of facet_spec::process_geometry (envutil_basic.h:508-520) from the target's (= the facet's) extent
    const double dv = std::fabs(t->y1 - t->y0) / 2.0, dh = std::fabs(t->x1 - t->x0) / 2.0;
    const double aspect = (dh >= dv) ? dh / dv : dv / dh;
    std::vector<float> coef;
    if (!eu::make_inverse_lcp(f->a, f->b, f->c, std::sqrt(1 + aspect * aspect), 100, coef, q->rr_max))
      return fail(EU_ERR_ARGUMENT, "--single: the lens polynomial has no inverse over the facet (the reference asserts here)");
    HIPCHK(g.tables.host_wait());
    if (!g.inv_coef) HIPCHK(hipMalloc((void **)&g.inv_coef, 128 * sizeof(float)));
    HIPCHK(hipMemcpyAsync(g.inv_coef, coef.data(), coef.size() * sizeof(float), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    q->nk = (int)coef.size() - 4;
    q->coef = g.inv_coef + 2;
    eu::weight_matrix(3, q->m);
  }
  return EU_OK;
}

// the tap table as the kernels read it: x and y pre-multiplied by the bias 4.0 (twine_t ctor, twining.h:106-121)
std::vector<float> biased_taps(const float *taps, int ntaps)
{
  std::vector<float> v(taps, taps + 3 * (size_t)ntaps);
  for (int k = 0; k < ntaps; k++)
    for (int a = 0; a < 2; a++) v[3 * k + a] *= 4.0f;
  return v;
}

// The key of a target's cached plan for nsrc facets, everything the stepper tables depend on: the target without
// the fields that only say which part of the frame a call renders and how it is stored (the tables cover the
// whole frame), [the number of facets - the multi-facet cache's keys only,] the facets' orientations, the taps.
std::vector<unsigned char> plan_key_of(const eu_target *t, eu_source *const *srcs, int nsrc, bool multi)
{
  const size_t ntap_bytes = 3 * sizeof(float) * (size_t)t->ntaps;
  std::vector<unsigned char> key(sizeof(eu_target) + (multi ? sizeof(int) : 0) + (size_t)nsrc * 3 * sizeof(double) + ntap_bytes);
  eu_target tk = *t;
  tk.taps = nullptr; tk.single = nullptr; tk.row_begin = 0; tk.row_end = 0; tk.stage = 0; tk.nchannels = 0; tk.out_format = 0;
  tk.band_rows = 0; tk.band_count = 0; tk.band_index = 0;
  unsigned char *q = key.data();
  memcpy(q, &tk, sizeof tk); q += sizeof tk;
  if (multi) { memcpy(q, &nsrc, sizeof(int)); q += sizeof(int); }
  for (int f = 0; f < nsrc; f++) {
    double fo[3] = { srcs[f]->fct.yaw, srcs[f]->fct.pitch, srcs[f]->fct.roll };
    memcpy(q, fo, sizeof fo); q += sizeof fo;
  }
  if (t->ntaps > 0) memcpy(q, t->taps, ntap_bytes);
  return key;
}

// the frame and band fields eu_render_params and eu_multi_params share (p zeroed: no bands)
template <class P> void fill_frame(const eu_target *t, P *p)
{
  p->width = frame_w(t); p->height = frame_h(t);
  p->row_begin = t->row_begin; p->row_end = t->row_end;
  if (t->band_count > 1) {
    p->band_shift = band_shift_of(t->band_rows); p->band_count = t->band_count; p->band_index = t->band_index;
  }
}

int build_params(const eu_target *t, eu_source *const *srcs, int nsrc, float *out_dev,
                 size_t row_stride_bytes, const eu_switches &sw, eu_render_params *p)
{
  if (!t || !srcs || !out_dev) return fail(EU_ERR_ARGUMENT, "null argument");
  if (nsrc != 1)
    return fail(EU_ERR_ARGUMENT, "build_params takes one source (several facets go through build_multi)");
  eu_source *s = srcs[0];
  if (!s) return fail(EU_ERR_HANDLE, "null source");
  { int rc0 = check_target(t); if (rc0) return rc0; }
  if (row_stride_bytes % sizeof(float))
    return fail(EU_ERR_ARGUMENT, "row stride must be a multiple of 4 bytes");
  const bool twine = t->ntaps > 0;
  // orientation: envutil_payload.cc:1923-1948
  eu::mat3 r_cam = eu::make_r3(t->roll, t->pitch, t->yaw, false);
  eu::mat3 r_fct = eu::make_r3(s->fct.roll, s->fct.pitch, s->fct.yaw, true);
  eu::mat3 basis = eu::rotate(r_cam, r_fct);
  // plan key: everything the tables depend on
  // a facet with translation parameters: generic_stepper over tf_ex_facet (envutil_payload.cc:2095-2110,
  // :2214-2224), normalised only under twining (deriv_stepper<..., generic_stepper, true>)
  eu_generic gen;
  memset(&gen, 0, sizeof gen);
  if ((eu::has_translation(s->fct) || eu::generic_target(*t)) && !eu::make_generic(*t, s->fct, gen))
    return fail(EU_ERR_UNSUPPORTED, "generic stepper (translation, --single): no planar-to-ray functor for this target projection");
  eu_inv_planar inv;
  { int rci = build_inv_planar(t, &inv); if (rci) return rci; }
  std::vector<unsigned char> key = plan_key_of(t, srcs, 1, false);
  int form = g.plan_form, norm_mode = g.plan_norm;
  if (key != g.plan_key) {
    eu::stepper_tables tb;
    if (!eu::build_stepper_tables(*t, basis, twine, twine, tb))
      return fail(EU_ERR_UNSUPPORTED, "no stepper for this target projection");
    // kernels of earlier jobs may still read the tables on callers' streams (the library's own has the copies behind them)
    HIPCHK(g.tables.host_wait());
    HIPCHK(g.col.reserve(tb.col.size()));
    HIPCHK(g.row.reserve(tb.row.size()));
    HIPCHK(hipMemcpyAsync(g.col.p, tb.col.data(), tb.col.size() * sizeof(float), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(g.row.p, tb.row.data(), tb.row.size() * sizeof(float), hipMemcpyHostToDevice, g.stream));
    const std::vector<float> taps = biased_taps(t->taps, t->ntaps);
    if (twine) {
      HIPCHK(g.taps.reserve(taps.size()));
      HIPCHK(hipMemcpyAsync(g.taps.p, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice, g.stream));
    }
    // the host vectors die at the end of this block: the copies must have left them
    HIPCHK(hipStreamSynchronize(g.stream));
    form = g.plan_form = tb.form;
    norm_mode = g.plan_norm = tb.norm_mode;
    g.plan_key.swap(key);
    g.h_col.swap(tb.col);
    g.h_row.swap(tb.row);
    g.seg_valid = false;
    g.plan_gen++;
    g.tab_finite = 1;
    for (float v : g.h_col) if (!std::isfinite(v)) g.tab_finite = 0;
    for (float v : g.h_row) if (!std::isfinite(v)) g.tab_finite = 0;
  }
  memset(p, 0, sizeof *p);
  p->tab_finite = g.tab_finite;
  fill_frame(t, p);
  p->form = form; p->norm_mode = norm_mode;
  if (gen.on) {                // the tables (planar x per column, planar y per row) are the same
    p->form = EU_FORM_GENERIC;
    p->norm_mode = twine ? EU_NORM_DIV : EU_NORM_NONE;
    p->gen = gen;
    p->inv = inv;
  }
  p->twine = twine; p->ntaps = t->ntaps; p->stage = t->stage; p->nch = s->nch;
  p->nch_out = t->nchannels;
  p->col = g.col.p; p->row = g.row.p; p->taps = g.taps.p;
  p->out = out_dev;
  p->out_stride = (long long)(row_stride_bytes / sizeof(float));
  p->src = s->sd;
  p->direct = sw.direct;
  return EU_OK;
}

// The multi-facet kernels' second early-miss stage (eu_render_multi.hip: eu_multi_maybe): for a fisheye facet
// (no shear) a table over u = cos(angle to the facet's axis), u in [rej_cos, 1], of a lower bound of the
// radius R(theta) = theta * lens polynomial(theta / s) a ray of that angle maps to (environment.h:254-284,
// geometry.h:513-531), and the window's edges moved out by 0.1 %. tab: EU_REJ_STRIDE floats (eu_launch.h); false: no table.
static bool build_reject_table(const eu_src_dev &d, float *tab, bool analytic)
{
  for (int i = 0; i < EU_REJ_STRIDE; i++) tab[i] = 0.0f;
  if (d.prj != EU_FISHEYE || d.has_shear || d.mask_all || !(d.rej_cos > -1.5f) || !(d.rej_cos < 0.999f)) return false;
  const double u0 = d.rej_cos, du = (1.0 - u0) / EU_REJ_N;
  auto radius = [&](double th, bool &okk) {
    double sum = 1.0;
    if (d.has_lcp) {
      const double x = th / d.lens_s;
      sum = d.lens_d + d.lens_c * x + d.lens_b * x * x + d.lens_a * x * x * x;
    }
    if (!(sum > 0.0)) okk = false;
    return th * sum;
  };
  std::vector<double> raw(EU_REJ_N);
  bool okk = true;
  for (int k = 0; k < EU_REJ_N; k++) {
    const double ua = std::min(1.0, std::max(-1.0, u0 + k * du)), ub = std::min(1.0, std::max(-1.0, u0 + (k + 1) * du));
    const double t_hi = std::acos(ua), t_lo = std::acos(ub);
    double m = 1e300;
    for (int j = 0; j <= 16; j++) m = std::min(m, radius(t_lo + (t_hi - t_lo) * j / 16.0, okk));
    raw[k] = m;
  }
  if (!okk) return false;
  for (int k = 0; k < EU_REJ_N; k++) {
    double m = raw[k];
    if (k > 0) m = std::min(m, raw[k - 1]);
    if (k + 1 < EU_REJ_N) m = std::min(m, raw[k + 1]);
    tab[EU_REJ_HDR + k] = (float)(m * (1.0 - 2e-3));
  }
  const double W = std::max(std::max(std::fabs((double)d.wex0), std::fabs((double)d.wex1)),
                            std::max(std::fabs((double)d.wex2), std::fabs((double)d.wex3)));
  const double mg = 1e-3 * W;
  tab[0] = (float)u0; tab[1] = (float)(1.0 / du); tab[2] = 1.0f;
  // the table-free form (EU_HIP_REJ=2): needs R increasing over the cone
  {
    bool mono = true;
    double prev = -1.0;
    const double tmax = std::acos(std::max(-1.0, u0));
    for (int i = 0; i <= 4096 && mono; i++) {
      bool k2 = true;
      const double r = radius(tmax * i / 4096.0, k2);
      mono = k2 && r > prev;
      prev = r;
    }
    if (mono && analytic) {
      tab[2] = 2.0f;
      const double f = 1.0 - 2e-3;
      tab[10] = d.has_lcp ? 1.0f / d.lens_s : 0.0f;
      tab[11] = (float)(f * (d.has_lcp ? d.lens_d : 1.0)); tab[12] = d.has_lcp ? (float)(f * d.lens_c) : 0.0f;
      tab[13] = d.has_lcp ? (float)(f * d.lens_b) : 0.0f; tab[14] = d.has_lcp ? (float)(f * d.lens_a) : 0.0f;
    }
  }
  tab[4] = d.has_shift ? d.lens_h : 0.0f; tab[5] = d.has_shift ? d.lens_v : 0.0f;
  tab[6] = (float)(d.wex0 - mg); tab[7] = (float)(d.wex1 + mg); tab[8] = (float)(d.wex2 - mg); tab[9] = (float)(d.wex3 + mg);
  return true;
}

// fuse() for several facets (envutil_payload.cc:2139-2180, :2240-2281): one
// stepper per facet, all with normalize = true, synopsis by channel count
int build_multi(const eu_target *t, eu_source *const *srcs, int nsrc, float *out_dev,
                size_t row_stride_bytes, const eu_switches &sw, eu_multi_params *p, int *degree)
{
  { int rc0 = check_target(t); if (rc0) return rc0; }
  const eu_source *s0 = srcs[0];
  for (int f = 0; f < nsrc; f++) {
    if (!srcs[f]) return fail(EU_ERR_HANDLE, "null source");
    if (srcs[f]->degree != s0->degree) return fail(EU_ERR_ARGUMENT, "facets must share the spline degree");
  }
  const bool twine = t->ntaps > 0;
  std::vector<unsigned char> key = plan_key_of(t, srcs, nsrc, true);
  HIPCHK(g.tables.host_wait());   // g.msrc and the tables are rewritten below
  if (key != g.mplan_key) {
    eu::mat3 r_cam = eu::make_r3(t->roll, t->pitch, t->yaw, false);
    std::vector<float> rows;
    eu::stepper_tables tb;
    for (int f = 0; f < nsrc; f++) {
      eu::mat3 r_fct = eu::make_r3(srcs[f]->fct.roll, srcs[f]->fct.pitch, srcs[f]->fct.yaw, true);
      eu::mat3 basis = eu::rotate(r_cam, r_fct);
      if (!eu::build_stepper_tables(*t, basis, true, twine, tb))
        return fail(EU_ERR_UNSUPPORTED, "no stepper for this target projection");
      rows.insert(rows.end(), tb.row.begin(), tb.row.end());
    }
    HIPCHK(g.mcol.reserve(tb.col.size()));
    HIPCHK(g.mrow.reserve(rows.size()));
    HIPCHK(hipMemcpyAsync(g.mcol.p, tb.col.data(), tb.col.size() * sizeof(float), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(g.mrow.p, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice, g.stream));
    const std::vector<float> taps = biased_taps(t->taps, t->ntaps);
    if (twine) {
      HIPCHK(g.mtaps.reserve(taps.size()));
      HIPCHK(hipMemcpyAsync(g.mtaps.p, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice, g.stream));
    }
    HIPCHK(hipStreamSynchronize(g.stream));
    g.mplan_form = tb.form; g.mplan_norm = tb.norm_mode;
    g.mplan_key.swap(key);
  }
  // the facets' evaluator parameters (they can change between jobs: always refreshed)
  std::vector<eu_src_dev> sd((size_t)nsrc);
  for (int f = 0; f < nsrc; f++) sd[f] = srcs[f]->sd;
  HIPCHK(g.msrc.reserve((size_t)nsrc));
  HIPCHK(hipMemcpyAsync(g.msrc.p, sd.data(), sizeof(eu_src_dev) * (size_t)nsrc, hipMemcpyHostToDevice, g.stream));
  // the early-miss tables of the fisheye facets - OFF unless EU_HIP_REJ=1: measured on config 5 the second
  // stage drops a third of the exact hit tests and the step takes 7.67 instead of 7.30 ms (the table read is
  // one more round trip on a path that waits for memory already)
  bool any_rej = false;
  std::vector<float> rej;
  if (sw.rej) {                          // 2: the table-free form where it applies
    rej.resize((size_t)nsrc * EU_REJ_STRIDE);
    for (int f = 0; f < nsrc; f++) any_rej |= build_reject_table(sd[f], rej.data() + (size_t)f * EU_REJ_STRIDE, sw.rej == 2);
  }
  if (any_rej) {
    HIPCHK(g.mrej.reserve(rej.size()));
    HIPCHK(hipMemcpyAsync(g.mrej.p, rej.data(), rej.size() * sizeof(float), hipMemcpyHostToDevice, g.stream));
  }
  // facets with translation parameters step through generic_stepper (envutil_payload.cc:2145-2158,
  // :2246-2258); like the evaluator parameters these are refreshed on every job
  std::vector<eu_generic> gv((size_t)nsrc);
  bool any_generic = false;
  for (int f = 0; f < nsrc; f++) {
    memset(&gv[f], 0, sizeof(eu_generic));
    if (!eu::has_translation(srcs[f]->fct) && !eu::generic_target(*t)) continue;
    if (!eu::make_generic(*t, srcs[f]->fct, gv[f]))
      return fail(EU_ERR_UNSUPPORTED, "generic stepper (translation, --single): no planar-to-ray functor for this target projection");
    any_generic = true;
  }
  if (any_generic) {
    HIPCHK(g.mgen.reserve((size_t)nsrc));
    HIPCHK(hipMemcpyAsync(g.mgen.p, gv.data(), sizeof(eu_generic) * (size_t)nsrc, hipMemcpyHostToDevice, g.stream));
  }
  HIPCHK(hipStreamSynchronize(g.stream));
  eu_inv_planar inv;
  { int rci = build_inv_planar(t, &inv); if (rci) return rci; }
  memset(p, 0, sizeof *p);
  p->gen = any_generic ? g.mgen.p : nullptr;
  p->rej = any_rej ? g.mrej.p : nullptr;
  p->inv = inv;
  fill_frame(t, p);
  p->form = g.mplan_form; p->norm_mode = g.mplan_norm; p->twine = twine; p->ntaps = t->ntaps;
  p->nch = t->nchannels; p->nfct = nsrc; p->plus = (t->nchannels == 2 || t->nchannels == 4);
  p->hdr = t->synopsis == EU_SYN_HDR_MERGE;
  {
    // _hdr_merge_syn ctor (envutil_payload.cc:1346-1376): the first strict minimum / maximum of brighten
    float lowest = 100000.0f, highest = -1.0f;
    p->hdr_low = p->hdr_high = -1;
    for (int f = 0; f < nsrc; f++) {
      const float b = srcs[f]->sd.brighten;
      if (b < lowest) { lowest = b; p->hdr_low = f; }
      if (b > highest) { highest = b; p->hdr_high = f; }
    }
  }
  p->col = g.mcol.p; p->row = g.mrow.p; p->taps = g.mtaps.p; p->srcs = g.msrc.p;
  p->out = out_dev; p->out_stride = (long long)(row_stride_bytes / sizeof(float));
  *degree = s0->degree;
  return EU_OK;
}

// Launch-level hybrid of the packed kernel's two work layouts. Where source rows run
// ACROSS target rows (the inner half of the polar faces of a cubemap made from a lat/lon
// image: 0.098 -> 0.071 ms per 1024 rows) 32x16 tiles beat the 128x4 row strips; everywhere
// else the strips win (0.045 vs 0.055 ms). The frame is cut into segments of EU_SEG_ROWS
// rows (eu_select.h: eu_split_runs); 16 probe pixels per segment, evaluated on the host from the plan's stepper
// tables, say how the source rows run there. Lat/lon sources only.
// (kept while the plan's tables and the source's parameters stay the same)
void refresh_seg_flags(const eu_render_params *p)
{
  eu_src_dev cmp = p->src;
  cmp.base = nullptr;
  if (g.seg_valid && !memcmp(&cmp, &g.seg_sd, sizeof cmp)) return;
  g.seg_sd = cmp;
  g.seg_valid = true;
  const int W = p->width, H = p->height;
  const int nseg = (H + EU_SEG_ROWS - 1) / EU_SEG_ROWS;
  g.seg_flags.assign((size_t)nseg, 0);
  const eu_src_dev &s = p->src;
  if (s.prj != EU_SPHERICAL || W < 64 || g.h_col.size() < (size_t)2 * W || g.h_row.size() < (size_t)H * EU_ROW_FLOATS)
    return;
  const double kx = (double)s.total_w / s.ext_w, ky = (double)s.total_h / s.ext_h;   // pixels per radian
  auto ray = [&](int x, int y, double *r) {
    const float *rt = &g.h_row[(size_t)y * EU_ROW_FLOATS];
    const float c0 = g.h_col[(size_t)x], c1 = g.h_col[(size_t)W + x];
    for (int i = 0; i < 3; i++)
      r[i] = p->form == EU_FORM_BCA ? (double)rt[3 + i] * c0 + (double)rt[6 + i] * c1 + rt[i]
                                    : (double)rt[3 + i] * c0 + rt[i];
  };
  for (int k = 0; k < nseg; k++) {
    const int yc = std::min(k * EU_SEG_ROWS + EU_SEG_ROWS / 2, H - 1);
    int across = 0;
    for (int j = 0; j < 16; j++) {
      const int xc = std::min((int)((j + 0.5) * W / 16), W - 2);
      double a[3], b[3];
      ray(xc, yc, a);
      ray(xc + 1, yc, b);
      const double lon0 = std::atan2(a[0], a[2]), lon1 = std::atan2(b[0], b[2]);
      const double lat0 = std::atan2(a[1], std::hypot(a[0], a[2])), lat1 = std::atan2(b[1], std::hypot(b[0], b[2]));
      double dlon = std::fabs(lon1 - lon0);
      if (dlon > M_PI) dlon = 2.0 * M_PI - dlon;
      if (std::fabs(lat1 - lat0) * ky > 0.5 * dlon * kx) across++;
    }
    g.seg_flags[(size_t)k] = across > 8;
  }
}

// the staged kernels: their work list (eu_render4.hip: chunk counters of the persistent kernel, lists of the
// tiles left to the direct-gather kernel that follows it on the same stream) and its order between streams
int launch_staged(const eu_render_params *p, const eu_switches &sw, hipStream_t st, int *launches)
{
  // (more tiles than the work list has ids for: eu_staged_covers said no, and eu_select_path never names this path)
  const unsigned long long ntiles = eu_staged_tiles(p->width, p->row_begin, p->row_end);
  if (ntiles > EU4_WL_MAX_TILES) return -2;
  // every tile of the launch may be listed: the capacity holds for all of them (eu_worklist.h). A buffer that grows
  // starts with an empty header - the entries need no clearing, the counters say how many of them count - and a
  // smaller job behind a larger one finds the lists emptied by the larger one's last workgroup
  const size_t need = eu_render4_worklist_ints((size_t)ntiles);
  if (g.wl.cap < need) {
    if (g.wl_pair.host_wait() != hipSuccess || g.wl.reserve(need) != hipSuccess) return -1;
    if (hipMemsetAsync(g.wl.p, 0, eu_render4_worklist_header_ints() * sizeof(int), st) != hipSuccess) { g.wl.cap = 0; return -1; }
  }
  eu_render_params q = *p;
  q.wl = g.wl.p;
  // the work list, the persistent kernel's queues and the cached plans belong to ONE launch pair at a time: `st` waits
  // for the pair before, the event moves behind this one - on any stream, for eu_hip_listed_tiles() the library's own too
  if (g.wl_pair.order_after(st) != hipSuccess) return -1;
  const int rc = eu_launch_render4(&q, &sw, g.h_row.data(), g.h_row.size(), g.plan_gen, st, launches);
  if (rc || !*launches) return rc;
  return g.wl_pair.note(st) != hipSuccess ? -1 : 0;
}

// the packed kernel, one launch per run of rows that want the same work layout (eu_select.h: eu_split_runs)
int launch_packed_runs(const eu_render_params *p, const eu_switches &sw, hipStream_t st, int *launches)
{
  refresh_seg_flags(p);
  const std::vector<eu_run> runs = eu_split_runs(g.seg_flags.data(), (int)g.seg_flags.size(), *p, sw.hybrid == 2);
  if (runs.empty()) { *launches = 1; return eu_launch_render2(p, &sw, st); }
  for (const eu_run &r : runs) {
    eu_render_params q = *p;
    q.row_begin = r.row_begin; q.row_end = r.row_end;
    q.out = p->out + (long long)(r.row_begin - p->row_begin) * p->out_stride;
    q.layout = r.layout;
    ++*launches;
    const int rc = eu_launch_render2(&q, &sw, st);
    if (rc) return rc;
  }
  return 0;
}

// the kernel eu_select_path() names for the job
int launch_render(const eu_render_params *p, const eu_switches &sw, hipStream_t st)
{
  eu_path path = eu_select_path(*p, sw);
  int rc = 0, n = 0;
  if (path == EU_PATH_STAGED) {
    rc = launch_staged(p, sw, st, &n);
    if (!rc && !n) path = eu_select_path(*p, sw, false);       // the plan says no (eu_staged_worth)
  }
  switch (path) {
    case EU_PATH_STAGED: break;
    case EU_PATH_PACKED_RUNS: rc = launch_packed_runs(p, sw, st, &n); break;
    case EU_PATH_PACKED: n = 1; rc = eu_launch_render2(p, &sw, st); break;
    case EU_PATH_GENERAL: n = 1; rc = eu_launch_render(p, st); break;
    case EU_PATH_GENERAL_DIRECT: {
      eu_render_params q = *p;
      q.direct = 1;                       // not the LDS-staged variant: it evaluates inline
      n = 1;
      rc = eu_launch_render(&q, st);
    }
  }
  g.launches += n;
  return rc;
}


// ---- PTO masks and lens crops on the device (eu_alpha.hip) ----------------------------------------

// the refusals of eu_hip_facet_alpha, for an eu_facet_edit; *asked: the edit changes anything at all
int check_edit(const eu_facet_edit *e, int nch, const char *who, bool *asked)
{
  const std::string w(who);
  *asked = false;
  if (!e) return EU_OK;
  if (e->npolygons < 0 || (e->npolygons > 0 && !e->polygons) || e->crop_kind < 0 || e->crop_kind > 2)
    return fail(EU_ERR_ARGUMENT, w + ": polygons / crop kind");
  for (int i = 0; i < e->npolygons; i++)
    if (e->polygons[i].n < 0 || (e->polygons[i].n > 0 && (!e->polygons[i].x || !e->polygons[i].y)))
      return fail(EU_ERR_ARGUMENT, w + ": polygon without vertices");
  if (e->pixel_channels < 1 || (e->pixel_channels != nch && e->pixel_channels != nch - 1))
    return fail(EU_ERR_ARGUMENT, w + ": pixel_channels must be the facet's nchannels or one less");
  *asked = e->npolygons > 0 || e->crop_kind != 0 || e->pixel_channels != nch;
  if (*asked && nch != 2 && nch != 4)
    return fail(EU_ERR_ARGUMENT, w + ": a masked or cropped facet has 2 or 4 channels (alpha last)");
  return EU_OK;
}

// the row plan of an edit (eu::facet_alpha_rows), uploaded into the context's plan buffer; fills p's tables
int upload_alpha_plan(const eu_facet_edit *e, int w, int h, eu_alpha_params *p)
{
  std::vector<eu::mask_polygon> ps;
  for (int i = 0; e && i < e->npolygons; i++) ps.push_back({ e->polygons[i].n, e->polygons[i].x, e->polygons[i].y });
  std::vector<int> plan, row_start, spans;
  try {
    eu::facet_alpha_rows(w, h, ps.data(), int(ps.size()), e ? e->crop_kind : 0, e ? e->crop_x0 : 0, e ? e->crop_x1 : 0,
                         e ? e->crop_y0 : 0, e ? e->crop_y1 : 0, plan, row_start, spans);
    plan.insert(plan.end(), row_start.begin(), row_start.end());
    plan.insert(plan.end(), spans.begin(), spans.end());
  } catch (...) { return fail(EU_ERR_MEMORY, "facet alpha: host memory"); }
  // an earlier edit may still read the buffer, on a caller's stream or on the library's own
  HIPCHK(g.alpha.host_wait());
  HIPCHK(hipStreamSynchronize(g.stream));
  HIPCHK(g.aplan.reserve(plan.size() + 2));
  HIPCHK(hipMemcpy(g.aplan.p, plan.data(), plan.size() * sizeof(int), hipMemcpyHostToDevice));
  p->keep = g.aplan.p;
  p->row_start = p->keep + size_t(h) * 2;
  p->spans = p->row_start + size_t(h) + 1;
  return EU_OK;
}

// ---- the load pipeline: pixels -> braced, prefiltered container ------------------------------------------

// where a loader's pixels come from
enum feed_kind {
  FEED_HOST_FLOATS,      // host floats at the facet's channel count, no edit: copied straight to the destination
  FEED_EDITED_FLOATS,    // floats on the host (staged on the device first) or on the device, through the edit
  FEED_SAMPLES           // 8- or 16-bit samples on the host (uploaded behind their tables) or on the device, decoded there
};
struct load_feed {
  feed_kind kind;
  const char *who;             // the entry point, as messages name it
  const void *data;            // the floats or the samples
  bool on_device;              // data lies in device memory
  int src_ch;                  // channels of data: the facet's, or one less
  const eu_facet_edit *edit;   // masks and crop (FEED_HOST_FLOATS: none)
  bool alter;                  // the edit's kernel runs: FEED_EDITED_FLOATS whenever the edit changes something (a gained
                               // channel too), FEED_SAMPLES for masks or a crop (the decoder writes a gained channel itself)
  const eu_samples *smp;       // FEED_SAMPLES: bits, byte order, tables
};

// One load pipeline with three feeds. Written once: the source and its container (source_bcs, new_source), the plane
// the pixels arrive in - the facet's window as the core of the container, or the stack of a cubemap's six faces in
// scratch -, the clearing of a flat container, the finish (cube build, or the prefilter full_sphere() picks), the one
// synchronisation, and the error precedence: the message the plan upload or a kernel launch set, then the HIP error,
// then "device set-up stage failed". The feed is all that differs. Host floats: one H2D copy into the plane (1-D
// into the faces, 2-D into the core), no staging, no kernel. Floats through the edit: host pixels are staged on the
// device at their own channel count; upload_alpha_plan + eu_launch_facet_alpha write the plane, or - an edit that
// changes nothing, pixels on the device - a 2-D D2D copy. Integer samples: both tables and, behind them, the samples
// of a host image go into one device block; eu_launch_decode writes the plane, or - with masks or a crop - a dense
// buffer that eu_launch_facet_alpha then reads. Scratch is freed by scope, after the synchronisation.
// The entry points make their own argument checks, in their own order, and find the device (ensure_init).
int load_source(const eu_facet *fct, int spline_degree, int prefilter_degree, int support_min, int tile_size,
                const load_feed &feed, eu_source **out)
{
  int rc, bc0, bc1;
  source_bcs(fct, &bc0, &bc1);
  eu_source *s = nullptr;
  if ((rc = new_source(fct, spline_degree, bc0, bc1, support_min, tile_size, &s))) return rc;
  const std::string who(feed.who);
  const int nch = s->nch, src_ch = feed.src_ch, iir_stream = eu_read_switches().iir_stream;
  const bool cube = eu_cube_source(fct->projection);
  eu::metrics m {};
  if (cube) m = eu::make_metrics(fct->width, fct->hfov, support_min, tile_size);
  const eu_container &gm = s->geom;
  const int w = cube ? int(m.face_px) : int(gm.core[0]), h = cube ? int(6 * m.face_px) : int(gm.core[1]);
  const size_t npix = size_t(w) * size_t(h);
  eu_dev_tmp<float> staged, faces;   // floats in front of the edit, at src_ch channels; the faces of a cubemap
  eu_dev_tmp<char> block;            // samples: both tables and, behind them, the samples of a host image, as they are
  std::vector<float> tabs;
  const void *src = feed.data;
  hipError_t e = hipSuccess;
  int prc = 0;
  // what the feed brings to the device first
  if (feed.kind == FEED_SAMPLES) {
    const size_t ntab = size_t(1) << feed.smp->bits, nbytes = npix * size_t(src_ch) * size_t(feed.smp->bits / 8);
    try {
      tabs.assign(feed.smp->colour_table, feed.smp->colour_table + ntab);
      const float *at = feed.smp->alpha_table ? feed.smp->alpha_table : feed.smp->colour_table;
      tabs.insert(tabs.end(), at, at + ntab);
    } catch (...) { destroy_source(s); return fail(EU_ERR_MEMORY, who + ": host memory"); }
    const size_t tab_bytes = tabs.size() * sizeof(float);
    e = block.alloc(tab_bytes + (feed.on_device ? 0 : nbytes));
    if (e == hipSuccess) e = hipMemcpyAsync(block.p, tabs.data(), tab_bytes, hipMemcpyHostToDevice, g.stream);
    if (e == hipSuccess && !feed.on_device) {
      e = hipMemcpyAsync(block.p + tab_bytes, feed.data, nbytes, hipMemcpyHostToDevice, g.stream);
      src = block.p + tab_bytes;
    }
    if (e == hipSuccess && feed.alter) e = staged.alloc(npix * src_ch);
  } else if (feed.kind == FEED_EDITED_FLOATS && !feed.on_device) {
    e = staged.alloc(npix * src_ch);
    if (e == hipSuccess) e = hipMemcpyAsync(staged.p, feed.data, npix * src_ch * sizeof(float), hipMemcpyHostToDevice, g.stream);
    src = staged.p;
  }
  // the plane: w x h pixels of nch floats at dst, rows dst_pitch pixels apart
  if (e == hipSuccess && cube) e = faces.alloc(npix * nch);
  if (e == hipSuccess && !cube) e = hipMemsetAsync(s->dev, 0, s->nfloats * sizeof(float), g.stream);
  float *dst = cube ? faces.p : s->dev + ((size_t)gm.left[1] * gm.shape[0] + gm.left[0]) * nch;
  const size_t dst_pitch = cube ? size_t(w) : size_t(gm.shape[0]);
  const size_t row_bytes = size_t(w) * nch * sizeof(float), pitch_bytes = dst_pitch * nch * sizeof(float);
  if (e == hipSuccess) {
    eu_alpha_params p {};            // the edit, where it runs: src (src_ch channels, dense) -> the plane
    p.src = static_cast<const float *>(src); p.dst = dst;
    p.src_pitch = size_t(w); p.dst_pitch = dst_pitch;
    p.w = w; p.h = h; p.nch = nch; p.src_ch = src_ch;
    if (feed.kind == FEED_HOST_FLOATS) {
      e = cube ? hipMemcpyAsync(dst, src, npix * nch * sizeof(float), hipMemcpyHostToDevice, g.stream)
               : hipMemcpy2DAsync(dst, pitch_bytes, src, row_bytes, row_bytes, size_t(h), hipMemcpyHostToDevice, g.stream);
    } else if (feed.kind == FEED_EDITED_FLOATS) {
      if (!feed.alter)
        e = hipMemcpy2DAsync(dst, pitch_bytes, src, row_bytes, row_bytes, size_t(h), hipMemcpyDeviceToDevice, g.stream);
    } else {
      // samples -> floats: straight into the plane, or into the dense buffer the edit reads as it reads
      // pixels_on_device input (the channel a facet gains is then the edit's work)
      eu_decode_params d {};
      d.src = src; d.tables = reinterpret_cast<const float *>(block.p);
      d.dst = feed.alter ? staged.p : dst;
      d.dst_pitch = feed.alter ? size_t(w) : dst_pitch;
      d.w = w; d.h = h; d.bits = feed.smp->bits; d.big_endian = feed.smp->big_endian != 0;
      d.nch = feed.alter ? src_ch : nch; d.src_ch = src_ch;
      if (eu_launch_decode(&d, g.stream)) prc = fail(EU_ERR_NO_DEVICE, who + ": kernel launch failed");
      if (feed.alter) p.src = staged.p;
    }
    if (feed.alter && !prc) {
      prc = upload_alpha_plan(feed.edit, w, h, &p);
      if (!prc && eu_launch_facet_alpha(&p, g.stream)) prc = fail(EU_ERR_NO_DEVICE, who + ": kernel launch failed");
    }
  }
  // the finish: the IR image of a cubemap from its faces, or prefilter + brace of the container (a core narrower
  // than the spline's frame on an axis is braced slice by slice in zimt's order, eu_setup.hip: brace_seq_kernel)
  if (e == hipSuccess && !prc)
    rc = cube ? eu_launch_cubemap_build(faces.p, s->dev, nch, m.face_px, m.section_px, m.left_frame_px, m.right_frame_px,
                                        m.refc_md, m.model_to_px, prefilter_degree, iir_stream, g.stream)
              : eu_launch_prefilter(s->dev, &s->geom, nch, bc0, bc1, prefilter_degree, full_sphere(fct), iir_stream, g.stream);
  const hipError_t e2 = hipStreamSynchronize(g.stream);
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess || rc || prc) {
    destroy_source(s);
    if (prc) return prc;           // the plan's upload or a kernel launch: the message is set
    if (e != hipSuccess) return fail(EU_ERR_NO_DEVICE, hipGetErrorString(e));
    return fail(rc, "device set-up stage failed");
  }
  *out = s;
  return EU_OK;
}

// mean GPU time of `iters` calls of once() on g.stream between two events, after one untimed call (which builds
// whatever the first call builds: a plan's tables, derived copies)
template <class F> int time_on_stream(F once, int iters, float *mean_ms)
{
  int rc;
  if ((rc = once())) return rc;
  struct events {
    hipEvent_t a = nullptr, b = nullptr;
    ~events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  } ev;
  HIPCHK(hipEventCreate(&ev.a));
  HIPCHK(hipEventCreate(&ev.b));
  HIPCHK(hipEventRecord(ev.a, g.stream));
  for (int i = 0; i < iters; i++)
    if ((rc = once())) return rc;
  HIPCHK(hipEventRecord(ev.b, g.stream));
  HIPCHK(hipEventSynchronize(ev.b));
  float ms = 0.0f;
  HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
  *mean_ms = ms / iters;
  return EU_OK;
}

}  // namespace

extern "C" {

const char *eu_hip_last_error(void) { return g_err.c_str(); }

int eu_hip_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int eu_hip_init(int device)
{
  int n = eu_hip_device_count();
  if (n <= 0) return fail(EU_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
  if (device < 0 || device >= n) return fail(EU_ERR_ARGUMENT, "device index out of range");
  if (g.device == device) return EU_OK;
  // one device per process (one process per GPU): the stream, the LUT, the plan tables and
  // every resident source live on the device chosen first
  if (g.device >= 0)
    return fail(EU_ERR_ARGUMENT, "the library is already initialised on another device");
  return init_device(device);
}

int eu_hip_get_extent(int prj, int w, int h, double hfov, double *e)
{
  if (!e || prj < 0 || prj > EU_BIATAN6) return fail(EU_ERR_ARGUMENT, "bad projection");
  eu::get_extent(prj, w, h, hfov, e);
  return EU_OK;
}

double eu_hip_get_step(int prj, int w, int h, double hfov) { return eu::get_step(prj, w, h, hfov); }

int eu_hip_make_spread(int w, int h, float d, float sigma, float threshold, float *taps, int max_taps)
{
  std::vector<float> v;
  int n = eu::make_spread(w, h, d, sigma, threshold, v);
  if (n > max_taps) return fail(EU_ERR_ARGUMENT, "tap buffer too small");
  memcpy(taps, v.data(), v.size() * sizeof(float));
  return n;
}

int eu_hip_facet_alpha(float *pixels, int width, int height, int nchannels, const eu_mask_polygon *polygons,
                       int npolygons, int crop_kind, int crop_x0, int crop_x1, int crop_y0, int crop_y1,
                       float *alpha_out)
{
  if (width <= 0 || height <= 0 || (nchannels != 2 && nchannels != 4) || (!pixels && !alpha_out))
    return fail(EU_ERR_ARGUMENT, "facet_alpha: width x height x {2, 4} channels");
  if (npolygons < 0 || (npolygons > 0 && !polygons) || crop_kind < 0 || crop_kind > 2)
    return fail(EU_ERR_ARGUMENT, "facet_alpha: polygons / crop kind");
  std::vector<eu::mask_polygon> ps;
  for (int i = 0; i < npolygons; i++) {
    if (polygons[i].n < 0 || (polygons[i].n > 0 && (!polygons[i].x || !polygons[i].y)))
      return fail(EU_ERR_ARGUMENT, "facet_alpha: polygon without vertices");
    ps.push_back({ polygons[i].n, polygons[i].x, polygons[i].y });
  }
  std::vector<float> alpha;
  try { alpha.resize(size_t(width) * height); } catch (...) { return fail(EU_ERR_MEMORY, "facet_alpha: host memory"); }
  eu::facet_alpha(alpha.data(), width, height, ps.data(), int(ps.size()), crop_kind, crop_x0, crop_x1, crop_y0, crop_y1);
  if (pixels)
    eu::parallel_rows(height, [&](int y0, int y1) {
      for (size_t i = size_t(y0) * width; i < size_t(y1) * width; i++)
        for (int c = 0; c < nchannels; c++) pixels[i * nchannels + c] = pixels[i * nchannels + c] * alpha[i];
    });
  if (alpha_out) memcpy(alpha_out, alpha.data(), alpha.size() * sizeof(float));
  return EU_OK;
}

int eu_hip_cubemap_metrics(int face_px, double face_fov, int support_min, int tile_px,
                           int64_t *section_px, int64_t *left_frame_px, double *refc_md,
                           double *model_to_px)
{
  if (face_px <= 0 || tile_px <= 0 || (tile_px & (tile_px - 1)) || face_fov < M_PI_2 - 1e-12)
    return fail(EU_ERR_ARGUMENT, "bad cubemap metrics arguments");
  eu::metrics m = eu::make_metrics(face_px, face_fov, support_min, tile_px);
  if (section_px) *section_px = m.section_px;
  if (left_frame_px) *left_frame_px = m.left_frame_px;
  if (refc_md) *refc_md = m.refc_md;
  if (model_to_px) *model_to_px = m.model_to_px;
  return EU_OK;
}

int eu_hip_container_geometry(int degree, int bc0, int bc1, int64_t w, int64_t h, eu_container *out)
{
  if (!out || degree < 0 || degree > EU_MAX_DEGREE || w <= 0 || h <= 0)
    return fail(EU_ERR_ARGUMENT, "bad container geometry arguments");
  eu::container_geometry(degree, bc0, bc1, w, h, out);
  return EU_OK;
}

int eu_hip_source_adopt(const eu_facet *fct, const float *container, int spline_degree,
                        int bc0, int bc1, int support_min, int tile_size, eu_source **out)
{
  int rc;
  if ((rc = ensure_init())) return rc;
  if ((rc = check_facet(fct))) return rc;
  if (!container || !out) return fail(EU_ERR_ARGUMENT, "null argument");
  eu_source *s = nullptr;
  if ((rc = new_source(fct, spline_degree, bc0, bc1, support_min, tile_size, &s))) return rc;
  hipError_t e = hipMemcpy(s->dev, container, s->nfloats * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) { destroy_source(s); return fail(EU_ERR_NO_DEVICE, hipGetErrorString(e)); }
  *out = s;
  return EU_OK;
}

int eu_hip_source_load(const eu_facet *fct, const float *pixels, int spline_degree,
                       int prefilter_degree, int support_min, int tile_size, eu_source **out)
{
  int rc;
  if ((rc = ensure_init())) return rc;
  if ((rc = check_facet(fct))) return rc;
  if (!pixels || !out) return fail(EU_ERR_ARGUMENT, "null argument");
  if (prefilter_degree < 0 || prefilter_degree > EU_MAX_DEGREE)
    return fail(EU_ERR_ARGUMENT, "prefilter degree out of range");
  const load_feed feed { FEED_HOST_FLOATS, "source_load", pixels, false, fct->nchannels, nullptr, false, nullptr };
  return load_source(fct, spline_degree, prefilter_degree, support_min, tile_size, feed, out);
}

int eu_hip_facet_alpha_rows(int width, int height, const eu_mask_polygon *polygons, int npolygons, int crop_kind,
                            int crop_x0, int crop_x1, int crop_y0, int crop_y1, int32_t *keep, int32_t *row_start,
                            int32_t *spans, int max_spans)
{
  if (width <= 0 || height <= 0) return fail(EU_ERR_ARGUMENT, "facet_alpha_rows: empty image");
  if (npolygons < 0 || (npolygons > 0 && !polygons) || crop_kind < 0 || crop_kind > 2)
    return fail(EU_ERR_ARGUMENT, "facet_alpha_rows: polygons / crop kind");
  std::vector<eu::mask_polygon> ps;
  for (int i = 0; i < npolygons; i++) {
    if (polygons[i].n < 0 || (polygons[i].n > 0 && (!polygons[i].x || !polygons[i].y)))
      return fail(EU_ERR_ARGUMENT, "facet_alpha_rows: polygon without vertices");
    ps.push_back({ polygons[i].n, polygons[i].x, polygons[i].y });
  }
  std::vector<int> k, r, sp;
  try {
    eu::facet_alpha_rows(width, height, ps.data(), int(ps.size()), crop_kind, crop_x0, crop_x1, crop_y0, crop_y1, k, r, sp);
  } catch (...) { return fail(EU_ERR_MEMORY, "facet_alpha_rows: host memory"); }
  const size_t n = sp.size() / 2;
  if (n > size_t(INT32_MAX)) return fail(EU_ERR_UNSUPPORTED, "facet_alpha_rows: too many spans");
  if (keep) memcpy(keep, k.data(), k.size() * sizeof(int32_t));
  if (row_start) memcpy(row_start, r.data(), r.size() * sizeof(int32_t));
  if (spans) {
    if (max_spans < 0 || n > size_t(max_spans)) return fail(EU_ERR_ARGUMENT, "facet_alpha_rows: span buffer too small");
    if (n) memcpy(spans, sp.data(), sp.size() * sizeof(int32_t));
  }
  return int(n);
}

int eu_hip_facet_alpha_dev(void *pixels_dev, int width, int height, int nchannels, const eu_facet_edit *edit,
                           float *alpha_out_dev, void *stream)
{
  if (width <= 0 || height <= 0 || (nchannels != 2 && nchannels != 4) || (!pixels_dev && !alpha_out_dev))
    return fail(EU_ERR_ARGUMENT, "facet_alpha_dev: width x height x {2, 4} channels");
  bool asked;
  int rc;
  if ((rc = check_edit(edit, nchannels, "facet_alpha_dev", &asked))) return rc;
  if (edit && edit->pixel_channels != nchannels)
    return fail(EU_ERR_ARGUMENT, "facet_alpha_dev: an edit in place keeps the channel count");
  if ((rc = ensure_init())) return rc;
  eu_alpha_params p {};
  if ((rc = upload_alpha_plan(edit, width, height, &p))) return rc;
  p.src = p.dst = static_cast<float *>(pixels_dev);
  p.alpha_out = alpha_out_dev;
  p.src_pitch = p.dst_pitch = size_t(width);
  p.w = width; p.h = height; p.nch = p.src_ch = nchannels;
  hipStream_t st = stream ? (hipStream_t)stream : g.stream;
  if (eu_launch_facet_alpha(&p, st)) return fail(EU_ERR_NO_DEVICE, "facet_alpha_dev: kernel launch failed");
  return note_caller(g.alpha, stream, EU_OK);
}

int eu_hip_source_load_edited(const eu_facet *fct, const void *pixels, const eu_facet_edit *edit, int spline_degree,
                              int prefilter_degree, int support_min, int tile_size, eu_source **out)
{
  int rc;
  if ((rc = check_facet(fct))) return rc;
  if (!pixels || !out) return fail(EU_ERR_ARGUMENT, "null argument");
  if (spline_degree < 0 || spline_degree > EU_MAX_DEGREE) return fail(EU_ERR_ARGUMENT, "spline degree out of range");
  if (prefilter_degree < 0 || prefilter_degree > EU_MAX_DEGREE)
    return fail(EU_ERR_ARGUMENT, "prefilter degree out of range");
  bool asked;
  if ((rc = check_edit(edit, fct->nchannels, "source_load_edited", &asked))) return rc;
  const bool on_device = edit && edit->pixels_on_device;
  if (!asked && !on_device)
    return eu_hip_source_load(fct, static_cast<const float *>(pixels), spline_degree, prefilter_degree, support_min,
                              tile_size, out);
  if ((rc = ensure_init())) return rc;
  const load_feed feed { FEED_EDITED_FLOATS, "source_load_edited", pixels, on_device, edit->pixel_channels, edit, asked, nullptr };
  return load_source(fct, spline_degree, prefilter_degree, support_min, tile_size, feed, out);
}

int eu_hip_source_load_samples(const eu_facet *fct, const eu_samples *smp, const eu_facet_edit *edit, int spline_degree,
                               int prefilter_degree, int support_min, int tile_size, eu_source **out)
{
  int rc;
  if ((rc = check_facet(fct))) return rc;
  if (!smp || !smp->data || !out) return fail(EU_ERR_ARGUMENT, "null argument");
  if (smp->bits != 8 && smp->bits != 16) return fail(EU_ERR_ARGUMENT, "source_load_samples: bits must be 8 or 16");
  if (!smp->colour_table) return fail(EU_ERR_ARGUMENT, "source_load_samples: null colour table");
  // the edit as given, with the samples' channel count in place of its own
  eu_facet_edit ed {};
  if (edit) ed = *edit;
  ed.pixel_channels = smp->pixel_channels;
  ed.pixels_on_device = 0;
  bool asked;
  if ((rc = check_edit(&ed, fct->nchannels, "source_load_samples", &asked))) return rc;
  if (smp->on_device && smp->bits == 16 && reinterpret_cast<uintptr_t>(smp->data) % 2)
    return fail(EU_ERR_ARGUMENT, "source_load_samples: 16-bit samples on the device lie at an even address");
  if (spline_degree < 0 || spline_degree > EU_MAX_DEGREE) return fail(EU_ERR_ARGUMENT, "spline degree out of range");
  if (prefilter_degree < 0 || prefilter_degree > EU_MAX_DEGREE)
    return fail(EU_ERR_ARGUMENT, "prefilter degree out of range");
  if ((rc = ensure_init())) return rc;
  const bool edited = ed.npolygons > 0 || ed.crop_kind != 0;     // the alpha plane is wanted, not only the new channel
  const load_feed feed { FEED_SAMPLES, "source_load_samples", smp->data, smp->on_device != 0, smp->pixel_channels, &ed, edited, smp };
  return load_source(fct, spline_degree, prefilter_degree, support_min, tile_size, feed, out);
}

int eu_hip_source_alloc(const eu_facet *fct, int spline_degree, int support_min, int tile_size,
                        eu_source **out)
{
  int rc;
  if ((rc = ensure_init())) return rc;
  if ((rc = check_facet(fct))) return rc;
  if (!out) return fail(EU_ERR_ARGUMENT, "null argument");
  int bc0, bc1;
  source_bcs(fct, &bc0, &bc1);
  return new_source(fct, spline_degree, bc0, bc1, support_min, tile_size, out);
}

int eu_hip_source_update_facet(eu_source *src, const eu_facet *fct)
{
  int rc;
  if (!src) return fail(EU_ERR_HANDLE, "null source");
  if ((rc = check_facet(fct))) return rc;
  const eu_facet &o = src->fct;
  // what the resident container was built from stays as it is
  if (fct->projection != o.projection || fct->nchannels != o.nchannels || fct->width != o.width ||
      fct->height != o.height || fct->window_width != o.window_width || fct->window_height != o.window_height)
    return fail(EU_ERR_ARGUMENT, "the facet's image (projection, size, channels) differs from the resident one");
  if (eu_cube_source(o.projection) && fct->hfov != o.hfov)
    return fail(EU_ERR_ARGUMENT, "a cubemap's field of view is part of its resident image");
  const eu_src_dev keep = src->sd;
  src->fct = *fct;
  fill_src_dev(src);
  if (eu_cube_source(o.projection)) {
    src->sd.refc_md = keep.refc_md; src->sd.model_to_px = keep.model_to_px; src->sd.section_px = keep.section_px;
  }
  return EU_OK;
}

int eu_hip_source_device_ptr(const eu_source *src, void **dev_ptr, size_t *nfloats)
{
  if (!src) return fail(EU_ERR_HANDLE, "null source");
  if (dev_ptr) *dev_ptr = src->dev;
  if (nfloats) *nfloats = src->nfloats;
  return EU_OK;
}

int eu_hip_source_download(const eu_source *src, float *container, size_t nfloats)
{
  if (!src || !container) return fail(EU_ERR_HANDLE, "null argument");
  if (nfloats != src->nfloats) return fail(EU_ERR_ARGUMENT, "container size mismatch");
  HIPCHK(hipMemcpy(container, src->dev, nfloats * sizeof(float), hipMemcpyDeviceToHost));
  return EU_OK;
}

int eu_hip_source_info(const eu_source *src, eu_container *geom, int *nch)
{
  if (!src) return fail(EU_ERR_HANDLE, "null source");
  if (geom) *geom = src->geom;
  if (nch) *nch = src->nch;
  return EU_OK;
}

int eu_hip_source_release(eu_source *src)
{
  if (!src) return EU_OK;
  for (int k = 0; k < EU_MAX_SLOTS; k++) destroy_source(src->replica[k]);
  destroy_source(src);
  return EU_OK;
}

// `st` is about to use the frame buffer or the step tables, rewriting them or behind a rewrite: it goes behind every
// earlier job that uses them. On a caller's stream such a job left an event - a render in g.tables, eu_hip_encode_samples
// in g.encode. The library's own stream leaves none: a caller's stream waits for it by handle, once per change of sides.
static int order_encoders(hipStream_t st)
{
  if (st == g.stream) g.encode_own = true;
  else if (g.encode_own) { HIPCHK(hipStreamSynchronize(g.stream)); g.encode_own = false; }
  HIPCHK(g.tables.order_after(st));
  HIPCHK(g.encode.order_after(st));
  return EU_OK;
}

// one job, everything on the device: float pixels straight into out_dev, or float pixels into the library's
// frame buffer followed by a post-pass that writes out_dev - tethered, the to_screen_t pass and its packed words;
// with `enc` (its tables are in g.esteps: upload_steps), the encode to integer samples
static int render_on_device(const eu_target *trg, eu_source *const *srcs, int nsrc, float *out_dev,
                            size_t stride_bytes, const eu_switches &sw, hipStream_t st, const eu_encode *enc = nullptr)
{
  int rc;
  const bool multi = nsrc > 1;
  const bool screen = trg->out_format == EU_OUT_SRGBA8;
  eu_target tf = *trg;
  float *fout = out_dev;
  size_t fstride = stride_bytes;
  const size_t rows = (size_t)(trg->row_end - trg->row_begin);
  if (screen || enc) {
    if (screen && !g.lut) return fail(EU_ERR_NO_DEVICE, "sRGB table missing: library not initialised");
    // a post-pass queued on another stream may still read the frame buffer (upload_steps has ordered `st` where enc is set)
    if (screen && (rc = order_encoders(st))) return rc;
    tf.out_format = EU_OUT_FLOAT;
    fstride = (size_t)frame_w(trg) * trg->nchannels * sizeof(float);
    if (g.scr.cap < rows * frame_w(trg) * trg->nchannels) HIPCHK(g.tables.host_wait());      // reserve() will free it
    HIPCHK(g.scr.reserve(rows * frame_w(trg) * trg->nchannels));
    fout = g.scr.p;
  }
  if (multi) {
    eu_multi_params mp;
    int mdeg = 0;
    if ((rc = build_multi(&tf, srcs, nsrc, fout, fstride, sw, &mp, &mdeg))) return rc;
    if (eu_launch_render_multi(&mp, mdeg, st)) return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
  } else {
    eu_render_params p;
    if ((rc = build_params(&tf, srcs, nsrc, fout, fstride, sw, &p))) return rc;
    if (launch_render(&p, sw, st)) return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
  }
  if (screen &&
      eu_launch_to_screen(fout, (long long)(fstride / sizeof(float)), (unsigned *)out_dev,
                          (long long)(stride_bytes / sizeof(unsigned)), frame_w(trg), (int)rows,
                          trg->nchannels, g.lut, st))
    return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
  if (enc && rows) {
    eu_encode_params ep {};
    ep.src = fout; ep.src_stride_bytes = fstride;
    ep.dst = out_dev; ep.dst_stride_bytes = stride_bytes;
    ep.tables = g.esteps.p;
    ep.w = frame_w(trg); ep.h = (int)rows; ep.nch = trg->nchannels;
    ep.bits = enc->bits; ep.big_endian = enc->big_endian;
    if (eu_launch_encode(&ep, st)) return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
  }
  return EU_OK;
}

// ---- integer samples on the way out (eu_encode.hip) -------------------------------------------------------------
// a step table as eu_hip.h defines it: steps[1 .. m] free of NaN and non-decreasing, m >= 1, NaN behind m
static int check_steps(const float *s, int bits, const char *who, const char *which)
{
  const int n = 1 << bits;
  const std::string head = std::string(who) + ": " + which + " steps: ";
  if (std::isnan(s[1])) return fail(EU_ERR_ARGUMENT, head + "entry 1 is NaN, a table has at least one code above 0");
  int m = 1;
  for (; m + 1 < n && !std::isnan(s[m + 1]); m++)
    if (s[m + 1] < s[m]) return fail(EU_ERR_ARGUMENT, head + "entry " + std::to_string(m + 1) + " is smaller than the one before it");
  for (int k = m + 1; k < n; k++)
    if (!std::isnan(s[k]))
      return fail(EU_ERR_ARGUMENT, head + "entry " + std::to_string(k) + " is a number behind the NaN at entry " + std::to_string(m + 1));
  return EU_OK;
}

// what both sample entry points ask of `enc` and `out`: rows of `width` pixels of `nch` samples
static int check_encode(const char *who, const eu_encode *enc, int width, int nch, const void *out, size_t out_row_stride_bytes)
{
  const std::string head = std::string(who) + ": ";
  if (!enc || !out) return fail(EU_ERR_ARGUMENT, head + "null argument");
  if (enc->bits != 8 && enc->bits != 16) return fail(EU_ERR_ARGUMENT, head + "bits must be 8 or 16");
  if (!enc->colour_steps) return fail(EU_ERR_ARGUMENT, head + "null colour steps");
  if (nch < 1 || nch > 4) return fail(EU_ERR_ARGUMENT, head + "channels must be 1..4");
  if (width < 0 || (size_t)width * nch > (size_t(1) << 28)) return fail(EU_ERR_ARGUMENT, head + "rows of 0 .. 2^28 samples");
  if (out_row_stride_bytes < (size_t)width * nch * (enc->bits / 8)) return fail(EU_ERR_ARGUMENT, head + "row stride smaller than a row");
  if (enc->bits == 16 && (reinterpret_cast<uintptr_t>(out) % 2 || out_row_stride_bytes % 2))
    return fail(EU_ERR_ARGUMENT, head + "16-bit samples lie at even addresses: out and its row stride are multiples of 2");
  int rc;
  if ((rc = check_steps(enc->colour_steps, enc->bits, who, "colour"))) return rc;
  if (enc->alpha_steps && (rc = check_steps(enc->alpha_steps, enc->bits, who, "alpha"))) return rc;
  return EU_OK;
}

// The tables of `enc` into g.esteps, in front of the work this call queues on `st`. The buffers of the sample entry
// points (tables, frame buffer) are about to be used on `st`: it goes behind the calls that used them before
// (order_encoders). The upload reads the library's own host copy, never the caller's memory; tables equal to the last
// ones are not sent again.
static int upload_steps(const eu_encode *enc, hipStream_t st)
{
  { int rc = order_encoders(st); if (rc) return rc; }
  const size_t n = size_t(1) << enc->bits;
  const float *alpha = enc->alpha_steps ? enc->alpha_steps : enc->colour_steps;
  if (g.esteps.p && g.esteps_host.size() == 2 * n && !memcmp(g.esteps_host.data(), enc->colour_steps, n * sizeof(float)) &&
      !memcmp(g.esteps_host.data() + n, alpha, n * sizeof(float)))
    return EU_OK;
  // earlier work may still read the device tables, and their upload the host copy: `st` is behind all of it
  HIPCHK(hipStreamSynchronize(st));
  g.esteps_host.assign(enc->colour_steps, enc->colour_steps + n);
  g.esteps_host.insert(g.esteps_host.end(), alpha, alpha + n);
  hipError_t e = g.esteps.reserve(2 * n);
  if (e == hipSuccess) e = hipMemcpyAsync(g.esteps.p, g.esteps_host.data(), 2 * n * sizeof(float), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) {
    g.esteps_host.clear();
    return fail(EU_ERR_NO_DEVICE, std::string("step tables: ") + hipGetErrorString(e));
  }
  return EU_OK;
}

static int check_render_sources(const eu_target *trg, eu_source *const *srcs, int nsrc)
{
  if (nsrc > 1 && trg->stage) return fail(EU_ERR_ARGUMENT, "stage outputs exist for single-facet jobs only");
  for (int f = 0; f < nsrc; f++) {
    if (!srcs[f]) return fail(EU_ERR_HANDLE, "null source");
    // a masking job adapts channel counts with mono_t, which knows 1 and 2 output channels only
    // (environment.h:1339: the reference asserts)
    if (srcs[f]->fct.mask_paint && srcs[f]->nch != trg->nchannels && trg->nchannels > 2 && !trg->stage)
      return fail(EU_ERR_ARGUMENT, "--mask_for: facets whose channel count differs from the target's need a 1- or 2-channel target");
  }
  return EU_OK;
}

// The job of eu_hip_render and of eu_hip_render_samples behind their argument checks: `out` receives rows of
// row_bytes bytes - floats or packed words, or, with `enc`, integer samples.
static int render_frame(const eu_target *trg, eu_source *const *srcs, int nsrc, void *out, size_t row_bytes,
                        size_t out_row_stride_bytes, int out_on_device, void *stream, const eu_encode *enc)
{
  int rc;
  hipStream_t st = stream ? (hipStream_t)stream : g.stream;
  const eu_switches sw = eu_read_switches();
  if (enc && (rc = upload_steps(enc, st))) return rc;
  if (out_on_device)
    return note_caller(g.tables, stream, render_on_device(trg, srcs, nsrc, (float *)out, out_row_stride_bytes, sw, st, enc));
  const size_t rows = (size_t)(trg->row_end - trg->row_begin);
  if (!rows) return EU_OK;
  HIPCHK(g.stage.reserve((rows * row_bytes + sizeof(float) - 1) / sizeof(float)));
  // The frame goes to the host in up to four row chunks: every chunk is a launch of its own
  // on `st`, and its copy (second stream, behind the chunk's event) runs while the later
  // chunks render - the link (57 GB/s pinned, 21 ms for the 1.2 GB headline frame) is the
  // whole cost, the kernels hide under the first copy. Samples: the encode runs behind each chunk's render,
  // and the link carries a quarter or half of the bytes.
  const size_t nchunk = rows >= 1024 ? 4 : 1;
  if (!g.copy) HIPCHK(hipStreamCreateWithFlags(&g.copy, hipStreamNonBlocking));
  for (size_t c = 0; c < 4; c++)
    if (!g.chunk_done[c]) HIPCHK(hipEventCreateWithFlags(&g.chunk_done[c], hipEventDisableTiming));
  const size_t per = ((rows + nchunk - 1) / nchunk + 7) / 8 * 8;
  drain drain_on_exit{ g.copy, st };      // a host output leaves nothing behind on `st`
  for (size_t c = 0; c < nchunk; c++) {
    const size_t a = std::min(rows, c * per), b = std::min(rows, (c + 1) * per);
    if (a >= b) break;
    eu_target tc = *trg;
    tc.row_begin = trg->row_begin + (int)a;
    tc.row_end = trg->row_begin + (int)b;
    char *dst = (char *)g.stage.p + a * row_bytes;
    if ((rc = render_on_device(&tc, srcs, nsrc, (float *)dst, row_bytes, sw, st, enc))) return rc;
    HIPCHK(hipEventRecord(g.chunk_done[c], st));
    HIPCHK(hipStreamWaitEvent(g.copy, g.chunk_done[c], 0));
    HIPCHK(hipMemcpy2DAsync((char *)out + a * out_row_stride_bytes, out_row_stride_bytes, dst, row_bytes,
                            row_bytes, b - a, hipMemcpyDeviceToHost, g.copy));
  }
  HIPCHK(hipStreamSynchronize(g.copy));
  HIPCHK(hipStreamSynchronize(st));
  return EU_OK;
}

int eu_hip_render(const eu_target *trg, eu_source *const *srcs, int nsrc, float *out,
                  size_t out_row_stride_bytes, int out_on_device, void *stream)
{
  int rc;
  if ((rc = ensure_init())) return rc;
  if (!trg) return fail(EU_ERR_ARGUMENT, "null target");
  if (!srcs || nsrc < 1 || !out) return fail(EU_ERR_ARGUMENT, "no source / no output");
  if ((rc = check_target(trg))) return rc;
  // words per pixel: a packed sRGBA8 word, 3 floats of a stage output, or the channels
  const int och = trg->out_format == EU_OUT_SRGBA8 ? 1 : trg->stage ? 3 : trg->nchannels;
  const size_t min_stride = (size_t)frame_w(trg) * och * sizeof(float);
  if (out_row_stride_bytes < min_stride) return fail(EU_ERR_ARGUMENT, "row stride smaller than a row");
  if (out_row_stride_bytes % sizeof(float)) return fail(EU_ERR_ARGUMENT, "row stride must be a multiple of 4 bytes");
  if ((rc = check_render_sources(trg, srcs, nsrc))) return rc;
  return render_frame(trg, srcs, nsrc, out, min_stride, out_row_stride_bytes, out_on_device, stream, nullptr);
}

int eu_hip_render_samples(const eu_target *trg, eu_source *const *srcs, int nsrc, const eu_encode *enc, void *out,
                          size_t out_row_stride_bytes, int out_on_device, void *stream)
{
  int rc;
  if (!trg) return fail(EU_ERR_ARGUMENT, "render_samples: null target");
  if (!srcs || nsrc < 1 || !out) return fail(EU_ERR_ARGUMENT, "render_samples: no source / no output");
  if ((rc = check_target(trg))) return rc;
  if (trg->stage) return fail(EU_ERR_ARGUMENT, "render_samples: stage outputs are float only");
  if (trg->out_format != EU_OUT_FLOAT) return fail(EU_ERR_ARGUMENT, "render_samples: EU_OUT_SRGBA8 is a format of its own, not a frame to encode");
  if ((rc = check_encode("render_samples", enc, frame_w(trg), trg->nchannels, out, out_row_stride_bytes))) return rc;
  if ((rc = check_render_sources(trg, srcs, nsrc))) return rc;
  if ((rc = ensure_init())) return rc;
  if (trg->row_end == trg->row_begin) return EU_OK;
  const size_t row_bytes = (size_t)frame_w(trg) * trg->nchannels * (enc->bits / 8);
  return render_frame(trg, srcs, nsrc, out, row_bytes, out_row_stride_bytes, out_on_device, stream, enc);
}

// bytes (frame and samples together) of one staged chunk of an eu_hip_encode_samples call with a host buffer
#define EU_ENCODE_CHUNK_BYTES ((size_t)64 << 20)

int eu_hip_encode_samples(const float *frame, size_t frame_row_stride_bytes, int frame_on_device, int width, int height,
                          int nchannels, const eu_encode *enc, void *out, size_t out_row_stride_bytes, int out_on_device,
                          void *stream)
{
  int rc;
  if (!frame) return fail(EU_ERR_ARGUMENT, "encode_samples: null argument");
  if (height < 0) return fail(EU_ERR_ARGUMENT, "encode_samples: negative height");
  if ((rc = check_encode("encode_samples", enc, width, nchannels, out, out_row_stride_bytes))) return rc;
  const size_t in_row = (size_t)width * nchannels * sizeof(float), out_row = (size_t)width * nchannels * (enc->bits / 8);
  if (frame_row_stride_bytes < in_row) return fail(EU_ERR_ARGUMENT, "encode_samples: frame row stride smaller than a row");
  if (frame_row_stride_bytes % sizeof(float) || reinterpret_cast<uintptr_t>(frame) % sizeof(float))
    return fail(EU_ERR_ARGUMENT, "encode_samples: the frame and its row stride are multiples of 4 bytes");
  if (!width || !height) return EU_OK;
  if ((rc = ensure_init())) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : g.stream;
  if ((rc = upload_steps(enc, st))) return rc;
  eu_encode_params ep {};
  ep.tables = g.esteps.p;
  ep.w = width; ep.nch = nchannels; ep.bits = enc->bits; ep.big_endian = enc->big_endian;
  if (frame_on_device && out_on_device) {
    ep.src = frame; ep.src_stride_bytes = frame_row_stride_bytes;
    ep.dst = out; ep.dst_stride_bytes = out_row_stride_bytes;
    ep.h = height;
    if (eu_launch_encode(&ep, st)) return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
    return note_caller(g.encode, stream, EU_OK);
  }
  // A host buffer on either side: the rows go through in chunks of bounded size - copy in, encode, copy out, in
  // order on `st`; the call returns when `out` is complete
  const int ch = (int)std::min<size_t>((size_t)height, std::max<size_t>(1, EU_ENCODE_CHUNK_BYTES / (in_row + out_row)));
  if (!frame_on_device) HIPCHK(g.eframe.reserve((size_t)ch * width * nchannels));
  if (!out_on_device) HIPCHK(g.eout.reserve(((size_t)ch * out_row + 3) / 4));
  drain drain_on_exit{ st, st };
  for (int y0 = 0; y0 < height; y0 += ch) {
    const int h = std::min(ch, height - y0);
    const char *fin = (const char *)frame + (size_t)y0 * frame_row_stride_bytes;
    char *fout = (char *)out + (size_t)y0 * out_row_stride_bytes;
    ep.src = (const float *)fin; ep.src_stride_bytes = frame_row_stride_bytes;
    ep.dst = fout; ep.dst_stride_bytes = out_row_stride_bytes;
    ep.h = h;
    if (!frame_on_device) {
      ep.src = g.eframe.p; ep.src_stride_bytes = in_row;
      HIPCHK(hipMemcpy2DAsync(g.eframe.p, in_row, fin, frame_row_stride_bytes, in_row, (size_t)h, hipMemcpyHostToDevice, st));
    }
    if (!out_on_device) { ep.dst = g.eout.p; ep.dst_stride_bytes = out_row; }
    if (eu_launch_encode(&ep, st)) return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
    if (!out_on_device)
      HIPCHK(hipMemcpy2DAsync(fout, out_row_stride_bytes, g.eout.p, out_row, out_row, (size_t)h, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  return EU_OK;
}

// ---------------------------------------------------------------------------------------------------------
// one process, several devices (include/eu_hip.h)
// ---------------------------------------------------------------------------------------------------------
int eu_hip_device_slots(void) { return nslots_; }
int eu_current_slot(void) { return cur_slot_; }

int eu_hip_init_devices(const int *devices, int ndevices)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(EU_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
  if (!devices || ndevices < 1 || ndevices > EU_MAX_SLOTS) return fail(EU_ERR_ARGUMENT, "1 .. EU_MAX_SLOTS devices");
  for (int k = 0; k < ndevices; k++)
    if (devices[k] < 0 || devices[k] >= n) return fail(EU_ERR_ARGUMENT, "device index out of range");
  // slot 0 may already be initialised (sources exist on it): it keeps its device
  if (ctx_[0].device >= 0 && ctx_[0].device != devices[0])
    return fail(EU_ERR_ARGUMENT, "the library is already initialised on another device than devices[0]");
  for (int k = 1; k < nslots_; k++)
    if (k >= ndevices || ctx_[k].device != devices[k])
      return fail(EU_ERR_ARGUMENT, "device slots cannot be re-assigned once made");
  int rc = EU_OK;
  for (int k = 0; k < ndevices && !rc; k++) {
    cur_slot_ = k;
    if (ctx_[k].device < 0) rc = init_device(devices[k]);
    // peers: slot k reads slot 0's containers and slot 0 receives the strips (a no-op for the same device)
    if (!rc && devices[k] != devices[0]) {
      int can = 0;
      (void)hipDeviceCanAccessPeer(&can, devices[k], devices[0]);
      if (can) { hipError_t e = hipDeviceEnablePeerAccess(devices[0], 0); if (e != hipSuccess) (void)hipGetLastError(); }
    }
  }
  nslots_ = std::max(nslots_, ndevices);
  int rc2 = set_slot(0);
  return rc ? rc : rc2;
}

namespace {

// the source's copy on slot k (made on first use: one peer copy of the braced container)
int replica_of(eu_source *src, int k, eu_source **out)
{
  if (k == src->slot) { *out = src; return EU_OK; }
  if (!src->replica[k]) {
    eu_source *r = new (std::nothrow) eu_source(*src);
    if (!r) return fail(EU_ERR_NO_DEVICE, "out of host memory");
    for (int j = 0; j < EU_MAX_SLOTS; j++) r->replica[j] = nullptr;
    r->is_replica = true; r->slot = k; r->dev = nullptr;
    int rc = set_slot(k);
    if (rc) { delete r; return rc; }
    hipError_t e = hipMalloc((void **)&r->dev, src->nfloats * sizeof(float));
    if (e == hipSuccess) {
      if (ctx_[k].device == ctx_[src->slot].device)
        e = hipMemcpyAsync(r->dev, src->dev, src->nfloats * sizeof(float), hipMemcpyDeviceToDevice, g.stream);
      else
        e = hipMemcpyPeerAsync(r->dev, ctx_[k].device, src->dev, ctx_[src->slot].device, src->nfloats * sizeof(float), g.stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    if (e != hipSuccess) { destroy_source(r); return fail(EU_ERR_NO_DEVICE, hipGetErrorString(e)); }
    // the evaluator parameters are the original's (same geometry, same verified constants) on another base
    r->sd.base = r->dev + (src->sd.base - src->dev);
    src->replica[k] = r;
  } else if (memcmp(&src->replica[k]->fct, &src->fct, sizeof(eu_facet))) {
    // the facet's geometry changed since (eu_hip_source_update_facet): same container, new mount
    eu_source *r = src->replica[k];
    const float *base = r->sd.base;
    r->fct = src->fct; r->sd = src->sd; r->sd.base = base;
  }
  *out = src->replica[k];
  return EU_OK;
}

// contiguous strips of equal estimated cost: the segments the layout probe marks (source rows running across
// target rows: the polar faces of a cubemap made from a lat/lon image) cost ~1.6x the others with every kernel
void cost_strips(const eu_target *trg, eu_source *const *srcs, int nsrc, int n, int *begin, int *end)
{
  const int H = frame_h(trg);
  std::vector<unsigned char> flags((size_t)(H / EU_SEG_ROWS + 2), 0);
  int seg = EU_SEG_ROWS, nseg = 0;
  if (nsrc == 1) {
    nseg = eu_hip_layout_segments(trg, srcs, 1, flags.data(), (int)flags.size(), &seg);
    if (nseg < 0) nseg = 0;
  }
  auto cost_upto = [&](int y) {          // cost of rows [0, y)
    double c = 0.0;
    for (int k = 0; k * seg < y; k++) {
      const int a = k * seg, b = std::min(y, a + seg);
      c += (b - a) * ((k < nseg && flags[(size_t)k]) ? 1.6 : 1.0);
    }
    return c;
  };
  const double total = cost_upto(H);
  int prev = 0;
  for (int k = 0; k < n; k++) {
    int y = H;
    if (k + 1 < n) {
      const double want = total * (k + 1) / n;
      int lo = prev, hi = H;
      while (lo < hi) { const int mid = (lo + hi) / 2; if (cost_upto(mid) < want) lo = mid + 1; else hi = mid; }
      y = std::min(H, (lo + 15) / 16 * 16);          // whole 16-row tile rows (the staged kernel's pairs)
    }
    begin[k] = prev; end[k] = std::max(prev, y);
    prev = end[k];
  }
}

}  // namespace

int eu_hip_device_strips(const eu_target *trg, eu_source *const *srcs, int nsrc, int *begin, int *end)
{
  int rc;
  if ((rc = ensure_init())) return rc;
  if (!trg || !srcs || nsrc < 1 || !begin || !end) return fail(EU_ERR_ARGUMENT, "null argument");
  if ((rc = check_target(trg))) return rc;
  cost_strips(trg, srcs, nsrc, nslots_, begin, end);
  return EU_OK;
}

int eu_hip_render_devices(const eu_target *trg, eu_source *const *srcs, int nsrc, float *out,
                          size_t out_row_stride_bytes, int out_on_device)
{
  int rc;
  if ((rc = ensure_init())) return rc;
  if (nslots_ <= 1) return eu_hip_render(trg, srcs, nsrc, out, out_row_stride_bytes, out_on_device, nullptr);
  if (!trg || !srcs || nsrc < 1 || !out) return fail(EU_ERR_ARGUMENT, "no source / no output");
  if ((rc = check_target(trg))) return rc;
  if (trg->band_count > 1 || trg->row_begin != 0 || trg->row_end != frame_h(trg))
    return fail(EU_ERR_ARGUMENT, "eu_hip_render_devices renders whole frames (it does the tiling itself)");
  if (nsrc > 64) return fail(EU_ERR_UNSUPPORTED, "more than 64 facets over several devices");
  const int och = trg->out_format == EU_OUT_SRGBA8 ? 1 : trg->stage ? 3 : trg->nchannels;
  const size_t min_stride = (size_t)frame_w(trg) * och * sizeof(float);
  if (out_row_stride_bytes < min_stride || out_row_stride_bytes % sizeof(float))
    return fail(EU_ERR_ARGUMENT, "row stride smaller than a row / not a multiple of 4 bytes");
  int begin[EU_MAX_SLOTS], end[EU_MAX_SLOTS];
  cost_strips(trg, srcs, nsrc, nslots_, begin, end);
  const eu_switches sw = eu_read_switches();
  // every slot: its replicas, its strip into its own buffer, the strip's way to `out` behind it on the
  // slot's stream; the slots run concurrently, one host thread feeds them
  struct guard { ~guard() { for (int k = 0; k < nslots_; k++) { cur_slot_ = k; if (ctx_[k].device >= 0 && hipSetDevice(ctx_[k].device) == hipSuccess && ctx_[k].stream) (void)hipStreamSynchronize(ctx_[k].stream); } cur_slot_ = 0; if (ctx_[0].device >= 0) (void)hipSetDevice(ctx_[0].device); } } sync_all_on_exit;
  for (int k = 0; k < nslots_; k++) {
    if (end[k] <= begin[k]) continue;
    eu_source *reps[64];
    for (int f = 0; f < nsrc; f++) {
      if (!srcs[f]) return fail(EU_ERR_HANDLE, "null source");
      if ((rc = replica_of(srcs[f], k, &reps[f]))) return rc;
    }
    if ((rc = set_slot(k))) return rc;
    eu_target t = *trg;
    t.row_begin = begin[k]; t.row_end = end[k];
    const size_t rows = (size_t)(end[k] - begin[k]);
    const bool direct = out_on_device && ctx_[k].device == ctx_[0].device && out_row_stride_bytes == min_stride;
    float *dst = nullptr;
    if (direct) dst = out + (size_t)begin[k] * (min_stride / sizeof(float));
    else {
      HIPCHK(g.strip.reserve(rows * (min_stride / sizeof(float))));
      dst = g.strip.p;
    }
    if ((rc = render_on_device(&t, reps, nsrc, dst, min_stride, sw, g.stream))) return rc;
    if (!direct) {
      char *o = (char *)out + (size_t)begin[k] * out_row_stride_bytes;
      if (!out_on_device)
        HIPCHK(hipMemcpy2DAsync(o, out_row_stride_bytes, dst, min_stride, min_stride, rows, hipMemcpyDeviceToHost, g.stream));
      else if (ctx_[k].device == ctx_[0].device)
        HIPCHK(hipMemcpy2DAsync(o, out_row_stride_bytes, dst, min_stride, min_stride, rows, hipMemcpyDeviceToDevice, g.stream));
      else if (out_row_stride_bytes == min_stride)
        HIPCHK(hipMemcpyPeerAsync(o, ctx_[0].device, dst, ctx_[k].device, rows * min_stride, g.stream));
      else
        for (size_t r = 0; r < rows; r++)
          HIPCHK(hipMemcpyPeerAsync(o + r * out_row_stride_bytes, ctx_[0].device, (char *)dst + r * min_stride, ctx_[k].device, min_stride, g.stream));
    }
  }
  return EU_OK;      // the guard waits for every slot
}

// the layout choice per segment of the (cropped) frame for this job: flags[k] = 1 where
// rows [k * seg_rows, (k + 1) * seg_rows) render faster - and cost about 1.55x the others -
// with the tile layout; returns the number of segments (0: no lat/lon source / no table)
int eu_hip_layout_segments(const eu_target *trg, eu_source *const *srcs, int nsrc,
                           unsigned char *flags, int max_flags, int *seg_rows)
{
  int rc;
  if ((rc = ensure_init())) return rc;
  if (!trg || !srcs || nsrc != 1 || !srcs[0] || !flags) return fail(EU_ERR_ARGUMENT, "one source, flags buffer");
  eu_render_params p;
  eu_target t = *trg;
  t.band_rows = 0; t.band_count = 0; t.band_index = 0;
  t.row_begin = 0; t.row_end = frame_h(trg);
  float dummy;
  if ((rc = build_params(&t, srcs, 1, &dummy, (size_t)frame_w(trg) * t.nchannels * sizeof(float), eu_read_switches(), &p))) return rc;
  if (seg_rows) *seg_rows = EU_SEG_ROWS;
  if (p.twine || p.norm_mode != EU_NORM_NONE || p.src.prj != EU_SPHERICAL) return 0;
  refresh_seg_flags(&p);
  const int n = (int)g.seg_flags.size();
  if (n > max_flags) return fail(EU_ERR_ARGUMENT, "flags buffer too small");
  memcpy(flags, g.seg_flags.data(), (size_t)n);
  return n;
}

// render kernel launches of this process so far (a render step of a big cubic job is
// several: launch-level layout choice); lets a benchmark report launches per step
unsigned long long eu_hip_launch_count(void) { return g.launches; }

unsigned long long eu_hip_listed_tiles(void)
{
  // the direct-gather kernel's last workgroup leaves the sum of the lists' counters in the header; the event
  // behind the pair is the library's own (the caller's stream may be gone by now)
  int n = 0;
  if (!g.wl.p || !g.wl_pair.recorded || g.wl_pair.host_wait() != hipSuccess) return 0;
  if (hipMemcpy(&n, g.wl.p + EU4_WL_LISTED, sizeof n, hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return n > 0 ? (unsigned long long)n : 0ull;
}

int eu_hip_band_rows(int height, int band_rows, int band_count, int band_index)
{
  if (height < 0 || (band_count > 1 && (band_rows < 1 || band_index < 0 || band_index >= band_count))) return 0;
  return local_rows(height, band_rows, band_count, band_index);
}

// ---------------------------------------------------------------------------------------------------------
// `act` alone: a resident source evaluated at the caller's rays (include/eu_hip.h, eu_render_rays.hip)
// ---------------------------------------------------------------------------------------------------------

// everything that can be wrong with the arguments, found without a device
static int check_rays(const eu_rays *r, const eu_source *src, const float *out, size_t out_row_stride_bytes)
{
  if (!r || !src || !out || !r->rays) return fail(EU_ERR_ARGUMENT, "render_rays: null argument");
  if (r->ninputs != 3 && r->ninputs != 9)
    return fail(EU_ERR_ARGUMENT, "render_rays: ninputs is 3 (rays) or 9 (ninepacks)");
  if (r->ninputs == 3 && (r->ntaps != 0 || r->taps))
    return fail(EU_ERR_ARGUMENT, "render_rays: a tap table goes with ninepacks (ninputs 9) only");
  if (r->ninputs == 9 && (r->ntaps <= 0 || r->ntaps > EU_MAX_TAPS || !r->taps))
    return fail(EU_ERR_ARGUMENT, "render_rays: ninepacks need a tap table of 1 .. EU_MAX_TAPS taps");
  if (r->nchannels < 1 || r->nchannels > 4) return fail(EU_ERR_ARGUMENT, "render_rays: output channels must be 1..4");
  // as eu_hip_render: a masking source adapts channel counts with mono_t, which knows 1 and 2 output channels only
  if (src->fct.mask_paint && src->nch != r->nchannels && r->nchannels > 2)
    return fail(EU_ERR_ARGUMENT, "--mask_for: a facet whose channel count differs from the output's needs 1 or 2 output channels");
  if (r->width <= 0 || r->height <= 0) return fail(EU_ERR_ARGUMENT, "render_rays: empty ray array");
  if (r->ray_row_stride_bytes % sizeof(float) || out_row_stride_bytes % sizeof(float))
    return fail(EU_ERR_ARGUMENT, "render_rays: row strides must be multiples of 4 bytes");
  if (r->ray_row_stride_bytes < (size_t)r->width * r->ninputs * sizeof(float))
    return fail(EU_ERR_ARGUMENT, "render_rays: ray row stride smaller than a row");
  if (out_row_stride_bytes < (size_t)r->width * r->nchannels * sizeof(float))
    return fail(EU_ERR_ARGUMENT, "render_rays: output row stride smaller than a row");
  return EU_OK;
}

// the tap table on the device (biased_taps)
static int upload_ray_taps(const eu_rays *r)
{
  if (r->ninputs != 9) return EU_OK;
  std::vector<float> taps = biased_taps(r->taps, r->ntaps);
  if (g.rtaps.p && taps.size() == g.rtaps_host.size() &&
      !memcmp(taps.data(), g.rtaps_host.data(), taps.size() * sizeof(float)))
    return EU_OK;
  // an earlier call may still read the table, on a caller's stream or on the library's own
  HIPCHK(g.rays.host_wait());
  HIPCHK(hipStreamSynchronize(g.stream));
  g.rtaps_host.clear();
  HIPCHK(g.rtaps.reserve(taps.size()));
  HIPCHK(hipMemcpy(g.rtaps.p, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice));
  g.rtaps_host.swap(taps);
  return EU_OK;
}

// one launch: a w x h piece of the grid, both buffers on the device
static int launch_rays(const eu_rays *r, const eu_source *src, const eu_switches &sw, const float *rays_dev,
                       size_t ray_stride_bytes, float *out_dev, size_t out_stride_bytes, int w, int h, hipStream_t st)
{
  eu_rays_params p;
  memset(&p, 0, sizeof p);
  p.width = w; p.height = h;
  p.ninputs = r->ninputs; p.ntaps = r->ntaps;
  p.nch = src->nch; p.nch_out = r->nchannels;
  p.rays = rays_dev; p.ray_stride = (long long)(ray_stride_bytes / sizeof(float));
  p.taps = g.rtaps.p;
  p.out = out_dev; p.out_stride = (long long)(out_stride_bytes / sizeof(float));
  p.src = src->sd;
  if (eu_launch_render_rays(&p, eu_select_ray_path(p, sw), st)) return fail(EU_ERR_NO_DEVICE, "render_rays: kernel launch failed");
  return EU_OK;
}

// pixels (rays and their output together) of one staged chunk of a call with a host buffer
#define EU_RAYS_CHUNK_BYTES ((size_t)64 << 20)

int eu_hip_render_rays(const eu_rays *r, eu_source *src, float *out, size_t out_row_stride_bytes, int out_on_device,
                       void *stream)
{
  int rc;
  if ((rc = check_rays(r, src, out, out_row_stride_bytes))) return rc;
  if ((rc = ensure_init())) return rc;
  if (!src->dev) return fail(EU_ERR_HANDLE, "render_rays: the source has no container");
  const eu_switches sw = eu_read_switches();
  if ((rc = upload_ray_taps(r))) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : g.stream;
  if (r->rays_on_device && out_on_device)
    return note_caller(g.rays, stream, launch_rays(r, src, sw, r->rays, r->ray_row_stride_bytes, out, out_row_stride_bytes,
                                                   r->width, r->height, st));
  // A host buffer on either side: the grid goes through in chunks of rows - a flat list in chunks of its one
  // row - of bounded size, copy in, launch, copy out, all in order on `st`; the call returns when `out` is complete
  const size_t in_px = (size_t)r->ninputs * sizeof(float), out_px = (size_t)r->nchannels * sizeof(float);
  const bool flat = r->height == 1;
  const size_t px_per_chunk = std::max<size_t>(1, EU_RAYS_CHUNK_BYTES / (in_px + out_px));
  const int cw = flat ? (int)std::min<size_t>((size_t)r->width, px_per_chunk) : r->width;
  const int ch = flat ? 1 : (int)std::min<size_t>((size_t)r->height, std::max<size_t>(1, px_per_chunk / (size_t)r->width));
  if (!r->rays_on_device) HIPCHK(g.rstage.reserve((size_t)cw * ch * r->ninputs));
  if (!out_on_device) HIPCHK(g.stage.reserve((size_t)cw * ch * r->nchannels));
  drain drain_on_exit{ st, st };
  for (int y0 = 0; y0 < r->height; y0 += ch)
    for (int x0 = 0; x0 < r->width; x0 += cw) {
      const int w = std::min(cw, r->width - x0), h = std::min(ch, r->height - y0);
      const char *rin = (const char *)r->rays + (size_t)y0 * r->ray_row_stride_bytes + (size_t)x0 * in_px;
      char *rout = (char *)out + (size_t)y0 * out_row_stride_bytes + (size_t)x0 * out_px;
      const float *rays_dev = (const float *)rin;
      size_t rays_stride = r->ray_row_stride_bytes;
      if (!r->rays_on_device) {
        rays_dev = g.rstage.p; rays_stride = (size_t)w * in_px;
        HIPCHK(hipMemcpy2DAsync(g.rstage.p, rays_stride, rin, r->ray_row_stride_bytes, rays_stride, (size_t)h,
                                hipMemcpyHostToDevice, st));
      }
      float *out_dev = (float *)rout;
      size_t out_stride = out_row_stride_bytes;
      if (!out_on_device) { out_dev = g.stage.p; out_stride = (size_t)w * out_px; }
      if ((rc = launch_rays(r, src, sw, rays_dev, rays_stride, out_dev, out_stride, w, h, st))) return rc;
      if (!out_on_device)
        HIPCHK(hipMemcpy2DAsync(rout, out_row_stride_bytes, g.stage.p, out_stride, out_stride, (size_t)h,
                                hipMemcpyDeviceToHost, st));
    }
  HIPCHK(hipStreamSynchronize(st));
  return EU_OK;
}

int eu_hip_render_rays_timed(const eu_rays *r, eu_source *src, float *out_dev, size_t out_row_stride_bytes, int iters,
                             float *mean_ms)
{
  int rc;
  if ((rc = check_rays(r, src, out_dev, out_row_stride_bytes))) return rc;
  if (iters <= 0 || !mean_ms) return fail(EU_ERR_ARGUMENT, "bad iteration count");
  if (!r->rays_on_device) return fail(EU_ERR_ARGUMENT, "render_rays_timed: the rays lie in device memory");
  if ((rc = ensure_init())) return rc;
  if (!src->dev) return fail(EU_ERR_HANDLE, "render_rays: the source has no container");
  const eu_switches sw = eu_read_switches();
  if ((rc = upload_ray_taps(r))) return rc;
  auto once = [&]() {
    return launch_rays(r, src, sw, r->rays, r->ray_row_stride_bytes, out_dev, out_row_stride_bytes, r->width, r->height,
                       g.stream);
  };
  return time_on_stream(once, iters, mean_ms);
}

// ---------------------------------------------------------------------------------------------------------
// many views of one resident source in one call (include/eu_hip.h, eu_render_views.hip)
// ---------------------------------------------------------------------------------------------------------

// bytes of a host output that are staged on the device at a time (at least one view)
#define EU_VIEWS_STAGE_BYTES ((size_t)64 << 20)

static bool view_finite(const eu_view &v)
{
  return std::isfinite(v.yaw) && std::isfinite(v.pitch) && std::isfinite(v.roll) && std::isfinite(v.x0) &&
         std::isfinite(v.x1) && std::isfinite(v.y0) && std::isfinite(v.y1);
}

// everything that can be wrong with the shared target and the source, found without a device
static int check_views_target(const eu_target *t, const eu_source *src)
{
  if (!t || !src) return fail(EU_ERR_ARGUMENT, "render_views: null argument");
  { int rc0 = check_target(t); if (rc0) return rc0; }
  if (t->stage != 0) return fail(EU_ERR_ARGUMENT, "render_views: stage outputs belong to eu_hip_render");
  if (t->crop_w != 0) return fail(EU_ERR_ARGUMENT, "render_views: whole frames only, no crop window");
  if (t->band_count > 1) return fail(EU_ERR_ARGUMENT, "render_views: whole frames only, no row bands");
  if (t->single) return fail(EU_ERR_ARGUMENT, "render_views: a --single target belongs to eu_hip_render");
  if (t->out_format != EU_OUT_FLOAT) return fail(EU_ERR_ARGUMENT, "render_views: float output only");
  if (t->row_begin != 0 || t->row_end != t->height)
    return fail(EU_ERR_ARGUMENT, "render_views: whole frames only (row_begin 0, row_end height)");
  // as eu_hip_render: a masking source adapts channel counts with mono_t, which knows 1 and 2 output channels only
  if (src->fct.mask_paint && src->nch != t->nchannels && t->nchannels > 2)
    return fail(EU_ERR_ARGUMENT, "--mask_for: a facet whose channel count differs from the target's needs a 1- or 2-channel target");
  return EU_OK;
}

// eu_tanf has libm's bits for in-face coordinates up to 1.75 (eu_math.h); columns reach |x0|, |x1| plus the
// x bias, rows the in-face value of the first and the last row of every face plus the y bias
static int check_views_biatan6(const eu_target *t, const eu_view *views, int nviews)
{
  if (t->projection != EU_BIATAN6) return EU_OK;
  for (int k = 0; k < nviews; k++) {
    const eu_view &v = views[k];
    const float a0 = (float)v.x0, a1 = (float)v.x1, b0 = (float)v.y0, b1 = (float)v.y1;
    double m = std::max(std::fabs((double)a0), std::fabs((double)a1)) + 0.25 * std::fabs((double)a1 - a0) / t->width;
    const float section_md = a1 - a0, refc_md = (float)((a1 - a0) / 2.0);
    for (int face = 0; face < 6; face++)
      for (int e = 0; e < 2; e++)
        for (int b = 0; b < 2; b++) {
          const int y = face * t->width + (e ? t->width - 1 : 0);
          const float pp = eu::planar_row(t->height, b0, b1, b ? 0.25f : 0.0f, y) + (float)(3 - face) * section_md - refc_md;
          m = std::max(m, std::fabs((double)pp));
        }
    if (!(m <= 1.75))
      return fail(EU_ERR_UNSUPPORTED, "render_views: a biatan6 view whose in-face coordinates exceed 1.75 (the range tanf is reproduced over): use eu_hip_render");
  }
  return EU_OK;
}

// what this path does not render: EU_ERR_UNSUPPORTED. `who` is the entry point the message names; a multi-facet
// job always normalises (build_multi)
static int check_views_supported(const char *who, const eu_target *t, const eu_view *views, int nviews,
                                 eu_source *const *srcs, int nsrc, int *form, int *norm_mode)
{
  for (int f = 0; f < nsrc; f++)
    if (eu::has_translation(srcs[f]->fct))
      return fail(EU_ERR_UNSUPPORTED, std::string(who) + ": a facet with PTO translation is stepped by the generic stepper: use eu_hip_render");
  if (!eu::stepper_form(t->projection, nsrc > 1 || t->ntaps > 0, *form, *norm_mode))
    return fail(EU_ERR_UNSUPPORTED, "no stepper for this target projection");
  return check_views_biatan6(t, views, nviews);
}

// the tap table on the device (biased_taps); where the buffer is rewritten that happens on `st`, from *keep: the
// caller synchronises
static int upload_view_taps(const eu_target *t, hipStream_t st, std::vector<float> *keep)
{
  if (t->ntaps <= 0) return EU_OK;
  *keep = biased_taps(t->taps, t->ntaps);
  if (g.vtaps.p && keep->size() == g.vtaps_host.size() &&
      !memcmp(keep->data(), g.vtaps_host.data(), keep->size() * sizeof(float)))
    return EU_OK;
  g.vtaps_host.clear();
  HIPCHK(g.vtaps.reserve(keep->size()));
  HIPCHK(hipMemcpyAsync(g.vtaps.p, keep->data(), keep->size() * sizeof(float), hipMemcpyHostToDevice, st));
  g.vtaps_host = *keep;
  return EU_OK;
}

// one block per (view, facet), [view][facet]: basis = rotate(r_cam(view), r_fct(facet)), as build_multi forms it
static void view_scalar_blocks(const eu_target *t, const eu_view *views, int nviews, eu_source *const *srcs, int nsrc,
                               std::vector<eu_view_dev> &sc)
{
  sc.resize((size_t)nviews * nsrc);
  std::vector<eu::mat3> r_fct((size_t)nsrc);
  for (int f = 0; f < nsrc; f++) r_fct[f] = eu::make_r3(srcs[f]->fct.roll, srcs[f]->fct.pitch, srcs[f]->fct.yaw, true);
  for (int k = 0; k < nviews; k++) {
    const eu_view &v = views[k];
    const eu::mat3 r_cam = eu::make_r3(v.roll, v.pitch, v.yaw, false);
    for (int f = 0; f < nsrc; f++)
      eu::view_scalars(t->width, t->height, v.x0, v.x1, v.y0, v.y1, eu::rotate(r_cam, r_fct[f]), sc[(size_t)k * nsrc + f]);
  }
}

// One view sequence, of one source or of a multi-facet job (nsrc > 1): the checks behind the entry point's own, in
// the order both entry points have always made them, the chunk size, the scalar blocks, the buffer waits, the one
// synchronising upload, and the chunk loop with its device or staged output. The buffers are g.vcol, g.vrow, g.vscal,
// g.vtaps, g.vstage and, for the facets' parameter blocks of a multi-facet job, g.vsrc; none of build_multi's is touched.
// `who` is the entry point that messages name where they always have.
// `job` is what the entry point supplies:
//   job.prepare(form, norm_mode, sw)   once, when the buffers stand: the kernel parameters of the call
//   job.launch(nv, vs, sw, st)         renders nv views from the tables in g.vcol / g.vrow to job.p.out, rows
//                                      job.p.out_stride apart; nonzero: the launch failed
extern "C++" template <class JOB>
static int run_view_sequence(const char *who, const eu_target *trg, const eu_view *views, int nviews,
                             eu_source *const *srcs, int nsrc, float *out, size_t out_row_stride_bytes,
                             size_t out_view_stride_bytes, int out_on_device, void *stream, JOB &job)
{
  int rc;
  const bool multi = nsrc > 1;
  // the target, and the --mask_for channel rule of every facet
  for (int f = 0; f < nsrc; f++)
    if ((rc = check_views_target(trg, srcs[f]))) return rc;
  for (int f = 1; f < nsrc; f++)
    if (srcs[f]->degree != srcs[0]->degree)
      return fail(EU_ERR_ARGUMENT, "render_views_multi: facets must share the spline degree");
  for (int k = 0; k < nviews; k++)
    if (!view_finite(views[k])) return fail(EU_ERR_ARGUMENT, "render_views: a view with a non-finite field");
  const size_t row_bytes = (size_t)trg->width * trg->nchannels * sizeof(float);
  if (out_row_stride_bytes % sizeof(float) || out_view_stride_bytes % sizeof(float))
    return fail(EU_ERR_ARGUMENT, "render_views: strides must be multiples of 4 bytes");
  if (out_row_stride_bytes < row_bytes) return fail(EU_ERR_ARGUMENT, "render_views: row stride smaller than a row");
  if (out_view_stride_bytes / (size_t)trg->height < out_row_stride_bytes)
    return fail(EU_ERR_ARGUMENT, "render_views: view stride smaller than `height` rows");
  int form = 0, norm_mode = 0;
  if ((rc = check_views_supported(who, trg, views, nviews, srcs, nsrc, &form, &norm_mode))) return rc;
  if (nviews == 0) return EU_OK;
  if ((rc = ensure_init())) return rc;
  for (int f = 0; f < nsrc; f++)
    if (!srcs[f]->dev)
      return fail(EU_ERR_HANDLE, multi ? "render_views_multi: a source has no container" : "render_views: the source has no container");
  const eu_switches sw = eu_read_switches();
  hipStream_t st = stream ? (hipStream_t)stream : g.stream;

  const int W = trg->width, H = trg->height;
  // one table block per (view, facet): the columns of a view are those of its first block
  const size_t col_floats = (size_t)6 * W * nsrc, row_floats = (size_t)H * EU_ROW_FLOATS * nsrc;
  const size_t frame_bytes = (size_t)H * row_bytes;
  int per_chunk = std::min(nviews, eu_views_per_chunk(W, H, sw.views_max_kb, nsrc));
  if (!out_on_device) per_chunk = (int)std::min<size_t>((size_t)per_chunk, std::max<size_t>(1, EU_VIEWS_STAGE_BYTES / frame_bytes));

  std::vector<eu_view_dev> sc;
  view_scalar_blocks(trg, views, nviews, srcs, nsrc, sc);
  // the facets' evaluator parameters (they can change between calls: always refreshed); one source's travel in
  // the kernel argument
  std::vector<eu_src_dev> sd;
  if (multi)
    for (int f = 0; f < nsrc; f++) sd.push_back(srcs[f]->sd);
  std::vector<float> taps;
  drain drain_on_exit{ st, st };          // the host vectors above are among what the call lets go of
  // the view buffers are rewritten on `st`, and reserve() may free them: the view calls before this one have to be
  // through, on callers' streams (the event) and on the library's own. The host waits, as it always has here
  HIPCHK(g.views.host_wait());
  if (stream) HIPCHK(hipStreamSynchronize(g.stream));
  HIPCHK(g.vcol.reserve(col_floats * per_chunk));
  HIPCHK(g.vrow.reserve(row_floats * per_chunk));
  if (!out_on_device) HIPCHK(g.vstage.reserve((size_t)per_chunk * frame_bytes / sizeof(float)));
  // the one host synchronisation of the call: the scalar blocks, the facets, and a new tap table, in flight from host vectors
  HIPCHK(g.vscal.reserve(sc.size()));
  if (multi) HIPCHK(g.vsrc.reserve(sd.size()));
  HIPCHK(hipMemcpyAsync(g.vscal.p, sc.data(), sc.size() * sizeof(eu_view_dev), hipMemcpyHostToDevice, st));
  if (multi) HIPCHK(hipMemcpyAsync(g.vsrc.p, sd.data(), sd.size() * sizeof(eu_src_dev), hipMemcpyHostToDevice, st));
  if ((rc = upload_view_taps(trg, st, &taps))) return rc;
  HIPCHK(hipStreamSynchronize(st));

  eu_view_strides vs;
  vs.col = (long long)col_floats; vs.row = (long long)row_floats;
  vs.out = (long long)((out_on_device ? out_view_stride_bytes : frame_bytes) / sizeof(float));
  job.prepare(form, norm_mode, sw);
  job.p.out_stride = (long long)((out_on_device ? out_row_stride_bytes : row_bytes) / sizeof(float));
  for (int c0 = 0; c0 < nviews; c0 += per_chunk) {
    const int nv = std::min(per_chunk, nviews - c0);
    if (eu_launch_view_tables(g.vscal.p + (size_t)c0 * nsrc, nv * nsrc, trg->projection, W, H, trg->ntaps > 0, g.vcol.p, g.vrow.p, st))
      return fail(EU_ERR_NO_DEVICE, std::string(who) + ": table kernel launch failed");
    char *dst = (char *)out + (size_t)c0 * out_view_stride_bytes;
    job.p.out = out_on_device ? (float *)dst : g.vstage.p;
    if (job.launch(nv, vs, sw, st))
      return fail(EU_ERR_NO_DEVICE, std::string(who) + ": kernel launch failed");
    if (!out_on_device)
      for (int k = 0; k < nv; k++)
        HIPCHK(hipMemcpy2DAsync(dst + (size_t)k * out_view_stride_bytes, out_row_stride_bytes,
                                (const char *)g.vstage.p + (size_t)k * frame_bytes, row_bytes, row_bytes, (size_t)H,
                                hipMemcpyDeviceToHost, st));
  }
  if (!out_on_device) HIPCHK(hipStreamSynchronize(st));
  drain_on_exit.on = false;          // a device output stays queued: `st` goes on reading the view buffers
  return note_caller(g.views, out_on_device ? stream : nullptr, EU_OK);
}

int eu_hip_render_views(const eu_target *trg, const eu_view *views, int nviews, eu_source *src, float *out,
                        size_t out_row_stride_bytes, size_t out_view_stride_bytes, int out_on_device, void *stream)
{
  if (!trg || !views || !src || !out) return fail(EU_ERR_ARGUMENT, "render_views: null argument");
  if (nviews < 0) return fail(EU_ERR_ARGUMENT, "render_views: negative number of views");
  struct {
    const eu_target *trg;
    const eu_source *src;
    eu_render_params p;
    int path;
    void prepare(int form, int norm_mode, const eu_switches &sw)
    {
      memset(&p, 0, sizeof p);
      p.width = trg->width; p.height = trg->height; p.row_begin = 0; p.row_end = trg->height;
      p.form = form; p.norm_mode = norm_mode;
      p.twine = trg->ntaps > 0; p.ntaps = trg->ntaps; p.nch = src->nch; p.nch_out = trg->nchannels;
      p.col = g.vcol.p; p.row = g.vrow.p; p.taps = g.vtaps.p;
      p.src = src->sd;
      p.direct = 1;
      path = eu_select_view_path(p, sw);
    }
    int launch(int nv, const eu_view_strides &vs, const eu_switches &sw, hipStream_t st)
    {
      return eu_launch_render_views(&p, &vs, nv, path, &sw, st);
    }
  } job{ trg, src };
  return run_view_sequence("render_views", trg, views, nviews, &src, 1, out, out_row_stride_bytes, out_view_stride_bytes,
                           out_on_device, stream, job);
}

// ---------------------------------------------------------------------------------------------------------
// many views of a multi-facet job in one call (include/eu_hip.h, eu_render_views_multi.hip)
// ---------------------------------------------------------------------------------------------------------
// What build_multi does per camera on the host - one build_stepper_tables per facet, a pageable upload of the row
// tables, two synchronisations - is one scalar block per (view, facet) here: the table kernel makes the tables of
// a chunk of views in one launch, the render kernel has the view on blockIdx.y. EU_HIP_REJ is not applied: the
// early-miss tables change no bit and were measured slower (build_multi).
int eu_hip_render_views_multi(const eu_target *trg, const eu_view *views, int nviews, eu_source *const *srcs, int nsrc,
                              float *out, size_t out_row_stride_bytes, size_t out_view_stride_bytes, int out_on_device,
                              void *stream)
{
  if (!trg || !views || !srcs || !out) return fail(EU_ERR_ARGUMENT, "render_views_multi: null argument");
  if (nsrc < 1) return fail(EU_ERR_ARGUMENT, "render_views_multi: no source");
  if (nsrc > EU_VIEWS_MAX_GRID_Y) return fail(EU_ERR_ARGUMENT, "render_views_multi: more than 65535 facets");
  if (nviews < 0) return fail(EU_ERR_ARGUMENT, "render_views: negative number of views");
  for (int f = 0; f < nsrc; f++)
    if (!srcs[f]) return fail(EU_ERR_HANDLE, "render_views_multi: null source");
  if (nsrc == 1)
    return eu_hip_render_views(trg, views, nviews, srcs[0], out, out_row_stride_bytes, out_view_stride_bytes,
                               out_on_device, stream);
  struct {
    const eu_target *trg;
    eu_source *const *srcs;
    int nsrc;
    eu_multi_params p;
    void prepare(int form, int norm_mode, const eu_switches &)
    {
      memset(&p, 0, sizeof p);
      p.width = trg->width; p.height = trg->height; p.row_begin = 0; p.row_end = trg->height;
      p.form = form; p.norm_mode = norm_mode; p.twine = trg->ntaps > 0; p.ntaps = trg->ntaps;
      p.nch = trg->nchannels; p.nfct = nsrc; p.plus = (trg->nchannels == 2 || trg->nchannels == 4);
      p.hdr = trg->synopsis == EU_SYN_HDR_MERGE;
      // _hdr_merge_syn ctor (envutil_payload.cc:1346-1376): the first strict minimum / maximum of brighten
      float lowest = 100000.0f, highest = -1.0f;
      p.hdr_low = p.hdr_high = -1;
      for (int f = 0; f < nsrc; f++) {
        const float b = srcs[f]->sd.brighten;
        if (b < lowest) { lowest = b; p.hdr_low = f; }
        if (b > highest) { highest = b; p.hdr_high = f; }
      }
      p.col = g.vcol.p; p.row = g.vrow.p; p.taps = g.vtaps.p; p.srcs = g.vsrc.p;
    }
    int launch(int nv, const eu_view_strides &vs, const eu_switches &, hipStream_t st)
    {
      return eu_launch_render_views_multi(&p, &vs, nv, srcs[0]->degree, st);
    }
  } job{ trg, srcs, nsrc };
  return run_view_sequence("render_views_multi", trg, views, nviews, srcs, nsrc, out, out_row_stride_bytes,
                           out_view_stride_bytes, out_on_device, stream, job);
}

// For tests: the tables the table kernel writes for one view, and eu::build_stepper_tables for the same view
int eu_hip_view_tables(const eu_target *trg, const eu_view *view, eu_source *src, float *col_dev_built,
                       float *row_dev_built, float *col_host_built, float *row_host_built)
{
  int rc;
  if (!trg || !view || !src || !col_dev_built || !row_dev_built || !col_host_built || !row_host_built)
    return fail(EU_ERR_ARGUMENT, "view_tables: null argument");
  if ((rc = check_views_target(trg, src))) return rc;
  if (!view_finite(*view)) return fail(EU_ERR_ARGUMENT, "view_tables: a view with a non-finite field");
  int form = 0, norm_mode = 0;
  if ((rc = check_views_supported("render_views", trg, view, 1, &src, 1, &form, &norm_mode))) return rc;
  if ((rc = ensure_init())) return rc;
  if (!src->dev) return fail(EU_ERR_HANDLE, "view_tables: the source has no container");
  const int W = trg->width, H = trg->height;
  const bool twine = trg->ntaps > 0;
  const size_t col_floats = (size_t)6 * W, row_floats = (size_t)H * EU_ROW_FLOATS;
  {
    eu_target t = *trg;
    t.yaw = view->yaw; t.pitch = view->pitch; t.roll = view->roll;
    t.x0 = view->x0; t.x1 = view->x1; t.y0 = view->y0; t.y1 = view->y1;
    const eu::mat3 basis = eu::rotate(eu::make_r3(t.roll, t.pitch, t.yaw, false),
                                      eu::make_r3(src->fct.roll, src->fct.pitch, src->fct.yaw, true));
    eu::stepper_tables tb;
    if (!eu::build_stepper_tables(t, basis, twine, twine, tb) || tb.form != form || tb.norm_mode != norm_mode)
      return fail(EU_ERR_UNSUPPORTED, "no stepper for this target projection");
    memcpy(col_host_built, tb.col.data(), col_floats * sizeof(float));
    memcpy(row_host_built, tb.row.data(), row_floats * sizeof(float));
  }
  std::vector<eu_view_dev> sc;
  view_scalar_blocks(trg, view, 1, &src, 1, sc);
  HIPCHK(g.views.host_wait());
  HIPCHK(g.vcol.reserve(col_floats));
  HIPCHK(g.vrow.reserve(row_floats));
  HIPCHK(g.vscal.reserve(1));
  HIPCHK(hipMemcpyAsync(g.vscal.p, sc.data(), sizeof(eu_view_dev), hipMemcpyHostToDevice, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  if (eu_launch_view_tables(g.vscal.p, 1, trg->projection, W, H, twine, g.vcol.p, g.vrow.p, g.stream))
    return fail(EU_ERR_NO_DEVICE, "view_tables: table kernel launch failed");
  HIPCHK(hipMemcpyAsync(col_dev_built, g.vcol.p, col_floats * sizeof(float), hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipMemcpyAsync(row_dev_built, g.vrow.p, row_floats * sizeof(float), hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  return EU_OK;
}

// DIAGNOSTIC (not declared in eu_hip.h): a source handle without a container, made without a device, so that
// the argument checks of eu_hip_render_rays can be exercised where there is none (tests/test_rays_host.py).
// Only eu_hip_render_rays[_timed] - which refuse it once they have a device - and eu_hip_source_release take it.
int eu_hip_diag_host_source(const eu_facet *fct, int spline_degree, eu_source **out)
{
  int rc;
  if ((rc = check_facet(fct))) return rc;
  if (!out) return fail(EU_ERR_ARGUMENT, "null argument");
  eu_source *s = bare_source(fct, spline_degree);
  if (!s) return fail(EU_ERR_MEMORY, "host allocation failed");
  *out = s;
  return EU_OK;
}

int eu_hip_sync(void)
{
  if (g.device < 0) return EU_OK;
  HIPCHK(hipStreamSynchronize(g.stream));
  for (const eu_readers *r : { &g.tables, &g.wl_pair, &g.rays, &g.views, &g.encode, &g.alpha }) HIPCHK(r->host_wait());
  return EU_OK;
}

int eu_hip_render_timed(const eu_target *trg, eu_source *const *srcs, int nsrc, float *out_dev,
                        size_t out_row_stride_bytes, int iters, float *mean_ms)
{
  int rc;
  if ((rc = ensure_init())) return rc;
  if (iters <= 0 || !mean_ms) return fail(EU_ERR_ARGUMENT, "bad iteration count");
  if (!srcs || nsrc < 1 || !trg || !out_dev) return fail(EU_ERR_ARGUMENT, "no source / no output");
  if ((rc = check_target(trg))) return rc;
  const eu_switches sw = eu_read_switches();
  // (the untimed launch builds the plan: stepper tables, derived copies)
  auto once = [&]() { return render_on_device(trg, srcs, nsrc, out_dev, out_row_stride_bytes, sw, g.stream); };
  return time_on_stream(once, iters, mean_ms);
}

// DIAGNOSTIC (not declared in eu_hip.h): phase stamps of the headline path,
// 8 x uint64 per wave: t0..t5, XCC id, tile index
int eu_hip_diag_stamps(const eu_target *trg, eu_source *const *srcs, int nsrc, float *out_dev,
                       size_t out_row_stride_bytes, unsigned long long *host_stamps,
                       size_t nwaves)
{
  int rc;
  if ((rc = ensure_init())) return rc;
  eu_render_params p;
  if ((rc = build_params(trg, srcs, nsrc, out_dev, out_row_stride_bytes, eu_read_switches(), &p))) return rc;
  if (p.nch != 3 || p.src.degree != 3 || p.twine) return fail(EU_ERR_ARGUMENT, "diag: NCH 3, degree 3, no twining");
  eu_dev_tmp<unsigned long long> d;
  HIPCHK(d.alloc(nwaves * 8));
  HIPCHK(hipMemsetAsync(d.p, 0, nwaves * 8 * sizeof(unsigned long long), g.stream));
  for (int i = 0; i < 3; i++)
    if (eu_launch_diag(&p, d.p, g.stream)) return fail(EU_ERR_NO_DEVICE, "diag launch failed");
  HIPCHK(hipStreamSynchronize(g.stream));
  HIPCHK(hipMemcpy(host_stamps, d.p, nwaves * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return EU_OK;
}

// DIAGNOSTIC (not in eu_hip.h): the ray -> source coordinate stage of the kernels on
// caller-supplied rays (n x 3 floats, host): variant 0 eu_source_coordinate, 1 eu_coord2,
// 2 eu_coord2_ok (eu_diag.hip). out = n x 3 floats: x, y, cube face | 0; a miss is 0, 0, -1
int eu_hip_diag_source_coordinates(const eu_source *src, const float *rays, long n, int variant, float *out)
{
  int rc;
  if ((rc = ensure_init())) return rc;
  if (!src || !rays || !out || n < 0) return fail(EU_ERR_ARGUMENT, "null argument");
  if (n == 0) return EU_OK;
  eu_dev_tmp<float> buf;
  HIPCHK(buf.alloc((size_t)n * 6));
  float *d = buf.p;
  HIPCHK(hipMemcpy(d, rays, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice));
  const int lrc = eu_launch_diag_coords(&src->sd, d, n, variant, d + (size_t)n * 3, g.stream);
  if (lrc > 0) return fail(EU_ERR_UNSUPPORTED, "the packed forms cover lat/lon, cubemap and biatan6 sources");
  if (lrc < 0) return fail(EU_ERR_NO_DEVICE, "diag launch failed");
  HIPCHK(hipStreamSynchronize(g.stream));
  HIPCHK(hipMemcpy(out, d + (size_t)n * 3, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost));
  return EU_OK;
}

// DIAGNOSTIC (not in eu_hip.h): mismatch counts {div, sqrt, atan2, const div}
int eu_hip_selftest_math(unsigned long long seed, int blocks, int iters, unsigned long long *bad4)
{
  int rc;
  if ((rc = ensure_init())) return rc;
  eu_dev_tmp<unsigned long long> d;
  HIPCHK(d.alloc(4));
  HIPCHK(hipMemsetAsync(d.p, 0, 4 * sizeof(unsigned long long), g.stream));
  if (eu_launch_selftest(seed, blocks, iters, d.p, g.stream)) return fail(EU_ERR_NO_DEVICE, "selftest launch failed");
  HIPCHK(hipStreamSynchronize(g.stream));
  HIPCHK(hipMemcpy(bad4, d.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return EU_OK;
}

int eu_hip_malloc(void **p, size_t bytes)
{
  int rc;
  if ((rc = ensure_init())) return rc;
  HIPCHK(hipMalloc(p, bytes));
  return EU_OK;
}
int eu_hip_free(void *p) { if (p) HIPCHK(hipFree(p)); return EU_OK; }
int eu_hip_memcpy_d2h(void *dst, const void *src, size_t bytes)
{
  HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return EU_OK;
}
int eu_hip_memcpy_h2d(void *dst, const void *src, size_t bytes)
{
  HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return EU_OK;
}

}  // extern "C"
