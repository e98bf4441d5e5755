// C ABI (include/eu_hip.h): host glue between the reference-shaped job
// description and the HIP kernels. No CPU rendering path exists in this
// library: without a HIP device every render/load call fails with
// EU_ERR_NO_DEVICE.
// This file: the state and the helpers the call families share (eu_context.h), initialisation, the pure queries,
// memory. The families: eu_api_source.hip, eu_api_render.hip, eu_api_devices.hip, eu_api_rays.hip, eu_api_views.hip,
// eu_api_layers.hip, eu_api_multiband.hip.

#include "eu_context.h"
#include "eu_setup_math.h"

namespace eu_host __attribute__((visibility("hidden"))) {

thread_local std::string g_err;
context ctx_[EU_MAX_SLOTS];
int nslots_ = 1, cur_slot_ = 0;

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
  if (!cur().stream) HIPCHK(hipStreamCreateWithFlags(&cur().stream, hipStreamNonBlocking));
  if (!cur().lut) {
    float lut[257];
    eu::screen_lut(lut);
    HIPCHK(hipMalloc((void **)&cur().lut, sizeof lut));
    HIPCHK(hipMemcpy(cur().lut, lut, sizeof lut, hipMemcpyHostToDevice));
  }
  cur().device = dev;
  return EU_OK;
}

int ensure_init()
{
  if (cur().device >= 0) return EU_OK;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(EU_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
  int dev = 0;
  const char *lr = getenv("LOCAL_RANK");
  if (lr) dev = atoi(lr) % n;
  return init_device(dev);
}

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

// the synopsis and its width: asked on its own by the entry points that look for a device before they look at
// the target (eu_hip_render, eu_hip_render_devices), so that these refusals need none
int check_synopsis(const eu_target *t)
{
  if (t->synopsis != EU_SYN_PANORAMA && t->synopsis != EU_SYN_HDR_MERGE && t->synopsis != EU_SYN_FEATHER &&
      t->synopsis != EU_SYN_MULTIBAND)
    return fail(EU_ERR_ARGUMENT, "unknown synopsis");
  if (!std::isfinite(t->feather) || t->feather < 0.0)
    return fail(EU_ERR_ARGUMENT, "feather must be a finite width in source pixels, 0 for the default");
  if (t->synopsis == EU_SYN_MULTIBAND && t->bands < 0)
    return fail(EU_ERR_ARGUMENT, "bands must be 0 (the default) or the number of pyramid levels");
  return EU_OK;
}

// What a multi-band job cannot be, because its pyramid needs the whole float frame at once; each with a message
// of its own, and without a device. Single-facet jobs ignore the synopsis.
int check_multiband(const eu_target *t, eu_source *const *srcs, int nsrc)
{
  if (t->synopsis != EU_SYN_MULTIBAND || nsrc < 2) return EU_OK;
  if (t->ntaps > 0) return fail(EU_ERR_ARGUMENT, "multiband: no twining - the pyramid blends whole frames, not tap rays");
  if (t->band_count > 1) return fail(EU_ERR_ARGUMENT, "multiband: no row bands - the pyramid needs the whole frame");
  if (t->crop_w > 0) return fail(EU_ERR_ARGUMENT, "multiband: no crop window - the pyramid needs the whole frame");
  if (t->row_begin != 0 || t->row_end != t->height)
    return fail(EU_ERR_ARGUMENT, "multiband: the row range must be the whole frame");
  if (t->out_format == EU_OUT_SRGBA8) return fail(EU_ERR_ARGUMENT, "multiband: EU_OUT_SRGBA8 is not blended, render floats");
  for (int f = 0; srcs && f < nsrc; f++)
    if (srcs[f] && srcs[f]->fct.mask_paint)
      return fail(EU_ERR_ARGUMENT, "multiband: --mask_for paints facets, a pyramid of paint is no mask");
  return EU_OK;
}

// the multi-band levels of a target: columns wrap on a spherical or cylindrical target of 360 degrees
void multiband_geom(const eu_target *t, eu_mb_geom *g)
{
  const bool wrap = (t->projection == EU_SPHERICAL || t->projection == EU_CYLINDRICAL) &&
                    std::fabs((t->x1 - t->x0) - 2.0 * M_PI) < .000001;
  eu_mb_levels(t->width, t->height, t->bands, wrap, g);
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
  { int rcs = check_synopsis(t); if (rcs) return rcs; }
  if (t->out_format != EU_OUT_FLOAT && t->out_format != EU_OUT_SRGBA8)
    return fail(EU_ERR_ARGUMENT, "unknown output format");
  if (t->out_format == EU_OUT_SRGBA8 && t->stage)
    return fail(EU_ERR_ARGUMENT, "stage outputs are float only");
  if ((t->stage == 3 || t->stage == 4) && t->ntaps == 0)
    return fail(EU_ERR_ARGUMENT, "stages 3 and 4 are the neighbour rays of a twined job: they need a tap table");
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

// what an eu_multi_params takes from the target and the facets: synopsis by channel count, and for an HDR merge
// the _hdr_merge_syn ctor (envutil_payload.cc:1346-1376): the first strict minimum / maximum of brighten
void fill_synopsis(const eu_target *t, eu_source *const *srcs, int nsrc, eu_multi_params *p)
{
  p->nch = t->nchannels; p->nfct = nsrc; p->plus = (t->nchannels == 2 || t->nchannels == 4);
  p->mode = t->synopsis == EU_SYN_HDR_MERGE ? EU_MODE_HDR : t->synopsis == EU_SYN_FEATHER ? EU_MODE_FEATHER
            : t->synopsis == EU_SYN_MULTIBAND ? EU_MODE_LAYERS : EU_MODE_PANORAMA;
  // a facet with a distance plane (EU_LOAD_EDGES): the loops that sample it; every other job keeps its kernels
  bool planes = false;
  for (int f = 0; f < nsrc; f++) planes = planes || srcs[f]->edge;
  if (planes && p->mode == EU_MODE_FEATHER) p->mode = EU_MODE_FEATHER_EDGES;
  if (planes && p->mode == EU_MODE_LAYERS) p->mode = EU_MODE_LAYERS_EDGES;
  float lowest = 100000.0f, highest = -1.0f;
  p->hdr_low = p->hdr_high = -1;
  for (int f = 0; f < nsrc; f++) {
    const float b = srcs[f]->sd.brighten;
    if (b < lowest) { lowest = b; p->hdr_low = f; }
    if (b > highest) { highest = b; p->hdr_high = f; }
  }
}

// The edge weight's constants per facet (eu_synopsis_feather). The width is the target's `feather` in source
// pixels; 0: half the shorter side of that facet's window, so that the ramp reaches the centre. An axis has no
// border where the facet wraps or closes there: axis 0 where the load chose PERIODIC, axis 1 for a full sphere
// (the load's own condition for the spherical prefilter), both for cube sources and wherever the mask is
// constant true.
std::vector<eu_feather_dev> feather_table(const eu_target *t, eu_source *const *srcs, int nsrc)
{
  std::vector<eu_feather_dev> v((size_t)nsrc);
  for (int f = 0; f < nsrc; f++) {
    memset(&v[f], 0, sizeof v[f]);              // (the padding too: the table is compared and hashed as bytes)
    const eu_source *s = srcs[f];
    const eu_facet &fc = s->fct;
    const bool closed = eu_cube_source(fc.projection) || s->sd.mask_all;
    const bool wrap0 = closed || s->bc[0] == EU_BC_PERIODIC;
    const bool wrap1 = closed || (full_sphere(&fc) && s->bc[0] == EU_BC_PERIODIC);
    const double width_px = t->feather > 0.0 ? t->feather : 0.5 * (double)std::min(fc.window_width, fc.window_height);
    v[f].rcp = (float)(1.0 / width_px);
    v[f].lim_x = (float)fc.window_width - 0.5f;
    v[f].lim_y = (float)fc.window_height - 0.5f;
    v[f].border = (wrap0 ? 0 : 1) | (wrap1 ? 0 : 2);
    // the distance plane of a source loaded with EU_LOAD_EDGES: its rows close where the load made axis 0 periodic
    v[f].dist = s->edge;
    v[f].dist_w = s->edge ? fc.window_width : 0;
    v[f].dist_h = s->edge ? fc.window_height : 0;
    v[f].cyclic = s->edge && s->bc[0] == EU_BC_PERIODIC;
  }
  return v;
}

}  // namespace eu_host

using namespace eu_host;

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
  if (cur().device == device) return EU_OK;
  // one device per process (one process per GPU): the stream, the LUT, the plan tables and
  // every resident source live on the device chosen first
  if (cur().device >= 0)
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

int eu_hip_band_rows(int height, int band_rows, int band_count, int band_index)
{
  if (height < 0 || (band_count > 1 && (band_rows < 1 || band_index < 0 || band_index >= band_count))) return 0;
  return local_rows(height, band_rows, band_count, band_index);
}

int eu_hip_sync(void)
{
  if (cur().device < 0) return EU_OK;
  HIPCHK(hipStreamSynchronize(cur().stream));
  const context &c = cur();
  for (const eu_readers *r : { &c.tables, &c.staged.wl_pair, &c.rays.readers, &c.views.readers, &c.layers.readers, &c.enc.readers, &c.alpha.readers, &c.reload.readers })
    HIPCHK(r->host_wait());
  return EU_OK;
}

// DIAGNOSTIC (not in eu_hip.h): mismatch counts {div, sqrt, atan2, const div}
int eu_hip_selftest_math(unsigned long long seed, int blocks, int iters, unsigned long long *bad4)
{
  int rc;
  if ((rc = ensure_init())) return rc;
  eu_dev_tmp<unsigned long long> d;
  HIPCHK(d.alloc(4));
  HIPCHK(hipMemsetAsync(d.p, 0, 4 * sizeof(unsigned long long), cur().stream));
  if (eu_launch_selftest(seed, blocks, iters, d.p, cur().stream)) return fail(EU_ERR_NO_DEVICE, "selftest launch failed");
  HIPCHK(hipStreamSynchronize(cur().stream));
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
