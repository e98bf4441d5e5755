// C ABI (include/eu_hip.h), host glue: sources - the handle and its container, the alpha edit, the load pipeline.

#include "eu_context.h"
#include "eu_setup_math.h"
#include "eu_imageprep.h"
#include "eu_alpha.h"
#include "eu_edges.h"
#include "eu_decode.h"
#include "eu_rgbe_dev.h"
#include "eu_ycbcr_dev.h"
#include "../../include/eu_ycbcr.h"

using namespace eu_host;

namespace {

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
  d.cdiv_ok = eu_verify_const_div(d.ext_w, 2.0f * d.ext_w, cur().stream)
           && eu_verify_const_div(d.ext_h, 2.0f * d.ext_h, cur().stream);
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
  s->support_min = support_min; s->tile_size = tile_size;
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
// (full_sphere: eu_context.h - the feathered synopsis asks the same question)

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
  HIPCHK(cur().alpha.readers.host_wait());
  HIPCHK(hipStreamSynchronize(cur().stream));
  HIPCHK(cur().alpha.plan.reserve(plan.size() + 2));
  HIPCHK(hipMemcpy(cur().alpha.plan.p, plan.data(), plan.size() * sizeof(int), hipMemcpyHostToDevice));
  p->keep = cur().alpha.plan.p;
  p->row_start = p->keep + size_t(h) * 2;
  p->spans = p->row_start + size_t(h) + 1;
  return EU_OK;
}

// ---- the load pipeline: pixels -> braced, prefiltered container ------------------------------------------

// where a loader's pixels come from
enum feed_kind {
  FEED_HOST_FLOATS,      // host floats at the facet's channel count, no edit: copied straight to the destination
  FEED_EDITED_FLOATS,    // floats on the host (staged on the device first) or on the device, through the edit
  FEED_SAMPLES,          // 8- or 16-bit samples on the host (uploaded behind their tables) or on the device, decoded there
  FEED_RGBE,             // Radiance RGBE quads on the host (uploaded behind their table, if any) or on the device, decoded there
  FEED_YCBCR             // the planes of a Y'CbCr frame on the host (uploaded behind their tables, row by row) or on the device, decoded there
};
struct load_feed {
  feed_kind kind;
  const char *who;             // the entry point, as messages name it
  const void *data;            // the floats or the samples (FEED_YCBCR: the luma plane)
  bool on_device;              // data lies in device memory
  int src_ch;                  // channels of data: the facet's, or one less
  const eu_facet_edit *edit;   // masks and crop (FEED_HOST_FLOATS: none)
  bool alter;                  // the edit's kernel runs: FEED_EDITED_FLOATS whenever the edit changes something (a gained
                               // channel too), the integer feeds for masks or a crop (the decoder writes a gained channel itself)
  const eu_samples *smp;       // FEED_SAMPLES: bits, byte order, tables
  const float *rgbe_table;     // FEED_RGBE: 65536 floats, or nullptr for the format's own decode
  const eu_ycbcr *ycc;         // FEED_YCBCR: planes, layout, tables, matrix
};

// Where a fill keeps what it needs beside the container. A load's is its own and freed by scope, after the load's one
// synchronisation. A reload's cannot be - its work may still be queued when it returns - so it lies in the context
// (context::reload), grows on demand and serves the next reload: that one's stream goes behind reload.readers, and a
// buffer that has to grow (reserve() frees) or a table that changes is waited for by the host first.
struct fill_scratch {
  const bool resident;
  eu_dev_tmp<char> t_block;
  eu_dev_tmp<float> t_staged, t_faces;
  eu_dev_tmp<int32_t> t_edges;
  std::vector<float> tabs;           // a load's tables on their way up: alive until the load has synchronised
  explicit fill_scratch(bool res) : resident(res) {}

  template <class T> static hipError_t grow(eu_dev_buf<T> &b, size_t n)
  {
    if (b.cap >= n) return hipSuccess;
    hipError_t e = cur().reload.readers.host_wait();
    if (e == hipSuccess) e = hipStreamSynchronize(cur().stream);
    return e == hipSuccess ? b.reserve(n) : e;
  }
  // the feed's tables (`tabs`, possibly none) on the device and room for nbytes bytes of a host image: a load's in
  // ONE block, tables first; a reload's tables are held (equal ones are not sent again), its bytes a buffer of their own
  hipError_t tables_and_bytes(size_t nbytes, hipStream_t st, const float **tab, char **bytes)
  {
    const size_t tab_bytes = tabs.size() * sizeof(float);
    *tab = nullptr; *bytes = nullptr;
    hipError_t e = hipSuccess;
    if (!resident) {
      if (!tab_bytes && !nbytes) return e;
      e = t_block.alloc(tab_bytes + nbytes);
      if (e == hipSuccess && tab_bytes) e = hipMemcpyAsync(t_block.p, tabs.data(), tab_bytes, hipMemcpyHostToDevice, st);
      if (tab_bytes) *tab = reinterpret_cast<const float *>(t_block.p);
      *bytes = t_block.p + tab_bytes;
      return e;
    }
    held_table &h = cur().reload.tables;
    if (tab_bytes && !h.holds(tabs.data(), tabs.size())) {
      // an earlier reload may still read the device table, and its upload the host copy
      e = cur().reload.readers.host_wait();
      if (e == hipSuccess) e = hipStreamSynchronize(cur().stream);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      h.host.clear();
      if (e == hipSuccess) e = h.dev.reserve(tabs.size());
      if (e == hipSuccess) {
        h.host.swap(tabs);
        e = hipMemcpyAsync(h.dev.p, h.host.data(), tab_bytes, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) h.host.clear();
      }
    }
    if (tab_bytes) *tab = h.dev.p;
    if (e == hipSuccess && nbytes) { e = grow(cur().reload.block, nbytes); *bytes = cur().reload.block.p; }
    return e;
  }
  hipError_t staged(size_t n, float **p)
  {
    const hipError_t e = resident ? grow(cur().reload.staged, n) : t_staged.alloc(n);
    *p = resident ? cur().reload.staged.p : t_staged.p;
    return e;
  }
  hipError_t edges(size_t n, int32_t **p)
  {
    const hipError_t e = resident ? grow(cur().reload.edges, n) : t_edges.alloc(n);
    *p = resident ? cur().reload.edges.p : t_edges.p;
    return e;
  }
  hipError_t faces(size_t n, float **p)
  {
    const hipError_t e = resident ? grow(cur().reload.faces, n) : t_faces.alloc(n);
    *p = resident ? cur().reload.faces.p : t_faces.p;
    return e;
  }
};

// what a fill leaves: the HIP error of an allocation or a copy, the result of the finish, and the status of a plan
// upload or a kernel launch (its message is set)
struct fill_result { hipError_t e; int rc, prc; };

// One load pipeline with five feeds, in two halves. load_source MAKES the source and its container (source_bcs,
// new_source), has it filled, synchronises once and settles the error precedence: the message the plan upload or a
// kernel launch set, then the HIP error, then "device set-up stage failed". fill_source FILLS a source that exists,
// for a load and for eu_hip_source_reload alike, all of it queued on `st`: the plane the pixels arrive in - the
// facet's window as the core of the container, or the stack of a cubemap's six faces in scratch -, the clearing of a
// flat container, the finish (cube build, or the prefilter full_sphere() picks). The feed is all that differs. Host
// floats: one H2D copy into the plane (1-D into the faces, 2-D into the core), no staging, no kernel. Floats through the
// edit: host pixels are staged on the device at their own channel count; upload_alpha_plan + eu_launch_facet_alpha
// write the plane, or - an edit that changes nothing, pixels on the device - a 2-D D2D copy. Integer samples: both
// tables and, behind them, the samples of a host image go to the device; eu_launch_decode writes the plane, or - with
// masks or a crop - a dense buffer that eu_launch_facet_alpha then reads. RGBE quads: the integer feed with a dword
// per pixel - the optional table and, behind it, the quads of a host image; eu_launch_rgbe_decode writes what
// eu_launch_decode writes for three samples per pixel. Y'CbCr planes: both tables and, behind them, the planes of a host
// frame as their rows lie (a 2-D copy each; interleaved chroma once); eu_launch_ycbcr_decode writes what the RGBE
// decode writes. The geometry is the source's own: its container, the boundary conditions it holds, what it was built
// with (support_min, tile_size). The entry points make their own argument checks, in their own order, and find the device.
fill_result fill_source(eu_source *s, int prefilter_degree, const load_feed &feed, hipStream_t st, fill_scratch &sc)
{
  const eu_facet *fct = &s->fct;
  const std::string who(feed.who);
  const int nch = s->nch, src_ch = feed.src_ch, iir_stream = eu_read_switches().iir_stream;
  const bool cube = eu_cube_source(fct->projection);
  eu::metrics m {};
  if (cube) m = eu::make_metrics(fct->width, fct->hfov, s->support_min, s->tile_size);
  const eu_container &gm = s->geom;
  const int w = cube ? int(m.face_px) : int(gm.core[0]), h = cube ? int(6 * m.face_px) : int(gm.core[1]);
  const size_t npix = size_t(w) * size_t(h);
  float *staged = nullptr, *faces = nullptr;   // floats in front of the edit, at src_ch channels; the faces of a cubemap
  const float *tab = nullptr;                  // the feed's tables on the device
  char *bytes = nullptr;                       // the samples, quads or planes of a host image, as they are
  const void *src = feed.data;
  eu_ycbcr_decode_params yd {};
  hipError_t e = hipSuccess;
  int rc = 0, prc = 0;
  // what the feed brings to the device first
  if (feed.kind == FEED_SAMPLES) {
    const size_t ntab = size_t(1) << feed.smp->bits, nbytes = npix * size_t(src_ch) * size_t(feed.smp->bits / 8);
    try {
      sc.tabs.assign(feed.smp->colour_table, feed.smp->colour_table + ntab);
      const float *at = feed.smp->alpha_table ? feed.smp->alpha_table : feed.smp->colour_table;
      sc.tabs.insert(sc.tabs.end(), at, at + ntab);
    } catch (...) { return { e, rc, fail(EU_ERR_MEMORY, who + ": host memory") }; }
    e = sc.tables_and_bytes(feed.on_device ? 0 : nbytes, st, &tab, &bytes);
    if (e == hipSuccess && !feed.on_device) {
      e = hipMemcpyAsync(bytes, feed.data, nbytes, hipMemcpyHostToDevice, st);
      src = bytes;
    }
    if (e == hipSuccess && feed.alter) e = sc.staged(npix * src_ch, &staged);
  } else if (feed.kind == FEED_RGBE) {
    const size_t nbytes = npix * 4;
    if (feed.rgbe_table) {
      try { sc.tabs.assign(feed.rgbe_table, feed.rgbe_table + 65536); }
      catch (...) { return { e, rc, fail(EU_ERR_MEMORY, who + ": host memory") }; }
    }
    e = sc.tables_and_bytes(feed.on_device ? 0 : nbytes, st, &tab, &bytes);
    if (e == hipSuccess && !feed.on_device) {
      e = hipMemcpyAsync(bytes, feed.data, nbytes, hipMemcpyHostToDevice, st);
      src = bytes;
    }
    if (e == hipSuccess && feed.alter) e = sc.staged(npix * src_ch, &staged);
  } else if (feed.kind == FEED_YCBCR) {
    const eu_ycbcr &y = *feed.ycc;
    const size_t ntab = size_t(1) << y.bits, sb = size_t(y.bits / 8);
    const size_t cw = (size_t(w) + y.sub_x - 1) / y.sub_x, chh = (size_t(h) + y.sub_y - 1) / y.sub_y;
    try {
      sc.tabs.assign(y.y_table, y.y_table + ntab);
      sc.tabs.insert(sc.tabs.end(), y.c_table, y.c_table + ntab);
    } catch (...) { return { e, rc, fail(EU_ERR_MEMORY, who + ": host memory") }; }
    yd.y = y.y; yd.cb = y.cb; yd.cr = y.cr; yd.y_pitch = y.y_pitch; yd.c_pitch = y.c_pitch;
    // a host frame: the rows of each plane, as they lie, at a pitch of whole dwords; chroma samples that interleave in
    // ONE plane (NV12, NV21: the two pointers one sample apart) go up once
    const char *pb = static_cast<const char *>(y.cb), *pr = static_cast<const char *>(y.cr);
    // (the last row of a plane may end with its last sample, so a single row is one 1-D copy whatever its pitch)
    const bool one = y.c_step == 2 && (pr == pb + sb || pb == pr + sb) && (chh == 1 || y.c_pitch >= 2 * cw * sb);
    auto rows_up = [&](char *d, size_t dp, const void *s, size_t sp, size_t width, size_t rows) {
      return rows == 1 ? hipMemcpyAsync(d, s, width, hipMemcpyHostToDevice, st)
                       : hipMemcpy2DAsync(d, dp, s, sp, width, rows, hipMemcpyHostToDevice, st);
    };
    const size_t y_row = size_t(w) * sb, c_row = one ? 2 * cw * sb : ((cw - 1) * y.c_step + 1) * sb;
    const size_t y_dp = (y_row + 3) & ~size_t(3), c_dp = (c_row + 3) & ~size_t(3);
    const size_t nbytes = y_dp * h + (one ? 1 : 2) * c_dp * chh;
    e = sc.tables_and_bytes(feed.on_device ? 0 : nbytes, st, &tab, &bytes);
    if (e == hipSuccess && !feed.on_device) {
      char *dy = bytes, *dc0 = dy + y_dp * h, *dc1 = dc0 + c_dp * chh;
      e = rows_up(dy, y_dp, y.y, y.y_pitch, y_row, size_t(h));
      if (one) {
        const char *first = pb < pr ? pb : pr;
        if (e == hipSuccess) e = rows_up(dc0, c_dp, first, y.c_pitch, c_row, chh);
        yd.cb = dc0 + (pb - first); yd.cr = dc0 + (pr - first);
      } else {
        if (e == hipSuccess) e = rows_up(dc0, c_dp, pb, y.c_pitch, c_row, chh);
        if (e == hipSuccess) e = rows_up(dc1, c_dp, pr, y.c_pitch, c_row, chh);
        yd.cb = dc0; yd.cr = dc1;
      }
      yd.y = dy; yd.y_pitch = y_dp; yd.c_pitch = c_dp;
    }
    if (e == hipSuccess && feed.alter) e = sc.staged(npix * src_ch, &staged);
  } else if (feed.kind == FEED_EDITED_FLOATS && !feed.on_device) {
    e = sc.staged(npix * src_ch, &staged);
    if (e == hipSuccess) e = hipMemcpyAsync(staged, feed.data, npix * src_ch * sizeof(float), hipMemcpyHostToDevice, st);
    src = staged;
  }
  // the plane: w x h pixels of nch floats at dst, rows dst_pitch pixels apart
  if (e == hipSuccess && cube) e = sc.faces(npix * nch, &faces);
  if (e == hipSuccess && !cube) e = hipMemsetAsync(s->dev, 0, s->nfloats * sizeof(float), st);
  float *dst = cube ? faces : s->dev + ((size_t)gm.left[1] * gm.shape[0] + gm.left[0]) * nch;
  const size_t dst_pitch = cube ? size_t(w) : size_t(gm.shape[0]);
  const size_t row_bytes = size_t(w) * nch * sizeof(float), pitch_bytes = dst_pitch * nch * sizeof(float);
  if (e == hipSuccess) {
    eu_alpha_params p {};            // the edit, where it runs: src (src_ch channels, dense) -> the plane
    p.src = static_cast<const float *>(src); p.dst = dst;
    p.src_pitch = size_t(w); p.dst_pitch = dst_pitch;
    p.w = w; p.h = h; p.nch = nch; p.src_ch = src_ch;
    if (feed.kind == FEED_HOST_FLOATS) {
      e = cube ? hipMemcpyAsync(dst, src, npix * nch * sizeof(float), hipMemcpyHostToDevice, st)
               : hipMemcpy2DAsync(dst, pitch_bytes, src, row_bytes, row_bytes, size_t(h), hipMemcpyHostToDevice, st);
    } else if (feed.kind == FEED_EDITED_FLOATS) {
      if (!feed.alter)
        e = hipMemcpy2DAsync(dst, pitch_bytes, src, row_bytes, row_bytes, size_t(h), hipMemcpyDeviceToDevice, st);
    } else if (feed.kind == FEED_RGBE) {
      // quads -> floats, as the samples below: into the plane, or into the dense buffer the edit reads
      eu_rgbe_decode_params d {};
      d.src = static_cast<const uint32_t *>(src);
      d.table = feed.rgbe_table ? tab : nullptr;
      d.dst = feed.alter ? staged : dst;
      d.dst_pitch = feed.alter ? size_t(w) : dst_pitch;
      d.w = w; d.h = h; d.nch = feed.alter ? src_ch : nch;
      if (eu_launch_rgbe_decode(&d, st)) prc = fail(EU_ERR_NO_DEVICE, who + ": kernel launch failed");
      if (feed.alter) p.src = staged;
    } else if (feed.kind == FEED_YCBCR) {
      // planes -> floats, as the quads above
      const eu_ycbcr &y = *feed.ycc;
      yd.tables = tab;
      yd.dst = feed.alter ? staged : dst;
      yd.dst_pitch = feed.alter ? size_t(w) : dst_pitch;
      yd.w = w; yd.h = h; yd.nch = feed.alter ? src_ch : nch;
      yd.bits = y.bits; yd.c_step = y.c_step; yd.sub_x = y.sub_x; yd.sub_y = y.sub_y;
      yd.m_rv = y.m_rv; yd.m_gu = y.m_gu; yd.m_gv = y.m_gv; yd.m_bu = y.m_bu;
      if (eu_launch_ycbcr_decode(&yd, st)) prc = fail(EU_ERR_NO_DEVICE, who + ": kernel launch failed");
      if (feed.alter) p.src = staged;
    } else {
      // samples -> floats: straight into the plane, or into the dense buffer the edit reads as it reads
      // pixels_on_device input (the channel a facet gains is then the edit's work)
      eu_decode_params d {};
      d.src = src; d.tables = tab;
      d.dst = feed.alter ? staged : dst;
      d.dst_pitch = feed.alter ? size_t(w) : dst_pitch;
      d.w = w; d.h = h; d.bits = feed.smp->bits; d.big_endian = feed.smp->big_endian != 0;
      d.nch = feed.alter ? src_ch : nch; d.src_ch = src_ch;
      if (eu_launch_decode(&d, st)) prc = fail(EU_ERR_NO_DEVICE, who + ": kernel launch failed");
      if (feed.alter) p.src = staged;
    }
    if (feed.alter && !prc) {
      prc = upload_alpha_plan(feed.edit, w, h, &p);
      if (!prc && eu_launch_facet_alpha(&p, st)) prc = fail(EU_ERR_NO_DEVICE, who + ": kernel launch failed");
    }
  }
  // the distance plane of a source that keeps one (EU_LOAD_EDGES; never a cubemap): from the alpha channel of the plane
  // as the prefilter is about to read it, behind the edit and in front of the finish
  if (e == hipSuccess && !prc && s->edge) {
    eu_edges_params ep {};
    ep.plane = dst; ep.pitch = dst_pitch; ep.w = w; ep.h = h; ep.nch = nch;
    ep.cyclic = s->bc[0] == EU_BC_PERIODIC;
    ep.dist = s->edge;
    e = sc.edges(npix, &ep.scratch);
    if (e == hipSuccess && eu_launch_edges(&ep, st)) prc = fail(EU_ERR_NO_DEVICE, who + ": kernel launch failed");
  }
  // the finish: the IR image of a cubemap from its faces, or prefilter + brace of the container (a core narrower
  // than the spline's frame on an axis is braced slice by slice in zimt's order, eu_setup.hip: brace_seq_kernel)
  if (e == hipSuccess && !prc)
    rc = cube ? eu_launch_cubemap_build(faces, s->dev, nch, m.face_px, m.section_px, m.left_frame_px, m.right_frame_px,
                                        m.refc_md, m.model_to_px, prefilter_degree, iir_stream, st)
              // (a load's full sphere is always PERIODIC - source_bcs; the second condition is there for a source that
              // eu_hip_source_adopt made with other boundary conditions, which a refill keeps)
              : eu_launch_prefilter(s->dev, &s->geom, nch, s->bc[0], s->bc[1], prefilter_degree,
                                    full_sphere(fct) && s->bc[0] == EU_BC_PERIODIC, iir_stream, st);
  return { e, rc, prc };
}

// the precedence of a fill's errors: the plan's upload or a kernel launch (the message is set), the HIP error, the finish
int fill_status(const fill_result &r, hipError_t e2)
{
  const hipError_t e = r.e != hipSuccess ? r.e : e2;
  if (r.prc) return r.prc;
  if (e != hipSuccess) return fail(EU_ERR_NO_DEVICE, hipGetErrorString(e));
  if (r.rc) return fail(r.rc, "device set-up stage failed");
  return EU_OK;
}

// flags: eu_hip_source_load_pixels' (EU_LOAD_EDGES: the source gets its distance plane, which fill_source then fills)
int load_source(const eu_facet *fct, int spline_degree, int prefilter_degree, int support_min, int tile_size,
                const load_feed &feed, unsigned flags, eu_source **out)
{
  int rc, bc0, bc1;
  source_bcs(fct, &bc0, &bc1);
  eu_source *s = nullptr;
  if ((rc = new_source(fct, spline_degree, bc0, bc1, support_min, tile_size, &s))) return rc;
  if (flags & EU_LOAD_EDGES) {
    const hipError_t ee = hipMalloc((void **)&s->edge, size_t(fct->window_width) * size_t(fct->window_height) * sizeof(float));
    if (ee != hipSuccess) {
      s->edge = nullptr;
      destroy_source(s);
      return fail(EU_ERR_MEMORY, std::string("hipMalloc: ") + hipGetErrorString(ee));
    }
  }
  fill_scratch sc(false);            // freed by scope, after the synchronisation
  const fill_result r = fill_source(s, prefilter_degree, feed, cur().stream, sc);
  rc = fill_status(r, hipStreamSynchronize(cur().stream));
  if (rc) { destroy_source(s); return rc; }
  *out = s;
  return EU_OK;
}

// ---- what the feeds' entry points refuse, for a load and for a reload alike (`who` names the entry point) ----------

// *ed: the edit as given, with the samples' channel count in place of its own; *edited: masks or a crop
int check_samples_feed(const std::string &who, int nch, const eu_samples *smp, const eu_facet_edit *edit,
                       eu_facet_edit *ed, bool *edited)
{
  int rc;
  if (smp->bits != 8 && smp->bits != 16) return fail(EU_ERR_ARGUMENT, who + ": bits must be 8 or 16");
  if (!smp->colour_table) return fail(EU_ERR_ARGUMENT, who + ": null colour table");
  *ed = eu_facet_edit {};
  if (edit) *ed = *edit;
  ed->pixel_channels = smp->pixel_channels;
  ed->pixels_on_device = 0;
  bool asked;
  if ((rc = check_edit(ed, nch, who.c_str(), &asked))) return rc;
  if (smp->on_device && smp->bits == 16 && reinterpret_cast<uintptr_t>(smp->data) % 2)
    return fail(EU_ERR_ARGUMENT, who + ": 16-bit samples on the device lie at an even address");
  *edited = ed->npolygons > 0 || ed->crop_kind != 0;     // the alpha plane is wanted, not only the new channel
  return EU_OK;
}

// the same for quads: three channels in place of the edit's own
int check_rgbe_feed(const std::string &who, int nch, const eu_rgbe *px, const eu_facet_edit *edit, eu_facet_edit *ed,
                    bool *edited)
{
  int rc;
  if (nch != 3 && nch != 4)
    return fail(EU_ERR_ARGUMENT, who + ": a facet of RGBE pixels has 3 channels, or 4 where it gains alpha");
  *ed = eu_facet_edit {};
  if (edit) *ed = *edit;
  ed->pixel_channels = 3;
  ed->pixels_on_device = 0;
  bool asked;
  if ((rc = check_edit(ed, nch, who.c_str(), &asked))) return rc;
  if (px->on_device && reinterpret_cast<uintptr_t>(px->data) % 4)
    return fail(EU_ERR_ARGUMENT, who + ": quads on the device lie on a 4-byte boundary");
  *edited = ed->npolygons > 0 || ed->crop_kind != 0;
  return EU_OK;
}

// the planes of a w x h frame, whatever is done with them (eu_hip_ycbcr_floats too)
int check_ycbcr_planes(const std::string &who, const eu_ycbcr *px, int w, int h)
{
  if (!px) return fail(EU_ERR_ARGUMENT, who + ": null ycbcr");
  if (!px->y || !px->cb || !px->cr) return fail(EU_ERR_ARGUMENT, who + ": null plane (y, cb, cr)");
  if (!px->y_table || !px->c_table) return fail(EU_ERR_ARGUMENT, who + ": null table (y_table, c_table)");
  if (px->bits != 8 && px->bits != 16) return fail(EU_ERR_ARGUMENT, who + ": bits must be 8 or 16");
  if (px->c_step != 1 && px->c_step != 2) return fail(EU_ERR_ARGUMENT, who + ": c_step must be 1 or 2");
  if (px->sub_x != 1 && px->sub_x != 2) return fail(EU_ERR_ARGUMENT, who + ": sub_x must be 1 or 2");
  if (px->sub_y != 1 && px->sub_y != 2) return fail(EU_ERR_ARGUMENT, who + ": sub_y must be 1 or 2");
  if (w <= 0 || h <= 0) return fail(EU_ERR_ARGUMENT, who + ": empty frame (width, height)");
  const size_t sb = size_t(px->bits / 8), cw = (size_t(w) + px->sub_x - 1) / px->sub_x;
  if (px->y_pitch < size_t(w) * sb) return fail(EU_ERR_ARGUMENT, who + ": y_pitch shorter than a row of luma samples");
  if (px->c_pitch < ((cw - 1) * px->c_step + 1) * sb)
    return fail(EU_ERR_ARGUMENT, who + ": c_pitch shorter than a row of chroma samples");
  if (px->bits == 16 && ((reinterpret_cast<uintptr_t>(px->y) | reinterpret_cast<uintptr_t>(px->cb) |
                          reinterpret_cast<uintptr_t>(px->cr)) & 1))
    return fail(EU_ERR_ARGUMENT, who + ": 16-bit planes (y, cb, cr) lie at even addresses");
  if (px->bits == 16 && ((px->y_pitch | px->c_pitch) & 1))
    return fail(EU_ERR_ARGUMENT, who + ": 16-bit planes have even pitches (y_pitch, c_pitch)");
  return EU_OK;
}

// the frame a facet's container takes: its window, or the stack of a cubemap's six faces
void facet_frame(const eu_facet *f, int *w, int *h)
{
  const bool cube = eu_cube_source(f->projection);
  *w = cube ? f->width : f->window_width;
  *h = cube ? 6 * f->width : f->window_height;
}

int check_ycbcr_feed(const std::string &who, const eu_facet *fct, const eu_ycbcr *px, const eu_facet_edit *edit,
                     eu_facet_edit *ed, bool *edited)
{
  int rc, w, h;
  if (fct->nchannels != 3 && fct->nchannels != 4)
    return fail(EU_ERR_ARGUMENT, who + ": a facet of YCbCr pixels has 3 channels (nchannels), or 4 where it gains alpha");
  facet_frame(fct, &w, &h);
  if ((rc = check_ycbcr_planes(who, px, w, h))) return rc;
  *ed = eu_facet_edit {};
  if (edit) *ed = *edit;
  ed->pixel_channels = 3;
  ed->pixels_on_device = 0;
  bool asked;
  if ((rc = check_edit(ed, fct->nchannels, who.c_str(), &asked))) return rc;
  *edited = ed->npolygons > 0 || ed->crop_kind != 0;
  return EU_OK;
}

}  // namespace

extern "C" {

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

static int load_flagged(const eu_facet *fct, const float *pixels, int spline_degree,
                       int prefilter_degree, int support_min, int tile_size, unsigned flags, eu_source **out)
{
  int rc;
  if ((rc = ensure_init())) return rc;
  if ((rc = check_facet(fct))) return rc;
  if (!pixels || !out) return fail(EU_ERR_ARGUMENT, "null argument");
  if (prefilter_degree < 0 || prefilter_degree > EU_MAX_DEGREE)
    return fail(EU_ERR_ARGUMENT, "prefilter degree out of range");
  const load_feed feed { FEED_HOST_FLOATS, "source_load", pixels, false, fct->nchannels, nullptr, false, nullptr, nullptr, nullptr };
  return load_source(fct, spline_degree, prefilter_degree, support_min, tile_size, feed, flags, out);
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
  hipStream_t st = stream ? (hipStream_t)stream : cur().stream;
  if (eu_launch_facet_alpha(&p, st)) return fail(EU_ERR_NO_DEVICE, "facet_alpha_dev: kernel launch failed");
  return note_caller(cur().alpha.readers, stream, EU_OK);
}

static int load_edited_flagged(const eu_facet *fct, const void *pixels, const eu_facet_edit *edit, int spline_degree,
                              int prefilter_degree, int support_min, int tile_size, unsigned flags, eu_source **out)
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
    return load_flagged(fct, static_cast<const float *>(pixels), spline_degree, prefilter_degree, support_min, tile_size,
                        flags, out);
  if ((rc = ensure_init())) return rc;
  const load_feed feed { FEED_EDITED_FLOATS, "source_load_edited", pixels, on_device, edit->pixel_channels, edit, asked, nullptr, nullptr, nullptr };
  return load_source(fct, spline_degree, prefilter_degree, support_min, tile_size, feed, flags, out);
}

static int load_samples_flagged(const eu_facet *fct, const eu_samples *smp, const eu_facet_edit *edit, int spline_degree,
                               int prefilter_degree, int support_min, int tile_size, unsigned flags, eu_source **out)
{
  int rc;
  if ((rc = check_facet(fct))) return rc;
  if (!smp || !smp->data || !out) return fail(EU_ERR_ARGUMENT, "null argument");
  eu_facet_edit ed;
  bool edited;
  if ((rc = check_samples_feed("source_load_samples", fct->nchannels, smp, edit, &ed, &edited))) return rc;
  if (spline_degree < 0 || spline_degree > EU_MAX_DEGREE) return fail(EU_ERR_ARGUMENT, "spline degree out of range");
  if (prefilter_degree < 0 || prefilter_degree > EU_MAX_DEGREE)
    return fail(EU_ERR_ARGUMENT, "prefilter degree out of range");
  if ((rc = ensure_init())) return rc;
  const load_feed feed { FEED_SAMPLES, "source_load_samples", smp->data, smp->on_device != 0, smp->pixel_channels, &ed, edited, smp, nullptr, nullptr };
  return load_source(fct, spline_degree, prefilter_degree, support_min, tile_size, feed, flags, out);
}

static int load_rgbe_flagged(const eu_facet *fct, const eu_rgbe *px, const eu_facet_edit *edit, int spline_degree,
                            int prefilter_degree, int support_min, int tile_size, unsigned flags, eu_source **out)
{
  int rc;
  if ((rc = check_facet(fct))) return rc;
  if (!px || !px->data || !out) return fail(EU_ERR_ARGUMENT, "null argument");
  eu_facet_edit ed;
  bool edited;
  if ((rc = check_rgbe_feed("source_load_rgbe", fct->nchannels, px, edit, &ed, &edited))) return rc;
  if (spline_degree < 0 || spline_degree > EU_MAX_DEGREE) return fail(EU_ERR_ARGUMENT, "spline degree out of range");
  if (prefilter_degree < 0 || prefilter_degree > EU_MAX_DEGREE)
    return fail(EU_ERR_ARGUMENT, "prefilter degree out of range");
  if ((rc = ensure_init())) return rc;
  const load_feed feed { FEED_RGBE, "source_load_rgbe", px->data, px->on_device != 0, 3, &ed, edited, nullptr, px->colour_table, nullptr };
  return load_source(fct, spline_degree, prefilter_degree, support_min, tile_size, feed, flags, out);
}

static int load_ycbcr_flagged(const eu_facet *fct, const eu_ycbcr *px, const eu_facet_edit *edit, int spline_degree,
                             int prefilter_degree, int support_min, int tile_size, unsigned flags, eu_source **out)
{
  int rc;
  if ((rc = check_facet(fct))) return rc;
  if (!px || !out) return fail(EU_ERR_ARGUMENT, "null argument");
  eu_facet_edit ed;
  bool edited;
  if ((rc = check_ycbcr_feed("source_load_ycbcr", fct, px, edit, &ed, &edited))) return rc;
  if (spline_degree < 0 || spline_degree > EU_MAX_DEGREE) return fail(EU_ERR_ARGUMENT, "spline degree out of range");
  if (prefilter_degree < 0 || prefilter_degree > EU_MAX_DEGREE)
    return fail(EU_ERR_ARGUMENT, "prefilter degree out of range");
  if ((rc = ensure_init())) return rc;
  const load_feed feed { FEED_YCBCR, "source_load_ycbcr", px->y, px->on_device != 0, 3, &ed, edited, nullptr, nullptr, px };
  return load_source(fct, spline_degree, prefilter_degree, support_min, tile_size, feed, flags, out);
}

// The five loads of the ABI, as they have always been: the bodies above without flags.
int eu_hip_source_load(const eu_facet *fct, const float *pixels, int spline_degree,
                       int prefilter_degree, int support_min, int tile_size, eu_source **out)
{
  return load_flagged(fct, pixels, spline_degree, prefilter_degree, support_min, tile_size, 0u, out);
}
int eu_hip_source_load_edited(const eu_facet *fct, const void *pixels, const eu_facet_edit *edit, int spline_degree,
                              int prefilter_degree, int support_min, int tile_size, eu_source **out)
{
  return load_edited_flagged(fct, pixels, edit, spline_degree, prefilter_degree, support_min, tile_size, 0u, out);
}
int eu_hip_source_load_samples(const eu_facet *fct, const eu_samples *smp, const eu_facet_edit *edit, int spline_degree,
                               int prefilter_degree, int support_min, int tile_size, eu_source **out)
{
  return load_samples_flagged(fct, smp, edit, spline_degree, prefilter_degree, support_min, tile_size, 0u, out);
}
int eu_hip_source_load_rgbe(const eu_facet *fct, const eu_rgbe *px, const eu_facet_edit *edit, int spline_degree,
                            int prefilter_degree, int support_min, int tile_size, eu_source **out)
{
  return load_rgbe_flagged(fct, px, edit, spline_degree, prefilter_degree, support_min, tile_size, 0u, out);
}
int eu_hip_source_load_ycbcr(const eu_facet *fct, const eu_ycbcr *px, const eu_facet_edit *edit, int spline_degree,
                             int prefilter_degree, int support_min, int tile_size, eu_source **out)
{
  return load_ycbcr_flagged(fct, px, edit, spline_degree, prefilter_degree, support_min, tile_size, 0u, out);
}

// One load for every feed (eu_hip.h, "feathering to alpha edges"): the flags' own refusals, then the matching load's
// body - its checks, in its order, with its messages.
int eu_hip_source_load_pixels(const eu_facet *fct, const eu_pixels *px, int spline_degree, int prefilter_degree,
                              int support_min, int tile_size, unsigned flags, eu_source **out)
{
  int rc;
  if ((rc = check_facet(fct))) return rc;
  if (!px) return fail(EU_ERR_ARGUMENT, "source_load_pixels: null pixels (px)");
  if (flags & ~unsigned(EU_LOAD_EDGES)) return fail(EU_ERR_ARGUMENT, "source_load_pixels: unknown flag bit (flags)");
  if (flags & EU_LOAD_EDGES) {
    if (eu_cube_source(fct->projection))
      return fail(EU_ERR_ARGUMENT, "source_load_pixels: EU_LOAD_EDGES on a cubemap: a distance plane belongs to a facet with a window");
    if (fct->nchannels != 2 && fct->nchannels != 4)
      return fail(EU_ERR_ARGUMENT, "source_load_pixels: EU_LOAD_EDGES needs an alpha channel: nchannels 2 or 4");
    if (fct->window_width > EU_EDGES_MAX_SIDE || fct->window_height > EU_EDGES_MAX_SIDE)
      return fail(EU_ERR_ARGUMENT, "source_load_pixels: EU_LOAD_EDGES on a window side above 32768 (window_width, window_height)");
    if (fct->window_width < 1 || fct->window_height < 1)
      return fail(EU_ERR_ARGUMENT, "source_load_pixels: EU_LOAD_EDGES on an empty window (window_width, window_height)");
  }
  switch (px->kind) {
    case EU_PX_FLOATS: {
      eu_facet_edit ed {};
      if (px->edit) ed = *px->edit;
      ed.pixel_channels = px->pixel_channels;
      ed.pixels_on_device = px->on_device;
      return load_edited_flagged(fct, px->floats, &ed, spline_degree, prefilter_degree, support_min, tile_size, flags, out);
    }
    case EU_PX_SAMPLES:
      return load_samples_flagged(fct, px->samples, px->edit, spline_degree, prefilter_degree, support_min, tile_size, flags, out);
    case EU_PX_RGBE:
      return load_rgbe_flagged(fct, px->rgbe, px->edit, spline_degree, prefilter_degree, support_min, tile_size, flags, out);
    case EU_PX_YCBCR:
      return load_ycbcr_flagged(fct, px->ycbcr, px->edit, spline_degree, prefilter_degree, support_min, tile_size, flags, out);
  }
  return fail(EU_ERR_ARGUMENT, "source_load_pixels: unknown kind (px->kind)");
}

int eu_hip_source_has_edges(const eu_source *src) { return src && src->edge ? 1 : 0; }

int eu_hip_source_edge_device_ptr(const eu_source *src, void **dev_ptr)
{
  if (!src) return fail(EU_ERR_HANDLE, "null source");
  if (dev_ptr) *dev_ptr = src->edge;
  return EU_OK;
}

int eu_hip_source_edge_distance(const eu_source *src, float *out, size_t row_stride_bytes, int out_on_device, void *stream)
{
  if (!src) return fail(EU_ERR_HANDLE, "source_edge_distance: null source (src)");
  if (!out) return fail(EU_ERR_ARGUMENT, "source_edge_distance: null out");
  if (!src->edge)
    return fail(EU_ERR_ARGUMENT, "source_edge_distance: the source keeps no distance plane: it was not loaded with EU_LOAD_EDGES");
  const size_t w = size_t(src->fct.window_width), h = size_t(src->fct.window_height), row = w * sizeof(float);
  if (row_stride_bytes < row || row_stride_bytes % sizeof(float))
    return fail(EU_ERR_ARGUMENT, "source_edge_distance: row_stride_bytes is a multiple of 4 and at least a row");
  int rc;
  if ((rc = ensure_init())) return rc;
  const int back = cur_slot_;
  if (src->slot != back && (rc = set_slot(src->slot))) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : cur().stream;
  // behind the reload that may still be writing the plane, on a caller's stream or on the library's own
  hipError_t e = hipSuccess;
  if (src->own_written && st != cur().stream) e = hipStreamSynchronize(cur().stream);
  if (e == hipSuccess) e = src->written.order_after(st);
  if (e == hipSuccess)
    e = hipMemcpy2DAsync(out, row_stride_bytes, src->edge, row, row, h, out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && !out_on_device) e = hipStreamSynchronize(st);
  if (src->slot != back && (rc = set_slot(back))) return rc;
  if (e != hipSuccess) return fail(EU_ERR_NO_DEVICE, std::string("source_edge_distance: ") + hipGetErrorString(e));
  // a copy left on a caller's stream reads the plane as a render reads the container
  return out_on_device ? note_caller(const_cast<eu_source *>(src)->readers, stream, EU_OK) : EU_OK;
}

int eu_hip_ycbcr_floats(const eu_ycbcr *px, int width, int height, int nchannels, float *out)
{
  int rc;
  if ((rc = check_ycbcr_planes("ycbcr_floats", px, width, height))) return rc;
  if (nchannels != 3 && nchannels != 4) return fail(EU_ERR_ARGUMENT, "ycbcr_floats: nchannels must be 3 or 4");
  if (!out) return fail(EU_ERR_ARGUMENT, "ycbcr_floats: null out");
  if (px->on_device) return fail(EU_ERR_ARGUMENT, "ycbcr_floats: a host function, on_device must be 0");
  eu_ycbcr_rows(px->y, px->cb, px->cr, px->y_pitch, px->c_pitch, px->c_step, px->sub_x, px->sub_y, px->bits, px->y_table,
                px->c_table, px->m_rv, px->m_gu, px->m_gv, px->m_bu, width, height, nchannels, out);
  return EU_OK;
}

// New pixels into a resident container: fill_source without new_source. Stream order ("A source refilled
// in place"): `st` goes behind the renders that read the container, behind earlier reloads of it and of the scratch,
// and behind the library's own stream; behind the call stands `written` (and reload.readers) on a caller's stream,
// own_written on the library's own.
int eu_hip_source_reload(eu_source *src, const eu_pixels *px, int prefilter_degree, void *stream)
{
  int rc;
  if (!src) return fail(EU_ERR_HANDLE, "source_reload: null source (src)");
  if (src->is_replica) return fail(EU_ERR_HANDLE, "source_reload: src is a copy on another device slot (is_replica): reload the original");
  if (!px) return fail(EU_ERR_ARGUMENT, "source_reload: null pixels (px)");
  const eu_facet *fct = &src->fct;
  const int nch = src->nch;
  eu_facet_edit ed {};
  bool edited = false;
  load_feed feed { FEED_HOST_FLOATS, "source_reload", nullptr, false, nch, nullptr, false, nullptr, nullptr, nullptr };
  switch (px->kind) {
    case EU_PX_FLOATS: {
      if (!px->floats) return fail(EU_ERR_ARGUMENT, "source_reload: null floats");
      if (px->edit) ed = *px->edit;
      ed.pixel_channels = px->pixel_channels;
      ed.pixels_on_device = px->on_device;
      bool asked;
      if ((rc = check_edit(&ed, nch, "source_reload", &asked))) return rc;
      feed.data = px->floats; feed.on_device = px->on_device != 0; feed.src_ch = px->pixel_channels;
      if (asked || feed.on_device) { feed.kind = FEED_EDITED_FLOATS; feed.edit = &ed; feed.alter = asked; }
      edited = asked;
      break;
    }
    case EU_PX_SAMPLES:
      if (!px->samples) return fail(EU_ERR_ARGUMENT, "source_reload: kind EU_PX_SAMPLES without samples");
      if (!px->samples->data) return fail(EU_ERR_ARGUMENT, "source_reload: null samples->data");
      if ((rc = check_samples_feed("source_reload", nch, px->samples, px->edit, &ed, &edited))) return rc;
      feed = load_feed { FEED_SAMPLES, "source_reload", px->samples->data, px->samples->on_device != 0,
                         px->samples->pixel_channels, &ed, edited, px->samples, nullptr, nullptr };
      break;
    case EU_PX_RGBE:
      if (!px->rgbe) return fail(EU_ERR_ARGUMENT, "source_reload: kind EU_PX_RGBE without rgbe");
      if (!px->rgbe->data) return fail(EU_ERR_ARGUMENT, "source_reload: null rgbe->data");
      if ((rc = check_rgbe_feed("source_reload", nch, px->rgbe, px->edit, &ed, &edited))) return rc;
      feed = load_feed { FEED_RGBE, "source_reload", px->rgbe->data, px->rgbe->on_device != 0, 3, &ed, edited, nullptr,
                         px->rgbe->colour_table, nullptr };
      break;
    case EU_PX_YCBCR:
      if (!px->ycbcr) return fail(EU_ERR_ARGUMENT, "source_reload: kind EU_PX_YCBCR without ycbcr");
      if ((rc = check_ycbcr_feed("source_reload", fct, px->ycbcr, px->edit, &ed, &edited))) return rc;
      feed = load_feed { FEED_YCBCR, "source_reload", px->ycbcr->y, px->ycbcr->on_device != 0, 3, &ed, edited, nullptr,
                         nullptr, px->ycbcr };
      break;
    default:
      return fail(EU_ERR_ARGUMENT, "source_reload: unknown kind");
  }
  if (prefilter_degree < 0 || prefilter_degree > EU_MAX_DEGREE)
    return fail(EU_ERR_ARGUMENT, "source_reload: prefilter degree out of range (prefilter_degree)");
  if ((rc = ensure_init())) return rc;
  if (!src->dev) return fail(EU_ERR_HANDLE, "source_reload: the source has no container (src)");
  if (src->slot != cur_slot_) return fail(EU_ERR_HANDLE, "source_reload: the source lives on another device slot (src)");
  // copies on other device slots: their renders are through (eu_hip_render_devices waits for every slot); they go,
  // and eu_hip_render_devices makes them again from the new content
  for (int k = 0; k < EU_MAX_SLOTS; k++)
    if (src->replica[k]) {
      if (ctx_[k].stream) {
        const int back = cur_slot_;
        if ((rc = set_slot(k))) return rc;
        const hipError_t es = hipStreamSynchronize(cur().stream);
        if ((rc = set_slot(back))) return rc;
        if (es != hipSuccess) return fail(EU_ERR_NO_DEVICE, std::string("source_reload: replica: ") + hipGetErrorString(es));
      }
      destroy_source(src->replica[k]);
      src->replica[k] = nullptr;
    }
  context &c = cur();
  hipStream_t st = stream ? (hipStream_t)stream : c.stream;
  // behind everything that reads or wrote the container and the scratch
  HIPCHK(src->readers.order_after(st));
  HIPCHK(src->written.order_after(st));
  HIPCHK(c.reload.readers.order_after(st));
  if (stream) {
    // the library's own stream leaves no event of its own accord: a mark on it, which `st` waits for - not the host
    HIPCHK(c.reload.own.note(c.stream));
    HIPCHK(c.reload.own.order_after(st));
  }
  fill_scratch sc(true);
  const fill_result r = fill_source(src, prefilter_degree, feed, st, sc);
  // host pixels must not be read after the call, an edit's plan is the next edit's to rewrite, and a failure is
  // reported when it has happened: those calls wait. Device pixels without masks or a crop stay queued.
  const bool wait = !feed.on_device || feed.alter || r.e != hipSuccess || r.rc || r.prc;
  rc = fill_status(r, wait ? hipStreamSynchronize(st) : hipSuccess);
  if (stream) {
    rc = note_caller(src->written, stream, rc);
    rc = note_caller(c.reload.readers, stream, rc);
  } else if (!wait) src->own_written = true;
  if (rc) return fail(rc, g_err + " (source_reload: the handle stays valid, the container's content is unspecified)");
  return EU_OK;
}

int eu_hip_reload_scratch_release(void)
{
  for (int k = 0; k < nslots_; k++) {
    context &c = ctx_[k];
    if (c.device < 0) continue;
    if (!c.reload.tables.dev.p && !c.reload.block.p && !c.reload.staged.p && !c.reload.faces.p && !c.reload.edges.p) continue;
    const int back = cur_slot_;
    int rc;
    if ((rc = set_slot(k))) return rc;
    hipError_t e = c.reload.readers.host_wait();
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    auto drop = [&](auto &b) { if (b.p) { const hipError_t f = hipFree(b.p); if (e == hipSuccess) e = f; } b.p = nullptr; b.cap = 0; };
    drop(c.reload.tables.dev); drop(c.reload.block); drop(c.reload.staged); drop(c.reload.faces); drop(c.reload.edges);
    c.reload.tables.host.clear();
    if ((rc = set_slot(back))) return rc;
    if (e != hipSuccess) return fail(EU_ERR_NO_DEVICE, std::string("reload_scratch_release: ") + hipGetErrorString(e));
  }
  return EU_OK;
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
  // a reload may still be filling the container, on a caller's stream or on the library's own: the handle alone is safe
  HIPCHK(src->written.host_wait());
  if (src->own_written) HIPCHK(hipStreamSynchronize(ctx_[src->slot].stream));
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
  // whoever still reads or refills the container on a caller's stream is waited for by the events it left (hipFree
  // waits for the device as well; this says so)
  if (src->dev) { (void)src->readers.host_wait(); (void)src->written.host_wait(); }
  for (int k = 0; k < EU_MAX_SLOTS; k++) destroy_source(src->replica[k]);
  destroy_source(src);
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

// DIAGNOSTIC (not declared in eu_hip.h): the same handle marked as a copy on another device slot, which only
// eu_hip_render_devices makes - so that what the entry points refuse of such a handle can be exercised without a device
int eu_hip_diag_host_replica(const eu_facet *fct, int spline_degree, eu_source **out)
{
  const int rc = eu_hip_diag_host_source(fct, spline_degree, out);
  if (rc == EU_OK) (*out)->is_replica = true;
  return rc;
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
  const int lrc = eu_launch_diag_coords(&src->sd, d, n, variant, d + (size_t)n * 3, cur().stream);
  if (lrc > 0) return fail(EU_ERR_UNSUPPORTED, "the packed forms cover lat/lon, cubemap and biatan6 sources");
  if (lrc < 0) return fail(EU_ERR_NO_DEVICE, "diag launch failed");
  HIPCHK(hipStreamSynchronize(cur().stream));
  HIPCHK(hipMemcpy(out, d + (size_t)n * 3, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost));
  return EU_OK;
}

}  // extern "C"
