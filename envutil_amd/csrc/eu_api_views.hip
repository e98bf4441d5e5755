// C ABI (include/eu_hip.h), host glue: many views of one resident source, or of a multi-facet job, in one call
// (eu_render_views.hip, eu_render_views_multi.hip).

#include "eu_context.h"
#include "eu_setup_math.h"

using namespace eu_host;

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
  if (cur().views.taps.holds(keep->data(), keep->size())) return EU_OK;
  cur().views.taps.host.clear();
  HIPCHK(cur().views.taps.dev.reserve(keep->size()));
  HIPCHK(hipMemcpyAsync(cur().views.taps.dev.p, keep->data(), keep->size() * sizeof(float), hipMemcpyHostToDevice, st));
  cur().views.taps.host = *keep;
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
// synchronising upload, and the chunk loop with its device or staged output. The buffers are the context's
// `views`, `src` among them for the facets' parameter blocks of a multi-facet job; none of build_multi's is touched.
// `who` is the entry point that messages name where they always have.
// `job` is what the entry point supplies:
//   job.prepare(form, norm_mode, sw)   once, when the buffers stand: the kernel parameters of the call
//   job.launch(nv, vs, sw, st)         renders nv views from the tables in views.col / views.row to job.p.out, rows
//                                      job.p.out_stride apart; nonzero: the launch failed
template <class JOB>
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
  hipStream_t st = stream ? (hipStream_t)stream : cur().stream;

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
  const bool feather = multi && trg->synopsis == EU_SYN_FEATHER;
  const std::vector<eu_feather_dev> fth = feather ? feather_table(trg, srcs, nsrc) : std::vector<eu_feather_dev>();
  std::vector<float> taps;
  drain drain_on_exit{ st, st };          // the host vectors above are among what the call lets go of
  // the view buffers are rewritten on `st`, and reserve() may free them: the view calls before this one have to be
  // through, on callers' streams (the event) and on the library's own. The host waits, as it always has here
  HIPCHK(cur().views.readers.host_wait());
  if (stream) HIPCHK(hipStreamSynchronize(cur().stream));
  HIPCHK(cur().views.col.reserve(col_floats * per_chunk));
  HIPCHK(cur().views.row.reserve(row_floats * per_chunk));
  if (!out_on_device) HIPCHK(cur().views.stage.reserve((size_t)per_chunk * frame_bytes / sizeof(float)));
  if ((rc = order_sources(srcs, nsrc, st))) return rc;      // behind a reload of a source
  // the one host synchronisation of the call: the scalar blocks, the facets, and a new tap table, in flight from host vectors
  HIPCHK(cur().views.scal.reserve(sc.size()));
  if (multi) HIPCHK(cur().views.src.reserve(sd.size()));
  HIPCHK(hipMemcpyAsync(cur().views.scal.p, sc.data(), sc.size() * sizeof(eu_view_dev), hipMemcpyHostToDevice, st));
  if (multi) HIPCHK(hipMemcpyAsync(cur().views.src.p, sd.data(), sd.size() * sizeof(eu_src_dev), hipMemcpyHostToDevice, st));
  if (feather) {
    HIPCHK(cur().views.fth.reserve(fth.size()));
    HIPCHK(hipMemcpyAsync(cur().views.fth.p, fth.data(), fth.size() * sizeof(eu_feather_dev), hipMemcpyHostToDevice, st));
  }
  if ((rc = upload_view_taps(trg, st, &taps))) return rc;
  HIPCHK(hipStreamSynchronize(st));

  eu_view_strides vs;
  vs.col = (long long)col_floats; vs.row = (long long)row_floats;
  vs.out = (long long)((out_on_device ? out_view_stride_bytes : frame_bytes) / sizeof(float));
  job.prepare(form, norm_mode, sw);
  job.p.out_stride = (long long)((out_on_device ? out_row_stride_bytes : row_bytes) / sizeof(float));
  for (int c0 = 0; c0 < nviews; c0 += per_chunk) {
    const int nv = std::min(per_chunk, nviews - c0);
    if (eu_launch_view_tables(cur().views.scal.p + (size_t)c0 * nsrc, nv * nsrc, trg->projection, W, H, trg->ntaps > 0,
                              cur().views.col.p, cur().views.row.p, st))
      return fail(EU_ERR_NO_DEVICE, std::string(who) + ": table kernel launch failed");
    char *dst = (char *)out + (size_t)c0 * out_view_stride_bytes;
    job.p.out = out_on_device ? (float *)dst : cur().views.stage.p;
    if (job.launch(nv, vs, sw, st))
      return fail(EU_ERR_NO_DEVICE, std::string(who) + ": kernel launch failed");
    if (!out_on_device)
      for (int k = 0; k < nv; k++)
        HIPCHK(hipMemcpy2DAsync(dst + (size_t)k * out_view_stride_bytes, out_row_stride_bytes,
                                (const char *)cur().views.stage.p + (size_t)k * frame_bytes, row_bytes, row_bytes, (size_t)H,
                                hipMemcpyDeviceToHost, st));
  }
  if (!out_on_device) HIPCHK(hipStreamSynchronize(st));
  drain_on_exit.on = false;          // a device output stays queued: `st` goes on reading the view buffers
  return note_readers(cur().views.readers, srcs, nsrc, out_on_device ? stream : nullptr, EU_OK);
}

extern "C" {

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
      p.col = cur().views.col.p; p.row = cur().views.row.p; p.taps = cur().views.taps.dev.p;
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
  if (trg->synopsis == EU_SYN_MULTIBAND)
    return fail(EU_ERR_ARGUMENT, "render_views_multi: no multiband synopsis - a pyramid per view is a job per view, call eu_hip_render");
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
      fill_synopsis(trg, srcs, nsrc, &p);
      p.fth = eu_mode_feather(p.mode) ? cur().views.fth.p : nullptr;
      p.col = cur().views.col.p; p.row = cur().views.row.p; p.taps = cur().views.taps.dev.p; p.srcs = cur().views.src.p;
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
  HIPCHK(cur().views.readers.host_wait());
  HIPCHK(cur().views.col.reserve(col_floats));
  HIPCHK(cur().views.row.reserve(row_floats));
  HIPCHK(cur().views.scal.reserve(1));
  HIPCHK(hipMemcpyAsync(cur().views.scal.p, sc.data(), sizeof(eu_view_dev), hipMemcpyHostToDevice, cur().stream));
  HIPCHK(hipStreamSynchronize(cur().stream));
  if (eu_launch_view_tables(cur().views.scal.p, 1, trg->projection, W, H, twine, cur().views.col.p, cur().views.row.p, cur().stream))
    return fail(EU_ERR_NO_DEVICE, "view_tables: table kernel launch failed");
  HIPCHK(hipMemcpyAsync(col_dev_built, cur().views.col.p, col_floats * sizeof(float), hipMemcpyDeviceToHost, cur().stream));
  HIPCHK(hipMemcpyAsync(row_dev_built, cur().views.row.p, row_floats * sizeof(float), hipMemcpyDeviceToHost, cur().stream));
  HIPCHK(hipStreamSynchronize(cur().stream));
  return EU_OK;
}

}  // extern "C"
