// C ABI (include/eu_hip.h), host glue: many pictures of one geometry in one call (eu_render_layers.hip).

#include "eu_context.h"
#include "eu_setup_math.h"

using namespace eu_host;

// bytes of a host output that are staged on the device at a time (at least one layer)
#define EU_LAYERS_STAGE_BYTES ((size_t)64 << 20)

// everything that can be wrong with the target, found without a device: the view calls' rules
static int check_layers_target(const eu_target *t)
{
  { int rc0 = check_target(t); if (rc0) return rc0; }
  if (t->stage != 0) return fail(EU_ERR_ARGUMENT, "render_layers: stage outputs belong to eu_hip_render");
  if (t->crop_w != 0) return fail(EU_ERR_ARGUMENT, "render_layers: whole frames only, no crop window");
  if (t->band_count > 1) return fail(EU_ERR_ARGUMENT, "render_layers: whole frames only, no row bands");
  if (t->single) return fail(EU_ERR_ARGUMENT, "render_layers: a --single target belongs to eu_hip_render");
  if (t->out_format != EU_OUT_FLOAT) return fail(EU_ERR_ARGUMENT, "render_layers: float output only");
  if (t->row_begin != 0 || t->row_end != t->height)
    return fail(EU_ERR_ARGUMENT, "render_layers: whole frames only (row_begin 0, row_end height)");
  return EU_OK;
}

// The agreement rule: the kernels compute coordinates, gates and weights from layer 0's parameter block, so layer
// k's must equal it byte for byte apart from the container's address and brighten; the stepper tables come from
// layer 0's orientation, so that is shared too.
static int check_layers_agree(eu_source *const *layers, int nlayers)
{
  const eu_source *a = layers[0];
  eu_src_dev ref = a->sd;
  ref.base = nullptr; ref.brighten = 0.0f;
  for (int k = 1; k < nlayers; k++) {
    const eu_source *b = layers[k];
    const char *what = nullptr;
    eu_src_dev d = b->sd;
    d.base = nullptr; d.brighten = 0.0f;
    if (b->nch != a->nch) what = "channel count";
    else if (b->degree != a->degree) what = "spline degree";
    else if (b->fct.projection != a->fct.projection) what = "projection";
    else if (b->fct.width != a->fct.width || b->fct.height != a->fct.height) what = "size";
    else if (b->fct.hfov != a->fct.hfov) what = "field of view";
    else if (b->fct.yaw != a->fct.yaw || b->fct.pitch != a->fct.pitch || b->fct.roll != a->fct.roll) what = "orientation";
    else if (memcmp(&d, &ref, sizeof d)) what = "source parameters (window, lens, boundary conditions or container layout)";
    if (what)
      return fail(EU_ERR_ARGUMENT, "render_layers: layer " + std::to_string(k) + " differs from layer 0 in its " + what +
                                   ": layers share everything but their pixels and brighten");
  }
  return EU_OK;
}

// the tap table on the device (biased_taps); where the buffer is rewritten that happens on `st`, from *keep: the
// caller synchronises
static int upload_layer_taps(const eu_target *t, hipStream_t st, std::vector<float> *keep)
{
  if (t->ntaps <= 0) return EU_OK;
  *keep = biased_taps(t->taps, t->ntaps);
  auto &taps = cur().layers.taps;
  if (taps.holds(keep->data(), keep->size())) return EU_OK;
  taps.host.clear();
  HIPCHK(taps.dev.reserve(keep->size()));
  HIPCHK(hipMemcpyAsync(taps.dev.p, keep->data(), keep->size() * sizeof(float), hipMemcpyHostToDevice, st));
  taps.host = *keep;
  return EU_OK;
}

extern "C" {

int eu_hip_render_layers(const eu_target *trg, eu_source *const *layers, int nlayers, float *out,
                         size_t out_row_stride_bytes, size_t out_layer_stride_bytes, int out_on_device, void *stream)
{
  int rc;
  if (!trg || !layers || !out) return fail(EU_ERR_ARGUMENT, "render_layers: null argument");
  if (nlayers < 0) return fail(EU_ERR_ARGUMENT, "render_layers: negative number of layers");
  for (int k = 0; k < nlayers; k++)
    if (!layers[k]) return fail(EU_ERR_HANDLE, "render_layers: null source (layer " + std::to_string(k) + ")");
  if ((rc = check_layers_target(trg))) return rc;
  for (int k = 0; k < nlayers; k++)
    if (layers[k]->fct.mask_paint)
      return fail(EU_ERR_ARGUMENT, "render_layers: layer " + std::to_string(k) + " is a --mask_for source: its paint replaces the picture, render it with eu_hip_render");
  const size_t row_bytes = (size_t)trg->width * trg->nchannels * sizeof(float);
  if (out_row_stride_bytes % sizeof(float) || out_layer_stride_bytes % sizeof(float))
    return fail(EU_ERR_ARGUMENT, "render_layers: strides must be multiples of 4 bytes");
  if (out_row_stride_bytes < row_bytes) return fail(EU_ERR_ARGUMENT, "render_layers: row stride smaller than a row");
  if (out_layer_stride_bytes / (size_t)trg->height < out_row_stride_bytes)
    return fail(EU_ERR_ARGUMENT, "render_layers: layer stride smaller than `height` rows");
  if (nlayers > 0 && (rc = check_layers_agree(layers, nlayers))) return rc;
  // what this path does not render, the view calls' choices: the generic stepper, a projection without tables
  for (int k = 0; k < nlayers; k++)
    if (eu::has_translation(layers[k]->fct))
      return fail(EU_ERR_UNSUPPORTED, "render_layers: a facet with PTO translation (layer " + std::to_string(k) + ") is stepped by the generic stepper: use eu_hip_render");
  if (eu::generic_target(*trg))
    return fail(EU_ERR_UNSUPPORTED, "render_layers: this target is stepped by the generic stepper: use eu_hip_render");
  const bool twine = trg->ntaps > 0;
  int form = 0, norm_mode = 0;
  if (!eu::stepper_form(trg->projection, twine, form, norm_mode))
    return fail(EU_ERR_UNSUPPORTED, "no stepper for this target projection");
  if (nlayers == 0) return EU_OK;
  if ((rc = ensure_init())) return rc;
  for (int k = 0; k < nlayers; k++)
    if (!layers[k]->dev) return fail(EU_ERR_HANDLE, "render_layers: a source has no container (layer " + std::to_string(k) + ")");
  const eu_switches sw = eu_read_switches();
  hipStream_t st = stream ? (hipStream_t)stream : cur().stream;

  // one camera: the stepper tables once, on the host, as eu_hip_render builds them
  const eu_source *s0 = layers[0];
  const eu::mat3 basis = eu::rotate(eu::make_r3(trg->roll, trg->pitch, trg->yaw, false),
                                    eu::make_r3(s0->fct.roll, s0->fct.pitch, s0->fct.yaw, true));
  eu::stepper_tables tb;
  if (!eu::build_stepper_tables(*trg, basis, twine, twine, tb))
    return fail(EU_ERR_UNSUPPORTED, "no stepper for this target projection");

  const int H = trg->height;
  const size_t frame_bytes = (size_t)H * row_bytes;
  int per_launch = eu_layers_per_launch(nlayers, sw.layers_max);
  if (!out_on_device)
    per_launch = (int)std::min<size_t>((size_t)per_launch, std::max<size_t>(1, EU_LAYERS_STAGE_BYTES / frame_bytes));

  std::vector<eu_layer_dev> tab((size_t)nlayers);
  for (int k = 0; k < nlayers; k++) {
    tab[k].base = layers[k]->sd.base;
    tab[k].brighten = layers[k]->sd.brighten;
    tab[k].pad = 0;
  }
  std::vector<float> taps;
  drain drain_on_exit{ st, st };          // the host vectors above are among what the call lets go of
  // the buffers are rewritten on `st`, and reserve() may free them: the layered calls before this one have to be
  // through, on callers' streams (the event) and on the library's own
  auto &lb = cur().layers;
  HIPCHK(lb.readers.host_wait());
  if (stream) HIPCHK(hipStreamSynchronize(cur().stream));
  HIPCHK(lb.col.reserve(tb.col.size()));
  HIPCHK(lb.row.reserve(tb.row.size()));
  HIPCHK(lb.tab.reserve(tab.size()));
  if (!out_on_device) HIPCHK(lb.stage.reserve((size_t)per_launch * frame_bytes / sizeof(float)));
  if ((rc = order_sources(layers, nlayers, st))) return rc;      // behind a reload of a layer
  // the one host synchronisation of the call: tables, layer table and a new tap table, in flight from host vectors
  HIPCHK(hipMemcpyAsync(lb.col.p, tb.col.data(), tb.col.size() * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(lb.row.p, tb.row.data(), tb.row.size() * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(lb.tab.p, tab.data(), tab.size() * sizeof(eu_layer_dev), hipMemcpyHostToDevice, st));
  if ((rc = upload_layer_taps(trg, st, &taps))) return rc;
  HIPCHK(hipStreamSynchronize(st));

  eu_render_params p;
  memset(&p, 0, sizeof p);
  p.width = trg->width; p.height = H; p.row_begin = 0; p.row_end = H;
  p.form = tb.form; p.norm_mode = tb.norm_mode;
  p.twine = twine; p.ntaps = trg->ntaps; p.nch = s0->nch; p.nch_out = trg->nchannels;
  p.col = lb.col.p; p.row = lb.row.p; p.taps = lb.taps.dev.p;
  p.src = s0->sd;
  p.direct = 1;
  p.out_stride = (long long)((out_on_device ? out_row_stride_bytes : row_bytes) / sizeof(float));
  const int path = eu_select_layer_path(p, sw);
  eu_layers_params lp;
  lp.out_layer = (long long)((out_on_device ? out_layer_stride_bytes : frame_bytes) / sizeof(float));
  const int launches = eu_layers_launches(nlayers, per_launch);
  for (int c = 0; c < launches; c++) {
    const int c0 = c * per_launch, nl = std::min(per_launch, nlayers - c0);
    char *dst = (char *)out + (size_t)c0 * out_layer_stride_bytes;
    p.out = out_on_device ? (float *)dst : lb.stage.p;
    lp.layers = lb.tab.p + c0; lp.nlayers = nl;
    if (eu_launch_render_layers(&p, &lp, path, &sw, st))
      return fail(EU_ERR_NO_DEVICE, "render_layers: kernel launch failed");
    if (!out_on_device)
      for (int k = 0; k < nl; k++)
        HIPCHK(hipMemcpy2DAsync(dst + (size_t)k * out_layer_stride_bytes, out_row_stride_bytes,
                                (const char *)lb.stage.p + (size_t)k * frame_bytes, row_bytes, row_bytes, (size_t)H,
                                hipMemcpyDeviceToHost, st));
  }
  if (!out_on_device) HIPCHK(hipStreamSynchronize(st));
  drain_on_exit.on = false;          // a device output stays queued: `st` goes on reading the call's buffers
  return note_readers(lb.readers, layers, nlayers, out_on_device ? stream : nullptr, EU_OK);
}

}  // extern "C"
