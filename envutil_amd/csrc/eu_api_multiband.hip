// C ABI (include/eu_hip.h), host glue: the multi-band scratch and eu_hip_blend_layers, the pyramid on the caller's
// own pictures (eu_multiband.hip). The render path of EU_SYN_MULTIBAND is in eu_api_render.hip (render_on_device).

#include "eu_context.h"

namespace eu_host __attribute__((visibility("hidden"))) {

// `st` is about to rewrite the multi-band buffers: it goes behind every job that used them before - a caller's stream
// by the event it left, the library's own by handle, once per change of sides. A buffer that has to grow is freed:
// the host waits for all of them first. A failed allocation is the library's memory error; nothing is launched.
static int multiband_reserve3(size_t floats, size_t in_floats, size_t frame_floats, hipStream_t st)
{
  auto &m = cur().mband;
  if (st == cur().stream) m.own = true;
  else if (m.own) { HIPCHK(hipStreamSynchronize(cur().stream)); m.own = false; }
  HIPCHK(m.readers.order_after(st));
  if (m.buf.cap < floats || m.in.cap < in_floats || m.frame.cap < frame_floats) {
    HIPCHK(m.readers.host_wait());
    HIPCHK(hipStreamSynchronize(cur().stream));
    HIPCHK(hipStreamSynchronize(st));
  }
  struct { eu_dev_buf<float> *b; size_t n; const char *what; } want[3] = {
    { &m.buf, floats, "scratch" }, { &m.in, in_floats, "staged pictures" }, { &m.frame, frame_floats, "staged frame" } };
  for (auto &w : want)
    if (w.b->reserve(w.n) != hipSuccess) {
      (void)hipGetLastError();
      return fail(EU_ERR_MEMORY, std::string("multiband: cannot allocate ") + std::to_string(w.n * sizeof(float)) +
                                 " bytes of device memory (" + w.what + ")");
    }
  return EU_OK;
}

int multiband_reserve(size_t floats, hipStream_t st) { return multiband_reserve3(floats, 0, 0, st); }

}  // namespace eu_host

using namespace eu_host;

extern "C" {

size_t eu_hip_multiband_scratch_bytes(const eu_target *trg, int nsrc)
{
  if (!trg || nsrc < 2 || trg->width < 1 || trg->height < 1 || trg->nchannels < 1 || trg->nchannels > 4 || trg->bands < 0) return 0;
  eu_mb_geom g;
  multiband_geom(trg, &g);
  const bool alpha = trg->nchannels == 2 || trg->nchannels == 4;
  return eu_mb_scratch_floats(g, alpha ? trg->nchannels - 1 : trg->nchannels, nsrc) * sizeof(float);
}

int eu_hip_multiband_levels(int width, int height, int bands, int wrap)
{
  if (width < 1 || height < 1 || bands < 0) return fail(EU_ERR_ARGUMENT, "multiband_levels: sizes of 1 or more, bands 0 or more");
  eu_mb_geom g;
  eu_mb_levels(width, height, bands, wrap != 0, &g);
  return g.L;
}

int eu_hip_multiband_scratch_release(void)
{
  for (int k = 0; k < nslots_; k++) {
    context &c = ctx_[k];
    if (c.device < 0) continue;
    if (!c.mband.buf.p && !c.mband.in.p && !c.mband.frame.p) continue;
    const int back = cur_slot_;
    int rc;
    if ((rc = set_slot(k))) return rc;
    hipError_t e = c.mband.readers.host_wait();
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    auto drop = [&](auto &b) { if (b.p) { const hipError_t f = hipFree(b.p); if (e == hipSuccess) e = f; } b.p = nullptr; b.cap = 0; };
    drop(c.mband.buf); drop(c.mband.in); drop(c.mband.frame);
    c.mband.own = false;
    if ((rc = set_slot(back))) return rc;
    if (e != hipSuccess) return fail(EU_ERR_NO_DEVICE, std::string("multiband_scratch_release: ") + hipGetErrorString(e));
  }
  return EU_OK;
}

int eu_hip_blend_layers(const float *colour, size_t c_row, size_t c_layer, const float *weight, size_t w_row, size_t w_layer,
                        int in_on_device, int nlayers, int width, int height, int nchannels, int bands, int wrap,
                        float *out, size_t out_row_stride_bytes, int out_on_device, void *stream)
{
  int rc;
  if (!colour || !weight || !out) return fail(EU_ERR_ARGUMENT, "blend_layers: null argument");
  if (nlayers < 1) return fail(EU_ERR_ARGUMENT, "blend_layers: at least one layer");
  if (nchannels < 1 || nchannels > EU_MB_MAXCOL) return fail(EU_ERR_ARGUMENT, "blend_layers: channels must be 1..4");
  if (width < 1 || height < 1) return fail(EU_ERR_ARGUMENT, "blend_layers: empty pictures");
  if ((size_t)width * nchannels > (size_t(1) << 28) || (size_t)height > (size_t(1) << 18))
    return fail(EU_ERR_ARGUMENT, "blend_layers: rows of up to 2^28 floats, up to 2^18 rows");
  if (bands < 0) return fail(EU_ERR_ARGUMENT, "blend_layers: bands must be 0 (the default) or the number of pyramid levels");
  const size_t crow = (size_t)width * nchannels * sizeof(float), wrow = (size_t)width * sizeof(float);
  if (c_row < crow || w_row < wrow || out_row_stride_bytes < crow) return fail(EU_ERR_ARGUMENT, "blend_layers: row stride smaller than a row");
  if (c_layer < c_row * (size_t)height || w_layer < w_row * (size_t)height)
    return fail(EU_ERR_ARGUMENT, "blend_layers: layer stride smaller than a picture");
  if ((c_row | c_layer | w_row | w_layer | out_row_stride_bytes) % sizeof(float) ||
      (reinterpret_cast<uintptr_t>(colour) | reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(out)) % sizeof(float))
    return fail(EU_ERR_ARGUMENT, "blend_layers: pointers and strides are multiples of 4 bytes");
  if ((rc = ensure_init())) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : cur().stream;
  eu_mb_geom g;
  eu_mb_levels(width, height, bands, wrap != 0, &g);
  const size_t S0 = g.off[1], N = (size_t)nlayers;
  const size_t in_floats = in_on_device ? 0 : N * S0 * (nchannels + 1), frame_floats = out_on_device ? 0 : S0 * nchannels;
  if ((rc = multiband_reserve3(eu_mb_scratch_floats(g, nchannels, nlayers), in_floats, frame_floats, st))) return rc;
  auto &m = cur().mband;
  drain drain_on_exit{ st, st, !in_on_device || !out_on_device };   // a host buffer on either side: complete on return
  eu_mb_in in { colour, weight, (long long)(c_layer / sizeof(float)), (long long)(c_row / sizeof(float)),
                (long long)(w_layer / sizeof(float)), (long long)(w_row / sizeof(float)) };
  if (!in_on_device) {
    float *dc = m.in.p, *dw = m.in.p + N * S0 * nchannels;
    for (size_t f = 0; f < N; f++) {
      HIPCHK(hipMemcpy2DAsync(dc + f * S0 * nchannels, crow, (const char *)colour + f * c_layer, c_row, crow, (size_t)height, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpy2DAsync(dw + f * S0, wrow, (const char *)weight + f * w_layer, w_row, wrow, (size_t)height, hipMemcpyHostToDevice, st));
    }
    in = eu_mb_in { dc, dw, (long long)(S0 * nchannels), (long long)width * nchannels, (long long)S0, (long long)width };
  }
  if (eu_launch_mb_prep(m.buf.p, &g, nchannels, nlayers, &in, st)) return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
  const eu_mb_out mo { out_on_device ? out : m.frame.p, (long long)((out_on_device ? out_row_stride_bytes : crow) / sizeof(float)), nchannels, 0, 0 };
  if (eu_launch_mb_blend(m.buf.p, &g, nchannels, nlayers, &mo, st, nullptr)) return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
  if (!out_on_device)
    HIPCHK(hipMemcpy2DAsync(out, out_row_stride_bytes, m.frame.p, crow, crow, (size_t)height, hipMemcpyDeviceToHost, st));
  return note_caller(m.readers, stream, EU_OK);
}

// DIAGNOSTIC (not declared in eu_hip.h; tools/multiband_time.py): kernel time in ms and nominal bytes per stage
// (EU_MB_T_*: stage A, normalise, reduce, band, collapse) of ONE multiband job into device memory, means over
// `iters` runs after one untimed run; events around every launch, the stream drained between runs
int eu_hip_multiband_stage_times(const eu_target *trg, eu_source *const *srcs, int nsrc, float *out_dev, size_t out_row_stride_bytes,
                                 int iters, double *ms, double *bytes)
{
  int rc;
  if (!trg || !srcs || nsrc < 2 || !out_dev || iters < 1 || !ms || !bytes) return fail(EU_ERR_ARGUMENT, "multiband_stage_times: arguments");
  if (trg->synopsis != EU_SYN_MULTIBAND) return fail(EU_ERR_ARGUMENT, "multiband_stage_times: a multiband job");
  if ((rc = check_target(trg)) || (rc = check_multiband(trg, srcs, nsrc))) return rc;
  if ((rc = ensure_init())) return rc;
  const eu_switches sw = eu_read_switches();
  if ((rc = render_on_device(trg, srcs, nsrc, out_dev, out_row_stride_bytes, sw, cur().stream))) return rc;
  HIPCHK(hipStreamSynchronize(cur().stream));
  eu_mb_times t {};
  for (int i = 0; i < iters; i++)
    if ((rc = render_on_device(trg, srcs, nsrc, out_dev, out_row_stride_bytes, sw, cur().stream, nullptr, false, nullptr, &t))) return rc;
  for (int k = 0; k < EU_MB_T_N; k++) { ms[k] = t.ms[k] / iters; bytes[k] = t.bytes[k] / iters; }
  return EU_OK;
}

}  // extern "C"
