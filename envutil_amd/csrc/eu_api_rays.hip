// C ABI (include/eu_hip.h), host glue: `act` alone - a resident source evaluated at the caller's rays
// (eu_render_rays.hip).

#include "eu_context.h"

using namespace eu_host;

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
  if (cur().rays.taps.holds(taps.data(), taps.size())) return EU_OK;
  // an earlier call may still read the table, on a caller's stream or on the library's own
  HIPCHK(cur().rays.readers.host_wait());
  HIPCHK(hipStreamSynchronize(cur().stream));
  cur().rays.taps.host.clear();
  HIPCHK(cur().rays.taps.dev.reserve(taps.size()));
  HIPCHK(hipMemcpy(cur().rays.taps.dev.p, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice));
  cur().rays.taps.host.swap(taps);
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
  p.taps = cur().rays.taps.dev.p;
  p.out = out_dev; p.out_stride = (long long)(out_stride_bytes / sizeof(float));
  p.src = src->sd;
  if (eu_launch_render_rays(&p, eu_select_ray_path(p, sw), st)) return fail(EU_ERR_NO_DEVICE, "render_rays: kernel launch failed");
  return EU_OK;
}

// pixels (rays and their output together) of one staged chunk of a call with a host buffer
#define EU_RAYS_CHUNK_BYTES ((size_t)64 << 20)

extern "C" {

int eu_hip_render_rays(const eu_rays *r, eu_source *src, float *out, size_t out_row_stride_bytes, int out_on_device,
                       void *stream)
{
  int rc;
  if ((rc = check_rays(r, src, out, out_row_stride_bytes))) return rc;
  if ((rc = ensure_init())) return rc;
  if (!src->dev) return fail(EU_ERR_HANDLE, "render_rays: the source has no container");
  const eu_switches sw = eu_read_switches();
  if ((rc = upload_ray_taps(r))) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : cur().stream;
  if ((rc = order_sources(&src, 1, st))) return rc;      // behind a reload of the source
  if (r->rays_on_device && out_on_device)
    return note_readers(cur().rays.readers, &src, 1, stream, launch_rays(r, src, sw, r->rays, r->ray_row_stride_bytes, out, out_row_stride_bytes,
                                                   r->width, r->height, st));
  // A host buffer on either side: the grid goes through in chunks of rows - a flat list in chunks of its one
  // row - of bounded size, copy in, launch, copy out, all in order on `st`; the call returns when `out` is complete
  const size_t in_px = (size_t)r->ninputs * sizeof(float), out_px = (size_t)r->nchannels * sizeof(float);
  const bool flat = r->height == 1;
  const size_t px_per_chunk = std::max<size_t>(1, EU_RAYS_CHUNK_BYTES / (in_px + out_px));
  const int cw = flat ? (int)std::min<size_t>((size_t)r->width, px_per_chunk) : r->width;
  const int ch = flat ? 1 : (int)std::min<size_t>((size_t)r->height, std::max<size_t>(1, px_per_chunk / (size_t)r->width));
  if (!r->rays_on_device) HIPCHK(cur().rays.stage.reserve((size_t)cw * ch * r->ninputs));
  if (!out_on_device) HIPCHK(cur().out.stage.reserve((size_t)cw * ch * r->nchannels));
  drain drain_on_exit{ st, st };
  for (int y0 = 0; y0 < r->height; y0 += ch)
    for (int x0 = 0; x0 < r->width; x0 += cw) {
      const int w = std::min(cw, r->width - x0), h = std::min(ch, r->height - y0);
      const char *rin = (const char *)r->rays + (size_t)y0 * r->ray_row_stride_bytes + (size_t)x0 * in_px;
      char *rout = (char *)out + (size_t)y0 * out_row_stride_bytes + (size_t)x0 * out_px;
      const float *rays_dev = (const float *)rin;
      size_t rays_stride = r->ray_row_stride_bytes;
      if (!r->rays_on_device) {
        rays_dev = cur().rays.stage.p; rays_stride = (size_t)w * in_px;
        HIPCHK(hipMemcpy2DAsync(cur().rays.stage.p, rays_stride, rin, r->ray_row_stride_bytes, rays_stride, (size_t)h,
                                hipMemcpyHostToDevice, st));
      }
      float *out_dev = (float *)rout;
      size_t out_stride = out_row_stride_bytes;
      if (!out_on_device) { out_dev = cur().out.stage.p; out_stride = (size_t)w * out_px; }
      if ((rc = launch_rays(r, src, sw, rays_dev, rays_stride, out_dev, out_stride, w, h, st))) return rc;
      if (!out_on_device)
        HIPCHK(hipMemcpy2DAsync(rout, out_row_stride_bytes, cur().out.stage.p, out_stride, out_stride, (size_t)h,
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
                       cur().stream);
  };
  return time_on_stream(once, iters, mean_ms);
}

}  // extern "C"
