// C ABI (include/eu_hip.h), host glue: one process, several devices. Reaches the render family through
// render_on_device (eu_context.h) and the public entry points only.

#include "eu_context.h"

using namespace eu_host;

extern "C" {

// (inside extern "C", where these two have always stood: the compiler gives them their plain names, which the
// library's symbol table has held since)
namespace {

// the source's copy on slot k (made on first use: one peer copy of the braced container)
int replica_of(eu_source *src, int k, eu_source **out)
{
  if (k == src->slot) { *out = src; return EU_OK; }
  if (!src->replica[k]) {
    eu_source *r = new (std::nothrow) eu_source(*src);
    if (!r) return fail(EU_ERR_NO_DEVICE, "out of host memory");
    for (int j = 0; j < EU_MAX_SLOTS; j++) r->replica[j] = nullptr;
    r->is_replica = true; r->slot = k; r->dev = nullptr; r->edge = nullptr;
    r->readers = eu_readers(); r->written = eu_readers(); r->own_written = false;      // the original's events stay its own
    int rc = set_slot(k);
    if (rc) { delete r; return rc; }
    hipError_t e = hipMalloc((void **)&r->dev, src->nfloats * sizeof(float));
    if (e == hipSuccess) {
      if (ctx_[k].device == ctx_[src->slot].device)
        e = hipMemcpyAsync(r->dev, src->dev, src->nfloats * sizeof(float), hipMemcpyDeviceToDevice, cur().stream);
      else
        e = hipMemcpyPeerAsync(r->dev, ctx_[k].device, src->dev, ctx_[src->slot].device, src->nfloats * sizeof(float), cur().stream);
    }
    if (e == hipSuccess && src->edge) {
      // the distance plane of a source loaded with EU_LOAD_EDGES travels with the container
      const size_t nb = (size_t)src->fct.window_width * (size_t)src->fct.window_height * sizeof(float);
      e = hipMalloc((void **)&r->edge, nb);
      if (e != hipSuccess) r->edge = nullptr;
      else if (ctx_[k].device == ctx_[src->slot].device)
        e = hipMemcpyAsync(r->edge, src->edge, nb, hipMemcpyDeviceToDevice, cur().stream);
      else
        e = hipMemcpyPeerAsync(r->edge, ctx_[k].device, src->edge, ctx_[src->slot].device, nb, cur().stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(cur().stream);
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
  if (trg && (rc = check_synopsis(trg))) return rc;      // before a device is looked for
  if (trg && trg->synopsis == EU_SYN_MULTIBAND && nsrc > 1 && nslots_ > 1)
    return fail(EU_ERR_ARGUMENT, "render_devices: no multiband synopsis on more than one device - the pyramid needs the whole frame on one");
  if ((rc = ensure_init())) return rc;
  if (nslots_ <= 1) return eu_hip_render(trg, srcs, nsrc, out, out_row_stride_bytes, out_on_device, nullptr);
  if (!trg || !srcs || nsrc < 1 || !out) return fail(EU_ERR_ARGUMENT, "no source / no output");
  if ((rc = check_target(trg))) return rc;
  if (trg->band_count > 1 || trg->row_begin != 0 || trg->row_end != frame_h(trg))
    return fail(EU_ERR_ARGUMENT, "eu_hip_render_devices renders whole frames (it does the tiling itself)");
  if (nsrc > 64) return fail(EU_ERR_UNSUPPORTED, "more than 64 facets over several devices");
  const size_t min_stride = frame_row_bytes(trg);
  if (out_row_stride_bytes < min_stride || out_row_stride_bytes % sizeof(float))
    return fail(EU_ERR_ARGUMENT, "row stride smaller than a row / not a multiple of 4 bytes");
  int begin[EU_MAX_SLOTS], end[EU_MAX_SLOTS];
  cost_strips(trg, srcs, nsrc, nslots_, begin, end);
  const eu_switches sw = eu_read_switches();
  // the slots read the originals (slot 0 renders them, the others copy them on first use): a reload of one of them,
  // on a caller's stream or on the library's own, has to be through. The call leaves no reader behind: the guard waits
  for (int f = 0; f < nsrc; f++) {
    if (!srcs[f]) return fail(EU_ERR_HANDLE, "null source");
    HIPCHK(srcs[f]->written.host_wait());
    if (srcs[f]->own_written) { HIPCHK(hipStreamSynchronize(ctx_[srcs[f]->slot].stream)); srcs[f]->own_written = false; }
  }
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
      HIPCHK(cur().out.strip.reserve(rows * (min_stride / sizeof(float))));
      dst = cur().out.strip.p;
    }
    if ((rc = render_on_device(&t, reps, nsrc, dst, min_stride, sw, cur().stream))) return rc;
    if (!direct) {
      char *o = (char *)out + (size_t)begin[k] * out_row_stride_bytes;
      if (!out_on_device)
        HIPCHK(hipMemcpy2DAsync(o, out_row_stride_bytes, dst, min_stride, min_stride, rows, hipMemcpyDeviceToHost, cur().stream));
      else if (ctx_[k].device == ctx_[0].device)
        HIPCHK(hipMemcpy2DAsync(o, out_row_stride_bytes, dst, min_stride, min_stride, rows, hipMemcpyDeviceToDevice, cur().stream));
      else if (out_row_stride_bytes == min_stride)
        HIPCHK(hipMemcpyPeerAsync(o, ctx_[0].device, dst, ctx_[k].device, rows * min_stride, cur().stream));
      else
        for (size_t r = 0; r < rows; r++)
          HIPCHK(hipMemcpyPeerAsync(o + r * out_row_stride_bytes, ctx_[0].device, (char *)dst + r * min_stride, ctx_[k].device, min_stride, cur().stream));
    }
  }
  return EU_OK;      // the guard waits for every slot
}

}  // extern "C"
