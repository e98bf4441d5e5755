// What the C ABI's host glue shares (eu_api.hip and eu_api_*.hip, one translation unit per call family; nothing else
// includes this): the source handle, the per-device context with its buffers grouped by the event that guards them,
// the error string, and the few helpers more than one family uses. Host only. Everything but eu_source lives in
// eu_host, which has hidden visibility: none of it enters the library's dynamic symbol table.
#ifndef EU_CONTEXT_H
#define EU_CONTEXT_H
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>
#include <new>
#include "eu_device.h"
#include "eu_launch.h"
#include "eu_multiband.h"

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
  // what the container was built with, for eu_hip_source_reload (a cubemap's metrics follow from them)
  int support_min = 0, tile_size = 0;
  // the container can be refilled in place (eu_hip_source_reload), so it is guarded like the library's own buffers:
  // `readers` is noted behind every job that leaves work reading it on a caller's stream, `written` behind a reload
  // on a caller's stream; own_written: a reload is queued on the library's own stream, which leaves no event, and no
  // caller's stream has waited for it since. Copies on other slots have neither: they are dropped by a reload.
  eu_readers readers, written;
  bool own_written = false;
  // EU_LOAD_EDGES: the distance plane D of the window (eu_edges.hip), window_width x window_height floats, dense; it is
  // written wherever the container is - by the load and by every reload, on the same stream -, so the container's
  // guards are its own. nullptr: the source keeps none.
  float *edge = nullptr;
};

namespace eu_host __attribute__((visibility("hidden"))) {

extern thread_local std::string g_err;
inline int fail(int code, const std::string &msg) { g_err = msg; return code; }

#define HIPCHK(call)                                                          \
  do {                                                                        \
    hipError_t e_ = (call);                                                   \
    if (e_ != hipSuccess)                                                     \
      return fail(EU_ERR_NO_DEVICE, std::string(#call ": ") + hipGetErrorString(e_)); \
  } while (0)

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

// The device tables of a cached plan and what they were made for: they stay valid while (target geometry,
// orientation, taps) repeat - streaming / tethered jobs re-render the same target many times
// (envutil_main.cc:1948-1982). A single-source job and a multi-facet job each keep their own.
struct plan_cache {
  eu_dev_buf<float> col, row, taps;
  std::vector<unsigned char> key;                 // plan_key_of
  int form = 0, norm = 0;
};

// A device table and the host copy of what it holds: equal contents are not sent again.
struct held_table {
  eu_dev_buf<float> dev;
  std::vector<float> host;
  // the device table already holds exactly the na floats at a followed by the nb floats at b
  bool holds(const float *a, size_t na, const float *b = nullptr, size_t nb = 0) const
  {
    return dev.p && host.size() == na + nb && !memcmp(host.data(), a, na * sizeof(float)) &&
           (!nb || !memcmp(host.data() + na, b, nb * sizeof(float)));
  }
};

// The buffers that outlive a call lie next to the eu_readers that says who may still read them on a caller's
// stream ("Buffers that outlive a call").
struct context {
  int device = -1;
  hipStream_t stream = nullptr;
  float *lut = nullptr;        // to_screen_t's sRGB LUT, 257 floats
  unsigned long long launches = 0;                // render kernel launches so far
  float *inv_coef = nullptr;                      // --single: the inverse lens model's coefficients (eu_inv_planar)
  // ONE guard for several families, all of them read by the render kernels of eu_hip_render[_samples]: both cached
  // plans (plan, mplan), inv_coef and the float frame out.scr
  eu_readers tables;
  // the single-source plan, with host copies of its stepper tables and, from them, the layout the packed
  // kernel should use per segment of EU_SEG_ROWS frame rows (launch-level hybrid)
  struct : plan_cache {
    std::vector<float> h_col, h_row;
    std::vector<unsigned char> seg_flags;
    bool seg_valid = false;
    eu_src_dev seg_sd;
    unsigned long long plan_gen = 0;              // bumped whenever the stepper tables change
    int tab_finite = 0;                           // every entry of the plan's stepper tables is finite
  } plan;
  // the multi-facet plan, with what every job refreshes beside it
  struct : plan_cache {
    eu_dev_buf<eu_src_dev> src;                   // the facets' evaluator parameters
    eu_dev_buf<float> rej;                        // early-miss tables
    eu_dev_buf<eu_generic> gen;                   // the translated facets' transformations
    eu_dev_buf<eu_feather_dev> fth;               // the feathered synopsis' edge-weight table
  } mplan;
  struct {
    eu_dev_buf<int> wl;                           // eu_render4.hip work list: two sets of counters, tile ids (eu_worklist.h)
    int parity = 0;                               // the set the NEXT launch pair uses; moves when both launches went out
    int last_set = -1;                            // the set the last pair used, for eu_hip_listed_tiles(); -1: no pair yet
    eu_readers wl_pair;                           // wl and the staged kernels' cached plans: behind EVERY launch pair
  } staged;
  // eu_hip_render_rays keeps its own tap table (the plan's is part of the cached plan of eu_hip_render) and its
  // own staging of host rays
  struct {
    held_table taps;
    eu_dev_buf<float> stage;
    eu_readers readers;                           // taps
  } rays;
  // eu_hip_render_views[_multi]: the views' scalar blocks, the stepper tables the table kernel makes from them (one
  // chunk of views), the tap table, the facets' evaluator parameters of a multi-facet job and the staging of a host
  // output - all its own, like eu_hip_render_rays' buffers
  struct {
    eu_dev_buf<eu_view_dev> scal;
    eu_dev_buf<float> col, row, stage;
    held_table taps;
    eu_dev_buf<eu_src_dev> src;
    eu_dev_buf<eu_feather_dev> fth;               // the feathered synopsis' edge-weight table
    eu_readers readers;                           // scal, col, row, taps, src, fth
  } views;
  // eu_hip_render_layers: the one camera's stepper tables (built on the host per call), the tap table, the layer
  // table and the staging of a host output - all its own, like the view calls' buffers
  struct {
    eu_dev_buf<float> col, row, stage;
    held_table taps;
    eu_dev_buf<eu_layer_dev> tab;
    eu_readers readers;                           // col, row, taps, tab
  } layers;
  // eu_hip_encode_samples / eu_hip_render_samples: the step tables on the device (colour, then alpha) with the host
  // copy they were uploaded from - it stays, so that an upload queued on a stream never reads a caller's memory after
  // the call - and the staging of a host frame and of a host output
  struct {
    held_table steps;
    eu_dev_buf<float> frame;
    eu_dev_buf<uint32_t> out;
    eu_readers readers;                           // steps
    bool own = false;                             // the library's own stream has used out.scr or steps since a caller's
                                                  // stream last waited for it (it leaves no event: order_encoders)
  } enc;
  struct {
    eu_dev_buf<int32_t> plan;                     // row plan of the last device alpha edit
    eu_readers readers;
  } alpha;
  // eu_hip_source_reload: what a load frees by scope stays here and serves the next reload - the feed's tables (with
  // their host copy: equal tables are not sent again), the bytes of a host image, the dense buffer in front of an
  // edit and the six faces of a cubemap
  struct {
    held_table tables;
    eu_dev_buf<char> block;
    eu_dev_buf<float> staged, faces;
    eu_dev_buf<int32_t> edges;                    // the scratch plane of a distance transform (eu_edges.h)
    eu_readers readers;                           // all of them: behind every reload on a caller's stream
    eu_readers own;                               // a mark on the library's own stream, for a caller's stream to wait for
  } reload;
  // EU_SYN_MULTIBAND / eu_hip_blend_layers: the layer planes and pyramids of one job (eu_multiband.h has the layout),
  // kept for the next one; `in` and `frame` stage host pictures and a host frame of eu_hip_blend_layers
  struct {
    eu_dev_buf<float> buf, in, frame;
    eu_readers readers;                           // all of them: behind every job on a caller's stream
    bool own = false;                             // the library's own stream has used them since a caller's stream last waited
  } mband;
  // the way out of a frame: nothing here is read after the call that used it but scr, which `tables` guards
  struct {
    eu_dev_buf<float> stage;                      // host-output staging
    hipStream_t copy = nullptr;                   // D2H of a host-output frame, chunk by chunk
    hipEvent_t chunk_done[4] = { nullptr, nullptr, nullptr, nullptr };
    eu_dev_buf<float> scr;                        // float frame of a tethered job or of one encoded to samples
    eu_dev_buf<float> strip;                      // eu_hip_render_devices: this slot's rows before they are gathered
  } out;
};
// One context per device SLOT. A process that never calls eu_hip_init_devices has one slot (one process per
// GPU, the set-up bench.py's multi-rank runs use); eu_hip_init_devices makes a slot per listed device, and every
// entry point works on the current one.
extern context ctx_[EU_MAX_SLOTS];
extern int nslots_, cur_slot_;
inline context &cur() { return ctx_[cur_slot_]; }

int set_slot(int k);
int init_device(int dev);
int ensure_init();

// the end of a call with result `rc` that may have left work on a caller's stream (null: the library's own, no event)
inline int note_caller(eu_readers &r, void *stream, int rc)
{
  const hipError_t e = stream ? r.note((hipStream_t)stream) : hipSuccess;
  return rc || e == hipSuccess ? rc : fail(EU_ERR_NO_DEVICE, std::string("stream order: ") + hipGetErrorString(e));
}

// Sources as a job's input. Before the job's first launch: `st` goes behind every reload of one of them - on a
// caller's stream by the event it left, on the library's own stream by handle.
inline int order_sources(eu_source *const *srcs, int nsrc, hipStream_t st)
{
  for (int f = 0; f < nsrc; f++) {
    eu_source *s = srcs[f];
    if (!s) continue;
    if (s->own_written && st != cur().stream) { HIPCHK(hipStreamSynchronize(cur().stream)); s->own_written = false; }
    HIPCHK(s->written.order_after(st));
  }
  return EU_OK;
}
// The end of such a job with result `rc`, where note_caller stands for the library's buffers `r`: the sources too
// note that a caller's stream may still read them.
inline int note_readers(eu_readers &r, eu_source *const *srcs, int nsrc, void *stream, int rc)
{
  rc = note_caller(r, stream, rc);
  for (int f = 0; stream && f < nsrc; f++)
    if (srcs[f]) rc = note_caller(srcs[f]->readers, stream, rc);
  return rc;
}

// whatever happens after this, nothing of the call may still use the caller's host memory or a staging buffer when it returns
struct drain {
  hipStream_t a, b; bool on = true;
  ~drain() { if (on) { (void)hipStreamSynchronize(a); if (b != a) (void)hipStreamSynchronize(b); } }
};

// the processed frame: the whole target or its crop window (store_cropped)
inline int frame_w(const eu_target *t) { return t->crop_w > 0 ? t->crop_w : t->width; }
inline int frame_h(const eu_target *t) { return t->crop_w > 0 ? t->crop_h : t->height; }

// bytes of a row of a float or packed frame; words per pixel: a packed sRGBA8 word, 3 floats of a stage output, or
// the channels
inline size_t frame_row_bytes(const eu_target *t)
{
  const int och = t->out_format == EU_OUT_SRGBA8 ? 1 : t->stage ? 3 : t->nchannels;
  return (size_t)frame_w(t) * och * sizeof(float);
}

int local_rows(int height, int band_rows, int band_count, int band_index);
int check_target(const eu_target *t);
int check_synopsis(const eu_target *t);
int check_multiband(const eu_target *t, eu_source *const *srcs, int nsrc);
void multiband_geom(const eu_target *t, eu_mb_geom *g);
// `st` is about to rewrite the multi-band scratch: behind the jobs that used it before; then reserve() it
int multiband_reserve(size_t floats, hipStream_t st);
std::vector<float> biased_taps(const float *taps, int ntaps);
void fill_synopsis(const eu_target *t, eu_source *const *srcs, int nsrc, eu_multi_params *p);

// the source is a full sphere: the load gives it the two-axis periodic prefilter and pole rows (eu_api_source.hip),
// and the feathered synopsis gives it no border on axis 1
inline bool full_sphere(const eu_facet *f)
{
  return f->projection == EU_SPHERICAL && std::fabs(f->hfov - 2.0 * M_PI) < .000001 && f->width == 2 * f->height;
}
// the per-job table of the feathered synopsis (eu_feather_dev, eu_launch.h), one entry per facet
std::vector<eu_feather_dev> feather_table(const eu_target *t, eu_source *const *srcs, int nsrc);

// the handle and its container (not the copies on other device slots: eu_hip_source_release)
inline void destroy_source(eu_source *s)
{
  if (!s) return;
  if (s->dev) (void)hipFree(s->dev);
  if (s->edge) (void)hipFree(s->edge);
  if (s->readers.ev) (void)hipEventDestroy(s->readers.ev);
  if (s->written.ev) (void)hipEventDestroy(s->written.ev);
  delete s;
}

// The planes one launch of the Y'CbCr encode writes (eu_ycbcr_out.hip): `o` says layout, depth and coefficients, the
// pointers and pitches are those of the launch - the caller's planes on the device, or a staging buffer's.
struct ycbcr_dst {
  const eu_ycbcr_out *o;
  void *y, *cb, *cr;
  size_t y_pitch, c_pitch;
};

// eu_api_render.hip. One job, everything on the device: what eu_hip_render_devices takes from the render family
int render_on_device(const eu_target *trg, eu_source *const *srcs, int nsrc, float *out_dev, size_t stride_bytes,
                     const eu_switches &sw, hipStream_t st, const eu_encode *enc = nullptr, bool rgbe = false,
                     const ycbcr_dst *yc = nullptr, eu_mb_times *mb_times = nullptr);

// mean GPU time of `iters` calls of once() on the library's stream between two events, after one untimed call (which
// builds whatever the first call builds: a plan's tables, derived copies)
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
  HIPCHK(hipEventRecord(ev.a, cur().stream));
  for (int i = 0; i < iters; i++)
    if ((rc = once())) return rc;
  HIPCHK(hipEventRecord(ev.b, cur().stream));
  HIPCHK(hipEventSynchronize(ev.b));
  float ms = 0.0f;
  HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
  *mean_ms = ms / iters;
  return EU_OK;
}

}  // namespace eu_host

#endif
