// The boundary between the C ABI's host glue (eu_api.hip, eu_api_*.hip) and the kernel files, declared once: the
// launchers, the argument structure of the multi-facet kernels and a typed device buffer.
#ifndef EU_LAUNCH_H
#define EU_LAUNCH_H
#include <hip/hip_runtime.h>
#include <cstddef>
#include "eu_device.h"
#include "eu_select.h"
#include "eu_worklist.h"

// early-miss tables of a multi-facet job (eu_render_multi.hip: eu_multi_maybe): per facet a header and
// EU_REJ_N bins over u = cos(angle to the facet's axis)
#define EU_REJ_N 1024
#define EU_REJ_HDR 16
#define EU_REJ_STRIDE (EU_REJ_HDR + EU_REJ_N)

// how a multi-facet job composes its facets: eu_target::synopsis (EU_SYN_*), one kernel family per mode
// (EU_MODE_LAYERS: stage A of EU_SYN_MULTIBAND, eu_synopsis_layers - the feathered loop writing layer planes)
// EU_MODE_FEATHER_EDGES, EU_MODE_LAYERS_EDGES: the same two loops in jobs where some facet keeps a distance plane
// (EU_LOAD_EDGES) - instantiations of their own, so that every other job runs the kernels it ran without them
enum { EU_MODE_PANORAMA = 0, EU_MODE_HDR = 1, EU_MODE_FEATHER = 2, EU_MODE_LAYERS = 3, EU_MODE_FEATHER_EDGES = 4,
       EU_MODE_LAYERS_EDGES = 5 };
constexpr bool eu_mode_feather(int m) { return m == EU_MODE_FEATHER || m == EU_MODE_FEATHER_EDGES; }
constexpr bool eu_mode_layers(int m) { return m == EU_MODE_LAYERS || m == EU_MODE_LAYERS_EDGES; }

// feathered seams (eu_synopsis_feather): what the edge weight of one facet needs. It belongs to the JOB - the
// width is the target's - and not to the resident source, so it travels beside eu_src_dev: 40 bytes per facet,
// read wave-uniformly through the scalar cache.
struct eu_feather_dev {
  float rcp;                 // float(1.0 / width_px): the ramp's slope per window pixel
  float lim_x, lim_y;        // float(window size) - 0.5f: the far border in pixel coordinates
  int border;                // bit 0: axis 0 has a border, bit 1: axis 1; 0: the weight is 1
  const float *dist;         // the facet's distance plane (EU_LOAD_EDGES), dist_w x dist_h floats, dense; nullptr: none
  int dist_w, dist_h;
  int cyclic;                // the plane's rows close: column indices wrap
};

struct eu_multi_params {
  int width, height, row_begin, row_end;
  int form, norm_mode, twine, ntaps, nch, nfct, plus;
  const float *col;          // [4][width], shared by all facets
  const float *row;          // [nfct][height][EU_ROW_FLOATS]
  const float *taps;         // [ntaps][3], x/y scaled by 4
  const eu_src_dev *srcs;    // [nfct]
  float *out;
  long long out_stride;
  int tiles_x, tiles_y;
  int band_shift, band_count, band_index;   // eu_frame_row
  int mode;                                 // EU_MODE_* (fill_synopsis: the _EDGES forms where a facet has a plane)
  int hdr_low, hdr_high;                    // _hdr_merge_syn: the facets that rule the shadows / the highlights
  const eu_feather_dev *fth;                // [nfct], EU_MODE_FEATHER / EU_MODE_LAYERS: the job's edge-weight table
  float *lay;                               // EU_MODE_LAYERS: the layer planes (eu_multiband.h), `out` is not written
  long long lay_plane;                      // floats from one plane to the next: width * rows
  const eu_generic *gen;                    // [nfct] or nullptr: facets stepped by generic_stepper (translation)
  eu_inv_planar inv;                        // tf22 of a --single job
  const float *rej;                         // [nfct][EU_REJ_STRIDE] or nullptr: early-miss tables (eu_multi_maybe)
};

struct eu_alpha_params;      // eu_alpha.h

// Device memory that only ever grows. reserve() frees and allocates: the old contents are gone, and the
// capacity stays 0 when the allocation fails.
template <class T> struct eu_dev_buf {
  T *p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t n)
  {
    if (cap >= n) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    const hipError_t e = hipMalloc((void **)&p, n * sizeof(T));
    if (e == hipSuccess) cap = n; else p = nullptr;
    return e;
  }
};

// Who may still read a family of such buffers on a CALLER's stream: one event of the library's own, recorded behind
// every call that leaves work on such a stream, so no stream handle outlives the call that brought it. Whoever
// rewrites the buffers waits first - the host (host_wait: a blocking copy, a reserve() that may free, a host copy
// an upload still reads) or, where the rewrite is itself queued on a stream, that stream (order_after). The
// library's own stream records nothing: it is waited for by handle.
struct eu_readers {
  hipEvent_t ev = nullptr;
  bool recorded = false;
  // One event serves any number of streams: `st` waits for the readers noted before it, then the event moves behind
  // st's work, so the event's completion still means that ALL of them are through. The wait delays nothing this call
  // queued, only what `st` gets later; for an event last recorded on `st` itself the runtime does nothing.
  hipError_t note(hipStream_t st)
  {
    hipError_t e = ev ? order_after(st) : hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(ev, st);
    if (e == hipSuccess) recorded = true;
    return e;
  }
  hipError_t host_wait() const { return recorded ? hipEventSynchronize(ev) : hipSuccess; }
  hipError_t order_after(hipStream_t st) const { return recorded ? hipStreamWaitEvent(st, ev, 0) : hipSuccess; }
};

// The render launchers return 0, or a negative value: -1 a HIP error, -2 a job outside the kernel's
// coverage (eu_select.h decides before the call, so that is a bug of the caller).
extern "C" {
int eu_launch_render(const eu_render_params *p, void *stream);
int eu_launch_render2(const eu_render_params *p, const eu_switches *sw, void *stream);
// h_row, h_col: the host copies of the plan's row table (whole frame) and column table, plan_gen: changes whenever the stepper tables
// change. *launches: kernels launched for the job - 0 where the plan of a lat/lon job says that the
// direct-gather kernels are faster (eu_staged_worth; the plan stays cached). The cached plans and p->wl belong to
// one launch pair at a time: the caller has ordered `stream` behind the pair launched before (launch_staged).
// p->wl is this pair's set of the work list's two, wl_next the other one, whose counters the pair empties for the
// pair behind it (eu_worklist.h)
int eu_launch_render4(const eu_render_params *p, int *wl_next, const eu_switches *sw, const float *h_row, size_t h_row_floats,
                      const float *h_col, size_t h_col_floats, unsigned long long plan_gen, void *stream, int *launches);
// path: an eu_ray_path, as eu_select_ray_path() chose it
int eu_launch_render_rays(const eu_rays_params *p, int path, void *stream);
// eu_render_views.hip. The table kernel: col [nviews][6][width] and row [nviews][height][EU_ROW_FLOATS] from the
// views' scalar blocks. The render kernels: p describes view 0 of the launch, path is an eu_view_path
int eu_launch_view_tables(const eu_view_dev *views, int nviews, int prj, int width, int height, int twine, float *col,
                          float *row, void *stream);
int eu_launch_render_views(const eu_render_params *p, const eu_view_strides *vs, int nviews, int path,
                           const eu_switches *sw, void *stream);
// eu_render_layers.hip: p describes the job with layer 0's source block, lp the layers of this launch; path is an
// eu_layer_path
int eu_launch_render_layers(const eu_render_params *p, const eu_layers_params *lp, int path, const eu_switches *sw,
                            void *stream);
int eu_launch_render_multi(const eu_multi_params *p, int degree, void *stream);
int eu_launch_render_multi_nch1(const eu_multi_params *p, int degree, void *stream);
int eu_launch_render_multi_nch2(const eu_multi_params *p, int degree, void *stream);
int eu_launch_render_multi_nch3(const eu_multi_params *p, int degree, void *stream);
int eu_launch_render_multi_nch4(const eu_multi_params *p, int degree, void *stream);
// eu_render_views_multi.hip: p describes view 0 of the launch (col [6][width], row [nfct][height][EU_ROW_FLOATS],
// out), vs what lies between one view's tables and frame and the next one's
int eu_launch_render_views_multi(const eu_multi_params *p, const eu_view_strides *vs, int nviews, int degree, void *stream);
int eu_launch_render_views_multi_nch1(const eu_multi_params *p, const eu_view_strides *vs, int nviews, int degree, void *stream);
int eu_launch_render_views_multi_nch2(const eu_multi_params *p, const eu_view_strides *vs, int nviews, int degree, void *stream);
int eu_launch_render_views_multi_nch3(const eu_multi_params *p, const eu_view_strides *vs, int nviews, int degree, void *stream);
int eu_launch_render_views_multi_nch4(const eu_multi_params *p, const eu_view_strides *vs, int nviews, int degree, void *stream);
int eu_launch_to_screen(const float *in, long long in_stride, unsigned *out, long long out_stride, int w, int rows,
                        int nch, const float *lut, void *stream);
// iir_stream: eu_switches::iir_stream
int eu_launch_prefilter(float *container, const eu_container *g, int nch, int bc0, int bc1, int prefilter_degree,
                        int spherical, int iir_stream, void *stream);
int eu_launch_cubemap_build(const float *faces_dev, float *ir_dev, int nch, long face_px, long section_px,
                            long left_frame, long right_frame, double refc_md, double model_to_px,
                            int prefilter_degree, int iir_stream, void *stream);
int eu_launch_facet_alpha(const eu_alpha_params *p, void *stream);
int eu_launch_diag(const eu_render_params *p, unsigned long long *stamps_dev, void *stream);
int eu_launch_diag_coords(const eu_src_dev *s, const float *rays_dev, long n, int variant, float *out_dev,
                          void *stream);
int eu_launch_selftest(unsigned long long seed, int blocks, int iters, unsigned long long *bad_dev, void *stream);
int eu_verify_const_div(float c, float limit, void *stream);   // 1: the three-operation division is exact
int eu_current_slot(void);                                     // the device slot the entry points work on
}

#endif
