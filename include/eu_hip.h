/* eu_hip.h - C ABI of the MI355X-native envutil reprojection path.
 *
 * This is the drop-in boundary for ONE path of kfjahnke/envutil: the
 * per-output-pixel reprojection that the reference runs as
 *   zimt::process(trg.shape, get, act, cstor, bill)      envutil_payload.cc:541
 * behind
 *   dispatch_base::payload(nchannels, ninputs, projection) envutil_dispatch.h:49-65
 * Everything here is plain C: pointers, sizes, PODs. No torch types, no C++.
 * A reference maintainer binds it exactly where the per-ISA `dispatch` structs
 * are built today (envutil_payload.cc:2390-2442); INTEGRATION.md shows the stub.
 *
 * Conventions: axes RIGHT, DOWN, FORWARD; cube faces
 * LEFT0 RIGHT1 TOP2 BOTTOM3 FRONT4 BACK5 stacked vertically; angles in radians;
 * pixels are interleaved float32 channels, x fastest, rows contiguous.
 *
 * All functions return 0 on success or a negative eu_status code; none of them
 * aborts. eu_hip_last_error() gives the text for the calling thread.
 *
 * Threading: like the reference's payload (called on the main thread, global `args`), the
 * library is NOT re-entrant: one host thread at a time, one device per process (the first
 * eu_hip_init or the first call fixes it). A caller-supplied stream orders the KERNELS of a
 * render; the stepper tables of a job are uploaded synchronously before its launch. Behind
 * every call that leaves work on a caller's stream the library records an event of its own,
 * and it waits for those events before it rewrites a buffer such work may read, so jobs on
 * different streams never race on the library's own buffers, nor on a source's container: every
 * source notes the renders that read it on a caller's stream, eu_hip_source_reload goes behind
 * them, and every render goes behind the reloads of its sources. No stream handle is kept beyond
 * the call that brought it: a stream may be destroyed once its own work is done.
 * eu_hip_sync() waits for the library's stream and for everything any call so far has left
 * on a caller's stream.
 */
#ifndef EU_HIP_H
#define EU_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mirrors projection_t, envutil_basic.h:68-78 */
typedef enum {
  EU_SPHERICAL = 0, EU_CYLINDRICAL, EU_RECTILINEAR, EU_STEREOGRAPHIC,
  EU_FISHEYE, EU_CUBEMAP, EU_BIATAN6, EU_PRJ_NONE
} eu_projection;

/* mirrors zimt::bc_code, zimt/common.h:82-91 */
typedef enum {
  EU_BC_MIRROR = 0, EU_BC_PERIODIC, EU_BC_REFLECT, EU_BC_NATURAL,
  EU_BC_CONSTANT, EU_BC_ZEROPAD, EU_BC_GUESS
} eu_bc;

typedef enum {
  EU_OK = 0,
  EU_ERR_NO_DEVICE = -1,     /* no HIP device / HIP runtime error            */
  EU_ERR_ARGUMENT = -2,      /* inconsistent or out-of-range argument        */
  EU_ERR_UNSUPPORTED = -3,   /* valid for the reference, not built yet here  */
  EU_ERR_MEMORY = -4,
  EU_ERR_HANDLE = -5
} eu_status;

#define EU_MAX_DEGREE 9
#define EU_MAX_TAPS 1024
#define EU_MAX_FACETS 64

/* One source image. Mirrors the fields of facet_spec / facet_base that the
 * render path reads (envutil_basic.h:432-520). `step`, `brighten` as there. */
typedef struct eu_facet {
  int32_t projection;            /* eu_projection                              */
  int32_t nchannels;             /* 1..4                                       */
  double  hfov;                  /* radians                                    */
  int32_t width, height;         /* total size; cubemaps: face width, height=6w*/
  int32_t window_width, window_height, window_x_offset, window_y_offset;
  double  yaw, pitch, roll;      /* radians                                    */
  double  brighten;              /* facet_spec::brighten                       */
  double  step;                  /* facet_base::step (get_step)                */
  int32_t has_lcp;               /* lens polynomial / shift / shear present    */
  double  a, b, c, h, v, s, shear_g, shear_t;
  /* PTO translation (facet_base::tr_*, tp_*, envutil_basic.h:446-447): position of the virtual camera
   * in model space units and the orientation of the translation plane (radians). A facet with
   * tr_x/y/z != 0 is stepped by generic_stepper over tf_ex_facet (envutil_payload.cc:2095-2110,
   * :2145-2158; geometry.h:1850-1941) instead of the target projection's own stepper.            */
  double  tr_x, tr_y, tr_z, tp_y, tp_p, tp_r;
  /* --mask_for (facet_spec::masked, envutil_main.cc:1077-1092; masking.h:70-135): 0 ordinary
   * pixels (masked == -1), 1 the facet is painted black (masked == 0), 2 white (masked == 1).
   * Facets of 1 / 3 channels yield the paint, facets with alpha paint * alpha and their alpha;
   * a target with another channel count takes them through mono_t (1 or 2 channels only).   */
  int32_t mask_paint;
} eu_facet;

typedef struct eu_source eu_source;   /* opaque: coefficients resident in HBM */

/* Geometry of a braced b-spline container as zimt::bspline lays it out
 * (zimt/bspline.h:305-450, :759-820); filled by eu_hip_container_geometry. */
typedef struct eu_container {
  int64_t shape[2];              /* container shape, pixels                    */
  int64_t left[2], right[2];     /* frame widths                               */
  int64_t core[2];               /* core shape                                 */
} eu_container;

/* The target image and job parameters that travel in envutil's global `args`
 * (envutil_basic.h:633-705): extent as computed by get_extent
 * (envutil_basic.cc:156-229), camera orientation, twining tap table as
 * produced by make_spread (envutil_main.cc:1253-1355; ntaps = 0: ninputs 3). */
typedef struct eu_target {
  int32_t projection;
  int32_t width, height;
  /* EU_SYN_MULTIBAND: multi-band (Burt-Adelson) blending, this library's own like EU_SYN_FEATHER; `bands` is the
   * number of pyramid levels above level 0, 0 for the default, negative: EU_ERR_ARGUMENT. `feather` is read as
   * under EU_SYN_FEATHER. Float32 throughout, one operation at a time, no contraction.
   * Stage A, per target pixel, facets in job order: feather's own steps (ray, early miss, exact hit, the facet's
   * pixel, the ramp e). A facet the ray hits gives q = e and the colour c = pixel, with alpha a: q = a * e and
   * c = a > 1e-6 ? v / a : 0. Layers: Q_f = q on a hit, else 0; M_f = Q_f > 0 ? 1 : 0; X_f = M_f ? c : 0 per
   * colour channel. qsum = sum Q_f, amax = the largest alpha over the hits, count = the hits;
   * W_f = qsum > 0 ? Q_f / qsum : 0.
   * Levels: w_{l+1} = (w_l + 1) >> 1, h likewise. L = bands clamped to L_max, the largest L whose coarsest level
   * keeps min(w_L, h_L) >= 4 (L_max may be 0: the frame is then the level-0 blend alone); bands = 0:
   * min(L_max, 8). Column indices wrap (i mod n) when the target is spherical or cylindrical with 360 degrees,
   * and L_max is then further limited so that width % 2^L == 0; otherwise, and for rows always, indices clamp.
   * Reduce R, along the rows first:
   *   h[r, i] = (((A[r, 2i-2] + A[r, 2i+2]) + 4 * (A[r, 2i-1] + A[r, 2i+1])) + 6 * A[r, 2i]) * 0.0625
   * then the same formula down the rows 2j-2 .. 2j+2 of h. Expand E to the finer level's size, along the rows
   * first, then the same down the columns of the result: even 2i: ((A[i-1] + A[i+1]) + 6 * A[i]) * 0.125,
   * odd 2i+1: (A[i] + A[i+1]) * 0.5.
   * Pyramids per facet: X^{l+1} = R(X^l), M^{l+1} = R(M^l), W^{l+1} = R(W^l). Bands, facets in job order, only
   * where M_f^l > 0: l < L: B = X^l / M^l - E(X^{l+1}) / E(M^{l+1}), the second term 0 where E(M^{l+1}) is not
   * positive; l = L: B = X^L / M^L; num^l += W_f^l * B, den^l += W_f^l.
   * Collapse: O^L = den > 0 ? num / den : 0; O^l = (den^l > 0 ? num^l / den^l : 0) + E(O^{l+1}).
   * Pixel: zeros where count == 0; without alpha O^0; with alpha O^0 * amax and alpha = amax.
   * Unlike EU_SYN_FEATHER, a pixel that only ONE facet covers is NOT that facet's pixel bit for bit: it has been
   * through the pyramid. Another facet's weights reach 4 * 2^l pixels beyond it on level l, so next to a seam the
   * low bands of the neighbour are mixed in, by design. Out of every other facet's reach a facet of ONE colour comes
   * back within rounding; a textured facet comes back changed in the pixels near its own border too, because there
   * E(X^{l+1}) / E(M^{l+1}) is not E(X^{l+1} / M^{l+1}), and within rounding only in its interior, where M is 1.
   * The pyramid needs the whole frame at once: twining, a row range other than the whole frame, row bands, a crop
   * window, EU_OUT_SRGBA8, --mask_for facets, eu_hip_render_devices with more than one slot and
   * eu_hip_render_views_multi are refused with EU_ERR_ARGUMENT before a device is looked for. The scratch lives
   * in the device context: eu_hip_multiband_scratch_bytes, eu_hip_multiband_scratch_release.
   * Other synopses ignore the field; set it (0) always.
   * The field lies in what was the 4-byte alignment gap in front of x0: the structure's size and every other
   * field's offset are what they were, so callers built against the older header keep working (they never set
   * EU_SYN_MULTIBAND, and the field is read under that synopsis alone).                                                       */
  int32_t bands;
  double  x0, x1, y0, y1;
  double  yaw, pitch, roll;
  int32_t nchannels;
  int32_t ntaps;
  const float *taps;             /* host pointer, ntaps x {x, y, weight}       */
  int32_t row_begin, row_end;    /* rows [row_begin,row_end): multi-GPU tiling */
  int32_t stage;                 /* 0 pixels; 1 rays; 2 source coordinates;
                                    3 / 4 the rays of the x-biased / y-biased
                                    stepper of a twined job (ntaps > 0; else
                                    EU_ERR_ARGUMENT): with stage 1 the ninepack
                                    twine_t::eval reads, see eu_rays. Stages
                                    1-4 write 3 floats per pixel, single-facet
                                    jobs only                                  */
  /* args.store_cropped + p_crop_* (envutil_basic.h:684-687; applied at
   * envutil_payload.cc:440-474): the job renders crop_w x crop_h pixels whose
   * discrete coordinates start at (crop_x0, crop_y0) of the width x height
   * frame (zimt's bill.get_offset). crop_w == 0: the whole frame. Rows,
   * row_begin/row_end and the output buffer are those of the cropped frame.  */
  int32_t crop_x0, crop_y0, crop_w, crop_h;
  /* EU_OUT_FLOAT: nchannels floats per pixel (zimt::storer).
   * EU_OUT_SRGBA8: one packed uint32 per pixel, the tethered 'act + to_screen_t'
   * pipeline writing args.p_screen_data (envutil_payload.cc:251-413, :524-530);
   * the output buffer is then uint32 and strides still count bytes.          */
  int32_t out_format;
  /* Multi-GPU tiling by INTERLEAVED row bands (load balance: rows differ in
   * cost, e.g. the polar faces of a cubemap target take 1.7x the others): the
   * frame's rows are cut into bands of band_rows rows (a power of two >= 4),
   * band b belongs to part b % band_count, and this call renders the bands of
   * part band_index, compacted in order: local row l is frame row
   * ((l / band_rows) * band_count + band_index) * band_rows + l % band_rows.
   * row_begin/row_end and the output buffer then count LOCAL rows
   * (eu_hip_band_rows tells how many there are). band_count <= 1: off.       */
  int32_t band_rows, band_count, band_index;
  /* args.synopsis (envutil_main.cc:232, dispatched at envutil_payload.cc:2302-2318): how a job
   * with several facets composes them. EU_SYN_PANORAMA: voronoi_syn (1/3 channels) or
   * voronoi_syn_plus (2/4 channels); EU_SYN_HDR_MERGE: _hdr_merge_syn (envutil_payload.cc:
   * 1325-1626), the quality-weighted sum of ALL facets; EU_SYN_FEATHER: feathered seams, this library's own
   * (the reference has no blending): every facet the ray hits, weighted by its distance to the nearest border
   * of the facet's window - see `feather` below. Ignored for single-facet jobs.                 */
  int32_t synopsis;
  /* args.single (envutil_main.cc:1161-1180; envutil_payload.cc:2058-2069): the target RECREATES this facet.
   * Projection, size, extent and orientation above are then the facet's own ((facet_base&) args = fspec);
   * this pointer hands over what a target otherwise does not have - lens polynomial, shift, shear and
   * translation - and when any of them is set every facet of the job is stepped by generic_stepper over
   * tf_ex_facet with the inverse planar transformation (pto_planar<T, L, true>, inverse_lcp) and the
   * inverse translation. Host pointer, read during the call; NULL: an ordinary target.            */
  const eu_facet *single;
  /* EU_SYN_FEATHER: the width of the blending ramp in SOURCE pixels; 0, the default: half the shorter side of
   * each facet's window, so that the ramp reaches the window's centre. Per facet the ray hits, in float32, one
   * operation at a time, facets in job order:
   *   dx = min(sx + 0.5, (window_width - 0.5) - sx), dy likewise   (sx, sy: the source coordinate, centres whole)
   *   d  = the smaller over the axes that have a border - not axis 0 of a 360-degree spherical / cylindrical
   *        source, not axis 1 of a full sphere, neither of a cubemap or of a fisheye of 360 degrees or more
   *   e  = clamp(d * float(1.0 / width), 2^-16, 1), or 1 without a bordered axis
   *   no alpha: acc += pixel * e, qsum += e;   alpha a: acc += (a > 1e-6 ? colour / a : 0) * (a * e),
   *   qsum += a * e, amax = max(amax, a)
   * and the pixel is acc / qsum (0 unless qsum > 0), with alpha times amax and alpha = amax. A miss contributes
   * nothing; a pixel ONE facet hits is that facet's pixel as it is; none: zeros. With --mask_for N (mask_paint)
   * the frame is facet N's normalised blend weight. Negative or non-finite: EU_ERR_ARGUMENT. Other synopses and
   * single-facet jobs ignore the field, but the plan cache hashes the structure's bytes: set it (0) always.  */
  double feather;
} eu_target;

/* How the library would lay the job's rows out (eu_api_render.hip: launch-level choice between
 * row strips and 32x16 tiles): flags[k] = 1 for segment k of *seg_rows frame rows where
 * source rows run across target rows - those rows take about 1.55x the time of the others,
 * about 2x when they are part of a strip they break into several launches. For hosts that
 * split a frame into CONTIGUOUS strips of equal cost. Returns the number of segments
 * (0 when the job has no such structure) or a negative eu_status. */
int  eu_hip_layout_segments(const eu_target *trg, eu_source *const *srcs, int nsrc,
                            unsigned char *flags, int max_flags, int *seg_rows);

/* render kernel launches issued so far by this process (single-facet path) */
unsigned long long eu_hip_launch_count(void);

/* 16x16 tiles that the last staged launch (eu_render5_kernel's first loop) rendered from the
 * coordinates of another tile - the column mirror, the same rows of another cube face; 0 where
 * the tables the kernel reads do not agree bit for bit, and under EU_HIP_SHARE=0 */
unsigned long long eu_hip_share_follower_tiles(void);

/* 16x8 tiles that the last staged launch (eu_render5_kernel's second loop, where it reads the box table)
 * rendered from the angles of another tile - the twin on the opposite polar face, the column mirror; 0
 * where the tables the kernel reads do not agree bit for bit, and under EU_HIP_POLAR_SHARE=0 */
unsigned long long eu_hip_polar_follower_tiles(void);

/* 16x8 wave tiles that the last staged launch pair of this process handed to its second kernel, the
 * direct-gather kernel, through the work list (tiles whose texel box does not fit a wave's LDS slice, tiles
 * with a lane on a scalar fallback of the coordinate arithmetic); waits for that pair. 0 before the first
 * staged launch. A job that took another path leaves the count of the last staged pair in place, and so does
 * a staged strip of no tiles (nothing is launched for it). A hook for tests, for a process that renders on ONE
 * device: it reads the current device's list without selecting a device, and it copies the word with a
 * blocking hipMemcpy on the null stream, which also waits for every other blocking stream. */
unsigned long long eu_hip_listed_tiles(void);

/* number of local rows of part band_index (see eu_target.band_*) in a frame of
 * `height` rows; height itself when band_count <= 1 */
int  eu_hip_band_rows(int height, int band_rows, int band_count, int band_index);

enum { EU_OUT_FLOAT = 0, EU_OUT_SRGBA8 = 1 };
/* (3 is not assigned: it stays an unknown synopsis, refused with EU_ERR_ARGUMENT) */
enum { EU_SYN_PANORAMA = 0, EU_SYN_HDR_MERGE = 1, EU_SYN_FEATHER = 2, EU_SYN_MULTIBAND = 4 };

/* ---- multi-band blending (eu_target::bands has the definition) ------------- */
/* Bytes of device scratch an EU_SYN_MULTIBAND job of `nsrc` facets on `trg` takes (0 for nsrc < 2); a host
 * function, no device is looked for. With S_l = w_l * h_l, T = S_0 + .. + S_L and ncol colour channels (the
 * channels without alpha): 4 * (S_0 * (nsrc * (ncol + 1) + 3) + ncol * (T - S_0) + 2 * T + (ncol + 1) * T).   */
size_t eu_hip_multiband_scratch_bytes(const eu_target *trg, int nsrc);
/* waits for every multi-band job so far and frees the scratch they share (all device slots) */
int  eu_hip_multiband_scratch_release(void);
/* The pyramid on the caller's own remapped pictures - what a multi-band render runs behind stage A: `colour` is
 * (nlayers, height, width, nchannels) float32 and plays c, `weight` is (nlayers, height, width) and plays Q
 * (a weight that is not positive counts as 0); there is no alpha and no count: every pixel is O^0. Strides in
 * bytes, multiples of 4; pixels are dense. `in_on_device` says where colour and weight lie, `out_on_device` where
 * `out` (height rows of width * nchannels floats) lies; `stream` as for eu_hip_render (NULL: the library's own; a
 * host buffer on either side makes the call return when `out` is complete). wrap != 0: column indices wrap.
 * EU_ERR_ARGUMENT, before a device is looked for: null pointers, nlayers < 1, nchannels outside 1 .. 4, sizes
 * below 1, negative bands, strides smaller than a row / a picture or no multiple of 4. EU_ERR_MEMORY: the scratch
 * could not be allocated.                                                                                     */
int  eu_hip_blend_layers(const float *colour, size_t colour_row_stride_bytes, size_t colour_layer_stride_bytes,
                         const float *weight, size_t weight_row_stride_bytes, size_t weight_layer_stride_bytes,
                         int in_on_device, int nlayers, int width, int height, int nchannels, int bands, int wrap,
                         float *out, size_t out_row_stride_bytes, int out_on_device, void *stream);
/* the levels a width x height frame gets for `bands` (eu_target::bands): L, or a negative eu_status */
int  eu_hip_multiband_levels(int width, int height, int bands, int wrap);

/* ---- device / lifecycle ------------------------------------------------- */
int  eu_hip_device_count(void);
int  eu_hip_init(int device);                 /* selects the device for this process */
const char *eu_hip_last_error(void);

/* ---- one process, several devices (round 3; SURVEY 8e: the output rows tiled across the GPUs of a node;
 * the reference has no counterpart - its payload() runs on the host's cores) --------------------------------
 * eu_hip_init_devices makes one device SLOT per entry of `devices` (at most EU_MAX_SLOTS; the same device may
 * be listed more than once: separate streams, tables and buffers - how a one-GPU box tests this). Sources are
 * created on slot 0 as before; eu_hip_render_devices replicates them onto the other slots on first use
 * (hipMemcpyPeerAsync over xGMI: the "broadcast of the source environment"), cuts the frame into contiguous
 * strips of equal estimated cost, renders strip k on slot k - all slots concurrently - and gathers the strips
 * into `out` (a host buffer, or device memory of slot 0: peer copies). Same pixels as eu_hip_render. */
#define EU_MAX_SLOTS 16
int  eu_hip_init_devices(const int *devices, int ndevices);
int  eu_hip_device_slots(void);               /* 1 unless eu_hip_init_devices was called */
int  eu_hip_render_devices(const eu_target *trg, eu_source *const *srcs, int nsrc, float *out,
                           size_t out_row_stride_bytes, int out_on_device);
/* the rows [begin[k], end[k]) eu_hip_render_devices gives slot k for this job (nslots entries each) */
int  eu_hip_device_strips(const eu_target *trg, eu_source *const *srcs, int nsrc, int *begin, int *end);

/* ---- set-up arithmetic shared with the reference's host code ------------- */
/* get_extent / get_vfov / get_step, envutil_basic.cc:49-229 */
int  eu_hip_get_extent(int projection, int width, int height, double hfov,
                       double *x0x1y0y1);
double eu_hip_get_step(int projection, int width, int height, double hfov);
/* make_spread, envutil_main.cc:1253-1355; returns tap count or <0 */
int  eu_hip_make_spread(int w, int h, float d, float sigma, float threshold,
                        float *taps, int max_taps);
/* metrics_t, cubemap.h:233-400: section_px, left/right frame, refc_md, model_to_px */
/* PTO exclude masks and lens crops: the edit of a facet's loaded pixels that source_t's
 * constructor makes before it prefilters (environment.h:700-890; fill_polygon,
 * envutil_basic.cc:236-320; zimt::convolve with the binomial 1 4 6 4 1 / 16, REFLECT).
 * HOST function, no device needed: `pixels` (width x height x nchannels, nchannels 2 or 4,
 * alpha last) is multiplied in place, every channel, by the softened alpha plane; `alpha_out`
 * (width x height floats) receives that plane when it is not NULL.
 * crop_kind: 0 none, 1 rectangular [x0, x1) x [y0, y1), 2 elliptic (fisheye images). */
typedef struct eu_mask_polygon { int n; const float *x; const float *y; } eu_mask_polygon;
int  eu_hip_facet_alpha(float *pixels, int width, int height, int nchannels,
                        const eu_mask_polygon *polygons, int npolygons, int crop_kind,
                        int crop_x0, int crop_x1, int crop_y0, int crop_y1, float *alpha_out);
/* rows of the stage-0 alpha plane (before the binomial): pixel (x, y) is 0 iff x is outside
 * keep[2y] .. keep[2y+1] or inside one of the spans row_start[y] .. row_start[y+1] (pairs [x0, x1),
 * clipped to the image). keep: 2 x height, row_start: height + 1 entries (either may be NULL).
 * spans == NULL: count only. Returns the number of spans or a negative eu_status (EU_ERR_ARGUMENT
 * when there are more than max_spans). Host function: this integer plan is all the device form of
 * the edit reads, a few KB whatever the image's size. */
int  eu_hip_facet_alpha_rows(int width, int height, const eu_mask_polygon *polygons, int npolygons,
                             int crop_kind, int crop_x0, int crop_x1, int crop_y0, int crop_y1,
                             int32_t *keep, int32_t *row_start, int32_t *spans, int max_spans);
/* The same edit, made on the device (eu_alpha.hip; bit for bit the host function's result). */
typedef struct eu_facet_edit {
  const eu_mask_polygon *polygons; int32_t npolygons;      /* PTO k-lines, variant 0          */
  int32_t crop_kind, crop_x0, crop_x1, crop_y0, crop_y1;   /* as eu_hip_facet_alpha           */
  int32_t pixel_channels;     /* channels of `pixels`: fct->nchannels or fct->nchannels - 1   */
  int32_t pixels_on_device;   /* `pixels` is device memory of the library's device            */
} eu_facet_edit;
/* device twin of eu_hip_facet_alpha: pixels_dev (may be NULL; width x height x nchannels, dense,
 * edit->pixel_channels == nchannels) edited in place, alpha_out_dev (may be NULL) receives the
 * plane; asynchronous on `stream` (NULL: the library's). edit == NULL: nothing is cleared. */
int  eu_hip_facet_alpha_dev(void *pixels_dev, int width, int height, int nchannels,
                            const eu_facet_edit *edit, float *alpha_out_dev, void *stream);
int  eu_hip_cubemap_metrics(int face_px, double face_fov, int support_min,
                            int tile_px, int64_t *section_px,
                            int64_t *left_frame_px, double *refc_md,
                            double *model_to_px);
int  eu_hip_container_geometry(int degree, int bc0, int bc1, int64_t w,
                               int64_t h, eu_container *out);

/* ---- sources: the asset_handler residency (environment.h:84-227) --------- */
/* Load pixel data (host pointer, window_width x window_height interleaved
 * floats; cubemaps: 6 stacked faces), build the braced coefficient container
 * in HBM and prefilter it ON THE DEVICE, as source_t's constructor
 * (environment.h:594-962) or cubemap_t::load (cubemap.h:1147-1233) do on the
 * CPU. */
int  eu_hip_source_load(const eu_facet *fct, const float *pixels,
                        int spline_degree, int prefilter_degree,
                        int support_min, int tile_size, eu_source **out);
/* eu_hip_source_load with source_t's alpha edit (environment.h:700-890) done on the device on the
 * way into the container: a facet of a PTO project with exclude masks or a lens crop. `pixels` has
 * edit->pixel_channels channels - where that is nchannels - 1 the facet gains its alpha channel
 * here, set to 1 before the edit (environment.h:707-725) - and lies in host memory or, with
 * edit->pixels_on_device, in memory of the library's device. Cubemaps: the plane is the stack of
 * six faces. An edit needs nchannels 2 or 4. edit == NULL, or no polygons, crop_kind 0 and
 * pixel_channels == nchannels: the same container as eu_hip_source_load. Argument errors are
 * reported before a device is looked for. */
int  eu_hip_source_load_edited(const eu_facet *fct, const void *pixels, const eu_facet_edit *edit,
                               int spline_degree, int prefilter_degree, int support_min,
                               int tile_size, eu_source **out);
/* The same container from 8- or 16-bit integer samples: a decoder's frame, the payload of a PNM / PAM file.
 * The samples go to the device as they are - a quarter or half of the float image's bytes - and become
 * floats there (eu_decode.hip) through the caller's tables, on the way into the container: bit for bit the
 * container eu_hip_source_load_edited builds from float pixels p[i] = table_of_channel[sample[i]] with the
 * same edit (edit == NULL: none; edit->pixel_channels and edit->pixels_on_device are ignored in favour of
 * smp). The tables ALWAYS have 1 << bits entries, so that every bit pattern has one - samples above a PNM
 * file's maxval too; the library knows nothing of colour spaces or of maxval, the tables say it all. Argument
 * errors (EU_ERR_ARGUMENT) are reported before a device is looked for: null pointers, bits other than 8 or
 * 16, pixel_channels other than nchannels or nchannels - 1 or below 1, a null colour_table, an edit or a
 * gained channel on a facet whose nchannels is not 2 or 4, device data of 16-bit samples at an odd address,
 * degrees out of range. */
typedef struct eu_samples {
  const void *data;          /* width x height x pixel_channels samples, rows dense; cubemaps: the six faces stacked */
  int32_t bits;              /* 8: uint8_t, 16: uint16_t */
  int32_t big_endian;        /* bits 16: high byte first, as PNM / PAM store it; 0: host order */
  int32_t pixel_channels;    /* fct->nchannels, or fct->nchannels - 1: the facet gains alpha = 1.0f here */
  int32_t on_device;         /* `data` is memory of the library's device */
  const float *colour_table; /* host, 1 << bits floats: the float a colour sample becomes */
  const float *alpha_table;  /* host, 1 << bits floats: the same for the LAST channel when pixel_channels is 2 or 4;
                                NULL: colour_table for it too */
} eu_samples;
int  eu_hip_source_load_samples(const eu_facet *fct, const eu_samples *smp, const eu_facet_edit *edit,
                                int spline_degree, int prefilter_degree, int support_min, int tile_size,
                                eu_source **out);
/* The same container from Radiance RGBE pixels (include/eu_rgbe.h): the payload of a .hdr / .pic file with its
 * scanlines expanded. The quads go to the device as they are - a third of the float image's bytes - or are read
 * where they lie there, and become floats (eu_rgbe.hip) on the way into the container: bit for bit the container
 * eu_hip_source_load_edited builds from the decoded floats with the same edit (edit == NULL: none;
 * edit->pixel_channels and edit->pixels_on_device are ignored in favour of px). fct->nchannels is 3, or 4: the facet
 * gains alpha = 1.0f here. The optional table serves a facet whose colour space is not the working one: a channel's
 * float is a function of its (E, mantissa) pair alone, so 65536 entries say it all. Argument errors
 * (EU_ERR_ARGUMENT) are reported before a device is looked for: null pointers, nchannels other than 3 or 4, masks
 * or a crop on a facet of 3 channels, device data off a 4-byte boundary, degrees out of range. */
typedef struct eu_rgbe {
  const void *data;          /* width x height quads R G B E, rows dense; cubemaps: the six faces stacked */
  int32_t on_device;         /* `data` is memory of the library's device */
  const float *colour_table; /* host, 65536 floats indexed (E << 8) | mantissa: the float a channel becomes; NULL: mantissa * 2^(E-136), E == 0 -> 0 */
} eu_rgbe;
int  eu_hip_source_load_rgbe(const eu_facet *fct, const eu_rgbe *px, const eu_facet_edit *edit, int spline_degree,
                             int prefilter_degree, int support_min, int tile_size, eu_source **out);
/* The same container from the planes of a Y'CbCr frame, as video decoders hand it out: planar (I420, I422, I444)
 * or with interleaved chroma (NV12, P010; NV21 with cb == cr + 1 sample), 8-bit or 16-bit samples. The planes go to
 * the device as their rows lie (a 2-D copy per plane) or are read where they lie there, and become floats
 * (eu_ycbcr.hip) on the way into the container. With Y = y_table[y], U = c_table[cb], V = c_table[cr], every product
 * and every sum a float32 operation rounded on its own (include/eu_ycbcr.h):
 *   R = Y + m_rv * V        G = (Y + m_gu * U) + m_gv * V        B = Y + m_bu * U
 * Chroma is replicated, not interpolated. The container is bit for bit the one eu_hip_source_load[_edited] builds
 * from eu_hip_ycbcr_floats' output with the same edit (edit == NULL: none; edit->pixel_channels and
 * edit->pixels_on_device are ignored in favour of px). fct->nchannels is 3, or 4: the facet gains alpha = 1.0f here.
 * The frame has fct->window_width x window_height pixels; cubemaps: width x 6 width, the stack of faces as one image.
 * Argument errors (EU_ERR_ARGUMENT) are reported before a device is looked for: null planes or tables, bits other
 * than 8 or 16, c_step, sub_x or sub_y outside {1, 2}, pitches shorter than a row, 16-bit planes or pitches at odd
 * addresses, nchannels other than 3 or 4, masks or a crop on a facet of 3 channels, degrees out of range. */
typedef struct eu_ycbcr {
  const void *y, *cb, *cr;      /* first sample of each plane                                        */
  size_t y_pitch, c_pitch;      /* BYTES between rows of the luma plane / of both chroma planes       */
  int32_t c_step;               /* samples from one chroma sample to the next in a row: 1 planar
                                   (I420, I422, I444), 2 interleaved (NV12: cr == cb + 1 sample)      */
  int32_t sub_x, sub_y;         /* 1 or 2 each: pixel (x, y) takes chroma sample (x / sub_x, y / sub_y);
                                   the chroma planes hold ceil(w / sub_x) x ceil(h / sub_y) samples   */
  int32_t bits;                 /* 8: uint8_t, 16: uint16_t in host order                            */
  int32_t on_device;            /* all three planes are memory of the library's device               */
  const float *y_table, *c_table; /* host, 1 << bits floats each: the float a luma / chroma sample
                                   becomes - range, depth, bit alignment (P010) and the chroma offset
                                   are the tables' business, the library knows none of them          */
  float m_rv, m_gu, m_gv, m_bu; /* the matrix                                                         */
} eu_ycbcr;
int  eu_hip_source_load_ycbcr(const eu_facet *fct, const eu_ycbcr *px, const eu_facet_edit *edit,
                              int spline_degree, int prefilter_degree, int support_min, int tile_size,
                              eu_source **out);
/* HOST function, no device needed: the floats of a width x height frame of host planes, dense rows of nchannels
 * (3, or 4 with alpha 1.0f) floats - the definition of what eu_hip_source_load_ycbcr loads. px->on_device must be 0. */
int  eu_hip_ycbcr_floats(const eu_ycbcr *px, int width, int height, int nchannels, float *out);
/* Adopt an already prefiltered and braced container (host pointer, shape as
 * eu_hip_container_geometry reports; cubemaps: the IR image section_px x
 * 6*section_px). This is what a bound reference hands over when it keeps its
 * own set-up stage. */
int  eu_hip_source_adopt(const eu_facet *fct, const float *container,
                         int spline_degree, int bc0, int bc1,
                         int support_min, int tile_size, eu_source **out);
/* Allocate the container for a facet without filling it, and expose its device
 * address: the multi-GPU host broadcasts rank 0's prefiltered coefficients
 * straight into it over RCCL/xGMI - one broadcast per source,
 * after which the source stays resident like any other. */
int  eu_hip_source_alloc(const eu_facet *fct, int spline_degree,
                         int support_min, int tile_size, eu_source **out);
/* The asset_handler caches the b-spline only; the facet's geometry (yaw / pitch / roll,
 * hfov, window offsets, lens a/b/c/h/v, shear, brighten, step) is read fresh from facet_spec
 * on every job (environment.h:84-227). A host that keeps sources resident calls this before a
 * job whose facet_spec changed: the evaluator and mount parameters are rebuilt from `fct`, the
 * coefficients stay. The image itself (projection, size, channels) must be the resident one. */
int  eu_hip_source_update_facet(eu_source *src, const eu_facet *fct);
int  eu_hip_source_device_ptr(const eu_source *src, void **dev_ptr,
                              size_t *nfloats);
/* copy the device-resident container back (tests, checkpointing) */
int  eu_hip_source_download(const eu_source *src, float *container,
                            size_t nfloats);
int  eu_hip_source_info(const eu_source *src, eu_container *geom, int *nch);
int  eu_hip_source_release(eu_source *src);
/* New pixels into a resident container: the second half of a load, without its first. After the call, in stream
 * order behind it, the container of `src` is bit for bit the one the matching eu_hip_source_load* call builds from
 * the same pixels for src's facet, degree, support_min and tile_size - core, frame, brace, a cubemap's support frame,
 * zero slack behind it - whatever stood there before. Geometry, degree, boundary conditions, cube metrics and the
 * device address stay. Nothing is allocated once the library's reload scratch has reached the feed's size, nothing
 * is freed, and tables that repeat from call to call are not uploaded again.
 * `stream` is a hipStream_t (NULL: the library's own); all device work of the call is queued on it, behind every
 * render that still reads the container on any stream and behind the library's own stream; every later render of
 * `src`, on any stream, goes behind the reload. With pixel data on the device and no masks or crop the call does not
 * wait for the device; with host data or an edit it may block as the loads do - rely on neither: eu_hip_sync(), or
 * synchronising `stream`, says the container is ready. Copies of `src` on other device slots are waited for and
 * freed; eu_hip_render_devices makes them again on first use.
 * Refused before a device is looked for, with a message that names the field: a null or replica handle
 * (EU_ERR_HANDLE), an unknown kind, a missing feed struct, whatever the matching load call refuses, pixels whose
 * channel count the facet cannot take (EU_ERR_ARGUMENT). A reload that fails on the device leaves the handle valid
 * and the container's content unspecified. */
enum { EU_PX_FLOATS = 0, EU_PX_SAMPLES = 1, EU_PX_RGBE = 2, EU_PX_YCBCR = 3 };
typedef struct eu_pixels {
  int32_t kind;                 /* EU_PX_* */
  const void *floats;           /* EU_PX_FLOATS: as eu_hip_source_load[_edited] takes them      */
  int32_t pixel_channels;       /* EU_PX_FLOATS: the facet's nchannels or one less              */
  int32_t on_device;            /* EU_PX_FLOATS: `floats` is memory of the library's device     */
  const eu_samples *samples;    /* EU_PX_SAMPLES */
  const eu_rgbe *rgbe;          /* EU_PX_RGBE    */
  const eu_ycbcr *ycbcr;        /* EU_PX_YCBCR   */
  const eu_facet_edit *edit;    /* masks / crop, or NULL; same rules as the matching load call  */
} eu_pixels;
int  eu_hip_source_reload(eu_source *src, const eu_pixels *px, int prefilter_degree, void *stream);
/* waits for every reload so far and frees the scratch they share ("A source refilled in place") */
int  eu_hip_reload_scratch_release(void);

/* ---- feathering to alpha edges: a distance plane per source ------------------------------------------------
 * eu_hip_source_load_pixels is the load eu_hip_source_reload is the second half of: one call for every feed, through
 * eu_pixels. flags == 0 builds, bit for bit, what the matching eu_hip_source_load* call builds (EU_PX_FLOATS:
 * eu_hip_source_load_edited with px->edit, px->pixel_channels and px->on_device in the edit's place) and refuses what
 * that call refuses. EU_LOAD_EDGES also keeps the distance plane D of the facet's window, 4 bytes per window pixel
 * (a quarter on top of an RGBA container's core), which the feathered synopses (EU_SYN_FEATHER, EU_SYN_MULTIBAND)
 * then take into the blend weight: the ramp falls towards mask, crop and alpha edges too, not only towards the window.
 * The definition, for a source of 2 or 4 channels that is no cubemap, window w x h, both at most 32768:
 *   Outside set  O = { (u, v) : not (alpha(u, v) > 0) }, alpha the last channel of the plane the prefilter reads -
 *                behind the decode, a gained channel, the edit and its binomial. An IEEE compare: NaN, negative values
 *                and both zeros are outside, a positive denormal is inside.
 *   Row distance g(x, y) = the smallest |x - u| over (u, y) in O; where the load chose the periodic boundary condition
 *                for axis 0 (a 360-degree spherical or cylindrical source) the smallest min(|x - u|, w - |x - u|).
 *                A row without an outside pixel has none.
 *   D2(x, y)     = the smallest g(x, v)^2 + (y - v)^2 over the rows v that have a g(x, v), an exact int32
 *                (2 * 32767^2 < 2^31); 2^31 - 1 if no row has one. Rows never wrap: the distance does not cross
 *                the pole of a full sphere.
 *   D(x, y)      = sqrt(float(D2)): int32 to float32 rounded to nearest, then a correctly rounded float32 root.
 *   Sampling, per facet the ray hits, float32, every operation rounded on its own, no contraction:
 *                ix = floor(sx), fx = sx - float(ix), iy and fy likewise; ix and ix + 1 wrap modulo w where the rows
 *                are periodic and clamp to [0, w - 1] otherwise, iy and iy + 1 clamp;
 *                top = D00 + (D10 - D00) * fx, bot = D01 + (D11 - D01) * fx, dm = (top + (bot - top) * fy) - 0.5f
 *                (D10: column ix + 1, row iy). The - 0.5 measures to the outside pixel's edge, as the window ramp
 *                measures to the border at -0.5.
 *   Weight       d = the smaller of dm and the window ramp's d (eu_target::feather), dm alone where no axis has a
 *                border; e = clamp(d * float(1.0 / width), 2^-16, 1). Everything behind e is eu_target::feather's and
 *                eu_target::bands' definition, unchanged - a pixel ONE facet hits is still that facet's pixel as it is.
 * A facet without a plane is weighted as before, also beside facets that have one; jobs in which no facet has a plane
 * run the kernels they ran before. Out of scope: cubemap sources, per-facet widths, a metric in ray space.
 * Refused with EU_ERR_ARGUMENT before a device is looked for: an unknown flag bit; EU_LOAD_EDGES on a cubemap, on a
 * facet whose nchannels is not 2 or 4, on a window side above 32768.
 * eu_hip_source_reload of a source with a plane refills the plane too, in the same stream order, at the same device
 * address; eu_hip_source_release frees it; the copies eu_hip_render_devices makes carry it. eu_hip_source_adopt and
 * eu_hip_source_alloc make sources without a plane. */
enum { EU_LOAD_EDGES = 1 };
int  eu_hip_source_load_pixels(const eu_facet *fct, const eu_pixels *px, int spline_degree, int prefilter_degree,
                               int support_min, int tile_size, unsigned flags, eu_source **out);
/* D of a source loaded with EU_LOAD_EDGES: window_height rows of window_width floats into `out`, rows
 * row_stride_bytes apart (a multiple of 4, at least a row); out_on_device != 0: `out` is device memory and the copy is
 * queued on `stream` (NULL: the library's own) behind the load or reload that wrote the plane; else the call returns
 * when `out` is complete. EU_ERR_ARGUMENT for a source without a plane. */
int  eu_hip_source_edge_distance(const eu_source *src, float *out, size_t row_stride_bytes, int out_on_device,
                                 void *stream);
/* 1: the source keeps a distance plane, 0: it does not (also for a null handle) */
int  eu_hip_source_has_edges(const eu_source *src);
/* the plane where it lies on the device, as eu_hip_source_device_ptr gives the container: window_width x
 * window_height floats, dense; it stays there for the source's life, reloads included. NULL without a plane. */
int  eu_hip_source_edge_device_ptr(const eu_source *src, void **dev_ptr);

/* ---- the hot path --------------------------------------------------------- */
/* zimt::process(shape, stepper, environment|twine_t, storer): renders rows
 * [row_begin,row_end) of the target into `out` (row stride in bytes).
 * out_on_device != 0: `out` is a device pointer, the call is asynchronous on
 * `stream` (a hipStream_t, NULL = the library's own stream) until
 * eu_hip_sync(); otherwise `out` is host memory and the call returns when the
 * rows are there. With trg->out_format == EU_OUT_SRGBA8 `out` points to uint32
 * words (one per pixel, cast the pointer); with a crop window the rows are
 * crop_w pixels wide. */
int  eu_hip_render(const eu_target *trg, eu_source *const *srcs, int nsrc,
                   float *out, size_t out_row_stride_bytes, int out_on_device,
                   void *stream);
int  eu_hip_sync(void);

/* Time the render kernel alone with HIP events on its own stream: runs the
 * launch `iters` times back to back, returns the mean kernel duration. */
int  eu_hip_render_timed(const eu_target *trg, eu_source *const *srcs, int nsrc,
                         float *out_dev, size_t out_row_stride_bytes,
                         int iters, float *mean_ms);

/* ---- `act` alone: a resident source at the caller's rays -------------------- */
/* The reference's pipeline is get (a stepper), act (environment, inside twine_t when twining) and put.
 * eu_hip_render is all three; this entry is act + put on rays the CALLER supplies: a viewer with a projection
 * the library has no stepper for, a remap from a precomputed ray map, an environment lookup at an array of
 * directions.
 *
 * Rays are what `act` sees: three floats x, y, z (RIGHT, DOWN, FORWARD) in the SOURCE's frame - exactly what
 * eu_target.stage = 1 writes. In the reference the facet's orientation is folded into the stepper's basis, so
 * this path applies NEITHER the facet's yaw / pitch / roll NOR any camera orientation: a caller who wants them
 * rotates the rays. Rays need not be normalised; they are used as given.
 *
 * ninputs = 9: every element is a ninepack {ray, x-neighbour, y-neighbour} as twine_t::eval reads it
 * (twining.h:128-263, differencing branch; eu_target.stage = 1, 3, 4 write the three parts for a job):
 * dx = in[3..5] - in[0..2], dy = in[6..8] - in[0..2], out = sum over the taps, in order, of
 * w * inner(ray + 4x * dx + 4y * dy). `taps` is make_spread's output ({x, y, weight} per tap, host memory).
 *
 * Arithmetic: the device functions of the render kernels in their order - the rays of a job give that job's
 * frame bit for bit. One documented difference from the reference, because a caller's array holds arbitrary
 * bit patterns: a ray with a non-finite component, or with all three components zero, is a MISS - zeros in
 * every channel - and so is a ninepack with a non-finite float among its nine or a null centre ray
 * (eu_ray_guard.h; no other ray can make a read leave the container).
 *
 * The array is a width x height grid (a flat list: height = 1); row strides count bytes, are multiples of 4 and
 * may exceed the rows. One source, float output. `rays` and `out` may each lie in host or in device memory:
 * with both on the device the call is asynchronous on `stream` (NULL: the library's) until eu_hip_sync();
 * otherwise the grid is staged in bounded chunks and the call returns when `out` is complete. Argument errors
 * (EU_ERR_ARGUMENT) are reported before a device is looked for. eu_hip_render, its plan caches and
 * eu_hip_launch_count() are not touched. */
typedef struct eu_rays {
  int32_t width, height;            /* rays per row, rows                                   */
  int32_t ninputs;                  /* 3: rays; 9: ninepacks (twine_t)                      */
  int32_t nchannels;                /* output channels 1..4 (repix_t as eu_target.nchannels)*/
  int32_t ntaps; const float *taps; /* ninputs 9: make_spread output, host, <= EU_MAX_TAPS  */
  const float *rays; size_t ray_row_stride_bytes; int32_t rays_on_device;
} eu_rays;
int  eu_hip_render_rays(const eu_rays *r, eu_source *src, float *out,
                        size_t out_row_stride_bytes, int out_on_device, void *stream);
/* the kernel alone, `iters` launches back to back on the library's stream (rays and output in device memory) */
int  eu_hip_render_rays_timed(const eu_rays *r, eu_source *src, float *out_dev,
                              size_t out_row_stride_bytes, int iters, float *mean_ms);

/* Many views of one resident source in one call: the jobs of a tethered viewer or a pipe-mode loop, which differ
 * only in yaw, pitch, roll and hfov (envutil_main.cc:1755-1869), a camera path, a batch of crops from one panorama.
 * `trg` supplies what all views share - projection, width, height, nchannels, the tap table; its own orientation
 * and extent are ignored. View k is written at out + k * out_view_stride_bytes, rows out_row_stride_bytes apart,
 * and is bit for bit the frame eu_hip_render gives for `trg` with that view's orientation and extent. The stepper
 * tables of every view are made on the device from a few scalars per view (eu_render_views.hip), so the host does
 * per view neither libm work nor an upload nor a synchronisation; tables of at most EU_HIP_VIEWS_MAX_KB KiB are
 * kept at a time (a longer sequence, or one of more than 65535 views, goes through in chunks of views).
 *
 * One source, float output, whole frames. EU_ERR_ARGUMENT, before a device is looked for: null pointers,
 * nviews < 0, a non-finite field of a view, stage != 0, a crop window, row bands, single != NULL, EU_OUT_SRGBA8,
 * row_begin / row_end other than the whole frame, strides that are no multiples of 4, a row stride smaller than a
 * row, a view stride smaller than `height` rows. EU_ERR_UNSUPPORTED: a facet with PTO translation, a target
 * projection without a stepper, a biatan6 target whose in-face coordinates leave [-1.75, 1.75]. nviews == 0 is
 * EU_OK and writes nothing.
 *
 * With `out` on the device the call is asynchronous on `stream` (NULL: the library's) until eu_hip_sync();
 * otherwise the views are staged through a bounded device buffer and the call returns when `out` is complete.
 * The call uses buffers of its own: eu_hip_render, its plan caches, eu_hip_launch_count() and the staged kernels'
 * work list are not touched. */
typedef struct eu_view {
  double yaw, pitch, roll;      /* camera orientation, radians (as eu_target)            */
  double x0, x1, y0, y1;        /* extent of this view (get_extent of its hfov)          */
} eu_view;
int  eu_hip_render_views(const eu_target *trg, const eu_view *views, int nviews, eu_source *src, float *out,
                         size_t out_row_stride_bytes, size_t out_view_stride_bytes, int out_on_device, void *stream);
/* The same for a multi-facet job: view k is bit for bit the frame eu_hip_render(trg', srcs, nsrc, ...) gives, trg'
 * being `trg` with view k's orientation and extent; trg->synopsis selects panorama (voronoi_syn / voronoi_syn_plus),
 * hdr_merge or feather as there. Layout, strides, `out_on_device` and `stream` are those of eu_hip_render_views. nsrc == 1
 * forwards to eu_hip_render_views. Per (view, facet) the host computes one block of scalars - the basis
 * rotate(r_cam(view), r_fct(facet)) - and nothing else; the facets' parameters and the tap table go up once per
 * call. A view's tables take nsrc * (6 * width + 24 * height) * 4 bytes of the EU_HIP_VIEWS_MAX_KB bound.
 *
 * EU_ERR_ARGUMENT, before a device is looked for: everything eu_hip_render_views refuses (the --mask_for channel
 * rule per facet), nsrc < 1 or > 65535, srcs == NULL, facets that do not share the spline degree. A null entry of
 * srcs is EU_ERR_HANDLE. EU_ERR_UNSUPPORTED: any facet with PTO translation, a target projection without a
 * stepper, the biatan6 range of a view. nviews == 0 is EU_OK and writes nothing.
 *
 * The call uses the buffers of eu_hip_render_views and one more of its own: eu_hip_render's multi-facet tables and
 * plan key, eu_hip_launch_count() and the work list are not touched. EU_HIP_REJ has no effect here. */
int  eu_hip_render_views_multi(const eu_target *trg, const eu_view *views, int nviews, eu_source *const *srcs, int nsrc,
                               float *out, size_t out_row_stride_bytes, size_t out_view_stride_bytes, int out_on_device,
                               void *stream);
/* For tests. All four are host buffers of 6 * width and height * 24 floats (the column table [6][width], the row
 * table [height][24]): the first two receive what the table kernel wrote for this view, the last two what the host
 * function behind eu_hip_render builds for it. */
int  eu_hip_view_tables(const eu_target *trg, const eu_view *view, eu_source *src, float *col_dev_built,
                        float *row_dev_built, float *col_host_built, float *row_host_built);

/* ---- many pictures of one geometry -------------------------------------------- */
/* The other axis of batching: ONE camera, many pictures that share projection, size, field of view, orientation and
 * lens - the eyes of a stereo pair, the exposures of a bracket, the passes of a rendered panorama, frames of a
 * video. Layer k is written at out + k * out_layer_stride_bytes, rows out_row_stride_bytes apart, and is bit for
 * bit the frame eu_hip_render(trg, &layers[k], 1, ...) gives (NaN payloads apart, as everywhere). What does not
 * depend on the picture - ray, source coordinate, gate, split, weights, per tap for a twined job - is computed once
 * per pixel; per layer only the taps, the weighted sum and the store are new work (eu_render_layers.hip).
 *
 * `trg` is whatever a single-facet eu_hip_render job may be with float output and whole frames: its own orientation
 * and extent, a tap table, nchannels different from the layers'. The layers must agree in everything the kernels
 * compute coordinates, gates and weights from: the device parameter block of layer k equals layer 0's byte for
 * byte apart from the container's address and `brighten` (which may differ per layer: a bracket).
 *
 * EU_ERR_ARGUMENT, before a device is looked for: null pointers, nlayers < 0, stage != 0, a crop window, row bands,
 * row_begin / row_end other than the whole frame, single != NULL, EU_OUT_SRGBA8, a --mask_for source, strides that
 * are no multiples of 4, a row stride smaller than a row, a layer stride smaller than `height` rows, layers that
 * do not agree (the message names the first differing layer). A null entry of `layers` is EU_ERR_HANDLE.
 * EU_ERR_UNSUPPORTED: a facet with PTO translation or a target that needs the generic stepper, a target projection
 * without a stepper. nlayers == 0 is EU_OK and writes nothing.
 *
 * With `out` on the device the call is asynchronous on `stream` (NULL: the library's) until eu_hip_sync();
 * otherwise the layers are staged through at most 64 MiB of device memory and the call returns when `out` is
 * complete. At most EU_HIP_LAYERS_MAX layers are walked by one launch (default 4; 0: all); a longer list goes through
 * in chunks in stream order. The call uses buffers of its own: eu_hip_render, its plan caches,
 * eu_hip_launch_count() and the staged kernels' work list are not touched. */
int  eu_hip_render_layers(const eu_target *trg, eu_source *const *layers, int nlayers, float *out,
                          size_t out_row_stride_bytes, size_t out_layer_stride_bytes, int out_on_device, void *stream);
/* For tests and tools: how many layers the twined kernels of this build take through one tap loop (EU_LAYERS_GROUP). */
int  eu_hip_layers_group(void);

/* ---- the way out as integer samples ------------------------------------------ */
/* Float pixels to 8- or 16-bit samples ON THE DEVICE (eu_encode.hip), the mirror of eu_hip_source_load_samples: a
 * frame leaves as a quarter or half of its float bytes, and the host does no per-sample work. The library knows
 * no colour spaces and no maxval; a TABLE says it all. With steps = colour_steps, or alpha_steps for the last
 * channel of 2 or 4:
 *   code(v) = the number of k in 1 .. (1 << bits) - 1 with v >= steps[k]            (steps[0] is ignored)
 * A valid table has steps[1 .. m] free of NaN and non-decreasing, m >= 1, and NaN in every entry behind m: codes
 * above a file's maxval = m are then never produced. Equal neighbours are allowed (a code is skipped). A NaN pixel
 * fails every compare and is code 0; +inf is code m. Because the code a float becomes by clamp / scale / round
 * behind a transfer curve is a non-decreasing step function of the float, a host finds steps[k] - the smallest
 * float whose code is >= k - by bisection over the very expression its float route applies
 * (include/eu_image_io.hpp: encode_steps), and the device's samples are that route's, bit for bit. */
typedef struct eu_encode {
  int32_t bits;              /* 8: uint8_t, 16: uint16_t */
  int32_t big_endian;        /* bits 16: high byte first, as PNM / PAM store it; 0: host order */
  const float *colour_steps; /* host, 1 << bits floats */
  const float *alpha_steps;  /* host, 1 << bits floats: the LAST channel of 2 or 4; NULL: colour_steps for it too */
} eu_encode;
/* Any float frame of width x height pixels of nchannels floats, rows frame_row_stride_bytes apart: host memory
 * (staged to the device in bounded chunks) or, with frame_on_device, device memory read where it lies - the output
 * of eu_hip_render or eu_hip_render_rays, the N * H rows of an eu_hip_render_views result. `out` receives width *
 * nchannels samples per row, rows out_row_stride_bytes apart; rows start at any byte (bits 16: any even byte), and
 * no byte outside the samples of a row is written. With frame and `out` both on the device the call is asynchronous
 * on `stream` (NULL: the library's) until eu_hip_sync(); otherwise it returns when `out` is complete. The tables go
 * up in front of the kernel into a buffer of the call's own; the library orders the upload behind the calls that
 * used it before, on whatever stream. EU_ERR_ARGUMENT, before a device is looked for: null pointers, bits other than 8
 * or 16, nchannels outside 1..4, negative sizes, a stride smaller than a row, float strides that are no multiple of
 * 4, a 16-bit `out` or stride at an odd byte, an invalid table. width == 0 or height == 0 is EU_OK and writes
 * nothing. */
int  eu_hip_encode_samples(const float *frame, size_t frame_row_stride_bytes, int frame_on_device,
                           int width, int height, int nchannels, const eu_encode *enc,
                           void *out, size_t out_row_stride_bytes, int out_on_device, void *stream);
/* eu_hip_render with the encode behind it: every job eu_hip_render runs (single- and multi-facet, crops, row_begin /
 * row_end, bands), `out` receiving what eu_hip_encode_samples makes of that job's float frame, byte for byte. The
 * float frame goes to the library's frame buffer and never leaves the device; with a host `out` the pipeline of up
 * to four row chunks is eu_hip_render's, the encode running behind each chunk's render and the copy moving samples.
 * EU_ERR_ARGUMENT, before a device is looked for: what eu_hip_render and eu_hip_encode_samples refuse, stage != 0
 * and EU_OUT_SRGBA8. */
int  eu_hip_render_samples(const eu_target *trg, eu_source *const *srcs, int nsrc, const eu_encode *enc,
                           void *out, size_t out_row_stride_bytes, int out_on_device, void *stream);

/* ---- the way out as Radiance RGBE pixels --------------------------------------- */
/* Any float frame of width x height pixels of THREE floats to RGBE quads ON THE DEVICE (eu_rgbe.hip), the mirror of
 * eu_hip_source_load_rgbe: a frame leaves as a third of its float bytes, and the host does no per-pixel work. The
 * quad of a pixel is eu_rgbe_encode's (include/eu_rgbe.h), the function the file route calls on the host: defined for
 * every float, channels above 255 * 2^119 clamped to it. Frame, strides, `out_on_device` and `stream` as
 * eu_hip_encode_samples; `out` receives width quads per row, rows out_row_stride_bytes apart, and no byte outside the
 * quads of a row is written. There is no table, so nothing is uploaded and no buffer of the library's is read after a
 * call with both pointers on the device. EU_ERR_ARGUMENT, before a device is looked for: null pointers, negative sizes,
 * a stride smaller than a row, a frame or a float stride that is no multiple of 4, `out` or its stride off a 4-byte
 * boundary. width == 0 or height == 0 is EU_OK and writes nothing. */
int  eu_hip_encode_rgbe(const float *frame, size_t frame_row_stride_bytes, int frame_on_device, int width, int height,
                        void *out, size_t out_row_stride_bytes, int out_on_device, void *stream);
/* eu_hip_render with that encode behind it, as eu_hip_render_samples is built: every job eu_hip_render runs with a
 * 3-channel target (single- and multi-facet, crops, row_begin / row_end, bands), the float frame in the library's frame
 * buffer, the same pipeline of up to four row chunks for a host `out`. EU_ERR_ARGUMENT, before a device is looked
 * for: what eu_hip_render and eu_hip_encode_rgbe refuse, a target channel count other than 3, stage != 0 and
 * EU_OUT_SRGBA8. */
int  eu_hip_render_rgbe(const eu_target *trg, eu_source *const *srcs, int nsrc, void *out,
                        size_t out_row_stride_bytes, int out_on_device, void *stream);

/* ---- the way out as Y'CbCr planes ------------------------------------------------ */
/* Any float frame of 3 or 4 channels (alpha is ignored) to the planes of a Y'CbCr frame ON THE DEVICE
 * (eu_ycbcr_out.hip), the mirror of eu_hip_source_load_ycbcr: what a hardware encoder takes as its input surface -
 * planar (I420, I422, I444) or with interleaved chroma (NV12, NV21, P010). Every product and sum a float32 operation
 * rounded on its own (include/eu_ycbcr.h):
 *   Y = (k_r * R + k_g * G) + k_b * B        U = (B - Y) * c_u        V = (R - Y) * c_v
 * Chroma is a box mean over sub_x x sub_y pixels with the edge replicated at odd sizes (include/eu_ycbcr.h has the
 * order of the sums). Y goes through y_steps, the means of U and V through c_steps: tables of 1 << bits floats with
 * eu_encode's semantics and validity rules (above). The stored sample is the low `bits` bits of code << shift, in
 * host order. Range, depth and the chroma offset are the tables' business, the library knows none of them.
 * The layout is eu_ycbcr's: rows y_pitch / c_pitch BYTES apart; c_step 1 planar; c_step 2 interleaved, and then cr
 * is cb plus or minus exactly one sample. The chroma planes hold ceil(w / sub_x) x ceil(h / sub_y) samples. No byte
 * outside the samples of a row of a plane is written; in interleaved chroma both samples of a pair are the call's.
 * EU_ERR_ARGUMENT, before a device is looked for, each with a message of its own: null pointers, bits other than 8
 * or 16, shift outside 0 .. bits - 1, sub_x or sub_y outside {1, 2}, c_step outside {1, 2} or an interleaved pair
 * that is no pair, pitches shorter than a row, 16-bit planes or pitches at odd addresses, nchannels other than 3 or
 * 4, a frame or a float stride that is no multiple of 4, an invalid table. width == 0 or height == 0 is EU_OK and
 * writes nothing. */
typedef struct eu_ycbcr_out {
  void *y, *cb, *cr;            /* first sample of each plane                                              */
  size_t y_pitch, c_pitch;      /* BYTES between rows of the luma plane / of both chroma planes            */
  int32_t c_step;               /* 1 planar; 2 interleaved (NV12: cr == cb + 1 sample, NV21: cb == cr + 1) */
  int32_t sub_x, sub_y;         /* 1 or 2 each                                                             */
  int32_t bits;                 /* 8: uint8_t, 16: uint16_t in host order                                  */
  int32_t shift;                /* 0 .. bits - 1: the sample is code << shift (P010: 6)                    */
  int32_t on_device;            /* all three planes are memory of the library's device                     */
  const float *y_steps, *c_steps; /* host, 1 << bits floats each                                           */
  float k_r, k_g, k_b, c_u, c_v;  /* the forward coefficients                                              */
} eu_ycbcr_out;
/* Frame, strides, frame_on_device and `stream` as eu_hip_encode_samples. With frame and planes on the device the call
 * is asynchronous on `stream` (NULL: the library's) until eu_hip_sync(); a host buffer on either side goes through
 * bounded chunks of that call's staging buffers - whole chroma rows each - and the call returns when the planes are
 * complete. */
int  eu_hip_encode_ycbcr(const float *frame, size_t frame_row_stride_bytes, int frame_on_device, int width, int height,
                         int nchannels, const eu_ycbcr_out *dst, void *stream);
/* eu_hip_render with that encode behind it, as eu_hip_render_samples is built: every job eu_hip_render runs with a 3-
 * or 4-channel target, the float frame in the library's frame buffer, the same pipeline of up to four row chunks for
 * host planes. The planes are those of the rows row_begin .. row_end taken as an image of its own. EU_ERR_ARGUMENT,
 * before a device is looked for: what eu_hip_render and eu_hip_encode_ycbcr refuse, stage != 0 and EU_OUT_SRGBA8. */
int  eu_hip_render_ycbcr(const eu_target *trg, eu_source *const *srcs, int nsrc, const eu_ycbcr_out *dst, void *stream);
/* HOST function, no device needed: the definition of the two calls above, one loop over eu_ycbcr.h's statement.
 * dst->on_device must be 0. */
int  eu_hip_ycbcr_planes(const float *frame, size_t frame_row_stride_bytes, int width, int height, int nchannels,
                         const eu_ycbcr_out *dst);

/* device memory helpers for hosts without a HIP binding of their own */
int  eu_hip_malloc(void **p, size_t bytes);
int  eu_hip_free(void *p);
int  eu_hip_memcpy_d2h(void *dst, const void *src, size_t bytes);
int  eu_hip_memcpy_h2d(void *dst, const void *src, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif
