// How a single-facet job finds its kernel, and the EU_HIP_* switches that can change the answer.
// Plain C++ (no HIP): the host glue (eu_api_*.hip) and the launchers include it, and so does a host test program
// (tests/csrc/select_demo.cc).
//
//   general          eu_render.hip    one pixel per lane, every job
//   general, direct  the same with the inline evaluation: --mask_for jobs paint the facet there
//   packed           eu_render2.hip   two pixels per lane, direct gathers (eu_packed_covers)
//   packed in runs   the same, one launch per run of rows that want the same work layout
//   staged           eu_render4.hip   LDS-staged tiles plus the direct-gather kernel behind them
//                                     (eu_staged_covers), two launches
// A call with the caller's own rays (eu_hip_render_rays) has two forms of its own: eu_select_ray_path().
// So has a sequence of views (eu_hip_render_views): eu_select_view_path(), and a set of pictures of one geometry
// (eu_hip_render_layers): eu_select_layer_path().
#ifndef EU_SELECT_H
#define EU_SELECT_H
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <vector>
#include "eu_device.h"
#include "eu_share_groups.h"
#include "eu_worklist.h"

// ---- the switches ------------------------------------------------------------------------------
// One field per EU_HIP_* variable the library reads. eu_read_switches() is the only reader: every
// entry point calls it once and hands the result down, so all of them are read on every call.
struct eu_switches {
  int force_general;   // EU_HIP_KERNEL=1: the general kernel for every job (A/B switch)
  int hybrid;          // EU_HIP_HYBRID: 0 never split a frame into runs, 2 split wherever the layouts differ (tests); else 1
  int r4;              // EU_HIP_R4: 0 never the staged kernels, 1 wherever they apply (tests, A/B runs); unset: -1
  int colmajor;        // EU_HIP_COLMAJOR: 0 / non-zero forces the packed kernel's walk; unset or empty: -1
  int rej;             // EU_HIP_REJ: 1 the early-miss tables of a multi-facet job, 2 their table-free form; else 0
  int colplan;         // EU_HIP_COLPLAN=0: no column plans (0); else 1
  int share;           // EU_HIP_SHARE: EU_SHARE_* bits - 0: none, m: mirrors, f: faces; else both
  int polar_share;     // EU_HIP_POLAR_SHARE: EU_POLAR_* bits, the second loop's groups (with the box table) - 0: none, t: twins,
                       // m: mirrors; else both
  int direct;          // EU_HIP_DIRECT=1: the general kernel never stages through LDS
  int iir_stream;      // EU_HIP_IIR_STREAM: bit 0 rows, bit 1 columns, bit 2 checkpoints; unset: 7
  int boxtab;          // EU_HIP_BOXTAB=0: the persistent staged kernel's second loop reduces its tile boxes per frame (0); else 1:
                       // it reads them from a table built with the plans
  int boxtab_max_kb;   // EU_HIP_BOXTAB_MAX_KB: the largest box table built, KiB (EU_BOXTAB_MAX_KB); a job beyond it gets none
  int views_max_kb;    // EU_HIP_VIEWS_MAX_KB: the most stepper tables eu_hip_render_views keeps at a time, KiB
                       // (EU_VIEWS_MAX_KB); a longer sequence goes through in chunks of views
  int layers_max;      // EU_HIP_LAYERS_MAX: the most layers one launch of eu_hip_render_layers walks (EU_LAYERS_MAX); 0 or
                       // negative: 0, all of them. A longer list goes through in chunks, in stream order
};

// 64 bytes per second-loop tile: 64 MiB hold the polar faces of a 6 x 8192 cubemap, four times the headline's 16 MiB
#define EU_BOXTAB_MAX_KB 65536
// 120 KiB per 1024 x 1024 view: 64 MiB hold the tables of 546 of them
#define EU_VIEWS_MAX_KB 65536
// measured ("Many pictures of one geometry"): of 1, 2, 4 and all at eight layers, four is the fastest or
// within 6 % of the fastest on every job timed; all of them cost the big cubemap jobs 3 to 8 %
#define EU_LAYERS_MAX 4

inline eu_switches eu_read_switches()
{
  auto first = [](const char *name) { const char *e = getenv(name); return e ? e[0] : '\0'; };
  eu_switches s;
  s.force_general = first("EU_HIP_KERNEL") == '1';
  const char hy = first("EU_HIP_HYBRID");
  s.hybrid = hy == '0' ? 0 : hy == '2' ? 2 : 1;
  const char *r4 = getenv("EU_HIP_R4");
  s.r4 = r4 ? atoi(r4) : -1;
  const char *cm = getenv("EU_HIP_COLMAJOR");
  s.colmajor = cm && cm[0] ? atoi(cm) : -1;
  const char rj = first("EU_HIP_REJ");
  s.rej = rj == '1' ? 1 : rj == '2' ? 2 : 0;
  s.colplan = first("EU_HIP_COLPLAN") != '0';
  const char sh = first("EU_HIP_SHARE");
  s.share = sh == '0' ? 0 : sh == 'm' ? EU_SHARE_MIRRORS : sh == 'f' ? EU_SHARE_FACES : EU_SHARE_FACES | EU_SHARE_MIRRORS;
  const char ps = first("EU_HIP_POLAR_SHARE");
  s.polar_share = ps == '0' ? 0 : ps == 't' ? EU_POLAR_TWINS : ps == 'm' ? EU_POLAR_MIRRORS : EU_POLAR_TWINS | EU_POLAR_MIRRORS;
  s.direct = first("EU_HIP_DIRECT") == '1';
  const char *iir = getenv("EU_HIP_IIR_STREAM");
  s.iir_stream = iir ? atoi(iir) : 7;
  s.boxtab = first("EU_HIP_BOXTAB") != '0';
  const char *bm = getenv("EU_HIP_BOXTAB_MAX_KB");
  s.boxtab_max_kb = bm && bm[0] ? std::max(0, std::min(atoi(bm), 16 * 1024 * 1024)) : EU_BOXTAB_MAX_KB;
  const char *vm = getenv("EU_HIP_VIEWS_MAX_KB");
  s.views_max_kb = vm && vm[0] ? std::max(0, std::min(atoi(vm), 16 * 1024 * 1024)) : EU_VIEWS_MAX_KB;
  const char *lm = getenv("EU_HIP_LAYERS_MAX");
  s.layers_max = lm && lm[0] ? std::max(0, atoi(lm)) : EU_LAYERS_MAX;
  return s;
}

// ---- coverage ----------------------------------------------------------------------------------
inline bool eu_cube_source(int prj) { return prj == EU_CUBEMAP || prj == EU_BIATAN6; }

// the packed two-pixel kernels (eu_render2.hip): table-driven forms on lat/lon and cube sources
// ... what they ask of the source and the channel counts: a lat/lon or cube source without lens polynomial,
// degrees 1-3, dense texels, no channel adaption
inline bool eu_packed_covers_source(const eu_src_dev &s, int nch, int nch_out)
{
  if (s.has_lcp || nch_out != nch) return false;
  if (s.prj != EU_SPHERICAL && !eu_cube_source(s.prj)) return false;
  if (s.degree < 1 || s.degree > 3 || s.es0 != nch) return false;
  return nch >= 1 && nch <= 4;
}
inline bool eu_packed_covers(const eu_render_params &p)
{
  if (p.stage != 0 || p.form >= EU_FORM_FISH) return false;
  return eu_packed_covers_source(p.src, p.nch, p.nch_out);
}

// the staged kernels (eu_render4.hip): 16x8 wave tiles, at most 65535 * 8 units of 4 tile rows, and no more
// tiles in a launch than the work list has ids for (eu_worklist.h: a tile id is an int)
#define EU_STAGED_TILE_ROWS 8
#define EU_STAGED_TILE_COLS 16
#define EU_STAGED_MAX_TILES_Y (65535 * 8 * 4)
// wave tiles of a launch over rows [row_begin, row_end) of a frame `width` pixels wide
inline unsigned long long eu_staged_tiles(int width, int row_begin, int row_end)
{
  const long long tx = ((long long)width + EU_STAGED_TILE_COLS - 1) / EU_STAGED_TILE_COLS;
  const long long ty = ((long long)row_end - row_begin + EU_STAGED_TILE_ROWS - 1) / EU_STAGED_TILE_ROWS;
  return tx > 0 && ty > 0 ? (unsigned long long)tx * (unsigned long long)ty : 0ull;
}
inline bool eu_staged_covers(const eu_render_params &p)
{
  if (!eu_packed_covers(p) || p.twine) return false;
  if (p.norm_mode != EU_NORM_NONE && p.norm_mode != EU_NORM_DIV) return false;
  if (p.nch != 3 && p.nch != 4) return false;
  if (p.src.es1 * 4 >= (1ll << 31)) return false;            // the staging offsets are 32-bit
  if ((p.row_end - p.row_begin + EU_STAGED_TILE_ROWS - 1) / EU_STAGED_TILE_ROWS > EU_STAGED_MAX_TILES_Y) return false;
  return eu_staged_tiles(p.width, p.row_begin, p.row_end) <= EU4_WL_MAX_TILES;
}

// 'ray = B * c0 + A' without normalisation over the whole frame, on a source every finite ray hits
inline bool eu_plain_ba(const eu_render_params &p)
{
  return p.form == EU_FORM_BA && p.norm_mode == EU_NORM_NONE && p.band_count <= 1 && p.src.brighten == 1.0f &&
         p.src.always_hit;
}

// lat/lon jobs that go to the staged kernels without being asked to: cubic / quadratic jobs whose target
// can have column plans (an upright cubemap or rectilinear target)
inline bool eu_staged_default(const eu_render_params &p)
{
  return p.src.prj == EU_SPHERICAL && p.src.degree >= 2 && !p.twine && eu_plain_ba(p);
}

// the FAST form of the persistent staged kernel (eu_render5.h), for a lat/lon job eu_staged_covers():
// eu_div2_rr's range - the divisor in [2^-20, 2^20], the extent's origin 0 or in that range (so that a
// non-zero difference 'angle - origin' is at least 2^-73) - and finite stepper tables
inline bool eu_staged_fast_profile(const eu_render_params &p)
{
  auto mag_ok = [](double v) { const double a = v < 0 ? -v : v; return a == 0.0 || (a >= 0x1p-20 && a <= 0x1p20); };
  return eu_plain_ba(p) && mag_ok(p.src.tex_x0) && mag_ok(p.src.tex_y0) && p.src.ext_w >= 0x1p-20f &&
         p.src.ext_w <= 0x1p20f && p.src.ext_h >= 0x1p-20f && p.src.ext_h <= 0x1p20f && p.tab_finite;
}

// Known only once the column plans of a lat/lon job exist: the staged kernels measured faster than the
// direct-gather ones for cubic / quadratic jobs with column plans on at least half of the tile rows
// (DESIGN.md 5). Not asked under EU_HIP_R4=1, nor for cube sources.
inline bool eu_staged_worth(int degree, int planned_rows, int tiles_y)
{
  return degree >= 2 && planned_rows * 2 >= tiles_y;
}

// ---- the decision ------------------------------------------------------------------------------
enum eu_path { EU_PATH_GENERAL, EU_PATH_GENERAL_DIRECT, EU_PATH_PACKED, EU_PATH_PACKED_RUNS, EU_PATH_STAGED };

// staged_allowed = false: the answer for a job whose plan said no to eu_staged_worth().
// EU_PATH_PACKED_RUNS: the job is split where eu_split_runs() finds runs, and is one packed launch otherwise.
inline eu_path eu_select_path(const eu_render_params &p, const eu_switches &sw, bool staged_allowed = true)
{
  // a --mask_for job paints the facet at the inner evaluation: only the general kernel does that
  if (p.src.mask_paint) return EU_PATH_GENERAL_DIRECT;
  if (sw.force_general) return EU_PATH_GENERAL;
  // Measured: the staged kernels win where the taps dominate and the tile boxes are small - cubic /
  // quadratic jobs on cube sources (config 3: 1.13 -> 0.99 ms) and, in their persistent form, on lat/lon sources
  // whose target has column plans (the headline) - and lose to the direct-gather kernels on bilinear jobs
  const bool want_staged = sw.r4 == 1 || (sw.r4 != 0 && p.src.degree >= 2 && (eu_cube_source(p.src.prj) || eu_staged_default(p)));
  if (staged_allowed && want_staged && eu_staged_covers(p)) return EU_PATH_STAGED;
  if (!eu_packed_covers(p)) return EU_PATH_GENERAL;
  // the two work layouts of the packed kernel differ on lat/lon sources only, and a 0.2 ms bilinear job
  // has little to gain from more launches; EU_HIP_HYBRID=2 lifts that limit (tests)
  const bool worth = sw.hybrid == 2 || p.src.degree >= 2;
  if (sw.hybrid && worth && !p.twine && p.norm_mode == EU_NORM_NONE && p.src.prj == EU_SPHERICAL) return EU_PATH_PACKED_RUNS;
  return EU_PATH_PACKED;
}

// ---- rays from the caller (eu_hip_render_rays, eu_render_rays.hip) -------------------------------
// There is no stepper, so no form, no normalisation and no plan: the source and the channel counts decide.
//   general  eu_rays_kernel   one ray or ninepack per lane: every mount, every degree, channel adaption, --mask_for
//   packed   eu_rays2_kernel  two per lane through eu_coord2 / eu_eval2: what eu_packed_covers_source() admits
enum eu_ray_path { EU_RAYS_GENERAL, EU_RAYS_PACKED };

inline eu_ray_path eu_select_ray_path(const eu_rays_params &p, const eu_switches &sw)
{
  if (p.src.mask_paint || sw.force_general) return EU_RAYS_GENERAL;
  return eu_packed_covers_source(p.src, p.nch, p.nch_out) ? EU_RAYS_PACKED : EU_RAYS_GENERAL;
}

// ---- a sequence of views (eu_hip_render_views, eu_render_views.hip) --------------------------------
// The stepper tables of every view are made on the device, so nothing here may depend on a plan: no runs, no
// staged kernels, row strips only.
//   general  eu_views_kernel   one pixel per lane, as eu_render_kernel: every mount and degree, channel adaption,
//                              twining, --mask_for
//   packed   eu_views2_kernel  two per lane, as eu_render2_kernel: what eu_packed_covers() admits
enum eu_view_path { EU_VIEWS_GENERAL, EU_VIEWS_PACKED };

inline eu_view_path eu_select_view_path(const eu_render_params &p, const eu_switches &sw)
{
  if (p.src.mask_paint || sw.force_general) return EU_VIEWS_GENERAL;
  return eu_packed_covers(p) ? EU_VIEWS_PACKED : EU_VIEWS_GENERAL;
}

// views of one chunk: as many as the table bound holds (at least one), and no more than a grid's y extent
// A multi-facet job (eu_hip_render_views_multi) has one table block per (view, facet), and the table kernel has the
// block on blockIdx.y: views * nfct stays within the grid's y extent (nfct itself does: the entry point sees to it)
#define EU_VIEWS_MAX_GRID_Y 65535
inline int eu_views_per_chunk(int width, int height, int max_kb, int nfct = 1)
{
  const unsigned long long nf = (unsigned long long)std::max(nfct, 1);
  const unsigned long long per = nf * ((unsigned long long)6 * width + (unsigned long long)EU_ROW_FLOATS * height) * sizeof(float);
  const unsigned long long n = per ? (unsigned long long)max_kb * 1024ull / per : EU_VIEWS_MAX_GRID_Y;
  return (int)std::max<unsigned long long>(1, std::min<unsigned long long>(n, EU_VIEWS_MAX_GRID_Y / nf));
}

// ---- many pictures of one geometry (eu_hip_render_layers, eu_render_layers.hip) --------------------
// One camera, so the host builds the stepper tables once, as eu_hip_render does; like the view calls there is no
// plan behind the launch: no runs, no staged kernels, row strips only.
//   general  eu_layers_kernel   one pixel per lane: every mount and degree, channel adaption, twining
//   packed   eu_layers2_kernel  two per lane: what eu_packed_covers() admits
// p.src is layer 0's block; the layers agree in everything asked here. A --mask_for source is refused by the entry
// point (the paint would replace every layer's pixels alike); should one arrive, only the general form could paint it.
enum eu_layer_path { EU_LAYERS_GENERAL, EU_LAYERS_PACKED };

inline eu_layer_path eu_select_layer_path(const eu_render_params &p, const eu_switches &sw)
{
  if (p.src.mask_paint || sw.force_general) return EU_LAYERS_GENERAL;
  return eu_packed_covers(p) ? EU_LAYERS_PACKED : EU_LAYERS_GENERAL;
}

// A twined job carries one sum per layer across its tap loop: the layers of a launch are taken in groups of
// EU_LAYERS_GROUP, each group running the tap loop once. Chosen from the compiler's figures ("Many
// pictures of one geometry"): the largest of 1, 2, 4 at which the cubic RGB lat/lon twined kernels keep the three
// wavefronts per SIMD of their single-picture counterparts. That is 1 - at 2 the packed form needs 188 VGPRs (two
// wavefronts), at 4 219 - so a twined launch shares the rays and their differences between layers, not yet the
// coordinates of a tap.
#ifndef EU_LAYERS_GROUP
#define EU_LAYERS_GROUP 1
#endif

// The chunking arithmetic, in one place for the host glue, the kernels and the host test (constexpr: device code
// calls them too). Layers of one launch: layers_max of them (0: all), never more than there are
constexpr int eu_layers_per_launch(int nlayers, int layers_max)
{
  return layers_max > 0 && layers_max < nlayers ? layers_max : nlayers;
}
// launches a list of nlayers takes (eu_hip_render_layers' loop)
constexpr int eu_layers_launches(int nlayers, int layers_max)
{
  return eu_layers_per_launch(nlayers, layers_max) > 0
             ? (nlayers + eu_layers_per_launch(nlayers, layers_max) - 1) / eu_layers_per_launch(nlayers, layers_max) : 0;
}
// tap loops a twined launch of n layers runs per pixel, and the layers of group g (the last one may be partial): the
// twined kernels' group loop
constexpr int eu_layers_groups(int n, int group = EU_LAYERS_GROUP) { return n > 0 ? (n + group - 1) / group : 0; }
constexpr int eu_layers_in_group(int n, int g, int group = EU_LAYERS_GROUP)
{
  return n - g * group <= 0 ? 0 : n - g * group < group ? n - g * group : group;
}

// ---- the run splitter of the packed kernel's launch-level hybrid --------------------------------
// The frame is cut into segments of EU_SEG_ROWS rows; flags[k] != 0 where segment k renders faster with
// 32x16 tiles than with 128x4 row strips (eu_api_render.hip: refresh_seg_flags).
#define EU_SEG_ROWS 512

struct eu_run { int row_begin, row_end, layout; };     // local rows; layout 1 row strips, 2 tiles

// Runs of local rows whose segments want the same layout, in chunks of 64 rows. Empty: one launch for
// the whole job. Every run is a launch of its own, so only a few long runs are worth it (the whole
// frame: 5; a contiguous strip of a split: 1-3), not the many short ones of a band-interleaved share
// (0.18 -> 0.21 ms when split up); any = true (EU_HIP_HYBRID=2) lifts the limits.
inline std::vector<eu_run> eu_split_runs(const unsigned char *flags, int nflags, const eu_render_params &p, bool any)
{
  std::vector<eu_run> runs;
  bool mixed = false;
  for (int k = 0; k < nflags; k++) mixed = mixed || flags[k];
  if (!mixed) return runs;
  auto flag_of = [&](int r) {
    const int fy = eu_frame_row(std::min(r, p.row_end - 1), p.band_shift, p.band_count, p.band_index);
    return (int)flags[std::min(fy / EU_SEG_ROWS, nflags - 1)];
  };
  auto run_end = [&](int a, int fl) {
    int b = std::min((a / 64 + 1) * 64, p.row_end);
    while (b < p.row_end && flag_of(b) == fl) b = std::min(b + 64, p.row_end);
    return b;
  };
  int tiled = 0, shortest = INT_MAX;
  for (int a = p.row_begin; a < p.row_end;) {
    const int fl = flag_of(a), b = run_end(a, fl);
    tiled += fl;
    shortest = std::min(shortest, b - a);
    runs.push_back({ a, b, fl ? 2 : 1 });
    a = b;
  }
  const int nruns = (int)runs.size();
  if (!(tiled > 0 && (any || nruns <= 3 || (nruns <= 5 && shortest >= EU_SEG_ROWS)))) runs.clear();
  return runs;
}

#endif
