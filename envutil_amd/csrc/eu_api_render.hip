// C ABI (include/eu_hip.h), host glue: one frame of a job - the cached plans, the choice of the kernel, the way out
// of the frame as floats, packed words or integer samples.

#include "eu_context.h"
#include "eu_setup_math.h"
#include "eu_encode.h"
#include "eu_rgbe_dev.h"
#include "eu_ycbcr_out.h"
#include "../../include/eu_ycbcr.h"

using namespace eu_host;

namespace {

int band_shift_of(int band_rows)
{
  int sh = 0;
  while ((1 << sh) < band_rows) sh++;
  return sh;
}

// tf22 of a --single job: the inverse planar transformation of the facet the target recreates
// (environment.h:285-307); the inverse lens model goes to device memory (inv_coef)
int build_inv_planar(const eu_target *t, eu_inv_planar *q)
{
  memset(q, 0, sizeof *q);
  const eu_facet *f = t->single;
  if (!f || !eu::has_2d_tf(*f)) return EU_OK;
  q->shear = f->shear_g != 0.0 || f->shear_t != 0.0;
  q->shift = f->h != 0.0 || f->v != 0.0;
  q->lcp = f->a != 0.0 || f->b != 0.0 || f->c != 0.0;
  q->shear_g = f->shear_g; q->shear_t = f->shear_t;
  { // the reference radius: half the smaller edge of the facet's extent (envutil_basic.h:508-513)
    const double dv0 = std::fabs(t->y1 - t->y0) / 2.0, dh0 = std::fabs(t->x1 - t->x0) / 2.0;
    q->s = (dh0 < dv0) ? dh0 : dv0; }
  q->h = (float)f->h; q->v = (float)f->v;
  if (q->lcp) {
    // r_max of facet_spec::process_geometry (envutil_basic.h:508-520) from the target's (= the facet's) extent
    const double dv = std::fabs(t->y1 - t->y0) / 2.0, dh = std::fabs(t->x1 - t->x0) / 2.0;
    const double aspect = (dh >= dv) ? dh / dv : dv / dh;
    std::vector<float> coef;
    if (!eu::make_inverse_lcp(f->a, f->b, f->c, std::sqrt(1 + aspect * aspect), 100, coef, q->rr_max))
      return fail(EU_ERR_ARGUMENT, "--single: the lens polynomial has no inverse over the facet (the reference asserts here)");
    HIPCHK(cur().tables.host_wait());
    if (!cur().inv_coef) HIPCHK(hipMalloc((void **)&cur().inv_coef, 128 * sizeof(float)));
    HIPCHK(hipMemcpyAsync(cur().inv_coef, coef.data(), coef.size() * sizeof(float), hipMemcpyHostToDevice, cur().stream));
    HIPCHK(hipStreamSynchronize(cur().stream));
    q->nk = (int)coef.size() - 4;
    q->coef = cur().inv_coef + 2;
    eu::weight_matrix(3, q->m);
  }
  return EU_OK;
}

// The key of a target's cached plan for nsrc facets, everything the stepper tables depend on: the target without
// the fields that only say which part of the frame a call renders and how it is stored (the tables cover the
// whole frame), [the number of facets - the multi-facet cache's keys only,] the facets' orientations, the taps.
std::vector<unsigned char> plan_key_of(const eu_target *t, eu_source *const *srcs, int nsrc, bool multi)
{
  const size_t ntap_bytes = 3 * sizeof(float) * (size_t)t->ntaps;
  std::vector<unsigned char> key(sizeof(eu_target) + (multi ? sizeof(int) : 0) + (size_t)nsrc * 3 * sizeof(double) + ntap_bytes);
  eu_target tk = *t;
  tk.taps = nullptr; tk.single = nullptr; tk.row_begin = 0; tk.row_end = 0; tk.stage = 0; tk.nchannels = 0; tk.out_format = 0;
  tk.band_rows = 0; tk.band_count = 0; tk.band_index = 0;
  tk.feather = 0.0;                 // the synopsis' business: no table depends on it
  tk.bands = 0;
  unsigned char *q = key.data();
  memcpy(q, &tk, sizeof tk); q += sizeof tk;
  if (multi) { memcpy(q, &nsrc, sizeof(int)); q += sizeof(int); }
  for (int f = 0; f < nsrc; f++) {
    double fo[3] = { srcs[f]->fct.yaw, srcs[f]->fct.pitch, srcs[f]->fct.roll };
    memcpy(q, fo, sizeof fo); q += sizeof fo;
  }
  if (t->ntaps > 0) memcpy(q, t->taps, ntap_bytes);
  return key;
}

// the frame and band fields eu_render_params and eu_multi_params share (p zeroed: no bands)
template <class P> void fill_frame(const eu_target *t, P *p)
{
  p->width = frame_w(t); p->height = frame_h(t);
  p->row_begin = t->row_begin; p->row_end = t->row_end;
  if (t->band_count > 1) {
    p->band_shift = band_shift_of(t->band_rows); p->band_count = t->band_count; p->band_index = t->band_index;
  }
}

// New tables into a plan cache: reserve, upload col / row / taps on the library's stream, synchronise - the host
// vectors may die behind this call -, take the key. `row` is tb.row, or every facet's behind one another. The caller
// has waited for the tables' readers.
int upload_plan(plan_cache &pc, const eu_target *t, const eu::stepper_tables &tb, const std::vector<float> &row,
                std::vector<unsigned char> &key)
{
  HIPCHK(pc.col.reserve(tb.col.size()));
  HIPCHK(pc.row.reserve(row.size()));
  HIPCHK(hipMemcpyAsync(pc.col.p, tb.col.data(), tb.col.size() * sizeof(float), hipMemcpyHostToDevice, cur().stream));
  HIPCHK(hipMemcpyAsync(pc.row.p, row.data(), row.size() * sizeof(float), hipMemcpyHostToDevice, cur().stream));
  const std::vector<float> taps = biased_taps(t->taps, t->ntaps);
  if (t->ntaps > 0) {
    HIPCHK(pc.taps.reserve(taps.size()));
    HIPCHK(hipMemcpyAsync(pc.taps.p, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice, cur().stream));
  }
  HIPCHK(hipStreamSynchronize(cur().stream));
  pc.form = tb.form; pc.norm = tb.norm_mode;
  pc.key.swap(key);
  return EU_OK;
}

int build_params(const eu_target *t, eu_source *const *srcs, int nsrc, float *out_dev,
                 size_t row_stride_bytes, const eu_switches &sw, eu_render_params *p)
{
  if (!t || !srcs || !out_dev) return fail(EU_ERR_ARGUMENT, "null argument");
  if (nsrc != 1)
    return fail(EU_ERR_ARGUMENT, "build_params takes one source (several facets go through build_multi)");
  eu_source *s = srcs[0];
  if (!s) return fail(EU_ERR_HANDLE, "null source");
  { int rc0 = check_target(t); if (rc0) return rc0; }
  if (row_stride_bytes % sizeof(float))
    return fail(EU_ERR_ARGUMENT, "row stride must be a multiple of 4 bytes");
  const bool twine = t->ntaps > 0;
  // orientation: envutil_payload.cc:1923-1948
  eu::mat3 r_cam = eu::make_r3(t->roll, t->pitch, t->yaw, false);
  eu::mat3 r_fct = eu::make_r3(s->fct.roll, s->fct.pitch, s->fct.yaw, true);
  eu::mat3 basis = eu::rotate(r_cam, r_fct);
  // plan key: everything the tables depend on
  // a facet with translation parameters: generic_stepper over tf_ex_facet (envutil_payload.cc:2095-2110,
  // :2214-2224), normalised only under twining (deriv_stepper<..., generic_stepper, true>)
  eu_generic gen;
  memset(&gen, 0, sizeof gen);
  if ((eu::has_translation(s->fct) || eu::generic_target(*t)) && !eu::make_generic(*t, s->fct, gen))
    return fail(EU_ERR_UNSUPPORTED, "generic stepper (translation, --single): no planar-to-ray functor for this target projection");
  eu_inv_planar inv;
  { int rci = build_inv_planar(t, &inv); if (rci) return rci; }
  std::vector<unsigned char> key = plan_key_of(t, srcs, 1, false);
  auto &pl = cur().plan;
  if (key != pl.key) {
    eu::stepper_tables tb;
    if (!eu::build_stepper_tables(*t, basis, twine, twine, tb))
      return fail(EU_ERR_UNSUPPORTED, "no stepper for this target projection");
    // kernels of earlier jobs may still read the tables on callers' streams (the library's own has the copies behind them)
    HIPCHK(cur().tables.host_wait());
    { int rcu = upload_plan(pl, t, tb, tb.row, key); if (rcu) return rcu; }
    pl.h_col.swap(tb.col);
    pl.h_row.swap(tb.row);
    pl.seg_valid = false;
    pl.plan_gen++;
    pl.tab_finite = 1;
    for (float v : pl.h_col) if (!std::isfinite(v)) pl.tab_finite = 0;
    for (float v : pl.h_row) if (!std::isfinite(v)) pl.tab_finite = 0;
  }
  memset(p, 0, sizeof *p);
  p->tab_finite = pl.tab_finite;
  fill_frame(t, p);
  p->form = pl.form; p->norm_mode = pl.norm;
  if (gen.on) {                // the tables (planar x per column, planar y per row) are the same
    p->form = EU_FORM_GENERIC;
    p->norm_mode = twine ? EU_NORM_DIV : EU_NORM_NONE;
    p->gen = gen;
    p->inv = inv;
  }
  p->twine = twine; p->ntaps = t->ntaps; p->stage = t->stage; p->nch = s->nch;
  p->nch_out = t->nchannels;
  p->col = pl.col.p; p->row = pl.row.p; p->taps = pl.taps.p;
  p->out = out_dev;
  p->out_stride = (long long)(row_stride_bytes / sizeof(float));
  p->src = s->sd;
  p->direct = sw.direct;
  return EU_OK;
}

// The multi-facet kernels' second early-miss stage (eu_render_multi.hip: eu_multi_maybe): for a fisheye facet
// (no shear) a table over u = cos(angle to the facet's axis), u in [rej_cos, 1], of a lower bound of the
// radius R(theta) = theta * lens polynomial(theta / s) a ray of that angle maps to (environment.h:254-284,
// geometry.h:513-531), and the window's edges moved out by 0.1 %. tab: EU_REJ_STRIDE floats (eu_launch.h); false: no table.
static bool build_reject_table(const eu_src_dev &d, float *tab, bool analytic)
{
  for (int i = 0; i < EU_REJ_STRIDE; i++) tab[i] = 0.0f;
  if (d.prj != EU_FISHEYE || d.has_shear || d.mask_all || !(d.rej_cos > -1.5f) || !(d.rej_cos < 0.999f)) return false;
  const double u0 = d.rej_cos, du = (1.0 - u0) / EU_REJ_N;
  auto radius = [&](double th, bool &okk) {
    double sum = 1.0;
    if (d.has_lcp) {
      const double x = th / d.lens_s;
      sum = d.lens_d + d.lens_c * x + d.lens_b * x * x + d.lens_a * x * x * x;
    }
    if (!(sum > 0.0)) okk = false;
    return th * sum;
  };
  std::vector<double> raw(EU_REJ_N);
  bool okk = true;
  for (int k = 0; k < EU_REJ_N; k++) {
    const double ua = std::min(1.0, std::max(-1.0, u0 + k * du)), ub = std::min(1.0, std::max(-1.0, u0 + (k + 1) * du));
    const double t_hi = std::acos(ua), t_lo = std::acos(ub);
    double m = 1e300;
    for (int j = 0; j <= 16; j++) m = std::min(m, radius(t_lo + (t_hi - t_lo) * j / 16.0, okk));
    raw[k] = m;
  }
  if (!okk) return false;
  for (int k = 0; k < EU_REJ_N; k++) {
    double m = raw[k];
    if (k > 0) m = std::min(m, raw[k - 1]);
    if (k + 1 < EU_REJ_N) m = std::min(m, raw[k + 1]);
    tab[EU_REJ_HDR + k] = (float)(m * (1.0 - 2e-3));
  }
  const double W = std::max(std::max(std::fabs((double)d.wex0), std::fabs((double)d.wex1)),
                            std::max(std::fabs((double)d.wex2), std::fabs((double)d.wex3)));
  const double mg = 1e-3 * W;
  tab[0] = (float)u0; tab[1] = (float)(1.0 / du); tab[2] = 1.0f;
  // the table-free form (EU_HIP_REJ=2): needs R increasing over the cone
  {
    bool mono = true;
    double prev = -1.0;
    const double tmax = std::acos(std::max(-1.0, u0));
    for (int i = 0; i <= 4096 && mono; i++) {
      bool k2 = true;
      const double r = radius(tmax * i / 4096.0, k2);
      mono = k2 && r > prev;
      prev = r;
    }
    if (mono && analytic) {
      tab[2] = 2.0f;
      const double f = 1.0 - 2e-3;
      tab[10] = d.has_lcp ? 1.0f / d.lens_s : 0.0f;
      tab[11] = (float)(f * (d.has_lcp ? d.lens_d : 1.0)); tab[12] = d.has_lcp ? (float)(f * d.lens_c) : 0.0f;
      tab[13] = d.has_lcp ? (float)(f * d.lens_b) : 0.0f; tab[14] = d.has_lcp ? (float)(f * d.lens_a) : 0.0f;
    }
  }
  tab[4] = d.has_shift ? d.lens_h : 0.0f; tab[5] = d.has_shift ? d.lens_v : 0.0f;
  tab[6] = (float)(d.wex0 - mg); tab[7] = (float)(d.wex1 + mg); tab[8] = (float)(d.wex2 - mg); tab[9] = (float)(d.wex3 + mg);
  return true;
}

// fuse() for several facets (envutil_payload.cc:2139-2180, :2240-2281): one
// stepper per facet, all with normalize = true, synopsis by channel count
int build_multi(const eu_target *t, eu_source *const *srcs, int nsrc, float *out_dev,
                size_t row_stride_bytes, const eu_switches &sw, eu_multi_params *p, int *degree)
{
  { int rc0 = check_target(t); if (rc0) return rc0; }
  const eu_source *s0 = srcs[0];
  for (int f = 0; f < nsrc; f++) {
    if (!srcs[f]) return fail(EU_ERR_HANDLE, "null source");
    if (srcs[f]->degree != s0->degree) return fail(EU_ERR_ARGUMENT, "facets must share the spline degree");
  }
  const bool twine = t->ntaps > 0;
  std::vector<unsigned char> key = plan_key_of(t, srcs, nsrc, true);
  auto &mp = cur().mplan;
  HIPCHK(cur().tables.host_wait());   // mp.src and the tables are rewritten below
  if (key != mp.key) {
    eu::mat3 r_cam = eu::make_r3(t->roll, t->pitch, t->yaw, false);
    std::vector<float> rows;
    eu::stepper_tables tb;
    for (int f = 0; f < nsrc; f++) {
      eu::mat3 r_fct = eu::make_r3(srcs[f]->fct.roll, srcs[f]->fct.pitch, srcs[f]->fct.yaw, true);
      eu::mat3 basis = eu::rotate(r_cam, r_fct);
      if (!eu::build_stepper_tables(*t, basis, true, twine, tb))
        return fail(EU_ERR_UNSUPPORTED, "no stepper for this target projection");
      rows.insert(rows.end(), tb.row.begin(), tb.row.end());
    }
    { int rcu = upload_plan(mp, t, tb, rows, key); if (rcu) return rcu; }
  }
  // the facets' evaluator parameters (they can change between jobs: always refreshed)
  std::vector<eu_src_dev> sd((size_t)nsrc);
  for (int f = 0; f < nsrc; f++) sd[f] = srcs[f]->sd;
  HIPCHK(mp.src.reserve((size_t)nsrc));
  HIPCHK(hipMemcpyAsync(mp.src.p, sd.data(), sizeof(eu_src_dev) * (size_t)nsrc, hipMemcpyHostToDevice, cur().stream));
  // the early-miss tables of the fisheye facets - OFF unless EU_HIP_REJ=1: measured on config 5 the second
  // stage drops a third of the exact hit tests and the step takes 7.67 instead of 7.30 ms (the table read is
  // one more round trip on a path that waits for memory already)
  bool any_rej = false;
  std::vector<float> rej;
  if (sw.rej) {                          // 2: the table-free form where it applies
    rej.resize((size_t)nsrc * EU_REJ_STRIDE);
    for (int f = 0; f < nsrc; f++) any_rej |= build_reject_table(sd[f], rej.data() + (size_t)f * EU_REJ_STRIDE, sw.rej == 2);
  }
  if (any_rej) {
    HIPCHK(mp.rej.reserve(rej.size()));
    HIPCHK(hipMemcpyAsync(mp.rej.p, rej.data(), rej.size() * sizeof(float), hipMemcpyHostToDevice, cur().stream));
  }
  // facets with translation parameters step through generic_stepper (envutil_payload.cc:2145-2158,
  // :2246-2258); like the evaluator parameters these are refreshed on every job
  std::vector<eu_generic> gv((size_t)nsrc);
  bool any_generic = false;
  for (int f = 0; f < nsrc; f++) {
    memset(&gv[f], 0, sizeof(eu_generic));
    if (!eu::has_translation(srcs[f]->fct) && !eu::generic_target(*t)) continue;
    if (!eu::make_generic(*t, srcs[f]->fct, gv[f]))
      return fail(EU_ERR_UNSUPPORTED, "generic stepper (translation, --single): no planar-to-ray functor for this target projection");
    any_generic = true;
  }
  if (any_generic) {
    HIPCHK(mp.gen.reserve((size_t)nsrc));
    HIPCHK(hipMemcpyAsync(mp.gen.p, gv.data(), sizeof(eu_generic) * (size_t)nsrc, hipMemcpyHostToDevice, cur().stream));
  }
  // the feathered synopsis' edge-weight table: the job's, like the two above
  const bool feather = t->synopsis == EU_SYN_FEATHER || t->synopsis == EU_SYN_MULTIBAND;
  const std::vector<eu_feather_dev> fth = feather ? feather_table(t, srcs, nsrc) : std::vector<eu_feather_dev>();
  if (feather) {
    HIPCHK(mp.fth.reserve((size_t)nsrc));
    HIPCHK(hipMemcpyAsync(mp.fth.p, fth.data(), sizeof(eu_feather_dev) * (size_t)nsrc, hipMemcpyHostToDevice, cur().stream));
  }
  HIPCHK(hipStreamSynchronize(cur().stream));
  eu_inv_planar inv;
  { int rci = build_inv_planar(t, &inv); if (rci) return rci; }
  memset(p, 0, sizeof *p);
  p->fth = feather ? mp.fth.p : nullptr;
  p->gen = any_generic ? mp.gen.p : nullptr;
  p->rej = any_rej ? mp.rej.p : nullptr;
  p->inv = inv;
  fill_frame(t, p);
  p->form = mp.form; p->norm_mode = mp.norm; p->twine = twine; p->ntaps = t->ntaps;
  fill_synopsis(t, srcs, nsrc, p);
  p->col = mp.col.p; p->row = mp.row.p; p->taps = mp.taps.p; p->srcs = mp.src.p;
  p->out = out_dev; p->out_stride = (long long)(row_stride_bytes / sizeof(float));
  *degree = s0->degree;
  return EU_OK;
}

// Launch-level hybrid of the packed kernel's two work layouts. Where source rows run
// ACROSS target rows (the inner half of the polar faces of a cubemap made from a lat/lon
// image: 0.098 -> 0.071 ms per 1024 rows) 32x16 tiles beat the 128x4 row strips; everywhere
// else the strips win (0.045 vs 0.055 ms). The frame is cut into segments of EU_SEG_ROWS
// rows (eu_select.h: eu_split_runs); 16 probe pixels per segment, evaluated on the host from the plan's stepper
// tables, say how the source rows run there. Lat/lon sources only.
// (kept while the plan's tables and the source's parameters stay the same)
void refresh_seg_flags(const eu_render_params *p)
{
  eu_src_dev cmp = p->src;
  cmp.base = nullptr;
  if (cur().plan.seg_valid && !memcmp(&cmp, &cur().plan.seg_sd, sizeof cmp)) return;
  cur().plan.seg_sd = cmp;
  cur().plan.seg_valid = true;
  const int W = p->width, H = p->height;
  const int nseg = (H + EU_SEG_ROWS - 1) / EU_SEG_ROWS;
  cur().plan.seg_flags.assign((size_t)nseg, 0);
  const eu_src_dev &s = p->src;
  if (s.prj != EU_SPHERICAL || W < 64 || cur().plan.h_col.size() < (size_t)2 * W || cur().plan.h_row.size() < (size_t)H * EU_ROW_FLOATS)
    return;
  const double kx = (double)s.total_w / s.ext_w, ky = (double)s.total_h / s.ext_h;   // pixels per radian
  auto ray = [&](int x, int y, double *r) {
    const float *rt = &cur().plan.h_row[(size_t)y * EU_ROW_FLOATS];
    const float c0 = cur().plan.h_col[(size_t)x], c1 = cur().plan.h_col[(size_t)W + x];
    for (int i = 0; i < 3; i++)
      r[i] = p->form == EU_FORM_BCA ? (double)rt[3 + i] * c0 + (double)rt[6 + i] * c1 + rt[i]
                                    : (double)rt[3 + i] * c0 + rt[i];
  };
  for (int k = 0; k < nseg; k++) {
    const int yc = std::min(k * EU_SEG_ROWS + EU_SEG_ROWS / 2, H - 1);
    int across = 0;
    for (int j = 0; j < 16; j++) {
      const int xc = std::min((int)((j + 0.5) * W / 16), W - 2);
      double a[3], b[3];
      ray(xc, yc, a);
      ray(xc + 1, yc, b);
      const double lon0 = std::atan2(a[0], a[2]), lon1 = std::atan2(b[0], b[2]);
      const double lat0 = std::atan2(a[1], std::hypot(a[0], a[2])), lat1 = std::atan2(b[1], std::hypot(b[0], b[2]));
      double dlon = std::fabs(lon1 - lon0);
      if (dlon > M_PI) dlon = 2.0 * M_PI - dlon;
      if (std::fabs(lat1 - lat0) * ky > 0.5 * dlon * kx) across++;
    }
    cur().plan.seg_flags[(size_t)k] = across > 8;
  }
}

// the staged kernels: their work list (eu_render4.hip: chunk counters of the persistent kernel, lists of the
// tiles left to the direct-gather kernel that follows it on the same stream) and its order between streams
int launch_staged(const eu_render_params *p, const eu_switches &sw, hipStream_t st, int *launches)
{
  // (more tiles than the work list has ids for: eu_staged_covers said no, and eu_select_path never names this path)
  const unsigned long long ntiles = eu_staged_tiles(p->width, p->row_begin, p->row_end);
  if (ntiles > EU4_WL_MAX_TILES) return -2;
  // every tile of the launch may be listed: the capacity holds for all of them (eu_worklist.h). A buffer that grows
  // starts with both sets of counters empty - the entries need no clearing, the counters say how many of them count -
  // and a smaller job behind a larger one finds its set emptied by the second kernel of the pair before it
  const size_t need = eu_render4_worklist_buffer_ints((size_t)ntiles);
  if (cur().staged.wl.cap < need) {
    if (cur().staged.wl_pair.host_wait() != hipSuccess || cur().staged.wl.reserve(need) != hipSuccess) return -1;
    if (hipMemsetAsync(cur().staged.wl.p, 0, eu_render4_worklist_clear_ints() * sizeof(int), st) != hipSuccess) {
      cur().staged.wl.cap = 0;
      return -1;
    }
  }
  eu_render_params q = *p;
  const int set = cur().staged.parity;
  q.wl = EU4_WL_SET(cur().staged.wl.p, set);
  // the work list, the persistent kernel's queues and the cached plans belong to ONE launch pair at a time: `st` waits
  // for the pair before, the event moves behind this one - on any stream, for eu_hip_listed_tiles() the library's own too
  if (cur().staged.wl_pair.order_after(st) != hipSuccess) return -1;
  const int rc = eu_launch_render4(&q, EU4_WL_SET(cur().staged.wl.p, set ^ 1), &sw, cur().plan.h_row.data(), cur().plan.h_row.size(),
                                   cur().plan.h_col.data(), cur().plan.h_col.size(), cur().plan.plan_gen, st, launches);
  if (rc || !*launches || !ntiles) return rc;     // (a job of no tiles launches nothing)
  // both launches went out: the pair behind this one takes the set this one has emptied
  cur().staged.last_set = set;
  cur().staged.parity = set ^ 1;
  return cur().staged.wl_pair.note(st) != hipSuccess ? -1 : 0;
}

// the packed kernel, one launch per run of rows that want the same work layout (eu_select.h: eu_split_runs)
int launch_packed_runs(const eu_render_params *p, const eu_switches &sw, hipStream_t st, int *launches)
{
  refresh_seg_flags(p);
  const std::vector<eu_run> runs = eu_split_runs(cur().plan.seg_flags.data(), (int)cur().plan.seg_flags.size(), *p, sw.hybrid == 2);
  if (runs.empty()) { *launches = 1; return eu_launch_render2(p, &sw, st); }
  for (const eu_run &r : runs) {
    eu_render_params q = *p;
    q.row_begin = r.row_begin; q.row_end = r.row_end;
    q.out = p->out + (long long)(r.row_begin - p->row_begin) * p->out_stride;
    q.layout = r.layout;
    ++*launches;
    const int rc = eu_launch_render2(&q, &sw, st);
    if (rc) return rc;
  }
  return 0;
}

// the kernel eu_select_path() names for the job
int launch_render(const eu_render_params *p, const eu_switches &sw, hipStream_t st)
{
  eu_path path = eu_select_path(*p, sw);
  int rc = 0, n = 0;
  if (path == EU_PATH_STAGED) {
    rc = launch_staged(p, sw, st, &n);
    if (!rc && !n) path = eu_select_path(*p, sw, false);       // the plan says no (eu_staged_worth)
  }
  switch (path) {
    case EU_PATH_STAGED: break;
    case EU_PATH_PACKED_RUNS: rc = launch_packed_runs(p, sw, st, &n); break;
    case EU_PATH_PACKED: n = 1; rc = eu_launch_render2(p, &sw, st); break;
    case EU_PATH_GENERAL: n = 1; rc = eu_launch_render(p, st); break;
    case EU_PATH_GENERAL_DIRECT: {
      eu_render_params q = *p;
      q.direct = 1;                       // not the LDS-staged variant: it evaluates inline
      n = 1;
      rc = eu_launch_render(&q, st);
    }
  }
  cur().launches += n;
  return rc;
}

// `st` is about to use the frame buffer or the step tables, rewriting them or behind a rewrite: it goes behind every
// earlier job that uses them. On a caller's stream such a job left an event - a render in `tables`, eu_hip_encode_samples
// in `enc.readers`. The library's own stream leaves none: a caller's stream waits for it by handle, once per change of sides.
int order_encoders(hipStream_t st)
{
  if (st == cur().stream) cur().enc.own = true;
  else if (cur().enc.own) { HIPCHK(hipStreamSynchronize(cur().stream)); cur().enc.own = false; }
  HIPCHK(cur().tables.order_after(st));
  HIPCHK(cur().enc.readers.order_after(st));
  return EU_OK;
}

// the launch of the Y'CbCr encode into the planes `d` names, without its frame
eu_ycbcr_encode_params ycbcr_launch_params(const ycbcr_dst &d, const float *tables)
{
  const eu_ycbcr_out &o = *d.o;
  eu_ycbcr_encode_params ep {};
  ep.y = d.y; ep.cb = d.cb; ep.cr = d.cr; ep.y_pitch = d.y_pitch; ep.c_pitch = d.c_pitch;
  ep.tables = tables;
  ep.bits = o.bits; ep.shift = o.shift; ep.sub_x = o.sub_x; ep.sub_y = o.sub_y; ep.c_step = o.c_step;
  ep.k_r = o.k_r; ep.k_g = o.k_g; ep.k_b = o.k_b; ep.c_u = o.c_u; ep.c_v = o.c_v;
  return ep;
}

// Host planes are staged DENSE on the device, plane behind plane on 4-byte boundaries, and copied out per plane at the
// caller's pitches; interleaved chroma is one plane of 2 cw samples per row that starts at the lower of cb and cr.
struct ycbcr_stage {
  size_t sb, sub_y, yrow, crow, cb_off, cr_off, total;   // bytes of a sample, of a dense luma / chroma row; plane offsets
  bool pairs, v_first;
  ycbcr_stage() : sb(1), sub_y(1), yrow(0), crow(0), cb_off(0), cr_off(0), total(0), pairs(false), v_first(false) {}
  ycbcr_stage(const eu_ycbcr_out &o, size_t w, size_t rows)
  {
    sb = (size_t)o.bits / 8; sub_y = (size_t)o.sub_y;
    pairs = o.c_step == 2;
    v_first = pairs && reinterpret_cast<uintptr_t>(o.cr) < reinterpret_cast<uintptr_t>(o.cb);
    const size_t cw = (w + o.sub_x - 1) / o.sub_x, crows = (rows + sub_y - 1) / sub_y;
    yrow = w * sb;
    crow = (pairs ? 2 : 1) * cw * sb;
    cb_off = (rows * yrow + 3) / 4 * 4;
    cr_off = pairs ? cb_off : cb_off + (crows * crow + 3) / 4 * 4;
    total = cr_off + (crows * crow + 3) / 4 * 4;
  }
  // the planes of the staged rows from luma row `a` (a multiple of sub_y) on
  ycbcr_dst at(const eu_ycbcr_out *o, char *base, size_t a) const
  {
    char *y = base + a * yrow, *c0 = base + cb_off + a / sub_y * crow, *c1 = base + cr_off + a / sub_y * crow;
    if (pairs) return ycbcr_dst { o, y, v_first ? c0 + sb : c0, v_first ? c0 : c0 + sb, yrow, crow };
    return ycbcr_dst { o, y, c0, c1, yrow, crow };
  }
  // the n luma rows staged from row `a` on, and their chroma rows, to the caller's planes from luma row `to` on
  hipError_t copy_out(const eu_ycbcr_out &o, const char *base, size_t a, size_t to, size_t n, hipStream_t s) const
  {
    const size_t cn = (n + sub_y - 1) / sub_y;
    hipError_t e = hipMemcpy2DAsync((char *)o.y + to * o.y_pitch, o.y_pitch, base + a * yrow, yrow, yrow, n, hipMemcpyDeviceToHost, s);
    char *cb = (char *)(v_first ? o.cr : o.cb) + to / sub_y * o.c_pitch;
    if (e == hipSuccess)
      e = hipMemcpy2DAsync(cb, o.c_pitch, base + cb_off + a / sub_y * crow, crow, crow, cn, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && !pairs)
      e = hipMemcpy2DAsync((char *)o.cr + to / sub_y * o.c_pitch, o.c_pitch, base + cr_off + a / sub_y * crow, crow, crow, cn,
                           hipMemcpyDeviceToHost, s);
    return e;
  }
};

}  // namespace

namespace eu_host __attribute__((visibility("hidden"))) {

// one job, everything on the device: float pixels straight into out_dev, or float pixels into the library's
// frame buffer followed by a post-pass that writes out_dev - tethered, the to_screen_t pass and its packed words;
// with `enc` (its tables are in enc.steps: upload_steps), the encode to integer samples; with `rgbe`, the encode to
// Radiance quads (no tables; render_frame has ordered `st`); with `yc`, the encode to the planes `yc` names (out_dev is
// not used; the tables are in enc.steps as for `enc`)
int render_on_device(const eu_target *trg, eu_source *const *srcs, int nsrc, float *out_dev, size_t stride_bytes,
                     const eu_switches &sw, hipStream_t st, const eu_encode *enc, bool rgbe, const ycbcr_dst *yc,
                     eu_mb_times *mb_times)
{
  int rc;
  const bool multi = nsrc > 1;
  const bool screen = trg->out_format == EU_OUT_SRGBA8;
  eu_target tf = *trg;
  float *fout = out_dev;
  size_t fstride = stride_bytes;
  const size_t rows = (size_t)(trg->row_end - trg->row_begin);
  if (screen || enc || rgbe || yc) {
    if (screen && !cur().lut) return fail(EU_ERR_NO_DEVICE, "sRGB table missing: library not initialised");
    // a post-pass queued on another stream may still read the frame buffer (render_frame has ordered `st` where enc or rgbe is set)
    if (screen && (rc = order_encoders(st))) return rc;
    tf.out_format = EU_OUT_FLOAT;
    fstride = (size_t)frame_w(trg) * trg->nchannels * sizeof(float);
    if (cur().out.scr.cap < rows * frame_w(trg) * trg->nchannels) HIPCHK(cur().tables.host_wait());      // reserve() will free it
    HIPCHK(cur().out.scr.reserve(rows * frame_w(trg) * trg->nchannels));
    fout = cur().out.scr.p;
  }
  if (multi) {
    eu_multi_params mp;
    int mdeg = 0;
    if ((rc = build_multi(&tf, srcs, nsrc, fout, fstride, sw, &mp, &mdeg))) return rc;
    if (trg->synopsis == EU_SYN_MULTIBAND) {
      // stage A writes the facets' layers into the scratch, the pyramid kernels blend them into the frame
      if ((rc = check_multiband(trg, srcs, nsrc))) return rc;
      eu_mb_geom g;
      multiband_geom(trg, &g);
      const bool alpha = trg->nchannels == 2 || trg->nchannels == 4;
      const int ncol = alpha ? trg->nchannels - 1 : trg->nchannels;
      if ((rc = multiband_reserve(eu_mb_scratch_floats(g, ncol, nsrc), st))) return rc;
      mp.lay = cur().mband.buf.p; mp.lay_plane = (long long)g.off[1];
      // (the stage-time diagnostic: stage A between two events of its own, destroyed whatever happens)
      struct stage_events {
        hipEvent_t a = nullptr, b = nullptr;
        ~stage_events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
      } se;
      if (mb_times) { HIPCHK(hipEventCreate(&se.a)); HIPCHK(hipEventCreate(&se.b)); HIPCHK(hipEventRecord(se.a, st)); }
      if (eu_launch_render_multi(&mp, mdeg, st)) return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
      if (mb_times) {
        float ms = 0.0f;
        HIPCHK(hipEventRecord(se.b, st));
        HIPCHK(hipEventSynchronize(se.b));
        HIPCHK(hipEventElapsedTime(&ms, se.a, se.b));
        mb_times->ms[EU_MB_T_STAGE_A] += ms;
        mb_times->bytes[EU_MB_T_STAGE_A] += 4.0 * ((double)nsrc * (ncol + 1) + 3) * (double)g.off[1];   // what it writes
      }
      const eu_mb_out mo { fout, (long long)(fstride / sizeof(float)), trg->nchannels, alpha ? 1 : 0, 1 };
      if (eu_launch_mb_blend(cur().mband.buf.p, &g, ncol, nsrc, &mo, st, mb_times)) return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
      if (st != cur().stream) HIPCHK(cur().mband.readers.note(st));
    } else if (eu_launch_render_multi(&mp, mdeg, st)) return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
  } else {
    eu_render_params p;
    if ((rc = build_params(&tf, srcs, nsrc, fout, fstride, sw, &p))) return rc;
    if (launch_render(&p, sw, st)) return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
  }
  if (screen &&
      eu_launch_to_screen(fout, (long long)(fstride / sizeof(float)), (unsigned *)out_dev,
                          (long long)(stride_bytes / sizeof(unsigned)), frame_w(trg), (int)rows,
                          trg->nchannels, cur().lut, st))
    return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
  if (enc && rows) {
    eu_encode_params ep {};
    ep.src = fout; ep.src_stride_bytes = fstride;
    ep.dst = out_dev; ep.dst_stride_bytes = stride_bytes;
    ep.tables = cur().enc.steps.dev.p;
    ep.w = frame_w(trg); ep.h = (int)rows; ep.nch = trg->nchannels;
    ep.bits = enc->bits; ep.big_endian = enc->big_endian;
    if (eu_launch_encode(&ep, st)) return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
  }
  if (rgbe && rows) {
    eu_rgbe_encode_params ep {};
    ep.src = fout; ep.src_stride_bytes = fstride;
    ep.dst = reinterpret_cast<uint32_t *>(out_dev); ep.dst_stride_bytes = stride_bytes;
    ep.w = frame_w(trg); ep.h = (int)rows;
    if (eu_launch_rgbe_encode(&ep, st)) return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
  }
  if (yc && rows) {
    eu_ycbcr_encode_params ep = ycbcr_launch_params(*yc, cur().enc.steps.dev.p);
    ep.src = fout; ep.src_stride_bytes = fstride;
    ep.w = frame_w(trg); ep.h = (int)rows; ep.nch = trg->nchannels;
    if (eu_launch_ycbcr_encode(&ep, st)) return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
  }
  return EU_OK;
}

}  // namespace eu_host

extern "C" {

// ---- integer samples on the way out (eu_encode.hip) -------------------------------------------------------------
// a step table as eu_hip.h defines it: steps[1 .. m] free of NaN and non-decreasing, m >= 1, NaN behind m
static int check_steps(const float *s, int bits, const char *who, const char *which)
{
  const int n = 1 << bits;
  const std::string head = std::string(who) + ": " + which + " steps: ";
  if (std::isnan(s[1])) return fail(EU_ERR_ARGUMENT, head + "entry 1 is NaN, a table has at least one code above 0");
  int m = 1;
  for (; m + 1 < n && !std::isnan(s[m + 1]); m++)
    if (s[m + 1] < s[m]) return fail(EU_ERR_ARGUMENT, head + "entry " + std::to_string(m + 1) + " is smaller than the one before it");
  for (int k = m + 1; k < n; k++)
    if (!std::isnan(s[k]))
      return fail(EU_ERR_ARGUMENT, head + "entry " + std::to_string(k) + " is a number behind the NaN at entry " + std::to_string(m + 1));
  return EU_OK;
}

// what both sample entry points ask of `enc` and `out`: rows of `width` pixels of `nch` samples
static int check_encode(const char *who, const eu_encode *enc, int width, int nch, const void *out, size_t out_row_stride_bytes)
{
  const std::string head = std::string(who) + ": ";
  if (!enc || !out) return fail(EU_ERR_ARGUMENT, head + "null argument");
  if (enc->bits != 8 && enc->bits != 16) return fail(EU_ERR_ARGUMENT, head + "bits must be 8 or 16");
  if (!enc->colour_steps) return fail(EU_ERR_ARGUMENT, head + "null colour steps");
  if (nch < 1 || nch > 4) return fail(EU_ERR_ARGUMENT, head + "channels must be 1..4");
  if (width < 0 || (size_t)width * nch > (size_t(1) << 28)) return fail(EU_ERR_ARGUMENT, head + "rows of 0 .. 2^28 samples");
  if (out_row_stride_bytes < (size_t)width * nch * (enc->bits / 8)) return fail(EU_ERR_ARGUMENT, head + "row stride smaller than a row");
  if (enc->bits == 16 && (reinterpret_cast<uintptr_t>(out) % 2 || out_row_stride_bytes % 2))
    return fail(EU_ERR_ARGUMENT, head + "16-bit samples lie at even addresses: out and its row stride are multiples of 2");
  int rc;
  if ((rc = check_steps(enc->colour_steps, enc->bits, who, "colour"))) return rc;
  if (enc->alpha_steps && (rc = check_steps(enc->alpha_steps, enc->bits, who, "alpha"))) return rc;
  return EU_OK;
}

// The tables of `enc` into enc.steps, in front of the work this call queues on `st`. The buffers of the sample entry
// points (tables, frame buffer) are about to be used on `st`: it goes behind the calls that used them before
// (order_encoders). The upload reads the library's own host copy, never the caller's memory; tables equal to the last
// ones are not sent again.
static int upload_steps(const eu_encode *enc, hipStream_t st)
{
  { int rc = order_encoders(st); if (rc) return rc; }
  const size_t n = size_t(1) << enc->bits;
  const float *alpha = enc->alpha_steps ? enc->alpha_steps : enc->colour_steps;
  held_table &steps = cur().enc.steps;
  if (steps.holds(enc->colour_steps, n, alpha, n)) return EU_OK;
  // earlier work may still read the device tables, and their upload the host copy: `st` is behind all of it
  HIPCHK(hipStreamSynchronize(st));
  steps.host.assign(enc->colour_steps, enc->colour_steps + n);
  steps.host.insert(steps.host.end(), alpha, alpha + n);
  hipError_t e = steps.dev.reserve(2 * n);
  if (e == hipSuccess) e = hipMemcpyAsync(steps.dev.p, steps.host.data(), 2 * n * sizeof(float), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) {
    steps.host.clear();
    return fail(EU_ERR_NO_DEVICE, std::string("step tables: ") + hipGetErrorString(e));
  }
  return EU_OK;
}

static int check_render_sources(const eu_target *trg, eu_source *const *srcs, int nsrc)
{
  if (nsrc > 1 && trg->stage) return fail(EU_ERR_ARGUMENT, "stage outputs exist for single-facet jobs only");
  { int rcm = check_multiband(trg, srcs, nsrc); if (rcm) return rcm; }
  for (int f = 0; f < nsrc; f++) {
    if (!srcs[f]) return fail(EU_ERR_HANDLE, "null source");
    // a masking job adapts channel counts with mono_t, which knows 1 and 2 output channels only
    // (environment.h:1339: the reference asserts)
    if (srcs[f]->fct.mask_paint && srcs[f]->nch != trg->nchannels && trg->nchannels > 2 && !trg->stage)
      return fail(EU_ERR_ARGUMENT, "--mask_for: facets whose channel count differs from the target's need a 1- or 2-channel target");
  }
  return EU_OK;
}

// The job of eu_hip_render, eu_hip_render_samples and eu_hip_render_rgbe behind their argument checks: `out` receives
// rows of row_bytes bytes - floats or packed words, or, with `enc`, integer samples, or, with `rgbe`, Radiance quads.
// With `yco`, `enc` holds its two tables (for the upload alone) and the planes it names receive the frame; `out`, row_bytes
// and the stride are not used.
static int render_frame(const eu_target *trg, eu_source *const *srcs, int nsrc, void *out, size_t row_bytes,
                        size_t out_row_stride_bytes, int out_on_device, void *stream, const eu_encode *enc, bool rgbe = false,
                        const eu_ycbcr_out *yco = nullptr)
{
  int rc;
  hipStream_t st = stream ? (hipStream_t)stream : cur().stream;
  const eu_switches sw = eu_read_switches();
  if (enc && (rc = upload_steps(enc, st))) return rc;
  // the frame buffer is about to be rewritten on `st`: behind the calls that used it before, as upload_steps orders it
  if (rgbe && (rc = order_encoders(st))) return rc;
  // the sources may have been refilled in place (eu_hip_source_reload): `st` reads them behind that
  if ((rc = order_sources(srcs, nsrc, st))) return rc;
  if (yco && out_on_device) {
    const ycbcr_dst yd { yco, yco->y, yco->cb, yco->cr, yco->y_pitch, yco->c_pitch };
    return note_readers(cur().tables, srcs, nsrc, stream, render_on_device(trg, srcs, nsrc, nullptr, 0, sw, st, nullptr, false, &yd));
  }
  if (out_on_device)
    return note_readers(cur().tables, srcs, nsrc, stream, render_on_device(trg, srcs, nsrc, (float *)out, out_row_stride_bytes, sw, st, enc, rgbe));
  const size_t rows = (size_t)(trg->row_end - trg->row_begin);
  if (!rows) return EU_OK;
  const ycbcr_stage ys = yco ? ycbcr_stage(*yco, (size_t)frame_w(trg), rows) : ycbcr_stage();
  HIPCHK(cur().out.stage.reserve(((yco ? ys.total : rows * row_bytes) + sizeof(float) - 1) / sizeof(float)));
  // The frame goes to the host in up to four row chunks: every chunk is a launch of its own
  // on `st`, and its copy (second stream, behind the chunk's event) runs while the later
  // chunks render - the link (57 GB/s pinned, 21 ms for the 1.2 GB headline frame) is the
  // whole cost, the kernels hide under the first copy. Samples and quads: the encode runs behind each chunk's render,
  // and the link carries a quarter, half or a third of the bytes.
  // (a multi-band job is one chunk: its pyramid needs the whole frame)
  const size_t nchunk = rows >= 1024 && !(nsrc > 1 && trg->synopsis == EU_SYN_MULTIBAND) ? 4 : 1;
  if (!cur().out.copy) HIPCHK(hipStreamCreateWithFlags(&cur().out.copy, hipStreamNonBlocking));
  for (size_t c = 0; c < 4; c++)
    if (!cur().out.chunk_done[c]) HIPCHK(hipEventCreateWithFlags(&cur().out.chunk_done[c], hipEventDisableTiming));
  const size_t per = ((rows + nchunk - 1) / nchunk + 7) / 8 * 8;
  drain drain_on_exit{ cur().out.copy, st };      // a host output leaves nothing behind on `st`
  for (size_t c = 0; c < nchunk; c++) {
    const size_t a = std::min(rows, c * per), b = std::min(rows, (c + 1) * per);
    if (a >= b) break;
    eu_target tc = *trg;
    tc.row_begin = trg->row_begin + (int)a;
    tc.row_end = trg->row_begin + (int)b;
    char *dst = (char *)cur().out.stage.p + a * row_bytes;
    if (yco) {                                    // `a` is a multiple of 8: no chunk splits a chroma row
      const ycbcr_dst yd = ys.at(yco, (char *)cur().out.stage.p, a);
      if ((rc = render_on_device(&tc, srcs, nsrc, nullptr, 0, sw, st, nullptr, false, &yd))) return rc;
    } else if ((rc = render_on_device(&tc, srcs, nsrc, (float *)dst, row_bytes, sw, st, enc, rgbe))) return rc;
    HIPCHK(hipEventRecord(cur().out.chunk_done[c], st));
    HIPCHK(hipStreamWaitEvent(cur().out.copy, cur().out.chunk_done[c], 0));
    if (yco) HIPCHK(ys.copy_out(*yco, (const char *)cur().out.stage.p, a, a, b - a, cur().out.copy));
    else
      HIPCHK(hipMemcpy2DAsync((char *)out + a * out_row_stride_bytes, out_row_stride_bytes, dst, row_bytes,
                              row_bytes, b - a, hipMemcpyDeviceToHost, cur().out.copy));
  }
  HIPCHK(hipStreamSynchronize(cur().out.copy));
  HIPCHK(hipStreamSynchronize(st));
  return EU_OK;
}

int eu_hip_render(const eu_target *trg, eu_source *const *srcs, int nsrc, float *out,
                  size_t out_row_stride_bytes, int out_on_device, void *stream)
{
  int rc;
  if (trg && (rc = check_synopsis(trg))) return rc;      // before a device is looked for
  if (trg && srcs && (rc = check_multiband(trg, srcs, nsrc))) return rc;
  if ((rc = ensure_init())) return rc;
  if (!trg) return fail(EU_ERR_ARGUMENT, "null target");
  if (!srcs || nsrc < 1 || !out) return fail(EU_ERR_ARGUMENT, "no source / no output");
  if ((rc = check_target(trg))) return rc;
  const size_t min_stride = frame_row_bytes(trg);
  if (out_row_stride_bytes < min_stride) return fail(EU_ERR_ARGUMENT, "row stride smaller than a row");
  if (out_row_stride_bytes % sizeof(float)) return fail(EU_ERR_ARGUMENT, "row stride must be a multiple of 4 bytes");
  if ((rc = check_render_sources(trg, srcs, nsrc))) return rc;
  return render_frame(trg, srcs, nsrc, out, min_stride, out_row_stride_bytes, out_on_device, stream, nullptr);
}

int eu_hip_render_samples(const eu_target *trg, eu_source *const *srcs, int nsrc, const eu_encode *enc, void *out,
                          size_t out_row_stride_bytes, int out_on_device, void *stream)
{
  int rc;
  if (!trg) return fail(EU_ERR_ARGUMENT, "render_samples: null target");
  if (!srcs || nsrc < 1 || !out) return fail(EU_ERR_ARGUMENT, "render_samples: no source / no output");
  if ((rc = check_target(trg))) return rc;
  if (trg->stage) return fail(EU_ERR_ARGUMENT, "render_samples: stage outputs are float only");
  if (trg->out_format != EU_OUT_FLOAT) return fail(EU_ERR_ARGUMENT, "render_samples: EU_OUT_SRGBA8 is a format of its own, not a frame to encode");
  if ((rc = check_encode("render_samples", enc, frame_w(trg), trg->nchannels, out, out_row_stride_bytes))) return rc;
  if ((rc = check_render_sources(trg, srcs, nsrc))) return rc;
  if ((rc = ensure_init())) return rc;
  if (trg->row_end == trg->row_begin) return EU_OK;
  const size_t row_bytes = (size_t)frame_w(trg) * trg->nchannels * (enc->bits / 8);
  return render_frame(trg, srcs, nsrc, out, row_bytes, out_row_stride_bytes, out_on_device, stream, enc);
}

// bytes (frame and samples together) of one staged chunk of an eu_hip_encode_samples call with a host buffer
#define EU_ENCODE_CHUNK_BYTES ((size_t)64 << 20)

int eu_hip_encode_samples(const float *frame, size_t frame_row_stride_bytes, int frame_on_device, int width, int height,
                          int nchannels, const eu_encode *enc, void *out, size_t out_row_stride_bytes, int out_on_device,
                          void *stream)
{
  int rc;
  if (!frame) return fail(EU_ERR_ARGUMENT, "encode_samples: null argument");
  if (height < 0) return fail(EU_ERR_ARGUMENT, "encode_samples: negative height");
  if ((rc = check_encode("encode_samples", enc, width, nchannels, out, out_row_stride_bytes))) return rc;
  const size_t in_row = (size_t)width * nchannels * sizeof(float), out_row = (size_t)width * nchannels * (enc->bits / 8);
  if (frame_row_stride_bytes < in_row) return fail(EU_ERR_ARGUMENT, "encode_samples: frame row stride smaller than a row");
  if (frame_row_stride_bytes % sizeof(float) || reinterpret_cast<uintptr_t>(frame) % sizeof(float))
    return fail(EU_ERR_ARGUMENT, "encode_samples: the frame and its row stride are multiples of 4 bytes");
  if (!width || !height) return EU_OK;
  if ((rc = ensure_init())) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : cur().stream;
  if ((rc = upload_steps(enc, st))) return rc;
  eu_encode_params ep {};
  ep.tables = cur().enc.steps.dev.p;
  ep.w = width; ep.nch = nchannels; ep.bits = enc->bits; ep.big_endian = enc->big_endian;
  if (frame_on_device && out_on_device) {
    ep.src = frame; ep.src_stride_bytes = frame_row_stride_bytes;
    ep.dst = out; ep.dst_stride_bytes = out_row_stride_bytes;
    ep.h = height;
    if (eu_launch_encode(&ep, st)) return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
    return note_caller(cur().enc.readers, stream, EU_OK);
  }
  // A host buffer on either side: the rows go through in chunks of bounded size - copy in, encode, copy out, in
  // order on `st`; the call returns when `out` is complete
  const int ch = (int)std::min<size_t>((size_t)height, std::max<size_t>(1, EU_ENCODE_CHUNK_BYTES / (in_row + out_row)));
  if (!frame_on_device) HIPCHK(cur().enc.frame.reserve((size_t)ch * width * nchannels));
  if (!out_on_device) HIPCHK(cur().enc.out.reserve(((size_t)ch * out_row + 3) / 4));
  drain drain_on_exit{ st, st };
  for (int y0 = 0; y0 < height; y0 += ch) {
    const int h = std::min(ch, height - y0);
    const char *fin = (const char *)frame + (size_t)y0 * frame_row_stride_bytes;
    char *fout = (char *)out + (size_t)y0 * out_row_stride_bytes;
    ep.src = (const float *)fin; ep.src_stride_bytes = frame_row_stride_bytes;
    ep.dst = fout; ep.dst_stride_bytes = out_row_stride_bytes;
    ep.h = h;
    if (!frame_on_device) {
      ep.src = cur().enc.frame.p; ep.src_stride_bytes = in_row;
      HIPCHK(hipMemcpy2DAsync(cur().enc.frame.p, in_row, fin, frame_row_stride_bytes, in_row, (size_t)h, hipMemcpyHostToDevice, st));
    }
    if (!out_on_device) { ep.dst = cur().enc.out.p; ep.dst_stride_bytes = out_row; }
    if (eu_launch_encode(&ep, st)) return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
    if (!out_on_device)
      HIPCHK(hipMemcpy2DAsync(fout, out_row_stride_bytes, cur().enc.out.p, out_row, out_row, (size_t)h, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  return EU_OK;
}

// ---- Y'CbCr planes on the way out (eu_ycbcr_out.hip) -----------------------------------------------------------------
// what the three entry points ask of `dst` for rows of `width` pixels of `nch` floats
static int check_ycbcr_out(const char *who, const eu_ycbcr_out *o, int width, int nch)
{
  const std::string head = std::string(who) + ": ";
  if (!o) return fail(EU_ERR_ARGUMENT, head + "null dst");
  if (!o->y || !o->cb || !o->cr) return fail(EU_ERR_ARGUMENT, head + "null plane (y, cb, cr)");
  if (!o->y_steps || !o->c_steps) return fail(EU_ERR_ARGUMENT, head + "null table (y_steps, c_steps)");
  if (o->bits != 8 && o->bits != 16) return fail(EU_ERR_ARGUMENT, head + "bits must be 8 or 16");
  if (o->shift < 0 || o->shift >= o->bits) return fail(EU_ERR_ARGUMENT, head + "shift must be 0 .. bits - 1");
  if (o->sub_x != 1 && o->sub_x != 2) return fail(EU_ERR_ARGUMENT, head + "sub_x must be 1 or 2");
  if (o->sub_y != 1 && o->sub_y != 2) return fail(EU_ERR_ARGUMENT, head + "sub_y must be 1 or 2");
  if (o->c_step != 1 && o->c_step != 2) return fail(EU_ERR_ARGUMENT, head + "c_step must be 1 or 2");
  const size_t sb = (size_t)o->bits / 8;
  const uintptr_t ab = reinterpret_cast<uintptr_t>(o->cb), ar = reinterpret_cast<uintptr_t>(o->cr);
  if (o->c_step == 2 && ar != ab + sb && ab != ar + sb)
    return fail(EU_ERR_ARGUMENT, head + "c_step 2 is interleaved chroma: cr is cb plus or minus exactly one sample");
  if (nch != 3 && nch != 4) return fail(EU_ERR_ARGUMENT, head + "nchannels must be 3 or 4");
  if (width < 0 || (size_t)width * nch > (size_t(1) << 28)) return fail(EU_ERR_ARGUMENT, head + "rows of 0 .. 2^28 floats (width)");
  if (width > 0) {
    const size_t cw = ((size_t)width + o->sub_x - 1) / o->sub_x;
    if (o->y_pitch < (size_t)width * sb) return fail(EU_ERR_ARGUMENT, head + "y_pitch shorter than a row of luma samples");
    if (o->c_pitch < ((cw - 1) * o->c_step + 1) * sb) return fail(EU_ERR_ARGUMENT, head + "c_pitch shorter than a row of chroma samples");
  }
  if (o->bits == 16 && ((reinterpret_cast<uintptr_t>(o->y) | ab | ar) & 1))
    return fail(EU_ERR_ARGUMENT, head + "16-bit planes (y, cb, cr) lie at even addresses");
  if (o->bits == 16 && ((o->y_pitch | o->c_pitch) & 1))
    return fail(EU_ERR_ARGUMENT, head + "16-bit planes have even pitches (y_pitch, c_pitch)");
  int rc;
  if ((rc = check_steps(o->y_steps, o->bits, who, "y"))) return rc;
  if ((rc = check_steps(o->c_steps, o->bits, who, "c"))) return rc;
  return EU_OK;
}

// ... and of the float frame that feeds them
static int check_ycbcr_frame(const char *who, const float *frame, size_t stride, int width, int height, int nch)
{
  const std::string head = std::string(who) + ": ";
  if (!frame) return fail(EU_ERR_ARGUMENT, head + "null frame");
  if (height < 0) return fail(EU_ERR_ARGUMENT, head + "negative height");
  if (stride < (size_t)width * nch * sizeof(float)) return fail(EU_ERR_ARGUMENT, head + "frame row stride smaller than a row");
  if (stride % sizeof(float) || reinterpret_cast<uintptr_t>(frame) % sizeof(float))
    return fail(EU_ERR_ARGUMENT, head + "the frame and its row stride are multiples of 4 bytes");
  return EU_OK;
}

int eu_hip_ycbcr_planes(const float *frame, size_t frame_row_stride_bytes, int width, int height, int nchannels,
                        const eu_ycbcr_out *dst)
{
  int rc;
  if ((rc = check_ycbcr_out("ycbcr_planes", dst, width, nchannels))) return rc;
  if ((rc = check_ycbcr_frame("ycbcr_planes", frame, frame_row_stride_bytes, width, height, nchannels))) return rc;
  if (dst->on_device) return fail(EU_ERR_ARGUMENT, "ycbcr_planes: a host function, on_device must be 0");
  if (!width || !height) return EU_OK;
  eu_ycbcr_planes_rows(frame, frame_row_stride_bytes, width, height, nchannels, dst->y, dst->cb, dst->cr, dst->y_pitch,
                       dst->c_pitch, dst->c_step, dst->sub_x, dst->sub_y, dst->bits, dst->shift, dst->y_steps, dst->c_steps,
                       dst->k_r, dst->k_g, dst->k_b, dst->c_u, dst->c_v);
  return EU_OK;
}

int eu_hip_encode_ycbcr(const float *frame, size_t frame_row_stride_bytes, int frame_on_device, int width, int height,
                        int nchannels, const eu_ycbcr_out *dst, void *stream)
{
  int rc;
  if ((rc = check_ycbcr_out("encode_ycbcr", dst, width, nchannels))) return rc;
  if ((rc = check_ycbcr_frame("encode_ycbcr", frame, frame_row_stride_bytes, width, height, nchannels))) return rc;
  if (!width || !height) return EU_OK;
  if ((rc = ensure_init())) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : cur().stream;
  const eu_encode tabs { dst->bits, 0, dst->y_steps, dst->c_steps };
  if ((rc = upload_steps(&tabs, st))) return rc;
  const ycbcr_dst whole { dst, dst->y, dst->cb, dst->cr, dst->y_pitch, dst->c_pitch };
  if (frame_on_device && dst->on_device) {
    eu_ycbcr_encode_params ep = ycbcr_launch_params(whole, cur().enc.steps.dev.p);
    ep.src = frame; ep.src_stride_bytes = frame_row_stride_bytes;
    ep.w = width; ep.h = height; ep.nch = nchannels;
    if (eu_launch_ycbcr_encode(&ep, st)) return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
    return note_caller(cur().enc.readers, stream, EU_OK);
  }
  // A host buffer on either side: the chunks of eu_hip_encode_samples through its staging buffers, each a whole
  // number of chroma rows - a chunk that split one would make two half-filled means of it
  const size_t sb = (size_t)dst->bits / 8, cw = ((size_t)width + dst->sub_x - 1) / dst->sub_x;
  const size_t in_row = (size_t)width * nchannels * sizeof(float), out_row = ((size_t)width + 2 * cw) * sb;
  size_t fit = std::max<size_t>(1, EU_ENCODE_CHUNK_BYTES / (in_row + out_row));
  fit = std::max<size_t>((size_t)dst->sub_y, fit / dst->sub_y * dst->sub_y);
  const int ch = (int)std::min<size_t>((size_t)height, fit);
  const ycbcr_stage ys(*dst, (size_t)width, (size_t)ch);
  if (!frame_on_device) HIPCHK(cur().enc.frame.reserve((size_t)ch * width * nchannels));
  if (!dst->on_device) HIPCHK(cur().enc.out.reserve((ys.total + 3) / 4));
  drain drain_on_exit{ st, st };
  for (int y0 = 0; y0 < height; y0 += ch) {
    const int h = std::min(ch, height - y0);
    const char *fin = (const char *)frame + (size_t)y0 * frame_row_stride_bytes;
    const size_t c0 = (size_t)(y0 / dst->sub_y) * dst->c_pitch;
    const ycbcr_dst yd = dst->on_device
      ? ycbcr_dst { dst, (char *)dst->y + (size_t)y0 * dst->y_pitch, (char *)dst->cb + c0, (char *)dst->cr + c0, dst->y_pitch, dst->c_pitch }
      : ys.at(dst, (char *)cur().enc.out.p, 0);
    eu_ycbcr_encode_params ep = ycbcr_launch_params(yd, cur().enc.steps.dev.p);
    ep.src = (const float *)fin; ep.src_stride_bytes = frame_row_stride_bytes;
    ep.w = width; ep.h = h; ep.nch = nchannels;
    if (!frame_on_device) {
      ep.src = cur().enc.frame.p; ep.src_stride_bytes = in_row;
      HIPCHK(hipMemcpy2DAsync(cur().enc.frame.p, in_row, fin, frame_row_stride_bytes, in_row, (size_t)h, hipMemcpyHostToDevice, st));
    }
    if (eu_launch_ycbcr_encode(&ep, st)) return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
    if (!dst->on_device) HIPCHK(ys.copy_out(*dst, (const char *)cur().enc.out.p, 0, (size_t)y0, (size_t)h, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  return EU_OK;
}

int eu_hip_render_ycbcr(const eu_target *trg, eu_source *const *srcs, int nsrc, const eu_ycbcr_out *dst, void *stream)
{
  int rc;
  if (!trg) return fail(EU_ERR_ARGUMENT, "render_ycbcr: null target");
  if (!srcs || nsrc < 1) return fail(EU_ERR_ARGUMENT, "render_ycbcr: no source");
  if ((rc = check_target(trg))) return rc;
  if (trg->stage) return fail(EU_ERR_ARGUMENT, "render_ycbcr: stage outputs are float only");
  if (trg->out_format != EU_OUT_FLOAT) return fail(EU_ERR_ARGUMENT, "render_ycbcr: EU_OUT_SRGBA8 is a format of its own, not a frame to encode");
  if ((rc = check_ycbcr_out("render_ycbcr", dst, frame_w(trg), trg->nchannels))) return rc;
  if ((rc = check_render_sources(trg, srcs, nsrc))) return rc;
  if ((rc = ensure_init())) return rc;
  if (trg->row_end == trg->row_begin) return EU_OK;
  const eu_encode tabs { dst->bits, 0, dst->y_steps, dst->c_steps };
  return render_frame(trg, srcs, nsrc, nullptr, 0, 0, dst->on_device, stream, &tabs, false, dst);
}

// ---- Radiance RGBE quads on the way out (eu_rgbe.hip) -------------------------------------------------------------
// what both entry points ask of `out`: rows of `width` quads on 4-byte boundaries
static int check_rgbe_out(const char *who, int width, const void *out, size_t out_row_stride_bytes)
{
  const std::string head = std::string(who) + ": ";
  if (!out) return fail(EU_ERR_ARGUMENT, head + "null argument");
  if (width < 0 || (size_t)width > (size_t(1) << 28)) return fail(EU_ERR_ARGUMENT, head + "rows of 0 .. 2^28 pixels");
  if (out_row_stride_bytes < (size_t)width * 4) return fail(EU_ERR_ARGUMENT, head + "row stride smaller than a row");
  if (reinterpret_cast<uintptr_t>(out) % 4 || out_row_stride_bytes % 4)
    return fail(EU_ERR_ARGUMENT, head + "quads lie on 4-byte boundaries: out and its row stride are multiples of 4");
  return EU_OK;
}

int eu_hip_render_rgbe(const eu_target *trg, eu_source *const *srcs, int nsrc, void *out, size_t out_row_stride_bytes,
                       int out_on_device, void *stream)
{
  int rc;
  if (!trg) return fail(EU_ERR_ARGUMENT, "render_rgbe: null target");
  if (!srcs || nsrc < 1 || !out) return fail(EU_ERR_ARGUMENT, "render_rgbe: no source / no output");
  if ((rc = check_target(trg))) return rc;
  if (trg->stage) return fail(EU_ERR_ARGUMENT, "render_rgbe: stage outputs are float only");
  if (trg->out_format != EU_OUT_FLOAT) return fail(EU_ERR_ARGUMENT, "render_rgbe: EU_OUT_SRGBA8 is a format of its own, not a frame to encode");
  if (trg->nchannels != 3) return fail(EU_ERR_ARGUMENT, "render_rgbe: a Radiance picture holds 3 channels");
  if ((rc = check_rgbe_out("render_rgbe", frame_w(trg), out, out_row_stride_bytes))) return rc;
  if ((rc = check_render_sources(trg, srcs, nsrc))) return rc;
  if ((rc = ensure_init())) return rc;
  if (trg->row_end == trg->row_begin) return EU_OK;
  return render_frame(trg, srcs, nsrc, out, (size_t)frame_w(trg) * 4, out_row_stride_bytes, out_on_device, stream, nullptr, true);
}

int eu_hip_encode_rgbe(const float *frame, size_t frame_row_stride_bytes, int frame_on_device, int width, int height,
                       void *out, size_t out_row_stride_bytes, int out_on_device, void *stream)
{
  int rc;
  if (!frame) return fail(EU_ERR_ARGUMENT, "encode_rgbe: null argument");
  if (height < 0) return fail(EU_ERR_ARGUMENT, "encode_rgbe: negative height");
  if ((rc = check_rgbe_out("encode_rgbe", width, out, out_row_stride_bytes))) return rc;
  const size_t in_row = (size_t)width * 3 * sizeof(float), out_row = (size_t)width * 4;
  if (frame_row_stride_bytes < in_row) return fail(EU_ERR_ARGUMENT, "encode_rgbe: frame row stride smaller than a row");
  if (frame_row_stride_bytes % sizeof(float) || reinterpret_cast<uintptr_t>(frame) % sizeof(float))
    return fail(EU_ERR_ARGUMENT, "encode_rgbe: the frame and its row stride are multiples of 4 bytes");
  if (!width || !height) return EU_OK;
  if ((rc = ensure_init())) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : cur().stream;
  eu_rgbe_encode_params ep {};
  ep.w = width;
  if (frame_on_device && out_on_device) {
    // nothing of the library's is read: no table, no staging - so the call leaves no event behind either
    ep.src = frame; ep.src_stride_bytes = frame_row_stride_bytes;
    ep.dst = static_cast<uint32_t *>(out); ep.dst_stride_bytes = out_row_stride_bytes;
    ep.h = height;
    if (eu_launch_rgbe_encode(&ep, st)) return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
    return EU_OK;
  }
  // A host buffer on either side: the chunks of eu_hip_encode_samples, through its staging buffers. `st` goes behind
  // the calls that used them before; the call returns when `out` is complete.
  if ((rc = order_encoders(st))) return rc;
  const int ch = (int)std::min<size_t>((size_t)height, std::max<size_t>(1, EU_ENCODE_CHUNK_BYTES / (in_row + out_row)));
  if (!frame_on_device) HIPCHK(cur().enc.frame.reserve((size_t)ch * width * 3));
  if (!out_on_device) HIPCHK(cur().enc.out.reserve((size_t)ch * width));
  drain drain_on_exit{ st, st };
  for (int y0 = 0; y0 < height; y0 += ch) {
    const int h = std::min(ch, height - y0);
    const char *fin = (const char *)frame + (size_t)y0 * frame_row_stride_bytes;
    char *fout = (char *)out + (size_t)y0 * out_row_stride_bytes;
    ep.src = (const float *)fin; ep.src_stride_bytes = frame_row_stride_bytes;
    ep.dst = (uint32_t *)fout; ep.dst_stride_bytes = out_row_stride_bytes;
    ep.h = h;
    if (!frame_on_device) {
      ep.src = cur().enc.frame.p; ep.src_stride_bytes = in_row;
      HIPCHK(hipMemcpy2DAsync(cur().enc.frame.p, in_row, fin, frame_row_stride_bytes, in_row, (size_t)h, hipMemcpyHostToDevice, st));
    }
    if (!out_on_device) { ep.dst = cur().enc.out.p; ep.dst_stride_bytes = out_row; }
    if (eu_launch_rgbe_encode(&ep, st)) return fail(EU_ERR_NO_DEVICE, "kernel launch failed");
    if (!out_on_device)
      HIPCHK(hipMemcpy2DAsync(fout, out_row_stride_bytes, cur().enc.out.p, out_row, out_row, (size_t)h, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  return EU_OK;
}

// the layout choice per segment of the (cropped) frame for this job: flags[k] = 1 where
// rows [k * seg_rows, (k + 1) * seg_rows) render faster - and cost about 1.55x the others -
// with the tile layout; returns the number of segments (0: no lat/lon source / no table)
int eu_hip_layout_segments(const eu_target *trg, eu_source *const *srcs, int nsrc,
                           unsigned char *flags, int max_flags, int *seg_rows)
{
  int rc;
  if ((rc = ensure_init())) return rc;
  if (!trg || !srcs || nsrc != 1 || !srcs[0] || !flags) return fail(EU_ERR_ARGUMENT, "one source, flags buffer");
  eu_render_params p;
  eu_target t = *trg;
  t.band_rows = 0; t.band_count = 0; t.band_index = 0;
  t.row_begin = 0; t.row_end = frame_h(trg);
  float dummy;
  if ((rc = build_params(&t, srcs, 1, &dummy, (size_t)frame_w(trg) * t.nchannels * sizeof(float), eu_read_switches(), &p))) return rc;
  if (seg_rows) *seg_rows = EU_SEG_ROWS;
  if (p.twine || p.norm_mode != EU_NORM_NONE || p.src.prj != EU_SPHERICAL) return 0;
  refresh_seg_flags(&p);
  const int n = (int)cur().plan.seg_flags.size();
  if (n > max_flags) return fail(EU_ERR_ARGUMENT, "flags buffer too small");
  memcpy(flags, cur().plan.seg_flags.data(), (size_t)n);
  return n;
}

// render kernel launches of this process so far (a render step of a big cubic job is
// several: launch-level layout choice); lets a benchmark report launches per step
unsigned long long eu_hip_launch_count(void) { return cur().launches; }

unsigned long long eu_hip_listed_tiles(void)
{
  // the last pair's set of counters stays as that pair left it until the next pair's second kernel empties it: the
  // lists' counters come to the host and are added up here (a diagnostic call; 64 KB). The event behind the pair is
  // the library's own (the caller's stream may be gone by now)
  if (!cur().staged.wl.p || cur().staged.last_set < 0 || !cur().staged.wl_pair.recorded ||
      cur().staged.wl_pair.host_wait() != hipSuccess)
    return 0;
  std::vector<int> h((size_t)EU4_WL_SHARD(EU4_SHARDS));
  if (hipMemcpy(h.data(), EU4_WL_SET(cur().staged.wl.p, cur().staged.last_set), h.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
    return 0;
  unsigned long long n = 0;
  for (int s = 0; s < EU4_SHARDS; s++) n += (unsigned long long)std::max(0, h[(size_t)EU4_WL_SHARD(s)]);
  return n;
}

int eu_hip_render_timed(const eu_target *trg, eu_source *const *srcs, int nsrc, float *out_dev,
                        size_t out_row_stride_bytes, int iters, float *mean_ms)
{
  int rc;
  if ((rc = ensure_init())) return rc;
  if (iters <= 0 || !mean_ms) return fail(EU_ERR_ARGUMENT, "bad iteration count");
  if (!srcs || nsrc < 1 || !trg || !out_dev) return fail(EU_ERR_ARGUMENT, "no source / no output");
  if ((rc = check_target(trg))) return rc;
  const eu_switches sw = eu_read_switches();
  // (the untimed launch builds the plan: stepper tables, derived copies)
  auto once = [&]() { return render_on_device(trg, srcs, nsrc, out_dev, out_row_stride_bytes, sw, cur().stream); };
  return time_on_stream(once, iters, mean_ms);
}

// DIAGNOSTIC (not declared in eu_hip.h): phase stamps of the headline path,
// 8 x uint64 per wave: t0..t5, XCC id, tile index
int eu_hip_diag_stamps(const eu_target *trg, eu_source *const *srcs, int nsrc, float *out_dev,
                       size_t out_row_stride_bytes, unsigned long long *host_stamps,
                       size_t nwaves)
{
  int rc;
  if ((rc = ensure_init())) return rc;
  eu_render_params p;
  if ((rc = build_params(trg, srcs, nsrc, out_dev, out_row_stride_bytes, eu_read_switches(), &p))) return rc;
  if (p.nch != 3 || p.src.degree != 3 || p.twine) return fail(EU_ERR_ARGUMENT, "diag: NCH 3, degree 3, no twining");
  eu_dev_tmp<unsigned long long> d;
  HIPCHK(d.alloc(nwaves * 8));
  HIPCHK(hipMemsetAsync(d.p, 0, nwaves * 8 * sizeof(unsigned long long), cur().stream));
  for (int i = 0; i < 3; i++)
    if (eu_launch_diag(&p, d.p, cur().stream)) return fail(EU_ERR_NO_DEVICE, "diag launch failed");
  HIPCHK(hipStreamSynchronize(cur().stream));
  HIPCHK(hipMemcpy(host_stamps, d.p, nwaves * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return EU_OK;
}

}  // extern "C"
