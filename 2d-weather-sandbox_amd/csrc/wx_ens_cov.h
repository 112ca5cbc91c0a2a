// wx_ens_cov.h -- covariance, correlation and sensitivity maps over the members of an ensemble on the device (include/wxsim.h: wx_ens_cov,
// wx_ens_cov_pred, wx_ensemble_covariance, wx_ens_cov_cells): for every cell-channel of a rectangle the sample covariance between the
// members' values and up to WX_ENS_COV_MAX scalar predictors, in ONE pass over the members for all of them, defined bit for bit by
// wx_ens_cov_cell.h. Included at the end of wxsim.hip behind wx_ens_inflate.h (the entry points are declared extern "C" by
// include/wxsim.h). Two launches, nothing written but the ensemble's own output buffer.
//
// k_ens_cov_pred (one workgroup, one wave per predictor slot). The predictor table e[j][k] of doubles arrives holding t_k for the
// VALUES predictors (the host uploads them). Wave j's lanes gather a POINT predictor's t_k through the member table (NaN where the cell
// is a wall cell in that member: "not finite" then means "invalid"), a workgroup barrier orders those stores, and lane 0 of the wave runs
// wxc::pred_of -- the serial chain of the definition -- over row j in place: e_k = t_k - jm, the result, and the header {valid, Qj} the
// map kernel reads. Rows of e past n_pred (the template bucket's padding) become zeros; they get no header. The table is read and written through
// ordinary global pointers here: it changes during the launch.
//
// k_ens_cov<SOURCE, NP>. k_ens_inflate's shape: one lane per cell of the rectangle, a wave takes 64 consecutive x of one row, waves
// grid-stride over the (row, chunk) pairs with a capped grid. Walk 1: Sx and the entry test (16 B field or snapshot + 4 B wall). A cell
// none of whose channels is eligible stores its NaNs and ends there. Walk 2: Qx and the NP Cq_j (16 B, the same lines again: L2, one expects). Each
// walk has the loads of UNROLL members issued before the first is consumed -- written out here, not wxe::member_walk: through the
// template four instantiations need more registers and one is slower ("One member walk") --; the member table, the headers and e[j][k] are read at
// wave-uniform addresses through the constant address space (scalar loads; the pre-pass wrote them in an EARLIER launch). Only the
// wanted planes are stored, 16 B per lane. No LDS, no atomics, no device-side waiting. The template on the source keeps the snapshot
// address arithmetic out of CURRENT; the template on the bucket NP = 1 / 2 / 4 / 8 of n_pred sizes the accumulators (4 NP doubles):
// DESIGN.md section 4 has each instantiation's registers. What it does not try: holding the members of a small ensemble in registers
// across the two walks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/wxsim.h"
#include "wx_ens_frame.h"
#include "wx_ens_inflate.h"
#include "wx_ens_cov_cell.h"

namespace wxc {

// one predictor as the map kernel reads it (the pre-pass writes it)
struct PredHdr {
  int32_t valid, pad;
  double Q;
};
struct DevPred {
  int32_t kind, field, x, y, channel;
};

// the predictor table: the head of the ensemble's output buffer, every part 8-byte aligned; NP rows of e (the bucket, not n_pred)
struct Table {
  double *e;               // NP x n_sel
  wx_ens_cov_result *res;  // WX_ENS_COV_MAX
  PredHdr *hdr;            // WX_ENS_COV_MAX
};
inline size_t table_layout(int np, int n_sel, size_t at[3])
{
  const size_t bytes[3] = {8 * (size_t)np * (size_t)n_sel, sizeof(wx_ens_cov_result) * WX_ENS_COV_MAX, sizeof(PredHdr) * WX_ENS_COV_MAX};
  size_t total = 0;
  for (int i = 0; i < 3; i++) at[i] = total, total += (bytes[i] + 15) & ~(size_t)15;
  return total;
}
inline int bucket_of(int n_pred) { return n_pred <= 1 ? 1 : n_pred <= 2 ? 2 : n_pred <= 4 ? 4 : 8; }

struct PredArgs {
  int X, n_sel, n_pred, np;
  DevPred pred[WX_ENS_COV_MAX];
  const wxe::Member *tab; // 2 n_sel entries: the members' base fields, then their water fields
  Table t;
};

struct Args {
  int X;
  int x0, y0, w, h;
  int n_sel, n_pred;
  const wxe::Member *tab; // n_sel entries of the field (CURRENT: read; PRIOR: only their walls are)
  const float4 *prior;    // the snapshot [n_sel][ph][pw] of the rectangle (px0, py0, pw, ph); CURRENT: not looked at
  int px0, py0, pw, ph;
  const double *e;
  const PredHdr *hdr;
  float4 *cov, *corr, *slope; // n_pred planes of w * h texels each, or nullptr
  float4 *variance;           // w * h texels, or nullptr
};

enum { WG = 256, WAVES = WG / 64, MAX_WGS = 2048, UNROLL = 8, PRED_WG = 64 * WX_ENS_COV_MAX };

#if defined(__HIPCC__)
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) PredHdr *CHdr;
typedef const __attribute__((address_space(4))) double *CE;
__device__ __forceinline__ CHdr const_hdr(const PredHdr *h) { return (CHdr)(unsigned long long)h; }
__device__ __forceinline__ CE const_e(const double *e) { return (CE)(unsigned long long)e; }
#else // host pass of the single-source compile: same meaning, never executed
typedef const PredHdr *CHdr;
typedef const double *CE;
__device__ __forceinline__ CHdr const_hdr(const PredHdr *h) { return h; }
__device__ __forceinline__ CE const_e(const double *e) { return e; }
#endif

__global__ __launch_bounds__(PRED_WG) void k_ens_cov_pred(const PredArgs a)
{
  const unsigned lane = threadIdx.x & 63u, j = threadIdx.x >> 6; // wave j takes predictor slot j
  const unsigned n = (unsigned)a.n_sel;
  const wxe::CTab tab = wxe::const_table(a.tab);
  const bool row = j < (unsigned)a.np, live = j < (unsigned)a.n_pred;
  double *t = a.t.e + (size_t)j * n; // (looked at only where `row`)
  // 1. a point's values through the member table; a padding row is zeros; a VALUES row is there already
  if (row && (!live || a.pred[j].kind == WX_COV_PRED_POINT)) {
    const DevPred q = a.pred[live ? j : 0];
    const size_t off = (size_t)q.y * (size_t)a.X + (size_t)q.x;
    for (unsigned k = lane; k < n; k += 64u) {
      double v = 0.0;
      if (live) {
        const wxe::CTab m = tab + (q.field == WX_FIELD_BASE_CUR ? 0u : n) + k;
        const float f = wxq::ld_chan(m, off, (unsigned)q.channel);
        v = wxe::ld_wall_dist(m, off) != 0 ? (double)f : f64_nan();
      }
      t[k] = v;
    }
  }
  __threadfence_block();
  __syncthreads();
  // 2. the chain, serial in member order by definition: one lane per predictor
  if (lane == 0 && live) { // (the results and headers of unused slots are read by nobody)
    const Pred p = pred_of((int)n, t, t);
    result_of(a.t.res[j], p, (int)n);
    a.t.hdr[j].valid = p.valid ? 1 : 0, a.t.hdr[j].pad = 0, a.t.hdr[j].Q = p.Q;
  }
}

template <int SOURCE, int NP>
__global__ __launch_bounds__(WG) void k_ens_cov(const Args a)
{
  constexpr bool PRIOR = SOURCE == WX_COV_SOURCE_PRIOR;
  const wxe::WaveOfGrid wg = wxe::wave_of_grid(WAVES);
  const unsigned chunks = wxe::chunks_per_row(a.w) * (unsigned)a.h;
  const wxe::CTab tab = wxe::const_table(a.tab);
  const CHdr hdr = const_hdr(a.hdr);
  const CE e = const_e(a.e);
  const int n = a.n_sel;
  const size_t pstride = PRIOR ? (size_t)a.pw * (size_t)a.ph : 0; // texels per member of the snapshot
  const size_t plane = (size_t)a.w * (size_t)a.h;
  const float nanf = __builtin_nanf("");
  for (unsigned ch = wg.wave; ch < chunks; ch += wg.n_waves) {
    const wxe::Chunk at = wxe::chunk_at(ch, wg.lane, a.x0, a.y0, a.w);
    if (!at.valid) continue;
    const size_t off = wxe::texel_at(a.X, at.gx, at.gy), o = wxe::plane_at(a.w, at.x, at.y);
    const size_t poff = PRIOR ? (size_t)(at.gy - a.py0) * (size_t)a.pw + (size_t)(at.gx - a.px0) : 0;
    const auto ld_x = [&](int k) { return PRIOR ? wxi::ld_prior(a.prior, (size_t)k * pstride + poff) : wxe::ld_field(tab + k, off); };
    // walk 1: Sx and the entry test
    double S[4] = {0.0, 0.0, 0.0, 0.0};
    bool ok[4] = {true, true, true, true};
    int k = 0;
    for (; k + UNROLL <= n; k += UNROLL) { // the loads of UNROLL members are issued before the first of them is consumed
      wxe::f32x4 v[UNROLL];
      int wd[UNROLL];
#pragma unroll
      for (int i = 0; i < UNROLL; i++) v[i] = ld_x(k + i), wd[i] = wxe::ld_wall_dist(tab + k + i, off);
      WX_ENS_LOADS_ISSUED();
#pragma unroll
      for (int i = 0; i < UNROLL; i++) {
        const bool air = wd[i] != 0;
        sum_add(S[0], ok[0], v[i].x, air), sum_add(S[1], ok[1], v[i].y, air), sum_add(S[2], ok[2], v[i].z, air), sum_add(S[3], ok[3], v[i].w, air);
      }
    }
    for (; k < n; k++) {
      const wxe::f32x4 v = ld_x(k);
      const bool air = wxe::ld_wall_dist(tab + k, off) != 0;
      sum_add(S[0], ok[0], v.x, air), sum_add(S[1], ok[1], v.y, air), sum_add(S[2], ok[2], v.z, air), sum_add(S[3], ok[3], v.w, air);
    }
    wxe::f32x4 o_var = {nanf, nanf, nanf, nanf};
    if (!(ok[0] || ok[1] || ok[2] || ok[3])) { // nothing eligible: the NaNs, and no second walk
      if (a.variance) wxi::st_texel(a.variance, o, o_var);
      for (int j = 0; j < a.n_pred; j++) {
        if (a.cov) wxi::st_texel(a.cov, (size_t)j * plane + o, o_var);
        if (a.corr) wxi::st_texel(a.corr, (size_t)j * plane + o, o_var);
        if (a.slope) wxi::st_texel(a.slope, (size_t)j * plane + o, o_var);
      }
      continue;
    }
    double xm[4];
#pragma unroll
    for (int c = 0; c < 4; c++) xm[c] = S[c] / (double)n;
    // walk 2: Qx and the Cq_j from the same d_k
    double Qx[4] = {0.0, 0.0, 0.0, 0.0}, Cq[NP][4];
#pragma unroll
    for (int j = 0; j < NP; j++) Cq[j][0] = Cq[j][1] = Cq[j][2] = Cq[j][3] = 0.0;
    auto take = [&](int m, const wxe::f32x4 v) {
      const double d[4] = {dev_of(v.x, xm[0]), dev_of(v.y, xm[1]), dev_of(v.z, xm[2]), dev_of(v.w, xm[3])};
      q_add(Qx[0], d[0]), q_add(Qx[1], d[1]), q_add(Qx[2], d[2]), q_add(Qx[3], d[3]);
#pragma unroll
      for (int j = 0; j < NP; j++) {
        const double ek = e[(size_t)j * (size_t)n + (size_t)m];
        c_add(Cq[j][0], d[0], ek), c_add(Cq[j][1], d[1], ek), c_add(Cq[j][2], d[2], ek), c_add(Cq[j][3], d[3], ek);
      }
    };
    for (k = 0; k + UNROLL <= n; k += UNROLL) {
      wxe::f32x4 v[UNROLL];
#pragma unroll
      for (int i = 0; i < UNROLL; i++) v[i] = ld_x(k + i);
      WX_ENS_LOADS_ISSUED();
#pragma unroll
      for (int i = 0; i < UNROLL; i++) take(k + i, v[i]);
    }
    for (; k < n; k++) take(k, ld_x(k));
    if (a.variance) {
      o_var.x = ok[0] ? variance_of(Qx[0], n) : nanf, o_var.y = ok[1] ? variance_of(Qx[1], n) : nanf;
      o_var.z = ok[2] ? variance_of(Qx[2], n) : nanf, o_var.w = ok[3] ? variance_of(Qx[3], n) : nanf;
      wxi::st_texel(a.variance, o, o_var);
    }
#pragma unroll
    for (int j = 0; j < NP; j++) {
      if (j >= a.n_pred) break; // (uniform)
      const bool valid = hdr[j].valid != 0;
      const double Qj = hdr[j].Q;
      const size_t at = (size_t)j * plane + o;
      wxe::f32x4 r;
      if (a.cov) {
        r.x = valid && ok[0] ? cov_of(Cq[j][0], n) : nanf, r.y = valid && ok[1] ? cov_of(Cq[j][1], n) : nanf;
        r.z = valid && ok[2] ? cov_of(Cq[j][2], n) : nanf, r.w = valid && ok[3] ? cov_of(Cq[j][3], n) : nanf;
        wxi::st_texel(a.cov, at, r);
      }
      if (a.corr) {
        r.x = valid && ok[0] ? corr_of(Cq[j][0], Qx[0], Qj) : nanf, r.y = valid && ok[1] ? corr_of(Cq[j][1], Qx[1], Qj) : nanf;
        r.z = valid && ok[2] ? corr_of(Cq[j][2], Qx[2], Qj) : nanf, r.w = valid && ok[3] ? corr_of(Cq[j][3], Qx[3], Qj) : nanf;
        wxi::st_texel(a.corr, at, r);
      }
      if (a.slope) {
        r.x = valid && ok[0] ? slope_of(Cq[j][0], Qx[0]) : nanf, r.y = valid && ok[1] ? slope_of(Cq[j][1], Qx[1]) : nanf;
        r.z = valid && ok[2] ? slope_of(Cq[j][2], Qx[2]) : nanf, r.w = valid && ok[3] ? slope_of(Cq[j][3], Qx[3]) : nanf;
        wxi::st_texel(a.slope, at, r);
      }
    }
  }
}

template <int SOURCE>
static void launch_cov(int np, unsigned wgs, hipStream_t stream, const Args &a)
{
  if (np == 1) hipLaunchKernelGGL((k_ens_cov<SOURCE, 1>), dim3(wgs), dim3(WG), 0, stream, a);
  else if (np == 2) hipLaunchKernelGGL((k_ens_cov<SOURCE, 2>), dim3(wgs), dim3(WG), 0, stream, a);
  else if (np == 4) hipLaunchKernelGGL((k_ens_cov<SOURCE, 4>), dim3(wgs), dim3(WG), 0, stream, a);
  else hipLaunchKernelGGL((k_ens_cov<SOURCE, 8>), dim3(wgs), dim3(WG), 0, stream, a);
}
#endif // __HIPCC__

} // namespace wxc

int wx_ens_cov_cells(const wx_ens_cov *c, const wx_ens_cov_pred *pred, wx_ens_cov_result *result, int X, int Y, int n_members, const float *const *base,
                     const float *const *water, const int8_t *const *wall, const float *const *prior, const uint8_t *member_mask)
{
  return wxc::cov_cells(c, pred, result, X, Y, n_members, base, water, wall, prior, member_mask);
}

int wx_ensemble_covariance(wx_ensemble *e, const wx_ens_cov *c, const wx_ens_cov_pred *pred, wx_ens_cov_result *result, const uint8_t *member_mask)
{
  static const char *const call = "wx_ensemble_covariance";
  if (!e || !c || !pred) return WX_E_INVALID;
  // the arguments first: nothing below this block is reached with a bad one, and nothing in it touches the device
  const char *why;
  if (int rc = wxc::check_desc(c, pred, &why)) return efail(e, rc, "wx_ensemble_covariance: %s", why);
  const std::vector<int> sel = ens_select(e, member_mask);
  if (sel.size() < 2) return efail(e, WX_E_INVALID, "wx_ensemble_covariance: the member mask selects %zu member(s); a sample covariance takes two", sel.size());
  if (int rc = wxc::check_values(c, pred, sel, &why)) return efail(e, rc, "wx_ensemble_covariance: %s", why);
  if (int rc = wxc::check_rect(c, pred, e->X, e->Y, &why)) return efail(e, rc, "wx_ensemble_covariance: %s", why);
  if (int rc = ens_require_uploaded(e, call, sel)) return rc;
  const bool from_prior = c->source == WX_COV_SOURCE_PRIOR;
  const EnsPriorSlot *snap = nullptr;
  if (from_prior)
    if (int rc = ens_snapshot_for(e, call, c->field, member_mask, c->x, c->y, c->w, c->h, &snap)) return rc;

  const int n = (int)sel.size(), n_pred = c->n_pred, np = wxc::bucket_of(n_pred);
  const size_t plane = (size_t)c->w * (size_t)c->h * sizeof(float4);
  // the output buffer: the predictor table, then the wanted planes back to back (cov, corr, slope: n_pred each; variance)
  float *const want[4] = {c->cov, c->corr, c->slope, c->variance};
  size_t tat[3], at[4];
  const size_t table_bytes = wxc::table_layout(np, n, tat);
  size_t total = table_bytes;
  for (int i = 0; i < 4; i++) {
    at[i] = total;
    if (want[i]) total += plane * (size_t)(i < 3 ? n_pred : 1);
  }
  EnsCall frame(e, call, K_ENS_COV_PRED);
  if (int rc = ens_begin(frame, 2 * n, total)) return rc;
  EnsStage *st = frame.st;
  // the host's numbers, by position among the selected members; the other rows are the pre-pass's
  double *e_host = (double *)(st->out_host + tat[0]);
  memset(e_host, 0, 8 * (size_t)np * (size_t)n);
  for (int j = 0; j < n_pred; j++)
    if (pred[j].kind == WX_COV_PRED_VALUES)
      for (int k = 0; k < n; k++) e_host[(size_t)j * (size_t)n + (size_t)k] = pred[j].values[sel[k]];

  wxc::PredArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.X = e->X, pa.n_sel = n, pa.n_pred = n_pred, pa.np = np, pa.tab = st->tab_dev;
  for (int j = 0; j < n_pred; j++) pa.pred[j] = wxc::DevPred{pred[j].kind, pred[j].field, pred[j].x, pred[j].y, pred[j].channel};
  pa.t.e = (double *)(st->out_dev + tat[0]), pa.t.res = (wx_ens_cov_result *)(st->out_dev + tat[1]), pa.t.hdr = (wxc::PredHdr *)(st->out_dev + tat[2]);

  wxc::Args a;
  memset(&a, 0, sizeof(a));
  a.X = e->X, a.x0 = c->x, a.y0 = c->y, a.w = c->w, a.h = c->h, a.n_sel = n, a.n_pred = n_pred;
  a.tab = st->tab_dev + (c->field == WX_FIELD_BASE_CUR ? 0 : n);
  if (from_prior) a.prior = snap->buf, a.px0 = snap->x, a.py0 = snap->y, a.pw = snap->w, a.ph = snap->h;
  a.e = pa.t.e, a.hdr = pa.t.hdr;
  a.cov = want[0] ? (float4 *)(st->out_dev + at[0]) : nullptr, a.corr = want[1] ? (float4 *)(st->out_dev + at[1]) : nullptr;
  a.slope = want[2] ? (float4 *)(st->out_dev + at[2]) : nullptr, a.variance = want[3] ? (float4 *)(st->out_dev + at[3]) : nullptr;

  // table and host values, the pre-pass, the maps, results and planes to the pinned copy
  ens_table_base_water(frame, sel);
  if (frame.he == hipSuccess) frame.he = hipMemcpyAsync(pa.t.e, e_host, 8 * (size_t)np * (size_t)n, hipMemcpyHostToDevice, e->stream);
  ens_launch(frame, K_ENS_COV_PRED, [&] { hipLaunchKernelGGL(wxc::k_ens_cov_pred, dim3(1), dim3(wxc::PRED_WG), 0, e->stream, pa); });
  const unsigned wgs = ens_wgs_wave_per_item(ens_chunks(c->w, c->h), wxc::WAVES, wxc::MAX_WGS);
  ens_launch(frame, K_ENS_COV, [&] {
    if (from_prior) wxc::launch_cov<WX_COV_SOURCE_PRIOR>(np, wgs, e->stream, a);
    else wxc::launch_cov<WX_COV_SOURCE_CURRENT>(np, wgs, e->stream, a);
  });
  // (the e rows are not wanted back: the copy starts at the results)
  if (frame.he == hipSuccess) frame.he = hipMemcpyAsync(st->out_host + tat[1], st->out_dev + tat[1], total - tat[1], hipMemcpyDeviceToHost, e->stream);
  if (int rc = ens_finish(frame)) return rc;
  if (result) memcpy(result, st->out_host + tat[1], sizeof(wx_ens_cov_result) * (size_t)n_pred);
  for (int i = 0; i < 4; i++)
    if (want[i]) memcpy(want[i], st->out_host + at[i], plane * (size_t)(i < 3 ? n_pred : 1));
  return WX_OK;
}
