// wx_ens_assim.h -- point observations assimilated into the members of an ensemble on the device (include/wxsim.h: wx_ens_assim,
// wx_ens_obs, wx_ensemble_assimilate, wx_ens_assim_cells): a serial ensemble square-root filter with separable Gaspari-Cohn
// localization, defined bit for bit by wx_ens_assim_cell.h, in THREE launches at most whatever the number of observations. Included at
// the end of wxsim.hip behind wx_ens_quant.h (the entry points are declared extern "C" by include/wxsim.h).
//
// The serial definition makes observation j see the state observations 0 .. j-1 left. For a POINT observation the only state its prior
// reads is the observed channel of the observed cell, and that cell evolves by the per-cell function alone (cells never interact within
// one observation). So the whole chain of priors can be computed in observation space first:
//
// k_ens_assim_obs (one workgroup of one wave). A working copy W[j][k] of every observation's observed channel in every selected member
// is gathered (lanes over (j, k)), and whether the observation is usable (air cell and finite value in every member: neither changes
// under the filter; W lives in LDS where it fits 64 KiB -- 256 observations x 64 members --, else in the table). Then for j = 0 .. n_obs-1: every lane computes observation j's header from W[j] (redundantly: the sums are serial
// in k by definition, and a header in registers needs no hand-off), the lanes write e(j)[k] = W[j][k] - hm and lane 0 the header to the
// observation table, and the lanes take the later usable observations j' > j that lie inside the rectangle and apply wxa::update_channel
// -- the function the state update is made of -- to W[j'] with the gain and the clamp of j''s own field and channel. W[j'] is then what
// the state's cell will hold after observation j: two observations of one cell and channel keep two equal copies. A workgroup barrier
// (which orders the wave's global stores and loads) follows every j. Bounded loops, no grid barrier, no spin-wait. The table is read
// and written through ordinary global pointers here: it changes during the launch, so nothing of it may come through the scalar cache.
//
// k_ens_assim (one launch per state field with a non-zero gain). One lane per cell of the rectangle, a wave takes 64 consecutive x of
// one row, waves grid-stride over the (row, chunk) pairs with a capped grid -- k_ens_stat's shape. Per cell the observations in order;
// an observation that was not applied, whose row weight is 0 (wave-uniform, tested first) or whose rho is 0 in this lane is skipped.
// Otherwise three walks over the members (wxe::member_walk), as the definition says: Sx and the entry test; Cq; the write -- the member table, the headers and e(j) read at wave-uniform addresses through the constant
// address space (scalar loads; the pre-pass wrote them in an EARLIER launch), and 16-byte stores in place, only of texels whose bits
// change. The lane re-reads its own stores for the next observation: same thread, same address, program order. 20 B read three times
// and 16 B written per member-cell and observation in range, at most.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/wxsim.h"
#include "wx_ens_frame.h"
#include "wx_ens_perturb.h"
#include "wx_ens_assim_cell.h"

namespace wxa {

// one observation as the update kernel reads it (the pre-pass writes it)
struct ObsHdr {
  int32_t applied, x, y, pad;
  Prior p;
};

// the observation table: one device buffer, every part 8-byte aligned
struct Table {
  wx_ens_obs *obs;          // n_obs, as the caller gave them
  wx_ens_obs_result *res;   // n_obs, what goes back to the caller
  ObsHdr *hdr;              // n_obs
  double *e;                // n_obs x n_sel: e(j)[k]
  float *W;                 // n_obs x n_sel: the pre-pass's working copies
};
inline size_t table_layout(int n_obs, int n_sel, size_t at[5])
{
  const size_t bytes[5] = {sizeof(wx_ens_obs) * (size_t)n_obs, sizeof(wx_ens_obs_result) * (size_t)n_obs, sizeof(ObsHdr) * (size_t)n_obs,
                           8 * (size_t)n_obs * (size_t)n_sel, 4 * (size_t)n_obs * (size_t)n_sel};
  size_t total = 0;
  for (int i = 0; i < 5; i++) at[i] = total, total += (bytes[i] + 7) & ~(size_t)7;
  return total;
}

struct ObsArgs {
  int X, n_sel, n_obs;
  int w_in_lds; // the working copies fit the workgroup's LDS (n_obs * n_sel floats <= OBS_LDS_BYTES): W is there, t.W is not used
  wx_ens_assim a;
  const wxe::Member *tab; // 2 n_sel entries: the members' base fields, then their water fields
  Table t;
};

struct Args {
  int X;
  int x0, y0, w, h;
  int n_sel, n_obs;
  Loc loc;
  float gain[4], lo[4], hi[4]; // of this launch's field
  const wxe::Member *tab;      // n_sel entries of this launch's field (written in place)
  const ObsHdr *hdr;
  const double *e;
};

enum { WG = 256, WAVES = WG / 64, MAX_WGS = 2048, UNROLL = 8, OBS_WG = 64, OBS_LDS_BYTES = 65536 };

#if defined(__HIPCC__)
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) ObsHdr *CHdr;
typedef const __attribute__((address_space(4))) double *CE;
__device__ __forceinline__ CHdr const_hdr(const ObsHdr *h) { return (CHdr)(unsigned long long)h; }
__device__ __forceinline__ CE const_e(const double *e) { return (CE)(unsigned long long)e; }
#else // host pass of the single-source compile: same meaning, never executed
typedef const ObsHdr *CHdr;
typedef const double *CE;
__device__ __forceinline__ CHdr const_hdr(const ObsHdr *h) { return h; }
__device__ __forceinline__ CE const_e(const double *e) { return e; }
#endif

__global__ __launch_bounds__(OBS_WG) void k_ens_assim_obs(const ObsArgs a)
{
  const unsigned lane = threadIdx.x;
  const unsigned n = (unsigned)a.n_sel, n_obs = (unsigned)a.n_obs;
  const wxe::CTab tab = wxe::const_table(a.tab);
  const Loc loc{a.X, a.a.wrap_x ? 1 : 0, a.a.loc_x, a.a.loc_y};
  const wx_ens_obs *obs = a.t.obs;
  ObsHdr *hdr = a.t.hdr;
  extern __shared__ float wxa_lds[];
  float *W = a.w_in_lds ? wxa_lds : a.t.W; // (every pass over W is a chain of dependent loads: LDS latency where it fits, e.g. 256 x 64)
  // 1a. the working copies: lanes over (j, k)
  for (unsigned i = lane; i < n_obs * n; i += OBS_WG) {
    const unsigned j = i / n, k = i - j * n;
    const wx_ens_obs o = obs[j];
    const size_t off = (size_t)o.y * (size_t)a.X + (size_t)o.x;
    W[i] = wxq::ld_chan(tab + (o.field == WX_FIELD_BASE_CUR ? 0u : n) + k, off, (unsigned)o.channel);
  }
  __syncthreads();
  // 1b. usable: lanes over j
  for (unsigned j = lane; j < n_obs; j += OBS_WG) {
    const wx_ens_obs o = obs[j];
    const size_t off = (size_t)o.y * (size_t)a.X + (size_t)o.x;
    bool ok = true;
    for (unsigned k = 0; k < n; k++) ok = ok && wxe::ld_wall_dist(tab + k, off) != 0 && f32_finite(W[j * n + k]);
    hdr[j].applied = ok ? 1 : 0, hdr[j].x = o.x, hdr[j].y = o.y, hdr[j].pad = 0;
  }
  // 2. the observations in order (every condition that skips a barrier-free stretch is workgroup-uniform; the barrier is at the top)
  for (unsigned j = 0; j < n_obs; j++) {
    __syncthreads();
    const wx_ens_obs o = obs[j];
    if (!hdr[j].applied) {
      if (lane == 0) result_skipped(a.t.res[j]);
      continue;
    }
    const float *t = W + (size_t)j * n;
    const Prior p = prior_of((int)n, t, o.value, o.error_var);
    for (unsigned k = lane; k < n; k += OBS_WG) a.t.e[(size_t)j * n + k] = (double)t[k] - p.hm;
    if (lane == 0) {
      hdr[j].p = p;
      result_applied(a.t.res[j], p);
    }
    for (unsigned jp = j + 1u + lane; jp < n_obs; jp += OBS_WG) {
      if (!hdr[jp].applied) continue;
      const wx_ens_obs op = obs[jp];
      if (!in_rect(a.a, op.x, op.y)) continue;
      const bool is_base = op.field == WX_FIELD_BASE_CUR;
      const float g = (is_base ? a.a.gain_base : a.a.gain_water)[op.channel];
      if (g == 0.0f) continue;
      const double rho = rho_of(loc, op.x, op.y, o.x, o.y);
      if (rho == 0.0) continue;
      update_channel((int)n, W + (size_t)jp * n, t, p, (double)g * rho, (is_base ? a.a.lo_base : a.a.lo_water)[op.channel],
                     (is_base ? a.a.hi_base : a.a.hi_water)[op.channel]);
    }
  }
}

// what pass 1 and pass 2 accumulate
struct Sum4 {
  double S[4];
  bool ok[4];
};
struct Cov4 {
  double Cq[4];
};

__global__ __launch_bounds__(WG) void k_ens_assim(const Args a)
{
  const wxe::WaveOfGrid wg = wxe::wave_of_grid(WAVES);
  const unsigned chunks = wxe::chunks_per_row(a.w) * (unsigned)a.h;
  const wxe::CTab tab = wxe::const_table(a.tab);
  const CHdr hdr = const_hdr(a.hdr);
  const int n = a.n_sel;
  for (unsigned ch = wg.wave; ch < chunks; ch += wg.n_waves) {
    const wxe::Chunk at = wxe::chunk_at(ch, wg.lane, a.x0, a.y0, a.w);
    if (!at.valid) continue;
    const int gx = at.gx, gy = at.gy;
    const size_t off = wxe::texel_at(a.X, gx, gy);
    const auto load = [&](int k) { return wxe::ld_field(tab + k, off); };
    const auto load_wall = [&](int k) { return wxe::ld_field_wall(tab + k, off); };
    for (int j = 0; j < a.n_obs; j++) {
      if (!hdr[j].applied) continue; // (uniform)
      const double wy = axis_weight(dist_y(gy, hdr[j].y), a.loc.loc_y);
      if (wy == 0.0) continue; // (uniform: a wave is one row)
      const double rho = axis_weight(dist_x(a.loc, gx, hdr[j].x), a.loc.loc_x) * wy;
      if (rho == 0.0) continue;
      Prior p;
      p.hm = hdr[j].p.hm, p.V = hdr[j].p.V, p.D = hdr[j].p.D, p.innovation = hdr[j].p.innovation, p.alpha = hdr[j].p.alpha;
      const CE e = const_e(a.e) + (size_t)j * (size_t)n;
      // pass 1: Sx and the entry test
      const Sum4 s = wxe::member_walk<UNROLL>(n, Sum4{{0.0, 0.0, 0.0, 0.0}, {true, true, true, true}}, load_wall, [](Sum4 &q, int, const wxe::TexelWall &m) {
        const bool air = m.wd != 0;
        sum_add(q.S[0], q.ok[0], m.v.x, air), sum_add(q.S[1], q.ok[1], m.v.y, air), sum_add(q.S[2], q.ok[2], m.v.z, air), sum_add(q.S[3], q.ok[3], m.v.w, air);
      });
      double xm[4];
      bool ok[4], any = false;
#pragma unroll
      for (int c = 0; c < 4; c++) {
        ok[c] = s.ok[c] && a.gain[c] != 0.0f;
        xm[c] = s.S[c] / (double)n;
        any = any || ok[c];
      }
      if (!any) continue;
      // pass 2: Cq
      const Cov4 cq = wxe::member_walk<UNROLL>(n, Cov4{{0.0, 0.0, 0.0, 0.0}}, load, [&](Cov4 &q, int k, const wxe::f32x4 &v) {
        const double ek = e[k];
        cov_add(q.Cq[0], v.x, xm[0], ek), cov_add(q.Cq[1], v.y, xm[1], ek), cov_add(q.Cq[2], v.z, xm[2], ek), cov_add(q.Cq[3], v.w, xm[3], ek);
      });
      Gain g[4];
      any = false;
#pragma unroll
      for (int c = 0; c < 4; c++) {
        g[c] = gain_of(ok[c], cq.Cq[c], n, (double)a.gain[c] * rho, p);
        any = any || g[c].on;
      }
      if (!any) continue;
      // pass 3: the write; a texel whose bits do not change is not stored
      wxe::member_walk<UNROLL>(n, wxe::Nothing{}, load, [&](wxe::Nothing &, int k, const wxe::f32x4 &v) {
        const double ek = e[k];
        wxe::f32x4 o;
        o.x = g[0].on ? post_value(v.x, g[0], ek, a.lo[0], a.hi[0]) : v.x;
        o.y = g[1].on ? post_value(v.y, g[1], ek, a.lo[1], a.hi[1]) : v.y;
        o.z = g[2].on ? post_value(v.z, g[2], ek, a.lo[2], a.hi[2]) : v.z;
        o.w = g[3].on ? post_value(v.w, g[3], ek, a.lo[3], a.hi[3]) : v.w;
        if (wxcell::texel_changed(o, v)) wxp::st_field(tab + k, off, o);
      });
    }
  }
}
#endif // __HIPCC__

} // namespace wxa

int wx_ens_assim_cells(const wx_ens_assim *a, int n_obs, const wx_ens_obs *obs, wx_ens_obs_result *result, int X, int Y, int n_members,
                       float *const *base, float *const *water, const int8_t *const *wall, const uint8_t *member_mask)
{
  return wxa::assim_cells(a, n_obs, obs, result, X, Y, n_members, base, water, wall, member_mask);
}

int wx_ensemble_assimilate(wx_ensemble *e, const wx_ens_assim *a, int n_obs, const wx_ens_obs *obs, wx_ens_obs_result *result, const uint8_t *member_mask)
{
  static const char *const call = "wx_ensemble_assimilate";
  if (!e || !a || !obs) return WX_E_INVALID;
  // the arguments first: nothing below this block is reached with a bad one, and nothing in it touches the device
  const char *why;
  if (int rc = wxa::check_desc(a, n_obs, obs, e->X, e->Y, &why)) return efail(e, rc, "wx_ensemble_assimilate: %s", why);
  const std::vector<int> sel = ens_select(e, member_mask);
  if (sel.size() < 2) return efail(e, WX_E_INVALID, "wx_ensemble_assimilate: the member mask selects %zu member(s); a sample variance takes two", sel.size());
  if (int rc = ens_require_uploaded(e, call, sel)) return rc;

  const int n = (int)sel.size();
  size_t at[5];
  const size_t total = wxa::table_layout(n_obs, n, at);
  EnsCall c(e, call, K_ENS_ASSIM_OBS);
  if (int rc = ens_begin(c, 2 * n, total)) return rc;
  EnsStage *st = c.st;
  bool update[2] = {false, false}; // base, water
  for (int ch = 0; ch < 4; ch++) update[0] = update[0] || a->gain_base[ch] != 0.0f, update[1] = update[1] || a->gain_water[ch] != 0.0f;
  for (int i : sel) {
    if (update[0])
      if (int rc = epass(e, i, ens_perturb_prepare(e->member[i], WX_FIELD_BASE_CUR))) return rc;
    if (update[1])
      if (int rc = epass(e, i, ens_perturb_prepare(e->member[i], WX_FIELD_WATER_CUR))) return rc;
  }
  memcpy(st->out_host + at[0], obs, sizeof(wx_ens_obs) * (size_t)n_obs);

  wxa::ObsArgs oa;
  memset(&oa, 0, sizeof(oa));
  oa.X = e->X, oa.n_sel = n, oa.n_obs = n_obs, oa.a = *a, oa.tab = st->tab_dev;
  oa.t.obs = (wx_ens_obs *)(st->out_dev + at[0]), oa.t.res = (wx_ens_obs_result *)(st->out_dev + at[1]);
  oa.t.hdr = (wxa::ObsHdr *)(st->out_dev + at[2]), oa.t.e = (double *)(st->out_dev + at[3]), oa.t.W = (float *)(st->out_dev + at[4]);
  const size_t w_bytes = 4 * (size_t)n_obs * (size_t)n;
  oa.w_in_lds = w_bytes <= wxa::OBS_LDS_BYTES ? 1 : 0;

  // table and observations, the pre-pass, the update launches, the results
  ens_table_base_water(c, sel);
  if (c.he == hipSuccess) c.he = hipMemcpyAsync(oa.t.obs, st->out_host + at[0], sizeof(wx_ens_obs) * (size_t)n_obs, hipMemcpyHostToDevice, e->stream);
  ens_launch(c, K_ENS_ASSIM_OBS, [&] { hipLaunchKernelGGL(wxa::k_ens_assim_obs, dim3(1), dim3(wxa::OBS_WG), oa.w_in_lds ? w_bytes : 0, e->stream, oa); });
  const unsigned wgs = ens_wgs_wave_per_item(ens_chunks(a->w, a->h), wxa::WAVES, wxa::MAX_WGS);
  for (int f = 0; f < 2; f++) {
    if (!update[f]) continue;
    wxa::Args ka;
    memset(&ka, 0, sizeof(ka));
    ka.X = e->X, ka.x0 = a->x, ka.y0 = a->y, ka.w = a->w, ka.h = a->h, ka.n_sel = n, ka.n_obs = n_obs;
    ka.loc = wxa::Loc{e->X, a->wrap_x ? 1 : 0, a->loc_x, a->loc_y};
    memcpy(ka.gain, f ? a->gain_water : a->gain_base, 16), memcpy(ka.lo, f ? a->lo_water : a->lo_base, 16), memcpy(ka.hi, f ? a->hi_water : a->hi_base, 16);
    ka.tab = st->tab_dev + (f ? n : 0), ka.hdr = oa.t.hdr, ka.e = oa.t.e;
    ens_launch(c, K_ENS_ASSIM, [&] { hipLaunchKernelGGL(wxa::k_ens_assim, dim3(wgs), dim3(wxa::WG), 0, e->stream, ka); });
  }
  if (c.he == hipSuccess && result)
    c.he = hipMemcpyAsync(st->out_host + at[1], oa.t.res, sizeof(wx_ens_obs_result) * (size_t)n_obs, hipMemcpyDeviceToHost, e->stream);
  const int rc = ens_finish(c);
  // The members are changed by now, so what the filter did goes back even when the sync hands on a member's pending report (an
  // overflowed list of an earlier step, say): the report is about that member, not about this call. Not after a failed enqueue.
  if (c.he == hipSuccess && result) memcpy(result, st->out_host + at[1], sizeof(wx_ens_obs_result) * (size_t)n_obs);
  return rc;
}
