// wx_ens_inflate.h -- covariance inflation and relaxation to the prior on the device (include/wxsim.h: wx_ens_inflate,
// wx_ensemble_inflate, wx_ensemble_prior_save, wx_ensemble_prior_drop, wx_ens_inflate_cells): the spread that wx_ensemble_assimilate
// removes put back, in one launch, defined bit for bit by wx_ens_inflate_cell.h. Included at the end of wxsim.hip behind wx_ens_assim.h
// (the entry points are declared extern "C" by include/wxsim.h).
//
// k_ens_prior_save. The snapshot the relaxation modes read: the rectangle of one field of every selected member into one buffer laid
// out [k][h][w] float4. k_ens_perturb's walk: one lane per cell, waves grid-stride over the (member, row, 64-column chunk) triples with
// a capped grid (its head written out, not wxe::member_chunk_at: DESIGN.md section 4, "One member walk"). 16 B read and 16 B written per member-cell.
//
// k_ens_inflate<MODE>. k_ens_assim's shape without the observation loop: one lane per cell of the rectangle, a wave takes 64
// consecutive x of one row, waves grid-stride over the (row, chunk) pairs with a capped grid. Per cell the walks over the members that
// the definition names, each with the loads of UNROLL members issued before the first is consumed (written out here, not
// wxe::member_walk: through the template the RTPS instantiation spills scalar registers; DESIGN.md section 4, "One member walk"), the
// member table read at wave-uniform addresses through the constant address space, and 16-byte stores in place, only of texels whose bits change:
//   CONST  walk 1: S and the entry test (16 B field + 4 B wall)        walk 2: the write (16 B read, 16 B written)
//   RTPS   walk 1: S, Sb and the entry test (16 + 4 + 16 B snapshot)   walk 2: Qa, Qb (16 + 16 B)   walk 3: the write (16 B, 16 B)
//   RTPP   walk 1: S, Sb and the entry test (16 + 4 + 16 B)            walk 2: the write (16 + 16 B read, 16 B written)
// so a member-cell moves at most 52 B (CONST), 100 B (RTPS) and 84 B (RTPP); a cell whose four channels are all left alone ends after
// walk 1. The template on the mode keeps every snapshot load out of CONST. The snapshot is read through an ordinary global pointer (its
// address is per lane). No LDS, no atomics, no device-side waiting. What it does not try: holding the members in registers across the
// walks for small n.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/wxsim.h"
#include "wx_ens_frame.h"
#include "wx_ens_perturb.h"
#include "wx_ens_inflate_cell.h"

namespace wxi {

struct SaveArgs {
  int X;
  int x0, y0, w, h;
  int n_sel;
  const wxe::Member *tab; // n_sel entries of the saved field
  float4 *out;            // [n_sel][h][w]
};

struct Args {
  int X;
  int x0, y0, w, h;
  int n_sel;
  int on[4];              // the channel's coefficient is not neutral
  float coef[4], lam_lo, lam_hi, lo[4], hi[4];
  const wxe::Member *tab; // n_sel entries of the field (written in place)
  const float4 *prior;    // the snapshot [n_sel][ph][pw] of the rectangle (px0, py0, pw, ph); CONST: not looked at
  int px0, py0, pw, ph;
  float4 *lambda_out;     // w * h texels, or nullptr
};

enum { WG = 256, WAVES = WG / 64, MAX_WGS = 2048, UNROLL = 8, SAVE_MAX_WGS = 2048 };

#if defined(__HIPCC__)
__global__ __launch_bounds__(WG) void k_ens_prior_save(const SaveArgs a)
{
  const unsigned lane = threadIdx.x & 63u, wave = blockIdx.x * WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * WAVES;
  const unsigned cpr = ((unsigned)a.w + 63u) / 64u, per_member = cpr * (unsigned)a.h; // (below 2^31: 16 Ki chunks per row x 64 Ki rows)
  const unsigned long long items = (unsigned long long)per_member * (unsigned)a.n_sel;
  const wxe::CTab tab = wxe::const_table(a.tab);
  for (unsigned long long it = wave; it < items; it += n_waves) {
    const unsigned k = (unsigned)(it / per_member), ch = (unsigned)(it - (unsigned long long)k * per_member);
    const unsigned y = ch / cpr, x = (ch - y * cpr) * 64u + lane;
    if (x >= (unsigned)a.w) continue;
    const size_t off = (size_t)(a.y0 + (int)y) * (size_t)a.X + (size_t)(a.x0 + (int)x);
    st_texel(a.out, ((size_t)k * (size_t)a.h + y) * (size_t)a.w + x, wxe::ld_field(tab + k, off));
  }
}

template <int MODE>
__global__ __launch_bounds__(WG) void k_ens_inflate(const Args a)
{
  constexpr bool RELAX = MODE != WX_INFLATE_CONST;
  const wxe::WaveOfGrid wg = wxe::wave_of_grid(WAVES);
  const unsigned chunks = wxe::chunks_per_row(a.w) * (unsigned)a.h;
  const wxe::CTab tab = wxe::const_table(a.tab);
  const int n = a.n_sel;
  const size_t pstride = RELAX ? (size_t)a.pw * (size_t)a.ph : 0; // texels per member of the snapshot
  for (unsigned ch = wg.wave; ch < chunks; ch += wg.n_waves) {
    const wxe::Chunk at = wxe::chunk_at(ch, wg.lane, a.x0, a.y0, a.w);
    if (!at.valid) continue;
    const size_t off = wxe::texel_at(a.X, at.gx, at.gy);
    const size_t poff = RELAX ? (size_t)(at.gy - a.py0) * (size_t)a.pw + (size_t)(at.gx - a.px0) : 0;
    Lambda l[4];
#pragma unroll
    for (int c = 0; c < 4; c++) l[c] = lambda_tail(false, 1.0);
    // walk 1: S, Sb and the entry test
    double S[4] = {0.0, 0.0, 0.0, 0.0}, Sb[4] = {0.0, 0.0, 0.0, 0.0};
    bool ok[4] = {a.on[0] != 0, a.on[1] != 0, a.on[2] != 0, a.on[3] != 0};
    int k = 0;
    for (; k + UNROLL <= n; k += UNROLL) { // the loads of UNROLL members are issued before the first of them is consumed
      wxe::f32x4 v[UNROLL], p[UNROLL];
      int wd[UNROLL];
#pragma unroll
      for (int i = 0; i < UNROLL; i++) {
        v[i] = wxe::ld_field(tab + k + i, off), wd[i] = wxe::ld_wall_dist(tab + k + i, off);
        if (RELAX) p[i] = ld_prior(a.prior, (size_t)(k + i) * pstride + poff);
      }
      WX_ENS_LOADS_ISSUED();
#pragma unroll
      for (int i = 0; i < UNROLL; i++) {
        const bool air = wd[i] != 0;
        sum_add(S[0], ok[0], v[i].x, air), sum_add(S[1], ok[1], v[i].y, air), sum_add(S[2], ok[2], v[i].z, air), sum_add(S[3], ok[3], v[i].w, air);
        if (RELAX) prior_add(Sb[0], ok[0], p[i].x), prior_add(Sb[1], ok[1], p[i].y), prior_add(Sb[2], ok[2], p[i].z), prior_add(Sb[3], ok[3], p[i].w);
      }
    }
    for (; k < n; k++) {
      const wxe::f32x4 v = wxe::ld_field(tab + k, off);
      const bool air = wxe::ld_wall_dist(tab + k, off) != 0;
      sum_add(S[0], ok[0], v.x, air), sum_add(S[1], ok[1], v.y, air), sum_add(S[2], ok[2], v.z, air), sum_add(S[3], ok[3], v.w, air);
      if (RELAX) {
        const wxe::f32x4 p = ld_prior(a.prior, (size_t)k * pstride + poff);
        prior_add(Sb[0], ok[0], p.x), prior_add(Sb[1], ok[1], p.y), prior_add(Sb[2], ok[2], p.z), prior_add(Sb[3], ok[3], p.w);
      }
    }
    if (ok[0] || ok[1] || ok[2] || ok[3]) {
      double m[4], mb[4];
#pragma unroll
      for (int c = 0; c < 4; c++) m[c] = S[c] / (double)n, mb[c] = Sb[c] / (double)n;
      if (MODE == WX_INFLATE_RTPP) {
        // walk 2: the write; a texel whose bits do not change is not stored
        double ca[4], cg[4];
#pragma unroll
        for (int c = 0; c < 4; c++) ca[c] = (double)a.coef[c], cg[c] = 1.0 - ca[c];
        auto write = [&](int mi, const wxe::f32x4 v, const wxe::f32x4 p) {
          wxe::f32x4 o;
          o.x = ok[0] ? post_rtpp(v.x, p.x, m[0], mb[0], ca[0], cg[0], a.lo[0], a.hi[0]) : v.x;
          o.y = ok[1] ? post_rtpp(v.y, p.y, m[1], mb[1], ca[1], cg[1], a.lo[1], a.hi[1]) : v.y;
          o.z = ok[2] ? post_rtpp(v.z, p.z, m[2], mb[2], ca[2], cg[2], a.lo[2], a.hi[2]) : v.z;
          o.w = ok[3] ? post_rtpp(v.w, p.w, m[3], mb[3], ca[3], cg[3], a.lo[3], a.hi[3]) : v.w;
          if (wxcell::texel_changed(o, v)) wxp::st_field(tab + mi, off, o);
        };
        for (k = 0; k + UNROLL <= n; k += UNROLL) {
          wxe::f32x4 v[UNROLL], p[UNROLL];
#pragma unroll
          for (int i = 0; i < UNROLL; i++) v[i] = wxe::ld_field(tab + k + i, off), p[i] = ld_prior(a.prior, (size_t)(k + i) * pstride + poff);
          WX_ENS_LOADS_ISSUED();
#pragma unroll
          for (int i = 0; i < UNROLL; i++) write(k + i, v[i], p[i]);
        }
        for (; k < n; k++) write(k, wxe::ld_field(tab + k, off), ld_prior(a.prior, (size_t)k * pstride + poff));
      } else {
        if (MODE == WX_INFLATE_CONST) {
#pragma unroll
          for (int c = 0; c < 4; c++) l[c] = lambda_tail(ok[c], (double)a.coef[c]);
        } else {
          // walk 2: Qa about m, Qb about mb
          double Qa[4] = {0.0, 0.0, 0.0, 0.0}, Qb[4] = {0.0, 0.0, 0.0, 0.0};
          for (k = 0; k + UNROLL <= n; k += UNROLL) {
            wxe::f32x4 v[UNROLL], p[UNROLL];
#pragma unroll
            for (int i = 0; i < UNROLL; i++) v[i] = wxe::ld_field(tab + k + i, off), p[i] = ld_prior(a.prior, (size_t)(k + i) * pstride + poff);
            WX_ENS_LOADS_ISSUED();
#pragma unroll
            for (int i = 0; i < UNROLL; i++) {
              q_add(Qa[0], v[i].x, m[0]), q_add(Qa[1], v[i].y, m[1]), q_add(Qa[2], v[i].z, m[2]), q_add(Qa[3], v[i].w, m[3]);
              q_add(Qb[0], p[i].x, mb[0]), q_add(Qb[1], p[i].y, mb[1]), q_add(Qb[2], p[i].z, mb[2]), q_add(Qb[3], p[i].w, mb[3]);
            }
          }
          for (; k < n; k++) {
            const wxe::f32x4 v = wxe::ld_field(tab + k, off), p = ld_prior(a.prior, (size_t)k * pstride + poff);
            q_add(Qa[0], v.x, m[0]), q_add(Qa[1], v.y, m[1]), q_add(Qa[2], v.z, m[2]), q_add(Qa[3], v.w, m[3]);
            q_add(Qb[0], p.x, mb[0]), q_add(Qb[1], p.y, mb[1]), q_add(Qb[2], p.z, mb[2]), q_add(Qb[3], p.w, mb[3]);
          }
#pragma unroll
          for (int c = 0; c < 4; c++) l[c] = lambda_rtps(ok[c], Qa[c], Qb[c], n, a.coef[c], a.lam_lo, a.lam_hi);
        }
        if (l[0].on || l[1].on || l[2].on || l[3].on) {
          // the last walk: the write; a texel whose bits do not change is not stored
          auto write = [&](int mi, const wxe::f32x4 v) {
            wxe::f32x4 o;
            o.x = l[0].on ? post_scale(v.x, m[0], l[0].v, a.lo[0], a.hi[0]) : v.x;
            o.y = l[1].on ? post_scale(v.y, m[1], l[1].v, a.lo[1], a.hi[1]) : v.y;
            o.z = l[2].on ? post_scale(v.z, m[2], l[2].v, a.lo[2], a.hi[2]) : v.z;
            o.w = l[3].on ? post_scale(v.w, m[3], l[3].v, a.lo[3], a.hi[3]) : v.w;
            if (wxcell::texel_changed(o, v)) wxp::st_field(tab + mi, off, o);
          };
          for (k = 0; k + UNROLL <= n; k += UNROLL) {
            wxe::f32x4 v[UNROLL];
#pragma unroll
            for (int i = 0; i < UNROLL; i++) v[i] = wxe::ld_field(tab + k + i, off);
            WX_ENS_LOADS_ISSUED();
#pragma unroll
            for (int i = 0; i < UNROLL; i++) write(k + i, v[i]);
          }
          for (; k < n; k++) write(k, wxe::ld_field(tab + k, off));
        }
      }
    }
    if (a.lambda_out) { // (uniform; never with RTPP)
      wxe::f32x4 lf;
      lf.x = lambda_float(l[0]), lf.y = lambda_float(l[1]), lf.z = lambda_float(l[2]), lf.w = lambda_float(l[3]);
      st_texel(a.lambda_out, wxe::plane_at(a.w, at.x, at.y), lf);
    }
  }
}
#endif // __HIPCC__

} // namespace wxi

// ---- the ensemble's side: one snapshot slot per field ----
struct EnsPriorSlot {
  float4 *buf = nullptr;
  size_t bytes = 0;
  bool have = false;
  int x = 0, y = 0, w = 0, h = 0;
  std::vector<uint8_t> selected; // one byte per member of the ensemble
};
struct EnsPriorState {
  EnsPriorSlot slot[2]; // BASE_CUR, WATER_CUR
};

static void ens_prior_slot_free(EnsPriorSlot &s)
{
  hipFree(s.buf);
  s = EnsPriorSlot{};
}

static void ens_prior_release(wx_ensemble *e)
{
  if (!e->prior) return;
  for (EnsPriorSlot &s : e->prior->slot) ens_prior_slot_free(s);
  delete e->prior;
  e->prior = nullptr;
}

int wx_ens_inflate_cells(const wx_ens_inflate *p, int n_members, size_t n_cells, float *const *field, const int8_t *const *wall, const float *const *prior,
                         const uint8_t *member_mask)
{
  return wxi::inflate_cells(p, n_members, n_cells, field, wall, prior, member_mask);
}

int wx_ensemble_prior_drop(wx_ensemble *e, int field)
{
  if (!e) return WX_E_INVALID;
  if (field != WX_FIELD_BASE_CUR && field != WX_FIELD_WATER_CUR)
    return efail(e, WX_E_INVALID, "wx_ensemble_prior_drop: field %d: WX_FIELD_BASE_CUR or WX_FIELD_WATER_CUR", field);
  if (!e->prior) return WX_OK;
  DeviceScope dev_scope(e->member[0]);
  ens_prior_slot_free(e->prior->slot[field == WX_FIELD_BASE_CUR ? 0 : 1]); // (every call that reads a snapshot blocks: nothing is in flight)
  return WX_OK;
}

// The snapshot a call reads (RTPS / RTPP, WX_COV_SOURCE_PRIOR): there is one of this field, it was taken of exactly this selection, and
// the rectangle lies inside its rectangle.
static int ens_snapshot_for(wx_ensemble *e, const char *call, int field, const uint8_t *member_mask, int x, int y, int w, int h, const EnsPriorSlot **snap)
{
  const EnsPriorSlot *s = e->prior ? &e->prior->slot[field == WX_FIELD_BASE_CUR ? 0 : 1] : nullptr;
  if (!s || !s->have) return efail(e, WX_E_STATE, "%s: no snapshot of field %d (wx_ensemble_prior_save comes first)", call, field);
  for (int i = 0; i < (int)e->member.size(); i++)
    if ((s->selected[(size_t)i] != 0) != (!member_mask || member_mask[i])) return efail(e, WX_E_STATE, "%s: the selection differs from the snapshot's (member %d)", call, i);
  if (x < s->x || y < s->y || x + w > s->x + s->w || y + h > s->y + s->h)
    return efail(e, WX_E_STATE, "%s: rect (%d,%d %dx%d) is not inside the snapshot's (%d,%d %dx%d)", call, x, y, w, h, s->x, s->y, s->w, s->h);
  *snap = s;
  return WX_OK;
}

int wx_ensemble_prior_save(wx_ensemble *e, int field, int x, int y, int w, int h, const uint8_t *member_mask)
{
  static const char *const call = "wx_ensemble_prior_save";
  if (!e) return WX_E_INVALID;
  // the arguments first: nothing below this block is reached with a bad one, and nothing in it touches the device
  if (int rc = ens_check_state_field(e, call, field)) return rc;
  if (int rc = ens_check_rect(e, call, x, y, w, h)) return rc;
  const std::vector<int> sel = ens_select(e, member_mask);
  if (sel.empty()) return efail(e, WX_E_INVALID, "wx_ensemble_prior_save: the member mask selects nobody");
  if (int rc = ens_require_uploaded(e, call, sel)) return rc;

  const int n = (int)sel.size();
  EnsCall c(e, call, K_ENS_PRIOR_SAVE);
  if (int rc = ens_begin(c, n, 16)) return rc;
  if (!e->prior) e->prior = new EnsPriorState();
  EnsPriorSlot &s = e->prior->slot[field == WX_FIELD_BASE_CUR ? 0 : 1];
  const size_t bytes = (size_t)n * (size_t)w * (size_t)h * sizeof(float4);
  s.have = false;
  if (bytes != s.bytes) {
    ens_prior_slot_free(s);
    if (hipMalloc((void **)&s.buf, bytes) != hipSuccess) {
      (void)hipGetLastError();
      s.buf = nullptr;
      return efail(e, WX_E_NOMEM, "wx_ensemble_prior_save: %zu bytes for the snapshot of %d members x %d x %d cells", bytes, n, w, h);
    }
    s.bytes = bytes;
  }
  ens_table_field(c, sel, field);

  wxi::SaveArgs a;
  memset(&a, 0, sizeof(a));
  a.X = e->X, a.x0 = x, a.y0 = y, a.w = w, a.h = h, a.n_sel = n, a.tab = c.st->tab_dev, a.out = s.buf;
  const unsigned wgs = ens_wgs_wave_per_item((unsigned long long)ens_chunks(w, h) * (unsigned)n, wxi::WAVES, wxi::SAVE_MAX_WGS);
  ens_launch(c, K_ENS_PRIOR_SAVE, [&] { hipLaunchKernelGGL(wxi::k_ens_prior_save, dim3(wgs), dim3(wxi::WG), 0, e->stream, a); });
  if (c.he == hipSuccess) { // (the snapshot stands once its kernel is enqueued, whatever the sync hands on about a member)
    s.have = true, s.x = x, s.y = y, s.w = w, s.h = h;
    s.selected.assign(e->member.size(), 0);
    for (int i : sel) s.selected[(size_t)i] = 1;
  }
  return ens_finish(c);
}

int wx_ensemble_inflate(wx_ensemble *e, const wx_ens_inflate *p, const uint8_t *member_mask)
{
  static const char *const call = "wx_ensemble_inflate";
  if (!e || !p) return WX_E_INVALID;
  // the arguments first: nothing below this block is reached with a bad one, and nothing in it touches the device
  const char *why;
  if (int rc = wxi::check_desc(p, &why)) return efail(e, rc, "wx_ensemble_inflate: %s", why);
  const std::vector<int> sel = ens_select(e, member_mask);
  if (sel.size() < 2) return efail(e, WX_E_INVALID, "wx_ensemble_inflate: the member mask selects %zu member(s); a spread takes two", sel.size());
  if (int rc = wxi::check_rect(p, e->X, e->Y, &why)) return efail(e, rc, "wx_ensemble_inflate: %s", why);
  if (int rc = ens_require_uploaded(e, call, sel)) return rc;
  const bool relax = p->mode != WX_INFLATE_CONST;
  const EnsPriorSlot *snap = nullptr;
  if (relax)
    if (int rc = ens_snapshot_for(e, call, p->field, member_mask, p->x, p->y, p->w, p->h, &snap)) return rc;

  const int n = (int)sel.size();
  const size_t lam_bytes = p->lambda_out ? (size_t)p->w * (size_t)p->h * sizeof(float4) : 0;
  EnsCall c(e, call, K_ENS_INFLATE);
  if (int rc = ens_begin(c, n, std::max<size_t>(lam_bytes, 16))) return rc;
  EnsStage *st = c.st;
  for (int i : sel)
    if (int rc = epass(e, i, ens_perturb_prepare(e->member[i], p->field))) return rc;
  ens_table_field(c, sel, p->field);

  wxi::Args a;
  memset(&a, 0, sizeof(a));
  a.X = e->X, a.x0 = p->x, a.y0 = p->y, a.w = p->w, a.h = p->h, a.n_sel = n;
  for (int ch = 0; ch < 4; ch++) a.on[ch] = wxi::neutral(p->mode, p->coef[ch]) ? 0 : 1, a.coef[ch] = p->coef[ch], a.lo[ch] = p->lo[ch], a.hi[ch] = p->hi[ch];
  a.lam_lo = p->lambda_lo, a.lam_hi = p->lambda_hi;
  a.tab = st->tab_dev;
  if (relax) a.prior = snap->buf, a.px0 = snap->x, a.py0 = snap->y, a.pw = snap->w, a.ph = snap->h;
  a.lambda_out = lam_bytes ? (float4 *)st->out_dev : nullptr;

  // behind the table: kernel, the map to the pinned copy
  const dim3 grid(ens_wgs_wave_per_item(ens_chunks(p->w, p->h), wxi::WAVES, wxi::MAX_WGS)), wg(wxi::WG);
  ens_launch(c, K_ENS_INFLATE, [&] {
    if (p->mode == WX_INFLATE_CONST) hipLaunchKernelGGL(wxi::k_ens_inflate<WX_INFLATE_CONST>, grid, wg, 0, e->stream, a);
    else if (p->mode == WX_INFLATE_RTPS) hipLaunchKernelGGL(wxi::k_ens_inflate<WX_INFLATE_RTPS>, grid, wg, 0, e->stream, a);
    else hipLaunchKernelGGL(wxi::k_ens_inflate<WX_INFLATE_RTPP>, grid, wg, 0, e->stream, a);
  });
  if (c.he == hipSuccess && lam_bytes) c.he = hipMemcpyAsync(st->out_host, st->out_dev, lam_bytes, hipMemcpyDeviceToHost, e->stream);
  const int rc = ens_finish(c);
  // The members are changed by now, so the map of what was applied goes back even when the sync hands on a member's pending report:
  // the report is about that member, not about this call. Not after a failed enqueue.
  if (c.he == hipSuccess && lam_bytes) memcpy(p->lambda_out, st->out_host, lam_bytes);
  return rc;
}
