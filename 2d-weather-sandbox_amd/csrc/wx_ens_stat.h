// wx_ens_stat.h -- statistics over the MEMBER axis of an ensemble (include/wxsim.h: wx_ens_stat, wx_ensemble_statistics,
// wx_ens_stat_cells): per cell and channel of a rectangle the mean, population variance, extremes with the member that holds them, the
// number of values that entered, the number above a threshold, and per cell the number of members in which it is a wall cell. Included
// at the end of wxsim.hip, behind wx_ens_frame.h (the entry points are declared extern "C" by include/wxsim.h). What wx_diag.h does for
// the space axis this does for the member axis -- with one difference that the header comment states: the sums are NOT exact sums but
// sums IN MEMBER ORDER, one double addition per entered value (a 320-bit accumulator per cell and channel would cost more than the
// fields it summarises), so the definition fixes the order and every implementation of it -- k_ens_stat, wx_ens_stat_cells, the
// tests' Python loop -- walks the members 0 first.
//
// THE per-cell function is cell_add / spread_add / the *_of finishers below, __host__ __device__: the kernel and the host entry point
// run the same program text. libwxsim.so (-ffp-contract=off) and libwxsim_fast.so (-ffp-contract=fast) give the same bits, on the
// host and on the device: Q += d * d is a rounded product and a rounded sum, never an FMA. Two things guarantee that. The contraction
// pragma at the head of every function that rounds tells the front end, which is enough for the host; the device code generator of a
// -ffp-contract=fast build fuses a multiply with a dependent add all the same, so there the one product that feeds a sum (`product`
// below) passes through an opaque register-constraint asm first. tests/test_ensemble_statistics_gpu.py runs the tolerance build on
// the device over cells on which a fused Q changes the float32 variance (tools/find_variance_separators.py found them). Double
// division, int -> double and double -> float conversions are correctly rounded on the device and on the host alike.
//
// The kernel: one lane per cell of the rectangle; the 64 lanes of a wave take 64 consecutive x of one row (a member's float4 load is
// 16 B per lane, 1 KiB per wave, contiguous; its wall texel 4 B per lane), waves grid-stride over the (row, 64-column chunk) pairs.
// Per cell the member loop is serial BY DEFINITION -- a dependent double add chain per channel --: the chunk cursor and the member walk
// are wx_ens_frame.h's (wxe::chunk_at, wxe::member_walk). Pass 1: sum, count, extremes, exceedance, walls. Pass 2 (only if the variance
// is wanted): the members again for Q = sum (v - mean)^2. The members' {field, wall, index} triples come from the ensemble's device table (wx_ens_frame.h: constant address
// space, wave-uniform addresses: scalar loads). Only the wanted planes are written, with 16-byte (n_wall: 4-byte) vector stores; nothing
// else is written, no atomics, no LDS. profiles/ensemble_statistics_isa.txt records the loads and waits of one gfx950 build.
// What it does not try: a w x h rectangle is ceil(w / 64) * h waves whatever the number of members (100 x 100: 200 waves on a chip
// with 1024 SIMDs). Splitting one cell's members over lanes would change the defined order of summation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <cmath>
#include <limits>
#include "../../include/wxsim.h"
#include "wx_diag.h"
#include "wx_rounded.h"
#include "wx_ens_frame.h"

namespace wxe {

// one channel of one cell, pass 1. mn / mx start at +Inf / -Inf: every entered value is finite, so the first one replaces both, and
// "strictly better" keeps the smallest member index among equal values (-0.0 == 0.0 in a float compare)
struct Chan {
  double S;
  float mn, mx;
  int amn, amx, n, above;
};
struct Cell {
  Chan c[4];
  int n_wall;
};
// pass 2: the means (double, unrounded to float) and the sums of squared deviations
struct Spread {
  double m[4], Q[4];
};

__host__ __device__ inline void cell_init(Cell &a)
{
#pragma unroll
  for (int c = 0; c < 4; c++) a.c[c] = Chan{0.0, __builtin_inff(), -__builtin_inff(), -1, -1, 0, 0};
  a.n_wall = 0;
}

// one member's texel: v = the field's four channels, wall_dist = channel 1 of its WX_FIELD_WALL_CUR texel, member = its index.
// Written with selects, not branches: the kernel's group of UNROLL members is meant to stay ONE basic block, so that the compiler can
// keep the group's loads in front of it with counted waits (a branch per member invites it to sink each wall load to its consumer: a
// full round trip per member). A select keeps the old value bit for bit, so "does not enter" still means "untouched".
__host__ __device__ inline void cell_add(Cell &a, const float v[4], int wall_dist, int member, const float thr[4])
{
#pragma clang fp contract(off)
  const bool air = wall_dist != 0;
  a.n_wall += air ? 0 : 1;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    Chan &q = a.c[c];
    const bool take = air && wxd::f32_finite(v[c]);
    const double s1 = q.S + (double)v[c];
    q.S = take ? s1 : q.S;
    q.n += take ? 1 : 0;
    const bool lo = take && v[c] < q.mn, hi = take && v[c] > q.mx;
    q.mn = lo ? v[c] : q.mn, q.amn = lo ? member : q.amn;
    q.mx = hi ? v[c] : q.mx, q.amx = hi ? member : q.amx;
    q.above += (take && v[c] > thr[c]) ? 1 : 0;
  }
}

__host__ __device__ inline void spread_init(Spread &s, const Cell &a)
{
#pragma clang fp contract(off)
#pragma unroll
  for (int c = 0; c < 4; c++) {
    s.m[c] = a.c[c].n ? a.c[c].S / (double)a.c[c].n : (double)__builtin_nanf("");
    s.Q[c] = 0.0;
  }
}

// A product that feeds a sum. In the tolerance build (-ffp-contract=fast) the device code generator fuses d * d into the add that
// follows, whatever the pragma says (k_ens_stat was the one kernel in which it did), so there the product passes
// through wx_rounded.h's opaque value first. The default build never contracts (-ffp-contract=off) and is left exactly as it
// was: an opaque value in the middle of the member group moves its waits (profiles/ensemble_statistics_isa.txt).
__host__ __device__ inline double product(double x)
{
#if defined(WX_FAST_ARITH) && WX_FAST_ARITH
  return wxr::rounded(x);
#else
  return x;
#endif
}

__host__ __device__ inline void spread_add(Spread &s, const float v[4], int wall_dist)
{
#pragma clang fp contract(off)
  const bool air = wall_dist != 0;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const bool take = air && wxd::f32_finite(v[c]);
    const double d = (double)v[c] - s.m[c];
    const double dd = product(d * d);
    const double q1 = s.Q[c] + dd;
    s.Q[c] = take ? q1 : s.Q[c];
  }
}

__host__ __device__ inline float mean_of(const Spread &s, int c) { return (float)s.m[c]; }
__host__ __device__ inline float variance_of(const Spread &s, const Cell &a, int c)
{
#pragma clang fp contract(off)
  return a.c[c].n ? (float)(s.Q[c] / (double)a.c[c].n) : __builtin_nanf("");
}
// a zero extreme is +0.0
__host__ __device__ inline float extreme_of(float e, int n) { return n ? (e == 0.0f ? 0.0f : e) : __builtin_nanf(""); }

struct Args {
  int X;              // cells per row of the members' arrays
  int x0, y0, w, h;   // the rectangle
  int n_sel;          // selected members
  const Member *tab;  // n_sel entries, member order
  float thr[4];
  // the wanted planes (w * h texels, rows bottom-up), nullptr: not wanted
  float4 *mean, *variance, *mn, *mx;
  int4 *amn, *amx, *count, *above;
  int *n_wall;
};

enum { WG = 256, WAVES = WG / 64, MAX_WGS = 2048, UNROLL = 8 };

#if defined(__HIPCC__)
__global__ __launch_bounds__(WG) void k_ens_stat(const Args a)
{
  const WaveOfGrid g = wave_of_grid(WAVES);
  const unsigned chunks = chunks_per_row(a.w) * (unsigned)a.h;
  const CTab tab = const_table(a.tab);
  const float thr[4] = {a.thr[0], a.thr[1], a.thr[2], a.thr[3]};
  for (unsigned ch = g.wave; ch < chunks; ch += g.n_waves) {
    const Chunk at = chunk_at(ch, g.lane, a.x0, a.y0, a.w);
    if (!at.valid) continue;
    const size_t off = texel_at(a.X, at.gx, at.gy), o = plane_at(a.w, at.x, at.y);
    const auto load = [&](int k) { return ld_field_wall(tab + k, off); };
    Cell cell;
    cell_init(cell);
    cell = member_walk<UNROLL>(a.n_sel, cell, load, [&](Cell &c, int k, const TexelWall &m) {
      const float f[4] = {m.v.x, m.v.y, m.v.z, m.v.w};
      cell_add(c, f, m.wd, tab[k].index, thr);
    });
    Spread sp;
    spread_init(sp, cell);
    if (a.variance) { // (wave-uniform)
      sp = member_walk<UNROLL>(a.n_sel, sp, load, [&](Spread &s, int, const TexelWall &m) {
        const float f[4] = {m.v.x, m.v.y, m.v.z, m.v.w};
        spread_add(s, f, m.wd);
      });
      a.variance[o] = make_float4(variance_of(sp, cell, 0), variance_of(sp, cell, 1), variance_of(sp, cell, 2), variance_of(sp, cell, 3));
    }
    const Chan *q = cell.c;
    if (a.mean) a.mean[o] = make_float4(mean_of(sp, 0), mean_of(sp, 1), mean_of(sp, 2), mean_of(sp, 3));
    if (a.mn) a.mn[o] = make_float4(extreme_of(q[0].mn, q[0].n), extreme_of(q[1].mn, q[1].n), extreme_of(q[2].mn, q[2].n), extreme_of(q[3].mn, q[3].n));
    if (a.mx) a.mx[o] = make_float4(extreme_of(q[0].mx, q[0].n), extreme_of(q[1].mx, q[1].n), extreme_of(q[2].mx, q[2].n), extreme_of(q[3].mx, q[3].n));
    if (a.amn) a.amn[o] = make_int4(q[0].amn, q[1].amn, q[2].amn, q[3].amn);
    if (a.amx) a.amx[o] = make_int4(q[0].amx, q[1].amx, q[2].amx, q[3].amx);
    if (a.count) a.count[o] = make_int4(q[0].n, q[1].n, q[2].n, q[3].n);
    if (a.above) a.above[o] = make_int4(q[0].above, q[1].above, q[2].above, q[3].above);
    if (a.n_wall) a.n_wall[o] = cell.n_wall;
  }
}
#endif // __HIPCC__

// the nine planes of wx_ens_stat in the order of the struct: bytes per cell, and the caller's pointer
enum { N_PLANES = 9 };
inline size_t plane_bytes(int p) { return p < 8 ? 16 : 4; }
inline void *plane_ptr(const wx_ens_stat *o, int p)
{
  void *const ptr[N_PLANES] = {o->mean, o->variance, o->min, o->max, o->argmin, o->argmax, o->count, o->n_above, o->n_wall};
  return ptr[p];
}

// host only, pure: the kernel's per-cell function over cells the caller holds
inline int stat_cells(int n_members, size_t n_cells, const float *const *field, const int8_t *const *wall, const uint8_t *mask, wx_ens_stat *out)
{
  if (n_members < 1 || !field || !wall || !out) return WX_E_INVALID;
  int n_sel = 0;
  for (int i = 0; i < n_members; i++) {
    if (mask && !mask[i]) continue;
    if (n_cells && (!field[i] || !wall[i])) return WX_E_INVALID;
    n_sel++;
  }
  if (n_sel == 0) return WX_E_INVALID;
  for (size_t i = 0; i < n_cells; i++) {
    Cell cell;
    cell_init(cell);
    for (int k = 0; k < n_members; k++) {
      if (mask && !mask[k]) continue;
      float v[4];
      memcpy(v, field[k] + 4 * i, 16);
      cell_add(cell, v, wall[k][4 * i + 1], k, out->threshold);
    }
    Spread sp;
    spread_init(sp, cell);
    if (out->variance)
      for (int k = 0; k < n_members; k++) {
        if (mask && !mask[k]) continue;
        float v[4];
        memcpy(v, field[k] + 4 * i, 16);
        spread_add(sp, v, wall[k][4 * i + 1]);
      }
    for (int c = 0; c < 4; c++) {
      const Chan &q = cell.c[c];
      if (out->mean) out->mean[4 * i + c] = mean_of(sp, c);
      if (out->variance) out->variance[4 * i + c] = variance_of(sp, cell, c);
      if (out->min) out->min[4 * i + c] = extreme_of(q.mn, q.n);
      if (out->max) out->max[4 * i + c] = extreme_of(q.mx, q.n);
      if (out->argmin) out->argmin[4 * i + c] = q.amn;
      if (out->argmax) out->argmax[4 * i + c] = q.amx;
      if (out->count) out->count[4 * i + c] = q.n;
      if (out->n_above) out->n_above[4 * i + c] = q.above;
    }
    if (out->n_wall) out->n_wall[i] = cell.n_wall;
  }
  return WX_OK;
}

} // namespace wxe

int wx_ens_stat_cells(int n_members, size_t n_cells, const float *const *field, const int8_t *const *wall, const uint8_t *member_mask, wx_ens_stat *out)
{
  return wxe::stat_cells(n_members, n_cells, field, wall, member_mask, out);
}

int wx_ensemble_statistics(wx_ensemble *e, int field, int x, int y, int w, int h, const uint8_t *member_mask, wx_ens_stat *out)
{
  static const char *const call = "wx_ensemble_statistics";
  if (!e || !out) return WX_E_INVALID;
  // the arguments first: nothing below this block is reached with a bad one, and nothing in it touches the device
  if (int rc = ens_check_state_field(e, call, field)) return rc;
  if (int rc = ens_check_rect(e, call, x, y, w, h)) return rc;
  const std::vector<int> sel = ens_select(e, member_mask);
  if (sel.empty()) return efail(e, WX_E_INVALID, "wx_ensemble_statistics: the member mask selects nobody");
  if (int rc = ens_require_uploaded(e, call, sel)) return rc;

  const size_t cells = (size_t)w * h;
  size_t at[wxe::N_PLANES], out_bytes = 0;
  for (int p = 0; p < wxe::N_PLANES; p++) {
    at[p] = out_bytes;
    if (wxe::plane_ptr(out, p)) out_bytes += cells * wxe::plane_bytes(p);
  }
  EnsCall c(e, call, K_ENS_STAT);
  if (int rc = ens_begin(c, (int)sel.size(), std::max<size_t>(out_bytes, 16))) return rc;
  EnsStage *st = c.st;
  ens_table_field(c, sel, field);

  wxe::Args a;
  memset(&a, 0, sizeof(a));
  a.X = e->X, a.x0 = x, a.y0 = y, a.w = w, a.h = h, a.n_sel = (int)sel.size();
  a.tab = st->tab_dev;
  memcpy(a.thr, out->threshold, sizeof(a.thr));
  auto dev_plane = [&](int p) -> void * { return wxe::plane_ptr(out, p) ? (void *)(st->out_dev + at[p]) : nullptr; };
  a.mean = (float4 *)dev_plane(0), a.variance = (float4 *)dev_plane(1), a.mn = (float4 *)dev_plane(2), a.mx = (float4 *)dev_plane(3);
  a.amn = (int4 *)dev_plane(4), a.amx = (int4 *)dev_plane(5), a.count = (int4 *)dev_plane(6), a.above = (int4 *)dev_plane(7);
  a.n_wall = (int *)dev_plane(8);

  // behind the table: kernel, planes to the pinned copy
  const unsigned wgs = ens_wgs_wave_per_item(ens_chunks(w, h), wxe::WAVES, wxe::MAX_WGS);
  ens_launch(c, K_ENS_STAT, [&] { hipLaunchKernelGGL(wxe::k_ens_stat, dim3(wgs), dim3(wxe::WG), 0, e->stream, a); });
  if (c.he == hipSuccess && out_bytes) c.he = hipMemcpyAsync(st->out_host, st->out_dev, out_bytes, hipMemcpyDeviceToHost, e->stream);
  if (int rc = ens_finish(c)) return rc;
  for (int p = 0; p < wxe::N_PLANES; p++)
    if (void *dst = wxe::plane_ptr(out, p)) memcpy(dst, st->out_host + at[p], cells * wxe::plane_bytes(p));
  return WX_OK;
}
