// wx_ens_assim_cell.h -- THE functions of wx_ensemble_assimilate (include/wxsim.h: wx_ens_assim, wx_ens_obs) and the pure host entry
// point built on them, as plain C++ that a host compiler takes without the HIP headers (tests/native/ens_assim_main.cpp compiles it
// under AddressSanitizer and UBSan); wx_ens_assim.h includes it for the kernels. A serial ensemble square-root filter (Whitaker and
// Hamill 2002) for point observations with separable Gaspari-Cohn localization: the Gaspari-Cohn polynomial (gc), the prior of an
// observation (prior_of), the member walk of one channel of one cell (sum_add, cov_add, gain_of, post_value; update_channel strings
// them together over an array), the argument checks and assim_cells, which IS the serial definition: for each observation its prior,
// then every cell of the rectangle, both fields. Every function that rounds switches floating-point contraction off for itself, every
// operation is a separate double operation, and a product that feeds a sum or a difference passes through wxr::rounded.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/wxsim.h"
#include "wx_rounded.h"
#include "wx_ens_cell_common.h"
#include <vector>

namespace wxa {

using wxr::rounded;

using wxcell::f32_bits;
using wxcell::f32_finite;
using wxcell::f64_finite;

// Gaspari and Cohn's fifth-order piecewise rational function of z = distance / half-width (z >= 0), by Horner
WX_HD inline double gc(double z)
{
#pragma clang fp contract(off)
  if (z >= 2.0) return 0.0;
  double p;
  if (z <= 1.0) {
    p = rounded(-0.25 * z) + 0.5;
    p = rounded(p * z) + 0.625;
    p = rounded(p * z) - 5.0 / 3.0;
    p = p * z;
    p = rounded(p * z) + 1.0;
  } else {
    p = rounded((1.0 / 12.0) * z) - 0.5;
    p = rounded(p * z) + 0.625;
    p = rounded(p * z) + 5.0 / 3.0;
    p = rounded(p * z) - 5.0;
    p = rounded(p * z) + 4.0;
    p = p - (2.0 / 3.0) / z;
  }
  return p < 0.0 ? 0.0 : p;
}

// what the localization needs of the descriptor and the grid
struct Loc {
  int X, wrap_x;
  float loc_x, loc_y;
};
WX_HD inline double axis_weight(int d, float loc)
{
#pragma clang fp contract(off)
  return loc == 0.0f ? 1.0 : gc((double)d / (double)loc);
}
WX_HD inline int dist_x(const Loc &l, int x, int ox)
{
  int dx = x > ox ? x - ox : ox - x;
  if (l.wrap_x && l.X - dx < dx) dx = l.X - dx;
  return dx;
}
WX_HD inline int dist_y(int y, int oy) { return y > oy ? y - oy : oy - y; }
WX_HD inline double rho_of(const Loc &l, int x, int y, int ox, int oy)
{
#pragma clang fp contract(off)
  return axis_weight(dist_x(l, x, ox), l.loc_x) * axis_weight(dist_y(y, oy), l.loc_y);
}

// the header of an applied observation: what does not depend on the cell (e_k = (double)t_k - hm goes with it)
struct Prior {
  double hm, V, D, innovation, alpha;
};

// t: the n selected members' values of the observed channel, member order; every t_k finite
WX_HD inline Prior prior_of(int n, const float *t, float value, float error_var)
{
#pragma clang fp contract(off)
  Prior p;
  double S = 0.0;
  for (int k = 0; k < n; k++) S = S + (double)t[k];
  p.hm = S / (double)n;
  double Q = 0.0;
  for (int k = 0; k < n; k++) {
    const double e = (double)t[k] - p.hm;
    Q = Q + rounded(e * e);
  }
  p.V = Q / (double)(n - 1);
  p.D = p.V + (double)error_var;
  p.innovation = (double)value - p.hm;
  p.alpha = 1.0 / (1.0 + __builtin_sqrt((double)error_var / p.D));
  return p;
}

// ---- one channel of one cell, member by member (the kernel keeps four of each; selects, not branches, as wx_ens_stat.h's cell_add) ----
// pass 1: Sx, and whether every member's value may enter (wx_ens_cell_common.h)
using wxcell::sum_add;
// pass 2: Cq
WX_HD inline void cov_add(double &Cq, float x, double xm, double e)
{
#pragma clang fp contract(off)
  const double d = (double)x - xm;
  Cq = Cq + rounded(d * e);
}
// between pass 2 and 3: a and b of the definition; on == false: the channel is untouched in all members
struct Gain {
  double a, b;
  bool on;
};
WX_HD inline Gain gain_of(bool ok, double Cq, int n, double w, const Prior &p)
{
#pragma clang fp contract(off)
  const double C = Cq / (double)(n - 1);
  const double K = (w * C) / p.D;
  Gain g;
  g.on = ok && K != 0.0 && f64_finite(K);
  g.a = K * p.innovation;
  g.b = p.alpha * K;
  return g;
}
// pass 3: the member's new value, or x itself (bit for bit)
WX_HD inline float post_value(float x, const Gain &g, double e, float lo, float hi)
{
#pragma clang fp contract(off)
  const double be = rounded(g.b * e);
  const double inc = g.a - be;
  float o = (float)((double)x + inc);
  if (lo == lo && o < lo) o = lo;
  if (hi == hi && o > hi) o = hi;
  return f32_finite(o) ? o : x;
}

// The whole walk over an array: x[0 .. n) the members' values of one channel of one cell that is an air cell in all of them, t / p the
// observation's values and header, w = (double)gain * rho (gain != 0, rho != 0). Returns whether any bits changed. The host entry
// point and the observation-space pre-pass of the device (on its working copies of the observed channels) both call this.
WX_HD inline bool update_channel(int n, float *x, const float *t, const Prior &p, double w, float lo, float hi)
{
#pragma clang fp contract(off)
  double S = 0.0;
  bool ok = true;
  for (int k = 0; k < n; k++) sum_add(S, ok, x[k], true);
  if (!ok) return false;
  const double xm = S / (double)n;
  double Cq = 0.0;
  for (int k = 0; k < n; k++) cov_add(Cq, x[k], xm, (double)t[k] - p.hm);
  const Gain g = gain_of(ok, Cq, n, w, p);
  if (!g.on) return false;
  bool changed = false;
  for (int k = 0; k < n; k++) {
    const float o = post_value(x[k], g, (double)t[k] - p.hm, lo, hi);
    changed = changed || f32_bits(o) != f32_bits(x[k]);
    x[k] = o;
  }
  return changed;
}

WX_HD inline bool in_rect(const wx_ens_assim &a, int x, int y) { return x >= a.x && x < a.x + a.w && y >= a.y && y < a.y + a.h; }

// the argument checks wx_ensemble_assimilate and wx_ens_assim_cells share (nothing here touches a device)
inline int check_desc(const wx_ens_assim *a, int n_obs, const wx_ens_obs *obs, int X, int Y, const char **why)
{
  *why = "";
  if (n_obs < 1 || n_obs > WX_ENS_OBS_MAX) {
    *why = "n_obs: 1 .. WX_ENS_OBS_MAX";
    return WX_E_INVALID;
  }
  if (!f32_finite(a->loc_x) || !f32_finite(a->loc_y) || a->loc_x < 0.0f || a->loc_y < 0.0f) {
    *why = "loc_x, loc_y: finite, >= 0 (0: no localization along that axis)";
    return WX_E_INVALID;
  }
  for (int c = 0; c < 4; c++)
    if (!f32_finite(a->gain_base[c]) || !f32_finite(a->gain_water[c])) {
      *why = "gain_base, gain_water: finite";
      return WX_E_INVALID;
    }
  for (int j = 0; j < n_obs; j++) {
    const wx_ens_obs &o = obs[j];
    if (o.field != WX_FIELD_BASE_CUR && o.field != WX_FIELD_WATER_CUR) {
      *why = "an observation's field: WX_FIELD_BASE_CUR or WX_FIELD_WATER_CUR (the fields that are stored whole and interleaved)";
      return WX_E_INVALID;
    }
    if (o.channel < 0 || o.channel > 3) {
      *why = "an observation's channel: 0 .. 3";
      return WX_E_INVALID;
    }
    if (!f32_finite(o.value) || !f32_finite(o.error_var) || !(o.error_var > 0.0f)) {
      *why = "an observation's value: finite; its error_var: finite, > 0";
      return WX_E_INVALID;
    }
  }
  if (a->w <= 0 || a->h <= 0 || a->x < 0 || a->y < 0 || (long long)a->x + a->w > X || (long long)a->y + a->h > Y) {
    *why = "the rectangle lies outside the grid (no wrap)";
    return WX_E_RANGE;
  }
  for (int j = 0; j < n_obs; j++)
    if (obs[j].x < 0 || obs[j].y < 0 || obs[j].x >= X || obs[j].y >= Y) {
      *why = "an observation lies outside the grid";
      return WX_E_RANGE;
    }
  return WX_OK;
}

WX_HD inline void result_skipped(wx_ens_obs_result &r)
{
  r.applied = 0, r.pad = 0;
  r.prior_mean = r.prior_var = r.innovation = r.alpha = (double)__builtin_nanf("");
}
WX_HD inline void result_applied(wx_ens_obs_result &r, const Prior &p)
{
  r.applied = 1, r.pad = 0;
  r.prior_mean = p.hm, r.prior_var = p.V, r.innovation = p.innovation, r.alpha = p.alpha;
}

// host only, pure: the serial definition over whole X x Y grids held by the caller (an observation may lie outside the rectangle)
inline int assim_cells(const wx_ens_assim *a, int n_obs, const wx_ens_obs *obs, wx_ens_obs_result *result, int X, int Y, int n_members,
                       float *const *base, float *const *water, const int8_t *const *wall, const uint8_t *mask)
{
  if (!a || !obs || n_members < 1 || !base || !water || !wall || X < 1 || Y < 1) return WX_E_INVALID;
  const char *why;
  if (int rc = check_desc(a, n_obs, obs, X, Y, &why)) return rc;
  std::vector<int> sel;
  for (int i = 0; i < n_members; i++) {
    if (mask && !mask[i]) continue;
    if (!base[i] || !water[i] || !wall[i]) return WX_E_INVALID;
    sel.push_back(i);
  }
  const int n = (int)sel.size();
  if (n < 2) return WX_E_INVALID;
  const Loc loc{X, a->wrap_x ? 1 : 0, a->loc_x, a->loc_y};
  std::vector<float> t((size_t)n), xs((size_t)n);
  auto air_in_all = [&](size_t cell) {
    for (int k = 0; k < n; k++)
      if (wall[sel[k]][4 * cell + 1] == 0) return false;
    return true;
  };
  for (int j = 0; j < n_obs; j++) {
    const wx_ens_obs &o = obs[j];
    const size_t ocell = (size_t)o.y * (size_t)X + (size_t)o.x;
    float *const *ofield = o.field == WX_FIELD_BASE_CUR ? base : water;
    bool usable = air_in_all(ocell);
    for (int k = 0; k < n; k++) {
      t[k] = ofield[sel[k]][4 * ocell + o.channel]; // (a copy: the observed cell may itself be updated below)
      usable = usable && f32_finite(t[k]);
    }
    if (!usable) {
      if (result) result_skipped(result[j]);
      continue;
    }
    const Prior p = prior_of(n, t.data(), o.value, o.error_var);
    if (result) result_applied(result[j], p);
    for (int y = a->y; y < a->y + a->h; y++)
      for (int x = a->x; x < a->x + a->w; x++) {
        const double rho = rho_of(loc, x, y, o.x, o.y);
        if (rho == 0.0) continue;
        const size_t cell = (size_t)y * (size_t)X + (size_t)x;
        if (!air_in_all(cell)) continue;
        for (int f = 0; f < 2; f++) {
          float *const *field = f ? water : base;
          const float *gain = f ? a->gain_water : a->gain_base, *lo = f ? a->lo_water : a->lo_base, *hi = f ? a->hi_water : a->hi_base;
          for (int c = 0; c < 4; c++) {
            if (gain[c] == 0.0f) continue;
            for (int k = 0; k < n; k++) memcpy(&xs[k], field[sel[k]] + 4 * cell + c, 4);
            if (update_channel(n, xs.data(), t.data(), p, (double)gain[c] * rho, lo[c], hi[c]))
              for (int k = 0; k < n; k++) memcpy(field[sel[k]] + 4 * cell + c, &xs[k], 4);
          }
        }
      }
  }
  return WX_OK;
}

} // namespace wxa
