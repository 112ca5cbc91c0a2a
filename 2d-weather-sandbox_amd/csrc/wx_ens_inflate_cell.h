// wx_ens_inflate_cell.h -- THE functions of wx_ensemble_inflate (include/wxsim.h: wx_ens_inflate) and the pure host entry point built
// on them, as plain C++ that a host compiler takes without the HIP headers (tests/native/ens_inflate_main.cpp compiles it under
// AddressSanitizer and UBSan); wx_ens_inflate.h includes it for the kernel. Covariance inflation about the ensemble mean (CONST),
// relaxation to prior spread (RTPS, Whitaker and Hamill 2012) and relaxation to prior perturbations (RTPP, Zhang et al. 2004): the
// member walks of one channel of one cell (sum_add, prior_add, q_add), the factor (lambda_rtps, lambda_tail), the member's new value
// (post_scale, post_rtpp); inflate_channel strings them together over an array and IS the definition. Every function that rounds
// switches floating-point contraction off for itself, every operation is a separate double operation, and a product that feeds a sum
// passes through wxr::rounded.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/wxsim.h"
#include "wx_rounded.h"
#include "wx_ens_cell_common.h"
#include <vector>

namespace wxi {

using wxr::rounded;

using wxcell::f32_bits;
using wxcell::f32_finite;
using wxcell::f64_finite;

// a channel whose coefficient is neutral is not looked at
WX_HD inline bool neutral(int mode, float coef) { return mode == WX_INFLATE_CONST ? coef == 1.0f : coef == 0.0f; }

// ---- one channel of one cell, member by member (the kernel keeps four of each; selects, not branches, as wx_ens_stat.h's cell_add) ----
// walk 1: S, and whether every member's value may enter (wx_ens_cell_common.h)
using wxcell::sum_add;
// walk 1, the relaxation modes: Sb over the snapshot
WX_HD inline void prior_add(double &Sb, bool &ok, float p)
{
#pragma clang fp contract(off)
  ok = ok && f32_finite(p);
  Sb = Sb + (double)p;
}
// walk 2 (RTPS): Qa about m, Qb about mb
WX_HD inline void q_add(double &Q, float v, double mean)
{
#pragma clang fp contract(off)
  const double d = (double)v - mean;
  Q = Q + rounded(d * d);
}

// the factor of CONST and RTPS; on == false: the channel is untouched in all members
struct Lambda {
  double v;
  bool on;
};
// the common tail: a factor that is not finite, or is 1, changes nothing
WX_HD inline Lambda lambda_tail(bool ok, double lam)
{
  Lambda l;
  l.v = lam;
  l.on = ok && f64_finite(lam) && lam != 1.0;
  return l;
}
WX_HD inline Lambda lambda_rtps(bool ok, double Qa, double Qb, int n, float alpha, float lam_lo, float lam_hi)
{
#pragma clang fp contract(off)
  const double sa = __builtin_sqrt(Qa / (double)(n - 1)), sb = __builtin_sqrt(Qb / (double)(n - 1));
  if (sa == 0.0) return lambda_tail(false, 1.0);
  const double r = (sb - sa) / sa;
  double lam = 1.0 + rounded((double)alpha * r);
  if (lam_lo == lam_lo && lam < (double)lam_lo) lam = (double)lam_lo;
  if (lam_hi == lam_hi && lam > (double)lam_hi) lam = (double)lam_hi;
  return lambda_tail(ok, lam);
}
WX_HD inline float lambda_float(const Lambda &l) { return l.on ? (float)l.v : __builtin_nanf(""); }

// wx_ens_perturb's clamp; a result that is not finite keeps the member's bits
WX_HD inline float clamp_or_keep(float o, float x, float lo, float hi)
{
  if (lo == lo && o < lo) o = lo;
  if (hi == hi && o > hi) o = hi;
  return f32_finite(o) ? o : x;
}
// walk 3, CONST and RTPS: the member's new value, or x itself (bit for bit)
WX_HD inline float post_scale(float x, double m, double lam, float lo, float hi)
{
#pragma clang fp contract(off)
  const double d = (double)x - m;
  const double ld = rounded(lam * d);
  return clamp_or_keep((float)(m + ld), x, lo, hi);
}
// walk 2, RTPP
WX_HD inline float post_rtpp(float x, float p, double m, double mb, double a, double g, float lo, float hi)
{
#pragma clang fp contract(off)
  const double d = (double)x - m, b = (double)p - mb;
  const double gd = rounded(g * d), ab = rounded(a * b);
  const double mix = gd + ab;
  return clamp_or_keep((float)(m + mix), x, lo, hi);
}

// The whole walk over an array: x[0 .. n) the members' values of one channel of one cell, p[0 .. n) their snapshot values (not looked
// at in CONST), air: the cell is an air cell in all of them. *lambda_out: the factor applied, or NaN. Returns whether any bits changed.
WX_HD inline bool inflate_channel(int mode, float coef, float lam_lo, float lam_hi, float lo, float hi, int n, float *x, const float *p, bool air, float *lambda_out)
{
#pragma clang fp contract(off)
  *lambda_out = __builtin_nanf("");
  if (neutral(mode, coef)) return false;
  const bool relax = mode != WX_INFLATE_CONST;
  double S = 0.0, Sb = 0.0;
  bool ok = true;
  for (int k = 0; k < n; k++) {
    sum_add(S, ok, x[k], air);
    if (relax) prior_add(Sb, ok, p[k]);
  }
  if (!ok) return false;
  const double m = S / (double)n, mb = Sb / (double)n;
  bool changed = false;
  if (mode == WX_INFLATE_RTPP) {
    const double a = (double)coef, g = 1.0 - a;
    for (int k = 0; k < n; k++) {
      const float o = post_rtpp(x[k], p[k], m, mb, a, g, lo, hi);
      changed = changed || f32_bits(o) != f32_bits(x[k]);
      x[k] = o;
    }
    return changed;
  }
  Lambda l;
  if (mode == WX_INFLATE_CONST) {
    l = lambda_tail(true, (double)coef);
  } else {
    double Qa = 0.0, Qb = 0.0;
    for (int k = 0; k < n; k++) q_add(Qa, x[k], m), q_add(Qb, p[k], mb);
    l = lambda_rtps(true, Qa, Qb, n, coef, lam_lo, lam_hi);
  }
  if (!l.on) return false;
  *lambda_out = lambda_float(l);
  for (int k = 0; k < n; k++) {
    const float o = post_scale(x[k], m, l.v, lo, hi);
    changed = changed || f32_bits(o) != f32_bits(x[k]);
    x[k] = o;
  }
  return changed;
}

// the argument checks wx_ensemble_inflate and wx_ens_inflate_cells share (nothing here touches a device)
inline int check_desc(const wx_ens_inflate *p, const char **why)
{
  *why = "";
  if (p->field != WX_FIELD_BASE_CUR && p->field != WX_FIELD_WATER_CUR) {
    *why = "field: WX_FIELD_BASE_CUR or WX_FIELD_WATER_CUR (the fields that are stored whole and interleaved)";
    return WX_E_INVALID;
  }
  if (p->mode != WX_INFLATE_CONST && p->mode != WX_INFLATE_RTPS && p->mode != WX_INFLATE_RTPP) {
    *why = "mode: WX_INFLATE_CONST, WX_INFLATE_RTPS or WX_INFLATE_RTPP";
    return WX_E_INVALID;
  }
  for (int c = 0; c < 4; c++) {
    if (!f32_finite(p->coef[c]) || p->coef[c] < 0.0f) {
      *why = "coef: finite, >= 0";
      return WX_E_INVALID;
    }
    if (p->mode == WX_INFLATE_RTPP && p->coef[c] > 1.0f) {
      *why = "coef: an RTPP alpha lies in [0, 1]";
      return WX_E_INVALID;
    }
  }
  if (p->mode == WX_INFLATE_RTPP && p->lambda_out) {
    *why = "lambda_out: RTPP applies no single factor";
    return WX_E_INVALID;
  }
  return WX_OK;
}
inline int check_rect(const wx_ens_inflate *p, int X, int Y, const char **why)
{
  *why = "";
  if (p->w <= 0 || p->h <= 0 || p->x < 0 || p->y < 0 || (long long)p->x + p->w > X || (long long)p->y + p->h > Y) {
    *why = "the rectangle lies outside the grid (no wrap)";
    return WX_E_RANGE;
  }
  return WX_OK;
}

// host only, pure: the definition over n_cells cells held by the caller (the descriptor's rectangle is not looked at)
inline int inflate_cells(const wx_ens_inflate *p, int n_members, size_t n_cells, float *const *field, const int8_t *const *wall, const float *const *prior,
                         const uint8_t *mask)
{
  if (!p || n_members < 1 || !field || !wall) return WX_E_INVALID;
  const char *why;
  if (int rc = check_desc(p, &why)) return rc;
  const bool relax = p->mode != WX_INFLATE_CONST;
  if (relax && !prior) return WX_E_INVALID;
  std::vector<int> sel;
  for (int i = 0; i < n_members; i++) {
    if (mask && !mask[i]) continue;
    if (!field[i] || !wall[i] || (relax && !prior[i])) return WX_E_INVALID;
    sel.push_back(i);
  }
  const int n = (int)sel.size();
  if (n < 2) return WX_E_INVALID;
  std::vector<float> xs((size_t)n), ps((size_t)n, 0.0f);
  for (size_t cell = 0; cell < n_cells; cell++) {
    bool air = true;
    for (int k = 0; k < n; k++) air = air && wall[sel[k]][4 * cell + 1] != 0;
    for (int c = 0; c < 4; c++) {
      for (int k = 0; k < n; k++) {
        memcpy(&xs[k], field[sel[k]] + 4 * cell + c, 4);
        if (relax) memcpy(&ps[k], prior[sel[k]] + 4 * cell + c, 4);
      }
      float lam;
      if (inflate_channel(p->mode, p->coef[c], p->lambda_lo, p->lambda_hi, p->lo[c], p->hi[c], n, xs.data(), ps.data(), air, &lam))
        for (int k = 0; k < n; k++) memcpy(field[sel[k]] + 4 * cell + c, &xs[k], 4);
      if (p->lambda_out) p->lambda_out[4 * cell + c] = lam;
    }
  }
  return WX_OK;
}

} // namespace wxi
