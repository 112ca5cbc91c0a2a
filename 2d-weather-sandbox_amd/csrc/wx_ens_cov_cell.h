// wx_ens_cov_cell.h -- THE functions of wx_ensemble_covariance (include/wxsim.h: wx_ens_cov, wx_ens_cov_pred, wx_ens_cov_result) and the
// pure host entry point built on them, as plain C++ that a host compiler takes without the HIP headers (tests/native/ens_cov_main.cpp
// compiles it under AddressSanitizer and UBSan); wx_ens_cov.h includes it for the kernels. The sample covariance, over the members,
// between every cell-channel of a rectangle and up to WX_ENS_COV_MAX scalar predictors, with the correlation and the regression slope
// (the ensemble sensitivity of Torn and Hakim 2008) that go with it: the predictor's chain (pred_of), the member walks of one channel
// of one cell (sum_add, q_add, c_add), the finishers (variance_of, cov_of, slope_of, corr_of); cov_channel strings them together over
// an array and cov_cells IS the definition. Every function that rounds switches floating-point contraction off for itself, every
// operation is a separate double operation, and a product that feeds a sum passes through wxr::rounded.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/wxsim.h"
#include "wx_rounded.h"
#include "wx_ens_cell_common.h"
#include <vector>

namespace wxc {

using wxr::rounded;

using wxcell::f32_bits;
using wxcell::f32_finite;
using wxcell::f64_finite;
WX_HD inline double f64_nan() { return (double)__builtin_nanf(""); }

// ---- a predictor: the chain over its n values t[0 .. n), member order ----
struct Pred {
  double mean, Q; // jm, Qj
  bool valid;
};
// t: one double per selected member (a point's value converted, or the host's number); a t that is not finite makes the predictor
// invalid (the caller turns "wall in this member" into such a t). e[0 .. n) receives e_k = t_k - jm (0 if invalid); e may be t.
WX_HD inline Pred pred_of(int n, const double *t, double *e)
{
#pragma clang fp contract(off)
  Pred p;
  bool ok = true;
  double S = 0.0;
  for (int k = 0; k < n; k++) {
    ok = ok && f64_finite(t[k]);
    S = S + t[k];
  }
  if (!ok) {
    for (int k = 0; k < n; k++) e[k] = 0.0;
    p.valid = false, p.mean = p.Q = f64_nan();
    return p;
  }
  p.valid = true;
  p.mean = S / (double)n;
  double Q = 0.0;
  for (int k = 0; k < n; k++) {
    const double ek = t[k] - p.mean;
    e[k] = ek;
    Q = Q + rounded(ek * ek);
  }
  p.Q = Q;
  return p;
}
WX_HD inline void result_of(wx_ens_cov_result &r, const Pred &p, int n)
{
#pragma clang fp contract(off)
  r.valid = p.valid ? 1 : 0, r.pad = 0;
  r.mean = p.mean;
  r.variance = p.valid ? p.Q / (double)(n - 1) : f64_nan();
}

// ---- one channel of one cell, member by member (the kernel keeps four of each; selects, not branches, as wx_ens_stat.h's cell_add) ----
// walk 1: Sx, and whether every member's value may enter (wx_ens_cell_common.h)
using wxcell::sum_add;
// walk 2: Qx and one Cq_j per predictor, from the same d_k
WX_HD inline double dev_of(float x, double xm)
{
#pragma clang fp contract(off)
  return (double)x - xm;
}
WX_HD inline void q_add(double &Q, double d)
{
#pragma clang fp contract(off)
  Q = Q + rounded(d * d);
}
WX_HD inline void c_add(double &Cq, double d, double e)
{
#pragma clang fp contract(off)
  Cq = Cq + rounded(d * e);
}
// the finishers (a double beyond the float range converts to +-Inf)
WX_HD inline float variance_of(double Qx, int n)
{
#pragma clang fp contract(off)
  return (float)(Qx / (double)(n - 1));
}
WX_HD inline float cov_of(double Cq, int n)
{
#pragma clang fp contract(off)
  return (float)(Cq / (double)(n - 1));
}
WX_HD inline float slope_of(double Cq, double Qx)
{
#pragma clang fp contract(off)
  return Qx == 0.0 ? __builtin_nanf("") : (float)(Cq / Qx);
}
WX_HD inline float corr_of(double Cq, double Qx, double Qj)
{
#pragma clang fp contract(off)
  const double den = __builtin_sqrt(rounded(Qx * Qj));
  if (den == 0.0) return __builtin_nanf("");
  double r = Cq / den;
  if (r < -1.0) r = -1.0;
  if (r > 1.0) r = 1.0;
  return (float)r;
}

// The whole walk over an array: x[0 .. n) the members' values of one channel of one cell, air: the cell is an air cell in all of them,
// p[j] / e[j * n + k] the predictors. variance: one float or NULL; cov / corr / slope: n_pred floats each or NULL.
WX_HD inline void cov_channel(int n, const float *x, bool air, int n_pred, const Pred *p, const double *e, float *variance, float *cov, float *corr,
                               float *slope)
{
#pragma clang fp contract(off)
  const float nan = __builtin_nanf("");
  double S = 0.0;
  bool ok = true;
  for (int k = 0; k < n; k++) sum_add(S, ok, x[k], air);
  if (!ok) {
    if (variance) *variance = nan;
    for (int j = 0; j < n_pred; j++) {
      if (cov) cov[j] = nan;
      if (corr) corr[j] = nan;
      if (slope) slope[j] = nan;
    }
    return;
  }
  const double xm = S / (double)n;
  double Qx = 0.0, Cq[WX_ENS_COV_MAX];
  for (int j = 0; j < n_pred; j++) Cq[j] = 0.0;
  for (int k = 0; k < n; k++) {
    const double d = dev_of(x[k], xm);
    q_add(Qx, d);
    for (int j = 0; j < n_pred; j++) c_add(Cq[j], d, e[(size_t)j * (size_t)n + (size_t)k]);
  }
  if (variance) *variance = variance_of(Qx, n);
  for (int j = 0; j < n_pred; j++) {
    if (cov) cov[j] = p[j].valid ? cov_of(Cq[j], n) : nan;
    if (corr) corr[j] = p[j].valid ? corr_of(Cq[j], Qx, p[j].Q) : nan;
    if (slope) slope[j] = p[j].valid ? slope_of(Cq[j], Qx) : nan;
  }
}

// the argument checks wx_ensemble_covariance and wx_ens_cov_cells share (nothing here touches a device)
inline bool state_field(int f) { return f == WX_FIELD_BASE_CUR || f == WX_FIELD_WATER_CUR; }
inline int check_desc(const wx_ens_cov *c, const wx_ens_cov_pred *pred, const char **why)
{
  *why = "";
  if (!state_field(c->field)) {
    *why = "field: WX_FIELD_BASE_CUR or WX_FIELD_WATER_CUR (the fields that are stored whole and interleaved)";
    return WX_E_INVALID;
  }
  if (c->source != WX_COV_SOURCE_CURRENT && c->source != WX_COV_SOURCE_PRIOR) {
    *why = "source: WX_COV_SOURCE_CURRENT or WX_COV_SOURCE_PRIOR";
    return WX_E_INVALID;
  }
  if (c->n_pred < 1 || c->n_pred > WX_ENS_COV_MAX) {
    *why = "n_pred: 1 .. WX_ENS_COV_MAX";
    return WX_E_INVALID;
  }
  for (int j = 0; j < c->n_pred; j++) {
    const wx_ens_cov_pred &q = pred[j];
    if (q.kind == WX_COV_PRED_POINT) {
      if (!state_field(q.field)) {
        *why = "a point predictor's field: WX_FIELD_BASE_CUR or WX_FIELD_WATER_CUR";
        return WX_E_INVALID;
      }
      if (q.channel < 0 || q.channel > 3) {
        *why = "a point predictor's channel: 0 .. 3";
        return WX_E_INVALID;
      }
    } else if (q.kind == WX_COV_PRED_VALUES) {
      if (!q.values) {
        *why = "a values predictor's array is NULL";
        return WX_E_INVALID;
      }
    } else {
      *why = "a predictor's kind: WX_COV_PRED_POINT or WX_COV_PRED_VALUES";
      return WX_E_INVALID;
    }
  }
  return WX_OK;
}
// the host's numbers of the selected members: finite and inside the float range
inline int check_values(const wx_ens_cov *c, const wx_ens_cov_pred *pred, const std::vector<int> &sel, const char **why)
{
  *why = "";
  const double fmax = 3.4028234663852886e38;
  for (int j = 0; j < c->n_pred; j++) {
    if (pred[j].kind != WX_COV_PRED_VALUES) continue;
    for (int i : sel) {
      const double v = pred[j].values[i];
      if (!f64_finite(v) || v > fmax || v < -fmax) {
        *why = "a values predictor's entry of a selected member: finite, |v| <= FLT_MAX";
        return WX_E_INVALID;
      }
    }
  }
  return WX_OK;
}
inline int check_rect(const wx_ens_cov *c, const wx_ens_cov_pred *pred, int X, int Y, const char **why)
{
  *why = "";
  if (c->w <= 0 || c->h <= 0 || c->x < 0 || c->y < 0 || (long long)c->x + c->w > X || (long long)c->y + c->h > Y) {
    *why = "the rectangle lies outside the grid (no wrap)";
    return WX_E_RANGE;
  }
  for (int j = 0; j < c->n_pred; j++)
    if (pred[j].kind == WX_COV_PRED_POINT && (pred[j].x < 0 || pred[j].y < 0 || pred[j].x >= X || pred[j].y >= Y)) {
      *why = "a point predictor lies outside the grid";
      return WX_E_RANGE;
    }
  return WX_OK;
}

// host only, pure: the definition over whole X x Y grids held by the caller (a point may lie outside the rectangle); prior[i]: the w * h
// cells of the rectangle, looked at with WX_COV_SOURCE_PRIOR only
inline int cov_cells(const wx_ens_cov *c, const wx_ens_cov_pred *pred, wx_ens_cov_result *result, int X, int Y, int n_members, const float *const *base,
                     const float *const *water, const int8_t *const *wall, const float *const *prior, const uint8_t *mask)
{
  if (!c || !pred || n_members < 1 || !wall || X < 1 || Y < 1) return WX_E_INVALID;
  const char *why;
  if (int rc = check_desc(c, pred, &why)) return rc;
  const bool from_prior = c->source == WX_COV_SOURCE_PRIOR;
  bool need[2] = {false, false}; // base, water
  if (!from_prior) need[c->field == WX_FIELD_BASE_CUR ? 0 : 1] = true;
  for (int j = 0; j < c->n_pred; j++)
    if (pred[j].kind == WX_COV_PRED_POINT) need[pred[j].field == WX_FIELD_BASE_CUR ? 0 : 1] = true;
  if ((need[0] && !base) || (need[1] && !water) || (from_prior && !prior)) return WX_E_INVALID;
  std::vector<int> sel;
  for (int i = 0; i < n_members; i++) {
    if (mask && !mask[i]) continue;
    if (!wall[i] || (need[0] && !base[i]) || (need[1] && !water[i]) || (from_prior && !prior[i])) return WX_E_INVALID;
    sel.push_back(i);
  }
  const int n = (int)sel.size();
  if (n < 2) return WX_E_INVALID;
  if (int rc = check_values(c, pred, sel, &why)) return rc;
  if (int rc = check_rect(c, pred, X, Y, &why)) return rc;

  const int n_pred = c->n_pred;
  std::vector<double> e((size_t)n_pred * (size_t)n);
  Pred p[WX_ENS_COV_MAX];
  for (int j = 0; j < n_pred; j++) {
    const wx_ens_cov_pred &q = pred[j];
    double *t = e.data() + (size_t)j * (size_t)n;
    for (int k = 0; k < n; k++) {
      if (q.kind == WX_COV_PRED_VALUES) {
        t[k] = q.values[sel[k]];
      } else {
        const size_t cell = (size_t)q.y * (size_t)X + (size_t)q.x;
        float v;
        memcpy(&v, (q.field == WX_FIELD_BASE_CUR ? base : water)[sel[k]] + 4 * cell + q.channel, 4);
        t[k] = wall[sel[k]][4 * cell + 1] != 0 ? (double)v : f64_nan();
      }
    }
    p[j] = pred_of(n, t, t);
    if (result) result_of(result[j], p[j], n);
  }
  const size_t plane = (size_t)c->w * (size_t)c->h * 4;
  std::vector<float> xs((size_t)n);
  float cv[WX_ENS_COV_MAX], cr[WX_ENS_COV_MAX], sl[WX_ENS_COV_MAX];
  for (int ry = 0; ry < c->h; ry++)
    for (int rx = 0; rx < c->w; rx++) {
      const size_t cell = (size_t)(c->y + ry) * (size_t)X + (size_t)(c->x + rx), rcell = (size_t)ry * (size_t)c->w + (size_t)rx;
      bool air = true;
      for (int k = 0; k < n; k++) air = air && wall[sel[k]][4 * cell + 1] != 0;
      for (int ch = 0; ch < 4; ch++) {
        for (int k = 0; k < n; k++) {
          const float *src = from_prior ? prior[sel[k]] + 4 * rcell : (c->field == WX_FIELD_BASE_CUR ? base : water)[sel[k]] + 4 * cell;
          memcpy(&xs[k], src + ch, 4);
        }
        float var;
        cov_channel(n, xs.data(), air, n_pred, p, e.data(), &var, cv, cr, sl);
        if (c->variance) c->variance[4 * rcell + ch] = var;
        for (int j = 0; j < n_pred; j++) {
          if (c->cov) c->cov[(size_t)j * plane + 4 * rcell + ch] = cv[j];
          if (c->corr) c->corr[(size_t)j * plane + 4 * rcell + ch] = cr[j];
          if (c->slope) c->slope[(size_t)j * plane + 4 * rcell + ch] = sl[j];
        }
      }
    }
  return WX_OK;
}

} // namespace wxc
