// wx_ens_gram_cell.h -- THE functions of wx_ensemble_gram (include/wxsim.h: wx_ens_gram) and the pure host entry point built on them, as
// plain C++ that a host compiler takes without the HIP headers (tests/native/ens_gram_main.cpp compiles it under AddressSanitizer and
// UBSan); wx_ens_gram.h includes it for the kernels. The members' Gram matrix over a rectangle: per cell-channel the first member walk
// of the covariance call (wxcell::sum_add), the centre (centre_of), the deviations (wxc::dev_of), the float term of a pair (term_of_pair)
// and the overflow test on the diagonal (diag_overflows); cell_devs strings them together over an array, and gram_cells IS the
// definition: cells x pairs into wx_diag's integer bins (wxd::term_of), normalised every 2^20 cells, finished by wxd::bins_to_double.
// Every function that rounds switches floating-point contraction off for itself, and the product passes through wxr::rounded.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/wxsim.h"
#include "wx_diag.h"
#include "wx_ens_cov_cell.h"
#include "wx_rounded.h"

namespace wxg {

using wxc::dev_of;
using wxcell::f32_finite;
using wxcell::sum_add;
using wxr::rounded;

enum { MAX_MEMBERS = WX_ENS_GRAM_MAX_MEMBERS };
// what became of a cell-channel, in the order the definition tests them
enum { ENTERED = 0, EXCLUDED, OVERFLOW_ };

// the centre from the first walk's sum
WX_HD inline double centre_of(double S, int n, int center)
{
#pragma clang fp contract(off)
  return center == WX_GRAM_CENTER_MEAN ? S / (double)n : 0.0;
}
// p_ab: one double product, then the C conversion (beyond the float range: +-Inf)
WX_HD inline float term_of_pair(double da, double db)
{
#pragma clang fp contract(off)
  return (float)rounded(da * db);
}
// the whole overflow test of a cell-channel is this, over its members (include/wxsim.h has the argument)
WX_HD inline bool diag_overflows(double d) { return !f32_finite(term_of_pair(d, d)); }

// the pairs a <= b of n members, row-major: (0,0) (0,1) .. (0,n-1) (1,1) ..
WX_HD inline int pair_count(int n) { return n * (n + 1) / 2; }
WX_HD inline int pair_index(int n, int a, int b) { return a * (2 * n - a + 1) / 2 + (b - a); }

// One channel of one cell over an array: x[0 .. n) the members' values, air: the cell is an air cell in all of them. ENTERED: d[0 .. n)
// holds the deviations and *xm the centre.
WX_HD inline int cell_devs(int n, const float *x, bool air, int center, double *d, double *xm)
{
#pragma clang fp contract(off)
  double S = 0.0;
  bool ok = true;
  for (int k = 0; k < n; k++) sum_add(S, ok, x[k], air);
  if (!ok) return EXCLUDED;
  *xm = centre_of(S, n, center);
  bool ovf = false;
  for (int k = 0; k < n; k++) {
    d[k] = dev_of(x[k], *xm);
    ovf = ovf || diag_overflows(d[k]);
  }
  return ovf ? OVERFLOW_ : ENTERED;
}

// the argument checks wx_ensemble_gram and wx_ens_gram_cells share (nothing here touches a device), in the order of the header
inline int check_desc(const wx_ens_gram *g, const char **why)
{
  *why = "";
  if (!wxc::state_field(g->field)) {
    *why = "field: WX_FIELD_BASE_CUR or WX_FIELD_WATER_CUR (the fields that are stored whole and interleaved)";
    return WX_E_INVALID;
  }
  if (g->center != WX_GRAM_CENTER_MEAN && g->center != WX_GRAM_CENTER_NONE) {
    *why = "center: WX_GRAM_CENTER_MEAN or WX_GRAM_CENTER_NONE";
    return WX_E_INVALID;
  }
  if (!g->gram) {
    *why = "gram is NULL";
    return WX_E_INVALID;
  }
  return WX_OK;
}
inline int check_selection(const wx_ens_gram *g, size_t n_sel, const char **why)
{
  *why = "";
  if (n_sel < (g->center == WX_GRAM_CENTER_MEAN ? 2u : 1u)) {
    *why = g->center == WX_GRAM_CENTER_MEAN ? "the member mask selects fewer than two members; deviations from a mean take two" : "the member mask selects nobody";
    return WX_E_INVALID;
  }
  if (n_sel > (size_t)MAX_MEMBERS) {
    *why = "more than wx_ens_gram_max_members() (64) members selected";
    return WX_E_INVALID;
  }
  return WX_OK;
}
inline int check_rect(const wx_ens_gram *g, int X, int Y, const char **why)
{
  *why = "";
  if (g->w <= 0 || g->h <= 0 || g->x < 0 || g->y < 0 || (long long)g->x + g->w > X || (long long)g->y + g->h > Y) {
    *why = "the rectangle lies outside the grid (no wrap)";
    return WX_E_RANGE;
  }
  return WX_OK;
}

// the rectangle's accumulators: wx_diag's bins per channel and pair, the counts
struct Acc {
  int n, pairs;
  std::vector<int64_t> hi;  // [channel][pair][bin]
  std::vector<uint64_t> lo;
  int64_t cnt[3][4]; // [ENTERED | EXCLUDED | OVERFLOW_][channel]
  explicit Acc(int n_) : n(n_), pairs(pair_count(n_)), hi((size_t)4 * pairs * wxd::NB, 0), lo((size_t)4 * pairs * wxd::NB, 0) { memset(cnt, 0, sizeof(cnt)); }
  size_t at(int c, int pair) const { return ((size_t)c * pairs + pair) * wxd::NB; }
};
inline void acc_norm(Acc &a)
{
  for (size_t i = 0; i < a.hi.size(); i++) wxd::bin_norm(a.hi[i], a.lo[i]);
}
inline void acc_finish(Acc &a, wx_ens_gram *g)
{
  acc_norm(a);
  const size_t n = (size_t)a.n;
  for (int c = 0; c < 4; c++) {
    g->n_entered[c] = a.cnt[ENTERED][c], g->n_excluded[c] = a.cnt[EXCLUDED][c], g->n_overflow[c] = a.cnt[OVERFLOW_][c];
    for (int i = 0; i < a.n; i++)
      for (int j = i; j < a.n; j++) {
        const size_t at = a.at(c, pair_index(a.n, i, j));
        const double v = wxd::bins_to_double(&a.hi[at], &a.lo[at]);
        g->gram[((size_t)c * n + i) * n + j] = g->gram[((size_t)c * n + j) * n + i] = v;
      }
  }
  g->n_selected = a.n, g->pad = 0;
}

// host only, pure: the definition over whole X x Y grids held by the caller
inline int gram_cells(wx_ens_gram *g, int X, int Y, int n_members, const float *const *field, const int8_t *const *wall, const uint8_t *mask)
{
  if (!g || n_members < 1 || !field || !wall || X < 1 || Y < 1) return WX_E_INVALID;
  const char *why;
  if (int rc = check_desc(g, &why)) return rc;
  std::vector<int> sel;
  for (int i = 0; i < n_members; i++) {
    if (mask && !mask[i]) continue;
    if (!field[i] || !wall[i]) return WX_E_INVALID;
    sel.push_back(i);
  }
  if (int rc = check_selection(g, sel.size(), &why)) return rc;
  if (int rc = check_rect(g, X, Y, &why)) return rc;
  const int n = (int)sel.size();
  Acc acc(n);
  float xs[MAX_MEMBERS];
  double d[MAX_MEMBERS], xm;
  size_t met = 0;
  for (int ry = 0; ry < g->h; ry++)
    for (int rx = 0; rx < g->w; rx++) {
      const size_t cell = (size_t)(g->y + ry) * (size_t)X + (size_t)(g->x + rx);
      bool air = true;
      for (int k = 0; k < n; k++) air = air && wall[sel[k]][4 * cell + 1] != 0;
      for (int c = 0; c < 4; c++) {
        for (int k = 0; k < n; k++) memcpy(&xs[k], field[sel[k]] + 4 * cell + c, 4);
        const int what = cell_devs(n, xs, air, g->center, d, &xm);
        acc.cnt[what][c] += 1;
        if (what != ENTERED) continue;
        size_t at = acc.at(c, 0);
        for (int a = 0; a < n; a++)
          for (int b = a; b < n; b++, at += wxd::NB) {
            const wxd::Term t = wxd::term_of(term_of_pair(d[a], d[b]), true);
            acc.lo[at + t.bin] += (uint64_t)(uint32_t)t.addend; // (a normalised low word + 2^20 addends' low words stay below 2^53)
            acc.hi[at + t.bin] += t.addend >> 32;
          }
      }
      if ((++met & 0xFFFFF) == 0) acc_norm(acc);
    }
  acc_finish(acc, g);
  return WX_OK;
}

} // namespace wxg
