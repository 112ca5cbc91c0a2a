// wx_ens_nbhd_cell.h -- THE definition of wx_ensemble_neighbourhood (include/wxsim.h: wx_ens_nbhd) as plain C++ that a host compiler
// takes without the HIP headers (tests/native/ens_nbhd_main.cpp compiles it under AddressSanitizer and UBSan); wx_ens_nbhd.h includes
// it for the kernels. Three pieces: the POINT function (point_add: does this member's value count, does the event hold), the packed
// counts the points pass leaves per cell (pack_f / pack_o), and the WINDOW function (window_cell: four integer window sums -> two
// fractions and three float terms). Between the two stand integer box sums, which the kernel forms separably in LDS and nbhd_cells below
// with prefix sums -- integers: how they are added is nobody's business. The three terms go into wx_diag's integer bins
// (wxd::term_of) and are finished by its bins_to_double, as wx_ens_score_cell.h's are. No product here feeds a sum (d*d, pf*pf, po*po
// each feed a conversion), so there is nothing a contracting build could fuse: no wx_rounded.h detour. The functions that round
// switch contraction off for themselves all the same (clang pragma; a gcc build passes -ffp-contract=off).
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/wxsim.h"
#include "wx_diag.h"

namespace wxn {

enum { MAX_RADIUS = WX_ENS_NBHD_MAX_RADIUS, MAX_SCALES = WX_ENS_NBHD_MAX_SCALES, NT = 3 }; // NT: the three summed terms d2, f2, o2
// the largest window sum: 4225 cells of at most 65535 members (wx_ensemble_create's limit)
static_assert((long long)(2 * MAX_RADIUS + 1) * (2 * MAX_RADIUS + 1) * 65535 < 0x7FFFFFFFll, "window sums fit int32");

// the event of one value (a NaN threshold: false both ways; -0.0 == 0.0)
WX_HD inline bool event_of(float v, float thr, int above) { return above ? v > thr : v < thr; }
// one member's (or the truth's) value of the channel and channel 1 of its wall texel: n counts it if it is an air cell with a finite
// value, ev if the event holds there too. Selects, no branches (the kernel's group of loads stays one basic block, as in wx_ens_stat.h)
WX_HD inline void point_add(unsigned &n, unsigned &ev, float v, int wall_dist, float thr, int above)
{
  const bool take = wall_dist != 0 && wxd::f32_finite(v);
  n += take ? 1u : 0u;
  ev += (take && event_of(v, thr, above)) ? 1u : 0u;
}
// what the points pass leaves per cell: Nf | Ef << 16 (both <= 65535) and, in a byte of its own, No | Eo << 1
WX_HD inline uint32_t pack_f(unsigned n, unsigned ev) { return n | (ev << 16); }
WX_HD inline uint8_t pack_o(unsigned n, unsigned ev) { return (uint8_t)(n | (ev << 1)); }

// one output cell of one scale
struct Cell {
  float pf, po;  // NaN where the window holds no counted cell
  float t[NT];   // d2, f2, o2 (meaningful where scored)
  bool scored;
};
WX_HD inline Cell window_cell(int Af, int Bf, int Ao, int Bo)
{
#pragma clang fp contract(off)
  Cell r;
  const float nan = __builtin_nanf("");
  r.scored = Bf > 0 && Bo > 0;
  const double pf = Bf > 0 ? (double)Af / (double)Bf : 0.0;
  const double po = Bo > 0 ? (double)Ao / (double)Bo : 0.0;
  const double d = pf - po;
  const double dd = d * d, ff = pf * pf, oo = po * po; // (each feeds a conversion, no sum)
  r.pf = Bf > 0 ? (float)pf : nan, r.po = Bo > 0 ? (float)po : nan;
  r.t[0] = (float)dd, r.t[1] = (float)ff, r.t[2] = (float)oo;
  return r;
}

// the argument checks wx_ensemble_neighbourhood and wx_ens_nbhd_cells share (nothing here touches a device), in the order of the header
inline int check_desc(const wx_ens_nbhd *a, bool have_truth, const char **why)
{
  *why = "";
  if (a->field != WX_FIELD_BASE_CUR && a->field != WX_FIELD_WATER_CUR) {
    *why = "field: WX_FIELD_BASE_CUR or WX_FIELD_WATER_CUR (the fields that are stored whole and interleaved)";
    return WX_E_INVALID;
  }
  if (a->channel < 0 || a->channel > 3) {
    *why = "channel outside 0 .. 3";
    return WX_E_INVALID;
  }
  if (a->n_scales < 1 || a->n_scales > MAX_SCALES) {
    *why = "n_scales outside 1 .. WX_ENS_NBHD_MAX_SCALES (8)";
    return WX_E_INVALID;
  }
  for (int s = 0; s < a->n_scales; s++)
    if (a->rx[s] < 0 || a->rx[s] > MAX_RADIUS || a->ry[s] < 0 || a->ry[s] > MAX_RADIUS) {
      *why = "a radius outside 0 .. wx_ens_nbhd_max_radius() (32)";
      return WX_E_INVALID;
    }
  if (!wxd::f32_finite(a->threshold) && !wxd::f32_nan(a->threshold)) {
    *why = "an infinite threshold (finite, or NaN for no event)";
    return WX_E_INVALID;
  }
  if (a->obs_fraction && !have_truth) {
    *why = "obs_fraction wanted without a truth";
    return WX_E_INVALID;
  }
  return WX_OK;
}
inline int check_range(const wx_ens_nbhd *a, int X, int Y, const char **why)
{
  *why = "";
  if (a->w <= 0 || a->h <= 0 || a->x < 0 || a->y < 0 || (long long)a->x + a->w > X || (long long)a->y + a->h > Y) {
    *why = "the rectangle lies outside the grid (no wrap)";
    return WX_E_RANGE;
  }
  if (a->wrap_x)
    for (int s = 0; s < a->n_scales; s++)
      if (2 * a->rx[s] + 1 > X) {
        *why = "wrap_x with a window wider than the grid: a cell would be counted twice";
        return WX_E_RANGE;
      }
  return WX_OK;
}

// the domain's accumulators: wx_diag's bins for the three terms of each scale, the counters
struct Acc {
  int64_t hi[MAX_SCALES][NT][wxd::NB];
  uint64_t lo[MAX_SCALES][NT][wxd::NB];
  int64_t scored[MAX_SCALES], unscored[MAX_SCALES];
  int64_t total[4]; // ev_f, n_f, ev_o, n_o
};
inline void acc_norm(Acc &a)
{
  for (int s = 0; s < MAX_SCALES; s++)
    for (int k = 0; k < NT; k++)
      for (int b = 0; b < wxd::NB; b++) wxd::bin_norm(a.hi[s][k][b], a.lo[s][k][b]);
}
inline void acc_finish(Acc &a, wx_ens_nbhd_result *out)
{
  acc_norm(a);
  memset(out, 0, sizeof(*out));
  double *sums[NT] = {out->sum_d2, out->sum_f2, out->sum_o2};
  for (int s = 0; s < MAX_SCALES; s++) {
    out->n_scored[s] = a.scored[s], out->n_unscored[s] = a.unscored[s];
    for (int k = 0; k < NT; k++) sums[k][s] = wxd::bins_to_double(a.hi[s][k], a.lo[s][k]);
  }
  out->ev_f = a.total[0], out->n_f = a.total[1], out->ev_o = a.total[2], out->n_o = a.total[3];
}

// host only, pure: the definition over whole grids the caller holds. The point counts of every cell, then per scale the box sums --
// per row a prefix sum and the window's one or two column ranges, per output column a prefix sum over the rows -- and the window function
inline int nbhd_cells(const wx_ens_nbhd *a, wx_ens_nbhd_result *out, int X, int Y, int n_members, const float *const *field, const int8_t *const *wall,
                      const float *truth_field, const int8_t *truth_wall, const uint8_t *mask)
{
  if (!a || !out || n_members < 1 || X < 1 || Y < 1 || !field || !wall) return WX_E_INVALID;
  if ((truth_field == nullptr) != (truth_wall == nullptr)) return WX_E_INVALID;
  const bool have_truth = truth_field != nullptr;
  const char *why;
  if (int rc = check_desc(a, have_truth, &why)) return rc;
  int n_sel = 0;
  for (int i = 0; i < n_members; i++) {
    if (mask && !mask[i]) continue;
    if (!field[i] || !wall[i]) return WX_E_INVALID;
    n_sel++;
  }
  if (n_sel == 0) return WX_E_INVALID;
  if (int rc = check_range(a, X, Y, &why)) return rc;

  // the point counts of the grid: [Ef, Nf, Eo, No]
  const size_t cells = (size_t)X * (size_t)Y;
  std::vector<uint32_t> cnt[4];
  for (int q = 0; q < 4; q++) cnt[q].assign(cells, 0u);
  for (size_t i = 0; i < cells; i++) {
    unsigned n = 0, ev = 0, no = 0, eo = 0;
    float v;
    for (int k = 0; k < n_members; k++) {
      if (mask && !mask[k]) continue;
      memcpy(&v, field[k] + 4 * i + a->channel, 4);
      point_add(n, ev, v, wall[k][4 * i + 1], a->threshold, a->above);
    }
    if (have_truth) {
      memcpy(&v, truth_field + 4 * i + a->channel, 4);
      point_add(no, eo, v, truth_wall[4 * i + 1], a->threshold, a->above);
    }
    cnt[0][i] = ev, cnt[1][i] = n, cnt[2][i] = eo, cnt[3][i] = no;
  }

  Acc *acc = new Acc();
  memset(acc, 0, sizeof(*acc));
  const int x = a->x, y = a->y, w = a->w, h = a->h;
  for (int j = 0; j < h; j++)
    for (int i = 0; i < w; i++) {
      const size_t g = (size_t)(y + j) * X + (size_t)(x + i);
      for (int q = 0; q < 4; q++) acc->total[q] += (int64_t)cnt[q][g];
    }
  std::vector<int64_t> P((size_t)X + 1), V;
  std::vector<int32_t> H[4];
  size_t since_norm = 0;
  for (int s = 0; s < a->n_scales; s++) {
    const int rx = a->rx[s], ry = a->ry[s];
    const int r0 = std::max(0, y - ry), r1 = std::min(Y, y + h + ry); // the rows any window of the rectangle reaches
    const size_t rows = (size_t)(r1 - r0);
    for (int q = 0; q < 4; q++) {
      H[q].assign(rows * (size_t)w, 0);
      for (int r = r0; r < r1; r++) {
        const uint32_t *row = cnt[q].data() + (size_t)r * X;
        P[0] = 0;
        for (int c = 0; c < X; c++) P[(size_t)c + 1] = P[(size_t)c] + (int64_t)row[c];
        for (int i = 0; i < w; i++) {
          int lo = x + i - rx, hi = x + i + rx;
          int64_t sum;
          if (!a->wrap_x) {
            lo = std::max(lo, 0), hi = std::min(hi, X - 1);
            sum = P[(size_t)hi + 1] - P[(size_t)lo];
          } else if (lo < 0) { // (2 rx + 1 <= X: the two ranges do not meet)
            sum = (P[(size_t)X] - P[(size_t)(lo + X)]) + P[(size_t)hi + 1];
          } else if (hi >= X) {
            sum = (P[(size_t)X] - P[(size_t)lo]) + P[(size_t)(hi - X) + 1];
          } else {
            sum = P[(size_t)hi + 1] - P[(size_t)lo];
          }
          H[q][(size_t)(r - r0) * (size_t)w + (size_t)i] = (int32_t)sum;
        }
      }
    }
    V.assign(4 * (rows + 1), 0);
    for (int i = 0; i < w; i++) {
      for (int q = 0; q < 4; q++) {
        int64_t *v = V.data() + (size_t)q * (rows + 1);
        for (size_t r = 0; r < rows; r++) v[r + 1] = v[r] + (int64_t)H[q][r * (size_t)w + (size_t)i];
      }
      for (int j = 0; j < h; j++) {
        const int lo = std::max(y + j - ry, r0), hi = std::min(y + j + ry, r1 - 1);
        int box[4];
        for (int q = 0; q < 4; q++) {
          const int64_t *v = V.data() + (size_t)q * (rows + 1);
          box[q] = (int)(v[(size_t)(hi - r0) + 1] - v[(size_t)(lo - r0)]);
        }
        const Cell c = window_cell(box[0], box[1], box[2], box[3]);
        const size_t o = ((size_t)s * (size_t)h + (size_t)j) * (size_t)w + (size_t)i;
        if (a->nep) a->nep[o] = c.pf;
        if (a->obs_fraction) a->obs_fraction[o] = c.po;
        if (!c.scored) {
          acc->unscored[s] += 1;
          continue;
        }
        acc->scored[s] += 1;
        for (int k = 0; k < NT; k++) {
          const wxd::Term tm = wxd::term_of(c.t[k], true);
          acc->lo[s][k][tm.bin] += (uint64_t)(uint32_t)tm.addend; // (a normalised low word + 2^20 addends' low words stay below 2^53)
          acc->hi[s][k][tm.bin] += tm.addend >> 32;
        }
        if (++since_norm == 0x100000) acc_norm(*acc), since_norm = 0;
      }
    }
  }
  acc_finish(*acc, out);
  delete acc;
  return WX_OK;
}

} // namespace wxn
