// wx_ens_score_cell.h -- THE per-cell function of wx_ensemble_scores (include/wxsim.h: wx_ens_score) and the pure host entry point built
// on it, as plain C++ that a host compiler takes without the HIP headers (tests/native/ens_score_main.cpp compiles it under
// AddressSanitizer and UBSan); wx_ens_score.h includes it for the kernel. The values that enter are the quantile call's keys
// (wx_ens_quant_cell.h: cell_key, value_of, Tally) in ascending order -- how they got into that order is the implementation's business:
// a bitonic network in registers, std::sort --, and everything the definition asks for is read off that order by sum_step / dev_step /
// cell_finish below: the same program text on the host and on the device, two passes over i = 0 .. n-1. The five floats of a scored
// cell-channel go into wx_diag's integer bins (wxd::term_of) and are finished by its bins_to_double, so host and device meet in integers:
// the domain sums do not depend on the order of the cells either. Every function that rounds switches floating-point contraction off for
// itself (clang pragma; a gcc build passes -ffp-contract=off).
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/wxsim.h"
#include "wx_diag.h"
#include "wx_ens_quant_cell.h"
#include "wx_rounded.h"

namespace wxs {

using wxq::KEY_PAD;
using wxr::rounded;

enum { MAX_MEMBERS = 64, BINS = WX_ENS_SCORE_BINS, NT = 5 }; // NT: the five summed terms e, ae, se, vr, cr
static_assert(BINS == MAX_MEMBERS + 1, "n_below + n_equal reaches the number of selected members");
// why a cell-channel is not scored, in the order the definition tests them
enum { SCORED = 0, TRUTH_EXCLUDED, EMPTY, OVERFLOW_ };

// the truth's key: KEY_PAD if the cell is a wall cell in `truth` or its value is not finite
WX_HD inline uint32_t truth_key(float v, int wall_dist) { return wxq::rank_key(wxq::cell_key(v, wall_dist)); }

// the running sums over the ascending values, all starting at +0.0
struct Sums {
  double S, Q, A, G;
};
WX_HD inline void sums_init(Sums &s) { s.S = s.Q = s.A = s.G = 0.0; }
// pass 1, value i
WX_HD inline void sum_step(Sums &s, uint32_t key)
{
#pragma clang fp contract(off)
  s.S = s.S + (double)wxq::value_of(key);
}
// pass 2, value i of n, around the mean m = S / n and the truth t
WX_HD inline void dev_step(Sums &s, uint32_t key, int i, int n, double m, double t)
{
#pragma clang fp contract(off)
  const double v = (double)wxq::value_of(key);
  const double d = v - m;
  const double dd = rounded(d * d);
  s.Q = s.Q + dd;
  const double u = v - t;
  s.A = s.A + __builtin_fabs(u);
  const double gu = rounded((double)(2 * i - n + 1) * u);
  s.G = s.G + gu;
}
WX_HD inline double mean_of(const Sums &s, int n)
{
#pragma clang fp contract(off)
  return s.S / (double)n;
}

// one cell-channel's result
struct Cell {
  float f[NT]; // e, ae, se, vr, cr
  int reason;  // SCORED or why not
};
// n >= 1 ascending values summed into s, the truth t finite
WX_HD inline void five_of(const Sums &s, int n, double m, double t, float f[NT])
{
#pragma clang fp contract(off)
  const double err = m - t;
  const double var = s.Q / (double)n;
  const double nn = (double)n * (double)n;
  const double a = s.A / (double)n;
  const double g = s.G / nn;
  const double crps = a - g;
  const double sq = err * err; // (feeds a conversion, no sum: nothing a build could fuse it with)
  f[0] = (float)err, f[1] = (float)__builtin_fabs(err), f[2] = (float)sq, f[3] = (float)var, f[4] = (float)crps;
}
WX_HD inline int reason_of(uint32_t t_key, int n, const float f[NT])
{
  if (t_key == KEY_PAD) return TRUTH_EXCLUDED;
  if (n < 1) return EMPTY;
  bool fin = true;
  for (int k = 0; k < NT; k++) fin = fin && wxq::f32_finite(f[k]);
  return fin ? SCORED : OVERFLOW_;
}

// the argument checks wx_ensemble_scores and wx_ens_score_cells share (nothing here touches a device)
inline int check_selection(int n_members, const uint8_t *mask, const char **why)
{
  *why = "";
  int n_sel = 0;
  for (int i = 0; i < n_members; i++) n_sel += (!mask || mask[i]) ? 1 : 0;
  if (n_sel == 0) {
    *why = "the member mask selects nobody";
    return WX_E_INVALID;
  }
  if (n_sel > MAX_MEMBERS) {
    *why = "more than wx_ens_score_max_members() (64) members selected: the scores are taken over values sorted in registers";
    return WX_E_INVALID;
  }
  return WX_OK;
}

// the domain's accumulators: wx_diag's bins for the five terms of each channel, the counters, the histograms
struct Acc {
  int64_t hi[4][NT][wxd::NB];
  uint64_t lo[4][NT][wxd::NB];
  int64_t cnt[4][4]; // [reason][channel]
  int64_t sum_count[4];
  int64_t low[4][BINS], high[4][BINS];
};
inline void acc_norm(Acc &a)
{
  for (int c = 0; c < 4; c++)
    for (int k = 0; k < NT; k++)
      for (int b = 0; b < wxd::NB; b++) wxd::bin_norm(a.hi[c][k][b], a.lo[c][k][b]);
}
inline void acc_finish(Acc &a, wx_ens_score *out)
{
  acc_norm(a);
  double *sums[NT] = {out->sum_error, out->sum_abs_error, out->sum_sq_error, out->sum_variance, out->sum_crps};
  for (int c = 0; c < 4; c++) {
    out->n_scored[c] = a.cnt[SCORED][c], out->n_truth_excluded[c] = a.cnt[TRUTH_EXCLUDED][c];
    out->n_empty[c] = a.cnt[EMPTY][c], out->n_overflow[c] = a.cnt[OVERFLOW_][c];
    out->sum_count[c] = a.sum_count[c];
    for (int k = 0; k < NT; k++) sums[k][c] = wxd::bins_to_double(a.hi[c][k], a.lo[c][k]);
    for (int b = 0; b < BINS; b++) out->rank_low[c][b] = a.low[c][b], out->rank_high[c][b] = a.high[c][b];
  }
}

// host only, pure: the per-cell function over cells the caller holds
inline int score_cells(int n_members, size_t n_cells, const float *const *field, const int8_t *const *wall, const float *truth_field, const int8_t *truth_wall,
                       const uint8_t *mask, wx_ens_score *out)
{
  if (n_members < 1 || !field || !wall || !out) return WX_E_INVALID;
  const char *why;
  if (int rc = check_selection(n_members, mask, &why)) return rc;
  if (n_cells && (!truth_field || !truth_wall)) return WX_E_INVALID;
  for (int i = 0; i < n_members; i++)
    if ((!mask || mask[i]) && n_cells && (!field[i] || !wall[i])) return WX_E_INVALID;
  std::vector<uint32_t> keys;
  keys.reserve((size_t)n_members);
  Acc *acc = new Acc();
  memset(acc, 0, sizeof(*acc));
  const float nan = __builtin_nanf("");
  for (size_t i = 0; i < n_cells; i++) {
    for (int c = 0; c < 4; c++) {
      float v;
      memcpy(&v, truth_field + 4 * i + c, 4);
      const uint32_t t_key = truth_key(v, truth_wall[4 * i + 1]);
      keys.clear();
      wxq::Tally tl{0, 0, 0, 0};
      for (int k = 0; k < n_members; k++) {
        if (mask && !mask[k]) continue;
        memcpy(&v, field[k] + 4 * i + c, 4);
        const uint32_t key = wxq::cell_key(v, wall[k][4 * i + 1]);
        wxq::tally_add(tl, key, t_key);
        if (wxq::key_entered(key)) keys.push_back(key);
      }
      std::sort(keys.begin(), keys.end());
      const int n = tl.n;
      Cell r;
      for (int k = 0; k < NT; k++) r.f[k] = nan;
      if (t_key != KEY_PAD && n >= 1) {
        const double t = (double)wxq::value_of(t_key);
        Sums s;
        sums_init(s);
        for (int k = 0; k < n; k++) sum_step(s, keys[(size_t)k]);
        const double m = mean_of(s, n);
        for (int k = 0; k < n; k++) dev_step(s, keys[(size_t)k], k, n, m, t);
        five_of(s, n, m, t, r.f);
      }
      r.reason = reason_of(t_key, n, r.f);
      acc->cnt[r.reason][c] += 1;
      const bool scored = r.reason == SCORED;
      if (scored) {
        acc->sum_count[c] += n;
        acc->low[c][tl.below] += 1, acc->high[c][tl.below + tl.equal] += 1;
        for (int k = 0; k < NT; k++) {
          const wxd::Term tm = wxd::term_of(r.f[k], true);
          acc->lo[c][k][tm.bin] += (uint64_t)(uint32_t)tm.addend; // (a normalised low word + 2^20 addends' low words stay below 2^53)
          acc->hi[c][k][tm.bin] += tm.addend >> 32;
        }
      }
      if (out->error) out->error[4 * i + c] = scored ? r.f[0] : nan;
      if (out->variance) out->variance[4 * i + c] = scored ? r.f[3] : nan;
      if (out->crps) out->crps[4 * i + c] = scored ? r.f[4] : nan;
    }
    if ((i & 0xFFFFF) == 0xFFFFF) acc_norm(*acc);
  }
  acc_finish(*acc, out);
  delete acc;
  return WX_OK;
}

} // namespace wxs
