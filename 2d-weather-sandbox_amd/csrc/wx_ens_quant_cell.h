// wx_ens_quant_cell.h -- THE per-cell function of wx_ensemble_quantiles (include/wxsim.h: wx_ens_quant) and the pure host entry point
// built on it, as plain C++ that a host compiler takes without the HIP headers (tests/native/ens_quant_main.cpp compiles it under
// AddressSanitizer and UBSan); wx_ens_quant.h includes it for the kernels. A value that enters is turned into its KEY -- the
// order-preserving uint32 of the float with -0.0 taken as +0.0 --, the keys of a cell and channel are put in ascending order (how is
// the implementation's business: a bitonic network in LDS, a radix select, std::sort), and everything the definition asks for is read
// off that order: the function of the order statistics is position_of / quantile_of / the three counters of Tally below, and those are
// the same program text everywhere. No sums in member order occur: the result does not depend on the order of the members. Every
// function that rounds switches floating-point contraction off for itself (clang pragma; a gcc build passes -ffp-contract=off).
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/wxsim.h"
#include "wx_rounded.h"
#include "wx_ens_cell_common.h"

namespace wxq {

using wxcell::f32_bits;
using wxcell::f32_finite;
WX_HD inline float f32_of(uint32_t u)
{
  float v;
  memcpy(&v, &u, 4);
  return v;
}

// Keys. A finite float's key: sign bit flipped for v >= 0, all bits flipped for v < 0 -- unsigned order == float order, equal floats
// have equal keys once -0.0 is +0.0. The largest finite key is 0xFF7FFFFF (FLT_MAX); the three values at the top of the range are the
// keys of NaN bit patterns, never of a value that enters, and stand for what does NOT enter. They sort behind every finite key, so
// v(0) .. v(n-1) are the first n of the ascending order, and the three can still be told apart: the number of KEY_WALL in a column is
// n_wall without a second array.
enum : uint32_t {
  KEY_PAD = 0xFFFFFFFDu,       // no member here (the staged path pads the selection to a power of two; a lane outside the rectangle)
  KEY_NONFINITE = 0xFFFFFFFEu, // NaN, +Inf, -Inf in an air cell
  KEY_WALL = 0xFFFFFFFFu,      // the cell is a wall cell in this member
};
WX_HD inline uint32_t key_of(float v) // v finite
{
  uint32_t u = f32_bits(v);
  u = (u << 1) == 0u ? 0u : u; // -0.0 is taken as +0.0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
WX_HD inline float value_of(uint32_t key) { return f32_of((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key); }
WX_HD inline bool key_entered(uint32_t key) { return key < KEY_PAD; }
// one member's value of a cell and channel; wall_dist = channel 1 of its WX_FIELD_WALL_CUR texel
WX_HD inline uint32_t cell_key(float v, int wall_dist) { return wall_dist == 0 ? (uint32_t)KEY_WALL : (f32_finite(v) ? key_of(v) : (uint32_t)KEY_NONFINITE); }

using wxr::rounded; // (wx_rounded.h: a product that feeds a sum or a difference is a value of its own, in every build)

// where quantile p lies among n >= 1 ascending values: v(k), v(k1) and the weight g of the second
struct Position {
  int k, k1;
  double g;
};
WX_HD inline Position position_of(float p, int n)
{
#pragma clang fp contract(off)
  const double h = rounded((double)p * (double)(n - 1)); // one rounded product; 0 <= h <= n - 1 for p in [0, 1]
  const double kf = __builtin_floor(h);
  Position q;
  q.k = (int)kf;
  q.g = h - kf; // (exact)
  q.k1 = q.k + 1 < n ? q.k + 1 : n - 1;
  return q;
}
// the quantile from the two order statistics
WX_HD inline float quantile_of(int interp, float vk, float vk1, double g)
{
#pragma clang fp contract(off)
  if (interp == WX_QUANT_LOWER) return vk;
  if (interp == WX_QUANT_HIGHER) return g > 0.0 ? vk1 : vk;
  const double d = (double)vk1 - (double)vk;
  const double gd = rounded(g * d);
  const double s = (double)vk + gd;
  return (float)s;
}

// what one pass over a cell's keys (in any order) counts. With a rank member: t_key = the key of its value, or KEY_PAD if the cell is
// wall in it or its value is not finite (rank_count then answers -1 whatever was counted)
struct Tally {
  int n, n_wall, below, equal;
};
WX_HD inline void tally_add(Tally &t, uint32_t key, uint32_t t_key)
{
  t.n += key_entered(key) ? 1 : 0;
  t.n_wall += key == KEY_WALL ? 1 : 0;
  t.below += key < t_key ? 1 : 0;
  t.equal += key == t_key ? 1 : 0;
}
WX_HD inline uint32_t rank_key(uint32_t member_key) { return key_entered(member_key) ? member_key : (uint32_t)KEY_PAD; }
WX_HD inline int rank_count(uint32_t t_key, int c) { return t_key == KEY_PAD ? -1 : c; }

// the argument checks wx_ensemble_quantiles and wx_ens_quant_cells share (nothing here touches a device). n_members: of the ensemble /
// of the tables; mask: NULL = all
inline int check_desc(const wx_ens_quant *o, int n_members, const uint8_t *mask, const char **why)
{
  *why = "";
  if (o->n_q < 0 || o->n_q > WX_ENS_QUANT_MAX) {
    *why = "n_q: 0 .. WX_ENS_QUANT_MAX";
    return WX_E_INVALID;
  }
  if (o->n_q > 0 && !o->q) {
    *why = "n_q > 0 without a q array";
    return WX_E_INVALID;
  }
  for (int j = 0; j < o->n_q; j++)
    if (!(o->p[j] >= 0.0f && o->p[j] <= 1.0f)) {
      *why = "p: every quantile is a number in [0, 1]";
      return WX_E_INVALID;
    }
  if (o->interp != WX_QUANT_LINEAR && o->interp != WX_QUANT_LOWER && o->interp != WX_QUANT_HIGHER) {
    *why = "interp: WX_QUANT_LINEAR, WX_QUANT_LOWER or WX_QUANT_HIGHER";
    return WX_E_INVALID;
  }
  int n_sel = 0;
  for (int i = 0; i < n_members; i++) n_sel += (!mask || mask[i]) ? 1 : 0;
  if (n_sel == 0) {
    *why = "the member mask selects nobody";
    return WX_E_INVALID;
  }
  if (o->rank_member < -1 || o->rank_member >= n_members) {
    *why = "rank_member: -1 or a member of the ensemble";
    return WX_E_INVALID;
  }
  if (o->rank_member >= 0 && (!mask || mask[o->rank_member])) {
    *why = "rank_member is selected: the member that is ranked does not enter (mask it out)";
    return WX_E_INVALID;
  }
  if (o->rank_member < 0 && (o->n_below || o->n_equal)) {
    *why = "n_below / n_equal without a rank_member";
    return WX_E_INVALID;
  }
  return WX_OK;
}

// host only, pure: the per-cell function over cells the caller holds
inline int quant_cells(int n_members, size_t n_cells, const float *const *field, const int8_t *const *wall, const uint8_t *mask, wx_ens_quant *out)
{
  if (n_members < 1 || !field || !wall || !out) return WX_E_INVALID;
  const char *why;
  if (int rc = check_desc(out, n_members, mask, &why)) return rc;
  for (int i = 0; i < n_members; i++) {
    const bool used = !mask || mask[i] || i == out->rank_member;
    if (used && n_cells && (!field[i] || !wall[i])) return WX_E_INVALID;
  }
  std::vector<uint32_t> keys;
  keys.reserve((size_t)n_members);
  const int r = out->rank_member;
  for (size_t i = 0; i < n_cells; i++) {
    int n_wall = 0;
    for (int c = 0; c < 4; c++) {
      float v;
      uint32_t t_key = KEY_PAD;
      if (r >= 0) {
        memcpy(&v, field[r] + 4 * i + c, 4);
        t_key = rank_key(cell_key(v, wall[r][4 * i + 1]));
      }
      keys.clear();
      Tally t{0, 0, 0, 0};
      for (int k = 0; k < n_members; k++) {
        if (mask && !mask[k]) continue;
        memcpy(&v, field[k] + 4 * i + c, 4);
        const uint32_t key = cell_key(v, wall[k][4 * i + 1]);
        tally_add(t, key, t_key);
        if (key_entered(key)) keys.push_back(key);
      }
      std::sort(keys.begin(), keys.end());
      n_wall = t.n_wall;
      for (int j = 0; j < out->n_q; j++) {
        float q = __builtin_nanf("");
        if (t.n > 0) {
          const Position ps = position_of(out->p[j], t.n);
          q = quantile_of(out->interp, value_of(keys[(size_t)ps.k]), value_of(keys[(size_t)ps.k1]), ps.g);
        }
        out->q[((size_t)j * n_cells + i) * 4 + c] = q;
      }
      if (out->count) out->count[4 * i + c] = t.n;
      if (out->n_below) out->n_below[4 * i + c] = rank_count(t_key, t.below);
      if (out->n_equal) out->n_equal[4 * i + c] = rank_count(t_key, t.equal);
    }
    if (out->n_wall) out->n_wall[i] = n_wall;
  }
  return WX_OK;
}

} // namespace wxq
