// wx_ens_perturb_cell.h -- THE per-cell function of wx_ensemble_perturb (include/wxsim.h: wx_ens_perturb) and the pure host entry point
// built on it, as plain C++ that a host compiler takes without the HIP headers (tests/native/ens_perturb_main.cpp compiles it under
// AddressSanitizer and UBSan); wx_ens_perturb.h includes it for the kernel. Every function that rounds switches floating-point
// contraction off for itself (clang pragma; a gcc build passes -ffp-contract=off), every operation is a separate double operation.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/wxsim.h"
#include "wx_rounded.h"
#include "wx_ens_cell_common.h"

namespace wxp {

using wxcell::f32_bits;
using wxcell::f32_finite;

using wxr::rounded; // (wx_rounded.h: a product that feeds a sum is a value of its own, in every build)

// the shaders' integer hash (common.glsl:103-111; wx_kernels.h hash_u32), here for the host as well
WX_HD inline uint32_t hash32(uint32_t x)
{
  x += (x << 10u);
  x ^= (x >> 6u);
  x += (x << 3u);
  x ^= (x >> 11u);
  x += (x << 15u);
  return x;
}

// what does not depend on the cell
struct Noise {
  int X;          // cells per row of the grid (the period of the noise with wrap_x)
  int mode, scale, wrap_x;
  uint32_t seed_h; // hash32(seed)
  float amp[4], lo[4], hi[4];
};

inline Noise noise_of(const wx_ens_perturb &p, int X)
{
  Noise n;
  n.X = X, n.mode = p.mode, n.scale = p.scale, n.wrap_x = p.wrap_x ? 1 : 0;
  n.seed_h = hash32(p.seed);
  for (int c = 0; c < 4; c++) n.amp[c] = p.amplitude[c], n.lo[c] = p.lo[c], n.hi[c] = p.hi[c];
  return n;
}

// value of lattice node (gx, gy) for (member, channel): 24 hashed bits as a double in [-1, 1)
WX_HD inline double node_value(uint32_t seed_h, int member, int c, uint32_t gx, uint32_t gy)
{
#pragma clang fp contract(off)
  const uint32_t h = hash32(gx + hash32(gy + hash32(4u * (uint32_t)member + (uint32_t)c + seed_h)));
  return ((double)(h >> 8) - 8388608.0) / 8388608.0;
}

// where cell (x, y) lies on the lattice: the four nodes and the two weights. The same for every member and channel
struct Lattice {
  uint32_t gx0, gx1, gy0, gy1;
  double tx, ty;
};
WX_HD inline Lattice lattice_of(const Noise &n, int x, int y)
{
#pragma clang fp contract(off)
  Lattice l;
  const int gx = x / n.scale, gy = y / n.scale;
  int lenx = n.scale;
  l.gx0 = (uint32_t)gx, l.gx1 = (uint32_t)gx + 1u;
  if (n.wrap_x && gx == (n.X - 1) / n.scale) { // the last node interval of a row: as long as what is left of the row, closed by node 0
    lenx = n.X - gx * n.scale;
    l.gx1 = 0u;
  }
  l.gy0 = (uint32_t)gy, l.gy1 = (uint32_t)gy + 1u;
  l.tx = (double)(x - gx * n.scale) / (double)lenx;
  l.ty = (double)(y - gy * n.scale) / (double)n.scale;
  return l;
}

// r of the header: every operation rounded to double separately
WX_HD inline double noise_at(const Noise &n, const Lattice &l, int member, int c)
{
#pragma clang fp contract(off)
  const double u00 = node_value(n.seed_h, member, c, l.gx0, l.gy0), u10 = node_value(n.seed_h, member, c, l.gx1, l.gy0);
  const double u01 = node_value(n.seed_h, member, c, l.gx0, l.gy1), u11 = node_value(n.seed_h, member, c, l.gx1, l.gy1);
  const double sx = 1.0 - l.tx, sy = 1.0 - l.ty;
  const double p00 = rounded(sx * u00), p10 = rounded(l.tx * u10), p01 = rounded(sx * u01), p11 = rounded(l.tx * u11);
  const double bottom = p00 + p10, top = p01 + p11;
  const double qb = rounded(sy * bottom), qt = rounded(l.ty * top);
  return qb + qt;
}

// one channel: the new value, or v itself (bit for bit) where the header says "untouched"
WX_HD inline float perturb_value(const Noise &n, float v, double r, int c)
{
#pragma clang fp contract(off)
  const float a = n.amp[c];
  if (a == 0.0f || !f32_finite(v)) return v;
  const double ar = rounded((double)a * r);
  double d;
  if (n.mode == 0) {
    d = (double)v + ar;
  } else {
    const double f = 1.0 + ar;
    d = (double)v * f;
  }
  float o = (float)d;
  if (n.lo[c] == n.lo[c] && o < n.lo[c]) o = n.lo[c];
  if (n.hi[c] == n.hi[c] && o > n.hi[c]) o = n.hi[c];
  return f32_finite(o) ? o : v;
}

// one cell of one member; returns whether any channel's bits changed (a lane that changed nothing does not store)
WX_HD inline bool perturb_cell(const Noise &n, int member, int x, int y, int wall_dist, float v[4])
{
  if (wall_dist == 0) return false;
  const Lattice l = lattice_of(n, x, y);
  bool changed = false;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    if (n.amp[c] == 0.0f) continue; // (uniform over the launch: no hash chain for a channel that is not perturbed)
    const float o = perturb_value(n, v[c], noise_at(n, l, member, c), c);
    changed = changed || f32_bits(o) != f32_bits(v[c]);
    v[c] = o;
  }
  return changed;
}

// the argument checks wx_ensemble_perturb and wx_ens_perturb_cells share (nothing here touches a device)
inline int check_desc(const wx_ens_perturb *p, int X, int Y, const char **why)
{
  *why = "";
  if (p->field != WX_FIELD_BASE_CUR && p->field != WX_FIELD_WATER_CUR) {
    *why = "field: WX_FIELD_BASE_CUR or WX_FIELD_WATER_CUR (the fields that are stored whole and interleaved)";
    return WX_E_INVALID;
  }
  if (p->mode != 0 && p->mode != 1) {
    *why = "mode: 0 (v + a r) or 1 (v (1 + a r))";
    return WX_E_INVALID;
  }
  if (p->scale < 1) {
    *why = "scale >= 1";
    return WX_E_INVALID;
  }
  if (p->w <= 0 || p->h <= 0 || p->x < 0 || p->y < 0 || (long long)p->x + p->w > X || (long long)p->y + p->h > Y) {
    *why = "the rectangle lies outside the grid (no wrap)";
    return WX_E_RANGE;
  }
  return WX_OK;
}

// host only, pure: the kernel's per-cell function over the rectangle's cells of n_members members held by the caller
inline int perturb_cells(const wx_ens_perturb *p, int X, int Y, int n_members, float *const *field, const int8_t *const *wall, const uint8_t *mask)
{
  if (!p || n_members < 1 || !field || !wall || X < 1 || Y < 1) return WX_E_INVALID;
  const char *why;
  if (int rc = check_desc(p, X, Y, &why)) return rc;
  int n_sel = 0;
  for (int i = 0; i < n_members; i++) {
    if (mask && !mask[i]) continue;
    if (!field[i] || !wall[i]) return WX_E_INVALID;
    n_sel++;
  }
  if (n_sel == 0) return WX_E_INVALID;
  const Noise n = noise_of(*p, X);
  for (int i = 0; i < n_members; i++) {
    if (mask && !mask[i]) continue;
    for (int y = 0; y < p->h; y++)
      for (int x = 0; x < p->w; x++) {
        const size_t o = (size_t)y * p->w + x;
        float v[4];
        memcpy(v, field[i] + 4 * o, 16);
        if (perturb_cell(n, i, p->x + x, p->y + y, wall[i][4 * o + 1], v)) memcpy(field[i] + 4 * o, v, 16);
      }
  }
  return WX_OK;
}

} // namespace wxp
