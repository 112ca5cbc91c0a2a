// Stand-alone driver of the inflation's host function (csrc/wx_ens_inflate_cell.h) for a host-compiler build under AddressSanitizer /
// UBSan (tests/test_ensemble_inflate_cpu.py): wxi::inflate_cells over arrays that are allocated to the byte -- a read or write one cell
// outside them is a report -- with the planted cells of the CPU test (a wall in one member, NaN / +-Inf / FLT_MAX in one member's value
// and in one snapshot value, -0.0 with lambda == 1 and with a neutral coefficient, equal members, lambda driven to each bound, a result
// that overflows in one member only, both clamp edges) and randomised ones: any bit pattern as a value, masks with absent members, all
// three modes, the lambda map wanted and not. Checks what needs no second implementation: unselected members, cells that are a wall in
// a selected member, channels with a neutral coefficient and channels that hold a non-finite value keep their bits, finite values stay
// finite, clamps hold, the lambda map is NaN exactly where nothing could change, refused arguments write nothing.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../2d-weather-sandbox_amd/csrc/wx_ens_inflate_cell.h"

static uint32_t rng_state = 0x2545F491u;
static uint32_t rnd()
{
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}
static float unit() { return (float)(rnd() >> 8) / 16777216.0f; }
static uint32_t bits(float v) { return wxi::f32_bits(v); }

#define REQUIRE(c)                                                   \
  do {                                                               \
    if (!(c)) {                                                      \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);        \
      return 1;                                                      \
    }                                                                \
  } while (0)

static wx_ens_inflate desc(int mode, float coef)
{
  wx_ens_inflate p;
  memset(&p, 0, sizeof(p));
  p.field = WX_FIELD_BASE_CUR, p.w = p.h = 1, p.mode = mode;
  p.lambda_lo = p.lambda_hi = NAN;
  for (int c = 0; c < 4; c++) p.coef[c] = coef, p.lo[c] = p.hi[c] = NAN;
  return p;
}

// one cell, n members, channel 3 holds x / prior, the other channels 1.0 + k
struct OneCell {
  std::vector<std::vector<float>> f, p;
  std::vector<std::vector<int8_t>> w;
  std::vector<float *> fp;
  std::vector<const float *> pp;
  std::vector<const int8_t *> wp;
  OneCell(const std::vector<float> &x, const std::vector<float> &prior)
  {
    const size_t n = x.size();
    for (size_t k = 0; k < n; k++) {
      f.push_back({1.0f + (float)k, 1.0f + (float)k, 1.0f + (float)k, x[k]});
      p.push_back({2.0f * (float)k, 2.0f * (float)k, 2.0f * (float)k, prior[k]});
      w.push_back({0, 3, 0, 0});
    }
    for (size_t k = 0; k < n; k++) fp.push_back(f[k].data()), pp.push_back(p[k].data()), wp.push_back(w[k].data());
  }
  int run(const wx_ens_inflate &d) { return wxi::inflate_cells(&d, (int)f.size(), 1, fp.data(), wp.data(), pp.data(), nullptr); }
};

static int planted()
{
  const float FMAX = 3.4028234663852886e38f;
  float lam[4];
  { // a wall in one member: nothing changes, the map is NaN
    OneCell c({1.0f, 2.0f, 4.0f}, {0.0f, 2.0f, 8.0f});
    c.w[1][1] = 0;
    for (int mode = 0; mode < 3; mode++) {
      wx_ens_inflate d = desc(mode, mode ? 0.5f : 1.5f);
      d.lambda_out = mode == WX_INFLATE_RTPP ? nullptr : lam;
      REQUIRE(c.run(d) == WX_OK);
      REQUIRE(c.f[0][3] == 1.0f && c.f[1][3] == 2.0f && c.f[2][3] == 4.0f && c.f[2][0] == 3.0f);
      REQUIRE(mode == WX_INFLATE_RTPP || (lam[0] != lam[0] && lam[3] != lam[3]));
    }
  }
  const float specials[3] = {NAN, INFINITY, -INFINITY};
  for (float s : specials) { // in one member's value: that channel is left alone in all members; in one snapshot value: in the relaxation modes
    for (int mode = 0; mode < 3; mode++) {
      OneCell c({1.0f, s, 4.0f}, {0.0f, 2.0f, 8.0f});
      wx_ens_inflate d = desc(mode, mode ? 0.5f : 1.5f);
      REQUIRE(c.run(d) == WX_OK);
      REQUIRE(c.f[0][3] == 1.0f && bits(c.f[1][3]) == bits(s) && c.f[2][3] == 4.0f && c.f[0][0] != 1.0f);
      OneCell q({1.0f, 2.0f, 4.0f}, {0.0f, s, 8.0f});
      REQUIRE(q.run(d) == WX_OK);
      REQUIRE((q.f[0][3] == 1.0f && q.f[2][3] == 4.0f) == (mode != WX_INFLATE_CONST));
    }
  }
  { // FLT_MAX in one member is finite and enters; its own result overflows and keeps its bits, the others move
    OneCell c({300.0f, FMAX, 301.0f}, {0.0f, 0.0f, 0.0f});
    wx_ens_inflate d = desc(WX_INFLATE_CONST, 1.5f);
    d.lambda_out = lam;
    REQUIRE(c.run(d) == WX_OK);
    REQUIRE(c.f[1][3] == FMAX && c.f[0][3] != 300.0f && c.f[2][3] != 301.0f && std::isfinite(c.f[0][3]) && lam[3] == 1.5f);
  }
  { // -0.0: a neutral coefficient and lambda == 1 keep the sign bit; equal members (sa == 0) are untouched
    OneCell c({-0.0f, -0.0f, -0.0f}, {-0.0f, -0.0f, -0.0f});
    wx_ens_inflate d = desc(WX_INFLATE_CONST, 1.0f);
    REQUIRE(c.run(d) == WX_OK && bits(c.f[0][3]) == 0x80000000u && c.f[1][0] == 2.0f);
    d = desc(WX_INFLATE_RTPS, 0.5f);
    d.lambda_out = lam;
    REQUIRE(c.run(d) == WX_OK && bits(c.f[0][3]) == 0x80000000u && bits(c.f[2][3]) == 0x80000000u && lam[3] != lam[3] && lam[0] == lam[0]);
    OneCell e({-0.0f, 1.0f, 2.0f}, {-0.0f, 1.0f, 2.0f}); // the prior IS the state: lambda == 1
    REQUIRE(e.run(d) == WX_OK && bits(e.f[0][3]) == 0x80000000u && e.f[2][3] == 2.0f && lam[3] != lam[3]);
  }
  { // lambda driven to each bound, exactly
    OneCell c({299.0f, 300.0f, 301.0f}, {296.0f, 300.0f, 304.0f});
    wx_ens_inflate d = desc(WX_INFLATE_RTPS, 1.0f);
    d.lambda_lo = 0.5f, d.lambda_hi = 2.0f, d.lambda_out = lam;
    REQUIRE(c.run(d) == WX_OK && lam[3] == 2.0f && c.f[0][3] == 298.0f && c.f[1][3] == 300.0f && c.f[2][3] == 302.0f);
    OneCell q({296.0f, 300.0f, 304.0f}, {299.5f, 300.0f, 300.5f});
    REQUIRE(q.run(d) == WX_OK && lam[3] == 0.5f && q.f[0][3] == 298.0f && q.f[2][3] == 302.0f);
    d.lambda_lo = 3.0f; // crossed: the upper bound is applied last
    OneCell r({299.0f, 300.0f, 301.0f}, {296.0f, 300.0f, 304.0f});
    REQUIRE(r.run(d) == WX_OK && lam[3] == 2.0f);
  }
  { // both clamp edges
    OneCell c({299.0f, 300.0f, 301.0f}, {0.0f, 0.0f, 0.0f});
    wx_ens_inflate d = desc(WX_INFLATE_CONST, 3.0f);
    d.lo[3] = 299.5f, d.hi[3] = 300.5f;
    REQUIRE(c.run(d) == WX_OK && c.f[0][3] == 299.5f && c.f[1][3] == 300.0f && c.f[2][3] == 300.5f && c.f[2][0] == 5.0f);
  }
  { // exact: RTPP alpha = 1 gives m + b_k; refusals write nothing
    OneCell c({299.0f, 300.0f, 301.0f}, {10.0f, 14.0f, 12.0f});
    wx_ens_inflate d = desc(WX_INFLATE_RTPP, 1.0f);
    REQUIRE(c.run(d) == WX_OK && c.f[0][3] == 298.0f && c.f[1][3] == 302.0f && c.f[2][3] == 300.0f);
    d.lambda_out = lam;
    REQUIRE(c.run(d) == WX_E_INVALID);
    d = desc(WX_INFLATE_RTPP, 1.5f);
    REQUIRE(c.run(d) == WX_E_INVALID);
    d = desc(WX_INFLATE_CONST, -1.0f);
    REQUIRE(c.run(d) == WX_E_INVALID);
    d = desc(3, 1.0f);
    REQUIRE(c.run(d) == WX_E_INVALID);
    d = desc(WX_INFLATE_RTPS, NAN);
    REQUIRE(c.run(d) == WX_E_INVALID);
    d = desc(WX_INFLATE_RTPS, 0.5f);
    REQUIRE(wxi::inflate_cells(&d, 3, 1, c.fp.data(), c.wp.data(), nullptr, nullptr) == WX_E_INVALID);
    const uint8_t one[3] = {0, 1, 0};
    REQUIRE(wxi::inflate_cells(&d, 3, 1, c.fp.data(), c.wp.data(), c.pp.data(), one) == WX_E_INVALID);
    REQUIRE(c.f[0][3] == 298.0f && c.f[1][3] == 302.0f && c.f[2][3] == 300.0f);
  }
  return 0;
}

int main()
{
  if (planted()) return 1;
  const size_t sizes[] = {1, 2, 63, 64, 65, 910};
  long member_cells = 0, moved = 0, lam_cells = 0;
  for (size_t n_cells : sizes) {
    for (int round = 0; round < 18; round++) {
      const int mode = round % 3;
      const bool wild = round >= 12; // any bit pattern as a value
      wx_ens_inflate d = desc(mode, 0.0f);
      for (int c = 0; c < 4; c++) {
        const bool neutral = rnd() % 4 == 0;
        d.coef[c] = mode == WX_INFLATE_CONST ? (neutral ? 1.0f : 0.5f + 2.0f * unit()) : (neutral ? 0.0f : (mode == WX_INFLATE_RTPP ? unit() : 3.0f * unit()));
        d.lo[c] = (rnd() & 1) ? NAN : -0.25f, d.hi[c] = (rnd() & 1) ? NAN : ((rnd() & 3) ? 1.25f : INFINITY);
      }
      if (round % 5 == 1) d.lambda_lo = 0.9f;
      if (round % 5 == 2) d.lambda_hi = 1.1f;
      const int B = 2 + (int)(rnd() % 16);
      std::vector<float *> field(B, nullptr);
      std::vector<const float *> prior(B, nullptr);
      std::vector<const int8_t *> wall(B, nullptr);
      std::vector<std::vector<float>> before(B);
      std::vector<uint8_t> mask(B, 0);
      const unsigned first = rnd() % B;
      int n_sel = 0;
      for (int i = 0; i < B; i++) {
        mask[i] = (unsigned)i == first || (unsigned)i == (first + 1) % B || (rnd() % 3) != 0;
        n_sel += mask[i];
        if (!mask[i] && (rnd() & 1)) continue; // an unselected member may be absent
        float *f = (float *)malloc(n_cells * 16), *p = (float *)malloc(n_cells * 16);
        int8_t *w = (int8_t *)malloc(n_cells * 4);
        for (size_t j = 0; j < n_cells * 4; j++) {
          uint32_t u = rnd(), v = rnd();
          if (wild && (rnd() % 7) == 0) memcpy(&f[j], &u, 4), memcpy(&p[j], &v, 4);
          else f[j] = unit() - 0.25f, p[j] = 1.5f * unit() - 0.5f;
          w[j] = (int8_t)((rnd() % 9) ? 1 + rnd() % 100 : 0);
        }
        field[i] = f, prior[i] = p, wall[i] = w;
        before[i].assign(f, f + n_cells * 4);
      }
      const bool use_mask = (round & 1) || n_sel < B;
      const bool want_lam = mode != WX_INFLATE_RTPP && (round & 2);
      std::vector<float> lam(want_lam ? n_cells * 4 : 0);
      if (want_lam) d.lambda_out = lam.data();
      if (!use_mask)
        for (int i = 0; i < B; i++) REQUIRE(field[i]); // (every member is selected then)
      const int rc = wxi::inflate_cells(&d, B, n_cells, field.data(), wall.data(), mode == WX_INFLATE_CONST && (round & 4) ? nullptr : prior.data(),
                                        use_mask ? mask.data() : nullptr);
      REQUIRE(rc == WX_OK);
      for (size_t j = 0; j < n_cells; j++) {
        bool air = true;
        for (int i = 0; i < B; i++)
          if (!use_mask || mask[i]) air = air && wall[i][4 * j + 1] != 0;
        for (int c = 0; c < 4; c++) {
          bool all_finite = true, any_moved = false;
          for (int i = 0; i < B; i++) {
            if (use_mask && !mask[i]) continue;
            all_finite = all_finite && wxi::f32_finite(before[i][4 * j + c]) && (mode == WX_INFLATE_CONST || wxi::f32_finite(prior[i][4 * j + c]));
          }
          const bool may_change = air && all_finite && !wxi::neutral(mode, d.coef[c]);
          for (int i = 0; i < B; i++) {
            if (!field[i]) continue;
            const float o = field[i][4 * j + c], b = before[i][4 * j + c];
            const bool selected = !use_mask || mask[i];
            if (!selected || !may_change) REQUIRE(bits(o) == bits(b));
            if (bits(o) != bits(b)) {
              any_moved = true;
              REQUIRE(wxi::f32_finite(o));
              REQUIRE(!(d.lo[c] == d.lo[c]) || o >= d.lo[c]);
              REQUIRE(!(d.hi[c] == d.hi[c]) || o <= d.hi[c]);
            }
            member_cells++;
          }
          moved += any_moved;
          if (want_lam) {
            const float l = lam[4 * j + c];
            REQUIRE(may_change || l != l);
            REQUIRE(!any_moved || l == l);
            if (l == l) {
              lam_cells++;
              if (mode == WX_INFLATE_CONST) REQUIRE(l == d.coef[c]);
              if (mode == WX_INFLATE_RTPS && d.lambda_lo == d.lambda_lo) REQUIRE(l >= d.lambda_lo);
              if (mode == WX_INFLATE_RTPS && d.lambda_hi == d.lambda_hi) REQUIRE(l <= d.lambda_hi);
            }
          }
        }
      }
      for (int i = 0; i < B; i++) free(field[i]), free((void *)prior[i]), free((void *)wall[i]);
    }
  }
  REQUIRE(moved > 1000 && lam_cells > 100);
  printf("ens_inflate_main ok: %ld member-cell channels, %ld cell channels moved, %ld lambdas\n", member_cells, moved, lam_cells);
  return 0;
}
