// Stand-alone driver of the assimilation's host function (csrc/wx_ens_assim_cell.h) for a host-compiler build under AddressSanitizer /
// UBSan (tests/test_ensemble_assimilate_cpu.py): wxa::assim_cells over grids that are allocated to the byte -- a read or write one cell
// outside the grid is a report -- with the planted cases of the CPU test (an observed cell that is a wall or holds a NaN / Inf in one
// member, a NaN in a state cell, equal members, -0.0, gain 0, clamps, values at the edge of the float range, loc 0 on either axis,
// wrap_x with observations at x = 0 and X - 1, observations outside the rectangle, duplicates, overlapping footprints) and randomised
// ones: any bit pattern as a value, masks with absent members, up to WX_ENS_OBS_MAX observations. Checks what needs no second
// implementation: unselected members, wall cells, cells outside the rectangle, channels with gain 0 and non-finite values keep their
// bits, finite values stay finite, clamps hold, a skipped observation reports NaN, refused arguments write nothing.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../2d-weather-sandbox_amd/csrc/wx_ens_assim_cell.h"

static uint32_t rng_state = 0x2545F491u;
static uint32_t rnd()
{
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}
static float unit() { return (float)(rnd() >> 8) / 16777216.0f; }

#define REQUIRE(c)                                                   \
  do {                                                               \
    if (!(c)) {                                                      \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);        \
      return 1;                                                      \
    }                                                                \
  } while (0)

int main()
{
  const int grids[][2] = {{2, 1}, {17, 7}, {37, 11}, {130, 40}, {64, 3}};
  long member_cells = 0, applied = 0, skipped = 0;
  for (const auto &g : grids) {
    const int X = g[0], Y = g[1];
    for (int round = 0; round < 12; round++) {
      const bool wild = round >= 8; // any bit pattern as a value
      wx_ens_assim a;
      memset(&a, 0, sizeof(a));
      a.w = 1 + (int)(rnd() % (unsigned)X), a.h = 1 + (int)(rnd() % (unsigned)Y);
      a.x = (int)(rnd() % (unsigned)(X - a.w + 1)), a.y = (int)(rnd() % (unsigned)(Y - a.h + 1));
      a.wrap_x = round & 1;
      a.loc_x = (round % 3 == 0) ? 0.0f : 1.0f + 6.0f * unit(), a.loc_y = (round % 4 == 1) ? 0.0f : 0.5f + 3.0f * unit();
      for (int c = 0; c < 4; c++) {
        a.gain_base[c] = (rnd() % 3) ? 0.25f + unit() : 0.0f, a.gain_water[c] = (rnd() % 3) ? 1.0f : 0.0f;
        a.lo_base[c] = (rnd() & 1) ? NAN : 0.05f, a.hi_base[c] = (rnd() & 1) ? NAN : ((rnd() & 1) ? 300.5f : INFINITY);
        a.lo_water[c] = (rnd() & 1) ? NAN : 0.0f, a.hi_water[c] = NAN;
      }
      if (round == 5) a.gain_base[3] = 3.0e38f;
      const int B = 2 + (int)(rnd() % 7);
      const size_t n = (size_t)X * Y;
      std::vector<float *> base(B, nullptr), water(B, nullptr);
      std::vector<int8_t *> wall(B, nullptr);
      std::vector<std::vector<float>> before_b(B), before_w(B);
      std::vector<uint8_t> mask(B, 0);
      const unsigned first = rnd() % B;
      mask[first] = mask[(first + 1) % B] = 1;
      const bool equal_members = round == 6;
      for (int i = 0; i < B; i++) {
        if (rnd() & 1) mask[i] = 1;
        if (!mask[i] && (rnd() & 1)) continue; // an unselected member may be absent
        base[i] = (float *)malloc(n * 16), water[i] = (float *)malloc(n * 16);
        wall[i] = (int8_t *)malloc(n * 4);
        for (size_t k = 0; k < 4 * n; k++) {
          float b = (k & 3) == 3 ? 300.0f + 3.0f * unit() : unit() - 0.5f, w = 0.01f * unit();
          if (equal_members) b = (k & 3) == 0 ? -0.0f : 1.0f + (float)(k % 7), w = 0.0f;
          if (wild && (rnd() & 7) == 0) {
            const uint32_t bits = rnd();
            memcpy(&b, &bits, 4);
          }
          if (round == 7 && (k & 3) == 3) b = ((rnd() & 1) ? 3.0e38f : -3.0e38f) * (0.5f + 0.5f * unit());
          memcpy(base[i] + k, &b, 4), memcpy(water[i] + k, &w, 4);
          wall[i][k] = (int8_t)((rnd() % 23) ? 1 + (rnd() & 0x3F) : 0);
        }
        before_b[i].assign(base[i], base[i] + 4 * n), before_w[i].assign(water[i], water[i] + 4 * n);
      }
      const int n_obs = round == 9 ? WX_ENS_OBS_MAX : 1 + (int)(rnd() % 9);
      std::vector<wx_ens_obs> obs((size_t)n_obs);
      for (int j = 0; j < n_obs; j++) {
        wx_ens_obs &o = obs[(size_t)j];
        o.field = (rnd() & 3) ? WX_FIELD_BASE_CUR : WX_FIELD_WATER_CUR;
        o.x = (j % 5 == 1) ? 0 : (j % 5 == 2) ? X - 1 : (int)(rnd() % (unsigned)X);
        o.y = (int)(rnd() % (unsigned)Y);
        o.channel = o.field == WX_FIELD_BASE_CUR ? ((rnd() & 1) ? 3 : (int)(rnd() & 3)) : (int)(rnd() & 3);
        o.value = o.channel == 3 ? 300.0f + 3.0f * unit() : unit();
        if (round == 7) o.value = (rnd() & 1) ? 3.4e38f : -3.4e38f;
        o.error_var = (rnd() & 1) ? 0.25f : ((rnd() & 1) ? 1.0e-30f : 1.0e30f);
        if (j > 0 && j % 4 == 3) o.field = obs[(size_t)j - 1].field, o.x = obs[(size_t)j - 1].x, o.y = obs[(size_t)j - 1].y, o.channel = obs[(size_t)j - 1].channel; // a duplicate
      }
      std::vector<wx_ens_obs_result> res((size_t)n_obs);
      REQUIRE(wxa::assim_cells(&a, n_obs, obs.data(), res.data(), X, Y, B, base.data(), water.data(), wall.data(), mask.data()) == WX_OK);
      for (int j = 0; j < n_obs; j++) {
        const wx_ens_obs_result &r = res[(size_t)j];
        REQUIRE(r.applied == 0 || r.applied == 1);
        if (r.applied) {
          REQUIRE(wxa::f64_finite(r.prior_mean) && r.prior_var >= 0.0 && r.alpha >= 0.5 && r.alpha <= 1.0);
          applied++;
        } else {
          REQUIRE(r.prior_mean != r.prior_mean && r.prior_var != r.prior_var && r.innovation != r.innovation && r.alpha != r.alpha);
          skipped++;
        }
      }
      for (int i = 0; i < B; i++) {
        if (!base[i]) continue;
        for (size_t k = 0; k < n; k++) {
          const int x = (int)(k % (size_t)X), y = (int)(k / (size_t)X);
          bool air = true;
          for (int m = 0; m < B; m++)
            if (mask[m] && wall[m][4 * k + 1] == 0) air = false;
          for (int f = 0; f < 2; f++)
            for (int c = 0; c < 4; c++) {
              const float was = (f ? before_w : before_b)[i][4 * k + c], is = (f ? water : base)[i][4 * k + c];
              const float gain = (f ? a.gain_water : a.gain_base)[c], lo = (f ? a.lo_water : a.lo_base)[c], hi = (f ? a.hi_water : a.hi_base)[c];
              const bool same = wxa::f32_bits(was) == wxa::f32_bits(is);
              if (!mask[i] || !air || !wxa::in_rect(a, x, y) || gain == 0.0f || !wxa::f32_finite(was)) REQUIRE(same);
              if (wxa::f32_finite(was)) REQUIRE(wxa::f32_finite(is));
              if (equal_members) REQUIRE(same);
              if (!same && lo == lo) REQUIRE(is >= lo);
              if (!same && hi == hi) REQUIRE(is <= hi);
            }
        }
        member_cells += (long)n;
      }
      // refused arguments write nothing
      for (int i = 0; i < B; i++)
        if (base[i]) before_b[i].assign(base[i], base[i] + 4 * n), before_w[i].assign(water[i], water[i] + 4 * n);
      wx_ens_assim bad = a;
      bad.x = X - a.w + 1;
      REQUIRE(wxa::assim_cells(&bad, n_obs, obs.data(), res.data(), X, Y, B, base.data(), water.data(), wall.data(), mask.data()) == WX_E_RANGE);
      bad = a, bad.loc_x = -1.0f;
      REQUIRE(wxa::assim_cells(&bad, n_obs, obs.data(), res.data(), X, Y, B, base.data(), water.data(), wall.data(), mask.data()) == WX_E_INVALID);
      std::vector<wx_ens_obs> bad_obs = obs;
      bad_obs.back().x = X;
      REQUIRE(wxa::assim_cells(&a, n_obs, bad_obs.data(), res.data(), X, Y, B, base.data(), water.data(), wall.data(), mask.data()) == WX_E_RANGE);
      bad_obs = obs, bad_obs.back().error_var = 0.0f;
      REQUIRE(wxa::assim_cells(&a, n_obs, bad_obs.data(), res.data(), X, Y, B, base.data(), water.data(), wall.data(), mask.data()) == WX_E_INVALID);
      REQUIRE(wxa::assim_cells(&a, WX_ENS_OBS_MAX + 1, obs.data(), res.data(), X, Y, B, base.data(), water.data(), wall.data(), mask.data()) == WX_E_INVALID);
      std::vector<uint8_t> one(B, 0);
      one[first] = 1;
      REQUIRE(wxa::assim_cells(&a, n_obs, obs.data(), res.data(), X, Y, B, base.data(), water.data(), wall.data(), one.data()) == WX_E_INVALID);
      for (int i = 0; i < B; i++)
        if (base[i]) REQUIRE(memcmp(before_b[i].data(), base[i], n * 16) == 0 && memcmp(before_w[i].data(), water[i], n * 16) == 0);
      for (int i = 0; i < B; i++) {
        free(base[i]), free(water[i]);
        free(wall[i]);
      }
    }
  }
  // the Gaspari-Cohn polynomial: 1 at 0, 5/24 at 1, 0 from 2 on, inside [0, 1] and not increasing
  double last = 1.0;
  REQUIRE(wxa::gc(0.0) == 1.0 && wxa::gc(2.0) == 0.0 && std::fabs(wxa::gc(1.0) - 5.0 / 24.0) < 1e-15);
  for (int k = 0; k <= 4000; k++) {
    const double v = wxa::gc(k / 2000.0);
    REQUIRE(v >= 0.0 && v <= 1.0 && v <= last + 1e-15);
    last = v;
  }
  REQUIRE(applied > 0 && skipped > 0);
  printf("ens_assim_main ok: %ld member-cells, %ld observations applied, %ld skipped\n", member_cells, applied, skipped);
  return 0;
}
