// Stand-alone driver of the perturbation's per-cell function (csrc/wx_ens_perturb_cell.h) for a host-compiler build under
// AddressSanitizer / UBSan (tests/test_ensemble_perturb_cpu.py): wxp::perturb_cells over randomised buffers that are allocated to the
// byte -- a read or write one cell outside the rectangle is a report -- with every mode, lattice pitches from 1 to beyond the grid,
// wrap_x, clamps, masks with absent members, extreme seeds and member counts. Checks what needs no second implementation: wall cells,
// channels with amplitude 0 and non-finite values keep their bits, finite values stay finite, refused descriptors write nothing.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../2d-weather-sandbox_amd/csrc/wx_ens_perturb_cell.h"

static uint32_t rng_state = 0x2545F491u;
static uint32_t rnd()
{
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

#define REQUIRE(c)                                                   \
  do {                                                               \
    if (!(c)) {                                                      \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);        \
      return 1;                                                      \
    }                                                                \
  } while (0)

int main()
{
  const int grids[][2] = {{1, 1}, {37, 11}, {130, 40}, {64, 3}};
  const int scales[] = {1, 3, 8, 64, 100000, 2147483647};
  const uint32_t seeds[] = {0u, 1u, 0xFFFFFFFFu, 0x80000000u};
  long cells = 0;
  for (const auto &g : grids) {
    const int X = g[0], Y = g[1];
    for (int scale : scales)
      for (int mode = 0; mode < 2; mode++)
        for (int wrap = 0; wrap < 2; wrap++) {
          wx_ens_perturb p;
          memset(&p, 0, sizeof(p));
          p.field = (rnd() & 1) ? WX_FIELD_BASE_CUR : WX_FIELD_WATER_CUR;
          p.w = 1 + (int)(rnd() % (unsigned)X), p.h = 1 + (int)(rnd() % (unsigned)Y);
          p.x = (int)(rnd() % (unsigned)(X - p.w + 1)), p.y = (int)(rnd() % (unsigned)(Y - p.h + 1));
          p.mode = mode, p.scale = scale, p.wrap_x = wrap, p.seed = seeds[rnd() % 4];
          const float amps[4] = {0.05f, 0.0f, 3.0e38f, NAN};
          for (int c = 0; c < 4; c++) {
            p.amplitude[c] = amps[(c + (int)(rnd() % 4)) % 4];
            p.lo[c] = (rnd() & 1) ? NAN : -1.0f;
            p.hi[c] = (rnd() & 1) ? NAN : ((rnd() & 1) ? 2.0f : INFINITY);
          }
          const int B = 1 + (int)(rnd() % 5);
          const size_t n = (size_t)p.w * p.h;
          std::vector<float *> field(B, nullptr);
          std::vector<int8_t *> wall(B, nullptr);
          std::vector<std::vector<float>> before(B);
          std::vector<uint8_t> mask(B, 0);
          mask[rnd() % B] = 1;
          for (int i = 0; i < B; i++) {
            if (rnd() & 1) mask[i] = 1;
            if (!mask[i] && (rnd() & 1)) continue; // an unselected member may be absent
            field[i] = (float *)malloc(n * 16);
            wall[i] = (int8_t *)malloc(n * 4);
            for (size_t k = 0; k < 4 * n; k++) {
              const uint32_t bits = (rnd() & 3) ? (0x3C000000u + (rnd() & 0x07FFFFFFu)) | (rnd() & 0x80000000u) : rnd(); // ordinary values, and any bit pattern
              memcpy(field[i] + k, &bits, 4);
              wall[i][k] = (int8_t)((rnd() % 5) ? (rnd() & 0x7F) : 0);
            }
            before[i].assign(field[i], field[i] + 4 * n);
          }
          const bool use_mask = (rnd() & 3) != 0;
          bool all_present = true;
          for (int i = 0; i < B; i++) all_present = all_present && field[i];
          const uint8_t *mk = (use_mask || !all_present) ? mask.data() : nullptr;
          REQUIRE(wxp::perturb_cells(&p, X, Y, B, field.data(), wall.data(), mk) == WX_OK);
          for (int i = 0; i < B; i++) {
            if (!field[i]) continue;
            for (size_t k = 0; k < n; k++)
              for (int c = 0; c < 4; c++) {
                const float was = before[i][4 * k + c], is = field[i][4 * k + c];
                const bool same = wxp::f32_bits(was) == wxp::f32_bits(is);
                if ((mk && !mk[i]) || wall[i][4 * k + 1] == 0 || p.amplitude[c] == 0.0f || !wxp::f32_finite(was) || p.amplitude[c] != p.amplitude[c]) REQUIRE(same);
                if (wxp::f32_finite(was)) REQUIRE(wxp::f32_finite(is));
                if (!same && p.lo[c] == p.lo[c]) REQUIRE(is >= p.lo[c]);
                if (!same && p.hi[c] == p.hi[c]) REQUIRE(is <= p.hi[c]);
              }
            cells += (long)n;
          }
          // a refused descriptor writes nothing
          wx_ens_perturb bad = p;
          bad.x = X - p.w + 1;
          for (int i = 0; i < B; i++)
            if (field[i]) before[i].assign(field[i], field[i] + 4 * n);
          REQUIRE(wxp::perturb_cells(&bad, X, Y, B, field.data(), wall.data(), mk) == WX_E_RANGE);
          bad = p, bad.scale = 0;
          REQUIRE(wxp::perturb_cells(&bad, X, Y, B, field.data(), wall.data(), mk) == WX_E_INVALID);
          for (int i = 0; i < B; i++)
            if (field[i]) REQUIRE(memcmp(before[i].data(), field[i], n * 16) == 0);
          for (int i = 0; i < B; i++) {
            free(field[i]);
            free(wall[i]);
          }
        }
  }
  // node values are 24-bit fractions in [-1, 1); the noise stays inside that interval
  for (int k = 0; k < 100000; k++) {
    const double u = wxp::node_value(rnd(), (int)(rnd() % 70000), (int)(rnd() % 4), rnd(), rnd());
    REQUIRE(u >= -1.0 && u < 1.0 && u * 8388608.0 == std::floor(u * 8388608.0));
  }
  printf("ens_perturb_main ok: %ld member-cells\n", cells);
  return 0;
}
