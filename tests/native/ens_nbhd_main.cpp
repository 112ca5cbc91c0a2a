// Stand-alone driver of the neighbourhood call's definition (csrc/wx_ens_nbhd_cell.h) for a host-compiler build under
// AddressSanitizer / UBSan (tests/test_ensemble_neighbourhood_cpu.py): wxn::nbhd_cells over randomised grids that are allocated to the
// byte -- a read or write one cell outside is a report -- with masks and absent members, with and without a truth, wrap on and off,
// rectangles at the corners, radii up to the limit. Checks what needs no second implementation: every cell is counted exactly once
// per scale, the maps are NaN exactly where a window holds no counted cell and lie in [0, 1] elsewhere, radius 0 is the point counts,
// members identical to the truth score d2 == 0, the rectangle in four quarters adds up, a refused call writes nothing.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../2d-weather-sandbox_amd/csrc/wx_ens_nbhd_cell.h"

static uint32_t rng_state = 0x9E3779B9u;
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

template <typename T>
static T *exact(size_t n) // n elements and not a byte more (n >= 1 here)
{
  return (T *)malloc(n * sizeof(T));
}

static void fill(float *f, int8_t *w, size_t n)
{
  for (size_t k = 0; k < 4 * n; k++) {
    const uint32_t bits = (rnd() & 7) ? (0x3C000000u + (rnd() & 0x07FFFFFFu)) | (rnd() & 0x80000000u) : ((rnd() & 1) ? rnd() : (rnd() & 0x80000000u)); // ordinary values, any bit pattern, zeros
    memcpy(f + k, &bits, 4);
    w[k] = (int8_t)((rnd() % 6) ? (rnd() & 0x7F) : 0);
  }
}

int main()
{
  const int shapes[][2] = {{1, 1}, {5, 3}, {17, 9}, {70, 12}, {3, 40}};
  const int member_counts[] = {1, 2, 9, 70};
  long cells = 0;
  for (auto &sh : shapes)
    for (int B : member_counts)
      for (int round = 0; round < 4; round++) {
        const int X = sh[0], Y = sh[1];
        const size_t n = (size_t)X * Y;
        const bool have_truth = round != 3, wrap = round & 1;
        std::vector<float *> field(B, nullptr);
        std::vector<int8_t *> wall(B, nullptr);
        std::vector<uint8_t> mask(B, 0);
        mask[rnd() % B] = 1;
        for (int i = 0; i < B; i++) {
          if (rnd() % 3) mask[i] = 1;
          if (!mask[i] && (rnd() & 1)) continue; // an unselected member may be absent
          field[i] = exact<float>(4 * n), wall[i] = exact<int8_t>(4 * n);
          fill(field[i], wall[i], n);
        }
        float *tf = have_truth ? exact<float>(4 * n) : nullptr;
        int8_t *tw = have_truth ? exact<int8_t>(4 * n) : nullptr;
        if (have_truth) fill(tf, tw, n);
        int n_sel = 0, first = -1;
        for (int i = 0; i < B; i++)
          if (mask[i]) n_sel++, first = first < 0 ? i : first;
        if (round == 2) { // every selected member is the truth
          for (int i = 0; i < B; i++)
            if (mask[i]) memcpy(field[i], tf, 16 * n), memcpy(wall[i], tw, 4 * n);
        }
        wx_ens_nbhd a;
        memset(&a, 0, sizeof(a));
        a.field = (rnd() & 1) ? WX_FIELD_BASE_CUR : WX_FIELD_WATER_CUR, a.channel = (int)(rnd() % 4);
        a.threshold = 0.01f, a.above = (int)(rnd() & 1), a.wrap_x = wrap;
        a.w = 1 + (int)(rnd() % X), a.h = 1 + (int)(rnd() % Y);
        a.x = (rnd() & 1) ? X - a.w : (int)(rnd() % (X - a.w + 1)), a.y = (rnd() & 1) ? 0 : Y - a.h;
        const int rmax = wrap ? std::min((X - 1) / 2, (int)wxn::MAX_RADIUS) : (int)wxn::MAX_RADIUS;
        a.n_scales = 1 + (int)(rnd() % wxn::MAX_SCALES);
        for (int s = 0; s < a.n_scales; s++) a.rx[s] = s ? (int)(rnd() % (rmax + 1)) : 0, a.ry[s] = s ? (int)(rnd() % (wxn::MAX_RADIUS + 1)) : 0;
        if (a.n_scales > 1) a.rx[1] = rmax, a.ry[1] = wxn::MAX_RADIUS;
        const size_t m = (size_t)a.n_scales * a.w * a.h;
        a.nep = exact<float>(m);
        a.obs_fraction = have_truth ? exact<float>(m) : nullptr;
        wx_ens_nbhd_result o;
        memset(&o, 0x5A, sizeof(o));
        REQUIRE(wxn::nbhd_cells(&a, &o, X, Y, B, field.data(), wall.data(), tf, tw, mask.data()) == WX_OK);
        const int64_t rect_cells = (int64_t)a.w * a.h;
        REQUIRE(o.n_f >= 0 && o.n_f <= rect_cells * n_sel && o.ev_f >= 0 && o.ev_f <= o.n_f && o.n_o >= 0 && o.n_o <= rect_cells && o.ev_o >= 0 && o.ev_o <= o.n_o);
        if (!have_truth) REQUIRE(o.n_o == 0 && o.ev_o == 0);
        for (int s = 0; s < wxn::MAX_SCALES; s++) {
          if (s >= a.n_scales) {
            REQUIRE(o.n_scored[s] == 0 && o.n_unscored[s] == 0 && o.sum_d2[s] == 0.0 && o.sum_f2[s] == 0.0 && o.sum_o2[s] == 0.0);
            continue;
          }
          REQUIRE(o.n_scored[s] >= 0 && o.n_unscored[s] >= 0 && o.n_scored[s] + o.n_unscored[s] == rect_cells);
          REQUIRE(o.sum_d2[s] >= 0.0 && o.sum_f2[s] >= 0.0 && o.sum_o2[s] >= 0.0 && o.sum_d2[s] <= (double)o.n_scored[s] && o.sum_f2[s] <= (double)o.n_scored[s]);
          if (!have_truth) REQUIRE(o.n_scored[s] == 0 && o.sum_d2[s] == 0.0 && o.sum_f2[s] == 0.0);
          if (round == 2) REQUIRE(o.sum_d2[s] == 0.0 && o.sum_f2[s] == o.sum_o2[s]);
          int64_t both = 0;
          for (int64_t i = 0; i < rect_cells; i++) {
            const float pf = a.nep[(size_t)s * rect_cells + i];
            REQUIRE(pf != pf || (pf >= 0.0f && pf <= 1.0f));
            if (a.obs_fraction) {
              const float po = a.obs_fraction[(size_t)s * rect_cells + i];
              REQUIRE(po != po || (po >= 0.0f && po <= 1.0f));
              both += (pf == pf && po == po) ? 1 : 0;
              if (round == 2) REQUIRE((pf != pf && po != po) || pf == po);
            }
          }
          REQUIRE(both == o.n_scored[s]);
        }
        // radius 0 is the point counts: the sum of nep * Nf over the rectangle is ev_f
        {
          double ev = 0.0;
          for (int j = 0; j < a.h; j++)
            for (int i = 0; i < a.w; i++) {
              const size_t g = (size_t)(a.y + j) * X + (size_t)(a.x + i);
              unsigned nf = 0, ef = 0;
              for (int k = 0; k < B; k++) {
                if (!mask[k]) continue;
                float v;
                memcpy(&v, field[k] + 4 * g + a.channel, 4);
                wxn::point_add(nf, ef, v, wall[k][4 * g + 1], a.threshold, a.above);
              }
              const float pf = a.nep[(size_t)j * a.w + i];
              REQUIRE((nf == 0) == (pf != pf));
              if (nf) REQUIRE(pf == (float)((double)ef / (double)nf));
              ev += ef;
            }
          REQUIRE(ev == (double)o.ev_f);
        }
        cells += (long)n * n_sel;
        // the rectangle in two halves: the counters add up
        if (a.w >= 2) {
          wx_ens_nbhd l = a, r = a;
          l.w = a.w / 2, r.x = a.x + l.w, r.w = a.w - l.w;
          l.nep = l.obs_fraction = r.nep = r.obs_fraction = nullptr;
          wx_ens_nbhd_result ol, orr;
          REQUIRE(wxn::nbhd_cells(&l, &ol, X, Y, B, field.data(), wall.data(), tf, tw, mask.data()) == WX_OK);
          REQUIRE(wxn::nbhd_cells(&r, &orr, X, Y, B, field.data(), wall.data(), tf, tw, mask.data()) == WX_OK);
          REQUIRE(ol.ev_f + orr.ev_f == o.ev_f && ol.n_f + orr.n_f == o.n_f && ol.ev_o + orr.ev_o == o.ev_o && ol.n_o + orr.n_o == o.n_o);
          for (int s = 0; s < a.n_scales; s++) REQUIRE(ol.n_scored[s] + orr.n_scored[s] == o.n_scored[s] && ol.n_unscored[s] + orr.n_unscored[s] == o.n_unscored[s]);
        }
        // a refused call writes nothing: nobody selected, a selected member absent, a radius too far, a rectangle outside
        {
          wx_ens_nbhd_result bad = o;
          std::vector<float> before(a.nep, a.nep + m);
          std::vector<uint8_t> nobody(B, 0);
          REQUIRE(wxn::nbhd_cells(&a, &bad, X, Y, B, field.data(), wall.data(), tf, tw, nobody.data()) == WX_E_INVALID);
          float *keep = field[first];
          field[first] = nullptr;
          REQUIRE(wxn::nbhd_cells(&a, &bad, X, Y, B, field.data(), wall.data(), tf, tw, mask.data()) == WX_E_INVALID);
          field[first] = keep;
          wx_ens_nbhd far = a;
          far.ry[0] = wxn::MAX_RADIUS + 1;
          REQUIRE(wxn::nbhd_cells(&far, &bad, X, Y, B, field.data(), wall.data(), tf, tw, mask.data()) == WX_E_INVALID);
          far = a, far.x = X - a.w + 1;
          REQUIRE(wxn::nbhd_cells(&far, &bad, X, Y, B, field.data(), wall.data(), tf, tw, mask.data()) == WX_E_RANGE);
          far = a, far.wrap_x = 1, far.rx[0] = X / 2 + 1;
          if (far.rx[0] <= wxn::MAX_RADIUS) REQUIRE(wxn::nbhd_cells(&far, &bad, X, Y, B, field.data(), wall.data(), tf, tw, mask.data()) == WX_E_RANGE);
          REQUIRE(memcmp(&o, &bad, sizeof(o)) == 0 && memcmp(before.data(), a.nep, 4 * m) == 0);
        }
        for (int i = 0; i < B; i++) free(field[i]), free(wall[i]);
        free(tf), free(tw), free(a.nep), free(a.obs_fraction);
      }
  // the window function on numbers anybody can check
  {
    const wxn::Cell c = wxn::window_cell(1, 4, 1, 2);
    REQUIRE(c.scored && c.pf == 0.25f && c.po == 0.5f && c.t[0] == 0.0625f && c.t[1] == 0.0625f && c.t[2] == 0.25f);
    const wxn::Cell e = wxn::window_cell(0, 0, 1, 2), t = wxn::window_cell(3, 3, 0, 0);
    REQUIRE(!e.scored && e.pf != e.pf && e.po == 0.5f && !t.scored && t.pf == 1.0f && t.po != t.po);
  }
  printf("ens_nbhd_main ok: %ld member-cells\n", cells);
  return 0;
}
