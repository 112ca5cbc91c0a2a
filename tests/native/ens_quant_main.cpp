// Stand-alone driver of the quantile kernels' per-cell function (csrc/wx_ens_quant_cell.h) for a host-compiler build under
// AddressSanitizer / UBSan (tests/test_ensemble_quantiles_cpu.py): wxq::quant_cells over randomised buffers that are allocated to the
// byte -- a read or write one cell outside is a report -- with every interpolation, any number of quantiles, masks with absent
// members, a rank member or none, member counts from 1 to beyond the staged limit, and output planes wanted or not. Checks what needs
// no second implementation: the keys are an order-preserving bijection, quantiles are monotone in p and lie between the extremes,
// counts add up, a refused descriptor writes nothing.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../2d-weather-sandbox_amd/csrc/wx_ens_quant_cell.h"

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
static T *exact(size_t n) // n elements and not a byte more (never NULL: one element for n = 0 would hide an overrun, so n >= 1 here)
{
  return (T *)malloc(n * sizeof(T));
}

int main()
{
  // the keys: order-preserving, -0.0 == +0.0, finite keys below the three markers, value_of inverts
  for (int k = 0; k < 200000; k++) {
    const float a = wxq::f32_of(rnd()), b = wxq::f32_of(rnd());
    if (!wxq::f32_finite(a) || !wxq::f32_finite(b)) continue;
    const uint32_t ka = wxq::key_of(a), kb = wxq::key_of(b);
    REQUIRE((a < b) == (ka < kb) && (a == b) == (ka == kb));
    REQUIRE(wxq::key_entered(ka) && wxq::value_of(ka) == a && (a != 0.0f || wxq::f32_bits(wxq::value_of(ka)) == 0u));
  }
  REQUIRE(wxq::key_of(-0.0f) == wxq::key_of(0.0f) && wxq::key_of(3.4028234663852886e38f) == 0xFF7FFFFFu && wxq::key_of(-3.4028234663852886e38f) == 0x00800000u);
  REQUIRE(wxq::cell_key(1.0f, 0) == wxq::KEY_WALL && wxq::cell_key(NAN, 3) == wxq::KEY_NONFINITE && wxq::cell_key(-INFINITY, 3) == wxq::KEY_NONFINITE);

  const int member_counts[] = {1, 2, 3, 7, 64, 65, 300};
  const size_t cell_counts[] = {1, 5, 64, 129};
  long cells = 0;
  for (int B : member_counts)
    for (size_t n : cell_counts)
      for (int interp = 0; interp < 3; interp++) {
        const int n_tab = B + 1; // the last member is the one that may be ranked
        std::vector<float *> field(n_tab, nullptr);
        std::vector<int8_t *> wall(n_tab, nullptr);
        std::vector<uint8_t> mask(n_tab, 0);
        mask[rnd() % B] = 1;
        const bool with_rank = (rnd() & 1) != 0;
        for (int i = 0; i < n_tab; i++) {
          if (i < B && (rnd() % 3)) mask[i] = 1;
          if (!mask[i] && !(i == B && with_rank) && (rnd() & 1)) continue; // an unused member may be absent
          field[i] = exact<float>(4 * n);
          wall[i] = exact<int8_t>(4 * n);
          for (size_t k = 0; k < 4 * n; k++) {
            const uint32_t bits = (rnd() & 3) ? (0x3C000000u + (rnd() & 0x07FFFFFFu)) | (rnd() & 0x80000000u) : ((rnd() & 1) ? rnd() : (rnd() & 0x80000000u)); // ordinary values, any bit pattern, zeros
            memcpy(field[i] + k, &bits, 4);
            wall[i][k] = (int8_t)((rnd() % 5) ? (rnd() & 0x7F) : 0);
          }
        }
        int n_sel = 0;
        for (int i = 0; i < B; i++) n_sel += mask[i];
        wx_ens_quant o;
        memset(&o, 0, sizeof(o));
        o.n_q = (int)(rnd() % (WX_ENS_QUANT_MAX + 1));
        o.interp = interp;
        o.rank_member = with_rank ? B : -1;
        for (int j = 0; j < o.n_q; j++) o.p[j] = (float)j / (float)(o.n_q > 1 ? o.n_q - 1 : 1); // ascending, 0 .. 1
        if (o.n_q > 2) o.p[1] = 0.1f;
        o.q = (o.n_q > 0) ? exact<float>((size_t)o.n_q * 4 * n) : nullptr;
        o.count = exact<int32_t>(4 * n);
        o.n_wall = (rnd() & 1) ? exact<int32_t>(n) : nullptr;
        o.n_below = with_rank ? exact<int32_t>(4 * n) : nullptr;
        o.n_equal = with_rank && (rnd() & 1) ? exact<int32_t>(4 * n) : nullptr;
        REQUIRE(wxq::quant_cells(n_tab, n, field.data(), wall.data(), mask.data(), &o) == WX_OK);
        for (size_t i = 0; i < n; i++)
          for (int c = 0; c < 4; c++) {
            const int cnt = o.count[4 * i + c];
            REQUIRE(cnt >= 0 && cnt <= n_sel);
            if (o.n_wall) REQUIRE(o.n_wall[i] >= 0 && o.n_wall[i] + cnt <= n_sel);
            for (int j = 0; j < o.n_q; j++) {
              const float q = o.q[((size_t)j * n + i) * 4 + c];
              REQUIRE(cnt > 0 ? wxq::f32_finite(q) : q != q);
              REQUIRE(wxq::f32_bits(q) != 0x80000000u);
              if (j > 0 && cnt > 0 && o.p[j] >= o.p[j - 1]) REQUIRE(q >= o.q[((size_t)(j - 1) * n + i) * 4 + c]); // monotone in p
            }
            if (o.n_below) {
              const int below = o.n_below[4 * i + c];
              REQUIRE(below >= -1 && below <= cnt);
              if (o.n_equal) REQUIRE((o.n_equal[4 * i + c] == -1) == (below == -1) && below + o.n_equal[4 * i + c] <= cnt);
            }
          }
        cells += (long)n * n_sel;
        // a refused descriptor writes nothing: the ranked member selected, a NaN quantile
        std::vector<int32_t> before(o.count, o.count + 4 * n);
        wx_ens_quant bad = o;
        bad.n_q = 1, bad.p[0] = NAN;
        float one[4] = {7.0f, 7.0f, 7.0f, 7.0f};
        bad.q = one;
        REQUIRE(wxq::quant_cells(n_tab, n, field.data(), wall.data(), mask.data(), &bad) == WX_E_INVALID);
        bad = o, bad.rank_member = 0;
        for (int i = 0; i < B; i++)
          if (mask[i]) bad.rank_member = i;
        REQUIRE(wxq::quant_cells(n_tab, n, field.data(), wall.data(), mask.data(), &bad) == WX_E_INVALID);
        REQUIRE(memcmp(before.data(), o.count, 16 * n) == 0 && one[0] == 7.0f);
        for (int i = 0; i < n_tab; i++) {
          free(field[i]);
          free(wall[i]);
        }
        free(o.q), free(o.count), free(o.n_wall), free(o.n_below), free(o.n_equal);
      }
  // positions: k <= k1 <= n - 1, 0 <= g < 1, p = 1 is the last value exactly
  for (int k = 0; k < 200000; k++) {
    const int n = 1 + (int)(rnd() % 65535u);
    const float p = (float)(rnd() >> 8) / 16777216.0f;
    const wxq::Position ps = wxq::position_of(p, n);
    REQUIRE(ps.k >= 0 && ps.k <= ps.k1 && ps.k1 <= n - 1 && ps.k1 <= ps.k + 1 && ps.g >= 0.0 && ps.g < 1.0);
    const wxq::Position last = wxq::position_of(1.0f, n);
    REQUIRE(last.k == n - 1 && last.k1 == n - 1 && last.g == 0.0);
  }
  printf("ens_quant_main ok: %ld member-cells\n", cells);
  return 0;
}
