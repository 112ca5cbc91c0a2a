// Host-only harness for the segment height of the one-iteration dry marching kernel (csrc/wx_march.h: march_seg_rows; no GPU needed:
// without a device the capacity falls back to 256 CUs x 4 SIMDs x WX_MARCH_MINWAVES). Prints, per grid, the strips, the capacity and
// the segment height launch_march_dry starts from: tests/test_vx_watch_cpu.py holds the row segments of its case list to it.
#include "../../2d-weather-sandbox_amd/csrc/wx_wet.h"
#include "../../2d-weather-sandbox_amd/csrc/wx_march.h"
#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
  printf("[");
  for (int a = 1; a + 1 < argc; a += 2) {
    wx::Geo g{};
    g.X = atoi(argv[a]);
    g.Y = atoi(argv[a + 1]);
    const int n_strips = wx::march_dry_strips(g);
    printf("%s{\"X\": %d, \"Y\": %d, \"n_strips\": %d, \"capacity\": %d, \"seg_rows\": %d}", a > 1 ? ", " : "", g.X, g.Y, n_strips, wx::march_capacity(),
           wx::march_seg_rows(n_strips, g.Y));
  }
  printf("]\n");
  return 0;
}
