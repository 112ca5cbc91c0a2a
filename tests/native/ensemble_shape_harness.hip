// Host-only harness for the share-of-chip launch shape of an ensemble member (csrc/wx_wet.h: wet_launch_shape_member). Arguments:
// triples X Y n_members. Prints, per triple, the member's segment table next to the lone handle's (wet_launch_shape) for every row-bands
// mode: tests/test_ensemble_cpu.py checks coverage and that a lone member gets the lone handle's shape. No GPU needed (without a device
// the capacity falls back to 256 CUs x 12 waves).
#include "../../2d-weather-sandbox_amd/csrc/wx_wet.h"
#include <cstdio>
#include <cstdlib>

static void print_shape(const char *name, const wx::WetLaunch &w)
{
  printf("\"%s\": {\"n_strips\": %d, \"bands\": %d, \"n_seg\": %d, \"groups_x\": %d, \"start\": [", name, w.n_strips, w.segs.bands, w.segs.n_seg, wx::ens_member_groups(w));
  for (int s = 0; s <= w.segs.n_seg; s++) printf("%s%d", s ? ", " : "", w.segs.start[s]);
  printf("]}");
}

int main(int argc, char **argv)
{
  printf("[");
  bool first = true;
  for (int a = 1; a + 2 < argc; a += 3) {
    wx::Geo g{};
    g.X = atoi(argv[a]);
    g.Y = atoi(argv[a + 1]);
    const int members = atoi(argv[a + 2]);
    for (int mode = 0; mode <= 2; mode++) {
      printf("%s{\"X\": %d, \"Y\": %d, \"members\": %d, \"bands_mode\": %d, \"capacity\": %d, \"share\": %d, ", first ? "" : ", ", g.X, g.Y, members, mode, wx::wet_capacity(),
             wx::wet_member_share(g, members, 0));
      first = false;
      print_shape("member", wx::wet_launch_shape_member(g, -1, mode, members));
      printf(", ");
      print_shape("lone", wx::wet_launch_shape(g, -1, mode));
      printf("}");
    }
  }
  printf("]\n");
  return 0;
}
