// wx_precip_ens.h -- the particle pass of an ensemble (wx_ensemble_step): the four launches a lone handle makes per iteration --
// k_precipitation, k_splat_classify, k_splat_box, k_splat_clear -- over ALL members that carry droplets, member = blockIdx.y, blockIdx.x =
// the workgroup's place in the lone kernel's grid. The bodies are the lone kernels' own program text (wx_precip_bodies.h, included by
// both as wx_wet_march_body.h is): a member cannot drift from a lone handle, and the lone kernels stay as they were. A workgroup never spans
// members, so the 256-thread workgroups, the wave64 ballots and the one px_count atomic per workgroup carry over; their targets are the
// member's own DevState, SplatGrid and textures, taken from its slot of the device table.
//
// WX_OPT_SPLAT_ORDER 1 ("for tests"): the deposit records are sorted PER MEMBER -- the member's own hipcub::DeviceRadixSort + k_splat_runs
// between the shared precipitation and classify launches, on the ensemble's stream -- not by one segmented sort: any stable sort gives
// the same bits, and the members' key / value buffers stay where a borrowed wx_step expects them. Members of either order share the
// precipitation launch (DetSplat::key == NULL selects atomics per member).
#pragma once
#include "wx_kernels.h"
#include "wx_wet.h"
#include <algorithm>

namespace wx {

// one member's particle pass of one iteration (device table, staged with the marching kernel's WetEnsSlot table in the same copy)
struct PrecipEnsSlot {
  const FullCtx *ctx; // the member's Geo and Uni (wx_set_params); iterNum / iterI are this iteration's
  float iterNum;
  int n_drops;
  const float *drops_in;
  float *drops_out;
  const float4 *base_in, *water_in; // the iteration's post-pressure base and post-advection water (the marching kernel's outputs)
  const float *t_in;                // ... its tdisp plane
  const char4 *wall_in;
  DevState *st;
  SplatGrid sg;
  float3 *fb;
  float2 *dep;
  DetSplat det;
  int par, seam;    // SplatGrid::work parity of this iteration
  LightningArgs la; // (refresh_inactive: this member's iteration counter % 600 == 0)
};
static_assert(sizeof(PrecipEnsSlot) % 8 == 0, "table slots hold pointers");

// (each kernel names the member's arguments as the lone kernel names its parameters and includes the lone kernel's body)
__global__ __launch_bounds__(256) void k_precipitation_ens(const PrecipEnsSlot *__restrict__ table)
{
  const PrecipEnsSlot &sl = table[blockIdx.y];
  const Geo g = sl.ctx->g;
  Uni u = sl.ctx->u;
  u.iterNum = sl.iterNum;
  u.iterI = (int)u.iterNum;
  const int n_drops = sl.n_drops;
  const float *__restrict__ drops_in = sl.drops_in;
  const float4 *__restrict__ base_in = sl.base_in;
  const float4 *__restrict__ water_in = sl.water_in;
  DevState *__restrict__ st = sl.st;
  float *__restrict__ drops_out = sl.drops_out;
  const SplatGrid sg = sl.sg;
  const SlabP sp{0, g.X, 0, g.X, 0, 0, nullptr, nullptr, nullptr, 0}; // whole-domain members
  const float *__restrict__ t_in = sl.t_in;
  const DetSplat det = sl.det;
  const char4 *__restrict__ wall_in = sl.wall_in;
#define WX_PRECIP_BODY 1
#include "wx_precip_bodies.h"
}

__global__ __launch_bounds__(256) void k_splat_classify_ens(const PrecipEnsSlot *__restrict__ table)
{
  const PrecipEnsSlot &sl = table[blockIdx.y];
  const int X = sl.ctx->g.X, Y = sl.ctx->g.Y, mailbox = sl.la.mailbox, par = sl.par;
  const SplatGrid sg = sl.sg;
#define WX_PRECIP_BODY 2
#include "wx_precip_bodies.h"
}

__global__ __launch_bounds__(256, 4) void k_splat_box_ens(const PrecipEnsSlot *__restrict__ table)
{
  const PrecipEnsSlot &sl = table[blockIdx.y];
  const int X = sl.ctx->g.X, Y = sl.ctx->g.Y, seam = sl.seam, mailbox = sl.la.mailbox, par = sl.par;
  const SplatGrid sg = sl.sg;
  const DevState *__restrict__ st = sl.st;
  float3 *__restrict__ fb = sl.fb;
  float2 *__restrict__ dep = sl.dep;
#define WX_PRECIP_BODY 3
#include "wx_precip_bodies.h"
}

__global__ __launch_bounds__(256) void k_splat_clear_ens(const PrecipEnsSlot *__restrict__ table)
{
  const PrecipEnsSlot &sl = table[blockIdx.y];
  const int par = sl.par;
  const SplatGrid sg = sl.sg;
  const LightningArgs la = sl.la;
#define WX_PRECIP_BODY 4
#include "wx_precip_bodies.h"
}

// Launch shapes: the lone launches' rules with the device divided among the members (every kernel walks its work grid-stride within the
// member's row of the grid, so any size is correct). n_drops, X, Y are the members' common ones; tiles = SplatGrid TXn * TYn.
struct PrecipEnsShape {
  int precip_wgs, classify_wgs, box_wgs, clear_wgs;
};
inline PrecipEnsShape precip_ens_shape(int n_members, int n_drops, int tiles)
{
  PrecipEnsShape p;
  // ceil(n_drops / 256) chunks per member, capped so that all members together stay at the lone kernel's 768 workgroups
  p.precip_wgs = std::max(1, std::min((n_drops + 255) / 256, 768 / n_members));
  p.classify_wgs = (tiles + 255) / 256; // (one thread per tile: not a grid-stride kernel)
  // no more workgroups than the device holds at once (k_splat_box's rule), at least one per member
  p.box_wgs = std::max(1, std::min(tiles, splat_box_grid() / n_members));
  p.clear_wgs = std::max(1, std::min(tiles, 2048 / n_members));
  return p;
}
// the three splat launches behind the precipitation launch (and behind the order-1 members' sorts)
inline void launch_precipitation_ens(const PrecipEnsSlot *table, int n_members, const PrecipEnsShape &p, hipStream_t stream)
{
  hipLaunchKernelGGL(k_precipitation_ens, dim3(p.precip_wgs, n_members), dim3(256), 0, stream, table);
}
inline void launch_splat_ens(const PrecipEnsSlot *table, int n_members, const PrecipEnsShape &p, hipStream_t stream)
{
  hipLaunchKernelGGL(k_splat_classify_ens, dim3(p.classify_wgs, n_members), dim3(256), 0, stream, table);
  hipLaunchKernelGGL(k_splat_box_ens, dim3(p.box_wgs, n_members), dim3(256), 0, stream, table);
  hipLaunchKernelGGL(k_splat_clear_ens, dim3(p.clear_wgs, n_members), dim3(256), 0, stream, table);
}

} // namespace wx
