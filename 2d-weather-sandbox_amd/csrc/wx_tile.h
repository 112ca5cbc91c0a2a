// wx_tile.h -- what the tiled dry kernel (wx_dry.h), the row-marching kernels and the host code share: the 64 x 16 tile order,
// fp32 LDS planes, the planar layout of the light texture and the result record of the out-of-line exact advection.
// (Round 1's two fused LDS-tiled kernels for the wet iteration lived here; the single row-marching kernel of wx_wet.h replaced them,
// and the per-pass kernels of wx_kernels.h stay as the independent cross-check -- history in DESIGN.md section 5.)
#pragma once
#include "wx_cells.h"

#include <cstdlib>
#include <algorithm>
// Tuning switches are environment variables ONLY in builds with -DWX_DEBUG (make debug: variants/libwxsim_debug.so; the experiment
// scripts under tools/ load that one through WXSIM_LIB). The shipped library reads no environment variable: it has one launch shape,
// and what a host may choose goes through wx_set_option.
#ifdef WX_DEBUG
inline const char *wx_tune_env(const char *name) { return std::getenv(name); }
#else
inline const char *wx_tune_env(const char *) { return nullptr; }
#endif

namespace wx {

constexpr int TX = 64, TY = 16;

// The light texture of the single-kernel path is stored as three planes: sunlight (x), net heating (y) and the two IR
// fluxes (zw). The boundary stage needs x and y only (8 instead of 16 B/cell); lighting reads x at its four filter taps
// and z / w of one row each, and writes all four channels.
template <typename F, typename F2> struct LightPlanesT {
  F *x, *y;
  F2 *zw;
};
using LightPlanes = LightPlanesT<float, float2>;
using LightPlanesC = LightPlanesT<const float, const float2>;

__device__ __forceinline__ size_t fidx(int x, int y, int X) { return (size_t)y * X + x; }
// wrap for i in [-n, 2n): tile halos of grids at least as large as the halo
__device__ __forceinline__ int wrapfast(int i, int n) { return i < 0 ? i + n : (i >= n ? i - n : i); }

// One workgroup per tile, 2-D grid in the natural order. (An XCD-aware order -- XCD k walks its own column block, so that neighbouring
// tiles share an L2 -- dropped the tiled dry kernel's FETCH_SIZE from 1.18x to 1.05x of the algorithmic bytes at 16384x2048 and made it
// 2 % SLOWER: the re-fetched halo lines came from the Infinity Cache, and the column blocks concentrate each XCD on fewer HBM channels.)
inline dim3 tile_grid(int X, int Y) { return dim3((X + 63) / 64, (Y + 15) / 16); }

// fp32 plane set of a float4 field
template <int H, int W> struct Planes4 {
  float x[H][W], y[H][W], z[H][W], w[H][W];
  __device__ __forceinline__ void put(int r, int c, float4 v)
  {
    x[r][c] = v.x;
    y[r][c] = v.y;
    z[r][c] = v.z;
    w[r][c] = v.w;
  }
  __device__ __forceinline__ float4 get(int r, int c) const { return make_float4(x[r][c], y[r][c], z[r][c], w[r][c]); }
};

namespace fb_ {
// advection is evaluated on x,y in [-1,0] (pressure needs the left and lower neighbour); its 7-point velocity
// stencil reaches 1 further, and so does the back-traced bilinear footprint as long as |v| < 1 cell/iteration
// (REACH = 1; the shaders document velocities as "-1.0 to 1.0", common.glsl:40-41): inputs on [-2,+1].
// Cells with a longer back-trace take the exact out-of-line path.
constexpr int REACH = 1;
constexpr int HL = 1 + REACH, HR = REACH, HD = 1 + REACH, HU = REACH;
constexpr int IW = TX + HL + HR, IH = TY + HD + HU;
constexpr int AW = TX + 1, AH = TY + 1;             // advection results on [-1,0]
constexpr float VMAX = 0.9f;                        // back-traces shorter than this stay inside the staged tile
struct SmemOut { // advection output needed by neighbours (aliases the input tiles after a barrier)
  float vx[AH][AW], vy[AH][AW], T[AH][AW];
  char4 w[AH][AW + 1];
};
} // namespace fb_

struct AdvOut {
  float4 b, w;
  char4 wl;
};

// ---- split iterations of a slab (wx_step_overlap): the issue priority of the edge group ----
// All waves of a slab's launches are resident at once, so launching the edge strips on a high-priority stream alone does not make them
// finish first -- the SIMD's issue priority can. An instrument (WX_SPLIT_PRIO, 0 in shipped builds): the s_setprio level of the waves of
// the edge group's wet launch (0: none).
__device__ __forceinline__ void edge_wave_prio(int prio)
{
#if defined(__HIP_DEVICE_COMPILE__)
  if (prio == 1) __builtin_amdgcn_s_setprio(1);
  else if (prio == 2) __builtin_amdgcn_s_setprio(2);
  else if (prio >= 3) __builtin_amdgcn_s_setprio(3);
#endif
}
// ---- slabs exact at any speed: the fastest |vx| of an exchange period ----
// One iteration's dependency cone is 5 + (1 + floor|vx|) columns per side: the advection pass back-traces `fragCoord - vel` for ANY vel
// (advectionShader.frag:85-99, no clamp) and interpolates from the two columns around the foot point. The marching kernels therefore keep
// the largest |vx| they produce (post-boundary velocities in the wet kernel, the velocity pass's output in the dry one: what the
// back-trace uses) -- one v_max per row step and lane, one wave reduction + at most two atomics per wave -- so that the hosts can size
// the next exchange period (cone = 6 + floor(bound), wx_comm.h) and so that a period whose assumed bound was exceeded is REPORTED.
// Only the flow NEAR THE SLAB EDGES matters: the front of invalid ghost columns moves inwards from the edge of the local array, and a
// jet further inside needs many iterations to get there (it enters the watched zone -- three halo widths from either edge -- at least
// 2 * halo / |vx| iterations before it reaches the ghost columns: several exchange periods). A wave whose strip lies outside the zone
// reports nothing (zone_l / zone_r in strips; whole-domain handles watch everything).
struct VxTrack {
  int *max_bits;   // float bits of the largest |vx| since the last roll (only values >= 0.5 are recorded: below that the cone is 6 anyway)
  int *violation;  // float bits of a |vx| that reached `limit` (0: none)
  float limit;     // |vx| the current period's ghost columns allow (cone - 5); <= 0: whole-domain handle, nothing to check
  int zone_l, zone_r; // strips [0, zone_l) and [zone_r, n) are watched (zone_l >= zone_r: all of them)
  float limit_in;  // the strips in between consume no ghost column -- until |vx| spans the two halo widths that separate them from the ghost
                   // columns: a jet that fast (2 * halo - 8 cells / iteration: a state that has blown up) is a violation too (0: not checked)
};
// The per-lane speed test of the marching kernels (rare path, behind a wave vote): the largest of the eight |velocity components| a
// cell's three back-traces are built from. fmaxf returns the OTHER operand for a NaN; the sum of the magnitudes keeps it, and a NaN among
// them counts as +Inf: such a cell takes the exact path, whose taps are bounds-checked stages and wrapped global reads.
__device__ __forceinline__ float speed8(float q0, float q1, float q2, float q3, float q4, float q5, float q6, float q7)
{
  const float m = fmaxf(fmaxf(fmaxf(fabsf(q0), fabsf(q1)), fmaxf(fabsf(q2), fabsf(q3))), fmaxf(fmaxf(fabsf(q4), fabsf(q5)), fmaxf(fabsf(q6), fabsf(q7))));
  const float sn = ((fabsf(q0) + fabsf(q1)) + (fabsf(q2) + fabsf(q3))) + ((fabsf(q4) + fabsf(q5)) + (fabsf(q6) + fabsf(q7)));
  return sn == sn ? m : __builtin_inff();
}
// |v| for the velocity watch where it is not accumulated row by row: a NaN counts as +Inf (fmaxf would drop it, and a blown-up
// neighbour must not pass for a calm one). The marching loops keep their one v_max per row step and raise +Inf from the rare branch
// behind the wave vote, which a NaN velocity always sets.
__device__ __forceinline__ float vx_mag(float v)
{
  const float a = fabsf(v);
  return a == a ? a : __builtin_inff();
}
__device__ __forceinline__ void vx_track_commit(const VxTrack &t, float lane_max, int lane, int strip = 0)
{
#if defined(__HIP_DEVICE_COMPILE__)
  float m = lane_max;
  if (t.zone_l < t.zone_r && strip >= t.zone_l && strip < t.zone_r) { // (wave-uniform) an interior strip
    if (!(t.limit_in > 0.0f)) return;
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0 && t.violation != nullptr && m >= t.limit_in) atomicMax(t.violation, __float_as_int(m));
    return;
  }
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if (lane == 0 && t.max_bits != nullptr && m >= 0.5f) {
    atomicMax(t.max_bits, __float_as_int(m)); // (bit patterns of positive floats order like ints)
    if (t.limit > 0.0f && m >= t.limit) atomicMax(t.violation, __float_as_int(m));
  }
#endif
}
// the same for kernels that do not track while they run (tiled dry kernel, per-pass kernels) and after uploads: max |vx| of a base texture
// (columns [0, col_l) and [col_r, X) of every row; col_l >= col_r: all columns)
__global__ void k_vx_scan(int X, int Y, int col_l, int col_r, const float4 *__restrict__ base, VxTrack t)
{
  float m = 0.0f, m_in = 0.0f;
  const size_t n = (size_t)X * Y;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % (size_t)X);
    const float v = vx_mag(base[i].x);
    if (col_l >= col_r || x < col_l || x >= col_r)
      m = fmaxf(m, v);
    else
      m_in = fmaxf(m_in, v);
  }
  t.zone_l = t.zone_r = 0;
  vx_track_commit(t, m, threadIdx.x & 63);
  if (t.limit_in > 0.0f) { // the columns in between: only against the interior limit
    t.zone_l = 0;
    t.zone_r = 1;
    vx_track_commit(t, m_in, threadIdx.x & 63, 0);
  }
}

// light texture: interleaved RGBA32F (the reference's layout: per-pass / single-kernel paths, readback, halo buffers of
// those paths) <-> the three planes of the marching kernel
__global__ void k_light_to_planes(size_t n, const float4 *__restrict__ src, LightPlanes dst)
{
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float4 l = src[i];
    dst.x[i] = l.x;
    dst.y[i] = l.y;
    dst.zw[i] = make_float2(l.z, l.w);
  }
}
__global__ void k_light_from_planes(size_t n, LightPlanesC src, float4 *__restrict__ dst)
{
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float2 zw = src.zw[i];
    dst[i] = make_float4(src.x[i], src.y[i], zw.x, zw.y);
  }
}

} // namespace wx
