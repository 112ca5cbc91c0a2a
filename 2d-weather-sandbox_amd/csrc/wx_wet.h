// wx_wet.h -- the WHOLE wet iteration (reference draws 1-7, app.js:5832-5930: velocity -> curl -> vorticity -> boundary ->
// advection -> pressure -> lighting) as ONE row-MARCHING kernel (gfx950). One wavefront owns a 64-column strip (a workgroup
// = four neighbouring strips, no barrier between them) and walks up the rows of its segment; per step (newest input row r) it
//
//   loads row r+1 (prefetch)  |  velocity(r-1)  |  curl(r-2)  |  vortForce(r-3)  |  boundary(r-3)  |  advection(r-4)  |
//   pressure(r-4) + lighting(r-4) -> stores row r-4
//
// * every intermediate texture of the reference (velocity output, curl, vortForce, post-boundary base / water / wall,
//   advection output) lives in registers or in a wave-PRIVATE LDS ring of the last six rows; nothing but the iteration's
//   inputs and outputs touches HBM: base 16 R + 16 W, water 16 R + 16 W, wall 4 R + 4 W, light 16 R + 16 W = 104 B/cell
//   (round 1's two-kernel form: 184 B/cell; reference pass structure: ~380 B/cell);
// * vertical neighbours are the wave's own earlier rows (ring or carried registers), horizontal neighbours of values that
//   were just computed come from whole-wave DPP shifts (v_mov_b32_dpp wave_shr / wave_shl: one VALU instruction, no LDS
//   round trip), data-dependent taps (advection's back-trace, the sun ray) from the ring;
// * the boundary stage overwrites its input rows IN PLACE (the only later readers of the pre-boundary values are the same
//   lane one row up: carried in registers), so six ring rows serve both the pre- and the post-boundary state;
// * no vertical halo is re-loaded or re-computed, there are no workgroup barriers (the wave's LDS queue is in order;
//   wavefront-scope fences keep the compiler from reordering across stages); 56 of the 64 lanes produce output
//   (cone of the seven chained stencils: 4 columns per side for |v| < 0.9 cell/iteration);
// * cells whose back-trace is longer than that (|v| >= 0.9 cell/iteration: the core of a strong updraft) are only RECORDED by the
//   marching loop: the (up to three) OUTPUT cells each of them feeds -- its own, the right neighbour's pressure, the upper
//   neighbour's pressure / lighting -- are appended to a device list, and a second small kernel (k_wet_fix, one wavefront per list
//   entry, spread over the whole chip) recomputes them exactly and overwrites the placeholders: 64 lanes rebuild an 8 x 8 patch
//   of post-boundary texels around the cell from the iteration's inputs, three lanes advect from that patch. The hot loop contains
//   no call and no scratch access, and a storm core costs microseconds (round 2: the recording wave redid such cells serially from
//   global memory after its loop, ~1 ms PER CELL -- one fast cell tripled the iteration time);
// * global loads are issued one step ahead of their use (software prefetch), each with the lag its consumer has (base / wall
//   row r+1, water and light row r-1, feedback row r-2), and the stores of a row are issued at the top of the NEXT step, right
//   behind the prefetch: the only vmcnt wait of the common path (top of the step) then covers operations that have had a
//   whole step to complete -- gfx9 counts loads and stores in one in-order counter.
// * launch shape (wet_launch_shape): the rows are cut into eight bands, one per XCD, each band into a few full segments followed
//   by segments of 1/2, 1/4 (and 1/8) the height -- short segments at the END of the dispatch order shorten the drain phase of
//   the launch; grids lower than 512 rows use column blocks per XCD instead.
// Same per-cell arithmetic as the per-pass kernels (wx_cells.h): bit-identical results.
#pragma once
#include "wx_cells.h"
#include "wx_tile.h"
#include <cstddef>
#include <type_traits>
#include <cstdlib>
#include <algorithm>

namespace wx {

#ifndef WX_WET_MINWAVES
#define WX_WET_MINWAVES 4
#endif
#ifndef WX_WET_WPB
#define WX_WET_WPB 4 // wavefronts per workgroup: independent strips (no barrier between them); the dispatcher spreads the waves of
                     // ONE workgroup evenly over the four SIMDs of a CU, which it does not guarantee for single-wave workgroups
#endif
#ifndef WX_ABL_FORCE_AIR
#define WX_ABL_FORCE_AIR 0 // (instruction-budget builds: every row takes the free-air instantiations; wrong near terrain)
#endif

struct FullCtx { // static per wx_set_params; the per-launch items (buffer pointers, iterNum) travel as arguments
  Geo g;
  Uni u;
  const float *initial_T, *snd_T, *snd_W, *snd_Vel;
};

struct WetIn {
  const float4 *base;   // base_0: post-pressure state of the previous iteration
  const char4 *wall;    // wall_0
  const float4 *water;  // water_1: post-advection water of the previous iteration
  LightPlanesC l0;      // lightTexture_0 (what boundaryShader samples)
  LightPlanesC lsrc;    // source of this iteration's lighting pass (light_0 or light_1)
  const float3 *fb;     // precipitation feedback (three channels) / deposition, or NULL when known to be zero
  const float2 *dep;
  const unsigned char *fb_zero; // per 64x16 tile t: [2t] feedback all zero there, [2t + 1] deposition all zero there (may be NULL)
  const float4 *zero_row;       // one row (X texels) of zeros: what rows of all-zero tiles are "loaded" from
  int fb_txn;
};
struct WetOut {
  float4 *base;      // post-pressure
  char4 *wall;
  float4 *water;     // post-advection
  LightPlanes light;
  float *p_disp;     // optional (OPT_OUT): post-advection PRESSURE -- all of baseTexture_1 (what the display samples) that the post-pressure base texture and
                     // t_disp do not already hold: pressure_cell changes P everywhere and T directly above land only (k_base_disp_assemble makes the RGBA texels on demand)
  float4 *water0;    // optional (OPT_OUT): post-boundary water (waterTexture_0); NULL = not stored (made on demand)
  float *curl;       // optional (OPT_OUT)
  float *t_disp;     // optional (runtime): post-advection temperature where the pressure pass changes it, for the droplets and for baseTexture_1 on demand
#ifdef WX_WET_TIMING
  unsigned long long *cycles; // (tuning builds) per wave: s_memtime at start / end
#endif
};

// Output cells left to the exact path (see k_wet_fix): appended by the marching kernel, consumed by the fix kernel of the same
// launch group. count keeps counting past cap (the host reports the overflow as an error: the state has blown up).
struct WetFixList {
  int *count;
  int2 *cells;
  int cap;
  const int *hint_host; // (host address of the same word)
  int *fastest; // bit pattern of the largest |velocity component| [cells / iteration] that sent a cell to this list (wx_fastest_velocity)
  int *hint; // host-visible word (pinned, mapped): the fix pass leaves the length of the list it consumed here; the host looks at it
             // (stale, never waited for) to size the NEXT fix launches -- a launch over the whole chip costs 10 us to find an empty list
};

// ---- exact out-of-line path: the post-boundary texel of an ARBITRARY cell recomputed from global memory (velocity, curl
//      and vortForce evaluated on the fly). Only used for output cells fed by a back-trace longer than 0.9 cells. ----
struct WetSlowArgs {
  const FullCtx *ctx;
  WetIn in;
  float iterNum;
};
struct GWetRecomputeAcc {
  const Uni &u_;
  const WetIn &in_;
  int X, Y, x, y;
  __device__ __forceinline__ int wx_(int dx) const { return wrapmod(x + dx, X); }
  __device__ __forceinline__ int wy_(int dy) const { return wrapmod(y + dy, Y); }
  __device__ __forceinline__ float4 vel_at(int xx, int yy) const
  { // velocity pass output at (xx,yy) (already wrapped)
    const int xr = xx + 1 == X ? 0 : xx + 1, yu = yy + 1 == Y ? 0 : yy + 1;
    return velocity_cell(u_, in_.base[fidx(xx, yy, X)], in_.base[fidx(xr, yy, X)].z, in_.base[fidx(xx, yu, X)].z, in_.wall[fidx(xx, yy, X)].y);
  }
  __device__ __forceinline__ float curl_at(int xx, int yy) const
  {
    const int xr = xx + 1 == X ? 0 : xx + 1, yu = yy + 1 == Y ? 0 : yy + 1;
    const float4 v = vel_at(xx, yy);
    return curl_cell(v.x, v.y, vel_at(xr, yy).y, vel_at(xx, yu).x);
  }
  __device__ __forceinline__ float4 base(int dx, int dy) const { return vel_at(wx_(dx), wy_(dy)); }
  __device__ __forceinline__ char4 wall(int dx, int dy) const { return in_.wall[fidx(wx_(dx), wy_(dy), X)]; }
  __device__ __forceinline__ float4 water(int dx, int dy) const { return in_.water[fidx(wx_(dx), wy_(dy), X)]; }
  __device__ __forceinline__ float2 vort(int dx, int dy) const
  {
    const int xx = wx_(dx), yy = wy_(dy);
    const int xl = xx == 0 ? X - 1 : xx - 1, xr = xx + 1 == X ? 0 : xx + 1, yd = yy == 0 ? Y - 1 : yy - 1, yu = yy + 1 == Y ? 0 : yy + 1;
    return vorticity_cell(curl_at(xx, yy), curl_at(xl, yy), curl_at(xr, yy), curl_at(xx, yd), curl_at(xx, yu));
  }
  __device__ __forceinline__ float light_y0() const { return in_.l0.y[fidx(x, y, X)]; }
  __device__ __forceinline__ float light_x0() const { return in_.l0.x[fidx(x, y, X)]; }
  __device__ __forceinline__ float2 light_xy_up() const
  {
    const size_t i = fidx(x, y + 1 > Y - 1 ? Y - 1 : y + 1, X); // light textures: CLAMP_TO_EDGE in T
    return make_float2(in_.l0.x[i], in_.l0.y[i]);
  }
  __device__ __forceinline__ bool has_fb() const { return in_.fb != nullptr; }
  __device__ __forceinline__ float4 fb() const
  {
    if (!in_.fb) return make_float4(0.f, 0.f, 0.f, 0.f);
    const float3 v = in_.fb[fidx(x, y, X)];
    return make_float4(v.x, v.y, v.z, 0.f);
  }
  __device__ __forceinline__ float2 dep() const { return in_.dep ? in_.dep[fidx(x, y, X)] : make_float2(0.f, 0.f); }
};
struct BOut {
  float4 b, w;
  char4 wl;
};
__device__ __noinline__ BOut wet_boundary_texel_global(const WetSlowArgs *__restrict__ sa, int x, int y)
{
  const FullCtx *c = sa->ctx;
  GWetRecomputeAcc a{c->u, sa->in, c->g.X, c->g.Y, x, y};
  BOut o;
  boundary_cell(c->u, sa->iterNum, (int)sa->iterNum, c->g, c->initial_T, x, y, a, o.b, o.w, o.wl);
  return o;
}
struct GWetAdvectAcc {
  const WetSlowArgs *sa;
  int X, Y, x, y;
  __device__ __forceinline__ BOut at(int dx, int dy) const { return wet_boundary_texel_global(sa, wrapmod(x + dx, X), wrapmod(y + dy, Y)); }
  __device__ __forceinline__ float4 base(int dx, int dy) const { return at(dx, dy).b; }
  __device__ __forceinline__ char4 wall(int dx, int dy) const { return at(dx, dy).wl; }
  __device__ __forceinline__ float4 base_off(int dx, int dy) const { return at(dx, dy).b; }
  __device__ __forceinline__ float4 water_off(int dx, int dy) const { return at(dx, dy).w; }
  __device__ __forceinline__ char4 wall_off(int dx, int dy) const { return at(dx, dy).wl; }
};
__device__ __noinline__ AdvOut wet_advection_cell_recompute(const WetSlowArgs *__restrict__ sa, int x, int y)
{
  const FullCtx *c = sa->ctx;
  GWetAdvectAcc a{sa, c->g.X, c->g.Y, x, y};
  AdvOut o;
  advection_cell(c->u, c->g, c->initial_T, c->snd_T, c->snd_W, c->snd_Vel, x, y, a, o.b, o.w, o.wl);
  return o;
}
struct GWetLightAcc {
  LightPlanesC l;
  float4 water_;
  char4 wall_;
  float T0, Td;
  int X, x;
  __device__ __forceinline__ float T(int dy) const { return dy == 0 ? T0 : Td; }
  __device__ __forceinline__ float4 water() const { return water_; }
  __device__ __forceinline__ char4 wall() const { return wall_; }
  __device__ __forceinline__ float sun_at(int dx, int j) const { return l.x[fidx(wrapmod(x + dx, X), j, X)]; }
  __device__ __forceinline__ float ir_down_at(int j) const { return l.zw[fidx(x, j, X)].x; }
  __device__ __forceinline__ float ir_up_at(int j) const { return l.zw[fidx(x, j, X)].y; }
};
// every output of the iteration at cell (x, y) -- post-pressure base, post-advection water / wall, light -- from the
// iteration's inputs alone, any back-trace length
__device__ __noinline__ void wet_output_cell_exact(const FullCtx *__restrict__ c, const WetIn *__restrict__ in, const WetOut *__restrict__ out, float iterNum,
                                                   int opt_out, int x, int y)
{
  const WetSlowArgs sa{c, *in, iterNum};
  const int X = c->g.X, Y = c->g.Y;
  const AdvOut o0 = wet_advection_cell_recompute(&sa, x, y);
  const AdvOut oL = wet_advection_cell_recompute(&sa, x == 0 ? X - 1 : x - 1, y);
  const AdvOut oD = wet_advection_cell_recompute(&sa, x, y == 0 ? Y - 1 : y - 1);
  const size_t gi = fidx(x, y, X);
  out->base[gi] = pressure_cell(o0.b, oL.b.x, oD.b.y, oD.b.w, oD.wl.x, oD.wl.y);
  out->water[gi] = o0.w;
  out->wall[gi] = o0.wl;
  GWetLightAcc la{in->lsrc, o0.w, o0.wl, o0.b.w, oD.b.w, X, x};
  const float4 l = lighting_cell(c->u, c->g, x, y, la);
  out->light.x[gi] = l.x;
  out->light.y[gi] = l.y;
  out->light.zw[gi] = make_float2(l.z, l.w);
  if (opt_out) out->p_disp[gi] = o0.b.z;
  if (out->t_disp) out->t_disp[gi] = o0.b.w;
}

// ---- the wave-private ring ----
constexpr int WOUT = 56;          // output columns per wave: lanes 4 .. 59
constexpr int WLO = 4;            // first output lane
constexpr int WPAD = 1;           // never-written pad entry on each side of a ring row (lane -1 / lane 64 reads land there)
constexpr int WRW = 64 + 2 * WPAD;
constexpr int WQ = 3;             // rows r-5 .. r-3 of the post-boundary base / wall / water planes: slot = row mod 3 (round 4: rows
                                  // r-2 .. r are carried in registers until the boundary stage needs their horizontal neighbours --
                                  // the ring is what bounds the occupancy: 50 -> 35 plane-rows = 3 -> 4 waves per SIMD)
constexpr int WL = 4;             // rows r-5 .. r-2 of the source light planes: slot = row & 3
struct WetRing {
  float P[WQ][WRW], T[WQ][WRW], vx[WQ][WRW], vy[WQ][WRW];
  char4 wl[WQ][WRW];
  float qx[WQ][WRW], qy[WQ][WRW], qz[WQ][WRW], qw[WQ][WRW];
  float lx[WL][WRW], lw[WL][WRW]; // sunlight and upward IR of the source light texture
};
static_assert(sizeof(WetRing) == (5 * WQ + 4 * WQ + 2 * WL) * WRW * 4, "ring layout");

// whole-wave shifts: lane i <- lane i-1 / lane i+1; the edge lane keeps its own value
__device__ __forceinline__ float wave_from_left(float v)
{
  const int i = __float_as_int(v);
  return __int_as_float(__builtin_amdgcn_update_dpp(i, i, 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_from_right(float v)
{
  const int i = __float_as_int(v);
  return __int_as_float(__builtin_amdgcn_update_dpp(i, i, 0x130 /* wave_shl:1 */, 0xf, 0xf, false));
}
// orders the wave's LDS traffic across stages for the compiler; the hardware executes one wave's LDS operations in order
__device__ __forceinline__ void wave_fence()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ char4 unpack_wall(int w)
{
  return make_char4((signed char)(w & 0xff), (signed char)((w >> 8) & 0xff), (signed char)((w >> 16) & 0xff), (signed char)(w >> 24));
}

// boundary stage, row yb: own texel, the row below and the water / light_0 texels of the row above in registers, the base / wall
// texels of the row above and the horizontal wall neighbours in the ring
struct MWBoundaryAcc {
  const WetRing &rg;
  int li, o0;              // ring column; in-plane offset of ring row yb (its pre-boundary T and wall: the horizontal neighbours)
  float vxU, TU;           // row above: velocity-pass vx, T (carried registers)
  char4 wU;
  float4 b00, q00, qU;     // velocity output / pre-boundary water of the own cell; pre-boundary water of the cell above
  char4 w00, wD;
  float vxD, TD, qzD, qwD; // row below: velocity-pass vx, pre-boundary T, soil moisture / snow of the pre-boundary water
  float qzL, qwL, qzR, qwR; // left / right neighbour's soil moisture / snow (fetched only in the iterations that use them)
  float2 vf;
  float vfLy, vfDx;
  float l0x, l0y, l0xU, l0yU; // light_0 sunlight / net heating at the own cell and the cell above (row clamped)
  float4 fb_;
  float2 dep_;
  bool hasfb;
  __device__ __forceinline__ float4 base(int dx, int dy) const
  {
    if (dx == 0 && dy == 0) return b00;
    if (dy == 1) return make_float4(vxU, 0.f, 0.f, TU);
    if (dy == -1) return make_float4(vxD, 0.f, 0.f, TD);
    return make_float4(0.f, 0.f, 0.f, (&rg.T[0][0])[o0 + li + dx]); // (+-1, 0): temperature of the neighbouring sea cell
  }
  __device__ __forceinline__ float4 water(int dx, int dy) const
  {
    if (dx == 0 && dy == 0) return q00;
    if (dx == 0 && dy == -1) return make_float4(0.f, 0.f, qzD, qwD);
    if (dx == 0 && dy == 1) return qU;
    return dx < 0 ? make_float4(0.f, 0.f, qzL, qwL) : make_float4(0.f, 0.f, qzR, qwR);
  }
  __device__ __forceinline__ char4 wall(int dx, int dy) const
  {
    if (dx == 0 && dy == 0) return w00;
    if (dy == -1) return wD;
    if (dy == 1) return wU;
    return (&rg.wl[0][0])[o0 + li + dx];
  }
  __device__ __forceinline__ float2 vort(int dx, int dy) const
  {
    if (dx == 0 && dy == 0) return vf;
    if (dx == -1) return make_float2(0.f, vfLy); // the boundary pass uses .y of the left and .x of the lower neighbour only
    return make_float2(vfDx, 0.f);
  }
  __device__ __forceinline__ float light_y0() const { return l0y; }
  __device__ __forceinline__ float light_x0() const { return l0x; }
  __device__ __forceinline__ float2 light_xy_up() const { return make_float2(l0xU, l0yU); }
  __device__ __forceinline__ bool has_fb() const { return hasfb; }
  __device__ __forceinline__ float4 fb() const { return fb_; }
  __device__ __forceinline__ float2 dep() const { return dep_; }
};

// advection stage, row ya: post-boundary rows ya-1 .. ya+1 in the ring
struct MWAdvAcc {
  const WetRing &rg;
  int li;
  int ob[3]; // in-plane offsets of rows ya-1, ya, ya+1 (wave-uniform; the base / wall and the water planes share their slots)
  __device__ __forceinline__ float4 base(int dx, int dy) const
  {
    const int o = ob[dy + 1] + li + dx;
    return make_float4((&rg.vx[0][0])[o], (&rg.vy[0][0])[o], (&rg.P[0][0])[o], (&rg.T[0][0])[o]);
  }
  __device__ __forceinline__ char4 wall(int dx, int dy) const { return (&rg.wl[0][0])[ob[dy + 1] + li + dx]; }
  __device__ __forceinline__ float4 base_off(int dx, int dy) const { return base(dx, dy); }
  __device__ __forceinline__ char4 wall_off(int dx, int dy) const { return wall(dx, dy); }
  __device__ __forceinline__ float4 water_off(int dx, int dy) const
  {
    const int o = ob[dy + 1] + li + dx;
    return make_float4((&rg.qx[0][0])[o], (&rg.qy[0][0])[o], (&rg.qz[0][0])[o], (&rg.qw[0][0])[o]);
  }
};
// bilinear footprint (dx0, dy0 in {-1, 0}): the two rows are picked per lane from the three wave-uniform row offsets
struct MWFp {
  const WetRing &rg;
  int b0, b1, q0, q1; // offsets (row offset + column) of the lower / upper footprint row in the base and water planes
  __device__ __forceinline__ float4 base(int i, int j) const
  {
    const int o = (j ? b1 : b0) + i;
    return make_float4((&rg.vx[0][0])[o], (&rg.vy[0][0])[o], (&rg.P[0][0])[o], (&rg.T[0][0])[o]);
  }
  __device__ __forceinline__ char4 wall(int i, int j) const { return (&rg.wl[0][0])[(j ? b1 : b0) + i]; }
  __device__ __forceinline__ float4 water(int i, int j) const
  {
    const int o = (j ? q1 : q0) + i;
    return make_float4((&rg.qx[0][0])[o], (&rg.qy[0][0])[o], (&rg.qz[0][0])[o], (&rg.qw[0][0])[o]);
  }
};
__device__ __forceinline__ MWFp make_fp(const MWAdvAcc &a, int dx0, int dy0)
{
  const bool lo = dy0 < 0; // dy0 is -1 or 0 for every cell that takes this path
  const int c = a.li + dx0;
  const int o0 = (lo ? a.ob[0] : a.ob[1]) + c, o1 = (lo ? a.ob[1] : a.ob[2]) + c;
  return MWFp{a.rg, o0, o1, o0, o1};
}

// lighting stage, row y (an OUTPUT row: unwrapped == wrapped row index); ring row k of the light planes holds texture row clamp(k)
struct MWLightAcc {
  const WetRing &rg;
  int li;
  float T0, Tdown, lz_up;
  float4 water_;
  char4 wall_;
  __device__ __forceinline__ float T(int dy) const { return dy == 0 ? T0 : Tdown; } // dy in {0,-1}
  __device__ __forceinline__ float4 water() const { return water_; }
  __device__ __forceinline__ char4 wall() const { return wall_; }
  __device__ __forceinline__ float sun_at(int dx, int j) const { return rg.lx[(j + 8) & (WL - 1)][li + dx]; }
  __device__ __forceinline__ float ir_down_at(int) const { return lz_up; }                           // row min(y+1, Y-1): carried register
  __device__ __forceinline__ float ir_up_at(int j) const { return rg.lw[(j + 8) & (WL - 1)][li]; } // row max(y-1, 0)
};

// global access as (wave-uniform row pointer) + (per-lane 32-bit byte offset): the form the hardware addresses with a scalar base
// register pair and one offset VGPR -- no 64-bit vector arithmetic per access
// (the readfirstlane pair pins the row pointer to scalar registers and keeps the loop optimiser from turning the access into a
// per-lane 64-bit pointer induction variable)
__device__ __forceinline__ unsigned long long uniform_addr(const void *p)
{
  const unsigned long long v = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}
#if defined(__HIP_DEVICE_COMPILE__)
template <class T> __device__ __forceinline__ T ld_row(const T *row, unsigned &byte_off)
{
  typedef const __attribute__((address_space(1))) char *GBytes; // (an integer round trip would otherwise yield a generic "flat" pointer)
  typedef const __attribute__((address_space(1))) T *GPtr;
  // keeps the zero-extension next to the access (instruction selection folds it only within a block). The offset is taken by
  // reference and redefined IN PLACE: on a by-value copy every access paid a v_mov of the loop-invariant original (15 per row step)
  asm("" : "+v"(byte_off));
  return *(GPtr)((GBytes)uniform_addr(row) + byte_off);
}
template <class T> __device__ __forceinline__ void st_row(T *row, unsigned &byte_off, T v)
{
  typedef __attribute__((address_space(1))) char *GBytes;
  asm("" : "+v"(byte_off));
  // (plain stores: nontemporal ones bring the re-read halo and warm-up lines from 1.25x back to 1.19x of the algorithmic bytes without
  // moving the time, and cost a cache-sized grid 17 %)
  typedef __attribute__((address_space(1))) T *GPtr;
  *(GPtr)((GBytes)uniform_addr(row) + byte_off) = v;
}
#else // host pass of the single-source compile: same meaning, never executed
template <class T> __device__ __forceinline__ T ld_row(const T *row, unsigned &byte_off) { return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(row) + byte_off); }
template <class T> __device__ __forceinline__ void st_row(T *row, unsigned &byte_off, T v) { *reinterpret_cast<T *>(reinterpret_cast<char *>(row) + byte_off) = v; }
#endif
// by-value forms (a private copy of the offset per access): what the dry marching kernel uses -- there the in-place form is 2 % slower
template <class T> __device__ __forceinline__ T ld_row_v(const T *row, unsigned byte_off) { return ld_row(row, byte_off); }
template <class T> __device__ __forceinline__ void st_row_v(T *row, unsigned byte_off, T v) { st_row(row, byte_off, v); }
__device__ __forceinline__ int ring_back(int s, int k, int n) // slot of the row k steps behind the one in slot s (ring of n)
{
  const int v = s - k;
  return v < 0 ? v + n : v;
}

// A launch covers the strips [strip_lo, strip_lo + n_strips) of the n_strips_all strips of the (slab of the) grid: the whole
// width normally; the edge strips and the interior separately where a slab overlaps its halo exchange with compute.
// OPT_OUT: also store what only display-side consumers see (curl, post-boundary water, post-advection base): last iteration of a
// wx_step call. HAS_FB: the precipitation feedback / deposition textures may be non-zero.
// fix: the list the output cells fed by a back-trace longer than 0.9 cells are appended to (k_wet_fix recomputes them).
// The rows are cut into segments of (possibly) different heights: start[s] .. start[s+1]. Rows near terrain take the general,
// branchy instantiations and cost about twice as much as free air, so the host makes the bottom segments shorter
// (wet_launch_shape) and all waves of a launch finish together.
constexpr int WMAXSEG = 128;
struct WetSegs {
  int n_seg;
  int bands;              // != 0: XCD k takes the row band [k*Y/8, (k+1)*Y/8) of ALL strips; start[] is relative to it
  int start[WMAXSEG + 1];
};
// The argument block of one marching launch: the parameter list of k_march_wet as a struct -- the layout of its kernel-argument segment,
// and of one member's slot in an ensemble's device table (k_march_wet_ens)
struct WetKArgs {
  const FullCtx *ctx;
  float iterNum;
  WetIn in;
  WetOut out;
  WetFixList fix;
  int n_strips, strip_lo, n_strips_all;
  WetSegs segs;
  int split_at, strip_lo2;
  int edge_prio; // issue priority of the waves (edge_wave_prio, wx_tile.h): != 0 only in the edge group of a split iteration
  VxTrack vx;
};
// one member's slot of an ensemble's device table
struct WetEnsSlot {
  WetKArgs ka;
  int *overflow; // the member's own overflow flag (k_wet_fix_ens)
  int pad_[2 + (16 - (sizeof(WetKArgs) + sizeof(int *) + 8) % 16) % 16 / 4];
};
static_assert(sizeof(WetEnsSlot) % 16 == 0, "table slots keep the 16-byte alignment of the wide scalar loads");
// QUIET: no brush input and no airplane event in this iteration (the host looks at the uniforms): advection_cell without those sections.
template <bool OPT_OUT, bool HAS_FB, bool QUIET>
__global__ __launch_bounds__(64 * WX_WET_WPB, WX_WET_MINWAVES) void k_march_wet(const FullCtx *__restrict__ ctx, float iterNum, WetIn in_arg, WetOut out_arg,
                                                                    WetFixList fix_arg, int n_strips, int strip_lo,
                                                                    int n_strips_all, WetSegs segs, int split_at, int strip_lo2, int edge_prio_arg, VxTrack vx_arg)
{
  typedef WetKArgs KArgs; // layout of the kernel-argument segment (the parameter list as a struct)
  // The ~22 plane pointers are read from the kernel-argument segment (constant address space) where they are used: separate
  // two-dword scalar loads that the register allocator can re-issue, instead of 44 SGPRs preloaded in wide loads that it can only
  // spill -- and an SGPR spill / restore is a v_writelane / v_readlane, i.e. a VECTOR instruction in a VALU-bound loop. The struct
  // parameters (in_arg ... vx_arg) are therefore never named below: they give the segment its layout.
  typedef const __attribute__((address_space(4))) char *KBytes;
#if defined(__HIP_DEVICE_COMPILE__)
  const KBytes ka_c = (KBytes)__builtin_amdgcn_kernarg_segment_ptr();
#else // host pass of the single-source compile: the body is parsed, never emitted
  const KBytes ka_c = nullptr;
#endif
  // (the body is program text shared with k_march_wet_ens: wx_wet_march_body.h. Included, not called -- an inlined function taking these
  // arguments changes the instruction stream of this kernel, and its layout is worth 2-4 % of the clean flow)
#include "wx_wet_march_body.h"
}

// The ensemble instantiation (wx_ensemble_step): B independent simulations of one size in ONE launch. Member = blockIdx.y -- a workgroup
// never spans members, so everything derived from the member's arguments (iterNum -> smooth_iter, the segment table, the strip counts)
// stays wave-uniform. The member's argument block is its slot of a device table (one WetEnsSlot per member, written by a stream-ordered
// copy in front of the launch), read through the constant address space exactly as the lone kernel reads its kernel-argument segment:
// the row loop keeps its scalar loads where it has them, and the scalars the body names directly come from the same slot. gridDim.x is a
// multiple of 8 (blockIdx.x & 7 is still the XCD) sized for the member with the most segments; the surplus workgroups of the others
// exit at once. Whole-domain members, no edge group. HAS_FB as on a lone handle: the members of a launch all hand in feedback textures
// (their droplets ran in the iteration before) or none does -- the driver partitions by it.
template <bool OPT_OUT, bool HAS_FB, bool QUIET>
__global__ __launch_bounds__(64 * WX_WET_WPB, WX_WET_MINWAVES) void k_march_wet_ens(const WetEnsSlot *__restrict__ table)
{
  typedef WetKArgs KArgs;
  typedef const __attribute__((address_space(4))) char *KBytes;
  const KBytes ka_c = (KBytes)(const char *)table + (size_t)blockIdx.y * sizeof(WetEnsSlot);
  const __attribute__((address_space(4))) KArgs &ka = *(const __attribute__((address_space(4))) KArgs *)ka_c;
  const FullCtx *__restrict__ ctx = ka.ctx;
  const float iterNum = ka.iterNum;
  const int n_strips = ka.n_strips, strip_lo = ka.strip_lo, n_strips_all = ka.n_strips_all, split_at = ka.split_at, strip_lo2 = ka.strip_lo2;
  const __attribute__((address_space(4))) WetSegs &segs = ka.segs;
#include "wx_wet_march_body.h"
}

#undef WX_WALL_RAW
#undef WX_H_SET
#undef WX_H_ROT

// ---- k_wet_fix: the output cells on the fix list, recomputed exactly -- one wavefront per cell ----
// Output (X0, Y0) = pressure + lighting of the advected cells (X0, Y0), (X0 - 1, Y0) [vx of the left neighbour] and (X0, Y0 - 1)
// [vy, T, wall of the lower one]. The 64 lanes rebuild the 8 x 8 patch [X0 - 4, X0 + 3] x [Y0 - 4, Y0 + 3] of POST-BOUNDARY texels from
// the iteration's inputs (velocity, curl and vortForce evaluated on the fly, wet_boundary_texel_global), three lanes advect the three
// cells from that patch with the very same advection_cell -- it covers every back-trace shorter than two cells -- and lane 0
// finishes and stores the cell. Should a footprint leave the patch (|v| >= 2: the state has blown up) the fully general path from
// global memory (wet_output_cell_exact) takes over. Recomputing an output is idempotent (always from the iteration's inputs), so
// duplicates on the list and the order of the entries do not matter.
constexpr int WPATCH = 8, WPATCH_C = 4;
struct WetPatch {
  float vx[WPATCH * WPATCH], vy[WPATCH * WPATCH], P[WPATCH * WPATCH], T[WPATCH * WPATCH];
  float qx[WPATCH * WPATCH], qy[WPATCH * WPATCH], qz[WPATCH * WPATCH], qw[WPATCH * WPATCH];
  char4 wl[WPATCH * WPATCH];
};
struct WetPatchAcc {
  const WetPatch &p;
  int cx, cy; // patch coordinates of the own cell
  bool *bad;  // set when a texel outside the patch is asked for
  __device__ __forceinline__ int at(int dx, int dy) const
  {
    const int x = cx + dx, y = cy + dy;
    if (x < 0 || x >= WPATCH || y < 0 || y >= WPATCH) {
      *bad = true;
      return 0;
    }
    return y * WPATCH + x;
  }
  __device__ __forceinline__ float4 base(int dx, int dy) const
  {
    const int i = at(dx, dy);
    return make_float4(p.vx[i], p.vy[i], p.P[i], p.T[i]);
  }
  __device__ __forceinline__ char4 wall(int dx, int dy) const { return p.wl[at(dx, dy)]; }
  __device__ __forceinline__ float4 base_off(int dx, int dy) const { return base(dx, dy); }
  __device__ __forceinline__ char4 wall_off(int dx, int dy) const { return wall(dx, dy); }
  __device__ __forceinline__ float4 water_off(int dx, int dy) const
  {
    const int i = at(dx, dy);
    return make_float4(p.qx[i], p.qy[i], p.qz[i], p.qw[i]);
  }
};

// The patch of post-boundary texels is built COOPERATIVELY, stage by stage through LDS, the way the reference's passes follow each
// other (round 3, second version; the first let every lane rebuild its texel recursively from global memory -- velocity, curl and
// vortForce of the same cells up to 45 times per lane -- and took ~33 us per list entry):
//   base / wall      13 x 13  [-6, 6]   loaded once
//   velocity output  12 x 12  [-6, 5]   velocity_cell
//   curl             11 x 11  [-6, 4]   curl_cell
//   vortForce         9 x 9   [-5, 3]   vorticity_cell
//   boundary          8 x 8   [-4, 3]   boundary_cell on an accessor that reads the stages (water, light_0, feedback: global)
// Same cell functions, same operands: the same values as the marching loop computes.
constexpr int WSB = 13, WSV = 12, WSC = 11, WSF = 9; // stage widths; all stages start at offset -6 but vortForce (-5) and the patch (-4)
struct WetFixStage {
  float bx[WSB * WSB], by[WSB * WSB], bP[WSB * WSB], bT[WSB * WSB];
  char4 bw[WSB * WSB];
  float vx[WSV * WSV], vy[WSV * WSV];
  float cu[WSC * WSC];
  float fx[WSF * WSF], fy[WSF * WSF];
};
struct WetStageBoundaryAcc { // the interface of GWetRecomputeAcc, served from the stages; (px, py) = patch coordinates of the own texel
  const WetFixStage &st;
  const Uni &u_;
  const WetIn &in_;
  int X, Y, x, y; // wrapped global coordinates of the own texel
  int px, py;
  __device__ __forceinline__ float4 base(int dx, int dy) const
  { // the velocity pass's output: vx, vy from the velocity stage, P and T unchanged (offset -6 -> patch offset -4: +2)
    const int iv = (py + 2 + dy) * WSV + (px + 2 + dx), ib = (py + 2 + dy) * WSB + (px + 2 + dx);
    return make_float4(st.vx[iv], st.vy[iv], st.bP[ib], st.bT[ib]);
  }
  __device__ __forceinline__ char4 wall(int dx, int dy) const { return st.bw[(py + 2 + dy) * WSB + (px + 2 + dx)]; }
  __device__ __forceinline__ float4 water(int dx, int dy) const { return in_.water[fidx(wrapmod(x + dx, X), wrapmod(y + dy, Y), X)]; }
  __device__ __forceinline__ float2 vort(int dx, int dy) const
  { // vortForce stage starts at -5: patch offset -4 -> +1
    const int i = (py + 1 + dy) * WSF + (px + 1 + dx);
    return make_float2(st.fx[i], st.fy[i]);
  }
  __device__ __forceinline__ float light_y0() const { return in_.l0.y[fidx(x, y, X)]; }
  __device__ __forceinline__ float light_x0() const { return in_.l0.x[fidx(x, y, X)]; }
  __device__ __forceinline__ float2 light_xy_up() const
  {
    const size_t i = fidx(x, y + 1 > Y - 1 ? Y - 1 : y + 1, X); // light textures: CLAMP_TO_EDGE in T
    return make_float2(in_.l0.x[i], in_.l0.y[i]);
  }
  __device__ __forceinline__ bool has_fb() const { return in_.fb != nullptr; }
  __device__ __forceinline__ float4 fb() const
  {
    if (!in_.fb) return make_float4(0.f, 0.f, 0.f, 0.f);
    const float3 v = in_.fb[fidx(x, y, X)];
    return make_float4(v.x, v.y, v.z, 0.f);
  }
  __device__ __forceinline__ float2 dep() const { return in_.dep ? in_.dep[fidx(x, y, X)] : make_float2(0.f, 0.f); }
};
// the 8 x 8 patch of post-boundary texels around (cx, cy), all 64 lanes of the wave
__device__ __noinline__ void wet_fix_build_patch(const FullCtx *__restrict__ c, const WetIn *__restrict__ in, float iterNum, WetFixStage *__restrict__ stp,
                                                 WetPatch *__restrict__ ptp, int cx, int cy, int lane)
{
  WetFixStage &st = *stp;
  WetPatch &pt = *ptp;
  const int X = c->g.X, Y = c->g.Y;
  for (int i = lane; i < WSB * WSB; i += 64) { // base_0 and wall_0 of the 13 x 13 neighbourhood
    const int sy = i / WSB, sx = i - sy * WSB;
    const size_t gi = fidx(wrapmod(cx - 6 + sx, X), wrapmod(cy - 6 + sy, Y), X);
    const float4 b = in->base[gi];
    st.bx[i] = b.x;
    st.by[i] = b.y;
    st.bP[i] = b.z;
    st.bT[i] = b.w;
    st.bw[i] = in->wall[gi];
  }
  wave_fence();
  for (int i = lane; i < WSV * WSV; i += 64) { // velocity pass
    const int sy = i / WSV, sx = i - sy * WSV, ib = sy * WSB + sx;
    const float4 v = velocity_cell(c->u, make_float4(st.bx[ib], st.by[ib], st.bP[ib], st.bT[ib]), st.bP[ib + 1], st.bP[ib + WSB], st.bw[ib].y);
    st.vx[i] = v.x;
    st.vy[i] = v.y;
  }
  wave_fence();
  for (int i = lane; i < WSC * WSC; i += 64) { // curl
    const int sy = i / WSC, sx = i - sy * WSC, iv = sy * WSV + sx;
    st.cu[i] = curl_cell(st.vx[iv], st.vy[iv], st.vy[iv + 1], st.vx[iv + WSV]);
  }
  wave_fence();
  for (int i = lane; i < WSF * WSF; i += 64) { // vortForce of [-5, 3]: curl index +1
    const int sy = i / WSF, sx = i - sy * WSF, ic = (sy + 1) * WSC + (sx + 1);
    const float2 f = vorticity_cell(st.cu[ic], st.cu[ic - 1], st.cu[ic + 1], st.cu[ic - WSC], st.cu[ic + WSC]);
    st.fx[i] = f.x;
    st.fy[i] = f.y;
  }
  wave_fence();
  { // boundary pass, one patch texel per lane
    const int px = lane & (WPATCH - 1), py = lane >> 3;
    const int gx = wrapmod(cx - WPATCH_C + px, X), gy = wrapmod(cy - WPATCH_C + py, Y);
    const WetStageBoundaryAcc a{st, c->u, *in, X, Y, gx, gy, px, py};
    float4 bb, bq;
    char4 bwl;
    boundary_cell(c->u, iterNum, (int)iterNum, c->g, c->initial_T, gx, gy, a, bb, bq, bwl);
    pt.vx[lane] = bb.x;
    pt.vy[lane] = bb.y;
    pt.P[lane] = bb.z;
    pt.T[lane] = bb.w;
    pt.qx[lane] = bq.x;
    pt.qy[lane] = bq.y;
    pt.qz[lane] = bq.z;
    pt.qw[lane] = bq.w;
    pt.wl[lane] = bwl;
  }
  wave_fence();
}

template <bool OPT_OUT>
__global__ __launch_bounds__(256) void k_wet_fix(const FullCtx *__restrict__ ctx, float iterNum, WetIn in, WetOut out, int *__restrict__ count,
                                                 const int2 *__restrict__ cells, int cap, int *__restrict__ overflow, int *__restrict__ hint)
{
  // (shared with k_wet_fix_ens as program text, like the marching kernel's body)
#include "wx_wet_fix_body.h"
}

// The fix pass of an ensemble launch: member = blockIdx.y walks its OWN list (grid-stride over the gridDim.x workgroups of its row of the
// grid -- the arrival ticket counts those), reports to its own overflow flag and hint word.
template <bool OPT_OUT>
__global__ __launch_bounds__(256) void k_wet_fix_ens(const WetEnsSlot *__restrict__ table)
{
  const WetEnsSlot &sl = table[blockIdx.y];
  const FullCtx *__restrict__ ctx = sl.ka.ctx;
  const float iterNum = sl.ka.iterNum;
  // (copies, as the lone kernel's by-value arguments are: the out-of-line exact path the two kernels share takes their addresses, and
  // handing it pointers into the table instead changes ITS code -- and with it the lone kernel's)
  const WetIn in = sl.ka.in;
  const WetOut out = sl.ka.out;
  int *__restrict__ count = sl.ka.fix.count;
  const int2 *__restrict__ cells = sl.ka.fix.cells;
  const int cap = sl.ka.fix.cap;
  int *__restrict__ overflow = sl.overflow;
  int *__restrict__ hint = sl.ka.fix.hint;
#include "wx_wet_fix_body.h"
}

// Segmentation. The grid is cut into about WX_WET_ROUNDS times as many waves as the device holds at once (the hardware deals
// workgroups to CUs as earlier ones retire; bottom segments are dispatched first), and rows below `air_from_row` -- the lowest
// row above which every cell is free air, -1 if unknown -- count WX_WET_ALPHA times a free-air row when the segment borders
// are placed. Measured at 16384x2048 (gpurun_out/r2j..r2l): 1 round 29-34, 2 rounds 36-37, 4 rounds 38-40, 6 rounds 38-40
// Gcell-steps/s -- many short waves beat few long ones although each segment re-runs 8 warm-up rows; weighting terrain rows
// (alpha 2-2.5) is worth +15 % with one round and nothing from two rounds on.
// Why (tuning build -DWX_WET_TIMING: s_memtime per wave, profiles/r02_wet_wave_timing.txt): the kernel is VALU-bound at 3 waves per
// SIMD (524 VALU instructions per row step x 4 cycles x 3 waves = the ~6800 cycles a wave takes per row), and the SIMD issues its
// OLDEST ready wave first. With one round of 9 long segments the first-dispatched waves run at 6000 cycles / row and the last at 8100;
// when the old ones retire nothing refills their slots and the young ones finish at 1-2 waves per SIMD, which cannot hide their own
// memory latency: 77 % of the SIMD-time is used, against 89 % with four rounds, and that costs more than the warm-up rows saved
// (0.87-0.90 ms against 0.835-0.845). Rotating s_setprio per step equalises the rates but marches the waves of a SIMD in lock-step
// into their memory waits (-5 %); giving older segments more rows shifts the rates with it.
// Halo columns are not the problem: an s_barrier per row step, which keeps the four strips of a workgroup on the same rows, lowers
// FETCH_SIZE by 2 % and costs 6 % of time -- the neighbouring strips' lines already hit in L2; what the counters show above the
// algorithmic bytes (reads 1.15x) is the 8 warm-up rows per segment.
#ifndef WX_WET_ROUNDS
#define WX_WET_ROUNDS 4
#endif
struct WetLaunch {
  int n_strips;
  WetSegs segs;
};
inline int wet_capacity()
{
  static int capacity = 0;
  if (!capacity) {
    int dev = 0, ncu = 0, nb = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_march_wet<false, false, true>, 64 * WX_WET_WPB, 0) != hipSuccess || ncu <= 0 || nb <= 0) {
      capacity = 256 * 4 * WX_WET_MINWAVES;
    } else {
      // the occupancy API can answer one workgroup per CU too many (MI355X_MICROARCH.md, "Residency"): bound it by what the kernel's own
      // register and LDS footprint admit -- 512 registers per lane and SIMD in granules of 8, 160 KiB of LDS per CU; a workgroup is
      // WX_WET_WPB waves, one per SIMD
      hipFuncAttributes fa;
      int by_regs = nb, by_lds = nb;
      if (hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k_march_wet<false, false, true>)) == hipSuccess) {
        if (fa.numRegs > 0) by_regs = (512 / (((fa.numRegs + 7) / 8) * 8)) * 4 / WX_WET_WPB;
        if (fa.sharedSizeBytes > 0) by_lds = (int)(163840 / fa.sharedSizeBytes);
        if (wx_tune_env("WX_MARCH_DEBUG")) fprintf(stderr, "[wx_wet] numRegs=%d lds=%zu: blocks/CU by registers %d, by LDS %d, occupancy API %d\n", fa.numRegs, fa.sharedSizeBytes, by_regs, by_lds, nb);
      }
      nb = std::max(1, std::min(nb, std::min(by_regs, by_lds)));
      capacity = ncu * nb * WX_WET_WPB;
    }
    if (wx_tune_env("WX_MARCH_DEBUG")) fprintf(stderr, "[wx_wet] CUs=%d blocks/CU=%d capacity=%d\n", ncu, nb, capacity);
  }
  return capacity;
}
inline double wet_alpha()
{
  double alpha = 1.0; // cost of a row below air_from_row relative to a free-air row when the segment borders are placed
  if (const char *e = wx_tune_env("WX_WET_ALPHA")) alpha = atof(e) >= 1.0 ? atof(e) : alpha;
  return alpha;
}
// bands_mode (WX_OPT_ROW_BANDS): 0 = column blocks, 1 = row bands on grids at least 512 rows high (default), 2 = row bands wherever
// a band has two rows (tests: the shape of wide slabs on small grids)
// (capacity: the wave slots the launch may count on -- the whole chip for a lone handle, a member's share in an ensemble)
inline WetLaunch wet_launch_shape_cap(const Geo &g, int air_from_row, int bands_mode, const int capacity)
{
  WetLaunch w;
  // Grids at least 512 rows high: XCD k takes the row band [k*Y/8, (k+1)*Y/8) of ALL strips instead of a column block of every
  // segment -- each XCD then streams one contiguous eighth of every plane: -3..-8 % kernel time at 16384x2048 and 32768x4096,
  // -5 % on a 4192x4096 slab, -9 % on a 2144x2048 one (profiles/r02_wet_tail_shape.txt).
  // Round 5, the reference's own sizes (tools/ref_sizes_bands.py, profiles/r05_ref_sizes.txt): NARROW grids below 512 rows gain from the
  // bands too -- 2500 x 300 (the reference's default: 45 strips) 45.3 -> 36.9 us per iteration, 5000 x 400 65.4 -> 60.0 -- while wide low
  // ones lose (16000 x 300: 120.5 -> 142.6): bands also for grids of fewer than 128 strips that are at least 128 rows high.
  // Round 6 (tools/ref_sizes_minrows.py, profiles/r06_ref_sizes_minrows.txt): the border re-measured on 17 sizes -- 7200 x 256 / x 448
  // (129 strips) -15 / -8 % with bands, 8000 x 300 ... 500 (143 strips) -5 % (x 350: +2.5 %), 10000 x 480 (179) +9 %, 12000 and 16000
  // columns even or worse: fewer than 146 strips. The minimum segment height below is at its optimum for every reference size.
  const int strips_all = (g.X + WOUT - 1) / WOUT;
  bool bands = bands_mode >= 2 ? g.Y >= 16 : (bands_mode != 0 && (g.Y >= 8 * 64 || (strips_all < 146 && g.Y >= 128)));
  if (const char *e = wx_tune_env("WX_WET_BANDS")) bands = atoi(e) >= 2 ? g.Y >= 16 : (atoi(e) != 0 && g.Y >= 8 * 64); // (2: tests force it on small grids)
  const int Y = bands ? (g.Y + 7) / 8 : g.Y; // (bands: the shape of ONE band; the kernel clips it to the band's own height)
  w.segs.bands = bands ? 1 : 0;
  w.n_strips = (g.X + WOUT - 1) / WOUT;
  int rounds = WX_WET_ROUNDS, minrows = 24; // (narrow slabs: 2144x2048 runs 17 % faster with 30-row unit segments + tail than with equal 32-row ones)
  const double alpha = wet_alpha();
  if (const char *e = wx_tune_env("WX_WET_ROUNDS")) rounds = atoi(e) > 0 ? atoi(e) : rounds;
  // Grids that cannot fill the chip with 24-row segments (the reference's own sizes, 100 x 100 ... 2048 x 512): a wave's row steps
  // are serial, so parallelism is worth more than the 8 redundant warm-up rows of a segment -- rows per segment that fill the chip
  // once, at least 4 (2 while there is less than one wave per CU). 100x100: 64 -> 21 us per iteration, 1024x512: 87 -> 39,
  // 2048x512: 86 -> 51; from 4096x1024 on nothing changes (profiles/r04_small_grid_segments.txt).
  {
    const long long cap = capacity, per_row_set = (long long)w.n_strips * (bands ? 8 : 1);
    auto waves_at = [&](int m) { return per_row_set * ((Y + m - 1) / m); };
    if (waves_at(minrows) < cap) {
      const int fill = (int)(per_row_set * Y / cap), floor_rows = waves_at(4) <= 256 ? 2 : 4;
      minrows = std::max(floor_rows, std::min(minrows, fill));
    }
  }
  if (const char *e = wx_tune_env("WX_WET_MINROWS")) minrows = atoi(e) > 0 ? atoi(e) : minrows;
  // workgroups per segment: 8 XCD column blocks x ceil(strips of the block / waves per workgroup); the device holds capacity / WPB
  const int wg_per_seg = bands ? 8 * ((w.n_strips + WX_WET_WPB - 1) / WX_WET_WPB) : 8 * (((w.n_strips + 7) / 8 + WX_WET_WPB - 1) / WX_WET_WPB);
  int n_seg = (int)((long long)rounds * (capacity / WX_WET_WPB) / wg_per_seg);
  n_seg = n_seg < 1 ? 1 : (n_seg > WMAXSEG ? WMAXSEG : n_seg);
  if (n_seg > (Y + minrows - 1) / minrows) n_seg = (Y + minrows - 1) / minrows; // (8 warm-up rows per segment are redundant work)
  const int A = (air_from_row < 0 || air_from_row > Y) ? 0 : air_from_row;           // unknown: uniform segments
  const double total = alpha * A + (Y - A);
  // weights of the segments in dispatch order (bottom first): equal, the tail shape below, or an explicit list
  // WX_WET_SPEC="29x1,5x0.5,5x0.25" (count x weight, ...; the counts give the number of segments): short segments LAST shorten the
  // drain phase of the launch, in which finished waves are not replaced
  double wt[WMAXSEG];
  for (int sg = 0; sg < n_seg; sg++) wt[sg] = 1.0;
  if (!wx_tune_env("WX_WET_NOTAIL")) {
    // default shape: (rounds - 1) rounds of full segments, then about half a round each of segments of weight 1/2, 1/4 and 1/8.
    // The launch ends with a drain phase in which finished waves are not replaced; short segments at the end of the dispatch order
    // make it short: -5 % kernel time against equal segments (interleaved A/B, profiles/r02_wet_tail_shape.txt)
    const double per_round = (double)(capacity / WX_WET_WPB) / wg_per_seg;
    // (a band segment is a large part of a round already: one segment per tail level there)
    const int c = bands ? 1 : ((int)(per_round / 2.0 + 0.5) > 1 ? (int)(per_round / 2.0 + 0.5) : 1);
    const double rr_list[6] = {(double)rounds, 3.0, 2.0, 1.75, 1.5, 1.25};
    for (int ri = 0; ri < 6; ri++) { // (fewer rounds if a unit segment would fall below `minrows` rows; else equal segments)
      const double rr = rr_list[ri];
      if (rr > rounds) continue;
      int n_full = (int)((rr - 1.0) * per_round + 0.1); // (16384x2048: 3.9 -> 3 full segments of 68 rows per band: 0.770-0.772 against 0.789-0.826 ms with 4 of 54, two boxes)
      if (bands) { // unit segments of about 64 rows
        const int by_rows = (int)(Y / 64.0 + 0.5) - 1;
        n_full = n_full > by_rows ? n_full : by_rows;
        // ... and not below ~52 while the launch still holds well over one round of waves: at four waves per SIMD the rounds rule
        // alone asks for 5 x 44 rows + tail at 16384 x 2048; 4 x 52 + 1/2 + 1/4 + 1/8 is 1.3 % faster on one placement
        // (profiles/r04_ring_diet.txt). Narrow slabs stay with the short segments that fill the chip.
        const int by_unit = (int)(Y / 52.0 - 0.875 + 0.5);
        // (... "well over": three and a half rounds. The 8192-column slab of a 2-GPU run -- 148 strips, two rounds of 52-row units -- runs
        // 6.6 % faster with the ten 25-row units + tail the rounds rule gives it: profiles/r05_slab_segment_specs.txt)
        if (n_full > by_unit && by_unit >= 1 && (long long)w.n_strips * 8 * (by_unit + 3) >= 7LL * capacity / 2) n_full = by_unit;
      }
      const int n8 = bands ? (n_full >= 4 ? 1 : 0) : c - 1; // segments of weight 1/8
      const int n = n_full + 2 * c + n8;
      const double units = n_full + c * 0.5 + c * 0.25 + n8 * 0.125;
      if (n_full >= 1 && n <= WMAXSEG && Y / units >= minrows) {
        n_seg = n;
        for (int sg = 0; sg < n; sg++) wt[sg] = sg < n_full ? 1.0 : (sg < n_full + c ? 0.5 : (sg < n_full + 2 * c ? 0.25 : 0.125));
        break;
      }
    }
  }
  if (const char *e = wx_tune_env("WX_WET_SPEC")) {
    int n = 0;
    for (const char *q = e; *q && n < WMAXSEG;) {
      char *end = nullptr;
      const long cnt = strtol(q, &end, 10);
      if (end == q || *end != 'x') break;
      const double wv = strtod(end + 1, &end);
      for (long k = 0; k < cnt && n < WMAXSEG; k++) wt[n++] = wv > 0.0 ? wv : 1.0;
      q = *end == ',' ? end + 1 : end;
      if (*q == 0) break;
    }
    if (n > 0 && n <= (Y + 7) / 8) n_seg = n;
  }
  // border s at the row where the accumulated cost reaches the share of segments 0 .. s-1
  w.segs.start[0] = 0;
  double wsum = 0.0, wacc = 0.0;
  for (int sg = 0; sg < n_seg; sg++) wsum += wt[sg];
  for (int sg = 1; sg < n_seg; sg++) {
    wacc += wt[sg - 1];
    const double c = total * wacc / wsum;
    int y = c <= alpha * A ? (int)(c / alpha + 0.5) : A + (int)(c - alpha * A + 0.5);
    if (y <= w.segs.start[sg - 1]) y = w.segs.start[sg - 1] + 1;
    w.segs.start[sg] = y < Y ? y : Y;
  }
  w.segs.start[n_seg] = Y;
  while (n_seg > 1 && w.segs.start[n_seg - 1] >= Y) n_seg--; // (tiny grids: drop empty segments)
  w.segs.start[n_seg] = Y;
  w.segs.n_seg = n_seg;
  return w;
}

inline WetLaunch wet_launch_shape(const Geo &g, int air_from_row, int bands_mode = 1) { return wet_launch_shape_cap(g, air_from_row, bands_mode, wet_capacity()); }

// The shape of ONE MEMBER of an ensemble launch (k_march_wet_ens): the same rules, told the member's SHARE of the chip -- capacity /
// n_members wave slots, at least one wave per strip -- so that the members of a large ensemble march tall segments (few warm-up rows)
// while their neighbours fill the other wave slots, and a lone member (n_members == 1) gets what wet_launch_shape gives it.
// `capacity` <= 0: the device's (wet_capacity).
inline int wet_member_share(const Geo &g, int n_members, int capacity)
{
  const int cap = capacity > 0 ? capacity : wet_capacity();
  if (const char *e = wx_tune_env("WX_ENS_SHARE")) n_members = atoi(e) > 0 ? atoi(e) : n_members; // (tools/ensemble_bench.py --share: the segment-height sweep)
  if (n_members <= 1) return cap;
  const int strips = (g.X + WOUT - 1) / WOUT;
  return std::max(cap / n_members, std::min(cap, strips));
}
inline WetLaunch wet_launch_shape_member(const Geo &g, int air_from_row, int bands_mode, int n_members, int capacity = 0)
{
  return wet_launch_shape_cap(g, air_from_row, bands_mode, wet_member_share(g, n_members, capacity));
}

// the same shape with every segment cut in two (segments of fewer than 12 rows stay): for a launch of a few strips that runs NEXT TO a
// launch that fills the chip -- the edge strips of a slab beside its interior -- and should be done first: half the row steps per wave
inline WetLaunch wet_shape_halved(const WetLaunch &w)
{
  WetLaunch h = w;
  int n = 0;
  for (int sg = 0; sg < w.segs.n_seg; sg++) n += w.segs.start[sg + 1] - w.segs.start[sg] >= 12 ? 2 : 1;
  if (n > WMAXSEG) return w; // (the table is full: leave the shape as it is)
  n = 0;
  for (int sg = 0; sg < w.segs.n_seg; sg++) {
    const int a = w.segs.start[sg], b = w.segs.start[sg + 1];
    h.segs.start[n++] = a;
    if (b - a >= 12) h.segs.start[n++] = a + (b - a) / 2;
  }
  h.segs.start[n] = w.segs.start[w.segs.n_seg];
  h.segs.n_seg = n;
  return h;
}

// edge_prio: the issue priority of the launch's waves (the edge group of a split iteration, edge_wave_prio; 0: none)
inline void launch_march_wet(const WetLaunch &w, float iterNum, const FullCtx *ctx, const WetIn &in, const WetOut &out, const WetFixList &fix,
                             bool opt_out, bool quiet, hipStream_t stream, int strip_lo = 0, int strip_count = -1, int strip_lo2 = 0, int strip_count2 = 0,
                             int edge_prio = 0, const VxTrack *vx = nullptr)
{
  // (strip_count2 > 0: a second strip range in the same launch -- the two edges of a slab)
  const int ns1 = strip_count < 0 ? w.n_strips : strip_count, ns = ns1 + (strip_count2 > 0 ? strip_count2 : 0);
  if (ns <= 0) return;
  // 8 XCDs x (workgroups of the largest column block) x segments; surplus workgroups / waves exit at once
  const int groups = ((w.segs.bands ? ns : (ns + 7) / 8) + WX_WET_WPB - 1) / WX_WET_WPB;
  const dim3 grid(8 * groups * w.segs.n_seg);
  static bool dbg = wx_tune_env("WX_MARCH_DEBUG") != nullptr;
  if (dbg) {
    fprintf(stderr, "[wx_wet] strips=%d segs=%d waves=%d first/last segment rows=%d/%d\n", w.n_strips, w.segs.n_seg, w.n_strips * w.segs.n_seg,
            w.segs.start[1] - w.segs.start[0], w.segs.start[w.segs.n_seg] - w.segs.start[w.segs.n_seg - 1]);
    dbg = false;
  }
  const bool has_fb = in.fb != nullptr;
  VxTrack vt = vx ? *vx : VxTrack{nullptr, nullptr, 0.0f, 0, 0};
  if (vx && vx->zone_l < vx->zone_r) { // the watched zone arrives in COLUMNS: this kernel's strips are WOUT columns wide
    vt.zone_l = (vx->zone_l + WOUT - 1) / WOUT;
    vt.zone_r = vx->zone_r / WOUT;
  }
#define WX_LAUNCH_W(O, F, Q) \
  hipLaunchKernelGGL((k_march_wet<O, F, Q>), grid, dim3(64 * WX_WET_WPB), 0, stream, ctx, iterNum, in, out, fix, ns, strip_lo, w.n_strips, w.segs, ns1, strip_lo2, edge_prio, vt)
#define WX_LAUNCH_WQ(O, F) \
  do { if (quiet) WX_LAUNCH_W(O, F, true); else WX_LAUNCH_W(O, F, false); } while (0)
  if (opt_out) {
    if (has_fb) WX_LAUNCH_WQ(true, true); else WX_LAUNCH_WQ(true, false);
  } else {
    if (has_fb) WX_LAUNCH_WQ(false, true); else WX_LAUNCH_WQ(false, false);
  }
#undef WX_LAUNCH_WQ
#undef WX_LAUNCH_W
}

// the fix pass of a launch group: every list entry recomputed exactly, spread over the chip (exits at once while the list is empty)
inline void launch_wet_fix(float iterNum, const FullCtx *ctx, const WetIn &in, const WetOut &out, const WetFixList &fix, int *overflow, bool opt_out,
                           hipStream_t stream, int wgs = 0)
{
  // the whole chip (512 workgroups = one wavefront per list entry up to 2048 entries) while the last list the host has heard of held
  // entries, a corner of it while the lists are empty; any grid is correct (grid-stride loop)
  const int last = fix.hint ? *(volatile const int *)fix.hint_host : -1; // (-1: no host word -- the whole chip every time)
  // four entries per workgroup with room for four times the last list (its length varies from iteration to iteration: room for twice
  // cost the particle flow 6 us, 21 -> 27), 32 .. 512 workgroups (wgs: the edge group of a slab -- a few strips -- asks for 64); the
  // list is walked grid-stride, so any size is correct
  const int want = last < 0 ? 512 : (last > 0 ? std::min(512, std::max(32, last)) : 32);
  const dim3 grid(wgs > 0 ? wgs : want), block(256);
  if (opt_out)
    hipLaunchKernelGGL((k_wet_fix<true>), grid, block, 0, stream, ctx, iterNum, in, out, fix.count, fix.cells, fix.cap, overflow, fix.hint);
  else
    hipLaunchKernelGGL((k_wet_fix<false>), grid, block, 0, stream, ctx, iterNum, in, out, fix.count, fix.cells, fix.cap, overflow, fix.hint);
}

// An ensemble launch (wx_ensemble_step): `table` holds n_members slots (device memory, written in front of the launch on the same stream),
// groups_x = the largest ens_member_groups among the members' shapes. All members run the instantiation <opt_out, has_fb, quiet>.
inline int ens_member_groups(const WetLaunch &w)
{
  const int groups = ((w.segs.bands ? w.n_strips : (w.n_strips + 7) / 8) + WX_WET_WPB - 1) / WX_WET_WPB;
  return 8 * groups * w.segs.n_seg;
}
inline void launch_march_wet_ens(const WetEnsSlot *table, int n_members, int groups_x, bool opt_out, bool has_fb, bool quiet, hipStream_t stream)
{
  const dim3 grid(groups_x, n_members), block(64 * WX_WET_WPB);
#define WX_LAUNCH_E(O, F, Q) hipLaunchKernelGGL((k_march_wet_ens<O, F, Q>), grid, block, 0, stream, table)
#define WX_LAUNCH_EQ(O, F) \
  do { if (quiet) WX_LAUNCH_E(O, F, true); else WX_LAUNCH_E(O, F, false); } while (0)
  if (opt_out) {
    if (has_fb) WX_LAUNCH_EQ(true, true); else WX_LAUNCH_EQ(true, false);
  } else {
    if (has_fb) WX_LAUNCH_EQ(false, true); else WX_LAUNCH_EQ(false, false);
  }
#undef WX_LAUNCH_EQ
#undef WX_LAUNCH_E
}
// wgs_per_member: sized by the caller from the largest stale hint word of the members (launch_wet_fix's rule); any size is correct
inline void launch_wet_fix_ens(const WetEnsSlot *table, int n_members, int wgs_per_member, bool opt_out, hipStream_t stream)
{
  const dim3 grid(wgs_per_member, n_members), block(256);
  if (opt_out) hipLaunchKernelGGL((k_wet_fix_ens<true>), grid, block, 0, stream, table);
  else hipLaunchKernelGGL((k_wet_fix_ens<false>), grid, block, 0, stream, table);
}

// lowest row above which every cell is free air in the sense of air_cell(): 1 + the highest row holding a wall cell, a cell next
// to one, or a cell less than 9 rows above one (block-wise maximum into *out, which the caller zeroes)
__global__ void k_air_from_row(int X, int Y, const char4 *__restrict__ wall, int *__restrict__ out)
{
  int best = 0;
  const size_t n = (size_t)X * Y;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const char4 w = wall[i];
    if (w.y <= 1 || w.z <= 9) {
      const int row = (int)(i / X) + 1;
      // (the top row always sees the wall row 0 through the y-wrap: it is not terrain, and one row does not matter to the cost model)
      if (row < Y) best = row > best ? row : best;
    }
  }
  for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o));
  if ((threadIdx.x & 63) == 0 && best > 0) atomicMax(out, best);
}

} // namespace wx
