// wx_ens_frame.h -- what every member-axis call of an ensemble (wx_ensemble_statistics, _perturb, _quantiles, _scores, _assimilate,
// _prior_save, _inflate, _covariance, _neighbourhood) shares: the member table and its device-side accessors, the chunk cursor and the
// member walk of the kernels, the ensemble's staging buffers, and the host frame of a call. Included at the end of wxsim.hip behind wx_ensemble.h and in front of the wx_ens_*.h call headers; the
// definition headers (wx_ens_*_cell.h) and the host-only test drivers do not include it: it needs HIP.
//
// A call is five parts: its own argument checks, in its own order (the pieces below are used where two calls refuse with the same
// words); the frame -- ens_begin: the broken-ensemble guard and the staging buffers, then ens_table_*: the selected members' {field,
// wall, index} entries as they are NOW (a step rotates the planes) and their stream-ordered copy to the device --; its argument block;
// its launches (ens_launch) and copies, each skipped once an earlier step failed; and ens_finish, behind which the caller copies out
// of the pinned buffer what it wants. Everything is enqueued on the ensemble's stream, behind everything pending.
//
// What the frame guarantees: the pinned table and the pinned output are rewritten only by a call, and every call ends in ens_finish,
// which leaves the stream idle -- a failed enqueue drains the stream before the call returns WX_E_DEVICE, so that a copy still in
// flight never reads a table the next call rewrites; otherwise wx_ensemble_sync blocks, and is the one place where every member's
// pending report is looked at and consumed. A launch's status is taken once: the callable's own where it returns one (hipGetLastError
// clears what it reports: asking twice would swallow the error), hipGetLastError otherwise.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "../../include/wxsim.h"

namespace wxe {

// a selected member, as the kernels see it
struct Member {
  const float4 *field;
  const char4 *wall;
  int index, pad;
};

#if defined(__HIPCC__)
// One member's texel. The table is read through the constant address space (as k_march_wet_ens reads its slots: scalar loads, the entry
// index is wave-uniform), and the pointers it holds are turned into global-address-space pointers by an integer round trip -- a pointer
// loaded from memory is otherwise a generic one, whose loads may become flat loads that count on both wait counters. The table holds
// hipMalloc'ed addresses only, so the cast states a fact. (The record under profiles/: global_load only, the table by s_load.)
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) Member *CTab;
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ CTab const_table(const Member *tab) { return (CTab)(unsigned long long)tab; }
__device__ __forceinline__ f32x4 ld_field(CTab m, size_t off) { return ((const __attribute__((address_space(1))) f32x4 *)(unsigned long long)m->field)[off]; }
// (the whole 4-byte wall texel; only "is channel 1 zero" is looked at)
__device__ __forceinline__ int ld_wall_dist(CTab m, size_t off) { return (((const __attribute__((address_space(1))) unsigned *)(unsigned long long)m->wall)[off] >> 8) & 0xFF; }
// between a group's loads and its consumers: the instruction scheduler moves nothing across (it is otherwise free to interleave the
// loads with the consumers to save registers -- one round trip per member again)
#define WX_ENS_LOADS_ISSUED() __builtin_amdgcn_sched_barrier(0)
#else // host pass of the single-source compile: same meaning, never executed
typedef const Member *CTab;
struct f32x4 {
  float x, y, z, w;
};
__device__ __forceinline__ CTab const_table(const Member *tab) { return tab; }
__device__ __forceinline__ f32x4 ld_field(CTab m, size_t off) { return f32x4{m->field[off].x, m->field[off].y, m->field[off].z, m->field[off].w}; }
__device__ __forceinline__ int ld_wall_dist(CTab m, size_t off) { return m->wall[off].y; }
#define WX_ENS_LOADS_ISSUED() ((void)0)
#endif

// ---- the chunk cursor: where a lane stands ----
// The items of a rectangle are its chunks of 64 consecutive x of one row, row-major (ens_chunks: below 2^31, 16 Ki chunks per row x
// 64 Ki rows); lane l of whoever takes chunk ch -- a wave, or the four waves of a workgroup alike -- stands on cell (x, y) of the
// rectangle. A lane past the ragged edge (x >= w) is not valid: its offsets are numbers, not places to touch.
struct Chunk {
  unsigned x, y; // the cell in the rectangle
  int gx, gy;    // the cell in the grid
  bool valid;
};
__device__ __forceinline__ unsigned chunks_per_row(int w) { return ((unsigned)w + 63u) / 64u; }
__device__ __forceinline__ Chunk chunk_at(unsigned ch, unsigned lane, int x0, int y0, int w)
{
  const unsigned cpr = chunks_per_row(w);
  Chunk c;
  c.y = ch / cpr, c.x = (ch - c.y * cpr) * 64u + lane;
  c.valid = c.x < (unsigned)w;
  c.gx = x0 + (int)c.x, c.gy = y0 + (int)c.y;
  return c;
}
// item `it` of n_members x chunks (member, chunk) pairs, member-major (a 64-bit count): the member into k
__device__ __forceinline__ Chunk member_chunk_at(unsigned long long it, unsigned lane, int x0, int y0, int w, int h, unsigned &k)
{
  const unsigned per_member = chunks_per_row(w) * (unsigned)h;
  k = (unsigned)(it / per_member);
  return chunk_at((unsigned)(it - (unsigned long long)k * per_member), lane, x0, y0, w);
}
// The two offsets of a cell: its texel in a member's array of X cells per row, and in a w * h plane of the rectangle. Functions, not
// fields of the cursor: they are computed where they are asked for -- behind the valid test.
__device__ __forceinline__ size_t texel_at(int X, int gx, int gy) { return (size_t)gy * (size_t)X + (size_t)gx; }
__device__ __forceinline__ size_t plane_at(int w, unsigned x, unsigned y) { return (size_t)y * (size_t)w + x; }
// a wave of a grid of `waves`-wave workgroups that grid-strides over items: its lane, its first item, its stride
struct WaveOfGrid {
  unsigned lane, wave, n_waves;
};
__device__ __forceinline__ WaveOfGrid wave_of_grid(unsigned waves) { return WaveOfGrid{threadIdx.x & 63u, blockIdx.x * waves + (threadIdx.x >> 6), gridDim.x * waves}; }

// ---- the member walk ----
// Per cell a walk over the members is serial BY DEFINITION (a dependent double add chain per channel, member 0 first), so what a
// kernel can do about latency is to have the loads of UNROLL members in flight before the first is consumed: `load(k)` returns what
// member k's step needs from memory, a group's loads are issued, then `take(acc, k, loaded)` consumes them in member order (the
// compiler's counted s_waitcnt vmcnt(N) in front of each consumer), and the remainder (n % UNROLL members) goes one by one through the
// same two. The walk OWNS what it accumulates -- acc goes in and comes back by value -- and that is not a matter of taste: with the
// accumulator behind a reference the optimiser unrolls the group before it has turned the consumer's short-circuit tests into selects,
// and the last member of k_ens_stat's group keeps four branches ("One member walk"). `take` is meant to stay
// free of branches: a group is one basic block (wx_ens_stat.h, over cell_add). A walk that only writes passes Nothing.
// k_ens_inflate and k_ens_cov keep their walks written out: through this template they need more registers (same place).
struct Nothing {};
template <int UNROLL, class Acc, class Load, class Take>
__device__ __forceinline__ Acc member_walk(int n, Acc acc, const Load &load, const Take &take)
{
  int k = 0;
  for (; k + UNROLL <= n; k += UNROLL) {
    decltype(load(0)) m[UNROLL];
#pragma unroll
    for (int i = 0; i < UNROLL; i++) m[i] = load(k + i);
    WX_ENS_LOADS_ISSUED();
#pragma unroll
    for (int i = 0; i < UNROLL; i++) take(acc, k + i, m[i]);
  }
  for (; k < n; k++) take(acc, k, load(k));
  return acc;
}
// what most walks load: a member's texel, and its wall texel's channel 1 with it
struct TexelWall {
  f32x4 v;
  int wd;
};
__device__ __forceinline__ TexelWall ld_field_wall(CTab m, size_t off) { return TexelWall{ld_field(m, off), ld_wall_dist(m, off)}; }
#endif // __HIPCC__

} // namespace wxe

// ---- accessors that one call's kernels define and another's borrow, each in the namespace it was written in ----
#if defined(__HIPCC__)
namespace wxp {
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ void st_field(wxe::CTab m, size_t off, wxe::f32x4 v) { ((__attribute__((address_space(1))) wxe::f32x4 *)(unsigned long long)m->field)[off] = v; }
#else // host pass of the single-source compile: same meaning, never executed
__device__ __forceinline__ void st_field(wxe::CTab m, size_t off, wxe::f32x4 v) { const_cast<float4 *>(m->field)[off] = make_float4(v.x, v.y, v.z, v.w); }
#endif
} // namespace wxp

namespace wxq {
#if defined(__HIP_DEVICE_COMPILE__)
// channel c of a member's texel (the streaming kernel and the rank member)
__device__ __forceinline__ float ld_chan(wxe::CTab m, size_t off, unsigned c) { return ((const __attribute__((address_space(1))) float *)(unsigned long long)m->field)[4 * off + c]; }
#else // host pass of the single-source compile: same meaning, never executed
__device__ __forceinline__ float ld_chan(wxe::CTab m, size_t off, unsigned c) { return ((const float *)m->field)[4 * off + c]; }
#endif
} // namespace wxq

namespace wxi {
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ wxe::f32x4 ld_prior(const float4 *p, size_t i) { return ((const __attribute__((address_space(1))) wxe::f32x4 *)(unsigned long long)p)[i]; }
__device__ __forceinline__ void st_texel(float4 *p, size_t i, wxe::f32x4 v) { ((__attribute__((address_space(1))) wxe::f32x4 *)(unsigned long long)p)[i] = v; }
#else // host pass of the single-source compile: same meaning, never executed
__device__ __forceinline__ wxe::f32x4 ld_prior(const float4 *p, size_t i) { return wxe::f32x4{p[i].x, p[i].y, p[i].z, p[i].w}; }
__device__ __forceinline__ void st_texel(float4 *p, size_t i, wxe::f32x4 v) { p[i] = make_float4(v.x, v.y, v.z, v.w); }
#endif
} // namespace wxi
#endif // __HIPCC__

// ---- the ensemble's staging buffers: the device table of the selected members, the output of one call, and their pinned copies ----
struct EnsStage {
  wxe::Member *tab_host = nullptr, *tab_dev = nullptr; // pinned staging + device table, tab_cap entries
  int tab_cap = 0;
  char *out_dev = nullptr, *out_host = nullptr;         // what one call wants back (and its device-side tables), out_cap bytes
  size_t out_cap = 0;
  char *aux_dev = nullptr;                              // device-only scratch of one call (wx_ensemble_gram's planes of centres): no pinned copy
  size_t aux_cap = 0;
};

static void ens_stage_release(wx_ensemble *e)
{
  EnsStage *st = e->stage;
  if (!st) return;
  if (st->tab_host) hipHostFree(st->tab_host);
  hipFree(st->tab_dev);
  if (st->out_host) hipHostFree(st->out_host);
  hipFree(st->out_dev);
  hipFree(st->aux_dev);
  delete st;
  e->stage = nullptr;
}

// only grows; the table and the output grow independently. call: the entry point's name, for the message
static int ens_stage_reserve(wx_ensemble *e, const char *call, int entries, size_t out_bytes)
{
  if (!e->stage) e->stage = new EnsStage();
  EnsStage *st = e->stage;
  if (entries > st->tab_cap) {
    if (st->tab_host) hipHostFree(st->tab_host);
    hipFree(st->tab_dev);
    st->tab_host = st->tab_dev = nullptr;
    st->tab_cap = 0;
    const size_t bytes = (size_t)entries * sizeof(wxe::Member);
    if (hipHostMalloc((void **)&st->tab_host, bytes, hipHostMallocDefault) != hipSuccess || hipMalloc((void **)&st->tab_dev, bytes) != hipSuccess) {
      (void)hipGetLastError();
      return efail(e, WX_E_NOMEM, "%s: %zu bytes for the table of %d members", call, bytes, entries);
    }
    st->tab_cap = entries;
  }
  if (out_bytes > st->out_cap) {
    if (st->out_host) hipHostFree(st->out_host);
    hipFree(st->out_dev);
    st->out_host = st->out_dev = nullptr;
    st->out_cap = 0;
    if (hipHostMalloc((void **)&st->out_host, out_bytes, hipHostMallocDefault) != hipSuccess || hipMalloc((void **)&st->out_dev, out_bytes) != hipSuccess) {
      (void)hipGetLastError();
      return efail(e, WX_E_NOMEM, "%s: %zu bytes (device and pinned host) for the planes of the rectangle", call, out_bytes);
    }
    st->out_cap = out_bytes;
  }
  return WX_OK;
}

// device-only scratch, behind ens_begin; only grows
static int ens_aux_reserve(wx_ensemble *e, const char *call, size_t bytes)
{
  EnsStage *st = e->stage;
  if (bytes <= st->aux_cap) return WX_OK;
  hipFree(st->aux_dev);
  st->aux_dev = nullptr, st->aux_cap = 0;
  if (hipMalloc((void **)&st->aux_dev, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return efail(e, WX_E_NOMEM, "%s: %zu bytes of device scratch", call, bytes);
  }
  st->aux_cap = bytes;
  return WX_OK;
}

// ---- argument checks that several calls word alike (each call keeps its own ORDER of checks) ----
static std::vector<int> ens_select(const wx_ensemble *e, const uint8_t *member_mask)
{
  std::vector<int> sel;
  for (int i = 0; i < (int)e->member.size(); i++)
    if (!member_mask || member_mask[i]) sel.push_back(i);
  return sel;
}

static int ens_require_uploaded(wx_ensemble *e, const char *call, const std::vector<int> &sel)
{
  for (int i : sel)
    if (!e->member[i]->uploaded) return efail(e, WX_E_STATE, "member %d: %s before wx_upload", i, call);
  return WX_OK;
}

static int ens_check_state_field(wx_ensemble *e, const char *call, int field)
{
  if (field != WX_FIELD_BASE_CUR && field != WX_FIELD_WATER_CUR)
    return efail(e, WX_E_INVALID, "%s: field %d: WX_FIELD_BASE_CUR or WX_FIELD_WATER_CUR (the fields that are stored whole and interleaved)", call, field);
  return WX_OK;
}

static int ens_check_rect(wx_ensemble *e, const char *call, int x, int y, int w, int h)
{
  if (w <= 0 || h <= 0 || x < 0 || y < 0 || (long long)x + w > e->X || (long long)y + h > e->Y)
    return efail(e, WX_E_RANGE, "%s: rect (%d,%d %dx%d) outside %dx%d (no wrap)", call, x, y, w, h, e->X, e->Y);
  return WX_OK;
}

// ---- one call in flight ----
struct EnsCall {
  wx_ensemble *e;
  const char *name;          // the entry point, for its messages
  const char *kernel;        // the kernel launched last (until the first launch: the call's first kernel); the failure message names it
  DeviceScope dev_scope;
  EnsStage *st = nullptr;
  hipError_t he = hipSuccess; // the first enqueue that failed; every later step is skipped
  EnsCall(wx_ensemble *e_, const char *name_, int first_kernel) : e(e_), name(name_), kernel(kKernelNames[first_kernel]), dev_scope(e_->member[0]) {}
};

// the guard and the staging buffers: `entries` table entries, out_bytes of output
static int ens_begin(EnsCall &c, int entries, size_t out_bytes)
{
  if (c.e->broken) return WX_E_STATE; // (the message of the failed step is kept)
  if (int rc = ens_stage_reserve(c.e, c.name, entries, out_bytes)) return rc;
  c.st = c.e->stage;
  return WX_OK;
}

// the member's pointers as they are NOW (a step rotates the planes): base_0 / water_1 and wall_0, what wx_diag reads
static wxe::Member ens_member_entry(const wx_sim *m, int field, int index)
{
  return wxe::Member{field == WX_FIELD_BASE_CUR ? m->base[0] : m->water[1], m->wall[0], index, 0};
}

static void ens_table_upload(EnsCall &c, size_t entries)
{
  c.he = hipMemcpyAsync(c.st->tab_dev, c.st->tab_host, entries * sizeof(wxe::Member), hipMemcpyHostToDevice, c.e->stream);
}

// one field: the selected members in order, and `extra` (the truth, the ranked member) behind them where there is one
static void ens_table_field(EnsCall &c, const std::vector<int> &sel, int field, const wx_sim *extra = nullptr, int extra_index = -1)
{
  size_t n = 0;
  for (int i : sel) c.st->tab_host[n++] = ens_member_entry(c.e->member[i], field, i);
  if (extra) c.st->tab_host[n++] = ens_member_entry(extra, field, extra_index);
  ens_table_upload(c, n);
}

// both state fields: the selected members' base entries, then their water entries
static void ens_table_base_water(EnsCall &c, const std::vector<int> &sel)
{
  const size_t n = sel.size();
  for (size_t k = 0; k < n; k++) {
    const wx_sim *m = c.e->member[sel[k]];
    c.st->tab_host[k] = ens_member_entry(m, WX_FIELD_BASE_CUR, sel[k]);
    c.st->tab_host[n + k] = ens_member_entry(m, WX_FIELD_WATER_CUR, sel[k]);
  }
  ens_table_upload(c, 2 * n);
}

// the launch grids, from the kernel's own WAVES / MAX_WGS: one wave per item, or one workgroup per item; and the items of a
// rectangle: its chunks of 64 consecutive x of one row (below 2^31: 16 Ki chunks per row x 64 Ki rows)
static unsigned ens_chunks(int w, int h) { return (unsigned)((w + 63) / 64) * (unsigned)h; }
static unsigned ens_wgs_wave_per_item(unsigned long long items, unsigned waves, unsigned max_wgs) { return (unsigned)std::min<unsigned long long>((items + waves - 1) / waves, max_wgs); }
static unsigned ens_wgs_wg_per_item(unsigned items, unsigned max_wgs) { return std::min(items, max_wgs); }

// one kernel (or one switch over a kernel's instantiations) under its profile scope -- wx_profile on member 0 sees the launch, whoever
// is selected. A callable that returns hipError_t has asked for the launch status itself
template <class Launch>
static void ens_launch(EnsCall &c, int kernel, Launch &&launch)
{
  if (c.he != hipSuccess) return;
  c.kernel = kKernelNames[kernel];
  constexpr bool own_status = std::is_same<decltype(launch()), hipError_t>::value;
  {
    ProfScope ps(c.e->member[0], kernel);
    if constexpr (own_status) c.he = launch();
    else launch();
  }
  if constexpr (!own_status) c.he = hipGetLastError();
}

// The end of every call; returns wx_ensemble_sync's code, and the caller decides what it copies out of the pinned buffer.
static int ens_finish(EnsCall &c)
{
  if (c.he != hipSuccess) {
    (void)hipStreamSynchronize(c.e->stream); // (the pinned table is not rewritten while a copy may still read it)
    return efail(c.e, WX_E_DEVICE, "%s (%s): %s", c.name, c.kernel, hipGetErrorString(c.he));
  }
  // blocking like wx_ensemble_sync, and like it a place where every member's pending report is looked at and consumed
  return wx_ensemble_sync(c.e);
}
