// wx_ens_quant.h -- order statistics over the MEMBER axis of an ensemble (include/wxsim.h: wx_ens_quant, wx_ensemble_quantiles,
// wx_ens_quant_cells): per cell and channel of a rectangle up to WX_ENS_QUANT_MAX quantiles of the members' values, the number of values
// that entered, the number of members in which the cell is a wall cell, and the rank of one unselected member's value among the
// entered ones. Included at the end of wxsim.hip behind wx_ens_perturb.h (the entry points are declared extern "C" by include/wxsim.h).
//
// THE per-cell function is in wx_ens_quant_cell.h (wxq::cell_key, position_of, quantile_of, Tally), __host__ __device__: the kernels
// and the host entry point run the same program text on the same ascending keys. Where wx_ens_stat.h is member-sequential by
// definition, nothing here depends on the order of the members, so the members are spread over the workgroup.
//
// k_ens_quant_staged<P> (n_sel <= STAGED_MEMBERS, padded to a power of two P, a template parameter). One workgroup of 256 threads per
// chunk of 64 consecutive x of one row (the chunk of k_ens_stat), workgroups grid-stride over the chunks; lane = cell, wave c = channel c.
//   1. Staging. Wave w loads members w, w + 4, ... -- a member's float4 texel (16 B per lane, 1 KiB per wave, contiguous) and its
//      wall texel, all of the wave's P / 4 members in flight at once (at most 8: 32 per workgroup), through the device table of {field,
//      wall, index} (wx_ens_frame.h: constant address space, scalar loads) -- and writes the four keys to dynamic LDS as
//      [member][channel][lane]: 1 KiB per member. Members past the selection and lanes beyond the rectangle's right edge get KEY_PAD.
//   2. __syncthreads(). From here on wave c owns channel c: thread (c, lane) reads and writes ONLY the addresses [i][c][lane], its own
//      column (bank = lane: conflict-free), so nothing below needs a barrier until the results are exchanged. The column goes into P
//      registers and a bitonic network over the member index puts it in ascending order: P/2 * log2 P (log2 P + 1)/2
//      compare-exchanges (672 at P = 64), each a v_min_u32 and a v_max_u32 on constant register indices, the same for every lane.
//      (The network was first run in LDS, two reads and two writes per compare-exchange: 8000 LDS cycles per wave at P = 64 on an
//      LDS that four waves share -- 48 us against 18 us at 100 x 100 x 64, profiles/ensemble_quantiles_cost.txt.)
//   3. The counts from the registers (n, n_wall -- the number of KEY_WALL --, n_below, n_equal); the ascending column goes back to LDS
//      and v(k), v(k1) are read by per-lane index for each quantile: the cost does not depend on n_q.
//   4. The results go through the column's first rows ([plane][channel][lane]), __syncthreads(), and wave w stores planes
//      w, w + 4, ... with one 16-byte store per lane (n_wall: 4-byte); only the wanted planes. __syncthreads() before the next chunk
//      is staged.
//   LDS: max(P, RESULT_ROWS) KiB per workgroup, at most 64 KiB of the CU's 160 KiB: two workgroups (8 waves) per CU at P = 64 (116
//   VGPRs: registers would allow four), four at P = 32, up to the 32-wave limit (eight workgroups) for P <= 16. 128 KiB would double
//   STAGED_MEMBERS at one workgroup per CU -- and 128 keys per thread in registers; 64 KiB keeps two chunks per CU in flight, so one
//   sorts while the other loads.
//   BARRIERS: the chunk loop's trip count depends on blockIdx and gridDim only, there is no `continue` or `return` inside it, and lanes
//   beyond the right edge load and store nothing but walk through every barrier.
//
// k_ens_quant_stream (more members, up to 65535). No LDS, no barrier: wave = (chunk, channel), lane = cell; the wave reads channel c
// of every member from global memory (4 of every 16 bytes of a line). Pass 0 counts (n, n_wall, rank), then a bitwise radix select
// from the top bit down finds the keys of all 2 n_q wanted positions at once: 32 more passes over the members. 4-byte stores (the
// four channels of a texel are in four waves). Slow and rare; correct.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/wxsim.h"
#include "wx_ens_frame.h"
#include "wx_ens_quant_cell.h"

namespace wxq {

enum { WG = 256, WAVES = WG / 64, MAX_WGS = 16384, STAGED_MEMBERS = 64 };
// rows of the result image: the quantiles, then count, n_below, n_equal, n_wall
enum { ROW_COUNT = WX_ENS_QUANT_MAX, ROW_BELOW, ROW_EQUAL, ROW_WALL, RESULT_ROWS = 16 };
static_assert(ROW_WALL < RESULT_ROWS && STAGED_MEMBERS == 64, "the LDS image; the launch switch of wx_ensemble_quantiles");

struct Args {
  int X;             // cells per row of the members' arrays
  int x0, y0, w, h;  // the rectangle
  int n_sel;         // selected members: tab[0 .. n_sel); tab[n_sel] is the rank member if has_rank
  int P;             // staged path: n_sel padded to a power of two; rows = max(P, RESULT_ROWS)
  int has_rank;
  int n_q, interp;
  float p[WX_ENS_QUANT_MAX];
  const wxe::Member *tab;
  // the wanted planes (w * h texels each, rows bottom-up; q: n_q of them back to back), nullptr: not wanted
  float4 *q;
  int4 *count, *below, *equal;
  int *n_wall;
};

#if defined(__HIPCC__)
// What k_ens_quant_staged<P> and k_ens_score<P> (wx_ens_score.h) share: the staging of one chunk's keys into the LDS image and the
// register sort of a thread's column. P: the selection padded to a power of two, a template parameter so that a column's keys live in
// registers with constant indices.
template <int P>
struct Staged {
  static constexpr int UN = P >= 32 ? 8 : (P >= 4 ? P / 4 : 1); // members a wave has in flight: all of its P / 4, at most 8 (32 per workgroup)
  static_assert((P & (P - 1)) == 0 && P <= STAGED_MEMBERS, "the LDS image");
  // 1. staging: wave wv takes members wv, wv + 4, ..., UN of them per batch. A member index past the selection is clamped for the
  // load (the last member again, from the cache) and its keys are KEY_PAD: the batch stays one block of loads without a branch each
  static __device__ __forceinline__ void stage(unsigned *lds, wxe::CTab tab, unsigned n_sel, size_t off, bool valid, unsigned lane, unsigned wv)
  {
    for (unsigned k = wv; k < (unsigned)P; k += 4u * UN) {
      unsigned key[UN][4];
#pragma unroll
      for (int j = 0; j < UN; j++) key[j][0] = key[j][1] = key[j][2] = key[j][3] = KEY_PAD;
      if (valid) {
        wxe::f32x4 v[UN];
        int wd[UN];
#pragma unroll
        for (int j = 0; j < UN; j++) {
          const unsigned m = k + 4u * j < n_sel ? k + 4u * j : n_sel - 1u;
          v[j] = wxe::ld_field(tab + m, off), wd[j] = wxe::ld_wall_dist(tab + m, off);
        }
#pragma unroll
        for (int j = 0; j < UN; j++)
          if (k + 4u * j < n_sel) // (uniform)
            key[j][0] = cell_key(v[j].x, wd[j]), key[j][1] = cell_key(v[j].y, wd[j]), key[j][2] = cell_key(v[j].z, wd[j]), key[j][3] = cell_key(v[j].w, wd[j]);
      }
#pragma unroll
      for (int j = 0; j < UN; j++)
#pragma unroll
        for (int c = 0; c < 4; c++) lds[((k + 4u * j) * 4u + c) * 64u + lane] = key[j][c];
    }
  }
  // 2. the thread's column (row i at col[i * 256]) into registers, a bitonic network over the member index (every index a constant)
  static __device__ __forceinline__ void sorted_column(unsigned (&key)[P], const unsigned *col)
  {
#pragma unroll
    for (int i = 0; i < P; i++) key[i] = col[i * 256];
#pragma unroll
    for (int kk = 2; kk <= P; kk <<= 1)
#pragma unroll
      for (int j = kk >> 1; j > 0; j >>= 1)
#pragma unroll
        for (int i = 0; i < P; i++)
          if ((i ^ j) > i) {
            const unsigned lo = key[i] < key[i ^ j] ? key[i] : key[i ^ j], hi = key[i] < key[i ^ j] ? key[i ^ j] : key[i];
            key[i] = (i & kk) == 0 ? lo : hi, key[i ^ j] = (i & kk) == 0 ? hi : lo;
          }
  }
};

template <int P>
__global__ __launch_bounds__(WG) void k_ens_quant_staged(const Args a)
{
  constexpr unsigned ROWS = P > RESULT_ROWS ? P : RESULT_ROWS;
  extern __shared__ unsigned wxq_lds[]; // [row][channel][lane], ROWS rows
  const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const unsigned cpr = ((unsigned)a.w + 63u) / 64u, chunks = cpr * (unsigned)a.h; // (below 2^31: 16 Ki chunks per row x 64 Ki rows)
  const wxe::CTab tab = wxe::const_table(a.tab);
  const unsigned n_sel = (unsigned)a.n_sel;
  unsigned *const col = wxq_lds + wv * 64u + lane; // this thread's column: row i at col[i * 256]
  static_assert(ROWS * 1024u <= 65536u && (P & (P - 1)) == 0, "the LDS image");
  for (unsigned ch = blockIdx.x; ch < chunks; ch += gridDim.x) { // (workgroup-uniform trip count: every barrier below is reached by all)
    const unsigned y = ch / cpr, x = (ch - y * cpr) * 64u + lane;
    const bool valid = x < (unsigned)a.w;
    const size_t off = valid ? (size_t)(a.y0 + (int)y) * (size_t)a.X + (size_t)(a.x0 + (int)x) : 0, o = valid ? (size_t)y * (size_t)a.w + x : 0;
    Staged<P>::stage(wxq_lds, tab, n_sel, off, valid, lane, wv); // 1.
    // the rank member's value of this thread's channel (in flight across the barrier)
    unsigned t_key = KEY_PAD;
    if (a.has_rank && valid) t_key = rank_key(cell_key(ld_chan(tab + n_sel, off, wv), wxe::ld_wall_dist(tab + n_sel, off)));
    __syncthreads();
    // 2. wave wv takes channel wv: its column into registers, a bitonic network over the member index (every index a constant)
    unsigned key[P];
    Staged<P>::sorted_column(key, col);
    // 3. the counts, then -- the ascending column back in LDS -- v(k), v(k1) by per-lane index
    Tally tl{0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < P; i++) tally_add(tl, key[i], t_key);
    float res[WX_ENS_QUANT_MAX];
    if (a.n_q > 0) { // (uniform)
#pragma unroll
      for (int i = 0; i < P; i++) col[i * 256] = key[i];
    }
#pragma unroll
    for (int j = 0; j < WX_ENS_QUANT_MAX; j++) {
      res[j] = __builtin_nanf("");
      if (j < a.n_q) { // (uniform)
        const Position ps = position_of(a.p[j], tl.n > 0 ? tl.n : 1);
        const float vk = value_of(col[(unsigned)ps.k * 256u]), vk1 = value_of(col[(unsigned)ps.k1 * 256u]); // (n = 0: row 0, not used)
        res[j] = tl.n > 0 ? quantile_of(a.interp, vk, vk1, ps.g) : res[j];
      }
    }
    // 4. the results into the column's first rows (every read of the keys is done), then whole texels out
#pragma unroll
    for (int j = 0; j < WX_ENS_QUANT_MAX; j++)
      if (j < a.n_q) col[j * 256] = f32_bits(res[j]);
    col[ROW_COUNT * 256] = (unsigned)tl.n;
    col[ROW_BELOW * 256] = (unsigned)rank_count(t_key, tl.below);
    col[ROW_EQUAL * 256] = (unsigned)rank_count(t_key, tl.equal);
    col[ROW_WALL * 256] = (unsigned)tl.n_wall;
    __syncthreads();
    for (unsigned r = wv; r < ROW_WALL; r += WAVES) {
      uint4 *dst = nullptr; // (uniform)
      if (r < (unsigned)a.n_q) dst = a.q ? (uint4 *)a.q + (size_t)r * ((size_t)a.w * (size_t)a.h) : nullptr;
      else if (r == ROW_COUNT) dst = (uint4 *)a.count;
      else if (r == ROW_BELOW) dst = (uint4 *)a.below;
      else if (r == ROW_EQUAL) dst = (uint4 *)a.equal;
      if (dst && valid) {
        const unsigned *src = wxq_lds + r * 256u + lane;
        dst[o] = make_uint4(src[0], src[64], src[128], src[192]);
      }
    }
    if (wv == WAVES - 1 && a.n_wall && valid) a.n_wall[o] = (int)wxq_lds[ROW_WALL * 256u + lane]; // (channel 0's count: the wall test is per cell)
    __syncthreads(); // the image is free for the next chunk
  }
}

// this lane's key of selected member m
__device__ __forceinline__ unsigned stream_key(wxe::CTab tab, unsigned m, size_t off, unsigned c) { return cell_key(ld_chan(tab + m, off, c), wxe::ld_wall_dist(tab + m, off)); }

__global__ __launch_bounds__(WG) void k_ens_quant_stream(const Args a)
{
  enum { T = 2 * WX_ENS_QUANT_MAX };
  const unsigned lane = threadIdx.x & 63u, wave = blockIdx.x * WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * WAVES;
  const unsigned cpr = ((unsigned)a.w + 63u) / 64u, chunks = cpr * (unsigned)a.h;
  const unsigned long long items = 4ull * chunks;
  const wxe::CTab tab = wxe::const_table(a.tab);
  const unsigned n_sel = (unsigned)a.n_sel, n_t = 2u * (unsigned)a.n_q;
  const size_t cells = (size_t)a.w * (size_t)a.h;
  for (unsigned long long it = wave; it < items; it += n_waves) { // (no barrier in this kernel)
    const unsigned c = (unsigned)(it & 3u), ch = (unsigned)(it >> 2);
    const unsigned y = ch / cpr, x = (ch - y * cpr) * 64u + lane;
    if (x >= (unsigned)a.w) continue;
    const size_t off = (size_t)(a.y0 + (int)y) * (size_t)a.X + (size_t)(a.x0 + (int)x), o = (size_t)y * (size_t)a.w + x;
    unsigned t_key = KEY_PAD;
    if (a.has_rank) t_key = rank_key(stream_key(tab, n_sel, off, c));
    Tally tl{0, 0, 0, 0};
#pragma unroll 4
    for (unsigned m = 0; m < n_sel; m++) tally_add(tl, stream_key(tab, m, off, c), t_key);
    if (a.q && n_t) { // (uniform)
      // rank[t]: the position still looked for among the keys that share prefix[t]'s bits above `bit`
      unsigned rank[T], prefix[T];
      double g[WX_ENS_QUANT_MAX];
#pragma unroll
      for (int j = 0; j < WX_ENS_QUANT_MAX; j++) {
        const Position ps = position_of(j < a.n_q ? a.p[j] : 0.0f, tl.n > 0 ? tl.n : 1);
        rank[2 * j] = (unsigned)ps.k, rank[2 * j + 1] = (unsigned)ps.k1, g[j] = ps.g;
        prefix[2 * j] = prefix[2 * j + 1] = 0u;
      }
      for (int bit = 31; bit >= 0; bit--) {
        unsigned zero[T]; // entered keys that agree with prefix[t] above `bit` and have a 0 there
#pragma unroll
        for (int t = 0; t < T; t++) zero[t] = 0u;
#pragma unroll 4
        for (unsigned m = 0; m < n_sel; m++) {
          const unsigned key = stream_key(tab, m, off, c);
          const bool in = key_entered(key);
#pragma unroll
          for (int t = 0; t < T; t++)
            if ((unsigned)t < n_t) zero[t] += (in && ((key ^ prefix[t]) >> bit) == 0u) ? 1u : 0u;
        }
#pragma unroll
        for (int t = 0; t < T; t++) {
          const bool one = rank[t] >= zero[t];
          rank[t] -= one ? zero[t] : 0u;
          prefix[t] |= one ? (1u << bit) : 0u;
        }
      }
#pragma unroll
      for (int j = 0; j < WX_ENS_QUANT_MAX; j++)
        if (j < a.n_q) {
          const float r = tl.n > 0 ? quantile_of(a.interp, value_of(prefix[2 * j]), value_of(prefix[2 * j + 1]), g[j]) : __builtin_nanf("");
          ((float *)a.q)[((size_t)j * cells + o) * 4 + c] = r;
        }
    }
    if (a.count) ((int *)a.count)[4 * o + c] = tl.n;
    if (a.below) ((int *)a.below)[4 * o + c] = rank_count(t_key, tl.below);
    if (a.equal) ((int *)a.equal)[4 * o + c] = rank_count(t_key, tl.equal);
    if (a.n_wall && c == 0) a.n_wall[o] = tl.n_wall;
  }
}
#endif // __HIPCC__

} // namespace wxq

int wx_ens_quant_staged_members(void) { return wxq::STAGED_MEMBERS; }

int wx_ens_quant_cells(int n_members, size_t n_cells, const float *const *field, const int8_t *const *wall, const uint8_t *member_mask, wx_ens_quant *out)
{
  return wxq::quant_cells(n_members, n_cells, field, wall, member_mask, out);
}

int wx_ensemble_quantiles(wx_ensemble *e, int field, int x, int y, int w, int h, const uint8_t *member_mask, wx_ens_quant *out)
{
  static const char *const call = "wx_ensemble_quantiles";
  if (!e || !out) return WX_E_INVALID;
  // the arguments first: nothing below this block is reached with a bad one, and nothing in it touches the device
  if (int rc = ens_check_state_field(e, call, field)) return rc;
  const char *why;
  if (int rc = wxq::check_desc(out, (int)e->member.size(), member_mask, &why)) return efail(e, rc, "wx_ensemble_quantiles: %s", why);
  if (int rc = ens_check_rect(e, call, x, y, w, h)) return rc;
  const std::vector<int> sel = ens_select(e, member_mask);
  if (int rc = ens_require_uploaded(e, call, sel)) return rc;
  const int rank = out->rank_member;
  if (rank >= 0 && !e->member[rank]->uploaded) return efail(e, WX_E_STATE, "member %d (rank_member): wx_ensemble_quantiles before wx_upload", rank);

  // the wanted planes back to back: q (n_q of them), count, n_below, n_equal, n_wall
  const size_t cells = (size_t)w * h;
  void *const host_ptr[5] = {out->n_q > 0 ? (void *)out->q : nullptr, out->count, out->n_below, out->n_equal, out->n_wall};
  const size_t bytes[5] = {cells * 16 * (size_t)out->n_q, cells * 16, cells * 16, cells * 16, cells * 4};
  size_t at[5], out_bytes = 0;
  for (int p = 0; p < 5; p++) {
    at[p] = out_bytes;
    if (host_ptr[p]) out_bytes += bytes[p];
  }
  const int n_sel = (int)sel.size();
  EnsCall c(e, call, K_ENS_QUANT);
  if (int rc = ens_begin(c, n_sel + 1, std::max<size_t>(out_bytes, 16))) return rc;
  EnsStage *st = c.st;
  // the rank member behind the selected ones (without one: an entry that is not looked at)
  const int behind = rank >= 0 ? rank : sel[0];
  ens_table_field(c, sel, field, e->member[behind], behind);

  wxq::Args a;
  memset(&a, 0, sizeof(a));
  a.X = e->X, a.x0 = x, a.y0 = y, a.w = w, a.h = h, a.n_sel = n_sel;
  a.has_rank = rank >= 0 ? 1 : 0;
  a.n_q = out->n_q, a.interp = out->interp;
  memcpy(a.p, out->p, sizeof(a.p));
  a.tab = st->tab_dev;
  auto dev_plane = [&](int p) -> void * { return host_ptr[p] ? (void *)(st->out_dev + at[p]) : nullptr; };
  a.q = (float4 *)dev_plane(0), a.count = (int4 *)dev_plane(1), a.below = (int4 *)dev_plane(2), a.equal = (int4 *)dev_plane(3), a.n_wall = (int *)dev_plane(4);
  const bool staged = n_sel <= wxq::STAGED_MEMBERS;
  a.P = 1;
  while (staged && a.P < n_sel) a.P <<= 1;

  // behind the table: kernel, planes to the pinned copy
  const dim3 grid(ens_wgs_wg_per_item(ens_chunks(w, h), wxq::MAX_WGS)), wg(wxq::WG); // (the streaming kernel: chunks x 4 waves)
  ens_launch(c, K_ENS_QUANT, [&] {
    const size_t lds = (size_t)std::max<int>(a.P, wxq::RESULT_ROWS) * 1024;
    if (!staged) hipLaunchKernelGGL(wxq::k_ens_quant_stream, grid, wg, 0, e->stream, a);
    else
      switch (a.P) {
      case 1: hipLaunchKernelGGL(wxq::k_ens_quant_staged<1>, grid, wg, lds, e->stream, a); break;
      case 2: hipLaunchKernelGGL(wxq::k_ens_quant_staged<2>, grid, wg, lds, e->stream, a); break;
      case 4: hipLaunchKernelGGL(wxq::k_ens_quant_staged<4>, grid, wg, lds, e->stream, a); break;
      case 8: hipLaunchKernelGGL(wxq::k_ens_quant_staged<8>, grid, wg, lds, e->stream, a); break;
      case 16: hipLaunchKernelGGL(wxq::k_ens_quant_staged<16>, grid, wg, lds, e->stream, a); break;
      case 32: hipLaunchKernelGGL(wxq::k_ens_quant_staged<32>, grid, wg, lds, e->stream, a); break;
      default: hipLaunchKernelGGL(wxq::k_ens_quant_staged<wxq::STAGED_MEMBERS>, grid, wg, lds, e->stream, a); break;
      }
  });
  if (c.he == hipSuccess && out_bytes) c.he = hipMemcpyAsync(st->out_host, st->out_dev, out_bytes, hipMemcpyDeviceToHost, e->stream);
  if (int rc = ens_finish(c)) return rc;
  for (int p = 0; p < 5; p++)
    if (host_ptr[p]) memcpy(host_ptr[p], st->out_host + at[p], bytes[p]);
  return WX_OK;
}
