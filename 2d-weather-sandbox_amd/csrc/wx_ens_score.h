// wx_ens_score.h -- the selected members of an ensemble scored against a truth handle (include/wxsim.h: wx_ens_score, wx_ensemble_scores,
// wx_ens_score_cells): per channel the exact domain sums of error, absolute error, squared error, ensemble variance and CRPS, two rank
// histograms and the counts, plus three optional maps. Included at the end of wxsim.hip behind wx_ens_quant.h (the entry points are
// declared extern "C" by include/wxsim.h).
//
// THE per-cell function is in wx_ens_score_cell.h (wxs::sum_step, dev_step, five_of, reason_of), __host__ __device__: the kernel and the
// host entry point run the same program text on the same ascending keys.
//
// k_ens_score<P> (n_sel <= 64, padded to a power of two P). The launch shape, the staging and the register sort are those of
// k_ens_quant_staged<P> (wxq::Staged<P>: one workgroup of 256 threads per chunk of 64 consecutive x of one row, lane = cell, wave c =
// channel c after the barrier); the truth is the table entry behind the selection, as the quantile kernel's rank member is.
//   1. Staging, __syncthreads(), the column into P registers, the bitonic network.
//   2. The walk. Thread (c, lane) counts n, n_below, n_equal from its registers and walks them twice with constant indices, predicated
//      on i < n: S, then Q, A, G around the mean -- about 9 double operations per value --, then the five floats and the reason.
//   3. The five terms become wx_diag's (bin, addend) and go into per-wave bin registers (wxd::wave_add: while the 64 cells of the wave
//      share a bin nothing crosses lanes) that live ACROSS the chunk loop; the counters are ballot counts in wave-uniform registers; the
//      two histogram increments are LDS integer atomics of the scored lanes.
//   4. If a map is wanted (a kernel argument: the same for every thread of the grid) the maps go through the column's first rows,
//      __syncthreads(), and waves 0 .. 2 store one plane each as whole texels. __syncthreads() before the next chunk is staged.
//   5. Behind the loop: the bin registers are flushed into the workgroup's LDS bins, the counters added, __syncthreads(), and ONE push of
//      the workgroup's table into its shard (blockIdx % 8) of the device table: integer atomics, so any launch shape gives the same
//      table. The host copies the 8 shards back once, adds them and rounds each sum once (wxd::bins_to_double).
//   LDS: max(P, 4) KiB of image + 4720 bytes of tables, STATIC (P is a template parameter, so the runtime is asked for nothing):
//   70256 bytes at P = 64 -- above 64 KiB, which gfx950 allows a workgroup --, two workgroups per CU as for the quantile kernel.
//   BARRIERS: the chunk loop's trip count depends on blockIdx and gridDim only, there is no `continue` or `return` inside it, the one
//   conditional barrier hangs on a kernel argument, lanes beyond
//   the right edge load and store nothing, contribute nothing and walk through every barrier. Nothing waits on the device: no spin, no
//   grid barrier, no flag.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/wxsim.h"
#include "wx_diag.h"
#include "wx_ens_quant.h"
#include "wx_ens_score_cell.h"

namespace wxs {

typedef unsigned long long u64;
// MAX_WGS: what the chip holds at once (256 CUs x up to 8 workgroups). A workgroup pays for its tables once -- 4.7 KiB zeroed, up to 860
// words pushed with atomics --, so the chunks are shared among resident workgroups instead of one each (at 2500 x 300 x 8, 12000
// chunks, one workgroup per chunk cost 88 us against the quantile kernel's 45; profiles/ensemble_scores_cost.txt).
// Overflow bounds of the bins (wx_diag.h): a lane adds at most 2^14 addends below 2^39 (2^31 cells over 64 lanes x 2048 workgroups):
// 2^53, a wave 2^59; the low words of 256 workgroups of a shard stay below 2^40.
enum { WG = wxq::WG, WAVES = wxq::WAVES, MAX_WGS = 2048, SHARDS = 8, MAP_ROWS = 4 };
// the device table in 64-bit words, SHARDS copies: the bins of term k of channel c at (k * 4 + c) * NB (low words, then high words),
// the counters [reason][channel] and sum_count[channel], the two histograms [channel][bin]
enum { NQ = NT * 4, T_LO = 0, T_HI = NQ * wxd::NB, T_CNT = 2 * NQ * wxd::NB, T_SUMN = T_CNT + 16, T_LOW = T_SUMN + 4, T_HIGH = T_LOW + 4 * BINS, T_WORDS = T_HIGH + 4 * BINS };
// the workgroup's LDS tables behind the image, in 32-bit words: whole bin partials (64-bit), then counters and histograms (32-bit:
// a workgroup meets fewer than 2^32 cells)
enum { L_BINS = 0, L_CNT = 2 * NQ * wxd::NB, L_SUMN = L_CNT + 16, L_LOW = L_SUMN + 4, L_HIGH = L_LOW + 4 * BINS, L_WORDS = L_HIGH + 4 * BINS };
static_assert(MAX_MEMBERS == wxq::STAGED_MEMBERS && L_WORDS * 4 == 4720 && T_WORDS == 1180, "the tables");

struct Args {
  int X;            // cells per row of the members' arrays
  int x0, y0, w, h; // the rectangle
  int n_sel;        // selected members: tab[0 .. n_sel); tab[n_sel] is the truth
  const wxe::Member *tab;
  u64 *table;                      // SHARDS * T_WORDS words, zeroed in front of the launch
  float4 *error, *variance, *crps; // the wanted maps (w * h texels each, rows bottom-up), nullptr: not wanted
};

template <int P>
__global__ __launch_bounds__(WG) void k_ens_score(const Args a)
{
  constexpr unsigned ROWS = P > MAP_ROWS ? P : MAP_ROWS;
  __shared__ __attribute__((aligned(16))) unsigned wxq_lds[ROWS * 256u + L_WORDS]; // [row][channel][lane], ROWS rows; behind it the tables (64-bit bins first)
  unsigned *const tabs = wxq_lds + ROWS * 256u;
  u64 *const bins = (u64 *)(tabs + L_BINS);
  const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const unsigned chunks = wxe::chunks_per_row(a.w) * (unsigned)a.h;
  const wxe::CTab tab = wxe::const_table(a.tab);
  const unsigned n_sel = (unsigned)a.n_sel;
  unsigned *const col = wxq_lds + wv * 64u + lane; // this thread's column: row i at col[i * 256]
  for (unsigned i = threadIdx.x; i < (unsigned)L_WORDS; i += WG) tabs[i] = 0u;
  __syncthreads();
  int cur[NT];
  long long acc[NT];
#pragma unroll
  for (int k = 0; k < NT; k++) cur[k] = 0, acc[k] = 0;
  unsigned cnt[4] = {0u, 0u, 0u, 0u}, sum_n = 0u; // cnt: wave-uniform; sum_n: this lane's
  const float nan = __builtin_nanf("");
  const bool maps = a.error || a.variance || a.crps;
  for (unsigned ch = blockIdx.x; ch < chunks; ch += gridDim.x) { // (workgroup-uniform trip count: every barrier below is reached by all)
    const wxe::Chunk at = wxe::chunk_at(ch, lane, a.x0, a.y0, a.w); // (a lane past the edge stays for the barriers, with offsets 0)
    const size_t off = at.valid ? wxe::texel_at(a.X, at.gx, at.gy) : 0, o = at.valid ? wxe::plane_at(a.w, at.x, at.y) : 0;
    wxq::Staged<P>::stage(wxq_lds, tab, n_sel, off, at.valid, lane, wv); // 1.
    // the truth's value of this thread's channel (in flight across the barrier)
    unsigned t_key = KEY_PAD;
    if (at.valid) t_key = truth_key(wxq::ld_chan(tab + n_sel, off, wv), wxe::ld_wall_dist(tab + n_sel, off));
    __syncthreads();
    unsigned key[P];
    wxq::Staged<P>::sorted_column(key, col);
    // 2. the walk over the registers
    wxq::Tally tl{0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < P; i++) wxq::tally_add(tl, key[i], t_key);
    const int n = tl.n;
    Cell r;
#pragma unroll
    for (int k = 0; k < NT; k++) r.f[k] = nan;
    if (t_key != KEY_PAD && n >= 1) {
      const double t = (double)wxq::value_of(t_key);
      Sums s;
      sums_init(s);
#pragma unroll
      for (int i = 0; i < P; i++)
        if (i < n) sum_step(s, key[i]);
      const double m = mean_of(s, n);
#pragma unroll
      for (int i = 0; i < P; i++)
        if (i < n) dev_step(s, key[i], i, n, m, t);
      five_of(s, n, m, t, r.f);
    }
    r.reason = reason_of(t_key, n, r.f);
    const bool scored = at.valid && r.reason == SCORED;
    // 3. the terms, the counters, the histograms (every lane of the wave is here)
#pragma unroll
    for (int k = 0; k < NT; k++) wxd::wave_add(cur[k], acc[k], wxd::term_of(r.f[k], scored), bins + (k * 4 + (int)wv) * wxd::NB);
#pragma unroll
    for (int q = 0; q < 4; q++) cnt[q] += (unsigned)__popcll(__ballot(at.valid && r.reason == q));
    sum_n += scored ? (unsigned)n : 0u;
    if (scored) {
      atomicAdd(&tabs[L_LOW + wv * BINS + (unsigned)tl.below], 1u);
      atomicAdd(&tabs[L_HIGH + wv * BINS + (unsigned)(tl.below + tl.equal)], 1u);
    }
    // 4. the wanted maps through the column's first rows (every read of the keys is done), then whole texels out
    if (maps) { // (uniform: a kernel argument; every thread of the grid takes the same side, the barrier inside included)
      col[0 * 256] = wxq::f32_bits(scored ? r.f[0] : nan);
      col[1 * 256] = wxq::f32_bits(scored ? r.f[3] : nan);
      col[2 * 256] = wxq::f32_bits(scored ? r.f[4] : nan);
      __syncthreads();
      if (wv < 3u) {
        uint4 *dst = (uint4 *)(wv == 0u ? a.error : (wv == 1u ? a.variance : a.crps)); // (uniform)
        if (dst && at.valid) {
          const unsigned *src = wxq_lds + wv * 256u + lane;
          dst[o] = make_uint4(src[0], src[64], src[128], src[192]);
        }
      }
    }
    __syncthreads(); // the image is free for the next chunk
  }
  // 5. the wave's registers into the workgroup's tables, the workgroup's tables into its shard
#pragma unroll
  for (int k = 0; k < NT; k++) wxd::wave_flush(cur[k], acc[k], bins + (k * 4 + (int)wv) * wxd::NB);
  const unsigned total_n = (unsigned)wxd::wave_sum((long long)sum_n);
  if (lane == 0u) {
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (cnt[q]) atomicAdd(&tabs[L_CNT + q * 4 + wv], cnt[q]);
    if (total_n) atomicAdd(&tabs[L_SUMN + wv], total_n);
  }
  __syncthreads();
  u64 *const shard = a.table + (size_t)(blockIdx.x % SHARDS) * T_WORDS;
  for (unsigned i = threadIdx.x; i < (unsigned)(NQ * wxd::NB); i += WG) {
    const long long p = (long long)bins[i], h = p >> 32;
    if (!p) continue;
    atomicAdd(&shard[T_LO + i], (u64)(uint32_t)p);
    if (h) atomicAdd(&shard[T_HI + i], (u64)h);
  }
  for (unsigned i = threadIdx.x; i < (unsigned)(L_WORDS - L_CNT); i += WG) { // (counters and histograms: the two layouts agree behind the bins)
    const unsigned v = tabs[L_CNT + i];
    if (v) atomicAdd(&shard[T_CNT + i], (u64)v);
  }
}
static_assert(T_SUMN - T_CNT == L_SUMN - L_CNT && T_LOW - T_CNT == L_LOW - L_CNT && T_HIGH - T_CNT == L_HIGH - L_CNT && T_WORDS - T_CNT == L_WORDS - L_CNT, "one push loop");

// the SHARDS copies of the device table -> the domain's accumulators
inline void acc_from_table(const u64 *tab, Acc &a)
{
  memset(&a, 0, sizeof(a));
  for (int s = 0; s < SHARDS; s++, tab += T_WORDS)
    for (int c = 0; c < 4; c++) {
      for (int k = 0; k < NT; k++)
        for (int b = 0; b < wxd::NB; b++) {
          a.lo[c][k][b] += tab[T_LO + (k * 4 + c) * wxd::NB + b];
          a.hi[c][k][b] += (int64_t)tab[T_HI + (k * 4 + c) * wxd::NB + b];
        }
      for (int q = 0; q < 4; q++) a.cnt[q][c] += (int64_t)tab[T_CNT + q * 4 + c];
      a.sum_count[c] += (int64_t)tab[T_SUMN + c];
      for (int b = 0; b < BINS; b++) a.low[c][b] += (int64_t)tab[T_LOW + c * BINS + b], a.high[c][b] += (int64_t)tab[T_HIGH + c * BINS + b];
    }
}

template <int P>
static hipError_t launch(const Args &a, unsigned wgs, hipStream_t stream)
{
  hipLaunchKernelGGL(k_ens_score<P>, dim3(wgs), dim3(WG), 0, stream, a);
  return hipGetLastError();
}

} // namespace wxs

int wx_ens_score_max_members(void) { return wxs::MAX_MEMBERS; }

int wx_ens_score_cells(int n_members, size_t n_cells, const float *const *field, const int8_t *const *wall, const float *truth_field, const int8_t *truth_wall,
                       const uint8_t *member_mask, wx_ens_score *out)
{
  return wxs::score_cells(n_members, n_cells, field, wall, truth_field, truth_wall, member_mask, out);
}

int wx_ensemble_scores(wx_ensemble *e, wx_sim *truth, int field, int x, int y, int w, int h, const uint8_t *member_mask, wx_ens_score *out)
{
  static const char *const call = "wx_ensemble_scores";
  if (!e || !truth || !out) return WX_E_INVALID;
  // the arguments first: nothing below this block is reached with a bad one, and nothing in it touches the device
  if (int rc = ens_check_state_field(e, call, field)) return rc;
  const char *why;
  if (int rc = wxs::check_selection((int)e->member.size(), member_mask, &why)) return efail(e, rc, "wx_ensemble_scores: %s", why);
  const std::vector<int> sel = ens_select(e, member_mask);
  for (int i : sel)
    if (e->member[i] == truth) return efail(e, WX_E_INVALID, "wx_ensemble_scores: truth is member %d, which is selected: the truth does not enter (mask it out)", i);
  if (truth->halo != 0 || truth->X != truth->Xg) return efail(e, WX_E_INVALID, "wx_ensemble_scores: truth is a slab handle (whole-domain handles only)");
  if (truth->X != e->X || truth->Y != e->Y) return efail(e, WX_E_INVALID, "wx_ensemble_scores: truth has %d x %d cells, the members %d x %d", truth->X, truth->Y, e->X, e->Y);
  if (truth->device != e->device) return efail(e, WX_E_INVALID, "wx_ensemble_scores: truth lives on device %d, the ensemble on device %d", truth->device, e->device);
  if (int rc = ens_check_rect(e, call, x, y, w, h)) return rc;
  if (int rc = ens_require_uploaded(e, call, sel)) return rc;
  if (!truth->uploaded) return efail(e, WX_E_STATE, "truth: wx_ensemble_scores before wx_upload");
  if (e->broken) return WX_E_STATE; // (the message of the failed step is kept; in front of the wait for truth)
  EnsCall c(e, call, K_ENS_SCORE);

  // behind everything pending on truth's stream, as wx_copy_state orders its two handles: truth's pending report is consumed and
  // returned here, and then nothing is launched (a member of this ensemble is on the ensemble's stream: wx_ensemble_sync below)
  if (truth->ens != e)
    if (int rc = wx_sync(truth)) return efail(e, rc, "truth: %s", truth->err.c_str());

  // the table, then the wanted maps back to back
  const size_t cells = (size_t)w * h, table_bytes = (size_t)wxs::SHARDS * wxs::T_WORDS * sizeof(wxs::u64);
  float *const host_ptr[3] = {out->error, out->variance, out->crps};
  size_t at[3], out_bytes = table_bytes;
  for (int p = 0; p < 3; p++) {
    at[p] = out_bytes;
    if (host_ptr[p]) out_bytes += cells * 16;
  }
  const int n_sel = (int)sel.size();
  if (int rc = ens_begin(c, n_sel + 1, out_bytes)) return rc;
  EnsStage *st = c.st;
  ens_table_field(c, sel, field, truth, -1); // the truth behind the selected ones

  wxs::Args a;
  memset(&a, 0, sizeof(a));
  a.X = e->X, a.x0 = x, a.y0 = y, a.w = w, a.h = h, a.n_sel = n_sel;
  a.tab = st->tab_dev;
  a.table = (wxs::u64 *)st->out_dev;
  auto dev_plane = [&](int p) -> float4 * { return host_ptr[p] ? (float4 *)(st->out_dev + at[p]) : nullptr; };
  a.error = dev_plane(0), a.variance = dev_plane(1), a.crps = dev_plane(2);
  int P = 1;
  while (P < n_sel) P <<= 1;

  // behind the table of members: the zeroed table of sums, kernel, everything to the pinned copy
  if (c.he == hipSuccess) c.he = hipMemsetAsync(st->out_dev, 0, table_bytes, e->stream);
  const unsigned wgs = ens_wgs_wg_per_item(ens_chunks(w, h), wxs::MAX_WGS);
  ens_launch(c, K_ENS_SCORE, [&]() -> hipError_t {
    switch (P) {
    case 1: return wxs::launch<1>(a, wgs, e->stream);
    case 2: return wxs::launch<2>(a, wgs, e->stream);
    case 4: return wxs::launch<4>(a, wgs, e->stream);
    case 8: return wxs::launch<8>(a, wgs, e->stream);
    case 16: return wxs::launch<16>(a, wgs, e->stream);
    case 32: return wxs::launch<32>(a, wgs, e->stream);
    default: return wxs::launch<wxs::MAX_MEMBERS>(a, wgs, e->stream);
    }
  });
  if (c.he == hipSuccess) c.he = hipMemcpyAsync(st->out_host, st->out_dev, out_bytes, hipMemcpyDeviceToHost, e->stream);
  if (int rc = ens_finish(c)) return rc;
  wxs::Acc *acc = new wxs::Acc();
  wxs::acc_from_table((const wxs::u64 *)st->out_host, *acc);
  wxs::acc_finish(*acc, out);
  delete acc;
  for (int p = 0; p < 3; p++)
    if (host_ptr[p]) memcpy(host_ptr[p], st->out_host + at[p], cells * 16);
  return WX_OK;
}
