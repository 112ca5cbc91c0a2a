// wx_ens_gram.h -- the members' Gram matrix over a rectangle on the device (include/wxsim.h: wx_ens_gram, wx_ensemble_gram,
// wx_ens_gram_cells): per channel the n x n matrix of the exact sums of the float terms (float)(d_a * d_b), defined bit for bit by
// wx_ens_gram_cell.h. Included at the end of wxsim.hip behind wx_ens_nbhd.h (the entry points are declared extern "C" by
// include/wxsim.h). Two launches; nothing is written but the ensemble's own output buffer, and what leaves the device is integers.
//
// k_ens_gram_centre. k_ens_cov's shape and its first walk: one lane per cell, a wave takes 64 consecutive x of one row, waves grid-stride
// over the chunks with a capped grid. Walk 1: Sx and the entry test; walk 2 (the same lines again: L2) the overflow test on the diagonal
// terms over ALL selected members. It stores, per channel, one double per cell into a plane of the rectangle -- the centre xm if the
// cell-channel ENTERS, a NaN if it does not (an eligible cell's xm is finite: at most 64 finite floats summed in double) -- and counts
// entered / excluded / overflow per channel (ballots in wave-uniform registers, the workgroup's LDS words, one push per workgroup).
// A pre-pass, and not the mean recomputed per pair tile: a tile holds 32 of up to 64 members, so every one of the up to 40 (tile,
// channel) jobs of a chunk would walk all members again for a number that is the same for all of them; the planes cost 32 B per cell
// written once and 8 B per cell and job read back, coalesced.
//
// k_ens_gram. The inverse of the other ensemble kernels: a lane OWNS A PAIR, not a cell. The pairs a <= b of the selected members are
// cut into TILE x TILE member blocks (A, B), A <= B; a JOB is one (tile, channel), and workgroup g of the grid has job g % n_jobs FOR
// THE WHOLE LAUNCH and walks the chunks slot, slot + n_slots, ... (slot = g / n_jobs) with the shared chunk cursor. Per chunk: the four
// waves stage the channel's values of the tile's members (rows of 64 cells, 65 floats apart: the 32 lanes of a read group that read
// different rows at one cell meet different banks) and the 64 centres, __syncthreads(), then thread (al, bl) = (tid / 16, tid % 16)
// walks the 64 cells for ITS pair (A*16 + al, B*16 + bl): two LDS reads of a value, one broadcast read of the centre, d_a, d_b, the
// term, wxd::term_of, and the addend goes into a register while the bin stays the same and into the thread's own LDS column
// bins[bin][tid] (8-byte words, 2048 bytes between a thread's bins: no bank is shared between threads, whatever their bins) when it
// changes -- the bin is a dynamic index, so the sixteen words are in LDS, not in registers. Nobody else touches a thread's column: no
// atomics and no barrier on the accumulators. A diagonal tile (A == B) uses the threads with al <= bl and stages its rows once.
// Flush: every FLUSH_CHUNKS chunks and behind the loop each thread adds its non-zero words into the device table
// [channel][pair][bin] as (low 32 bits, rest): two 64-bit integer atomics, met by the n_slots workgroups of the same job only.
//   CAPACITY: an addend is below 2^39 (wx_diag.h); a thread adds at most 64 per chunk, so FLUSH_CHUNKS = 2^17 chunks stay below 2^62 in
//   a register and in a word. The table: a flush adds less than 2^32 to a low word and less than 2^31 in magnitude to a high word;
//   2^31 cells are at most 2^25 chunks per slot, 2^8 periodic flushes and one final one from each of at most MAX_WGS workgroups.
//   LDS: 32768 (bins) + 8320 (values) + 512 (centres) = 41600 bytes static: three workgroups of 4 waves per CU of 160 KiB.
//   BARRIERS: the chunk loop's trip count depends on blockIdx and gridDim only; lanes past the right edge of the rectangle load
//   nothing, stage a NaN centre -- their cells contribute to no pair -- and walk through every barrier. Nothing waits on the device.
// What it does not try: MFMA or any floating-point reduction (the hardware's summation order is not the definition); cells split
// among the idle threads of a small ensemble's single tile (n = 8 uses 36 of 256 threads); all four channels of a tile in one workgroup
// (128 KiB of bins: one workgroup per CU).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/wxsim.h"
#include "wx_diag.h"
#include "wx_ens_frame.h"
#include "wx_ens_gram_cell.h"

namespace wxg {

typedef unsigned long long u64;
// MAX_WGS caps both grids; a job's workgroups are MAX_WGS / n_jobs at most (n_jobs <= 40)
enum { WG = 256, WAVES = WG / 64, MAX_WGS = 2048, TILE = 16, UNROLL = 8, ROW = 65, FLUSH_CHUNKS = 1 << 17 };
static_assert(TILE * TILE == WG && MAX_MEMBERS % TILE == 0, "a thread per pair of a tile");
// the head of the output buffer in 64-bit words: the table [channel][pair][bin][low, high], then the counts [what][channel]
inline size_t table_words(int n) { return (size_t)4 * (size_t)pair_count(n) * wxd::NB * 2; }
enum { N_COUNTS = 12 };
// tiles of n members: the blocks (A, B), A <= B, row-major
inline int blocks_of(int n) { return (n + TILE - 1) / TILE; }
inline int jobs_of(int n) { return blocks_of(n) * (blocks_of(n) + 1) / 2 * 4; }

struct CentreArgs {
  int X;
  int x0, y0, w, h;
  int n_sel, center;
  const wxe::Member *tab; // n_sel entries of the field
  double *mean;           // 4 planes of w * h doubles: the centre, or NaN where the cell-channel does not enter
  u64 *counts;            // N_COUNTS words, zeroed in front of the launch
};

struct Args {
  int X;
  int x0, y0, w, h;
  int n_sel, n_jobs;
  const wxe::Member *tab;
  const double *mean;
  u64 *table; // table_words(n_sel) words, zeroed in front of the launch
};

#if defined(__HIPCC__)
struct Walk1 {
  double S[4];
  bool ok[4];
};
struct Walk2 {
  bool ovf[4];
};

__global__ __launch_bounds__(WG) void k_ens_gram_centre(const CentreArgs a)
{
  __shared__ unsigned sh_cnt[N_COUNTS];
  if (threadIdx.x < (unsigned)N_COUNTS) sh_cnt[threadIdx.x] = 0u;
  __syncthreads();
  const wxe::WaveOfGrid wg = wxe::wave_of_grid(WAVES);
  const unsigned chunks = wxe::chunks_per_row(a.w) * (unsigned)a.h;
  const wxe::CTab tab = wxe::const_table(a.tab);
  const int n = a.n_sel;
  const size_t plane = (size_t)a.w * (size_t)a.h;
  unsigned cnt[3][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}}; // wave-uniform
  for (unsigned ch = wg.wave; ch < chunks; ch += wg.n_waves) {
    const wxe::Chunk at = wxe::chunk_at(ch, wg.lane, a.x0, a.y0, a.w);
    int what[4] = {-1, -1, -1, -1}; // (a lane past the edge: counted nowhere)
    if (at.valid) {
      const size_t off = wxe::texel_at(a.X, at.gx, at.gy), o = wxe::plane_at(a.w, at.x, at.y);
      const auto load = [&](int k) { return wxe::ld_field_wall(tab + k, off); };
      // walk 1: Sx and the entry test
      const Walk1 w1 = wxe::member_walk<UNROLL>(n, Walk1{{0.0, 0.0, 0.0, 0.0}, {true, true, true, true}}, load, [](Walk1 &w, int, const wxe::TexelWall &m) {
        const bool air = m.wd != 0;
        sum_add(w.S[0], w.ok[0], m.v.x, air), sum_add(w.S[1], w.ok[1], m.v.y, air), sum_add(w.S[2], w.ok[2], m.v.z, air), sum_add(w.S[3], w.ok[3], m.v.w, air);
      });
      double xm[4];
#pragma unroll
      for (int c = 0; c < 4; c++) xm[c] = centre_of(w1.S[c], n, a.center);
      Walk2 w2 = {{false, false, false, false}};
      if (w1.ok[0] || w1.ok[1] || w1.ok[2] || w1.ok[3]) // walk 2: the diagonal terms of every selected member
        w2 = wxe::member_walk<UNROLL>(n, w2, [&](int k) { return wxe::ld_field(tab + k, off); }, [&](Walk2 &w, int, const wxe::f32x4 &v) {
          w.ovf[0] = w.ovf[0] || diag_overflows(dev_of(v.x, xm[0])), w.ovf[1] = w.ovf[1] || diag_overflows(dev_of(v.y, xm[1]));
          w.ovf[2] = w.ovf[2] || diag_overflows(dev_of(v.z, xm[2])), w.ovf[3] = w.ovf[3] || diag_overflows(dev_of(v.w, xm[3]));
        });
#pragma unroll
      for (int c = 0; c < 4; c++) {
        what[c] = !w1.ok[c] ? EXCLUDED : (w2.ovf[c] ? OVERFLOW_ : ENTERED);
        a.mean[(size_t)c * plane + o] = what[c] == ENTERED ? xm[c] : wxc::f64_nan();
      }
    }
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
      for (int c = 0; c < 4; c++) cnt[q][c] += (unsigned)__popcll(__ballot(what[c] == q));
  }
  if (wg.lane == 0u) {
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
      for (int c = 0; c < 4; c++)
        if (cnt[q][c]) atomicAdd(&sh_cnt[q * 4 + c], cnt[q][c]); // (a workgroup meets fewer than 2^32 cells)
  }
  __syncthreads();
  if (threadIdx.x < (unsigned)N_COUNTS && sh_cnt[threadIdx.x]) atomicAdd(&a.counts[threadIdx.x], (u64)sh_cnt[threadIdx.x]);
}

__global__ __launch_bounds__(WG) void k_ens_gram(const Args a)
{
  __shared__ long long bins[wxd::NB * WG]; // [bin][thread]
  __shared__ float vals[2 * TILE * ROW];   // [row][cell]: rows 0 .. 15 the members of block A, 16 .. 31 of block B (A != B)
  __shared__ double xm_s[64];
  const unsigned tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const unsigned n = (unsigned)a.n_sel, n_jobs = (unsigned)a.n_jobs;
  const unsigned job = blockIdx.x % n_jobs, slot = blockIdx.x / n_jobs, n_slots = gridDim.x / n_jobs; // (the grid is n_slots * n_jobs)
  const unsigned c = job & 3u, nb = (n + TILE - 1u) / TILE;
  unsigned A = 0, t = job >> 2;
  while (t >= nb - A) t -= nb - A, A++; // tile t -> (A, B), row-major over A <= B
  const unsigned B = A + t;
  const bool diagonal = A == B;
  const unsigned al = tid / TILE, bl = tid % TILE, ma = A * TILE + al, mb = B * TILE + bl;
  const bool active = ma < n && mb < n && ma <= mb;
  const float *const row_a = vals + al * ROW, *const row_b = vals + (diagonal ? bl : TILE + bl) * ROW;
  long long *const col = bins + tid; // this thread's column: bin i at col[i * WG]
  u64 *const out = a.table + ((size_t)c * (size_t)pair_count((int)n) + (size_t)(active ? pair_index((int)n, (int)ma, (int)mb) : 0)) * wxd::NB * 2;
#pragma unroll
  for (int i = 0; i < wxd::NB; i++) col[i * WG] = 0;
  int cur = 0;
  long long acc = 0;
  const auto flush = [&] { // this thread's words into the device table (its own column: no barrier)
    if (!active) return;
    col[cur * WG] += acc, acc = 0;
#pragma unroll
    for (int i = 0; i < wxd::NB; i++) {
      const long long p = col[i * WG], h = p >> 32;
      if (!p) continue;
      atomicAdd(&out[2 * i], (u64)(uint32_t)p);
      if (h) atomicAdd(&out[2 * i + 1], (u64)h);
      col[i * WG] = 0;
    }
  };
  const unsigned chunks = wxe::chunks_per_row(a.w) * (unsigned)a.h;
  const wxe::CTab tab = wxe::const_table(a.tab);
  const size_t plane = (size_t)a.w * (size_t)a.h;
  unsigned since = 0;
  for (unsigned ch = slot; ch < chunks; ch += n_slots) { // (workgroup-uniform trip count: every barrier below is reached by all)
    const wxe::Chunk at = wxe::chunk_at(ch, lane, a.x0, a.y0, a.w); // (a lane past the edge stays for the barriers and loads nothing)
    const size_t off = at.valid ? wxe::texel_at(a.X, at.gx, at.gy) : 0;
#pragma unroll
    for (unsigned i = 0; i < 2u * TILE / WAVES; i++) {
      const unsigned r = wv + WAVES * i; // (wave-uniform)
      if (r >= TILE && diagonal) break;
      const unsigned m = r < TILE ? A * TILE + r : B * TILE + (r - TILE);
      float v = 0.0f;
      if (at.valid && m < n) v = wxq::ld_chan(tab + m, off, c);
      vals[r * ROW + lane] = v;
    }
    if (wv == 0u) xm_s[lane] = at.valid ? a.mean[(size_t)c * plane + wxe::plane_at(a.w, at.x, at.y)] : wxc::f64_nan();
    __syncthreads();
    if (active) {
#pragma unroll 4
      for (unsigned i = 0; i < 64u; i++) {
        const double xm = xm_s[i];
        if (!wxcell::f64_finite(xm)) continue; // (the same for every thread of the workgroup)
        const wxd::Term tm = wxd::term_of(term_of_pair(dev_of(row_a[i], xm), dev_of(row_b[i], xm)), true);
        if (tm.addend != 0 && tm.bin != cur) col[cur * WG] += acc, acc = 0, cur = tm.bin;
        acc += tm.addend;
      }
    }
    __syncthreads(); // the image is free for the next chunk
    if (++since == (unsigned)FLUSH_CHUNKS) flush(), since = 0;
  }
  flush();
}
#endif // __HIPCC__

// the device table -> the rectangle's accumulators
inline void acc_from_table(const u64 *tab, Acc &a)
{
  const size_t words = (size_t)4 * (size_t)a.pairs * wxd::NB;
  for (size_t i = 0; i < words; i++) a.lo[i] = tab[2 * i], a.hi[i] = (int64_t)tab[2 * i + 1];
  const u64 *cnt = tab + 2 * words;
  for (int q = 0; q < 3; q++)
    for (int c = 0; c < 4; c++) a.cnt[q][c] = (int64_t)cnt[q * 4 + c];
}

} // namespace wxg

int wx_ens_gram_max_members(void) { return wxg::MAX_MEMBERS; }

int wx_ens_gram_cells(wx_ens_gram *g, int X, int Y, int n_members, const float *const *field, const int8_t *const *wall, const uint8_t *member_mask)
{
  return wxg::gram_cells(g, X, Y, n_members, field, wall, member_mask);
}

int wx_ensemble_gram(wx_ensemble *e, wx_ens_gram *g, const uint8_t *member_mask)
{
  static const char *const call = "wx_ensemble_gram";
  if (!e || !g) return WX_E_INVALID;
  // the arguments first: nothing below this block is reached with a bad one, and nothing in it touches the device
  const char *why;
  if (int rc = wxg::check_desc(g, &why)) return efail(e, rc, "wx_ensemble_gram: %s", why);
  const std::vector<int> sel = ens_select(e, member_mask);
  if (int rc = wxg::check_selection(g, sel.size(), &why)) return efail(e, rc, "wx_ensemble_gram: %s (%zu selected)", why, sel.size());
  if (int rc = wxg::check_rect(g, e->X, e->Y, &why)) return efail(e, rc, "wx_ensemble_gram: %s", why);
  if (int rc = ens_require_uploaded(e, call, sel)) return rc;

  const int n = (int)sel.size(), n_jobs = wxg::jobs_of(n);
  const size_t plane = (size_t)g->w * (size_t)g->h;
  // the output buffer: the table and the counts (what comes back); the four planes of centres are device-only scratch
  const size_t head_bytes = (wxg::table_words(n) + wxg::N_COUNTS) * sizeof(wxg::u64);
  EnsCall frame(e, call, K_ENS_GRAM_CENTRE);
  if (int rc = ens_begin(frame, n, head_bytes)) return rc;
  if (int rc = ens_aux_reserve(e, call, 4 * plane * sizeof(double))) return rc;
  EnsStage *st = frame.st;

  wxg::CentreArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.X = e->X, ca.x0 = g->x, ca.y0 = g->y, ca.w = g->w, ca.h = g->h, ca.n_sel = n, ca.center = g->center;
  ca.tab = st->tab_dev;
  ca.mean = (double *)st->aux_dev;
  ca.counts = (wxg::u64 *)st->out_dev + wxg::table_words(n);
  wxg::Args a;
  memset(&a, 0, sizeof(a));
  a.X = e->X, a.x0 = g->x, a.y0 = g->y, a.w = g->w, a.h = g->h, a.n_sel = n, a.n_jobs = n_jobs;
  a.tab = st->tab_dev, a.mean = ca.mean, a.table = (wxg::u64 *)st->out_dev;

  // behind the table of members: the zeroed head, the centres, the pairs, the head to the pinned copy
  ens_table_field(frame, sel, g->field);
  if (frame.he == hipSuccess) frame.he = hipMemsetAsync(st->out_dev, 0, head_bytes, e->stream);
  const unsigned chunks = ens_chunks(g->w, g->h);
  const unsigned c_wgs = ens_wgs_wave_per_item(chunks, wxg::WAVES, wxg::MAX_WGS);
  ens_launch(frame, K_ENS_GRAM_CENTRE, [&] { hipLaunchKernelGGL(wxg::k_ens_gram_centre, dim3(c_wgs), dim3(wxg::WG), 0, e->stream, ca); });
  const unsigned n_slots = std::max(1u, std::min(chunks, (unsigned)wxg::MAX_WGS / (unsigned)n_jobs));
  ens_launch(frame, K_ENS_GRAM, [&] { hipLaunchKernelGGL(wxg::k_ens_gram, dim3(n_slots * (unsigned)n_jobs), dim3(wxg::WG), 0, e->stream, a); });
  if (frame.he == hipSuccess) frame.he = hipMemcpyAsync(st->out_host, st->out_dev, head_bytes, hipMemcpyDeviceToHost, e->stream);
  if (int rc = ens_finish(frame)) return rc;
  wxg::Acc acc(n);
  wxg::acc_from_table((const wxg::u64 *)st->out_host, acc);
  wxg::acc_finish(acc, g);
  return WX_OK;
}
