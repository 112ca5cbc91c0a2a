// wx_ens_nbhd.h -- neighbourhood ensemble probabilities and the sums of the fractions skill score (include/wxsim.h: wx_ens_nbhd,
// wx_ensemble_neighbourhood, wx_ens_nbhd_cells). Included at the end of wxsim.hip behind wx_ens_cov.h (the entry points are declared
// extern "C" by include/wxsim.h). THE definition is in wx_ens_nbhd_cell.h (wxn::point_add, window_cell), __host__ __device__: the
// kernels and the host entry point run the same program text. Two launches; the members are read ONCE per grid cell, whatever the
// number of scales.
//
// k_ens_nbhd_points. One lane per cell of the GROWN rectangle -- the output rectangle grown by the largest rx / ry, rows clipped to
// the grid, columns clipped (no wrap) or continued around the seam (wrap_x; at most X columns) --, the launch shape and the member
// walk of k_ens_stat: a wave takes 64 consecutive column slots of one row, waves grid-stride over the chunks (wxe::chunk_at, the column wrap
// behind it; wxe::member_walk), the truth is the table entry behind the selection. One channel is looked at, so
// a member costs a 4-byte load of its value and the 4-byte wall texel (the same cache lines k_ens_stat's 16-byte loads touch). Out:
// Nf | Ef << 16 in a 32-bit word and No | Eo << 1 in a byte per cell, in the ensemble's device staging: 5 bytes per cell.
//
// k_ens_nbhd_windows<HX, HY>. An ITEM is (scale, tile of TILE_W x TILE_H output cells); persistent workgroups of 256 threads walk
// the items, scale-major, so a workgroup meets each scale's items in one run. Per item:
//   1. the tile plus its halo of THIS scale -- (TILE_W + 2 rx) x (TILE_H + 2 ry) packed counts -- from the staging into LDS; slots
//      outside the grid (or, for the ragged edge of the rectangle, outside the grown rectangle) are zeros. __syncthreads().
//   2. rows: every staged row's box sum over 2 rx + 1 columns for the TILE_W output columns, Ef with Eo and Nf with No in one word each
//      (a row sum is below 2^23, the truth's below 2^7). Consecutive lanes read consecutive words: no bank conflict. __syncthreads().
//   3. columns: thread (lx, ly) sums 2 ry + 1 rows, makes the window function and turns the three terms into wx_diag's (bin, addend),
//      which go into per-wave bin registers that live ACROSS the item loop (wxd::wave_add, as in k_ens_score); a wave is one row of
//      the tile, so the map stores are 256 contiguous bytes. The point totals ride with scale 0 (the centre of the staged image).
//      __syncthreads() before the next item is staged.
//   When the scale changes, and behind the loop, the registers are flushed into the workgroup's LDS bins of that scale; at the end ONE
//   push of the workgroup's table into its shard (blockIdx % 8) of the device table: integer atomics, so any launch shape gives the
//   same table. The host copies the 8 shards back once, adds them and rounds each sum once (wxd::bins_to_double).
//   LDS is STATIC, so the halo the image is sized for is a template parameter, chosen by the launch as the smallest of 8, 16, 32 that
//   holds the largest radius asked for: 34.7 / 52.7 / 96.2 KiB at TILE 64 x 16 (4 / 3 / 1 workgroups per CU).
//   BARRIERS: the item loop's trip count depends on blockIdx and gridDim only, the scale and the tile of an item are workgroup-uniform,
//   there is no `continue` or `return` inside the loop; lanes beyond the ragged edge store nothing, contribute nothing and walk
//   through every barrier. Nothing waits on the device: no spin, no grid barrier, no flag.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/wxsim.h"
#include "wx_diag.h"
#include "wx_ens_frame.h"
#include "wx_ens_nbhd_cell.h"

namespace wxn {

typedef unsigned long long u64;
// the points pass: k_ens_stat's shape. The windows pass: MAX_WGS is what the chip holds of the smallest image (256 CUs x 4); a
// workgroup pays for its table once (6.2 KiB zeroed, up to 788 words pushed), so the items are shared among resident workgroups.
// Overflow bounds of the bins (wx_diag.h): the terms lie in [0, 1], so an addend is below 2^39. A rectangle has fewer than 2^32 cells;
// once there are more items than workgroups a workgroup meets at most 2^32 / 1024 = 2^22 of them per scale, a lane 2^14: a lane's
// register stays below 2^53, a wave's sum below 2^59, a workgroup's LDS bin below 2^61; the low words of the 128 workgroups of a shard
// stay below 2^39. (The registers are flushed when the scale changes, so the scales do not add up.)
enum { WG = 256, WAVES = WG / 64, UNROLL = 8, POINTS_MAX_WGS = 2048 };
enum { TILE_W = 64, TILE_H = 16, WINDOWS_MAX_WGS = 1024, SHARDS = 8 };
// the device table in 64-bit words, SHARDS copies: the bins of term k of scale s at (s * NT + k) * NB (low words, then high words),
// then n_scored[s], n_unscored[s], and the four point totals. The workgroup's LDS table has the same layout: T_LO holds whole bin
// partials, T_HI stays unused.
enum { NQ = MAX_SCALES * NT, T_LO = 0, T_HI = NQ * wxd::NB, T_SCORED = 2 * NQ * wxd::NB, T_UNSCORED = T_SCORED + MAX_SCALES, T_TOTAL = T_UNSCORED + MAX_SCALES, T_WORDS = T_TOTAL + 4 };
static_assert(TILE_W == 64 && (TILE_W * TILE_H) % WG == 0 && T_WORDS == 788, "a wave is one row of the tile; the table");

struct PointArgs {
  int X;                  // cells per row of the members' arrays
  int gx0, gy0, gw, gh;   // the grown rectangle: column slot j is grid column (gx0 + j) mod X (gx0 may be negative under wrap_x), gw <= X
  int n_sel, has_truth;   // selected members: tab[0 .. n_sel); tab[n_sel] is the truth if there is one
  int channel, above;
  float thr;
  const wxe::Member *tab;
  uint32_t *cf;           // gw * gh words: Nf | Ef << 16
  uint8_t *co;            // gw * gh bytes: No | Eo << 1
};

struct WinArgs {
  int X, Y;
  int x0, y0, w, h;       // the rectangle
  int gx0, gy0, gw, gh;   // the grown rectangle the packed counts cover
  int wrap, n_scales;
  int rx[MAX_SCALES], ry[MAX_SCALES];
  const uint32_t *cf;
  const uint8_t *co;
  u64 *table;             // SHARDS * T_WORDS words, zeroed in front of the launch
  float *nep, *obs;       // the wanted maps ([s][h][w]), nullptr: not wanted
};

#if defined(__HIPCC__)
// what the points pass loads of a member: one channel's value and the wall texel's channel 1
struct ChanWall {
  float v;
  int wd;
};
// ... and accumulates: the members that enter, and those with the event
struct Counts {
  unsigned n, ev;
};

__global__ __launch_bounds__(WG) void k_ens_nbhd_points(const PointArgs a)
{
  const wxe::WaveOfGrid wg = wxe::wave_of_grid(WAVES);
  const unsigned chunks = wxe::chunks_per_row(a.gw) * (unsigned)a.gh;
  const wxe::CTab tab = wxe::const_table(a.tab);
  const unsigned c = (unsigned)a.channel;
  const float thr = a.thr;
  const int above = a.above;
  for (unsigned ch = wg.wave; ch < chunks; ch += wg.n_waves) {
    const wxe::Chunk at = wxe::chunk_at(ch, wg.lane, a.gx0, a.gy0, a.gw); // (of column SLOTS)
    if (!at.valid) continue;
    int col = at.gx; // in (-X, 2X): gx0 > -X and the slot is below gw <= X
    col += col < 0 ? a.X : 0;
    col -= col >= a.X ? a.X : 0;
    const size_t off = wxe::texel_at(a.X, col, at.gy), o = wxe::plane_at(a.gw, at.x, at.y);
    const Counts f = wxe::member_walk<UNROLL>(a.n_sel, Counts{0u, 0u}, [&](int k) { return ChanWall{wxq::ld_chan(tab + k, off, c), wxe::ld_wall_dist(tab + k, off)}; },
                                              [&](Counts &q, int, const ChanWall &m) { point_add(q.n, q.ev, m.v, m.wd, thr, above); });
    unsigned no = 0, eo = 0;
    if (a.has_truth) { // (uniform: a kernel argument)
      const float v = wxq::ld_chan(tab + a.n_sel, off, c);
      const int wd = wxe::ld_wall_dist(tab + a.n_sel, off);
      point_add(no, eo, v, wd, thr, above);
    }
    a.cf[o] = pack_f(f.n, f.ev);
    a.co[o] = pack_o(no, eo);
  }
}

// one scale's registers into the workgroup's table (every thread of the workgroup calls this together)
__device__ __forceinline__ void scale_flush(int s, int cur[NT], long long acc[NT], unsigned &n_sc, unsigned &n_un, u64 *tabs)
{
#pragma unroll
  for (int k = 0; k < NT; k++) wxd::wave_flush(cur[k], acc[k], tabs + T_LO + (s * NT + k) * wxd::NB);
  const long long sc = wxd::wave_sum((long long)n_sc), un = wxd::wave_sum((long long)n_un);
  if ((threadIdx.x & 63u) == 0u) {
    if (sc) atomicAdd(&tabs[T_SCORED + s], (u64)sc);
    if (un) atomicAdd(&tabs[T_UNSCORED + s], (u64)un);
  }
  n_sc = n_un = 0u;
}

template <int HX, int HY>
__global__ __launch_bounds__(WG) void k_ens_nbhd_windows(const WinArgs a)
{
  constexpr int SW = TILE_W + 2 * HX, SH = TILE_H + 2 * HY; // the staged image at the largest halo of this instantiation
  __shared__ u64 tabs[T_WORDS];
  __shared__ uint32_t s_f[SW * SH];         // [row][column]: Nf | Ef << 16
  __shared__ uint32_t s_h[2][TILE_W * SH];  // [row][output column]: the row sums, Ef | Eo << 24 and Nf | No << 24
  __shared__ uint8_t s_o[SW * SH];          // [row][column]: No | Eo << 1
  for (unsigned i = threadIdx.x; i < (unsigned)T_WORDS; i += WG) tabs[i] = 0;
  __syncthreads();
  const unsigned tpr = ((unsigned)a.w + TILE_W - 1) / TILE_W, tiles = tpr * (((unsigned)a.h + TILE_H - 1) / TILE_H), items = tiles * (unsigned)a.n_scales;
  int cur[NT];
  long long acc[NT];
#pragma unroll
  for (int k = 0; k < NT; k++) cur[k] = 0, acc[k] = 0;
  unsigned n_sc = 0u, n_un = 0u;
  u64 tot[4] = {0, 0, 0, 0};
  int at = blockIdx.x < items ? (int)(blockIdx.x / tiles) : 0; // the scale the registers belong to (workgroup-uniform)
  for (unsigned it = blockIdx.x; it < items; it += gridDim.x) { // (workgroup-uniform trip count: every barrier below is reached by all)
    const int s = (int)(it / tiles);
    const unsigned t = it - (unsigned)s * tiles, ty = t / tpr, tx = t - ty * tpr;
    if (s != at) { // (uniform)
      scale_flush(at, cur, acc, n_sc, n_un, tabs);
      at = s;
    }
    const int rx = a.rx[s], ry = a.ry[s], sw = TILE_W + 2 * rx, sh = TILE_H + 2 * ry; // rx <= HX, ry <= HY: the launch saw to it
    const int ox = a.x0 + (int)tx * TILE_W, oy = a.y0 + (int)ty * TILE_H;             // the tile's first output cell in the grid
    // 1. the image: rows oy - ry .., columns ox - rx ..
    for (int i = (int)threadIdx.x; i < sw * sh; i += WG) {
      const int r = i / sw, cc = i - r * sw, row = oy - ry + r, col = ox - rx + cc;
      int slot;
      bool in = row >= a.gy0 && row < a.gy0 + a.gh; // (the grown rectangle's rows are rows of the grid)
      if (a.wrap) {
        int cm = col % a.X;
        cm += cm < 0 ? a.X : 0;
        slot = cm - a.gx0; // gx0 in (-X, X): slot in (-X, 2X)
        slot += slot < 0 ? a.X : 0;
        slot -= slot >= a.X ? a.X : 0;
      } else {
        in = in && col >= 0 && col < a.X;
        slot = col - a.gx0;
      }
      in = in && slot >= 0 && slot < a.gw;
      const size_t g = in ? (size_t)(row - a.gy0) * (size_t)a.gw + (size_t)slot : 0;
      s_f[r * SW + cc] = in ? a.cf[g] : 0u;
      s_o[r * SW + cc] = in ? a.co[g] : (uint8_t)0;
    }
    __syncthreads();
    // 2. rows
    for (int i = (int)threadIdx.x; i < TILE_W * sh; i += WG) {
      const int r = i / TILE_W, cc = i - r * TILE_W;
      const uint32_t *f = s_f + r * SW + cc;
      const uint8_t *o = s_o + r * SW + cc;
      unsigned ef = 0, nf = 0, eo = 0, no = 0;
      for (int d = 0; d <= 2 * rx; d++) {
        const uint32_t pf = f[d], po = o[d];
        nf += pf & 0xFFFFu, ef += pf >> 16, no += po & 1u, eo += po >> 1;
      }
      s_h[0][i] = ef | (eo << 24), s_h[1][i] = nf | (no << 24);
    }
    __syncthreads();
    // 3. columns, the window function, the terms (every lane of the wave is here)
#pragma unroll
    for (int q = 0; q < TILE_W * TILE_H / WG; q++) {
      const int i = q * WG + (int)threadIdx.x, ly = i / TILE_W, lx = i - ly * TILE_W;
      int Af = 0, Bf = 0, Ao = 0, Bo = 0;
      for (int d = 0; d <= 2 * ry; d++) {
        const uint32_t h0 = s_h[0][(ly + d) * TILE_W + lx], h1 = s_h[1][(ly + d) * TILE_W + lx];
        Af += (int)(h0 & 0xFFFFFFu), Ao += (int)(h0 >> 24), Bf += (int)(h1 & 0xFFFFFFu), Bo += (int)(h1 >> 24);
      }
      const int px = ox - a.x0 + lx, py = oy - a.y0 + ly; // the output cell in the rectangle
      const bool valid = px < a.w && py < a.h;
      const Cell c = window_cell(Af, Bf, Ao, Bo);
      const bool scored = valid && c.scored;
#pragma unroll
      for (int k = 0; k < NT; k++) wxd::wave_add(cur[k], acc[k], wxd::term_of(c.t[k], scored), tabs + T_LO + (s * NT + k) * wxd::NB);
      n_sc += scored ? 1u : 0u, n_un += (valid && !scored) ? 1u : 0u;
      if (valid) {
        const size_t o = ((size_t)s * (size_t)a.h + (size_t)py) * (size_t)a.w + (size_t)px;
        if (a.nep) a.nep[o] = c.pf;
        if (a.obs) a.obs[o] = c.po;
        if (s == 0) { // the point totals: the cell's own counts, the centre of its window
          const uint32_t pf = s_f[(ly + ry) * SW + lx + rx], po = s_o[(ly + ry) * SW + lx + rx];
          tot[0] += pf >> 16, tot[1] += pf & 0xFFFFu, tot[2] += po >> 1, tot[3] += po & 1u;
        }
      }
    }
    __syncthreads(); // the image is free for the next item
  }
  scale_flush(at, cur, acc, n_sc, n_un, tabs);
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const long long v = wxd::wave_sum((long long)tot[q]);
    if ((threadIdx.x & 63u) == 0u && v) atomicAdd(&tabs[T_TOTAL + q], (u64)v);
  }
  __syncthreads();
  u64 *const shard = a.table + (size_t)(blockIdx.x % SHARDS) * T_WORDS;
  for (unsigned i = threadIdx.x; i < (unsigned)T_WORDS; i += WG) {
    const u64 v = tabs[i];
    if (!v) continue;
    if (i < (unsigned)T_HI) {
      const long long p = (long long)v, h = p >> 32;
      atomicAdd(&shard[T_LO + i], (u64)(uint32_t)p);
      if (h) atomicAdd(&shard[T_HI + i], (u64)h);
    } else {
      atomicAdd(&shard[i], v);
    }
  }
}

template <int HX, int HY>
static hipError_t launch_windows(const WinArgs &a, unsigned wgs, hipStream_t stream)
{
  hipLaunchKernelGGL((k_ens_nbhd_windows<HX, HY>), dim3(wgs), dim3(WG), 0, stream, a);
  return hipGetLastError();
}
#endif // __HIPCC__

// the SHARDS copies of the device table -> the domain's accumulators
inline void acc_from_table(const u64 *tab, Acc &a)
{
  memset(&a, 0, sizeof(a));
  for (int sh = 0; sh < SHARDS; sh++, tab += T_WORDS)
    for (int s = 0; s < MAX_SCALES; s++) {
      for (int k = 0; k < NT; k++)
        for (int b = 0; b < wxd::NB; b++) {
          a.lo[s][k][b] += tab[T_LO + (s * NT + k) * wxd::NB + b];
          a.hi[s][k][b] += (int64_t)tab[T_HI + (s * NT + k) * wxd::NB + b];
        }
      a.scored[s] += (int64_t)tab[T_SCORED + s], a.unscored[s] += (int64_t)tab[T_UNSCORED + s];
      if (s < 4) a.total[s] += (int64_t)tab[T_TOTAL + s];
    }
}

} // namespace wxn

int wx_ens_nbhd_max_radius(void) { return wxn::MAX_RADIUS; }

int wx_ens_nbhd_cells(const wx_ens_nbhd *args, wx_ens_nbhd_result *out, int X, int Y, int n_members, const float *const *field, const int8_t *const *wall,
                      const float *truth_field, const int8_t *truth_wall, const uint8_t *member_mask)
{
  return wxn::nbhd_cells(args, out, X, Y, n_members, field, wall, truth_field, truth_wall, member_mask);
}

int wx_ensemble_neighbourhood(wx_ensemble *e, wx_sim *truth, const wx_ens_nbhd *args, const uint8_t *member_mask, wx_ens_nbhd_result *out)
{
  static const char *const call = "wx_ensemble_neighbourhood";
  if (!e || !args || !out) return WX_E_INVALID;
  // the arguments first: nothing below this block is reached with a bad one, and nothing in it touches the device
  const char *why;
  if (int rc = wxn::check_desc(args, truth != nullptr, &why)) return efail(e, rc, "wx_ensemble_neighbourhood: %s", why);
  const std::vector<int> sel = ens_select(e, member_mask);
  if (sel.empty()) return efail(e, WX_E_INVALID, "wx_ensemble_neighbourhood: the member mask selects nobody");
  if (truth) {
    for (int i : sel)
      if (e->member[i] == truth) return efail(e, WX_E_INVALID, "wx_ensemble_neighbourhood: truth is member %d, which is selected: the truth does not enter (mask it out)", i);
    if (truth->halo != 0 || truth->X != truth->Xg) return efail(e, WX_E_INVALID, "wx_ensemble_neighbourhood: truth is a slab handle (whole-domain handles only)");
    if (truth->X != e->X || truth->Y != e->Y) return efail(e, WX_E_INVALID, "wx_ensemble_neighbourhood: truth has %d x %d cells, the members %d x %d", truth->X, truth->Y, e->X, e->Y);
    if (truth->device != e->device) return efail(e, WX_E_INVALID, "wx_ensemble_neighbourhood: truth lives on device %d, the ensemble on device %d", truth->device, e->device);
  }
  if (int rc = wxn::check_range(args, e->X, e->Y, &why))
    return efail(e, rc, "wx_ensemble_neighbourhood: rect (%d,%d %dx%d) in %dx%d: %s", args->x, args->y, args->w, args->h, e->X, e->Y, why);
  if (int rc = ens_require_uploaded(e, call, sel)) return rc;
  if (truth && !truth->uploaded) return efail(e, WX_E_STATE, "truth: wx_ensemble_neighbourhood before wx_upload");
  if (e->broken) return WX_E_STATE; // (the message of the failed step is kept; in front of the wait for truth)
  EnsCall c(e, call, K_ENS_NBHD_POINTS);

  // behind everything pending on truth's stream, as wx_ensemble_scores orders it: truth's pending report is consumed and returned
  // here, and then nothing is launched (a member of this ensemble is on the ensemble's stream: wx_ensemble_sync below)
  if (truth && truth->ens != e)
    if (int rc = wx_sync(truth)) return efail(e, rc, "truth: %s", truth->err.c_str());

  // the grown rectangle: what any window of the rectangle reaches
  const int X = e->X, Y = e->Y, x = args->x, y = args->y, w = args->w, h = args->h, ns = args->n_scales;
  int mrx = 0, mry = 0;
  for (int s = 0; s < ns; s++) mrx = std::max(mrx, (int)args->rx[s]), mry = std::max(mry, (int)args->ry[s]);
  const int gy0 = std::max(0, y - mry), gh = std::min(Y, y + h + mry) - gy0;
  int gx0, gw;
  if (args->wrap_x && w + 2 * mrx >= X) gx0 = 0, gw = X;           // every column
  else if (args->wrap_x) gx0 = x - mrx, gw = w + 2 * mrx;          // around the seam where it has to (gx0 > -X: mrx < X)
  else gx0 = std::max(0, x - mrx), gw = std::min(X, x + w + mrx) - gx0;

  // the table and the wanted maps back to back (what comes back), behind them the packed counts (what stays)
  const size_t cells = (size_t)w * h, gcells = (size_t)gw * gh, table_bytes = (size_t)wxn::SHARDS * wxn::T_WORDS * sizeof(wxn::u64);
  const size_t map_bytes = (size_t)ns * cells * sizeof(float);
  const size_t at_nep = table_bytes, at_obs = at_nep + (args->nep ? map_bytes : 0), back_bytes = at_obs + (args->obs_fraction ? map_bytes : 0);
  const size_t at_cf = (back_bytes + 15) & ~(size_t)15, at_co = at_cf + gcells * sizeof(uint32_t), out_bytes = at_co + gcells;
  const int n_sel = (int)sel.size();
  if (int rc = ens_begin(c, n_sel + 1, out_bytes)) return rc;
  EnsStage *st = c.st;
  ens_table_field(c, sel, args->field, truth, -1); // the truth behind the selected ones

  wxn::PointArgs p;
  memset(&p, 0, sizeof(p));
  p.X = X, p.gx0 = gx0, p.gy0 = gy0, p.gw = gw, p.gh = gh, p.n_sel = n_sel, p.has_truth = truth ? 1 : 0;
  p.channel = args->channel, p.above = args->above ? 1 : 0, p.thr = args->threshold;
  p.tab = st->tab_dev;
  p.cf = (uint32_t *)(st->out_dev + at_cf), p.co = (uint8_t *)(st->out_dev + at_co);
  wxn::WinArgs a;
  memset(&a, 0, sizeof(a));
  a.X = X, a.Y = Y, a.x0 = x, a.y0 = y, a.w = w, a.h = h, a.gx0 = gx0, a.gy0 = gy0, a.gw = gw, a.gh = gh;
  a.wrap = args->wrap_x ? 1 : 0, a.n_scales = ns;
  for (int s = 0; s < ns; s++) a.rx[s] = args->rx[s], a.ry[s] = args->ry[s];
  a.cf = p.cf, a.co = p.co;
  a.table = (wxn::u64 *)st->out_dev;
  a.nep = args->nep ? (float *)(st->out_dev + at_nep) : nullptr, a.obs = args->obs_fraction ? (float *)(st->out_dev + at_obs) : nullptr;

  // behind the table of members: the zeroed table of sums, the two kernels, what comes back to the pinned copy
  if (c.he == hipSuccess) c.he = hipMemsetAsync(st->out_dev, 0, table_bytes, e->stream);
  const unsigned p_wgs = ens_wgs_wave_per_item(ens_chunks(gw, gh), wxn::WAVES, wxn::POINTS_MAX_WGS);
  ens_launch(c, K_ENS_NBHD_POINTS, [&] { hipLaunchKernelGGL(wxn::k_ens_nbhd_points, dim3(p_wgs), dim3(wxn::WG), 0, e->stream, p); });
  const unsigned long long items =
      (unsigned long long)((w + wxn::TILE_W - 1) / wxn::TILE_W) * (unsigned long long)((h + wxn::TILE_H - 1) / wxn::TILE_H) * (unsigned long long)ns;
  const unsigned w_wgs = (unsigned)std::min<unsigned long long>(items, wxn::WINDOWS_MAX_WGS);
  const int halo = std::max(mrx, mry);
  ens_launch(c, K_ENS_NBHD_WINDOWS, [&]() -> hipError_t {
    if (halo <= 8) return wxn::launch_windows<8, 8>(a, w_wgs, e->stream);
    if (halo <= 16) return wxn::launch_windows<16, 16>(a, w_wgs, e->stream);
    return wxn::launch_windows<wxn::MAX_RADIUS, wxn::MAX_RADIUS>(a, w_wgs, e->stream);
  });
  if (c.he == hipSuccess) c.he = hipMemcpyAsync(st->out_host, st->out_dev, back_bytes, hipMemcpyDeviceToHost, e->stream);
  if (int rc = ens_finish(c)) return rc;
  wxn::Acc *acc = new wxn::Acc();
  wxn::acc_from_table((const wxn::u64 *)st->out_host, *acc);
  wxn::acc_finish(*acc, out);
  delete acc;
  if (args->nep) memcpy(args->nep, st->out_host + at_nep, map_bytes);
  if (args->obs_fraction) memcpy(args->obs_fraction, st->out_host + at_obs, map_bytes);
  return WX_OK;
}
