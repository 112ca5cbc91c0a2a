// Exact conservation and health diagnostics (include/wxsim.h: wx_diag, wx_diag_raw): one pass over the owned cells' base, water and
// wall texels (36 B per cell) plus one small pass over the droplets; the counterpart of the reference's commented-out
// readPixels-and-sum block (app.js:6736-6762).
//
// Exact sums: a finite float is m * 2^(e - 150), |m| < 2^24, e = 1..254 (subnormals: e = 1, no hidden bit). A quantity keeps 16 integer
// bins; bin e >> 4 receives the addend m << (e & 15), |addend| < 2^39, in int64. Integer addition is associative, so any order, launch
// shape or decomposition gives the same bins; the host combines them in a 320-bit integer and rounds once (diag_finish).
// Overflow bounds: a lane adds at most 2^13 addends (2^32 cells over 2048 x 256 lanes) -> 2^52; a wave 2^58, a workgroup 2^60. A
// workgroup's bin partial goes to the device table as its low 32 bits (unsigned) and the rest (signed), two 64-bit integer atomics: the
// low words of at most 2^11 workgroups stay below 2^43, the high words below 2^39. The table has one copy per XCD (workgroup index
// modulo 8) so that the atomics of a finishing workgroup meet those of its own XCD only.
//
// Real fields occupy one or two bins per quantity. While the 64 values of a wave share their bin (zero addends join any bin) every lane
// adds into a register of its own -- no cross-lane traffic per cell; the wave reduces that register when its bin changes and at the end.
// A wave whose lanes disagree adds lane by lane into the workgroup's LDS bins (ds_add_u64).
//
// Extremes: per lane the best order-preserving key and its global index per channel (a lane meets its cells in rising global index, so
// "strictly better" keeps the first occurrence), combined at the end as 64-bit keys (float order above the inverted index) with max.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include "../../include/wxsim.h"
#include "wx_ens_cell_common.h" // (plain C++: a host compiler takes the binning function and the 320-bit finish without the HIP headers)

namespace wxd {

enum { NQ = WX_DIAG_QUANTITIES, NB = WX_DIAG_BINS, NQ_CELL = 10, Q_DROP = 10 };
enum { C_AIR, C_WALL, C_MISMATCH, C_NEGW, C_NFB, C_NFW, C_VEG, C_DROPS, C_DROPS_NF, C_CELLS, NC };
// the device table, in 64-bit words, SHARDS copies: bins (low words, high words), 8 max keys + 8 min keys, first non-finite base / water, counters
enum { T_LO = 0, T_HI = NQ * NB, T_KEY = 2 * NQ * NB, T_FIRST = T_KEY + 16, T_CNT = T_FIRST + 2, T_WORDS = T_CNT + NC };
enum { SHARDS = 8, WG = 256, MAX_WGS = 2048 };
typedef unsigned long long u64;

struct Term {
  int bin;
  long long addend; // 0: nothing to add (a zero, a non-finite value, a value outside the quantity's set of cells)
};

using wxcell::f32_bits;
using wxcell::f32_finite;

// THE binning function: the kernel, wx_diag_accumulate and wx_diag_accumulate_cells all go through it
WX_HD inline Term term_of(float v, bool take)
{
  const uint32_t b = f32_bits(v), e = (b >> 23) & 255u, frac = b & 0x7FFFFFu;
  const uint32_t m = e ? (frac | 0x800000u) : frac, e1 = e ? e : 1u;
  long long a = (long long)m << (e1 & 15u);
  if (b >> 31) a = -a;
  if (e == 255u || !take) a = 0;
  return Term{(int)(e1 >> 4), a};
}
WX_HD inline bool f32_nan(float v) { return (f32_bits(v) & 0x7FFFFFFFu) > 0x7F800000u; }
// order-preserving key of a non-NaN float: a < b <=> ord(a) < ord(b); -0.0 and 0.0 share a key; never 0 and never 0xFFFFFFFF
WX_HD inline uint32_t ord_of(float v)
{
  uint32_t b = f32_bits(v);
  if (b == 0x80000000u) b = 0;
  return (b >> 31) ? ~b : (b | 0x80000000u);
}
inline float float_of_ord(uint32_t k)
{
  const uint32_t b = (k >> 31) ? (k & 0x7FFFFFFFu) : ~k;
  return __builtin_bit_cast(float, b);
}

// what one cell contributes
struct CellOut {
  Term t[NQ_CELL];
  uint32_t kmax[8], kmin[8]; // 0: no candidate
  int cnt[7];                // C_AIR .. C_VEG
};
WX_HD inline void classify(const float v[8], int wall_dist, int wall_veg, bool in, CellOut &o)
{
  const bool wall = in && wall_dist == 0, air = in && wall_dist != 0;
  bool nfb = false, nfw = false;
#pragma unroll
  for (int c = 0; c < 8; c++) {
    o.t[c] = term_of(v[c], air);
    const bool fin = f32_finite(v[c]);
    if (c < 4) nfb |= !fin;
    else nfw |= !fin;
    const bool cand = air && !f32_nan(v[c]);
    const uint32_t k = ord_of(v[c]);
    o.kmax[c] = cand ? k : 0u;
    o.kmin[c] = cand ? ~k : 0u;
  }
  o.t[8] = term_of(v[6], wall);
  o.t[9] = term_of(v[7], wall);
  o.cnt[C_AIR] = air;
  o.cnt[C_WALL] = wall;
  o.cnt[C_MISMATCH] = in && ((v[4] > 1000.0f) != wall);
  o.cnt[C_NEGW] = air && v[4] < 0.0f;
  o.cnt[C_NFB] = in && nfb;
  o.cnt[C_NFW] = in && nfw;
  o.cnt[C_VEG] = wall ? wall_veg : 0;
}

#if defined(__HIPCC__)
__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ u64 wave_max(u64 v)
{
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const u64 w = __shfl_xor(v, o);
    v = w > v ? w : v;
  }
  return v;
}
// one quantity of one wave: `cur` (wave-uniform) is the bin the lanes' registers `acc` belong to; bins = the workgroup's 16 LDS bins
__device__ __forceinline__ void wave_flush(int cur, long long &acc, u64 *bins)
{
  const long long s = wave_sum(acc);
  if ((threadIdx.x & 63) == 0 && s != 0) atomicAdd(&bins[cur], (u64)s);
  acc = 0;
}
// (all 64 lanes of the wave call this together)
__device__ __forceinline__ void wave_add(int &cur, long long &acc, const Term t, u64 *bins)
{
  const u64 act = __ballot(t.addend != 0);
  if (!act) return;
  const int b0 = __builtin_amdgcn_readlane(t.bin, (int)__ffsll(act) - 1);
  if (__ballot(t.addend != 0 && t.bin != b0) == 0) { // one bin for the whole wave: registers
    if (b0 != cur) {
      wave_flush(cur, acc, bins);
      cur = b0;
    }
    acc += t.addend;
  } else if (t.addend != 0) { // mixed exponents inside the wave: lane by lane into LDS
    atomicAdd(&bins[t.bin], (u64)t.addend);
  }
}
// the workgroup's LDS table -> its shard of the device table
__device__ __forceinline__ void table_push(const u64 *sh, u64 *table)
{
  u64 *tab = table + (size_t)(blockIdx.x % SHARDS) * T_WORDS;
  for (int i = threadIdx.x; i < T_WORDS; i += WG) {
    const u64 v = sh[i];
    if (!v) continue;
    if (i < T_HI) {
      const long long p = (long long)v, h = p >> 32;
      atomicAdd(&tab[T_LO + i], (u64)(uint32_t)p);
      if (h) atomicAdd(&tab[T_HI + i], (u64)h);
    } else if (i >= T_KEY && i < T_CNT) {
      atomicMax(&tab[i], v);
    } else if (i >= T_CNT) {
      atomicAdd(&tab[i], v);
    }
  }
}

// Owned columns [halo, halo + Xo) of a local array X wide, all Y rows; chunks of 256 cells of one row per workgroup step (16-byte loads,
// 1 KiB per wave and field); global index of local column halo + x in row y: y * Xg + x0 + x (below 2^32 - 1: checked by the host)
__global__ __launch_bounds__(WG) void k_diag_cells(int X, int Y, int halo, int Xo, int Xg, int x0, const float4 *__restrict__ base, const float4 *__restrict__ water,
                                                   const char4 *__restrict__ wall, u64 *__restrict__ table)
{
  __shared__ u64 sh[T_WORDS]; // (the device table's layout; T_LO holds whole bin partials, T_HI stays unused)
  for (int i = threadIdx.x; i < T_WORDS; i += WG) sh[i] = 0;
  __syncthreads();
  int cur[NQ_CELL];
  long long acc[NQ_CELL];
  uint32_t kbest[16], ibest[16];
  int cnt[7];
  uint32_t first_b = 0xFFFFFFFFu, first_w = 0xFFFFFFFFu;
#pragma unroll
  for (int q = 0; q < NQ_CELL; q++) cur[q] = 0, acc[q] = 0;
#pragma unroll
  for (int k = 0; k < 16; k++) kbest[k] = 0, ibest[k] = 0;
#pragma unroll
  for (int k = 0; k < 7; k++) cnt[k] = 0;

  const unsigned cpr = ((unsigned)Xo + WG - 1) / WG, chunks = cpr * (unsigned)Y;
  for (unsigned c = blockIdx.x; c < chunks; c += gridDim.x) {
    const unsigned y = c / cpr, x = (c - y * cpr) * WG + threadIdx.x;
    const bool in = x < (unsigned)Xo;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int wd = 1, wv = 0;
    if (in) {
      const size_t off = (size_t)y * X + halo + x;
      const float4 b = base[off], w = water[off];
      const char4 wl = wall[off];
      v[0] = b.x, v[1] = b.y, v[2] = b.z, v[3] = b.w, v[4] = w.x, v[5] = w.y, v[6] = w.z, v[7] = w.w;
      wd = wl.y, wv = wl.w;
    }
    CellOut o;
    classify(v, wd, wv, in, o);
    const uint32_t g = y * (unsigned)Xg + (unsigned)x0 + x;
#pragma unroll
    for (int q = 0; q < NQ_CELL; q++) wave_add(cur[q], acc[q], o.t[q], sh + T_LO + q * NB);
#pragma unroll
    for (int k = 0; k < 8; k++) {
      if (o.kmax[k] > kbest[k]) kbest[k] = o.kmax[k], ibest[k] = g;
      if (o.kmin[k] > kbest[8 + k]) kbest[8 + k] = o.kmin[k], ibest[8 + k] = g;
    }
#pragma unroll
    for (int k = 0; k < 7; k++) cnt[k] += o.cnt[k];
    if (o.cnt[C_NFB] && g < first_b) first_b = g;
    if (o.cnt[C_NFW] && g < first_w) first_w = g;
  }

  const bool lane0 = (threadIdx.x & 63) == 0;
#pragma unroll
  for (int q = 0; q < NQ_CELL; q++) wave_flush(cur[q], acc[q], sh + T_LO + q * NB);
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const u64 key = wave_max(kbest[k] ? ((u64)kbest[k] << 32) | (uint32_t)~ibest[k] : 0ull);
    if (lane0 && key) atomicMax(&sh[T_KEY + k], key);
  }
  {
    const u64 fb = wave_max(first_b != 0xFFFFFFFFu ? ~(u64)first_b : 0ull), fw = wave_max(first_w != 0xFFFFFFFFu ? ~(u64)first_w : 0ull);
    if (lane0 && fb) atomicMax(&sh[T_FIRST + 0], fb);
    if (lane0 && fw) atomicMax(&sh[T_FIRST + 1], fw);
  }
#pragma unroll
  for (int k = 0; k < 7; k++) {
    const long long n = wave_sum((long long)cnt[k]);
    if (lane0 && n) atomicAdd(&sh[T_CNT + k], (u64)n);
  }
  __syncthreads();
  table_push(sh, table);
}

// The droplet buffer (5 floats per droplet: pos.xy, mass.xy, density). A droplet counts when mass.x >= 0; on a slab with a partitioned
// pool (remote != nullptr) when, in addition, this rank tracks it and it lies inside the owned columns [own_lo, own_hi) -- flag 2 of
// k_pool_flags, THE record of the droplet.
__global__ __launch_bounds__(WG) void k_diag_drops(wx::Geo g, int n, int own_lo, int own_hi, const float *__restrict__ drops, const unsigned char *__restrict__ remote,
                                                   u64 *__restrict__ table)
{
  __shared__ u64 sh[T_WORDS];
  for (int i = threadIdx.x; i < T_WORDS; i += WG) sh[i] = 0;
  __syncthreads();
  int cur[2] = {0, 0};
  long long acc[2] = {0, 0};
  int n_act = 0, n_nf = 0;
  const int steps = (n + (int)(gridDim.x * WG) - 1) / (int)(gridDim.x * WG);
  for (int it = 0; it < steps; it++) {
    const long long i = ((long long)it * gridDim.x + blockIdx.x) * WG + threadIdx.x;
    bool act = false;
    float m0 = 0.f, m1 = 0.f;
    if (i < n) {
      m0 = drops[5 * (size_t)i + 2], m1 = drops[5 * (size_t)i + 3];
      act = m0 >= 0.0f;
      if (act && remote) {
        const int lc = wx::local_col(g, drops[5 * (size_t)i] / 2.0f + 0.5f);
        act = !remote[i] && lc >= own_lo && lc < own_hi;
      }
    }
    wave_add(cur[0], acc[0], term_of(m0, act), sh + T_LO + Q_DROP * NB);
    wave_add(cur[1], acc[1], term_of(m1, act), sh + T_LO + (Q_DROP + 1) * NB);
    n_act += act;
    n_nf += act && !(f32_finite(m0) && f32_finite(m1));
  }
  const bool lane0 = (threadIdx.x & 63) == 0;
  wave_flush(cur[0], acc[0], sh + T_LO + Q_DROP * NB);
  wave_flush(cur[1], acc[1], sh + T_LO + (Q_DROP + 1) * NB);
  const long long a = wave_sum((long long)n_act), f = wave_sum((long long)n_nf);
  if (lane0 && a) atomicAdd(&sh[T_CNT + C_DROPS], (u64)a);
  if (lane0 && f) atomicAdd(&sh[T_CNT + C_DROPS_NF], (u64)f);
  __syncthreads();
  table_push(sh, table);
}
#endif // __HIPCC__

// ---------------- host side: pure functions over wx_diag_raw ----------------

// the one representation of a bin's value hi * 2^32 + lo: 0 <= lo < 2^32
inline void bin_norm(int64_t &hi, uint64_t &lo)
{
  hi += (int64_t)(lo >> 32);
  lo &= 0xFFFFFFFFull;
}
inline void bin_add(wx_diag_raw *r, int q, const Term t)
{
  r->bin_lo[q][t.bin] += (uint64_t)(uint32_t)t.addend; // (a normalised low word + 2^24 addends' low words stay below 2^57)
  r->bin_hi[q][t.bin] += t.addend >> 32;
}
inline void raw_norm(wx_diag_raw *r, int q)
{
  for (int b = 0; b < NB; b++) bin_norm(r->bin_hi[q][b], r->bin_lo[q][b]);
}

// the SHARDS copies of the device table -> *out (geometry and iteration are the caller's)
inline void raw_from_table(const u64 *tab, wx_diag_raw *out)
{
  memset(out, 0, sizeof(*out));
  for (int s = 0; s < SHARDS; s++, tab += T_WORDS) {
    for (int q = 0; q < NQ; q++)
      for (int b = 0; b < NB; b++) {
        out->bin_lo[q][b] += tab[T_LO + q * NB + b];
        out->bin_hi[q][b] += (int64_t)tab[T_HI + q * NB + b];
      }
    for (int k = 0; k < 8; k++) {
      out->key_max[k] = std::max<uint64_t>(out->key_max[k], tab[T_KEY + k]);
      out->key_min[k] = std::max<uint64_t>(out->key_min[k], tab[T_KEY + 8 + k]);
    }
    for (int k = 0; k < 2; k++) out->first_nonfinite[k] = std::max<uint64_t>(out->first_nonfinite[k], tab[T_FIRST + k]);
    for (int k = 0; k < NC; k++) out->count[k] += (int64_t)tab[T_CNT + k];
  }
  for (int q = 0; q < NQ; q++) raw_norm(out, q);
}

inline int diag_accumulate(wx_diag_raw *into, int quantity, const float *values, size_t n)
{
  if (!into || quantity < 0 || quantity >= NQ || (!values && n)) return WX_E_INVALID;
  for (size_t i = 0; i < n; i++) {
    bin_add(into, quantity, term_of(values[i], true));
    if ((i & 0xFFFFF) == 0xFFFFF) raw_norm(into, quantity);
  }
  raw_norm(into, quantity);
  return WX_OK;
}

inline int diag_accumulate_cells(wx_diag_raw *r, int Xg, int Yr, int x, int y, int n, const float *base, const float *water, const int8_t *wall)
{
  if (!r || n < 0 || (n && (!base || !water || !wall))) return WX_E_INVALID;
  if (Xg < 1 || Yr < 1 || x < 0 || y < 0 || y >= Yr || (long long)x + n > Xg || (unsigned long long)Xg * (unsigned long long)Yr >= 0xFFFFFFFFull) return WX_E_INVALID;
  if (r->x_global == 0) r->x_global = Xg, r->y_rows = Yr;
  if (r->x_global != Xg || r->y_rows != Yr) return WX_E_INVALID;
  for (int i = 0; i < n; i++) {
    float v[8];
    memcpy(v, base + 4 * (size_t)i, 16);
    memcpy(v + 4, water + 4 * (size_t)i, 16);
    CellOut o;
    classify(v, wall[4 * (size_t)i + 1], wall[4 * (size_t)i + 3], true, o);
    const uint32_t g = (uint32_t)y * (uint32_t)Xg + (uint32_t)(x + i);
    for (int q = 0; q < NQ_CELL; q++)
      if (o.t[q].addend) bin_add(r, q, o.t[q]);
    for (int k = 0; k < 8; k++) {
      if (o.kmax[k]) r->key_max[k] = std::max<uint64_t>(r->key_max[k], ((uint64_t)o.kmax[k] << 32) | (uint32_t)~g);
      if (o.kmin[k]) r->key_min[k] = std::max<uint64_t>(r->key_min[k], ((uint64_t)o.kmin[k] << 32) | (uint32_t)~g);
    }
    for (int k = 0; k < 7; k++) r->count[k] += o.cnt[k];
    r->count[C_CELLS] += 1;
    if (o.cnt[C_NFB]) r->first_nonfinite[0] = std::max<uint64_t>(r->first_nonfinite[0], ~(uint64_t)g);
    if (o.cnt[C_NFW]) r->first_nonfinite[1] = std::max<uint64_t>(r->first_nonfinite[1], ~(uint64_t)g);
    if ((i & 0xFFFFF) == 0xFFFFF)
      for (int q = 0; q < NQ_CELL; q++) raw_norm(r, q);
  }
  for (int q = 0; q < NQ_CELL; q++) raw_norm(r, q);
  return WX_OK;
}

inline int diag_merge(wx_diag_raw *a, const wx_diag_raw *b)
{
  if (!a || !b) return WX_E_INVALID;
  if (a->x_global && b->x_global && (a->x_global != b->x_global || a->y_rows != b->y_rows || a->iter != b->iter)) return WX_E_INVALID;
  if (!a->x_global && b->x_global) a->x_global = b->x_global, a->y_rows = b->y_rows, a->iter = b->iter;
  for (int k = 0; k < NC; k++) a->count[k] += b->count[k];
  for (int k = 0; k < 2; k++) a->first_nonfinite[k] = std::max(a->first_nonfinite[k], b->first_nonfinite[k]);
  for (int k = 0; k < 8; k++) {
    a->key_max[k] = std::max(a->key_max[k], b->key_max[k]);
    a->key_min[k] = std::max(a->key_min[k], b->key_min[k]);
  }
  for (int q = 0; q < NQ; q++)
    for (int i = 0; i < NB; i++) {
      a->bin_hi[q][i] += b->bin_hi[q][i];
      a->bin_lo[q][i] += b->bin_lo[q][i];
      bin_norm(a->bin_hi[q][i], a->bin_lo[q][i]);
    }
  return WX_OK;
}

// 320-bit two's complement integer, little-endian words: 39 bits of addend + 15 x 16 bits of bin offset + 32 bits of count + sign = 312
struct Wide {
  uint64_t w[5] = {0, 0, 0, 0, 0};
  void add_shifted(__int128 v, int shift) // += v << shift, shift a multiple of 16 below 256
  {
    uint64_t t[5];
    const uint64_t fill = v < 0 ? ~0ull : 0ull;
    const uint64_t src[5] = {(uint64_t)v, (uint64_t)((unsigned __int128)v >> 64), fill, fill, fill};
    const int ws = shift / 64, bs = shift % 64;
    for (int i = 0; i < 5; i++) {
      const int j = i - ws;
      uint64_t x = 0;
      if (j >= 0) {
        x = src[j] << bs;
        if (bs && j >= 1) x |= src[j - 1] >> (64 - bs);
      }
      t[i] = x;
    }
    unsigned carry = 0;
    for (int i = 0; i < 5; i++) {
      const unsigned __int128 sum = (unsigned __int128)w[i] + t[i] + carry;
      w[i] = (uint64_t)sum;
      carry = (unsigned)(sum >> 64);
    }
  }
  bool bit(int i) const { return i >= 0 && ((w[i >> 6] >> (i & 63)) & 1u); }
};

// the exact value sum_b bin[b] * 2^(16 b - 150), rounded to nearest-even ONCE; +0.0 for an exact zero. Always a normal double:
// magnitudes lie between 2^-150 and 2^161.
inline double bins_to_double(const int64_t hi[NB], const uint64_t lo[NB])
{
  Wide W;
  for (int b = 0; b < NB; b++) W.add_shifted((__int128)hi[b] * ((__int128)1 << 32) + (__int128)lo[b], 16 * b);
  const bool neg = W.w[4] >> 63;
  if (neg) { // magnitude
    unsigned carry = 1;
    for (int i = 0; i < 5; i++) {
      const unsigned __int128 sum = (unsigned __int128)(~W.w[i]) + carry;
      W.w[i] = (uint64_t)sum;
      carry = (unsigned)(sum >> 64);
    }
  }
  int k = 0; // bit length
  for (int i = 319; i >= 0; i--)
    if (W.bit(i)) {
      k = i + 1;
      break;
    }
  if (k == 0) return 0.0;
  uint64_t mant = 0;
  const int low = k > 53 ? k - 53 : 0; // the mantissa is bits [low, k)
  for (int i = k - 1; i >= low; i--) mant = (mant << 1) | (W.bit(i) ? 1u : 0u);
  if (low > 0) {
    const bool half = W.bit(low - 1);
    bool sticky = false;
    for (int i = low - 2; i >= 0 && !sticky; i--) sticky = W.bit(i);
    if (half && (sticky || (mant & 1u))) mant += 1; // (2^53 after a carry is still exact in a double)
  }
  const double r = std::ldexp((double)mant, low - 150);
  return neg ? -r : r;
}

inline void key_decode(uint64_t key, bool is_min, int64_t Xg, double *val, int64_t *x, int64_t *y)
{
  if (!key) {
    *val = std::nan("");
    *x = *y = -1;
    return;
  }
  const uint32_t k = (uint32_t)(key >> 32), g = ~(uint32_t)key;
  *val = (double)float_of_ord(is_min ? ~k : k);
  *x = Xg > 0 ? (int64_t)(g % Xg) : -1;
  *y = Xg > 0 ? (int64_t)(g / Xg) : -1;
}

inline int diag_finish(const wx_diag_raw *r, wx_diag *o)
{
  if (!r || !o) return WX_E_INVALID;
  memset(o, 0, sizeof(*o));
  o->iter = r->iter;
  o->n_air = r->count[C_AIR], o->n_wall = r->count[C_WALL], o->n_marker_mismatch = r->count[C_MISMATCH], o->n_negative_water = r->count[C_NEGW];
  o->n_nonfinite_base = r->count[C_NFB], o->n_nonfinite_water = r->count[C_NFW], o->sum_vegetation = r->count[C_VEG];
  o->n_droplets_active = r->count[C_DROPS], o->n_droplets_nonfinite = r->count[C_DROPS_NF];
  int64_t *first[2][2] = {{&o->first_nonfinite_base_x, &o->first_nonfinite_base_y}, {&o->first_nonfinite_water_x, &o->first_nonfinite_water_y}};
  for (int k = 0; k < 2; k++) {
    const uint64_t g = ~r->first_nonfinite[k];
    const bool have = r->first_nonfinite[k] != 0 && r->x_global > 0;
    *first[k][0] = have ? (int64_t)(g % (uint64_t)r->x_global) : -1;
    *first[k][1] = have ? (int64_t)(g / (uint64_t)r->x_global) : -1;
  }
  for (int c = 0; c < 4; c++) {
    o->sum_base[c] = bins_to_double(r->bin_hi[c], r->bin_lo[c]);
    o->sum_water[c] = bins_to_double(r->bin_hi[4 + c], r->bin_lo[4 + c]);
    key_decode(r->key_min[c], true, r->x_global, &o->min_base[c], &o->min_base_x[c], &o->min_base_y[c]);
    key_decode(r->key_max[c], false, r->x_global, &o->max_base[c], &o->max_base_x[c], &o->max_base_y[c]);
    key_decode(r->key_min[4 + c], true, r->x_global, &o->min_water[c], &o->min_water_x[c], &o->min_water_y[c]);
    key_decode(r->key_max[4 + c], false, r->x_global, &o->max_water[c], &o->max_water_x[c], &o->max_water_y[c]);
  }
  o->sum_soil_moisture = bins_to_double(r->bin_hi[8], r->bin_lo[8]);
  o->sum_snow = bins_to_double(r->bin_hi[9], r->bin_lo[9]);
  o->sum_droplet_mass_x = bins_to_double(r->bin_hi[Q_DROP], r->bin_lo[Q_DROP]);
  o->sum_droplet_mass_y = bins_to_double(r->bin_hi[Q_DROP + 1], r->bin_lo[Q_DROP + 1]);
  return WX_OK;
}

} // namespace wxd
