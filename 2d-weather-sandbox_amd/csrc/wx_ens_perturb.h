// wx_ens_perturb.h -- the members of an ensemble made different on the device (include/wxsim.h: wx_ens_perturb, wx_ensemble_perturb,
// wx_ens_perturb_cells): per member, cell and channel a smooth pseudo-random number r in [-1, 1) -- bilinear interpolation of hashed
// values on a lattice of `scale` cells, a pure function of (seed, member index, channel, absolute cell) -- is added to the value
// (v + a r) or scales it (v (1 + a r)), the result is clamped, and wall cells, non-finite values and results that would not be finite are
// left alone bit for bit. Included at the end of wxsim.hip behind wx_ens_stat.h (the entry points are declared extern "C" by
// include/wxsim.h).
//
// THE per-cell function is wxp::perturb_cell (wx_ens_perturb_cell.h), __host__ __device__: the kernel and the host entry point run the same program text, in
// double, with floating-point contraction switched off inside every function that rounds (as wx_ens_stat.h does), so libwxsim.so,
// libwxsim_fast.so, the device and the host give the same bits. int -> double and double -> float conversions and double division are
// correctly rounded on the device and on the host alike.
//
// The kernel: one lane per cell, the 64 lanes of a wave take 64 consecutive x of one row; per lane and member one 16-byte load of the
// field's texel, the 4-byte wall texel, one 16-byte store -- 36 B per member-cell. Waves grid-stride over the (member, row, 64-column
// chunk) triples with a capped grid. The selected members' {field, wall, index} triples come from the device table of wx_ens_frame.h
// (wxe::Member), read through the constant address space at wave-uniform addresses. The node values -- up to four integer hash chains
// of four hashes per channel -- are computed between the loads and the store; a channel with amplitude 0 computes none. No LDS, no
// atomics; lanes outside the rectangle and cells that are left alone do not store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/wxsim.h"
#include "wx_ens_frame.h"
#include "wx_ens_perturb_cell.h"

namespace wxp {

struct Args {
  int X;             // cells per row of the members' arrays
  int x0, y0, w, h;  // the rectangle
  int n_sel;
  const wxe::Member *tab; // n_sel entries (field: written in place)
  Noise noise;
};

enum { WG = 256, WAVES = WG / 64, MAX_WGS = 4096 };

#if defined(__HIPCC__)
__global__ __launch_bounds__(WG) void k_ens_perturb(const Args a)
{
  const wxe::WaveOfGrid wg = wxe::wave_of_grid(WAVES);
  const unsigned long long items = (unsigned long long)(wxe::chunks_per_row(a.w) * (unsigned)a.h) * (unsigned)a.n_sel;
  const wxe::CTab tab = wxe::const_table(a.tab);
  for (unsigned long long it = wg.wave; it < items; it += wg.n_waves) {
    unsigned k;
    const wxe::Chunk at = wxe::member_chunk_at(it, wg.lane, a.x0, a.y0, a.w, a.h, k);
    if (!at.valid) continue;
    const int gx = at.gx, gy = at.gy;
    const size_t off = wxe::texel_at(a.X, gx, gy);
    const wxe::f32x4 v = wxe::ld_field(tab + k, off);
    const int wd = wxe::ld_wall_dist(tab + k, off);
    float f[4] = {v.x, v.y, v.z, v.w};
    if (perturb_cell(a.noise, tab[k].index, gx, gy, wd, f)) {
      wxe::f32x4 o;
      o.x = f[0], o.y = f[1], o.z = f[2], o.w = f[3];
      st_field(tab + k, off, o);
    }
  }
}
#endif // __HIPCC__

} // namespace wxp

int wx_ens_perturb_cells(const wx_ens_perturb *p, int X, int Y, int n_members, float *const *field, const int8_t *const *wall, const uint8_t *member_mask)
{
  return wxp::perturb_cells(p, X, Y, n_members, field, wall, member_mask);
}

// What a perturbation means to a member's bookkeeping: a host write through wx_device_ptr (same rules), plus what a write to the WATER
// field means to the water-free dry state. Enqueues on the member's (= the ensemble's) stream; never blocks.
static int ens_perturb_prepare(wx_sim *m, int field)
{
  const void *ptr;
  int ch, el;
  if (m->run.ran_fused && m->run.disp_lazy) { // baseTexture_1 on demand is assembled from base_0 / wall_0: whole, now, and a stored texture from here on
    if (field_info(m, WX_FIELD_BASE_DISP, &ptr, &ch, &el)) return WX_E_DEVICE;
    m->run.disp_lazy = false;
  }
  // a pending waterTexture_0 is made now, in stream order in front of the write: the display-side fields of the last display iteration
  // are all stored textures once a member's state has been edited
  if (int rc = materialize_water0(m)) return rc;
  if (field == WX_FIELD_BASE_CUR) m->vx.untracked = true; // velocities written: the next |vx| scan looks at the state
  if (field == WX_FIELD_WATER_CUR) m->run.water_trivial = m->run.local_water_free = m->run.halo_base_only = false; // no water-free dry kernel on a perturbed water field
  return WX_OK;
}

int wx_ensemble_perturb(wx_ensemble *e, const wx_ens_perturb *p, const uint8_t *member_mask)
{
  static const char *const call = "wx_ensemble_perturb";
  if (!e || !p) return WX_E_INVALID;
  // the arguments first: nothing below this block is reached with a bad one, and nothing in it touches the device
  const char *why;
  if (int rc = wxp::check_desc(p, e->X, e->Y, &why)) return efail(e, rc, "wx_ensemble_perturb: %s", why);
  const std::vector<int> sel = ens_select(e, member_mask);
  if (sel.empty()) return efail(e, WX_E_INVALID, "wx_ensemble_perturb: the member mask selects nobody");
  if (int rc = ens_require_uploaded(e, call, sel)) return rc;

  EnsCall c(e, call, K_ENS_PERTURB);
  if (int rc = ens_begin(c, (int)sel.size(), 16)) return rc;
  for (int i : sel)
    if (int rc = epass(e, i, ens_perturb_prepare(e->member[i], p->field))) return rc;
  ens_table_field(c, sel, p->field);

  wxp::Args a;
  memset(&a, 0, sizeof(a));
  a.X = e->X, a.x0 = p->x, a.y0 = p->y, a.w = p->w, a.h = p->h, a.n_sel = (int)sel.size();
  a.tab = c.st->tab_dev;
  a.noise = wxp::noise_of(*p, e->X);

  const unsigned wgs = ens_wgs_wave_per_item((unsigned long long)ens_chunks(p->w, p->h) * sel.size(), wxp::WAVES, wxp::MAX_WGS);
  ens_launch(c, K_ENS_PERTURB, [&] { hipLaunchKernelGGL(wxp::k_ens_perturb, dim3(wgs), dim3(wxp::WG), 0, e->stream, a); });
  return ens_finish(c);
}
