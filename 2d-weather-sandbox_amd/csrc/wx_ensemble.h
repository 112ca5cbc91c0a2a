// wx_ensemble.h -- ensembles: B independent whole-domain simulations of one size that advance in ONE marching launch (+ one fix launch)
// per iteration and instantiation (included at the end of wxsim.hip, behind wx_comm.h; the entry points are declared extern "C" by
// include/wxsim.h). A member is an ordinary handle (wx_sim) owned by its ensemble as a slab is owned by its wx_group; what the ensemble
// adds is the driver below: march_wet_prepare for every member of a partition -> the members' argument blocks into a device table ->
// k_march_wet_ens / k_wet_fix_ens over the table -> march_wet_commit for every member. Results are those of wx_step on each member, bit
// for bit: the kernels' bodies are the lone kernels' own program text (wx_wet_march_body.h, wx_wet_fix_body.h). Members that carry
// droplets (wx_ensemble_create_droplets) get their particle pass the same way: one PrecipEnsSlot per member and iteration behind the
// chunk's WetEnsSlots, k_precipitation_ens / k_splat_*_ens over them behind the iteration's fix launches (wx_precip_ens.h).
//
// The table. A launch reads its members' slots while it runs, and wx_ensemble_step(e, n) enqueues n iterations without waiting, so a slot
// is never rewritten while an earlier launch may still read it: the slots of up to `chunk` iterations are filled on the host in one of
// ENS_BUFS pinned staging buffers (the members' bookkeeping -- plane rotation, display flags, droplet buffer and work-list parity -- is
// pure host work that can run ahead of the launches), copied to that buffer's own device range by ONE stream-ordered copy and consumed by
// the chunk's launches; an event behind the last of them guards the pair of buffers, and the host waits for it only when it comes round
// to the same buffer again (ENS_BUFS chunks later).

struct EnsStage; // wx_ens_frame.h
struct EnsPriorState; // wx_ens_inflate.h

struct wx_ensemble {
  std::vector<wx_sim *> member;
  int X = 0, Y = 0, device = 0;
  hipStream_t stream = nullptr;
  static constexpr int ENS_BUFS = 4;
  int chunk = 1; // iterations per staging buffer
  // a buffer holds the chunk's WetEnsSlots (iterations x batched members) directly followed by its PrecipEnsSlots (iterations x members
  // whose droplets run): one contiguous range, one copy
  char *host[ENS_BUFS] = {nullptr, nullptr, nullptr, nullptr}, *dev[ENS_BUFS] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t done[ENS_BUFS] = {nullptr, nullptr, nullptr, nullptr};
  bool pending[ENS_BUFS] = {false, false, false, false};
  int next = 0;
  int64_t iters_batched = 0, iters_solo = 0, march_launches = 0; // wx_ensemble_stats
  int64_t iters_particles = 0, particle_launches = 0;            // wx_ensemble_particle_stats
  EnsStage *stage = nullptr; // the member-axis calls: their device table of members, output buffer and pinned copies (made by the first call)
  EnsPriorState *prior = nullptr; // wx_ensemble_prior_save: one device-side snapshot per field (made by the first call)
  bool broken = false; // a step failed half-way: members' host state ran ahead of what was launched (wx_ensemble_step refuses from then on)
  std::string err;
};

static void ens_stage_release(wx_ensemble *e); // wx_ens_frame.h
static void ens_prior_release(wx_ensemble *e); // wx_ens_inflate.h

static int efail(wx_ensemble *e, int code, const char *fmt, ...)
{
  char buf[640];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (e) e->err = buf;
  else g_create_error = buf;
  return code;
}
// an error of member i: the message names the member
static int epass(wx_ensemble *e, int i, int rc)
{
  if (rc != WX_OK) {
    char head[48];
    snprintf(head, sizeof(head), "member %d: ", i);
    e->err = head + e->member[i]->err;
  }
  return rc;
}

const char *wx_ensemble_last_error(const wx_ensemble *e) { return e ? e->err.c_str() : g_create_error.c_str(); }
int wx_ensemble_count(const wx_ensemble *e) { return e ? (int)e->member.size() : 0; }
wx_sim *wx_ensemble_member(wx_ensemble *e, int i) { return e && i >= 0 && i < (int)e->member.size() ? e->member[i] : nullptr; }

void wx_ensemble_destroy(wx_ensemble *e)
{
  if (!e) return;
  int prev = 0;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(e->device);
  if (e->stream) hipStreamSynchronize(e->stream);
  for (wx_sim *s : e->member) {
    if (!s) continue;
    wx_destroy(s); // (synchronises the ensemble's stream, which is idle by now; the stream itself is destroyed last)
  }
  for (int b = 0; b < wx_ensemble::ENS_BUFS; b++) {
    if (e->done[b]) hipEventDestroy(e->done[b]);
    if (e->host[b]) hipHostFree(e->host[b]);
    hipFree(e->dev[b]);
  }
  ens_stage_release(e);
  ens_prior_release(e);
  if (e->stream) hipStreamDestroy(e->stream);
  (void)hipSetDevice(prev);
  delete e;
}

// fn: the entry point's name, for its messages
static int ensemble_create(const char *fn, int n_members, int X, int Y, int n_droplets, wx_ensemble **out)
{
  if (!out) return WX_E_INVALID;
  *out = nullptr;
  if (n_members < 1 || n_members > 65535) return efail(nullptr, WX_E_INVALID, "%s: n_members = %d (1 .. 65535: one row of the launch grid per member)", fn, n_members);
  if (X < 2 || Y < 4 || X > 65535 * 16 || Y > 65535) return efail(nullptr, WX_E_INVALID, "%s: bad geometry X=%d Y=%d", fn, X, Y);
  if (n_droplets < 0) return efail(nullptr, WX_E_INVALID, "%s: n_droplets = %d", fn, n_droplets);
  int ndev = 0;
  const hipError_t he = hipGetDeviceCount(&ndev);
  if (he != hipSuccess || ndev == 0) return efail(nullptr, WX_E_DEVICE, "no HIP device available (%s): libwxsim has no CPU fallback", hipGetErrorString(he));
  wx_ensemble *e = new wx_ensemble();
  e->X = X;
  e->Y = Y;
  (void)hipGetDevice(&e->device);
  e->member.assign(n_members, nullptr);
  int rc = WX_OK;
  if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) rc = efail(nullptr, WX_E_DEVICE, "%s: hipStreamCreate", fn);
  for (int i = 0; i < n_members && rc == WX_OK; i++) {
    wx_sim *s = nullptr;
    rc = wx_create(X, Y, n_droplets, &s);
    if (rc != WX_OK) break;
    e->member[i] = s;
    s->ens = e;
    s->stream = e->stream;
    s->place.done = true; // (the implicit placement search never runs on a member, as on a slab)
  }
  // the table: `chunk` iterations of n_members slots per buffer -- up to 16 iterations, about 4 Ki slots
  e->chunk = std::max(1, std::min(16, 4096 / n_members));
  const size_t bytes = (size_t)e->chunk * n_members * (sizeof(WetEnsSlot) + (n_droplets > 0 ? sizeof(PrecipEnsSlot) : 0));
  for (int b = 0; b < wx_ensemble::ENS_BUFS && rc == WX_OK; b++) {
    if (hipHostMalloc((void **)&e->host[b], bytes, hipHostMallocDefault) != hipSuccess || hipMalloc((void **)&e->dev[b], bytes) != hipSuccess)
      rc = efail(nullptr, WX_E_NOMEM, "%s: %zu bytes for the members' argument table", fn, bytes);
    else if (hipEventCreateWithFlags(&e->done[b], hipEventDisableTiming) != hipSuccess)
      rc = efail(nullptr, WX_E_DEVICE, "%s: hipEventCreate", fn);
  }
  if (rc != WX_OK) {
    (void)hipGetLastError();
    const std::string keep = g_create_error;
    wx_ensemble_destroy(e);
    g_create_error = keep;
    return rc;
  }
  *out = e;
  return WX_OK;
}
int wx_ensemble_create(int n_members, int X, int Y, wx_ensemble **out) { return ensemble_create("wx_ensemble_create", n_members, X, Y, 0, out); }
int wx_ensemble_create_droplets(int n_members, int X, int Y, int n_droplets, wx_ensemble **out)
{
  return ensemble_create("wx_ensemble_create_droplets", n_members, X, Y, n_droplets, out);
}

// the fix launch of a partition: workgroups per member from the largest (stale) hint word among its members -- launch_wet_fix's rule,
// with the empty-list corner shared between the members (an empty list costs its member one load)
static int ens_fix_wgs(wx_sim *const *part, size_t n)
{
  int last = 0;
  for (size_t k = 0; k < n; k++) {
    const wx_sim *m = part[k];
    const int v = m->fix.hint_dev ? *(volatile const int *)m->fix.hint_host : -1;
    if (v < 0) return 64;
    last = std::max(last, v);
  }
  return last > 0 ? std::min(512, std::max(8, last)) : std::max(1, 32 / (int)n);
}

// does a step of this member run its droplets? (wx_step_overlap's `precip`)
static bool ens_member_precip(const wx_sim *m) { return (m->p.pass_mask & WX_PASS_PRECIPITATION) && m->p.enablePrecipitation && m->n_drops > 0; }

int wx_ensemble_step(wx_ensemble *e, int n_iter)
{
  if (!e) return WX_E_INVALID;
  if (n_iter < 0) return efail(e, WX_E_INVALID, "wx_ensemble_step: n_iter < 0");
  DeviceScope dev_scope(e->member[0]);
  if (e->broken) return WX_E_STATE; // (the message of the failed step is kept)
  const int B = (int)e->member.size();
  // From the first member's bookkeeping to the last launch a failure leaves members whose planes are rotated and whose iteration counter is
  // advanced for iterations that never ran: the ensemble is marked broken, every later wx_ensemble_step returns WX_E_STATE with the
  // message of the failure, and the members' contents are undefined until they are uploaded again into a new ensemble.
  struct BreakGuard {
    wx_ensemble *e;
    bool armed;
    ~BreakGuard() { if (armed) e->broken = true; }
  } guard{e, false};
  for (int i = 0; i < B; i++)
    if (!e->member[i]->uploaded || !e->member[i]->have_params) return efail(e, WX_E_STATE, "member %d: wx_ensemble_step before wx_upload / wx_set_params", i);
  // Who is batched: the members whose iterations the marching wet kernel would run on a lone handle (default kernel set, all grid passes).
  // The instantiation is <OPT_OUT, HAS_FB, QUIET>: OPT_OUT is common (the last iteration of the call is everybody's display iteration),
  // QUIET is the member's and constant over the call, HAS_FB -- does the member hand in the feedback textures of droplets that ran in the
  // iteration before -- is the member's too and can change behind the call's first iteration (precipitation switched on or off since
  // the last step): the partitions are made per iteration, class = QUIET ? 0 : 1, + 2 with HAS_FB.
  // Of those, the members whose droplets run (pm) share the particle launches; the selection is constant over the call.
  std::vector<wx_sim *> bm, pm;
  std::vector<int> bm_index, pm_index, solo;
  for (int i = 0; i < B; i++) {
    wx_sim *m = e->member[i];
    if (step_runs_march_wet(m)) {
      bm.push_back(m);
      bm_index.push_back(i);
      if (ens_member_precip(m)) {
        pm.push_back(m);
        pm_index.push_back(i);
      }
    } else {
      solo.push_back(i);
    }
  }
  const int nB = (int)bm.size(), nP = (int)pm.size();
  guard.armed = true;
  if (n_iter > 0)
    for (int k = 0; k < nB; k++) {
      if (int rc = epass(e, bm_index[k], step_begin(bm[k], false))) return rc;
      step_begin_iterations(bm[k], n_iter);
    }
  bool check = false;
  for (wx_sim *m : bm) check = check || m->opt.check_launches;
  const PrecipEnsShape pshape = nP > 0 ? precip_ens_shape(nP, pm[0]->n_drops, pm[0]->sg.TXn * pm[0]->sg.TYn) : PrecipEnsShape{};
  static const char *const class_name[4] = {"quiet", "brush / airplane", "quiet, with feedback", "brush / airplane, with feedback"};
  struct IterPlan { // one iteration of the chunk: where its classes lie in its row of the table, and who is in them
    int count[4], groups_x[4];
    std::vector<int> order; // positions in bm, sorted by class
  };
  std::vector<WetEnsSlot> row_tmp((size_t)nB);
  std::vector<int> row_class((size_t)nB);
  for (int it0 = 0; it0 < n_iter && nB > 0; it0 += e->chunk) {
    const int n_it = std::min(e->chunk, n_iter - it0), b = e->next;
    e->next = (e->next + 1) % wx_ensemble::ENS_BUFS;
    if (e->pending[b]) { // the launches that read this buffer's device range last time round
      e->pending[b] = false;
      if (hipEventSynchronize(e->done[b]) != hipSuccess) return efail(e, WX_E_DEVICE, "wx_ensemble_step: %s", hipGetErrorString(hipGetLastError()));
      e->pending[b] = false;
    }
    // (Running the bookkeeping of iteration k + 1 before iteration k is launched is valid only while march_wet_prepare / _commit enqueue
    // NOTHING per iteration -- see the precondition at march_wet_prepare: what they do enqueue happens in a member's first prepared
    // iteration only, i.e. in front of every launch of the chunk. The one-time clear of the feedback textures of a member whose
    // precipitation was switched off is different: that member's first iteration still READS the textures (a lone handle clears behind
    // its launch), so the loop only notes the member, and the memsets are enqueued behind the launches of that iteration, below.)
    // 1. the host side of n_it iterations of every batched member: its WetEnsSlot of iteration `it` is wet[it * nB + position in the
    // iteration's class order], its PrecipEnsSlot prc[it * nP + position in pm]
    const size_t wet_bytes = (size_t)n_it * nB * sizeof(WetEnsSlot), prc_bytes = (size_t)n_it * nP * sizeof(PrecipEnsSlot);
    WetEnsSlot *const wet = (WetEnsSlot *)e->host[b];
    PrecipEnsSlot *const prc = (PrecipEnsSlot *)(e->host[b] + wet_bytes);
    const WetEnsSlot *const wet_dev = (const WetEnsSlot *)e->dev[b];
    const PrecipEnsSlot *const prc_dev = (const PrecipEnsSlot *)(e->dev[b] + wet_bytes);
    std::vector<IterPlan> plan((size_t)n_it);
    std::vector<std::pair<int, wx_sim *>> clear_behind; // (iteration of the chunk, member): feedback textures to clear behind its launches
    for (int it = 0; it < n_it; it++) {
      const bool opt_out = it0 + it == n_iter - 1;
      IterPlan &pl = plan[(size_t)it];
      for (int c = 0; c < 4; c++) pl.count[c] = 0, pl.groups_x[c] = 8;
      int kp = 0;
      for (int k = 0; k < nB; k++) {
        wx_sim *m = bm[k];
        const bool precip = ens_member_precip(m);
        WetIter wi;
        if (int rc = epass(e, bm_index[k], march_wet_prepare(m, opt_out, precip, wi, B))) return rc;
        const WetLaunch &w = m->wet_shape;
        WetEnsSlot &sl = row_tmp[(size_t)k];
        memset(&sl, 0, sizeof(sl));
        const WetFixList fix = m->fix.wet(&m->state->fastest_bits);
        sl.ka.ctx = m->full_ctx;
        sl.ka.iterNum = wi.iter;
        sl.ka.in = wi.in;
        sl.ka.out = wi.out;
        sl.ka.fix = fix;
        sl.ka.n_strips = sl.ka.n_strips_all = sl.ka.split_at = w.n_strips; // the whole width, one strip range, no priority (launch_march_wet's defaults)
        sl.ka.segs = w.segs;
        sl.ka.vx = vx_track(m);
        sl.overflow = &m->state->fix_overflow;
        const int c = (wi.quiet ? 0 : 1) + (wi.in.fb != nullptr ? 2 : 0);
        row_class[(size_t)k] = c;
        pl.count[c]++;
        pl.groups_x[c] = std::max(pl.groups_x[c], ens_member_groups(w));
        m->run.fix_check = true;
        march_wet_commit(m);
        m->run.ran_fused = true;
        // behind the grid passes, as in wx_step_overlap: the droplets' buffers by `even`, then the particle pass or the one-time clear
        const int src = m->run.even ? 0 : 1, dst = m->run.even ? 1 : 0;
        m->run.even = !m->run.even;
        if (precip) {
          PrecipEnsSlot &ps = prc[(size_t)it * nP + kp++];
          memset(&ps, 0, sizeof(ps));
          ps.ctx = m->full_ctx;
          ps.iterNum = (float)m->run.iter;
          ps.n_drops = m->n_drops;
          ps.drops_in = m->drops[src];
          ps.drops_out = m->drops[dst];
          ps.base_in = m->base[0]; // (the marching kernel's path: velocity from the post-pressure base, temperature through tdisp)
          ps.water_in = m->water[1];
          ps.t_in = m->tdisp;
          ps.wall_in = m->wall[0];
          ps.st = m->state;
          ps.sg = m->sg;
          ps.fb = m->fb;
          ps.dep = m->dep;
          ps.det = DetSplat{m->opt.splat_order ? m->det_key[0] : nullptr, m->det_val};
          ps.par = m->run.splat_par;
          ps.seam = m->seam;
          ps.la = LightningArgs{ps.iterNum, (int)(m->run.iter % 600 == 0), 1, 0, m->fb, m->state};
          m->run.splat_par ^= 1;
          m->run.drop_cur = dst;
          m->run.fb_dirty = true;
        } else if (m->run.fb_dirty) { // particles were switched off: the clear goes behind this iteration's launches
          clear_behind.emplace_back(it, m);
          m->run.fb_dirty = false;
        }
        m->run.iter++;
      }
      // the row of the table, class by class
      int at[4], pos = 0;
      for (int c = 0; c < 4; c++) at[c] = pos, pos += pl.count[c];
      pl.order.assign((size_t)nB, 0);
      for (int k = 0; k < nB; k++) {
        const int p = at[row_class[(size_t)k]]++;
        wet[(size_t)it * nB + p] = row_tmp[(size_t)k];
        pl.order[(size_t)p] = k;
      }
    }
    // 2. one copy for the chunk, 3. its launches: per iteration and non-empty class one marching launch and one fix launch, then the
    // particle launches over the members whose droplets run
    if (hipMemcpyAsync(e->dev[b], e->host[b], wet_bytes + prc_bytes, hipMemcpyHostToDevice, e->stream) != hipSuccess)
      return efail(e, WX_E_DEVICE, "wx_ensemble_step: table copy: %s", hipGetErrorString(hipGetLastError()));
    size_t clear_next = 0;
    for (int it = 0; it < n_it; it++) {
      const bool opt_out = it0 + it == n_iter - 1;
      const IterPlan &pl = plan[(size_t)it];
      int pos = 0;
      for (int c = 0; c < 4; c++) {
        const int n = pl.count[c], first = pos;
        pos += n;
        if (n == 0) continue;
        std::vector<wx_sim *> part((size_t)n);
        for (int k = 0; k < n; k++) part[(size_t)k] = bm[(size_t)pl.order[(size_t)(first + k)]];
        const WetEnsSlot *table = wet_dev + (size_t)it * nB + first;
        launch_march_wet_ens(table, n, pl.groups_x[c], opt_out, (c & 2) != 0, (c & 1) == 0, e->stream);
        launch_wet_fix_ens(table, n, ens_fix_wgs(part.data(), part.size()), opt_out, e->stream);
        e->march_launches++;
        hipError_t he = hipGetLastError();
        if (he == hipSuccess && check) he = hipStreamSynchronize(e->stream); // (WX_OPT_CHECK_LAUNCHES on any batched member)
        if (he != hipSuccess) {
          const int i_lo = bm_index[(size_t)pl.order[(size_t)first]], i_hi = bm_index[(size_t)pl.order[(size_t)(first + n - 1)]];
          const int rc = efail(e, WX_E_DEVICE, "wx_ensemble_step: march_wet over members %d .. %d (%d %s members, iteration %d of the call): %s", i_lo, i_hi, n, class_name[c],
                               it0 + it, hipGetErrorString(he));
          for (wx_sim *m : part) m->err = e->err;
          return rc;
        }
      }
      if (nP > 0) {
        const PrecipEnsSlot *table = prc_dev + (size_t)it * nP;
        launch_precipitation_ens(table, nP, pshape, e->stream);
        e->particle_launches++;
        for (wx_sim *m : pm) { // deterministic order: the member's own stable sort and run sums (wx_precip_ens.h), between the shared launches
          if (!m->opt.splat_order) continue;
          if (hipcub::DeviceRadixSort::SortPairs(m->det_tmp, m->det_tmp_bytes, m->det_key[0], m->det_key[1], m->det_idx[0], m->det_idx[1], m->n_drops, 0, 31, e->stream) != hipSuccess)
            break; // (reported below)
          hipLaunchKernelGGL(k_splat_runs, dim3((m->n_drops + 255) / 256), dim3(256), 0, e->stream, m->n_drops, m->det_key[1], m->det_idx[1], m->det_val, m->sg, m->state);
          e->particle_launches += 2;
        }
        launch_splat_ens(table, nP, pshape, e->stream);
        e->particle_launches += 3;
        hipError_t he = hipGetLastError();
        if (he == hipSuccess && check) he = hipStreamSynchronize(e->stream);
        if (he != hipSuccess) {
          const int rc = efail(e, WX_E_DEVICE, "wx_ensemble_step: particle pass over members %d .. %d (%d members, iteration %d of the call): %s", pm_index.front(), pm_index.back(),
                               nP, it0 + it, hipGetErrorString(he));
          for (wx_sim *m : pm) m->err = e->err;
          return rc;
        }
      }
      for (; clear_next < clear_behind.size() && clear_behind[clear_next].first == it; clear_next++) clear_particle_textures_enqueue(clear_behind[clear_next].second);
    }
    if (hipEventRecord(e->done[b], e->stream) != hipSuccess) return efail(e, WX_E_DEVICE, "wx_ensemble_step: hipEventRecord: %s", hipGetErrorString(hipGetLastError()));
    e->pending[b] = true; // (only with the event recorded behind the buffer's last reader)
    e->iters_batched += (int64_t)n_it * nB;
    e->iters_particles += (int64_t)n_it * nP;
  }
  for (wx_sim *m : bm) step_end(m, n_iter, false);
  // the others run their own path on the ensemble's stream, in member order
  for (int i : solo) {
    if (int rc = epass(e, i, wx_step(e->member[i], n_iter))) return rc;
    e->iters_solo += n_iter;
  }
  if (hipGetLastError() != hipSuccess) return efail(e, WX_E_DEVICE, "wx_ensemble_step: launch failed");
  guard.armed = false;
  return WX_OK;
}

int wx_ensemble_sync(wx_ensemble *e)
{
  if (!e) return WX_E_INVALID;
  DeviceScope dev_scope(e->member[0]);
  int first = WX_OK;
  for (size_t i = 0; i < e->member.size(); i++) { // every member is looked at: its report is consumed here as by its own blocking call
    const int rc = wx_sync(e->member[i]);
    if (rc != WX_OK && first == WX_OK) first = epass(e, (int)i, rc);
  }
  return first;
}

// every member's passes are enqueued first, then collected (as wx_group_diagnostics does for its slabs)
int wx_ensemble_diagnostics(wx_ensemble *e, wx_diag *out)
{
  if (!e || !out) return WX_E_INVALID;
  DeviceScope dev_scope(e->member[0]);
  for (size_t i = 0; i < e->member.size(); i++)
    if (int rc = epass(e, (int)i, diag_enqueue(e->member[i]))) return rc;
  for (size_t i = 0; i < e->member.size(); i++) {
    wx_diag_raw raw;
    if (int rc = epass(e, (int)i, diag_complete(e->member[i], &raw))) return rc;
    if (int rc = wxd::diag_finish(&raw, out + i)) return rc;
  }
  return WX_OK;
}

int wx_ensemble_stats(wx_ensemble *e, int64_t *member_iters_batched, int64_t *member_iters_solo, int64_t *march_launches)
{
  if (!e) return WX_E_INVALID;
  if (member_iters_batched) *member_iters_batched = e->iters_batched;
  if (member_iters_solo) *member_iters_solo = e->iters_solo;
  if (march_launches) *march_launches = e->march_launches;
  return WX_OK;
}

int wx_ensemble_particle_stats(wx_ensemble *e, int64_t *member_iters_particles_batched, int64_t *particle_launches)
{
  if (!e) return WX_E_INVALID;
  if (member_iters_particles_batched) *member_iters_particles_batched = e->iters_particles;
  if (particle_launches) *particle_launches = e->particle_launches;
  return WX_OK;
}
