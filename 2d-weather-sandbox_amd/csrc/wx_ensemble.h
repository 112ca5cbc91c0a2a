// wx_ensemble.h -- ensembles: B independent whole-domain simulations of one size that advance in ONE marching launch (+ one fix launch)
// per iteration and instantiation (included at the end of wxsim.hip, behind wx_comm.h; the entry points are declared extern "C" by
// include/wxsim.h). A member is an ordinary handle (wx_sim) owned by its ensemble as a slab is owned by its wx_group; what the ensemble
// adds is the driver below: march_wet_prepare for every member of a partition -> the members' argument blocks into a device table ->
// k_march_wet_ens / k_wet_fix_ens over the table -> march_wet_commit for every member. Results are those of wx_step on each member, bit
// for bit: the kernels' bodies are the lone kernels' own program text (wx_wet_march_body.h, wx_wet_fix_body.h).
//
// The table. A launch reads its members' slots while it runs, and wx_ensemble_step(e, n) enqueues n iterations without waiting, so a slot
// is never rewritten while an earlier launch may still read it: the slots of up to `chunk` iterations are filled on the host in one of
// ENS_BUFS pinned staging buffers (the members' bookkeeping -- plane rotation, display flags -- is pure host work that can run ahead of the
// launches), copied to that buffer's own device range by ONE stream-ordered copy and consumed by the chunk's launches; an event behind
// the last of them guards the pair of buffers, and the host waits for it only when it comes round to the same buffer again (ENS_BUFS
// chunks later).

struct wx_ensemble {
  std::vector<wx_sim *> member;
  int X = 0, Y = 0, device = 0;
  hipStream_t stream = nullptr;
  static constexpr int ENS_BUFS = 4;
  int chunk = 1; // iterations per staging buffer
  WetEnsSlot *host[ENS_BUFS] = {nullptr, nullptr, nullptr, nullptr}, *dev[ENS_BUFS] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t done[ENS_BUFS] = {nullptr, nullptr, nullptr, nullptr};
  bool pending[ENS_BUFS] = {false, false, false, false};
  int next = 0;
  int64_t iters_batched = 0, iters_solo = 0, march_launches = 0; // wx_ensemble_stats
  bool broken = false; // a step failed half-way: members' host state ran ahead of what was launched (wx_ensemble_step refuses from then on)
  std::string err;
};

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
  if (e->stream) hipStreamDestroy(e->stream);
  (void)hipSetDevice(prev);
  delete e;
}

int wx_ensemble_create(int n_members, int X, int Y, wx_ensemble **out)
{
  if (!out) return WX_E_INVALID;
  *out = nullptr;
  if (n_members < 1 || n_members > 65535) return efail(nullptr, WX_E_INVALID, "wx_ensemble_create: n_members = %d (1 .. 65535: one row of the launch grid per member)", n_members);
  if (X < 2 || Y < 4 || X > 65535 * 16 || Y > 65535) return efail(nullptr, WX_E_INVALID, "wx_ensemble_create: bad geometry X=%d Y=%d", X, Y);
  int ndev = 0;
  const hipError_t he = hipGetDeviceCount(&ndev);
  if (he != hipSuccess || ndev == 0) return efail(nullptr, WX_E_DEVICE, "no HIP device available (%s): libwxsim has no CPU fallback", hipGetErrorString(he));
  wx_ensemble *e = new wx_ensemble();
  e->X = X;
  e->Y = Y;
  (void)hipGetDevice(&e->device);
  e->member.assign(n_members, nullptr);
  int rc = WX_OK;
  if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) rc = efail(nullptr, WX_E_DEVICE, "wx_ensemble_create: hipStreamCreate");
  for (int i = 0; i < n_members && rc == WX_OK; i++) {
    wx_sim *s = nullptr;
    rc = wx_create(X, Y, 0, &s);
    if (rc != WX_OK) break;
    e->member[i] = s;
    s->ens = e;
    s->stream = e->stream;
    s->place.done = true; // (the implicit placement search never runs on a member, as on a slab)
  }
  // the table: `chunk` iterations of n_members slots per buffer -- up to 16 iterations, about 4 Ki slots
  e->chunk = std::max(1, std::min(16, 4096 / n_members));
  const size_t bytes = (size_t)e->chunk * n_members * sizeof(WetEnsSlot);
  for (int b = 0; b < wx_ensemble::ENS_BUFS && rc == WX_OK; b++) {
    if (hipHostMalloc((void **)&e->host[b], bytes, hipHostMallocDefault) != hipSuccess || hipMalloc((void **)&e->dev[b], bytes) != hipSuccess)
      rc = efail(nullptr, WX_E_NOMEM, "wx_ensemble_create: %zu bytes for the members' argument table", bytes);
    else if (hipEventCreateWithFlags(&e->done[b], hipEventDisableTiming) != hipSuccess)
      rc = efail(nullptr, WX_E_DEVICE, "wx_ensemble_create: hipEventCreate");
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

// the fix launch of a partition: workgroups per member from the largest (stale) hint word among its members -- launch_wet_fix's rule,
// with the empty-list corner shared between the members (an empty list costs its member one load)
static int ens_fix_wgs(const std::vector<wx_sim *> &part)
{
  int last = 0;
  for (const wx_sim *m : part) {
    const int v = m->fix.hint_dev ? *(volatile const int *)m->fix.hint_host : -1;
    if (v < 0) return 64;
    last = std::max(last, v);
  }
  return last > 0 ? std::min(512, std::max(8, last)) : std::max(1, 32 / (int)part.size());
}

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
  // Who is batched: the members whose iterations the marching wet kernel would run on a lone handle (default kernel set, all grid passes;
  // members carry no droplets). The instantiation is <OPT_OUT, QUIET>: OPT_OUT is common (the last iteration of the call is everybody's
  // display iteration), QUIET is the member's -- both are constant over the call, so the partitions are too.
  std::vector<wx_sim *> part[2]; // [0]: QUIET, [1]: the general instantiation (a brush or an airplane event)
  std::vector<int> part_index[2], solo;
  for (int i = 0; i < B; i++) {
    wx_sim *m = e->member[i];
    if (step_runs_march_wet(m)) {
      const int q = march_wet_quiet(m) ? 0 : 1;
      part[q].push_back(m);
      part_index[q].push_back(i);
    } else {
      solo.push_back(i);
    }
  }
  const int nB = (int)(part[0].size() + part[1].size());
  guard.armed = true;
  if (n_iter > 0)
    for (int q = 0; q < 2; q++)
      for (size_t k = 0; k < part[q].size(); k++) {
        wx_sim *m = part[q][k];
        if (int rc = epass(e, part_index[q][k], step_begin(m, false))) return rc;
        step_begin_iterations(m, n_iter);
      }
  bool check = false;
  for (int q = 0; q < 2; q++)
    for (wx_sim *m : part[q]) check = check || m->opt.check_launches;
  for (int it0 = 0; it0 < n_iter && nB > 0; it0 += e->chunk) {
    const int n_it = std::min(e->chunk, n_iter - it0), b = e->next;
    e->next = (e->next + 1) % wx_ensemble::ENS_BUFS;
    if (e->pending[b]) { // the launches that read this buffer's device range last time round
      e->pending[b] = false;
      if (hipEventSynchronize(e->done[b]) != hipSuccess) return efail(e, WX_E_DEVICE, "wx_ensemble_step: %s", hipGetErrorString(hipGetLastError()));
      e->pending[b] = false;
    }
    // (Running the bookkeeping of iteration k + 1 before iteration k is launched is valid only while march_wet_prepare / _commit and
    // clear_particle_textures enqueue NOTHING per iteration -- see the precondition at march_wet_prepare: what they do enqueue happens in
    // a member's first prepared iteration only, i.e. in front of every launch of the chunk.)
    // 1. the host side of n_it iterations of every batched member: its slot of iteration `it` is host[b][it * nB + position in its partition]
    std::vector<int> groups_x((size_t)n_it * 2, 8);
    for (int it = 0; it < n_it; it++) {
      const bool opt_out = it0 + it == n_iter - 1;
      WetEnsSlot *row = e->host[b] + (size_t)it * nB;
      for (int q = 0; q < 2; q++) {
        WetEnsSlot *slots = row + (q ? part[0].size() : 0);
        for (size_t k = 0; k < part[q].size(); k++) {
          wx_sim *m = part[q][k];
          WetIter wi;
          if (int rc = epass(e, part_index[q][k], march_wet_prepare(m, opt_out, false, wi, B))) return rc;
          const WetLaunch &w = m->wet_shape;
          WetEnsSlot &sl = slots[k];
          memset(&sl, 0, sizeof(sl));
          const WetFixList fix = m->fix.wet(&m->state->fastest_bits);
          sl.ka.ctx = m->full_ctx;
          sl.ka.iterNum = wi.iter;
          sl.ka.in = wi.in;
          sl.ka.out = wi.out;
          sl.ka.fix[0] = sl.ka.fix[1] = fix;
          sl.ka.n_strips = sl.ka.n_strips_all = sl.ka.split_at = w.n_strips; // the whole width, one strip range, no order (launch_march_wet's defaults)
          sl.ka.segs = w.segs;
          sl.ka.vx = vx_track(m);
          sl.overflow = &m->state->fix_overflow;
          groups_x[(size_t)it * 2 + q] = std::max(groups_x[(size_t)it * 2 + q], ens_member_groups(w));
          m->run.fix_check = true;
          march_wet_commit(m);
          m->run.ran_fused = true;
          m->run.even = !m->run.even;
          clear_particle_textures(m);
          m->run.iter++;
        }
      }
    }
    // 2. one copy for the chunk, 3. its launches: per iteration and non-empty partition one marching launch and one fix launch
    if (hipMemcpyAsync(e->dev[b], e->host[b], (size_t)n_it * nB * sizeof(WetEnsSlot), hipMemcpyHostToDevice, e->stream) != hipSuccess)
      return efail(e, WX_E_DEVICE, "wx_ensemble_step: table copy: %s", hipGetErrorString(hipGetLastError()));
    for (int it = 0; it < n_it; it++) {
      const bool opt_out = it0 + it == n_iter - 1;
      for (int q = 0; q < 2; q++) {
        if (part[q].empty()) continue;
        const WetEnsSlot *table = e->dev[b] + (size_t)it * nB + (q ? part[0].size() : 0);
        launch_march_wet_ens(table, (int)part[q].size(), groups_x[(size_t)it * 2 + q], opt_out, q == 0, e->stream);
        launch_wet_fix_ens(table, (int)part[q].size(), ens_fix_wgs(part[q]), opt_out, e->stream);
        e->march_launches++;
        hipError_t he = hipGetLastError();
        if (he == hipSuccess && check) he = hipStreamSynchronize(e->stream); // (WX_OPT_CHECK_LAUNCHES on any member of the partition)
        if (he != hipSuccess) {
          const int rc = efail(e, WX_E_DEVICE, "wx_ensemble_step: march_wet over members %d .. %d (%zu %s members, iteration %d of the call): %s", part_index[q].front(),
                               part_index[q].back(), part[q].size(), q == 0 ? "quiet" : "brush / airplane", it0 + it, hipGetErrorString(he));
          for (wx_sim *m : part[q]) m->err = e->err;
          return rc;
        }
      }
    }
    if (hipEventRecord(e->done[b], e->stream) != hipSuccess) return efail(e, WX_E_DEVICE, "wx_ensemble_step: hipEventRecord: %s", hipGetErrorString(hipGetLastError()));
    e->pending[b] = true; // (only with the event recorded behind the buffer's last reader)
    e->iters_batched += (int64_t)n_it * nB;
  }
  for (int q = 0; q < 2; q++)
    for (wx_sim *m : part[q]) step_end(m, n_iter, false);
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
