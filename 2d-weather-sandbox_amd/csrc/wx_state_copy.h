// wx_state_copy.h -- a complete device-side clone of one handle's simulation into another (include/wxsim.h: wx_copy_state,
// wx_ensemble_broadcast). Included at the end of wxsim.hip behind wx_ensemble.h (the entry points are declared extern "C" by
// include/wxsim.h).
//
// Two handles of one geometry and droplet count were given their storage by the same sequence of dalloc calls in wx_create_slab: the same
// blocks of the same sizes, the same registered pointers in the same order (Storage::created_*; what WX_OPT_SPLAT_ORDER adds later lies
// behind that and stays the handle's own). The clone is therefore wx_tune_placement's machinery across handles: the blocks copied one to
// one (copy_set), src's registered pointers re-expressed as (block, offset) in dst's blocks (snap_take / snap_put: the ping-pongs have
// rotated them), RunState assigned, a fresh FullCtx written for dst -- plus what an iteration reads that lies OUTSIDE the blocks or
// outside RunState. The audit, item by item (the declarations in wxsim.hip say "not snapshotted" where that is so):
//   wx_params / Geo / Uni / have_params   copied (host structs; the sounding arrays and initial_T are in the blocks). FullCtx holds device
//                                         pointers into the set it was written for: written anew for dst behind the block copy.
//   Water0 (even, uni, initT_saved)       copied: a pending waterTexture_0 stays pending in dst and is made there when asked for, from the
//                                         copied inputs with the copied parameters. The saved initial_T row (hipMalloc'ed by the first
//                                         wx_set_params that needed it) is copied if src holds one. The scratch planes stay dst's own:
//                                         written before they are read by every materialize_water0.
//   FixList fix, Split::edge_fix          nothing crosses a sync: the fix pass leaves count and ticket at 0, the cells are consumed by the
//                                         launch that recorded them. The hint word and words[told] only size the next fix launch (any
//                                         size is correct: the pass grid-strides); dst keeps its own, consistent with each other, and
//                                         its own capacity (WX_OPT_FIX_CAP is an option: options are dst's).
//   FixList pair, pair_epoch              the same: count / ticket / barriers are 0 between launches, the redo epoch is compared with
//                                         dst's own pair_epoch only. The two statistics words (wx_pair_stats) describe dst's launches:
//                                         zeroed.
//   SplatGrid (acc, dirty, fb_zero, work) in the blocks; the work-list parity is RunState::splat_par.
//   det_* (WX_OPT_SPLAT_ORDER)            records of ONE iteration, written by k_precipitation and consumed by the sort and k_splat_runs
//                                         of the same iteration; det_idx[0] is the constant 0 .. n-1. dst keeps its own (it may have
//                                         none).
//   DevState                              in the blocks. The words that describe a handle's own launches or exchanges -- fastest_bits,
//                                         vx_max_bits, cone_violation, ghost_nontrivial, pool_overflow, pool_seen_max, fix_overflow --
//                                         are zeroed in dst as wx_upload zeroes them; lightning, inactiveDroplets, mailbox_w stay.
//   VxWatch                               as after wx_upload: stale (the next |vx| scan looks at the state itself), nothing measured.
//   wet_shape / RunState::wet_shape_valid the cached launch shape was made for dst's old state and options, and src's flag says nothing
//                                         about dst's cache (a dst that never stepped has none): invalidated. air_from_row is a property
//                                         of the terrain: src's.
//   RunState::emit_uni, emit_lit          in RunState. The emitted-light image, fb_rgba and the diagnostics table are made by their readers.
//   RunState::fix_check                   cleared: src's report was consumed in front of the copy, dst's old one describes a state that
//                                         is gone.
// Not copied by design: Options, streams, Profile, Placement, ensemble membership, Transport / Split / Pool (whole-domain handles only).
#pragma once

namespace {

struct StateCopyPlan { // what state_copy_enqueue leaves alive until the stream has been waited for
  FullCtx fc;
};

// geometry, layout and call-sequence checks of one (dst, src) pair; touches no device
int state_copy_check(wx_sim *dst, const wx_sim *src, const char *fn)
{
  if (src->halo != 0 || dst->halo != 0 || src->X != src->Xg || dst->X != dst->Xg) return fail(dst, WX_E_INVALID, "%s: whole-domain handles only (a slab's ghost columns and pool bookkeeping belong to its ring)", fn);
  if (src->X != dst->X || src->Y != dst->Y || src->n_drops != dst->n_drops)
    return fail(dst, WX_E_INVALID, "%s: %d x %d cells with %d droplets into %d x %d cells with %d droplets", fn, src->X, src->Y, src->n_drops, dst->X, dst->Y, dst->n_drops);
  if (src->device != dst->device) return fail(dst, WX_E_INVALID, "%s: the handles live on devices %d and %d", fn, src->device, dst->device);
  if (!src->uploaded) return fail(dst, WX_E_STATE, "%s: src was never uploaded", fn);
  if (!src->have_params) return fail(dst, WX_E_STATE, "%s: src has no parameters (wx_set_params)", fn);
  const Storage &a = src->store, &b = dst->store;
  bool same = a.created_blocks == b.created_blocks && a.created_slots == b.created_slots && a.created_small_used == b.created_small_used && a.created_blocks > 0 &&
              (int)a.blocks.size() >= a.created_blocks && (int)b.blocks.size() >= b.created_blocks;
  for (int i = 1; same && i < a.created_blocks; i++) same = a.blocks[i].bytes == b.blocks[i].bytes;
  if (!same) return fail(dst, WX_E_STATE, "%s: the two handles' storage was not laid out alike", fn);
  return WX_OK;
}

// The clone itself, enqueued on `st`: the caller has ordered `st` behind everything pending on both handles and waits for it before
// `plan` goes away. Host bookkeeping of dst is final when this returns.
int state_copy_enqueue(wx_sim *dst, wx_sim *src, hipStream_t st, StateCopyPlan &plan)
{
  const Storage &a = src->store;
  Storage &b = dst->store;
  if (dst->copy_in_flight) HIPCHK(dst, hipStreamWaitEvent(st, dst->ev_copy_done, 0)); // a streamed frame still reads dst's display fields
  // 1. the blocks wx_create made: blocks[0] as far as wx_create filled it, the planes whole
  for (int i = 0; i < a.created_blocks; i++) {
    const size_t bytes = i == 0 ? (a.one_arena ? a.blocks[0].bytes : a.created_small_used) : a.blocks[i].bytes;
    HIPCHK(dst, hipMemcpyAsync(b.blocks[i].p, a.blocks[i].p, bytes, hipMemcpyDeviceToDevice, st));
  }
  // 2. where src's registered pointers point, in dst's blocks
  for (int k = 0; k < a.created_slots; k++) {
    const int i = block_of(a.blocks, *a.slots[k]);
    if (i < 0 || i >= a.created_blocks) return fail(dst, WX_E_STATE, "wx_copy_state: a registered pointer of src lies outside its blocks");
    *b.slots[k] = b.blocks[i].p + ((const char *)*a.slots[k] - a.blocks[i].p);
  }
  // 3. host state
  dst->run = src->run;
  dst->run.wet_shape_valid = false;
  dst->run.fix_check = false;
  dst->p = src->p;
  dst->geo = src->geo;
  dst->uni = src->uni;
  dst->have_params = src->have_params;
  dst->uploaded = true;
  dst->w0.even = src->w0.even;
  dst->w0.uni = src->w0.uni;
  dst->w0.initT_saved = src->w0.initT_saved;
  if (src->w0.initT_saved) {
    const size_t nb = ((size_t)src->Y + 1) * 4;
    if (!dst->w0.initT) HIPCHK(dst, hipMalloc((void **)&dst->w0.initT, nb));
    HIPCHK(dst, hipMemcpyAsync(dst->w0.initT, src->w0.initT, nb, hipMemcpyDeviceToDevice, st));
  }
  dst->vx.stale = true;
  dst->vx.untracked = false;
  dst->vx.have[0] = dst->vx.have[1] = false;
  dst->vx.check = false;
  // 4. device words outside the blocks, and the words in them that are dst's own
  plan.fc = FullCtx{dst->geo, dst->uni, dst->initial_T, dst->snd_T, dst->snd_W, dst->snd_Vel}; // (device pointers into dst's blocks)
  HIPCHK(dst, hipMemcpyAsync(dst->full_ctx, &plan.fc, sizeof(FullCtx), hipMemcpyHostToDevice, st));
  HIPCHK(dst, hipMemsetAsync(&dst->state->ghost_nontrivial, 0, 5 * 4, st)); // ghost_nontrivial, fix_overflow, pool_overflow, pool_seen_max, fastest_bits
  HIPCHK(dst, hipMemsetAsync(&dst->state->vx_max_bits, 0, 2 * 4, st));      // vx_max_bits, cone_violation
  if (dst->pair.words) {
    HIPCHK(dst, hipMemsetAsync(dst->pair.words + D2_N_REDO, 0, 4, st));
    HIPCHK(dst, hipMemsetAsync(dst->pair.words + D2_FIXED, 0, 8, st));
  }
  return WX_OK;
}

static_assert(offsetof(DevState, fastest_bits) - offsetof(DevState, ghost_nontrivial) == 16 && offsetof(DevState, cone_violation) - offsetof(DevState, vx_max_bits) == 4,
              "state_copy_enqueue zeroes these words as two runs");

} // namespace

int wx_copy_state(wx_sim *dst, wx_sim *src)
{
  if (!dst || !src) return WX_E_INVALID;
  if (dst == src) return WX_OK;
  if (int rc = state_copy_check(dst, src, "wx_copy_state")) return rc;
  DeviceScope dev_scope(src);
  // behind everything pending on both; src's pending report is consumed and returned here, and then nothing is copied
  if (int rc = wx_sync(src)) {
    dst->err = "wx_copy_state: src: " + src->err;
    return rc;
  }
  if (dst->comm_stream) HIPCHK(dst, hipStreamSynchronize(dst->comm_stream));
  HIPCHK(dst, hipStreamSynchronize(dst->stream));
  StateCopyPlan plan;
  int rc = state_copy_enqueue(dst, src, dst->stream, plan);
  const hipError_t he = hipStreamSynchronize(dst->stream); // (also when the enqueue failed half-way: `plan` is read by a pending copy)
  if (rc == WX_OK && he != hipSuccess) rc = fail(dst, WX_E_DEVICE, "wx_copy_state: %s", hipGetErrorString(he));
  return rc;
}

int wx_ensemble_broadcast(wx_ensemble *e, int src_member, const uint8_t *member_mask)
{
  if (!e) return WX_E_INVALID;
  const int B = (int)e->member.size();
  if (src_member < 0 || src_member >= B) return efail(e, WX_E_INVALID, "wx_ensemble_broadcast: member %d of %d", src_member, B);
  wx_sim *src = e->member[src_member];
  if (!src->uploaded) return efail(e, WX_E_STATE, "member %d: wx_ensemble_broadcast: src was never uploaded", src_member);
  if (!src->have_params) return efail(e, WX_E_STATE, "member %d: wx_ensemble_broadcast: src has no parameters (wx_set_params)", src_member);
  if (e->broken) return WX_E_STATE; // (the message of the failed step is kept)
  std::vector<int> sel;
  for (int i = 0; i < B; i++)
    if (i != src_member && (!member_mask || member_mask[i])) sel.push_back(i);
  for (int i : sel)
    if (int rc = epass(e, i, state_copy_check(e->member[i], src, "wx_ensemble_broadcast"))) return rc;
  if (sel.empty()) return WX_OK;
  DeviceScope dev_scope(src);
  // src's pending report (looked at only if its iterations left one to look at: that look waits for the stream)
  if (int rc = epass(e, src_member, validate_ghost_flag(src))) return rc;
  std::vector<StateCopyPlan> plans(sel.size());
  int rc = WX_OK;
  for (size_t k = 0; k < sel.size() && rc == WX_OK; k++) rc = epass(e, sel[k], state_copy_enqueue(e->member[sel[k]], src, e->stream, plans[k]));
  const hipError_t he = hipStreamSynchronize(e->stream); // the one wait
  if (rc == WX_OK && he != hipSuccess) rc = efail(e, WX_E_DEVICE, "wx_ensemble_broadcast: %s", hipGetErrorString(he));
  return rc;
}
