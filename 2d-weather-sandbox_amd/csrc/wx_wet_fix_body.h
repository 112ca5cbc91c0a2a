// wx_wet_fix_body.h -- the body of the exact-path fix kernel, included by k_wet_fix and k_wet_fix_ens (wx_wet.h) inside their braces.
// Expects in scope: OPT_OUT; ctx, iterNum, in, out, count, cells, cap, overflow, hint.
  __shared__ WetPatch patches[4];
  __shared__ WetFixStage stages[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  WetPatch &pt = patches[wave];
  // An OVERFLOWED list is not consumed at all: an appender whose 1-3 entries straddle cap writes none of them (k_march_wet, `at + n_add <=
  // fix.cap`), so up to two slots below cap may hold whatever the allocation held before -- coordinates nobody checked (found by
  // tools/fuzz_parity.py: a memory access fault a few cases after a handle whose list had overflowed). The overflow is reported and the results
  // since are invalid either way (wx_step's next blocking call fails with WX_E_STATE).
  const int total = *count, n = total <= cap ? total : 0;
  if (total == 0) {
    // The usual case, and a launch that is pure latency on a small grid (5 us of a 20 us iteration at 100 x 100): nothing to recompute and
    // nothing to reset -- one load, and out. count[2] remembers what the host's hint word was last told: it is set back once.
    if (blockIdx.x == 0 && threadIdx.x == 0 && hint && count[2] != 0) {
      count[2] = 0;
      __hip_atomic_store(hint, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    return;
  }
  if (total > cap && blockIdx.x == 0 && threadIdx.x == 0) *overflow = total;
  const int X = ctx->g.X, Y = ctx->g.Y;
  // (entries whose footprints leave the patch fall back to wet_output_cell_exact, which builds its own argument block)
  for (int i = blockIdx.x * 4 + wave; i < n; i += gridDim.x * 4) {
    const int2 c = cells[i];
    wet_fix_build_patch(ctx, &in, iterNum, &stages[wave], &pt, c.x, c.y, lane);
    AdvOut o;
    o.b = o.w = make_float4(0.f, 0.f, 0.f, 0.f);
    o.wl = make_char4(0, 0, 0, 0);
    bool bad = false;
    if (lane < 3) { // lane 0: the cell itself, lane 1: its left neighbour, lane 2: the cell below
      const int ox = lane == 1 ? -1 : 0, oy = lane == 2 ? -1 : 0;
      const WetPatchAcc a{pt, WPATCH_C + ox, WPATCH_C + oy, &bad};
      advection_cell(ctx->u, ctx->g, ctx->initial_T, ctx->snd_T, ctx->snd_W, ctx->snd_Vel, wrapmod(c.x + ox, X), wrapmod(c.y + oy, Y), a, o.b, o.w, o.wl);
    }
    const bool any_bad = __any(bad);
    const float vx_l = __shfl(o.b.x, 1), vy_d = __shfl(o.b.y, 2), T_d = __shfl(o.b.w, 2);
    const int wl_d = __shfl(*reinterpret_cast<const int *>(&o.wl), 2);
    if (lane == 0) {
      if (any_bad) {
        wet_output_cell_exact(ctx, &in, &out, iterNum, OPT_OUT, c.x, c.y);
      } else {
        const char4 wD = unpack_wall(wl_d);
        const size_t gi = fidx(c.x, c.y, X);
        out.base[gi] = pressure_cell(o.b, vx_l, vy_d, T_d, wD.x, wD.y);
        out.water[gi] = o.w;
        out.wall[gi] = o.wl;
        GWetLightAcc la{in.lsrc, o.w, o.wl, o.b.w, T_d, X, c.x};
        const float4 l = lighting_cell(ctx->u, ctx->g, c.x, c.y, la);
        out.light.x[gi] = l.x;
        out.light.y[gi] = l.y;
        out.light.zw[gi] = make_float2(l.z, l.w);
        if (OPT_OUT) out.p_disp[gi] = o.b.z;
        if (out.t_disp) out.t_disp[gi] = o.b.w;
      }
    }
    wave_fence(); // the patch is rewritten by the next entry
  }
  // the list is empty again for the next launch group: reset by the LAST workgroup to get here (every workgroup has read the count
  // by then) -- count[1] is the arrival ticket -- which saves a memset in the stream per iteration
  __syncthreads();
  if (threadIdx.x == 0 && atomicAdd(count + 1, 1) == (int)gridDim.x - 1) {
    count[1] = 0;
    count[2] = total;
    __hip_atomic_store(count, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (hint) __hip_atomic_store(hint, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
