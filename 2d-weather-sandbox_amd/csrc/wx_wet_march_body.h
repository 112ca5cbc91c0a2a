// wx_wet_march_body.h -- the body of the marching wet kernel, included by k_march_wet and k_march_wet_ens (wx_wet.h) inside their braces.
// Expects in scope: the template parameters OPT_OUT, HAS_FB, QUIET; KArgs (= WetKArgs) and ka_c, the argument block in the constant
// address space; ctx, iterNum, n_strips, strip_lo, n_strips_all, segs, split_at, strip_lo2 (kernel arguments, or read from the block).
  const __attribute__((address_space(4))) WetIn &in = *(const __attribute__((address_space(4))) WetIn *)(ka_c + offsetof(KArgs, in));
  const __attribute__((address_space(4))) WetOut &out = *(const __attribute__((address_space(4))) WetOut *)(ka_c + offsetof(KArgs, out));
  // (the edge group's issue priority likewise: read where it is used -- the prologue --, nothing of it lives in the row loop)
  const int edge_prio = *(const __attribute__((address_space(4))) int *)(ka_c + offsetof(KArgs, edge_prio));
  __shared__ WetRing rings[WX_WET_WPB];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  WetRing &rg = rings[wave];
  // Everything the wave reads from the context goes through the constant address space: scalar loads that the compiler may
  // issue (and re-issue) anywhere. Through a generic pointer every such load behind the kernel's first store becomes a VECTOR
  // load with a uniform address, and waiting for it means waiting for the row prefetch issued just before (one in-order counter).
  CUni &u = as_constant(ctx->u);
  const Geo g = ctx->g;
  const CFloatP initial_T = as_constant(ctx->initial_T), snd_T = as_constant(ctx->snd_T), snd_W = as_constant(ctx->snd_W), snd_Vel = as_constant(ctx->snd_Vel);
  const int X = g.X, Y = g.Y;
  const int lane = threadIdx.x & 63, li = lane + WPAD;
  const int iterI = (int)iterNum;
  const bool smooth_iter = iterI % 100 == 0; // the only iterations in which the boundary pass reads its horizontal water neighbours
  // XCD-aware placement: workgroup id lands on XCD id % 8 (MI355X_MICROARCH.md), every XCD has its own L2. XCD k takes the
  // column block of strips [k*S/8, (k+1)*S/8) of EVERY segment: neighbouring strips (which share two 128-byte lines of halo
  // columns per field) hit the same L2, and every XCD gets the same mix of cheap free-air rows and expensive rows near terrain
  // (a contiguous range of segment-major items would hand all the terrain segments to XCD 0). Bottom segments first.
  // A workgroup = WX_WET_WPB neighbouring strips of one segment, one wavefront each.
  const int n_seg = segs.n_seg, k = blockIdx.x & 7, j = blockIdx.x >> 3;
  const bool bands = segs.bands != 0;
  const int sk0 = bands ? 0 : (k * n_strips) >> 3, nk = bands ? n_strips : (((k + 1) * n_strips) >> 3) - sk0, gk = (nk + WX_WET_WPB - 1) / WX_WET_WPB;
  if (j >= gk * n_seg) return;
  const int seg = j / gk;
  const int sloc = (j - seg * gk) * WX_WET_WPB + wave;
  if (sloc >= nk) return;
  // (a launch may cover two strip ranges -- the left and the right edge strips of a slab: the first split_at strips start at strip_lo,
  // the others at strip_lo2)
  const int sidx = sk0 + sloc;
  const int strip = sidx < split_at ? strip_lo + sidx : strip_lo2 + (sidx - split_at);
  const int item = ((bands ? k * n_seg : 0) + seg) * n_strips_all + strip;
  const int band_lo = bands ? (int)(((long long)k * g.Y) >> 3) : 0, band_hi = bands ? (int)(((long long)(k + 1) * g.Y) >> 3) : g.Y;
  const int c_out = strip * WOUT + lane - WLO; // output column of this lane (may be >= X in the last strip, < 0 in the first)
  const int col = wrapmod(c_out, X);           // column this lane loads / computes
  const bool lane_out = lane >= WLO && lane < WLO + WOUT && c_out < X;
  unsigned lo4 = (unsigned)col * 4u, lo8 = (unsigned)col * 8u, lo16 = (unsigned)col * 16u; // byte offsets of the loaded column
  unsigned lo12 = (unsigned)col * 12u; // (feedback texels)
  unsigned so4 = lane_out ? (unsigned)c_out * 4u : 0u, so8 = so4 * 2u, so16 = so4 * 4u;    // ... of the stored column
  const int y_lo = band_lo + segs.start[seg], y_hi = min(band_lo + segs.start[seg + 1], band_hi);
  if (y_lo >= y_hi) return; // (an empty segment of a clipped band)
  edge_wave_prio(edge_prio); // (!= 0 only in the edge group of a split iteration, wx_tile.h)
#define WX_WALL_RAW (reinterpret_cast<const int *>(in.wall))
  (void)item;

  // ---- registers carried from step to step ----
  float4 pf_b, pf_q = make_float4(0.f, 0.f, 0.f, 0.f);                // prefetched: base row r, water row r-2
  int pf_w;                                                          // wall row r (raw dword)
  float pf_lx = 0.f, pf_l0x = 0.f, pf_l0y = 0.f;                      // source sunlight, light_0 sunlight / net heating, row r-2
  float2 pf_lzw = make_float2(0.f, 0.f);                              // source IR fluxes row r-2
  float3 pf_fb = make_float3(0.f, 0.f, 0.f);                          // feedback / deposition row r-3 (HAS_FB)
  float2 pf_dep = make_float2(0.f, 0.f);
  bool fb_have = false, dep_have = false;                             // wave-uniform: the tile(s) of that row hold feedback / deposition
  unsigned short pf_flag = 0x0101;                                    // "feedback | deposition tile is all zero" flags (low | high byte) of the row prefetched next
  float4 b_prev = make_float4(0.f, 0.f, 0.f, 0.f);                    // base_0 row r-1
  int w_prev = 0;
  float4 q1 = make_float4(0.f, 0.f, 0.f, 0.f);                        // pre-boundary water row r-3
  float v1x = 0.f, v1y = 0.f;                                         // velocity row r-2
  float p2 = 0.f, t2 = 0.f;                                           // P, T of row r-2 (unchanged by the velocity pass)
  int w2 = 0;                                                         // wall row r-2 (raw dword)
  float v3x = 0.f, v3y = 0.f, p3 = 0.f, t3 = 0.f;                     // velocity output of row r-3: what the boundary stage starts from
  int w3 = 0;
  float c1 = 0.f, c2 = 0.f;                                           // curl rows r-3, r-4
  float vfDx = 0.f;                                                   // vortForce.x row r-4
  float TD = 0.f, vxD = 0.f, qzD = 0.f, qwD = 0.f;                    // pre-boundary values of row r-4 (see MWBoundaryAcc)
  char4 wD = make_char4(0, 0, 0, 0);
  float l0x1 = 0.f, l0y1 = 0.f, lz1 = 0.f;                            // light_0 sunlight / net heating, source IR_down of row r-3
  float adv_vy_prev = 0.f, adv_T_prev = 0.f;                          // advection output row r-5
  char4 adv_w_prev = make_char4(0, 0, 0, 0);
  // wave-uniform row flags as bit histories (bit 0 = the newest row, shifted up by one per step; one SGPR each instead of one per row:
  // the loop is short of them -- every spilled SGPR is a v_writelane / v_readlane, i.e. a vector instruction)
  unsigned h_big = 0;    // "some |v| >= 0.9" of post-boundary rows r-3, r-4, r-5
  unsigned h_nowall = 0; // "no wall cell" of the same rows
  unsigned h_zw0 = 0;    // "precipitation-visual and smoke channels of the water are all zero" of the same rows
  unsigned h_near = 15;  // "some cell at or next to a wall" of input rows r .. r-3
  float vx_seen = 0.f;   // largest |vx| among the post-boundary velocities of this wave's rows (VxTrack: slabs size their exchange period by it)
#define WX_H_SET(h, v) h = ((h) & ~1u) | ((v) ? 1u : 0u)
#define WX_H_ROT(h) h = ((h) << 1) | ((h) & 1u)
  // outputs of the previous step, stored at the top of this one
  float4 st_p = make_float4(0.f, 0.f, 0.f, 0.f), st_q = st_p, st_l = st_p, st_ab = st_p;
  char4 st_w = make_char4(0, 0, 0, 0);
  bool st_valid = false;
  bool st_td = false; // (wave-uniform) the stored row holds a cell directly above a land surface cell: its post-advection T differs from the post-pressure one

#ifdef WX_WET_TIMING
  const unsigned long long t_begin = __builtin_readcyclecounter();
#endif
  int r = y_lo - 4;
  { // prefetch of the first row
    const size_t e = (size_t)wrapmod(r, Y) * X;
    pf_b = ld_row(in.base + e, lo16);
    pf_w = ld_row(WX_WALL_RAW + e, lo4);
  }
  int sq3 = (r - 3 + 12) % WQ; // ring slot of row r-3 (base / wall / water planes)
  // wrapped (REPEAT) row indices of rows r+1, r-1 .. r-4, advanced by one per step (a general modulo costs ~20 scalar instructions)
  int yw_p1 = wrapmod(r + 1, Y), yw_m1 = wrapmod(r - 1, Y), yw_m2 = wrapmod(r - 2, Y), yw_m3 = wrapmod(r - 3, Y), yw_m4 = wrapmod(r - 4, Y);
  int t = 0;
  // WARM: one of the first eight steps of the segment, in which the stages come alive one after the other (t >= ...); the steady-state
  // instantiation has none of those wave-uniform branches -- every one of them is a control-flow merge at which the carried values of
  // both paths meet, i.e. a bundle of v_mov copies per step (a third of the loop's vector instructions were v_mov_b32)
#define WX_T_GE(n) (!WARM || t >= (n))
  auto step = [&](auto warm_tag) __attribute__((always_inline)) {
    constexpr bool WARM = decltype(warm_tag)::value;
    const float4 b_cur = pf_b, q_up = pf_q;       // base row r, water row r-2
    int w_raw = pf_w;
    const float lx_cur = pf_lx, l0x_cur = pf_l0x, l0y_cur = pf_l0y; // light row r-2
    const float2 lzw_cur = pf_lzw;
    const float4 fb_cur = make_float4(pf_fb.x, pf_fb.y, pf_fb.z, 0.f); // feedback row r-3
    const float2 dep_cur = pf_dep;
    const bool fb_cur_have = fb_have || dep_have;
    asm volatile("" : "+v"(w_raw)); // keeps the byte unpacking on this side of the prefetch
    const char4 w_cur = unpack_wall(w_raw);
#ifdef WX_STAGE_MARKS
    asm volatile("; @@ring");
#endif
    // ---- row r-3 enters the ring with its pre-boundary T and wall (what the boundary stage reads of its horizontal neighbours; the
    //      slot was row r-6's, last read by the previous step's advection); light row r-2 ----
    // Ahead of the prefetch: behind it (and behind the deferred stores) the compiler puts an s_waitcnt vmcnt in front of these LDS
    // writes that waits for the loads just issued -- a memory latency per step (5 % of the feedback instantiation,
    // profiles/r02_particles_ring_first.txt; the other one shows the same wait as soon as the stores lose their address copies).
    auto ring_in = [&]() {
      const int o = sq3 * WRW + li;
      (&rg.T[0][0])[o] = t3;
      (&rg.wl[0][0])[o] = unpack_wall(w3);
      rg.lx[(r - 2 + 8) & (WL - 1)][li] = lx_cur;
      rg.lw[(r - 2 + 8) & (WL - 1)][li] = lzw_cur.y;
    };
    ring_in();
#ifdef WX_STAGE_MARKS
    asm volatile("; @@prefetch");
#endif
    // ---- software prefetch: the loads of the next step are in flight while this one computes ----
    if (r < y_hi + 3) {
      {
        const size_t e = (size_t)yw_p1 * X;
        pf_b = ld_row(in.base + e, lo16);
        pf_w = ld_row(WX_WALL_RAW + e, lo4);
      }
      if (WX_T_GE(2)) { // (the first warm-up steps of a segment only feed velocity / curl: no water, no light yet)
        const int rl = r - 1;
        const size_t ew = (size_t)yw_m1 * X;
        pf_q = ld_row(in.water + ew, lo16);
        // light textures clamp in y (sun ray / IR taps of the lighting pass) ...
        const size_t el = (size_t)(rl < 0 ? 0 : (rl > Y - 1 ? Y - 1 : rl)) * X;
        pf_lx = ld_row(in.lsrc.x + el, lo4);
        pf_lzw = ld_row(in.lsrc.zw + el, lo8);
        // ... while the boundary pass samples light_0 at its own (wrapped) row and at the row above it, clamped
        pf_l0y = ld_row(in.l0.y + ew, lo4);
        // light_0's sunlight is only read by cells next to a wall and by surface wall cells, of rows r-1 and r-2: skipped while
        // none of the wall rows loaded so far (r-3 .. r) has such a cell (in even iterations the load coincides with pf_lx anyway)
        WX_H_SET(h_near, __any(w_cur.y <= 1));
        if (h_near & 15u) pf_l0x = ld_row(in.l0.x + ew, lo4);
      }
      if (HAS_FB) {
        // does any of the (up to three) 64x16 tiles under this strip hold feedback in row r-2? The flag byte was loaded one step
        // ago (pf_flag), so the vote costs no wait of its own
        fb_have = __any((pf_flag & 0xffu) == 0);
        dep_have = __any((pf_flag >> 8) == 0); // (only droplets that reach the ground deposit: few tiles)
#if defined(WX_ABL_FB_NOFLAG) || defined(WX_ABL_FB_NOLOAD)
        fb_have = dep_have = false; // (timing experiments only: wrong results)
#endif
#ifdef WX_ABL_FB_NOLOAD
        pf_fb = make_float3(0.f, 0.f, 0.f);
        pf_dep = make_float2(0.f, 0.f);
#else
        {
          // always the same two loads -- from the textures' row, or from a row of zeros (L2 resident) where the tiles are known
          // to be zero: a conditional load would make the number of loads per step, which the waits are built on, vary
          // (0.974-0.977 ms with the always-issued loads, 1.012-1.021 with loads only where a tile holds feedback)
          const size_t e = (size_t)yw_m2 * X;
          pf_fb = ld_row(fb_have ? in.fb + e : reinterpret_cast<const float3 *>(in.zero_row), lo12);
          // (the deposition texture is only read by surface wall cells, boundaryShader.frag:390-475: rows without a cell at or next to
          // a wall take it from the row of zeros too)
          pf_dep = ld_row((dep_have && (h_near & 4u)) ? in.dep + e : reinterpret_cast<const float2 *>(in.zero_row), lo8);
        }
#endif
#if !defined(WX_ABL_FB_NOFLAG) && !defined(WX_ABL_FB_NOLOAD)
        pf_flag = in.fb_zero != nullptr ? reinterpret_cast<const unsigned short *>(in.fb_zero)[(yw_m1 >> 4) * in.fb_txn + (col >> 6)] : (unsigned short)0; // row r-1, voted on next step
#endif
      }
    }
#ifdef WX_STAGE_MARKS
    asm volatile("; @@stores");
#endif
    // ---- the stores of the previous step's row (r-5), issued behind the prefetch ----
    if (st_valid && lane_out) {
      const size_t e = (size_t)(r - 5) * X;
      st_row(out.base + e, so16, st_p);
      st_row(out.water + e, so16, st_q);
      st_row(out.wall + e, so4, st_w);
      st_row(out.light.x + e, so4, st_l.x);
      st_row(out.light.y + e, so4, st_l.y);
      st_row(out.light.zw + e, so8, make_float2(st_l.z, st_l.w));
      if (OPT_OUT) st_row(out.p_disp + e, so4, st_ab.z);
#ifndef WX_ABL_NO_TDISP
      // post-advection temperature for the droplets: only rows in which the pressure pass changed it (k_precipitation's precip_T makes
      // the same test per texel and reads the post-pressure T everywhere else)
      if (out.t_disp && st_td) st_row(out.t_disp + e, so4, st_ab.w);
#endif
    }
    st_valid = false;
#ifdef WX_STAGE_MARKS
    asm volatile("; @@velocity");
#endif
    // ---- velocity of row r-1 ----
    float v0x = 0.f, v0y = 0.f;
    if (WX_T_GE(1)) {
      const float4 v = velocity_cell(u, b_prev, wave_from_right(b_prev.z), b_cur.z, unpack_wall(w_prev).y);
      v0x = v.x;
      v0y = v.y;
    }
#ifdef WX_STAGE_MARKS
    asm volatile("; @@curlvort");
#endif
    // ---- curl of row r-2, vortForce of row r-3 (registers + wave shifts only) ----
    float c0 = 0.f;
    if (WX_T_GE(2)) {
      c0 = curl_cell(v1x, v1y, wave_from_right(v1y), v0x);
      if (OPT_OUT) {
        const int yc = r - 2;
        if (lane_out && yc >= y_lo && yc < y_hi) st_row(out.curl + (size_t)yc * X, so4, c0);
      }
    }
    float2 vf = make_float2(0.f, 0.f);
    if (WX_T_GE(4)) vf = vorticity_cell(c1, wave_from_left(c1), wave_from_right(c1), c2, c0);
    const float vfLy = wave_from_left(vf.y);
    float qzL = 0.f, qwL = 0.f, qzR = 0.f, qwR = 0.f;
    if (smooth_iter) { // (wave-uniform) soil moisture / snow smoothing between surface cells: the neighbours' water texels
      qzL = wave_from_left(q1.z);
      qwL = wave_from_left(q1.w);
      qzR = wave_from_right(q1.z);
      qwR = wave_from_right(q1.w);
    }
    wave_fence();

#ifdef WX_STAGE_MARKS
    asm volatile("; @@boundary");
#endif
    // ---- boundary of row yb = r-3, written back in place ----
    if (WX_T_GE(4)) {
      const int ob0 = sq3 * WRW;
      const float4 b00 = make_float4(v3x, v3y, p3, t3);
      const char4 w00 = unpack_wall(w3);
      if (WX_T_GE(5)) {
        const int yb = yw_m3;
        const bool top = yb + 1 > Y - 1; // light_0 is CLAMP_TO_EDGE in y: the row "above" the top row is the top row itself
        MWBoundaryAcc a{rg, li, ob0, v1x, t2, unpack_wall(w2), b00, q1, q_up, w00, wD, vxD, TD, qzD, qwD, qzL, qwL, qzR, qwR, vf, vfLy, vfDx,
                        l0x1, l0y1, top ? l0x1 : l0x_cur, top ? l0y1 : l0y_cur, fb_cur, dep_cur, HAS_FB && fb_cur_have};
        float4 bb, bq;
        char4 bwl;
#ifdef WX_ABL_NOBOUNDARY // (ablation builds for the per-stage instruction budget; not bit-exact)
        bb = a.base(0, 0);
        bq = a.water(0, 0);
        bwl = a.wall(0, 0);
        bb.x += vf.x + vfLy + vfDx;
#else
        // free air (no wall within one cell, terrain at least 8 rows below) in every lane that feeds something: the
        // branch-free instantiation. Most rows of most strips; the general one handles everything else.
        if (WX_ABL_FORCE_AIR || __all(lane < 2 || lane > 60 || air_cell(w00, a.wall(-1, 0), wD, a.wall(1, 0), a.wall(0, 1))))
          boundary_cell<true>(u, iterNum, iterI, g, initial_T, col, yb, a, bb, bq, bwl);
        else
          boundary_cell<false>(u, iterNum, iterI, g, initial_T, col, yb, a, bb, bq, bwl);
#endif
        wave_fence(); // every lane has read its neighbours' pre-boundary values
        (&rg.vx[0][0])[ob0 + li] = bb.x;
        (&rg.vy[0][0])[ob0 + li] = bb.y;
        (&rg.P[0][0])[ob0 + li] = bb.z;
        (&rg.T[0][0])[ob0 + li] = bb.w;
        (&rg.wl[0][0])[ob0 + li] = bwl;
        const int oq = sq3 * WRW + li;
        (&rg.qx[0][0])[oq] = bq.x;
        (&rg.qy[0][0])[oq] = bq.y;
        (&rg.qz[0][0])[oq] = bq.z;
        (&rg.qw[0][0])[oq] = bq.w;
        vx_seen = fmaxf(vx_seen, fabsf(bb.x));
        // back-traces of this row that may leave the 3x3 cells? (lanes 2 .. 60 feed an advection that is used)
        // (one compare per component, not their fmaxf: that returns the other operand for a NaN, and a NaN back-trace has no footprint in
        // the ring. For finite velocities the vote is what it was: max >= 0.9)
        WX_H_SET(h_big, __any(lane >= 2 && lane <= 60 && (!(fabsf(bb.x) < 0.9f) || !(fabsf(bb.y) < 0.9f))));
        WX_H_SET(h_nowall, __all(lane < 2 || lane > 60 || bwl.y != 0)); // no wall cell in this post-boundary row (as far as advection reads it)
        WX_H_SET(h_zw0, __all(bq.z == 0.0f && bq.w == 0.0f));          // no rain / snow / smoke anywhere in it
        if (OPT_OUT) {
          const int yo = r - 3;
          // (NULL: the host makes waterTexture_0 on demand -- only saves read it, wxsim.hip materialize_water0)
          if (out.water0 && lane_out && yo >= y_lo && yo < y_hi) st_row(out.water0 + (size_t)yo * X, so16, bq);
        }
      }
      // the pre-boundary values of this row are what the row above reads as its lower neighbour
      TD = b00.w;
      vxD = b00.x;
      wD = w00;
      qzD = q1.z;
      qwD = q1.w;
    }
    wave_fence();

#ifdef WX_STAGE_MARKS
    asm volatile("; @@advection");
#endif
    // ---- advection of row ya = r-4 ----
    if (WX_T_GE(7)) {
      const int ya = yw_m4;
      float4 ab, aw;
      char4 awl;
      MWAdvAcc a{rg, li, {ring_back(sq3, 2, WQ) * WRW, ring_back(sq3, 1, WQ) * WRW, sq3 * WRW}};
      bool fast = true;
      if (h_big & 7u) { // wave-uniform: some velocity of rows ya-1 .. ya+1 is large -> per-lane test of the eight that matter
        const float *vxp = &rg.vx[0][0], *vyp = &rg.vy[0][0];
        const int o0 = a.ob[1] + li, om = a.ob[0] + li, op = a.ob[2] + li;
        const float m = speed8(vxp[o0], vxp[o0 - 1], vxp[op], vxp[op - 1], vyp[o0], vyp[om], vyp[o0 + 1], vyp[om + 1]); // (a NaN among them: +Inf)
        if (vxp[o0] != vxp[o0]) vx_seen = __builtin_inff(); // (the watch: fmaxf dropped a NaN vx in the row loop; it set the vote, so it is seen here and counts as +Inf)
        fast = m < 0.9f || lane < 3 || lane > 59; // (lanes outside 3 .. 59 feed nothing)
        if (!fast) {
          // This cell (column c_out, unwrapped row yu) keeps a placeholder; the OUTPUT cells it feeds that this wave owns -- its own,
          // the right neighbour's (pressure: vx of the left cell), the upper neighbour's (pressure / lighting: vy, T, wall of the lower
          // cell) -- go to the fix list. Rare path: one returning atomic per such lane.
          const int yu = r - 4; // == y_lo - 1 + (t - 7)
          const bool row_mine = yu >= y_lo, up_mine = yu + 1 < y_hi;
          const bool oA = lane_out && row_mine, oB = lane + 1 >= WLO && lane + 1 < WLO + WOUT && c_out + 1 < X && row_mine, oC = lane_out && up_mine;
          int n_add = (int)oA + (int)oB + (int)oC;
#ifdef WX_ABL_NOFIX // (timing-only ablation builds produce garbage velocities: keep them from flooding the exact path)
          n_add = 0;
#endif
          // (the list: read from the kernel-argument segment HERE, in the rare branch -- nothing of it is live in the loop)
          const __attribute__((address_space(4))) WetFixList &fix = *(const __attribute__((address_space(4))) WetFixList *)(ka_c + offsetof(KArgs, fix));
          if (fix.fastest) atomicMax(fix.fastest, __float_as_int(m)); // (m >= 0.9, +Inf for a NaN or Inf component: the bit patterns of positive floats order like ints)
          if (n_add) {
            int at = atomicAdd(fix.count, n_add);
            if (at + n_add <= fix.cap) {
              if (oA) fix.cells[at++] = make_int2(c_out, yu);
              if (oB) fix.cells[at++] = make_int2(c_out + 1, yu);
              if (oC) fix.cells[at++] = make_int2(c_out, yu + 1);
            }
          }
        }
      }
#ifdef WX_ABL_NOADV
      fast = false;
#endif
      if (fast) {
        if (WX_ABL_FORCE_AIR || (h_nowall & 7u) == 7u) { // (wave-uniform) plain instead of wall-aware interpolation, no wall branch
          if ((h_zw0 & 7u) == 7u) // ... and nothing to interpolate in the precipitation-visual / smoke channels
          {
#ifdef WX_STAGE_MARKS
            asm volatile("; @@advair");
#endif
            advection_cell<false, true, true, QUIET>(u, g, initial_T, snd_T, snd_W, snd_Vel, col, ya, a, ab, aw, awl);
#ifdef WX_STAGE_MARKS
            asm volatile("; @@advairend");
#endif
          }
          else
            advection_cell<false, true, false, QUIET>(u, g, initial_T, snd_T, snd_W, snd_Vel, col, ya, a, ab, aw, awl);
        } else {
          advection_cell<false, false, false, QUIET>(u, g, initial_T, snd_T, snd_W, snd_Vel, col, ya, a, ab, aw, awl);
        }
      } else { // placeholder (the post-boundary texel): this cell and the two it feeds are recomputed after the loop
        ab = a.base(0, 0);
        aw = a.water_off(0, 0);
        awl = a.wall(0, 0);
      }
#ifdef WX_STAGE_MARKS
    asm volatile("; @@presslight");
#endif
      // ---- pressure + lighting of row ya: kept in registers, stored at the top of the next step ----
      const float vx_l = wave_from_left(ab.x);
      if (WX_T_GE(8)) {
        st_p = pressure_cell(ab, vx_l, adv_vy_prev, adv_T_prev, adv_w_prev.x, adv_w_prev.y);
        if (out.t_disp) st_td = __any(adv_w_prev.y == 0 && adv_w_prev.x == 1); // (pressure_cell's condition, any lane of the row)
        MWLightAcc la{rg, li, ab.w, adv_T_prev, lz1, aw, awl};
#ifdef WX_ABL_NOLIGHT
        st_l = make_float4(la.sun_at(0, r - 4), la.ir_up_at(r - 5), lz1, ab.w);
#else
        if (WX_ABL_FORCE_AIR || __all(lane < WLO || lane >= WLO + WOUT || (awl.y != 0 && awl.z != 1)))
          st_l = lighting_cell<true>(u, g, col, r - 4, la);
        else
          st_l = lighting_cell<false>(u, g, col, r - 4, la);
#endif
        st_q = aw;
        st_w = awl;
        st_ab = ab;
        st_valid = true;
      }
      adv_vy_prev = ab.y;
      adv_T_prev = ab.w;
      adv_w_prev = awl;
    }
#ifdef WX_STAGE_MARKS
    asm volatile("; @@rotate");
#endif
    // ---- rotate the carried rows ----
    v3x = v1x;
    v3y = v1y;
    p3 = p2;
    t3 = t2;
    w3 = w2;
    p2 = b_prev.z;
    t2 = b_prev.w;
    w2 = w_prev;
    b_prev = b_cur;
    w_prev = w_raw;
    q1 = q_up;
    v1x = v0x;
    v1y = v0y;
    c2 = c1;
    c1 = c0;
    vfDx = vf.x;
    l0x1 = l0x_cur;
    l0y1 = l0y_cur;
    lz1 = lzw_cur.x;
    WX_H_ROT(h_big);
    WX_H_ROT(h_nowall);
    WX_H_ROT(h_zw0);
    WX_H_ROT(h_near);
    sq3 = sq3 + 1 == WQ ? 0 : sq3 + 1;
    yw_m4 = yw_m3;
    yw_m3 = yw_m2;
    yw_m2 = yw_m1;
    yw_m1 = yw_m1 + 1 == Y ? 0 : yw_m1 + 1;
    yw_p1 = yw_p1 + 1 == Y ? 0 : yw_p1 + 1;
  };
  // (a segment has at least one row: at least nine steps)
  for (; t < 8; r++, t++) step(std::true_type{});
  if (!HAS_FB && !OPT_OUT) { // (doubling the other instantiations re-measured at four waves per SIMD: neutral, profiles/r04_unroll_variants_four_waves.txt)
    // two steps per loop iteration: the values carried from step to step (prefetched rows, the previous rows' registers, the deferred
    // stores) change registers between the two copies instead of being moved: -1.2 .. -1.6 % at 16384x2048 without feedback loads; WITH them (particles on)
    // the doubled loop is 4-6 % slower, and the display-writing one (every tenth iteration) loses 2-8 %: only the plain instantiation
    // is doubled (profiles/r03_unroll_variants.txt)
    for (; r <= y_hi + 3;) {
      step(std::false_type{});
      r++;
      if (r > y_hi + 3) break;
      step(std::false_type{});
      r++;
    }
  } else {
    for (; r <= y_hi + 3; r++) step(std::false_type{});
  }
#undef WX_T_GE
  // ---- the last row ----
  if (st_valid && lane_out) {
    const size_t e = (size_t)(y_hi - 1) * X;
    st_row(out.base + e, so16, st_p);
    st_row(out.water + e, so16, st_q);
    st_row(out.wall + e, so4, st_w);
    st_row(out.light.x + e, so4, st_l.x);
    st_row(out.light.y + e, so4, st_l.y);
    st_row(out.light.zw + e, so8, make_float2(st_l.z, st_l.w));
    if (OPT_OUT) st_row(out.p_disp + e, so4, st_ab.z);
    if (out.t_disp && st_td) st_row(out.t_disp + e, so4, st_ab.w);
  }
  {
    const __attribute__((address_space(4))) VxTrack &vc = *(const __attribute__((address_space(4))) VxTrack *)(ka_c + offsetof(KArgs, vx));
    // (lanes 2 .. 60 only, the ones whose post-boundary velocity feeds an advection that is used: the vorticity stage reads the curl of
    // both neighbours, so lanes 61 and 62 hold values built from lane 63's missing right neighbour -- a lone cell of 1.12 cells / iteration in
    // the second column of a strip was reported as 1.68 by the wave to its left, tests/test_vx_watch_gpu.py. Every column is an
    // output lane, 4 .. 59, of the wave that owns it; masked here, behind the row loop, which keeps its one v_max per row step)
    vx_track_commit(VxTrack{vc.max_bits, vc.violation, vc.limit, vc.zone_l, vc.zone_r, vc.limit_in}, lane >= 2 && lane <= 60 ? vx_seen : 0.0f, lane, strip);
  }
#ifdef WX_WET_TIMING
  if (lane == 0) {
    out.cycles[2 * (size_t)item] = t_begin;
    out.cycles[2 * (size_t)item + 1] = __builtin_readcyclecounter();
  }
#endif
