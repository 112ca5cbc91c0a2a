// wx_precip_bodies.h -- the bodies of the four particle kernels as program text, included inside the braces of the lone kernels
// (wx_kernels.h: k_precipitation, k_splat_classify, k_splat_box, k_splat_clear) and of their ensemble instantiations (wx_precip_ens.h:
// k_*_ens, member = blockIdx.y), so that a member of an ensemble cannot drift from a lone handle and the lone kernels keep their
// instruction streams. No include guard: WX_PRECIP_BODY selects the body (1 precipitation, 2 classify, 3 box sum, 4 clear) and is
// undefined again at the end. Expects in scope, by the lone kernels' parameter names:
//   1: g, u, n_drops, drops_in, base_in, water_in, st, drops_out, sg, sp, t_in, det, wall_in
//   2: X, Y, sg, mailbox, par           3: X, Y, sg, st, fb, dep, seam, mailbox, par           4: X, Y, sg, par, la
// blockIdx.x / gridDim.x are the workgroup's place in the lone kernel's grid in both.
#if WX_PRECIP_BODY == 1
  // t_in != nullptr (two-kernel path): base_in is the POST-pressure base texture, whose velocity components equal the
  // post-advection ones the reference samples (pressure_cell only touches P and T), and t_in holds the post-advection
  // temperature -- kernel B then stores 4 instead of 16 extra bytes per cell for the droplets.
  int count = 0; // still-inactive droplets seen by this wave (wave-uniform)
  for (int base_i = blockIdx.x * 256; base_i < n_drops; base_i += gridDim.x * 256) {
    const bool c = precip_droplet(base_i + (int)threadIdx.x, g, u, n_drops, drops_in, base_in, water_in, st, drops_out, sg, sp, t_in, det, wall_in);
    count += __popcll(__ballot(c));
  }
  // one atomic per workgroup (integers: exact in fp32 in any order)
  __shared__ int wave_count[4];
  if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int c = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
    if (c) unsafeAtomicAdd(&st->px_count, (float)c);
  }
#elif WX_PRECIP_BODY == 2
  const int T = sg.TXn * sg.TYn, t = blockIdx.x * blockDim.x + threadIdx.x;
  int *cnt = sg.work + 8 * par;
  if (t == 0)
    for (int k = 0; k < 5; k++) sg.work[8 * (par ^ 1) + k] = 0;
  // (no early return: wave_append needs the whole wave)
  const bool tile = t < T;
  const int tc = tile ? t : 0, tby = tc / sg.TXn, tbx = tc - tby * sg.TXn;
  wave_append(&cnt[2], sg.work + 16 + 2 * T, tile && sg.dirty[tc] != 0, tc);
  const bool tex = tile && tbx * STX < X && tby * STY < Y; // (the accumulation grid is one anchor wider / higher than the texture)
  int a = 0, a2 = 0;
  if (tex)
    for (int dy = -1; dy <= 1; dy++)
      for (int dx = -1; dx <= 1; dx++) {
        const int ax = tbx + dx, ay = tby + dy;
        if (ax >= 0 && ay >= 0 && ax < sg.TXn && ay < sg.TYn) {
          a |= sg.dirty[ay * sg.TXn + ax];
          a2 |= sg.dirty[T + ay * sg.TXn + ax];
        }
      }
  const bool corner = mailbox && tc == 0;
  wave_append(&cnt[0], sg.work + 16, tex && a != 0, tc);
  wave_append(&cnt[1], sg.work + 16 + T, tex && a == 0 && (!sg.fb_zero[2 * tc] || corner), tc);
  wave_append(&cnt[3], sg.work + 16 + 3 * T, tex && a2 != 0, tc);
  wave_append(&cnt[4], sg.work + 16 + 4 * T, tex && a2 == 0 && !sg.fb_zero[2 * tc + 1], tc);
#elif WX_PRECIP_BODY == 3
  constexpr int WH = STY + 11, PW = 77; // (pitch 77: the 4 rows x 8 runs a half-wave reads in the horizontal pass hit 32 banks)
  __shared__ float pl[3][WH][PW];
  const int tid = threadIdx.x;
  const int T = sg.TXn * sg.TYn, n_box = sg.work[8 * par], n_zero = sg.work[8 * par + 1], n_box2 = sg.work[8 * par + 3], n_zero2 = sg.work[8 * par + 4];
  const int cx = tid & 63, cyg = tid >> 6;
  // items: (tile, texture) for the tiles to box-sum, then the tiles to zero, dealt out round-robin. The launch must not hold more
  // workgroups than the chip does at once (splat_box_grid): with 2048 of them on a chip that holds 1536, the 512 of the second round
  // started their twelve items when the first round had finished. (Handing the items out through an atomic counter instead costs more
  // than it balances: 24 000 returning atomics on one address serialise, 0.37 instead of 0.25 ms.)
  // items: feedback tiles to box-sum, deposition tiles to box-sum (few: only where droplets reach the ground), feedback tiles to
  // zero, deposition tiles to zero
  const int e0 = n_box, e1 = e0 + n_box2, e2 = e1 + n_zero, e3 = e2 + n_zero2;
  for (int wi = blockIdx.x; wi < e3; wi += gridDim.x) {
    const int kind = wi < e0 ? 0 : (wi < e1 ? 1 : (wi < e2 ? 2 : 3));
    const int tile = kind == 0 ? sg.work[16 + wi] : (kind == 1 ? sg.work[16 + 3 * T + (wi - e0)] : (kind == 2 ? sg.work[16 + T + (wi - e1)] : sg.work[16 + 4 * T + (wi - e2)]));
    const int tby = tile / sg.TXn, tbx = tile - tby * sg.TXn;
    const int x0 = tbx * STX, y0 = tby * STY;
    const bool corner = mailbox && (tbx == 0 && tby == 0);
    const bool right = seam > 0 && x0 >= seam;
    const int qmin = right ? seam : 0, qmax = (seam > 0 && !right) ? seam : X, qshift = right ? 1 : 0;
    if (kind == 2) { // the texture tile holds the feedback of an earlier iteration (or the mailbox texels): zero it
      for (int k = 0; k < STY / 4; k++) {
        const int x = x0 + cx, y = y0 + cyg + 4 * k;
        if (x < X && y < Y) {
          float3 v = make_float3(0.f, 0.f, 0.f);
          if (corner && y == 0 && x == 0) v.x = st->px_count;
          if (corner && y == 0 && x == 1) v = make_float3(st->px_light[0], st->px_light[1], st->px_light[2]);
          fb[(size_t)y * X + x] = v;
        }
      }
      if (tid == 0) sg.fb_zero[2 * tile] = corner ? 0 : 1;
    } else if (kind == 3) { // ... the deposition of an earlier iteration
      for (int k = 0; k < STY / 4; k++) {
        const int x = x0 + cx, y = y0 + cyg + 4 * k;
        if (x < X && y < Y) dep[(size_t)y * X + x] = make_float2(0.f, 0.f);
      }
      if (tid == 0) sg.fb_zero[2 * tile + 1] = 1;
    } else if (kind == 0) {
      splat_box_tile<0>(pl, X, Y, sg, st, fb, dep, x0, y0, qmin, qmax, qshift, corner);
      if (tid == 0) sg.fb_zero[2 * tile] = 0;
    } else {
      splat_box_tile<1>(pl, X, Y, sg, st, fb, dep, x0, y0, qmin, qmax, qshift, corner);
      if (tid == 0) sg.fb_zero[2 * tile + 1] = 0;
    }
  }
#elif WX_PRECIP_BODY == 4
  if (la.st && blockIdx.x == 0 && threadIdx.x == 0) lightning_update(la.iterNum, la.refresh_inactive, la.fb, la.st, la.mailbox, la.defer);
  const int T = sg.TXn * sg.TYn, n = sg.work[8 * par + 2];
  for (int wi = blockIdx.x; wi < n; wi += gridDim.x) {
    const int tile = sg.work[16 + 2 * T + wi];
    const bool rain = sg.dirty[T + tile] != 0; // (uniform; the flag is reset below, behind the barrier)
    const int tby = tile / sg.TXn, tbx = tile - tby * sg.TXn;
    const int x0 = tbx * STX, y0 = tby * STY;
    for (int i = threadIdx.x; i < STX * STY; i += 256) {
      const int q = x0 + (i & 63), r = y0 + (i >> 6);
      if (q < sg.AP && r < sg.AH) {
        sg.acc3[(size_t)r * sg.AP + q] = make_float3(0.f, 0.f, 0.f);
        if (rain) sg.acc2[(size_t)r * sg.AP + q] = make_float2(0.f, 0.f);
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) sg.dirty[tile] = sg.dirty[T + tile] = 0;
  }
#else
#error "WX_PRECIP_BODY: 1 .. 4"
#endif
#undef WX_PRECIP_BODY
