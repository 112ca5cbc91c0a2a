/*
 * wxsim.h -- C ABI of the MI355X-native simulation engine (libwxsim.so).
 *
 * Drop-in boundary for the reference's "simulation step + field readback" seam
 * (niels747/2D-Weather-Sandbox has no FFI/plugin API: the seam is draw()'s simulation block and the
 * gl.readPixels / gl.getBufferSubData call sites, all talking to module-scope WebGL objects).
 * Every entry point cites the reference code it replaces (paths relative to the reference root).
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a negative
 * WX_E_* code, the message is available from wx_last_error(); no exceptions cross the ABI.
 * One caller thread per handle (the reference is single-threaded JS issuing an in-order GL command
 * stream). All grids are row-major with y = 0 at the BOTTOM, x fastest, 4 interleaved channels per
 * cell -- byte-identical to the reference's textures, readPixels results and save files
 * (app.js:1297-1312, 6586-6593).
 */
#ifndef WXSIM_H
#define WXSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WX_ABI_VERSION 11

/* error codes */
#define WX_OK 0
#define WX_E_INVALID (-1)   /* bad argument */
#define WX_E_DEVICE (-2)    /* HIP runtime error (message in wx_last_error) */
#define WX_E_NOMEM (-3)
#define WX_E_RANGE (-4)     /* rectangle / particle range outside the grid (no wrap, as readPixels) */
#define WX_E_STATE (-5)     /* call sequence error (e.g. step before upload) */

/* Uniform values of the simulation programs (what gl.uniform* pushes):
 *   velocityShader.frag:14-16, boundaryShader.frag:22-38, advectionShader.frag:21-43,
 *   lightingShader.frag:22-29, precipitationShader.vert:31-48; host side app.js:3401-3443
 *   (setGuiUniforms), app.js:5479-5635 (constants), app.js:6557-6561 (sun), app.js:5804-5808 (brush),
 *   app.js:3335 (airplane). All values are fp32 exactly as the GL uniform would hold them. */
typedef struct wx_params {
  float dragMultiplier, wind;
  float vorticity, landEvaporation, waterEvaporation, dynamicWaterTemperature;
  float evapHeat, waterWeight;
  float sunAngle;  /* solar zenith angle, rad (app.js:6538-6539) */
  float dryLapse;  /* simHeight * dryLapseRate / 1000 (app.js:5439) */
  float meltingHeat, condensationRate, globalDrying, globalHeating, soundingForcing;
  float globalEffectsStartAlt, globalEffectsEndAlt; /* normalised by simHeight (app.js:3425-3426) */
  float waterTemperature;                           /* K (app.js:3427) */
  float sunIntensity;                               /* W/m2 (app.js:6550) */
  float greenhouseGases, waterGreenHouseEffect, IR_rate;
  float aboveZeroThreshold, subZeroThreshold, spawnChanceMult, snowDensity, fallSpeed;
  float growthRate0C, growthRate_30C, freezingRate, meltingRate, evapRate;
  float inactiveDroplets; /* < 0: keep the engine's own measured value (app.js:5957-5966) */
  float userInputValues[4]; /* xpos ypos intensity brushSize (advectionShader.frag:21) */
  float userInputMove[2];
  int32_t userInputType;    /* -1 none (app.js:5749) */
  int32_t wrapHorizontally;
  float airplaneValues[4];
  int32_t enablePrecipitation; /* guiControls.enablePrecipitation (app.js:5936) */
  int32_t quad_scale;          /* 0: fragCoord = (x+.5, y+.5) exactly (the reference author's intent,
                                  app.js:4766-4769); 1: model the *1.0000001 quad UV scale */
  uint32_t pass_mask;          /* WX_PASS_* bits; WX_PASS_ALL = the reference loop */
} wx_params;

#define WX_PASS_VELOCITY 1u
#define WX_PASS_VORTICITY 2u   /* curl + vorticity */
#define WX_PASS_BOUNDARY 4u
#define WX_PASS_ADVECTION 8u
#define WX_PASS_PRESSURE 16u
#define WX_PASS_LIGHTING 32u
#define WX_PASS_PRECIPITATION 64u
#define WX_PASS_ALL 0x7Fu
#define WX_PASS_DRY (WX_PASS_VELOCITY | WX_PASS_ADVECTION | WX_PASS_PRESSURE)

/* Fields for wx_read_rect / wx_device_ptr. "FB0"/"FB1" are the reference's frameBuff_0 / frameBuff_1
 * (app.js:5243-5252); which one a consumer reads is listed in SURVEY.md section 3.5. */
enum {
  WX_FIELD_BASE_CUR = 0,   /* baseTexture_0: post-pressure state (FB0; weather stations, save) */
  WX_FIELD_BASE_DISP = 1,  /* baseTexture_1: post-advection, pre-pressure (FB1; display, sounding) */
  WX_FIELD_WATER_0 = 2,    /* waterTexture_0: post-boundary (what a save stores, app.js:6587-6589) */
  WX_FIELD_WATER_CUR = 3,  /* waterTexture_1: post-advection (current) */
  WX_FIELD_WALL_CUR = 4,   /* wallTexture_0 */
  WX_FIELD_WALL_DISP = 5,  /* wallTexture_1 */
  WX_FIELD_LIGHT_0 = 6,    /* lightTexture_0 (the one boundaryShader samples, app.js:5868-5869) */
  WX_FIELD_LIGHT_1 = 7,
  WX_FIELD_CURL = 8,       /* R32F */
  WX_FIELD_VORT = 9,       /* RG32F vortForce (an intermediate: only the per-pass kernel set, WX_FUSED=0, stores it) */
  WX_FIELD_PRECIP_FB = 10, /* RGBA32F precipitationFeedbackTexture (stored with its three written channels; alpha -- 0, and the lightning
                            * request's fourth component at texel (1,0), precipitationShader.vert:135-139 -- is added when the field is read) */
  WX_FIELD_PRECIP_DEP = 11,/* RG32F precipitationDepositionTexture */
  WX_FIELD_LIGHTNING = 12, /* 1x1 RGBA32F lightningDataTexture */
  /* RGBA16F emittedLight: the lighting pass's second render target (app.js:838, 5283, 5294; lightingShader.frag:15, 60-78,
   * 98-101, 143-166), read only by the renderer's ambient-light pyramid (app.js:6096). Not stored per iteration: computed for
   * the requested rectangle when read, from what the most recent lighting pass sampled (zero before the first one). The inputs of
   * that pass live until the next iteration: after a step whose last iteration ran WITHOUT the lighting pass (pass_mask) the field
   * reads zero, where the reference's texture would still show the last image drawn. */
  WX_FIELD_EMITTED = 13,
  WX_FIELD_COUNT = 14
};

/* destination element types of wx_read_rect (WX_DTYPE_F16: IEEE binary16, WX_FIELD_EMITTED only) */
enum { WX_DTYPE_F32 = 0, WX_DTYPE_I8 = 1, WX_DTYPE_I32 = 2, WX_DTYPE_F16 = 3 };

typedef struct wx_sim wx_sim;

/* Replaces texture/FBO creation app.js:5149-5317 and particle buffers app.js:4891-5002.
 * Allocates both ping-pong copies of every field on the current HIP device. */
int wx_create(int X, int Y, int n_droplets, wx_sim **out);

/* Column-slab variant (no reference counterpart: the reference is single-GPU). The handle owns columns
 * [x0, x0 + X_owned) of a periodic domain X_global wide and stores `halo` ghost columns on each side
 * (local width X_owned + 2*halo; local column i is global column (x0 - halo + i) mod X_global). */
int wx_create_slab(int X_global, int Y, int x0, int X_owned, int halo, int n_droplets, wx_sim **out);
/* Dependency cone of one iteration, columns per side: `halo` ghost columns stay exact for halo / WX_SLAB_CONE
 * iterations, then the halo must be exchanged (wx_halo_pack / wx_halo_unpack).
 * With particles the cone is wider from the second iteration of a period on: a droplet deposits within a sprite radius (6 columns) of
 * where it is, and the next boundary pass feeds that deposit through advection and pressure (3 more) -- 9 columns per iteration, after 6
 * for the first (whose feedback texture came with the exchange). Iteration j (0-based) of a period is exact on the owned columns +
 * halo - 6 - 9j ghost columns, droplets are processed there, and the owned columns need a sprite radius of that left in the last
 * iteration: WX_SLAB_PERIOD_PARTICLES(halo) iterations per exchange (at most 15: the flip history is a 16-bit mask). (For flows of one
 * cell per iteration and more wx_slab_period() is the authority: the cone is 6 + floor|vx|, and the last iteration keeps cone + 1 columns
 * instead of 6 -- a droplet is tested where it starts from and deposits where it arrives.)
 * (Rounds 2-3 assumed 6 per iteration throughout, which the measured spread -- 6 to 7 columns -- satisfied in every test but the
 * worst case does not.) */
#define WX_SLAB_CONE 6
#define WX_SLAB_CONE_PARTICLES 9
#define WX_SLAB_PERIOD_PARTICLES(halo) ((halo) < 12 ? 0 : ((1 + ((halo) - 12) / WX_SLAB_CONE_PARTICLES) < 15 ? (1 + ((halo) - 12) / WX_SLAB_CONE_PARTICLES) : 15))
/* Slabs exact at ANY speed (round 5). The figures above hold for |vx| < 1 cell / iteration -- the shaders' documented range
 * (common.glsl:40-41), which the reference never enforces: advectionShader.frag:85-99 back-traces `fragCoord - vel` for any vel, so one
 * iteration's cone really is 6 + floor|vx| columns. The marching kernels therefore keep the largest |vx| they produce, and the HOSTS OF ALL
 * SLABS agree on a bound per exchange period:
 *   wx_slab_vx_take(s, &v)       the largest |vx| this slab has seen since the last take (0 below 0.5; synchronises; after an upload /
 *                                wx_device_ptr(BASE_CUR) the state itself is scanned first)
 *   wx_slab_set_vx_bound(s, v)   v = the maximum over ALL slabs: the coming period assumes |vx| < 1.25 v + 0.25 (a flow measured at v may
 *                                have accelerated by the time the period is over), i.e. cone = 6 + floor(1.25 v + 0.25) once that
 *                                reaches 1 -- WX_E_STATE if the halo is too thin for it
 *   wx_slab_cone(s), wx_slab_period(s)   ghost columns per iteration / iterations per exchange under the current bound (with particles:
 *                                cone for the first iteration, cone + 3 for every further one, a sprite radius left in the last)
 * A non-finite vx (NaN or Inf: a state that has blown up) counts as +Inf in all of this: wx_slab_vx_take returns +Inf, for which no halo
 * is wide enough (wx_slab_set_vx_bound: WX_E_STATE), and inside a period it is reported wherever in the slab it lies.
 * A |vx| that reaches the bound inside a period is REPORTED by the next blocking call (WX_E_STATE), never silent; so is a velocity of
 * 2 * halo - 8 cells / iteration and more anywhere in the slab (beyond that even the strips three halo widths from the edges read ghost columns). wx_slab_step /
 * wx_group_step do all of this themselves without a host round trip inside a period: the maxima travel with the exchange (one word per
 * slab, all-gathered) and size the period after the next; slab.py's host-driven exchange all-reduces them. Which measurement sizes
 * which period: the first period after an upload, and the one that starts at the first exchange, are sized by the maximum of the
 * uploaded state (every slab scans its own, once); the period that starts at exchange e > 1 is sized by the larger of the two latest
 * COMPLETED measurements -- the maxima rolled at exchanges e - 1 and e - 2 (at e = 2: e - 1 alone), each the largest |vx| of 0.5 and more
 * any slab recorded between the exchange before it and itself, else 0. The measurement taken AT exchange e is still on its way to the
 * hosts then and is used from e + 1 on; the older of the two keeps a flow that slowed down for one period its margin for one more.
 * Hosts that drive wx_step_overlap / wx_halo_* themselves call the three functions once per period. */
int wx_slab_vx_take(wx_sim *s, float *vmax);
int wx_slab_set_vx_bound(wx_sim *s, float v_measured);
int wx_slab_cone(const wx_sim *s);
int wx_slab_period(const wx_sim *s);

void wx_destroy(wx_sim *s);
const char *wx_last_error(const wx_sim *s); /* also valid with s == NULL for create failures */
int wx_abi_version(void);
/* (ABI 11) Which arithmetic this library was built with. WX_ARITH_EXACT (libwxsim.so, the default and the one every parity claim is about):
 * no FMA contraction, correctly rounded division and sqrt -- bit-identical to the CPU oracle. WX_ARITH_FAST (libwxsim_fast.so, `make -C
 * csrc fast`; SURVEY.md Appendix A's opt-in tolerance build): contraction allowed, 1-ulp hardware reciprocal / sqrt -- the freedom a GL
 * driver takes with the reference's shaders (common.glsl:177-180, advectionShader.frag:111-131); masks stay bit-exact, float fields stay
 * inside the calibrated rounding envelope of the exact build (tests/test_fast_arith.py). A host picks one by the file it loads. */
#define WX_ARITH_EXACT 0
#define WX_ARITH_FAST 1
int wx_arith(void);

/* Replaces setupTextures() app.js:5189-5234 (the same data goes into BOTH _0 and _1) and
 * setupPrecipitationBuffers() app.js:4915-5002. Host arrays are copied; the caller keeps ownership.
 * Resets even=true, light/curl/vort/feedback/lightning = 0; iterNum is NOT reset (the reference keeps
 * it across KeyL reloads, app.js:4628-4640). Arrays cover the handle's LOCAL width. drops may be NULL. */
int wx_upload(wx_sim *s, const float *base, const float *water, const int8_t *wall, const float *drops);

/* Device-side initialiser of a new simulation: replaces the setup draw (shaders/fragment/setupShader.frag:36-92,
 * app.js `setupTextures` path for a new simulation) WITHOUT three X*Y host arrays. The caller passes the 1-D part of the
 * generator -- per local column: number of wall rows (0..Y), sea (1) / land (0), the vegetation noise term
 * `noise(x*0.01 + rand(seed)*10) * 150` (double) and the snow height; per row: air temperature, total and cloud water of
 * the initial sounding (setupShader.frag:78-89) -- and the textures are filled on the device. Equivalent to wx_upload of
 * the arrays that weather_sandbox_amd.synth.terrain_grid builds from the same descriptors (tested bit for bit); resets
 * the same state as wx_upload. */
int wx_setup_columns(wx_sim *s, const int32_t *wall_rows, const uint8_t *sea_column, const double *veg_noise, const float *snow,
                     const float *T_air, const float *total_water, const float *cloud_water, const float *drops);

/* The same with the 1-D part generated on the device too (k_terrain_columns: rand / noise of setupShader.frag:26-33, the octave sum of
 * :52-59, vegetation noise :72, snow :74 -- in double, operation for operation what the host generators evaluate, so the result equals
 * wx_setup_columns of weather_sandbox_amd.synth.terrain_columns(X, Y, seed=, height_mult=, snap=) unless the device's sin() differs in
 * the last bit at a column whose height sits on a row boundary). seed / height_mult: the shader's uniforms (app.js: Math.random() and the
 * new-simulation dialog); snap: terrain constant over `snap` columns and an even number of rows thick (1 = the shader's raw terrain);
 * sim_height: simHeight [m]; the three per-row arrays (Y entries) are the initial sounding as for wx_setup_columns. A slab handle
 * generates its own local columns (global column (x0 - halo + i) mod X_global): no host array scales with the grid. */
int wx_setup_terrain(wx_sim *s, double seed, double height_mult, int snap, double sim_height, const float *T_air, const float *total_water,
                     const float *cloud_water, const float *drops);

/* initRainDrops() (app.js:4901-4913) on the device: a fresh pool of inactive droplets whose five fields are random seeds, (r, r, -10 + r,
 * r, r) with r in [0, 1). Field c of droplet i = 24 bits of hash(seed + hash(5 i + c)) with the shaders' integer hash (common.glsl:103-111):
 * a pure function of the seed, so every slab of a decomposed domain generates the same pool (the partitioned pool wants the WHOLE pool
 * on every slab) and no host array scales with the droplet count. The grid is untouched; the pool bookkeeping of slab handles is reset
 * as after wx_upload. */
int wx_init_droplets(wx_sim *s, uint32_t seed);

/* Replaces the uniform pushes (see wx_params) plus the `initial_Tv` / realWorldSounding_* arrays
 * (app.js:5444-5474, 5485-5537). initial_T has Y+1 entries; sounding arrays Y+1 entries or NULL (= 0).
 * Takes effect at the next wx_step. */
int wx_set_params(wx_sim *s, const wx_params *p, const float *initial_T, const float *sounding_T,
                  const float *sounding_W, const float *sounding_Vel);

/* Replaces the loop body app.js:5830-6005: n_iter iterations, enqueued asynchronously on the handle's
 * stream; iterNum++ per iteration; the 600-iteration inactive-droplet count (app.js:5957-5966) is
 * refreshed on the device without a host round trip. */
int wx_step(wx_sim *s, int n_iter);
int wx_sync(wx_sim *s);

/* Engine options (no reference counterpart).
 * WX_OPT_SPLAT_ORDER: how the additive particle splats (gl.blendFunc(ONE, ONE) point sprites, app.js:5940-5953) are summed.
 *   0 (default): fp32 atomics in arrival order -- like the reference's blend unit the result depends on the order;
 *   1: deterministic -- every droplet records its deposit, the records are sorted by anchor texel (stable radix sort) and each
 *      texel's deposits are added in droplet-index order, so the feedback / deposition textures (and everything downstream)
 *      are a pure function of the state. Slower; meant for tests that compare coupled particle runs bit for bit.
 * WX_OPT_CHECK_LAUNCHES: 1 = synchronise after every kernel launch of wx_step and report a fault with the kernel's name
 *   (debugging; the launch status itself is always checked).
 * WX_OPT_KERNEL_SET: 1 (default) = the row-marching single-kernel iteration; 0 = one kernel per reference pass -- the independent
 *   cross-check every parity test also runs. WX_OPT_DRY_KERNEL: the water-free dry iteration as the row-marching kernel (1, default)
 *   or the LDS-tiled one (0). WX_OPT_ROW_BANDS: launch shape of the marching wet kernel -- 0 column blocks per XCD, 1 (default) row
 *   bands per XCD on grids at least 512 rows high, 2 row bands on any grid (tests). WX_OPT_FIX_CAP: entries of the exact-path cell
 *   list (default: a quarter of the grid's cells; tests provoke the overflow report), before the first step.
 * With s == NULL an option becomes the process-wide default of handles created afterwards (the library itself reads NO environment
 * variable; tuning switches exist only in -DWX_DEBUG builds). */
#define WX_OPT_SPLAT_ORDER 1
#define WX_OPT_CHECK_LAUNCHES 2
#define WX_OPT_KERNEL_SET 3
#define WX_OPT_DRY_KERNEL 4
#define WX_OPT_ROW_BANDS 5
#define WX_OPT_FIX_CAP 6
/* WX_OPT_POOL_EXACT (slab handles with particles): 1 = the partitioned droplet pool reproduces the undecomposed run EXACTLY. The
 *   default protocol exchanges nothing inside an exchange period, so a droplet that retires is not probed for re-spawning by the other
 *   ranks until the next exchange, a droplet can spawn a second time from a stale record, and the lightning state / inactive count are
 *   a period late. In exact mode the hosts run ONE iteration per wx_step and follow it with wx_pool_events_pack -> all-gather ->
 *   wx_pool_events_apply: the buffers then also carry every rank's lightning request (summed over the ranks before the accept test of
 *   lightningLocationShader.frag:24-38, so two requests in one iteration cancel as in the reference) and, every 600 iterations, what the
 *   `inactiveDroplets` refresh needs (app.js:5957-5966). Grid halos and edge droplets still travel once per period. With
 *   WX_OPT_SPLAT_ORDER 1 the slabs are then bit-identical to one handle (SURVEY 8e's determinism check); the price is a latency-bound
 *   all-gather of a few KB per iteration. */
#define WX_OPT_POOL_EXACT 7
/* WX_OPT_EXCHANGE_OVERLAP (slab handles driven by the library's transport: wx_slab_step / wx_group_step): 1 (default) = pack, transfers
 *   and unpack run on a side stream of the handle and hide behind the interior strips of the neighbouring iterations (grid-only: the
 *   iteration before AND after; with particles the iteration after, because precipitation needs its whole iteration and the exchange
 *   needs precipitation's feedback texture); 0 = everything in order on the compute stream -- same results bit for bit (tests), and
 *   what the exact particle mode always does. */
#define WX_OPT_EXCHANGE_OVERLAP 8
/* 9: retired, was the one-launch split iteration; not reused */
/* WX_OPT_DRY_PAIRS (round 5; default 1): the water-free dry stencil (pass_mask WX_PASS_DRY, no water anywhere, no brush, wall texture
 *   constant) runs TWO iterations per launch wherever two are left in a wx_step call and neither is a split iteration -- the second
 *   iteration's input never leaves the wavefront (csrc/wx_march2.h): 18 instead of 36 bytes per cell-step, 0.71 instead of 0.86 ms per
 *   iteration at 32768 x 4096. Same results bit for bit: cells whose back-trace is 0.9 cells or more (no exact path inside the march) are
 *   handled by tiles -- first-iteration ones taint what depends on them (NaN), second-iteration cells that are fast or tainted put their
 *   8 x 8 tile on a list, and a small fix kernel behind the pair recomputes both iterations for those tiles from the pair's untouched
 *   inputs (round 6; wx_pair_stats); only a back-trace of three cells or more -- or an overflowing list -- makes one further launch repeat
 *   the whole pair with the one-iteration stencil. 0 = one iteration per launch. */
#define WX_OPT_DRY_PAIRS 10
/* (ABI 10) 1 (default): waterTexture_0 -- the post-boundary water of a step's last iteration, which only saves read (app.js:6587-6589) --
 * is made when somebody asks for WX_FIELD_WATER_0 (per-pass kernels on the retained inputs of that iteration, with its parameters)
 * instead of being stored by every frame's last iteration: 16 of the 36 display-side bytes per cell. Applies to the marching wet kernel
 * without particles; 0 = always stored by the iteration itself. Bit-identical either way (tests/test_gpu_parity.py). */
#define WX_OPT_WATER0_ON_DEMAND 11
/* (ABI 11) WX_OPT_PLACEMENT_SEARCH: the number of further allocation sets the handle's ONE placement search tries (default 6; 0 = never).
 * A whole-domain handle of WX_PLACEMENT_AUTO_CELLS cells or more runs wx_tune_placement(s, tries, 20, ..) by itself inside its first
 * wx_step (a quarter of a second at 16384 x 2048; state, counters and results untouched; skipped silently if the device has no room for
 * two more copies of the state) unless the host has called wx_tune_placement before -- see "Placement tuning" below. Device pointers
 * taken before that first step are invalid after it. Slab handles never search by themselves (their hosts call wx_tune_placement). With
 * s == NULL: the default of handles created afterwards (tests switch the search off). */
#define WX_OPT_PLACEMENT_SEARCH 12
#define WX_PLACEMENT_AUTO_CELLS (8u << 20)
int wx_set_option(wx_sim *s, int option, int value);

/* iterNum global (app.js:440) */
int64_t wx_get_iter(const wx_sim *s);
int wx_set_iter(wx_sim *s, int64_t iter);

/* Replaces every gl.readPixels of SURVEY.md section 3.5 (app.js:1084-1092, 3931-3943, 3020-3065,
 * 1840-1906, 4215-4237, 4347-4357, 5958-5961, 5986-5988, 6584-6593). Rows bottom-up, no wrap
 * (WX_E_RANGE outside the local grid); float fields accept WX_DTYPE_F32, wall fields WX_DTYPE_I8 or
 * WX_DTYPE_I32 (both are used by the reference: app.js:6593 vs 3943), WX_FIELD_EMITTED WX_DTYPE_F16 (the texture's own
 * format) or WX_DTYPE_F32 (what readPixels(..., gl.FLOAT) of a half-float attachment returns). Synchronises the stream. */
int wx_read_rect(wx_sim *s, int field, int x, int y, int w, int h, void *dst, int dtype);

/* Replaces gl.getBufferSubData on the transform-feedback buffers (app.js:5019, 5086, 6597):
 * 5 floats per droplet (pos.xy, mass.xy, density) from the destination buffer of the last step. A blocking call like wx_read_rect:
 * whatever the iterations have to report (WX_E_STATE: an overflowed exact-path list, ...) is reported here instead of droplets. */
int wx_read_particles(wx_sim *s, int first, int count, float *dst);

/* Field streaming for a display consumer: what the reference's renderer binds every frame (app.js:6081-6219)
 * -- BASE_DISP, WATER_CUR, WALL_DISP (int8), LIGHT_0, CURL, PRECIP_FB, EMITTED (binary16) of the viewport rect, in this order,
 * each field contiguous (w*h texels, rows bottom-up, no wrap) -- copied asynchronously into ONE host buffer of wx_stream_bytes(w, h)
 * bytes, ideally pinned (wx_host_alloc). wx_stream_frame returns at once: the copies run on the handle's own copy
 * stream after everything enqueued so far; later wx_step calls are ordered after them on the device, so the host never
 * blocks; wx_stream_wait blocks until the frame is complete in host memory. One frame in flight per handle. */
size_t wx_stream_bytes(int w, int h);
void *wx_host_alloc(size_t bytes); /* pinned host memory; NULL on failure */
void wx_host_free(void *p);
int wx_stream_frame(wx_sim *s, int x, int y, int w, int h, void *host_dst);
int wx_stream_wait(wx_sim *s);

/* Placement tuning (no reference counterpart). Where a handle's planes lie in physical device memory decides how the ~13 streams of
 * the marching kernels spread over the HBM channels: the same binary runs the same iteration in 0.72 .. 0.87 ms depending on the
 * allocations (profiles/r03_alloc_probe.txt). wx_tune_placement times the handle's own iteration (current parameters and
 * pass mask; 4 untimed + iters_per_try timed iterations) on the allocations it has and on up to `tries` further sets that receive a
 * copy of the state, keeps the fastest as the handle's storage and restores the state from a backup taken at the start: state,
 * iteration counter and all fields are unchanged;
 * device pointers obtained from wx_device_ptr before the call are invalid afterwards. ms_before / ms_after (may be NULL): the
 * iteration time on the allocation the handle had and on the winner. Needs three times the handle's memory while it runs (more is used
 * if free: rejected candidates are kept until the end so that the allocator does not hand the same memory out again). */
int wx_tune_placement(wx_sim *s, int tries, int iters_per_try, float *ms_before, float *ms_after);
/* (ABI 11) Returns 1 and the two iteration times [ms] of the handle's placement search -- the host's call above or the implicit one of
 * the first wx_step (WX_OPT_PLACEMENT_SEARCH) -- if one has run, else 0. Either pointer may be NULL. */
int wx_placement_info(const wx_sim *s, float *ms_first, float *ms_kept);

/* ---- plumbing for hosts that own device memory / streams (PyTorch, multi-GPU halo exchange) ---- */
int wx_set_stream(wx_sim *s, void *hip_stream);     /* NULL = legacy default stream */
void *wx_device_ptr(wx_sim *s, int field);          /* device address of a field's current storage; WX_FIELD_LIGHT_0/1, WX_FIELD_EMITTED,
                                                     * WX_FIELD_PRECIP_FB and (after the marching wet kernel, round 6) WX_FIELD_BASE_DISP are
                                                     * stored in another form (planes / on demand / three channels / post-advection P only): the
                                                     * pointer is to the RGBA texture made at the time of the call, valid until the next wx_step.
                                                     * WX_FIELD_BASE_CUR / _WALL_CUR may be written through: the on-demand WX_FIELD_BASE_DISP,
                                                     * which is assembled from them, is made whole first, so a later read still shows the last
                                                     * display iteration's texture, not the host's edit.
                                                     * Slabs: velocities written through WX_FIELD_BASE_CUR are looked at by the next exchange
                                                     * (a |vx| beyond the current period's bound is REPORTED, WX_E_STATE); only wx_upload /
                                                     * wx_setup_* re-size the first period -- and on the slabs of an initialised ring those are
                                                     * COLLECTIVE: every rank calls them alike before the next wx_slab_step / wx_exchange (the
                                                     * ranks all-gather their |vx| once after an upload: a rank that skipped it would pair the
                                                     * ring's later collectives off by one) */
int wx_local_width(const wx_sim *s);                /* X_owned + 2*halo */
/* Halo exchange of the state carried across iterations (base_0, wall_0, water_1, both light textures; with particles also
 * the feedback and deposition textures):
 * pack the `halo` outermost OWNED columns of one side into a contiguous device buffer / unpack a
 * neighbour's buffer into this handle's ghost columns. side: 0 = left (low x), 1 = right. */
size_t wx_halo_bytes(const wx_sim *s);
/* (ABI 10) How much of such a buffer a message of the CURRENT period occupies, from its first byte: wx_halo_bytes normally; between slabs
 * that agreed on the water-free dry stencil (wx_slab_assert_water_free(s, 1) below) the base texture alone -- 16 of the 68 bytes per cell:
 * that iteration writes nothing else, so the ghost columns of water, wall and light stay what the upload made them. A host transport
 * sends / receives this many bytes of the buffers it packs / unpacks (buffers are still sized by wx_halo_bytes). The value changes only
 * through calls every rank makes alike -- wx_slab_assert_water_free, or a wx_step whose parameters leave the water-free dry stencil --, so
 * neighbours never disagree about a message's size; a slab that was given new contents in between is refused by wx_halo_pack
 * (WX_E_STATE) until the slabs have agreed again. Such slabs also run their periods in order (iterations in pairs, none split:
 * wx_step_overlap's flags are ignored), which is faster there than the overlap (profiles/r05_dry_slab_inorder.txt). */
size_t wx_halo_message_bytes(const wx_sim *s);
int wx_halo_pack(wx_sim *s, int side, void *dev_buf);
int wx_halo_unpack(wx_sim *s, int side, const void *dev_buf);
/* both sides in ONE launch each (ABI 8): next to a marching kernel that holds every wave slot of the chip a second small launch queues
 * behind thousands of workgroups (profiles/r04_slab_protocol_cost.txt); dev_left / dev_right as side 0 / 1 above */
int wx_halo_pack_both(wx_sim *s, void *dev_left, void *dev_right);
int wx_halo_unpack_both(wx_sim *s, const void *dev_left, const void *dev_right);
/* Overlap of the halo exchange with compute (no reference counterpart; BASELINE north_star: "halo exchange ... overlapped on a
 * side HIP stream"). After wx_set_comm_stream(s, stream) the pack / unpack kernels run on `stream` -- the stream the host also
 * issues its send / recv on -- fenced against the handle's compute stream by events inside the library:
 *   wx_step_overlap(s, n, WX_OVERLAP_EDGES_FIRST): in the LAST iteration of the call the edge strips (every column
 *     wx_halo_pack reads) are a launch group of their own, on a high-priority stream of the handle next to the interior strips'
 *     group, and an event is recorded behind them; wx_halo_pack waits for that event only, so packing and sending run while the
 *     interior strips of that iteration still compute;
 *   wx_step_overlap(s, n, WX_OVERLAP_EDGES_LAST): in the FIRST iteration the interior strips start at once; the edge strips'
 *     group, the only one that reads ghost columns, waits for the event wx_halo_unpack recorded on the comm stream.
 * The compute stream goes on behind both groups. This is the one form of a split iteration (a one-launch form with device-side
 * hand-offs was built, measured not faster and retired: DESIGN.md section 6).
 * Both flags may be combined. The split needs a row-marching kernel (default kernel set; all grid passes on, or the water-free
 * dry iteration; particles off) and a slab wide enough to have interior strips; otherwise the call degrades to the in-order exchange: wx_halo_pack waits
 * for everything enqueued on the compute stream, the next wx_step waits for the unpack. wx_step(s, n) == wx_step_overlap(s, n, 0). */
/* The water-free dry iteration on slabs. pass_mask == WX_PASS_DRY runs a kernel that does not touch the water texture at all
 * (36 B/cell) while the handle KNOWS it is trivial (0 in air, only the wall marker in walls: established by wx_upload, dropped by
 * anything that can create water). A slab also receives its neighbours' ghost columns, so it relies on that only after the host
 * has established it for every slab: wx_water_free(s) reports what the last wx_upload found for THIS handle, the host combines
 * the answers of all ranks (slab.py: all-reduce MIN) and passes the result to wx_slab_assert_water_free on every handle. A
 * wrong assertion is never silent: the slab whose own contents contradict it refuses its next wx_halo_pack (WX_E_STATE; ABI 10 --
 * agreed slabs exchange the base texture alone, wx_halo_message_bytes), and handles that carry particles, which keep the full
 * message, validate the arriving water on the device at every wx_halo_unpack (reported by the next blocking call). Without the
 * assertion a slab handle runs the water-carrying dry kernel. */
int wx_water_free(const wx_sim *s);
int wx_slab_assert_water_free(wx_sim *s, int agreed);

#define WX_OVERLAP_EDGES_FIRST 1u
#define WX_OVERLAP_EDGES_LAST 2u
/* (ABI 10) This call is one piece of a longer step -- another wx_step / wx_step_overlap follows before anything reads a display-side
 * field (WX_FIELD_BASE_DISP, _WATER_0, _CURL, the emitted-light image): its last iteration does not store them. A slab host cuts
 * a frame of 10 iterations into exchange periods of 6 or 7; without the flag every piece ends with an iteration that stores 36 B per
 * cell nobody looks at -- 4 of 30 iterations, +4 % on the metric's slab (profiles/r05_slab_protocol_cost.txt). wx_slab_step /
 * wx_group_step set it themselves for every piece but the last. */
#define WX_OVERLAP_MORE_TO_COME 4u
int wx_set_comm_stream(wx_sim *s, void *hip_stream); /* NULL: pack / unpack on the compute stream again */
int wx_step_overlap(wx_sim *s, int n_iter, unsigned flags);

/* Particles on slabs (n_droplets > 0 with halo > 0; halo and X_owned multiples of 64): the PARTITIONED droplet pool.
 * wx_upload hands every rank the whole pool once; from then on an active droplet is tracked by the rank whose owned columns contain
 * it (and, as a ghost copy, by the neighbour while it is within `halo` columns of the common edge); the other ranks only know
 * "active elsewhere" and skip it. Inactive droplets are static records that every rank holds; every rank tests every inactive
 * record's hashed spawn probe (precipitationShader.vert:82-84: anywhere in the domain) against its own columns and acts on the ones
 * that land where its grid is valid. Nothing is communicated inside an exchange period (WX_SLAB_PERIOD_PARTICLES(halo) iterations, at
 * most 15). At the halo exchange (all buffers are DEVICE pointers; calls are enqueued on the handle's stream):
 *   wx_pool_events_pack  -> all-gather of the buffers -> wx_pool_events_apply(gathered, n_ranks, stride_bytes):
 *       a buffer = 16-byte header (first int32: number of events) + 32-byte events, wx_pool_event_bytes() in all (room for every
 *       droplet: the start-up burst of an all-inactive pool flips most of them in one period); the hosts normally gather only the
 *       filled part -- stride_bytes = bytes per rank in `gathered` (0 = whole buffers), the same on every rank, >= the largest count;
 *       the droplets whose active / inactive status flipped (spawned, evaporated, deposited) with their final records; per droplet
 *       the report with the earliest first flip wins, then the longest flip history, then the rank that processed it last -- a rank
 *       that spawned a droplet from a stale inactive record after another rank had (it cannot know inside a period) drops its phantom;
 *   wx_pool_edges_pack(left, right, refresh_inactive) -> send / recv with the ring neighbours (same batch as the grid halos)
 *       -> wx_pool_edges_apply(buffer received from either neighbour): active droplets that left the owned columns are handed over,
 *       the ones within `halo` columns of an edge become the neighbour's ghost copies. refresh_inactive != 0 also refreshes the
 *       `inactiveDroplets` uniform (app.js:5957-5966) from the inactive records -- every rank holds all of them: no collective;
 *   lightning state: wx_lightning_get -> pick the latest strike -> wx_lightning_set;  then wx_slab_period_begin.
 * Buffer overflows (more status flips / edge droplets than the fixed capacities) are reported by the next blocking call (WX_E_STATE).
 * wx_pool_events_apply checks the header of every one of its n_ranks buffers against the stride's capacity, whatever n_ranks is.
 * wx_read_particles returns the LOCAL view of the pool; wx_pool_flags says per droplet what it is worth: 0 = tracked by another rank
 * (stale here), 1 = inactive (the same record on every rank), 2 = active inside this rank's owned columns (THE record), 3 = ghost copy. */
int wx_slab_set_rank(wx_sim *s, int rank);
int wx_slab_period_begin(wx_sim *s);
size_t wx_pool_event_bytes(const wx_sim *s);
size_t wx_pool_edge_bytes(const wx_sim *s);
int wx_pool_events_pack(wx_sim *s, void *dev_buf);
int wx_pool_events_apply(wx_sim *s, const void *dev_bufs, int n_ranks, size_t stride_bytes);
int wx_pool_edges_pack(wx_sim *s, void *dev_left, void *dev_right, int refresh_inactive);
int wx_pool_edges_apply(wx_sim *s, const void *dev_buf);
int wx_pool_flags(wx_sim *s, uint8_t *host_dst);
int wx_lightning_get(wx_sim *s, float out[4]);
int wx_lightning_set(wx_sim *s, const float in[4]);

/* ---- the halo exchange inside the library (no reference counterpart: the reference is single-GPU; BASELINE north_star: "halo
 * exchange on RCCL send/recv over xGMI overlapped on a side HIP stream; host code stays in JavaScript"). RCCL is bound at run time
 * (dlopen), so nothing here is needed to run on one GPU.
 *
 * One rank per process (what `bench.py --gpus N` runs under torchrun, which then only launches the ranks and carries the 128-byte
 * id from rank 0 to the others):
 *   wx_comm_unique_id(id)                  ncclGetUniqueId
 *   wx_comm_init(s, id, rank, world)       ncclCommInitRank on the handle's device; rank r owns columns [r, r + 1) * X_global / world
 *   wx_exchange(s)                         pack both edges -> ncclGroupStart; ncclSend x 2; ncclRecv x 2; ncclGroupEnd -> unpack both
 *                                          ghost strips, all enqueued on the handle's comm stream (one of the library's own unless
 *                                          wx_set_comm_stream named one); never blocks the host
 *   wx_slab_step(s, n)                     n iterations with one wx_exchange per wx_slab_period(s) iterations; the iteration before
 *                                          an exchange launches its edge strips first, the one after it its interior strips first
 *                                          (wx_step_overlap), so the transfer runs behind the interior of both. Replaces the loop
 *                                          body app.js:5830-6005 for one slab of a decomposed domain.
 * One process, N slabs (the Node host: `node host/sim_host.js --gpus N`): */
#define WX_UNIQUE_ID_BYTES 128
int wx_comm_unique_id(void *id128);
int wx_comm_init(wx_sim *s, const void *id128, int rank, int world);
int wx_exchange(wx_sim *s);
int wx_slab_step(wx_sim *s, int n_iter);

typedef struct wx_group wx_group;
#define WX_TRANSPORT_AUTO 0  /* RCCL if every slab has a device of its own, else local */
#define WX_TRANSPORT_RCCL 1  /* ncclCommInitAll over the slabs' devices (RCCL refuses two ranks on one device) */
#define WX_TRANSPORT_LOCAL 2 /* device-to-device copies between the slabs' halo buffers, event-fenced: any number of slabs per device */
/* n_slabs handles of X_global / n_slabs columns each (+ `halo` ghost columns per side), slab i on devices[i] (NULL: i modulo the
 * device count), every slab with compute and comm streams of its own. Upload / set parameters / read through the per-slab handles
 * (wx_group_slab; local arrays incl. ghost columns, as for wx_create_slab), then wx_group_agree once, then step the group. */
int wx_group_create(int n_slabs, const int *devices, int X_global, int Y, int halo, int n_droplets, int transport, wx_group **out);
void wx_group_destroy(wx_group *g); /* destroys the slab handles too */
const char *wx_group_last_error(const wx_group *g);
int wx_group_count(const wx_group *g);
int wx_group_transport(const wx_group *g);
wx_sim *wx_group_slab(wx_group *g, int i);
int wx_group_agree(wx_group *g);            /* after the uploads: wx_water_free of every slab -> wx_slab_assert_water_free on all */
int wx_group_set_option(wx_group *g, int option, int value); /* wx_set_option on every slab (WX_OPT_SPLAT_ORDER, WX_OPT_POOL_EXACT ...) */
int wx_group_step(wx_group *g, int n_iter); /* like wx_slab_step, for all slabs; asynchronous */
int wx_group_exchange(wx_group *g);         /* an exchange now: afterwards every active droplet is owned by exactly one slab (read the pool then) */
int wx_group_sync(wx_group *g);
/* Slabs with particles (n_droplets > 0; halo and X_global / n_slabs multiples of 64) on the library's transport: wx_upload hands every
 * slab the WHOLE pool; wx_exchange / wx_slab_step / wx_group_step then also run the droplet-pool protocol above -- status flips (+ every
 * rank's lightning state) all-gathered with a stride every rank derives from the headers of the PREVIOUS period's rounds (the whole
 * event buffer at first, then 4 x the largest count seen, at least 65536 events: no host round trip inside a period; a burst beyond
 * that is reported as WX_E_STATE by the next blocking call), edge droplets in the same batch of transfers as the grid halos -- every
 * WX_SLAB_PERIOD_PARTICLES(halo) iterations, on the handle's side stream behind the interior strips of the next iteration
 * (WX_OPT_EXCHANGE_OVERLAP); with WX_OPT_POOL_EXACT in order, one iteration at a time, each followed by the all-gather of its flips and
 * lightning requests. */

/* The largest |velocity component| [cells / iteration] among the cells the marching wet kernel handed to its exact path (back-traces
 * of 0.9 cells and more) since the last call; 0 if there was none; +Inf if one of them was NaN or Inf (a NaN never shows as a small
 * number: the state has blown up). Resets the value; synchronises the
 * handle's stream. Whole-domain handles and slabs are exact at any speed (slabs size their exchange period by the |vx| they measure:
 * wx_slab_set_vx_bound above); the value is a diagnostic of the flow, nothing more. */
int wx_fastest_velocity(wx_sim *s, float *cells_per_iteration);

/* (ABI 11) The pair kernel's exact path (WX_OPT_DRY_PAIRS) since the last call: how many output cells k_dry2_fix recomputed (81 per
 * recorded 8 x 8 tile of cells with back-traces of 0.9 .. 3 cells in either iteration: one wavefront per tile) and how many pairs were repeated WHOLE with the
 * one-iteration kernel (a second-iteration back-trace of three cells or more, or more recorded cells than the list holds: 1/64 of the
 * grid's cells, 64 Ki .. 1 Mi tiles, WX_OPT_FIX_CAP). Either pointer may be NULL. Resets both; synchronises the handle's stream. The
 * reference has no velocity clamp (advectionShader.frag:85-99); results are bit-identical to one iteration per launch whatever these say. */
int wx_pair_stats(wx_sim *s, int64_t *cells_recomputed, int64_t *pairs_repeated);

/* ---- Conservation and health diagnostics, computed on the device in one pass over the state ----
 * Replaces the reference's commented-out block app.js:6736-6762 (readPixels of the whole water texture, then a JavaScript loop that sums
 * vapour, cloud and smoke over the non-wall cells). Covers the handle's OWNED columns (the ghost columns of a slab are excluded), all
 * rows, of the CURRENT state: WX_FIELD_BASE_CUR, WX_FIELD_WATER_CUR, WX_FIELD_WALL_CUR and the droplet buffer wx_read_particles returns.
 * A cell is a WALL cell iff channel 1 (distance) of its WX_FIELD_WALL_CUR texel is 0 -- the engine's own test in bilerpWall
 * (common.glsl:216-254) --, otherwise an AIR cell.
 *
 * Every floating-point sum is EXACT: the correctly rounded (round-to-nearest-even, to double) value of the mathematically exact sum of
 * the float values it covers -- what Python's math.fsum returns. It therefore does not depend on the order of summation, the launch
 * shape or the decomposition: N slabs merged give the bits of the undecomposed handle. A non-finite VALUE (NaN, +-Inf) is never added
 * into a sum (the other channels of its cell are); such cells are counted. A sum over no values is +0.0.
 * Extremes: NaNs are skipped; -0.0 and 0.0 compare equal (a zero extreme is reported as +0.0); among equal values the cell with the
 * smallest global index y * X_global + x is reported. Locations are GLOBAL (x, y), y = 0 at the bottom; -1, -1 means "none".
 * A diagnostics call changes nothing: not the state, not the fields that are made on demand, not the iteration counter. */
#define WX_HAVE_DIAGNOSTICS 1
typedef struct wx_diag {
  int64_t iter;               /* the iteration counter the numbers belong to */
  int64_t n_air, n_wall;      /* census of the covered cells */
  int64_t n_marker_mismatch;  /* cells where (water.x > 1000) differs from "is a wall cell": the reference's diagnostic tests the marker, the engine the wall texture */
  int64_t n_negative_water;   /* air cells with water.x < 0 */
  int64_t n_nonfinite_base, n_nonfinite_water;  /* cells (air and wall) with a NaN or +-Inf in any channel */
  int64_t first_nonfinite_base_x, first_nonfinite_base_y;   /* the first such cell in order of the global index; -1, -1: none */
  int64_t first_nonfinite_water_x, first_nonfinite_water_y;
  double sum_base[4];         /* over the air cells: vx, vy, pressure, temperature */
  double sum_water[4];        /* over the air cells: total water, cloud water, precipitation (visual), smoke */
  double sum_soil_moisture;   /* over the wall cells: water.z */
  double sum_snow;            /* over the wall cells: water.w */
  int64_t sum_vegetation;     /* over the wall cells: wall channel 3 */
  double min_base[4], max_base[4], min_water[4], max_water[4]; /* over the air cells, NaNs skipped; NaN if there is no such value */
  int64_t min_base_x[4], min_base_y[4], max_base_x[4], max_base_y[4];     /* where each extreme FIRST occurs; -1, -1: none */
  int64_t min_water_x[4], min_water_y[4], max_water_x[4], max_water_y[4];
  int64_t n_droplets_active;    /* droplets with mass.x >= 0 (a slab counts the ones inside its owned columns that it tracks itself) */
  int64_t n_droplets_nonfinite; /* active droplets whose mass.x or mass.y is not finite */
  double sum_droplet_mass_x, sum_droplet_mass_y; /* over the active droplets: mass.x (water), mass.y (ice) */
} wx_diag;

/* What leaves the device: integers only, nothing rounded yet. A zero-filled wx_diag_raw is the empty set. Sums: a finite float is
 * m * 2^(e - 150) with an integer |m| < 2^24 and a biased exponent e in 1..254 (subnormals: e = 1, no hidden bit); quantity q keeps 16 integer
 * bins, bin e >> 4 receives m << (e & 15). A bin's value is hi * 2^32 + lo with 0 <= lo < 2^32 (one representation per value, so a merge
 * is associative and commutative bit for bit). Extremes: one 64-bit key per channel, order-preserving float bits above the inverted
 * global index, combined with max (the keys of the minima hold the inverted float order). */
#define WX_DIAG_QUANTITIES 12  /* 0-3 base, 4-7 water (air cells); 8 soil moisture, 9 snow (wall cells); 10 droplet mass.x, 11 droplet mass.y */
#define WX_DIAG_BINS 16
typedef struct wx_diag_raw {
  int64_t x_global, y_rows;   /* geometry the global indices refer to; 0: no device pass went into this yet */
  int64_t iter;
  int64_t count[10];          /* n_air, n_wall, n_marker_mismatch, n_negative_water, n_nonfinite_base, n_nonfinite_water, sum_vegetation,
                                 n_droplets_active, n_droplets_nonfinite, cells covered */
  uint64_t first_nonfinite[2]; /* base, water: ~global index, combined with max; 0: none */
  uint64_t key_max[8], key_min[8];
  int64_t bin_hi[WX_DIAG_QUANTITIES][WX_DIAG_BINS];
  uint64_t bin_lo[WX_DIAG_QUANTITIES][WX_DIAG_BINS];
} wx_diag_raw;

/* Device pass over this handle's owned columns, enqueued on the handle's stream behind the pending iterations; synchronous like
 * wx_read_rect, and like it the place where the iterations report WX_E_STATE. WX_E_STATE before wx_upload. */
int wx_diag_collect(wx_sim *s, wx_diag_raw *out);
/* Host only, pure: `into` becomes the union of two disjoint sets of cells of ONE domain (WX_E_INVALID if geometry or iteration differ). */
int wx_diag_merge(wx_diag_raw *into, const wx_diag_raw *other);
/* Host only, pure: combines the bins of every quantity in a 320-bit integer and rounds ONCE to double. */
int wx_diag_finish(const wx_diag_raw *raw, wx_diag *out);
/* Host only: adds n floats to the bins of `quantity` with the binning function the kernel uses (non-finite values are skipped). */
int wx_diag_accumulate(wx_diag_raw *into, int quantity, const float *values, size_t n);
/* Host only: the kernel's per-cell function over n cells of row y starting at global column x (base, water: 4 floats per cell, wall: 4
 * bytes per cell), for hosts that hold cells themselves and for tests without a GPU. Sets the geometry of an empty `into`. */
int wx_diag_accumulate_cells(wx_diag_raw *into, int x_global, int y_rows, int x, int y, int n, const float *base, const float *water, const int8_t *wall);
/* wx_diag_collect + wx_diag_finish. */
int wx_diagnostics(wx_sim *s, wx_diag *out);
/* Every slab of the group collects on its own device and stream; merged and finished: the numbers of the undecomposed domain (with
 * droplets: the pool protocol makes one slab THE owner of an active droplet at the iterations that end with an exchange -- every
 * wx_slab_period iterations of wx_group_step, or after wx_group_exchange; in between a droplet that crossed a slab edge may be counted by
 * neither or both). A failed slab reports through wx_group_last_error. */
int wx_group_diagnostics(wx_group *g, wx_diag *out);

/* ---- Ensembles: many independent simulations of one size, stepped in one launch (no reference counterpart: the reference runs one
 * simulation per page). A lone 100 x 100 grid is two strips and two dependent launches per iteration, a lone 2500 x 300 grid has to be cut
 * into 4-row segments to put a wave on every SIMD; a host that has MANY such grids -- a sweep over the sliders, a perturbed ensemble, a
 * fuzzer -- puts them into an ensemble: n_members whole-domain handles of X x Y cells on the current device, with or without droplets
 * (wx_ensemble_create_droplets: every member as from wx_create(X, Y, n_droplets); wx_ensemble_create: n_droplets = 0), whose iterations
 * share ONE marching launch and ONE fix launch per iteration and kernel instantiation, and whose particle passes share their launches too.
 *
 * A MEMBER IS AN ORDINARY HANDLE (wx_ensemble_member; borrowed, like wx_group_slab): wx_upload / wx_setup_* / wx_set_params / wx_set_option /
 * wx_set_iter / wx_read_rect / wx_diagnostics / wx_fastest_velocity exactly as on a handle from wx_create, and with droplets wx_upload /
 * wx_setup_* with a pool, wx_init_droplets, wx_read_particles, WX_OPT_SPLAT_ORDER, inactiveDroplets / enablePrecipitation of wx_set_params,
 * the droplet entries of wx_diagnostics and WX_FIELD_PRECIP_FB / _PRECIP_DEP / _LIGHTNING. After wx_ensemble_step(e, n)
 * every readable field, wx_get_iter, wx_diagnostics, wx_fastest_velocity and every reported error of member i are what a handle from
 * wx_create(X, Y, n_droplets) with the same uploads, parameters, options and iteration counter shows after wx_step(h, n), the
 * display-side fields (WX_FIELD_BASE_DISP, _WATER_0, _CURL, _WALL_DISP, _EMITTED) included: the last iteration of the call is the
 * display iteration for all members. Bit for bit where a lone handle is reproducible: always without droplets; with droplets the pool
 * always, and every readable field under WX_OPT_SPLAT_ORDER 1. Under the default order (fp32 atomics in arrival order) the pool after the
 * first iteration and whatever lone sprites make order-free are bit-identical, and the rest agrees to summation order -- exactly as two
 * runs of a lone handle do. Members differ freely in state, droplet pool, parameters (every uniform of wx_params, the sounding arrays,
 * wrapHorizontally, brush / airplane inputs), options, iteration counter and terrain.
 *
 * What is batched: the member-iterations the marching wet kernel would run on a lone handle (default kernel set, all grid passes). The
 * members of a call are partitioned by the instantiation they need -- a brush held on one member does not push the others into the general
 * instantiation --, one marching and one fix launch per iteration and non-empty partition; every member keeps its own exact-path list,
 * hint word, fastest-velocity word and overflow flag. (Whether a member hands in feedback textures -- its droplets ran in the iteration
 * before -- is part of the instantiation, as on a lone handle.) Of the batched members, those whose droplets run (WX_PASS_PRECIPITATION in
 * the pass mask, enablePrecipitation, n_droplets > 0) share the particle pass behind the fix launches: ONE launch each of the
 * precipitation, classify, box-sum and clear kernels per iteration, however many members -- every member keeps its own pool, device
 * state, accumulation grid and textures. Under WX_OPT_SPLAT_ORDER 1 a member's deposit records are sorted by its own radix sort and
 * added by its own run-sum launch between the shared launches (a per-member sort, not a segmented one: the mode is for tests, and any
 * stable sort gives the same bits); members of either order share the four launches. What is not batched: a member whose iterations do
 * not qualify (WX_PASS_DRY or any partial pass mask, WX_OPT_KERNEL_SET 0) runs n_iter iterations of its own path (wx_step), droplets
 * included, on the ensemble's stream, behind the batched members, in member order. wx_ensemble_stats counts both, so that a host can
 * see that the batch path ran: member-iterations batched / run solo and marching launches issued, since the ensemble was created (any
 * pointer may be NULL). wx_ensemble_particle_stats counts the member-iterations whose particle pass was shared and the particle launches
 * issued for them (4 per iteration, + 2 per order-1 member: its sort and its run sums), likewise.
 *
 * An error is the member's: an overflowed exact-path list of member 3 is reported (WX_E_STATE) by member 3's next blocking call or by
 * wx_ensemble_sync / wx_ensemble_diagnostics -- whichever looks first consumes the report, as on a lone handle --, and
 * wx_ensemble_last_error names the member ("member 3: ..."); the other members' results are unaffected. A failed launch names the
 * members of its partition. A wx_ensemble_step that fails half-way (WX_E_DEVICE / WX_E_NOMEM) leaves the ensemble unusable: every later
 * wx_ensemble_step returns WX_E_STATE with the message of that failure. wx_ensemble_diagnostics fills n_members entries of `out`.
 *
 * All members live on the device that was current at wx_ensemble_create and share one stream owned by the ensemble: wx_set_stream /
 * wx_set_comm_stream / wx_tune_placement on a member return WX_E_STATE, and the implicit placement search never runs on a member (as on a
 * slab). wx_step on a member stays legal and means what it always meant. wx_ensemble_step is asynchronous like wx_step; wx_profile on a
 * member does not see the shared launches. wx_ensemble_destroy destroys the member handles too (do not wx_destroy them).
 * Refused with WX_E_INVALID: n_members < 1 or > 65535, n_droplets < 0; there are no slab members, no members of different sizes or
 * droplet counts (there is no way to add a handle to an ensemble). WX_OPT_CHECK_LAUNCHES on any batched member synchronises behind the
 * particle launches too. Not batched yet: the water-free dry kernels. */
#define WX_HAVE_ENSEMBLE 1
#define WX_HAVE_ENSEMBLE_DROPLETS 1
typedef struct wx_ensemble wx_ensemble;
int wx_ensemble_create(int n_members, int X, int Y, wx_ensemble **out);
int wx_ensemble_create_droplets(int n_members, int X, int Y, int n_droplets, wx_ensemble **out);
void wx_ensemble_destroy(wx_ensemble *e);
const char *wx_ensemble_last_error(const wx_ensemble *e); /* also valid with e == NULL for create failures */
int wx_ensemble_count(const wx_ensemble *e);
wx_sim *wx_ensemble_member(wx_ensemble *e, int i);
int wx_ensemble_step(wx_ensemble *e, int n_iter);
int wx_ensemble_sync(wx_ensemble *e);
int wx_ensemble_diagnostics(wx_ensemble *e, wx_diag *out);
int wx_ensemble_stats(wx_ensemble *e, int64_t *member_iters_batched, int64_t *member_iters_solo, int64_t *march_launches);
int wx_ensemble_particle_stats(wx_ensemble *e, int64_t *member_iters_particles_batched, int64_t *particle_launches);

/* ---- Ensemble statistics: per cell of a rectangle the mean, spread, extremes and exceedance count OVER THE MEMBERS, computed on the
 * device in one launch (no reference counterpart). What wx_diag is for the space axis this is for the member axis: without it every
 * per-cell look at an ensemble is n_members wx_read_rect calls and host arithmetic.
 *
 * THE PER-CELL FUNCTION (the kernel, wx_ens_stat_cells and the tests all evaluate this definition). For cell (x, y) and channel c take
 * the selected members in MEMBER ORDER, 0 first.
 *   Which values enter. A member in which the cell is a WALL cell -- wx_diag's test: channel 1 of its WX_FIELD_WALL_CUR texel is 0 --
 *   counts into n_wall and contributes nothing. Of the remaining values the FINITE ones enter, and `count` counts them; NaN and +-Inf
 *   do not enter (their number is: selected members - n_wall - count).
 *   Sums. n = count. S = the entered values converted to double and added one at a time in member order, every addition rounded to
 *   double. m = S / n in double; mean = (float)m. Q = the sum, in the same order, of d * d with d = (double)v - m, the product and the
 *   addition rounded separately (no fused multiply-add); variance = (float)(Q / n), the POPULATION variance. n = 0: mean and variance
 *   are NaN.
 *   Extremes. min and max over the entered values; -0.0 and 0.0 compare equal, a zero extreme is reported as +0.0; among equal values
 *   the smallest member index wins (argmin / argmax: the member's index in the ensemble -- in `field` for wx_ens_stat_cells --, not
 *   its position in the selection). n = 0: min and max are NaN, argmin and argmax -1.
 *   Exceedance. n_above = the number of entered values with v > threshold[c]; a NaN threshold gives 0. Probabilities are left to the
 *   host: an integer is exact.
 * These are NOT math.fsum sums like wx_diag's: they are sums IN A FIXED ORDER, and the result depends on that order (1e30, 1, -1e30, 1
 * sums to 1, sorted to 0). An exact sum needs a 320-bit accumulator per quantity -- per cell and channel that is more memory than the
 * fields it summarises. The order is part of the definition instead, the function is evaluated with floating-point contraction off
 * in every build, and libwxsim.so, libwxsim_fast.so, the device and the host give the same bits.
 *
 * wx_ensemble_statistics: `field` is WX_FIELD_BASE_CUR or WX_FIELD_WATER_CUR (the fields that are stored whole and interleaved, the
 * ones wx_diag covers; any other: WX_E_INVALID), the rectangle lies inside the grid (no wrap, as wx_read_rect: WX_E_RANGE),
 * member_mask has one byte per member, non-zero = selected, NULL = all (nobody selected: WX_E_INVALID; a selected member that was
 * never uploaded: WX_E_STATE, the message names it); e or out NULL: WX_E_INVALID. These checks answer before the device is touched.
 * The work is enqueued on the ensemble's stream behind everything pending -- the members' pointers are taken at the time of the call
 * --, and the call then BLOCKS like wx_ensemble_sync; like it, it is a place where a member's pending report (an overflowed
 * exact-path list, ...) is consumed and returned ("member i: ...") instead of numbers. It changes nothing: not the members' fields,
 * not the fields that are made on demand, not the iteration counters, the diagnostics or wx_ensemble_stats. The device buffers (a
 * table of the selected members, the wanted planes of the rectangle and their pinned copy) belong to the ensemble, are made by the
 * first call, grow on demand and go with wx_ensemble_destroy. wx_profile on member 0 times the launch, whoever is selected (kernel name
 * "ensemble_statistics"). The kernel takes one lane per cell and walks the members serially, as
 * the definition demands: a small rectangle under-fills the chip whatever the number of members. */
#define WX_HAVE_ENSEMBLE_STATISTICS 1
typedef struct wx_ens_stat {      /* caller-owned host arrays over the rectangle, rows bottom-up; any pointer may be NULL (not wanted) */
  float   *mean, *variance;       /* w*h*4, channel-interleaved like the field */
  float   *min, *max;             /* w*h*4 */
  int32_t *argmin, *argmax;       /* w*h*4: member index of the extreme; -1: none */
  int32_t *count;                 /* w*h*4: values that entered (see above) */
  int32_t *n_above;               /* w*h*4: entered values with v > threshold[c] */
  int32_t *n_wall;                /* w*h:   selected members in which the cell is a wall cell */
  float    threshold[4];
} wx_ens_stat;

int wx_ensemble_statistics(wx_ensemble *e, int field, int x, int y, int w, int h,
                           const uint8_t *member_mask /* n_members bytes, NULL = all */, wx_ens_stat *out);
/* host only, pure: the kernel's per-cell function over n_cells cells held by the caller, member i's cells at field[i] (4 floats per cell) /
 * wall[i] (4 bytes per cell); outputs as above with w*h = n_cells. WX_E_INVALID: n_members < 1, a NULL table or output struct, a NULL
 * entry of a selected member, nobody selected. */
int wx_ens_stat_cells(int n_members, size_t n_cells, const float *const *field, const int8_t *const *wall,
                      const uint8_t *member_mask, wx_ens_stat *out);

/* ---- (ABI 11, WX_HAVE_STATE_COPY) A complete device-side clone: after wx_copy_state(dst, src) dst IS src's simulation, for everything a
 * host can observe -- every readable WX_FIELD_* (the ones made on demand included: WATER_0, BASE_DISP, EMITTED, PRECIP_FB; CURL, both
 * light textures, LIGHTNING), the droplet pool wx_read_particles returns, wx_get_iter, wx_diagnostics, the inactive-droplet count, the
 * parameters and sounding arrays of the last wx_set_params -- and every later wx_step(dst, n) / wx_ensemble_step yields bit for bit what
 * the same call on src yields (droplets: as between two runs of one handle -- the pool always, everything under WX_OPT_SPLAT_ORDER 1).
 * wx_upload cannot do this: it resets the light textures, curl, the feedback textures, the lightning state and `even`, so a handle
 * "uploaded from" another's wx_read_rect output diverges from the first iteration. A spun-up simulation is handed to the members of an
 * ensemble, a fuzzer or a what-if host branches a run, a checkpoint is a second handle.
 * Which handles: two whole-domain handles (no halo) of the same X, Y and droplet count on the same device; each a lone handle or a
 * member of any ensemble. WX_E_INVALID: a NULL argument (answered before the device is touched), a geometry or droplet-count mismatch,
 * a slab handle, handles on different devices. WX_E_STATE: src was never uploaded, or src has no parameters (the message says which).
 * dst == src: WX_OK, nothing done. dst may never have been uploaded.
 * OPTIONS ARE NOT COPIED: dst goes on under its own, as if they had been set by wx_set_option mid-run; streams, profile, placement and
 * ensemble membership stay dst's. The counters that describe a handle's own launches -- wx_fastest_velocity, wx_pair_stats, the profile
 * accumulators, wx_ensemble_stats -- are not state: dst's read as after a fresh upload (the profile's and the ensemble's are left
 * alone), src's are untouched. src is unchanged in every observable respect.
 * Ordering: the two handles may be on different streams; the copy is ordered behind everything pending on both, and the call blocks
 * like wx_sync on both. It is a place where src's pending report (an overflowed exact-path list, ...) is consumed and returned
 * (WX_E_STATE, on both handles' wx_last_error): then nothing is copied and dst keeps its state. Device pointers obtained from
 * wx_device_ptr(dst, ..) before the call are invalid afterwards. A device error half-way (WX_E_DEVICE / WX_E_NOMEM) leaves dst's
 * contents undefined until it is uploaded or copied into again.
 * wx_ensemble_broadcast(e, src_member, member_mask): the same copy from one member to every selected other member (member_mask: one
 * byte per member, non-zero = selected, NULL = all others; the source's own byte is ignored), enqueued on the ensemble's stream with one
 * wait at the end (the source's pending report is looked at first, as above). Members outside the mask are untouched; wx_ensemble_stats
 * is unchanged. WX_E_INVALID: e NULL, src_member outside the ensemble; WX_E_STATE: the source was never uploaded or has no parameters. */
#define WX_HAVE_STATE_COPY 1
int wx_copy_state(wx_sim *dst, wx_sim *src);
int wx_ensemble_broadcast(wx_ensemble *e, int src_member, const uint8_t *member_mask);

/* ---- (ABI 11, WX_HAVE_ENSEMBLE_PERTURB) The members of an ensemble made different in one launch: smooth pseudo-random noise added to
 * (or multiplied into) one field of every selected member, on the device. With wx_ensemble_broadcast a perturbed ensemble starts from a
 * spun-up state without one host array: spin up, clone, perturb, step, wx_ensemble_statistics.
 *
 * THE PER-CELL FUNCTION (the kernel, wx_ens_perturb_cells and the tests all evaluate this definition). All integer arithmetic is
 * wrapping uint32, all floating-point arithmetic is double with every operation rounded separately (no fused multiply-add: contraction
 * is off inside the function in every build, so libwxsim.so, libwxsim_fast.so, the device and the host give the same bits).
 *   Node value. hash_u32 is the shaders' integer hash (common.glsl:103-111, the one wx_init_droplets uses). For member index i (its
 *   index in the ensemble -- in `field` for wx_ens_perturb_cells --, not its position in the mask), channel c and lattice node (gx, gy):
 *     h = hash_u32(gx + hash_u32(gy + hash_u32(4*i + c + hash_u32(seed))));   u = ((double)(h >> 8) - 8388608.0) / 8388608.0   in [-1, 1).
 *   Noise at the absolute cell (x, y). gx = x / scale, gy = y / scale (integer division); tx = (double)(x - gx*scale) / (double)len,
 *   ty = (double)(y - gy*scale) / (double)scale; len = scale and the right-hand node is gx + 1 -- except with wrap_x in the last node
 *   interval of a row, gx == (X - 1) / scale: there len = X - gx*scale (possibly shorter) and the right-hand node is node 0, so the
 *   noise is periodic in x with the grid's width X. The upper node is gy + 1. With u00 = u(gx, gy), u10 = u(right, gy), u01 = u(gx, gy+1),
 *   u11 = u(right, gy+1):   r = (1-ty)*((1-tx)*u00 + tx*u10) + ty*((1-tx)*u01 + tx*u11)   -- two subtractions, six products, three sums.
 *   Application to the value v of a channel with amplitude a.  mode 0: d = (double)v + (double)a*r.  mode 1: d = (double)v * (1.0 +
 *   (double)a*r).  o = (float)d; then the clamp: if lo[c] is not NaN and o < lo[c], o = lo[c]; then if hi[c] is not NaN and o > hi[c],
 *   o = hi[c]. The channel becomes o.
 *   What is left untouched, bit for bit: every channel of a cell that is a WALL cell in that member (wx_diag's test: channel 1 of its
 *   WX_FIELD_WALL_CUR texel is 0); a channel with a == 0; a channel whose v is not finite; a channel whose o is not finite (an overflow,
 *   a NaN amplitude, an infinite clamp).
 * The noise is a function of absolute coordinates, member, channel and seed only -- not of the rectangle or the mask: perturbing two
 * disjoint rectangles equals perturbing their union, and a member's noise is the same whoever else is selected.
 *
 * wx_ensemble_perturb: WX_E_INVALID: e or p NULL, a field other than WX_FIELD_BASE_CUR / WX_FIELD_WATER_CUR, mode not 0 or 1, scale < 1,
 * nobody selected; WX_E_RANGE: the rectangle does not lie inside the grid (no wrap); WX_E_STATE: a selected member was never uploaded
 * (the message names it). These checks answer before the device is touched; member_mask as for wx_ensemble_statistics. To a member's
 * bookkeeping the perturbation is a host write through wx_device_ptr: a lazy WX_FIELD_BASE_DISP is assembled whole first and a pending
 * WX_FIELD_WATER_0 is made first (the display-side fields keep showing the last display iteration), velocities written are looked at by
 * the next |vx| scan, and a perturbed water field is no longer known to be water-free (wx_water_free: 0; the water-free dry kernel
 * does not run on it). The launch is enqueued on the ensemble's stream behind everything pending, and the call then BLOCKS like
 * wx_ensemble_statistics and, like it, consumes and returns a member's pending report ("member i: ..."; the perturbation has been
 * applied by then). wx_profile on member 0 times the launch (kernel name "ensemble_perturb"). The kernel takes one lane per cell and
 * member: 36 B per member-cell, DESIGN.md section 4.
 * wx_ens_perturb_cells (host only, pure): the same function over cells the caller holds -- member i's w*h cells of the rectangle
 * (p->x, p->y, p->w, p->h) of an X x Y grid at field[i] (4 floats per cell, rows bottom-up, changed in place) and wall[i] (4 bytes per
 * cell). WX_E_INVALID / WX_E_RANGE as above, and for n_members < 1, a NULL table, a NULL entry of a selected member. */
#define WX_HAVE_ENSEMBLE_PERTURB 1
typedef struct wx_ens_perturb {
  int32_t  field;          /* WX_FIELD_BASE_CUR or WX_FIELD_WATER_CUR (the fields wx_ensemble_statistics reads) */
  int32_t  x, y, w, h;     /* rectangle inside the grid, no wrap (WX_E_RANGE) */
  int32_t  mode;           /* 0: v + a*r     1: v * (1 + a*r) */
  int32_t  scale;          /* >= 1: lattice pitch of the noise in cells; 1 = white noise */
  int32_t  wrap_x;         /* the noise is periodic across x = 0 (for wrapHorizontally domains) */
  uint32_t seed;
  float    amplitude[4];   /* per channel; 0: the channel's bits are not touched */
  float    lo[4], hi[4];   /* clamp of the result; NaN: none */
} wx_ens_perturb;
int wx_ensemble_perturb(wx_ensemble *e, const wx_ens_perturb *p, const uint8_t *member_mask /* n_members bytes, NULL = all */);
int wx_ens_perturb_cells(const wx_ens_perturb *p, int X, int Y, int n_members, float *const *field, const int8_t *const *wall,
                         const uint8_t *member_mask);

/* ---- (ABI 11, WX_HAVE_ENSEMBLE_QUANTILES) Order statistics over the members: per cell of a rectangle up to WX_ENS_QUANT_MAX quantiles
 * of the members' values -- the median, the 10 / 90 % band, the inter-quartile range -- and the RANK of one member's value among the
 * others' (rank histograms, spread-skill), computed on the device in one launch. A call of its own next to wx_ensemble_statistics:
 * wx_ens_stat and its planes are unchanged.
 *
 * THE PER-CELL FUNCTION (the kernels, wx_ens_quant_cells and the tests all evaluate this definition). For cell (x, y) and channel c:
 *   Which values enter. Exactly as in wx_ensemble_statistics: a selected member in which the cell is a WALL cell (channel 1 of its
 *   WX_FIELD_WALL_CUR texel is 0) counts into n_wall and contributes nothing; of the remaining values the FINITE ones enter, and
 *   `count` = n counts them. An entered -0.0 is taken as +0.0. v(0) <= v(1) <= ... <= v(n-1) are the entered values in ascending order.
 *   Quantile p (a float in [0, 1]). h = (double)p * (double)(n - 1), one rounded product; k = floor(h), g = h - k (exact),
 *   k1 = min(k + 1, n - 1).
 *     WX_QUANT_LOWER:  v(k).
 *     WX_QUANT_HIGHER: g > 0 ? v(k1) : v(k).
 *     WX_QUANT_LINEAR: (float)((double)v(k) + g * ((double)v(k1) - (double)v(k))) -- the difference, the product and the sum are
 *     rounded to double separately (no fused multiply-add: contraction is off inside the function in every build, so libwxsim.so,
 *     libwxsim_fast.so, the device and the host give the same bits), the conversion to float happens once. This is not numpy's lerp.
 *     n = 0: NaN.
 *   Rank. t = the value of member `rank_member` in that cell and channel. If the cell is a wall cell in that member, or t is not
 *   finite: n_below = n_equal = -1. Otherwise n_below = the number of entered values with v < t, n_equal = the number with v == t
 *   (float compare: -0.0 == 0.0). Rank histograms and the breaking of ties are left to the host: integers are exact.
 * NO SUM IN MEMBER ORDER OCCURS ANYWHERE: unlike wx_ensemble_statistics the result does not depend on the order of the members --
 * the same members uploaded in another order give the same bits.
 *
 * wx_ensemble_quantiles. Answered before the device is touched -- WX_E_INVALID: e or out NULL; a field other than WX_FIELD_BASE_CUR /
 * WX_FIELD_WATER_CUR; n_q outside 0 .. WX_ENS_QUANT_MAX; n_q > 0 with q == NULL; a p that is NaN or outside [0, 1]; an unknown interp;
 * nobody selected; rank_member outside the ensemble (other than -1) or selected by the mask (the ranked member does not enter: mask it
 * out); n_below or n_equal non-NULL with rank_member == -1. WX_E_RANGE: the rectangle does not lie inside the grid (no wrap).
 * WX_E_STATE: a selected member, or rank_member, was never uploaded (the message names it). Everything else as for
 * wx_ensemble_statistics: member_mask has one byte per member (NULL = all), the work is enqueued on the ensemble's stream behind
 * everything pending with the members' pointers taken at the time of the call, the call then BLOCKS like wx_ensemble_sync and consumes
 * and returns a member's pending report ("member i: ..."), it changes nothing, its device buffers belong to the ensemble and go with
 * wx_ensemble_destroy, and wx_profile on member 0 times the launch (kernel name "ensemble_quantiles"). Up to
 * wx_ens_quant_staged_members() selected members the kernel reads every member once, through LDS, and sorts in registers; beyond that
 * (up to all 65535) a streaming kernel selects the order statistics in 33 passes over the members: slow, correct.
 * wx_ens_quant_cells (host only, pure): the same function over n_cells cells the caller holds, member i's cells at field[i] (4 floats
 * per cell) / wall[i] (4 bytes per cell), rank_member an index into these tables; outputs as above with w*h = n_cells. WX_E_INVALID
 * as above, and for n_members < 1, a NULL table or output struct, a NULL entry of a selected member or of rank_member. */
#define WX_HAVE_ENSEMBLE_QUANTILES 1
#define WX_ENS_QUANT_MAX 8
#define WX_QUANT_LINEAR 0
#define WX_QUANT_LOWER  1
#define WX_QUANT_HIGHER 2
typedef struct wx_ens_quant {
  int32_t  n_q;                    /* 0 .. WX_ENS_QUANT_MAX */
  int32_t  interp;                 /* WX_QUANT_* */
  float    p[WX_ENS_QUANT_MAX];    /* each finite, in [0, 1] */
  int32_t  rank_member;            /* -1: none; else a member that is NOT selected */
  float   *q;                      /* n_q planes of w*h*4, plane j = quantile p[j]; NULL: not wanted */
  int32_t *count;                  /* w*h*4, as wx_ens_stat.count */
  int32_t *n_wall;                 /* w*h,   as wx_ens_stat.n_wall */
  int32_t *n_below, *n_equal;      /* w*h*4, only with rank_member >= 0 */
} wx_ens_quant;
int wx_ensemble_quantiles(wx_ensemble *e, int field, int x, int y, int w, int h,
                          const uint8_t *member_mask /* n_members bytes, NULL = all */, wx_ens_quant *out);
int wx_ens_quant_cells(int n_members, size_t n_cells, const float *const *field, const int8_t *const *wall,
                       const uint8_t *member_mask, wx_ens_quant *out);
int wx_ens_quant_staged_members(void);  /* largest number of selected members the LDS path takes */

/* ---- (ABI 11, WX_HAVE_ENSEMBLE_ASSIMILATE) Point observations assimilated into the members on the device: the ensemble Kalman analysis
 * that closes the loop perturb -> step -> statistics / quantiles. A host that holds observations (stations on a nature run, a sounding)
 * pulls the selected members towards them without one host array and without wx_upload, which would reset light, curl, the feedback
 * textures and the lightning state. A serial ensemble square-root filter (EnSRF, Whitaker and Hamill 2002) with separable Gaspari-Cohn
 * localization in x and in height, defined bit for bit, in three launches at most whatever the number of observations.
 *
 * THE DEFINITION (the kernels, wx_ens_assim_cells and the tests all evaluate it). All arithmetic is double, every operation rounded
 * separately (no fused multiply-add: contraction is off inside every function that rounds, and every product that feeds a sum or a
 * difference is a value of its own in every build, so libwxsim.so, libwxsim_fast.so, the device and the host give the same bits). "In
 * member order": the n selected members k = 0 .. n-1 by ascending member index.
 *   Order. Observations are taken in order, j = 0 first; observation j sees the members' values as observations 0 .. j-1 left them.
 *   Prior of observation j. t_k = channel `channel` of cell (x, y) of `field` in member k. The observation is SKIPPED (applied = 0, its
 *   result doubles NaN, nothing changes) unless in every selected member that cell is an air cell (channel 1 of its WX_FIELD_WALL_CUR
 *   texel != 0: wx_diag's test) and t_k is finite. Otherwise S = sum (double)t_k in member order, hm = S / n, e_k = (double)t_k - hm,
 *   Q = sum e_k*e_k in member order, V = Q / (n - 1), D = V + (double)R, innovation = (double)value - hm,
 *   alpha = 1 / (1 + sqrt((double)R / D)) with the correctly rounded double square root.
 *   Localization weight of cell (x, y). dx = |x - ox|, with wrap_x dx = min(dx, X - dx); dy = |y - oy|. Per axis the factor is 1 if that
 *   axis's loc is 0, else G((double)d / (double)loc), G by Horner with the double constants 5.0/3.0, 1.0/12.0, 2.0/3.0 as those C
 *   expressions:   0 <= z <= 1: p = -0.25*z + 0.5; p = p*z + 0.625; p = p*z - 5.0/3.0; p = p*z; p = p*z + 1.0
 *                  1 < z < 2:   p = (1.0/12.0)*z - 0.5; p = p*z + 0.625; p = p*z + 5.0/3.0; p = p*z - 5.0; p = p*z + 4.0; p = p - (2.0/3.0)/z
 *                  z >= 2: 0.   A negative p is 0.     rho = Gx * Gy, one rounded product. (Separable and anisotropic on purpose: the
 *   grid is a vertical slice, horizontal and vertical length scales differ, and no cell needs a square root.)
 *   Per cell of the rectangle, state field F in {BASE_CUR, WATER_CUR} (not necessarily the observed one) and channel c with
 *   g = gain_F[c] != 0: if rho == 0 the channel is untouched. It is updated only if in every selected member the cell is an air cell and
 *   the value x_k is finite, else untouched in all members. Sx = sum (double)x_k in member order, xm = Sx / n, d_k = (double)x_k - xm,
 *   Cq = sum d_k*e_k in member order, C = Cq / (n - 1), w = (double)g * rho, K = (w * C) / D. If K == 0 or K is not finite the channel is
 *   untouched (so a -0.0 never becomes +0.0 by a zero increment). Otherwise a = K * innovation, b = alpha * K and for every member
 *   o_k = (float)((double)x_k + (a - b*e_k)), then wx_ens_perturb's clamp (lo first, then hi, NaN = none); if o_k is not finite that
 *   member's channel keeps its bits.
 * Cells never interact within one observation, and an observation may lie outside the rectangle: its prior is read, its cell is never
 * changed. A cell's result depends on the rectangle only through the priors: two rectangles that hold the same observed cells give
 * their common cells the same bits.
 *
 * wx_ensemble_assimilate. Answered before the device is touched -- WX_E_INVALID: e, a or obs NULL; n_obs outside 1 .. WX_ENS_OBS_MAX; an
 * observation's field other than WX_FIELD_BASE_CUR / WX_FIELD_WATER_CUR or channel outside 0 .. 3; a value, error_var, loc or gain that
 * is not finite; error_var <= 0; loc < 0; fewer than two selected members. WX_E_RANGE: the rectangle or an observation outside the grid.
 * WX_E_STATE: a selected member was never uploaded (the message names it). Ordering, blocking, error reports and bookkeeping as for
 * wx_ensemble_perturb, for every selected member and every state field with a non-zero gain: a lazy WX_FIELD_BASE_DISP is assembled
 * whole first, a pending WX_FIELD_WATER_0 is made first, velocities written are looked at by the next |vx| scan, an updated water field
 * is no longer known to be water-free. With all gains 0 the call is legal: it fills `result` and changes nothing. `result` (n_obs entries
 * or NULL) is computed on the device and copied back once. Launches: "ensemble_assimilate_obs" once -- the chain of priors in observation
 * space, on working copies of the observed channels --, then "ensemble_assimilate" once per state field with a non-zero gain (wx_profile
 * on member 0 times both); DESIGN.md section 4.
 * wx_ens_assim_cells (host only, pure): the serial definition, literally, over WHOLE X x Y grids the caller holds (an observation may lie
 * outside the rectangle) -- member i's cells at base[i] / water[i] (4 floats per cell, rows bottom-up, changed in place) and wall[i]
 * (4 bytes per cell). WX_E_INVALID / WX_E_RANGE as above, and for n_members < 1, a NULL table, a NULL entry of a selected member. */
#define WX_HAVE_ENSEMBLE_ASSIMILATE 1
#define WX_ENS_OBS_MAX 256
typedef struct wx_ens_obs {        /* one scalar observation of one channel of one cell */
  int32_t field;                   /* WX_FIELD_BASE_CUR or WX_FIELD_WATER_CUR */
  int32_t x, y, channel;           /* inside the grid (WX_E_RANGE), channel 0..3 */
  float   value;                   /* finite */
  float   error_var;               /* R: finite, > 0 */
} wx_ens_obs;
typedef struct wx_ens_obs_result { /* one per observation, filled by the call (computed on the device by wx_ensemble_assimilate) */
  int32_t applied, pad;            /* 1: used; 0: skipped (see above), the doubles are then NaN */
  double  prior_mean, prior_var, innovation, alpha;
} wx_ens_obs_result;
typedef struct wx_ens_assim {
  int32_t x, y, w, h;              /* the cells that may be changed; no wrap (WX_E_RANGE) */
  int32_t wrap_x;                  /* distances in x are taken around the grid's width */
  float   loc_x, loc_y;            /* localization half-widths in cells, finite, >= 0; 0: no localization along that axis */
  float   gain_base[4], gain_water[4];  /* per channel of the two state fields; 0: the channel's bits are not touched; 1: the full update */
  float   lo_base[4], hi_base[4], lo_water[4], hi_water[4];  /* clamp of the result, NaN: none (as wx_ens_perturb) */
} wx_ens_assim;
int wx_ensemble_assimilate(wx_ensemble *e, const wx_ens_assim *a, int n_obs, const wx_ens_obs *obs,
                           wx_ens_obs_result *result /* n_obs entries or NULL */, const uint8_t *member_mask);
int wx_ens_assim_cells(const wx_ens_assim *a, int n_obs, const wx_ens_obs *obs, wx_ens_obs_result *result, int X, int Y, int n_members,
                       float *const *base, float *const *water, const int8_t *const *wall, const uint8_t *member_mask);

/* ---- (ABI 11, WX_HAVE_ENSEMBLE_SCORES) The members scored against a truth run on the device: what an observing-system experiment
 * asks after every cycle -- did the ensemble get closer to the nature run, and is its spread honest? One call reads the selected
 * members and the truth once and returns, per channel, the exact domain sums of error, absolute error, squared error, ensemble
 * variance and CRPS, two rank histograms and the counts that go with them: a few hundred bytes instead of a dozen planes. The result
 * does not depend on the order of the members, the launch shape or the build.
 *
 * THE PER-CELL FUNCTION (the kernel, wx_ens_score_cells and the tests all evaluate this definition). For cell (x, y) and channel c:
 *   Which values enter. Exactly as in wx_ensemble_quantiles, with the same keys: a selected member in which the cell is a wall cell
 *   contributes nothing, of the remaining values the FINITE ones enter, an entered -0.0 is taken as +0.0. n counts them and
 *   v(0) <= v(1) <= ... <= v(n-1) are the entered values in ascending order.
 *   Truth. t = channel c of the same cell of `truth`'s `field`, -0.0 taken as +0.0.
 *   When a cell-channel is scored. All three must hold, otherwise it is counted in exactly ONE of the reason counters, tested in this
 *   order: (1) the cell is an air cell in `truth` (channel 1 of its WX_FIELD_WALL_CUR texel != 0) and t is finite -- else
 *   n_truth_excluded; (2) n >= 1 -- else n_empty; (3) all five per-cell floats below are finite -- else n_overflow.
 *   Per-cell arithmetic. All arithmetic is double, every operation rounded separately (no fused multiply-add: contraction is off inside
 *   every function that rounds and every product that feeds a sum is a value of its own in every build, so libwxsim.so,
 *   libwxsim_fast.so, the device and the host give the same bits). All sums start at +0.0 and run in ASCENDING order of the values,
 *   i = 0 first -- not in member order.
 *     u_i = (double)v(i) - (double)t
 *     S = sum (double)v(i);  m = S / n;  err = m - (double)t
 *     Q = sum d_i*d_i with d_i = (double)v(i) - m;  var = Q / n -- the POPULATION variance. Its bits differ from the variance plane of
 *       wx_ensemble_statistics, which sums in member order.
 *     A = sum |u_i|;  G = sum (double)(2*i - n + 1) * u_i;  crps = A / n - G / ((double)n * (double)n) -- the standard ensemble CRPS,
 *       mean |x - t| - 1/(2 n^2) sum sum |x_i - x_j|, the double sum taken over the sorted values. No clamp at 0. With identical members
 *       equal to t, G is exactly 0 and crps is +0.0.
 *     The five floats: e = (float)err, ae = (float)fabs(err), se = (float)(err*err), vr = (float)var, cr = (float)crps.
 *   Rank. n_below = the number of entered values with v < t, n_equal = the number with v == t (the quantile call's float compare:
 *   -0.0 == 0.0). Each scored cell-channel adds 1 to rank_low[c][n_below] and 1 to rank_high[c][n_below + n_equal]: an untied cell lands
 *   in the same bin of both. How ties are split between the two is the host's business: integers are exact.
 *   Domain sums. Per channel, over the scored cell-channels: sum_error, sum_abs_error, sum_sq_error, sum_variance and sum_crps are the
 *   EXACT sums of the floats e, ae, se, vr, cr, rounded to double once -- the correctly rounded double of the exact sum, what Python's
 *   math.fsum returns -- taken with wx_diag's integer bins and its 320-bit finish. n_scored[c] counts the scored cell-channels,
 *   sum_count[c] is the sum of their n.
 *   The optional maps error, variance, crps (w*h*4 each) hold e, vr, cr, NaN where the cell-channel is not scored.
 *
 * wx_ensemble_scores. Answered before the device is touched -- WX_E_INVALID: e, truth or out NULL; a field other than WX_FIELD_BASE_CUR /
 * WX_FIELD_WATER_CUR; nobody selected; more than wx_ens_score_max_members() selected (the message says so: a streaming path can follow);
 * `truth` is a selected member of e; `truth` is a slab handle, a handle of another X or Y, or a handle on another device. WX_E_RANGE: the
 * rectangle does not lie inside the grid (no wrap). WX_E_STATE: a selected member, or `truth`, was never uploaded (the message names it).
 * `truth` is any whole-domain handle: a lone one, an unselected member of e, a member of another ensemble. The work is ordered behind
 * everything pending on the ensemble's stream AND on truth's stream, as wx_copy_state orders two handles: truth's pending report is
 * consumed and returned first ("truth: ..."), and then nothing is launched. Everything else as for wx_ensemble_quantiles: member_mask has
 * one byte per member (NULL = all), the members' pointers are taken at the time of the call, the call BLOCKS like wx_ensemble_sync and
 * consumes and returns a member's pending report ("member i: ..."), it changes nothing, its device buffers belong to the ensemble and go
 * with wx_ensemble_destroy, and wx_profile on member 0 times the launch (kernel name "ensemble_scores").
 * wx_ens_score_cells (host only, pure): the same function over n_cells cells the caller holds, member i's cells at field[i] (4 floats
 * per cell) / wall[i] (4 bytes per cell), the truth's at truth_field / truth_wall; maps as above with w*h = n_cells. WX_E_INVALID as
 * above, and for n_members < 1, a NULL table, truth array or output struct, a NULL entry of a selected member. */
#define WX_HAVE_ENSEMBLE_SCORES 1
#define WX_ENS_SCORE_BINS 65       /* n_below and n_below + n_equal lie in 0 .. wx_ens_score_max_members() */
typedef struct wx_ens_score {
  int64_t n_scored[4], n_truth_excluded[4], n_empty[4], n_overflow[4], sum_count[4];
  double  sum_error[4], sum_abs_error[4], sum_sq_error[4], sum_variance[4], sum_crps[4];
  int64_t rank_low[4][WX_ENS_SCORE_BINS], rank_high[4][WX_ENS_SCORE_BINS];
  float  *error, *variance, *crps; /* optional w*h*4 maps, NaN where the cell-channel is not scored; NULL: not wanted */
} wx_ens_score;
int wx_ensemble_scores(wx_ensemble *e, wx_sim *truth, int field, int x, int y, int w, int h,
                       const uint8_t *member_mask /* n_members bytes, NULL = all */, wx_ens_score *out);
int wx_ens_score_cells(int n_members, size_t n_cells, const float *const *field, const int8_t *const *wall,
                       const float *truth_field, const int8_t *truth_wall, const uint8_t *member_mask, wx_ens_score *out);
int wx_ens_score_max_members(void);  /* == wx_ens_quant_staged_members() */

/* ---- (ABI 11, WX_HAVE_ENSEMBLE_INFLATE) Covariance inflation and relaxation to the prior, on the device: the step of a cycling filter
 * that puts back the spread wx_ensemble_assimilate removes. A square-root filter with localization under-estimates its analysis
 * variance; without inflation the spread collapses, the members stop listening to observations and the rank histograms of
 * wx_ensemble_scores go U-shaped. (wx_ensemble_perturb in mode 1 is NOT inflation: v * (1 + a r) scales the whole value by a noise
 * field, moves the mean and knows nothing of the spread the analysis took away.) Three schemes, one launch, no host array and no
 * wx_upload: WX_INFLATE_CONST, multiplicative inflation about the ensemble mean; WX_INFLATE_RTPS, relaxation to prior spread (Whitaker
 * and Hamill 2012); WX_INFLATE_RTPP, relaxation to prior perturbations (Zhang et al. 2004). The two relaxation schemes read the prior
 * from a device-side snapshot that the host takes with wx_ensemble_prior_save before the analysis.
 *
 * THE SNAPSHOT. wx_ensemble_prior_save copies the rectangle of `field` of every selected member into a buffer the ensemble owns, laid
 * out [k][h][w] texels of 4 floats (k: position among the selected members, ascending member index): n * w * h * 16 bytes -- 10 MB for
 * 64 members of 100 x 100, 96 MB for 8 of 2500 x 300. One slot per field: the next save of that field replaces it, wx_ensemble_prior_drop
 * or wx_ensemble_destroy frees it. The snapshot remembers its field, rectangle and selection. A later wx_ensemble_step does not
 * invalidate it: the prior is whatever the host saved. One launch (kernel name "ensemble_prior_save", one lane per member-cell: 16 B
 * read, 16 B written). Refusals, ordering, blocking and report consumption as for wx_ensemble_statistics (WX_E_INVALID: e NULL, a field
 * other than WX_FIELD_BASE_CUR / WX_FIELD_WATER_CUR, nobody selected; WX_E_RANGE: the rectangle; WX_E_STATE: a selected member never
 * uploaded; WX_E_NOMEM: the buffer -- the old snapshot of that field is gone then); it changes nothing a host can observe.
 *
 * THE PER-CELL FUNCTION (the kernel, wx_ens_inflate_cells and the tests all evaluate this definition). All arithmetic is double, every
 * operation rounded separately (no fused multiply-add: contraction is off inside every function that rounds, and every product that
 * feeds a sum is a value of its own in every build, so libwxsim.so, libwxsim_fast.so, the device and the host give the same bits);
 * sqrt is the correctly rounded double square root. "In member order": the n selected members k = 0 .. n-1 by ascending member index.
 * x_k is member k's value of channel c of the cell, p_k its snapshot value.
 *   Neutral. A channel whose coef[c] is neutral -- CONST: 1, RTPS / RTPP: 0 -- is untouched.
 *   Eligibility. Otherwise the channel is updated only if in every selected member the cell is an air cell (channel 1 of its
 *   WX_FIELD_WALL_CUR texel != 0: wx_diag's test) and x_k is finite, and in RTPS / RTPP every p_k is finite too; else it is untouched in
 *   all members.
 *   Mean. S = sum (double)x_k in member order, m = S / n, d_k = (double)x_k - m.
 *   CONST. lambda = (double)coef[c].
 *   RTPS. Qa = sum d_k*d_k in member order; Sb = sum (double)p_k, mb = Sb / n, b_k = (double)p_k - mb, Qb = sum b_k*b_k, both in member
 *   order; sa = sqrt(Qa / (n - 1)), sb = sqrt(Qb / (n - 1)). If sa == 0 the channel is untouched. Otherwise
 *   lambda = 1 + (double)coef[c] * ((sb - sa) / sa) -- a difference, a quotient, a rounded product, a sum --, then the bounds: if
 *   lambda_lo is not NaN and lambda < lambda_lo, lambda = lambda_lo; then if lambda_hi is not NaN and lambda > lambda_hi, lambda = lambda_hi.
 *   CONST and RTPS, common tail. If lambda is not finite or lambda == 1 the channel is untouched (so a -0.0 never becomes +0.0 by a
 *   factor of one). Otherwise for every member o_k = (float)(m + lambda*d_k).
 *   RTPP. a = (double)coef[c], g = 1 - a, and for every member o_k = (float)(m + (g*d_k + a*b_k)) with b_k as above: two rounded
 *   products and two rounded sums. (a == 1: o_k - m is b_k, the prior's perturbation about the analysis mean.)
 *   Clamp. Then wx_ens_perturb's clamp (lo first, then hi, NaN = none). If o_k is not finite that member's channel keeps its bits.
 *   lambda_out (CONST and RTPS) holds (float)lambda where the channel was updated -- where the common tail was reached and passed --
 *   and NaN elsewhere.
 * Cells never interact, and neither do channels: any split of a rectangle gives the same bits.
 *
 * wx_ensemble_inflate. Answered before the device is touched -- WX_E_INVALID: e or p NULL; a field other than WX_FIELD_BASE_CUR /
 * WX_FIELD_WATER_CUR; an unknown mode; a coef that is not finite or is negative; an RTPP coef > 1; lambda_out given with RTPP; fewer than
 * two selected members. WX_E_RANGE: the rectangle does not lie inside the grid (no wrap). WX_E_STATE: a selected member was never
 * uploaded; in RTPS / RTPP, no snapshot of that field, a selection that differs from the snapshot's, a rectangle not inside the
 * snapshot's (the message says which). CONST never looks at a snapshot. Bookkeeping, ordering, blocking and report consumption exactly
 * as for wx_ensemble_perturb: a lazy WX_FIELD_BASE_DISP is assembled whole first, a pending WX_FIELD_WATER_0 is made first, velocities
 * written are looked at by the next |vx| scan, written water ends the water-free state. The snapshot is read, never written.
 * wx_profile on member 0 times the launch (kernel name "ensemble_inflate"); traffic per member-cell: DESIGN.md section 4.
 * wx_ens_inflate_cells (host only, pure): the same function over n_cells cells the caller holds -- member i's cells at field[i]
 * (4 floats per cell, changed in place), wall[i] (4 bytes per cell) and prior[i] (4 floats per cell; the table or its entries may be
 * NULL in CONST). The rectangle of the descriptor is not looked at; lambda_out, if given, holds n_cells * 4 floats. WX_E_INVALID as
 * above, and for n_members < 1, a NULL table, a NULL entry of a selected member. */
#define WX_HAVE_ENSEMBLE_INFLATE 1
#define WX_INFLATE_CONST 0
#define WX_INFLATE_RTPS  1
#define WX_INFLATE_RTPP  2
typedef struct wx_ens_inflate {
  int32_t field;            /* WX_FIELD_BASE_CUR or WX_FIELD_WATER_CUR */
  int32_t x, y, w, h;       /* cells that may change; no wrap (WX_E_RANGE) */
  int32_t mode;             /* WX_INFLATE_* */
  float   coef[4];          /* per channel. CONST: lambda (neutral 1). RTPS / RTPP: alpha (neutral 0). Neutral: bits untouched */
  float   lambda_lo, lambda_hi; /* RTPS only: bounds of the derived lambda, NaN: none */
  float   lo[4], hi[4];     /* clamp of the result as wx_ens_perturb, NaN: none */
  float  *lambda_out;       /* optional w*h*4 map (CONST, RTPS): the lambda applied, NaN where the channel was left alone */
} wx_ens_inflate;
int wx_ensemble_prior_save(wx_ensemble *e, int field, int x, int y, int w, int h, const uint8_t *member_mask);
int wx_ensemble_prior_drop(wx_ensemble *e, int field);   /* frees that field's snapshot; WX_OK if there is none */
int wx_ensemble_inflate(wx_ensemble *e, const wx_ens_inflate *p, const uint8_t *member_mask);
int wx_ens_inflate_cells(const wx_ens_inflate *p, int n_members, size_t n_cells, float *const *field,
                         const int8_t *const *wall, const float *const *prior /* NULL entries allowed in CONST */,
                         const uint8_t *member_mask);   /* host only, pure; lambda_out over n_cells */

/* ---- (ABI 11, WX_HAVE_ENSEMBLE_COVARIANCE) Covariance, correlation and sensitivity maps on the device: the quantity the filter runs
 * on, made visible. wx_ensemble_assimilate forms the sample covariance, over the members, between a state cell and a scalar, weights
 * it and throws it away. This call returns it, for every cell and channel of a rectangle, against up to WX_ENS_COV_MAX scalar
 * PREDICTORS at once -- the members are read once for all of them --, together with the correlation (where does it sink into the
 * sampling noise of about 1/sqrt(n-1)? that is how loc_x / loc_y are chosen) and the regression slope dJ/dx = cov(J, x) / var(x), the
 * ensemble sensitivity of Torn and Hakim (2008). The state x is the members' field as it is now (WX_COV_SOURCE_CURRENT) or the snapshot
 * wx_ensemble_prior_save took of it (WX_COV_SOURCE_PRIOR): "which part of the analysis decides the rain 500 iterations later" regresses
 * a forecast metric J_k (e.g. from wx_ensemble_diagnostics) onto the saved prior, which lives only on the device.
 *
 * THE DEFINITION (the kernels, wx_ens_cov_cells and the tests all evaluate it). All arithmetic is double, every operation rounded
 * separately (no fused multiply-add: contraction is off inside every function that rounds, and every product that feeds a sum is a
 * value of its own in every build, so libwxsim.so, libwxsim_fast.so, the device and the host give the same bits); sqrt is the correctly
 * rounded double square root. "In member order": the n selected members k = 0 .. n-1 by ascending member index. All sums start at +0.0.
 *   Predictor j. WX_COV_PRED_POINT: t_k = (double) of channel `channel` of cell (x, y) of member k's CURRENT `field` (whatever the
 *   source of the state); valid only if in every selected member that cell is an air cell (channel 1 of its WX_FIELD_WALL_CUR texel
 *   != 0) and the value is finite. WX_COV_PRED_VALUES: t_k = values[member index] (n_members entries, by member index; the entries of
 *   unselected members are not looked at); always valid, because entries that are not finite or exceed the float range are refused.
 *   Valid: Sj = sum t_k in member order, jm = Sj / n, e_k = t_k - jm, Qj = sum e_k*e_k in member order; result[j] = {1, jm, Qj / (n-1)}.
 *   For a point these are the bits wx_ens_obs_result.prior_mean / prior_var have for the same cell and channel. Invalid:
 *   result[j] = {0, NaN, NaN} and every plane of that predictor is NaN everywhere.
 *   Cell-channel. x_k is member k's value of channel c of the cell: of `field` (CURRENT) or of its snapshot (PRIOR). It is ELIGIBLE iff
 *   in every selected member the cell is an air cell -- by the CURRENT wall texture in both sources: the snapshot holds no walls -- and
 *   x_k is finite. Eligible: Sx = sum (double)x_k, xm = Sx / n, d_k = (double)x_k - xm, Qx = sum d_k*d_k, and for every valid predictor
 *   Cq_j = sum d_k*e_jk, all in member order. Then
 *     variance = (float)(Qx / (n-1))                the members' own sample variance
 *     cov_j    = (float)(Cq_j / (n-1))
 *     slope_j  = Qx == 0 ? NaN : (float)(Cq_j / Qx)    dJ/dx, the sensitivity
 *     corr_j   = den == 0 ? NaN : (float)clamp(Cq_j / den, -1, 1)  with den = sqrt(Qx * Qj) (a rounded product, then the root)
 *   Not eligible: NaN in all four. A double beyond the float range converts to +-Inf, as the C conversion does.
 *   No product or sum here can overflow a double: |x_k|, |t_k| <= FLT_MAX (that is why VALUES are held to the float range), so
 *   |d*e| <= 4 FLT_MAX^2, a Q or Cq is at most 65535 times that, and Qx * Qj < 1e166.
 * Consequences. A point predictor's own cell-channel (same field, CURRENT) has Cq == Qx == Qj bit for bit: corr and slope are exactly
 * 1.0f and cov has the bits of variance (unless Q is 0: NaN, NaN, 0). Cells never interact, and neither do channels: any split of the
 * rectangle gives the same bits. Plane j depends on no other predictor.
 *
 * wx_ensemble_covariance. Answered before the device is touched -- WX_E_INVALID: e, c or pred NULL; a field other than
 * WX_FIELD_BASE_CUR / WX_FIELD_WATER_CUR, for the state or for a point; an unknown kind or source; n_pred outside 1 .. WX_ENS_COV_MAX; a
 * point channel outside 0 .. 3; VALUES with a NULL pointer, or with a selected member's entry that is not finite or has |v| > FLT_MAX;
 * fewer than two selected members. WX_E_RANGE: the rectangle or a point lies outside the grid (no wrap). WX_E_STATE: a selected member
 * was never uploaded (the message names it); with WX_COV_SOURCE_PRIOR, no snapshot of that field, a selection that differs from the
 * snapshot's, a rectangle not inside the snapshot's (wx_ensemble_inflate's three checks; the message says which). `result` holds n_pred
 * entries or is NULL. Everything else as for wx_ensemble_statistics: member_mask has one byte per member (NULL = all), the members'
 * pointers are taken at the time of the call, the work is ordered behind everything pending on the ensemble's stream, the call BLOCKS
 * like wx_ensemble_sync and consumes and returns a member's pending report ("member i: ..."), its device buffers belong to the ensemble
 * and go with wx_ensemble_destroy. It CHANGES NOTHING a host can observe: no member is written, no lazy field is assembled, the
 * snapshot is read only. Two launches: the predictors' chains (kernel name "ensemble_covariance_pred", one workgroup), then the maps
 * (kernel name "ensemble_covariance"); wx_profile on member 0 times them; traffic per member-cell: DESIGN.md section 4.
 * wx_ens_cov_cells (host only, pure): the same definition over whole X x Y grids the caller holds -- member i's at base[i] / water[i]
 * (4 floats per cell) and wall[i] (4 bytes per cell); a table no predictor and no CURRENT state needs may be NULL -- and, with
 * WX_COV_SOURCE_PRIOR, prior[i]: the w*h cells of the rectangle (4 floats per cell). Planes as above. WX_E_INVALID / WX_E_RANGE as above,
 * and WX_E_INVALID for n_members < 1, a NULL table that is needed, a NULL entry of a selected member. */
#define WX_HAVE_ENSEMBLE_COVARIANCE 1
#define WX_ENS_COV_MAX 8
#define WX_COV_PRED_POINT  0   /* the members' own value of one channel of one cell of their CURRENT state */
#define WX_COV_PRED_VALUES 1   /* one double per member from the host: a forecast metric */
#define WX_COV_SOURCE_CURRENT 0  /* x_k: the members' field as it is now */
#define WX_COV_SOURCE_PRIOR   1  /* x_k: the snapshot wx_ensemble_prior_save took of that field */
typedef struct wx_ens_cov_pred {
  int32_t kind;             /* WX_COV_PRED_* */
  int32_t field, x, y, channel;  /* POINT: WX_FIELD_BASE_CUR or WX_FIELD_WATER_CUR, the cell, 0 .. 3; VALUES: not looked at */
  int32_t pad;
  const double *values;     /* VALUES: n_members entries, by member index; POINT: not looked at */
} wx_ens_cov_pred;
typedef struct wx_ens_cov_result {
  int32_t valid, pad;
  double  mean, variance;   /* jm and Qj / (n-1); NaN if not valid */
} wx_ens_cov_result;
typedef struct wx_ens_cov {
  int32_t field;            /* WX_FIELD_BASE_CUR or WX_FIELD_WATER_CUR */
  int32_t source;           /* WX_COV_SOURCE_* */
  int32_t x, y, w, h;       /* the rectangle; no wrap (WX_E_RANGE) */
  int32_t n_pred, pad;      /* 1 .. WX_ENS_COV_MAX */
  float  *cov, *corr, *slope;  /* n_pred planes of w*h*4 each, plane j = predictor j; NULL: not wanted */
  float  *variance;         /* w*h*4: the members' own sample variance; NULL: not wanted */
} wx_ens_cov;
int wx_ensemble_covariance(wx_ensemble *e, const wx_ens_cov *c, const wx_ens_cov_pred *pred,
                           wx_ens_cov_result *result /* n_pred entries or NULL */, const uint8_t *member_mask);
int wx_ens_cov_cells(const wx_ens_cov *c, const wx_ens_cov_pred *pred, wx_ens_cov_result *result, int X, int Y, int n_members,
                     const float *const *base, const float *const *water, const int8_t *const *wall,
                     const float *const *prior /* w*h cells of the rectangle per member; WX_COV_SOURCE_PRIOR only */,
                     const uint8_t *member_mask);   /* host only, pure */

/* ---- (ABI 11, WX_HAVE_ENSEMBLE_NEIGHBOURHOOD) Neighbourhood ensemble probabilities and the fractions skill score (FSS, Roberts and
 * Lean 2008) on the device: verification at a SCALE. Cloud and precipitation are intermittent; a convective cell forecast a few
 * columns off is penalised twice by every point-wise score of wx_ensemble_scores, although the forecast was good at the scale anyone
 * would use it. This call counts, per cell, in how many selected members an event (one channel above or below a threshold) holds,
 * sums the counts over boxes of up to WX_ENS_NBHD_MAX_SCALES sizes at once, compares the forecast fraction with the truth's and
 * returns the three domain sums the FSS is made of, per scale, with the two fraction maps if they are wanted. The members are read
 * once per grid cell, whatever the number of scales; there is no cap on the number of members beyond the ensemble's own.
 *
 * THE DEFINITION (the kernels, wx_ens_nbhd_cells and the tests all evaluate it). Everything up to one division per cell is integer
 * arithmetic, so the result does not depend on the order of the members, the launch shape or the build.
 *   Event. For a value v of channel `channel` of `field`: above != 0: v > threshold (the float compare of wx_ens_stat's n_above);
 *   above == 0: v < threshold. A NaN threshold gives no event anywhere; -0.0 == 0.0.
 *   Point counts, for every cell of the GRID. Nf = the number of selected members in which the cell is an air cell (channel 1 of its
 *   WX_FIELD_WALL_CUR texel != 0: wx_diag's test) and the channel's value is finite; Ef = the number of those in which the event
 *   holds. No and Eo: the same for `truth`, each 0 or 1 (both 0 everywhere if truth is NULL).
 *   Window of scale s = (rx, ry) around output cell (cx, cy): columns cx-rx .. cx+rx, rows cy-ry .. cy+ry. Rows outside 0 .. Y-1
 *   contribute nothing. Columns outside 0 .. X-1 contribute nothing without wrap_x; with wrap_x they are taken modulo X, and then
 *   2*rx+1 > X is WX_E_RANGE, so that no cell is counted twice. Windows reach outside the rectangle into the grid: a cell's result
 *   does not depend on the rectangle. Af, Bf, Ao, Bo are the window sums of Ef, Nf, Eo, No: integers, at most
 *   (2*32+1)^2 * 65535 = 276 885 375 (a window of 4225 cells, an ensemble of at most 65535 members), which fits int32.
 *   Per cell and scale. The cell is SCORED when Bf > 0 and Bo > 0; otherwise it counts into n_unscored[s]. In double, each operation
 *   rounded once: pf = (double)Af / (double)Bf, po = (double)Ao / (double)Bo, d = pf - po; three floats d2 = (float)(d*d),
 *   f2 = (float)(pf*pf), o2 = (float)(po*po). They lie in [0, 1]: always finite. (No product feeds a sum: nothing a build could fuse.)
 *   Domain sums per scale, over the scored cells of the rectangle: n_scored[s]; sum_d2[s], sum_f2[s], sum_o2[s], the EXACT sums of
 *   those floats rounded to double once -- what Python's math.fsum returns --, taken with wx_diag's integer bins and its 320-bit
 *   finish as wx_ens_score's sums are. FSS(s) = 1 - sum_d2 / (sum_f2 + sum_o2) is the host's one line.
 *   Point-level totals over the rectangle, independent of scale: ev_f, n_f, ev_o, n_o = the sums of Ef, Nf, Eo, No (int64).
 *   Optional maps, laid out [s][h][w] in float32, rows bottom-up: nep = (float)pf, NaN where Bf == 0 (the neighbourhood ensemble
 *   probability); obs_fraction = (float)po, NaN where Bo == 0.
 *   truth may be NULL: the forecast product alone -- nep, ev_f, n_f. Every truth-side number is 0, n_scored is 0 (every cell counts
 *   into n_unscored), and obs_fraction must not be requested.
 *
 * wx_ensemble_neighbourhood. Answered before the device is touched -- WX_E_INVALID: e, args or out NULL; a field other than
 * WX_FIELD_BASE_CUR / WX_FIELD_WATER_CUR; a channel outside 0 .. 3; n_scales outside 1 .. WX_ENS_NBHD_MAX_SCALES; a radius outside
 * 0 .. WX_ENS_NBHD_MAX_RADIUS; a threshold that is +-Inf (NaN is taken); obs_fraction wanted without a truth; nobody selected;
 * `truth` is a selected member of e; `truth` is a slab handle, a handle of another X or Y, or a handle on another device.
 * WX_E_RANGE: the rectangle does not lie inside the grid (no wrap of the rectangle itself), or wrap_x with a window wider than X.
 * WX_E_STATE: a selected member, or `truth`, was never uploaded (the message names it). `truth` is any whole-domain handle: a lone
 * one, an unselected member of e, a member of another ensemble. Ordering behind both streams, blocking, consumption of pending
 * reports ("truth: ...", "member i: ...") and "changes nothing" exactly as for wx_ensemble_scores; member_mask has one byte per
 * member (NULL = all); any number of selected members from 1 up. Two launches: the point counts (kernel name
 * "ensemble_nbhd_points", the member walk of wx_ensemble_statistics, 5 bytes per cell written to the ensemble's device staging),
 * then the windows (kernel name "ensemble_nbhd_windows"); wx_profile on member 0 times them; DESIGN.md section 4.
 * wx_ens_nbhd_cells (host only, pure): the same definition over whole X x Y grids the caller holds, because windows leave the
 * rectangle -- member i's at field[i] (4 floats per cell) and wall[i] (4 bytes per cell), the truth's at truth_field / truth_wall
 * (both NULL: no truth). WX_E_INVALID / WX_E_RANGE as above, and WX_E_INVALID for n_members < 1, X or Y < 1, a NULL table, a NULL
 * entry of a selected member, one truth array without the other. A refused call writes nothing. */
#define WX_HAVE_ENSEMBLE_NEIGHBOURHOOD 1
#define WX_ENS_NBHD_MAX_RADIUS 32
#define WX_ENS_NBHD_MAX_SCALES 8
typedef struct wx_ens_nbhd {
  int32_t field;            /* WX_FIELD_BASE_CUR or WX_FIELD_WATER_CUR */
  int32_t channel;          /* 0 .. 3 */
  float   threshold;        /* finite or NaN (no event anywhere) */
  int32_t above;            /* non-zero: the event is v > threshold; 0: v < threshold */
  int32_t wrap_x;           /* window columns are taken modulo X */
  int32_t x, y, w, h;       /* the output cells; the rectangle itself does not wrap (WX_E_RANGE) */
  int32_t n_scales;         /* 1 .. WX_ENS_NBHD_MAX_SCALES */
  int32_t rx[WX_ENS_NBHD_MAX_SCALES], ry[WX_ENS_NBHD_MAX_SCALES];  /* half-widths of scale s in cells, 0 .. WX_ENS_NBHD_MAX_RADIUS */
  float  *nep, *obs_fraction;  /* optional n_scales*h*w maps, NaN where the window holds no counted cell; NULL: not wanted */
} wx_ens_nbhd;
typedef struct wx_ens_nbhd_result {
  int64_t n_scored[WX_ENS_NBHD_MAX_SCALES], n_unscored[WX_ENS_NBHD_MAX_SCALES];
  double  sum_d2[WX_ENS_NBHD_MAX_SCALES], sum_f2[WX_ENS_NBHD_MAX_SCALES], sum_o2[WX_ENS_NBHD_MAX_SCALES];  /* entries >= n_scales: 0 */
  int64_t ev_f, n_f, ev_o, n_o;
} wx_ens_nbhd_result;
int wx_ensemble_neighbourhood(wx_ensemble *e, wx_sim *truth /* or NULL */, const wx_ens_nbhd *args,
                              const uint8_t *member_mask /* n_members bytes, NULL = all */, wx_ens_nbhd_result *out);
int wx_ens_nbhd_cells(const wx_ens_nbhd *args, wx_ens_nbhd_result *out, int X, int Y, int n_members,
                      const float *const *field, const int8_t *const *wall, const float *truth_field, const int8_t *truth_wall,
                      const uint8_t *member_mask);   /* host only, pure */
int wx_ens_nbhd_max_radius(void);  /* == WX_ENS_NBHD_MAX_RADIUS */

/* ---- (ABI 11, WX_HAVE_ENSEMBLE_GRAM) The members' Gram matrix on the device: the ensemble seen in MEMBER SPACE. Every call above looks
 * at a cell across the members; this one looks at the members across the cells: the n x n matrix of inner products of the members'
 * deviations over a rectangle, per channel. How far member i is from member j (G_ii + G_jj - 2 G_ij), which member is the most
 * representative (the medoid), whether the members fall into two scenarios, how many independent directions the spread has left after
 * ten analysis cycles (the rank of G), and the EOFs -- G / (n-1) has the non-zero eigenvalues of the spatial covariance, its
 * eigenvectors are the principal-component scores, and wx_ensemble_covariance with those scores as WX_COV_PRED_VALUES turns them into
 * the spatial patterns -- are a few lines of host arithmetic on a matrix of at most 64 x 64.
 *
 * THE DEFINITION (the kernels, wx_ens_gram_cells and the tests all evaluate it). The arithmetic of a cell is double, every operation
 * rounded separately, a product is a value of its own in every build (as for wx_ensemble_covariance, whose first walk this reuses).
 * "In member order": the n selected members k = 0 .. n-1 by ascending member index.
 *   Eligibility. x_k is member k's value of channel c of the cell. The cell-channel is ELIGIBLE iff in every selected member the cell is
 *   an air cell (channel 1 of its WX_FIELD_WALL_CUR texel != 0) and x_k is finite; otherwise it is EXCLUDED.
 *   Centre. WX_GRAM_CENTER_MEAN: Sx = sum (double)x_k in member order from +0.0, xm = Sx / n. WX_GRAM_CENTER_NONE: xm = +0.0 (the raw
 *   inner products). In both modes d_k = (double)x_k - xm.
 *   Term. For a <= b: p_ab = (float)(d_a * d_b): one double product, then the C conversion (round to nearest; a product beyond the
 *   float range converts to +-Inf, a tiny one to a subnormal float or to a zero).
 *   Overflow. The cell-channel is OVERFLOW iff some diagonal term p_kk is not finite; then NONE of its terms enters. The conversion is
 *   monotone and |d_a d_b| <= max(d_a^2, d_b^2), so |p_ab| <= max(p_aa, p_bb): an off-diagonal term of a cell-channel that is not
 *   OVERFLOW is always finite, and the diagonal test is the whole test.
 *   Sum. gram[c][a][b] = gram[c][b][a] = the correctly rounded double of the EXACT sum of p_ab over the cell-channels of the rectangle
 *   that entered (eligible, not overflow) -- what Python's math.fsum returns --, taken with wx_diag's integer bins and its 320-bit
 *   finish as wx_ens_score's sums are. So the matrix does not depend on the order of the cells, the launch shape or the build; it is
 *   exactly symmetric and its diagonal is >= 0; with NONE it does not depend on the order of the members either (permuting the members
 *   permutes the matrix bit for bit); with MEAN it inherits the member-order mean, as the covariance does. A sum over nothing is +0.0.
 *   Counts per channel: n_entered + n_excluded + n_overflow = w*h.
 *
 * wx_ensemble_gram. Answered before the device is touched -- WX_E_INVALID: e or g NULL; a field other than WX_FIELD_BASE_CUR /
 * WX_FIELD_WATER_CUR; an unknown center; gram NULL; fewer than two selected members with MEAN, fewer than one with NONE; more than
 * WX_ENS_GRAM_MAX_MEMBERS selected. WX_E_RANGE: the rectangle lies outside the grid (no wrap). WX_E_STATE: a selected member was never
 * uploaded (the message names it). Everything else as for wx_ensemble_covariance: member_mask has one byte per member (NULL = all), the
 * work is ordered behind everything pending on the ensemble's stream, the call BLOCKS like wx_ensemble_sync and consumes and returns a
 * member's pending report, its device buffers belong to the ensemble, and it CHANGES NOTHING a host can observe. n_selected is filled
 * in. Two launches: the centres and the entry test of every cell-channel (kernel name "ensemble_gram_centre"), then the pairs (kernel
 * name "ensemble_gram"); what leaves the device is integers; wx_profile on member 0 times both; DESIGN.md section 4.
 * wx_ens_gram_cells (host only, pure): the same definition over whole X x Y grids the caller holds -- member i's `field` at field[i]
 * (4 floats per cell) and wall[i] (4 bytes per cell). WX_E_INVALID / WX_E_RANGE as above, and WX_E_INVALID for n_members < 1, X or
 * Y < 1, a NULL table, a NULL entry of a selected member. A refused call writes nothing.
 * Out of scope: the snapshot of wx_ensemble_prior_save as a source; more than 64 members; the raw bins as an output, for merging
 * rectangles (add the matrices of disjoint rectangles instead: one more rounding per entry). */
#define WX_HAVE_ENSEMBLE_GRAM 1
#define WX_ENS_GRAM_MAX_MEMBERS 64
#define WX_GRAM_CENTER_MEAN 0   /* deviations from the members' mean of the cell-channel */
#define WX_GRAM_CENTER_NONE 1   /* the raw values */
typedef struct wx_ens_gram {
  int32_t field;            /* WX_FIELD_BASE_CUR or WX_FIELD_WATER_CUR */
  int32_t center;           /* WX_GRAM_CENTER_* */
  int32_t x, y, w, h;       /* the rectangle; no wrap (WX_E_RANGE) */
  double *gram;             /* 4 * n * n doubles: gram[(c*n + a)*n + b]; a, b: position among the selected members, ascending member index */
  int64_t n_entered[4], n_excluded[4], n_overflow[4];   /* per channel; they add up to w*h */
  int32_t n_selected, pad;
} wx_ens_gram;
int wx_ensemble_gram(wx_ensemble *e, wx_ens_gram *g, const uint8_t *member_mask /* n_members bytes, NULL = all */);
int wx_ens_gram_cells(wx_ens_gram *g, int X, int Y, int n_members, const float *const *field,
                      const int8_t *const *wall, const uint8_t *member_mask);   /* host only, pure */
int wx_ens_gram_max_members(void);  /* == WX_ENS_GRAM_MAX_MEMBERS */

/* Per-kernel device time from HIP events recorded on the handle's stream around every launch.
 * wx_profile(s, 1) starts collecting, wx_profile_read returns accumulated milliseconds and launch counts
 * for up to `cap` kernels (names via wx_kernel_name) and resets the accumulators. */
int wx_profile(wx_sim *s, int enable);
int wx_profile_read(wx_sim *s, int cap, float *ms, int *launches);
int wx_kernel_count(void);
const char *wx_kernel_name(int k);

#ifdef __cplusplus
}
#endif
#endif /* WXSIM_H */
