/*
 * sphx.h -- C ABI of libsphx.so, the MI355X (gfx950) HIP implementation of the per-step SPH hot
 * path of KIYOYOZU/SPH-Poiseuille-Flow.
 *
 * Boundary being replaced: the two MEX gateways
 *     sph_neighbor_search_mex   (reference mex/sph_neighbor_search_mex.c:185, 5 in / 7 out)
 *     sph_physics_shell_mex     (reference mex/sph_physics_mex.c:1745, mode string + per-mode arity)
 * called from SPH_Poiseuille.m:167,169,366,380,388,398,406,419,428.
 *
 * Conventions (identical to the MEX surface):
 *   - every array is IEEE double, column-major: [n x 2] = x column then y column, B[n x 4] =
 *     B11|B12|B21|B22 columns (sph_physics_mex.c:362-365);
 *   - pair_i / pair_j hold 1-based particle indices stored as doubles
 *     (sph_neighbor_search_mex.c:375-376); fluid-fluid pairs appear once with i < j, fluid-wall
 *     pairs once with the fluid particle as i; wall particles are rows n_fluid..n_total-1;
 *   - inputs are borrowed and never written; outputs are caller-allocated with the sizes the MEX
 *     gateway would mxCreateDoubleMatrix.
 * All pointers are HOST pointers unless a name ends in _dev.  Functions return SPHX_OK (0) or a
 * negative status; sphx_last_error()/sphx_last_error_id() give the message and the MEX-style id
 * ("SPH:Neighbor:count", "SPH:Physics:int1:B" ...) a gateway passes to mexErrMsgIdAndTxt.
 * Thread model: like MATLAB, one caller thread per context; the library is not re-entrant on one
 * context.  There is no CPU fallback: without a HIP device every compute entry point fails with
 * SPHX_ERR_DEVICE.
 */
#ifndef SPHX_H
#define SPHX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPHX_OK 0
#define SPHX_ERR_ARG (-1)      /* invalid argument (message carries the MEX id)                      */
#define SPHX_ERR_DEVICE (-2)   /* no HIP device / HIP runtime error                                  */
#define SPHX_ERR_STATE (-3)    /* call sequence error (e.g. fetch without search)                    */
#define SPHX_ERR_DIVERGED (-4) /* dt collapsed below 1e-14 (SPH_Poiseuille.m:260-263)                */
#define SPHX_ERR_GRID (-5)     /* particle left the cell grid / cell displacement bound violated      */

const char *sphx_version(void);
const char *sphx_last_error(void);
const char *sphx_last_error_id(void);
int sphx_device_count(void);
int sphx_set_device(int device);

/* Diagnostics of the caching pool all device memory comes from.  The pool hands a freed block to the next request of its size
 * class as it was returned; results must not depend on what it held.
 * sphx_pool_stats: out = { cached_bytes, cached_blocks, hits, misses }; a hit is an allocation served from the cache, a miss
 * one that went to hipMalloc, both counted since process start.  No HIP call: all zeros on a machine without a device.
 * sphx_pool_scrub: fill every cached free block of the current device with the 32-bit `word`, under the pool's lock, and wait
 * for the device; *n_blocks (may be NULL) = the blocks filled.  Free blocks are in nobody's use, so nothing else changes.
 * With nothing cached: 0 blocks and no HIP call.  Must not be called while a stream is capturing.
 * sphx_pool_poison_on_free: test support, off by default.  on != 0: from now on a block that goes back into the cache is first
 * filled with the 32-bit `word`, on a non-blocking stream the pool owns; that stream alone is waited for, under the pool's lock,
 * before the block can be handed out again, so a late fill never overwrites a later owner.  Work the former owner left in
 * flight on its own streams is NOT waited for: it races with the fill, and a block released too early shows as wrong numbers
 * in its former owner's results -- or in its next owner's: a filled block is handed out before older blocks of its size class.
 * Blocks that go straight to hipFree are not filled, nor are blocks freed on a thread that is
 * inside one of the library's own stream captures.  on == 0: the free path is as before and makes no HIP call.  Toggling makes
 * no HIP call.  Must not be called while a stream is capturing; the mode costs a stream wait per free and is not for timed runs.
 * sphx_pool_poison_stats: out = { blocks filled, fills skipped inside a capture }, both counted since process start.  No HIP
 * call: zeros on a machine without a device. */
int sphx_pool_stats(uint64_t out[4]);
int sphx_pool_scrub(uint32_t word, uint64_t *n_blocks);
int sphx_pool_poison_on_free(int on, uint32_t word);
int sphx_pool_poison_stats(uint64_t out[2]);

/* ------------------------------------------------------------------------------------------------
 * 1. Stateless MEX-surface entry points (one per gateway call).  Host arrays in, host arrays out;
 *    the work runs in HIP kernels on the current device.
 * ---------------------------------------------------------------------------------------------- */

/* [pair_i,pair_j,dx,dy,r,W,dW] = sph_neighbor_search_mex(pos,n_fluid,n_total,h,DL)
 * (sph_neighbor_search_mex.c:12-28,185-421).  n_pairs is an output, so the call is two-phase: search
 * keeps the pair list in library-owned device memory and reports its length; fetch copies it into
 * caller arrays of at least that length and releases it.  Pairs come out ordered by i, then j. */
int sphx_neighbor_search(const double *pos, int n_fluid, int n_total, double h, double DL,
                         size_t *n_pairs);
int sphx_neighbor_fetch(double *pair_i, double *pair_j, double *dx, double *dy, double *r,
                        double *W, double *dW, size_t capacity);

/* 'density_correction' (sph_physics_mex.c:95-374): rho[n_total], Vol[n_total], B[n_total x 4]. */
int sphx_density_correction(size_t n_pairs, const double *pair_i, const double *pair_j,
                            const double *dx, const double *dy, const double *r, const double *W,
                            const double *dW, const double *mass, int n_fluid, int n_total,
                            double rho0, double h, double inv_sigma0, double *rho, double *Vol,
                            double *B);

/* 'viscous_force' (sph_physics_mex.c:396-550): force[n_total x 2]. */
int sphx_viscous_force(size_t n_pairs, const double *pair_i, const double *pair_j,
                       const double *dx, const double *dy, const double *r, const double *dW,
                       const double *vel, const double *Vol, const double *B, double mu, double h,
                       int n_fluid, int n_total, const double *mass, const double *wall_vel,
                       double *force);

/* 'transport_correction' (sph_physics_mex.c:569-714): pos_out[n_total x 2].  The 13-argument MEX
 * form uses transport_coeff = 0.2 (:584); the gateway passes that default explicitly. */
int sphx_transport_correction(size_t n_pairs, const double *pair_i, const double *pair_j,
                              const double *dx, const double *dy, const double *r,
                              const double *dW, const double *Vol, const double *B,
                              const double *pos, double h, int n_fluid, int n_total,
                              double transport_coeff, double *pos_out);

/* 'integration_1st' (sph_physics_mex.c:736-967): rho, p, pos, force, drho(diss). */
int sphx_integration_1st(size_t n_pairs, const double *pair_i, const double *pair_j,
                         const double *dx, const double *dy, const double *r, const double *dW,
                         const double *Vol, const double *B, const double *rho, const double *mass,
                         const double *pos, const double *vel, const double *drho_dt,
                         const double *force_prior, double dt, int n_fluid, int n_total,
                         double rho0, double p0, double c_f, const double *wall_vel,
                         double *rho_out, double *p_out, double *pos_out, double *force_out,
                         double *drho_out);

/* 'integration_2nd' (sph_physics_mex.c:987-1119): pos, drho_dt, zeros[n_total x 2] (may be NULL). */
int sphx_integration_2nd(size_t n_pairs, const double *pair_i, const double *pair_j,
                         const double *dx, const double *dy, const double *r, const double *dW,
                         const double *Vol, const double *rho, const double *pos,
                         const double *vel, double dt, int n_fluid, int n_total,
                         const double *wall_vel, double *pos_out, double *drho_out,
                         double *zeros_out);

/* 'integration_verlet' (sph_physics_mex.c:1316-1469): rho, p, pos, vel, drho_dt, force. */
int sphx_integration_verlet(size_t n_pairs, const double *pair_i, const double *pair_j,
                            const double *dx, const double *dy, const double *r, const double *dW,
                            const double *Vol, const double *B, const double *rho,
                            const double *mass, const double *pos, const double *vel,
                            const double *drho_dt, const double *force_prior, double dt,
                            int n_fluid, int n_total, double rho0, double p0, double c_f,
                            const double *wall_vel, double *rho_out, double *p_out,
                            double *pos_out, double *vel_out, double *drho_out, double *force_out);

/* 'advance_shell_step' (sph_physics_mex.c:1490-1639): density -> viscous(+mass*g) -> transport(0.2)
 * -> verlet in one call; 9 outputs rho,p,pos,vel,drho_dt,force,force_prior,Vol,B (:1623-1631). */
int sphx_advance_shell_step(size_t n_pairs, const double *pair_i, const double *pair_j,
                            const double *dx, const double *dy, const double *r, const double *W,
                            const double *dW, const double *mass, const double *pos,
                            const double *vel, const double *wall_vel, const double *rho,
                            const double *drho_dt, double dt, int n_fluid, int n_total,
                            double rho0, double p0, double c_f, double mu, double h,
                            double inv_sigma0, double gravity_g, double *rho_out, double *p_out,
                            double *pos_out, double *vel_out, double *drho_out, double *force_out,
                            double *force_prior_out, double *Vol_out, double *B_out);

/* 'wall_shear_monitor' (sph_physics_mex.c:1653-1743): tau_bottom, tau_top. */
int sphx_wall_shear_monitor(size_t n_pairs, const double *pair_i, const double *pair_j,
                            const double *dx, const double *dy, const double *r, const double *dW,
                            const double *pos, const double *vel, const double *wall_vel,
                            const double *Vol, const double *B, int n_fluid, int n_total, double DL,
                            double DH, double mu, double h, double *tau_bottom, double *tau_top);

/* ------------------------------------------------------------------------------------------------
 * 2. Device-resident context: the whole step loop of SPH_Poiseuille.m:250-292 stays in HBM.
 *    One context = one x-slab of the channel on one GPU (slab == whole channel for one GPU).
 * ---------------------------------------------------------------------------------------------- */

typedef struct sphx_ctx sphx_ctx;

typedef struct sphx_params {
    /* physical / numerical constants, SPH_Poiseuille.m:46-80 */
    double DL, DH, dp, h;
    double rho0, mu, c_f, p0, inv_sigma0, gravity_g;
    double transport_coeff; /* 0.30 in the main loop (:77); 0.2 reproduces advance_shell_step        */
    double t_end;           /* loop bound, SPH_Poiseuille.m:247                                     */
    int32_t sort_interval;  /* kept for signature parity; the device keeps cell order (see rebuild_every) */
    int32_t lanes_per_particle; /* 0 = auto; 1,2,4,8,16,32: lanes cooperating on one neighbour ring */
    int32_t steps_per_graph;    /* 0 = auto; steps captured per hipGraph replay (even)               */
    int32_t dual_rate;          /* 0 / 1 = the reference's single-rate loop (SPH_Poiseuille.m:250-292, the parity path).
                                   2..4 = opt-in dual-rate loop for small channels (<= ~30 k fluid particles, 16 / 32
                                   lanes per particle): one step slot is an OUTER step -- density summation, KGC, viscous
                                   force, transport shift once -- of up to dual_rate acoustic sub-steps of pressure /
                                   continuity.  The count is fixed per context: as many acoustic steps as fit into the
                                   viscous / body-force step (1 on fine channels, which are viscous-limited, and on
                                   contexts that are not eligible; sphx_ctx_substeps reports it).  Not the reference's
                                   loop, but composed of its operators: tests/dual_rate_reference.py takes the reference's
                                   neighbour search, density / KGC, viscous force and transport shift once and its
                                   integration_verlet n_in times on the carried state (same pairs, Vol, B, force_prior), and
                                   tests/test_gpu_dual_rate_parity.py compares every field with it.  Against the analytic
                                   profile, 2 sub-steps reproduce the single-rate L2 and wall shear at dp = 0.05 / 0.025 /
                                   0.02; 4 is noisier at dp = 0.05. */
    int32_t rebuild_every;      /* 0 = auto; K >= 1: particles are re-binned into cells every K-th step; in
                                   between, sweeps are centred on the cell a particle was binned into and
                                   the cells carry a skin (results do not depend on K beyond summation
                                   order: the device stops and re-bins before any neighbour can be missed) */
    int32_t dynamic_rebin;      /* device-decided re-binning (no host round trips): 0 = by size (on from 2 x 10^6 fluid
                                   particles), 1 = on, 2 = off                                              */
    double skin_h;              /* cell skin in units of h for K > 1; <= 0 = sized from K.  Both left at 0: the
                                   measured pair for the size class (K = 16 up to 20 k fluid particles, 8 up to 300 k,
                                   10 with 0.42 h up to 2 x 10^6, 24 with 0.28 h where the device re-bins by itself)  */
} sphx_params;

typedef struct sphx_status {
    double t;            /* simulated time reached                                                  */
    double dt_last;      /* dt of the last completed step                                           */
    double dt_next;      /* dt the next step would use                                              */
    double vmax;         /* max |v| over fluid after the last step (SPH_Poiseuille.m:286)           */
    int64_t step;        /* steps completed since creation (state.step)                             */
    int32_t done;        /* 1 when t >= t_target - 1e-12                                            */
    int32_t device_status; /* 0 ok, else SPHX_ERR_DIVERGED / SPHX_ERR_GRID raised on device          */
} sphx_status;

/* Create a context from host state in MEX layout.  pos/vel/wall_vel [n_total x 2]; drho_dt, mass
 * [n_total].  Rows 0..n_fluid-1 fluid, the rest wall (SPH_Poiseuille.m:107).  Builds the cell grid
 * (the neighbour structure of SPH_Poiseuille.m:167) on the device. */
int sphx_ctx_create(sphx_ctx **ctx, const sphx_params *prm, int n_fluid, int n_total,
                    const double *pos, const double *vel, const double *drho_dt,
                    const double *mass, const double *wall_vel, double t0, int64_t step0);
void sphx_ctx_destroy(sphx_ctx *ctx);

/* Run steps until t >= t_target - 1e-12 (one pass of the inner while of SPH_Poiseuille.m:250; dt is
 * clipped by remain = min(t_target - t, t_end - t), :252) or until max_steps steps have been taken
 * (max_steps <= 0: unlimited).  Blocks until the device is idle.  Steps of sphx_ctx_enqueue_steps still in flight are
 * waited for first, and the steps such a batch still owes are taken (see sphx_ctx_download): max_steps counts from there. */
int sphx_ctx_advance(sphx_ctx *ctx, double t_target, int64_t max_steps, sphx_status *status);

/* Enqueue exactly n_steps steps without host synchronisation (benchmark / pipelined use), dt clipped
 * only by t_end.  sphx_ctx_sync waits and reports. */
int sphx_ctx_enqueue_steps(sphx_ctx *ctx, int64_t n_steps);
int sphx_ctx_sync(sphx_ctx *ctx, sphx_status *status);

/* Steps are replayed as hipGraphs captured per (schedule phase, batch length); a combination that has not come up
 * before is captured on first use (a few ms).  sphx_ctx_prepare_steps captures, without running anything, what
 * an sphx_ctx_enqueue_steps(n_steps) / sphx_ctx_advance(.., max_steps = n_steps) issued next would replay, so
 * that the call itself is pure replay.  sphx_ctx_graph_stats: step slots replayed from graphs / launched
 * eagerly / graphs captured since creation. */
int sphx_ctx_prepare_steps(sphx_ctx *ctx, int64_t n_steps);
int sphx_ctx_graph_stats(sphx_ctx *ctx, int64_t *slots_replayed, int64_t *slots_eager,
                         int64_t *graphs_captured);

/* Copy state back in the caller's original row order.  Any pointer may be NULL.  rho,p,force,
 * force_prior,Vol,B are those of the last completed step (what integration_verlet / density_correction
 * returned in SPH_Poiseuille.m:254-266).  Like sphx_ctx_sync, download and monitor first wait for everything
 * enqueued and take the steps a batch of sphx_ctx_enqueue_steps still owes (a batch stops early when the cell
 * grid goes stale): "last completed step" is the last step of everything asked for, and the state and the
 * step outputs handed out belong to that same step. */
int sphx_ctx_download(sphx_ctx *ctx, double *pos, double *vel, double *rho, double *p,
                      double *drho_dt, double *force, double *force_prior, double *Vol, double *B);

/* Monitors of SPH_Poiseuille.m:281-291 on the current neighbour structure: wall shear (new pairs,
 * new pos/vel, previous Vol/B), pair count of the current list. */
int sphx_ctx_monitor(sphx_ctx *ctx, double *tau_bottom, double *tau_top, double *n_pairs);

/* The neighbour list the context currently holds, in the MEX convention and the caller's original
 * row numbering (two-phase like sphx_neighbor_search / sphx_neighbor_fetch).  Like sphx_ctx_download it first waits for
 * everything enqueued and takes the steps still owed: the list is that of the state download hands out. */
int sphx_ctx_neighbor_list(sphx_ctx *ctx, size_t *n_pairs);

/* Average device time (ms) of each per-step kernel since the last call, measured with HIP events on
 * the context's stream when profiling is enabled.  names: array of const char* filled by the library. */
int sphx_ctx_profile_enable(sphx_ctx *ctx, int on);
int sphx_ctx_profile_read(sphx_ctx *ctx, int capacity, const char **names, double *avg_ms,
                          int64_t *launches, int *n_kernels);

/* Average duration (ms) of ONE neighbour-pass kernel ("k_density", "k_kgc", "k_forces", "k_continuity") in
 * the hipGraph-replay regime: `reps` back-to-back launches between two HIP events.  pos/vel/drho_dt are left
 * unchanged; the per-step outputs (rho, p, force, Vol, B) are overwritten and cannot be downloaded again until
 * the next step has been taken. */
int sphx_ctx_time_kernel(sphx_ctx *ctx, const char *name, int reps, double *avg_ms);

/* Cell-grid policy in force: re-binning interval K (constant), skin in length units, the number of unscheduled
 * re-binnings so far (the drift bound was hit: host-driven contexts then re-bin every step for a cool-down of
 * 16..1024 steps, dynamic contexts just re-bin), and the largest distance of any particle from where it was
 * binned (as of the last advance / sync; always <= skin/2). */
int sphx_ctx_grid_policy(sphx_ctx *ctx, int *rebuild_every, double *skin, int64_t *forced_rebuilds,
                         double *drift);

/* The launch shape the context chose (lanes cooperating per particle, steps per hipGraph replay). */
int sphx_ctx_tuning(sphx_ctx *ctx, int *lanes_per_particle, int *steps_per_graph);

/* Threads per workgroup of the compact step kernels (16 / 32 lanes per particle): 64, 128 or 256.  256 for every context
 * that does not run them, and for batches, slabs and dynamic contexts. */
int sphx_ctx_block_size(sphx_ctx *ctx, int *block_size);

/* The launch schedule the context runs: fuse_ea = pass E of a step and pass A of the next one share a launch
 * (three launches per step), tail_clock = the clock update rides in the last launch of a step, dynamic = the device
 * decides when to re-bin; rebins = re-binnings carried out by step slots so far (scheduled ones; dynamic contexts:
 * all of them), not counting the forced ones sphx_ctx_grid_policy reports. */
int sphx_ctx_schedule(sphx_ctx *ctx, int *fuse_ea, int *tail_clock, int *dynamic, int64_t *rebins);

/* The kernel forms the context runs: walk_kernels = the large-channel ("_w") passes with 16-bit neighbour lists (up to 8
 * lanes per particle), lds_tiles = the force pass stages its workgroup's neighbourhood in LDS, tiles_abe = passes A, B and E
 * do too, coded_lists = the lists name tile slots instead of index differences. */
int sphx_ctx_kernel_forms(sphx_ctx *ctx, int *walk_kernels, int *lds_tiles, int *tiles_abe, int *coded_lists);

/* Inner sub-steps per step slot: 1 unless sphx_params::dual_rate asked for the dual-rate loop and the context is
 * eligible.  With n_inner > 1 a "step" of sphx_status / max_steps is an outer step (t advances by n_inner * dt_last). */
int sphx_ctx_substeps(sphx_ctx *ctx, int *n_inner);

/* Global particle counts and the cell grid the context built. */
int sphx_ctx_info(sphx_ctx *ctx, int *n_fluid, int *n_wall, int *n_cell_x, int *n_cell_y);

/* ------------------------------------------------------------------------------------------------
 * 2b. Batched contexts: M independent channels of ONE geometry stepped by the same launches (parameter sweeps,
 *     ensembles of perturbed realisations).  A small channel leaves most of the GPU idle and pays a launch floor per
 *     step; a batch gives every launch M times the workgroups.
 *
 *     Shared by all members (refused with SPHX:Batch:geometry, naming the field and the member, when they differ):
 *     DL, DH, dp, h, rho0, inv_sigma0, t_end, n_fluid, n_total, the wall particles (positions, mass, wall_vel), the
 *     cell grid, lanes_per_particle, steps_per_graph, rebuild_every, skin_h.  Per member: mu, c_f, p0, gravity_g,
 *     transport_coeff and the fluid state.  Batches run the compact kernels only (16 or 32 lanes per particle: what a
 *     context of up to ~30 k fluid particles runs; larger channels are refused with SPHX:Batch:size) and refuse
 *     dual_rate > 1 and dynamic_rebin == 1 (SPHX:Batch:mode).  1 <= n_members <= 4096 (SPHX:Batch:members); device
 *     memory bounds M further on larger channels (about 10 MB per member at 5 760 particles).
 *
 *     Every member keeps its own clock: its dt comes from its own state and parameters exactly as in a standalone
 *     context, and a member that has reached t_target, used up max_steps or stopped on the drift bound sits out the
 *     rest of the call.  Members that never fell out of step compute bit for bit what standalone contexts with the same
 *     parameters compute.  When a call ends with members at different points of the re-binning schedule (they reached
 *     one t_target in different step counts) or a member hit the drift bound, every member is re-binned at once into one
 *     layout (a "realignment": summation order only); sphx_batch_info counts them.
 *
 *     Host arrays in MEX layout as in section 2, one block per member: pos / vel [n_members blocks of n_total x 2],
 *     drho_dt [n_members blocks of n_total]; mass [n_total] and wall_vel [n_total x 2] are shared.  prm [n_members];
 *     status [n_members].  A member that diverges stops the batch with SPHX_ERR_DIVERGED (the message names it).
 * ---------------------------------------------------------------------------------------------- */

typedef struct sphx_batch sphx_batch;

int sphx_batch_create(sphx_batch **batch, int n_members, const sphx_params *prm, int n_fluid, int n_total,
                      const double *pos, const double *vel, const double *drho_dt, const double *mass,
                      const double *wall_vel, double t0, int64_t step0);
void sphx_batch_destroy(sphx_batch *batch);
/* sphx_ctx_advance for every member: one t_target, one max_steps (<= 0: unlimited) */
int sphx_batch_advance(sphx_batch *batch, double t_target, int64_t max_steps, sphx_status *status);
/* sphx_ctx_enqueue_steps / sphx_ctx_sync for every member */
int sphx_batch_enqueue_steps(sphx_batch *batch, int64_t n_steps);
int sphx_batch_sync(sphx_batch *batch, sphx_status *status);
/* sphx_ctx_download / sphx_ctx_monitor of one member (SPHX:Batch:member when out of range) */
int sphx_batch_download(sphx_batch *batch, int member, double *pos, double *vel, double *rho, double *p,
                        double *drho_dt, double *force, double *force_prior, double *Vol, double *B);
int sphx_batch_monitor(sphx_batch *batch, int member, double *tau_bottom, double *tau_top, double *n_pairs);
/* the shared launch shape and grid policy; forced_rebuilds = realignments caused by the drift bound */
int sphx_batch_info(sphx_batch *batch, int *n_members, int *lanes_per_particle, int *steps_per_graph,
                    int *rebuild_every, double *skin, int64_t *forced_rebuilds, int64_t *realignments);
int sphx_batch_graph_stats(sphx_batch *batch, int64_t *slots_replayed, int64_t *slots_eager,
                           int64_t *graphs_captured);

/* ------------------------------------------------------------------------------------------------
 * 2a. Flow statistics: time-averaged velocity profiles accumulated on the device, inside the step loop.
 *
 *  Bins: the reference's profile binning (SPH_Poiseuille.m:579-605, profile.compute_binned_profile_mean):
 *    n_bins y-bins over [0, DH] with edges[k] = k * (DH / n_bins) and edges[n_bins] = DH (numpy's linspace);
 *    bin k holds edges[k] <= y < edges[k+1], the last bin also y == DH; fluid particles outside [0, DH] are
 *    dropped.  Wall particles are never binned.
 *  Bands: band 0 is the whole channel; bands 1 .. n_bands are x-bands (band_x[b-1], band_hw[b-1]) with the membership of
 *    compute_mid_channel_profile: xw = x mod DL, d = |xw - xc|, d = min(d, DL - d), member when d <= hw.  The
 *    reference's mid-channel monitor is (DL/2, max(dp, h)); a band around the periodic seam is (0, hw).
 *  Per bin and band: particle samples N, sum u_x, sum u_x^2, sum u_y, sum u_y^2 over all samples; per context the
 *    number of samples and the times of the first and the last one.  Only pos / vel are sampled.
 *  Sample point: the state a completed step leaves -- exactly what sphx_ctx_download returns for pos / vel after that
 *    step.  A step is sampled when its step count (sphx_status.step after it) is a multiple of `every` and it ends at
 *    t >= t_from.  Dual-rate contexts sample once per outer step.  The sampling kernel closes every step slot (it skips
 *    itself on the other steps) and is captured in the replayed graphs; enable / disable re-capture them, and with the
 *    statistics off a step enqueues exactly the launches it does without this feature.
 *  Determinism: a sample is summed exactly (int64 fixed point, scales picked per sample from the particle count and
 *    2 max|v|) and added to double running sums bin by bin: two identical runs give bit-identical sums, independent of
 *    particle order, re-binning and host chunking.  A velocity above that bound (a non-finite state) makes a later
 *    read fail with SPHX:Stats:range.
 *  Errors: SPHX:Stats:config (bad config), SPHX:Stats:band, SPHX:Stats:capacity, SPHX:Stats:disabled (SPHX_ERR_STATE),
 *    SPHX:Stats:range (SPHX_ERR_STATE); every call on a slab context fails with SPHX_ERR_ARG, SPHX:Stats:slab.
 * ---------------------------------------------------------------------------------------------- */

typedef struct sphx_flow_stats_config {
    int32_t n_bins;            /* 0 = max(20, floor(DH/dp + 0.5)), the reference's profile bins;
                                  n_bins * (n_bands + 1) <= 1536                                          */
    int32_t every;             /* sample every `every`-th completed step (step count % every == 0), >= 1 */
    double t_from;             /* only steps ending at t >= t_from                                       */
    int32_t n_bands;           /* 0..2 x-bands besides the whole channel                                 */
    double band_x[2], band_hw[2];
} sphx_flow_stats_config;

/* (Re)configure and zero the statistics; waits for the stream.  Off by default. */
int sphx_ctx_flow_stats_enable(sphx_ctx *ctx, const sphx_flow_stats_config *cfg);
/* Stop sampling (no-op when off); the sums are dropped. */
int sphx_ctx_flow_stats_disable(sphx_ctx *ctx);
/* Zero the sums and the sample count after everything enqueued has been taken. */
int sphx_ctx_flow_stats_reset(sphx_ctx *ctx);
/* Add one sample of the current state (what sphx_ctx_download would return) now, without gating. */
int sphx_ctx_flow_stats_sample(sphx_ctx *ctx);
/* Sums of band `band` (0 = whole channel), n_bins entries each; any array may be NULL (all NULL: capacity is not
 * checked, so n_bins can be asked for first).  Waits for and settles everything enqueued, like sphx_ctx_download.
 * t_first / t_last: simulated times of the first / last sample (NaN before the first). */
int sphx_ctx_flow_stats_read(sphx_ctx *ctx, int band, int capacity, int *n_bins, double *count, double *sum_ux,
                             double *sum_ux2, double *sum_uy, double *sum_uy2, int64_t *n_samples,
                             double *t_first, double *t_last);

/* ------------------------------------------------------------------------------------------------
 * 2c. Flow statistics of a batch (section 2b): the statistics of section 2a for every member at once.
 *
 *  One config for all members (bins and bands come from the shared geometry); every member has its own sums, sample
 *  count, t_first / t_last and range flag.  Each member is sampled on its own clock with the gating of section 2a, so a
 *  member that sits out slots (it reached t_target, used up its steps, stopped on the drift bound) is not sampled in
 *  them.  A member's sums are bit for bit those of a standalone context with the same parameters and config that took
 *  the same steps; realignments move particles only and change no sum.  With the statistics on, every step slot of the
 *  batch ends with one sampling launch for all members; off, a slot enqueues exactly the launches it does without this
 *  feature.  Enable / disable wait for the stream and re-capture the batch's graphs.  The sums take
 *  2 * n_members * (n_bands + 1) * n_bins * 5 doubles of device memory; when they do not fit, enable fails and the
 *  batch goes on without statistics.
 *  Errors: SPHX:Batch:null (NULL batch), SPHX:Stats:config, SPHX:Stats:band, SPHX:Stats:capacity, SPHX:Stats:disabled as in
 *  section 2a; SPHX:Stats:range names the member whose flag is set.
 * ---------------------------------------------------------------------------------------------- */

int sphx_batch_flow_stats_enable(sphx_batch *batch, const sphx_flow_stats_config *cfg);
int sphx_batch_flow_stats_disable(sphx_batch *batch);
/* settles what is enqueued, then zeroes */
int sphx_batch_flow_stats_reset(sphx_batch *batch);
/* settles; samples what sphx_batch_download returns, every member, without gating */
int sphx_batch_flow_stats_sample(sphx_batch *batch);
/* One call for all members.  Per-bin arrays are n_members blocks of `capacity` doubles (member m at m * capacity);
 * n_samples / t_first / t_last are [n_members].  All NULL: capacity is not checked.  Settles first, as
 * sphx_batch_download does. */
int sphx_batch_flow_stats_read(sphx_batch *batch, int band, int capacity, int *n_bins, double *count, double *sum_ux,
                               double *sum_ux2, double *sum_uy, double *sum_uy2, int64_t *n_samples,
                               double *t_first, double *t_last);

/* ------------------------------------------------------------------------------------------------
 * 2d. Step history: the scalar series of a run -- wall shear, kinetic energy, bulk velocity, dt and max |v| per step --
 *     recorded on the device, inside the step loop.  The reference computes the wall shear after every step
 *     (SPH_Poiseuille.m:281-283) and logs it with dt, vmax and the pair count (:285-291); sphx_ctx_monitor gives it at the
 *     price of a host round trip per call.
 *
 *  A record is SPHX_HISTORY_FIELDS doubles describing the state a completed step leaves -- exactly what sphx_ctx_download /
 *  sphx_ctx_monitor / sphx_status would report if called after that step:
 *    0 step            sphx_status.step after the step (exact as a double)
 *    1 t               sphx_status.t
 *    2 dt              sphx_status.dt_last (dual-rate contexts: the inner dt; t advanced by n_inner * dt)
 *    3 vmax            sphx_status.vmax
 *    4 tau_bottom      as sphx_ctx_monitor (sph_physics_mex.c:1713-1742): new neighbour structure and new pos / vel, with
 *    5 tau_top           Vol / B of the step just finished
 *    6 kinetic_energy  sum over the fluid particles of 1/2 mass (u_x^2 + u_y^2)
 *    7 u_bulk          arithmetic mean of u_x over the fluid particles
 *  Gating: as for the flow statistics (section 2a).  A step is recorded when its step count (sphx_status.step after it) is
 *    a multiple of `every` and it ends at t >= t_from.  Dual-rate contexts record once per outer step.  A step slot that did
 *    not run records nothing.
 *  Buffer: `capacity` records live in device memory and are filled in step order.  When the buffer is full further records
 *    are dropped and counted in n_dropped; it does not wrap.
 *  Off by default.  With it off a step slot enqueues exactly the launches it does without this feature; on, every step slot
 *    ends with one more launch (k_step_history, which skips itself on the steps gated out) that is captured in the
 *    replayed graphs; enable / disable re-capture them.  Independent of the flow statistics: both may be on at once.
 *  Determinism: no floating-point atomics; two identical runs give bit-identical records.  How the host chunks its calls
 *    changes the summation order of fields 4-7 only (the re-binning phase differs after a stop on the drift bound).
 *  Batches (section 2b) record one history per member: section 2f.
 *  Errors: SPHX:History:config (every < 1, capacity < 1 or > 1 << 22, non-finite t_from, or the allocation fails: the
 *    context then goes on without a history), SPHX:History:disabled (SPHX_ERR_STATE: a call that needs the history while
 *    it is off), SPHX:History:capacity (the caller's buffer is smaller than n_records); every call on a slab context fails
 *    with SPHX_ERR_ARG, SPHX:History:slab.
 * ---------------------------------------------------------------------------------------------- */

#define SPHX_HISTORY_FIELDS 8

typedef struct sphx_history_config {
    int32_t every;     /* record every `every`-th completed step (step count % every == 0), >= 1 */
    int32_t capacity;  /* records the device buffer holds, 1 .. 1 << 22                          */
    double t_from;     /* only steps ending at t >= t_from                                       */
} sphx_history_config;

/* (Re)configure and empty the buffer; waits for the stream. */
int sphx_ctx_history_enable(sphx_ctx *ctx, const sphx_history_config *cfg);
/* Stop recording (no-op when off); the records are dropped. */
int sphx_ctx_history_disable(sphx_ctx *ctx);
/* The records so far, in step order: records [capacity][SPHX_HISTORY_FIELDS], row-major (NULL: only the counts are
 * reported and capacity is not checked).  Waits for and settles everything enqueued, like sphx_ctx_download.  drain != 0:
 * the buffer is emptied and n_dropped zeroed after copying. */
int sphx_ctx_history_read(sphx_ctx *ctx, int capacity, double *records, int *n_records, int64_t *n_dropped, int drain);

/* ------------------------------------------------------------------------------------------------
 * 2e. Field maps: the velocity field sampled on a regular grid in x and y, accumulated on the device, inside the step
 *     loop.  The reference's result figure interpolates u_x onto such a grid on the host (panel (b) of
 *     SPH_Poiseuille_postprocess.m:184-201); a y-binned profile (section 2a) averages over x by construction and cannot
 *     show a seam defect or a standing structure along x.
 *
 *  Nodes: nx x ny of them, x_i = i * (DL / (nx - 1)) with x_{nx-1} = DL, y_k = k * (DH / (ny - 1)) with y_{ny-1} = DH
 *    (numpy's and MATLAB's linspace, both ends included).  nx = 0 / ny = 0: the reference's shape 2 * round(DL / dp),
 *    2 * round(DH / dp) (postprocess.m:185-186).  Column 0 and column nx - 1 are the same physical line of the periodic
 *    channel.  Node (i, k) is stored at i * ny + k: y fastest, like the cells -- a MATLAB [ny x nx] matrix in
 *    column-major order.
 *  One sample at a node: Shepard interpolation over the fluid particles, from pos and vel of the state sphx_ctx_download
 *    would return and nothing else.  dx = minimum image of x_node - x_j, dy = y_node - y_j; a particle contributes when
 *    dx^2 + dy^2 < (2h)^2 (no lower cut: a particle on a node contributes W(0)); W is the two-piece cubic spline of the
 *    physics (sigma = 10 / (7 pi h^2)); S0 = sum W, S1 = sum W u_x, S2 = sum W u_y.  with_walls = 1: the wall particles
 *    enter the same three sums with their wall velocity (the no-slip picture); the default is fluid only.  For DL < 4h a
 *    particle counts by its nearest image only, as in the neighbour search.
 *  Accumulated per node, as six planes of nx * ny doubles, when S0 > 0: count += 1, sum_w += S0 * dp^2 (about 1 inside
 *    the fluid, about 0.4 at a wall node with fluid only), sum_ux += S1 / S0, sum_uy += S2 / S0, sum_ux2 += (S1 / S0)^2,
 *    sum_uy2 += (S2 / S0)^2.  A node with no contributor is skipped for that sample; a node never sampled reads back
 *    with count = 0.  Per context: n_samples and the times of the first and the last sample (NaN before the first).
 *  Gating: as in sections 2a and 2d.  A step is sampled when its step count (sphx_status.step after it) is a multiple of
 *    `every` and it ends at t >= t_from.  Dual-rate contexts sample once per outer step.  A step slot that did not run
 *    samples nothing.
 *  Determinism: every node is owned by one thread, which adds its candidates in an order that depends on the particle
 *    layout only; no atomics.  Two identical runs give bit-identical planes; another layout (another re-binning phase,
 *    e.g. after a stop on the drift bound) changes the summation order only.
 *  Off by default.  With it off a step slot enqueues exactly the launches it does without this feature; on, every step
 *    slot ends with one more launch (k_field_map, behind k_flow_stats and k_step_history; it skips itself on the steps
 *    gated out) that is captured in the replayed graphs; enable / disable re-capture them.  Independent of the flow
 *    statistics and the step history: all three may be on at once.  The planes take 6 * nx * ny doubles of device memory.
 *  Batches (section 2b) keep one map per member: section 2g.  The slabs of a ring each keep a block of node columns: section 3a.
 *  Errors: SPHX:Field:config (nx or ny equal to 1 or negative, nx * ny > 1 << 25, every < 1, NaN t_from, with_walls not
 *    0 or 1, or the allocation fails: the context then goes on without a map), SPHX:Field:disabled (SPHX_ERR_STATE: a
 *    call that needs the map while it is off), SPHX:Field:capacity (the caller's arrays are smaller than nx * ny); every
 *    call on a slab context fails with SPHX_ERR_ARG, SPHX:Field:slab.
 * ---------------------------------------------------------------------------------------------- */

typedef struct sphx_field_map_config {
    int32_t nx, ny;      /* nodes along x / y, both ends included; 0 = 2 * round(DL / dp), 2 * round(DH / dp); never 1 */
    int32_t every;       /* sample every `every`-th completed step (step count % every == 0), >= 1 */
    int32_t with_walls;  /* 1: wall particles contribute with their wall velocity; 0: fluid only   */
    double t_from;       /* only steps ending at t >= t_from                                       */
} sphx_field_map_config;

/* (Re)configure and zero the map; waits for the stream.  Off by default. */
int sphx_ctx_field_map_enable(sphx_ctx *ctx, const sphx_field_map_config *cfg);
/* Stop sampling (no-op when off); the sums are dropped. */
int sphx_ctx_field_map_disable(sphx_ctx *ctx);
/* Zero the sums and the sample count after everything enqueued has been taken. */
int sphx_ctx_field_map_reset(sphx_ctx *ctx);
/* Add one sample of the current state (what sphx_ctx_download would return) now, without gating. */
int sphx_ctx_field_map_sample(sphx_ctx *ctx);
/* The six planes, nx * ny entries each, node (i, k) at i * ny + k; any array may be NULL (all NULL: capacity is not
 * checked, so the shape can be asked for first).  Waits for and settles everything enqueued, like sphx_ctx_download.
 * t_first / t_last: simulated times of the first / last sample (NaN before the first). */
int sphx_ctx_field_map_read(sphx_ctx *ctx, int capacity, int *nx, int *ny, double *count, double *sum_w,
                            double *sum_ux, double *sum_uy, double *sum_ux2, double *sum_uy2, int64_t *n_samples,
                            double *t_first, double *t_last);

/* ------------------------------------------------------------------------------------------------
 * 2f. Step history of a batch (section 2b): the history of section 2d for every member at once.
 *
 *  One config for all members; `capacity` is per member.  Every member has its own record buffer, n_records and
 *  n_dropped, and is recorded on its own clock with the gating of section 2d, so a member that sits out slots (it reached
 *  t_target, used up its steps, stopped on the drift bound) records nothing in them and its counters are not touched.  A
 *  member's records are bit for bit those of a standalone context with the same parameters and config that took the same
 *  steps: the same workgroups per member, the same runs of particles per workgroup, the same order of the partial sums.
 *  After a realignment (section 2b) a member's particles are laid out differently, which changes the summation order of
 *  fields 4-7 only, as a stop on the drift bound does for a context.  With the history on, every step slot of the batch
 *  ends with one recording launch for all members (k_step_history_b); off, a slot enqueues exactly the launches it does
 *  without this feature.  Enable / disable wait for the stream and re-capture the batch's graphs.  Independent of the
 *  batch's flow statistics (section 2c): both may be on at once.
 *  Memory: n_members * capacity * SPHX_HISTORY_FIELDS doubles.  Besides the per-member bound of section 2d,
 *  n_members * capacity must not exceed 1 << 24 records (1 GiB); when the buffers do not fit, enable fails and the batch
 *  goes on without a history.  A refused enable leaves a running history, and its records, untouched.
 *  Errors: SPHX:Batch:null (NULL batch), SPHX:History:config (as in section 2d, or n_members * capacity > 1 << 24),
 *  SPHX:History:disabled, SPHX:History:capacity (the caller's capacity is below the largest n_records of any member).
 * ---------------------------------------------------------------------------------------------- */

/* (Re)configure and empty every member's buffer; waits for the stream. */
int sphx_batch_history_enable(sphx_batch *batch, const sphx_history_config *cfg);
/* Stop recording (no-op when off); the records are dropped. */
int sphx_batch_history_disable(sphx_batch *batch);
/* One call for all members.  records is [n_members][capacity][SPHX_HISTORY_FIELDS], row-major: member m's records so far,
 * in step order, fill rows 0 .. n_records[m] - 1 of its block and the other rows are left as they are (NULL: only the
 * counts are reported and capacity is not checked).  n_records and n_dropped are [n_members]; either may be NULL.  Settles
 * first, as sphx_batch_download does.  drain != 0: every member's buffer is emptied and its n_dropped zeroed after
 * copying. */
int sphx_batch_history_read(sphx_batch *batch, int capacity, double *records, int *n_records, int64_t *n_dropped, int drain);

/* ------------------------------------------------------------------------------------------------
 * 2g. Field maps of a batch (section 2b): the map of section 2e for every member at once.
 *
 *  One config for all members; the shape comes from the shared geometry.  Every member has its own six planes, sample
 *  count and t_first / t_last, and is sampled on its own clock with the gating of section 2e, so a member that sits out
 *  slots (it reached t_target, used up its steps, stopped on the drift bound) is not sampled in them and neither its
 *  planes nor its count are touched.  A member's planes are bit for bit those of a standalone context with the same
 *  parameters and config that took the same steps: the same thread owns a node and adds its candidates in the same
 *  order.  After a realignment (section 2b) a member's particles are laid out differently, which changes the summation
 *  order only, as a stop on the drift bound does for a context.  With the map on, every step slot of the batch ends
 *  with one sampling launch for all members (k_field_map_b, behind the batch's statistics and history launches); off, a
 *  slot enqueues exactly the launches it does without this feature.  Enable / disable wait for the stream and
 *  re-capture the batch's graphs.  Independent of the batch's flow statistics (section 2c) and step history
 *  (section 2f): all three may be on at once.
 *  Memory: n_members * 6 * nx * ny doubles.  n_members * nx * ny must not exceed 1 << 25 nodes; when the planes do not
 *  fit, enable fails and the batch goes on without a map.  A refused enable leaves a running map, and its sums,
 *  untouched.
 *  Errors: SPHX:Batch:null (NULL batch), SPHX:Field:config (as in section 2e, or n_members * nx * ny > 1 << 25),
 *  SPHX:Field:disabled, SPHX:Field:capacity (the caller's capacity is below nx * ny).
 * ---------------------------------------------------------------------------------------------- */

/* (Re)configure and zero every member's map; waits for the stream. */
int sphx_batch_field_map_enable(sphx_batch *batch, const sphx_field_map_config *cfg);
/* Stop sampling (no-op when off); the sums are dropped. */
int sphx_batch_field_map_disable(sphx_batch *batch);
/* settles what is enqueued, then zeroes */
int sphx_batch_field_map_reset(sphx_batch *batch);
/* settles; samples what sphx_batch_download returns, every member, without gating */
int sphx_batch_field_map_sample(sphx_batch *batch);
/* One call for all members.  Each plane array is n_members blocks of `capacity` doubles: member m at m * capacity, node
 * (i, k) at i * ny + k within it, the rest of a block left as it is; any array may be NULL (all NULL: capacity is not
 * checked, so the shape can be asked for first).  n_samples / t_first / t_last are [n_members].  Settles first, as
 * sphx_batch_download does. */
int sphx_batch_field_map_read(sphx_batch *batch, int capacity, int *nx, int *ny, double *count, double *sum_w,
                              double *sum_ux, double *sum_uy, double *sum_ux2, double *sum_uy2, int64_t *n_samples,
                              double *t_first, double *t_last);

/* ------------------------------------------------------------------------------------------------
 * 2h. Point probes: the flow at fixed points, step by step, recorded on the device, inside the step loop.  The flow
 *     statistics (section 2a) and the field map (2e) average time away, the step history (2d) has the time axis and no
 *     place; a probe is resolved in both.  It is what shows a pulsation -- an acoustic wave sloshing across the channel is a
 *     line in the spectrum of rho and u_y at a point -- without a download and a host interpolation per step.
 *
 *  Points: P of them, (x_p, y_p), 1 <= P <= SPHX_PROBE_MAX_POINTS, given at enable and copied.  x may be any finite value
 *    and is folded into [0, DL) on the host (x - floor(x / DL) * DL; x = DL and x = -DL become 0); 0 <= y <= DH.
 *  One sample at a point: the field map's sample at a node (section 2e) plus a density, from pos, vel and mass of the state
 *    sphx_ctx_download would return and nothing else.  dx = minimum image of x_p - x_j, dy = y_p - y_j; a particle
 *    contributes when dx^2 + dy^2 < (2h)^2 (no lower cut); W is the two-piece cubic spline of the physics; S0 = sum W,
 *    S1 = sum W u_x, S2 = sum W u_y over the fluid particles, and Sm = sum m_j W_j.  with_walls = 1: the wall particles
 *    enter S0, S1 and S2 with their wall velocity, exactly as in the map.  Sm is always the sum over the fluid particles
 *    alone: the summation density from the fluid; within 2h of a wall it lacks the wall's share.
 *  Values: SPHX_PROBE_FIELDS = 4 per probe and sample:
 *    0 weight   S0 * dp^2 (about 1 inside the fluid)
 *    1 u_x      S1 / S0
 *    2 u_y      S2 / S0
 *    3 rho      Sm (p0 * (rho / rho0 - 1) is a pressure)
 *    Where S0 = 0 (no contributor): weight = 0, rho = 0 and both velocities are NaN -- the series' "no value".
 *  Records: one per sampled step: `step` and `t` (two doubles, as the history stores them: sphx_status.step and .t after the
 *    step) and the P x 4 values, in the arrays times[capacity][2] and values[capacity][P][4].  `capacity` records live in
 *    device memory and are filled in step order; when the buffer is full further records are dropped and counted in
 *    n_dropped; it does not wrap (the semantics of section 2d).  capacity >= 1, and capacity * P * 4 <= 1 << 27 doubles.
 *  Gating: as in sections 2a / 2d / 2e.  A step is recorded when its step count (sphx_status.step after it) is a multiple
 *    of `every` and it ends at t >= t_from.  Dual-rate contexts record once per outer step.  A step slot that did not run
 *    records nothing.  sphx_ctx_probes_sample appends a record of the state now, without gating.
 *  Determinism: one wave per probe; a lane adds its candidates in an order that depends on the particle layout only, the
 *    lanes' sums are reduced in a fixed order; no floating-point atomics.  Two identical runs give bit-identical records;
 *    another layout (another re-binning phase, e.g. after a stop on the drift bound) changes the summation order only.
 *  Off by default.  With it off a step slot enqueues exactly the launches it does without this feature; on, every step slot
 *    ends with one more launch (k_point_probes, behind k_field_map; it skips itself on the steps gated out) that is captured
 *    in the replayed graphs; enable / disable re-capture them.  Independent of the other three samplers: all four may be on
 *    at once.  Batches (section 2b) record one series per member: section 2i.
 *  Errors: SPHX:Probe:config (NULL config or points, n_points out of range, a non-finite coordinate, y outside [0, DH],
 *    every < 1, capacity < 1 or capacity * n_points * 4 > 1 << 27, non-finite t_from, with_walls not 0 or 1, or the
 *    allocation fails: the context then goes on without probes), SPHX:Probe:disabled (SPHX_ERR_STATE: a call that needs
 *    the probes while they are off), SPHX:Probe:capacity (the caller's arrays are smaller than n_records); every call on
 *    a slab context fails with SPHX_ERR_ARG, SPHX:Probe:slab (the probes of a ring: sphx_slab_probes_*, section 3a).  A refused enable leaves running probes, and their
 *    records, untouched.
 * ---------------------------------------------------------------------------------------------- */

#define SPHX_PROBE_FIELDS 4
#define SPHX_PROBE_MAX_POINTS 4096

typedef struct sphx_probes_config {
    int32_t n_points;      /* P, 1 .. SPHX_PROBE_MAX_POINTS                                          */
    int32_t every;         /* record every `every`-th completed step (step count % every == 0), >= 1 */
    int32_t capacity;      /* records the device buffer holds, >= 1                                  */
    int32_t with_walls;    /* 1: wall particles contribute to S0, S1, S2 with their wall velocity    */
    double t_from;         /* only steps ending at t >= t_from                                       */
    const double *points;  /* [n_points][2]: x, y; copied at enable                                  */
} sphx_probes_config;

/* (Re)configure and empty the buffer; waits for the stream.  Off by default. */
int sphx_ctx_probes_enable(sphx_ctx *ctx, const sphx_probes_config *cfg);
/* Stop recording (no-op when off); the records are dropped. */
int sphx_ctx_probes_disable(sphx_ctx *ctx);
/* Append one record of the current state (what sphx_ctx_download would return) now, without gating. */
int sphx_ctx_probes_sample(sphx_ctx *ctx);
/* The records so far, in step order: times [capacity][2] and values [capacity][n_points][SPHX_PROBE_FIELDS], row-major
 * (times / values NULL: that array is not copied; both NULL: only the counts are reported and capacity is not checked).
 * Waits for and settles everything enqueued, like sphx_ctx_download.  drain != 0: the buffer is emptied and n_dropped
 * zeroed after copying. */
int sphx_ctx_probes_read(sphx_ctx *ctx, int capacity, double *times, double *values, int *n_points, int *n_records,
                         int64_t *n_dropped, int drain);

/* ------------------------------------------------------------------------------------------------
 * 2i. Point probes of a batch (section 2b): the probes of section 2h for every member at once.
 *
 *  One config and one set of points for all members; `capacity` is per member.  Every member has its own record buffer,
 *  n_records and n_dropped, and is recorded on its own clock with the gating of section 2h, so a member that sits out slots
 *  records nothing in them and its counters are not touched.  A member's records are bit for bit those of a standalone
 *  context with the same parameters and config that took the same steps: the same wave owns a probe and its lanes add the
 *  same candidates in the same order.  After a realignment (section 2b) a member's particles are laid out differently,
 *  which changes the summation order only.  With probes on, every step slot of the batch ends with one recording launch
 *  for all members (k_point_probes_b, behind the batch's other samplers); off, a slot enqueues exactly the launches it
 *  does without this feature.  Enable / disable wait for the stream and re-capture the batch's graphs.
 *  Memory: n_members * capacity * (2 + n_points * 4) doubles; n_members * capacity * n_points * 4 must not exceed
 *  1 << 27 doubles.  A refused enable leaves running probes, and their records, untouched.
 *  Errors: SPHX:Batch:null (NULL batch), SPHX:Probe:config (as in section 2h, with the total over the members),
 *  SPHX:Probe:disabled, SPHX:Probe:capacity (the caller's capacity is below the largest n_records of any member).
 * ---------------------------------------------------------------------------------------------- */

/* (Re)configure and empty every member's buffer; waits for the stream. */
int sphx_batch_probes_enable(sphx_batch *batch, const sphx_probes_config *cfg);
/* Stop recording (no-op when off); the records are dropped. */
int sphx_batch_probes_disable(sphx_batch *batch);
/* settles; appends a record of what sphx_batch_download returns, every member, without gating */
int sphx_batch_probes_sample(sphx_batch *batch);
/* One call for all members.  times is [n_members][capacity][2] and values [n_members][capacity][n_points][SPHX_PROBE_FIELDS],
 * row-major: member m's block lies behind member m - 1's, its records fill rows 0 .. n_records[m] - 1 and the other rows are
 * left as they are.  n_records and n_dropped are [n_members]; any pointer may be NULL.  Settles first, as
 * sphx_batch_download does.  drain != 0: every member's buffer is emptied and its n_dropped zeroed after copying. */
int sphx_batch_probes_read(sphx_batch *batch, int capacity, double *times, double *values, int *n_points, int *n_records,
                           int64_t *n_dropped, int drain);

/* ------------------------------------------------------------------------------------------------
 * 2j. Profile series: the binned velocity profile at every sampled step, recorded on the device, inside the step loop.
 *     "Flow statistics (section 2a) that record instead of accumulate": the statistics and the field map (2e) average time
 *     away, the step history (2d) and the point probes (2h) have no y-profile.  The series is what shows a profile DEVELOP
 *     -- the start-up of plane Poiseuille flow from rest, whose series solution is known in closed form
 *     (profile.poiseuille_startup) -- without a download and a host binning per sample.
 *
 *  One sample: exactly the flow statistics' sample of section 2a -- the same bins (n_bins = 0: the reference's), band 0 the
 *    whole channel plus up to two x-bands, and per bin and band the five values N, sum u_x, sum u_x^2, sum u_y, sum u_y^2 of
 *    THAT step, summed exactly in int64 fixed point.  Only pos / vel are sampled.
 *  Records: one per sampled step: `step` and `t` (two doubles: sphx_status.step and .t after the step) in
 *    times[capacity][2], and the sample in records[capacity][n_bands + 1][n_bins][SPHX_PROFILE_SERIES_FIELDS].  `capacity`
 *    records live in device memory and are filled in step order; when the buffer is full further records are dropped and
 *    counted in n_dropped; it does not wrap (the semantics of sections 2d / 2h).  A record is (n_bands + 1) * n_bins * 5
 *    doubles: at dp = 0.025 with two bands 3.2 KB, not the 64 B of a history record -- size `capacity` accordingly (the
 *    wrappers default to 4 096, not the history's 65 536).  Cap: capacity * (n_bands + 1) * n_bins * 5 <= 1 << 27 doubles
 *    (1 GiB), over all members of a batch.
 *  Gating: as in section 2a: a step is recorded when its step count (sphx_status.step after it) is a multiple of `every` and
 *    it ends at t >= t_from.  Dual-rate contexts record once per outer step.  A step slot that did not run records nothing.
 *    sphx_ctx_profile_series_sample appends a record of the state now, without gating.
 *  Determinism: a sample is summed exactly and every value of a record is converted from its integer by one thread: two
 *    identical runs give bit-identical records, independent of particle order, re-binning and host chunking, and adding the
 *    records of a series in order gives the sums of section 2a (same config) to the bit.  A velocity above the bound of
 *    section 2a (a non-finite state) makes a later read fail with SPHX:ProfileSeries:range.
 *  Off by default.  With it off a step slot enqueues exactly the launches it does without this feature; on, every step slot
 *    ends with one more launch (k_profile_series, behind k_point_probes; it skips itself on the steps gated out) that is
 *    captured in the replayed graphs; enable / disable re-capture them.  Independent of the other four samplers.
 *  Errors: SPHX:ProfileSeries:config (NULL config, n_bins < 0, every < 1, capacity < 1, a NaN t_from, n_bands outside
 *    0..2, a band centre or half-width that is not finite or a negative half-width, n_bins * (n_bands + 1) > 1536, the cap on
 *    the record buffer, or the allocation fails: the context then goes on without a series), SPHX:ProfileSeries:disabled
 *    (SPHX_ERR_STATE: a call that needs the series while it is off), SPHX:ProfileSeries:range (SPHX_ERR_STATE),
 *    SPHX:ProfileSeries:capacity (the caller's arrays are smaller than n_records); every call on a slab context fails with
 *    SPHX_ERR_ARG, SPHX:ProfileSeries:slab (the series of a ring: sphx_slab_pseries_*, section 3a).  A refused enable leaves
 *    a running series, and its records, untouched.
 * ---------------------------------------------------------------------------------------------- */

#define SPHX_PROFILE_SERIES_FIELDS 5

typedef struct sphx_profile_series_config {
    int32_t n_bins;            /* 0 = max(20, floor(DH/dp + 0.5)), the reference's profile bins;
                                  n_bins * (n_bands + 1) <= 1536                                          */
    int32_t every;             /* record every `every`-th completed step (step count % every == 0), >= 1 */
    int32_t capacity;          /* records the device buffer holds, >= 1                                  */
    double t_from;             /* only steps ending at t >= t_from                                       */
    int32_t n_bands;           /* 0..2 x-bands besides the whole channel                                 */
    double band_x[2], band_hw[2];
} sphx_profile_series_config;

/* (Re)configure and empty the buffer; waits for the stream.  Off by default. */
int sphx_ctx_profile_series_enable(sphx_ctx *ctx, const sphx_profile_series_config *cfg);
/* Stop recording (no-op when off); the records are dropped. */
int sphx_ctx_profile_series_disable(sphx_ctx *ctx);
/* Append one record of the current state (what sphx_ctx_download would return) now, without gating. */
int sphx_ctx_profile_series_sample(sphx_ctx *ctx);
/* The records so far, in step order: times [capacity][2] and records [capacity][*n_bands][*n_bins][5], row-major, where
 * *n_bands counts band 0 (times / records NULL: that array is not copied; both NULL: only the shape and the counts are
 * reported and capacity is not checked).  Waits for and settles everything enqueued, like sphx_ctx_download.  drain != 0:
 * the buffer is emptied and n_dropped zeroed after copying. */
int sphx_ctx_profile_series_read(sphx_ctx *ctx, int capacity, double *times, double *records, int *n_bins, int *n_bands,
                                 int *n_records, int64_t *n_dropped, int drain);

/* ------------------------------------------------------------------------------------------------
 * 2k. Profile series of a batch (section 2b): the series of section 2j for every member at once.
 *
 *  One config for all members (bins and bands come from the shared geometry); `capacity` is per member.  Every member has
 *  its own record buffer, n_records, n_dropped and range flag, and is recorded on its own clock with the gating of section
 *  2j, so a member that sits out slots records nothing in them and its counters are not touched.  A member's records are
 *  bit for bit those of a standalone context with the same parameters and config that took the same steps; realignments
 *  move particles only and change no record.  With the series on, every step slot of the batch ends with one recording
 *  launch for all members (k_profile_series_b, behind the batch's other samplers); off, a slot enqueues exactly the
 *  launches it does without this feature.  Enable / disable wait for the stream and re-capture the batch's graphs.
 *  Memory: n_members * capacity * (2 + (n_bands + 1) * n_bins * 5) doubles; n_members * capacity * (n_bands + 1) * n_bins * 5
 *  must not exceed 1 << 27 doubles.  A refused enable leaves a running series, and its records, untouched.
 *  Errors: SPHX:Batch:null (NULL batch), SPHX:ProfileSeries:config (as in section 2j, with the total over the members),
 *  SPHX:ProfileSeries:disabled, SPHX:ProfileSeries:capacity (the caller's capacity is below the largest n_records of any
 *  member); SPHX:ProfileSeries:range names the member whose flag is set.
 * ---------------------------------------------------------------------------------------------- */

/* (Re)configure and empty every member's buffer; waits for the stream. */
int sphx_batch_profile_series_enable(sphx_batch *batch, const sphx_profile_series_config *cfg);
/* Stop recording (no-op when off); the records are dropped. */
int sphx_batch_profile_series_disable(sphx_batch *batch);
/* settles; appends a record of what sphx_batch_download returns, every member, without gating */
int sphx_batch_profile_series_sample(sphx_batch *batch);
/* One call for all members.  times is [n_members][capacity][2] and records [n_members][capacity][*n_bands][*n_bins][5],
 * row-major: member m's block lies behind member m - 1's, its records fill rows 0 .. n_records[m] - 1 and the other rows are
 * left as they are.  n_records and n_dropped are [n_members]; any pointer may be NULL.  Settles first, as
 * sphx_batch_download does.  drain != 0: every member's buffer is emptied and its n_dropped zeroed after copying. */
int sphx_batch_profile_series_read(sphx_batch *batch, int capacity, double *times, double *records, int *n_bins, int *n_bands,
                                   int *n_records, int64_t *n_dropped, int drain);

/* ------------------------------------------------------------------------------------------------
 * 2l. Pair statistics: the pair-distance histogram of the fluid particles, counted on the device, inside the step loop.
 *     The five samplers above describe the velocity field; this one describes the particle ARRANGEMENT: the radial
 *     distribution function g(r), the mean neighbour count, the width of the first shell and the smallest separation --
 *     what pairing or clumping, a missing neighbour at the periodic seam or a transport_coeff that is too small show in first.
 *     It is integer work and therefore EXACT: profile.pair_histogram (numpy) reproduces it count for count.
 *
 *  Centres: a fluid particle i with y_margin <= y_i <= DH - y_margin.  Band 0 is the whole channel, bands 1..2 are x-bands
 *    with the membership rule of section 2a (x mod DL within half_width of the centre, the short way round).
 *  Partners: every fluid particle j != i (by slot), anywhere; with_walls: also every wall particle, in a histogram of its own.
 *  Distance: dx = x_i - x_j folded by the minimum image (dx > DL/2 -> dx - DL, dx < -DL/2 -> dx + DL), dy = y_i - y_j,
 *    r2 = dx*dx + dy*dy rounded after every operation (no fused multiply-add): the very double numpy computes.  Only the
 *    nearest image counts: a channel shorter than 4h can hold a second image of a partner within 2h, and that one is missed.
 *  Bins: n_bins uniform bins in r on [0, r_max).  Squared edges e2[k] = (k * (r_max / n_bins))^2 for k < n_bins and
 *    e2[n_bins] = r_max * r_max; bin k holds e2[k] <= r2 < e2[k+1]; r2 >= e2[n_bins] is not counted; coincident particles
 *    (r2 = 0) count in bin 0.  Comparisons against e2 decide the bin (numpy: searchsorted(e2, r2, side="right") - 1).
 *  Limits: r_max = 0 means 2h, otherwise 0 < r_max <= 2h: beyond 2h the sweep of the three cell columns around a centre is no
 *    longer complete, so it is refused.  1 <= n_bins <= 1024: with three bands and walls that is 6144 counters, which with the
 *    bands' centres and minima are the 49 200 B of LDS a workgroup of the sampler asks for: every allowed combination fits.
 *  Sums, per band, over all samples, all int64: `centres`, ff[n_bins] (ordered fluid-fluid pairs: a pair of two centres counts
 *    twice), fw[n_bins] (fluid-wall pairs; zeros without walls), and r2_min, a double: the smallest fluid-fluid r2 among the
 *    counted pairs so far, +inf before any.  Per sampler: n_samples, t_first, t_last.
 *  Gating: as in section 2a: a step is sampled when its step count (sphx_status.step after it) is a multiple of `every` and
 *    it ends at t >= t_from.  Dual-rate contexts sample once per outer step.  sphx_ctx_pair_dist_sample adds a sample of
 *    the state now, without gating.
 *  Determinism: integer sums and a minimum do not depend on the order they arrive in: the sums are independent of particle
 *    order, layout (lanes_per_particle, skin, dynamic_rebin), re-binning phase and batch membership, to the last count.
 *  Off by default.  With it off a step slot enqueues exactly the launches it does without this feature; on, every step slot
 *    ends with one more launch (k_pair_dist, behind k_profile_series; it skips itself on the steps gated out) that is
 *    captured in the replayed graphs; enable / disable re-capture them.  A sample costs 1.6 to 1.9 cell sweeps of the step's
 *    density pass: `every` is the control.  Independent of the other five samplers.
 *  Errors: SPHX:PairDist:config (NULL config, n_bins outside 1..1024, every < 1, a NaN t_from, r_max that is not finite,
 *    negative or above 2h, a y_margin that is not finite or negative, with_walls not 0 / 1, n_bands outside 0..2, a band
 *    centre or half-width that is not finite or a negative half-width, or the allocation fails: the context
 *    then goes on without pair statistics), SPHX:PairDist:band, SPHX:PairDist:capacity (ff or fw given and capacity <
 *    n_bins), SPHX:PairDist:disabled (SPHX_ERR_STATE: a call that needs the sampler while it is off); every call on a slab
 *    context fails with SPHX_ERR_ARG, SPHX:PairDist:slab (the pair statistics of a ring: sphx_slab_pairs_*, section 3a).  A
 *    refused enable leaves a running sampler, and its sums, untouched.
 * ---------------------------------------------------------------------------------------------- */

#define SPHX_PAIR_DIST_MAX_BINS 1024

typedef struct sphx_pair_dist_config {
    int32_t n_bins;            /* 1..1024 uniform bins in r on [0, r_max)                                */
    int32_t every;             /* sample every `every`-th completed step (step count % every == 0), >= 1 */
    double t_from;             /* only steps ending at t >= t_from                                       */
    double r_max;              /* 0 = 2h; otherwise 0 < r_max <= 2h                                      */
    double y_margin;           /* centres: y_margin <= y <= DH - y_margin, >= 0                          */
    int32_t with_walls;        /* 1: the wall particles are partners too, in fw                          */
    int32_t n_bands;           /* 0..2 x-bands besides the whole channel                                 */
    double band_x[2], band_hw[2];
} sphx_pair_dist_config;

/* (Re)configure and zero the sums; waits for the stream.  Off by default. */
int sphx_ctx_pair_dist_enable(sphx_ctx *ctx, const sphx_pair_dist_config *cfg);
/* Stop sampling (no-op when off); the sums are dropped. */
int sphx_ctx_pair_dist_disable(sphx_ctx *ctx);
/* Zero the sums and the sample count; the configuration stays. */
int sphx_ctx_pair_dist_reset(sphx_ctx *ctx);
/* Add one sample of the current state (what sphx_ctx_download would return) now, without gating. */
int sphx_ctx_pair_dist_sample(sphx_ctx *ctx);
/* The sums of one band so far: ff and fw are [capacity] (capacity >= n_bins where either is given), every pointer may be
 * NULL.  Waits for and settles everything enqueued, like sphx_ctx_download.  t_first / t_last are NaN before a sample. */
int sphx_ctx_pair_dist_read(sphx_ctx *ctx, int band, int capacity, int *n_bins, int64_t *ff, int64_t *fw, int64_t *centres,
                            double *r2_min, int64_t *n_samples, double *t_first, double *t_last);

/* ------------------------------------------------------------------------------------------------
 * 2m. Pair statistics of a batch (section 2b): the sums of section 2l for every member at once.
 *
 *  One config for all members (h, DL, DH and the walls come from the shared geometry).  Every member has its own block of
 *  sums and its own head and is sampled on its own clock with the gating of section 2l, so a member that sits out slots is
 *  not sampled in them.  The sums are exact: a member's are those of a standalone context with the same parameters and
 *  config that took the same steps; realignments move particles between slots only and change no count.  With the sampler
 *  on, every step slot of the batch ends with one launch for all members (k_pair_dist_b, behind the batch's other
 *  samplers); off, a slot enqueues exactly the launches it does without this feature.  Memory: n_members blocks of
 *  (n_bands + 1) * (n_bins * (1 + with_walls) + 2) words of 8 bytes.  A refused enable leaves a running sampler untouched.
 *  Errors: SPHX:Batch:null (NULL batch) and those of section 2l.
 * ---------------------------------------------------------------------------------------------- */

int sphx_batch_pair_dist_enable(sphx_batch *batch, const sphx_pair_dist_config *cfg);
int sphx_batch_pair_dist_disable(sphx_batch *batch);
int sphx_batch_pair_dist_reset(sphx_batch *batch);
/* settles; adds a sample of what sphx_batch_download returns, every member, without gating */
int sphx_batch_pair_dist_sample(sphx_batch *batch);
/* One call for all members: ff and fw are [n_members][capacity] (member m's bins at m * capacity), centres, r2_min,
 * n_samples, t_first and t_last are [n_members]; any pointer may be NULL.  Settles first, as sphx_batch_download does. */
int sphx_batch_pair_dist_read(sphx_batch *batch, int band, int capacity, int *n_bins, int64_t *ff, int64_t *fw, int64_t *centres,
                              double *r2_min, int64_t *n_samples, double *t_first, double *t_last);

/* ------------------------------------------------------------------------------------------------
 * 2n. Gradient statistics: the velocity gradient at every fluid particle, estimated and binned on the device, inside the
 *     step loop: the shear-rate profile du_x/dy (hence the shear stress tau(y) = mu du_x/dy, which the momentum balance makes
 *     linear in y), the velocity divergence (how weakly compressible the flow really is) and the vorticity.  The step
 *     history's wall shear (section 2d) is two scalars at the walls; this is the profile across the channel.
 *
 *  Estimate: for every fluid particle i, over every other fluid particle j within 2h (nearest image in x, r2 > 1e-24) and,
 *    with_walls, every wall particle within 2h (with the wall's velocity):
 *        d = r_i - r_j,  w_j = V_j W'(|d|) / |d|,  V_j = mass_j / rho0 (a wall particle: its volume),  W' the cubic spline's
 *        M_i = - sum_j w_j d (x) d        A_i = sum_j w_j (v_j - v_i) (x) d        G_i = A_i M_i^-1
 *    G_ab = d u_a / d x_b: g_xx, g_xy, g_yx, g_yy.  The estimate is exact for any linear velocity field whatever the particle
 *    arrangement, and first order at the one-sided support next to a wall.  with_walls is off by default: the wall particles
 *    carry the wall's velocity, not the extrapolated one, and pull the estimate of the wall-adjacent bin down (2.65 against
 *    the exact 3.80 in units of U_max / DH on the analytic parabola at dp = 0.05; without them 3.56).
 *  Skipped: a particle with det M_i <= det_min (no partner, or collinear ones), with a component of G_i that is not finite,
 *    or with one above the sample's bound 2^e > 16 vmax / h in magnitude (vmax: sphx_status.vmax of the step) is counted in
 *    `skipped` and summed nowhere.  This is not an error.
 *  Bins and bands: those of section 2a -- n_bins y-bins over [0, DH] (0: the reference's profile bins), y outside dropped,
 *    band 0 the whole channel, up to two x-bands.  Per bin and band count + skipped equals the flow statistics' count.
 *  Sums, per bin and band, over all samples, SPHX_GRAD_STATS_FIELDS = 12 doubles in this order: count, sum g_xx, sum g_xy,
 *    sum g_yx, sum g_yy, sum g_xx^2, sum g_xy^2, sum g_yx^2, sum g_yy^2, sum div^2 (div = g_xx + g_yy), sum omega^2
 *    (omega = g_yx - g_xy), skipped.  count and skipped are integers held in doubles.  Per sampler: n_samples, t_first, t_last.
 *  Exactness: a sample is summed in int64 fixed point at power-of-two scales picked from the particle count and the bound, so
 *    the sums are bit-identical between runs and independent of the workgroups' dispatch order, and a batch member's are a
 *    standalone context's.  Unlike the pair statistics' counts they DO depend on the order of the particle slots (a particle's
 *    partners are added in slot order): two layouts of one state agree within floating-point rounding, not bit for bit.
 *  Limits: n_bins * (n_bands + 1) <= 640, the 61 440 B of LDS counters of a workgroup.
 *  Gating: as in section 2l.  sphx_ctx_grad_stats_sample adds a sample of the state now, without gating.
 *  Off by default.  With it off a step slot enqueues exactly the launches it does without this feature; on, every step slot
 *    ends with one more launch (k_grad_stats, behind k_pair_dist; it skips itself on the steps gated out) that is captured
 *    in the replayed graphs; enable / disable re-capture them.  A sample costs 2.6 to 3.5 cell sweeps of the step's density
 *    pass (1.5 to 1.8 samples of the pair statistics): `every` is the control.  Independent of the other six samplers.
 *  Errors: SPHX:GradStats:config (NULL config, n_bins < 0 or n_bins * (n_bands + 1) > 640, every < 1, a NaN t_from, a det_min
 *    that is not finite or negative, with_walls not 0 / 1, n_bands outside 0..2, a band centre or half-width that is not
 *    finite or a negative half-width, or the allocation fails: the context then goes on without gradient statistics),
 *    SPHX:GradStats:band, SPHX:GradStats:capacity (sums given and capacity < n_bins), SPHX:GradStats:disabled (SPHX_ERR_STATE:
 *    a call that needs the sampler while it is off); every call on a slab context fails with SPHX_ERR_ARG,
 *    SPHX:GradStats:slab (the gradient statistics of a ring: sphx_slab_gstats_*, section 3a).  A refused enable leaves a running sampler, and its sums, untouched.
 * ---------------------------------------------------------------------------------------------- */

#define SPHX_GRAD_STATS_FIELDS 12
#define SPHX_GRAD_STATS_MAX_BINS 640

typedef struct sphx_grad_stats_config {
    int32_t n_bins;            /* y-bins over [0, DH]; 0 = the reference's profile bins                  */
    int32_t every;             /* sample every `every`-th completed step (step count % every == 0), >= 1 */
    double t_from;             /* only steps ending at t >= t_from                                       */
    double det_min;            /* a particle with det M <= det_min is skipped; >= 0 (0.05 is a good default) */
    int32_t with_walls;        /* 1: the wall particles are partners too, with the wall's velocity       */
    int32_t n_bands;           /* 0..2 x-bands besides the whole channel                                 */
    double band_x[2], band_hw[2];
} sphx_grad_stats_config;

/* (Re)configure and zero the sums; waits for the stream.  Off by default. */
int sphx_ctx_grad_stats_enable(sphx_ctx *ctx, const sphx_grad_stats_config *cfg);
/* Stop sampling (no-op when off); the sums are dropped. */
int sphx_ctx_grad_stats_disable(sphx_ctx *ctx);
/* Zero the sums and the sample count; the configuration stays. */
int sphx_ctx_grad_stats_reset(sphx_ctx *ctx);
/* Add one sample of the current state (what sphx_ctx_download would return) now, without gating. */
int sphx_ctx_grad_stats_sample(sphx_ctx *ctx);
/* The sums of one band so far: sums is [SPHX_GRAD_STATS_FIELDS][capacity] (field f of bin k at f * capacity + k; capacity >=
 * n_bins where it is given), every pointer may be NULL.  Waits for and settles everything enqueued, like sphx_ctx_download.
 * t_first / t_last are NaN before a sample. */
int sphx_ctx_grad_stats_read(sphx_ctx *ctx, int band, int capacity, int *n_bins, double *sums, int64_t *n_samples, double *t_first,
                             double *t_last);

/* ------------------------------------------------------------------------------------------------
 * 2o. Gradient statistics of a batch (section 2b): the sums of section 2n for every member at once.
 *
 *  One config for all members (bins, bands and the walls come from the shared geometry).  Every member has its own block of
 *  sums and its own head and is sampled on its own clock, with its own rho0, with the gating of section 2n, so a member that
 *  sits out slots is not sampled in them.  A member's sums are, bit for bit, those of a standalone context with the same
 *  parameters and config that took the same steps in the same slot order; a realignment reorders a member's slots, after
 *  which its sums agree within floating-point rounding and its counts exactly.  With the sampler on, every step slot of the
 *  batch ends with one launch for all members (k_grad_stats_b, behind the batch's other samplers); off, a slot enqueues
 *  exactly the launches it does without this feature.  A refused enable leaves a running sampler untouched.
 *  Errors: SPHX:Batch:null (NULL batch) and those of section 2n.
 * ---------------------------------------------------------------------------------------------- */

int sphx_batch_grad_stats_enable(sphx_batch *batch, const sphx_grad_stats_config *cfg);
int sphx_batch_grad_stats_disable(sphx_batch *batch);
int sphx_batch_grad_stats_reset(sphx_batch *batch);
/* settles; adds a sample of what sphx_batch_download returns, every member, without gating */
int sphx_batch_grad_stats_sample(sphx_batch *batch);
/* One call for all members: sums is [n_members][SPHX_GRAD_STATS_FIELDS][capacity], n_samples, t_first and t_last are
 * [n_members]; any pointer may be NULL.  Settles first, as sphx_batch_download does. */
int sphx_batch_grad_stats_read(sphx_batch *batch, int band, int capacity, int *n_bins, double *sums, int64_t *n_samples,
                               double *t_first, double *t_last);

/* ------------------------------------------------------------------------------------------------
 * 2p. Particle tracers: chosen particles followed step by step, recorded on the device, inside the step loop.  The other
 *     samplers are Eulerian -- they report what passes a bin, a node or a point; a tracer record follows the particle.  In
 *     laminar Poiseuille flow a fluid element never leaves its streamline, so every cross-stream displacement of a tracer is
 *     numerical, and u_x of a tracer against the analytic u(y) at its own y is the Lagrangian velocity error.
 *
 *  Tracers: T of them, 1 <= T <= n_fluid, each a fluid row number of the caller's order (0 <= id < n_fluid: the row of
 *    sphx_ctx_download), given at enable and copied, in any order.  A duplicate, an id out of range or a wall row
 *    (n_fluid <= id < n_total) is refused.
 *  Values: SPHX_TRACER_FIELDS = 4 per tracer and record: x, y, u_x, u_y of the particle, copied from the pos and vel the step
 *    slot left -- exactly what sphx_ctx_download would return in that row, x wrapped into the period as the state holds it,
 *    no arithmetic on the values.  Column k of a record is tracer k of the caller's list.
 *  Records: one per sampled step: `step` and `t` (two doubles, as the probes and the history store them) and the T x 4
 *    values, in the arrays times[capacity][2] and values[capacity][T][4].  `capacity` records live in device memory and are
 *    filled in step order; when the buffer is full further records are dropped and counted in n_dropped; it does not wrap
 *    (the semantics of sections 2d and 2h).  capacity >= 1, and capacity * T * 4 <= 1 << 27 doubles.
 *  Gating: as in the other samplers.  A step is recorded when its step count (sphx_status.step after it) is a multiple of
 *    `every` and it ends at t >= t_from.  Dual-rate contexts record once per outer step.  A step slot that did not run
 *    records nothing.  sphx_ctx_tracers_sample appends a record of the state now, without gating.
 *  n_missing: every id of the list must be met in exactly one slot of the population.  The kernel counts the tracers it met
 *    and adds T minus that count to a sticky counter, reported by the read and cleared by enable and by a draining read.  On
 *    a context and on a member of a batch it is always 0: it is the invariant of the library's id bookkeeping.
 *  Determinism: a column has exactly one writer and the values are copies: records are bit-identical between runs, between a
 *    member of a batch and a standalone context, between replayed and eager step slots, and whatever the particle layout.
 *  Off by default.  With it off a step slot enqueues exactly the launches it does without this feature; on, every step slot
 *    ends with one more launch (k_tracers, behind the other samplers; it skips itself on the steps gated out) that is captured
 *    in the replayed graphs; enable / disable re-capture them.  Independent of the other samplers.  Cost: one pass over the
 *    ids of the population per sampled step (there is no map from id to slot on the device).
 *  Errors: SPHX:Tracers:config (NULL config or ids, n_tracers outside 1 .. n_fluid, a duplicate id, an id out of range, a
 *    wall row, every < 1, capacity < 1 or capacity * n_tracers * 4 > 1 << 27, non-finite t_from, or the allocation fails:
 *    the context then goes on without tracers), SPHX:Tracers:disabled (SPHX_ERR_STATE: a call that needs the tracers while
 *    they are off), SPHX:Tracers:capacity (the caller's arrays are smaller than n_records); every call on a slab context
 *    fails with SPHX_ERR_ARG, SPHX:Tracers:slab (the tracers of a ring: sphx_slab_tracers_*, section 3a).  A refused enable leaves running tracers, and their records, untouched.
 * ---------------------------------------------------------------------------------------------- */

#define SPHX_TRACER_FIELDS 4

typedef struct sphx_tracers_config {
    int32_t n_tracers;   /* T, 1 .. n_fluid                                                        */
    int32_t every;       /* record every `every`-th completed step (step count % every == 0), >= 1 */
    int32_t capacity;    /* records the device buffer holds, >= 1                                  */
    double t_from;       /* only steps ending at t >= t_from                                       */
    const int32_t *ids;  /* [n_tracers] fluid rows of the caller's order, 0-based; copied at enable */
} sphx_tracers_config;

/* (Re)configure and empty the buffer; waits for the stream.  Off by default. */
int sphx_ctx_tracers_enable(sphx_ctx *ctx, const sphx_tracers_config *cfg);
/* Stop recording (no-op when off); the records are dropped. */
int sphx_ctx_tracers_disable(sphx_ctx *ctx);
/* Append one record of the current state (what sphx_ctx_download would return) now, without gating. */
int sphx_ctx_tracers_sample(sphx_ctx *ctx);
/* The records so far, in step order: times [capacity][2] and values [capacity][n_tracers][SPHX_TRACER_FIELDS], row-major
 * (times / values NULL: that array is not copied; both NULL: only the counts are reported and capacity is not checked);
 * ids [n_tracers]: the list as given at enable (NULL: not copied).  Waits for and settles everything enqueued, like
 * sphx_ctx_download.  drain != 0: the buffer is emptied and n_dropped and n_missing zeroed after copying. */
int sphx_ctx_tracers_read(sphx_ctx *ctx, int capacity, double *times, double *values, int32_t *ids, int *n_tracers,
                          int *n_records, int64_t *n_dropped, int64_t *n_missing, int drain);

/* ------------------------------------------------------------------------------------------------
 * 2q. Particle tracers of a batch (section 2b): the tracers of section 2p for every member at once.
 *
 *  One config and one id list for all members (they share a geometry, hence the row numbering); `capacity` is per member.
 *  Every member has its own record buffer, n_records, n_dropped and n_missing, and is recorded on its own clock with the
 *  gating of section 2p, so a member that sits out slots records nothing in them and its counters are not touched.  A
 *  member's records are bit for bit those of a standalone context with the same parameters and config that took the same
 *  steps: the layout decides which thread copies a particle, not what is copied.  After a realignment (section 2b) a member's
 *  state itself differs from a standalone context's within floating-point rounding, and its records are that state's: what
 *  sphx_batch_download returns in the tracked rows, bit for bit.  With tracers on, every step slot of the batch ends with one recording launch for all members (k_tracers_b, behind the batch's
 *  other samplers); off, a slot enqueues exactly the launches it does without this feature.
 *  Memory: n_members * capacity * (2 + n_tracers * 4) doubles; n_members * capacity * n_tracers * 4 must not exceed
 *  1 << 27 doubles.  A refused enable leaves running tracers, and their records, untouched.
 *  Errors: SPHX:Batch:null (NULL batch), SPHX:Tracers:config (as in section 2p, with the total over the members),
 *  SPHX:Tracers:disabled, SPHX:Tracers:capacity (the caller's capacity is below the largest n_records of any member).
 * ---------------------------------------------------------------------------------------------- */

/* (Re)configure and empty every member's buffer; waits for the stream. */
int sphx_batch_tracers_enable(sphx_batch *batch, const sphx_tracers_config *cfg);
/* Stop recording (no-op when off); the records are dropped. */
int sphx_batch_tracers_disable(sphx_batch *batch);
/* settles; appends a record of what sphx_batch_download returns, every member, without gating */
int sphx_batch_tracers_sample(sphx_batch *batch);
/* One call for all members.  times is [n_members][capacity][2] and values [n_members][capacity][n_tracers][SPHX_TRACER_FIELDS],
 * row-major: member m's block lies behind member m - 1's, its records fill rows 0 .. n_records[m] - 1 and the other rows are
 * left as they are.  ids is [n_tracers]; n_records, n_dropped and n_missing are [n_members]; any pointer may be NULL.
 * Settles first, as sphx_batch_download does.  drain != 0: every member's buffer is emptied and its counters zeroed after
 * copying. */
int sphx_batch_tracers_read(sphx_batch *batch, int capacity, double *times, double *values, int32_t *ids, int *n_tracers,
                            int *n_records, int64_t *n_dropped, int64_t *n_missing, int drain);

/* ------------------------------------------------------------------------------------------------
 * 2r. Density statistics: the density the next step starts from, re-summed at every fluid particle and binned on the
 *     device, inside the step loop: the relative deviation delta = rho / rho0 - 1 the weakly compressible method keeps
 *     small, its profile across the channel and next to the walls, the pressure p0 delta (flat in y in plane Poiseuille
 *     flow) and the packing sum m / rho.  Section 2n's div v is the rate of compression; this is its state.  The solver's own
 *     rho is an output field in the layout of the step that wrote it; this is computed from what sphx_ctx_download returns.
 *
 *  One sample: for every fluid particle i with 0 <= y_i <= DH (outside: dropped, as in section 2a), over every other fluid
 *    particle j with 1e-24 < r2 < (2h)^2 (nearest image in x) and every wall particle in the same range -- the walls are
 *    always in, this is the solver's density:
 *        s_in  = W(0) + sum over the fluid partners of W(r_ij)          W the cubic spline
 *        s_ct  = sum over the wall partners of W(r_ij) V_j              V_j the wall particle's volume
 *        rho_i = s_in rho0 inv_sigma0 + s_ct rho0^2 inv_sigma0 / mass_i   (rho0 where that is <= 1e-12: the step's floor)
 *        delta_i = rho_i / rho0 - 1      wall_i = s_ct rho0 inv_sigma0 / mass_i      dvol_i = rho0 / rho_i - 1
 *    rho_i is the density the next step's first pass computes for the same state.
 *  Outliers: a particle with |delta_i| > delta_bound, or a delta_i that is not finite, is counted in `outliers` and summed
 *    nowhere, in no histogram.  This is not an error.
 *  Bins and bands: those of section 2a.  Per bin and band count + outliers equals the flow statistics' count.
 *  Sums, per bin and band, over all samples, SPHX_DENS_STATS_FIELDS = 8 doubles in this order: count, sum delta, sum delta^2,
 *    sum dvol, sum wall, outliers, d_min, d_max -- the last two the running extremes of delta over every particle summed so
 *    far, +inf / -inf before the first.  count and outliers are integers held in doubles.
 *  Histogram, per band, over all samples: n_hist uniform bins on [-hist_range, hist_range), the particle in bin
 *    floor((delta + hist_range) * n_hist / (2 hist_range)); `below` and `above` count the particles outside the range.  Per
 *    band sum(hist) + below + above equals sum(count).  A delta within rounding of an edge may fall either side.
 *  Per sampler: n_samples, t_first, t_last.
 *  Exactness: a sample is summed in int64 fixed point at power-of-two scales picked from the particle count (n <= 2^L) and
 *    delta_bound (2^e >= delta_bound): delta in units of 2^-(62-L-e), delta^2 of 2^-(62-L-2e), dvol of 2^-(61-L-e), wall of
 *    2^-(61-L); the extremes go through order-preserving integer keys.  The sums are bit-identical between runs and
 *    independent of the workgroups' dispatch order, and a batch member's are a standalone context's.  They depend on the order
 *    of the particle slots within the floating-point rounding of s_in and s_ct only.
 *  Limits: 1 <= n_hist <= 1024, 0 < delta_bound <= 0.5, 0 < hist_range <= delta_bound, and
 *    (n_bands + 1) * (8 * n_bins + n_hist + 2) <= 7680, the 60 KB of LDS of a workgroup.
 *  Gating: as in section 2l.  sphx_ctx_dens_stats_sample adds a sample of the state now, without gating.
 *  Off by default.  With it off a step slot enqueues exactly the launches it does without this feature; on, every step slot
 *    ends with one more launch (k_dens_stats, the last of the slot; it skips itself on the steps gated out) that is captured
 *    in the replayed graphs; enable / disable re-capture them.  Independent of the other eight samplers.
 *  Errors: SPHX:DensStats:config (NULL config, a value outside the limits above, n_bins < 0, every < 1, a NaN t_from, n_bands
 *    outside 0..2, a band centre or half-width that is not finite or a negative half-width, or the allocation fails: the
 *    context then goes on without density statistics), SPHX:DensStats:band, SPHX:DensStats:capacity (sums given and capacity <
 *    n_bins, or hist given and hist_capacity < n_hist), SPHX:DensStats:disabled (SPHX_ERR_STATE: a call that needs the sampler
 *    while it is off); every call on a slab context fails with SPHX_ERR_ARG, SPHX:DensStats:slab (the density statistics of a
 *    ring: sphx_slab_dstats_*, section 3a).  A refused enable leaves a running sampler, and its sums, untouched.
 * ---------------------------------------------------------------------------------------------- */

#define SPHX_DENS_STATS_FIELDS 8
#define SPHX_DENS_STATS_MAX_HIST 1024

typedef struct sphx_dens_stats_config {
    int32_t n_bins;            /* y-bins over [0, DH]; 0 = the reference's profile bins                  */
    int32_t every;             /* sample every `every`-th completed step (step count % every == 0), >= 1 */
    double t_from;             /* only steps ending at t >= t_from                                       */
    int32_t n_hist;            /* histogram bins on [-hist_range, hist_range), 1..1024 (64 is a good default) */
    int32_t n_bands;           /* 0..2 x-bands besides the whole channel                                 */
    double hist_range;         /* 0 < hist_range <= delta_bound (0.05 is a good default)                 */
    double delta_bound;        /* a particle with |delta| > delta_bound is an outlier; 0 < delta_bound <= 0.5 */
    double band_x[2], band_hw[2];
} sphx_dens_stats_config;

/* (Re)configure and zero the sums; waits for the stream.  Off by default. */
int sphx_ctx_dens_stats_enable(sphx_ctx *ctx, const sphx_dens_stats_config *cfg);
/* Stop sampling (no-op when off); the sums are dropped. */
int sphx_ctx_dens_stats_disable(sphx_ctx *ctx);
/* Zero the sums, the extremes, the histogram and the sample count; the configuration stays. */
int sphx_ctx_dens_stats_reset(sphx_ctx *ctx);
/* Add one sample of the current state (what sphx_ctx_download would return) now, without gating. */
int sphx_ctx_dens_stats_sample(sphx_ctx *ctx);
/* One band so far: sums is [SPHX_DENS_STATS_FIELDS][capacity] (field f of bin k at f * capacity + k; capacity >= n_bins where
 * it is given), hist is [hist_capacity] (hist_capacity >= n_hist where it is given), below and above one number each; every
 * pointer may be NULL.  Waits for and settles everything enqueued, like sphx_ctx_download.  t_first / t_last are NaN before
 * a sample. */
int sphx_ctx_dens_stats_read(sphx_ctx *ctx, int band, int capacity, int hist_capacity, int *n_bins, int *n_hist, double *sums,
                             int64_t *hist, int64_t *below, int64_t *above, int64_t *n_samples, double *t_first, double *t_last);

/* ------------------------------------------------------------------------------------------------
 * 2s. Density statistics of a batch (section 2b): the sums of section 2r for every member at once.
 *
 *  One config for all members (bins, bands, histogram and the walls come from the shared geometry).  Every member has its
 *  own sums, extremes and histogram and its own head and is sampled on its own clock, with its own rho0, with the gating of
 *  section 2r, so a member that sits out slots is not sampled in them.  A member's sums are, bit for bit, those of a
 *  standalone context with the same parameters and config that took the same steps in the same slot order; a realignment
 *  reorders a member's slots, after which its sums agree within floating-point rounding.  With the sampler on, every step
 *  slot of the batch ends with one launch for all members (k_dens_stats_b, behind the batch's other samplers); off, a slot
 *  enqueues exactly the launches it does without this feature.  A refused enable leaves a running sampler untouched.
 *  Errors: SPHX:Batch:null (NULL batch), SPHX:Batch:member (the read's member outside 0 .. n_members - 1) and those of
 *  section 2r.
 * ---------------------------------------------------------------------------------------------- */

int sphx_batch_dens_stats_enable(sphx_batch *batch, const sphx_dens_stats_config *cfg);
int sphx_batch_dens_stats_disable(sphx_batch *batch);
int sphx_batch_dens_stats_reset(sphx_batch *batch);
/* settles; adds a sample of what sphx_batch_download returns, every member, without gating */
int sphx_batch_dens_stats_sample(sphx_batch *batch);
/* Section 2r's read of one member.  Settles first, as sphx_batch_download does. */
int sphx_batch_dens_stats_read(sphx_batch *batch, int member, int band, int capacity, int hist_capacity, int *n_bins, int *n_hist,
                               double *sums, int64_t *hist, int64_t *below, int64_t *above, int64_t *n_samples, double *t_first,
                               double *t_last);

/* ------------------------------------------------------------------------------------------------
 * 2t. Mode amplitudes: the flow projected on the channel's own modes at every sampled step, recorded on the device, inside
 *     the step loop.  The other samplers describe the flow in y-bins, at nodes, at points, per particle and per pair; this
 *     one says which LENGTH SCALES carry a signal.  The channel is periodic in x and has walls in y, so its acoustic
 *     eigenmodes and the eigenfunctions of its viscous start-up are products of exp(i 2 pi m x / DL) with cos(n pi y / DH)
 *     or sin(n pi y / DH): the sine coefficients of u_x are the terms of the start-up series (profile.poiseuille_startup),
 *     the amplitudes of the count are the structure factor.
 *
 *  One sample: with thx = 2 pi x_i / DL and thy = pi y_i / DH of fluid particle i, for every mode 0 <= m <= mx,
 *    0 <= n <= ny, every field f -- n (q = 1), ux (q = u_x), uy (q = u_y) -- and every basis k -- cc = cos(m thx) cos(n thy),
 *    sc = sin cos, cs = cos sin, ss = sin sin -- the sum S[m][n][f][k] = sum_i q_i * basis_k(i) over ALL fluid particles,
 *    unweighted (the fluid masses are equal: mass * n is the density mode); walls are never in.  Only pos / vel are sampled.
 *  Records: one per sampled step: `step` and `t` in times[capacity][2] and the sample in
 *    records[capacity][mx + 1][ny + 1][SPHX_MODE_FIELDS][SPHX_MODE_BASES], filled in step order; a full buffer drops and
 *    counts further records in n_dropped, it does not wrap (the semantics of section 2j).  mx, ny <= 16.  Cap:
 *    capacity * (mx + 1) * (ny + 1) * 12 <= 1 << 27 doubles (1 GiB), over all members of a batch.
 *  Gating: as in section 2j.  sphx_ctx_modes_sample appends a record of the state now, without gating.
 *  Determinism: every term q_i * basis_k(i) is rounded once to int64 fixed point and depends on particle i alone, and the
 *    integers are added exactly: a record is bit-identical whatever the particle order, layout, lanes per particle,
 *    re-binning phase or workgroup count.  m = 0 and n = 0 are exact: S[0][0][n][cc] is the particle count and every sine sum
 *    of a zero mode is 0.  A velocity above the bound of section 2a (a non-finite state) makes a later read fail with
 *    SPHX:Modes:range.
 *  Off by default.  With it off a step slot enqueues exactly the launches it does without this feature; on, every step slot
 *    ends with one more launch (k_modes, behind the other samplers; it skips itself on the steps gated out) that is captured
 *    in the replayed graphs; enable / disable re-capture them.  Independent of the other samplers.
 *  Errors: SPHX:Modes:config (NULL config, mx or ny outside 0..16, every < 1, capacity < 1, a NaN t_from, the cap on the
 *    record buffer, or the allocation fails: the context then goes on without the sampler), SPHX:Modes:disabled
 *    (SPHX_ERR_STATE), SPHX:Modes:range (SPHX_ERR_STATE), SPHX:Modes:capacity (the caller's arrays are smaller than
 *    n_records); every call on a slab context fails with SPHX_ERR_ARG, SPHX:Modes:slab.  A refused enable leaves a running
 *    sampler, and its records, untouched.
 * ---------------------------------------------------------------------------------------------- */

#define SPHX_MODE_FIELDS 3 /* n, ux, uy */
#define SPHX_MODE_BASES 4  /* cc, sc, cs, ss */
#define SPHX_MODES_MAX 16

typedef struct sphx_modes_config {
    int32_t mx, ny;            /* modes 0 .. mx in x and 0 .. ny in y, each 0 .. 16                      */
    int32_t every;             /* record every `every`-th completed step (step count % every == 0), >= 1 */
    int32_t capacity;          /* records the device buffer holds, >= 1                                  */
    double t_from;             /* only steps ending at t >= t_from                                       */
} sphx_modes_config;

/* (Re)configure and empty the buffer; waits for the stream.  Off by default. */
int sphx_ctx_modes_enable(sphx_ctx *ctx, const sphx_modes_config *cfg);
/* Stop recording (no-op when off); the records are dropped. */
int sphx_ctx_modes_disable(sphx_ctx *ctx);
/* Append one record of the current state (what sphx_ctx_download would return) now, without gating. */
int sphx_ctx_modes_sample(sphx_ctx *ctx);
/* The records so far, in step order: times [capacity][2] and records [capacity][*mx + 1][*ny + 1][3][4], row-major (times /
 * records NULL: that array is not copied; both NULL: only the shape and the counts are reported and capacity is not
 * checked).  Waits for and settles everything enqueued, like sphx_ctx_download.  drain != 0: the buffer is emptied and
 * n_dropped zeroed after copying. */
int sphx_ctx_modes_read(sphx_ctx *ctx, int capacity, double *times, double *records, int *mx, int *ny, int *n_records,
                        int64_t *n_dropped, int drain);

/* ------------------------------------------------------------------------------------------------
 * 2u. Mode amplitudes of a batch (section 2b): the records of section 2t for every member at once.
 *
 *  One config for all members; `capacity` is per member.  Every member has its own record buffer, n_records, n_dropped and
 *  range flag, and is recorded on its own clock with the gating of section 2t, so a member that sits out slots records
 *  nothing in them and its counters are not touched.  A member's records are bit for bit those of a standalone context
 *  with the same parameters and config that took the same steps.  With the sampler on, every step slot of the batch ends
 *  with one recording launch for all members (k_modes_b, behind the batch's other samplers); off, a slot enqueues exactly the
 *  launches it does without this feature.  n_members * capacity * (mx + 1) * (ny + 1) * 12 must not exceed 1 << 27 doubles.
 *  Errors: SPHX:Batch:null (NULL batch), SPHX:Modes:config (as in section 2t, with the total over the members),
 *  SPHX:Modes:disabled, SPHX:Modes:capacity (the caller's capacity is below the largest n_records of any member);
 *  SPHX:Modes:range names the member whose flag is set.
 * ---------------------------------------------------------------------------------------------- */

int sphx_batch_modes_enable(sphx_batch *batch, const sphx_modes_config *cfg);
int sphx_batch_modes_disable(sphx_batch *batch);
/* settles; appends a record of what sphx_batch_download returns, every member, without gating */
int sphx_batch_modes_sample(sphx_batch *batch);
/* One call for all members.  times is [n_members][capacity][2] and records [n_members][capacity][*mx + 1][*ny + 1][3][4],
 * row-major: member m's block lies behind member m - 1's, its records fill rows 0 .. n_records[m] - 1 and the other rows are
 * left as they are.  n_records and n_dropped are [n_members]; any pointer may be NULL.  Settles first, as
 * sphx_batch_download does.  drain != 0: every member's buffer is emptied and its n_dropped zeroed after copying. */
int sphx_batch_modes_read(sphx_batch *batch, int capacity, double *times, double *records, int *mx, int *ny, int *n_records,
                          int64_t *n_dropped, int drain);

/* ------------------------------------------------------------------------------------------------
 * 3. x-slab contexts (multi-GPU). The channel is cut into n_ranks slabs of whole cell columns; each
 *    rank (one process per GPU) holds its columns plus halo_cols columns of copies on either side.
 *    The reference has no counterpart (single process).  One step is
 *        sphx_slab_compute -> {exchange two messages with the ring neighbours, all-reduce max|v|}
 *        -> sphx_slab_finish
 *    either driven by the caller with its own transport (the three calls below) or by the library's native loop
 *    over RCCL (sphx_slab_run).
 *    All *_dev pointers are DEVICE pointers (e.g. torch tensors) and every call is asynchronous on the
 *    context's stream (hip_stream of sphx_slab_create, or an internal one when NULL).
 * ---------------------------------------------------------------------------------------------- */

/* Create rank `rank` of `n_ranks` from the GLOBAL host state (same arguments as sphx_ctx_create on
 * every rank).  halo_cols >= 4.  prm->rebuild_every selects the protocol: 1 = the slab re-bins every step and is
 * driven by the caller (sphx_slab_local_vmax / _prepare / _compute / _finish below, any transport); any other value
 * (0 = auto: 5) = skinned slab for the library's own loops only (sphx_slab_run over RCCL, sphx_slab_group_run): it
 * re-bins every K-th step or when the device sees the drift bound hit, and the four caller-driven calls refuse it
 * with SPHX:Slab:protocol. */
int sphx_slab_create(sphx_ctx **ctx, const sphx_params *prm, int n_fluid, int n_total,
                     const double *pos, const double *vel, const double *drho_dt, const double *mass,
                     const double *wall_vel, double t0, int64_t step0, int rank, int n_ranks,
                     int halo_cols, void *hip_stream);
/* Message length in doubles (1 + 7*capacity: count, then x,y,vx,vy,drho,mass,id blocks), the owned
 * global cell columns [col0,col1), current local particle count and array capacity. */
int sphx_slab_layout(sphx_ctx *ctx, int64_t *msg_doubles, int *col0, int *col1, int *n_local,
                     int *capacity);
/* max |v| over the owned particles of the current state -> vmax_dev[0]. */
int sphx_slab_local_vmax(sphx_ctx *ctx, double *vmax_dev);
/* Arm the device clock for a run to t_target / at most max_steps (<=0: unlimited) steps; the first dt
 * uses vmax_global_dev[0] (the all-reduced value). */
int sphx_slab_prepare(sphx_ctx *ctx, double t_target, int64_t max_steps, const double *vmax_global_dev);
/* First half of a step: the four neighbour passes, local max |v| -> vmax_local_dev[0], and the two
 * outgoing messages (left / right ring neighbour). */
int sphx_slab_compute(sphx_ctx *ctx, double *send_left_dev, double *send_right_dev,
                      double *vmax_local_dev);
/* Second half: take the messages received from the left / right neighbour and the global max |v|,
 * update the clock and rebuild the cell grid. */
int sphx_slab_finish(sphx_ctx *ctx, const double *recv_left_dev, const double *recv_right_dev,
                     const double *vmax_global_dev);
/* Native step loop.  sphx_slab_run enqueues n_steps whole steps (compute -> two sends + two receives with the ring
 * neighbours and an 8-byte max all-reduce through RCCL -> finish) on the context's stream, in library-owned message
 * buffers; nothing of the host language runs between steps.  One context per process (one process per GPU): rank 0
 * makes an id with sphx_comm_unique_id (128 bytes), the launcher carries it to the other ranks (torch.distributed
 * broadcast, MPI, a file ...), every rank joins with sphx_slab_comm_init.  librccl is loaded at that moment.
 * sphx_slab_group_run: all slabs of the ring in ONE process on one device -- the same loop with device-to-device
 * copies as the transport (tests and rehearsals on a one-GPU box).  Both return without waiting; sphx_slab_sync
 * waits and reports. */
/* SPHX_OK when librccl can be loaded with every entry point the native loop needs (purely local, no communication):
 * a launcher lets all ranks agree on this BEFORE anyone enters the collective sphx_slab_comm_init. */
int sphx_comm_available(void);
int sphx_comm_unique_id(void *id_bytes, int capacity);
/* Diagnostic: runs the exchange pattern of sphx_slab_run (grouped sends / receives, the all-reduce) on a one-rank
 * communicator on the current device and checks what comes back.  SPHX_OK, or an error naming the RCCL call that failed. */
int sphx_comm_selftest(void);
/* The same calls captured into a hipGraph and replayed (one-rank communicator): can this RCCL be captured?  What
 * sphx_slab_graph_prepare relies on. */
int sphx_comm_selftest_graph(void);
int sphx_slab_comm_init(sphx_ctx *ctx, const void *id_bytes);
int sphx_slab_comm_destroy(sphx_ctx *ctx);
int sphx_slab_run(sphx_ctx *ctx, double t_target, int64_t n_steps);
int sphx_slab_group_run(sphx_ctx **ctxs, int n_ranks, double t_target, int64_t n_steps);
/* Capture ten whole steps of the native loop -- kernels and the RCCL calls (n_ranks = 1: the context of this process's
 * rank) or the copies and cross-stream dependencies of an in-process ring (n_ranks >= 2) -- into one hipGraph; the two
 * loops above then replay it for every full batch of ten steps.  Call after the loop has run at least two steps, on
 * every rank at the same point (the graph is warmed with one idle replay, which communicates).  Skinned slabs only. */
int sphx_slab_graph_prepare(sphx_ctx **ctxs, int n_ranks);
/* Wait for the stream; fails if a step was enqueued after the loop had stopped or a buffer overflowed. */
int sphx_slab_sync(sphx_ctx *ctx, sphx_status *status);
/* Host copy of the slab's current particles (owned + halo copies); owned[i] = 1 for owned ones. */
int sphx_slab_snapshot(sphx_ctx *ctx, int capacity, int *n, double *x, double *y, double *vx,
                       double *vy, double *drho, int *id, int *owned);

/* ------------------------------------------------------------------------------------------------
 * 3a. Samplers of a slab ring: the flow statistics of section 2a, the step history of section 2d, the velocity-field
 *    map of section 2e, the point probes of section 2h, the profile series of section 2j, the pair statistics of
 *    section 2l, the gradient statistics of section 2n, the particle tracers of section 2p and the density statistics of
 *    section 2r (the last six described with their calls, at the end) for the slabs of the library's own loops (sphx_slab_run, sphx_slab_group_run), so that
 *    a ring reports its time-averaged profile, the settling of its wall shear, its averaged field and its profile at every
 *    sampled step without a snapshot per sample.  The config structs, their checks, the layouts and the SPHX:Stats:* / SPHX:History:* / SPHX:Field:*
 *    identifiers are those of sections 2a / 2d / 2e; sphx_ctx_flow_stats_*,
 *    sphx_ctx_history_* and sphx_ctx_field_map_* keep refusing a slab (SPHX:Stats:slab, SPHX:History:slab,
 *    SPHX:Field:slab).
 *    Statistics and history: a slab samples, at the end of a step, the fluid particles it OWNS (those sphx_slab_snapshot
 *    marks owned), never its halo copies, and what a read returns are the slab's PARTIAL sums: the ring's value is the
 *    sum over the ranks.
 *      flow statistics: every array elementwise, count included; n_samples, t_first and t_last are the same on every
 *        rank.  Band membership goes by x mod DL, whatever frame a slab keeps x in.  The sums are exact integers per
 *        sample, so the pooled sums do not depend on how the channel is cut.
 *      history: fields 0..3 of a record (step, t, dt, vmax) come from the clock and are the same on every rank;
 *        fields 4..7 are additive: tau_bottom / tau_top = -(the slab's wall-force sum) / DL, kinetic_energy = the
 *        slab's sum, u_bulk = (the slab's sum of u_x) / the GLOBAL n_fluid.  The ring's record is fields 0..3 of any
 *        rank and the sum over the ranks of fields 4..7.  capacity and n_dropped are per slab; every slab records
 *        the same steps.
 *    Field map: a node's sample is a ratio (S1 / S0 and its square are accumulated per sample), so partial sums over
 *    owned particles could not be pooled.  The NODES are divided instead: of the nx x ny grid of section 2e (linspace
 *    over [0, DL] and [0, DH], ends included) a slab owns the node columns i_lo <= i < i_hi, all ny rows of each, and
 *    computes the COMPLETE sample of each of its nodes from the particles it owns and from its halo copies, which
 *    carry the finished step's state in the cell columns next to the owned ones.  The blocks of ranks 0 .. G-1
 *    partition [0, nx): they are computed once, at enable, by one rule that is the same on every rank -- rank r's
 *    block starts at the first node column whose x is not left of the left edge of rank r's first cell column, rank
 *    0's at 0, and rank r's i_hi is rank r+1's i_lo -- so a node column that falls on a cut belongs to exactly one
 *    slab.  Node column nx-1 (x = DL) is the last slab's and is evaluated at x = DL in that slab's frame, whose right
 *    halo holds the first slab's particles at x + DL.  The ring's map is the slabs' blocks side by side; nothing is
 *    added.  A slab may own no node column (i_lo == i_hi, a coarse nx): it still counts the samples, so n_samples,
 *    t_first and t_last are the same on every rank.  The device allocation is the block, not the grid; nx * ny is
 *    bounded as in section 2e.
 *    Every call refuses a context that is not a slab with SPHX:Slab:ctx and a slab created for the caller-driven
 *    protocol (rebuild_every == 1) with SPHX:Slab:protocol.  A read, reset or disable waits for the slab's stream(s)
 *    itself, whether sphx_slab_sync has been called for the enqueued steps or not.  Enabling or disabling a sampler
 *    drops a step graph prepared with sphx_slab_graph_prepare (on any slab of an in-process ring: the ring's): the
 *    loops run eagerly until it is prepared again, and the new graph carries the launches.  There is no "sample now"
 *    call on slabs.
 * ---------------------------------------------------------------------------------------------- */
int sphx_slab_flow_stats_enable(sphx_ctx *ctx, const sphx_flow_stats_config *cfg);
int sphx_slab_flow_stats_disable(sphx_ctx *ctx);
/* Clears the sums and the sample count (SPHX:Stats:disabled while the sampler is off, as for the read). */
int sphx_slab_flow_stats_reset(sphx_ctx *ctx);
/* The slab's partial sums of one band; arguments as sphx_ctx_flow_stats_read. */
int sphx_slab_flow_stats_read(sphx_ctx *ctx, int band, int capacity, int *n_bins, double *count, double *sum_ux,
                              double *sum_ux2, double *sum_uy, double *sum_uy2, int64_t *n_samples, double *t_first,
                              double *t_last);
int sphx_slab_history_enable(sphx_ctx *ctx, const sphx_history_config *cfg);
int sphx_slab_history_disable(sphx_ctx *ctx);
/* The slab's records (fields 4..7: its partials); arguments as sphx_ctx_history_read (SPHX:History:disabled while off). */
int sphx_slab_history_read(sphx_ctx *ctx, int capacity, double *records, int *n_records, int64_t *n_dropped, int drain);
/* Config and checks as sphx_ctx_field_map_enable (SPHX:Field:config); nx, ny are the RING's grid, the same on every rank. */
int sphx_slab_field_map_enable(sphx_ctx *ctx, const sphx_field_map_config *cfg);
int sphx_slab_field_map_disable(sphx_ctx *ctx);
/* Clears the planes and the sample count (SPHX:Field:disabled while the map is off, as for the read). */
int sphx_slab_field_map_reset(sphx_ctx *ctx);
/* The slab's block: the ring's shape (*nx, *ny), the node columns *i_lo <= i < *i_hi it owns, the six planes of
 * (*i_hi - *i_lo) * ny doubles each -- node (i, k) at (i - *i_lo) * ny + k -- and the head, as sphx_ctx_field_map_read.
 * Any output may be NULL; capacity: the doubles each plane given can take, SPHX:Field:capacity when that is less than
 * the block (call once with every plane NULL to learn the block, then with arrays of its size). */
int sphx_slab_field_map_read(sphx_ctx *ctx, int capacity, int *nx, int *ny, int *i_lo, int *i_hi, double *count,
                             double *sum_w, double *sum_ux, double *sum_uy, double *sum_ux2, double *sum_uy2,
                             int64_t *n_samples, double *t_first, double *t_last);
/* Point probes of a ring (the probes of section 2h; k_point_probes_s).  A probe's sample is a ratio and a density, so, like
 * the map's nodes, the POINTS are divided among the slabs: cfg holds the RING's whole list, the same on every rank, and a
 * slab owns the points with edge(r) <= x < edge(r + 1), x as folded into [0, DL) and
 * edge(r) = ((r * ncx) / n_ranks) * (DL / ncx) the left edge of rank r's first cell column (ncx: the ring's cell columns);
 * rank 0 owns from 0 and the last rank up to DL.  Every point has exactly one owner -- a point on a cut belongs to the slab
 * right of it, two equal points to the same slab -- computed once, at enable, by the same arithmetic on every rank.  A slab
 * records the COMPLETE sample of each probe it owns (weight, u_x, u_y and rho: the masses of its halo copies enter rho) from
 * the particles it owns and from its halo copies, in its own buffer of `capacity` records with its own n_records and
 * n_dropped.  A slab that owns no probe still records {step, t} and counts, so every slab's series has the same length and
 * the same steps.  The ring's series is the slabs' columns put back in the list's order (`index`); nothing is added.
 * Gating, values, determinism and the SPHX:Probe:config checks are those of section 2h (the bound on
 * capacity * n_points * 4 is taken with the ring's n_points).  A refused enable leaves running probes, their records and a
 * prepared graph as they are.  SPHX:Probe:disabled: a read while the probes are off.  sphx_ctx_probes_* keep refusing a
 * slab (SPHX:Probe:slab). */
int sphx_slab_probes_enable(sphx_ctx *ctx, const sphx_probes_config *cfg);
int sphx_slab_probes_disable(sphx_ctx *ctx);
/* The slab's records: times [capacity][2] and values [capacity][*n_owned][SPHX_PROBE_FIELDS], row-major, as
 * sphx_ctx_probes_read; index [*n_owned]: the positions of the owned probes in the ring's list of *n_points_ring points,
 * ascending.  Any output may be NULL.  capacity = 0: only the sizes and counts are reported, nothing is copied or drained
 * (call once so to learn n_owned and n_records, then with arrays of that size); SPHX:Probe:capacity when an array is given
 * and capacity is below n_records.  drain != 0: the buffer is emptied and n_dropped zeroed after copying. */
int sphx_slab_probes_read(sphx_ctx *ctx, int capacity, double *times, double *values, int *index, int *n_points_ring,
                          int *n_owned, int *n_records, int64_t *n_dropped, int drain);
/* Profile series of a ring (the series of section 2j; k_profile_series_s).  The names say pseries: no function of this
 * header has both "slab" and "profile_series" in its name.  The config, its checks, the record layout, capacity and drops,
 * drain, the gating and the SPHX:ProfileSeries:* identifiers are those of section 2j.  Like the flow statistics, a slab
 * bins, at the end of a sampled step, the fluid particles it OWNS, never its halo copies, and a slab's record is the PARTIAL
 * sample over them: the ring's record is the element-wise sum over the ranks of all five fields, count included -- exact
 * integers per slab, each converted once, so the ring's record does not depend on how the channel is cut, and per slab the
 * records added in order are that slab's flow-statistics sums (same config) to the bit.  Band membership goes by x mod DL,
 * whatever frame a slab keeps x in.  Every slab has its own buffer of `capacity` records with its own n_records and
 * n_dropped; `step` and `t` come from the clock, so step, t, n_records and n_dropped are the same on every rank, and a slab
 * that owns nothing in a band (or nothing at all) still stores that band's zeros and counts the record.  A refused enable
 * leaves a running series, its records and a prepared graph as they are.  SPHX:ProfileSeries:disabled: a read while the
 * series is off; disable is a no-op then.  There is no "sample now" call.  sphx_ctx_profile_series_* keep refusing a slab
 * (SPHX:ProfileSeries:slab). */
int sphx_slab_pseries_enable(sphx_ctx *ctx, const sphx_profile_series_config *cfg);
int sphx_slab_pseries_disable(sphx_ctx *ctx);
/* The slab's records (its partial samples); arguments as sphx_ctx_profile_series_read: both arrays NULL reports only the
 * shape and the counts. */
int sphx_slab_pseries_read(sphx_ctx *ctx, int capacity, double *times, double *records, int *n_bins, int *n_bands,
                           int *n_records, int64_t *n_dropped, int drain);
/* Pair statistics of a ring (the sampler of section 2l; k_pair_dist_s).  The names say pairs: no function of this header has
 * both "slab" and "pair_dist" in its name.  The config, its checks and limits, the bins, the gating and the SPHX:PairDist:*
 * identifiers are those of section 2l.  A sample is a sum over centres, so it is divided like the flow statistics': a slab
 * counts, at the end of a sampled step, the pairs whose CENTRE it owns (a fluid particle sphx_slab_snapshot marks owned, with
 * y_margin <= y <= DH - y_margin), and what a read returns are the slab's PARTIAL sums -- the ring's ff, fw and centres are
 * the element-wise sums over the ranks, its r2_min the minimum over the ranks; n_samples, t_first and t_last come from the
 * clock and are the same on every rank, also on a slab that owns no centre of a band.  The PARTNERS of a centre are all the
 * other fluid particles the slab holds, its halo copies included -- they carry the finished step's positions in the cell
 * columns next to the owned ones, up to the summation order of their own neighbour lists, a few ulps of x -- and, with
 * with_walls, the wall particles the slab holds.  The slab's window is open: the first slab holds the last slab's particles
 * at x - DL and the last slab the first slab's at x + DL, so a pair across the periodic seam is counted with its plain dx and
 * no minimum image; a ring is at least 20h long, so no copy is a centre's own image within r_max <= 2h.  Band membership
 * goes by x mod DL, whatever frame a slab keeps x in.  Integers and a minimum: the ring's sums do not depend on how the
 * channel is cut, and where no pair lies within a rounding of a bin edge they are a single context's count for count.  A
 * refused enable leaves a running sampler, its sums and a prepared graph as they are.  SPHX:PairDist:disabled: a reset or a
 * read while the sampler is off; disable is a no-op then.  There is no "sample now" call.  sphx_ctx_pair_dist_* keep refusing
 * a slab (SPHX:PairDist:slab). */
int sphx_slab_pairs_enable(sphx_ctx *ctx, const sphx_pair_dist_config *cfg);
int sphx_slab_pairs_disable(sphx_ctx *ctx);
/* Clears the sums and the sample count; the configuration stays. */
int sphx_slab_pairs_reset(sphx_ctx *ctx);
/* The slab's partial sums of one band; arguments as sphx_ctx_pair_dist_read. */
int sphx_slab_pairs_read(sphx_ctx *ctx, int band, int capacity, int *n_bins, int64_t *ff, int64_t *fw, int64_t *centres,
                         double *r2_min, int64_t *n_samples, double *t_first, double *t_last);
/* Gradient statistics of a ring (the sampler of section 2n; k_grad_stats_s).  The names say gstats: no function of this header
 * has both "slab" and "grad" in its name.  The config, its checks and limits (n_bins * (n_bands + 1) <= 640), the bins, the
 * gating and the SPHX:GradStats:* identifiers are those of section 2n.  A sample is a sum over particles, so it is divided
 * like the flow statistics': a slab bins, at the end of a sampled step, the estimates of the fluid particles it owns (those
 * sphx_slab_snapshot marks owned, with 0 <= y <= DH), and what a read returns are the slab's PARTIAL sums -- the ring's twelve
 * fields, count and skipped included, are the element-wise sums over the ranks; n_samples, t_first and t_last come from the
 * clock and are the same on every rank, also on a slab that owns no particle of a band.  The PARTNERS of a particle are all
 * the other fluid particles the slab holds, its halo copies included -- in the cell columns next to the owned ones they carry
 * the finished step's positions and velocities up to the summation order of their own neighbour lists, a few ulps, and their
 * particles' masses -- and, with with_walls, the wall particles the slab holds.  The slab's window is open: the first slab
 * holds the last slab's particles at x - DL and the last slab the first slab's at x + DL, so a partner across the periodic
 * seam enters with its plain dx and no minimum image; a ring is at least 20h long, so no copy is a particle's own image
 * within 2h.  Band membership goes by x mod DL, whatever frame a slab keeps x in.  The bound 2^e > 16 vmax / h that decides
 * between summed and skipped comes from the ring's maximum speed and is the same on every rank; the fixed-point quantum
 * comes from the number of particles the slab holds and is the slab's own.  The estimate differentiates the copies' state,
 * so a ring's sums equal a single context's within a few hundred times the copies' few ulps, not to the last bits; count and
 * skipped are equal wherever no particle sits at a bin or band edge, at det M = det_min or at the bound.  A refused enable
 * leaves a running sampler, its sums and a prepared graph as they are.  SPHX:GradStats:disabled: a reset or a read while the
 * sampler is off; disable is a no-op then.  There is no "sample now" call.  sphx_ctx_grad_stats_* keep refusing a slab
 * (SPHX:GradStats:slab). */
int sphx_slab_gstats_enable(sphx_ctx *ctx, const sphx_grad_stats_config *cfg);
int sphx_slab_gstats_disable(sphx_ctx *ctx);
/* Clears the sums and the sample count; the configuration stays. */
int sphx_slab_gstats_reset(sphx_ctx *ctx);
/* The slab's partial sums of one band; arguments as sphx_ctx_grad_stats_read. */
int sphx_slab_gstats_read(sphx_ctx *ctx, int band, int capacity, int *n_bins, double *sums, int64_t *n_samples, double *t_first,
                          double *t_last);
/* Particle tracers of a ring (the tracers of section 2p; k_tracers_s).  The one sampler whose subject moves between the slabs:
 * OWNERSHIP MOVES WITH THE PARTICLE.  cfg holds the RING's id list, the same on every rank (the rows of the channel the ring was
 * cut from); the config, its checks and the SPHX:Tracers:config identifier are those of section 2p, the bound
 * capacity * n_tracers * 4 <= 1 << 27 doubles holding per slab with the ring's n_tracers.  At the end of a sampled step a slab
 * copies x, y, u_x, u_y of every tracked particle it OWNS at that step -- the fluid particles sphx_slab_snapshot marks owned,
 * never a halo copy, which is its owner's to record -- into the particle's column of a DENSE row of n_tracers columns, the bits
 * sphx_slab_snapshot returns for that id, with no arithmetic: x in the slab's own frame as the state holds it, which may be
 * below 0 on the first slab and at or above DL on the last.  Every fluid row has exactly one owner at every step, so every
 * column of a record is written by exactly one slab of the ring; ownership changes hands at the ring's re-binnings only.
 *  Columns a slab did not own: the value buffer is filled with NaN (every byte 0xFF) at enable and the rows a draining read
 *    hands out are filled again, so a column the slab did not write reads NaN in all four fields.  A particle's x is never NaN.
 *  n_owned replaces n_missing: the slab stores the number of tracers it met, per record, beside {step, t}.  The ring's
 *    invariant is that the slabs' n_owned of a record add up to n_tracers: a particle lost or held twice when ownership changes
 *    hands shows in the record of the very step it happens.  A slab that owns no tracer still records {step, t} with
 *    n_owned = 0, so step, t, n_records and n_dropped are the same on every rank.
 *  The ring's series: every column of every record from the one rank where it is not NaN; nothing is added.
 *  Memory: capacity * (3 + n_tracers * 4) doubles per slab -- the dense form costs n_ranks times a context's ring-wide.
 *  A refused enable leaves a running series, its records and a prepared graph as they are.  SPHX:Tracers:disabled: a read while
 *  the tracers are off; disable is a no-op then.  There is no "sample now" call.  sphx_ctx_tracers_* keep refusing a slab
 *  (SPHX:Tracers:slab). */
int sphx_slab_tracers_enable(sphx_ctx *ctx, const sphx_tracers_config *cfg);
int sphx_slab_tracers_disable(sphx_ctx *ctx);
/* The slab's records: times [capacity][2], values [capacity][*n_tracers][SPHX_TRACER_FIELDS] (row-major, NaN where the slab
 * was not the owner) and n_owned [capacity]; ids [*n_tracers]: the ring's list as given at enable.  Any output may be NULL.
 * capacity = 0: only the sizes and counts are reported, nothing is copied or drained; SPHX:Tracers:capacity when an array is
 * given and capacity is below n_records.  drain != 0: the buffer is emptied, n_dropped zeroed and the rows handed out filled
 * with NaN again after copying.  Waits for the slab's stream(s) itself. */
int sphx_slab_tracers_read(sphx_ctx *ctx, int capacity, double *times, double *values, int64_t *n_owned, int32_t *ids,
                           int *n_tracers, int *n_records, int64_t *n_dropped, int drain);
/* Density statistics of a ring (the sampler of section 2r; k_dens_stats_s).  The names say dstats: no function of this header
 * has both "slab" and "dens" in its name.  The config, its checks and limits, the bins, the histogram, the gating and the
 * SPHX:DensStats:* identifiers are those of section 2r.  A sample is a sum over particles, so it is divided like the flow
 * statistics': a slab bins, at the end of a sampled step, the re-summed densities of the fluid particles it owns (those
 * sphx_slab_snapshot marks owned, with 0 <= y <= DH), and what a read returns are the slab's PARTIAL sums -- the ring's count,
 * outliers, four summed fields, histogram, below and above are the element-wise sums over the ranks, its d_min the smallest and
 * its d_max the largest of the ranks' (+inf / -inf on a slab that has summed no particle of the bin); n_samples, t_first and
 * t_last come from the clock and are the same on every rank, also on a slab that owns no particle of a band.  The PARTNERS of
 * a particle are all the other fluid particles the slab holds, its halo copies included, and the wall particles the slab holds,
 * always.  Of a partner only the position is read -- in the cell columns next to the owned ones a copy carries the finished
 * step's position up to the summation order of its own neighbour lists, a few ulps -- and of the particle itself its position
 * and its mass: nothing is asked of a copy's mass or velocity.  The slab's window is open: the first slab holds the last slab's
 * particles at x - DL and the last slab the first slab's at x + DL, so a partner across the periodic seam enters with its plain
 * dx and no minimum image; a ring is at least 20h long, so no copy is a particle's own image within 2h.  Band membership goes
 * by x mod DL, whatever frame a slab keeps x in.  2^e >= delta_bound, which decides between summed and outlier, comes from the
 * config and is the same on every rank; the fixed-point quantum comes from the number of particles the slab holds and is the
 * slab's own.  A density is continuous in the copies' positions, so a ring's sums equal a single context's within the copies'
 * few ulps times the slope of W, not to the last bits; count, outliers and the histogram are equal wherever no particle sits
 * at a bin, band or histogram edge or at the bound.  A refused enable leaves a running sampler, its sums and a prepared graph
 * as they are.  SPHX:DensStats:disabled: a reset or a read while the sampler is off; disable is a no-op then.  There is no
 * "sample now" call.  sphx_ctx_dens_stats_* keep refusing a slab (SPHX:DensStats:slab). */
int sphx_slab_dstats_enable(sphx_ctx *ctx, const sphx_dens_stats_config *cfg);
int sphx_slab_dstats_disable(sphx_ctx *ctx);
/* Clears the sums, the extremes, the histogram and the sample count; the configuration stays. */
int sphx_slab_dstats_reset(sphx_ctx *ctx);
/* The slab's partial sums of one band; arguments as sphx_ctx_dens_stats_read. */
int sphx_slab_dstats_read(sphx_ctx *ctx, int band, int capacity, int hist_capacity, int *n_bins, int *n_hist, double *sums,
                          int64_t *hist, int64_t *below, int64_t *above, int64_t *n_samples, double *t_first, double *t_last);

#ifdef __cplusplus
}
#endif
#endif /* SPHX_H */
