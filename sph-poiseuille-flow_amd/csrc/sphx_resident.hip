// sphx_resident.hip -- host side of the device-resident SPH step (include/sphx.h section 2):
// context creation (cell grid build on device), the step loop as hipGraph replays, download, monitors,
// MEX-convention pair-list emission, per-kernel HIP-event timing, and the x-slab (multi-GPU) entry
// points.  The kernels are in sphx_kernels.hpp.
#include <dlfcn.h>
#include <rccl/rccl.h>  // types and prototypes only: librccl is loaded at run time (see Rccl), libsphx does not link it

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <map>

#include "sphx_common.hpp"
#include "sphx_kernels.hpp"
#include "sphx_sampler_state.hpp"

namespace sphx {

struct KernelTimer {
    std::vector<std::string> names;
    std::vector<double> total_ms;
    std::vector<int64_t> launches;
    struct Pending { int idx; hipEvent_t a, b; };
    std::vector<Pending> pending;     // eager launches: one-shot events
    std::vector<Pending> graph_evs;   // events recorded by nodes of the profiling graph (re-armed per replay)
    bool warned = false, timer_log = false;  // (timer_log: SPHX_DEBUG_SWITCHES=log)
    int index_of(const char *name)
    {
        for (size_t k = 0; k < names.size(); ++k) if (names[k] == name) return (int)k;
        names.emplace_back(name); total_ms.push_back(0.0); launches.push_back(0);
        return (int)names.size() - 1;
    }
    void add(int idx, hipEvent_t a, hipEvent_t b)
    {
        float ms = 0.f;
        const hipError_t e = hipEventElapsedTime(&ms, a, b);
        if (e == hipSuccess) { total_ms[idx] += ms; launches[idx] += 1; }
        else {
            (void)hipGetLastError();
            if (timer_log && !warned) { warned = true; fprintf(stderr, "sphx: hipEventElapsedTime: %s\n", hipGetErrorString(e)); }
        }
    }
    void collect()
    {
        for (auto &p : pending) { add(p.idx, p.a, p.b); (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
        pending.clear();
    }
    void collect_graph() { for (auto &p : graph_evs) add(p.idx, p.a, p.b); }
    void drop_graph_events()
    {
        for (auto &p : graph_evs) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
        graph_evs.clear();
    }
};

// The host's step-slot schedule of a context, of a batch and of each member of a batch.  A step slot is the set of launches
// of one step; it does nothing when the device clock says the loop has stopped.  The phase: state buffers S[cur]
// (x,y,vx,vy,drho), layout buffers L[lay] (mass,id,start,cell), `pos` = steps taken since the grid was built.  `slot` is the
// step index the next enqueued slot will have if every slot before it executes.
struct Schedule {
    int cur = 0, lay = 0, pos = 0;
    int64_t slot = 0;
    int64_t cool_until = 0;  // after a forced re-binning every slot up to this index re-bins (cool-down)
    int64_t cool_len = 0;    // length of the last cool-down (doubles when forced re-binnings keep coming)
    int64_t n_forced = 0;    // forced re-binnings so far
    // Replayable graphs, keyed by the phase they were captured from and their length: {cur, lay, pos, slots}.  A graph
    // of graph_slots() slots (a multiple of the 2K-step period) hands the phase back unchanged, so a long run replays
    // ONE graph whatever phase it was entered at; exact-length batches (sphx_ctx_enqueue_steps, advance with
    // max_steps -- a caller logging every 20 steps) get a graph per (phase, length), captured the first time that
    // combination comes up (or ahead of time by sphx_ctx_prepare_steps).
    struct Graph { hipGraphExec_t exec = nullptr; bool launched = false; };
    std::map<std::array<int, 4>, Graph> graphs;
    int64_t slots_replayed = 0, slots_eager = 0, graphs_captured = 0;

    // A forced re-binning is answered with a COOL-DOWN: for the next cool_len steps every step re-bins (exactly the loop
    // without a skin), then the schedule returns to K.  What outruns the skin is almost always one particle making a
    // few large transport shifts in a row (max over millions of particles: at 0.5-6 M particles it happens every few
    // thousand steps); shrinking K for thousands of steps -- the first policy -- cost 30 % of the throughput of long
    // runs at those sizes.  cool_until only changes at forced re-binnings (device-side events): the schedule stays
    // independent of how the host chunks its calls.
    bool rebuilds(int K) const { return pos >= K - 1 || slot < cool_until; }

    // one slot on; returns whether it re-binned
    bool advance(int K)
    {
        const bool rebuild = rebuilds(K);
        slot += 1;
        cur ^= 1;
        if (rebuild) { lay ^= 1; pos = 0; }
        else pos += 1;
        return rebuild;
    }

    // a forced re-binning at slot `now`: 16 slots of cool-down, doubled (up to 1024) while the next forced re-binning
    // follows the previous cool-down within two re-binning cycles, so a flow that really is too fast for the skin
    // degrades to re-binning every step
    void cool_down(int64_t now, int K)
    {
        const bool again = n_forced > 0 && now - cool_until <= 2 * (int64_t)K;
        cool_len = again ? std::min<int64_t>(2 * std::max<int64_t>(cool_len, 16), 1024) : 16;
        cool_until = now + cool_len;
        n_forced += 1;
    }

    void drop_graphs()
    {
        for (auto &kv : graphs)
            if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
        graphs.clear();
    }
};

}  // namespace sphx

using namespace sphx;

namespace sphx {
struct BatchArena;
}

struct sphx_ctx {
    sphx_params prm{};
    Grid grid{};
    Phys phys{};
    int nf = 0, nw = 0, nt = 0;  // caller's global counts (single GPU: nf particles resident)
    int cap = 0;                 // particle capacity of the device arrays
    int lpp = 1, spg = 2;
    bool big_scan = false;
    int n_vpart = 0;             // entries of vpart / dpart the clock kernel reduces
    int n_tiles = 0;
    hipStream_t stream = nullptr;
    bool own_stream = true;

    // Cell grid with a skin: cells are 2h + skin wide, particles are re-binned only every `rebuild_every` steps
    // ("rebuild" step: 7 launches, "move" step: 5).  Between two builds every sweep is centred on the cell a
    // particle was binned into, which finds all neighbours while nobody has drifted more than skin/2; the
    // device clock tracks the largest drift (Clock::drift) and stops the loop before the bound is violated.
    double skin = 0.0;
    int rebuild_every = 1;       // re-binning interval K (constant)

    // where the current state lives (Schedule: phase, cool-down, graphs); the phase is derived from the device step count
    Schedule sched;
    int64_t epoch_step = 0;      // step count at which (epoch_cur, epoch_lay, epoch_pos, ...) held
    int epoch_cur = 0, epoch_lay = 0, epoch_pos = 0;
    int epoch_out_lay = 0;
    int out_lay = 0;             // layout the per-step outputs (rho,p,force,Vol,B) are stored in; when it is not
                                 // `lay`, tmp.src_of maps current slots to the slots of those outputs
    int64_t last_forced_step = 0;
    int64_t n_rebins = 0, epoch_n_rebins = 0;  // re-binnings executed by step slots of the static schedule (not the forced ones)
    int64_t pending_target = 0;  // step count the sphx_ctx_enqueue_steps calls since the last sync aim for
    bool have_step_outputs = false;

    // storage
    DevBuf<double2> fpos_[2], fvel_[2], fposb_[2];
    DevBuf<double> fdrho_[2], fmass_[2];
    DevBuf<int> fid_[2], fstart_[2], fcell_[2];
    DevBuf<double2> posn, veln, ffp, ff;
    DevBuf<double4> fa, fB;
    DevBuf<double> drhon, rho_out, p_out, vpart, dpart, vtile, fvol;
    int n_vtiles = 0;            // > 0: k_max_tiles folds the per-block maxima first (very many blocks)
    DevBuf<int> cellid, count, perm, src_of, nl_idx, nl_cnt, sl_idx, sl_cnt, flags, tile;
    DevBuf<int> nl_pk, sl_pk, nl_pk2;  // large-channel kernels: fluid entries as 16-bit index differences (FluidTmp::nl_pk)
    DevBuf<int> tmap;                  // ... and every workgroup's tile layout (FluidTmp::tmap)
    DevBuf<double2> wpos;
    DevBuf<double4> wa;
    DevBuf<int> wid, wstart, wrow_any;
    DevBuf<Clock> clock;
    DevBuf<double> tau_part, tau_out;
    Clock *h_clock = nullptr;  // pinned
    Clock *h_pub = nullptr;    // pinned + mapped: the device writes the clock here whenever the loop stops (Clock::pub)
    long long host_seq = 0;    // batches armed so far (k_prepare launches), cf. Clock::seq

    FluidTmp tmp{};
    Walls walls{};
    int n_blocks_particles = 0;  // grid of the LPP kernels (capacity based), in workgroups of 256 threads
    int n_blocks_flat = 0;       // grid of one-thread-per-particle kernels
    // Compact step kernels (16 / 32 lanes per particle): threads per workgroup of the passes that are not part of the re-binning
    // step (pick_block), and the workgroups of such a pass.  vpart / dpart hold one entry per workgroup of THAT size (n_vpart =
    // n_blocks_pass); the 256-thread kernels of the re-binning step fill every entry they cover.
    int block = kBlock;
    int n_blocks_pass = 0;

    int64_t chunk_slots = 128;   // slots enqueued between two host looks at the clock (adaptive, see advance)
    bool profiling = false;
    KernelTimer timer;

    // pair list held for sphx_neighbor_fetch
    DevBuf<double> pl_i, pl_j, pl_dx, pl_dy, pl_r, pl_W, pl_dW;
    size_t pl_n = 0;
    bool pl_valid = false;

    // x-slab state
    bool is_slab = false;
    int rank = 0, n_ranks = 1, halo_cols = 0, msg_cap = 0;
    int col0 = 0, col1 = 0;  // owned global columns [col0, col1)
    int ncx_ring = 0;        // ... of the ring's ncx_ring cell columns: rank r owns from (r * ncx_ring) / n_ranks
    DevBuf<double2> kpos, kvel;
    DevBuf<double> kdrho, kmass;
    DevBuf<int> kid, counters, n_new, ticket;  // (ticket: see last_workgroup_out)
    SlabPack pack{};
    int64_t slab_steps_enqueued = 0, slab_step0 = 0;
    // native step loop (sphx_slab_run / sphx_slab_group_run): library-owned message buffers, RCCL communicator
    DevBuf<double> msg_sl, msg_sr, msg_rl, msg_rr, vmax_l, vmax_g;  // (vmax_*: {max |v|, max drift})
    // skinned slabs (re-binning every K-th step): the exchange lists of the cycle, see SlabLists
    DevBuf<int> send_idx_[2], recv_slot_[2], send_cnt, recv_cnt, slot_of_id, ids_s_[2], ids_r_[2];
    SlabLists lists{};
    bool lists_ready = false;
    ncclComm_t comm = nullptr;
    hipEvent_t ev_computed = nullptr, ev_received = nullptr;  // single-process ring: cross-stream ordering
    // Skinned slabs, native loops: the local maxima and the all-reduce behind them run on a second stream beside pass E
    // (k_slab_maxima): fork after pass CD (ev_cd), join in front of k_slab_pack3 (ev_ar); ev_max: "my local maxima are out"
    // (in-process rings, where a kernel stands in for the all-reduce)
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_cd = nullptr, ev_ar = nullptr, ev_max = nullptr;
    DevBuf<double> max_part;
    DevBuf<int> ticket2;
    hipEvent_t ev_p = nullptr, ev_u = nullptr;  // "message A is packed" / "the halo is refreshed (or the layout rebuilt)"
    bool a_interior_done = false;  // the interior workgroups of the coming step's pass A were launched behind this step's pack3
    // Whole slab steps as ONE replayable graph (sphx_slab_graph_prepare): kSlabGraphSteps steps of the native loop -- kernels,
    // the RCCL calls (sphx_slab_run) or the device-to-device copies and cross-stream dependencies of an in-process ring
    // (sphx_slab_group_run; held by slab 0) -- captured once the loop has run eagerly at least twice
    hipGraphExec_t steps_graph = nullptr;
    std::vector<const sphx_ctx *> steps_graph_ring;  // the contexts the graph was captured for
    int steps_graph_cur = 0;                          // ... and the state parity it starts from
    // The graph carries the launches of the slab samplers that were on when it was captured (sphx_slab_flow_stats_* /
    // sphx_slab_history_* / sphx_slab_field_map_*): every enable / disable counts up the slab's sampler_epoch, and the graph is replayed only while the
    // epochs of the ring's slabs still add up to what they were at the capture
    int64_t sampler_epoch = 0, steps_graph_epochs = 0;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;

    // Dynamic re-binning (large channels): the device decides when to re-bin, every step carries the (self-skipping)
    // re-binning kernels, the layout is rebuilt in place -> lay stays 0, only the state parity alternates
    bool dyn = false;
    // Small channels: pass E of a step that does not re-bin and pass A of the next step share one launch
    // (k_continuity_density).  The neighbour list and the {Vol, p, rho_h, rho} records then exist once per state parity:
    // tmp_par[p] is `tmp` with the buffers of parity p; out_par = the parity of the last executed step (its Vol).
    bool fuse_ea = false;
    // ... and the step that re-bins is three launches: pass CD takes the histogram (k_forces_hist), pass E re-bins and carries the
    // clock (k_continuity_rebin) -- no k_clock_scan / k_scatter / k_reorder; the next cell sweep clears the histogram (k_density_zero)
    bool fold_rebin = false;
    bool lds_tiles_a = false;    // pass A's walk gathers the candidate positions from an LDS tile
    bool sweep_kernels = false;  // pass A's cell sweep in its large-channel form (k_density_sweep_w)
    int n_in = 1;                // dual-rate loop: inner sub-steps per step slot (1 = the reference's single-rate loop)
    DevBuf<double2> vel2;        // ... and the second velocity array its sub-steps alternate with
    DevBuf<double4> fa2;
    DevBuf<double> fvol2;
    DevBuf<int> nl_idx2, nl_cnt2;
    FluidTmp tmp_par[2] = {};
    int out_par = 0, epoch_out_par = 0;
    bool walk_kernels = false;   // lanes_per_particle <= 8: passes B, CD, E run their large-channel ("_w") forms
    bool lds_tiles = false;      // ... and the force pass stages its tile's neighbourhood in LDS
    bool lds_tiles_be = false;   // ... KGC and continuity too (2 lanes per particle, channel larger than the Infinity Cache)
    bool coded_lists = false;    // ... and the lists name tile slots instead of index differences (kSlotCodes, sphx_kernels.hpp)
    bool tail_clock = false;     // move steps carry their clock update in a tail workgroup of pass E (small channels)

    // slot samplers (sphx_sampler_state.hpp): while one is on, every step slot ends with its launch
    FlowStats fstats;  // (of a batch: member 0's serves every member, the other members' stay off)
    History hist;
    FieldMap fmap;
    Probes probes;
    ProfileSeries pseries;
    PairDist pairs;
    GradStats grads;
    Tracers tracers;
    DensStats dens;
    Modes modes;

    // Member of a batch (sphx_batch_*): the device arrays are this member's blocks of batch-wide allocations (BatchArena)
    sphx::BatchArena *arena = nullptr;
    int member = 0;
    const int *out_ids = nullptr;  // after a realignment: ids of the slots the last step's outputs are stored in (else fid_[out_lay])
    // Member 0 stands for the whole batch in the step's launch layer (launch_forms): the batch's member table and M
    const Members *members = nullptr;
    int n_members = 1;

    FluidSet view(int q, int l)
    {
        return FluidSet{fpos_[q].get(), fvel_[q].get(), fdrho_[q].get(), fmass_[l].get(), fid_[l].get(),
                        fstart_[l].get(), fcell_[l].get(), skin > 0.0 ? fposb_[l].get() : nullptr};
    }
    double half_skin() const { return 0.5 * skin; }
    unsigned long long *vpart_reset() const
    {
        return tail_clock ? reinterpret_cast<unsigned long long *>(vpart.get()) : nullptr;
    }

    ~sphx_ctx()
    {
        if (stream) (void)hipStreamSynchronize(stream);  // the buffers go back to the pool: nothing may still use them
        sched.drop_graphs();
        if (steps_graph) (void)hipGraphExecDestroy(steps_graph);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        timer.collect();
        timer.drop_graph_events();
        if (ev_computed) (void)hipEventDestroy(ev_computed);
        if (ev_received) (void)hipEventDestroy(ev_received);
        if (stream2) (void)hipStreamSynchronize(stream2);
        if (ev_cd) (void)hipEventDestroy(ev_cd);
        if (ev_ar) (void)hipEventDestroy(ev_ar);
        if (ev_max) (void)hipEventDestroy(ev_max);
        if (ev_p) (void)hipEventDestroy(ev_p);
        if (ev_u) (void)hipEventDestroy(ev_u);
        if (stream2) (void)hipStreamDestroy(stream2);
        if (h_clock) (void)hipHostFree(h_clock);
        if (h_pub) (void)hipHostFree(h_pub);
        if (stream && own_stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

// A/B switches for measurements, all behind ONE environment variable read once per process:
//   SPHX_DEBUG_SWITCHES=no_tail_clock,no_fuse_ea,no_fold_rebin,no_lds_tiles,no_coded_lists,no_lazy_out,no_xcd_align,no_wall_paths,forces_tile_320,log
// (no_tail_clock: the clock update as a launch of its own on every step; no_fuse_ea: passes E and A in separate launches;
//  no_fold_rebin: small channels re-bin with the chain k_clock_scan -> k_scatter -> k_reorder behind pass E;
//  no_lds_tiles: large-channel passes gather from global memory; no_coded_lists: index differences in every list, never tile
//  slots; no_lazy_out: force, force_prior, rho, p written by every step (FluidTmp::lazy_out); no_xcd_align: the A half of the
//  fused launch, which starts at physical block nb, numbers its blocks as if it started at block 0 (xcd_block, sphx_xcd_block.hpp);
//  block_64 / block_128 / block_256: the compact passes in workgroups of that many threads whatever pick_block says (block_256:
//  the launches as they were before the block size became a choice);
//  no_wall_paths: pass CD at 16 / 32 lanes per particle builds the pair of a prefetched wall row twice, as before the kept pairs
//  (forces_pass, WP; sphx_kernels.hpp);
//  log: forced re-binnings and timer
//  problems on stderr)
struct DebugSwitches {
    bool no_fold_rebin = false;
    bool no_tail_clock = false, no_fuse_ea = false, no_lds_tiles = false, no_coded_lists = false, no_lazy_out = false, log = false;
    bool no_xcd_align = false;
    bool no_wall_paths = false;
    bool no_slab_overlap = false;  // skinned slabs: the local maxima from pass E's tail workgroup, the all-reduce on the step's only stream (round 3)
    bool full_copyback = false;  // dynamic contexts: the in-place re-binning copies the whole layout back (round 3)
    int tail_limit = 0;  // > 0: largest pass (in workgroups) whose clock update rides in pass E's tail workgroup
    int forces_tile = 0;    // 320: the old tile size of the slot-coded force pass
    int block = 0;          // block_64 / block_128 / block_256: threads per workgroup of the compact passes (0: pick_block)
    int tiles_be_from = 0;  // > 0: passes B, E and A stage LDS tiles from this many resident particles (2 lanes per particle)
};
const DebugSwitches &debug_switches()
{
    static const DebugSwitches sw = [] {
        DebugSwitches d;
        const char *e = std::getenv("SPHX_DEBUG_SWITCHES");
        const std::string v = e ? e : "";
        auto has = [&](const char *name) { return ("," + v + ",").find(std::string(",") + name + ",") != std::string::npos; };
        d.no_tail_clock = has("no_tail_clock");
        d.no_fuse_ea = has("no_fuse_ea");
        d.no_fold_rebin = has("no_fold_rebin");
        d.no_lds_tiles = has("no_lds_tiles");
        d.no_coded_lists = has("no_coded_lists");
        d.no_lazy_out = has("no_lazy_out");
        d.no_xcd_align = has("no_xcd_align");
        d.no_wall_paths = has("no_wall_paths");
        d.log = has("log");
        d.no_slab_overlap = has("no_slab_overlap");
        d.full_copyback = has("full_copyback");
        for (int lim : {1024, 2048, 4096, 8192, 16384})
            if (has(("tail_limit_" + std::to_string(lim)).c_str())) d.tail_limit = lim;
        for (int from : {1, 250000, 500000, 750000, 1000000, 1500000, 3000000})
            if (has(("tiles_be_from_" + std::to_string(from)).c_str())) d.tiles_be_from = from;
        if (has("forces_tile_320")) d.forces_tile = 320;
        for (int b : {64, 128, 256, 320, 384, 512, 1024})
            if (has(("block_" + std::to_string(b)).c_str())) d.block = b;
        return d;
    }();
    return sw;
}

// largest pass, in workgroups, whose clock update rides in a tail workgroup of pass E (and whose passes E and A share a launch)
// Round 3: 2 048 -> 4 096.  Fusing E and A and dropping the clock launch still pays at 0.3-0.5 M particles (2 lanes: 324 k
// 139.7 -> 129.3 us/step, C4 = 499 k 180.5 -> 172.2); at 0.83 M (6 500 workgroups) it is neutral to slightly worse (270 -> 271.5).
constexpr int kTailClockBlocks = 4096;
int tail_clock_limit() { return debug_switches().tail_limit > 0 ? debug_switches().tail_limit : kTailClockBlocks; }

thread_local sphx_ctx *g_search_ctx = nullptr;  // owns the temporary context of sphx_neighbor_search until fetch
thread_local sphx_ctx *g_fetch_src = nullptr;   // context whose pair list the next sphx_neighbor_fetch copies out

template <typename K, typename... Args>
void launch_s(sphx_ctx *c, const char *name, K kernel, dim3 grid, dim3 block, size_t shmem, Args... args)
{
    if (c->profiling) {  // eager launch with an event pair (event-record nodes in a replayed graph read 0 on ROCm 7.2)
        KernelTimer::Pending p;
        p.idx = c->timer.index_of(name);
        SPHX_HIP(hipEventCreate(&p.a));
        SPHX_HIP(hipEventCreate(&p.b));
        SPHX_HIP(hipEventRecord(p.a, c->stream));
        hipLaunchKernelGGL(kernel, grid, block, shmem, c->stream, args...);
        SPHX_HIP(hipEventRecord(p.b, c->stream));
        c->timer.pending.push_back(p);
    } else {
        hipLaunchKernelGGL(kernel, grid, block, shmem, c->stream, args...);
    }
}

template <typename K, typename... Args>
void launch(sphx_ctx *c, const char *name, K kernel, dim3 grid, dim3 block, Args... args)
{
    launch_s(c, name, kernel, grid, block, 0, args...);
}

// gather of the persistent fields (pos, vel, drho, mass) into destination view d
ReorderArgs reorder_args(const double2 *pos, const double2 *vel, const double *drho, const double *mass, const int *id_src,
                         const FluidSet &d, int *src_of, int *slot_of_id = nullptr)
{
    ReorderArgs ra{};
    ra.n2 = 2;
    ra.src2[0] = pos; ra.dst2[0] = d.pos;
    ra.src2[1] = vel; ra.dst2[1] = d.vel;
    if (d.posb) {  // remember where every particle was when it was binned
        ra.n2 = 3;
        ra.src2[2] = pos; ra.dst2[2] = d.posb;
    }
    ra.n1 = 2;
    ra.src1[0] = drho; ra.dst1[0] = d.drho;
    ra.src1[1] = mass; ra.dst1[1] = d.mass;
    ra.id_src = id_src;
    ra.id_dst = d.id;
    ra.src_of = src_of;
    ra.cell_dst = d.cell;
    ra.slot_of_id = slot_of_id;
    return ra;
}

// Inner sub-steps per step slot a context asking for the dual-rate loop would run (1 = single rate).
int dual_rate_substeps(const sphx_params &prm)
{
    if (prm.dual_rate <= 1) return 1;
    const double h = prm.h;
    const double dt_ac = 0.25 * h / (1.1 * prm.c_f);  // at max|v| = 0.1 c_f, where the reference's set-up runs
    const double dt_visc = 0.125 * h * h * prm.rho0 / std::max(prm.mu, 1e-12);
    const double dt_body = 0.25 * std::sqrt(h / std::max(std::fabs(prm.gravity_g), 1e-12));
    const int fit = (int)std::floor(std::min(dt_visc, dt_body) / dt_ac);
    return std::max(1, std::min(fit, (int)prm.dual_rate));
}

// ---- The four neighbour passes on state view `s`, writing the end-of-step state through t.posn / veln / drhon ----

// What pass A does.  Sweep: sweeps the cells; SweepBuild: sweeps and writes the superset list (first step after a re-bin);
// Walk: walks the superset list; DynBuildWalk (dynamic contexts): build and walk, each skipping itself according to the
// clock's `fresh`; SlabWalk (slabs): the walk alone, on a grid that is not fresh
enum class PassA { Sweep, SweepBuild, Walk, DynBuildWalk, SlabWalk };
// The workgroups a slab's walk covers (slab_part_skips; the values are its `part`)
enum class SlabPart { All = 0, Interior = 1, Boundary = 2 };
// Pass E gets one workgroup more (the values are the kernels' `tail`), which advances the clock -- no k_clock_scan after
// this step -- or leaves a slab's local maxima (slab_seal_tail)
enum class Tail { None = 0, Clock = 1, SlabMaxima = 2 };
// Dual-rate loop, compact kernels only: this launch of pass CD / E belongs to an inner sub-step -- CD does the pressure part
// only, E hands the next sub-step its half-step density
enum class Rate { Outer = 0, Inner = 1 };
// Pass E's histogram of the new positions (the values are continuity_body's do_hist).  ThisStep: this step re-bins (static
// schedule); hist_from_step(K): a dynamic context, from the K-th step since the last re-binning on
enum class Hist : int { None = 0, ThisStep = 1 };
Hist hist_from_step(int K) { return Hist(100 + K); }
// The walk kernels' cond_fresh (density_pass): kAlways, kIfFresh, or "not on a fresh grid" with the slab part above it
constexpr int kAlways = -1, kIfFresh = 1;
int unless_fresh(SlabPart part) { return (int)part << kPassPartShift; }

// f(std::integral_constant<int, LPP>) for the context's lanes per particle
template <typename F>
void with_lpp(const sphx_ctx *c, F &&f)
{
    switch (c->lpp) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        case 16: f(std::integral_constant<int, 16>{}); break;
        case 32: f(std::integral_constant<int, 32>{}); break;
        default: throw Error(SPHX_ERR_ARG, "SPHX:Ctx:lpp", "lanes_per_particle must be 1,2,4,8,16 or 32");
    }
}

// f(std::integral_constant<int, BLK>) for the context's block size (compact kernels)
template <typename F>
void with_block(const sphx_ctx *c, F &&f)
{
    switch (c->block) {
        case 64: f(std::integral_constant<int, 64>{}); break;
        case 128: f(std::integral_constant<int, 128>{}); break;
        case 256: f(std::integral_constant<int, 256>{}); break;
        case 320: f(std::integral_constant<int, 320>{}); break;
        case 384: f(std::integral_constant<int, 384>{}); break;
        case 512: f(std::integral_constant<int, 512>{}); break;
        case 1024: f(std::integral_constant<int, 1024>{}); break;
        default: throw Error(SPHX_ERR_STATE, "SPHX:Ctx:block", "internal: block size must be 64, 128, 256, 512 or 1024");
    }
}

// f(std::bool_constant<WP>): the compact pass CD with its kept wall pairs, or (no_wall_paths) in its earlier form
template <typename F>
void with_wall_paths(F &&f)
{
    if (debug_switches().no_wall_paths) f(std::false_type{});
    else f(std::true_type{});
}

// The form of a large-channel ("_w") kernel, handed to f as compile-time TILE / CODED: slot-coded lists (2 lanes per particle,
// every pass with a tile: the CODED forms of the same kernels) on a tile of TILE_CODED slots, an LDS tile of TILE_LDS slots
// (tile_ranges), or gathers from global memory
template <int LPP, int TILE_CODED, int TILE_LDS, typename F>
void with_form(const sphx_ctx *c, bool lds, F &&f)
{
    if constexpr (LPP == 2) {
        if (c->coded_lists) { f(std::integral_constant<int, TILE_CODED>{}, std::true_type{}); return; }
    }
    if (lds) f(std::integral_constant<int, TILE_LDS>{}, std::false_type{});
    else f(std::integral_constant<int, 0>{}, std::false_type{});
}

// ---- Where a batch differs.  The step slots of a batch are launched on its member 0 (sphx_ctx::members), and a kernel of the
// step runs in its batch form there: the "_b" wrapper of the same body (Members, sphx_kernels.hpp) on a grid of M rows, member =
// blockIdx.y, taking (members, q, ...) for (clock, q, ...) and every pointer as member 0's.  launch_forms is the only place that
// tells the two apart; only the compact kernels have batch forms. ----

// a step kernel named together with its batch form (nullptr: it has none)
template <typename K, typename KB = std::nullptr_t>
struct Forms {
    K one;
    KB batch = nullptr;
};
template <typename K, typename KB> Forms(K, KB) -> Forms<K, KB>;
template <typename K> Forms(K) -> Forms<K>;

// An argument of the single form that its batch form does not take: per_member -- the batch form has it by member, from the
// Members table; single_only -- it is fixed at zero there, and so must be zero for a batch
template <typename T, bool MustBeZero>
struct NotInBatch { T v; };
template <typename T> NotInBatch<T, false> per_member(T v) { return {v}; }
template <typename T> NotInBatch<T, true> single_only(T v) { return {v}; }
// ... and one only the batch form takes (the single form has it among its leading arguments, see hot_list)
template <typename T>
struct OnlyInBatch { T v; };
template <typename T> OnlyInBatch<T> batch_only(T v) { return {v}; }

[[noreturn]] void no_batch_form(const char *name)
{
    throw Error(SPHX_ERR_STATE, "SPHX:Batch:internal", std::string("internal: a batch met ") + name + ", which has no batch form here");
}
// a launch of the step that no batch may reach
void single_form_only(const sphx_ctx *c, const char *name) { if (c->members) no_batch_form(name); }

template <typename T> std::tuple<T> single_arg(const T &x) { return std::tuple<T>(x); }
template <typename T, bool Z> std::tuple<T> single_arg(NotInBatch<T, Z> x) { return std::tuple<T>(x.v); }
template <typename T> std::tuple<> single_arg(OnlyInBatch<T>) { return {}; }
template <typename T> std::tuple<T> batch_arg(const char *, const T &x) { return std::tuple<T>(x); }
template <typename T> std::tuple<T> batch_arg(const char *, OnlyInBatch<T> x) { return std::tuple<T>(x.v); }
template <typename T, bool Z> std::tuple<> batch_arg(const char *name, NotInBatch<T, Z> x)
{
    if constexpr (Z) { if (!(x.v == T{})) no_batch_form(name); }
    return {};
}

// kernel k on `blocks` workgroups (per member) of `block` threads: k.one(clock, q, args...) or k.batch(members, q, args...)
template <typename C, typename... P, typename KB, typename... A>
void launch_forms(sphx_ctx *c, const char *name, Forms<void (*)(C, P...), KB> k, unsigned blocks, unsigned block, size_t shmem, int q, const A &... args)
{
    if (!c->members) {
        std::apply([&](const auto &... a) { launch_s(c, name, k.one, dim3(blocks), dim3(block), shmem, static_cast<C>(c->clock.get()), q, a...); },
                   std::tuple_cat(single_arg(args)...));
    } else if constexpr (std::is_null_pointer_v<KB>) {
        no_batch_form(name);
    } else {
        std::apply([&](const auto &... a) { launch_s(c, name, k.batch, dim3(blocks, c->n_members), dim3(block), shmem, *c->members, q, a...); },
                   std::tuple_cat(batch_arg(name, args)...));
    }
}

// every pass kernel takes (clock, q, grid, phys, S, temporaries, walls) first
template <typename K, typename KB, typename... X>
void launch_pass(sphx_ctx *c, const char *name, Forms<K, KB> k, unsigned blocks, int q, const FluidSet &s, const FluidTmp &t, X... extra)
{
    launch_forms(c, name, k, blocks, kBlock, 0, q, c->grid, per_member(c->phys), s, t, c->walls, extra...);
}
template <typename K, typename... X>  // (a pass kernel that has no batch form)
void launch_pass(sphx_ctx *c, const char *name, K kernel, unsigned blocks, int q, const FluidSet &s, const FluidTmp &t, X... extra)
{
    launch_pass(c, name, Forms{kernel}, blocks, q, s, t, extra...);
}

// The compact kernels at 16 / 32 lanes per particle take a block of leading arguments in front of (grid, phys, S, ...): at most
// fourteen dwords with the clock and q, delivered in registers with the wave (sphx_kernels.hpp, "Leading arguments").  Each
// kernel writes them over the fields of the structs it gets by value, so every value is taken HERE, from the very views the
// same launch passes -- s, t for a pass of the step, sn, tn for the A half of the fused launch.  A batch form has none of
// them: it derives its views from the Members table.
// shape (workgroups of the pass without its tail, the pass's flag), row counts, list, stride, capacity
auto hot_list(unsigned nblk, int flag, const FluidTmp &t) { return std::make_tuple(pass_shape((int)nblk, flag), t.nl_cnt, t.nl_idx, t.nl_stride, t.cap); }
auto hot_kgc(unsigned nblk, int flag, const FluidSet &s, const FluidTmp &t) { return std::tuple_cat(hot_list(nblk, flag, t), std::make_tuple(s.pos, t.a)); }
auto hot_forces(unsigned nblk, int flag, const FluidSet &s, const FluidTmp &t) { return std::tuple_cat(hot_list(nblk, flag, t), std::make_tuple(s.pos, s.vel)); }
auto hot_continuity(unsigned nblk, int flag, const FluidSet &s, const FluidTmp &t) { return std::tuple_cat(hot_list(nblk, flag, t), std::make_tuple(s.pos, t.veln)); }
auto hot_walk(unsigned nblk, int flag, const FluidSet &s, const FluidTmp &t)  // (the superset list)
{
    return std::make_tuple(pass_shape((int)nblk, flag), t.sl_cnt, t.sl_idx, t.nl_stride, t.cap, s.pos, s.mass);
}
auto hot_fused(unsigned nblk, int flag, const FluidTmp &t, const FluidTmp &tn)  // (pass E's list, the superset list of pass A's side)
{
    return std::make_tuple(pass_shape((int)nblk, flag), t.nl_cnt, t.nl_idx, tn.sl_cnt, tn.sl_idx, t.nl_stride, tn.nl_stride);
}
template <typename K, typename KB, typename... H, typename... X>
void launch_pass_hot_blk(sphx_ctx *c, const char *name, Forms<K, KB> k, unsigned blocks, unsigned block, int q, const std::tuple<H...> &hot,
                         const FluidSet &s, const FluidTmp &t, X... extra)
{
    std::apply([&](auto... h) { launch_forms(c, name, k, blocks, block, 0, q, per_member(h)..., c->grid, per_member(c->phys), s, t, c->walls, extra...); },
               hot);
}
template <typename K, typename KB, typename... H, typename... X>
void launch_pass_hot(sphx_ctx *c, const char *name, Forms<K, KB> k, unsigned blocks, int q, const std::tuple<H...> &hot, const FluidSet &s,
                     const FluidTmp &t, X... extra)
{
    launch_pass_hot_blk(c, name, k, blocks, kBlock, q, hot, s, t, extra...);
}

// 16 / 32 lanes per particle (small channels) run the compact kernels (32-bit lists); fewer lanes (large channels) the "_w"
// forms, see sphx_kernels.hpp -- fluid list entries are 16-bit index differences, so builders and walkers always go together.
// LDS tiles: the force pass always; KGC and continuity where measured to pay (lds_tiles_be)
void launch_pass_a(sphx_ctx *c, int q, const FluidSet &s, const FluidTmp &t, PassA mode, SlabPart part = SlabPart::All)
{
    const unsigned np = c->n_blocks_particles;
    const bool walks = mode == PassA::Walk || mode == PassA::DynBuildWalk || mode == PassA::SlabWalk;
    const bool sweeps = !walks || mode == PassA::DynBuildWalk;
    const bool builds = mode == PassA::SweepBuild || mode == PassA::DynBuildWalk;
    const char *sweep_name = builds ? "k_density_build" : "k_density";
    const int cond_sweep = mode == PassA::DynBuildWalk ? kIfFresh : kAlways;
    const int cond_walk = mode == PassA::Walk ? kAlways : unless_fresh(part);
    with_lpp(c, [&](auto lpp) {
        constexpr int LPP = decltype(lpp)::value;
        if constexpr (LPP >= 16) {
            if (mode == PassA::Sweep) launch_pass(c, sweep_name, Forms{k_density<LPP, 0>, k_density_b<LPP, 0>}, np, q, s, t, cond_sweep);
            else if (mode == PassA::SweepBuild && c->fold_rebin) launch_pass(c, sweep_name, k_density_zero<LPP>, np, q, s, t, cond_sweep);
            else if (sweeps) launch_pass(c, sweep_name, Forms{k_density<LPP, 1>, k_density_b<LPP, 1>}, np, q, s, t, cond_sweep);
            if (walks)
                with_block(c, [&](auto blk) {
                    constexpr int BLK = decltype(blk)::value;
                    const unsigned nb = c->n_blocks_pass;
                    launch_pass_hot_blk(c, "k_density_walk", Forms{k_density_walk<LPP, BLK>, k_density_b<LPP, 2>}, nb, BLK, q,
                                        hot_walk(nb, cond_walk, s, t), s, t, batch_only(cond_walk));
                });
        } else {
            // the cell sweep: mode 0 writes the step's list, mode 1 the superset list as well
            // the build variant of a dynamic context is idle on four steps out of five: a grid-stride launch of an eighth
            // of the workgroups costs an eighth to skip (6 M particles: 47 k idle workgroups were ~70 us of every step)
            const unsigned nb = cond_sweep >= 0 ? std::max<unsigned>(1u, (unsigned)c->n_blocks_particles / 8u) : (unsigned)c->n_blocks_particles;
            if (sweeps)
                with_form<LPP, 0, 0>(c, false, [&](auto, auto coded) {
                    constexpr bool CODED = decltype(coded)::value;
                    if (builds) launch_pass(c, sweep_name, k_density_sweep_w<LPP, 1, CODED>, nb, q, s, t, cond_sweep, c->n_blocks_particles);
                    else launch_pass(c, sweep_name, k_density_sweep_w<LPP, 0, CODED>, nb, q, s, t, cond_sweep, c->n_blocks_particles);
                });
            if (walks)
                with_form<LPP, kSlotCodes, tile_slots(LPP)>(c, c->lds_tiles_a, [&](auto tile, auto coded) {
                    launch_pass(c, "k_density_walk", k_density_w<LPP, decltype(tile)::value, decltype(coded)::value>, np, q, s, t, cond_walk);
                });
        }
    });
}

// The temporaries as a compact pass at the context's block size gets them.  The kernels of the re-binning step (k_forces_hist,
// k_continuity_rebin) always run 256 threads, so a context whose other passes do not has two sets of per-workgroup maxima in
// vpart / dpart: the first n_blocks_particles entries for the 256-thread kernels, n_blocks_pass entries behind them for the
// passes.  Pass CD and pass E (with its tail) of one step always run at the same size, so a tail finds its step's entries.
FluidTmp pass_tmp(const sphx_ctx *c, FluidTmp t)
{
    if (c->lpp >= 16 && c->block != kBlock) { t.vpart += c->n_blocks_particles; t.dpart += c->n_blocks_particles; t.n_vpart = c->n_blocks_pass; }
    return t;
}

void launch_pass_b(sphx_ctx *c, int q, const FluidSet &s, const FluidTmp &t)
{
    const unsigned np = c->n_blocks_particles;
    const int finish_half = c->fuse_ea ? 1 : 0;
    with_lpp(c, [&](auto lpp) {
        constexpr int LPP = decltype(lpp)::value;
        if constexpr (LPP >= 16)
            with_block(c, [&](auto blk) {
                constexpr int BLK = decltype(blk)::value;
                const unsigned nb = c->n_blocks_pass;
                launch_pass_hot_blk(c, "k_kgc", Forms{k_kgc<LPP, BLK>, k_kgc_b<LPP>}, nb, BLK, q, hot_kgc(nb, finish_half, s, t), s, t,
                                    batch_only(finish_half));
            });
        else
            with_form<LPP, kSlotCodes, tile_slots(LPP)>(c, c->lds_tiles_be, [&](auto tile, auto coded) {
                launch_pass(c, "k_kgc", k_kgc_w<LPP, decltype(tile)::value, decltype(coded)::value>, np, q, s, t, finish_half);
            });
    });
}

void launch_pass_cd(sphx_ctx *c, int q, const FluidSet &s, const FluidTmp &t_, Rate rate = Rate::Outer)
{
    const FluidTmp t = pass_tmp(c, t_);
    const unsigned np = c->n_blocks_particles;
    with_lpp(c, [&](auto lpp) {
        constexpr int LPP = decltype(lpp)::value;
        if constexpr (LPP >= 16) {
            with_block(c, [&](auto blk) {
                constexpr int BLK = decltype(blk)::value;
                const unsigned nb = c->n_blocks_pass;
                with_wall_paths([&](auto wp) {
                    constexpr bool WP = decltype(wp)::value;
                    launch_pass_hot_blk(c, rate == Rate::Inner ? "k_forces_inner" : "k_forces", Forms{k_forces<LPP, BLK, WP>, k_forces_b<LPP, WP>}, nb,
                                        BLK, q, hot_forces(nb, (int)rate, s, t), s, t, batch_only((int)rate));
                });
            });
        } else {
            auto forces = [&](auto tile, auto coded) {
                launch_pass(c, "k_forces", k_forces_w<LPP, decltype(tile)::value, decltype(coded)::value>, np, q, s, t);
            };
            constexpr int TILE_LDS = LPP <= 2 ? 320 : tile_slots(LPP);
            // (the whole layout, four workgroups per CU: with 320 slots, five per CU, a quarter of the neighbours came from
            //  global memory in nearly every trip of every wave -- 6 M particles 516 -> 489 us, forces_tile_320 for the old size)
            if (debug_switches().forces_tile == 320) with_form<LPP, 320, TILE_LDS>(c, c->lds_tiles, forces);
            else with_form<LPP, kForceSlots, TILE_LDS>(c, c->lds_tiles, forces);
        }
    });
}

void launch_pass_e(sphx_ctx *c, int q, const FluidSet &s, const FluidTmp &t_, Tail tail = Tail::None, Hist hist = Hist::None,
                   Rate rate = Rate::Outer)
{
    const FluidTmp t = pass_tmp(c, t_);
    const unsigned ne = c->n_blocks_particles + (tail != Tail::None ? 1 : 0);
    const char *name = rate == Rate::Inner ? "k_continuity_inner" : tail != Tail::None ? "k_continuity_clock" : "k_continuity";
    with_lpp(c, [&](auto lpp) {
        constexpr int LPP = decltype(lpp)::value;
        if constexpr (LPP >= 16)
            with_block(c, [&](auto blk) {
                constexpr int BLK = decltype(blk)::value;
                const unsigned nb = c->n_blocks_pass;
                launch_pass_hot_blk(c, name, Forms{k_continuity_compact<LPP, BLK>, k_continuity_b<LPP>}, nb + (tail != Tail::None ? 1 : 0), BLK, q,
                                    hot_continuity(nb, (int)tail, s, t), s, t, (int)hist, batch_only((int)tail), single_only((int)rate));
            });
        else
            with_form<LPP, kSlotCodes, tile_slots(LPP)>(c, c->lds_tiles_be, [&](auto tile, auto coded) {
                launch_pass(c, name, k_continuity<LPP, true, decltype(tile)::value, decltype(coded)::value>, ne, q, s, t, (int)hist, (int)tail, 0);
            });
    });
}

// all four, as the steps that launch every pass on its own run them
void launch_passes(sphx_ctx *c, int q, const FluidSet &s, const FluidTmp &t, PassA mode, Tail tail = Tail::None, Hist hist = Hist::None)
{
    launch_pass_a(c, q, s, t, mode);
    launch_pass_b(c, q, s, t);
    launch_pass_cd(c, q, s, t);
    launch_pass_e(c, q, s, t, tail, hist);
}

// `t` with its end-of-step outputs going straight into state view o
FluidTmp writing_into(FluidTmp t, const FluidSet &o)
{
    t.posn = o.pos; t.veln = o.vel; t.drhon = o.drho;
    return t;
}

// Exclusive scan of the cell histogram `count` into start_next.  single(count, start, n, of_tiles) launches the one-workgroup
// kernel that scans: the histogram itself or, on big grids, the tile sums between k_scan_tiles and k_scan_add
template <typename F>
void launch_scan_around(sphx_ctx *c, const Clock *clk, int q, const int *count, int *start_next, F &&single)
{
    if (!c->big_scan) { single(count, start_next, c->grid.ncells, false); return; }
    int *tile_sum = c->tile.get(), *tile_off = c->tile.get() + c->n_tiles + 1;
    launch(c, "k_scan_tiles", k_scan_tiles, dim3(c->n_tiles), dim3(kScanBlock), clk, q, count, start_next, tile_sum, c->grid.ncells);
    single((const int *)tile_sum, tile_off, c->n_tiles, true);
    launch(c, "k_scan_add", k_scan_add, dim3(c->n_tiles), dim3(kScanBlock), clk, q, start_next, (const int *)tile_off,
           c->grid.ncells, c->n_tiles);
}
void launch_cell_scan(sphx_ctx *c, const Clock *clk, int q, const int *count, int *start_next)
{
    launch_scan_around(c, clk, q, count, start_next, [&](const int *cnt, int *start, int n, bool of_tiles) {
        launch(c, of_tiles ? "k_scan_sums" : "k_scan", k_scan_only, dim3(1), dim3(kScanBlock), clk, q, cnt, start, n);
    });
}

// What k_clock_scan gets besides the context's own (clock_scan_body, sphx_kernels.hpp); every default is "absent"
struct ClockScan {
    const double *vpart = nullptr;        // the per-block maxima of |v|^2 the kernel reduces ...
    const double *vmax_global = nullptr;  // ... or (slabs) the all-reduced max |v| that replaces the reduction
    const int *count = nullptr;           // the cell histogram ...
    int *start_next = nullptr;            // ... and the cell starts it is scanned into (steps that re-bin)
    const int *n_new = nullptr;           // slabs: the new particle count
    const double *dpart = nullptr;        // the per-block maxima of the squared drift (grids with a skin)
    int rebuilt = 0;                      // the step ends with a fresh grid
    double half_skin = 0.0;
    int *slab_counters = nullptr;
    unsigned long long *vpart_reset = nullptr;
    int dyn_K = 0;                        // dynamic contexts: the re-binning interval the clock decides rebuild_now by
};
// Finish the clock of step slot q -- and, where a.start_next is given, scan the cell histogram in the same single-workgroup kernel
// (on big grids: the tile sums, between k_scan_tiles and k_scan_add)
void launch_clock_scan(sphx_ctx *c, int q, ClockScan a)
{
    Clock *clk = c->clock.get();
    // what k_clock_scan reduces: the per-block maxima, or (many blocks) their per-tile maxima
    int n_red = a.vpart ? c->n_vpart : 0;
    if (a.vpart && c->n_vtiles) {
        double *vtile = c->vtile.get(), *dtile = vtile + c->n_vtiles;
        single_form_only(c, "k_max_tiles");
        launch(c, "k_max_tiles", k_max_tiles, dim3(c->n_vtiles), dim3(kScanBlock), (const Clock *)clk, q, c->n_vpart, a.vpart,
               a.dpart, vtile, dtile);
        a.vpart = vtile;
        if (a.dpart) a.dpart = dtile;
        n_red = c->n_vtiles;
    }
    auto clock = [&](const int *cnt, int *start, int n, bool of_tiles) {
        if (of_tiles) single_form_only(c, "k_clock_scan of tile sums");
        launch_forms(c, "k_clock_scan", Forms{k_clock_scan, k_clock_scan_b}, 1, kScanBlock, 0, q, per_member(c->phys), per_member(n_red),
                     a.vpart, single_only(a.vmax_global), (const int *)c->flags.get(), cnt, start, n, single_only(a.n_new), a.dpart,
                     a.rebuilt, a.half_skin, single_only(a.slab_counters), a.vpart_reset, single_only(a.dyn_K));
    };
    if (a.start_next) launch_scan_around(c, clk, q, a.count, a.start_next, clock);  // clock update and cell scan share one single-block kernel
    else clock(nullptr, nullptr, 0, false);
}

// index -> cell slot, then the gather of the persistent fields into destination view d
void launch_scatter_reorder(sphx_ctx *c, int q, const ReorderArgs &ra, const FluidSet &d, int max_blocks = 0)
{
    const unsigned g1 = max_blocks > 0 ? std::min(c->n_blocks_flat, max_blocks) : c->n_blocks_flat;
    const int n_fixed = 0;  // (the count is the clock's)
    launch_forms(c, "k_scatter", Forms{k_scatter, k_scatter_b}, g1, kBlock, 0, q, single_only(n_fixed), (const int *)c->cellid.get(),
                 c->count.get(), (const int *)d.start, c->perm.get());
    launch_forms(c, "k_reorder", Forms{k_reorder, k_reorder_b}, g1, kBlock, 0, q, single_only(n_fixed), (const int *)c->cellid.get(),
                 (const int *)d.start, (const int *)c->perm.get(), ra);
}

// The folded re-binning step (sphx_ctx::fold_rebin): pass CD with the histogram, then pass E re-binning into view d
void launch_fold_rebin(sphx_ctx *c, int q, const FluidSet &s, const FluidTmp &t, const FluidSet &d)
{
    with_lpp(c, [&](auto lpp) {
        constexpr int LPP = decltype(lpp)::value;
        if constexpr (LPP >= 16) {
            // (256 threads whatever the block size of the other passes, with per-workgroup maxima of their own: pass_tmp)
            const unsigned np = c->n_blocks_particles;
            with_wall_paths([&](auto wp) {
                launch_pass_hot(c, "k_forces_hist", Forms{k_forces_hist<LPP, decltype(wp)::value>}, np, q, hot_forces(np, 0, s, t), s, t);
            });
            launch_pass_hot(c, "k_continuity_rebin", Forms{k_continuity_rebin<LPP>}, np + 1, q, hot_continuity(np, 1, s, t), s, t, d);
        } else {
            throw Error(SPHX_ERR_STATE, "SPHX:Ctx:fold", "internal: folded re-binning step at this lane count");
        }
    });
}
// Pass E of a step and pass A of the next in one launch.  Tail::None: without the clock workgroup (kernel timing)
void launch_fused_ea(sphx_ctx *c, int q, const FluidSet &s, const FluidTmp &t_, const FluidSet &sn, const FluidTmp &tn, Tail tail = Tail::Clock)
{
    const FluidTmp t = pass_tmp(c, t_);
    const bool compact = c->lpp >= 16;
    const unsigned nb = compact ? c->n_blocks_pass : c->n_blocks_particles, blocks = 2 * nb + (int)tail;
    const int flags = (int)tail | (debug_switches().no_xcd_align ? kFusedUnaligned : 0);  // (the batch form numbers as before)
    with_lpp(c, [&](auto lpp) {  // 16 / 32 lanes per particle: the compact kernels; fewer: their large-channel forms
        constexpr int LPP = decltype(lpp)::value;
        if constexpr (LPP >= 16)
            with_block(c, [&](auto blk) {
                constexpr int BLK = decltype(blk)::value;
                launch_pass_hot_blk(c, "k_continuity_density", Forms{k_continuity_density<LPP, BLK>, k_continuity_density_b<LPP>}, blocks, BLK, q,
                                    hot_fused(nb, flags, t, tn), s, t, sn, tn, batch_only((int)tail));
            });
        else if constexpr (LPP >= 2)
            launch_pass(c, "k_continuity_density", k_continuity_density_w<LPP>, blocks, q, s, t, sn, tn, flags);
        else
            throw Error(SPHX_ERR_STATE, "SPHX:Ctx:fuse", "internal: fused E|A launch at this lane count");
    });
}

// One single-GPU step slot: state S[q], layout L[l].  rebuild: the step ends with re-binning into S[1-q], L[1-l]
// (7 launches); otherwise the passes write the new state straight into S[1-q] and the layout stays (5 launches).
void launch_step(sphx_ctx *c, int q, int l, int pos, bool rebuild)
{
    const PassA mode = c->skin > 0.0 ? (pos == 0 ? PassA::SweepBuild : PassA::Walk) : PassA::Sweep;
    const FluidSet s = c->view(q, l);
    ClockScan clock;
    clock.vpart = c->vpart.get();
    if (c->skin > 0.0) clock.dpart = c->dpart.get();
    clock.half_skin = c->half_skin();
    clock.vpart_reset = c->vpart_reset();
    // Dual-rate loop: passes CD and E of the inner sub-steps 1 .. n_in-1 (CD of sub-step 0 comes first, E of the last
    // sub-step after).  Sub-step m reads the velocities W_m and writes W_m+1; the W alternate between the step's output
    // array and vel2 so that the last one lands in the output array.
    auto inner_substeps = [c, q, &s](FluidTmp &t) {
        double2 *const w_final = t.veln;  // (n_in = 1: W_1 is the output array, pass CD alone)
        auto w_of = [&](int m) { return ((c->n_in - m) & 1) ? c->vel2.get() : w_final; };  // W_m, m = 1 .. n_in
        FluidSet sm = s;
        t.veln = w_of(1);
        launch_pass_cd(c, q, sm, t);
        for (int m = 1; m < c->n_in; ++m) {
            launch_pass_e(c, q, sm, t, Tail::None, Hist::None, Rate::Inner);  // E of sub-step m-1: rho, drho and the next half-step state
            sm.vel = w_of(m);
            t.veln = w_of(m + 1);
            launch_pass_cd(c, q, sm, t, Rate::Inner);  // CD of sub-step m (pressure part)
        }
    };
    if (!rebuild && c->fuse_ea) {
        // pass A of this step ran inside the previous step's last launch, unless this is the first step on a fresh grid
        const FluidSet o = c->view(1 - q, l);
        FluidTmp t = writing_into(c->tmp_par[q], o);
        if (pos == 0) launch_pass_a(c, q, s, t, PassA::SweepBuild);
        launch_pass_b(c, q, s, t);
        inner_substeps(t);
        launch_fused_ea(c, q, s, t, o, c->tmp_par[1 - q]);
        return;
    }
    if (!rebuild) {
        const FluidTmp t = writing_into(c->tmp, c->view(1 - q, l));
        if (c->tail_clock) {  // 4 launches: the last workgroup of pass E advances the clock
            launch_passes(c, q, s, t, mode, Tail::Clock);
            return;
        }
        launch_passes(c, q, s, t, mode);
        launch_clock_scan(c, q, clock);
        return;
    }
    if (c->fuse_ea) {  // re-binning step: pass A came with the previous step (or stands alone at pos 0), E has a launch of its own
        FluidTmp t = c->tmp_par[q];
        if (pos == 0) launch_pass_a(c, q, s, t, PassA::SweepBuild);
        launch_pass_b(c, q, s, t);
        if (c->fold_rebin) {  // three launches: the histogram rides in pass CD, re-binning and clock in pass E
            launch_fold_rebin(c, q, s, t, c->view(1 - q, 1 - l));
            return;
        }
        inner_substeps(t);
        launch_pass_e(c, q, s, t, Tail::None, Hist::ThisStep);
    } else {
        launch_passes(c, q, s, c->tmp, mode, Tail::None, Hist::ThisStep);
    }
    const FluidSet d = c->view(1 - q, 1 - l);
    clock.count = c->count.get();
    clock.start_next = d.start;
    clock.rebuilt = 1;
    launch_clock_scan(c, q, clock);
    launch_scatter_reorder(c, q, reorder_args(c->tmp.posn, c->tmp.veln, c->tmp.drhon, s.mass, s.id, d, c->tmp.src_of), d);
}

// One step slot of a dynamic context: the four passes on S[q] writing the new state into S[1-q], the clock (which
// decides rebuild_now), then the re-binning chain, every kernel of which returns at once unless rebuild_now is set:
// histogram of the new positions, scan, scatter, id-canonical reorder into temporaries, copy back in place.
void launch_step_dyn(sphx_ctx *c, int q)
{
    Clock *clk = c->clock.get();
    const FluidSet s = c->view(q, 0), o = c->view(1 - q, 0);
    launch_passes(c, q, s, writing_into(c->tmp, o), PassA::DynBuildWalk, Tail::None, hist_from_step(c->rebuild_every));
    ClockScan clock;
    clock.vpart = c->vpart.get();
    clock.dpart = c->dpart.get();
    clock.half_skin = c->half_skin();
    clock.dyn_K = c->rebuild_every;
    launch_clock_scan(c, q, clock);
    const int qf = q | kOnlyIfRebuild;
    const int kDynBlocks = 4096;  // grid-stride kernels: a launch that skips costs ~3 us instead of an empty 24k-block grid
    const dim3 g1(std::min(c->n_blocks_flat, kDynBlocks)), bp(kBlock);
    // Re-binning in place.  Temporaries: the tmp state arrays and the (otherwise unused) second layout's mass and id.  What
    // nobody reads during the re-ordering -- binning positions, cells, cell starts -- is written straight into the layout
    // (round 4: 52 instead of 72 bytes per particle to copy back; SPHX_DEBUG_SWITCHES=full_copyback for the old form).
    const bool lean = !debug_switches().full_copyback;
    const FluidSet d{c->posn.get(), c->veln.get(), c->drhon.get(), c->fmass_[1].get(), c->fid_[1].get(),
                     lean ? o.start : c->fstart_[1].get(), lean ? o.cell : c->fcell_[1].get(), lean ? o.posb : c->fposb_[1].get()};
    launch(c, "k_bin", k_bin, g1, bp, (const Clock *)clk, qf | kOnlyIfNoHistogram, c->grid, 0, (const double2 *)o.pos,
           c->cellid.get(), c->count.get());  // drift-triggered re-binnings only: pass E bins on the scheduled ones
    launch_cell_scan(c, clk, qf, c->count.get(), d.start);
    launch_scatter_reorder(c, qf, reorder_args(o.pos, o.vel, o.drho, s.mass, s.id, d, c->tmp.src_of), d, kDynBlocks);
    CopyBack cb{d.pos, d.vel, d.posb, o.pos, o.vel, o.posb, d.drho, d.mass, o.drho, o.mass, d.id, d.cell, d.start,
                o.id, o.cell, o.start, c->grid.ncells + 1, lean ? 1 : 0};
    launch(c, "k_copyback", k_copyback, g1, bp, (const Clock *)clk, qf, cb);
}

// host-side bookkeeping of one step slot
void track_step(sphx_ctx *c)
{
    Schedule &s = c->sched;
    if (c->dyn) {  // the layout is rebuilt in place: only the parity alternates (lay and pos stay 0, the graphs go by cur)
        s.slot += 1;
        s.cur ^= 1;
        return;
    }
    c->out_lay = s.lay;  // outputs are stored in the layout the step ran in; after a rebuild tmp.src_of maps to it
    c->out_par = s.cur;  // ... and (fuse_ea) in the record buffers of the step's state parity
    if (s.advance(c->rebuild_every)) c->n_rebins += 1;
}

// arm the device clock for a batch (k_prepare) and count it (Clock::seq / sphx_ctx::host_seq)
void arm_clock(sphx_ctx *c, double t_target, long long max_steps, int q0, const double *vmax_in)
{
    c->host_seq += 1;
    hipLaunchKernelGGL(k_prepare, dim3(1), dim3(1), 0, c->stream, c->clock.get(), c->phys, t_target, max_steps, q0, vmax_in);
}

int graph_slots(const sphx_ctx *c)
{
    const int period = c->dyn ? 2 : 2 * c->rebuild_every;  // (cur, lay, pos) returns to itself after 2K steps
    return period * std::max(1, c->spg / period);
}

constexpr int kMinGraphSlots = 4;    // shorter exact batches are launched eagerly (a replay costs ~50 us of host time)
constexpr size_t kMaxGraphs = 96;    // cache bound: 2 * 2 * K phases for a caller with one cadence, K <= 16 in practice

// ---- the step-slot schedule of contexts and batches: slot(q, l, p, rebuild) launches one step slot at phase (q, l, p) ----

// How many of the `left` slots still to enqueue from the phase of s go into one graph: a whole graph of per_graph slots
// (0: none), or -- exact_tail: the caller asked for exactly this many steps -- a shorter tail of at least kMinGraphSlots.
// 0: the next slot is launched eagerly, as is every slot of a cool-down (every slot re-bins, see Schedule::rebuilds).
int graph_run(const Schedule &s, int64_t left, int per_graph, bool exact_tail)
{
    if (s.slot < s.cool_until) return 0;
    if (left >= per_graph) return per_graph;
    return exact_tail && left >= kMinGraphSlots ? (int)left : 0;
}

// the graph of `n` step slots entered at the phase of s (static schedule: every K-th slot re-bins), captured on stream st
// the first time it is asked for
template <typename Slot>
Schedule::Graph &capture_slots(Schedule &s, hipStream_t st, int K, int n, const Slot &slot)
{
    const std::array<int, 4> key{s.cur, s.lay, s.pos, n};
    auto it = s.graphs.find(key);
    if (it != s.graphs.end()) return it->second;
    if (s.graphs.size() >= kMaxGraphs) {
        SPHX_HIP(hipStreamSynchronize(st));  // earlier batches may still be replaying the graphs about to be destroyed
        s.drop_graphs();
    }
    hipGraph_t g = nullptr;
    {
        CaptureScope capturing;  // (a pool_free on this thread in here is not poison-filled: a fill cannot join a capture)
        SPHX_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        try {
            int q = s.cur, l = s.lay, p = s.pos;
            for (int j = 0; j < n; ++j) {
                const bool rebuild = p == K - 1;
                slot(q, l, p, rebuild);
                if (rebuild) { l ^= 1; p = 0; }
                else ++p;
                q ^= 1;
            }
        } catch (...) {
            hipGraph_t junk = nullptr;
            (void)hipStreamEndCapture(st, &junk);
            if (junk) (void)hipGraphDestroy(junk);
            throw;
        }
        SPHX_HIP(hipStreamEndCapture(st, &g));
    }
    hipGraphExec_t exec = nullptr;
    const hipError_t e = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    SPHX_HIP(e);
    Schedule::Graph &cached = s.graphs[key];
    cached.exec = exec;
    s.graphs_captured += 1;
    return cached;
}

// Enqueue `slots` step slots from the phase of s on stream st; slots that find run[q]==0 are no-ops.  Whole graphs are
// replayed from ANY phase of the static schedule (see Schedule::graphs), exact tails as graphs of their own (graph_run),
// the rest is launched eagerly.  track() is the caller's bookkeeping of one slot (Schedule::advance at the least): the
// phase advances as if every slot executed, the caller recomputes it from the executed step counts.
template <typename Slot, typename Track>
void enqueue_slots(Schedule &s, hipStream_t st, int K, int per_graph, int64_t slots, bool exact_tail, const Slot &slot,
                   const Track &track)
{
    for (int64_t left = slots; left > 0;) {
        const int n = graph_run(s, left, per_graph, exact_tail);
        if (n > 0) {
            Schedule::Graph &g = capture_slots(s, st, K, n, slot);
            SPHX_HIP(hipGraphLaunch(g.exec, st));
            g.launched = true;
            s.slots_replayed += n;
            for (int k = 0; k < n; ++k) track();
            left -= n;
        } else {
            slot(s.cur, s.lay, s.pos, s.rebuilds(K));
            s.slots_eager += 1;
            track();
            left -= 1;
        }
    }
    SPHX_HIP(hipGetLastError());
}

// ---- a context's side of it ----

// one step slot of a context: the static schedule's launches or a dynamic context's, then the slot samplers that are on
auto ctx_slot(sphx_ctx *c)
{
    return [c](int q, int l, int p, bool rebuild) {
        if (c->dyn) launch_step_dyn(c, q);
        else launch_step(c, q, l, p, rebuild);
        launch_slot_samplers(c, q, l, rebuild);
    };
}

// graph length of a context's enqueues; 0 while profiling: every slot runs eagerly between its event pairs, and no graph is
// captured with them
int ctx_graph_slots(const sphx_ctx *c) { return c->profiling ? 0 : graph_slots(c); }

// enqueue_slots for a context; read_clock() recomputes the phase from the executed step count
void ctx_enqueue(sphx_ctx *c, int64_t slots, bool exact_tail)
{
    enqueue_slots(c->sched, c->stream, c->rebuild_every, ctx_graph_slots(c), slots, exact_tail, ctx_slot(c),
                  [c] { track_step(c); });
}

// Capture the graphs ctx_enqueue(c, slots, true) would replay, walking the phases on copies; no step is launched
// (sphx_ctx_prepare_steps).  First replays are slow (~4 us per step slot on ROCm 7.2: the executable graph is set up on the
// device at its first launch, hipGraphUpload does not take that over): a graph that has never run is replayed once now with
// the clock disarmed (k_disarm, see sphx_ctx_prepare_steps), so every kernel of every slot returns at once and nothing
// changes.  Small channels only: there a step is ~20 us; on millions of particles a first replay is noise and an idle pass
// over the arrays is not free.
void prepare_graphs(sphx_ctx *c, int64_t slots)
{
    Schedule &s = c->sched;
    const int cur0 = s.cur, lay0 = s.lay, pos0 = s.pos, out_lay0 = c->out_lay;
    const int64_t slot0 = s.slot;
    for (int64_t left = slots; left > 0;) {
        const int n = graph_run(s, left, ctx_graph_slots(c), true);
        if (n > 0) {
            Schedule::Graph &g = capture_slots(s, c->stream, c->rebuild_every, n, ctx_slot(c));
            if (!g.launched && c->n_blocks_particles <= 8192) {
                SPHX_HIP(hipGraphLaunch(g.exec, c->stream));
                g.launched = true;
            }
        }
        const int taken = std::max(n, 1);
        for (int k = 0; k < taken; ++k) track_step(c);
        left -= taken;
    }
    s.cur = cur0; s.lay = lay0; s.pos = pos0; c->out_lay = out_lay0; s.slot = slot0;
    SPHX_HIP(hipGetLastError());
}

void set_epoch(sphx_ctx *c)
{
    c->epoch_step = c->h_clock->step;
    c->epoch_cur = c->sched.cur; c->epoch_lay = c->sched.lay; c->epoch_pos = c->sched.pos; c->epoch_out_lay = c->out_lay;
    c->epoch_out_par = c->out_par;
    c->epoch_n_rebins = c->n_rebins;
    c->sched.slot = c->epoch_step;
}

// wait for the stream: poll for a while (a blocking wait costs ~10 us of wake-up latency, which a 20-step batch of a
// small channel notices), then block
void wait_stream(sphx_ctx *c)
{
    for (int k = 0; k < 20000; ++k) {
        const hipError_t e = hipStreamQuery(c->stream);
        if (e == hipSuccess) return;
        if (e != hipErrorNotReady) SPHX_HIP(e);
        (void)hipGetLastError();
    }
    SPHX_HIP(hipStreamSynchronize(c->stream));
}

void replay_executed(sphx_ctx *c);

void read_clock(sphx_ctx *c)
{
    wait_stream(c);
    if (c->h_pub && c->h_pub->seq == c->host_seq) {
        *c->h_clock = *c->h_pub;  // the device published the clock when the last batch stopped
    } else {  // nothing armed since the last read, or the batch ran out of slots with the loop still going
        SPHX_HIP(hipMemcpyAsync(c->h_clock, c->clock.get(), sizeof(Clock), hipMemcpyDeviceToHost, c->stream));
        SPHX_HIP(hipStreamSynchronize(c->stream));
    }
    c->timer.collect();
    replay_executed(c);
}

// replay the bookkeeping of the steps that really executed since the epoch (h_clock holds the device clock)
void replay_executed(sphx_ctx *c)
{
    const int64_t executed = (int64_t)c->h_clock->step - c->epoch_step;
    Schedule &s = c->sched;
    s.cur = c->epoch_cur; s.lay = c->epoch_lay; s.pos = c->epoch_pos; c->out_lay = c->epoch_out_lay;
    c->out_par = c->epoch_out_par;
    c->n_rebins = c->epoch_n_rebins;
    s.slot = c->epoch_step;
    if (executed > 0) {
        int64_t left = executed;
        if (c->dyn) {  // only the parity matters
            s.slot += left - (left & 1);
            left &= 1;
        }
        while (left > 0) {
            if (s.slot >= s.cool_until && left > 4 * c->rebuild_every) {
                // steady interval: (cur, lay, pos) repeats every 2K steps -> skip whole periods
                const int64_t period = 2 * c->rebuild_every, skip = ((left - 1) / period - 1) * period;
                if (skip > 0) { s.slot += skip; left -= skip; c->n_rebins += 2 * (skip / period); }
            }
            track_step(c);
            --left;
        }
        c->have_step_outputs = true;
    }
    set_epoch(c);
}

// Sort n particles into cell order without a clock (context creation, forced re-binnings, realignments of batch members):
// histogram of the positions `pos`, scan into `start`, scatter, and the gather `ra` into that order.  Not timed.
void host_rebin(sphx_ctx *c, int n, const double2 *pos, int *cellid, int *count, int *start, int *perm, const ReorderArgs &ra)
{
    if (n <= 0) {
        SPHX_HIP(hipMemsetAsync(start, 0, ((size_t)c->grid.ncells + 1) * sizeof(int), c->stream));
        return;
    }
    // (a folded re-binning step leaves its histogram for the next cell sweep to clear: the batch may have ended in between)
    if (c->fold_rebin && count == c->count.get()) SPHX_HIP(hipMemsetAsync(count, 0, ((size_t)c->grid.ncells + 1) * sizeof(int), c->stream));
    const bool prof = c->profiling;
    c->profiling = false;
    const dim3 g1(div_up(n, kBlock)), bp(kBlock);
    launch(c, "k_bin", k_bin, g1, bp, (const Clock *)nullptr, 0, c->grid, n, pos, cellid, count);
    launch_cell_scan(c, nullptr, 0, count, start);
    launch(c, "k_scatter", k_scatter, g1, bp, (const Clock *)nullptr, 0, n, (const int *)cellid, count, (const int *)start, perm);
    launch(c, "k_reorder", k_reorder, g1, bp, (const Clock *)nullptr, 0, n, (const int *)cellid, (const int *)start,
           (const int *)perm, ra);
    c->profiling = prof;
    SPHX_HIP(hipGetLastError());
}

// Re-bin the current state into the other buffers without taking a step: the device stopped the loop because
// some particle drifted further than skin/2 from where it was binned.  Happens only when the flow is faster than
// the skin was sized for; a cool-down follows (Schedule::cool_down).
void forced_rebuild(sphx_ctx *c)
{
    const int q = c->sched.cur, l = c->sched.lay;
    if (c->have_step_outputs && c->out_lay != l)
        throw Error(SPHX_ERR_STATE, "SPHX:Ctx:rebuild", "internal: forced rebuild straight after a rebuild step");
    const FluidSet s = c->view(q, l), d = c->view(1 - q, 1 - l);
    // src_of: new slot -> slot of the layout the last step's outputs (rho, p, force, Vol, B) are stored in
    host_rebin(c, c->h_clock->n, s.pos, c->cellid.get(), c->count.get(), d.start, c->perm.get(),
               reorder_args(s.pos, s.vel, s.drho, s.mass, s.id, d, c->tmp.src_of));
    hipLaunchKernelGGL(k_rebinned, dim3(1), dim3(1), 0, c->stream, c->clock.get());
    SPHX_HIP(hipGetLastError());
    c->sched.cur = 1 - q; c->sched.lay = 1 - l; c->sched.pos = 0;  // out_lay stays l
    c->h_clock->need_rebuild = 0;
    c->h_clock->drift = 0.0;
    if (c->h_pub) { c->h_pub->need_rebuild = 0; c->h_pub->drift = 0.0; }  // (the published copy may be read again before the next batch)
    const int64_t now = c->h_clock->step;
    c->sched.cool_down(now, c->rebuild_every);
    if (debug_switches().log)
        fprintf(stderr, "sphx: forced rebuild #%lld at step %lld (drift bound hit): re-binning every step for %lld steps\n",
                (long long)c->sched.n_forced, (long long)now, (long long)c->sched.cool_len);
    c->last_forced_step = now;
    set_epoch(c);
}

void fill_status(sphx_ctx *c, sphx_status *st)
{
    if (!st) return;
    const Clock &k = *c->h_clock;
    st->t = k.t;
    st->dt_last = k.dt_last;
    st->dt_next = k.dt;
    st->vmax = k.vmax;
    st->step = k.step;
    st->done = (k.t < k.t_target - 1e-12) ? 0 : 1;
    st->device_status = k.status;
}

int pick_lpp(int nf)
{
    // enough lanes to put ~4 waves on each of the 1024 SIMDs; 4..32 lanes per particle (measured: with the
    // balanced neighbour list 4 lanes beat 1-2 even at 6 M particles, 32 beat 16 at 5 k)
    // Round 2 (entries ahead, LDS tile in the force pass): 2 lanes beat 4 from 0.5 M particles (189 vs 193 us/step) and
    // clearly at 6 M (2195 vs 2416); at 65 k particles 4 lanes keep more waves in flight (51 vs 60 us/step).
    // With pass E and the next pass A in one launch and the clock in its tail (up to 2048 workgroups: 131 k particles at
    // 4 lanes, 262 k at 2) the three-launch step of 2 lanes beats the five launches of 4: 194 k particles 90.9 vs 96.4 us/step,
    // 259 k 109.1 vs 117.4; at 130 k, where both fuse, 4 lanes win (68.0 vs 70.6).
    // Round 3 (the fused launch now reaches 4 096 workgroups = 262 k particles at 4 lanes): both lane counts fused, 4 lanes win
    // at 151 k (76.4 vs 79.8) and 194 k (89.9 vs 90.9), 2 lanes from 259 k (110.2 vs 110.8) -> the switch moves to 220 k.
    const long target = 256L * 4 * 4 * 64;
    if (nf > 220000) return 2;
    int lpp = 4;
    while (lpp < 32 && (long)nf * lpp * 2 <= target) lpp *= 2;
    // Round 3, compact kernels with passes E and A in one launch: 32 lanes win at 1 875 fluid particles (16.1 vs 17.2 us/step),
    // tie at 2 494, and lose from 3 300 (18.1 vs 17.5; C2 = 4 800: 19.9 vs 19.3; 5 852: 20.9 vs 19.7) -- profiles/r03_lanes_small.txt
    if (lpp == 32 && nf > 2400) lpp = 16;
    return lpp;
}

// Threads per workgroup of the compact passes (k_kgc, k_forces, k_continuity_density, k_continuity_compact, k_density_walk).
// A pass of 256-thread workgroups gets slower by 1.3 us/step where it stops fitting one workgroup per compute unit (256 of
// them: 243 workgroups 12.0 us/step, 257 workgroups 13.3).  Smaller workgroups do not help -- every workgroup costs dispatch
// time: C2 at 128 threads +0.1..0.5, at 64 +1.4 us/step -- and neither do 150 workgroups of 512 threads (+0.7: eight waves on
// every compute unit that has any).  What helps is the smallest workgroup with which the pass fits the 256 compute units
// again, where that is one wave more: C2's 1 200 waves as 240 workgroups of 320 threads, 13.51 against 13.94 us/step; six
// waves (384 threads, 200 workgroups) are back at 14.03.  profiles/r44_block_size.txt.
// Only the three-launch step with the folded re-binning (fold_rebin, ctx_alloc checks that it agrees): its re-binning kernels
// keep 256 threads and per-workgroup maxima of their own (pass_tmp).  Batches, slabs, dynamic contexts: 256.
// (called from ctx_alloc, with tail_clock decided)
int pick_block(const sphx_ctx *c)
{
    const DebugSwitches &dbg = debug_switches();
    const Grid &g = c->grid;
    const bool three_launches = c->tail_clock && c->lpp >= 16 && !c->arena && !dbg.no_fuse_ea && !dbg.no_fold_rebin &&
                                dual_rate_substeps(c->prm) == 1 && g.periodic && g.ncx >= 3 && g.ncells < kFoldCells &&
                                g.ncells <= kBigScanCells && 5 * (size_t)c->n_blocks_particles <= (size_t)(4 * kMaxTile);
    if (!three_launches) return kBlock;
    if (dbg.block > 0) return dbg.block;
    // (taken where it is worth 2 %: C2, 1 200 waves, -2.8 % and -4.4 % on the 20-step line; at 1 083 waves it is 1.3 %, so not
    //  there, and nothing in between has been measured: the class begins half-way)
    const size_t waves = div_up((size_t)c->cap * c->lpp, (size_t)64);
    return (waves > 4 * 256 + 128 && waves <= 5 * 256) ? 320 : kBlock;
}

// rows of the per-lane neighbour list: >= 96 entries per particle (fluid ring ~30-45 + wall ring up to ~20)
int nl_cap_for(int lpp) { return std::max(96 / lpp, 16); }

Phys make_phys(const sphx_params *prm)
{
    Phys ph{};
    ph.kc = make_kernel_const(prm->h);
    ph.rho0 = prm->rho0; ph.inv_sigma0 = prm->inv_sigma0; ph.mu = prm->mu; ph.p0 = prm->p0; ph.c_f = prm->c_f;
    ph.g = prm->gravity_g; ph.tc = prm->transport_coeff; ph.nu = prm->mu / prm->rho0; ph.DL = prm->DL; ph.DH = prm->DH;
    ph.w0 = ph.kc.sigma;
    ph.dt_viscous = 0.125 * prm->h * prm->h / std::max(ph.nu, 1e-12);
    ph.dt_body = 0.25 * std::sqrt(prm->h / std::max(std::fabs(ph.g), 1e-12));
    return ph;
}

}  // namespace

namespace sphx {
// The device arrays of the members of a batch: array X of member m is block m of one allocation of n_members blocks, so that
// a "_b" kernel reaches every member's X from member 0's pointer (Members, sphx_kernels.hpp).  Keyed by where the DevBuf sits
// in sphx_ctx -- every member asks for the same arrays in the same sizes.
struct BatchArena {
    int n_members = 1;
    struct Block {
        DevBuf<char> mem;
        size_t bytes = 0;  // per member
    };
    std::map<size_t, Block> blocks;
};
}  // namespace sphx

namespace {

template <typename T>
void dev_alloc(sphx_ctx *c, DevBuf<T> &b, size_t n)
{
    if (!c->arena) {
        b.alloc(n);
        return;
    }
    BatchArena::Block &blk = c->arena->blocks[(size_t)(reinterpret_cast<char *>(&b) - reinterpret_cast<char *>(c))];
    const size_t bytes = n * sizeof(T);
    if (!blk.mem.get() && bytes) {
        blk.mem.alloc(bytes * (size_t)c->arena->n_members);
        blk.bytes = bytes;
    }
    if (blk.bytes != bytes) throw Error(SPHX_ERR_STATE, "SPHX:Batch:internal", "members ask for arrays of different sizes");
    b.alias(bytes ? reinterpret_cast<T *>(blk.mem.get() + bytes * (size_t)c->member) : nullptr, n);
}

// allocate every device array for `cap` particles and the grid of the context
void ctx_alloc(sphx_ctx *c, int cap)
{
    const Grid &g = c->grid;
    c->cap = cap;
    c->n_blocks_particles = (int)div_up((size_t)cap * c->lpp, kBlock);
    c->n_blocks_flat = (int)div_up((size_t)cap, kBlock);
    for (int k = 0; k < 2; ++k) {
        dev_alloc(c, c->fpos_[k], cap); dev_alloc(c, c->fvel_[k], cap); dev_alloc(c, c->fdrho_[k], cap); dev_alloc(c, c->fmass_[k], cap);
        dev_alloc(c, c->fid_[k], cap); dev_alloc(c, c->fstart_[k], (size_t)g.ncells + 1); dev_alloc(c, c->fcell_[k], cap);
        if (c->skin > 0.0) dev_alloc(c, c->fposb_[k], cap);
    }
    dev_alloc(c, c->posn, cap); dev_alloc(c, c->veln, cap); dev_alloc(c, c->ffp, cap); dev_alloc(c, c->ff, cap); dev_alloc(c, c->fa, cap); dev_alloc(c, c->fB, cap);
    dev_alloc(c, c->drhon, cap); dev_alloc(c, c->rho_out, cap); dev_alloc(c, c->p_out, cap); dev_alloc(c, c->fvol, cap); c->fvol.zero(c->stream);
    c->posn.zero(c->stream); c->veln.zero(c->stream); c->ffp.zero(c->stream); c->ff.zero(c->stream);
    c->fa.zero(c->stream); c->fB.zero(c->stream); c->drhon.zero(c->stream); c->rho_out.zero(c->stream); c->p_out.zero(c->stream);
    // Small channels with a skin: move steps are 4 launches, the clock update rides in pass E (continuity_tail);
    // vpart entries then double as "ready" flags and start out empty (all ones)
    c->tail_clock = c->skin > 0.0 && !c->is_slab && !c->dyn && c->n_blocks_particles <= tail_clock_limit() && !debug_switches().no_tail_clock;
    c->block = pick_block(c);
    c->n_blocks_pass = (int)div_up((size_t)cap * c->lpp, (size_t)c->block);
    // vpart / dpart: one entry per workgroup.  Passes of another size than 256 threads keep theirs behind those of the 256-thread
    // kernels (pass_tmp): whichever kernels run a step, its tail workgroup collects what the same step's workgroups left
    c->n_vpart = c->n_blocks_particles + (c->block != kBlock ? c->n_blocks_pass : 0);
    dev_alloc(c, c->vpart, c->n_vpart);
    // (skinned slabs: the same hand-over feeds slab_seal_tail)
    const bool vpart_flags = c->tail_clock || (c->is_slab && c->rebuild_every > 1);
    SPHX_HIP(hipMemsetAsync(c->vpart.get(), vpart_flags ? 0xFF : 0, (size_t)c->n_vpart * sizeof(double), c->stream));
    dev_alloc(c, c->dpart, c->n_vpart);
    c->dpart.zero(c->stream);
    c->n_vtiles = (!c->is_slab && c->n_vpart > 4 * kMaxTile) ? (int)div_up((size_t)c->n_vpart, kMaxTile) : 0;
    if (c->n_vtiles) dev_alloc(c, c->vtile, 2 * (size_t)c->n_vtiles);
    dev_alloc(c, c->cellid, cap); dev_alloc(c, c->count, (size_t)g.ncells + 1); dev_alloc(c, c->perm, cap); dev_alloc(c, c->src_of, cap);
    c->count.zero(c->stream);
    const int nl_cap = nl_cap_for(c->lpp);
    // one list column per launched lane, of the 256-thread kernels and of the passes at the context's block size
    const size_t stride = std::max((size_t)c->n_blocks_particles * kBlock, (size_t)c->n_blocks_pass * c->block);
    dev_alloc(c, c->nl_idx, stride * nl_cap);
    dev_alloc(c, c->nl_cnt, stride);
    c->nl_cnt.zero(c->stream);
    const size_t nl_words = (size_t)(nl_cap + 1) / 2;  // two 16-bit rows per word
    if (c->walk_kernels) { dev_alloc(c, c->nl_pk, stride * std::max<size_t>(nl_words, 2)); c->nl_pk.zero(c->stream); }
    const int sl_cap = c->skin > 0.0 ? (3 * nl_cap + 1) / 2 : 0;
    if (sl_cap) {
        dev_alloc(c, c->sl_idx, stride * sl_cap);
        dev_alloc(c, c->sl_cnt, stride);
        c->sl_cnt.zero(c->stream);
        if (c->walk_kernels) { dev_alloc(c, c->sl_pk, stride * std::max<size_t>((size_t)(sl_cap + 1) / 2, 4)); c->sl_pk.zero(c->stream); }
    }
    const double sl_r = 2.0 * c->prm.h + c->skin;
    dev_alloc(c, c->flags, 1);
    c->flags.zero(c->stream);
    c->big_scan = g.ncells > kBigScanCells;
    c->n_tiles = (int)div_up((size_t)g.ncells, kScanBlock);
    dev_alloc(c, c->tile, 2 * ((size_t)c->n_tiles + 1));
    c->tmp = FluidTmp{c->posn.get(), c->veln.get(), c->drhon.get(), c->fa.get(), c->fB.get(), c->ffp.get(), c->ff.get(),
                      c->rho_out.get(), c->p_out.get(), c->cellid.get(), c->count.get(), c->perm.get(), c->src_of.get(),
                      c->vpart.get(), c->dpart.get(), c->nl_idx.get(), c->nl_cnt.get(), c->flags.get(), c->tile.get(),
                      (int)stride, nl_cap, c->sl_idx.get(), c->sl_cnt.get(), sl_cap, sl_r * sl_r, cap, c->n_vpart,
                      c->skin > 0.0 ? c->half_skin() : -1.0, c->fvol.get(), c->nl_pk.get(), c->sl_pk.get(), c->is_slab ? 1 : 0, nullptr, 0, nullptr};
    // (2 = never: a slab hands out its state only, sphx_slab_snapshot; the dual-rate loop, which reads force_prior in its
    //  inner sub-steps, runs on the compact kernels only)
    c->tmp.n_vpart = c->n_blocks_particles;  // (the entries of the 256-thread kernels; pass_tmp for the others)
    c->tmp.lazy_out = (c->walk_kernels && !debug_switches().no_lazy_out) ? (c->is_slab ? 2 : 1) : 0;
    if (c->walk_kernels) {  // (zeros = empty layouts until the first cell sweep has run)
        dev_alloc(c, c->tmap, 8 * (size_t)c->n_blocks_particles); c->tmap.zero(c->stream);
        c->tmp.tmap = c->tmap.get();
    }
    // E|A fusion: small static-schedule channels on the compact kernels (the clock rides in the tail workgroup)
    c->fuse_ea = c->tail_clock && (c->lpp >= 16 || (c->walk_kernels && !c->lds_tiles_be && c->lpp >= 2)) && !debug_switches().no_fuse_ea;
    c->tmp_par[0] = c->tmp;
    c->tmp_par[1] = c->tmp;
    if (c->fuse_ea) {
        dev_alloc(c, c->fa2, cap); dev_alloc(c, c->fvol2, cap); c->fa2.zero(c->stream); c->fvol2.zero(c->stream);
        dev_alloc(c, c->nl_idx2, stride * nl_cap); dev_alloc(c, c->nl_cnt2, stride); c->nl_cnt2.zero(c->stream);
        c->tmp_par[1].a = c->fa2.get(); c->tmp_par[1].vol = c->fvol2.get();
        c->tmp_par[1].nl_idx = c->nl_idx2.get(); c->tmp_par[1].nl_cnt = c->nl_cnt2.get();
        if (c->walk_kernels) {
            dev_alloc(c, c->nl_pk2, stride * std::max<size_t>(nl_words, 2)); c->nl_pk2.zero(c->stream);
            c->tmp_par[1].nl_pk = c->nl_pk2.get();
        }
    }
    // Opt-in dual-rate loop (sphx_params::dual_rate): small channels on the compact kernels, where the fused launches give
    // the step a fixed shape.  The number of inner sub-steps is fixed per context (the graphs are static): how many acoustic
    // steps fit into the viscous / body-force step, at most dual_rate.  Fine channels are viscous-limited: n_in = 1 there.
    c->n_in = (c->fuse_ea && c->lpp >= 16) ? dual_rate_substeps(c->prm) : 1;
    if (c->n_in > 1) { dev_alloc(c, c->vel2, cap); c->vel2.zero(c->stream); }
    // Folded re-binning step: the compact kernels with the fused E|A launch, single-rate, a periodic grid of at least three
    // columns (the +-1 columns of a cell are distinct) small enough for every workgroup to scan in LDS (kFoldCells)
    c->fold_rebin = c->fuse_ea && c->lpp >= 16 && c->n_in == 1 && !c->arena && !c->big_scan && c->n_vtiles == 0 &&
                    g.periodic && g.ncx >= 3 && g.ncells < kFoldCells && !debug_switches().no_fold_rebin;
    if (c->block != kBlock && !c->fold_rebin)
        throw Error(SPHX_ERR_STATE, "SPHX:Ctx:block", "internal: a block size other than 256 without the folded re-binning step");

    dev_alloc(c, c->tau_part, (size_t)2 * c->n_blocks_flat);
    dev_alloc(c, c->tau_out, 2);
}

// upload n fluid particles (host SoA) and sort them into state 0 / layout 0
void upload_fluid(sphx_ctx *c, int n, const double *hx, const double *hy, const double *hvx, const double *hvy,
                  const double *hdrho, const double *hmass, const int *hid, bool wrap)
{
    hipStream_t s = c->stream;
    std::vector<double2> hp((size_t)std::max(n, 1)), hv((size_t)std::max(n, 1));
    for (int i = 0; i < n; ++i) { hp[i] = make_double2(hx[i], hy[i]); hv[i] = make_double2(hvx[i], hvy[i]); }
    if (n > 0) {
        c->posn.upload(hp.data(), n, s); c->veln.upload(hv.data(), n, s);
        c->drhon.upload(hdrho, n, s);
        c->fmass_[1].upload(hmass, n, s);
        if (hid) c->fid_[1].upload(hid, n, s);
        else hipLaunchKernelGGL(k_iota, dim3(div_up(n, kBlock)), dim3(kBlock), 0, s, n, c->fid_[1].get(), 0);
        if (wrap) hipLaunchKernelGGL(k_wrap_x, dim3(div_up(n, kBlock)), dim3(kBlock), 0, s, n, c->posn.get(), c->prm.DL);
    }
    const FluidSet d = c->view(0, 0);
    host_rebin(c, n, c->posn.get(), c->cellid.get(), c->count.get(), d.start, c->perm.get(),
               reorder_args(c->posn.get(), c->veln.get(), c->drhon.get(), c->fmass_[1].get(), c->fid_[1].get(), d, nullptr));
    SPHX_HIP(hipStreamSynchronize(s));  // host staging vectors die after this
}

// upload nw wall particles (host SoA, x already in this context's frame) and sort them once
void upload_walls(sphx_ctx *c, int nw, const double *hx, const double *hy, const double *hmass, const double *hvx,
                  const double *hvy, const int *hid, bool wrap)
{
    const Grid &g = c->grid;
    hipStream_t s = c->stream;
    const size_t nwz = nw > 0 ? (size_t)nw : 1;
    c->wpos.alloc(nwz); c->wa.alloc(nwz); c->wid.alloc(nwz);
    c->wstart.alloc((size_t)g.ncells + 1); c->wrow_any.alloc(g.ncy);
    DevBuf<double2> tpos(nwz);
    DevBuf<double4> ta(nwz);
    DevBuf<int> tid(nwz), tcell(nwz), tperm(nwz), tcount((size_t)g.ncells + 1);
    tcount.zero(s);
    std::vector<double2> hp(nwz);
    std::vector<double4> ha(nwz);
    for (int i = 0; i < nw; ++i) {
        hp[i] = make_double2(hx[i], hy[i]);
        ha[i] = make_double4(hmass[i] / c->prm.rho0, hvx[i], hvy[i], 0.0);  // walls keep rho = rho0 (sph_physics_mex.c:214-216,233)
    }
    if (nw > 0) {
        tpos.upload(hp.data(), nw, s); ta.upload(ha.data(), nw, s); tid.upload(hid, nw, s);
        if (wrap) hipLaunchKernelGGL(k_wrap_x, dim3(div_up(nw, kBlock)), dim3(kBlock), 0, s, nw, tpos.get(), c->prm.DL);
    }
    ReorderArgs ra{};
    ra.n2 = 1; ra.src2[0] = tpos.get(); ra.dst2[0] = c->wpos.get();
    ra.n4 = 1; ra.src4[0] = ta.get(); ra.dst4[0] = c->wa.get();
    ra.id_src = tid.get(); ra.id_dst = c->wid.get(); ra.src_of = nullptr; ra.cell_dst = nullptr;
    host_rebin(c, nw, tpos.get(), tcell.get(), tcount.get(), c->wstart.get(), tperm.get(), ra);
    hipLaunchKernelGGL(k_row_any, dim3(div_up(g.ncy, 64)), dim3(64), 0, s, g, (const int *)c->wstart.get(), c->wrow_any.get());
    SPHX_HIP(hipGetLastError());
    SPHX_HIP(hipStreamSynchronize(s));  // temporaries die here
    c->walls = Walls{c->wpos.get(), c->wa.get(), c->wid.get(), c->wstart.get(), c->wrow_any.get(), nw};
}

void init_clock(sphx_ctx *c, int n, double t0, int64_t step0)
{
    hipStream_t s = c->stream;
    dev_alloc(c, c->clock, 1);
    Clock k{};
    k.t = t0; k.dt = 0.0; k.dt_last = 0.0; k.t_target = t0; k.t_end = c->prm.t_end; k.vmax = 0.0;
    k.step = step0; k.steps_left = -1; k.run[0] = 0; k.run[1] = 0; k.status = 0; k.n = n;
    k.drift = 0.0; k.need_rebuild = 0;
    k.fresh = 1; k.rebuild_now = 0; k.pos_count = 0; k.n_drift_rebuilds = 0;
    k.seq = 0;
    k.n_in = c->n_in;
    if (!c->h_pub) SPHX_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->h_pub), sizeof(Clock), hipHostMallocMapped));
    void *pub_dev = nullptr;
    SPHX_HIP(hipHostGetDevicePointer(&pub_dev, c->h_pub, 0));
    k.pub = static_cast<Clock *>(pub_dev);
    *c->h_pub = k;
    c->h_pub->seq = -1;  // nothing published yet
    c->host_seq = 0;
    *c->h_clock = k;
    SPHX_HIP(hipMemcpyAsync(c->clock.get(), c->h_clock, sizeof(Clock), hipMemcpyHostToDevice, s));
    SPHX_HIP(hipStreamSynchronize(s));
    hipLaunchKernelGGL(k_vmax_init, dim3(1), dim3(kScanBlock), 0, s, c->clock.get(), c->grid, (const double2 *)c->fpos_[0].get(),
                       (const double2 *)c->fvel_[0].get(), (double *)nullptr);
    SPHX_HIP(hipGetLastError());
    c->sched.cur = 0; c->sched.lay = 0; c->sched.pos = 0; c->out_lay = 0;
    set_epoch(c);
    c->pending_target = step0;
}

void common_checks(const sphx_params *prm, int n_fluid, int n_total)
{
    require(prm != nullptr, "SPHX:Ctx:params", "params must not be NULL");
    require(prm->dual_rate >= 0 && prm->dual_rate <= 4, "SPHX:Ctx:dual_rate",
            "dual_rate must be 0, 1 or 2..4 (inner sub-steps per outer step)");
    require(n_total > 0 && n_fluid > 0 && n_fluid <= n_total, "SPH:Neighbor:count",
            "Invalid n_fluid/n_total or inconsistent pos size.");
    require(prm->h > 0.0 && prm->DL > 0.0, "SPH:Neighbor:param", "h and DL must be positive.");
}

void y_extent(const double *py, int n_total, double &y_min, double &y_max)
{
    y_min = py[0]; y_max = py[0];
    for (int i = 1; i < n_total; ++i) { y_min = std::min(y_min, py[i]); y_max = std::max(y_max, py[i]); }
    require(std::isfinite(y_min) && std::isfinite(y_max), "SPH:Neighbor:pos", "pos must be finite.");
}

// Which kernel forms the context runs, once lanes per particle and the grid are known.  Up to 8 lanes per particle: the
// large-channel ("_w") forms, whose lists hold fluid neighbours as 16-bit index differences -- a neighbour sits at most one
// cell column (+ a few cells) away, so a column must hold well under 2^15 particles; a grid with taller columns (a channel
// thousands of particles high) goes to 16 lanes per particle and the compact kernels instead.
void choose_kernel_forms(sphx_ctx *c, bool lpp_given, double column_load, int n_resident)
{
    if (c->lpp <= 8 && 1.3 * column_load + 64.0 > (double)kDeltaMax) {
        if (lpp_given)
            throw Error(SPHX_ERR_ARG, "SPHX:Ctx:lpp", "cell columns too populous for the 16-bit neighbour lists of the "
                                                      "large-channel kernels: use lanes_per_particle >= 16 (or 0 = auto)");
        c->lpp = 16;
    }
    const DebugSwitches &dbg = debug_switches();
    c->walk_kernels = c->lpp <= 8;
    c->sweep_kernels = c->walk_kernels;
    c->lds_tiles = c->walk_kernels && !dbg.no_lds_tiles;  // (65 k particles: 46.8 with, 46.3 us/step without;
    // 100-130 k: equal; 194 k: 96.4 / 97.1; 259 k: 117.3 / 119.5; 360 k: 145.8 / 151.0 -- kept on at every size)
    // (round 3, layouts stored + slot-coded lists: 0.5 M 164 without / 175 us/step with -- it gives up the fused E|A launch --,
    //  0.83 M 260 / 260, 1.3 M 430 / 420; before that: 270 / 285 at 0.83 M, 440 / 457 at 1.3 M, hence 2 M then)
    //  A slab has no fused launch to give up: in-process rings of 0.51 M / 0.76 M-particle slabs run 5 % / 9 % faster with the
    //  tiles (C5 as 12 / 8 slabs: 2 970 -> 2 821, 2 546 -> 2 323 us/step), 0.25 M-particle slabs do not (276 / 279); a single
    //  context of 0.76 M particles is a tie (239.5 / 239.8).
    //  Round 4 (walks that do not look at the entry, two-slot staging): a single context takes the tiles from where the fused
    //  E|A launch ends (4096 workgroups per pass = 524 k particles at 2 lanes each) -- 0.59 M particles 189 / 198 -> 181 / 186
    //  us/step (window / sustained), 0.79 M 242 / 257 -> 231 / 240; below, the fused launch is worth more: 0.52 M 165 / 172
    //  fused against 170 / 176 with tiles (profiles/r04_tiles_from_*.txt).  It was 10^6 before.
    //  Slabs: from 0.3 M particles held (0.5 M before): C5 as 16 slabs of 0.39 M 3 539 -> 3 221 us/step in an in-process ring,
    //  slabs of 0.24 M 290 / 290 (profiles/r04_slab_tiles_from.txt).
    const bool fits_fused = div_up((size_t)std::max(n_resident, 0) * (size_t)c->lpp, (size_t)kBlock) <= (size_t)tail_clock_limit();
    const int tiles_from = dbg.tiles_be_from > 0 ? dbg.tiles_be_from : (c->is_slab ? 300000 : (fits_fused ? 1000000 : 0));
    c->lds_tiles_be = c->lds_tiles && c->lpp <= 2 && n_resident >= tiles_from;
    c->lds_tiles_a = c->lds_tiles_be;  // (6 M particles: 450 with, 478 us without; 0.5 M: 50.5 with, 42.3 without)
    // every pass stages the same layout: the lists can name its slots (kSlotCodes) -- the index differences that remain need a
    // little more room than the plain ones
    static_assert(tile_slots(2) == kSlotCodes, "the layout the lists are coded against is the tile of passes A, B and E");
    c->coded_lists = c->lds_tiles_be && c->lpp == 2 && 1.3 * column_load + 64.0 <= (double)kCodedDeltaMax && !dbg.no_coded_lists;
}

void check_lpp(int lpp)
{
    require(lpp == 1 || lpp == 2 || lpp == 4 || lpp == 8 || lpp == 16 || lpp == 32, "SPHX:Ctx:lpp",
            "lanes_per_particle must be 1,2,4,8,16 or 32");
}

// what a context decides from its parameters and the particle extent, before the device is touched: lanes per particle,
// re-binning interval and skin, cell grid, kernel forms
void ctx_configure(sphx_ctx *c, const sphx_params *prm, int n_fluid, int n_total, const double *pos)
{
    c->prm = *prm;
    c->nf = n_fluid;
    c->nt = n_total;
    c->nw = n_total - n_fluid;
    const int nf = c->nf;
    const double *py = pos + (size_t)n_total;

    c->lpp = prm->lanes_per_particle > 0 ? prm->lanes_per_particle : pick_lpp(nf);
    check_lpp(c->lpp);
    c->spg = prm->steps_per_graph > 0 ? prm->steps_per_graph : 40;  // measured at C2: 10 -> 25.4, 40 -> 25.1, 80 -> 24.8 us/step
    if (c->spg & 1) c->spg += 1;

    // Rebuild interval K and the cell skin that pays for it.  One step moves a particle by at most
    // dt*v <= 0.25 h v/(c_f+v); the reference sets c_f = 10 U_max, so v/c_f stays near 0.1-0.15 (0.033 h per
    // step; measured 0.017 h at c_f = 15) plus transport shifts of single particles (up to ~0.09 h measured):
    // the skin covers K-1 steps of 0.035 h.  If a flow outruns it the device clock stops the loop and
    // forced_rebuild() takes over, so this is a speed heuristic, never a correctness assumption.
    // Measured (MI355X, us/step, K=1 -> K=5): 4.8 k particles 47.5 -> 37.5 (launch-bound: 7 -> 5 launches per
    // step), 60 k 93.9 -> 80.2, 0.5 M 343 -> 316, 6 M 4101 -> 3907 (the wider cells lengthen the candidate sweeps
    // by ~10 %, the scatter/reorder kernels run on every fifth step only).
    // With the superset list: K = 5 / 8 / 10 give 24.9 / 24.3 / 24.1 us/step at 5 k particles (fewer rebuild
    // launches per step) but 2443 / 2490 / 2488 at 6 M (longer superset lists) -> 8 for small channels, 5 otherwise.
    // Round 2 (pass E and the next pass A share a launch: a step is 3 launches, a re-binning step 6): 5 k particles,
    // K = 8 / 12 / 16 / 24 / 32 -> 21.1 / 19.95 / 19.6 / 19.6 / 19.4 us/step, the 20 s run's L2 0.85 / 0.85 / 0.80 / 0.90 % -> 16.
    // 20 k - 250 k particles, K = 5 / 8 / 12 / 16: 28.8 / 27.6 / 27.1 / 27.8 us/step at 21 k, 49.8 / 48.7 / 49.1 / 49.4 at 65 k,
    // 79.5 / 72.1 / 72.6 / 74.8 at 130 k, 142 / 118 / 119 / 121 at 250 k (K = 5: its thin skin forces rebuilds + cool-downs) -> 8;
    // 0.5 M: 189 / 192 at K = 5 / 8, 6 M: 2 201 / 2 262 -> 5.
    // Round 4: the interval and the skin are two things (profiles/r04_k_skin_*.txt).  The skin prices EVERY step (the superset
    // list grows with it: 1.30 x the neighbours at 0.28 h, 1.55 x at 0.49 h) and, with the drift check, is all that correctness
    // needs; K only says when a re-binning is taken whether or not the drift asks for one.  Where the device re-bins by itself
    // (from 10^6 particles) a late scheduled re-binning costs nothing -- the drift bound comes first -- so the skin stays that
    // of K = 5 and K goes up: C5 1 632 -> 1 507 us/step in bench.py's window at K = 12, 1 723 -> 1 598 sustained (K = 12 with
    // 0.31 h: 1 514 / 1 603); on another box K = 12 / 16 / 24 / 64: 1 550 / 1 523 / 1 503 / 1 493 in the window, 1 645 sustained for
    // all four (the drift bound decides there) -> 24.  1.25 M particles 384 -> 354 / 413 -> 401.  On the host-driven schedule a
    // drift stop is a round trip and a cool-down, so the skin has to grow with K: 0.3-2 M particles K = 10 with 0.42 h (C4 160 ->
    // 157 in the window, 170 -> 164 sustained, one forced re-binning in 3 000 steps; K = 8 with 0.28 h: 17 of them, 263 us/step).
    // Up to 20 k particles K = 16 stays: K = 24 on the same skin (1.05 h) is 3 % faster on the bench's flow (C2 17.4 -> 16.8
    // us/step, C1 14.2 -> 13.7, no forced re-binning in 12 000 developed steps) but a flow AT the reference's U_max drifts
    // 0.023 h a step -- 23 steps of that are the whole half-skin, and tests/test_gpu_headline_parity.py's state forced 16
    // re-binnings in 50 steps with it (K = 32: 86 in the bench's own flow, 50 us/step); 20 k - 300 k stays at 8 (every other
    // pair measured slower there: profiles/r04_k_skin_c3.txt, _194k.txt).
    // Who re-bins: the device by itself from 2 x 10^6 particles (round 4; 10^6 before the wider skins).  Measured with K = 10 /
    // 0.42 h on the host's schedule against K = 24 / 0.28 h on the device's (window / sustained us/step, profiles/
    // r04_static_vs_dyn_*.txt): 1.25 M particles 338 / 353 against 337-340 / 381-384, 2.5 M 664 / 685 against 636 / 705,
    // 6 M 1 526 / 1 564 against 1 407 / 1 542 -- the self-skipping launches of a device-decided step are 7 % of a step at
    // 1.25 M and 1.7 % at 6 M, the thin skin's shorter lists are worth more the longer the passes.
    const bool dyn_wanted = prm->dynamic_rebin == 1 || (prm->dynamic_rebin == 0 && nf >= 2000000);
    const bool auto_policy = prm->rebuild_every <= 0 && prm->skin_h <= 0.0;
    int K = prm->rebuild_every > 0 ? std::min(prm->rebuild_every, 64) : (nf <= 20000 ? 16 : (nf <= 300000 ? 8 : (dyn_wanted ? 24 : 10)));
    // dual-rate loop: a slot moves particles n_sub times as far.  Same eligibility as ctx_alloc's n_in (the fused E|A launch
    // with the clock in its tail workgroup: a skin, static schedule, <= 2048 workgroups, compact kernels)
    const bool dual_ok = c->lpp >= 16 && !c->is_slab && K > 1 && prm->dynamic_rebin != 1 &&
                         div_up((size_t)nf * c->lpp, kBlock) <= (size_t)tail_clock_limit() && !debug_switches().no_tail_clock && !debug_switches().no_fuse_ea;
    const int n_sub = dual_ok ? dual_rate_substeps(*prm) : 1;
    if (n_sub > 1 && prm->rebuild_every <= 0) K = std::max(2, K / n_sub);
    const double d_step = 0.035 * prm->h * n_sub;
    double skin = K > 1 ? (prm->skin_h > 0.0 ? prm->skin_h * prm->h : 2.0 * std::max((K - 1) * d_step, 0.1 * prm->h)) : 0.0;
    if (auto_policy && nf > 300000 && K > 1) skin = (dyn_wanted ? 0.28 : 0.42) * prm->h;  // (see above: not the skin of this K)
    if (K > 1 && (int)std::floor(prm->DL / (2.0 * prm->h + skin)) < 3) { K = 1; skin = 0.0; }
    c->rebuild_every = K;
    c->skin = skin;
    // Dynamic re-binning pays where a handful of empty launches per step is noise next to the passes (measured: the
    // host-driven forced rebuilds + cool-downs cost 10-25 % of the sustained rate from 0.5 M particles up).
    // dynamic_rebin: 0 = by size, 1 = on, 2 = off.
    c->dyn = skin > 0.0 && dyn_wanted;

    // grid: exact periodic tiling in x (cells >= 2h + skin), rows of 2h + skin in y over fluid + wall extent
    double y_min, y_max;
    y_extent(py, n_total, y_min, y_max);
    const double cs = 2.0 * prm->h + skin;
    Grid g{};
    // Any DL > 0 (the reference's grid is ceil(DL/2h) >= 1 columns plus ghost entries, neighbor.c:253-296): below three
    // columns the sweeps visit each distinct column once (duplicate_column) and the fold picks the nearest image.
    g.ncx = std::max(1, (int)std::floor(prm->DL / cs));
    g.ncy = (int)std::ceil((y_max - y_min + 1e-12) / cs) + 1;
    require((double)g.ncx * (double)g.ncy < 2.0e9, "SPH:Neighbor:param", "cell grid too large.");
    g.ncells = g.ncx * g.ncy;
    g.periodic = 1;
    g.DL = prm->DL;
    g.half_DL = 0.5 * prm->DL;
    g.x0 = 0.0;
    g.y0 = y_min;
    g.inv_csx = (double)g.ncx / prm->DL;
    g.inv_csy = 1.0 / cs;
    g.own_lo = -std::numeric_limits<double>::infinity();
    g.own_hi = std::numeric_limits<double>::infinity();
    c->grid = g;
    c->phys = make_phys(prm);
    choose_kernel_forms(c, prm->lanes_per_particle > 0, (double)nf / g.ncx, nf);
}

void ctx_setup(sphx_ctx *c, const sphx_params *prm, int n_fluid, int n_total, const double *pos, const double *vel,
               const double *drho_dt, const double *mass, const double *wall_vel, double t0, int64_t step0)
{
    common_checks(prm, n_fluid, n_total);
    ensure_device();
    ctx_configure(c, prm, n_fluid, n_total, pos);
    const int nf = c->nf, nw = c->nw;
    const size_t ntz = (size_t)n_total;
    const double *px = pos, *py = pos + ntz;

    SPHX_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    SPHX_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->h_clock), sizeof(Clock), hipHostMallocDefault));
    ctx_alloc(c, nf);
    upload_fluid(c, nf, px, py, vel, vel + ntz, drho_dt, mass, nullptr, true);
    std::vector<int> wid((size_t)std::max(nw, 1));
    for (int k = 0; k < nw; ++k) wid[k] = nf + k;
    upload_walls(c, nw, px + nf, py + nf, mass + nf, wall_vel + nf, wall_vel + ntz + nf, wid.data(), true);
    init_clock(c, nf, t0, step0);
    read_clock(c);
    // capture the step graphs now, not inside somebody's timed region (a few ms) -- unless this context can never
    // step (the one-shot contexts behind sphx_neighbor_search)
    if (prm->t_end > t0) (void)capture_slots(c->sched, c->stream, c->rebuild_every, graph_slots(c), ctx_slot(c));
}

// emit the MEX-convention pair list of the current ordering into the ctx-held buffers
void emit_pairs(sphx_ctx *c, bool fill)
{
    const int nf = c->nf;
    hipStream_t s = c->stream;
    DevBuf<int> cnt(nf), off((size_t)nf + 1);
    const FluidSet fs = c->view(c->sched.cur, c->sched.lay);
    const Clock *clk = c->clock.get();
    const dim3 g1(div_up(nf, kBlock)), b1(kBlock);
    hipLaunchKernelGGL(k_pairs<0>, g1, b1, 0, s, clk, c->grid, c->phys, fs, c->walls, cnt.get(), (const int *)nullptr,
                       (double *)nullptr, (double *)nullptr, (double *)nullptr, (double *)nullptr, (double *)nullptr,
                       (double *)nullptr, (double *)nullptr);
    hipLaunchKernelGGL(k_scan_only, dim3(1), dim3(kScanBlock), 0, s, (const Clock *)nullptr, 0, (const int *)cnt.get(), off.get(), nf);
    int total = 0;
    SPHX_HIP(hipMemcpyAsync(&total, off.get() + nf, sizeof(int), hipMemcpyDeviceToHost, s));
    SPHX_HIP(hipStreamSynchronize(s));
    c->pl_n = (size_t)total;
    if (!fill) return;
    const size_t m = c->pl_n ? c->pl_n : 1;
    c->pl_i.alloc(m); c->pl_j.alloc(m); c->pl_dx.alloc(m); c->pl_dy.alloc(m); c->pl_r.alloc(m); c->pl_W.alloc(m); c->pl_dW.alloc(m);
    hipLaunchKernelGGL(k_pairs<1>, g1, b1, 0, s, clk, c->grid, c->phys, fs, c->walls, (int *)nullptr, (const int *)off.get(),
                       c->pl_i.get(), c->pl_j.get(), c->pl_dx.get(), c->pl_dy.get(), c->pl_r.get(), c->pl_W.get(), c->pl_dW.get());
    SPHX_HIP(hipGetLastError());
    SPHX_HIP(hipStreamSynchronize(s));
    c->pl_valid = true;
}

// time one step slot advances by, before clipping to the target (dual-rate loop: n_in sub-steps, see next_dt)
double host_dt_unclipped(const sphx_ctx *c, double vmax)
{
    const double hh = c->phys.kc.h;
    const double dt_ac = 0.25 * hh / std::max(c->phys.c_f + vmax, 1e-12);
    const double dt_rest = std::min(0.125 * hh * hh / std::max(c->phys.nu, 1e-12),
                                    0.25 * std::sqrt(hh / std::max(std::fabs(c->phys.g), 1e-12)));
    return std::min(c->n_in * dt_ac, dt_rest);
}

void throw_on_status(const sphx_ctx *c)
{
    if (c->h_clock->status == SPHX_ERR_GRID)
        throw Error(SPHX_ERR_GRID, "SPHX:Ctx:grid", "neighbour list / slab buffer capacity exceeded on device");
    if (c->h_clock->status != 0)
        throw Error(c->h_clock->status, "SPHX:Ctx:diverged", "device step loop raised a status (non-finite velocity)");
}

}  // namespace

SPHX_EXPORT int sphx_ctx_create(sphx_ctx **out, const sphx_params *prm, int n_fluid, int n_total, const double *pos,
                                const double *vel, const double *drho_dt, const double *mass, const double *wall_vel,
                                double t0, int64_t step0)
{
    sphx_ctx *c = nullptr;
    try {
        require(out != nullptr, "SPHX:Ctx:out", "ctx output pointer must not be NULL");
        c = new sphx_ctx();
        ctx_setup(c, prm, n_fluid, n_total, pos, vel, drho_dt, mass, wall_vel, t0, step0);
        *out = c;
        return SPHX_OK;
    } catch (const Error &e) {
        delete c;
        return report(e);
    } catch (const std::exception &e) {
        delete c;
        return report_unknown(e);
    }
}

SPHX_EXPORT void sphx_ctx_destroy(sphx_ctx *ctx)
{
    if (!ctx) return;
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->comm) (void)sphx_slab_comm_destroy(ctx);
    if (g_fetch_src == ctx) g_fetch_src = nullptr;
    delete ctx;
}

static void settle_owed(sphx_ctx *c);

SPHX_EXPORT int sphx_ctx_advance(sphx_ctx *c, double t_target, int64_t max_steps, sphx_status *status)
{
    SPHX_TRY
    require(c != nullptr, "SPHX:Ctx:null", "ctx must not be NULL");
    require(!c->is_slab, "SPHX:Ctx:slab", "slab contexts are advanced with sphx_slab_compute/finish");
    // steps enqueued with sphx_ctx_enqueue_steps may still be in flight, and a batch of them that stopped early (stale grid)
    // still owes steps: they are taken first, as sphx_ctx_sync would -- "exactly n_steps" holds whatever call comes next
    settle_owed(c);
    for (int guard = 0; guard < 1000000; ++guard) {
        if (c->h_clock->need_rebuild && c->h_clock->status == 0) forced_rebuild(c);
        arm_clock(c, t_target, (long long)max_steps, c->sched.cur, (const double *)nullptr);
        // how many slots this call needs, from the unclipped dt; over-provision to whole graphs when unlimited
        const Clock &k = *c->h_clock;
        const double dt_est = host_dt_unclipped(c, k.vmax);
        double want = std::ceil(std::max(0.0, std::min(t_target, k.t_end) - k.t) / std::max(dt_est, 1e-12)) + 1.0;
        // Slots behind a stop (target reached, stale grid) are empty launches, ~10 us each: look at the clock
        // often while the device keeps stopping for forced rebuilds, rarely (4096 slots) once it runs through.
        want = std::min(want, (double)c->chunk_slots);
        int64_t slots = (int64_t)want;
        const int per_graph = graph_slots(c);
        bool exact = false;
        if (max_steps > 0 && slots >= max_steps) { slots = max_steps; exact = true; }  // exact: no no-op slots
        else if (!c->profiling && slots > per_graph) slots = ((slots + per_graph - 1) / per_graph) * per_graph;
        if (slots < 1) slots = 1;
        const int64_t step_before = c->h_clock->step;
        ctx_enqueue(c, slots, exact);
        read_clock(c);
        const int64_t executed = c->h_clock->step - step_before;
        // ... and in between by how often it has been stopping: behind a stop the rest of the chunk drains as empty launches
        // (half a 4096-slot chunk: ~35 ms at 0.5 M particles, measured), a look at the clock costs ~40 us -- chunks of 1/16 of
        // the steps since the last forced rebuild keep both near 0.5 us per step.
        const int64_t cap = c->sched.n_forced == 0
                                ? 4096
                                : std::clamp<int64_t>((c->h_clock->step - c->last_forced_step) / 16, 64, 4096);
        c->chunk_slots = c->h_clock->need_rebuild ? 64 : std::min<int64_t>(cap, 2 * c->chunk_slots);
        if (max_steps > 0) {
            max_steps -= executed;
            if (max_steps <= 0) break;
        }
        if (c->h_clock->status != 0) break;
        if (!(c->h_clock->t < t_target - 1e-12)) break;
        if (!(c->h_clock->t < c->h_clock->t_end - 1e-12)) break;
    }
    c->pending_target = c->h_clock->step;
    fill_status(c, status);
    throw_on_status(c);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_enqueue_steps(sphx_ctx *c, int64_t n_steps)
{
    SPHX_TRY
    require(c != nullptr, "SPHX:Ctx:null", "ctx must not be NULL");
    require(!c->is_slab, "SPHX:Ctx:slab", "slab contexts are advanced with sphx_slab_compute/finish");
    require(n_steps > 0, "SPHX:Ctx:steps", "n_steps must be positive");
    // no host sync here: if an earlier batch stopped early (end time, status, stale grid) the loop condition is
    // still false when k_prepare re-evaluates it, so every slot of this batch is a no-op; sphx_ctx_sync sorts
    // out the grid and takes the steps that are still owed
    arm_clock(c, c->prm.t_end, (long long)n_steps, c->sched.cur, (const double *)nullptr);
    ctx_enqueue(c, n_steps, true);
    c->pending_target = std::max<int64_t>(c->pending_target, c->h_clock->step) + n_steps;
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_prepare_steps(sphx_ctx *c, int64_t n_steps)
{
    SPHX_TRY
    require(c != nullptr, "SPHX:Ctx:null", "ctx must not be NULL");
    require(!c->is_slab, "SPHX:Ctx:slab", "slab contexts are advanced with sphx_slab_run");
    require(n_steps > 0, "SPHX:Ctx:steps", "n_steps must be positive");
    read_clock(c);  // the phase the next batch starts from
    if (c->h_clock->need_rebuild && c->h_clock->status == 0) forced_rebuild(c);
    hipLaunchKernelGGL(k_disarm, dim3(1), dim3(1), 0, c->stream, c->clock.get());  // (every batch re-arms with k_prepare)
    prepare_graphs(c, n_steps);
    SPHX_HIP(hipStreamSynchronize(c->stream));
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_graph_stats(sphx_ctx *c, int64_t *slots_replayed, int64_t *slots_eager, int64_t *graphs_captured)
{
    SPHX_TRY
    require(c != nullptr, "SPHX:Ctx:null", "ctx must not be NULL");
    if (slots_replayed) *slots_replayed = c->sched.slots_replayed;
    if (slots_eager) *slots_eager = c->sched.slots_eager;
    if (graphs_captured) *graphs_captured = c->sched.graphs_captured;
    return SPHX_OK;
    SPHX_CATCH
}

// Wait for what is enqueued and take the steps a batch of sphx_ctx_enqueue_steps still owes: a batch stops early when the
// drift bound is hit (static schedule) -- re-bin, then go on, in chunks (slots behind another stop would be empty launches).
// Leaves the clock read.  Whoever hands out results calls this first: a batch that stopped before its armed last step has
// not written the output-only fields of that step (FluidTmp::lazy_out), so force / rho / p would be those of an older batch.
static void settle_owed(sphx_ctx *c)
{
    read_clock(c);
    for (int guard = 0; guard < 1000000; ++guard) {
        const Clock &k = *c->h_clock;
        const int64_t owed = c->pending_target - (int64_t)k.step;
        if (!(k.status == 0 && owed > 0 && k.t < k.t_end - 1e-12)) break;
        if (k.need_rebuild) {
            forced_rebuild(c);
            c->chunk_slots = 64;
        }
        const int64_t n = std::min(owed, c->chunk_slots);
        arm_clock(c, c->prm.t_end, (long long)n, c->sched.cur, (const double *)nullptr);
        ctx_enqueue(c, n, false);
        read_clock(c);
        if (!c->h_clock->need_rebuild) c->chunk_slots = std::min<int64_t>(4096, 2 * c->chunk_slots);
    }
    c->pending_target = c->h_clock->step;
}

SPHX_EXPORT int sphx_ctx_sync(sphx_ctx *c, sphx_status *status)
{
    SPHX_TRY
    require(c != nullptr, "SPHX:Ctx:null", "ctx must not be NULL");
    require(!c->is_slab, "SPHX:Ctx:slab", "use sphx_slab_sync on a slab context");
    settle_owed(c);
    fill_status(c, status);
    throw_on_status(c);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_download(sphx_ctx *c, double *pos, double *vel, double *rho, double *p, double *drho_dt,
                                  double *force, double *force_prior, double *Vol, double *B)
{
    SPHX_TRY
    require(c != nullptr, "SPHX:Ctx:null", "ctx must not be NULL");
    require(!c->is_slab, "SPHX:Ctx:slab", "use sphx_slab_snapshot on a slab context");
    settle_owed(c);  // (state and step outputs of the SAME step: the last one of everything enqueued, see settle_owed)
    const bool need_outputs = rho || p || force || force_prior || Vol || B;
    if (need_outputs && !c->have_step_outputs)
        throw Error(SPHX_ERR_STATE, "SPHX:Ctx:download", "rho/p/force/Vol/B exist only after at least one step");
    const int nf = c->nf, nw = c->nw, nt = c->nt;
    hipStream_t s = c->stream;
    const FluidSet fs = c->view(c->sched.cur, c->sched.lay);
    // ordering the step outputs are stored in: the layout the step ran in (static schedule), or -- dynamic contexts,
    // which re-bin in place -- the current ids reached through src_of when the last step ended with a re-binning
    const int *id_old = c->dyn ? fs.id : (c->out_ids ? c->out_ids : c->fid_[c->out_lay].get());
    const int *out_map = (c->dyn && c->h_clock->fresh) ? (const int *)c->src_of.get() : nullptr;
    DevBuf<double> stage((size_t)4 * nt);
    const dim3 gf(div_up(nf, kBlock)), gw(div_up(std::max(nw, 1), kBlock)), b(kBlock);
    auto col = [&](int cidx) { return stage.get() + (size_t)cidx * nt; };
    // component `comp` of a field stored as records of `stride` doubles
    auto unsort_f = [&](const int *id, const void *src, int stride, int comp, int cidx) {  // current state
        hipLaunchKernelGGL(k_unsort, gf, b, 0, s, nf, id, (const double *)src + comp, stride, col(cidx), (const int *)nullptr);
    };
    auto unsort_o = [&](const void *src, int stride, int comp, int cidx) {  // outputs of the last step
        hipLaunchKernelGGL(k_unsort, gf, b, 0, s, nf, id_old, (const double *)src + comp, stride, col(cidx), out_map);
    };
    auto unsort_w = [&](const void *src, int stride, int comp, int cidx) {
        if (nw > 0)
            hipLaunchKernelGGL(k_unsort, gw, b, 0, s, nw, (const int *)c->wid.get(), (const double *)src + comp, stride, col(cidx),
                               (const int *)nullptr);
    };
    auto fill_w = [&](int cidx, double v) {
        if (nw > 0) hipLaunchKernelGGL(k_fill, gw, b, 0, s, nw, col(cidx) + nf, v);
    };
    auto out = [&](double *host, int ncol) {
        SPHX_HIP(hipMemcpyAsync(host, stage.get(), (size_t)ncol * nt * sizeof(double), hipMemcpyDeviceToHost, s));
        SPHX_HIP(hipStreamSynchronize(s));
    };
    if (pos) {
        unsort_f(fs.id, fs.pos, 2, 0, 0); unsort_f(fs.id, fs.pos, 2, 1, 1);
        unsort_w(c->wpos.get(), 2, 0, 0); unsort_w(c->wpos.get(), 2, 1, 1);
        out(pos, 2);
    }
    if (vel) { unsort_f(fs.id, fs.vel, 2, 0, 0); unsort_f(fs.id, fs.vel, 2, 1, 1); fill_w(0, 0.0); fill_w(1, 0.0); out(vel, 2); }
    if (drho_dt) { unsort_f(fs.id, fs.drho, 1, 0, 0); fill_w(0, 0.0); out(drho_dt, 1); }
    if (rho) { unsort_o(c->rho_out.get(), 1, 0, 0); fill_w(0, c->prm.rho0); out(rho, 1); }
    if (p) { unsort_o(c->p_out.get(), 1, 0, 0); fill_w(0, 0.0); out(p, 1); }
    if (force) { unsort_o(c->ff.get(), 2, 0, 0); unsort_o(c->ff.get(), 2, 1, 1); fill_w(0, 0.0); fill_w(1, 0.0); out(force, 2); }
    if (force_prior) { unsort_o(c->ffp.get(), 2, 0, 0); unsort_o(c->ffp.get(), 2, 1, 1); fill_w(0, 0.0); fill_w(1, 0.0); out(force_prior, 2); }
    if (Vol) { unsort_o(c->tmp_par[c->fuse_ea ? c->out_par : 0].a, 4, 0, 0); unsort_w(c->wa.get(), 4, 0, 0); out(Vol, 1); }
    if (B) {
        for (int k = 0; k < 4; ++k) unsort_o(c->fB.get(), 4, k, k);
        fill_w(0, 1.0); fill_w(1, 0.0); fill_w(2, 0.0); fill_w(3, 1.0);
        out(B, 4);
    }
    SPHX_HIP(hipGetLastError());
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_monitor(sphx_ctx *c, double *tau_bottom, double *tau_top, double *n_pairs)
{
    SPHX_TRY
    require(c != nullptr, "SPHX:Ctx:null", "ctx must not be NULL");
    require(!c->is_slab, "SPHX:Ctx:slab", "monitors are not available on a slab context");
    settle_owed(c);
    if (c->h_clock->need_rebuild && c->h_clock->status == 0) forced_rebuild(c);  // the pair sweeps need valid bins
    hipStream_t s = c->stream;
    const FluidSet fs = c->view(c->sched.cur, c->sched.lay);
    if (tau_bottom || tau_top) {
        if (!c->have_step_outputs)
            throw Error(SPHX_ERR_STATE, "SPHX:Ctx:monitor", "wall shear needs Vol/B of a completed step");
        const int nblk = c->n_blocks_flat;
        hipLaunchKernelGGL(k_wall_shear, dim3(nblk), dim3(kBlock), 0, s, (const Clock *)c->clock.get(), c->grid, c->phys, fs,
                           c->tmp_par[c->fuse_ea ? c->out_par : 0], c->walls,
                           (c->dyn ? c->h_clock->fresh != 0 : (c->out_lay != c->sched.lay || c->out_ids)) ? 1 : 0, c->tau_part.get());
        hipLaunchKernelGGL(k_tau_final, dim3(1), dim3(kScanBlock), 0, s, nblk, (const double *)c->tau_part.get(),
                           c->phys.DL, c->tau_out.get());
        double h[2];
        SPHX_HIP(hipMemcpyAsync(h, c->tau_out.get(), sizeof(h), hipMemcpyDeviceToHost, s));
        SPHX_HIP(hipStreamSynchronize(s));
        if (tau_bottom) *tau_bottom = h[0];
        if (tau_top) *tau_top = h[1];
    }
    if (n_pairs) {
        emit_pairs(c, false);
        *n_pairs = (double)c->pl_n;
    }
    SPHX_HIP(hipGetLastError());
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_neighbor_list(sphx_ctx *c, size_t *n_pairs)
{
    SPHX_TRY
    require(c != nullptr && n_pairs != nullptr, "SPHX:Ctx:null", "ctx / n_pairs must not be NULL");
    require(!c->is_slab, "SPHX:Ctx:slab", "pair lists are not available on a slab context");
    settle_owed(c);  // (the list of the last step of everything enqueued, like the state sphx_ctx_download hands out)
    if (c->h_clock->need_rebuild && c->h_clock->status == 0) forced_rebuild(c);
    emit_pairs(c, true);
    *n_pairs = c->pl_n;
    g_fetch_src = c;
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_neighbor_search(const double *pos, int n_fluid, int n_total, double h, double DL, size_t *n_pairs)
{
    sphx_ctx *c = nullptr;
    try {
        require(n_pairs != nullptr && pos != nullptr, "SPH:Neighbor:pos", "pos must be a double matrix of size [n_total x 2].");
        require(n_total > 0 && n_fluid > 0 && n_fluid <= n_total, "SPH:Neighbor:count",
                "Invalid n_fluid/n_total or inconsistent pos size.");
        require(h > 0.0 && DL > 0.0, "SPH:Neighbor:param", "h and DL must be positive.");
        sphx_params prm{};
        prm.DL = DL; prm.DH = 1.0; prm.dp = h / 1.3; prm.h = h; prm.rho0 = 1.0; prm.mu = 1.0; prm.c_f = 1.0; prm.p0 = 1.0;
        prm.inv_sigma0 = 1.0; prm.gravity_g = 0.0; prm.transport_coeff = 0.0; prm.t_end = 0.0; prm.lanes_per_particle = 1;
        prm.rebuild_every = 1;
        const size_t nt = (size_t)n_total;
        std::vector<double> zeros2(2 * nt, 0.0), ones(nt, 1.0);
        // The driver calls this once per step with the same sizes (SPH_Poiseuille.m:428): keep the search context
        // (stream, pinned clock, device arrays, wall grid shape) and only reload the positions.  Creating and
        // destroying it every call cost 4.1 ms at 5 760 particles, the search itself 0.4 ms.
        sphx_ctx *old = g_search_ctx;
        bool reuse = false;
        if (old && old->nf == n_fluid && old->nt == n_total && old->prm.h == h && old->prm.DL == DL) {
            double y_min, y_max;
            y_extent(pos + nt, n_total, y_min, y_max);
            const double cs = 2.0 * h;
            reuse = old->grid.y0 == y_min && old->grid.ncy == (int)std::ceil((y_max - y_min + 1e-12) / cs) + 1;
        }
        if (reuse) {
            c = old;
            const int nw = n_total - n_fluid;
            upload_fluid(c, n_fluid, pos, pos + nt, zeros2.data(), zeros2.data(), zeros2.data(), ones.data(), nullptr, true);
            std::vector<int> wid((size_t)std::max(nw, 1));
            for (int k = 0; k < nw; ++k) wid[k] = n_fluid + k;
            upload_walls(c, nw, pos + n_fluid, pos + nt + n_fluid, ones.data(), zeros2.data(), zeros2.data(), wid.data(), true);
        } else {
            c = new sphx_ctx();
            ctx_setup(c, &prm, n_fluid, n_total, pos, zeros2.data(), zeros2.data(), ones.data(), zeros2.data(), 0.0, 0);
        }
        emit_pairs(c, true);
        *n_pairs = c->pl_n;
        if (old && old != c) delete old;
        g_search_ctx = c;
        g_fetch_src = c;
        return SPHX_OK;
    } catch (const Error &e) {
        if (c == g_search_ctx) g_search_ctx = nullptr;
        if (g_fetch_src == c) g_fetch_src = nullptr;
        delete c;
        return report(e);
    } catch (const std::exception &e) {
        if (c == g_search_ctx) g_search_ctx = nullptr;
        if (g_fetch_src == c) g_fetch_src = nullptr;
        delete c;
        return report_unknown(e);
    }
}

SPHX_EXPORT int sphx_neighbor_fetch(double *pair_i, double *pair_j, double *dx, double *dy, double *r, double *W,
                                    double *dW, size_t capacity)
{
    SPHX_TRY
    sphx_ctx *c = g_fetch_src;
    if (!c || !c->pl_valid) throw Error(SPHX_ERR_STATE, "SPHX:Neighbor:fetch", "no pair list pending (call a search first)");
    require(capacity >= c->pl_n, "SPHX:Neighbor:capacity", "output arrays are shorter than the pair list");
    const size_t n = c->pl_n;
    hipStream_t s = c->stream;
    if (n) {
        if (pair_i) c->pl_i.download(pair_i, n, s);
        if (pair_j) c->pl_j.download(pair_j, n, s);
        if (dx) c->pl_dx.download(dx, n, s);
        if (dy) c->pl_dy.download(dy, n, s);
        if (r) c->pl_r.download(r, n, s);
        if (W) c->pl_W.download(W, n, s);
        if (dW) c->pl_dW.download(dW, n, s);
        SPHX_HIP(hipStreamSynchronize(s));
    }
    c->pl_valid = false;
    c->pl_i.release(); c->pl_j.release(); c->pl_dx.release(); c->pl_dy.release(); c->pl_r.release(); c->pl_W.release(); c->pl_dW.release();
    g_fetch_src = nullptr;  // the search context itself stays for the next search of the same shape
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_profile_enable(sphx_ctx *c, int on)
{
    SPHX_TRY
    require(c != nullptr, "SPHX:Ctx:null", "ctx must not be NULL");
    SPHX_HIP(hipStreamSynchronize(c->stream));
    c->timer.collect();
    c->profiling = on != 0;
    c->timer.timer_log = debug_switches().log;
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_profile_read(sphx_ctx *c, int capacity, const char **names, double *avg_ms, int64_t *launches,
                                      int *n_kernels)
{
    SPHX_TRY
    require(c != nullptr && n_kernels != nullptr, "SPHX:Ctx:null", "ctx must not be NULL");
    SPHX_HIP(hipStreamSynchronize(c->stream));
    c->timer.collect();
    const int n = (int)c->timer.names.size();
    *n_kernels = n;
    for (int k = 0; k < n && k < capacity; ++k) {
        if (names) names[k] = c->timer.names[k].c_str();
        if (avg_ms) avg_ms[k] = c->timer.launches[k] ? c->timer.total_ms[k] / (double)c->timer.launches[k] : 0.0;
        if (launches) launches[k] = c->timer.launches[k];
    }
    for (auto &v : c->timer.total_ms) v = 0.0;
    for (auto &v : c->timer.launches) v = 0;
    return SPHX_OK;
    SPHX_CATCH
}

#include "sphx_samplers.hpp"  // the slot samplers: launches, lifecycle, sphx_ctx_flow_stats_* / history_* / field_map_* / probes_* / profile_series_* / pair_dist_* / grad_stats_* / tracers_* / dens_stats_* / modes_*

SPHX_EXPORT int sphx_ctx_info(sphx_ctx *c, int *n_fluid, int *n_wall, int *n_cell_x, int *n_cell_y)
{
    SPHX_TRY
    require(c != nullptr, "SPHX:Ctx:null", "ctx must not be NULL");
    if (n_fluid) *n_fluid = c->nf;
    if (n_wall) *n_wall = c->nw;
    if (n_cell_x) *n_cell_x = c->grid.ncx;
    if (n_cell_y) *n_cell_y = c->grid.ncy;
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_grid_policy(sphx_ctx *c, int *rebuild_every, double *skin, int64_t *forced_rebuilds,
                                     double *drift)
{
    SPHX_TRY
    require(c != nullptr, "SPHX:Ctx:null", "ctx must not be NULL");
    if (rebuild_every) *rebuild_every = c->rebuild_every;
    if (skin) *skin = c->skin;
    if (forced_rebuilds) *forced_rebuilds = c->dyn ? (int64_t)c->h_clock->n_drift_rebuilds : c->sched.n_forced;
    if (drift) *drift = c->h_clock->drift;
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_tuning(sphx_ctx *c, int *lanes_per_particle, int *steps_per_graph)
{
    SPHX_TRY
    require(c != nullptr, "SPHX:Ctx:null", "ctx must not be NULL");
    if (lanes_per_particle) *lanes_per_particle = c->lpp;
    if (steps_per_graph) *steps_per_graph = c->spg;
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_block_size(sphx_ctx *c, int *block_size)
{
    SPHX_TRY
    require(c != nullptr && block_size != nullptr, "SPHX:Ctx:null", "ctx / block_size must not be NULL");
    *block_size = c->block;
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_schedule(sphx_ctx *c, int *fuse_ea, int *tail_clock, int *dynamic, int64_t *rebins)
{
    SPHX_TRY
    require(c != nullptr, "SPHX:Ctx:null", "ctx must not be NULL");
    if (fuse_ea) *fuse_ea = c->fuse_ea ? 1 : 0;
    if (tail_clock) *tail_clock = c->tail_clock ? 1 : 0;
    if (dynamic) *dynamic = c->dyn ? 1 : 0;
    if (rebins) *rebins = c->dyn ? (int64_t)c->h_clock->n_rebins : c->n_rebins;
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_kernel_forms(sphx_ctx *c, int *walk_kernels, int *lds_tiles, int *tiles_abe, int *coded_lists)
{
    SPHX_TRY
    require(c != nullptr, "SPHX:Ctx:null", "ctx must not be NULL");
    if (walk_kernels) *walk_kernels = c->walk_kernels ? 1 : 0;
    if (lds_tiles) *lds_tiles = c->lds_tiles ? 1 : 0;
    if (tiles_abe) *tiles_abe = c->lds_tiles_be ? 1 : 0;
    if (coded_lists) *coded_lists = c->coded_lists ? 1 : 0;
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_substeps(sphx_ctx *c, int *n_inner)
{
    SPHX_TRY
    require(c != nullptr && n_inner != nullptr, "SPHX:Ctx:null", "ctx / n_inner must not be NULL");
    *n_inner = c->n_in;
    return SPHX_OK;
    SPHX_CATCH
}

// =================================================================================================
// x-slab contexts (multi-GPU): one context per rank holds the particles of its column range plus
// `halo_cols` columns of copies on either side, in an OPEN grid window.  Per step:
//   sphx_slab_compute : k_density..k_continuity on everything held, local max|v| of owned particles,
//                       pack keep / send-left / send-right
//   (caller: exchange the two messages with the ring neighbours, all-reduce max|v|)
//   sphx_slab_finish  : unpack, clock update with the global max|v|, cell rebuild.
// Validity: with halo H columns (each >= 2h wide) pass A is exact on columns >= own-(H-1), pass B on
// >= own-(H-2), the force pass on >= own-(H-3) and the continuity pass on the owned columns for H = 4;
// whatever is computed on halo copies is discarded (their owner sends fresh state).
// =================================================================================================
namespace {

struct HostParticles {
    std::vector<double> x, y, vx, vy, drho, mass;
    std::vector<int> id;
    void push(double X, double Y, double VX, double VY, double D, double M, int I)
    {
        x.push_back(X); y.push_back(Y); vx.push_back(VX); vy.push_back(VY); drho.push_back(D); mass.push_back(M); id.push_back(I);
    }
};

void slab_setup(sphx_ctx *c, const sphx_params *prm, int n_fluid, int n_total, const double *pos, const double *vel,
                const double *drho_dt, const double *mass, const double *wall_vel, double t0, int64_t step0, int rank,
                int n_ranks, int halo_cols, void *stream)
{
    common_checks(prm, n_fluid, n_total);
    require(n_ranks >= 2 && rank >= 0 && rank < n_ranks, "SPHX:Slab:rank", "slab contexts need n_ranks >= 2 and 0 <= rank < n_ranks");
    require(halo_cols >= 4, "SPHX:Slab:halo", "halo_cols must be >= 4 (four dependent neighbour passes per step)");
    ensure_device();
    c->prm = *prm;
    c->is_slab = true;
    c->rank = rank; c->n_ranks = n_ranks; c->halo_cols = halo_cols;
    c->nf = n_fluid; c->nt = n_total; c->nw = n_total - n_fluid;
    const size_t ntz = (size_t)n_total;
    const double *px = pos, *py = pos + ntz;
    double y_min, y_max;
    y_extent(py, n_total, y_min, y_max);
    // Re-binning interval of the slab: 1 = every step (the protocol of sphx_slab_compute / _finish, a caller-driven
    // transport); K > 1 (0 = auto: 5) = every K-th step with a cell skin, frozen layouts and fixed exchange lists in between
    // (the native loops sphx_slab_run / sphx_slab_group_run only).
    // (round 4: a slab decides on the device like a dynamic context -- the skin of K = 5, scheduled re-binnings every 24th step,
    //  see ctx_setup)
    const bool auto_policy = prm->rebuild_every <= 0 && prm->skin_h <= 0.0;
    int K = prm->rebuild_every > 0 ? std::min(prm->rebuild_every, 64) : 24;
    const double d_step = 0.035 * prm->h;
    double skin = K > 1 ? (prm->skin_h > 0.0 ? prm->skin_h * prm->h : 2.0 * std::max((K - 1) * d_step, 0.1 * prm->h)) : 0.0;
    if (auto_policy) skin = 0.28 * prm->h;
    c->rebuild_every = K;
    c->skin = skin;
    c->dyn = K > 1;  // the device decides when to re-bin (from all-reduced maxima), the layout is rebuilt in place
    const double cs = 2.0 * prm->h + skin, DL = prm->DL;
    const int ncx_g = (int)std::floor(DL / cs);
    require(ncx_g >= 3, "SPH:Neighbor:param", "channel too short for three cell columns.");
    const double csx = DL / ncx_g;
    const int H = halo_cols;
    auto col_lo = [&](int r) { return (int)(((long long)r * ncx_g) / n_ranks); };
    c->col0 = col_lo(rank);
    c->col1 = col_lo(rank + 1);
    c->ncx_ring = ncx_g;
    for (int r = 0; r < n_ranks; ++r)
        require(col_lo(r + 1) - col_lo(r) >= H + 1, "SPHX:Slab:width",
                "every slab must own at least halo_cols+1 cell columns (use fewer ranks or a longer channel)");
    require((c->col1 - c->col0) + 2 * H < ncx_g, "SPHX:Slab:width", "slab window would cover the whole period");

    Grid g{};
    g.ncx = (c->col1 - c->col0) + 2 * H;
    g.ncy = (int)std::ceil((y_max - y_min + 1e-12) / cs) + 1;
    g.ncells = g.ncx * g.ncy;
    g.periodic = 0;
    g.DL = DL;
    g.half_DL = std::numeric_limits<double>::infinity();
    g.x0 = (double)(c->col0 - H) * csx;
    g.y0 = y_min;
    g.inv_csx = (double)ncx_g / DL;
    g.inv_csy = 1.0 / cs;
    g.own_lo = (double)c->col0 * csx;
    g.own_hi = (rank == n_ranks - 1) ? DL : (double)c->col1 * csx;
    g.own_by_cell = K > 1 ? 1 : 0;
    g.own_c0 = H;
    g.own_c1 = H + (c->col1 - c->col0);
    c->grid = g;
    c->phys = make_phys(prm);
    const double win_lo = g.x0, win_hi = g.x0 + (double)g.ncx * csx;

    // select the particles (and periodic images) inside this rank's window
    HostParticles hf, hw;
    std::vector<double> wvx, wvy;
    for (int i = 0; i < n_total; ++i) {
        const double xw = px[i] - std::floor(px[i] / DL) * DL;
        for (int im = -1; im <= 1; ++im) {
            const double xs = xw + im * DL;
            if (!(xs >= win_lo && xs < win_hi)) continue;
            if (i < n_fluid) hf.push(xs, py[i], vel[i], vel[ntz + i], drho_dt[i], mass[i], i);
            else { hw.push(xs, py[i], 0, 0, 0, mass[i], i); wvx.push_back(wall_vel[i]); wvy.push_back(wall_vel[ntz + i]); }
        }
    }
    const int n_local = (int)hf.x.size(), nw_local = (int)hw.x.size();
    // capacities: a message carries the H boundary columns plus what crossed in one step -- (H+1) columns at 1.3x the mean
    // column load (the whole buffer travels every step: 1 + 7 cap doubles per neighbour; overflow raises SPHX_ERR_GRID)
    const double per_col = (double)n_fluid / ncx_g;
    c->msg_cap = (int)(1.3 * (H + 1) * per_col) + 1024;
    // (every kernel is launched for `cap` particles: slack costs time -- 15 % headroom over the initial population of this
    // weakly compressible flow; an overflow raises SPHX_ERR_GRID on the device, never a silent loss)
    const int cap = (int)(1.15 * std::max<double>(n_local, per_col * g.ncx)) + 2 * c->msg_cap + 1024;
    require(n_local <= cap, "SPHX:Slab:capacity", "initial slab population exceeds capacity");

    c->lpp = prm->lanes_per_particle > 0 ? prm->lanes_per_particle : pick_lpp(n_local);
    check_lpp(c->lpp);
    choose_kernel_forms(c, prm->lanes_per_particle > 0, per_col, n_local);
    c->spg = 2;
    if (stream) { c->stream = (hipStream_t)stream; c->own_stream = false; }
    else SPHX_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    SPHX_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->h_clock), sizeof(Clock), hipHostMallocDefault));
    ctx_alloc(c, cap);
    upload_fluid(c, n_local, hf.x.data(), hf.y.data(), hf.vx.data(), hf.vy.data(), hf.drho.data(), hf.mass.data(),
                 hf.id.data(), false);
    upload_walls(c, nw_local, hw.x.data(), hw.y.data(), hw.mass.data(), wvx.data(), wvy.data(), hw.id.data(), false);

    c->kpos.alloc(cap); c->kvel.alloc(cap); c->kdrho.alloc(cap); c->kmass.alloc(cap);
    c->kid.alloc(cap); c->counters.alloc(3); c->n_new.alloc(1); c->ticket.alloc(1);
    c->counters.zero(c->stream); c->ticket.zero(c->stream); c->n_new.zero(c->stream);
    SlabPack p{};
    p.counters = c->counters.get();
    p.kpos = c->kpos.get(); p.kvel = c->kvel.get(); p.kdrho = c->kdrho.get();
    p.kmass = c->kmass.get(); p.kid = c->kid.get();
    p.cellid = c->cellid.get(); p.count = c->count.get();
    p.halo_w = (double)H * csx;
    p.shift_l = (rank == 0) ? DL : 0.0;             // my left neighbour is the last slab: it sees me at x + DL
    p.shift_r = (rank == n_ranks - 1) ? -DL : 0.0;  // my right neighbour is the first slab
    p.win_lo = win_lo;
    p.win_hi = win_hi;
    p.msg_cap = c->msg_cap;
    p.keep_cap = cap;
    c->pack = p;
    if (K > 1) {
        for (int k = 0; k < 2; ++k) {
            c->send_idx_[k].alloc(c->msg_cap); c->recv_slot_[k].alloc(c->msg_cap);
            c->ids_s_[k].alloc((size_t)c->msg_cap + 1); c->ids_r_[k].alloc((size_t)c->msg_cap + 1);
            c->ids_s_[k].zero(c->stream); c->ids_r_[k].zero(c->stream);
        }
        c->send_cnt.alloc(2); c->recv_cnt.alloc(2); c->slot_of_id.alloc((size_t)n_fluid);
        c->send_cnt.zero(c->stream); c->recv_cnt.zero(c->stream);
        SPHX_HIP(hipMemsetAsync(c->slot_of_id.get(), 0xFF, (size_t)n_fluid * sizeof(int), c->stream));
        c->lists = SlabLists{{c->send_idx_[0].get(), c->send_idx_[1].get()}, c->send_cnt.get(),
                             {c->recv_slot_[0].get(), c->recv_slot_[1].get()}, c->recv_cnt.get(), c->slot_of_id.get(),
                             {c->ids_s_[0].get(), c->ids_s_[1].get()}};
        if (n_local > 0)
            hipLaunchKernelGGL(k_slot_of_id, dim3(div_up(n_local, kBlock)), dim3(kBlock), 0, c->stream, n_local,
                               (const int *)c->fid_[0].get(), c->slot_of_id.get());
        SPHX_HIP(hipGetLastError());
    }
    init_clock(c, n_local, t0, step0);
    c->slab_step0 = step0;
    read_clock(c);
}

}  // namespace

SPHX_EXPORT int sphx_slab_create(sphx_ctx **out, const sphx_params *prm, int n_fluid, int n_total, const double *pos,
                                 const double *vel, const double *drho_dt, const double *mass, const double *wall_vel,
                                 double t0, int64_t step0, int rank, int n_ranks, int halo_cols, void *hip_stream)
{
    sphx_ctx *c = nullptr;
    try {
        require(out != nullptr, "SPHX:Ctx:out", "ctx output pointer must not be NULL");
        c = new sphx_ctx();
        slab_setup(c, prm, n_fluid, n_total, pos, vel, drho_dt, mass, wall_vel, t0, step0, rank, n_ranks, halo_cols, hip_stream);
        *out = c;
        return SPHX_OK;
    } catch (const Error &e) {
        delete c;
        return report(e);
    } catch (const std::exception &e) {
        delete c;
        return report_unknown(e);
    }
}

SPHX_EXPORT int sphx_slab_layout(sphx_ctx *c, int64_t *msg_doubles, int *col0, int *col1, int *n_local, int *capacity)
{
    SPHX_TRY
    require(c != nullptr && c->is_slab, "SPHX:Slab:ctx", "not a slab context");
    if (msg_doubles) *msg_doubles = 1 + 7 * (int64_t)c->msg_cap;
    if (col0) *col0 = c->col0;
    if (col1) *col1 = c->col1;
    if (n_local) *n_local = c->h_clock->n;
    if (capacity) *capacity = c->cap;
    return SPHX_OK;
    SPHX_CATCH
}

// local max |v| of owned particles at the current state -> vmax_dev[0] (device pointer); async.
SPHX_EXPORT int sphx_slab_local_vmax(sphx_ctx *c, double *vmax_dev)
{
    SPHX_TRY
    require(c != nullptr && c->is_slab && vmax_dev != nullptr, "SPHX:Slab:ctx", "not a slab context");
    require(c->rebuild_every == 1, "SPHX:Slab:protocol", "local_vmax / prepare / compute / finish drive a slab created with rebuild_every = 1");
    const FluidSet fs = c->view(c->sched.cur, c->sched.cur);
    hipLaunchKernelGGL(k_vmax_init, dim3(1), dim3(kScanBlock), 0, c->stream, c->clock.get(), c->grid, (const double2 *)fs.pos,
                       (const double2 *)fs.vel, vmax_dev);
    SPHX_HIP(hipGetLastError());
    return SPHX_OK;
    SPHX_CATCH
}

// arm the clock with the all-reduced max |v| (device pointer); async.
SPHX_EXPORT int sphx_slab_prepare(sphx_ctx *c, double t_target, int64_t max_steps, const double *vmax_global_dev)
{
    SPHX_TRY
    require(c != nullptr && c->is_slab, "SPHX:Slab:ctx", "not a slab context");
    require(c->rebuild_every == 1, "SPHX:Slab:protocol", "local_vmax / prepare / compute / finish drive a slab created with rebuild_every = 1");
    arm_clock(c, t_target, (long long)max_steps, c->sched.cur, vmax_global_dev);
    SPHX_HIP(hipGetLastError());
    return SPHX_OK;
    SPHX_CATCH
}

namespace {

// first half of a slab step on the context's stream: the four neighbour passes, pack, seal + local max |v|
void slab_compute_impl(sphx_ctx *c, double *send_left_dev, double *send_right_dev, double *vmax_local_dev)
{
    const int q = c->sched.cur;
    const Clock *clk = c->clock.get();
    launch_passes(c, q, c->view(q, q), c->tmp, PassA::Sweep);
    SlabPack p = c->pack;
    p.send_l = send_left_dev;
    p.send_r = send_right_dev;
    launch(c, "k_slab_pack", k_slab_pack, dim3(c->n_blocks_flat), dim3(kBlock), clk, q, c->grid, c->view(q, q), c->tmp, p);
    launch(c, "k_slab_seal_vmax", k_slab_seal_vmax, dim3(1), dim3(kScanBlock), clk, q, p, c->n_vpart,
           (const double *)c->vpart.get(), vmax_local_dev);
    SPHX_HIP(hipGetLastError());
}

// second half: unpack the received messages, clock update with the global max |v|, cell rebuild
void slab_finish_impl(sphx_ctx *c, const double *recv_left_dev, const double *recv_right_dev, const double *vmax_global_dev)
{
    const int q = c->sched.cur;
    Clock *clk = c->clock.get();
    const dim3 bp(kBlock);
    // kept particles were binned by the pack kernel, the received ones are binned here
    launch(c, "k_slab_unpack", k_slab_unpack, dim3(div_up((size_t)2 * c->msg_cap, kBlock)), bp, (const Clock *)clk, q,
           c->grid, c->pack, recv_left_dev, recv_right_dev, c->n_new.get(), c->flags.get());
    // clock: t += dt, new particle count, next dt from the global max |v| -- and the scan of the cell histogram
    // and the reset of the pack counters.  It arms run[1-q]; the remaining kernels of this slot still test
    // run[q], and from here on clk->n is the new particle count.
    const FluidSet d = c->view(1 - q, 1 - q);
    ClockScan clock;
    clock.vmax_global = vmax_global_dev;
    clock.count = c->count.get();
    clock.start_next = d.start;
    clock.n_new = c->n_new.get();
    clock.rebuilt = 1;
    clock.slab_counters = c->counters.get();
    launch_clock_scan(c, q, clock);
    launch_scatter_reorder(c, q,
                           reorder_args(c->kpos.get(), c->kvel.get(), c->kdrho.get(), c->kmass.get(), c->kid.get(), d, nullptr), d);
    SPHX_HIP(hipGetLastError());
    c->sched.cur ^= 1;
    c->slab_steps_enqueued += 1;
}

}  // namespace

SPHX_EXPORT int sphx_slab_compute(sphx_ctx *c, double *send_left_dev, double *send_right_dev, double *vmax_local_dev)
{
    SPHX_TRY
    require(c != nullptr && c->is_slab, "SPHX:Slab:ctx", "not a slab context");
    require(send_left_dev && send_right_dev && vmax_local_dev, "SPHX:Slab:buffers", "message / vmax buffers must not be NULL");
    require(c->rebuild_every == 1, "SPHX:Slab:protocol", "compute/finish drive a slab created with rebuild_every = 1");
    slab_compute_impl(c, send_left_dev, send_right_dev, vmax_local_dev);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_finish(sphx_ctx *c, const double *recv_left_dev, const double *recv_right_dev,
                                 const double *vmax_global_dev)
{
    SPHX_TRY
    require(c != nullptr && c->is_slab, "SPHX:Slab:ctx", "not a slab context");
    require(recv_left_dev && recv_right_dev && vmax_global_dev, "SPHX:Slab:buffers", "message / vmax buffers must not be NULL");
    require(c->rebuild_every == 1, "SPHX:Slab:protocol", "compute/finish drive a slab created with rebuild_every = 1");
    slab_finish_impl(c, recv_left_dev, recv_right_dev, vmax_global_dev);
    return SPHX_OK;
    SPHX_CATCH
}

// =================================================================================================
// Native step loop of the slabs: everything a step needs is enqueued from here, no host language in the loop.
//   sphx_slab_run        one context per process (one process per GPU): messages and the max all-reduce go through
//                        RCCL on the context's stream -- two sends + two receives in one group per step (ring
//                        neighbours: direct xGMI hops) and one 8-byte all-reduce;
//   sphx_slab_group_run  all slabs of the ring live in one process on one device (tests, rehearsals on a one-GPU box):
//                        the same loop with device-to-device copies as the transport and events for the ordering.
// Both are slab_run / slab_step over a transport (RcclRing, InProcessRing): every step form is stated once.
// librccl is loaded when the first communicator is made (dlopen: PyTorch carries its own copy of the library and the two
// must not be linked into one image twice), so a box without RCCL can still run everything single-GPU.
// =================================================================================================
namespace {

struct Rccl {
    void *lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;

    static Rccl &get()
    {
        static Rccl r;
        static bool ready = false;
        if (ready) return r;
        // resolve into a local table and publish it only when every entry point is there: a failed attempt leaves nothing
        // half-initialised behind (an older librccl lacking a symbol must fail every call, not only the first)
        Rccl t;
        std::string why;
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            t.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (t.lib) break;
            if (const char *e = dlerror()) why = e;
        }
        if (!t.lib) throw Error(SPHX_ERR_DEVICE, "SPHX:Slab:rccl", "cannot load librccl: " + why);
        auto sym = [&](const char *n) {
            void *p = dlsym(t.lib, n);
            if (!p) {
                (void)dlclose(t.lib);
                throw Error(SPHX_ERR_DEVICE, "SPHX:Slab:rccl", std::string("librccl lacks ") + n);
            }
            return p;
        };
        t.GetUniqueId = (decltype(t.GetUniqueId))sym("ncclGetUniqueId");
        t.CommInitRank = (decltype(t.CommInitRank))sym("ncclCommInitRank");
        t.CommDestroy = (decltype(t.CommDestroy))sym("ncclCommDestroy");
        t.GroupStart = (decltype(t.GroupStart))sym("ncclGroupStart");
        t.GroupEnd = (decltype(t.GroupEnd))sym("ncclGroupEnd");
        t.Send = (decltype(t.Send))sym("ncclSend");
        t.Recv = (decltype(t.Recv))sym("ncclRecv");
        t.AllReduce = (decltype(t.AllReduce))sym("ncclAllReduce");
        t.GetErrorString = (decltype(t.GetErrorString))sym("ncclGetErrorString");
        r = t;
        ready = true;
        return r;
    }
    void check(ncclResult_t e, const char *what)
    {
        if (e != ncclSuccess) throw Error(SPHX_ERR_DEVICE, "SPHX:Slab:rccl", std::string(what) + ": " + GetErrorString(e));
    }
};

// The RCCL calls of the native loop as functions of (communicator, ring neighbours; stream, buffers, counts): RcclRing issues
// them for a rank of a real ring, the self-tests on a communicator of one rank that is its own neighbour (left = right = 0).
struct Wire {
    Rccl &R;
    ncclComm_t comm;
    int left, right;
    // My left message is my left neighbour's "from the right" message and vice versa; with two ranks both go to the same
    // peer, which posts its receives in the order the sends are posted here.
    void ring(hipStream_t st, const void *to_l, const void *to_r, void *from_l, void *from_r, size_t count, ncclDataType_t ty)
    {
        R.check(R.GroupStart(), "ncclGroupStart");
        R.check(R.Send(to_l, count, ty, left, comm, st), "ncclSend");
        R.check(R.Send(to_r, count, ty, right, comm, st), "ncclSend");
        R.check(R.Recv(from_r, count, ty, right, comm, st), "ncclRecv");
        R.check(R.Recv(from_l, count, ty, left, comm, st), "ncclRecv");
        R.check(R.GroupEnd(), "ncclGroupEnd");
    }
    // the exchange of a skinned step: message A and the list ids of the previous step in ONE group (four sends, four receives)
    void ring_step(hipStream_t st, const double *msg_to_l, const double *msg_to_r, const int *ids_to_l, const int *ids_to_r,
                   double *msg_from_l, double *msg_from_r, int *ids_from_l, int *ids_from_r, size_t n_msg, size_t n_ids)
    {
        R.check(R.GroupStart(), "ncclGroupStart");
        R.check(R.Send(msg_to_l, n_msg, ncclDouble, left, comm, st), "ncclSend");
        R.check(R.Send(msg_to_r, n_msg, ncclDouble, right, comm, st), "ncclSend");
        R.check(R.Send(ids_to_l, n_ids, ncclInt32, left, comm, st), "ncclSend");
        R.check(R.Send(ids_to_r, n_ids, ncclInt32, right, comm, st), "ncclSend");
        R.check(R.Recv(msg_from_r, n_msg, ncclDouble, right, comm, st), "ncclRecv");
        R.check(R.Recv(msg_from_l, n_msg, ncclDouble, left, comm, st), "ncclRecv");
        R.check(R.Recv(ids_from_r, n_ids, ncclInt32, right, comm, st), "ncclRecv");
        R.check(R.Recv(ids_from_l, n_ids, ncclInt32, left, comm, st), "ncclRecv");
        R.check(R.GroupEnd(), "ncclGroupEnd");
    }
    void max(hipStream_t st, const double *mine, double *of_all, size_t count)
    {
        R.check(R.AllReduce(mine, of_all, count, ncclDouble, ncclMax, comm, st), "ncclAllReduce");
    }
};

void slab_native_buffers(sphx_ctx *c)
{
    if (c->msg_sl.get()) return;
    const size_t n = 1 + 7 * (size_t)c->msg_cap;
    c->msg_sl.alloc(n); c->msg_sr.alloc(n); c->msg_rl.alloc(n); c->msg_rr.alloc(n);
    c->vmax_l.alloc(2); c->vmax_g.alloc(2);
    for (DevBuf<double> *b : {&c->msg_sl, &c->msg_sr, &c->msg_rl, &c->msg_rr, &c->vmax_l, &c->vmax_g}) b->zero(c->stream);
    // The second stream of a skinned slab (k_slab_maxima beside pass E, the exchange beside the interior of pass A) -- where there
    // is something to hide the latencies behind: the two-stream step has five event hand-overs, one reduction kernel and one
    // launch of pass A more than the chain, ~15 us on the critical path of a slab whose passes take 5 us each (ring of two C2
    // slabs on one device 125 against 200-230 us/step), against an all-reduce and an exchange of 20-30 us each that pass E
    // (>= 20 us) and the interior of pass A (>= 25 us) cover from ~150 k particles per slab.  Ranks may decide differently
    // (unequal column counts): both forms issue the same sequence of RCCL calls.
    // SPHX_SLAB_OVERLAP=always|never (read when a slab's buffers are made, not once per process: the tests run both forms).
    const char *ov = std::getenv("SPHX_SLAB_OVERLAP");
    const bool ov_always = ov && std::strcmp(ov, "always") == 0, ov_never = ov && std::strcmp(ov, "never") == 0;
    if (c->rebuild_every > 1 && !debug_switches().no_slab_overlap && !ov_never && (c->cap >= 150000 || ov_always)) {
        SPHX_HIP(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
        SPHX_HIP(hipEventCreateWithFlags(&c->ev_cd, hipEventDisableTiming));
        SPHX_HIP(hipEventCreateWithFlags(&c->ev_ar, hipEventDisableTiming));
        SPHX_HIP(hipEventCreateWithFlags(&c->ev_max, hipEventDisableTiming));
        SPHX_HIP(hipEventCreateWithFlags(&c->ev_p, hipEventDisableTiming));
        SPHX_HIP(hipEventCreateWithFlags(&c->ev_u, hipEventDisableTiming));
        c->max_part.alloc(2 * kSlabMaxBlocks); c->max_part.zero(c->stream);
        c->ticket2.alloc(1); c->ticket2.zero(c->stream);
    }
    SPHX_HIP(hipStreamSynchronize(c->stream));
}

// End a capture that went wrong and drop whatever it produced.
void abandon_capture(hipStream_t st)
{
    hipGraph_t junk = nullptr;
    (void)hipStreamEndCapture(st, &junk);
    if (junk) (void)hipGraphDestroy(junk);
    (void)hipGetLastError();
}

struct PtrList {
    const double *p[16];
};
// max of one double per rank (single-process ring: stands in for the all-reduce)
__global__ void k_max_of(int n, PtrList src, double *out)  // thread j: component j of {max |v|, max drift}
{
    const int j = threadIdx.x;
    double m = src.p[0][j];
    for (int k = 1; k < n; ++k) m = fmax(m, src.p[k][j]);
    out[j] = m;
}

}  // namespace

SPHX_EXPORT int sphx_comm_available(void)
{
    SPHX_TRY
    (void)Rccl::get();  // loads librccl and resolves every entry point the native loop uses, or says what is missing
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_comm_unique_id(void *id_bytes, int capacity)
{
    SPHX_TRY
    require(id_bytes != nullptr && capacity >= NCCL_UNIQUE_ID_BYTES, "SPHX:Slab:rccl", "id buffer must hold 128 bytes");
    ncclUniqueId id;
    Rccl &R = Rccl::get();
    R.check(R.GetUniqueId(&id), "ncclGetUniqueId");
    std::memcpy(id_bytes, id.internal, NCCL_UNIQUE_ID_BYTES);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_comm_init(sphx_ctx *c, const void *id_bytes)
{
    SPHX_TRY
    require(c != nullptr && c->is_slab && id_bytes != nullptr, "SPHX:Slab:ctx", "not a slab context");
    require(c->comm == nullptr, "SPHX:Slab:rccl", "communicator already initialised");
    ncclUniqueId id;
    std::memcpy(id.internal, id_bytes, NCCL_UNIQUE_ID_BYTES);
    Rccl &R = Rccl::get();
    slab_native_buffers(c);  // (before the collective call: a rank that cannot allocate must not leave the others inside it)
    SPHX_HIP(hipStreamSynchronize(c->stream));
    ncclComm_t comm = nullptr;
    R.check(R.CommInitRank(&comm, c->n_ranks, id, c->rank), "ncclCommInitRank");
    c->comm = comm;
    return SPHX_OK;
    SPHX_CATCH
}

// The exchange patterns of sphx_slab_run on a communicator of ONE rank (its own neighbour on both sides): two sends and two
// receives in one group, then four and four with both element types (a skinned step) -- the receives must be served in the
// order of the sends, which is what the two-rank ring relies on -- then the 16-byte all-reduce(max).  Checks the dlopen'ed entry points, enum values and stream use on this machine.
SPHX_EXPORT int sphx_comm_selftest(void)
{
    SPHX_TRY
    ensure_device();
    Rccl &R = Rccl::get();
    ncclUniqueId id;
    R.check(R.GetUniqueId(&id), "ncclGetUniqueId");
    ncclComm_t comm = nullptr;
    R.check(R.CommInitRank(&comm, 1, id, 0), "ncclCommInitRank");
    hipStream_t st = nullptr;
    const size_t n = 1000;
    DevBuf<double> sl(n), sr(n), rl(n), rr(n), v(2), vg(2);
    DevBuf<int> il(n), ir(n), jl(n), jr(n);
    std::vector<double> hl(n), hr(n), got_l(n), got_r(n);
    std::vector<int> kl(n), kr(n), gi_l(n), gi_r(n);
    for (size_t k = 0; k < n; ++k) { hl[k] = 1.0 + k; hr[k] = -2.0 - k; kl[k] = 7 + (int)k; kr[k] = -9 - (int)k; }
    const double hv[2] = {3.25, -1.5};
    double gv[2] = {0.0, 0.0};
    bool ok = false;
    try {
        SPHX_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        sl.upload(hl.data(), n, st); sr.upload(hr.data(), n, st); il.upload(kl.data(), n, st); ir.upload(kr.data(), n, st);
        v.upload(hv, 2, st);
        rl.zero(st); rr.zero(st); jl.zero(st); jr.zero(st); vg.zero(st);
        Wire w{R, comm, 0, 0};
        w.ring(st, sl.get(), sr.get(), rl.get(), rr.get(), n, ncclDouble);
        w.ring(st, il.get(), ir.get(), jl.get(), jr.get(), n, ncclInt32);
        SPHX_HIP(hipMemcpyAsync(got_l.data(), rl.get(), n * sizeof(double), hipMemcpyDeviceToHost, st));
        SPHX_HIP(hipMemcpyAsync(got_r.data(), rr.get(), n * sizeof(double), hipMemcpyDeviceToHost, st));
        SPHX_HIP(hipMemcpyAsync(gi_l.data(), jl.get(), n * sizeof(int), hipMemcpyDeviceToHost, st));
        SPHX_HIP(hipMemcpyAsync(gi_r.data(), jr.get(), n * sizeof(int), hipMemcpyDeviceToHost, st));
        SPHX_HIP(hipStreamSynchronize(st));
        const bool ok_two = got_r == hl && got_l == hr && gi_r == kl && gi_l == kr;
        // ... and the exchange of a skinned step: both messages and both id lists in ONE group (four sends, four receives)
        rl.zero(st); rr.zero(st); jl.zero(st); jr.zero(st);
        w.ring_step(st, sl.get(), sr.get(), il.get(), ir.get(), rl.get(), rr.get(), jl.get(), jr.get(), n, n);
        w.max(st, v.get(), vg.get(), 2);
        SPHX_HIP(hipMemcpyAsync(got_l.data(), rl.get(), n * sizeof(double), hipMemcpyDeviceToHost, st));
        SPHX_HIP(hipMemcpyAsync(got_r.data(), rr.get(), n * sizeof(double), hipMemcpyDeviceToHost, st));
        SPHX_HIP(hipMemcpyAsync(gi_l.data(), jl.get(), n * sizeof(int), hipMemcpyDeviceToHost, st));
        SPHX_HIP(hipMemcpyAsync(gi_r.data(), jr.get(), n * sizeof(int), hipMemcpyDeviceToHost, st));
        SPHX_HIP(hipMemcpyAsync(gv, vg.get(), 2 * sizeof(double), hipMemcpyDeviceToHost, st));
        SPHX_HIP(hipStreamSynchronize(st));
        // what went to the left arrives "from the right" and vice versa
        ok = ok_two && got_r == hl && got_l == hr && gi_r == kl && gi_l == kr && gv[0] == hv[0] && gv[1] == hv[1];
    } catch (...) {
        (void)R.CommDestroy(comm);
        if (st) (void)hipStreamDestroy(st);
        throw;
    }
    R.check(R.CommDestroy(comm), "ncclCommDestroy");
    SPHX_HIP(hipStreamDestroy(st));
    if (!ok) throw Error(SPHX_ERR_DEVICE, "SPHX:Slab:rccl", "RCCL self-test: the exchanged data came back wrong");
    return SPHX_OK;
    SPHX_CATCH
}

// The exchange of a skinned step and the all-reduce once more, this time CAPTURED into a hipGraph and replayed twice with
// fresh payloads on a communicator of one rank: tells whether this RCCL can be captured at all (sphx_slab_graph_prepare
// relies on it) before a multi-rank run stakes its loop on it.
SPHX_EXPORT int sphx_comm_selftest_graph(void)
{
    SPHX_TRY
    ensure_device();
    Rccl &R = Rccl::get();
    ncclUniqueId id;
    R.check(R.GetUniqueId(&id), "ncclGetUniqueId");
    ncclComm_t comm = nullptr;
    R.check(R.CommInitRank(&comm, 1, id, 0), "ncclCommInitRank");
    hipStream_t st = nullptr;
    hipGraph_t g = nullptr;
    hipGraphExec_t exec = nullptr;
    const size_t n = 1000;
    DevBuf<double> sl(n), sr(n), rl(n), rr(n), v(2), vg(2);
    DevBuf<int> il(n), ir(n), jl(n), jr(n);
    std::vector<double> hl(n), hr(n), got_l(n), got_r(n);
    std::vector<int> kl(n), kr(n), gi_l(n), gi_r(n);
    bool ok = true;
    Wire w{R, comm, 0, 0};
    auto exchange = [&]() {
        w.max(st, v.get(), vg.get(), 2);
        w.ring_step(st, sl.get(), sr.get(), il.get(), ir.get(), rl.get(), rr.get(), jl.get(), jr.get(), n, n);
    };
    try {
        SPHX_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        rl.zero(st); rr.zero(st); jl.zero(st); jr.zero(st); vg.zero(st); v.zero(st); sl.zero(st); sr.zero(st); il.zero(st); ir.zero(st);
        exchange();  // eagerly first: channels and buffers of the communicator are set up outside the capture
        SPHX_HIP(hipStreamSynchronize(st));
        SPHX_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
        try {
            exchange();
            exchange();  // (two steps per graph, as the step graph holds several)
        } catch (...) {
            abandon_capture(st);
            throw;
        }
        SPHX_HIP(hipStreamEndCapture(st, &g));
        SPHX_HIP(hipGraphInstantiate(&exec, g, nullptr, nullptr, 0));
        for (int rep = 0; rep < 2 && ok; ++rep) {
            for (size_t k = 0; k < n; ++k) {
                hl[k] = 1.0 + k + 1000.0 * rep; hr[k] = -2.0 - k - 1000.0 * rep;
                kl[k] = 7 + (int)k + 100000 * rep; kr[k] = -9 - (int)k - 100000 * rep;
            }
            const double hv[2] = {3.25 + rep, -1.5 - rep};
            double gv[2] = {0.0, 0.0};
            sl.upload(hl.data(), n, st); sr.upload(hr.data(), n, st); il.upload(kl.data(), n, st); ir.upload(kr.data(), n, st);
            v.upload(hv, 2, st);
            rl.zero(st); rr.zero(st); jl.zero(st); jr.zero(st); vg.zero(st);
            SPHX_HIP(hipStreamSynchronize(st));  // (the host vectors are reused)
            SPHX_HIP(hipGraphLaunch(exec, st));
            SPHX_HIP(hipMemcpyAsync(got_l.data(), rl.get(), n * sizeof(double), hipMemcpyDeviceToHost, st));
            SPHX_HIP(hipMemcpyAsync(got_r.data(), rr.get(), n * sizeof(double), hipMemcpyDeviceToHost, st));
            SPHX_HIP(hipMemcpyAsync(gi_l.data(), jl.get(), n * sizeof(int), hipMemcpyDeviceToHost, st));
            SPHX_HIP(hipMemcpyAsync(gi_r.data(), jr.get(), n * sizeof(int), hipMemcpyDeviceToHost, st));
            SPHX_HIP(hipMemcpyAsync(gv, vg.get(), 2 * sizeof(double), hipMemcpyDeviceToHost, st));
            SPHX_HIP(hipStreamSynchronize(st));
            ok = got_r == hl && got_l == hr && gi_r == kl && gi_l == kr && gv[0] == hv[0] && gv[1] == hv[1];
        }
    } catch (...) {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (g) (void)hipGraphDestroy(g);
        (void)R.CommDestroy(comm);
        if (st) (void)hipStreamDestroy(st);
        throw;
    }
    (void)hipGraphExecDestroy(exec);
    (void)hipGraphDestroy(g);
    R.check(R.CommDestroy(comm), "ncclCommDestroy");
    SPHX_HIP(hipStreamDestroy(st));
    if (!ok) throw Error(SPHX_ERR_DEVICE, "SPHX:Slab:rccl", "RCCL graph self-test: a replayed exchange delivered the wrong data");
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_comm_destroy(sphx_ctx *c)
{
    SPHX_TRY
    require(c != nullptr && c->is_slab, "SPHX:Slab:ctx", "not a slab context");
    if (c->comm) {
        SPHX_HIP(hipStreamSynchronize(c->stream));
        Rccl &R = Rccl::get();
        R.check(R.CommDestroy(c->comm), "ncclCommDestroy");
        c->comm = nullptr;
    }
    return SPHX_OK;
    SPHX_CATCH
}

namespace {

// ---- one step of a skinned slab, in four phases separated by the three exchanges (see SlabLists) ----
FluidSet slab_new_state(sphx_ctx *c) { return c->view(1 - c->sched.cur, 0); }  // S[1-q] with the (in-place) layout arrays

constexpr int kTicketBlocks = 1024;  // largest grid of the kernels that end with last_workgroup_out (~20 ns per ticket)

// the step slot of parity q: S[q], and the passes' temporaries writing the new state into S[1-q]
struct SlabSlot {
    const int q;
    const FluidSet s, o;
    FluidTmp t;
    SlabSlot(sphx_ctx *c, int q_) : q(q_), s(c->view(q_, 0)), o(c->view(1 - q_, 0)), t(writing_into(c->tmp, o)) {}
};

void slab_phase1(sphx_ctx *c)  // passes A..E into S[1-q]; the tail workgroup of pass E leaves the local maxima in vmax_l[0..1]
{
    SlabSlot k(c, c->sched.cur);
    k.t.seal_out = c->vmax_l.get();
    launch_passes(c, k.q, k.s, k.t, PassA::DynBuildWalk, Tail::SlabMaxima);
}

// ... in three pieces (contexts with a second stream, see sphx_ctx::stream2): passes A, B, CD on the slab's stream; the local
// maxima -- both exist once pass CD is through -- on `aux`, where the all-reduce follows them; pass E, without a tail, on the
// slab's stream again, beside the two
void slab_phase1_abc(sphx_ctx *c)
{
    const SlabSlot k(c, c->sched.cur);
    // (the interior workgroups of this pass A may have run already, behind the previous step's pack3: slab_pass_a_interior)
    launch_pass_a(c, k.q, k.s, k.t, PassA::DynBuildWalk, c->a_interior_done ? SlabPart::Boundary : SlabPart::All);
    c->a_interior_done = false;
    launch_pass_b(c, k.q, k.s, k.t);
    launch_pass_cd(c, k.q, k.s, k.t);
}
// message A of the step being taken is packed, the clock advanced (the host's parity flips only in slab_phase4: q is the
// parity it will have): the interior workgroups of the NEXT step's pass A (the step slot of parity q) need nothing the
// exchange brings -- they run while it is under way
void slab_pass_a_interior(sphx_ctx *c, int q)
{
    const SlabSlot k(c, q);
    launch_pass_a(c, k.q, k.s, k.t, PassA::SlabWalk, SlabPart::Interior);
    c->a_interior_done = true;
}
void slab_local_maxima_of_step(sphx_ctx *c, hipStream_t aux)
{
    const SlabSlot k(c, c->sched.cur);
    hipLaunchKernelGGL(k_slab_maxima, dim3(kSlabMaxBlocks), dim3(kBlock), 0, aux, (const Clock *)c->clock.get(), k.q, c->grid,
                       c->n_vpart, (const double *)c->dpart.get(), (const double2 *)k.o.vel, (const int *)k.s.cell, c->max_part.get(),
                       c->vmax_l.get(), c->ticket2.get());
}
void slab_phase1_e(sphx_ctx *c)
{
    const SlabSlot k(c, c->sched.cur);
    launch_pass_e(c, k.q, k.s, k.t);
}

void slab_phase2(sphx_ctx *c)  // global maxima known: re-binning decision, message A, clock -- one launch
{
    const int q = c->sched.cur;
    SlabPack p = c->pack;
    p.send_l = c->msg_sl.get();
    p.send_r = c->msg_sr.get();
    // grid-stride on at most one workgroup per CU: the kernel ends with a ticket per workgroup (last_workgroup_out)
    const unsigned nb = std::min<unsigned>(kTicketBlocks, std::max<unsigned>(c->n_blocks_flat, div_up((size_t)2 * c->msg_cap, kBlock)));
    launch(c, "k_slab_pack3", k_slab_pack3, dim3(nb), dim3(kBlock), c->clock.get(), q, c->grid, c->phys, slab_new_state(c), p,
           c->lists, (const double *)c->vmax_g.get(), c->flags.get(), c->half_skin(), c->rebuild_every, c->ticket.get());
}

void slab_phase3(sphx_ctx *c)  // message A arrived (and with it the ids of the lists the neighbours made in the previous step):
                               // refresh the halo copies, or re-bin and make the lists of the next cycle
{
    const int q = c->sched.cur, qf = q | kOnlyIfRebuild;
    Clock *clk = c->clock.get();
    const FluidSet d = slab_new_state(c);
    launch(c, "k_slab_unpack3", k_slab_unpack3, dim3(div_up((size_t)2 * c->msg_cap, kBlock)), dim3(kBlock), clk, q, c->grid, d,
           c->pack, c->lists, (const double *)c->msg_rl.get(), (const double *)c->msg_rr.get(), (const int *)c->ids_r_[0].get(),
           (const int *)c->ids_r_[1].get(), c->n_new.get(), c->flags.get(), c->ticket.get());
    const int kRebinBlocks = 4096;  // grid-stride: on the steps that do not re-bin these launches return at once
    launch_cell_scan(c, clk, qf, c->count.get(), d.start);
    launch_scatter_reorder(c, qf,
                           reorder_args(c->kpos.get(), c->kvel.get(), c->kdrho.get(), c->kmass.get(), c->kid.get(), d, nullptr,
                                        c->slot_of_id.get()),
                           d, kRebinBlocks);
    launch(c, "k_slab_sendlist", k_slab_sendlist, dim3(std::min(c->n_blocks_flat, kTicketBlocks)), dim3(kBlock), (const Clock *)clk,
           q, c->grid, d, c->pack, c->lists, c->flags.get(), 0, c->ticket.get());
}

void slab_phase4(sphx_ctx *c)  // host bookkeeping of the step (the ids made in phase 3 travel with the next step's message A)
{
    SPHX_HIP(hipGetLastError());
    c->sched.cur ^= 1;
    c->slab_steps_enqueued += 1;
}

// the exchange lists of the first cycle (the layout of slab_setup): send lists + ids out, then (ids in) receive slots
void slab_lists_out(sphx_ctx *c)
{
    const FluidSet d = c->view(c->sched.cur, 0);
    SPHX_HIP(hipMemsetAsync(c->send_cnt.get(), 0, 2 * sizeof(int), c->stream));
    hipLaunchKernelGGL(k_slab_sendlist, dim3(std::min(c->n_blocks_flat, kTicketBlocks)), dim3(kBlock), 0, c->stream,
                       (const Clock *)c->clock.get(), 0, c->grid, d, c->pack, c->lists, c->flags.get(), 1, c->ticket.get());
}
void slab_lists_in(sphx_ctx *c)
{
    hipLaunchKernelGGL(k_slab_recvslots, dim3(div_up((size_t)2 * c->msg_cap, kBlock)), dim3(kBlock), 0, c->stream,
                       (const Clock *)c->clock.get(), 0, c->pack, c->lists, (const int *)c->ids_r_[0].get(),
                       (const int *)c->ids_r_[1].get(), (const int *)c->view(c->sched.cur, 0).id, c->flags.get(), 1);
    SPHX_HIP(hipGetLastError());
    c->lists_ready = true;
}

void slab_local_maxima(sphx_ctx *c)  // arming: max |v| of the owned particles of the current state, drift 0
{
    const FluidSet fs = c->view(c->sched.cur, c->rebuild_every > 1 ? 0 : c->sched.cur);
    SPHX_HIP(hipMemsetAsync(c->vmax_l.get(), 0, 2 * sizeof(double), c->stream));
    hipLaunchKernelGGL(k_vmax_init, dim3(1), dim3(kScanBlock), 0, c->stream, c->clock.get(), c->grid, (const double2 *)fs.pos,
                       (const double2 *)fs.vel, c->vmax_l.get(), (const int *)fs.cell);
}

}  // namespace

namespace {

constexpr int kSlabGraphSteps = 10;  // steps per replay of a slab's step graph (even: the state parity comes back)

// ---- The transports beneath the step: which slabs this process drives, the all-reduce(max) of vmax_l into vmax_g, the three
// exchanges (messages; ids; both in one group), the phase boundaries.  The step forms below are written once against them -- a
// template parameter, as Forms is in the launch layer: no virtual call on the step path -- so the in-process ring of the tests
// runs the statements the RCCL loop runs.  What really differs between the two is a named member with its reason. ----
using SlabEvent = hipEvent_t sphx_ctx::*;

// what `to` gets from here on comes after what `from` has got so far
void order_after(hipEvent_t ev, hipStream_t from, hipStream_t to)
{
    SPHX_HIP(hipEventRecord(ev, from));
    SPHX_HIP(hipStreamWaitEvent(to, ev, 0));
}

// one rank per process: RCCL on the slab's streams.  RCCL orders the ranks by itself: the phase boundaries are empty.
struct RcclRing {
    sphx_ctx *c;
    Wire w;
    size_t n_msg, n_ids;
    bool captured = false;  // under stream capture: everything on the one capturing stream
    explicit RcclRing(sphx_ctx *ctx)
        : c(ctx), w{Rccl::get(), ctx->comm, (ctx->rank + ctx->n_ranks - 1) % ctx->n_ranks, (ctx->rank + 1) % ctx->n_ranks},
          n_msg(1 + 7 * (size_t)ctx->msg_cap), n_ids(1 + (size_t)ctx->msg_cap) {}
    sphx_ctx **begin() { return &c; }
    sphx_ctx **end() { return &c + 1; }
    // the protocol form reduces max |v| alone (8 bytes on the wire per step): nothing measures a drift when every step re-bins
    static constexpr size_t kProtocolMaxima = 1;
    // a captured split step does not launch the interior of the next pass A: on one stream the early launch hides nothing and
    // costs a launch per step
    static constexpr bool kInteriorWhenCaptured = false;
    void all_reduce(sphx_ctx *, hipStream_t st, size_t count) { w.max(st, c->vmax_l.get(), c->vmax_g.get(), count); }
    void exchange_msgs(sphx_ctx *, hipStream_t st)
    {
        w.ring(st, c->msg_sl.get(), c->msg_sr.get(), c->msg_rl.get(), c->msg_rr.get(), n_msg, ncclDouble);
    }
    void exchange_ids(sphx_ctx *, hipStream_t st)
    {
        w.ring(st, c->ids_s_[0].get(), c->ids_s_[1].get(), c->ids_r_[0].get(), c->ids_r_[1].get(), n_ids, ncclInt32);
    }
    void exchange_step(sphx_ctx *, hipStream_t st)
    {
        w.ring_step(st, c->msg_sl.get(), c->msg_sr.get(), c->ids_s_[0].get(), c->ids_s_[1].get(), c->msg_rl.get(), c->msg_rr.get(),
                    c->ids_r_[0].get(), c->ids_r_[1].get(), n_msg, n_ids);
    }
    void done(sphx_ctx *, SlabEvent, hipStream_t) {}
    void done_all(SlabEvent) {}
    void wait_others(sphx_ctx *, SlabEvent, hipStream_t) {}
    void gather_on_first() {}  // (a replay of the step graph: one stream, nothing to order)
    void release_from_first() {}
    // The split form's exchange and phase 3 run on the second stream, beside the interior workgroups of the next step's pass A:
    // the point-to-point latencies are what the split hides.  ev_p: "message A is packed", ev_u: "the halo is refreshed".
    hipStream_t exchange_stream(sphx_ctx *) const { return captured ? c->stream : c->stream2; }
    void hand_over(sphx_ctx *) { if (!captured) order_after(c->ev_p, c->stream, c->stream2); }
    void hand_back(sphx_ctx *) { if (!captured) order_after(c->ev_u, c->stream2, c->stream); }
};

// all slabs of the ring in one process on one device: k_max_of and device-to-device copies, events for the ordering
struct InProcessRing {
    sphx_ctx **ctxs;
    int n;
    PtrList vls{};
    size_t msg_bytes, ids_bytes;
    bool captured = false;  // every slab enqueues on the same stream: stream order is the only ordering needed
    InProcessRing(sphx_ctx **cs, int count) : ctxs(cs), n(count)
    {
        for (int r = 0; r < n; ++r) vls.p[r] = ctxs[r]->vmax_l.get();
        msg_bytes = (1 + 7 * (size_t)ctxs[0]->msg_cap) * sizeof(double);
        ids_bytes = (1 + (size_t)ctxs[0]->msg_cap) * sizeof(int);
    }
    sphx_ctx **begin() { return ctxs; }
    sphx_ctx **end() { return ctxs + n; }
    static constexpr size_t kProtocolMaxima = 2;  // k_max_of costs the same for both components (the drift entry is 0)
    // under capture the interior of the next pass A is still launched early: what the ring tests is the split of pass A itself
    static constexpr bool kInteriorWhenCaptured = true;
    sphx_ctx *left_of(sphx_ctx *c) const { return ctxs[(c->rank + n - 1) % n]; }
    sphx_ctx *right_of(sphx_ctx *c) const { return ctxs[(c->rank + 1) % n]; }
    void all_reduce(sphx_ctx *c, hipStream_t st, size_t count)  // thread j: component j
    {
        hipLaunchKernelGGL(k_max_of, dim3(1), dim3((unsigned)count), 0, st, n, vls, c->vmax_g.get());
    }
    void exchange_msgs(sphx_ctx *c, hipStream_t st)  // what my ring neighbours addressed to me
    {
        SPHX_HIP(hipMemcpyAsync(c->msg_rl.get(), left_of(c)->msg_sr.get(), msg_bytes, hipMemcpyDeviceToDevice, st));
        SPHX_HIP(hipMemcpyAsync(c->msg_rr.get(), right_of(c)->msg_sl.get(), msg_bytes, hipMemcpyDeviceToDevice, st));
    }
    void exchange_ids(sphx_ctx *c, hipStream_t st)
    {
        SPHX_HIP(hipMemcpyAsync(c->ids_r_[0].get(), left_of(c)->ids_s_[1].get(), ids_bytes, hipMemcpyDeviceToDevice, st));
        SPHX_HIP(hipMemcpyAsync(c->ids_r_[1].get(), right_of(c)->ids_s_[0].get(), ids_bytes, hipMemcpyDeviceToDevice, st));
    }
    void exchange_step(sphx_ctx *c, hipStream_t st) { exchange_msgs(c, st); exchange_ids(c, st); }
    // A phase boundary of the ring: every slab records "my outputs of this phase are complete" and, before it touches
    // anything another slab produced (or overwrites what another slab may still be reading), waits for all the others.
    void done(sphx_ctx *c, SlabEvent ev, hipStream_t st) { if (!captured) SPHX_HIP(hipEventRecord(c->*ev, st)); }
    void done_all(SlabEvent ev) { for (sphx_ctx *c : *this) done(c, ev, c->stream); }
    void wait_others(sphx_ctx *c, SlabEvent ev, hipStream_t st)
    {
        if (captured) return;
        for (sphx_ctx *o : *this) if (o != c) SPHX_HIP(hipStreamWaitEvent(st, o->*ev, 0));
    }
    // the copies that stand in for the exchange, and phase 3 behind them, stay on the slab's own stream: the neighbours wait for
    // this slab's message A at ev_received, recorded in front of the interior of pass A, and need no second hand-over
    hipStream_t exchange_stream(sphx_ctx *c) const { return c->stream; }
    void hand_over(sphx_ctx *) {}
    void hand_back(sphx_ctx *) {}
    // a replay of slab 0's step graph: everything the slabs enqueued before it is ordered ahead of it, everything they enqueue
    // afterwards behind it
    void gather_on_first() { for (int r = 1; r < n; ++r) order_after(ctxs[r]->ev_join, ctxs[r]->stream, ctxs[0]->stream); }
    void release_from_first()
    {
        SPHX_HIP(hipEventRecord(ctxs[0]->ev_fork, ctxs[0]->stream));
        for (int r = 1; r < n; ++r) SPHX_HIP(hipStreamWaitEvent(ctxs[r]->stream, ctxs[0]->ev_fork, 0));
    }
};

// slab_phase3 enqueues on "the" stream of its context: run it on another one for a scope
struct OnStream {
    sphx_ctx *c;
    hipStream_t own;
    OnStream(sphx_ctx *ctx, hipStream_t st) : c(ctx), own(ctx->stream) { c->stream = st; }
    ~OnStream() { c->stream = own; }
};

// ---- the three forms of a step.  Each starts with the slabs waiting until the others have consumed their previous messages
// and maxima (ev_received). ----

// rebuild_every = 1, the protocol of compute / finish: re-binning every step, whole messages
template <typename T> void step_protocol(T &t)
{
    for (sphx_ctx *c : t) {
        t.wait_others(c, &sphx_ctx::ev_received, c->stream);
        slab_compute_impl(c, c->msg_sl.get(), c->msg_sr.get(), c->vmax_l.get());
    }
    t.done_all(&sphx_ctx::ev_computed);
    for (sphx_ctx *c : t) {
        t.wait_others(c, &sphx_ctx::ev_computed, c->stream);
        t.all_reduce(c, c->stream, T::kProtocolMaxima);
        t.exchange_msgs(c, c->stream);
    }
    t.done_all(&sphx_ctx::ev_received);
    for (sphx_ctx *c : t) slab_finish_impl(c, c->msg_rl.get(), c->msg_rr.get(), c->vmax_g.get());
}

// second half of both skinned forms: message A and the ids of the previous step's lists in; halo refresh or re-binning chain
// (the lists / ids of the next cycle overwrite the old ones); host bookkeeping.  split: on the transport's exchange stream.
template <typename T> void step_exchange_and_after(T &t, bool split)
{
    auto xs = [&](sphx_ctx *c) { return split ? t.exchange_stream(c) : c->stream; };
    for (sphx_ctx *c : t) {
        t.wait_others(c, &sphx_ctx::ev_received, c->stream);
        t.exchange_step(c, xs(c));
    }
    t.done_all(&sphx_ctx::ev_computed);  // (reused: "I have taken what the neighbours addressed to me")
    for (sphx_ctx *c : t) {
        t.wait_others(c, &sphx_ctx::ev_computed, c->stream);
        { OnStream on(c, xs(c)); slab_phase3(c); }
        if (split) t.hand_back(c);
        slab_phase4(c);
    }
    t.done_all(&sphx_ctx::ev_received);
}

// the skinned step as one chain per slab (below ~150 k particles per slab, see slab_native_buffers)
template <typename T> void step_chain(T &t)
{
    for (sphx_ctx *c : t) {
        t.wait_others(c, &sphx_ctx::ev_received, c->stream);
        slab_phase1(c);
    }
    t.done_all(&sphx_ctx::ev_computed);
    for (sphx_ctx *c : t) {  // all-reduce, decision, message A
        t.wait_others(c, &sphx_ctx::ev_computed, c->stream);
        t.all_reduce(c, c->stream, 2);
        slab_phase2(c);
    }
    t.done_all(&sphx_ctx::ev_received);  // (reused: "my maxima have been read by me, my message A is complete")
    for (sphx_ctx *c : t) launch_slab_samplers(c);  // (in front of the exchange and phase 3, which follow on this stream)
    step_exchange_and_after(t, false);
}

// The skinned step on two streams: passes A, B, CD; the local maxima and the all-reduce on the second stream (fork ev_cd, join
// ev_ar in front of pack3) beside pass E; the exchange beside the interior workgroups of the next step's pass A.  Under stream
// capture (t.captured): the same pieces in one chain on the capturing stream, no events.
template <typename T> void step_split(T &t)
{
    const bool two = !t.captured;
    auto aux = [&](sphx_ctx *c) { return two ? c->stream2 : c->stream; };
    for (sphx_ctx *c : t) {
        t.wait_others(c, &sphx_ctx::ev_received, c->stream);
        slab_phase1_abc(c);
        if (two) order_after(c->ev_cd, c->stream, c->stream2);
        slab_local_maxima_of_step(c, aux(c));
        t.done(c, &sphx_ctx::ev_max, aux(c));  // "my local maxima are out"
    }
    for (sphx_ctx *c : t) {  // all-reduce beside pass E, decision, message A
        t.wait_others(c, &sphx_ctx::ev_max, aux(c));
        t.all_reduce(c, aux(c), 2);
        slab_phase1_e(c);
        if (two) order_after(c->ev_ar, c->stream2, c->stream);
        slab_phase2(c);
        // "my maxima have been read by me, my message A is complete" -- recorded HERE, in front of the interior workgroups of
        // the next step's pass A, which the neighbours need not wait for
        t.done(c, &sphx_ctx::ev_received, c->stream);
        // The samplers read S[1-q], Vol / B and the cell array of the step: in front of the hand-over, behind which phase 3 may
        // overwrite the first and the last on the exchange stream, and in front of the interior of the next pass A, which
        // overwrites Vol
        launch_slab_samplers(c);
        t.hand_over(c);
        if (two || T::kInteriorWhenCaptured) slab_pass_a_interior(c, 1 - c->sched.cur);  // (phase 4 flips the parity)
    }
    step_exchange_and_after(t, true);
}

// what the slabs' enable / disable calls of their samplers have counted up so far (sphx_ctx::sampler_epoch)
template <typename T> int64_t sampler_epochs(T &t)
{
    int64_t sum = 0;
    for (sphx_ctx *c : t) sum += c->sampler_epoch;
    return sum;
}

template <typename T> void slab_step(T &t)
{
    const sphx_ctx *c0 = *t.begin();
    if (c0->rebuild_every <= 1) step_protocol(t);
    else if (c0->stream2) step_split(t);
    else step_chain(t);
}

template <typename T> void slab_replay(T &t)  // one replay of the step graph, on the first slab's stream
{
    sphx_ctx *c0 = *t.begin();
    t.gather_on_first();
    SPHX_HIP(hipGraphLaunch(c0->steps_graph, c0->stream));
    t.release_from_first();
    t.done_all(&sphx_ctx::ev_received);  // (the eager steps that may follow wait for these)
    for (sphx_ctx *c : t) { c->slab_steps_enqueued += kSlabGraphSteps; c->a_interior_done = false; }
}

// n_steps steps of the slabs of t: arm, first exchange lists, whole replays of the step graph, the rest step by step
template <typename T> void slab_run(T &t, double t_target, int64_t n_steps)
{
    const sphx_ctx *c0 = *t.begin();
    const bool skinned = c0->rebuild_every > 1;
    // Arm the clock with the global max |v| of the current state: after a step the clock holds it already (the all-reduced
    // value that step's dt rule used); only a state that has never been stepped needs the reduction (k_vmax_init is one
    // workgroup over the whole slab: 0.9 ms at 0.76 M particles)
    bool fresh_state = false;
    for (sphx_ctx *c : t) {
        c->a_interior_done = false;  // (whatever the previous call launched ahead found the loop stopped: the first step sweeps / walks everything)
        fresh_state = fresh_state || c->slab_steps_enqueued == 0;
    }
    for (sphx_ctx *c : t) if (fresh_state) slab_local_maxima(c);
    t.done_all(&sphx_ctx::ev_computed);
    for (sphx_ctx *c : t) {
        t.wait_others(c, &sphx_ctx::ev_computed, c->stream);
        if (fresh_state) t.all_reduce(c, c->stream, 2);
        arm_clock(c, t_target, (long long)n_steps, c->sched.cur, fresh_state ? (const double *)c->vmax_g.get() : (const double *)nullptr);
        if (skinned && !c->lists_ready) slab_lists_out(c);
    }
    t.done_all(&sphx_ctx::ev_received);
    if (skinned && !c0->lists_ready) {
        for (sphx_ctx *c : t) {
            t.wait_others(c, &sphx_ctx::ev_received, c->stream);
            t.exchange_ids(c, c->stream);
            slab_lists_in(c);
        }
        t.done_all(&sphx_ctx::ev_received);
    }
    int64_t k = 0;
    if (c0->steps_graph && c0->steps_graph_cur == c0->sched.cur && c0->steps_graph_epochs == sampler_epochs(t) &&
        // whole replays of the step graph (sphx_slab_graph_prepare) ...
        std::equal(t.begin(), t.end(), c0->steps_graph_ring.begin(), c0->steps_graph_ring.end()))
        for (; n_steps - k >= kSlabGraphSteps; k += kSlabGraphSteps) slab_replay(t);
    for (; k < n_steps; ++k) slab_step(t);  // ... the rest step by step
    SPHX_HIP(hipGetLastError());
}

void check_ring(sphx_ctx **ctxs, int n)
{
    require(ctxs != nullptr && n >= 2 && n <= 16, "SPHX:Slab:group", "a ring needs 2..16 slab contexts");
    for (int r = 0; r < n; ++r) {
        sphx_ctx *c = ctxs[r];
        require(c != nullptr && c->is_slab && c->rank == r && c->n_ranks == n, "SPHX:Slab:group",
                "ctxs[r] must be slab r of an n-slab ring");
        require(c->msg_cap == ctxs[0]->msg_cap && c->rebuild_every == ctxs[0]->rebuild_every, "SPHX:Slab:group",
                "slabs of one ring share the message capacity and the re-binning interval");
        slab_native_buffers(c);
        if (!c->ev_computed) {
            SPHX_HIP(hipEventCreateWithFlags(&c->ev_computed, hipEventDisableTiming));
            SPHX_HIP(hipEventCreateWithFlags(&c->ev_received, hipEventDisableTiming));
            SPHX_HIP(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
            SPHX_HIP(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
        }
    }
}

}  // namespace

SPHX_EXPORT int sphx_slab_run(sphx_ctx *c, double t_target, int64_t n_steps)
{
    SPHX_TRY
    require(c != nullptr && c->is_slab, "SPHX:Slab:ctx", "not a slab context");
    require(c->comm != nullptr, "SPHX:Slab:rccl", "sphx_slab_comm_init first");
    require(n_steps > 0, "SPHX:Ctx:steps", "n_steps must be positive");
    RcclRing t(c);
    slab_run(t, t_target, n_steps);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_group_run(sphx_ctx **ctxs, int n, double t_target, int64_t n_steps)
{
    SPHX_TRY
    check_ring(ctxs, n);
    require(n_steps > 0, "SPHX:Ctx:steps", "n_steps must be positive");
    InProcessRing t(ctxs, n);
    slab_run(t, t_target, n_steps);
    return SPHX_OK;
    SPHX_CATCH
}

namespace {

template <typename T> void slab_graph_prepare(T &t)
{
    sphx_ctx *c0 = *t.begin();
    for (sphx_ctx *c : t) {
        require(c->lists_ready && c->slab_steps_enqueued >= 2, "SPHX:Slab:graph",
                "run at least two steps before capturing the step graph");
        SPHX_HIP(hipStreamSynchronize(c->stream));
    }
    if (c0->steps_graph) { (void)hipGraphExecDestroy(c0->steps_graph); c0->steps_graph = nullptr; }
    const int64_t enq0 = c0->slab_steps_enqueued;
    const int cur0 = c0->sched.cur;
    hipStream_t s0 = c0->stream;
    hipGraph_t g = nullptr;
    // An in-process ring is captured as ONE chain on slab 0's stream (the slabs take turns phase by phase): a graph whose
    // branches meet at every phase boundary replays slower than the eager loop on ROCm 7.2 (0.25 M particles per slab: 334
    // against 289 us/step), and the slabs of a ring share one device anyway.
    std::vector<hipStream_t> own_streams;
    for (sphx_ctx *c : t) {
        own_streams.push_back(c->stream);
        c->stream = s0;
        c->a_interior_done = false;  // (the graph's first step sweeps / walks everything)
    }
    auto restore_streams = [&]() { size_t r = 0; for (sphx_ctx *c : t) c->stream = own_streams[r++]; };
    hipError_t e_end = hipSuccess;
    {
        CaptureScope capturing;
        const hipError_t e_begin = hipStreamBeginCapture(s0, hipStreamCaptureModeRelaxed);
        if (e_begin != hipSuccess) { restore_streams(); SPHX_HIP(e_begin); }
        t.captured = true;
        try {
            for (int k = 0; k < kSlabGraphSteps; ++k) slab_step(t);
        } catch (...) {
            abandon_capture(s0);
            restore_streams();
            for (sphx_ctx *c : t) { c->sched.cur = cur0; c->slab_steps_enqueued = enq0; }
            throw;
        }
        t.captured = false;
        restore_streams();
        for (sphx_ctx *c : t) { c->slab_steps_enqueued -= kSlabGraphSteps; c->a_interior_done = false; }  // nothing has executed
        e_end = hipStreamEndCapture(s0, &g);
    }
    if (e_end != hipSuccess) { (void)hipGetLastError(); if (g) (void)hipGraphDestroy(g); SPHX_HIP(e_end); }
    hipGraphExec_t exec = nullptr;
    const hipError_t e_inst = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    SPHX_HIP(e_inst);
    // warm replay with the clock disarmed: every kernel returns at once, the messages that travel are ignored (ids made by
    // the last real step are delivered -- that is what the next real step would have done first)
    for (sphx_ctx *c : t) hipLaunchKernelGGL(k_disarm, dim3(1), dim3(1), 0, c->stream, c->clock.get());
    c0->steps_graph = exec;
    c0->steps_graph_cur = cur0;
    c0->steps_graph_ring.assign(t.begin(), t.end());
    c0->steps_graph_epochs = sampler_epochs(t);
    slab_replay(t);
    for (sphx_ctx *c : t) {
        c->slab_steps_enqueued -= kSlabGraphSteps;  // (the warm replay stepped nothing)
        SPHX_HIP(hipStreamSynchronize(c->stream));
    }
}

}  // namespace

// Capture kSlabGraphSteps whole steps of the native loop into one graph; sphx_slab_run / sphx_slab_group_run then replay it
// for every full batch of that many steps and launch only the remainder step by step.  n = 1: the context of this
// process's rank (sphx_slab_run; the RCCL calls are captured with the kernels -- every rank of the communicator must
// make this call at the same point of its sequence, because the graph is warmed with one idle replay that exchanges
// messages); n >= 2: an in-process ring (the graph is held by slab 0).  The loop must have run at least two steps
// (communicator channels, exchange lists and pools are set up by then: nothing may allocate during capture).  Without
// this call the loops stay eager; a failed capture leaves them eager and reports the error.
SPHX_EXPORT int sphx_slab_graph_prepare(sphx_ctx **ctxs, int n)
{
    SPHX_TRY
    require(ctxs != nullptr && n >= 1 && ctxs[0] != nullptr && ctxs[0]->is_slab, "SPHX:Slab:ctx", "not a slab context");
    require(ctxs[0]->rebuild_every > 1, "SPHX:Slab:protocol", "step graphs are for skinned slabs (rebuild_every != 1)");
    if (n == 1) {  // (the one choice of transport)
        require(ctxs[0]->comm != nullptr, "SPHX:Slab:rccl", "sphx_slab_comm_init first");
        RcclRing t(ctxs[0]);
        slab_graph_prepare(t);
    } else {
        check_ring(ctxs, n);
        InProcessRing t(ctxs, n);
        slab_graph_prepare(t);
    }
    return SPHX_OK;
    SPHX_CATCH
}

// wait for the stream, verify that every enqueued slab step really executed, report the clock
SPHX_EXPORT int sphx_slab_sync(sphx_ctx *c, sphx_status *status)
{
    SPHX_TRY
    require(c != nullptr && c->is_slab, "SPHX:Slab:ctx", "not a slab context");
    SPHX_HIP(hipMemcpyAsync(c->h_clock, c->clock.get(), sizeof(Clock), hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(hipStreamSynchronize(c->stream));
    c->timer.collect();
    fill_status(c, status);
    const int64_t executed = (int64_t)c->h_clock->step - c->slab_step0;
    throw_on_status(c);
    if (executed != c->slab_steps_enqueued)
        throw Error(SPHX_ERR_STATE, "SPHX:Slab:overrun", "a slab step was enqueued after the loop had stopped");
    return SPHX_OK;
    SPHX_CATCH
}

// copy the current particles of the slab to host arrays of `capacity` entries; *n = count.  owned[i]
// tells whether particle i belongs to this rank (the rest are halo copies).
SPHX_EXPORT int sphx_slab_snapshot(sphx_ctx *c, int capacity, int *n, double *x, double *y, double *vx, double *vy,
                                   double *drho, int *id, int *owned)
{
    SPHX_TRY
    require(c != nullptr && c->is_slab && n != nullptr, "SPHX:Slab:ctx", "not a slab context");
    SPHX_HIP(hipMemcpyAsync(c->h_clock, c->clock.get(), sizeof(Clock), hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(hipStreamSynchronize(c->stream));
    const int m = c->h_clock->n;
    *n = m;
    require(capacity >= m, "SPHX:Slab:capacity", "snapshot arrays are too short");
    const bool skinned = c->rebuild_every > 1;
    const FluidSet fs = c->view(c->sched.cur, skinned ? 0 : c->sched.cur);
    hipStream_t s = c->stream;
    auto dl = [&](const void *src, void *dst, size_t bytes) {
        if (dst && m) SPHX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
    };
    std::vector<double2> hp((size_t)std::max(m, 1)), hv((size_t)std::max(m, 1));
    std::vector<int> hcell((size_t)std::max(m, 1), 0);
    dl(fs.pos, hp.data(), (size_t)m * 16); dl(fs.vel, hv.data(), (size_t)m * 16);
    dl(fs.drho, drho, (size_t)m * 8); dl(fs.id, id, (size_t)m * 4);
    if (skinned) dl(fs.cell, hcell.data(), (size_t)m * 4);  // ownership goes by the binned column
    SPHX_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < m; ++i) {
        if (x) x[i] = hp[i].x;
        if (y) y[i] = hp[i].y;
        if (vx) vx[i] = hv[i].x;
        if (vy) vy[i] = hv[i].y;
        if (owned) {
            const int cx = hcell[i] / c->grid.ncy;
            owned[i] = skinned ? (cx >= c->grid.own_c0 && cx < c->grid.own_c1) : (hp[i].x >= c->grid.own_lo && hp[i].x < c->grid.own_hi);
        }
    }
    return SPHX_OK;
    SPHX_CATCH
}

// Average duration of one neighbour-pass kernel in the hipGraph-replay regime: `reps` back-to-back launches of
// that kernel alone are captured in a graph and replayed between two HIP events on the context's stream.  The
// passes only write per-step temporaries (continuity runs without its histogram), so the state is unchanged.
// This is the same quantity rocprofv3's kernel trace reports for the timed region (start of a dispatch to its
// end, dispatch gap included); the eager event-pair numbers of sphx_ctx_profile_* carry extra launch overhead
// at small particle counts.
SPHX_EXPORT int sphx_ctx_time_kernel(sphx_ctx *c, const char *name, int reps, double *avg_ms)
{
    SPHX_TRY
    require(c != nullptr && name != nullptr && avg_ms != nullptr && reps > 0, "SPHX:Ctx:null", "bad arguments");
    require(!c->is_slab, "SPHX:Ctx:slab", "not available on a slab context");
    const std::string n(name);
    enum class Pass { None, A, B, CD, E, EA } pass = Pass::None;
    if (n == "k_density" || n == "k_density_build" || n == "k_density_walk" || n == "k_density_dyn") pass = Pass::A;
    else if (n == "k_kgc") pass = Pass::B;
    else if (n == "k_forces") pass = Pass::CD;
    else if (n == "k_continuity" || n == "k_continuity_clock") pass = Pass::E;
    else if (n == "k_continuity_density" && c->fuse_ea) pass = Pass::EA;  // pass E and the next pass A in one launch
    require(pass != Pass::None, "SPHX:Ctx:kernel", "time_kernel knows k_density, k_kgc, k_forces, k_continuity (and k_continuity_density)");
    read_clock(c);
    if (c->h_clock->need_rebuild && c->h_clock->status == 0) forced_rebuild(c);
    const bool prof = c->profiling;
    c->profiling = false;
    hipGraph_t g = nullptr;
    hipGraphExec_t e = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    try {
        // arm run[cur] so the kernels execute; no step slot follows, so the clock does not advance
        arm_clock(c, c->prm.t_end, (long long)1, c->sched.cur, (const double *)nullptr);
        const int q = c->sched.cur;
        const FluidSet fs = c->view(q, c->sched.lay);
        const PassA mode = c->dyn ? PassA::DynBuildWalk
                                  : (c->skin > 0.0 ? (c->sched.pos == 0 ? PassA::SweepBuild : PassA::Walk) : PassA::Sweep);
        const FluidTmp &tt = c->tmp_par[c->fuse_ea ? q : 0];  // (fuse_ea: the records / list of the current state parity)
        // make every temporary the timed kernel reads valid.  Where pass A of the coming step came with the last step's final
        // launch its list and records are there already, and stay: a timing call should not change what follows (the
        // stand-alone pass is a different kernel and may round differently in the last bit).
        if (!(c->fuse_ea && c->sched.pos != 0)) launch_pass_a(c, q, fs, tt, mode);
        launch_pass_b(c, q, fs, tt);
        launch_pass_cd(c, q, fs, tt);
        launch_pass_e(c, q, fs, tt);
        SPHX_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        for (int k = 0; k < reps; ++k) {
            if (pass == Pass::A) launch_pass_a(c, q, fs, tt, mode);
            else if (pass == Pass::B) launch_pass_b(c, q, fs, tt);
            else if (pass == Pass::CD) launch_pass_cd(c, q, fs, tt);
            else if (pass == Pass::E) launch_pass_e(c, q, fs, tt);
            else {  // Pass::EA (writes the other parity's list / records and the other state's drho: all rewritten by the next step)
                const FluidSet o = c->view(1 - q, c->sched.lay);
                launch_fused_ea(c, q, fs, writing_into(tt, o), o, c->tmp_par[1 - q], Tail::None);
            }
        }
        SPHX_HIP(hipStreamEndCapture(c->stream, &g));
        SPHX_HIP(hipGraphInstantiate(&e, g, nullptr, nullptr, 0));
        SPHX_HIP(hipGraphLaunch(e, c->stream));  // warm
        SPHX_HIP(hipEventCreate(&a));
        SPHX_HIP(hipEventCreate(&b));
        SPHX_HIP(hipEventRecord(a, c->stream));
        SPHX_HIP(hipGraphLaunch(e, c->stream));
        SPHX_HIP(hipEventRecord(b, c->stream));
        if (c->tail_clock)  // the timed passes stored plain maxima: back to "empty" for the next real step
            SPHX_HIP(hipMemsetAsync(c->vpart.get(), 0xFF, (size_t)c->n_vpart * sizeof(double), c->stream));
        SPHX_HIP(hipStreamSynchronize(c->stream));
        float ms = 0.f;
        SPHX_HIP(hipEventElapsedTime(&ms, a, b));
        *avg_ms = (double)ms / reps;
        // the timed passes overwrote the per-step outputs (rho, p, force, Vol, B) with values of a step that was never
        // taken: they are not downloadable until the next real step has produced them again
        c->have_step_outputs = false;
    } catch (...) {
        c->profiling = prof;
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
        if (e) (void)hipGraphExecDestroy(e);
        if (g) (void)hipGraphDestroy(g);
        throw;
    }
    c->profiling = prof;
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    (void)hipGraphExecDestroy(e); (void)hipGraphDestroy(g);
    return SPHX_OK;
    SPHX_CATCH
}

#include "sphx_batch.hpp"
