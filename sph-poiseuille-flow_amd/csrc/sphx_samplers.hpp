// sphx_samplers.hpp -- the ten slot samplers ("Slot samplers"), part of the sphx_resident.hip translation
// unit: flow statistics (include/sphx.h section 2a; of a batch: 2c), the step history (2d; 2f), the velocity-field map (2e; 2g),
// the point probes (2h; 2i), the profile series (2j; 2k), the pair statistics (2l; 2m), the gradient statistics (2n; 2o), the
// particle tracers (2p; 2q) and the density statistics (2r; 2s) -- all nine also of a slab of a ring (3a, at the end of this
// file) -- and the mode amplitudes (2t; 2u).  Their state, shapes and names are in sphx_sampler_state.hpp, their kernels in
// sphx_flow_stats.hpp, sphx_history.hpp, sphx_field_map.hpp, sphx_probes.hpp, sphx_profile_series.hpp, sphx_pair_dist.hpp,
// sphx_grad_stats.hpp, sphx_tracers.hpp, sphx_dens_stats.hpp and sphx_modes.hpp, a batch's entry points in sphx_batch.hpp.
// What the ten share comes first and is stated once: the owner of a sampler (a context, a batch or a slab: admission, settle,
// what a change of setting costs), the lifecycle over it (enable, disable, reset, sample), the view a slot leaves, the head
// read-out, the record-ring read of the five samplers that keep records, and the bins-and-bands check of the five that bin.
// Then each sampler's launch, and per sampler what is its own: check, alloc, read and the entry points.
#pragma once

namespace {

// ---- shared ----

std::string sampler_id(const SamplerNames &n, const char *leaf) { return std::string("SPHX:") + n.stem + ":" + leaf; }

// How an entry point reaches a sampler: the owner of the call.  ctx_owner(c), batch_owner(b) (sphx_batch.hpp) and slab_owner(c)
// make one and raise the owner's own refusals while they do (SPHX:Ctx:null; SPHX:Batch:null; SPHX:Slab:ctx, SPHX:Slab:protocol).
struct Owner {
    sphx_ctx *c;                     // whose sampler members are used (a batch: member 0, which serves every member)
    Schedule &sched;                 // whose replayed graphs carry the samplers' launches
    hipStream_t st;
    int M;                           // channels sampled
    const char *where;               // "context" / "batch" / "slab": the last word of SPHX:<stem>:disabled
    bool has_walls;                  // the channel (a slab: this slab) holds wall particles
    std::function<void()> settle;    // what is enqueued, and the steps still owed, have run: the state a download returns
    bool context;                    // a context's entry points refuse a slab context (SPHX:<stem>:slab), and a change of
                                     // setting settles first, whatever comes of it, as a read or a reset does: the steps a
                                     // batch of sphx_ctx_enqueue_steps still owes were asked for under the old setting
    std::function<void()> changing;  // a slab: in front of on / off (slab_samplers_changed); else empty
};

Owner ctx_owner(sphx_ctx *c)
{
    require(c != nullptr, "SPHX:Ctx:null", "ctx must not be NULL");
    return Owner{c, c->sched, c->stream, 1, "context", c->nw > 0, [c] { settle_owed(c); }, true, {}};
}

// sampler `which` of owner o; need_on: the call needs it enabled (SPHX:<stem>:disabled)
template <typename S>
S &sampler_of(const Owner &o, S sphx_ctx::*which, bool need_on)
{
    S &x = o.c->*which;
    if (o.context && o.c->is_slab) throw Error(SPHX_ERR_ARG, sampler_id(S::names, "slab"), S::names.no_slab);
    if (need_on && !x.on) throw Error(SPHX_ERR_STATE, sampler_id(S::names, "disabled"), std::string(S::names.off) + o.where);
    return x;
}

// ... for a change of its setting (enable, disable)
template <typename S>
S &sampler_to_change(const Owner &o, S sphx_ctx::*which)
{
    S &x = sampler_of(o, which, false);
    if (o.context) o.settle();
    return x;
}

// ... enabled, and everything enqueued has landed: for a reset, a sample or a read without argument checks of its own
template <typename S>
S &sampler_settled(const Owner &o, S sphx_ctx::*which)
{
    S &x = sampler_of(o, which, true);
    o.settle();
    return x;
}

// The replayed graphs of schedule s carry a sampler's launch (and its arguments) or not: a change of the setting waits for
// what is enqueued and drops them, so the next enqueue captures them again.
template <typename S>
void sampler_off(S &x, Schedule &s, hipStream_t st)
{
    SPHX_HIP(hipStreamSynchronize(st));
    s.drop_graphs();
    x.on = false;
    x.release();
}

template <typename S>
void sampler_zero(S &x, hipStream_t st)
{
    x.zero(st);
    SPHX_HIP(hipStreamSynchronize(st));
}

// The enable tail: on, with the CHECKED shape and what alloc() sets up from it, zeroed.  The caller has made every check of the
// configuration: a refused enable leaves a running sampler -- and a slab's prepared step graph -- untouched.  Out of device
// memory the sampler stays off with nothing allocated; flow statistics hand the allocator's error on as it is, the others
// report theirs as a configuration error (SamplerNames::no_memory).
template <typename S, typename Shape>
void sampler_on(const Owner &o, S sphx_ctx::*which, const Shape &checked)
{
    S &x = o.c->*which;
    if (o.changing) o.changing();
    sampler_off(x, o.sched, o.st);
    try {
        x.alloc(checked, o.M, o.st);
        sampler_zero(x, o.st);
    } catch (const Error &e) {
        x.release();
        (void)hipGetLastError();
        if (!S::names.no_memory) throw;
        throw Error(SPHX_ERR_ARG, sampler_id(S::names, "config"), std::string(S::names.no_memory) + e.what());
    }
    x.on = true;
}

// Enable with the configuration check(args...) accepts: every check first, so a refusal changes nothing.  (A batch: bins,
// bands, shapes, points, ids and the walls come from the shared geometry; out of device memory it goes on without the sampler.)
template <typename S, typename... Args>
void sampler_enable(const Owner &o, S sphx_ctx::*which, Args &&...args)
{
    sampler_to_change(o, which);
    S checked;
    checked.check(args...);
    sampler_on(o, which, checked);
}

// off, where it is on (a slab whose sampler is off: nothing is touched)
template <typename S>
void sampler_disable(const Owner &o, S sphx_ctx::*which)
{
    S &x = sampler_to_change(o, which);
    if (!x.on) return;
    if (o.changing) o.changing();
    sampler_off(x, o.sched, o.st);
}

// (the samples of everything enqueued land before the sums are cleared)
template <typename S>
void sampler_reset(const Owner &o, S sphx_ctx::*which)
{
    sampler_zero(sampler_settled(o, which), o.st);
}

// The state step slot q, which ran on layout l, leaves: S[1-q] on every schedule (a re-binning step reorders into S[1-q]
// too, a dynamic context copies back into it), in the other layout when the slot re-binned (a dynamic context re-bins in
// place).  A sampler's launch comes after the slot's clock update, whichever kernel carries it.
FluidSet slot_end_view(sphx_ctx *c, int q, int l, bool rebuild)
{
    return c->dyn ? c->view(1 - q, 0) : c->view(1 - q, rebuild ? 1 - l : l);
}

// A sample of the state now: settled -- the state a download would return; of a batch: every member at the batch's phase --
// then launch(c, q, state, every) with every = 0 on the current view of the owner's schedule
template <typename S, typename Launch>
void sampler_sample(const Owner &o, S sphx_ctx::*which, Launch &&launch)
{
    sampler_settled(o, which);
    launch(o.c, 0, o.c->view(o.sched.cur, o.sched.lay), 0);
    SPHX_HIP(hipGetLastError());
}

// a head's sample count and times, where asked for; no sample yet: the times are NaN
template <typename Head>
void read_head(const Head &h, int64_t *n_samples, double *t_first, double *t_last)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (n_samples) *n_samples = (int64_t)h.n_samples;
    if (t_first) *t_first = h.n_samples ? h.t_first : nan;
    if (t_last) *t_last = h.n_samples ? h.t_last : nan;
}

// SPHX:<stem>:range: member m's sticky flag is up
[[noreturn]] void throw_range(const SamplerNames &n, int M, int m)
{
    throw Error(SPHX_ERR_STATE, sampler_id(n, "range"), (M > 1 ? "member " + std::to_string(m) + ": " : std::string()) +
                                                            "a sampled velocity exceeded twice the clock's max |v| (non-finite state?)");
}

// the sticky range flag of a head that has one
template <typename Head> auto head_range(const Head &h, int) -> decltype(h.range != 0) { return h.range != 0; }
template <typename Head> bool head_range(const Head &, long) { return false; }

// One block of a record ring: member m's rows of `width` doubles at dev + m * cfg.capacity * width, wanted -- where out is
// given -- at out + m * capacity * width of a [members][capacity][width] array
struct RingBlock {
    double *out = nullptr;
    const double *dev = nullptr;
    size_t width = 0;
};

enum class RingStage { Rows, Counts, Drain };  // where ring_read calls its hook

// The read of record ring x (History, Probes, Tracers, ProfileSeries, Modes) of M = x.members members: every member's counts
// (n_records[m], n_dropped[m], where given) and its filled rows 0 .. n_records[m] of the blocks a and b, each where its out is
// given; drain empties every ring.  SPHX:<stem>:state when a count is out of range, SPHX:<stem>:range when a member's sticky
// flag is up (the heads that have one), SPHX:<stem>:capacity when an array is asked for -- a's, b's or, `more`, one of the
// hook's -- and capacity is below the largest count `most`: nothing is copied or drained then.  hook(stage, heads, most) is for
// what is a sampler's own: Rows -- behind the capacity check, in front of the row copies; Counts -- with the counts; Drain --
// behind the zeroing of a draining read, in front of its synchronisation.
template <typename S, typename Head, typename Hook>
void ring_read(S &x, const DevBuf<Head> &head, hipStream_t st, int capacity, RingBlock a, RingBlock b, bool more, int *n_records,
               int64_t *n_dropped, bool drain, Hook &&hook)
{
    const int M = x.members;
    std::vector<Head> h(M);
    SPHX_HIP(hipMemcpyAsync(h.data(), head.get(), sizeof(Head) * M, hipMemcpyDeviceToHost, st));
    SPHX_HIP(hipStreamSynchronize(st));
    long long most = 0;
    for (int m = 0; m < M; ++m) {
        const long long n = h[m].n_records;
        if (n < 0 || n > (long long)x.cfg.capacity)
            throw Error(SPHX_ERR_STATE, sampler_id(S::names, "state"), "internal: record count out of range");
        if (head_range(h[m], 0)) throw_range(S::names, M, m);
        most = std::max(most, n);
    }
    const bool rows = a.out || b.out;
    if ((rows || more) && (long long)capacity < most)
        throw Error(SPHX_ERR_ARG, sampler_id(S::names, "capacity"), "capacity is smaller than the number of records");
    hook(RingStage::Rows, h, most);
    if (rows && most > 0) {
        for (int m = 0; m < M; ++m) {  // only the filled rows of each member's block
            const size_t n = (size_t)h[m].n_records;
            if (n == 0) continue;
            for (const RingBlock &k : {a, b})
                if (k.out)
                    SPHX_HIP(hipMemcpyAsync(k.out + (size_t)m * capacity * k.width, k.dev + (size_t)m * x.cfg.capacity * k.width,
                                            n * k.width * sizeof(double), hipMemcpyDeviceToHost, st));
        }
        SPHX_HIP(hipStreamSynchronize(st));
    }
    for (int m = 0; m < M; ++m) {
        if (n_records) n_records[m] = (int)h[m].n_records;
        if (n_dropped) n_dropped[m] = (int64_t)h[m].n_dropped;
    }
    hook(RingStage::Counts, h, most);
    if (drain) {
        x.zero(st);
        hook(RingStage::Drain, h, most);
        SPHX_HIP(hipStreamSynchronize(st));
    }
}

// ... of a sampler with nothing of its own
template <typename S, typename Head>
void ring_read(S &x, const DevBuf<Head> &head, hipStream_t st, int capacity, RingBlock a, RingBlock b, int *n_records, int64_t *n_dropped,
               bool drain)
{
    ring_read(x, head, st, capacity, a, b, false, n_records, n_dropped, drain, [](RingStage, const std::vector<Head> &, long long) {});
}

// The bins and bands in force of a sampler that bins over y and over x-bands, and the unused bands of cfg -- the shape's copy --
// zeroed: n_bands 0 .. 2, centres and half-widths finite; n_bins as given (its range is the caller's check) or, 0, the
// reference's profile bins.  SPHX:<stem>:config (id) errors; the LDS limit that follows is the sampler's own.
template <typename Cfg>
void bins_and_bands(const char *id, const sphx_params &prm, Cfg &cfg, int &n_bins, int &n_bands)
{
    require(cfg.n_bands >= 0 && cfg.n_bands <= 2, id, "n_bands must be 0, 1 or 2");
    for (int b = 0; b < cfg.n_bands; ++b)
        require(std::isfinite(cfg.band_x[b]) && std::isfinite(cfg.band_hw[b]) && cfg.band_hw[b] >= 0.0, id,
                "band centres must be finite and half-widths finite and >= 0");
    for (int b = cfg.n_bands; b < 2; ++b) { cfg.band_x[b] = 0.0; cfg.band_hw[b] = 0.0; }
    n_bins = cfg.n_bins > 0 ? cfg.n_bins : std::max(20, (int)std::floor(prm.DH / prm.dp + 0.5));
    n_bands = cfg.n_bands + 1;
}

// the bands of cfg into the kernel arguments a
template <typename Args, typename Cfg>
void fill_bands(Args &a, const Cfg &cfg)
{
    for (int b = 0; b < 2; ++b) { a.band_x[b] = cfg.band_x[b]; a.band_hw[b] = cfg.band_hw[b]; }
}

// ---- launches: every >= 1 = the in-loop sample closing step slot q, 0 = a sample of the state now ----

// the arguments of a flow-statistics launch on state s into c->fstats
FlowStatsArgs flow_stats_args(sphx_ctx *c, const FluidSet &s, int every)
{
    const FlowStats &f = c->fstats;
    FlowStatsArgs a{};
    a.pos = s.pos; a.vel = s.vel;
    a.isum = f.isum.get(); a.dsum = f.dsum.get(); a.head = f.head.get();
    a.DH = c->prm.DH; a.bin_w = c->prm.DH / f.n_bins; a.DL = c->prm.DL;
    a.t_from = f.cfg.t_from;
    fill_bands(a, f.cfg);
    a.n_bins = f.n_bins; a.n_bands = f.n_bands;
    a.every = every;
    return a;
}

// workgroups of the sample of a channel that holds n particles
unsigned flow_stats_blocks(size_t n)
{
    return std::clamp<unsigned>(div_up(n, (size_t)kStatsBlock * kStatsPerThread), 1u, (unsigned)kStatsMaxBlocks);
}

// k_flow_stats on state s -- of a batch: member 0's -- into c->fstats
void launch_flow_stats(sphx_ctx *c, int q, const FluidSet &s, int every)
{
    launch_forms(c, "k_flow_stats", Forms{k_flow_stats, k_flow_stats_b}, flow_stats_blocks((size_t)c->nf), kStatsBlock, c->fstats.shmem(), q,
                 flow_stats_args(c, s, every));
}

// the arguments of a history launch into c->hist; src: where Vol / B of a slot are (HistorySrc)
HistoryArgs history_args(sphx_ctx *c, int src)
{
    const History &h = c->hist;
    HistoryArgs a{};
    a.records = h.records.get(); a.part = h.part.get(); a.head = h.head.get();
    a.t_from = h.cfg.t_from; a.capacity = h.cfg.capacity; a.every = h.cfg.every;
    a.src = src;
    return a;
}

// workgroups of the record of a channel that holds n particles
unsigned history_blocks(size_t n)
{
    return std::clamp<unsigned>(div_up(n, (size_t)kHistoryBlock * kHistoryPerThread), 1u, (unsigned)kHistoryMaxBlocks);
}

// k_step_history behind step slot q, which left state s -- of a batch: member 0's -- into c->hist: Vol / B of the finished step
// are where sphx_ctx_monitor looks them up after it: the record buffers of the step's parity (fuse_ea), in the order of the
// layout the step ran in, so read through src_of when the slot re-binned.  The static schedule knows that when the launch is
// made (or captured); a dynamic context re-bins in place and says so in Clock::fresh.  A batch runs the static schedule, and
// its shared slot's `rebuild` holds for every member that runs in the slot.
void launch_history(sphx_ctx *c, int q, const FluidSet &s, bool rebuild)
{
    const HistoryArgs a = history_args(c, c->dyn ? kHistoryByClock : (rebuild ? kHistorySrcOf : kHistoryInPlace));
    launch_forms(c, "k_step_history", Forms{k_step_history, k_step_history_b}, history_blocks((size_t)c->nf), kHistoryBlock, 0, q, c->grid,
                 per_member(c->phys), s, c->tmp_par[c->fuse_ea ? q : 0], c->walls, a);
}

// the arguments of a field-map launch into c->fmap over nx node columns (a slab: those of its block)
FieldMapArgs field_map_args(sphx_ctx *c, int nx, int every)
{
    const FieldMap &f = c->fmap;
    FieldMapArgs a{};
    a.planes = f.planes.get(); a.head = f.head.get();
    a.step_x = c->prm.DL / (nx - 1); a.step_y = c->prm.DH / (f.ny - 1);
    a.dp2 = c->prm.dp * c->prm.dp;
    a.t_from = f.cfg.t_from;
    a.nx = nx; a.ny = f.ny;
    a.tiles_y = (int)div_up((size_t)f.ny, (size_t)kFieldTile);
    a.n_tiles = (int)div_up((size_t)nx, (size_t)kFieldTile) * a.tiles_y;
    a.every = every;
    a.with_walls = f.cfg.with_walls && c->nw > 0 ? 1 : 0;
    return a;
}

// workgroups of one channel's sample (at least one: it writes the head)
unsigned field_map_blocks(const FieldMapArgs &a)
{
    return std::max<unsigned>(div_up((size_t)a.n_tiles, (size_t)(kFieldBlock / 64)), 1u);
}

// k_field_map on state s (pos, vel and the cell ranges of the layout it is stored in) -- of a batch: member 0's -- into c->fmap
void launch_field_map(sphx_ctx *c, int q, const FluidSet &s, int every)
{
    const FieldMapArgs a = field_map_args(c, c->fmap.nx, every);
    launch_forms(c, "k_field_map", Forms{k_field_map, k_field_map_b}, field_map_blocks(a), kFieldBlock, 0, q, c->grid,
                 per_member(c->phys), s, c->walls, a);
}

// the arguments of a probes launch into c->probes
ProbeArgs probe_args(sphx_ctx *c, int every)
{
    const Probes &p = c->probes;
    ProbeArgs a{};
    a.points = p.points.get(); a.times = p.times.get(); a.values = p.values.get(); a.head = p.head.get();
    a.dp2 = c->prm.dp * c->prm.dp;
    a.t_from = p.cfg.t_from;
    a.n_points = p.held(); a.capacity = p.cfg.capacity;  // (a slab: the probes it owns)
    a.every = every;
    a.with_walls = p.cfg.with_walls && c->nw > 0 ? 1 : 0;
    return a;
}

// workgroups of one channel's record: a wave per probe
unsigned probe_blocks(const ProbeArgs &a)
{
    return (unsigned)div_up((size_t)a.n_points, (size_t)kProbeWaves);
}

// k_point_probes on state s (pos, vel, mass and the cell ranges of the layout it is stored in) -- of a batch: member 0's -- into
// c->probes
void launch_probes(sphx_ctx *c, int q, const FluidSet &s, int every)
{
    const ProbeArgs a = probe_args(c, every);
    launch_forms(c, "k_point_probes", Forms{k_point_probes, k_point_probes_b}, probe_blocks(a), kProbeBlock, 0, q, c->grid,
                 per_member(c->phys), s, c->walls, a);
}

// the arguments of a profile-series launch on state s into c->pseries
ProfileSeriesArgs profile_series_args(sphx_ctx *c, const FluidSet &s, int every)
{
    const ProfileSeries &p = c->pseries;
    ProfileSeriesArgs a{};
    a.bin.pos = s.pos; a.bin.vel = s.vel;
    a.bin.isum = p.isum.get();
    a.bin.DH = c->prm.DH; a.bin.bin_w = c->prm.DH / p.n_bins; a.bin.DL = c->prm.DL;
    a.bin.t_from = p.cfg.t_from;
    fill_bands(a.bin, p.cfg);
    a.bin.n_bins = p.n_bins; a.bin.n_bands = p.n_bands;
    a.bin.every = every;
    a.times = p.times.get(); a.records = p.records.get(); a.head = p.head.get();
    a.capacity = p.cfg.capacity;
    return a;
}

// k_profile_series on state s -- of a batch: member 0's -- into c->pseries: the workgroups of a flow-statistics sample
void launch_profile_series(sphx_ctx *c, int q, const FluidSet &s, int every)
{
    launch_forms(c, "k_profile_series", Forms{k_profile_series, k_profile_series_b}, flow_stats_blocks((size_t)c->nf), kStatsBlock,
                 c->pseries.shmem(), q, profile_series_args(c, s, every));
}

// the arguments of a pair-statistics launch into c->pairs
PairDistArgs pair_dist_args(sphx_ctx *c, int every)
{
    const PairDist &p = c->pairs;
    PairDistArgs a{};
    a.sums = p.sums.get(); a.head = p.head.get();
    a.bin_w = p.r_max / p.n_bins; a.rmax2 = p.r_max * p.r_max;
    a.y_lo = p.cfg.y_margin; a.y_hi = c->prm.DH - p.cfg.y_margin;
    a.DL = c->prm.DL; a.t_from = p.cfg.t_from;
    fill_bands(a, p.cfg);
    a.n_bins = p.n_bins; a.n_bands = p.n_bands; a.kinds = p.kinds;
    a.block = (int)p.block();
    a.every = every;
    return a;
}

// workgroups of the sample of a channel that holds n particles: kPairCentres centres a trip
unsigned pair_dist_blocks(size_t n)
{
    return std::clamp<unsigned>(div_up(n, (size_t)kPairCentres), 1u, (unsigned)kPairMaxBlocks);
}

// k_pair_dist on state s (pos and the cell ranges and binned cells of the layout it is stored in) -- of a batch: member 0's --
// into c->pairs
void launch_pair_dist(sphx_ctx *c, int q, const FluidSet &s, int every)
{
    launch_forms(c, "k_pair_dist", Forms{k_pair_dist, k_pair_dist_b}, pair_dist_blocks((size_t)c->nf), kPairBlock, c->pairs.shmem(), q,
                 c->grid, s, c->walls, pair_dist_args(c, every));
}

// the arguments of a gradient-statistics launch into c->grads
GradStatsArgs grad_stats_args(sphx_ctx *c, int every)
{
    const GradStats &f = c->grads;
    GradStatsArgs a{};
    a.isum = f.isum.get(); a.dsum = f.dsum.get(); a.head = f.head.get();
    a.DH = c->prm.DH; a.bin_w = c->prm.DH / f.n_bins; a.DL = c->prm.DL;
    a.t_from = f.cfg.t_from; a.det_min = f.cfg.det_min;
    fill_bands(a, f.cfg);
    a.n_bins = f.n_bins; a.n_bands = f.n_bands;
    a.block = (int)f.block();
    a.with_walls = f.walls ? 1 : 0;
    a.every = every;
    return a;
}

// workgroups of the sample of a channel that holds n particles: kGradTrips trips of kGradCentres particles each
unsigned grad_stats_blocks(size_t n)
{
    return std::clamp<unsigned>(div_up(n, (size_t)kGradCentres * kGradTrips), 1u, (unsigned)kGradMaxBlocks);
}

// k_grad_stats on state s (pos, vel, mass and the cell ranges and binned cells of the layout it is stored in) -- of a batch:
// member 0's -- into c->grads
void launch_grad_stats(sphx_ctx *c, int q, const FluidSet &s, int every)
{
    launch_forms(c, "k_grad_stats", Forms{k_grad_stats, k_grad_stats_b}, grad_stats_blocks((size_t)c->nf), kGradBlock, c->grads.shmem(), q,
                 c->grid, per_member(c->phys), s, c->walls, grad_stats_args(c, every));
}

// the arguments of a tracers launch into c->tracers
TracerArgs tracer_args(sphx_ctx *c, int every)
{
    const Tracers &t = c->tracers;
    TracerArgs a{};
    a.index_of = t.index_of.get(); a.times = t.times.get(); a.values = t.values.get(); a.head = t.head.get();
    a.t_from = t.cfg.t_from;
    a.n_tracers = t.cfg.n_tracers; a.n_fluid = t.n_fluid; a.n_slots = c->nf; a.capacity = t.cfg.capacity;
    a.every = every;
    return a;
}

// workgroups of the scan of a channel that holds n particles: a grid-stride loop under a fixed cap
unsigned tracer_blocks(size_t n)
{
    return std::clamp<unsigned>(div_up(n, (size_t)kTracerBlock), 1u, (unsigned)kTracerMaxBlocks);
}

// k_tracers on state s (pos, vel and the ids of the layout it is stored in) -- of a batch: member 0's -- into c->tracers
void launch_tracers(sphx_ctx *c, int q, const FluidSet &s, int every)
{
    launch_forms(c, "k_tracers", Forms{k_tracers, k_tracers_b}, tracer_blocks((size_t)c->nf), kTracerBlock, 0, q, s, tracer_args(c, every));
}

// the arguments of a density-statistics launch into c->dens
DensStatsArgs dens_stats_args(sphx_ctx *c, int every)
{
    const DensStats &f = c->dens;
    DensStatsArgs a{};
    a.isum = f.isum.get(); a.dsum = f.dsum.get(); a.keys = f.keys.get(); a.head = f.head.get();
    a.DH = c->prm.DH; a.bin_w = c->prm.DH / f.n_bins; a.DL = c->prm.DL;
    a.t_from = f.cfg.t_from;
    a.delta_bound = f.cfg.delta_bound; a.hist_range = f.cfg.hist_range;
    a.hist_scale = (double)f.cfg.n_hist / (2.0 * f.cfg.hist_range);
    fill_bands(a, f.cfg);
    a.n_bins = f.n_bins; a.n_bands = f.n_bands; a.n_hist = f.cfg.n_hist;
    a.block = (int)f.block(); a.kblock = (int)f.kblock();
    a.e = f.e;
    a.every = every;
    return a;
}

// workgroups of the sample of a channel that holds n particles: kDensTrips trips of kDensCentres particles each
unsigned dens_stats_blocks(size_t n)
{
    return std::clamp<unsigned>(div_up(n, (size_t)kDensCentres * kDensTrips), 1u, (unsigned)kDensMaxBlocks);
}

// k_dens_stats on state s (pos, mass and the cell ranges and binned cells of the layout it is stored in) -- of a batch: member
// 0's -- into c->dens
void launch_dens_stats(sphx_ctx *c, int q, const FluidSet &s, int every)
{
    launch_forms(c, "k_dens_stats", Forms{k_dens_stats, k_dens_stats_b}, dens_stats_blocks((size_t)c->nf), kDensBlock, c->dens.shmem(), q,
                 c->grid, per_member(c->phys), s, c->walls, dens_stats_args(c, every));
}

// the arguments of a mode-amplitudes launch on state s into c->modes
ModesArgs modes_args(sphx_ctx *c, const FluidSet &s, int every)
{
    const Modes &p = c->modes;
    ModesArgs a{};
    a.pos = s.pos; a.vel = s.vel;
    a.isum = p.isum.get(); a.times = p.times.get(); a.records = p.records.get(); a.head = p.head.get();
    a.DL = c->prm.DL; a.DH = c->prm.DH;
    a.t_from = p.cfg.t_from;
    a.mx = p.cfg.mx; a.ny = p.cfg.ny;
    a.n_groups = p.groups();
    a.every = every;
    a.capacity = p.cfg.capacity;
    return a;
}

// workgroups of the sample of a channel that holds n particles: chunks x groups, every group over every chunk
unsigned modes_blocks(size_t n, int groups)
{
    const unsigned most = std::max(1u, (unsigned)kModesMaxBlocks / (unsigned)groups);
    return std::clamp<unsigned>(div_up(n, (size_t)kModesBlock * kModesPerThread), 1u, most) * (unsigned)groups;
}

// k_modes on state s -- of a batch: member 0's -- into c->modes
void launch_modes(sphx_ctx *c, int q, const FluidSet &s, int every)
{
    launch_forms(c, "k_modes", Forms{k_modes, k_modes_b}, modes_blocks((size_t)c->nf, c->modes.groups()), kModesBlock, c->modes.shmem(), q,
                 modes_args(c, s, every));
}

}  // namespace

void sphx::launch_slot_samplers(sphx_ctx *c, int q, int l, bool rebuild)
{
    const FluidSet s = slot_end_view(c, q, l, rebuild);
    if (c->fstats.on) launch_flow_stats(c, q, s, c->fstats.cfg.every);
    if (c->hist.on) launch_history(c, q, s, rebuild);
    if (c->fmap.on) launch_field_map(c, q, s, c->fmap.cfg.every);
    if (c->probes.on) launch_probes(c, q, s, c->probes.cfg.every);
    if (c->pseries.on) launch_profile_series(c, q, s, c->pseries.cfg.every);
    if (c->pairs.on) launch_pair_dist(c, q, s, c->pairs.cfg.every);
    if (c->grads.on) launch_grad_stats(c, q, s, c->grads.cfg.every);
    if (c->tracers.on) launch_tracers(c, q, s, c->tracers.cfg.every);
    if (c->dens.on) launch_dens_stats(c, q, s, c->dens.cfg.every);
    if (c->modes.on) launch_modes(c, q, s, c->modes.cfg.every);
}

// ---- flow statistics ----

// the checked configuration cfg of channels with parameters prm (cfg, n_bins, n_bands); SPHX:Stats:config errors
void FlowStatsShape::check(const sphx_params &prm, const sphx_flow_stats_config *cfg)
{
    require(cfg != nullptr, "SPHX:Stats:config", "config must not be NULL");
    require(cfg->n_bins >= 0, "SPHX:Stats:config", "n_bins must be >= 0 (0 = the reference's profile bins)");
    require(cfg->every >= 1, "SPHX:Stats:config", "every must be >= 1");
    require(!std::isnan(cfg->t_from), "SPHX:Stats:config", "t_from must not be NaN");
    this->cfg = *cfg;
    bins_and_bands("SPHX:Stats:config", prm, this->cfg, n_bins, n_bands);
    require((int64_t)n_bins * n_bands <= kStatsMaxBins, "SPHX:Stats:config",
            "n_bins * (n_bands + 1) must not exceed 1536 (the per-workgroup LDS counters)");
}

// the checked shape, and sums and heads for M members
void FlowStats::alloc(const FlowStatsShape &checked, int M, hipStream_t)
{
    static_cast<FlowStatsShape &>(*this) = checked;
    members = M;
    isum.alloc(block() * M);
    dsum.alloc(block() * M);
    head.alloc(M);
}

// Band `band` of every member's sums (sums: into out[field][m * stride + bin], where out[field] is given) and the heads
// (n_samples[m], t_first[m], t_last[m], where given).  SPHX:Stats:range when a member's sticky flag is up.
void FlowStats::read(hipStream_t st, int band, int stride, bool sums, double *const out[kStatsFields], int64_t *n_samples,
                     double *t_first, double *t_last) const
{
    const int M = members;
    std::vector<double> host(sums ? (size_t)M * row() : 0);
    std::vector<FlowStatsHead> h(M);
    if (sums)  // one copy: a row of every member's block
        SPHX_HIP(hipMemcpy2DAsync(host.data(), row() * sizeof(double), dsum.get() + (size_t)band * row(), block() * sizeof(double),
                                  row() * sizeof(double), M, hipMemcpyDeviceToHost, st));
    SPHX_HIP(hipMemcpyAsync(h.data(), head.get(), sizeof(FlowStatsHead) * M, hipMemcpyDeviceToHost, st));
    SPHX_HIP(hipStreamSynchronize(st));
    for (int m = 0; m < M; ++m)
        if (h[m].range) throw_range(names, M, m);
    for (int j = 0; j < kStatsFields; ++j)
        if (out[j])
            for (int m = 0; m < M; ++m)
                for (int k = 0; k < n_bins; ++k) out[j][(size_t)m * stride + k] = host[(size_t)m * row() + (size_t)k * kStatsFields + j];
    for (int m = 0; m < M; ++m)
        read_head(h[m], n_samples ? n_samples + m : nullptr, t_first ? t_first + m : nullptr, t_last ? t_last + m : nullptr);
}

namespace {

// the argument checks of a read, then what is enqueued lands, and the read
void stats_read(const Owner &o, int band, int capacity, int *n_bins, double *count, double *sum_ux, double *sum_ux2, double *sum_uy,
                double *sum_uy2, int64_t *n_samples, double *t_first, double *t_last)
{
    const FlowStats &f = sampler_of(o, &sphx_ctx::fstats, true);
    require(band >= 0 && band < f.n_bands, "SPHX:Stats:band", "band must be 0 (whole channel) .. n_bands");
    double *const out[kStatsFields] = {count, sum_ux, sum_ux2, sum_uy, sum_uy2};
    bool any = false;
    for (double *p : out) any = any || p != nullptr;
    require(!any || capacity >= f.n_bins, "SPHX:Stats:capacity", "capacity is smaller than the number of bins");
    o.settle();
    f.read(o.st, band, capacity, any, out, n_samples, t_first, t_last);
    if (n_bins) *n_bins = f.n_bins;
}

}  // namespace

SPHX_EXPORT int sphx_ctx_flow_stats_enable(sphx_ctx *c, const sphx_flow_stats_config *cfg)
{
    SPHX_TRY
    const Owner o = ctx_owner(c);
    sampler_enable(o, &sphx_ctx::fstats, o.c->prm, cfg);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_flow_stats_disable(sphx_ctx *c)
{
    SPHX_TRY
    sampler_disable(ctx_owner(c), &sphx_ctx::fstats);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_flow_stats_reset(sphx_ctx *c)
{
    SPHX_TRY
    sampler_reset(ctx_owner(c), &sphx_ctx::fstats);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_flow_stats_sample(sphx_ctx *c)
{
    SPHX_TRY
    sampler_sample(ctx_owner(c), &sphx_ctx::fstats, launch_flow_stats);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_flow_stats_read(sphx_ctx *c, int band, int capacity, int *n_bins, double *count, double *sum_ux,
                                         double *sum_ux2, double *sum_uy, double *sum_uy2, int64_t *n_samples,
                                         double *t_first, double *t_last)
{
    SPHX_TRY
    stats_read(ctx_owner(c), band, capacity, n_bins, count, sum_ux, sum_ux2, sum_uy, sum_uy2, n_samples, t_first, t_last);
    return SPHX_OK;
    SPHX_CATCH
}

// ---- step history ----

// every check of a configuration for M channels; SPHX:History:config errors
void HistoryShape::check(const sphx_history_config *cfg, int M)
{
    require(cfg != nullptr, "SPHX:History:config", "config must not be NULL");
    require(cfg->every >= 1, "SPHX:History:config", "every must be >= 1");
    require(cfg->capacity >= 1 && cfg->capacity <= kHistoryMaxCapacity, "SPHX:History:config", "capacity must be 1 .. 1 << 22 records");
    require((int64_t)M * cfg->capacity <= kHistoryMaxTotal, "SPHX:History:config",
            "n_members * capacity must not exceed 1 << 24 records");
    require(std::isfinite(cfg->t_from), "SPHX:History:config", "t_from must be finite");
    this->cfg = *cfg;
}

// the checked shape, and records, partials and heads for M members
void History::alloc(const HistoryShape &checked, int M, hipStream_t)
{
    static_cast<HistoryShape &>(*this) = checked;
    members = M;
    records.alloc((size_t)M * cfg.capacity * kHistoryFields);
    part.alloc((size_t)M * kHistoryMaxBlocks * kHistorySums);
    head.alloc(M);
}

// Every member's counts and, with `out`, its filled rows into out[m][0 .. n_records[m])[kHistoryFields] (ring_read)
void History::read(hipStream_t st, int capacity, double *out, int *n_records, int64_t *n_dropped, bool drain)
{
    ring_read(*this, head, st, capacity, {out, records.get(), (size_t)kHistoryFields}, {}, n_records, n_dropped, drain);
}

SPHX_EXPORT int sphx_ctx_history_enable(sphx_ctx *c, const sphx_history_config *cfg)
{
    SPHX_TRY
    const Owner o = ctx_owner(c);
    sampler_enable(o, &sphx_ctx::hist, cfg, o.M);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_history_disable(sphx_ctx *c)
{
    SPHX_TRY
    sampler_disable(ctx_owner(c), &sphx_ctx::hist);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_history_read(sphx_ctx *c, int capacity, double *records, int *n_records, int64_t *n_dropped, int drain)
{
    SPHX_TRY
    const Owner o = ctx_owner(c);
    sampler_settled(o, &sphx_ctx::hist).read(o.st, capacity, records, n_records, n_dropped, drain != 0);
    return SPHX_OK;
    SPHX_CATCH
}

// ---- velocity-field map ----

// every check of a configuration for M channels with parameters prm (cfg and the shape in force); SPHX:Field:config errors
void FieldMapShape::check(const sphx_params &prm, const sphx_field_map_config *cfg, int M)
{
    require(cfg != nullptr, "SPHX:Field:config", "config must not be NULL");
    require(cfg->nx == 0 || cfg->nx >= 2, "SPHX:Field:config", "nx must be 0 (the reference's shape) or >= 2");
    require(cfg->ny == 0 || cfg->ny >= 2, "SPHX:Field:config", "ny must be 0 (the reference's shape) or >= 2");
    require(cfg->every >= 1, "SPHX:Field:config", "every must be >= 1");
    require(!std::isnan(cfg->t_from), "SPHX:Field:config", "t_from must not be NaN");
    require(cfg->with_walls == 0 || cfg->with_walls == 1, "SPHX:Field:config", "with_walls must be 0 or 1");
    // 0: the grid of SPH_Poiseuille_postprocess.m:185-186
    const double gx = cfg->nx > 0 ? (double)cfg->nx : 2.0 * std::floor(prm.DL / prm.dp + 0.5);
    const double gy = cfg->ny > 0 ? (double)cfg->ny : 2.0 * std::floor(prm.DH / prm.dp + 0.5);
    require(gx >= 2.0 && gy >= 2.0, "SPHX:Field:config", "the reference's shape has fewer than 2 nodes along x or y: give nx and ny");
    if (!((double)M * gx * gy <= (double)kFieldMaxNodes))
        throw Error(SPHX_ERR_ARG, "SPHX:Field:config", std::string(M > 1 ? "n_members * " : "") + "nx * ny must not exceed 1 << 25 nodes");
    this->cfg = *cfg;
    nx = (int)gx;
    ny = (int)gy;
}

// the checked shape, and planes and heads for M members
void FieldMap::alloc(const FieldMapShape &checked, int M, hipStream_t)
{
    static_cast<FieldMapShape &>(*this) = checked;
    members = M;
    planes.alloc(std::max<size_t>(block() * M, 1));  // (a slab that owns no node column still has a head)
    head.alloc(M);
}

// Every member's planes (into out[plane][m * stride + node], where out[plane] is given) and heads (n_samples[m], t_first[m],
// t_last[m], where given)
void FieldMap::read(hipStream_t st, int stride, double *const out[kFieldPlanes], int64_t *n_samples, double *t_first,
                    double *t_last) const
{
    const int M = members;
    std::vector<FieldMapHead> h(M);
    for (int j = 0; j < kFieldPlanes; ++j)
        if (out[j] && nodes() > 0)
            for (int m = 0; m < M; ++m)
                SPHX_HIP(hipMemcpyAsync(out[j] + (size_t)m * stride, planes.get() + (size_t)m * block() + (size_t)j * nodes(),
                                        nodes() * sizeof(double), hipMemcpyDeviceToHost, st));
    SPHX_HIP(hipMemcpyAsync(h.data(), head.get(), sizeof(FieldMapHead) * M, hipMemcpyDeviceToHost, st));
    SPHX_HIP(hipStreamSynchronize(st));
    for (int m = 0; m < M; ++m)
        read_head(h[m], n_samples ? n_samples + m : nullptr, t_first ? t_first + m : nullptr, t_last ? t_last + m : nullptr);
}

namespace {

// the argument checks of a read, then what is enqueued lands, and the read
const FieldMap &field_read(const Owner &o, int capacity, int *nx, int *ny, double *count, double *sum_w, double *sum_ux, double *sum_uy,
                           double *sum_ux2, double *sum_uy2, int64_t *n_samples, double *t_first, double *t_last)
{
    const FieldMap &f = sampler_of(o, &sphx_ctx::fmap, true);
    double *const out[kFieldPlanes] = {count, sum_w, sum_ux, sum_uy, sum_ux2, sum_uy2};
    bool any = false;
    for (double *p : out) any = any || p != nullptr;
    require(!any || (size_t)std::max(capacity, 0) >= f.nodes(), "SPHX:Field:capacity", "capacity is smaller than nx * ny");
    o.settle();  // (the samples of everything enqueued)
    f.read(o.st, capacity, out, n_samples, t_first, t_last);
    if (nx) *nx = f.nx;
    if (ny) *ny = f.ny;
    return f;
}

}  // namespace

SPHX_EXPORT int sphx_ctx_field_map_enable(sphx_ctx *c, const sphx_field_map_config *cfg)
{
    SPHX_TRY
    const Owner o = ctx_owner(c);
    sampler_enable(o, &sphx_ctx::fmap, o.c->prm, cfg, o.M);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_field_map_disable(sphx_ctx *c)
{
    SPHX_TRY
    sampler_disable(ctx_owner(c), &sphx_ctx::fmap);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_field_map_reset(sphx_ctx *c)
{
    SPHX_TRY
    sampler_reset(ctx_owner(c), &sphx_ctx::fmap);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_field_map_sample(sphx_ctx *c)
{
    SPHX_TRY
    sampler_sample(ctx_owner(c), &sphx_ctx::fmap, launch_field_map);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_field_map_read(sphx_ctx *c, int capacity, int *nx, int *ny, double *count, double *sum_w, double *sum_ux,
                                        double *sum_uy, double *sum_ux2, double *sum_uy2, int64_t *n_samples, double *t_first,
                                        double *t_last)
{
    SPHX_TRY
    field_read(ctx_owner(c), capacity, nx, ny, count, sum_w, sum_ux, sum_uy, sum_ux2, sum_uy2, n_samples, t_first, t_last);
    return SPHX_OK;
    SPHX_CATCH
}

// ---- point probes ----

namespace {

// x folded into [0, DL): x - floor(x / DL) * DL, each operation rounded by itself (numpy's value), and 0 where the rounding
// of a tiny negative x lands on DL
double probe_fold(double x, double DL)
{
#pragma clang fp contract(off)
    const double k = std::floor(x / DL);
    const double f = x - k * DL;
    return f >= 0.0 && f < DL ? f : 0.0;
}

}  // namespace

// every check of a configuration for M channels with parameters prm (cfg without the pointer, and the folded points);
// SPHX:Probe:config errors
void ProbesShape::check(const sphx_params &prm, const sphx_probes_config *cfg, int M)
{
    require(cfg != nullptr, "SPHX:Probe:config", "config must not be NULL");
    require(cfg->points != nullptr, "SPHX:Probe:config", "points must not be NULL");
    require(cfg->n_points >= 1 && cfg->n_points <= kProbeMaxPoints, "SPHX:Probe:config", "n_points must be 1 .. 4096");
    require(cfg->every >= 1, "SPHX:Probe:config", "every must be >= 1");
    require(cfg->capacity >= 1, "SPHX:Probe:config", "capacity must be >= 1");
    if (!((double)M * (double)cfg->capacity * (double)cfg->n_points * kProbeFields <= (double)kProbeMaxTotal))
        throw Error(SPHX_ERR_ARG, "SPHX:Probe:config",
                    std::string(M > 1 ? "n_members * " : "") + "capacity * n_points * 4 must not exceed 1 << 27 doubles");
    require(std::isfinite(cfg->t_from), "SPHX:Probe:config", "t_from must be finite");
    require(cfg->with_walls == 0 || cfg->with_walls == 1, "SPHX:Probe:config", "with_walls must be 0 or 1");
    folded.resize((size_t)cfg->n_points * 2);
    for (int p = 0; p < cfg->n_points; ++p) {
        const double x = cfg->points[2 * p], y = cfg->points[2 * p + 1];
        require(std::isfinite(x) && std::isfinite(y), "SPHX:Probe:config", "the coordinates of a point must be finite");
        require(y >= 0.0 && y <= prm.DH, "SPHX:Probe:config", "the y of a point must lie in [0, DH]");
        folded[2 * p] = probe_fold(x, prm.DL);
        folded[2 * p + 1] = y;
    }
    this->cfg = *cfg;
    this->cfg.points = nullptr;
}

// the checked shape, and points, records and heads for M members
void Probes::alloc(const ProbesShape &checked, int M, hipStream_t st)
{
    static_cast<ProbesShape &>(*this) = checked;
    members = M;
    points.alloc(std::max<size_t>((size_t)held(), 1));  // (a slab that owns no probe still has a head and its times)
    times.alloc((size_t)M * cfg.capacity * 2);
    values.alloc(std::max<size_t>((size_t)M * cfg.capacity * row(), 1));
    head.alloc(M);
    if (!part) {
        points.upload(reinterpret_cast<const double2 *>(folded.data()), (size_t)cfg.n_points, st);  // (sampler_on waits for st)
        return;
    }
    std::vector<double> own(index.size() * 2);  // the owned subset, compacted in the ring's order
    for (size_t k = 0; k < index.size(); ++k) {
        own[2 * k] = folded[2 * (size_t)index[k]];
        own[2 * k + 1] = folded[2 * (size_t)index[k] + 1];
    }
    points.upload(reinterpret_cast<const double2 *>(own.data()), index.size(), st);
    SPHX_HIP(hipStreamSynchronize(st));  // (`own` goes out of scope here)
}

// Every member's counts and its filled rows, into times[m][0 .. n_records[m])[2] and values[m][0 .. n_records[m])[row()], each
// where given (ring_read)
void Probes::read(hipStream_t st, int capacity, double *t_out, double *v_out, int *n_records, int64_t *n_dropped, bool drain)
{
    ring_read(*this, head, st, capacity, {t_out, times.get(), 2}, {v_out, values.get(), row()}, n_records, n_dropped, drain);
}

SPHX_EXPORT int sphx_ctx_probes_enable(sphx_ctx *c, const sphx_probes_config *cfg)
{
    SPHX_TRY
    const Owner o = ctx_owner(c);
    sampler_enable(o, &sphx_ctx::probes, o.c->prm, cfg, o.M);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_probes_disable(sphx_ctx *c)
{
    SPHX_TRY
    sampler_disable(ctx_owner(c), &sphx_ctx::probes);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_probes_sample(sphx_ctx *c)
{
    SPHX_TRY
    sampler_sample(ctx_owner(c), &sphx_ctx::probes, launch_probes);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_probes_read(sphx_ctx *c, int capacity, double *times, double *values, int *n_points, int *n_records,
                                     int64_t *n_dropped, int drain)
{
    SPHX_TRY
    const Owner o = ctx_owner(c);
    Probes &p = sampler_settled(o, &sphx_ctx::probes);  // (the records of everything enqueued)
    p.read(o.st, capacity, times, values, n_records, n_dropped, drain != 0);
    if (n_points) *n_points = p.cfg.n_points;
    return SPHX_OK;
    SPHX_CATCH
}

// ---- particle tracers ----

// every check of a configuration for M channels of n_fluid fluid rows among n_total (cfg without the pointer, and the ids);
// SPHX:Tracers:config errors
void TracersShape::check(int n_fluid, int n_total, const sphx_tracers_config *cfg, int M)
{
    const char *id = "SPHX:Tracers:config";
    require(cfg != nullptr, id, "config must not be NULL");
    require(cfg->ids != nullptr, id, "ids must not be NULL");
    require(cfg->n_tracers >= 1 && cfg->n_tracers <= n_fluid, id, "n_tracers must be 1 .. n_fluid");
    require(cfg->every >= 1, id, "every must be >= 1");
    require(cfg->capacity >= 1, id, "capacity must be >= 1");
    if (!((double)M * (double)cfg->capacity * (double)cfg->n_tracers * kTracerFields <= (double)kTracerMaxTotal))
        throw Error(SPHX_ERR_ARG, id, std::string(M > 1 ? "n_members * " : "") + "capacity * n_tracers * 4 must not exceed 1 << 27 doubles");
    require(std::isfinite(cfg->t_from), id, "t_from must be finite");
    std::vector<char> seen((size_t)n_fluid, 0);
    ids.assign(cfg->ids, cfg->ids + cfg->n_tracers);
    for (const int32_t r : ids) {
        require(r < n_fluid || r >= n_total, id, "a tracer must be a fluid row: rows n_fluid .. n_total - 1 are wall particles");
        require(r >= 0 && r < n_fluid, id, "a tracer id must be a row number in 0 .. n_fluid - 1");
        require(!seen[(size_t)r], id, "a row is listed twice");
        seen[(size_t)r] = 1;
    }
    this->cfg = *cfg;
    this->cfg.ids = nullptr;
    this->n_fluid = n_fluid;
}

// the checked shape, the table, and records and heads for M members
void Tracers::alloc(const TracersShape &checked, int M, hipStream_t st)
{
    static_cast<TracersShape &>(*this) = checked;
    members = M;
    index_of.alloc((size_t)n_fluid);
    times.alloc((size_t)M * cfg.capacity * 2);
    values.alloc((size_t)M * cfg.capacity * row());
    if (part) n_owned.alloc((size_t)cfg.capacity);
    head.alloc(M);
    if (part) nan_fill(st, (size_t)cfg.capacity);
    std::vector<int> table((size_t)n_fluid, -1);
    for (int k = 0; k < cfg.n_tracers; ++k) table[(size_t)ids[(size_t)k]] = k;
    index_of.upload(table.data(), table.size(), st);
    SPHX_HIP(hipStreamSynchronize(st));  // (`table` goes out of scope here)
}

// A slab's value rows 0 .. rows - 1 read NaN again (every byte 0xFF), enqueued on st: a column is written only by the slab that
// owns the particle at that step, so what nobody wrote must be recognisable -- and a particle's x is never NaN.
void Tracers::nan_fill(hipStream_t st, size_t rows)
{
    if (rows) SPHX_HIP(hipMemsetAsync(values.get(), 0xFF, rows * row() * sizeof(double), st));
}

// Every member's counts (with n_missing[m], where given) and its filled rows, into times[m][0 .. n_records[m])[2] and
// values[m][0 .. n_records[m])[row()], each where given (ring_read).  A slab's (one channel): owned_out [0 .. n_records) the
// tracers it met per record, an array like the other two, and a draining read refills the rows it hands out with NaN.
void Tracers::read(hipStream_t st, int capacity, double *t_out, double *v_out, int *n_records, int64_t *n_dropped, int64_t *n_missing,
                   bool drain, int64_t *owned_out)
{
    if (!part) owned_out = nullptr;
    static_assert(sizeof(long long) == sizeof(int64_t), "n_owned is copied as it is");
    ring_read(*this, head, st, capacity, {t_out, times.get(), 2}, {v_out, values.get(), row()}, owned_out != nullptr, n_records, n_dropped,
              drain, [&](RingStage stage, const std::vector<TracerHead> &h, long long most) {
                  if (stage == RingStage::Rows && owned_out) {
                      if (most > 0) SPHX_HIP(hipMemcpyAsync(owned_out, n_owned.get(), (size_t)most * sizeof(int64_t), hipMemcpyDeviceToHost, st));
                      if (!(t_out || v_out)) SPHX_HIP(hipStreamSynchronize(st));
                  }
                  if (stage == RingStage::Counts && n_missing)
                      for (int m = 0; m < members; ++m) n_missing[m] = (int64_t)h[m].n_missing;
                  // (rows beyond n_records were never written: a dropped record stores no value)
                  if (stage == RingStage::Drain && part) nan_fill(st, (size_t)most);
              });
}

namespace {

// what is enqueued lands, then the read, the list and its length
void tracers_read(const Owner &o, int capacity, double *times, double *values, int32_t *ids, int *n_tracers, int *n_records,
                  int64_t *n_dropped, int64_t *n_missing, int drain)
{
    Tracers &t = sampler_settled(o, &sphx_ctx::tracers);  // (the records of everything enqueued)
    t.read(o.st, capacity, times, values, n_records, n_dropped, n_missing, drain != 0);
    if (ids) std::copy(t.ids.begin(), t.ids.end(), ids);
    if (n_tracers) *n_tracers = t.cfg.n_tracers;
}

}  // namespace

SPHX_EXPORT int sphx_ctx_tracers_enable(sphx_ctx *c, const sphx_tracers_config *cfg)
{
    SPHX_TRY
    const Owner o = ctx_owner(c);
    sampler_enable(o, &sphx_ctx::tracers, o.c->nf, o.c->nt, cfg, o.M);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_tracers_disable(sphx_ctx *c)
{
    SPHX_TRY
    sampler_disable(ctx_owner(c), &sphx_ctx::tracers);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_tracers_sample(sphx_ctx *c)
{
    SPHX_TRY
    sampler_sample(ctx_owner(c), &sphx_ctx::tracers, launch_tracers);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_tracers_read(sphx_ctx *c, int capacity, double *times, double *values, int32_t *ids, int *n_tracers,
                                      int *n_records, int64_t *n_dropped, int64_t *n_missing, int drain)
{
    SPHX_TRY
    tracers_read(ctx_owner(c), capacity, times, values, ids, n_tracers, n_records, n_dropped, n_missing, drain);
    return SPHX_OK;
    SPHX_CATCH
}

// ---- profile series ----

// every check of a configuration for M channels with parameters prm (cfg, n_bins, n_bands): the bins and bands as the flow
// statistics have them, the record buffer by the checks of ProbesShape::check; SPHX:ProfileSeries:config errors
void ProfileSeriesShape::check(const sphx_params &prm, const sphx_profile_series_config *cfg, int M)
{
    const char *id = "SPHX:ProfileSeries:config";
    require(cfg != nullptr, id, "config must not be NULL");
    require(cfg->n_bins >= 0, id, "n_bins must be >= 0 (0 = the reference's profile bins)");
    require(cfg->every >= 1, id, "every must be >= 1");
    require(cfg->capacity >= 1, id, "capacity must be >= 1");
    require(!std::isnan(cfg->t_from), id, "t_from must not be NaN");
    this->cfg = *cfg;
    bins_and_bands(id, prm, this->cfg, n_bins, n_bands);
    require((int64_t)n_bins * n_bands <= kStatsMaxBins, id, "n_bins * (n_bands + 1) must not exceed 1536 (the per-workgroup LDS counters)");
    if (!((double)M * (double)cfg->capacity * (double)n_bins * n_bands * kStatsFields <= (double)kSeriesMaxTotal))
        throw Error(SPHX_ERR_ARG, id,
                    std::string(M > 1 ? "n_members * " : "") + "capacity * (n_bands + 1) * n_bins * 5 must not exceed 1 << 27 doubles");
}

// the checked shape, and sums in flight, records and heads for M members
void ProfileSeries::alloc(const ProfileSeriesShape &checked, int M, hipStream_t)
{
    static_cast<ProfileSeriesShape &>(*this) = checked;
    members = M;
    isum.alloc(block() * M);
    times.alloc((size_t)M * cfg.capacity * 2);
    records.alloc((size_t)M * cfg.capacity * block());
    head.alloc(M);
}

// Every member's counts and its filled rows, into times[m][0 .. n_records[m])[2] and records[m][0 .. n_records[m])[block()],
// each where given (ring_read; SPHX:ProfileSeries:range when a member's sticky flag is up)
void ProfileSeries::read(hipStream_t st, int capacity, double *t_out, double *r_out, int *n_records, int64_t *n_dropped, bool drain)
{
    ring_read(*this, head, st, capacity, {t_out, times.get(), 2}, {r_out, records.get(), block()}, n_records, n_dropped, drain);
}

namespace {

// what is enqueued lands, then the read and the shape
void series_read(const Owner &o, int capacity, double *times, double *records, int *n_bins, int *n_bands, int *n_records,
                 int64_t *n_dropped, int drain)
{
    ProfileSeries &p = sampler_settled(o, &sphx_ctx::pseries);  // (the records of everything enqueued)
    p.read(o.st, capacity, times, records, n_records, n_dropped, drain != 0);
    if (n_bins) *n_bins = p.n_bins;
    if (n_bands) *n_bands = p.n_bands;
}

}  // namespace

SPHX_EXPORT int sphx_ctx_profile_series_enable(sphx_ctx *c, const sphx_profile_series_config *cfg)
{
    SPHX_TRY
    const Owner o = ctx_owner(c);
    sampler_enable(o, &sphx_ctx::pseries, o.c->prm, cfg, o.M);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_profile_series_disable(sphx_ctx *c)
{
    SPHX_TRY
    sampler_disable(ctx_owner(c), &sphx_ctx::pseries);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_profile_series_sample(sphx_ctx *c)
{
    SPHX_TRY
    sampler_sample(ctx_owner(c), &sphx_ctx::pseries, launch_profile_series);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_profile_series_read(sphx_ctx *c, int capacity, double *times, double *records, int *n_bins, int *n_bands,
                                             int *n_records, int64_t *n_dropped, int drain)
{
    SPHX_TRY
    series_read(ctx_owner(c), capacity, times, records, n_bins, n_bands, n_records, n_dropped, drain);
    return SPHX_OK;
    SPHX_CATCH
}

// ---- pair statistics ----

// every check of a configuration of channels with parameters prm (cfg, n_bins, n_bands, kinds, r_max); has_walls: the
// channel holds wall particles (without any, with_walls leaves fw at zero); SPHX:PairDist:config errors
void PairDistShape::check(const sphx_params &prm, const sphx_pair_dist_config *cfg, bool has_walls)
{
    const char *id = "SPHX:PairDist:config";
    require(cfg != nullptr, id, "config must not be NULL");
    require(cfg->n_bins >= 1 && cfg->n_bins <= kPairMaxBins, id, "n_bins must be 1 .. 1024");
    require(cfg->every >= 1, id, "every must be >= 1");
    require(!std::isnan(cfg->t_from), id, "t_from must not be NaN");
    const double two_h = 2.0 * prm.h;
    require(std::isfinite(cfg->r_max) && cfg->r_max >= 0.0 && cfg->r_max <= two_h, id,
            "r_max must be 0 (= 2h) or 0 < r_max <= 2h: beyond 2h the sweep of the three cell columns is not complete");
    require(std::isfinite(cfg->y_margin) && cfg->y_margin >= 0.0, id, "y_margin must be finite and >= 0");
    require(cfg->with_walls == 0 || cfg->with_walls == 1, id, "with_walls must be 0 or 1");
    this->cfg = *cfg;
    bins_and_bands(id, prm, this->cfg, n_bins, n_bands);
    kinds = cfg->with_walls && has_walls ? 2 : 1;
    r_max = cfg->r_max > 0.0 ? cfg->r_max : two_h;
}

// the checked shape, and sums and heads for M members
void PairDist::alloc(const PairDistShape &checked, int M, hipStream_t)
{
    static_cast<PairDistShape &>(*this) = checked;
    members = M;
    empty.assign(block() * M, 0ull);
    for (int m = 0; m < M; ++m)
        for (int b = 0; b < n_bands; ++b) empty[(size_t)m * block() + counters() + n_bands + b] = kPairInfBits;
    sums.alloc(block() * M);
    head.alloc(M);
}

// zero counts and centres, r2_min = +inf, no sample (`empty` lives as long as the sampler, and sampler_zero, the only caller,
// waits for the stream)
void PairDist::zero(hipStream_t st)
{
    SPHX_HIP(hipMemcpyAsync(sums.get(), empty.data(), empty.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    head.zero(st);
}

// Band `band` of every member's sums (ff / fw: into out[m * stride + bin], where given; fw: zeros without a wall histogram;
// centres[m], r2_min[m]) and the heads (n_samples[m], t_first[m], t_last[m], where given)
void PairDist::read(hipStream_t st, int band, int stride, int64_t *ff, int64_t *fw, int64_t *centres, double *r2_min, int64_t *n_samples,
                    double *t_first, double *t_last) const
{
    const int M = members;
    std::vector<unsigned long long> host(block() * M);
    std::vector<PairDistHead> h(M);
    SPHX_HIP(hipMemcpyAsync(host.data(), sums.get(), host.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    SPHX_HIP(hipMemcpyAsync(h.data(), head.get(), sizeof(PairDistHead) * M, hipMemcpyDeviceToHost, st));
    SPHX_HIP(hipStreamSynchronize(st));
    for (int m = 0; m < M; ++m) {
        const unsigned long long *blk = host.data() + (size_t)m * block();
        const unsigned long long *row = blk + (size_t)band * kinds * n_bins;
        for (int k = 0; k < n_bins; ++k) {
            if (ff) ff[(size_t)m * stride + k] = (int64_t)row[k];
            if (fw) fw[(size_t)m * stride + k] = kinds > 1 ? (int64_t)row[n_bins + k] : 0;
        }
        if (centres) centres[m] = (int64_t)blk[counters() + band];
        if (r2_min) std::memcpy(r2_min + m, blk + counters() + n_bands + band, sizeof(double));
        read_head(h[m], n_samples ? n_samples + m : nullptr, t_first ? t_first + m : nullptr, t_last ? t_last + m : nullptr);
    }
}

namespace {

// the argument checks of a read, then what is enqueued lands, and the read
void pair_dist_read(const Owner &o, int band, int capacity, int *n_bins, int64_t *ff, int64_t *fw, int64_t *centres, double *r2_min,
                    int64_t *n_samples, double *t_first, double *t_last)
{
    const PairDist &p = sampler_of(o, &sphx_ctx::pairs, true);
    require(band >= 0 && band < p.n_bands, "SPHX:PairDist:band", "band must be 0 (whole channel) .. n_bands");
    require((ff == nullptr && fw == nullptr) || capacity >= p.n_bins, "SPHX:PairDist:capacity", "capacity is smaller than the number of bins");
    o.settle();
    p.read(o.st, band, capacity, ff, fw, centres, r2_min, n_samples, t_first, t_last);
    if (n_bins) *n_bins = p.n_bins;
}

}  // namespace

SPHX_EXPORT int sphx_ctx_pair_dist_enable(sphx_ctx *c, const sphx_pair_dist_config *cfg)
{
    SPHX_TRY
    const Owner o = ctx_owner(c);
    sampler_enable(o, &sphx_ctx::pairs, o.c->prm, cfg, o.has_walls);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_pair_dist_disable(sphx_ctx *c)
{
    SPHX_TRY
    sampler_disable(ctx_owner(c), &sphx_ctx::pairs);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_pair_dist_reset(sphx_ctx *c)
{
    SPHX_TRY
    sampler_reset(ctx_owner(c), &sphx_ctx::pairs);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_pair_dist_sample(sphx_ctx *c)
{
    SPHX_TRY
    sampler_sample(ctx_owner(c), &sphx_ctx::pairs, launch_pair_dist);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_pair_dist_read(sphx_ctx *c, int band, int capacity, int *n_bins, int64_t *ff, int64_t *fw, int64_t *centres,
                                        double *r2_min, int64_t *n_samples, double *t_first, double *t_last)
{
    SPHX_TRY
    pair_dist_read(ctx_owner(c), band, capacity, n_bins, ff, fw, centres, r2_min, n_samples, t_first, t_last);
    return SPHX_OK;
    SPHX_CATCH
}

// ---- gradient statistics ----

// every check of a configuration of channels with parameters prm (cfg, n_bins, n_bands, walls); has_walls: the channel holds
// wall particles (without any, with_walls changes nothing); SPHX:GradStats:config errors
void GradStatsShape::check(const sphx_params &prm, const sphx_grad_stats_config *cfg, bool has_walls)
{
    const char *id = "SPHX:GradStats:config";
    require(cfg != nullptr, id, "config must not be NULL");
    require(cfg->n_bins >= 0, id, "n_bins must be >= 0 (0 = the reference's profile bins)");
    require(cfg->every >= 1, id, "every must be >= 1");
    require(!std::isnan(cfg->t_from), id, "t_from must not be NaN");
    require(std::isfinite(cfg->det_min) && cfg->det_min >= 0.0, id, "det_min must be finite and >= 0");
    require(cfg->with_walls == 0 || cfg->with_walls == 1, id, "with_walls must be 0 or 1");
    this->cfg = *cfg;
    bins_and_bands(id, prm, this->cfg, n_bins, n_bands);
    require((int64_t)n_bins * n_bands <= kGradMaxBins, id, "n_bins * (n_bands + 1) must not exceed 640 (the per-workgroup LDS counters)");
    walls = cfg->with_walls && has_walls;
}

// the checked shape, and sums and heads for M members
void GradStats::alloc(const GradStatsShape &checked, int M, hipStream_t)
{
    static_cast<GradStatsShape &>(*this) = checked;
    members = M;
    isum.alloc(block() * M);
    dsum.alloc(block() * M);
    head.alloc(M);
}

// Band `band` of every member's sums (into sums[(m * kGradFields + field) * stride + bin], where given) and the heads
// (n_samples[m], t_first[m], t_last[m], where given)
void GradStats::read(hipStream_t st, int band, int stride, double *sums, int64_t *n_samples, double *t_first, double *t_last) const
{
    const int M = members;
    std::vector<double> host(sums ? (size_t)M * row() : 0);
    std::vector<GradStatsHead> h(M);
    if (sums)  // one copy: a row of every member's block
        SPHX_HIP(hipMemcpy2DAsync(host.data(), row() * sizeof(double), dsum.get() + (size_t)band * row(), block() * sizeof(double),
                                  row() * sizeof(double), M, hipMemcpyDeviceToHost, st));
    SPHX_HIP(hipMemcpyAsync(h.data(), head.get(), sizeof(GradStatsHead) * M, hipMemcpyDeviceToHost, st));
    SPHX_HIP(hipStreamSynchronize(st));
    if (sums)
        for (int m = 0; m < M; ++m)
            for (int j = 0; j < kGradFields; ++j)
                for (int k = 0; k < n_bins; ++k)
                    sums[((size_t)m * kGradFields + j) * stride + k] = host[(size_t)m * row() + (size_t)k * kGradFields + j];
    for (int m = 0; m < M; ++m)
        read_head(h[m], n_samples ? n_samples + m : nullptr, t_first ? t_first + m : nullptr, t_last ? t_last + m : nullptr);
}

namespace {

// the argument checks of a read, then what is enqueued lands, and the read
void grad_stats_read(const Owner &o, int band, int capacity, int *n_bins, double *sums, int64_t *n_samples, double *t_first, double *t_last)
{
    const GradStats &f = sampler_of(o, &sphx_ctx::grads, true);
    require(band >= 0 && band < f.n_bands, "SPHX:GradStats:band", "band must be 0 (whole channel) .. n_bands");
    require(sums == nullptr || capacity >= f.n_bins, "SPHX:GradStats:capacity", "capacity is smaller than the number of bins");
    o.settle();
    f.read(o.st, band, capacity, sums, n_samples, t_first, t_last);
    if (n_bins) *n_bins = f.n_bins;
}

}  // namespace

SPHX_EXPORT int sphx_ctx_grad_stats_enable(sphx_ctx *c, const sphx_grad_stats_config *cfg)
{
    SPHX_TRY
    const Owner o = ctx_owner(c);
    sampler_enable(o, &sphx_ctx::grads, o.c->prm, cfg, o.has_walls);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_grad_stats_disable(sphx_ctx *c)
{
    SPHX_TRY
    sampler_disable(ctx_owner(c), &sphx_ctx::grads);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_grad_stats_reset(sphx_ctx *c)
{
    SPHX_TRY
    sampler_reset(ctx_owner(c), &sphx_ctx::grads);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_grad_stats_sample(sphx_ctx *c)
{
    SPHX_TRY
    sampler_sample(ctx_owner(c), &sphx_ctx::grads, launch_grad_stats);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_grad_stats_read(sphx_ctx *c, int band, int capacity, int *n_bins, double *sums, int64_t *n_samples, double *t_first,
                                         double *t_last)
{
    SPHX_TRY
    grad_stats_read(ctx_owner(c), band, capacity, n_bins, sums, n_samples, t_first, t_last);
    return SPHX_OK;
    SPHX_CATCH
}

// ---- density statistics ----

// every check of a configuration of channels with parameters prm (cfg, n_bins, n_bands, e); SPHX:DensStats:config errors
void DensStatsShape::check(const sphx_params &prm, const sphx_dens_stats_config *cfg)
{
    const char *id = "SPHX:DensStats:config";
    require(cfg != nullptr, id, "config must not be NULL");
    require(cfg->n_bins >= 0, id, "n_bins must be >= 0 (0 = the reference's profile bins)");
    require(cfg->every >= 1, id, "every must be >= 1");
    require(!std::isnan(cfg->t_from), id, "t_from must not be NaN");
    require(cfg->n_hist >= 1 && cfg->n_hist <= kDensMaxHist, id, "n_hist must be 1 .. 1024");
    require(cfg->delta_bound > 0.0 && cfg->delta_bound <= 0.5, id, "delta_bound must be in (0, 0.5]");  // (a NaN fails)
    require(cfg->hist_range > 0.0 && cfg->hist_range <= cfg->delta_bound, id, "hist_range must be in (0, delta_bound]");
    this->cfg = *cfg;
    bins_and_bands(id, prm, this->cfg, n_bins, n_bands);
    require(((uint64_t)dens_sum_words(n_bands, n_bins, cfg->n_hist) + dens_key_words(n_bands, n_bins)) * sizeof(unsigned long long)
                <= kDensMaxShmem,
            id, "(n_bands + 1) * (8 * n_bins + n_hist + 2) must not exceed 7680 (the 60 KB of LDS of a workgroup)");
    // 2^e >= delta_bound: frexp gives delta_bound = m 2^e with 0.5 <= m < 1, and m = 0.5 is the power of two itself
    int ex = 0;
    const double m = std::frexp(cfg->delta_bound, &ex);
    e = m == 0.5 ? ex - 1 : ex;
}

// the checked shape, and sums, keys and heads for M members
void DensStats::alloc(const DensStatsShape &checked, int M, hipStream_t)
{
    static_cast<DensStatsShape &>(*this) = checked;
    members = M;
    isum.alloc(block() * M);
    dsum.alloc(block() * M);
    keys.alloc(kblock() * M);
    head.alloc(M);
}

// Band `band` of member m: the binned sums with d_min and d_max behind them (into sums[field * stride + bin], where given),
// the histogram (hist[0 .. n_hist), below, above, where given) and the head (where given)
void DensStats::read(hipStream_t st, int m, int band, int stride, double *sums, int64_t *hist, int64_t *below, int64_t *above,
                     int64_t *n_samples, double *t_first, double *t_last) const
{
    std::vector<double> binned(row()), hrow_(hrow());
    std::vector<unsigned long long> k((size_t)n_bins * kDensKeys);
    DensStatsHead h{};
    const double *base = dsum.get() + (size_t)m * block();
    SPHX_HIP(hipMemcpyAsync(binned.data(), base + (size_t)band * row(), row() * sizeof(double), hipMemcpyDeviceToHost, st));
    SPHX_HIP(hipMemcpyAsync(hrow_.data(), base + (size_t)n_bands * row() + (size_t)band * hrow(), hrow() * sizeof(double),
                            hipMemcpyDeviceToHost, st));
    SPHX_HIP(hipMemcpyAsync(k.data(), keys.get() + (size_t)m * kblock() + (size_t)band * n_bins * kDensKeys, k.size() * sizeof(unsigned long long),
                            hipMemcpyDeviceToHost, st));
    SPHX_HIP(hipMemcpyAsync(&h, head.get() + m, sizeof(DensStatsHead), hipMemcpyDeviceToHost, st));
    SPHX_HIP(hipStreamSynchronize(st));
    // dens_key back to the double; 0: no particle yet
    auto unkey = [](unsigned long long key, double none) {
        if (!key) return none;
        const unsigned long long b = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
        double v;
        std::memcpy(&v, &b, sizeof(v));
        return v;
    };
    const double inf = std::numeric_limits<double>::infinity();
    if (sums)
        for (int b = 0; b < n_bins; ++b) {
            for (int j = 0; j < kDensFields; ++j) sums[(size_t)j * stride + b] = binned[(size_t)b * kDensFields + j];
            sums[(size_t)kDensFields * stride + b] = -unkey(k[(size_t)b * kDensKeys + 1], -inf);  // d_min (+inf before the first)
            sums[(size_t)(kDensFields + 1) * stride + b] = unkey(k[(size_t)b * kDensKeys], -inf);  // d_max (-inf before the first)
        }
    if (hist)
        for (int b = 0; b < cfg.n_hist; ++b) hist[b] = (int64_t)hrow_[b];
    if (below) *below = (int64_t)hrow_[cfg.n_hist];
    if (above) *above = (int64_t)hrow_[cfg.n_hist + 1];
    read_head(h, n_samples, t_first, t_last);
}

namespace {

// the argument checks of a read of member m, then what is enqueued lands, and the read
void dens_stats_read(const Owner &o, int m, int band, int capacity, int hist_capacity, int *n_bins, int *n_hist, double *sums, int64_t *hist,
                     int64_t *below, int64_t *above, int64_t *n_samples, double *t_first, double *t_last)
{
    const DensStats &f = sampler_of(o, &sphx_ctx::dens, true);
    require(band >= 0 && band < f.n_bands, "SPHX:DensStats:band", "band must be 0 (whole channel) .. n_bands");
    require(sums == nullptr || capacity >= f.n_bins, "SPHX:DensStats:capacity", "capacity is smaller than the number of bins");
    require(hist == nullptr || hist_capacity >= f.cfg.n_hist, "SPHX:DensStats:capacity",
            "hist_capacity is smaller than the number of histogram bins");
    o.settle();
    f.read(o.st, m, band, capacity, sums, hist, below, above, n_samples, t_first, t_last);
    if (n_bins) *n_bins = f.n_bins;
    if (n_hist) *n_hist = f.cfg.n_hist;
}

}  // namespace

SPHX_EXPORT int sphx_ctx_dens_stats_enable(sphx_ctx *c, const sphx_dens_stats_config *cfg)
{
    SPHX_TRY
    const Owner o = ctx_owner(c);
    sampler_enable(o, &sphx_ctx::dens, o.c->prm, cfg);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_dens_stats_disable(sphx_ctx *c)
{
    SPHX_TRY
    sampler_disable(ctx_owner(c), &sphx_ctx::dens);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_dens_stats_reset(sphx_ctx *c)
{
    SPHX_TRY
    sampler_reset(ctx_owner(c), &sphx_ctx::dens);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_dens_stats_sample(sphx_ctx *c)
{
    SPHX_TRY
    sampler_sample(ctx_owner(c), &sphx_ctx::dens, launch_dens_stats);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_dens_stats_read(sphx_ctx *c, int band, int capacity, int hist_capacity, int *n_bins, int *n_hist, double *sums,
                                         int64_t *hist, int64_t *below, int64_t *above, int64_t *n_samples, double *t_first, double *t_last)
{
    SPHX_TRY
    dens_stats_read(ctx_owner(c), 0, band, capacity, hist_capacity, n_bins, n_hist, sums, hist, below, above, n_samples, t_first, t_last);
    return SPHX_OK;
    SPHX_CATCH
}

// ---- mode amplitudes ----

// every check of a configuration for M channels (cfg): the modes by the kernel's limits, the record buffer by the checks of
// ProfileSeriesShape::check; SPHX:Modes:config errors
void ModesShape::check(const sphx_modes_config *cfg, int M)
{
    const char *id = "SPHX:Modes:config";
    require(cfg != nullptr, id, "config must not be NULL");
    require(cfg->mx >= 0 && cfg->mx <= kModesMax, id, "mx must be 0 .. 16");
    require(cfg->ny >= 0 && cfg->ny <= kModesMax, id, "ny must be 0 .. 16");
    require(cfg->every >= 1, id, "every must be >= 1");
    require(cfg->capacity >= 1, id, "capacity must be >= 1");
    require(!std::isnan(cfg->t_from), id, "t_from must not be NaN");
    if (!((double)M * (double)cfg->capacity * (double)(cfg->mx + 1) * (double)(cfg->ny + 1) * kModeSums <= (double)kSeriesMaxTotal))
        throw Error(SPHX_ERR_ARG, id,
                    std::string(M > 1 ? "n_members * " : "") + "capacity * (mx + 1) * (ny + 1) * 12 must not exceed 1 << 27 doubles");
    this->cfg = *cfg;
}

// the checked shape, and sums in flight, records and heads for M members
void Modes::alloc(const ModesShape &checked, int M, hipStream_t)
{
    static_cast<ModesShape &>(*this) = checked;
    members = M;
    isum.alloc(block() * M);
    times.alloc((size_t)M * cfg.capacity * 2);
    records.alloc((size_t)M * cfg.capacity * block());
    head.alloc(M);
}

// Every member's counts and its filled rows, into times[m][0 .. n_records[m])[2] and records[m][0 .. n_records[m])[block()],
// each where given (ring_read; SPHX:Modes:range when a member's sticky flag is up)
void Modes::read(hipStream_t st, int capacity, double *t_out, double *r_out, int *n_records, int64_t *n_dropped, bool drain)
{
    ring_read(*this, head, st, capacity, {t_out, times.get(), 2}, {r_out, records.get(), block()}, n_records, n_dropped, drain);
}

namespace {

// what is enqueued lands, then the read and the shape
void modes_read(const Owner &o, int capacity, double *times, double *records, int *mx, int *ny, int *n_records, int64_t *n_dropped, int drain)
{
    Modes &p = sampler_settled(o, &sphx_ctx::modes);  // (the records of everything enqueued)
    p.read(o.st, capacity, times, records, n_records, n_dropped, drain != 0);
    if (mx) *mx = p.cfg.mx;
    if (ny) *ny = p.cfg.ny;
}

}  // namespace

SPHX_EXPORT int sphx_ctx_modes_enable(sphx_ctx *c, const sphx_modes_config *cfg)
{
    SPHX_TRY
    const Owner o = ctx_owner(c);
    sampler_enable(o, &sphx_ctx::modes, cfg, o.M);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_modes_disable(sphx_ctx *c)
{
    SPHX_TRY
    sampler_disable(ctx_owner(c), &sphx_ctx::modes);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_modes_sample(sphx_ctx *c)
{
    SPHX_TRY
    sampler_sample(ctx_owner(c), &sphx_ctx::modes, launch_modes);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_ctx_modes_read(sphx_ctx *c, int capacity, double *times, double *records, int *mx, int *ny, int *n_records,
                                    int64_t *n_dropped, int drain)
{
    SPHX_TRY
    modes_read(ctx_owner(c), capacity, times, records, mx, ny, n_records, n_dropped, drain);
    return SPHX_OK;
    SPHX_CATCH
}

// ---- samplers of a slab ring (include/sphx.h section 3a) ----
// Flow statistics and step history of a skinned slab, recorded inside the library's own loops (sphx_slab_run,
// sphx_slab_group_run): a slab samples the particles it OWNS, what it keeps are partial sums, and the ring's value is the sum
// over its slabs.  The configurations, their checks, the layouts and the SPHX:Stats:* / SPHX:History:* identifiers are a
// context's (sections 2a, 2d); sphx_ctx_flow_stats_* / sphx_ctx_history_* keep refusing a slab.
// The velocity-field map: a node's sample is a ratio, so partial sums over owned particles cannot be pooled -- the NODES are
// divided among the slabs instead, a slab computes the complete sample of every node column it owns (field_block) from its
// owned particles and its halo copies, and the ring's map is the slabs' blocks side by side.
// The point probes: the same reasoning with points for nodes -- the POINTS are divided (probe_owner), a slab records the
// complete sample of every probe it owns, and the ring's series is the slabs' columns back in the list's order.
// The profile series: the flow statistics' reasoning -- a record is the slab's PARTIAL sample over the particles it owns, exact
// integers converted once, and the ring's record is the slabs' records added up field by field (sphx_slab_pseries_*: no
// function of include/sphx.h carries both "slab" and "profile_series" in its name).
// The pair statistics: a sample is a sum over CENTRES, so the flow statistics' reasoning holds for the centres -- a slab counts
// the pairs whose centre it owns, against every slot it holds, halo copies included (the field map's premise for the
// partners), and the ring's histogram is the slabs' added up, its r2_min their minimum (sphx_slab_pairs_*: no function of
// include/sphx.h carries both "slab" and "pair_dist" in its name).
// The gradient statistics: a sample is a sum over particles, so a slab bins the estimates of the particles it owns; an estimate
// takes its partners from every slot the slab holds, halo copies included -- their positions, velocities and masses (the field
// map's and the probes' premises) -- and the ring's sums are the slabs' added up, count and skipped included
// (sphx_slab_gstats_*: no function of include/sphx.h carries both "slab" and "grad" in its name).
// The density statistics: the gradient statistics' reasoning -- a slab bins the re-summed densities of the particles it owns; a
// density takes its partners' POSITIONS from every slot the slab holds, halo copies included (the pair statistics' premise),
// and the slab's wall particles, always; the ring's sums and histograms are the slabs' added up, d_min / d_max their minimum /
// maximum (sphx_slab_dstats_*: no function of include/sphx.h carries both "slab" and "dens" in its name).
// The particle tracers: the one sampler whose subject moves between the slabs.  A slab copies the tracked particles it OWNS at
// the sampled step -- the ring's id list and table on every rank, dense rows, NaN where it was not the owner -- and counts
// them per record (n_owned); every fluid row has one owner at every step, so the ring's record is each column taken from the
// one rank that wrote it, and the slabs' n_owned add up to T.  The halo is never read.

namespace {

// The samplers of slab c that are on, behind k_slab_pack3 of the step slot the host's parity names (slab_phase4 flips it
// later) and in front of everything of phase 3: the clock is the finished step's, S[1-q] holds the owned particles' new state,
// Vol / B (c->tmp) and the layout arrays (cell, mass) are those of the layout the step ran in -- clk->n is still that
// layout's count (k_slab_unpack3 sets the new one), so a re-binning step needs no src_of.  One self-skipping launch each,
// on the slab's stream, in the order statistics, history, map, probes, profile series, pair statistics, gradient statistics,
// tracers, density statistics;
// all off: nothing is enqueued, and a sampler that is off adds nothing to what the others enqueue.
void launch_slab_samplers(sphx_ctx *c)
{
    if (!c->fstats.on && !c->hist.on && !c->fmap.on && !c->probes.on && !c->pseries.on && !c->pairs.on && !c->grads.on && !c->tracers.on &&
        !c->dens.on)
        return;
    const int q = c->sched.cur;
    const Clock *clk = c->clock.get();
    const FluidSet s = c->view(1 - q, 0);
    // (workgroups from the capacity: what a slab holds changes with every re-binning, a launch captured in a graph does not)
    if (c->fstats.on)
        launch_s(c, "k_flow_stats_s", k_flow_stats_s, dim3(flow_stats_blocks((size_t)c->cap)), dim3(kStatsBlock), c->fstats.shmem(), clk, q,
                 flow_stats_args(c, s, c->fstats.cfg.every), c->grid, (const int *)s.cell);
    if (c->hist.on)
        launch_s(c, "k_step_history_s", k_step_history_s, dim3(history_blocks((size_t)c->cap)), dim3(kHistoryBlock), 0, clk, q, c->grid,
                 c->phys, s, c->tmp, c->walls, history_args(c, kHistoryInPlace), c->nf);
    // (pos, vel and the cell ranges of S[1-q]: the halo copies binned in the columns own - 1 and own + 1, which the clamped sweep
    //  reads beside the owned ones, were stepped like everything held and carry the finished step's state, DESIGN.md section 5;
    //  workgroups from the block of node columns, fixed at enable)
    if (c->fmap.on) {
        const FieldMap &f = c->fmap;
        FieldMapArgs a = field_map_args(c, f.cols(), c->fmap.cfg.every);
        a.step_x = c->prm.DL / (f.nx - 1);  // (the ring's grid, not the block's)
        a.with_walls = f.cfg.with_walls && c->walls.n > 0 ? 1 : 0;
        launch_s(c, "k_field_map_s", k_field_map_s, dim3(field_map_blocks(a)), dim3(kFieldBlock), 0, clk, q, c->grid, c->phys, s,
                 c->walls, a, f.i_lo, f.nx);
    }
    // (pos, vel, MASS and the cell ranges of S[1-q]: the view's mass is the layout array of the layout the step ran in, which a
    //  halo copy entered with its particle's mass at the last re-binning -- sphx_probes.hpp; workgroups from the owned probes,
    //  fixed at enable, at least one: a slab without a probe still stamps and counts the record)
    if (c->probes.on) {
        ProbeArgs a = probe_args(c, c->probes.cfg.every);
        a.with_walls = c->probes.cfg.with_walls && c->walls.n > 0 ? 1 : 0;
        launch_s(c, "k_point_probes_s", k_point_probes_s, dim3(std::max(probe_blocks(a), 1u)), dim3(kProbeBlock), 0, clk, q, c->grid,
                 c->phys, s, c->walls, a);
    }
    // (the flow statistics' workgroups, from the capacity; the record is the slab's partial sample, into its own buffer)
    if (c->pseries.on)
        launch_s(c, "k_profile_series_s", k_profile_series_s, dim3(flow_stats_blocks((size_t)c->cap)), dim3(kStatsBlock), c->pseries.shmem(),
                 clk, q, profile_series_args(c, s, c->pseries.cfg.every), c->grid, (const int *)s.cell);
    // (pos, the binned cells and the cell ranges of S[1-q], the halo copies in own - 1 and own + 1 as for the map; the centres
    //  are the owned slots of the clk->n held, so the workgroups come from the capacity; `kinds` was settled at enable from the
    //  slab's own wall particles)
    if (c->pairs.on)
        launch_s(c, "k_pair_dist_s", k_pair_dist_s, dim3(pair_dist_blocks((size_t)c->cap)), dim3(kPairBlock), c->pairs.shmem(), clk, q,
                 c->grid, s, c->walls, pair_dist_args(c, c->pairs.cfg.every));
    // (pos, VEL, MASS, the binned cells and the cell ranges of S[1-q]: the halo copies in own - 1 and own + 1 as for the map,
    //  their mass as for the probes; the particles of the sample are the owned slots of the clk->n held, so the workgroups come
    //  from the capacity; with_walls was settled at enable from the slab's own wall particles)
    if (c->grads.on)
        launch_s(c, "k_grad_stats_s", k_grad_stats_s, dim3(grad_stats_blocks((size_t)c->cap)), dim3(kGradBlock), c->grads.shmem(), clk, q,
                 c->grid, c->phys, s, c->walls, grad_stats_args(c, c->grads.cfg.every));
    // (pos, vel, the ids and the binned cells of S[1-q]: only slots the slab OWNS are copied, so nothing is asked of the halo;
    //  the scan runs over the clk->n held, bounded by the capacity, from which the workgroups come too; the table is the ring's)
    if (c->tracers.on) {
        TracerArgs a = tracer_args(c, c->tracers.cfg.every);
        a.n_slots = c->cap;
        launch_s(c, "k_tracers_s", k_tracers_s, dim3(tracer_blocks((size_t)c->cap)), dim3(kTracerBlock), 0, clk, q, s, a, c->grid,
                 c->tracers.n_owned.get());
    }
    // (pos, the binned cells and the cell ranges of S[1-q], the halo copies in own - 1 and own + 1 as for the pair statistics;
    //  MASS of the owned slot alone; the slab's wall particles always; the particles of the sample are the owned slots of the
    //  clk->n held, so the workgroups come from the capacity)
    if (c->dens.on)
        launch_s(c, "k_dens_stats_s", k_dens_stats_s, dim3(dens_stats_blocks((size_t)c->cap)), dim3(kDensBlock), c->dens.shmem(), clk, q,
                 c->grid, c->phys, s, c->walls, dens_stats_args(c, c->dens.cfg.every));
}

// The rank of slab c's ring that owns a probe at x, folded into [0, DL): rank r when edge(r) <= x < edge(r + 1), with
// edge(r) = ((r * ncx_ring) / n_ranks) * (DL / ncx_ring) -- the left edge of rank r's first cell column, the arithmetic of
// Grid::own_lo (slab_setup) and of field_block -- rank 0 from 0 and the last rank up to DL.  The edges ascend, so every x has
// exactly one owner, a point ON a cut (rank r's, never rank r - 1's) and both of two equal points included; every rank
// evaluates the same expression on the same list, and no kernel tests ownership in its own frame.
int probe_owner(const sphx_ctx *c, double x)
{
    const double csx = c->prm.DL / c->ncx_ring;
    int owner = 0;
    for (int r = 1; r < c->n_ranks; ++r)
        if (x >= (double)(((long long)r * c->ncx_ring) / c->n_ranks) * csx) owner = r;
    return owner;
}

// The block of node columns [i_lo, i_hi) of the ring's nx that slab c samples.  One monotone rule from the global cell-column
// boundaries, the same arithmetic on every rank: rank r's block starts at the first node column at or right of the left edge
// of its first cell column, x_i >= ((r * ncx_ring) / n_ranks) * (DL / ncx_ring) with x_i as the kernel and numpy's linspace
// make it; rank 0 starts at 0 and the last rank ends at nx, so node nx - 1 (x = DL) is the last slab's.  Rank r's i_hi is
// rank r + 1's i_lo by construction: the blocks partition [0, nx) wherever a node column falls, on a cut included, and no
// kernel tests ownership in its own frame.
void field_block(const sphx_ctx *c, int nx, int &i_lo, int &i_hi)
{
    const double DL = c->prm.DL, step = DL / (nx - 1), csx = DL / c->ncx_ring;
    auto first_node = [&](int r) {
        if (r <= 0) return 0;
        if (r >= c->n_ranks) return nx;
        const double edge = (double)(((long long)r * c->ncx_ring) / c->n_ranks) * csx;
        int i = std::clamp((int)std::ceil(edge / step), 0, nx);
        auto x_of = [&](int k) { return k == nx - 1 ? DL : (double)k * step; };
        while (i > 0 && x_of(i - 1) >= edge) --i;   // (the quotient's rounding: settle on the nodes' own coordinates)
        while (i < nx && x_of(i) < edge) ++i;
        return i;
    };
    i_lo = first_node(c->rank);
    i_hi = first_node(c->rank + 1);
}

// everything enqueued for slab c has run: its stream (a replayed ring graph runs ahead of it, release_from_first) and, where it
// has one, its second stream
void slab_settle(sphx_ctx *c)
{
    SPHX_HIP(hipStreamSynchronize(c->stream));
    if (c->stream2) SPHX_HIP(hipStreamSynchronize(c->stream2));
}

// A sampler of slab c goes on or off: a prepared step graph carries the launches as they were, so it is dropped -- this slab's
// own here, a ring's (held by its slab 0) by the epoch that slab_run compares -- and the loop runs eagerly until
// sphx_slab_graph_prepare is called again
void slab_samplers_changed(sphx_ctx *c)
{
    slab_settle(c);
    c->sampler_epoch += 1;
    if (c->steps_graph) { (void)hipGraphExecDestroy(c->steps_graph); c->steps_graph = nullptr; }
}

// a slab of the native loops, or SPHX:Slab:ctx / SPHX:Slab:protocol.  A configuration is checked in full before anything is
// changed: a refused one leaves a running sampler and a prepared step graph as they are
Owner slab_owner(sphx_ctx *c)
{
    require(c != nullptr && c->is_slab, "SPHX:Slab:ctx", "not a slab context");
    require(c->rebuild_every > 1, "SPHX:Slab:protocol",
            "the samplers of a slab live in sphx_slab_run / sphx_slab_group_run (a slab created with rebuild_every != 1)");
    return Owner{c, c->sched, c->stream, 1, "slab", c->walls.n > 0, [c] { slab_settle(c); }, false, [c] { slab_samplers_changed(c); }};
}

}  // namespace

SPHX_EXPORT int sphx_slab_flow_stats_enable(sphx_ctx *c, const sphx_flow_stats_config *cfg)
{
    SPHX_TRY
    const Owner o = slab_owner(c);
    sampler_enable(o, &sphx_ctx::fstats, o.c->prm, cfg);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_flow_stats_disable(sphx_ctx *c)
{
    SPHX_TRY
    sampler_disable(slab_owner(c), &sphx_ctx::fstats);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_flow_stats_reset(sphx_ctx *c)
{
    SPHX_TRY
    sampler_reset(slab_owner(c), &sphx_ctx::fstats);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_flow_stats_read(sphx_ctx *c, int band, int capacity, int *n_bins, double *count, double *sum_ux,
                                          double *sum_ux2, double *sum_uy, double *sum_uy2, int64_t *n_samples,
                                          double *t_first, double *t_last)
{
    SPHX_TRY
    stats_read(slab_owner(c), band, capacity, n_bins, count, sum_ux, sum_ux2, sum_uy, sum_uy2, n_samples, t_first, t_last);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_history_enable(sphx_ctx *c, const sphx_history_config *cfg)
{
    SPHX_TRY
    const Owner o = slab_owner(c);
    sampler_enable(o, &sphx_ctx::hist, cfg, o.M);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_history_disable(sphx_ctx *c)
{
    SPHX_TRY
    sampler_disable(slab_owner(c), &sphx_ctx::hist);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_history_read(sphx_ctx *c, int capacity, double *records, int *n_records, int64_t *n_dropped, int drain)
{
    SPHX_TRY
    const Owner o = slab_owner(c);
    sampler_settled(o, &sphx_ctx::hist).read(o.st, capacity, records, n_records, n_dropped, drain != 0);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_field_map_enable(sphx_ctx *c, const sphx_field_map_config *cfg)
{
    SPHX_TRY
    const Owner o = slab_owner(c);
    FieldMapShape checked;
    checked.check(c->prm, cfg, o.M);
    checked.part = true;
    field_block(c, checked.nx, checked.i_lo, checked.i_hi);
    sampler_on(o, &sphx_ctx::fmap, checked);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_field_map_disable(sphx_ctx *c)
{
    SPHX_TRY
    sampler_disable(slab_owner(c), &sphx_ctx::fmap);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_field_map_reset(sphx_ctx *c)
{
    SPHX_TRY
    sampler_reset(slab_owner(c), &sphx_ctx::fmap);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_field_map_read(sphx_ctx *c, int capacity, int *nx, int *ny, int *i_lo, int *i_hi, double *count,
                                         double *sum_w, double *sum_ux, double *sum_uy, double *sum_ux2, double *sum_uy2,
                                         int64_t *n_samples, double *t_first, double *t_last)
{
    SPHX_TRY
    const FieldMap &f = field_read(slab_owner(c), capacity, nx, ny, count, sum_w, sum_ux, sum_uy, sum_ux2, sum_uy2, n_samples, t_first,
                                   t_last);
    if (i_lo) *i_lo = f.i_lo;
    if (i_hi) *i_hi = f.i_hi;
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_probes_enable(sphx_ctx *c, const sphx_probes_config *cfg)
{
    SPHX_TRY
    const Owner o = slab_owner(c);
    ProbesShape checked;
    checked.check(c->prm, cfg, o.M);
    checked.part = true;
    for (int p = 0; p < checked.cfg.n_points; ++p)
        if (probe_owner(c, checked.folded[2 * (size_t)p]) == c->rank) checked.index.push_back(p);
    sampler_on(o, &sphx_ctx::probes, checked);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_probes_disable(sphx_ctx *c)
{
    SPHX_TRY
    sampler_disable(slab_owner(c), &sphx_ctx::probes);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_probes_read(sphx_ctx *c, int capacity, double *times, double *values, int *index, int *n_points_ring,
                                      int *n_owned, int *n_records, int64_t *n_dropped, int drain)
{
    SPHX_TRY
    const Owner o = slab_owner(c);
    Probes &p = sampler_settled(o, &sphx_ctx::probes);  // (the records of everything enqueued)
    const bool sizes_only = capacity == 0;  // nothing is copied and nothing drained
    p.read(o.st, capacity, sizes_only ? nullptr : times, sizes_only ? nullptr : values, n_records, n_dropped, !sizes_only && drain != 0);
    if (index) std::copy(p.index.begin(), p.index.end(), index);
    if (n_points_ring) *n_points_ring = p.cfg.n_points;
    if (n_owned) *n_owned = p.held();
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_pseries_enable(sphx_ctx *c, const sphx_profile_series_config *cfg)
{
    SPHX_TRY
    const Owner o = slab_owner(c);
    sampler_enable(o, &sphx_ctx::pseries, o.c->prm, cfg, o.M);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_pseries_disable(sphx_ctx *c)
{
    SPHX_TRY
    sampler_disable(slab_owner(c), &sphx_ctx::pseries);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_pseries_read(sphx_ctx *c, int capacity, double *times, double *records, int *n_bins, int *n_bands,
                                       int *n_records, int64_t *n_dropped, int drain)
{
    SPHX_TRY
    series_read(slab_owner(c), capacity, times, records, n_bins, n_bands, n_records, n_dropped, drain);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_pairs_enable(sphx_ctx *c, const sphx_pair_dist_config *cfg)
{
    SPHX_TRY
    const Owner o = slab_owner(c);
    sampler_enable(o, &sphx_ctx::pairs, o.c->prm, cfg, o.has_walls);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_pairs_disable(sphx_ctx *c)
{
    SPHX_TRY
    sampler_disable(slab_owner(c), &sphx_ctx::pairs);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_pairs_reset(sphx_ctx *c)
{
    SPHX_TRY
    sampler_reset(slab_owner(c), &sphx_ctx::pairs);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_pairs_read(sphx_ctx *c, int band, int capacity, int *n_bins, int64_t *ff, int64_t *fw, int64_t *centres,
                                     double *r2_min, int64_t *n_samples, double *t_first, double *t_last)
{
    SPHX_TRY
    pair_dist_read(slab_owner(c), band, capacity, n_bins, ff, fw, centres, r2_min, n_samples, t_first, t_last);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_gstats_enable(sphx_ctx *c, const sphx_grad_stats_config *cfg)
{
    SPHX_TRY
    const Owner o = slab_owner(c);
    sampler_enable(o, &sphx_ctx::grads, o.c->prm, cfg, o.has_walls);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_gstats_disable(sphx_ctx *c)
{
    SPHX_TRY
    sampler_disable(slab_owner(c), &sphx_ctx::grads);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_gstats_reset(sphx_ctx *c)
{
    SPHX_TRY
    sampler_reset(slab_owner(c), &sphx_ctx::grads);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_gstats_read(sphx_ctx *c, int band, int capacity, int *n_bins, double *sums, int64_t *n_samples, double *t_first,
                                      double *t_last)
{
    SPHX_TRY
    grad_stats_read(slab_owner(c), band, capacity, n_bins, sums, n_samples, t_first, t_last);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_dstats_enable(sphx_ctx *c, const sphx_dens_stats_config *cfg)
{
    SPHX_TRY
    const Owner o = slab_owner(c);
    sampler_enable(o, &sphx_ctx::dens, o.c->prm, cfg);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_dstats_disable(sphx_ctx *c)
{
    SPHX_TRY
    sampler_disable(slab_owner(c), &sphx_ctx::dens);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_dstats_reset(sphx_ctx *c)
{
    SPHX_TRY
    sampler_reset(slab_owner(c), &sphx_ctx::dens);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_dstats_read(sphx_ctx *c, int band, int capacity, int hist_capacity, int *n_bins, int *n_hist, double *sums,
                                      int64_t *hist, int64_t *below, int64_t *above, int64_t *n_samples, double *t_first, double *t_last)
{
    SPHX_TRY
    dens_stats_read(slab_owner(c), 0, band, capacity, hist_capacity, n_bins, n_hist, sums, hist, below, above, n_samples, t_first, t_last);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_tracers_enable(sphx_ctx *c, const sphx_tracers_config *cfg)
{
    SPHX_TRY
    const Owner o = slab_owner(c);
    TracersShape checked;
    checked.check(c->nf, c->nt, cfg, o.M);
    checked.part = true;
    sampler_on(o, &sphx_ctx::tracers, checked);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_tracers_disable(sphx_ctx *c)
{
    SPHX_TRY
    sampler_disable(slab_owner(c), &sphx_ctx::tracers);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_slab_tracers_read(sphx_ctx *c, int capacity, double *times, double *values, int64_t *n_owned, int32_t *ids,
                                       int *n_tracers, int *n_records, int64_t *n_dropped, int drain)
{
    SPHX_TRY
    const Owner o = slab_owner(c);
    Tracers &t = sampler_settled(o, &sphx_ctx::tracers);  // (the records of everything enqueued)
    const bool sizes_only = capacity == 0;  // nothing is copied and nothing drained
    t.read(o.st, capacity, sizes_only ? nullptr : times, sizes_only ? nullptr : values, n_records, n_dropped, nullptr,
           !sizes_only && drain != 0, sizes_only ? nullptr : n_owned);
    if (ids) std::copy(t.ids.begin(), t.ids.end(), ids);
    if (n_tracers) *n_tracers = t.cfg.n_tracers;
    return SPHX_OK;
    SPHX_CATCH
}
