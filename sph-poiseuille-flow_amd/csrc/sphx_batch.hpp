// sphx_batch.hpp -- batched contexts (include/sphx.h section 2b), part of the sphx_resident.hip translation unit.
//
// A batch steps M independent channels of one geometry with the launches of one: every step-slot kernel of the compact
// context runs as its "_b" form on a grid of (workgroups of one member) x M, member = blockIdx.y (Members,
// sphx_kernels.hpp).  Each member is an sphx_ctx whose device arrays are its blocks of batch-wide allocations (BatchArena):
// the cold paths -- creation, initial sort, downloads, monitors -- are the single-context code run on that member.  So is the
// step: the batch enqueues a context's step slot (ctx_slot: launch_step, then the slot samplers that are on) on member 0, which
// carries the member table, and the launch layer puts every kernel into its batch form (launch_forms).  The host
// schedule (re-binning slots, graph phases) is the batch's; every member has its own clock, so a member that has reached
// its target, used up its steps or stopped on the drift bound sits out the rest of the call.  When a call leaves members at
// different phases of the schedule, or one of them stopped on the drift bound, every member is re-binned into one phase at
// pos = 0 (a realignment) -- a change of summation order only.
#pragma once

struct sphx_batch {
    int M = 0;
    std::vector<sphx_ctx *> mem;  // mem[0]'s arrays are the bases of the batch-wide allocations
    BatchArena arena;
    hipStream_t stream = nullptr;
    DevBuf<Phys> phys;
    Members mb{};
    Clock *h_clocks = nullptr;        // pinned [M]: all clocks in one copy
    long long *h_budget = nullptr;    // pinned [M]: step budgets of an arm
    DevBuf<long long> budget;
    DevBuf<double> st_mass;           // realignment staging (one member at a time)
    DevBuf<int> st_id, st_src, out_id;  // (out_id: [M x cap], see sphx_ctx::out_ids)
    Schedule sched;                   // shared by all members: sched.slot counts the step slots the batch has taken (lockstep)
    int64_t epoch_slot = 0;           // sched.slot when the members' epochs were set
    int64_t n_realign = 0;
    std::vector<int64_t> pending;     // per member: step count the sphx_batch_enqueue_steps calls since the last sync aim for
    // (the ten slot samplers, sphx_batch_flow_stats_* ... sphx_batch_modes_*: mem[0]'s sampler members, for all M members --
    //  batch_owner, at the end of this file)

    ~sphx_batch()
    {
        if (stream) (void)hipStreamSynchronize(stream);
        sched.drop_graphs();
        for (sphx_ctx *c : mem) delete c;  // (before the arena their arrays live in)
        mem.clear();
        if (h_clocks) (void)hipHostFree(h_clocks);
        if (h_budget) (void)hipHostFree(h_budget);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

constexpr int kMaxBatchMembers = 4096;  // (grid rows; memory runs out first on large channels: sphx_batch_create reports it)

// arm every member's clock: one budget for all (max_steps) or one per member (b->h_budget, budgets = true)
void batch_arm(sphx_batch *b, double t_target, long long max_steps, bool budgets)
{
    for (sphx_ctx *c : b->mem) c->host_seq += 1;
    const long long *dev_budget = nullptr;
    if (budgets) {
        SPHX_HIP(hipMemcpyAsync(b->budget.get(), b->h_budget, sizeof(long long) * b->M, hipMemcpyHostToDevice, b->stream));
        dev_budget = b->budget.get();
    }
    hipLaunchKernelGGL(k_prepare_b, dim3(1, b->M), dim3(1), 0, b->stream, b->mb, t_target, max_steps, dev_budget, b->sched.cur);
    SPHX_HIP(hipGetLastError());
}

// every member at the batch's phase, epoch = now (its cool-down expressed in its own step count)
void batch_set_epochs(sphx_batch *b)
{
    for (sphx_ctx *c : b->mem) {
        c->sched.cur = b->sched.cur; c->sched.lay = b->sched.lay; c->sched.pos = b->sched.pos;
        set_epoch(c);
        c->sched.cool_until = c->h_clock->step + std::max<int64_t>(0, b->sched.cool_until - b->sched.slot);
    }
    b->epoch_slot = b->sched.slot;
}

// Re-bin member m from wherever its state is into (Q, L), pos 0.  The source is staged first, so any (Q, L) will do; the
// outputs of the member's last step stay where they are, reachable through out_ids / src_of (see sphx_ctx::out_ids).
void realign_member(sphx_batch *b, int m, int Q, int L)
{
    sphx_ctx *c = b->mem[m];
    hipStream_t st = b->stream;
    const int n = c->h_clock->n, q = c->sched.cur, l = c->sched.lay;
    const FluidSet s = c->view(q, l), d = c->view(Q, L);
    const bool outputs = c->have_step_outputs;
    const bool mapped = outputs && (c->out_ids != nullptr || c->out_lay != l);  // src_of: current slot -> output slot
    auto copy = [&](void *dst, const void *src, size_t bytes) {
        SPHX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
    };
    if (outputs && !c->out_ids) {
        int *ids = b->out_id.get() + (size_t)m * c->cap;
        copy(ids, c->fid_[c->out_lay].get(), sizeof(int) * n);
        c->out_ids = ids;
    }
    if (mapped) copy(b->st_src.get(), c->src_of.get(), sizeof(int) * n);
    copy(c->posn.get(), s.pos, sizeof(double2) * n);
    copy(c->veln.get(), s.vel, sizeof(double2) * n);
    copy(c->drhon.get(), s.drho, sizeof(double) * n);
    copy(b->st_mass.get(), s.mass, sizeof(double) * n);
    copy(b->st_id.get(), s.id, sizeof(int) * n);
    host_rebin(c, n, c->posn.get(), c->cellid.get(), c->count.get(), d.start, c->perm.get(),
               reorder_args(c->posn.get(), c->veln.get(), c->drhon.get(), b->st_mass.get(), b->st_id.get(), d, c->src_of.get()));
    if (mapped) hipLaunchKernelGGL(k_compose, dim3(div_up(n, kBlock)), dim3(kBlock), 0, st, n, (const int *)b->st_src.get(), c->src_of.get());
    hipLaunchKernelGGL(k_rebinned, dim3(1), dim3(1), 0, st, c->clock.get());
    SPHX_HIP(hipGetLastError());
    c->sched.cur = Q; c->sched.lay = L; c->sched.pos = 0;
    c->h_clock->need_rebuild = 0;
    c->h_clock->drift = 0.0;
    if (c->h_pub) { c->h_pub->need_rebuild = 0; c->h_pub->drift = 0.0; }
}

// all members into one phase at pos 0; forced: because the drift bound was hit (batch-wide cool-down, as forced_rebuild)
void realign(sphx_batch *b, bool forced)
{
    Schedule &s = b->sched;
    const int Q = 1 - b->mem[0]->sched.cur, L = 1 - b->mem[0]->sched.lay;
    for (int m = 0; m < b->M; ++m) realign_member(b, m, Q, L);
    SPHX_HIP(hipStreamSynchronize(b->stream));
    s.cur = Q; s.lay = L; s.pos = 0;
    b->n_realign += 1;
    if (forced) {
        s.cool_down(s.slot, b->mem[0]->rebuild_every);
        if (debug_switches().log)
            fprintf(stderr, "sphx: batch forced re-binning #%lld at slot %lld\n", (long long)s.n_forced, (long long)s.slot);
    }
    batch_set_epochs(b);
}

void batch_throw_on_status(const sphx_batch *b)
{
    for (int m = 0; m < b->M; ++m) {
        const int st = b->mem[m]->h_clock->status;
        if (st == 0) continue;
        const std::string who = "member " + std::to_string(m) + ": ";
        if (st == SPHX_ERR_GRID) throw Error(SPHX_ERR_GRID, "SPHX:Batch:grid", who + "neighbour list capacity exceeded on device");
        throw Error(st, "SPHX:Batch:diverged", who + "device step loop raised a status (non-finite velocity)");
    }
}

// Wait, read every clock, replay each member's executed steps from the epoch; realign when the members ended up at
// different phases or one of them stopped on the drift bound.  Returns the steps each member executed.
std::vector<int64_t> batch_read(sphx_batch *b)
{
    wait_stream(b->mem[0]);
    SPHX_HIP(hipMemcpyAsync(b->h_clocks, b->mb.clk, sizeof(Clock) * b->M, hipMemcpyDeviceToHost, b->stream));
    SPHX_HIP(hipStreamSynchronize(b->stream));
    std::vector<int64_t> ex(b->M);
    int64_t e_max = 0;
    bool same = true, drift = false, bad = false;
    for (int m = 0; m < b->M; ++m) {
        sphx_ctx *c = b->mem[m];
        *c->h_clock = b->h_clocks[m];
        ex[m] = c->h_clock->step - c->epoch_step;
        replay_executed(c);  // (ends with set_epoch)
        if (ex[m] > 0) c->out_ids = nullptr;  // a new step wrote new outputs in the current layout
        e_max = std::max(e_max, ex[m]);
        const sphx_ctx *c0 = b->mem[0];
        same = same && c->sched.cur == c0->sched.cur && c->sched.lay == c0->sched.lay && c->sched.pos == c0->sched.pos;
        drift = drift || c->h_clock->need_rebuild;
        bad = bad || c->h_clock->status != 0;
    }
    b->sched.slot = b->epoch_slot + e_max;
    if (bad) return ex;  // (the caller throws; nothing is stepped again)
    if (same && !drift) {
        const Schedule &s0 = b->mem[0]->sched;
        b->sched.cur = s0.cur; b->sched.lay = s0.lay; b->sched.pos = s0.pos;
        batch_set_epochs(b);
    } else {
        realign(b, drift);
    }
    return ex;
}

// Step every member until it reaches t_target (clipped to t_end) or its budget (h_budget semantics: < 0 unlimited)
void batch_run(sphx_batch *b, double t_target, std::vector<int64_t> budget)
{
    for (int guard = 0; guard < 1000000; ++guard) {
        batch_throw_on_status(b);
        int64_t want = 0, most = 0;
        bool limited = true;
        for (int m = 0; m < b->M; ++m) {
            const sphx_ctx *c = b->mem[m];
            const Clock &k = *c->h_clock;
            const double goal = std::min(t_target, k.t_end);
            if (budget[m] == 0 || !(k.t < goal - 1e-12)) continue;
            const double dt_est = host_dt_unclipped(c, k.vmax);
            // A non-finite max |v| (a NaN or Inf in the state as given) makes the estimate NaN or absurd, and its conversion
            // to an integer left `want` at 0: a batch whose every member was non-finite took no step and raised nothing.
            // Such a member asks for one slot; arming its clock raises SPHX_ERR_DIVERGED on the device (prepare_clock).
            const double n_est = std::ceil(std::max(0.0, goal - k.t) / std::max(dt_est, 1e-12));
            want = std::max<int64_t>(want, std::isfinite(k.vmax) && n_est < 9e18 ? (int64_t)n_est + 1 : 1);
            if (budget[m] < 0) limited = false;
            else most = std::max(most, budget[m]);
        }
        if (want == 0) break;
        int64_t slots = std::min<int64_t>(want, b->sched.n_forced ? 256 : 4096);
        bool exact = false;
        const int K = b->mem[0]->rebuild_every, per_graph = graph_slots(b->mem[0]);
        if (limited && slots >= most) { slots = most; exact = true; }
        else if (slots > per_graph) slots = ((slots + per_graph - 1) / per_graph) * per_graph;
        // (k_prepare: a budget <= 0 is "unlimited"; a member whose budget is used up is armed and disarmed at once, so that
        //  it sits the call out)
        for (int m = 0; m < b->M; ++m) b->h_budget[m] = budget[m] > 0 ? budget[m] : (budget[m] == 0 ? 1 : -1);
        batch_arm(b, t_target, 0, true);
        for (int m = 0; m < b->M; ++m)
            if (budget[m] == 0) hipLaunchKernelGGL(k_disarm, dim3(1), dim3(1), 0, b->stream, b->mem[m]->clock.get());
        enqueue_slots(b->sched, b->stream, K, per_graph, slots, exact, ctx_slot(b->mem[0]), [b, K] { b->sched.advance(K); });
        const std::vector<int64_t> ex = batch_read(b);
        for (int m = 0; m < b->M; ++m)
            if (budget[m] > 0) budget[m] = std::max<int64_t>(0, budget[m] - ex[m]);
    }
    batch_throw_on_status(b);
    for (int m = 0; m < b->M; ++m) b->pending[m] = b->mem[m]->h_clock->step;
    for (sphx_ctx *c : b->mem) c->pending_target = c->h_clock->step;
}

// what sphx_batch_enqueue_steps calls still owe, then status
void batch_settle(sphx_batch *b)
{
    batch_read(b);
    std::vector<int64_t> owed(b->M);
    for (int m = 0; m < b->M; ++m) owed[m] = std::max<int64_t>(0, b->pending[m] - b->mem[m]->h_clock->step);
    batch_run(b, std::numeric_limits<double>::infinity(), owed);
}

void batch_check_member(const sphx_batch *b, int m)
{
    require(b != nullptr, "SPHX:Batch:null", "batch must not be NULL");
    if (m < 0 || m >= b->M)
        throw Error(SPHX_ERR_ARG, "SPHX:Batch:member", "member " + std::to_string(m) + " out of range [0, " + std::to_string(b->M) + ")");
}

// The batch as the owner of its samplers (sphx_samplers.hpp): member 0's sampler members serve all M members on the batch's
// schedule and stream.  An enable checks and goes on -- there is nothing to settle beyond the stream synchronisation of
// sampler_off; a reset, a sample and a read settle what sphx_batch_enqueue_steps still owes first.
Owner batch_owner(sphx_batch *b)
{
    require(b != nullptr, "SPHX:Batch:null", "batch must not be NULL");
    return Owner{b->mem[0], b->sched, b->stream, b->M, "batch", b->mem[0]->nw > 0, [b] { batch_settle(b); }, false, {}};
}

// argument checks (no device): shared fields, refused modes, the kernel forms members of this size would run
void batch_check(int M, const sphx_params *prm, int n_fluid, int n_total, const double *pos, const double *vel,
                 const double *drho_dt, const double *mass, const double *wall_vel)
{
    if (M < 1 || M > kMaxBatchMembers)
        throw Error(SPHX_ERR_ARG, "SPHX:Batch:members", "n_members must be 1.." + std::to_string(kMaxBatchMembers));
    require(prm != nullptr, "SPHX:Ctx:params", "params must not be NULL");
    require(pos && vel && drho_dt && mass && wall_vel, "SPHX:Batch:null", "pos / vel / drho_dt / mass / wall_vel must not be NULL");
    for (int m = 0; m < M; ++m) common_checks(&prm[m], n_fluid, n_total);
    auto differs = [&](int m, const char *field) {
        throw Error(SPHX_ERR_ARG, "SPHX:Batch:geometry",
                    std::string("member ") + std::to_string(m) + ": " + field + " differs from member 0 (members share one geometry)");
    };
    const sphx_params &p0 = prm[0];
    for (int m = 0; m < M; ++m) {
        const sphx_params &p = prm[m];
        if (p.dual_rate > 1)
            throw Error(SPHX_ERR_ARG, "SPHX:Batch:mode", "member " + std::to_string(m) + ": batches run the single-rate loop (dual_rate <= 1)");
        if (p.dynamic_rebin == 1)
            throw Error(SPHX_ERR_ARG, "SPHX:Batch:mode", "member " + std::to_string(m) + ": batches re-bin on the host's schedule (dynamic_rebin != 1)");
        if (p.dp != p0.dp) differs(m, "dp");
        if (p.DL != p0.DL) differs(m, "DL");
        if (p.DH != p0.DH) differs(m, "DH");
        if (p.h != p0.h) differs(m, "h");
        if (p.rho0 != p0.rho0) differs(m, "rho0");
        if (p.inv_sigma0 != p0.inv_sigma0) differs(m, "inv_sigma0");
        if (p.t_end != p0.t_end) differs(m, "t_end");
        if (p.lanes_per_particle != p0.lanes_per_particle) differs(m, "lanes_per_particle");
        if (p.steps_per_graph != p0.steps_per_graph) differs(m, "steps_per_graph");
        if (p.rebuild_every != p0.rebuild_every) differs(m, "rebuild_every");
        if (p.skin_h != p0.skin_h) differs(m, "skin_h");
        if (p.dynamic_rebin != p0.dynamic_rebin) differs(m, "dynamic_rebin");
    }
    const size_t nt = (size_t)n_total, nf = (size_t)n_fluid;
    for (int m = 1; m < M; ++m) {
        const double *pm = pos + 2 * nt * m;
        for (size_t k = nf; k < nt; ++k)
            if (pm[k] != pos[k] || pm[nt + k] != pos[nt + k]) differs(m, "wall positions");
    }
    sphx_ctx c0;
    for (int m = 0; m < M; ++m) {
        sphx_ctx c;
        ctx_configure(&c, &prm[m], n_fluid, n_total, pos + 2 * nt * m);
        if (m == 0) ctx_configure(&c0, &prm[0], n_fluid, n_total, pos);
        if (c.lpp < 16 || c.dyn)
            throw Error(SPHX_ERR_ARG, "SPHX:Batch:size", "channels of this size run the large-channel kernels (" + std::to_string(c.lpp) +
                                                          " lanes per particle" + (c.dyn ? ", device-decided re-binning" : "") +
                                                          "); batches run the compact kernels (16 or 32 lanes per particle)");
        if (c.grid.ncells > kBigScanCells || div_up((size_t)c.nf * c.lpp, kBlock) > (size_t)(4 * kMaxTile))
            throw Error(SPHX_ERR_ARG, "SPHX:Batch:size", "channel too large for a batch (cells scanned by one workgroup, per-workgroup "
                                                          "maxima reduced by one workgroup)");
        if (c.lpp != c0.lpp) differs(m, "lanes per particle");
        if (c.rebuild_every != c0.rebuild_every || c.skin != c0.skin) differs(m, "re-binning interval / skin");
        if (c.grid.ncx != c0.grid.ncx || c.grid.ncy != c0.grid.ncy || c.grid.y0 != c0.grid.y0) differs(m, "cell grid (y extent)");
    }
}

}  // namespace

SPHX_EXPORT int sphx_batch_create(sphx_batch **out, int n_members, const sphx_params *prm, int n_fluid, int n_total,
                                  const double *pos, const double *vel, const double *drho_dt, const double *mass,
                                  const double *wall_vel, double t0, int64_t step0)
{
    sphx_batch *b = nullptr;
    try {
        require(out != nullptr, "SPHX:Batch:out", "batch output pointer must not be NULL");
        batch_check(n_members, prm, n_fluid, n_total, pos, vel, drho_dt, mass, wall_vel);
        ensure_device();
        const int M = n_members;
        const size_t nt = (size_t)n_total;
        b = new sphx_batch();
        b->M = M;
        b->arena.n_members = M;
        b->pending.assign(M, step0);
        SPHX_HIP(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
        std::vector<int> wid((size_t)std::max(n_total - n_fluid, 1));
        for (int k = 0; k < n_total - n_fluid; ++k) wid[k] = n_fluid + k;
        std::vector<Phys> ph(M);
        for (int m = 0; m < M; ++m) {
            sphx_ctx *c = new sphx_ctx();
            b->mem.push_back(c);
            const double *pm = pos + 2 * nt * m, *vm = vel + 2 * nt * m, *dm = drho_dt + nt * m;
            ctx_configure(c, &prm[m], n_fluid, n_total, pm);
            c->stream = b->stream;
            c->own_stream = false;
            c->arena = &b->arena;
            c->member = m;
            SPHX_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->h_clock), sizeof(Clock), hipHostMallocDefault));
            ctx_alloc(c, n_fluid);
            upload_fluid(c, n_fluid, pm, pm + nt, vm, vm + nt, dm, mass, nullptr, true);
            if (m == 0) {
                upload_walls(c, n_total - n_fluid, pm + n_fluid, pm + nt + n_fluid, mass + n_fluid, wall_vel + n_fluid,
                             wall_vel + nt + n_fluid, wid.data(), true);
            } else {  // walls, wall cells and grid: member 0's
                const sphx_ctx *c0 = b->mem[0];
                c->wpos.alias(c0->wpos.get(), c0->wpos.size()); c->wa.alias(c0->wa.get(), c0->wa.size());
                c->wid.alias(c0->wid.get(), c0->wid.size()); c->wstart.alias(c0->wstart.get(), c0->wstart.size());
                c->wrow_any.alias(c0->wrow_any.get(), c0->wrow_any.size());
                c->walls = c0->walls;
            }
            init_clock(c, n_fluid, t0, step0);
            ph[m] = c->phys;
        }
        sphx_ctx *c0 = b->mem[0];
        for (sphx_ctx *c : b->mem) read_clock(c);
        b->phys.alloc(M);
        b->phys.upload(ph.data(), M, b->stream);
        b->mb = Members{c0->clock.get(), b->phys.get(), (long long)c0->cap, c0->grid.ncells + 1, c0->n_vpart, c0->tmp.nl_stride,
                        (long long)c0->tmp.nl_stride * c0->tmp.nl_cap, (long long)c0->tmp.nl_stride * c0->tmp.sl_cap};
        c0->members = &b->mb;  // member 0 stands for the batch in the step's launch layer
        c0->n_members = M;
        if (M > 1 && (b->mem[1]->clock.get() != c0->clock.get() + 1 || b->mem[1]->fpos_[0].get() != c0->fpos_[0].get() + c0->cap ||
                      b->mem[1]->nl_idx.get() != c0->nl_idx.get() + b->mb.list))
            throw Error(SPHX_ERR_STATE, "SPHX:Batch:internal", "member arrays are not laid out at the member strides");
        b->st_mass.alloc(c0->cap); b->st_id.alloc(c0->cap); b->st_src.alloc(c0->cap);
        b->out_id.alloc((size_t)M * c0->cap);
        b->budget.alloc(M);
        SPHX_HIP(hipHostMalloc(reinterpret_cast<void **>(&b->h_clocks), sizeof(Clock) * M, hipHostMallocDefault));
        SPHX_HIP(hipHostMalloc(reinterpret_cast<void **>(&b->h_budget), sizeof(long long) * M, hipHostMallocDefault));
        SPHX_HIP(hipStreamSynchronize(b->stream));
        batch_set_epochs(b);
        if (prm[0].t_end > t0) (void)capture_slots(b->sched, b->stream, c0->rebuild_every, graph_slots(c0), ctx_slot(b->mem[0]));
        *out = b;
        return SPHX_OK;
    } catch (const Error &e) {
        delete b;
        return report(e);
    } catch (const std::exception &e) {
        delete b;
        return report_unknown(e);
    }
}

SPHX_EXPORT void sphx_batch_destroy(sphx_batch *b)
{
    delete b;
}

SPHX_EXPORT int sphx_batch_advance(sphx_batch *b, double t_target, int64_t max_steps, sphx_status *status)
{
    SPHX_TRY
    require(b != nullptr, "SPHX:Batch:null", "batch must not be NULL");
    batch_settle(b);  // sphx_batch_enqueue_steps calls may still be in flight
    batch_run(b, t_target, std::vector<int64_t>(b->M, max_steps > 0 ? max_steps : -1));
    if (status)
        for (int m = 0; m < b->M; ++m) fill_status(b->mem[m], &status[m]);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_enqueue_steps(sphx_batch *b, int64_t n_steps)
{
    SPHX_TRY
    require(b != nullptr, "SPHX:Batch:null", "batch must not be NULL");
    require(n_steps > 0, "SPHX:Batch:steps", "n_steps must be positive");
    // no host sync: a member that stopped early (end time, status, drift bound) stays stopped when k_prepare re-evaluates its
    // loop condition; sphx_batch_sync realigns and takes the steps still owed
    const int K = b->mem[0]->rebuild_every;
    batch_arm(b, b->mem[0]->prm.t_end, (long long)n_steps, false);
    enqueue_slots(b->sched, b->stream, K, graph_slots(b->mem[0]), n_steps, true, ctx_slot(b->mem[0]), [b, K] { b->sched.advance(K); });
    for (int m = 0; m < b->M; ++m) b->pending[m] = std::max<int64_t>(b->pending[m], b->mem[m]->h_clock->step) + n_steps;
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_sync(sphx_batch *b, sphx_status *status)
{
    SPHX_TRY
    require(b != nullptr, "SPHX:Batch:null", "batch must not be NULL");
    batch_settle(b);
    if (status)
        for (int m = 0; m < b->M; ++m) fill_status(b->mem[m], &status[m]);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_download(sphx_batch *b, int member, double *pos, double *vel, double *rho, double *p, double *drho_dt,
                                    double *force, double *force_prior, double *Vol, double *B)
{
    SPHX_TRY
    batch_check_member(b, member);
    batch_settle(b);
    SPHX_CATCH
    return sphx_ctx_download(b->mem[member], pos, vel, rho, p, drho_dt, force, force_prior, Vol, B);
}

SPHX_EXPORT int sphx_batch_monitor(sphx_batch *b, int member, double *tau_bottom, double *tau_top, double *n_pairs)
{
    SPHX_TRY
    batch_check_member(b, member);
    batch_settle(b);
    SPHX_CATCH
    return sphx_ctx_monitor(b->mem[member], tau_bottom, tau_top, n_pairs);
}

SPHX_EXPORT int sphx_batch_info(sphx_batch *b, int *n_members, int *lanes_per_particle, int *steps_per_graph, int *rebuild_every,
                                double *skin, int64_t *forced_rebuilds, int64_t *realignments)
{
    SPHX_TRY
    require(b != nullptr, "SPHX:Batch:null", "batch must not be NULL");
    const sphx_ctx *c = b->mem[0];
    if (n_members) *n_members = b->M;
    if (lanes_per_particle) *lanes_per_particle = c->lpp;
    if (steps_per_graph) *steps_per_graph = graph_slots(c);
    if (rebuild_every) *rebuild_every = c->rebuild_every;
    if (skin) *skin = c->skin;
    if (forced_rebuilds) *forced_rebuilds = b->sched.n_forced;
    if (realignments) *realignments = b->n_realign;
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_graph_stats(sphx_batch *b, int64_t *slots_replayed, int64_t *slots_eager, int64_t *graphs_captured)
{
    SPHX_TRY
    require(b != nullptr, "SPHX:Batch:null", "batch must not be NULL");
    if (slots_replayed) *slots_replayed = b->sched.slots_replayed;
    if (slots_eager) *slots_eager = b->sched.slots_eager;
    if (graphs_captured) *graphs_captured = b->sched.graphs_captured;
    return SPHX_OK;
    SPHX_CATCH
}

// ---- the slot samplers of every member: a context's (sphx_samplers.hpp) over batch_owner ----
// One configuration for all members -- bins, bands, shapes, points, ids and the walls come from the shared geometry -- each
// member sampled on its own clock.  Out of device memory on enable: the batch goes on without the sampler.  A "sample now" is
// taken with every member at the batch's phase: the state sphx_batch_download would return.

// ---- flow statistics (include/sphx.h section 2c) ----

SPHX_EXPORT int sphx_batch_flow_stats_enable(sphx_batch *b, const sphx_flow_stats_config *cfg)
{
    SPHX_TRY
    const Owner o = batch_owner(b);
    sampler_enable(o, &sphx_ctx::fstats, o.c->prm, cfg);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_flow_stats_disable(sphx_batch *b)
{
    SPHX_TRY
    sampler_disable(batch_owner(b), &sphx_ctx::fstats);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_flow_stats_reset(sphx_batch *b)
{
    SPHX_TRY
    sampler_reset(batch_owner(b), &sphx_ctx::fstats);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_flow_stats_sample(sphx_batch *b)
{
    SPHX_TRY
    sampler_sample(batch_owner(b), &sphx_ctx::fstats, launch_flow_stats);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_flow_stats_read(sphx_batch *b, int band, int capacity, int *n_bins, double *count, double *sum_ux,
                                           double *sum_ux2, double *sum_uy, double *sum_uy2, int64_t *n_samples,
                                           double *t_first, double *t_last)
{
    SPHX_TRY
    stats_read(batch_owner(b), band, capacity, n_bins, count, sum_ux, sum_ux2, sum_uy, sum_uy2, n_samples, t_first, t_last);
    return SPHX_OK;
    SPHX_CATCH
}

// ---- step history (include/sphx.h section 2f) ----

SPHX_EXPORT int sphx_batch_history_enable(sphx_batch *b, const sphx_history_config *cfg)
{
    SPHX_TRY
    const Owner o = batch_owner(b);
    sampler_enable(o, &sphx_ctx::hist, cfg, o.M);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_history_disable(sphx_batch *b)
{
    SPHX_TRY
    sampler_disable(batch_owner(b), &sphx_ctx::hist);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_history_read(sphx_batch *b, int capacity, double *records, int *n_records, int64_t *n_dropped, int drain)
{
    SPHX_TRY
    const Owner o = batch_owner(b);
    sampler_settled(o, &sphx_ctx::hist).read(o.st, capacity, records, n_records, n_dropped, drain != 0);
    return SPHX_OK;
    SPHX_CATCH
}

// ---- velocity-field map (include/sphx.h section 2g) ----

SPHX_EXPORT int sphx_batch_field_map_enable(sphx_batch *b, const sphx_field_map_config *cfg)
{
    SPHX_TRY
    const Owner o = batch_owner(b);
    sampler_enable(o, &sphx_ctx::fmap, o.c->prm, cfg, o.M);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_field_map_disable(sphx_batch *b)
{
    SPHX_TRY
    sampler_disable(batch_owner(b), &sphx_ctx::fmap);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_field_map_reset(sphx_batch *b)
{
    SPHX_TRY
    sampler_reset(batch_owner(b), &sphx_ctx::fmap);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_field_map_sample(sphx_batch *b)
{
    SPHX_TRY
    sampler_sample(batch_owner(b), &sphx_ctx::fmap, launch_field_map);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_field_map_read(sphx_batch *b, int capacity, int *nx, int *ny, double *count, double *sum_w, double *sum_ux,
                                          double *sum_uy, double *sum_ux2, double *sum_uy2, int64_t *n_samples, double *t_first,
                                          double *t_last)
{
    SPHX_TRY
    field_read(batch_owner(b), capacity, nx, ny, count, sum_w, sum_ux, sum_uy, sum_ux2, sum_uy2, n_samples, t_first, t_last);
    return SPHX_OK;
    SPHX_CATCH
}

// ---- point probes (include/sphx.h section 2i) ----

SPHX_EXPORT int sphx_batch_probes_enable(sphx_batch *b, const sphx_probes_config *cfg)
{
    SPHX_TRY
    const Owner o = batch_owner(b);
    sampler_enable(o, &sphx_ctx::probes, o.c->prm, cfg, o.M);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_probes_disable(sphx_batch *b)
{
    SPHX_TRY
    sampler_disable(batch_owner(b), &sphx_ctx::probes);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_probes_sample(sphx_batch *b)
{
    SPHX_TRY
    sampler_sample(batch_owner(b), &sphx_ctx::probes, launch_probes);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_probes_read(sphx_batch *b, int capacity, double *times, double *values, int *n_points, int *n_records,
                                       int64_t *n_dropped, int drain)
{
    SPHX_TRY
    const Owner o = batch_owner(b);
    Probes &p = sampler_settled(o, &sphx_ctx::probes);  // (the records of everything enqueued)
    p.read(o.st, capacity, times, values, n_records, n_dropped, drain != 0);
    if (n_points) *n_points = p.cfg.n_points;
    return SPHX_OK;
    SPHX_CATCH
}

// ---- particle tracers (include/sphx.h section 2q) ----

SPHX_EXPORT int sphx_batch_tracers_enable(sphx_batch *b, const sphx_tracers_config *cfg)
{
    SPHX_TRY
    const Owner o = batch_owner(b);
    sampler_enable(o, &sphx_ctx::tracers, o.c->nf, o.c->nt, cfg, o.M);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_tracers_disable(sphx_batch *b)
{
    SPHX_TRY
    sampler_disable(batch_owner(b), &sphx_ctx::tracers);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_tracers_sample(sphx_batch *b)
{
    SPHX_TRY
    sampler_sample(batch_owner(b), &sphx_ctx::tracers, launch_tracers);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_tracers_read(sphx_batch *b, int capacity, double *times, double *values, int32_t *ids, int *n_tracers,
                                        int *n_records, int64_t *n_dropped, int64_t *n_missing, int drain)
{
    SPHX_TRY
    tracers_read(batch_owner(b), capacity, times, values, ids, n_tracers, n_records, n_dropped, n_missing, drain);
    return SPHX_OK;
    SPHX_CATCH
}

// ---- profile series (include/sphx.h section 2k) ----

SPHX_EXPORT int sphx_batch_profile_series_enable(sphx_batch *b, const sphx_profile_series_config *cfg)
{
    SPHX_TRY
    const Owner o = batch_owner(b);
    sampler_enable(o, &sphx_ctx::pseries, o.c->prm, cfg, o.M);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_profile_series_disable(sphx_batch *b)
{
    SPHX_TRY
    sampler_disable(batch_owner(b), &sphx_ctx::pseries);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_profile_series_sample(sphx_batch *b)
{
    SPHX_TRY
    sampler_sample(batch_owner(b), &sphx_ctx::pseries, launch_profile_series);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_profile_series_read(sphx_batch *b, int capacity, double *times, double *records, int *n_bins, int *n_bands,
                                               int *n_records, int64_t *n_dropped, int drain)
{
    SPHX_TRY
    series_read(batch_owner(b), capacity, times, records, n_bins, n_bands, n_records, n_dropped, drain);
    return SPHX_OK;
    SPHX_CATCH
}

// ---- pair statistics (include/sphx.h section 2m) ----

SPHX_EXPORT int sphx_batch_pair_dist_enable(sphx_batch *b, const sphx_pair_dist_config *cfg)
{
    SPHX_TRY
    const Owner o = batch_owner(b);
    sampler_enable(o, &sphx_ctx::pairs, o.c->prm, cfg, o.has_walls);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_pair_dist_disable(sphx_batch *b)
{
    SPHX_TRY
    sampler_disable(batch_owner(b), &sphx_ctx::pairs);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_pair_dist_reset(sphx_batch *b)
{
    SPHX_TRY
    sampler_reset(batch_owner(b), &sphx_ctx::pairs);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_pair_dist_sample(sphx_batch *b)
{
    SPHX_TRY
    sampler_sample(batch_owner(b), &sphx_ctx::pairs, launch_pair_dist);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_pair_dist_read(sphx_batch *b, int band, int capacity, int *n_bins, int64_t *ff, int64_t *fw, int64_t *centres,
                                          double *r2_min, int64_t *n_samples, double *t_first, double *t_last)
{
    SPHX_TRY
    pair_dist_read(batch_owner(b), band, capacity, n_bins, ff, fw, centres, r2_min, n_samples, t_first, t_last);
    return SPHX_OK;
    SPHX_CATCH
}

// ---- gradient statistics (include/sphx.h section 2o) ----

SPHX_EXPORT int sphx_batch_grad_stats_enable(sphx_batch *b, const sphx_grad_stats_config *cfg)
{
    SPHX_TRY
    const Owner o = batch_owner(b);
    sampler_enable(o, &sphx_ctx::grads, o.c->prm, cfg, o.has_walls);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_grad_stats_disable(sphx_batch *b)
{
    SPHX_TRY
    sampler_disable(batch_owner(b), &sphx_ctx::grads);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_grad_stats_reset(sphx_batch *b)
{
    SPHX_TRY
    sampler_reset(batch_owner(b), &sphx_ctx::grads);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_grad_stats_sample(sphx_batch *b)
{
    SPHX_TRY
    sampler_sample(batch_owner(b), &sphx_ctx::grads, launch_grad_stats);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_grad_stats_read(sphx_batch *b, int band, int capacity, int *n_bins, double *sums, int64_t *n_samples,
                                           double *t_first, double *t_last)
{
    SPHX_TRY
    grad_stats_read(batch_owner(b), band, capacity, n_bins, sums, n_samples, t_first, t_last);
    return SPHX_OK;
    SPHX_CATCH
}

// ---- density statistics (include/sphx.h section 2s) ----

SPHX_EXPORT int sphx_batch_dens_stats_enable(sphx_batch *b, const sphx_dens_stats_config *cfg)
{
    SPHX_TRY
    const Owner o = batch_owner(b);
    sampler_enable(o, &sphx_ctx::dens, o.c->prm, cfg);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_dens_stats_disable(sphx_batch *b)
{
    SPHX_TRY
    sampler_disable(batch_owner(b), &sphx_ctx::dens);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_dens_stats_reset(sphx_batch *b)
{
    SPHX_TRY
    sampler_reset(batch_owner(b), &sphx_ctx::dens);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_dens_stats_sample(sphx_batch *b)
{
    SPHX_TRY
    sampler_sample(batch_owner(b), &sphx_ctx::dens, launch_dens_stats);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_dens_stats_read(sphx_batch *b, int member, int band, int capacity, int hist_capacity, int *n_bins, int *n_hist,
                                           double *sums, int64_t *hist, int64_t *below, int64_t *above, int64_t *n_samples, double *t_first,
                                           double *t_last)
{
    SPHX_TRY
    const Owner o = batch_owner(b);
    sampler_of(o, &sphx_ctx::dens, true);
    batch_check_member(b, member);
    dens_stats_read(o, member, band, capacity, hist_capacity, n_bins, n_hist, sums, hist, below, above, n_samples, t_first, t_last);
    return SPHX_OK;
    SPHX_CATCH
}

// ---- mode amplitudes (include/sphx.h section 2u) ----

SPHX_EXPORT int sphx_batch_modes_enable(sphx_batch *b, const sphx_modes_config *cfg)
{
    SPHX_TRY
    const Owner o = batch_owner(b);
    sampler_enable(o, &sphx_ctx::modes, cfg, o.M);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_modes_disable(sphx_batch *b)
{
    SPHX_TRY
    sampler_disable(batch_owner(b), &sphx_ctx::modes);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_modes_sample(sphx_batch *b)
{
    SPHX_TRY
    sampler_sample(batch_owner(b), &sphx_ctx::modes, launch_modes);
    return SPHX_OK;
    SPHX_CATCH
}

SPHX_EXPORT int sphx_batch_modes_read(sphx_batch *b, int capacity, double *times, double *records, int *mx, int *ny, int *n_records,
                                      int64_t *n_dropped, int drain)
{
    SPHX_TRY
    modes_read(batch_owner(b), capacity, times, records, mx, ny, n_records, n_dropped, drain);
    return SPHX_OK;
    SPHX_CATCH
}
