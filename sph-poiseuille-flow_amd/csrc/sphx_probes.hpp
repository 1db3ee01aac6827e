// sphx_probes.hpp -- point probes of a resident context (include/sphx.h section 2h), of every member of a batch (section
// 2i, k_point_probes_b) and of a slab of a ring (section 3a, k_point_probes_s): a slot sampler (sphx_slot_sample.hpp) that interpolates the state the step left onto P fixed points
// and appends one record -- {step, t} and P x kProbeFields values -- to a record buffer in device memory.  The one sampler
// whose signal is resolved in space AND time.
//
// One sample at a point is the field map's sample at a node (sphx_field_map.hpp) plus a density: Shepard sums with the cubic
// spline of spline_W over every particle within 2h (minimum image in x, no lower cut), S0 = sum W, S1 = sum W u_x,
// S2 = sum W u_y, and Sm = sum m_j W_j over the FLUID particles alone -- the summation density from the fluid; within 2h of
// a wall it lacks the wall's share.  with_walls adds the wall particles to S0, S1, S2 with their wall velocity, as the map does.
//
// Why the 3 x 3 sweep suffices: the argument of sphx_field_map.hpp, word for word, with "point" for "node".  A probe finds
// the cell its own coordinates fall into (cell_of) and visits the three cell columns around it through neighbour_column (a
// period of one or two columns is visited once per distinct column and the minimum-image fold picks the nearest image).  A
// particle within 2h of the point was binned at most 2h + drift from it; the cells are 2h + skin wide, the clock stops or
// re-bins at a drift of skin / 2, so that binning position lies in the point's cell or one next to it.  Walls do not move.
//
// Mapping: ONE WAVE PER PROBE.  k_field_map gives a node to a thread, which walks ~150 candidates four at a time: ~36
// dependent load trips, and on a small channel the wave is alone on its SIMD, so the sample IS that chain.  A handful of
// probes is the worst case of that mapping.  Here lane l of the probe's wave takes the candidates lo + l, lo + l + 64, ... of a
// column's run start[base + cylo] .. start[base + cyhi + 1] -- three cells, about 48 particles on a channel at rest, so a
// column is one trip.  The chain of dependent loads is: the clock and the point (wave-uniform, scalar loads, one trip), the
// range words of the three columns of the fluid AND of the walls (scalar loads, requested together), the first candidate of
// every column -- pos, vel, mass of the fluid, pos and {Vol, vx, vy} of the walls -- requested together before the first one is
// used.  Three trips where a node has ~36; a run longer than 64 adds one trip per further 64 (dense columns only).  The
// record index (below) is requested with the clock and used at the end.
//
// Determinism: a lane adds its own candidates in column and slot order, fluid first, then walls; the four sums are reduced
// across the wave with the fixed __shfl_xor butterfly of k_step_history, which leaves the same bits in every lane; lane 0
// writes the probe's four values with plain stores.  No floating-point atomics.  The order of the adds depends on the
// particle layout only: two identical runs give identical bits, another layout (re-binning phase, host chunking) changes the
// summation order only.  A member of a batch runs the same body on the same workgroups: bit for bit a standalone context's.
//
// The record index.  Every wave that owns a probe reads head->n_records on entry and writes its values into that row when the
// row is below capacity.  Nobody advances the counter before every workgroup has read it:
//  * one thread of the launch writes the head -- thread 0 of the LAST workgroup out -- and it does so behind the final barrier of
//    its workgroup (last_out_fenced's, or the plain __syncthreads of a launch of one workgroup);
//  * a wave's read of n_records has COMPLETED before its workgroup passes that barrier when the row is below capacity: lane 0's
//    stores are addressed with it, they are issued before the barrier (last_out_fenced also drains them, vmcnt(0)), and a store
//    cannot be issued before the load that forms its address has returned.  When the row is NOT below capacity the advance only
//    touches n_dropped, and n_records reads the same before and after;
//  * with several workgroups, thread 0 draws the workgroup's ticket behind that barrier, and the last workgroup out is the one
//    that draws the last ticket: every other workgroup has drawn, hence passed its barrier, hence read.
// So every probe of a launch lands in one row, the row the last one out then stamps with {step, t} and counts.  Launches on a
// stream do not overlap, and a kernel boundary publishes the head to the next launch.  The values of the other workgroups are
// not read by the last one; the release / acquire of last_out_fenced costs a few workgroups a fence on the steps sampled.
// Up to kProbeBlock / 64 probes fit one workgroup and need no ticket.
//
// A slab of a ring (include/sphx.h section 3a, k_point_probes_s = point_probes_body<true>).  The POINTS are divided among the
// slabs as the map's node columns are (probe_owner, sphx_samplers.hpp: rank r owns edge(r) <= x < edge(r + 1), edge(r) the
// left edge of its first cell column, decided once on the host); ProbeArgs is unchanged and holds the owned subset, compacted
// at enable, with the slab's own times / values / head.  A slab computes the complete sample of each probe it owns -- S0, S1,
// S2 and Sm -- in its own open window (Grid::periodic = 0, half_DL = +inf: min_image is a no-op and the one probe_add stays),
// with the sweep centred on the point's cell column CLAMPED into the owned columns [own_c0, own_c1), the clamp of
// field_map_body<true>: it reads the columns own - 1 .. own + 1 only, where the halo copies carry the finished step's state
// (DESIGN.md section 5).  Why the map's argument carries over from a node to a point:
//  * no shift: the point is x as the host folded it into [0, DL), and its owner's owned range [own_lo, own_hi) = [edge(r),
//    edge(r + 1)) contains that very number -- the slab keeps its owned particles at their global x, the first slab holds the
//    last slab's particles at x - DL and the last slab the first slab's at x + DL, so cell_of on the folded x finds the right
//    column and a probe at x = 0 (also what x = DL and -DL fold to) or within rounding of DL needs no minimum image;
//  * a point strictly inside the owned range falls into an owned column and the clamp does nothing;
//  * a point ON a cut is x = edge(r) = own_lo exactly, owned by rank r.  cell_of computes (x - x0) * inv_csx, which may round
//    to just below own_c0: the clamp moves the centre up by one column, as for a node column that falls on a cut.  A particle
//    within 2h of the point was binned within 2h + drift of the edge, i.e. in the outermost owned column or in the first halo
//    column beside it -- both among the clamped centre's three, because a column is 2h + skin wide and the ring re-bins at a
//    drift of skin / 2.  The same holds at own_hi for a point within rounding of DL in the last slab (x < DL after the fold,
//    (x - x0) * inv_csx may round up to own_c1): the spare half of the skin is many orders of magnitude more than the rounding;
//  * a point within 2h of a cut but off it: its cell is the outermost owned column, the three columns include the first halo
//    column, and the halo is four columns deep.
// Sm needs the MASS of a halo copy -- the first sampled value that does.  It is there: s.mass of the view is the layout array
// fmass_[l] (sphx_ctx::view, sphx_resident.hip:267-270), in slot order with S[1-q].pos / .vel.  Every image inside the window
// enters it with its particle's mass at creation (slab_setup, sphx_resident.hip:2162-2169, 2189).  At a re-binning the owner
// sends m = sn.mass[i] with the state (k_slab_pack3, sphx_kernels.hpp:3628, 3647-3654), the receiver stores it beside the
// kept particles' (kmass, k_slab_unpack3, sphx_kernels.hpp:3639, 3732) and the re-binning chain reorders kmass into the new
// layout's mass (slab_phase3, sphx_resident.hip:2786-2789).  On a frozen step message A carries 0.0 in the mass block
// (sphx_kernels.hpp:3597-3598) and the receiver writes pos, vel and drho of the fixed slots only (sphx_kernels.hpp:3705-3710):
// the mass of a halo copy is not touched between two re-binnings, and a particle's mass never changes.  The sampler runs in
// front of phase 3, so on a re-binning step it still reads the layout the step ran in.  Fluid candidates read s.mass[j], wall
// candidates add zero, on a slab as on a context; nothing assumes a uniform mass.
// A slab that owns no probe launches one workgroup all the same (n_points = 0): no wave owns a probe, thread 0 passes the plain
// barrier, stamps {step, t} and counts the record, as a block of zero node columns still counts its sample -- every slab's
// series has the length of its neighbours'.
#pragma once
#include "../../include/sphx.h"
#include "sphx_slot_sample.hpp"
#include "sphx_history.hpp"

namespace sphx {

constexpr int kProbeFields = SPHX_PROBE_FIELDS;     // weight, u_x, u_y, rho
constexpr int kProbeMaxPoints = SPHX_PROBE_MAX_POINTS;
constexpr int kProbeBlock = 1024;                   // 16 waves = 16 probes a workgroup: at most 256 workgroups draw a ticket
constexpr int kProbeWaves = kProbeBlock / 64;
constexpr long long kProbeMaxTotal = 1ll << 27;     // doubles (1 GiB) of values of all members together

using ProbeHead = HistoryHead;  // n_records, n_dropped, ticket: the counters of a record buffer

struct ProbeArgs {
    const double2 *points;  // [n_points] (x folded into [0, DL), y), shared by the members of a batch
    double *times;          // [capacity][2]: step, t (of a batch: member 0's, member m's block behind)
    double *values;         // [capacity][n_points][kProbeFields]
    ProbeHead *head;        // (of a batch: [M])
    double dp2;             // dp^2: weight = S0 dp^2
    double t_from;
    int n_points;
    int capacity;
    int every;              // >= 1: in-loop sample, gated on the clock; 0: sample unconditionally
    int with_walls;         // 1: the wall particles enter S0, S1, S2 with their wall velocity
};

struct ProbeSums {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, sm = 0.0;  // sum W, sum W u_x, sum W u_y, sum m W
};

struct ProbeCand {
    double2 p, v;
    double m;  // (a wall particle: 0 -- adding W * 0 changes no bit of sm)
};

// the runs of the three cell columns around (cx, cy), rows cylo .. cyhi; a column that does not exist (neighbour_column) is empty
struct ProbeRuns {
    int lo[3], hi[3];
};

__device__ __forceinline__ ProbeRuns probe_runs(const Grid &g, const int *__restrict__ start, int cx, int cylo, int cyhi)
{
    ProbeRuns r;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        int col;
        const bool ok = neighbour_column(g, cx, u - 1, col);
        const int base = (ok ? col : 0) * g.ncy;  // (a valid address either way: the words are requested without a branch)
        const int lo = start[base + cylo], hi = start[base + cyhi + 1];
        r.lo[u] = ok ? lo : 0;
        r.hi[u] = ok ? hi : 0;
    }
    return r;
}

// slot k of a run, or the run's last one beyond it (slot 0 of the array for an empty run: always in bounds, never added)
__device__ __forceinline__ int probe_slot(const ProbeRuns &r, int u, int k) { return max(min(k, r.hi[u] - 1), 0); }

__device__ __forceinline__ void probe_add(const Grid &g, const KernelConst &kc, double xp, double yp, const ProbeCand &c, ProbeSums &S)
{
    const double dx = min_image(g, xp - c.p.x), dy = yp - c.p.y;
    const double r2 = dx * dx + dy * dy;
    if (r2 < kc.rcut2) {
        const double W = spline_W(kc, sqrt(r2));
        S.s0 += W;
        S.s1 += W * c.v.x;
        S.s2 += W * c.v.y;
        S.sm += W * c.m;
    }
}

// lane `lane`'s candidates of the runs r -- first[u] is its first one of column u, already requested -- added in column and slot order
template <typename Fetch>
__device__ __forceinline__ void probe_columns(const Grid &g, const KernelConst &kc, const ProbeRuns &r, int lane, double xp, double yp,
                                              const ProbeCand (&first)[3], ProbeSums &S, Fetch &&fetch)
{
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        int k = r.lo[u] + lane;
        if (k < r.hi[u]) probe_add(g, kc, xp, yp, first[u], S);
        for (k += 64; k < r.hi[u]; k += 64) probe_add(g, kc, xp, yp, fetch(k), S);  // (a run longer than a wave)
    }
}

// The record of one channel closing the step slot of parity q, on clock clk, by the gridDim.x workgroups of a grid row; s is the
// state the step left (pos, vel, mass and the cell ranges of the layout it is stored in); a's times / values / head are that
// channel's own.  Every thread of every workgroup reaches the final barrier.
// kSlab: the channel is a slab of a ring -- a.points, a.n_points and the values are those of the probes the slab OWNS (possibly
// none: the one workgroup still stamps and counts the record), and the sweep is centred on a column the slab owns.
template <bool kSlab = false>
__device__ __forceinline__ void point_probes_body(const Clock *clk, int q, const Grid &g, const Phys &ph, const FluidSet &s,
                                                  const Walls &w, const ProbeArgs &a)
{
    if (!sample_due(clk, q, a.every, a.t_from)) return;
    __shared__ int s_last;
    const int lane = (int)threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);  // (wave-uniform: what follows is scalar work)
    const int probe = (int)blockIdx.x * kProbeWaves + wave;
    ProbeHead *h = a.head;
    if (probe < a.n_points) {
        const long long at = h->n_records;  // requested now, used at the end (see the header)
        const double2 pt = a.points[probe];
        const double xp = pt.x, yp = pt.y;
        int cx, cy;
        cell_of(g, xp, yp, cx, cy);
        if constexpr (kSlab) cx = min(max(cx, g.own_c0), g.own_c1 - 1);
        cx = __builtin_amdgcn_readfirstlane(cx);
        cy = __builtin_amdgcn_readfirstlane(cy);
        const int cylo = max(cy - 1, 0), cyhi = min(cy + 1, g.ncy - 1);
        const bool walls = a.with_walls != 0;
        // the range words of fluid and walls together ...
        const ProbeRuns rf = probe_runs(g, s.start, cx, cylo, cyhi);
        ProbeRuns rw{};
        if (walls) rw = probe_runs(g, w.start, cx, cylo, cyhi);
        // ... and a lane's first candidate of every column, before the first one is used
        auto fluid = [&](int j) { return ProbeCand{s.pos[j], s.vel[j], s.mass[j]}; };
        auto wall = [&](int j) {
            const double4 wj = w.a[j];  // {Vol, vx, vy, 0}
            return ProbeCand{w.pos[j], make_double2(wj.y, wj.z), 0.0};
        };
        ProbeCand cf[3], cw[3] = {};
#pragma unroll
        for (int u = 0; u < 3; ++u) cf[u] = fluid(probe_slot(rf, u, rf.lo[u] + lane));
        if (walls) {
#pragma unroll
            for (int u = 0; u < 3; ++u) cw[u] = wall(probe_slot(rw, u, rw.lo[u] + lane));
        }
        ProbeSums S;
        probe_columns(g, ph.kc, rf, lane, xp, yp, cf, S, fluid);
        if (walls) probe_columns(g, ph.kc, rw, lane, xp, yp, cw, S, wall);
        double s0 = S.s0, s1 = S.s1, s2 = S.s2, sm = S.sm;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            s0 += __shfl_xor(s0, off);
            s1 += __shfl_xor(s1, off);
            s2 += __shfl_xor(s2, off);
            sm += __shfl_xor(sm, off);
        }
        if (lane == 0 && at < (long long)a.capacity) {
            const bool any = s0 > 0.0;
            const double none = __builtin_nan("");
            double2 *out = reinterpret_cast<double2 *>(a.values + ((size_t)at * (size_t)a.n_points + (size_t)probe) * kProbeFields);
            out[0] = make_double2(any ? s0 * a.dp2 : 0.0, any ? s1 / s0 : none);
            out[1] = make_double2(any ? s2 / s0 : none, any ? sm : 0.0);
        }
    }
    if (gridDim.x > 1) {
        last_out_fenced(&h->ticket, s_last);
        if (!s_last) return;
    } else {
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    // {step, t} and the counters, by the one thread of the launch that advances them: plain vector stores
    const long long at = h->n_records;
    if (at < (long long)a.capacity) {
        *reinterpret_cast<double2 *>(a.times + (size_t)at * 2) = make_double2((double)clk->step, clk->t);
        h->n_records = at + 1;
    } else {
        h->n_dropped += 1;
    }
    if (gridDim.x > 1) __hip_atomic_store(&h->ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// q: parity of the step slot this launch closes
__global__ __launch_bounds__(kProbeBlock) void k_point_probes(const Clock *clk, int q, Grid g, Phys ph, FluidSet s, Walls w, ProbeArgs a)
{
    point_probes_body(clk, q, g, ph, s, w, a);
}

// batch (sphx_batch_probes_*): member m = blockIdx.y samples its own state (member_set of the view, which is member 0's) on its
// own clock and parameters into its own block of records (m * capacity rows) and its own head; Grid, Walls and the points are
// shared.  gridDim.x is the workgroup count of a context with these points, a probe is owned by the same wave of the same
// workgroup of the row and its lanes add the same candidates in the same order: a member's records are bit for bit a
// standalone context's.  A member whose gate is closed returns before it touches its head or its records.
__global__ __launch_bounds__(kProbeBlock) void k_point_probes_b(Members mb, int q, Grid g, FluidSet s, Walls w, ProbeArgs a)
{
    const int m = (int)blockIdx.y;
    const Phys ph = mb.ph[m];
    a.times += (size_t)m * (size_t)a.capacity * 2;
    a.values += (size_t)m * (size_t)a.capacity * (size_t)a.n_points * kProbeFields;
    a.head += m;
    point_probes_body(mb.clk + m, q, g, ph, member_set(mb, m, s), w, a);
}

// slab of a ring (sphx_slab_probes_*): the complete sample -- S0, S1, S2 and Sm -- of every probe this slab owns (the host
// compacted the owned subset at enable, probe_owner in sphx_samplers.hpp), from the particles it owns and from its halo copies,
// into the slab's own times / values / head.  Launched behind k_slab_pack3 and in front of everything of phase 3
// (launch_slab_samplers): s is S[1-q] with the masses and the cell ranges of the layout the step ran in.  gridDim.x is fixed at
// enable from the owned count, at least 1.
__global__ __launch_bounds__(kProbeBlock) void k_point_probes_s(const Clock *clk, int q, Grid g, Phys ph, FluidSet s, Walls w, ProbeArgs a)
{
    point_probes_body<true>(clk, q, g, ph, s, w, a);
}

}  // namespace sphx
