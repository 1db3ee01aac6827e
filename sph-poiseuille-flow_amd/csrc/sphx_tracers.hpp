// sphx_tracers.hpp -- particle tracers of a resident context (include/sphx.h section 2p), of every member of a batch
// (section 2q, k_tracers_b) and of a slab of a ring (section 3a, k_tracers_s): a slot sampler (sphx_slot_sample.hpp) that follows T chosen fluid rows of the caller's numbering
// and appends one record -- {step, t} and T x kTracerFields values -- to a record buffer in device memory.  The one sampler
// that is Lagrangian: the other seven report what passes a bin, a node or a point.
//
// One value set of a tracer is x, y, u_x, u_y of its particle, COPIED from pos and vel of the state the step slot left: what
// sphx_ctx_download returns in that row, x wrapped into the period as the state holds it.  No arithmetic on the values.
//
// Mapping: A SCAN OF THE POPULATION.  The step kernels keep no map from id to slot (and must not grow one for a diagnostic), so
// thread i looks at slot i: it reads s.id[i], looks the id up in index_of[n_fluid] (int32, the tracer's column or -1, built on
// the host at enable, shared by the members of a batch) and on a hit copies the slot's pos and vel -- two 16-byte loads, two
// 16-byte stores -- into column k of the row.  The common case is a miss: 4 bytes of id and 4 bytes of table per particle, both
// coalesced or nearly so (ids of neighbouring slots are neighbours in space, not in number: the table gathers are served from
// L2).  T = 1 and T = n_fluid run the same code.
//
// Bounds.
//  * Slots: i < min(clk->n, a.n_slots).  clk->n is the population; arrays with slack (a slab's: n_slots is its capacity) hold
//    stale ids behind it, which would write a column twice.  a.n_slots, the particle count the host allocated the view for, is a second
//    bound that costs nothing: no word of the clock can send a load past the arrays.
//  * Table: the id is compared as unsigned against n_fluid in front of the table read, so a negative or foreign id reads nothing.
//  * Column: 0 <= k < n_tracers is checked although the host built the table: the store's address depends on it.
//  * Row: `at < capacity` is checked in front of every store; a full buffer stores nothing and counts the record as dropped.
//
// Bounded grid: a grid-stride loop on at most kTracerMaxBlocks = 256 workgroups of kTracerBlock = 1024 threads (the probes'
// cap): a 6 M-particle channel draws no more tickets than a small one, 23 trips of the loop per thread.
//
// Determinism: a column has exactly one writer -- the thread that meets the one slot holding that id -- and what it writes are
// the bits it read.  No floating-point arithmetic, no atomics on values.  Records are bit-identical between runs, between a
// batch member and a standalone context, between replayed and eager slots and whatever the layout: the layout decides WHICH
// thread copies a particle, never what is copied.
//
// The record index: the probes' protocol (sphx_probes.hpp), with the head read by every thread.
//  * every thread reads head->n_records on entry (`at`); a thread that stores addresses its stores with it and tests it against
//    the capacity first, so its read has completed before its stores are issued, hence before its workgroup's barrier; a thread
//    that stores nothing never uses the value;
//  * one thread of the launch writes the head -- thread 0 of the LAST workgroup out -- behind that barrier and behind its own
//    draw of the last ticket: every other workgroup has drawn, hence passed its barrier, hence read.  When the row is not below
//    the capacity the advance touches n_dropped only and n_records reads the same before and after.
// So every tracer of a launch lands in one row, the row the last one out then stamps with {step, t} and counts.  Launches on a
// stream do not overlap and a kernel boundary publishes head and values to the next launch and to the host copy.
//
// Fenced or fence-free?  FENCE-FREE.  last_out_fenced exists for samplers whose last workgroup READS what the others stored
// (partial sums): it needs their plain stores released and acquired.  Here the values are read by no workgroup of the launch.
// The ONE datum that crosses workgroups inside the launch is the count of tracers met, which the stamping thread needs for
// n_missing -- and that count travels IN the ticket: the ticket is a 64-bit word, a workgroup's thread 0 adds
// (1 << 32) + (tracers its workgroup met) with one returning agent-scope atomic, and the thread whose add returns
// gridDim.x - 1 in the high half reads the others' total in the low half of the very value that made it last.  Atomics on one
// address are totally ordered at the coherence point: nothing else has to be visible, so no release, no acquire, no L2
// write-back.  A workgroup's own count is gathered in LDS (one __popcll of a ballot per trip and wave, one LDS add per wave)
// in front of the barrier thread 0 passes before it draws.  The last thread stores the ticket back to zero behind the add
// that told it so; the kernel boundary publishes that too.
//
// n_missing.  Every id of the list must be met in exactly one slot of the population; the stamping thread adds T - met to a
// sticky counter the read reports.  On a context and on a batch member it is always 0: it is the invariant of the id
// bookkeeping (FluidSet::id through the fold-rebin path, the scatter / reorder chain, the in-place dynamic path, a batch's
// realignment).  The tracers are counted as MET whether or not the row had room, so a dropped record still checks it.
//
// A slab of a ring (include/sphx.h section 3a, k_tracers_s = tracers_body<true>).  OWNERSHIP MOVES WITH THE PARTICLE: a slab
// holds the particles it owns and halo copies of its neighbours', the copies under their particles' ids, and a particle
// changes hands at a re-binning (the id lists of message B).  TracerArgs is unchanged -- index_of is the RING's table, the
// same on every rank, n_fluid the ring's count, n_slots the slab's capacity -- and the scan is the one above with one more
// condition for a hit: the slab OWNS the slot, owns(g, pos.x, s.cell[i]), the binned column on a skinned slab, which is what
// sphx_slab_snapshot marks owned and what every other ring sampler sums by.  A halo copy is its owner's to record.  Every
// fluid row has exactly one owner at every step, so every tracked id has exactly one writer in the whole ring: no premise
// about the halo's state is needed, the copies are never read.  What is copied are the bits of pos and vel of S[1-q], x in
// the SLAB'S frame as the state holds it -- the first slab keeps particles it took over from the last one below 0 until they
// are folded, the last slab may hold x >= DL -- which is what sphx_slab_snapshot returns for that id.
//  * n_owned replaces n_missing.  "Not met" is normal on a slab, so the stamping thread does not touch the sticky n_missing;
//    it stores the count of tracers met -- the total that rode in the ticket, fence-free as above -- into n_owned[row], an
//    int64 array beside {step, t}.  The ring's invariant: the slabs' n_owned of a record add up to T.  A particle lost or
//    held twice at a re-binning shows in the record of the very step it happens.
//  * Columns the slab does not own are never written.  The host fills the value buffer with NaN (byte 0xFF) at enable and
//    refills the rows a draining read hands out, on the slab's stream, so a column nobody wrote reads NaN -- a particle's x
//    never does -- and the step loop pays nothing for it.
//  * The dense row costs G times the memory ring-wide; see DESIGN.md section 5 for why it was taken.
//  * Grid: tracer_blocks(capacity), fixed, so a captured step graph outlives a re-binning.  Launched behind k_slab_pack3 and
//    in front of everything of phase 3 (launch_slab_samplers): clk->n and s.cell are those of the layout the step ran in.
#pragma once
#include "../../include/sphx.h"
#include "sphx_slot_sample.hpp"

namespace sphx {

constexpr int kTracerFields = SPHX_TRACER_FIELDS;   // x, y, u_x, u_y
constexpr int kTracerBlock = 1024;
constexpr int kTracerMaxBlocks = 256;               // one workgroup per CU at most: every one of them draws a ticket
constexpr long long kTracerMaxTotal = 1ll << 27;    // doubles (1 GiB) of values of all members together

// the counters of the record buffer; only the last workgroup out of a launch writes them
struct TracerHead {
    long long n_records;        // records in the buffer, filled in step order
    long long n_dropped;        // records that found the buffer full
    long long n_missing;        // sticky: tracers no slot of the population held, summed over the records
    unsigned long long ticket;  // high half: workgroups out, low half: tracers they met (zero between launches)
};

struct TracerArgs {
    const int *index_of;  // [n_fluid] column of the tracer with this id, -1: not tracked; shared by the members of a batch
    double *times;        // [capacity][2]: step, t (of a batch: member 0's, member m's block behind)
    double *values;       // [capacity][n_tracers][kTracerFields]
    TracerHead *head;     // (of a batch: [M])
    double t_from;
    int n_tracers;
    int n_fluid;          // ids are 0 .. n_fluid - 1
    int n_slots;          // slots the view was allocated for, at least the population
    int capacity;
    int every;            // >= 1: in-loop sample, gated on the clock; 0: sample unconditionally
};

// The record of one channel closing the step slot of parity q, on clock clk, by the gridDim.x workgroups of a grid row; s is the
// state the step left (pos, vel and the ids of the layout it is stored in); a's times / values / head are that channel's own.
// Every thread of every workgroup reaches the barrier.
// kSlab: the channel is a slab of a ring -- of the slots it holds only those it owns (owns() on grid g) are copied and
// counted, and the count goes into n_owned[row] instead of n_missing (k_tracers_s).
template <bool kSlab = false>
__device__ __forceinline__ void tracers_body(const Clock *clk, int q, const FluidSet &s, const TracerArgs &a, const Grid *g = nullptr,
                                             long long *n_owned = nullptr)
{
    if (!sample_due(clk, q, a.every, a.t_from)) return;
    __shared__ unsigned s_met;
    if (threadIdx.x == 0) s_met = 0u;
    __syncthreads();
    TracerHead *h = a.head;
    const long long at = h->n_records;  // requested now, used by the stores (see the header)
    const bool room = at < (long long)a.capacity;
    const int n = min(clk->n, a.n_slots);
    const unsigned nf = (unsigned)a.n_fluid;
    const int stride = (int)gridDim.x * kTracerBlock;
    unsigned met = 0u;  // (wave-uniform)
    // whole trips only, so that every lane of a wave reaches the ballot: trips = ceil(n / stride) for all threads alike
    const int first = (int)blockIdx.x * kTracerBlock + (int)threadIdx.x;
    for (long long base = 0; base < (long long)n; base += stride) {
        const long long i = base + first;
        int k = -1;
        if (i < (long long)n) {
            const unsigned id = (unsigned)s.id[i];
            if (id < nf) k = a.index_of[id];
        }
        bool hit = k >= 0 && k < a.n_tracers;
        if constexpr (kSlab) hit = hit && owns(*g, s.pos[i].x, s.cell[i]);  // (a halo copy: its owner records it)
        if (hit && room) {
            const double2 p = s.pos[i], v = s.vel[i];
            double2 *out = reinterpret_cast<double2 *>(a.values + ((size_t)at * (size_t)a.n_tracers + (size_t)k) * kTracerFields);
            out[0] = p;
            out[1] = v;
        }
        met += (unsigned)__popcll(__ballot(hit));
    }
    if (((int)threadIdx.x & 63) == 0 && met) atomicAdd(&s_met, met);  // (LDS)
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned long long total = s_met;
    if (gridDim.x > 1) {
        const unsigned long long drawn =
            __hip_atomic_fetch_add(&h->ticket, (1ull << 32) + total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((drawn >> 32) != (unsigned long long)gridDim.x - 1ull) return;
        total += drawn & 0xffffffffull;
        __hip_atomic_store(&h->ticket, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // {step, t} and the counters, by the one thread of the launch that advances them: plain vector stores
    if (room) {
        *reinterpret_cast<double2 *>(a.times + (size_t)at * 2) = make_double2((double)clk->step, clk->t);
        h->n_records = at + 1;
    } else {
        h->n_dropped += 1;
    }
    if constexpr (kSlab) {
        if (room) n_owned[at] = (long long)total;
    } else {
        const long long missing = (long long)a.n_tracers - (long long)total;
        if (missing != 0) h->n_missing += missing;
    }
}

// q: parity of the step slot this launch closes
__global__ __launch_bounds__(kTracerBlock) void k_tracers(const Clock *clk, int q, FluidSet s, TracerArgs a)
{
    tracers_body(clk, q, s, a);
}

// batch (sphx_batch_tracers_*): member m = blockIdx.y scans its own state (member_set of the view, which is member 0's) on its
// own clock into its own block of records (m * capacity rows) and its own head; the table is shared.  What is copied does not
// depend on which thread copies it: a member's records are bit for bit a standalone context's.  A member whose gate is closed
// returns before it touches its head or its records.
__global__ __launch_bounds__(kTracerBlock) void k_tracers_b(Members mb, int q, FluidSet s, TracerArgs a)
{
    const int m = (int)blockIdx.y;
    a.times += (size_t)m * (size_t)a.capacity * 2;
    a.values += (size_t)m * (size_t)a.capacity * (size_t)a.n_tracers * kTracerFields;
    a.head += m;
    tracers_body(mb.clk + m, q, member_set(mb, m, s), a);
}

// slab of a ring (sphx_slab_tracers_*): the tracers this slab OWNS at this step, out of the ring's list, into the slab's own
// times / values / n_owned / head; the columns it does not own keep the host's NaN fill.  g: the slab's grid (ownership by the
// binned column); a.n_slots: the slab's capacity; n_owned: [capacity] tracers met per record.
__global__ __launch_bounds__(kTracerBlock) void k_tracers_s(const Clock *clk, int q, FluidSet s, TracerArgs a, Grid g, long long *n_owned)
{
    tracers_body<true>(clk, q, s, a, &g, n_owned);
}

}  // namespace sphx
