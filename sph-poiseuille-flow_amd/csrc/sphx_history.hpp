// sphx_history.hpp -- the step history of a resident context (include/sphx.h section 2d), of every member of a batch
// (section 2f, k_step_history_b) and of a slab of a ring (section 3a, k_step_history_s): a slot sampler
// (sphx_slot_sample.hpp) that reduces the state the step left to one record of kHistoryFields doubles -- step, t, dt, vmax of the device clock, the wall shear of SPH_Poiseuille.m:281-283, the kinetic
// energy and the bulk velocity -- and appends it to a record buffer in device memory.
//
// The wall-shear term is k_wall_shear's, term for term (sphx_kernels.hpp; kept as a copy here so that the monitor's kernel
// stays what it is): the wall cells around the cell a particle was binned into, new pos / vel, Vol / B of the step just
// finished.  Where those records are is the launch's business (launch_history, sphx_samplers.hpp): the buffers of the finished step's
// parity, read through src_of when the slot re-binned -- known at capture time on the static schedule, Clock::fresh on a
// dynamic one.
//
// Determinism: no floating-point atomics.  A workgroup takes a contiguous run of slots, reduces inside the wave with
// shuffles and across its waves in LDS (wave order), and leaves four partial sums; the last workgroup out
// (last_out_fenced) adds the partials in index order and writes the record.  Two identical
// runs give identical bits; another layout of the particles (re-binning phase, host chunking) changes the summation order
// only.  A channel small enough for one workgroup finishes without partials and ticket.
#pragma once
#include "../../include/sphx.h"
#include "sphx_slot_sample.hpp"

namespace sphx {

constexpr int kHistoryFields = SPHX_HISTORY_FIELDS;  // step, t, dt, vmax, tau_bottom, tau_top, kinetic_energy, u_bulk
constexpr int kHistorySums = 4;                      // wall force bottom / top, kinetic energy, sum u_x
constexpr int kHistoryBlock = 512;
constexpr int kHistoryMaxBlocks = 256;               // one workgroup per CU at most: every one of them draws a ticket
constexpr int kHistoryPerThread = 4;                 // particles a thread takes before another workgroup is added: up to
                                                     // 2 048 particles ONE workgroup writes the record by itself
constexpr int kHistoryMaxCapacity = 1 << 22;         // records (256 MB) of one channel
constexpr long long kHistoryMaxTotal = 1ll << 24;    // records (1 GiB) of all members of a batch together

// the counters of the record buffer, in a block of their own (Clock must not grow, see sphx_kernels.hpp); only the last
// workgroup out of a launch touches them
struct HistoryHead {
    long long n_records;  // records in the buffer, filled in step order
    long long n_dropped;  // records that found the buffer full
    int ticket;           // last workgroup out (zero between launches)
    int pad;
};

enum HistorySrc : int {
    kHistoryInPlace = 0,   // Vol / B of slot i are at i
    kHistorySrcOf = 1,     // the slot re-binned: at src_of[i]
    kHistoryByClock = 2,   // dynamic contexts: at src_of[i] when the step ended with a re-binning (Clock::fresh)
};

struct HistoryArgs {
    double *records;       // [capacity][kHistoryFields]
    double *part;          // [kHistoryMaxBlocks][kHistorySums] per-workgroup partial sums
    HistoryHead *head;
    double t_from;
    int capacity;
    int every;             // >= 1
    int src;               // HistorySrc
};

// one fluid particle's contribution to the wall force sums: sph_physics_mex.c:1713-1742 as k_wall_shear evaluates it
// (kSlab: the caller has already asked owns() -- a skinned slab owns by the binned column, not by position)
template <bool kSlab = false>
__device__ __forceinline__ void history_wall_terms(const Grid &g, const Phys &ph, const FluidSet &s, const FluidTmp &t,
                                                   const Walls &w, int i, bool use_src, double2 p, double2 v, double &fb,
                                                   double &ft)
{
    const double xi = p.x, yi = p.y;
    int cx, cy;
    binned_cell(g, s, i, cx, cy);
    if constexpr (kSlab) {
        if (!w.row_any[cy]) return;
    } else {
        if (!(w.row_any[cy] && xi >= g.own_lo && xi < g.own_hi)) return;
    }
    const int o = use_src ? t.src_of[i] : i;
    const double Voli = t.a[o].x;
    const double4 Bo = t.B[o];
    const double b11 = Bo.x, b12 = Bo.y, b21 = Bo.z, b22 = Bo.w;
    const double vxi = v.x;
    sweep<1>(g, w.start, cx, cy, 0, [&](int k) {
        const double2 pj = w.pos[k];
        const double dx = min_image(g, xi - pj.x), dy = yi - pj.y;
        const double r2 = dx * dx + dy * dy;
        if (r2 > kR2Min && r2 < ph.kc.rcut2) {
            const double4 wj = w.a[k];
            const double r = sqrt(r2);
            const double ex = dx / r, ey = dy / r;
            const double eBe = ex * (b11 * ex + b12 * ey) + ey * (b21 * ex + b22 * ey);
            const double f = 4.0 * ph.mu * eBe * spline_dW(ph.kc, r) * wj.x * (vxi - wj.y) / (r + 0.01 * ph.kc.h) * Voli;
            const double yj = pj.y;
            // (selects, not branches around the adds: the sums stay in registers -- k_wall_shear's if / else if puts them
            //  in scratch; adding 0.0 changes no bit of a sum)
            const bool bottom = yj <= 0.0;
            fb += bottom ? f : 0.0;
            ft += !bottom && yj >= ph.DH ? f : 0.0;
        }
    });
}

// The record of one channel closing the step slot of parity q, on clock clk, shared by the gridDim.x workgroups of a grid row;
// s is the state the step left, t holds its Vol / B; a's records / part / head are that channel's own.
// kSlab: the channel is a slab of a ring -- of the clk->n particles it holds only those it owns (owns()) enter the sums, and
// u_bulk is the slab's sum of u_x over the n_bulk fluid particles of the WHOLE channel: the four sums are additive partials,
// the ring's record is the sum over its slabs.
template <bool kSlab = false>
__device__ __forceinline__ void step_history_body(const Clock *clk, int q, const Grid &g, const Phys &ph, const FluidSet &s,
                                                  const FluidTmp &t, const Walls &w, const HistoryArgs &a, int n_bulk = 0)
{
    if (!slot_due(clk, q, a.every, a.t_from)) return;
    const int n = clk->n;
    const bool use_src = a.src == kHistoryByClock ? clk->fresh != 0 : a.src == kHistorySrcOf;
    const int chunk = (n + (int)gridDim.x - 1) / (int)gridDim.x;  // a contiguous run of slots per workgroup
    const int i0 = (int)blockIdx.x * chunk;
    const int i1 = min(n, i0 + chunk);
    double fb = 0.0, ft = 0.0, ke = 0.0, su = 0.0;  // wall force bottom, top; kinetic energy; sum u_x
    for (int i = i0 + (int)threadIdx.x; i < i1; i += kHistoryBlock) {
        const double2 p = s.pos[i], v = s.vel[i];
        if constexpr (kSlab) {
            if (!owns(g, p.x, g.own_by_cell ? s.cell[i] : 0)) continue;  // (a halo copy: its owner sums it)
        }
        ke += 0.5 * s.mass[i] * (v.x * v.x + v.y * v.y);
        su += v.x;
        history_wall_terms<kSlab>(g, ph, s, t, w, i, use_src, p, v, fb, ft);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        fb += __shfl_xor(fb, off);
        ft += __shfl_xor(ft, off);
        ke += __shfl_xor(ke, off);
        su += __shfl_xor(su, off);
    }
    constexpr int kWaves = kHistoryBlock / 64;
    __shared__ double s_wave[kHistorySums][kWaves];
    __shared__ double s_tot[kHistorySums];
    __shared__ int s_last;
    if ((threadIdx.x & 63) == 0) {
        const int wv = threadIdx.x >> 6;
        s_wave[0][wv] = fb; s_wave[1][wv] = ft; s_wave[2][wv] = ke; s_wave[3][wv] = su;
    }
    __syncthreads();
    // thread f adds field f: the waves of this workgroup in wave order, then (several workgroups) the partials in index order
    double tot = 0.0;
    if (threadIdx.x < kHistorySums)
        for (int k = 0; k < kWaves; ++k) tot += s_wave[threadIdx.x][k];
    if (gridDim.x > 1) {
        if (threadIdx.x < kHistorySums) a.part[(size_t)blockIdx.x * kHistorySums + threadIdx.x] = tot;
        last_out_fenced(&a.head->ticket, s_last);
        if (!s_last) return;
        if (threadIdx.x < kHistorySums) {
            tot = 0.0;
            for (int b = 0; b < (int)gridDim.x; ++b)
                tot += __hip_atomic_load(a.part + (size_t)b * kHistorySums + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (threadIdx.x < kHistorySums) s_tot[threadIdx.x] = tot;
    __syncthreads();
    if (threadIdx.x != 0) return;
    // the record, by the one thread that also advances the counters: plain vector stores
    HistoryHead *h = a.head;
    const long long at = h->n_records;
    if (at < (long long)a.capacity) {
        double2 *rec = reinterpret_cast<double2 *>(a.records + (size_t)at * kHistoryFields);
        rec[0] = make_double2((double)clk->step, clk->t);
        rec[1] = make_double2(clk->dt_last, clk->vmax);
        rec[2] = make_double2(-s_tot[0] / ph.DL, -s_tot[1] / ph.DL);  // (k_tau_final: -sum / DL)
        rec[3] = make_double2(s_tot[2], s_tot[3] / (double)(kSlab ? n_bulk : n));
        h->n_records = at + 1;
    } else {
        h->n_dropped += 1;
    }
    if (gridDim.x > 1) __hip_atomic_store(&h->ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// q: parity of the step slot this launch closes
__global__ __launch_bounds__(kHistoryBlock) void k_step_history(const Clock *clk, int q, Grid g, Phys ph, FluidSet s,
                                                                 FluidTmp t, Walls w, HistoryArgs a)
{
    step_history_body(clk, q, g, ph, s, t, w, a);
}

// batch (sphx_batch_history_*): member m = blockIdx.y records its own state (member_set / member_tmp of the views, which are
// member 0's) on its own clock and parameters into its own block of records (m * capacity * kHistoryFields), its own partials
// (m * kHistoryMaxBlocks * kHistorySums) and its own head: ticket, n_records and n_dropped are per member.  gridDim.x is the
// workgroup count of a context of this size, each workgroup takes the same contiguous run and the winner adds the partials
// in the same order: a member's record is bit for bit a standalone context's.
__global__ __launch_bounds__(kHistoryBlock) void k_step_history_b(Members mb, int q, Grid g, FluidSet s, FluidTmp t, Walls w,
                                                                   HistoryArgs a)
{
    const int m = (int)blockIdx.y;
    const Phys ph = mb.ph[m];
    a.records += (size_t)m * (size_t)a.capacity * kHistoryFields;
    a.part += (size_t)m * kHistoryMaxBlocks * kHistorySums;
    a.head += m;
    step_history_body(mb.clk + m, q, g, ph, member_set(mb, m, s), member_tmp(mb, m, t), w, a);
}

// slab of a ring (sphx_slab_history_*): the record of the particles this slab owns.  Launched behind k_slab_pack3 and in front of
// everything of phase 3 (sphx_samplers.hpp, launch_slab_samplers): s, t and the cell array are those of the layout the step ran
// in, so Vol / B of slot i are at i (kHistoryInPlace) whether the step ends with a re-binning or not.
__global__ __launch_bounds__(kHistoryBlock) void k_step_history_s(const Clock *clk, int q, Grid g, Phys ph, FluidSet s,
                                                                   FluidTmp t, Walls w, HistoryArgs a, int n_bulk)
{
    step_history_body<true>(clk, q, g, ph, s, t, w, a, n_bulk);
}

}  // namespace sphx
