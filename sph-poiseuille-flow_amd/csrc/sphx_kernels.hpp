// sphx_kernels.hpp -- the device-resident SPH step for MI355X (gfx950): HIP kernels.
//
// One time step of SPH_Poiseuille.m:250-292 (density_correction -> viscous_force + gravity ->
// transport_correction -> verlet_time_step -> integration_verlet -> periodic wrap -> neighbour
// rebuild) is four neighbour passes with no host round trip,
//     A k_density (list + density)  ->  B k_kgc  ->  CD k_forces  ->  E k_continuity (+ clock)
// followed on every K-th step by the re-binning chain k_clock_scan -> k_scatter -> k_reorder (small channels: folded into
// passes CD and E of that step instead, k_forces_hist -> k_continuity_rebin).  On small channels pass E
// of a step and pass A of the next one share a launch (k_continuity_density): 3 launches per step.  Design (long form
// in DESIGN.md):
//   * particles are sorted by cell, cell id = cx*ncy + cy (y fastest): the 3x3 neighbourhood of a cell is
//     three contiguous index ranges and an x-slab of the channel is one contiguous range; everything a
//     pass gathers per neighbour is a 16- or 32-byte record (double2 pos / vel, double4 {Vol,p,rho_h,rho},
//     double4 B) because the passes are bound by the number of scattered loads, not by bytes;
//   * in x the cells tile the period exactly (ncx = floor(DL/(2h+skin)), width >= 2h+skin), so the wrapped
//     3x3 sweep with a min-image dx sees every neighbour and the reference's ghost entries +
//     seen_neighbor (mex/sph_neighbor_search_mex.c:282-295,342,383) are not needed; the accepted set is
//     the same {1e-24 < r^2 < (2h)^2} (:368).  A slab of a multi-GPU run uses the same kernels on an
//     open (non-periodic) window of columns;
//   * cell skin: between two re-binnings the layout is frozen, sweeps are centred on the cell a particle
//     was binned into, and the clock stops the loop (or, large channels and slabs: re-bins by itself) before any
//     particle is further than skin/2 from where it was binned -- see Clock::drift, FluidSet::cell / posb;
//   * pass A records the accepted neighbours (fluid first, then wall) of the step in a lane-major index list;
//     the other three passes walk that list (all lanes busy, no cut-off branch, no cell lookups) -- the
//     geometry is frozen for the step exactly as in the reference, which reuses dx,dy,r,W,dW of the pair
//     list built at the end of the previous step.  The first step after a re-binning also records every
//     pair within 2h+skin (superset list); the other steps of the cycle walk that instead of the cells;
//   * every pair sum is a per-particle gather (each fluid-fluid update of mex/sph_physics_mex.c is
//     symmetric under i<->j): no atomics in the physics, bitwise reproducible run to run;
//   * LPP lanes of a wavefront share one particle's ring and combine with __shfl_xor (wave64): 32 / 16 at a few thousand
//     particles (compact kernels: a pass is a chain of dependent memory round trips, every pass requests its
//     own-particle data, its list row count and its first list rows before it waits for the run flag), 8 / 4 / 2 above
//     (the "_w" forms: list entries three rows ahead, fluid / wall loops, LDS tiles of the neighbourhood);
//   * dt, t, the step counter, the particle count and the stop test live in a device-side clock so
//     steps can be captured into a hipGraph and replayed.  Small channels: the clock update rides in a tail workgroup of
//     the last launch of a step (continuity_tail).  Large channels ("dynamic" contexts) and slabs: the clock also decides
//     when to re-bin and the re-binning kernels of every step skip themselves otherwise (slot_active, clock_step);
//   * x-slabs (multi-GPU): k_slab_* at the end of this file.
#pragma once
#include <type_traits>

#include "sphx_device.hpp"
#include "sphx_xcd_block.hpp"

namespace sphx {

constexpr int kBlock = 256;
constexpr int kScanBlock = 1024;
constexpr int kBigScanCells = 8192;  // above this the cell scan runs as three multi-block kernels

struct Grid {
    int ncx, ncy, ncells;
    int periodic;         // 1: columns wrap in x (single GPU); 0: open window (slab)
    double DL, half_DL;   // min-image: |dx| > half_DL -> dx -+ DL ; half_DL = +inf in an open window
    double x0, y0, inv_csx, inv_csy;
    double own_lo, own_hi;  // particles with own_lo <= x < own_hi are owned by this context
    // Slabs that re-bin every K-th step: between two re-binnings ownership is frozen, it goes by the column a particle
    // was BINNED into (own_c0 <= column < own_c1), not by where it has drifted since
    int own_by_cell, own_c0, own_c1;
};

__device__ __forceinline__ bool owns(const Grid &g, double x, int cell)
{
    if (!g.own_by_cell) return x >= g.own_lo && x < g.own_hi;
    const int cx = cell / g.ncy;
    return cx >= g.own_c0 && cx < g.own_c1;
}

struct Phys {
    KernelConst kc;
    double rho0, inv_sigma0, mu, p0, c_f, g, tc, nu, DL, DH, w0;
    double dt_viscous, dt_body;  // the two step limits that do not depend on the state (next_dt): 0.125 h^2 / nu, 0.25 sqrt(h / |g|)
};

// Device-side clock: replaces the host variables state.t / state.step / dt_step / remain of
// SPH_Poiseuille.m:247-267 so the loop needs no host decisions.
struct Clock {
    double t, dt, dt_last, t_target, t_end, vmax;
    long long step, steps_left;  // steps_left < 0: unlimited
    int run[2];                  // run[q]: the step slot of parity q executes
    int status;
    int n;                       // particles currently held (fluid, incl. slab halo copies)
    double drift;                // largest distance of any particle from where it was when the grid was built
    int need_rebuild;            // 1: drift exceeded half the cell skin -> the loop stopped, host must re-bin
    int n_rebins;                // dynamic contexts / skinned slabs: re-binnings decided by the clock so far (statistics)
    // "dynamic" contexts (large channels): the device itself decides when to re-bin -- at the K-th step since the
    // last re-binning or as soon as the drift exceeds skin/2 -- and the re-binning kernels of every step skip
    // themselves unless rebuild_now is set; no host round trip, need_rebuild is never raised
    int fresh;                   // 1: the grid has just been rebuilt (pass A sweeps the cells and records the superset list)
    int rebuild_now;             // 1: the re-binning kernels of this step run
    int pos_count;               // steps since the last re-binning
    int n_drift_rebuilds;        // re-binnings triggered by the drift bound (statistics)
    // Whenever the loop stops (step budget used up, target reached, status, stale grid) the clock is also written to
    // `pub`, a copy in pinned host memory: the host then needs no device-to-host copy to learn how a batch ended.
    // seq counts the batches armed (k_prepare), so the host can tell a fresh copy from an old one.
    long long seq;
    Clock *pub;
    // Opt-in dual-rate loop (sphx_params::dual_rate, the outer / inner stepping the reference's README describes): a step
    // slot is one OUTER step of n_in inner sub-steps of length dt -- density, KGC, viscous force and transport shift once,
    // pressure / continuity n_in times.  n_in = 1 is the reference's loop (SPH_Poiseuille.m:250-292), the parity path.
    int n_in;
    // pos_count as the step slot of parity q has to see it: written by the clock update of the slot BEFORE it (parity 1 - q,
    // or k_prepare), never by the slot's own.  k_slab_pack3's workgroups take the re-binning decision each by itself while the
    // last one out already advances the clock: a workgroup dispatched late must still read what the others read.
    // (two shorts in the place of a padding word: a Clock lives in registers in the tail workgroups of pass E, whose kernels
    //  sit exactly at their register budget -- the struct must not grow)
    short pos_q[2];
};

// Everything a neighbour pass GATHERS per neighbour is stored as 16- or 32-byte records (position, velocity,
// {Vol, p_half, rho_half, rho}, B): the passes are bound by the number of scattered load instructions (texture
// addresser), not by bytes, and one 16-byte load costs the same address work as one 8-byte load.
struct FluidSet {  // persistent per-particle state, sorted by cell
    double2 *pos, *vel;
    double *drho, *mass;
    int *id;
    int *start;  // [ncells+1] cell ranges of this ordering
    int *cell;   // [n] the cell each slot was BINNED into (positions may since have drifted by < skin/2)
    double2 *posb;  // [n] position at binning time (nullptr: grid rebuilt every step, drift not tracked)
};

struct FluidTmp {
    double2 *posn, *veln;      // end-of-step state, pre-sort order
    double *drhon;
    double4 *a;                // per-step fields {Vol, p_half, rho_half, rho}
    double4 *B;                // per-step KGC matrix {B11, B12, B21, B22}
    double2 *fp, *f;           // outputs of the step: force_prior, force
    double *rho_out, *p_out;
    int *cellid, *count, *perm, *src_of;
    double *vpart;   // per-block max |v|^2 of pass E (owned particles only)
    double *dpart;   // per-block max drift^2 from the binning positions after this step (pass CD)
    int *nl_idx;     // neighbour list, entry m of lane l at nl_idx[m*nl_stride + l]
    int *nl_cnt;     // [nl_stride] entries per lane
    int *flags;      // [1] sticky device status bits (list overflow ...)
    int *tile_sum;   // big scan: per-tile sums / offsets
    int nl_stride, nl_cap;
    // Superset list (contexts that re-bin every K-th step): every pair within 2h + skin at binning time, same
    // lane-major layout.  Built by pass A of the first step after a re-bin; the other steps of the cycle walk it
    // (~1.3x the true neighbours) instead of sweeping cells (~3.7x).
    int *sl_idx, *sl_cnt;
    int sl_cap;
    double sl_rcut2;  // (2h + skin)^2
    int cap;         // particle capacity of every per-particle array (loads below it are always in bounds)
    int n_vpart;     // entries of vpart / dpart (= workgroups of a pass)
    double half_skin;  // < 0: drift not tracked
    double *vol;     // Vol once more, 8 bytes per particle: passes B and E gather nothing else of `a`, and pulling the
                     // 32-byte records through the caches for one double costs them ~15 % (measured the other way
                     // round: 64-byte records made them 25 % slower)
    // Large-channel kernels (LPP <= 8) keep the FLUID entries of both lists as 16-bit index differences k - i (modulo the
    // population on a periodic grid), two rows per 32-bit word: word p of lane l = rows 2p (low half) and 2p+1 at
    // nl_pk[p*nl_stride + l].  The neighbours of a particle lie in the three cell columns around its own: a few thousand
    // slots either way.  Wall entries (rows behind a lane's fluid rows) stay in nl_idx / sl_idx at their row.  Halves the
    // list bytes the passes move (at 6 M particles the lists were 40-60 % of every pass's HBM traffic).  nullptr: compact kernels.
    int *nl_pk, *sl_pk;
    int has_slack;     // 1: the arrays hold markedly more slots than particles (slabs), see beyond_population
    double *seal_out;  // skinned slabs: the tail workgroup of pass E leaves {max |v|, max drift} of the owned particles here
                       // (the input of the step's max all-reduce), see slab_seal_tail
    int lazy_out;      // large-channel kernels: 1 = the output-only fields of a step (force, force_prior, rho, p) are written by the
                       // LAST step of a batch only, 2 = never, see step_outputs_wanted
    int *tmap;         // large-channel kernels: the tile layout of every workgroup (8 ints each, see tile_map_of), written by the
                       // cell sweep at each re-binning
};

// "no value yet" in vpart when pass E carries the clock update in a tail workgroup (see continuity_tail)
constexpr unsigned long long kVpartEmpty = ~0ull;

struct Walls {
    const double2 *pos;
    const double4 *a;  // {Vol, vx, vy, 0}
    const int *id;
    const int *start;    // [ncells+1]
    const int *row_any;  // [ncy] 1 when rows cy-1..cy+1 hold any wall particle
    int n;
};

// A batch (sphx_batch_*): M channels of one geometry stepped by the same launches.  Member m is blockIdx.y of every "_b"
// kernel.  Each per-member array is ONE allocation of M blocks, member m's block at base + m * stride: the FluidSet /
// FluidTmp / raw pointers a "_b" kernel receives are those of member 0, and member_view moves them to member m.  Walls and
// Grid are shared and stored once; clocks and the parameters that may differ (Phys) are tables indexed by member.  The
// bodies are the ones the single-channel kernels run (same source, same flags): a member's arithmetic is bit for bit that
// of a standalone context.
struct Members {
    Clock *clk;         // [M]
    const Phys *ph;     // [M]
    long long part;     // stride of the per-particle arrays (FluidTmp::cap)
    int cells;          // ... of cell ranges and histograms (ncells + 1)
    int blocks;         // ... of the per-workgroup maxima (n_vpart)
    int lanes;          // ... of the list row counts (nl_stride)
    long long list, slist;  // ... of the step list and the superset list (nl_stride * nl_cap, nl_stride * sl_cap)
};

template <typename T>
__device__ __forceinline__ T *member_ptr(T *p, long long stride, int m)
{
    return p ? p + stride * m : p;  // (nullptr stays nullptr: optional arrays)
}

__device__ __forceinline__ FluidSet member_set(const Members &mb, int m, FluidSet s)
{
    s.pos = member_ptr(s.pos, mb.part, m); s.vel = member_ptr(s.vel, mb.part, m);
    s.drho = member_ptr(s.drho, mb.part, m); s.mass = member_ptr(s.mass, mb.part, m);
    s.id = member_ptr(s.id, mb.part, m); s.cell = member_ptr(s.cell, mb.part, m); s.posb = member_ptr(s.posb, mb.part, m);
    s.start = member_ptr(s.start, mb.cells, m);
    return s;
}

__device__ __forceinline__ FluidTmp member_tmp(const Members &mb, int m, FluidTmp t)
{
    const long long P = mb.part;
    t.posn = member_ptr(t.posn, P, m); t.veln = member_ptr(t.veln, P, m); t.drhon = member_ptr(t.drhon, P, m);
    t.a = member_ptr(t.a, P, m); t.B = member_ptr(t.B, P, m); t.fp = member_ptr(t.fp, P, m); t.f = member_ptr(t.f, P, m);
    t.rho_out = member_ptr(t.rho_out, P, m); t.p_out = member_ptr(t.p_out, P, m); t.vol = member_ptr(t.vol, P, m);
    t.cellid = member_ptr(t.cellid, P, m); t.perm = member_ptr(t.perm, P, m); t.src_of = member_ptr(t.src_of, P, m);
    t.count = member_ptr(t.count, (long long)mb.cells, m);
    t.vpart = member_ptr(t.vpart, (long long)mb.blocks, m); t.dpart = member_ptr(t.dpart, (long long)mb.blocks, m);
    t.nl_idx = member_ptr(t.nl_idx, mb.list, m); t.sl_idx = member_ptr(t.sl_idx, mb.slist, m);
    t.nl_cnt = member_ptr(t.nl_cnt, (long long)mb.lanes, m); t.sl_cnt = member_ptr(t.sl_cnt, (long long)mb.lanes, m);
    t.flags = member_ptr(t.flags, 1ll, m);
    t.tile_sum = nullptr;  // (batches scan their cells in one workgroup, see sphx_batch_create)
    return t;
}

__device__ __forceinline__ void cell_of(const Grid &g, double x, double y, int &cx, int &cy)
{
    cx = (int)floor((x - g.x0) * g.inv_csx);
    cx = min(max(cx, 0), g.ncx - 1);
    cy = (int)floor((y - g.y0) * g.inv_csy);
    cy = min(max(cy, 0), g.ncy - 1);
}

// the cell a slot is stored in (set when the grid was built); sweeps are centred on it, not on the cell of the
// current position, because between two grid builds particles drift by up to skin/2
__device__ __forceinline__ void binned_cell(const Grid &g, const FluidSet &s, int i, int &cx, int &cy)
{
    const int c = s.cell[i];
    cx = c / g.ncy;
    cy = c - cx * g.ncy;
}

__device__ __forceinline__ double wrap_x(double x, double DL) { return x - floor(x / DL) * DL; }

// minimum-image separation (mex/sph_neighbor_search_mex.c:357-363); a no-op in an open window
__device__ __forceinline__ double min_image(const Grid &g, double dx)
{
    if (dx > g.half_DL) dx -= g.DL;
    else if (dx < -g.half_DL) dx += g.DL;
    return dx;
}

// (xcd_block(first, j, nb), which block of a pass a workgroup takes: sphx_xcd_block.hpp)
// A workgroup of a pass: its index j among the pass's workgroups, and the physical block the pass starts at
struct PassWg {
    int j, first;
    __host__ __device__ PassWg(int j, int first = 0) : j(j), first(first) {}
};
__device__ __forceinline__ int xcd_block(PassWg b, int nb) { return xcd_block(b.first, b.j, nb); }

// A period of one or two cell columns (DL < 6h): the columns cx-1, cx, cx+1 are not distinct -- the reference meets the
// same particle as a real and as a ghost entry there and de-duplicates with seen_neighbor
// (mex/sph_neighbor_search_mex.c:282-295,342,383); here each distinct column is swept once and the minimum-image fold
// picks the nearest image.
__device__ __forceinline__ bool duplicate_column(const Grid &g, int ox)
{
    return (g.ncx == 1 && ox != 0) || (g.ncx == 2 && ox == 1);
}

// Column cx + ox (ox = -1, 0, 1) of the three that hold a cell's neighbours -> col.  False: there is none -- beyond the end of an
// open window, or the same column as another of the three.
__device__ __forceinline__ bool neighbour_column(const Grid &g, int cx, int ox, int &col)
{
    col = cx + ox;
    bool ok = true;
    if (g.periodic) {
        if (duplicate_column(g, ox)) ok = false;
        if (col < 0) col += g.ncx;
        else if (col >= g.ncx) col -= g.ncx;
    } else if (col < 0 || col >= g.ncx) {
        ok = false;
    }
    return ok;
}
// Three index ranges walked as ONE virtual index range (a group of lanes then needs one or two trips instead of one or two
// per range, and each trip's loads are independent of the previous trip's): position v -> index; n0, n1: the lengths of the
// first two ranges
__device__ __forceinline__ int ranges_index(int lo0, int lo1, int lo2, int n0, int n1, int v)
{
    return v < n0 ? lo0 + v : (v < n0 + n1 ? lo1 + (v - n0) : lo2 + (v - n0 - n1));
}

// Folded re-binning (k_forces_hist, k_continuity_rebin): is cell c_new one of the 3 x 3 cells around c_old (columns wrap on a
// periodic grid of at least three columns)?  Between two re-binnings nobody moves further than half a skin plus one step, far
// less than a cell, so every member of a new cell was binned in that cell's 3 x 3 neighbourhood.
__device__ __forceinline__ bool rebin_near(const Grid &g, int c_old, int c_new)
{
    const int ox = c_old / g.ncy, oy = c_old - ox * g.ncy;
    const int nx = c_new / g.ncy, ny = c_new - nx * g.ncy;
    int dx = abs(nx - ox);
    if (g.periodic && dx == g.ncx - 1) dx = 1;
    return dx <= 1 && abs(ny - oy) <= 1;
}
constexpr int kFoldCells = 2048;  // the folded re-binning scans the histogram in LDS in every workgroup: fewer cells than this

// the value of the other lane of a pair (lanes 2k, 2k + 1): one DPP move (quad_perm [1 0 3 2]), no LDS crossbar, no ballot
__device__ __forceinline__ int pair_partner(int v) { return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true); }

// Sum over the LPP lanes of a particle, in every lane.  Up to 16 lanes a group lies in one DPP row: two quad permutes
// (lane ^ 1, lane ^ 2), row_half_mirror and row_mirror pair every lane with one that holds the other part -- two v_mov_dpp
// and an add per stage, where __shfl_xor is two ds_bpermute through the LDS crossbar and a wait (a pass of the small
// channels ends with four to seven such sums, four stages each, all on its critical path).
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v)
{
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
// max over the wave of non-negative values (squares), in every lane: four DPP stages inside the rows, two crossbar stages across
__device__ __forceinline__ double wave_max(double v)
{
    v = fmax(v, dpp_f64<0xB1>(v));
    v = fmax(v, dpp_f64<0x4E>(v));
    v = fmax(v, dpp_f64<0x141>(v));
    v = fmax(v, dpp_f64<0x140>(v));
    v = fmax(v, __shfl_xor(v, 16));
    return fmax(v, __shfl_xor(v, 32));
}
// largest / smallest value of an int over the LPP lanes of a particle, in every lane (same stages as group_sum)
template <int LPP, bool MAX>
__device__ __forceinline__ int group_extreme(int v)
{
    auto pick = [](int a, int b) { return MAX ? max(a, b) : min(a, b); };
    if (LPP >= 2) v = pick(v, __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true));
    if (LPP >= 4) v = pick(v, __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true));
    if (LPP >= 8) v = pick(v, __builtin_amdgcn_mov_dpp(v, 0x141, 0xF, 0xF, true));
    if (LPP >= 16) v = pick(v, __builtin_amdgcn_mov_dpp(v, 0x140, 0xF, 0xF, true));
#pragma unroll
    for (int off = LPP / 2; off >= 16; off >>= 1) v = pick(v, __shfl_xor(v, off));
    return v;
}
template <int LPP>
__device__ __forceinline__ double group_sum(double v)
{
    if (LPP >= 2) v += dpp_f64<0xB1>(v);    // quad_perm [1 0 3 2]
    if (LPP >= 4) v += dpp_f64<0x4E>(v);    // quad_perm [2 3 0 1]
    if (LPP >= 8) v += dpp_f64<0x141>(v);   // row_half_mirror
    if (LPP >= 16) v += dpp_f64<0x140>(v);  // row_mirror
#pragma unroll
    for (int off = LPP / 2; off >= 16; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Pass CD, lead lane: squared drift of the particle's new position from where it was binned (pb: its FluidSet::posb record) --
// zero for a particle a slab does not own, infinite for a NaN: the maximum has to see it
__device__ __forceinline__ double tracked_drift2(const Grid &g, const FluidSet &s, int i, double xo, double yo, const double2 pb)
{
    if (g.own_by_cell && !owns(g, 0.0, s.cell[i])) return 0.0;  // (a slab bounds the drift of what it owns)
    const double ddx = min_image(g, xo - pb.x), ddy = yo - pb.y;
    const double d2 = ddx * ddx + ddy * ddy;
    return d2 != d2 ? INFINITY : d2;
}
// ... and its maximum over the workgroup -> t.dpart[blk]: the largest drift from the binning positions bounds how stale the cell
// grid may get (Clock::drift).  Every thread of the workgroup calls this (one barrier).
// BLK: the threads of the workgroup.  A one-wave workgroup (BLK = 64) has no workgroup epilogue: the wave's maximum is the entry,
// no LDS, no barrier.
template <int BLK = kBlock>
__device__ __forceinline__ void store_block_drift(const FluidTmp &t, int blk, double d2)
{
    d2 = wave_max(d2);
    if constexpr (BLK == 64) {
        if (threadIdx.x == 0) t.dpart[blk] = d2;
    } else {
        __shared__ double s_d2[BLK / 64];
        if ((threadIdx.x & 63) == 0) s_d2[threadIdx.x >> 6] = d2;
        __syncthreads();
        if (threadIdx.x == 0) {
            double m = s_d2[0];
            for (int k = 1; k < BLK / 64; ++k) m = fmax(m, s_d2[k]);
            t.dpart[blk] = m;
        }
    }
}

// Visit the candidates of the three cell columns around (cx,cy): body(k).
template <int LPP, typename Body>
__device__ __forceinline__ void sweep(const Grid &g, const int *__restrict__ start, int cx, int cy,
                                      int sub, Body &&body)
{
    const int cylo = max(cy - 1, 0), cyhi = min(cy + 1, g.ncy - 1);
#pragma unroll
    for (int ox = -1; ox <= 1; ++ox) {
        int col;
        if (!neighbour_column(g, cx, ox, col)) continue;
        const int base = col * g.ncy;
        const int lo = start[base + cylo], hi = start[base + cyhi + 1];
        for (int k = lo + sub; k < hi; k += LPP) body(k);
    }
}

__device__ __forceinline__ double next_dt(const Clock &c, const Phys &ph)
{  // SPH_Poiseuille.m:519-527 with remain of :252
    const double remain = fmin(c.t_target - c.t, c.t_end - c.t);
    const double h = ph.kc.h;
    const double dt_acoustic = 0.25 * h / fmax(ph.c_f + c.vmax, 1e-12);
    // (the clock's thread runs this between two steps, with the whole chip waiting: the viscous and the body-force limit -- two
    //  divisions and a square root of constants -- come precomputed, make_phys)
    const double dt_viscous = ph.dt_viscous, dt_body = ph.dt_body;
    if (c.n_in > 1) {
        // outer step by the advection / viscous / body-force scales, at most n_in acoustic steps long; dt is the inner step
        const double dt_adv = 0.25 * h / fmax(c.vmax, 1e-12);
        const double Dt = fmin(fmin(fmin(dt_adv, dt_viscous), fmin(dt_body, remain)), c.n_in * dt_acoustic);
        return fmax(Dt / c.n_in, 1e-12);
    }
    const double dt = fmin(fmin(dt_acoustic, dt_viscous), fmin(dt_body, remain));
    return fmax(dt, 1e-12);
}

__device__ __forceinline__ bool loop_continues(const Clock &c)
{  // while state.t < target_time - 1e-12 (SPH_Poiseuille.m:250) and step budget left
    return (c.t < c.t_target - 1e-12) && (c.steps_left != 0) && (c.status == 0) && (c.need_rebuild == 0);
}

// force, force_prior (pass CD) and rho, p (pass E) are results for the caller: no later step reads them (the next pass A sums
// the density afresh, the next pass CD builds both forces from scratch), and they are 48 of the ~650 bytes a large-channel
// step moves per particle.  Contexts with FluidTmp::lazy_out write them only in the step after which the batch stops --
// the step budget's last step, or the one that reaches the target time -- which is the only state a caller can look at.
// (The clock still holds the state BEFORE this step while its passes run: clock_step comes after pass E.)
__device__ __forceinline__ bool step_outputs_wanted(const Clock *clk, const FluidTmp &t)
{
    if (!t.lazy_out) return true;
    if (t.lazy_out == 2) return false;  // (a slab: nobody can ask for them, sphx_slab_snapshot hands out the state only)
    return clk->steps_left == 1 || !(clk->t + clk->dt < clk->t_target - 1e-12);  // (the test of loop_continues, a step early)
}

// Kernels of the re-binning chain take the slot parity with a flag: bit 1 set = "only when the clock says
// rebuild_now" (dynamic contexts), so the same kernels serve the scheduled and the device-decided re-binning.
constexpr int kOnlyIfRebuild = 2, kOnlyIfNoHistogram = 4;
__device__ __forceinline__ bool slot_active(const Clock *clk, int qf)
{
    if (!clk->run[qf & 1]) return false;
    if ((qf & kOnlyIfNoHistogram) && clk->rebuild_now == 2) return false;  // pass E binned the particles already
    return !(qf & kOnlyIfRebuild) || clk->rebuild_now != 0;
}

// one thread: arm the clock for an advance call.  vmax_in (optional) overrides the stored vmax (slab:
// the all-reduced global value).
__device__ __forceinline__ void prepare_clock(Clock *clk, const Phys &ph, double t_target, long long max_steps, int q0,
                                              const double *vmax_in)
{
    Clock c = *clk;
    if (vmax_in) c.vmax = *vmax_in;
    c.t_target = fmin(t_target, c.t_end);  // target_time = min(t + output_interval, t_end), SPH_Poiseuille.m:248
    c.steps_left = max_steps > 0 ? max_steps : -1;
    if (!(c.vmax == c.vmax) || isinf(c.vmax)) c.status = SPHX_ERR_DIVERGED;
    c.dt = next_dt(c, ph);
    const int go = loop_continues(c) ? 1 : 0;
    c.run[0] = q0 == 0 ? go : 0;  // constant indices: a dynamically indexed member forces the struct into scratch
    c.run[1] = q0 == 0 ? 0 : go;
    c.pos_q[0] = (short)c.pos_count;     // (the first slot of the batch reads its parity's copy; the other one is rewritten before use)
    c.pos_q[1] = (short)c.pos_count;
    c.seq += 1;
    *clk = c;
    if (!go && c.pub) *c.pub = c;
}
__global__ void k_prepare(Clock *clk, Phys ph, double t_target, long long max_steps, int q0, const double *vmax_in)
{
    prepare_clock(clk, ph, t_target, max_steps, q0, vmax_in);
}
// batch: one workgroup of one thread per member; max_steps_of (optional): a step budget per member instead of max_steps
__global__ __launch_bounds__(64) void k_prepare_b(Members mb, double t_target, long long max_steps, const long long *max_steps_of,
                                                  int q0)
{
    const int m = (int)blockIdx.y;
    const Phys ph = mb.ph[m];
    prepare_clock(mb.clk + m, ph, t_target, max_steps_of ? max_steps_of[m] : max_steps, q0, nullptr);
}

// ---------------------------------------------------------------------------------------------
// The neighbour list of a step.  Pass A sweeps the candidates (3 cell columns of fluid, and of wall
// particles next to a wall) and packs the accepted ones into ONE list per particle: entry m belongs to
// lane m % LPP, row m / LPP, so every lane owns ceil-or-floor(cnt / LPP) neighbours in the later passes
// (balanced trip counts) and the lanes of a group walk adjacent particles.  Wall neighbours carry
// kWallBit: passes B..E walk one list and never touch the cell structure again (at a few thousand
// particles a pass is a chain of dependent memory round trips; cell -> row flag -> cell range -> wall
// particle was three of them).
// ---------------------------------------------------------------------------------------------
constexpr int kWallBit = 1 << 30;
// nl_cnt[lane]: rows this lane owns (low half) and how many of them, the first ones, hold fluid neighbours (high half)
__device__ __forceinline__ int list_rows(int packed) { return packed & 0x3fff; }
__device__ __forceinline__ int list_fluid_rows(int packed) { return packed >> 16; }
// ... and the word of lane `sub` of a particle with cnt neighbours: the lane owns entries sub, sub + LPP, ...  Fluid neighbours
// come first (cnt_fl of them), so a lane's rows are its fluid rows followed by its wall rows.
template <int LPP>
__device__ __forceinline__ int list_row_counts(int cnt, int cnt_fl, int sub)
{
    return (cnt > sub ? (cnt - sub + LPP - 1) / LPP : 0) | ((cnt_fl > sub ? (cnt_fl - sub + LPP - 1) / LPP : 0) << 16);
}
// Bits 14 and 15 of a lane's packed counts (slot-coded lists only, see kSlotCodes): some fluid entry of the lane's column of the
// SUPERSET list -- so of every list walked until the next re-binning -- names something beyond the first kForceSlots /
// kSlotCodes slots of the workgroup's layout.  Set by the cell sweep, handed on by pass A's walk.  A wavefront none of whose
// lanes has the bit reads its tile without looking at the entries (the `near` walks): the per-lane choice between the tile
// and global memory is a pair of exec-mask regions around every fetch and, because both arms load into the same registers,
// a wait for every outstanding global load -- the list words requested ahead -- in front of every LDS read.  Measured at 6 M
// particles with a timing-only build whose fetches never look (profiles/r04_pretend_lds_only_fetch_*.txt): pass A's walk
// 420 -> 369 us, KGC 252 -> 239, forces 522 -> 507, continuity 288 -> 275.
constexpr int kFarForcesBit = 1 << 14, kFarTileBit = 1 << 15;

// 16-bit entries of the large-channel lists (FluidTmp::nl_pk / sl_pk)
constexpr int kDeltaMax = 32767;
__device__ __forceinline__ void put_delta(int *pk, int stride, int row, int col, int d)
{
    reinterpret_cast<short *>(pk)[((size_t)((unsigned)row >> 1) * (unsigned)stride + (unsigned)col) * 2 + ((unsigned)row & 1u)] = (short)d;
}
__device__ __forceinline__ int delta_lo(int word) { return (int)(short)(word & 0xffff); }
__device__ __forceinline__ int delta_hi(int word) { return word >> 16; }
__device__ __forceinline__ int delta_of_row(const int *pk, int stride, int row, int col)
{
    const int word = pk[(size_t)(row >> 1) * stride + col];
    return (row & 1) ? delta_hi(word) : delta_lo(word);
}
// index difference k - i as stored (periodic grids: the representative nearest to zero modulo the population n)
__device__ __forceinline__ int encode_delta(int k, int i, int n, bool periodic, int *flags, int limit = kDeltaMax)
{
    int d = k - i;
    if (periodic) {
        const int half = n >> 1;
        if (d > half) d -= n;
        else if (d < -half) d += n;
    }
    if (d > limit || d < -limit) atomicOr(flags, 1);  // (ctx_setup keeps such grids on the compact kernels)
    return d;
}
// Slot-coded entries (template parameter CODED of the large-channel kernels; contexts whose four passes all stage LDS tiles,
// sphx_ctx::coded_lists).  The passes of such a context spent 13 vector instructions per neighbour turning its index into a
// tile slot (TileMap::slot: three ranges), four times a step -- and the answer does not change between two re-binnings.
// So the cell sweep, which runs once per re-binning, stores the answer: a 16-bit entry below kSlotCodes IS the neighbour's
// position in the workgroup's tile layout (tile_ranges at capacity kSlotCodes: own column, left, right -- a pass with a
// smaller tile stages a prefix of the same layout); any other value is the index difference + kCodeBias (neighbours the
// layout does not reach: a workgroup running across a column end, ranges longer than the layout).
#ifndef SPHX_EXP_PRETEND_COMPLETE_TILE
#define SPHX_EXP_PRETEND_COMPLETE_TILE 0  // measurement builds only (tools/probes/build_variant_lib.sh), see k_forces_w
#endif
constexpr int kSlotCodes = 480;
constexpr int kForceSlots = 464;  // the force pass stages this many (88-byte records: four workgroups of 40 864 B are the 160 KB of a CU)
constexpr int kCodeBias = 33000;
constexpr int kCodedDeltaMax = 32500;  // kSlotCodes <= kCodeBias - kCodedDeltaMax,  kCodeBias + kCodedDeltaMax <= 65535
__device__ __forceinline__ int code_lo(int word) { return word & 0xffff; }
__device__ __forceinline__ int code_hi(int word) { return (int)((unsigned)word >> 16); }
__device__ __forceinline__ int code_of_row(const int *pk, int stride, int row, int col)
{
    const int word = pk[(size_t)(row >> 1) * stride + col];
    return (row & 1) ? code_hi(word) : code_lo(word);
}
// ... and back: only wavefronts near the periodic seam can hold a particle whose neighbours wrap (see near_seam)
__device__ __forceinline__ int wrap_index(int k, int n) { return k < 0 ? k + n : (k >= n ? k - n : k); }

// Appending to a list (pass A).  The LPP lanes of a particle test LPP consecutive candidates at a time (uniform trip count over
// the group); accepted ones are packed with ballot + popcount.  A group (LPP <= 32 aligned lanes) lies in one 32-bit half of
// the wave's ballot: 32-bit shifts / popcounts (the candidate loop of the sweeping variants is VALU-bound).
template <int LPP>
struct LaneGroup {
    int sub, lane, half_shift, row_base;  // row_base: list column of lane 0 of this group
    unsigned grp_mask, below_me;
    __device__ __forceinline__ LaneGroup(int tid, int sub)
        : sub(sub), lane(threadIdx.x & 63), half_shift((lane & ~(LPP - 1)) & 31), row_base(tid - sub),
          grp_mask(LPP >= 32 ? 0xffffffffu : ((1u << (LPP & 31)) - 1u)), below_me((1u << sub) - 1u)  // sub <= 31
    {
    }
    __device__ __forceinline__ unsigned bits(bool acc) const  // who of the group accepts: bit k = its lane k
    {
        const unsigned long long bal = __ballot(acc);
        const unsigned half = lane < 32 ? (unsigned)bal : (unsigned)(bal >> 32);
        return (half >> half_shift) & grp_mask;
    }
};
// compact lists (32-bit entries, nl_idx / sl_idx of `cap` rows): the group's accepted entries go behind the n it holds
template <int LPP>
__device__ __forceinline__ void list_push(const LaneGroup<LPP> &lg, int *idx, int cap, int stride, int &n, bool acc, int entry)
{
    if (LPP == 1) {
        if (acc) {
            if (n < cap) idx[(size_t)n * stride + lg.row_base] = entry;
            ++n;
        }
    } else {
        const unsigned grp = lg.bits(acc);
        if (acc) {
            const int m = n + __popc(grp & lg.below_me);
            if (m / LPP < cap) idx[(size_t)(m / LPP) * stride + lg.row_base + (m % LPP)] = entry;
        }
        n += __popc(grp);
    }
}
// large-channel lists: a fluid entry goes to the packed list pk (16 bits: the index difference to the group's particle, or a
// slot code), a wall entry to the 32-bit one
// (2 lanes per particle: who else accepts is one DPP move away -- the ballot, the half select, the shift and the two
//  popcounts were 9 of the ~55 vector instructions of a candidate in a pass that is ALU-bound; unsigned row arithmetic:
//  m / LPP on a signed m costs a sign fix-up per use)
template <int LPP>
__device__ __forceinline__ void list_push_w(const LaneGroup<LPP> &lg, int *idx, int *pk, int cap, int stride, int &n, bool acc,
                                            int entry, bool wall)
{
    int below, all;
    if constexpr (LPP == 2) {
        const int mine = acc ? 1 : 0, other = pair_partner(mine);
        below = lg.sub ? other : 0;
        all = mine + other;
    } else {
        const unsigned grp = LPP == 1 ? (acc ? 1u : 0u) : lg.bits(acc);
        below = __popc(grp & lg.below_me);
        all = __popc(grp);
    }
    if (acc) {
        const unsigned m = (unsigned)(n + below), row = m / LPP, col = (unsigned)lg.row_base + m % LPP;
        if ((int)row < cap) {
            if (wall) idx[(size_t)row * stride + col] = entry;
            else put_delta(pk, stride, (int)row, (int)col, entry);
        }
    }
    n += all;
}

// Prologue shared by the passes: everything whose address does not depend on the clock is requested
// BEFORE the run flag is looked at, so the clock read overlaps the particle's own loads.
// (threads: those of the workgroup -- the compact passes take it as a template parameter, BLK; nblk counts workgroups of that size)
#define SPHX_PASS_INDEX_BLK(bid, nblk, threads)                            \
    const int blk = xcd_block((bid), (nblk));                              \
    const int tid = blk * (threads) + threadIdx.x;                         \
    const int i = tid / LPP, sub = tid % LPP;                              \
    const bool in_cap = i < t.cap
#define SPHX_PASS_INDEX_AT(bid, nblk) SPHX_PASS_INDEX_BLK(bid, nblk, kBlock)
#define SPHX_PASS_INDEX() SPHX_PASS_INDEX_AT((int)blockIdx.x, (int)gridDim.x)

// Compact kernels at 16 and 32 lanes per particle (kRowsAhead): a pass is a chain of dependent memory round trips behind a launch,
// so what it asks for has to leave in as few request waves as there are true dependences:
//   wave 1: the clock's words, the row count and the first rows of the list (ListHead: addressed from leading arguments, no
//           scalar wait in front), the particle's own records (behind the one scalar batch, SPHX_ARGS_BATCH);
//   wave 2 (behind the rows): the neighbour records of ALL of those rows, before the first one is used.
// Left alone, the compiler sinks a load into the branch that uses its value -- the rows behind the count, row 1's records
// behind row 0's arithmetic -- and every sunk load is one more round trip on the critical path.  requests_issued() closes a
// wave: loads cannot move across it (to the compiler it may write memory), and it costs no instruction and no wait.
// A lane that does not own a prefetched row asks for its own particle's records instead: rows beyond a lane's count hold
// stale words, and no address is ever formed from one.  The arithmetic stays in row order, so every sum keeps its bits.
// The arguments: a pass reads 25-40 of the ~220 dwords of its kernels' argument segment, and the compiler loads each where it is
// first used -- six to twelve scalar round trips, one behind the other.  An empty asm statement that takes arguments as scalar
// operands makes their loads leave together, with one wait (SPHX_ARGS_BATCH below, "Leading arguments").
template <int LPP>
constexpr bool kRowsAhead = LPP >= 16;
__device__ __forceinline__ void requests_issued() { asm volatile("" ::: "memory"); }
// What a wave of these kernels issues besides its pairs' arithmetic is paid once per four (two) particles, and where a SIMD holds
// two waves of a pass the second one's instructions queue behind the first's: the pass heads keep them few.
//   own_slot: the particle's own records are loaded from slot min(i, cap - 1) without a test.  Every `in_cap ? load : default`
//   was an exec-mask region of its own (save, branch, restore, the defaults moved in front); slot cap - 1 exists, lanes beyond
//   the population (i >= clk->n, so every lane beyond cap) are never `active`, and a group's lanes share i, so what they load
//   reaches no sum and no store.  Records only the lead lane uses are loaded by all of the group: one line, one request.
//   pair_dx: the minimum-image fold of a pair, skipped by a wave in which no lane's pair crosses the periodic seam -- nearly
//   every wave -- for one compare and one scalar branch; otherwise min_image as everywhere else, so the same bits either way.
template <int LPP>
__device__ __forceinline__ int own_slot(int i, int cap) { return kRowsAhead<LPP> ? min(i, cap - 1) : i; }
template <int LPP>
__device__ __forceinline__ double pair_dx(const Grid &g, double dx)
{
    if (kRowsAhead<LPP> && !__any(fabs(dx) > g.half_DL)) return dx;
    return min_image(g, dx);
}
// Leading arguments.  The single-channel forms of these kernels take what wave 1 forms its first addresses from -- the clock,
// the number of workgroups of the pass, the row counts, the list and its stride, and as many own-record pointers as fit -- as
// plain parameters IN FRONT of the structs: built with -amdgpu-kernarg-preload-count the first 14 dwords of the argument
// segment arrive in scalar registers together with the wave (the preload stops at the first struct passed by value), so the
// list loads leave without a scalar round trip in front of them.  The kernel writes the values over the fields of its own
// copies of FluidSet / FluidTmp before it calls the body: the body cannot read the struct's copy of a hot value, and the
// host takes each from the very view it passes by value (hot_* in sphx_resident.hip).  Everything else a pass reads of its
// arguments is named by ONE SPHX_ARGS_BATCH(...) behind the list loads: those scalar loads leave together at the top of the
// kernel and are in flight while wave 1 is; the own records that missed the preload go out when they land.
// `shape` = the workgroups of the pass (the tail workgroup not counted) and the pass's small flag in one dword.
constexpr int kShapeBits = 24;
__host__ __device__ inline int pass_shape(int nblk, int flag) { return (int)(((unsigned)flag << kShapeBits) | (unsigned)nblk); }
__device__ __forceinline__ int shape_blocks(int shape) { return shape & ((1 << kShapeBits) - 1); }
__device__ __forceinline__ int shape_flag(int shape) { return shape >> kShapeBits; }  // (signed: -1 comes back as -1)
#define SPHX_ARGS_BATCH(...) asm volatile("" ::__VA_ARGS__)
// The first rows of a lane's list column, requested together with the row count (at 32 lanes per particle a lane rarely owns
// more than two): count -> entry -> neighbour data becomes {count, entries} -> neighbour data.
// (rows 2 and 3 only where lanes own that many: few lanes per particle)
template <int LPP>
struct FirstRows {
    int e0, e1, e2, e3;
    __device__ __forceinline__ FirstRows(const int *idx, int stride, int tid)
        : e0(idx[tid]), e1(idx[(size_t)stride + tid]), e2(LPP <= 8 ? idx[2 * (size_t)stride + tid] : 0),
          e3(LPP <= 8 ? idx[3 * (size_t)stride + tid] : 0)
    {
    }
    __device__ __forceinline__ FirstRows(int e0, int e1) : e0(e0), e1(e1), e2(0), e3(0) {}  // (requested already: ListHead)
    __device__ __forceinline__ int row(int m, const int *idx, int stride, int tid) const  // entry of row m of the column
    {
        return m == 0 ? e0 : (m == 1 ? e1 : (LPP <= 8 && m == 2 ? e2 : (LPP <= 8 && m == 3 ? e3 : idx[(size_t)m * stride + tid])));
    }
};

// The part of wave 1 whose addresses come from leading arguments alone: the lane's packed row count, its first two rows and
// the clock's words.  Requested in front of SPHX_ARGS_BATCH, so nothing scalar stands between the launch and these loads.
// (Passes B, CD and A read the clock through a pointer to const with scalar loads: they name run, n and dt in their batch, so
//  that the clock's words leave with it and not behind the own records.)
struct ListHead {
    int packed = 0, e0 = 0, e1 = 0, run = 0, n = 0;
    double dt = 0.0;
    __device__ __forceinline__ void request(const Clock *clk, int q, const int *cnt, const int *idx, int stride, int tid)
    {
        run = clk->run[q]; n = clk->n; dt = clk->dt;
        packed = cnt[tid];
        e0 = idx[tid];
        e1 = idx[(size_t)stride + tid];
    }
};

// ---------------------------------------------------------------------------------------------
// pass A: candidate sweep -> neighbour list; number-density summation -> rho, Vol
// (mex/sph_physics_mex.c:188-234) and the half-step density/pressure of integration_1st's pre-pass
// (:857-862), which only needs own-particle data.
// ---------------------------------------------------------------------------------------------
// the half-step density / pressure of a particle (integration_1st's pre-pass, sph_physics_mex.c:857-862)
__device__ __forceinline__ void half_state(const Phys &ph, double rho, double drho, double dt, double &rhoh, double &ph_)
{
    rhoh = rho + 0.5 * dt * drho;
    if (rhoh < 1e-10) rhoh = ph.rho0;
    ph_ = eos_pressure(rhoh, ph.rho0, ph.p0);
}

// Pass A's lead lane, all three forms: the sigma sums of particle i -> rho and Vol, and its record t.a = {Vol, p_half, rho_half,
// rho} (half: with the half-step pair; otherwise pass B completes the record, see density_body)
__device__ __forceinline__ void store_density(const Phys &ph, const FluidTmp &t, int i, double s_in, double s_ct, double mass_i,
                                              double drho_i, double dt, bool half)
{
    const double rho = density_from_sigma(ph.w0 + s_in, s_ct, mass_i, ph.rho0, ph.inv_sigma0);
    const double vol = mass_i / rho;
    double rhoh, p_half;
    half_state(ph, rho, drho_i, dt, rhoh, p_half);
    t.a[i] = half ? make_double4(vol, p_half, rhoh, rho) : make_double4(vol, 0.0, 0.0, rho);
    t.vol[i] = vol;
}

// MODE 0: sweep the cells, write the step's list.  MODE 1: same sweep, also write the superset list.
// MODE 2: walk the superset list instead of the cells.
// bid / nblk: the workgroup's index among the nblk workgroups of this pass, and where the pass starts in the grid (the fused
// launch k_continuity_density runs the pass in a sub-range of its grid; PassWg).  half: also write the half-step density /
// pressure (needs the step's dt; the fused launch runs pass A of the NEXT step, whose dt is not known yet -- pass B completes
// the record there).
template <int LPP, int MODE, int BLK = kBlock>
__device__ __forceinline__ void density_body(const Clock *clk, int q, const Grid &g, const Phys &ph, const FluidSet &s,
                                             const FluidTmp &t, const Walls &w, PassWg bid, int nblk, bool half)
{
    SPHX_PASS_INDEX_BLK(bid, nblk, BLK);
    // the walk at 16 / 32 lanes: row count, first rows and the clock's words leave first (leading arguments, see ListHead)
    constexpr bool kHot = MODE == 2 && kRowsAhead<LPP>;
    constexpr int kAhead = kHot ? 64 / LPP : 2;
    int ns = 0, e_row0 = 0, e_row1 = 0, e_row2 = 0, e_row3 = 0, run_h = 0, n_h = 0;
    double dt_h = 0.0;
    if (kHot) {
        dt_h = clk->dt; run_h = clk->run[q]; n_h = clk->n;
        ns = list_rows(t.sl_cnt[tid]);
        e_row0 = t.sl_idx[tid];
        e_row1 = t.sl_idx[(size_t)t.nl_stride + tid];
        if (kAhead > 2) {
            e_row2 = t.sl_idx[2 * (size_t)t.nl_stride + tid];
            e_row3 = t.sl_idx[3 * (size_t)t.nl_stride + tid];
        }
        SPHX_ARGS_BATCH("s"(s.pos), "s"(s.mass), "s"(s.drho), "s"(t.cap), "s"(t.nl_cnt), "s"(t.nl_idx), "s"(t.nl_cap), "s"(t.a),
                        "s"(t.vol), "s"(w.pos), "s"(w.a), "s"(g.DL), "s"(g.half_DL), "s"(ph.kc.rcut2), "s"(ph.kc.inv_h),
                        "s"(ph.kc.sigma), "s"(ph.w0), "s"(ph.rho0), "s"(ph.inv_sigma0), "s"(run_h), "s"(n_h), "s"(dt_h));
    }
    const int io = kHot ? own_slot<LPP>(i, t.cap) : i;  // (the walk at 16 / 32 lanes: no test around the own records)
    const double2 pi = (kHot || in_cap) ? s.pos[io] : make_double2(0.0, 0.0);
    const int ci = in_cap ? s.cell[i] : 0;
    const bool lead = kHot || (in_cap && sub == 0);  // the lane that finishes the particle
    const double mass_i = lead ? s.mass[io] : 1.0, drho_i = lead ? s.drho[io] : 0.0;
    // list-walking variant: row count and the first two rows are requested here as well (a lane rarely owns more
    // at 32 lanes per particle): count -> entry -> position becomes {count, entries} -> position
    // (kRowsAhead: the first kAhead rows -- 64 candidates; the superset list holds about 48 of them at skin 1.05 h, so three
    //  rows for every lane at 16 lanes per particle and a fourth for some -- and the clock's words in the same wave)
    if (MODE == 2 && !kHot) {
        ns = list_rows(t.sl_cnt[tid]);
        e_row0 = t.sl_idx[tid];
        e_row1 = t.sl_idx[(size_t)t.nl_stride + tid];
    }
    const double dt = kHot ? dt_h : clk->dt;
    const int run_q = kHot ? run_h : clk->run[q], n_now = kHot ? n_h : clk->n;
    if (kHot) requests_issued();
    if (!run_q) return;
    const bool active = i < n_now;
    double s_in = 0.0, s_ct = 0.0;
    int cnt = 0, scnt = 0, cnt_fl = 0, scnt_fl = 0;
    const LaneGroup<LPP> lg(tid, sub);
    auto push = [&](bool acc, int entry) { list_push(lg, t.nl_idx, t.nl_cap, t.nl_stride, cnt, acc, entry); };
    auto push_super = [&](bool acc, int entry) { list_push(lg, t.sl_idx, t.sl_cap, t.nl_stride, scnt, acc, entry); };
    constexpr bool walk = MODE == 2;
    constexpr bool record = MODE == 1;  // also write the superset list
    if (walk) {
        const int rows = group_extreme<LPP, true>(ns);  // (= lane 0's: it owns the most rows)
        if (active) {
            const double xi = pi.x, yi = pi.y;
            // one candidate (has: this lane owns the row; e = 0 where it does not)
            auto test = [&](bool has, int e, const double2 pj, double Volw) {
                bool acc = false;
                if (has) {
                    const bool wall = (e & kWallBit) != 0;
                    const double dx = pair_dx<LPP>(g, xi - pj.x), dy = yi - pj.y;
                    const double r2 = dx * dx + dy * dy;
                    if (r2 > kR2Min && r2 < ph.kc.rcut2) {
                        acc = true;
                        const double W = spline_W_sel(ph.kc, r2 * rsqrt_nr(r2));
                        if (wall) s_ct += W * Volw;
                        else s_in += W;
                    }
                }
                // wall candidates sit behind the fluid ones: the fluid count is the count reached before the first row
                // that holds a wall entry, plus that row's accepted fluid entries
                const bool wall_row = (e & kWallBit) != 0;
                if (!__any(wall_row)) {
                    push(acc, e);
                    cnt_fl = cnt;
                } else {
                    cnt_fl += LPP == 1 ? ((acc && !wall_row) ? 1 : 0) : __popc(lg.bits(acc && !wall_row));
                    push(acc, e);
                }
            };
            if (kRowsAhead<LPP>) {
                // the positions of all prefetched rows in one wave (Vol of a wall candidate with them; a fluid row re-reads its
                // position's first word there, so that the request needs no branch)
                int e_pre[kAhead];
                double2 p_pre[kAhead];
                double v_pre[kAhead];
#pragma unroll
                for (int m = 0; m < kAhead; ++m) {
                    const int e_m = m == 0 ? e_row0 : (m == 1 ? e_row1 : (m == 2 ? e_row2 : e_row3));
                    e_pre[m] = m < ns ? e_m : 0;
                    const bool wall = (e_pre[m] & kWallBit) != 0;
                    const int k = m < ns ? (e_pre[m] & (kWallBit - 1)) : i;
                    const double2 *pp = (wall ? w.pos : (const double2 *)s.pos) + k;
                    p_pre[m] = *pp;
                    v_pre[m] = *(wall ? &w.a[k].x : &pp->x);
                }
                requests_issued();
#pragma unroll
                for (int m = 0; m < kAhead; ++m)
                    if (m < rows) test(m < ns, e_pre[m], p_pre[m], v_pre[m]);
            }
            for (int m = kRowsAhead<LPP> ? kAhead : 0; m < rows; ++m) {
                int e = 0;
                double2 pj = make_double2(0.0, 0.0);
                double Volw = 0.0;
                if (m < ns) {
                    e = m == 0 ? e_row0 : (m == 1 ? e_row1 : t.sl_idx[(size_t)m * t.nl_stride + tid]);
                    const bool wall = (e & kWallBit) != 0;
                    const int k = e & (kWallBit - 1);
                    pj = (wall ? w.pos : (const double2 *)s.pos)[k];
                    Volw = wall ? w.a[k].x : 0.0;  // requested with the position, not after the distance test
                }
                test(m < ns, e, pj, Volw);
            }
            if (cnt > t.nl_cap * LPP) { atomicOr(t.flags, 1); cnt = t.nl_cap * LPP; }
            cnt_fl = min(cnt_fl, cnt);
        }
    } else if (active) {
        const double xi = pi.x, yi = pi.y;
        const int cx = ci / g.ncy, cy = ci - cx * g.ncy;
        const int cylo = max(cy - 1, 0), cyhi = min(cy + 1, g.ncy - 1);
        const bool near_wall = w.row_any[cy] != 0;
        // cell ranges of the three columns, fluid and wall, requested together; each set is walked as one range (ranges_index)
        int lo[3], hi[3], wlo[3], whi[3];
#pragma unroll
        for (int ox = -1; ox <= 1; ++ox) {
            int col;
            const bool ok = neighbour_column(g, cx, ox, col);
            const int c0 = col * g.ncy + cylo, c1 = col * g.ncy + cyhi + 1;
            lo[ox + 1] = ok ? s.start[c0] : 0;
            hi[ox + 1] = ok ? s.start[c1] : 0;
            wlo[ox + 1] = ok ? w.start[c0] : 0;
            whi[ox + 1] = ok ? w.start[c1] : 0;
        }
        const int n0 = hi[0] - lo[0], n1 = hi[1] - lo[1], n2 = hi[2] - lo[2];
        const int nfl = n0 + n1 + n2;
        for (int vb = 0; vb < nfl; vb += LPP) {
            const int v = vb + sub;
            bool acc = false, wide = false;
            int k = 0;
            if (v < nfl) {
                k = ranges_index(lo[0], lo[1], lo[2], n0, n1, v);
                const double2 pj = s.pos[k];
                const double dx = pair_dx<LPP>(g, xi - pj.x), dy = yi - pj.y;
                const double r2 = dx * dx + dy * dy;
                if (r2 > kR2Min && r2 < ph.kc.rcut2) {
                    acc = true;
                    s_in += spline_W_sel(ph.kc, r2 * rsqrt_nr(r2));
                }
                wide = r2 > kR2Min && r2 < t.sl_rcut2;
            }
            push(acc, k);
            if (record) push_super(wide, k);
        }
        cnt_fl = cnt;
        scnt_fl = scnt;
        if (near_wall) {
            const int w0 = whi[0] - wlo[0], w1 = whi[1] - wlo[1], w2 = whi[2] - wlo[2];
            const int nwl = w0 + w1 + w2;
            for (int vb = 0; vb < nwl; vb += LPP) {
                const int v = vb + sub;
                bool acc = false, wide = false;
                int k = 0;
                if (v < nwl) {
                    k = ranges_index(wlo[0], wlo[1], wlo[2], w0, w1, v);
                    const double2 pj = w.pos[k];
                    const double Volj = w.a[k].x;  // requested with the position, not after the distance test
                    const double dx = pair_dx<LPP>(g, xi - pj.x), dy = yi - pj.y;
                    const double r2 = dx * dx + dy * dy;
                    if (r2 > kR2Min && r2 < ph.kc.rcut2) {
                        acc = true;
                        s_ct += spline_W_sel(ph.kc, r2 * rsqrt_nr(r2)) * Volj;
                    }
                    wide = r2 > kR2Min && r2 < t.sl_rcut2;
                }
                push(acc, k | kWallBit);
                if (record) push_super(wide, k | kWallBit);
            }
        }
        if (cnt > t.nl_cap * LPP) { atomicOr(t.flags, 1); cnt = t.nl_cap * LPP; }
        cnt_fl = min(cnt_fl, cnt);
        if (record && scnt > t.sl_cap * LPP) { atomicOr(t.flags, 1); scnt = t.sl_cap * LPP; }
        scnt_fl = min(scnt_fl, scnt);
    }
    // cnt is the particle's neighbour count (identical in all lanes of the group)
    if (tid < t.nl_stride) t.nl_cnt[tid] = list_row_counts<LPP>(cnt, cnt_fl, sub);
    if (record && tid < t.nl_stride) t.sl_cnt[tid] = list_row_counts<LPP>(scnt, scnt_fl, sub);
    s_in = group_sum<LPP>(s_in);
    s_ct = group_sum<LPP>(s_ct);
    if (active && sub == 0) store_density(ph, t, i, s_in, s_ct, mass_i, drho_i, dt, half);
}

// Slabs, frozen steps: pass A of the next step in two launches, so that the halo exchange of this step hides behind the
// first.  part = 1: only the INTERIOR workgroups -- every particle of theirs binned in the columns [own_c0 + 1, own_c1 - 1),
// so that their candidates (one column either side) and the tiles they stage lie in owned columns, which the incoming message
// does not touch -- launched right behind k_slab_pack3; part = 2: the rest (boundary workgroups), behind k_slab_unpack3.
// part rides in the walk kernels' cond_fresh argument: bits 4 and up (kPassPartShift).
constexpr int kPassPartShift = 4;
template <int LPP, int BLK = kBlock>
__device__ __forceinline__ bool slab_part_skips(const Grid &g, const FluidSet &s, int blk, int part)
{
    const int first = blk * (BLK / LPP), last = first + BLK / LPP - 1;
    const int lo = s.start[(g.own_c0 + 1) * g.ncy], hi = s.start[(g.own_c1 - 1) * g.ncy];
    const bool interior = first >= lo && last < hi;
    return interior != (part == 1);
}

// cond_fresh (dynamic contexts launch both MODE 1 and MODE 2 on every step): -1 = always run, 1 = only on a fresh grid,
// 0 = only on a grid that is not fresh.  Measured at 6 M particles, average pass A per step: two launches of which one
// returns 786 us; one kernel holding both bodies 891 us (it runs at the register budget of the bigger one); one
// body deciding per candidate at run time 795 us.
template <int LPP, int MODE, int BLK = kBlock>
__device__ __forceinline__ void density_pass(const Clock *clk, int q, const Grid &g, const Phys &ph, const FluidSet &s,
                                             const FluidTmp &t, const Walls &w, int cond_fresh, int nblk)
{
    const int part = cond_fresh >= 0 ? cond_fresh >> kPassPartShift : 0;
    if (part) cond_fresh &= (1 << kPassPartShift) - 1;
    if (cond_fresh >= 0 && (clk->fresh != 0) != (cond_fresh != 0)) return;
    if (MODE == 2 && part && slab_part_skips<LPP, BLK>(g, s, xcd_block((int)blockIdx.x, nblk), part)) return;
    density_body<LPP, MODE, BLK>(clk, q, g, ph, s, t, w, (int)blockIdx.x, nblk, true);
}
template <int LPP, int MODE>
__global__ __launch_bounds__(kBlock) void k_density(const Clock *clk, int q, Grid g, Phys ph,
                                                    FluidSet s, FluidTmp t, Walls w, int cond_fresh)
{
    density_pass<LPP, MODE>(clk, q, g, ph, s, t, w, cond_fresh, (int)gridDim.x);
}
// The walk at 16 / 32 lanes per particle with leading arguments (shape: cond_fresh), in workgroups of BLK threads
template <int LPP, int BLK = kBlock>
__global__ __launch_bounds__(BLK) void k_density_walk(const Clock *clk, int q, int shape, int *sl_cnt, int *sl_idx, int nl_stride,
                                                         int cap, double2 *pos, double *mass, Grid g, Phys ph, FluidSet s,
                                                         FluidTmp t, Walls w)
{
    t.sl_cnt = sl_cnt; t.sl_idx = sl_idx; t.nl_stride = nl_stride; t.cap = cap; s.pos = pos; s.mass = mass;
    density_pass<LPP, 2, BLK>(clk, q, g, ph, s, t, w, shape_flag(shape), shape_blocks(shape));
}
// Contexts whose re-binning step is folded into passes CD and E (k_forces_hist, k_continuity_rebin): nobody counts the cell
// histogram back down there (k_scatter's atomicSub did), and the tail workgroup of pass E advances the clock while the other
// workgroups still read it.  The cell sweep of the step after a re-binning -- always the next launch that runs -- clears it.
// (idle slot or not: a histogram is taken and used up inside one step slot, never across this launch)
template <int LPP>
__global__ __launch_bounds__(kBlock) void k_density_zero(const Clock *clk, int q, Grid g, Phys ph,
                                                         FluidSet s, FluidTmp t, Walls w, int cond_fresh)
{
    for (int k = (int)(blockIdx.x * kBlock + threadIdx.x); k < g.ncells; k += (int)(gridDim.x * kBlock)) t.count[k] = 0;
    density_pass<LPP, 1>(clk, q, g, ph, s, t, w, cond_fresh, (int)gridDim.x);
}
// (the "_b" wrappers take the run-time arguments of their single-channel kernels as run-time arguments too: a constant there
//  would let the compiler merge the bodies' blocks differently, and its fused multiply-adds -- so the last bits -- with them)
template <int LPP, int MODE>
__global__ __launch_bounds__(kBlock) void k_density_b(Members mb, int q, Grid g, FluidSet s, FluidTmp t, Walls w, int cond_fresh)
{
    const int m = (int)blockIdx.y;
    const Phys ph = mb.ph[m];
    density_pass<LPP, MODE>(mb.clk + m, q, g, ph, member_set(mb, m, s), member_tmp(mb, m, t), w, cond_fresh, (int)gridDim.x);
}

// ---------------------------------------------------------------------------------------------
// pass B: kernel-gradient-correction matrix A -> blended pseudo-inverse B
// (mex/sph_physics_mex.c:239-366).  Fluid and wall neighbours contribute the same term (Vol_j of a wall
// particle is m/rho0), so the walk does not branch.
// ---------------------------------------------------------------------------------------------
// finish_half: pass A of this step ran inside the previous step's fused launch and left {p_half, rho_half} open
template <int LPP, int BLK = kBlock>
__device__ __forceinline__ void kgc_pass(const Clock *clk, int q, const Grid &g, const Phys &ph, const FluidSet &s,
                                         const FluidTmp &t, const Walls &w, int finish_half, int nblk)
{
    SPHX_PASS_INDEX_BLK((int)blockIdx.x, nblk, BLK);
    ListHead head;
    if (kRowsAhead<LPP>) {
        head.request(clk, q, t.nl_cnt, t.nl_idx, t.nl_stride, tid);
        SPHX_ARGS_BATCH("s"(s.pos), "s"(s.drho), "s"(t.a), "s"(t.B), "s"(t.cap), "s"(t.vol), "s"(w.pos), "s"(w.a), "s"(g.DL),
                        "s"(g.half_DL), "s"(ph.kc.h), "s"(ph.kc.inv_h), "s"(ph.kc.sigma_over_h), "s"(ph.rho0), "s"(ph.p0), "s"(head.run),
                        "s"(head.n), "s"(head.dt));
    }
    constexpr bool kOwn = kRowsAhead<LPP>;  // (own_slot: no test around the own records)
    const int io = own_slot<LPP>(i, t.cap);
    const double2 pi = (kOwn || in_cap) ? s.pos[io] : make_double2(0.0, 0.0);
    const bool closes = finish_half && (kOwn || (in_cap && sub == 0));
    const double4 a_own = closes ? t.a[io] : make_double4(0.0, 0.0, 0.0, 0.0);
    const double drho_own = closes ? s.drho[io] : 0.0;
    const int nn_all = list_rows(kRowsAhead<LPP> ? head.packed : t.nl_cnt[tid]);
    const FirstRows<LPP> first = kRowsAhead<LPP> ? FirstRows<LPP>(head.e0, head.e1) : FirstRows<LPP>(t.nl_idx, t.nl_stride, tid);
    const double dt = kRowsAhead<LPP> ? head.dt : clk->dt;
    const int run_q = kRowsAhead<LPP> ? head.run : clk->run[q], n_now = kRowsAhead<LPP> ? head.n : clk->n;
    if (kRowsAhead<LPP>) requests_issued();
    if (!run_q) return;
    const bool active = i < n_now;
    double a11 = 0.0, a12 = 0.0, a21 = 0.0, a22 = 0.0;
    if (active) {
        const double xi = pi.x, yi = pi.y;
        auto fetch = [&](int e, int k, double2 &pj, double &Volj) {
            const bool wall = (e & kWallBit) != 0;
            pj = (wall ? w.pos : (const double2 *)s.pos)[k];
            Volj = *(wall ? &w.a[k].x : (const double *)&t.vol[k]);
        };
        auto term = [&](const double2 pj, double Volj) {
            kgc_moment_add(ph.kc, pair_dx<LPP>(g, xi - pj.x), yi - pj.y, Volj, a11, a12, a21, a22);
        };
        if (kRowsAhead<LPP>) {  // rows 0 and 1: both rows' records in one wave
            const int e0 = nn_all > 0 ? first.e0 : 0, e1 = nn_all > 1 ? first.e1 : 0;
            double2 p0, p1;
            double V0, V1;
            fetch(e0, nn_all > 0 ? (e0 & (kWallBit - 1)) : i, p0, V0);
            fetch(e1, nn_all > 1 ? (e1 & (kWallBit - 1)) : i, p1, V1);
            requests_issued();
            if (nn_all > 0) term(p0, V0);
            if (nn_all > 1) term(p1, V1);
        }
        for (int m = kRowsAhead<LPP> ? 2 : 0; m < nn_all; ++m) {
            const int e = first.row(m, t.nl_idx, t.nl_stride, tid);
            double2 pj;
            double Volj;
            fetch(e, e & (kWallBit - 1), pj, Volj);
            term(pj, Volj);
        }
    }
    a11 = group_sum<LPP>(a11);
    a12 = group_sum<LPP>(a12);
    a21 = group_sum<LPP>(a21);
    a22 = group_sum<LPP>(a22);
    if (active && sub == 0) {
        const Mat2 B = kgc_from_A(a11, a12, a21, a22);
        t.B[i] = make_double4(B.m11, B.m12, B.m21, B.m22);
        if (finish_half) {
            double rhoh, p_half;
            half_state(ph, a_own.w, drho_own, dt, rhoh, p_half);
            t.a[i] = make_double4(a_own.x, p_half, rhoh, a_own.w);
        }
    }
}
template <int LPP, int BLK = kBlock>
__global__ __launch_bounds__(BLK) void k_kgc(const Clock *clk, int q, int shape, int *nl_cnt, int *nl_idx, int nl_stride, int cap,
                                                double2 *pos, double4 *a, Grid g, Phys ph, FluidSet s, FluidTmp t, Walls w)
{
    t.nl_cnt = nl_cnt; t.nl_idx = nl_idx; t.nl_stride = nl_stride; t.cap = cap; s.pos = pos; t.a = a;  // shape: finish_half
    kgc_pass<LPP, BLK>(clk, q, g, ph, s, t, w, shape_flag(shape), shape_blocks(shape));
}
template <int LPP>
__global__ __launch_bounds__(kBlock) void k_kgc_b(Members mb, int q, Grid g, FluidSet s, FluidTmp t, Walls w, int finish_half)
{
    const int m = (int)blockIdx.y;
    const Phys ph = mb.ph[m];
    kgc_pass<LPP>(mb.clk + m, q, g, ph, member_set(mb, m, s), member_tmp(mb, m, t), w, finish_half, (int)gridDim.x);
}

// ---------------------------------------------------------------------------------------------
// pass CD: viscous force (+gravity) [sph_physics_mex.c:469-545, SPH_Poiseuille.m:392], transport
// shift [:636-710], Riemann pressure force of integration_1st [:870-957], velocity kick
// [:1400-1408] and both position half-drifts [:863-864,:1066-1069] + periodic wrap
// [SPH_Poiseuille.m:570-577].  One walk over the list serves all three operators because they share
// e, dW, B_i+B_j; the wall entries are visited a second time because the wall pressure needs the
// complete viscous+gravity force of the particle first (p_wall uses force_prior_i, :931-934).
// ---------------------------------------------------------------------------------------------
// later = 1 (dual-rate loop, inner sub-steps after the first): the pressure part only -- viscous force and gravity
// are those of the first sub-step (t.fp), there is no transport shift, the particle moves on from t.posn; pair geometry
// stays that of the start of the outer step (s.pos), velocities are the latest ones (s.vel = the previous sub-step's).
// HIST (the step that re-bins, contexts with a folded re-binning step, see k_continuity_rebin): the lead lane holds the new
// position, so the cell histogram is taken here instead of in pass E, which then finds it complete.  A particle that lands
// further than one cell from where it was binned raises the grid flag: pass E of this step looks for the members of a new cell
// only that far (rebin_near), and its tail workgroup turns the flag into SPHX_ERR_GRID.
// BLK: the threads of the workgroup (HIST stays at 256)
// WP (kept wall pairs, 16 / 32 lanes per particle; WP = false: SPHX_DEBUG_SWITCHES=no_wall_paths, the pair built twice as
// before): a prefetched wall row keeps what wall_pair made of it -- in place of the position and the volume -- and the second
// loop forms the wall pressure from that (wall_pressure_from) instead of building the pair again.  Rows beyond the prefetched
// ones are read and built again as before.  (later: the first loop builds the pair of a prefetched wall row all the same and
// leaves out its viscous and transport terms.)
template <int LPP, bool HIST = false, int BLK = kBlock, bool WP = true>
__device__ __forceinline__ void forces_pass(const Clock *clk, int q, const Grid &g, const Phys &ph, const FluidSet &s,
                                            const FluidTmp &t, const Walls &w, int later, int nblk)
{
    SPHX_PASS_INDEX_BLK((int)blockIdx.x, nblk, BLK);
    ListHead head;
    if (kRowsAhead<LPP>) {
        head.request(clk, q, t.nl_cnt, t.nl_idx, t.nl_stride, tid);
        SPHX_ARGS_BATCH("s"(s.pos), "s"(s.vel), "s"(t.a), "s"(t.B), "s"(s.mass), "s"(t.cap), "s"(s.posb), "s"(t.fp), "s"(t.posn),
                        "s"(w.pos), "s"(w.a), "s"(g.DL), "s"(g.half_DL), "s"(ph.kc.h), "s"(ph.kc.inv_h), "s"(ph.kc.sigma_over_h),
                        "s"(ph.mu), "s"(ph.c_f), "s"(ph.g), "s"(ph.tc), "s"(ph.DL), "s"(head.run), "s"(head.n), "s"(head.dt));
    }
    constexpr bool kOwn = kRowsAhead<LPP>;  // (own_slot: no test around the own records)
    const int io = own_slot<LPP>(i, t.cap);
    const bool own = kOwn || in_cap, own_lead = kOwn || (in_cap && sub == 0);
    const int c_binned = (HIST && own_lead) ? s.cell[io] : 0;
    const double2 pi = own ? s.pos[io] : make_double2(0.0, 0.0);
    const double2 vi = own ? s.vel[io] : make_double2(0.0, 0.0);
    const double4 ai = own ? t.a[io] : make_double4(1.0, 0.0, 0.0, 0.0);
    const double4 Bi = own ? t.B[io] : make_double4(1.0, 0.0, 0.0, 1.0);
    const double mi = own ? s.mass[io] : 1.0;
    const int nn_all = list_rows(kRowsAhead<LPP> ? head.packed : t.nl_cnt[tid]);
    const FirstRows<LPP> first = kRowsAhead<LPP> ? FirstRows<LPP>(head.e0, head.e1) : FirstRows<LPP>(t.nl_idx, t.nl_stride, tid);
    const bool tracked = s.posb != nullptr;
    const double2 pb = (tracked && own_lead) ? s.posb[io] : make_double2(0.0, 0.0);
    const double2 fp_own = (later && own) ? t.fp[io] : make_double2(0.0, 0.0);
    const double2 p_now = (later && own_lead) ? t.posn[io] : make_double2(0.0, 0.0);
    const double dt = kRowsAhead<LPP> ? head.dt : clk->dt;
    const int run_q = kRowsAhead<LPP> ? head.run : clk->run[q], n_now = kRowsAhead<LPP> ? head.n : clk->n;
    if (kRowsAhead<LPP>) requests_issued();
    if (!run_q) return;
    const bool active = i < n_now;
    const double h = ph.kc.h;
    double ax = 0.0, ay = 0.0, ix = 0.0, iy = 0.0, px = 0.0, py = 0.0, d2 = 0.0;
    const double xi = pi.x, yi = pi.y, vxi = vi.x, vyi = vi.y;
    const double Voli = ai.x, p_i = ai.y, rhoh_i = ai.z;
    const double b11i = Bi.x, b12i = Bi.y, b21i = Bi.z, b22i = Bi.w;
    int first_wall = 1 << 20;  // wall neighbours are appended behind the fluid ones: this lane's rows >= first_wall
    int h_cell = -1;           // HIST: the new cell of the lead lane's particle
    // kRowsAhead: rows 0 and 1 of the lane -- {position, a} of either kind of neighbour, velocity and B of a fluid one (a wall
    // row asks for the particle's own) -- are requested in one wave; the wall rows among them keep position and volume in
    // registers for the second wall loop, which otherwise reads its entries and records again behind the group sums
    double2 pj0 = make_double2(0.0, 0.0), pj1 = pj0;
    double4 aj0 = make_double4(0.0, 0.0, 0.0, 0.0), aj1 = aj0;
    auto fluid_term = [&](const double2 pj, const double2 vj, const double4 aj, const double4 Bj) {
        const auto [r, ex, ey] = pair_geom(pair_dx<LPP>(g, xi - pj.x), yi - pj.y);
        const double dW = spline_dW_in(ph.kc, r);
        const double Volj = aj.x;
        const double tx = (b11i + Bj.x) * ex + (b12i + Bj.y) * ey;
        const double ty = (b21i + Bj.z) * ex + (b22i + Bj.w) * ey;
        const double eBe = ex * tx + ey * ty;
        const double vxj = vj.x, vyj = vj.y;
        const double dWVj = dW * Volj;
        if (!later) {
            // viscous
            const double coeff = eBe * ph.mu * dWVj * rcp_nr(r + 0.01 * h);
            ax += coeff * (vxi - vxj);
            ay += coeff * (vyi - vyj);
            // transport
            ix -= dWVj * tx;
            iy -= dWVj * ty;
        }
        // pressure (Riemann-dissipated face pressure)
        const double p_j = aj.y;
        const double rho_bar = 0.5 * (rhoh_i + aj.z);
        const double un_l = vxi * ex + vyi * ey, un_r = vxj * ex + vyj * ey;
        const double beta = riemann_beta(un_l, un_r, ph.c_f);
        const double p_avg = 0.5 * (p_i + p_j);
        const double p_star = p_avg + 0.5 * beta * rho_bar * (un_l - un_r);
        const double p_face = 0.5 * (p_avg + p_star);
        px -= (p_face * tx) * dWVj;
        py -= (p_face * ty) * dWVj;
    };
    auto wall_term = [&](const double2 pj, const double4 wj) {
        const WallPair wp = wall_pair(ph.kc, pair_dx<LPP>(g, xi - pj.x), yi - pj.y, wj.x, Bi);
        const double coeff = 4.0 * wp.eBe * ph.mu * wp.dWVj * rcp_nr(wp.r + 0.01 * h);
        ax += coeff * (vxi - wj.y);
        ay += coeff * (vyi - wj.z);
        ix -= 2.0 * wp.dWVj * wp.tx;
        iy -= 2.0 * wp.dWVj * wp.ty;
    };
    // (wall_term in two halves, for a prefetched wall row whose pair is kept for the second loop)
    auto wall_pair_of = [&](const double2 pj, const double4 wj) {
        return wall_pair(ph.kc, pair_dx<LPP>(g, xi - pj.x), yi - pj.y, wj.x, Bi);
    };
    auto wall_apply = [&](const WallPair &wp, const double4 wj) {
        const double coeff = 4.0 * wp.eBe * ph.mu * wp.dWVj * rcp_nr(wp.r + 0.01 * h);
        ax += coeff * (vxi - wj.y);
        ay += coeff * (vyi - wj.z);
        ix -= 2.0 * wp.dWVj * wp.tx;
        iy -= 2.0 * wp.dWVj * wp.ty;
    };
    constexpr bool kKeep = kRowsAhead<LPP> && WP;
    bool kept0 = false, kept1 = false;  // kKeep: the prefetched row is a wall row, and this is its pair
    WallPair wp0, wp1;
    if (kKeep && active) {  // both kinds of row as below; a prefetched wall row keeps its pair, not its position and volume
        const bool has0 = nn_all > 0, has1 = nn_all > 1;
        const bool w0 = has0 && (first.e0 & kWallBit) != 0, w1 = has1 && (first.e1 & kWallBit) != 0;
        const int k0 = has0 ? (first.e0 & (kWallBit - 1)) : i, k1 = has1 ? (first.e1 & (kWallBit - 1)) : i;
        const int kf0 = w0 ? i : k0, kf1 = w1 ? i : k1;
        const double2 qj0 = (w0 ? w.pos : (const double2 *)s.pos)[k0];
        const double4 cj0 = (w0 ? w.a : (const double4 *)t.a)[k0];
        const double2 vj0 = s.vel[kf0];
        const double4 Bj0 = t.B[kf0];
        const double2 qj1 = (w1 ? w.pos : (const double2 *)s.pos)[k1];
        const double4 cj1 = (w1 ? w.a : (const double4 *)t.a)[k1];
        const double2 vj1 = s.vel[kf1];
        const double4 Bj1 = t.B[kf1];
        requests_issued();
        if (has0) {
            if (!w0) fluid_term(qj0, vj0, cj0, Bj0);
            else {
                kept0 = true;
                wp0 = wall_pair_of(qj0, cj0);
                if (!later) wall_apply(wp0, cj0);  // (wall entries contribute to the pressure part in the second loop only)
            }
        }
        if (has1) {
            if (!w1) fluid_term(qj1, vj1, cj1, Bj1);
            else {
                kept1 = true;
                wp1 = wall_pair_of(qj1, cj1);
                if (!later) wall_apply(wp1, cj1);
            }
        }
        for (int m = 2; m < nn_all; ++m) {
            const int e = t.nl_idx[(size_t)m * t.nl_stride + tid];
            const int k = e & (kWallBit - 1);
            if (!(e & kWallBit)) {
                const double2 pj = s.pos[k], vj = s.vel[k];
                const double4 aj = t.a[k], Bj = t.B[k];
                fluid_term(pj, vj, aj, Bj);
            } else {
                first_wall = min(first_wall, m);
                if (later) continue;
                const double2 pj = w.pos[k];
                const double4 wj = w.a[k];
                wall_term(pj, wj);
            }
        }
    }
    if (!kKeep && active) {
        if (kRowsAhead<LPP>) {
            const bool has0 = nn_all > 0, has1 = nn_all > 1;
            const bool w0 = has0 && (first.e0 & kWallBit) != 0, w1 = has1 && (first.e1 & kWallBit) != 0;
            const int k0 = has0 ? (first.e0 & (kWallBit - 1)) : i, k1 = has1 ? (first.e1 & (kWallBit - 1)) : i;
            const int kf0 = w0 ? i : k0, kf1 = w1 ? i : k1;
            pj0 = (w0 ? w.pos : (const double2 *)s.pos)[k0];
            aj0 = (w0 ? w.a : (const double4 *)t.a)[k0];
            const double2 vj0 = s.vel[kf0];
            const double4 Bj0 = t.B[kf0];
            pj1 = (w1 ? w.pos : (const double2 *)s.pos)[k1];
            aj1 = (w1 ? w.a : (const double4 *)t.a)[k1];
            const double2 vj1 = s.vel[kf1];
            const double4 Bj1 = t.B[kf1];
            requests_issued();
            if (has0) {
                if (!w0) fluid_term(pj0, vj0, aj0, Bj0);
                else {
                    first_wall = 0;
                    if (!later) wall_term(pj0, aj0);  // (wall entries contribute to the pressure part in the second loop only)
                }
            }
            if (has1) {
                if (!w1) fluid_term(pj1, vj1, aj1, Bj1);
                else {
                    first_wall = min(first_wall, 1);
                    if (!later) wall_term(pj1, aj1);
                }
            }
        }
        for (int m = kRowsAhead<LPP> ? 2 : 0; m < nn_all; ++m) {
            const int e = first.row(m, t.nl_idx, t.nl_stride, tid);
            const int k = e & (kWallBit - 1);
            if (!(e & kWallBit)) {
                const double2 pj = s.pos[k], vj = s.vel[k];
                const double4 aj = t.a[k], Bj = t.B[k];
                fluid_term(pj, vj, aj, Bj);
            } else {
                first_wall = min(first_wall, m);
                if (later) continue;  // (wall entries contribute to the pressure part in the second loop only)
                const double2 pj = w.pos[k];
                const double4 wj = w.a[k];
                wall_term(pj, wj);
            }
        }
    }
    ax = group_sum<LPP>(ax);
    ay = group_sum<LPP>(ay);
    ix = group_sum<LPP>(ix);
    iy = group_sum<LPP>(iy);
    const double fpx = later ? fp_own.x : ax * Voli + mi * ph.g;  // + gravity, SPH_Poiseuille.m:392
    const double fpy = later ? fp_own.y : ay * Voli;
    const double inv_m = rcp_nr(mi);
    if (active) {
        const double acx = fpx * inv_m, acy = fpy * inv_m;
        auto wall_pressure = [&](const double2 pj, double Volw) {
            wall_pressure_add(ph.kc, pair_dx<LPP>(g, xi - pj.x), yi - pj.y, Volw, Bi, acx, acy, p_i, rhoh_i, px, py);
        };
        if (kKeep) {  // (the prefetched rows from their kept pairs; first_wall counts from row 2 here)
            if (kept0) wall_pressure_from(wp0, acx, acy, p_i, rhoh_i, px, py);
            if (kept1) wall_pressure_from(wp1, acx, acy, p_i, rhoh_i, px, py);
        } else if (kRowsAhead<LPP>) {  // (the prefetched rows from registers; lanes with more wall rows read the rest again)
            if (first_wall <= 0 && nn_all > 0) wall_pressure(pj0, aj0.x);
            if (first_wall <= 1 && nn_all > 1) wall_pressure(pj1, aj1.x);
        }
        for (int m = kRowsAhead<LPP> ? max(first_wall, 2) : first_wall; m < nn_all; ++m) {
            const int k = t.nl_idx[(size_t)m * t.nl_stride + tid] & (kWallBit - 1);
            wall_pressure(w.pos[k], w.a[k].x);
        }
    }
    px = group_sum<LPP>(px);
    py = group_sum<LPP>(py);
    if (active && sub == 0) {
        const double fx = px * Voli, fy = py * Voli;
        const double vxn = vxi + (fpx + fx) * inv_m * dt;
        const double vyn = vyi + (fpy + fy) * inv_m * dt;
        double sx = 0.0, sy = 0.0;
        if (!later) transport_shift(ix, iy, h, ph.tc, sx, sy);
        double xo = later ? p_now.x : xi + sx, yo = later ? p_now.y : yi + sy;
        xo += 0.5 * dt * vxi;
        yo += 0.5 * dt * vyi;
        xo += 0.5 * dt * vxn;
        yo += 0.5 * dt * vyn;
        if (tracked) d2 = tracked_drift2(g, s, i, xo, yo, pb);
        t.posn[i] = make_double2(g.periodic ? wrap_x(xo, ph.DL) : xo, yo);  // a slab wraps when particles change owner
        t.veln[i] = make_double2(vxn, vyn);
        if (!later) t.fp[i] = make_double2(fpx, fpy);
        t.f[i] = make_double2(fx, fy);
        if (HIST) {
            int cx, cy;
            cell_of(g, g.periodic ? wrap_x(xo, ph.DL) : xo, yo, cx, cy);
            h_cell = cx * g.ncy + cy;
            t.cellid[i] = h_cell;
            if (!rebin_near(g, c_binned, h_cell)) atomicOr(t.flags, 1);
        }
    }
    static_assert(!HIST || BLK == kBlock, "the histogram epilogue is written for 256 threads");
    __shared__ int s_hc[HIST ? kBlock / LPP : 1];
    if (HIST && sub == 0) s_hc[threadIdx.x / LPP] = h_cell;
    store_block_drift<BLK>(t, blk, d2);  // (its barrier also closes s_hc)
    // HIST: a workgroup's particles are neighbours in the old ordering and land in two or three cells: one atomic per cell and
    // workgroup instead of one per particle (fifteen particles of a cell, in as many workgroups on eight L2s, queue up on one word)
    if (HIST && threadIdx.x < kBlock / LPP) {
        const int c = s_hc[threadIdx.x];
        int same = 0;
        bool first = true;
#pragma unroll
        for (int k = 0; k < kBlock / LPP; ++k) {
            const bool eq = s_hc[k] == c;
            same += eq ? 1 : 0;
            if (eq && k < (int)threadIdx.x) first = false;
        }
        if (c >= 0 && first) atomicAdd(&t.count[c], same);
    }
}
template <int LPP, int BLK = kBlock, bool WP = true>
__global__ __launch_bounds__(BLK) void k_forces(const Clock *clk, int q, int shape, int *nl_cnt, int *nl_idx, int nl_stride, int cap,
                                                   double2 *pos, double2 *vel, Grid g, Phys ph, FluidSet s, FluidTmp t, Walls w)
{
    t.nl_cnt = nl_cnt; t.nl_idx = nl_idx; t.nl_stride = nl_stride; t.cap = cap; s.pos = pos; s.vel = vel;  // shape: later
    forces_pass<LPP, false, BLK, WP>(clk, q, g, ph, s, t, w, shape_flag(shape), shape_blocks(shape));
}
template <int LPP, bool WP = true>
__global__ __launch_bounds__(kBlock) void k_forces_hist(const Clock *clk, int q, int shape, int *nl_cnt, int *nl_idx, int nl_stride,
                                                        int cap, double2 *pos, double2 *vel, Grid g, Phys ph, FluidSet s, FluidTmp t,
                                                        Walls w)
{
    t.nl_cnt = nl_cnt; t.nl_idx = nl_idx; t.nl_stride = nl_stride; t.cap = cap; s.pos = pos; s.vel = vel;
    forces_pass<LPP, true, kBlock, WP>(clk, q, g, ph, s, t, w, shape_flag(shape), shape_blocks(shape));
}
template <int LPP, bool WP = true>
__global__ __launch_bounds__(kBlock) void k_forces_b(Members mb, int q, Grid g, FluidSet s, FluidTmp t, Walls w, int later)
{
    const int m = (int)blockIdx.y;
    const Phys ph = mb.ph[m];
    forces_pass<LPP, false, kBlock, WP>(mb.clk + m, q, g, ph, member_set(mb, m, s), member_tmp(mb, m, t), w, later, (int)gridDim.x);
}

// =================================================================================================
// Large channels (few lanes per particle, LPP <= 8): the "_w" variants of passes B, CD and E.
// Counters of the round-1 kernels at 0.5-6 M particles: VALU 55-75 % busy, texture addresser 60-90 %, and a wave
// spending ~5 x its own issue time in flight -- every trip of the walk was two dependent memory round trips
// (list entry -> neighbour records) followed by 55-100 VALU instructions under per-entry fluid/wall and kernel-piece
// branches.  Here
//   * list entries run three rows ahead of their use (one register each): one round trip per trip;
//   * fluid and wall neighbours have loops of their own (fluid entries come first in a lane's rows, pass A stores both
//     row counts) -- no per-entry branch, no pointer selects;
//   * the minimum-image fold runs only in wavefronts holding a particle near the periodic seam;
//   * the kernel derivative is branch-free, 1/sqrt and the viscous division are Newton-refined hardware estimates;
//   * the force pass can stage its tile's neighbourhood in LDS (TILE > 0), see k_forces_w.
// Small channels keep the compact kernels above: at a few thousand particles a pass is a chain of dependent round
// trips and code size (instruction-cache fill per launch) matters more than instruction count.
// =================================================================================================

// Large-channel kernels are launched for the CAPACITY of the arrays; a workgroup whose first particle lies beyond the
// current population has nothing to do.  Its lanes used to request their own records like everybody else before looking
// at the clock (the latency trick of the small channels) -- on a slab, whose capacity holds 15-20 % of slack, that was
// 15-20 % more waves going through every pass's prologue.
// (only where there is slack -- FluidTmp::has_slack: the check is a look at the clock before anything else is requested)
template <int LPP>
__device__ __forceinline__ bool beyond_population(const Clock *clk, const FluidTmp &t, int blk)
{
    return t.has_slack && blk * (kBlock / LPP) >= clk->n;
}

// A neighbour's x can be a period away from the particle's only if one of them was binned in the first or last cell
// column and has since been wrapped; particles whose x lies within 2.5 columns of either end of the period cover every
// such pair (a column is wider than the skin, so a particle binned in column <= 1 is still left of 2.5 columns).
__device__ __forceinline__ bool near_seam(const Grid &g, double x)
{
    const double w = 2.5 / g.inv_csx;
    return g.periodic && (x < w || x > g.DL - w);
}

// Rows [0, rows_fl) of this lane's list column hold fluid neighbours as index differences, two rows per word (nl_pk):
// body(i + d) for each, the words two ahead of their use (= rows 4-5 ahead).  w0 / w1: the first two words, requested by
// the caller together with the row counts.
// (CODED: body(code), see kSlotCodes)
template <bool CODED = false, typename Body>
__device__ __forceinline__ void walk_fluid_rows(const FluidTmp &t, int tid, int i, int rows_fl, int w0, int w1, Body &&body)
{
    if (rows_fl <= 0) return;
    const int n_words = (rows_fl + 1) >> 1;
    int wa = w0, wb = w1;
    for (int p = 0; p < n_words; ++p) {
        const int wc = p + 2 < n_words ? t.nl_pk[(size_t)(p + 2) * t.nl_stride + tid] : 0;
        body(CODED ? code_lo(wa) : i + delta_lo(wa));
        if (2 * p + 1 < rows_fl) body(CODED ? code_hi(wa) : i + delta_hi(wa));
        wa = wb; wb = wc;
    }
}

// The five forms of a fluid-row walk (large-channel passes B, CD and E), one per wavefront:
//   slot-coded lists: near the periodic seam (fold) / every entry in the tile (all_near, see kFarTileBit) / the general one;
//   index differences: near the seam (wrap and fold) / plain.
// near(code), coded(code), plain(k) fetch the neighbour's record, a struct whose member p is its position; pair(record, dx)
// is the pair term, dx folded where it has to be.  The fetches stay the callers' own: their early returns and LDS-qualified reads
// keep the compiler from merging the tile arm and the global arm into FLAT loads through selected pointers (see k_kgc_w).
template <bool CODED, typename Near, typename Coded, typename Plain, typename Pair>
__device__ __forceinline__ void walk_fluid_forms(const Grid &g, const FluidTmp &t, int tid, int i, int n_now, int rows_fl, int w0, int w1,
                                                 double xi, bool seam, bool all_near, Near &&near, Coded &&coded, Plain &&plain,
                                                 Pair &&pair)
{
    if (CODED && seam)
        walk_fluid_rows<true>(t, tid, i, rows_fl, w0, w1, [&](int e) {
            const auto n = coded(e);
            pair(n, min_image(g, xi - n.p.x));
        });
    else if (CODED && all_near)
        walk_fluid_rows<true>(t, tid, i, rows_fl, w0, w1, [&](int e) {
            const auto n = near(e);
            pair(n, xi - n.p.x);
        });
    else if (CODED)
        walk_fluid_rows<true>(t, tid, i, rows_fl, w0, w1, [&](int e) {
            const auto n = coded(e);
            pair(n, xi - n.p.x);
        });
    else if (seam)
        walk_fluid_rows(t, tid, i, rows_fl, w0, w1, [&](int k) {
            const auto n = plain(wrap_index(k, n_now));
            pair(n, min_image(g, xi - n.p.x));
        });
    else
        walk_fluid_rows(t, tid, i, rows_fl, w0, w1, [&](int k) {
            const auto n = plain(k);
            pair(n, xi - n.p.x);
        });
}

// Rows [rows_fl, rows) hold wall neighbours (only next to a wall): body(k)
template <typename Body>
__device__ __forceinline__ void walk_wall_rows(const FluidTmp &t, int tid, int rows_fl, int rows, Body &&body)
{
    for (int m = rows_fl; m < rows; ++m) body(t.nl_idx[(size_t)m * t.nl_stride + tid] & (kWallBit - 1));
}

// LDS tile of a neighbour pass.  The workgroup's particles are consecutive in cell order -- a run of cells of one
// column -- and every fluid neighbour (or superset candidate) of theirs was binned into the same rows (+-1) of the three
// columns around it: three CONTIGUOUS index ranges.  The first `cap` particles of those ranges (own column first) are
// copied into LDS with coalesced loads once per workgroup and the walk gathers from there; a neighbour outside the staged
// ranges (a tile running across a column end, ranges longer than the tile) is read from global memory, so results do
// not depend on the tile size, bit for bit.  Measured (us per launch, with / without the tile):
//   6 M particles, 2 lanes per particle: forces 607 / 872, KGC 295 / 320, continuity 375 / 452, pass A walk 475 / 434
//   6 M particles, 4 lanes            : forces 673 / 740, KGC 372 / 344, continuity 465 / 446, pass A walk 511 / 451
//   0.5 M particles, 2 lanes          : forces 57.1 / 64.2, KGC 33.1 / 29.0, continuity 36.7 / 37.0, walk 51.8 / 46.6
// -- the fewer lanes share a particle the less its global gathers coalesce, and only records of >= 40 bytes per neighbour
// repay the staging: the force pass always uses the tile, KGC and continuity at 2 lanes per particle on channels that do
// not fit the Infinity Cache, pass A never.  (The 6 M figures without entries running ahead: 803 with / 784 without --
// the exposed round trip was the list entry, not the gather.)
struct TileMap {
    int lo0, lo1, lo2, len0, len1, len2;
    __device__ __forceinline__ int total() const { return len0 + len1 + len2; }
    __device__ __forceinline__ int index(int sl) const  // staged slot -> particle
    {
        return ranges_index(lo0, lo1, lo2, len0, len1, sl);
    }
    __device__ __forceinline__ int slot(int k) const  // particle -> staged slot, -1: not staged
    {
        // three independent selects, not a nested choice: the nested form compiles to a chain of exec-mask branches (five
        // per neighbour in the walks, with their s_nop hazards), this one to compares and v_cndmask
        const unsigned u0 = (unsigned)(k - lo0), u1 = (unsigned)(k - lo1), u2 = (unsigned)(k - lo2);
        int sl = -1;
        sl = u2 < (unsigned)len2 ? len0 + len1 + (int)u2 : sl;
        sl = u1 < (unsigned)len1 ? len0 + (int)u1 : sl;
        sl = u0 < (unsigned)len0 ? (int)u0 : sl;
        return sl;
    }
    __device__ __forceinline__ TileMap capped(int cap) const  // the first `cap` slots of the same layout
    {
        TileMap m = *this;
        m.len0 = min(len0, cap);
        m.len1 = min(len1, cap - m.len0);
        m.len2 = min(len2, cap - m.len0 - m.len1);
        return m;
    }
};
#ifndef SPHX_EXP_N2_PROLOGUE
#define SPHX_EXP_N2_PROLOGUE 0  // measurement builds only (tools/probes/build_variant_lib.sh)
#endif
// MEASUREMENT ONLY: what decoding a layout of 3 + 14 ranges would add to every staged slot (a blocked particle order's tile
// neighbourhood: the strip's own run plus one cell above and below per column).  Fourteen compare / select /
// add steps on values the compiler cannot fold; the result is 0, so the staged data -- and every result -- stay what they are.
__device__ __forceinline__ int n2_prologue_cost(int sl, const TileMap &m)
{
#if SPHX_EXP_N2_PROLOGUE
    int acc = 0;
#pragma unroll
    for (int j = 0; j < 14; ++j) acc = sl >= m.len0 + m.len1 + m.len2 + 1000 + 37 * j ? acc + m.lo0 + j : acc;
    return acc;
#else
    return 0;
#endif
}
// The layout (tile_ranges at capacity kSlotCodes) of every workgroup is worked out ONCE per re-binning, by the cell sweep, and
// kept in FluidTmp::tmap.  Working it out in every pass put two dependent memory round trips (first / last cell of the
// workgroup -> six cell starts) in front of the staging loads, in a prologue that already waits for the clock: the workgroups
// of a compute unit start together and stay in step, so while they all wait nobody computes (6 M particles: a workgroup of
// the force pass lives ~16 us, of which the vector units have work for ~9).  Read here with the workgroup's first requests.
__device__ __forceinline__ TileMap tile_map_of(const FluidTmp &t, int blk)
{
    const int4 lo = reinterpret_cast<const int4 *>(t.tmap)[2 * blk], len = reinterpret_cast<const int4 *>(t.tmap)[2 * blk + 1];
    return TileMap{lo.x, lo.y, lo.z, len.x, len.y, len.z};
}
__device__ __forceinline__ void store_tile_map(const FluidTmp &t, int blk, const TileMap &m)
{
    reinterpret_cast<int4 *>(t.tmap)[2 * blk] = make_int4(m.lo0, m.lo1, m.lo2, 0);
    reinterpret_cast<int4 *>(t.tmap)[2 * blk + 1] = make_int4(m.len0, m.len1, m.len2, 0);
}
// ... cut to a pass's tile size (nothing for a workgroup beyond the population)
template <int LPP>
__device__ __forceinline__ TileMap staged_map(const TileMap &layout, int blk, int n_now, int cap)
{
    if (blk * (kBlock / LPP) >= n_now) return TileMap{0, 0, 0, 0, 0, 0};
    return layout.capped(cap);
}

// Staging a tile: thread x fills slots x and x + kBlock of the staged map tm -- store(slot, load(particle)) -- and the workgroup
// meets at a barrier.  Both of a thread's slots are requested before either is waited for: as a loop, the second trip's
// loads left only after the first trip's had come back and gone to LDS -- a memory round trip more in the prologue every
// workgroup of the CU waits through.
template <int TILE, typename Load, typename Store>
__device__ __forceinline__ void stage_tile(const TileMap &tm, Load &&load, Store &&store)
{
    static_assert(TILE <= 2 * kBlock, "two slots per thread");
    const int total = tm.total(), sl0 = threadIdx.x, sl1 = threadIdx.x + kBlock;
    const bool h0 = sl0 < total, h1 = sl1 < total;
    const int k0 = tm.index(h0 ? sl0 : 0) + n2_prologue_cost(sl0, tm), k1 = tm.index(h1 ? sl1 : 0) + n2_prologue_cost(sl1, tm);
    decltype(load(0)) r0, r1;
    if (h0) r0 = load(k0);
    if (h1) r1 = load(k1);
    if (h0) store(sl0, r0);
    if (h1) store(sl1, r1);
    __syncthreads();
}

// the particle a slot-coded entry of particle i names (full: the layout at capacity kSlotCodes); the passes call this only for
// the entries their tile does not hold
__device__ __forceinline__ int coded_index(const TileMap &full, int code, int i, int n)
{
    // (slot -> particle as two independent selects on the layout's range ends, like fluid_index of the sweep: TileMap::index
    // is a nested choice and compiles to exec-mask branches, five of them per neighbour the force pass does not stage)
    const int n0 = full.len0, n01 = full.len0 + full.len1;
    const int o0 = full.lo0, o1 = full.lo1 - n0, o2 = full.lo2 - n01;
    const int k_slot = code + o2 + (code < n01 ? o1 - o2 : 0) + (code < n0 ? o0 - o1 : 0);
    const int k_far = wrap_index(i + code - kCodeBias, n);
    return code < kSlotCodes ? k_slot : k_far;
}

template <int LPP>
__device__ __forceinline__ TileMap tile_ranges(const Grid &g, const FluidSet &s, int blk, int n_now, int cap)
{
    TileMap tm{0, 0, 0, 0, 0, 0};
    constexpr int per_tile = kBlock / LPP;
    const int p_first = blk * per_tile;
    if (p_first >= n_now) return tm;
    const int p_last = min(p_first + per_tile, n_now) - 1;
    const int c_first = s.cell[p_first], c_last = s.cell[p_last];
    const int cx = c_first / g.ncy, r_lo = c_first - cx * g.ncy;
    const int r_hi = (c_last / g.ncy == cx) ? c_last - cx * g.ncy : g.ncy - 1;  // the tile's part in column cx
    const int ra = max(r_lo - 1, 0), rb = min(r_hi + 1, g.ncy - 1) + 1;
    int lo[3], len[3];
#pragma unroll
    for (int ox = -1; ox <= 1; ++ox) {
        int col;
        const bool ok = neighbour_column(g, cx, ox, col);
        const int a0 = ok ? s.start[col * g.ncy + ra] : 0, a1 = ok ? s.start[col * g.ncy + rb] : 0;
        lo[ox + 1] = a0;
        len[ox + 1] = a1 - a0;
    }
    tm.lo0 = lo[1]; tm.len0 = min(len[1], cap);
    tm.lo1 = lo[0]; tm.len1 = min(len[0], cap - tm.len0);
    tm.lo2 = lo[2]; tm.len2 = min(len[2], cap - tm.len0 - tm.len1);
    return tm;
}

// Tile arrays that reach a device function as plain pointer arguments (continuity_body, density_walk_body: the same bodies
// serve kernels with and without a tile) are generic pointers to the compiler, and it read them with FLAT loads -- the texture
// path plus an aperture check -- instead of ds_read (round 3: k_continuity<2, true, 448> at 6 M particles 415 -> 376 us once
// told).  Read them through LDS-qualified pointers.
using lds_f64 = const __attribute__((address_space(3))) double;
__device__ __forceinline__ double2 lds_double2(const double2 *tile, int slot)
{
    lds_f64 *p = (lds_f64 *)tile;
    return make_double2(p[2 * slot], p[2 * slot + 1]);
}
__device__ __forceinline__ double lds_double(const double *tile, int slot) { return ((lds_f64 *)tile)[slot]; }
__device__ __forceinline__ double4 lds_double4(const double4 *tile, int slot)
{
    lds_f64 *p = (lds_f64 *)tile;
    return make_double4(p[4 * slot], p[4 * slot + 1], p[4 * slot + 2], p[4 * slot + 3]);
}

// tile capacity in particles: the three-column neighbourhood of kBlock / LPP particles at ~9 particles per cell
__host__ __device__ constexpr int tile_slots(int lpp) { return lpp >= 8 ? 192 : (lpp == 4 ? 320 : 480); }

// pass A, walking the superset list (see density_body MODE 2).  The LPP lanes of a particle test one list row at a
// time and pack the accepted entries with ballot + popcount, so a group's trip count is uniform: the rows in which all
// of its lanes hold fluid candidates run a branch-free fluid body with the entries three rows ahead, the (at most one
// mixed + the wall) rows behind them run the general body.
// (LDS tile: staging the candidate positions makes this pass slower at 0.5 M particles -- 50.5 against 42.3 us, it gathers
// only 16 bytes per candidate -- and, now that the pass runs at the texture addresser's limit, 6 % faster at 6 M: used
// where KGC and continuity use theirs.)
// (CODED: both lists hold slot-coded entries, see kSlotCodes -- the walk copies them as they stand)
template <int LPP, int TILE = 0, bool CODED = false>
__device__ __forceinline__ void density_walk_body(const Clock *clk, int q, const Grid &g, const Phys &ph, const FluidSet &s,
                                                  const FluidTmp &t, const Walls &w, PassWg bid, int nblk, bool half,
                                                  double2 *c_pos = nullptr)
{
    static_assert(!CODED || TILE == kSlotCodes, "slot-coded lists: the walk stages the whole layout");
    SPHX_PASS_INDEX_AT(bid, nblk);
    if (beyond_population<LPP>(clk, t, blk)) return;  // (nl_cnt of lanes beyond the population is never looked at)
    const double2 pi = in_cap ? s.pos[i] : make_double2(0.0, 0.0);
    const bool lead = in_cap && sub == 0;
    const double mass_i = lead ? s.mass[i] : 1.0, drho_i = lead ? s.drho[i] : 0.0;
    const int spacked = t.sl_cnt[tid];
    const int w_first0 = t.sl_pk[tid], w_first1 = t.sl_pk[(size_t)t.nl_stride + tid];  // rows 0-3 of the packed fluid rows
    const TileMap layout = TILE > 0 ? tile_map_of(t, blk) : TileMap{0, 0, 0, 0, 0, 0};
    const double dt = clk->dt;
    if (!clk->run[q]) return;
    const int n_now = clk->n;
    const bool active = i < n_now;
    TileMap tm{0, 0, 0, 0, 0, 0};
    if (TILE > 0) {  // candidate positions of the workgroup's three-column neighbourhood staged in LDS (see tile_ranges)
        tm = staged_map<LPP>(layout, blk, n_now, TILE);
        stage_tile<TILE>(tm, [&](int k) { return s.pos[k]; }, [&](int sl, const double2 &p) { c_pos[sl] = p; });
    }
    const LaneGroup<LPP> lg(tid, sub);
    int cnt = 0;
    // the step's list takes the candidate's entry as it stands in the superset list: a fluid entry is the index difference to
    // THIS particle in both, a wall entry the wall slot
    auto push = [&](bool acc, int entry, bool wall) { list_push_w(lg, t.nl_idx, t.nl_pk, t.nl_cap, t.nl_stride, cnt, acc, entry, wall); };
    const int ns = active ? list_rows(spacked) : 0;
    // group-uniform trip counts: lane 0 of the group owns the most rows, its last lane the fewest fluid rows
    const int rows_all = group_extreme<LPP, true>(ns);
    const int my_fl = active ? list_fluid_rows(spacked) : 0;
    const int rows_fl = group_extreme<LPP, false>(my_fl);
    const double xi = pi.x, yi = pi.y;
    double s_in = 0.0, s_ct = 0.0;
    // Three rows per turn.  A row is entry -> position -> test: the entries (16-bit index differences, two rows per word) run
    // ahead by whole words, the positions three rows (each requested into the register whose value has just been used -- a
    // rotating buffer would make every turn wait for the newest request); requests past the last row repeat it: no branch
    // around the loads, the values are not used.
    auto fluid_rows = [&](auto fold, auto near) {
        if (rows_fl <= 0) return;
        const int last = rows_fl - 1;
        constexpr bool kFold = decltype(fold)::value;
        constexpr bool kNear = decltype(near)::value;  // every entry of the wavefront names a staged slot (kFarTileBit)
        // (clamped by this lane's last word.  Clamping by the array instead makes the word's row x stride scalar arithmetic -- four
        //  64-bit multiply-adds less per turn -- and was measured slower, 378 -> 387 us at 6 M particles: the words behind a
        //  lane's last one are then real loads of lines nobody needs; profiles/r04_scalar_words_walk_c5.txt)
        auto word = [&](int p) { return t.sl_pk[(size_t)min(p, last >> 1) * t.nl_stride + tid]; };
        auto index = [&](int d) { return kFold ? wrap_index(i + d, n_now) : i + d; };
        auto row = [&](int d, const double2 &pj) {
            double dx = xi - pj.x;
            if (kFold) dx = min_image(g, dx);
            const double dy = yi - pj.y;
            const double r2 = dx * dx + dy * dy;
            const bool acc = r2 > kR2Min && r2 < ph.kc.rcut2;
            const double W = spline_W_sel(ph.kc, r2 * rsqrt_nr(r2));  // (NaN for a coincident pair: discarded by the select)
            s_in += acc ? W : 0.0;
            push(acc, d, false);
        };
        // words: [wa wb] hold rows m .. m+3 of the current turn and the next, [wc wd] the four behind them
        int wa = w_first0, wb = w_first1, wc = word(2), wd = word(3);
        if (TILE > 0) {  // positions from the tile (a few cycles away): only the entries run ahead
            auto fetch = [&](int e) -> double2 {  // (early return, not if/else: see k_kgc_w)
                if (CODED) {
#if SPHX_EXP_PRETEND_COMPLETE_TILE & 1
                    return lds_double2(c_pos, min(e, kSlotCodes - 1));  // MEASUREMENT ONLY, see k_forces_w
#endif
                    if (kNear) return lds_double2(c_pos, e);
                    if (e < kSlotCodes) return lds_double2(c_pos, e);
                    return s.pos[wrap_index(i + e - kCodeBias, n_now)];
                }
                const int k = index(e), slot = tm.slot(k);
                if (slot >= 0) return lds_double2(c_pos, slot);
                return s.pos[k];
            };
            // (measured on the near walk at 6 M particles and not kept, 375-383 us either way: the turn's words through a walking
            //  pointer instead of word()'s two 64-bit multiply-adds; a turn's four tile reads requested together instead of one
            //  LDS round trip at the head of every row -- profiles/r04_walking_pointer_walk_c5.txt, r04_batched_lds_walk_c5.txt)
            for (int m = 0; m < rows_fl; m += 4) {
                const int we = word((m >> 1) + 4), wf = word((m >> 1) + 5);
                const int d0 = CODED ? code_lo(wa) : delta_lo(wa), d1 = CODED ? code_hi(wa) : delta_hi(wa);
                const int d2 = CODED ? code_lo(wb) : delta_lo(wb), d3 = CODED ? code_hi(wb) : delta_hi(wb);
                row(d0, fetch(d0));
                if (m + 1 < rows_fl) row(d1, fetch(d1));
                if (m + 2 < rows_fl) row(d2, fetch(d2));
                if (m + 3 < rows_fl) row(d3, fetch(d3));
                wa = wc; wb = wd; wc = we; wd = wf;
            }
            return;
        }
        // four rows per turn, their positions requested one turn ahead.  Requests past the last row decode whatever the word
        // holds -- an index difference some earlier list left there: a slot of the arrays, clamped to be sure -- so there
        // is no branch and no select around the loads; the values are not used.
        auto ahead = [&](int d) { return kFold ? wrap_index(i + d, n_now) : max(0, min(i + d, t.cap - 1)); };
        int d0 = delta_lo(wa), d1 = delta_hi(wa), d2 = delta_lo(wb), d3 = delta_hi(wb);
        double2 p0 = s.pos[index(d0)], p1 = s.pos[ahead(d1)], p2 = s.pos[ahead(d2)], p3 = s.pos[ahead(d3)];
        for (int m = 0; m < rows_fl; m += 4) {
            const int we = word((m >> 1) + 4), wf = word((m >> 1) + 5);
            const int n0 = delta_lo(wc), n1 = delta_hi(wc), n2 = delta_lo(wd), n3 = delta_hi(wd);
            row(d0, p0);
            p0 = s.pos[ahead(n0)];
            if (m + 1 < rows_fl) row(d1, p1);
            p1 = s.pos[ahead(n1)];
            if (m + 2 < rows_fl) row(d2, p2);
            p2 = s.pos[ahead(n2)];
            if (m + 3 < rows_fl) row(d3, p3);
            p3 = s.pos[ahead(n3)];
            d0 = n0; d1 = n1; d2 = n2; d3 = n3;
            wa = wc; wb = wd; wc = we; wd = wf;
        }
    };
    const bool all_near = CODED && TILE > 0 && !__any(spacked & kFarTileBit);  // (see kFarTileBit)
    if (__any(active && near_seam(g, xi))) fluid_rows(std::true_type{}, std::false_type{});
    else if (CODED && all_near) fluid_rows(std::false_type{}, std::true_type{});
    else fluid_rows(std::false_type{}, std::false_type{});
    int cnt_fl = cnt;
    for (int m = rows_fl; m < rows_all; ++m) {  // the mixed row and the wall rows
        bool acc = false, wall = false;
        int e = 0;
        if (m < ns) {
            wall = m >= my_fl;  // a lane's fluid rows come first
            double2 pj;
            if (wall) {
                e = t.sl_idx[(size_t)m * t.nl_stride + tid];
                pj = w.pos[e & (kWallBit - 1)];
            } else {
                e = CODED ? code_of_row(t.sl_pk, t.nl_stride, m, tid) : delta_of_row(t.sl_pk, t.nl_stride, m, tid);
                pj = s.pos[CODED ? coded_index(tm, e, i, n_now) : wrap_index(i + e, n_now)];
            }
            const double dx = min_image(g, xi - pj.x), dy = yi - pj.y;
            const double r2 = dx * dx + dy * dy;
            if (r2 > kR2Min && r2 < ph.kc.rcut2) {
                acc = true;
                const double W = spline_W_sel(ph.kc, r2 * rsqrt_nr(r2));
                if (wall) s_ct += W * w.a[e & (kWallBit - 1)].x;
                else s_in += W;
            }
        }
        cnt_fl += LPP == 1 ? ((acc && !wall) ? 1 : 0) : __popc(lg.bits(acc && !wall));
        push(acc, e, wall);
    }
    if (active && cnt > t.nl_cap * LPP) { atomicOr(t.flags, 1); cnt = t.nl_cap * LPP; }
    cnt_fl = min(cnt_fl, cnt);
    if (tid < t.nl_stride)
        t.nl_cnt[tid] = list_row_counts<LPP>(cnt, cnt_fl, sub) | (CODED ? spacked & (kFarForcesBit | kFarTileBit) : 0);
    s_in = group_sum<LPP>(s_in);
    s_ct = group_sum<LPP>(s_ct);
    if (active && sub == 0) store_density(ph, t, i, s_in, s_ct, mass_i, drho_i, dt, half);
}

// pass A, sweeping the cells (see density_body MODE 0 / 1), large-channel form.  At a few lanes per particle a lane tests
// 20-40 candidates: in the compact form every trip was a load followed by a wait for it.  Here the candidates' addresses
// -- three contiguous index ranges, known before the loop -- are requested two trips ahead, the minimum-image fold runs
// only in wavefronts near the periodic seam, the kernel value is branch-free, and kernel value and list stores are spent on
// the candidates inside the radius only (two phases, see fluid_sweep).
// (CODED: fluid entries are written slot-coded, see kSlotCodes)
template <int LPP, int MODE, bool CODED = false>
__device__ __forceinline__ void density_sweep_body_w(const Clock *clk, int q, const Grid &g, const Phys &ph, const FluidSet &s,
                                                     const FluidTmp &t, const Walls &w, int bid, int nblk, bool half)
{
    static_assert(MODE == 0 || MODE == 1, "sweeping forms only");
    __shared__ int far_parked[CODED ? kBlock : 1];
    SPHX_PASS_INDEX_AT(bid, nblk);
    if (beyond_population<LPP>(clk, t, blk)) return;
    const double2 pi = in_cap ? s.pos[i] : make_double2(0.0, 0.0);
    const int ci = in_cap ? s.cell[i] : 0;
    const bool lead = in_cap && sub == 0;
    const double mass_i = lead ? s.mass[i] : 1.0, drho_i = lead ? s.drho[i] : 0.0;
    const double dt = clk->dt;
    if (!clk->run[q]) return;
    const int n_now = clk->n;
    const bool active = i < n_now;
    constexpr bool record = MODE == 1;
    // the workgroup's tile layout, the one its passes stage until the next re-binning (tile_map_of; CODED: the lists name its slots)
    TileMap layout{0, 0, 0, 0, 0, 0};
    if (t.tmap != nullptr) {
        layout = tile_ranges<LPP>(g, s, blk, n_now, kSlotCodes);
        if (threadIdx.x == 0) store_tile_map(t, blk, layout);
    }
    double s_in = 0.0, s_ct = 0.0;
    int cnt = 0, scnt = 0;
    const LaneGroup<LPP> lg(tid, sub);
    auto push_to = [&](int *idx, int *pk, int cap, int &n, bool acc, int entry, bool wall) {
        list_push_w(lg, idx, pk, cap, t.nl_stride, n, acc, entry, wall);
    };
    const double xi = pi.x, yi = pi.y;
    int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, wlo[3] = {0, 0, 0}, whi[3] = {0, 0, 0};
    bool near_wall = false;
    if (active) {
        const int cx = ci / g.ncy, cy = ci - cx * g.ncy;
        const int cylo = max(cy - 1, 0), cyhi = min(cy + 1, g.ncy - 1);
        near_wall = w.row_any[cy] != 0;
#pragma unroll
        for (int ox = -1; ox <= 1; ++ox) {
            int col;
            const bool ok = neighbour_column(g, cx, ox, col);
            const int c0 = col * g.ncy + cylo, c1 = col * g.ncy + cyhi + 1;
            lo[ox + 1] = ok ? s.start[c0] : 0;
            hi[ox + 1] = ok ? s.start[c1] : 0;
            wlo[ox + 1] = ok ? w.start[c0] : 0;
            whi[ox + 1] = ok ? w.start[c1] : 0;
        }
    }
    // the three ranges as one (see ranges_index); a group's lanes take LPP consecutive candidates per trip
    const int n0 = hi[0] - lo[0], n1 = hi[1] - lo[1], n2 = hi[2] - lo[2];
    const int nfl = n0 + n1 + n2;
    // v -> particle index: two independent selects (a nested choice of three becomes branches, or a table in scratch memory)
    const int n01 = n0 + n1, off2 = lo[2] - n01, d12 = (lo[1] - n0) - off2, d01 = lo[0] - (lo[1] - n0);
    auto fluid_index = [&](int v) { return v + off2 + (v < n01 ? d12 : 0) + (v < n0 ? d01 : 0); };
    // kFarTileBit / kFarForcesBit from the candidate ranges rather than from the entries handed out (a running maximum is one
    // register more than this kernel has for six waves -- and so is this word, which waits in LDS until the counts are stored):
    // each of the particle's three ranges must lie inside the layout's range of that column.  The lanes of a group agree; which of them stores an entry and which one walks it differ, but they sit in
    // one wavefront, and wavefronts decide.
    if (CODED) {
        // (the particle's left / own / right range against the layout's second / first / third: a particle of the column the
        //  layout was made for; any other one -- the tail of a workgroup that runs into the next column -- fails the test)
        const bool miss = (n0 > 0 && (lo[0] < layout.lo1 || hi[0] > layout.lo1 + layout.len1)) ||
                          (n1 > 0 && (lo[1] < layout.lo0 || hi[1] > layout.lo0 + layout.len0)) ||
                          (n2 > 0 && (lo[2] < layout.lo2 || hi[2] > layout.lo2 + layout.len2));
        const int top = n2 > 0 ? layout.len0 + layout.len1 + (hi[2] - layout.lo2) : (n0 > 0 ? layout.len0 + (hi[0] - layout.lo1) : hi[1] - layout.lo0);
        far_parked[threadIdx.x] = miss ? (kFarForcesBit | kFarTileBit) : (top > kForceSlots ? kFarForcesBit : 0);
    }
    // Two phases per chunk of 64 trips.  Only a third of the candidates of the 3 x 3 cells lie inside the (superset) radius,
    // and kernel value + packed list stores are four fifths of a trip's instructions: phase 1 only measures distances and
    // marks the trips inside the radius in a bit mask (positions requested three trips ahead, each into a register of its
    // own -- a rotating buffer would make every turn wait for the newest request; requests past the end repeat the last
    // candidate: no branch around the load); phase 2 visits the marked trips only.  A group's lanes mark different
    // trips, so its list holds the same entries as the compact form's in a slightly different (still fixed) order.
    const double r2_mark = record ? t.sl_rcut2 : ph.kc.rcut2;
    auto fluid_sweep = [&](auto fold) {
        if (nfl <= 0) return;
        auto index_at = [&](int v) { return fluid_index(min(v, nfl - 1)); };
        auto dist2 = [&](const double2 &pj) {
            double dx = xi - pj.x;
            if (decltype(fold)::value) dx = min_image(g, dx);
            const double dy = yi - pj.y;
            return dx * dx + dy * dy;
        };
        for (int base = 0; base < nfl; base += 64 * LPP) {
            const int n_tr = min((nfl - base + LPP - 1) / LPP, 64);  // trips of this chunk (the same for the group's lanes)
            unsigned long long mask = 0;
            auto mark = [&](int tt, const double2 &pj) {
                const double r2 = dist2(pj);
                const bool inside = base + tt * LPP + sub < nfl && r2 > kR2Min && r2 < r2_mark;
                mask |= (unsigned long long)(inside ? 1 : 0) << tt;
            };
            double2 pa = s.pos[index_at(base + sub)], pb = s.pos[index_at(base + LPP + sub)],
                    pc = s.pos[index_at(base + 2 * LPP + sub)];
            for (int tt = 0; tt < n_tr; tt += 3) {
                mark(tt, pa);
                pa = s.pos[index_at(base + (tt + 3) * LPP + sub)];
                if (tt + 1 < n_tr) mark(tt + 1, pb);
                pb = s.pos[index_at(base + (tt + 4) * LPP + sub)];
                if (tt + 2 < n_tr) mark(tt + 2, pc);
                pc = s.pos[index_at(base + (tt + 5) * LPP + sub)];
            }
            int rounds = __popcll(mask);
#pragma unroll
            for (int off = LPP / 2; off > 0; off >>= 1) rounds = max(rounds, __shfl_xor(rounds, off));
            // (the position of the next marked trip is requested before the current one is worked on)
            auto next_marked = [&](bool &has, int &k) {
                has = mask != 0;
                const int tt = has ? __ffsll((long long)mask) - 1 : 0;
                mask &= mask - 1;
                k = index_at(base + tt * LPP + sub);
            };
            bool has, has_n;
            int k, k_n;
            next_marked(has, k);
            double2 pj = s.pos[k];
            for (int r = 0; r < rounds; ++r) {
                next_marked(has_n, k_n);
                const double2 pj_n = s.pos[k_n];
                const double r2 = dist2(pj);
                const bool acc = has && r2 < ph.kc.rcut2;
                const double W = spline_W_sel(ph.kc, r2 * rsqrt_nr(r2));
                s_in += acc ? W : 0.0;
                int d = 0;
                if (has) {
                    const int slot = CODED ? layout.slot(k) : -1;
                    d = slot >= 0 ? slot
                                  : encode_delta(k, i, n_now, g.periodic != 0, t.flags, CODED ? kCodedDeltaMax : kDeltaMax) + (CODED ? kCodeBias : 0);
                }
                push_to(t.nl_idx, t.nl_pk, t.nl_cap, cnt, acc, d, false);
                if (record) push_to(t.sl_idx, t.sl_pk, t.sl_cap, scnt, has, d, false);
                has = has_n; k = k_n; pj = pj_n;
            }
        }
    };
    if (__any(active && near_seam(g, xi))) fluid_sweep(std::true_type{});
    else fluid_sweep(std::false_type{});
    int cnt_fl = cnt, scnt_fl = scnt;
    if (near_wall) {
        const int w0 = whi[0] - wlo[0], w1 = whi[1] - wlo[1], w2 = whi[2] - wlo[2];
        const int nwl = w0 + w1 + w2;
        auto wall_index = [&](int v) { return ranges_index(wlo[0], wlo[1], wlo[2], w0, w1, v); };
        if (nwl > 0) {
            int ka = wall_index(min(sub, nwl - 1));
            double2 pa = w.pos[ka];
            double va = w.a[ka].x;
            for (int vb = 0; vb < nwl; vb += LPP) {
                const int kb = wall_index(min(vb + LPP + sub, nwl - 1));
                const double2 pb = w.pos[kb];
                const double vb_ = w.a[kb].x;
                const double dx = min_image(g, xi - pa.x), dy = yi - pa.y;
                const double r2 = dx * dx + dy * dy;
                const bool in = vb + sub < nwl && r2 > kR2Min;
                const bool acc = in && r2 < ph.kc.rcut2;
                const double W = spline_W_sel(ph.kc, r2 * rsqrt_nr(r2));
                s_ct += acc ? W * va : 0.0;
                push_to(t.nl_idx, t.nl_pk, t.nl_cap, cnt, acc, ka | kWallBit, true);
                if (record) push_to(t.sl_idx, t.sl_pk, t.sl_cap, scnt, in && r2 < t.sl_rcut2, ka | kWallBit, true);
                ka = kb; pa = pb; va = vb_;
            }
        }
    }
    if (active && cnt > t.nl_cap * LPP) { atomicOr(t.flags, 1); cnt = t.nl_cap * LPP; }
    cnt_fl = min(cnt_fl, cnt);
    if (record && active && scnt > t.sl_cap * LPP) { atomicOr(t.flags, 1); scnt = t.sl_cap * LPP; }
    scnt_fl = min(scnt_fl, scnt);
    const int far_bits = CODED ? far_parked[threadIdx.x] : 0;
    if (tid < t.nl_stride) t.nl_cnt[tid] = list_row_counts<LPP>(cnt, cnt_fl, sub) | far_bits;
    if (record && tid < t.nl_stride) t.sl_cnt[tid] = list_row_counts<LPP>(scnt, scnt_fl, sub) | far_bits;
    s_in = group_sum<LPP>(s_in);
    s_ct = group_sum<LPP>(s_ct);
    if (active && sub == 0) store_density(ph, t, i, s_in, s_ct, mass_i, drho_i, dt, half);
}

// n_tiles: workgroup-sized tiles of the pass; the grid may be smaller (grid-stride over the tiles: the conditional launches
// of a dynamic context, which are idle most of the time, see launch_pass_a)
template <int LPP, int MODE, bool CODED = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(CODED ? 6 : 5))) void k_density_sweep_w(const Clock *clk, int q, Grid g, Phys ph, FluidSet s,
                                                            FluidTmp t, Walls w, int cond_fresh, int n_tiles)
{
    if (cond_fresh >= 0 && (clk->fresh != 0) != (cond_fresh != 0)) return;
    for (int b = (int)blockIdx.x; b < n_tiles; b += (int)gridDim.x)
        density_sweep_body_w<LPP, MODE, CODED>(clk, q, g, ph, s, t, w, b, n_tiles, true);
}

template <int LPP, int TILE = 0, bool CODED = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu((TILE > 0 || LPP <= 2) ? 8 : 1))) void k_density_w(const Clock *clk, int q, Grid g, Phys ph, FluidSet s,
                                                      FluidTmp t, Walls w, int cond_fresh)
{
    constexpr int kSlots = TILE > 0 ? TILE : 1;
    __shared__ double2 c_pos[kSlots];
    const int part = cond_fresh >= 0 ? cond_fresh >> kPassPartShift : 0;  // (see slab_part_skips)
    if (part) cond_fresh &= (1 << kPassPartShift) - 1;
    if (cond_fresh >= 0 && (clk->fresh != 0) != (cond_fresh != 0)) return;
    if (part && slab_part_skips<LPP>(g, s, xcd_block((int)blockIdx.x, (int)gridDim.x), part)) return;
    density_walk_body<LPP, TILE, CODED>(clk, q, g, ph, s, t, w, (int)blockIdx.x, (int)gridDim.x, true, c_pos);
}

// pass B (see k_kgc); CODED: slot-coded list entries (kSlotCodes)
template <int LPP, int TILE, bool CODED = false>
__global__ __launch_bounds__(kBlock) void k_kgc_w(const Clock *clk, int q, Grid g, Phys ph, FluidSet s,
                                                  FluidTmp t, Walls w, int finish_half)
{
    static_assert(!CODED || TILE == kSlotCodes, "slot-coded lists: this pass stages the whole layout");
    constexpr int kSlots = TILE > 0 ? TILE : 1;
    __shared__ double2 c_pos[kSlots];
    __shared__ double c_vol[kSlots];
    SPHX_PASS_INDEX();
    if (beyond_population<LPP>(clk, t, blk)) return;
    const double2 pi = in_cap ? s.pos[i] : make_double2(0.0, 0.0);
    const bool closes = finish_half && in_cap && sub == 0;  // (see k_kgc)
    const double4 a_own = closes ? t.a[i] : make_double4(0.0, 0.0, 0.0, 0.0);
    const double drho_own = closes ? s.drho[i] : 0.0;
    const int packed = t.nl_cnt[tid];
    const int w0 = t.nl_pk[tid], w1 = t.nl_pk[(size_t)t.nl_stride + tid];
    const TileMap layout = TILE > 0 ? tile_map_of(t, blk) : TileMap{0, 0, 0, 0, 0, 0};
    if (!clk->run[q]) return;
    const int n_now = clk->n;
    const bool active = i < n_now;
    TileMap tm{0, 0, 0, 0, 0, 0};
    if (TILE > 0) {
        tm = staged_map<LPP>(layout, blk, n_now, TILE);
        struct Rec { double2 p; double vol; };
        stage_tile<TILE>(tm, [&](int k) { return Rec{s.pos[k], t.vol[k]}; },
                         [&](int sl, const Rec &r) { c_pos[sl] = r.p; c_vol[sl] = r.vol; });
    }
    // (early return, not if/else: the compiler would merge the two arms into one FLAT load through a selected pointer)
    auto fetch = [&](int k, double2 &pj, double &Volj) {
        if (TILE > 0) {
            const int slot = tm.slot(k);
            if (slot >= 0) { pj = c_pos[slot]; Volj = c_vol[slot]; return; }
        }
        pj = s.pos[k]; Volj = t.vol[k];
    };
    const int rows = active ? list_rows(packed) : 0, rows_fl = active ? list_fluid_rows(packed) : 0;
    const double xi = pi.x, yi = pi.y;
    double a11 = 0.0, a12 = 0.0, a21 = 0.0, a22 = 0.0;
    auto term = [&](double dx, double dy, double Volj) { kgc_moment_add(ph.kc, dx, dy, Volj, a11, a12, a21, a22); };
    auto fetch_code = [&](int e, double2 &pj, double &Volj) {  // (CODED; early return: see above)
        // (LDS-qualified reads: with plain ones the compiler folds both arms into FLAT loads through selected pointers)
#if SPHX_EXP_PRETEND_COMPLETE_TILE & 2
        e = min(e, kSlotCodes - 1);  // MEASUREMENT ONLY, see k_forces_w
#endif
        if (e < kSlotCodes) { pj = lds_double2(c_pos, e); Volj = lds_double(c_vol, e); return; }
        const int k = wrap_index(i + e - kCodeBias, n_now);
        pj = s.pos[k]; Volj = t.vol[k];
    };
    const bool seam = __any(active && near_seam(g, xi));
    const bool all_near = CODED && !__any(packed & kFarTileBit);  // (see kFarTileBit)
    // (the five forms written out, not through walk_fluid_forms: with it k_kgc_w<2, 480, true> takes two scalar registers more)
    if (CODED && seam)
        walk_fluid_rows<true>(t, tid, i, rows_fl, w0, w1, [&](int e) {
            double2 pj; double Volj;
            fetch_code(e, pj, Volj);
            term(min_image(g, xi - pj.x), yi - pj.y, Volj);
        });
    else if (CODED && all_near)
        walk_fluid_rows<true>(t, tid, i, rows_fl, w0, w1, [&](int e) {
            const double2 pj = lds_double2(c_pos, e);
            term(xi - pj.x, yi - pj.y, lds_double(c_vol, e));
        });
    else if (CODED)
        walk_fluid_rows<true>(t, tid, i, rows_fl, w0, w1, [&](int e) {
            double2 pj; double Volj;
            fetch_code(e, pj, Volj);
            term(xi - pj.x, yi - pj.y, Volj);
        });
    else if (seam)
        walk_fluid_rows(t, tid, i, rows_fl, w0, w1, [&](int k) {
            double2 pj; double Volj;
            fetch(wrap_index(k, n_now), pj, Volj);
            term(min_image(g, xi - pj.x), yi - pj.y, Volj);
        });
    else
        walk_fluid_rows(t, tid, i, rows_fl, w0, w1, [&](int k) {
            double2 pj; double Volj;
            fetch(k, pj, Volj);
            term(xi - pj.x, yi - pj.y, Volj);
        });
    walk_wall_rows(t, tid, rows_fl, rows, [&](int k) {
        const double2 pj = w.pos[k];
        term(min_image(g, xi - pj.x), yi - pj.y, w.a[k].x);
    });
    a11 = group_sum<LPP>(a11);
    a12 = group_sum<LPP>(a12);
    a21 = group_sum<LPP>(a21);
    a22 = group_sum<LPP>(a22);
    if (active && sub == 0) {
        const Mat2 B = kgc_from_A(a11, a12, a21, a22);
        t.B[i] = make_double4(B.m11, B.m12, B.m21, B.m22);
        if (finish_half) {
            double rhoh, p_half;
            half_state(ph, a_own.w, drho_own, clk->dt, rhoh, p_half);
            t.a[i] = make_double4(a_own.x, p_half, rhoh, a_own.w);
        }
    }
}

// pass CD (see k_forces); TILE > 0: neighbour records come from the LDS tile (tile_ranges)
struct FluidNb {
    double2 p, v;
    double4 a, B;
};

// (CODED: slot-coded list entries, see kSlotCodes -- this pass's tile holds the first TILE slots of the layout)
template <int LPP, int TILE, bool CODED = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(TILE > 400 ? 4 : 5))) void k_forces_w(const Clock *clk, int q, Grid g, Phys ph, FluidSet s,
                                                     FluidTmp t, Walls w)
{
    static_assert(!CODED || (TILE > 0 && TILE <= kSlotCodes), "slot-coded lists need a tile");
    constexpr int kSlots = TILE > 0 ? TILE : 1;
    // (88 bytes per staged neighbour: of {Vol, p_half, rho_half, rho} the pass reads three)
    __shared__ double2 c_pos[kSlots], c_vel[kSlots], c_vp[kSlots];
    __shared__ double c_rh[kSlots];
    __shared__ double4 c_B[kSlots];
    SPHX_PASS_INDEX();
    if (beyond_population<LPP>(clk, t, blk)) {  // (a slab's arrays have 15-20 % of slack: see beyond_population)
        if (threadIdx.x == 0 && clk->run[q]) t.dpart[blk] = 0.0;
        return;
    }
    const double2 pi = in_cap ? s.pos[i] : make_double2(0.0, 0.0);
    const double2 vi = in_cap ? s.vel[i] : make_double2(0.0, 0.0);
    const double4 ai = in_cap ? t.a[i] : make_double4(1.0, 0.0, 0.0, 0.0);
    const double4 Bi = in_cap ? t.B[i] : make_double4(1.0, 0.0, 0.0, 1.0);
    const double mi = in_cap ? s.mass[i] : 1.0;
    const int packed = t.nl_cnt[tid];
    const int w0 = t.nl_pk[tid], w1 = t.nl_pk[(size_t)t.nl_stride + tid];
    const bool tracked = s.posb != nullptr;
    const double2 pb = (tracked && in_cap && sub == 0) ? s.posb[i] : make_double2(0.0, 0.0);
    const TileMap layout = TILE > 0 ? tile_map_of(t, blk) : TileMap{0, 0, 0, 0, 0, 0};
    const double dt = clk->dt;
    const bool want_out = step_outputs_wanted(clk, t);
    if (!clk->run[q]) return;
    const int n_now = clk->n;
    const bool active = i < n_now;
    const int rows = active ? list_rows(packed) : 0, rows_fl = active ? list_fluid_rows(packed) : 0;
    const double h = ph.kc.h, soft = 0.01 * h;
    double ax = 0.0, ay = 0.0, ix = 0.0, iy = 0.0, px = 0.0, py = 0.0, d2 = 0.0;
    const double xi = pi.x, yi = pi.y, vxi = vi.x, vyi = vi.y;
    const double Voli = ai.x, p_i = ai.y, rhoh_i = ai.z;
    const double b11i = Bi.x, b12i = Bi.y, b21i = Bi.z, b22i = Bi.w;

    TileMap tm{0, 0, 0, 0, 0, 0};
    if (TILE > 0) {
        tm = staged_map<LPP>(layout, blk, n_now, TILE);
        stage_tile<TILE>(tm, [&](int k) { return FluidNb{s.pos[k], s.vel[k], t.a[k], t.B[k]}; }, [&](int sl, const FluidNb &n) {
            c_pos[sl] = n.p; c_vel[sl] = n.v; c_vp[sl] = make_double2(n.a.x, n.a.y); c_rh[sl] = n.a.z; c_B[sl] = n.B;
        });
    }
    const int n_staged = tm.total();
    auto fetch_code = [&](int e) {  // (CODED)
        FluidNb n;
#if SPHX_EXP_PRETEND_COMPLETE_TILE & 4
        // MEASUREMENT ONLY (tools/probes/build_variant_lib.sh -DSPHX_EXP_PRETEND_COMPLETE_TILE=<1 pass A | 2 B | 4 CD | 8 E>, never
        // in libsphx.so): what would a particle order buy whose
        // neighbourhoods fit TILE slots?  Entries the tile does not hold read some staged slot instead of global memory: the
        // results are wrong, the instruction and memory streams are those of a complete tile (timed with sphx_ctx_time_kernel,
        // which does not feed the outputs back into the state).
        e = e < n_staged ? e : (e & 255);
#endif
        if (e < n_staged) {  // (LDS-qualified reads: see k_kgc_w)
            const double2 vp = lds_double2(c_vp, e);
            n.p = lds_double2(c_pos, e); n.v = lds_double2(c_vel, e); n.a = make_double4(vp.x, vp.y, lds_double(c_rh, e), 0.0); n.B = lds_double4(c_B, e);
            return n;
        }
        const int k = coded_index(layout, e, i, n_now);
        n.p = s.pos[k]; n.v = s.vel[k]; n.a = t.a[k]; n.B = t.B[k];
        return n;
    };
    auto fetch = [&](int k) {
        FluidNb n;
        if (TILE > 0) {  // (early return, not if/else: see k_kgc_w)
            const int slot = tm.slot(k);
            if (slot >= 0) {
                const double2 vp = c_vp[slot];
                n.p = c_pos[slot]; n.v = c_vel[slot]; n.a = make_double4(vp.x, vp.y, c_rh[slot], 0.0); n.B = c_B[slot];
                return n;
            }
        }
        n.p = s.pos[k]; n.v = s.vel[k]; n.a = t.a[k]; n.B = t.B[k];
        return n;
    };
    // The pair term, arranged for the instruction count (the pass is VALU-bound: ~70 % of its cycles issue vector
    // instructions).  Against the reference's order of operations (sph_physics_mex.c:1100-1140), equal up to rounding:
    //   * un_l - un_r = (v_i - v_j) . e, with the velocity difference the viscous term needs anyway;
    //   * p_face = (p_avg + p_star) / 2 with p_star = p_avg + beta rho_bar (un_l - un_r) / 2 collapses to
    //     (p_i + p_j) / 2 + [beta / 8] (rho_i + rho_j) (un_l - un_r); beta / 8 = min(3/8 max(du, 0), c_f / 8) exactly
    //     (powers of two);
    //   * mu is multiplied into the viscous sums once, after the walk.
    const double c_f8 = 0.125 * ph.c_f;
    auto fluid_pair = [&](const FluidNb &n, double dx) {
        const auto [r, ex, ey] = pair_geom(dx, yi - n.p.y);
        const double dWVj = spline_dW_in(ph.kc, r) * n.a.x;
        const double tx = (b11i + n.B.x) * ex + (b12i + n.B.y) * ey;
        const double ty = (b21i + n.B.z) * ex + (b22i + n.B.w) * ey;
        const double eBe = ex * tx + ey * ty;
        const double dvx = vxi - n.v.x, dvy = vyi - n.v.y;
        // viscous (without mu)
        const double coeff = eBe * dWVj * rcp_nr(r + soft);
        ax += coeff * dvx;
        ay += coeff * dvy;
        // transport
        ix -= dWVj * tx;
        iy -= dWVj * ty;
        // pressure (Riemann-dissipated face pressure)
        const double du = dvx * ex + dvy * ey;
        const double beta8 = fmin(0.375 * fmax(du, 0.0), c_f8);
        const double p_face = fma(beta8 * (rhoh_i + n.a.z), du, 0.5 * (p_i + n.a.y));
        const double pw = p_face * dWVj;
        px -= pw * tx;
        py -= pw * ty;
    };
    const bool seam = __any(active && near_seam(g, xi));
    const bool all_near = CODED && TILE == kForceSlots && !__any(packed & kFarForcesBit);  // (see kFarTileBit)
    auto fetch_near = [&](int e) {  // (CODED, all_near)
        FluidNb n;
        const double2 vp = lds_double2(c_vp, e);
        n.p = lds_double2(c_pos, e); n.v = lds_double2(c_vel, e); n.a = make_double4(vp.x, vp.y, lds_double(c_rh, e), 0.0); n.B = lds_double4(c_B, e);
        return n;
    };
    walk_fluid_forms<CODED>(g, t, tid, i, n_now, rows_fl, w0, w1, xi, seam, all_near, fetch_near, fetch_code, fetch, fluid_pair);
    // wall neighbours: viscous and transport now, pressure once force_prior is complete (p_wall needs it, :931-934)
    walk_wall_rows(t, tid, rows_fl, rows, [&](int k) {
        const double2 pj = w.pos[k];
        const double4 wj = w.a[k];
        const WallPair wp = wall_pair(ph.kc, min_image(g, xi - pj.x), yi - pj.y, wj.x, Bi);
        const double coeff = 4.0 * wp.eBe * wp.dWVj * rcp_nr(wp.r + soft);  // (mu: after the walk, see fluid_pair)
        ax += coeff * (vxi - wj.y);
        ay += coeff * (vyi - wj.z);
        ix -= 2.0 * wp.dWVj * wp.tx;
        iy -= 2.0 * wp.dWVj * wp.ty;
    });
    ax = group_sum<LPP>(ax) * ph.mu;
    ay = group_sum<LPP>(ay) * ph.mu;
    ix = group_sum<LPP>(ix);
    iy = group_sum<LPP>(iy);
    const double fpx = ax * Voli + mi * ph.g;  // + gravity, SPH_Poiseuille.m:392
    const double fpy = ay * Voli;
    const double inv_m = rcp_nr(mi);
    if (rows > rows_fl) {
        const double acx = fpx * inv_m, acy = fpy * inv_m;
        walk_wall_rows(t, tid, rows_fl, rows, [&](int k) {
            const double2 pj = w.pos[k];
            wall_pressure_add(ph.kc, min_image(g, xi - pj.x), yi - pj.y, w.a[k].x, Bi, acx, acy, p_i, rhoh_i, px, py);
        });
    }
    px = group_sum<LPP>(px);
    py = group_sum<LPP>(py);
    if (active && sub == 0) {
        const double fx = px * Voli, fy = py * Voli;
        const double vxn = vxi + (fpx + fx) * inv_m * dt;
        const double vyn = vyi + (fpy + fy) * inv_m * dt;
        // transport limiter min(1, 100 |inc|^2 / h^2) (sph_physics_mex.c:702-710) with 1/h^2 multiplied in
        const double lim = fmin(100.0 * (ix * ix + iy * iy) * (ph.kc.inv_h * ph.kc.inv_h), 1.0);
        const double sx = ph.tc * h * h * lim * ix, sy = ph.tc * h * h * lim * iy;
        double xo = xi + sx, yo = yi + sy;
        xo += 0.5 * dt * vxi;
        yo += 0.5 * dt * vyi;
        xo += 0.5 * dt * vxn;
        yo += 0.5 * dt * vyn;
        if (tracked) d2 = tracked_drift2(g, s, i, xo, yo, pb);
        // periodic wrap (SPH_Poiseuille.m:570-577): a step moves a particle by a tiny fraction of DL, so x - floor(x/DL) DL
        // is x - DL, x + DL or x -- the same values without the division (a slab wraps when particles change owner)
        if (g.periodic) xo = xo >= ph.DL ? xo - ph.DL : (xo < 0.0 ? xo + ph.DL : xo);
        t.posn[i] = make_double2(xo, yo);
        t.veln[i] = make_double2(vxn, vyn);
        if (want_out) {
            t.fp[i] = make_double2(fpx, fpy);
            t.f[i] = make_double2(fx, fy);
        }
    }
    store_block_drift(t, blk, d2);
}

// block-wide exclusive scan of one int per thread (NT threads); returns the block total
template <int NT>
__device__ __forceinline__ int block_exclusive_scan_t(int v, int &total, int *s_wave /*[NT/64+1]*/)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(inc, off);
        if (lane >= off) inc += o;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    if (wave == 0) {
        const int ws = lane < NT / 64 ? s_wave[lane] : 0;
        int winc = ws;
#pragma unroll
        for (int off = 1; off < NT / 64; off <<= 1) {
            const int o = __shfl_up(winc, off);
            if (lane >= off) winc += o;
        }
        if (lane < NT / 64) s_wave[lane] = winc - ws;  // exclusive wave offsets
        if (lane == NT / 64 - 1) s_wave[NT / 64] = winc;
    }
    __syncthreads();
    const int res = s_wave[wave] + inc - v;
    total = s_wave[NT / 64];
    __syncthreads();
    return res;
}

// advance the device clock by the step that has just been computed (one thread)
// drift: largest distance from the binning positions (< 0: not tracked); rebuilt: this step ends with a fresh grid.
// dyn_K > 0: dynamic context -- decide here whether this step ends with a re-binning (K-th step, or drift bound hit)
__device__ __forceinline__ void clock_step(Clock *clk, Clock c, int q, const Phys &ph, double vmax, int flags,
                                           int n_new, double drift = -1.0, int rebuilt = 1, double half_skin = 0.0,
                                           int dyn_K = 0)
{
    if (dyn_K > 0) {
        const bool by_drift = !(drift <= half_skin);
        const bool sched = c.pos_count >= dyn_K - 1;  // pass E has taken the histogram already
        const bool rb = by_drift || sched;
        c.rebuild_now = rb ? (sched ? 2 : 1) : 0;     // 2: histogram done, k_bin skips
        c.fresh = c.rebuild_now;  // the next pass A starts from a fresh grid
        c.pos_count = rb ? 0 : c.pos_count + 1;
        if (q == 0) c.pos_q[1] = (short)c.pos_count;  // (for the NEXT slot; this slot's own copy stays as its workgroups read it)
        else c.pos_q[0] = (short)c.pos_count;
        c.drift = rb ? 0.0 : drift;
        if (by_drift) c.n_drift_rebuilds += 1;
        if (rb) c.n_rebins += 1;
    } else if (drift >= 0.0) {
        c.drift = rebuilt ? 0.0 : drift;
        // every step sweeps the cells the particles were BINNED into; that finds all neighbours only while no
        // particle has drifted more than half the skin -> stop the loop, the host re-bins and resumes
        if (!(c.drift <= half_skin)) c.need_rebuild = 1;
    }
    c.vmax = vmax;
    c.t += c.n_in > 1 ? c.dt * c.n_in : c.dt;  // SPH_Poiseuille.m:267 (dual-rate: n_in sub-steps of dt were taken)
    c.dt_last = c.dt;
    c.step += 1;
    if (c.steps_left > 0) c.steps_left -= 1;
    if (!(c.vmax == c.vmax) || isinf(c.vmax)) c.status = SPHX_ERR_DIVERGED;
    if (flags) c.status = SPHX_ERR_GRID;  // neighbour-list / slab-buffer overflow
    if (n_new >= 0) c.n = n_new;
    c.dt = next_dt(c, ph);
    const int go = loop_continues(c) ? 1 : 0;
    if (q == 0) c.run[1] = go;  // constant indices: c.run[1 - q] would force the whole struct into scratch memory --
    else c.run[0] = go;         // 120 bytes per lane of EVERY wave of pass E when the tail workgroup lives there
    *clk = c;
    if (!go && c.pub) *c.pub = c;  // the batch ends here: tell the host (see Clock::pub)
}

// ---------------------------------------------------------------------------------------------
// pass E: continuity rate with the kicked velocities (integration_2nd, sph_physics_mex.c:1076-1116),
// final half-step of rho and EOS (:1440-1450), per-block max |v|^2 over owned particles for the next
// dt (SPH_Poiseuille.m:521) and -- single-GPU -- the cell histogram of the end-of-step positions
// (neighbour rebuild, the K0 insert of mex/sph_neighbor_search_mex.c:269-296).
// ---------------------------------------------------------------------------------------------
// Small channels: the clock update rides in pass E instead of being a launch of its own.  One extra workgroup
// (the last one) waits for the per-block max |v|^2 of all the others, then advances the clock exactly as
// k_clock_scan would.  Every vpart entry is its own "ready" flag: the producers store it with an agent-scope
// atomic (past the non-coherent L2), the tail polls with agent-scope atomic loads and puts the "empty" pattern
// back for the next step.  Nobody waits for the tail, so it cannot deadlock whatever the dispatch order; a grid
// barrier (all wait for all) was measured at 70-90 us for 600 workgroups, this costs the tail ~1-2 us.
// rebuilt: the step ends with a fresh grid (k_continuity_rebin), as k_clock_scan's argument of that name
// A tail of fewer than 256 threads (BLK = 64 / 128: the passes run in smaller workgroups, so there are two to four times as many
// entries and a quarter to a half of the threads): a thread asks for ALL of its entries of a round -- 1 024 per workgroup --
// before it looks at any, and polls again only those that came back empty.  One polling round trip per entry and thread, as
// at 256 threads, would be five to nineteen of them one behind the other.  The bounded spin and `lost` are the same.
template <int BLK>
__device__ __forceinline__ void continuity_tail_small(Clock *clk, int q, const Phys &ph, const FluidTmp &t, int nb, int rebuilt)
{
    static_assert(BLK == 64 || BLK == 128, "the tail of 256 threads is continuity_tail's own");
    if (!clk->run[q]) {
        if (threadIdx.x == 0) clk->run[1 - q] = 0;  // idle slot keeps the following slots idle
        return;
    }
    Clock c0;
    int fl = 0;
    if (threadIdx.x == 0) { c0 = *clk; fl = *t.flags; }
    double m = 0.0, d = 0.0;
    int lost = 0;
    const bool track = t.half_skin >= 0.0;
    constexpr int kPer = 1024 / BLK;  // entries a thread has in flight
    for (int base = 0; base < nb; base += BLK * kPer) {
        unsigned long long bits[kPer];
        double dv[kPer];
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int k = base + j * BLK + (int)threadIdx.x;
            const int kk = min(k, nb - 1);  // (a thread without an entry asks for the last one and drops the answer)
            bits[j] = __hip_atomic_load(reinterpret_cast<unsigned long long *>(&t.vpart[kk]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            dv[j] = track ? t.dpart[kk] : 0.0;  // written by pass CD, a kernel ago
        }
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int k = base + j * BLK + (int)threadIdx.x;
            if (k < nb) {
                unsigned long long *slot = reinterpret_cast<unsigned long long *>(&t.vpart[k]);
                unsigned long long b = bits[j];
                unsigned spins = 0;
                while (b == kVpartEmpty) {
                    __builtin_amdgcn_s_sleep(2);
                    if (++spins > (1u << 22)) { lost = 1; break; }  // never hang the device on a protocol bug
                    b = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                if (b != kVpartEmpty) m = fmax(m, __longlong_as_double((long long)b));
                d = fmax(d, dv[j]);
                __hip_atomic_store(slot, kVpartEmpty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    m = wave_max(m);
    d = wave_max(d);
    lost = __any(lost) ? 1 : 0;
    if constexpr (BLK > 64) {
        __shared__ double s_m[BLK / 64], s_d[BLK / 64];
        __shared__ int s_l[BLK / 64];
        if ((threadIdx.x & 63) == 0) { s_m[threadIdx.x >> 6] = m; s_d[threadIdx.x >> 6] = d; s_l[threadIdx.x >> 6] = lost; }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 1; k < BLK / 64; ++k) { m = fmax(m, s_m[k]); d = fmax(d, s_d[k]); lost |= s_l[k]; }
    }
    if (threadIdx.x == 0) {
        if (lost) c0.status = SPHX_ERR_DIVERGED;
        clock_step(clk, c0, q, ph, sqrt(m), fl, -1, track ? sqrt(d) : -1.0, rebuilt, t.half_skin);
    }
}
// ... and a tail of more than 256 threads: continuity_tail's own loop, one polling
// round trip per entry and thread, with BLK threads
template <int BLK>
__device__ __forceinline__ void continuity_tail_wide(Clock *clk, int q, const Phys &ph, const FluidTmp &t, int nb, int rebuilt)
{
    static_assert(BLK > kBlock && BLK % 64 == 0, "the tail of 256 threads is continuity_tail's own");
    if (!clk->run[q]) {
        if (threadIdx.x == 0) clk->run[1 - q] = 0;  // idle slot keeps the following slots idle
        return;
    }
    Clock c0;
    int fl = 0;
    if (threadIdx.x == 0) { c0 = *clk; fl = *t.flags; }
    double m = 0.0, d = 0.0;
    int lost = 0;
    const bool track = t.half_skin >= 0.0;
    for (int k = threadIdx.x; k < nb; k += BLK) {
        if (track) d = fmax(d, t.dpart[k]);  // written by pass CD, a kernel ago
        unsigned long long *slot = reinterpret_cast<unsigned long long *>(&t.vpart[k]);
        unsigned long long bits;
        unsigned spins = 0;
        while ((bits = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == kVpartEmpty) {
            __builtin_amdgcn_s_sleep(2);
            if (++spins > (1u << 22)) { lost = 1; break; }  // never hang the device on a protocol bug
        }
        if (!lost) m = fmax(m, __longlong_as_double((long long)bits));
        __hip_atomic_store(slot, kVpartEmpty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    m = wave_max(m);
    d = wave_max(d);
    lost = __any(lost) ? 1 : 0;
    __shared__ double s_m[BLK / 64], s_d[BLK / 64];
    __shared__ int s_l[BLK / 64];
    if ((threadIdx.x & 63) == 0) { s_m[threadIdx.x >> 6] = m; s_d[threadIdx.x >> 6] = d; s_l[threadIdx.x >> 6] = lost; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < BLK / 64; ++k) { m = fmax(m, s_m[k]); d = fmax(d, s_d[k]); lost |= s_l[k]; }
        if (lost) c0.status = SPHX_ERR_DIVERGED;
        clock_step(clk, c0, q, ph, sqrt(m), fl, -1, track ? sqrt(d) : -1.0, rebuilt, t.half_skin);
    }
}
template <int BLK = kBlock>
__device__ __forceinline__ void continuity_tail(Clock *clk, int q, const Phys &ph, const FluidTmp &t, int nb, int rebuilt = 0)
{
    if constexpr (BLK != kBlock) {
        if constexpr (BLK < kBlock) continuity_tail_small<BLK>(clk, q, ph, t, nb, rebuilt);
        else continuity_tail_wide<BLK>(clk, q, ph, t, nb, rebuilt);
        return;
    }
    if (!clk->run[q]) {
        if (threadIdx.x == 0) clk->run[1 - q] = 0;  // idle slot keeps the following slots idle
        return;
    }
    Clock c0;
    int fl = 0;
    if (threadIdx.x == 0) { c0 = *clk; fl = *t.flags; }
    double m = 0.0, d = 0.0;
    int lost = 0;
    const bool track = t.half_skin >= 0.0;
    for (int k = threadIdx.x; k < nb; k += kBlock) {
        if (track) d = fmax(d, t.dpart[k]);  // written by pass CD, a kernel ago
        unsigned long long *slot = reinterpret_cast<unsigned long long *>(&t.vpart[k]);
        unsigned long long bits;
        unsigned spins = 0;
        while ((bits = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == kVpartEmpty) {
            __builtin_amdgcn_s_sleep(2);
            if (++spins > (1u << 22)) { lost = 1; break; }  // never hang the device on a protocol bug
        }
        if (!lost) m = fmax(m, __longlong_as_double((long long)bits));
        __hip_atomic_store(slot, kVpartEmpty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    m = wave_max(m);
    d = wave_max(d);
    lost = __any(lost) ? 1 : 0;
    __shared__ double s_m[kBlock / 64], s_d[kBlock / 64];
    __shared__ int s_l[kBlock / 64];
    if ((threadIdx.x & 63) == 0) { s_m[threadIdx.x >> 6] = m; s_d[threadIdx.x >> 6] = d; s_l[threadIdx.x >> 6] = lost; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kBlock / 64; ++k) { m = fmax(m, s_m[k]); d = fmax(d, s_d[k]); lost |= s_l[k]; }
        if (lost) c0.status = SPHX_ERR_DIVERGED;
        clock_step(clk, c0, q, ph, sqrt(m), fl, -1, track ? sqrt(d) : -1.0, rebuilt, t.half_skin);
    }
}

// Skinned slabs: the local maxima the step's all-reduce needs -- max |v| and max drift of the owned particles -- are
// reduced by a tail workgroup of pass E (same hand-over as continuity_tail: every vpart entry is its own "ready" flag)
// instead of a one-workgroup kernel behind it.  out[0..1] = {max |v|, max drift}; a stopped loop reports zeros.
__device__ __forceinline__ void slab_seal_tail(const Clock *clk, int q, const FluidTmp &t, int nb)
{
    if (!clk->run[q]) {
        if (threadIdx.x == 0) { t.seal_out[0] = 0.0; t.seal_out[1] = 0.0; }
        return;
    }
    double m = 0.0, d = 0.0;
    int lost = 0;
    for (int k = threadIdx.x; k < nb; k += kBlock) {
        d = fmax(d, t.dpart[k]);  // written by pass CD, a kernel ago
        unsigned long long *slot = reinterpret_cast<unsigned long long *>(&t.vpart[k]);
        unsigned long long bits;
        unsigned spins = 0;
        while ((bits = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == kVpartEmpty) {
            __builtin_amdgcn_s_sleep(2);
            if (++spins > (1u << 22)) { lost = 1; break; }  // never hang the device on a protocol bug
        }
        if (!lost) m = fmax(m, __longlong_as_double((long long)bits));
        __hip_atomic_store(slot, kVpartEmpty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    m = wave_max(m);
    d = wave_max(d);
    lost = __any(lost) ? 1 : 0;
    __shared__ double s_m[kBlock / 64], s_d[kBlock / 64];
    __shared__ int s_l[kBlock / 64];
    if ((threadIdx.x & 63) == 0) { s_m[threadIdx.x >> 6] = m; s_d[threadIdx.x >> 6] = d; s_l[threadIdx.x >> 6] = lost; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kBlock / 64; ++k) { m = fmax(m, s_m[k]); d = fmax(d, s_d[k]); lost |= s_l[k]; }
        t.seal_out[0] = lost ? INFINITY : sqrt(m);  // (a lost hand-over poisons the maximum: the clock raises DIVERGED)
        t.seal_out[1] = sqrt(d);
    }
}

// tail: 1 = the launch has one workgroup more than the pass needs; it runs continuity_tail (2: slab_seal_tail)
// WALK: the large-channel form of the walk (see the "_w" kernels): entries ahead, fluid / wall loops, fold hoisted
// (bid, nb: this workgroup's index among the nb workgroups of the pass; c_*: the LDS tile arrays of the calling kernel)
// CODED: slot-coded list entries (kSlotCodes)
// REBIN (compact kernels, k_continuity_rebin): the pass also re-bins.  Pass CD of the step has taken the histogram of the new
// cells (k_forces_hist).  The slot of a particle in the new ordering is canonical -- new cell first, then ascending id
// (reorder_body) -- so nobody has to wait for anybody: every workgroup scans the histogram in LDS, the lanes of a particle
// count the members of its new cell with a smaller id among the particles BINNED in the 3 x 3 cells around that cell (three
// runs of the old layout, see rebin_near), and the lead lane stores the persistent fields straight into the other state and
// layout `d`.  Histogram, new cells, ids and the runs are requested in the prologue, the first kFoldAhead candidates of every
// lane in front of the walk.  Workgroup 0 stores the new cell ranges.
constexpr int kFoldAhead = 8;
// What a thread holds of the folded re-binning: the particle's new cell and id (every lane of the group), what only the lead lane
// moves, this thread's share of the histogram, the three runs of the old layout that hold whoever can land in the new cell, and
// the new cells and ids of the lane's first kFoldAhead candidates
struct FoldRebin {
    static constexpr int kPer = kFoldCells / kBlock;
    int cnew = 0, id = 0, cold = 0, lo[3] = {0, 0, 0}, n[3] = {0, 0, 0}, hist[kPer], ccell[kFoldAhead], cid[kFoldAhead];
    double mass = 0.0;
    __device__ __forceinline__ int candidates() const { return n[0] + n[1] + n[2]; }
    __device__ __forceinline__ int slot(int v) const { return ranges_index(lo[0], lo[1], lo[2], n[0], n[1], v); }
};
// load: what the prologue requests ...
// (io: the particle's own slot, own_slot -- every lane loads, only the lead lane of an active particle uses cold and mass)
__device__ __forceinline__ void fold_load(FoldRebin &r, const Grid &g, const FluidSet &s, const FluidTmp &t, int io)
{
    r.cnew = t.cellid[io];
    r.id = s.id[io];
    r.cold = s.cell[io];
    r.mass = s.mass[io];
#pragma unroll
    for (int j = 0; j < FoldRebin::kPer; ++j) r.hist[j] = t.count[min((int)threadIdx.x * FoldRebin::kPer + j, g.ncells)];
}
// ... and, behind the clock's loads (these wait for the new cell), the three runs
__device__ __forceinline__ void fold_runs(FoldRebin &r, const Grid &g, const FluidSet &s)
{
    r.cnew = min(max(r.cnew, 0), g.ncells - 1);  // (slots beyond the population hold no cell: any valid one keeps the loads in bounds)
    const int cxn = r.cnew / g.ncy, cyn = r.cnew - cxn * g.ncy;
    const int cylo = max(cyn - 1, 0), cyhi = min(cyn + 1, g.ncy - 1);
#pragma unroll
    for (int ox = -1; ox <= 1; ++ox) {
        int col = cxn + ox;  // (at least three columns, periodic: the three are distinct -- neighbour_column's tests are not needed)
        if (col < 0) col += g.ncx;
        else if (col >= g.ncx) col -= g.ncx;
        r.lo[ox + 1] = s.start[col * g.ncy + cylo];
        r.n[ox + 1] = s.start[col * g.ncy + cyhi + 1] - r.lo[ox + 1];
    }
}
// scan: exclusive scan of the histogram -- the cell ranges of the new ordering, r_start[ncells] = the population (workgroup 0 stores
// them to the new layout d) -- and the requests for the first candidates of every lane (slot 0 stands in where a lane has fewer)
template <int LPP>
__device__ __forceinline__ void fold_scan(FoldRebin &r, const Grid &g, const FluidSet &s, const FluidTmp &t, const FluidSet &d, int bid,
                                          int sub, int *r_start, int *r_wave)
{
    int sum = 0, total;
#pragma unroll
    for (int j = 0; j < FoldRebin::kPer; ++j) {
        const int v = (int)threadIdx.x * FoldRebin::kPer + j < g.ncells ? r.hist[j] : 0;
        r.hist[j] = sum;
        sum += v;
    }
    const int base = block_exclusive_scan_t<kBlock>(sum, total, r_wave);
#pragma unroll
    for (int j = 0; j < FoldRebin::kPer; ++j) {
        const int c = (int)threadIdx.x * FoldRebin::kPer + j;
        if (c <= g.ncells) {
            r_start[c] = base + r.hist[j];
            if (bid == 0) d.start[c] = base + r.hist[j];
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kFoldAhead; ++j) {
        const int v = sub + j * LPP;
        const int k = v < r.candidates() ? r.slot(v) : 0;
        r.ccell[j] = t.cellid[k];
        r.cid[j] = s.id[k];
    }
}
// rank: the members of the particle's new cell with a smaller id, counted by the lanes of its group
template <int LPP>
__device__ __forceinline__ int fold_rank(const FoldRebin &r, const FluidSet &s, const FluidTmp &t, int sub, bool active)
{
    int rank = 0;
    if (active) {
        const int nv = r.candidates();
#pragma unroll
        for (int j = 0; j < kFoldAhead; ++j) rank += (sub + j * LPP < nv && r.ccell[j] == r.cnew && r.cid[j] < r.id) ? 1 : 0;
        for (int v = sub + kFoldAhead * LPP; v < nv; v += LPP) {
            const int k = r.slot(v);
            rank += (t.cellid[k] == r.cnew && s.id[k] < r.id) ? 1 : 0;
        }
    }
    return (int)group_sum<LPP>((double)rank);  // (exact: a handful)
}
// store (lead lane): the persistent fields of particle i straight into their slot of the other state and layout d
__device__ __forceinline__ void fold_store(const FoldRebin &r, const Grid &g, const FluidTmp &t, const FluidSet &d, const int *r_start,
                                           int rank, int i, const double2 pn, const double2 vi, double drho_new)
{
    const int dst = r_start[r.cnew] + rank;
    // (the clock does not test the drift of the step that re-bins: a particle that is not where the count looked for it
    //  must not take a slot somebody else may own -- pass CD has raised the flag already, the step ends in SPHX_ERR_GRID)
    if (rebin_near(g, r.cold, r.cnew) && (unsigned)dst < (unsigned)t.cap) {
        d.pos[dst] = pn;
        d.vel[dst] = vi;
        if (d.posb) d.posb[dst] = pn;
        d.drho[dst] = drho_new;
        d.mass[dst] = r.mass;
        d.id[dst] = r.id;
        d.cell[dst] = r.cnew;
        t.src_of[dst] = i;
    } else {
        atomicOr(t.flags, 1);
    }
}

// Tiled form of pass E: the cell histogram goes through LDS.  A particle's new cell lies within a cell or two of the workgroup's
// old ones, so the workgroup counts into a window of kCols x kRows cells around its first particle's cell with LDS atomics and
// adds the window to the global histogram once -- 6 M global atomics, ~60 per cell and step, were 135 us of the pass on every
// step that takes the histogram (6 M particles).  Anything outside the window is counted globally as before.
struct HistWindow {
    static constexpr int kCols = 3, kRows = 48, kLead = 4, kCells = kCols * kRows;
    int cx0 = 0, r0 = 0;
    // open: place the window and clear it (a barrier has to follow: the one behind the tile staging)
    __device__ __forceinline__ void open(const Grid &g, int c_first, int *h_win)
    {
        cx0 = c_first / g.ncy - 1;
        r0 = c_first % g.ncy - kLead;
        if (threadIdx.x < kCells) h_win[threadIdx.x] = 0;
    }
    // count: one particle in cell (cx, cy); false: outside the window
    __device__ __forceinline__ bool count(const Grid &g, int cx, int cy, int *h_win) const
    {
        int dcol = cx - cx0;
        if (g.periodic) dcol = dcol < 0 ? dcol + g.ncx : (dcol >= g.ncx ? dcol - g.ncx : dcol);
        const int drow = cy - r0;
        if ((unsigned)dcol >= (unsigned)kCols || (unsigned)drow >= (unsigned)kRows) return false;
        atomicAdd(&h_win[dcol * kRows + drow], 1);
        return true;
    }
    // flush (behind a barrier): the window's counts into the global histogram
    __device__ __forceinline__ void flush(const Grid &g, const FluidTmp &t, const int *h_win) const
    {
        if (threadIdx.x >= kCells) return;
        const int v = h_win[threadIdx.x];
        if (v) {
            int col = cx0 + (int)threadIdx.x / kRows;
            if (g.periodic) col = col < 0 ? col + g.ncx : (col >= g.ncx ? col - g.ncx : col);
            const int row = r0 + (int)threadIdx.x % kRows;
            atomicAdd(&t.count[col * g.ncy + row], v);  // (v > 0: somebody's cell, so col and row are inside the grid)
        }
    }
};
// BLK: the threads of the workgroup (other than 256: the compact form without the re-binning)
template <int LPP, bool WALK, int TILE, bool CODED = false, bool REBIN = false, int BLK = kBlock>
__device__ __forceinline__ void continuity_body(Clock *clk, int q, const Grid &g, const Phys &ph, const FluidSet &s,
                                                const FluidTmp &t, const Walls &w, int do_hist, int tail, PassWg bid, int nb,
                                                double2 *c_pos, double2 *c_vel, double *c_vol, int next_half = 0,
                                                const FluidSet &d = FluidSet{})
{
    static_assert(!CODED || (WALK && TILE == kSlotCodes), "slot-coded lists: this pass stages the whole layout");
    static_assert(!REBIN || (!WALK && TILE == 0 && LPP >= 16), "the folded re-binning belongs to the compact kernels");
    static_assert(BLK == kBlock || (!WALK && !REBIN && LPP >= 16), "smaller workgroups: the compact passes only");
    const int blk = xcd_block(bid, nb);
    const int tid = blk * BLK + threadIdx.x;
    const int i = tid / LPP, sub = tid % LPP;
    const bool in_cap = i < t.cap;
    if (WALK && beyond_population<LPP>(clk, t, blk)) {  // nothing here: only the workgroup's entry of the max |v|^2 reduction is owed
        if (threadIdx.x == 0 && clk->run[q] && !next_half) {
            if (tail) __hip_atomic_store(reinterpret_cast<unsigned long long *>(&t.vpart[blk]), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else t.vpart[blk] = 0.0;
        }
        return;
    }
    // kRowsAhead: this pass reads the clock through a pointer somebody writes (the tail workgroup), so with vector loads, which
    // come back in order -- the words the pass waits for first are asked for first, in one go
    constexpr bool kAhead = !WALK && kRowsAhead<LPP>;
    ListHead head;
    if (kAhead) {
        head.request(clk, q, t.nl_cnt, t.nl_idx, t.nl_stride, tid);
        SPHX_ARGS_BATCH("s"(s.pos), "s"(t.veln), "s"(t.a), "s"(t.cap), "s"(t.posn), "s"(t.vol), "s"(t.vpart), "s"(w.pos), "s"(w.a),
                        "s"(g.DL), "s"(g.half_DL), "s"(g.own_by_cell), "s"(ph.kc.h), "s"(ph.kc.inv_h), "s"(ph.kc.sigma_over_h));
    }
    const int run_first = head.run, n_first = head.n;
    const double dt_first = head.dt;
    const int io = kAhead ? own_slot<LPP>(i, t.cap) : i;  // (the compact form: no test around the own records)
    const double2 pi = (kAhead || in_cap) ? s.pos[io] : make_double2(0.0, 0.0);
    const double2 vi = (kAhead || in_cap) ? t.veln[io] : make_double2(0.0, 0.0);
    const int packed = kAhead ? head.packed : t.nl_cnt[tid];
    const int nn_all = list_rows(packed);
    // (WALK: the first two words of the packed fluid rows, see FluidTmp::nl_pk)
    const FirstRows<LPP> first = kAhead ? FirstRows<LPP>(head.e0, head.e1) : FirstRows<LPP>(WALK ? t.nl_pk : t.nl_idx, t.nl_stride, tid);
    const bool lead = kAhead || (in_cap && sub == 0);
    const double4 a_own = lead ? t.a[io] : make_double4(0.0, 0.0, 0.0, 0.0);
    const double rhoh_i = a_own.z;
    const double2 pn = (lead && (do_hist || REBIN)) ? t.posn[io] : make_double2(0.0, 0.0);  // (requested whenever a histogram is possible)
    FoldRebin fold;
    if (REBIN) fold_load(fold, g, s, t, io);
    const TileMap layout = (WALK && TILE > 0) ? tile_map_of(t, blk) : TileMap{0, 0, 0, 0, 0, 0};
    const double dt = kAhead ? dt_first : clk->dt;
    const bool want_out = !WALK || step_outputs_wanted(clk, t);
    const int cell_own = (g.own_by_cell && lead) ? s.cell[io] : 0;
    if (kAhead) requests_issued();
    if (REBIN) fold_runs(fold, g, s);
    if (!(kAhead ? run_first : clk->run[q])) return;
    const int n_now = kAhead ? n_first : clk->n;
    const bool active = i < n_now;
    double rate = 0.0;
    const double xi = pi.x, yi = pi.y, vxi = vi.x, vyi = vi.y;
    // do_hist: 1 = this step re-bins (static schedule); 100 + K = dynamic context: the K-th step since the last re-binning will
    // re-bin whatever the drift says, so its histogram can be taken here (k_bin then skips)
    const bool hist = do_hist == 1 || (do_hist >= 100 && clk->pos_count >= do_hist - 101);
    constexpr bool kHistWindow = WALK && TILE > 0;  // (tiled form: the histogram goes through LDS)
    __shared__ int h_win[kHistWindow ? HistWindow::kCells : 1];
    HistWindow window;
    if (kHistWindow && hist) window.open(g, s.cell[min(blk * (kBlock / LPP), max(n_now - 1, 0))], h_win);
    // The workgroup's entry of the max |v|^2 reduction needs nothing but the particles' own records.  The compact kernels (small
    // channels) publish it HERE, before the walk, so that the tail workgroup reduces and advances the clock while the walks are
    // still running -- the clock update used to start when the last workgroup had finished (C1 14.55 -> 14.25, C2 17.55 -> 17.35
    // us/step).  (Every workgroup has read what it needs of the clock by the time it publishes -- dt, the run flag, the
    // population are read above -- and the tail cannot finish before all of them have published.)  The large-channel forms
    // publish at the end as before: there the extra barrier in front of the walk costs more than the early clock gains (C3
    // 44.5 -> 45.2 us/step with it).
    auto publish_vmax = [&]() {
        double v2 = 0.0;
        if (active && sub == 0 && owns(g, xi, cell_own)) {
            v2 = vxi * vxi + vyi * vyi;
            if (v2 != v2) v2 = INFINITY;  // NaN poisons the max on purpose
        }
        v2 = wave_max(v2);
        auto store = [&](int k, double m) {
            if (tail)
                __hip_atomic_store(reinterpret_cast<unsigned long long *>(&t.vpart[k]), (unsigned long long)__double_as_longlong(m),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else
                t.vpart[k] = m;
        };
        if constexpr (BLK == 64) {  // one wave: its maximum is the workgroup's -- no LDS, no barrier
            if (threadIdx.x == 0 && !next_half) store(blk, v2);
        } else {
            __shared__ double s_max[BLK / 64];
            if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = v2;
            __syncthreads();
            if (threadIdx.x == 0 && !next_half) {  // (an inner sub-step leaves the "ready" slots of the step's last pass E alone)
                double m = s_max[0];
                for (int k = 1; k < BLK / 64; ++k) m = fmax(m, s_max[k]);
                store(blk, m);
            }
        }
    };
    if (!WALK) publish_vmax();
    __shared__ int r_start[REBIN ? kFoldCells + 1 : 1], r_wave[REBIN ? kBlock / 64 + 1 : 1];
    if (REBIN) fold_scan<LPP>(fold, g, s, t, d, bid.j, sub, r_start, r_wave);
    if (WALK) {
        const int rows = active ? nn_all : 0, rows_fl = active ? list_fluid_rows(packed) : 0;
        struct Nb {  // what the pass reads of a fluid neighbour
            double2 p, v;
            double vol;
        };
        TileMap tm{0, 0, 0, 0, 0, 0};
        if (TILE > 0) {
            tm = staged_map<LPP>(layout, blk, n_now, TILE);
            stage_tile<TILE>(tm, [&](int k) { return Nb{s.pos[k], t.veln[k], t.vol[k]}; },
                             [&](int sl, const Nb &n) { c_pos[sl] = n.p; c_vel[sl] = n.v; c_vol[sl] = n.vol; });
        }
        auto fetch_near = [&](int e) { return Nb{lds_double2(c_pos, e), lds_double2(c_vel, e), lds_double(c_vol, e)}; };
        auto fetch = [&](int k) {
            if (TILE > 0) {  // (early return, not if/else: see k_kgc_w)
                const int slot = tm.slot(k);
                if (slot >= 0) return fetch_near(slot);
            }
            return Nb{s.pos[k], t.veln[k], t.vol[k]};
        };
        auto term = [&](double dx, double dy, double ujx, double ujy, double Volj) {
            continuity_add(ph.kc, dx, dy, vxi, vyi, ujx, ujy, Volj, rate);
        };
        auto fetch_code = [&](int e) {  // (CODED)
#if SPHX_EXP_PRETEND_COMPLETE_TILE & 8
            e = min(e, kSlotCodes - 1);  // MEASUREMENT ONLY, see k_forces_w
#endif
            if (e < kSlotCodes) return fetch_near(e);
            const int k = wrap_index(i + e - kCodeBias, n_now);
            return Nb{s.pos[k], t.veln[k], t.vol[k]};
        };
        const bool seam = __any(active && near_seam(g, xi));
        const bool all_near = CODED && !__any(packed & kFarTileBit);  // (see kFarTileBit)
        walk_fluid_forms<CODED>(g, t, tid, i, n_now, rows_fl, first.e0, first.e1, xi, seam, all_near, fetch_near, fetch_code, fetch,
                                [&](const Nb &n, double dx) { term(dx, yi - n.p.y, n.v.x, n.v.y, n.vol); });
        walk_wall_rows(t, tid, rows_fl, rows, [&](int k) {
            const double2 pj = w.pos[k];
            const double4 wj = w.a[k];  // {Vol, vx, vy, -}; the wall presents its velocity mirrored through the particle's
            term(min_image(g, xi - pj.x), yi - pj.y, 2.0 * wj.y - vxi, 2.0 * wj.z - vyi, wj.x);
        });
    } else if (active) {
        auto term = [&](const double2 pj, const double2 vj, double Volj) {
            continuity_add(ph.kc, pair_dx<LPP>(g, xi - pj.x), yi - pj.y, vxi, vyi, vj.x, vj.y, Volj, rate);
        };
        if (kAhead) {
            // rows 0 and 1: both rows' records in one wave -- position, volume and velocity of either kind of neighbour through
            // selected pointers (a wall's record is {Vol, vx, vy, -}), so that the requests need no branch
            double2 pj_[2], uj_[2];
            double Vj_[2];
            bool wall_[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int e = m < nn_all ? (m == 0 ? first.e0 : first.e1) : 0;
                wall_[m] = (e & kWallBit) != 0;
                const int k = m < nn_all ? (e & (kWallBit - 1)) : i;
                pj_[m] = (wall_[m] ? w.pos : (const double2 *)s.pos)[k];
                Vj_[m] = *(wall_[m] ? &w.a[k].x : (const double *)&t.vol[k]);
                uj_[m].x = *(wall_[m] ? &w.a[k].y : (const double *)&t.veln[k].x);
                uj_[m].y = *(wall_[m] ? &w.a[k].z : (const double *)&t.veln[k].y);
            }
            requests_issued();
#pragma unroll
            for (int m = 0; m < 2; ++m)
                if (m < nn_all)
                    term(pj_[m], wall_[m] ? make_double2(2.0 * uj_[m].x - vxi, 2.0 * uj_[m].y - vyi) : uj_[m], Vj_[m]);  // mirrored wall velocity
        }
        for (int m = kAhead ? 2 : 0; m < nn_all; ++m) {
            const int e = first.row(m, t.nl_idx, t.nl_stride, tid);
            const bool wall = (e & kWallBit) != 0;
            const int k = e & (kWallBit - 1);
            const double2 pj = (wall ? w.pos : (const double2 *)s.pos)[k];
            double2 vj;
            double Volj;
            if (wall) {
                const double4 wj = w.a[k];  // {Vol, vx, vy, -}
                Volj = wj.x;
                vj = make_double2(2.0 * wj.y - vxi, 2.0 * wj.z - vyi);  // mirrored wall velocity
            } else {
                Volj = t.vol[k];
                vj = t.veln[k];
            }
            term(pj, vj, Volj);
        }
    }
    rate = group_sum<LPP>(rate);
    const int r_rank = REBIN ? fold_rank<LPP>(fold, s, t, sub, active) : 0;
    if (active && sub == 0) {
        const double rhoh = rhoh_i;
        const double drho_new = rate * rhoh;
        double rho = rhoh + drho_new * (0.5 * dt);
        if (rho < 1e-10) rho = ph.rho0;
        t.drhon[i] = drho_new;
        if (want_out) {
            t.rho_out[i] = rho;
            t.p_out[i] = eos_pressure(rho, ph.rho0, ph.p0);
        }
        if (next_half) {  // dual-rate loop: another sub-step follows, with the density carried on (not re-summed)
            double rhoh2, p2;
            half_state(ph, rho, drho_new, dt, rhoh2, p2);
            t.a[i] = make_double4(a_own.x, p2, rhoh2, rho);
        }
        if (REBIN) fold_store(fold, g, t, d, r_start, r_rank, i, pn, vi, drho_new);
        if (hist) {
            int cx, cy;
            cell_of(g, pn.x, pn.y, cx, cy);
            const int c = cx * g.ncy + cy;
            t.cellid[i] = c;
            if (!(kHistWindow && window.count(g, cx, cy, h_win))) atomicAdd(&t.count[c], 1);
        }
    }
    if (WALK) publish_vmax();  // (its barrier also closes the window histogram)
    if (kHistWindow && hist) window.flush(g, t, h_win);
}

// (waves_per_eu: the large-channel forms of passes E and A fit eight waves per SIMD by their vector registers (62-67) but took 106
//  scalar registers -- seven waves; they are latency-bound, the eighth wave is worth 9 % of pass E at 6 M particles.  Asked for,
//  the compiler finds a 78-SGPR allocation without spills.)
template <int LPP, bool WALK, int TILE, bool CODED = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(WALK ? 8 : 1))) void k_continuity(Clock *clk, int q, Grid g, Phys ph,
                                                       FluidSet s, FluidTmp t, Walls w, int do_hist, int tail, int next_half)
{
    constexpr int kSlots = TILE > 0 ? TILE : 1;
    __shared__ double2 c_pos[kSlots], c_vel[kSlots];
    __shared__ double c_vol[kSlots];
    const int nb = (int)gridDim.x - (tail ? 1 : 0);
    if (tail && (int)blockIdx.x == nb) {
        if (tail == 2) slab_seal_tail(clk, q, t, nb);
        else continuity_tail(clk, q, ph, t, nb);
        return;
    }
    continuity_body<LPP, WALK, TILE, CODED>(clk, q, g, ph, s, t, w, do_hist, tail, (int)blockIdx.x, nb, c_pos, c_vel, c_vol, next_half);
}

// Pass E of the compact kernels at 16 / 32 lanes per particle with leading arguments (shape: the workgroups of the pass, tail)
template <int LPP, int BLK = kBlock>
__global__ __launch_bounds__(BLK) void k_continuity_compact(Clock *clk, int q, int shape, int *nl_cnt, int *nl_idx, int nl_stride,
                                                               int cap, double2 *pos, double2 *veln, Grid g, Phys ph, FluidSet s,
                                                               FluidTmp t, Walls w, int do_hist, int next_half)
{
    t.nl_cnt = nl_cnt; t.nl_idx = nl_idx; t.nl_stride = nl_stride; t.cap = cap; s.pos = pos; t.veln = veln;
    const int nb = shape_blocks(shape), tail = shape_flag(shape);
    if (tail && (int)blockIdx.x == nb) {
        if constexpr (BLK == kBlock) {
            if (tail == 2) { slab_seal_tail(clk, q, t, nb); return; }  // (slabs run 256 threads)
        }
        continuity_tail<BLK>(clk, q, ph, t, nb);
        return;
    }
    continuity_body<LPP, false, 0, false, false, BLK>(clk, q, g, ph, s, t, w, do_hist, tail, (int)blockIdx.x, nb, nullptr, nullptr, nullptr,
                                                      next_half);
}

// Small channels, the step that re-bins: pass E with the re-binning folded in (continuity_body, REBIN) and the clock in the tail
// workgroup, which advances it as k_clock_scan does on such a step.  d: the state / layout the new ordering goes to.
template <int LPP>
__global__ __launch_bounds__(kBlock) void k_continuity_rebin(Clock *clk, int q, int shape, int *nl_cnt, int *nl_idx, int nl_stride,
                                                             int cap, double2 *pos, double2 *veln, Grid g, Phys ph, FluidSet s,
                                                             FluidTmp t, Walls w, FluidSet d)
{
    t.nl_cnt = nl_cnt; t.nl_idx = nl_idx; t.nl_stride = nl_stride; t.cap = cap; s.pos = pos; t.veln = veln;
    const int nb = shape_blocks(shape);
    if ((int)blockIdx.x == nb) {
        continuity_tail(clk, q, ph, t, nb, 1);
        return;
    }
    continuity_body<LPP, false, 0, false, true>(clk, q, g, ph, s, t, w, 0, 1, (int)blockIdx.x, nb, nullptr, nullptr, nullptr, 0, d);
}

// Small channels, steps that do not re-bin: pass E of this step and pass A of the NEXT step in one launch, side by
// side.  Both depend only on pass CD (E on the kicked velocities, A on the new positions) and not on each other, and at
// a few thousand particles the chip is mostly idle, so the launch takes as long as the longer of the two instead of
// their sum plus a kernel boundary.  Workgroups [0, nb): pass E on state s with the step's list (t); [nb, 2 nb): pass A
// on the new state s_next, walking the superset list, into the other list / record buffers (t_next) -- without the
// half-step density and pressure, which need the next step's dt (the tail workgroup of this very launch computes it):
// pass B of the next step closes that (k_kgc, finish_half); workgroup 2 nb: the clock (continuity_tail).
// The A half starts at physical block nb and numbers its blocks from there (xcd_block): its lists and records are stored
// by the XCD that reads them in passes B, CD and E.  kFusedUnaligned (SPHX_DEBUG_SWITCHES=no_xcd_align, a bit of the launch's
// flag word above the tail's codes) numbers it as if it began at block 0, as it did before.
constexpr int kFusedTail = 1, kFusedUnaligned = 4;
__device__ __forceinline__ int fused_first_a(int flags, int nb) { return flags & kFusedUnaligned ? 0 : nb; }
template <int LPP, int BLK = kBlock>
__global__ __launch_bounds__(BLK) void k_continuity_density(Clock *clk, int q, int shape, int *e_cnt, int *e_idx, int *a_cnt,
                                                               int *a_idx, int e_stride, int a_stride, Grid g, Phys ph, FluidSet s,
                                                               FluidTmp t, Walls w, FluidSet s_next, FluidTmp t_next)
{
    // (fourteen dwords hold the lists of both halves and nothing else: the own records of either go out behind the scalar batch;
    //  the two strides side by side: an int in front of a pointer costs a dword of padding, and the last one would miss the preload)
    t.nl_cnt = e_cnt; t.nl_idx = e_idx; t.nl_stride = e_stride;
    t_next.sl_cnt = a_cnt; t_next.sl_idx = a_idx; t_next.nl_stride = a_stride;
    const int nb = shape_blocks(shape), with_tail = shape_flag(shape) & kFusedTail;  // (with_tail = 0: kernel timing, the clock must not advance)
    const int b = (int)blockIdx.x;
    if (with_tail && b == 2 * nb) {
        continuity_tail<BLK>(clk, q, ph, t, nb);
        return;
    }
    if (b < nb) continuity_body<LPP, false, 0, false, false, BLK>(clk, q, g, ph, s, t, w, 0, with_tail, b, nb, nullptr, nullptr, nullptr);
    else density_body<LPP, 2, BLK>(clk, q, g, ph, s_next, t_next, w, PassWg(b - nb, fused_first_a(shape_flag(shape), nb)), nb, false);
}

// Batches (Members): pass E of the compact kernels (the tail workgroup of member m is workgroup nb of row m: it waits for the
// per-workgroup maxima of its own member only) and the fused E|A launch
template <int LPP>
__global__ __launch_bounds__(kBlock) void k_continuity_b(Members mb, int q, Grid g, FluidSet s, FluidTmp t, Walls w,
                                                         int do_hist, int tail)
{
    const int m = (int)blockIdx.y;
    Clock *clk = mb.clk + m;
    const Phys ph = mb.ph[m];
    const FluidTmp tm = member_tmp(mb, m, t);
    const int nb = (int)gridDim.x - (tail ? 1 : 0);
    if (tail && (int)blockIdx.x == nb) {
        continuity_tail(clk, q, ph, tm, nb);
        return;
    }
    continuity_body<LPP, false, 0>(clk, q, g, ph, member_set(mb, m, s), tm, w, do_hist, tail, (int)blockIdx.x, nb, nullptr,
                                   nullptr, nullptr);
}
template <int LPP>
__global__ __launch_bounds__(kBlock) void k_continuity_density_b(Members mb, int q, Grid g, FluidSet s, FluidTmp t, Walls w,
                                                                 FluidSet s_next, FluidTmp t_next, int with_tail)
{
    const int m = (int)blockIdx.y;
    Clock *clk = mb.clk + m;
    const Phys ph = mb.ph[m];
    const int nb = ((int)gridDim.x - with_tail) / 2;
    const int b = (int)blockIdx.x;
    if (with_tail && b == 2 * nb) {
        continuity_tail(clk, q, ph, member_tmp(mb, m, t), nb);
        return;
    }
    if (b < nb) continuity_body<LPP, false, 0>(clk, q, g, ph, member_set(mb, m, s), member_tmp(mb, m, t), w, 0, with_tail, b, nb, nullptr, nullptr, nullptr);
    else density_body<LPP, 2>(clk, q, g, ph, member_set(mb, m, s_next), member_tmp(mb, m, t_next), w, b - nb, nb, false);
}

// the same with the large-channel forms of the two passes (mid-size channels: 4-8 lanes per particle, clock in the tail)
template <int LPP>
__global__ __launch_bounds__(kBlock) void k_continuity_density_w(Clock *clk, int q, Grid g, Phys ph, FluidSet s, FluidTmp t,
                                                                 Walls w, FluidSet s_next, FluidTmp t_next, int tail_flags)
{
    const int with_tail = tail_flags & kFusedTail;
    const int nb = ((int)gridDim.x - with_tail) / 2;  // (with_tail = 0: kernel timing, the clock must not advance)
    const int b = (int)blockIdx.x;
    if (with_tail && b == 2 * nb) {
        continuity_tail(clk, q, ph, t, nb);
        return;
    }
    if (b < nb) continuity_body<LPP, true, 0>(clk, q, g, ph, s, t, w, 0, with_tail, b, nb, nullptr, nullptr, nullptr);
    else density_walk_body<LPP>(clk, q, g, ph, s_next, t_next, w, PassWg(b - nb, fused_first_a(tail_flags, nb)), nb, false);
}

// standalone cell histogram (context creation, wall grid, slab steps): same binning as pass E
__global__ __launch_bounds__(kBlock) void k_bin(const Clock *clk, int q, Grid g, int n_fixed, const double2 *pos,
                                                int *cellid, int *count)
{
    if (clk && !slot_active(clk, q)) return;
    const int n = clk ? clk->n : n_fixed;
    // grid-stride: dynamic contexts launch the re-binning kernels on every step with a small grid, so that the
    // launches that skip cost next to nothing
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        int cx, cy;
        const double2 p = pos[i];
        cell_of(g, p.x, p.y, cx, cy);
        const int c = cx * g.ncy + cy;
        cellid[i] = c;
        atomicAdd(&count[c], 1);
    }
}

// block-wide exclusive scan of one int per thread (kScanBlock threads); returns the block total
__device__ __forceinline__ int block_exclusive_scan(int v, int &total, int *s_wave /*[17]*/)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(inc, off);
        if (lane >= off) inc += o;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    if (wave == 0) {
        const int ws = lane < kScanBlock / 64 ? s_wave[lane] : 0;
        int winc = ws;
#pragma unroll
        for (int off = 1; off < kScanBlock / 64; off <<= 1) {
            const int o = __shfl_up(winc, off);
            if (lane >= off) winc += o;
        }
        if (lane < kScanBlock / 64) s_wave[lane] = winc - ws;  // exclusive wave offsets
        if (lane == kScanBlock / 64 - 1) s_wave[kScanBlock / 64] = winc;
    }
    __syncthreads();
    const int res = s_wave[wave] + inc - v;
    total = s_wave[kScanBlock / 64];
    __syncthreads();
    return res;
}

// exclusive scan of count[0..n) into start[0..n], by one block
__device__ __forceinline__ void scan_counts(const int *count, int *start, int n)
{
    __shared__ int s_wave[kScanBlock / 64 + 1];
    int carry = 0;
    for (int base = 0; base < n; base += kScanBlock) {
        const int idx = base + (int)threadIdx.x;
        const int v = idx < n ? count[idx] : 0;
        int total;
        const int ex = block_exclusive_scan(v, total, s_wave);
        if (idx < n) start[idx] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) start[n] = carry;
}

// big grids: tile-local exclusive scan (one 1024-cell tile per block) + tile sums
__global__ __launch_bounds__(kScanBlock) void k_scan_tiles(const Clock *clk, int q, const int *count, int *start,
                                                           int *tile_sum, int n)
{
    if (clk && !slot_active(clk, q)) return;
    __shared__ int s_wave[kScanBlock / 64 + 1];
    const int idx = blockIdx.x * kScanBlock + (int)threadIdx.x;
    const int v = idx < n ? count[idx] : 0;
    int total;
    const int ex = block_exclusive_scan(v, total, s_wave);
    if (idx < n) start[idx] = ex;
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kScanBlock) void k_scan_add(const Clock *clk, int q, int *start, const int *tile_off,
                                                         int n, int n_tiles)
{
    if (clk && !slot_active(clk, q)) return;
    const int idx = blockIdx.x * kScanBlock + (int)threadIdx.x;
    if (idx < n) start[idx] += tile_off[blockIdx.x];
    if (idx == 0) start[n] = tile_off[n_tiles];
}

// Millions of particles leave ~10^5 per-block maxima; one workgroup reading them all took 84 us at 6 M particles.
// This pre-pass folds kMaxTile of them per workgroup (max is exact, so the result does not depend on the split).
constexpr int kMaxTile = 4096;
__global__ __launch_bounds__(kScanBlock) void k_max_tiles(const Clock *clk, int q, int n, const double *a, const double *b,
                                                          double *out_a, double *out_b)
{
    if (!clk->run[q]) return;
    const int base = blockIdx.x * kMaxTile;
    double m = 0.0, d = 0.0;
    for (int k = base + threadIdx.x; k < min(base + kMaxTile, n); k += kScanBlock) {
        m = fmax(m, a[k]);
        if (b) d = fmax(d, b[k]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { m = fmax(m, __shfl_xor(m, off)); d = fmax(d, __shfl_xor(d, off)); }
    __shared__ double s_m[kScanBlock / 64], s_d[kScanBlock / 64];
    if ((threadIdx.x & 63) == 0) { s_m[threadIdx.x >> 6] = m; s_d[threadIdx.x >> 6] = d; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kScanBlock / 64; ++k) { m = fmax(m, s_m[k]); d = fmax(d, s_d[k]); }
        out_a[blockIdx.x] = m;
        if (b) out_b[blockIdx.x] = d;
    }
}

// Step kernel 5: finish the clock of this step (vmax -> next dt, t += dt, stop test) and scan the
// cell histogram (small grids) or the tile sums (big grids).  Single block.
//   vmax_global: slab mode -- the all-reduced max |v| replaces the local reduction.
//   dpart / rebuilt / half_skin: displacement bookkeeping of grids that are rebuilt only every few steps.
//   slab_counters: slab mode -- the keep/left/right counters of k_slab_pack, zeroed for the next step (the unpack
//   kernel of this step has read them).  vpart_reset: see continuity_tail.
__device__ __forceinline__ void clock_scan_body(Clock *clk, int q, const Phys &ph, int n_vpart,
                                                const double *vpart, const double *vmax_global,
                                                const int *flags, const int *count,
                                                int *start_next, int n_scan, const int *n_new,
                                                const double *dpart, int rebuilt, double half_skin,
                                                int *slab_counters, unsigned long long *vpart_reset, int dyn_K)
{
    // everything is requested before the run flag is looked at (stale values are harmless when the slot turns
    // out to be idle); only the thread that advances the clock loads it
    Clock c0;
    int fl = 0, nn = -1;
    double vg = 0.0;
    if (threadIdx.x == 0) {
        c0 = *clk;
        fl = *flags;
        if (n_new) nn = *n_new;
        if (vmax_global) vg = *vmax_global;
    }
    double m = 0.0, d = 0.0;
    if (!vmax_global)
        for (int k = threadIdx.x; k < n_vpart; k += kScanBlock) m = fmax(m, vpart[k]);
    if (dpart)
        for (int k = threadIdx.x; k < n_vpart; k += kScanBlock) d = fmax(d, dpart[k]);
    if (!clk->run[q]) {
        if (threadIdx.x == 0) clk->run[1 - q] = 0;
        return;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { m = fmax(m, __shfl_xor(m, off)); d = fmax(d, __shfl_xor(d, off)); }
    __shared__ double s_m[kScanBlock / 64], s_d[kScanBlock / 64];
    if ((threadIdx.x & 63) == 0) { s_m[threadIdx.x >> 6] = m; s_d[threadIdx.x >> 6] = d; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kScanBlock / 64; ++k) { m = fmax(m, s_m[k]); d = fmax(d, s_d[k]); }
        // max of sqrt == sqrt of max (monotone, correctly rounded)
        clock_step(clk, c0, q, ph, vmax_global ? vg : sqrt(m), fl, nn, dpart ? sqrt(d) : -1.0, rebuilt, half_skin, dyn_K);
        if (slab_counters) { slab_counters[0] = 0; slab_counters[1] = 0; slab_counters[2] = 0; }  // pack counters of the next step
    }
    // contexts whose move steps use the tail workgroup of pass E expect "empty" entries before every pass E
    if (vpart_reset)
        for (int k = threadIdx.x; k < n_vpart; k += kScanBlock) vpart_reset[k] = kVpartEmpty;
    if (count) scan_counts(count, start_next, n_scan);
}
__global__ __launch_bounds__(kScanBlock) void k_clock_scan(Clock *clk, int q, Phys ph, int n_vpart,
                                                           const double *vpart, const double *vmax_global,
                                                           const int *flags, const int *count,
                                                           int *start_next, int n_scan, const int *n_new,
                                                           const double *dpart, int rebuilt, double half_skin,
                                                           int *slab_counters, unsigned long long *vpart_reset, int dyn_K)
{
    clock_scan_body(clk, q, ph, n_vpart, vpart, vmax_global, flags, count, start_next, n_scan, n_new, dpart, rebuilt, half_skin,
                    slab_counters, vpart_reset, dyn_K);
}
// batch: one workgroup per member (static schedule: no slab inputs, no device-decided re-binning)
__global__ __launch_bounds__(kScanBlock) void k_clock_scan_b(Members mb, int q, const double *vpart, const int *flags,
                                                             const int *count, int *start_next, int n_scan,
                                                             const double *dpart, int rebuilt, double half_skin,
                                                             unsigned long long *vpart_reset)
{
    const int m = (int)blockIdx.y;
    const Phys ph = mb.ph[m];
    clock_scan_body(mb.clk + m, q, ph, mb.blocks, member_ptr(vpart, (long long)mb.blocks, m), nullptr, member_ptr(flags, 1ll, m),
                    member_ptr(count, (long long)mb.cells, m), member_ptr(start_next, (long long)mb.cells, m), n_scan, nullptr,
                    member_ptr(dpart, (long long)mb.blocks, m), rebuilt, half_skin, nullptr,
                    member_ptr(vpart_reset, (long long)mb.blocks, m), 0);
}

__global__ __launch_bounds__(kScanBlock) void k_scan_only(const Clock *clk, int q, const int *count, int *start, int n)
{
    if (clk && !slot_active(clk, q)) return;
    scan_counts(count, start, n);
}

// Step kernel 6: place every particle index into its cell range (arrival order, made canonical by
// k_reorder).  atomicSub counts the histogram back down to zero, ready for the next step.
__device__ __forceinline__ void scatter_body(const Clock *clk, int q, int n_fixed, const int *cellid, int *count,
                                             const int *start_next, int *perm)
{
    if (clk && !slot_active(clk, q)) return;
    const int n = clk ? clk->n : n_fixed;
    // Particles arrive nearly sorted (the previous cell order), so the 64 of a wavefront fall into a handful of cells:
    // one returning atomic per (wavefront, cell) instead of one per particle -- the lanes of a cell take consecutive slots
    // of the range their leader reserved.  (6 M returning atomics were 330 us; the order inside a cell is made canonical
    // by k_reorder anyway.)
    const int lane = threadIdx.x & 63;
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (int base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {  // (uniform trip count per workgroup)
        const int i = base + (int)threadIdx.x;
        const bool live = i < n;
        const int c = live ? cellid[i] : -1;
        unsigned long long todo = __ballot(live);
        while (todo) {
            const int lead = __ffsll((long long)todo) - 1;
            const int c_lead = __shfl(c, lead);
            const unsigned long long same = __ballot(live && c == c_lead) & todo;
            if (live && c == c_lead && (todo >> lane & 1ull)) {
                const int cnt = __popcll(same), rank = __popcll(same & below);
                int first = 0;
                if (rank == 0) first = atomicSub(&count[c], cnt);  // returns the count before: slots first-cnt .. first-1
                first = __shfl(first, __ffsll((long long)same) - 1);
                perm[start_next[c] + first - 1 - rank] = i;
            }
            todo &= ~same;
        }
    }
}
__global__ __launch_bounds__(kBlock) void k_scatter(const Clock *clk, int q, int n_fixed, const int *cellid,
                                                    int *count, const int *start_next, int *perm)
{
    scatter_body(clk, q, n_fixed, cellid, count, start_next, perm);
}
__global__ __launch_bounds__(kBlock) void k_scatter_b(Members mb, int q, const int *cellid, int *count, const int *start_next,
                                                      int *perm)
{
    const int m = (int)blockIdx.y;
    scatter_body(mb.clk + m, q, 0, member_ptr(cellid, mb.part, m), member_ptr(count, (long long)mb.cells, m),
                 member_ptr(start_next, (long long)mb.cells, m), member_ptr(perm, mb.part, m));
}

struct ReorderArgs {
    int n1, n2, n4;  // number of 8-, 16- and 32-byte fields
    const double *src1[2];
    double *dst1[2];
    const double2 *src2[3];
    double2 *dst2[3];
    const double4 *src4[1];
    double4 *dst4[1];
    const int *id_src;
    int *id_dst;
    int *src_of;
    int *cell_dst;  // binned cell of every destination slot (nullptr: not needed, walls)
    int *slot_of_id;  // skinned slabs: particle id -> its slot in the new ordering (nullptr: not needed)
};

// Step kernel 7: canonical rank inside the cell (ascending particle id -> an order that does not
// depend on arrival order, launch shape or domain decomposition) and the gather of every persistent
// field into the new ordering.
__device__ __forceinline__ void reorder_body(const Clock *clk, int q, int n_fixed, const int *cellid, const int *start_next,
                                             const int *perm, const ReorderArgs &a)
{
    if (clk && !slot_active(clk, q)) return;
    const int n = clk ? clk->n : n_fixed;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const int c = cellid[i];
        const int lo = start_next[c], hi = start_next[c + 1];
        const int my_id = a.id_src[i];
        int rank = 0;
        for (int k = lo; k < hi; ++k) {
            const int o = perm[k];
            const int oid = a.id_src[o];
            rank += (oid < my_id || (oid == my_id && o < i)) ? 1 : 0;  // tie (periodic images in a slab): by slot
        }
        const int dst = lo + rank;
#pragma unroll
        for (int f = 0; f < 3; ++f)
            if (f < a.n2) a.dst2[f][dst] = a.src2[f][i];
#pragma unroll
        for (int f = 0; f < 2; ++f)
            if (f < a.n1) a.dst1[f][dst] = a.src1[f][i];
        if (a.n4) a.dst4[0][dst] = a.src4[0][i];
        a.id_dst[dst] = my_id;
        if (a.src_of) a.src_of[dst] = i;
        if (a.cell_dst) a.cell_dst[dst] = c;
        if (a.slot_of_id) a.slot_of_id[my_id] = dst;
    }
}
__global__ __launch_bounds__(kBlock) void k_reorder(const Clock *clk, int q, int n_fixed, const int *cellid,
                                                    const int *start_next, const int *perm, ReorderArgs a)
{
    reorder_body(clk, q, n_fixed, cellid, start_next, perm, a);
}
// batch: every field of a ReorderArgs is a per-particle array (slot_of_id is not used)
__global__ __launch_bounds__(kBlock) void k_reorder_b(Members mb, int q, const int *cellid, const int *start_next,
                                                      const int *perm, ReorderArgs a)
{
    const int m = (int)blockIdx.y;
    const long long P = mb.part;
#pragma unroll
    for (int f = 0; f < 3; ++f) { a.src2[f] = member_ptr(a.src2[f], P, m); a.dst2[f] = member_ptr(a.dst2[f], P, m); }
#pragma unroll
    for (int f = 0; f < 2; ++f) { a.src1[f] = member_ptr(a.src1[f], P, m); a.dst1[f] = member_ptr(a.dst1[f], P, m); }
    a.src4[0] = member_ptr(a.src4[0], P, m); a.dst4[0] = member_ptr(a.dst4[0], P, m);
    a.id_src = member_ptr(a.id_src, P, m); a.id_dst = member_ptr(a.id_dst, P, m);
    a.src_of = member_ptr(a.src_of, P, m); a.cell_dst = member_ptr(a.cell_dst, P, m);
    a.slot_of_id = nullptr;
    reorder_body(mb.clk + m, q, 0, member_ptr(cellid, P, m), member_ptr(start_next, (long long)mb.cells, m),
                 member_ptr(perm, P, m), a);
}

// both step-slot flags off: whatever is enqueued next returns at once (sphx_ctx_prepare_steps warms graphs this way)
__global__ void k_disarm(Clock *clk)
{
    clk->run[0] = 0;
    clk->run[1] = 0;
}

// map[j] = via[map[j]]: a batch member re-binned again before its next step (realignment) keeps reaching the slots its last
// step's outputs are stored in
__global__ __launch_bounds__(kBlock) void k_compose(int n, const int *via, int *map)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j < n) map[j] = via[map[j]];
}

__global__ void k_rebinned(Clock *clk)
{
    clk->drift = 0.0;
    clk->need_rebuild = 0;
}

__global__ __launch_bounds__(kBlock) void k_iota(int n, int *a, int base)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) a[i] = base + i;
}

__global__ __launch_bounds__(kBlock) void k_wrap_x(int n, double2 *pos, double DL)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) pos[i].x = wrap_x(pos[i].x, DL);
}

__global__ void k_row_any(Grid g, const int *wstart, int *row_any)
{
    const int cy = blockIdx.x * blockDim.x + threadIdx.x;
    if (cy >= g.ncy) return;
    int any = 0;
    for (int r = max(cy - 1, 0); r <= min(cy + 1, g.ncy - 1) && !any; ++r)
        for (int cx = 0; cx < g.ncx; ++cx) {
            const int c = cx * g.ncy + r;
            if (wstart[c + 1] > wstart[c]) { any = 1; break; }
        }
    row_any[cy] = any;
}

// initial max |v| over owned particles (vecnorm over the fluid, SPH_Poiseuille.m:521); single block
__global__ __launch_bounds__(kScanBlock) void k_vmax_init(Clock *clk, Grid g, const double2 *pos, const double2 *vel,
                                                          double *vmax_out, const int *cell = nullptr)
{
    const int n = clk->n;
    double m = 0.0;
    for (int k = threadIdx.x; k < n; k += kScanBlock) {
        const double x = pos[k].x;
        if (!owns(g, x, (g.own_by_cell && cell) ? cell[k] : 0)) continue;
        const double2 v = vel[k];
        double v2 = v.x * v.x + v.y * v.y;
        if (v2 != v2) v2 = INFINITY;
        m = fmax(m, v2);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
    __shared__ double s_m[kScanBlock / 64];
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kScanBlock / 64; ++k) m = fmax(m, s_m[k]);
        clk->vmax = sqrt(m);
        if (vmax_out) *vmax_out = sqrt(m);
    }
}

// ---------------------------------------------------------------------------------------------
// monitors and pair-list emission on the current ordering
// ---------------------------------------------------------------------------------------------

// wall shear (sph_physics_mex.c:1713-1742): new neighbour structure, new pos/vel, Vol/B of the step
// that just finished (reached through src_of).  Per-block partial sums, reduced by k_tau_final.
__global__ __launch_bounds__(kBlock) void k_wall_shear(const Clock *clk, Grid g, Phys ph, FluidSet s, FluidTmp t,
                                                       Walls w, int use_src, double *part /*[2*grid]*/)
{
    const int n = clk->n;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    double fb = 0.0, ft = 0.0;
    if (i < n) {
        const double xi = s.pos[i].x, yi = s.pos[i].y;
        int cx, cy;
        binned_cell(g, s, i, cx, cy);
        if (w.row_any[cy] && xi >= g.own_lo && xi < g.own_hi) {
            const int o = use_src ? t.src_of[i] : i;
            const double Voli = t.a[o].x;
            const double4 Bo = t.B[o];
            const double b11 = Bo.x, b12 = Bo.y, b21 = Bo.z, b22 = Bo.w;
            const double vxi = s.vel[i].x;
            sweep<1>(g, w.start, cx, cy, 0, [&](int k) {
                const double2 pj = w.pos[k];
                const double dx = min_image(g, xi - pj.x), dy = yi - pj.y;
                const double r2 = dx * dx + dy * dy;
                if (r2 > kR2Min && r2 < ph.kc.rcut2) {
                    const double4 wj = w.a[k];
                    const double r = sqrt(r2);
                    const double ex = dx / r, ey = dy / r;
                    const double eBe = ex * (b11 * ex + b12 * ey) + ey * (b21 * ex + b22 * ey);
                    const double f = 4.0 * ph.mu * eBe * spline_dW(ph.kc, r) * wj.x * (vxi - wj.y) /
                                     (r + 0.01 * ph.kc.h) * Voli;
                    const double yj = pj.y;
                    if (yj <= 0.0) fb += f;
                    else if (yj >= ph.DH) ft += f;
                }
            });
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        fb += __shfl_xor(fb, off);
        ft += __shfl_xor(ft, off);
    }
    __shared__ double sb[kBlock / 64], st[kBlock / 64];
    if ((threadIdx.x & 63) == 0) { sb[threadIdx.x >> 6] = fb; st[threadIdx.x >> 6] = ft; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int k = 0; k < kBlock / 64; ++k) { a += sb[k]; b += st[k]; }
        part[2 * blockIdx.x] = a;
        part[2 * blockIdx.x + 1] = b;
    }
}

__global__ __launch_bounds__(kScanBlock) void k_tau_final(int nblk, const double *part, double DL, double *out)
{
    double a = 0.0, b = 0.0;
    for (int k = threadIdx.x; k < nblk; k += kScanBlock) { a += part[2 * k]; b += part[2 * k + 1]; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
    __shared__ double sa[kScanBlock / 64], sb[kScanBlock / 64];
    if ((threadIdx.x & 63) == 0) { sa[threadIdx.x >> 6] = a; sb[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = 0.0; b = 0.0;
        for (int k = 0; k < kScanBlock / 64; ++k) { a += sa[k]; b += sb[k]; }
        out[0] = -a / DL;  // the caller sums slabs; -sum/DL is linear
        out[1] = -b / DL;
    }
}

// Pair emission in the MEX convention (sph_neighbor_search_mex.c:353-383): a fluid-fluid pair is
// produced once, from the particle with the smaller ORIGINAL index; fluid-wall pairs always.
// MODE 0: count into cnt[orig]; MODE 1: write at off[orig].  (single-GPU contexts only)
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_pairs(const Clock *clk, Grid g, Phys ph, FluidSet s, Walls w, int *cnt,
                                                  const int *off, double *o_i, double *o_j, double *o_dx,
                                                  double *o_dy, double *o_r, double *o_W, double *o_dW)
{
    const int nf = clk->n;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nf) return;
    const double xi = s.pos[i].x, yi = s.pos[i].y;
    const int a = s.id[i];
    int cx, cy;
    binned_cell(g, s, i, cx, cy);
    int n = 0;
    const int base = MODE ? off[a] : 0;
    auto emit = [&](int b, double dx, double dy, double r2) {
        if (MODE) {
            const double r = sqrt(r2);
            double W, dW;
            spline(ph.kc, r, W, dW);
            const int p = base + n;
            o_i[p] = (double)(a + 1);
            o_j[p] = (double)(b + 1);
            o_dx[p] = dx; o_dy[p] = dy; o_r[p] = r; o_W[p] = W; o_dW[p] = dW;
        }
        ++n;
    };
    sweep<1>(g, s.start, cx, cy, 0, [&](int k) {
        const double2 pj = s.pos[k];
        const double dx = min_image(g, xi - pj.x), dy = yi - pj.y;
        const double r2 = dx * dx + dy * dy;
        if (r2 > kR2Min && r2 < ph.kc.rcut2) {
            const int b = s.id[k];
            if (b > a) emit(b, dx, dy, r2);
        }
    });
    if (w.row_any[cy]) {
        sweep<1>(g, w.start, cx, cy, 0, [&](int k) {
            const double2 pj = w.pos[k];
            const double dx = min_image(g, xi - pj.x), dy = yi - pj.y;
            const double r2 = dx * dx + dy * dy;
            if (r2 > kR2Min && r2 < ph.kc.rcut2) emit(w.id[k], dx, dy, r2);
        });
    }
    if (!MODE) cnt[a] = n;
}

// scatter one component of a sorted field (records of `stride` doubles) back to the caller's row numbering;
// src_of (optional): the field is stored in the ordering before the last re-binning, slot i was slot src_of[i] there
__global__ __launch_bounds__(kBlock) void k_unsort(int n, const int *id, const double *src, int stride, double *dst,
                                                   const int *src_of)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) dst[id[i]] = src[(size_t)(src_of ? src_of[i] : i) * stride];
}

// Dynamic contexts re-bin in place: k_reorder gathers into temporaries, this copies them back over the state of
// the next step and the layout arrays (only on steps that re-bin).
struct CopyBack {
    const double2 *pos_s, *vel_s, *posb_s;
    double2 *pos_d, *vel_d, *posb_d;
    const double *drho_s, *mass_s;
    double *drho_d, *mass_d;
    const int *id_s, *cell_s, *start_s;
    int *id_d, *cell_d, *start_d;
    int n_start;  // ncells + 1
    // 1: binning positions, cells and cell starts were written in place -- nobody reads the old ones during the re-ordering, so
    // k_scan_* and k_reorder can take the layout's own arrays as their destination -- and only what the re-ordering itself reads
    // while it writes (state, mass, id) went through temporaries: 52 bytes per particle to bring back instead of 72
    int lean;
};
__global__ __launch_bounds__(kBlock) void k_copyback(const Clock *clk, int qf, CopyBack a)
{
    if (!slot_active(clk, qf)) return;
    const int n = clk->n;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < (a.lean ? n : max(n, a.n_start)); i += gridDim.x * kBlock) {
        if (i < n) {
            a.pos_d[i] = a.pos_s[i];
            a.vel_d[i] = a.vel_s[i];
            a.drho_d[i] = a.drho_s[i];
            a.mass_d[i] = a.mass_s[i];
            a.id_d[i] = a.id_s[i];
            if (!a.lean) {
                a.posb_d[i] = a.posb_s[i];
                a.cell_d[i] = a.cell_s[i];
            }
        }
        if (!a.lean && i < a.n_start) a.start_d[i] = a.start_s[i];
    }
}

__global__ __launch_bounds__(kBlock) void k_fill(int n, double *dst, double v)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) dst[i] = v;
}

// ---------------------------------------------------------------------------------------------
// x-slab halo exchange (multi-GPU): pack the end-of-step state of OWNED particles into
//   keep  : still inside this rank's window [win_lo, win_hi) -> compacted for the next step (a particle
//           that crossed into a neighbour's columns stays here as a halo copy: its new owner did not
//           own it during this step and therefore does not send it back yet)
//   sendL : x_new < own_lo + halo_w  (shifted by shift_l: +DL on the first slab)
//   sendR : x_new >= own_hi - halo_w (shifted by shift_r: -DL on the last slab)
// A message is double[1 + 7*cap]: count, then x,y,vx,vy,drho,mass,id blocks of `cap`.
// Particles that were halo copies at the start of the step are dropped: their owner sends fresh ones.
// ---------------------------------------------------------------------------------------------
struct SlabPack {
    double *send_l, *send_r;   // device message buffers
    int *counters;             // [3]: keep, left, right (zeroed by k_slab_unpack of the previous step)
    double2 *kpos, *kvel;      // keep arrays (compacted)
    double *kdrho, *kmass;
    int *kid;
    int *cellid, *count;       // cell of every kept / received particle and the cell histogram (binned on the fly)
    double halo_w, shift_l, shift_r, win_lo, win_hi;
    int msg_cap, keep_cap;
};

__device__ __forceinline__ void msg_put(double *msg, int cap, int slot, double x, double y, double vx, double vy,
                                        double drho, double mass, int id)
{
    double *b = msg + 1;
    b[slot] = x;
    b[(size_t)cap + slot] = y;
    b[2 * (size_t)cap + slot] = vx;
    b[3 * (size_t)cap + slot] = vy;
    b[4 * (size_t)cap + slot] = drho;
    b[5 * (size_t)cap + slot] = mass;
    b[6 * (size_t)cap + slot] = (double)id;
}

__global__ __launch_bounds__(kBlock) void k_slab_pack(const Clock *clk, int q, Grid g, FluidSet s, FluidTmp t,
                                                      SlabPack p)
{
    if (!clk->run[q]) return;
    const int n = clk->n;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double x_ref = s.pos[i].x;
    if (!(x_ref >= g.own_lo && x_ref < g.own_hi)) return;  // halo copy
    const double2 pn = t.posn[i], vn = t.veln[i];
    const double xn = pn.x, yn = pn.y, vxn = vn.x, vyn = vn.y, dr = t.drhon[i], m = s.mass[i];
    const int id = s.id[i];
    if (xn >= p.win_lo && xn < p.win_hi) {
        const int k = atomicAdd(&p.counters[0], 1);
        if (k < p.keep_cap) {
            p.kpos[k] = pn; p.kvel[k] = vn; p.kdrho[k] = dr; p.kmass[k] = m; p.kid[k] = id;
            int cx, cy;
            cell_of(g, xn, yn, cx, cy);
            const int c = cx * g.ncy + cy;
            p.cellid[k] = c;
            atomicAdd(&p.count[c], 1);
        } else atomicOr(t.flags, 2);
    }
    if (xn < g.own_lo + p.halo_w) {
        const int k = atomicAdd(&p.counters[1], 1);
        if (k < p.msg_cap) msg_put(p.send_l, p.msg_cap, k, xn + p.shift_l, yn, vxn, vyn, dr, m, id);
        else atomicOr(t.flags, 2);
    }
    if (xn >= g.own_hi - p.halo_w) {
        const int k = atomicAdd(&p.counters[2], 1);
        if (k < p.msg_cap) msg_put(p.send_r, p.msg_cap, k, xn + p.shift_r, yn, vxn, vyn, dr, m, id);
        else atomicOr(t.flags, 2);
    }
}

// after the pack kernel, one workgroup: publish the message counts and reduce the per-block max |v|^2 of the
// owned particles to max |v| (input of the all-reduce)
__global__ __launch_bounds__(kScanBlock) void k_slab_seal_vmax(const Clock *clk, int q, SlabPack p, int n_vpart,
                                                               const double *vpart, double *vmax_out)
{
    const bool run = clk->run[q] != 0;
    if (threadIdx.x == 0) {
        p.send_l[0] = run ? (double)min(p.counters[1], p.msg_cap) : -1.0;
        p.send_r[0] = run ? (double)min(p.counters[2], p.msg_cap) : -1.0;
    }
    if (!run) { if (threadIdx.x == 0) *vmax_out = 0.0; return; }
    double m = 0.0;
    for (int k = threadIdx.x; k < n_vpart; k += kScanBlock) m = fmax(m, vpart[k]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
    __shared__ double s_m[kScanBlock / 64];
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kScanBlock / 64; ++k) m = fmax(m, s_m[k]);
        *vmax_out = sqrt(m);
    }
}

// append the received halo/migrant particles behind the kept ones; writes the new particle count.
__global__ __launch_bounds__(kBlock) void k_slab_unpack(const Clock *clk, int q, Grid g, SlabPack p, const double *recv_l,
                                                        const double *recv_r, int *n_new, int *flags)
{
    if (!clk->run[q]) return;
    const int nk = min(p.counters[0], p.keep_cap);
    const int nl = (int)recv_l[0], nr = (int)recv_r[0];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (nl < 0 || nr < 0 || nk + nl + nr > p.keep_cap) {
        if (i == 0) { atomicOr(flags, 2); *n_new = min(nk, p.keep_cap); }
        return;
    }
    if (i == 0) *n_new = nk + nl + nr;
    const int cap = p.msg_cap;
    if (i < nl + nr) {
        const double *b = (i < nl ? recv_l : recv_r) + 1;
        const int sl = i < nl ? i : i - nl;
        const int d = nk + i;
        const double x = b[sl], y = b[(size_t)cap + sl];
        p.kpos[d] = make_double2(x, y);
        int cx, cy;
        cell_of(g, x, y, cx, cy);
        const int c = cx * g.ncy + cy;
        p.cellid[d] = c;
        atomicAdd(&p.count[c], 1);
        p.kvel[d] = make_double2(b[2 * (size_t)cap + sl], b[3 * (size_t)cap + sl]);
        p.kdrho[d] = b[4 * (size_t)cap + sl];
        p.kmass[d] = b[5 * (size_t)cap + sl];
        p.kid[d] = (int)b[6 * (size_t)cap + sl];
    }
}

// ---------------------------------------------------------------------------------------------
// Skinned slabs: a slab re-bins (and re-negotiates its halo) only on the K-th step or when the drift bound is hit -- the
// device decides, from ALL-REDUCED max |v| and max drift, so every rank takes the same decision without the host.  In
// between the layout is frozen: each rank sends the new state of a fixed list of boundary particles (send_idx) and the
// receiver writes it into fixed slots (recv_slot); the lists are rebuilt with the layout.  Per step:
//   passes A..E (the local maxima come out of pass E's tail workgroup, slab_seal_tail) -> [max all-reduce of {max|v|, max drift}]
//   -> k_slab_pack3 (decision, message A, clock) -> [to both ring neighbours: message A, and message B = the ids of the send
//   lists made in the PREVIOUS step] -> k_slab_unpack3 (new ids -> slots; message A) -> {re-binning chain, k_slab_sendlist:
//   only when the clock says so}
// (round 3: ten launches of this sequence folded into three -- "last workgroup out" epilogues instead of one-thread kernels)
// Ownership goes by the binned column (Grid::own_by_cell).  A particle that crosses a slab boundary changes owner at
// the next re-binning: both ranks hold it (the old owner keeps everything in its window), the new owner names it in
// its id list and the old owner finds its copy through slot_of_id.
// ---------------------------------------------------------------------------------------------
struct SlabLists {
    int *send_idx[2];   // [msg_cap] slots whose state goes to the left / right neighbour every step
    int *send_cnt;      // [2]
    int *recv_slot[2];  // [msg_cap] slots the entries of the left / right neighbour's messages are written to
    int *recv_cnt;      // [2]
    int *slot_of_id;    // [global fluid count] particle id -> slot in the current layout (stale once a particle has left)
    int *ids_send[2];   // message B, outgoing: [1 + msg_cap] count, ids (device buffers owned by the context)
};

// "Last workgroup out": every workgroup of a kernel takes a ticket when its work is done; the one that draws the last
// ticket sees the complete result of all the others (counters are read with agent-scope atomics) and finishes the
// kernel's single-thread epilogue -- what used to be a one-thread kernel of its own behind it.  Returns true in every
// thread of that workgroup; the ticket counter is back at zero for the next kernel that uses it.  Atomics on one
// address are served at ~20 ns apiece: kernels that end this way run on a few hundred workgroups at most (grid-stride).
__device__ __forceinline__ bool last_workgroup_out(int *ticket, int n_workgroups)  // n_workgroups: how many draw a ticket
{
    // No agent-scope fence here: on this chip a release fence writes the XCD's whole L2 back, once per workgroup (measured:
    // a 0.76 M-particle slab step 380 -> 510 us).  What the epilogue reads of the other workgroups' work are counters
    // kept by RETURNING atomics (performed at the coherence point before their wave went on) and relaxed agent-scope
    // stores by the ticket-drawing thread itself, which the s_waitcnt below has seen acknowledged.
    __shared__ int s_last;
    __syncthreads();
    if (threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int drawn = atomicAdd(ticket, 1);
        s_last = drawn == n_workgroups - 1 ? 1 : 0;
        if (s_last) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    return s_last != 0;
}
__device__ __forceinline__ int peek(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// one slot of a shared counter per accepted lane, one atomic per wavefront (750 k single atomics on one address were
// 200 us of every re-binning step of a 0.76 M-particle slab)
__device__ __forceinline__ int wave_take_slot(int *counter, bool take)
{
    const unsigned long long m = __ballot(take);
    if (!m) return 0;
    const int lane = threadIdx.x & 63, lead = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == lead) base = atomicAdd(counter, __popcll(m));
    base = __shfl(base, lead);
    return base + __popcll(m & (lane ? (~0ull >> (64 - lane)) : 0ull));
}

// Global maxima known (vd_global = all-reduced {max |v|, max drift}): decide whether this step ends with a re-binning,
// write message A, advance the clock.  Every workgroup takes the decision by itself, from values the kernel's own epilogue
// never changes: the run flag of this parity, the all-reduced drift, and Clock::pos_q[q] -- the copy of pos_count that the
// PREVIOUS slot's clock update left for this one.  (On a frozen step only the first n_ticket workgroups draw a ticket, so
// the last of them may advance the clock while a workgroup beyond n_ticket has not even been dispatched yet -- slabs of an
// in-process ring share the chip; read from pos_count itself such a latecomer would see the NEW count, take the re-binning
// branch on the step before a scheduled re-binning and pollute counters, histogram and ticket.)
//   frozen step    : the new state of the send-list particles, in list order;
//   re-binning step: every owned particle's new state goes to `keep` (it stays in this window) and, near a boundary,
//                    to the neighbour -- as in k_slab_pack.
// sn = the NEW state (S[1-q]); layout arrays (mass, id, cell) are those of the step.
__global__ __launch_bounds__(kBlock) void k_slab_pack3(Clock *clk, int q, Grid g, Phys ph, FluidSet sn, SlabPack p, SlabLists L,
                                                       const double *vd_global, int *flags, double half_skin, int K, int *ticket)
{
    const bool run = clk->run[q] != 0;
    if (!run) {  // a stopped loop keeps the following slots idle and sends -1
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            clk->run[1 - q] = 0;
            p.send_l[0] = -1.0;
            p.send_r[0] = -1.0;
        }
        return;
    }
    const double drift = vd_global[1];
    const bool rb = !(drift <= half_skin) || clk->pos_q[q] >= K - 1;  // = clock_step's decision (dyn_K = K)
    const int stride = (int)gridDim.x * kBlock;
    int n_ticket = (int)gridDim.x;
    if (!rb) {
        n_ticket = min(n_ticket, (2 * p.msg_cap + kBlock - 1) / kBlock);
        if ((int)blockIdx.x >= n_ticket) return;  // nothing to do and nothing to wait for
        for (int e = blockIdx.x * kBlock + threadIdx.x; e < 2 * p.msg_cap; e += stride) {
            const int side = e < p.msg_cap ? 0 : 1, sl = e - side * p.msg_cap;
            if (sl >= L.send_cnt[side]) continue;
            const int k = L.send_idx[side][sl];
            const double2 pn = sn.pos[k], vn = sn.vel[k];
            msg_put(side ? p.send_r : p.send_l, p.msg_cap, sl, pn.x + (side ? p.shift_r : p.shift_l), pn.y, vn.x, vn.y,
                    sn.drho[k], 0.0, 0);
        }
    } else {
        // Every workgroup takes one contiguous chunk of the slots.  The kept particles of a chunk get consecutive places
        // in the keep arrays: count them, reserve the range with ONE atomic per workgroup, then hand the places out with a
        // block scan per sweep (a place per wavefront and sweep meant 12 k returning atomics on one address, ~13 ns each:
        // 150 us of every re-binning step of a 0.76 M-particle slab; the few boundary particles keep theirs).
        __shared__ int s_wave[kBlock / 64 + 1];
        __shared__ int s_base;
        const int n = clk->n;
        const int chunk = ((n + (int)gridDim.x - 1) / (int)gridDim.x + kBlock - 1) / kBlock * kBlock;
        const int lo = min(n, (int)blockIdx.x * chunk), hi = min(n, lo + chunk);
        auto kept = [&](int i) {
            if (i >= hi || !owns(g, 0.0, sn.cell[i])) return false;  // (halo copies: their owner sends fresh ones)
            const double x = sn.pos[i].x;
            return x >= p.win_lo && x < p.win_hi;
        };
        int mine_cnt = 0;
        for (int i = lo + (int)threadIdx.x; i < hi; i += kBlock) mine_cnt += kept(i) ? 1 : 0;
        int total;
        (void)block_exclusive_scan_t<kBlock>(mine_cnt, total, s_wave);
        if (threadIdx.x == 0) s_base = total > 0 ? atomicAdd(&p.counters[0], total) : 0;
        __syncthreads();
        int place = s_base;
        for (int base = lo; base < hi; base += kBlock) {  // (uniform trip count per workgroup)
            const int i = base + (int)threadIdx.x;
            const bool mine = i < hi && owns(g, 0.0, sn.cell[i]);
            double2 pn = make_double2(0.0, 0.0), vn = pn;
            double dr = 0.0, m = 0.0;
            int id = 0;
            if (mine) { pn = sn.pos[i]; vn = sn.vel[i]; dr = sn.drho[i]; m = sn.mass[i]; id = sn.id[i]; }
            const double xn = pn.x, yn = pn.y;
            const bool keep = mine && xn >= p.win_lo && xn < p.win_hi;
            const bool to_l = mine && xn < g.own_lo + p.halo_w, to_r = mine && xn >= g.own_hi - p.halo_w;
            int sweep_total;
            const int kk = place + block_exclusive_scan_t<kBlock>(keep ? 1 : 0, sweep_total, s_wave);
            place += sweep_total;
            const int kl = wave_take_slot(&p.counters[1], to_l);
            const int kr = wave_take_slot(&p.counters[2], to_r);
            if (keep) {
                if (kk < p.keep_cap) {
                    p.kpos[kk] = pn; p.kvel[kk] = vn; p.kdrho[kk] = dr; p.kmass[kk] = m; p.kid[kk] = id;
                    int cx, cy;
                    cell_of(g, xn, yn, cx, cy);
                    const int c = cx * g.ncy + cy;
                    p.cellid[kk] = c;
                    atomicAdd(&p.count[c], 1);
                } else atomicOr(flags, 2);
            }
            if (to_l) {
                if (kl < p.msg_cap) msg_put(p.send_l, p.msg_cap, kl, xn + p.shift_l, yn, vn.x, vn.y, dr, m, id);
                else atomicOr(flags, 2);
            }
            if (to_r) {
                if (kr < p.msg_cap) msg_put(p.send_r, p.msg_cap, kr, xn + p.shift_r, yn, vn.x, vn.y, dr, m, id);
                else atomicOr(flags, 2);
            }
        }
    }
    if (!last_workgroup_out(ticket, n_ticket) || threadIdx.x != 0) return;
    p.send_l[0] = (double)(rb ? min(peek(&p.counters[1]), p.msg_cap) : L.send_cnt[0]);
    p.send_r[0] = (double)(rb ? min(peek(&p.counters[2]), p.msg_cap) : L.send_cnt[1]);
    const Clock c0 = *clk;
    clock_step(clk, c0, q, ph, vd_global[0], peek(flags), -1, drift, 0, half_skin, K);
    if (clk->rebuild_now) clk->rebuild_now = 1;  // (no histogram is taken ahead of time in a slab)
}

// Message A arrived, and with it message B: the ids of the send lists the neighbours made in the PREVIOUS step (header
// -1: the lists of the cycle stay).  New ids are resolved to slots first (where do the particles the neighbours will
// keep sending live here?) -- not tied to the step slot being active: the slot after the loop's last step still
// delivers the ids that step made.  Then message A.  Frozen step: scatter the entries into their slots of the new
// state.  Re-binning step: append them behind the kept particles and bin them (k_slab_unpack); the last workgroup out
// then opens the new layout (particle count, counters back to zero).
__global__ __launch_bounds__(kBlock) void k_slab_unpack3(Clock *clk, int q, Grid g, FluidSet sn, SlabPack p, SlabLists L,
                                                         const double *recv_l, const double *recv_r, const int *ids_l,
                                                         const int *ids_r, int *n_new, int *flags, int *ticket)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int cap = p.msg_cap;
    const bool run = clk->run[q] != 0, rb = clk->rebuild_now != 0;
    const int n_now = clk->n;
    const int side = i < cap ? 0 : 1, sl = i - side * cap;
    int slot = -1, n_list = 0;
    if (i < 2 * cap) {
        const int *ids = side ? ids_r : ids_l;
        const int cnt = ids[0];
        if (cnt >= 0) {  // new lists
            n_list = min(cnt, cap);
            if (sl == 0) {
                if (cnt > cap) atomicOr(flags, 2);
                L.recv_cnt[side] = n_list;
            }
            if (sl < n_list) {
                const int id = ids[1 + sl];
                const int k = L.slot_of_id[id];
                if (k < 0 || k >= n_now || sn.id[k] != id) atomicOr(flags, 2);  // I do not hold that particle
                else { L.recv_slot[side][sl] = k; slot = k; }
            }
        } else {
            n_list = L.recv_cnt[side];
            if (sl < n_list) slot = L.recv_slot[side][sl];
        }
    }
    if (run && !rb) {
        if (i < 2 * cap) {
            const double *msg = side ? recv_r : recv_l;
            if (sl == 0 && (int)msg[0] != n_list) atomicOr(flags, 2);  // the neighbour disagrees with my lists
            if (slot >= 0) {
                const double *b = msg + 1;
                sn.pos[slot] = make_double2(b[sl], b[(size_t)cap + sl]);
                sn.vel[slot] = make_double2(b[2 * (size_t)cap + sl], b[3 * (size_t)cap + sl]);
                sn.drho[slot] = b[4 * (size_t)cap + sl];
            }
        }
    } else if (run) {
        const int nl = (int)recv_l[0], nr = (int)recv_r[0];
        const int nk = min(peek(&p.counters[0]), p.keep_cap);
        if (nl < 0 || nr < 0 || nk + nl + nr > p.keep_cap) {
            if (i == 0) { atomicOr(flags, 2); __hip_atomic_store(n_new, min(nk, p.keep_cap), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
        } else {
            if (i == 0) __hip_atomic_store(n_new, nk + nl + nr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (i < nl + nr) {
                const double *b = (i < nl ? recv_l : recv_r) + 1;
                const int s2 = i < nl ? i : i - nl;
                const int d = nk + i;
                const double x = b[s2], y = b[(size_t)cap + s2];
                p.kpos[d] = make_double2(x, y);
                int cx, cy;
                cell_of(g, x, y, cx, cy);
                const int c = cx * g.ncy + cy;
                p.cellid[d] = c;
                atomicAdd(&p.count[c], 1);
                p.kvel[d] = make_double2(b[2 * (size_t)cap + s2], b[3 * (size_t)cap + s2]);
                p.kdrho[d] = b[4 * (size_t)cap + s2];
                p.kmass[d] = b[5 * (size_t)cap + s2];
                p.kid[d] = (int)b[6 * (size_t)cap + s2];
            }
        }
    }
    if (!(run && rb)) return;  // (uniform over the grid: nobody takes a ticket)
    if (!last_workgroup_out(ticket, (int)gridDim.x) || threadIdx.x != 0) return;
    clk->n = peek(n_new);  // from here on the re-binning chain works on the new particle count
    p.counters[0] = 0; p.counters[1] = 0; p.counters[2] = 0;
    L.send_cnt[0] = 0; L.send_cnt[1] = 0;
}

// The local maxima a skinned slab feeds into the step's all-reduce -- max |v| of the kicked velocities and max drift of the
// owned particles -- as a kernel of its own on the slab's SECOND stream: both exist once pass CD is through, so the reduction
// and the all-reduce behind it run beside pass E instead of behind it (round 3: a tail workgroup of pass E, the all-reduce
// exposed on the step's only stream).  out[0..1] = {max |v|, max drift}; a stopped loop reports zeros.
constexpr int kSlabMaxBlocks = 256;
__global__ __launch_bounds__(kBlock) void k_slab_maxima(const Clock *clk, int q, Grid g, int n_vpart, const double *dpart,
                                                        const double2 *veln, const int *cell, double *part, double *out,
                                                        int *ticket)
{
    const bool run = clk->run[q] != 0;
    double m = 0.0, d = 0.0;
    if (run) {
        const int n = clk->n, stride = (int)gridDim.x * kBlock;
        // (four particles per trip, their loads requested together and unconditionally: the loop is a chain of memory round
        //  trips -- 23 of them per thread with one particle per trip cost 38 us at 0.76 M particles)
        for (int i0 = blockIdx.x * kBlock + threadIdx.x; i0 < n; i0 += 4 * stride) {
            int ce[4];
            double2 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = min(i0 + u * stride, n - 1);
                ce[u] = cell[i];
                v[u] = veln[i];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (i0 + u * stride >= n || !owns(g, 0.0, ce[u])) continue;  // (skinned slabs own by the binned column)
                double v2 = v[u].x * v[u].x + v[u].y * v[u].y;
                if (v2 != v2) v2 = INFINITY;  // NaN poisons the maximum on purpose
                m = fmax(m, v2);
            }
        }
        for (int k = blockIdx.x * kBlock + threadIdx.x; k < n_vpart; k += gridDim.x * kBlock) d = fmax(d, dpart[k]);
    }
    m = wave_max(m);
    d = wave_max(d);
    __shared__ double s_m[kBlock / 64], s_d[kBlock / 64];
    if ((threadIdx.x & 63) == 0) { s_m[threadIdx.x >> 6] = m; s_d[threadIdx.x >> 6] = d; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kBlock / 64; ++k) { m = fmax(m, s_m[k]); d = fmax(d, s_d[k]); }
        __hip_atomic_store(reinterpret_cast<unsigned long long *>(&part[2 * blockIdx.x]), (unsigned long long)__double_as_longlong(m),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(reinterpret_cast<unsigned long long *>(&part[2 * blockIdx.x + 1]), (unsigned long long)__double_as_longlong(d),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // the last workgroup out folds the partial maxima -- one per thread: a single thread reading them with agent-scope loads
    // one after the other took 80 us (the compiler does not overlap atomic loads)
    if (!last_workgroup_out(ticket, (int)gridDim.x)) return;
    m = 0.0; d = 0.0;
    for (int b = (int)threadIdx.x; b < (int)gridDim.x; b += kBlock) {
        m = fmax(m, __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<unsigned long long *>(&part[2 * b]),
                                                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
        d = fmax(d, __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<unsigned long long *>(&part[2 * b + 1]),
                                                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
    }
    m = wave_max(m);
    d = wave_max(d);
    __syncthreads();  // (s_m / s_d are reused)
    if ((threadIdx.x & 63) == 0) { s_m[threadIdx.x >> 6] = m; s_d[threadIdx.x >> 6] = d; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < kBlock / 64; ++k) { m = fmax(m, s_m[k]); d = fmax(d, s_d[k]); }
    out[0] = run ? sqrt(m) : 0.0;
    out[1] = run ? sqrt(d) : 0.0;
}

__global__ __launch_bounds__(kBlock) void k_slot_of_id(int n, const int *id, int *slot_of_id)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) slot_of_id[id[i]] = i;
}

// re-binning steps, on the NEW layout: owned particles within halo_w of a boundary form the send lists of the cycle;
// their ids are message B, whose header the last workgroup out writes (-1: the lists of the cycle stay)
__global__ __launch_bounds__(kBlock) void k_slab_sendlist(const Clock *clk, int q, Grid g, FluidSet sn, SlabPack p, SlabLists L,
                                                          int *flags, int force, int *ticket)
{
    const bool rb = force || (clk->run[q] && clk->rebuild_now);  // force: the lists of the first cycle
    if (!rb) {  // (uniform over the grid)
        if (blockIdx.x == 0 && threadIdx.x == 0) { L.ids_send[0][0] = -1; L.ids_send[1][0] = -1; }
        return;
    }
    const int n = clk->n;
    for (int base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {  // (uniform trip count per workgroup)
        const int i = base + (int)threadIdx.x;
        const bool mine = i < n && owns(g, 0.0, sn.cell[i]);
        const double x = mine ? sn.pos[i].x : 0.0;
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const bool near = mine && (side ? x >= g.own_hi - p.halo_w : x < g.own_lo + p.halo_w);
            const int k = wave_take_slot(&L.send_cnt[side], near);
            if (!near) continue;
            if (k < p.msg_cap) {
                L.send_idx[side][k] = i;
                L.ids_send[side][1 + k] = sn.id[i];
            } else atomicOr(flags, 2);
        }
    }
    if (!last_workgroup_out(ticket, (int)gridDim.x) || threadIdx.x != 0) return;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const int cnt = min(peek(&L.send_cnt[side]), p.msg_cap);
        L.send_cnt[side] = cnt;
        L.ids_send[side][0] = cnt;
    }
}

// message B, receiving side: where do the particles the neighbours will keep sending live here?  The ids travel with the
// NEXT step's message A (one exchange per step instead of two) and are looked at before that message is unpacked; a header
// of -1 says the lists of the cycle stay.  Not tied to the step slot being active: the slot after the loop's last step
// still delivers the ids that step made.
__global__ __launch_bounds__(kBlock) void k_slab_recvslots(const Clock *clk, int q, SlabPack p, SlabLists L, const int *ids_l,
                                                           const int *ids_r, const int *id_of_slot, int *flags, int force)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= 2 * p.msg_cap) return;
    const int side = i < p.msg_cap ? 0 : 1, sl = i - side * p.msg_cap;
    const int *ids = side ? ids_r : ids_l;
    const int cnt = ids[0];
    if (!force && cnt < 0) return;
    if (sl == 0) {
        if (cnt < 0 || cnt > p.msg_cap) atomicOr(flags, 2);  // (force: the first lists of a run must be there)
        L.recv_cnt[side] = max(0, min(cnt, p.msg_cap));
    }
    if (sl >= cnt || sl >= p.msg_cap) return;
    const int id = ids[1 + sl];
    const int k = L.slot_of_id[id];
    if (k < 0 || k >= clk->n || id_of_slot[k] != id) { atomicOr(flags, 2); return; }  // I do not hold that particle
    L.recv_slot[side][sl] = k;
}

}  // namespace sphx
