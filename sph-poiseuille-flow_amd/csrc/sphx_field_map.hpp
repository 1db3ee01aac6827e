// sphx_field_map.hpp -- velocity-field maps of a resident context (include/sphx.h section 2e), of every member of a
// batch (section 2g, k_field_map_b) and of a slab of a ring (section 3a, k_field_map_s): a slot sampler (sphx_slot_sample.hpp) that interpolates the velocity of the state the step left onto a regular nx x ny grid of nodes
// (both ends included in x and y, the shape of panel (b) of SPH_Poiseuille_postprocess.m:184-201 by default) and adds
// the sample to running sums per node.
//
// One sample at a node is Shepard interpolation with the cubic spline of spline_W over every particle within 2h
// (minimum image in x, no lower cut): S0 = sum W, S1 = sum W u_x, S2 = sum W u_y, and S1 / S0, S2 / S0 where S0 > 0.
//
// Why the 3 x 3 sweep suffices.  A node finds the cell its own coordinates fall into (cell_of) and walks the three cell
// columns around it (field_columns: the columns, rows and slot order of sweep<1>, through neighbour_column -- a period
// of one or two columns is visited once per distinct column and the minimum-image fold picks the nearest image,
// duplicate_column).  The sweep is centred on the NODE's cell, not on a cell something was binned into, while the
// particles of a cell range are those BINNED there, which may since have drifted.  A particle within 2h of the node was
// binned at most 2h + drift from it; the cells are 2h + skin wide in x and y, so as long as the drift stays below the
// whole skin that binning position lies in the node's cell or one next to it.  The clock stops (or re-bins) at a drift
// of skin / 2: every state a sample can see -- the one a step slot left, the one a stopped loop left for
// sphx_ctx_download -- is inside the bound with half the skin to spare.  Wall particles do not move at all.
//
// A slab of a ring (k_field_map_s) samples the node columns it owns, in its own open window, with the sweep centred on the
// node's cell column CLAMPED into the owned columns [own_c0, own_c1): it reads the columns own - 1 .. own + 1 only, where the
// halo copies carry the finished step's state.  The argument carries over.  An owned node lies in
// [own_lo, own_hi] up to the rounding of the host's block rule, so the clamp moves the centre by at most one column, and only
// for a node ON the outer edge of the owned range (x = DL of the last slab; a node column that falls on a cut).  A particle
// within 2h of such a node was binned within 2h + drift of the edge: in the outermost owned column or in the first halo
// column beside it, both among the clamped centre's three, because a column is 2h + skin wide and the ring re-bins at a
// drift of skin / 2 -- the spare half of the skin is many orders of magnitude more than the rounding.  The window is open
// (half_DL = +inf): the first slab holds the last slab's particles at x - DL and the last slab the first slab's at x + DL, so
// node 0 and node nx - 1 (x = DL, evaluated there) need no minimum image.
//
// Mapping: one thread per node, a wave covers an 8 x 8 tile of nodes (about 4 dp x 4 dp at the default shape, one and a
// half cells), so the lanes of a wave walk nearly the same candidate runs and their 16-byte loads of pos / vel hit the
// same cache lines; consecutive node indices along y would spread a wave over about twelve cells.  Wave tiles are
// numbered y fastest, like the cells and the nodes.  The grid grows with the node count (four wave tiles a workgroup).
//
// Determinism: every node is owned by one thread, which adds the candidates in the sweep's column and slot order and
// updates the six sums of its node with plain loads and stores: no atomics, no ticket.  Two identical runs give identical
// bits; another layout of the particles (re-binning phase, host chunking) changes the summation order only.  The head is
// written by thread 0 of workgroup 0 alone (of a batch: of workgroup 0 of the member's grid row).
#pragma once
#include "../../include/sphx.h"
#include "sphx_slot_sample.hpp"

namespace sphx {

constexpr int kFieldPlanes = 6;             // count, sum_w, sum_ux, sum_uy, sum_ux2, sum_uy2: planes of nx * ny doubles
constexpr int kFieldTile = 8;               // a wave's tile of nodes: kFieldTile x kFieldTile = 64 lanes
constexpr int kFieldBlock = 256;            // four wave tiles per workgroup
constexpr long long kFieldMaxNodes = 1ll << 25;  // 6 planes: 1.5 GB

struct FieldMapHead {
    long long n_samples;
    double t_first, t_last;
};

struct FieldMapArgs {
    double *planes;        // [kFieldPlanes][nx * ny], node (i, k) at i * ny + k (of a batch: member 0's, member m's block behind)
    FieldMapHead *head;    // (of a batch: [M])
    double step_x, step_y; // DL / (nx - 1), DH / (ny - 1): the step of numpy's linspace
    double dp2;            // dp^2: sum_w accumulates S0 dp^2
    double t_from;
    int nx, ny;
    int tiles_y, n_tiles;  // wave tiles along y, and in all
    int every;             // >= 1: in-loop sample, gated on the clock; 0: sample unconditionally
    int with_walls;        // 1: the wall particles enter the sums with their wall velocity
};

struct FieldSums {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;  // sum W, sum W u_x, sum W u_y
};

// The candidates of the three cell columns around (cx, cy) -- sweep<1>'s columns, rows and slot order -- added to S for the node
// at (xn, yn).  kFieldAhead candidates a trip: their positions AND velocities are requested before the first one is looked at
// (a slot beyond the run repeats the run's last one and is not added), so a trip costs one memory round trip where one
// candidate a trip cost one per candidate and a second, dependent one per hit -- at a few thousand particles a wave is alone
// on its SIMD and the sample is that chain of round trips.  The order of the adds is the slot order either way.
constexpr int kFieldAhead = 4;
template <typename Vel>
__device__ __forceinline__ void field_columns(const Grid &g, const KernelConst &kc, const int *__restrict__ start, int cx, int cy,
                                              double xn, double yn, FieldSums &S, const double2 *__restrict__ pos, Vel &&vel)
{
    const int cylo = max(cy - 1, 0), cyhi = min(cy + 1, g.ncy - 1);
#pragma unroll 1
    for (int ox = -1; ox <= 1; ++ox) {
        int col;
        if (!neighbour_column(g, cx, ox, col)) continue;
        const int base = col * g.ncy;
        const int lo = start[base + cylo], hi = start[base + cyhi + 1];
        for (int k = lo; k < hi; k += kFieldAhead) {
            double2 p[kFieldAhead], v[kFieldAhead];
#pragma unroll
            for (int u = 0; u < kFieldAhead; ++u) {
                const int j = min(k + u, hi - 1);
                p[u] = pos[j];
                v[u] = vel(j);
            }
#pragma unroll
            for (int u = 0; u < kFieldAhead; ++u) {
                const double dx = min_image(g, xn - p[u].x), dy = yn - p[u].y;
                const double r2 = dx * dx + dy * dy;
                if (k + u < hi && r2 < kc.rcut2) {
                    const double W = spline_W(kc, sqrt(r2));
                    S.s0 += W;
                    S.s1 += W * v[u].x;
                    S.s2 += W * v[u].y;
                }
            }
        }
    }
}

// The sample of one channel closing the step slot of parity q, on clock clk, by the gridDim.x workgroups of a grid row; s is the
// state the step left (pos, vel and the cell ranges of the layout it is stored in); a's planes and head are that channel's own.
// kSlab: the channel is a slab of a ring -- a.nx, the tiles and the planes are those of the BLOCK of node columns the slab
// owns, column i of the block is column i_lo + i of the ring's nx_all columns (a.step_x is the ring's), and the sweep is
// centred on a column the slab owns.  A block may be empty (a.nx = 0, no tiles): the head still counts the sample.
template <bool kSlab = false>
__device__ __forceinline__ void field_map_body(const Clock *clk, int q, const Grid &g, const Phys &ph, const FluidSet &s,
                                               const Walls &w, const FieldMapArgs &a, int i_lo = 0, int nx_all = 0)
{
    if (!sample_due(clk, q, a.every, a.t_from)) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) note_sample(a.head, clk->t);  // the head, by one thread: plain vector stores
    const int lane = (int)threadIdx.x & 63;
    const int tile = (int)blockIdx.x * (kFieldBlock / 64) + ((int)threadIdx.x >> 6);
    if (tile >= a.n_tiles) return;
    const int tx = tile / a.tiles_y, ty = tile - tx * a.tiles_y;
    const int i = tx * kFieldTile + (lane >> 3), k = ty * kFieldTile + (lane & 7);
    if (i >= a.nx || k >= a.ny) return;
    // numpy's linspace: i * step, the last node the end itself
    double xn;
    if constexpr (kSlab) xn = i_lo + i == nx_all - 1 ? ph.DL : (double)(i_lo + i) * a.step_x;
    else xn = i == a.nx - 1 ? ph.DL : (double)i * a.step_x;
    const double yn = k == a.ny - 1 ? ph.DH : (double)k * a.step_y;
    int cx, cy;
    cell_of(g, xn, yn, cx, cy);
    if constexpr (kSlab) cx = min(max(cx, g.own_c0), g.own_c1 - 1);
    FieldSums S;
    field_columns(g, ph.kc, s.start, cx, cy, xn, yn, S, s.pos, [&](int j) { return s.vel[j]; });
    if (a.with_walls && w.row_any[cy])
        field_columns(g, ph.kc, w.start, cx, cy, xn, yn, S, w.pos, [&](int j) {
            const double4 wj = w.a[j];  // {Vol, vx, vy, 0}
            return make_double2(wj.y, wj.z);
        });
    const double S0 = S.s0, S1 = S.s1, S2 = S.s2;
    if (!(S0 > 0.0)) return;  // no contributor: the node is skipped for this sample
    const size_t nn = (size_t)a.nx * (size_t)a.ny, at = (size_t)i * (size_t)a.ny + (size_t)k;
    const double ux = S1 / S0, uy = S2 / S0;
    double *p = a.planes + at;
    p[0] += 1.0;
    p[nn] += S0 * a.dp2;
    p[2 * nn] += ux;
    p[3 * nn] += uy;
    p[4 * nn] += ux * ux;
    p[5 * nn] += uy * uy;
}

// q: parity of the step slot this launch closes
__global__ __launch_bounds__(kFieldBlock) void k_field_map(const Clock *clk, int q, Grid g, Phys ph, FluidSet s, Walls w,
                                                           FieldMapArgs a)
{
    field_map_body(clk, q, g, ph, s, w, a);
}

// batch (sphx_batch_field_map_*): member m = blockIdx.y samples its own state (member_set of the view, which is member 0's) on
// its own clock and parameters into its own six planes (m * kFieldPlanes * nx * ny) and its own head; Grid and Walls are
// shared.  gridDim.x is the workgroup count of a context's map of this shape, every node is owned by the same thread of the
// same workgroup of the row and adds its candidates in the same order: a member's planes are bit for bit a standalone
// context's.  A member whose gate is closed returns before it touches its head or its planes.
__global__ __launch_bounds__(kFieldBlock) void k_field_map_b(Members mb, int q, Grid g, FluidSet s, Walls w, FieldMapArgs a)
{
    const int m = (int)blockIdx.y;
    const Phys ph = mb.ph[m];
    a.planes += (size_t)m * kFieldPlanes * (size_t)a.nx * (size_t)a.ny;
    a.head += m;
    field_map_body(mb.clk + m, q, g, ph, member_set(mb, m, s), w, a);
}

// slab of a ring (sphx_slab_field_map_*): the complete sample of every node of the block of node columns this slab owns
// (i_lo <= column < i_lo + a.nx of the ring's nx_all; the host fixed the blocks at enable, sphx_samplers.hpp), from the
// particles it owns and from its halo copies.  Launched behind k_slab_pack3 and in front of everything of phase 3
// (launch_slab_samplers): s is S[1-q] with the cell ranges of the layout the step ran in.  Every node is owned by one thread of
// one slab, which adds its candidates in the sweep's column and slot order: no atomics, no ticket.
__global__ __launch_bounds__(kFieldBlock) void k_field_map_s(const Clock *clk, int q, Grid g, Phys ph, FluidSet s, Walls w,
                                                             FieldMapArgs a, int i_lo, int nx_all)
{
    field_map_body<true>(clk, q, g, ph, s, w, a, i_lo, nx_all);
}

}  // namespace sphx
