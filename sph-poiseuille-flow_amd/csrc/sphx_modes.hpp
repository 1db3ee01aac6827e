// sphx_modes.hpp -- the mode amplitudes of a resident context (include/sphx.h section 2t) and of every member of a batch
// (section 2u, k_modes_b): a slot sampler (sphx_slot_sample.hpp) that projects the state the step left on the channel's own
// basis -- periodic in x, walls in y -- and appends the projection as one record, as the profile series does
// (sphx_profile_series.hpp).  For fluid particle i, thx = 2 pi x_i / DL and thy = pi y_i / DH; for every mode 0 <= m <= mx,
// 0 <= n <= ny the four bases cc, sc, cs, ss = {cos, sin}(m thx) * {cos, sin}(n thy) and the three fields q = 1, u_x, u_y:
//   S[m][n][f][k] = sum_i q_i * basis_k(i),  counter ((m (ny + 1) + n) * kModeFields + f) * kModeBases + k.
// Unweighted sums over the fluid particles, walls never in.
//
// The reduction.  Every other sampler is a histogram: a particle lands in a few bins and LDS atomics serve.  Here every
// particle adds to EVERY counter, so an atomic per particle and counter would serialise the whole sample on nc addresses.
// Instead the modes are cut into GROUPS of kModesRun consecutive n of one m (kModesRun * 12 counters, contiguous), and the
// grid's x-dimension is chunks x groups: workgroup blockIdx.x serves group blockIdx.x % n_groups over the particles of chunk
// blockIdx.x / n_groups.  A lane takes the particles i0 + lane, i0 + lane + kModesBlock, ... of the chunk and keeps the
// kModesRun * 12 int64 sums of its group in registers across all of them (every loop over them is unrolled: no indexed
// register array, no scratch).  Behind the loop a wave folds each sum over its 64 lanes with integer adds -- four DPP stages
// inside the rows of 16, two __shfl_xor stages across them, both on the two 32-bit halves -- once; lane 0 adds the wave's
// totals to the workgroup's LDS counters (one LDS add per wave and counter), and the workgroup adds every non-zero counter
// to the global int64 sums with one atomic.  No atomic per particle anywhere.
//
// Exact sums.  Each term q * basis is rounded ONCE, to int64 fixed point, and integers add exactly in any order: with
// n <= 2^L particles the field `n` (|basis| <= 1) has scale 62 - L, u_x and u_y the s1 = 62 - L - e of stats_scales
// (2 vmax < 2^e).  q is scaled first -- by a power of two, exactly -- so a term is one product chain and one
// __double2ll_rn.  A |u| above the bound (a non-finite state) raises the sticky range flag and the read fails.
//
// Trigonometry.  One sincospi per axis and particle -- of 2 x / DL and y / DH: the reduction of sincospi is exact, so a
// particle on the seam or on a wall gets an exact 0 or +-1 -- and the multiples by the rotation c' = c c1 - s s1,
// s' = s c1 + c s1 from exactly (1, 0): m = 0 and n = 0 are exact, so S[0][0][n][cc] = N and every sine sum of a zero mode
// is 0, to the bit.  The products are not contracted (fp contract off): a term is the same bits wherever the compiler
// places it.
//
// Determinism.  A particle's term depends on that particle alone -- its position, its velocity, the sample's scales -- not
// on its slot, its neighbours, the lane or workgroup that meets it.  Integer adds in any order give the same integers and
// each counter is converted once by one thread: the records are bit-identical whatever the particle order, layout, lane
// count, re-binning phase or workgroup count, and a member of a batch records bit for bit what a standalone context does.
//
// The record: profile_series_body's.  The finishing workgroup -- the only one, or the last one out (last_out_fenced) -- reads
// slot = head->n_records and, when slot < capacity, stores EVERY counter, zeros included, into records[slot * nc + k]; the
// buffer is never cleared.  Thread 0 stamps {step, t} and counts the record, or a dropped one; either way the global sums
// are back at zero (atomicExch) and the ticket is cleared.
#pragma once
#include "sphx_profile_series.hpp"

namespace sphx {

constexpr int kModeFields = 3;        // n (q = 1), ux, uy
constexpr int kModeBases = 4;         // cc, sc, cs, ss
constexpr int kModeSums = kModeFields * kModeBases;  // per mode
constexpr int kModesMax = 16;         // mx, ny <= 16: 289 modes, 3 468 counters, 27 744 B of LDS counters per workgroup
constexpr int kModesRun = 3;          // consecutive n of one m a lane serves: 36 int64 sums = 72 VGPRs
constexpr int kModesBlock = 256;
constexpr int kModesPerThread = 8;    // particles a thread takes before another chunk is added
constexpr int kModesMaxBlocks = 1024; // workgroups of a sample (per member), chunks x groups; at least one chunk

struct ModesHead {
    long long n_records, n_dropped;
    int range;   // sticky: some |u| of some sample exceeded the bound of that sample
    int ticket;  // last workgroup out (zero between launches)
};

struct ModesArgs {
    const double2 *pos, *vel;   // the state to sample (fluid slots 0 .. clk->n-1, any order; of a batch: member 0's)
    unsigned long long *isum;   // [mx+1][ny+1][kModeFields][kModeBases] integer sums of the sample in flight (zero in between)
    double *times;              // [capacity][2]: step, t (of a batch: member 0's, member m's block behind)
    double *records;            // [capacity][mx+1][ny+1][kModeFields][kModeBases]
    ModesHead *head;            // (of a batch: [M])
    double DL, DH;
    double t_from;
    int mx, ny;
    int n_groups;               // (mx + 1) * ceil((ny + 1) / kModesRun): gridDim.x = chunks * n_groups
    int every;                  // >= 1: in-loop sample, gated on the clock; 0: sample unconditionally
    int capacity;
};

// groups of a sample with modes 0 .. mx, 0 .. ny (host and device)
__host__ __device__ constexpr int modes_runs(int ny) { return (ny + kModesRun) / kModesRun; }

// (c, s) turned on by the angle of (c1, s1); from exactly (1, 0) the first turn gives (c1, s1) itself
__device__ __forceinline__ void modes_turn(double &c, double &s, double c1, double s1)
{
#pragma clang fp contract(off)
    const double cn = c * c1 - s * s1;
    const double sn = s * c1 + c * s1;
    c = cn;
    s = sn;
}

// one term, rounded once: q (already scaled by its power of two) times the basis value
__device__ __forceinline__ long long modes_term(double q, double bx, double by)
{
#pragma clang fp contract(off)
    const double b = bx * by;
    return __double2ll_rn(q * b);
}

template <int CTRL>
__device__ __forceinline__ long long dpp_i64(long long v)
{
    const int lo = __builtin_amdgcn_mov_dpp((int)(unsigned long long)v, CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp((int)((unsigned long long)v >> 32), CTRL, 0xF, 0xF, true);
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
}

// sum of an int64 over the wave, in every lane: the stages of wave_max (sphx_kernels.hpp) with integer adds
__device__ __forceinline__ long long wave_sum_i64(long long v)
{
    v += dpp_i64<0xB1>(v);    // quad_perm [1 0 3 2]
    v += dpp_i64<0x4E>(v);    // quad_perm [2 3 0 1]
    v += dpp_i64<0x141>(v);   // row_half_mirror
    v += dpp_i64<0x140>(v);   // row_mirror
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

// counter k of a sample as the double it stands for: field (k / kModeBases) % kModeFields, its scale taken back out
__device__ __forceinline__ double modes_value(int k, unsigned long long v, int s0, int s1)
{
    const int f = (k / kModeBases) % kModeFields;
    return ldexp((double)(long long)v, -(f == 0 ? s0 : s1));
}

// The record of one channel closing the step slot of parity q, on clock clk, shared by the gridDim.x workgroups of a grid row;
// pos / vel / isum / times / records / h are that channel's own.
__device__ __forceinline__ void modes_body(const Clock *clk, int q, const ModesArgs &a, const double2 *pos, const double2 *vel,
                                           unsigned long long *isum, double *times, double *records, ModesHead *h)
{
    if (!sample_due(clk, q, a.every, a.t_from)) return;
    const int n = clk->n;
    const double vmax = clk->vmax, t_now = clk->t, step_now = (double)clk->step;
    extern __shared__ unsigned long long s_cnt[];  // [mx+1][ny+1][kModeFields][kModeBases]
    __shared__ int s_last;
    const int nc = (a.mx + 1) * (a.ny + 1) * kModeSums;
    for (int k = threadIdx.x; k < nc; k += kModesBlock) s_cnt[k] = 0ull;
    __syncthreads();

    int s1, s2;
    double bound;
    stats_scales(vmax, n, s1, s2, bound);
    const int s0 = s1 + ilogb(bound);  // 62 - L: the scale of the field n, |basis| <= 1
    const double q0 = ldexp(1.0, s0);

    // this workgroup's group -- mode m, n0 <= n < n0 + kModesRun -- and its chunk of the particles
    const int g = (int)blockIdx.x % a.n_groups, chunk_id = (int)blockIdx.x / a.n_groups, chunks = (int)gridDim.x / a.n_groups;
    const int runs = modes_runs(a.ny);
    const int m = g / runs, n0 = (g % runs) * kModesRun;
    const int chunk = (n + chunks - 1) / chunks;
    const int i0 = chunk_id * chunk;
    const int i1 = min(n, i0 + chunk);

    long long acc[kModesRun][kModeSums];
#pragma unroll
    for (int j = 0; j < kModesRun; ++j)
#pragma unroll
        for (int k = 0; k < kModeSums; ++k) acc[j][k] = 0;
    bool out_of_range = false;
    for (int i = i0 + (int)threadIdx.x; i < i1; i += kModesBlock) {
        const double2 p = pos[i], v = vel[i];
        if (!(fabs(v.x) <= bound && fabs(v.y) <= bound)) { out_of_range = true; continue; }
        double cx1, sx1, cy1, sy1;
        sincospi(2.0 * p.x / a.DL, &sx1, &cx1);
        sincospi(p.y / a.DH, &sy1, &cy1);
        double cx = 1.0, sx = 0.0, cy = 1.0, sy = 0.0;
        for (int t = 0; t < m; ++t) modes_turn(cx, sx, cx1, sx1);
        for (int t = 0; t < n0; ++t) modes_turn(cy, sy, cy1, sy1);
        const double qs[kModeFields] = {q0, ldexp(v.x, s1), ldexp(v.y, s1)};
#pragma unroll
        for (int j = 0; j < kModesRun; ++j) {
#pragma unroll
            for (int f = 0; f < kModeFields; ++f) {
                acc[j][f * kModeBases + 0] += modes_term(qs[f], cx, cy);
                acc[j][f * kModeBases + 1] += modes_term(qs[f], sx, cy);
                acc[j][f * kModeBases + 2] += modes_term(qs[f], cx, sy);
                acc[j][f * kModeBases + 3] += modes_term(qs[f], sx, sy);
            }
            modes_turn(cy, sy, cy1, sy1);
        }
    }
    if (out_of_range) atomicOr(&h->range, 1);

    // fold over the wave, once; lane 0 adds the wave's totals to the workgroup's counters (a run past ny: nothing to add)
#pragma unroll
    for (int j = 0; j < kModesRun; ++j) {
        if (n0 + j > a.ny) break;
        unsigned long long *dst = s_cnt + (size_t)(m * (a.ny + 1) + n0 + j) * kModeSums;
#pragma unroll
        for (int k = 0; k < kModeSums; ++k) {
            const long long tot = wave_sum_i64(acc[j][k]);
            if ((threadIdx.x & 63) == 0 && tot != 0) atomicAdd(dst + k, (unsigned long long)tot);
        }
    }
    __syncthreads();

    const bool alone = gridDim.x == 1;  // one group, one chunk: one workgroup holds the whole sample -- no global sums, no ticket
    if (!alone) {
        for (int k = threadIdx.x; k < nc; k += kModesBlock) {
            const unsigned long long v = s_cnt[k];
            if (v) atomicAdd(isum + k, v);
        }
        last_out_fenced(&h->ticket, s_last);
        if (!s_last) return;
    }
    // the finishing workgroup: the only writer of this sample
    const long long slot = h->n_records;
    const bool keep = slot < (long long)a.capacity;
    double *rec = records + (size_t)slot * (size_t)nc;  // (not dereferenced unless keep)
    for (int k = threadIdx.x; k < nc; k += kModesBlock) {
        const unsigned long long v = alone ? s_cnt[k] : atomicExch(isum + k, 0ull);
        if (keep) rec[k] = modes_value(k, v, s0, s1);  // every counter, zeros included: the buffer is never cleared
    }
    __syncthreads();  // every thread has read n_records
    if (threadIdx.x != 0) return;
    if (keep) {
        *reinterpret_cast<double2 *>(times + (size_t)slot * 2) = make_double2(step_now, t_now);
        h->n_records = slot + 1;
    } else {
        h->n_dropped += 1;
    }
    if (!alone) __hip_atomic_store(&h->ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// q: parity of the step slot this launch closes
__global__ __launch_bounds__(kModesBlock) void k_modes(const Clock *clk, int q, ModesArgs a)
{
    modes_body(clk, q, a, a.pos, a.vel, a.isum, a.times, a.records, a.head);
}

// batch (sphx_batch_modes_*): member m = blockIdx.y records its own state (pos / vel at m * Members::part) on its own clock
// into its own block of records (m * capacity rows), its own int64 sums (m * nc), its own head and ticket; gridDim.x
// workgroups per member.  The sums are exact, so a member's records are bit for bit a standalone context's.  A member whose
// gate is closed returns before it touches its head or its records.
__global__ __launch_bounds__(kModesBlock) void k_modes_b(Members mb, int q, ModesArgs a)
{
    const int m = (int)blockIdx.y;
    const size_t nc = (size_t)(a.mx + 1) * (size_t)(a.ny + 1) * kModeSums;
    modes_body(mb.clk + m, q, a, a.pos + mb.part * m, a.vel + mb.part * m, a.isum + (size_t)m * nc,
               a.times + (size_t)m * (size_t)a.capacity * 2, a.records + (size_t)m * (size_t)a.capacity * nc, a.head + m);
}

}  // namespace sphx
