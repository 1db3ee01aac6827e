// Probe (manual tool, not part of the library): where are the workgroups of a step's three dependent launches placed, and
// does a line that an XCD stored in one launch still hit that XCD's L2 in the next one?
//   hipcc -O3 --offload-arch=gfx950 tools/probes/probe_xcd_affinity.hip -o tools/probes/probe_xcd_affinity
//   tools/probes/probe_xcd_affinity [replays=50]
// A graph of STEPS x 3 dependent kernels with the compact step's grid shapes (nb, nb, 2nb+1 workgroups of 256 threads) is
// replayed; nb = 300 (the headline, nb % 8 = 4) and nb = 304 (a multiple of eight).
//  (a) Placement: every workgroup records HW_REG_XCC_ID.  Per launch position the host counts the launches in which
//      xcc(b) == (xcc(0) + b) % 8 holds for every b, lists the values xcc(0) took, and counts how often xcc(0) continues from
//      where the grid before it ended ((xcc(0) of the previous launch + its workgroup count) % 8).
//  (b) Retention: launch 1 plain-stores the 4 KB chunks b and nb + b of a 2.4 MB buffer from workgroup b.  In launch 2, lane 0
//      of workgroup b times one 16-byte load from chunk b ("same": stored by a workgroup of the same residue mod 8) or from
//      chunk b + 4 ("far").  Launch 3 does the same two boundaries later, its workgroup b reading what workgroup b % nb
//      stored: for nb = 300 the upper half [nb, 2nb) then reads what residue (b + 4) % 8 stored, which is how the fused
//      launch numbered its pass-A half before xcd_block took the physical residue.
// No spin loops, no flags: the only ordering is the kernel boundary.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1);} } while (0)

constexpr int STEPS = 8;            // steps per graph: 24 launches back to back
constexpr int CHUNK = 4096;         // bytes a workgroup stores
constexpr int MAXNB = 304;
typedef unsigned int u4 __attribute__((ext_vector_type(4)));

struct Slot { int xcc; unsigned cyc, ref; int pad; };  // one per workgroup per launch

// HW_REG_XCC_ID is hardware register 20; bits 3:0 hold the XCD number: s_getreg_b32 hwreg(20, 0, 4)
__device__ __forceinline__ int xcc_id() { return (int)__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)); }

__global__ __launch_bounds__(256) void k_store(char *buf, Slot *out, unsigned tag)
{
    const int b = (int)blockIdx.x;
    u4 v = {tag, (unsigned)b, threadIdx.x, 0u};
    *reinterpret_cast<u4 *>(buf + (size_t)b * CHUNK + threadIdx.x * 16) = v;
    *reinterpret_cast<u4 *>(buf + (size_t)(b + (int)gridDim.x) * CHUNK + threadIdx.x * 16) = v;  // 2 nb chunks: 2.4 MB
    if (threadIdx.x == 0) out[b] = Slot{xcc_id(), 0u, 0u, 0};
}

// workgroup b reads the chunk that workgroup (b % nb + off) % nb stored, the upper half of a 2nb+1 grid the second copy
__global__ __launch_bounds__(256) void k_time(const char *buf, Slot *out, int nb, int off, unsigned *sink)
{
    const int b = (int)blockIdx.x;
    if (threadIdx.x != 0) return;
    const char *p = buf + (size_t)((b >= nb && b < 2 * nb ? nb : 0) + (b % nb + off) % nb) * CHUNK;
    uint64_t t0, t1;
    u4 v;
    const uint64_t r0 = wall_clock64();
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)\n\tglobal_load_dwordx4 %2, %3, off\n\ts_waitcnt vmcnt(0)\n\t"
                 "s_memtime %1\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(t0), "=&s"(t1), "=&v"(v)
                 : "v"(p)
                 : "memory");
    const uint64_t r1 = wall_clock64();
    out[b] = Slot{xcc_id(), (unsigned)(t1 - t0), (unsigned)(r1 - r0), 0};
    if (v.x == 0xffffffffu) *sink = v.y;  // keeps the load; tags never take this value
}

static double median(std::vector<unsigned> &v)
{
    if (v.empty()) return 0.0;
    std::sort(v.begin(), v.end());
    return v.size() & 1 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + (double)v[v.size() / 2]);
}

struct Place { long launches = 0, strict = 0, cont = 0, cont_of = 0; long first[8] = {0, 0, 0, 0, 0, 0, 0, 0}; };

int main(int argc, char **argv)
{
    const int replays = argc > 1 ? atoi(argv[1]) : 50;
    hipStream_t s; CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    char *buf; unsigned *sink; Slot *slots;
    const int per_step_max = 4 * MAXNB + 1;
    CK(hipMalloc(&buf, (size_t)2 * MAXNB * CHUNK)); CK(hipMemset(buf, 0, (size_t)2 * MAXNB * CHUNK));
    CK(hipMalloc(&sink, sizeof(unsigned))); CK(hipMemset(sink, 0, sizeof(unsigned)));
    CK(hipMalloc(&slots, sizeof(Slot) * STEPS * per_step_max));
    std::vector<Slot> h(STEPS * per_step_max);

    for (int nb : {300, 304}) {
        const int grid[3] = {nb, nb, 2 * nb + 1}, start[3] = {0, nb, 2 * nb}, per_step = 4 * nb + 1;
        hipGraphExec_t ge[2];
        for (int var = 0; var < 2; ++var) {  // 0: same, 1: far
            hipGraph_t g;
            CK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            for (int st = 0; st < STEPS; ++st) {
                Slot *o = slots + (size_t)st * per_step;
                hipLaunchKernelGGL(k_store, dim3(grid[0]), dim3(256), 0, s, buf, o + start[0], (unsigned)(st + 1));
                hipLaunchKernelGGL(k_time, dim3(grid[1]), dim3(256), 0, s, (const char *)buf, o + start[1], nb, var ? 4 : 0, sink);
                hipLaunchKernelGGL(k_time, dim3(grid[2]), dim3(256), 0, s, (const char *)buf, o + start[2], nb, var ? 4 : 0, sink);
            }
            CK(hipStreamEndCapture(s, &g)); CK(hipGraphInstantiate(&ge[var], g, nullptr, nullptr, 0));
            CK(hipGraphDestroy(g));
        }
        for (int w = 0; w < 4; ++w) CK(hipGraphLaunch(ge[w & 1], s));
        CK(hipStreamSynchronize(s));

        Place pl[3];
        long same_xcd_reads[2][3] = {{0, 0, 0}, {0, 0, 0}}, reads[2][3] = {{0, 0, 0}, {0, 0, 0}};
        printf("nb %d: grids %d %d %d, %d steps per graph, %d replays per run\n", nb, grid[0], grid[1], grid[2], STEPS, replays);
        for (int run = 0; run < 6; ++run) {  // three alternating runs of each variant
            const int var = run & 1;
            std::vector<unsigned> c2, r2, c3lo, r3lo, c3hi, r3hi;
            for (int rp = 0; rp < replays; ++rp) {
                CK(hipGraphLaunch(ge[var], s)); CK(hipStreamSynchronize(s));
                CK(hipMemcpy(h.data(), slots, sizeof(Slot) * STEPS * per_step, hipMemcpyDeviceToHost));
                int prev_first = -1, prev_grid = 0;
                for (int st = 0; st < STEPS; ++st)
                    for (int p = 0; p < 3; ++p) {
                        const Slot *o = h.data() + (size_t)st * per_step + start[p];
                        const int x0 = o[0].xcc & 7;
                        bool strict = true;
                        for (int b = 0; b < grid[p]; ++b) strict = strict && o[b].xcc == ((x0 + b) & 7);
                        pl[p].launches++; pl[p].strict += strict; pl[p].first[x0]++;
                        if (prev_first >= 0) { pl[p].cont_of++; pl[p].cont += x0 == ((prev_first + prev_grid) & 7); }
                        prev_first = x0; prev_grid = grid[p];
                        if (p == 0) continue;
                        const Slot *w = h.data() + (size_t)st * per_step;  // the storing launch of this step
                        for (int b = 0; b < grid[p]; ++b) {
                            reads[var][p]++;
                            same_xcd_reads[var][p] += w[(b % nb + (var ? 4 : 0)) % nb].xcc == o[b].xcc;
                            if (p == 1) { c2.push_back(o[b].cyc); r2.push_back(o[b].ref); }
                            else if (b < nb) { c3lo.push_back(o[b].cyc); r3lo.push_back(o[b].ref); }
                            else if (b < 2 * nb) { c3hi.push_back(o[b].cyc); r3hi.push_back(o[b].ref); }
                        }
                    }
            }
            printf("  run %d %-4s  launch 2: %6.1f memtime ticks, %5.1f x10ns | launch 3 [0,nb): %6.1f, %5.1f | launch 3 [nb,2nb): %6.1f, %5.1f\n",
                   run / 2 + 1, var ? "far" : "same", median(c2), median(r2), median(c3lo), median(r3lo), median(c3hi), median(r3hi));
        }
        for (int p = 0; p < 3; ++p) {
            printf("  launch %d (%d wgs): strict round-robin in %ld of %ld; continues the previous grid in %ld of %ld; xcc(0) seen:",
                   p + 1, grid[p], pl[p].strict, pl[p].launches, pl[p].cont, pl[p].cont_of);
            for (int x = 0; x < 8; ++x) printf(" %d:%ld", x, pl[p].first[x]);
            printf("\n");
        }
        for (int var = 0; var < 2; ++var)
            printf("  %-4s: reader on the storing XCD in %ld of %ld reads of launch 2, %ld of %ld of launch 3\n", var ? "far" : "same",
                   same_xcd_reads[var][1], reads[var][1], same_xcd_reads[var][2], reads[var][2]);
        CK(hipGraphExecDestroy(ge[0])); CK(hipGraphExecDestroy(ge[1]));
    }
    CK(hipFree(buf)); CK(hipFree(sink)); CK(hipFree(slots));
    return 0;
}
