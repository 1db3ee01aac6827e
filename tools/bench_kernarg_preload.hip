// Micro-benchmark (manual tool, not part of the library): what does the first scalar round trip of a kernel -- the load of
// its leading arguments from the argument segment -- cost per launch on MI355X, and does the firmware deliver preloaded
// kernel arguments at all?  Build twice and compare the figures:
//   hipcc -O3 --offload-arch=gfx950 bench_kernarg_preload.hip -o bench_kernarg_plain
//   hipcc -O3 --offload-arch=gfx950 -mllvm -amdgpu-kernarg-preload-count=14 bench_kernarg_preload.hip -o bench_kernarg_preload
// The kernel has the shape of a compact step pass: 14 dwords of leading pointer / int parameters, a ~800-byte struct by value
// behind them, 300 workgroups of 256 threads; each thread loads through a leading pointer, loads again through the value it
// got, and stores.  A replayed hipGraph of dependent launches is timed with events.  A kernel built for preload keeps a
// prologue that loads the same arguments itself, so on firmware that ignores preload the two builds time the same.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1);} } while (0)

struct Rest {  // stands for Grid, Phys, FluidSet, FluidTmp, Walls: read late, after the dependent load
    double c[96];
    const double *tab;
    int n_tab, pad[5];
};
static_assert(sizeof(Rest) >= 800 && sizeof(Rest) <= 832, "about the size of the step kernels' structs");

// 6 pointers (12 dwords) + 2 ints = 14 dwords
__global__ __launch_bounds__(256) void k_pass(const int *idx, const double *src, double *dst, const int *run, const double *aux,
                                              const int *cnt, int n, int q, Rest r)
{
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    const bool in = i < n;
    const int k = in ? idx[i] : 0;      // wave 1: through leading pointers
    const int c = in ? cnt[i] : 0;
    const int go = run[q];
    const double a = aux[in ? i : 0];
    if (!go) return;
    const double v = src[k];            // wave 2: the dependent load
    if (in) dst[i] = v + a + (double)c + r.c[q] * r.tab[min(k, r.n_tab - 1)];
}

int main(int argc, char **argv)
{
    const int launches = argc > 1 ? atoi(argv[1]) : 600, reps = argc > 2 ? atoi(argv[2]) : 15;
    const int blocks = 300, n = blocks * 256 - 100;  // a partial last workgroup
    hipStream_t s; CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    std::vector<int> h_idx(n), h_cnt(n, 1);
    for (int i = 0; i < n; ++i) h_idx[i] = (int)(((long long)i * 7919) % n);
    std::vector<double> h_src(n, 1.0);
    int *idx, *cnt, *run; double *buf[2], *aux, *tab;
    CK(hipMalloc(&idx, n * sizeof(int))); CK(hipMalloc(&cnt, n * sizeof(int))); CK(hipMalloc(&run, 2 * sizeof(int)));
    CK(hipMalloc(&buf[0], n * sizeof(double))); CK(hipMalloc(&buf[1], n * sizeof(double)));
    CK(hipMalloc(&aux, n * sizeof(double))); CK(hipMalloc(&tab, 64 * sizeof(double)));
    CK(hipMemcpy(idx, h_idx.data(), n * sizeof(int), hipMemcpyHostToDevice));
    CK(hipMemcpy(cnt, h_cnt.data(), n * sizeof(int), hipMemcpyHostToDevice));
    CK(hipMemcpy(buf[0], h_src.data(), n * sizeof(double), hipMemcpyHostToDevice));
    CK(hipMemcpy(buf[1], h_src.data(), n * sizeof(double), hipMemcpyHostToDevice));
    CK(hipMemset(aux, 0, n * sizeof(double))); CK(hipMemset(tab, 0, 64 * sizeof(double)));
    const int h_run[2] = {1, 1};
    CK(hipMemcpy(run, h_run, sizeof(h_run), hipMemcpyHostToDevice));
    Rest r{};
    for (int j = 0; j < 96; ++j) r.c[j] = 0.5;
    r.tab = tab; r.n_tab = 64;
    // dependent launches: each reads what the one before wrote (ping-pong), as the passes of a step do
    hipGraph_t g; hipGraphExec_t ge;
    CK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    for (int it = 0; it < launches; ++it)
        hipLaunchKernelGGL(k_pass, dim3(blocks), dim3(256), 0, s, (const int *)idx, (const double *)buf[it & 1], buf[(it + 1) & 1],
                           (const int *)run, (const double *)aux, (const int *)cnt, n, it & 1, r);
    CK(hipStreamEndCapture(s, &g)); CK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    for (int w = 0; w < 3; ++w) CK(hipGraphLaunch(ge, s));
    CK(hipStreamSynchronize(s));
    std::vector<double> us(reps);
    for (int rep = 0; rep < reps; ++rep) {
        float ms;
        CK(hipEventRecord(a, s)); CK(hipGraphLaunch(ge, s)); CK(hipEventRecord(b, s)); CK(hipStreamSynchronize(s));
        CK(hipEventElapsedTime(&ms, a, b));
        us[rep] = 1e3 * ms / launches;
    }
    std::sort(us.begin(), us.end());
    double out = 0.0;
    CK(hipMemcpy(&out, buf[launches & 1], sizeof(double), hipMemcpyDeviceToHost));
    printf("%d dependent launches of %d x 256, %d replays: us per launch min %.3f median %.3f max %.3f (dst[0] = %g)\n", launches,
           blocks, reps, us.front(), us[reps / 2], us.back(), out);
    CK(hipGraphExecDestroy(ge)); CK(hipGraphDestroy(g));
    return 0;
}
