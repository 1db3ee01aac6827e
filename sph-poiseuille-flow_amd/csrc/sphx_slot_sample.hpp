// sphx_slot_sample.hpp -- what the slot samplers' kernels share (k_flow_stats, k_step_history, k_field_map, k_point_probes, k_profile_series and their batch forms;
// DESIGN.md section 4, "Slot samplers").  A slot sampler is one self-skipping launch at the end of every step slot, behind
// the slot's clock update: clk->step / t / dt_last / vmax are those of the step just completed, and the state the slot left
// is what it samples.
#pragma once
#include "sphx_kernels.hpp"

namespace sphx {

// The gate of an in-loop sample closing the step slot of parity q: the slot ran iff run[q] is still set (a clock update only
// ever writes the flag of the NEXT slot), every `every`-th step, from t_from on.
__device__ __forceinline__ bool slot_due(const Clock *clk, int q, int every, double t_from)
{
    if (!clk->run[q]) return false;
    if (clk->step % every != 0) return false;
    if (!(clk->t >= t_from)) return false;
    return true;
}

// every >= 1: an in-loop sample, gated on the clock; every == 0: a sample of the state now, unconditionally
__device__ __forceinline__ bool sample_due(const Clock *clk, int q, int every, double t_from)
{
    return every > 0 ? slot_due(clk, q, every, t_from) : true;
}

// "Last workgroup out" with fences, for every thread of a workgroup whose global stores and adds are issued: each wave
// drains them, thread 0 releases at agent scope and draws the ticket, and the workgroup that draws the last one acquires.
// s_last ends up 1 in that workgroup and 0 in the others; whoever wins sets *ticket back to zero when it is done.
// Why two forms: what a sampler publishes are PLAIN stores and non-returning adds by many threads, read by other threads of
// the last workgroup, so they need the release / acquire pair.  last_workgroup_out (sphx_kernels.hpp) publishes RETURNING
// atomics and the drawing thread's own stores only, and does without a fence (which costs an L2 write-back per workgroup
// there, on hundreds of workgroups every step; a sampler has a few workgroups on the steps it samples).
__device__ __forceinline__ void last_out_fenced(int *ticket, int &s_last)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int drawn = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = drawn == (int)gridDim.x - 1 ? 1 : 0;
        if (s_last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
}

// one more sample at time t_now in a head with n_samples, t_first, t_last (FlowStatsHead, FieldMapHead); by one thread
template <typename Head>
__device__ __forceinline__ void note_sample(Head *h, double t_now)
{
    const long long ns = h->n_samples;
    if (ns == 0) h->t_first = t_now;
    h->t_last = t_now;
    h->n_samples = ns + 1;
}

}  // namespace sphx
