// sphx_xcd_block.hpp -- which block of a pass a workgroup takes.  Plain C++ as well as HIP: tests/test_xcd_block_host.py
// compiles it into a host program.
#pragma once
#if defined(__HIPCC__)
#define SPHX_HOST_DEVICE __host__ __device__
#else
#define SPHX_HOST_DEVICE
#endif

namespace sphx {

// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b+8 share an L2).  Give each XCD one
// contiguous eighth of the particle range instead, so the neighbour columns a block reads are the ones
// the previous block on the same XCD just pulled into that XCD's L2 (measured at 6 M particles without
// this: k_forces fetched 4x its algorithmic bytes from HBM, L2 hit rate 36 %).  Speed only.
// A pass whose workgroups are the physical blocks first + j, j in [0, nb) (the A half of the fused
// launch): the eighth is chosen by the PHYSICAL residue c = (first + j) & 7, so that eighth c runs on the same XCD in every
// pass of a step and a pass finds what the pass before it stored in its own L2 (every dispatch starts its round-robin on the
// same XCD; a line an XCD stored still hits its L2 behind a kernel boundary: profiles/r27_xcd_affinity.txt).  The k-th
// workgroup of residue c takes block c * per + k; the nb % 8 workgroups left over take the blocks behind the eight eighths.
// (The first j of residue c is j0 = (c - first) & 7 = j & 7, and k = (j - j0) >> 3 = j >> 3; first % 8 == 0 is the mapping of
//  a pass that starts at physical block 0.)
SPHX_HOST_DEVICE inline int xcd_block(int first, int j, int nb)
{
    const int per = nb >> 3, c = (first + j) & 7;
    return j < (per << 3) ? c * per + (j >> 3) : j;
}

}  // namespace sphx
