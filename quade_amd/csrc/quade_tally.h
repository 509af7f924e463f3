// Device-only primitives of the two device-resident key tallies: the unknown barcodes (quade_unknown.hip) and the duplication
// report's read-pair keys (quade_dup.hip).  Both count 64-bit-tagged keys of up to QD_KEY_WORDS words in an UnknownTable
// (quade_unknown.h: layout, tag, home slot, probe limit) by the same two-launch protocol:
//   claim : tally_claim per listed key -- a bounded linear probe over the tag words with a 64-bit compare-and-swap at agent scope;
//           the lane whose swap installed the tag writes the key words with plain vector stores;
//   count : a launch of its own, so that those stores are visible to every XCD at the kernel boundary.  Each lane compares its key
//           with the entry's (the caller), then tally_combine adds the equal slots of a wave together and hands one add per slot to
//           the workgroup's LDS hash of slot -> count (TallyLds), which is flushed once: a hot key costs one global atomic per
//           workgroup, not one per pair.
// The read-out (uk_gather behind qd_launch_unknown_gather) works on the table alone and serves both.
//
// Everything here is __device__ __forceinline__ in an unnamed namespace, as the kernels' own helpers are.
#ifndef QUADE_TALLY_H
#define QUADE_TALLY_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "quade_common.h"
#include "quade_unknown.h"

typedef uint64_t u64;

namespace {

constexpr int UK_BLOCK = 256;
constexpr int UK_LDS = 1024;      // entries of the workgroup's slot -> count hash
constexpr int UK_LDS_PROBES = 8;  // then the add goes to global memory directly
constexpr uint32_t UK_LDS_EMPTY = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t uk_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The slot of key k4 (its tag already trimmed): the entry that holds the tag, installed by this lane when no entry did (then
// ++installs and the key words are written here), or QD_UK_NONE when the probe limit is reached.
__device__ __forceinline__ uint32_t tally_claim(const UnknownTable& t, const u64 (&k4)[QD_KEY_WORDS], u64 tag, uint32_t& installs) {
    uint32_t s = qd_uk_home(tag, t.lg);
    for (uint32_t probe = 0; probe < t.probes; ++probe) {
        // a stale 0 is corrected by the swap; a tag word changes once only (0 -> tag), so a non-zero value read is final
        u64 cur = __hip_atomic_load(&t.tags[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS(reinterpret_cast<unsigned long long*>(&t.tags[s]), 0ull, (unsigned long long)tag);
            if (cur == 0) {  // this lane owns the entry: its key words, 2 x 16 bytes
                ulonglong2* kp = reinterpret_cast<ulonglong2*>(t.keys + (size_t)s * QD_KEY_WORDS);
                kp[0] = make_ulonglong2(k4[0], k4[1]);
                kp[1] = make_ulonglong2(k4[2], k4[3]);
                ++installs;
                return s;
            }
        }
        if (cur == tag) return s;
        s = (s + 1) & t.mask;
    }
    return QD_UK_NONE;
}

// the workgroup's installs -> the table's QD_UK_DISTINCT (installs_wg: LDS, zeroed before a barrier; every lane calls it)
__device__ __forceinline__ void tally_installs(const UnknownTable& t, uint32_t installs, uint32_t* installs_wg) {
    installs = uk_wave_sum(installs);
    if ((threadIdx.x & 63) == 0 && installs) atomicAdd(installs_wg, installs);
    __syncthreads();
    if (threadIdx.x == 0 && *installs_wg)
        atomicAdd(reinterpret_cast<unsigned long long*>(&t.totals[QD_UK_DISTINCT]), (unsigned long long)*installs_wg);
}

// c more pairs of `slot`: into the workgroup's hash, or to global memory when its probe sequence is taken
__device__ __forceinline__ void uk_add(uint32_t* lslot, uint32_t* lcnt, u64* counts, uint32_t slot, uint32_t c) {
    uint32_t h = (slot * 0x9E3779B1u) >> 22;  // 10 bits: UK_LDS entries
    for (int j = 0; j < UK_LDS_PROBES; ++j) {
        const uint32_t old = atomicCAS(&lslot[h], UK_LDS_EMPTY, slot);
        if (old == UK_LDS_EMPTY || old == slot) {
            atomicAdd(&lcnt[h], c);
            return;
        }
        h = (h + 1) & (UK_LDS - 1);
    }
    atomicAdd(reinterpret_cast<unsigned long long*>(&counts[slot]), (unsigned long long)c);
}

// every lane of the workgroup, before the first tally_combine (a barrier follows in the caller)
__device__ __forceinline__ void tally_lds_init(uint32_t* lslot, uint32_t* lcnt) {
    for (int i = threadIdx.x; i < UK_LDS; i += UK_BLOCK) {
        lslot[i] = UK_LDS_EMPTY;
        lcnt[i] = 0;
    }
}

// Every lane of the wave: a lane with pend adds one pair to slot res.  Equal slots are combined in the wave first (two rounds of
// leader election: a hot key is most of a wave), what is left goes lane by lane.
__device__ __forceinline__ void tally_combine(uint32_t* lslot, uint32_t* lcnt, u64* counts, bool pend, uint32_t res, int lane) {
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        const u64 m = __ballot(pend);
        if (m == 0) break;
        const int leader = __ffsll((unsigned long long)m) - 1;
        const uint32_t ls = __shfl(res, leader, 64);
        const bool mine = pend && res == ls;
        const u64 sm = __ballot(mine);
        if (lane == leader) uk_add(lslot, lcnt, counts, ls, (uint32_t)__popcll(sm));
        if (mine) pend = false;
    }
    if (pend) uk_add(lslot, lcnt, counts, res, 1u);
}

// every lane of the workgroup, behind a barrier after the last tally_combine: the hash's counts join the table's
__device__ __forceinline__ void tally_lds_flush(const uint32_t* lslot, const uint32_t* lcnt, u64* counts) {
    for (int i = threadIdx.x; i < UK_LDS; i += UK_BLOCK) {
        const uint32_t c = lcnt[i];
        if (c) atomicAdd(reinterpret_cast<unsigned long long*>(&counts[lslot[i]]), (unsigned long long)c);
    }
}

}  // namespace

#endif
