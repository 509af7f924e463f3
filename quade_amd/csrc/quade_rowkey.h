// Device helpers shared by the post-passes that rebuild a pair's fused barcode key from the packed rows (the mismatch rescue,
// quade_mismatch.hip, and the unknown-barcode tally, quade_unknown.hip): unaligned slice loads and the shifted merge of the two
// index reads' parts into the canonical key words.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef uint64_t u64;

// nbytes (<= 8 * NW) bytes at p (any alignment) -> little-endian words, zero padded: aligned dword loads, no word read that
// holds no byte of the slice.  Same scheme as load_bytes in quade_generic.hip (wmax = nbytes: every listed pair covers its window).
template <int NW>
__device__ __forceinline__ void mm_load(const uint8_t* p, int nbytes, u64 (&w)[NW]) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
    const int sh = (int)(a & 3), need = sh + nbytes;
    const int ju = nbytes > 0 ? (nbytes + 6) >> 2 : 0;  // dwords that can hold 3 + nbytes bytes (uniform)
    const int jl = need > 0 ? (need - 1) >> 2 : 0;      // the lane's last needed dword: re-read instead of a per-lane branch
    uint32_t d[2 * NW + 1];
#pragma unroll
    for (int j = 0; j < 2 * NW + 1; ++j) d[j] = (j < ju) ? q[j < jl ? j : jl] : 0u;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const u64 lo = (u64)d[2 * i] | ((u64)d[2 * i + 1] << 32), nx = d[2 * i + 2];
        const u64 v = sh ? (lo >> (8 * sh)) | (nx << (64 - 8 * sh)) : lo;
        const int left = nbytes - 8 * i;
        w[i] = left >= 8 ? v : (left <= 0 ? 0 : v & ((1ull << (8 * left)) - 1));
    }
}

// w |= v << (8 * off) over the 64 * NW bits
template <int NW>
__device__ __forceinline__ void mm_or_shifted(u64 (&w)[NW], const u64 (&v)[NW], int off) {
    const int ws = off >> 3, bs = (off & 7) * 8;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        u64 cur = 0, prev = 0;
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            cur = (j == i - ws) ? v[j] : cur;
            prev = (j == i - ws - 1) ? v[j] : prev;
        }
        w[i] |= bs ? (cur << bs) | (prev >> (64 - bs)) : cur;
    }
}

}  // namespace
