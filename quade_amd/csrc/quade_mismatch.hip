// gfx950 (CDNA4 / MI355X): mismatch-tolerant matching, the post-pass behind an exact-match launch (qd_set_mismatches).
//
// Only when a budget is set.  Two kernels on the launch's stream, after the fast / generic / fixup kernels:
//   mm_compact : reads the batch's routing codes 16 bytes per lane and lists the undetermined pairs (one atomic per workgroup);
//   mm_rescue  : one lane per listed pair.  It gathers the pair's fused key and barcode qualities from the rows (as the
//                generic kernel does), skips pairs whose key slice is short (rows are zero padded where a read ends), finds
//                candidates by pigeonhole -- within budget m one of a part's m + 1 segments is equal, and the host hashed the
//                segments of one part to candidate lists -- and verifies each candidate with 64-bit SWAR per-part Hamming
//                distances.  The collision rule (checked on the host before any table is built) leaves at most one sample
//                within budget, so the first one found is the answer.  Counts move into the 64-bit totals, aggregated per
//                workgroup in an LDS histogram.
// The exact-match kernels are untouched: a pair that matched exactly keeps its code.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <map>
#include <thread>

#include "quade_kernels.h"
#include "quade_mismatch.h"
#include "quade_rowkey.h"

namespace {

typedef uint64_t u64;
constexpr int MM_BLOCK = 256;
constexpr int MM_ITERS = 16;  // 8-code groups per lane of mm_compact

// undetermined flags of the 8 codes codes[base .. base + 8) (bit i = codes[base + i]); 16-byte loads where all 8 are in the batch
__device__ __forceinline__ uint32_t mm_undet_bits(const uint16_t* codes, int64_t n, int64_t base) {
    uint32_t bits = 0;
    if (base + 8 <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(codes + base);  // codes is 16-byte aligned (launch() checks)
        const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bits |= ((d[i] & 0xFFFFu) == QD_CODE_UNDET ? 1u : 0u) << (2 * i);
            bits |= ((d[i] >> 16) == QD_CODE_UNDET ? 1u : 0u) << (2 * i + 1);
        }
    } else {
        for (int i = 0; i < 8; ++i)
            if (base + i < n && codes[base + i] == QD_CODE_UNDET) bits |= 1u << i;
    }
    return bits;
}

// A workgroup takes MM_ITERS x 256 x 8 consecutive codes, keeps their flags in registers, and reserves room for all of its
// misses with ONE atomic: with one atomic per wave (512 codes) the ~200 k atomics of a 100 M-pair batch on a single word took
// 2.2 ms, four times the exact-match kernel (tools/mismatch_bench.py, rocprofv3 kernel trace).
__global__ __launch_bounds__(MM_BLOCK) void mm_compact(const uint16_t* codes, int64_t n, uint32_t* miss) {
    __shared__ uint32_t wsum[MM_BLOCK / 64];
    __shared__ uint32_t bbase;
    const int64_t g0 = (int64_t)blockIdx.x * MM_BLOCK * MM_ITERS + threadIdx.x;
    uint32_t bits[MM_ITERS];
    uint32_t c = 0;
#pragma unroll
    for (int it = 0; it < MM_ITERS; ++it) {
        bits[it] = mm_undet_bits(codes, n, (g0 + (int64_t)it * MM_BLOCK) * 8);
        c += __popc(bits[it]);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (int w = 0; w < MM_BLOCK / 64; ++w) total += wsum[w];
        bbase = total ? atomicAdd(miss, total) : 0;
    }
    __syncthreads();
    size_t at = (size_t)bbase + inc - c;
    for (int w = 0; w < wave; ++w) at += wsum[w];
#pragma unroll
    for (int it = 0; it < MM_ITERS; ++it) {
        uint32_t b = bits[it];
        const int64_t base = (g0 + (int64_t)it * MM_BLOCK) * 8;
        while (b) {
            const int i = __ffs(b) - 1;
            b &= b - 1;
            miss[4 + at++] = (uint32_t)(base + i);
        }
    }
}

template <int KW>
__device__ __forceinline__ bool mm_within(const MismatchParams& p, const u64 (&w)[KW], uint32_t id) {
    const u64* b = p.bk32 + (size_t)id * QD_KEY_WORDS;
    int d0 = 0, d1 = 0;
#pragma unroll
    for (int q = 0; q < KW; ++q) {
        const u64 nz = qd_nz_bytes(w[q] ^ b[q]);
        d0 += __popcll(nz & p.part[0][q]);
        d1 += __popcll(nz & p.part[1][q]);
    }
    return d0 <= p.m[0] && d1 <= p.m[1];
}

template <int KW>
__global__ __launch_bounds__(MM_BLOCK) void mm_rescue(const MismatchParams p) {
    extern __shared__ uint32_t hist[];  // 2S pass / fail counters of this workgroup (hist_entries, 0 = global atomics)
    const uint32_t S = p.n_samples;
    for (uint32_t i = threadIdx.x; i < p.hist_entries; i += MM_BLOCK) hist[i] = 0;
    if (p.hist_entries) __syncthreads();
    const uint32_t nm = p.miss[0];
    const u64 L = 0x0101010101010101ull, H = 0x8080808080808080ull;
    uint32_t moved = 0;
    for (uint32_t i = blockIdx.x * MM_BLOCK + threadIdx.x; i < nm; i += gridDim.x * MM_BLOCK) {
        const int64_t r = p.miss[4 + (size_t)i];
        if (r >= p.n) continue;
        u64 w[KW];
#pragma unroll
        for (int q = 0; q < KW; ++q) w[q] = 0;
        uint32_t pass = 1;
        bool full = true;
        int at = 0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (k >= p.n_streams) break;
            const int iw = p.idx_w[k];
            u64 v[KW], qv[KW];
            mm_load<KW>(p.seq[k] + r * p.seq_stride[k] + p.idx_off[k], iw, v);
            mm_load<KW>(p.qual[k] + r * p.qual_stride[k], iw, qv);
#pragma unroll
            for (int q = 0; q < KW; ++q) {
                const int left = iw - 8 * q;  // bytes of this word inside the slice; the others read as 0xFF
                const u64 keep = left >= 8 ? 0 : (left <= 0 ? ~0ull : ~0ull << (8 * left));
                const u64 x = v[q] | keep;
                full = full && (((x - L) & ~x & H) == 0);  // a zero byte: the read ends inside its slice
                v[q] = qd_fold8(v[q]);
                pass &= qd_all_ge8(qv[q] | keep, p.thr);
            }
            mm_or_shifted<KW>(w, v, at);
            at += iw;
        }
        if (!full) continue;  // short slice: exact matching only
        int found = -1;
        if (p.nseg == 0) {
            for (uint32_t c = 0; c < p.ncand && found < 0; ++c)
                if (mm_within<KW>(p, w, p.cand[c])) found = p.cand[c];
        } else {
            for (int j = 0; j < p.nseg && found < 0; ++j) {
                u64 s[QD_KEY_WORDS] = {0, 0, 0, 0};
#pragma unroll
                for (int q = 0; q < KW; ++q) s[q] = w[q] & p.segmask[j][q];
                const u64 tag = qd_mm_seg_tag(s, j);
                uint32_t h = (uint32_t)(tag >> 17) & p.hmask;
                for (;;) {
                    const QdMmBucket b = p.htab[h];
                    if (b.count == 0) break;
                    if (b.tag_lo == (uint32_t)tag && b.tag_hi == (uint32_t)(tag >> 32)) {
                        for (uint32_t c = 0; c < b.count && found < 0; ++c)
                            if (mm_within<KW>(p, w, p.cand[b.start + c])) found = p.cand[b.start + c];
                        break;
                    }
                    h = (h + 1) & p.hmask;
                }
            }
        }
        if (found < 0) continue;
        const uint32_t code = (uint32_t)found * 2u + (pass ^ 1u);
        p.codes[r] = (uint16_t)code;
        ++moved;
        if (p.hist_entries) atomicAdd(&hist[code], 1u);
        else atomicAdd(reinterpret_cast<unsigned long long*>(&p.adjust[code]), 1ull);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) moved += __shfl_xor(moved, o, 64);
    if ((threadIdx.x & 63) == 0 && moved)  // -moved on UNDETERMINED
        atomicAdd(reinterpret_cast<unsigned long long*>(&p.adjust[2 * S]), (unsigned long long)(-(int64_t)moved));
    if (p.hist_entries) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < p.hist_entries; i += MM_BLOCK) {
            const uint32_t v = hist[i];
            if (v) atomicAdd(reinterpret_cast<unsigned long long*>(&p.adjust[i]), (unsigned long long)v);
        }
    }
}

// canonical key (quade_api.cpp canon)
void mm_canon(const uint8_t* b, int len, u64 w[QD_KEY_WORDS]) {
    for (int i = 0; i < QD_KEY_WORDS; ++i) w[i] = 0;
    for (int i = 0; i < len && i < QD_MAX_KEY_BYTES; ++i) w[i >> 3] |= (u64)b[i] << (8 * (i & 7));
}

// 0x01 lanes of the two parts [0, w1) and [w1, K)
void mm_parts(int K, int w1, u64 (&part)[2][QD_KEY_WORDS]) {
    for (int p = 0; p < 2; ++p)
        for (int q = 0; q < QD_KEY_WORDS; ++q) part[p][q] = 0;
    for (int i = 0; i < K; ++i) part[i < w1 ? 0 : 1][i >> 3] |= 1ull << (8 * (i & 7));
}

}  // namespace

bool qd_mm_first_collision(int32_t S, const uint8_t* barcodes, const int32_t* offsets, int32_t K, int32_t w1, int32_t m1, int32_t m2,
                           int32_t* first, int32_t* second) {
    std::vector<int32_t> ids;
    std::vector<u64> keys;
    for (int i = 0; i < S; ++i) {
        if (offsets[i + 1] - offsets[i] != K) continue;  // a barcode of another length matches exactly only
        ids.push_back(i);
        keys.resize(keys.size() + QD_KEY_WORDS);
        mm_canon(barcodes + offsets[i], K, &keys[keys.size() - QD_KEY_WORDS]);
    }
    u64 part[2][QD_KEY_WORDS];
    mm_parts(K, w1, part);
    const int nw = (K + 7) / 8, t1 = 2 * m1, t2 = 2 * m2;
    const int64_t n = (int64_t)ids.size();
    // rows i are dealt round robin; a thread stops at its first hit (its rows ascend) or behind a row that already has one
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>({16, (int64_t)std::max(1u, std::thread::hardware_concurrency()), n / 512}));
    std::atomic<int64_t> best_row(n);
    std::vector<std::pair<int64_t, int64_t>> hit((size_t)T, std::make_pair(n, n));
    auto scan = [&](int t) {
        for (int64_t a = t; a < n && a < best_row.load(std::memory_order_relaxed); a += T) {
            const u64* x = &keys[(size_t)a * QD_KEY_WORDS];
            for (int64_t b = a + 1; b < n; ++b) {
                const u64* y = &keys[(size_t)b * QD_KEY_WORDS];
                int d1 = 0, d2 = 0;
                for (int q = 0; q < nw; ++q) {
                    const u64 z = qd_nz_bytes(x[q] ^ y[q]);
                    d1 += __builtin_popcountll(z & part[0][q]);
                    d2 += __builtin_popcountll(z & part[1][q]);
                }
                if (d1 <= t1 && d2 <= t2) {
                    hit[(size_t)t] = std::make_pair(a, b);
                    int64_t cur = best_row.load();
                    while (a < cur && !best_row.compare_exchange_weak(cur, a)) {
                    }
                    return;
                }
            }
        }
    };
    if (T == 1) {
        scan(0);
    } else {
        std::vector<std::thread> th;
        for (int t = 0; t < T; ++t) th.emplace_back(scan, t);
        for (auto& x : th) x.join();
    }
    const auto best = *std::min_element(hit.begin(), hit.end());
    if (best.first >= n) return false;
    *first = ids[(size_t)best.first];
    *second = ids[(size_t)best.second];
    return true;
}

void qd_mm_build(int32_t S, const uint8_t* barcodes, const int32_t* offsets, int32_t K, int32_t w1, int32_t m1, int32_t m2,
                 MismatchParams& p, std::vector<QdMmBucket>& htab, std::vector<uint16_t>& cand) {
    std::vector<int32_t> ids;
    std::vector<u64> keys;
    for (int i = 0; i < S; ++i) {
        if (offsets[i + 1] - offsets[i] != K) continue;
        ids.push_back(i);
        keys.resize(keys.size() + QD_KEY_WORDS);
        mm_canon(barcodes + offsets[i], K, &keys[keys.size() - QD_KEY_WORDS]);
    }
    p.m[0] = m1;
    p.m[1] = m2;
    mm_parts(K, w1, p.part);
    // per usable part (as wide as its budget + 1 segments at least): segment tag -> candidate ordinals; the part whose longest
    // list is shorter wins (combinatorial kits share one i7 across many samples)
    const int off[2] = {0, w1}, width[2] = {w1, K - w1}, budget[2] = {m1, m2};
    int best = -1;
    size_t best_longest = ~(size_t)0;
    std::map<u64, std::vector<uint16_t>> best_lists;
    u64 best_mask[QD_MM_MAX_SEG][QD_KEY_WORDS] = {};
    for (int pt = 0; pt < 2; ++pt) {
        const int nseg = budget[pt] + 1;
        if (width[pt] < nseg) continue;
        u64 mask[QD_MM_MAX_SEG][QD_KEY_WORDS] = {};
        for (int j = 0; j < nseg; ++j)
            for (int i = off[pt] + width[pt] * j / nseg; i < off[pt] + width[pt] * (j + 1) / nseg; ++i) mask[j][i >> 3] |= 0xFFull << (8 * (i & 7));
        std::map<u64, std::vector<uint16_t>> lists;
        for (size_t a = 0; a < ids.size(); ++a)
            for (int j = 0; j < nseg; ++j) {
                u64 s[QD_KEY_WORDS];
                for (int q = 0; q < QD_KEY_WORDS; ++q) s[q] = keys[a * QD_KEY_WORDS + q] & mask[j][q];
                lists[qd_mm_seg_tag(s, j)].push_back((uint16_t)ids[a]);
            }
        size_t longest = 0;
        for (auto& kv : lists) longest = std::max(longest, kv.second.size());
        if (longest < best_longest) {
            best = pt;
            best_longest = longest;
            best_lists.swap(lists);
            memcpy(best_mask, mask, sizeof mask);
        }
    }
    cand.clear();
    uint32_t m = 16;
    if (best < 0) {  // neither part can be split: every K-long barcode is a candidate
        p.nseg = 0;
        for (int32_t id : ids) cand.push_back((uint16_t)id);
        p.ncand = (uint32_t)cand.size();
    } else {
        p.nseg = budget[best] + 1;
        memcpy(p.segmask, best_mask, sizeof best_mask);
        p.ncand = 0;
        while (m < 2 * best_lists.size()) m <<= 1;
    }
    htab.assign(m, QdMmBucket{0, 0, 0, 0});
    p.hmask = m - 1;
    for (auto& kv : best_lists) {
        uint32_t h = (uint32_t)(kv.first >> 17) & p.hmask;
        while (htab[h].count) h = (h + 1) & p.hmask;
        htab[h] = QdMmBucket{(uint32_t)kv.first, (uint32_t)(kv.first >> 32), (uint32_t)cand.size(), (uint32_t)kv.second.size()};
        cand.insert(cand.end(), kv.second.begin(), kv.second.end());
    }
    if (cand.empty()) cand.push_back(0);  // never read (ncand 0, no bucket), keeps the device array non-empty
}

hipError_t qd_launch_compact(const uint16_t* codes, int64_t n, uint32_t* miss, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(miss, 0, 4, st);
    if (e != hipSuccess) return e;
    const int64_t groups = (n + 7) / 8, per_block = (int64_t)MM_BLOCK * MM_ITERS;
    hipLaunchKernelGGL(mm_compact, dim3((unsigned)((groups + per_block - 1) / per_block)), dim3(MM_BLOCK), 0, st, codes, n, miss);
    return hipGetLastError();
}

hipError_t qd_launch_mismatch(const MismatchParams& p, uint32_t* miss, int cus, hipStream_t st) {
    if (p.n <= 0) return hipSuccess;
    hipError_t e = qd_launch_compact(p.codes, p.n, miss, st);
    if (e != hipSuccess) return e;
    const int64_t nb = (p.n + MM_BLOCK - 1) / MM_BLOCK;
    const unsigned grid = (unsigned)std::min<int64_t>(nb, (int64_t)cus * 8);
    const size_t lds = (size_t)p.hist_entries * 4;
    if (p.K <= 16) hipLaunchKernelGGL(mm_rescue<2>, dim3(grid), dim3(MM_BLOCK), lds, st, p);
    else hipLaunchKernelGGL(mm_rescue<4>, dim3(grid), dim3(MM_BLOCK), lds, st, p);
    return hipGetLastError();
}
