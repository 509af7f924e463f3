// gfx950 (CDNA4 / MI355X): trailing-N, poly-X tail trimming and the max_length crop of a batch's insert reads (qd_posttrim_set)
// while their text sits in HBM, behind the clip, 3' trimming and overlap trimming stages.  A post-trim is a new seq_len: the kernel
// writes copies of the record tables it receives and counts what it cut.  include/quade_hip.h states the rule.
//
// Shape (quade_row.h's searching stage): 16 lanes (one DPP row) share a read; blockIdx.y says R1 or R2.  The sequence line is
// staged in the row's slab of LDS with its case folded; the quality line is never loaded.
//   trailing N : t counts bases from the 3' end, in rounds of 64: lane i looks at t = 4 i + 1 .. 4 i + 4 of the round and notes the
//                first base that is no N; the row minimum ends the count.  A read without an N at its end stops in the first round.
//   poly-X     : a walk for X can cut only if it is alive at t = P, that is with at most min(5, P / 8) bases other than X among
//                the last P, and two bases cannot both be that rare (every byte differs from one of them, and 2 (P / 8) < P).  So
//                the row counts A, C, G and T over the last P bytes, four counts packed in a word, and walks once, for the one
//                base that passes -- or not at all.  The walk is the clip stage's poly-G walk with the base as a value: rounds of
//                64, lane i takes t = 4 i + 1 .. 4 i + 4, the counts of other bases are scanned over the row, every lane walks its
//                four bases again from the true count, notes the first t at which the walk stops and the last X in front of it.
//                The lowest lane that stopped ends the walk; the largest X position of the lanes up to it is the cut.
// A line of more than 21 words does not fit its slab: the same steps then read bytes from global memory.  With neither rule
// configured (a crop alone) no text is read.  Every lane of a row keeps one of the sixteen counters in a register (quade_row.h's
// flush_row_counters).
#include <hip/hip_runtime.h>

#include "quade_row.h"
#include "quade_posttrim.h"

namespace {

constexpr uint32_t PO_BLOCK = 256;
constexpr uint32_t PO_GROUPS = PO_BLOCK / ROW;      // reads per step of a workgroup
constexpr uint32_t PO_WG_READS = 1024;              // reads per workgroup
constexpr uint32_t PO_STEP = 4;                     // bases per lane and round of the two walks
constexpr uint32_t PO_NONE = 0xFFFFFFFFu;
static_assert(PO_WG_READS % PO_GROUPS == 0, "whole steps");
static_assert(QD_POST_COUNTERS == ROW, "one counter per lane of the row");
static_assert(QD_POST_MAX_POLYX < 256, "the four letter counts share a word");

// Trailing-N rule over s[0 .. L) (the bytes are folded here: a staged line is folded already): k, the N bytes at the 3' end, in
// every lane
template <typename PTR>
__device__ __forceinline__ uint32_t tail_n_count(PTR s, uint32_t L, uint32_t sub) {
    constexpr uint32_t ROUND = ROW * PO_STEP;
    for (uint32_t t0 = 0; t0 < L; t0 += ROUND) {
        const uint32_t n = min(L - t0, ROUND);
        const uint32_t a = min(sub * PO_STEP, n), b = min(a + PO_STEP, n);  // this lane: the bytes L - 1 - (t0 + a) down to L - (t0 + b)
        uint32_t first = PO_NONE;
        for (uint32_t i = a; i < b; ++i)
            if ((s[L - 1 - (t0 + i)] & 0xDFu) != 'N') {
                first = t0 + i;
                break;
            }
        first = row_min(first);  // as many N lie behind the first other byte
        if (first != PO_NONE) return first;
    }
    return L;
}

// A, C, G and T among the last P bytes of s[0 .. Ln), Ln >= P: the counts in bytes 0 .. 3 of a word, in every lane
template <typename PTR>
__device__ __forceinline__ uint32_t tail_letters(PTR s, uint32_t Ln, uint32_t P, uint32_t sub) {
    uint32_t c = 0;
    for (uint32_t i = sub; i < P; i += ROW) {
        const uint32_t b = s[Ln - 1 - i] & 0xDFu;
        c += b == 'A' ? 1u : b == 'C' ? 1u << 8 : b == 'G' ? 1u << 16 : b == 'T' ? 1u << 24 : 0u;
    }
    return row_sum(c);
}

// The poly-X walk for the base x over s[0 .. Lw) with minimum run P >= 6 (the clip stage's poly-G walk, the base a value): Lx in
// every lane
template <typename PTR>
__device__ __forceinline__ uint32_t polyx_walk(PTR s, uint32_t Lw, uint32_t P, uint32_t x, uint32_t sub) {
    constexpr uint32_t ROUND = ROW * PO_STEP;
    uint32_t mm0 = 0, g = 0;  // mismatches and the largest X position of the rounds done
    for (uint32_t t0 = 0; t0 < Lw;) {
        const uint32_t n = min(Lw - t0, ROUND);
        const uint32_t a = min(sub * PO_STEP, n), b = min(a + PO_STEP, n);  // this lane: t = t0 + a + 1 .. t0 + b
        uint32_t c = 0;
        for (uint32_t i = a; i < b; ++i) c += (s[Lw - 1 - (t0 + i)] & 0xDFu) != x;
        uint32_t mm = mm0 + row_sum_below(c);
        uint32_t stop = PO_NONE, last = 0;
        for (uint32_t i = a; i < b; ++i) {
            const uint32_t t = t0 + i + 1;
            const bool is_x = (s[Lw - t] & 0xDFu) == x;
            mm += !is_x;
            if (mm > 5 || (t >= P && 8 * mm > t)) {
                stop = t;
                break;
            }
            if (is_x) last = t;
        }
        // stretches ascend with the lane: the lowest lane that stopped holds the first stop; the lanes above it saw nothing real
        const uint32_t w = row_min(stop != PO_NONE ? sub : ROW);
        g = max(g, row_max(sub <= w ? last : 0u));
        if (w < ROW) {
            const uint32_t T = row_min(stop);
            return T - 1 >= P ? Lw - g : Lw;
        }
        mm0 = row_max(mm);  // no lane stopped: the counts ascend with the lane
        t0 += n;
    }
    return Lw >= P ? Lw - g : Lw;  // the walk reached the 5' end
}

// Steps 1 and 2 over s[0 .. L): Ln, Lp and the tail base (0 .. 3 for A, C, G, T; PO_NONE: no base cut), in every lane
template <typename PTR>
__device__ __forceinline__ void tail_rules(PTR s, uint32_t L, const qd_posttrim_dev& P, uint32_t sub, uint32_t& Ln, uint32_t& Lp, uint32_t& base) {
    Ln = P.tail_n ? L - tail_n_count(s, L, sub) : L;
    Lp = Ln;
    base = PO_NONE;
    if (!P.poly_x || Ln < P.poly_x) return;  // a walk cuts a run of at least P bases
    const uint32_t letters = tail_letters(s, Ln, P.poly_x, sub), most = P.poly_x - min(5u, P.poly_x / 8);
    uint32_t b = PO_NONE;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
        if (((letters >> (8 * k)) & 0xFFu) >= most) b = k;
    if (b == PO_NONE) return;
    Lp = polyx_walk(s, Ln, P.poly_x, (uint32_t)(b == 0 ? 'A' : b == 1 ? 'C' : b == 2 ? 'G' : 'T'), sub);
    if (Lp < Ln) base = b;
}

__global__ __launch_bounds__(PO_BLOCK) void posttrim_reads(qd_posttrim_dev P, qd_posttrim_args a, uint32_t n) {
    __shared__ uint4 slab[PO_GROUPS][FAST_WORDS];  // per row: the folded sequence line (read by bytes: no dword ahead)
    __shared__ unsigned long long part[QD_POST_COUNTERS];
    const uint32_t r = blockIdx.y;
    if (threadIdx.x < QD_POST_COUNTERS) part[threadIdx.x] = 0;
    const uint32_t sub = threadIdx.x & (ROW - 1), group = threadIdx.x / ROW;
    const uint8_t* text = a.text[r];
    const qd_rec* recs = a.recs[r];
    qd_rec* out = a.out[r];
    const uint32_t M = P.max_length[r];
    const bool reads_text = P.tail_n || P.poly_x;
    uint4* ss = slab[group];
    uint64_t acc = 0;  // counter `sub` of this row's reads
    const uint32_t first = blockIdx.x * PO_WG_READS, last = min(n, first + PO_WG_READS);
    for (uint32_t j0 = first; j0 < last; j0 += PO_GROUPS) {  // (the same trips for every wave: a barrier inside)
        const uint32_t j = j0 + group;
        const bool valid = j < last;
        qd_rec rec{};
        if (valid) rec = recs[j];
        const uint32_t L = rec.seq_len;
        const Line sl = make_line(text, rec.seq, L);
        const bool staged = sl.n_words <= FAST_WORDS;
        __syncthreads();  // the row's earlier read is done with the slab
        if (staged && reads_text) stage_line<true>(ss, sl, sub);
        __syncthreads();
        uint32_t Ln = L, Lp = L, base = PO_NONE;
        if (reads_text) {
            if (staged) tail_rules(reinterpret_cast<const uint8_t*>(ss) + sl.s, L, P, sub, Ln, Lp, base);
            else tail_rules(text + rec.seq, L, P, sub, Ln, Lp, base);
        }
        const uint32_t Lm = M ? min(Lp, M) : Lp;
        const uint32_t Lout = max(Lm, min(P.min_length, L));
        if (valid) {
            if (sub == 0) {
                rec.seq_len = Lout;
                out[j] = rec;
            }
            const uint32_t cut = Ln - Lp;
            const uint32_t v[QD_POST_COUNTERS] = {1u, L, Lout, Ln < L, L - Ln, base == 0, base == 0 ? cut : 0u, base == 1, base == 1 ? cut : 0u,
                                                  base == 2, base == 2 ? cut : 0u, base == 3, base == 3 ? cut : 0u, Lm < Lp, Lp - Lm, Lout > Lm};
#pragma unroll
            for (uint32_t i = 0; i < QD_POST_COUNTERS; ++i)
                if (sub == i) acc += v[i];
        }
    }
    flush_row_counters<QD_POST_COUNTERS>(acc, sub, part, reinterpret_cast<unsigned long long*>(a.table) + r * QD_POST_COUNTERS);
}

}  // namespace

hipError_t qd_posttrim_launch(const qd_posttrim_dev& P, const qd_posttrim_args& a, uint32_t n, hipStream_t st) {
    if (!n) return hipSuccess;
    if (n > 0x7FFFFFFFu || P.tail_n > 1 || (P.poly_x && (P.poly_x < QD_POST_MIN_POLYX || P.poly_x > QD_POST_MAX_POLYX))) return hipErrorInvalidValue;
    const uint32_t grid = (n + PO_WG_READS - 1) / PO_WG_READS;
    hipLaunchKernelGGL(posttrim_reads, dim3(grid, 2), dim3(PO_BLOCK), 0, st, P, a, n);
    return hipGetLastError();
}
