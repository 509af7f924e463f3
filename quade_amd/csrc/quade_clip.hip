// gfx950 (CDNA4 / MI355X): end clipping, sliding-window quality trimming and poly-G tail trimming of a batch's insert reads
// (qd_clip_set) while their text sits in HBM.  A clip is a new seq, qual and seq_len: the kernel writes copies of the scan's
// record tables and counts what it cut.  include/quade_hip.h states the rule.
//
// Shape (quade_row.h's searching stage): 16 lanes (one DPP row) share a read; blockIdx.y says R1 or R2.  What the fixed clip
// leaves of the quality and the sequence line is staged in the row's slab of LDS, the sequence with its case folded.
//   window : lane i takes the starts in the i-th stretch of T = ceil(Lc / 16) bytes, slides the window over them and notes the first
//            that fails; the row minimum is the cut.  The window's sum at the lane's first start: for W <= 2 T its W bytes are
//            added up; for a longer window the stretch sums are scanned over the row (DPP row_shr), which gives every lane the
//            prefix sum at its first byte, the prefix sum W bytes further on is the one of the lane that holds that byte
//            (ds_bpermute) plus the bytes up to it, and the window's sum is the difference of the two running prefix sums.
//   poly-G : t counts bases from the 3' end, in rounds of 64: lane i takes t = 4 i + 1 .. 4 i + 4 of the round, the counts of
//            bases other than G are scanned over the row, and every lane walks its four bases again from the true count, notes the
//            first t at which the walk stops and the last G in front of it.  The lowest lane that stopped ends the walk; the
//            largest G position of the lanes up to it is the cut.  A read without a G tail stops in the first round.
// A line of more than 21 words does not fit its slab: the same two walks then read bytes from global memory, the window's sums in
// 64 bits.  Lanes 0 .. 11 of every row keep one counter each in a register (quade_row.h's flush_row_counters).
#include <hip/hip_runtime.h>

#include "quade_row.h"
#include "quade_clip.h"

namespace {

constexpr uint32_t CL_BLOCK = 256;
constexpr uint32_t CL_GROUPS = CL_BLOCK / ROW;      // reads per step of a workgroup
constexpr uint32_t CL_WG_READS = 1024;              // reads per workgroup
constexpr uint32_t CL_G_STEP = 4;                   // bases per lane and round of the poly-G walk
static_assert(CL_WG_READS % CL_GROUPS == 0, "whole steps");

// Window rule over q[0 .. Lc) (the caller's row holds one read): the smallest p in [0, Lc - W] whose W Phred values sum to less
// than QW = Q * W, Lc when there is none; in every lane.  SUM: wide enough for Lc * 222.
template <typename SUM, typename PTR>
__device__ __forceinline__ uint32_t window_trim(PTR q, uint32_t Lc, uint32_t W, uint32_t QW, uint32_t sub) {
    if (Lc < W) return Lc;
    const uint32_t n_p = Lc - W + 1;                     // starts
    const uint32_t T = (Lc + ROW - 1) / ROW;   // lane i: bytes [i T, (i + 1) T)
    const uint32_t lo = min(sub * T, Lc), hi = lo + min(T, Lc - lo);
    auto ph = [&](uint32_t i) {
        const uint32_t b = q[i];
        return (SUM)(b > 33 ? b - 33 : 0);
    };
    uint32_t hit = 0xFFFFFFFFu;
    const uint32_t end = min(hi, n_p);  // this lane's starts: [lo, end)
    if (W <= 2 * T) {
        // a short window: its sum at the lane's first start costs fewer reads than the two prefix sums below (W against up to 2 T)
        if (lo < end) {
            SUM S = 0;
            for (uint32_t i = lo; i < lo + W; ++i) S += ph(i);
            for (uint32_t p = lo; p < end; ++p) {
                if (S < (SUM)QW) {
                    hit = p;
                    break;
                }
                if (p + W < Lc) S += ph(p + W) - ph(p);
            }
        }
    } else {
        SUM sum = 0;
        for (uint32_t i = lo; i < hi; ++i) sum += ph(i);
        const SUM below = row_sum_below(sum);  // the prefix sum at lo
        // ... and at lo + W: from the lane whose stretch holds that byte (a lane without starts asks for Lc: every lane takes part)
        const uint32_t e = lo + min(W, Lc - lo), j = min(e / T, ROW - 1);
        SUM B = row_get(below, j);
        for (uint32_t i = j * T; i < e; ++i) B += ph(i);
        SUM A = below;
        for (uint32_t p = lo; p < end; ++p) {
            if (B - A < (SUM)QW) {
                hit = p;
                break;
            }
            A += ph(p);
            if (p + W < Lc) B += ph(p + W);
        }
    }
    hit = row_min(hit);
    return hit != 0xFFFFFFFFu ? hit : Lc;
}

// Poly-G rule over s[0 .. Lw) with minimum run P >= 6 (the bytes are folded here: a staged line is folded already): Lg in every lane
template <typename PTR>
__device__ __forceinline__ uint32_t polyg_trim(PTR s, uint32_t Lw, uint32_t P, uint32_t sub) {
    constexpr uint32_t ROUND = ROW * CL_G_STEP;
    uint32_t mm0 = 0, g = 0;  // mismatches and the largest G position of the rounds done
    for (uint32_t t0 = 0; t0 < Lw;) {
        const uint32_t n = min(Lw - t0, ROUND);
        const uint32_t a = min(sub * CL_G_STEP, n), b = min(a + CL_G_STEP, n);  // this lane: t = t0 + a + 1 .. t0 + b
        uint32_t c = 0;
        for (uint32_t i = a; i < b; ++i) c += (s[Lw - 1 - (t0 + i)] & 0xDFu) != 'G';
        uint32_t mm = mm0 + row_sum_below(c);
        uint32_t stop = 0xFFFFFFFFu, last = 0;
        for (uint32_t i = a; i < b; ++i) {
            const uint32_t t = t0 + i + 1;
            const bool is_g = (s[Lw - t] & 0xDFu) == 'G';
            mm += !is_g;
            if (mm > 5 || (t >= P && 8 * mm > t)) {
                stop = t;
                break;
            }
            if (is_g) last = t;
        }
        // stretches ascend with the lane: the lowest lane that stopped holds the first stop; the lanes above it saw nothing real
        const uint32_t w = row_min(stop != 0xFFFFFFFFu ? sub : ROW);
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

__global__ __launch_bounds__(CL_BLOCK) void clip_reads(qd_clip_dev P, qd_clip_args a, uint32_t n) {
    __shared__ uint4 slab[CL_GROUPS][2][FAST_WORDS];  // per row: the quality line, the folded sequence line (read by bytes: no dword ahead)
    __shared__ unsigned long long part[QD_CLIP_COUNTERS];
    const uint32_t r = blockIdx.y;
    if (threadIdx.x < QD_CLIP_COUNTERS) part[threadIdx.x] = 0;
    const uint32_t sub = threadIdx.x & (ROW - 1), group = threadIdx.x / ROW;
    const uint8_t* text = a.text[r];
    const qd_rec* recs = a.recs[r];
    qd_rec* out = a.out[r];
    const uint32_t F = P.front[r], Tl = P.tail[r], W = P.window, G = P.poly_g;
    uint4* sq = slab[group][0];
    uint4* ss = slab[group][1];
    uint64_t acc = 0;  // counter `sub` of this row's reads
    const uint32_t first = blockIdx.x * CL_WG_READS, last = min(n, first + CL_WG_READS);
    for (uint32_t j0 = first; j0 < last; j0 += CL_GROUPS) {  // (the same trips for every wave: a barrier inside)
        const uint32_t j = j0 + group;
        const bool valid = j < last;
        qd_rec rec{};
        if (valid) rec = recs[j];
        const uint32_t L = rec.seq_len;
        const uint32_t f = min(F, L), Lc = L - f > Tl ? L - f - Tl : 0;
        const uint32_t seq = rec.seq + f, qual = rec.qual + f;
        const Line ql = make_line(text, qual, Lc), sl = make_line(text, seq, Lc);
        const bool staged = ql.n_words <= FAST_WORDS && sl.n_words <= FAST_WORDS;
        __syncthreads();  // the row's earlier read is done with the slab
        if (staged) {
            if (W) stage_line<false>(sq, ql, sub);
            if (G) stage_line<true>(ss, sl, sub);
        }
        __syncthreads();
        uint32_t Lw = Lc, Lg;
        if (staged) {
            if (W) Lw = window_trim<int32_t>(reinterpret_cast<const uint8_t*>(sq) + ql.s, Lc, W, P.window_sum, sub);
            Lg = G ? polyg_trim(reinterpret_cast<const uint8_t*>(ss) + sl.s, Lw, G, sub) : Lw;
        } else {
            if (W) Lw = window_trim<int64_t>(text + qual, Lc, W, P.window_sum, sub);
            Lg = G ? polyg_trim(text + seq, Lw, G, sub) : Lw;
        }
        const uint32_t Lout = max(Lg, min(P.min_length, L - f));
        if (valid) {
            if (sub == 0) {
                rec.seq = seq;
                rec.qual = qual;
                rec.seq_len = Lout;
                out[j] = rec;
            }
            const uint32_t v[QD_CLIP_COUNTERS] = {1u, L, Lout, f > 0, f, Lc < L - f, L - f - Lc, Lw < Lc, Lc - Lw, Lg < Lw, Lw - Lg, Lout > Lg};
#pragma unroll
            for (uint32_t i = 0; i < QD_CLIP_COUNTERS; ++i)
                if (sub == i) acc += v[i];
        }
    }
    flush_row_counters<QD_CLIP_COUNTERS>(acc, sub, part, reinterpret_cast<unsigned long long*>(a.table) + r * QD_CLIP_COUNTERS);
}

}  // namespace

hipError_t qd_clip_launch(const qd_clip_dev& P, const qd_clip_args& a, uint32_t n, hipStream_t st) {
    if (!n) return hipSuccess;
    if (n > 0x7FFFFFFFu || P.window > QD_CLIP_MAX_WINDOW || P.poly_g > QD_CLIP_MAX_POLYG || (P.poly_g && P.poly_g < 6) ||
        (P.window && !P.window_sum))
        return hipErrorInvalidValue;
    const uint32_t grid = (n + CL_WG_READS - 1) / CL_WG_READS;
    hipLaunchKernelGGL(clip_reads, dim3(grid, 2), dim3(CL_BLOCK), 0, st, P, a, n);
    return hipGetLastError();
}
