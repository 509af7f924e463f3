// Host-only test of quade_amd/csrc/out_plan.h (the plan of a batch's output: regions -> gzip members -> 64 KiB sub-blocks -> CRC
// ranges) and quade_amd/csrc/batch_sizes.h (how many bytes every buffer of a batch needs).  No HIP call is linked.  Built and run by
// tests/test_host_batch_plan.py, plain and under AddressSanitizer + UBSan.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../quade_amd/csrc/batch_sizes.h"
#include "../../quade_amd/csrc/out_plan.h"

namespace {

int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (++g_failed < 40) printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                  \
    } while (0)

constexpr uint32_t SUB = QD_LZ_SUB;
constexpr uint32_t NONE = 0xFFFFFFFFu;

// ---- the output plan against a model that divides where the plan steps ------------------------------------------------------------------
struct Model {
    std::vector<qd_deflate_piece> pieces;
    std::vector<qd_lz_sub> subs;
    std::vector<uint32_t> first_sub;
    std::vector<outplan::FileRun> files;
};
Model model_of(const std::vector<qd_out_region>& regions, uint32_t piece_bytes, uint32_t n_samples) {
    Model m;
    for (const qd_out_region& rg : regions) {
        const uint64_t np = (rg.bytes + piece_bytes - 1) / piece_bytes;
        m.files.push_back(outplan::FileRun{rg.dest == 2 * n_samples ? 0xFFFFu : rg.dest, rg.k, (uint32_t)m.pieces.size(), (uint32_t)np, rg.bytes});
        for (uint64_t j = 0; j < np; ++j) {
            const uint64_t off = rg.at + j * piece_bytes;
            const uint64_t len = j + 1 < np ? piece_bytes : rg.bytes - j * piece_bytes;
            m.first_sub.push_back((uint32_t)m.subs.size());
            const uint64_t ns = (len + SUB - 1) / SUB;
            for (uint64_t q = 0; q < ns; ++q)
                m.subs.push_back(qd_lz_sub{off + q * SUB, (uint32_t)(q + 1 < ns ? SUB : len - q * SUB), (uint32_t)m.pieces.size()});
            m.pieces.push_back(qd_deflate_piece{off, (uint32_t)len, 0});
        }
    }
    m.first_sub.push_back((uint32_t)m.subs.size());
    return m;
}

// bytes1[d] / bytes2[d]: the text of destination d's two files (a destination without pairs: both 0 and `has[d]` false)
void check_plan(const std::vector<uint32_t>& bytes1, const std::vector<uint32_t>& bytes2, const std::vector<bool>& has, uint32_t piece_bytes) {
    const uint32_t nd = (uint32_t)bytes1.size(), S = (nd - 1) / 2;  // (nd = 2 * S + 1 when odd; any nd serves the plan)
    std::vector<uint32_t> first(nd), g1f(nd), g2f(nd);
    uint32_t t1 = 0, t2 = 0, pos = 0;
    for (uint32_t d = 0; d < nd; ++d) {
        first[d] = has[d] ? pos : NONE;
        g1f[d] = has[d] ? t1 : 0xDEADBEEFu;  // (of a destination without pairs the layout reads `first` alone)
        g2f[d] = has[d] ? t2 : 0xDEADBEEFu;
        if (has[d]) {
            t1 += bytes1[d];
            t2 += bytes2[d];
            ++pos;
        }
    }
    std::vector<int64_t> base1(nd), base2(nd);
    std::vector<qd_out_region> regions;
    const uint64_t total = qd_text_out_layout(nd, first.data(), g1f.data(), g2f.data(), t1, t2, base1.data(), base2.data(), &regions);
    const outplan::Plan pl = outplan::plan_output(regions, piece_bytes, S);
    const size_t np = pl.pieces.size(), ns = pl.subs.size();
    const uint64_t T = (uint64_t)t1 + t2;

    // the regions are the non-empty files, in buffer order, where the layout put them
    {
        size_t r = 0;
        uint64_t at = 0;
        for (int k = 0; k < 2; ++k)
            for (uint32_t d = 0; d < nd; ++d) {
                const uint32_t b = has[d] ? (k ? bytes2[d] : bytes1[d]) : 0;
                if (!b) continue;
                CHECK(r < regions.size() && regions[r].dest == d && regions[r].k == k && regions[r].at == at && regions[r].bytes == b);
                at = (at + b + 15) & ~(uint64_t)15;
                ++r;
            }
        CHECK(r == regions.size() && at == total);
    }
    // the file runs cover every piece once, in buffer order; the pieces of a region tile it exactly
    CHECK(pl.files.size() == regions.size());
    uint32_t next_piece = 0;
    for (size_t r = 0; r < regions.size() && r < pl.files.size(); ++r) {
        const outplan::FileRun& f = pl.files[r];
        const qd_out_region& rg = regions[r];
        CHECK(f.first == next_piece && f.k == rg.k && f.text_bytes == rg.bytes && f.n >= 1);
        CHECK(f.code == (rg.dest == 2 * S ? (uint32_t)QD_CODE_UNDETERMINED : rg.dest));
        uint64_t at = rg.at;
        for (uint32_t i = f.first; i < f.first + f.n && i < np; ++i) {
            CHECK(pl.pieces[i].text_off == at && pl.pieces[i].text_len >= 1 && pl.pieces[i].text_len <= piece_bytes && pl.pieces[i].crc32 == 0);
            CHECK(i + 1 == f.first + f.n || pl.pieces[i].text_len == piece_bytes);  // only a region's last piece is short
            at += pl.pieces[i].text_len;
        }
        CHECK(at == rg.at + rg.bytes);
        next_piece += f.n;
    }
    CHECK(next_piece == np);
    // first_sub is the running count, with n_pieces + 1 entries; the sub-blocks of a piece tile it exactly, in order
    CHECK(pl.first_sub.size() == np + 1 && pl.first_sub[0] == 0 && pl.first_sub[np] == ns);
    for (size_t i = 0; i < np && i + 1 < pl.first_sub.size(); ++i) {
        CHECK(pl.first_sub[i] < pl.first_sub[i + 1]);
        uint64_t at = pl.pieces[i].text_off;
        for (uint32_t k = pl.first_sub[i]; k < pl.first_sub[i + 1] && k < ns; ++k) {
            CHECK(pl.subs[k].text_off == at && pl.subs[k].piece == i);
            CHECK(pl.subs[k].text_len >= 1 && pl.subs[k].text_len <= SUB);  // no sub-block is empty or longer than QD_LZ_SUB
            CHECK(k + 1 == pl.first_sub[i + 1] || pl.subs[k].text_len == SUB);
            at += pl.subs[k].text_len;
        }
        CHECK(at == pl.pieces[i].text_off + pl.pieces[i].text_len);
    }
    // ranges[k] is subs[k]'s offset and length
    CHECK(pl.ranges.size() == ns);
    for (size_t k = 0; k < ns && k < pl.ranges.size(); ++k) CHECK(pl.ranges[k].off == pl.subs[k].text_off && pl.ranges[k].len == pl.subs[k].text_len && pl.ranges[k].pad == 0);
    // the same tables from the model
    const Model m = model_of(regions, piece_bytes, S);
    CHECK(m.pieces.size() == np && m.subs.size() == ns && m.first_sub == pl.first_sub && m.files.size() == pl.files.size());
    for (size_t i = 0; i < np && i < m.pieces.size(); ++i) CHECK(m.pieces[i].text_off == pl.pieces[i].text_off && m.pieces[i].text_len == pl.pieces[i].text_len);
    for (size_t k = 0; k < ns && k < m.subs.size(); ++k)
        CHECK(m.subs[k].text_off == pl.subs[k].text_off && m.subs[k].text_len == pl.subs[k].text_len && m.subs[k].piece == pl.subs[k].piece);
    for (size_t r = 0; r < pl.files.size() && r < m.files.size(); ++r)
        CHECK(m.files[r].code == pl.files[r].code && m.files[r].k == pl.files[r].k && m.files[r].first == pl.files[r].first && m.files[r].n == pl.files[r].n &&
              m.files[r].text_bytes == pl.files[r].text_bytes);
    // the reservation's bounds
    CHECK(np <= bsz::max_pieces((size_t)T, piece_bytes, nd));
    CHECK(np <= T / piece_bytes + 2 * (uint64_t)nd + 2);
    CHECK(ns <= bsz::max_subs((size_t)T, np));
    CHECK(ns <= T / SUB + np);
}

void test_plans() {
    std::mt19937 rng(20261021);
    for (uint32_t pb : {65536u, 131072u, 1u << 20}) {
        const uint32_t sizes[] = {1, 15, 16, 17, 65535, 65536, 65537, pb - 1, pb, pb + 1, 3 * pb + 5};
        // hand-made: nothing at all; one destination with every size in either file; every size side by side
        check_plan({0}, {0}, {false}, pb);
        check_plan({0, 0, 0}, {0, 0, 0}, {false, false, false}, pb);
        for (uint32_t a : sizes) {
            check_plan({a}, {a}, {true}, pb);
            check_plan({a}, {0}, {true}, pb);          // (a destination whose R2 takes no room)
            check_plan({0, a, 0}, {0, 1, 0}, {false, true, false}, pb);
            check_plan({0, 0, a}, {0, 0, a}, {false, false, true}, pb);  // Undetermined alone
        }
        {
            std::vector<uint32_t> b1(sizes, sizes + 11), b2(sizes, sizes + 11);
            std::reverse(b2.begin(), b2.end());
            check_plan(b1, b2, std::vector<bool>(11, true), pb);
        }
        check_plan(std::vector<uint32_t>(40, 1), std::vector<uint32_t>(40, 1), std::vector<bool>(40, true), pb);
        check_plan(std::vector<uint32_t>(40, 3 * pb + 5), std::vector<uint32_t>(40, pb + 1), std::vector<bool>(40, true), pb);
        // random: 1 to 40 destinations, some empty
        for (int trial = 0; trial < 60; ++trial) {
            const uint32_t nd = 1 + rng() % 40;
            std::vector<uint32_t> b1(nd, 0), b2(nd, 0);
            std::vector<bool> has(nd, false);
            for (uint32_t d = 0; d < nd; ++d) {
                has[d] = rng() % 3 != 0;
                if (!has[d]) continue;
                b1[d] = sizes[rng() % 11];
                b2[d] = sizes[rng() % 11];
            }
            check_plan(b1, b2, has, pb);
        }
    }
}

// ---- the cut of one piece against the loop qd_deflater_run had ------------------------------------------------------------------------------
void test_cut_piece() {
    const int64_t text_len[] = {0, 1, 65536, 65537, 200000};
    const int n_pieces = 5;
    // the model: qd_deflater_run's loop as it stood, sub-blocks and then the ranges made of them
    std::vector<qd_lz_sub> sub_h;
    std::vector<uint32_t> first_h(n_pieces + 1);
    std::vector<qd_crc_range> rg_h;
    {
        size_t js = 0, off = 0;
        size_t n_subs = 0;
        for (int i = 0; i < n_pieces; ++i) n_subs += ((size_t)text_len[i] + QD_LZ_SUB - 1) / QD_LZ_SUB;
        sub_h.resize(n_subs + 1);
        for (int i = 0; i < n_pieces; ++i) {
            first_h[i] = (uint32_t)js;
            for (int64_t a = 0; a < text_len[i]; a += QD_LZ_SUB)
                sub_h[js++] = qd_lz_sub{(uint64_t)(off + (size_t)a), (uint32_t)std::min<int64_t>(QD_LZ_SUB, text_len[i] - a), (uint32_t)i};
            off += ((size_t)text_len[i] + 15) & ~(size_t)15;
        }
        first_h[n_pieces] = (uint32_t)js;
        sub_h.resize(js);
        CHECK(js == n_subs);
        for (size_t k = 0; k < js; ++k) rg_h.push_back(qd_crc_range{sub_h[k].text_off, sub_h[k].text_len, 0});
    }
    std::vector<qd_lz_sub> subs;
    std::vector<qd_crc_range> ranges;
    std::vector<uint32_t> first;
    size_t off = 0, counted = 0;
    for (int i = 0; i < n_pieces; ++i) {
        first.push_back((uint32_t)subs.size());
        counted += outplan::subs_of((uint64_t)text_len[i]);
        outplan::cut_piece(off, (uint32_t)text_len[i], (uint32_t)i, [&](const qd_lz_sub& s, const qd_crc_range& r) {
            subs.push_back(s);
            ranges.push_back(r);
        });
        off += ((size_t)text_len[i] + 15) & ~(size_t)15;
    }
    first.push_back((uint32_t)subs.size());
    CHECK(counted == subs.size() && subs.size() == sub_h.size() && subs.size() == 1 + 1 + 2 + 4 && first == first_h && ranges.size() == rg_h.size());
    for (size_t k = 0; k < subs.size() && k < sub_h.size(); ++k) {
        CHECK(subs[k].text_off == sub_h[k].text_off && subs[k].text_len == sub_h[k].text_len && subs[k].piece == sub_h[k].piece);
        CHECK(ranges[k].off == rg_h[k].off && ranges[k].len == rg_h[k].len && ranges[k].pad == rg_h[k].pad);
    }
}

// ---- sizes --------------------------------------------------------------------------------------------------------------------------
qd_layout layout(int streams) {
    qd_layout L;
    memset(&L, 0, sizeof L);
    L.n_streams = streams;
    L.seq_stride[0] = L.qual_stride[0] = streams == 2 ? 16 : 8;
    if (streams == 2) {
        L.seq_stride[1] = L.qual_stride[1] = 8;
        L.mol_width = 12;
    }
    return L;
}
bsz::StagesOn all_stages() {
    bsz::StagesOn on;
    for (bool& b : on.recs_out) b = true;
    on.inserts = on.drop = true;
    return on;
}
template <class Z>
bool every_field_at_most(const Z& a, const Z& b) {  // (the size structs hold nothing but counts of one width)
    static_assert(sizeof(Z) % sizeof(size_t) == 0, "counts alone");
    size_t x[sizeof(Z) / sizeof(size_t)], y[sizeof(Z) / sizeof(size_t)];
    memcpy(x, &a, sizeof(Z));
    memcpy(y, &b, sizeof(Z));
    for (size_t i = 0; i < sizeof(Z) / sizeof(size_t); ++i)
        if (x[i] > y[i]) return false;
    return true;
}

void test_monotone() {
    static_assert(sizeof(int64_t) == sizeof(size_t), "OutSizes' strides compare as counts");
    const size_t ns[] = {0, 1, 2, 63, 64, 1023, 1024, 1025, 2047, 4095, 4096, 4097, 100000, 2000000, 2000001, 16000000};
    for (int streams : {1, 2})
        for (size_t a : ns)
            for (size_t b : ns) {
                if (a > b) continue;
                for (const bsz::StagesOn& on : {bsz::StagesOn(), all_stages()}) {
                    CHECK(every_field_at_most(bsz::pair_sizes(layout(streams), a, 7, on), bsz::pair_sizes(layout(streams), b, 7, on)));
                    CHECK(every_field_at_most(bsz::pair_sizes(layout(streams), a, 7, on), bsz::pair_sizes(layout(streams), a, 2001, on)));
                }
                CHECK(every_field_at_most(bsz::pair_sizes(layout(streams), a, 7, bsz::StagesOn()), bsz::pair_sizes(layout(streams), a, 7, all_stages())));
                CHECK(every_field_at_most(bsz::scan_sizes(a, 4096), bsz::scan_sizes(b, 4096)));
                CHECK(every_field_at_most(bsz::scan_sizes(1 << 20, a), bsz::scan_sizes(1 << 20, b)));
            }
    const size_t vs[] = {0, 1, 3, 4, 5, 2047 * 4, 2048 * 4, 2048 * 4 + 1, 10000, 60000};
    const uint32_t pbs[] = {65536, 131072, 262144, 524288, 1u << 20};
    for (size_t a : vs)
        for (size_t b : vs) {
            if (a > b) continue;
            for (uint32_t pb : pbs) {
                CHECK(every_field_at_most(bsz::out_sizes(a, 100, 400, pb), bsz::out_sizes(b, 100, 400, pb)));
                CHECK(every_field_at_most(bsz::out_sizes(1000, a, 400, pb), bsz::out_sizes(1000, b, 400, pb)));
                CHECK(every_field_at_most(bsz::out_sizes(1000, 100, a, pb), bsz::out_sizes(1000, 100, b, pb)));
            }
            for (uint32_t p1 : pbs)
                for (uint32_t p2 : pbs)
                    if (p1 <= p2) CHECK(every_field_at_most(bsz::out_sizes(a, a, b, p1), bsz::out_sizes(a, a, b, p2)));
        }
}

// each pair-sized buffer: the larger of the two formulas the code had, one in the reservation (r) and one in the batch (b); a buffer
// the reservation did not know has the batch's alone
void test_pinned() {
    const size_t ns[] = {0, 1, 1023, 1024, 1025, 4096, 2000000};
    const size_t nd = 2 * 3 + 1;
    for (int streams : {1, 2})
        for (size_t n : ns) {
            const qd_layout L = layout(streams);
            const bsz::PairSizes z = bsz::pair_sizes(L, n, nd, all_stages());
            const bsz::PairSizes off = bsz::pair_sizes(L, n, nd, bsz::StagesOn());
            auto larger = [](size_t r, size_t b) { return std::max(r, b); };
            for (int k = 0; k < 2; ++k) {
                const bool there = k < L.n_streams;
                CHECK(z.rows_seq[k] == (there ? larger(n * L.seq_stride[k] + 64, (size_t)n * L.seq_stride[k] + 64) : 0));
                CHECK(z.rows_qual[k] == (there ? larger(n * L.qual_stride[k] + 64, (size_t)n * L.qual_stride[k] + 64) : 0));
                CHECK(z.rows_len[k] == (there ? larger(n + 64, (size_t)n + 64) : 0));
            }
            CHECK(z.halves == larger(n * 2 + 64, (size_t)n * 2 + 64));                      // codes, dest, sdest
            CHECK(z.mol == (L.mol_width ? larger(n * L.mol_width + 64, (size_t)n * L.mol_width + 64) : 0));
            CHECK(z.short_idx == larger((n / 2 + 64) * 4, (size_t)((uint32_t)n / 2 + 64) * 4));
            const size_t H = 256 * ((n + 1023) / 1024);
            CHECK(z.hist == larger((H + H / 4096 + 8) * 4, (H + H / 4096 + 8) * 4));
            CHECK(z.words == larger((n + 1) * 4 + 64, (size_t)n * 4 + 64));                 // len1, len2, tmp, perm
            CHECK(z.words == larger((n + 1) * 4 + 64, ((size_t)n + 1) * 4 + 64));           // g1, g2
            CHECK(z.scan_tiles == larger((n / 4096 + 4) * 4, ((size_t)n / 4096 + 4) * 4));
            CHECK(z.dest_words == (size_t)nd * 4);                                          // first, g1_first, g2_first
            CHECK(z.dest_longs == (size_t)nd * 8);                                          // base1, base2
            CHECK(z.h_first == (size_t)nd * 12 + 16);
            for (int s = 0; s < 4; ++s) CHECK(z.recs_out[s] == (size_t)n * 24 + 64 && off.recs_out[s] == 0);
            CHECK(z.inserts == (size_t)n * 8 + 64 && off.inserts == 0);
            CHECK(z.drop == (size_t)n + 64 && off.drop == 0);
        }
    {  // ... and as plain numbers, worked out by hand from the larger formula: 1025 and 2 000 000 pairs, two index streams, every stage on
        const bsz::PairSizes z = bsz::pair_sizes(layout(2), 1025, 7, all_stages());
        CHECK(z.rows_seq[0] == 16464 && z.rows_qual[0] == 16464 && z.rows_seq[1] == 8264 && z.rows_qual[1] == 8264 && z.rows_len[0] == 1089 && z.rows_len[1] == 1089);
        CHECK(z.mol == 12364 && z.halves == 2114 && z.words == 4168 && z.short_idx == 2304 && z.hist == 2080 && z.scan_tiles == 16);
        CHECK(z.dest_words == 28 && z.dest_longs == 56 && z.h_first == 100 && z.recs_out[0] == 24664 && z.recs_out[3] == 24664 && z.inserts == 8264 && z.drop == 1089);
        const bsz::PairSizes y = bsz::pair_sizes(layout(1), 2000000, 7, bsz::StagesOn());
        CHECK(y.rows_seq[0] == 16000064 && y.rows_seq[1] == 0 && y.rows_len[0] == 2000064 && y.mol == 0 && y.halves == 4000064 && y.words == 8000068);
        CHECK(y.short_idx == 4000256 && y.hist == 2001416 && y.scan_tiles == 1968 && bsz::short_cap(2000000) == 1000064);
    }
    // the scan's tables: scan_window's formulas for a window of len bytes, the reservation's for `text` bytes and `lines` lines
    for (size_t len : {(size_t)0, (size_t)1, (size_t)16383, (size_t)16384, (size_t)1000000, (size_t)1 << 30}) {
        const size_t line_cap = 65536 + len / 64 * 4;
        const bsz::ScanSizes z = bsz::scan_sizes(len, line_cap);
        const uint32_t n_tiles = (uint32_t)len / 16384u + 1;
        CHECK(z.tiles == (size_t)(n_tiles + 2) * 4 && z.tiles == (len / 16384u + 3) * 4);
        CHECK(z.lines == line_cap * 4 + 64);
        CHECK(z.rec_tile == (line_cap / 4 / 1024 + 4) * 4);
        CHECK(z.recs == (line_cap / 4 + 1) * 24);
    }
    // the output side: reserve_output's list and process_batch's
    for (uint32_t pb : {65536u, 1u << 20}) {
        const size_t T = 123456789, np = 321, ns = 2345;
        const bsz::OutSizes z = bsz::out_sizes(T, np, ns, pb);
        const size_t out_stride = (size_t)bsz::huffman_member_bound(pb), sub_stride = (size_t)bsz::huffman_member_bound(65536);
        CHECK(z.out_stride == (int64_t)out_stride && z.sub_stride == (int64_t)sub_stride);
        CHECK(z.text == T + 64 && z.pieces == np * 16 && z.members == np * out_stride && z.packed == np * out_stride);
        CHECK(z.member_len == np * 4 && z.member_off == (np + 1) * 8);
        CHECK(z.subs == (ns + 1) * 16 && z.ranges == (ns + 1) * 16 && z.crc == (ns + 1) * 4 && z.first_sub == (np + 1) * 4);
        CHECK(z.tokens == (size_t)std::max<uint32_t>(2048, ((uint32_t)ns + 3) / 4) * 65536 * 4 && z.sub_out == ns * sub_stride && z.sub_bytes == ns * 4);
    }
    CHECK(bsz::lz_slice_subs(0) == 2048 && bsz::lz_slice_subs(8192) == 2048 && bsz::lz_slice_subs(8193) == 2049 && bsz::lz_slice_subs(50000) == 12500);
}

void test_rules() {
    // the top-up target at run_chunk's four call sites, as they were written, the cap included
    const size_t WM = (size_t)1 << 30;
    const uint32_t Bs[] = {1024, 2000000, 0x7FFFFFFF};
    const double avgs[] = {16.0, 95.5, 256.0, 331.25, 4000.0};
    for (uint32_t B : Bs)
        for (double avg : avgs) {
            // a chunk's first round
            CHECK(bsz::want_text(0, B, avg, WM) == std::min<size_t>((size_t)((double)B * avg * 1.03) + 4096, WM * 3 / 4));
            for (uint32_t len : {0u, 1u, 70000u, 700000000u, 0xF0000000u}) {
                // behind the kept records a shared chunk drops
                for (uint64_t skip_kept : {(uint64_t)0, (uint64_t)5, (uint64_t)3000000000ull})
                    CHECK(bsz::want_text(len, skip_kept + B, avg, WM) == std::min<size_t>((size_t)len + (size_t)((double)(skip_kept + B) * avg * 1.03) + 4096, WM * 3 / 4));
                for (uint32_t kept : {0u, 1u, 1000u, B - 1, B, B + 7}) {
                    if (kept < B) {  // a stream short of records
                        const size_t more = (size_t)((double)(B - kept) * avg * 1.03) + 4096;
                        CHECK(bsz::want_text(len, B - kept, avg, WM) == std::min<size_t>(std::max<size_t>((size_t)len + more, (size_t)len + 1), WM * 3 / 4));
                    }
                    // behind a batch: what the carry left
                    CHECK(bsz::want_text(len, B > kept ? B - kept : 0, avg, WM) ==
                          std::min<size_t>((size_t)len + (size_t)((double)(B > kept ? B - kept : 0) * avg * 1.03) + 4096, WM * 3 / 4));
                }
            }
        }
    CHECK(bsz::want_text(0, 2000000, 331.25, WM) == 682379096 && bsz::want_text(0, 0x7FFFFFFF, 4000.0, WM) == 805306368 && bsz::want_text(100, 0, 1.0, WM) == 4196);
    // bytes per record: the learned size, or the caller's default
    CHECK(bsz::record_bytes(0, bsz::RECORD_INSERT) == 400.0 && bsz::record_bytes(0, bsz::RECORD_INDEX) == 64.0 && bsz::record_bytes(0, bsz::RECORD_TOP_UP) == 256.0);
    CHECK(bsz::record_bytes(-1, 7.0) == 7.0 && bsz::record_bytes(16.0, 400.0) == 16.0 && bsz::record_bytes(331.25, 64.0) == 331.25);
    // the pairs the reservation is made for
    for (uint32_t B : Bs)
        for (int64_t r1 : {(int64_t)0, (int64_t)1000, (int64_t)50000000, (int64_t)1 << 40})
            for (bool comp : {false, true})
                for (double avg : {0.0, 16.0, 331.25}) {
                    const double avg1 = avg > 0 ? avg : 400.0;
                    CHECK(bsz::most_pairs(B, r1, comp, avg) == (uint32_t)std::min<double>((double)B, (double)r1 * (comp ? 8.0 : 1.0) / avg1 + 1024.0));
                }
    CHECK(bsz::most_pairs(2000000, 1000, true, 0) == 1044 && bsz::most_pairs(2000000, (int64_t)1 << 40, false, 100.0) == 2000000);
    // text per member: halves down to 64 KiB and no further
    const int64_t slots = (int64_t)12 << 30;
    CHECK(bsz::piece_bytes_for(slots, 1000000000, 7) == 1u << 20);
    CHECK(bsz::piece_bytes_for(slots, 1000000000, 4000) == 1u << 20);
    CHECK(bsz::piece_bytes_for(slots, 1000000000, 6000) == 1u << 19);
    CHECK(bsz::piece_bytes_for(slots, 1000000000, 100000) == 65536);
    CHECK(bsz::piece_bytes_for(slots, 1000000000, 100000000) == 65536);
    CHECK(bsz::piece_bytes_for(0, 0, 0) == 65536 && bsz::piece_bytes_for(1, 1, 1) == 65536);
    for (uint64_t nd : {(uint64_t)1, (uint64_t)769, (uint64_t)5000, (uint64_t)20001, (uint64_t)77777, (uint64_t)1000000}) {
        uint32_t pb = 1u << 20;  // (the loop as it stood)
        const uint64_t text_bytes = 1300000000;
        while (pb > 65536 && (text_bytes / pb + 2 * nd + 2) * (uint64_t)bsz::huffman_member_bound(pb) > (uint64_t)slots) pb >>= 1;
        CHECK(bsz::piece_bytes_for(slots, text_bytes, nd) == pb && pb >= 65536);
    }
    // a member's slot
    CHECK(bsz::huffman_member_bound(0) == 1024 && bsz::huffman_member_bound(1) == 1028 && bsz::huffman_member_bound(65536) == 75776);
    CHECK(bsz::huffman_member_bound(1 << 20) == 1197056 && bsz::huffman_member_bound(-1) == -1);
    for (int64_t t : {(int64_t)0, (int64_t)1, (int64_t)65536, (int64_t)1 << 20, (int64_t)-1})
        CHECK(bsz::huffman_member_bound(t) == (t < 0 ? -1 : ((t * 9 + 7) / 8 + t / 64 + 1024 + 3) & ~(int64_t)3));
}

}  // namespace

int main() {
    test_plans();
    test_cut_piece();
    test_monotone();
    test_pinned();
    test_rules();
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("ok\n");
    return 0;
}
