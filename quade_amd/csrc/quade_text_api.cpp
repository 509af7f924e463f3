// Host-buffer entry points over the device text stages (quade_text.hip): what qd_pipe_run chains on the device, one stage
// at a time, for bindings that hold text in host memory and for the tests (each stage on its own).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/quade_hip.h"
#include "quade_buf.h"
#include "quade_text.h"

namespace {
struct Scratch : qbuf::Buf<qbuf::DriverDev> {  // a scratch allocation freed at scope exit; never empty: a kernel gets a real address for n == 0 too
    hipError_t alloc(size_t n) { return Buf::alloc(n ? n : 16); }
};
#define TCHK(call)                            \
    do {                                      \
        if ((call) != hipSuccess) return QD_ERR_HIP; \
    } while (0)
}  // namespace

extern "C" {

int64_t qd_dev_fastq_scan(int device_id, const uint8_t* text, int64_t text_len, int32_t at_eof, int32_t want_names, int32_t need,
                          int64_t line_cap, uint32_t* recs_out, int64_t recs_cap, uint32_t* result_out) {
    if (!text || text_len < 0 || text_len > (int64_t)1 << 30 || line_cap < 4 || !result_out) return QD_ERR_INVALID;
    TCHK(hipSetDevice(device_id));
    const uint32_t len = (uint32_t)text_len, n_tiles = len / QD_TEXT_TILE + 1;
    line_cap &= ~(int64_t)3;
    Scratch d_text, tc, tb, lines, rt, recs, res;
    TCHK(d_text.alloc((size_t)len + 2 * QD_TEXT_TILE));
    TCHK(tc.alloc((size_t)(n_tiles + 2) * 4));
    TCHK(tb.alloc((size_t)(n_tiles + 2) * 4));
    TCHK(lines.alloc((size_t)line_cap * 4 + 64));
    TCHK(rt.alloc(((size_t)line_cap / 4 / 1024 + 4) * 4));
    TCHK(recs.alloc(((size_t)line_cap / 4 + 1) * sizeof(qd_rec)));
    TCHK(res.alloc(sizeof(qd_scan_result)));
    TCHK(hipMemset(res.p, 0xFF, sizeof(qd_scan_result)));
    if (len) TCHK(hipMemcpy(d_text.p, text, len, hipMemcpyHostToDevice));
    qd_scan_scratch sc;
    sc.tile_counts = tc.as<uint32_t>();
    sc.tile_base = tb.as<uint32_t>();
    sc.lines = lines.as<uint32_t>();
    sc.line_cap = (uint32_t)line_cap;
    sc.rec_tile = rt.as<uint32_t>();
    sc.recs = recs.as<qd_rec>();
    TCHK(qd_text_scan(d_text.as<uint8_t>(), len, at_eof, want_names, (uint32_t)need, sc, res.as<qd_scan_result>(), nullptr));
    TCHK(hipDeviceSynchronize());
    qd_scan_result r;
    TCHK(hipMemcpy(&r, res.p, sizeof r, hipMemcpyDeviceToHost));
    memcpy(result_out, &r, sizeof r);
    if (r.overflow) return 0;
    const int64_t n = std::min<int64_t>(r.n_kept, recs_cap);
    if (n && recs_out) TCHK(hipMemcpy(recs_out, recs.p, (size_t)n * sizeof(qd_rec), hipMemcpyDeviceToHost));
    return r.n_kept;
}

int qd_dev_crc32(int device_id, const uint8_t* data, int64_t n, int64_t range_bytes, uint32_t* crc_out) {
    if ((!data && n) || n < 0 || range_bytes < 1 || range_bytes > 65536 || !crc_out) return QD_ERR_INVALID;
    TCHK(hipSetDevice(device_id));
    std::vector<qd_crc_range> ranges;
    for (int64_t a = 0; a < n; a += range_bytes) ranges.push_back(qd_crc_range{(uint64_t)a + 3, (uint32_t)std::min<int64_t>(range_bytes, n - a), 0});
    const uint32_t first[2] = {0, (uint32_t)ranges.size()};
    Scratch d, dr, dc, df, out;
    TCHK(d.alloc((size_t)n + 16));
    TCHK(dr.alloc(ranges.size() * sizeof(qd_crc_range)));
    TCHK(dc.alloc(ranges.size() * 4));
    TCHK(df.alloc(8));
    TCHK(out.alloc(4));
    if (n) TCHK(hipMemcpy(d.as<uint8_t>() + 3, data, (size_t)n, hipMemcpyHostToDevice));  // (a misaligned start on purpose)
    if (!ranges.empty()) TCHK(hipMemcpy(dr.p, ranges.data(), ranges.size() * sizeof(qd_crc_range), hipMemcpyHostToDevice));
    TCHK(hipMemcpy(df.p, first, 8, hipMemcpyHostToDevice));
    TCHK(qd_text_crc32(d.as<uint8_t>(), dr.as<qd_crc_range>(), (uint32_t)ranges.size(), dc.as<uint32_t>(), nullptr));
    TCHK(qd_text_crc32_combine(dr.as<qd_crc_range>(), dc.as<uint32_t>(), df.as<uint32_t>(), 1, out.as<uint32_t>(), 1, nullptr));
    TCHK(hipDeviceSynchronize());
    TCHK(hipMemcpy(crc_out, out.p, 4, hipMemcpyDeviceToHost));
    return QD_OK;
}

int qd_dev_sort_by_dest(int device_id, const uint16_t* dest, int64_t n, int32_t n_dest, const uint32_t* len, uint32_t* perm_out, uint32_t* offsets_out) {
    if (!dest || n < 1 || n > 0x7FFFFFFF || n_dest < 1 || n_dest > 65536 || !perm_out) return QD_ERR_INVALID;
    TCHK(hipSetDevice(device_id));
    const size_t H = 256 * (((size_t)n + 1023) / 1024);
    Scratch d, hist, tmp, perm, dl, tiles, g;
    TCHK(d.alloc((size_t)n * 2));
    TCHK(hist.alloc((H + H / 4096 + 8) * 4));
    TCHK(tmp.alloc((size_t)n * 4));
    TCHK(perm.alloc((size_t)n * 4));
    TCHK(dl.alloc((size_t)n * 4));
    TCHK(tiles.alloc(((size_t)n / 4096 + 4) * 4));
    TCHK(g.alloc(((size_t)n + 1) * 4));
    TCHK(hipMemcpy(d.p, dest, (size_t)n * 2, hipMemcpyHostToDevice));
    TCHK(qd_text_sort_by_dest(d.as<uint16_t>(), (uint32_t)n, (uint32_t)n_dest, hist.as<uint32_t>(), tmp.as<uint32_t>(), perm.as<uint32_t>(), nullptr));
    if (len && offsets_out) {
        TCHK(hipMemcpy(dl.p, len, (size_t)n * 4, hipMemcpyHostToDevice));
        TCHK(qd_text_scan_gathered(dl.as<uint32_t>(), perm.as<uint32_t>(), (uint32_t)n, tiles.as<uint32_t>(), g.as<uint32_t>(), nullptr, nullptr, nullptr));
    }
    TCHK(hipDeviceSynchronize());
    TCHK(hipMemcpy(perm_out, perm.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (len && offsets_out) TCHK(hipMemcpy(offsets_out, g.p, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost));
    return QD_OK;
}

int qd_dev_pack_rows(int device_id, const qd_layout* layout, const uint8_t* const text[2], const int64_t text_len[2],
                     const uint32_t* const recs[2], int64_t n, int64_t short_cap, uint8_t* const seq_rows[2], uint8_t* const qual_rows[2],
                     uint8_t* const len_rows[2], uint32_t* short_idx, int64_t short_room, uint32_t* n_short) {
    if (!layout || !text || !text_len || !recs || !seq_rows || !qual_rows || !len_rows || !short_idx || !n_short) return QD_ERR_INVALID;
    if (n < 1 || n > 0x7FFFFFFF || short_cap < 0 || short_room < short_cap || short_room > 0x7FFFFFFF) return QD_ERR_INVALID;
    const qd_layout& L = *layout;
    if (L.n_streams < 1 || L.n_streams > 2) return QD_ERR_INVALID;
    for (int k = 0; k < L.n_streams; ++k) {
        if (!recs[k] || !seq_rows[k] || !qual_rows[k] || !len_rows[k] || text_len[k] < 0 || text_len[k] > (int64_t)1 << 30 || (!text[k] && text_len[k]))
            return QD_ERR_INVALID;
        for (const int32_t stride : {L.seq_stride[k], L.qual_stride[k]})
            if (stride < 2 || (stride & 1) || stride > QD_MAX_WINDOW + 2) return QD_ERR_INVALID;
        if (L.seq_off[k] < 0 || L.qual_off[k] < 0 || L.seq_width[k] < 0 || L.qual_width[k] < 0 || L.seq_width[k] > L.seq_stride[k] ||
            L.qual_width[k] > L.qual_stride[k])
            return QD_ERR_INVALID;
        // every range is checked here: a bad table cannot become a bad address
        for (int64_t j = 0; j < n; ++j) {
            const qd_rec* q = reinterpret_cast<const qd_rec*>(recs[k]) + j;
            if ((int64_t)q->seq + q->seq_len > text_len[k] || (int64_t)q->qual + q->seq_len > text_len[k]) return QD_ERR_INVALID;
        }
    }
    TCHK(hipSetDevice(device_id));
    Scratch d_text[2], d_recs[2], d_seq[2], d_qual[2], d_len[2], d_short, d_n;
    qd_pack_args pa{};
    for (int k = 0; k < L.n_streams; ++k) {
        TCHK(d_text[k].alloc((size_t)text_len[k] + 64));
        TCHK(d_recs[k].alloc((size_t)n * sizeof(qd_rec)));
        TCHK(d_seq[k].alloc((size_t)n * L.seq_stride[k]));
        TCHK(d_qual[k].alloc((size_t)n * L.qual_stride[k]));
        TCHK(d_len[k].alloc((size_t)n));
        if (text_len[k]) TCHK(hipMemcpy(d_text[k].p, text[k], (size_t)text_len[k], hipMemcpyHostToDevice));
        TCHK(hipMemcpy(d_recs[k].p, recs[k], (size_t)n * sizeof(qd_rec), hipMemcpyHostToDevice));
        pa.text[k] = d_text[k].as<uint8_t>();
        pa.recs[k] = d_recs[k].as<qd_rec>();
        pa.seq[k] = d_seq[k].as<uint8_t>();
        pa.qual[k] = d_qual[k].as<uint8_t>();
        pa.len[k] = d_len[k].as<uint8_t>();
    }
    TCHK(d_short.alloc((size_t)short_room * 4));
    TCHK(d_n.alloc(4));
    if (short_room) TCHK(hipMemset(d_short.p, 0xFF, (size_t)short_room * 4));  // entries the kernel does not write stay 0xFFFFFFFF
    TCHK(hipMemset(d_n.p, 0, 4));
    pa.short_idx = d_short.as<uint32_t>();
    pa.n_short = d_n.as<uint32_t>();
    pa.short_cap = (uint32_t)short_cap;
    TCHK(qd_text_pack_rows(L, (uint32_t)n, pa, nullptr));
    TCHK(hipDeviceSynchronize());
    for (int k = 0; k < L.n_streams; ++k) {
        TCHK(hipMemcpy(seq_rows[k], d_seq[k].p, (size_t)n * L.seq_stride[k], hipMemcpyDeviceToHost));
        TCHK(hipMemcpy(qual_rows[k], d_qual[k].p, (size_t)n * L.qual_stride[k], hipMemcpyDeviceToHost));
        TCHK(hipMemcpy(len_rows[k], d_len[k].p, (size_t)n, hipMemcpyDeviceToHost));
    }
    if (short_room) TCHK(hipMemcpy(short_idx, d_short.p, (size_t)short_room * 4, hipMemcpyDeviceToHost));
    TCHK(hipMemcpy(n_short, d_n.p, 4, hipMemcpyDeviceToHost));
    return QD_OK;
}

int qd_dev_route_format(int device_id, const qd_plan* plan, int32_t n_samples, int32_t write_pass, int32_t write_fail, int32_t write_undet,
                        const uint8_t* const text[4], const int64_t text_len[4], const uint32_t* const recs[4], const uint16_t* codes,
                        const uint8_t* drop, int64_t n, int32_t shift, uint16_t* dest, uint32_t* len1, uint32_t* len2, uint32_t* perm,
                        uint16_t* sdest, uint32_t* g1, uint32_t* g2, uint32_t* first, uint32_t* g1_first, uint32_t* g2_first, int64_t* base1,
                        int64_t* base2, uint8_t* out, int64_t out_cap, int64_t* out_used) {
    if (!plan || !text || !text_len || !recs || !codes || !dest || !len1 || !len2 || !perm || !sdest || !g1 || !g2 || !first || !g1_first ||
        !g2_first || !base1 || !base2 || (!out && out_cap) || !out_used)
        return QD_ERR_INVALID;
    if (n < 1 || n > 0x7FFFFFFF || n_samples < 1 || n_samples > QD_MAX_SAMPLES || shift < 0 || shift > 15 || out_cap < 0) return QD_ERR_INVALID;
    qd_layout lay;
    const int lrc = qd_plan_layout(plan, &lay);  // (the pipeline runs no plan that this refuses)
    if (lrc != QD_OK) return lrc;
    const int ns = 2 + lay.n_streams;
    // every range is checked here: a bad table cannot become a bad address; and the output's size stays below 2^32
    uint64_t bound = 0;
    for (int s = 0; s < ns; ++s) {
        if (!recs[s] || text_len[s] < 0 || text_len[s] > (int64_t)1 << 30 || (!text[s] && text_len[s])) return QD_ERR_INVALID;
        for (int64_t j = 0; j < n; ++j) {
            const qd_rec* q = reinterpret_cast<const qd_rec*>(recs[s]) + j;
            if ((int64_t)q->seq + q->seq_len > text_len[s]) return QD_ERR_INVALID;
            if (s < 2) {
                if ((int64_t)q->qual + q->seq_len > text_len[s] || (int64_t)q->name_off + q->name_len > text_len[s]) return QD_ERR_INVALID;
                bound += (uint64_t)q->name_len + 2ull * q->seq_len + 8 + 4 * 255;
            }
        }
    }
    if (bound >= 0xFFFFFFFFull) return QD_ERR_INVALID;
    TCHK(hipSetDevice(device_id));
    const uint32_t N = (uint32_t)n, S = (uint32_t)n_samples, nd = 2 * S + 1;
    const size_t H = 256 * (((size_t)n + 1023) / 1024);
    Scratch d_text[4], d_recs[4], d_codes, d_drop, d_dest, d_len1, d_len2, hist, tmp, d_perm, d_sdest, d_g1, d_g2, tiles, d_first, d_g1f, d_g2f, d_b1,
        d_b2, d_out;
    const uint8_t* t[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int s = 0; s < ns; ++s) {  // byte o of a text lies at device address o + shift (mod 16)
        TCHK(d_text[s].alloc((size_t)text_len[s] + 64));
        TCHK(d_recs[s].alloc((size_t)n * sizeof(qd_rec)));
        if (text_len[s]) TCHK(hipMemcpy(d_text[s].as<uint8_t>() + shift, text[s], (size_t)text_len[s], hipMemcpyHostToDevice));
        TCHK(hipMemcpy(d_recs[s].p, recs[s], (size_t)n * sizeof(qd_rec), hipMemcpyHostToDevice));
        t[s] = d_text[s].as<uint8_t>() + shift;
    }
    TCHK(d_codes.alloc((size_t)n * 2));
    TCHK(hipMemcpy(d_codes.p, codes, (size_t)n * 2, hipMemcpyHostToDevice));
    if (drop) {
        TCHK(d_drop.alloc((size_t)n));
        TCHK(hipMemcpy(d_drop.p, drop, (size_t)n, hipMemcpyHostToDevice));
    }
    TCHK(d_dest.alloc((size_t)n * 2));
    TCHK(d_sdest.alloc((size_t)n * 2));
    for (Scratch* b : {&d_len1, &d_len2, &tmp, &d_perm, &d_g1, &d_g2}) TCHK(b->alloc(((size_t)n + 1) * 4));
    TCHK(hist.alloc((H + H / 4096 + 8) * 4));
    TCHK(tiles.alloc(((size_t)n / 4096 + 4) * 4));
    for (Scratch* b : {&d_first, &d_g1f, &d_g2f}) {
        TCHK(b->alloc((size_t)nd * 4));
        TCHK(hipMemset(b->p, 0xFF, (size_t)nd * 4));  // an entry of g1_first / g2_first that no kernel writes stays 0xFFFFFFFF
    }
    TCHK(d_b1.alloc((size_t)nd * 8));
    TCHK(d_b2.alloc((size_t)nd * 8));
    TCHK(d_out.alloc((size_t)out_cap));
    if (out_cap) TCHK(hipMemset(d_out.p, QD_DEV_GUARD_BYTE, (size_t)out_cap));
    // the chain of process_batch (quade_pipe.cpp), steps 3 to 6
    qd_route_args ra{};
    ra.codes = d_codes.as<uint16_t>();
    ra.drop = drop ? d_drop.as<uint8_t>() : nullptr;
    ra.r1 = d_recs[0].as<qd_rec>();
    ra.r2 = d_recs[1].as<qd_rec>();
    for (int k = 0; k < lay.n_streams; ++k) ra.idx[k] = d_recs[2 + k].as<qd_rec>();
    ra.dest = d_dest.as<uint16_t>();
    ra.len1 = d_len1.as<uint32_t>();
    ra.len2 = d_len2.as<uint32_t>();
    TCHK(qd_text_dest_lens(*plan, S, write_pass, write_fail, write_undet, N, ra, nullptr));
    TCHK(qd_text_sort_by_dest(ra.dest, N, nd, hist.as<uint32_t>(), tmp.as<uint32_t>(), d_perm.as<uint32_t>(), nullptr));
    TCHK(qd_text_scan_gathered(ra.len1, d_perm.as<uint32_t>(), N, tiles.as<uint32_t>(), d_g1.as<uint32_t>(), ra.dest, d_sdest.as<uint16_t>(), nullptr));
    TCHK(qd_text_scan_gathered(ra.len2, d_perm.as<uint32_t>(), N, tiles.as<uint32_t>(), d_g2.as<uint32_t>(), nullptr, nullptr, nullptr));
    TCHK(qd_text_dest_bounds(d_sdest.as<uint16_t>(), d_g1.as<uint32_t>(), d_g2.as<uint32_t>(), N, nd, d_first.as<uint32_t>(), d_g1f.as<uint32_t>(),
                             d_g2f.as<uint32_t>(), nullptr));
    TCHK(hipDeviceSynchronize());
    TCHK(hipMemcpy(dest, d_dest.p, (size_t)n * 2, hipMemcpyDeviceToHost));
    TCHK(hipMemcpy(len1, d_len1.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    TCHK(hipMemcpy(len2, d_len2.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    TCHK(hipMemcpy(perm, d_perm.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    TCHK(hipMemcpy(sdest, d_sdest.p, (size_t)n * 2, hipMemcpyDeviceToHost));
    TCHK(hipMemcpy(g1, d_g1.p, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost));
    TCHK(hipMemcpy(g2, d_g2.p, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost));
    TCHK(hipMemcpy(first, d_first.p, (size_t)nd * 4, hipMemcpyDeviceToHost));
    TCHK(hipMemcpy(g1_first, d_g1f.p, (size_t)nd * 4, hipMemcpyDeviceToHost));
    TCHK(hipMemcpy(g2_first, d_g2f.p, (size_t)nd * 4, hipMemcpyDeviceToHost));
    std::vector<qd_out_region> regions;
    const uint64_t at = qd_text_out_layout(nd, first, g1_first, g2_first, g1[n], g2[n], base1, base2, &regions);
    *out_used = (int64_t)at;
    if (at > (uint64_t)out_cap) return QD_ERR_INVALID;  // (*out_used says how much room the text needs)
    if (regions.empty()) {  // every write flag off or every pair dropped: the pipeline launches nothing more for such a batch
        if (out_cap) TCHK(hipMemcpy(out, d_out.p, (size_t)out_cap, hipMemcpyDeviceToHost));
        return QD_OK;
    }
    TCHK(hipMemcpy(d_b1.p, base1, (size_t)nd * 8, hipMemcpyHostToDevice));
    TCHK(hipMemcpy(d_b2.p, base2, (size_t)nd * 8, hipMemcpyHostToDevice));
    qd_format_args fa{};
    fa.drop = ra.drop;
    fa.perm = d_perm.as<uint32_t>();
    fa.sdest = d_sdest.as<uint16_t>();
    fa.g1 = d_g1.as<uint32_t>();
    fa.g2 = d_g2.as<uint32_t>();
    fa.base1 = d_b1.as<int64_t>();
    fa.base2 = d_b2.as<int64_t>();
    fa.text1 = t[0];
    fa.text2 = t[1];
    fa.r1 = ra.r1;
    fa.r2 = ra.r2;
    for (int k = 0; k < lay.n_streams; ++k) {
        fa.itext[k] = t[2 + k];
        fa.idx[k] = ra.idx[k];
    }
    fa.out1 = d_out.as<uint8_t>();
    fa.out2 = d_out.as<uint8_t>();
    TCHK(qd_text_format(*plan, S, write_pass, write_fail, write_undet, N, fa, nullptr));
    TCHK(hipDeviceSynchronize());
    if (out_cap) TCHK(hipMemcpy(out, d_out.p, (size_t)out_cap, hipMemcpyDeviceToHost));
    return QD_OK;
}

int qd_dev_pack_members(int device_id, const uint8_t* slots, int64_t stride, const uint32_t* len, int64_t n, uint64_t* offsets, uint8_t* packed,
                        int64_t packed_cap) {
    if (n < 0 || n > 0x7FFFFFFF || stride < 1 || stride > (int64_t)1 << 30 || !offsets || packed_cap < 0 || (!packed && packed_cap) ||
        (n && (!slots || !len)) || n * stride > (int64_t)1 << 32)
        return QD_ERR_INVALID;
    uint64_t total = 0;
    for (int64_t i = 0; i < n; ++i) {  // a member lies inside its slot, and all of them inside `packed`
        if (len[i] > (uint64_t)stride) return QD_ERR_INVALID;
        total += len[i];
    }
    if (total > (uint64_t)packed_cap) return QD_ERR_INVALID;
    TCHK(hipSetDevice(device_id));
    Scratch d_slots, d_len, d_off, d_packed;
    TCHK(d_slots.alloc((size_t)(n * stride)));
    TCHK(d_len.alloc((size_t)n * 4));
    TCHK(d_off.alloc(((size_t)n + 1) * 8));
    TCHK(d_packed.alloc((size_t)packed_cap));
    if (n) {
        TCHK(hipMemcpy(d_slots.p, slots, (size_t)(n * stride), hipMemcpyHostToDevice));
        TCHK(hipMemcpy(d_len.p, len, (size_t)n * 4, hipMemcpyHostToDevice));
    }
    TCHK(hipMemset(d_off.p, 0xFF, ((size_t)n + 1) * 8));
    if (packed_cap) TCHK(hipMemset(d_packed.p, QD_DEV_GUARD_BYTE, (size_t)packed_cap));
    TCHK(qd_text_pack_members(d_slots.as<uint8_t>(), stride, d_len.as<uint32_t>(), (uint32_t)n, d_off.as<uint64_t>(), d_packed.as<uint8_t>(), nullptr));
    TCHK(hipDeviceSynchronize());
    TCHK(hipMemcpy(offsets, d_off.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost));
    if (packed_cap) TCHK(hipMemcpy(packed, d_packed.p, (size_t)packed_cap, hipMemcpyDeviceToHost));
    return QD_OK;
}

}  // extern "C"
