// The progressive JPEG decoder (SOF2) as arithmetic, shared by the host statement (whenet_jpeg_parse_scans,
// whenet_jpeg_decode_progressive_host, ..._planes_host, whenet_jpeg_progressive_coefficients_host) and the kernels of jpeg_prog.hip:
// the parser of a stream of several scans with its scan plan, the four scan kinds of T.81 annex G (G.1.2 / G.2, as jdphuff.c
// executes them) and the finish that turns the raw coefficients into the records the inverse DCT of jpeg_dec_host.h reads.  The
// contract is in include/whenet_hip.h (JPEG DECODER, PROGRESSIVE).  Integers only; nothing here needs the HIP runtime: a plain
// C++17 compiler builds this header (tools/jpeg_prog_host_check.cpp does, under the host sanitizers).
//
// Reference: demo.py (`cv2.imread` of Sample/*.jpeg): stills are where progressive streams are common.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "jpeg_dec_host.h"

namespace whenet {

constexpr int JPEG_PROG_MAX_SCANS = WHENET_JPEG_PROG_MAX_SCANS;
constexpr int JPEG_PROG_LANES = 16;      // items per workgroup of the scan kernel: the item lists are padded to it scan by scan
// (JPEG_PROG_SEQUENTIAL: a scan of a sequential frame that goes through the scan plan -- include/whenet_hip.h, JPEG DECODER, LAYOUTS)
enum { JPEG_PROG_DC_FIRST = 0, JPEG_PROG_DC_REFINE = 1, JPEG_PROG_AC_FIRST = 2, JPEG_PROG_AC_REFINE = 3, JPEG_PROG_SEQUENTIAL = 4 };
// the counter block of whenet_jpeg_progressive_coefficients_host
enum { JPEG_PROG_CNT_SCANS = 0, JPEG_PROG_CNT_ITEMS, JPEG_PROG_CNT_LEVELS, JPEG_PROG_CNT_EOBRUN, JPEG_PROG_CNT_REFINE_ZRL,
       JPEG_PROG_CNT_CORRECTION_BITS, JPEG_PROG_CNT_CORRECTIONS, JPEG_PROG_CNT_WORDS = 8 };

// A scan as the decode reads it (host and device).  Positions are relative to the plan's first entropy byte.
struct JpegProgScan {
    int32_t ns, comp[3];          // its components: indices into the frame's
    int32_t ss, se, ah, al, kind;
    int32_t ri, intervals;        // in the SCAN's MCUs: the frame's for an interleaved scan, single blocks for a scan of one component
    int32_t units;                // the scan's MCUs
    int32_t bw, bh;               // a scan of one component: its block grid ceil(cw / 8) x ceil(ch / 8), raster order
    int32_t first_item, level;    // level: 0-based here
    int32_t data_off, data_end;   // its entropy data
    int32_t list_off, list_cnt;   // its share of the item list (list_cnt: a multiple of JPEG_PROG_LANES)
    int32_t items;                // the intervals listed there: 0 .. items - 1, those whose start the data holds, up to the first one
                                  // the scan's markers make bad
};
// One (scan, interval) item.  scan < 0: padding
struct JpegProgItem {
    int32_t scan, interval, start, end;
};

struct JpegProgPlan {
    bool baseline = false;                     // SOF0: one scan, decoded by the baseline decoder
    bool sequential = false;                   // SOF0 / SOF1 through the scan plan: every scan is of the kind JPEG_PROG_SEQUENTIAL
    std::vector<whenet_jpeg_scan_t> scans;     // the public records
    std::vector<JpegProgScan> dev;
    std::vector<JpegDecHuff> huff;             // 3 per scan: the table of the scan's i-th component (DC first), [0] for an AC scan;
                                               // a sequential frame: 6 per scan, the DC tables of its components, then their AC tables
    int huff_per_scan() const { return sequential ? 6 : 3; }
    int16_t qz[3][64] = {};                    // per component: its quantiser in ZIGZAG order
    std::vector<JpegProgItem> items;           // level by level, inside a level scan by scan, each scan's share padded
    std::vector<int32_t> level_off, level_cnt; // a level's share of `items`
    int levels = 0, total_items = 0;
    int first_bad = JPEG_DEC_NO_BAD;           // what the host knows before the decode: a bad marker's item, or total_items where the
                                               // progression is incomplete
    int64_t data_base = 0, data_bytes = 0;     // the stream's bytes [data_base, data_base + data_bytes): every scan's entropy data
};

// ---- parse (pure host) ----
// SOI .. the last scan into `in` and `plan`; returns nullptr, or the reason the stream is refused.  A SOF0 stream is jpeg_parse's
// (plan.baseline, one scan record).  For SOF2 `in` holds the frame, the quantisers and the first scan's data_offset and DRI; its
// Huffman fields stay empty (the tables change between scans: they are the plan's).  The walk and the SOF / DQT / DHT readers are
// jpeg_dec_host.h's, shared with jpeg_parse.
// layouts: jpeg_parse's argument, and the same samplings for a SOF2 frame (the scan geometry below is written in hs, vs and bpm);
// a DC scan of a SOF2 frame may hold two components; and a sequential frame (SOF0 / SOF1) the baseline parser refuses for its scan
// structure or its table ids -- any number of scans that hold every component once, Ns 1..3, Huffman ids 0..3 -- gets a scan plan of
// JPEG_PROG_SEQUENTIAL scans, all of level 1 (plan.sequential).  A sequential frame of ONE interleaved scan and ids 0..1 stays the
// baseline decoder's (plan.baseline).  sof2 = false: a SOF2 frame is refused with the baseline parser's text.
inline const char* jpeg_prog_parse(const uint8_t* d, int64_t size, whenet_jpeg_info_t& in, JpegProgPlan& plan, bool layouts = false,
                                   bool sof2 = true) {
    plan = JpegProgPlan();
    std::memset(&in, 0, sizeof(in));
    if (size > JPEG_DEC_MAX_BYTES) return "a stream above 2^31 - 1 bytes";
    if (size < 4 || d[0] != 0xFF || d[1] != 0xD8) return "no SOI marker at the start: not a JPEG stream";
    {   // which frame?  (the first SOFn decides; anything else is the baseline parser's to refuse)
        int64_t p = 2;
        int sof = 0;
        while (p + 4 <= size && d[p] == 0xFF) {
            const int m = d[p + 1];
            if (m == 0xFF) {
                ++p;
                continue;
            }
            if (m == 0xD8 || m == 0xD9 || m == 0x01 || (m >= 0xD0 && m <= 0xD7) || m == 0xDA) break;
            if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
                sof = m;
                break;
            }
            p += 2 + ((d[p + 2] << 8) | d[p + 3]);
        }
        if (sof == 0xC2 && !sof2) {
            const char* bad = jpeg_parse(d, size, in, layouts);
            return bad != nullptr ? bad : "progressive DCT (SOF2): baseline sequential streams only";
        }
        if (sof != 0xC2) {
            const char* bad = jpeg_parse(d, size, in, layouts);
            if (bad == nullptr) plan.baseline = true;
            else if (!(layouts && (sof == 0xC0 || sof == 0xC1))) return bad;
            else plan.sequential = true, std::memset(&in, 0, sizeof(in));
        }
        if (plan.baseline) {
            whenet_jpeg_scan_t s{};
            s.ns = in.components;
            for (int c = 0; c < in.components; ++c) s.comp[c] = c, s.dc[c] = in.dc[c], s.ac[c] = in.ac[c];
            s.ss = 0, s.se = 63, s.level = 1;
            s.ri = jpeg_dec_geom(in).ri, s.intervals = in.intervals;
            s.data_offset = in.data_offset, s.data_bytes = size - in.data_offset;
            plan.scans.push_back(s);
            plan.levels = 1, plan.total_items = in.intervals;
            return nullptr;
        }
    }
    const bool seq = plan.sequential;
    uint8_t hc[8][16], hv[8][256];            // the Huffman tables in force, at index 2 id + class
    uint8_t hp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int dht_seen = 0;
    int cur_al[3][64];                        // per component and coefficient: -1 (no scan yet) or the Al it has reached
    for (auto& c : cur_al)
        for (int& v : c) v = -1;
    int comp_id[3] = {0, 0, 0};
    bool sof = false;
    int dri = 0;
    JpegDecGeom g{};
    int64_t p = 2;
    for (;;) {
        int m, n;
        const uint8_t* s;
        const bool scanned = !plan.dev.empty();
        const char* refused = jpeg_next_segment(d, size, scanned, p, m, s, n);
        if (refused != nullptr) return refused;
        if (m == 0xD9) break;      // (behind the first scan: EOI, or the end of the bytes)
        if (seq && m == 0xC2) return "a second frame header";
        if (m == 0xC2 || (seq && (m == 0xC0 || m == 0xC1))) {
            if (sof) return seq ? "a second SOF0" : "a second SOF2";
            refused = jpeg_read_sof(s, n, !seq, in, comp_id, layouts);
            if (refused == nullptr && in.components == 3 && (comp_id[0] == comp_id[1] || comp_id[0] == comp_id[2] || comp_id[1] == comp_id[2]))
                return "two components of the frame share an id";
            sof = true;
        } else if (m >= 0xC0 && m <= 0xCF && m != 0xC4) {
            if (seq) return jpeg_parse(d, size, in, layouts);      // (another frame type, arithmetic coding: the baseline parser's texts)
            return "a second frame header in a progressive stream";
        } else if (m == 0xDB) {
            if (scanned) return seq ? "a quantiser table (DQT) behind the first scan" : "a quantiser table (DQT) behind the first scan of a progressive stream";
            refused = jpeg_read_dqt(s, n, in);
        } else if (m == 0xC4) {
            refused = jpeg_read_dht(s, n, 3, hc, hv, hp);
            ++dht_seen;
        } else if (m == 0xDD) {
            if (n != 2) return "a DRI of the wrong length";
            dri = (s[0] << 8) | s[1];
        } else if (m == 0xDA) {
            if (!sof) return seq ? "SOS before SOF0" : "SOS before SOF2";
            if (n < 1) return "a short SOS";
            const int ns = s[0];
            if (ns == 2 && !layouts) return "a scan of two components: scans hold one component or all of them";
            if (ns != 1 && ns != in.components && !(ns == 2 && in.components == 3))
                return seq ? "a scan must hold one to three of the frame's components" : "a scan must hold one component or all of the frame's";
            if (n != 4 + 2 * ns) return "the length of SOS does not match its components";
            if (int(plan.dev.size()) >= JPEG_PROG_MAX_SCANS) return "more than 128 scans";
            JpegProgScan sc{};
            whenet_jpeg_scan_t pub{};
            sc.ns = ns;
            for (int i = 0; i < ns; ++i) {
                int c = -1;
                for (int j = 0; j < in.components; ++j)
                    if (s[1 + 2 * i] == comp_id[j]) c = j;
                if (c < 0 || (ns > 1 && (ns == 2 ? (i > 0 && c <= sc.comp[0]) : c != i))) return "the scan's components are not the frame's, in order";
                sc.comp[i] = c;
                pub.comp[i] = c, pub.dc[i] = s[2 + 2 * i] >> 4, pub.ac[i] = s[2 + 2 * i] & 15;
                if (pub.dc[i] > 3 || pub.ac[i] > 3) return "a Huffman table id above 3";
            }
            sc.ss = s[1 + 2 * ns], sc.se = s[2 + 2 * ns], sc.ah = s[3 + 2 * ns] >> 4, sc.al = s[3 + 2 * ns] & 15;
            if (seq) {
                if (sc.ss != 0 || sc.se != 63 || sc.ah != 0 || sc.al != 0)
                    return "a spectral selection or successive approximation in a sequential frame (Ss = 0, Se = 63, Ah = Al = 0 only)";
                for (int i = 0; i < ns; ++i)
                    if (cur_al[sc.comp[i]][0] >= 0) return "a component in two scans of a sequential frame";
            }
            if (sc.ss > sc.se || sc.se > 63) return "a spectral selection with Ss > Se or Se > 63";
            if (sc.ss == 0 && sc.se != 0 && !seq) return "a scan of DC and AC coefficients together (Ss = 0 with Se != 0)";
            if (sc.ss > 0 && ns > 1) return "an interleaved AC scan (Ss > 0 with several components)";
            if (sc.ah > 13 || sc.al > 13) return "a successive approximation bit position above 13";
            for (int i = 0; i < ns; ++i) {
                int* const al = cur_al[sc.comp[i]];
                if (sc.ss > 0 && al[0] < 0) return "an AC scan of a component whose DC coefficient has had no scan";
                for (int k = sc.ss; k <= sc.se; ++k) {
                    if (sc.ah == 0) {
                        if (al[k] >= 0) return "a first scan of a coefficient that already had one";
                    } else if (al[k] < 0) {
                        return "a refinement scan of a coefficient that has had no first scan";
                    } else if (al[k] != sc.ah || sc.al != sc.ah - 1) {
                        return "a refinement scan whose Ah is not the coefficient's bit position, or whose Al is not Ah - 1";
                    }
                }
            }
            for (int i = 0; i < ns; ++i)
                for (int k = sc.ss; k <= sc.se; ++k) cur_al[sc.comp[i]][k] = sc.al;
            for (int c = 0; c < in.components; ++c)
                if (!in.q_present[in.qt[c]]) return "a missing quantiser table (DQT)";
            sc.kind = sc.ss == 0 ? (sc.ah == 0 ? JPEG_PROG_DC_FIRST : JPEG_PROG_DC_REFINE) : (sc.ah == 0 ? JPEG_PROG_AC_FIRST : JPEG_PROG_AC_REFINE);
            if (seq) sc.kind = JPEG_PROG_SEQUENTIAL;
            JpegDecHuff hu[6];
            std::memset(hu, 0, sizeof(hu));
            if (seq) {
                for (int i = 0; i < ns; ++i) {
                    if (!hp[2 * pub.dc[i]] || !hp[2 * pub.ac[i] + 1]) return "a missing Huffman table (DHT)";
                    jpeg_dec_build_huff(hc[2 * pub.dc[i]], hv[2 * pub.dc[i]], hu[i]);
                    jpeg_dec_build_huff(hc[2 * pub.ac[i] + 1], hv[2 * pub.ac[i] + 1], hu[3 + i]);
                }
            } else if (sc.kind == JPEG_PROG_DC_FIRST) {
                for (int i = 0; i < ns; ++i) {
                    if (!hp[2 * pub.dc[i]]) return "a missing Huffman table (DHT)";
                    jpeg_dec_build_huff(hc[2 * pub.dc[i]], hv[2 * pub.dc[i]], hu[i]);
                }
            } else if (sc.ss > 0) {
                if (!hp[2 * pub.ac[0] + 1]) return "a missing Huffman table (DHT)";
                jpeg_dec_build_huff(hc[2 * pub.ac[0] + 1], hv[2 * pub.ac[0] + 1], hu[0]);
            }
            if (plan.dev.empty()) {
                in.restart_interval = dri, in.data_offset = p;
                g = jpeg_dec_geom(in);
                in.intervals = g.intervals;
            }
            // geometry: the frame's MCUs, or the component's own block grid
            if (ns > 1 || in.components == 1) {
                sc.bw = g.mcu_cols, sc.bh = g.mcu_rows;
            } else {
                const int c = sc.comp[0];
                const int cw = c == 0 ? in.w : (in.w + g.hs - 1) / g.hs, ch = c == 0 ? in.h : (in.h + g.vs - 1) / g.vs;
                sc.bw = (cw + 7) / 8, sc.bh = (ch + 7) / 8;
            }
            sc.units = sc.bw * sc.bh;
            sc.ri = dri > 0 && dri < sc.units ? dri : sc.units;
            sc.intervals = (sc.units + sc.ri - 1) / sc.ri;
            // levels: 1 + the largest level of an earlier scan that shares a component and overlaps the band
            sc.level = 0;
            for (const JpegProgScan& e : plan.dev) {
                bool share = false;
                for (int i = 0; i < ns; ++i)
                    for (int j = 0; j < e.ns; ++j) share = share || sc.comp[i] == e.comp[j];
                if (share && e.ss <= sc.se && sc.ss <= e.se) sc.level = std::max(sc.level, e.level + 1);
            }
            // the scan's end and its restart markers
            const int64_t from = p;
            if (plan.dev.empty()) plan.data_base = from;
            // (list_off: for now the scan's place in `items`; the lists are laid out below.  An item is listed where the data holds
            //  its start -- interval 0, and interval k + 1 behind marker k --, so the list is bounded by the bytes, never by what a
            //  header claims: 8192 x 8192 with DRI 1 claims a million intervals per scan)
            sc.list_off = int32_t(plan.items.size()), sc.list_cnt = 0;
            plan.items.push_back({int32_t(plan.dev.size()), 0, int32_t(from - plan.data_base), 0});
            int bad = JPEG_DEC_NO_BAD, k = 0;
            int64_t q = from;
            for (;;) {
                const void* f = q < size ? std::memchr(d + q, 0xFF, size_t(size - q)) : nullptr;
                if (f == nullptr) {
                    q = size;
                    break;
                }
                q = static_cast<const uint8_t*>(f) - d;
                if (q + 1 >= size) {      // a lone 0xFF at the end: the bit reader stops there
                    q = size;
                    break;
                }
                const int b = d[q + 1];
                if (b == 0) {
                    q += 2;
                } else if (b == 0xFF) {
                    ++q;
                } else if (b >= 0xD0 && b <= 0xD7) {
                    if (k >= sc.intervals - 1) bad = std::min(bad, sc.intervals - 1);
                    else if ((b & 7) != (k & 7)) bad = std::min(bad, k);
                    if (k + 1 < sc.intervals) plan.items.push_back({int32_t(plan.dev.size()), k + 1, int32_t(q + 2 - plan.data_base), 0});
                    ++k, q += 2;
                } else {
                    break;      // another marker: the scan ends in front of it
                }
            }
            if (k < sc.intervals - 1) bad = std::min(bad, k);
            sc.data_off = int32_t(from - plan.data_base), sc.data_end = int32_t(q - plan.data_base);
            sc.first_item = plan.total_items;
            plan.total_items += sc.intervals;
            if (bad != JPEG_DEC_NO_BAD) plan.first_bad = std::min(plan.first_bad, sc.first_item + bad);
            plan.data_bytes = q - plan.data_base;
            // the intervals behind the one the markers make bad are not decoded: not listed either
            while (plan.items.back().interval > bad) plan.items.pop_back();
            sc.items = int32_t(plan.items.size()) - sc.list_off;
            for (int i = 0; i < sc.items; ++i) plan.items[size_t(sc.list_off + i)].end = sc.data_end;
            pub.ns = ns, pub.ss = sc.ss, pub.se = sc.se, pub.ah = sc.ah, pub.al = sc.al, pub.tables = dht_seen;
            pub.ri = sc.ri, pub.intervals = sc.intervals, pub.level = sc.level + 1, pub.first_item = sc.first_item, pub.progressive = seq ? 0 : 1;
            pub.data_offset = from, pub.data_bytes = q - from;
            plan.scans.push_back(pub), plan.dev.push_back(sc);
            for (int i = 0; i < plan.huff_per_scan(); ++i) plan.huff.push_back(hu[i]);
            p = q;
            continue;
        } else if (!((m >= 0xE0 && m <= 0xEF) || m == 0xFE)) {      // (APPn, COM: skipped)
            return "an unexpected marker in the header";
        }
        if (refused != nullptr) return refused;
    }
    // the item lists: level by level, a scan's share padded to whole workgroups
    std::vector<JpegProgItem> flat;
    flat.swap(plan.items);
    for (const JpegProgScan& sc : plan.dev) plan.levels = std::max(plan.levels, sc.level + 1);
    for (int l = 0; l < plan.levels; ++l) {
        plan.level_off.push_back(int32_t(plan.items.size()));
        for (JpegProgScan& sc : plan.dev) {
            if (sc.level != l) continue;
            const int from = sc.list_off;
            sc.list_off = int32_t(plan.items.size());
            for (int i = 0; i < sc.items; ++i) plan.items.push_back(flat[size_t(from + i)]);
            while (plan.items.size() % JPEG_PROG_LANES) plan.items.push_back({-1, 0, 0, 0});
            sc.list_cnt = int32_t(plan.items.size()) - sc.list_off;
        }
        plan.level_cnt.push_back(int32_t(plan.items.size()) - plan.level_off.back());
    }
    for (int c = 0; c < in.components; ++c)
        for (int k = 0; k < 64; ++k) {
            plan.qz[c][k] = int16_t(in.q[in.qt[c]][JPEG_ZIGZAG[k]]);
            if (cur_al[c][k] != 0) plan.first_bad = std::min(plan.first_bad, plan.total_items);      // incomplete progression
        }
    return nullptr;
}

// ---- the scan decode (host and device) ----
// k <= 16 raw bits; false: the data ends inside them
WHENET_HD inline bool jpeg_prog_bits(JpegBitReader& br, int k, int& v) {
    v = 0;
    if (k == 0) return true;
    br.fill();
    if (k > br.n) return false;
    v = int((br.acc >> (br.n - k)) & ((1u << k) - 1u));
    br.n -= k;
    return true;
}
WHENET_HD inline int16_t jpeg_prog_i16(int v) { return int16_t(jpeg_dec_clamp(v, -32768, 32767)); }

// the record of unit u of a scan (b: the block inside the MCU of an interleaved scan)
WHENET_HD inline long long jpeg_prog_record(const JpegDecGeom& g, const JpegProgScan& sc, int u, int b) {
    if (sc.ns > 1) return (long long)(u) * g.bpm + b;
    if (g.comps == 1) return u;
    const int by = u / sc.bw, bx = u - by * sc.bw;
    if (sc.comp[0] == 0) return ((long long)(by / g.vs) * g.mcu_cols + bx / g.hs) * g.bpm + (by % g.vs) * g.hs + bx % g.hs;
    return ((long long)(by) * g.mcu_cols + bx) * g.bpm + (g.bpm - 2) + (sc.comp[0] - 1);
}

// the blocks scan component i has in a unit of the scan (an interleaved scan: H_c V_c of them, T.81 A.2.3), and block j of them as its
// index in the frame's MCU (what jpeg_prog_record takes)
WHENET_HD inline int jpeg_prog_unit_blocks(const JpegDecGeom& g, const JpegProgScan& sc, int i) {
    return sc.ns > 1 && sc.comp[i] == 0 ? g.bpm - 2 : 1;
}
WHENET_HD inline int jpeg_prog_unit_block(const JpegDecGeom& g, const JpegProgScan& sc, int i, int j) {
    return sc.ns > 1 ? (sc.comp[i] == 0 ? j : g.bpm - 2 + sc.comp[i] - 1) : 0;
}

// one correction bit for a coefficient that is already non-zero; false: the data ends inside it
WHENET_HD inline bool jpeg_prog_correct(JpegBitReader& br, int16_t& coef, int p1, long long* cnt) {
    int bit;
    if (!jpeg_prog_bits(br, 1, bit)) return false;
    if (cnt != nullptr) ++cnt[JPEG_PROG_CNT_CORRECTION_BITS];
    if (bit != 0 && (int(coef) & p1) == 0) {
        coef = jpeg_prog_i16(int(coef) + (coef >= 0 ? p1 : -p1));
        if (cnt != nullptr) ++cnt[JPEG_PROG_CNT_CORRECTIONS];
    }
    return true;
}

// One (scan, interval) item into raw ([block][64] int16, zigzag order inside a record).  Only the int16s of the scan's band are
// stored: scans of one level write other bands of the same records at the same time.  false: the interval is damaged; the block in
// hand keeps what was written, the rest of the interval is not touched.
// (stage: nullptr, or 64 int16 of fast memory: an AC refinement copies its band there, works on it and stores the band back.
//  cnt: nullptr, or the counter block)
WHENET_HD inline bool jpeg_prog_item(const uint8_t* data, int start, int end, const JpegProgScan& sc, const JpegDecHuff* huff, const JpegDecGeom& g,
                                     int interval, int16_t* raw, int16_t* stage = nullptr, long long* cnt = nullptr) {
    JpegBitReader br(data, start, end);
    const int first = interval * sc.ri;
    const int last = first + sc.ri < sc.units ? first + sc.ri : sc.units;
    const int p1 = 1 << sc.al;
    if (sc.kind == JPEG_PROG_DC_FIRST) {
        int pred0 = 0, pred1 = 0, pred2 = 0;
        for (int u = first; u < last; ++u)
            for (int i = 0; i < sc.ns; ++i)      // the scan's i-th component
                for (int j = 0, nb = jpeg_prog_unit_blocks(g, sc, i); j < nb; ++j) {
                    int v;
                    const int s = br.decode(huff[i]);
                    if (s < 0 || !br.receive(s & 15, v)) return false;
                    int& pred = i == 0 ? pred0 : (i == 1 ? pred1 : pred2);
                    pred = jpeg_dec_clamp(pred + v, -32768, 32767);
                    raw[jpeg_prog_record(g, sc, u, jpeg_prog_unit_block(g, sc, i, j)) * 64] = jpeg_prog_i16(pred * p1);
                }
        return true;
    }
    if (sc.kind == JPEG_PROG_DC_REFINE) {
        for (int u = first; u < last; ++u)
            for (int i = 0; i < sc.ns; ++i)
                for (int j = 0, nb = jpeg_prog_unit_blocks(g, sc, i); j < nb; ++j) {
                    int bit;
                    if (!jpeg_prog_bits(br, 1, bit)) return false;
                    int16_t* const rec = raw + jpeg_prog_record(g, sc, u, jpeg_prog_unit_block(g, sc, i, j)) * 64;
                    if (bit != 0) rec[0] = int16_t(rec[0] | p1);
                }
        return true;
    }
    int eobrun = 0;
    if (sc.kind == JPEG_PROG_AC_FIRST) {
        for (int u = first; u < last; ++u) {
            if (eobrun > 0) {
                --eobrun;
                continue;
            }
            int16_t* const rec = raw + jpeg_prog_record(g, sc, u, 0) * 64;
            for (int k = sc.ss; k <= sc.se;) {
                const int sym = br.decode(huff[0]);
                if (sym < 0) return false;
                const int r = sym >> 4, s = sym & 15;
                int v;
                if (s != 0) {
                    k += r;
                    if (k > sc.se || !br.receive(s, v)) return false;
                    rec[k] = jpeg_prog_i16(v * p1);
                    ++k;
                } else if (r == 15) {
                    k += 16;
                    if (k > sc.se + 1) return false;
                } else {
                    if (!jpeg_prog_bits(br, r, v)) return false;
                    eobrun = (1 << r) + v;
                    if (cnt != nullptr && eobrun > cnt[JPEG_PROG_CNT_EOBRUN]) cnt[JPEG_PROG_CNT_EOBRUN] = eobrun;
                    if (u + eobrun > last) return false;      // the run passes the interval's last block
                    --eobrun;
                    break;
                }
            }
        }
        return true;
    }
    // AC refinement (G.1.2.3)
    for (int u = first; u < last; ++u) {
        int16_t* const rec = raw + jpeg_prog_record(g, sc, u, 0) * 64;
        int16_t* const w = stage != nullptr ? stage : rec;
        if (stage != nullptr)
            for (int k = sc.ss; k <= sc.se; ++k) stage[k] = rec[k];
        bool ok = true;
        int k = sc.ss;
        if (eobrun == 0) {
            while (k <= sc.se) {
                const int sym = br.decode(huff[0]);
                if (sym < 0) {
                    ok = false;
                    break;
                }
                int r = sym >> 4, s = sym & 15, v = 0;
                if (s != 0) {
                    if (s != 1 || !jpeg_prog_bits(br, 1, v)) {
                        ok = false;
                        break;
                    }
                    v = v != 0 ? p1 : -p1;
                } else if (r != 15) {
                    if (!jpeg_prog_bits(br, r, v)) {
                        ok = false;
                        break;
                    }
                    eobrun = (1 << r) + v;
                    if (cnt != nullptr && eobrun > cnt[JPEG_PROG_CNT_EOBRUN]) cnt[JPEG_PROG_CNT_EOBRUN] = eobrun;
                    if (u + eobrun > last) ok = false, eobrun = 0;
                    break;
                } else if (cnt != nullptr) {
                    ++cnt[JPEG_PROG_CNT_REFINE_ZRL];
                }
                // over r coefficients without a history; every one with a history on the way reads its correction bit
                bool placed = false;
                for (; k <= sc.se; ++k) {
                    if (w[k] != 0) {
                        if (!jpeg_prog_correct(br, w[k], p1, cnt)) {
                            ok = false;
                            break;
                        }
                    } else if (--r < 0) {
                        placed = true;
                        break;
                    }
                }
                if (!ok) break;
                if (!placed) {      // the run passes Se
                    ok = false;
                    break;
                }
                if (s != 0) w[k] = jpeg_prog_i16(v);
                ++k;
            }
        }
        if (ok && eobrun > 0) {
            for (; k <= sc.se; ++k)
                if (w[k] != 0 && !jpeg_prog_correct(br, w[k], p1, cnt)) {
                    ok = false;
                    break;
                }
            --eobrun;
        }
        if (stage != nullptr)
            for (int j = sc.ss; j <= sc.se; ++j) rec[j] = stage[j];
        if (!ok) return false;
    }
    return true;
}

// ---- a scan of a sequential frame (JPEG_PROG_SEQUENTIAL; host and device) ----
// One block as the baseline decoder reads it (jpeg_dec_block: DC symbol + EXTEND on the component's predictor, then AC symbols, no EOB
// runs), but RAW: out[zigzag k] = the value itself (out is zero on entry).  The finish multiplies and clamps, which gives exactly
// jpeg_dec_block's record.  false: damage; what was written stays.
WHENET_HD inline bool jpeg_seq_block(JpegBitReader& br, const JpegDecHuff& dc, const JpegDecHuff& ac, int& pred, int16_t* out) {
    int s = br.decode(dc), v;
    if (s < 0 || !br.receive(s & 15, v)) return false;
    pred = jpeg_dec_clamp(pred + v, -32768, 32767);
    out[0] = int16_t(pred);
    for (int k = 1; k < 64;) {
        const int sym = br.decode(ac);
        if (sym < 0) return false;
        const int r = sym >> 4;
        s = sym & 15;
        if (s == 0) {
            if (r != 15) break;      // EOB
            k += 16;                 // ZRL
            if (k > 64) return false;
            continue;
        }
        k += r;
        if (k > 63 || !br.receive(s, v)) return false;      // (|v| < 2^15: s <= 15)
        out[k] = int16_t(v);
        ++k;
    }
    return true;
}

// One (scan, interval) item of a sequential scan into raw.  huff: the scan's six tables (DC of its i-th component at [i], AC at
// [3 + i]).  The scans of a sequential frame hold different components, so an item owns its records: a block is decoded in `stage`
// (64 int16 of fast memory, 16-byte aligned like raw; nullptr: in place) and leaves as a whole record.  false: the interval is
// damaged; the block in hand keeps what was decoded of it, the blocks behind it stay zero.
WHENET_HD inline bool jpeg_seq_item(const uint8_t* data, int start, int end, const JpegProgScan& sc, const JpegDecHuff* huff, const JpegDecGeom& g,
                                    int interval, int16_t* raw, int16_t* stage = nullptr) {
    JpegBitReader br(data, start, end);
    const int first = interval * sc.ri;
    const int last = first + sc.ri < sc.units ? first + sc.ri : sc.units;
    int pred0 = 0, pred1 = 0, pred2 = 0;
    for (int u = first; u < last; ++u)
        for (int i = 0; i < sc.ns; ++i)
            for (int j = 0, nb = jpeg_prog_unit_blocks(g, sc, i); j < nb; ++j) {
                int16_t* const rec = raw + jpeg_prog_record(g, sc, u, jpeg_prog_unit_block(g, sc, i, j)) * 64;
                if (stage != nullptr) std::memset(__builtin_assume_aligned(stage, 16), 0, 128);
                int& pred = i == 0 ? pred0 : (i == 1 ? pred1 : pred2);
                const bool ok = jpeg_seq_block(br, huff[i], huff[3 + i], pred, stage != nullptr ? stage : rec);
                if (stage != nullptr) std::memcpy(__builtin_assume_aligned(rec, 16), __builtin_assume_aligned(stage, 16), 128);
                if (!ok) return false;
            }
    return true;
}

// the finish of one value: record[natural k] = clamp(raw[zigzag k] x Q[k], -2048, 2047)
WHENET_HD inline int16_t jpeg_prog_finish_value(int raw, int q) { return int16_t(jpeg_dec_clamp(raw * q, -2048, 2047)); }

// ---- the host statement ----
struct JpegProgResult {
    std::vector<int16_t> raw, coef;      // [blocks][64]: zigzag order as the scans left them; natural order, dequantised, clamped
    long long cnt[JPEG_PROG_CNT_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// every scan in stream order (a scan depends on earlier scans only, and the scans of one level touch different values), then the
// finish; status[0] = WHENET_OK or WHENET_EFORMAT, status[1] = the smallest bad flat item (the item count for an incomplete
// progression) or -1
inline void jpeg_prog_coefficients_host(const whenet_jpeg_info_t& in, const JpegProgPlan& plan, const uint8_t* data, JpegProgResult& out,
                                        int32_t status[2]) {
    const JpegDecGeom g = jpeg_dec_geom(in);
    const size_t blocks = size_t(g.mcu_cols) * size_t(g.mcu_rows) * size_t(g.bpm);
    out.raw.assign(blocks * 64, 0), out.coef.assign(blocks * 64, 0);
    int bad = plan.first_bad;
    alignas(16) int16_t stage[64];
    for (const JpegProgScan& sc : plan.dev)
        for (int i = 0; i < sc.items; ++i) {
            const JpegProgItem& it = plan.items[size_t(sc.list_off + i)];
            const size_t s = size_t(&sc - plan.dev.data());
            const JpegDecHuff* const hu = plan.huff.data() + size_t(plan.huff_per_scan()) * s;
            const bool ok = sc.kind == JPEG_PROG_SEQUENTIAL ? jpeg_seq_item(data, it.start, it.end, sc, hu, g, it.interval, out.raw.data(), stage)
                                                            : jpeg_prog_item(data, it.start, it.end, sc, hu, g, it.interval, out.raw.data(), stage, out.cnt);
            if (!ok) bad = std::min(bad, sc.first_item + it.interval);
        }
    for (size_t b = 0; b < blocks; ++b) {
        const int bi = int(b % size_t(g.bpm)), c = g.comps == 1 || bi < g.bpm - 2 ? 0 : bi - (g.bpm - 2) + 1;
        for (int k = 0; k < 64; ++k) out.coef[b * 64 + JPEG_ZIGZAG[k]] = jpeg_prog_finish_value(out.raw[b * 64 + size_t(k)], plan.qz[c][k]);
    }
    out.cnt[JPEG_PROG_CNT_SCANS] = (long long)(plan.dev.size()), out.cnt[JPEG_PROG_CNT_ITEMS] = plan.total_items;
    out.cnt[JPEG_PROG_CNT_LEVELS] = plan.levels;
    status[0] = bad == JPEG_DEC_NO_BAD ? WHENET_OK : WHENET_EFORMAT;
    status[1] = bad == JPEG_DEC_NO_BAD ? -1 : bad;
}

// finished records -> the padded component planes by the rule's inverse DCT
inline void jpeg_prog_planes_host(const JpegDecGeom& g, const std::vector<int16_t>& coef, JpegDecPlanes& out, int rule) {
    for (int c = 0; c < g.comps; ++c) out.plane[c].assign(size_t(g.plane_pitch[c]) * size_t(g.plane_rows[c]), 0);
    const long long mcus = (long long)(g.mcu_cols) * g.mcu_rows;
    for (long long m = 0; m < mcus; ++m)
        for (int b = 0; b < g.bpm; ++b) {
            int comp, y0, x0;
            uint8_t smp[8][8];
            jpeg_dec_block_origin(g, m, b, comp, y0, x0);
            jpeg_dec_block_samples(coef.data() + (size_t(m) * size_t(g.bpm) + size_t(b)) * 64, rule, smp);
            uint8_t* dst = out.plane[comp].data() + size_t(y0) * size_t(g.plane_pitch[comp]) + size_t(x0);
            for (int y = 0; y < 8; ++y) std::memcpy(dst + size_t(y) * size_t(g.plane_pitch[comp]), smp[y], 8);
        }
}

// a whole stream -> planes: a SOF0 stream by the baseline statement, a SOF2 stream by the above
inline void jpeg_prog_decode_planes_host(const whenet_jpeg_info_t& in, const JpegProgPlan& plan, const uint8_t* d, int64_t size, JpegDecPlanes& out,
                                         int32_t status[2], int rule) {
    if (plan.baseline) {
        jpeg_dec_planes_host(in, d + in.data_offset, int(size - in.data_offset), out, status, rule);
        return;
    }
    JpegProgResult r;
    jpeg_prog_coefficients_host(in, plan, d + plan.data_base, r, status);
    jpeg_prog_planes_host(jpeg_dec_geom(in), r.coef, out, rule);
}

}  // namespace whenet
