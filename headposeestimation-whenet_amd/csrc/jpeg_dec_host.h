// The baseline JPEG decoder as arithmetic, shared by the host statement (whenet_jpeg_parse, whenet_jpeg_decode_host,
// whenet_jpeg_decode_planes_host) and the kernels of jpeg_dec.hip: the marker parser, the decode tables of a DHT, the bit reader,
// the Huffman decode of a block, the inverse DCT and the planes -> pixel rule, each exactly as include/whenet_hip.h states it
// (JPEG DECODER), and for rule 1 (libjpeg's bytes) jidctint's pass, the fancy upsampling and jdcolor's row (JPEG DECODER, RULE 1).
// The marker walk, the SOF / DQT / DHT readers and the builder of a decode table are written once here: the progressive parser
// (jpeg_prog_host.h) walks the same grammar with them.
// Integers only.  Nothing here needs the HIP runtime: a plain C++17 compiler builds this header
// (tools/jpeg_dec_host_check.cpp does, under the host sanitizers).
//
// Reference: demo.py (`cv2.imread` of Sample/*.jpeg) and demo_video.py:49-53 (`cap.read()`: for a camera or an MJPG file a
// Motion-JPEG decode): the stage that produces the pixels.  The decoding procedure is the JPEG standard's (ITU-T T.81, annex F.2).
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "jpeg_host.h"

namespace whenet {

constexpr int JPEG_DEC_LOOK_BITS = 9;                 // the lookahead table resolves codes of up to 9 bits
constexpr int JPEG_DEC_NO_BAD = 0x7FFFFFFF;           // "no bad interval" while the decode runs
constexpr int64_t JPEG_DEC_MAX_BYTES = 0x7FFFFFFF;    // positions in a stream are int32

// A DHT as the decoder reads it: look[next 9 bits] = (length << 8) | symbol (0: no code of <= 9 bits starts there); for the longer
// codes T.81 F.2.2.3: a code of length l is one iff code <= maxcode[l], its symbol is vals[valoff[l] + code]
struct JpegDecHuff {
    uint16_t look[1 << JPEG_DEC_LOOK_BITS];
    int32_t maxcode[17];      // -1: no code of that length
    int32_t valoff[17];
    uint8_t vals[256];
};
// What the entropy decode needs besides the bytes: the four tables (2 id + class: DC0, AC0, DC1, AC1) and the quantisers
struct JpegDecTables {
    JpegDecHuff huff[4];
    int16_t q[4][64];         // natural order
    uint8_t zz[64];           // zigzag position -> natural index (with the tables: a lookup beside them, not a load from memory)
};
// The geometry of a stream, from its whenet_jpeg_info_t
struct JpegDecGeom {
    int h, w, comps, hs, vs;          // hs, vs: the luma sampling factors, hs 1, 2 or 4 and vs 1 or 2 (grey: 1, 1)
    int mcu_cols, mcu_rows, bpm;      // blocks per MCU: hs vs + 2 (up to 10, T.81's limit), or 1 for grey
    int ri, intervals;                // MCUs per interval (no DRI: all of them), ceil(MCUs / ri)
    int qt[3], dc[3], ac[3];          // per component: quantiser id, index of its DC / AC table in JpegDecTables::huff
    int plane_pitch[3], plane_rows[3];// the component planes padded to whole MCUs: every block lies inside its plane
};

inline JpegDecGeom jpeg_dec_geom(const whenet_jpeg_info_t& in) {
    JpegDecGeom g{};
    g.h = in.h, g.w = in.w, g.comps = in.components;
    g.hs = in.components == 3 ? in.hs : 1, g.vs = in.components == 3 ? in.vs : 1;
    g.mcu_cols = (in.w + 8 * g.hs - 1) / (8 * g.hs), g.mcu_rows = (in.h + 8 * g.vs - 1) / (8 * g.vs);
    g.bpm = in.components == 3 ? g.hs * g.vs + 2 : 1;
    const int64_t mcus = int64_t(g.mcu_cols) * g.mcu_rows;
    g.ri = in.restart_interval > 0 && in.restart_interval < mcus ? in.restart_interval : int(mcus);
    g.intervals = int((mcus + g.ri - 1) / g.ri);
    for (int c = 0; c < 3; ++c) {
        g.qt[c] = in.qt[c] & 3, g.dc[c] = 2 * (in.dc[c] & 1), g.ac[c] = 2 * (in.ac[c] & 1) + 1;
        g.plane_pitch[c] = g.mcu_cols * 8 * (c == 0 ? g.hs : 1), g.plane_rows[c] = g.mcu_rows * 8 * (c == 0 ? g.vs : 1);
    }
    return g;
}

// log2 of a sampling factor 1, 2 or 4: the shift that takes a pixel's coordinate to its chroma sample's (host and device)
WHENET_HD inline int jpeg_dec_shift(int factor) { return factor >> 1; }
// the luma factors the decoder has geometry for: the baseline set, and with `layouts` 1x2 (4:4:0), 4x1 (4:1:1) and 4x2 (4:1:0) too
inline bool jpeg_dec_sampling_ok(int hs, int vs, bool layouts) {
    if ((hs == 2 && vs == 2) || (hs == 2 && vs == 1) || (hs == 1 && vs == 1)) return true;
    return layouts && ((hs == 1 && vs == 2) || (hs == 4 && vs == 1) || (hs == 4 && vs == 2));
}

// ---- the segment readers (pure host): one grammar for jpeg_parse below and jpeg_prog_parse (jpeg_prog_host.h) ----
// Each returns nullptr, or the reason the stream is refused.  The order of the checks is part of the contract: it decides which
// text a stream with two defects gets (tests/test_jpeg_parse_pins_cpu.py).

// One step of the marker walk: the segment at p, fill bytes skipped, as its marker m and the n bytes s behind its length; p ends up
// behind the segment.  scanned: behind the first scan of a progressive stream EOI or the end of the bytes ends the stream (an
// incomplete progression is decoded from what it holds): m = 0xD9 then.
inline const char* jpeg_next_segment(const uint8_t* d, int64_t size, bool scanned, int64_t& p, int& m, const uint8_t*& s, int& n) {
    m = 0xD9;
    for (;; ++p) {
        if (p + 2 > size) return scanned ? nullptr : "the header ends before SOS (truncated)";
        if (d[p] != 0xFF) return "a marker is expected in the header";
        if (d[p + 1] != 0xFF) break;      // (0xFF 0xFF: a fill byte)
    }
    const int marker = d[p + 1];
    p += 2;
    if (marker == 0xD8 || marker == 0x01 || (marker >= 0xD0 && marker <= 0xD7)) return "an unexpected marker without a segment in the header";
    if (marker == 0xD9) return scanned ? nullptr : "EOI before SOS: the stream has no scan";
    if (p + 2 > size) return scanned ? nullptr : "the header ends before SOS (truncated)";
    const int len = (d[p] << 8) | d[p + 1];
    if (len < 2 || p + len > size) return scanned ? nullptr : "a segment passes the end of the stream (truncated)";
    m = marker, s = d + p + 2, n = len - 2, p += len;
    return nullptr;
}

// SOF0, or SOF2 (sof2: the name in the texts): the frame into `in`, its component ids into comp_id
// (layouts: the samplings of the header's JPEG DECODER, LAYOUTS are frames too; the other factors are refused by name)
inline const char* jpeg_read_sof(const uint8_t* s, int n, bool sof2, whenet_jpeg_info_t& in, int comp_id[3], bool layouts = false) {
    if (n < 6) return sof2 ? "a short SOF2" : "a short SOF0";
    if (s[0] == 12) return "12-bit samples: 8-bit streams only";
    if (s[0] != 8) return "the sample precision is not 8 bit";
    in.h = (s[1] << 8) | s[2], in.w = (s[3] << 8) | s[4], in.components = s[5];
    if (in.components == 4) return "4 components (CMYK / YCCK): 1 or 3 only";
    if (in.components != 1 && in.components != 3) return "the frame must have 1 or 3 components";
    if (in.h < 1 || in.w < 1 || in.h > JPEG_MAX_SIDE || in.w > JPEG_MAX_SIDE) return "frame sides must be 1..8192";
    if (n != 6 + 3 * in.components) return sof2 ? "the length of SOF2 does not match its components" : "the length of SOF0 does not match its components";
    for (int c = 0; c < in.components; ++c) {
        comp_id[c] = s[6 + 3 * c];
        const int hv = s[7 + 3 * c], tq = s[8 + 3 * c];
        if (tq > 3) return "a quantiser id above 3";
        in.qt[c] = tq;
        if (in.components == 1) {
            in.hs = in.vs = 1;      // one component: the MCU is one block whatever the factors say
        } else if (c == 0) {
            if (!jpeg_dec_sampling_ok(hv >> 4, hv & 15, layouts))
                return !layouts          ? "luma sampling must be 2x2 (4:2:0), 2x1 (4:2:2) or 1x1 (4:4:4)"
                       : (hv & 15) == 4  ? "a luma sampling factor vs = 4: the luma factors must be hs 1, 2 or 4 by vs 1 or 2"
                                         : "luma sampling factors other than hs 1, 2 or 4 by vs 1 or 2";
            in.hs = hv >> 4, in.vs = hv & 15;
        } else if (hv != 0x11) {
            if (layouts && c == 2) return "Cb and Cr sampling factors that differ: chroma sampling must be 1x1";      // (Cb's were 1x1)
            return layouts ? "chroma sampling factors other than 1x1: chroma sampling must be 1x1" : "chroma sampling must be 1x1";
        }
    }
    return nullptr;
}

// DQT: its tables into in.q (natural order)
inline const char* jpeg_read_dqt(const uint8_t* s, int n, whenet_jpeg_info_t& in) {
    for (int i = 0; i < n; i += 65) {
        const int pq = s[i] >> 4, tq = s[i] & 15;
        if (pq != 0) return "a 16-bit quantiser table (DQT): 8-bit tables only";
        if (tq > 3) return "a quantiser id above 3";
        if (i + 65 > n) return "a short DQT";
        for (int k = 0; k < 64; ++k) {
            if (s[i + 1 + k] == 0) return "a quantiser of 0";
            in.q[tq][JPEG_ZIGZAG[k]] = s[i + 1 + k];
        }
        in.q_present[tq] = 1;
    }
    return nullptr;
}

// The 16 code-length counts of a Huffman table: the symbols they count, or -1 where they are no prefix code
inline int jpeg_huff_symbols(const uint8_t counts[16]) {
    int total = 0;
    unsigned code = 0;
    for (int l = 1; l <= 16; ++l) {
        total += counts[l - 1], code += counts[l - 1];
        if (code > (1u << l)) return -1;
        code <<= 1;
    }
    return total;
}
// a DC table's symbols are the categories 0..11
inline bool jpeg_huff_dc_symbols_ok(const uint8_t* values, int total) {
    for (int k = 0; k < total; ++k)
        if (values[k] > 11) return false;
    return true;
}

// DHT: its tables into counts / values / present at index 2 id + class (the order of JpegDecTables::huff); ids 0..max_id
inline const char* jpeg_read_dht(const uint8_t* s, int n, int max_id, uint8_t (*counts)[16], uint8_t (*values)[256], uint8_t* present) {
    for (int i = 0; i < n;) {
        const int tc = s[i] >> 4, th = s[i] & 15;
        if (tc > 1 || th > max_id)
            return max_id == 1 ? "a Huffman table class or id above 1 (baseline: ids 0..1)" : "a Huffman table class above 1 or id above 3";
        if (i + 17 > n) return "a short DHT";
        const int tb = 2 * th + tc;
        const int total = jpeg_huff_symbols(s + i + 1);
        if (total < 0) return "a DHT whose code lengths are no prefix code";
        if (total > 256 || i + 17 + total > n) return "a short DHT";
        std::memcpy(counts[tb], s + i + 1, 16);
        std::memset(values[tb], 0, 256);
        std::memcpy(values[tb], s + i + 17, size_t(total));
        if (tc == 0 && !jpeg_huff_dc_symbols_ok(values[tb], total)) return "a DC Huffman symbol above 11";
        present[tb] = 1;
        i += 17 + total;
    }
    return nullptr;
}

// ---- parse (pure host) ----
// SOI .. SOS into `in`; returns nullptr, or the reason the stream is refused.
// layouts (the header's JPEG DECODER, LAYOUTS): the luma samplings 1x2, 4x1 and 4x2 are frames too, and so is a SOF1 frame that
// is a baseline one but for its marker (8 bit, one interleaved scan, Huffman ids 0..1).  Without it every text is the one it was.
inline const char* jpeg_parse(const uint8_t* d, int64_t size, whenet_jpeg_info_t& in, bool layouts = false) {
    std::memset(&in, 0, sizeof(in));
    if (size > JPEG_DEC_MAX_BYTES) return "a stream above 2^31 - 1 bytes";
    if (size < 4 || d[0] != 0xFF || d[1] != 0xD8) return "no SOI marker at the start: not a JPEG stream";
    int64_t p = 2;
    bool sof = false;
    int comp_id[3] = {0, 0, 0};
    for (;;) {
        int m, n;
        const uint8_t* s;
        const char* bad = jpeg_next_segment(d, size, false, p, m, s, n);
        if (bad != nullptr) return bad;
        if (m == 0xC2) return "progressive DCT (SOF2): baseline sequential streams only";
        if (m == 0xC1 && !layouts) return "extended sequential DCT (SOF1): baseline sequential streams only";
        if (m == 0xC3 || (m >= 0xC5 && m <= 0xC7)) return "a lossless, differential or hierarchical frame (SOF3, SOF5-7): baseline only";
        if (m == 0xCC || (m >= 0xC9 && m <= 0xCB) || (m >= 0xCD && m <= 0xCF)) return "arithmetic coding (SOF9-15, DAC): Huffman streams only";
        if (m == 0xC8) return "a reserved marker (JPG)";
        if (m == 0xC0 || m == 0xC1) {
            if (sof) return "a second SOF0";
            bad = jpeg_read_sof(s, n, false, in, comp_id, layouts);
            sof = true;
        } else if (m == 0xDB) {
            bad = jpeg_read_dqt(s, n, in);
        } else if (m == 0xC4) {
            bad = jpeg_read_dht(s, n, 1, in.huff_counts, in.huff_values, in.huff_present);
        } else if (m == 0xDD) {
            if (n != 2) return "a DRI of the wrong length";
            in.restart_interval = (s[0] << 8) | s[1];
        } else if (m == 0xDA) {
            if (!sof) return "SOS before SOF0";
            if (n < 1) return "a short SOS";
            const int ns = s[0];
            if (ns != in.components) return "several scans (a scan that does not hold every component): one interleaved scan only";
            if (n != 4 + 2 * ns) return "the length of SOS does not match its components";
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != comp_id[c]) return "the scan's components are not the frame's, in order";
                const int td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
                if (td > 1 || ta > 1) return "a Huffman table id above 1";
                in.dc[c] = td, in.ac[c] = ta;
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return "a spectral selection or successive approximation: baseline only";
            for (int c = 0; c < ns; ++c) {
                if (!in.q_present[in.qt[c]]) return "a missing quantiser table (DQT)";
                if (!in.huff_present[2 * in.dc[c]] || !in.huff_present[2 * in.ac[c] + 1]) return "a missing Huffman table (DHT)";
            }
            in.data_offset = p;
            in.intervals = jpeg_dec_geom(in).intervals;
            return nullptr;
        } else if (!((m >= 0xE0 && m <= 0xEF) || m == 0xFE)) {      // (APPn, COM: skipped)
            return "an unexpected marker in the header";
        }
        if (bad != nullptr) return bad;
    }
}

// ---- default Huffman tables (pure host; include/whenet_hip.h, JPEG DECODER, DEFAULT TABLES) ----
// MJPG frames of UVC cameras and of many AVI writers carry no DHT: their tables are T.81's Annex K ones, which every player installs
// (libjpeg's std_huff_tables).  This copies the stream to `out` with ONE DHT segment directly in front of the first SOS marker that
// holds, in the order DC 0, AC 0, DC 1, AC 1, the Annex K table (jpeg_host.h: K.3 / K.5 for id 0, K.4 / K.6 for id 1) of every one
// of these four slots that no DHT in front of that SOS defines: at most JPEG_DEFAULT_TABLES_MAX bytes more.  A stream that defines
// all four, and a header the walker cannot follow to an SOS (no SOI, a truncated or malformed segment, a DHT jpeg_read_dht
// refuses), is copied byte for byte: this never refuses a stream, the decoder gives its own reason.  Ids 2 and 3 are never filled.
// `out` has room for size + JPEG_DEFAULT_TABLES_MAX bytes; returns the bytes written.  Every byte is read inside [0, size).
constexpr int JPEG_DEFAULT_TABLES_MAX = 4 + 4 * 17 + 12 + 162 + 12 + 162;      // 420
inline int64_t jpeg_add_default_tables(const uint8_t* d, int64_t size, uint8_t* out) {
    int64_t sos = -1;                                   // where the first SOS marker stands
    uint8_t present[8] = {};
    if (size <= JPEG_DEC_MAX_BYTES && size >= 4 && d[0] == 0xFF && d[1] == 0xD8) {
        std::vector<uint8_t> scratch(8 * (16 + 256));   // (jpeg_read_dht writes the tables it reads somewhere)
        uint8_t(*counts)[16] = reinterpret_cast<uint8_t(*)[16]>(scratch.data());
        uint8_t(*values)[256] = reinterpret_cast<uint8_t(*)[256]>(scratch.data() + 8 * 16);
        for (int64_t p = 2;;) {
            int m, n;
            const uint8_t* s;
            if (jpeg_next_segment(d, size, false, p, m, s, n) != nullptr) break;
            if (m == 0xC4 && jpeg_read_dht(s, n, 3, counts, values, present) != nullptr) break;
            if (m == 0xDA) {
                sos = p - n - 4;
                break;
            }
        }
    }
    const bool missing = sos >= 0 && !(present[0] && present[1] && present[2] && present[3]);
    if (!missing) {
        if (size > 0) std::memcpy(out, d, size_t(size));
        return size;
    }
    std::memcpy(out, d, size_t(sos));
    uint8_t* q = out + sos;
    uint8_t* const seg = q;
    q += 4;
    for (int t = 0; t < 4; ++t) {                       // index 2 id + class: DC 0, AC 0, DC 1, AC 1
        if (present[t]) continue;
        *q++ = uint8_t(((t & 1) << 4) | (t >> 1));
        std::memcpy(q, JPEG_HUFF_BITS[t], 16), q += 16;
        std::memcpy(q, JPEG_HUFF_VALS[t], size_t(JPEG_HUFF_COUNT[t])), q += JPEG_HUFF_COUNT[t];
    }
    const int len = int(q - seg) - 2;
    seg[0] = 0xFF, seg[1] = 0xC4, seg[2] = uint8_t(len >> 8), seg[3] = uint8_t(len & 255);
    std::memcpy(q, d + sos, size_t(size - sos));
    return int64_t(q - out) + (size - sos);
}

// ---- EXIF orientation (pure host; include/whenet_hip.h, JPEG DECODER, ORIENTATION) ----
// The orientation tag (0x0112) of a stream, 1..8: from IFD0 of the FIRST APP1 segment in front of SOS whose payload starts with
// "Exif\0\0" (an XMP APP1 in front of it is passed, a second Exif APP1 is never read), count 1, type SHORT or LONG, either byte
// order.  Anything else -- no such segment, a bad TIFF header, an offset, an entry count or an entry that leaves the segment, another
// type or count, a value outside 1..8 -- is 1: broken EXIF never refuses a stream.  Every byte is read inside [0, size).
inline int jpeg_exif_orientation(const uint8_t* d, int64_t size) {
    if (d == nullptr || size < 4 || size > JPEG_DEC_MAX_BYTES || d[0] != 0xFF || d[1] != 0xD8) return 1;
    int64_t p = 2;
    for (;;) {
        int m, n;
        const uint8_t* s;
        if (jpeg_next_segment(d, size, false, p, m, s, n) != nullptr || m == 0xDA) return 1;
        if (m != 0xE1 || n < 6 || std::memcmp(s, "Exif\0\0", 6) != 0) continue;
        const uint8_t* const t = s + 6;      // the TIFF header: offsets count from here
        const int64_t tn = n - 6;
        if (tn < 8) return 1;
        const bool le = t[0] == 'I' && t[1] == 'I';
        if (!le && !(t[0] == 'M' && t[1] == 'M')) return 1;
        const auto rd16 = [&](int64_t at) { return le ? int64_t(t[at]) | int64_t(t[at + 1]) << 8 : int64_t(t[at]) << 8 | int64_t(t[at + 1]); };
        const auto rd32 = [&](int64_t at) { return le ? rd16(at) | rd16(at + 2) << 16 : rd16(at) << 16 | rd16(at + 2); };
        if (rd16(2) != 42) return 1;
        const int64_t ifd = rd32(4);
        if (ifd > tn - 2) return 1;
        const int64_t entries = rd16(ifd);
        if (ifd + 2 + 12 * entries > tn) return 1;
        for (int64_t e = ifd + 2; e < ifd + 2 + 12 * entries; e += 12) {
            if (rd16(e) != 0x0112) continue;
            const int64_t type = rd16(e + 2), count = rd32(e + 4);
            if (count != 1 || (type != 3 && type != 4)) return 1;
            const int64_t v = type == 3 ? rd16(e + 8) : rd32(e + 8);
            return v >= 1 && v <= 8 ? int(v) : 1;
        }
        return 1;
    }
}

// The oriented frame D of an upright frame u [h][w] (the EXIF standard's eight values; 5..8 turn rows into columns: D is w x h):
// D[Y][X] = u[y][x].  Host and device.
WHENET_HD inline bool jpeg_orient_ok(long long o) { return o >= 1 && o <= 8; }
WHENET_HD inline int jpeg_orient_h(int o, int h, int w) { return o >= 5 ? w : h; }
WHENET_HD inline int jpeg_orient_w(int o, int h, int w) { return o >= 5 ? h : w; }
WHENET_HD inline bool jpeg_orient_flip_x(int o) { return o == 2 || o == 3 || o == 7 || o == 8; }      // x runs against its destination axis
WHENET_HD inline bool jpeg_orient_flip_y(int o) { return o == 3 || o == 4 || o == 6 || o == 7; }
WHENET_HD inline void jpeg_orient_source(int o, int h, int w, int Y, int X, int& y, int& x) {
    const int sy = o >= 5 ? X : Y, sx = o >= 5 ? Y : X;
    y = jpeg_orient_flip_y(o) ? h - 1 - sy : sy, x = jpeg_orient_flip_x(o) ? w - 1 - sx : sx;
}
// the header of a stream as the oriented frame's: the sides swapped for 5..8 (what a destination is checked and sized against)
inline whenet_jpeg_info_t jpeg_orient_info(const whenet_jpeg_info_t& in, int o) {
    whenet_jpeg_info_t out = in;
    out.h = jpeg_orient_h(o, in.h, in.w), out.w = jpeg_orient_w(o, in.h, in.w);
    return out;
}

// What a whenet_jpeg_info_t must satisfy before anything is computed from it (the parser's own output does; a caller of
// whenet_jpeg_decode_device may have filled one by hand): a text, or nullptr
inline const char* jpeg_dec_check_info(const whenet_jpeg_info_t& in, bool layouts = false) {
    if (in.h < 1 || in.w < 1 || in.h > JPEG_MAX_SIDE || in.w > JPEG_MAX_SIDE) return "frame sides must be 1..8192";
    if (in.components != 1 && in.components != 3) return "the frame must have 1 or 3 components";
    if (in.components == 3 && !jpeg_dec_sampling_ok(in.hs, in.vs, layouts))
        return layouts ? "luma sampling factors other than hs 1, 2 or 4 by vs 1 or 2" : "luma sampling must be 2x2 (4:2:0), 2x1 (4:2:2) or 1x1 (4:4:4)";
    if (in.restart_interval < 0 || in.restart_interval > 65535) return "a restart interval outside 0..65535";
    for (int c = 0; c < in.components; ++c) {
        if (in.qt[c] < 0 || in.qt[c] > 3 || in.dc[c] < 0 || in.dc[c] > 1 || in.ac[c] < 0 || in.ac[c] > 1) return "a table id out of range";
        if (!in.q_present[in.qt[c]]) return "a missing quantiser table (DQT)";
        if (!in.huff_present[2 * in.dc[c]] || !in.huff_present[2 * in.ac[c] + 1]) return "a missing Huffman table (DHT)";
    }
    for (int tb = 0; tb < 4; ++tb) {
        if (!in.huff_present[tb]) continue;
        const int total = jpeg_huff_symbols(in.huff_counts[tb]);
        if (total < 0) return "a Huffman table whose code lengths are no prefix code";
        if (total > 256) return "a Huffman table of more than 256 symbols";
        if ((tb & 1) == 0 && !jpeg_huff_dc_symbols_ok(in.huff_values[tb], total)) return "a DC Huffman symbol above 11";
    }
    if (in.intervals != jpeg_dec_geom(in).intervals) return "the interval count is not that of the size, the sampling and the restart interval";
    return nullptr;
}

// ---- decode tables (pure host) ----
// One table as the decoder reads it, from the 16 counts and the symbols of its DHT
inline void jpeg_dec_build_huff(const uint8_t counts[16], const uint8_t values[256], JpegDecHuff& h) {
    std::memset(&h, 0, sizeof(h));
    std::memcpy(h.vals, values, 256);
    unsigned code = 0;
    int n = 0;
    for (int l = 1; l <= 16; ++l) {
        const int cnt = counts[l - 1];
        h.valoff[l] = n - int(code);
        h.maxcode[l] = cnt > 0 ? int(code) + cnt - 1 : -1;
        for (int i = 0; i < cnt; ++i, ++n, ++code)
            if (l <= JPEG_DEC_LOOK_BITS) {
                const int first = int(code) << (JPEG_DEC_LOOK_BITS - l);
                for (int j = 0; j < (1 << (JPEG_DEC_LOOK_BITS - l)); ++j) h.look[first + j] = uint16_t((l << 8) | h.vals[n]);
            }
        code <<= 1;
    }
    h.maxcode[0] = -1, h.valoff[0] = 0;
}

inline void jpeg_dec_build_tables(const whenet_jpeg_info_t& in, JpegDecTables& t) {
    static const uint8_t no_codes[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};      // an absent table
    std::memset(&t, 0, sizeof(t));
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 64; ++k) t.q[i][k] = int16_t(in.q[i][k]);
    for (int k = 0; k < 64; ++k) t.zz[k] = JPEG_ZIGZAG[k];
    for (int tb = 0; tb < 4; ++tb) jpeg_dec_build_huff(in.huff_present[tb] ? in.huff_counts[tb] : no_codes, in.huff_values[tb], t.huff[tb]);
}

// ---- the bit reader (host and device) ----
// The bits of one restart interval, most significant first.  0xFF 0x00 yields one 0xFF byte; any other byte behind 0xFF is a
// marker, and there, or at the end of the data, the reader stops for good.  EVERY byte it fetches is checked against `end`.
struct JpegBitReader {
    const uint8_t* d;
    int pos, end;
    uint32_t acc;      // the low n bits are the next n bits
    int n;
    bool stop;
    // a window of 16 bytes of the data in registers, so that a byte costs a memory access once in sixteen: the aligned 16 bytes
    // around a position are loaded only where ALL of them lie inside [0, end); elsewhere the byte is fetched on its own
    uint64_t win_lo, win_hi;
    int win_pos;       // the position of the window's first byte (-16: none)
    WHENET_HD JpegBitReader(const uint8_t* data, int from, int size)
        : d(data), pos(from), end(size), acc(0), n(0), stop(false), win_lo(0), win_hi(0), win_pos(-16) {}
    // byte p of the data; the caller has checked 0 <= p < end
    WHENET_HD uint32_t byte_at(int p) {
        const int off = int(reinterpret_cast<uintptr_t>(d + p) & 15u);
        const int first = p - off;
        if (first != win_pos) {
            if (first < 0 || first + 16 > end) return d[p];
            uint64_t w[2];
            std::memcpy(w, __builtin_assume_aligned(d + first, 16), 16);      // (one 16-byte load)
            win_lo = w[0], win_hi = w[1], win_pos = first;
        }
        return uint32_t((off < 8 ? win_lo >> (8 * off) : win_hi >> (8 * (off - 8))) & 255u);
    }
    WHENET_HD void fill() {
        while (n <= 24 && !stop) {
            if (pos >= end) {
                stop = true;
                break;
            }
            const uint32_t b = byte_at(pos);
            if (b == 0xFFu) {
                if (pos + 1 >= end || byte_at(pos + 1) != 0) {
                    stop = true;
                    break;
                }
                pos += 2;
            } else {
                ++pos;
            }
            acc = (acc << 8) | b, n += 8;
        }
    }
    // the next k <= 16 bits, zeros where the data has ended
    WHENET_HD uint32_t peek(int k) const { return (n >= k ? acc >> (n - k) : acc << (k - n)) & ((1u << k) - 1u); }
    // one Huffman symbol, or -1: no code word, or the data ends inside it
    WHENET_HD int decode(const JpegDecHuff& h) {
        fill();
        const uint32_t e = h.look[peek(JPEG_DEC_LOOK_BITS)];
        int l = int(e >> 8);
        if (l != 0) {
            if (l > n) return -1;
            n -= l;
            return int(e & 255u);
        }
        for (l = JPEG_DEC_LOOK_BITS + 1; l <= 16; ++l) {
            if (l > n) return -1;
            const int code = int(peek(l));
            if (code <= h.maxcode[l]) {
                n -= l;
                return h.vals[(h.valoff[l] + code) & 255];
            }
        }
        return -1;
    }
    // s <= 15 extra bits as a value (T.81 F.2.2.1 EXTEND); false: the data ends inside them
    WHENET_HD bool receive(int s, int& v) {
        v = 0;
        if (s == 0) return true;
        fill();
        if (s > n) return false;
        v = int((acc >> (n - s)) & ((1u << s) - 1u));
        n -= s;
        if (v < (1 << (s - 1))) v -= (1 << s) - 1;
        return true;
    }
};

WHENET_HD inline int jpeg_dec_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One block: its dequantised coefficients, clamped to -2048..2047, into out[64] in natural order (out is zero on entry; only the
// non-zero ones are written).  pred: the component's DC predictor, kept inside -32768..32767.  false: the data is damaged; what
// was written before stays.
WHENET_HD inline bool jpeg_dec_block(JpegBitReader& br, const JpegDecHuff& dc, const JpegDecHuff& ac, const int16_t* q, const uint8_t* zz, int& pred, int16_t* out) {
    int s = br.decode(dc), v;
    if (s < 0 || !br.receive(s & 15, v)) return false;
    pred = jpeg_dec_clamp(pred + v, -32768, 32767);
    out[0] = int16_t(jpeg_dec_clamp(pred * int(q[0]), -2048, 2047));
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
        if (k > 63 || !br.receive(s, v)) return false;
        const int nat = zz[k];
        out[nat] = int16_t(jpeg_dec_clamp(v * int(q[nat]), -2048, 2047));
        ++k;
    }
    return true;
}

// The interval's MCUs into coef (zeroed, [blocks][64]); returns false where the data is damaged: the block in hand keeps what was
// decoded of it, the blocks behind it stay zero
// (coef's first record is MCU mcu_base's first block.  stage: nullptr, or 64 int16 of fast memory, 16-byte aligned like coef: a
// block is then decoded there and leaves as eight 16-byte stores, so that the walk itself issues no store it would have to wait for)
WHENET_HD inline bool jpeg_dec_interval(const uint8_t* data, int size, int from, const JpegDecTables& t, const JpegDecGeom& g, int interval,
                                        int16_t* coef, long long mcu_base, int16_t* stage = nullptr) {
    JpegBitReader br(data, from, size);
    int pred[3] = {0, 0, 0};
    const long long mcus = (long long)(g.mcu_cols) * g.mcu_rows;
    const long long first = (long long)(interval) * g.ri;
    const long long last = first + g.ri < mcus ? first + g.ri : mcus;
    const int ny = g.bpm - 2;
    for (long long m = first; m < last; ++m)
        for (int b = 0; b < g.bpm; ++b) {
            const int c = g.comps == 1 || b < ny ? 0 : b - ny + 1;
            int16_t* const rec = coef + (size_t(m - mcu_base) * size_t(g.bpm) + size_t(b)) * 64;
            if (stage != nullptr) std::memset(__builtin_assume_aligned(stage, 16), 0, 128);
            const bool ok = jpeg_dec_block(br, t.huff[g.dc[c]], t.huff[g.ac[c]], t.q[g.qt[c]], t.zz, pred[c], stage != nullptr ? stage : rec);
            if (stage != nullptr) std::memcpy(__builtin_assume_aligned(rec, 16), __builtin_assume_aligned(stage, 16), 128);
            if (!ok) return false;
        }
    return true;
}

// ---- inverse DCT ----
// out[y] = sum_v T[v][y] in[v]: one pass of the inverse DCT over 8 values
WHENET_HD inline void jpeg_idct8(const int in[8], int out[8]) {
    constexpr int T[8][8] = WHENET_JPEG_DCT;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int y = 0; y < 8; ++y) {
        int a = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int v = 0; v < 8; ++v) a += T[v][y] * in[v];
        out[y] = a;
    }
}
WHENET_HD inline int jpeg_idct_round(int a) { return (a + 128) >> 8; }
WHENET_HD inline int jpeg_idct_sample(int b) { return jpeg_dec_clamp(((b + 32768) >> 16) + 128, 0, 255); }

// where block b of MCU m lies: its component and its first sample on the component's (padded) plane
WHENET_HD inline void jpeg_dec_block_origin(const JpegDecGeom& g, long long m, int b, int& comp, int& y0, int& x0) {
    const int my = int(m / g.mcu_cols), mx = int(m - (long long)(my) * g.mcu_cols);
    const int ny = g.bpm - 2;
    if (g.comps == 1 || b < ny) {
        comp = 0;
        y0 = (my * g.vs + (g.comps == 1 ? 0 : b / g.hs)) * 8, x0 = (mx * g.hs + (g.comps == 1 ? 0 : b % g.hs)) * 8;
    } else {
        comp = b - ny + 1, y0 = my * 8, x0 = mx * 8;
    }
}

// ---- planes -> pixel ----
// B, G, R of a pixel from its samples: the JFIF row of the YUV ingest
WHENET_HD inline void jpeg_dec_pixel(int y, int u, int v, int& b, int& g, int& r) {
    constexpr int K[WHENET_YUV_MATRICES][6] = WHENET_YUV_COEFFS;      // yoff, CY, CVR, CUG, CVG, CUB
    const int c = y - K[WHENET_YUV_JFIF][0] < 0 ? 0 : y - K[WHENET_YUV_JFIF][0], d = u - 128, e = v - 128;
    const int base = K[WHENET_YUV_JFIF][1] * c + (1 << 19);
    r = jpeg_dec_clamp((base + K[WHENET_YUV_JFIF][2] * e) >> 20, 0, 255);
    g = jpeg_dec_clamp((base - K[WHENET_YUV_JFIF][3] * d - K[WHENET_YUV_JFIF][4] * e) >> 20, 0, 255);
    b = jpeg_dec_clamp((base + K[WHENET_YUV_JFIF][5] * d) >> 20, 0, 255);
}

// ---- rule 1: libjpeg's bytes (include/whenet_hip.h, JPEG DECODER, RULE 1) ----
constexpr int JPEG_RULE_OWN = 0, JPEG_RULE_LIBJPEG = 1;
inline bool jpeg_rule_ok(long long v) { return v == JPEG_RULE_OWN || v == JPEG_RULE_LIBJPEG; }

// One 8-point pass of jidctint's inverse DCT (13 constant bits), exact integer arithmetic in T, outputs before the descale.  The
// pass is linear: out[k] = sum_j C[j][k] in[j], and the columns of |C| sum to at most 61,214.  Pass 1 (|in| <= 2048): |out| <=
// 1.26e8 and every intermediate below 3.5e8, T = int32.  Its descaled results are at most 61,214 in size, so pass 2 reaches
// 61,214^2 = 3.75e9 > 2^31: T = int64 there, on the host and in the kernel alike.
template <class T>
WHENET_HD inline void jpeg_idct8_islow(const T i[8], T out[8]) {
    T z1 = (i[2] + i[6]) * 4433;
    const T t2 = z1 - i[6] * 15137, t3 = z1 + i[2] * 6270;
    const T t0 = (i[0] + i[4]) * 8192, t1 = (i[0] - i[4]) * 8192;      // (<< 13 of a value that may be negative)
    const T t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    T a0 = i[7], a1 = i[5], a2 = i[3], a3 = i[1];
    z1 = a0 + a3;
    T z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const T z5 = (z3 + z4) * 9633;
    a0 *= 2446, a1 *= 16819, a2 *= 25172, a3 *= 12299;
    z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    a0 += z1 + z3, a1 += z2 + z4, a2 += z2 + z3, a3 += z1 + z4;
    out[0] = t10 + a3, out[1] = t11 + a2, out[2] = t12 + a1, out[3] = t13 + a0;
    out[4] = t13 - a0, out[5] = t12 - a1, out[6] = t11 - a2, out[7] = t10 - a3;
}
WHENET_HD inline int jpeg_islow_round1(int a) { return (a + 1024) >> 11; }
WHENET_HD inline int jpeg_islow_sample(long long b) {
    const long long v = ((b + 131072) >> 18) + 128;
    return int(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// Fancy upsampling (jdsample.c).  A chroma column's value is the sample itself (4:2:2) or 3 x the row's + the vertical neighbour's
// (4:2:0: v2); a pixel takes 3 x its own column + the horizontal neighbour's: the left one for even x, the right one for odd x.
WHENET_HD inline int jpeg_fancy_col(int own_row, int other_row, bool v2) { return v2 ? 3 * own_row + other_row : own_row; }
WHENET_HD inline int jpeg_fancy_up(int own, int other, bool odd, bool v2) {
    return v2 ? (3 * own + other + (odd ? 7 : 8)) >> 4 : (3 * own + other + (odd ? 2 : 1)) >> 2;
}
// 4:4:0 (h1v2_fancy_upsample): a pixel takes 3 x its own chroma row + the vertical neighbour's, the row above for even y (bias 1),
// the row below for odd y (bias 2); no horizontal filter and no narrow-width switch
WHENET_HD inline int jpeg_fancy_v(int own_row, int other_row, bool odd) { return (3 * own_row + other_row + (odd ? 2 : 1)) >> 2; }
// B, G, R of a pixel by jdcolor.c's tables: F(x) = int(x 65536 + 0.5)
WHENET_HD inline void jpeg_ycc_pixel(int y, int u, int v, int& b, int& g, int& r) {
    const int d = u - 128, e = v - 128;
    r = jpeg_dec_clamp(y + ((91881 * e + 32768) >> 16), 0, 255);
    b = jpeg_dec_clamp(y + ((116130 * d + 32768) >> 16), 0, 255);
    g = jpeg_dec_clamp(y + ((-22554 * d + 32768 - 46802 * e) >> 16), 0, 255);
}

// a block's 64 records -> its 8 x 8 samples by the rule's two passes (the statement the idct kernels are held to)
inline void jpeg_dec_block_samples(const int16_t* cf, int rule, uint8_t s[8][8]) {
    if (rule == JPEG_RULE_LIBJPEG) {
        int r[8][8];
        for (int u = 0; u < 8; ++u) {
            int col[8], a[8];
            for (int v = 0; v < 8; ++v) col[v] = cf[v * 8 + u];
            jpeg_idct8_islow<int>(col, a);
            for (int y = 0; y < 8; ++y) r[y][u] = jpeg_islow_round1(a[y]);
        }
        for (int y = 0; y < 8; ++y) {
            long long row[8], bb[8];
            for (int u = 0; u < 8; ++u) row[u] = r[y][u];
            jpeg_idct8_islow<long long>(row, bb);
            for (int x = 0; x < 8; ++x) s[y][x] = uint8_t(jpeg_islow_sample(bb[x]));
        }
        return;
    }
    int r[8][8];
    for (int u = 0; u < 8; ++u) {
        int col[8], a[8];
        for (int v = 0; v < 8; ++v) col[v] = cf[v * 8 + u];
        jpeg_idct8(col, a);
        for (int y = 0; y < 8; ++y) r[y][u] = jpeg_idct_round(a[y]);
    }
    for (int y = 0; y < 8; ++y) {
        int bb[8];
        jpeg_idct8(r[y], bb);
        for (int x = 0; x < 8; ++x) s[y][x] = uint8_t(jpeg_idct_sample(bb[x]));
    }
}

// ---- the host statement ----
// The restart markers of the entropy data (0xFF 0xD0..0xD7 pairs, in order): start[i] = where interval i's bits begin, for every
// interval that has a start; returns the first interval the markers make bad, or JPEG_DEC_NO_BAD: marker k must be RST(k mod 8)
// and there must be intervals - 1 of them.  Intervals behind the bad one are not decoded.
inline int jpeg_dec_scan_host(const uint8_t* data, int size, int intervals, std::vector<int32_t>& start) {
    start.assign(size_t(intervals), 0);
    int bad = JPEG_DEC_NO_BAD, k = 0;
    for (int p = 0; p + 1 < size; ++p) {
        if (data[p] != 0xFF || data[p + 1] < 0xD0 || data[p + 1] > 0xD7) continue;
        if (k >= intervals - 1) {
            if (intervals - 1 < bad) bad = intervals - 1;
        } else if ((data[p + 1] & 7) != (k & 7)) {
            if (k < bad) bad = k;
        }
        if (k + 1 < intervals) start[size_t(k) + 1] = p + 2;
        ++k;
    }
    if (k < intervals - 1 && k < bad) bad = k;
    return bad;
}

struct JpegDecPlanes {
    std::vector<uint8_t> plane[3];
};

// entropy data -> the padded component planes; status[0] = WHENET_OK or WHENET_EFORMAT, status[1] = the first bad interval or -1
inline void jpeg_dec_planes_host(const whenet_jpeg_info_t& in, const uint8_t* data, int size, JpegDecPlanes& out, int32_t status[2],
                                 int rule = JPEG_RULE_OWN) {
    const JpegDecGeom g = jpeg_dec_geom(in);
    std::vector<JpegDecTables> tables(1);
    jpeg_dec_build_tables(in, tables[0]);
    std::vector<int32_t> start;
    const int scan_bad = jpeg_dec_scan_host(data, size, g.intervals, start);
    int bad = scan_bad;
    for (int c = 0; c < g.comps; ++c) out.plane[c].assign(size_t(g.plane_pitch[c]) * size_t(g.plane_rows[c]), 0);
    const size_t interval_blocks = size_t(g.ri) * size_t(g.bpm);
    std::vector<int16_t> coef(interval_blocks * 64);
    alignas(16) int16_t stage[64];      // (the staged form of the walk, as the kernel runs it)
    const long long mcus = (long long)(g.mcu_cols) * g.mcu_rows;
    for (int i = 0; i < g.intervals; ++i) {
        std::fill(coef.begin(), coef.end(), int16_t(0));
        const long long first = (long long)(i) * g.ri;
        const long long count = first + g.ri < mcus ? g.ri : mcus - first;
        if (i <= scan_bad && !jpeg_dec_interval(data, size, start[size_t(i)], tables[0], g, i, coef.data(), first, stage))
            if (i < bad) bad = i;
        for (long long m = 0; m < count; ++m)
            for (int b = 0; b < g.bpm; ++b) {
                const int16_t* cf = coef.data() + (size_t(m) * size_t(g.bpm) + size_t(b)) * 64;
                int comp, y0, x0;
                uint8_t smp[8][8];
                jpeg_dec_block_origin(g, first + m, b, comp, y0, x0);
                jpeg_dec_block_samples(cf, rule, smp);
                uint8_t* dst = out.plane[comp].data() + size_t(y0) * size_t(g.plane_pitch[comp]) + size_t(x0);
                for (int y = 0; y < 8; ++y) std::memcpy(dst + size_t(y) * size_t(g.plane_pitch[comp]), smp[y], 8);
            }
    }
    status[0] = bad == JPEG_DEC_NO_BAD ? WHENET_OK : WHENET_EFORMAT;
    status[1] = bad == JPEG_DEC_NO_BAD ? -1 : bad;
}

// Argument errors of a decode destination, as a text (nullptr: none)
inline const char* jpeg_dec_check_dst(const whenet_jpeg_info_t& in, const whenet_surface_t* dst, int channel_order, int rule = JPEG_RULE_OWN) {
    if (dst == nullptr) return "NULL argument";
    if (!jpeg_rule_ok(rule)) return "the rule must be 0 (the project's own) or 1 (libjpeg)";
    int rows[3], row_bytes[3];
    const int planes = overlay_surface_planes(dst->format, in.h, in.w, rows, row_bytes);
    if (planes == 0) return "unknown surface format (WHENET_SURF_PACKED, WHENET_YUV_NV12 or WHENET_YUV_I420)";
    if (dst->format == WHENET_SURF_PACKED) {
        if (channel_order != WHENET_RGB && channel_order != WHENET_BGR) return "unknown channel order";
    } else {
        if (rule == JPEG_RULE_LIBJPEG) return "rule 1 (libjpeg) decodes to WHENET_SURF_PACKED only";
        if (in.components != 3 || in.hs != 2 || in.vs != 2) return "only a 4:2:0 stream decodes into an I420 or NV12 surface";
        if (dst->matrix != WHENET_YUV_JFIF) return "a YUV destination must have the matrix WHENET_YUV_JFIF (JFIF is full-range BT.601)";
    }
    for (int p = 0; p < planes; ++p) {
        if (dst->plane[p] == nullptr) return "a plane of the surface is NULL";
        if (dst->pitch[p] < row_bytes[p]) return "a pitch of the surface is below its row bytes";
    }
    return nullptr;
}

// the padded planes -> the destination surface (host memory)
// (rule 1: a packed destination only, jpeg_dec_check_dst; the chroma planes' rows >= ch and columns >= cw are never read)
inline void jpeg_dec_frame_host(const JpegDecGeom& g, const JpegDecPlanes& pl, const whenet_surface_t& dst, int channel_order,
                                int rule = JPEG_RULE_OWN) {
    const int hsh = jpeg_dec_shift(g.hs), vsh = jpeg_dec_shift(g.vs);
    if (dst.format == WHENET_SURF_PACKED && rule == JPEG_RULE_LIBJPEG) {
        const int ri = channel_order == WHENET_BGR ? 2 : 0;
        const int ch = (g.h + g.vs - 1) / g.vs, cw = (g.w + g.hs - 1) / g.hs;
        // hs = 2: the triangle filter (libjpeg's own switch to replication at cw <= 2); hs = 1, vs = 2 (4:4:0): the vertical filter
        // alone, at every width; hs = 4 (4:1:1, 4:1:0): replication in both directions (int_upsample)
        const bool fancy = g.comps == 3 && g.hs == 2 && cw > 2, v2 = g.vs == 2 && g.hs != 4, fancy_v = g.comps == 3 && g.hs == 1 && g.vs == 2;
        for (int y = 0; y < g.h; ++y) {
            uint8_t* o = static_cast<uint8_t*>(dst.plane[0]) + size_t(y) * size_t(dst.pitch[0]);
            const uint8_t* yr = pl.plane[0].data() + size_t(y) * size_t(g.plane_pitch[0]);
            const int cr = y >> vsh, cn = v2 ? jpeg_dec_clamp(cr + ((y & 1) ? 1 : -1), 0, ch - 1) : cr;
            for (int x = 0; x < g.w; ++x) {
                int b, gg, r;
                if (g.comps == 1) {
                    b = gg = r = yr[x];
                } else {
                    int uv[2];
                    for (int c = 1; c < 3; ++c) {
                        const uint8_t* row = pl.plane[c].data() + size_t(cr) * size_t(g.plane_pitch[c]);
                        const uint8_t* other = pl.plane[c].data() + size_t(cn) * size_t(g.plane_pitch[c]);
                        if (fancy_v) {
                            uv[c - 1] = jpeg_fancy_v(row[x], other[x], (y & 1) != 0);
                        } else if (fancy) {
                            const int i = x >> 1, n = jpeg_dec_clamp(i + ((x & 1) ? 1 : -1), 0, cw - 1);
                            uv[c - 1] = jpeg_fancy_up(jpeg_fancy_col(row[i], other[i], v2), jpeg_fancy_col(row[n], other[n], v2), (x & 1) != 0, v2);
                        } else {
                            uv[c - 1] = row[x >> hsh];
                        }
                    }
                    jpeg_ycc_pixel(yr[x], uv[0], uv[1], b, gg, r);
                }
                o[3 * x + ri] = uint8_t(r), o[3 * x + 1] = uint8_t(gg), o[3 * x + 2 - ri] = uint8_t(b);
            }
        }
        return;
    }
    if (dst.format == WHENET_SURF_PACKED) {
        const int ri = channel_order == WHENET_BGR ? 2 : 0;
        for (int y = 0; y < g.h; ++y) {
            uint8_t* o = static_cast<uint8_t*>(dst.plane[0]) + size_t(y) * size_t(dst.pitch[0]);
            const uint8_t* yr = pl.plane[0].data() + size_t(y) * size_t(g.plane_pitch[0]);
            for (int x = 0; x < g.w; ++x) {
                int b, gg, r;
                if (g.comps == 1) {
                    b = gg = r = yr[x];
                } else {
                    const size_t ci = size_t(y >> vsh) * size_t(g.plane_pitch[1]) + size_t(x >> hsh);
                    jpeg_dec_pixel(yr[x], pl.plane[1][ci], pl.plane[2][ci], b, gg, r);
                }
                o[3 * x + ri] = uint8_t(r), o[3 * x + 1] = uint8_t(gg), o[3 * x + 2 - ri] = uint8_t(b);
            }
        }
        return;
    }
    const int ch = (g.h + 1) >> 1, cw = (g.w + 1) >> 1;
    for (int y = 0; y < g.h; ++y)
        std::memcpy(static_cast<uint8_t*>(dst.plane[0]) + size_t(y) * size_t(dst.pitch[0]), pl.plane[0].data() + size_t(y) * size_t(g.plane_pitch[0]),
                    size_t(g.w));
    for (int y = 0; y < ch; ++y)
        for (int c = 1; c < 3; ++c) {
            const uint8_t* s = pl.plane[c].data() + size_t(y) * size_t(g.plane_pitch[c]);
            if (dst.format == WHENET_YUV_I420) {
                std::memcpy(static_cast<uint8_t*>(dst.plane[c]) + size_t(y) * size_t(dst.pitch[c]), s, size_t(cw));
            } else {
                uint8_t* o = static_cast<uint8_t*>(dst.plane[1]) + size_t(y) * size_t(dst.pitch[1]) + size_t(c - 1);
                for (int x = 0; x < cw; ++x) o[2 * x] = s[x];
            }
        }
}

// the padded planes -> the ORIENTED frame in a packed destination of jpeg_orient_h x jpeg_orient_w pixels: the table of
// jpeg_orient_source applied to the upright frame of the same rule (the statement the oriented frame kernels are held to)
inline void jpeg_dec_frame_oriented_host(const JpegDecGeom& g, const JpegDecPlanes& pl, const whenet_surface_t& dst, int channel_order, int rule,
                                         int orient) {
    if (orient <= 1) return jpeg_dec_frame_host(g, pl, dst, channel_order, rule);
    std::vector<uint8_t> up(size_t(g.h) * size_t(g.w) * 3);
    whenet_surface_t u{};
    u.plane[0] = up.data(), u.pitch[0] = 3 * g.w, u.format = WHENET_SURF_PACKED;
    jpeg_dec_frame_host(g, pl, u, channel_order, rule);
    const int oh = jpeg_orient_h(orient, g.h, g.w), ow = jpeg_orient_w(orient, g.h, g.w);
    for (int Y = 0; Y < oh; ++Y) {
        uint8_t* o = static_cast<uint8_t*>(dst.plane[0]) + size_t(Y) * size_t(dst.pitch[0]);
        for (int X = 0; X < ow; ++X) {
            int y, x;
            jpeg_orient_source(orient, g.h, g.w, Y, X, y, x);
            std::memcpy(o + 3 * X, up.data() + (size_t(y) * size_t(g.w) + size_t(x)) * 3, 3);
        }
    }
}

}  // namespace whenet
