// The baseline JPEG encoder as arithmetic, shared by the host statement (whenet_jpeg_encode_host, whenet_jpeg_header,
// whenet_jpeg_bound) and the kernels of jpeg.hip: the sample fetch, the forward DCT, the quantiser and the code words of a block,
// each exactly as include/whenet_hip.h states it (JPEG ENCODER).  Integers only.  Nothing here needs the HIP runtime: a plain
// C++17 compiler builds this header (tools/jpeg_host_check.cpp does, under the host sanitizers).
//
// Reference: demo_video.py:46-47, :60 (`cv2.VideoWriter(..., 'MJPG', ...)`, `out.write(frame)`): the annotated frame stored as
// Motion-JPEG.  The quantiser tables, the Huffman tables and the zigzag order below are those of the JPEG standard (ITU-T T.81,
// Annex K.1, K.3 and figure A.6), written out as data.
#pragma once

#include <cstdint>
#include <cstring>
#include <memory>

#include "overlay_host.h"

namespace whenet {

constexpr int JPEG_MAX_SIDE = 8192;
constexpr int JPEG_HEADER_BYTES = WHENET_JPEG_HEADER_BYTES;
constexpr int JPEG_BLOCK_MAX_BITS = 11 + 11 + 63 * (16 + 10);      // DC code + extra bits, 63 x (AC code + extra bits): no EOB then
constexpr int JPEG_MCU_BLOCKS = 6;                                  // 4:2:0: Y00, Y01, Y10, Y11, Cb, Cr
constexpr int JPEG_MAX_INTERVAL_BLOCKS = (JPEG_MAX_SIDE / 16) * JPEG_MCU_BLOCKS;      // 3,072: the most blocks of an interval of the ENCODER, at any of its three samplings (the decoder does not read it)
constexpr int JPEG_HUFF_MAX_LEN = 257;                              // no code of 257 symbols is longer before the lengths are limited
constexpr int JPEG_CODE_MAX_BITS = 26;                              // the longest code word with its extra bits

// zigzag position -> natural index v * 8 + u (T.81 figure A.6)
constexpr uint8_t JPEG_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// T.81 tables K.1 (luminance) and K.2 (chrominance), natural order
constexpr uint8_t JPEG_QBASE[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// T.81 tables K.3 - K.6: the number of codes of each length 1..16, then the symbols in code order; DC0, AC0, DC1, AC1
constexpr uint8_t JPEG_HUFF_BITS[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                           {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                                           {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                           {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr int JPEG_HUFF_COUNT[4] = {12, 162, 12, 162};
constexpr uint8_t JPEG_HUFF_VALS[4][162] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11},
    {1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161, 8,   35,  66,  177,
     193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,  39,  40,  41,  42,  52,  53,  54,  55,
     56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106,
     115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
     164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211,
     212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11},
    {0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,  145, 161, 177, 193,
     9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,  26,  38,  39,  40,  41,  42,  53,  54,
     55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105,
     106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
     162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
     210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}};

// What a call needs besides the pixels, built on the host for (h, w, quality) and read by the host statement and the kernels alike.
struct JpegTables {
    int32_t q[2][64];            // the scaled quantisers, natural order
    uint16_t code[4][256];       // DC0, AC0, DC1, AC1: the code word of a symbol, right-aligned
    uint8_t len[4][256];         // ... its length (0: the table has no such symbol)
    uint8_t zz_pos[64];          // natural index -> zigzag position
    uint8_t header[JPEG_HEADER_BYTES + 3];
};

// The MCU of a sampling (WHENET_JPEG_420 / 422 / 444): hs x vs luma blocks in row order, then Cb, then Cr; the chroma planes are
// ceil(h / vs) x ceil(w / hs).  A restart interval is one MCU row: ceil(w / 8 hs) MCUs.
struct JpegGeom {
    int sampling, hs, vs, luma, blocks;      // luma = hs vs blocks of Y in an MCU, blocks = luma + 2
};
WHENET_HD constexpr JpegGeom jpeg_geom(int sampling) {
    return sampling == WHENET_JPEG_444 ? JpegGeom{WHENET_JPEG_444, 1, 1, 1, 3}
                                       : (sampling == WHENET_JPEG_422 ? JpegGeom{WHENET_JPEG_422, 2, 1, 2, 4} : JpegGeom{WHENET_JPEG_420, 2, 2, 4, 6});
}
inline bool jpeg_sampling_ok(int sampling) { return sampling == WHENET_JPEG_420 || sampling == WHENET_JPEG_422 || sampling == WHENET_JPEG_444; }

// One source frame: planes (host or device memory), their pitches, and the JFIF row of the BGR -> 4:2:0 rule for packed pixels
struct JpegSource {
    const uint8_t* plane[3];
    int pitch[3];
    int format, channel_order, h, w;
    Bgr2YuvCoeffs kc;
};

inline int jpeg_mcu_cols(int w, int sampling = WHENET_JPEG_420) { return (w + 8 * jpeg_geom(sampling).hs - 1) / (8 * jpeg_geom(sampling).hs); }
inline int jpeg_mcu_rows(int h, int sampling = WHENET_JPEG_420) { return (h + 8 * jpeg_geom(sampling).vs - 1) / (8 * jpeg_geom(sampling).vs); }
// the unstuffed bytes an interval (one MCU row) can have at most, and the bound of the whole stream (header, every byte stuffed,
// RSTm behind every interval but the last, EOI behind the last)
inline int64_t jpeg_interval_bytes(int w, int sampling = WHENET_JPEG_420) {
    return (int64_t(jpeg_mcu_cols(w, sampling)) * jpeg_geom(sampling).blocks * JPEG_BLOCK_MAX_BITS + 7) / 8;
}
inline int64_t jpeg_bound(int h, int w, int sampling = WHENET_JPEG_420) {
    return JPEG_HEADER_BYTES + int64_t(jpeg_mcu_rows(h, sampling)) * (2 * jpeg_interval_bytes(w, sampling) + 2);
}

inline int jpeg_scaled_q(int base, int quality) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int q = (base * scale + 50) / 100;
    return q < 1 ? 1 : (q > 255 ? 255 : q);
}

// Argument errors of a frame size and a quality, as a text (nullptr: none)
inline const char* jpeg_check_size(int h, int w, int quality) {
    if (h < 1 || w < 1 || h > JPEG_MAX_SIDE || w > JPEG_MAX_SIDE) return "frame sides must be 1..8192";
    if (quality < 1 || quality > 100) return "quality must be 1..100";
    return nullptr;
}

// ... and of a whole encode call
inline const char* jpeg_check(const whenet_surface_t* src, int h, int w, int channel_order, int quality, const void* out, int64_t cap,
                              const void* size, int sampling = WHENET_JPEG_420) {
    if (src == nullptr || size == nullptr || (out == nullptr && cap > 0)) return "NULL argument";
    if (!jpeg_sampling_ok(sampling)) return "unknown sampling (WHENET_JPEG_420, WHENET_JPEG_422 or WHENET_JPEG_444)";
    if (sampling != WHENET_JPEG_420 && (src->format == WHENET_YUV_NV12 || src->format == WHENET_YUV_I420))
        return "an NV12 / I420 source carries 4:2:0 chroma: 4:2:2 and 4:4:4 streams take packed pixels (WHENET_SURF_PACKED)";
    if (cap < 0) return "negative capacity";
    if (const char* bad = jpeg_check_size(h, w, quality)) return bad;
    int rows[3], row_bytes[3];
    const int planes = overlay_surface_planes(src->format, h, w, rows, row_bytes);
    if (planes == 0) return "unknown surface format (WHENET_SURF_PACKED, WHENET_YUV_NV12 or WHENET_YUV_I420)";
    if (src->format == WHENET_SURF_PACKED) {
        if (channel_order != WHENET_RGB && channel_order != WHENET_BGR) return "unknown channel order";
    } else if (src->matrix != WHENET_YUV_JFIF) {
        return "a YUV source must have the matrix WHENET_YUV_JFIF (JFIF is full-range BT.601)";
    }
    for (int p = 0; p < planes; ++p) {
        if (src->plane[p] == nullptr) return "a plane of the surface is NULL";
        if (src->pitch[p] < row_bytes[p]) return "a pitch of the surface is below its row bytes";
    }
    return nullptr;
}

inline JpegSource jpeg_source(const whenet_surface_t& src, int h, int w, int channel_order) {
    JpegSource s{};
    for (int p = 0; p < 3; ++p) s.plane[p] = static_cast<const uint8_t*>(src.plane[p]), s.pitch[p] = src.pitch[p];
    s.format = src.format, s.channel_order = channel_order, s.h = h, s.w = w;
    (void)bgr2yuv_coeffs(WHENET_YUV_JFIF, s.kc);
    return s;
}

// The tables and the header of (h, w, quality, sampling), all four valid
inline void jpeg_build_tables(int h, int w, int quality, JpegTables& t, int sampling = WHENET_JPEG_420) {
    const JpegGeom g = jpeg_geom(sampling);
    std::memset(&t, 0, sizeof(t));
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 64; ++i) t.q[c][i] = jpeg_scaled_q(JPEG_QBASE[c][i], quality);
    for (int k = 0; k < 64; ++k) t.zz_pos[JPEG_ZIGZAG[k]] = uint8_t(k);
    for (int tb = 0; tb < 4; ++tb) {      // the canonical codes of T.81 annex C: in order of length, counting up
        unsigned code = 0;
        int n = 0;
        for (int l = 1; l <= 16; ++l) {
            for (int i = 0; i < JPEG_HUFF_BITS[tb][l - 1]; ++i, ++n) {
                const int sym = JPEG_HUFF_VALS[tb][n];
                t.code[tb][sym] = uint16_t(code++), t.len[tb][sym] = uint8_t(l);
            }
            code <<= 1;
        }
    }
    uint8_t* p = t.header;
    const auto put = [&p](int b) { *p++ = uint8_t(b); };
    const auto put16 = [&put](int v) { put(v >> 8), put(v & 255); };
    put(0xFF), put(0xD8);                                              // SOI
    put(0xFF), put(0xE0), put16(16);                                   // APP0
    put('J'), put('F'), put('I'), put('F'), put(0), put(1), put(1), put(0), put16(1), put16(1), put(0), put(0);
    for (int c = 0; c < 2; ++c) {                                      // DQT: 8 bit, table c, zigzag order
        put(0xFF), put(0xDB), put16(67), put(c);
        for (int k = 0; k < 64; ++k) put(t.q[c][JPEG_ZIGZAG[k]]);
    }
    put(0xFF), put(0xC0), put16(17), put(8), put16(h), put16(w), put(3);      // SOF0
    put(1), put((g.hs << 4) | g.vs), put(0), put(2), put(0x11), put(1), put(3), put(0x11), put(1);
    for (int tb = 0; tb < 4; ++tb) {                                   // DHT: DC0, AC0, DC1, AC1
        put(0xFF), put(0xC4), put16(2 + 1 + 16 + JPEG_HUFF_COUNT[tb]), put(((tb & 1) << 4) | (tb >> 1));
        for (int l = 0; l < 16; ++l) put(JPEG_HUFF_BITS[tb][l]);
        for (int i = 0; i < JPEG_HUFF_COUNT[tb]; ++i) put(JPEG_HUFF_VALS[tb][i]);
    }
    put(0xFF), put(0xDD), put16(4), put16(jpeg_mcu_cols(w, sampling));      // DRI: one interval per MCU row
    put(0xFF), put(0xDA), put16(12), put(3), put(1), put(0x00), put(2), put(0x11), put(3), put(0x11), put(0), put(63), put(0);      // SOS
}

// The sample (y, x) of component comp (0 Y, 1 Cb, 2 Cr) on its own plane, the edge replicated.  A chroma sample of packed pixels is
// overlay_cb / overlay_cr of R, G, B sums worth four pixels: the hs x vs pixels it covers, times 4 / (hs vs).
template <int S = WHENET_JPEG_420>
WHENET_HD inline int jpeg_sample(const JpegSource& s, int comp, int y, int x) {
    constexpr JpegGeom g = jpeg_geom(S);
    if (comp == 0) {
        y = y < s.h - 1 ? y : s.h - 1, x = x < s.w - 1 ? x : s.w - 1;
        if (s.format != WHENET_SURF_PACKED) return s.plane[0][size_t(y) * size_t(s.pitch[0]) + size_t(x)];
        const uint8_t* p = s.plane[0] + size_t(y) * size_t(s.pitch[0]) + 3 * size_t(x);
        const int ri = s.channel_order == WHENET_BGR ? 2 : 0;
        return overlay_luma(s.kc, p[ri], p[1], p[2 - ri]);
    }
    const int ch = (s.h + g.vs - 1) / g.vs, cw = (s.w + g.hs - 1) / g.hs;
    y = y < ch - 1 ? y : ch - 1, x = x < cw - 1 ? x : cw - 1;
    if (s.format == WHENET_YUV_I420) return s.plane[comp][size_t(y) * size_t(s.pitch[comp]) + size_t(x)];
    if (s.format == WHENET_YUV_NV12) return s.plane[1][size_t(y) * size_t(s.pitch[1]) + 2 * size_t(x) + size_t(comp - 1)];
    const int ri = s.channel_order == WHENET_BGR ? 2 : 0;
    int rs = 0, gs = 0, bs = 0;
    for (int dy = 0; dy < g.vs; ++dy)
        for (int dx = 0; dx < g.hs; ++dx) {
            const int yy = g.vs * y + dy < s.h - 1 ? g.vs * y + dy : s.h - 1, xx = g.hs * x + dx < s.w - 1 ? g.hs * x + dx : s.w - 1;
            const uint8_t* p = s.plane[0] + size_t(yy) * size_t(s.pitch[0]) + 3 * size_t(xx);
            rs += p[ri], gs += p[1], bs += p[2 - ri];
        }
    constexpr int k = 4 / (g.hs * g.vs);
    return comp == 1 ? overlay_cb(s.kc, k * rs, k * gs, k * bs) : overlay_cr(s.kc, k * rs, k * gs, k * bs);
}

// block i of an interval's blocks: its component and the first sample of it on the component's plane
template <int S = WHENET_JPEG_420>
WHENET_HD inline void jpeg_block_origin(int interval, int i, int& comp, int& y0, int& x0) {
    constexpr JpegGeom g = jpeg_geom(S);
    const int m = i / g.blocks, c = i - m * g.blocks;
    if (c < g.luma) {
        comp = 0, y0 = (interval * g.vs + c / g.hs) * 8, x0 = (m * g.hs + c % g.hs) * 8;
    } else {
        comp = c - g.luma + 1, y0 = interval * 8, x0 = m * 8;
    }
}
// ... and the block before it of the same component in the interval, whose DC is its predictor (-1: none, the predictor is 0)
template <int S = WHENET_JPEG_420>
WHENET_HD inline int jpeg_block_before(int i) {
    constexpr JpegGeom g = jpeg_geom(S);
    const int m = i / g.blocks, c = i - m * g.blocks;
    if (c >= 1 && c < g.luma) return i - 1;
    if (m == 0) return -1;
    return c == 0 ? i - g.blocks + g.luma - 1 : i - g.blocks;      // the last luma block of the MCU before, or the same chroma block of it
}
// ... and whether it is a luma block (tables 0) or a chroma block (tables 1)
template <int S = WHENET_JPEG_420>
WHENET_HD inline bool jpeg_block_is_luma(int i) {
    return i % jpeg_geom(S).blocks < jpeg_geom(S).luma;
}

// out[u] = sum_x T[u][x] in[x]: one pass of the forward DCT over 8 values
WHENET_HD inline void jpeg_dct8(const int in[8], int out[8]) {
    constexpr int T[8][8] = WHENET_JPEG_DCT;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int u = 0; u < 8; ++u) {
        int a = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int x = 0; x < 8; ++x) a += T[u][x] * in[x];
        out[u] = a;
    }
}
WHENET_HD inline int jpeg_dct_round(int a) { return (a + 256) >> 9; }

// k = sign(b) ((|b| + (Q << 14)) / (Q << 15)), AC clamped to +-1023
WHENET_HD inline int jpeg_quant(int b, int q, bool ac) {
    const unsigned mag = unsigned(b < 0 ? -b : b);
    int k = int((mag + (unsigned(q) << 14)) / (unsigned(q) << 15));
    if (ac && k > 1023) k = 1023;
    return b < 0 ? -k : k;
}

WHENET_HD inline int jpeg_bit_size(int v) {      // the category of a value: the bits of |v|
    const unsigned m = unsigned(v < 0 ? -v : v);
    return m == 0 ? 0 : 32 - __builtin_clz(m);
}

// The code words of a block, in order, to sink.put(bits, n): n <= JPEG_CODE_MAX_BITS bits, right-aligned.  zz: the quantised
// coefficients in zigzag order; pred: the DC predictor; dc / ac: the component's table indices into JpegTables::code / len.
template <typename Sink>
WHENET_HD inline void jpeg_block_codes(const int16_t* zz, int pred, const uint16_t* dc_code, const uint8_t* dc_len, const uint16_t* ac_code,
                                       const uint8_t* ac_len, Sink& sink) {
    const int d = int(zz[0]) - pred;
    int s = jpeg_bit_size(d);
    sink.put((uint32_t(dc_code[s]) << s) | (uint32_t(d < 0 ? d - 1 : d) & ((1u << s) - 1u)), int(dc_len[s]) + s);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int c = zz[k];
        if (c == 0) {
            ++run;
            continue;
        }
        for (; run > 15; run -= 16) sink.put(ac_code[0xF0], ac_len[0xF0]);      // ZRL
        s = jpeg_bit_size(c);
        const int sym = (run << 4) | s;
        sink.put((uint32_t(ac_code[sym]) << s) | (uint32_t(c < 0 ? c - 1 : c) & ((1u << s) - 1u)), int(ac_len[sym]) + s);
        run = 0;
    }
    if (run > 0) sink.put(ac_code[0x00], ac_len[0x00]);                          // EOB: coefficient 63 is zero
}

struct JpegBitCounter {
    int bits = 0;
    WHENET_HD void put(uint32_t, int n) { bits += n; }
};

// ---- the host statement ----
// bytes to out[0 .. cap): `pos` counts every byte, written or not
struct JpegByteSink {
    uint8_t* out;
    int64_t cap, pos;
    void byte(int b) {
        if (pos < cap) out[pos] = uint8_t(b);
        ++pos;
    }
};
// the entropy-coded bits of an interval, most significant first, 0xFF followed by 0x00
struct JpegBitWriter {
    JpegByteSink& o;
    uint64_t acc = 0;
    int n = 0;
    void put(uint32_t bits, int len) {
        acc = (acc << len) | bits, n += len;
        while (n >= 8) {
            const int b = int((acc >> (n - 8)) & 0xFF);
            o.byte(b);
            if (b == 0xFF) o.byte(0);
            n -= 8;
        }
    }
    void pad() {      // 1-bits up to the byte's end
        if (n > 0) put((1u << (8 - n)) - 1u, 8 - n);
    }
};

template <int S = WHENET_JPEG_420>
inline void jpeg_block_host(const JpegSource& s, const JpegTables& t, int comp, int y0, int x0, int16_t zz[64]) {
    int r[8][8], col[8], b[8];
    for (int y = 0; y < 8; ++y) {
        int p[8], a[8];
        for (int x = 0; x < 8; ++x) p[x] = jpeg_sample<S>(s, comp, y0 + y, x0 + x) - 128;
        jpeg_dct8(p, a);
        for (int u = 0; u < 8; ++u) r[y][u] = jpeg_dct_round(a[u]);
    }
    const int32_t* q = t.q[comp == 0 ? 0 : 1];
    for (int u = 0; u < 8; ++u) {
        for (int y = 0; y < 8; ++y) col[y] = r[y][u];
        jpeg_dct8(col, b);
        for (int v = 0; v < 8; ++v) zz[t.zz_pos[v * 8 + u]] = int16_t(jpeg_quant(b[v], q[v * 8 + u], v + u > 0));
    }
}

// ---- optimised Huffman tables (T.81 K.2, figures K.1 - K.4, ties as libjpeg's jpeg_gen_optimal_table breaks them) ----
// The symbols of a block, in order, to sink.symbol(cls, sym): cls 0 the DC category, cls 1 a (run, size) symbol, ZRL or EOB.  The
// walk of jpeg_block_codes without the tables.
template <typename Sink>
WHENET_HD inline void jpeg_block_symbols(const int16_t* zz, int pred, Sink& sink) {
    sink.symbol(0, jpeg_bit_size(int(zz[0]) - pred));
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int c = zz[k];
        if (c == 0) {
            ++run;
            continue;
        }
        for (; run > 15; run -= 16) sink.symbol(1, 0xF0);
        sink.symbol(1, (run << 4) | jpeg_bit_size(c));
        run = 0;
    }
    if (run > 0) sink.symbol(1, 0x00);
}

// What an optimised encode builds for itself: the four histograms (DC0, AC0, DC1, AC1), the codes the pack stage reads, and the
// header with DHT segments that list the occurring symbols only (at most JPEG_HEADER_BYTES long)
struct JpegOptTables {
    uint32_t hist[4][256];
    uint16_t code[4][256];
    uint8_t len[4][256];
    uint8_t header[JPEG_HEADER_BYTES + 3];
    int32_t header_bytes;
};

// The work arrays of one table's construction (LDS on the device): frequencies with the reserved code point at 256, the code size
// and the chain of every symbol, the number of codes of each length
struct JpegHuffWork {
    uint64_t freq[257];      // (the sum of 256 uint32 frequencies fits)
    int16_t codesize[257];
    int16_t others[257];
    int16_t bits[JPEG_HUFF_MAX_LEN + 1];
    int16_t pos[JPEG_HUFF_MAX_LEN + 1];
};

inline void jpeg_huff_begin(const uint32_t freq[256], JpegHuffWork& k) {
    for (int i = 0; i < 256; ++i) k.freq[i] = freq[i], k.codesize[i] = 0, k.others[i] = -1;
    k.freq[256] = 1, k.codesize[256] = 0, k.others[256] = -1;      // the reserved code point: no code is all ones
}
// the symbol of least non-zero frequency other than `skip`, the LARGER value on a tie (-1: none): figure K.1's search (the host's
// form; the table kernel runs the same search as a wave-wide minimum)
inline int jpeg_huff_least(const JpegHuffWork& k, int skip) {
    int c = -1;
    uint64_t v = ~uint64_t(0);
    for (int i = 0; i <= 256; ++i)
        if (k.freq[i] != 0 && k.freq[i] <= v && i != skip) v = k.freq[i], c = i;
    return c;
}
// figure K.1's merge of the two least frequent trees
WHENET_HD inline void jpeg_huff_merge(JpegHuffWork& k, int c1, int c2) {
    k.freq[c1] += k.freq[c2], k.freq[c2] = 0;
    for (++k.codesize[c1]; k.others[c1] >= 0;) c1 = k.others[c1], ++k.codesize[c1];
    k.others[c1] = int16_t(c2);
    for (++k.codesize[c2]; k.others[c2] >= 0;) c2 = k.others[c2], ++k.codesize[c2];
}
// figures K.2 - K.4: the number of codes of each length, limited to 16, the reserved code point removed; the symbols by code size,
// then by value.  Returns the number of symbols.
WHENET_HD inline int jpeg_huff_finish(JpegHuffWork& k, uint8_t bits[16], uint8_t vals[256]) {
    for (int l = 0; l <= JPEG_HUFF_MAX_LEN; ++l) k.bits[l] = 0;
    for (int i = 0; i <= 256; ++i)
        if (k.codesize[i] > 0) ++k.bits[k.codesize[i]];
    int n = 0;      // where the symbols of a code size begin: the sizes, not the limited lengths, order the symbols
    for (int l = 1; l <= JPEG_HUFF_MAX_LEN; ++l) k.pos[l] = int16_t(n), n += k.bits[l] - (k.codesize[256] == l ? 1 : 0);
    for (int i = 0; i < 256; ++i)
        if (k.codesize[i] > 0) vals[k.pos[k.codesize[i]]++] = uint8_t(i);
    for (int i = JPEG_HUFF_MAX_LEN; i > 16; --i)
        while (k.bits[i] > 0) {
            int j = i - 2;
            while (k.bits[j] == 0) --j;
            k.bits[i] -= 2, ++k.bits[i - 1], k.bits[j + 1] += 2, --k.bits[j];
        }
    int last = 16;
    while (last > 0 && k.bits[last] == 0) --last;
    if (last > 0) --k.bits[last];      // (last = 0: no symbol occurs at all, a table that is never built)
    for (int l = 1; l <= 16; ++l) bits[l - 1] = uint8_t(k.bits[l]);
    return n;
}
// The table of a histogram: whenet_jpeg_optimal_table
inline int jpeg_optimal_table(const uint32_t freq[256], uint8_t bits[16], uint8_t vals[256]) {
    JpegHuffWork k;
    jpeg_huff_begin(freq, k);
    for (;;) {
        const int c1 = jpeg_huff_least(k, -1), c2 = jpeg_huff_least(k, c1);
        if (c2 < 0) break;
        jpeg_huff_merge(k, c1, c2);
    }
    return jpeg_huff_finish(k, bits, vals);
}
// (bits, vals) -> the code and length of every symbol: the canonical codes of T.81 annex C
WHENET_HD inline void jpeg_huff_codes(const uint8_t bits[16], const uint8_t* vals, uint16_t code[256], uint8_t len[256]) {
    for (int i = 0; i < 256; ++i) code[i] = 0, len[i] = 0;
    unsigned c = 0;
    int n = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i, ++n) code[vals[n]] = uint16_t(c++), len[vals[n]] = uint8_t(l);
        c <<= 1;
    }
}
// The header of an optimised stream from the standard one of the same (h, w, quality, sampling): everything but the DHT segments
// is copied (SOI .. SOF0 in front of them, DRI and SOS behind).  Returns its length.
WHENET_HD inline int jpeg_opt_header(const uint8_t* std_header, const uint8_t bits[4][16], const uint8_t vals[4][256], const int count[4],
                                     uint8_t* out) {
    constexpr int front = 2 + 18 + 2 * 69 + 19, tail = 6 + 14;      // SOI APP0 DQT DQT SOF0 | DRI SOS
    int p = 0;
    for (int i = 0; i < front; ++i) out[p++] = std_header[i];
    for (int tb = 0; tb < 4; ++tb) {
        const int n = 2 + 1 + 16 + count[tb];
        out[p++] = 0xFF, out[p++] = 0xC4, out[p++] = uint8_t(n >> 8), out[p++] = uint8_t(n & 255), out[p++] = uint8_t(((tb & 1) << 4) | (tb >> 1));
        for (int l = 0; l < 16; ++l) out[p++] = bits[tb][l];
        for (int i = 0; i < count[tb]; ++i) out[p++] = vals[tb][i];
    }
    for (int i = 0; i < tail; ++i) out[p++] = std_header[JPEG_HEADER_BYTES - tail + i];
    return p;
}

struct JpegHistSink {
    uint32_t* hist;      // [2][256]: the component's DC and AC histogram
    void symbol(int cls, int sym) { ++hist[cls * 256 + sym]; }
};

// The whole stream to out[0 .. cap); returns its full length.  optimize: the tables are built from the frame's own symbols first
// (hist, when not NULL, receives the four histograms)
template <int S>
inline int64_t jpeg_encode_host_s(const JpegSource& s, const JpegTables& t, uint8_t* out, int64_t cap, bool optimize, uint32_t (*hist)[256]) {
    constexpr JpegGeom g = jpeg_geom(S);
    JpegByteSink o{out, cap, 0};
    const int R = jpeg_mcu_rows(s.h, S), B = jpeg_mcu_cols(s.w, S) * g.blocks;
    const uint16_t(*code)[256] = t.code;
    const uint8_t(*len)[256] = t.len;
    const uint8_t* header = t.header;
    int header_bytes = JPEG_HEADER_BYTES;
    std::unique_ptr<JpegOptTables> opt;
    if (optimize) {
        opt.reset(new JpegOptTables);
        std::memset(opt.get(), 0, sizeof(JpegOptTables));
        for (int r = 0; r < R; ++r) {
            int pred[3] = {0, 0, 0};
            for (int i = 0; i < B; ++i) {
                int comp, y0, x0;
                int16_t zz[64];
                jpeg_block_origin<S>(r, i, comp, y0, x0);
                jpeg_block_host<S>(s, t, comp, y0, x0, zz);
                JpegHistSink sink{opt->hist[comp == 0 ? 0 : 2]};
                jpeg_block_symbols(zz, pred[comp], sink);
                pred[comp] = zz[0];
            }
        }
        uint8_t bits[4][16], vals[4][256];
        int count[4];
        for (int tb = 0; tb < 4; ++tb) {
            count[tb] = jpeg_optimal_table(opt->hist[tb], bits[tb], vals[tb]);
            jpeg_huff_codes(bits[tb], vals[tb], opt->code[tb], opt->len[tb]);
        }
        opt->header_bytes = jpeg_opt_header(t.header, bits, vals, count, opt->header);
        code = opt->code, len = opt->len, header = opt->header, header_bytes = opt->header_bytes;
        if (hist != nullptr) std::memcpy(hist, opt->hist, sizeof(opt->hist));
    }
    for (int i = 0; i < header_bytes; ++i) o.byte(header[i]);
    for (int r = 0; r < R; ++r) {
        JpegBitWriter bw{o};
        int pred[3] = {0, 0, 0};
        for (int i = 0; i < B; ++i) {
            int comp, y0, x0;
            int16_t zz[64];
            jpeg_block_origin<S>(r, i, comp, y0, x0);
            jpeg_block_host<S>(s, t, comp, y0, x0, zz);
            const int tb = comp == 0 ? 0 : 2;
            jpeg_block_codes(zz, pred[comp], code[tb], len[tb], code[tb + 1], len[tb + 1], bw);
            pred[comp] = zz[0];
        }
        bw.pad();
        o.byte(0xFF), o.byte(r + 1 < R ? 0xD0 + (r & 7) : 0xD9);      // RSTm, or EOI behind the last interval
    }
    return o.pos;
}

// `t`: the tables of jpeg_build_tables for the same sampling
inline int64_t jpeg_encode_host(const JpegSource& s, const JpegTables& t, uint8_t* out, int64_t cap, int sampling = WHENET_JPEG_420,
                                bool optimize = false, uint32_t (*hist)[256] = nullptr) {
    if (sampling == WHENET_JPEG_444) return jpeg_encode_host_s<WHENET_JPEG_444>(s, t, out, cap, optimize, hist);
    if (sampling == WHENET_JPEG_422) return jpeg_encode_host_s<WHENET_JPEG_422>(s, t, out, cap, optimize, hist);
    return jpeg_encode_host_s<WHENET_JPEG_420>(s, t, out, cap, optimize, hist);
}

}  // namespace whenet
