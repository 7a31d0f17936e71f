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

#include "overlay_host.h"

namespace whenet {

constexpr int JPEG_MAX_SIDE = 8192;
constexpr int JPEG_HEADER_BYTES = WHENET_JPEG_HEADER_BYTES;
constexpr int JPEG_BLOCK_MAX_BITS = 11 + 11 + 63 * (16 + 10);      // DC code + extra bits, 63 x (AC code + extra bits): no EOB then
constexpr int JPEG_MCU_BLOCKS = 6;                                  // Y00, Y01, Y10, Y11, Cb, Cr
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

// One source frame: planes (host or device memory), their pitches, and the JFIF row of the BGR -> 4:2:0 rule for packed pixels
struct JpegSource {
    const uint8_t* plane[3];
    int pitch[3];
    int format, channel_order, h, w;
    Bgr2YuvCoeffs kc;
};

inline int jpeg_mcu_cols(int w) { return (w + 15) >> 4; }
inline int jpeg_mcu_rows(int h) { return (h + 15) >> 4; }
// the unstuffed bytes an interval (one MCU row) can have at most, and the bound of the whole stream (header, every byte stuffed,
// RSTm behind every interval but the last, EOI behind the last)
inline int64_t jpeg_interval_bytes(int w) { return (int64_t(jpeg_mcu_cols(w)) * JPEG_MCU_BLOCKS * JPEG_BLOCK_MAX_BITS + 7) / 8; }
inline int64_t jpeg_bound(int h, int w) { return JPEG_HEADER_BYTES + int64_t(jpeg_mcu_rows(h)) * (2 * jpeg_interval_bytes(w) + 2); }

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
                              const void* size) {
    if (src == nullptr || size == nullptr || (out == nullptr && cap > 0)) return "NULL argument";
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

// The tables and the header of (h, w, quality), all three valid
inline void jpeg_build_tables(int h, int w, int quality, JpegTables& t) {
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
    put(1), put(0x22), put(0), put(2), put(0x11), put(1), put(3), put(0x11), put(1);
    for (int tb = 0; tb < 4; ++tb) {                                   // DHT: DC0, AC0, DC1, AC1
        put(0xFF), put(0xC4), put16(2 + 1 + 16 + JPEG_HUFF_COUNT[tb]), put(((tb & 1) << 4) | (tb >> 1));
        for (int l = 0; l < 16; ++l) put(JPEG_HUFF_BITS[tb][l]);
        for (int i = 0; i < JPEG_HUFF_COUNT[tb]; ++i) put(JPEG_HUFF_VALS[tb][i]);
    }
    put(0xFF), put(0xDD), put16(4), put16(jpeg_mcu_cols(w));           // DRI: one interval per MCU row
    put(0xFF), put(0xDA), put16(12), put(3), put(1), put(0x00), put(2), put(0x11), put(3), put(0x11), put(0), put(63), put(0);      // SOS
}

// The sample (y, x) of component comp (0 Y, 1 Cb, 2 Cr) on its own plane, the edge replicated
WHENET_HD inline int jpeg_sample(const JpegSource& s, int comp, int y, int x) {
    if (comp == 0) {
        y = y < s.h - 1 ? y : s.h - 1, x = x < s.w - 1 ? x : s.w - 1;
        if (s.format != WHENET_SURF_PACKED) return s.plane[0][size_t(y) * size_t(s.pitch[0]) + size_t(x)];
        const uint8_t* p = s.plane[0] + size_t(y) * size_t(s.pitch[0]) + 3 * size_t(x);
        const int ri = s.channel_order == WHENET_BGR ? 2 : 0;
        return overlay_luma(s.kc, p[ri], p[1], p[2 - ri]);
    }
    const int ch = (s.h + 1) >> 1, cw = (s.w + 1) >> 1;
    y = y < ch - 1 ? y : ch - 1, x = x < cw - 1 ? x : cw - 1;
    if (s.format == WHENET_YUV_I420) return s.plane[comp][size_t(y) * size_t(s.pitch[comp]) + size_t(x)];
    if (s.format == WHENET_YUV_NV12) return s.plane[1][size_t(y) * size_t(s.pitch[1]) + 2 * size_t(x) + size_t(comp - 1)];
    const int ri = s.channel_order == WHENET_BGR ? 2 : 0;
    int rs = 0, gs = 0, bs = 0;
    for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx) {
            const int yy = 2 * y + dy < s.h - 1 ? 2 * y + dy : s.h - 1, xx = 2 * x + dx < s.w - 1 ? 2 * x + dx : s.w - 1;
            const uint8_t* p = s.plane[0] + size_t(yy) * size_t(s.pitch[0]) + 3 * size_t(xx);
            rs += p[ri], gs += p[1], bs += p[2 - ri];
        }
    return comp == 1 ? overlay_cb(s.kc, rs, gs, bs) : overlay_cr(s.kc, rs, gs, bs);
}

// block i of an interval's 6 * mcu_cols blocks: its component and the first sample of it on the component's plane
WHENET_HD inline void jpeg_block_origin(int interval, int i, int& comp, int& y0, int& x0) {
    const int m = i / JPEG_MCU_BLOCKS, c = i - m * JPEG_MCU_BLOCKS;
    if (c < 4) {
        comp = 0, y0 = interval * 16 + (c >> 1) * 8, x0 = m * 16 + (c & 1) * 8;
    } else {
        comp = c - 3, y0 = interval * 8, x0 = m * 8;
    }
}
// ... and the block before it of the same component in the interval, whose DC is its predictor (-1: none, the predictor is 0)
WHENET_HD inline int jpeg_block_before(int i) {
    const int m = i / JPEG_MCU_BLOCKS, c = i - m * JPEG_MCU_BLOCKS;
    if (c >= 1 && c <= 3) return i - 1;
    if (m == 0) return -1;
    return c == 0 ? i - 3 : i - JPEG_MCU_BLOCKS;
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

inline void jpeg_block_host(const JpegSource& s, const JpegTables& t, int comp, int y0, int x0, int16_t zz[64]) {
    int r[8][8], col[8], b[8];
    for (int y = 0; y < 8; ++y) {
        int p[8], a[8];
        for (int x = 0; x < 8; ++x) p[x] = jpeg_sample(s, comp, y0 + y, x0 + x) - 128;
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

// The whole stream to out[0 .. cap); returns its full length
inline int64_t jpeg_encode_host(const JpegSource& s, const JpegTables& t, uint8_t* out, int64_t cap) {
    JpegByteSink o{out, cap, 0};
    for (int i = 0; i < JPEG_HEADER_BYTES; ++i) o.byte(t.header[i]);
    const int R = jpeg_mcu_rows(s.h), B = jpeg_mcu_cols(s.w) * JPEG_MCU_BLOCKS;
    for (int r = 0; r < R; ++r) {
        JpegBitWriter bw{o};
        int pred[3] = {0, 0, 0};
        for (int i = 0; i < B; ++i) {
            int comp, y0, x0;
            int16_t zz[64];
            jpeg_block_origin(r, i, comp, y0, x0);
            jpeg_block_host(s, t, comp, y0, x0, zz);
            const int tb = comp == 0 ? 0 : 2;
            jpeg_block_codes(zz, pred[comp], t.code[tb], t.len[tb], t.code[tb + 1], t.len[tb + 1], bw);
            pred[comp] = zz[0];
        }
        bw.pad();
        o.byte(0xFF), o.byte(r + 1 < R ? 0xD0 + (r & 7) : 0xD9);      // RSTm, or EOI behind the last interval
    }
    return o.pos;
}

}  // namespace whenet
