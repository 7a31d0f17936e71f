// The pose overlay as arithmetic, shared by the host statement (whenet_annotate_host, whenet_overlay_segments) and the kernels of
// overlay.hip: the segments of a head, the raster rule and the BGR -> 4:2:0 leg, each exactly as include/whenet_hip.h states it.
// Nothing here needs the HIP runtime: a plain C++17 compiler builds this header (tools/probes/overlay_host_probe.cpp does, under
// the host sanitizers).
//
// Reference: utils.py:13-43 (`draw_axis`: angles to radians, six sin / cos products, `int()` of every endpoint, three cv2.line calls
// of thickness 2) and demo_video.py:26-29 (`cv2.rectangle` of the window, colour (0,0,0), then draw_axis from the window's centre).
// The raster of a segment is the project's own rule (OpenCV has never run next to this code): distance to the closed segment <= 1.
// demo_video.py:31-34 (`--display full`: three cv2.putText lines per head): the text is the executed reference's, "{}".format(np.round(a)),
// built from rintf and integer digits; the font and its thin raster (distance <= 1/2) are the project's own, stated in the header.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/whenet_hip.h"

#if defined(__HIPCC__)
#define WHENET_HD __host__ __device__
#else
#define WHENET_HD
#endif

namespace whenet {

constexpr int OVERLAY_MAX_HEADS = 256;
constexpr int OVERLAY_SEG_INTS = 16;          // (x, y) of: window corner 0, window corner 1, then P, Q of the X, Y and Z axis
constexpr int OVERLAY_COORD_MIN = -4096;      // window coordinates a head may have: |endpoint| < 2^14 follows (header, BOUNDS)
constexpr int OVERLAY_COORD_MAX = 8192;
constexpr int OVERLAY_MAX_FRAME_SIDE = 8192;
enum { OVERLAY_RECT = 1, OVERLAY_AXES = 2, OVERLAY_LABELS = 4 };  // flags of a head: what it paints
constexpr int OVERLAY_REACH_THICK = 2, OVERLAY_REACH_THIN = 1;     // twice the distance a segment paints to: 1 (axes, rectangle), 1/2 (glyphs)
constexpr int OVERLAY_GLYPHS = 25, OVERLAY_GLYPH_SEGS = 8;
constexpr int OVERLAY_GLYPH_W = 6, OVERLAY_GLYPH_TOP = -9, OVERLAY_GLYPH_ROWS = 13, OVERLAY_ADVANCE = 7;      // a glyph's box, the pen's step
constexpr int OVERLAY_LINE_CHARS = 14, OVERLAY_LINE_STEP = 15;     // "pitch: -9999.0"; the baselines of a head's lines are 15 rows apart
constexpr int OVERLAY_LABEL_WORDS = 12;                            // a head's label record: 3 lines x 4 words

struct Bgr2YuvCoeffs {
    int ry, gy, by, ru, gu, bu, rv, gv, bv, yoff;
};

WHENET_HD inline bool overlay_rect_in_range(const int32_t rect[4]) {
    for (int i = 0; i < 4; ++i)
        if (rect[i] < OVERLAY_COORD_MIN || rect[i] > OVERLAY_COORD_MAX) return false;
    return true;
}

// window (y0, x0, y1, x1) + angles in degrees (float32 widened to double by the caller) -> the 16 endpoint ints; returns the flags.
// utils.py:15-42 operation for operation in double, every operation rounded on its own (no contraction).
WHENET_HD inline int overlay_segments(const int32_t rect[4], int valid, double yaw, double pitch, double roll, int32_t seg[OVERLAY_SEG_INTS]) {
#pragma clang fp contract(off)
    for (int i = 0; i < OVERLAY_SEG_INTS; ++i) seg[i] = 0;
    if (!valid || !overlay_rect_in_range(rect)) return 0;
    const int y0 = rect[0], x0 = rect[1], y1 = rect[2], x1 = rect[3];
    seg[0] = x0, seg[1] = y0, seg[2] = x1, seg[3] = y1;
    if (!(std::isfinite(yaw) && std::isfinite(pitch) && std::isfinite(roll))) return OVERLAY_RECT;
    const double tdx = double(x0 + x1) / 2.0, tdy = double(y0 + y1) / 2.0;
    const int dx = x1 - x0;
    const double size = double(dx >= 0 ? dx / 2 : -((-dx + 1) / 2));      // Python's // (floor)
    const double pi = 3.141592653589793;
    pitch = pitch * pi / 180.0;
    yaw = -(yaw * pi / 180.0);
    roll = roll * pi / 180.0;
    const double cy = cos(yaw), sy = sin(yaw), cp = cos(pitch), sp = sin(pitch), cr = cos(roll), sr = sin(roll);
    const double ax = size * (cy * cr) + tdx;
    const double ay = size * (cp * sr + cr * sp * sy) + tdy;
    const double bx = size * (-cy * sr) + tdx;
    const double by = size * (cp * cr - sp * sy * sr) + tdy;
    const double cx = size * (sy) + tdx;
    const double cyy = size * (-cy * sp) + tdy;
    const int px = int(tdx), py = int(tdy);
    seg[4] = px, seg[5] = py, seg[6] = int(ax), seg[7] = int(ay);
    seg[8] = px, seg[9] = py, seg[10] = int(bx), seg[11] = int(by);
    seg[12] = px, seg[13] = py, seg[14] = int(cx), seg[15] = int(cyy);
    return OVERLAY_RECT | OVERLAY_AXES;
}

// the raster rule: is pixel (x, y) within distance reach / 2 of the closed segment P -> Q?  64-bit integers, exact.  reach 2 is the
// rule of the axes and the rectangle (4 d^2 <= 4 L2 is divided through: no product leaves 64 bits at the header's bounds); reach 1
// is the glyphs' rule, applied in a character cell's own coordinates, where every number is below 2^5.
WHENET_HD constexpr inline bool overlay_hit(int px, int py, int qx, int qy, int x, int y, int reach = OVERLAY_REACH_THICK) {
    const int64_t dx = qx - px, dy = qy - py, vx = x - px, vy = y - py;
    const int64_t L2 = dx * dx + dy * dy, t = vx * dx + vy * dy;
    const int64_t r2 = reach == OVERLAY_REACH_THICK ? 1 : 0;              // floor(reach^2 / 4): what an integer |v|^2 is compared with
    if (t <= 0) return vx * vx + vy * vy <= r2;
    if (t >= L2) {
        const int64_t wx = x - qx, wy = y - qy;
        return wx * wx + wy * wy <= r2;
    }
    const int64_t c = vx * dy - vy * dx;
    return reach == OVERLAY_REACH_THICK ? c * c <= L2 : 4 * c * c <= L2;
}

// ---- the labels: font, text, hit test ----
// The stroke font of the header (WHENET_OVERLAY_GLYPHS, WHENET_OVERLAY_FONT) and, built from it at compile time by the thin rule,
// every glyph's 13 rows of 6 bits: bit cx of rows[g][cy + 9] says whether the glyph paints (cx, cy) of its cell.  A glyph's strokes
// lie inside its box and reach 1/2 paints no pixel off a stroke's own rows and columns, so the rows ARE the glyph.
struct OverlayFont {
    int8_t seg[OVERLAY_GLYPHS][1 + 4 * OVERLAY_GLYPH_SEGS];
    uint8_t rows[OVERLAY_GLYPHS][16];
};
constexpr OverlayFont overlay_make_font() {
    constexpr int table[OVERLAY_GLYPHS][1 + 4 * OVERLAY_GLYPH_SEGS] = WHENET_OVERLAY_FONT;
    OverlayFont f{};
    for (int g = 0; g < OVERLAY_GLYPHS; ++g) {
        for (int j = 0; j < 1 + 4 * OVERLAY_GLYPH_SEGS; ++j) f.seg[g][j] = int8_t(table[g][j]);
        for (int cy = 0; cy < OVERLAY_GLYPH_ROWS; ++cy) {
            unsigned bits = 0;
            for (int cx = 0; cx < OVERLAY_GLYPH_W; ++cx)
                for (int s = 0; s < table[g][0]; ++s) {
                    const int* e = table[g] + 1 + 4 * s;
                    if (overlay_hit(e[0], e[1], e[2], e[3], cx, cy + OVERLAY_GLYPH_TOP, OVERLAY_REACH_THIN)) bits |= 1u << cx;
                }
            f.rows[g][cy] = uint8_t(bits);
        }
    }
    return f;
}
#if defined(__HIPCC__)
__device__ __constant__ constexpr OverlayFont OVERLAY_FONT_DEVICE = overlay_make_font();
#endif
constexpr OverlayFont OVERLAY_FONT = overlay_make_font();
WHENET_HD inline unsigned overlay_glyph_row(int g, int row) {
#if defined(__HIP_DEVICE_COMPILE__)
    return OVERLAY_FONT_DEVICE.rows[g][row];
#else
    return OVERLAY_FONT.rows[g][row];
#endif
}

// index of a character in WHENET_OVERLAY_GLYPHS, or -1
inline int overlay_glyph_index(int ch) {
    const char* all = WHENET_OVERLAY_GLYPHS;
    for (int g = 0; g < OVERLAY_GLYPHS; ++g)
        if (all[g] == ch) return g;
    return -1;
}

// A line of text as glyph indices, one per byte: characters 0..7 in `lo`, 8..14 in `hi` (byte 0 first), the length in hi's top byte.
// In memory four little-endian words {lo, lo >> 32, hi, hi >> 32}: the label record of a head is three of them (yaw, pitch, roll).
struct OverlayLine {
    uint64_t lo, hi;
};
WHENET_HD inline int overlay_line_length(const OverlayLine& t) { return int(t.hi >> 56); }
WHENET_HD inline int overlay_line_glyph(const OverlayLine& t, int i) { return int(((i < 8 ? t.lo >> (8 * i) : t.hi >> (8 * (i - 8)))) & 255u); }
WHENET_HD inline void overlay_line_put(OverlayLine& t, int& n, int g) {
    if (n < 8) t.lo |= uint64_t(g) << (8 * n);
    else t.hi |= uint64_t(g) << (8 * (n - 8));
    ++n;
}

// Line `line` (0 yaw, 1 pitch, 2 roll) for the float32 angle a: the name, ": ", then "{}".format(np.round(a)) -- r = rintf(a) (half
// to even), '-' if signbit(r), the digits of |r| without leading zeros, ".0".  false (and no text): |r| > 9999 or r is not a number.
WHENET_HD inline bool overlay_label_line(int line, float a, OverlayLine& t) {
    enum { A = 10, C, H, I, L, O, P, R, T, W, Y, COLON, SPACE, MINUS, DOT };
    t.lo = 0, t.hi = 0;
    const float r = rintf(a);
    if (!(fabsf(r) <= 9999.f)) return false;
    int n = 0;
    if (line == 0) {
        overlay_line_put(t, n, Y), overlay_line_put(t, n, A), overlay_line_put(t, n, W);
    } else if (line == 1) {
        overlay_line_put(t, n, P), overlay_line_put(t, n, I), overlay_line_put(t, n, T), overlay_line_put(t, n, C), overlay_line_put(t, n, H);
    } else {
        overlay_line_put(t, n, R), overlay_line_put(t, n, O), overlay_line_put(t, n, L), overlay_line_put(t, n, L);
    }
    overlay_line_put(t, n, COLON), overlay_line_put(t, n, SPACE);
    if (std::signbit(r)) overlay_line_put(t, n, MINUS);
    const int v = int(fabsf(r));
    const int d3 = v / 1000, d2 = v / 100 % 10, d1 = v / 10 % 10, d0 = v % 10;
    if (v >= 1000) overlay_line_put(t, n, d3);
    if (v >= 100) overlay_line_put(t, n, d2);
    if (v >= 10) overlay_line_put(t, n, d1);
    overlay_line_put(t, n, d0), overlay_line_put(t, n, DOT), overlay_line_put(t, n, 0);
    t.hi |= uint64_t(n) << 56;
    return true;
}

// The labels of a head whose segments and flags overlay_segments returned: the three lines and their baseline-left origins
// (x0, y0), (x0, y0 - 15), (x0, y0 - 30).  Returns OVERLAY_LABELS, or 0 (lines cleared): the head paints no axes, or a rounded angle
// is beyond +-9999.
WHENET_HD inline int overlay_labels(const int32_t seg[OVERLAY_SEG_INTS], int flags, float yaw, float pitch, float roll, OverlayLine lines[3],
                                    int32_t origin[3][2]) {
    bool ok = (flags & OVERLAY_AXES) != 0;
    ok = overlay_label_line(0, yaw, lines[0]) && ok;
    ok = overlay_label_line(1, pitch, lines[1]) && ok;
    ok = overlay_label_line(2, roll, lines[2]) && ok;
    for (int i = 0; i < 3; ++i) {
        origin[i][0] = seg[0], origin[i][1] = seg[1] - OVERLAY_LINE_STEP * i;
        if (!ok) lines[i].lo = 0, lines[i].hi = 0;
    }
    return ok ? OVERLAY_LABELS : 0;
}

// does the line with origin (ox, oy) paint pixel (x, y)?  The pixel lies in at most one character's cell: column (x - ox) / 7, and
// only the first 6 of a cell's 7 columns belong to the glyph's box.
WHENET_HD inline bool overlay_text_hit(const OverlayLine& t, int ox, int oy, int x, int y) {
    const int dx = x - ox, row = y - oy - OVERLAY_GLYPH_TOP;
    if (dx < 0 || row < 0 || row >= OVERLAY_GLYPH_ROWS) return false;
    const int cell = dx / OVERLAY_ADVANCE, cx = dx - cell * OVERLAY_ADVANCE;
    if (cell >= overlay_line_length(t) || cx >= OVERLAY_GLYPH_W) return false;
    return ((overlay_glyph_row(overlay_line_glyph(t, cell), row) >> cx) & 1u) != 0;
}

// the labels' colour (100, 255, 0) as B, G, R, in the frame's channel order, as overlay_colour packs a pixel
WHENET_HD inline uint32_t overlay_label_colour(int channel_order) { return channel_order == WHENET_BGR ? 0x00FF64u : 0x64FF00u; }

// The seven segments of a head in paint order (rectangle sides, then X, Y, Z): segment i of `seg` as P, Q and its colour index
// (0 = the rectangle's black, 1 = X red, 2 = Y green, 3 = Z blue).
WHENET_HD inline void overlay_head_segment(const int32_t seg[OVERLAY_SEG_INTS], int i, int& px, int& py, int& qx, int& qy, int& colour) {
    const int x0 = seg[0], y0 = seg[1], x1 = seg[2], y1 = seg[3];
    switch (i) {
        case 0: px = x0, py = y0, qx = x1, qy = y0, colour = 0; break;
        case 1: px = x1, py = y0, qx = x1, qy = y1, colour = 0; break;
        case 2: px = x1, py = y1, qx = x0, qy = y1, colour = 0; break;
        case 3: px = x0, py = y1, qx = x0, qy = y0, colour = 0; break;
        default: {
            const int32_t* a = seg + 4 * (i - 3);
            px = a[0], py = a[1], qx = a[2], qy = a[3], colour = i - 3;
        }
    }
}

// colour index -> the three bytes of a pixel in the frame's channel order, as a 24-bit little-endian value (byte 0 first)
WHENET_HD inline uint32_t overlay_colour(int colour, int channel_order) {
    const uint32_t r = channel_order == WHENET_BGR ? 0xFF0000u : 0x0000FFu;
    const uint32_t b = channel_order == WHENET_BGR ? 0x0000FFu : 0xFF0000u;
    return colour == 0 ? 0u : (colour == 1 ? r : (colour == 2 ? 0x00FF00u : b));
}

WHENET_HD inline int overlay_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
WHENET_HD inline int overlay_luma(const Bgr2YuvCoeffs& k, int r, int g, int b) {
    return overlay_clip8(((k.ry * r + k.gy * g + k.by * b + (1 << 19)) >> 20) + k.yoff);
}
WHENET_HD inline int overlay_cb(const Bgr2YuvCoeffs& k, int rs, int gs, int bs) {
    return overlay_clip8(((k.ru * rs + k.gu * gs + k.bu * bs + (1 << 21)) >> 22) + 128);
}
WHENET_HD inline int overlay_cr(const Bgr2YuvCoeffs& k, int rs, int gs, int bs) {
    return overlay_clip8(((k.rv * rs + k.gv * gs + k.bv * bs + (1 << 21)) >> 22) + 128);
}

inline bool bgr2yuv_coeffs(int matrix, Bgr2YuvCoeffs& out) {
    static const int table[WHENET_YUV_MATRICES][10] = WHENET_BGR2YUV_COEFFS;
    if (matrix < 0 || matrix >= WHENET_YUV_MATRICES) return false;
    const int* t = table[matrix];
    out = {t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], t[9]};
    return true;
}

// rows and row bytes of a surface's planes for an fh x fw frame; returns the number of planes (0: unknown format)
inline int overlay_surface_planes(int format, int fh, int fw, int rows[3], int row_bytes[3]) {
    const int cw = (fw + 1) >> 1, ch = (fh + 1) >> 1;
    if (format == WHENET_SURF_PACKED) {
        rows[0] = fh, row_bytes[0] = 3 * fw;
        return 1;
    }
    if (format == WHENET_YUV_NV12) {
        rows[0] = fh, row_bytes[0] = fw, rows[1] = ch, row_bytes[1] = 2 * cw;
        return 2;
    }
    if (format == WHENET_YUV_I420) {
        rows[0] = fh, row_bytes[0] = fw, rows[1] = rows[2] = ch, row_bytes[1] = row_bytes[2] = cw;
        return 3;
    }
    return 0;
}

// Argument errors of the host statement and of the kernels' entry points, as a text (nullptr: none)
inline const char* overlay_check(const void* frame, int fh, int fw, int channel_order, const int32_t* rects, const int32_t* valid,
                                 const float* ypr, int k, const whenet_surface_t* dst) {
    if (frame == nullptr || dst == nullptr) return "NULL argument";
    if (fh < 1 || fw < 1 || fh > OVERLAY_MAX_FRAME_SIDE || fw > OVERLAY_MAX_FRAME_SIDE) return "frame sides must be 1..8192";
    if (channel_order != WHENET_RGB && channel_order != WHENET_BGR) return "unknown channel order";
    if (k < 0 || k > OVERLAY_MAX_HEADS) return "0..256 heads";
    if (k > 0 && (rects == nullptr || ypr == nullptr)) return "NULL argument";
    int rows[3], row_bytes[3];
    const int planes = overlay_surface_planes(dst->format, fh, fw, rows, row_bytes);
    if (planes == 0) return "unknown surface format (WHENET_SURF_PACKED, WHENET_YUV_NV12 or WHENET_YUV_I420)";
    if (dst->format != WHENET_SURF_PACKED && (dst->matrix < 0 || dst->matrix >= WHENET_YUV_MATRICES))
        return "unknown matrix (WHENET_YUV_BT601, _BT709 or _JFIF)";
    for (int p = 0; p < planes; ++p) {
        if (dst->plane[p] == nullptr) return "a plane of the surface is NULL";
        if (dst->pitch[p] < row_bytes[p]) return "a pitch of the surface is below its row bytes";
    }
    for (int i = 0; i < k; ++i)
        if ((valid == nullptr || valid[i] != 0) && !overlay_rect_in_range(rects + 4 * i)) return "a window coordinate outside -4096..8192";
    return nullptr;
}

// The overlay as pure host arithmetic: what the kernels are held to.  `frame` uint8 [fh][fw][3] tight; segs [k][16], flags [k] as
// overlay_segments returns them; the surface's planes are host memory.  Only the rows' bytes are written.  lines [k][3]: the label
// records, read for the heads whose flags hold OVERLAY_LABELS (nullptr: none does).
inline void overlay_paint_host(const uint8_t* frame, int fh, int fw, int channel_order, const int32_t* segs, const int32_t* flags, int k,
                               const whenet_surface_t& dst, const OverlayLine* lines = nullptr) {
    // the annotated frame, packed, row by row (two rows at a time for 4:2:0)
    const bool packed = dst.format == WHENET_SURF_PACKED;
    Bgr2YuvCoeffs kc{};
    if (!packed) (void)bgr2yuv_coeffs(dst.matrix, kc);
    const int ri = channel_order == WHENET_BGR ? 2 : 0, bi = 2 - ri;
    const size_t rb = size_t(fw) * 3;
    std::vector<uint8_t> two_rows(2 * rb);
    uint8_t* const two = two_rows.data();
    for (int y0 = 0; y0 < fh; y0 += 2) {
        const int nrows = fh - y0 < 2 ? fh - y0 : 2;
        for (int r = 0; r < nrows; ++r) {
            const int y = y0 + r;
            uint8_t* row = two + r * rb;
            std::memcpy(row, frame + size_t(y) * rb, rb);
            for (int h = 0; h < k; ++h) {
                const int nseg = (flags[h] & OVERLAY_RECT) ? ((flags[h] & OVERLAY_AXES) ? 7 : 4) : 0;
                for (int s = 0; s < nseg; ++s) {
                    int px, py, qx, qy, colour;
                    overlay_head_segment(segs + size_t(h) * OVERLAY_SEG_INTS, s, px, py, qx, qy, colour);
                    const int ylo = (py < qy ? py : qy) - 1, yhi = (py > qy ? py : qy) + 1;
                    if (y < ylo || y > yhi) continue;
                    int xlo = (px < qx ? px : qx) - 1, xhi = (px > qx ? px : qx) + 1;
                    xlo = xlo < 0 ? 0 : xlo, xhi = xhi > fw - 1 ? fw - 1 : xhi;
                    const uint32_t c = overlay_colour(colour, channel_order);
                    for (int x = xlo; x <= xhi; ++x)
                        if (overlay_hit(px, py, qx, qy, x, y)) {
                            row[3 * x + 0] = uint8_t(c), row[3 * x + 1] = uint8_t(c >> 8), row[3 * x + 2] = uint8_t(c >> 16);
                        }
                }
                if (lines == nullptr || !(flags[h] & OVERLAY_LABELS)) continue;
                for (int l = 0; l < 3; ++l) {                      // the yaw, the pitch and the roll line, behind the head's segments
                    const OverlayLine& t = lines[size_t(h) * 3 + l];
                    const int ox = segs[size_t(h) * OVERLAY_SEG_INTS], oy = segs[size_t(h) * OVERLAY_SEG_INTS + 1] - OVERLAY_LINE_STEP * l;
                    if (y < oy + OVERLAY_GLYPH_TOP || y >= oy + OVERLAY_GLYPH_TOP + OVERLAY_GLYPH_ROWS) continue;
                    const int xlo = ox < 0 ? 0 : ox, xend = ox + OVERLAY_ADVANCE * overlay_line_length(t) - 1;
                    const uint32_t c = overlay_label_colour(channel_order);
                    for (int x = xlo; x < xend && x < fw; ++x)
                        if (overlay_text_hit(t, ox, oy, x, y)) {
                            row[3 * x + 0] = uint8_t(c), row[3 * x + 1] = uint8_t(c >> 8), row[3 * x + 2] = uint8_t(c >> 16);
                        }
                }
            }
            if (packed) {
                std::memcpy(static_cast<uint8_t*>(dst.plane[0]) + size_t(y) * size_t(dst.pitch[0]), row, rb);
            } else {
                uint8_t* yrow = static_cast<uint8_t*>(dst.plane[0]) + size_t(y) * size_t(dst.pitch[0]);
                for (int x = 0; x < fw; ++x) yrow[x] = uint8_t(overlay_luma(kc, row[3 * x + ri], row[3 * x + 1], row[3 * x + bi]));
            }
        }
        if (packed) continue;
        const int cy = y0 >> 1, cw = (fw + 1) >> 1;
        const bool nv12 = dst.format == WHENET_YUV_NV12;
        uint8_t* urow = static_cast<uint8_t*>(dst.plane[1]) + size_t(cy) * size_t(dst.pitch[1]);
        uint8_t* vrow = nv12 ? urow + 1 : static_cast<uint8_t*>(dst.plane[2]) + size_t(cy) * size_t(dst.pitch[2]);
        const int step = nv12 ? 2 : 1;
        for (int cx = 0; cx < cw; ++cx) {
            int rs = 0, gs = 0, bs = 0;
            for (int dy = 0; dy < 2; ++dy)
                for (int dxx = 0; dxx < 2; ++dxx) {
                    const int yy = (2 * cy + dy < fh - 1 ? 2 * cy + dy : fh - 1) - y0;
                    const int xx = 2 * cx + dxx < fw - 1 ? 2 * cx + dxx : fw - 1;
                    const uint8_t* p = two + size_t(yy) * rb + 3 * size_t(xx);
                    rs += p[ri], gs += p[1], bs += p[bi];
                }
            urow[cx * step] = uint8_t(overlay_cb(kc, rs, gs, bs));
            vrow[cx * step] = uint8_t(overlay_cr(kc, rs, gs, bs));
        }
    }
}

// whenet_annotate_host_ex behind its argument checks (display: WHENET_DISPLAY_SIMPLE or WHENET_DISPLAY_FULL)
inline void overlay_annotate_host(const uint8_t* frame, int fh, int fw, int channel_order, const int32_t* rects, const int32_t* valid,
                                  const float* ypr, int k, const whenet_surface_t& dst, int display = WHENET_DISPLAY_SIMPLE) {
    std::vector<int32_t> table(size_t(k > 0 ? k : 1) * (OVERLAY_SEG_INTS + 1));
    int32_t* const segs = table.data();
    int32_t* const flags = segs + size_t(k > 0 ? k : 1) * OVERLAY_SEG_INTS;
    std::vector<OverlayLine> lines(display == WHENET_DISPLAY_FULL ? size_t(k) * 3 : 0);
    for (int i = 0; i < k; ++i) {
        flags[i] = overlay_segments(rects + 4 * i, valid ? valid[i] : 1, double(ypr[3 * i]), double(ypr[3 * i + 1]), double(ypr[3 * i + 2]),
                                    segs + size_t(i) * OVERLAY_SEG_INTS);
        if (display == WHENET_DISPLAY_FULL) {
            int32_t origin[3][2];
            flags[i] |= overlay_labels(segs + size_t(i) * OVERLAY_SEG_INTS, flags[i], ypr[3 * i], ypr[3 * i + 1], ypr[3 * i + 2],
                                       lines.data() + size_t(i) * 3, origin);
        }
    }
    overlay_paint_host(frame, fh, fw, channel_order, segs, flags, k, dst, lines.empty() ? nullptr : lines.data());
}

}  // namespace whenet
