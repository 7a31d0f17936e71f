// The pose overlay as arithmetic, shared by the host statement (whenet_annotate_host, whenet_overlay_segments) and the kernels of
// overlay.hip: the segments of a head, the raster rule and the BGR -> 4:2:0 leg, each exactly as include/whenet_hip.h states it.
// Nothing here needs the HIP runtime: a plain C++17 compiler builds this header (tools/probes/overlay_host_probe.cpp does, under
// the host sanitizers).
//
// Reference: utils.py:13-43 (`draw_axis`: angles to radians, six sin / cos products, `int()` of every endpoint, three cv2.line calls
// of thickness 2) and demo_video.py:26-29 (`cv2.rectangle` of the window, colour (0,0,0), then draw_axis from the window's centre).
// The raster of a segment is the project's own rule (OpenCV has never run next to this code): distance to the closed segment <= 1.
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
enum { OVERLAY_RECT = 1, OVERLAY_AXES = 2 };  // flags of a head: what it paints

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

// the raster rule: is pixel (x, y) within distance 1 of the closed segment P -> Q?  64-bit integers, exact.
WHENET_HD inline bool overlay_hit(int px, int py, int qx, int qy, int x, int y) {
    const int64_t dx = qx - px, dy = qy - py, vx = x - px, vy = y - py;
    const int64_t L2 = dx * dx + dy * dy, t = vx * dx + vy * dy;
    if (t <= 0) return vx * vx + vy * vy <= 1;
    if (t >= L2) {
        const int64_t wx = x - qx, wy = y - qy;
        return wx * wx + wy * wy <= 1;
    }
    const int64_t c = vx * dy - vy * dx;
    return c * c <= L2;
}

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
// overlay_segments returns them; the surface's planes are host memory.  Only the rows' bytes are written.
inline void overlay_paint_host(const uint8_t* frame, int fh, int fw, int channel_order, const int32_t* segs, const int32_t* flags, int k,
                               const whenet_surface_t& dst) {
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

// whenet_annotate_host behind its argument checks
inline void overlay_annotate_host(const uint8_t* frame, int fh, int fw, int channel_order, const int32_t* rects, const int32_t* valid,
                                  const float* ypr, int k, const whenet_surface_t& dst) {
    std::vector<int32_t> table(size_t(k > 0 ? k : 1) * (OVERLAY_SEG_INTS + 1));
    int32_t* const segs = table.data();
    int32_t* const flags = segs + size_t(k > 0 ? k : 1) * OVERLAY_SEG_INTS;
    for (int i = 0; i < k; ++i)
        flags[i] = overlay_segments(rects + 4 * i, valid ? valid[i] : 1, double(ypr[3 * i]), double(ypr[3 * i + 1]), double(ypr[3 * i + 2]),
                                    segs + size_t(i) * OVERLAY_SEG_INTS);
    overlay_paint_host(frame, fh, fw, channel_order, segs, flags, k, dst);
}

}  // namespace whenet
