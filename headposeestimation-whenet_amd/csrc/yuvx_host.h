// The host side of the extended YUV ingest (include/whenet_hip_yuv_ext.h): the geometry of a frame's planes, the argument checks,
// the per-pixel function -- the SAME one the kernels of yuvx.hip run -- the host statement built on it, and the tight staging of a
// frame's planes that the upload form of the kernels reads.  Plain C++: no HIP runtime, so tools/yuvx_host_check.cpp builds it
// alone under the host sanitizers.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/whenet_hip_yuv_ext.h"

#if defined(__HIPCC__)
#define YUVX_HD __host__ __device__
#else
#define YUVX_HD
#endif

namespace whenet {

constexpr int YUVX_MAX_FRAME_SIDE = 8192;
constexpr int YUVX_MAX_FRAMES = 16;             // a clip (MIXED_MAX_FRAMES)

struct YuvxCoeffs {
    int yoff, cy, cvr, cug, cvg, cub;
};
inline const YuvxCoeffs* yuvx_coeffs_or_null(int matrix) {
    static const YuvxCoeffs table[WHENET_YUVX_MATRICES] = WHENET_YUVX_COEFFS;
    return matrix >= 0 && matrix < WHENET_YUVX_MATRICES ? &table[matrix] : nullptr;
}

// ---- geometry: the planes a layout has (1..3), plane p's rows and row bytes in a frame of h x w with bs = 1 or 2 bytes per sample
YUVX_HD inline bool yuvx_layout_packed(int layout) { return layout == WHENET_YUV_YUYV || layout == WHENET_YUV_UYVY; }
YUVX_HD inline bool yuvx_layout_known(int layout) {
    return layout == WHENET_YUV_NV12 || layout == WHENET_YUV_I420 || yuvx_layout_packed(layout) || layout == WHENET_YUVX_I444;
}
YUVX_HD inline int yuvx_plane_count(int layout) { return yuvx_layout_packed(layout) ? 1 : (layout == WHENET_YUV_NV12 ? 2 : 3); }
YUVX_HD inline int yuvx_plane_rows(int layout, int p, int h) { return p == 0 || layout == WHENET_YUVX_I444 ? h : (h + 1) >> 1; }
YUVX_HD inline int yuvx_plane_row_bytes(int layout, int p, int w, int bs) {
    const int cw = (w + 1) >> 1;
    if (yuvx_layout_packed(layout)) return 4 * cw;
    if (p == 0 || layout == WHENET_YUVX_I444) return w * bs;
    return (layout == WHENET_YUV_NV12 ? 2 * cw : cw) * bs;
}
// the bytes of a frame's planes lying TIGHT behind one another (every plane of a 16-bit frame then starts at an even offset from
// the first)
inline size_t yuvx_plane_bytes(int h, int w, int layout, int container) {
    size_t n = 0;
    for (int p = 0; p < yuvx_plane_count(layout); ++p)
        n += size_t(yuvx_plane_rows(layout, p, h)) * size_t(yuvx_plane_row_bytes(layout, p, w, container >> 3));
    return n;
}
// Where frame f's planes start in the staging / device plane buffer (src) and its BGR bytes in the frame buffer (dst).  The BGR
// frames lie back to back.  The planes lie back to back too, but for one padding byte in front of a 16-bit frame that would
// otherwise start at an odd offset (behind an odd-sized 8-bit frame of a mixed clip): its words are loaded as words.
struct YuvxLayout {
    size_t src[YUVX_MAX_FRAMES + 1] = {}, dst[YUVX_MAX_FRAMES + 1] = {}, end = 0;      // end: the bytes of all planes
    YuvxLayout(const whenet_yuvx_frame_t* frames, int nframes) {
        for (int f = 0; f < nframes; ++f) {
            const whenet_yuvx_frame_t& g = frames[f];
            src[f] = g.container == WHENET_YUVX_U16 ? (end + 1) & ~size_t(1) : end;
            end = src[f] + yuvx_plane_bytes(g.h, g.w, g.layout, g.container);
            dst[f + 1] = dst[f] + size_t(g.h) * g.w * 3;
        }
        src[nframes] = end;
    }
};

// ---- argument checks: "" or why frame i is refused (the text starts with "frame <i>")
inline std::string yuvx_check_frame(const whenet_yuvx_frame_t& f, int i) {
    const std::string who = "frame " + std::to_string(i);
    if (!yuvx_layout_known(f.layout))
        return who + ": unknown layout " + std::to_string(f.layout) +
               " (WHENET_YUV_NV12, WHENET_YUV_I420, WHENET_YUV_YUYV, WHENET_YUV_UYVY or WHENET_YUVX_I444)";
    if (f.container != WHENET_YUVX_U8 && f.container != WHENET_YUVX_U16)
        return who + ": unknown container " + std::to_string(f.container) + " (WHENET_YUVX_U8 or WHENET_YUVX_U16)";
    if (f.matrix < 0 || f.matrix >= WHENET_YUVX_MATRICES)
        return who + ": unknown matrix " + std::to_string(f.matrix) + " (WHENET_YUV_BT601, _BT709, _JFIF or _BT2020)";
    if (f.shift < 0 || f.shift > WHENET_YUVX_MAX_SHIFT) return who + ": shift " + std::to_string(f.shift) + " is outside 0..8";
    if (f.shift != 0 && f.container == WHENET_YUVX_U8)
        return who + ": shift " + std::to_string(f.shift) + " with an 8-bit container (a shift belongs to 16-bit samples)";
    if (yuvx_layout_packed(f.layout) && f.container != WHENET_YUVX_U8)
        return who + ": a packed layout has an 8-bit container (Y210 / Y216 are not built)";
    if (f.h < 1 || f.w < 1 || f.h > YUVX_MAX_FRAME_SIDE || f.w > YUVX_MAX_FRAME_SIDE)
        return who + " is " + std::to_string(f.h) + " x " + std::to_string(f.w) + ": sides must be 1.." + std::to_string(YUVX_MAX_FRAME_SIDE);
    for (int p = 0; p < yuvx_plane_count(f.layout); ++p) {
        const int row_bytes = yuvx_plane_row_bytes(f.layout, p, f.w, f.container >> 3);
        if (f.plane[p] == nullptr) return who + ": plane " + std::to_string(p) + " is NULL";
        if (f.pitch[p] < row_bytes)
            return who + ": pitch " + std::to_string(f.pitch[p]) + " of plane " + std::to_string(p) + " is below its row of " +
                   std::to_string(row_bytes) + " bytes";
        if (f.container == WHENET_YUVX_U16 && (reinterpret_cast<uintptr_t>(f.plane[p]) & 1))
            return who + ": plane " + std::to_string(p) + " of 16-bit samples lies at an odd address";
        if (f.container == WHENET_YUVX_U16 && (f.pitch[p] & 1))
            return who + ": pitch " + std::to_string(f.pitch[p]) + " of plane " + std::to_string(p) + " of 16-bit samples is odd";
    }
    return "";
}
// "" or the refusal of a frame list, `what` (the caller's name) in front
inline std::string yuvx_check_frames(const char* what, const whenet_yuvx_frame_t* frames, int nframes) {
    const std::string w = what;
    if (frames == nullptr) return w + ": NULL argument";
    if (nframes < 1 || nframes > YUVX_MAX_FRAMES)
        return w + ": " + std::to_string(nframes) + " frames: a clip holds 1..16 (the detector's batch limit)";
    for (int i = 0; i < nframes; ++i) {
        const std::string bad = yuvx_check_frame(frames[i], i);
        if (!bad.empty()) return w + ": " + bad;
    }
    return "";
}

// ---- the per-pixel function.  WIDE: samples at 16 bits (the statement of whenet_hip_yuv_ext.h, 64-bit terms); otherwise samples
// at 8 bits (the statement of whenet_hip.h, int32).  The chroma terms of a sample are built once and serve every pixel that takes it.
template <bool WIDE> struct YuvxAcc { using type = int; };
template <> struct YuvxAcc<true> { using type = long long; };
template <bool WIDE> struct YuvxTerms {
    typename YuvxAcc<WIDE>::type r, g, b;
};
YUVX_HD inline int yuvx_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
template <bool WIDE> YUVX_HD inline YuvxTerms<WIDE> yuvx_terms(const YuvxCoeffs& k, int u, int v) {
    using A = typename YuvxAcc<WIDE>::type;
    const A d = u - (WIDE ? 32768 : 128), e = v - (WIDE ? 32768 : 128);
    return {A(k.cvr) * e, -A(k.cug) * d - A(k.cvg) * e, A(k.cub) * d};
}
// B | G << 8 | R << 16
template <bool WIDE> YUVX_HD inline uint32_t yuvx_pixel(const YuvxCoeffs& k, int y, const YuvxTerms<WIDE>& c) {
    using A = typename YuvxAcc<WIDE>::type;
    constexpr int SH = WIDE ? 28 : 20;
    int l = y - (WIDE ? k.yoff << 8 : k.yoff);
    l = l < 0 ? 0 : l;
    const A base = A(k.cy) * l + (A(1) << (SH - 1));
    const uint32_t b = uint32_t(yuvx_clip8(int((base + c.b) >> SH)));
    const uint32_t g = uint32_t(yuvx_clip8(int((base + c.g) >> SH)));
    const uint32_t r = uint32_t(yuvx_clip8(int((base + c.r) >> SH)));
    return b | (g << 8) | (r << 16);
}
// the sample a stored 16-bit word stands for: MSB-aligned at 16 bits
YUVX_HD inline int yuvx_sample16(uint32_t word, int shift) { return int((word << shift) & 0xFFFFu); }

// ---- the host statement: bgr = uint8 [h][w][3].  The frame has passed yuvx_check_frame.
namespace yuvx_detail {
inline int fetch(const uint8_t* row, int i, bool wide, int shift) {      // sample i of a row
    if (!wide) return row[i];
    return yuvx_sample16(uint32_t(row[2 * i]) | (uint32_t(row[2 * i + 1]) << 8), shift);
}
template <bool WIDE> inline void put(const YuvxCoeffs& k, int y, int u, int v, uint8_t* out) {
    const uint32_t px = yuvx_pixel<WIDE>(k, y, yuvx_terms<WIDE>(k, u, v));
    out[0] = uint8_t(px), out[1] = uint8_t(px >> 8), out[2] = uint8_t(px >> 16);
}
}  // namespace yuvx_detail

inline void yuvx_to_bgr_host(const whenet_yuvx_frame_t& f, uint8_t* bgr) {
    using namespace yuvx_detail;
    const YuvxCoeffs& k = *yuvx_coeffs_or_null(f.matrix);
    const bool wide = f.container == WHENET_YUVX_U16;
    for (int y = 0; y < f.h; ++y) {
        uint8_t* out = bgr + size_t(y) * f.w * 3;
        const uint8_t* yrow = f.plane[0] + size_t(y) * f.pitch[0];
        if (yuvx_layout_packed(f.layout)) {         // pair x >> 1 of the pixel's own row: Y0 U Y1 V, or U Y0 V Y1
            const int yat = f.layout == WHENET_YUV_YUYV ? 0 : 1, uat = 1 - yat, vat = 3 - yat;
            for (int x = 0; x < f.w; ++x) {
                const uint8_t* pair = yrow + 4 * (x >> 1);
                put<false>(k, pair[yat + 2 * (x & 1)], pair[uat], pair[vat], out + 3 * x);
            }
            continue;
        }
        const bool full = f.layout == WHENET_YUVX_I444, nv12 = f.layout == WHENET_YUV_NV12;
        const size_t crow = full ? size_t(y) : size_t(y >> 1);
        const uint8_t* urow = f.plane[1] + crow * f.pitch[1];
        const uint8_t* vrow = nv12 ? urow : f.plane[2] + crow * f.pitch[2];
        for (int x = 0; x < f.w; ++x) {
            const int cx = full ? x : x >> 1;
            const int yy = fetch(yrow, x, wide, f.shift);
            const int u = fetch(urow, nv12 ? 2 * cx : cx, wide, f.shift), v = fetch(vrow, nv12 ? 2 * cx + 1 : cx, wide, f.shift);
            if (wide) put<true>(k, yy, u, v, out + 3 * x);
            else put<false>(k, yy, u, v, out + 3 * x);
        }
    }
}

// the tight copy of a frame's planes that the device reads: yuvx_plane_bytes() bytes at dst
inline void yuvx_stage_planes(const whenet_yuvx_frame_t& f, uint8_t* dst) {
    for (int p = 0; p < yuvx_plane_count(f.layout); ++p) {
        const size_t rb = size_t(yuvx_plane_row_bytes(f.layout, p, f.w, f.container >> 3));
        const int rows = yuvx_plane_rows(f.layout, p, f.h);
        if (size_t(f.pitch[p]) == rb) {
            std::memcpy(dst, f.plane[p], rb * rows);
        } else {
            for (int r = 0; r < rows; ++r) std::memcpy(dst + r * rb, f.plane[p] + size_t(r) * f.pitch[p], rb);
        }
        dst += rb * rows;
    }
}

}  // namespace whenet
