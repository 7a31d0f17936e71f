// Frame ingest from a video decoder: 4:2:0 YUV planes (NV12 / I420) -> the packed BGR frame [h][w][3] that the rest of the frame
// path reads (letterbox.hip, frame.hip).  The conversion is the integer form stated in include/whenet_hip.h: 20 fractional bits,
// nearest-neighbour chroma (pixel (y, x) takes the sample (y >> 1, x >> 1)), the coefficient rows WHENET_YUV_COEFFS.  And from a
// camera: packed 4:2:2 frames (YUYV / UYVY), the same arithmetic with every row's own chroma -- yuv_item_packed below, on the same
// item grid and through the same store stage.
//
// A thread owns 4 horizontally adjacent pixels on the two rows of one chroma row: the two chroma pairs are fetched once (one dword
// of an NV12 row), each luma row is one dword, and the 12 output bytes of a row leave as three dwords.  Adjacent lanes own
// adjacent groups, so a wave reads 256 contiguous luma bytes per row and writes 768 contiguous output bytes.
//
// Nothing here assumes an alignment: in a mixed clip the frames lie back to back, so a frame's planes, its first output byte and
// its row pitch 3 w are aligned to nothing in general.  A dword load is taken only where the address is a multiple of 4 and the
// four bytes belong to the row; otherwise the bytes are read one by one.  An output row whose address is r mod 4 stores 4 - r head
// bytes, two aligned dwords (the 12 bytes funnel-shifted) and r tail bytes.  The last group of a row (1..3 pixels when w is no
// multiple of 4) stores its own bytes one by one: no thread writes a byte outside its pixels, the neighbouring frame starts there.
//
// Two sources.  The host-pointer entry points stage a frame's planes TIGHT in one device buffer (kernels.h) and launch the first
// three kernels.  whenet_yuv_planes_to_bgr_kernel reads planes that are already in device memory where they are -- a decoder's
// surface, a tensor: three pointers and three pitches per frame -- through the same per-item function, which takes the planes'
// addresses and pitches as arguments; the tight form calls it with the pitches w, 2 cw / cw, cw.
#include <algorithm>
#include <cstring>

#include "kernels.h"

namespace whenet {

namespace {

constexpr int THREADS = 256;
constexpr int SHIFT = 20;

__host__ __device__ inline int yuv_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// the 12 bytes B G R of 4 pixels (luma y4: one byte per pixel; chroma terms of pixels 0-1 and 2-3) as three little-endian dwords
struct ChromaTerms {
    int r, g, b;
};
__device__ __forceinline__ ChromaTerms chroma_terms(const YuvCoeffs& k, int u, int v) {
    const int d = u - 128, e = v - 128;
    return {k.cvr * e, -k.cug * d - k.cvg * e, k.cub * d};
}
__device__ __forceinline__ uint32_t pixel_bgr(const YuvCoeffs& k, int y, const ChromaTerms& c) {
    int l = y - k.yoff;
    l = l < 0 ? 0 : l;
    const int base = k.cy * l + (1 << (SHIFT - 1));
    const uint32_t b = uint32_t(yuv_clip8((base + c.b) >> SHIFT));
    const uint32_t g = uint32_t(yuv_clip8((base + c.g) >> SHIFT));
    const uint32_t r = uint32_t(yuv_clip8((base + c.r) >> SHIFT));
    return b | (g << 8) | (r << 16);
}

#include "yuv_store.h"      // funnel, store_group: the output stage, shared with yuvx.hip

// one item of a frame: group gx (pixels 4 gx ..) of chroma row p (luma rows 2 p, 2 p + 1).  The planes are wherever they are:
// luma rows pitch_y bytes apart at py; NV12: interleaved rows pitch_u apart at pu (pv unused); I420: U rows pitch_u apart at pu,
// V rows pitch_v apart at pv.
__device__ __forceinline__ void yuv_item_planes(const uint8_t* __restrict__ py, const uint8_t* __restrict__ pu, const uint8_t* __restrict__ pv,
                                                size_t pitch_y, size_t pitch_u, size_t pitch_v, uint8_t* __restrict__ bgr, int h, int w,
                                                int format, const YuvCoeffs& k, int item) {
    const int ch = (h + 1) >> 1, gw = (w + 3) >> 2;
    const int p = item / gw, gx = item - p * gw;
    if (p >= ch) return;
    const int x = gx << 2;
    const int n = min(4, w - x);                    // pixels of the group, 1..4
    const int y0 = p << 1;
    const int rows = min(2, h - y0);
    const int cx = x >> 1;
    const bool two = n > 2;                         // the group has a second chroma sample (cx + 1 < cw)

    int u0, v0, u1, v1;
    if (format == WHENET_YUV_NV12) {
        const uint8_t* c = pu + size_t(p) * pitch_u + 2 * cx;
        if (two && (reinterpret_cast<uintptr_t>(c) & 3) == 0) {
            const uint32_t q = *reinterpret_cast<const uint32_t*>(c);
            u0 = q & 255, v0 = (q >> 8) & 255, u1 = (q >> 16) & 255, v1 = q >> 24;
        } else {
            u0 = c[0], v0 = c[1];
            u1 = two ? int(c[2]) : u0, v1 = two ? int(c[3]) : v0;
        }
    } else {
        const uint8_t* cu = pu + size_t(p) * pitch_u + cx;
        const uint8_t* cv = pv + size_t(p) * pitch_v + cx;
        if (two && ((reinterpret_cast<uintptr_t>(cu) | reinterpret_cast<uintptr_t>(cv)) & 1) == 0) {
            const uint32_t qu = *reinterpret_cast<const uint16_t*>(cu), qv = *reinterpret_cast<const uint16_t*>(cv);
            u0 = qu & 255, u1 = qu >> 8, v0 = qv & 255, v1 = qv >> 8;
        } else {
            u0 = cu[0], v0 = cv[0];
            u1 = two ? int(cu[1]) : u0, v1 = two ? int(cv[1]) : v0;
        }
    }
    const ChromaTerms c0 = chroma_terms(k, u0, v0), c1 = chroma_terms(k, u1, v1);

    for (int r = 0; r < rows; ++r) {
        const uint8_t* yp = py + size_t(y0 + r) * pitch_y + x;
        uint32_t y4;
        if (n == 4 && (reinterpret_cast<uintptr_t>(yp) & 3) == 0) {
            y4 = *reinterpret_cast<const uint32_t*>(yp);
        } else {
            y4 = yp[0];
            if (n > 1) y4 |= uint32_t(yp[1]) << 8;
            if (n > 2) y4 |= uint32_t(yp[2]) << 16;
            if (n > 3) y4 |= uint32_t(yp[3]) << 24;
        }
        const uint32_t p0 = pixel_bgr(k, y4 & 255, c0), p1 = pixel_bgr(k, (y4 >> 8) & 255, c0);
        const uint32_t p2 = pixel_bgr(k, (y4 >> 16) & 255, c1), p3 = pixel_bgr(k, y4 >> 24, c1);
        store_group(bgr + (size_t(y0 + r) * w + x) * 3, n, p0, p1, p2, p3);
    }
}

// The same item of a PACKED 4:2:2 frame (YUYV: Y0 U Y1 V per pixel pair, UYVY: U Y0 V Y1): rows of 4 cw bytes, `pitch` bytes apart
// at src.  The group's 4 pixels are 2 pairs = 8 source bytes at 2 x of each row (one pair = 4 bytes where n <= 2: the row ends
// there, and the last pair of an odd row is whole in memory).  Every row has its own chroma, so both ChromaTerms are built per row.
// One 8-byte load where the address is a multiple of 8 and the 8 bytes belong to the row, dwords at a multiple of 4, bytes otherwise:
// adjacent lanes own adjacent groups, so a wave reads 512 contiguous source bytes per row and writes 768.
__device__ __forceinline__ void yuv_item_packed(const uint8_t* __restrict__ src, size_t pitch, uint8_t* __restrict__ bgr, int h, int w, int format,
                                                const YuvCoeffs& k, int item) {
    const int ch = (h + 1) >> 1, gw = (w + 3) >> 2;
    const int p = item / gw, gx = item - p * gw;
    if (p >= ch) return;
    const int x = gx << 2;
    const int n = min(4, w - x);                    // pixels of the group, 1..4
    const int y0 = p << 1;
    const int rows = min(2, h - y0);
    const bool two = n > 2;                         // the group has a second pair (x / 2 + 1 < cw)

    for (int r = 0; r < rows; ++r) {
        const uint8_t* sp = src + size_t(y0 + r) * pitch + 2 * size_t(x);
        const uintptr_t a = reinterpret_cast<uintptr_t>(sp);
        uint32_t q0, q1 = 0;
        if (two && (a & 7) == 0) {
            const uint2 q = *reinterpret_cast<const uint2*>(sp);
            q0 = q.x, q1 = q.y;
        } else if ((a & 3) == 0) {
            q0 = *reinterpret_cast<const uint32_t*>(sp);
            if (two) q1 = *reinterpret_cast<const uint32_t*>(sp + 4);
        } else {
            q0 = uint32_t(sp[0]) | (uint32_t(sp[1]) << 8) | (uint32_t(sp[2]) << 16) | (uint32_t(sp[3]) << 24);
            if (two) q1 = uint32_t(sp[4]) | (uint32_t(sp[5]) << 8) | (uint32_t(sp[6]) << 16) | (uint32_t(sp[7]) << 24);
        }
        if (format == WHENET_YUV_UYVY) {            // U Y0 V Y1 -> Y0 U Y1 V: the bytes of every 16-bit half swapped
            q0 = ((q0 >> 8) & 0x00FF00FFu) | ((q0 & 0x00FF00FFu) << 8);
            q1 = ((q1 >> 8) & 0x00FF00FFu) | ((q1 & 0x00FF00FFu) << 8);
        }
        if (!two) q1 = q0;                          // (pixels 2, 3 are not stored)
        const ChromaTerms c0 = chroma_terms(k, (q0 >> 8) & 255, q0 >> 24), c1 = chroma_terms(k, (q1 >> 8) & 255, q1 >> 24);
        const uint32_t p0 = pixel_bgr(k, q0 & 255, c0), p1 = pixel_bgr(k, (q0 >> 16) & 255, c0);
        const uint32_t p2 = pixel_bgr(k, q1 & 255, c1), p3 = pixel_bgr(k, (q1 >> 16) & 255, c1);
        store_group(bgr + (size_t(y0 + r) * w + x) * 3, n, p0, p1, p2, p3);
    }
}

__device__ __forceinline__ bool packed_format(int format) { return format == WHENET_YUV_YUYV || format == WHENET_YUV_UYVY; }

// the same item of a frame whose planes lie TIGHT behind one another at `planes` (kernels.h).  The format is the frame's and a
// workgroup belongs to one frame: the branch is the same in every lane.
__device__ __forceinline__ void yuv_item(const uint8_t* __restrict__ planes, uint8_t* __restrict__ bgr, const YuvGeom& g, int item) {
    const size_t cw = size_t((g.w + 1) >> 1), ch = size_t((g.h + 1) >> 1);
    if (packed_format(g.format)) {
        yuv_item_packed(planes, 4 * cw, bgr, g.h, g.w, g.format, g.k, item);
        return;
    }
    const uint8_t* const chroma = planes + size_t(g.h) * g.w;
    const bool nv12 = g.format == WHENET_YUV_NV12;
    yuv_item_planes(planes, chroma, chroma + ch * cw, size_t(g.w), nv12 ? 2 * cw : cw, cw, bgr, g.h, g.w, g.format, g.k, item);
}

__global__ __launch_bounds__(THREADS) void whenet_yuv_to_bgr_kernel(const uint8_t* __restrict__ planes, uint8_t* __restrict__ bgr, YuvGeom g) {
    yuv_item(planes + g.src_off, bgr + g.dst_off, g, int(blockIdx.x) * THREADS + int(threadIdx.x));
}

// F frames of one size, format and matrix: the frame is grid dimension y
__global__ __launch_bounds__(THREADS) void whenet_yuv_to_bgr_batch_kernel(const uint8_t* __restrict__ planes, uint8_t* __restrict__ bgr, YuvGeom g,
                                                                          unsigned long long src_stride, unsigned long long dst_stride) {
    const size_t f = blockIdx.y;
    yuv_item(planes + g.src_off + f * src_stride, bgr + g.dst_off + f * dst_stride, g, int(blockIdx.x) * THREADS + int(threadIdx.x));
}

// Frames of their own sizes: workgroup b belongs to the last frame whose block0 is <= b (a scan of at most 16 values, the same in
// every lane)
__global__ __launch_bounds__(THREADS) void whenet_yuv_to_bgr_mixed_kernel(const uint8_t* __restrict__ planes, uint8_t* __restrict__ bgr, YuvMixed clip) {
    const int b = int(blockIdx.x);
    int f = 0;
    for (int i = 1; i < clip.frames; ++i)
        if (clip.f[i].block0 <= b) f = i;
    const YuvGeom& g = clip.f[f];
    yuv_item(planes + g.src_off, bgr + g.dst_off, g, (b - g.block0) * THREADS + int(threadIdx.x));
}

// Planes where a decoder (or a tensor) left them in device memory, each with its own pitch: the records travel by value in the
// argument block, the frame of a workgroup is found as in the mixed kernel above
__global__ __launch_bounds__(THREADS) void whenet_yuv_planes_to_bgr_kernel(uint8_t* __restrict__ bgr, YuvPlanes clip) {
    const int b = int(blockIdx.x);
    int f = 0;
    for (int i = 1; i < clip.frames; ++i)
        if (clip.f[i].block0 <= b) f = i;
    const YuvPlanesFrame& g = clip.f[f];
    if (packed_format(g.format)) {
        yuv_item_packed(g.plane[0], size_t(g.pitch[0]), bgr + g.dst_off, g.h, g.w, g.format, g.k, (b - g.block0) * THREADS + int(threadIdx.x));
        return;
    }
    yuv_item_planes(g.plane[0], g.plane[1], g.plane[2], size_t(g.pitch[0]), size_t(g.pitch[1]), size_t(g.pitch[2]), bgr + g.dst_off, g.h, g.w,
                    g.format, g.k, (b - g.block0) * THREADS + int(threadIdx.x));
}

int yuv_blocks(int h, int w) { return (((w + 3) >> 2) * ((h + 1) >> 1) + THREADS - 1) / THREADS; }

void check_geom(const YuvGeom& g) {
    WHENET_REQUIRE(g.h >= 1 && g.w >= 1 && g.h <= YUV_MAX_FRAME_SIDE && g.w <= YUV_MAX_FRAME_SIDE &&
                       (g.format == WHENET_YUV_NV12 || g.format == WHENET_YUV_I420 || yuv_is_packed(g.format)),
                   WHENET_EINVAL, "yuv_to_bgr: bad frame geometry");
}

}  // namespace

const YuvCoeffs& yuv_coeffs(int matrix) {
    static const YuvCoeffs table[WHENET_YUV_MATRICES] = WHENET_YUV_COEFFS;
    WHENET_REQUIRE(matrix >= 0 && matrix < WHENET_YUV_MATRICES, WHENET_EINVAL, "unknown YUV matrix " + std::to_string(matrix));
    return table[matrix];
}

void check_yuv_frames(const char* what, const whenet_yuv_frame_t* frames, int nframes) {
    const std::string w = what;
    WHENET_REQUIRE(frames != nullptr, WHENET_EINVAL, w + ": NULL argument");
    WHENET_REQUIRE(nframes >= 1 && nframes <= MIXED_MAX_FRAMES, WHENET_EINVAL,
                   w + ": " + std::to_string(nframes) + " frames: a clip holds 1..16 (the detector's batch limit)");
    for (int i = 0; i < nframes; ++i) {
        const whenet_yuv_frame_t& f = frames[i];
        const std::string who = w + ": frame " + std::to_string(i);
        WHENET_REQUIRE(f.format == WHENET_YUV_NV12 || f.format == WHENET_YUV_I420 || yuv_is_packed(f.format), WHENET_EINVAL,
                       who + ": unknown format " + std::to_string(f.format) +
                           " (WHENET_YUV_NV12, WHENET_YUV_I420, WHENET_YUV_YUYV or WHENET_YUV_UYVY)");
        WHENET_REQUIRE(f.matrix >= 0 && f.matrix < WHENET_YUV_MATRICES, WHENET_EINVAL,
                       who + ": unknown matrix " + std::to_string(f.matrix) + " (WHENET_YUV_BT601, _BT709 or _JFIF)");
        WHENET_REQUIRE(f.h >= 1 && f.w >= 1 && f.h <= YUV_MAX_FRAME_SIDE && f.w <= YUV_MAX_FRAME_SIDE, WHENET_EINVAL,
                       who + " is " + std::to_string(f.h) + " x " + std::to_string(f.w) + ": sides must be 1.." +
                           std::to_string(YUV_MAX_FRAME_SIDE));
        for (int p = 0; p < yuv_plane_count(f.format); ++p) {
            const int row_bytes = yuv_plane_row_bytes(f.format, p, f.w);
            WHENET_REQUIRE(f.plane[p] != nullptr, WHENET_EINVAL, who + ": plane " + std::to_string(p) + " is NULL");
            WHENET_REQUIRE(f.pitch[p] >= row_bytes, WHENET_EINVAL,
                           who + ": pitch " + std::to_string(f.pitch[p]) + " of plane " + std::to_string(p) + " is below its row of " +
                               std::to_string(row_bytes) + " bytes");
        }
    }
}

void yuv_to_bgr_host(const whenet_yuv_frame_t& f, uint8_t* bgr) {
    const YuvCoeffs& k = yuv_coeffs(f.matrix);
    if (yuv_is_packed(f.format)) {                  // pair x >> 1 of the pixel's own row: Y0 U Y1 V, or U Y0 V Y1
        const int yat = f.format == WHENET_YUV_YUYV ? 0 : 1, uat = 1 - yat, vat = 3 - yat;
        for (int y = 0; y < f.h; ++y) {
            const uint8_t* row = f.plane[0] + size_t(y) * f.pitch[0];
            uint8_t* out = bgr + size_t(y) * f.w * 3;
            for (int x = 0; x < f.w; ++x) {
                const uint8_t* pair = row + 4 * (x >> 1);
                const int c = std::max(0, int(pair[yat + 2 * (x & 1)]) - k.yoff);
                const int d = int(pair[uat]) - 128, e = int(pair[vat]) - 128;
                const int base = k.cy * c + (1 << (SHIFT - 1));
                out[3 * x + 0] = uint8_t(yuv_clip8((base + k.cub * d) >> SHIFT));
                out[3 * x + 1] = uint8_t(yuv_clip8((base - k.cug * d - k.cvg * e) >> SHIFT));
                out[3 * x + 2] = uint8_t(yuv_clip8((base + k.cvr * e) >> SHIFT));
            }
        }
        return;
    }
    const bool nv12 = f.format == WHENET_YUV_NV12;
    for (int y = 0; y < f.h; ++y) {
        const uint8_t* yrow = f.plane[0] + size_t(y) * f.pitch[0];
        const uint8_t* urow = f.plane[1] + size_t(y >> 1) * f.pitch[1];
        const uint8_t* vrow = nv12 ? urow + 1 : f.plane[2] + size_t(y >> 1) * f.pitch[2];
        const int step = nv12 ? 2 : 1;
        uint8_t* out = bgr + size_t(y) * f.w * 3;
        for (int x = 0; x < f.w; ++x) {
            const int c = std::max(0, int(yrow[x]) - k.yoff);
            const int d = int(urow[(x >> 1) * step]) - 128, e = int(vrow[(x >> 1) * step]) - 128;
            const int base = k.cy * c + (1 << (SHIFT - 1));
            out[3 * x + 0] = uint8_t(yuv_clip8((base + k.cub * d) >> SHIFT));
            out[3 * x + 1] = uint8_t(yuv_clip8((base - k.cug * d - k.cvg * e) >> SHIFT));
            out[3 * x + 2] = uint8_t(yuv_clip8((base + k.cvr * e) >> SHIFT));
        }
    }
}

void yuv_stage_planes(const whenet_yuv_frame_t& f, uint8_t* dst) {
    for (int p = 0; p < yuv_plane_count(f.format); ++p) {
        const size_t rb = size_t(yuv_plane_row_bytes(f.format, p, f.w));
        const int rows = yuv_plane_rows(f.format, p, f.h);
        if (size_t(f.pitch[p]) == rb) {
            std::memcpy(dst, f.plane[p], rb * rows);
        } else {
            for (int r = 0; r < rows; ++r) std::memcpy(dst + r * rb, f.plane[p] + size_t(r) * f.pitch[p], rb);
        }
        dst += rb * rows;
    }
}

void launch_yuv_to_bgr(const uint8_t* d_planes, uint8_t* d_bgr, const YuvGeom& g, hipStream_t stream) {
    check_geom(g);
    hipLaunchKernelGGL(whenet_yuv_to_bgr_kernel, dim3(yuv_blocks(g.h, g.w)), dim3(THREADS), 0, stream, d_planes, d_bgr, g);
    WHENET_HIP_CHECK(hipGetLastError());
}

void launch_yuv_to_bgr_batch(const uint8_t* d_planes, uint8_t* d_bgr, const YuvGeom& g, int frames, size_t src_stride, size_t dst_stride,
                             hipStream_t stream) {
    check_geom(g);
    WHENET_REQUIRE(frames >= 1 && frames <= MIXED_MAX_FRAMES && src_stride >= yuv_plane_bytes(g.h, g.w, g.format) && dst_stride >= size_t(g.h) * g.w * 3,
                   WHENET_EINVAL, "yuv_to_bgr_batch: bad frame count or strides");
    hipLaunchKernelGGL(whenet_yuv_to_bgr_batch_kernel, dim3(yuv_blocks(g.h, g.w), frames), dim3(THREADS), 0, stream, d_planes, d_bgr, g,
                       (unsigned long long)src_stride, (unsigned long long)dst_stride);
    WHENET_HIP_CHECK(hipGetLastError());
}

// block0 / total_blocks are set here
void launch_yuv_to_bgr_mixed(const uint8_t* d_planes, uint8_t* d_bgr, YuvMixed clip, hipStream_t stream) {
    WHENET_REQUIRE(clip.frames >= 1 && clip.frames <= MIXED_MAX_FRAMES, WHENET_EINVAL, "yuv_to_bgr_mixed: 1..16 frames");
    int blocks = 0;
    for (int f = 0; f < clip.frames; ++f) {
        check_geom(clip.f[f]);
        clip.f[f].block0 = blocks;
        blocks += yuv_blocks(clip.f[f].h, clip.f[f].w);
    }
    clip.total_blocks = blocks;
    hipLaunchKernelGGL(whenet_yuv_to_bgr_mixed_kernel, dim3(blocks), dim3(THREADS), 0, stream, d_planes, d_bgr, clip);
    WHENET_HIP_CHECK(hipGetLastError());
}

// block0 / total_blocks are set here.  The callers have checked the planes (Engine::check_device_plane): the kernel reads
// rows x row bytes of each at its pitch and nothing else.
void launch_yuv_planes_to_bgr(uint8_t* d_bgr, YuvPlanes clip, hipStream_t stream) {
    WHENET_REQUIRE(clip.frames >= 1 && clip.frames <= MIXED_MAX_FRAMES, WHENET_EINVAL, "yuv_planes_to_bgr: 1..16 frames");
    int blocks = 0;
    for (int f = 0; f < clip.frames; ++f) {
        const YuvPlanesFrame& g = clip.f[f];
        bool good = g.h >= 1 && g.w >= 1 && g.h <= YUV_MAX_FRAME_SIDE && g.w <= YUV_MAX_FRAME_SIDE &&
                    (g.format == WHENET_YUV_NV12 || g.format == WHENET_YUV_I420 || yuv_is_packed(g.format));
        for (int p = 0; good && p < yuv_plane_count(g.format); ++p)
            good = g.plane[p] != nullptr && g.pitch[p] >= yuv_plane_row_bytes(g.format, p, g.w);
        WHENET_REQUIRE(good, WHENET_EINVAL, "yuv_planes_to_bgr: bad frame geometry");
        clip.f[f].block0 = blocks;
        blocks += yuv_blocks(g.h, g.w);
    }
    clip.total_blocks = blocks;
    hipLaunchKernelGGL(whenet_yuv_planes_to_bgr_kernel, dim3(blocks), dim3(THREADS), 0, stream, d_bgr, clip);
    WHENET_HIP_CHECK(hipGetLastError());
}

}  // namespace whenet
