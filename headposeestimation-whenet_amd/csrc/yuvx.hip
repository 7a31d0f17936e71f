// The extended YUV ingest (include/whenet_hip_yuv_ext.h): 16-bit sample containers (P010 / P016, I010 / yuv420p10le, a decoder's
// 16-bit surfaces), planar 4:4:4 (8 or 16 bit) and the four formats of yuv.hip, under four matrices -> the packed BGR frame
// [h][w][3] that the rest of the frame path reads.  The kernels of yuv.hip are not touched: this file has its own, and shares their
// store stage (yuv_store.h) and their item grid.
//
// The item grid is yuv.hip's: a lane owns 4 horizontally adjacent pixels on the two rows of one chroma row (4:4:4: on the same two
// rows, every row with its own chroma), adjacent lanes own adjacent groups, a workgroup belongs to one frame.  A group's luma is 8
// bytes per row in a 16-bit frame and so are the two interleaved chroma pairs of an NV12-like frame: one 8-byte load where the
// address is a multiple of 8 and the 8 bytes belong to the row, dwords where it is a multiple of 4, 16-bit words otherwise
// (load4_u16: the ladder of yuv.hip's yuv_item_packed, one rung up -- a 16-bit plane lies at an even address with an even pitch,
// whenet_hip_yuv_ext.h).  A wave then reads 512 contiguous source bytes per row.  An 8-bit 4:4:4 group is three dword loads per row.
// Every load takes exactly the group's samples (n = 1..4 in the last group of a row), every store goes through store_group: no
// lane reads behind a row or writes outside its pixels -- in a mixed clip the next frame starts there.
//
// The per-pixel function is yuvx_host.h's yuvx_terms / yuvx_pixel, the one the host statement runs: int32 for 8-bit samples (the
// statement of whenet_hip.h), 64-bit terms for 16-bit samples (CY * c reaches 2^36.2; the compiler forms each product from one
// v_mul_lo_u32 and one v_mul_hi_i32).  The chroma terms of a sample are built once per lane and serve its 2 x 2 pixels.
//
// Two forms, one per-item function (yuvx_dispatch).  whenet_yuvx_to_bgr_kernel reads planes staged TIGHT in the upload buffer
// (YuvxLayout: single frames, clips and mixed clips are all a list of 1..16 records); whenet_yuvx_planes_to_bgr_kernel reads planes
// where they are in device memory, three pointers and three byte pitches per frame.
//
// hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage (ROCm 7, this file as built by __graft_entry__.py):
//   whenet_yuvx_to_bgr_kernel          TotalSGPRs 66  VGPRs 41  ScratchSize 0 bytes/lane  Occupancy 8 waves/SIMD  LDS 0 bytes/block
//   whenet_yuvx_planes_to_bgr_kernel   TotalSGPRs 66  VGPRs 41  ScratchSize 0 bytes/lane  Occupancy 8 waves/SIMD  LDS 0 bytes/block
// (yuv.hip's four kernels report what they reported before this file existed: 47 / 47 / 46 / 46 SGPRs, 32 / 32 / 32 / 31 VGPRs, no scratch.)
#include <algorithm>

#include "kernels.h"

namespace whenet {

namespace {

constexpr int THREADS = 256;

#include "yuv_store.h"      // funnel, store_group: the output stage of yuv.hip, its text unchanged

struct S4 {
    int a, b, c, d;
};

// n = 1..4 bytes at p (any address): one dword where p is a multiple of 4 and the row holds all four, bytes otherwise
__device__ __forceinline__ S4 load4_u8(const uint8_t* __restrict__ p, int n) {
    uint32_t q;
    if (n == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        q = *reinterpret_cast<const uint32_t*>(p);
    } else {
        q = p[0];
        if (n > 1) q |= uint32_t(p[1]) << 8;
        if (n > 2) q |= uint32_t(p[2]) << 16;
        if (n > 3) q |= uint32_t(p[3]) << 24;
    }
    return {int(q & 255), int((q >> 8) & 255), int((q >> 16) & 255), int(q >> 24)};
}

// n = 1..4 little-endian 16-bit words at p (an even address), each as the sample it stands for: 8 bytes at a multiple of 8 where
// the row holds all four, dwords at a multiple of 4 (a last odd word on its own), words otherwise.  Exactly 2 n bytes are read.
__device__ __forceinline__ S4 load4_u16(const uint8_t* __restrict__ p, int n, int shift) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    uint32_t q0, q1 = 0;
    if (n == 4 && (a & 7) == 0) {
        const uint2 q = *reinterpret_cast<const uint2*>(p);
        q0 = q.x, q1 = q.y;
    } else if ((a & 3) == 0) {
        q0 = n > 1 ? *reinterpret_cast<const uint32_t*>(p) : uint32_t(*reinterpret_cast<const uint16_t*>(p));
        if (n > 2) q1 = n > 3 ? *reinterpret_cast<const uint32_t*>(p + 4) : uint32_t(*reinterpret_cast<const uint16_t*>(p + 4));
    } else {
        const uint16_t* s = reinterpret_cast<const uint16_t*>(p);
        q0 = s[0];
        if (n > 1) q0 |= uint32_t(s[1]) << 16;
        if (n > 2) q1 = s[2];
        if (n > 3) q1 |= uint32_t(s[3]) << 16;
    }
    return {yuvx_sample16(q0 & 0xFFFFu, shift), yuvx_sample16(q0 >> 16, shift), yuvx_sample16(q1 & 0xFFFFu, shift),
            yuvx_sample16(q1 >> 16, shift)};
}

template <bool WIDE> __device__ __forceinline__ S4 load4(const uint8_t* __restrict__ p, int n, int shift) {
    if constexpr (WIDE) return load4_u16(p, n, shift);
    else return load4_u8(p, n);
}

enum { K_NV12 = 0, K_I420 = 1, K_PACKED = 2, K_I444 = 3 };

// one item of a frame: group gx (pixels 4 gx ..) of row pair p (rows 2 p, 2 p + 1).  The planes are wherever they are, rows
// pitch_* bytes apart.  K_NV12: pu = the interleaved plane (pv unused); K_PACKED: py = the one plane, uyvy tells the byte order.
template <int KIND, bool WIDE>
__device__ __forceinline__ void yuvx_item(const uint8_t* __restrict__ py, const uint8_t* __restrict__ pu, const uint8_t* __restrict__ pv,
                                          size_t pitch_y, size_t pitch_u, size_t pitch_v, uint8_t* __restrict__ bgr, int h, int w, bool uyvy,
                                          int shift, const YuvxCoeffs& k, int item) {
    constexpr int BS = WIDE ? 2 : 1;                // bytes per sample
    const int ch = (h + 1) >> 1, gw = (w + 3) >> 2;
    const int p = item / gw, gx = item - p * gw;
    if (p >= ch) return;
    const int x = gx << 2;
    const int n = min(4, w - x);                    // pixels of the group, 1..4
    const int y0 = p << 1;
    const int rows = min(2, h - y0);
    const int cx = x >> 1;
    const bool two = n > 2;                         // the group has a second chroma sample / pixel pair

    YuvxTerms<WIDE> t0{}, t1{}, t2{}, t3{};         // the chroma terms of pixels 0..3 (4:2:0 and 4:2:2: t0 for 0-1, t1 for 2-3)
    if constexpr (KIND == K_NV12) {
        const S4 q = load4<WIDE>(pu + size_t(p) * pitch_u + size_t(2 * cx) * BS, two ? 4 : 2, shift);
        t0 = yuvx_terms<WIDE>(k, q.a, q.b);
        t1 = two ? yuvx_terms<WIDE>(k, q.c, q.d) : t0;
    } else if constexpr (KIND == K_I420) {
        const S4 qu = load4<WIDE>(pu + size_t(p) * pitch_u + size_t(cx) * BS, two ? 2 : 1, shift);
        const S4 qv = load4<WIDE>(pv + size_t(p) * pitch_v + size_t(cx) * BS, two ? 2 : 1, shift);
        t0 = yuvx_terms<WIDE>(k, qu.a, qv.a);
        t1 = two ? yuvx_terms<WIDE>(k, qu.b, qv.b) : t0;
    }

    for (int r = 0; r < rows; ++r) {
        const size_t row = size_t(y0 + r);
        S4 yq;
        if constexpr (KIND == K_PACKED) {           // 2 pairs = 8 bytes at 2 x; the last pair of an odd row is whole in memory
            const uint8_t* sp = py + row * pitch_y + 2 * size_t(x);
            const S4 a = load4_u8(sp, 4), b = two ? load4_u8(sp + 4, 4) : a;
            yq = uyvy ? S4{a.b, a.d, b.b, b.d} : S4{a.a, a.c, b.a, b.c};
            t0 = uyvy ? yuvx_terms<false>(k, a.a, a.c) : yuvx_terms<false>(k, a.b, a.d);
            t1 = uyvy ? yuvx_terms<false>(k, b.a, b.c) : yuvx_terms<false>(k, b.b, b.d);
        } else {
            if constexpr (KIND == K_I444) {
                const S4 qu = load4<WIDE>(pu + row * pitch_u + size_t(x) * BS, n, shift);
                const S4 qv = load4<WIDE>(pv + row * pitch_v + size_t(x) * BS, n, shift);
                t0 = yuvx_terms<WIDE>(k, qu.a, qv.a), t1 = yuvx_terms<WIDE>(k, qu.b, qv.b);
                t2 = yuvx_terms<WIDE>(k, qu.c, qv.c), t3 = yuvx_terms<WIDE>(k, qu.d, qv.d);
            }
            yq = load4<WIDE>(py + row * pitch_y + size_t(x) * BS, n, shift);
        }
        constexpr bool OWN = KIND == K_I444;        // every pixel has its own chroma sample
        const uint32_t p0 = yuvx_pixel<WIDE>(k, yq.a, t0), p1 = yuvx_pixel<WIDE>(k, yq.b, OWN ? t1 : t0);
        const uint32_t p2 = yuvx_pixel<WIDE>(k, yq.c, OWN ? t2 : t1), p3 = yuvx_pixel<WIDE>(k, yq.d, OWN ? t3 : t1);
        store_group(bgr + (row * w + x) * 3, n, p0, p1, p2, p3);
    }
}

// the item of a frame of any layout and container.  A workgroup belongs to one frame: the branches are the same in every lane.
__device__ __forceinline__ void yuvx_dispatch(const uint8_t* __restrict__ py, const uint8_t* __restrict__ pu, const uint8_t* __restrict__ pv,
                                              size_t pitch_y, size_t pitch_u, size_t pitch_v, uint8_t* __restrict__ bgr, const YuvxFrame& g,
                                              int item) {
    const bool wide = g.container == WHENET_YUVX_U16;
#define YUVX_ITEM(KIND, WIDE) yuvx_item<KIND, WIDE>(py, pu, pv, pitch_y, pitch_u, pitch_v, bgr, g.h, g.w, g.layout == WHENET_YUV_UYVY, g.shift, g.k, item)
    if (g.layout == WHENET_YUV_NV12) {
        if (wide) YUVX_ITEM(K_NV12, true);
        else YUVX_ITEM(K_NV12, false);
    } else if (g.layout == WHENET_YUV_I420) {
        if (wide) YUVX_ITEM(K_I420, true);
        else YUVX_ITEM(K_I420, false);
    } else if (g.layout == WHENET_YUVX_I444) {
        if (wide) YUVX_ITEM(K_I444, true);
        else YUVX_ITEM(K_I444, false);
    } else {
        YUVX_ITEM(K_PACKED, false);
    }
#undef YUVX_ITEM
}

// workgroup b belongs to the last frame whose block0 is <= b (a scan of at most 16 values, the same in every lane)
__device__ __forceinline__ int frame_of_block(const YuvxClip& clip, int b) {
    int f = 0;
    for (int i = 1; i < clip.frames; ++i)
        if (clip.f[i].block0 <= b) f = i;
    return f;
}

// planes staged tight in the upload buffer: plane p of a frame starts where plane p - 1 ends, its pitch is its row
__global__ __launch_bounds__(THREADS) void whenet_yuvx_to_bgr_kernel(const uint8_t* __restrict__ planes, uint8_t* __restrict__ bgr, YuvxClip clip) {
    const int b = int(blockIdx.x);
    const YuvxFrame& g = clip.f[frame_of_block(clip, b)];
    const int bs = g.container >> 3;
    const size_t rb0 = size_t(yuvx_plane_row_bytes(g.layout, 0, g.w, bs)), rb1 = size_t(yuvx_plane_row_bytes(g.layout, 1, g.w, bs));
    const uint8_t* const p0 = planes + g.src_off;
    const uint8_t* const p1 = p0 + size_t(yuvx_plane_rows(g.layout, 0, g.h)) * rb0;
    const uint8_t* const p2 = p1 + size_t(yuvx_plane_rows(g.layout, 1, g.h)) * rb1;
    yuvx_dispatch(p0, p1, p2, rb0, rb1, rb1, bgr + g.dst_off, g, (b - g.block0) * THREADS + int(threadIdx.x));
}

// planes where a decoder (or a tensor) left them in device memory, each with its own pitch
__global__ __launch_bounds__(THREADS) void whenet_yuvx_planes_to_bgr_kernel(uint8_t* __restrict__ bgr, YuvxClip clip) {
    const int b = int(blockIdx.x);
    const YuvxFrame& g = clip.f[frame_of_block(clip, b)];
    yuvx_dispatch(g.plane[0], g.plane[1], g.plane[2], size_t(g.pitch[0]), size_t(g.pitch[1]), size_t(g.pitch[2]), bgr + g.dst_off, g,
                  (b - g.block0) * THREADS + int(threadIdx.x));
}

int yuvx_blocks(int h, int w) { return (((w + 3) >> 2) * ((h + 1) >> 1) + THREADS - 1) / THREADS; }

// what a launcher holds a record to: the geometry the kernel's loads and stores are bounded by (`planes`: the plane form, whose
// pointers, pitches and alignments the kernel uses as they are)
bool good_record(const YuvxFrame& g, bool planes) {
    bool good = g.h >= 1 && g.w >= 1 && g.h <= YUVX_MAX_FRAME_SIDE && g.w <= YUVX_MAX_FRAME_SIDE && yuvx_layout_known(g.layout) &&
                (g.container == WHENET_YUVX_U8 || g.container == WHENET_YUVX_U16) && g.shift >= 0 && g.shift <= WHENET_YUVX_MAX_SHIFT &&
                !(yuvx_layout_packed(g.layout) && g.container != WHENET_YUVX_U8);
    const bool wide = g.container == WHENET_YUVX_U16;
    if (good && !planes) good = !(wide && (g.src_off & 1));
    for (int p = 0; good && planes && p < yuvx_plane_count(g.layout); ++p)
        good = g.plane[p] != nullptr && g.pitch[p] >= yuvx_plane_row_bytes(g.layout, p, g.w, g.container >> 3) &&
               !(wide && ((reinterpret_cast<uintptr_t>(g.plane[p]) | uintptr_t(g.pitch[p])) & 1));
    return good;
}

int set_blocks(YuvxClip& clip, bool planes, const char* what) {
    WHENET_REQUIRE(clip.frames >= 1 && clip.frames <= MIXED_MAX_FRAMES, WHENET_EINVAL, std::string(what) + ": 1..16 frames");
    int blocks = 0;
    for (int f = 0; f < clip.frames; ++f) {
        WHENET_REQUIRE(good_record(clip.f[f], planes), WHENET_EINVAL, std::string(what) + ": bad frame geometry");
        clip.f[f].block0 = blocks;
        blocks += yuvx_blocks(clip.f[f].h, clip.f[f].w);
    }
    clip.total_blocks = blocks;
    return blocks;
}

}  // namespace

const YuvxCoeffs& yuvx_coeffs(int matrix) {
    const YuvxCoeffs* k = yuvx_coeffs_or_null(matrix);
    WHENET_REQUIRE(k != nullptr, WHENET_EINVAL, "unknown YUV matrix " + std::to_string(matrix));
    return *k;
}

void check_yuvx_frames(const char* what, const whenet_yuvx_frame_t* frames, int nframes) {
    const std::string bad = yuvx_check_frames(what, frames, nframes);
    WHENET_REQUIRE(bad.empty(), WHENET_EINVAL, bad);
}

YuvxFrame yuvx_frame(const whenet_yuvx_frame_t& f, size_t src_off, size_t dst_off) {
    YuvxFrame g{};
    for (int p = 0; p < yuvx_plane_count(f.layout); ++p) g.plane[p] = f.plane[p], g.pitch[p] = f.pitch[p];
    g.h = f.h, g.w = f.w, g.layout = f.layout, g.container = f.container, g.shift = f.shift;
    g.k = yuvx_coeffs(f.matrix);
    g.src_off = src_off, g.dst_off = dst_off;
    return g;
}

void launch_yuvx_to_bgr(const uint8_t* d_planes, uint8_t* d_bgr, YuvxClip clip, hipStream_t stream) {
    const int blocks = set_blocks(clip, false, "yuvx_to_bgr");
    WHENET_REQUIRE((reinterpret_cast<uintptr_t>(d_planes) & 7) == 0, WHENET_EINVAL, "yuvx_to_bgr: the plane buffer is not 8-byte aligned");
    hipLaunchKernelGGL(whenet_yuvx_to_bgr_kernel, dim3(blocks), dim3(THREADS), 0, stream, d_planes, d_bgr, clip);
    WHENET_HIP_CHECK(hipGetLastError());
}

// The callers have checked the planes (Engine::check_device_plane): the kernel reads rows x row bytes of each at its pitch and
// nothing else.
void launch_yuvx_planes_to_bgr(uint8_t* d_bgr, YuvxClip clip, hipStream_t stream) {
    const int blocks = set_blocks(clip, true, "yuvx_planes_to_bgr");
    hipLaunchKernelGGL(whenet_yuvx_planes_to_bgr_kernel, dim3(blocks), dim3(THREADS), 0, stream, d_bgr, clip);
    WHENET_HIP_CHECK(hipGetLastError());
}

}  // namespace whenet
