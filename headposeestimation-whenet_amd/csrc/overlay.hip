// The pose overlay on the device: the annotated frame of demo_video.py:26-29, :60 (`cv2.rectangle` of every head's window, utils.py's
// `draw_axis` from its centre, the frame written out) from what the forward leaves in device memory -- the slot's frame, the
// windows, the angles -- into a packed BGR / RGB, NV12 or I420 destination.  The arithmetic is the integer statement of
// include/whenet_hip.h, shared with the host statement through overlay_host.h: the bytes are those of whenet_annotate_host.
//
// whenet_overlay_plan_kernel: one lane per head.  Window + float32 angles -> the 16 endpoint ints and the flags word (utils.py:15-42
// in double, every operation rounded on its own: contraction is off for this file as it is for headplan.hip's arithmetic).  With a
// label table it also writes the head's three lines of text as glyph indices (rintf and integer digits, float32 only) and sets
// OVERLAY_LABELS.
//
// whenet_overlay_draw_kernel: one pass, source frame in, destination out.  A workgroup of 256 lanes owns a tile of 128 x 16 pixels.
//   1. Lane t takes head t: its (up to) seven segments are tested against the tile's bounding box grown by the raster's reach of 1.
//      The survivors of all heads are numbered in paint order (an exclusive scan of the per-head counts through LDS) and written to
//      an LDS list: P and Q packed as two 16-bit coordinates each, and the colour index.  At most 256 x 7 entries of 9 bytes: 17 KB of LDS with the counts.
//   2. A lane owns 4 horizontally adjacent pixels on 2 rows, as in yuv.hip: it loads their 24 source bytes, walks the list once and
//      lets every hit overwrite the pixel's colour -- the last primitive in paint order wins -- with a bounding-box test of the
//      lane's 4 x 2 block in front of the eight exact tests.
//   3. Stores follow yuv.hip / ingest.hip: dwords only where the destination address is a multiple of 4 and the bytes belong to the
//      row, head / tail bytes and a row's last 1..3 pixels byte by byte.  4:2:0: the lane's block is exactly two chroma samples of one
//      chroma row (their 2 x 2 sums clamp at the frame's last row / column, which lie inside the block), one dword of an NV12 row.
//      No lane writes a byte outside its pixels: pitch padding and the neighbouring surface belong to the caller.
// Adjacent lanes own adjacent groups: a wave reads and writes 384 contiguous bytes on each of 4 rows.  The pixel arrays are indexed
// by unrolled constants only (no scratch).
//
// The draw kernel has two instantiations.  WHENET_DISPLAY_SIMPLE is the kernel above.  WHENET_DISPLAY_FULL puts, behind a head's
// seven segments, one list entry per line of text whose box meets the tile -- the origin as P, head * 3 + line and the line's length
// as Q, LINE_TAG as the colour -- so the list holds at most 256 x 10 entries (24 KB of LDS with the counts) however much text there
// is.  For such an entry a lane tests the line's box against its 4 x 2 block, loads the line's 16 bytes from the label table and asks
// overlay_text_hit for each of its pixels: the character cell is (x - ox) / 7, the glyph's row a byte of the 400-byte constant table
// that overlay_host.h builds from the header's strokes by the thin rule.
#include <algorithm>
#include <string>

#include "kernels.h"
#include "overlay_host.h"

namespace whenet {

namespace {

constexpr int THREADS = 256;
constexpr int TILE_W = 128, TILE_H = 16;      // 32 lanes x 4 pixels, 8 lane rows x 2 rows
constexpr int LINE_TAG = 4;                   // the colour byte of a list entry that is a line of text

__device__ __forceinline__ OverlayLine load_line(const uint32_t* labels, int index) {
    const uint4 w = *reinterpret_cast<const uint4*>(labels + size_t(index) * 4);
    return {uint64_t(w.x) | (uint64_t(w.y) << 32), uint64_t(w.z) | (uint64_t(w.w) << 32)};
}

__global__ __launch_bounds__(THREADS) void whenet_overlay_plan_kernel(OverlayPlanArgs a) {
    const int i = int(blockIdx.x) * THREADS + int(threadIdx.x);
    if (i >= a.k) return;
    const int32_t* r = a.rects + size_t(i) * a.rect_stride;
    int32_t rect[4] = {r[0], r[1], r[2], r[3]};
    if (a.rect_is_size) rect[2] += rect[0], rect[3] += rect[1];      // a crop plan's {y0, x0, h, w}
    int valid = a.valid ? a.valid[i] : 1;
    int row = i;
    if (a.row) {
        row = a.row[i];
        if (row < 0) valid = 0, row = 0;
    }
    const float* y = a.ypr + size_t(row) * 3;
    int32_t seg[OVERLAY_SEG_INTS];
    int flags = overlay_segments(rect, valid, double(y[0]), double(y[1]), double(y[2]), seg);
    if (a.labels != nullptr) {
        OverlayLine lines[3];
        int32_t origin[3][2];
        flags |= overlay_labels(seg, flags, y[0], y[1], y[2], lines, origin);
        uint4* rec = reinterpret_cast<uint4*>(a.labels + size_t(i) * OVERLAY_LABEL_WORDS);
#pragma unroll
        for (int l = 0; l < 3; ++l)
            rec[l] = make_uint4(uint32_t(lines[l].lo), uint32_t(lines[l].lo >> 32), uint32_t(lines[l].hi), uint32_t(lines[l].hi >> 32));
    }
    int32_t* out = a.segs + size_t(i) * OVERLAY_SEG_INTS;
#pragma unroll
    for (int j = 0; j < OVERLAY_SEG_INTS; ++j) out[j] = seg[j];
    a.flags[i] = flags;
}

__device__ __forceinline__ uint32_t pack_xy(int x, int y) { return (uint32_t(x) & 0xFFFFu) | (uint32_t(y) << 16); }
__device__ __forceinline__ int unpack_x(uint32_t p) { return int(int16_t(p & 0xFFFFu)); }
__device__ __forceinline__ int unpack_y(uint32_t p) { return int(p) >> 16; }

__device__ __forceinline__ uint32_t funnel(uint32_t lo, uint32_t hi, int shift_bits) {      // bits [shift, shift + 32) of hi:lo
    return uint32_t(((uint64_t(hi) << 32) | lo) >> shift_bits);
}

// 12 bytes (n == 4) or 3 n bytes at dp, which is aligned to nothing in general (yuv.hip's output stage)
__device__ __forceinline__ void store_pixels(uint8_t* dp, int n, uint32_t w0, uint32_t w1, uint32_t w2) {
    if (n == 4) {
        const int a = int(reinterpret_cast<uintptr_t>(dp) & 3);
        if (a == 0) {
            uint32_t* d = reinterpret_cast<uint32_t*>(dp);
            d[0] = w0, d[1] = w1, d[2] = w2;
        } else {
            const int head = 4 - a;
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (j < head) dp[j] = uint8_t(w0 >> (8 * j));
            uint32_t* d = reinterpret_cast<uint32_t*>(dp + head);
            d[0] = funnel(w0, w1, 8 * head), d[1] = funnel(w1, w2, 8 * head);
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (j < a) dp[12 - a + j] = uint8_t(w2 >> (8 * (head + j)));
        }
    } else {
        const int nb = 3 * n;                   // 3, 6 or 9 bytes
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const uint32_t word = j < 4 ? w0 : (j < 8 ? w1 : w2);
            if (j < nb) dp[j] = uint8_t(word >> (8 * (j & 3)));
        }
    }
}

template <int DISPLAY>
__global__ __launch_bounds__(THREADS) void whenet_overlay_draw_kernel(OverlayDrawArgs a) {
    constexpr bool FULL = DISPLAY == WHENET_DISPLAY_FULL;
    constexpr int MAX_SEGS = OVERLAY_MAX_HEADS * (FULL ? 10 : 7);
    __shared__ uint32_t s_p[MAX_SEGS], s_q[MAX_SEGS];
    __shared__ uint8_t s_c[MAX_SEGS];
    __shared__ int s_cnt[THREADS];
    const int tid = int(threadIdx.x);
    const int tile_x0 = int(blockIdx.x) * TILE_W, tile_y0 = int(blockIdx.y) * TILE_H;

    // 1. the tile's primitives, in paint order
    {
        const int bx0 = tile_x0 - 1, bx1 = min(tile_x0 + TILE_W, a.fw) - 1 + 1;       // the tile's box grown by the reach of 1
        const int by0 = tile_y0 - 1, by1 = min(tile_y0 + TILE_H, a.fh) - 1 + 1;
        int32_t seg[OVERLAY_SEG_INTS];
        int nseg = 0;
        unsigned mask = 0;
        [[maybe_unused]] int len[3] = {0, 0, 0};
        if (tid < a.k) {
            const int f = a.flags[tid];
            nseg = (f & OVERLAY_RECT) ? ((f & OVERLAY_AXES) ? 7 : 4) : 0;
            if (nseg > 0) {
                const int32_t* g = a.segs + size_t(tid) * OVERLAY_SEG_INTS;
#pragma unroll
                for (int j = 0; j < OVERLAY_SEG_INTS; ++j) seg[j] = g[j];
#pragma unroll
                for (int s = 0; s < 7; ++s) {
                    int px, py, qx, qy, colour;
                    overlay_head_segment(seg, s, px, py, qx, qy, colour);
                    const bool in = s < nseg && min(px, qx) <= bx1 && max(px, qx) >= bx0 && min(py, qy) <= by1 && max(py, qy) >= by0;
                    mask |= in ? (1u << s) : 0u;
                }
                if constexpr (FULL) {
                    if (f & OVERLAY_LABELS) {
#pragma unroll
                        for (int l = 0; l < 3; ++l) {      // the box of a line: its characters' boxes, nothing around them
                            len[l] = int(a.labels[(size_t(tid) * 3 + l) * 4 + 3] >> 24);
                            const int ox = seg[0], oy = seg[1] - OVERLAY_LINE_STEP * l;
                            const bool in = ox <= bx1 - 1 && ox + OVERLAY_ADVANCE * len[l] - 2 >= bx0 + 1 && oy + OVERLAY_GLYPH_TOP <= by1 - 1 &&
                                            oy + OVERLAY_GLYPH_TOP + OVERLAY_GLYPH_ROWS - 1 >= by0 + 1;
                            mask |= in ? (1u << (7 + l)) : 0u;
                        }
                    }
                }
            }
        }
        s_cnt[tid] = __popc(mask);
        __syncthreads();
        int base = 0;
        for (int j = 0; j < a.k; ++j) {             // (uniform trip count, broadcast reads)
            const int n = s_cnt[j];
            base += j < tid ? n : 0;
        }
        if (mask != 0) {
#pragma unroll
            for (int s = 0; s < 7; ++s) {
                int px, py, qx, qy, colour;
                overlay_head_segment(seg, s, px, py, qx, qy, colour);
                if (mask & (1u << s)) {
                    s_p[base] = pack_xy(px, py), s_q[base] = pack_xy(qx, qy), s_c[base] = uint8_t(colour);
                    ++base;
                }
            }
            if constexpr (FULL) {
#pragma unroll
                for (int l = 0; l < 3; ++l)
                    if (mask & (1u << (7 + l))) {
                        s_p[base] = pack_xy(seg[0], seg[1] - OVERLAY_LINE_STEP * l);
                        s_q[base] = uint32_t(tid * 3 + l) | (uint32_t(len[l]) << 16), s_c[base] = uint8_t(LINE_TAG);
                        ++base;
                    }
            }
        }
        __syncthreads();
    }
    int total = 0;
    for (int j = 0; j < a.k; ++j) total += s_cnt[j];

    // 2. the lane's 4 x 2 pixels
    const int x0 = tile_x0 + (tid & 31) * 4, y0 = tile_y0 + (tid >> 5) * 2;
    if (x0 >= a.fw || y0 >= a.fh) return;
    const int n = min(4, a.fw - x0), rows = min(2, a.fh - y0);
    uint32_t pix[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        uint32_t w0 = 0, w1 = 0, w2 = 0;
        if (r < rows) {
            const uint8_t* sp = a.frame + (size_t(y0 + r) * a.fw + x0) * 3;
            if (n == 4 && (reinterpret_cast<uintptr_t>(sp) & 3) == 0) {
                const uint32_t* s4 = reinterpret_cast<const uint32_t*>(sp);
                w0 = s4[0], w1 = s4[1], w2 = s4[2];
            } else {
                const int nb = 3 * n;
#pragma unroll
                for (int j = 0; j < 12; ++j) {
                    const uint32_t b = j < nb ? uint32_t(sp[j]) << (8 * (j & 3)) : 0u;
                    if (j < 4) w0 |= b;
                    else if (j < 8) w1 |= b;
                    else w2 |= b;
                }
            }
        }
        pix[r][0] = w0 & 0xFFFFFFu;
        pix[r][1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
        pix[r][2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
        pix[r][3] = w2 >> 8;
    }
    for (int s = 0; s < total; ++s) {
        const uint32_t p = s_p[s], q = s_q[s];
        if constexpr (FULL) {
            if (s_c[s] == LINE_TAG) {
                const int ox = unpack_x(p), oy = unpack_y(p), n_chars = int(q >> 16);
                if (ox > x0 + 3 || ox + OVERLAY_ADVANCE * n_chars - 2 < x0 || oy + OVERLAY_GLYPH_TOP > y0 + 1 ||
                    oy + OVERLAY_GLYPH_TOP + OVERLAY_GLYPH_ROWS - 1 < y0)
                    continue;
                const OverlayLine t = load_line(a.labels, int(q & 0xFFFFu));
                const uint32_t c = overlay_label_colour(a.channel_order);
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (overlay_text_hit(t, ox, oy, x0 + j, y0 + r)) pix[r][j] = c;
                continue;
            }
        }
        const int px = unpack_x(p), py = unpack_y(p), qx = unpack_x(q), qy = unpack_y(q);
        if (min(px, qx) > x0 + 4 || max(px, qx) < x0 - 1 || min(py, qy) > y0 + 2 || max(py, qy) < y0 - 1) continue;
        const uint32_t c = overlay_colour(int(s_c[s]), a.channel_order);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (overlay_hit(px, py, qx, qy, x0 + j, y0 + r)) pix[r][j] = c;
    }
    // pixels beyond the frame's last column / row repeat the last one: the 2 x 2 chroma sums clamp there
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int j = 1; j < 4; ++j)
            if (j >= n) pix[r][j] = pix[r][j - 1];
    if (rows < 2) {
#pragma unroll
        for (int j = 0; j < 4; ++j) pix[1][j] = pix[0][j];
    }

    // 3. the destination
    if (a.format == WHENET_SURF_PACKED) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r >= rows) break;
            const uint32_t w0 = pix[r][0] | (pix[r][1] << 24), w1 = (pix[r][1] >> 8) | (pix[r][2] << 16), w2 = (pix[r][2] >> 16) | (pix[r][3] << 8);
            store_pixels(a.plane[0] + size_t(y0 + r) * size_t(a.pitch[0]) + size_t(x0) * 3, n, w0, w1, w2);
        }
        return;
    }
    const int rsh = a.channel_order == WHENET_BGR ? 16 : 0, bsh = 16 - rsh;
    int rs[2] = {0, 0}, gs[2] = {0, 0}, bs[2] = {0, 0};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        uint32_t y4 = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int R = int((pix[r][j] >> rsh) & 255u), G = int((pix[r][j] >> 8) & 255u), B = int((pix[r][j] >> bsh) & 255u);
            y4 |= uint32_t(overlay_luma(a.kc, R, G, B)) << (8 * j);
            rs[j >> 1] += R, gs[j >> 1] += G, bs[j >> 1] += B;
        }
        if (r < rows) {
            uint8_t* yp = a.plane[0] + size_t(y0 + r) * size_t(a.pitch[0]) + x0;
            if (n == 4 && (reinterpret_cast<uintptr_t>(yp) & 3) == 0) {
                *reinterpret_cast<uint32_t*>(yp) = y4;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < n) yp[j] = uint8_t(y4 >> (8 * j));
            }
        }
    }
    const int cy = y0 >> 1, cx = x0 >> 1;
    const bool two = n > 2;                         // the block has a second chroma sample
    const uint32_t u0 = uint32_t(overlay_cb(a.kc, rs[0], gs[0], bs[0])), v0 = uint32_t(overlay_cr(a.kc, rs[0], gs[0], bs[0]));
    const uint32_t u1 = uint32_t(overlay_cb(a.kc, rs[1], gs[1], bs[1])), v1 = uint32_t(overlay_cr(a.kc, rs[1], gs[1], bs[1]));
    if (a.format == WHENET_YUV_NV12) {
        uint8_t* c = a.plane[1] + size_t(cy) * size_t(a.pitch[1]) + 2 * cx;
        if (two && (reinterpret_cast<uintptr_t>(c) & 3) == 0) {
            *reinterpret_cast<uint32_t*>(c) = u0 | (v0 << 8) | (u1 << 16) | (v1 << 24);
        } else {
            c[0] = uint8_t(u0), c[1] = uint8_t(v0);
            if (two) c[2] = uint8_t(u1), c[3] = uint8_t(v1);
        }
    } else {
        uint8_t* cu = a.plane[1] + size_t(cy) * size_t(a.pitch[1]) + cx;
        uint8_t* cv = a.plane[2] + size_t(cy) * size_t(a.pitch[2]) + cx;
        if (two && (reinterpret_cast<uintptr_t>(cu) & 1) == 0) {
            *reinterpret_cast<uint16_t*>(cu) = uint16_t(u0 | (u1 << 8));
        } else {
            cu[0] = uint8_t(u0);
            if (two) cu[1] = uint8_t(u1);
        }
        if (two && (reinterpret_cast<uintptr_t>(cv) & 1) == 0) {
            *reinterpret_cast<uint16_t*>(cv) = uint16_t(v0 | (v1 << 8));
        } else {
            cv[0] = uint8_t(v0);
            if (two) cv[1] = uint8_t(v1);
        }
    }
}

}  // namespace

void launch_overlay_plan(const OverlayPlanArgs& a, hipStream_t stream) {
    WHENET_REQUIRE(a.k >= 1 && a.k <= 1024 && a.rects != nullptr && a.ypr != nullptr && a.segs != nullptr && a.flags != nullptr &&
                       a.rect_stride >= 4,
                   WHENET_EINVAL, "overlay_plan: bad arguments");
    hipLaunchKernelGGL(whenet_overlay_plan_kernel, dim3((a.k + THREADS - 1) / THREADS), dim3(THREADS), 0, stream, a);
    WHENET_HIP_CHECK(hipGetLastError());
}

// The callers have checked the surface (overlay_check; device planes: Engine::check_device_plane): the kernel writes rows x row
// bytes of each plane at its pitch and nothing else.
void launch_overlay_draw(const OverlayDrawArgs& a, hipStream_t stream) {
    int rows[3], row_bytes[3];
    const int planes = overlay_surface_planes(a.format, a.fh, a.fw, rows, row_bytes);
    WHENET_REQUIRE(a.frame != nullptr && a.fh >= 1 && a.fw >= 1 && a.fh <= OVERLAY_MAX_FRAME_SIDE && a.fw <= OVERLAY_MAX_FRAME_SIDE &&
                       planes > 0 && a.k >= 0 && a.k <= OVERLAY_MAX_HEADS && (a.k == 0 || (a.segs != nullptr && a.flags != nullptr)) &&
                       (a.channel_order == WHENET_RGB || a.channel_order == WHENET_BGR),
                   WHENET_EINVAL, "overlay_draw: bad arguments");
    for (int p = 0; p < planes; ++p)
        WHENET_REQUIRE(a.plane[p] != nullptr && a.pitch[p] >= row_bytes[p], WHENET_EINVAL, "overlay_draw: bad surface");
    const dim3 grid((a.fw + TILE_W - 1) / TILE_W, (a.fh + TILE_H - 1) / TILE_H);
    if (a.display == WHENET_DISPLAY_FULL) {
        WHENET_REQUIRE(a.k == 0 || a.labels != nullptr, WHENET_EINVAL, "overlay_draw: display full without a label table");
        hipLaunchKernelGGL(whenet_overlay_draw_kernel<WHENET_DISPLAY_FULL>, grid, dim3(THREADS), 0, stream, a);
    } else {
        WHENET_REQUIRE(a.display == WHENET_DISPLAY_SIMPLE, WHENET_EINVAL, "overlay_draw: unknown display " + std::to_string(a.display));
        hipLaunchKernelGGL(whenet_overlay_draw_kernel<WHENET_DISPLAY_SIMPLE>, grid, dim3(THREADS), 0, stream, a);
    }
    WHENET_HIP_CHECK(hipGetLastError());
}

}  // namespace whenet
