// The baseline JPEG decoder on the device: the entropy data of one stream in, the frame out.  The format and every formula are in
// include/whenet_hip.h (JPEG DECODER); the arithmetic -- bit reader, Huffman decode of a block, inverse DCT pass, the pixel rule --
// is jpeg_dec_host.h's, the same functions the host statement runs.  Integers only.
//
// Reference: demo.py (`cv2.imread`) and demo_video.py:49-53 (`cap.read()` of a camera or an MJPG file).
//
// Restart intervals are what makes a baseline stream parallel: the DC predictors start at 0 in each and its bits start at a byte of
// their own.  The interval count comes from the header, so every launch size is known on the host and nothing waits.
//   whenet_jpeg_dec_scan_kernel     one workgroup.  A lane owns 16 bytes of the entropy data per step and finds its 0xFF 0xD0..0xD7
//                                   pairs (the byte behind its run included: a pair may straddle two runs); the counts are scanned in
//                                   order (wave shuffles + LDS totals, a carry from step to step) and marker k writes the start of
//                                   interval k + 1.  The numbers (k mod 8) and the count are checked: meta = the first bad interval.
//   whenet_jpeg_dec_entropy_kernel  one restart interval per lane, 16 intervals per workgroup (a wave's lanes diverge in the Huffman
//                                   walk: few lanes per wave, many waves).  The decode tables lie in LDS.  Dequantised, clamped int16
//                                   coefficients go into records [block][64] that a memset zeroed.  A stream without DRI is ONE lane.
//   whenet_jpeg_dec_idct_kernel     8 lanes per block: lane u runs the column pass of column u, the rounded values go through LDS,
//                                   lane y runs the row pass of row y and stores its 8 samples as one 8-byte store.  The component
//                                   planes are padded to whole MCUs, so every block lies inside its plane.  Writes the status words.
//   whenet_jpeg_dec_frame_kernel    planes -> packed pixels, 4 pixels of a row per lane: one luma dword, the chroma samples of
//                                   (x >> log2 hs, y >> log2 vs) (hs = 4: one byte for the group), 12 bytes out with the head / funnel-shift / tail stores of yuv.hip.
//                                   A tight BGR destination of a 4:2:0 stream goes through yuv.hip's own plane kernel instead.
//   whenet_jpeg_dec_yuv_kernel      4:2:0 planes -> an I420 or NV12 surface (a copy).
//   whenet_jpeg_dec_frame_oriented_kernel   in the frame kernel's place where the record's EXIF orientation is 2..8 (the header's JPEG
//                                   DECODER, ORIENTATION): the same pixel values at the oriented frame's addresses -- 2..4 a reversed
//                                   group in a mirrored row, 5..8 a 32 x 32 tile of the destination gathered in LDS.  No upright frame
//                                   is written anywhere.  27 VGPRs, 66 SGPRs, 4,224 B LDS, no scratch (rule 1's form: 44 / 76).
// RULE 1 (libjpeg's bytes; the header's JPEG DECODER, RULE 1) has its own forms of two of them, the rule fixed at compile time:
//   whenet_jpeg_dec_idct_libjpeg_kernel   the same mapping, jidctint's two passes (the row pass in int64), the same status words.
//   whenet_jpeg_dec_frame_libjpeg_kernel  the same 4 pixels per lane and the same stores; chroma by fancy upsampling from the lane's two
//                                   columns, the two neighbour columns and one vertical neighbour row, every index clamped to the
//                                   real plane, then jdcolor's row.  Every packed frame of rule 1 takes it, the tight 4:2:0 BGR one too.
#include <algorithm>
#include <string>

#include "kernels.h"
#include "jpeg_dec_host.h"

namespace whenet {

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int SCAN_BYTES = 16;                  // bytes per lane and step of the scan kernel
constexpr int ENT_THREADS = 64;                 // the entropy kernel's workgroup: all lanes load the tables,
constexpr int ENT_LANES = 16;                   // ... the first 16 decode an interval each
constexpr int IDCT_BLOCKS = THREADS / 8;        // blocks per workgroup of the idct kernel

static_assert(sizeof(JpegDecTables) % 4 == 0, "the tables are copied to LDS by dwords");

// exclusive scan of one int per lane over the workgroup (every lane calls it); total = the sum
__device__ inline int block_exclusive_scan(int v, int* s_wave, int& total) {
    const int lane = int(threadIdx.x) & 63, wave = int(threadIdx.x) >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const int t = s_wave[w];
        base += w < wave ? t : 0;
        total += t;
    }
    __syncthreads();
    return base + inc - v;
}

// ---- the bodies: what a workgroup does for ONE stream, given that stream's record and the workgroup's index within the stream's
// share of the grid (bx).  The single-stream kernels call them with their own argument and blockIdx.x, the clip kernels with the
// record of the frame the workgroup belongs to.
__device__ __forceinline__ void scan_body(const JpegDecArgs& a) {
    __shared__ int s_wave[WAVES];
    __shared__ int s_bad;
    const int tid = int(threadIdx.x), N = a.g.intervals;
    if (tid == 0) s_bad = JPEG_DEC_NO_BAD;
    __syncthreads();
    const long long nbytes = a.nbytes;
    int carry = 0;
    for (long long base = 0; base < nbytes; base += THREADS * SCAN_BYTES) {
        const long long first = base + tid * SCAN_BYTES;
        const uint8_t* p = a.data + first;
        uint32_t w[SCAN_BYTES / 4 + 1] = {0u, 0u, 0u, 0u, 0u};      // the run's 16 bytes and the byte behind it; 0 beyond the data
        if (first + SCAN_BYTES <= nbytes && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            const uint4 q = *reinterpret_cast<const uint4*>(p);
            w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < SCAN_BYTES; ++j)
                if (first + j < nbytes) w[j >> 2] |= uint32_t(p[j]) << (8 * (j & 3));
        }
        if (first + SCAN_BYTES < nbytes) w[4] = p[SCAN_BYTES];
        unsigned marks = 0;
#pragma unroll
        for (int j = 0; j < SCAN_BYTES; ++j) {
            const uint32_t cur = (w[j >> 2] >> (8 * (j & 3))) & 255u, nx = (w[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 255u;
            if (cur == 0xFFu && (nx & 0xF8u) == 0xD0u) marks |= 1u << j;
        }
        int total;
        int k = carry + block_exclusive_scan(__popc(marks), s_wave, total);
#pragma unroll
        for (int j = 0; j < SCAN_BYTES; ++j) {
            if (marks & (1u << j)) {
                const int m = int((w[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 7u);
                if (k >= N - 1) atomicMin(&s_bad, N - 1);
                else if (m != (k & 7)) atomicMin(&s_bad, k);
                if (k + 1 < N) a.start[k + 1] = int(first + j + 2);
                ++k;
            }
        }
        carry += total;
    }
    __syncthreads();
    if (tid == 0) {
        int bad = s_bad;
        if (carry < N - 1 && carry < bad) bad = carry;
        a.start[0] = 0;
        a.meta[0] = bad, a.meta[1] = bad;      // what the markers say; lowered by the entropy decode
    }
}

__device__ __forceinline__ void entropy_body(const JpegDecArgs& a, int bx) {
    __shared__ JpegDecTables s_t;
    __shared__ __attribute__((aligned(16))) int16_t s_block[ENT_LANES][64 + 8];      // a lane's block in hand (144-byte rows)
    const int tid = int(threadIdx.x);
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.tables);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&s_t);
        for (int i = tid; i < int(sizeof(JpegDecTables) / 4); i += ENT_THREADS) dst[i] = src[i];
    }
    __syncthreads();
    const long long i = (long long)(bx) * ENT_LANES + tid;
    if (tid >= ENT_LANES || i >= a.g.intervals || i > a.meta[0]) return;
    if (!jpeg_dec_interval(a.data, a.nbytes, a.start[i], s_t, a.g, int(i), a.coef, 0, s_block[tid])) atomicMin(&a.meta[1], int(i));
}

// RULE: the decode rule, fixed at compile time (0: the project's own passes, 1: jidctint's, whose row pass is 64-bit)
template <int RULE>
__device__ __forceinline__ void idct_body(const JpegDecArgs& a, int bx) {
    __shared__ int s_r[IDCT_BLOCKS][8][9];
    const int tid = int(threadIdx.x), lb = tid >> 3, l = tid & 7;
    const long long g = (long long)(bx) * IDCT_BLOCKS + lb;
    const long long total = (long long)(a.g.mcu_cols) * a.g.mcu_rows * a.g.bpm;
    const bool live = g < total;
    if (live) {
        const int16_t* c = a.coef + size_t(g) * 64;
        int col[8], o[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) col[v] = c[v * 8 + l];
        if constexpr (RULE == JPEG_RULE_LIBJPEG) jpeg_idct8_islow<int>(col, o);
        else jpeg_idct8(col, o);
#pragma unroll
        for (int y = 0; y < 8; ++y) s_r[lb][y][l] = RULE == JPEG_RULE_LIBJPEG ? jpeg_islow_round1(o[y]) : jpeg_idct_round(o[y]);
    }
    __syncthreads();
    if (bx == 0 && tid == 0) {      // (the entropy kernel has ended: a kernel boundary lies between)
        const int bad = a.meta[1];
        a.status[0] = bad == JPEG_DEC_NO_BAD ? WHENET_OK : WHENET_EFORMAT;
        a.status[1] = bad == JPEG_DEC_NO_BAD ? -1 : bad;
    }
    if (!live) return;
    uint32_t lo = 0, hi = 0;
    if constexpr (RULE == JPEG_RULE_LIBJPEG) {
        long long row[8], b[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) row[u] = s_r[lb][l][u];
        jpeg_idct8_islow<long long>(row, b);
#pragma unroll
        for (int x = 0; x < 4; ++x) lo |= uint32_t(jpeg_islow_sample(b[x])) << (8 * x), hi |= uint32_t(jpeg_islow_sample(b[x + 4])) << (8 * x);
    } else {
        int row[8], b[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) row[u] = s_r[lb][l][u];
        jpeg_idct8(row, b);
#pragma unroll
        for (int x = 0; x < 4; ++x) lo |= uint32_t(jpeg_idct_sample(b[x])) << (8 * x), hi |= uint32_t(jpeg_idct_sample(b[x + 4])) << (8 * x);
    }
    const long long m = g / a.g.bpm;
    int comp, y0, x0;
    jpeg_dec_block_origin(a.g, m, int(g - m * a.g.bpm), comp, y0, x0);
    // the planes are padded to whole MCUs and 8-byte aligned: the block's row lies inside its plane
    *reinterpret_cast<uint2*>(a.plane[comp] + size_t(y0 + l) * size_t(a.g.plane_pitch[comp]) + size_t(x0)) = make_uint2(lo, hi);
}

__device__ __forceinline__ uint32_t funnel(uint32_t lo, uint32_t hi, int shift_bits) {      // bits [shift, shift + 32) of hi:lo
    return uint32_t(((uint64_t(hi) << 32) | lo) >> shift_bits);
}

// the 1..4 packed pixels px of a lane's group to dp: 12 bytes as dwords where the group is whole (a head and a tail of bytes where dp
// is not aligned), else the 3, 6 or 9 bytes the row still has -- never a byte behind the row
__device__ __forceinline__ void store_group(uint8_t* dp, const uint32_t px[4], int n) {
    const uint32_t w0 = px[0] | (px[1] << 24), w1 = (px[1] >> 8) | (px[2] << 16), w2 = (px[2] >> 16) | (px[3] << 8);
    if (n == 4) {
        const int al = int(reinterpret_cast<uintptr_t>(dp) & 3);
        if (al == 0) {
            uint32_t* d = reinterpret_cast<uint32_t*>(dp);
            d[0] = w0, d[1] = w1, d[2] = w2;
        } else {
            const int head = 4 - al;
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (j < head) dp[j] = uint8_t(w0 >> (8 * j));
            uint32_t* d = reinterpret_cast<uint32_t*>(dp + head);
            d[0] = funnel(w0, w1, 8 * head), d[1] = funnel(w1, w2, 8 * head);
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (j < al) dp[12 - al + j] = uint8_t(w2 >> (8 * (head + j)));
        }
    } else {
        const int nb = 3 * n;                       // 3, 6 or 9 bytes: the row ends here, the bytes behind it are not the frame's
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const uint32_t word = j < 4 ? w0 : (j < 8 ? w1 : w2);
            if (j < nb) dp[j] = uint8_t(word >> (8 * (j & 3)));
        }
    }
}

// The packed pixels px of the 4-pixel group at (y, x) of the UPRIGHT frame, x a multiple of 4 below w, y < h, by the stream's rule:
// what the upright frame kernels store at (y, x) and the oriented ones at the place the orientation gives each pixel.  (The pixels
// of a group behind the row's end are computed from the planes' padding and never stored.)
template <int RULE>
__device__ __forceinline__ void frame_group(const JpegDecArgs& a, int y, int x, uint32_t px[4]);

template <>
__device__ __forceinline__ void frame_group<JPEG_RULE_OWN>(const JpegDecArgs& a, int y, int x, uint32_t px[4]) {
    // (x is a multiple of 4 and the planes' pitches are multiples of 8: the loads are aligned and inside the padded planes)
    const uint32_t y4 = *reinterpret_cast<const uint32_t*>(a.plane[0] + size_t(y) * size_t(a.g.plane_pitch[0]) + size_t(x));
    const int hsh = jpeg_dec_shift(a.g.hs), vsh = jpeg_dec_shift(a.g.vs);
    uint32_t u4 = 0, v4 = 0;
    if (a.g.comps == 3) {
        const size_t ci = size_t(y >> vsh) * size_t(a.g.plane_pitch[1]) + size_t(x >> hsh);
        if (hsh == 2) {      // hs = 4: the group's four pixels share ONE sample (j >> 2 = 0 below): a byte load, aligned wherever it lies
            u4 = a.plane[1][ci], v4 = a.plane[2][ci];
        } else if (hsh) {
            u4 = *reinterpret_cast<const uint16_t*>(a.plane[1] + ci), v4 = *reinterpret_cast<const uint16_t*>(a.plane[2] + ci);
        } else {
            u4 = *reinterpret_cast<const uint32_t*>(a.plane[1] + ci), v4 = *reinterpret_cast<const uint32_t*>(a.plane[2] + ci);
        }
    }
    const int rsh = a.channel_order == WHENET_BGR ? 16 : 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int yy = int((y4 >> (8 * j)) & 255u);
        int b = yy, g = yy, r = yy;
        if (a.g.comps == 3) jpeg_dec_pixel(yy, int((u4 >> (8 * (j >> hsh))) & 255u), int((v4 >> (8 * (j >> hsh))) & 255u), b, g, r);
        px[j] = (uint32_t(r) << rsh) | (uint32_t(g) << 8) | (uint32_t(b) << (16 - rsh));
    }
}

// Rule 1 (libjpeg): fancy upsampling and jdcolor's row.  A lane's 4 pixels lie over the chroma columns i and i + 1 (x = 2 i); it
// needs those and the two neighbour columns i - 1 and i + 2, from its own chroma row and, for 4:2:0, the one vertical neighbour
// (above for even y, below for odd y).  Every index is clamped to the REAL plane (ch x cw): what the padding holds never enters.
template <>
__device__ __forceinline__ void frame_group<JPEG_RULE_LIBJPEG>(const JpegDecArgs& a, int y, int x, uint32_t px[4]) {
    const int h = a.g.h, w = a.g.w;
    const uint32_t y4 = *reinterpret_cast<const uint32_t*>(a.plane[0] + size_t(y) * size_t(a.g.plane_pitch[0]) + size_t(x));
    const int hsh = jpeg_dec_shift(a.g.hs), vsh = jpeg_dec_shift(a.g.vs);
    const int ch = (h + a.g.vs - 1) >> vsh, cw = (w + a.g.hs - 1) >> hsh;
    int uv[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};      // Cb, Cr of the 4 pixels
    if (a.g.comps == 3) {
        const int cr = y >> vsh;
        if (hsh == 0 && vsh == 0) {                   // 4:4:4: the samples themselves (x + 3 lies inside the padded plane)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const uint32_t v = *reinterpret_cast<const uint32_t*>(a.plane[c + 1] + size_t(cr) * size_t(a.g.plane_pitch[c + 1]) + size_t(x));
#pragma unroll
                for (int j = 0; j < 4; ++j) uv[c][j] = int((v >> (8 * j)) & 255u);
            }
        } else if (hsh == 0) {                        // 4:4:0: the vertical filter alone, at every width (h1v2_fancy_upsample); the
            // neighbour row is clamped to the real plane, the columns x .. x + 3 lie inside the padded one (a dword each, aligned)
            const int cn = min(max(cr + ((y & 1) ? 1 : -1), 0), ch - 1);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const uint32_t own = *reinterpret_cast<const uint32_t*>(a.plane[c + 1] + size_t(cr) * size_t(a.g.plane_pitch[c + 1]) + size_t(x));
                const uint32_t oth = *reinterpret_cast<const uint32_t*>(a.plane[c + 1] + size_t(cn) * size_t(a.g.plane_pitch[c + 1]) + size_t(x));
#pragma unroll
                for (int j = 0; j < 4; ++j) uv[c][j] = jpeg_fancy_v(int((own >> (8 * j)) & 255u), int((oth >> (8 * j)) & 255u), (y & 1) != 0);
            }
        } else if (hsh == 2) {                        // 4:1:1, 4:1:0: replication in both directions (int_upsample): one byte per group
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int s = a.plane[c + 1][size_t(cr) * size_t(a.g.plane_pitch[c + 1]) + size_t(x >> 2)];
                uv[c][0] = uv[c][1] = uv[c][2] = uv[c][3] = s;
            }
        } else if (cw <= 2) {                         // libjpeg's own switch: replication, no vertical filter either
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const uint8_t* row = a.plane[c + 1] + size_t(cr) * size_t(a.g.plane_pitch[c + 1]);
                const int s0 = row[0], s1 = row[cw - 1];      // x = 0: columns 0 and min(1, cw - 1)
                uv[c][0] = uv[c][1] = s0, uv[c][2] = uv[c][3] = s1;
            }
        } else {
            const bool v2 = vsh != 0;
            const int cn = v2 ? min(max(cr + ((y & 1) ? 1 : -1), 0), ch - 1) : cr;
            const int i = x >> 1;                     // < cw: x < w
            const int cm = max(i - 1, 0), c1 = min(i + 1, cw - 1), c2 = min(i + 2, cw - 1);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const uint8_t* row = a.plane[c + 1] + size_t(cr) * size_t(a.g.plane_pitch[c + 1]);
                const uint8_t* other = a.plane[c + 1] + size_t(cn) * size_t(a.g.plane_pitch[c + 1]);
                const int sm = jpeg_fancy_col(row[cm], other[cm], v2), s0 = jpeg_fancy_col(row[i], other[i], v2);
                const int s1 = jpeg_fancy_col(row[c1], other[c1], v2), s2 = jpeg_fancy_col(row[c2], other[c2], v2);
                uv[c][0] = jpeg_fancy_up(s0, sm, false, v2), uv[c][1] = jpeg_fancy_up(s0, s1, true, v2);
                uv[c][2] = jpeg_fancy_up(s1, s0, false, v2), uv[c][3] = jpeg_fancy_up(s1, s2, true, v2);
            }
        }
    }
    const int rsh = a.channel_order == WHENET_BGR ? 16 : 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int yy = int((y4 >> (8 * j)) & 255u);
        int b = yy, g = yy, r = yy;
        if (a.g.comps == 3) jpeg_ycc_pixel(yy, uv[0][j], uv[1][j], b, g, r);
        px[j] = (uint32_t(r) << rsh) | (uint32_t(g) << 8) | (uint32_t(b) << (16 - rsh));
    }
}

// the upright frame: a lane's group goes where it came from
template <int RULE>
__device__ __forceinline__ void frame_body(const JpegDecArgs& a, int bx) {
    const int h = a.g.h, w = a.g.w, gw = (w + 3) >> 2;
    const long long item = (long long)(bx) * THREADS + threadIdx.x;
    const int y = int(item / gw), gx = int(item - (long long)(y) * gw);
    if (y >= h) return;
    const int x = gx << 2;
    const int n = min(4, w - x);                    // pixels of the group, 1..4
    uint32_t px[4];
    frame_group<RULE>(a, y, x, px);
    store_group(a.dst[0] + size_t(y) * size_t(a.dst_pitch[0]) + size_t(x) * 3, px, n);
}

// ---- the ORIENTED frame (JpegDecArgs::orient = 2..8; jpeg_dec_host.h: jpeg_orient_source): the pixel of source position (y, x) is
// frame_group's, only its destination differs.
//   2, 3, 4 (rows stay rows): the upright mapping, a group per lane.  The destination row is y or h - 1 - y; where x runs against the
//            destination the group's pixels are reversed and stored at w - x - n: generally unaligned, which store_group's head and
//            tail bytes take, and the row's short group (n < 4) lands at the row's START with exactly its 3 n bytes.
//   5..8 (rows become columns): a workgroup owns a 32 x 32 tile of the DESTINATION (oh = w rows, ow = h columns).  The source pixels
//            that map into it are a block of <= 32 rows and <= 32 columns whose first column need not be a multiple of 4 (7 and 8:
//            x = w - 1 - Y): the lanes compute the <= 9 aligned source groups per row that cover it (plane reads along rows) and
//            put each pixel that lies inside the tile into LDS at its DESTINATION place, a dword per pixel, rows 33 dwords apart
//            (the four pixels of a group go to four tile rows, the lanes of a source row to one tile column: with a pitch of 32
//            the <= 9 lanes of a source row would store to ONE bank, with 33 they are 4 banks apart: a 32-lane group of a whole
//            tile -- 4 source rows of 8 groups -- stores to 32 different banks, and so do the dword reads behind the barrier).
//            After the barrier lane t stores group t & 7 of tile row t >> 3: eight lanes write 96 contiguous bytes of a
//            destination row.  Tiling the destination keeps every stored group on the destination's own 4-pixel grid, so the
//            row's tail is the short one.
constexpr int ORIENT_TILE = 32, ORIENT_PITCH = ORIENT_TILE + 1;
static_assert(ORIENT_TILE * (ORIENT_TILE / 4) == THREADS, "a lane stores one group of the tile");

// workgroups of the oriented frame kernel for one stream
inline long long orient_workgroups(const JpegDecGeom& g, int orient) {
    if (orient < 5) return ((long long)(g.h) * ((g.w + 3) >> 2) + THREADS - 1) / THREADS;
    return (long long)((g.w + ORIENT_TILE - 1) / ORIENT_TILE) * ((g.h + ORIENT_TILE - 1) / ORIENT_TILE);
}

template <int RULE>
__device__ __forceinline__ void frame_oriented_body(const JpegDecArgs& a, int bx) {
    // (one kernel for the seven values, so that a clip's turned frames are ONE launch: the 4,224 B tile is allocated for the values 2..4
    // as well, which never touch it -- at 27 / 44 VGPRs the LDS does not bound the workgroups per CU)
    __shared__ uint32_t s_tile[ORIENT_TILE * ORIENT_PITCH];
    const int h = a.g.h, w = a.g.w, o = a.orient;
    const bool fx = jpeg_orient_flip_x(o), fy = jpeg_orient_flip_y(o);
    const int tid = int(threadIdx.x);
    if (o < 5) {
        const int gw = (w + 3) >> 2;
        const long long item = (long long)(bx) * THREADS + tid;
        const int y = int(item / gw), gx = int(item - (long long)(y) * gw);
        if (y >= h) return;
        const int x = gx << 2;
        const int n = min(4, w - x);
        uint32_t px[4];
        frame_group<RULE>(a, y, x, px);
        if (fx) {      // pixel j of the n goes to n - 1 - j
            uint32_t r[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = px[j];
#pragma unroll
            for (int j = 0; j < 4; ++j) px[j] = n == 4 ? r[3 - j] : (n == 3 ? r[(2 - j) & 3] : (n == 2 ? r[(1 - j) & 3] : r[0]));
        }
        const int Y = fy ? h - 1 - y : y, X = fx ? w - x - n : x;      // X + n <= w
        store_group(a.dst[0] + size_t(Y) * size_t(a.dst_pitch[0]) + size_t(X) * 3, px, n);
        return;
    }
    // the destination is w rows of h pixels
    const int tiles_x = (h + ORIENT_TILE - 1) / ORIENT_TILE;
    const int Y0 = (bx / tiles_x) * ORIENT_TILE, X0 = (bx % tiles_x) * ORIENT_TILE;
    const int rows = min(ORIENT_TILE, w - Y0), cols = min(ORIENT_TILE, h - X0);      // of the tile, inside the destination: >= 1
    // the source block: x over the tile's rows, y over its columns
    const int xlo = fx ? w - Y0 - rows : Y0, xhi = xlo + rows - 1, ylo = fy ? h - X0 - cols : X0;
    const int g0 = xlo >> 2, ng = (xhi >> 2) - g0 + 1;      // <= 9 groups per source row
    for (int it = tid; it < cols * ng; it += THREADS) {
        const int r = it / ng, gi = it - r * ng;
        const int y = ylo + r, x = (g0 + gi) << 2;            // y < h, x <= xhi < w
        uint32_t px[4];
        frame_group<RULE>(a, y, x, px);
        const int Xl = (fy ? h - 1 - y : y) - X0;             // 0 .. cols - 1
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xx = x + j;
            const int Yl = (fx ? w - 1 - xx : xx) - Y0;       // inside the tile where xlo <= xx <= xhi
            if (xx >= xlo && xx <= xhi) s_tile[Yl * ORIENT_PITCH + Xl] = px[j];
        }
    }
    __syncthreads();
    const int Yl = tid >> 3, Xl = (tid & 7) << 2;
    if (Yl >= rows || Xl >= cols) return;
    const int n = min(4, cols - Xl);
    uint32_t px[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) px[j] = j < n ? s_tile[Yl * ORIENT_PITCH + Xl + j] : 0u;
    store_group(a.dst[0] + size_t(Y0 + Yl) * size_t(a.dst_pitch[0]) + size_t(X0 + Xl) * 3, px, n);
}

// up to 4 bytes of `word` to dp: one dword where all four are the row's and dp is aligned
__device__ __forceinline__ void store_bytes(uint8_t* dp, uint32_t word, int n) {
    if (n == 4 && (reinterpret_cast<uintptr_t>(dp) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(dp) = word;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) dp[j] = uint8_t(word >> (8 * j));
    }
}

// items: the luma plane's 4-byte groups row by row, then the chroma rows' groups of 4 samples (U and V of a group by one lane)
__device__ __forceinline__ void yuv_body(const JpegDecArgs& a, int bx) {
    const int h = a.g.h, w = a.g.w, ch = (h + 1) >> 1, cw = (w + 1) >> 1, gw = (w + 3) >> 2, cgw = (cw + 3) >> 2;
    long long item = (long long)(bx) * THREADS + threadIdx.x;
    const long long luma_items = (long long)(h) * gw;
    if (item < luma_items) {
        const int y = int(item / gw), x = int(item - (long long)(y) * gw) << 2;
        const uint32_t v = *reinterpret_cast<const uint32_t*>(a.plane[0] + size_t(y) * size_t(a.g.plane_pitch[0]) + size_t(x));
        store_bytes(a.dst[0] + size_t(y) * size_t(a.dst_pitch[0]) + size_t(x), v, min(4, w - x));
        return;
    }
    item -= luma_items;
    const int y = int(item / cgw), x = int(item - (long long)(y) * cgw) << 2;
    if (y >= ch) return;
    const int n = min(4, cw - x);
    const size_t ci = size_t(y) * size_t(a.g.plane_pitch[1]) + size_t(x);
    const uint32_t u = *reinterpret_cast<const uint32_t*>(a.plane[1] + ci), v = *reinterpret_cast<const uint32_t*>(a.plane[2] + ci);
    if (a.format == WHENET_YUV_I420) {
        store_bytes(a.dst[1] + size_t(y) * size_t(a.dst_pitch[1]) + size_t(x), u, n);
        store_bytes(a.dst[2] + size_t(y) * size_t(a.dst_pitch[2]) + size_t(x), v, n);
    } else {
        uint8_t* dp = a.dst[1] + size_t(y) * size_t(a.dst_pitch[1]) + 2 * size_t(x);
        const uint32_t lo = (u & 255u) | ((v & 255u) << 8) | ((u & 0xFF00u) << 8) | ((v & 0xFF00u) << 16);
        const uint32_t hi = ((u >> 16) & 255u) | (((v >> 16) & 255u) << 8) | ((u >> 24) << 16) | ((v >> 24) << 24);
        store_bytes(dp, lo, min(4, 2 * n));
        if (n > 2) store_bytes(dp + 4, hi, 2 * n - 4);
    }
}

// ---- the single-stream kernels: the record by value, the grid that stream's ----
__global__ __launch_bounds__(THREADS) void whenet_jpeg_dec_scan_kernel(JpegDecArgs a) { scan_body(a); }
__global__ __launch_bounds__(ENT_THREADS) void whenet_jpeg_dec_entropy_kernel(JpegDecArgs a) { entropy_body(a, int(blockIdx.x)); }
__global__ __launch_bounds__(THREADS) void whenet_jpeg_dec_idct_kernel(JpegDecArgs a) { idct_body<JPEG_RULE_OWN>(a, int(blockIdx.x)); }
__global__ __launch_bounds__(THREADS) void whenet_jpeg_dec_frame_kernel(JpegDecArgs a) { frame_body<JPEG_RULE_OWN>(a, int(blockIdx.x)); }
// rule 1 (libjpeg): the same mappings, its arithmetic
__global__ __launch_bounds__(THREADS) void whenet_jpeg_dec_idct_libjpeg_kernel(JpegDecArgs a) { idct_body<JPEG_RULE_LIBJPEG>(a, int(blockIdx.x)); }
__global__ __launch_bounds__(THREADS) void whenet_jpeg_dec_frame_libjpeg_kernel(JpegDecArgs a) { frame_body<JPEG_RULE_LIBJPEG>(a, int(blockIdx.x)); }
// the oriented frame (orient 2..8) under either rule, in the frame kernel's place
__global__ __launch_bounds__(THREADS) void whenet_jpeg_dec_frame_oriented_kernel(JpegDecArgs a) { frame_oriented_body<JPEG_RULE_OWN>(a, int(blockIdx.x)); }
__global__ __launch_bounds__(THREADS) void whenet_jpeg_dec_frame_oriented_libjpeg_kernel(JpegDecArgs a) {
    frame_oriented_body<JPEG_RULE_LIBJPEG>(a, int(blockIdx.x));
}
__global__ __launch_bounds__(THREADS) void whenet_jpeg_dec_yuv_kernel(JpegDecArgs a) { yuv_body(a, int(blockIdx.x)); }

// ---- the clip kernels: up to 16 records in device memory (recs), the frames' workgroups back to back in one grid.  A workgroup
// finds its frame (kernels.h, jpeg_clip_frame_of: wave-uniform), copies that frame's record -- the address is the same for every
// lane and the memory is read-only for the kernel: scalar loads -- and runs the body with its index inside the frame's share.  A
// workgroup never straddles two frames (the LDS tables of the entropy body are one frame's): a frame's last workgroup has idle
// lanes instead.  A workgroup behind the grid's total exits before it touches memory.
// The record is read where it lies (a reference, not a copy: a copy whose address the non-inlined decode functions take went to
// 296 bytes of scratch per lane).  Resource report (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), VGPRs of
// the clip form / of the single-stream form, no scratch in either, the same LDS: scan 44 / 44, entropy 47 / 48, idct 47 / 47,
// frame 18 / 18, yuv 14 / 14; SGPRs grow by up to 21 (the prefix sums and the record's address).  Rule 1: idct 36 / 36, frame 38 / 38.
// The oriented frame kernels: 28 / 27 under rule 0 and 44 / 44 under rule 1, 4,224 B of LDS in all four, no scratch.
#define WHENET_JPEG_CLIP_KERNEL(name, threads, call)                                                                       \
    __global__ __launch_bounds__(threads) void name(const void* __restrict__ recs, JpegClipGrid grid) {                    \
        const int b = int(blockIdx.x);                                                                                     \
        if (b >= grid.total) return;                                                                                       \
        const int f = jpeg_clip_frame_of(grid, b);                                                                         \
        const JpegDecArgs& a = jpeg_clip_record(recs, f);                                                                  \
        const int bx = b - grid.first[f];                                                                                  \
        (void)bx;                                                                                                          \
        call;                                                                                                              \
    }
WHENET_JPEG_CLIP_KERNEL(whenet_jpeg_dec_clip_scan_kernel, THREADS, scan_body(a))
WHENET_JPEG_CLIP_KERNEL(whenet_jpeg_dec_clip_entropy_kernel, ENT_THREADS, entropy_body(a, bx))
WHENET_JPEG_CLIP_KERNEL(whenet_jpeg_dec_clip_idct_kernel, THREADS, idct_body<JPEG_RULE_OWN>(a, bx))
WHENET_JPEG_CLIP_KERNEL(whenet_jpeg_dec_clip_frame_kernel, THREADS, frame_body<JPEG_RULE_OWN>(a, bx))
WHENET_JPEG_CLIP_KERNEL(whenet_jpeg_dec_clip_idct_libjpeg_kernel, THREADS, idct_body<JPEG_RULE_LIBJPEG>(a, bx))
WHENET_JPEG_CLIP_KERNEL(whenet_jpeg_dec_clip_frame_libjpeg_kernel, THREADS, frame_body<JPEG_RULE_LIBJPEG>(a, bx))
WHENET_JPEG_CLIP_KERNEL(whenet_jpeg_dec_clip_frame_oriented_kernel, THREADS, frame_oriented_body<JPEG_RULE_OWN>(a, bx))
WHENET_JPEG_CLIP_KERNEL(whenet_jpeg_dec_clip_frame_oriented_libjpeg_kernel, THREADS, frame_oriented_body<JPEG_RULE_LIBJPEG>(a, bx))
WHENET_JPEG_CLIP_KERNEL(whenet_jpeg_dec_clip_yuv_kernel, THREADS, yuv_body(a, bx))
#undef WHENET_JPEG_CLIP_KERNEL

static_assert(sizeof(JpegDecArgs) <= JPEG_CLIP_RECORD_BYTES && JPEG_CLIP_RECORD_BYTES % 16 == 0, "a record fits its stride");

// everything launch_jpeg_decode asks of one stream's record, the layout apart
void check_jpeg_dec_args(const JpegDecArgs& a) {
    const JpegDecGeom& g = a.g;
    int rows[3], row_bytes[3];
    WHENET_REQUIRE(a.orient >= 0 && a.orient <= 8 && (a.orient <= 1 || a.format == WHENET_SURF_PACKED), WHENET_EINVAL,
                   "jpeg_decode: the orientation must be 0..8, and an oriented decode (2..8) writes packed surfaces only");
    // (the destination is the ORIENTED frame: for 5..8 g.w rows of 3 g.h bytes)
    const int planes = overlay_surface_planes(a.format, jpeg_orient_h(a.orient, g.h, g.w), jpeg_orient_w(a.orient, g.h, g.w), rows, row_bytes);
    WHENET_REQUIRE(planes > 0 && g.h >= 1 && g.w >= 1 && g.h <= JPEG_MAX_SIDE && g.w <= JPEG_MAX_SIDE && (g.comps == 1 || g.comps == 3) &&
                       (g.hs == 1 || g.hs == 2 || (g.hs == 4 && g.comps == 3)) && (g.vs == 1 || g.vs == 2) && g.bpm == (g.comps == 3 ? g.hs * g.vs + 2 : 1) &&
                       g.mcu_cols == (g.w + 8 * g.hs - 1) / (8 * g.hs) && g.mcu_rows == (g.h + 8 * g.vs - 1) / (8 * g.vs) && g.ri >= 1 &&
                       (long long)(g.intervals) == ((long long)(g.mcu_cols) * g.mcu_rows + g.ri - 1) / g.ri,
                   WHENET_EINVAL, "jpeg_decode: bad geometry");
    WHENET_REQUIRE(a.tables != nullptr && a.data != nullptr && a.nbytes >= 0 && a.start != nullptr && a.meta != nullptr && a.coef != nullptr &&
                       a.status != nullptr && (a.format == WHENET_SURF_PACKED || (g.comps == 3 && g.hs == 2 && g.vs == 2)),
                   WHENET_EINVAL, "jpeg_decode: bad arguments");
    for (int c = 0; c < g.comps; ++c)
        WHENET_REQUIRE(a.plane[c] != nullptr && reinterpret_cast<uintptr_t>(a.plane[c]) % 8 == 0 && g.plane_pitch[c] % 8 == 0 &&
                           g.plane_pitch[c] >= (c == 0 ? g.w : (g.w + g.hs - 1) / g.hs) && g.plane_rows[c] >= (c == 0 ? g.h : (g.h + g.vs - 1) / g.vs),
                       WHENET_EINVAL, "jpeg_decode: bad component plane " + std::to_string(c));
    for (int p = 0; p < planes; ++p)
        WHENET_REQUIRE(a.dst[p] != nullptr && a.dst_pitch[p] >= row_bytes[p], WHENET_EINVAL, "jpeg_decode: bad destination plane " + std::to_string(p));
    WHENET_REQUIRE(a.format != WHENET_SURF_PACKED || a.channel_order == WHENET_RGB || a.channel_order == WHENET_BGR, WHENET_EINVAL,
                   "jpeg_decode: unknown channel order");
    WHENET_REQUIRE(a.form == 0 || a.form == 1, WHENET_EINVAL, "jpeg_decode: the entropy form must be 0 or 1");
    WHENET_REQUIRE(jpeg_rule_ok(a.rule) && (a.rule == JPEG_RULE_OWN || a.format == WHENET_SURF_PACKED), WHENET_EINVAL,
                   "jpeg_decode: the rule must be 0 or 1, and rule 1 (libjpeg) decodes to WHENET_SURF_PACKED only");
    if (a.form == 1)
        WHENET_REQUIRE(jpeg_seg_bytes_ok(a.seg_bytes) && (long long)(a.seg_cap) == jpeg_seg_bound(a.nbytes, g.intervals, a.seg_bytes) &&
                           a.seg_stats != nullptr && a.first_seg != nullptr && a.seg_exit != nullptr && a.seg_count != nullptr && a.seg_blk != nullptr,
                       WHENET_EINVAL, "jpeg_decode: the work buffers are not those of the segmented form of this stream");
}

// the colour path of a stream: 0 the plane kernel of the YUV ingest (a tight BGR frame of a 4:2:0 stream under rule 0), 1 the frame
// kernel of the stream's rule, 2 the I420 / NV12 copy, 3 the oriented frame kernel of the stream's rule (orient 2..8)
int colour_path(const JpegDecArgs& a) {
    if (a.format != WHENET_SURF_PACKED) return 2;
    if (a.orient > 1) return 3;
    if (a.rule == JPEG_RULE_LIBJPEG) return 1;
    return a.g.comps == 3 && a.g.hs == 2 && a.g.vs == 2 && a.channel_order == WHENET_BGR && a.dst_pitch[0] == 3 * a.g.w ? 0 : 1;
}

}  // namespace

JpegDecScratch::JpegDecScratch(const JpegDecGeom& g, size_t data_bytes, long long nbytes, int form_, int seg_bytes_) {
    const auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
    tables = 0;
    data = up(sizeof(JpegDecTables));
    upload_bytes = data + data_bytes;
    start = up(upload_bytes);
    meta = up(start + size_t(g.intervals) * sizeof(int32_t));
    seg_stats = meta + 64;
    coef = up(seg_stats + 8 * sizeof(long long));
    zero_bytes = coef - start;
    coef_bytes = size_t(g.mcu_cols) * size_t(g.mcu_rows) * size_t(g.bpm) * 64 * sizeof(int16_t);
    size_t at = up(coef + coef_bytes);
    for (int c = 0; c < 3; ++c) {
        plane[c] = at;
        if (c < g.comps) at = up(at + size_t(g.plane_pitch[c]) * size_t(g.plane_rows[c]));
    }
    form = form_, seg_bytes = form_ == 1 ? seg_bytes_ : 0, seg_cap = 0;
    first_seg = seg_exit = seg_count = seg_blk = at;
    if (form == 1) {
        WHENET_REQUIRE(jpeg_seg_bytes_ok(seg_bytes), WHENET_EINVAL, "jpeg_decode: seg_bytes must be a power of two in 4..4096");
        seg_cap = jpeg_seg_bound(nbytes < 0 ? (long long)(data_bytes) : nbytes, g.intervals, seg_bytes);
        WHENET_REQUIRE(seg_cap < 0x7FFFFFFF, WHENET_EINVAL, "jpeg_decode: more segments than an int32 counts");
        first_seg = at, at = up(at + (size_t(g.intervals) + 1) * sizeof(int32_t));
        seg_exit = at, at = up(at + size_t(seg_cap) * sizeof(uint64_t));
        seg_count = at, at = up(at + size_t(seg_cap) * sizeof(JpegSegCount));
        seg_blk = at, at = up(at + size_t(seg_cap) * 4 * sizeof(int32_t));
    }
    bytes = at;
}

void launch_jpeg_decode(const JpegDecArgs& a, const JpegDecScratch& lay, hipStream_t stream) {
    const JpegDecGeom& g = a.g;
    check_jpeg_dec_args(a);
    WHENET_REQUIRE(lay.coef_bytes == size_t(g.mcu_cols) * size_t(g.mcu_rows) * size_t(g.bpm) * 128, WHENET_EINVAL,
                   "jpeg_decode: the work buffers are not those of the stream's geometry");
    // start | meta (contiguous) and the coefficient records start from zero
    WHENET_HIP_CHECK(hipMemsetAsync(a.start, 0, lay.zero_bytes, stream));
    WHENET_HIP_CHECK(hipMemsetAsync(a.coef, 0, lay.coef_bytes, stream));
    hipLaunchKernelGGL(whenet_jpeg_dec_scan_kernel, dim3(1), dim3(THREADS), 0, stream, a);
    WHENET_HIP_CHECK(hipGetLastError());
    // the entropy stage in the form the caller's layout was made for: an interval per lane, or the segmented form (jpeg_dec_seg.hip)
    WHENET_REQUIRE(a.form == 0 || a.form == 1, WHENET_EINVAL, "jpeg_decode: the entropy form must be 0 or 1");
    if (a.form == 1) {
        WHENET_REQUIRE(lay.form == 1 && jpeg_seg_bytes_ok(a.seg_bytes) && a.seg_bytes == lay.seg_bytes &&
                           (long long)(a.seg_cap) == jpeg_seg_bound(a.nbytes, g.intervals, a.seg_bytes) && (long long)(a.seg_cap) <= lay.seg_cap &&
                           a.seg_stats != nullptr && a.first_seg != nullptr && a.seg_exit != nullptr && a.seg_count != nullptr && a.seg_blk != nullptr,
                       WHENET_EINVAL, "jpeg_decode: the work buffers are not those of the segmented form of this stream");
        launch_jpeg_decode_segmented(a, stream);
    } else {
        hipLaunchKernelGGL(whenet_jpeg_dec_entropy_kernel, dim3((g.intervals + ENT_LANES - 1) / ENT_LANES), dim3(ENT_THREADS), 0, stream, a);
    }
    WHENET_HIP_CHECK(hipGetLastError());
    launch_jpeg_decode_tail(a, stream);
}

void launch_jpeg_decode_tail(const JpegDecArgs& a, hipStream_t stream) {
    const JpegDecGeom& g = a.g;
    check_jpeg_dec_args(a);
    const long long nblocks = (long long)(g.mcu_cols) * g.mcu_rows * g.bpm;
    hipLaunchKernelGGL(a.rule == JPEG_RULE_LIBJPEG ? whenet_jpeg_dec_idct_libjpeg_kernel : whenet_jpeg_dec_idct_kernel,
                       dim3(unsigned((nblocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS)), dim3(THREADS), 0, stream, a);
    WHENET_HIP_CHECK(hipGetLastError());
    if (colour_path(a) == 3) {
        hipLaunchKernelGGL(a.rule == JPEG_RULE_LIBJPEG ? whenet_jpeg_dec_frame_oriented_libjpeg_kernel : whenet_jpeg_dec_frame_oriented_kernel,
                           dim3(unsigned(orient_workgroups(g, a.orient))), dim3(THREADS), 0, stream, a);
    } else if (a.format == WHENET_SURF_PACKED) {
        if (colour_path(a) == 0) {
            // a tight BGR frame of a 4:2:0 stream: the plane kernel of the YUV ingest, JFIF row
            YuvPlanes clip{};
            clip.frames = 1;
            YuvPlanesFrame& f = clip.f[0];
            for (int c = 0; c < 3; ++c) f.plane[c] = a.plane[c], f.pitch[c] = g.plane_pitch[c];
            f.h = g.h, f.w = g.w, f.format = WHENET_YUV_I420, f.k = yuv_coeffs(WHENET_YUV_JFIF), f.dst_off = 0;
            launch_yuv_planes_to_bgr(a.dst[0], clip, stream);
            return;
        }
        const long long items = (long long)(g.h) * ((g.w + 3) >> 2);
        hipLaunchKernelGGL(a.rule == JPEG_RULE_LIBJPEG ? whenet_jpeg_dec_frame_libjpeg_kernel : whenet_jpeg_dec_frame_kernel,
                           dim3(unsigned((items + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, a);
    } else {
        const long long items = (long long)(g.h) * ((g.w + 3) >> 2) + (long long)((g.h + 1) >> 1) * ((((g.w + 1) >> 1) + 3) >> 2);
        hipLaunchKernelGGL(whenet_jpeg_dec_yuv_kernel, dim3(unsigned((items + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, a);
    }
    WHENET_HIP_CHECK(hipGetLastError());
}

void launch_jpeg_decode_clip(const JpegDecArgs* h_recs, const void* d_recs, int frames, void* d_zero, size_t zero_bytes, hipStream_t stream,
                             int64_t* enqueues) {
    launch_jpeg_decode_clip_entropy(h_recs, d_recs, frames, d_zero, zero_bytes, stream, enqueues, nullptr);
    launch_jpeg_decode_clip_tail(h_recs, d_recs, frames, stream, enqueues);
}

void launch_jpeg_decode_clip_entropy(const JpegDecArgs* h_recs, const void* d_recs, int frames, void* d_zero, size_t zero_bytes, hipStream_t stream,
                                     int64_t* enqueues, const uint8_t* progressive) {
    WHENET_REQUIRE(h_recs != nullptr && d_recs != nullptr && d_zero != nullptr && frames >= 1 && frames <= MIXED_MAX_FRAMES, WHENET_EINVAL,
                   "jpeg_decode_clip: NULL argument, or a frame count outside 1..16");
    const auto prog = [&](int f) { return progressive != nullptr && progressive[f] != 0; };
    for (int f = 0; f < frames; ++f) {
        const JpegDecArgs& a = h_recs[f];
        check_jpeg_dec_args(a);
        // what the one memset must cover: the frame's start | meta | seg_stats and its coefficient records
        const char *z0 = static_cast<const char*>(d_zero), *z1 = z0 + zero_bytes;
        const size_t coef_bytes = size_t(a.g.mcu_cols) * size_t(a.g.mcu_rows) * size_t(a.g.bpm) * 128;
        const auto zeroed = [&](const void* p, size_t n) { return static_cast<const char*>(p) >= z0 && static_cast<const char*>(p) + n <= z1; };
        WHENET_REQUIRE(a.rule == h_recs[0].rule, WHENET_EINVAL, "jpeg_decode_clip: the frames of a clip are decoded by one rule");
        // (a progressive frame: meta here, its raw coefficients in launch_jpeg_decode_clip_progressive; form 0 keeps it out of the segmented stages)
        WHENET_REQUIRE(prog(f) ? zeroed(a.meta, 8) && a.form == 0
                               : zeroed(a.start, size_t(a.g.intervals) * 4) && zeroed(a.meta, 8) && zeroed(a.seg_stats, 64) && zeroed(a.coef, coef_bytes),
                       WHENET_EINVAL, "jpeg_decode_clip: frame " + std::to_string(f) + ": its zeroed regions lie outside the clip's");
    }
    int64_t n = 0;
    JpegClipGrid grid;
    const auto launch = [&](auto kernel, int threads) {
        hipLaunchKernelGGL(kernel, dim3(unsigned(grid.total)), dim3(unsigned(threads)), 0, stream, d_recs, grid);
        WHENET_HIP_CHECK(hipGetLastError());
        ++n;
    };
    WHENET_HIP_CHECK(hipMemsetAsync(d_zero, 0, zero_bytes, stream));
    ++n;
    // (the counts see the records only: a progressive frame is told by its address in h_recs)
    const auto base = [&](const JpegDecArgs& a) { return !prog(int(&a - h_recs)); };
    if (jpeg_clip_grid(h_recs, frames, [&](const JpegDecArgs& a) { return base(a) ? 1 : 0; }, grid)) launch(whenet_jpeg_dec_clip_scan_kernel, THREADS);
    if (jpeg_clip_grid(h_recs, frames,
                       [&](const JpegDecArgs& a) { return base(a) && a.form == 0 ? (a.g.intervals + ENT_LANES - 1) / ENT_LANES : 0; }, grid))
        launch(whenet_jpeg_dec_clip_entropy_kernel, ENT_THREADS);
    if (enqueues != nullptr) *enqueues += n;
    launch_jpeg_decode_segmented_clip(h_recs, d_recs, frames, stream, enqueues);
}

void launch_jpeg_decode_clip_tail(const JpegDecArgs* h_recs, const void* d_recs, int frames, hipStream_t stream, int64_t* enqueues) {
    WHENET_REQUIRE(h_recs != nullptr && d_recs != nullptr && frames >= 1 && frames <= MIXED_MAX_FRAMES, WHENET_EINVAL,
                   "jpeg_decode_clip: NULL argument, or a frame count outside 1..16");
    int64_t n = 0;
    JpegClipGrid grid;
    const auto launch = [&](auto kernel, int threads) {
        hipLaunchKernelGGL(kernel, dim3(unsigned(grid.total)), dim3(unsigned(threads)), 0, stream, d_recs, grid);
        WHENET_HIP_CHECK(hipGetLastError());
        ++n;
    };
    jpeg_clip_grid(h_recs, frames,
              [](const JpegDecArgs& a) { return ((long long)(a.g.mcu_cols) * a.g.mcu_rows * a.g.bpm + IDCT_BLOCKS - 1) / IDCT_BLOCKS; }, grid);
    // (one rule per clip: its idct and frame kernels stand for rule 0's, the number of launches does not grow)
    const bool libjpeg = h_recs[0].rule == JPEG_RULE_LIBJPEG;
    if (libjpeg) launch(whenet_jpeg_dec_clip_idct_libjpeg_kernel, THREADS);
    else launch(whenet_jpeg_dec_clip_idct_kernel, THREADS);
    // the colour stage: each of the three paths once, for the frames that take it
    YuvPlanes tight{};
    uintptr_t base = ~uintptr_t(0);
    for (int f = 0; f < frames; ++f)
        if (colour_path(h_recs[f]) == 0) base = std::min(base, reinterpret_cast<uintptr_t>(h_recs[f].dst[0]));
    for (int f = 0; f < frames; ++f) {
        const JpegDecArgs& a = h_recs[f];
        if (colour_path(a) != 0) continue;
        YuvPlanesFrame& y = tight.f[tight.frames++];
        for (int c = 0; c < 3; ++c) y.plane[c] = a.plane[c], y.pitch[c] = a.g.plane_pitch[c];
        y.h = a.g.h, y.w = a.g.w, y.format = WHENET_YUV_I420, y.k = yuv_coeffs(WHENET_YUV_JFIF);
        y.dst_off = reinterpret_cast<uintptr_t>(a.dst[0]) - base;
    }
    if (tight.frames > 0) launch_yuv_planes_to_bgr(reinterpret_cast<uint8_t*>(base), tight, stream), ++n;
    if (jpeg_clip_grid(h_recs, frames,
                  [](const JpegDecArgs& a) { return colour_path(a) == 1 ? ((long long)(a.g.h) * ((a.g.w + 3) >> 2) + THREADS - 1) / THREADS : 0; }, grid))
        libjpeg ? launch(whenet_jpeg_dec_clip_frame_libjpeg_kernel, THREADS) : launch(whenet_jpeg_dec_clip_frame_kernel, THREADS);
    // (the turned frames of the clip: one launch more where there are any, whatever their number)
    if (jpeg_clip_grid(h_recs, frames, [](const JpegDecArgs& a) { return colour_path(a) == 3 ? orient_workgroups(a.g, a.orient) : 0; }, grid))
        libjpeg ? launch(whenet_jpeg_dec_clip_frame_oriented_libjpeg_kernel, THREADS) : launch(whenet_jpeg_dec_clip_frame_oriented_kernel, THREADS);
    if (jpeg_clip_grid(h_recs, frames,
                  [](const JpegDecArgs& a) {
                      const long long items = (long long)(a.g.h) * ((a.g.w + 3) >> 2) + (long long)((a.g.h + 1) >> 1) * ((((a.g.w + 1) >> 1) + 3) >> 2);
                      return colour_path(a) == 2 ? (items + THREADS - 1) / THREADS : 0;
                  },
                  grid))
        launch(whenet_jpeg_dec_clip_yuv_kernel, THREADS);
    if (enqueues != nullptr) *enqueues += n;
}

}  // namespace whenet
