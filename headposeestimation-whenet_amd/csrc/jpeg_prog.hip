// The progressive JPEG decoder's entropy stage on the device: the scans of a SOF2 stream into raw coefficients, level by level, and
// the finish that leaves the records jpeg_dec.hip's inverse DCT reads.  The format is in include/whenet_hip.h (JPEG DECODER,
// PROGRESSIVE); the arithmetic -- the four scan kinds, the finish of a value -- is jpeg_prog_host.h's, the same functions the host
// statement runs.  Integers only.
//
// Reference: demo.py (`cv2.imread` of Sample/*.jpeg): stills are where progressive streams are common.
//
// What is parallel in a progressive stream: the restart intervals of a scan, and the scans of one LEVEL (kernels.h).  The host has
// found every item's first byte while it looked for the scans' ends, so nothing here scans for markers and every launch size is
// the plan's.
//   whenet_jpeg_prog_scan_kernel    one item per decoding lane, 16 per workgroup, as the baseline form 0: a wave's lanes diverge in
//                                   the Huffman walk.  All 16 belong to one scan, whose record and tables the 64 lanes stage in LDS.
//                                   Scans of one level write other bands of the SAME 128-byte records at the same time: a lane
//                                   stores single int16s of its own band, never a wider word.  An AC refinement copies its band
//                                   into an LDS row of its own, works there and stores the band back.
//   whenet_jpeg_prog_finish_kernel  8 lanes per block: lane l loads the record's zigzag positions 8 l .. 8 l + 7 as 16 bytes,
//                                   multiplies by the quantiser, clamps, scatters to natural order in LDS, and stores the natural
//                                   positions 8 l .. 8 l + 7 as 16 bytes.
#include <string>

#include "kernels.h"

namespace whenet {

namespace {

constexpr int SCAN_THREADS = 64;
constexpr int FIN_THREADS = 256;
constexpr int FIN_BLOCKS = FIN_THREADS / 8;

// zigzag position -> natural index (jpeg_host.h's JPEG_ZIGZAG, as the device addresses it)
__constant__ uint8_t ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

static_assert(sizeof(JpegDecHuff) % 4 == 0 && sizeof(JpegProgScan) % 4 == 0, "copied to LDS by dwords");

// group: the workgroup's index in the item list (16 items each)
__global__ __launch_bounds__(SCAN_THREADS) void whenet_jpeg_prog_scan_kernel(JpegProgArgs a, int first_group) {
    __shared__ JpegDecHuff s_h[3];
    __shared__ JpegProgScan s_sc;
    __shared__ int16_t s_band[JPEG_PROG_LANES][64 + 2];      // an AC refinement's band in hand (132-byte rows)
    const int tid = int(threadIdx.x);
    const long long base = ((long long)(first_group) + blockIdx.x) * JPEG_PROG_LANES;
    const int s = a.items[base].scan;      // (a scan's share begins with a real item: uniform over the workgroup)
    if (s < 0) return;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.scans + s);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&s_sc);
        for (int i = tid; i < int(sizeof(JpegProgScan) / 4); i += SCAN_THREADS) dst[i] = src[i];
        const int kind = a.scans[s].kind;
        const int tables = kind == JPEG_PROG_DC_FIRST ? a.scans[s].ns : (kind == JPEG_PROG_DC_REFINE ? 0 : 1);
        src = reinterpret_cast<const uint32_t*>(a.huff + 3 * size_t(s));
        dst = reinterpret_cast<uint32_t*>(s_h);
        for (int i = tid; i < tables * int(sizeof(JpegDecHuff) / 4); i += SCAN_THREADS) dst[i] = src[i];
    }
    __syncthreads();
    if (tid >= JPEG_PROG_LANES) return;
    const JpegProgItem it = a.items[base + tid];
    if (it.scan != s || it.interval < 0 || it.interval >= s_sc.intervals || it.start < 0 || it.end > a.nbytes || it.start > it.end) return;
    if (!jpeg_prog_item(a.data, it.start, it.end, s_sc, s_h, a.g, it.interval, a.raw, s_band[tid]))
        atomicMax(&a.meta[0], JPEG_DEC_NO_BAD - (s_sc.first_item + it.interval));
}

__global__ __launch_bounds__(FIN_THREADS) void whenet_jpeg_prog_finish_kernel(JpegProgArgs a) {
    __shared__ __attribute__((aligned(16))) int16_t s_rec[FIN_BLOCKS][64 + 8];
    __shared__ int16_t s_q[3][64];
    const int tid = int(threadIdx.x), lb = tid >> 3, l = tid & 7;
    if (tid < 192) s_q[tid >> 6][tid & 63] = a.qz[tid];
    __syncthreads();
    const long long blk = (long long)(blockIdx.x) * FIN_BLOCKS + lb;
    const long long total = (long long)(a.g.mcu_cols) * a.g.mcu_rows * a.g.bpm;
    const bool live = blk < total;
    if (live) {
        const int bi = int(blk % a.g.bpm), c = a.g.comps == 1 || bi < a.g.bpm - 2 ? 0 : bi - (a.g.bpm - 2) + 1;
        const uint4 v = *reinterpret_cast<const uint4*>(a.raw + size_t(blk) * 64 + 8 * l);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * l + j;
            const int raw = int(int16_t(w[j >> 1] >> (16 * (j & 1))));
            s_rec[lb][ZZ[k]] = jpeg_prog_finish_value(raw, s_q[c][k]);
        }
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0) {      // (the scan kernels have ended: kernel boundaries lie between)
        const int m = a.meta[0];
        const int bad = m > 0 ? JPEG_DEC_NO_BAD - m : JPEG_DEC_NO_BAD;
        a.meta[1] = bad < a.first_bad ? bad : a.first_bad;
    }
    if (live) *reinterpret_cast<uint4*>(a.coef + size_t(blk) * 64 + 8 * l) = *reinterpret_cast<const uint4*>(&s_rec[lb][8 * l]);
}

}  // namespace

JpegProgLayout::JpegProgLayout(const JpegDecGeom& g, const JpegProgPlan& plan) {
    const auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
    scans = 0;
    huff = up(plan.dev.size() * sizeof(JpegProgScan));
    qz = up(huff + plan.huff.size() * sizeof(JpegDecHuff));
    items = up(qz + sizeof(plan.qz));
    data = up(items + plan.items.size() * sizeof(JpegProgItem));
    upload_bytes = data + size_t(plan.data_bytes);
    meta = up(upload_bytes);
    raw = meta + 256;
    coef_bytes = size_t(g.mcu_cols) * size_t(g.mcu_rows) * size_t(g.bpm) * 64 * sizeof(int16_t);
    zero_bytes = raw + coef_bytes - meta;
    coef = up(raw + coef_bytes);
    size_t at = up(coef + coef_bytes);
    for (int c = 0; c < 3; ++c) {
        plane[c] = at;
        if (c < g.comps) at = up(at + size_t(g.plane_pitch[c]) * size_t(g.plane_rows[c]));
    }
    bytes = at;
}

void jpeg_prog_stage(const JpegProgPlan& plan, const JpegProgLayout& lay, const uint8_t* data, uint8_t* stage) {
    std::memset(stage, 0, lay.data);
    std::memcpy(stage + lay.scans, plan.dev.data(), plan.dev.size() * sizeof(JpegProgScan));
    std::memcpy(stage + lay.huff, plan.huff.data(), plan.huff.size() * sizeof(JpegDecHuff));
    std::memcpy(stage + lay.qz, plan.qz, sizeof(plan.qz));
    std::memcpy(stage + lay.items, plan.items.data(), plan.items.size() * sizeof(JpegProgItem));
    if (plan.data_bytes > 0) std::memcpy(stage + lay.data, data, size_t(plan.data_bytes));
}

void launch_jpeg_decode_progressive(const JpegDecArgs& a, const JpegProgPlan& plan, const JpegProgLayout& lay, void* d_scratch, int levels,
                                    hipStream_t stream, int64_t* scan_launches) {
    const JpegDecGeom& g = a.g;
    char* const s = static_cast<char*>(d_scratch);
    WHENET_REQUIRE(d_scratch != nullptr && !plan.baseline && !plan.dev.empty() && plan.huff.size() == 3 * plan.dev.size() &&
                       plan.items.size() % JPEG_PROG_LANES == 0 && plan.data_bytes >= 0 && plan.data_bytes <= JPEG_DEC_MAX_BYTES,
                   WHENET_EINVAL, "jpeg_decode_progressive: not the plan of a progressive stream");
    WHENET_REQUIRE(lay.coef_bytes == size_t(g.mcu_cols) * size_t(g.mcu_rows) * size_t(g.bpm) * 128 && a.coef == reinterpret_cast<int16_t*>(s + lay.coef) &&
                       a.meta == reinterpret_cast<int32_t*>(s + lay.meta),
                   WHENET_EINVAL, "jpeg_decode_progressive: the work buffers are not those of the stream's geometry");
    // what a lane may index: every item inside its scan and the data, every scan's units inside the frame's records
    for (const JpegProgScan& sc : plan.dev) {
        const long long frame_units = sc.ns > 1 || g.comps == 1 ? (long long)(g.mcu_cols) * g.mcu_rows : -1;
        WHENET_REQUIRE(sc.units >= 1 && sc.ri >= 1 && sc.intervals == (sc.units + sc.ri - 1) / sc.ri && sc.ss >= 0 && sc.ss <= sc.se && sc.se <= 63 &&
                           sc.al >= 0 && sc.al <= 13 && sc.ns >= 1 && sc.ns <= g.comps && sc.bw >= 1 && sc.units == sc.bw * sc.bh &&
                           (frame_units < 0 ? (sc.comp[0] >= 0 && sc.comp[0] < 3 && sc.bw <= g.mcu_cols * (sc.comp[0] == 0 ? g.hs : 1) &&
                                               sc.bh <= g.mcu_rows * (sc.comp[0] == 0 ? g.vs : 1))
                                            : sc.units == frame_units) &&
                           sc.list_off >= 0 && sc.items >= 1 && sc.items <= sc.intervals && sc.list_cnt >= sc.items && sc.list_off % JPEG_PROG_LANES == 0 && sc.list_cnt % JPEG_PROG_LANES == 0 &&
                           size_t(sc.list_off) + size_t(sc.list_cnt) <= plan.items.size(),
                       WHENET_EINVAL, "jpeg_decode_progressive: a scan record outside the frame");
    }
    JpegProgArgs p{};
    p.g = g;
    p.scans = reinterpret_cast<const JpegProgScan*>(s + lay.scans), p.huff = reinterpret_cast<const JpegDecHuff*>(s + lay.huff);
    p.qz = reinterpret_cast<const int16_t*>(s + lay.qz), p.items = reinterpret_cast<const JpegProgItem*>(s + lay.items);
    p.data = reinterpret_cast<const uint8_t*>(s + lay.data), p.nbytes = int(plan.data_bytes);
    p.raw = reinterpret_cast<int16_t*>(s + lay.raw), p.coef = a.coef, p.meta = a.meta, p.first_bad = plan.first_bad;
    WHENET_HIP_CHECK(hipMemsetAsync(s + lay.meta, 0, lay.zero_bytes, stream));      // meta | raw
    const auto launch = [&](int off, int cnt) {
        if (cnt <= 0) return;
        hipLaunchKernelGGL(whenet_jpeg_prog_scan_kernel, dim3(unsigned(cnt / JPEG_PROG_LANES)), dim3(SCAN_THREADS), 0, stream, p,
                           off / JPEG_PROG_LANES);
        WHENET_HIP_CHECK(hipGetLastError());
        if (scan_launches != nullptr) ++*scan_launches;
    };
    if (levels != 0) {
        for (int l = 0; l < plan.levels; ++l) launch(plan.level_off[size_t(l)], plan.level_cnt[size_t(l)]);
    } else {
        for (const JpegProgScan& sc : plan.dev) launch(sc.list_off, sc.list_cnt);
    }
    const long long nblocks = (long long)(g.mcu_cols) * g.mcu_rows * g.bpm;
    hipLaunchKernelGGL(whenet_jpeg_prog_finish_kernel, dim3(unsigned((nblocks + FIN_BLOCKS - 1) / FIN_BLOCKS)), dim3(FIN_THREADS), 0, stream, p);
    WHENET_HIP_CHECK(hipGetLastError());
    launch_jpeg_decode_tail(a, stream);
}

}  // namespace whenet
