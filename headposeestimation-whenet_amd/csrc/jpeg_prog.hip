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
//   whenet_jpeg_seq_scan_kernel     the scans of a SEQUENTIAL frame that goes through the scan plan (the header's JPEG DECODER, LAYOUTS:
//                                   several scans, scans of two components, Huffman ids 2 / 3): the same item per lane and the same
//                                   16 lanes, the scan's six tables (DC and AC of up to three components) in LDS.  The scans of such
//                                   a frame hold different components, so an item owns whole records: a block is decoded in an LDS
//                                   row and leaves as eight 16-byte stores, as in the baseline entropy kernel.  All scans are level 1:
//                                   ONE launch per frame.  A kernel of its own, so that the progressive scan kernel keeps its 6,452
//                                   bytes of LDS and its registers.  whenet_jpeg_seq_clip_scan_kernel: the clip form, one launch for
//                                   all such frames of a clip.
//   whenet_jpeg_prog_clip_scan_kernel, whenet_jpeg_prog_clip_finish_kernel
//                                   the same bodies for a CLIP of up to 16 streams (jpeg_dec_clip_host.h: jpeg_clip_plan_progressive):
//                                   launch L of the scan kernel covers level L of every progressive frame that has one, the finish
//                                   kernel all progressive frames; a workgroup finds its frame in the per-frame workgroup counts.
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

// ---- the bodies: what a workgroup does for ONE stream, given that stream's record.  The single-stream kernels call them with their
// own argument and blockIdx.x, the clip kernels with the record of the frame the workgroup belongs to (as jpeg_dec.hip's do).
// group: the workgroup's index in the stream's item list (16 items each)
__device__ __forceinline__ void scan_body(const JpegProgArgs& a, long long group) {
    __shared__ JpegDecHuff s_h[3];
    __shared__ JpegProgScan s_sc;
    __shared__ int16_t s_band[JPEG_PROG_LANES][64 + 2];      // an AC refinement's band in hand (132-byte rows)
    const int tid = int(threadIdx.x);
    const long long base = group * JPEG_PROG_LANES;
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

// a sequential frame's scans (jpeg_prog_host.h: jpeg_seq_item); group: as above
__device__ __forceinline__ void seq_scan_body(const JpegProgArgs& a, long long group) {
    __shared__ JpegDecHuff s_h[6];
    __shared__ JpegProgScan s_sc;
    __shared__ __attribute__((aligned(16))) int16_t s_block[JPEG_PROG_LANES][64 + 8];      // a lane's block in hand (144-byte rows)
    const int tid = int(threadIdx.x);
    const long long base = group * JPEG_PROG_LANES;
    const int s = a.items[base].scan;      // (a scan's share begins with a real item: uniform over the workgroup)
    if (s < 0) return;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.scans + s);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&s_sc);
        for (int i = tid; i < int(sizeof(JpegProgScan) / 4); i += SCAN_THREADS) dst[i] = src[i];
        src = reinterpret_cast<const uint32_t*>(a.huff + 6 * size_t(s));      // (six per scan: unused ones are zeroed tables)
        dst = reinterpret_cast<uint32_t*>(s_h);
        for (int i = tid; i < 6 * int(sizeof(JpegDecHuff) / 4); i += SCAN_THREADS) dst[i] = src[i];
    }
    __syncthreads();
    if (tid >= JPEG_PROG_LANES || s_sc.kind != JPEG_PROG_SEQUENTIAL) return;
    const JpegProgItem it = a.items[base + tid];
    if (it.scan != s || it.interval < 0 || it.interval >= s_sc.intervals || it.start < 0 || it.end > a.nbytes || it.start > it.end) return;
    if (!jpeg_seq_item(a.data, it.start, it.end, s_sc, s_h, a.g, it.interval, a.raw, s_block[tid]))
        atomicMax(&a.meta[0], JPEG_DEC_NO_BAD - (s_sc.first_item + it.interval));
}

// bx: the workgroup's index among the stream's (32 blocks each)
__device__ __forceinline__ void finish_body(const JpegProgArgs& a, int bx) {
    __shared__ __attribute__((aligned(16))) int16_t s_rec[FIN_BLOCKS][64 + 8];
    __shared__ int16_t s_q[3][64];
    const int tid = int(threadIdx.x), lb = tid >> 3, l = tid & 7;
    if (tid < 192) s_q[tid >> 6][tid & 63] = a.qz[tid];
    __syncthreads();
    const long long blk = (long long)(bx) * FIN_BLOCKS + lb;
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
    if (bx == 0 && tid == 0) {      // (the scan kernels have ended: kernel boundaries lie between)
        const int m = a.meta[0];
        const int bad = m > 0 ? JPEG_DEC_NO_BAD - m : JPEG_DEC_NO_BAD;
        a.meta[1] = bad < a.first_bad ? bad : a.first_bad;
    }
    if (live) *reinterpret_cast<uint4*>(a.coef + size_t(blk) * 64 + 8 * l) = *reinterpret_cast<const uint4*>(&s_rec[lb][8 * l]);
}

// ---- the single-stream kernels: the record by value, the grid that stream's ----
__global__ __launch_bounds__(SCAN_THREADS) void whenet_jpeg_prog_scan_kernel(JpegProgArgs a, int first_group) {
    scan_body(a, (long long)(first_group) + blockIdx.x);
}
__global__ __launch_bounds__(SCAN_THREADS) void whenet_jpeg_seq_scan_kernel(JpegProgArgs a, int first_group) {
    seq_scan_body(a, (long long)(first_group) + blockIdx.x);
}
__global__ __launch_bounds__(FIN_THREADS) void whenet_jpeg_prog_finish_kernel(JpegProgArgs a) { finish_body(a, int(blockIdx.x)); }

// ---- the clip kernels: the frames' workgroups back to back in one grid (kernels.h, JpegClipGrid).  A workgroup finds its frame, reads
// that frame's progressive record where it lies in the uploaded records (the same address for every lane, read-only for the kernel) and
// runs the body with its index inside the frame's share; a workgroup never straddles two frames, and one behind the grid's total
// exits before it touches memory.  Frames share no record and no item list: inside a frame the lanes store single int16s of their own
// band, as in the single-stream kernel.
// Resource report (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), clip form / single-stream form, no scratch in
// either: scan 90 / 103 VGPRs, 106 / 106 SGPRs, 6452 / 6452 bytes of LDS; finish 23 / 23 VGPRs, 46 / 34 SGPRs, 4992 / 4992 bytes of LDS.
__global__ __launch_bounds__(SCAN_THREADS) void whenet_jpeg_prog_clip_scan_kernel(const void* __restrict__ recs, JpegClipGrid grid,
                                                                                  JpegProgClipLevel level) {
    const int b = int(blockIdx.x);
    if (b >= grid.total) return;
    const int f = jpeg_clip_frame_of(grid, b);
    scan_body(jpeg_clip_prog_record(recs, f), (long long)(level.first_group[f]) + (b - grid.first[f]));
}
__global__ __launch_bounds__(SCAN_THREADS) void whenet_jpeg_seq_clip_scan_kernel(const void* __restrict__ recs, JpegClipGrid grid,
                                                                                 JpegProgClipLevel level) {
    const int b = int(blockIdx.x);
    if (b >= grid.total) return;
    const int f = jpeg_clip_frame_of(grid, b);
    seq_scan_body(jpeg_clip_prog_record(recs, f), (long long)(level.first_group[f]) + (b - grid.first[f]));
}
__global__ __launch_bounds__(FIN_THREADS) void whenet_jpeg_prog_clip_finish_kernel(const void* __restrict__ recs, JpegClipGrid grid) {
    const int b = int(blockIdx.x);
    if (b >= grid.total) return;
    const int f = jpeg_clip_frame_of(grid, b);
    finish_body(jpeg_clip_prog_record(recs, f), b - grid.first[f]);
}

static_assert(sizeof(JpegDecArgs) <= JPEG_CLIP_PROG_RECORD_OFFSET && JPEG_CLIP_PROG_RECORD_OFFSET % 16 == 0 &&
                  JPEG_CLIP_PROG_RECORD_OFFSET + sizeof(JpegProgArgs) <= JPEG_CLIP_RECORD_BYTES,
              "a frame's two records fit the stride");

// what a lane may index: every item inside its scan and the data, every scan's units inside the frame's records
void check_jpeg_prog_plan(const JpegDecGeom& g, const JpegProgPlan& plan) {
    WHENET_REQUIRE(!plan.baseline && !plan.dev.empty() && plan.huff.size() == size_t(plan.huff_per_scan()) * plan.dev.size() &&
                       (!plan.sequential || plan.levels == 1) && plan.items.size() % JPEG_PROG_LANES == 0 &&
                       plan.data_bytes >= 0 && plan.data_bytes <= JPEG_DEC_MAX_BYTES,
                   WHENET_EINVAL, "jpeg_decode_progressive: not the plan of a progressive stream");
    for (const JpegProgScan& sc : plan.dev) {
        const long long frame_units = sc.ns > 1 || g.comps == 1 ? (long long)(g.mcu_cols) * g.mcu_rows : -1;
        // (a sequential frame's scans are all of that kind, a progressive frame's never; the components a scan names are the frame's)
        WHENET_REQUIRE((sc.kind == JPEG_PROG_SEQUENTIAL) == plan.sequential && sc.kind >= JPEG_PROG_DC_FIRST && sc.kind <= JPEG_PROG_SEQUENTIAL &&
                           sc.ns >= 1 && sc.ns <= g.comps && sc.comp[0] >= 0 && sc.comp[0] < g.comps && (sc.ns < 2 || (sc.comp[1] > sc.comp[0] && sc.comp[1] < g.comps)) &&
                           (sc.ns < 3 || (sc.comp[2] > sc.comp[1] && sc.comp[2] < g.comps)) && (sc.ns == 1 || g.comps == 3),
                       WHENET_EINVAL, "jpeg_decode_progressive: a scan record outside the frame");
        WHENET_REQUIRE(sc.units >= 1 && sc.ri >= 1 && sc.intervals == (sc.units + sc.ri - 1) / sc.ri && sc.ss >= 0 && sc.ss <= sc.se && sc.se <= 63 &&
                           sc.al >= 0 && sc.al <= 13 && sc.ns >= 1 && sc.ns <= g.comps && sc.bw >= 1 && sc.units == sc.bw * sc.bh &&
                           (frame_units < 0 ? (sc.comp[0] >= 0 && sc.comp[0] < 3 && sc.bw <= g.mcu_cols * (sc.comp[0] == 0 ? g.hs : 1) &&
                                               sc.bh <= g.mcu_rows * (sc.comp[0] == 0 ? g.vs : 1))
                                            : sc.units == frame_units) &&
                           sc.list_off >= 0 && sc.items >= 1 && sc.items <= sc.intervals && sc.list_cnt >= sc.items && sc.list_off % JPEG_PROG_LANES == 0 && sc.list_cnt % JPEG_PROG_LANES == 0 &&
                           size_t(sc.list_off) + size_t(sc.list_cnt) <= plan.items.size(),
                       WHENET_EINVAL, "jpeg_decode_progressive: a scan record outside the frame");
    }
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
    WHENET_REQUIRE(d_scratch != nullptr, WHENET_EINVAL, "jpeg_decode_progressive: not the plan of a progressive stream");
    check_jpeg_prog_plan(g, plan);
    WHENET_REQUIRE(lay.coef_bytes == size_t(g.mcu_cols) * size_t(g.mcu_rows) * size_t(g.bpm) * 128 && a.coef == reinterpret_cast<int16_t*>(s + lay.coef) &&
                       a.meta == reinterpret_cast<int32_t*>(s + lay.meta),
                   WHENET_EINVAL, "jpeg_decode_progressive: the work buffers are not those of the stream's geometry");
    JpegProgArgs p{};
    p.g = g;
    p.scans = reinterpret_cast<const JpegProgScan*>(s + lay.scans), p.huff = reinterpret_cast<const JpegDecHuff*>(s + lay.huff);
    p.qz = reinterpret_cast<const int16_t*>(s + lay.qz), p.items = reinterpret_cast<const JpegProgItem*>(s + lay.items);
    p.data = reinterpret_cast<const uint8_t*>(s + lay.data), p.nbytes = int(plan.data_bytes);
    p.raw = reinterpret_cast<int16_t*>(s + lay.raw), p.coef = a.coef, p.meta = a.meta, p.first_bad = plan.first_bad;
    WHENET_HIP_CHECK(hipMemsetAsync(s + lay.meta, 0, lay.zero_bytes, stream));      // meta | raw
    const auto launch = [&](int off, int cnt) {
        if (cnt <= 0) return;
        hipLaunchKernelGGL(plan.sequential ? whenet_jpeg_seq_scan_kernel : whenet_jpeg_prog_scan_kernel, dim3(unsigned(cnt / JPEG_PROG_LANES)), dim3(SCAN_THREADS), 0, stream, p,
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

void launch_jpeg_decode_clip_progressive(const JpegDecArgs* h_recs, const JpegProgArgs* h_prog, const JpegProgPlan* const* plans, const void* d_recs,
                                         int frames, void* d_zero, size_t zero_bytes, hipStream_t stream, int64_t* enqueues, int64_t* scan_launches) {
    WHENET_REQUIRE(h_recs != nullptr && h_prog != nullptr && plans != nullptr && d_recs != nullptr && d_zero != nullptr && frames >= 1 &&
                       frames <= MIXED_MAX_FRAMES,
                   WHENET_EINVAL, "jpeg_decode_clip: NULL argument, or a frame count outside 1..16");
    uint8_t prog[MIXED_MAX_FRAMES] = {};
    int levels = 0;
    bool any_sequential = false;
    for (int f = 0; f < frames; ++f) {
        if (!jpeg_clip_is_progressive(plans[f])) continue;
        const JpegProgPlan& plan = *plans[f];
        const JpegProgArgs& p = h_prog[f];
        const JpegDecGeom& g = h_recs[f].g;
        prog[f] = 1;
        check_jpeg_prog_plan(g, plan);
        const std::string who = "jpeg_decode_clip: frame " + std::to_string(f);
        WHENET_REQUIRE(plan.levels >= 1 && plan.level_off.size() == size_t(plan.levels) && plan.level_cnt.size() == size_t(plan.levels), WHENET_EINVAL,
                       who + ": not the plan of a progressive stream");
        size_t at = 0;      // the levels tile the item list, each a whole number of workgroups
        for (int l = 0; l < plan.levels; ++l) {
            WHENET_REQUIRE(plan.level_off[size_t(l)] >= 0 && size_t(plan.level_off[size_t(l)]) == at && plan.level_cnt[size_t(l)] >= 0 &&
                               plan.level_cnt[size_t(l)] % JPEG_PROG_LANES == 0,
                           WHENET_EINVAL, who + ": a level outside the item list");
            at += size_t(plan.level_cnt[size_t(l)]);
        }
        WHENET_REQUIRE(at == plan.items.size(), WHENET_EINVAL, who + ": a level outside the item list");
        // the record the kernels read: this geometry, the frame's own buffers, raw inside the zeroed bytes
        const size_t coef_bytes = size_t(g.mcu_cols) * size_t(g.mcu_rows) * size_t(g.bpm) * 128;
        const char *z0 = static_cast<const char*>(d_zero), *z1 = z0 + zero_bytes, *raw = reinterpret_cast<const char*>(p.raw);
        WHENET_REQUIRE(std::memcmp(&p.g, &g, sizeof(g)) == 0 && p.scans != nullptr && p.huff != nullptr && p.qz != nullptr && p.items != nullptr &&
                           p.data != nullptr && p.nbytes == int(plan.data_bytes) && p.raw != nullptr && raw >= z0 && raw + coef_bytes <= z1 &&
                           reinterpret_cast<uintptr_t>(p.raw) % 16 == 0 && p.coef == h_recs[f].coef && reinterpret_cast<uintptr_t>(p.coef) % 16 == 0 &&
                           p.meta == h_recs[f].meta && p.first_bad == plan.first_bad,
                       WHENET_EINVAL, who + ": the progressive record is not that of the frame's plan and buffers");
        if (plan.sequential) any_sequential = true;      // (one level, launched once for all such frames below)
        else levels = std::max(levels, plan.levels);
    }
    launch_jpeg_decode_clip_entropy(h_recs, d_recs, frames, d_zero, zero_bytes, stream, enqueues, prog);      // checks, the one memset, the baseline frames
    int64_t n = 0;
    JpegClipGrid grid;
    for (int l = 0; l < levels; ++l) {
        JpegProgClipLevel level{};
        const auto count = [&](const JpegDecArgs& a) {
            const int f = int(&a - h_recs);
            return prog[f] && !plans[f]->sequential && l < plans[f]->levels ? plans[f]->level_cnt[size_t(l)] / JPEG_PROG_LANES : 0;
        };
        for (int f = 0; f < frames; ++f)
            if (count(h_recs[f]) > 0) level.first_group[f] = plans[f]->level_off[size_t(l)] / JPEG_PROG_LANES;
        if (!jpeg_clip_grid(h_recs, frames, count, grid)) continue;
        hipLaunchKernelGGL(whenet_jpeg_prog_clip_scan_kernel, dim3(unsigned(grid.total)), dim3(SCAN_THREADS), 0, stream, d_recs, grid, level);
        WHENET_HIP_CHECK(hipGetLastError());
        ++n;
        if (scan_launches != nullptr) ++*scan_launches;
    }
    if (any_sequential) {      // the sequential frames' scans: level 1 of each, together
        JpegProgClipLevel level{};
        const auto count = [&](const JpegDecArgs& a) {
            const int f = int(&a - h_recs);
            return prog[f] && plans[f]->sequential ? plans[f]->level_cnt[0] / JPEG_PROG_LANES : 0;
        };
        for (int f = 0; f < frames; ++f)
            if (count(h_recs[f]) > 0) level.first_group[f] = plans[f]->level_off[0] / JPEG_PROG_LANES;
        if (jpeg_clip_grid(h_recs, frames, count, grid)) {
            hipLaunchKernelGGL(whenet_jpeg_seq_clip_scan_kernel, dim3(unsigned(grid.total)), dim3(SCAN_THREADS), 0, stream, d_recs, grid, level);
            WHENET_HIP_CHECK(hipGetLastError());
            ++n;
            if (scan_launches != nullptr) ++*scan_launches;
        }
    }
    if (jpeg_clip_grid(h_recs, frames,
                       [&](const JpegDecArgs& a) {
                           return prog[&a - h_recs] ? ((long long)(a.g.mcu_cols) * a.g.mcu_rows * a.g.bpm + FIN_BLOCKS - 1) / FIN_BLOCKS : 0;
                       },
                       grid)) {
        hipLaunchKernelGGL(whenet_jpeg_prog_clip_finish_kernel, dim3(unsigned(grid.total)), dim3(FIN_THREADS), 0, stream, d_recs, grid);
        WHENET_HIP_CHECK(hipGetLastError());
        ++n;
    }
    if (enqueues != nullptr) *enqueues += n;
    launch_jpeg_decode_clip_tail(h_recs, d_recs, frames, stream, enqueues);
}

}  // namespace whenet
