// The segmented form of the JPEG decoder's entropy stage on the device: every restart interval -- the single interval of a stream
// without DRI included -- decoded by many lanes, a lane per segment of seg_bytes of the entropy data.  The method (the
// self-synchronisation of Huffman streams) and its invariants are in include/whenet_hip.h (JPEG DECODER, ENTROPY FORMS); the
// arithmetic -- sync states, the walk, the count with its saturating DC maps, the write -- is jpeg_dec_seg_host.h's, the same
// functions the host emulation runs.  Integers only.  The marker scan in front and the inverse DCT behind are jpeg_dec.hip's.
//
// Reference: demo.py (`cv2.imread` of Sample/*.jpeg: streams without restart markers) and demo_video.py:49-53 (`cap.read()`).
//
// Every grid is sized from seg_cap = ceil(nbytes / seg_bytes) + intervals, the host's bound of the segment count; the device's own
// count is first_seg[intervals] and surplus lanes exit.  Every loop has a bound: a walk ends with the bits, the sync loop after
// WHENET_JPEG_SEG_WINDOW rounds, the stitch at the interval's last segment.
//   whenet_jpeg_dec_segtab_kernel   one workgroup: the segment count of every decoded interval (i <= meta[0]), scanned -> first_seg
//   whenet_jpeg_dec_sync_kernel     one workgroup per window, L decoding lanes per wave (a wave's lanes diverge in the Huffman walk),
//                                   the decode tables and the window's exit states in LDS; stores behind a barrier (Jacobi order)
//   whenet_jpeg_dec_stitch_kernel   one lane per interval, over the window boundaries inside it
//   whenet_jpeg_dec_count_kernel    one lane per segment: its blocks and its three DC maps
//   whenet_jpeg_dec_segscan_kernel  one workgroup per interval: an exclusive scan of (blocks, maps) over its segments in steps of 256
//                                   with a carry -> every segment's first block and entry predictors
//   whenet_jpeg_dec_write_kernel    one lane per segment: its blocks through an LDS stage into their records; damage lowers meta[1]
#include <algorithm>

#include "kernels.h"
#include "jpeg_dec_seg_host.h"

namespace whenet {

namespace {

constexpr int WINDOW = WHENET_JPEG_SEG_WINDOW;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int DEFAULT_LANES = 32;      // decoding lanes per wave (docs/experiments.md section 32)

static_assert(sizeof(JpegDecTables) % 4 == 0, "the tables are copied to LDS by dwords");
static_assert(WINDOW >= 64 && WINDOW <= JPEG_SEG_MAX_WINDOW && WINDOW % 64 == 0, "a window is whole waves of one workgroup");

__device__ inline void load_tables(JpegDecTables& s_t, const JpegDecTables* tables) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(tables);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&s_t);
    for (int i = int(threadIdx.x); i < int(sizeof(JpegDecTables) / 4); i += int(blockDim.x)) dst[i] = src[i];
    __syncthreads();
}

// the intervals the form decodes: those up to the first one the markers make bad
__device__ inline int decoded_intervals(const JpegDecArgs& a) { return min(a.meta[0], a.g.intervals - 1) + 1; }

// ---- the bodies (as in jpeg_dec.hip): one stream's record, bx = the workgroup's index within that stream's share of the grid ----
__device__ __forceinline__ void segtab_body(const JpegDecArgs& a) {
    __shared__ int s_wave[WAVES];
    const int tid = int(threadIdx.x), lane = tid & 63, wave = tid >> 6, N = a.g.intervals, nd = decoded_intervals(a);
    long long carry = 0;
    for (int base = 0; base < N; base += THREADS) {
        const int i = base + tid;
        const int v = i < nd ? jpeg_seg_count(a.start[i], jpeg_seg_interval_end(a.start, N, i, a.nbytes), a.seg_bytes) : 0;
        int inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(inc, d, 64);
            if (lane >= d) inc += t;
        }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const int t = s_wave[w];
            before += w < wave ? t : 0;
            total += t;
        }
        __syncthreads();
        if (i < N) a.first_seg[i] = int(min(carry + before + inc - v, (long long)(a.seg_cap)));      // (<= seg_cap by the host's bound)
        carry += total;
    }
    if (tid == 0) {
        const long long S = min(carry, (long long)(a.seg_cap));
        a.first_seg[N] = int(S);
        a.seg_stats[0] = nd, a.seg_stats[1] = S, a.seg_stats[2] = (S + WINDOW - 1) / WINDOW, a.seg_stats[6] = a.seg_bytes, a.seg_stats[7] = 1;
    }
}

__device__ inline void stat_max(long long* p, long long v) { atomicMax(reinterpret_cast<unsigned long long*>(p), (unsigned long long)(v)); }

// L decoding lanes per wave: the workgroup has WINDOW / L waves
template <int L>
__device__ __forceinline__ void sync_body(const JpegDecArgs& a, int bx) {
    __shared__ JpegDecTables s_t;
    __shared__ uint64_t s_exit[WINDOW];
    const int tid = int(threadIdx.x), lane = tid & 63, j = (tid >> 6) * L + lane;
    const int S = a.first_seg[a.g.intervals], base = bx * WINDOW;
    if (base >= S) return;      // (the whole workgroup)
    load_tables(s_t, a.tables);
    const int n = min(WINDOW, S - base);
    const bool active = lane < L && j < n;
    JpegSeg sg{};
    uint64_t run = JPEG_SEG_DEAD;
    long long bytes = 0;
    if (active) {
        sg = jpeg_seg_at(a.start, a.first_seg, decoded_intervals(a), a.seg_bytes, base + j);
        run = jpeg_seg_walk(a.data, a.nbytes, s_t, a.g, jpeg_seg_entry_guess(a.data, sg), sg.end, bytes);
        s_exit[j] = run;
    }
    bool done = !active || run == JPEG_SEG_DEAD;      // (a chain that died stores DEAD where it died and ends)
    int rounds = 0;
    for (int r = 1; r <= WINDOW; ++r) {
        bool act = false;
        if (!done) {
            if (j + r >= n || sg.q + r >= sg.nq) done = true;      // the window or the interval ends
            else act = true;
        }
        if (!__syncthreads_or(act)) break;      // (a barrier as well: the stores of the round before are seen)
        uint64_t y = 0;
        bool wrote = false;
        if (act) {
            y = jpeg_seg_walk(a.data, a.nbytes, s_t, a.g, run, jpeg_seg_end_of(sg, sg.q + r, a.seg_bytes), bytes);
            if (y == s_exit[j + r]) done = true;
            else run = y, wrote = true, done = y == JPEG_SEG_DEAD;
        }
        __syncthreads();
        if (wrote) s_exit[j + r] = y;
        rounds = r;
    }
    __syncthreads();
    if (active) {
        a.seg_exit[base + j] = s_exit[j];
        stat_max(&a.seg_stats[5], bytes);
    }
    if (tid == 0) stat_max(&a.seg_stats[3], rounds);
}

__device__ __forceinline__ void stitch_body(const JpegDecArgs& a, int bx) {
    __shared__ JpegDecTables s_t;
    load_tables(s_t, a.tables);
    const long long i = (long long)(bx) * 64 + threadIdx.x;
    if (i >= decoded_intervals(a)) return;
    const int s0 = a.first_seg[i], s1 = a.first_seg[i + 1];
    long long walked = 0, bytes = 0;
    for (long long wb = ((long long)(s0) / WINDOW + 1) * WINDOW; wb < s1; wb += WINDOW) {
        uint64_t state = a.seg_exit[wb - 1];
        for (int s = int(wb); s < s1 && state != JPEG_SEG_DEAD; ++s) {
            const JpegSeg sg = jpeg_seg_in(a.start, a.first_seg, int(i), a.seg_bytes, s);
            const uint64_t y = jpeg_seg_walk(a.data, a.nbytes, s_t, a.g, state, sg.end, bytes);
            ++walked;
            if (y == a.seg_exit[s]) break;
            a.seg_exit[s] = state = y;
        }
    }
    if (walked > 0) atomicAdd(reinterpret_cast<unsigned long long*>(&a.seg_stats[4]), (unsigned long long)(walked));
}

// the segment of a lane of the count and write kernels (L decoding lanes per wave), or -1
template <int L>
__device__ inline int lane_segment(const JpegDecArgs& a, int bx) {
    const int tid = int(threadIdx.x), lane = tid & 63;
    const long long s = (long long)(bx) * (WAVES * L) + (tid >> 6) * L + lane;
    return lane < L && s < a.first_seg[a.g.intervals] ? int(s) : -1;
}
__device__ inline uint64_t entry_state(const JpegDecArgs& a, const JpegSeg& sg, int s) {
    return sg.q == 0 ? jpeg_seg_entry_guess(a.data, sg) : a.seg_exit[s - 1];
}

template <int L>
__device__ __forceinline__ void count_body(const JpegDecArgs& a, int bx) {
    __shared__ JpegDecTables s_t;
    if ((long long)(bx) * (WAVES * L) >= a.first_seg[a.g.intervals]) return;      // (the whole workgroup)
    load_tables(s_t, a.tables);
    const int s = lane_segment<L>(a, bx);
    if (s < 0) return;
    const JpegSeg sg = jpeg_seg_at(a.start, a.first_seg, decoded_intervals(a), a.seg_bytes, s);
    JpegSegCount c = jpeg_seg_count_blocks(a.data, a.nbytes, s_t, a.g, entry_state(a, sg, s), sg.end);
    c.dead = a.seg_exit[s] == JPEG_SEG_DEAD;
    a.seg_count[s] = c;
}

// a, then b: blocks add (saturating: an associative sum whatever a damaged stream counts), the maps compose
__device__ inline JpegSegCount count_then(const JpegSegCount& x, const JpegSegCount& y) {
    JpegSegCount r;
    r.blocks = int(min((long long)(x.blocks) + y.blocks, 0x7FFFFFFFll));
    r.dead = x.dead | y.dead;
#pragma unroll
    for (int c = 0; c < 3; ++c) r.map[c] = jpeg_seg_map_then(x.map[c], y.map[c]);
    return r;
}

__device__ inline JpegSegCount count_none() {
    JpegSegCount r;
    r.blocks = 0, r.dead = 0;
    r.map[0] = r.map[1] = r.map[2] = jpeg_seg_map_identity();
    return r;
}

__device__ __forceinline__ void segscan_body(const JpegDecArgs& a, int bx) {
    __shared__ JpegSegCount s_e[2][THREADS];
    __shared__ JpegSegCount s_carry;      // what the steps before this one add up to
    const int i = bx, tid = int(threadIdx.x);
    if (i >= decoded_intervals(a)) return;      // (the whole workgroup)
    const int s0 = a.first_seg[i], s1 = a.first_seg[i + 1];
    if (tid == 0) s_carry = count_none();
    for (int base = s0; base < s1; base += THREADS) {
        const int s = base + tid;
        if (s < s1) s_e[0][tid] = a.seg_count[s];
        else s_e[0][tid] = count_none();
        __syncthreads();
        int cur = 0;
#pragma unroll
        for (int d = 1; d < THREADS; d <<= 1) {      // inclusive: element t becomes e[0] then .. then e[t]
            if (tid >= d) s_e[cur ^ 1][tid] = count_then(s_e[cur][tid - d], s_e[cur][tid]);
            else s_e[cur ^ 1][tid] = s_e[cur][tid];
            __syncthreads();
            cur ^= 1;
        }
        if (s < s1) {
            const JpegSegCount before = tid > 0 ? count_then(s_carry, s_e[cur][tid - 1]) : count_then(s_carry, count_none());
            int4 o;
            o.x = before.dead ? 0x7FFFFFFF : before.blocks;      // behind a DEAD exit state: no block is the segment's
            o.y = jpeg_seg_map_apply(before.map[0], 0), o.z = jpeg_seg_map_apply(before.map[1], 0), o.w = jpeg_seg_map_apply(before.map[2], 0);
            *reinterpret_cast<int4*>(a.seg_blk + size_t(s) * 4) = o;
        }
        __syncthreads();
        if (tid == 0) s_carry = count_then(s_carry, s_e[cur][THREADS - 1]);
        __syncthreads();
    }
}

template <int L>
__device__ __forceinline__ void write_body(const JpegDecArgs& a, int bx) {
    __shared__ JpegDecTables s_t;
    __shared__ __attribute__((aligned(16))) int16_t s_block[WAVES * L][64 + 8];      // a lane's block in hand (144-byte rows)
    if ((long long)(bx) * (WAVES * L) >= a.first_seg[a.g.intervals]) return;      // (the whole workgroup)
    load_tables(s_t, a.tables);
    const int s = lane_segment<L>(a, bx);
    if (s < 0) return;
    const JpegSeg sg = jpeg_seg_at(a.start, a.first_seg, decoded_intervals(a), a.seg_bytes, s);
    const int4 bp = *reinterpret_cast<const int4*>(a.seg_blk + size_t(s) * 4);
    const int pred[3] = {bp.y, bp.z, bp.w};
    int16_t* const rec0 = a.coef + size_t(sg.interval) * size_t(a.g.ri) * size_t(a.g.bpm) * 64;
    const int slot = (int(threadIdx.x) >> 6) * L + (int(threadIdx.x) & 63);
    if (!jpeg_seg_write(a.data, a.nbytes, s_t, a.g, entry_state(a, sg, s), sg.end, bp.x, pred, jpeg_seg_interval_blocks(a.g, sg.interval), rec0,
                        s_block[slot]))
        atomicMin(&a.meta[1], sg.interval);
}

// ---- the single-stream kernels: the record by value, the grid that stream's ----
__global__ __launch_bounds__(THREADS) void whenet_jpeg_dec_segtab_kernel(JpegDecArgs a) { segtab_body(a); }
template <int L>
__global__ __launch_bounds__(WINDOW * 64 / L) void whenet_jpeg_dec_sync_kernel(JpegDecArgs a) { sync_body<L>(a, int(blockIdx.x)); }
__global__ __launch_bounds__(64) void whenet_jpeg_dec_stitch_kernel(JpegDecArgs a) { stitch_body(a, int(blockIdx.x)); }
template <int L>
__global__ __launch_bounds__(THREADS) void whenet_jpeg_dec_count_kernel(JpegDecArgs a) { count_body<L>(a, int(blockIdx.x)); }
__global__ __launch_bounds__(THREADS) void whenet_jpeg_dec_segscan_kernel(JpegDecArgs a) { segscan_body(a, int(blockIdx.x)); }
template <int L>
__global__ __launch_bounds__(THREADS) void whenet_jpeg_dec_write_kernel(JpegDecArgs a) { write_body<L>(a, int(blockIdx.x)); }

// ---- the clip kernels (as in jpeg_dec.hip): the records of up to 16 frames in device memory, the form-1 frames' windows, groups
// and intervals back to back in one grid; a workgroup finds its frame, copies its record and runs the body.  Every frame has its
// own seg_stats, first_seg, seg_exit, seg_count and seg_blk regions and its own seg_cap: nothing is shared between frames.
// Resource report (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), VGPRs of the clip form / of the
// single-stream form, no scratch in either, the same LDS: segtab 26 / 27, sync 45 / 48, stitch 47 / 47, count 84 / 50 (the one
// kernel that grows by more than the lookup: 4 above the 48..80 of the single-stream kernels), segscan 82 / 80, write 53 / 72.
#define WHENET_JPEG_CLIP_KERNEL(prefix, name, threads, call)                                                               \
    prefix __global__ __launch_bounds__(threads) void name(const void* __restrict__ recs, JpegClipGrid grid) {             \
        const int b = int(blockIdx.x);                                                                                     \
        if (b >= grid.total) return;                                                                                       \
        const int f = jpeg_clip_frame_of(grid, b);                                                                         \
        const JpegDecArgs& a = jpeg_clip_record(recs, f);                                                                  \
        const int bx = b - grid.first[f];                                                                                  \
        (void)bx;                                                                                                          \
        call;                                                                                                              \
    }
WHENET_JPEG_CLIP_KERNEL(, whenet_jpeg_dec_clip_segtab_kernel, THREADS, segtab_body(a))
WHENET_JPEG_CLIP_KERNEL(template <int L>, whenet_jpeg_dec_clip_sync_kernel, WINDOW * 64 / L, sync_body<L>(a, bx))
WHENET_JPEG_CLIP_KERNEL(, whenet_jpeg_dec_clip_stitch_kernel, 64, stitch_body(a, bx))
WHENET_JPEG_CLIP_KERNEL(template <int L>, whenet_jpeg_dec_clip_count_kernel, THREADS, count_body<L>(a, bx))
WHENET_JPEG_CLIP_KERNEL(, whenet_jpeg_dec_clip_segscan_kernel, THREADS, segscan_body(a, bx))
WHENET_JPEG_CLIP_KERNEL(template <int L>, whenet_jpeg_dec_clip_write_kernel, THREADS, write_body<L>(a, bx))
#undef WHENET_JPEG_CLIP_KERNEL

template <int L>
void launch_lanes_clip(const JpegDecArgs* h, const void* d_recs, int frames, hipStream_t stream, int64_t& n) {
    JpegClipGrid grid;
    const auto launch = [&](auto kernel, int threads) {
        hipLaunchKernelGGL(kernel, dim3(unsigned(grid.total)), dim3(unsigned(threads)), 0, stream, d_recs, grid);
        WHENET_HIP_CHECK(hipGetLastError());
        ++n;
    };
    const auto windows = [](const JpegDecArgs& a) { return a.form == 1 ? (a.seg_cap + WINDOW - 1) / WINDOW : 0; };
    const auto groups = [](const JpegDecArgs& a) { return a.form == 1 ? (a.seg_cap + WAVES * L - 1) / (WAVES * L) : 0; };
    jpeg_clip_grid(h, frames, windows, grid);
    launch(whenet_jpeg_dec_clip_sync_kernel<L>, WINDOW * 64 / L);
    jpeg_clip_grid(h, frames, [](const JpegDecArgs& a) { return a.form == 1 ? (a.g.intervals + 63) / 64 : 0; }, grid);
    launch(whenet_jpeg_dec_clip_stitch_kernel, 64);
    jpeg_clip_grid(h, frames, groups, grid);
    launch(whenet_jpeg_dec_clip_count_kernel<L>, THREADS);
    jpeg_clip_grid(h, frames, [](const JpegDecArgs& a) { return a.form == 1 ? a.g.intervals : 0; }, grid);
    launch(whenet_jpeg_dec_clip_segscan_kernel, THREADS);
    jpeg_clip_grid(h, frames, groups, grid);
    launch(whenet_jpeg_dec_clip_write_kernel<L>, THREADS);
}

template <int L>
void launch_lanes(const JpegDecArgs& a, hipStream_t stream) {
    const unsigned windows = unsigned((a.seg_cap + WINDOW - 1) / WINDOW), groups = unsigned((a.seg_cap + WAVES * L - 1) / (WAVES * L));
    hipLaunchKernelGGL(whenet_jpeg_dec_sync_kernel<L>, dim3(windows), dim3(WINDOW * 64 / L), 0, stream, a);
    WHENET_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(whenet_jpeg_dec_stitch_kernel, dim3(unsigned((a.g.intervals + 63) / 64)), dim3(64), 0, stream, a);
    WHENET_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(whenet_jpeg_dec_count_kernel<L>, dim3(groups), dim3(THREADS), 0, stream, a);
    WHENET_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(whenet_jpeg_dec_segscan_kernel, dim3(unsigned(a.g.intervals)), dim3(THREADS), 0, stream, a);
    WHENET_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(whenet_jpeg_dec_write_kernel<L>, dim3(groups), dim3(THREADS), 0, stream, a);
    WHENET_HIP_CHECK(hipGetLastError());
}

}  // namespace

void launch_jpeg_decode_segmented(const JpegDecArgs& a, hipStream_t stream) {
    WHENET_REQUIRE(a.form == 1 && jpeg_seg_bytes_ok(a.seg_bytes) && a.seg_cap >= 1 && a.g.intervals >= 1, WHENET_EINVAL,
                   "jpeg_decode: bad arguments of the segmented form");
    const int lanes = a.seg_lanes == 0 ? DEFAULT_LANES : a.seg_lanes;
    WHENET_REQUIRE(lanes == 16 || lanes == 32 || lanes == 64, WHENET_EINVAL, "jpeg_decode: the decoding lanes per wave must be 16, 32 or 64");
    hipLaunchKernelGGL(whenet_jpeg_dec_segtab_kernel, dim3(1), dim3(THREADS), 0, stream, a);
    WHENET_HIP_CHECK(hipGetLastError());
    if (lanes == 16) launch_lanes<16>(a, stream);
    else if (lanes == 32) launch_lanes<32>(a, stream);
    else launch_lanes<64>(a, stream);
}

// the six launches over the form-1 frames of a clip (none: nothing is launched); seg_lanes is the first form-1 frame's, an option of
// the engine and so the same for all
void launch_jpeg_decode_segmented_clip(const JpegDecArgs* h_recs, const void* d_recs, int frames, hipStream_t stream, int64_t* enqueues) {
    WHENET_REQUIRE(h_recs != nullptr && d_recs != nullptr && frames >= 1 && frames <= MIXED_MAX_FRAMES, WHENET_EINVAL,
                   "jpeg_decode_clip: NULL argument, or a frame count outside 1..16");
    int lanes = -1;
    for (int f = 0; f < frames; ++f) {
        const JpegDecArgs& a = h_recs[f];
        if (a.form != 1) continue;
        WHENET_REQUIRE(jpeg_seg_bytes_ok(a.seg_bytes) && a.seg_cap >= 1 && a.g.intervals >= 1, WHENET_EINVAL,
                       "jpeg_decode_clip: bad arguments of the segmented form");
        const int l = a.seg_lanes == 0 ? DEFAULT_LANES : a.seg_lanes;
        WHENET_REQUIRE(l == 16 || l == 32 || l == 64, WHENET_EINVAL, "jpeg_decode: the decoding lanes per wave must be 16, 32 or 64");
        WHENET_REQUIRE(lanes < 0 || lanes == l, WHENET_EINVAL, "jpeg_decode_clip: the frames of a clip share the decoding lanes per wave");
        lanes = l;
    }
    if (lanes < 0) return;
    int64_t n = 0;
    JpegClipGrid grid;
    jpeg_clip_grid(h_recs, frames, [](const JpegDecArgs& a) { return a.form == 1 ? 1 : 0; }, grid);
    hipLaunchKernelGGL(whenet_jpeg_dec_clip_segtab_kernel, dim3(unsigned(grid.total)), dim3(THREADS), 0, stream, d_recs, grid);
    WHENET_HIP_CHECK(hipGetLastError());
    ++n;
    if (lanes == 16) launch_lanes_clip<16>(h_recs, d_recs, frames, stream, n);
    else if (lanes == 32) launch_lanes_clip<32>(h_recs, d_recs, frames, stream, n);
    else launch_lanes_clip<64>(h_recs, d_recs, frames, stream, n);
    if (enqueues != nullptr) *enqueues += n;
}

}  // namespace whenet
