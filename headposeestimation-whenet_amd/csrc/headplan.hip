// From the detector's selected boxes to the crop plans of their heads, on the device: what the host does between
// `detect` and `heads` of a frame (engine_post.cpp: the class-by-class concatenation of yolo_eval_maps, frame_box_rect,
// check_rects, build_crop_plan), so that a frame's detections never have to leave the device before its heads are cropped.
//
// Reference: demo_video.py:13-21 (`process_detection`: bbox margins in float32, order dependent, int() truncation, slice
// clipping) and OpenCV's INTER_LINEAR coefficient tables (modules/imgproc/src/resize.cpp), exactly as frame.hip's host code
// restates them.  The results are bit for bit the host's:
//   * every float32 / float64 operation is rounded on its own -- contraction is switched off in this file's arithmetic (the
//     host build has no FMA; `float((d + 0.5) * scale - 0.5)` as one FMA rounds differently for one (source size, entry) pair of
//     sizes 1..4096: size 32, entry 3 is 0.0 unfused and -2.8e-17 fused, which on the vertical axis turns (yofs, b0, b1) =
//     (0, 2048, 0) into (-1, 0, 2048) -- tests/test_frame_async_gpu.py checks every size 1..2048 and names that entry);
//   * float -> short is round half to even (lrintf on the host, rintf here);
//   * int(float) of a value no int can hold is INT_MIN, as the host's conversion instruction returns it.
//
// Mapping (gfx950): one workgroup per output row (detection slot), 256 lanes.  Every lane finds the row's source box from
// the per-class counts (at most 64 classes, uniform loads); lane 0 writes the row's box / score / class / window / valid
// flag; lanes 0..223 each write one entry of the six 224-entry tables (xofs | a0 | a1 | yofs | b0 | b1); the first column
// that reads a single sample (xmax) is an LDS atomic minimum.  A row beyond the detection count, or one whose window is
// empty or leaves the frame, gets valid = 0 and a plan of zeros: the crop kernel skips it.  The frames of a clip (of one size, or
// each of its own: the mixed kernel) are the grid's second dimension; whenet_head_compact_kernel then numbers the clip's live heads so that the forward runs
// over them alone.
#include <climits>

#include "kernels.h"

namespace whenet {

namespace {

constexpr int OUT = IMG;                    // 224
constexpr int COEF_SCALE = 1 << 11;         // INTER_RESIZE_COEF_SCALE

__device__ __forceinline__ int trunc_to_int(float v) {
    return (v >= -2147483648.0f && v < 2147483648.0f) ? int(v) : INT_MIN;
}

// frame_box_rect (frame.hip), operation for operation
__device__ void box_rect(int frame_h, int frame_w, float y_min, float x_min, float y_max, float x_max, int32_t rect[4]) {
#pragma clang fp contract(off)
    const float fh = float(frame_h), fw = float(frame_w);
    {
        const float v = y_min - fabsf(y_min - y_max) / 10.0f;
        y_min = (v > 0.f) ? v : 0.f;
    }
    {
        const float v = y_max + fabsf(y_min - y_max) / 10.0f;
        y_max = (v < fh) ? v : fh;
    }
    {
        const float v = x_min - fabsf(x_min - x_max) / 5.0f;
        x_min = (v > 0.f) ? v : 0.f;
    }
    {
        const float v = x_max + fabsf(x_min - x_max) / 5.0f;
        x_max = (v < fw) ? v : fw;
    }
    if (!(x_max < fw)) x_max = fw;
    int y0 = trunc_to_int(y_min), x0 = trunc_to_int(x_min), y1 = trunc_to_int(y_max), x1 = trunc_to_int(x_max);
    if (y1 > frame_h) y1 = frame_h;
    if (x1 > frame_w) x1 = frame_w;
    rect[0] = y0, rect[1] = x0, rect[2] = y1, rect[3] = x1;
}

// saturate_cast<short>(float): round half to even + saturation
__device__ __forceinline__ int32_t to_short(float v) {
    int r = int(rintf(v));
    r = r < -32768 ? -32768 : (r > 32767 ? 32767 : r);
    return r;
}

// entry d of axis_tables (frame.hip); returns whether the column reads a single sample (s + 1 >= src, horizontal only)
__device__ __forceinline__ bool axis_entry(int src, bool horizontal, int d, int32_t* ofs, int32_t* c0, int32_t* c1) {
#pragma clang fp contract(off)
    const double inv_scale = double(OUT) / double(src);
    const double scale = 1.0 / inv_scale;
    const double pos = (double(d) + 0.5) * scale;
    float f = float(pos - 0.5);
    int s = int(floorf(f));
    f -= float(s);
    bool single = false;
    if (horizontal) {
        if (s < 0) { f = 0.f; s = 0; }
        if (s + 1 >= src) {
            single = true;
            if (s >= src - 1) { f = 0.f; s = src - 1; }
        }
    }
    ofs[d] = s;
    const float w0 = 1.f - f;
    c0[d] = to_short(w0 * float(COEF_SCALE));
    c1[d] = to_short(f * float(COEF_SCALE));
    return single;
}

// one detection slot of frame blockIdx.y, whose size is frame_h x frame_w (s_xmax: one LDS word of the workgroup)
__device__ __forceinline__ void head_plan_slot(const HeadPlanArgs& a, const int frame_h, const int frame_w, int& s_xmax) {
    const int slot = blockIdx.x, tid = threadIdx.x;         // detection slot of its frame
    const size_t f = blockIdx.y;                            // frame of a clip: inputs [F][C]..., outputs [F][K]..., count [F]
    const size_t row = f * (size_t(a.num_classes) * a.max_boxes) + slot;
    const int* in_count = a.in_count + f * a.num_classes;
    // class-by-class concatenation (yolo_v3/model.py:227-229): row -> (class, position in the class)
    int cls = -1, pos = 0, total = 0;
    for (int c = 0; c < a.num_classes; ++c) {
        int n = in_count[c];
        n = n < 0 ? 0 : (n > a.max_boxes ? a.max_boxes : n);
        if (cls < 0 && slot < total + n) cls = c, pos = slot - total;
        total += n;
    }
    if (tid == 0) s_xmax = OUT;
    __syncthreads();

    int32_t rect[4] = {0, 0, 0, 0};
    bool ok = false;
    if (cls >= 0) {
        const size_t src = (f * a.num_classes + size_t(cls)) * a.max_boxes + pos;
        const float* b = a.in_boxes + src * 4;
        const float b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
        box_rect(frame_h, frame_w, b0, b1, b2, b3, rect);
        ok = rect[0] >= 0 && rect[1] >= 0 && rect[2] <= frame_h && rect[3] <= frame_w && rect[0] < rect[2] && rect[1] < rect[3];
        if (tid == 0) {
            float* ob = a.boxes + row * 4;
            ob[0] = b0, ob[1] = b1, ob[2] = b2, ob[3] = b3;
            a.scores[row] = a.in_scores ? a.in_scores[src] : 0.0f;
            a.classes[row] = cls;
        }
    } else if (tid == 0) {
        float* ob = a.boxes + row * 4;
        ob[0] = ob[1] = ob[2] = ob[3] = 0.0f;
        a.scores[row] = 0.0f;
        a.classes[row] = -1;
    }
    if (tid == 0) {
        int32_t* orc = a.rects + row * 4;
        orc[0] = rect[0], orc[1] = rect[1], orc[2] = rect[2], orc[3] = rect[3];
        a.valid[row] = ok ? 1 : 0;
        if (slot == 0) a.count[f] = total;
    }
    if (a.plans == nullptr) return;
    int32_t* P = a.plans + row * CROP_PLAN_INTS;
    if (!ok) {
        for (int i = tid; i < CROP_PLAN_INTS; i += 256) P[i] = 0;
        return;
    }
    const int ch = rect[2] - rect[0], cw = rect[3] - rect[1];
    int32_t* T = P + 8;
    if (tid < OUT) {
        if (axis_entry(cw, true, tid, T, T + OUT, T + 2 * OUT)) atomicMin(&s_xmax, tid);
        (void)axis_entry(ch, false, tid, T + 3 * OUT, T + 4 * OUT, T + 5 * OUT);
    }
    __syncthreads();
    if (tid == 0) {
        P[0] = rect[0], P[1] = rect[1], P[2] = ch, P[3] = cw;
        P[4] = (ch == 2 * OUT && cw == 2 * OUT) ? 1 : 0;
        P[5] = s_xmax;
        P[6] = 0, P[7] = 0;
    }
}

__global__ __launch_bounds__(256) void whenet_head_plan_kernel(HeadPlanArgs a) {
    __shared__ int s_xmax;
    head_plan_slot(a, a.frame_h, a.frame_w, s_xmax);
}

// the frames of a mixed clip: frame blockIdx.y has its own size
__global__ __launch_bounds__(256) void whenet_head_plan_mixed_kernel(HeadPlanArgs a, HeadPlanSizes m) {
    __shared__ int s_xmax;
    head_plan_slot(a, m.frame_h[blockIdx.y], m.frame_w[blockIdx.y], s_xmax);
}

// Compaction of a clip's heads (kernels.h): lane s owns slot s.  A wave's ballot numbers its live slots, the 16 wave totals
// go through LDS, every lane adds the totals of the waves before its own: an exclusive scan in slot order, the same on every
// run.  Rows from rows_used on get slot -1; no two lanes write the same word.
__global__ __launch_bounds__(HEAD_COMPACT_MAX_SLOTS) void whenet_head_compact_kernel(const int32_t* __restrict__ valid,
                                                                                     const int32_t* __restrict__ count, int frames,
                                                                                     int K, int max_heads, int32_t* __restrict__ row,
                                                                                     int32_t* __restrict__ slot_of_row,
                                                                                     int32_t* __restrict__ rows_used,
                                                                                     int32_t* __restrict__ overflow) {
    __shared__ int s_wave[HEAD_COMPACT_MAX_SLOTS / 64];
    const int s = threadIdx.x, slots = frames * K;
    bool live = false;
    if (s < slots) {
        const int f = s / K, i = s - f * K;
        int n = count[f];
        n = n < 0 ? 0 : (n > K ? K : n);
        live = i < n && valid[s] != 0;
    }
    const unsigned long long ballot = __ballot(live);
    const int lane = s & 63, wave = s >> 6;
    const int before = __popcll(ballot & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wave] = __popcll(ballot);
    __syncthreads();
    int base = 0, total = 0;
    for (int w = 0; w < HEAD_COMPACT_MAX_SLOTS / 64; ++w) {
        const int n = s_wave[w];
        if (w < wave) base += n;
        total += n;
    }
    const int used = total < max_heads ? total : max_heads;
    if (s < slots) {
        const int r = base + before;
        const bool placed = live && r < max_heads;
        row[s] = placed ? r : -1;
        if (placed) slot_of_row[r] = s;
    }
    for (int r = used + s; r < max_heads; r += HEAD_COMPACT_MAX_SLOTS) slot_of_row[r] = -1;
    if (s == 0) {
        *rows_used = used;
        *overflow = total - used;
    }
}

}  // namespace

void launch_head_plan(const HeadPlanArgs& a, hipStream_t stream, const HeadPlanSizes* mixed) {
    WHENET_REQUIRE(a.num_classes >= 1 && a.max_boxes >= 1 && a.frames >= 0 && a.frames <= 65535, WHENET_EINVAL, "head_plan: bad sizes");
    const dim3 grid(unsigned(a.num_classes) * unsigned(a.max_boxes), a.frames > 1 ? unsigned(a.frames) : 1u);
    if (mixed) {
        WHENET_REQUIRE(grid.y <= unsigned(MIXED_MAX_FRAMES), WHENET_EINVAL, "head_plan: too many frames of different sizes");
        for (unsigned f = 0; f < grid.y; ++f)
            WHENET_REQUIRE(mixed->frame_h[f] > 0 && mixed->frame_w[f] > 0, WHENET_EINVAL, "head_plan: bad sizes");
        hipLaunchKernelGGL(whenet_head_plan_mixed_kernel, grid, dim3(256), 0, stream, a, *mixed);
    } else {
        WHENET_REQUIRE(a.frame_h > 0 && a.frame_w > 0, WHENET_EINVAL, "head_plan: bad sizes");
        hipLaunchKernelGGL(whenet_head_plan_kernel, grid, dim3(256), 0, stream, a);
    }
    WHENET_HIP_CHECK(hipGetLastError());
}

void launch_head_compact(const int32_t* d_valid, const int32_t* d_count, int frames, int slots_per_frame, int max_heads, int32_t* d_row,
                         int32_t* d_slot_of_row, int32_t* d_rows_used, int32_t* d_overflow, hipStream_t stream) {
    WHENET_REQUIRE(frames >= 1 && slots_per_frame >= 1 && size_t(frames) * size_t(slots_per_frame) <= size_t(HEAD_COMPACT_MAX_SLOTS) &&
                       max_heads >= 1,
                   WHENET_EINVAL, "head_compact: frames x slots must be 1.." + std::to_string(HEAD_COMPACT_MAX_SLOTS) + " and max_heads >= 1");
    hipLaunchKernelGGL(whenet_head_compact_kernel, dim3(1), dim3(HEAD_COMPACT_MAX_SLOTS), 0, stream, d_valid, d_count, frames,
                       slots_per_frame, max_heads, d_row, d_slot_of_row, d_rows_used, d_overflow);
    WHENET_HIP_CHECK(hipGetLastError());
}

}  // namespace whenet
