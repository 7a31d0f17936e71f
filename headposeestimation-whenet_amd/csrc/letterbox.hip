// The detector's pre-processing on the GPU: frame -> (BGR->RGB) -> Pillow BICUBIC resize at unchanged aspect
// ratio -> paste centred on a grey (128) canvas -> uint8 canvas and float32 canvas / 255.
//
// Reference: /root/reference/yolo_v3/utils.py:23-34 (`letterbox_image`: scale = min(w/iw, h/ih), nw = int(iw*scale),
// nh = int(ih*scale), image.resize((nw, nh), Image.BICUBIC), paste at ((w-nw)//2, (h-nh)//2)) and
// /root/reference/yolo_v3/yolo_postprocess.py:186-196 (np.array(boxed_image, 'float32'), `image_data /= 255.`).
//
// Pillow's 8-bit resample (src/libImaging/Resample.c) is integer arithmetic on tables computed in double:
// precompute_coeffs (per output pixel a window [xmin, xmin + n) and n cubic weights, a = -0.5, normalised by their
// running sum), normalize_coeffs_8bpc (22 fractional bits, (int)(+-0.5 + k * 2^22)), then a horizontal pass and a
// vertical pass, each (2^21 + sum p * k) >> 22 clipped to 0..255 and stored as 8 bits in between.  The tables are built
// on the HOST with the same double operations in the same order (build_letterbox_plan), so both kernels are pure int32
// arithmetic and the canvas is bit-exact with Pillow's.  (Pillow skips a pass whose size does not change; in this
// arithmetic such a pass is the identity: one weight of exactly 2^22.)  The float canvas is a 256-entry table lookup
// built on the host (float(v) / 255.0f, correctly rounded as numpy's float32 division).
#include <cmath>

#include "kernels.h"

namespace whenet {

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;
constexpr int ROW_LDS_BYTES = LETTERBOX_MAX_FRAME_SIDE * 3 + 32;     // a frame row plus the two partial 16-byte chunks
constexpr int THREADS = 256;

__device__ inline int clip8(int acc) {
    const int v = acc >> PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// The two halves of the horizontal pass, shared by its kernels.
// The row of row_bytes bytes at address lo, staged into `row` as the 16-byte chunks (counted from lo ALIGNED DOWN) that hold it;
// [base, base + buf_bytes) is what may be read.  Returns the row's first byte in `row`.  Barriers inside: every thread calls it.
__device__ __forceinline__ int letterbox_stage_row(uint8_t* row, uintptr_t base, size_t buf_bytes, uintptr_t lo, size_t row_bytes) {
    const uintptr_t hi = lo + row_bytes;
    const uintptr_t first = lo & ~uintptr_t(15);
    const int skew = int(lo - first);
    const int chunks = int((hi - first + 15) >> 4);
    __syncthreads();                                     // (the previous row's readers are done)
    for (int c = threadIdx.x; c < chunks; c += THREADS) {
        const uintptr_t a = first + (uintptr_t(c) << 4);
        if (a >= base && a + 16 <= base + buf_bytes) {   // wholly inside the buffer: one 16-byte load
            *reinterpret_cast<uint4*>(row + (c << 4)) = *reinterpret_cast<const uint4*>(a);
        } else {                                         // the buffer's first / last partial chunk: its own bytes only
            for (int b = 0; b < 16; ++b) {
                const uintptr_t ab = a + b;
                row[(c << 4) + b] = (ab >= base && ab < base + buf_bytes) ? *reinterpret_cast<const uint8_t*>(ab) : uint8_t(0);
            }
        }
    }
    __syncthreads();
    return skew;
}

// the out_bytes output bytes of one staged row
__device__ __forceinline__ void letterbox_h_row(const uint8_t* src, uint8_t* __restrict__ dst, int out_bytes, int swap_rb,
                                                const int32_t* __restrict__ bounds, const int32_t* __restrict__ coeffs, int ksx) {
    for (int ob = threadIdx.x; ob < out_bytes; ob += THREADS) {
        const int ox = ob / 3, c = ob - ox * 3;
        const int cs = swap_rb ? 2 - c : c;
        const int xmin = bounds[2 * ox], n = bounds[2 * ox + 1];
        const int32_t* k = coeffs + size_t(ox) * ksx;
        const uint8_t* s = src + xmin * 3 + cs;
        int acc = 1 << (PRECISION_BITS - 1);
        for (int j = 0; j < n; ++j) acc += int(s[j * 3]) * k[j];
        dst[ob] = uint8_t(clip8(acc));
    }
}

// Horizontal pass: frame [ih][iw][3] -> mid [ih][nw][3].  A workgroup owns whole input rows: the row goes into LDS
// with 16-byte loads of the aligned chunks that cover it (the frame is read once, in whole lines), then thread t
// forms output BYTES t, t + 256, ... of the row (pixel = byte / 3), so the stores of a wave are contiguous and the
// threads of a pixel share its (xmin, n, k[]).
__global__ __launch_bounds__(THREADS) void whenet_letterbox_h_kernel(const uint8_t* __restrict__ frame, LetterboxPlan p,
                                                                     int swap_rb, const int32_t* __restrict__ tab,
                                                                     uint8_t* __restrict__ mid) {
    __shared__ __attribute__((aligned(16))) uint8_t row[ROW_LDS_BYTES];
    const int32_t* __restrict__ bounds = tab + p.off_bx;
    const int32_t* __restrict__ coeffs = tab + p.off_cx;
    const size_t row_bytes = size_t(p.iw) * 3, frame_bytes = size_t(p.ih) * row_bytes;
    const int out_bytes = p.nw * 3;
    const uintptr_t base = reinterpret_cast<uintptr_t>(frame);
    for (int y = blockIdx.x; y < p.ih; y += gridDim.x) {
        const int skew = letterbox_stage_row(row, base, frame_bytes, base + size_t(y) * row_bytes, row_bytes);
        letterbox_h_row(row + skew, mid + size_t(y) * out_bytes, out_bytes, swap_rb, bounds, coeffs, p.ksx);
    }
}

// The same over the rows of a MIXED clip: global row g belongs to the last frame whose row0 is <= g (a scan of at most 16
// values, the same in every lane), and is resampled with that frame's width, bounds and coefficients into its part of mid.
__global__ __launch_bounds__(THREADS) void whenet_letterbox_h_mixed_kernel(const uint8_t* __restrict__ frames, LetterboxMixed clip,
                                                                           int swap_rb, uint8_t* __restrict__ mid) {
    __shared__ __attribute__((aligned(16))) uint8_t row[ROW_LDS_BYTES];
    const uintptr_t base = reinterpret_cast<uintptr_t>(frames);
    for (int g = blockIdx.x; g < clip.total_rows; g += gridDim.x) {
        int f = 0;
        for (int i = 1; i < clip.frames; ++i)
            if (clip.f[i].row0 <= g) f = i;
        const LetterboxMixedFrame& fr = clip.f[f];
        const int y = g - fr.row0;
        const size_t row_bytes = size_t(fr.p.iw) * 3;
        const int out_bytes = fr.p.nw * 3;
        const int skew = letterbox_stage_row(row, base, size_t(clip.total_bytes), base + size_t(fr.frame_off) + size_t(y) * row_bytes, row_bytes);
        letterbox_h_row(row + skew, mid + size_t(fr.mid_off) + size_t(y) * out_bytes, out_bytes, swap_rb, fr.tab + fr.p.off_bx,
                        fr.tab + fr.p.off_cx, fr.p.ksx);
    }
}

// Vertical pass + paste + /255: mid [ih][nw][3] -> canvas [oh][ow][3] (uint8 and / or float32).  One thread per canvas
// byte, adjacent threads on adjacent bytes of a row; it walks the n source rows of its output row.
// one canvas byte of the vertical pass: output row oy, byte ob of the row
__device__ __forceinline__ void letterbox_v_byte(const uint8_t* __restrict__ mid, const LetterboxPlan& p, const int32_t* __restrict__ tab,
                                                 const float* __restrict__ lut, uint8_t* __restrict__ canvas_u8,
                                                 float* __restrict__ image_f32, int oy, int ob) {
    const int row_out = p.ow * 3;
    if (ob >= row_out) return;
    const int mid_row = p.nw * 3;
    const int b = ob - p.x0 * 3, yy = oy - p.y0;
    int v = 128;
    if (yy >= 0 && yy < p.nh && b >= 0 && b < mid_row) {
        const int32_t* bounds = tab + p.off_by;
        const int ymin = bounds[2 * yy], n = bounds[2 * yy + 1];
        const int32_t* k = tab + p.off_cy + size_t(yy) * p.ksy;
        const uint8_t* s = mid + size_t(ymin) * mid_row + b;
        int acc = 1 << (PRECISION_BITS - 1);
        for (int j = 0; j < n; ++j) acc += int(s[size_t(j) * mid_row]) * k[j];
        v = clip8(acc);
    }
    const size_t o = size_t(oy) * row_out + ob;
    if (canvas_u8) canvas_u8[o] = uint8_t(v);
    if (image_f32) image_f32[o] = lut[v];
}

__global__ __launch_bounds__(THREADS) void whenet_letterbox_v_kernel(const uint8_t* __restrict__ mid, LetterboxPlan p,
                                                                     const int32_t* __restrict__ tab,
                                                                     const float* __restrict__ lut,
                                                                     uint8_t* __restrict__ canvas_u8,
                                                                     float* __restrict__ image_f32) {
    letterbox_v_byte(mid, p, tab, lut, canvas_u8, image_f32, blockIdx.y, blockIdx.x * THREADS + threadIdx.x);
}

// The same over the frames of a clip (grid z): frame f reads mid + f * ih * nw * 3 and writes canvas f of [F][oh][ow][3].
// p is the plan of ONE frame; every frame shares its tables.
__global__ __launch_bounds__(THREADS) void whenet_letterbox_v_batch_kernel(const uint8_t* __restrict__ mid, LetterboxPlan p,
                                                                           const int32_t* __restrict__ tab,
                                                                           const float* __restrict__ lut,
                                                                           uint8_t* __restrict__ canvas_u8,
                                                                           float* __restrict__ image_f32) {
    const size_t f = blockIdx.z;
    const size_t mid_stride = size_t(p.ih) * p.nw * 3, out_stride = size_t(p.oh) * p.ow * 3;
    letterbox_v_byte(mid + f * mid_stride, p, tab, lut, canvas_u8 ? canvas_u8 + f * out_stride : nullptr,
                     image_f32 ? image_f32 + f * out_stride : nullptr, blockIdx.y, blockIdx.x * THREADS + threadIdx.x);
}

// The frames of a MIXED clip (grid z): frame f has its own plan, tables and place in mid; the canvases are [F][oh][ow][3].
__global__ __launch_bounds__(THREADS) void whenet_letterbox_v_mixed_kernel(const uint8_t* __restrict__ mid, LetterboxMixed clip,
                                                                           const float* __restrict__ lut,
                                                                           uint8_t* __restrict__ canvas_u8,
                                                                           float* __restrict__ image_f32) {
    const size_t f = blockIdx.z;
    const LetterboxMixedFrame& fr = clip.f[f];
    const size_t out_stride = size_t(fr.p.oh) * fr.p.ow * 3;
    letterbox_v_byte(mid + size_t(fr.mid_off), fr.p, fr.tab, lut, canvas_u8 ? canvas_u8 + f * out_stride : nullptr,
                     image_f32 ? image_f32 + f * out_stride : nullptr, blockIdx.y, blockIdx.x * THREADS + threadIdx.x);
}

// Resample.c bicubic_filter
inline double bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

}  // namespace

int letterbox_axis_ksize(int in_size, int out_size) {
    double filterscale = double(in_size) / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    return int(std::ceil(2.0 * filterscale)) * 2 + 1;
}

// Resample.c precompute_coeffs + normalize_coeffs_8bpc for the BICUBIC filter (support 2) over the whole axis.  No
// contraction: every product and sum is rounded to double on its own, as Pillow's build computes them.
void build_letterbox_axis(int in_size, int out_size, int32_t* bounds, int32_t* coeffs) {
#pragma clang fp contract(off)
    const double scale = double(in_size) / out_size;
    double filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 2.0 * filterscale;
    const int ksize = int(std::ceil(support)) * 2 + 1;
    const double ss = 1.0 / filterscale;
    std::vector<double> kk(size_t(ksize), 0.0);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = int(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = int(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) {
            const double w = bicubic((x + xmin - center + 0.5) * ss);
            kk[size_t(x)] = w;
            ww += w;
        }
        for (int x = 0; x < xmax; ++x)
            if (ww != 0.0) kk[size_t(x)] /= ww;
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
        int32_t* k = coeffs + size_t(xx) * ksize;
        for (int x = 0; x < ksize; ++x) {
            const double v = x < xmax ? kk[size_t(x)] : 0.0;
            k[x] = v < 0 ? int32_t(-0.5 + v * (1 << PRECISION_BITS)) : int32_t(0.5 + v * (1 << PRECISION_BITS));
        }
    }
}

LetterboxPlan letterbox_plan_layout(int ih, int iw, int out_h, int out_w) {
#pragma clang fp contract(off)
    WHENET_REQUIRE(ih >= 1 && iw >= 1 && ih <= LETTERBOX_MAX_FRAME_SIDE && iw <= LETTERBOX_MAX_FRAME_SIDE, WHENET_EINVAL,
                   "letterbox: frame sides must be 1.." + std::to_string(LETTERBOX_MAX_FRAME_SIDE));
    WHENET_REQUIRE(out_h >= 1 && out_w >= 1 && out_h <= LETTERBOX_MAX_BOX_SIDE && out_w <= LETTERBOX_MAX_BOX_SIDE, WHENET_EINVAL,
                   "letterbox: output sides must be 1.." + std::to_string(LETTERBOX_MAX_BOX_SIDE));
    LetterboxPlan p{};
    p.ih = ih, p.iw = iw, p.oh = out_h, p.ow = out_w;
    // utils.py:25-29 as Python evaluates it: true division in double, min(), int() truncation
    const double sw = double(out_w) / double(iw), sh = double(out_h) / double(ih);
    const double scale = sh < sw ? sh : sw;
    p.nw = int(double(iw) * scale);
    p.nh = int(double(ih) * scale);
    WHENET_REQUIRE(p.nw >= 1 && p.nh >= 1, WHENET_EINVAL,
                   "letterbox: the resized image would be " + std::to_string(p.nw) + " x " + std::to_string(p.nh) +
                       " pixels (Image.resize raises: height and width must be > 0)");
    p.x0 = (out_w - p.nw) / 2;       // utils.py:33 (nw <= w, nh <= h: floor division of a non-negative number)
    p.y0 = (out_h - p.nh) / 2;
    p.ksx = letterbox_axis_ksize(iw, p.nw);
    p.ksy = letterbox_axis_ksize(ih, p.nh);
    p.off_bx = 0;
    p.off_cx = p.off_bx + 2 * p.nw;
    p.off_by = p.off_cx + p.nw * p.ksx;
    p.off_cy = p.off_by + 2 * p.nh;
    p.table_ints = p.off_cy + p.nh * p.ksy;
    return p;
}

LetterboxPlan build_letterbox_plan(int ih, int iw, int out_h, int out_w, std::vector<int32_t>* tables) {
    const LetterboxPlan p = letterbox_plan_layout(ih, iw, out_h, out_w);
    tables->assign(size_t(p.table_ints), 0);
    build_letterbox_axis(iw, p.nw, tables->data() + p.off_bx, tables->data() + p.off_cx);
    build_letterbox_axis(ih, p.nh, tables->data() + p.off_by, tables->data() + p.off_cy);
    return p;
}

void letterbox_float_table(float lut[256]) {
    for (int v = 0; v < 256; ++v) lut[v] = float(v) / 255.0f;     // `image_data /= 255.` on a float32 array
}

void launch_letterbox(const uint8_t* d_frame, const LetterboxPlan& p, int swap_rb, const int32_t* d_tables,
                      const float* d_lut, uint8_t* d_mid, uint8_t* d_canvas_u8, float* d_image_f32, int num_cus,
                      hipStream_t stream) {
    if (d_canvas_u8 == nullptr && d_image_f32 == nullptr) return;
    const int rows_wg = p.ih < num_cus * 8 ? p.ih : num_cus * 8;
    hipLaunchKernelGGL(whenet_letterbox_h_kernel, dim3(rows_wg), dim3(THREADS), 0, stream, d_frame, p, swap_rb, d_tables,
                       d_mid);
    WHENET_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(whenet_letterbox_v_kernel, dim3((p.ow * 3 + THREADS - 1) / THREADS, p.oh), dim3(THREADS), 0, stream,
                       d_mid, p, d_tables, d_lut, d_canvas_u8, d_image_f32);
    WHENET_HIP_CHECK(hipGetLastError());
}

// F frames [F][ih][iw][3] of one geometry -> canvases [F][oh][ow][3].  The horizontal pass is row-independent: the clip is
// F * ih rows of one buffer (a frame's first byte need not be 16-byte aligned; neither is a row's), so it is the kernel above
// with the row count of the whole clip.  d_mid holds F * ih * nw * 3 bytes.
void launch_letterbox_batch(const uint8_t* d_frames, int frames, const LetterboxPlan& p, int swap_rb, const int32_t* d_tables,
                            const float* d_lut, uint8_t* d_mid, uint8_t* d_canvas_u8, float* d_image_f32, int num_cus,
                            hipStream_t stream) {
    WHENET_REQUIRE(frames >= 1 && frames <= 65535, WHENET_EINVAL, "letterbox: bad frame count");
    if (d_canvas_u8 == nullptr && d_image_f32 == nullptr) return;
    LetterboxPlan rows = p;
    rows.ih = p.ih * frames;
    const int rows_wg = rows.ih < num_cus * 8 ? rows.ih : num_cus * 8;
    hipLaunchKernelGGL(whenet_letterbox_h_kernel, dim3(rows_wg), dim3(THREADS), 0, stream, d_frames, rows, swap_rb, d_tables,
                       d_mid);
    WHENET_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(whenet_letterbox_v_batch_kernel, dim3((p.ow * 3 + THREADS - 1) / THREADS, p.oh, frames), dim3(THREADS), 0,
                       stream, d_mid, p, d_tables, d_lut, d_canvas_u8, d_image_f32);
    WHENET_HIP_CHECK(hipGetLastError());
}

void launch_letterbox_mixed(const uint8_t* d_frames, const LetterboxMixed& clip, int swap_rb, const float* d_lut, uint8_t* d_mid,
                            uint8_t* d_canvas_u8, float* d_image_f32, int num_cus, hipStream_t stream) {
    WHENET_REQUIRE(clip.frames >= 1 && clip.frames <= MIXED_MAX_FRAMES && clip.total_rows >= clip.frames, WHENET_EINVAL,
                   "letterbox: bad frame count");
    if (d_canvas_u8 == nullptr && d_image_f32 == nullptr) return;
    const LetterboxPlan& p0 = clip.f[0].p;
    for (int f = 0; f < clip.frames; ++f) {
        const LetterboxMixedFrame& fr = clip.f[f];
        WHENET_REQUIRE(fr.tab != nullptr && fr.p.oh == p0.oh && fr.p.ow == p0.ow && fr.p.iw >= 1 && fr.p.iw <= LETTERBOX_MAX_FRAME_SIDE &&
                           fr.frame_off + size_t(fr.p.ih) * fr.p.iw * 3 <= clip.total_bytes &&
                           fr.row0 + fr.p.ih <= clip.total_rows,
                       WHENET_EINVAL, "letterbox: inconsistent geometry record of frame " + std::to_string(f));
    }
    const int rows_wg = clip.total_rows < num_cus * 8 ? clip.total_rows : num_cus * 8;
    hipLaunchKernelGGL(whenet_letterbox_h_mixed_kernel, dim3(rows_wg), dim3(THREADS), 0, stream, d_frames, clip, swap_rb, d_mid);
    WHENET_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(whenet_letterbox_v_mixed_kernel, dim3((p0.ow * 3 + THREADS - 1) / THREADS, p0.oh, clip.frames), dim3(THREADS), 0,
                       stream, d_mid, clip, d_lut, d_canvas_u8, d_image_f32);
    WHENET_HIP_CHECK(hipGetLastError());
}

}  // namespace whenet
