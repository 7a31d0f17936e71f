// The detector body's layers (yolo_v3/model.py:20-122): dense 3x3 / 1x1 convolutions with folded BatchNorm, LeakyReLU(0.1),
// residual adds, the upsample + concatenate read, the 2x2 max-pools of the tiny body, and the image -> binary16 input stage.
//
// whenet_dconv_kernel is an implicit GEMM on v_mfma_f32_32x32x16_f16 in pw.hip's orientation: the WEIGHTS are the A operand (rows =
// out-channels), the ACTIVATIONS the B operand (columns = output pixels), so a lane owns ONE pixel (lane & 31) and its 16 accumulator
// registers are four runs of 4 consecutive out-channels (row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)): the epilogue stores 8-byte
// pieces straight into NHWC.  M = n * Ho * Wo output pixels, flattened over the batch (the halo test is made on each pixel's own
// (image, y, x), so a tile that spans two images reads neither's rows for the other); N = Cout; K = (tap, Cin) with one k-step of 16
// channels inside one tap.
//   * activation fragment: 8 consecutive channels of one input pixel = one 16-byte load, zeros (not clamped reads) outside the image.
//     Input row = stride * o + t - 1 for the 3x3 forms: pad 1 all round at stride 1, top / left only at stride 2
//     (ZeroPadding2D(((1,0),(1,0))) + 'valid', model.py:40-41).
//   * second source: channels [0, C0) come from the HALF-resolution tensor at (y >> 1, x >> 1) and [C0, C0 + C1) from the route
//     tensor: UpSampling2D(2) + Concatenate() (model.py:78-87, 114-120) never reach memory.
//   * weights: host-packed in fragment order [k-step][32-channel tile][lane][8] (detector.cpp pack_dconv), 1 KiB per wave load.
//   * a wave owns 32 pixels x NT 32-channel tiles (NT = 4, 2 or 1, dividing the layer's tile count) and is independent of the other
//     three of its workgroup (no LDS, no barrier): the nine taps of a pixel are nine loads of the same lines by neighbouring lanes
//     and waves, served by the vector cache.  The fragments of four k-steps are loaded before the first product waits.
//   * split-K (grid.y): each split writes its f32 accumulators to a workspace, whenet_dconv_combine_kernel adds them in split
//     order and runs the epilogue.  The number of splits is a function of the layer (dconv_splits), never of the batch.
//   * epilogue: + bias (f32), LeakyReLU as ONE f32 multiply by 0.1f, + skip (binary16 read, f32 add), one rounding to binary16 --
//     or, for the output convolutions, float32 stores into the unpadded [gh][gw][A (5 + C)] map yolo.hip reads.
//
// Float32 storage (T = float, engine option "detector_dtype" = 1) is the same kernel on v_mfma_f32_32x32x2_f32: a k-step is 8
// channels, the lane's 16-byte fragment is channels 4 hh .. 4 hh + 3 of the group (hh = lane >> 5) and goes through
// Mfma<float>::step as four instructions (instruction t multiplies channels t and 4 + t); weights in the same fragment order
// [k-step][32-channel tile][lane][4], still 1 KiB per wave load; the skip is read and the result stored as float32, so nothing is
// rounded to binary16 anywhere.  Tiling, split-K and the combine order are those of the binary16 form; a tile has TWO accumulator
// sets, fed alternately by the k-steps of a group of four and added once before the epilogue (half the chain of dependent float32
// additions: NT = 4 then holds 128 accumulators + ~135 registers of fragments and addresses, one wave per SIMD, nothing spills).
#include <algorithm>

#include "device_math.h"
#include "kernels.h"

namespace whenet {

namespace {

template <typename T>
__device__ __forceinline__ void dconv_store4(const DconvArgs& a, int p, int c0, float4v v) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float x = __fadd_rn(v[j], a.bias[c0 + j]);            // (bias is padded to the tile: always readable)
        if (a.leaky && x < 0.0f) x = __fmul_rn(x, 0.1f);
        v[j] = x;
    }
    if (a.f32_out) {
        float* o = static_cast<float*>(a.out) + size_t(p) * a.Cout;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c0 + j < a.Cout) o[c0 + j] = v[j];
        return;
    }
    if (c0 >= a.Cout) return;                                  // (activation outputs have Cout % 16 == 0: whole runs)
    const size_t off = size_t(p) * a.Cout + c0;
    if constexpr (IsF32<T>::value) {
        if (a.skip) {
            const float4v s = *reinterpret_cast<const float4v*>(static_cast<const float*>(a.skip) + off);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = __fadd_rn(v[j], s[j]);
        }
        *reinterpret_cast<float4v*>(static_cast<float*>(a.out) + off) = v;
    } else {
        if (a.skip) {
            const half4 s = *reinterpret_cast<const half4*>(static_cast<const half_t*>(a.skip) + off);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = __fadd_rn(v[j], float(s[j]));
        }
        half4 h;
#pragma unroll
        for (int j = 0; j < 4; ++j) h[j] = half_t(v[j]);
        *reinterpret_cast<half4*>(static_cast<half_t*>(a.out) + off) = h;
    }
}

template <typename T, int NT>
__global__ __launch_bounds__(256) void whenet_dconv_kernel(DconvArgs a) {
    constexpr int V = Vec<T>::V;                                // channels of a lane's 16-byte fragment
    constexpr int KC = 2 * V;                                   // channels of a k-step: 16 (binary16) or 8 (float32)
    constexpr int KSH = IsF32<T>::value ? 3 : 4;                // log2(KC)
    // float32: the k-steps of a group of four go alternately to TWO accumulator sets, added once at the end -- the dependent
    // chain of float32 additions behind a result is half as long and its rounding error about 1 / sqrt(2) of one chain's
    // (measured: docs/experiments.md section 20).  binary16's error is its storage rounding: one set.
    constexpr int CH = IsF32<T>::value ? 2 : 1;
    using VT = typename Vec<T>::type;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int HoWo = a.Ho * a.Wo;
    const int M = a.n * HoWo;
    const int MT = (M + 31) / 32;
    const int NT32 = (a.Cout + 31) / 32;
    const int NG = (NT32 + NT - 1) / NT;
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= MT * NG) return;                                // (wave-uniform; the waves share nothing)
    const int mt = tile / NG, ng = tile - mt * NG;
    const int r = lane & 31, hh = lane >> 5;
    const int p = mt * 32 + r;
    const bool pv = p < M;
    int img = 0, oy = 0, ox = 0;
    if (pv) {
        img = p / HoWo;
        const int rem = p - img * HoWo;
        oy = rem / a.Wo;
        ox = rem - oy * a.Wo;
    }
    const int CS = (a.C0 + a.C1) >> KSH;                         // k-steps per tap
    const int KS = a.k * a.k * CS;
    const int per = (KS + a.splits - 1) / a.splits;
    const int ks0 = int(blockIdx.y) * per;
    const int ks1 = ks0 + per < KS ? ks0 + per : KS;
    const int pad = a.k == 3 ? 1 : 0;
    const int H2 = a.H >> 1, W2 = a.W >> 1;

    float16v acc[CH][NT];
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[c][t][i] = 0.0f;

    const VT* const wp = static_cast<const VT*>(a.w);
    const T* const safe = static_cast<const T*>(a.w);           // any readable address for the lanes that load nothing
    const T* const in0 = static_cast<const T*>(a.in0);
    const T* const in1 = static_cast<const T*>(a.in1);
    const int CS0 = a.C0 >> KSH;                                // k-steps of a tap that read the first source
    const size_t wstep = size_t(NT32) * 64;                     // fragments per k-step of the weight image
    // `count` k-steps of one tap from one source: four steps at a time, so that the loads of four steps are
    // in flight before the first product waits
    auto run = [&](const T* bp, bool valid, int count, const VT* wk) {
        const T* const p0 = valid ? bp : safe;
        const int step = valid ? KC : 0;
        const VT zero = vec_zero<T>();
        int i = 0;
        for (; i + 4 <= count; i += 4) {
            VT x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = *reinterpret_cast<const VT*>(p0 + (i + u) * step);
            VT w[4][NT];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int t = 0; t < NT; ++t) w[u][t] = wk[(i + u) * wstep + t * 64];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const VT xu = valid ? x[u] : zero;
#pragma unroll
                for (int t = 0; t < NT; ++t) Mfma<T>::step(w[u][t], xu, acc[u % CH][t]);
            }
        }
        for (; i < count; ++i) {
            VT x = *reinterpret_cast<const VT*>(p0 + i * step);
            if (!valid) x = zero;
#pragma unroll
            for (int t = 0; t < NT; ++t) Mfma<T>::step(wk[i * wstep + t * 64], x, acc[0][t]);
        }
    };
    int tap = ks0 / CS, cs = ks0 - tap * CS;
    int ks = ks0;
    while (ks < ks1) {
        const int ky = tap / a.k, kx = tap - ky * a.k;
        const int iy = oy * a.stride + ky - pad, ix = ox * a.stride + kx - pad;
        const bool valid = pv && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
        const int cend = (CS - cs) < (ks1 - ks) ? CS : cs + (ks1 - ks);
        const VT* const wk = wp + (size_t(ks) * NT32 + size_t(ng) * NT) * 64 + lane;      // k-step cs of this tap
        // this lane's channels V hh.. of the tap's pixel in either source
        const int e0 = cend < CS0 ? cend : CS0;                 // [cs, e0): first source; [max(cs, CS0), cend): second
        if (cs < e0) {
            const T* const b0 = in1 ? in0 + ((size_t(img) * H2 + (iy >> 1)) * W2 + (ix >> 1)) * a.C0
                                    : in0 + ((size_t(img) * a.H + iy) * a.W + ix) * a.C0;
            run(b0 + KC * cs + V * hh, valid, e0 - cs, wk);
        }
        const int s1 = cs > CS0 ? cs : CS0;
        if (s1 < cend) {
            const T* const b1 = in1 + ((size_t(img) * a.H + iy) * a.W + ix) * a.C1;
            run(b1 + KC * (s1 - CS0) + V * hh, valid, cend - s1, wk + size_t(s1 - cs) * wstep);
        }
        ks += cend - cs;
        cs = cend;
        if (cs == CS) cs = 0, ++tap;
    }

    if (!pv) return;
    if constexpr (CH == 2) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[0][t][i] = __fadd_rn(acc[0][t][i], acc[1][t][i]);
    }
    const int NP = NT32 * 32;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int nt = ng * NT + t;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c0 = nt * 32 + 8 * g + 4 * hh;
            const float4v v = {acc[0][t][4 * g], acc[0][t][4 * g + 1], acc[0][t][4 * g + 2], acc[0][t][4 * g + 3]};
            if (a.splits > 1)
                *reinterpret_cast<float4v*>(a.partial + (size_t(blockIdx.y) * M + p) * NP + c0) = v;
            else
                dconv_store4<T>(a, p, c0, v);
        }
    }
}

// one lane per (pixel, 4 out-channels): the splits' partial sums added in split order, then the epilogue
template <typename T>
__global__ __launch_bounds__(256) void whenet_dconv_combine_kernel(DconvArgs a) {
    const int M = a.n * a.Ho * a.Wo;
    const int NP = ((a.Cout + 31) / 32) * 32, Q = NP >> 2;
    const size_t i = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= size_t(M) * Q) return;
    const int p = int(i / Q), c0 = int(i - size_t(p) * Q) * 4;
    float4v v = *reinterpret_cast<const float4v*>(a.partial + size_t(p) * NP + c0);
    for (int s = 1; s < a.splits; ++s) {
        const float4v w = *reinterpret_cast<const float4v*>(a.partial + (size_t(s) * M + p) * NP + c0);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = __fadd_rn(v[j], w[j]);
    }
    dconv_store4<T>(a, p, c0, v);
}

// MaxPooling2D(2, strides, 'same') on NHWC (model.py:96-107): one lane per (output pixel, 16 bytes of channels: 8 binary16 or 4
// float32).  'same' pads bottom / right only (stride 1 always, stride 2 on odd sides); a tap outside the image takes no part in
// the max.
template <typename T>
__global__ __launch_bounds__(256) void whenet_dpool_kernel(const T* __restrict__ in, T* __restrict__ out, int n, int H, int W, int C,
                                                           int stride, int Ho, int Wo) {
    constexpr int V = Vec<T>::V;
    using VT = typename Vec<T>::type;
    const int CG = C >> (IsF32<T>::value ? 2 : 3);
    const size_t i = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= size_t(n) * Ho * Wo * CG) return;
    const int cg = int(i % CG);
    size_t q = i / CG;
    const int ox = int(q % Wo);
    q /= Wo;
    const int oy = int(q % Ho), img = int(q / Ho);
    const int y0 = oy * stride, x0 = ox * stride;
    VT m = *reinterpret_cast<const VT*>(in + ((size_t(img) * H + y0) * W + x0) * C + V * cg);      // (always inside)
#pragma unroll
    for (int t = 1; t < 4; ++t) {
        const int y = y0 + (t >> 1), x = x0 + (t & 1);
        if (y >= H || x >= W) continue;
        const VT v = *reinterpret_cast<const VT*>(in + ((size_t(img) * H + y) * W + x) * C + V * cg);
#pragma unroll
        for (int j = 0; j < V; ++j) m[j] = v[j] > m[j] ? v[j] : m[j];
    }
    *reinterpret_cast<VT*>(out + i * V) = m;
}

// The first layer's input: [pixels][3] float32 (yolo_model.predict's image_data) or the letterbox canvas (uint8, through
// letterbox.hip's /255 table) -> [pixels][16] binary16, channels 3..15 zero, ONE rounding; or -> [pixels][8] float32, channels
// 3..7 zero, the values as they are.  The first convolution then is the general kernel with Cin = 16 / 8 (zero weights beyond
// channel 2).
template <typename T>
__global__ __launch_bounds__(256) void whenet_dimage_kernel(const float* __restrict__ f32, const uint8_t* __restrict__ u8,
                                                            const float* __restrict__ lut, T* __restrict__ out, size_t pixels) {
    using VT = typename Vec<T>::type;
    const size_t i = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= pixels) return;
    VT lo = vec_zero<T>();
    const VT hi = vec_zero<T>();
#pragma unroll
    for (int c = 0; c < 3; ++c) lo[c] = T(f32 ? f32[i * 3 + c] : lut[u8[i * 3 + c]]);
    VT* o = reinterpret_cast<VT*>(out) + i * 2;
    o[0] = lo;
    o[1] = hi;
}

}  // namespace

// 32-channel tiles per wave: the largest of 4, 2, 1 that divides the layer's tile count (every wave has NT whole tiles).  Narrower
// tiles on the layers with few pixel tiles were measured and gained nothing (docs/experiments.md section 16).
int dconv_tile_n(int cout) {
    const int NT32 = (cout + 31) / 32;
    return NT32 % 4 == 0 ? 4 : NT32 % 2 == 0 ? 2 : 1;
}

// Split-K per LAYER (one image's tiles, whatever the batch): the 13 x 13 and 26 x 26 layers have 6 / 22 pixel tiles per image, an
// M x N tiling alone leaves most of the chip idle (as pw.hip's deep GEMMs: fixed-order combine).
int dconv_splits(int k, int cin, int cout, int Ho, int Wo) {
    const int NT = dconv_tile_n(cout), NT32 = (cout + 31) / 32;
    const int tiles = ceil_div(Ho * Wo, 32) * ceil_div(NT32, NT);
    const int KS = k * k * (cin / 16);
    if (tiles >= 256 || KS < 32) return 1;
    return std::max(1, std::min({8, KS / 16, ceil_div(512, tiles)}));
}

size_t dconv_partial_floats(const DconvArgs& a) {
    return a.splits > 1 ? size_t(a.splits) * a.n * a.Ho * a.Wo * (size_t((a.Cout + 31) / 32) * 32) : 0;
}

template <typename T>
static void launch_dconv_t(const DconvArgs& a, int NT, dim3 grid, hipStream_t stream) {
    if (NT == 1) hipLaunchKernelGGL((whenet_dconv_kernel<T, 1>), grid, dim3(256), 0, stream, a);
    else if (NT == 2) hipLaunchKernelGGL((whenet_dconv_kernel<T, 2>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((whenet_dconv_kernel<T, 4>), grid, dim3(256), 0, stream, a);
}

void launch_dconv(const DconvArgs& a, hipStream_t stream) {
    const int KC = a.dtype == WHENET_F32 ? 8 : 16;              // channels of a k-step
    WHENET_REQUIRE((a.dtype == WHENET_F16 || a.dtype == WHENET_F32) && a.n >= 1 && a.Ho >= 1 && a.Wo >= 1 && a.Cout >= 1 &&
                       (a.k == 1 || a.k == 3) && (a.stride == 1 || a.stride == 2) && a.C0 >= KC && a.C0 % KC == 0 && a.C1 % KC == 0 &&
                       (a.C1 == 0) == (a.in1 == nullptr) && a.splits >= 1 && (a.splits == 1 || a.partial != nullptr) &&
                       (a.f32_out || a.Cout % 16 == 0) && (a.in1 == nullptr || (a.H % 2 == 0 && a.W % 2 == 0)),
                   WHENET_EINVAL, "dconv: unsupported layer shape");
    const long M = long(a.n) * a.Ho * a.Wo;
    WHENET_REQUIRE(M < (1L << 30), WHENET_EINVAL, "dconv: too many output pixels");
    const int NT = dconv_tile_n(a.Cout), NT32 = (a.Cout + 31) / 32;
    const long tiles = ((M + 31) / 32) * ceil_div(NT32, NT);
    const dim3 grid(unsigned((tiles + 3) / 4), unsigned(a.splits));
    if (a.dtype == WHENET_F32) launch_dconv_t<float>(a, NT, grid, stream);
    else launch_dconv_t<half_t>(a, NT, grid, stream);
    WHENET_HIP_CHECK(hipGetLastError());
    if (a.splits > 1) {
        const size_t lanes = size_t(M) * (size_t(NT32) * 8);
        const dim3 cgrid(unsigned((lanes + 255) / 256));
        if (a.dtype == WHENET_F32) hipLaunchKernelGGL(whenet_dconv_combine_kernel<float>, cgrid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL(whenet_dconv_combine_kernel<half_t>, cgrid, dim3(256), 0, stream, a);
        WHENET_HIP_CHECK(hipGetLastError());
    }
}

void launch_dpool(const void* in, void* out, int dtype, int n, int H, int W, int C, int stride, hipStream_t stream) {
    WHENET_REQUIRE((dtype == WHENET_F16 || dtype == WHENET_F32) && n >= 1 && H >= 1 && W >= 1 && C >= 8 && C % 8 == 0 &&
                       (stride == 1 || stride == 2),
                   WHENET_EINVAL, "dpool: unsupported shape");
    const int Ho = stride == 2 ? (H + 1) / 2 : H, Wo = stride == 2 ? (W + 1) / 2 : W;
    const size_t lanes = size_t(n) * Ho * Wo * (C / (dtype == WHENET_F32 ? 4 : 8));
    const dim3 grid(unsigned((lanes + 255) / 256));
    if (dtype == WHENET_F32)
        hipLaunchKernelGGL(whenet_dpool_kernel<float>, grid, dim3(256), 0, stream, static_cast<const float*>(in), static_cast<float*>(out), n,
                           H, W, C, stride, Ho, Wo);
    else
        hipLaunchKernelGGL(whenet_dpool_kernel<half_t>, grid, dim3(256), 0, stream, static_cast<const half_t*>(in),
                           static_cast<half_t*>(out), n, H, W, C, stride, Ho, Wo);
    WHENET_HIP_CHECK(hipGetLastError());
}

void launch_dimage(const float* f32, const uint8_t* u8, const float* lut, void* out, int dtype, size_t pixels, hipStream_t stream) {
    WHENET_REQUIRE((dtype == WHENET_F16 || dtype == WHENET_F32) && (f32 != nullptr) != (u8 != nullptr) && (u8 == nullptr || lut != nullptr) &&
                       pixels >= 1,
                   WHENET_EINVAL, "dimage: one source, and the table with the uint8 one");
    const dim3 grid(unsigned((pixels + 255) / 256));
    if (dtype == WHENET_F32)
        hipLaunchKernelGGL(whenet_dimage_kernel<float>, grid, dim3(256), 0, stream, f32, u8, lut, static_cast<float*>(out), pixels);
    else
        hipLaunchKernelGGL(whenet_dimage_kernel<half_t>, grid, dim3(256), 0, stream, f32, u8, lut, static_cast<half_t*>(out), pixels);
    WHENET_HIP_CHECK(hipGetLastError());
}

}  // namespace whenet
