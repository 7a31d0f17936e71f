// YOLOv3 post-processing on the device: box decode + score threshold + per-class greedy NMS.
//
// Reference: /root/reference/yolo_v3/model.py:125-150 (yolo_head), :153-178 (yolo_correct_boxes),
// :181-190 (yolo_boxes_and_scores), :193-232 (yolo_eval: anchor masks, `box_scores >= score_threshold`,
// tf.image.non_max_suppression per class, results concatenated class by class); run by the reference
// inside sess.run (yolo_postprocess.py:198-204) on the detector's 2 or 3 output maps.  SURVEY.md §8f row 4.
//
// Mapping (gfx950).  The work is small (10,647 boxes for a 416x416 input) and branchy, so it is two launches:
// A batch of images (a clip's frames) is the grid's second dimension of both launches: image f's maps, boxes, counters, keys
// and outputs lie f strides behind image 0's, the arithmetic and the key order are those of one image.
//   1. whenet_yolo_decode_kernel: one lane per box (layer, y, x, anchor), coalesced over the map.  It writes the
//      corrected box (y_min, x_min, y_max, x_max in image pixels) to a dense [N][4] array and, for every class
//      whose score = confidence * class probability passes the threshold, appends a 64-bit key
//      (score bits << 32 | ~box index) to that class's candidate list (one atomic counter per class).
//   2. whenet_yolo_nms_kernel: one workgroup per class.  The keys are sorted descending (bitonic, in LDS up to
//      4096 candidates, in the global key array beyond that): score first, LOWER box index first among equal
//      scores -- the append order of step 1 is arbitrary, the sorted order is not.  Wave 0 then walks the
//      candidates in that order: the lanes test the candidate against the boxes selected so far (TensorFlow's
//      IOU(): min/max-normalised corners, zero for a box of non-positive area, suppressed when IoU > threshold,
//      float32 with individually rounded operations), one ballot decides, selected boxes live in LDS.
// All arithmetic is float32 with the operation order of the reference's graph; exp / sigmoid go through expf,
// so box coordinates agree with a float32 CPU run to an ulp or two, not bitwise (tests/test_yolo.py).  On the logits where
// expf is exact (0 and +-128: sigmoid 0.5 / 1 / 0, exp 1 / inf / 0) boxes and scores ARE bitwise the float32 CPU run's, and the
// selection is the CPU NMS of the device's own decoded rows at every sort size (tests/test_yolo_exact_gpu.py).
#include <cmath>

#include "kernels.h"

namespace whenet {

namespace {

// One float32 operation, rounded on its own.  HIP's __fadd_rn / __fsub_rn / __fmul_rn are the plain operators, and hipcc contracts a
// plain a * b + c into one FMA: `cy - hy` below was fma(by - off_y, scale_y, -hy), an ulp off the graph's two roundings wherever the
// letterbox scale is not 1 (tests/test_yolo_exact_gpu.py).  Contraction is off for everything in this file from here on (as in
// headplan.hip), and every operation goes through these.
#pragma clang fp contract(off)
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }

__device__ __forceinline__ float sigmoid_ref(float x) { return 1.0f / (1.0f + expf(-x)); }

// one box of image img: decode, correction c (that of the image), candidate keys
__device__ __forceinline__ void yolo_decode_box(const YoloArgs& a, const MixedFrameCorrection& c, const size_t img, const int i) {
    int l = 0;
    while (l + 1 < a.num_layers && i >= a.layer[l + 1].first) ++l;
    const YoloLayer& L = a.layer[l];
    const int j = i - L.first;                                  // ((y * gw + x) * A + anchor)
    const int an = j % a.na, cell = j / a.na;
    const int y = cell / L.gw, x = cell - y * L.gw;
    const float* t = L.feats + (img * L.gh * L.gw * a.na + size_t(j)) * (5 + a.num_classes);

    // yolo_head (model.py:141-145)
    const float bx = div_rn(add_rn(sigmoid_ref(t[0]), float(x)), float(L.gw));
    const float by = div_rn(add_rn(sigmoid_ref(t[1]), float(y)), float(L.gh));
    const float bw = div_rn(mul_rn(expf(t[2]), L.anchor[an][0]), a.input_w);
    const float bh = div_rn(mul_rn(expf(t[3]), L.anchor[an][1]), a.input_h);
    const float conf = sigmoid_ref(t[4]);
    // yolo_correct_boxes (model.py:155-177): y first
    const float cy = mul_rn(sub_rn(by, c.off_y), c.scale_y), cx = mul_rn(sub_rn(bx, c.off_x), c.scale_x);
    const float hh = mul_rn(bh, c.scale_y), ww = mul_rn(bw, c.scale_x);
    const float hy = div_rn(hh, 2.0f), hx = div_rn(ww, 2.0f);
    float4 box;
    box.x = mul_rn(sub_rn(cy, hy), c.image_h);
    box.y = mul_rn(sub_rn(cx, hx), c.image_w);
    box.z = mul_rn(add_rn(cy, hy), c.image_h);
    box.w = mul_rn(add_rn(cx, hx), c.image_w);
    reinterpret_cast<float4*>(a.boxes)[img * a.N + i] = box;
    // yolo_boxes_and_scores (model.py:188) + the mask of yolo_eval (model.py:212)
    for (int cl = 0; cl < a.num_classes; ++cl) {
        const float score = mul_rn(conf, sigmoid_ref(t[5 + cl]));
        if (a.all_scores) a.all_scores[(img * a.N + i) * a.num_classes + cl] = score;
        if (score >= a.score_thr) {
            const size_t ic = img * a.num_classes + cl;
            const int slot = atomicAdd(&a.counts[ic], 1);
            a.keys[ic * a.NP + slot] =
                (static_cast<unsigned long long>(__float_as_uint(score)) << 32) | (0xffffffffu - unsigned(i));
        }
    }
}

__global__ __launch_bounds__(256) void whenet_yolo_decode_kernel(YoloArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    const MixedFrameCorrection c{a.image_h, a.image_w, a.off_y, a.off_x, a.scale_y, a.scale_x};
    yolo_decode_box(a, c, blockIdx.y, i);                       // image of a batch: every array is [images][...]
}

// images of different shapes (a mixed clip): image blockIdx.y has its own correction values
__global__ __launch_bounds__(256) void whenet_yolo_decode_mixed_kernel(YoloArgs a, YoloMixed m) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    yolo_decode_box(a, m.img[blockIdx.y], blockIdx.y, i);
}

// TensorFlow's IOU() (core/kernels/non_max_suppression_op.cc), float32, every operation rounded on its own
__device__ __forceinline__ float iou_tf(const float4 a, const float4 b) {
    const float ymin_a = fminf(a.x, a.z), xmin_a = fminf(a.y, a.w), ymax_a = fmaxf(a.x, a.z), xmax_a = fmaxf(a.y, a.w);
    const float ymin_b = fminf(b.x, b.z), xmin_b = fminf(b.y, b.w), ymax_b = fmaxf(b.x, b.z), xmax_b = fmaxf(b.y, b.w);
    const float area_a = mul_rn(sub_rn(ymax_a, ymin_a), sub_rn(xmax_a, xmin_a));
    const float area_b = mul_rn(sub_rn(ymax_b, ymin_b), sub_rn(xmax_b, xmin_b));
    if (area_a <= 0.0f || area_b <= 0.0f) return 0.0f;
    const float iymin = fmaxf(ymin_a, ymin_b), ixmin = fmaxf(xmin_a, xmin_b);
    const float iymax = fminf(ymax_a, ymax_b), ixmax = fminf(xmax_a, xmax_b);
    const float inter = mul_rn(fmaxf(sub_rn(iymax, iymin), 0.0f), fmaxf(sub_rn(ixmax, ixmin), 0.0f));
    return div_rn(inter, sub_rn(add_rn(area_a, area_b), inter));
}

constexpr int NMS_THREADS = 1024;
constexpr int NMS_LDS_KEYS = 4096;             // 32 KB of keys
constexpr int NMS_MAX_SELECT = 256;

__global__ __launch_bounds__(NMS_THREADS) void whenet_yolo_nms_kernel(YoloArgs a) {
    __shared__ unsigned long long s_keys[NMS_LDS_KEYS];
    __shared__ float4 s_sel[NMS_MAX_SELECT];
    const size_t c = size_t(blockIdx.y) * a.num_classes + blockIdx.x;      // (image, class): every array below is [images][C]...
    const int tid = threadIdx.x;
    int n = a.counts[c];
    if (n > a.N) n = a.N;
    int P = 1;
    while (P < n) P <<= 1;
    unsigned long long* gk = a.keys + c * a.NP;
    const bool in_lds = P <= NMS_LDS_KEYS;
    unsigned long long* k = in_lds ? s_keys : gk;           // (generic pointer: LDS or global)
    if (in_lds) {
        for (int i = tid; i < P; i += NMS_THREADS) s_keys[i] = (i < n) ? gk[i] : 0ull;
    } else {
        for (int i = n + tid; i < P; i += NMS_THREADS) gk[i] = 0ull;          // NP >= next power of two of N
    }
    __syncthreads();
    // bitonic sort, descending
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < (P >> 1); i += NMS_THREADS) {
                const int lo = 2 * i - (i & (stride - 1));
                const int hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const unsigned long long x = k[lo], y = k[hi];
                if (desc ? (x < y) : (x > y)) {
                    k[lo] = y;
                    k[hi] = x;
                }
            }
            __syncthreads();
        }
    }
    if (tid >= 64) return;
    // greedy selection by wave 0
    const float4* boxes = reinterpret_cast<const float4*>(a.boxes) + size_t(blockIdx.y) * a.N;
    float* ob = a.out_boxes + c * a.max_boxes * 4;
    float* os = a.out_scores + c * a.max_boxes;
    int* oi = a.out_index + c * a.max_boxes;
    int nsel = 0;
    for (int i = 0; i < n && nsel < a.max_boxes; ++i) {
        const unsigned long long key = k[i];
        const int idx = int(0xffffffffu - unsigned(key & 0xffffffffull));
        const float4 box = boxes[idx];
        bool sup = false;
        for (int j = tid; j < nsel; j += 64) {
            float4 sj;
            if (j < NMS_MAX_SELECT) {
                sj = s_sel[j];
            } else {                                      // beyond the LDS list: the output array itself, read from L2
                sj.x = __hip_atomic_load(ob + j * 4 + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                sj.y = __hip_atomic_load(ob + j * 4 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                sj.z = __hip_atomic_load(ob + j * 4 + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                sj.w = __hip_atomic_load(ob + j * 4 + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            sup = sup || (iou_tf(box, sj) > a.iou_thr);
        }
        if (__ballot(sup) == 0ull) {
            if (tid == 0) {
                if (nsel < NMS_MAX_SELECT) s_sel[nsel] = box;
                __hip_atomic_store(ob + nsel * 4 + 0, box.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(ob + nsel * 4 + 1, box.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(ob + nsel * 4 + 2, box.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(ob + nsel * 4 + 3, box.w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                os[nsel] = __uint_as_float(unsigned(key >> 32));
                oi[nsel] = idx;
            }
            ++nsel;
            // the new box is visible to the wave's next reads (LDS list; beyond it the write-through stores have
            // reached L2 before the L2 loads above are issued)
            if (nsel > NMS_MAX_SELECT) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    }
    if (tid == 0) a.out_count[c] = nsel;
}

}  // namespace

int yolo_max_select() { return NMS_MAX_SELECT; }

// model.py:158-162, float32 like the graph: new_shape = round(image_shape * min(input_shape / image_shape))
MixedFrameCorrection yolo_correction(float input_h, float input_w, float image_h, float image_w) {
    MixedFrameCorrection c{};
    c.image_h = image_h, c.image_w = image_w;
    const float ry = input_h / image_h, rx = input_w / image_w;
    const float r = ry < rx ? ry : rx;
    const float new_h = std::nearbyintf(image_h * r), new_w = std::nearbyintf(image_w * r);      // half to even
    c.off_y = (input_h - new_h) / 2.0f / input_h;
    c.off_x = (input_w - new_w) / 2.0f / input_w;
    c.scale_y = input_h / new_h;
    c.scale_x = input_w / new_w;
    return c;
}

void launch_yolo_eval(const YoloArgs& a, hipStream_t stream, const YoloMixed* mixed) {
    WHENET_REQUIRE(a.N > 0 && a.num_classes > 0 && a.max_boxes > 0 && a.max_boxes <= a.N, WHENET_EINVAL,
                   "yolo_eval: bad sizes (max_boxes must be 1..number of boxes)");
    const unsigned images = a.images > 1 ? unsigned(a.images) : 1u;
    WHENET_HIP_CHECK(hipMemsetAsync(a.counts, 0, size_t(images) * a.num_classes * sizeof(int), stream));
    WHENET_REQUIRE(mixed == nullptr || images <= unsigned(MIXED_MAX_FRAMES), WHENET_EINVAL, "yolo_eval: too many images of different shapes");
    if (mixed) hipLaunchKernelGGL(whenet_yolo_decode_mixed_kernel, dim3((a.N + 255) / 256, images), dim3(256), 0, stream, a, *mixed);
    else hipLaunchKernelGGL(whenet_yolo_decode_kernel, dim3((a.N + 255) / 256, images), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(whenet_yolo_nms_kernel, dim3(a.num_classes, images), dim3(NMS_THREADS), 0, stream, a);
    WHENET_HIP_CHECK(hipGetLastError());
}

}  // namespace whenet
