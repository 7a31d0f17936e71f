// The YOLOv3 detector body on the device (yolo_v3/model.py:20-122: yolo_body / tiny_yolo_body), between the letterbox
// (letterbox.hip) and the box selection (yolo.hip): the layer table, the snapshot -> folded, fragment-ordered weights, the
// activation plan and captured forward per input size, the single-layer entry points, and YOLO.detect's composition
// (yolo_postprocess.py:180-205) on a host frame and on a resident one.
#include <cmath>
#include <cstdio>
#include <map>
#include <tuple>

#include "engine_internal.h"

namespace whenet {

using namespace detail;

// ------------------------------------------------------------------------------------------
// layer table: the recursion of darknet_body / make_last_layers / yolo_body and of tiny_yolo_body.  A row is a convolution or a
// pool; ZeroPadding2D, BatchNormalization, LeakyReLU, Add, UpSampling2D and Concatenate are properties of the row that consumes
// them (stride 2 = top / left pad, bn, leaky, skip, src1).
// ------------------------------------------------------------------------------------------
namespace {

struct TableBuilder {
    std::vector<DetLayer> rows;
    int channels(int row) const { return row < 0 ? 3 : rows[size_t(row)].cout; }
    int conv(int src, int k, int stride, int cout, bool bn_leaky = true, int src1 = -1, int skip = -1) {
        DetLayer L{};
        L.op = DET_CONV, L.k = k, L.stride = stride;
        L.cin0 = channels(src);
        L.cin = L.cin0 + (src1 >= 0 ? channels(src1) : 0);
        L.cout = cout, L.bn = bn_leaky, L.leaky = bn_leaky;
        L.src0 = src, L.src1 = src1, L.skip = skip, L.is_output = !bn_leaky;
        rows.push_back(L);
        return int(rows.size()) - 1;
    }
    int pool(int src, int stride) {
        DetLayer L{};
        L.op = DET_POOL, L.k = 2, L.stride = stride;
        L.cin = L.cin0 = L.cout = channels(src);
        L.src0 = src, L.src1 = -1, L.skip = -1;
        rows.push_back(L);
        return int(rows.size()) - 1;
    }
    int resblock(int x, int filters, int blocks) {                      // model.py:37-47
        x = conv(x, 3, 2, filters);
        for (int i = 0; i < blocks; ++i) {
            const int y = conv(x, 1, 1, filters / 2);
            x = conv(y, 3, 1, filters, true, -1, x);                    // Add()([x, y]) closes the row
        }
        return x;
    }
    // model.py:59-70; `up` >= 0: x is Concatenate()([UpSampling2D(2)(up), x]).  Returns the fifth convolution (the next scale's source)
    int last_layers(int x, int up, int filters, int out_filters) {
        int y = up >= 0 ? conv(up, 1, 1, filters, true, x) : conv(x, 1, 1, filters);
        y = conv(y, 3, 1, filters * 2);
        y = conv(y, 1, 1, filters);
        y = conv(y, 3, 1, filters * 2);
        y = conv(y, 1, 1, filters);
        const int z = conv(y, 3, 1, filters * 2);
        conv(z, 1, 1, out_filters, false);
        return y;
    }
};

}  // namespace

std::vector<DetLayer> detector_table(int kind, int out_filters) {
    WHENET_REQUIRE((kind == 0 || kind == 1) && out_filters >= 1, WHENET_EINVAL, "detector_table: kind 0 (yolo_body) or 1 (tiny_yolo_body)");
    TableBuilder t;
    if (kind == 0) {
        int x = t.conv(-1, 3, 1, 32);                                   // darknet_body, model.py:49-57
        x = t.resblock(x, 64, 1);
        x = t.resblock(x, 128, 2);
        const int route2 = x = t.resblock(x, 256, 8);                   // darknet.layers[92]
        const int route1 = x = t.resblock(x, 512, 8);                   // darknet.layers[152]
        x = t.resblock(x, 1024, 4);
        x = t.last_layers(x, -1, 512, out_filters);                     // yolo_body, model.py:73-90
        x = t.conv(x, 1, 1, 256);
        x = t.last_layers(route1, x, 256, out_filters);
        x = t.conv(x, 1, 1, 128);
        t.last_layers(route2, x, 128, out_filters);
    } else {
        int x = -1;                                                     // tiny_yolo_body, model.py:92-122
        for (int f = 16; f <= 128; f *= 2) x = t.pool(t.conv(x, 3, 1, f), 2);
        const int x1 = t.conv(x, 3, 1, 256);
        x = t.conv(t.pool(x1, 2), 3, 1, 512);
        x = t.conv(t.pool(x, 1), 3, 1, 1024);
        const int x2 = t.conv(x, 1, 1, 256);
        t.conv(t.conv(x2, 3, 1, 512), 1, 1, out_filters, false);
        const int up = t.conv(x2, 1, 1, 128);
        t.conv(t.conv(up, 3, 1, 256, true, x1), 1, 1, out_filters, false);
    }
    return t.rows;
}

// ------------------------------------------------------------------------------------------
// weights
// ------------------------------------------------------------------------------------------
namespace {

// Keras HWIO kernel (scaled per out-channel) -> dconv.hip's operand image [k-step][32-channel tile][lane][V], V = 8 (binary16) or
// 4 (float32) elements of a 16-byte fragment: element j of lane l is out-channel 32 nt + (l & 31), tap ks / CS, in-channel
// 2 V (ks % CS) + V (l >> 5) + j; zero beyond Cout and beyond the true Cin (the first layer's 3 channels are padded to a k-step:
// 16 / 8).  The float64 product is rounded ONCE to T.
template <typename T>
std::vector<T> pack_dconv(const float* w, const std::vector<double>& scale, int k, int cin, int cout) {
    constexpr int V = Vec<T>::V, KC = 2 * V;
    const int cinp = (cin + KC - 1) / KC * KC, CS = cinp / KC, KS = k * k * CS, NT32 = (cout + 31) / 32;
    std::vector<T> out(size_t(KS) * NT32 * 64 * V, T(0));
    for (int ks = 0; ks < KS; ++ks)
        for (int nt = 0; nt < NT32; ++nt)
            for (int l = 0; l < 64; ++l) {
                const int co = nt * 32 + (l & 31);
                if (co >= cout) continue;
                for (int j = 0; j < V; ++j) {
                    const int tap = ks / CS, ci = KC * (ks % CS) + V * (l >> 5) + j;
                    if (ci >= cin) continue;
                    const double v = double(w[(size_t(tap) * cin + ci) * cout + co]) * scale[size_t(co)];
                    out[((size_t(ks) * NT32 + nt) * 64 + l) * V + j] = T(v);
                }
            }
    return out;
}

// the image of either storage type on the device
void upload_dconv(DeviceBuffer& dst, int dtype, const float* w, const std::vector<double>& scale, int k, int cin, int cout) {
    auto put = [&](const auto& packed) {
        const size_t bytes = packed.size() * sizeof(packed[0]);
        dst.reset(bytes, "detector weights");
        WHENET_HIP_CHECK(hipMemcpy(dst.as<void>(), packed.data(), bytes, hipMemcpyHostToDevice));
    };
    if (dtype == WHENET_F32) put(pack_dconv<float>(w, scale, k, cin, cout));
    else put(pack_dconv<half_t>(w, scale, k, cin, cout));
}

size_t det_esize(int dtype) { return dtype == WHENET_F32 ? sizeof(float) : sizeof(half_t); }
int det_kc(int dtype) { return dtype == WHENET_F32 ? 8 : 16; }        // channels of a k-step: what the first layer's 3 are padded to

const RawTensor& need(const std::map<std::string, RawTensor>& t, const std::string& name, std::vector<uint32_t> dims) {
    const auto it = t.find(name);
    WHENET_REQUIRE(it != t.end(), WHENET_EFORMAT, "detector snapshot: missing tensor " + name);
    if (it->second.dims != dims) {
        std::string want;
        for (uint32_t d : dims) want += (want.empty() ? "" : ",") + std::to_string(d);
        throw Error(WHENET_EFORMAT, "detector snapshot: " + name + ": shape does not match the layer table (expected [" + want + "])");
    }
    return it->second;
}

std::string det_name(const char* fmt, int i) {
    char buf[32];
    std::snprintf(buf, sizeof(buf), fmt, i);
    return buf;
}

}  // namespace

struct DetConv {
    DeviceBuffer w, bias;
};

// the activation plan and captured forward of one (n, H, W)
struct DetPlan {
    int n = 0, H = 0, W = 0;
    std::vector<int> rh, rw, slot;                 // per row: output height, width and activation slot (-1: an output map)
    std::vector<DeviceBuffer> slots;
    DeviceBuffer img, img_f32, partial;           // img: the first layer's input, [n,H,W,16] binary16 or [n,H,W,8] float32
    DeviceBuffer maps[3];
    int gh[3] = {0, 0, 0}, gw[3] = {0, 0, 0};
    hipGraphExec_t exec = nullptr;
    ~DetPlan() {
        if (exec) (void)hipGraphExecDestroy(exec);
    }
};

struct Detector {
    int kind = 0, out_filters = 0, num_maps = 0;
    int dtype = WHENET_F16;                        // storage of weights and activations (option "detector_dtype" when it was loaded)
    std::vector<DetLayer> table;
    std::vector<DetConv> convs;                    // by row (empty for pools)
    DeviceBuffer lut;                              // letterbox.hip's /255 table
};

void Engine::detector_load(const void* blob, size_t nbytes) {
    DeviceGuard guard(device_);
    WHENET_REQUIRE(blob != nullptr, WHENET_EINVAL, "detector_load: NULL snapshot");
    const auto t = parse_snapshot(blob, nbytes);
    int nconv = 0;
    while (t.count(det_name("dconv%03d/kernel", nconv))) ++nconv;
    WHENET_REQUIRE(nconv == 75 || nconv == 13, WHENET_EFORMAT,
                   "detector snapshot: " + std::to_string(nconv) + " dconvNNN/kernel tensors in sequence from dconv000 (yolo_body has 75, "
                   "tiny_yolo_body 13): missing tensor " + det_name("dconv%03d/kernel", nconv));
    const int kind = nconv == 75 ? 0 : 1;
    const RawTensor& last = t.at(det_name("dconv%03d/kernel", nconv - 1));
    WHENET_REQUIRE(last.dims.size() == 4 && last.dims[3] >= 1 && last.dims[3] <= 4096, WHENET_EFORMAT,
                   "detector snapshot: " + det_name("dconv%03d/kernel", nconv - 1) + ": not a convolution kernel");
    auto det = std::make_shared<Detector>();
    det->kind = kind;
    det->dtype = det_dtype_;
    det->out_filters = int(last.dims[3]);
    det->table = detector_table(kind, det->out_filters);
    det->convs.resize(det->table.size());
    int ci = 0, bi = 0;
    for (size_t r = 0; r < det->table.size(); ++r) {
        const DetLayer& L = det->table[r];
        if (L.op != DET_CONV) continue;
        const uint32_t k = uint32_t(L.k), cin = uint32_t(L.cin), cout = uint32_t(L.cout);
        const RawTensor& w = need(t, det_name("dconv%03d/kernel", ci), {k, k, cin, cout});
        std::vector<double> scale(cout, 1.0);
        std::vector<float> bias(size_t((L.cout + 31) / 32) * 32, 0.0f);
        if (L.bn) {                                 // folded in float64, Keras' default epsilon
            const std::string bn = det_name("dbn%03d/", bi++);
            const RawTensor& g = need(t, bn + "gamma", {cout});
            const RawTensor& b = need(t, bn + "beta", {cout});
            const RawTensor& m = need(t, bn + "moving_mean", {cout});
            const RawTensor& v = need(t, bn + "moving_variance", {cout});
            for (uint32_t c = 0; c < cout; ++c) {
                scale[c] = double(g.data[c]) / std::sqrt(double(v.data[c]) + 1e-3);
                bias[c] = float(double(b.data[c]) - double(m.data[c]) * scale[c]);
            }
        } else {
            const RawTensor& b = need(t, det_name("dconv%03d/bias", ci), {cout});
            for (uint32_t c = 0; c < cout; ++c) bias[c] = b.data[c];
        }
        DetConv& dc = det->convs[r];
        upload_dconv(dc.w, det->dtype, w.data, scale, L.k, L.cin, L.cout);
        dc.bias.reset(bias.size() * sizeof(float), "detector weights");
        WHENET_HIP_CHECK(hipMemcpy(dc.bias.as<void>(), bias.data(), bias.size() * sizeof(float), hipMemcpyHostToDevice));
        det->num_maps += L.is_output;
        ++ci;
    }
    float lut[256];
    letterbox_float_table(lut);
    det->lut.reset(sizeof(lut));
    WHENET_HIP_CHECK(hipMemcpy(det->lut.as<void>(), lut, sizeof(lut), hipMemcpyHostToDevice));
    WHENET_HIP_CHECK(hipStreamSynchronize(stream_));       // (a replaced detector's forwards are done before its buffers go)
    det_plans_.clear();
    det_ = std::move(det);
}

// the engines of one handle (one device) read the same weight images; plans and graphs are each engine's own
void Engine::share_detector(const Engine& from) {
    DeviceGuard guard(device_);
    WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
    det_plans_.clear();
    det_ = from.det_;
    if (det_) det_dtype_ = det_->dtype;
}

void Engine::require_detector() const {
    WHENET_REQUIRE(det_ != nullptr, WHENET_EINVAL, "no detector is loaded on this handle (whenet_detector_load)");
}

// ------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------
namespace {

void out_dims(const DetLayer& L, int H, int W, int* Ho, int* Wo) {
    if (L.op == DET_POOL) {
        *Ho = L.stride == 2 ? (H + 1) / 2 : H, *Wo = L.stride == 2 ? (W + 1) / 2 : W;
    } else if (L.stride == 2) {
        *Ho = (H - 2) / 2 + 1, *Wo = (W - 2) / 2 + 1;          // top / left pad 1, 'valid' 3x3
    } else {
        *Ho = H, *Wo = W;
    }
}

}  // namespace

// The plan of (n, H, W): every row's size, its activation slot (a slot is free again after the last row that reads it: two
// ping-pong slots plus one per live route / skip tensor), the output maps, the split-K workspace, and the captured forward
// from the input image (img) to the maps.  Activations and the image are sized by the detector's element type.
DetPlan& Engine::detector_plan(int n, int H, int W) {
    const Detector& det = *det_;
    const auto key = std::make_tuple(n, H, W);
    const auto it = det_plans_.find(key);
    if (it != det_plans_.end()) return *it->second;
    if (det_plans_.size() >= 8) {                   // (a video has one size; bound what a size sweep can hold)
        WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
        det_plans_.clear();
    }
    auto plan = std::make_shared<DetPlan>();
    DetPlan& p = *plan;
    p.n = n, p.H = H, p.W = W;
    const size_t R = det.table.size();
    p.rh.resize(R), p.rw.resize(R), p.slot.assign(R, -1);
    std::vector<int> last_use(R, -1);
    size_t slot_bytes = 0, partial_floats = 0;
    for (size_t r = 0; r < R; ++r) {
        const DetLayer& L = det.table[r];
        const int full = L.src1 >= 0 ? L.src1 : L.src0;          // the row that has the consumer's resolution
        const int h = full < 0 ? H : p.rh[size_t(full)], w = full < 0 ? W : p.rw[size_t(full)];
        out_dims(L, h, w, &p.rh[r], &p.rw[r]);
        WHENET_REQUIRE(p.rh[r] >= 1 && p.rw[r] >= 1, WHENET_EINVAL, "detector: input too small");
        for (int s : {L.src0, L.src1, L.skip})
            if (s >= 0) last_use[size_t(s)] = int(r);
        if (!L.is_output) slot_bytes = std::max(slot_bytes, size_t(n) * p.rh[r] * p.rw[r] * L.cout * det_esize(det.dtype));
        if (L.op == DET_CONV) {
            const int splits = dconv_splits(L.k, std::max(L.cin, 16), L.cout, p.rh[r], p.rw[r]);
            if (splits > 1) partial_floats = std::max(partial_floats, size_t(splits) * n * p.rh[r] * p.rw[r] * (size_t((L.cout + 31) / 32) * 32));
        }
    }
    std::vector<int> owner;                         // slot -> row whose output it holds (-1: free)
    int m = 0;
    for (size_t r = 0; r < R; ++r) {
        const DetLayer& L = det.table[r];
        for (int& o : owner)
            if (o >= 0 && last_use[size_t(o)] < int(r)) o = -1;
        if (L.is_output) {
            WHENET_REQUIRE(m < 3, WHENET_EINVAL, "detector: more than three output maps");
            p.gh[m] = p.rh[r], p.gw[m] = p.rw[r];
            p.maps[m].reset(size_t(n) * p.rh[r] * p.rw[r] * L.cout * sizeof(float), "detector output maps");
            ++m;
            continue;
        }
        size_t s = 0;
        while (s < owner.size() && owner[s] >= 0) ++s;
        if (s == owner.size()) {
            owner.push_back(-1);
            p.slots.emplace_back();
            p.slots.back().reset(slot_bytes, "detector activations");
        }
        owner[s] = int(r);
        p.slot[r] = int(s);
    }
    p.img.reset(size_t(n) * H * W * det_kc(det.dtype) * det_esize(det.dtype), "detector activations");
    p.img_f32.reset(size_t(n) * H * W * 3 * sizeof(float), "detector activations");
    p.partial.reset(partial_floats * sizeof(float), "detector activations");

    hipGraph_t graph = nullptr;
    WHENET_HIP_CHECK(hipStreamBeginCapture(stream_, hipStreamCaptureModeRelaxed));
    try {
        enqueue_detector(p, stream_);
    } catch (...) {
        (void)hipStreamEndCapture(stream_, &graph);
        if (graph) (void)hipGraphDestroy(graph);
        throw;
    }
    WHENET_HIP_CHECK(hipStreamEndCapture(stream_, &graph));
    const hipError_t e = hipGraphInstantiate(&p.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) throw Error(WHENET_EHIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
    return *det_plans_.emplace(key, std::move(plan)).first->second;
}

// the launches of one forward, input image -> output maps, on s
void Engine::enqueue_detector(DetPlan& p, hipStream_t s) {
    const Detector& det = *det_;
    int m = 0;
    auto act = [&](int row) { return row < 0 ? p.img.as<void>() : p.slots[size_t(p.slot[size_t(row)])].as<void>(); };
    for (size_t r = 0; r < det.table.size(); ++r) {
        const DetLayer& L = det.table[r];
        const int full = L.src1 >= 0 ? L.src1 : L.src0;
        const int h = full < 0 ? p.H : p.rh[size_t(full)], w = full < 0 ? p.W : p.rw[size_t(full)];
        if (L.op == DET_POOL) {
            launch_dpool(act(L.src0), act(int(r)), det.dtype, p.n, h, w, L.cin, L.stride, s);
            continue;
        }
        DconvArgs a{};
        a.in0 = act(L.src0);
        a.in1 = L.src1 >= 0 ? act(L.src1) : nullptr;
        a.dtype = det.dtype;
        a.w = det.convs[r].w.as<void>();
        a.bias = det.convs[r].bias.as<float>();
        a.skip = L.skip >= 0 ? act(L.skip) : nullptr;
        a.out = L.is_output ? p.maps[m++].as<void>() : act(int(r));
        a.partial = p.partial.as<float>();
        a.n = p.n, a.H = h, a.W = w;
        a.C0 = std::max(L.cin0, det_kc(det.dtype)), a.C1 = L.cin - L.cin0;
        a.Ho = p.rh[r], a.Wo = p.rw[r], a.Cout = L.cout, a.k = L.k, a.stride = L.stride, a.leaky = L.leaky, a.f32_out = L.is_output;
        a.splits = dconv_splits(L.k, std::max(L.cin, 16), L.cout, a.Ho, a.Wo);
        launch_dconv(a, s);
    }
}

namespace {
void check_detector_input(int n, int H, int W) {
    WHENET_REQUIRE(n >= 1 && n <= 16 && H >= 32 && H <= 1024 && W >= 32 && W <= 1024 && H % 32 == 0 && W % 32 == 0, WHENET_EINVAL,
                   "detector: n must be 1..16 and the input sides multiples of 32 in 32..1024");
}
}  // namespace

void Engine::detector_forward(const float* image, int n, int H, int W, float* const* maps) {
    DeviceGuard guard(device_);
    require_detector();
    WHENET_REQUIRE(image != nullptr && maps != nullptr, WHENET_EINVAL, "detector_forward: NULL argument");
    check_detector_input(n, H, W);
    for (int m = 0; m < det_->num_maps; ++m) WHENET_REQUIRE(maps[m] != nullptr, WHENET_EINVAL, "detector_forward: NULL output map");
    DetPlan& p = detector_plan(n, H, W);
    const size_t pixels = size_t(n) * H * W;
    WHENET_HIP_CHECK(hipMemcpyAsync(p.img_f32.as<void>(), image, pixels * 3 * sizeof(float), hipMemcpyHostToDevice, stream_));
    launch_dimage(p.img_f32.as<float>(), nullptr, nullptr, p.img.as<void>(), det_->dtype, pixels, stream_);
    WHENET_HIP_CHECK(hipGraphLaunch(p.exec, stream_));
    for (int m = 0; m < det_->num_maps; ++m)
        WHENET_HIP_CHECK(hipMemcpyAsync(maps[m], p.maps[m].as<void>(), p.maps[m].bytes(), hipMemcpyDeviceToHost, stream_));
    WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
}

// letterbox -> body -> yolo_eval of a frame that is on the device; nothing returns to the host before the selected boxes
int Engine::detect_device(const uint8_t* d_frame, int fh, int fw, int swap_rb, int out_h, int out_w, const float* anchors, int num_anchors,
                          float score_threshold, float iou_threshold, int max_boxes, float* boxes, float* scores, int32_t* classes) {
    check_detector_input(1, out_h, out_w);
    WHENET_REQUIRE(det_->out_filters % 3 == 0 && det_->out_filters / 3 > 5, WHENET_EINVAL,
                   "detect: the loaded detector's outputs are not 3 anchors x (5 + classes) wide");
    WHENET_REQUIRE(anchors != nullptr && boxes != nullptr && scores != nullptr && classes != nullptr, WHENET_EINVAL, "detect: NULL argument");
    DetPlan& p = detector_plan(1, out_h, out_w);
    const uint8_t* d_canvas = enqueue_letterbox(d_frame, fh, fw, swap_rb, out_h, out_w, true, false).first;
    launch_dimage(nullptr, d_canvas, det_->lut.as<float>(), p.img.as<void>(), det_->dtype, size_t(out_h) * out_w, stream_);
    WHENET_HIP_CHECK(hipGraphLaunch(p.exec, stream_));
    const float* feats[3] = {p.maps[0].as<float>(), p.maps[1].as<float>(), p.maps[2].as<float>()};
    return yolo_eval_maps(feats, true, p.gh, p.gw, det_->num_maps, anchors, num_anchors, det_->out_filters / 3 - 5, float(fh), float(fw),
                          score_threshold, iou_threshold, max_boxes, boxes, scores, classes, nullptr, nullptr, nullptr);
}

int Engine::op_detect(const uint8_t* frame, int fh, int fw, int swap_rb, int out_h, int out_w, const float* anchors, int num_anchors,
                      float score_threshold, float iou_threshold, int max_boxes, float* boxes, float* scores, int32_t* classes) {
    DeviceGuard guard(device_);
    require_detector();
    WHENET_REQUIRE(frame != nullptr, WHENET_EINVAL, "op_detect: frame must not be NULL");
    (void)letterbox_plan_layout(fh, fw, out_h, out_w);
    const size_t fbytes = size_t(fh) * fw * 3;
    lb_frame_.grow(fbytes);
    WHENET_HIP_CHECK(hipMemcpyAsync(lb_frame_.as<void>(), frame, fbytes, hipMemcpyHostToDevice, stream_));
    return detect_device(lb_frame_.as<uint8_t>(), fh, fw, swap_rb, out_h, out_w, anchors, num_anchors, score_threshold, iou_threshold,
                         max_boxes, boxes, scores, classes);
}

int Engine::frame_detect(int ticket, int out_h, int out_w, const float* anchors, int num_anchors, float score_threshold,
                         float iou_threshold, int max_boxes, float* boxes, float* scores, int32_t* classes) {
    DeviceGuard guard(device_);
    require_detector();
    Slot& slot = resident_slot(ticket, "frame_detect");
    (void)letterbox_plan_layout(slot.fh, slot.fw, out_h, out_w);
    WHENET_HIP_CHECK(hipStreamWaitEvent(stream_, slot.copied, 0));
    return detect_device(slot.frame.d.as<uint8_t>(), slot.fh, slot.fw, slot.swap_rb, out_h, out_w, anchors, num_anchors, score_threshold,
                         iou_threshold, max_boxes, boxes, scores, classes);
}

// begin -> detect_heads -> collect: what frame_detect + frame_heads do in two steps with the host in between, as ONE enqueue-only
// submission.  The boxes yolo.hip selected stay in yolo_scratch_; headplan.hip turns them into the detections, their windows and
// their crop plans in the slot's buffers; the crop kernel and the forward run over the CAPACITY K = classes x max_boxes (rows
// without a head are zero crops: a crop's result is bitwise independent of the batch and of its position, so head i equals
// the two-step path's); everything comes back with the copies enqueued here.  The letterbox scratch, the plan's activations
// and yolo_scratch_ are one per engine: the next frame's launches are behind this frame's on stream_.  Buffers are allocated
// and graphs captured on the first call for a shape; after that nothing here waits for the device.
void Engine::frame_detect_heads(int ticket, int out_h, int out_w, const float* anchors, int num_anchors, float score_threshold,
                                float iou_threshold, int max_boxes) {
    DeviceGuard guard(device_);
    require_model();
    require_detector();
    Slot& slot = resident_slot(ticket, "frame_detect_heads");
    (void)letterbox_plan_layout(slot.fh, slot.fw, out_h, out_w);
    check_detector_input(1, out_h, out_w);
    WHENET_REQUIRE(det_->out_filters % 3 == 0 && det_->out_filters / 3 > 5, WHENET_EINVAL,
                   "detect: the loaded detector's outputs are not 3 anchors x (5 + classes) wide");
    WHENET_REQUIRE(anchors != nullptr, WHENET_EINVAL, "detect: NULL argument");
    const int num_classes = det_->out_filters / 3 - 5;
    WHENET_REQUIRE(max_boxes >= 1 && max_boxes <= 64 && num_classes * max_boxes <= 64, WHENET_EINVAL,
                   "frame_detect_heads: classes x max_boxes = " + std::to_string(num_classes) + " x " + std::to_string(max_boxes) +
                       " must be 1..64 (every slot is a crop of the forward)");
    const int cap = num_classes * max_boxes;              // (allocations first: nothing is enqueued yet if one of them fails)
    ensure_capacity(cap);
    ensure_slot(slot, cap);
    ensure_slot_frame(slot, size_t(slot.fh) * slot.fw * 3, cap);
    slot.det.h.grow(DetRows(cap).bytes());
    slot.det.d.grow(DetRows(cap).bytes());
    DetPlan& p = detector_plan(1, out_h, out_w);
    WHENET_HIP_CHECK(hipStreamWaitEvent(stream_, slot.copied, 0));
    const uint8_t* d_canvas = enqueue_letterbox(slot.frame.d.as<uint8_t>(), slot.fh, slot.fw, slot.swap_rb, out_h, out_w, true, false).first;
    launch_dimage(nullptr, d_canvas, det_->lut.as<float>(), p.img.as<void>(), det_->dtype, size_t(out_h) * out_w, stream_);
    WHENET_HIP_CHECK(hipGraphLaunch(p.exec, stream_));
    const float* feats[3] = {p.maps[0].as<float>(), p.maps[1].as<float>(), p.maps[2].as<float>()};
    const YoloArgs y = enqueue_yolo_eval(feats, true, p.gh, p.gw, det_->num_maps, anchors, num_anchors, num_classes, float(slot.fh),
                                         float(slot.fw), score_threshold, iou_threshold, max_boxes, false);
    const int K = num_classes * y.max_boxes;              // (max_boxes is cut to the number of boxes the maps hold)
    const DetRows rows(K);
    void* const d_rows = slot.det.d.as<void>();
    HeadPlanArgs a{};
    a.in_boxes = y.out_boxes, a.in_scores = y.out_scores, a.in_count = y.out_count;
    a.num_classes = num_classes, a.max_boxes = y.max_boxes, a.frame_h = slot.fh, a.frame_w = slot.fw;
    a.boxes = rows.boxes(d_rows), a.scores = rows.scores(d_rows), a.classes = rows.classes(d_rows), a.count = rows.count(d_rows);
    a.rects = rows.rects(d_rows), a.valid = rows.valid(d_rows), a.plans = slot.plan.d.as<int32_t>();
    launch_head_plan(a, stream_);
    launch_crop_resize_masked(slot.frame.d.as<uint8_t>(), slot.fw, slot.swap_rb, a.plans, K, a.valid, a.count, slot.in.d.as<uint8_t>(),
                              stream_);
    run_forward(slot.in.d.as<uint8_t>(), K, slot.dev(), stream_);
    WHENET_HIP_CHECK(hipMemcpyAsync(slot.det.h.as<void>(), d_rows, rows.bytes(), hipMemcpyDeviceToHost, stream_));
    copy_results_async(slot.host(), slot.dev(), K, stream_);
    WHENET_HIP_CHECK(hipEventRecord(slot.done, stream_));
    slot.n = K;
    slot.det_cap = K;
    slot.frame_ticket = -1;
    slot.ann_kind = Slot::ANN_DET;
}

// clip_begin -> clip_detect_heads -> collect_clip: frame_detect_heads over the F frames of a clip (demo_video.py:49-63 with the
// next frames in hand).  The letterbox, the selection and the head plans take the frame as a grid dimension, the body runs its
// plan of n = F; the compaction kernel then numbers the slots that hold a head with a window in (frame, detection) order, the
// gathering crop kernel fills forward row r from slot_of_row[r] and the forward runs over max_heads rows instead of the
// capacity F x K.  Every stage is batch-invariant, so slot (f, i) holds the bytes frame_detect_heads returns for frame f alone.
// Allocations and the graph capture come first; after the first call for a shape nothing here waits for the device.
int Engine::clip_detect_heads(int ticket, int out_h, int out_w, const float* anchors, int num_anchors, float score_threshold,
                              float iou_threshold, int max_boxes, int max_heads) {
    DeviceGuard guard(device_);
    require_model();
    require_detector();
    Slot& slot = resident_slot(ticket, "clip_detect_heads", HOLDS_CLIP);
    const int F = slot.clip_f;
    const bool mixed = slot.clip_mixed;                   // frames of their own sizes: the mixed kernels of the size-dependent stages
    if (mixed) check_mixed_geometry("clip_detect_heads", F, slot.clip_fh, slot.clip_fw, out_h, out_w);
    else (void)letterbox_plan_layout(slot.fh, slot.fw, out_h, out_w);
    check_detector_input(F, out_h, out_w);
    WHENET_REQUIRE(det_->out_filters % 3 == 0 && det_->out_filters / 3 > 5, WHENET_EINVAL,
                   "detect: the loaded detector's outputs are not 3 anchors x (5 + classes) wide");
    WHENET_REQUIRE(anchors != nullptr, WHENET_EINVAL, "detect: NULL argument");
    const int num_classes = det_->out_filters / 3 - 5;
    int held = 0;                                         // boxes the maps hold: max_boxes is cut to it, as yolo_eval does
    for (int m = 0; m < det_->num_maps; ++m) held += ((out_h / 32) << m) * ((out_w / 32) << m) * 3;
    WHENET_REQUIRE(max_boxes >= 1, WHENET_EINVAL, "clip_detect_heads: max_boxes must be >= 1");
    const long K_long = long(num_classes) * std::min(max_boxes, held);
    WHENET_REQUIRE(K_long * F <= HEAD_COMPACT_MAX_SLOTS, WHENET_EINVAL,
                   "clip_detect_heads: frames x classes x max_boxes = " + std::to_string(F) + " x " + std::to_string(num_classes) + " x " +
                       std::to_string(std::min(max_boxes, held)) + " must be 1.." + std::to_string(HEAD_COMPACT_MAX_SLOTS));
    const int K = int(K_long);
    if (max_heads == 0) max_heads = std::min(F * K, 256);
    WHENET_REQUIRE(max_heads >= 1 && max_heads <= 256, WHENET_EINVAL,
                   "clip_detect_heads: max_heads = " + std::to_string(max_heads) + " must be 1..256 (the rows of the forward)");
    const ClipRows rows(F, K, max_heads);
    const size_t frame_bytes = size_t(slot.fh) * slot.fw * 3;
    ensure_capacity(max_heads);                           // (allocations first: nothing is enqueued yet if one of them fails)
    ensure_slot(slot, max_heads);
    slot.plan.d.grow(rows.S * CROP_PLAN_INTS * sizeof(int32_t));
    slot.det.h.grow(rows.bytes());
    slot.det.d.grow(rows.bytes());
    DetPlan& p = detector_plan(F, out_h, out_w);
    WHENET_HIP_CHECK(hipStreamWaitEvent(stream_, slot.copied, 0));
    const uint8_t* d_frames = slot.frame.d.as<uint8_t>();
    const uint8_t* d_canvas =
        mixed ? enqueue_letterbox_mixed(d_frames, F, slot.clip_fh, slot.clip_fw, slot.clip_off, slot.swap_rb, out_h, out_w, true, false).first
              : enqueue_letterbox(d_frames, slot.fh, slot.fw, slot.swap_rb, out_h, out_w, true, false, F).first;
    launch_dimage(nullptr, d_canvas, det_->lut.as<float>(), p.img.as<void>(), det_->dtype, size_t(F) * out_h * out_w, stream_);
    WHENET_HIP_CHECK(hipGraphLaunch(p.exec, stream_));
    const float* feats[3] = {p.maps[0].as<float>(), p.maps[1].as<float>(), p.maps[2].as<float>()};
    float shapes[2 * MIXED_MAX_FRAMES] = {};
    HeadPlanSizes sizes{};
    CropFrames crop_frames{};
    for (int f = 0; mixed && f < F; ++f) {
        shapes[2 * f] = float(slot.clip_fh[f]), shapes[2 * f + 1] = float(slot.clip_fw[f]);
        sizes.frame_h[f] = slot.clip_fh[f], sizes.frame_w[f] = slot.clip_fw[f];
        crop_frames.frame_off[f] = slot.clip_off[f], crop_frames.fw[f] = slot.clip_fw[f];
    }
    const YoloArgs y = enqueue_yolo_eval(feats, true, p.gh, p.gw, det_->num_maps, anchors, num_anchors, num_classes, float(slot.fh),
                                         float(slot.fw), score_threshold, iou_threshold, max_boxes, false, F, mixed ? shapes : nullptr);
    WHENET_REQUIRE(num_classes * y.max_boxes == K, WHENET_EINVAL, "clip_detect_heads: the selection's capacity differs from the plan's");
    void* const d_rows = slot.det.d.as<void>();
    HeadPlanArgs a{};
    a.in_boxes = y.out_boxes, a.in_scores = y.out_scores, a.in_count = y.out_count;
    a.num_classes = num_classes, a.max_boxes = y.max_boxes, a.frame_h = slot.fh, a.frame_w = slot.fw, a.frames = F;
    a.boxes = rows.boxes(d_rows), a.scores = rows.scores(d_rows), a.classes = rows.classes(d_rows), a.count = rows.count(d_rows);
    a.rects = rows.rects(d_rows), a.valid = rows.valid(d_rows), a.plans = slot.plan.d.as<int32_t>();
    launch_head_plan(a, stream_, mixed ? &sizes : nullptr);
    launch_head_compact(a.valid, a.count, F, K, max_heads, rows.row(d_rows), rows.slot_of_row(d_rows), rows.rows_used(d_rows),
                        rows.overflow(d_rows), stream_);
    if (mixed)
        launch_crop_resize_gather_mixed(d_frames, crop_frames, slot.swap_rb, a.plans, K, rows.slot_of_row(d_rows), max_heads,
                                        slot.in.d.as<uint8_t>(), stream_);
    else
        launch_crop_resize_gather(d_frames, frame_bytes, slot.fw, slot.swap_rb, a.plans, K, rows.slot_of_row(d_rows), max_heads,
                                  slot.in.d.as<uint8_t>(), stream_);
    run_forward(slot.in.d.as<uint8_t>(), max_heads, slot.dev(), stream_);
    WHENET_HIP_CHECK(hipMemcpyAsync(slot.det.h.as<void>(), d_rows, rows.bytes(), hipMemcpyDeviceToHost, stream_));
    copy_results_async(slot.host(), slot.dev(), max_heads, stream_);
    WHENET_HIP_CHECK(hipEventRecord(slot.done, stream_));
    slot.n = max_heads;
    slot.clip_cap = K;
    slot.clip_heads = max_heads;
    slot.frame_ticket = -1;
    slot.ann_kind = Slot::ANN_CLIP;
    return K;
}

// ------------------------------------------------------------------------------------------
// single layers on caller tensors (float32 in / out, converted on the device): exactly the kernels the body runs
// ------------------------------------------------------------------------------------------
void Engine::op_dconv(const float* in, int n, int H, int W, int cin, const float* in2, int cin2, const float* kernel, const float* bias,
                      int k, int stride, int cout, int leaky, const float* skip, int f32_out, float* out) {
    DeviceGuard guard(device_);
    WHENET_REQUIRE(in && kernel && bias && out, WHENET_EINVAL, "op_dconv: NULL argument");
    WHENET_REQUIRE(n >= 1 && n <= 64 && H >= 1 && W >= 1 && H <= 1024 && W <= 1024 && (k == 1 || k == 3) && (stride == 1 || (stride == 2 && k == 3)) &&
                       cout >= 1 && cout <= 4096 && cin <= 4096 && (cin == 3 || (cin >= 16 && cin % 16 == 0)) &&
                       ((in2 == nullptr && cin2 == 0) || (in2 != nullptr && cin != 3 && cin2 >= 16 && cin2 % 16 == 0 && cin2 <= 4096 && H % 2 == 0 && W % 2 == 0)) &&
                       (f32_out ? skip == nullptr : cout % 16 == 0) && (stride == 1 || (H >= 2 && W >= 2)),
                   WHENET_EINVAL, "op_dconv: unsupported shape (k 1 / 3, stride 2 with k 3 only, Cin 3 or a multiple of 16, binary16 outputs with "
                                  "Cout a multiple of 16, a second source only on even sides)");
    DetLayer L{};
    L.op = DET_CONV, L.k = k, L.stride = stride;
    int Ho = 0, Wo = 0;
    out_dims(L, H, W, &Ho, &Wo);
    const size_t N = size_t(n), in_elems = in2 ? N * (H / 2) * (W / 2) * cin : N * H * W * cin, in2_elems = in2 ? N * H * W * cin2 : 0;
    const size_t out_elems = N * Ho * Wo * cout;
    const int ctot = cin + cin2;
    const int dtype = det_dtype_;                          // the kernels of the handle's "detector_dtype"
    const size_t es = det_esize(dtype);
    std::vector<float> biasp(size_t((cout + 31) / 32) * 32, 0.0f);
    std::copy(bias, bias + cout, biasp.begin());
    TempBufs tmp;
    float* d_f32 = static_cast<float*>(tmp.get(std::max({in_elems, in2_elems, out_elems}) * sizeof(float)));
    void* d_in = tmp.get(std::max(in_elems, N * H * W * det_kc(dtype)) * es);
    void* d_in2 = in2 ? tmp.get(in2_elems * es) : nullptr;
    void* d_skip = skip ? tmp.get(out_elems * es) : nullptr;
    void* d_out = tmp.get(out_elems * sizeof(float));
    DeviceBuffer d_w;
    upload_dconv(d_w, dtype, kernel, std::vector<double>(size_t(cout), 1.0), k, ctot, cout);
    float* d_b = static_cast<float*>(tmp.get(biasp.size() * sizeof(float)));
    WHENET_HIP_CHECK(hipMemcpyAsync(d_b, biasp.data(), biasp.size() * sizeof(float), hipMemcpyHostToDevice, stream_));
    WHENET_HIP_CHECK(hipMemcpyAsync(d_f32, in, in_elems * sizeof(float), hipMemcpyHostToDevice, stream_));
    if (cin == 3) launch_dimage(d_f32, nullptr, nullptr, d_in, dtype, N * H * W, stream_);       // the body's own input stage
    else launch_f32_to_act(d_f32, d_in, in_elems, dtype, stream_);
    if (in2) {
        WHENET_HIP_CHECK(hipMemcpyAsync(d_f32, in2, in2_elems * sizeof(float), hipMemcpyHostToDevice, stream_));
        launch_f32_to_act(d_f32, d_in2, in2_elems, dtype, stream_);
    }
    if (skip) {
        WHENET_HIP_CHECK(hipMemcpyAsync(d_f32, skip, out_elems * sizeof(float), hipMemcpyHostToDevice, stream_));
        launch_f32_to_act(d_f32, d_skip, out_elems, dtype, stream_);
    }
    DconvArgs a{};
    a.dtype = dtype;
    a.in0 = d_in, a.in1 = d_in2, a.w = d_w.as<void>(), a.bias = d_b, a.skip = d_skip, a.out = d_out;
    a.n = n, a.H = H, a.W = W, a.C0 = std::max(cin, det_kc(dtype)), a.C1 = cin2;
    a.Ho = Ho, a.Wo = Wo, a.Cout = cout, a.k = k, a.stride = stride, a.leaky = leaky != 0, a.f32_out = f32_out != 0;
    a.splits = dconv_splits(k, std::max(cin, 16) + cin2, cout, Ho, Wo);
    a.partial = static_cast<float*>(tmp.get(dconv_partial_floats(a) * sizeof(float)));
    launch_dconv(a, stream_);
    if (f32_out) {
        WHENET_HIP_CHECK(hipMemcpyAsync(out, d_out, out_elems * sizeof(float), hipMemcpyDeviceToHost, stream_));
    } else {
        launch_act_to_f32(d_out, d_f32, out_elems, dtype, stream_);
        WHENET_HIP_CHECK(hipMemcpyAsync(out, d_f32, out_elems * sizeof(float), hipMemcpyDeviceToHost, stream_));
    }
    WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
}

void Engine::op_dpool(const float* in, int n, int H, int W, int c, int stride, float* out) {
    DeviceGuard guard(device_);
    WHENET_REQUIRE(in && out, WHENET_EINVAL, "op_dpool: NULL argument");
    WHENET_REQUIRE(n >= 1 && n <= 64 && H >= 1 && W >= 1 && H <= 1024 && W <= 1024 && c >= 8 && c % 8 == 0 && c <= 4096 && (stride == 1 || stride == 2),
                   WHENET_EINVAL, "op_dpool: stride 1 or 2, channels a multiple of 8");
    DetLayer L{};
    L.op = DET_POOL, L.stride = stride;
    int Ho = 0, Wo = 0;
    out_dims(L, H, W, &Ho, &Wo);
    const size_t in_elems = size_t(n) * H * W * c, out_elems = size_t(n) * Ho * Wo * c;
    TempBufs tmp;
    float* d_f32 = static_cast<float*>(tmp.get(in_elems * sizeof(float)));
    const int dtype = det_dtype_;
    void* d_in = tmp.get(in_elems * det_esize(dtype));
    void* d_out = tmp.get(out_elems * det_esize(dtype));
    WHENET_HIP_CHECK(hipMemcpyAsync(d_f32, in, in_elems * sizeof(float), hipMemcpyHostToDevice, stream_));
    launch_f32_to_act(d_f32, d_in, in_elems, dtype, stream_);
    launch_dpool(d_in, d_out, dtype, n, H, W, c, stride, stream_);
    launch_act_to_f32(d_out, d_f32, out_elems, dtype, stream_);
    WHENET_HIP_CHECK(hipMemcpyAsync(out, d_f32, out_elems * sizeof(float), hipMemcpyDeviceToHost, stream_));
    WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
}

}  // namespace whenet
