#include "engine_internal.h"

#include <mutex>

#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <cstring>

namespace whenet {

using namespace detail;

// ------------------------------------------------------------------------------------------
// construction / weights
// ------------------------------------------------------------------------------------------
void* Engine::upload_bytes(const void* p, size_t nbytes) {
    weight_allocs_.emplace_back();
    weight_allocs_.back().reset(nbytes);
    void* d = weight_allocs_.back().as<void>();
    if (nbytes) WHENET_HIP_CHECK(hipMemcpy(d, p, nbytes, hipMemcpyHostToDevice));
    return d;
}

template <typename T> T* Engine::upload(const std::vector<T>& v) {
    return static_cast<T*>(upload_bytes(v.data(), v.size() * sizeof(T)));
}

DevPw Engine::upload_pw(const HostPw& h) {
    DevPw d;
    d.K = h.K;
    d.N = h.N;
    d.KS = h.KS;
    d.NTILES = h.NTILES;
    d.wp = upload_bytes(h.packed.data(), h.packed.size());
    if (!h.packed_split.empty()) {
        d.wps = upload_bytes(h.packed_split.data(), h.packed_split.size());
        d.KSs = h.KS_split;
        d.wsi = h.wsi;
    }
    d.wdense = upload(h.dense);
    d.bias = upload(h.bias);
    return d;
}

Engine::Engine(const void* snapshot, size_t nbytes, int device_id, int dtype)
    : device_(device_id), dtype_(dtype == WHENET_F32S ? WHENET_F32 : dtype), split_(dtype == WHENET_F32S) {
    // host-side preparation first: a malformed snapshot is reported as such even on a box
    // without a GPU
    HostModel m = build_host_model(parse_snapshot(snapshot, nbytes), dtype_, split_);
    params_backbone_ = m.params_backbone;
    params_heads_ = m.params_heads;
    n_tensors_ = m.n_tensors;

    open_device(device_id);
    DeviceGuard guard(device_);
    has_model_ = true;

    d_lut_ = static_cast<float*>(upload_bytes(&m.lut[0][0], sizeof(m.lut)));
    d_stem_w_ = upload(m.stem_w);
    d_stem_b_ = upload(m.stem_b);
    {
        StemDwTable t;
        build_stemdw_table(m.stem_w.data(), &m.lut[0][0], &t);
        d_stemdw_tab_ = static_cast<StemDwTable*>(upload_bytes(&t, sizeof(t)));
    }
    for (const HostBlock& hb : m.blocks) {
        DevBlock b;
        b.spec = hb.spec;
        if (hb.spec.has_expand()) b.expand = upload_pw(hb.expand);
        b.dw.k = hb.dw.k;
        b.dw.C = hb.dw.C;
        b.dw.w = upload(hb.dw.w);
        b.dw.bias = upload(hb.dw.bias);
        b.dw.plan = plan_dw(dtype_, hb.spec.k, hb.spec.s, hb.spec.h_in, hb.spec.h_out, hb.dw.C);
        b.se.C = hb.se.C;
        b.se.R = hb.se.R;
        b.se.w1t = upload(hb.se.w1t);
        b.se.b1 = upload(hb.se.b1);
        b.se.w2 = upload(hb.se.w2);
        b.se.w2c = upload(hb.se.w2c);
        b.se.b2 = upload(hb.se.b2);
        if (split_ && !hb.se.excite.packed_split.empty()) {
            b.se.w2p = upload_bytes(hb.se.excite.packed_split.data(), hb.se.excite.packed_split.size());
            b.se.KSr = hb.se.excite.KS_split;
            b.se.w2_wsi = hb.se.excite.wsi;
        } else if (dtype_ == WHENET_F16 && !hb.se.excite.packed.empty()) {
            b.se.w2p = upload_bytes(hb.se.excite.packed.data(), hb.se.excite.packed.size());
            b.se.KSr = hb.se.excite.KS;
        }
        b.project = upload_pw(hb.project);
        partial_per_crop_ = std::max(partial_per_crop_, size_t(b.dw.plan.ntiles()) * b.dw.C);
        if (hb.spec.has_expand()) {
            b.fplan = plan_front(dtype_, hb.spec.k, hb.spec.s, hb.spec.h_in, hb.spec.h_out, hb.dw.C);
            partial_per_crop_ = std::max(partial_per_crop_, size_t(b.fplan.ntiles()) * b.dw.C);
            // blocks whose front kernel applies the SE reduce conv write [tiles][chunks][RP] partial vectors: with
            // narrow chunks that exceeds [tiles][C] (C = 1152, 32-channel chunks: 36 x 48 = 1728 floats per tile)
            partial_per_crop_ = std::max(partial_per_crop_, size_t(b.fplan.ntiles()) * size_t(b.fplan.chunks) *
                                                                size_t(se_padded_r(b.se.R)));
            if (dtype_ == WHENET_F16) {
                // f16: the same stage with the depthwise taps on the matrix cores (front2.hip) where that kernel is the
                // faster one; its Toeplitz image of the depthwise kernel is built once here
                b.f2plan = plan_front2(hb.spec.k, hb.spec.s, hb.spec.h_in, hb.spec.h_out, hb.dw.C);
                b.f2_preferred = front2_preferred(hb.spec.k, hb.spec.s, hb.spec.h_in, hb.dw.C);
                b.dw.wt = upload(pack_dw_toeplitz(hb.dw.w, hb.spec.k, hb.spec.s, hb.dw.C, b.f2plan.xs));
                partial_per_crop_ = std::max(partial_per_crop_, size_t(b.f2plan.ntiles()) * b.dw.C);
                partial_per_crop_ = std::max(partial_per_crop_, size_t(b.f2plan.ntiles()) * size_t(b.f2plan.chunks) *
                                                                    size_t(se_padded_r(b.se.R)));
            }
            if (split_ && front2s_supported(hb.spec.k, hb.spec.s, hb.spec.h_in, hb.spec.cin)) {
                // f32s: the same stage with both convolutions on the matrix cores (front2s.hip, round 6)
                b.f2s_supported = true;
                b.f2splan = plan_front2s(hb.spec.k, hb.spec.s, hb.spec.h_in, hb.spec.h_out, hb.dw.C, &b.f2s_tm);
                b.f2s_preferred = front2s_preferred(hb.spec.k, hb.spec.s, hb.spec.h_in, hb.dw.C);
                b.dw.wts = upload(pack_dw_toeplitz_s(hb.dw.w, hb.spec.k, hb.spec.s, hb.dw.C, b.f2s_tm, &b.dw.wts_wsi));
                partial_per_crop_ = std::max(partial_per_crop_, size_t(b.f2splan.ntiles()) * size_t(b.f2splan.chunks) *
                                                                    size_t(se_padded_r(b.se.R)));
            }
            // the 7 x 7 blocks, both dtypes: a group of crops per workgroup (front7.hip); f16: its Toeplitz image is group-aligned
            b.f7_supported = front7_supported(hb.spec.k, hb.spec.s, hb.spec.h_in, hb.spec.cin);
            if (b.f7_supported) {
                if (dtype_ == WHENET_F16) b.dw.wt7 = upload(pack_dw_toeplitz(hb.dw.w, hb.spec.k, 1, hb.dw.C, 4 - hb.spec.k / 2));
                b.f7_chunks = front7_plan_for(dtype_, hb.spec.cin, hb.dw.C, 64).chunks;
                partial_per_crop_ = std::max(partial_per_crop_, size_t(b.f7_chunks) * size_t(se_padded_r(b.se.R)));
            }
        }
        if (mb7_supported(dtype_, hb.spec.k, hb.spec.s, hb.spec.h_in, hb.spec.cin, hb.dw.C, hb.se.R, hb.spec.cout, hb.spec.has_skip())) {
            // f16, blocks 13-16: the whole block as one launch (mb7.hip, round 6) -- tap sequences and binary16 squeeze-excite kernels
            std::vector<half_t> w1p, w2p;
            pack_mb7_se(hb.se.w1t, hb.se.w2, hb.se.C, hb.se.R, &w1p, &w2p);
            b.mb7.wds = upload(pack_mb7_taps(hb.dw.w, hb.spec.k, hb.dw.C));
            b.mb7.w1p = upload(w1p);
            b.mb7.w2p = upload(w2p);
            b.mb7.ok = true;
        }
        blocks_.push_back(b);
    }
    head_ = upload_pw(m.head);
    fold12_pw_ = upload_pw(m.fold12);
    d_fold12_w32_ = upload(m.fold12_w32);
    d_dense_w_ = upload(m.dense_w);
    d_dense_b_ = upload(m.dense_b);
    WHENET_HIP_CHECK(hipDeviceSynchronize());

    const size_t es = esz();
    const size_t per_crop[A_COUNT] = {X_ELEMS * es, X_ELEMS * es, E_ELEMS * es, D_ELEMS * es, HC_ELEMS * es,
                                      partial_per_crop_ * sizeof(float), GATE_ELEMS * sizeof(float), sizeof(unsigned), IN_BYTES,
                                      3 * sizeof(float), 3 * sizeof(int32_t), N_LOGITS * sizeof(float)};
    for (int i = 0; i < A_COUNT; ++i) arena_[i].per_crop = per_crop[i];
}

void Engine::open_device(int device_id) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        throw Error(WHENET_ENODEV, std::string("no HIP device visible (") + hipGetErrorString(e) +
                                       "); libwhenet_hip has no CPU fallback");
    WHENET_REQUIRE(device_id >= 0 && device_id < count, WHENET_ENODEV,
                   "device_id " + std::to_string(device_id) + " out of range (" + std::to_string(count) + " devices)");
    DeviceGuard guard(device_id);
    WHENET_HIP_CHECK(hipGetDeviceProperties(&prop_, device_id));
    WHENET_REQUIRE(std::strstr(prop_.gcnArchName, "gfx950") != nullptr, WHENET_ENODEV,
                   std::string("device is ") + prop_.gcnArchName + "; this library carries gfx950 code only");
    num_cus_ = prop_.multiProcessorCount;

    WHENET_HIP_CHECK(hipStreamCreateWithFlags(stream_.put(), hipStreamNonBlocking));
    // Only the main stream exists up front: the runtime places a new stream on its least-loaded
    // hardware queue (4 of them), so streams are created in the order concurrency needs them -- the
    // main streams of the engines of one handle, then sub-batch lanes / the copy stream on first use --
    // instead of nine per engine, most of them idle ballast that skews that placement.
    fork_ev_.create();
    join_ev_.resize(MAX_LANES - 1);
    for (Event& ev : join_ev_) ev.create();
}

// A handle without a network: what whenet_yolo_eval / whenet_op_crop_resize need (device, stream, scratch).
Engine::Engine(int device_id) : device_(device_id), dtype_(WHENET_F32) { open_device(device_id); }

void Engine::require_model() const {
    WHENET_REQUIRE(has_model_, WHENET_EINVAL, "this handle was created without a network (whenet_create_postproc)");
}

// What has an order is done here: nothing is in flight and no graph refers to a buffer when the members go.  They free themselves
// after this body, on the device it selected: buffers and events first, the streams last (engine.h declares them in that order).
Engine::~Engine() {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
    if (copy_stream_) (void)hipStreamSynchronize(copy_stream_);
    for (hipStream_t st : lane_streams_) (void)hipStreamSynchronize(st);
    drop_graphs();
}

void Engine::set_option(const std::string& key, long value) {
    DeviceGuard guard(device_);
    if (key == "graph") {
        use_graph_ = value != 0;
        return;
    } else if (key == "pw_impl") {
        WHENET_REQUIRE(value == 0 || value == 1, WHENET_EINVAL, "pw_impl must be 0 (MFMA) or 1 (check kernel)");
        pw_impl_ = int(value);
    } else if (key == "fuse_front") {
        fuse_front_ = value != 0;
    } else if (key == "se_fuse") {
        WHENET_REQUIRE(value >= 0 && value <= 3, WHENET_EINVAL,
                       "se_fuse must be 0 (never), 1 (where the prologue form pays, default), 2 (prologue form on every block) or 3 (1 + the matrix-core form on blocks 7-16)");
        se_fuse_ = int(value);
    } else if (key == "front_impl") {
        WHENET_REQUIRE(value >= 0 && value <= 2, WHENET_EINVAL,
                       "front_impl must be 0 (front.hip everywhere), 1 (per layer, default) or 2 (front2.hip / front2s.hip wherever they exist)");
        front_impl_ = int(value);
    } else if (key == "f2s_mask") {
        // probes: bit i set = block i runs front2s.hip (f32s handles, front_impl = 1); -1 = the measured per-layer table
        WHENET_REQUIRE(value >= -1 && value < (1 << 17), WHENET_EINVAL, "f2s_mask must be -1 or a bit mask of blocks 2..12");
        f2s_mask_ = int(value);
    } else if (key == "head_fuse") {
        head_fuse_ = value != 0;
    } else if (key == "concurrent") {
        xcd_always_ = value != 0;
    } else if (key == "xcd_map") {
        WHENET_REQUIRE(value >= 0 && value <= 7, WHENET_EINVAL, "xcd_map must be a bit mask 0..7 (1 = front / front2, 2 = front7, 4 = head7)");
        xcd_map_ = int(value);
    } else if (key == "mb7") {
        mb7_ = value != 0;
    } else if (key == "front7") {
        front7_ = value != 0;
    } else if (key == "fold12") {
        fold12_ = value != 0;
    } else if (key == "front2_static") {
        WHENET_REQUIRE(value == 0 || value == 1, WHENET_EINVAL, "front2_static must be 0 (runtime tile geometry everywhere) or 1 (per layer, default)");
        front2_static_ = value != 0;
    } else if (key == "front_static") {
        WHENET_REQUIRE(value == 0 || value == 1, WHENET_EINVAL, "front_static must be 0 (runtime tile geometry everywhere) or 1 (per layer, default)");
        front_static_ = value != 0;
    } else if (key == "pw_static") {
        WHENET_REQUIRE(value == 0 || value == 1, WHENET_EINVAL, "pw_static must be 0 (runtime layer shapes everywhere) or 1 (per layer, default)");
        pw_static_ = value != 0;
    } else if (key == "stem_fuse") {
        stem_fuse_ = value != 0;
    } else if (key == "act_layout") {
        WHENET_REQUIRE(value >= 0 && value <= 2, WHENET_EINVAL,
                       "act_layout must be 0 (NHWC everywhere), 1 (16-channel blocks per layer, default) or 2 (16-channel blocks wherever supported)");
        act_layout_ = int(value);
    } else if (key == "poison") {
        poison_ = value != 0;
        return;
    } else if (key == "lanes" || key == "device_lanes") {
        // "lanes": every forward; "device_lanes" (set by the handle's "inflight" option): the asynchronous device-side
        // entry points only -- a blocking host forward keeps host_lanes_
        WHENET_REQUIRE(value >= 1 && value <= MAX_LANES, WHENET_EINVAL, "lanes must be 1..8");
        lanes_ = int(value);
        if (key == "lanes") host_lanes_ = int(value);
    } else if (key == "split_heads") {
        split_heads_ = value != 0;
    } else if (key == "lane_graphs") {
        lane_graphs_ = value != 0;
    } else if (key == "pw_staged") {
        pw_staged_ = value != 0;
    } else if (key == "split_pw") {
        WHENET_REQUIRE(split_ || value == 0, WHENET_EINVAL, "split_pw: the handle was not created as WHENET_F32S");
        split_pw_ = value != 0;
    } else if (key == "detector_dtype") {
        WHENET_REQUIRE(value == 0 || value == 1, WHENET_EINVAL, "detector_dtype must be 0 (binary16 storage, default) or 1 (float32)");
        const int dtype = value == 1 ? WHENET_F32 : WHENET_F16;
        WHENET_REQUIRE(det_ == nullptr || dtype == det_dtype_, WHENET_EINVAL,
                       "detector_dtype: a detector is attached and its weights were packed when it was loaded: set the option on a "
                       "handle without a detector, then load again");
        det_dtype_ = dtype;
        return;
    } else if (key == "host_pinned_max") {
        WHENET_REQUIRE(value >= 0 && value <= 4096, WHENET_EINVAL, "host_pinned_max must be 0..4096");
        sync();
        host_pinned_max_ = int(value);
        return;
    } else if (key == "se_fuse_tiny") {
        WHENET_REQUIRE(value >= 0 && value <= 64, WHENET_EINVAL, "se_fuse_tiny must be 0..64");
        se_fuse_tiny_ = int(value);
    } else if (key == "letterbox_cache") {
        // entries of the letterbox geometry cache (engine.h).  The entries go: nothing that reads their tables may be queued.
        WHENET_REQUIRE(value >= 1 && value <= 32, WHENET_EINVAL, "letterbox_cache must be 1..32");
        sync();
        lb_cache_.clear();
        lb_cache_cap_ = int(value);
        return;
    } else if (key == "jpeg_entropy") {
        WHENET_REQUIRE(value >= 0 && value <= 2, WHENET_EINVAL, "jpeg_entropy must be 0 (an interval per lane), 1 (segmented) or 2 (auto, default)");
        jpeg_entropy_ = int(value);
        return;
    } else if (key == "jpeg_progressive") {
        WHENET_REQUIRE(value == 0 || value == 1, WHENET_EINVAL, "jpeg_progressive must be 0 (SOF2 streams are refused, default) or 1 (they are decoded)");
        jpeg_progressive_ = int(value);
        return;
    } else if (key == "jpeg_layouts") {
        WHENET_REQUIRE(value == 0 || value == 1, WHENET_EINVAL,
                       "jpeg_layouts must be 0 (4:4:0 / 4:1:1 / 4:1:0 and SOF1 streams are refused, default) or 1 (they are decoded)");
        jpeg_layouts_ = int(value);
        return;
    } else if (key == "jpeg_orient") {
        WHENET_REQUIRE(value == 0 || value == 1, WHENET_EINVAL,
                       "jpeg_orient must be 0 (the EXIF orientation is ignored, default) or 1 (single streams are decoded upright)");
        jpeg_orient_ = int(value);
        return;
    } else if (key == "jpeg_prog_levels") {
        WHENET_REQUIRE(value == 0 || value == 1, WHENET_EINVAL, "jpeg_prog_levels must be 1 (a launch per level, default) or 0 (a launch per scan)");
        jpeg_prog_levels_ = int(value);
        return;
    } else if (key == "jpeg_rule") {
        WHENET_REQUIRE(jpeg_rule_ok(value), WHENET_EINVAL, "jpeg_rule must be 0 (the project's own rule, default) or 1 (libjpeg's bytes)");
        jpeg_rule_ = int(value);
        return;
    } else if (key == "jpeg_seg_lanes") {
        WHENET_REQUIRE(value == 0 || value == 16 || value == 32 || value == 64, WHENET_EINVAL, "jpeg_seg_lanes must be 0 (default), 16, 32 or 64");
        jpeg_seg_lanes_ = int(value);
        return;
    } else if (key == "jpeg_seg_bytes") {
        WHENET_REQUIRE(jpeg_seg_bytes_ok(value), WHENET_EINVAL, "jpeg_seg_bytes must be a power of two in 4..4096");
        jpeg_seg_bytes_ = int(value);
        return;
    } else if (key == "host_lanes") {
        WHENET_REQUIRE(value >= 1 && value <= MAX_LANES, WHENET_EINVAL, "host_lanes must be 1..8");
        host_lanes_ = int(value);
        return;
    } else if (key == "min_lane_crops") {
        WHENET_REQUIRE(value >= 1, WHENET_EINVAL, "min_lane_crops must be >= 1");
        min_lane_crops_ = int(value);
    } else if (key == "repeat") {
        WHENET_REQUIRE(value >= 1 && value <= 16, WHENET_EINVAL, "repeat must be 1..16");
        repeat_ = int(value);
    } else {
        throw Error(WHENET_EINVAL, "unknown option '" + key + "'");
    }
    // every key that did not return above changes what a forward enqueues: nothing in flight, no graph of the old schedule
    // ("graph", "poison", "host_lanes" and "host_pinned_max" return early: they are read per call and no graph depends on them)
    sync();
    drop_graphs();
}

void Engine::get_info(whenet_info_t* out) const {
    std::memset(out, 0, sizeof(*out));
    out->abi_version = WHENET_ABI_VERSION;
    out->dtype = dtype_;
    out->device_id = device_;
    out->compute_units = num_cus_;
    out->params_backbone = params_backbone_;
    out->params_heads = params_heads_;
    out->n_tensors = n_tensors_;
    {
        // stem + per block {expand, dw | front} {se} project + head conv + heads: the launches enqueue_block() issues
        int k = 1 + 2;
        for (const DevBlock& b : blocks_) {
            const BlockSchedule bs = block_schedule(b);
            if (bs.use_mb7) { k += 1; continue; }       // the whole block is one launch (mb7.hip)
            k += bs.fused ? 1 : (b.spec.has_expand() ? 2 : 1);
            k += bs.se_fused ? 1 : 2;                   // project alone when it computes the gate itself
        }
        if (fold12_active()) k -= 1;                    // block 1's project launch
        if (stem_fuse_active()) k -= 1;                 // the stem conv runs inside block 1's depthwise kernel
        out->n_kernels_per_forward = k;
    }
    out->macs_per_crop = 384857312;
    out->arena_bytes = int64_t(arena_bytes_);
    out->capacity = cap_;
    out->graph_enabled = use_graph_ ? 1 : 0;
    copy_name(out->device_name, sizeof(out->device_name), prop_.name);
    copy_name(out->arch, sizeof(out->arch), prop_.gcnArchName);
}

// ------------------------------------------------------------------------------------------
// arena
// ------------------------------------------------------------------------------------------
void Engine::drop_graphs() {
    for (auto& kv : graphs_) (void)hipGraphExecDestroy(kv.second);
    graphs_.clear();
}

void Engine::release_arena() {
    for (ArenaBuf& a : arena_) a.buf.release();
    cap_ = 0;
    arena_bytes_ = 0;
}

void Engine::ensure_capacity(int n) {
    WHENET_REQUIRE(n >= 1, WHENET_EINVAL, "n must be >= 1");
    if (n <= cap_) return;
    WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
    drop_graphs();
    release_arena();
    const size_t N = size_t(n);
    size_t total = 0;
    for (ArenaBuf& a : arena_) {
        const hipError_t e = a.buf.try_reset(N * a.per_crop);
        if (e != hipSuccess) {
            release_arena();
            throw Error(WHENET_ENOMEM, "activation arena for n=" + std::to_string(n) + ": " + hipGetErrorString(e));
        }
        total += a.buf.bytes();
    }
    // (on the engine's OWN stream, and complete before any forward is enqueued: hipMemset runs on the null stream, which
    //  the engine's non-blocking streams do not wait for -- with other engines keeping the GPU busy it used to land in
    //  the middle of this engine's first heads kernel and leave the per-crop ticket counters off by one for good)
    WHENET_HIP_CHECK(hipMemsetAsync(arena_[A_HCOUNT].buf.as<void>(), 0, N * sizeof(unsigned), stream_));
    WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
    cap_ = n;
    arena_bytes_ = total;
}

// ------------------------------------------------------------------------------------------
// the launch schedule
// ------------------------------------------------------------------------------------------
namespace {

struct Rec {
    LaunchRecorder* rec;
    hipStream_t s;
    int repeat = 1;      // debug option "repeat": issue every (idempotent) launch this many times
    template <typename F>
    void operator()(const std::string& layer, const char* kind, const std::string& kernel, double bytes, double flops,
                    F&& fn) {
        if (!rec) {
            for (int i = 0; i < repeat; ++i) fn();
            return;
        }
        if (rec->first_pass) {
            LaunchRecorder::Entry e;
            e.layer = layer;
            e.kind = kind;
            e.kernel = kernel;
            e.bytes = bytes;
            e.flops = flops;
            e.stop.create(hipEventDefault);
            rec->entries.push_back(std::move(e));
        }
        LaunchRecorder::Entry& e = rec->entries.at(rec->cursor++);
        fn();
        WHENET_HIP_CHECK(hipEventRecord(e.stop, s));     // ONE event between consecutive launches
    }
};

}  // namespace

// Block 1's project (linear) and block 2's expand are one affine map of block 1's gated depthwise output
// (snapshot.cpp builds its weights): with front2.hip on block 2, block 1 stops after its squeeze-excite and block 2's
// front kernel reads the 112 x 112 x 32 depthwise output directly, scaling its copy of the weights by the crop's gate.
// One launch and 77 MB of HBM traffic per 64 crops less; block 1's 16-channel output no longer exists (nothing else
// reads it: block 2 has no skip).
// Which kernels a block runs (options fuse_front / front_impl / se_fuse / pw_impl and the per-layer tables): ONE statement of
// it, used by enqueue_block() and by get_info()'s launch count.
Engine::BlockSchedule Engine::block_schedule(const DevBlock& b, int n) const {
    BlockSchedule r;
    r.fused = fuse_front_ && b.spec.has_expand() && pw_impl_ == 0;
    r.use_f7 = r.fused && front_impl_ == 1 && front7_ && b.f7_supported;
    // round 6: blocks 13-16 of an f16 handle as ONE launch (mb7.hip): one workgroup per crop, every intermediate tensor in LDS
    r.use_mb7 = r.use_f7 && mb7_ && dtype_ == WHENET_F16 && b.mb7.ok;
    r.use_f2 = r.fused && !r.use_f7 && dtype_ == WHENET_F16 && (front_impl_ == 2 || (front_impl_ == 1 && b.f2_preferred));
    const bool f2s_pick = f2s_mask_ >= 0 ? ((f2s_mask_ >> b.spec.index) & 1) != 0 : b.f2s_preferred;     // (option "f2s_mask": probes)
    r.use_f2s = r.fused && !r.use_f7 && split_ && split_pw_ && b.f2s_supported && b.expand.wps != nullptr &&
                (front_impl_ == 2 || (front_impl_ == 1 && f2s_pick));
    r.se_in_front = r.fused;                 // the front kernels apply the SE reduce conv to their channel sums
    r.se_ntiles = r.use_f7 ? 1 : (r.use_f2 ? b.f2plan.ntiles() : (r.use_f2s ? b.f2splan.ntiles() : (r.fused ? b.fplan.ntiles() : b.dw.plan.ntiles())));
    r.se_chunks = r.use_f7 ? b.f7_chunks : (r.use_f2 ? b.f2plan.chunks : (r.use_f2s ? b.f2splan.chunks : b.fplan.chunks));
    const bool se_pays = b.project.K < 320 && r.se_ntiles * r.se_chunks <= 24;
    // option "se_fuse_tiny": chains of at most that many crops are launch-bound (B=1: 46-49 launches x ~8 us), so every launch
    // saved pays -- EXCEPT on the 7 x 7 blocks (K = 1152), whose project workgroups would each pull the whole 221 KB excite
    // kernel: se_fuse=2 on all blocks measured 451 us against 420 us at B=1 (round 5).  Blocks 2-12 fuse; same bits either way.
    const bool tiny = !single_stage_call_ && n > 0 && n <= se_fuse_tiny_ && b.project.K < 1152;
    // option se_fuse = 3 (round 6): as 1, plus the deep contractions (blocks 7 - 16): their LDS-staged split-K project GEMM computes the
    // gate of each wave's own k-groups on the matrix cores (pw.hip GM = 3) -- f16 and f32s handles.  Ten launches fewer and SLOWER:
    // every project workgroup pulls the 110 KB excite image through a CU that already fetches at its ~55 GB/s limit (f16, 64 crops:
    // project 12.0 -> 17 us on 14x14, 13.1 -> 21.8 us on 7x7, against a 6.6 - 7.4 us squeeze-excite launch; B = 1: 288 -> 298 us;
    // line 162 -> 157 k crops/s; profiles/r06/se_mfma_ab.txt).  Not the default.
    r.se_mfma = r.se_in_front && pw_impl_ == 0 && se_fuse_ == 3 && pw_staged_ && b.project.K >= 320 && b.se.w2p != nullptr &&
                (dtype_ == WHENET_F16 || (split_ && split_pw_));
    r.se_fused = r.se_in_front && pw_impl_ == 0 && (se_fuse_ == 2 || r.se_mfma || ((se_fuse_ == 1 || se_fuse_ == 3) && (se_pays || tiny)));
    return r;
}

bool Engine::fold12_active() const {
    if (!(fold12_ && fuse_front_ && pw_impl_ == 0 && blocks_.size() >= 2)) return false;
    if (dtype_ == WHENET_F16) return front_impl_ == 2 || (front_impl_ == 1 && blocks_[1].f2_preferred);
    // f32s (round 6): front.hip's split form takes the gate on its float32 operand; the exact-f32 form does not fold (its expand is
    // matrix-pipe bound: doubling the contraction costs more than block 1's project launch saves)
    const BlockSchedule b2 = block_schedule(blocks_[1]);
    return split_ && split_pw_ && fold12_pw_.wps != nullptr && b2.fused && !b2.use_f2s && !b2.use_f7;
}

// The stem's output is read by block 1's depthwise conv only (block 1 has no expand conv and no skip): for handles fed
// uint8 crops the two are one kernel (stemdw.hip) when block 1's depthwise tile plan is the one that kernel is built for.
bool Engine::stem_fuse_active() const {
    if (!(stem_fuse_ && !blocks_.empty())) return false;
    const DevBlock& b = blocks_[0];
    return !b.spec.has_expand() && !b.spec.has_skip() &&
           stemdw_supported(dtype_, b.dw.plan, b.spec.k, b.spec.s, b.spec.h_in, b.spec.cexp());
}

bool Engine::heads_split_active() const { return split_heads_ && partial_per_crop_ >= size_t(heads_split()) * N_LOGITS; }

bool Engine::head_fused() const {
    return head_fuse_ && pw_impl_ == 0 && heads_split_active() && head7_supported(dtype_, head_.K, head_.N, 49);
}

void Engine::launch_heads_stage(const HeadsArgs& h, const View& v, hipStream_t s) {
    if (heads_split_active()) launch_heads_split(h, v.partial, v.hcount, dtype_, s);
    else launch_heads(h, dtype_, s);
}

// The 7 x 7 tensors between the blocks of an f16 handle (outputs of the projects of blocks 12-16) are stored in the order the matrix
// cores read them: [crop][C/16][HW][16] -- an MFMA operand of 32 pixels x 16 channels is then one or two runs
// of whole cache lines instead of 16 bytes of each of 32 pixel rows.  Same bytes per crop as NHWC, pure addressing: the bits do not
// change.  Blocked iff the producer (the split-K project epilogue, pw.hip) and EVERY consumer (the next block's front7.hip and,
// through its skip, its split-K project; head7.hip behind block 16) know the layout.  front2.hip (the 14 x 14 blocks: measured, the
// layout gains nothing there -- docs/experiments.md section 13), mb7.hip, front.hip and the unfused kernels do not: tensors they
// touch stay NHWC, as do the boundaries of the single-stage entry points (whenet_op_block_range: its input and its output; the
// tensors between its blocks are blocked as in the forward, so that the probes reach the blocked producer and readers).
bool Engine::act_blocked(int index) const {
    if (act_layout_ == 0 || dtype_ != WHENET_F16 || pw_impl_ != 0 || (single_stage_call_ && !range_call_)) return false;
    if (index < 1 || index > int(blocks_.size())) return false;
    const DevBlock& b = blocks_[size_t(index - 1)];
    if (block_schedule(b).use_mb7 || b.project.K < 320 || b.spec.cout % 16 != 0) return false;     // producer: the split-K epilogue
    if (index == int(blocks_.size())) {
        if (!head_fused()) return false;
    } else {
        const DevBlock& c = blocks_[size_t(index)];
        const BlockSchedule cs = block_schedule(c);
        if (cs.use_mb7 || !cs.use_f7) return false;
        if (c.spec.has_skip() && c.project.K < 320) return false;
    }
    // act_layout = 1, the per-layer table (one chain of 64 crops, blocked against the layer's own NHWC timing, profiles/r07): every
    // tensor that CAN be blocked wins -- front7 -1.1 us of 17, head7 -3.0 us of 15.4, their producers' stores -0.1 .. -0.3 us
    static constexpr bool WINS[17] = {false, false, false, false, false, false, false, false, false, false, false, false,
                                      true, true, true, true, true};      // [block index]: outputs of blocks 12-16
    return act_layout_ == 2 || (index <= 16 && WINS[index]);
}

// front2.hip's static-plan form (the tile geometry of front2_tuned.inc's row as compile-time constants): option front2_static = 1
// asks for it on the blocks of the per-layer table; launch_front2 still runs the generic form where the launch is not the row's
// layer and plan (fold12 = 0, WHENET_FRONT_NO_TUNED, WHENET_FRONT_THREADS).  Same bits either way.
bool Engine::front2_static(int index) const {
    // [block index]: the blocks whose shapes have a static form (docs/experiments.md section 24 holds the per-layer verdicts)
    static constexpr bool WINS[17] = {false, false, true, true, true, true, false, true, true, true, true, true, true,
                                      false, false, false, false};       // blocks 2-5 and 7-12
    return front2_static_ && index >= 0 && index <= 16 && WINS[index];
}

// pw.hip's static-shape form of the project GEMMs (the layer's K, N, HW, tile counts and squeeze-excite sizes as compile-time
// constants): option pw_static = 1 asks for it on the blocks of the per-layer table, with the default squeeze-excite placement
// only; launch_pw still runs the generic form where the launch is not a row of its shape table (other batch-dependent blocking,
// act_layout / pw_staged / se_fuse_tiny, the single-stage entry points with other shapes).  Same bits either way.
bool Engine::pw_static(int index) const {
    // [block index]: the blocks whose project layer has a static form (docs/experiments.md section 26 holds the per-layer verdicts)
    // (one chain of 64 crops, static against generic, us: b2 16.1 -> 13.8, b3 20.8 -> 17.6, b4 13.7 -> 10.6, b7 12.4 -> 11.9,
    //  b9 12.0 -> 11.6, b13-15 12.9 -> 11.7, b16 15.0 -> 14.0; b8 12.1 -> 11.8 is inside its own spread of 0.31; b12 lost in an
    //  earlier build; b5, b6, b10, b11 have no static form: profiles/r15/layers_b64.txt)
    static constexpr bool WINS[17] = {false, false, true, true, true, false, false, true, false, true, false, false, false,
                                      true, true, true, true};           // blocks 2-4, 7, 9, 13-16
    return pw_static_ && se_fuse_ == 1 && index >= 0 && index <= 16 && WINS[index];
}

// front.hip's static-shape form (block 6 of an f16 handle, the one block of the default forward that runs front.hip): option
// front_static = 1 asks for it on the blocks of the per-layer table; launch_front still runs the generic form where the launch is
// not the row's layer and plan (512-lane launches of at most 32 crops, WHENET_FRONT_NO_TUNED, WHENET_FRONT_THREADS).  Same bits.
bool Engine::front_static(int index) const {
    // (one chain of 64 crops: 18.9 -> 16.4 us, profiles/r15/layers_b64.txt)
    static constexpr bool WINS[17] = {false, false, false, false, false, false, true, false, false, false, false, false, false,
                                      false, false, false, false};       // block 6
    return front_static_ && index >= 0 && index <= 16 && WINS[index];
}

void* Engine::enqueue_blocks(int first, int last, const View& v, void* cur, int n, hipStream_t s, LaunchRecorder* rec,
                             bool b1_dw_done) {
    const bool fold = fold12_active() && first <= 1 && last >= 2;
    for (int i = first; i <= last; ++i) {
        void* nxt = (cur == v.x0) ? v.x1 : v.x0;
        enqueue_block(blocks_[size_t(i - 1)], v, cur, nxt, n, s, rec, fold && i <= 2 ? i : 0, b1_dw_done && i == 1,
                      i > first && act_blocked(i - 1), i < last || (last == int(blocks_.size()) && !range_call_) ? act_blocked(i) : false);
        cur = nxt;
    }
    return cur;
}

void Engine::enqueue_block(const DevBlock& b, const View& v, const void* in, void* out, int n, hipStream_t s,
                           LaunchRecorder* rec, int fold, bool dw_done, bool in_blocked, bool out_blocked) {
    const BlockSpec& sp = b.spec;
    const BlockSchedule bs = block_schedule(b, n);
    // (checked before anything is enqueued: a violated invariant must not leave half a block in a stream capture)
    WHENET_REQUIRE(fold == 0 || (fold == 1 && !bs.fused && sp.index == 1) ||
                       (fold == 2 && sp.index == 2 && (bs.use_f2 || (split_ && bs.fused && !bs.use_f2s && !bs.use_f7))), WHENET_EINVAL,
                   "fold12: block outside the folded pair");
    WHENET_REQUIRE(!(in_blocked || out_blocked) || (dtype_ == WHENET_F16 && !bs.use_mb7 && (!in_blocked || bs.use_f7)),
                   WHENET_EINVAL, "act_layout: a kernel of this block does not know the blocked layout");
    WHENET_REQUIRE(!bs.use_mb7 || fold == 0, WHENET_EINVAL, "mb7: block outside the 7 x 7 stage");
    if (bs.fused) enqueue_front(b, bs, v, in, out, n, s, rec, fold, in_blocked);
    else enqueue_expand_dw(b, v, in, fold == 1 ? out : v.d, n, s, rec, dw_done);
    if (bs.use_mb7) return;              // that one launch was the whole block
    const SeFuse sef = enqueue_se(b, bs, v, n, s, rec, fold);
    if (fold != 1) enqueue_project(b, sef, bs.se_fused, v, in, out, n, s, rec, in_blocked, out_blocked);
}

// The fields the four front kernels' argument structs share (kernels.h); the three tiled kinds add their geometry.
template <typename A>
void Engine::fill_front_common(A& a, const DevBlock& b, const View& v, const void* in, int n) const {
    a.x = in;
    a.be = b.expand.bias;
    a.bd = b.dw.bias;
    a.out = v.d;
    a.rpart = v.partial;
    a.w1t = b.se.w1t;                    // the SE reduce conv is applied by the front kernel to its channel sums
    a.R = b.se.R;
    a.k = b.spec.k;
    a.Cin = b.spec.cin;
    a.Cexp = b.spec.cexp();
    a.NTe = b.expand.NTILES;
    a.n = n;
}

namespace {
template <typename A>
void fill_front_tiled(A& a, const DevBlock& b) {
    a.s = b.spec.s;
    a.H = b.spec.h_in;
    a.Ho = b.spec.h_out;
    a.pad = b.spec.pad_before();
    a.KSe = b.expand.KS;
}
}  // namespace

void Engine::enqueue_front(const DevBlock& b, const BlockSchedule& bs, const View& v, const void* in, void* out, int n,
                           hipStream_t s, LaunchRecorder* rec, int fold, bool in_blocked) {
    Rec R{rec, s, repeat_};
    const BlockSpec& sp = b.spec;
    const std::string p = "b" + std::to_string(sp.index);
    const double es = double(esz());
    const int hw_in = sp.h_in * sp.h_in, hw_out = sp.h_out * sp.h_out;
    const int cexp = sp.cexp();
    // the stage's algorithmic traffic and work, for a contraction over cin input channels (fold12 changes it)
    auto bytes = [&](int cin) { return double(n) * (hw_in * cin + hw_out * cexp) * es; };
    auto flops = [&](int cin) { return 2.0 * n * (double(hw_in) * cin * cexp + double(hw_out) * sp.k * sp.k * cexp); };
    const bool split = split_ && split_pw_ && b.expand.wps != nullptr;
    if (bs.use_mb7) {
        Mb7Args a{};
        a.x = in;
        a.wep = b.expand.wp;
        a.be = b.expand.bias;
        a.wds = b.mb7.wds;
        a.bd = b.dw.bias;
        a.w1p = b.mb7.w1p;
        a.b1 = b.se.b1;
        a.w2p = b.mb7.w2p;
        a.b2 = b.se.b2;
        a.wpp = b.project.wp;
        a.bp = b.project.bias;
        a.out = out;
        if (single_stage_call_) {            // whenet_op_block reads the block's intermediate tensors back
            a.dbg_dw = v.d;
            a.dbg_gate = v.gate;
        }
        a.k = sp.k;
        a.Cout = sp.cout;
        a.skip = sp.has_skip();
        a.n = n;
        R(p + "/mbconv", "mbconv", kernel_name_mb7(sp.k, sp.cout, a.skip).c_str(),
          double(n) * (hw_in * sp.cin * (a.skip ? 2 : 1) + hw_out * sp.cout) * es,
          2.0 * n * (double(hw_in) * sp.cin * cexp + double(hw_out) * sp.k * sp.k * cexp + double(hw_out) * cexp * sp.cout),
          [&] { launch_mb7(a, s); });
    } else if (bs.use_f7) {
        Front7Args a{};
        fill_front_common(a, b, v, in, n);
        a.dtype = dtype_;
        a.wep = b.expand.wp;
        a.wdt = dtype_ == WHENET_F16 ? static_cast<const void*>(b.dw.wt7) : static_cast<const void*>(b.dw.w);
        a.split = split;
        a.weps = b.expand.wps;
        a.wsi = b.expand.wsi;
        a.xcd_grouped = xcd_grouped(2, n);
        a.x_blocked = in_blocked;
        a.plan = front7_plan_for(dtype_, sp.cin, cexp, n);
        R(p + "/front", "front", kernel_name_front7(dtype_, sp.k, a.plan, a.split).c_str(), bytes(a.Cin), flops(a.Cin),
          [&] { launch_front7(a, s); });
    } else if (bs.use_f2) {
        Front2Args a{};
        fill_front_common(a, b, v, in, n);
        fill_front_tiled(a, b);
        a.wep = b.expand.wp;
        a.wdt = b.dw.wt;
        if (fold == 2) {                     // input = block 1's depthwise output, gated; weights = project1 x expand2
            a.wep = d_fold12_w32_;            // (f32: scaled by the gate, then rounded once -- front2.hip)
            a.be = fold12_pw_.bias;
            a.Cin = fold12_pw_.K;
            a.KSe = fold12_pw_.KS;
            a.NTe = fold12_pw_.NTILES;
            a.in_gate = static_cast<const float*>(v.gate);
        }
        a.xcd_grouped = xcd_grouped(1, n);
        a.plan = b.f2plan;
        a.plan.threads = front2_threads(b.f2plan, n);
        a.static_form = front2_static(sp.index);
        R(p + "/front", "front",
          kernel_name_front2(sp.k, sp.s, a.KSe, a.plan.threads, a.plan.xs, a.in_gate != nullptr, front2_static_row(a)).c_str(),
          bytes(a.Cin), flops(a.Cin), [&] { launch_front2(a, s); });
    } else if (bs.use_f2s) {
        Front2sArgs a{};
        fill_front_common(a, b, v, in, n);
        fill_front_tiled(a, b);
        a.weps = b.expand.wps;
        a.wdt = b.dw.wts;
        a.KSe = b.expand.KSs;
        a.wsi = b.expand.wsi;
        a.wsi_d = b.dw.wts_wsi;
        a.tm = b.f2s_tm;
        a.plan = b.f2splan;
        R(p + "/front", "front", kernel_name_front2s(sp.k, sp.s, a.KSe, a.plan.threads, a.tm, false).c_str(), bytes(a.Cin),
          flops(a.Cin), [&] { launch_front2s(a, s); });
    } else {
        FrontArgs a{};
        fill_front_common(a, b, v, in, n);
        fill_front_tiled(a, b);
        a.wep = b.expand.wp;
        a.wd = b.dw.w;
        a.split = split;
        a.weps = b.expand.wps;
        a.KSes = b.expand.KSs;
        a.wsi = b.expand.wsi;
        if (fold == 2) {                     // input = block 1's depthwise output, gated; weights = project1 x expand2 (f32s)
            a.weps = fold12_pw_.wps;
            a.be = fold12_pw_.bias;
            a.Cin = fold12_pw_.K;
            a.KSe = fold12_pw_.KS;
            a.KSes = fold12_pw_.KSs;
            a.NTe = fold12_pw_.NTILES;
            a.wsi = fold12_pw_.wsi;
            a.in_gate = static_cast<const float*>(v.gate);
        }
        a.xcd_grouped = xcd_grouped(1, n);
        a.plan = b.fplan;
        a.plan.threads = front_threads(b.fplan, n);
        a.static_form = front_static(sp.index);
        R(p + "/front", "front", kernel_name_front(dtype_, sp.k, sp.s, a.plan.threads, front_static_row(a, dtype_)).c_str(), bytes(a.Cin), flops(a.Cin),
          [&] { launch_front(a, dtype_, s); });
    }
}

// The unfused pair: the expand conv (blocks that have one) into v.e, then the depthwise conv into dw_out.
void Engine::enqueue_expand_dw(const DevBlock& b, const View& v, const void* in, void* dw_out, int n, hipStream_t s,
                               LaunchRecorder* rec, bool dw_done) {
    Rec R{rec, s, repeat_};
    const BlockSpec& sp = b.spec;
    const std::string p = "b" + std::to_string(sp.index);
    const double es = double(esz());
    const int hw_in = sp.h_in * sp.h_in, hw_out = sp.h_out * sp.h_out;
    const int cexp = sp.cexp();
    const void* dw_in = in;
    if (sp.has_expand()) {
        const PwArgs a = pw_args(b.expand, in, v.e, n * hw_in, hw_in, ACT_SWISH);
        R(p + "/expand", "pw", kernel_name_pw(a, dtype_, pw_impl_, num_cus_).c_str(), double(a.M) * (a.K + a.N) * es,
          2.0 * a.M * a.K * a.N, [&] { launch_pw(a, dtype_, pw_impl_, num_cus_, s); });
        dw_in = v.e;
    }
    if (!dw_done) {
        DwArgs a{};
        a.in = dw_in;
        a.out = dw_out;
        a.w = b.dw.w;
        a.bias = b.dw.bias;
        a.partial = v.partial;
        a.k = sp.k;
        a.s = sp.s;
        a.H = sp.h_in;
        a.Ho = sp.h_out;
        a.C = cexp;
        a.pad = sp.pad_before();
        a.n = n;
        a.plan = b.dw.plan;
        R(p + "/dw", "dw", kernel_name_dw(dtype_, sp.k, sp.s), double(n) * (hw_in + hw_out) * cexp * es,
          2.0 * n * hw_out * sp.k * sp.k * cexp, [&] { launch_dw(a, dtype_, s); });
    }
}

// Second half of the SEBlock.  Where it pays, the project GEMM's workgroups compute the gate of their own rows'
// crops from the front kernel's partial vectors in their prologue (se_device.h; no launch, the gate never reaches
// HBM); otherwise a stand-alone launch writes the gate.  Measured per block at 64 crops (tools/ab_layers.sh,
// se_fuse=2 against 0): every workgroup has to pull the WHOLE excite kernel (K x R floats) and all partial vectors
// of its crops, so the prologue costs +1 us for blocks 4-6 (<= 12 KB, <= 20 vectors: a 7-8 us launch saved), +7 /
// +12 us for blocks 3 / 2 (40 / 48 partial vectors: three dependent round trips), +4..9 us for the 14x14 blocks
// (38-75 KB: break-even) and +24 us for the 7x7 blocks (221 KB per workgroup at ~50 GB/s per CU).  The bits are
// the same either way.  Option se_fuse: 0 = never, 1 = where it pays (default), 2 = every fused-front block.
SeFuse Engine::enqueue_se(const DevBlock& b, const BlockSchedule& bs, const View& v, int n, hipStream_t s, LaunchRecorder* rec,
                          int fold) {
    Rec R{rec, s, repeat_};
    const std::string p = "b" + std::to_string(b.spec.index);
    const int hw_out = b.spec.h_out * b.spec.h_out;
    SeFuse sef{};
    if (bs.se_fused) {
        sef.rpart = v.partial;
        sef.b1 = b.se.b1;
        sef.w2c = b.se.w2c;
        sef.b2 = b.se.b2;
        sef.np = bs.se_ntiles * bs.se_chunks;
        sef.R = b.se.R;
        sef.RP = se_padded_r(b.se.R);
        sef.inv_hw = 1.0f / float(hw_out);
        if (bs.se_mfma) {
            sef.w2p = b.se.w2p;
            sef.KSr = b.se.KSr;
            sef.w2_wsi = b.se.w2_wsi;
        }
    } else if (bs.se_in_front) {
        // the front kernel already applied se_reduce to its channel sums (v.partial holds the
        // (tiles x chunks) partial vectors of every crop): finish the SEBlock
        SeExciteArgs a{};
        a.rpart = v.partial;
        a.np = bs.se_ntiles * bs.se_chunks;
        a.inv_hw = 1.0f / float(hw_out);
        a.b1 = b.se.b1;
        a.w2c = b.se.w2c;
        a.b2 = b.se.b2;
        a.gate = v.gate;
        a.gate_f16 = dtype_ == WHENET_F16;
        a.C = b.se.C;
        a.R = b.se.R;
        a.n = n;
        R(p + "/se", "se", ("whenet_se_excite_kernel<" + std::to_string(se_padded_r(a.R)) + ">").c_str(),
          double(n) * (a.np * se_padded_r(a.R) + a.C) * 4.0 + double(a.C) * se_padded_r(a.R) * 4.0, 2.0 * n * a.C * a.R,
          [&] { launch_se_excite(a, s); });
    } else {
        SeArgs a{};
        a.partial = v.partial;
        a.ntiles = bs.se_ntiles;
        a.inv_hw = 1.0f / float(hw_out);
        a.w1t = b.se.w1t;
        a.b1 = b.se.b1;
        a.w2c = b.se.w2c;
        a.b2 = b.se.b2;
        a.gate = v.gate;
        a.gate_f16 = dtype_ == WHENET_F16 && fold != 1;      // (fold12: block 2 scales f32 weights by an f32 gate)
        a.C = b.se.C;
        a.R = b.se.R;
        a.n = n;
        R(p + "/se", "se", ("whenet_se_kernel<" + std::to_string(se_padded_r(a.R)) + ">").c_str(), double(n) * (a.ntiles + 1) * a.C * 4.0 + 2.0 * a.C * a.R * 4.0,
          4.0 * n * a.C * a.R, [&] { launch_se(a, s); });
    }
    return sef;
}

void Engine::enqueue_project(const DevBlock& b, const SeFuse& sef, bool se_fused, const View& v, const void* in, void* out, int n,
                             hipStream_t s, LaunchRecorder* rec, bool in_blocked, bool out_blocked) {
    Rec R{rec, s, repeat_};
    const BlockSpec& sp = b.spec;
    const int hw_out = sp.h_out * sp.h_out;
    PwArgs a = pw_args(b.project, v.d, out, n * hw_out, hw_out, ACT_NONE);
    a.gate = se_fused ? nullptr : v.gate;
    a.se = sef;
    a.res = sp.has_skip() ? in : nullptr;
    a.out_blocked = out_blocked;
    a.res_blocked = in_blocked && sp.has_skip();
    a.static_form = pw_static(sp.index);
    R("b" + std::to_string(sp.index) + "/project", "pw", kernel_name_pw(a, dtype_, pw_impl_, num_cus_).c_str(),
      double(a.M) * (a.K + a.N + (sp.has_skip() ? a.N : 0)) * double(esz()), 2.0 * a.M * a.K * a.N,
      [&] { launch_pw(a, dtype_, pw_impl_, num_cus_, s); });
}

Head7Args Engine::head7_args(const void* x, float* feat, int n) const {
    Head7Args a{};
    a.dtype = dtype_;
    a.x = x;
    a.wep = head_.wp;
    a.bias = head_.bias;
    a.feat = feat;
    a.K = head_.K;
    a.N = head_.N;
    a.NTILES = head_.NTILES;
    a.split = split_ && split_pw_ && head_.wps != nullptr;
    a.weps = head_.wps;
    a.wsi = head_.wsi;
    a.n = n;
    return a;
}

PwArgs Engine::pw_args(const DevPw& w, const void* a, void* out, int M, int HW, int act) const {
    PwArgs r{};
    r.a = a;
    r.wp = w.wp;
    r.wdense = w.wdense;
    r.bias = w.bias;
    r.out = out;
    r.M = M;
    r.K = w.K;
    r.N = w.N;
    r.KS = w.KS;
    r.NTILES = w.NTILES;
    r.HW = HW;
    r.act = act;
    // WHENET_F32S: 1x1 products as binary16 hi/lo pairs (option "split_pw" switches the pointwise kernels between the two forms)
    r.staged = pw_staged_;
    r.split = split_ && split_pw_ && w.wps != nullptr;
    r.wps = w.wps;
    r.KSs = w.KSs;
    r.wsi = w.wsi;
    return r;
}

void Engine::enqueue_forward(const View& v, const uint8_t* d_in, int n, Results out, hipStream_t s, LaunchRecorder* rec,
                             const float* d_in_f32) {
    Rec R{rec, s, repeat_};
    const double es = double(esz());
    const bool stemdw = stem_fuse_active() && d_in_f32 == nullptr;
    if (stemdw) {
        // stem + block 1's depthwise conv (stemdw.hip): writes what enqueue_block() would have block 1's dw.hip launch write
        const DevBlock& b1 = blocks_[0];
        const bool fold = fold12_active() && blocks_.size() >= 2;
        StemDwArgs a{};
        a.dtype = dtype_;
        a.w = d_stem_w_;
        a.lut = d_lut_;
        a.in = d_in;
        a.out = fold ? v.x1 : v.d;
        a.tab = d_stemdw_tab_;
        a.bias = d_stem_b_;
        a.wd = b1.dw.w;
        a.bd = b1.dw.bias;
        a.partial = v.partial;
        a.n = n;
        R("stem+b1/dw", "stem", kernel_name_stemdw(dtype_), double(n) * (IN_BYTES + X_ELEMS * es), 2.0 * n * (10838016.0 + 112.0 * 112 * 9 * 32),
          [&] { launch_stemdw(a, s); });
    } else {
        StemArgs a{d_in, v.x0, d_stem_w_, d_stem_b_, d_lut_, n};
        a.in_f32 = d_in_f32;
        R("stem", "stem", kernel_name_stem(dtype_), double(n) * (IN_BYTES + X_ELEMS * es), 2.0 * n * 10838016.0,
          [&] { launch_stem(a, dtype_, s); });
    }
    void* cur = enqueue_blocks(1, int(blocks_.size()), v, v.x0, n, s, rec, stemdw);
    HeadsArgs h{};
    h.w = d_dense_w_;
    h.b = d_dense_b_;
    h.logits = out.logits;
    h.ypr = out.ypr;
    h.argmax = out.amax;
    h.n = n;
    if (head_fused()) {
        // head conv + GlobalAveragePooling2D as one kernel (head7.hip): v.hc receives the pooled features [n][1280] f32
        Head7Args a = head7_args(cur, reinterpret_cast<float*>(v.hc), n);
        a.xcd_grouped = xcd_grouped(4, n);
        a.x_blocked = act_blocked(int(blocks_.size()));
        R("head", "pw", kernel_name_head7(dtype_, n, a.split).c_str(), double(n) * (49.0 * a.K * es + a.N * 4.0), 2.0 * n * 49.0 * a.K * a.N,
          [&] { launch_head7(a, s); });
        h.feat_in = reinterpret_cast<const float*>(v.hc);
        R("heads", "heads", "whenet_heads_split_kernel<float, true>", double(n) * ((FEAT + N_LOGITS + 6) * 4.0) + double(FEAT) * N_LOGITS * 4.0,
          2.0 * n * FEAT * N_LOGITS, [&] { launch_heads_stage(h, v, s); });
        return;
    }
    const PwArgs a = head_pw_args(cur, v.hc, n);
    R("head", "pw", kernel_name_pw(a, dtype_, pw_impl_, num_cus_).c_str(), double(a.M) * (a.K + a.N) * es, 2.0 * a.M * a.K * a.N,
      [&] { launch_pw(a, dtype_, pw_impl_, num_cus_, s); });
    h.x = v.hc;
    // (v.partial is free here: the last squeeze-excite is long done)
    const bool split = heads_split_active();
    const std::string hname = std::string(split ? "whenet_heads_split_kernel<" : "whenet_heads_kernel<") +
                              (dtype_ == WHENET_F16 ? "_Float16" : "float") + (split ? ", false>" : ">");
    R("heads", "heads", hname.c_str(), double(n) * (HC_ELEMS * es + (N_LOGITS + 6) * 4.0) + double(FEAT) * N_LOGITS * 4.0,
      2.0 * n * FEAT * N_LOGITS, [&] { launch_heads_stage(h, v, s); });
}

hipStream_t Engine::lane_stream(int i) {
    while (int(lane_streams_.size()) <= i) {
        Stream st;
        WHENET_HIP_CHECK(hipStreamCreateWithFlags(st.put(), hipStreamNonBlocking));
        lane_streams_.push_back(std::move(st));
    }
    return lane_streams_[size_t(i)];
}

// Drop the on-demand streams (and the graphs that reference them): called before a handle creates
// more engines, so that the new engines' main streams are placed on hardware queues as on a fresh
// process instead of behind this engine's idle lane / copy streams.
void Engine::release_aux_streams() {
    DeviceGuard guard(device_);
    sync();
    drop_graphs();
    lane_streams_.clear();
    copy_stream_.reset();
}

hipStream_t Engine::copy_stream() {
    if (!copy_stream_) WHENET_HIP_CHECK(hipStreamCreateWithFlags(copy_stream_.put(), hipStreamNonBlocking));
    return copy_stream_;
}

Engine::View Engine::view(int crop_off) const {
    auto at = [&](int i) { return arena_[i].buf.as<char>() + size_t(crop_off) * arena_[i].per_crop; };
    View v;
    v.x0 = at(A_X0);
    v.x1 = at(A_X1);
    v.e = at(A_E);
    v.d = at(A_D);
    v.hc = at(A_HC);
    v.partial = reinterpret_cast<float*>(at(A_PARTIAL));
    v.gate = reinterpret_cast<float*>(at(A_GATE));
    v.hcount = reinterpret_cast<unsigned*>(at(A_HCOUNT));
    v.in_u8 = reinterpret_cast<uint8_t*>(at(A_IN_U8));
    v.out = {reinterpret_cast<float*>(at(A_YPR)), reinterpret_cast<int32_t*>(at(A_AMAX)), reinterpret_cast<float*>(at(A_LOGITS))};
    return v;
}

// One forward = up to `lanes_` independent sub-batches, each a 51-kernel chain on its own
// stream (forked from / joined back into `s` with events, so that under capture they become
// parallel branches of ONE graph).  Crops are independent, so the split changes nothing in the
// results; what it buys is overlap: most kernels of this network are short (10-30 us) and
// latency-bound, and two chains in flight fill each other's launch / drain bubbles.
int Engine::lanes_for(int n, int want) const {
    int lanes = want > 0 ? std::min(want, MAX_LANES) : lanes_;
    while (lanes > 1 && n / lanes < min_lane_crops_) --lanes;
    return lanes;
}

template <typename F>
void Engine::for_each_lane(int n, int lanes, hipStream_t s, F&& body) {
    WHENET_HIP_CHECK(hipEventRecord(fork_ev_, s));
    int off = 0;
    for (int i = 0; i < lanes; ++i) {
        const int cnt = n / lanes + (i < n % lanes ? 1 : 0);
        hipStream_t st = (i == 0) ? s : lane_stream(i - 1);
        if (i > 0) WHENET_HIP_CHECK(hipStreamWaitEvent(st, fork_ev_, 0));
        body(i, off, cnt, st);
        if (i > 0) {
            WHENET_HIP_CHECK(hipEventRecord(join_ev_[size_t(i - 1)], st));
            WHENET_HIP_CHECK(hipStreamWaitEvent(s, join_ev_[size_t(i - 1)], 0));
        }
        off += cnt;
    }
}

void Engine::enqueue_lanes(const uint8_t* d_in, int n, Results out, hipStream_t s, int want) {
    const int lanes = lanes_for(n, want);
    if (lanes <= 1) {
        enqueue_forward(view(0), d_in, n, out, s, nullptr);
        return;
    }
    for_each_lane(n, lanes, s, [&](int, int off, int cnt, hipStream_t st) {
        enqueue_forward(view(off), d_in + size_t(off) * IN_BYTES, cnt, out.at(size_t(off)), st, nullptr);
    });
}

// Capture fn's launches on stream s into an executable graph (cached under key) and return it.
template <typename F>
hipGraphExec_t Engine::cached_graph(const GraphKey& key, hipStream_t s, F&& fn) {
    auto it = graphs_.find(key);
    if (it != graphs_.end()) return it->second;
    if (graphs_.size() >= size_t(MAX_GRAPHS)) {
        sync_streams(s);                 // (s may be a lane stream: the main stream's graphs are in flight too)
        WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
        drop_graphs();
    }
    hipGraph_t graph = nullptr;
    WHENET_HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
    try {
        fn();
    } catch (...) {
        (void)hipStreamEndCapture(s, &graph);
        if (graph) (void)hipGraphDestroy(graph);
        throw;
    }
    WHENET_HIP_CHECK(hipStreamEndCapture(s, &graph));
    hipGraphExec_t exec = nullptr;
    hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) throw Error(WHENET_EHIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
    graphs_.emplace(key, exec);
    return exec;
}

// debug option "poison": every activation buffer holds NaN bit patterns when the forward starts, so a kernel that reads what no
// kernel of THIS forward wrote shows up in the results (tests/test_gpu_parity.py)
void Engine::poison_arena(int n, hipStream_t s) {
    for (int i = 0; i < A_POISONED; ++i)
        WHENET_HIP_CHECK(hipMemsetAsync(arena_[i].buf.as<void>(), 0xff, size_t(n) * arena_[i].per_crop, s));
}

void Engine::run_forward(const uint8_t* d_in, int n, Results out, hipStream_t s, int want) {
    if (poison_) poison_arena(n, s);
    if (!use_graph_) {
        enqueue_lanes(d_in, n, out, s, want);
        return;
    }
    const int lanes = lanes_for(n, want);
    if (lanes > 1) (void)lane_stream(lanes - 2);        // the lane streams exist before any capture starts
    if (lane_graphs_ && lanes > 1) {
        // One graph PER LANE, each launched on its own stream: the chains then run as independent queues.
        // (Branches of a single graph cost ~5 us per edge on this runtime, which eats the overlap.)
        // (The lane's wait on the fork event is enqueued before its graph is built: a capture enqueues nothing on the stream.)
        for_each_lane(n, lanes, s, [&](int, int off, int cnt, hipStream_t st) {
            const uint8_t* in_i = d_in + size_t(off) * IN_BYTES;
            const Results out_i = out.at(size_t(off));
            hipGraphExec_t g = cached_graph(GraphKey{cnt, off, in_i, out_i.ypr, out_i.amax, out_i.logits}, st,
                                            [&] { enqueue_forward(view(off), in_i, cnt, out_i, st, nullptr); });
            WHENET_HIP_CHECK(hipGraphLaunch(g, st));
        });
        return;
    }
    hipGraphExec_t g = cached_graph(GraphKey{n, -lanes, d_in, out.ypr, out.amax, out.logits}, s,
                                    [&] { enqueue_lanes(d_in, n, out, s, lanes); });
    WHENET_HIP_CHECK(hipGraphLaunch(g, s));
}

// ------------------------------------------------------------------------------------------
// public paths
// ------------------------------------------------------------------------------------------
void Engine::forward_device(const uint8_t* d_crops, int n, float* d_ypr, int32_t* d_argmax, float* d_logits,
                            hipStream_t stream) {
    DeviceGuard guard(device_);
    require_model();
    WHENET_REQUIRE(d_crops != nullptr && d_ypr != nullptr, WHENET_EINVAL, "crops and ypr must not be NULL");
    WHENET_REQUIRE((reinterpret_cast<uintptr_t>(d_crops) & 3) == 0, WHENET_EINVAL, "crops must be 4-byte aligned");
    ensure_capacity(n);
    run_forward(d_crops, n, Results{d_ypr, d_argmax, d_logits}, stream ? stream : stream_);
}

void Engine::forward_host(const uint8_t* crops, int n, float* ypr, int32_t* argmax, float* logits) {
    DeviceGuard guard(device_);
    require_model();
    WHENET_REQUIRE(crops != nullptr && ypr != nullptr, WHENET_EINVAL, "crops and ypr must not be NULL");
    ensure_capacity(n);
    const size_t N = size_t(n);
    const Results caller{ypr, argmax, logits};
    if (n <= host_pinned_max_) {
        // The reference's own call shape -- get_angle(uint8[1,224,224,3]) per head (demo.py:14, demo_video.py:27): latency.
        // Copies to and from PAGEABLE memory are synchronous inside the runtime (the three result copies each wait for the
        // forward and go through its staging buffer one after the other); through a pinned slot the call is memcpy ->
        // H2D -> graph -> 3 D2H, all asynchronous on ONE stream, one wait, memcpy out (round 5: 490 -> see DESIGN us at B=1 f32).
        Slot& sl = host_slot_;
        ensure_slot(sl, std::max(n, std::min(host_pinned_max_, 16)));
        std::memcpy(sl.in.h.as<void>(), crops, N * IN_BYTES);
        WHENET_HIP_CHECK(hipMemcpyAsync(sl.in.d.as<void>(), sl.in.h.as<void>(), N * IN_BYTES, hipMemcpyHostToDevice, stream_));
        run_forward(sl.in.d.as<uint8_t>(), n, sl.dev(), stream_, host_lanes_);
        copy_results_async(sl.host(), sl.dev(), n, stream_, argmax != nullptr, logits != nullptr);
        WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
        copy_results_host(caller, sl.host(), n);
        return;
    }
    // (Measured, round 4: issuing the copy lane by lane in front of per-lane graphs, so that the first chain runs while the
    //  second lane's crops travel, changes nothing -- 68.5 k vs 69.6 k crops/s at 64 crops: the 9.6 MB copy from pageable
    //  memory is 0.18 ms of a 0.92 ms call, and two graphs on two streams lose what the overlap gains.)
    ensure_host_out(n);
    const View v = view(0);
    WHENET_HIP_CHECK(hipMemcpyAsync(v.in_u8, crops, N * IN_BYTES, hipMemcpyHostToDevice, stream_));
    // a blocking call has the GPU to itself whatever "inflight" says: the forward runs as host_lanes_ chains
    run_forward(v.in_u8, n, v.out, stream_, host_lanes_);
    // results: asynchronous copies into pinned memory, ONE wait (copies into the caller's pageable arrays each wait for the forward
    // and for each other inside the runtime)
    copy_results_async(hout(), v.out, n, stream_, argmax != nullptr, logits != nullptr);
    WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
    copy_results_host(caller, hout(), n);
}

void Engine::ensure_host_out(int n) {
    if (n <= hout_cap_) return;
    // One allocation that covers every blocking call below the fan-out threshold (264 KB of pinned memory), made under a process-wide
    // lock: growing these buffers (hipHostFree + hipHostMalloc) while another handle's thread was inside its own forward crashed
    // inside the runtime (2-3 of 8 runs of tests/test_multi_device.py with two handles on one device).
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
    hout_ypr_.release();
    hout_amax_.release();
    hout_logits_.release();
    hout_cap_ = 0;
    const size_t N = size_t(std::max(n, 256));
    hout_ypr_.reset(N * 3 * sizeof(float));
    hout_amax_.reset(N * 3 * sizeof(int32_t));
    hout_logits_.reset(N * N_LOGITS * sizeof(float));
    hout_cap_ = int(N);
}

// Model.predict on the NORMALISED float32 image (whenet.py:27) + decode: the path for real-valued
// crops (whenet.py:25 divides whatever dtype it is given by 255), which the byte LUT cannot serve.
// Eager launches (no graph): a compatibility path, not the one bench.py times.
void Engine::forward_host_f32(const float* x, int n, float* ypr, int32_t* argmax, float* logits) {
    DeviceGuard guard(device_);
    require_model();
    WHENET_REQUIRE(x != nullptr && ypr != nullptr, WHENET_EINVAL, "image and ypr must not be NULL");
    ensure_capacity(n);
    const size_t nbytes = size_t(n) * IN_BYTES * sizeof(float);
    if (nbytes > in_f32_.bytes()) {
        WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
        in_f32_.reset(nbytes, "float input buffer");
    }
    if (poison_) {
        poison_arena(n, stream_);
        WHENET_HIP_CHECK(hipMemsetAsync(in_f32_.as<void>(), 0xff, in_f32_.bytes(), stream_));
    }
    WHENET_HIP_CHECK(hipMemcpyAsync(in_f32_.as<void>(), x, nbytes, hipMemcpyHostToDevice, stream_));
    const View v = view(0);
    enqueue_forward(v, nullptr, n, v.out, stream_, nullptr, in_f32_.as<float>());
    copy_results_async(Results{ypr, argmax, logits}, v.out, n, stream_, argmax != nullptr, logits != nullptr);
    WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
}

void Engine::sync_streams(hipStream_t s) {
    WHENET_HIP_CHECK(hipStreamSynchronize(s));
    for (hipStream_t st : lane_streams_) WHENET_HIP_CHECK(hipStreamSynchronize(st));
}

void Engine::sync() {
    DeviceGuard guard(device_);
    WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
    if (copy_stream_) WHENET_HIP_CHECK(hipStreamSynchronize(copy_stream_));
    for (hipStream_t st : lane_streams_) WHENET_HIP_CHECK(hipStreamSynchronize(st));
}

void Engine::ensure_slot(Slot& s, int n) {
    if (!s.copied) {
        s.copied.create();
        s.done.create();
    }
    if (n <= s.capacity) return;
    s.capacity = 0;
    const size_t N = size_t(n);
    const size_t bytes[4] = {N * IN_BYTES, N * 3 * sizeof(float), N * 3 * sizeof(int32_t), N * N_LOGITS * sizeof(float)};
    StagedBuffer* const bufs[4] = {&s.in, &s.ypr, &s.amax, &s.logits};
    for (StagedBuffer* b : bufs) b->h.release(), b->d.release();      // (all eight go before the first of the larger ones comes)
    for (int i = 0; i < 4; ++i) bufs[i]->h.reset(bytes[i]);      // (the pinned four first, then the device four)
    for (int i = 0; i < 4; ++i) bufs[i]->d.reset(bytes[i]);
    s.capacity = n;
}

hipStream_t Engine::copy_stream_handle() {
    DeviceGuard guard(device_);
    return copy_stream();
}

hipEvent_t Engine::copied_event(int ticket) const {
    for (const Slot& s : slots_)
        if (s.busy && s.ticket == ticket) return s.copied;
    throw Error(WHENET_EINVAL, "unknown ticket " + std::to_string(ticket));
}

Engine::Slot* Engine::free_slot() {
    for (Slot& s : slots_)
        if (!s.busy) return &s;
    throw Error(WHENET_EINVAL, "too many submissions in flight (collect one first)");
}

int Engine::finish_submission(Slot& s, int n) {
    WHENET_HIP_CHECK(hipEventRecord(s.done, stream_));
    s.busy = true;
    s.n = n;
    s.det_cap = -1;
    s.clip_f = 0, s.clip_cap = -1, s.clip_mixed = false;
    s.ann_kind = Slot::ANN_NONE, s.ann_mask = 0;
    s.ann_host.clear(), s.jpg_host.clear();
    s.jpg_dec_out = nullptr;
    s.ticket = next_ticket_++;
    return s.ticket;
}

int Engine::submit(const uint8_t* crops, int n, int stage, int want_lanes, hipStream_t copy_on, hipEvent_t copy_after) {
    DeviceGuard guard(device_);
    require_model();
    WHENET_REQUIRE(crops != nullptr, WHENET_EINVAL, "crops must not be NULL");
    Slot& slot = *free_slot();
    ensure_capacity(n);
    ensure_slot(slot, n);
    const size_t N = size_t(n);
    // Through a pinned slot: a copy straight from the caller's pageable memory (hipMemcpyAsync stages it inside the runtime)
    // blocks the host until the DMA is done and serialises the submissions -- measured round 4: 67.8 k vs 90.4 k crops/s with
    // three 64-crop batches in flight.
    // stage 1 (the fan-out of one large blocking call, capi.cpp): straight from the caller's memory on the copy stream -- the
    // host blocks for THIS chunk's DMA only, while the forwards of the chunks before it run.
    const hipStream_t cs = copy_on != nullptr ? copy_on : copy_stream();
    if (copy_after != nullptr) WHENET_HIP_CHECK(hipStreamWaitEvent(cs, copy_after, 0));
    uint8_t* const d_in = slot.in.d.as<uint8_t>();
    if (stage == 1) {
        WHENET_HIP_CHECK(hipMemcpyAsync(d_in, crops, N * IN_BYTES, hipMemcpyHostToDevice, cs));
    } else {
        std::memcpy(slot.in.h.as<void>(), crops, N * IN_BYTES);
        WHENET_HIP_CHECK(hipMemcpyAsync(d_in, slot.in.h.as<void>(), N * IN_BYTES, hipMemcpyHostToDevice, cs));
    }
    WHENET_HIP_CHECK(hipEventRecord(slot.copied, cs));
    WHENET_HIP_CHECK(hipStreamWaitEvent(stream_, slot.copied, 0));
    run_forward(d_in, n, slot.dev(), stream_, want_lanes);
    copy_results_async(slot.host(), slot.dev(), n, stream_);
    return finish_submission(slot, n);
}

// After a failed fan-out: wait for whatever was enqueued and hand every slot back.
void Engine::abandon_submissions() {
    DeviceGuard guard(device_);
    (void)hipStreamSynchronize(stream_);
    if (copy_stream_) (void)hipStreamSynchronize(copy_stream_);
    for (Slot& s : slots_) s.busy = false, s.ann_host.clear(), s.jpg_host.clear(), s.jpg_dec_out = nullptr;
}

void Engine::collect(int ticket, float* ypr, int32_t* argmax, float* logits) {
    DeviceGuard guard(device_);
    Slot* slot = nullptr;
    for (Slot& s : slots_)
        if (s.busy && s.ticket == ticket) slot = &s;
    WHENET_REQUIRE(slot != nullptr, WHENET_EINVAL, "unknown or already collected ticket " + std::to_string(ticket));
    WHENET_REQUIRE(slot->det_cap < 0, WHENET_EINVAL,
                   "collect: ticket " + std::to_string(ticket) + " was submitted by frame_detect_heads: collect_detect returns it");
    WHENET_REQUIRE(slot->clip_cap < 0, WHENET_EINVAL,
                   "collect: ticket " + std::to_string(ticket) + " was submitted by clip_detect_heads: collect_clip returns it");
    WHENET_HIP_CHECK(hipEventSynchronize(slot->done));
    finish_annotations(*slot);
    copy_results_host(Results{ypr, argmax, logits}, slot->host(), slot->n);
    slot->busy = false;
}

int Engine::profile(const uint8_t* d_crops, int n, int iters, whenet_launch_stat_t* stats, int cap) {
    DeviceGuard guard(device_);
    require_model();
    WHENET_REQUIRE(d_crops != nullptr && iters >= 1, WHENET_EINVAL, "profile: bad arguments");
    ensure_capacity(n);
    const int lanes = lanes_for(n, 0);
    std::vector<LaunchRecorder> recs;      // (their events go with them)
    recs.resize(size_t(lanes));
    for (auto& lr : recs) lr.start.create(hipEventDefault);
    const Results out = view(0).out;
    // one untimed eager pass so that lazy code-object loading does not land in the numbers
    enqueue_forward(view(0), d_crops, n, out, stream_, nullptr);
    WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
    for (int it = 0; it < iters; ++it) {
        for_each_lane(n, lanes, stream_, [&](int i, int off, int cnt, hipStream_t st) {
            LaunchRecorder& lr = recs[size_t(i)];
            lr.cursor = 0;
            WHENET_HIP_CHECK(hipEventRecord(lr.start, st));
            enqueue_forward(view(off), d_crops + size_t(off) * IN_BYTES, cnt, out.at(size_t(off)), st, &lr);
            {   // calibration entry: an empty kernel timed the same way = the boundary + event cost
                Rec R{&lr, st, 1};
                R("(boundary)", "calib", "whenet_empty_kernel", 0.0, 0.0, [&] { launch_empty(st); });
            }
            lr.first_pass = false;
        });
        WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
        for (auto& lr : recs) {
            hipEvent_t prev = lr.start;
            for (auto& e : lr.entries) {
                float ms = 0.f;
                WHENET_HIP_CHECK(hipEventElapsedTime(&ms, prev, e.stop));
                e.total_ms += ms;
                prev = e.stop;
            }
        }
    }
    const int count = int(recs[0].entries.size());
    for (int i = 0; i < count && i < cap && stats; ++i) {
        const auto& e = recs[0].entries[size_t(i)];
        double tot = 0;
        for (auto& lr : recs) tot += lr.entries[size_t(i)].total_ms;
        whenet_launch_stat_t& o = stats[i];
        copy_name(o.layer, sizeof(o.layer), e.layer);
        copy_name(o.kind, sizeof(o.kind), e.kind);
        copy_name(o.kernel, sizeof(o.kernel), e.kernel);
        o.avg_us = tot * 1000.0 / (double(iters) * lanes);
        o.alg_bytes = e.bytes;
        o.alg_flops = e.flops;
        o.crops = n / lanes + (0 < n % lanes ? 1 : 0);       // (chain 0's sub-batch: what bytes / flops are counted for)
        o.chains = lanes;
    }
    return count;
}

}  // namespace whenet
