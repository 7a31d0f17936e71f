// Frame-level entry points around the hot path: one submission per video frame (crop + resize +
// colour order on the device, then the forward), the crop/resize stage alone, and the YOLOv3 detector's post-processing.
#include <limits>

#include "engine_internal.h"

namespace whenet {

using namespace detail;

void Engine::ensure_slot_frame(Slot& s, size_t frame_bytes, int k) {
    s.frame.h.grow(frame_bytes);
    s.frame.d.grow(frame_bytes);
    const size_t plan_bytes = size_t(k) * CROP_PLAN_INTS * sizeof(int32_t);
    s.plan.h.grow(plan_bytes);
    s.plan.d.grow(plan_bytes);
}

namespace {
void check_rects(int fh, int fw, const int32_t* rects, int k) {
    for (int i = 0; i < k; ++i) {
        const int32_t* r = rects + 4 * i;
        WHENET_REQUIRE(r[0] >= 0 && r[1] >= 0 && r[2] <= fh && r[3] <= fw && r[0] < r[2] && r[1] < r[3], WHENET_EINVAL,
                       "crop window " + std::to_string(i) + " is empty or outside the frame");
    }
}
}  // namespace

// One frame of demo_video.py:49-58 as ONE submission: the frame crosses PCIe once; every head is
// cropped / colour-swapped / resized on the device (frame.hip) straight into the forward's input.
int Engine::submit_frame(const uint8_t* frame, int fh, int fw, int swap_rb, const int32_t* rects, int k) {
    DeviceGuard guard(device_);
    require_model();
    WHENET_REQUIRE(frame != nullptr && fh > 0 && fw > 0 && k >= 0 && (k == 0 || rects != nullptr), WHENET_EINVAL,
                   "submit_frame: bad arguments");
    check_rects(fh, fw, rects, k);
    Slot& slot = *free_slot();
    if (k > 0) {
        ensure_capacity(k);
        ensure_slot(slot, k);
        const size_t fbytes = size_t(fh) * fw * 3;
        ensure_slot_frame(slot, fbytes, k);
        int32_t* const h_plan = slot.plan.h.as<int32_t>();
        std::memcpy(slot.frame.h.as<void>(), frame, fbytes);
        for (int i = 0; i < k; ++i) build_crop_plan(rects + 4 * i, h_plan + size_t(i) * CROP_PLAN_INTS);
        WHENET_HIP_CHECK(hipMemcpyAsync(slot.frame.d.as<void>(), slot.frame.h.as<void>(), fbytes, hipMemcpyHostToDevice, copy_stream()));
        WHENET_HIP_CHECK(hipMemcpyAsync(slot.plan.d.as<void>(), h_plan, size_t(k) * CROP_PLAN_INTS * sizeof(int32_t),
                                        hipMemcpyHostToDevice, copy_stream()));
        WHENET_HIP_CHECK(hipEventRecord(slot.copied, copy_stream()));
        WHENET_HIP_CHECK(hipStreamWaitEvent(stream_, slot.copied, 0));
        launch_crop_resize(slot.frame.d.as<uint8_t>(), fw, swap_rb, slot.plan.d.as<int32_t>(), k, slot.in.d.as<uint8_t>(), stream_);
        run_forward(slot.in.d.as<uint8_t>(), k, slot.dev(), stream_);
        copy_results_async(slot.host(), slot.dev(), k, stream_);
    } else {
        ensure_slot(slot, 1);
    }
    const int ticket = finish_submission(slot, k);
    if (k > 0) slot.fh = fh, slot.fw = fw, slot.swap_rb = swap_rb, slot.ann_kind = Slot::ANN_PLANS;      // (k = 0 uploads no frame)
    return ticket;
}

void Engine::op_crop_resize(const uint8_t* frame, int fh, int fw, int swap_rb, const int32_t* rects, int k,
                            uint8_t* crops_out) {
    DeviceGuard guard(device_);
    WHENET_REQUIRE(frame != nullptr && rects != nullptr && crops_out != nullptr && fh > 0 && fw > 0 && k > 0,
                   WHENET_EINVAL, "op_crop_resize: bad arguments");
    check_rects(fh, fw, rects, k);
    std::vector<int32_t> plan(size_t(k) * CROP_PLAN_INTS);
    for (int i = 0; i < k; ++i) build_crop_plan(rects + 4 * i, plan.data() + size_t(i) * CROP_PLAN_INTS);
    const size_t fbytes = size_t(fh) * fw * 3, obytes = size_t(k) * IN_BYTES;
    DeviceBuffer d_frame, d_plan, d_out;
    d_frame.reset(fbytes, "hipMalloc");
    d_plan.reset(plan.size() * sizeof(int32_t), "hipMalloc");
    d_out.reset(obytes, "hipMalloc");
    WHENET_HIP_CHECK(hipMemcpy(d_frame.as<void>(), frame, fbytes, hipMemcpyHostToDevice));
    WHENET_HIP_CHECK(hipMemcpy(d_plan.as<void>(), plan.data(), plan.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    launch_crop_resize(d_frame.as<uint8_t>(), fw, swap_rb, d_plan.as<int32_t>(), k, d_out.as<uint8_t>(), stream_);
    WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
    WHENET_HIP_CHECK(hipMemcpy(crops_out, d_out.as<void>(), obytes, hipMemcpyDeviceToHost));
}

// The letterbox geometry cache (engine.h): the entry of (fh, fw, out_h, out_w), its tables on the device or their copy queued
// on stream_.  pins: the entry is held until the caller's LbPins goes (a clip needs all of its entries live at once).
Engine::LbEntry& Engine::letterbox_entry(int fh, int fw, int out_h, int out_w, LbPins* pins) {
    ++lb_clock_;
    LbEntry* entry = nullptr;
    for (LbEntry& e : lb_cache_)
        if (e.valid && e.plan.ih == fh && e.plan.iw == fw && e.plan.oh == out_h && e.plan.ow == out_w) entry = &e;
    if (entry != nullptr) {
        ++lb_hits_;
    } else {
        const LetterboxPlan p = build_letterbox_plan(fh, fw, out_h, out_w, &lb_tables_host_);      // (throws before anything changes)
        if (int(lb_cache_.size()) < lb_cache_cap_) {
            lb_cache_.emplace_back();
            entry = &lb_cache_.back();
            entry->copied.create();
        } else {
            for (LbEntry& e : lb_cache_)
                if (e.pins == 0 && (entry == nullptr || e.last_use < entry->last_use)) entry = &e;
            WHENET_REQUIRE(entry != nullptr, WHENET_EINVAL,
                           "letterbox: the clip needs more geometries at once than option letterbox_cache = " + std::to_string(lb_cache_cap_) +
                               " holds");
        }
        ++lb_misses_;
        entry->valid = false;
        if (entry->staged && hipEventQuery(entry->copied) != hipSuccess) {      // its pinned block may still be read by its last copy
            (void)hipGetLastError();
            ++lb_host_waits_;
            WHENET_HIP_CHECK(hipEventSynchronize(entry->copied));
        }
        const size_t tbytes = lb_tables_host_.size() * sizeof(int32_t);
        size_t block = size_t(16) << 10;
        while (block < tbytes) block <<= 1;
        entry->tables.h.grow(block);
        entry->tables.d.grow(block);
        std::memcpy(entry->tables.h.as<void>(), lb_tables_host_.data(), tbytes);
        WHENET_HIP_CHECK(hipMemcpyAsync(entry->tables.d.as<void>(), entry->tables.h.as<void>(), tbytes, hipMemcpyHostToDevice, stream_));
        WHENET_HIP_CHECK(hipEventRecord(entry->copied, stream_));
        entry->staged = true;
        entry->plan = p;
        entry->valid = true;
    }
    entry->last_use = lb_clock_;
    if (pins != nullptr) {
        ++entry->pins;
        pins->held.push_back(entry);
    }
    return *entry;
}

void Engine::add_letterbox_cache_stats(int32_t out[4]) const {
    for (const LbEntry& e : lb_cache_) out[0] += e.valid ? 1 : 0;
    out[1] += lb_hits_, out[2] += lb_misses_, out[3] += lb_host_waits_;
}

void Engine::ensure_letterbox_outputs(size_t mid_bytes, size_t nout, bool want_u8, bool want_f32) {
    if (lb_lut_.bytes() == 0) {
        float lut[256];
        letterbox_float_table(lut);
        lb_lut_.reset(sizeof(lut));
        WHENET_HIP_CHECK(hipMemcpy(lb_lut_.as<void>(), lut, sizeof(lut), hipMemcpyHostToDevice));
    }
    lb_mid_.grow(mid_bytes);
    if (want_u8) lb_u8_.h.grow(nout), lb_u8_.d.grow(nout);
    if (want_f32) lb_f32_.h.grow(nout * sizeof(float)), lb_f32_.d.grow(nout * sizeof(float));
}

// The detector's pre-processing (yolo_v3/utils.py:23-34 + yolo_postprocess.py:191-195) of a frame that is on the device.
// The scratch is one per engine and safe because everything that touches it runs in order on stream_; the tables come from the
// geometry cache, so a change of the frame size (two cameras alternating on one handle) does not wait for the stream.
std::pair<uint8_t*, float*> Engine::enqueue_letterbox(const uint8_t* d_frame, int fh, int fw, int swap_rb, int out_h, int out_w,
                                                      bool want_u8, bool want_f32, int frames) {
    const LbEntry& e = letterbox_entry(fh, fw, out_h, out_w);
    const LetterboxPlan& p = e.plan;
    ensure_letterbox_outputs(size_t(frames) * fh * p.nw * 3, size_t(frames) * out_h * out_w * 3, want_u8, want_f32);
    uint8_t* const d_u8 = want_u8 ? lb_u8_.d.as<uint8_t>() : nullptr;
    float* const d_f32 = want_f32 ? lb_f32_.d.as<float>() : nullptr;
    if (frames == 1)
        launch_letterbox(d_frame, p, swap_rb, e.tables.d.as<int32_t>(), lb_lut_.as<float>(), lb_mid_.as<uint8_t>(), d_u8, d_f32,
                         num_cus_, stream_);
    else
        launch_letterbox_batch(d_frame, frames, p, swap_rb, e.tables.d.as<int32_t>(), lb_lut_.as<float>(), lb_mid_.as<uint8_t>(), d_u8,
                               d_f32, num_cus_, stream_);
    return {d_u8, d_f32};
}

// Frames of their own sizes: every geometry is looked up (or added) and pinned first, so that the F entries are live at once;
// the records go to the two launches by value.
std::pair<uint8_t*, float*> Engine::enqueue_letterbox_mixed(const uint8_t* d_frames, int frames, const int* fh, const int* fw,
                                                            const size_t* off, int swap_rb, int out_h, int out_w, bool want_u8,
                                                            bool want_f32) {
    LbPins pins;
    LetterboxMixed clip{};
    clip.frames = frames;
    clip.total_bytes = off[frames];
    size_t mid = 0;
    int rows = 0;
    for (int f = 0; f < frames; ++f) {
        const LbEntry& e = letterbox_entry(fh[f], fw[f], out_h, out_w, &pins);
        LetterboxMixedFrame& r = clip.f[f];
        r.frame_off = off[f], r.mid_off = mid, r.tab = e.tables.d.as<int32_t>(), r.p = e.plan, r.row0 = rows;
        mid += size_t(fh[f]) * e.plan.nw * 3;
        rows += fh[f];
    }
    clip.total_rows = rows;
    ensure_letterbox_outputs(mid, size_t(frames) * out_h * out_w * 3, want_u8, want_f32);
    uint8_t* const d_u8 = want_u8 ? lb_u8_.d.as<uint8_t>() : nullptr;
    float* const d_f32 = want_f32 ? lb_f32_.d.as<float>() : nullptr;
    launch_letterbox_mixed(d_frames, clip, swap_rb, lb_lut_.as<float>(), lb_mid_.as<uint8_t>(), d_u8, d_f32, num_cus_, stream_);
    return {d_u8, d_f32};
}

void Engine::letterbox_results_to_host(size_t nout, uint8_t* d_u8, float* d_f32, uint8_t* canvas_u8, float* image_f32) {
    if (canvas_u8) WHENET_HIP_CHECK(hipMemcpyAsync(lb_u8_.h.as<void>(), d_u8, nout, hipMemcpyDeviceToHost, stream_));
    if (image_f32) WHENET_HIP_CHECK(hipMemcpyAsync(lb_f32_.h.as<void>(), d_f32, nout * sizeof(float), hipMemcpyDeviceToHost, stream_));
    WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
    if (canvas_u8) std::memcpy(canvas_u8, lb_u8_.h.as<void>(), nout);
    if (image_f32) std::memcpy(image_f32, lb_f32_.h.as<void>(), nout * sizeof(float));
}

void Engine::run_letterbox(const uint8_t* d_frame, int fh, int fw, int swap_rb, int out_h, int out_w, uint8_t* canvas_u8,
                           float* image_f32, int frames) {
    WHENET_REQUIRE(canvas_u8 != nullptr || image_f32 != nullptr, WHENET_EINVAL, "letterbox: both outputs are NULL");
    const auto dev = enqueue_letterbox(d_frame, fh, fw, swap_rb, out_h, out_w, canvas_u8 != nullptr, image_f32 != nullptr, frames);
    letterbox_results_to_host(size_t(frames) * out_h * out_w * 3, dev.first, dev.second, canvas_u8, image_f32);
}

// ---- frames of different sizes ----
void Engine::check_mixed_frames(const char* what, const uint8_t* const* frames, int nframes, const int* fh, const int* fw) {
    const std::string w = what;
    WHENET_REQUIRE(frames != nullptr && fh != nullptr && fw != nullptr, WHENET_EINVAL, w + ": NULL argument");
    WHENET_REQUIRE(nframes >= 1 && nframes <= MIXED_MAX_FRAMES, WHENET_EINVAL,
                   w + ": " + std::to_string(nframes) + " frames: a clip holds 1..16 (the detector's batch limit)");
    for (int f = 0; f < nframes; ++f) {
        WHENET_REQUIRE(frames[f] != nullptr, WHENET_EINVAL, w + ": frame " + std::to_string(f) + " is NULL");
        WHENET_REQUIRE(fh[f] >= 1 && fw[f] >= 1 && fh[f] <= LETTERBOX_MAX_FRAME_SIDE && fw[f] <= LETTERBOX_MAX_FRAME_SIDE, WHENET_EINVAL,
                       w + ": frame " + std::to_string(f) + " is " + std::to_string(fh[f]) + " x " + std::to_string(fw[f]) +
                           ": sides must be 1.." + std::to_string(LETTERBOX_MAX_FRAME_SIDE));
    }
}

void Engine::check_mixed_geometry(const char* what, int frames, const int* fh, const int* fw, int out_h, int out_w) const {
    WHENET_REQUIRE(frames <= lb_cache_cap_, WHENET_EINVAL,
                   std::string(what) + ": " + std::to_string(frames) + " frames of their own sizes need option letterbox_cache >= " +
                       std::to_string(frames) + " (it is " + std::to_string(lb_cache_cap_) + ")");
    for (int f = 0; f < frames; ++f) {
        try {
            (void)letterbox_plan_layout(fh[f], fw[f], out_h, out_w);
        } catch (const Error& e) {
            throw Error(e.code, std::string(what) + ": frame " + std::to_string(f) + ": " + e.what());
        }
    }
}

void Engine::op_letterbox_mixed(const uint8_t* const* frames, int nframes, const int* fh, const int* fw, int swap_rb, int out_h, int out_w,
                                uint8_t* canvas_u8, float* image_f32) {
    DeviceGuard guard(device_);
    check_mixed_frames("op_letterbox_mixed", frames, nframes, fh, fw);
    WHENET_REQUIRE(canvas_u8 != nullptr || image_f32 != nullptr, WHENET_EINVAL, "letterbox: both outputs are NULL");
    check_mixed_geometry("op_letterbox_mixed", nframes, fh, fw, out_h, out_w);
    size_t off[MIXED_MAX_FRAMES + 1] = {};
    for (int f = 0; f < nframes; ++f) off[f + 1] = off[f] + size_t(fh[f]) * fw[f] * 3;
    lb_frame_.grow(off[nframes]);
    for (int f = 0; f < nframes; ++f)
        WHENET_HIP_CHECK(hipMemcpyAsync(lb_frame_.as<uint8_t>() + off[f], frames[f], off[f + 1] - off[f], hipMemcpyHostToDevice, stream_));
    const auto dev = enqueue_letterbox_mixed(lb_frame_.as<uint8_t>(), nframes, fh, fw, off, swap_rb, out_h, out_w, canvas_u8 != nullptr,
                                             image_f32 != nullptr);
    letterbox_results_to_host(size_t(nframes) * out_h * out_w * 3, dev.first, dev.second, canvas_u8, image_f32);
}

// clip_begin for frames of their own sizes: packed back to back (a frame's first byte is unaligned in general) into the slot's
// pinned staging, one H2D; the slot remembers every frame's size and offset.
int Engine::clip_begin_mixed(const uint8_t* const* frames, int nframes, const int* fh, const int* fw, int swap_rb) {
    DeviceGuard guard(device_);
    check_mixed_frames("clip_begin_mixed", frames, nframes, fh, fw);      // (before a slot is taken)
    WHENET_REQUIRE(nframes <= lb_cache_cap_, WHENET_EINVAL,
                   "clip_begin_mixed: " + std::to_string(nframes) + " frames of their own sizes need option letterbox_cache >= " +
                       std::to_string(nframes) + " (it is " + std::to_string(lb_cache_cap_) + ")");
    Slot& slot = *free_slot();
    ensure_slot(slot, 1);
    size_t off[MIXED_MAX_FRAMES + 1] = {};
    for (int f = 0; f < nframes; ++f) off[f + 1] = off[f] + size_t(fh[f]) * fw[f] * 3;
    const size_t bytes = off[nframes];
    slot.frame.h.grow(bytes);
    slot.frame.d.grow(bytes);
    for (int f = 0; f < nframes; ++f) std::memcpy(slot.frame.h.as<uint8_t>() + off[f], frames[f], off[f + 1] - off[f]);
    WHENET_HIP_CHECK(hipMemcpyAsync(slot.frame.d.as<void>(), slot.frame.h.as<void>(), bytes, hipMemcpyHostToDevice, copy_stream()));
    WHENET_HIP_CHECK(hipEventRecord(slot.copied, copy_stream()));
    slot.fh = fh[0], slot.fw = fw[0], slot.swap_rb = swap_rb;
    for (int f = 0; f < nframes; ++f) slot.clip_fh[f] = fh[f], slot.clip_fw[f] = fw[f];
    std::copy(off, off + nframes + 1, slot.clip_off);
    slot.frame_ticket = finish_submission(slot, 0);
    slot.clip_f = nframes;
    slot.clip_mixed = true;
    return slot.frame_ticket;
}

void Engine::op_letterbox(const uint8_t* frame, int fh, int fw, int swap_rb, int out_h, int out_w, uint8_t* canvas_u8,
                          float* image_f32) {
    DeviceGuard guard(device_);
    WHENET_REQUIRE(frame != nullptr, WHENET_EINVAL, "op_letterbox: frame must not be NULL");
    (void)letterbox_plan_layout(fh, fw, out_h, out_w);         // argument errors before anything is copied
    const size_t fbytes = size_t(fh) * fw * 3;
    lb_frame_.grow(fbytes);
    WHENET_HIP_CHECK(hipMemcpyAsync(lb_frame_.as<void>(), frame, fbytes, hipMemcpyHostToDevice, stream_));
    run_letterbox(lb_frame_.as<uint8_t>(), fh, fw, swap_rb, out_h, out_w, canvas_u8, image_f32);
}

void Engine::op_letterbox_batch(const uint8_t* frames, int nframes, int fh, int fw, int swap_rb, int out_h, int out_w, uint8_t* canvas_u8,
                                float* image_f32) {
    DeviceGuard guard(device_);
    WHENET_REQUIRE(frames != nullptr && nframes >= 1 && nframes <= 16, WHENET_EINVAL, "op_letterbox_batch: NULL frames, or a frame count outside 1..16");
    (void)letterbox_plan_layout(fh, fw, out_h, out_w);
    const size_t bytes = size_t(nframes) * fh * fw * 3;
    lb_frame_.grow(bytes);
    WHENET_HIP_CHECK(hipMemcpyAsync(lb_frame_.as<void>(), frames, bytes, hipMemcpyHostToDevice, stream_));
    run_letterbox(lb_frame_.as<uint8_t>(), fh, fw, swap_rb, out_h, out_w, canvas_u8, image_f32, nframes);
}

// The resident-frame form of submit_frame.  frame_begin: pinned staging copy + asynchronous H2D into the slot's frame buffer; the
// ticket is handed out here and the slot stays held.  (`done` is recorded at once with no heads: a collect that comes without
// frame_heads returns no results and frees the slot.)
int Engine::frame_begin(const uint8_t* frame, int fh, int fw, int swap_rb) {
    DeviceGuard guard(device_);
    WHENET_REQUIRE(frame != nullptr && fh > 0 && fw > 0, WHENET_EINVAL, "frame_begin: bad arguments");
    Slot& slot = *free_slot();
    ensure_slot(slot, 1);
    const size_t fbytes = size_t(fh) * fw * 3;
    slot.frame.h.grow(fbytes);
    slot.frame.d.grow(fbytes);
    std::memcpy(slot.frame.h.as<void>(), frame, fbytes);
    WHENET_HIP_CHECK(hipMemcpyAsync(slot.frame.d.as<void>(), slot.frame.h.as<void>(), fbytes, hipMemcpyHostToDevice, copy_stream()));
    WHENET_HIP_CHECK(hipEventRecord(slot.copied, copy_stream()));
    slot.fh = fh, slot.fw = fw, slot.swap_rb = swap_rb;
    slot.frame_ticket = finish_submission(slot, 0);
    return slot.frame_ticket;
}

// frame_begin for the F frames of a clip [F][fh][fw][3]: one pinned staging copy, one H2D; the slot's frame buffer holds them all
int Engine::clip_begin(const uint8_t* frames, int nframes, int fh, int fw, int swap_rb) {
    DeviceGuard guard(device_);
    WHENET_REQUIRE(frames != nullptr && fh > 0 && fw > 0, WHENET_EINVAL, "clip_begin: bad arguments");
    WHENET_REQUIRE(nframes >= 1 && nframes <= 16, WHENET_EINVAL,
                   "clip_begin: " + std::to_string(nframes) + " frames: a clip holds 1..16 (the detector's batch limit)");
    Slot& slot = *free_slot();
    ensure_slot(slot, 1);
    const size_t bytes = size_t(nframes) * fh * fw * 3;
    slot.frame.h.grow(bytes);
    slot.frame.d.grow(bytes);
    std::memcpy(slot.frame.h.as<void>(), frames, bytes);
    WHENET_HIP_CHECK(hipMemcpyAsync(slot.frame.d.as<void>(), slot.frame.h.as<void>(), bytes, hipMemcpyHostToDevice, copy_stream()));
    WHENET_HIP_CHECK(hipEventRecord(slot.copied, copy_stream()));
    slot.fh = fh, slot.fw = fw, slot.swap_rb = swap_rb;
    slot.frame_ticket = finish_submission(slot, 0);
    slot.clip_f = nframes;
    slot.clip_mixed = false;
    return slot.frame_ticket;
}

// ---- YUV 4:2:0 ingest (yuv.hip) ----
namespace {
// where frame f's planes lie in the staging / device plane buffer (src) and its BGR bytes in the frame buffer (dst): both back to
// back, without padding; entry nframes = the bytes of them all
struct YuvLayout {
    size_t src[MIXED_MAX_FRAMES + 1] = {}, dst[MIXED_MAX_FRAMES + 1] = {};
    YuvLayout(const whenet_yuv_frame_t* frames, int nframes) {
        for (int f = 0; f < nframes; ++f) {
            src[f + 1] = src[f] + yuv_plane_bytes(frames[f].h, frames[f].w, frames[f].format);
            dst[f + 1] = dst[f] + size_t(frames[f].h) * frames[f].w * 3;
        }
    }
};
YuvGeom yuv_geom(const whenet_yuv_frame_t& f, size_t src_off, size_t dst_off) {
    YuvGeom g{};
    g.src_off = src_off, g.dst_off = dst_off;
    g.h = f.h, g.w = f.w, g.format = f.format;
    g.k = yuv_coeffs(f.matrix);
    return g;
}
}  // namespace

void Engine::enqueue_yuv_ingest(const whenet_yuv_frame_t* frames, int nframes, uint8_t* h_stage, uint8_t* d_planes, uint8_t* d_bgr,
                                const size_t* off, hipStream_t s) {
    const YuvLayout lay(frames, nframes);
    bool uniform = true;
    for (int f = 0; f < nframes; ++f) {
        yuv_stage_planes(frames[f], h_stage + lay.src[f]);
        uniform = uniform && frames[f].h == frames[0].h && frames[f].w == frames[0].w && frames[f].format == frames[0].format &&
                  frames[f].matrix == frames[0].matrix && off[f] == lay.dst[f];
    }
    WHENET_HIP_CHECK(hipMemcpyAsync(d_planes, h_stage, lay.src[nframes], hipMemcpyHostToDevice, s));
    if (nframes == 1) {
        launch_yuv_to_bgr(d_planes, d_bgr, yuv_geom(frames[0], 0, off[0]), s);
    } else if (uniform) {
        launch_yuv_to_bgr_batch(d_planes, d_bgr, yuv_geom(frames[0], 0, 0), nframes, lay.src[1], lay.dst[1], s);
    } else {
        YuvMixed clip{};
        clip.frames = nframes;
        for (int f = 0; f < nframes; ++f) clip.f[f] = yuv_geom(frames[f], lay.src[f], off[f]);
        launch_yuv_to_bgr_mixed(d_planes, d_bgr, clip, s);
    }
}

void Engine::op_yuv_to_bgr(const whenet_yuv_frame_t* frames, int nframes, uint8_t* const* bgr) {
    DeviceGuard guard(device_);
    check_yuv_frames("op_yuv_to_bgr", frames, nframes);
    WHENET_REQUIRE(bgr != nullptr, WHENET_EINVAL, "op_yuv_to_bgr: NULL argument");
    for (int f = 0; f < nframes; ++f) WHENET_REQUIRE(bgr[f] != nullptr, WHENET_EINVAL, "op_yuv_to_bgr: output " + std::to_string(f) + " is NULL");
    const YuvLayout lay(frames, nframes);
    PinnedBuffer stage;
    DeviceBuffer d_planes, d_bgr;
    stage.reset(lay.src[nframes]);
    d_planes.reset(lay.src[nframes], "hipMalloc");
    d_bgr.reset(lay.dst[nframes], "hipMalloc");
    enqueue_yuv_ingest(frames, nframes, stage.as<uint8_t>(), d_planes.as<uint8_t>(), d_bgr.as<uint8_t>(), lay.dst, stream_);
    WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
    for (int f = 0; f < nframes; ++f)
        WHENET_HIP_CHECK(hipMemcpy(bgr[f], d_bgr.as<uint8_t>() + lay.dst[f], lay.dst[f + 1] - lay.dst[f], hipMemcpyDeviceToHost));
}

// frame_begin from a decoder's planes: the slot ends up exactly as frame_begin(bgr frame, WHENET_BGR) leaves it
int Engine::frame_begin_yuv(const whenet_yuv_frame_t& frame) {
    DeviceGuard guard(device_);
    check_yuv_frames("frame_begin_yuv", &frame, 1);      // (before a slot is taken)
    Slot& slot = *free_slot();
    ensure_slot(slot, 1);
    const YuvLayout lay(&frame, 1);
    // (the size every other user of the staging grows it to; the planes are fewer bytes, but for a packed 4:2:2 frame 1 pixel wide)
    slot.frame.h.grow(std::max(lay.dst[1], lay.src[1]));
    slot.yuv.grow(lay.src[1]);
    slot.frame.d.grow(lay.dst[1]);
    enqueue_yuv_ingest(&frame, 1, slot.frame.h.as<uint8_t>(), slot.yuv.as<uint8_t>(), slot.frame.d.as<uint8_t>(), lay.dst, copy_stream());
    WHENET_HIP_CHECK(hipEventRecord(slot.copied, copy_stream()));
    slot.fh = frame.h, slot.fw = frame.w, slot.swap_rb = 1;
    slot.frame_ticket = finish_submission(slot, 0);
    return slot.frame_ticket;
}

int Engine::clip_begin_yuv(const whenet_yuv_frame_t* frames, int nframes) {
    DeviceGuard guard(device_);
    check_yuv_frames("clip_begin_yuv", frames, nframes);      // (before a slot is taken)
    bool one_size = true;
    for (int f = 1; f < nframes; ++f) one_size = one_size && frames[f].h == frames[0].h && frames[f].w == frames[0].w;
    WHENET_REQUIRE(one_size || nframes <= lb_cache_cap_, WHENET_EINVAL,
                   "clip_begin_yuv: " + std::to_string(nframes) + " frames of their own sizes need option letterbox_cache >= " +
                       std::to_string(nframes) + " (it is " + std::to_string(lb_cache_cap_) + ")");
    Slot& slot = *free_slot();
    ensure_slot(slot, 1);
    const YuvLayout lay(frames, nframes);
    slot.frame.h.grow(std::max(lay.dst[nframes], lay.src[nframes]));
    slot.yuv.grow(lay.src[nframes]);
    slot.frame.d.grow(lay.dst[nframes]);
    enqueue_yuv_ingest(frames, nframes, slot.frame.h.as<uint8_t>(), slot.yuv.as<uint8_t>(), slot.frame.d.as<uint8_t>(), lay.dst, copy_stream());
    WHENET_HIP_CHECK(hipEventRecord(slot.copied, copy_stream()));
    slot.fh = frames[0].h, slot.fw = frames[0].w, slot.swap_rb = 1;
    if (!one_size) {
        for (int f = 0; f < nframes; ++f) slot.clip_fh[f] = frames[f].h, slot.clip_fw[f] = frames[f].w;
        std::copy(lay.dst, lay.dst + nframes + 1, slot.clip_off);
    }
    slot.frame_ticket = finish_submission(slot, 0);
    slot.clip_f = nframes;
    slot.clip_mixed = !one_size;
    return slot.frame_ticket;
}

// ---- ingest from device memory (ingest.hip, yuv.hip; the contract is in engine.h) ----
void Engine::check_device_plane(const std::string& who, const uint8_t* p, int rows, int pitch, int row_bytes) const {
    hipPointerAttribute_t attr{};
    const hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) (void)hipGetLastError();      // (a pointer the runtime does not know: not an error of ours to keep)
    WHENET_REQUIRE(e == hipSuccess && attr.type == hipMemoryTypeDevice && !attr.isManaged, WHENET_EINVAL,
                   who + " is not device memory (hipMalloc'ed memory of device " + std::to_string(device_) +
                       " is needed; host, registered and managed memory go through the host-pointer entry points)");
    WHENET_REQUIRE(attr.device == device_, WHENET_EINVAL,
                   who + " lies on device " + std::to_string(attr.device) + ", the handle runs on device " + std::to_string(device_));
    void* base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(reinterpret_cast<hipDeviceptr_t*>(&base), &size, const_cast<uint8_t*>(p)) != hipSuccess) {
        (void)hipGetLastError();                       // the runtime cannot report the range: the extent goes unchecked
        return;
    }
    const size_t extent = size_t(rows - 1) * size_t(pitch) + size_t(row_bytes);
    const size_t at = size_t(p - static_cast<const uint8_t*>(base));
    WHENET_REQUIRE(p >= static_cast<const uint8_t*>(base) && at <= size && extent <= size - at, WHENET_EINVAL,
                   who + " needs " + std::to_string(extent) + " bytes (" + std::to_string(rows) + " rows of " + std::to_string(row_bytes) +
                       " at pitch " + std::to_string(pitch) + "), its allocation has " + std::to_string(at <= size ? size - at : 0) +
                       " from there on");
}

void Engine::check_device_frames(const char* what, const uint8_t* const* d_frames, const int* pitch, int nframes, const int* fh,
                                 const int* fw) const {
    const std::string w = what;
    WHENET_REQUIRE(d_frames != nullptr && pitch != nullptr, WHENET_EINVAL, w + ": NULL argument");
    check_mixed_frames(what, d_frames, nframes, fh, fw);
    for (int f = 0; f < nframes; ++f) {
        const std::string who = w + ": frame " + std::to_string(f);
        WHENET_REQUIRE(pitch[f] >= 3 * fw[f], WHENET_EINVAL,
                       who + ": pitch " + std::to_string(pitch[f]) + " is below its row of " + std::to_string(3 * fw[f]) + " bytes");
        check_device_plane(who, d_frames[f], fh[f], pitch[f], 3 * fw[f]);
    }
}

void Engine::check_device_yuv_frames(const char* what, const whenet_yuv_frame_t* frames, int nframes) const {
    check_yuv_frames(what, frames, nframes);
    for (int i = 0; i < nframes; ++i) {
        const whenet_yuv_frame_t& f = frames[i];
        for (int p = 0; p < yuv_plane_count(f.format); ++p)
            check_device_plane(std::string(what) + ": frame " + std::to_string(i) + ": plane " + std::to_string(p), f.plane[p],
                               yuv_plane_rows(f.format, p, f.h), f.pitch[p], yuv_plane_row_bytes(f.format, p, f.w));
    }
}

void Engine::ingest_after_caller(Slot& slot, hipStream_t caller) {
    if (!slot.source) slot.source.create();
    WHENET_HIP_CHECK(hipEventRecord(slot.source, caller));
    WHENET_HIP_CHECK(hipStreamWaitEvent(copy_stream(), slot.source, 0));
}

void Engine::ingest_done(Slot& slot, hipStream_t caller) {
    WHENET_HIP_CHECK(hipEventRecord(slot.copied, copy_stream()));
    WHENET_HIP_CHECK(hipStreamWaitEvent(caller, slot.copied, 0));
}

namespace {
PackFrames pack_frames(const uint8_t* const* d_frames, const int* pitch, int nframes, const int* fh, const int* fw, const size_t* off) {
    PackFrames clip{};
    clip.frames = nframes;
    for (int f = 0; f < nframes; ++f) {
        clip.f[f].src = d_frames[f], clip.f[f].dst_off = off[f];
        clip.f[f].pitch = pitch[f], clip.f[f].h = fh[f], clip.f[f].row_bytes = 3 * fw[f];
    }
    return clip;
}
YuvPlanes yuv_planes(const whenet_yuv_frame_t* frames, int nframes, const size_t* off) {
    YuvPlanes clip{};
    clip.frames = nframes;
    for (int f = 0; f < nframes; ++f) {
        YuvPlanesFrame& g = clip.f[f];
        for (int p = 0; p < yuv_plane_count(frames[f].format); ++p) g.plane[p] = frames[f].plane[p], g.pitch[p] = frames[f].pitch[p];
        g.h = frames[f].h, g.w = frames[f].w, g.format = frames[f].format;
        g.k = yuv_coeffs(frames[f].matrix);
        g.dst_off = off[f];
    }
    return clip;
}
// The landing buffer of the two kernel-alone calls: the frames back to back at off[], between two guard zones, every byte set to
// a sentinel before the launch.  to_host waits for the stream, refuses (WHENET_EHIP) if a guard byte has changed -- a kernel wrote
// outside its frames -- and hands every frame to the caller's host array; a byte no thread wrote arrives as the sentinel.
struct GuardedOutput {
    static constexpr size_t GUARD = 64;       // (a multiple of 16: the frames keep the alignments they have in a slot's buffer)
    static constexpr int SENTINEL = 0xA5;
    DeviceBuffer buf;
    size_t bytes;
    GuardedOutput(size_t payload, hipStream_t s) : bytes(payload) {
        buf.reset(payload + 2 * GUARD, "hipMalloc");
        WHENET_HIP_CHECK(hipMemsetAsync(buf.as<void>(), SENTINEL, payload + 2 * GUARD, s));
    }
    uint8_t* frames() const { return buf.as<uint8_t>() + GUARD; }
    void to_host(hipStream_t s, const size_t* off, int nframes, uint8_t* const* out, const char* what) const {
        WHENET_HIP_CHECK(hipStreamSynchronize(s));
        uint8_t guards[2 * GUARD];
        WHENET_HIP_CHECK(hipMemcpy(guards, buf.as<uint8_t>(), GUARD, hipMemcpyDeviceToHost));
        WHENET_HIP_CHECK(hipMemcpy(guards + GUARD, frames() + bytes, GUARD, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < 2 * GUARD; ++i)
            WHENET_REQUIRE(guards[i] == SENTINEL, WHENET_EHIP, std::string(what) + ": the kernel wrote outside its frames (guard byte " +
                                                                   std::to_string(i) + ")");
        for (int f = 0; f < nframes; ++f)
            if (off[f + 1] > off[f]) WHENET_HIP_CHECK(hipMemcpy(out[f], frames() + off[f], off[f + 1] - off[f], hipMemcpyDeviceToHost));
    }
};

// Host SURFACES as a kernel's destination (op_jpeg_decode: one, op_jpeg_decode_clip: one per frame): every plane of every surface
// lies in one GuardedOutput at the caller's pitch and at the caller's address modulo 16, so that a store outside the rows' bytes --
// between two rows, into a neighbouring surface -- meets the sentinel and is seen.  add() every surface, alloc(), launch into
// device(f), to_host().
struct GuardedSurfaces {
    struct Plane {
        size_t off;
        int rows, row_bytes, pitch, surface, index;
        uint8_t* host;
    };
    std::vector<Plane> planes;
    std::vector<whenet_surface_t> d_dst;
    size_t total = 0;
    std::unique_ptr<GuardedOutput> out;
    void add(const whenet_surface_t& dst, int h, int w) {
        int rows[3], row_bytes[3];
        const int np = overlay_surface_planes(dst.format, h, w, rows, row_bytes);
        for (int p = 0; p < np; ++p) {
            const size_t at = ((total + 15) & ~size_t(15)) + (reinterpret_cast<uintptr_t>(dst.plane[p]) & 15);
            total = at + size_t(rows[p] - 1) * size_t(dst.pitch[p]) + size_t(row_bytes[p]);
            planes.push_back({at, rows[p], row_bytes[p], dst.pitch[p], int(d_dst.size()), p, static_cast<uint8_t*>(dst.plane[p])});
        }
        d_dst.push_back(dst);
    }
    void alloc(hipStream_t s) {
        out.reset(new GuardedOutput(total, s));
        for (const Plane& pl : planes) d_dst[size_t(pl.surface)].plane[pl.index] = out->frames() + pl.off;
    }
    const whenet_surface_t* device() const { return d_dst.data(); }
    // waits, checks the guard zones and the bytes between the rows, hands the rows to the caller's surfaces.  whose: "the surface" / "the surfaces"
    void to_host(hipStream_t s, const std::string& what, const char* whose) const {
        const size_t none[1] = {0};
        out->to_host(s, none, 0, nullptr, what.c_str());
        std::vector<uint8_t> back(total), is_row(total, 0);
        WHENET_HIP_CHECK(hipMemcpy(back.data(), out->frames(), total, hipMemcpyDeviceToHost));
        for (const Plane& pl : planes)
            for (int r = 0; r < pl.rows; ++r) {
                const size_t at = pl.off + size_t(r) * size_t(pl.pitch);
                std::memset(is_row.data() + at, 1, size_t(pl.row_bytes));
                std::memcpy(pl.host + size_t(r) * size_t(pl.pitch), back.data() + at, size_t(pl.row_bytes));
            }
        for (size_t i = 0; i < total; ++i)
            WHENET_REQUIRE(is_row[i] || back[i] == GuardedOutput::SENTINEL, WHENET_EHIP,
                           what + ": the kernel wrote outside the rows of " + whose + " (byte " + std::to_string(i) + ")");
    }
};
}  // namespace

void Engine::op_pack_device(const uint8_t* const* d_frames, const int* pitch, int nframes, const int* fh, const int* fw, hipStream_t stream,
                            uint8_t* const* out) {
    DeviceGuard guard(device_);
    check_device_frames("op_pack_device", d_frames, pitch, nframes, fh, fw);
    WHENET_REQUIRE(out != nullptr, WHENET_EINVAL, "op_pack_device: NULL argument");
    for (int f = 0; f < nframes; ++f) WHENET_REQUIRE(out[f] != nullptr, WHENET_EINVAL, "op_pack_device: output " + std::to_string(f) + " is NULL");
    size_t off[MIXED_MAX_FRAMES + 1] = {};
    for (int f = 0; f < nframes; ++f) off[f + 1] = off[f] + size_t(fh[f]) * fw[f] * 3;
    const GuardedOutput d_out(off[nframes], stream_);
    Event after;
    after.create();
    WHENET_HIP_CHECK(hipEventRecord(after, stream));
    WHENET_HIP_CHECK(hipStreamWaitEvent(stream_, after, 0));
    launch_frame_pack(d_out.frames(), pack_frames(d_frames, pitch, nframes, fh, fw, off), stream_);
    d_out.to_host(stream_, off, nframes, out, "op_pack_device");
}

void Engine::op_yuv_to_bgr_device(const whenet_yuv_frame_t* frames, int nframes, hipStream_t stream, uint8_t* const* bgr) {
    DeviceGuard guard(device_);
    check_device_yuv_frames("op_yuv_to_bgr_device", frames, nframes);
    WHENET_REQUIRE(bgr != nullptr, WHENET_EINVAL, "op_yuv_to_bgr_device: NULL argument");
    for (int f = 0; f < nframes; ++f)
        WHENET_REQUIRE(bgr[f] != nullptr, WHENET_EINVAL, "op_yuv_to_bgr_device: output " + std::to_string(f) + " is NULL");
    const YuvLayout lay(frames, nframes);
    const GuardedOutput d_bgr(lay.dst[nframes], stream_);
    Event after;
    after.create();
    WHENET_HIP_CHECK(hipEventRecord(after, stream));
    WHENET_HIP_CHECK(hipStreamWaitEvent(stream_, after, 0));
    launch_yuv_planes_to_bgr(d_bgr.frames(), yuv_planes(frames, nframes, lay.dst), stream_);
    d_bgr.to_host(stream_, lay.dst, nframes, bgr, "op_yuv_to_bgr_device");
}

// frame_begin from device memory: the slot ends up exactly as frame_begin leaves it
int Engine::frame_begin_device(const uint8_t* d_frame, int pitch, int fh, int fw, int swap_rb, hipStream_t stream) {
    DeviceGuard guard(device_);
    check_device_frames("frame_begin_device", &d_frame, &pitch, 1, &fh, &fw);      // (before a slot is taken)
    Slot& slot = *free_slot();
    ensure_slot(slot, 1);
    const size_t off[2] = {0, size_t(fh) * fw * 3};
    slot.frame.d.grow(off[1]);
    ingest_after_caller(slot, stream);
    launch_frame_pack(slot.frame.d.as<uint8_t>(), pack_frames(&d_frame, &pitch, 1, &fh, &fw, off), copy_stream());
    ingest_done(slot, stream);
    slot.fh = fh, slot.fw = fw, slot.swap_rb = swap_rb;
    slot.frame_ticket = finish_submission(slot, 0);
    return slot.frame_ticket;
}

int Engine::clip_begin_device(const uint8_t* const* d_frames, const int* pitch, int nframes, const int* fh, const int* fw, int swap_rb,
                              hipStream_t stream) {
    DeviceGuard guard(device_);
    check_device_frames("clip_begin_device", d_frames, pitch, nframes, fh, fw);      // (before a slot is taken)
    bool one_size = true;
    for (int f = 1; f < nframes; ++f) one_size = one_size && fh[f] == fh[0] && fw[f] == fw[0];
    WHENET_REQUIRE(one_size || nframes <= lb_cache_cap_, WHENET_EINVAL,
                   "clip_begin_device: " + std::to_string(nframes) + " frames of their own sizes need option letterbox_cache >= " +
                       std::to_string(nframes) + " (it is " + std::to_string(lb_cache_cap_) + ")");
    Slot& slot = *free_slot();
    ensure_slot(slot, 1);
    size_t off[MIXED_MAX_FRAMES + 1] = {};
    for (int f = 0; f < nframes; ++f) off[f + 1] = off[f] + size_t(fh[f]) * fw[f] * 3;
    slot.frame.d.grow(off[nframes]);
    ingest_after_caller(slot, stream);
    launch_frame_pack(slot.frame.d.as<uint8_t>(), pack_frames(d_frames, pitch, nframes, fh, fw, off), copy_stream());
    ingest_done(slot, stream);
    slot.fh = fh[0], slot.fw = fw[0], slot.swap_rb = swap_rb;
    if (!one_size) {
        for (int f = 0; f < nframes; ++f) slot.clip_fh[f] = fh[f], slot.clip_fw[f] = fw[f];
        std::copy(off, off + nframes + 1, slot.clip_off);
    }
    slot.frame_ticket = finish_submission(slot, 0);
    slot.clip_f = nframes;
    slot.clip_mixed = !one_size;
    return slot.frame_ticket;
}

// frame_begin_yuv from planes in device memory: the slot ends up exactly as frame_begin_yuv leaves it
int Engine::frame_begin_yuv_device(const whenet_yuv_frame_t& frame, hipStream_t stream) {
    DeviceGuard guard(device_);
    check_device_yuv_frames("frame_begin_yuv_device", &frame, 1);      // (before a slot is taken)
    Slot& slot = *free_slot();
    ensure_slot(slot, 1);
    const YuvLayout lay(&frame, 1);
    slot.frame.d.grow(lay.dst[1]);
    ingest_after_caller(slot, stream);
    launch_yuv_planes_to_bgr(slot.frame.d.as<uint8_t>(), yuv_planes(&frame, 1, lay.dst), copy_stream());
    ingest_done(slot, stream);
    slot.fh = frame.h, slot.fw = frame.w, slot.swap_rb = 1;
    slot.frame_ticket = finish_submission(slot, 0);
    return slot.frame_ticket;
}

int Engine::clip_begin_yuv_device(const whenet_yuv_frame_t* frames, int nframes, hipStream_t stream) {
    DeviceGuard guard(device_);
    check_device_yuv_frames("clip_begin_yuv_device", frames, nframes);      // (before a slot is taken)
    bool one_size = true;
    for (int f = 1; f < nframes; ++f) one_size = one_size && frames[f].h == frames[0].h && frames[f].w == frames[0].w;
    WHENET_REQUIRE(one_size || nframes <= lb_cache_cap_, WHENET_EINVAL,
                   "clip_begin_yuv_device: " + std::to_string(nframes) + " frames of their own sizes need option letterbox_cache >= " +
                       std::to_string(nframes) + " (it is " + std::to_string(lb_cache_cap_) + ")");
    Slot& slot = *free_slot();
    ensure_slot(slot, 1);
    const YuvLayout lay(frames, nframes);
    slot.frame.d.grow(lay.dst[nframes]);
    ingest_after_caller(slot, stream);
    launch_yuv_planes_to_bgr(slot.frame.d.as<uint8_t>(), yuv_planes(frames, nframes, lay.dst), copy_stream());
    ingest_done(slot, stream);
    slot.fh = frames[0].h, slot.fw = frames[0].w, slot.swap_rb = 1;
    if (!one_size) {
        for (int f = 0; f < nframes; ++f) slot.clip_fh[f] = frames[f].h, slot.clip_fw[f] = frames[f].w;
        std::copy(lay.dst, lay.dst + nframes + 1, slot.clip_off);
    }
    slot.frame_ticket = finish_submission(slot, 0);
    slot.clip_f = nframes;
    slot.clip_mixed = !one_size;
    return slot.frame_ticket;
}

// ---- extended YUV ingest (yuvx.hip; the contract is in include/whenet_hip_yuv_ext.h) ----
void Engine::check_device_yuvx_frames(const char* what, const whenet_yuvx_frame_t* frames, int nframes) const {
    check_yuvx_frames(what, frames, nframes);
    for (int i = 0; i < nframes; ++i) {
        const whenet_yuvx_frame_t& f = frames[i];
        for (int p = 0; p < yuvx_plane_count(f.layout); ++p)
            check_device_plane(std::string(what) + ": frame " + std::to_string(i) + ": plane " + std::to_string(p), f.plane[p],
                               yuvx_plane_rows(f.layout, p, f.h), f.pitch[p], yuvx_plane_row_bytes(f.layout, p, f.w, f.container >> 3));
    }
}

namespace {
YuvxClip yuvx_clip(const whenet_yuvx_frame_t* frames, int nframes, const size_t* src, const size_t* dst) {
    YuvxClip clip{};
    clip.frames = nframes;
    for (int f = 0; f < nframes; ++f) clip.f[f] = yuvx_frame(frames[f], src ? src[f] : 0, dst[f]);
    return clip;
}
}  // namespace

void Engine::enqueue_yuvx_ingest(const whenet_yuvx_frame_t* frames, int nframes, uint8_t* h_stage, uint8_t* d_planes, uint8_t* d_bgr,
                                 const size_t* off, hipStream_t s) {
    const YuvxLayout lay(frames, nframes);
    for (int f = 0; f < nframes; ++f) {
        if (f > 0) {                                   // (the padding byte in front of a 16-bit frame, if there is one)
            const size_t prev_end = lay.src[f - 1] + yuvx_plane_bytes(frames[f - 1].h, frames[f - 1].w, frames[f - 1].layout, frames[f - 1].container);
            if (lay.src[f] > prev_end) h_stage[prev_end] = 0;
        }
        yuvx_stage_planes(frames[f], h_stage + lay.src[f]);
    }
    WHENET_HIP_CHECK(hipMemcpyAsync(d_planes, h_stage, lay.end, hipMemcpyHostToDevice, s));
    launch_yuvx_to_bgr(d_planes, d_bgr, yuvx_clip(frames, nframes, lay.src, off), s);
}

void Engine::op_yuvx_to_bgr(const whenet_yuvx_frame_t* frames, int nframes, uint8_t* const* bgr) {
    DeviceGuard guard(device_);
    check_yuvx_frames("op_yuvx_to_bgr", frames, nframes);
    WHENET_REQUIRE(bgr != nullptr, WHENET_EINVAL, "op_yuvx_to_bgr: NULL argument");
    for (int f = 0; f < nframes; ++f) WHENET_REQUIRE(bgr[f] != nullptr, WHENET_EINVAL, "op_yuvx_to_bgr: output " + std::to_string(f) + " is NULL");
    const YuvxLayout lay(frames, nframes);
    PinnedBuffer stage;
    DeviceBuffer d_planes;
    stage.reset(lay.end);
    d_planes.reset(lay.end, "hipMalloc");
    const GuardedOutput d_bgr(lay.dst[nframes], stream_);
    enqueue_yuvx_ingest(frames, nframes, stage.as<uint8_t>(), d_planes.as<uint8_t>(), d_bgr.frames(), lay.dst, stream_);
    d_bgr.to_host(stream_, lay.dst, nframes, bgr, "op_yuvx_to_bgr");
}

void Engine::op_yuvx_to_bgr_device(const whenet_yuvx_frame_t* frames, int nframes, hipStream_t stream, uint8_t* const* bgr) {
    DeviceGuard guard(device_);
    check_device_yuvx_frames("op_yuvx_to_bgr_device", frames, nframes);
    WHENET_REQUIRE(bgr != nullptr, WHENET_EINVAL, "op_yuvx_to_bgr_device: NULL argument");
    for (int f = 0; f < nframes; ++f)
        WHENET_REQUIRE(bgr[f] != nullptr, WHENET_EINVAL, "op_yuvx_to_bgr_device: output " + std::to_string(f) + " is NULL");
    const YuvxLayout lay(frames, nframes);
    const GuardedOutput d_bgr(lay.dst[nframes], stream_);
    Event after;
    after.create();
    WHENET_HIP_CHECK(hipEventRecord(after, stream));
    WHENET_HIP_CHECK(hipStreamWaitEvent(stream_, after, 0));
    launch_yuvx_planes_to_bgr(d_bgr.frames(), yuvx_clip(frames, nframes, nullptr, lay.dst), stream_);
    d_bgr.to_host(stream_, lay.dst, nframes, bgr, "op_yuvx_to_bgr_device");
}

// frame_begin_yuv / clip_begin_yuv / frame_begin_yuv_device / clip_begin_yuv_device for whenet_yuvx_frame_t: the slot ends up
// exactly as the call of that name leaves it
int Engine::begin_yuvx(const char* what, const whenet_yuvx_frame_t* frames, int nframes, bool clip, bool device, hipStream_t stream) {
    DeviceGuard guard(device_);
    if (device) check_device_yuvx_frames(what, frames, nframes);      // (before a slot is taken)
    else check_yuvx_frames(what, frames, nframes);
    WHENET_REQUIRE(clip || nframes == 1, WHENET_EINVAL, std::string(what) + ": one frame");
    bool one_size = true;
    for (int f = 1; f < nframes; ++f) one_size = one_size && frames[f].h == frames[0].h && frames[f].w == frames[0].w;
    WHENET_REQUIRE(one_size || nframes <= lb_cache_cap_, WHENET_EINVAL,
                   std::string(what) + ": " + std::to_string(nframes) + " frames of their own sizes need option letterbox_cache >= " +
                       std::to_string(nframes) + " (it is " + std::to_string(lb_cache_cap_) + ")");
    Slot& slot = *free_slot();
    ensure_slot(slot, 1);
    const YuvxLayout lay(frames, nframes);
    slot.frame.d.grow(lay.dst[nframes]);
    if (device) {
        ingest_after_caller(slot, stream);
        launch_yuvx_planes_to_bgr(slot.frame.d.as<uint8_t>(), yuvx_clip(frames, nframes, nullptr, lay.dst), copy_stream());
        ingest_done(slot, stream);
    } else {
        // (the size every other user of the staging grows it to; the planes of a 16-bit 4:4:4 frame are more bytes than the frame)
        slot.frame.h.grow(std::max(lay.dst[nframes], lay.end));
        slot.yuv.grow(lay.end);
        enqueue_yuvx_ingest(frames, nframes, slot.frame.h.as<uint8_t>(), slot.yuv.as<uint8_t>(), slot.frame.d.as<uint8_t>(), lay.dst, copy_stream());
        WHENET_HIP_CHECK(hipEventRecord(slot.copied, copy_stream()));
    }
    slot.fh = frames[0].h, slot.fw = frames[0].w, slot.swap_rb = 1;
    if (clip && !one_size) {
        for (int f = 0; f < nframes; ++f) slot.clip_fh[f] = frames[f].h, slot.clip_fw[f] = frames[f].w;
        std::copy(lay.dst, lay.dst + nframes + 1, slot.clip_off);
    }
    slot.frame_ticket = finish_submission(slot, 0);
    if (clip) slot.clip_f = nframes, slot.clip_mixed = !one_size;
    return slot.frame_ticket;
}

Engine::Slot& Engine::resident_slot(int ticket, const char* what, int holds) {
    for (Slot& s : slots_)
        if (s.busy && s.ticket == ticket) {
            WHENET_REQUIRE(s.frame_ticket == ticket, WHENET_EINVAL,
                           std::string(what) + ": ticket " + std::to_string(ticket) +
                               " holds no frame that waits for its heads (not from frame_begin, or its heads are already enqueued)");
            WHENET_REQUIRE(holds != HOLDS_FRAME || s.clip_f == 0, WHENET_EINVAL,
                           std::string(what) + ": ticket " + std::to_string(ticket) + " holds a clip (clip_begin): clip_detect_heads enqueues it");
            WHENET_REQUIRE(holds != HOLDS_CLIP || s.clip_f > 0, WHENET_EINVAL,
                           std::string(what) + ": ticket " + std::to_string(ticket) + " holds a single frame (frame_begin), not a clip");
            return s;
        }
    throw Error(WHENET_EINVAL, std::string(what) + ": unknown or already collected ticket " + std::to_string(ticket));
}

void Engine::frame_letterbox(int ticket, int out_h, int out_w, uint8_t* canvas_u8, float* image_f32) {
    DeviceGuard guard(device_);
    Slot& slot = resident_slot(ticket, "frame_letterbox");
    WHENET_HIP_CHECK(hipStreamWaitEvent(stream_, slot.copied, 0));
    run_letterbox(slot.frame.d.as<uint8_t>(), slot.fh, slot.fw, slot.swap_rb, out_h, out_w, canvas_u8, image_f32);
}

// submit_frame from its crop plans on: nothing differs except that the frame is already on the device.
void Engine::frame_heads(int ticket, const int32_t* rects, int k) {
    DeviceGuard guard(device_);
    Slot& slot = resident_slot(ticket, "frame_heads", k == 0 ? HOLDS_EITHER : HOLDS_FRAME);      // (no heads: releases a clip as well)
    WHENET_REQUIRE(k >= 0 && (k == 0 || rects != nullptr), WHENET_EINVAL, "frame_heads: bad arguments");
    check_rects(slot.fh, slot.fw, rects, k);
    if (k > 0) {
        require_model();
        ensure_capacity(k);
        ensure_slot(slot, k);
        ensure_slot_frame(slot, size_t(slot.fh) * slot.fw * 3, k);
        int32_t* const h_plan = slot.plan.h.as<int32_t>();
        for (int i = 0; i < k; ++i) build_crop_plan(rects + 4 * i, h_plan + size_t(i) * CROP_PLAN_INTS);
        WHENET_HIP_CHECK(hipMemcpyAsync(slot.plan.d.as<void>(), h_plan, size_t(k) * CROP_PLAN_INTS * sizeof(int32_t),
                                        hipMemcpyHostToDevice, copy_stream()));
        WHENET_HIP_CHECK(hipEventRecord(slot.copied, copy_stream()));      // (in order behind the frame's copy)
        WHENET_HIP_CHECK(hipStreamWaitEvent(stream_, slot.copied, 0));
        launch_crop_resize(slot.frame.d.as<uint8_t>(), slot.fw, slot.swap_rb, slot.plan.d.as<int32_t>(), k, slot.in.d.as<uint8_t>(), stream_);
        run_forward(slot.in.d.as<uint8_t>(), k, slot.dev(), stream_);
        copy_results_async(slot.host(), slot.dev(), k, stream_);
    }
    WHENET_HIP_CHECK(hipEventRecord(slot.done, stream_));
    slot.n = k;
    slot.frame_ticket = -1;
    if (slot.clip_f == 0) slot.ann_kind = Slot::ANN_PLANS;      // (a released clip has nothing to annotate)
}

// yolo_eval (yolo_v3/model.py:193-232) on host feature maps: H2D, decode + NMS on the device, the selected boxes
// back, concatenated class by class like the reference.  Returns the number of detections.
int Engine::yolo_eval(const float* const* feats, const int* grid_h, const int* grid_w, int num_layers,
                      const float* anchors, int num_anchors, int num_classes, float image_h, float image_w,
                      float score_threshold, float iou_threshold, int max_boxes, float* boxes, float* scores,
                      int32_t* classes, int32_t* index, float* all_boxes, float* all_scores) {
    DeviceGuard guard(device_);
    return yolo_eval_maps(feats, false, grid_h, grid_w, num_layers, anchors, num_anchors, num_classes, image_h, image_w, score_threshold,
                          iou_threshold, max_boxes, boxes, scores, classes, index, all_boxes, all_scores);
}

// on_device: the maps are where the detector body left them (detector.cpp); nothing is uploaded
YoloArgs Engine::enqueue_yolo_eval(const float* const* feats, bool on_device, const int* grid_h, const int* grid_w, int num_layers,
                                   const float* anchors, int num_anchors, int num_classes, float image_h, float image_w,
                                   float score_threshold, float iou_threshold, int max_boxes, bool want_all_scores, int images,
                                   const float* image_shapes) {
    WHENET_REQUIRE(feats && grid_h && grid_w && anchors, WHENET_EINVAL, "yolo_eval: NULL argument");
    WHENET_REQUIRE(images >= 1 && images <= 16, WHENET_EINVAL, "yolo_eval: 1..16 images");
    WHENET_REQUIRE((num_layers == 3 && num_anchors == 9) || (num_layers == 2 && num_anchors == 6), WHENET_EINVAL,
                   "yolo_eval: 3 maps with 9 anchors or 2 maps with 6 (model.py:203)");
    WHENET_REQUIRE(num_classes >= 1 && num_classes <= 1024 && image_h > 0 && image_w > 0, WHENET_EINVAL,
                   "yolo_eval: bad num_classes / image shape");
    WHENET_REQUIRE(max_boxes >= 1, WHENET_EINVAL, "yolo_eval: max_boxes must be >= 1");      // (any value, as model.py:193)
    // model.py:203: anchor_mask = [[6,7,8],[3,4,5],[0,1,2]] for 3 maps, [[3,4,5],[1,2,3]] for 2
    static const int ANCHOR_MASK3[3][3] = {{6, 7, 8}, {3, 4, 5}, {0, 1, 2}};
    static const int ANCHOR_MASK2[2][3] = {{3, 4, 5}, {1, 2, 3}};
    YoloArgs a{};
    a.images = images;
    a.num_layers = num_layers;
    a.num_classes = num_classes;
    a.na = 3;
    a.input_h = float(grid_h[0] * 32);                    // model.py:204
    a.input_w = float(grid_w[0] * 32);
    a.image_h = image_h;
    a.image_w = image_w;
    {
        const MixedFrameCorrection c = yolo_correction(a.input_h, a.input_w, image_h, image_w);
        a.off_y = c.off_y, a.off_x = c.off_x, a.scale_y = c.scale_y, a.scale_x = c.scale_x;
    }
    YoloMixed mixed{};                                      // every image its own shape: the values of each, computed as for one image
    if (image_shapes != nullptr) {
        for (int f = 0; f < images; ++f) {
            const float h = image_shapes[2 * f], w = image_shapes[2 * f + 1];
            WHENET_REQUIRE(h > 0 && w > 0, WHENET_EINVAL, "yolo_eval: bad shape of image " + std::to_string(f));
            mixed.img[f] = yolo_correction(a.input_h, a.input_w, h, w);
        }
    }
    a.score_thr = score_threshold;
    a.iou_thr = iou_threshold;
    // one engine-owned scratch block, grown on demand (round 2 paid ~10 hipMalloc/hipFree per frame here)
    struct Carver {
        size_t used = 0;
        size_t add(size_t nbytes) {
            const size_t off = (used + 255) & ~size_t(255);
            used = off + (nbytes ? nbytes : 16);
            return off;
        }
    };
    int N = 0;
    const size_t per = size_t(5 + num_classes) * 3;
    size_t feat_off[3] = {0, 0, 0}, feat_bytes[3] = {0, 0, 0};
    Carver cv;
    for (int l = 0; l < num_layers; ++l) {
        WHENET_REQUIRE(feats[l] && grid_h[l] > 0 && grid_w[l] > 0 && grid_h[l] <= 4096 && grid_w[l] <= 4096, WHENET_EINVAL,
                       "yolo_eval: bad feature map");
        YoloLayer& L = a.layer[l];
        L.gh = grid_h[l];
        L.gw = grid_w[l];
        L.first = N;
        for (int k = 0; k < 3; ++k) {
            const int m = (num_layers == 3) ? ANCHOR_MASK3[l][k] : ANCHOR_MASK2[l][k];
            L.anchor[k][0] = anchors[2 * m];
            L.anchor[k][1] = anchors[2 * m + 1];
        }
        feat_bytes[l] = size_t(images) * L.gh * L.gw * per * sizeof(float);
        if (!on_device) feat_off[l] = cv.add(feat_bytes[l]);
        N += L.gh * L.gw * 3;
    }
    a.N = N;
    a.NP = 1;
    while (a.NP < N) a.NP <<= 1;
    if (max_boxes > N) max_boxes = N;                       // (no more selections than boxes)
    a.max_boxes = max_boxes;
    const size_t C = size_t(num_classes), MB = size_t(max_boxes), F = size_t(images);      // (every array: [images][...])
    const size_t o_boxes = cv.add(F * size_t(N) * 4 * sizeof(float));
    const size_t o_all = want_all_scores ? cv.add(F * size_t(N) * C * sizeof(float)) : 0;
    const size_t o_counts = cv.add(F * C * sizeof(int));
    const size_t o_keys = cv.add(F * C * size_t(a.NP) * sizeof(unsigned long long));
    const size_t o_ob = cv.add(F * C * MB * 4 * sizeof(float));
    const size_t o_os = cv.add(F * C * MB * sizeof(float));
    const size_t o_oi = cv.add(F * C * MB * sizeof(int));
    const size_t o_oc = cv.add(F * C * sizeof(int));
    if (cv.used > yolo_scratch_.bytes()) {
        WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
        yolo_scratch_.reset(cv.used, "yolo_eval scratch");
    }
    unsigned char* base = yolo_scratch_.as<unsigned char>();
    for (int l = 0; l < num_layers; ++l) {
        if (on_device) {
            a.layer[l].feats = feats[l];
            continue;
        }
        float* d = reinterpret_cast<float*>(base + feat_off[l]);
        WHENET_HIP_CHECK(hipMemcpyAsync(d, feats[l], feat_bytes[l], hipMemcpyHostToDevice, stream_));
        a.layer[l].feats = d;
    }
    a.boxes = reinterpret_cast<float*>(base + o_boxes);
    a.all_scores = want_all_scores ? reinterpret_cast<float*>(base + o_all) : nullptr;
    a.counts = reinterpret_cast<int*>(base + o_counts);
    a.keys = reinterpret_cast<unsigned long long*>(base + o_keys);
    a.out_boxes = reinterpret_cast<float*>(base + o_ob);
    a.out_scores = reinterpret_cast<float*>(base + o_os);
    a.out_index = reinterpret_cast<int*>(base + o_oi);
    a.out_count = reinterpret_cast<int*>(base + o_oc);
    launch_yolo_eval(a, stream_, image_shapes != nullptr ? &mixed : nullptr);
    return a;
}

int Engine::yolo_eval_maps(const float* const* feats, bool on_device, const int* grid_h, const int* grid_w, int num_layers,
                           const float* anchors, int num_anchors, int num_classes, float image_h, float image_w,
                           float score_threshold, float iou_threshold, int max_boxes, float* boxes, float* scores,
                           int32_t* classes, int32_t* index, float* all_boxes, float* all_scores) {
    WHENET_REQUIRE(boxes && scores && classes, WHENET_EINVAL, "yolo_eval: NULL argument");
    const YoloArgs a = enqueue_yolo_eval(feats, on_device, grid_h, grid_w, num_layers, anchors, num_anchors, num_classes, image_h, image_w,
                                         score_threshold, iou_threshold, max_boxes, all_scores != nullptr);
    const int N = a.N;
    const size_t C = size_t(num_classes), MB = size_t(a.max_boxes);
    // The per-class counts first, then ONLY the selected rows, straight into the caller's arrays (model.py:227-229:
    // concatenated class by class).  Round 3 copied all C x max_boxes slots into temporaries: ~20 MB per frame for 80
    // classes x 10,647 boxes where the reference returns a handful of detections.
    yolo_counts_.resize(C);
    WHENET_HIP_CHECK(hipMemcpyAsync(yolo_counts_.data(), a.out_count, C * sizeof(int), hipMemcpyDeviceToHost, stream_));
    if (all_boxes)
        WHENET_HIP_CHECK(hipMemcpyAsync(all_boxes, a.boxes, size_t(N) * 4 * sizeof(float), hipMemcpyDeviceToHost, stream_));
    if (all_scores)
        WHENET_HIP_CHECK(hipMemcpyAsync(all_scores, a.all_scores, size_t(N) * C * sizeof(float), hipMemcpyDeviceToHost, stream_));
    WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
    int out = 0;
    for (size_t c = 0; c < C; ++c) {
        const size_t k = size_t(yolo_counts_[c]);
        if (k == 0) continue;
        WHENET_HIP_CHECK(hipMemcpyAsync(boxes + size_t(out) * 4, a.out_boxes + c * MB * 4, k * 4 * sizeof(float),
                                        hipMemcpyDeviceToHost, stream_));
        WHENET_HIP_CHECK(hipMemcpyAsync(scores + out, a.out_scores + c * MB, k * sizeof(float), hipMemcpyDeviceToHost, stream_));
        if (index)
            WHENET_HIP_CHECK(hipMemcpyAsync(index + out, a.out_index + c * MB, k * sizeof(int), hipMemcpyDeviceToHost, stream_));
        for (size_t j = 0; j < k; ++j) classes[size_t(out) + j] = int32_t(c);
        out += int(k);
    }
    WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
    return out;
}

// What frame_detect_heads (detector.cpp) enqueued: one wait, then the detections and the results of their heads.
int Engine::collect_detect(int ticket, int capacity, float* boxes, float* scores, int32_t* classes, int32_t* rects, int32_t* valid,
                           float* ypr, int32_t* argmax, float* logits) {
    DeviceGuard guard(device_);
    Slot* slot = nullptr;
    for (Slot& s : slots_)
        if (s.busy && s.ticket == ticket) slot = &s;
    WHENET_REQUIRE(slot != nullptr, WHENET_EINVAL, "unknown or already collected ticket " + std::to_string(ticket));
    WHENET_REQUIRE(slot->det_cap >= 0, WHENET_EINVAL,
                   "collect_detect: ticket " + std::to_string(ticket) + " was not submitted by frame_detect_heads");
    WHENET_REQUIRE(boxes && scores && classes && rects && valid && ypr, WHENET_EINVAL, "collect_detect: NULL argument");
    WHENET_REQUIRE(capacity >= slot->det_cap, WHENET_EINVAL,
                   "collect_detect: capacity " + std::to_string(capacity) + " is below the submission's " + std::to_string(slot->det_cap) +
                       " rows (classes x max_boxes)");
    WHENET_HIP_CHECK(hipEventSynchronize(slot->done));
    finish_annotations(*slot);
    const DetRows rows(slot->det_cap);
    void* const base = slot->det.h.as<void>();
    const int count = std::max(0, std::min(*rows.count(base), slot->det_cap));
    const size_t n = size_t(count);
    std::memcpy(boxes, rows.boxes(base), n * 4 * sizeof(float));
    std::memcpy(scores, rows.scores(base), n * sizeof(float));
    std::memcpy(classes, rows.classes(base), n * sizeof(int32_t));
    std::memcpy(rects, rows.rects(base), n * 4 * sizeof(int32_t));
    std::memcpy(valid, rows.valid(base), n * sizeof(int32_t));
    copy_results_host(Results{ypr, argmax, logits}, slot->host(), count);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (size_t i = 0; i < n; ++i) {
        if (valid[i]) continue;
        std::fill(ypr + i * 3, ypr + i * 3 + 3, nan);
        if (argmax) std::fill(argmax + i * 3, argmax + i * 3 + 3, -1);
        if (logits) std::fill(logits + i * N_LOGITS, logits + (i + 1) * N_LOGITS, nan);
    }
    slot->busy = false;
    slot->det_cap = -1;
    return count;
}

// yolo_eval over the images of a batch (host maps [images][gh][gw][A (5 + C)] per layer): one upload, the two launches with the
// image as a grid dimension, the selected rows of every image back in one wait, concatenated class by class per image.
void Engine::yolo_eval_batch(const float* const* feats, int images, const int* grid_h, const int* grid_w, int num_layers,
                             const float* anchors, int num_anchors, int num_classes, float image_h, float image_w, float score_threshold,
                             float iou_threshold, int max_boxes, float* boxes, float* scores, int32_t* classes, int32_t* index,
                             int32_t* counts) {
    DeviceGuard guard(device_);
    WHENET_REQUIRE(boxes && scores && classes && counts, WHENET_EINVAL, "yolo_eval_batch: NULL argument");
    const YoloArgs a = enqueue_yolo_eval(feats, false, grid_h, grid_w, num_layers, anchors, num_anchors, num_classes, image_h, image_w,
                                         score_threshold, iou_threshold, max_boxes, false, images);
    yolo_batch_to_host(a, boxes, scores, classes, index, counts);
}

void Engine::yolo_eval_mixed(const float* const* feats, int images, const int* grid_h, const int* grid_w, int num_layers,
                             const float* anchors, int num_anchors, int num_classes, const float* image_shapes, float score_threshold,
                             float iou_threshold, int max_boxes, float* boxes, float* scores, int32_t* classes, int32_t* index,
                             int32_t* counts) {
    DeviceGuard guard(device_);
    WHENET_REQUIRE(boxes && scores && classes && counts && image_shapes, WHENET_EINVAL, "yolo_eval_mixed: NULL argument");
    WHENET_REQUIRE(images >= 1 && images <= MIXED_MAX_FRAMES, WHENET_EINVAL, "yolo_eval: 1..16 images");
    const YoloArgs a = enqueue_yolo_eval(feats, false, grid_h, grid_w, num_layers, anchors, num_anchors, num_classes, image_shapes[0],
                                         image_shapes[1], score_threshold, iou_threshold, max_boxes, false, images, image_shapes);
    yolo_batch_to_host(a, boxes, scores, classes, index, counts);
}

// the selected rows of every image of a batch back in one wait, concatenated class by class per image
void Engine::yolo_batch_to_host(const YoloArgs& a, float* boxes, float* scores, int32_t* classes, int32_t* index, int32_t* counts) {
    const int num_classes = a.num_classes, images = a.images;
    const size_t C = size_t(num_classes), MB = size_t(a.max_boxes), F = size_t(images), S = F * C * MB;
    std::vector<float> ob(S * 4), os(S);
    std::vector<int> oi(S), oc(F * C);
    WHENET_HIP_CHECK(hipMemcpyAsync(ob.data(), a.out_boxes, S * 4 * sizeof(float), hipMemcpyDeviceToHost, stream_));
    WHENET_HIP_CHECK(hipMemcpyAsync(os.data(), a.out_scores, S * sizeof(float), hipMemcpyDeviceToHost, stream_));
    WHENET_HIP_CHECK(hipMemcpyAsync(oi.data(), a.out_index, S * sizeof(int), hipMemcpyDeviceToHost, stream_));
    WHENET_HIP_CHECK(hipMemcpyAsync(oc.data(), a.out_count, F * C * sizeof(int), hipMemcpyDeviceToHost, stream_));
    WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
    for (size_t f = 0; f < F; ++f) {
        size_t out = f * C * MB;                            // image f's rows of the caller's arrays
        const size_t first = out;
        for (size_t c = 0; c < C; ++c) {
            const size_t src = (f * C + c) * MB, k = size_t(std::max(0, std::min(oc[f * C + c], int(MB))));
            std::memcpy(boxes + out * 4, ob.data() + src * 4, k * 4 * sizeof(float));
            std::memcpy(scores + out, os.data() + src, k * sizeof(float));
            if (index) std::memcpy(index + out, oi.data() + src, k * sizeof(int));
            for (size_t j = 0; j < k; ++j) classes[out + j] = int32_t(c);
            out += k;
        }
        counts[f] = int32_t(out - first);
    }
}

// What clip_detect_heads (detector.cpp) enqueued: one wait, then every frame's detections over its K slots and, scattered by `row`,
// the results of the heads that got a forward row.
void Engine::collect_clip(int ticket, int capacity, int* nframes, int32_t* counts, float* boxes, float* scores, int32_t* classes,
                          int32_t* rects, int32_t* valid, int32_t* row, float* ypr, int32_t* argmax, float* logits, int* rows_used,
                          int* overflow) {
    DeviceGuard guard(device_);
    Slot* slot = nullptr;
    for (Slot& s : slots_)
        if (s.busy && s.ticket == ticket) slot = &s;
    WHENET_REQUIRE(slot != nullptr, WHENET_EINVAL, "unknown or already collected ticket " + std::to_string(ticket));
    WHENET_REQUIRE(slot->clip_cap >= 0, WHENET_EINVAL,
                   "collect_clip: ticket " + std::to_string(ticket) + " was not submitted by clip_detect_heads");
    WHENET_REQUIRE(nframes && counts && boxes && scores && classes && rects && valid && row && ypr && rows_used && overflow, WHENET_EINVAL,
                   "collect_clip: NULL argument");
    const int F = slot->clip_f, K = slot->clip_cap, M = slot->clip_heads;
    WHENET_REQUIRE(capacity >= F * K, WHENET_EINVAL,
                   "collect_clip: capacity " + std::to_string(capacity) + " is below the submission's " + std::to_string(F * K) +
                       " rows (frames x classes x max_boxes)");
    WHENET_HIP_CHECK(hipEventSynchronize(slot->done));
    finish_annotations(*slot);
    const ClipRows rows(F, K, M);
    void* const base = slot->det.h.as<void>();
    const size_t S = rows.S;
    *nframes = F;
    *rows_used = std::max(0, std::min(*rows.rows_used(base), M));
    *overflow = std::max(0, *rows.overflow(base));
    for (int f = 0; f < F; ++f) counts[f] = std::max(0, std::min(rows.count(base)[f], K));
    std::memcpy(boxes, rows.boxes(base), S * 4 * sizeof(float));
    std::memcpy(scores, rows.scores(base), S * sizeof(float));
    std::memcpy(classes, rows.classes(base), S * sizeof(int32_t));
    std::memcpy(rects, rows.rects(base), S * 4 * sizeof(int32_t));
    std::memcpy(valid, rows.valid(base), S * sizeof(int32_t));
    const Results res = slot->host();
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (size_t s = 0; s < S; ++s) {
        const int r = rows.row(base)[s];
        const bool has = r >= 0 && r < M;
        row[s] = has ? r : -1;
        if (has) {
            std::memcpy(ypr + s * 3, res.ypr + size_t(r) * 3, 3 * sizeof(float));
            if (argmax) std::memcpy(argmax + s * 3, res.amax + size_t(r) * 3, 3 * sizeof(int32_t));
            if (logits) std::memcpy(logits + s * N_LOGITS, res.logits + size_t(r) * N_LOGITS, N_LOGITS * sizeof(float));
        } else {
            std::fill(ypr + s * 3, ypr + s * 3 + 3, nan);
            if (argmax) std::fill(argmax + s * 3, argmax + s * 3 + 3, -1);
            if (logits) std::fill(logits + s * N_LOGITS, logits + (s + 1) * N_LOGITS, nan);
        }
    }
    slot->busy = false;
    slot->clip_cap = -1;
    slot->clip_f = 0;
    slot->clip_mixed = false;
}

void Engine::op_head_compact(const int32_t* valid, const int32_t* count, int frames, int slots_per_frame, int max_heads, int32_t* row,
                             int32_t* slot_of_row, int32_t* rows_used, int32_t* overflow) {
    DeviceGuard guard(device_);
    WHENET_REQUIRE(valid && count && row && slot_of_row && rows_used && overflow, WHENET_EINVAL, "op_head_compact: NULL argument");
    WHENET_REQUIRE(frames >= 1 && frames <= 1024 && slots_per_frame >= 1 && slots_per_frame <= 1024 &&
                       frames * slots_per_frame <= HEAD_COMPACT_MAX_SLOTS && max_heads >= 1 && max_heads <= 256,
                   WHENET_EINVAL, "op_head_compact: frames x slots must be 1..1024 and max_heads 1..256");
    const size_t S = size_t(frames) * slots_per_frame;
    TempBufs tmp;
    int32_t* const d_valid = static_cast<int32_t*>(tmp.get(S * sizeof(int32_t)));
    int32_t* const d_count = static_cast<int32_t*>(tmp.get(size_t(frames) * sizeof(int32_t)));
    int32_t* const d_row = static_cast<int32_t*>(tmp.get(S * sizeof(int32_t)));
    int32_t* const d_sor = static_cast<int32_t*>(tmp.get(size_t(max_heads) * sizeof(int32_t)));
    int32_t* const d_two = static_cast<int32_t*>(tmp.get(2 * sizeof(int32_t)));
    WHENET_HIP_CHECK(hipMemcpyAsync(d_valid, valid, S * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
    WHENET_HIP_CHECK(hipMemcpyAsync(d_count, count, size_t(frames) * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
    launch_head_compact(d_valid, d_count, frames, slots_per_frame, max_heads, d_row, d_sor, d_two, d_two + 1, stream_);
    int32_t two[2] = {0, 0};
    WHENET_HIP_CHECK(hipMemcpyAsync(row, d_row, S * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
    WHENET_HIP_CHECK(hipMemcpyAsync(slot_of_row, d_sor, size_t(max_heads) * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
    WHENET_HIP_CHECK(hipMemcpyAsync(two, d_two, sizeof(two), hipMemcpyDeviceToHost, stream_));
    WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
    *rows_used = two[0], *overflow = two[1];
}

void Engine::op_head_plan(int fh, int fw, const float* boxes, int k, int32_t* rects, int32_t* valid, int32_t* plans) {
    DeviceGuard guard(device_);
    WHENET_REQUIRE(boxes != nullptr && rects != nullptr && valid != nullptr && fh > 0 && fw > 0 && k >= 1 && k <= 2048, WHENET_EINVAL,
                   "op_head_plan: NULL argument, an empty frame, or k outside 1..2048");
    const DetRows rows(k);
    const size_t in_bytes = size_t(k) * 4 * sizeof(float), plan_bytes = size_t(k) * CROP_PLAN_INTS * sizeof(int32_t);
    TempBufs tmp;
    float* const d_in = static_cast<float*>(tmp.get(in_bytes));
    int* const d_k = static_cast<int*>(tmp.get(sizeof(int)));
    void* const d_rows = tmp.get(rows.bytes());
    int32_t* const d_plans = plans ? static_cast<int32_t*>(tmp.get(plan_bytes)) : nullptr;
    WHENET_HIP_CHECK(hipMemcpyAsync(d_in, boxes, in_bytes, hipMemcpyHostToDevice, stream_));
    WHENET_HIP_CHECK(hipMemcpyAsync(d_k, &k, sizeof(int), hipMemcpyHostToDevice, stream_));
    HeadPlanArgs a{};
    a.in_boxes = d_in, a.in_scores = nullptr, a.in_count = d_k;
    a.num_classes = 1, a.max_boxes = k, a.frame_h = fh, a.frame_w = fw;
    a.boxes = rows.boxes(d_rows), a.scores = rows.scores(d_rows), a.classes = rows.classes(d_rows), a.count = rows.count(d_rows);
    a.rects = rows.rects(d_rows), a.valid = rows.valid(d_rows), a.plans = d_plans;
    launch_head_plan(a, stream_);
    WHENET_HIP_CHECK(hipMemcpyAsync(rects, a.rects, size_t(k) * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
    WHENET_HIP_CHECK(hipMemcpyAsync(valid, a.valid, size_t(k) * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
    if (plans) WHENET_HIP_CHECK(hipMemcpyAsync(plans, d_plans, plan_bytes, hipMemcpyDeviceToHost, stream_));
    WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
}

// ---- pose overlay (overlay.hip; the contract is in engine.h and include/whenet_hip.h) ----
namespace {
// a surface's planes laid TIGHT behind one another: plane p starts off[p] bytes in, off[planes] bytes in all
int tight_surface(int format, int fh, int fw, int rows[3], int row_bytes[3], size_t off[4]) {
    const int planes = overlay_surface_planes(format, fh, fw, rows, row_bytes);
    off[0] = 0;
    for (int p = 0; p < planes; ++p) off[p + 1] = off[p] + size_t(rows[p]) * size_t(row_bytes[p]);
    return planes;
}
OverlayDrawArgs draw_args(const uint8_t* d_frame, int fh, int fw, int channel_order, const int32_t* d_segs, const int32_t* d_flags, int k,
                          int format, int matrix, const uint32_t* d_labels, int display) {
    OverlayDrawArgs a{};
    a.frame = d_frame, a.fh = fh, a.fw = fw, a.channel_order = channel_order;
    a.segs = d_segs, a.flags = d_flags, a.k = k, a.format = format, a.labels = d_labels, a.display = display;
    if (format != WHENET_SURF_PACKED) WHENET_REQUIRE(bgr2yuv_coeffs(matrix, a.kc), WHENET_EINVAL, "unknown matrix " + std::to_string(matrix));
    return a;
}
void check_display(const char* what, int display) {
    WHENET_REQUIRE(display == WHENET_DISPLAY_SIMPLE || display == WHENET_DISPLAY_FULL, WHENET_EINVAL,
                   std::string(what) + ": unknown display " + std::to_string(display) + " (WHENET_DISPLAY_SIMPLE or WHENET_DISPLAY_FULL)");
}
}  // namespace

void Engine::check_surface(const char* what, const whenet_surface_t& dst, int fh, int fw) const {
    const std::string w = what;
    int rows[3], row_bytes[3];
    const int planes = overlay_surface_planes(dst.format, fh, fw, rows, row_bytes);
    WHENET_REQUIRE(planes > 0, WHENET_EINVAL,
                   w + ": unknown surface format " + std::to_string(dst.format) + " (WHENET_SURF_PACKED, WHENET_YUV_NV12 or WHENET_YUV_I420)");
    WHENET_REQUIRE(dst.format == WHENET_SURF_PACKED || (dst.matrix >= 0 && dst.matrix < WHENET_YUV_MATRICES), WHENET_EINVAL,
                   w + ": unknown matrix " + std::to_string(dst.matrix) + " (WHENET_YUV_BT601, _BT709 or _JFIF)");
    for (int p = 0; p < planes; ++p) {
        const std::string who = w + ": plane " + std::to_string(p);
        WHENET_REQUIRE(dst.plane[p] != nullptr, WHENET_EINVAL, who + " is NULL");
        WHENET_REQUIRE(dst.pitch[p] >= row_bytes[p], WHENET_EINVAL,
                       who + ": pitch " + std::to_string(dst.pitch[p]) + " is below its row of " + std::to_string(row_bytes[p]) + " bytes");
        if (dst.on_device) {
            check_device_plane(who, static_cast<const uint8_t*>(dst.plane[p]), rows[p], dst.pitch[p], row_bytes[p]);
        } else {
            hipPointerAttribute_t attr{};
            const hipError_t e = hipPointerGetAttributes(&attr, dst.plane[p]);
            if (e != hipSuccess) (void)hipGetLastError();      // (ordinary host memory: the runtime does not know it)
            WHENET_REQUIRE(e != hipSuccess || attr.type != hipMemoryTypeDevice, WHENET_EINVAL,
                           who + " is device memory, the surface says on_device = 0");
        }
    }
}

void Engine::op_annotate(const uint8_t* frame, int fh, int fw, int channel_order, const int32_t* rects, const int32_t* valid, const float* ypr,
                         int k, const whenet_surface_t& dst, int display) {
    DeviceGuard guard(device_);
    check_display("op_annotate", display);
    const char* bad = overlay_check(frame, fh, fw, channel_order, rects, valid, ypr, k, &dst);
    WHENET_REQUIRE(bad == nullptr, WHENET_EINVAL, std::string("op_annotate: ") + (bad ? bad : ""));
    WHENET_REQUIRE(dst.on_device == 0, WHENET_EINVAL, "op_annotate: the surface must be host memory (on_device = 0)");
    check_surface("op_annotate", dst, fh, fw);
    int rows[3], row_bytes[3];
    size_t off[4];
    const int planes = tight_surface(dst.format, fh, fw, rows, row_bytes, off);
    const size_t fbytes = size_t(fh) * fw * 3, K = size_t(std::max(k, 1));
    TempBufs tmp;
    uint8_t* const d_frame = static_cast<uint8_t*>(tmp.get(fbytes));
    int32_t* const d_rects = static_cast<int32_t*>(tmp.get(K * 4 * sizeof(int32_t)));
    int32_t* const d_valid = static_cast<int32_t*>(tmp.get(K * sizeof(int32_t)));
    float* const d_ypr = static_cast<float*>(tmp.get(K * 3 * sizeof(float)));
    int32_t* const d_segs = static_cast<int32_t*>(tmp.get(K * (OVERLAY_SEG_INTS + 1) * sizeof(int32_t)));
    int32_t* const d_flags = d_segs + K * OVERLAY_SEG_INTS;
    uint32_t* const d_labels =
        display == WHENET_DISPLAY_FULL ? static_cast<uint32_t*>(tmp.get(K * OVERLAY_LABEL_WORDS * sizeof(uint32_t))) : nullptr;
    std::vector<uint8_t> out(off[planes]);
    WHENET_HIP_CHECK(hipMemcpyAsync(d_frame, frame, fbytes, hipMemcpyHostToDevice, stream_));
    if (k > 0) {
        WHENET_HIP_CHECK(hipMemcpyAsync(d_rects, rects, K * 4 * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
        if (valid) WHENET_HIP_CHECK(hipMemcpyAsync(d_valid, valid, K * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
        WHENET_HIP_CHECK(hipMemcpyAsync(d_ypr, ypr, K * 3 * sizeof(float), hipMemcpyHostToDevice, stream_));
        OverlayPlanArgs p{};
        p.rects = d_rects, p.valid = valid ? d_valid : nullptr, p.row = nullptr, p.ypr = d_ypr;
        p.k = k, p.rect_stride = 4, p.rect_is_size = 0, p.segs = d_segs, p.flags = d_flags, p.labels = d_labels;
        launch_overlay_plan(p, stream_);
    }
    // the landing buffer between two guard zones, as the other kernel-alone calls have it: a byte no lane wrote arrives as the sentinel
    const GuardedOutput d_out(off[planes], stream_);
    OverlayDrawArgs a = draw_args(d_frame, fh, fw, channel_order, d_segs, d_flags, k, dst.format, dst.matrix, d_labels, display);
    for (int p = 0; p < planes; ++p) a.plane[p] = d_out.frames() + off[p], a.pitch[p] = row_bytes[p];
    launch_overlay_draw(a, stream_);
    uint8_t* const one = out.data();
    const size_t span[2] = {0, off[planes]};
    d_out.to_host(stream_, span, 1, &one, "op_annotate");
    for (int p = 0; p < planes; ++p)
        for (int r = 0; r < rows[p]; ++r)
            std::memcpy(static_cast<uint8_t*>(dst.plane[p]) + size_t(r) * size_t(dst.pitch[p]), out.data() + off[p] + size_t(r) * row_bytes[p],
                        size_t(row_bytes[p]));
}

Engine::Slot& Engine::annotate_target(int ticket, int frame_index, int& k, int& fh, int& fw, size_t& frame_off) {
    Slot* found = nullptr;
    for (Slot& s : slots_)
        if (s.busy && s.ticket == ticket) found = &s;
    WHENET_REQUIRE(found != nullptr, WHENET_EINVAL, "frame_annotate: unknown or already collected ticket " + std::to_string(ticket));
    Slot& slot = *found;
    WHENET_REQUIRE(slot.frame_ticket != ticket, WHENET_EINVAL,
                   "frame_annotate: the heads of ticket " + std::to_string(ticket) + " are not enqueued yet (frame_heads, frame_detect_heads "
                   "or clip_detect_heads first)");
    WHENET_REQUIRE(slot.ann_kind != Slot::ANN_NONE, WHENET_EINVAL,
                   "frame_annotate: ticket " + std::to_string(ticket) + " holds no frame with heads (crops only, a released frame, or a "
                   "submit_frame without heads)");
    const int F = slot.ann_kind == Slot::ANN_CLIP ? slot.clip_f : 1;
    WHENET_REQUIRE(frame_index >= 0 && frame_index < F, WHENET_EINVAL,
                   "frame_annotate: frame index " + std::to_string(frame_index) + " outside 0.." + std::to_string(F - 1));
    WHENET_REQUIRE((slot.ann_mask & (1u << frame_index)) == 0, WHENET_EINVAL,
                   "frame_annotate: frame " + std::to_string(frame_index) + " of ticket " + std::to_string(ticket) + " is annotated already");
    k = slot.ann_kind == Slot::ANN_PLANS ? slot.n : (slot.ann_kind == Slot::ANN_DET ? slot.det_cap : slot.clip_cap);
    WHENET_REQUIRE(k <= OVERLAY_MAX_HEADS, WHENET_EINVAL,
                   "frame_annotate: " + std::to_string(k) + " head slots per frame, the overlay takes at most " + std::to_string(OVERLAY_MAX_HEADS));
    const bool mixed = slot.ann_kind == Slot::ANN_CLIP && slot.clip_mixed;
    fh = mixed ? slot.clip_fh[frame_index] : slot.fh, fw = mixed ? slot.clip_fw[frame_index] : slot.fw;
    frame_off = mixed ? slot.clip_off[frame_index] : size_t(frame_index) * size_t(fh) * fw * 3;
    return slot;
}

void Engine::frame_annotate(int ticket, int frame_index, const whenet_surface_t& dst, hipStream_t stream, int display) {
    DeviceGuard guard(device_);
    check_display("frame_annotate", display);
    int k, fh, fw;
    size_t frame_off;
    Slot& slot = annotate_target(ticket, frame_index, k, fh, fw, frame_off);
    const int F = slot.ann_kind == Slot::ANN_CLIP ? slot.clip_f : 1;
    check_surface("frame_annotate", dst, fh, fw);
    int rows[3], row_bytes[3];
    size_t off[4];
    const int planes = tight_surface(dst.format, fh, fw, rows, row_bytes, off);
    const int channel_order = slot.swap_rb ? WHENET_BGR : WHENET_RGB;
    // allocations and the events first: nothing is enqueued yet if one of them fails
    const size_t S = size_t(F) * size_t(std::max(k, 1));
    slot.ann_table.grow(S * (OVERLAY_SEG_INTS + 1) * sizeof(int32_t));
    const bool full = display == WHENET_DISPLAY_FULL;
    if (full) slot.ann_labels.grow(S * OVERLAY_LABEL_WORDS * sizeof(uint32_t));
    StagedBuffer& stage = slot.ann_stage[frame_index];
    if (!dst.on_device) stage.h.grow(off[planes]), stage.d.grow(off[planes]);
    if (!slot.ann_done) slot.ann_done.create();
    if (dst.on_device && stream != nullptr && !slot.source) slot.source.create();
    int32_t* const d_segs = slot.ann_table.as<int32_t>() + size_t(frame_index) * size_t(k) * OVERLAY_SEG_INTS;
    int32_t* const d_flags = slot.ann_table.as<int32_t>() + S * OVERLAY_SEG_INTS + size_t(frame_index) * size_t(k);
    uint32_t* const d_labels = full ? slot.ann_labels.as<uint32_t>() + size_t(frame_index) * size_t(k) * OVERLAY_LABEL_WORDS : nullptr;
    OverlayDrawArgs a =
        draw_args(slot.frame.d.as<uint8_t>() + frame_off, fh, fw, channel_order, d_segs, d_flags, k, dst.format, dst.matrix, d_labels, display);
    for (int p = 0; p < planes; ++p) {
        a.plane[p] = dst.on_device ? static_cast<uint8_t*>(dst.plane[p]) : stage.d.as<uint8_t>() + off[p];
        a.pitch[p] = dst.on_device ? dst.pitch[p] : row_bytes[p];
    }
    // The frame was written on the copy stream (H2D, pack or conversion kernel) behind slot.copied.  The calls that enqueue heads
    // make stream_ wait for that event -- but frame_heads with k = 0 enqueues nothing and waits for nothing, and its frame is
    // annotated all the same: the wait is made here for every form (an event already waited for costs nothing).
    WHENET_HIP_CHECK(hipStreamWaitEvent(stream_, slot.copied, 0));
    if (k > 0) {
        OverlayPlanArgs p{};
        p.ypr = slot.dev().ypr, p.k = k, p.segs = d_segs, p.flags = d_flags, p.labels = d_labels;
        if (slot.ann_kind == Slot::ANN_PLANS) {
            p.rects = slot.plan.d.as<int32_t>(), p.rect_stride = CROP_PLAN_INTS, p.rect_is_size = 1;
        } else if (slot.ann_kind == Slot::ANN_DET) {
            const DetRows r(slot.det_cap);
            p.rects = r.rects(slot.det.d.as<void>()), p.valid = r.valid(slot.det.d.as<void>()), p.rect_stride = 4;
        } else {
            const ClipRows r(slot.clip_f, slot.clip_cap, slot.clip_heads);
            const size_t first = size_t(frame_index) * size_t(k);
            p.rects = r.rects(slot.det.d.as<void>()) + first * 4, p.valid = r.valid(slot.det.d.as<void>()) + first;
            p.row = r.row(slot.det.d.as<void>()) + first, p.rect_stride = 4;
        }
        launch_overlay_plan(p, stream_);
    }
    if (dst.on_device && stream != nullptr) {      // the surface's previous reader on the caller's stream goes first
        WHENET_HIP_CHECK(hipEventRecord(slot.source, stream));
        WHENET_HIP_CHECK(hipStreamWaitEvent(stream_, slot.source, 0));
    }
    launch_overlay_draw(a, stream_);
    if (dst.on_device) {
        if (stream != nullptr) {
            WHENET_HIP_CHECK(hipEventRecord(slot.ann_done, stream_));
            WHENET_HIP_CHECK(hipStreamWaitEvent(stream, slot.ann_done, 0));
        }
    } else {
        WHENET_HIP_CHECK(hipMemcpyAsync(stage.h.as<void>(), stage.d.as<void>(), off[planes], hipMemcpyDeviceToHost, stream_));
        slot.ann_host.push_back({dst, frame_index, fh, fw});
    }
    WHENET_HIP_CHECK(hipEventRecord(slot.done, stream_));      // the collect call waits for the overlay as well
    slot.ann_mask |= 1u << frame_index;
}

void Engine::finish_annotations(Slot& slot) {
    for (const Slot::AnnHost& h : slot.ann_host) {
        int rows[3], row_bytes[3];
        size_t off[4];
        const int planes = tight_surface(h.dst.format, h.fh, h.fw, rows, row_bytes, off);
        const uint8_t* src = slot.ann_stage[h.frame_index].h.as<uint8_t>();
        for (int p = 0; p < planes; ++p)
            for (int r = 0; r < rows[p]; ++r)
                std::memcpy(static_cast<uint8_t*>(h.dst.plane[p]) + size_t(r) * size_t(h.dst.pitch[p]), src + off[p] + size_t(r) * row_bytes[p],
                            size_t(row_bytes[p]));
    }
    slot.ann_host.clear();
    for (const Slot::JpegHost& j : slot.jpg_host) {      // the streams of frame_annotate_jpeg: pinned landing buffer -> the caller
        const size_t cap16 = (size_t(j.staged_cap) + 15) & ~size_t(15);
        const uint8_t* src = slot.jpg_stage[j.frame_index].host.as<uint8_t>();
        long long total = 0;
        std::memcpy(&total, src + cap16, sizeof(total));
        if (std::min<long long>(total, j.staged_cap) > 0) std::memcpy(j.out, src, size_t(std::min<long long>(total, j.staged_cap)));
        *j.size = total;
        *j.status = total <= j.cap ? WHENET_OK : WHENET_EOVERFLOW;
    }
    slot.jpg_host.clear();
    if (slot.jpg_dec_out != nullptr) {      // frame_begin_jpeg: the status words, written to pinned memory by the decode on the copy stream
        WHENET_HIP_CHECK(hipEventSynchronize(slot.copied));      // (a ticket collected without heads has waited for nothing yet)
        std::memcpy(slot.jpg_dec_out, slot.jpg_dec_status.as<void>(), size_t(slot.jpg_dec_pairs) * 2 * sizeof(int32_t));
        slot.jpg_dec_out = nullptr;
    }
}

// ---- JPEG encoder (jpeg.hip; the contract is in engine.h and include/whenet_hip.h) ----
void Engine::op_jpeg_encode(const whenet_surface_t& src, int h, int w, int channel_order, int quality, uint8_t* out, int64_t cap, int64_t* size,
                            int sampling, bool optimize, uint32_t (*hist)[256]) {
    DeviceGuard guard(device_);
    const char* bad = jpeg_check(&src, h, w, channel_order, quality, out, cap, size, sampling);
    WHENET_REQUIRE(bad == nullptr, WHENET_EINVAL, std::string("op_jpeg_encode: ") + (bad ? bad : ""));
    WHENET_REQUIRE(src.on_device == 0, WHENET_EINVAL, "op_jpeg_encode: the surface must be host memory (on_device = 0)");
    check_surface("op_jpeg_encode", src, h, w);
    int rows[3], row_bytes[3];
    size_t off[4];
    const int planes = tight_surface(src.format, h, w, rows, row_bytes, off);
    JpegTables tables;
    jpeg_build_tables(h, w, quality, tables, sampling);
    const JpegScratch lay(h, w, sampling);
    TempBufs tmp;
    uint8_t* const d_planes = static_cast<uint8_t*>(tmp.get(off[planes]));
    JpegTables* const d_tables = static_cast<JpegTables*>(tmp.get(sizeof(JpegTables)));
    void* const d_scratch = tmp.get(lay.bytes);
    long long* const d_size = static_cast<long long*>(tmp.get(sizeof(long long)));
    JpegSource s = jpeg_source(src, h, w, channel_order);
    for (int p = 0; p < planes; ++p) {
        WHENET_HIP_CHECK(hipMemcpy2DAsync(d_planes + off[p], size_t(row_bytes[p]), src.plane[p], size_t(src.pitch[p]), size_t(row_bytes[p]),
                                          size_t(rows[p]), hipMemcpyHostToDevice, stream_));
        s.plane[p] = d_planes + off[p], s.pitch[p] = row_bytes[p];
    }
    WHENET_HIP_CHECK(hipMemcpyAsync(d_tables, &tables, sizeof(tables), hipMemcpyHostToDevice, stream_));
    WHENET_HIP_CHECK(hipMemsetAsync(d_size, 0, sizeof(long long), stream_));
    // no stream is longer than the bound: a landing buffer of min(cap, bound) bytes answers as one of cap bytes would
    const int64_t dcap = std::min<int64_t>(cap, jpeg_bound(h, w, sampling));
    const GuardedOutput d_out(size_t(dcap), stream_);
    const JpegArgs a = jpeg_args(s, d_tables, d_scratch, lay, d_out.frames(), dcap, d_size, optimize);
    launch_jpeg_encode(a, lay, stream_);
    WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
    long long total = 0;
    WHENET_HIP_CHECK(hipMemcpy(&total, d_size, sizeof(total), hipMemcpyDeviceToHost));
    if (optimize && hist != nullptr) WHENET_HIP_CHECK(hipMemcpy(hist, a.opt->hist, sizeof(a.opt->hist), hipMemcpyDeviceToHost));
    // (an optimised header lists the occurring symbols only: SOI .. SOF0, four DHT of at least one symbol, DRI, SOS)
    WHENET_REQUIRE(total >= (optimize ? 177 + 4 * 22 + 20 : JPEG_HEADER_BYTES) + 2 && total <= jpeg_bound(h, w, sampling), WHENET_EHIP,
                   "op_jpeg_encode: the kernels report a stream of " + std::to_string(total) + " bytes");
    const size_t span[2] = {0, size_t(std::min<int64_t>(total, dcap))};
    d_out.to_host(stream_, span, 1, &out, "op_jpeg_encode");
    *size = total;
    WHENET_REQUIRE(total <= cap, WHENET_EOVERFLOW,
                   "op_jpeg_encode: the stream has " + std::to_string(total) + " bytes, the capacity is " + std::to_string(cap));
}

const JpegTables* Engine::jpeg_device_tables(int h, int w, int quality, int sampling) {
    for (const JpegTableSet& t : jpeg_tables_)
        if (t.h == h && t.w == w && t.quality == quality && t.sampling == sampling) return t.d.as<JpegTables>();
    if (jpeg_tables_.size() >= 8) {      // an earlier call's kernels may still read a set
        WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
        jpeg_tables_.clear();
    }
    JpegTables tables;
    jpeg_build_tables(h, w, quality, tables, sampling);
    JpegTableSet set{h, w, quality, sampling, DeviceBuffer()};
    set.d.reset(sizeof(JpegTables));
    WHENET_HIP_CHECK(hipMemcpy(set.d.as<void>(), &tables, sizeof(tables), hipMemcpyHostToDevice));
    jpeg_tables_.push_back(std::move(set));
    return jpeg_tables_.back().d.as<JpegTables>();
}

void Engine::jpeg_encode_device(const whenet_surface_t& src, int h, int w, int channel_order, int quality, void* dst, int64_t cap, int64_t* dsize,
                                hipStream_t stream, int sampling, bool optimize) {
    DeviceGuard guard(device_);
    const char* bad = jpeg_check(&src, h, w, channel_order, quality, dst, cap, dsize, sampling);
    WHENET_REQUIRE(bad == nullptr, WHENET_EINVAL, std::string("jpeg_encode_device: ") + (bad ? bad : ""));
    WHENET_REQUIRE(src.on_device == 1, WHENET_EINVAL, "jpeg_encode_device: the surface must be device memory (on_device = 1)");
    WHENET_REQUIRE(cap <= std::numeric_limits<int>::max(), WHENET_EINVAL, "jpeg_encode_device: a capacity above 2^31 - 1 bytes");
    check_surface("jpeg_encode_device", src, h, w);
    if (cap > 0) check_device_plane("jpeg_encode_device: dst", static_cast<const uint8_t*>(dst), 1, int(cap), int(cap));
    check_device_plane("jpeg_encode_device: dsize", reinterpret_cast<const uint8_t*>(dsize), 1, 8, 8);
    WHENET_REQUIRE(reinterpret_cast<uintptr_t>(dsize) % 8 == 0, WHENET_EINVAL, "jpeg_encode_device: dsize is not aligned to 8 bytes");
    // allocations, the tables and the events first: nothing is enqueued yet if one of them fails
    const JpegScratch lay(h, w, sampling);
    if (lay.bytes > jpeg_scratch_.bytes()) {      // (the buffer in hand may still be read by an earlier call's kernels)
        WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
        jpeg_scratch_.reset(lay.bytes);
    }
    const JpegTables* d_tables = jpeg_device_tables(h, w, quality, sampling);
    if (!jpeg_source_) jpeg_source_.create();
    if (!jpeg_done_) jpeg_done_.create();
    const JpegArgs a = jpeg_args(jpeg_source(src, h, w, channel_order), d_tables, jpeg_scratch_.as<void>(), lay, dst, cap, dsize, optimize);
    WHENET_HIP_CHECK(hipEventRecord(jpeg_source_, stream));
    WHENET_HIP_CHECK(hipStreamWaitEvent(stream_, jpeg_source_, 0));
    launch_jpeg_encode(a, lay, stream_);
    WHENET_HIP_CHECK(hipEventRecord(jpeg_done_, stream_));
    WHENET_HIP_CHECK(hipStreamWaitEvent(stream, jpeg_done_, 0));
}

void Engine::frame_annotate_jpeg(int ticket, int frame_index, int display, int quality, uint8_t* out, int64_t cap, int64_t* size,
                                 int32_t* status, int sampling, bool optimize) {
    DeviceGuard guard(device_);
    check_display("frame_annotate_jpeg", display);
    WHENET_REQUIRE(jpeg_sampling_ok(sampling), WHENET_EINVAL,
                   "frame_annotate_jpeg: unknown sampling (WHENET_JPEG_420, WHENET_JPEG_422 or WHENET_JPEG_444)");
    WHENET_REQUIRE(size != nullptr && status != nullptr && (out != nullptr || cap == 0), WHENET_EINVAL, "frame_annotate_jpeg: NULL argument");
    WHENET_REQUIRE(cap >= 0, WHENET_EINVAL, "frame_annotate_jpeg: negative capacity");
    WHENET_REQUIRE(quality >= 1 && quality <= 100, WHENET_EINVAL, "frame_annotate_jpeg: quality must be 1..100");
    int k, fh, fw;
    size_t frame_off;
    Slot& slot = annotate_target(ticket, frame_index, k, fh, fw, frame_off);
    // allocations and the tables first: nothing is enqueued yet if one of them fails
    int rows[3], row_bytes[3];
    size_t off[4];
    // 4:2:0: a tight I420 JFIF surface; 4:2:2 / 4:4:4: tight packed pixels in the frame's channel order (full-resolution chroma)
    const int format = sampling == WHENET_JPEG_420 ? WHENET_YUV_I420 : WHENET_SURF_PACKED;
    const int planes = tight_surface(format, fh, fw, rows, row_bytes, off);
    const long long staged_cap = std::min<long long>(cap, jpeg_bound(fh, fw, sampling));      // no stream is longer than the bound
    const size_t cap16 = (size_t(staged_cap) + 15) & ~size_t(15);
    Slot::JpegStage& stage = slot.jpg_stage[frame_index];
    stage.surface.grow(off[planes]);
    stage.stream.grow(cap16 + 16);
    stage.host.grow(cap16 + 16);
    const JpegScratch lay(fh, fw, sampling);
    if (lay.bytes > jpeg_scratch_.bytes()) {      // (the buffer in hand may still be read by an earlier call's kernels)
        WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
        jpeg_scratch_.reset(lay.bytes);
    }
    const JpegTables* d_tables = jpeg_device_tables(fh, fw, quality, sampling);
    void* h_dev = nullptr;                         // the pinned buffer as the device addresses it
    WHENET_HIP_CHECK(hipHostGetDevicePointer(&h_dev, stage.host.as<void>(), 0));
    whenet_surface_t surf{};
    for (int p = 0; p < planes; ++p) surf.plane[p] = stage.surface.as<uint8_t>() + off[p], surf.pitch[p] = row_bytes[p];
    surf.format = format, surf.matrix = format == WHENET_YUV_I420 ? WHENET_YUV_JFIF : 0, surf.on_device = 1;
    const int channel_order = slot.swap_rb ? WHENET_BGR : WHENET_RGB;      // (read for the packed surface only: frame_annotate wrote it so)
    // the overlay into the engine's surface (it counts as the frame's one annotate call), the encoder behind it on the same stream,
    // then min(size, cap) bytes and the size into the pinned buffer: the only bytes that cross the link
    frame_annotate(ticket, frame_index, surf, nullptr, display);
    uint8_t* const d_stream = stage.stream.as<uint8_t>();
    long long* const d_size = reinterpret_cast<long long*>(d_stream + cap16);
    launch_jpeg_encode(
        jpeg_args(jpeg_source(surf, fh, fw, channel_order), d_tables, jpeg_scratch_.as<void>(), lay, d_stream, staged_cap, d_size, optimize), lay,
        stream_);
    launch_jpeg_flush(d_stream, h_dev, d_size, staged_cap, reinterpret_cast<long long*>(static_cast<uint8_t*>(h_dev) + cap16), stream_);
    WHENET_HIP_CHECK(hipEventRecord(slot.done, stream_));      // the collect call waits for the stream's bytes as well
    slot.jpg_host.push_back({out, cap, staged_cap, size, status, frame_index});
}

// ---- JPEG decoder (jpeg_dec.hip; the contract is in engine.h and include/whenet_hip.h) ----
namespace {
// a slot's pinned status words: a pair per frame of the largest clip
constexpr size_t JPEG_STATUS_BYTES = size_t(MIXED_MAX_FRAMES) * 2 * sizeof(int32_t);
}  // namespace

JpegDecScratch Engine::jpeg_dec_layout(const JpegDecGeom& g, size_t data_bytes, int64_t nbytes, int entropy, int seg_bytes) const {
    const int form = jpeg_dec_form(entropy >= 0 ? entropy : jpeg_entropy_, nbytes, g.intervals);
    JpegDecScratch lay(g, data_bytes, nbytes, form, seg_bytes > 0 ? seg_bytes : jpeg_seg_bytes_);
    lay.seg_lanes = jpeg_seg_lanes_;
    return lay;
}

int Engine::jpeg_rule_of(const char* what, int rule) const {
    WHENET_REQUIRE(rule == -1 || jpeg_rule_ok(rule), WHENET_EINVAL,
                   std::string(what) + ": rule must be -1 (the handle's option), 0 (the project's own) or 1 (libjpeg)");
    return rule == -1 ? jpeg_rule_ : rule;
}

int Engine::jpeg_orient_of(const char* what, int orient, const uint8_t* data, int64_t size) const {
    WHENET_REQUIRE(orient >= -1 && orient <= 1, WHENET_EINVAL,
                   std::string(what) + ": orient must be -1 (the handle's option), 0 (the orientation is ignored) or 1 (it is applied)");
    return (orient == -1 ? jpeg_orient_ != 0 : orient != 0) ? jpeg_exif_orientation(data, size) : 1;
}

// an oriented decode (2..8) into an I420 / NV12 destination
static void jpeg_orient_require_packed(const std::string& what, int orient, const whenet_surface_t& dst) {
    WHENET_REQUIRE(orient <= 1 || (dst.format != WHENET_YUV_I420 && dst.format != WHENET_YUV_NV12), WHENET_EINVAL,
                   what + ": the stream's orientation is " + std::to_string(orient) +
                       ": an oriented decode writes packed surfaces only (WHENET_SURF_PACKED)");
}

// the accept bits of a single-stream call: the argument, or (-1) the handle's options "jpeg_progressive" and "jpeg_layouts"
int Engine::jpeg_accept_of(const char* what, int accept) const {
    WHENET_REQUIRE(accept == -1 || jpeg_accept_ok(accept), WHENET_EINVAL,
                   std::string(what) + ": the accept bits must be -1 (the handle's options) or 0..3 (1: progressive streams, 2: layouts)");
    return accept == -1 ? (jpeg_progressive_ != 0 ? JPEG_ACCEPT_PROGRESSIVE : 0) | (jpeg_layouts_ != 0 ? JPEG_ACCEPT_LAYOUTS : 0) : accept;
}

void Engine::add_jpeg_decode_counters(int64_t out[4]) const { out[0] += jpeg_dec_launched_[0], out[1] += jpeg_dec_launched_[1]; }
void Engine::add_jpeg_progressive_counters(int64_t out[4]) const {
    for (int i = 0; i < 3; ++i) out[i] += jpeg_prog_counts_[i];
}

// One parsed stream for the single-stream kernels (op_jpeg_decode, frame_begin_jpeg): the work buffer of its decoder -- the baseline
// one's (tables | compressed bytes | ...) or, for a progressive stream, the scan plan's; either way the front of the buffer is what
// ONE H2D uploads
struct Engine::JpegStreamJob {
    const whenet_jpeg_info_t& info;
    const JpegProgPlan& plan;      // (empty where the stream was parsed without one)
    const bool prog;
    const JpegDecGeom g;
    const size_t nbytes;           // the bytes behind data_offset
    const JpegDecScratch lay;
    const JpegProgLayout play;
    JpegStreamJob(const Engine& e, const whenet_jpeg_info_t& in, const JpegProgPlan& p, bool accept, int64_t size, int entropy, int seg_bytes)
        : info(in), plan(p), prog(accept && !p.baseline), g(jpeg_dec_geom(in)), nbytes(size_t(size - in.data_offset)),
          lay(e.jpeg_dec_layout(g, prog ? 0 : nbytes, prog ? 0 : int64_t(nbytes), prog ? 0 : entropy, seg_bytes)), play(g, p) {}
    size_t upload_bytes() const { return prog ? play.upload_bytes : lay.upload_bytes; }
    size_t work_bytes() const { return prog ? play.bytes : lay.bytes; }
};

// The stream's upload block laid out at `stage` (host memory of job.upload_bytes()), its one H2D into d_work and its launches on
// `stream`: memset, a scan-kernel launch per level and the finish, then the stages the baseline decoder ends with; or the baseline
// decoder.  Returns the scan-kernel launches.
int64_t Engine::jpeg_stream_launch(const JpegStreamJob& job, const uint8_t* data, uint8_t* stage, void* d_work, const whenet_surface_t& dst,
                                   int channel_order, int32_t* d_status, int rule, hipStream_t stream, int orient) {
    if (job.prog) {
        jpeg_prog_stage(job.plan, job.play, data + job.plan.data_base, stage);
    } else {      // tables | compressed bytes
        std::vector<JpegDecTables> tables(1);
        jpeg_dec_build_tables(job.info, tables[0]);
        std::memset(stage, 0, job.lay.data);
        std::memcpy(stage + job.lay.tables, tables.data(), sizeof(JpegDecTables));
        if (job.nbytes > 0) std::memcpy(stage + job.lay.data, data + job.info.data_offset, job.nbytes);
    }
    WHENET_HIP_CHECK(hipMemcpyAsync(d_work, stage, job.upload_bytes(), hipMemcpyHostToDevice, stream));
    int64_t launches = 0;
    if (job.prog) {
        launch_jpeg_decode_progressive(
            jpeg_dec_args(job.g, d_work, job.play.regions(), job.plan.data_bytes, dst, channel_order, d_status, rule, 0, orient), job.plan, job.play,
            d_work,
            jpeg_prog_levels_, stream, &launches);
        ++jpeg_prog_counts_[0], jpeg_prog_counts_[1] += launches, jpeg_prog_counts_[2] += int64_t(job.plan.dev.size());
    } else {
        launch_jpeg_decode(
            jpeg_dec_args(job.g, d_work, job.lay.regions(), (long long)(job.nbytes), dst, channel_order, d_status, rule, job.lay.seg_lanes, orient),
            job.lay, stream);
        ++jpeg_dec_launched_[job.lay.form];
    }
    return launches;
}

void Engine::op_jpeg_decode(const uint8_t* data, int64_t size, const whenet_surface_t& dst, int channel_order, int32_t* status, int entropy,
                            int seg_bytes, int64_t* stats, int rule, int progressive, int orient, int* applied) {
    DeviceGuard guard(device_);
    WHENET_REQUIRE(status != nullptr, WHENET_EINVAL, "op_jpeg_decode: NULL argument");
    rule = jpeg_rule_of("op_jpeg_decode", rule);
    whenet_jpeg_info_t info;
    JpegProgPlan plan;
    const int bits = jpeg_accept_of("op_jpeg_decode", progressive);
    const bool accept = bits != 0;      // (the stream has a scan plan: `plan.baseline` where the baseline decoder takes it)
    jpeg_parse_accept_or_refuse("op_jpeg_decode", data, size, info, plan, bits);
    const int o = jpeg_orient_of("op_jpeg_decode", orient, data, size);
    jpeg_orient_require_packed("op_jpeg_decode", o, dst);
    const whenet_jpeg_info_t landed = jpeg_orient_info(info, o);      // (the destination is the oriented frame)
    const char* bad = jpeg_dec_check_dst(landed, &dst, channel_order, rule);
    WHENET_REQUIRE(bad == nullptr, WHENET_EINVAL, std::string("op_jpeg_decode: ") + (bad ? bad : ""));
    WHENET_REQUIRE(dst.on_device == 0, WHENET_EINVAL, "op_jpeg_decode: the surface must be host memory (on_device = 0)");
    check_surface("op_jpeg_decode", dst, landed.h, landed.w);
    const JpegStreamJob job(*this, info, plan, accept, size, entropy, seg_bytes);
    GuardedSurfaces out;
    out.add(dst, landed.h, landed.w);
    TempBufs tmp;
    char* const d_scratch = static_cast<char*>(tmp.get(job.work_bytes()));
    int32_t* const d_status = static_cast<int32_t*>(tmp.get(2 * sizeof(int32_t)));
    std::vector<uint8_t> upload(job.upload_bytes());      // (alive until the wait below)
    out.alloc(stream_);
    const int64_t prog_launches = jpeg_stream_launch(job, data, upload.data(), d_scratch, out.device()[0], channel_order, d_status, rule, stream_, o);
    if (applied != nullptr) *applied = o;
    out.to_host(stream_, "op_jpeg_decode", "the surface");      // waits
    WHENET_HIP_CHECK(hipMemcpy(status, d_status, 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (stats != nullptr && job.prog) {
        std::fill(stats, stats + 8, int64_t(0));
        stats[0] = plan.total_items, stats[1] = plan.levels, stats[2] = int64_t(plan.dev.size()), stats[3] = prog_launches;
    } else if (stats != nullptr) {
        if (job.lay.form == 1) {
            WHENET_HIP_CHECK(hipMemcpy(stats, d_scratch + job.lay.seg_stats, 8 * sizeof(int64_t), hipMemcpyDeviceToHost));
        } else {      // an interval per lane: the intervals it decoded are those up to the first one the markers make bad
            int32_t meta0 = 0;
            WHENET_HIP_CHECK(hipMemcpy(&meta0, d_scratch + job.lay.meta, sizeof(int32_t), hipMemcpyDeviceToHost));
            std::fill(stats, stats + 8, int64_t(0));
            stats[0] = std::min(meta0, job.g.intervals - 1) + 1;
        }
    }
}

void Engine::jpeg_decode_device(const whenet_jpeg_info_t& info, const uint8_t* d_entropy, int64_t nbytes, const whenet_surface_t& dst,
                                int channel_order, int32_t* d_status, hipStream_t stream) {
    DeviceGuard guard(device_);
    WHENET_REQUIRE(d_entropy != nullptr && d_status != nullptr, WHENET_EINVAL, "jpeg_decode_device: NULL argument");
    WHENET_REQUIRE(nbytes >= 1 && nbytes <= JPEG_DEC_MAX_BYTES, WHENET_EINVAL, "jpeg_decode_device: nbytes must be 1..2^31 - 1");
    const char* bad = jpeg_dec_check_info(info, jpeg_layouts_ != 0);      // (no argument here: the handle's option "jpeg_layouts")
    WHENET_REQUIRE(bad == nullptr, WHENET_EINVAL, std::string("jpeg_decode_device: info: ") + (bad ? bad : ""));
    bad = jpeg_dec_check_dst(info, &dst, channel_order, jpeg_rule_);
    WHENET_REQUIRE(bad == nullptr, WHENET_EINVAL, std::string("jpeg_decode_device: ") + (bad ? bad : ""));
    WHENET_REQUIRE(dst.on_device == 1, WHENET_EINVAL, "jpeg_decode_device: the surface must be device memory (on_device = 1)");
    check_surface("jpeg_decode_device", dst, info.h, info.w);
    check_device_plane("jpeg_decode_device: d_entropy", d_entropy, 1, int(nbytes), int(nbytes));
    check_device_plane("jpeg_decode_device: d_status", reinterpret_cast<const uint8_t*>(d_status), 1, 8, 8);
    WHENET_REQUIRE(reinterpret_cast<uintptr_t>(d_status) % 4 == 0, WHENET_EINVAL, "jpeg_decode_device: d_status is not aligned to 4 bytes");
    // allocations, the tables and the events first: nothing is enqueued yet if one of them fails
    const JpegDecGeom g = jpeg_dec_geom(info);
    const JpegDecScratch lay = jpeg_dec_layout(g, 0, nbytes);
    if (lay.bytes > jpeg_dec_scratch_.bytes()) {      // (the buffer in hand may still be read by an earlier call's kernels)
        WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
        jpeg_dec_scratch_.reset(lay.bytes);
    }
    std::vector<JpegDecTables> tables(1);
    jpeg_dec_build_tables(info, tables[0]);
    if (jpeg_dec_tables_d_.bytes() == 0 || std::memcmp(&jpeg_dec_tables_h_[0], tables.data(), sizeof(JpegDecTables)) != 0) {
        // other tables than the last call's (an MJPG stream repeats its own): the set in hand may still be read
        WHENET_HIP_CHECK(hipStreamSynchronize(stream_));
        jpeg_dec_tables_d_.grow(sizeof(JpegDecTables));
        WHENET_HIP_CHECK(hipMemcpy(jpeg_dec_tables_d_.as<void>(), tables.data(), sizeof(JpegDecTables), hipMemcpyHostToDevice));
        jpeg_dec_tables_h_ = tables;
    }
    if (!jpeg_source_) jpeg_source_.create();
    if (!jpeg_done_) jpeg_done_.create();
    JpegDecArgs a = jpeg_dec_args(g, jpeg_dec_scratch_.as<void>(), lay.regions(), nbytes, dst, channel_order, d_status, jpeg_rule_, lay.seg_lanes);
    a.tables = jpeg_dec_tables_d_.as<JpegDecTables>(), a.data = d_entropy;      // (neither lies in the work buffer)
    WHENET_HIP_CHECK(hipEventRecord(jpeg_source_, stream));
    WHENET_HIP_CHECK(hipStreamWaitEvent(stream_, jpeg_source_, 0));
    launch_jpeg_decode(a, lay, stream_);
    ++jpeg_dec_launched_[lay.form];
    WHENET_HIP_CHECK(hipEventRecord(jpeg_done_, stream_));
    WHENET_HIP_CHECK(hipStreamWaitEvent(stream, jpeg_done_, 0));
}

// A free slot for the decoded frames of frame_begin_jpeg / clip_begin_jpeg: the pinned staging for an upload of upload_bytes, the
// frame buffer (frame f at off[f], tight), the decoder's work buffer and the status words.  dst[f]: frame f as the packed surface
// the kernels write; d_status: the pinned status words as the device addresses them.
Engine::Slot& Engine::jpeg_slot_begin(const whenet_jpeg_info_t* info, int nframes, size_t upload_bytes, size_t work_bytes, size_t* off,
                                      whenet_surface_t* dst, int32_t*& d_status) {
    Slot& slot = *free_slot();
    ensure_slot(slot, 1);
    off[0] = 0;
    for (int f = 0; f < nframes; ++f) off[f + 1] = off[f] + size_t(info[f].h) * info[f].w * 3;
    slot.frame.h.grow(std::max(off[nframes], upload_bytes));      // (>= the frames' bytes: the size every other user of the staging grows it to)
    slot.frame.d.grow(off[nframes]);
    slot.jpg_dec.grow(work_bytes);
    slot.jpg_dec_status.grow(JPEG_STATUS_BYTES);
    void* p = nullptr;
    WHENET_HIP_CHECK(hipHostGetDevicePointer(&p, slot.jpg_dec_status.as<void>(), 0));
    d_status = static_cast<int32_t*>(p);
    for (int f = 0; f < nframes; ++f) {
        dst[f] = whenet_surface_t{};
        dst[f].plane[0] = slot.frame.d.as<uint8_t>() + off[f], dst[f].pitch[0] = 3 * info[f].w, dst[f].format = WHENET_SURF_PACKED, dst[f].on_device = 1;
    }
    return slot;
}

// ... and its end, behind the launches on the copy stream: the slot as frame_begin (clip_frames = 0), clip_begin (frames of one size)
// or clip_begin_mixed (frames back to back at off) leaves it for the decoded frames; the ticket
int Engine::jpeg_slot_finish(Slot& slot, const whenet_jpeg_info_t* info, const size_t* off, int clip_frames, bool one_size, int channel_order,
                             int32_t* status) {
    WHENET_HIP_CHECK(hipEventRecord(slot.copied, copy_stream()));
    slot.fh = info[0].h, slot.fw = info[0].w, slot.swap_rb = channel_order == WHENET_BGR;
    if (!one_size) {
        for (int f = 0; f < clip_frames; ++f) slot.clip_fh[f] = info[f].h, slot.clip_fw[f] = info[f].w;
        std::copy(off, off + clip_frames + 1, slot.clip_off);
    }
    slot.frame_ticket = finish_submission(slot, 0);
    slot.clip_f = clip_frames;
    slot.clip_mixed = !one_size;
    slot.jpg_dec_out = status, slot.jpg_dec_pairs = std::max(clip_frames, 1);
    return slot.frame_ticket;
}

// frame_begin from a JPEG stream: the slot ends up exactly as frame_begin(decoded frame, channel_order) leaves it
int Engine::frame_begin_jpeg(const uint8_t* data, int64_t size, int channel_order, int32_t* status, int rule, int progressive, int orient,
                             int* applied) {
    DeviceGuard guard(device_);
    WHENET_REQUIRE(status != nullptr, WHENET_EINVAL, "frame_begin_jpeg: NULL argument");
    rule = jpeg_rule_of("frame_begin_jpeg", rule);
    WHENET_REQUIRE(channel_order == WHENET_RGB || channel_order == WHENET_BGR, WHENET_EINVAL, "frame_begin_jpeg: unknown channel order");
    whenet_jpeg_info_t info;
    JpegProgPlan plan;
    const int bits = jpeg_accept_of("frame_begin_jpeg", progressive);
    const bool accept = bits != 0;
    jpeg_parse_accept_or_refuse("frame_begin_jpeg", data, size, info, plan, bits);      // (before a slot is taken)
    const int o = jpeg_orient_of("frame_begin_jpeg", orient, data, size);
    const whenet_jpeg_info_t landed = jpeg_orient_info(info, o);      // (the slot's frame is the oriented one: the same byte count)
    const JpegStreamJob job(*this, info, plan, accept, size, -1, 0);
    size_t off[2];
    whenet_surface_t dst;
    int32_t* d_status = nullptr;
    Slot& slot = jpeg_slot_begin(&landed, 1, job.upload_bytes(), job.work_bytes(), off, &dst, d_status);
    jpeg_stream_launch(job, data, slot.frame.h.as<uint8_t>(), slot.jpg_dec.as<void>(), dst, channel_order, d_status, rule, copy_stream(), o);
    if (applied != nullptr) *applied = o;
    return jpeg_slot_finish(slot, &landed, off, 0, true, channel_order, status);
}

// ---- clips of JPEG streams (the contract is in engine.h) ----
struct Engine::JpegClipJob {
    int frames = 0;
    std::vector<whenet_jpeg_info_t> info;
    // the orientation each frame's kernel applies (1: upright) and the headers with the sides of the frames as they land
    int orient[MIXED_MAX_FRAMES];
    std::vector<whenet_jpeg_info_t> landed;
    JpegDecGeom g[MIXED_MAX_FRAMES];
    int64_t nbytes[MIXED_MAX_FRAMES];
    JpegClipPlan plan;
    int rule = JPEG_RULE_OWN;      // the clip's decode rule: one for all of its frames
    // a clip that accepts progressive streams: every frame's scan plan (`baseline` for a SOF0 stream) and the layout; `plan` is its base
    bool progressive = false;
    std::vector<JpegProgPlan> prog;
    JpegClipProgPlan pplan;
    bool is_prog(int f) const { return progressive && !prog[size_t(f)].baseline; }
};

void Engine::jpeg_clip_prepare(const char* what, const uint8_t* const* data, const int64_t* size, int nframes, int entropy, int seg_bytes,
                               int rule, JpegClipJob& job, int progressive, int orient) const {
    const std::string w(what);
    job.rule = jpeg_rule_of(what, rule);
    WHENET_REQUIRE(nframes >= 1 && nframes <= MIXED_MAX_FRAMES, WHENET_EINVAL,
                   w + ": " + std::to_string(nframes) + " frames: a clip holds 1..16 (the detector's batch limit)");
    WHENET_REQUIRE(data != nullptr && size != nullptr, WHENET_EINVAL, w + ": NULL argument");
    WHENET_REQUIRE(orient == 0 || orient == 1, WHENET_EINVAL, w + ": orient must be 0 (the orientation is ignored) or 1 (it is applied)");
    job.frames = nframes;
    job.info.resize(size_t(nframes));
    job.landed.resize(size_t(nframes));
    WHENET_REQUIRE(jpeg_accept_ok(progressive), WHENET_EINVAL, w + ": the accept bits must be 0..3 (1: progressive streams, 2: layouts)");
    job.progressive = progressive != 0;      // (every frame has a scan plan: `baseline` where the baseline decoder takes it)
    if (job.progressive) job.prog.resize(size_t(nframes));
    for (int f = 0; f < nframes; ++f) {
        const std::string who = w + ": frame " + std::to_string(f);
        JpegProgPlan none;
        jpeg_parse_accept_or_refuse(who.c_str(), data[f], size[f], job.info[f], job.progressive ? job.prog[size_t(f)] : none, progressive);
        job.g[f] = jpeg_dec_geom(job.info[f]);
        job.nbytes[f] = size[f] - job.info[f].data_offset;
        job.orient[f] = orient != 0 ? jpeg_exif_orientation(data[f], size[f]) : 1;
        job.landed[f] = jpeg_orient_info(job.info[f], job.orient[f]);
    }
    const int ent = entropy >= 0 ? entropy : jpeg_entropy_, seg = seg_bytes > 0 ? seg_bytes : jpeg_seg_bytes_;
    const char* bad = nullptr;
    if (job.progressive) {
        const JpegProgPlan* plans[MIXED_MAX_FRAMES];
        for (int f = 0; f < nframes; ++f) plans[f] = &job.prog[size_t(f)];
        bad = jpeg_clip_plan_progressive(job.g, job.nbytes, plans, nframes, ent, seg, job.pplan);
        job.plan = job.pplan.base;
    } else {
        bad = jpeg_clip_plan(job.g, job.nbytes, nframes, ent, seg, job.plan);
    }
    WHENET_REQUIRE(bad == nullptr, WHENET_EINVAL, w + ": " + (bad ? bad : ""));
}

void Engine::jpeg_clip_stage(const JpegClipJob& job, const uint8_t* const* data, uint8_t* stage, void* d_base, const whenet_surface_t* dst,
                             int channel_order, int32_t* d_status, JpegDecArgs* recs, JpegProgArgs* precs) const {
    const JpegClipPlan& p = job.plan;
    char* const s = static_cast<char*>(d_base);
    std::memset(stage + p.records.off, 0, p.records.len);
    for (int f = 0; f < job.frames; ++f) {
        const JpegClipFrame& q = p.f[f];
        precs[f] = JpegProgArgs{};
        uint8_t* const rec = stage + p.records.off + size_t(f) * JPEG_CLIP_RECORD_BYTES;
        if (job.is_prog(f)) {
            // the frame's record over its progressive regions (tables: the scans' Huffman tables, start: the item list), its progressive
            // record behind it, its scan plan's share of the upload
            const JpegClipProgFrame& r = job.pplan.pf[f];
            const JpegProgPlan& plan = job.prog[size_t(f)];
            JpegClipFrame regions = q;
            regions.tables = r.huff, regions.start = r.items;
            const JpegDecArgs a =
                jpeg_dec_args(job.g[f], d_base, regions, plan.data_bytes, dst[f], channel_order, d_status + 2 * f, job.rule, 0, job.orient[f]);
            JpegProgArgs x{};
            x.g = job.g[f];
            x.scans = reinterpret_cast<const JpegProgScan*>(s + r.scans.off), x.huff = reinterpret_cast<const JpegDecHuff*>(s + r.huff.off);
            x.qz = reinterpret_cast<const int16_t*>(s + r.qz.off), x.items = reinterpret_cast<const JpegProgItem*>(s + r.items.off);
            x.data = a.data, x.nbytes = a.nbytes;
            x.raw = reinterpret_cast<int16_t*>(s + r.raw.off), x.coef = a.coef, x.meta = a.meta, x.first_bad = plan.first_bad;
            recs[f] = a, precs[f] = x;
            std::memcpy(rec, &a, sizeof(a));
            std::memcpy(rec + JPEG_CLIP_PROG_RECORD_OFFSET, &x, sizeof(x));
            jpeg_clip_stage_progressive(plan, q, r, data[f] + plan.data_base, stage);
            continue;
        }
        recs[f] = jpeg_dec_args(job.g[f], d_base, q, job.nbytes[f], dst[f], channel_order, d_status + 2 * f, job.rule, jpeg_seg_lanes_, job.orient[f]);
        std::memcpy(rec, &recs[f], sizeof(JpegDecArgs));
        JpegDecTables* const t = reinterpret_cast<JpegDecTables*>(stage + q.tables.off);      // (256-byte aligned in pinned or vector memory)
        jpeg_dec_build_tables(job.info[f], *t);
        if (q.data.len > 0) std::memcpy(stage + q.data.off, data[f] + job.info[f].data_offset, q.data.len);
    }
}

void Engine::add_jpeg_clip_counters(int64_t out[4]) const {
    for (int i = 0; i < 4; ++i) out[i] += jpeg_clip_counts_[i];
}

void Engine::jpeg_clip_launch(const JpegClipJob& job, const JpegDecArgs* recs, const JpegProgArgs* precs, char* d_base, hipStream_t stream) {
    const JpegClipPlan& plan = job.plan;
    const int nframes = job.frames;
    if (job.progressive) {
        const JpegProgPlan* plans[MIXED_MAX_FRAMES];
        for (int f = 0; f < nframes; ++f) plans[f] = job.is_prog(f) ? &job.prog[size_t(f)] : nullptr;
        launch_jpeg_decode_clip_progressive(recs, precs, plans, d_base + plan.records.off, nframes, d_base + plan.zero.off, plan.zero.len, stream,
                                            &jpeg_clip_counts_[2], &jpeg_prog_counts_[1]);
    } else {
        launch_jpeg_decode_clip(recs, d_base + plan.records.off, nframes, d_base + plan.zero.off, plan.zero.len, stream, &jpeg_clip_counts_[2]);
    }
    ++jpeg_clip_counts_[0], jpeg_clip_counts_[1] += nframes, ++jpeg_clip_counts_[3];
    for (int f = 0; f < nframes; ++f) {
        if (job.is_prog(f)) ++jpeg_prog_counts_[0], jpeg_prog_counts_[2] += int64_t(job.prog[size_t(f)].dev.size());
        else ++jpeg_dec_launched_[plan.f[f].form];
    }
}

int Engine::clip_begin_jpeg(const uint8_t* const* data, const int64_t* size, int nframes, int channel_order, int32_t* status, int rule,
                            int progressive, int orient, int* applied) {
    DeviceGuard guard(device_);
    WHENET_REQUIRE(status != nullptr, WHENET_EINVAL, "clip_begin_jpeg: NULL argument");
    WHENET_REQUIRE(channel_order == WHENET_RGB || channel_order == WHENET_BGR, WHENET_EINVAL, "clip_begin_jpeg: unknown channel order");
    JpegClipJob job;
    jpeg_clip_prepare("clip_begin_jpeg", data, size, nframes, -1, 0, rule, job, progressive, orient);      // (before a slot is taken)
    bool one_size = true;      // (by the sizes of the frames as they land)
    for (int f = 1; f < nframes; ++f) one_size = one_size && job.landed[f].h == job.landed[0].h && job.landed[f].w == job.landed[0].w;
    WHENET_REQUIRE(one_size || nframes <= lb_cache_cap_, WHENET_EINVAL,
                   "clip_begin_jpeg: " + std::to_string(nframes) + " frames of their own sizes need option letterbox_cache >= " +
                       std::to_string(nframes) + " (it is " + std::to_string(lb_cache_cap_) + ")");
    size_t off[MIXED_MAX_FRAMES + 1];
    whenet_surface_t dst[MIXED_MAX_FRAMES];
    int32_t* d_status = nullptr;
    Slot& slot = jpeg_slot_begin(job.landed.data(), nframes, job.plan.upload_bytes, job.plan.bytes, off, dst, d_status);
    JpegDecArgs recs[MIXED_MAX_FRAMES];
    JpegProgArgs precs[MIXED_MAX_FRAMES];
    uint8_t* const stage = slot.frame.h.as<uint8_t>();
    jpeg_clip_stage(job, data, stage, slot.jpg_dec.as<void>(), dst, channel_order, d_status, recs, precs);
    WHENET_HIP_CHECK(hipMemcpyAsync(slot.jpg_dec.as<void>(), stage, job.plan.upload_bytes, hipMemcpyHostToDevice, copy_stream()));
    jpeg_clip_launch(job, recs, precs, slot.jpg_dec.as<char>(), copy_stream());
    if (applied != nullptr) std::copy(job.orient, job.orient + nframes, applied);
    return jpeg_slot_finish(slot, job.landed.data(), off, nframes, one_size, channel_order, status);
}

void Engine::op_jpeg_decode_clip(const uint8_t* const* data, const int64_t* size, int nframes, const whenet_surface_t* dst, int channel_order,
                                 int32_t* status, int entropy, int seg_bytes, int rule, int progressive, int orient, int* applied) {
    DeviceGuard guard(device_);
    WHENET_REQUIRE(status != nullptr && dst != nullptr, WHENET_EINVAL, "op_jpeg_decode_clip: NULL argument");
    JpegClipJob job;
    jpeg_clip_prepare("op_jpeg_decode_clip", data, size, nframes, entropy, seg_bytes, rule, job, progressive, orient);
    GuardedSurfaces out;
    for (int f = 0; f < nframes; ++f) {
        const std::string who = "op_jpeg_decode_clip: frame " + std::to_string(f);
        jpeg_orient_require_packed(who, job.orient[f], dst[f]);
        const char* bad = jpeg_dec_check_dst(job.landed[f], &dst[f], channel_order, job.rule);
        WHENET_REQUIRE(bad == nullptr, WHENET_EINVAL, who + ": " + (bad ? bad : ""));
        WHENET_REQUIRE(dst[f].on_device == 0, WHENET_EINVAL, who + ": the surface must be host memory (on_device = 0)");
        check_surface(who.c_str(), dst[f], job.landed[f].h, job.landed[f].w);
        out.add(dst[f], job.landed[f].h, job.landed[f].w);
    }
    const JpegClipPlan& plan = job.plan;
    TempBufs tmp;
    char* const d_work = static_cast<char*>(tmp.get(plan.bytes));
    int32_t* const d_status = static_cast<int32_t*>(tmp.get(size_t(nframes) * 2 * sizeof(int32_t)));
    out.alloc(stream_);
    std::vector<uint8_t> stage(plan.upload_bytes + 256);
    uint8_t* const st = stage.data() + ((256 - (reinterpret_cast<uintptr_t>(stage.data()) & 255)) & 255);
    JpegDecArgs recs[MIXED_MAX_FRAMES];
    JpegProgArgs precs[MIXED_MAX_FRAMES];
    jpeg_clip_stage(job, data, st, d_work, out.device(), channel_order, d_status, recs, precs);
    WHENET_HIP_CHECK(hipMemcpyAsync(d_work, st, plan.upload_bytes, hipMemcpyHostToDevice, stream_));
    jpeg_clip_launch(job, recs, precs, d_work, stream_);
    if (applied != nullptr) std::copy(job.orient, job.orient + nframes, applied);
    out.to_host(stream_, "op_jpeg_decode_clip", "the surfaces");      // waits
    WHENET_HIP_CHECK(hipMemcpy(status, d_status, size_t(nframes) * 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
}

}  // namespace whenet
