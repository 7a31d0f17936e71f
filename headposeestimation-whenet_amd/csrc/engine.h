// The per-GPU inference engine behind the C ABI: device weights, activation arena, launch
// schedule of the kernels of one forward, hipGraph cache, per-launch profiling, and the
// pinned-buffer submit/collect pipeline.  One engine = one device + one stream; not thread-safe.
#pragma once

#include <deque>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "common.h"
#include "kernels.h"
#include "snapshot.h"

namespace whenet {

// Move-only owners of what the engine takes from the runtime: each frees its resource in its destructor, on whichever device is
// current.  ~Engine selects the engine's own first; when a constructor throws part-way they go with the caller's device current,
// which hipFree / hipHostFree / hipEventDestroy / hipStreamDestroy accept (the handle carries its device).
template <typename H, hipError_t (*Destroy)(H)>
class Owned {
  public:
    Owned() = default;
    Owned(Owned&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    ~Owned() { reset(); }
    void reset() {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }
    H* put() {             // for the hip...Create call that fills it
        reset();
        return &h_;
    }
    operator H() const { return h_; }

  private:
    H h_ = nullptr;
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
struct Event : Owned<hipEvent_t, hipEventDestroy> {
    void create(unsigned flags = hipEventDisableTiming) { WHENET_HIP_CHECK(hipEventCreateWithFlags(put(), flags)); }
};

struct DeviceMem {
    static constexpr const char* NAME = "hipMalloc";
    static hipError_t alloc(void** p, size_t nbytes) { return hipMalloc(p, nbytes); }
    static void release(void* p) { (void)hipFree(p); }
};
struct PinnedMem {
    static constexpr const char* NAME = "hipHostMalloc";
    static hipError_t alloc(void** p, size_t nbytes) { return hipHostMalloc(p, nbytes, hipHostMallocDefault); }
    static void release(void* p) { (void)hipHostFree(p); }
};
template <typename Mem>
class Buffer {
  public:
    Buffer() = default;
    Buffer(Buffer&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr, o.bytes_ = 0; }
    ~Buffer() { release(); }
    size_t bytes() const { return bytes_; }
    template <typename T> T* as() const { return static_cast<T*>(p_); }
    void release() {
        if (p_) Mem::release(p_);
        p_ = nullptr, bytes_ = 0;
    }
    hipError_t try_reset(size_t nbytes) {          // free, then allocate (zero bytes allocates 16)
        release();
        const hipError_t e = Mem::alloc(&p_, nbytes ? nbytes : 16);
        if (e == hipSuccess) bytes_ = nbytes;
        else p_ = nullptr;
        return e;
    }
    // what: the sites that report a failed allocation as out of memory under their own text; the others report the HIP call
    void reset(size_t nbytes, const char* what = nullptr) {
        const hipError_t e = try_reset(nbytes);
        if (e == hipSuccess) return;
        if (what) throw Error(WHENET_ENOMEM, std::string(what) + ": " + hipGetErrorString(e));
        throw Error(WHENET_EHIP, std::string(Mem::NAME) + " of " + std::to_string(nbytes) + " bytes: " + hipGetErrorString(e));
    }
    void grow(size_t nbytes) {
        if (nbytes > bytes_) reset(nbytes);
    }

  private:
    void* p_ = nullptr;
    size_t bytes_ = 0;
};
using DeviceBuffer = Buffer<DeviceMem>;
using PinnedBuffer = Buffer<PinnedMem>;
struct StagedBuffer {      // a pinned host buffer and its device twin
    PinnedBuffer h;
    DeviceBuffer d;
};

// The three result arrays of a forward (argmax / logits may be nullptr where the caller does not want them).
struct Results {
    float* ypr;
    int32_t* amax;
    float* logits;
    Results at(size_t crop) const {
        return {ypr + crop * 3, amax ? amax + crop * 3 : nullptr, logits ? logits + crop * N_LOGITS : nullptr};
    }
};

struct DevPw {
    int K = 0, N = 0, KS = 0, NTILES = 0;
    void* wp = nullptr;
    void* wps = nullptr;       // WHENET_F32S: split weight images (HostPw::packed_split)
    int KSs = 0;
    float wsi = 1.0f;
    float* wdense = nullptr;
    float* bias = nullptr;
};
struct DevDw {
    int k = 0, C = 0;
    float* w = nullptr;
    float* bias = nullptr;
    half_t* wt = nullptr;      // f16: Toeplitz operand image of the kernel for front2.hip (pack_dw_toeplitz)
    half_t* wt7 = nullptr;     // f16, 7 x 7 blocks: the image front7.hip reads (group-aligned: xs = 4 - k / 2)
    float* wts = nullptr;      // WHENET_F32S: Toeplitz operand image for front2s.hip in the block's tap mode (pack_dw_toeplitz_s)
    float wts_wsi = 1.0f;      //   2^-shift of its scaled taps (tap mode 1)
    DwPlan plan;
};
struct DevSe {
    int C = 0, R = 0;
    float *w1t = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;
    float* w2c = nullptr;      // [C][RP] (se.hip reads a channel's whole excite row with 16-byte loads)
    void* w2p = nullptr;       // the excite kernel as an MFMA operand image (HostSe::excite), or nullptr
    int KSr = 0;
    float w2_wsi = 1.0f;
};
struct DevMb7 {                 // f16, blocks 13-16: operand images of the one-launch block kernel (mb7.hip)
    bool ok = false;
    half_t *wds = nullptr, *w1p = nullptr, *w2p = nullptr;
};
struct DevBlock {
    BlockSpec spec;
    DevPw expand;
    DevDw dw;
    FrontPlan fplan;       // fused expand+depthwise tiling (blocks with an expand conv)
    Front2Plan f2plan;     // f16: the same stage with the taps on the matrix cores (front2.hip)
    bool f2_preferred = false;
    Front2Plan f2splan;    // WHENET_F32S: front2s.hip's plan, tap mode, and whether it is the faster kernel on this layer
    int f2s_tm = 2;
    bool f2s_supported = false, f2s_preferred = false;
    bool f7_supported = false; // f16: the block's shape has a front7.hip kernel (7 x 7 maps, blocks 13-16)
    int f7_chunks = 1;         // channel chunks of its plans (the same for every group size: see front7_plan_for)
    DevSe se;
    DevPw project;
    DevMb7 mb7;
};

// Collects one entry per kernel launch when profiling (event pair around each launch).
struct LaunchRecorder {
    struct Entry {
        std::string layer, kind, kernel;
        double bytes = 0, flops = 0;
        Event stop;                      // recorded right after the launch; the previous entry's stop
        double total_ms = 0;             // (or the chain's start event) is this launch's start
    };
    std::vector<Entry> entries;
    Event start;                         // recorded on the chain's stream before its first launch
    size_t cursor = 0;
    bool first_pass = true;
};

constexpr int MAX_LANES = 8;

// One row of the detector body's layer table (detector.cpp): a convolution or a pool in the reference's layer-creation order; the
// layers around it (zero padding, BatchNorm, LeakyReLU, Add, UpSampling2D + Concatenate) are properties of the row.
enum { DET_CONV = 0, DET_POOL = 1 };
struct DetLayer {
    int op, k, stride, cin, cout, bn, leaky;
    int src0;          // row whose output is read (-1: the image); with src1 it is the HALF-resolution tensor, upsampled by 2
    int src1;          // row concatenated behind the upsampled src0 (channels cin0..), or -1
    int skip;          // row added to the activated output (Add), or -1
    int is_output;     // linear convolution with a bias, float32 map [gh][gw][A (5 + C)]
    int cin0;          // channels of src0
};
std::vector<DetLayer> detector_table(int kind, int out_filters);      // kind 0 = yolo_body (75 rows), 1 = tiny_yolo_body (19 rows)
struct Detector;
struct DetPlan;

class Engine {
  public:
    Engine(const void* snapshot, size_t nbytes, int device_id, int dtype);      // dtype: WHENET_F32 / F16 / F32S
    explicit Engine(int device_id);      // no network: device + stream + scratch for the frame / detector stages only
    ~Engine();
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;

    void set_option(const std::string& key, long value);
    void get_info(whenet_info_t* out) const;

    void forward_host(const uint8_t* crops, int n, float* ypr, int32_t* argmax, float* logits);
    void forward_host_f32(const float* x, int n, float* ypr, int32_t* argmax, float* logits);
    void forward_device(const uint8_t* d_crops, int n, float* d_ypr, int32_t* d_argmax, float* d_logits,
                        hipStream_t stream);
    void sync();
    void release_aux_streams();
    // stage: 0 = through the slot's pinned staging buffer, 1 = DMA straight from the caller's memory (pageable: the host blocks for the
    // copy; registered: asynchronous).
    // copy_on: the stream the H2D copy is issued on (default: this engine's own copy stream) -- a fan-out puts every chunk's copy on ONE
    // stream: in order, at the link's full rate
    // copy_after: the copy starts only after this event (the previous chunk's copy on ANOTHER engine's copy stream)
    int submit(const uint8_t* crops, int n, int stage = 0, int want_lanes = 0, hipStream_t copy_on = nullptr, hipEvent_t copy_after = nullptr);
    hipStream_t copy_stream_handle();
    hipEvent_t copied_event(int ticket) const;     // recorded when the H2D copy of that submission is done
    void abandon_submissions();
    bool has_pending() const {
        for (const Slot& s : slots_)
            if (s.busy) return true;
        return false;
    }
    int submit_frame(const uint8_t* frame, int fh, int fw, int swap_rb, const int32_t* rects, int k);
    void op_crop_resize(const uint8_t* frame, int fh, int fw, int swap_rb, const int32_t* rects, int k,
                        uint8_t* crops_out);
    void collect(int ticket, float* ypr, int32_t* argmax, float* logits);
    // a frame_detect_heads ticket: one wait, then the detections (count rows of each array) and their heads' results; the rows of
    // heads without a window inside the frame are NaN / -1 / NaN.  Returns the number of detections.
    int collect_detect(int ticket, int capacity, float* boxes, float* scores, int32_t* classes, int32_t* rects, int32_t* valid, float* ypr,
                       int32_t* argmax, float* logits);
    // the detector's letterbox (letterbox.hip) alone on a host frame, and the resident-frame form of submit_frame: the frame is
    // uploaded when it arrives (the ticket is handed out and the slot held from then on), the detector input and the head crops
    // are both cut from that one device copy; collect() returns the heads' results and frees the slot
    void op_letterbox(const uint8_t* frame, int fh, int fw, int swap_rb, int out_h, int out_w, uint8_t* canvas_u8, float* image_f32);
    int frame_begin(const uint8_t* frame, int fh, int fw, int swap_rb);
    void frame_letterbox(int ticket, int out_h, int out_w, uint8_t* canvas_u8, float* image_f32);
    void frame_heads(int ticket, const int32_t* rects, int k);
    int profile(const uint8_t* d_crops, int n, int iters, whenet_launch_stat_t* stats, int cap);

    void op_stem(const uint8_t* crops, int n, float* out);
    int yolo_eval(const float* const* feats, const int* grid_h, const int* grid_w, int num_layers, const float* anchors,
                  int num_anchors, int num_classes, float image_h, float image_w, float score_threshold,
                  float iou_threshold, int max_boxes, float* boxes, float* scores, int32_t* classes, int32_t* index,
                  float* all_boxes, float* all_scores);
    void op_block(int index, const float* in, int n, float* expand_out, float* dw_out, float* gate, float* out);
    void op_block_range(int first, int last, const float* in, int n, float* out);
    void op_head(const float* in, int n, float* feat, float* logits, float* ypr, int32_t* argmax);
    void op_decode(const float* logits, int n, float* ypr, int32_t* argmax);
    // the detector body (detector.cpp): attach its weights, the body alone on host images, YOLO.detect on a host frame and on a
    // resident one (letterbox -> body -> yolo_eval on the device; return the number of detections), and single layers for the tests
    void detector_load(const void* snapshot, size_t nbytes);
    void share_detector(const Engine& from);
    bool has_detector() const { return det_ != nullptr; }
    void detector_forward(const float* image, int n, int H, int W, float* const* maps);
    int op_detect(const uint8_t* frame, int fh, int fw, int swap_rb, int out_h, int out_w, const float* anchors, int num_anchors,
                  float score_threshold, float iou_threshold, int max_boxes, float* boxes, float* scores, int32_t* classes);
    int frame_detect(int ticket, int out_h, int out_w, const float* anchors, int num_anchors, float score_threshold, float iou_threshold,
                     int max_boxes, float* boxes, float* scores, int32_t* classes);
    // ONE enqueue-only submission per resident frame: letterbox -> body -> yolo_eval -> head plans (headplan.hip) -> crops over the
    // capacity C * max_boxes -> forward -> D2H of detections and results; nothing waits and nothing returns to the host in between
    void frame_detect_heads(int ticket, int out_h, int out_w, const float* anchors, int num_anchors, float score_threshold,
                            float iou_threshold, int max_boxes);
    // the plan kernel alone on caller boxes (host pointers): rects [k,4], valid [k], plans [k][CROP_PLAN_INTS] (may be nullptr)
    void op_head_plan(int fh, int fw, const float* boxes, int k, int32_t* rects, int32_t* valid, int32_t* plans);
    // A CLIP: F frames of one size as one submission (detector.cpp).  clip_begin uploads [F][fh][fw][3] once and holds the slot;
    // clip_detect_heads (enqueue-only; returns K = slots per frame) runs letterbox, body, selection and head plans over the F
    // frames, numbers the heads that have a window (headplan.hip's compaction) and runs the forward over max_heads rows
    // (0: min(F * K, 256)); collect_clip waits once and scatters: slot (f, i) gets the result of its row, or NaN / -1 / NaN.
    int clip_begin(const uint8_t* frames, int nframes, int fh, int fw, int swap_rb);
    int clip_detect_heads(int ticket, int out_h, int out_w, const float* anchors, int num_anchors, float score_threshold, float iou_threshold,
                          int max_boxes, int max_heads);
    void collect_clip(int ticket, int capacity, int* nframes, int32_t* counts, float* boxes, float* scores, int32_t* classes, int32_t* rects,
                      int32_t* valid, int32_t* row, float* ypr, int32_t* argmax, float* logits, int* rows_used, int* overflow);
    // single stages of a clip on host arrays, for the tests: the letterbox of F frames, the selection of F images (outputs
    // [F][C * max_boxes]..., counts [F]) and the compaction kernel alone
    void op_letterbox_batch(const uint8_t* frames, int nframes, int fh, int fw, int swap_rb, int out_h, int out_w, uint8_t* canvas_u8,
                            float* image_f32);
    void yolo_eval_batch(const float* const* feats, int images, const int* grid_h, const int* grid_w, int num_layers, const float* anchors,
                         int num_anchors, int num_classes, float image_h, float image_w, float score_threshold, float iou_threshold,
                         int max_boxes, float* boxes, float* scores, int32_t* classes, int32_t* index, int32_t* counts);
    // A MIXED clip: F frames, each of its own size, packed back to back (offsets = prefix sums of fh * fw * 3, no padding) with
    // one pinned staging copy and one H2D.  clip_detect_heads / collect_clip take its ticket as they take clip_begin's: every
    // frame's geometry comes from the letterbox cache (pinned while the launches are enqueued), the stages that depend on the
    // frame size run their mixed kernels, everything from the compaction on is the same code.  Frame f returns the bytes that
    // frame_begin; frame_detect_heads; collect_detect return for it alone.
    int clip_begin_mixed(const uint8_t* const* frames, int nframes, const int* fh, const int* fw, int swap_rb);
    // argument checks of the two calls above without an engine's state (the C ABI runs them before it takes an engine)
    static void check_mixed_frames(const char* what, const uint8_t* const* frames, int nframes, const int* fh, const int* fw);
    void op_letterbox_mixed(const uint8_t* const* frames, int nframes, const int* fh, const int* fw, int swap_rb, int out_h, int out_w,
                            uint8_t* canvas_u8, float* image_f32);
    // yolo_eval_batch over images of different shapes: image_shapes [images][2] = (h, w)
    void yolo_eval_mixed(const float* const* feats, int images, const int* grid_h, const int* grid_w, int num_layers, const float* anchors,
                         int num_anchors, int num_classes, const float* image_shapes, float score_threshold, float iou_threshold,
                         int max_boxes, float* boxes, float* scores, int32_t* classes, int32_t* index, int32_t* counts);
    void add_letterbox_cache_stats(int32_t out[4]) const;      // entries, hits, misses, host_waits
    // YUV 4:2:0 INGEST (yuv.hip): the decoder's planes are staged tight in the slot's pinned staging and travel in ONE H2D of
    // 1.5 bytes per pixel; the conversion kernel runs on the copy stream behind that copy and BEFORE slot.copied is recorded, so the
    // slot's frame buffer holds the packed BGR frame for every consumer that waits for the event, none of which changes.  The
    // callers have run check_yuv_frames.  clip_begin_yuv: frames of one size make a clip_begin slot, otherwise a clip_begin_mixed
    // slot (the packing is the same: back to back); op_yuv_to_bgr is the kernel alone, host to host, packed the same way.
    int frame_begin_yuv(const whenet_yuv_frame_t& frame);
    int clip_begin_yuv(const whenet_yuv_frame_t* frames, int nframes);
    void op_yuv_to_bgr(const whenet_yuv_frame_t* frames, int nframes, uint8_t* const* bgr);
    // INGEST FROM DEVICE MEMORY (ingest.hip, yuv.hip): the twins of frame_begin / clip_begin / clip_begin_mixed / frame_begin_yuv /
    // clip_begin_yuv for a source that is already in this device's memory -- packed 3-byte pixels with a row pitch, or NV12 / I420
    // planes with their pitches.  One kernel writes the slot's tight frame buffer; the slot ends up exactly as the host-pointer
    // twin leaves it and every later call runs unchanged.  No pinned staging is grown or touched.
    //   ORDER.  `stream` is the caller's hipStream_t (nullptr: the default stream).  An event is recorded on it, the copy stream
    //   waits for that event, the kernel runs, slot.copied is recorded, and the caller's stream is made to wait for slot.copied.  So:
    //   work the caller enqueued on `stream` BEFORE the call is seen by the ingest; work it enqueues on `stream` AFTER the call may
    //   overwrite or free the source; anything else that writes the source -- the host, another stream -- must wait until the
    //   ticket's collect has returned.  The host never waits here.
    //   CHECKS, all before a slot is taken or anything is enqueued, WHENET_EINVAL with the frame's index in the text: NULL pointers,
    //   a pitch below the row bytes, sides outside 1..8192, a frame count outside 1..16, unknown format or matrix; every plane must
    //   be hipMemoryTypeDevice memory of THIS engine's device (hipPointerGetAttributes: host, managed and other-device pointers
    //   are refused) and its extent (rows - 1) * pitch + row_bytes must lie inside the allocation hipMemGetAddressRange reports
    //   for it.  If the runtime cannot report the range, the extent check alone is skipped.
    // clip_begin_device: frames of one size make a clip_begin slot, otherwise a clip_begin_mixed slot (letterbox_cache limit).
    // op_pack_device / op_yuv_to_bgr_device: the kernels alone, device to host (out[f] = uint8 [h_f][w_f][3]), packed back to back
    // on the device as a mixed clip packs them; the host waits.
    int frame_begin_device(const uint8_t* d_frame, int pitch, int fh, int fw, int swap_rb, hipStream_t stream);
    int clip_begin_device(const uint8_t* const* d_frames, const int* pitch, int nframes, const int* fh, const int* fw, int swap_rb,
                          hipStream_t stream);
    int frame_begin_yuv_device(const whenet_yuv_frame_t& frame, hipStream_t stream);
    int clip_begin_yuv_device(const whenet_yuv_frame_t* frames, int nframes, hipStream_t stream);
    void op_pack_device(const uint8_t* const* d_frames, const int* pitch, int nframes, const int* fh, const int* fw, hipStream_t stream,
                        uint8_t* const* out);
    void op_yuv_to_bgr_device(const whenet_yuv_frame_t* frames, int nframes, hipStream_t stream, uint8_t* const* bgr);
    // EXTENDED YUV INGEST (yuvx.hip; include/whenet_hip_yuv_ext.h): the twins of the seven YUV calls above for whenet_yuvx_frame_t --
    // 16-bit containers, planar 4:4:4, BT.2020, and the old formats through the same struct.  The slots, the stream order, the size
    // rules of a clip and the device-pointer checks are those of the calls above; the planes of a host frame are staged by
    // YuvxLayout (a 16-bit frame at an even offset).  begin_yuvx is the one body of the four begin calls: `clip` tells whether the
    // slot is a clip's, `device` whether the planes are device memory ordered on `stream`.
    int begin_yuvx(const char* what, const whenet_yuvx_frame_t* frames, int nframes, bool clip, bool device, hipStream_t stream);
    void op_yuvx_to_bgr(const whenet_yuvx_frame_t* frames, int nframes, uint8_t* const* bgr);
    void op_yuvx_to_bgr_device(const whenet_yuvx_frame_t* frames, int nframes, hipStream_t stream, uint8_t* const* bgr);
    // POSE OVERLAY (overlay.hip; the contract is in include/whenet_hip.h).  frame_annotate: between the call that enqueues a ticket's
    // heads and its collect -- the plan kernel (windows, valid flags and angles where the heads' launches leave them: the crop
    // plans of submit_frame / frame_heads, the DetRows of frame_detect_heads, the ClipRows + row map of clip_detect_heads) and the
    // draw kernel go on stream_ behind the forward, slot.done is recorded again behind them.  ENQUEUE-ONLY.
    //   Device destination: written in place; with `stream` the engine's stream first waits for what the caller enqueued on it (the
    //   previous reader of the surface) and `stream` then waits for the kernel's end.  Host destination: the kernel writes tight
    //   planes in the slot's staging (one buffer pair per frame index), one D2H behind it; the collect call copies the rows out.
    //   Every refusal (WHENET_EINVAL) comes before anything is enqueued and leaves the ticket as it was.
    // op_annotate: the two kernels alone, host to host.
    // display: WHENET_DISPLAY_SIMPLE, or WHENET_DISPLAY_FULL -- the plan kernel then also writes the heads' label records (one more
    // per-slot table) and the draw kernel's other instantiation paints them.
    void frame_annotate(int ticket, int frame_index, const whenet_surface_t& dst, hipStream_t stream, int display);
    void op_annotate(const uint8_t* frame, int fh, int fw, int channel_order, const int32_t* rects, const int32_t* valid, const float* ypr,
                     int k, const whenet_surface_t& dst, int display);
    // JPEG ENCODER (jpeg.hip; the contract is in include/whenet_hip.h).  op_jpeg_encode: the kernels alone, host to host: the planes
    // are uploaded tight, the stream lands between two guard zones and min(size, cap) bytes of it go to the caller; the host waits.
    // jpeg_encode_device: ENQUEUE-ONLY on stream_ between the two event hand-overs of the device ingest; the work buffers are the
    // engine's (grown on the first call for a size), the tables and header of an (h, w, quality) are uploaded once and kept.
    // sampling / optimize: include/whenet_hip.h, SAMPLING AND OPTIMISED TABLES; hist (host, may be nullptr): the device histograms.
    void op_jpeg_encode(const whenet_surface_t& src, int h, int w, int channel_order, int quality, uint8_t* out, int64_t cap, int64_t* size,
                        int sampling = WHENET_JPEG_420, bool optimize = false, uint32_t (*hist)[256] = nullptr);
    void jpeg_encode_device(const whenet_surface_t& src, int h, int w, int channel_order, int quality, void* dst, int64_t cap, int64_t* dsize,
                            hipStream_t stream, int sampling = WHENET_JPEG_420, bool optimize = false);
    // frame_annotate_jpeg: frame_annotate into a surface of the slot's own (tight I420, JFIF matrix), the encoder behind it on stream_
    // into a landing buffer in device memory, and a flush kernel that copies min(length, cap) bytes and the length into pinned host
    // memory -- the total is data-dependent and the call must not wait, so no copy of a size known to the host can stand there.
    // ENQUEUE-ONLY; the collect call hands the bytes, the length and the status to the caller.  It counts as the frame's one annotate.
    // At 4:2:2 / 4:4:4 the slot's surface is PACKED pixels in the frame's channel order: an I420 surface cannot carry their chroma.
    void frame_annotate_jpeg(int ticket, int frame_index, int display, int quality, uint8_t* out, int64_t cap, int64_t* size, int32_t* status,
                             int sampling = WHENET_JPEG_420, bool optimize = false);
    // JPEG DECODER (jpeg_dec.hip; the contract is in include/whenet_hip.h).  Every entry point parses (or checks the info) on the host
    // first: a refused stream is WHENET_EFORMAT before a slot is taken or anything is enqueued.
    // op_jpeg_decode: the kernels alone, host to host; the destination lands at the caller's pitches between two guard zones.
    // jpeg_decode_device: ENQUEUE-ONLY on stream_ between the two event hand-overs of the device ingest; the work buffers are the
    // engine's (grown on the first call for a size).
    // frame_begin_jpeg: frame_begin whose H2D carries the compressed bytes (and the decode tables, one copy) and whose kernels run
    // on the copy stream before slot.copied; the two status words come back through pinned memory with the ticket's collect call.
    // The entropy stage's form (0: an interval per lane, 1: segmented, jpeg_dec_seg.hip) follows the options "jpeg_entropy" (2: auto,
    // by the bytes per interval) and "jpeg_seg_bytes"; op_jpeg_decode takes them from its arguments where entropy >= 0 and reads the
    // segmented form's statistics back into stats (8 int64, may be nullptr).
    // The decode RULE (0: the project's own inverse DCT, nearest chroma and JFIF row; 1: libjpeg's bytes -- jidctint, fancy
    // upsampling, jdcolor -- into packed destinations only) follows the option "jpeg_rule" (default 0) wherever `rule` is -1.
    // PROGRESSIVE streams (SOF2; jpeg_prog.hip, JPEG DECODER, PROGRESSIVE in the header) are opt-in: progressive = 1, or -1 with the
    // option "jpeg_progressive" set.  Then a SOF2 stream runs the scan plan (one H2D), a memset, a scan-kernel launch per level
    // (option "jpeg_prog_levels" = 0: per scan) and the finish in front of the inverse DCT; a SOF0 stream runs as ever.
    // ORIENTED decode (JPEG DECODER, ORIENTATION in the header) is opt-in: orient = 1, or -1 with the option "jpeg_orient" set (the
    // single-stream calls; clips take the argument only).  Then the stream's EXIF orientation (jpeg_exif_orientation, 1..8) goes into
    // the record and the frame kernel's place is taken by the oriented one: the destination, the slot's frame and its sizes are the
    // ORIENTED frame's (5..8: w rows of h pixels), no upright frame exists anywhere and no launch is added (a clip: at most one).
    // applied (may be nullptr): the value applied, 1 where the decode is not oriented; a clip's: one per frame.
    void op_jpeg_decode(const uint8_t* data, int64_t size, const whenet_surface_t& dst, int channel_order, int32_t* status, int entropy = -1,
                        int seg_bytes = 0, int64_t* stats = nullptr, int rule = -1, int progressive = -1, int orient = -1, int* applied = nullptr);
    void add_jpeg_progressive_counters(int64_t out[4]) const;      // decodes enqueued, scan-kernel launches, scans in them
    void add_jpeg_decode_counters(int64_t out[4]) const;      // decodes launched in form 0, in form 1
    void jpeg_decode_device(const whenet_jpeg_info_t& info, const uint8_t* d_entropy, int64_t nbytes, const whenet_surface_t& dst,
                            int channel_order, int32_t* d_status, hipStream_t stream);
    int frame_begin_jpeg(const uint8_t* data, int64_t size, int channel_order, int32_t* status, int rule = -1, int progressive = -1,
                         int orient = -1, int* applied = nullptr);
    // A CLIP of 1..16 JPEG streams (frame f: data[f], size[f] bytes), each with its own size, sampling, tables, DRI and entropy
    // form (the options are applied stream by stream): one plan (jpeg_dec_clip_host.h), ONE H2D of records | tables | entropy bytes,
    // one memset and every stage in one launch for all frames (launch_jpeg_decode_clip).  Refusals -- a frame count outside 1..16, a
    // NULL pointer or a size < 1, a stream the parser refuses (WHENET_EFORMAT), more sizes than letterbox_cache -- name the frame
    // and come before a slot is taken.
    // clip_begin_jpeg: the slot ends up as clip_begin (one size) or clip_begin_mixed (frames back to back) leaves it for the decoded
    // frames; status [frames][2] comes back through pinned memory with the ticket's collect call.
    // op_jpeg_decode_clip: the clip kernels alone, host to host, frame f into dst[f] at the caller's pitches between guard zones.
    // progressive = 1 (an argument only: clips do not read the option "jpeg_progressive"): a frame may be a SOF2 stream.  It is parsed
    // with its scan plan, refused by that parser's reason before a slot is taken, and laid out by jpeg_clip_plan_progressive; the clip
    // stays one H2D and one memset, launch L of the scan kernel covers level L of every progressive frame (always by level:
    // "jpeg_prog_levels" is the single-stream path's knob), one finish launch, then the clip's inverse DCT and colour launches
    // (launch_jpeg_decode_clip_progressive).  A baseline frame keeps the form it has in a baseline clip.  The progressive counters
    // add a decode per progressive frame, the clip's scan launches and the scans of its frames.
    int clip_begin_jpeg(const uint8_t* const* data, const int64_t* size, int nframes, int channel_order, int32_t* status, int rule = -1,
                        int progressive = 0, int orient = 0, int* applied = nullptr);
    void op_jpeg_decode_clip(const uint8_t* const* data, const int64_t* size, int nframes, const whenet_surface_t* dst, int channel_order,
                             int32_t* status, int entropy = -1, int seg_bytes = 0, int rule = -1, int progressive = 0, int orient = 0,
                             int* applied = nullptr);
    void add_jpeg_clip_counters(int64_t out[4]) const;      // clip decodes, their frames, their launches + memsets, their H2D copies
    void op_head_compact(const int32_t* valid, const int32_t* count, int frames, int slots_per_frame, int max_heads, int32_t* row,
                         int32_t* slot_of_row, int32_t* rows_used, int32_t* overflow);
    void op_dconv(const float* in, int n, int H, int W, int cin, const float* in2, int cin2, const float* kernel, const float* bias, int k,
                  int stride, int cout, int leaky, const float* skip, int f32_out, float* out);
    void op_dpool(const float* in, int n, int H, int W, int c, int stride, float* out);

    void* dev_alloc(size_t nbytes);
    void dev_free(void* p);
    void h2d(void* d, const void* s, size_t nbytes);
    void d2h(void* d, const void* s, size_t nbytes);

    std::string last_error;

  private:
    struct Slot {          // one in-flight submission of the pinned pipeline
        int capacity = 0, n = 0, ticket = -1;
        bool busy = false;
        StagedBuffer in, ypr, amax, logits;
        Event copied, done;
        Event source;                    // device ingest: recorded on the CALLER's stream, the copy stream waits for it (created on first use)
        StagedBuffer frame, plan;        // frame submissions: the frame and the crop plans travel instead of the crops
        DeviceBuffer yuv;                // YUV ingest: the planes on the device (frame.h stages them, frame.d gets the converted frame)
        int frame_ticket = -1;           // resident frame: the ticket whose frame is held here and still waits for its heads
        int fh = 0, fw = 0, swap_rb = 0; //   (tickets are never reused, so a stale value matches nothing)
        StagedBuffer det;                // frame_detect_heads: count | boxes | scores | classes | rects | valid over det_cap rows
        int det_cap = -1;                //   (DetRows); >= 0 marks a submission that collect_detect, not collect, returns
        int clip_f = 0;                  // clip_begin: frames held in `frame` (0: a single frame); with clip_detect_heads `det` is a
        int clip_cap = -1, clip_heads = 0;   // ClipRows(clip_f, clip_cap, clip_heads); clip_cap >= 0: collect_clip returns it
        bool clip_mixed = false;         // clip_begin_mixed: frame f is clip_fh[f] x clip_fw[f] and starts clip_off[f] bytes into `frame`
        int clip_fh[MIXED_MAX_FRAMES] = {}, clip_fw[MIXED_MAX_FRAMES] = {};
        size_t clip_off[MIXED_MAX_FRAMES + 1] = {};      // (the last entry: the bytes of the whole clip)
        // frame_annotate: what the ticket's heads left on the device (ANN_NONE: nothing to annotate -- crops only, no frame uploaded,
        // or the heads are not enqueued yet), the frames annotated so far, the table of the plan kernel, the event a caller's stream
        // waits for, and the host destinations that the collect call fills from their staging
        enum { ANN_NONE = 0, ANN_PLANS = 1, ANN_DET = 2, ANN_CLIP = 3 };
        int ann_kind = ANN_NONE;
        unsigned ann_mask = 0;
        DeviceBuffer ann_table;
        DeviceBuffer ann_labels;         // display full: the label records, [frames][head slots][3 lines][4 words]
        Event ann_done;
        struct AnnHost {
            whenet_surface_t dst;
            int frame_index, fh, fw;
        };
        std::vector<AnnHost> ann_host;
        StagedBuffer ann_stage[MIXED_MAX_FRAMES];
        // frame_annotate_jpeg, per frame index: the engine's tight I420 JFIF surface, the stream's landing buffer in device memory
        // (capacity rounded up to 16 bytes, the int64 length behind it) and its pinned twin, which the flush kernel fills with
        // min(length, capacity) bytes and the length; and the callers' destinations that the collect call fills from the pinned twins
        struct JpegStage {
            DeviceBuffer surface, stream;
            PinnedBuffer host;
        };
        JpegStage jpg_stage[MIXED_MAX_FRAMES];
        struct JpegHost {
            uint8_t* out;
            int64_t cap, staged_cap;
            int64_t* size;
            int32_t* status;
            int frame_index;
        };
        std::vector<JpegHost> jpg_host;
        // frame_begin_jpeg: the decoder's work buffers (tables | compressed bytes | starts | coefficients | planes | status), the
        // pinned landing of the two status words, and the caller's destination that the collect call fills (nullptr: none pending)
        DeviceBuffer jpg_dec;
        PinnedBuffer jpg_dec_status;
        int32_t* jpg_dec_out = nullptr;
        int jpg_dec_pairs = 1;           // the status pairs jpg_dec_out takes: 1, or the frames of clip_begin_jpeg
        Results host() const { return {ypr.h.as<float>(), amax.h.as<int32_t>(), logits.h.as<float>()}; }
        Results dev() const { return {ypr.d.as<float>(), amax.d.as<int32_t>(), logits.d.as<float>()}; }
    };

    template <typename T> T* upload(const std::vector<T>& v);
    void* upload_bytes(const void* p, size_t nbytes);
    DevPw upload_pw(const HostPw& h);
    // the arguments of a 1x1 conv with w's weights over M = n * HW rows: what every pointwise launch sets
    PwArgs pw_args(const DevPw& w, const void* a, void* out, int M, int HW, int act) const;
    bool split_ = false;        // the handle was created as WHENET_F32S
    bool split_pw_ = true;      // option "split_pw"
    bool pw_staged_ = true;     // option "pw_staged": split-K GEMMs fetch their activation rows coalesced, through LDS
    void ensure_capacity(int n);
    void release_arena();
    void drop_graphs();
    size_t esz() const { return dtype_ == WHENET_F16 ? 2 : 4; }

    struct View {          // the activation arena as seen by a sub-batch starting at some crop
        void *x0, *x1, *e, *d, *hc;
        float *partial, *gate;
        unsigned* hcount;
        uint8_t* in_u8;
        Results out;
    };
    View view(int crop_off) const;
    // enqueue the kernels of one forward on `s` (eager); rec != nullptr -> event pairs
    void enqueue_forward(const View& v, const uint8_t* d_in, int n, Results out, hipStream_t s, LaunchRecorder* rec,
                         const float* d_in_f32 = nullptr);
    // fold: 0 = the block as it stands; 1 = block 1 without its project (its depthwise output goes to `out`);
    //       2 = block 2 fed by that output, block 1's project folded into its expand weights (fold12_active())
    // in_blocked / out_blocked: the block's input / output tensor is in the blocked layout (act_blocked())
    void enqueue_block(const DevBlock& b, const View& v, const void* in, void* out, int n, hipStream_t s,
                       LaunchRecorder* rec, int fold = 0, bool dw_done = false, bool in_blocked = false, bool out_blocked = false);
    struct BlockSchedule;
    // its parts: the fused expand + depthwise stage (or the whole block: mb7.hip), the unfused pair, the rest of the SEBlock (returns
    // what the project needs to compute the gate itself, if it does), the project
    void enqueue_front(const DevBlock& b, const BlockSchedule& bs, const View& v, const void* in, void* out, int n, hipStream_t s,
                       LaunchRecorder* rec, int fold, bool in_blocked);
    void enqueue_expand_dw(const DevBlock& b, const View& v, const void* in, void* dw_out, int n, hipStream_t s, LaunchRecorder* rec,
                           bool dw_done);
    SeFuse enqueue_se(const DevBlock& b, const BlockSchedule& bs, const View& v, int n, hipStream_t s, LaunchRecorder* rec, int fold);
    void enqueue_project(const DevBlock& b, const SeFuse& sef, bool se_fused, const View& v, const void* in, void* out, int n,
                         hipStream_t s, LaunchRecorder* rec, bool in_blocked, bool out_blocked);
    template <typename A> void fill_front_common(A& a, const DevBlock& b, const View& v, const void* in, int n) const;
    // the head conv's arguments, fused with the pooling (head7.hip) and alone (pw.hip), for the forward and for op_head
    Head7Args head7_args(const void* x, float* feat, int n) const;
    PwArgs head_pw_args(const void* x, void* out, int n) const { return pw_args(head_, x, out, n * 49, 49, ACT_SWISH); }
    // blocks first..last (1-based) as the forward pass runs them; returns the buffer (x0 / x1 of `v`) holding the result
    void* enqueue_blocks(int first, int last, const View& v, void* cur, int n, hipStream_t s, LaunchRecorder* rec,
                         bool b1_dw_done = false);
    bool stem_fuse_active() const;
    bool fold12_active() const;
    bool head_fused() const;           // the head conv pools its own output (head7.hip)
    // The Dense + softmax + decode stage: four workgroups per crop (whenet_heads_split_kernel, partial vectors in v.partial, tickets
    // in v.hcount) or one (whenet_heads_kernel).  The ONE choice and the ONE launch site of the forward and of op_head.
    bool heads_split_active() const;
    void launch_heads_stage(const HeadsArgs& h, const View& v, hipStream_t s);
    // Layout of the OUTPUT of block `index` (1-based) in a whole forward: true = 16-channel blocks [crop][C/16][HW][16]
    // (DESIGN.md section 2), false = NHWC.  A function of the layer and the options only, never of the batch.
    bool act_blocked(int index) const;
    bool front_static(int index) const;      // block `index` asks front.hip for its static-shape form (option "front_static")
    bool pw_static(int index) const;         // block `index` asks pw.hip for the static-shape form of its project GEMM (option "pw_static")
    bool front2_static(int index) const;     // block `index` asks front2.hip for its static-plan form (option "front2_static")
    int act_layout_ = 1;               // option "act_layout": 0 = NHWC everywhere, 1 = the per-layer table, 2 = blocked wherever supported
    struct BlockSchedule {     // which kernels a block runs under the current options
        bool fused = false, use_f2 = false, use_f2s = false, use_f7 = false, se_in_front = false, se_fused = false, se_mfma = false;
        bool use_mb7 = false;  // the whole block is one launch (mb7.hip): no front / squeeze-excite / project launches
        int se_ntiles = 1, se_chunks = 1;
    };
    // n = crops of the chain the block runs in (0: not batch-specific, e.g. the launch count of get_info)
    BlockSchedule block_schedule(const DevBlock& b, int n = 0) const;
    int se_fuse_tiny_ = 0;             // option "se_fuse_tiny"
    int f2s_mask_ = -1;                // option "f2s_mask" (probes)
    bool single_stage_call_ = false;   // op_block / op_block_range: the schedule must not depend on the test's batch size
    bool range_call_ = false;          // op_block_range: the tensors BETWEEN its blocks take the layout the forward gives them (act_blocked);
                                       // its input and its output are NHWC, as the caller passes and reads them
    int lanes_for(int n, int want) const;     // chains a forward of n crops runs as (want = 0: option "lanes")
    // body(i, off, cnt, st): chain i of `lanes` takes crops [off, off + cnt) on stream st (chain 0: s itself), forked from and joined
    // back into s with events
    template <typename F> void for_each_lane(int n, int lanes, hipStream_t s, F&& body);
    void enqueue_lanes(const uint8_t* d_in, int n, Results out, hipStream_t s, int want = 0);
    void run_forward(const uint8_t* d_in, int n, Results out, hipStream_t s, int want = 0);
    void poison_arena(int n, hipStream_t s);        // option "poison": NaN bit patterns in every activation buffer of n crops
    void ensure_slot(Slot& s, int n);
    hipStream_t lane_stream(int i);     // created on first use
    using GraphKey = std::tuple<int, int, const void*, void*, void*, void*>;   // n, lane offset (-L: whole batch as L chains), buffers
    template <typename F>
    hipGraphExec_t cached_graph(const GraphKey& key, hipStream_t s, F&& fn);
    void sync_streams(hipStream_t s);
    hipStream_t copy_stream();          // created on first use
    void ensure_slot_frame(Slot& s, size_t frame_bytes, int k);
    Slot* free_slot();
    // the held slot of a frame_begin (HOLDS_FRAME) or clip_begin (HOLDS_CLIP) ticket that has no heads yet
    enum { HOLDS_FRAME = 0, HOLDS_CLIP = 1, HOLDS_EITHER = 2 };
    Slot& resident_slot(int ticket, const char* what, int holds = HOLDS_FRAME);
    // frame on the device -> canvas in the caller's host arrays (either may be nullptr), through pinned memory with one wait
    void run_letterbox(const uint8_t* d_frame, int fh, int fw, int swap_rb, int out_h, int out_w, uint8_t* canvas_u8,
                       float* image_f32, int frames = 1);
    int finish_submission(Slot& s, int n);      // record `done`, mark the slot busy, hand out its ticket
    // run_letterbox's launches alone: the device canvas (uint8, float32) of those asked for, valid until the next letterbox
    // frames > 1: d_frame is a clip [frames][fh][fw][3], the canvases are [frames][out_h][out_w][3]
    std::pair<uint8_t*, float*> enqueue_letterbox(const uint8_t* d_frame, int fh, int fw, int swap_rb, int out_h, int out_w, bool want_u8,
                                                  bool want_f32, int frames = 1);
    // the same for `frames` frames of their own sizes, frame f at d_frames + off[f] (off[frames]: the bytes of them all)
    std::pair<uint8_t*, float*> enqueue_letterbox_mixed(const uint8_t* d_frames, int frames, const int* fh, const int* fw, const size_t* off,
                                                        int swap_rb, int out_h, int out_w, bool want_u8, bool want_f32);
    void ensure_letterbox_outputs(size_t mid_bytes, size_t nout, bool want_u8, bool want_f32);
    // the planes of the frames, staged tight and back to back in h_stage -> d_planes (one copy) -> d_bgr (one launch) on `s`; frame
    // f's output starts off[f] bytes into d_bgr.  The three buffers are large enough (yuv_layout).
    void enqueue_yuv_ingest(const whenet_yuv_frame_t* frames, int nframes, uint8_t* h_stage, uint8_t* d_planes, uint8_t* d_bgr,
                            const size_t* off, hipStream_t s);
    // device ingest: the argument checks of the packed and the plane form (engine.h ORDER / CHECKS), the launches on the copy
    // stream between the two event hand-overs, and the kernels alone
    void check_device_plane(const std::string& who, const uint8_t* p, int rows, int pitch, int row_bytes) const;
    void check_device_frames(const char* what, const uint8_t* const* d_frames, const int* pitch, int nframes, const int* fh, const int* fw) const;
    void check_device_yuv_frames(const char* what, const whenet_yuv_frame_t* frames, int nframes) const;
    void check_device_yuvx_frames(const char* what, const whenet_yuvx_frame_t* frames, int nframes) const;
    // enqueue_yuv_ingest for whenet_yuvx_frame_t (one launch of yuvx.hip's upload form)
    void enqueue_yuvx_ingest(const whenet_yuvx_frame_t* frames, int nframes, uint8_t* h_stage, uint8_t* d_planes, uint8_t* d_bgr,
                             const size_t* off, hipStream_t s);
    void ingest_after_caller(Slot& slot, hipStream_t caller);      // caller's stream -> slot.source -> copy stream
    void ingest_done(Slot& slot, hipStream_t caller);              // copy stream -> slot.copied -> caller's stream
    // the argument checks of frame_annotate that concern the ticket; returns its slot, the head slots per frame and the frame's geometry
    Slot& annotate_target(int ticket, int frame_index, int& k, int& fh, int& fw, size_t& frame_off);
    void finish_annotations(Slot& slot);                            // collect calls, behind their wait: staging -> the callers' host surfaces
    void check_surface(const char* what, const whenet_surface_t& dst, int fh, int fw) const;      // overlay_check's surface part + memory kind
    void letterbox_results_to_host(size_t nout, uint8_t* d_u8, float* d_f32, uint8_t* canvas_u8, float* image_f32);
    // every frame's plan_layout, F <= letterbox_cache: what a mixed clip needs before anything is enqueued
    void check_mixed_geometry(const char* what, int frames, const int* fh, const int* fw, int out_h, int out_w) const;
    // the argument set-up of yolo_eval (scratch carved and grown, host maps uploaded) and its launches on stream_; no wait, no copy
    // back: the selected boxes stay in yolo_scratch_ (out_boxes / out_scores / out_count of the returned arguments)
    YoloArgs enqueue_yolo_eval(const float* const* feats, bool on_device, const int* grid_h, const int* grid_w, int num_layers,
                               const float* anchors, int num_anchors, int num_classes, float image_h, float image_w, float score_threshold,
                               float iou_threshold, int max_boxes, bool want_all_scores, int images = 1,
                               const float* image_shapes = nullptr /* [images][2]: every image its own shape */);
    // yolo_eval on maps that are in host memory (uploaded first) or already on the device
    int yolo_eval_maps(const float* const* feats, bool on_device, const int* grid_h, const int* grid_w, int num_layers, const float* anchors,
                       int num_anchors, int num_classes, float image_h, float image_w, float score_threshold, float iou_threshold,
                       int max_boxes, float* boxes, float* scores, int32_t* classes, int32_t* index, float* all_boxes, float* all_scores);
    void yolo_batch_to_host(const YoloArgs& a, float* boxes, float* scores, int32_t* classes, int32_t* index, int32_t* counts);
    void require_detector() const;
    DetPlan& detector_plan(int n, int H, int W);
    void enqueue_detector(DetPlan& p, hipStream_t s);
    int detect_device(const uint8_t* d_frame, int fh, int fw, int swap_rb, int out_h, int out_w, const float* anchors, int num_anchors,
                      float score_threshold, float iou_threshold, int max_boxes, float* boxes, float* scores, int32_t* classes);

    // the JPEG encoder's device-resident tables of (h, w, quality), kept (at most 8 sets: a full cache waits for stream_ and empties)
    struct JpegTableSet {
        int h, w, quality, sampling;
        DeviceBuffer d;
    };
    std::vector<JpegTableSet> jpeg_tables_;
    DeviceBuffer jpeg_scratch_;
    Event jpeg_source_, jpeg_done_;
    const JpegTables* jpeg_device_tables(int h, int w, int quality, int sampling);
    DeviceBuffer jpeg_dec_scratch_;      // jpeg_decode_device's work buffers, and the decode tables of its last stream (kept while
    DeviceBuffer jpeg_dec_tables_d_;     // the next stream's are the same: an MJPG stream repeats its tables)
    std::vector<JpegDecTables> jpeg_dec_tables_h_;
    int jpeg_entropy_ = 2, jpeg_seg_bytes_ = JPEG_SEG_DEFAULT_BYTES;      // options "jpeg_entropy", "jpeg_seg_bytes"
    int jpeg_rule_ = JPEG_RULE_OWN;                                       // option "jpeg_rule"
    int jpeg_progressive_ = 0, jpeg_prog_levels_ = 1;                     // options "jpeg_progressive", "jpeg_prog_levels"
    int jpeg_layouts_ = 0;                                                // option "jpeg_layouts" (the header's JPEG DECODER, LAYOUTS)
    int jpeg_accept_of(const char* what, int accept) const;               // the accept bits of a call: its argument, or (-1) the two options
    int jpeg_orient_ = 0;                                                 // option "jpeg_orient"
    // the orientation a single-stream call applies: the stream's tag where `orient` is 1, or -1 with the option set; else 1
    int jpeg_orient_of(const char* what, int orient, const uint8_t* data, int64_t size) const;
    int64_t jpeg_prog_counts_[3] = {0, 0, 0};                             // decodes enqueued, scan-kernel launches, scans in them
    // the rule of a call: its argument, or the option where that is -1; anything else is WHENET_EINVAL
    int jpeg_rule_of(const char* what, int rule) const;
    int jpeg_seg_lanes_ = 0;                                             // option "jpeg_seg_lanes" (a measurement knob; 0: the default)
    int64_t jpeg_dec_launched_[2] = {0, 0};                              // decodes launched in form 0, form 1
    int64_t jpeg_clip_counts_[4] = {0, 0, 0, 0};                         // add_jpeg_clip_counters
    struct JpegClipJob;      // the parsed headers, geometries and the plan of a clip (engine_post.cpp)
    void jpeg_clip_prepare(const char* what, const uint8_t* const* data, const int64_t* size, int nframes, int entropy, int seg_bytes, int rule,
                           JpegClipJob& job, int progressive = 0, int orient = 0) const;
    // records | tables | entropy bytes into `stage` (plan.upload_bytes), the records for a work buffer at d_base; recs: the same records
    // (a progressive frame: its scan plan's share, a record as jpeg_dec_args makes it of its regions, and its progressive record in precs)
    void jpeg_clip_stage(const JpegClipJob& job, const uint8_t* const* data, uint8_t* stage, void* d_base, const whenet_surface_t* dst,
                         int channel_order, int32_t* d_status, JpegDecArgs* recs, JpegProgArgs* precs) const;
    // the clip's launches behind its upload, and its counters
    void jpeg_clip_launch(const JpegClipJob& job, const JpegDecArgs* recs, const JpegProgArgs* precs, char* d_base, hipStream_t stream);
    // the layout of a decode's work buffers in the form the options (or `entropy` >= 0, `seg_bytes` > 0) give this stream
    JpegDecScratch jpeg_dec_layout(const JpegDecGeom& g, size_t data_bytes, int64_t nbytes, int entropy = -1, int seg_bytes = 0) const;
    // one stream through the single-stream kernels (op_jpeg_decode, frame_begin_jpeg): its layouts; stage + one H2D + launches + counters
    struct JpegStreamJob;
    int64_t jpeg_stream_launch(const JpegStreamJob& job, const uint8_t* data, uint8_t* stage, void* d_work, const whenet_surface_t& dst,
                               int channel_order, int32_t* d_status, int rule, hipStream_t stream, int orient = 1);
    // the slot of frame_begin_jpeg / clip_begin_jpeg: its buffers, destination surfaces and status words; its state and ticket
    // (info: the headers with the sides of the frames as they land -- jpeg_orient_info of an oriented decode)
    Slot& jpeg_slot_begin(const whenet_jpeg_info_t* info, int nframes, size_t upload_bytes, size_t work_bytes, size_t* off, whenet_surface_t* dst,
                          int32_t*& d_status);
    int jpeg_slot_finish(Slot& slot, const whenet_jpeg_info_t* info, const size_t* off, int clip_frames, bool one_size, int channel_order,
                         int32_t* status);

    void open_device(int device_id);
    void require_model() const;
    bool has_model_ = false;
    int device_ = 0, dtype_ = WHENET_F32, num_cus_ = 256;
    bool use_graph_ = true;
    int pw_impl_ = 0;
    int repeat_ = 1;
    bool split_heads_ = true;   // option "split_heads": GAP + Dense over 4 workgroups per crop, the last one decodes
    bool fuse_front_ = true;    // option "fuse_front": expand + depthwise as one kernel (front.hip / front2.hip)
    int se_fuse_ = 1;           // option "se_fuse": the project GEMM computes the SE gate of its own crops in its prologue (no
                                // squeeze-excite launch): 0 = never, 1 = on the blocks where that is faster, 2 = every fused-front block
    int front_impl_ = 1;        // option "front_impl": 0 = front.hip everywhere, 1 = per layer (f16: front2.hip where it is
                                // the faster kernel), 2 = front2.hip everywhere (f16)
    bool poison_ = false;       // debug option "poison": NaN-fill the activation arena before every forward (and forward_host_f32's
                                // input staging buffer before its copy: the copy must cover every byte the forward reads)
    bool head_fuse_ = true;     // option "head_fuse": the head conv pools its own output (head7.hip, f16 and f32); 0 = round 3's two stages
    bool front7_ = true;        // option "front7": blocks 13-16 of an f16 handle run front7.hip (a group of crops per workgroup)
                                // when front_impl = 1; 0 = the per-layer choice of round 3 (front.hip there)
    bool mb7_ = false;          // option "mb7": blocks 13-16 of an f16 handle run as ONE launch each (mb7.hip, round 6: one workgroup per crop,
                                // every intermediate tensor in LDS).  Measured (profiles/r06/mb7_*): 29 us per launch whatever the batch up to 256
                                // crops against 3 x 8 us at one crop and 67 us at 256 -- +3 % at batch 512, +-1 % at 64 x 3 in flight, -4 % one
                                // forward at a time, +60 us at batch 1.  Not the default: the schedule must not depend on the batch.
    int xcd_map_ = 7;           // option "xcd_map" (round 6), bit mask: the channel chunks that share an input are dealt to ONE XCD in
                                // 1 = front.hip / front2.hip, 2 = front7.hip, 4 = head7.hip (device_math.h xcd_unit).  Same bits either way.
                                // Measured on one box against the 3-D grid order of rounds 2-5 (profiles/r06/ab_xcd_map_*.txt): +0.8 % at
                                // 64 crops x 3 in flight, at batch 512 and for f32s; the 14 x 14 front kernels alone get slower with it
    bool xcd_always_ = false;   // option "concurrent" (set by the handle when it owns several engines): other forwards share the chip
    bool xcd_grouped(int bit, int n) const {      // the grouped placement pays when the chip is full: several forwards in flight, or a
        return (xcd_map_ & bit) != 0 && (xcd_always_ || n >= 128);     // launch of >= 128 crops; one small forward alone loses 1 % with it
    }
    bool stem_fuse_ = true;     // option "stem_fuse": uint8 input -- the stem conv is computed inside block 1's depthwise kernel (stemdw.hip)
    bool front_static_ = true;  // option "front_static": front.hip with the layer's geometry as compile-time constants, per layer
    bool pw_static_ = true;     // option "pw_static": the project GEMMs with the layer's shape as compile-time constants, per layer
    bool front2_static_ = true; // option "front2_static": front2.hip with the tile geometry as compile-time constants, per layer
    bool fold12_ = true;        // option "fold12": block 1's project folded into block 2's expand (f16 + front2.hip on block 2)
    int lanes_ = 2;             // concurrent sub-batch chains per forward (option "lanes"; round 3: 2 -- with the faster
                                // front kernels a third chain only adds contention: 100.1 k vs 97.2 k crops/s at batch 64,
                                // equal from 256 crops up and for f32)
    bool lane_graphs_ = false;  // one graph per lane on its own stream instead of one forked graph (option "lane_graphs")
    int min_lane_crops_ = 16;   // do not split below this many crops per chain
    int host_lanes_ = 2;        // chains of a BLOCKING host forward (it has the GPU to itself whatever "inflight" says)
    // (declaration order is destruction order reversed: every buffer and event below goes before these streams)
    Stream stream_, copy_stream_;
    std::vector<Stream> lane_streams_;
    std::vector<Event> join_ev_;
    Event fork_ev_;
    hipDeviceProp_t prop_{};
    int64_t params_backbone_ = 0, params_heads_ = 0;
    int n_tensors_ = 0;

    // weights
    std::vector<DeviceBuffer> weight_allocs_;
    float *d_lut_ = nullptr, *d_stem_w_ = nullptr, *d_stem_b_ = nullptr;
    StemDwTable* d_stemdw_tab_ = nullptr;   // stemdw.hip's packed LUT + stem weight fragments
    std::vector<DevBlock> blocks_;
    DevPw head_;
    DevPw fold12_pw_;           // block 1 project x block 2 expand, 32 -> 96 (snapshot.cpp)
    float* d_fold12_w32_ = nullptr;   // its f32 fragment image (front2.hip rounds AFTER the per-crop gate)
    float *d_dense_w_ = nullptr, *d_dense_b_ = nullptr;

    // activation arena (grown to the largest n seen)
    int cap_ = 0;
    size_t arena_bytes_ = 0;
    // ONE table of its buffers, in allocation order: sizes (ensure_capacity), per-crop offsets (view) and the NaN fill (poison_arena:
    // the first A_POISONED entries) all come from it.  A_HCOUNT: per-crop tickets of the split heads kernel (zero between launches)
    enum { A_X0, A_X1, A_E, A_D, A_HC, A_PARTIAL, A_GATE, A_HCOUNT, A_IN_U8, A_YPR, A_AMAX, A_LOGITS, A_COUNT, A_POISONED = A_HCOUNT };
    struct ArenaBuf {
        DeviceBuffer buf;
        size_t per_crop = 0;       // bytes
    };
    ArenaBuf arena_[A_COUNT];
    DeviceBuffer in_f32_;           // normalised float32 input of forward_host_f32 (grown on demand)
    size_t partial_per_crop_ = 0;
    DeviceBuffer yolo_scratch_;     // device scratch of yolo_eval, grown on demand
    std::vector<int> yolo_counts_;               // host staging of the per-class detection counts
    // letterbox scratch, grown on demand: the horizontal pass's output, the /255 table, the outputs and their pinned landing
    // zones, the frame of op_letterbox
    std::vector<int32_t> lb_tables_host_;
    StagedBuffer lb_u8_, lb_f32_;
    DeviceBuffer lb_mid_, lb_lut_, lb_frame_;
    // The letterbox geometry cache (option "letterbox_cache", 1..32 entries, default 16), keyed by (ih, iw, oh, ow): several
    // cameras on one handle, or the frames of a mixed clip, each keep their resample tables on the device.  An entry owns its
    // plan, its device table block, the pinned block the tables are staged through and an event recorded behind the H2D copy
    // out of that block.  A hit enqueues nothing and waits for nothing.  A miss builds the tables on the host, takes the least
    // recently used entry that no clip being enqueued has pinned, waits -- the host, and only if the copy is not done yet -- for
    // THAT entry's previous copy event before its pinned block is overwritten, and enqueues the new copy on stream_: the launches
    // that read the evicted tables are ahead of it in stream order.  stream_ itself is never waited for.  (A block that must
    // GROW is reallocated, as every grown buffer of the engine: blocks are rounded up so that this ends after the first frames.)
    struct LbEntry {
        LetterboxPlan plan{};
        bool valid = false, staged = false;
        StagedBuffer tables;
        Event copied;
        uint64_t last_use = 0;
        int pins = 0;
    };
    struct LbPins {            // the entries a clip holds while its launches are enqueued
        std::vector<LbEntry*> held;
        ~LbPins() {
            for (LbEntry* e : held) --e->pins;
        }
    };
    std::deque<LbEntry> lb_cache_;      // (a deque: entries never move, clips hold pointers to them)
    int lb_cache_cap_ = 16;
    uint64_t lb_clock_ = 0;
    int32_t lb_hits_ = 0, lb_misses_ = 0, lb_host_waits_ = 0;
    LbEntry& letterbox_entry(int fh, int fw, int out_h, int out_w, LbPins* pins = nullptr);

    std::map<GraphKey, hipGraphExec_t> graphs_;

    Slot slots_[WHENET_MAX_INFLIGHT];
    Slot host_slot_;                   // pinned staging of small BLOCKING host forwards (forward_host, n <= host_pinned_max_)
    // pinned landing zone of the RESULTS of larger blocking host forwards: three asynchronous D2H copies and one wait instead of three
    // synchronous copies into the caller's pageable arrays (round 6)
    PinnedBuffer hout_ypr_, hout_amax_, hout_logits_;
    int hout_cap_ = 0;
    Results hout() const { return {hout_ypr_.as<float>(), hout_amax_.as<int32_t>(), hout_logits_.as<float>()}; }
    void ensure_host_out(int n);
    int host_pinned_max_ = 8;      // measured round 5: pinned wins up to 8 crops (B=1 f32 420 vs 445 us), loses at 16-32
    int next_ticket_ = 0;
    int det_dtype_ = WHENET_F16;       // option "detector_dtype": the storage type detector_load packs for, and of op_dconv / op_dpool
    std::shared_ptr<Detector> det_;    // (declared last: its buffers and graphs go first)
    std::map<std::tuple<int, int, int>, std::shared_ptr<DetPlan>> det_plans_;      // by (n, H, W)
};

}  // namespace whenet
