// Definitions shared by the engine's translation units (engine.cpp: construction, options, arena, launch schedule,
// graphs, forward paths, profiling; engine_post.cpp: frame pre-processing and detector post-processing entry points;
// engine_ops.cpp: single-stage entry points for the tests).  Not part of any interface.
#pragma once

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "engine.h"

namespace whenet {
namespace detail {

constexpr size_t X_ELEMS = size_t(112) * 112 * 32;    // largest block input/output per crop (stem out)
constexpr size_t E_ELEMS = size_t(112) * 112 * 96;    // largest expanded tensor per crop (b2 expand)
constexpr size_t D_ELEMS = size_t(56) * 56 * 144;     // largest depthwise output per crop (b3 dw)
constexpr size_t HC_ELEMS = size_t(49) * FEAT;        // head conv output per crop
constexpr size_t GATE_ELEMS = 1152;                   // widest squeeze-excite gate per crop (blocks 13-16)
constexpr size_t IN_BYTES = size_t(IMG) * IMG * 3;
constexpr int MAX_GRAPHS = 16;

struct DeviceGuard {
    explicit DeviceGuard(int dev) { WHENET_HIP_CHECK(hipSetDevice(dev)); }
};

struct TempBufs {     // hipMalloc'd scratch of the single-stage entry points
    std::vector<DeviceBuffer> bufs;
    void* get(size_t nbytes) {
        bufs.emplace_back();
        bufs.back().reset(nbytes);
        return bufs.back().as<void>();
    }
};

// The header of a JPEG stream into `info`, for the engine and for the host statements of capi.cpp alike.  plan: nullptr (baseline
// streams only), or where the scan plan goes (the parser that accepts progressive streams too).  WHENET_EINVAL, or WHENET_EFORMAT
// with the parser's reason.
// layouts, sof2: the parsers' arguments (the header's JPEG DECODER, LAYOUTS): with layouts a plan is needed whether or not SOF2
// frames are accepted (a sequential frame of several scans has one), and sof2 says whether they are.
inline void jpeg_parse_or_refuse(const char* what, const uint8_t* data, int64_t size, whenet_jpeg_info_t& info, JpegProgPlan* plan = nullptr,
                                 bool layouts = false, bool sof2 = true) {
    WHENET_REQUIRE(data != nullptr && size >= 1, WHENET_EINVAL, std::string(what) + ": NULL argument or size < 1");
    const char* bad = plan != nullptr ? jpeg_prog_parse(data, size, info, *plan, layouts, sof2) : jpeg_parse(data, size, info, layouts);
    WHENET_REQUIRE(bad == nullptr, WHENET_EFORMAT, std::string(what) + ": " + (bad ? bad : ""));
}

// The `progressive` argument of the engine's JPEG calls is a set of accept bits (include/whenet_hip_jpeg_accept.h: WHENET_JPEG_ACCEPT_*): 0 and 1
// are what they were, 2 adds the layouts; -1 stands for the handle's options "jpeg_progressive" and "jpeg_layouts".
constexpr int JPEG_ACCEPT_PROGRESSIVE = 1, JPEG_ACCEPT_LAYOUTS = 2;
inline bool jpeg_accept_ok(int accept) { return accept >= 0 && accept <= (JPEG_ACCEPT_PROGRESSIVE | JPEG_ACCEPT_LAYOUTS); }
// a stream parsed with these bits (jpeg_accept_ok) into info and, where either bit is set, its scan plan
inline void jpeg_parse_accept_or_refuse(const char* what, const uint8_t* data, int64_t size, whenet_jpeg_info_t& info, JpegProgPlan& plan, int accept) {
    jpeg_parse_or_refuse(what, data, size, info, accept != 0 ? &plan : nullptr, (accept & JPEG_ACCEPT_LAYOUTS) != 0,
                         (accept & JPEG_ACCEPT_PROGRESSIVE) != 0);
}

struct FlagGuard {    // sets a flag for a scope
    bool& flag;
    explicit FlagGuard(bool& f) : flag(f) { flag = true; }
    ~FlagGuard() { flag = false; }
};

// The three result copies of n crops: device to host on a stream, and out of a pinned landing buffer into the caller's arrays
// (those of them that are not nullptr).
inline void copy_results_async(const Results& dst, const Results& src, int n, hipStream_t s, bool want_amax = true,
                               bool want_logits = true) {
    const size_t N = size_t(n);
    WHENET_HIP_CHECK(hipMemcpyAsync(dst.ypr, src.ypr, N * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
    if (want_amax) WHENET_HIP_CHECK(hipMemcpyAsync(dst.amax, src.amax, N * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (want_logits) WHENET_HIP_CHECK(hipMemcpyAsync(dst.logits, src.logits, N * N_LOGITS * sizeof(float), hipMemcpyDeviceToHost, s));
}
inline void copy_results_host(const Results& dst, const Results& src, int n) {
    const size_t N = size_t(n);
    if (dst.ypr) std::memcpy(dst.ypr, src.ypr, N * 3 * sizeof(float));
    if (dst.amax) std::memcpy(dst.amax, src.amax, N * 3 * sizeof(int32_t));
    if (dst.logits) std::memcpy(dst.logits, src.logits, N * N_LOGITS * sizeof(float));
}

// The detection block of a frame_detect_heads slot over a capacity of K rows, one allocation so that ONE copy brings it back:
// count (int32, padded to 16 bytes) | boxes [K][4] f32 | scores [K] f32 | classes [K] i32 | rects [K][4] i32 | valid [K] i32
struct DetRows {
    size_t K;
    explicit DetRows(int k) : K(size_t(k)) {}
    size_t bytes() const { return 16 + K * 44; }
    int32_t* count(void* base) const { return static_cast<int32_t*>(base); }
    float* boxes(void* base) const { return reinterpret_cast<float*>(static_cast<char*>(base) + 16); }
    float* scores(void* base) const { return boxes(base) + K * 4; }
    int32_t* classes(void* base) const { return reinterpret_cast<int32_t*>(scores(base) + K); }
    int32_t* rects(void* base) const { return classes(base) + K; }
    int32_t* valid(void* base) const { return rects(base) + K * 4; }
};

// The detection block of a clip_detect_heads slot: F frames x K slots (S = F * K <= 1024) and M forward rows, one allocation so
// that ONE copy brings it back:
// rows_used, overflow (int32, padded to 16 bytes) | count [16] i32 | boxes [S][4] f32 | scores [S] f32 | classes [S] i32 |
// rects [S][4] i32 | valid [S] i32 | row [S] i32 | slot_of_row [M] i32
struct ClipRows {
    size_t S, M;
    ClipRows(int frames, int k, int max_heads) : S(size_t(frames) * size_t(k)), M(size_t(max_heads)) {}
    size_t bytes() const { return 80 + S * 48 + M * 4; }
    int32_t* rows_used(void* base) const { return static_cast<int32_t*>(base); }
    int32_t* overflow(void* base) const { return static_cast<int32_t*>(base) + 1; }
    int32_t* count(void* base) const { return static_cast<int32_t*>(base) + 4; }
    float* boxes(void* base) const { return reinterpret_cast<float*>(static_cast<char*>(base) + 80); }
    float* scores(void* base) const { return boxes(base) + S * 4; }
    int32_t* classes(void* base) const { return reinterpret_cast<int32_t*>(scores(base) + S); }
    int32_t* rects(void* base) const { return classes(base) + S; }
    int32_t* valid(void* base) const { return rects(base) + S * 4; }
    int32_t* row(void* base) const { return valid(base) + S; }
    int32_t* slot_of_row(void* base) const { return row(base) + S; }
};

inline void copy_name(char* dst, size_t cap, const std::string& s) {
    std::memset(dst, 0, cap);
    std::memcpy(dst, s.data(), std::min(cap - 1, s.size()));
}

}  // namespace detail
}  // namespace whenet
