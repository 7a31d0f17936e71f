// extern "C" surface of libwhenet_hip.so (include/whenet_hip.h).  Every entry point catches
// everything: no exception crosses the ABI.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <mutex>
#include <new>
#include <exception>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "engine.h"
#include "engine_internal.h"
#include "../../include/whenet_hip_jpeg_accept.h"

// A handle = one primary engine plus, with option "inflight" > 1, replica engines (own streams,
// activation arena, hipGraphs and a copy of the 8.6-17 MB device weights).  A forward is a chain of
// 51 dependent launches -- about half of a batch-64 forward is launch latency -- so independent
// forwards are spread round-robin over the engines and overlap on the GPU.
constexpr int MAX_INFLIGHT_ENGINES = 4;
struct whenet_ctx {
    whenet::Engine* engine = nullptr;                            // primary: op_*, profile, blocking forward
    std::vector<whenet::Engine*> replicas;                       // engines 1..inflight-1
    std::vector<char> snapshot;
    int device_id = 0, dtype = WHENET_F32;
    int inflight = 1;
    size_t next = 0;                                             // round-robin cursor
    // one large BLOCKING call (whenet_forward_u8 with n >= fanout_min) is cut into fanout_chunk-crop forwards spread over the
    // engines through their pinned-slot pipelines: copies of chunk i+1 overlap the forward of chunk i, results are bitwise
    // those of one forward (the kernels are batch-invariant).  fanout_min = 0 switches it off.
    int fanout_min = 256, fanout_chunk = 128, fanout_stage = 2, fanout_depth = 2;
    // fanout_stage 2 (round 6, default): the caller's array is registered with the runtime for the duration of the call (2 us when the
    // pages are resident, ~0.2 ms for a fresh 77 MB array; profiles/r06/hostreg_probe.txt), so every chunk's H2D copy is asynchronous:
    // ONE host thread enqueues everything, and chunk c's copy starts when chunk c-1's is done (stream-ordered across the engines) --
    // the chunks arrive in order at the link's full rate instead of two engines' copies sharing it (chunk 0 after 0.17 ms, not 0.68).
    // 0 / 1: round 5's forms (pinned staging / the runtime's pageable path, one host thread per engine).
    // -1 = calibrate between 0 and 1: how fast the runtime moves PAGEABLE memory differs from box to box (round 5: the direct form read
    // 126 k / 90 k / 130 k crops/s on three boxes where pinned staging read 110 / 110 / 107 k).  Calls 0 and 1 run one form each UNTIMED
    // (slots, arena growth, graph captures and lane streams are one-time costs of whichever form runs first), calls 2..5 alternate
    // the two forms timed, the best rate of each is kept and the faster form serves every later call.
    int fanout_calib_calls = 0;
    double fanout_calib_rate[2] = {0.0, 0.0};
    int fanout_chosen = -1;                                      // the form the last fan-out call ran (whenet_last_error-free diagnosis: option "fanout_stage" read back)
    // engines of the fan-out beyond primary + replicas: created on the first large call (option "fanout_engines", default 2: measured
    // 133 k crops/s at N = 512 f16 in every process, against 115-141 k from process to process with 3 and 123-128 k with 4), private
    // to it -- "inflight", the round-robin cursor and the chains per forward of everything else are not touched (round 6: the class used
    // to set inflight = 2 behind the caller's back)
    std::vector<whenet::Engine*> fan;
    int fanout_engines = 2;
    std::vector<std::pair<std::string, long>> options;           // replayed on new replicas
    whenet::Engine& at(size_t i) { return i == 0 ? *engine : *replicas[i - 1]; }
    // engine i of a fan-out over `count` engines: primary, replicas, then the private ones
    whenet::Engine& fan_at(size_t i) {
        if (i == 0) return *engine;
        if (i - 1 < replicas.size()) return *replicas[i - 1];
        return *fan[i - 1 - replicas.size()];
    }
    int fan_count() {
        const int want = std::max(inflight, std::min(fanout_engines, 4));
        while (1 + int(replicas.size()) + int(fan.size()) < want) {
            std::unique_ptr<whenet::Engine> r(new whenet::Engine(snapshot.data(), snapshot.size(), device_id, dtype));
            for (const auto& kv : options) r->set_option(kv.first, kv.second);
            fan.push_back(r.release());
        }
        return want;
    }
    whenet::Engine& take() {
        whenet::Engine& e = at(next % size_t(inflight));
        next = (next + 1) % size_t(inflight);
        return e;
    }
};

namespace {

thread_local std::string g_create_error;

// Page ranges this library has registered with the runtime for the duration of a fan-out call (fanout_stage 2).  Two handles driven by
// two threads may be handed adjacent slices of ONE array (whenet_hip/multi.py): the slices share a page, and registering / unregistering
// it from both sides races inside the runtime (segfaults in 3 of 8 runs of tests/test_multi_device.py).  A call whose pages overlap a
// range already held falls back to the runtime's pageable path.
struct HostRegistry {
    std::mutex mu;
    std::vector<std::pair<uintptr_t, uintptr_t>> held;
    static std::pair<uintptr_t, uintptr_t> page_range(const void* p, size_t nbytes) {
        const uintptr_t page = 4096, a = reinterpret_cast<uintptr_t>(p);
        return {a & ~(page - 1), (a + nbytes + page - 1) & ~(page - 1)};
    }
    bool acquire(const void* p, size_t nbytes, hipError_t* err) {
        const auto range = page_range(p, nbytes);
        std::lock_guard<std::mutex> lock(mu);
        for (const auto& r : held)
            if (range.first < r.second && r.first < range.second) {
                *err = hipErrorUnknown;
                return false;
            }
        *err = hipHostRegister(const_cast<void*>(p), nbytes, hipHostRegisterDefault);
        if (*err != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        held.push_back(range);
        return true;
    }
    void release(const void* p, size_t nbytes) {
        const auto range = page_range(p, nbytes);
        std::lock_guard<std::mutex> lock(mu);
        (void)hipHostUnregister(const_cast<void*>(p));
        for (size_t i = 0; i < held.size(); ++i)
            if (held[i] == range) {
                held.erase(held.begin() + long(i));
                break;
            }
    }
};
HostRegistry g_host_registry;

// The exception in flight (call it inside a catch block) as the ABI's return code, its text in msg.
int translate_exception(std::string& msg) {
    try {
        throw;
    } catch (const whenet::Error& e) {
        msg = e.what();
        return e.code;
    } catch (const std::bad_alloc&) {
        msg = "out of host memory";
        return WHENET_ENOMEM;
    } catch (const std::exception& e) {
        msg = e.what();
        return WHENET_EHIP;
    } catch (...) {
        msg = "unknown error";
        return WHENET_EHIP;
    }
}

template <typename F>
int guarded(whenet_t* h, F&& fn) {
    if (h == nullptr || h->engine == nullptr) return WHENET_EINVAL;
    try {
        fn(*h->engine);
        return WHENET_OK;
    } catch (...) {
        return translate_exception(h->engine->last_error);
    }
}

// one begin call on the engine whose turn it is; a refused call (the engine throws before it takes a slot) does not shift the round-robin
template <typename F>
int begin_on_next_engine(whenet_t* h, int* ticket, F&& begin) {
    if (ticket == nullptr) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine&) {
        const size_t idx = h->next % size_t(h->inflight);
        const int t = begin(h->at(idx));
        h->next = (h->next + 1) % size_t(h->inflight);
        *ticket = t * MAX_INFLIGHT_ENGINES + int(idx);
    });
}

int create_impl(const void* blob, size_t nbytes, int device_id, int dtype, whenet_t** out) {
    if (out == nullptr) return WHENET_EINVAL;
    *out = nullptr;
    try {
        std::unique_ptr<whenet::Engine> e(new whenet::Engine(blob, nbytes, device_id, dtype));
        whenet_t* h = new whenet_t;
        h->engine = e.release();
        h->snapshot.assign(static_cast<const char*>(blob), static_cast<const char*>(blob) + nbytes);
        h->device_id = device_id;
        h->dtype = dtype;
        *out = h;
        return WHENET_OK;
    } catch (...) {
        return translate_exception(g_create_error);
    }
}

// ---- the JPEG decoder's host statements (jpeg_dec_host.h, jpeg_dec_seg_host.h, jpeg_prog_host.h) ----
// No handle: the text of a refusal is whenet_last_error(NULL)'s.  Each exported function (below, JPEG decoder) checks its own
// arguments in its own order and names itself in every text; what they share is here (templates cannot stand inside extern "C").
using whenet::detail::jpeg_parse_or_refuse;

// the body's exception as the return code, its text in whenet_last_error(NULL)
template <typename F>
int host_statement(F&& body) {
    try {
        body();
        return WHENET_OK;
    } catch (...) {
        return translate_exception(g_create_error);
    }
}

void require_seg_args(const std::string& what, int seg_bytes, int window) {
    WHENET_REQUIRE(whenet::jpeg_seg_bytes_ok(seg_bytes), WHENET_EINVAL, what + ": seg_bytes must be a power of two in 4..4096");
    WHENET_REQUIRE(window >= 1 && window <= whenet::JPEG_SEG_MAX_WINDOW, WHENET_EINVAL, what + ": window must be 1..1024");
}

// One stream into a host surface: the header (plan: nullptr, or where the scan plan of a stream that may be progressive goes), the
// destination's checks, the padded planes by make_planes(info, planes), the pixel rule
template <typename F>
void decode_into_host_surface(const std::string& what, const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int rule,
                              whenet::JpegProgPlan* plan, F&& make_planes, bool layouts = false, bool sof2 = true) {
    whenet_jpeg_info_t info;
    jpeg_parse_or_refuse(what.c_str(), data, size, info, plan, layouts, sof2);
    const char* bad = whenet::jpeg_dec_check_dst(info, dst, channel_order, rule);
    WHENET_REQUIRE(bad == nullptr, WHENET_EINVAL, what + ": " + (bad ? bad : ""));
    WHENET_REQUIRE(dst->on_device == 0, WHENET_EINVAL, what + ": the surface must be host memory (on_device = 0)");
    whenet::JpegDecPlanes planes;
    make_planes(info, planes);
    whenet::jpeg_dec_frame_host(whenet::jpeg_dec_geom(info), planes, *dst, channel_order, rule);
}

// One stream into the caller's component planes: the header, the plane arguments, the padded planes by make_planes(info, planes),
// their rows out at the caller's pitch
template <typename F>
void decode_into_host_planes(const std::string& what, const uint8_t* data, int64_t size, uint8_t* const* planes, const int* pitch,
                             whenet::JpegProgPlan* plan, F&& make_planes, bool layouts = false, bool sof2 = true) {
    whenet_jpeg_info_t info;
    jpeg_parse_or_refuse(what.c_str(), data, size, info, plan, layouts, sof2);
    const whenet::JpegDecGeom g = whenet::jpeg_dec_geom(info);
    for (int c = 0; c < g.comps; ++c) {
        const int cw = c == 0 ? g.w : (g.w + g.hs - 1) / g.hs;
        WHENET_REQUIRE(planes[c] != nullptr && pitch[c] >= cw, WHENET_EINVAL,
                       what + ": plane " + std::to_string(c) + " is NULL or its pitch is below its " + std::to_string(cw) + " samples");
    }
    whenet::JpegDecPlanes pl;
    make_planes(info, pl);
    for (int c = 0; c < g.comps; ++c) {
        const int cw = c == 0 ? g.w : (g.w + g.hs - 1) / g.hs, ch = c == 0 ? g.h : (g.h + g.vs - 1) / g.vs;
        for (int y = 0; y < ch; ++y)
            std::memcpy(planes[c] + size_t(y) * size_t(pitch[c]), pl.plane[c].data() + size_t(y) * size_t(g.plane_pitch[c]), size_t(cw));
    }
}

// whenet_jpeg_decode_host and whenet_jpeg_decode_rule_host
int decode_host_as(const std::string& what, const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int rule,
                   int32_t status[2]) {
    return host_statement([&] {
        WHENET_REQUIRE(dst != nullptr && status != nullptr, WHENET_EINVAL, what + ": NULL argument");
        decode_into_host_surface(what, data, size, dst, channel_order, rule, nullptr, [&](const whenet_jpeg_info_t& info, whenet::JpegDecPlanes& pl) {
            whenet::jpeg_dec_planes_host(info, data + info.data_offset, int(size - info.data_offset), pl, status, rule);
        });
    });
}

// whenet_jpeg_decode_segmented_host and whenet_jpeg_decode_segmented_rule_host
int decode_segmented_host_as(const std::string& what, const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order,
                             int seg_bytes, int window, int rule, int32_t status[2], int64_t stats[8]) {
    return host_statement([&] {
        WHENET_REQUIRE(dst != nullptr && status != nullptr, WHENET_EINVAL, what + ": NULL argument");
        require_seg_args(what, seg_bytes, window);
        decode_into_host_surface(what, data, size, dst, channel_order, rule, nullptr, [&](const whenet_jpeg_info_t& info, whenet::JpegDecPlanes& pl) {
            whenet::jpeg_dec_planes_seg_host(info, data + info.data_offset, int(size - info.data_offset), seg_bytes, window, pl, status, stats, rule);
        });
    });
}

}  // namespace

extern "C" {
#pragma GCC visibility push(default)

int whenet_create(const char* snapshot_path, int device_id, int dtype, whenet_t** out) {
    if (snapshot_path == nullptr || out == nullptr) {
        g_create_error = "whenet_create: NULL argument";
        return WHENET_EINVAL;
    }
    std::vector<char> blob;
    try {
        std::ifstream f(snapshot_path, std::ios::binary | std::ios::ate);
        if (!f) {
            g_create_error = std::string("cannot open snapshot '") + snapshot_path + "'";
            return WHENET_ENOENT;
        }
        const std::streamoff sz = f.tellg();
        // a directory or an unseekable path reports -1 (or nonsense): an I/O error, not an allocation
        if (sz < 0 || !f.seekg(0) || uint64_t(sz) > (uint64_t(1) << 32)) {
            g_create_error = std::string("snapshot '") + snapshot_path + "' is not a readable regular file";
            return WHENET_EIO;
        }
        blob.resize(size_t(sz));
        if (sz > 0 && !f.read(blob.data(), std::streamsize(sz))) {
            g_create_error = std::string("cannot read snapshot '") + snapshot_path + "'";
            return WHENET_EIO;
        }
    } catch (const std::bad_alloc&) {
        g_create_error = "out of host memory";
        return WHENET_ENOMEM;
    } catch (const std::exception& e) {
        g_create_error = std::string("cannot read snapshot '") + snapshot_path + "': " + e.what();
        return WHENET_EIO;
    } catch (...) {
        g_create_error = std::string("cannot read snapshot '") + snapshot_path + "'";
        return WHENET_EIO;
    }
    return create_impl(blob.data(), blob.size(), device_id, dtype, out);
}

int whenet_create_from_memory(const void* snapshot, size_t nbytes, int device_id, int dtype, whenet_t** out) {
    if (snapshot == nullptr || out == nullptr) {
        g_create_error = "whenet_create_from_memory: NULL argument";
        return WHENET_EINVAL;
    }
    return create_impl(snapshot, nbytes, device_id, dtype, out);
}

int whenet_create_postproc(int device_id, whenet_t** out) {
    if (out == nullptr) {
        g_create_error = "whenet_create_postproc: NULL argument";
        return WHENET_EINVAL;
    }
    *out = nullptr;
    try {
        std::unique_ptr<whenet::Engine> e(new whenet::Engine(device_id));
        whenet_t* h = new whenet_t;
        h->engine = e.release();
        h->device_id = device_id;
        *out = h;
        return WHENET_OK;
    } catch (...) {
        return translate_exception(g_create_error);
    }
}

void whenet_destroy(whenet_t* h) {
    if (h == nullptr) return;
    try {
        for (whenet::Engine* e : h->replicas) delete e;
        for (whenet::Engine* e : h->fan) delete e;
        delete h->engine;
    } catch (...) {
    }
    delete h;
}

const char* whenet_last_error(const whenet_t* h) {
    if (h == nullptr || h->engine == nullptr) return g_create_error.c_str();
    return h->engine->last_error.c_str();
}

int whenet_get_info(const whenet_t* h, whenet_info_t* out) {
    if (h == nullptr || h->engine == nullptr || out == nullptr) return WHENET_EINVAL;
    h->engine->get_info(out);
    return WHENET_OK;
}

int whenet_set_option(whenet_t* h, const char* key, long value) {
    if (key == nullptr) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine& e) {
        const std::string k = key;
        if (k == "inflight") {
            WHENET_REQUIRE(value >= 1 && value <= MAX_INFLIGHT_ENGINES, WHENET_EINVAL, "inflight must be 1..4");
            WHENET_REQUIRE(!h->snapshot.empty() || value == 1, WHENET_EINVAL, "inflight: this handle has no network");
            e.release_aux_streams();
            for (whenet::Engine* r : h->replicas) r->release_aux_streams();
            for (whenet::Engine* r : h->fan) delete r;            // (rebuilt on the next large call)
            h->fan.clear();
            while (int(h->replicas.size()) + 1 > value) {
                delete h->replicas.back();
                h->replicas.pop_back();
            }
            while (int(h->replicas.size()) + 1 < value) {
                std::unique_ptr<whenet::Engine> r(
                    new whenet::Engine(h->snapshot.data(), h->snapshot.size(), h->device_id, h->dtype));
                for (const auto& kv : h->options) r->set_option(kv.first, kv.second);
                if (e.has_detector()) r->share_detector(e);
                h->replicas.push_back(r.release());
            }
            h->inflight = int(value);
            h->next = 0;
            // several forwards in flight: each runs as ONE chain, the concurrency comes from the others (a blocking host
            // forward keeps its own chains: Engine::host_lanes_)
            const long lanes = value > 1 ? 1 : 2;
            e.set_option("device_lanes", lanes);
            for (whenet::Engine* r : h->replicas) r->set_option("device_lanes", lanes);
            // several forwards share the chip: the XCD-grouped placement of the fused kernels pays at every batch (engine.h xcd_grouped)
            e.set_option("concurrent", value > 1);
            for (whenet::Engine* r : h->replicas) r->set_option("concurrent", value > 1);
            return;
        }
        if (k == "fanout_min" || k == "fanout_chunk" || k == "fanout_stage" || k == "fanout_depth" || k == "fanout_engines") {
            if (k == "fanout_engines") {
                WHENET_REQUIRE(value >= 1 && value <= MAX_INFLIGHT_ENGINES, WHENET_EINVAL, "fanout_engines must be 1..4");
                h->fanout_engines = int(value);
                for (whenet::Engine* r : h->fan) delete r;
                h->fan.clear();
                return;
            }
            if (k == "fanout_min") {
                WHENET_REQUIRE(value >= 0, WHENET_EINVAL, "fanout_min must be >= 0 (0 = never)");
                h->fanout_min = int(std::min<long>(value, 1 << 30));
            } else if (k == "fanout_chunk") {
                WHENET_REQUIRE(value >= 1 && value <= 4096, WHENET_EINVAL, "fanout_chunk must be 1..4096");
                h->fanout_chunk = int(value);
            } else if (k == "fanout_stage") {
                WHENET_REQUIRE(value >= -1 && value <= 3, WHENET_EINVAL,
                               "fanout_stage must be -1 (calibrate 0 against 1), 0 (pinned staging), 1 (the runtime's pageable path), 2 (registered, default) or 3 (probe: registered, a copy stream per engine)");
                h->fanout_stage = int(value);
                h->fanout_calib_calls = 0;
                h->fanout_calib_rate[0] = h->fanout_calib_rate[1] = 0.0;
            } else {
                WHENET_REQUIRE(value >= 1 && value <= WHENET_MAX_INFLIGHT, WHENET_EINVAL, "fanout_depth must be 1..4");
                h->fanout_depth = int(value);
            }
            return;
        }
        e.set_option(k, value);
        for (whenet::Engine* r : h->replicas) r->set_option(k, value);
        for (whenet::Engine* r : h->fan) r->set_option(k, value);
        h->options.emplace_back(k, value);
    });
}

int whenet_forward_u8(whenet_t* h, const uint8_t* crops, int n, float* ypr, int32_t* argmax, float* logits) {
    return guarded(h, [&](whenet::Engine& e) {
        bool pending = e.has_pending();                 // the caller's own submissions hold slots: leave them alone
        for (whenet::Engine* r : h->replicas) pending = pending || r->has_pending();
        if (h->fanout_min <= 0 || n < h->fanout_min || n <= h->fanout_chunk || pending || h->snapshot.empty()) {
            e.forward_host(crops, n, ypr, argmax, logits);
            return;
        }
        WHENET_REQUIRE(crops != nullptr && ypr != nullptr, WHENET_EINVAL, "crops and ypr must not be NULL");
        // get_angle(np.uint8[N,...]) with a large N (whenet.py:22-27 takes any N): chunk c goes to engine c % E of the fan-out, at most
        // fanout_depth outstanding per engine, results land in the caller's arrays at the chunk's offset.  Round 6 (fanout_stage 2): the
        // array is registered for the call, so this ONE thread enqueues everything and the copies run in order on one stream.  Round 5's
        // forms (stages 0 / 1, further down): every engine is driven by its OWN host thread (the calling thread takes engine 0) --
        // staging a chunk is a 9.6 MB memcpy into pinned memory, ~0.6 ms on one core, more than the 0.42 ms the GPU needs for it, and a
        // copy from pageable memory blocks its caller.  Engines share nothing but the device.
        const int chunk = h->fanout_chunk;
        int stage = h->fanout_stage;
        const bool calibrating = stage < 0;
        if (calibrating)
            stage = h->fanout_calib_calls < 6 ? 1 - (h->fanout_calib_calls & 1) : (h->fanout_calib_rate[1] >= h->fanout_calib_rate[0] ? 1 : 0);
        const auto t_start = std::chrono::steady_clock::now();
        // one engine: the chunk itself supplies the concurrency (two chains); several engines: one chain each
        const int nfan = h->fan_count();
        const int lanes = nfan > 1 ? 1 : 2;
        if (stage == 2 || stage == 3) {
            const bool shared_copy_stream = stage == 2;           // 3 (probe): every engine's own copy stream, chained by events
            whenet::detail::DeviceGuard guard(h->device_id);
            const size_t nbytes = size_t(n) * 150528;
            hipError_t re = hipSuccess;
            const bool registered = g_host_registry.acquire(crops, nbytes, &re);
            if (registered || re == hipErrorHostMemoryAlreadyRegistered) {       // (already registered: the caller pinned it)
                h->fanout_chosen = stage;
                struct Pending { int eng, ticket, off; };
                std::vector<Pending> q;
                size_t head = 0;
                std::vector<int> outstanding(size_t(nfan), 0);
                // every chunk's copy goes through ONE stream (the primary engine's copy stream): in order at the link's full rate, and one
                // stream fewer per engine for the runtime to place on its four hardware queues (with a copy stream per engine the same
                // call read 102 k or 134 k crops/s from process to process: profiles/r06/host_path_probe.txt)
                const hipStream_t copy_on = shared_copy_stream ? h->engine->copy_stream_handle() : nullptr;
                hipEvent_t prev = nullptr;
                auto collect_head = [&] {
                    const Pending& p = q[head++];
                    const size_t o = size_t(p.off);
                    h->fan_at(size_t(p.eng)).collect(p.ticket, ypr + o * 3, argmax ? argmax + o * 3 : nullptr, logits ? logits + o * 252 : nullptr);
                    --outstanding[size_t(p.eng)];
                };
                std::exception_ptr err;
                try {
                    int off = 0, c = 0;
                    while (off < n) {
                        // the first two chunks are half-size: the GPU starts after half a chunk's copy
                        const int want = c < 2 && chunk >= 32 ? chunk / 2 : chunk;
                        const int cnt = std::min(want, n - off), ei = c % nfan;
                        while (outstanding[size_t(ei)] >= h->fanout_depth) collect_head();     // (in submission order: engine ei's oldest is reached)
                        whenet::Engine& eng = h->fan_at(size_t(ei));
                        const int ticket = eng.submit(crops + size_t(off) * 150528, cnt, 1, lanes, copy_on, shared_copy_stream ? nullptr : prev);
                        if (!shared_copy_stream) prev = eng.copied_event(ticket);
                        q.push_back(Pending{ei, ticket, off});
                        ++outstanding[size_t(ei)];
                        off += cnt;
                        ++c;
                    }
                    while (head < q.size()) collect_head();
                } catch (...) {
                    err = std::current_exception();
                    for (int i = 0; i < nfan; ++i) {
                        try { h->fan_at(size_t(i)).abandon_submissions(); } catch (...) {}
                    }
                }
                if (registered) g_host_registry.release(crops, nbytes);
                if (err) std::rethrow_exception(err);
                return;
            }
            stage = 1;                                           // the runtime would not register the array: its pageable path
        }
        h->fanout_chosen = stage;
        const int nthreads = nfan;
        const int nchunks = (n + chunk - 1) / chunk;
        std::vector<std::exception_ptr> errs;
        errs.resize(static_cast<size_t>(nthreads));
        auto drive = [&](int t) {
            whenet::Engine& eng = h->fan_at(size_t(t));
            struct Pending { int ticket, off; };
            std::vector<Pending> q;
            size_t head = 0;
            auto collect_one = [&] {
                const Pending& p = q[head++];
                const size_t o = size_t(p.off);
                eng.collect(p.ticket, ypr + o * 3, argmax ? argmax + o * 3 : nullptr, logits ? logits + o * 252 : nullptr);
            };
            try {
                for (int c = t; c < nchunks; c += nthreads) {
                    if (q.size() - head >= size_t(h->fanout_depth)) collect_one();
                    const int off = c * chunk, cnt = std::min(chunk, n - off);
                    q.push_back(Pending{eng.submit(crops + size_t(off) * 150528, cnt, stage, lanes), off});
                }
                while (head < q.size()) collect_one();
            } catch (...) {
                errs[size_t(t)] = std::current_exception();
                try {                                            // (on a worker thread nothing may escape: std::terminate)
                    eng.abandon_submissions();
                } catch (...) {
                }
            }
        };
        std::vector<std::thread> workers;
        workers.reserve(size_t(nthreads));
        int started = 1;                                         // (engine 0 is the calling thread's)
        try {
            for (int t = 1; t < nthreads; ++t, ++started) workers.emplace_back(drive, t);
        } catch (...) {                                          // no thread to be had: the engines without one are driven from here
        }
        drive(0);
        for (int t = started; t < nthreads; ++t) drive(t);
        for (std::thread& w : workers) w.join();
        for (const std::exception_ptr& ep : errs)
            if (ep) std::rethrow_exception(ep);
        if (calibrating && h->fanout_calib_calls < 6) {
            if (h->fanout_calib_calls >= 2) {                     // (calls 0 and 1 warm both forms up, untimed)
                const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
                h->fanout_calib_rate[stage] = std::max(h->fanout_calib_rate[stage], double(n) / (sec > 0 ? sec : 1e-9));
            }
            ++h->fanout_calib_calls;
        }
    });
}

int whenet_forward_f32(whenet_t* h, const float* image, int n, float* ypr, int32_t* argmax, float* logits) {
    return guarded(h, [&](whenet::Engine& e) { e.forward_host_f32(image, n, ypr, argmax, logits); });
}

int whenet_forward_u8_device(whenet_t* h, const uint8_t* d_crops, int n, float* d_ypr, int32_t* d_argmax,
                             float* d_logits, void* stream) {
    return guarded(h, [&](whenet::Engine& e) {
        // caller's stream: strictly ordered on it (primary engine); handle-owned streams: next engine
        whenet::Engine& eng = (stream != nullptr) ? e : h->take();
        eng.forward_device(d_crops, n, d_ypr, d_argmax, d_logits, static_cast<hipStream_t>(stream));
    });
}

int whenet_sync(whenet_t* h) {
    return guarded(h, [&](whenet::Engine& e) {
        e.sync();
        for (whenet::Engine* r : h->replicas) r->sync();
        for (whenet::Engine* r : h->fan) r->sync();
    });
}

// tickets of the pinned pipeline carry the engine index in their low bits
int whenet_submit_u8(whenet_t* h, const uint8_t* crops, int n, int* ticket) {
    if (ticket == nullptr) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine&) {
        const size_t idx = h->next % size_t(h->inflight);
        *ticket = h->take().submit(crops, n) * MAX_INFLIGHT_ENGINES + int(idx);
    });
}

int whenet_frame_rects(int frame_h, int frame_w, const float* bboxes, int k, int32_t* rects) {
    if (frame_h <= 0 || frame_w <= 0 || k < 0 || (k > 0 && (bboxes == nullptr || rects == nullptr))) return WHENET_EINVAL;
    for (int i = 0; i < k; ++i) whenet::frame_box_rect(frame_h, frame_w, bboxes + 4 * i, rects + 4 * i);
    return WHENET_OK;
}

int whenet_normalise_table(float lut[768]) {
    if (lut == nullptr) return WHENET_EINVAL;
    whenet::normalise_table(reinterpret_cast<float (*)[256]>(lut));
    return WHENET_OK;
}

int whenet_submit_frame(whenet_t* h, const uint8_t* frame, int frame_h, int frame_w, int channel_order,
                        const int32_t* rects, int k, int* ticket) {
    if (ticket == nullptr || (channel_order != WHENET_RGB && channel_order != WHENET_BGR)) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine&) {
        const size_t idx = h->next % size_t(h->inflight);
        *ticket = h->take().submit_frame(frame, frame_h, frame_w, channel_order == WHENET_BGR, rects, k) *
                      MAX_INFLIGHT_ENGINES + int(idx);
    });
}

int whenet_op_crop_resize(whenet_t* h, const uint8_t* frame, int frame_h, int frame_w, int channel_order,
                          const int32_t* rects, int k, uint8_t* crops) {
    if (channel_order != WHENET_RGB && channel_order != WHENET_BGR) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine& e) {
        e.op_crop_resize(frame, frame_h, frame_w, channel_order == WHENET_BGR, rects, k, crops);
    });
}

int whenet_letterbox_plan(int in_h, int in_w, int out_h, int out_w, int32_t geom[4], int axis, int32_t* bounds, int32_t* coeffs,
                          int cap, int* ksize) {
    if (geom == nullptr || ksize == nullptr || (axis != 0 && axis != 1) || (bounds == nullptr) != (coeffs == nullptr)) return WHENET_EINVAL;
    try {
        const whenet::LetterboxPlan p = whenet::letterbox_plan_layout(in_h, in_w, out_h, out_w);
        geom[0] = p.nw, geom[1] = p.nh, geom[2] = p.x0, geom[3] = p.y0;
        const int in_size = axis == 0 ? in_w : in_h, out_size = axis == 0 ? p.nw : p.nh;
        *ksize = axis == 0 ? p.ksx : p.ksy;
        if (bounds == nullptr) return WHENET_OK;
        if (cap < out_size * *ksize) return WHENET_EINVAL;
        whenet::build_letterbox_axis(in_size, out_size, bounds, coeffs);
        return WHENET_OK;
    } catch (const whenet::Error& e) {
        return e.code;
    } catch (...) {
        return WHENET_ENOMEM;
    }
}

int whenet_op_letterbox(whenet_t* h, const uint8_t* frame, int frame_h, int frame_w, int channel_order, int out_h, int out_w,
                        uint8_t* canvas_u8, float* image_f32) {
    if (channel_order != WHENET_RGB && channel_order != WHENET_BGR) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine& e) {
        e.op_letterbox(frame, frame_h, frame_w, channel_order == WHENET_BGR, out_h, out_w, canvas_u8, image_f32);
    });
}

// the resident-frame form: the ticket of whenet_frame_begin carries its engine like every other ticket
int whenet_frame_begin(whenet_t* h, const uint8_t* frame, int frame_h, int frame_w, int channel_order, int* ticket) {
    if (ticket == nullptr || (channel_order != WHENET_RGB && channel_order != WHENET_BGR)) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine&) {
        const size_t idx = h->next % size_t(h->inflight);
        *ticket = h->take().frame_begin(frame, frame_h, frame_w, channel_order == WHENET_BGR) * MAX_INFLIGHT_ENGINES + int(idx);
    });
}

int whenet_frame_letterbox(whenet_t* h, int ticket, int out_h, int out_w, uint8_t* canvas_u8, float* image_f32) {
    return guarded(h, [&](whenet::Engine&) {
        const int idx = ticket % MAX_INFLIGHT_ENGINES;
        WHENET_REQUIRE(ticket >= 0 && idx < h->inflight, WHENET_EINVAL, "unknown ticket " + std::to_string(ticket));
        h->at(size_t(idx)).frame_letterbox(ticket / MAX_INFLIGHT_ENGINES, out_h, out_w, canvas_u8, image_f32);
    });
}

int whenet_frame_heads(whenet_t* h, int ticket, const int32_t* rects, int k) {
    return guarded(h, [&](whenet::Engine&) {
        const int idx = ticket % MAX_INFLIGHT_ENGINES;
        WHENET_REQUIRE(ticket >= 0 && idx < h->inflight, WHENET_EINVAL, "unknown ticket " + std::to_string(ticket));
        h->at(size_t(idx)).frame_heads(ticket / MAX_INFLIGHT_ENGINES, rects, k);
    });
}

int whenet_yolo_eval(whenet_t* h, const float* const* feats, const int* grid_h, const int* grid_w, int num_layers,
                     const float* anchors, int num_anchors, int num_classes, float image_h, float image_w,
                     float score_threshold, float iou_threshold, int max_boxes, float* boxes, float* scores,
                     int32_t* classes, int32_t* index, int* count, float* all_boxes, float* all_scores) {
    if (count == nullptr) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine& e) {
        *count = e.yolo_eval(feats, grid_h, grid_w, num_layers, anchors, num_anchors, num_classes, image_h, image_w,
                             score_threshold, iou_threshold, max_boxes, boxes, scores, classes, index, all_boxes,
                             all_scores);
    });
}

// ---- the detector body (detector.cpp) ----
namespace {
int read_file(const char* path, std::vector<char>& blob, std::string& err) {
    try {
        std::ifstream f(path, std::ios::binary | std::ios::ate);
        if (!f) {
            err = std::string("cannot open snapshot '") + path + "'";
            return WHENET_ENOENT;
        }
        const std::streamoff sz = f.tellg();
        if (sz < 0 || !f.seekg(0) || uint64_t(sz) > (uint64_t(1) << 32)) {
            err = std::string("snapshot '") + path + "' is not a readable regular file";
            return WHENET_EIO;
        }
        blob.resize(size_t(sz));
        if (sz > 0 && !f.read(blob.data(), std::streamsize(sz))) {
            err = std::string("cannot read snapshot '") + path + "'";
            return WHENET_EIO;
        }
        return WHENET_OK;
    } catch (const std::bad_alloc&) {
        err = "out of host memory";
        return WHENET_ENOMEM;
    } catch (...) {
        err = std::string("cannot read snapshot '") + path + "'";
        return WHENET_EIO;
    }
}
}  // namespace

int whenet_detector_load_from_memory(whenet_t* h, const void* snapshot, size_t nbytes) {
    return guarded(h, [&](whenet::Engine& e) {
        e.detector_load(snapshot, nbytes);
        for (whenet::Engine* r : h->replicas) r->share_detector(e);
    });
}

int whenet_detector_load(whenet_t* h, const char* snapshot_path) {
    if (h == nullptr || h->engine == nullptr || snapshot_path == nullptr) return WHENET_EINVAL;
    std::vector<char> blob;
    const int rc = read_file(snapshot_path, blob, h->engine->last_error);
    if (rc != WHENET_OK) return rc;
    return whenet_detector_load_from_memory(h, blob.data(), blob.size());
}

int whenet_detector_spec(int kind, int anchors_per_scale, int num_classes, int index, int32_t out[12], int* count) {
    if ((kind != 0 && kind != 1) || anchors_per_scale < 1 || num_classes < 1 || anchors_per_scale > 64 || num_classes > 4096) return WHENET_EINVAL;
    try {
        const std::vector<whenet::DetLayer> t = whenet::detector_table(kind, anchors_per_scale * (num_classes + 5));
        if (count) *count = int(t.size());
        if (out == nullptr) return count ? WHENET_OK : WHENET_EINVAL;
        if (index < 0 || index >= int(t.size())) return WHENET_EINVAL;
        const whenet::DetLayer& L = t[size_t(index)];
        const int32_t v[12] = {L.op, L.k, L.stride, L.cin, L.cout, L.bn, L.leaky, L.src0, L.src1, L.skip, L.is_output, L.cin0};
        std::memcpy(out, v, sizeof(v));
        return WHENET_OK;
    } catch (const whenet::Error& e) {
        return e.code;
    } catch (...) {
        return WHENET_ENOMEM;
    }
}

int whenet_op_dconv(whenet_t* h, const float* in, int n, int H, int W, int cin, const float* in2, int cin2, const float* kernel,
                    const float* bias, int k, int stride, int cout, int leaky, const float* skip, int f32_out, float* out) {
    return guarded(h, [&](whenet::Engine& e) { e.op_dconv(in, n, H, W, cin, in2, cin2, kernel, bias, k, stride, cout, leaky, skip, f32_out, out); });
}

int whenet_op_dpool(whenet_t* h, const float* in, int n, int H, int W, int c, int stride, float* out) {
    return guarded(h, [&](whenet::Engine& e) { e.op_dpool(in, n, H, W, c, stride, out); });
}

int whenet_detector_forward(whenet_t* h, const float* image, int n, int H, int W, float* const* maps) {
    return guarded(h, [&](whenet::Engine& e) { e.detector_forward(image, n, H, W, maps); });
}

int whenet_op_detect(whenet_t* h, const uint8_t* frame, int frame_h, int frame_w, int channel_order, int out_h, int out_w,
                     const float* anchors, int num_anchors, float score_threshold, float iou_threshold, int max_boxes, float* boxes,
                     float* scores, int32_t* classes, int* count) {
    if (count == nullptr || (channel_order != WHENET_RGB && channel_order != WHENET_BGR)) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine& e) {
        *count = e.op_detect(frame, frame_h, frame_w, channel_order == WHENET_BGR, out_h, out_w, anchors, num_anchors, score_threshold,
                             iou_threshold, max_boxes, boxes, scores, classes);
    });
}

int whenet_frame_detect(whenet_t* h, int ticket, int out_h, int out_w, const float* anchors, int num_anchors, float score_threshold,
                        float iou_threshold, int max_boxes, float* boxes, float* scores, int32_t* classes, int* count) {
    if (count == nullptr) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine&) {
        const int idx = ticket % MAX_INFLIGHT_ENGINES;
        WHENET_REQUIRE(ticket >= 0 && idx < h->inflight, WHENET_EINVAL, "unknown ticket " + std::to_string(ticket));
        *count = h->at(size_t(idx)).frame_detect(ticket / MAX_INFLIGHT_ENGINES, out_h, out_w, anchors, num_anchors, score_threshold,
                                                 iou_threshold, max_boxes, boxes, scores, classes);
    });
}

int whenet_frame_detect_heads(whenet_t* h, int ticket, int out_h, int out_w, const float* anchors, int num_anchors, float score_threshold,
                              float iou_threshold, int max_boxes) {
    return guarded(h, [&](whenet::Engine&) {
        const int idx = ticket % MAX_INFLIGHT_ENGINES;
        WHENET_REQUIRE(ticket >= 0 && idx < h->inflight, WHENET_EINVAL, "unknown ticket " + std::to_string(ticket));
        h->at(size_t(idx)).frame_detect_heads(ticket / MAX_INFLIGHT_ENGINES, out_h, out_w, anchors, num_anchors, score_threshold,
                                              iou_threshold, max_boxes);
    });
}

int whenet_collect_detect(whenet_t* h, int ticket, int capacity, int* count, float* boxes, float* scores, int32_t* classes, int32_t* rects,
                          int32_t* valid, float* ypr, int32_t* argmax, float* logits) {
    if (count == nullptr) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine&) {
        const int idx = ticket % MAX_INFLIGHT_ENGINES;
        WHENET_REQUIRE(ticket >= 0 && idx < h->inflight, WHENET_EINVAL, "unknown ticket " + std::to_string(ticket));
        *count = h->at(size_t(idx)).collect_detect(ticket / MAX_INFLIGHT_ENGINES, capacity, boxes, scores, classes, rects, valid, ypr, argmax,
                                                   logits);
    });
}

int whenet_op_head_plan(whenet_t* h, int frame_h, int frame_w, const float* boxes, int k, int32_t* rects, int32_t* valid, int32_t* plans) {
    return guarded(h, [&](whenet::Engine& e) { e.op_head_plan(frame_h, frame_w, boxes, k, rects, valid, plans); });
}

// ---- clips: F frames per submission (detector.cpp, engine_post.cpp) ----
int whenet_clip_begin(whenet_t* h, const uint8_t* frames, int num_frames, int frame_h, int frame_w, int channel_order, int* ticket) {
    if (ticket == nullptr || (channel_order != WHENET_RGB && channel_order != WHENET_BGR)) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine& e) {
        // (argument errors before an engine is taken: a refused clip must not shift the round-robin)
        WHENET_REQUIRE(num_frames >= 1 && num_frames <= 16, WHENET_EINVAL,
                       "clip_begin: " + std::to_string(num_frames) + " frames: a clip holds 1..16 (the detector's batch limit)");
        (void)e;
        const size_t idx = h->next % size_t(h->inflight);
        *ticket = h->take().clip_begin(frames, num_frames, frame_h, frame_w, channel_order == WHENET_BGR) * MAX_INFLIGHT_ENGINES + int(idx);
    });
}

int whenet_clip_detect_heads(whenet_t* h, int ticket, int out_h, int out_w, const float* anchors, int num_anchors, float score_threshold,
                             float iou_threshold, int max_boxes, int max_heads, int* slots_per_frame) {
    if (slots_per_frame == nullptr) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine&) {
        const int idx = ticket % MAX_INFLIGHT_ENGINES;
        WHENET_REQUIRE(ticket >= 0 && idx < h->inflight, WHENET_EINVAL, "unknown ticket " + std::to_string(ticket));
        *slots_per_frame = h->at(size_t(idx)).clip_detect_heads(ticket / MAX_INFLIGHT_ENGINES, out_h, out_w, anchors, num_anchors,
                                                                score_threshold, iou_threshold, max_boxes, max_heads);
    });
}

int whenet_collect_clip(whenet_t* h, int ticket, int capacity, int* num_frames, int32_t* counts, float* boxes, float* scores,
                        int32_t* classes, int32_t* rects, int32_t* valid, int32_t* row, float* ypr, int32_t* argmax, float* logits,
                        int* rows_used, int* overflow) {
    return guarded(h, [&](whenet::Engine&) {
        const int idx = ticket % MAX_INFLIGHT_ENGINES;
        WHENET_REQUIRE(ticket >= 0 && idx < h->inflight, WHENET_EINVAL, "unknown ticket " + std::to_string(ticket));
        h->at(size_t(idx)).collect_clip(ticket / MAX_INFLIGHT_ENGINES, capacity, num_frames, counts, boxes, scores, classes, rects, valid, row,
                                        ypr, argmax, logits, rows_used, overflow);
    });
}

// ---- clips of frames of different sizes, and the letterbox geometry cache (engine_post.cpp) ----
int whenet_clip_begin_mixed(whenet_t* h, const uint8_t* const* frames, int num_frames, const int* frame_h, const int* frame_w, int channel_order,
                            int* ticket) {
    if (ticket == nullptr || (channel_order != WHENET_RGB && channel_order != WHENET_BGR)) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine&) {
        // (argument errors before an engine is taken: a refused clip must not shift the round-robin)
        whenet::Engine::check_mixed_frames("clip_begin_mixed", frames, num_frames, frame_h, frame_w);
        const size_t idx = h->next % size_t(h->inflight);
        whenet::Engine& e = h->at(idx);
        const int t = e.clip_begin_mixed(frames, num_frames, frame_h, frame_w, channel_order == WHENET_BGR);
        h->next = (h->next + 1) % size_t(h->inflight);
        *ticket = t * MAX_INFLIGHT_ENGINES + int(idx);
    });
}

int whenet_op_letterbox_mixed(whenet_t* h, const uint8_t* const* frames, int num_frames, const int* frame_h, const int* frame_w,
                              int channel_order, int out_h, int out_w, uint8_t* canvas_u8, float* image_f32) {
    if (channel_order != WHENET_RGB && channel_order != WHENET_BGR) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine& e) {
        e.op_letterbox_mixed(frames, num_frames, frame_h, frame_w, channel_order == WHENET_BGR, out_h, out_w, canvas_u8, image_f32);
    });
}

// ---- YUV 4:2:0 ingest (yuv.hip, engine_post.cpp) ----
int whenet_yuv_to_bgr_host(const whenet_yuv_frame_t* frame, uint8_t* bgr) {
    if (frame == nullptr || bgr == nullptr) return WHENET_EINVAL;
    try {
        whenet::check_yuv_frames("yuv_to_bgr_host", frame, 1);
        whenet::yuv_to_bgr_host(*frame, bgr);
        return WHENET_OK;
    } catch (...) {
        return translate_exception(g_create_error);      // (no handle: the text is whenet_last_error(NULL)'s)
    }
}

int whenet_op_yuv_to_bgr(whenet_t* h, const whenet_yuv_frame_t* frames, int num_frames, uint8_t* const* bgr) {
    return guarded(h, [&](whenet::Engine& e) { e.op_yuv_to_bgr(frames, num_frames, bgr); });
}

int whenet_frame_begin_yuv(whenet_t* h, const whenet_yuv_frame_t* frame, int* ticket) {
    if (ticket == nullptr) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine&) {
        // (argument errors before an engine is taken: a refused frame must not shift the round-robin)
        whenet::check_yuv_frames("frame_begin_yuv", frame, 1);
        const size_t idx = h->next % size_t(h->inflight);
        const int t = h->at(idx).frame_begin_yuv(*frame);
        h->next = (h->next + 1) % size_t(h->inflight);
        *ticket = t * MAX_INFLIGHT_ENGINES + int(idx);
    });
}

int whenet_clip_begin_yuv(whenet_t* h, const whenet_yuv_frame_t* frames, int num_frames, int* ticket) {
    if (ticket == nullptr) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine&) {
        whenet::check_yuv_frames("clip_begin_yuv", frames, num_frames);
        const size_t idx = h->next % size_t(h->inflight);
        const int t = h->at(idx).clip_begin_yuv(frames, num_frames);
        h->next = (h->next + 1) % size_t(h->inflight);
        *ticket = t * MAX_INFLIGHT_ENGINES + int(idx);
    });
}

// ---- ingest from device memory (ingest.hip, yuv.hip, engine_post.cpp) ----
int whenet_frame_begin_device(whenet_t* h, const uint8_t* d_frame, int pitch, int frame_h, int frame_w, int channel_order, void* stream,
                              int* ticket) {
    if (channel_order != WHENET_RGB && channel_order != WHENET_BGR) return WHENET_EINVAL;
    return begin_on_next_engine(h, ticket, [&](whenet::Engine& e) {
        return e.frame_begin_device(d_frame, pitch, frame_h, frame_w, channel_order == WHENET_BGR, static_cast<hipStream_t>(stream));
    });
}

int whenet_clip_begin_device(whenet_t* h, const uint8_t* const* d_frames, const int* pitch, int num_frames, const int* frame_h,
                             const int* frame_w, int channel_order, void* stream, int* ticket) {
    if (channel_order != WHENET_RGB && channel_order != WHENET_BGR) return WHENET_EINVAL;
    return begin_on_next_engine(h, ticket, [&](whenet::Engine& e) {
        return e.clip_begin_device(d_frames, pitch, num_frames, frame_h, frame_w, channel_order == WHENET_BGR, static_cast<hipStream_t>(stream));
    });
}

int whenet_frame_begin_yuv_device(whenet_t* h, const whenet_yuv_frame_t* frame, void* stream, int* ticket) {
    return begin_on_next_engine(h, ticket, [&](whenet::Engine& e) {
        whenet::check_yuv_frames("frame_begin_yuv_device", frame, 1);      // (NULL)
        return e.frame_begin_yuv_device(*frame, static_cast<hipStream_t>(stream));
    });
}

int whenet_clip_begin_yuv_device(whenet_t* h, const whenet_yuv_frame_t* frames, int num_frames, void* stream, int* ticket) {
    return begin_on_next_engine(h, ticket, [&](whenet::Engine& e) {
        return e.clip_begin_yuv_device(frames, num_frames, static_cast<hipStream_t>(stream));
    });
}

int whenet_op_pack_device(whenet_t* h, const uint8_t* const* d_frames, const int* pitch, int num_frames, const int* frame_h,
                          const int* frame_w, void* stream, uint8_t* const* out) {
    return guarded(h, [&](whenet::Engine& e) {
        e.op_pack_device(d_frames, pitch, num_frames, frame_h, frame_w, static_cast<hipStream_t>(stream), out);
    });
}

int whenet_op_yuv_to_bgr_device(whenet_t* h, const whenet_yuv_frame_t* frames, int num_frames, void* stream, uint8_t* const* bgr) {
    return guarded(h, [&](whenet::Engine& e) { e.op_yuv_to_bgr_device(frames, num_frames, static_cast<hipStream_t>(stream), bgr); });
}

// ---- extended YUV ingest (include/whenet_hip_yuv_ext.h; yuvx.hip, yuvx_host.h, engine_post.cpp) ----
int whenet_yuvx_to_bgr_host(const whenet_yuvx_frame_t* frame, uint8_t* bgr) {
    if (frame == nullptr || bgr == nullptr) return WHENET_EINVAL;
    try {
        whenet::check_yuvx_frames("yuvx_to_bgr_host", frame, 1);
        whenet::yuvx_to_bgr_host(*frame, bgr);
        return WHENET_OK;
    } catch (...) {
        return translate_exception(g_create_error);      // (no handle: the text is whenet_last_error(NULL)'s)
    }
}

int whenet_op_yuvx_to_bgr(whenet_t* h, const whenet_yuvx_frame_t* frames, int num_frames, uint8_t* const* bgr) {
    return guarded(h, [&](whenet::Engine& e) { e.op_yuvx_to_bgr(frames, num_frames, bgr); });
}

// (begin_yuvx checks the arguments before it takes a slot, and a refusal throws before the round-robin moves)
int whenet_frame_begin_yuvx(whenet_t* h, const whenet_yuvx_frame_t* frame, int* ticket) {
    return begin_on_next_engine(h, ticket, [&](whenet::Engine& e) { return e.begin_yuvx("frame_begin_yuvx", frame, 1, false, false, nullptr); });
}

int whenet_clip_begin_yuvx(whenet_t* h, const whenet_yuvx_frame_t* frames, int num_frames, int* ticket) {
    return begin_on_next_engine(h, ticket, [&](whenet::Engine& e) { return e.begin_yuvx("clip_begin_yuvx", frames, num_frames, true, false, nullptr); });
}

int whenet_frame_begin_yuvx_device(whenet_t* h, const whenet_yuvx_frame_t* frame, void* stream, int* ticket) {
    return begin_on_next_engine(h, ticket, [&](whenet::Engine& e) {
        return e.begin_yuvx("frame_begin_yuvx_device", frame, 1, false, true, static_cast<hipStream_t>(stream));
    });
}

int whenet_clip_begin_yuvx_device(whenet_t* h, const whenet_yuvx_frame_t* frames, int num_frames, void* stream, int* ticket) {
    return begin_on_next_engine(h, ticket, [&](whenet::Engine& e) {
        return e.begin_yuvx("clip_begin_yuvx_device", frames, num_frames, true, true, static_cast<hipStream_t>(stream));
    });
}

int whenet_op_yuvx_to_bgr_device(whenet_t* h, const whenet_yuvx_frame_t* frames, int num_frames, void* stream, uint8_t* const* bgr) {
    return guarded(h, [&](whenet::Engine& e) { e.op_yuvx_to_bgr_device(frames, num_frames, static_cast<hipStream_t>(stream), bgr); });
}

// ---- pose overlay (overlay.hip, overlay_host.h, engine_post.cpp) ----
int whenet_overlay_segments(const int32_t rect[4], float yaw, float pitch, float roll, int32_t segments[16], int32_t* flags) {
    if (rect == nullptr || segments == nullptr) return WHENET_EINVAL;
    if (!whenet::overlay_rect_in_range(rect)) {
        g_create_error = "overlay_segments: a window coordinate outside -4096..8192";
        return WHENET_EINVAL;
    }
    const int f = whenet::overlay_segments(rect, 1, double(yaw), double(pitch), double(roll), segments);
    if (flags) *flags = f;
    return WHENET_OK;
}

int whenet_overlay_labels(const int32_t rect[4], float yaw, float pitch, float roll, char text[3][16], int32_t origin[3][2], int32_t* flags) {
    if (rect == nullptr || text == nullptr || origin == nullptr) return WHENET_EINVAL;
    if (!whenet::overlay_rect_in_range(rect)) {
        g_create_error = "overlay_labels: a window coordinate outside -4096..8192";
        return WHENET_EINVAL;
    }
    int32_t seg[whenet::OVERLAY_SEG_INTS];
    whenet::OverlayLine lines[3];
    int f = whenet::overlay_segments(rect, 1, double(yaw), double(pitch), double(roll), seg);
    f |= whenet::overlay_labels(seg, f, yaw, pitch, roll, lines, origin);
    const char* const glyphs = WHENET_OVERLAY_GLYPHS;
    for (int l = 0; l < 3; ++l) {
        std::memset(text[l], 0, 16);
        for (int i = 0; i < whenet::overlay_line_length(lines[l]); ++i) text[l][i] = glyphs[whenet::overlay_line_glyph(lines[l], i)];
    }
    if (flags) *flags = f;
    return WHENET_OK;
}

int whenet_overlay_glyph(int ch, int32_t segs[8][4]) {
    const int g = whenet::overlay_glyph_index(ch);
    if (segs == nullptr || g < 0) return WHENET_EINVAL;
    const int8_t* row = whenet::OVERLAY_FONT.seg[g];
    for (int s = 0; s < whenet::OVERLAY_GLYPH_SEGS; ++s)
        for (int j = 0; j < 4; ++j) segs[s][j] = row[1 + 4 * s + j];
    return row[0];
}

int whenet_annotate_host(const uint8_t* frame, int frame_h, int frame_w, int channel_order, const int32_t* rects, const int32_t* valid,
                         const float* ypr, int k, const whenet_surface_t* dst) {
    return whenet_annotate_host_ex(frame, frame_h, frame_w, channel_order, rects, valid, ypr, k, dst, WHENET_DISPLAY_SIMPLE);
}

int whenet_annotate_host_ex(const uint8_t* frame, int frame_h, int frame_w, int channel_order, const int32_t* rects, const int32_t* valid,
                            const float* ypr, int k, const whenet_surface_t* dst, int display) {
    try {
        const char* bad = whenet::overlay_check(frame, frame_h, frame_w, channel_order, rects, valid, ypr, k, dst);
        WHENET_REQUIRE(bad == nullptr, WHENET_EINVAL, std::string("annotate_host: ") + (bad ? bad : ""));
        WHENET_REQUIRE(dst->on_device == 0, WHENET_EINVAL, "annotate_host: the surface must be host memory (on_device = 0)");
        WHENET_REQUIRE(display == WHENET_DISPLAY_SIMPLE || display == WHENET_DISPLAY_FULL, WHENET_EINVAL,
                       "annotate_host: unknown display " + std::to_string(display) + " (WHENET_DISPLAY_SIMPLE or WHENET_DISPLAY_FULL)");
        whenet::overlay_annotate_host(frame, frame_h, frame_w, channel_order, rects, valid, ypr, k, *dst, display);
        return WHENET_OK;
    } catch (...) {
        return translate_exception(g_create_error);      // (no handle: the text is whenet_last_error(NULL)'s)
    }
}

int whenet_op_annotate(whenet_t* h, const uint8_t* frame, int frame_h, int frame_w, int channel_order, const int32_t* rects,
                       const int32_t* valid, const float* ypr, int k, const whenet_surface_t* dst) {
    return whenet_op_annotate_ex(h, frame, frame_h, frame_w, channel_order, rects, valid, ypr, k, dst, WHENET_DISPLAY_SIMPLE);
}

int whenet_op_annotate_ex(whenet_t* h, const uint8_t* frame, int frame_h, int frame_w, int channel_order, const int32_t* rects,
                          const int32_t* valid, const float* ypr, int k, const whenet_surface_t* dst, int display) {
    return guarded(h, [&](whenet::Engine& e) {
        WHENET_REQUIRE(dst != nullptr, WHENET_EINVAL, "op_annotate: NULL argument");
        e.op_annotate(frame, frame_h, frame_w, channel_order, rects, valid, ypr, k, *dst, display);
    });
}

int whenet_frame_annotate(whenet_t* h, int ticket, int frame_index, const whenet_surface_t* dst, void* stream) {
    return whenet_frame_annotate_ex(h, ticket, frame_index, dst, stream, WHENET_DISPLAY_SIMPLE);
}

int whenet_frame_annotate_ex(whenet_t* h, int ticket, int frame_index, const whenet_surface_t* dst, void* stream, int display) {
    return guarded(h, [&](whenet::Engine&) {
        WHENET_REQUIRE(dst != nullptr, WHENET_EINVAL, "frame_annotate: NULL argument");
        const int idx = ticket % MAX_INFLIGHT_ENGINES;
        WHENET_REQUIRE(ticket >= 0 && idx < h->inflight, WHENET_EINVAL, "frame_annotate: unknown ticket " + std::to_string(ticket));
        h->at(size_t(idx)).frame_annotate(ticket / MAX_INFLIGHT_ENGINES, frame_index, *dst, static_cast<hipStream_t>(stream), display);
    });
}

// ---- JPEG encoder (jpeg.hip, jpeg_host.h, engine_post.cpp) ----
int whenet_jpeg_header(int h, int w, int quality, uint8_t* out, int cap, int32_t qtables[2][64]) {
    return whenet_jpeg_header_ex(h, w, quality, WHENET_JPEG_420, out, cap, qtables);
}

int whenet_jpeg_header_ex(int h, int w, int quality, int sampling, uint8_t* out, int cap, int32_t qtables[2][64]) {
    const char* bad = whenet::jpeg_check_size(h, w, quality);
    if (bad == nullptr && !whenet::jpeg_sampling_ok(sampling)) bad = "unknown sampling (WHENET_JPEG_420, WHENET_JPEG_422 or WHENET_JPEG_444)";
    if (bad == nullptr && out != nullptr && cap < whenet::JPEG_HEADER_BYTES) bad = "the header has 629 bytes, the capacity is below that";
    if (bad != nullptr) {
        g_create_error = std::string("jpeg_header: ") + bad;
        return WHENET_EINVAL;
    }
    whenet::JpegTables t;
    whenet::jpeg_build_tables(h, w, quality, t, sampling);
    if (out) std::memcpy(out, t.header, whenet::JPEG_HEADER_BYTES);
    if (qtables) std::memcpy(qtables, t.q, sizeof(t.q));
    return whenet::JPEG_HEADER_BYTES;
}

int64_t whenet_jpeg_bound(int h, int w) { return whenet_jpeg_bound_ex(h, w, WHENET_JPEG_420); }

int64_t whenet_jpeg_bound_ex(int h, int w, int sampling) {
    const char* bad = whenet::jpeg_check_size(h, w, WHENET_JPEG_DEFAULT_QUALITY);
    if (bad == nullptr && !whenet::jpeg_sampling_ok(sampling)) bad = "unknown sampling (WHENET_JPEG_420, WHENET_JPEG_422 or WHENET_JPEG_444)";
    if (bad != nullptr) {
        g_create_error = std::string("jpeg_bound: ") + bad;
        return WHENET_EINVAL;
    }
    return whenet::jpeg_bound(h, w, sampling);
}

int whenet_jpeg_optimal_table(const uint32_t freq[256], uint8_t bits[16], uint8_t vals[256], int* count) {
    bool any = false;
    for (int i = 0; freq != nullptr && i < 256; ++i) any = any || freq[i] != 0;
    if (freq == nullptr || bits == nullptr || vals == nullptr || count == nullptr || !any) {
        g_create_error = any ? "jpeg_optimal_table: NULL argument" : "jpeg_optimal_table: NULL argument or no symbol occurs";
        return WHENET_EINVAL;
    }
    *count = whenet::jpeg_optimal_table(freq, bits, vals);
    return WHENET_OK;
}

int whenet_jpeg_encode_host(const whenet_surface_t* src, int h, int w, int channel_order, int quality, uint8_t* out, int64_t cap, int64_t* size) {
    return whenet_jpeg_encode_host_ex(src, h, w, channel_order, quality, WHENET_JPEG_420, 0, out, cap, size, nullptr);
}

int whenet_jpeg_encode_host_ex(const whenet_surface_t* src, int h, int w, int channel_order, int quality, int sampling, int optimize, uint8_t* out,
                               int64_t cap, int64_t* size, uint32_t hist[4][256]) {
    try {
        const char* bad = whenet::jpeg_check(src, h, w, channel_order, quality, out, cap, size, sampling);
        WHENET_REQUIRE(bad == nullptr, WHENET_EINVAL, std::string("jpeg_encode_host: ") + (bad ? bad : ""));
        WHENET_REQUIRE(src->on_device == 0, WHENET_EINVAL, "jpeg_encode_host: the surface must be host memory (on_device = 0)");
        std::unique_ptr<whenet::JpegTables> t(new whenet::JpegTables);
        whenet::jpeg_build_tables(h, w, quality, *t, sampling);
        *size = whenet::jpeg_encode_host(whenet::jpeg_source(*src, h, w, channel_order), *t, out, cap, sampling, optimize != 0, hist);
        WHENET_REQUIRE(*size <= cap, WHENET_EOVERFLOW,
                       "jpeg_encode_host: the stream has " + std::to_string(*size) + " bytes, the capacity is " + std::to_string(cap));
        return WHENET_OK;
    } catch (...) {
        return translate_exception(g_create_error);      // (no handle: the text is whenet_last_error(NULL)'s)
    }
}

int whenet_op_jpeg_encode(whenet_t* h, const whenet_surface_t* src, int hh, int ww, int channel_order, int quality, uint8_t* out, int64_t cap,
                          int64_t* size) {
    return whenet_op_jpeg_encode_ex(h, src, hh, ww, channel_order, quality, WHENET_JPEG_420, 0, out, cap, size, nullptr);
}

int whenet_op_jpeg_encode_ex(whenet_t* h, const whenet_surface_t* src, int hh, int ww, int channel_order, int quality, int sampling, int optimize,
                             uint8_t* out, int64_t cap, int64_t* size, uint32_t hist[4][256]) {
    return guarded(h, [&](whenet::Engine& e) {
        WHENET_REQUIRE(src != nullptr, WHENET_EINVAL, "op_jpeg_encode: NULL argument");
        e.op_jpeg_encode(*src, hh, ww, channel_order, quality, out, cap, size, sampling, optimize != 0, hist);
    });
}

int whenet_jpeg_encode_device(whenet_t* h, const whenet_surface_t* src, int hh, int ww, int channel_order, int quality, void* dst, int64_t cap,
                              int64_t* dsize, void* stream) {
    return whenet_jpeg_encode_device_ex(h, src, hh, ww, channel_order, quality, WHENET_JPEG_420, 0, dst, cap, dsize, stream);
}

int whenet_jpeg_encode_device_ex(whenet_t* h, const whenet_surface_t* src, int hh, int ww, int channel_order, int quality, int sampling,
                                 int optimize, void* dst, int64_t cap, int64_t* dsize, void* stream) {
    return guarded(h, [&](whenet::Engine& e) {
        WHENET_REQUIRE(src != nullptr, WHENET_EINVAL, "jpeg_encode_device: NULL argument");
        e.jpeg_encode_device(*src, hh, ww, channel_order, quality, dst, cap, dsize, static_cast<hipStream_t>(stream), sampling, optimize != 0);
    });
}

int whenet_frame_annotate_jpeg(whenet_t* h, int ticket, int frame_index, int display, int quality, uint8_t* out, int64_t cap, int64_t* size,
                               int32_t* status) {
    return whenet_frame_annotate_jpeg_ex(h, ticket, frame_index, display, quality, WHENET_JPEG_420, 0, out, cap, size, status);
}

int whenet_frame_annotate_jpeg_ex(whenet_t* h, int ticket, int frame_index, int display, int quality, int sampling, int optimize, uint8_t* out,
                                  int64_t cap, int64_t* size, int32_t* status) {
    return guarded(h, [&](whenet::Engine&) {
        const int idx = ticket % MAX_INFLIGHT_ENGINES;
        WHENET_REQUIRE(ticket >= 0 && idx < h->inflight, WHENET_EINVAL, "frame_annotate_jpeg: unknown ticket " + std::to_string(ticket));
        h->at(size_t(idx)).frame_annotate_jpeg(ticket / MAX_INFLIGHT_ENGINES, frame_index, display, quality, out, cap, size, status, sampling,
                                               optimize != 0);
    });
}

// ---- JPEG decoder (jpeg_dec.hip, jpeg_dec_host.h, engine_post.cpp) ----
int whenet_jpeg_parse(const uint8_t* data, int64_t size, whenet_jpeg_info_t* info) {
    return host_statement([&] {
        WHENET_REQUIRE(info != nullptr, WHENET_EINVAL, "jpeg_parse: NULL argument");
        jpeg_parse_or_refuse("jpeg_parse", data, size, *info);
    });
}

int whenet_jpeg_decode_host(const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int32_t status[2]) {
    return decode_host_as("jpeg_decode_host", data, size, dst, channel_order, whenet::JPEG_RULE_OWN, status);
}

int whenet_jpeg_decode_planes_host(const uint8_t* data, int64_t size, uint8_t* const* planes, const int* pitch, int32_t status[2]) {
    return host_statement([&] {
        WHENET_REQUIRE(planes != nullptr && pitch != nullptr && status != nullptr, WHENET_EINVAL, "jpeg_decode_planes_host: NULL argument");
        decode_into_host_planes("jpeg_decode_planes_host", data, size, planes, pitch, nullptr,
                                [&](const whenet_jpeg_info_t& info, whenet::JpegDecPlanes& pl) {
                                    whenet::jpeg_dec_planes_host(info, data + info.data_offset, int(size - info.data_offset), pl, status);
                                });
    });
}

int whenet_jpeg_decode_segmented_host(const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int seg_bytes, int window,
                                      int32_t status[2], int64_t stats[8]) {
    return decode_segmented_host_as("jpeg_decode_segmented_host", data, size, dst, channel_order, seg_bytes, window, whenet::JPEG_RULE_OWN, status,
                                    stats);
}

int whenet_jpeg_decode_segmented_planes_host(const uint8_t* data, int64_t size, uint8_t* const* planes, const int* pitch, int seg_bytes, int window,
                                             int32_t status[2], int64_t stats[8]) {
    return host_statement([&] {
        WHENET_REQUIRE(planes != nullptr && pitch != nullptr && status != nullptr, WHENET_EINVAL, "jpeg_decode_segmented_planes_host: NULL argument");
        require_seg_args("jpeg_decode_segmented_planes_host", seg_bytes, window);
        decode_into_host_planes("jpeg_decode_segmented_planes_host", data, size, planes, pitch, nullptr,
                                [&](const whenet_jpeg_info_t& info, whenet::JpegDecPlanes& pl) {
                                    whenet::jpeg_dec_planes_seg_host(info, data + info.data_offset, int(size - info.data_offset), seg_bytes, window, pl,
                                                                     status, stats);
                                });
    });
}

int whenet_jpeg_seg_dc_scan_host(const int32_t* diff, int64_t n, int chunk, int32_t* pred) {
    if (n < 0 || chunk < 1 || (n > 0 && (diff == nullptr || pred == nullptr))) {
        g_create_error = "jpeg_seg_dc_scan_host: NULL argument, n < 0 or chunk < 1";
        return WHENET_EINVAL;
    }
    whenet::jpeg_seg_dc_scan_host(diff, n, chunk, pred);
    return WHENET_OK;
}

int whenet_op_jpeg_decode_ex(whenet_t* h, const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int entropy,
                             int seg_bytes, int32_t status[2], int64_t stats[8]) {
    return guarded(h, [&](whenet::Engine& e) {
        WHENET_REQUIRE(dst != nullptr, WHENET_EINVAL, "op_jpeg_decode_ex: NULL argument");
        WHENET_REQUIRE(entropy == 0 || entropy == 1, WHENET_EINVAL, "op_jpeg_decode_ex: entropy must be 0 (an interval per lane) or 1 (segmented)");
        WHENET_REQUIRE(entropy == 0 || whenet::jpeg_seg_bytes_ok(seg_bytes), WHENET_EINVAL,
                       "op_jpeg_decode_ex: seg_bytes must be a power of two in 4..4096");
        e.op_jpeg_decode(data, size, *dst, channel_order, status, entropy, entropy == 1 ? seg_bytes : 0, stats);
    });
}

int whenet_jpeg_decode_counters(whenet_t* h, int64_t out[4]) {
    if (out == nullptr) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine& e) {
        out[0] = out[1] = out[2] = out[3] = 0;
        e.add_jpeg_decode_counters(out);
        for (const whenet::Engine* r : h->replicas) r->add_jpeg_decode_counters(out);
        for (const whenet::Engine* r : h->fan) r->add_jpeg_decode_counters(out);
    });
}

int whenet_op_jpeg_decode(whenet_t* h, const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int32_t status[2]) {
    return guarded(h, [&](whenet::Engine& e) {
        WHENET_REQUIRE(dst != nullptr, WHENET_EINVAL, "op_jpeg_decode: NULL argument");
        e.op_jpeg_decode(data, size, *dst, channel_order, status);
    });
}

int whenet_jpeg_decode_device(whenet_t* h, const whenet_jpeg_info_t* info, const uint8_t* d_entropy, int64_t nbytes, const whenet_surface_t* dst,
                              int channel_order, int32_t* d_status, void* stream) {
    return guarded(h, [&](whenet::Engine& e) {
        WHENET_REQUIRE(info != nullptr && dst != nullptr, WHENET_EINVAL, "jpeg_decode_device: NULL argument");
        e.jpeg_decode_device(*info, d_entropy, nbytes, *dst, channel_order, d_status, static_cast<hipStream_t>(stream));
    });
}

int whenet_frame_begin_jpeg(whenet_t* h, const uint8_t* data, int64_t size, int channel_order, int* ticket, int32_t* status) {
    return begin_on_next_engine(h, ticket, [&](whenet::Engine& e) { return e.frame_begin_jpeg(data, size, channel_order, status); });
}

// ---- clips of JPEG streams ----
static_assert(WHENET_JPEG_CLIP_PLAN_FRAME_WORDS == whenet::JPEG_CLIP_PLAN_FRAME_WORDS &&
                  WHENET_JPEG_CLIP_PLAN_TOTAL_WORDS == whenet::JPEG_CLIP_PLAN_TOTAL_WORDS,
              "the header states the plan's words");
int whenet_clip_begin_jpeg(whenet_t* h, const uint8_t* const* data, const int64_t* size, int num_frames, int channel_order, int* ticket,
                           int32_t* status) {
    return begin_on_next_engine(h, ticket, [&](whenet::Engine& e) { return e.clip_begin_jpeg(data, size, num_frames, channel_order, status); });
}

int whenet_op_jpeg_decode_clip(whenet_t* h, const uint8_t* const* data, const int64_t* size, int num_frames, const whenet_surface_t* dst,
                               int channel_order, int32_t* status, int entropy, int seg_bytes) {
    return guarded(h, [&](whenet::Engine& e) {
        WHENET_REQUIRE(entropy >= -1 && entropy <= 1, WHENET_EINVAL,
                       "op_jpeg_decode_clip: entropy must be -1 (the handle's options), 0 (an interval per lane) or 1 (segmented)");
        WHENET_REQUIRE(entropy != 1 || whenet::jpeg_seg_bytes_ok(seg_bytes), WHENET_EINVAL,
                       "op_jpeg_decode_clip: seg_bytes must be a power of two in 4..4096");
        e.op_jpeg_decode_clip(data, size, num_frames, dst, channel_order, status, entropy, entropy == 1 ? seg_bytes : 0);
    });
}

int whenet_jpeg_clip_plan(const whenet_jpeg_info_t* infos, const int64_t* nbytes, int num_frames, int entropy, int seg_bytes, int64_t* out) {
    const char* bad = nullptr;
    if (infos == nullptr || nbytes == nullptr || out == nullptr) bad = "NULL argument";
    else if (num_frames < 1 || num_frames > whenet::JPEG_CLIP_MAX_FRAMES) bad = "a clip holds 1..16 frames";
    whenet::JpegDecGeom g[whenet::JPEG_CLIP_MAX_FRAMES];
    for (int f = 0; bad == nullptr && f < num_frames; ++f) {
        if ((bad = whenet::jpeg_dec_check_info(infos[f])) != nullptr) {
            g_create_error = "jpeg_clip_plan: frame " + std::to_string(f) + ": info: " + bad;
            return WHENET_EINVAL;
        }
        g[f] = whenet::jpeg_dec_geom(infos[f]);
    }
    whenet::JpegClipPlan plan;
    if (bad == nullptr) bad = whenet::jpeg_clip_plan(g, nbytes, num_frames, entropy, seg_bytes, plan);
    if (bad != nullptr) {
        g_create_error = std::string("jpeg_clip_plan: ") + bad;
        return WHENET_EINVAL;
    }
    whenet::jpeg_clip_plan_words(plan, out);
    return WHENET_OK;
}

int whenet_jpeg_clip_counters(whenet_t* h, int64_t out[4]) {
    if (out == nullptr) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine& e) {
        out[0] = out[1] = out[2] = out[3] = 0;
        e.add_jpeg_clip_counters(out);
        for (const whenet::Engine* r : h->replicas) r->add_jpeg_clip_counters(out);
        for (const whenet::Engine* r : h->fan) r->add_jpeg_clip_counters(out);
    });
}

// ---- the decode rule as an argument (JPEG DECODER, RULE 1): the calls above with `rule` beside their arguments ----
int whenet_jpeg_decode_rule_host(const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int rule, int32_t status[2]) {
    return decode_host_as("jpeg_decode_rule_host", data, size, dst, channel_order, rule, status);
}

int whenet_jpeg_decode_segmented_rule_host(const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int seg_bytes,
                                           int window, int rule, int32_t status[2], int64_t stats[8]) {
    return decode_segmented_host_as("jpeg_decode_segmented_rule_host", data, size, dst, channel_order, seg_bytes, window, rule, status, stats);
}

int whenet_op_jpeg_decode_rule(whenet_t* h, const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int entropy,
                               int seg_bytes, int rule, int32_t status[2], int64_t stats[8]) {
    return guarded(h, [&](whenet::Engine& e) {
        WHENET_REQUIRE(dst != nullptr, WHENET_EINVAL, "op_jpeg_decode_rule: NULL argument");
        WHENET_REQUIRE(entropy >= -1 && entropy <= 1, WHENET_EINVAL,
                       "op_jpeg_decode_rule: entropy must be -1 (the handle's options), 0 (an interval per lane) or 1 (segmented)");
        WHENET_REQUIRE(entropy != 1 || whenet::jpeg_seg_bytes_ok(seg_bytes), WHENET_EINVAL,
                       "op_jpeg_decode_rule: seg_bytes must be a power of two in 4..4096");
        e.op_jpeg_decode(data, size, *dst, channel_order, status, entropy, entropy == 1 ? seg_bytes : 0, stats, rule);
    });
}

int whenet_op_jpeg_decode_clip_rule(whenet_t* h, const uint8_t* const* data, const int64_t* size, int num_frames, const whenet_surface_t* dst,
                                    int channel_order, int32_t* status, int entropy, int seg_bytes, int rule) {
    return guarded(h, [&](whenet::Engine& e) {
        WHENET_REQUIRE(entropy >= -1 && entropy <= 1, WHENET_EINVAL,
                       "op_jpeg_decode_clip_rule: entropy must be -1 (the handle's options), 0 (an interval per lane) or 1 (segmented)");
        WHENET_REQUIRE(entropy != 1 || whenet::jpeg_seg_bytes_ok(seg_bytes), WHENET_EINVAL,
                       "op_jpeg_decode_clip_rule: seg_bytes must be a power of two in 4..4096");
        e.op_jpeg_decode_clip(data, size, num_frames, dst, channel_order, status, entropy, entropy == 1 ? seg_bytes : 0, rule);
    });
}

int whenet_frame_begin_jpeg_rule(whenet_t* h, const uint8_t* data, int64_t size, int channel_order, int rule, int* ticket, int32_t* status) {
    return begin_on_next_engine(h, ticket, [&](whenet::Engine& e) { return e.frame_begin_jpeg(data, size, channel_order, status, rule); });
}

int whenet_clip_begin_jpeg_rule(whenet_t* h, const uint8_t* const* data, const int64_t* size, int num_frames, int channel_order, int rule,
                                int* ticket, int32_t* status) {
    return begin_on_next_engine(h, ticket,
                                [&](whenet::Engine& e) { return e.clip_begin_jpeg(data, size, num_frames, channel_order, status, rule); });
}

// ---- progressive JPEG streams (jpeg_prog.hip, jpeg_prog_host.h) ----
int whenet_jpeg_parse_scans(const uint8_t* data, int64_t size, whenet_jpeg_info_t* info, whenet_jpeg_scan_t* scans, int cap, int* num_scans) {
    return host_statement([&] {
        WHENET_REQUIRE(info != nullptr && num_scans != nullptr && (scans != nullptr || cap == 0) && cap >= 0, WHENET_EINVAL,
                       "jpeg_parse_scans: NULL argument");
        whenet::JpegProgPlan plan;
        jpeg_parse_or_refuse("jpeg_parse_scans", data, size, *info, &plan);
        *num_scans = int(plan.scans.size());
        WHENET_REQUIRE(cap >= *num_scans, WHENET_EINVAL,
                       "jpeg_parse_scans: the stream has " + std::to_string(*num_scans) + " scans, the capacity is " + std::to_string(cap));
        for (size_t i = 0; i < plan.scans.size(); ++i) scans[i] = plan.scans[i];
    });
}

int whenet_jpeg_decode_progressive_host(const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int rule,
                                        int32_t status[2]) {
    return host_statement([&] {
        WHENET_REQUIRE(dst != nullptr && status != nullptr, WHENET_EINVAL, "jpeg_decode_progressive_host: NULL argument");
        whenet::JpegProgPlan plan;
        decode_into_host_surface("jpeg_decode_progressive_host", data, size, dst, channel_order, rule, &plan,
                                 [&](const whenet_jpeg_info_t& info, whenet::JpegDecPlanes& pl) {
                                     whenet::jpeg_prog_decode_planes_host(info, plan, data, size, pl, status, rule);
                                 });
    });
}

int whenet_jpeg_decode_progressive_planes_host(const uint8_t* data, int64_t size, uint8_t* const* planes, const int* pitch, int rule,
                                               int32_t status[2]) {
    return host_statement([&] {
        WHENET_REQUIRE(planes != nullptr && pitch != nullptr && status != nullptr, WHENET_EINVAL, "jpeg_decode_progressive_planes_host: NULL argument");
        WHENET_REQUIRE(whenet::jpeg_rule_ok(rule), WHENET_EINVAL, "jpeg_decode_progressive_planes_host: the rule must be 0 or 1");
        whenet::JpegProgPlan plan;
        decode_into_host_planes("jpeg_decode_progressive_planes_host", data, size, planes, pitch, &plan,
                                [&](const whenet_jpeg_info_t& info, whenet::JpegDecPlanes& pl) {
                                    whenet::jpeg_prog_decode_planes_host(info, plan, data, size, pl, status, rule);
                                });
    });
}

int whenet_jpeg_progressive_coefficients_host(const uint8_t* data, int64_t size, int16_t* coef, int16_t* raw, int64_t cap_blocks,
                                              int64_t counters[8], int32_t status[2]) {
    return host_statement([&] {
        WHENET_REQUIRE(coef != nullptr && status != nullptr, WHENET_EINVAL, "jpeg_progressive_coefficients_host: NULL argument");
        whenet_jpeg_info_t info;
        whenet::JpegProgPlan plan;
        jpeg_parse_or_refuse("jpeg_progressive_coefficients_host", data, size, info, &plan);
        WHENET_REQUIRE(!plan.baseline, WHENET_EINVAL, "jpeg_progressive_coefficients_host: a baseline (SOF0) stream has no scan plan");
        const whenet::JpegDecGeom g = whenet::jpeg_dec_geom(info);
        const int64_t blocks = int64_t(g.mcu_cols) * g.mcu_rows * g.bpm;
        WHENET_REQUIRE(cap_blocks >= blocks, WHENET_EINVAL,
                       "jpeg_progressive_coefficients_host: the stream has " + std::to_string(blocks) + " blocks, the capacity is " +
                           std::to_string(cap_blocks));
        whenet::JpegProgResult r;
        whenet::jpeg_prog_coefficients_host(info, plan, data + plan.data_base, r, status);
        std::memcpy(coef, r.coef.data(), r.coef.size() * sizeof(int16_t));
        if (raw != nullptr) std::memcpy(raw, r.raw.data(), r.raw.size() * sizeof(int16_t));
        if (counters != nullptr)
            for (int i = 0; i < 8; ++i) counters[i] = r.cnt[i];
    });
}

int whenet_op_jpeg_decode_progressive(whenet_t* h, const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int rule,
                                      int32_t status[2], int64_t stats[8]) {
    return guarded(h, [&](whenet::Engine& e) {
        WHENET_REQUIRE(dst != nullptr, WHENET_EINVAL, "op_jpeg_decode_progressive: NULL argument");
        e.op_jpeg_decode(data, size, *dst, channel_order, status, -1, 0, stats, rule, 1);
    });
}

int whenet_frame_begin_jpeg_progressive(whenet_t* h, const uint8_t* data, int64_t size, int channel_order, int rule, int* ticket,
                                        int32_t* status) {
    return begin_on_next_engine(h, ticket, [&](whenet::Engine& e) { return e.frame_begin_jpeg(data, size, channel_order, status, rule, 1); });
}

int whenet_jpeg_progressive_counters(whenet_t* h, int64_t out[4]) {
    if (out == nullptr) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine& e) {
        out[0] = out[1] = out[2] = out[3] = 0;
        e.add_jpeg_progressive_counters(out);
        for (const whenet::Engine* r : h->replicas) r->add_jpeg_progressive_counters(out);
        for (const whenet::Engine* r : h->fan) r->add_jpeg_progressive_counters(out);
    });
}

// ---- progressive streams in clips (jpeg_dec_clip_host.h: jpeg_clip_plan_progressive; jpeg_prog.hip) ----
static_assert(WHENET_JPEG_CLIP_PROG_PLAN_FRAME_WORDS == whenet::JPEG_CLIP_PROG_PLAN_FRAME_WORDS &&
                  WHENET_JPEG_CLIP_PROG_PLAN_TOTAL_WORDS == whenet::JPEG_CLIP_PROG_PLAN_TOTAL_WORDS,
              "the header states the plan's words");
int whenet_op_jpeg_decode_clip_progressive(whenet_t* h, const uint8_t* const* data, const int64_t* size, int num_frames, const whenet_surface_t* dst,
                                           int channel_order, int32_t* status, int entropy, int seg_bytes, int rule) {
    return guarded(h, [&](whenet::Engine& e) {
        WHENET_REQUIRE(entropy >= -1 && entropy <= 1, WHENET_EINVAL,
                       "op_jpeg_decode_clip_progressive: entropy must be -1 (the handle's options), 0 (an interval per lane) or 1 (segmented)");
        WHENET_REQUIRE(entropy != 1 || whenet::jpeg_seg_bytes_ok(seg_bytes), WHENET_EINVAL,
                       "op_jpeg_decode_clip_progressive: seg_bytes must be a power of two in 4..4096");
        e.op_jpeg_decode_clip(data, size, num_frames, dst, channel_order, status, entropy, entropy == 1 ? seg_bytes : 0, rule, 1);
    });
}

int whenet_clip_begin_jpeg_progressive(whenet_t* h, const uint8_t* const* data, const int64_t* size, int num_frames, int channel_order, int rule,
                                       int* ticket, int32_t* status) {
    return begin_on_next_engine(h, ticket,
                                [&](whenet::Engine& e) { return e.clip_begin_jpeg(data, size, num_frames, channel_order, status, rule, 1); });
}

int whenet_jpeg_clip_plan_progressive(const uint8_t* const* data, const int64_t* size, int num_frames, int entropy, int seg_bytes, int64_t* out) {
    try {
        WHENET_REQUIRE(num_frames >= 1 && num_frames <= whenet::JPEG_CLIP_MAX_FRAMES, WHENET_EINVAL,
                       "jpeg_clip_plan_progressive: a clip holds 1..16 frames");
        WHENET_REQUIRE(data != nullptr && size != nullptr && out != nullptr, WHENET_EINVAL, "jpeg_clip_plan_progressive: NULL argument");
        std::vector<whenet::JpegProgPlan> plans(static_cast<size_t>(num_frames));
        const whenet::JpegProgPlan* ptr[whenet::JPEG_CLIP_MAX_FRAMES];
        whenet::JpegDecGeom g[whenet::JPEG_CLIP_MAX_FRAMES];
        int64_t nbytes[whenet::JPEG_CLIP_MAX_FRAMES];
        for (int f = 0; f < num_frames; ++f) {
            whenet_jpeg_info_t info;
            const std::string who = "jpeg_clip_plan_progressive: frame " + std::to_string(f);
            whenet::detail::jpeg_parse_or_refuse(who.c_str(), data[f], size[f], info, &plans[size_t(f)]);
            g[f] = whenet::jpeg_dec_geom(info), nbytes[f] = size[f] - info.data_offset, ptr[f] = &plans[size_t(f)];
        }
        whenet::JpegClipProgPlan plan;
        const char* bad = whenet::jpeg_clip_plan_progressive(g, nbytes, ptr, num_frames, entropy, seg_bytes, plan);
        WHENET_REQUIRE(bad == nullptr, WHENET_EINVAL, std::string("jpeg_clip_plan_progressive: ") + (bad ? bad : ""));
        whenet::jpeg_clip_plan_progressive_words(plan, out);
        return WHENET_OK;
    } catch (...) {
        return translate_exception(g_create_error);
    }
}

// ---- oriented decode (JPEG DECODER, ORIENTATION; jpeg_dec_host.h: jpeg_exif_orientation, jpeg_dec.hip: the oriented frame kernels) ----
int whenet_jpeg_orientation(const uint8_t* data, int64_t size) { return whenet::jpeg_exif_orientation(data, size); }

// ---- default Huffman tables (JPEG DECODER, DEFAULT TABLES; jpeg_dec_host.h: jpeg_add_default_tables) ----
int whenet_jpeg_add_default_tables(const uint8_t* data, int64_t size, uint8_t* out, int64_t capacity, int64_t* out_size) {
    return host_statement([&] {
        WHENET_REQUIRE(data != nullptr && out != nullptr && out_size != nullptr, WHENET_EINVAL, "jpeg_add_default_tables: NULL argument");
        WHENET_REQUIRE(size >= 0 && capacity >= 0 && capacity - whenet::JPEG_DEFAULT_TABLES_MAX >= size, WHENET_EINVAL,
                       "jpeg_add_default_tables: capacity " + std::to_string(capacity) + " is below size + " +
                           std::to_string(whenet::JPEG_DEFAULT_TABLES_MAX) + " = " + std::to_string(size + whenet::JPEG_DEFAULT_TABLES_MAX));
        *out_size = whenet::jpeg_add_default_tables(data, size, out);
    });
}

int whenet_jpeg_decode_oriented_host(const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int rule, int progressive,
                                     int32_t status[2]) {
    return host_statement([&] {
        const std::string what = "jpeg_decode_oriented_host";
        WHENET_REQUIRE(dst != nullptr && status != nullptr, WHENET_EINVAL, what + ": NULL argument");
        WHENET_REQUIRE(progressive == 0 || progressive == 1, WHENET_EINVAL, what + ": progressive must be 0 or 1");
        whenet_jpeg_info_t info;
        whenet::JpegProgPlan plan;
        jpeg_parse_or_refuse(what.c_str(), data, size, info, progressive ? &plan : nullptr);
        const int o = whenet::jpeg_exif_orientation(data, size);
        WHENET_REQUIRE(o <= 1 || (dst->format != WHENET_YUV_I420 && dst->format != WHENET_YUV_NV12), WHENET_EINVAL,
                       what + ": the stream's orientation is " + std::to_string(o) +
                           ": an oriented decode writes packed surfaces only (WHENET_SURF_PACKED)");
        const whenet_jpeg_info_t landed = whenet::jpeg_orient_info(info, o);
        const char* bad = whenet::jpeg_dec_check_dst(landed, dst, channel_order, rule);
        WHENET_REQUIRE(bad == nullptr, WHENET_EINVAL, what + ": " + (bad ? bad : ""));
        WHENET_REQUIRE(dst->on_device == 0, WHENET_EINVAL, what + ": the surface must be host memory (on_device = 0)");
        whenet::JpegDecPlanes planes;
        if (progressive) whenet::jpeg_prog_decode_planes_host(info, plan, data, size, planes, status, rule);
        else whenet::jpeg_dec_planes_host(info, data + info.data_offset, int(size - info.data_offset), planes, status, rule);
        whenet::jpeg_dec_frame_oriented_host(whenet::jpeg_dec_geom(info), planes, *dst, channel_order, rule, o);
    });
}

int whenet_op_jpeg_decode_oriented(whenet_t* h, const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int entropy,
                                   int seg_bytes, int rule, int progressive, int orient, int32_t status[2], int64_t stats[8], int32_t* orientation) {
    return guarded(h, [&](whenet::Engine& e) {
        WHENET_REQUIRE(dst != nullptr, WHENET_EINVAL, "op_jpeg_decode_oriented: NULL argument");
        WHENET_REQUIRE(entropy >= -1 && entropy <= 1, WHENET_EINVAL,
                       "op_jpeg_decode_oriented: entropy must be -1 (the handle's options), 0 (an interval per lane) or 1 (segmented)");
        WHENET_REQUIRE(entropy != 1 || whenet::jpeg_seg_bytes_ok(seg_bytes), WHENET_EINVAL,
                       "op_jpeg_decode_oriented: seg_bytes must be a power of two in 4..4096");
        WHENET_REQUIRE(progressive >= -1 && progressive <= 1, WHENET_EINVAL, "op_jpeg_decode_oriented: progressive must be -1 (the handle's option), 0 or 1");
        int applied = 1;
        e.op_jpeg_decode(data, size, *dst, channel_order, status, entropy, entropy == 1 ? seg_bytes : 0, stats, rule, progressive, orient, &applied);
        if (orientation != nullptr) *orientation = applied;
    });
}

int whenet_op_jpeg_decode_clip_oriented(whenet_t* h, const uint8_t* const* data, const int64_t* size, int num_frames, const whenet_surface_t* dst,
                                        int channel_order, int32_t* status, int entropy, int seg_bytes, int rule, int progressive, int orient,
                                        int32_t* orientation) {
    return guarded(h, [&](whenet::Engine& e) {
        WHENET_REQUIRE(entropy >= -1 && entropy <= 1, WHENET_EINVAL,
                       "op_jpeg_decode_clip_oriented: entropy must be -1 (the handle's options), 0 (an interval per lane) or 1 (segmented)");
        WHENET_REQUIRE(entropy != 1 || whenet::jpeg_seg_bytes_ok(seg_bytes), WHENET_EINVAL,
                       "op_jpeg_decode_clip_oriented: seg_bytes must be a power of two in 4..4096");
        WHENET_REQUIRE(progressive == 0 || progressive == 1, WHENET_EINVAL, "op_jpeg_decode_clip_oriented: progressive must be 0 or 1");
        int applied[whenet::JPEG_CLIP_MAX_FRAMES];
        e.op_jpeg_decode_clip(data, size, num_frames, dst, channel_order, status, entropy, entropy == 1 ? seg_bytes : 0, rule, progressive, orient,
                              applied);
        if (orientation != nullptr) std::copy(applied, applied + num_frames, orientation);
    });
}

int whenet_frame_begin_jpeg_oriented(whenet_t* h, const uint8_t* data, int64_t size, int channel_order, int rule, int progressive, int orient,
                                     int* ticket, int32_t* status, int32_t* orientation) {
    int applied = 1;
    const int rc = begin_on_next_engine(
        h, ticket, [&](whenet::Engine& e) { return e.frame_begin_jpeg(data, size, channel_order, status, rule, progressive == -1 ? -1 : int(progressive != 0), orient, &applied); });
    if (rc == WHENET_OK && orientation != nullptr) *orientation = applied;
    return rc;
}

int whenet_clip_begin_jpeg_oriented(whenet_t* h, const uint8_t* const* data, const int64_t* size, int num_frames, int channel_order, int rule,
                                    int progressive, int orient, int* ticket, int32_t* status, int32_t* orientation) {
    int applied[whenet::JPEG_CLIP_MAX_FRAMES];
    const int rc = begin_on_next_engine(h, ticket, [&](whenet::Engine& e) {
        return e.clip_begin_jpeg(data, size, num_frames, channel_order, status, rule, int(progressive != 0), orient, applied);
    });
    if (rc == WHENET_OK && orientation != nullptr) std::copy(applied, applied + num_frames, orientation);
    return rc;
}

// ---- the accept bits (JPEG DECODER, LAYOUTS): the calls above with one `accept` bit set in the place of `progressive` ----
static_assert(WHENET_JPEG_ACCEPT_PROGRESSIVE == whenet::detail::JPEG_ACCEPT_PROGRESSIVE && WHENET_JPEG_ACCEPT_LAYOUTS == whenet::detail::JPEG_ACCEPT_LAYOUTS,
              "the header states the accept bits");
namespace {
void require_accept(const std::string& what, int accept, bool option_too) {
    WHENET_REQUIRE((option_too && accept == -1) || whenet::detail::jpeg_accept_ok(accept), WHENET_EINVAL,
                   what + (option_too ? ": accept must be -1 (the handle's options) or a set of WHENET_JPEG_ACCEPT_* bits (0..3)"
                                      : ": accept must be a set of WHENET_JPEG_ACCEPT_* bits (0..3)"));
}
// the padded planes of a stream parsed with the accept bits (plan: filled where a bit is set)
void planes_by_accept(const whenet_jpeg_info_t& info, const whenet::JpegProgPlan& plan, int accept, const uint8_t* data, int64_t size,
                      whenet::JpegDecPlanes& pl, int32_t status[2], int rule) {
    if (accept != 0) whenet::jpeg_prog_decode_planes_host(info, plan, data, size, pl, status, rule);
    else whenet::jpeg_dec_planes_host(info, data + info.data_offset, int(size - info.data_offset), pl, status, rule);
}
}  // namespace

int whenet_jpeg_parse_scans_accept(const uint8_t* data, int64_t size, int accept, whenet_jpeg_info_t* info, whenet_jpeg_scan_t* scans, int cap,
                                   int* num_scans) {
    return host_statement([&] {
        const std::string what = "jpeg_parse_scans_accept";
        WHENET_REQUIRE(info != nullptr && num_scans != nullptr && (scans != nullptr || cap == 0) && cap >= 0, WHENET_EINVAL, what + ": NULL argument");
        require_accept(what, accept, false);
        whenet::JpegProgPlan plan;      // (accept = 0: the baseline parser's refusals, and its one scan as the scan parser records it)
        jpeg_parse_or_refuse(what.c_str(), data, size, *info, &plan, (accept & WHENET_JPEG_ACCEPT_LAYOUTS) != 0,
                             (accept & WHENET_JPEG_ACCEPT_PROGRESSIVE) != 0);
        *num_scans = int(plan.scans.size());
        WHENET_REQUIRE(cap >= *num_scans, WHENET_EINVAL,
                       what + ": the stream has " + std::to_string(*num_scans) + " scans, the capacity is " + std::to_string(cap));
        for (size_t i = 0; i < plan.scans.size(); ++i) scans[i] = plan.scans[i];
    });
}

int whenet_jpeg_decode_accept_host(const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int rule, int accept, int orient,
                                   int32_t status[2], int32_t* orientation) {
    return host_statement([&] {
        const std::string what = "jpeg_decode_accept_host";
        WHENET_REQUIRE(dst != nullptr && status != nullptr, WHENET_EINVAL, what + ": NULL argument");
        require_accept(what, accept, false);
        WHENET_REQUIRE(orient == 0 || orient == 1, WHENET_EINVAL, what + ": orient must be 0 (the orientation is ignored) or 1 (it is applied)");
        whenet_jpeg_info_t info;
        whenet::JpegProgPlan plan;
        whenet::detail::jpeg_parse_accept_or_refuse(what.c_str(), data, size, info, plan, accept);
        const int o = orient ? whenet::jpeg_exif_orientation(data, size) : 1;
        WHENET_REQUIRE(o <= 1 || (dst->format != WHENET_YUV_I420 && dst->format != WHENET_YUV_NV12), WHENET_EINVAL,
                       what + ": the stream's orientation is " + std::to_string(o) +
                           ": an oriented decode writes packed surfaces only (WHENET_SURF_PACKED)");
        const whenet_jpeg_info_t landed = whenet::jpeg_orient_info(info, o);
        const char* bad = whenet::jpeg_dec_check_dst(landed, dst, channel_order, rule);
        WHENET_REQUIRE(bad == nullptr, WHENET_EINVAL, what + ": " + (bad ? bad : ""));
        WHENET_REQUIRE(dst->on_device == 0, WHENET_EINVAL, what + ": the surface must be host memory (on_device = 0)");
        whenet::JpegDecPlanes planes;
        planes_by_accept(info, plan, accept, data, size, planes, status, rule);
        whenet::jpeg_dec_frame_oriented_host(whenet::jpeg_dec_geom(info), planes, *dst, channel_order, rule, o);
        if (orientation != nullptr) *orientation = o;
    });
}

int whenet_jpeg_decode_accept_planes_host(const uint8_t* data, int64_t size, uint8_t* const* planes, const int* pitch, int rule, int accept,
                                          int32_t status[2]) {
    return host_statement([&] {
        const std::string what = "jpeg_decode_accept_planes_host";
        WHENET_REQUIRE(planes != nullptr && pitch != nullptr && status != nullptr, WHENET_EINVAL, what + ": NULL argument");
        WHENET_REQUIRE(whenet::jpeg_rule_ok(rule), WHENET_EINVAL, what + ": the rule must be 0 or 1");
        require_accept(what, accept, false);
        whenet::JpegProgPlan plan;
        decode_into_host_planes(
            what, data, size, planes, pitch, accept != 0 ? &plan : nullptr,
            [&](const whenet_jpeg_info_t& info, whenet::JpegDecPlanes& pl) { planes_by_accept(info, plan, accept, data, size, pl, status, rule); },
            (accept & WHENET_JPEG_ACCEPT_LAYOUTS) != 0, (accept & WHENET_JPEG_ACCEPT_PROGRESSIVE) != 0);
    });
}

int whenet_jpeg_decode_segmented_accept_host(const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int seg_bytes,
                                             int window, int rule, int accept, int32_t status[2], int64_t stats[8]) {
    return host_statement([&] {
        const std::string what = "jpeg_decode_segmented_accept_host";
        WHENET_REQUIRE(dst != nullptr && status != nullptr, WHENET_EINVAL, what + ": NULL argument");
        require_seg_args(what, seg_bytes, window);
        // (the segmented form is the baseline decoder's: the PROGRESSIVE bit has nothing to select here)
        WHENET_REQUIRE(accept == 0 || accept == WHENET_JPEG_ACCEPT_LAYOUTS, WHENET_EINVAL, what + ": accept must be 0 or WHENET_JPEG_ACCEPT_LAYOUTS");
        decode_into_host_surface(
            what, data, size, dst, channel_order, rule, nullptr,
            [&](const whenet_jpeg_info_t& info, whenet::JpegDecPlanes& pl) {
                whenet::jpeg_dec_planes_seg_host(info, data + info.data_offset, int(size - info.data_offset), seg_bytes, window, pl, status, stats, rule);
            },
            accept != 0);
    });
}

int whenet_jpeg_decode_segmented_accept_planes_host(const uint8_t* data, int64_t size, uint8_t* const* planes, const int* pitch, int seg_bytes,
                                                    int window, int rule, int accept, int32_t status[2], int64_t stats[8]) {
    return host_statement([&] {
        const std::string what = "jpeg_decode_segmented_accept_planes_host";
        WHENET_REQUIRE(planes != nullptr && pitch != nullptr && status != nullptr, WHENET_EINVAL, what + ": NULL argument");
        WHENET_REQUIRE(whenet::jpeg_rule_ok(rule), WHENET_EINVAL, what + ": the rule must be 0 or 1");
        require_seg_args(what, seg_bytes, window);
        WHENET_REQUIRE(accept == 0 || accept == WHENET_JPEG_ACCEPT_LAYOUTS, WHENET_EINVAL, what + ": accept must be 0 or WHENET_JPEG_ACCEPT_LAYOUTS");
        decode_into_host_planes(
            what, data, size, planes, pitch, nullptr,
            [&](const whenet_jpeg_info_t& info, whenet::JpegDecPlanes& pl) {
                whenet::jpeg_dec_planes_seg_host(info, data + info.data_offset, int(size - info.data_offset), seg_bytes, window, pl, status, stats, rule);
            },
            accept != 0);
    });
}

int whenet_op_jpeg_decode_accept(whenet_t* h, const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int entropy,
                                 int seg_bytes, int rule, int accept, int orient, int32_t status[2], int64_t stats[8], int32_t* orientation) {
    return guarded(h, [&](whenet::Engine& e) {
        const std::string what = "op_jpeg_decode_accept";
        WHENET_REQUIRE(dst != nullptr, WHENET_EINVAL, what + ": NULL argument");
        WHENET_REQUIRE(entropy >= -1 && entropy <= 1, WHENET_EINVAL,
                       what + ": entropy must be -1 (the handle's options), 0 (an interval per lane) or 1 (segmented)");
        WHENET_REQUIRE(entropy != 1 || whenet::jpeg_seg_bytes_ok(seg_bytes), WHENET_EINVAL, what + ": seg_bytes must be a power of two in 4..4096");
        require_accept(what, accept, true);
        int applied = 1;
        e.op_jpeg_decode(data, size, *dst, channel_order, status, entropy, entropy == 1 ? seg_bytes : 0, stats, rule, accept, orient, &applied);
        if (orientation != nullptr) *orientation = applied;
    });
}

int whenet_op_jpeg_decode_clip_accept(whenet_t* h, const uint8_t* const* data, const int64_t* size, int num_frames, const whenet_surface_t* dst,
                                      int channel_order, int32_t* status, int entropy, int seg_bytes, int rule, int accept, int orient,
                                      int32_t* orientation) {
    return guarded(h, [&](whenet::Engine& e) {
        const std::string what = "op_jpeg_decode_clip_accept";
        WHENET_REQUIRE(entropy >= -1 && entropy <= 1, WHENET_EINVAL,
                       what + ": entropy must be -1 (the handle's options), 0 (an interval per lane) or 1 (segmented)");
        WHENET_REQUIRE(entropy != 1 || whenet::jpeg_seg_bytes_ok(seg_bytes), WHENET_EINVAL, what + ": seg_bytes must be a power of two in 4..4096");
        require_accept(what, accept, false);
        int applied[whenet::JPEG_CLIP_MAX_FRAMES];
        e.op_jpeg_decode_clip(data, size, num_frames, dst, channel_order, status, entropy, entropy == 1 ? seg_bytes : 0, rule, accept, orient, applied);
        if (orientation != nullptr) std::copy(applied, applied + num_frames, orientation);
    });
}

int whenet_frame_begin_jpeg_accept(whenet_t* h, const uint8_t* data, int64_t size, int channel_order, int rule, int accept, int orient, int* ticket,
                                   int32_t* status, int32_t* orientation) {
    int applied = 1;
    const int rc = begin_on_next_engine(
        h, ticket, [&](whenet::Engine& e) { return e.frame_begin_jpeg(data, size, channel_order, status, rule, accept, orient, &applied); });
    if (rc == WHENET_OK && orientation != nullptr) *orientation = applied;
    return rc;
}

int whenet_clip_begin_jpeg_accept(whenet_t* h, const uint8_t* const* data, const int64_t* size, int num_frames, int channel_order, int rule,
                                  int accept, int orient, int* ticket, int32_t* status, int32_t* orientation) {
    int applied[whenet::JPEG_CLIP_MAX_FRAMES];
    const int rc = begin_on_next_engine(
        h, ticket, [&](whenet::Engine& e) { return e.clip_begin_jpeg(data, size, num_frames, channel_order, status, rule, accept, orient, applied); });
    if (rc == WHENET_OK && orientation != nullptr) std::copy(applied, applied + num_frames, orientation);
    return rc;
}

int whenet_jpeg_clip_plan_accept(const uint8_t* const* data, const int64_t* size, int num_frames, int entropy, int seg_bytes, int accept,
                                 int64_t* out) {
    try {
        const std::string what = "jpeg_clip_plan_accept";
        WHENET_REQUIRE(num_frames >= 1 && num_frames <= whenet::JPEG_CLIP_MAX_FRAMES, WHENET_EINVAL, what + ": a clip holds 1..16 frames");
        WHENET_REQUIRE(data != nullptr && size != nullptr && out != nullptr, WHENET_EINVAL, what + ": NULL argument");
        require_accept(what, accept, false);
        std::vector<whenet::JpegProgPlan> plans(static_cast<size_t>(num_frames));
        const whenet::JpegProgPlan* ptr[whenet::JPEG_CLIP_MAX_FRAMES];
        whenet::JpegDecGeom g[whenet::JPEG_CLIP_MAX_FRAMES];
        int64_t nbytes[whenet::JPEG_CLIP_MAX_FRAMES];
        for (int f = 0; f < num_frames; ++f) {
            whenet_jpeg_info_t info;
            const std::string who = what + ": frame " + std::to_string(f);
            whenet::detail::jpeg_parse_or_refuse(who.c_str(), data[f], size[f], info, &plans[size_t(f)], (accept & WHENET_JPEG_ACCEPT_LAYOUTS) != 0,
                                                 (accept & WHENET_JPEG_ACCEPT_PROGRESSIVE) != 0);
            g[f] = whenet::jpeg_dec_geom(info), nbytes[f] = size[f] - info.data_offset, ptr[f] = &plans[size_t(f)];
        }
        whenet::JpegClipProgPlan plan;
        const char* bad = whenet::jpeg_clip_plan_progressive(g, nbytes, ptr, num_frames, entropy, seg_bytes, plan);
        WHENET_REQUIRE(bad == nullptr, WHENET_EINVAL, what + ": " + (bad ? bad : ""));
        whenet::jpeg_clip_plan_progressive_words(plan, out);
        return WHENET_OK;
    } catch (...) {
        return translate_exception(g_create_error);
    }
}

int whenet_yolo_eval_mixed(whenet_t* h, const float* const* feats, int num_images, const int* grid_h, const int* grid_w, int num_layers,
                           const float* anchors, int num_anchors, int num_classes, const float* image_shapes, float score_threshold,
                           float iou_threshold, int max_boxes, float* boxes, float* scores, int32_t* classes, int32_t* index,
                           int32_t* counts) {
    return guarded(h, [&](whenet::Engine& e) {
        e.yolo_eval_mixed(feats, num_images, grid_h, grid_w, num_layers, anchors, num_anchors, num_classes, image_shapes, score_threshold,
                          iou_threshold, max_boxes, boxes, scores, classes, index, counts);
    });
}

int whenet_letterbox_cache_stats(whenet_t* h, int32_t out[4]) {
    if (out == nullptr) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine& e) {
        out[0] = out[1] = out[2] = out[3] = 0;
        e.add_letterbox_cache_stats(out);
        for (const whenet::Engine* r : h->replicas) r->add_letterbox_cache_stats(out);
        for (const whenet::Engine* r : h->fan) r->add_letterbox_cache_stats(out);
    });
}

int whenet_op_letterbox_batch(whenet_t* h, const uint8_t* frames, int num_frames, int frame_h, int frame_w, int channel_order, int out_h,
                              int out_w, uint8_t* canvas_u8, float* image_f32) {
    if (channel_order != WHENET_RGB && channel_order != WHENET_BGR) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine& e) {
        e.op_letterbox_batch(frames, num_frames, frame_h, frame_w, channel_order == WHENET_BGR, out_h, out_w, canvas_u8, image_f32);
    });
}

int whenet_yolo_eval_batch(whenet_t* h, const float* const* feats, int num_images, const int* grid_h, const int* grid_w, int num_layers,
                           const float* anchors, int num_anchors, int num_classes, float image_h, float image_w, float score_threshold,
                           float iou_threshold, int max_boxes, float* boxes, float* scores, int32_t* classes, int32_t* index,
                           int32_t* counts) {
    return guarded(h, [&](whenet::Engine& e) {
        e.yolo_eval_batch(feats, num_images, grid_h, grid_w, num_layers, anchors, num_anchors, num_classes, image_h, image_w, score_threshold,
                          iou_threshold, max_boxes, boxes, scores, classes, index, counts);
    });
}

int whenet_op_head_compact(whenet_t* h, const int32_t* valid, const int32_t* count, int num_frames, int slots_per_frame, int max_heads,
                           int32_t* row, int32_t* slot_of_row, int32_t* rows_used, int32_t* overflow) {
    return guarded(h, [&](whenet::Engine& e) {
        e.op_head_compact(valid, count, num_frames, slots_per_frame, max_heads, row, slot_of_row, rows_used, overflow);
    });
}

static_assert(WHENET_CROP_PLAN_INTS == whenet::CROP_PLAN_INTS, "whenet_hip.h and kernels.h disagree on the crop plan size");
int whenet_crop_plan(const int32_t rect[4], int32_t* plan) {
    if (rect == nullptr || plan == nullptr) return WHENET_EINVAL;
    try {
        whenet::build_crop_plan(rect, plan);
        return WHENET_OK;
    } catch (const whenet::Error& e) {
        return e.code;
    } catch (...) {
        return WHENET_ENOMEM;
    }
}

int whenet_collect(whenet_t* h, int ticket, float* ypr, int32_t* argmax, float* logits) {
    return guarded(h, [&](whenet::Engine&) {
        const int idx = ticket % MAX_INFLIGHT_ENGINES;
        WHENET_REQUIRE(ticket >= 0 && idx < h->inflight, WHENET_EINVAL, "unknown ticket " + std::to_string(ticket));
        h->at(size_t(idx)).collect(ticket / MAX_INFLIGHT_ENGINES, ypr, argmax, logits);
    });
}

int whenet_profile(whenet_t* h, const uint8_t* d_crops, int n, int iters, whenet_launch_stat_t* stats, int cap,
                   int* count) {
    return guarded(h, [&](whenet::Engine& e) {
        // one engine, alone on the GPU: per-launch figures comparable with rocprofv3's kernel trace
        // (which serialises concurrent work); with "inflight" > 1 the timed path overlaps such chains
        for (whenet::Engine* r : h->replicas) r->sync();
        const int c = e.profile(d_crops, n, iters, stats, cap);
        if (count) *count = c;
    });
}

int whenet_op_stem(whenet_t* h, const uint8_t* crops, int n, float* out) {
    return guarded(h, [&](whenet::Engine& e) { e.op_stem(crops, n, out); });
}

int whenet_op_block(whenet_t* h, int index, const float* in, int n, float* expand_out, float* dw_out, float* gate,
                    float* out) {
    return guarded(h, [&](whenet::Engine& e) { e.op_block(index, in, n, expand_out, dw_out, gate, out); });
}

int whenet_op_block_range(whenet_t* h, int first, int last, const float* in, int n, float* out) {
    return guarded(h, [&](whenet::Engine& e) { e.op_block_range(first, last, in, n, out); });
}

int whenet_op_head(whenet_t* h, const float* in, int n, float* feat, float* logits, float* ypr, int32_t* argmax) {
    return guarded(h, [&](whenet::Engine& e) { e.op_head(in, n, feat, logits, ypr, argmax); });
}

int whenet_op_decode(whenet_t* h, const float* logits, int n, float* ypr, int32_t* argmax) {
    return guarded(h, [&](whenet::Engine& e) { e.op_decode(logits, n, ypr, argmax); });
}

int whenet_block_spec(int index, int32_t out[8]) {
    if (out == nullptr) return WHENET_EINVAL;
    try {
        const auto blocks = whenet::make_blocks();
        if (index < 1 || index > int(blocks.size())) return WHENET_EINVAL;
        const whenet::BlockSpec& b = blocks[size_t(index - 1)];
        const int32_t v[8] = {b.k, b.s, b.expand, b.cin, b.cout, b.h_in, b.h_out, b.se_reduced()};
        std::memcpy(out, v, sizeof(v));
        return WHENET_OK;
    } catch (...) {
        return WHENET_ENOMEM;
    }
}

int whenet_dw_plan(int dtype, int index, int32_t out[12]) {
    if (out == nullptr || (dtype != WHENET_F32 && dtype != WHENET_F16)) return WHENET_EINVAL;
    try {
        const auto blocks = whenet::make_blocks();
        if (index < 1 || index > int(blocks.size())) return WHENET_EINVAL;
        const whenet::BlockSpec& b = blocks[size_t(index - 1)];
        const whenet::DwPlan p = whenet::plan_dw(dtype, b.k, b.s, b.h_in, b.h_out, b.cexp());
        const int32_t v[12] = {p.threads, p.CV, p.TH, p.NSX, p.tiles_x, p.tiles_y, p.chunks, p.IH, p.IW,
                               int32_t(p.lds_bytes), b.pad_before(), b.cexp()};
        std::memcpy(out, v, sizeof(v));
        return WHENET_OK;
    } catch (...) {
        return WHENET_EINVAL;
    }
}

int whenet_front_plan(int dtype, int index, int32_t out[12]) {
    if (out == nullptr || (dtype != WHENET_F32 && dtype != WHENET_F16)) return WHENET_EINVAL;
    try {
        const auto blocks = whenet::make_blocks();
        if (index < 2 || index > int(blocks.size())) return WHENET_EINVAL;
        const whenet::BlockSpec& b = blocks[size_t(index - 1)];
        const whenet::FrontPlan p = whenet::plan_front(dtype, b.k, b.s, b.h_in, b.h_out, b.cexp());
        const int32_t v[12] = {p.threads, p.CC, p.TH, p.NSX, p.tiles_x, p.tiles_y, p.chunks, p.EH, p.EW,
                               int32_t(p.lds_bytes), p.w_off, b.cexp()};
        std::memcpy(out, v, sizeof(v));
        return WHENET_OK;
    } catch (...) {
        return WHENET_EINVAL;
    }
}

int whenet_front2_static_check(int row, int field, int delta) {
    try {
        return whenet::front2_static_selftest(row, field, delta) == 0 ? WHENET_OK : WHENET_EINVAL;
    } catch (...) {
        return WHENET_EINVAL;
    }
}

int whenet_front_static_check(int row, int field, int delta) {
    try {
        return whenet::front_static_selftest(row, field, delta) == 0 ? WHENET_OK : WHENET_EINVAL;
    } catch (...) {
        return WHENET_EINVAL;
    }
}

int whenet_pw_static_check(int row, int field, int delta) {
    try {
        return whenet::pw_static_selftest(row, field, delta) == 0 ? WHENET_OK : WHENET_EINVAL;
    } catch (...) {
        return WHENET_EINVAL;
    }
}

int whenet_device_alloc(whenet_t* h, size_t nbytes, void** d_ptr) {
    if (d_ptr == nullptr) return WHENET_EINVAL;
    return guarded(h, [&](whenet::Engine& e) { *d_ptr = e.dev_alloc(nbytes); });
}

int whenet_device_free(whenet_t* h, void* d_ptr) {
    return guarded(h, [&](whenet::Engine& e) { e.dev_free(d_ptr); });
}

int whenet_memcpy_h2d(whenet_t* h, void* d_dst, const void* src, size_t nbytes) {
    return guarded(h, [&](whenet::Engine& e) { e.h2d(d_dst, src, nbytes); });
}

int whenet_memcpy_d2h(whenet_t* h, void* dst, const void* d_src, size_t nbytes) {
    return guarded(h, [&](whenet::Engine& e) { e.d2h(dst, d_src, nbytes); });
}

#pragma GCC visibility pop
}  // extern "C"
