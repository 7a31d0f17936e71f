// The LAYOUTS section of the JPEG decoder (include/whenet_hip.h, JPEG DECODER, LAYOUTS) as a stand-alone program for the HOST
// sanitizers: the parsers of csrc/jpeg_dec_host.h and csrc/jpeg_prog_host.h with their `layouts` argument, the geometry at luma
// 1x2 / 4x1 / 4x2, the sequential scan kind of the scan plan (jpeg_seq_item), two-component scans, the segmented form's host emulation
// at up to 10 blocks per MCU and the frame statement of both rules -- what the ..._accept calls run behind the C ABI.  Every argument
// is a file that holds one stream; tests/test_jpeg_layouts_cpu.py writes the streams of tests/jpeg_layout_cases.py.  A stream is read
// into a heap block of exactly its size and decoded into planes and a frame of exactly their sizes, so that a byte fetched or stored
// outside them is a sanitizer report; then every 7th truncation of it and 64 copies with seeded bit flips are parsed and decoded
// the same way.  It needs no GPU and no HIP runtime and is never loaded into Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_layouts_host_check.cpp \
//       -o tools/jpeg_layouts_host_check && tools/jpeg_layouts_host_check stream.jpg ...
//
// Output, one line per file: "<file name> <route> hs vs bpm scans <n> levels <n> status <code> <first bad item> crc <crc32 of rule
// 0's BGR frame> <crc32 of rule 1's> seg <same | n/a>", route = baseline | sequential | progressive; or "<file name> refused
// <reason>" followed by " | without: <the reason without the layouts argument>".  Exit status 0 unless a file cannot be read, the
// segmented emulation of a baseline-route stream differs from the interval form, or a stream is accepted WITHOUT the argument that
// the argument alone should admit.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../headposeestimation-whenet_amd/csrc/jpeg_dec_clip_host.h"

using namespace whenet;

namespace {

uint32_t g_state = 20261021u;
uint32_t rnd() { return g_state = g_state * 1664525u + 1013904223u; }

uint32_t crc32(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return ~c;
}

struct Result {
    const char* why = nullptr;      // refused
    const char* route = "";
    int hs = 0, vs = 0, bpm = 0, scans = 0, levels = 0;
    int32_t status[2] = {0, 0};
    uint32_t crc[2] = {0, 0};
    bool seg_checked = false, seg_same = true;
};

// `size` bytes in an exact-size heap block through the parser and, unless refused, the whole host statement under both rules
Result decode(const uint8_t* src, size_t size, bool segmented) {
    Result r;
    std::unique_ptr<uint8_t[]> d(new uint8_t[size ? size : 1]);
    std::memcpy(d.get(), src, size);
    whenet_jpeg_info_t info;
    JpegProgPlan plan;
    if ((r.why = jpeg_prog_parse(d.get(), int64_t(size), info, plan, true, true)) != nullptr) return r;
    const JpegDecGeom g = jpeg_dec_geom(info);
    r.route = plan.baseline ? "baseline" : (plan.sequential ? "sequential" : "progressive");
    r.hs = g.hs, r.vs = g.vs, r.bpm = g.bpm, r.scans = int(plan.scans.size()), r.levels = plan.levels;
    if ((long long)(g.h) * g.w > (1 << 16)) {
        r.why = "(not decoded here: too many pixels)";
        return r;
    }
    // the clip planner accepts the plan it will be laid out by
    const JpegProgPlan* plans[1] = {&plan};
    const int64_t nbytes[1] = {int64_t(size) - info.data_offset};
    JpegClipProgPlan pp;
    if (const char* bad = jpeg_clip_plan_progressive(&g, nbytes, plans, 1, 2, 128, pp)) {
        std::fprintf(stderr, "the clip planner refuses an accepted stream: %s\n", bad);
        std::exit(1);
    }
    for (int rule = 0; rule < 2; ++rule) {
        JpegDecPlanes planes;
        jpeg_prog_decode_planes_host(info, plan, d.get(), int64_t(size), planes, r.status, rule);
        const size_t bytes = size_t(g.h) * size_t(g.w) * 3;
        std::unique_ptr<uint8_t[]> frame(new uint8_t[bytes]);
        whenet_surface_t dst{};
        dst.plane[0] = frame.get(), dst.pitch[0] = 3 * g.w, dst.format = WHENET_SURF_PACKED;
        jpeg_dec_frame_host(g, planes, dst, WHENET_BGR, rule);
        r.crc[rule] = crc32(frame.get(), bytes);
        if (segmented && plan.baseline && rule == 0) {      // the segmented form's emulation: the same planes and status
            for (const int seg_bytes : {4, 16, 128})
                for (const int window : {1, 3, 256}) {
                    JpegDecPlanes sp;
                    int32_t st[2];
                    int64_t stats[8];
                    jpeg_dec_planes_seg_host(info, d.get() + info.data_offset, int(int64_t(size) - info.data_offset), seg_bytes, window, sp, st, stats, rule);
                    r.seg_checked = true;
                    for (int c = 0; c < g.comps; ++c) r.seg_same = r.seg_same && sp.plane[c] == planes.plane[c];
                    r.seg_same = r.seg_same && st[0] == r.status[0] && st[1] == r.status[1];
                }
        }
    }
    return r;
}

}  // namespace

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        std::FILE* f = std::fopen(argv[a], "rb");
        if (f == nullptr) {
            std::fprintf(stderr, "cannot read %s\n", argv[a]);
            return 2;
        }
        std::vector<uint8_t> data;
        uint8_t buf[4096];
        for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) data.insert(data.end(), buf, buf + n);
        std::fclose(f);
        const std::string path = argv[a];
        const std::string name = path.substr(path.find_last_of('/') + 1);
        const Result r = decode(data.data(), data.size(), true);
        // without the argument: the parsers' texts as they were
        whenet_jpeg_info_t info;
        JpegProgPlan plan;
        const char* without = jpeg_prog_parse(data.data(), int64_t(data.size()), info, plan);
        if (r.why != nullptr && r.route[0] == 0) {
            std::printf("%s refused %s | without: %s\n", name.c_str(), r.why, without ? without : "(accepted)");
        } else {
            std::printf("%s %s %d %d %d scans %d levels %d status %d %d crc %08x %08x seg %s | without: %s\n", name.c_str(), r.route, r.hs, r.vs, r.bpm,
                        r.scans, r.levels, r.status[0], r.status[1], r.crc[0], r.crc[1], r.seg_checked ? (r.seg_same ? "same" : "DIFFERS") : "n/a",
                        without ? without : "(accepted)");
            if (!r.seg_same) return 1;
        }
        for (size_t cut = 0; cut < data.size(); cut += 7) decode(data.data(), cut, false);
        for (int i = 0; i < 64 && !data.empty(); ++i) {
            std::vector<uint8_t> m = data;
            const size_t span = (i & 1) || m.size() < 200 ? m.size() : 200;      // even copies: inside the header
            const int flips = 1 + int(rnd() % 3);
            for (int j = 0; j < flips; ++j) m[rnd() % span] ^= uint8_t(1u << (rnd() % 8));
            decode(m.data(), m.size(), i % 16 == 1);
        }
    }
    return 0;
}
