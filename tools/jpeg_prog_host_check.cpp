// The host statement of the progressive JPEG decoder (csrc/jpeg_prog_host.h: what whenet_jpeg_parse_scans and
// whenet_jpeg_decode_progressive_host run behind the C ABI, and the scan decode the kernels of csrc/jpeg_prog.hip share with it) as
// a stand-alone program for the HOST sanitizers.  Every argument is a file that holds one stream -- tests/test_jpeg_prog_cpu.py
// writes the case table of tests/jpeg_prog_cases.py, the damaged and the refused streams included.  A stream is read into a heap
// block of exactly its size and decoded into a frame of exactly h * w * 3 bytes, under both rules, so that a byte fetched behind the
// data or stored outside a record or the frame is a sanitizer report.  Then the stream is damaged here as well: cut at up to 96
// places spread over its length, and with 96 seeded byte flips -- entropy bytes and header bytes alike: a flipped SOS or DHT is a
// script the parser must refuse or a table the decode must survive --, each copy again in its own exact-size block (copies of up
// to 128 x 128 pixels are decoded).  It needs no GPU and no
// HIP runtime and is never loaded into Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_prog_host_check.cpp \
//       -o tools/jpeg_prog_host_check && tools/jpeg_prog_host_check stream.jpg ...
//
// Output, one line per file: "<file name> status <code> <first bad item> crc <crc32 of rule 0's BGR frame> <crc32 of rule 1's> plan
// <64-bit FNV-1a of the scan plan's huff, dev and items, the bytes the device gets>", or "<file name> refused <reason>".  Exit status 0 unless a file cannot be read or the two rules disagree on a status.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../headposeestimation-whenet_amd/csrc/jpeg_prog_host.h"

using namespace whenet;

namespace {

uint32_t g_state = 20261020u;
uint32_t rnd() { return g_state = g_state * 1664525u + 1013904223u; }

uint32_t crc32(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return ~c;
}

uint64_t fnv1a(const void* p, size_t n, uint64_t h = 0xCBF29CE484222325ull) {
    for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const uint8_t*>(p)[i]) * 0x100000001B3ull;
    return h;
}

// one decode of `size` bytes held in an exact-size heap block; false: refused (reason in *why)
// (plan_sum: nullptr, or where the checksum of the scan plan goes)
bool decode(const uint8_t* src, size_t size, int rule, int32_t status[2], uint32_t* crc, const char** why, long long max_pixels = 1 << 20,
            uint64_t* plan_sum = nullptr) {
    std::unique_ptr<uint8_t[]> d(new uint8_t[size ? size : 1]);
    std::memcpy(d.get(), src, size);
    whenet_jpeg_info_t info;
    JpegProgPlan plan;
    if (const char* bad = jpeg_prog_parse(d.get(), int64_t(size), info, plan)) {
        *why = bad;
        return false;
    }
    if (plan_sum != nullptr) {
        *plan_sum = fnv1a(plan.huff.data(), plan.huff.size() * sizeof(JpegDecHuff));
        *plan_sum = fnv1a(plan.dev.data(), plan.dev.size() * sizeof(JpegProgScan), *plan_sum);
        *plan_sum = fnv1a(plan.items.data(), plan.items.size() * sizeof(JpegProgItem), *plan_sum);
    }
    const JpegDecGeom g = jpeg_dec_geom(info);
    if ((long long)(g.h) * g.w > max_pixels) {      // (a large picture, or a flipped size byte: the decode would only take long)
        *why = "(not decoded here: too many pixels)";
        return false;
    }
    JpegDecPlanes planes;
    jpeg_prog_decode_planes_host(info, plan, d.get(), int64_t(size), planes, status, rule);
    std::unique_ptr<uint8_t[]> frame(new uint8_t[size_t(g.h) * g.w * 3]);
    whenet_surface_t dst{};
    dst.plane[0] = frame.get(), dst.pitch[0] = 3 * g.w, dst.format = WHENET_SURF_PACKED;
    jpeg_dec_frame_host(g, planes, dst, WHENET_BGR, rule);
    *crc = crc32(frame.get(), size_t(g.h) * g.w * 3);
    return true;
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
        int32_t st0[2] = {0, 0}, st1[2] = {0, 0};
        uint32_t c0 = 0, c1 = 0;
        const char* why = "";
        uint64_t plan_sum = 0;
        if (!decode(data.data(), data.size(), JPEG_RULE_OWN, st0, &c0, &why, 1 << 20, &plan_sum)) {
            std::printf("%s refused %s\n", name.c_str(), why);
        } else {
            decode(data.data(), data.size(), JPEG_RULE_LIBJPEG, st1, &c1, &why);
            if (st0[0] != st1[0] || st0[1] != st1[1]) {
                std::fprintf(stderr, "%s: the rules disagree on the status\n", name.c_str());
                return 1;
            }
            std::printf("%s status %d %d crc %08x %08x plan %016llx\n", name.c_str(), st0[0], st0[1], c0, c1, (unsigned long long)(plan_sum));
        }
        constexpr long long SMALL = 1 << 14;      // mutated copies are decoded up to 128 x 128 pixels
        // cuts
        const size_t cuts = data.size() < 96 ? data.size() : 96;
        for (size_t i = 0; i < cuts; ++i) decode(data.data(), data.size() * i / cuts, int(i & 1), st0, &c0, &why, SMALL);
        // byte flips
        for (int i = 0; i < 96; ++i) {
            std::vector<uint8_t> m = data;
            const int flips = 1 + int(rnd() % 3);
            for (int j = 0; j < flips; ++j) m[rnd() % m.size()] ^= uint8_t(1u << (rnd() % 8));
            decode(m.data(), m.size(), i & 1, st0, &c0, &why, SMALL);
        }
    }
    return 0;
}
