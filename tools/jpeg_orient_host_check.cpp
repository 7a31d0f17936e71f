// The EXIF orientation parser and the oriented host statement (csrc/jpeg_dec_host.h: jpeg_exif_orientation,
// jpeg_dec_frame_oriented_host -- what whenet_jpeg_orientation and whenet_jpeg_decode_oriented_host run behind the C ABI) as a
// stand-alone program for the HOST sanitizers.  Every argument is a file that holds one stream -- tests/test_jpeg_orient_cpu.py writes
// one stream per constructed APP1 of tests/jpeg_orient_cases.py and a few tagged pictures.  A stream is read into a heap block of
// exactly its size; the parser then also gets EVERY truncation of it and 96 copies with seeded bit flips (in the header's first bytes,
// where the APP1 lies, and anywhere), each in its own exact-size block, so that a byte fetched behind the data is a sanitizer report.
// The answer must be 1..8 every time.  Then the stream is decoded under both rules into a destination of exactly the ORIENTED size
// (rows * columns * 3 bytes): a byte stored outside it is a report as well.  It needs no GPU and no HIP runtime and is never loaded
// into Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_orient_host_check.cpp \
//       -o tools/jpeg_orient_host_check && tools/jpeg_orient_host_check stream.jpg ...
//
// Output, one line per file: "<file name> orientation <1..8> <rows>x<columns> status <code> <first bad item> crc <crc32 of rule 0's
// oriented BGR frame> <crc32 of rule 1's>", or "<file name> orientation <1..8> refused <reason>".  Exit status 0 unless a file cannot
// be read or an answer lies outside 1..8.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../headposeestimation-whenet_amd/csrc/jpeg_prog_host.h"

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

// the parser on `size` bytes held in an exact-size heap block
int orientation(const uint8_t* src, size_t size) {
    std::unique_ptr<uint8_t[]> d(new uint8_t[size ? size : 1]);
    std::memcpy(d.get(), src, size);
    const int v = jpeg_exif_orientation(d.get(), int64_t(size));
    if (v < 1 || v > 8) {
        std::fprintf(stderr, "an orientation of %d\n", v);
        std::exit(1);
    }
    return v;
}

// the oriented host statement into a frame of exactly the oriented size; false: refused (reason in *why)
bool decode(const uint8_t* src, size_t size, int rule, int32_t status[2], uint32_t* crc, int* rows, int* cols, const char** why) {
    std::unique_ptr<uint8_t[]> d(new uint8_t[size ? size : 1]);
    std::memcpy(d.get(), src, size);
    whenet_jpeg_info_t info;
    JpegProgPlan plan;
    if (const char* bad = jpeg_prog_parse(d.get(), int64_t(size), info, plan)) {
        *why = bad;
        return false;
    }
    const JpegDecGeom g = jpeg_dec_geom(info);
    if ((long long)(g.h) * g.w > (1 << 16)) {
        *why = "(not decoded here: too many pixels)";
        return false;
    }
    const int o = jpeg_exif_orientation(d.get(), int64_t(size));
    *rows = jpeg_orient_h(o, g.h, g.w), *cols = jpeg_orient_w(o, g.h, g.w);
    JpegDecPlanes planes;
    jpeg_prog_decode_planes_host(info, plan, d.get(), int64_t(size), planes, status, rule);
    const size_t bytes = size_t(*rows) * size_t(*cols) * 3;
    std::unique_ptr<uint8_t[]> frame(new uint8_t[bytes]);
    whenet_surface_t dst{};
    dst.plane[0] = frame.get(), dst.pitch[0] = 3 * *cols, dst.format = WHENET_SURF_PACKED;
    jpeg_dec_frame_oriented_host(g, planes, dst, WHENET_BGR, rule, o);
    *crc = crc32(frame.get(), bytes);
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
        const int o = orientation(data.data(), data.size());
        int32_t st0[2] = {0, 0}, st1[2] = {0, 0};
        uint32_t c0 = 0, c1 = 0;
        int rows = 0, cols = 0;
        const char* why = "";
        if (!decode(data.data(), data.size(), JPEG_RULE_OWN, st0, &c0, &rows, &cols, &why)) {
            std::printf("%s orientation %d refused %s\n", name.c_str(), o, why);
        } else {
            decode(data.data(), data.size(), JPEG_RULE_LIBJPEG, st1, &c1, &rows, &cols, &why);
            std::printf("%s orientation %d %dx%d status %d %d crc %08x %08x\n", name.c_str(), o, rows, cols, st0[0], st0[1], c0, c1);
        }
        // every truncation
        for (size_t cut = 0; cut < data.size(); ++cut) orientation(data.data(), cut);
        // bit flips: even copies inside the first 96 bytes (SOI, APP0, the APP1), odd ones anywhere
        for (int i = 0; i < 96 && !data.empty(); ++i) {
            std::vector<uint8_t> m = data;
            const size_t span = (i & 1) || m.size() < 96 ? m.size() : 96;
            const int flips = 1 + int(rnd() % 3);
            for (int j = 0; j < flips; ++j) m[rnd() % span] ^= uint8_t(1u << (rnd() % 8));
            orientation(m.data(), m.size());
            if (i % 8 == 0) decode(m.data(), m.size(), i & 1, st0, &c0, &rows, &cols, &why);      // (a flipped size or tag: the oriented size follows)
        }
    }
    return 0;
}
