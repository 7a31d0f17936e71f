// The segmented form of the JPEG decoder's entropy stage (csrc/jpeg_dec_seg_host.h: what whenet_jpeg_decode_segmented_host runs
// behind the C ABI, and the sync states, walks, counts and writes the kernels of csrc/jpeg_dec_seg.hip share with it) as a
// stand-alone program for the HOST sanitizers.  Every argument is a file that holds one stream --
// tests/test_jpeg_decode_seg_cpu.py writes the case table of tests/jpeg_decode_cases.py, the damaged streams included.  A stream is
// read into a heap block of exactly its size and decoded by the host statement (csrc/jpeg_dec_host.h) and by the segmented form at
// seg_bytes 4 and 64 and windows of 2 and 256 segments: the planes and the status must be equal.  Then the stream is damaged here as
// well -- cut at many lengths, and with seeded byte flips -- each copy again in its own exact-size block, and the two forms must
// still agree: a guessed walk starts in the middle of a code word, and a byte fetched behind the data is a sanitizer report.  It
// needs no GPU and no HIP runtime and is never loaded into Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_dec_seg_host_check.cpp \
//       -o tools/jpeg_dec_seg_host_check && tools/jpeg_dec_seg_host_check stream.jpg ...
//
// Output, one line per file: "<file name> status <code> <first bad interval> segments <at seg_bytes 4> <at 64>", or "<file name>
// refused".  Exit status 0 unless a file cannot be read or the two forms differ.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../headposeestimation-whenet_amd/csrc/jpeg_dec_host.h"
#include "../headposeestimation-whenet_amd/csrc/jpeg_dec_seg_host.h"

using namespace whenet;

namespace {

uint32_t g_state = 20261020u;
uint32_t rnd() { return g_state = g_state * 1664525u + 1013904223u; }

// 0: refused; 1: both forms agree; exits where they differ
int decode(const char* what, const uint8_t* src, size_t size, int32_t status[2], int64_t segments[2]) {
    std::unique_ptr<uint8_t[]> data(new uint8_t[size ? size : 1]);
    std::memcpy(data.get(), src, size);
    whenet_jpeg_info_t info;
    if (jpeg_parse(data.get(), int64_t(size), info) != nullptr) return 0;
    if (size_t(info.h) * size_t(info.w) > (size_t(1) << 21)) return 0;      // (a flipped size field: parsed, not decoded)
    const uint8_t* ent = data.get() + info.data_offset;
    const int n = int(int64_t(size) - info.data_offset);
    JpegDecPlanes want;
    jpeg_dec_planes_host(info, ent, n, want, status);
    int at = 0;
    for (int seg_bytes : {4, 64})
        for (int window : {2, 256}) {
            JpegDecPlanes got;
            int32_t st[2];
            int64_t stats[8];
            jpeg_dec_planes_seg_host(info, ent, n, seg_bytes, window, got, st, stats);
            bool same = st[0] == status[0] && st[1] == status[1];
            for (int c = 0; c < 3; ++c) same = same && got.plane[c] == want.plane[c];
            if (!same) {
                std::printf("%s: seg_bytes %d window %d: status %d %d against %d %d, or other planes\n", what, seg_bytes, window, st[0], st[1], status[0],
                            status[1]);
                std::exit(1);
            }
            if (stats[1] > jpeg_seg_bound(n, jpeg_dec_geom(info).intervals, seg_bytes)) {
                std::printf("%s: seg_bytes %d: %lld segments pass the host's bound\n", what, seg_bytes, (long long)(stats[1]));
                std::exit(1);
            }
            segments[at / 2] = stats[1], ++at;
        }
    return 1;
}

}  // namespace

int main(int argc, char** argv) {
    long mutated = 0;
    for (int a = 1; a < argc; ++a) {
        std::FILE* f = std::fopen(argv[a], "rb");
        if (f == nullptr) {
            std::printf("cannot open %s\n", argv[a]);
            return 1;
        }
        std::vector<uint8_t> bytes;
        uint8_t buf[4096];
        for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) bytes.insert(bytes.end(), buf, buf + n);
        std::fclose(f);
        const std::string path = argv[a];
        const std::string name = path.substr(path.find_last_of('/') + 1);
        int32_t status[2] = {0, 0};
        int64_t segments[2] = {0, 0};
        if (!decode(name.c_str(), bytes.data(), bytes.size(), status, segments)) {
            std::printf("%s refused\n", name.c_str());
            continue;
        }
        std::printf("%s status %d %d segments %lld %lld\n", name.c_str(), status[0], status[1], (long long)(segments[0]), (long long)(segments[1]));
        whenet_jpeg_info_t info;
        (void)jpeg_parse(bytes.data(), int64_t(bytes.size()), info);
        const size_t off = size_t(info.data_offset), n = bytes.size() - off;
        if (size_t(info.h) * size_t(info.w) > 20000) continue;      // (the large streams are decoded once)
        for (size_t i = 0; i <= n; i += (i < 40 || i + 40 >= n) ? 1 : 1 + n / 24) {      // cut short
            int32_t st[2];
            int64_t sg[2];
            const std::string what = name + " cut to " + std::to_string(i) + " entropy bytes";
            (void)decode(what.c_str(), bytes.data(), off + i, st, sg);
            ++mutated;
        }
        for (int round = 0; round < 60 && n > 0; ++round) {      // byte flips in the entropy data (and a few in the tables)
            std::vector<uint8_t> m = bytes;
            const int flips = 1 + int(rnd() % 4);
            for (int k = 0; k < flips; ++k) {
                const size_t at = (round % 8 == 7) ? rnd() % bytes.size() : off + rnd() % n;
                m[at] = (rnd() & 1) ? uint8_t(rnd()) : uint8_t(m[at] ^ (1u << (rnd() % 8)));
            }
            int32_t st[2];
            int64_t sg[2];
            const std::string what = name + " flip round " + std::to_string(round);
            (void)decode(what.c_str(), m.data(), m.size(), st, sg);
            ++mutated;
        }
    }
    std::fprintf(stderr, "%d streams, %ld damaged copies: no report\n", argc - 1, mutated);
    return 0;
}
