// jpeg_add_default_tables (csrc/jpeg_dec_host.h -- what whenet_jpeg_add_default_tables runs behind the C ABI) as a stand-alone
// program for the HOST sanitizers.  Every argument is a file that holds one stream -- tests/test_jpeg_default_tables_cpu.py writes the
// streams of tests/jpeg_default_tables_cases.py and their DHT-stripped copies.  A stream is read into a heap block of exactly its
// size and completed into a heap block of exactly size + JPEG_DEFAULT_TABLES_MAX bytes, so that a byte fetched behind the data or
// stored behind the room the contract gives is a sanitizer report; the result goes into an exact-size block of its own and through
// the header parsers of the host decoder (jpeg_parse, jpeg_prog_parse).  The same happens to EVERY truncation of the stream up to
// its entropy data and to 128 copies with seeded bit flips (in the header, and anywhere).  It needs no GPU and no HIP runtime and is
// never loaded into Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_default_tables_host_check.cpp \
//       -o tools/jpeg_default_tables_host_check && tools/jpeg_default_tables_host_check stream.jpg ...
//
// Output, one line per file: "<file name> <size> -> <size of the completed stream> <accepted | refused: reason> crc <crc32 of the
// completed stream>".  Exit status 0 unless a file cannot be read or a result breaks the contract: more than 420 bytes added, a
// result that is neither the input nor the input with one segment inserted, a second pass that changes it again.
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

[[noreturn]] void broken(const char* what, size_t size) {
    std::fprintf(stderr, "contract broken on a stream of %zu bytes: %s\n", size, what);
    std::exit(1);
}

// the call on `size` bytes held in an exact-size heap block -> the completed stream in an exact-size block; *why: the baseline
// parser's reason for the result (nullptr: accepted)
std::vector<uint8_t> complete(const uint8_t* src, size_t size, const char** why) {
    std::unique_ptr<uint8_t[]> d(new uint8_t[size ? size : 1]);
    if (size > 0) std::memcpy(d.get(), src, size);
    std::unique_ptr<uint8_t[]> out(new uint8_t[size + JPEG_DEFAULT_TABLES_MAX]);
    const int64_t n = jpeg_add_default_tables(d.get(), int64_t(size), out.get());
    if (n < int64_t(size) || n > int64_t(size) + JPEG_DEFAULT_TABLES_MAX) broken("the size of the result", size);
    const size_t added = size_t(n) - size;
    if (added == 0) {
        if (std::memcmp(out.get(), d.get(), size) != 0) broken("an unchanged size with changed bytes", size);
    } else {
        // one DHT segment inserted somewhere: the bytes in front of it and behind it are the input's
        size_t at = 0;
        while (at < size && out[at] == d[at]) ++at;
        // (the segment starts with 0xFF 0xC4 as SOS starts with 0xFF: the common prefix may run one byte into it)
        if (at > 0 && !(out[at] == 0xFF && out[at + 1] == 0xC4)) --at;
        if (out[at] != 0xFF || out[at + 1] != 0xC4 || size_t((out[at + 2] << 8) | out[at + 3]) + 2 != added) broken("the inserted segment", size);
        if (std::memcmp(out.get() + at + added, d.get() + at, size - at) != 0) broken("the bytes behind the inserted segment", size);
        if (d[at] != 0xFF || d[at + 1] != 0xDA) broken("the segment does not stand in front of an SOS marker", size);
    }
    std::vector<uint8_t> r(out.get(), out.get() + n);
    std::unique_ptr<uint8_t[]> again(new uint8_t[r.size() + JPEG_DEFAULT_TABLES_MAX]);
    std::unique_ptr<uint8_t[]> exact(new uint8_t[r.size() ? r.size() : 1]);
    if (!r.empty()) std::memcpy(exact.get(), r.data(), r.size());
    if (jpeg_add_default_tables(exact.get(), int64_t(r.size()), again.get()) != n || std::memcmp(again.get(), exact.get(), r.size()) != 0)
        broken("a second pass changes the stream again", size);
    whenet_jpeg_info_t info;
    *why = jpeg_parse(exact.get(), int64_t(r.size()), info);
    JpegProgPlan plan;
    (void)jpeg_prog_parse(exact.get(), int64_t(r.size()), info, plan);
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
        const char* why = nullptr;
        const std::vector<uint8_t> r = complete(data.data(), data.size(), &why);
        std::printf("%s %zu -> %zu %s%s crc %08x\n", name.c_str(), data.size(), r.size(), why ? "refused: " : "accepted", why ? why : "",
                    crc32(r.data(), r.size()));
        // every truncation of the header (and a little of the entropy data behind it)
        whenet_jpeg_info_t info;
        const size_t header = jpeg_parse(r.data(), int64_t(r.size()), info) == nullptr ? size_t(info.data_offset) : data.size();
        for (size_t cut = 0; cut < data.size() && cut < header + 16; ++cut) complete(data.data(), cut, &why);
        // bit flips: even copies inside the header, odd ones anywhere
        for (int i = 0; i < 128 && !data.empty(); ++i) {
            std::vector<uint8_t> m = data;
            const size_t span = (i & 1) || header == 0 || header > m.size() ? m.size() : header;
            const int flips = 1 + int(rnd() % 3);
            for (int j = 0; j < flips; ++j) m[rnd() % span] ^= uint8_t(1u << (rnd() % 8));
            complete(m.data(), m.size(), &why);
        }
    }
    return 0;
}
