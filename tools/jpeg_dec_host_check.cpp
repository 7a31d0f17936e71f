// The host statement of the JPEG decoder (csrc/jpeg_dec_host.h: what whenet_jpeg_parse / whenet_jpeg_decode_host run behind the C
// ABI, and the bit reader, the block decode and the inverse DCT that the kernels of csrc/jpeg_dec.hip share with it) as a
// stand-alone program for the HOST sanitizers.  Every argument is a file that holds one stream -- tests/test_jpeg_decode_cpu.py
// writes the whole case table of tests/jpeg_decode_cases.py, the damaged and the refused streams included.  A stream is read into a
// heap block of exactly its size and decoded into a frame of exactly h * w * 3 bytes, so that a byte fetched behind the data or
// stored outside the frame is a sanitizer report.  Then the stream is damaged here as well: cut behind every one of its first and
// last 300 entropy bytes (and at 64 places between), and with seeded byte flips, each copy again in its own exact-size block.  A bit
// reader is where a one-byte overrun hides.  Every decode, of a stream and of each cut or flipped copy, is run under RULE 1 (libjpeg's
// inverse DCT, fancy upsampling and colour row) as well: its clamped neighbour indices are where a read outside a plane would hide,
// its 64-bit row pass where a signed overflow would.  It needs no GPU and no HIP runtime and is never loaded into Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_dec_host_check.cpp \
//       -o tools/jpeg_dec_host_check && tools/jpeg_dec_host_check stream.jpg ...
//
// Output, one line per file: "<file name> status <code> <first bad interval> crc <crc32 of the BGR frame> tables <64-bit FNV-1a of the
// stream's JpegDecTables, the bytes the device gets>", or "<file name> refused <reason>"; for a decoded file a second line "rule1:<file name> status <code> <first bad interval> crc <crc32 of rule 1's BGR frame>".
// Exit status 0 unless a file cannot be read, a mutated stream changes what it must not, or the two rules disagree on a status.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../headposeestimation-whenet_amd/csrc/jpeg_dec_host.h"

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

// decode `size` bytes held in a heap block of exactly that size; false: refused (reason)
bool decode(const uint8_t* src, size_t size, int32_t status[2], uint32_t& crc, const char*& reason, whenet_jpeg_info_t& info,
            uint32_t* crc_rule1 = nullptr) {
    std::unique_ptr<uint8_t[]> data(new uint8_t[size ? size : 1]);
    std::memcpy(data.get(), src, size);
    reason = jpeg_parse(data.get(), int64_t(size), info);
    if (reason != nullptr) return false;
    if (jpeg_dec_check_info(info) != nullptr) {
        std::printf("the parser's own info does not pass jpeg_dec_check_info: %s\n", jpeg_dec_check_info(info));
        std::exit(2);
    }
    if (size_t(info.h) * size_t(info.w) > (size_t(1) << 21)) {      // (a flipped size field: parsed, not decoded)
        status[0] = WHENET_OK, status[1] = -1, crc = 0;
        return true;
    }
    JpegDecPlanes planes;
    jpeg_dec_planes_host(info, data.get() + info.data_offset, int(int64_t(size) - info.data_offset), planes, status);
    const size_t fbytes = size_t(info.h) * size_t(info.w) * 3;
    std::unique_ptr<uint8_t[]> frame(new uint8_t[fbytes]);
    whenet_surface_t dst{};
    dst.plane[0] = frame.get(), dst.pitch[0] = 3 * info.w, dst.format = WHENET_SURF_PACKED;
    jpeg_dec_frame_host(jpeg_dec_geom(info), planes, dst, WHENET_BGR);
    crc = crc32(frame.get(), fbytes);
    if (info.components == 3 && info.hs == 2 && info.vs == 2) {      // the plane destinations, pitched, in exact-size blocks
        const int ch = (info.h + 1) >> 1, cw = (info.w + 1) >> 1;
        for (int format : {WHENET_YUV_I420, WHENET_YUV_NV12}) {
            const int pitch[3] = {info.w + 3, format == WHENET_YUV_NV12 ? 2 * cw + 1 : cw + 2, cw + 5};
            const int rows[3] = {info.h, ch, ch}, row_bytes[3] = {info.w, format == WHENET_YUV_NV12 ? 2 * cw : cw, cw};
            std::unique_ptr<uint8_t[]> mem[3];
            whenet_surface_t s{};
            s.format = format, s.matrix = WHENET_YUV_JFIF;
            for (int p = 0; p < (format == WHENET_YUV_NV12 ? 2 : 3); ++p) {
                mem[p].reset(new uint8_t[size_t(rows[p] - 1) * size_t(pitch[p]) + size_t(row_bytes[p])]);
                s.plane[p] = mem[p].get(), s.pitch[p] = pitch[p];
            }
            if (jpeg_dec_check_dst(info, &s, WHENET_BGR) != nullptr) std::exit(3);
            jpeg_dec_frame_host(jpeg_dec_geom(info), planes, s, WHENET_BGR);
            if (jpeg_dec_check_dst(info, &s, WHENET_BGR, JPEG_RULE_LIBJPEG) == nullptr) std::exit(4);      // rule 1: packed only
        }
    }
    {      // rule 1 from the same bytes: the same status words, a frame of its own in an exact-size block, both channel orders
        JpegDecPlanes p1;
        int32_t st1[2] = {0, 0};
        jpeg_dec_planes_host(info, data.get() + info.data_offset, int(int64_t(size) - info.data_offset), p1, st1, JPEG_RULE_LIBJPEG);
        if (st1[0] != status[0] || st1[1] != status[1]) {
            std::printf("rule 1 gives the status %d %d where rule 0 gives %d %d\n", st1[0], st1[1], status[0], status[1]);
            std::exit(5);
        }
        if (jpeg_dec_check_dst(info, &dst, WHENET_BGR, JPEG_RULE_LIBJPEG) != nullptr) std::exit(6);
        for (int order : {WHENET_RGB, WHENET_BGR}) {
            std::unique_ptr<uint8_t[]> f1(new uint8_t[fbytes]);
            whenet_surface_t d1 = dst;
            d1.plane[0] = f1.get();
            jpeg_dec_frame_host(jpeg_dec_geom(info), p1, d1, order, JPEG_RULE_LIBJPEG);
            if (crc_rule1 != nullptr) *crc_rule1 = crc32(f1.get(), fbytes);
        }
    }
    return true;
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
        uint32_t crc = 0;
        const char* reason = nullptr;
        whenet_jpeg_info_t info;
        uint32_t crc1 = 0;
        if (!decode(bytes.data(), bytes.size(), status, crc, reason, info, &crc1)) {
            std::printf("%s refused %s\n", name.c_str(), reason);
            for (size_t cut = 0; cut < bytes.size() && cut < 700; ++cut) {      // a refused header, cut anywhere, stays refused
                int32_t st[2];
                uint32_t c;
                whenet_jpeg_info_t in2;
                if (decode(bytes.data(), cut, st, c, reason, in2)) {
                    std::printf("%s: cut to %zu bytes it is accepted\n", name.c_str(), cut);
                    return 1;
                }
                ++mutated;
            }
            continue;
        }
        std::unique_ptr<JpegDecTables> tables(new JpegDecTables);
        jpeg_dec_build_tables(info, *tables);
        std::printf("%s status %d %d crc %08x tables %016llx\n", name.c_str(), status[0], status[1], crc,
                    (unsigned long long)(fnv1a(tables.get(), sizeof(JpegDecTables))));
        std::printf("rule1:%s status %d %d crc %08x\n", name.c_str(), status[0], status[1], crc1);
        // the same stream cut short: every length of the header is refused, every length of the data decodes to something
        const size_t off = size_t(info.data_offset), n = bytes.size() - off;
        if (size_t(info.h) * size_t(info.w) > 20000) continue;      // (the large streams are decoded once: the walk is quadratic)
        for (size_t cut = 1; cut < off; cut += 1 + off / 200) {
            int32_t st[2];
            uint32_t c;
            whenet_jpeg_info_t in2;
            if (decode(bytes.data(), cut, st, c, reason, in2)) {
                std::printf("%s: cut to %zu header bytes it is accepted\n", name.c_str(), cut);
                return 1;
            }
            ++mutated;
        }
        for (size_t i = 0; i <= n; i += (i < 300 || i + 300 >= n) ? 1 : 1 + n / 64) {
            int32_t st[2];
            uint32_t c;
            whenet_jpeg_info_t in2;
            if (!decode(bytes.data(), off + i, st, c, reason, in2)) {
                std::printf("%s: cut to %zu entropy bytes it is refused: %s\n", name.c_str(), i, reason);
                return 1;
            }
            if (st[0] != WHENET_OK && (st[0] != WHENET_EFORMAT || st[1] < 0 || st[1] >= info.intervals)) {
                std::printf("%s: cut to %zu entropy bytes the status is %d %d\n", name.c_str(), i, st[0], st[1]);
                return 1;
            }
            ++mutated;
        }
        for (int round = 0; round < 200 && n > 0; ++round) {      // byte flips in the entropy data (and a few in the tables)
            std::vector<uint8_t> m = bytes;
            const int flips = 1 + int(rnd() % 4);
            for (int k = 0; k < flips; ++k) {
                const size_t at = (round % 8 == 7) ? rnd() % bytes.size() : off + rnd() % n;
                m[at] = (rnd() & 1) ? uint8_t(rnd()) : uint8_t(m[at] ^ (1u << (rnd() % 8)));
            }
            int32_t st[2];
            uint32_t c;
            whenet_jpeg_info_t in2;
            (void)decode(m.data(), m.size(), st, c, reason, in2);      // refused or decoded: either is fine, a report is not
            ++mutated;
        }
    }
    std::fprintf(stderr, "%d streams, %ld damaged copies: no report\n", argc - 1, mutated);
    return 0;
}
