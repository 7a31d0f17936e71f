// The samplings and the optimised Huffman tables of the JPEG encoder's host statement (csrc/jpeg_host.h: what
// whenet_jpeg_encode_host_ex and whenet_jpeg_optimal_table run behind the C ABI) as a stand-alone program for the HOST sanitizers.
// It encodes the sizes of tests/jpeg_sampling_cases.py (1 x 1 .. 64 x 48, 8 x 704, 8 x 1040, 8 and 9 rows) with flat, ramp, noise
// and one-pixel-line content at 4:2:0, 4:2:2 and 4:4:4, standard and optimised tables, qualities 30 / 95 / 100, BGR and RGB, the
// pixels in an exact-size heap block and the destination in a heap block of exactly `cap` bytes (cap = the size, size - 1, the
// header's length and 0), and checks that an optimised stream is not longer than the standard one and its header not longer than
// 629 bytes.  Then the table builder alone on a few thousand seeded frequency vectors -- uniform, sparse, skewed to code sizes far
// above 16 and sums far above 2^32 -- with its outputs in exact-size blocks: lengths <= 16, a Kraft sum below 1, every occurring symbol
// listed once.  It needs no GPU and no HIP runtime and is never loaded into Python.
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_opt_host_check.cpp \
//       -o tools/jpeg_opt_host_check && tools/jpeg_opt_host_check
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../headposeestimation-whenet_amd/csrc/jpeg_host.h"

using namespace whenet;

namespace {

uint32_t g_state = 20261020u;
uint32_t rnd() { return g_state = g_state * 1664525u + 1013904223u; }

enum Picture { NOISE, FLAT, RAMP, LINES };

// a packed frame in a heap block of exactly (h - 1) * pitch + 3 w bytes
struct Frame {
    std::unique_ptr<uint8_t[]> mem;
    whenet_surface_t s{};
    Frame(int h, int w, int extra, Picture pic) {
        const int pitch = 3 * w + (h > 1 ? extra : 0);
        mem.reset(new uint8_t[size_t(h - 1) * size_t(pitch) + size_t(3 * w)]);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
                for (int c = 0; c < 3; ++c) {
                    int v = 96;
                    if (pic == NOISE) v = int(rnd() >> 24);
                    if (pic == RAMP) v = (3 * x + 5 * y + 40 * c) & 255;
                    if (pic == LINES && (y % 16 == 3 + 5 * c || x % 16 == 2 + 5 * c)) v = 255;
                    if (pic == LINES && (y % 16 == 3 + 5 * ((c + 1) % 3) || x % 16 == 2 + 5 * ((c + 1) % 3))) v = 0;
                    mem[size_t(y) * size_t(pitch) + size_t(3 * x + c)] = uint8_t(v);
                }
        s.plane[0] = mem.get(), s.pitch[0] = pitch, s.format = WHENET_SURF_PACKED, s.on_device = 0;
    }
};

int g_cases = 0, g_tables = 0;

int header_bytes_of(const std::vector<uint8_t>& d) {
    for (size_t i = 2; i + 1 < d.size(); ++i)
        if (d[i] == 0xFF && d[i + 1] == 0xDA) return int(i) + 14;
    return -1;
}

bool run(const char* name, int h, int w, int extra, Picture pic, int quality, int channel_order, int sampling) {
    const Frame f(h, w, extra, pic);
    int64_t size = -1;
    if (jpeg_check(&f.s, h, w, channel_order, quality, nullptr, 0, &size, sampling) != nullptr) {
        std::printf("%s: refused\n", name);
        return false;
    }
    std::unique_ptr<JpegTables> t(new JpegTables);
    jpeg_build_tables(h, w, quality, *t, sampling);
    const JpegSource src = jpeg_source(f.s, h, w, channel_order);
    int64_t full_of[2] = {0, 0};
    for (int optimize = 0; optimize < 2; ++optimize) {
        std::unique_ptr<uint32_t[]> hist(new uint32_t[4 * 256]);      // exactly the histograms' size
        const auto hist_arg = reinterpret_cast<uint32_t(*)[256]>(hist.get());
        const int64_t full = jpeg_encode_host(src, *t, nullptr, 0, sampling, optimize != 0, hist_arg);
        full_of[optimize] = full;
        if (full < 2 || full > jpeg_bound(h, w, sampling)) {
            std::printf("%s: %lld bytes, the bound is %lld\n", name, (long long)full, (long long)jpeg_bound(h, w, sampling));
            return false;
        }
        std::vector<uint8_t> whole(size_t(full), 0);
        if (jpeg_encode_host(src, *t, whole.data(), full, sampling, optimize != 0, hist_arg) != full || whole[0] != 0xFF || whole[1] != 0xD8 ||
            whole[size_t(full) - 2] != 0xFF || whole[size_t(full) - 1] != 0xD9) {
            std::printf("%s: the stream does not start with SOI and end with EOI\n", name);
            return false;
        }
        const int head = header_bytes_of(whole);
        if (head < 0 || head > JPEG_HEADER_BYTES || (optimize == 0 && head != JPEG_HEADER_BYTES)) {
            std::printf("%s: a header of %d bytes\n", name, head);
            return false;
        }
        const int64_t caps[4] = {full - 1, head, head - 1, 0};
        for (const int64_t cap : caps) {
            std::unique_ptr<uint8_t[]> out(new uint8_t[size_t(cap)]);      // exactly cap bytes: out[cap] is the sanitizer's
            if (jpeg_encode_host(src, *t, out.get(), cap, sampling, optimize != 0, nullptr) != full ||
                std::memcmp(out.get(), whole.data(), size_t(cap)) != 0) {
                std::printf("%s: cap %lld: another size or other bytes\n", name, (long long)cap);
                return false;
            }
        }
    }
    if (full_of[1] > full_of[0]) {
        std::printf("%s: the optimised stream has %lld bytes, the standard one %lld\n", name, (long long)full_of[1], (long long)full_of[0]);
        return false;
    }
    ++g_cases;
    return true;
}

// one frequency vector through the table builder, the outputs in exact-size blocks
bool table(const uint32_t* freq_in) {
    std::unique_ptr<uint32_t[]> freq(new uint32_t[256]);
    std::unique_ptr<uint8_t[]> bits(new uint8_t[16]), vals(new uint8_t[256]);
    std::memcpy(freq.get(), freq_in, 256 * sizeof(uint32_t));
    const int count = jpeg_optimal_table(freq.get(), bits.get(), vals.get());
    int listed = 0, occurring = 0;
    uint64_t kraft = 0;      // in units of 2^-16
    for (int l = 1; l <= 16; ++l) listed += bits[l - 1], kraft += uint64_t(bits[l - 1]) << (16 - l);
    bool seen[256] = {};
    for (int i = 0; i < count; ++i) {
        if (seen[vals[i]] || freq[vals[i]] == 0) return false;
        seen[vals[i]] = true;
    }
    for (int i = 0; i < 256; ++i) occurring += freq[i] != 0;
    std::unique_ptr<uint16_t[]> code(new uint16_t[256]);
    std::unique_ptr<uint8_t[]> len(new uint8_t[256]);
    jpeg_huff_codes(bits.get(), vals.get(), code.get(), len.get());
    for (int i = 0; i < 256; ++i)
        if (len[i] != 0 && code[i] == (1u << len[i]) - 1u) return false;      // no code is all ones
    ++g_tables;
    return count == occurring && listed == count && kraft < (1u << 16);
}

}  // namespace

int main() {
    bool ok = true;
    const int sizes[][2] = {{1, 1}, {8, 8}, {9, 7}, {17, 17}, {33, 18}, {35, 50}, {64, 48}, {8, 704}, {8, 1040}, {8, 24}, {9, 24}};
    const int qualities[] = {30, 95, 100};
    const Picture pictures[] = {NOISE, FLAT, RAMP, LINES};
    int n = 0;
    for (const auto& s : sizes)
        for (int sampling = WHENET_JPEG_420; sampling <= WHENET_JPEG_444; ++sampling)
            for (const int q : qualities)
                for (int order = 0; order < 2; ++order, ++n)
                    ok = run("frame", s[0], s[1], n % 3 == 0 ? 5 : 0, pictures[n % 4], q, order ? WHENET_RGB : WHENET_BGR, sampling) && ok;
    // an unknown sampling and a planar source at another sampling are refused before anything is read
    {
        const Frame f(16, 16, 0, FLAT);
        int64_t size = 0;
        whenet_surface_t planar = f.s;
        planar.format = WHENET_YUV_I420, planar.matrix = WHENET_YUV_JFIF;
        ok = jpeg_check(&f.s, 16, 16, WHENET_BGR, 95, nullptr, 0, &size, 3) != nullptr && ok;
        ok = jpeg_check(&planar, 16, 16, WHENET_BGR, 95, nullptr, 0, &size, WHENET_JPEG_444) != nullptr && ok;
    }
    // the table builder on seeded frequency vectors
    uint32_t freq[256];
    for (int round = 0; round < 4000; ++round) {
        const int kind = round % 5, symbols = 1 + int(rnd() % 256);
        std::memset(freq, 0, sizeof(freq));
        uint64_t a = 1, b = 1;
        for (int i = 0; i < symbols; ++i) {
            const int sym = kind == 4 ? i : int(rnd() >> 24);
            uint32_t v = 1;
            if (kind == 0) v = 1 + rnd() % 3;                               // ties everywhere
            if (kind == 1) v = 1 + rnd() % 100000;
            if (kind == 2) v = 1u << (rnd() % 28);                          // powers of two: a skewed, deep code
            if (kind == 3) v = uint32_t(a > 0x7FFFFFFFu ? 0x7FFFFFFFu : a); // Fibonacci-like until it saturates: sizes far above 16
            if (kind == 4) v = 0xFFFFFF00u + rnd() % 256;                   // every frequency near 2^32: the sums need 40 bits
            freq[sym] = v;
            const uint64_t c = a + b;
            a = b, b = c;
        }
        if (!table(freq)) {
            std::printf("table round %d failed\n", round);
            ok = false;
        }
    }
    std::printf("%s: %d frames, %d tables\n", ok ? "jpeg_opt_host_check OK" : "jpeg_opt_host_check FAILED", g_cases, g_tables);
    return ok ? 0 : 1;
}
