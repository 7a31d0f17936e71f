// The host statement of the JPEG encoder (csrc/jpeg_host.h: what whenet_jpeg_encode_host runs behind the C ABI) as a stand-alone
// program for the HOST sanitizers.  It walks the designed cases of tests/jpeg_cases.py -- the sizes 1 x 1 .. 130 x 250, 10 and 129
// intervals, one interval of 17, of 65 and of 512 MCUs, a flat frame, black next to white and a one-pixel checkerboard at quality 100,
// noise at quality 100 (stuffed 0xFF bytes), every quality of the table, I420 / NV12 / packed BGR / RGB sources with pitches above
// their row bytes -- with every plane in its own exact-size heap block and the destination in a heap block of exactly `cap` bytes,
// so that a byte read outside a row's bytes or written beyond out[cap - 1] is a sanitizer report.  Every case is encoded with
// cap = its size, size - 1, the header's length and 0: the size reported is the same each time and the bytes are a prefix of the
// full stream.  A bit writer is where a one-byte overrun hides.  It needs no GPU and no HIP runtime and is never loaded into Python.
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_host_check.cpp \
//       -o tools/jpeg_host_check && tools/jpeg_host_check
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../headposeestimation-whenet_amd/csrc/jpeg_host.h"

using namespace whenet;

namespace {

uint32_t g_state = 20261019u;
uint32_t rnd() { return g_state = g_state * 1664525u + 1013904223u; }

enum Picture { NOISE, FLAT, BLACK_WHITE, CHECKERBOARD, RAMP };

// a frame whose planes are heap blocks of exactly (rows - 1) * pitch + row_bytes bytes
struct Frame {
    std::unique_ptr<uint8_t[]> mem[3];
    whenet_surface_t s{};
    int h, w;
    Frame(int format, int h_, int w_, int extra, Picture pic) : h(h_), w(w_) {
        int rows[3], row_bytes[3];
        const int planes = overlay_surface_planes(format, h, w, rows, row_bytes);
        s.format = format, s.matrix = WHENET_YUV_JFIF, s.on_device = 0;
        for (int p = 0; p < planes; ++p) {
            const int pitch = row_bytes[p] + (rows[p] > 1 ? extra + p : 0);
            const size_t bytes = size_t(rows[p] - 1) * size_t(pitch) + size_t(row_bytes[p]);
            mem[p].reset(new uint8_t[bytes]);
            for (int y = 0; y < rows[p]; ++y)
                for (int x = 0; x < row_bytes[p]; ++x) {
                    int v = 128;
                    const int px = format == WHENET_SURF_PACKED ? x / 3 : x;
                    if (pic == NOISE) v = int(rnd() >> 24);
                    if (pic == RAMP) v = (3 * px + 5 * y) & 255;
                    if (p == 0 && pic == BLACK_WHITE) v = px < w / 2 ? 0 : 255;
                    if (p == 0 && pic == CHECKERBOARD) v = ((px + y) & 1) * 255;
                    mem[p][size_t(y) * size_t(pitch) + size_t(x)] = uint8_t(v);
                }
            s.plane[p] = mem[p].get(), s.pitch[p] = pitch;
        }
    }
};

int g_cases = 0;

bool run(const char* name, int format, int h, int w, int extra, Picture pic, int quality, int channel_order = WHENET_BGR) {
    const Frame f(format, h, w, extra, pic);
    int64_t size = -1;
    if (jpeg_check(&f.s, h, w, channel_order, quality, nullptr, 0, &size) != nullptr) {
        std::printf("%s: refused\n", name);
        return false;
    }
    std::unique_ptr<JpegTables> t(new JpegTables);
    jpeg_build_tables(h, w, quality, *t);
    const JpegSource src = jpeg_source(f.s, h, w, channel_order);
    const int64_t full = jpeg_encode_host(src, *t, nullptr, 0);
    if (full < JPEG_HEADER_BYTES + 2 || full > jpeg_bound(h, w)) {
        std::printf("%s: %lld bytes, the bound is %lld\n", name, (long long)full, (long long)jpeg_bound(h, w));
        return false;
    }
    std::vector<uint8_t> whole(size_t(full), 0);
    if (jpeg_encode_host(src, *t, whole.data(), full) != full || whole[0] != 0xFF || whole[1] != 0xD8 || whole[size_t(full) - 2] != 0xFF ||
        whole[size_t(full) - 1] != 0xD9) {
        std::printf("%s: the stream does not start with SOI and end with EOI\n", name);
        return false;
    }
    const int64_t caps[3] = {full - 1, JPEG_HEADER_BYTES, 0};
    for (const int64_t cap : caps) {
        std::unique_ptr<uint8_t[]> out(new uint8_t[size_t(cap)]);      // exactly cap bytes: out[cap] is the sanitizer's
        if (jpeg_encode_host(src, *t, out.get(), cap) != full || std::memcmp(out.get(), whole.data(), size_t(cap)) != 0) {
            std::printf("%s: cap %lld: another size or other bytes\n", name, (long long)cap);
            return false;
        }
    }
    ++g_cases;
    return true;
}

}  // namespace

int main() {
    bool ok = true;
    const int sizes[][2] = {{1, 1}, {8, 8}, {16, 16}, {17, 17}, {15, 33}, {48, 40}, {160, 16}, {16, 272}, {130, 250}, {16, 1040}, {2064, 16}, {16, 8192}};
    for (const auto& s : sizes) {
        ok = run("noise i420", WHENET_YUV_I420, s[0], s[1], 0, NOISE, 95) && ok;
        ok = run("ramp bgr", WHENET_SURF_PACKED, s[0], s[1], 0, RAMP, 75) && ok;
    }
    ok = run("flat", WHENET_YUV_I420, 32, 48, 0, FLAT, 95) && ok;
    ok = run("black / white", WHENET_YUV_I420, 16, 32, 0, BLACK_WHITE, 100) && ok;
    ok = run("checkerboard", WHENET_YUV_I420, 16, 32, 0, CHECKERBOARD, 95) && ok;
    ok = run("checkerboard", WHENET_YUV_NV12, 16, 32, 0, CHECKERBOARD, 100) && ok;
    ok = run("noise q100", WHENET_SURF_PACKED, 40, 48, 0, NOISE, 100) && ok;
    const int qualities[] = {1, 25, 49, 50, 51, 75, 95, 100};
    for (const int q : qualities) ok = run("quality", WHENET_SURF_PACKED, 40, 48, 0, NOISE, q) && ok;
    ok = run("i420 pitched", WHENET_YUV_I420, 33, 47, 5, NOISE, 75) && ok;
    ok = run("nv12 pitched", WHENET_YUV_NV12, 33, 47, 7, NOISE, 75) && ok;
    ok = run("bgr pitched", WHENET_SURF_PACKED, 33, 47, 6, NOISE, 75, WHENET_BGR) && ok;
    ok = run("rgb pitched", WHENET_SURF_PACKED, 33, 47, 9, NOISE, 75, WHENET_RGB) && ok;
    // the tables: every code word with its extra bits fits the bit writers' 26 bits
    std::unique_ptr<JpegTables> t(new JpegTables);
    jpeg_build_tables(16, 16, 100, *t);
    for (int tb = 0; tb < 4; ++tb)
        for (int sym = 0; sym < 256; ++sym)
            if (t->len[tb][sym] != 0 && t->len[tb][sym] + ((tb & 1) ? (sym & 15) : sym) > JPEG_CODE_MAX_BITS) ok = false;
    std::printf("%s: %d cases\n", ok ? "jpeg_host_check OK" : "jpeg_host_check FAILED", g_cases);
    return ok ? 0 : 1;
}
