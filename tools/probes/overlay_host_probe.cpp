// The host statement of the pose overlay (csrc/overlay_host.h: whenet_annotate_host and whenet_overlay_segments behind the C ABI)
// as a stand-alone program for the HOST sanitizers: it walks a case table -- the frame sizes of tests/overlay_cases.py, windows
// inside, across and outside the frame, NaN / Inf angles, invalid heads, 64 and 256 overlapping heads, both channel orders, every
// format and matrix, pitches above the row bytes -- with every plane in its own exact-size heap block, so that a byte read or
// written outside a row's bytes is a sanitizer report.  Every case runs with WHENET_DISPLAY_SIMPLE and with WHENET_DISPLAY_FULL; the
// labels add heads whose lines leave the frame on every side, angles at the edges of the printed range, the label lines of a sweep
// of float32 angles, and the font's compile-time rows against the strokes rastered here, three pixels beyond every glyph's box.
// It needs no GPU and no HIP runtime and is never loaded into Python.
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/probes/overlay_host_probe.cpp \
//       -o tools/probes/overlay_host_probe && tools/probes/overlay_host_probe
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

#include "../../headposeestimation-whenet_amd/csrc/overlay_host.h"

using namespace whenet;

namespace {

uint32_t g_state = 20261019u;
uint32_t rnd() { return g_state = g_state * 1664525u + 1013904223u; }
int rnd_in(int lo, int hi) { return lo + int(rnd() % uint32_t(hi - lo + 1)); }

struct Heads {
    std::vector<int32_t> rects, valid;
    std::vector<float> ypr;
    bool with_valid = false;
    void add(int y0, int x0, int y1, int x1, float y, float p, float r, int v = 1) {
        rects.insert(rects.end(), {y0, x0, y1, x1});
        ypr.insert(ypr.end(), {y, p, r});
        valid.push_back(v);
    }
    int k() const { return int(valid.size()); }
};

long run(const std::vector<uint8_t>& frame, int h, int w, int order, const Heads& heads, int format, int matrix, int extra, int display) {
    int rows[3], row_bytes[3];
    const int planes = overlay_surface_planes(format, h, w, rows, row_bytes);
    std::unique_ptr<uint8_t[]> mem[3];
    whenet_surface_t s{};
    s.format = format, s.matrix = matrix, s.on_device = 0;
    for (int p = 0; p < planes; ++p) {
        s.pitch[p] = row_bytes[p] + extra;
        const size_t bytes = size_t(rows[p] - 1) * s.pitch[p] + row_bytes[p];      // exactly the extent: one byte more is a report
        mem[p].reset(new uint8_t[bytes]);
        for (size_t i = 0; i < bytes; ++i) mem[p][i] = 0x5A;
        s.plane[p] = mem[p].get();
    }
    const char* bad = overlay_check(frame.data(), h, w, order, heads.rects.data(), heads.with_valid ? heads.valid.data() : nullptr,
                                    heads.ypr.data(), heads.k(), &s);
    if (bad) {
        std::printf("unexpected refusal: %s\n", bad);
        std::exit(1);
    }
    overlay_annotate_host(frame.data(), h, w, order, heads.rects.data(), heads.with_valid ? heads.valid.data() : nullptr, heads.ypr.data(),
                          heads.k(), s, display);
    long sum = 0;
    for (int p = 0; p < planes; ++p)
        for (int r = 0; r < rows[p]; ++r) {
            const uint8_t* row = mem[p].get() + size_t(r) * s.pitch[p];
            for (int i = 0; i < row_bytes[p]; ++i) sum += row[i];
            for (int i = row_bytes[p]; r + 1 < rows[p] && i < s.pitch[p]; ++i)
                if (row[i] != 0x5A) {
                    std::printf("pitch padding written: plane %d row %d byte %d\n", p, r, i);
                    std::exit(1);
                }
        }
    return sum;
}

}  // namespace

int main() {
    const int sizes[][2] = {{1, 1}, {1, 2}, {2, 1}, {2, 2}, {3, 5}, {5, 7}, {33, 19}, {64, 48}, {96, 128}};
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    long total = 0;
    int runs = 0;
    for (const auto& hw : sizes) {
        const int h = hw[0], w = hw[1];
        std::vector<uint8_t> frame(size_t(h) * w * 3);
        for (uint8_t& b : frame) b = uint8_t(rnd() >> 24);
        std::vector<Heads> table(10);
        table[1].add(0, 0, h, w, 0, 0, 0);
        table[2].add(h / 4, w / 4, 3 * h / 4 + 1, 3 * w / 4 + 1, 30.5f, -20.25f, 45.f);
        table[3].add(-h, -w, 2 * h, 2 * w, 40, 30, 80);                       // endpoints outside every edge
        table[3].add(h + 40, w + 40, h + 90, w + 120, -40, 30, 20);           // wholly outside
        table[3].add(-4096, -4096, 8192, 8192, 179, 98, -98);                 // the range's corners
        table[4].add(0, 0, h, w, nan, 0, 0);
        table[4].add(0, 0, h, w, 0, inf, -inf);
        table[5].with_valid = true;
        table[5].add(100000, -100000, 7, 7, nan, nan, nan, 0);                // an invalid head's window is never read
        table[5].add(0, 0, 1, 1, 90, -90, 180, 1);
        table[6].add(h / 2, w / 2, h / 2 + 1, w / 2, 10, 20, 30);             // size 0: discs
        for (int i = 0; i < 64; ++i) {
            const int y0 = rnd_in(-4, h), x0 = rnd_in(-4, w);
            table[7].add(y0, x0, y0 + rnd_in(1, h + 5), x0 + rnd_in(1, w + 5), float(rnd_in(-180, 180)), float(rnd_in(-99, 99)), float(rnd_in(-99, 99)));
        }
        table[8].with_valid = true;
        for (int i = 0; i < 256; ++i) {
            const int y0 = rnd_in(-8, h), x0 = rnd_in(-8, w);
            table[8].add(y0, x0, y0 + rnd_in(0, 60), x0 + rnd_in(0, 80), float(rnd_in(-180, 180)) + .5f, float(rnd_in(-99, 99)), float(rnd_in(-99, 99)),
                         rnd() % 10 != 0);
        }
        table[9].add(3, -30, h, w, -179.6f, 9999.4f, -9999.4f);                // lines off the top and the left edge, 14 characters
        table[9].add(h - 1, w - 3, h + 20, w + 40, -0.3f, 2.5f, 99.49999f);    // ... off the right edge
        table[9].add(h + 5, 0, h + 9, 4, 1, 2, 3);                            // ... the yaw line below the frame
        table[9].add(0, 0, h, w, 9999.5f, 0, 0);                              // a rounded angle of 10000: no line
        table[9].add(-4096, -4096, 8192, 8192, 1, 2, 3);
        table[9].add(8192, 8192, 8192, 8192, 1, 2, 3);
        for (size_t c = 0; c < table.size(); ++c)
            for (int format : {WHENET_SURF_PACKED, WHENET_YUV_NV12, WHENET_YUV_I420})
                for (int matrix = 0; matrix < WHENET_YUV_MATRICES; ++matrix) {
                    if (format == WHENET_SURF_PACKED && matrix > 0) continue;
                    const int extras[4] = {0, 1, 5, 64};
                    for (int display : {WHENET_DISPLAY_SIMPLE, WHENET_DISPLAY_FULL}) {
                        total += run(frame, h, w, (int(c) + matrix) & 1 ? WHENET_RGB : WHENET_BGR, table[c], format, matrix,
                                     extras[(c + size_t(matrix)) & 3], display);
                        ++runs;
                    }
                }
    }
    // the segments alone, at the corners of their range and on angles of every kind
    int32_t seg[OVERLAY_SEG_INTS];
    const float angles[] = {0.f, 90.f, -90.f, 180.f, -180.f, 1e30f, -1e30f, 3.4e38f, nan, inf, -inf, 1e-40f};
    const int32_t corners[][4] = {{-4096, -4096, 8192, 8192}, {8192, 8192, -4096, -4096}, {0, 0, 0, 0}, {5, 7, 5, 6}};
    for (const auto& rect : corners)
        for (float y : angles)
            for (float p : angles)
                for (float r : angles) total += overlay_segments(rect, 1, double(y), double(p), double(r), seg) + seg[6] + seg[15];
    // the font: the rows built at compile time are the strokes under the thin rule, and no stroke paints outside its glyph's box
    for (int g = 0; g < OVERLAY_GLYPHS; ++g)
        for (int y = OVERLAY_GLYPH_TOP - 3; y < OVERLAY_GLYPH_TOP + OVERLAY_GLYPH_ROWS + 3; ++y)
            for (int x = -3; x < OVERLAY_GLYPH_W + 3; ++x) {
                bool hit = false;
                for (int s = 0; s < OVERLAY_FONT.seg[g][0]; ++s) {
                    const int8_t* e = OVERLAY_FONT.seg[g] + 1 + 4 * s;
                    hit = hit || overlay_hit(e[0], e[1], e[2], e[3], x, y, OVERLAY_REACH_THIN);
                }
                const bool inside = x >= 0 && x < OVERLAY_GLYPH_W && y >= OVERLAY_GLYPH_TOP && y < OVERLAY_GLYPH_TOP + OVERLAY_GLYPH_ROWS;
                const bool row = inside && ((overlay_glyph_row(g, y - OVERLAY_GLYPH_TOP) >> x) & 1u);
                if (hit != row) {
                    std::printf("glyph %d: pixel (%d, %d) is %d by its strokes, %d by its rows\n", g, x, y, int(hit), int(row));
                    return 1;
                }
            }
    // the label lines of a sweep of float32 angles: every eighth up to +-10025, and angles of every kind
    const float kinds[] = {0.f, -0.f, 1e-45f, -1e-45f, 9999.49f, 9999.5f, -9999.5f, 1e30f, -1e30f, 3.4e38f, nan, inf, -inf};
    OverlayLine line{};
    for (int k8 = -80200; k8 <= 80200; ++k8)
        for (int l = 0; l < 3; ++l) {
            const bool ok = overlay_label_line(l, float(k8) / 8.f, line);
            const int n = overlay_line_length(line);
            if (n > OVERLAY_LINE_CHARS || (ok && n < 8) || (!ok && n != 0)) {
                std::printf("label line %d of %g: length %d\n", l, double(k8) / 8, n);
                return 1;
            }
            for (int i = 0; i < n; ++i) total += overlay_line_glyph(line, i) < OVERLAY_GLYPHS ? 1 : 1 << 20;
        }
    for (float a : kinds)
        for (int l = 0; l < 3; ++l) total += overlay_label_line(l, a, line) + overlay_line_length(line);
    std::printf("overlay_host_probe: %d annotate runs, checksum %ld: clean\n", runs, total);
    return 0;
}
