// The host side of the extended YUV ingest (csrc/yuvx_host.h: the argument checks, the host statement -- the per-pixel function the
// kernels of csrc/yuvx.hip run -- the plane layout of a clip and the tight staging) as a stand-alone program for the HOST sanitizers.
// Every argument is a file that holds one frame as tests/test_yuv_ext_cpu.py writes it: nine int32 (layout, container, shift,
// matrix, h, w, pitch[3]) and then the planes, plane p being exactly (rows - 1) * pitch[p] + row bytes long.  Every plane is read
// into a heap block of exactly that size, the frame is converted into a block of exactly h * w * 3 bytes, and ALL frames are staged
// as one clip (YuvxLayout: a 16-bit frame at an even offset, also behind an odd-sized 8-bit frame) into a block of exactly
// YuvxLayout::end bytes, from where every frame is converted again through a tight descriptor: a byte fetched or stored outside any
// of these is a sanitizer report.  Then every refusal of include/whenet_hip_yuv_ext.h is tried on the first frame.  It needs no GPU
// and no HIP runtime and is never loaded into Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/yuvx_host_check.cpp -o tools/yuvx_host_check \
//       && tools/yuvx_host_check frame0.bin frame1.bin ...
//
// Output: one line per file, "<file name> <h>x<w> crc <crc32 of the BGR frame> staged <crc32 of the frame converted from the staging>
// at <its offset in the staging>", and a last line "refusals <n> ok".  Exit status 0 unless a file cannot be read, a valid frame is
// refused, the two checksums of a frame differ, or a spoiled frame is accepted.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../headposeestimation-whenet_amd/csrc/yuvx_host.h"

using namespace whenet;

namespace {

uint32_t crc32(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return ~c;
}

struct Frame {
    whenet_yuvx_frame_t d{};
    std::unique_ptr<uint8_t[]> plane[3];
};

[[noreturn]] void fail(const std::string& why) {
    std::fprintf(stderr, "%s\n", why.c_str());
    std::exit(1);
}

Frame read_frame(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) fail(std::string("cannot open ") + path);
    int32_t head[9];
    if (std::fread(head, sizeof(int32_t), 9, f) != 9) fail(std::string("short header in ") + path);
    Frame fr;
    fr.d.layout = head[0], fr.d.container = head[1], fr.d.shift = head[2], fr.d.matrix = head[3], fr.d.h = head[4], fr.d.w = head[5];
    if (!yuvx_layout_known(fr.d.layout) || (fr.d.container != 8 && fr.d.container != 16) || fr.d.h < 1 || fr.d.w < 1 || fr.d.h > 8192 ||
        fr.d.w > 8192)
        fail(std::string("not a frame: ") + path);
    for (int p = 0; p < yuvx_plane_count(fr.d.layout); ++p) {
        const int rb = yuvx_plane_row_bytes(fr.d.layout, p, fr.d.w, fr.d.container >> 3), rows = yuvx_plane_rows(fr.d.layout, p, fr.d.h);
        if (head[6 + p] < rb) fail(std::string("pitch below the row in ") + path);
        const size_t n = size_t(rows - 1) * size_t(head[6 + p]) + size_t(rb);
        fr.plane[p].reset(new uint8_t[n]);
        if (std::fread(fr.plane[p].get(), 1, n, f) != n) fail(std::string("short plane in ") + path);
        fr.d.plane[p] = fr.plane[p].get(), fr.d.pitch[p] = head[6 + p];
    }
    std::fclose(f);
    return fr;
}

uint32_t convert(const whenet_yuvx_frame_t& d) {
    const std::string bad = yuvx_check_frame(d, 0);
    if (!bad.empty()) fail("a valid frame is refused: " + bad);
    const size_t n = size_t(d.h) * d.w * 3;
    std::unique_ptr<uint8_t[]> bgr(new uint8_t[n]);
    yuvx_to_bgr_host(d, bgr.get());
    return crc32(bgr.get(), n);
}

int refusals(const whenet_yuvx_frame_t& good) {
    int n = 0;
    auto refused = [&](whenet_yuvx_frame_t d, const char* text) {
        const std::string bad = yuvx_check_frames("check", &d, 1);
        if (bad.find("frame 0") == std::string::npos || bad.find(text) == std::string::npos)
            fail(std::string("not refused as '") + text + "': '" + bad + "'");
        ++n;
    };
    whenet_yuvx_frame_t d = good;
    d.plane[0] = nullptr, refused(d, "plane 0 is NULL");
    d = good, d.pitch[0] = yuvx_plane_row_bytes(d.layout, 0, d.w, d.container >> 3) - 1, refused(d, "pitch");
    for (int v : {2, 5, 7, -1, 17}) d = good, d.layout = v, refused(d, "unknown layout");
    for (int v : {0, 10, 32}) d = good, d.container = v, refused(d, "unknown container");
    for (int v : {-1, 4}) d = good, d.matrix = v, refused(d, "unknown matrix");
    for (int v : {-1, 9}) d = good, d.container = 16, d.shift = v, refused(d, "shift");
    d = good, d.container = 8, d.shift = 1, refused(d, "shift");
    d = good, d.layout = WHENET_YUV_YUYV, d.container = 16, d.shift = 0, refused(d, "packed layout");
    d = good, d.h = 0, refused(d, "sides must be 1..8192");
    d = good, d.w = 8193, refused(d, "sides must be 1..8192");
    if (good.container == 16) {
        d = good, d.plane[0] = good.plane[0] + 1, refused(d, "odd address");
        d = good, d.pitch[0] |= 1, d.pitch[0] += 2, refused(d, "is odd");
    }
    if (yuvx_check_frames("check", nullptr, 1).empty() || yuvx_check_frames("check", &good, 0).empty() ||
        yuvx_check_frames("check", &good, 17).empty())
        fail("a NULL list or a bad frame count is accepted");
    return n + 3;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) fail("usage: yuvx_host_check frame.bin ...");
    if (argc - 1 > YUVX_MAX_FRAMES) fail("at most 16 frames");
    std::vector<Frame> frames;
    std::vector<whenet_yuvx_frame_t> descs;
    for (int i = 1; i < argc; ++i) {
        frames.push_back(read_frame(argv[i]));
        descs.push_back(frames.back().d);
    }
    const int n = int(descs.size());
    const std::string bad = yuvx_check_frames("check", descs.data(), n);
    if (!bad.empty()) fail("a valid clip is refused: " + bad);
    const YuvxLayout lay(descs.data(), n);
    std::unique_ptr<uint8_t[]> stage(new uint8_t[lay.end]);
    for (int f = 0; f < n; ++f) yuvx_stage_planes(descs[f], stage.get() + lay.src[f]);
    for (int f = 0; f < n; ++f) {
        const whenet_yuvx_frame_t& d = descs[f];
        whenet_yuvx_frame_t t = d;             // the frame where the upload form of the kernels reads it: tight, behind one another
        const uint8_t* at = stage.get() + lay.src[f];
        if (d.container == 16 && (lay.src[f] & 1)) fail("a 16-bit frame is staged at an odd offset");
        for (int p = 0; p < yuvx_plane_count(d.layout); ++p) {
            t.plane[p] = at, t.pitch[p] = yuvx_plane_row_bytes(d.layout, p, d.w, d.container >> 3);
            at += size_t(t.pitch[p]) * size_t(yuvx_plane_rows(d.layout, p, d.h));
        }
        if (at != stage.get() + lay.src[f] + yuvx_plane_bytes(d.h, d.w, d.layout, d.container) || at > stage.get() + lay.end)
            fail("the staging layout and the plane sizes disagree");
        const uint32_t a = convert(d), b = convert(t);
        std::printf("%s %dx%d crc %08x staged %08x at %zu\n", argv[1 + f], d.h, d.w, a, b, lay.src[f]);
        if (a != b) fail("the staged frame converts to other bytes");
    }
    std::printf("refusals %d ok\n", refusals(descs[0]));
    return 0;
}
