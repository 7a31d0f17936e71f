// The plan of a clip of JPEG streams (csrc/jpeg_dec_clip_host.h: what Engine::clip_begin_jpeg, Engine::op_jpeg_decode_clip and
// whenet_jpeg_clip_plan lay their buffers out by) as a stand-alone program for the HOST sanitizers.  Every argument is a file that
// holds one stream -- tests/test_jpeg_clip_cpu.py writes streams of tests/jpeg_decode_cases.py.  The parsed streams are put into
// clips of every length 1..16 (consecutive files, wrapping round), under entropy 0, 1 and 2 and seg_bytes 4, 128 and 4096; for every
// plan the program checks what the kernels rely on -- every region at a multiple of 256, the regions pairwise disjoint and inside
// the total, the zeroed bytes covering start | meta | seg_stats | coef of every frame, a frame's form the one the rule gives it alone,
// a one-frame clip with the region lengths of the single-stream layout -- and then USES the layout as the engine does: a heap block
// of exactly the plan's bytes, every region of every frame filled over its whole length, the entropy bytes copied in and compared,
// the plan written out as whenet_jpeg_clip_plan's words into an exact-size array.  A byte outside the block is a sanitizer report.
// It needs no GPU and no HIP runtime and is never loaded into Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_dec_clip_host_check.cpp \
//       -o tools/jpeg_dec_clip_host_check && tools/jpeg_dec_clip_host_check stream.jpg ...
//
// Output: one line "plans <count> frames <count> form0 <count> form1 <count>" on stdout, "no report" on stderr.  Exit status 0
// unless a file cannot be read, a stream is refused or a check fails.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../headposeestimation-whenet_amd/csrc/jpeg_dec_host.h"
#include "../headposeestimation-whenet_amd/csrc/jpeg_dec_clip_host.h"

using namespace whenet;

namespace {

struct Stream {
    std::vector<uint8_t> bytes;
    whenet_jpeg_info_t info;
    JpegDecGeom g;
    int64_t nbytes;
};

[[noreturn]] void fail(const std::string& what) {
    std::fprintf(stderr, "FAILED: %s\n", what.c_str());
    std::exit(1);
}
void require(bool ok, const std::string& what) {
    if (!ok) fail(what);
}

std::vector<JpegClipRegion> regions_of(const JpegClipFrame& q) {
    return {q.tables, q.data, q.start, q.meta, q.seg_stats, q.coef, q.plane[0], q.plane[1], q.plane[2], q.first_seg, q.seg_exit, q.seg_count, q.seg_blk};
}

void check_plan(const std::vector<const Stream*>& clip, int entropy, int seg_bytes, long long counts[4]) {
    const int F = int(clip.size());
    JpegDecGeom g[JPEG_CLIP_MAX_FRAMES];
    int64_t nbytes[JPEG_CLIP_MAX_FRAMES];
    for (int f = 0; f < F; ++f) g[f] = clip[f]->g, nbytes[f] = clip[f]->nbytes;
    JpegClipPlan p;
    const char* bad = jpeg_clip_plan(g, nbytes, F, entropy, seg_bytes, p);
    require(bad == nullptr, std::string("refused: ") + (bad ? bad : ""));
    require(p.frames == F && p.forms[0] + p.forms[1] == F, "frame counts");
    std::vector<JpegClipRegion> all = {p.records};
    for (int f = 0; f < F; ++f) {
        const JpegClipFrame& q = p.f[f];
        require(q.form == jpeg_dec_form(entropy, nbytes[f], g[f].intervals), "a frame's form is not the one it gets alone");
        require(q.seg_bytes == (q.form == 1 ? seg_bytes : 0) && q.seg_cap == (q.form == 1 ? jpeg_seg_bound(nbytes[f], g[f].intervals, seg_bytes) : 0),
                "segment bound");
        // the lengths of the single-stream layout (csrc/jpeg_dec.hip, JpegDecScratch)
        const size_t blocks = size_t(g[f].mcu_cols) * size_t(g[f].mcu_rows) * size_t(g[f].bpm);
        require(q.tables.len == sizeof(JpegDecTables) && q.data.len == size_t(nbytes[f]) && q.start.len == size_t(g[f].intervals) * 4 &&
                    q.meta.len == 64 && q.seg_stats.len == 64 && q.coef.len == blocks * 128,
                "region lengths");
        for (int c = 0; c < 3; ++c)
            require(q.plane[c].len == (c < g[f].comps ? size_t(g[f].plane_pitch[c]) * size_t(g[f].plane_rows[c]) : 0), "plane length");
        require(q.first_seg.len == (q.form == 1 ? (size_t(g[f].intervals) + 1) * 4 : 0) && q.seg_exit.len == size_t(q.seg_cap) * 8 &&
                    q.seg_count.len == size_t(q.seg_cap) * sizeof(JpegSegCount) && q.seg_blk.len == size_t(q.seg_cap) * 16,
                "segment region lengths");
        require(q.seg_stats.off == q.meta.off + 64, "seg_stats follows meta");
        for (const JpegClipRegion& r : {q.start, q.meta, q.seg_stats, q.coef})
            require(r.off >= p.zero.off && r.off + r.len <= p.zero.off + p.zero.len, "a zeroed region lies outside the zeroed bytes");
        for (const JpegClipRegion& r : {q.tables, q.data}) require(r.off + r.len <= p.upload_bytes, "an uploaded region lies outside the upload");
        for (const JpegClipRegion& r : regions_of(q)) {
            if (r.len == 0) continue;
            require(r.off % 256 == 0 || r.off == q.seg_stats.off, "a region does not start at a multiple of 256");
            all.push_back(r);
        }
    }
    require(p.records.off == 0 && p.records.len == size_t(F) * JPEG_CLIP_RECORD_BYTES && p.zero.off >= p.upload_bytes, "records / zero");
    std::sort(all.begin(), all.end(), [](const JpegClipRegion& a, const JpegClipRegion& b) { return a.off < b.off; });
    for (size_t i = 0; i < all.size(); ++i) {
        require(all[i].off + all[i].len <= p.bytes, "a region ends behind the total");
        if (i > 0) require(all[i - 1].off + all[i - 1].len <= all[i].off, "two regions overlap");
    }
    // the layout in use: an exact-size block
    std::unique_ptr<uint8_t[]> block(new uint8_t[p.bytes]);
    std::memset(block.get() + p.zero.off, 0, p.zero.len);
    std::memset(block.get() + p.records.off, 0x11, p.records.len);
    for (int f = 0; f < F; ++f) {
        const JpegClipFrame& q = p.f[f];
        int tag = 0x20;
        for (const JpegClipRegion& r : regions_of(q))
            if (r.len > 0) std::memset(block.get() + r.off, tag++, r.len);
        jpeg_dec_build_tables(clip[f]->info, *reinterpret_cast<JpegDecTables*>(block.get() + q.tables.off));
        if (q.data.len > 0) std::memcpy(block.get() + q.data.off, clip[f]->bytes.data() + clip[f]->info.data_offset, q.data.len);
    }
    for (int f = 0; f < F; ++f)      // (no later frame's fill reached into an earlier frame's data)
        require(p.f[f].data.len == 0 ||
                    std::memcmp(block.get() + p.f[f].data.off, clip[f]->bytes.data() + clip[f]->info.data_offset, p.f[f].data.len) == 0,
                "the entropy bytes of a frame were overwritten");
    std::unique_ptr<int64_t[]> words(new int64_t[size_t(F) * JPEG_CLIP_PLAN_FRAME_WORDS + JPEG_CLIP_PLAN_TOTAL_WORDS]);
    jpeg_clip_plan_words(p, words.get());
    require(words[size_t(F) * JPEG_CLIP_PLAN_FRAME_WORDS + 5] == int64_t(p.bytes), "the words' total");
    ++counts[0], counts[1] += F, counts[2] += p.forms[0], counts[3] += p.forms[1];
}

}  // namespace

int main(int argc, char** argv) {
    std::vector<Stream> streams;
    for (int i = 1; i < argc; ++i) {
        std::FILE* f = std::fopen(argv[i], "rb");
        if (!f) fail(std::string("cannot read ") + argv[i]);
        Stream s;
        uint8_t buf[4096];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) s.bytes.insert(s.bytes.end(), buf, buf + n);
        std::fclose(f);
        if (jpeg_parse(s.bytes.data(), int64_t(s.bytes.size()), s.info) != nullptr) fail(std::string("refused: ") + argv[i]);
        s.g = jpeg_dec_geom(s.info);
        s.nbytes = int64_t(s.bytes.size()) - s.info.data_offset;
        streams.push_back(std::move(s));
    }
    require(!streams.empty(), "no stream given");
    long long counts[4] = {0, 0, 0, 0};
    for (int F = 1; F <= JPEG_CLIP_MAX_FRAMES; ++F)
        for (size_t first = 0; first < streams.size(); ++first) {
            std::vector<const Stream*> clip;
            for (int f = 0; f < F; ++f) clip.push_back(&streams[(first + size_t(f)) % streams.size()]);
            for (int entropy : {0, 1, 2})
                for (int seg_bytes : {4, 128, 4096}) check_plan(clip, entropy, seg_bytes, counts);
        }
    // refusals
    JpegClipPlan p;
    JpegDecGeom g = streams[0].g;
    int64_t nb = streams[0].nbytes;
    require(jpeg_clip_plan(&g, &nb, 0, 0, 128, p) != nullptr && jpeg_clip_plan(&g, &nb, 17, 0, 128, p) != nullptr &&
                jpeg_clip_plan(&g, &nb, 1, 3, 128, p) != nullptr && jpeg_clip_plan(&g, &nb, 1, 1, 100, p) != nullptr &&
                jpeg_clip_plan(nullptr, &nb, 1, 0, 128, p) != nullptr,
            "a bad argument was accepted");
    std::printf("plans %lld frames %lld form0 %lld form1 %lld\n", counts[0], counts[1], counts[2], counts[3]);
    std::fprintf(stderr, "no report\n");
    return 0;
}
