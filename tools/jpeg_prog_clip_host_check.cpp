// The plan of a clip that may hold progressive JPEG streams (csrc/jpeg_dec_clip_host.h, jpeg_clip_plan_progressive: what
// Engine::clip_begin_jpeg and Engine::op_jpeg_decode_clip lay their buffers out by with progressive = 1, and what
// whenet_jpeg_clip_plan_progressive hands out) as a stand-alone program for the HOST sanitizers.  Every argument is a file that holds
// one stream, baseline or progressive -- tests/test_jpeg_prog_clip_cpu.py writes streams of tests/jpeg_prog_cases.py and
// tests/jpeg_decode_cases.py.  Beside every stream the program makes a copy cut at three quarters of its length and copies with one
// bit flipped in the entropy data (a copy the parser refuses is left out).  The streams are put into clips of 1, 3 and 16 frames
// (consecutive streams, wrapping round, from every start), under entropy 0, 1 and 2.  For every plan it checks what the kernels rely
// on -- every region at a multiple of 256, the regions pairwise disjoint and inside the total, the upload block holding every
// uploaded region, the zeroed block holding meta | raw of a progressive frame and start | meta | seg_stats | coef of a baseline one,
// a clip without a progressive frame equal to jpeg_clip_plan's --, then USES the layout: the upload block is staged into a heap block of
// EXACTLY upload_bytes as the engine stages it, copied into a heap block of exactly the plan's bytes, the zeroed block cleared, and every
// progressive frame decoded the way the clip kernels walk it -- launch L: level L of every frame, workgroup by workgroup of 16 items,
// every pointer taken from the staged block -- and finished; raw, coef and the status must equal jpeg_prog_coefficients_host's.
// A byte outside a block is a sanitizer report.  It needs no GPU and no HIP runtime and is never loaded into Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_prog_clip_host_check.cpp \
//       -o tools/jpeg_prog_clip_host_check && tools/jpeg_prog_clip_host_check stream.jpg ...
//
// Output: one line "plans <count> frames <count> progressive <count> baseline <count> launches <count> variants <count>" on stdout,
// "no report" on stderr.  Exit status 0 unless a file cannot be read, an original stream is refused or a check fails.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../headposeestimation-whenet_amd/csrc/jpeg_dec_host.h"
#include "../headposeestimation-whenet_amd/csrc/jpeg_prog_host.h"
#include "../headposeestimation-whenet_amd/csrc/jpeg_dec_clip_host.h"

using namespace whenet;

namespace {

struct Stream {
    std::vector<uint8_t> bytes;
    whenet_jpeg_info_t info;
    JpegProgPlan plan;
    JpegDecGeom g;
    int64_t nbytes;
    JpegProgResult want;      // progressive: the host statement
    int32_t want_status[2];
};

[[noreturn]] void fail(const std::string& what) {
    std::fprintf(stderr, "FAILED: %s\n", what.c_str());
    std::exit(1);
}
void require(bool ok, const std::string& what) {
    if (!ok) fail(what);
}

bool load(std::vector<uint8_t> bytes, Stream& s) {
    s.bytes = std::move(bytes);
    if (jpeg_prog_parse(s.bytes.data(), int64_t(s.bytes.size()), s.info, s.plan) != nullptr) return false;
    s.g = jpeg_dec_geom(s.info);
    s.nbytes = int64_t(s.bytes.size()) - s.info.data_offset;
    if (!s.plan.baseline) jpeg_prog_coefficients_host(s.info, s.plan, s.bytes.data() + s.plan.data_base, s.want, s.want_status);
    return true;
}

void check_plan(const std::vector<const Stream*>& clip, int entropy, long long counts[5]) {
    const int F = int(clip.size());
    JpegDecGeom g[JPEG_CLIP_MAX_FRAMES];
    int64_t nbytes[JPEG_CLIP_MAX_FRAMES];
    const JpegProgPlan* prog[JPEG_CLIP_MAX_FRAMES];
    for (int f = 0; f < F; ++f) g[f] = clip[f]->g, nbytes[f] = clip[f]->nbytes, prog[f] = &clip[f]->plan;
    JpegClipProgPlan pp;
    const char* bad = jpeg_clip_plan_progressive(g, nbytes, prog, F, entropy, 128, pp);
    require(bad == nullptr, std::string("refused: ") + (bad ? bad : ""));
    const JpegClipPlan& p = pp.base;
    require(p.frames == F && p.forms[0] + p.forms[1] + pp.progressive == F, "frame counts");
    std::vector<JpegClipRegion> all = {p.records};
    int levels = 0;
    for (int f = 0; f < F; ++f) {
        const JpegClipFrame& q = p.f[f];
        const JpegClipProgFrame& r = pp.pf[f];
        const size_t blocks = size_t(g[f].mcu_cols) * size_t(g[f].mcu_rows) * size_t(g[f].bpm);
        const bool is_prog = !clip[f]->plan.baseline;
        require((q.form == JPEG_CLIP_FORM_PROGRESSIVE) == is_prog, "a frame's form");
        std::vector<JpegClipRegion> zeroed, uploaded;
        if (is_prog) {
            const JpegProgPlan& s = clip[f]->plan;
            require(r.scans.len == s.dev.size() * sizeof(JpegProgScan) && r.huff.len == s.huff.size() * sizeof(JpegDecHuff) && r.qz.len == sizeof(s.qz) &&
                        r.items.len == s.items.size() * sizeof(JpegProgItem) && q.data.len == size_t(s.data_bytes) && r.raw.len == blocks * 128 &&
                        q.coef.len == blocks * 128 && q.meta.len == 64 && q.tables.len == 0 && q.start.len == 0 && q.seg_stats.len == 0 &&
                        q.first_seg.len + q.seg_exit.len + q.seg_count.len + q.seg_blk.len == 0 && r.levels == s.levels && r.nscans == int(s.dev.size()),
                    "region lengths of a progressive frame");
            require(r.scans.off < r.huff.off && r.huff.off < r.qz.off && r.qz.off < r.items.off && r.items.off < q.data.off, "scans | huff | qz | items | data");
            require(q.coef.off >= p.zero.off + p.zero.len, "the finished records lie in the work block");
            zeroed = {q.meta, r.raw}, uploaded = {r.scans, r.huff, r.qz, r.items, q.data};
            levels = std::max(levels, s.levels);
        } else {
            require(q.form == jpeg_dec_form(entropy, nbytes[f], g[f].intervals), "a baseline frame's form is not the one it gets alone");
            require(q.tables.len == sizeof(JpegDecTables) && q.data.len == size_t(nbytes[f]) && q.start.len == size_t(g[f].intervals) * 4 &&
                        q.meta.len == 64 && q.seg_stats.len == 64 && q.coef.len == blocks * 128 &&
                        r.scans.len + r.huff.len + r.qz.len + r.items.len + r.raw.len == 0,
                    "region lengths of a baseline frame");
            zeroed = {q.start, q.meta, q.seg_stats, q.coef}, uploaded = {q.tables, q.data};
        }
        for (const JpegClipRegion& z : zeroed) require(z.off >= p.zero.off && z.off + z.len <= p.zero.off + p.zero.len, "a zeroed region lies outside the zeroed block");
        for (const JpegClipRegion& u : uploaded) require(u.off >= p.records.len && u.off + u.len <= p.upload_bytes, "an uploaded region lies outside the upload block");
        for (const JpegClipRegion& x : {q.tables, q.data, q.start, q.meta, q.seg_stats, q.coef, q.plane[0], q.plane[1], q.plane[2], q.first_seg, q.seg_exit,
                                        q.seg_count, q.seg_blk, r.scans, r.huff, r.qz, r.items, r.raw}) {
            if (x.len == 0) continue;
            require(x.off % 256 == 0 || (x.off == q.seg_stats.off && x.off == q.meta.off + 64), "a region does not start at a multiple of 256");
            all.push_back(x);
        }
    }
    require(pp.scan_launches == levels && levels <= 14, "the scan launches are the largest level count");
    require(p.records.off == 0 && p.records.len == size_t(F) * JPEG_CLIP_RECORD_BYTES && p.zero.off >= p.upload_bytes && p.upload_bytes % 256 == 0 &&
                p.zero.off % 256 == 0,
            "records / upload / zero");
    std::sort(all.begin(), all.end(), [](const JpegClipRegion& a, const JpegClipRegion& b) { return a.off < b.off; });
    for (size_t i = 0; i < all.size(); ++i) {
        require(all[i].off + all[i].len <= p.bytes, "a region ends behind the total");
        if (i > 0) require(all[i - 1].off + all[i - 1].len <= all[i].off, "two regions overlap");
    }
    if (pp.progressive == 0) {      // region for region the plan of a baseline clip
        JpegClipPlan b;
        require(jpeg_clip_plan(g, nbytes, F, entropy, 128, b) == nullptr, "jpeg_clip_plan refuses what jpeg_clip_plan_progressive takes");
        std::vector<int64_t> w0(size_t(F) * JPEG_CLIP_PLAN_FRAME_WORDS + JPEG_CLIP_PLAN_TOTAL_WORDS), w1(w0.size());
        jpeg_clip_plan_words(b, w0.data()), jpeg_clip_plan_words(p, w1.data());
        require(w0 == w1, "a clip without a progressive frame is not laid out as jpeg_clip_plan lays it out");
    }
    // the upload block as the engine stages it: exactly upload_bytes
    std::unique_ptr<uint8_t[]> stage(new uint8_t[p.upload_bytes]);
    std::memset(stage.get() + p.records.off, 0, p.records.len);
    for (int f = 0; f < F; ++f) {
        const JpegClipFrame& q = p.f[f];
        const Stream& s = *clip[f];
        if (q.form == JPEG_CLIP_FORM_PROGRESSIVE) {
            jpeg_clip_stage_progressive(s.plan, q, pp.pf[f], s.bytes.data() + s.plan.data_base, stage.get());
        } else {
            jpeg_dec_build_tables(s.info, *reinterpret_cast<JpegDecTables*>(stage.get() + q.tables.off));
            if (q.data.len > 0) std::memcpy(stage.get() + q.data.off, s.bytes.data() + s.info.data_offset, q.data.len);
        }
    }
    // the whole allocation: exactly the plan's bytes; ONE copy, ONE clear
    std::unique_ptr<uint8_t[]> work(new uint8_t[p.bytes]);
    std::memset(work.get() + p.upload_bytes, 0xA5, p.bytes - p.upload_bytes);
    std::memcpy(work.get(), stage.get(), p.upload_bytes);
    std::memset(work.get() + p.zero.off, 0, p.zero.len);
    for (int f = 0; f < F; ++f)
        require(p.f[f].data.len == 0 || std::memcmp(work.get() + p.f[f].data.off,
                                                    clip[f]->bytes.data() + (clip[f]->plan.baseline ? clip[f]->info.data_offset : clip[f]->plan.data_base),
                                                    p.f[f].data.len) == 0,
                "the entropy bytes of a frame were overwritten");
    // the scan launches as the clip kernel walks them: launch L, frame by frame, workgroup by workgroup, lane by lane
    long long launches = 0;
    for (int l = 0; l < pp.scan_launches; ++l, ++launches)
        for (int f = 0; f < F; ++f) {
            const Stream& s = *clip[f];
            if (s.plan.baseline || l >= s.plan.levels) continue;
            const JpegClipProgFrame& r = pp.pf[f];
            const JpegProgScan* scans = reinterpret_cast<const JpegProgScan*>(work.get() + r.scans.off);
            const JpegDecHuff* huff = reinterpret_cast<const JpegDecHuff*>(work.get() + r.huff.off);
            const JpegProgItem* items = reinterpret_cast<const JpegProgItem*>(work.get() + r.items.off);
            int16_t* raw = reinterpret_cast<int16_t*>(work.get() + r.raw.off);
            int32_t* meta = reinterpret_cast<int32_t*>(work.get() + p.f[f].meta.off);
            const int first = s.plan.level_off[size_t(l)] / JPEG_PROG_LANES, groups = s.plan.level_cnt[size_t(l)] / JPEG_PROG_LANES;
            for (int wg = first; wg < first + groups; ++wg) {
                const int sc = items[size_t(wg) * JPEG_PROG_LANES].scan;
                require(sc >= 0 && sc < r.nscans, "a workgroup's first item is no item of a scan");
                for (int lane = 0; lane < JPEG_PROG_LANES; ++lane) {
                    const JpegProgItem it = items[size_t(wg) * JPEG_PROG_LANES + size_t(lane)];
                    if (it.scan != sc || it.interval < 0 || it.interval >= scans[sc].intervals || it.start < 0 || it.end > int(p.f[f].data.len) ||
                        it.start > it.end)
                        continue;
                    int16_t band[64];
                    if (!jpeg_prog_item(work.get() + p.f[f].data.off, it.start, it.end, scans[sc], huff + 3 * size_t(sc), g[f], it.interval, raw, band))
                        meta[0] = std::max(meta[0], JPEG_DEC_NO_BAD - (scans[sc].first_item + it.interval));
                }
            }
        }
    for (int f = 0; f < F; ++f) {      // the finish, and what the inverse DCT reads: coef and meta[1]
        const Stream& s = *clip[f];
        if (s.plan.baseline) continue;
        const int16_t* qz = reinterpret_cast<const int16_t*>(work.get() + pp.pf[f].qz.off);
        const int16_t* raw = reinterpret_cast<const int16_t*>(work.get() + pp.pf[f].raw.off);
        int16_t* coef = reinterpret_cast<int16_t*>(work.get() + p.f[f].coef.off);
        int32_t* meta = reinterpret_cast<int32_t*>(work.get() + p.f[f].meta.off);
        const size_t blocks = size_t(g[f].mcu_cols) * size_t(g[f].mcu_rows) * size_t(g[f].bpm);
        for (size_t b = 0; b < blocks; ++b) {
            const int bi = int(b % size_t(g[f].bpm)), c = g[f].comps == 1 || bi < g[f].bpm - 2 ? 0 : bi - (g[f].bpm - 2) + 1;
            for (int k = 0; k < 64; ++k) coef[b * 64 + JPEG_ZIGZAG[k]] = jpeg_prog_finish_value(raw[b * 64 + size_t(k)], qz[c * 64 + k]);
        }
        const int bad = meta[0] > 0 ? JPEG_DEC_NO_BAD - meta[0] : JPEG_DEC_NO_BAD;
        meta[1] = std::min(bad, s.plan.first_bad);
        require(std::memcmp(raw, s.want.raw.data(), blocks * 128) == 0, "the raw coefficients differ from the host statement's");
        require(std::memcmp(coef, s.want.coef.data(), blocks * 128) == 0, "the finished records differ from the host statement's");
        require((meta[1] == JPEG_DEC_NO_BAD ? -1 : meta[1]) == s.want_status[1] &&
                    (meta[1] == JPEG_DEC_NO_BAD ? WHENET_OK : WHENET_EFORMAT) == s.want_status[0],
                "the status differs from the host statement's");
    }
    std::unique_ptr<int64_t[]> words(new int64_t[size_t(F) * JPEG_CLIP_PROG_PLAN_FRAME_WORDS + JPEG_CLIP_PROG_PLAN_TOTAL_WORDS]);
    jpeg_clip_plan_progressive_words(pp, words.get());
    require(words[size_t(F) * JPEG_CLIP_PROG_PLAN_FRAME_WORDS + 5] == int64_t(p.bytes) &&
                words[size_t(F) * JPEG_CLIP_PROG_PLAN_FRAME_WORDS + 9] == pp.scan_launches,
            "the words' totals");
    ++counts[0], counts[1] += F, counts[2] += pp.progressive, counts[3] += F - pp.progressive, counts[4] += launches;
}

}  // namespace

int main(int argc, char** argv) {
    std::vector<Stream> streams;
    long long variants = 0;
    for (int i = 1; i < argc; ++i) {
        std::FILE* f = std::fopen(argv[i], "rb");
        if (!f) fail(std::string("cannot read ") + argv[i]);
        std::vector<uint8_t> bytes;
        uint8_t buf[4096];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) bytes.insert(bytes.end(), buf, buf + n);
        std::fclose(f);
        Stream s;
        if (!load(bytes, s)) fail(std::string("refused: ") + argv[i]);
        const size_t from = size_t(s.plan.baseline ? s.info.data_offset : s.plan.data_base);
        streams.push_back(std::move(s));
        // the damaged copies: cut, and one bit flipped at three places of the entropy data
        std::vector<std::vector<uint8_t>> copies;
        copies.emplace_back(bytes.begin(), bytes.begin() + std::max<size_t>(from + 1, bytes.size() * 3 / 4));
        for (int k = 1; k <= 3 && bytes.size() > from + 2; ++k) {
            std::vector<uint8_t> v = bytes;
            v[from + (bytes.size() - 2 - from) * size_t(k) / 4] ^= uint8_t(1u << (k + 1));
            copies.push_back(std::move(v));
        }
        for (std::vector<uint8_t>& v : copies) {
            Stream d;
            if (v.size() <= bytes.size() && load(std::move(v), d)) streams.push_back(std::move(d)), ++variants;
        }
    }
    require(!streams.empty(), "no stream given");
    long long counts[5] = {0, 0, 0, 0, 0};
    for (int F : {1, 3, 16})
        for (size_t first = 0; first < streams.size(); ++first) {
            std::vector<const Stream*> clip;
            for (int f = 0; f < F; ++f) clip.push_back(&streams[(first + size_t(f)) % streams.size()]);
            for (int entropy : {0, 1, 2}) check_plan(clip, entropy, counts);
        }
    // refusals
    JpegClipProgPlan pp;
    JpegDecGeom g = streams[0].g;
    int64_t nb = streams[0].nbytes;
    const JpegProgPlan* one = &streams[0].plan;
    JpegProgPlan empty;      // says progressive, holds nothing
    const JpegProgPlan* none = &empty;
    require(jpeg_clip_plan_progressive(&g, &nb, &one, 0, 0, 128, pp) != nullptr && jpeg_clip_plan_progressive(&g, &nb, &one, 17, 0, 128, pp) != nullptr &&
                jpeg_clip_plan_progressive(&g, &nb, &one, 1, 3, 128, pp) != nullptr && jpeg_clip_plan_progressive(&g, &nb, &one, 1, 1, 100, pp) != nullptr &&
                jpeg_clip_plan_progressive(nullptr, &nb, &one, 1, 0, 128, pp) != nullptr && jpeg_clip_plan_progressive(&g, &nb, &none, 1, 0, 128, pp) != nullptr,
            "a bad argument was accepted");
    std::printf("plans %lld frames %lld progressive %lld baseline %lld launches %lld variants %lld\n", counts[0], counts[1], counts[2], counts[3],
                counts[4], variants);
    std::fprintf(stderr, "no report\n");
    return 0;
}
