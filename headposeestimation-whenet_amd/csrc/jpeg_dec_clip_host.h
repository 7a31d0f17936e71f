// A clip of JPEG streams: where every frame's share of the upload block and of the work buffer lies, and in which entropy form it
// runs.  One planner (jpeg_clip_plan_progressive; jpeg_clip_plan is it without scan plans) serves the engine (clip_begin_jpeg,
// op_jpeg_decode_clip) and whenet_jpeg_clip_plan / whenet_jpeg_clip_plan_progressive, so the layout the kernels of jpeg_dec.hip /
// jpeg_dec_seg.hip / jpeg_prog.hip get is the one the CPU tests see.  Nothing here needs the HIP runtime: a plain C++17 compiler
// builds this header (tools/jpeg_dec_clip_host_check.cpp does, under the host sanitizers).
//
// Reference: demo_video.py:49-53 (`cap.read()` in a loop: consecutive frames of one MJPG file).
//
// One allocation, offsets in bytes, every region at a multiple of 256 (the kernels need 8 for the planes and 16 for vector loads):
//   upload block   records [frames] of JPEG_CLIP_RECORD_BYTES | per frame: tables | entropy data        -- ONE H2D
//   zeroed bytes   per frame: start [intervals] | meta (64) | seg_stats (64); then per frame: coef        -- ONE memset
//   work           per frame: the component planes; per frame of form 1: first_seg | seg_exit | seg_count | seg_blk
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "jpeg_dec_seg_host.h"
#include "jpeg_prog_host.h"

namespace whenet {

constexpr int JPEG_CLIP_MAX_FRAMES = 16;
constexpr int JPEG_CLIP_RECORD_BYTES = 512;      // the stride of the argument records (>= sizeof(JpegDecArgs), checked in jpeg_dec.hip)
constexpr int JPEG_CLIP_PLAN_FRAME_WORDS = 32;   // whenet_jpeg_clip_plan: int64 words per frame ...
constexpr int JPEG_CLIP_PLAN_TOTAL_WORDS = 8;    // ... and behind the last frame

struct JpegClipRegion {
    size_t off, len;
};
struct JpegClipFrame {
    int form, seg_bytes;      // seg_bytes: 0 in form 0
    int64_t seg_cap;          // 0 in form 0
    // in the order whenet_jpeg_clip_plan writes them
    JpegClipRegion tables, data, start, meta, seg_stats, coef, plane[3], first_seg, seg_exit, seg_count, seg_blk;
};
struct JpegClipPlan {
    int frames, forms[2];     // forms[k]: the frames of form k
    JpegClipFrame f[JPEG_CLIP_MAX_FRAMES];
    JpegClipRegion records, zero;
    size_t upload_bytes, bytes;
};

// ---- clips that may hold PROGRESSIVE streams (jpeg_prog_host.h): the same planner, with a scan plan per such frame ----
// A frame is baseline (its JpegProgPlan is nullptr or says `baseline`: laid out as above, in the form the rule gives it alone) or
// progressive (form JPEG_CLIP_FORM_PROGRESSIVE).  The same three blocks:
//   upload block   records | per frame: tables | data, or, progressive: scans | huff | qz | items | data (what jpeg_prog_stage
//                  writes for the stream alone; list_off / level_off stay indices into the frame's OWN item list)   -- ONE H2D
//   zeroed bytes   per frame: start | meta | seg_stats, or meta; then per frame: coef, or, progressive: the raw coefficients -- ONE memset
//   work           per progressive frame: its finished coef; per frame: the planes; per frame of form 1: the segmented regions
// A clip without a progressive frame gets the layout at the head of this file: jpeg_clip_plan is this planner called without
// plans.  A frame's progressive record (JpegProgArgs) lies in the frame's own argument record, JPEG_CLIP_PROG_RECORD_OFFSET bytes
// behind its start (checked in jpeg_prog.hip).
constexpr int JPEG_CLIP_FORM_PROGRESSIVE = 2;
constexpr int JPEG_CLIP_PROG_RECORD_OFFSET = 320;
constexpr int JPEG_CLIP_PROG_PLAN_FRAME_WORDS = 48;      // whenet_jpeg_clip_plan_progressive: the 32 words above + 16 ...
constexpr int JPEG_CLIP_PROG_PLAN_TOTAL_WORDS = 16;      // ... and the 8 above + 8 behind the last frame

struct JpegClipProgFrame {
    JpegClipRegion scans, huff, qz, items, raw;      // empty for a baseline frame
    int nscans, levels, list;                        // list: the entries of the item list (a multiple of JPEG_PROG_LANES)
};
struct JpegClipProgPlan {
    // a progressive frame there: form 2, seg_bytes = seg_cap = 0; data (every scan's entropy bytes), meta, coef and plane[] are its
    // regions, tables / start / seg_stats / the segmented regions are empty; forms[] count the baseline frames only
    JpegClipPlan base;
    JpegClipProgFrame pf[JPEG_CLIP_MAX_FRAMES];
    int progressive;       // the progressive frames
    int scan_launches;     // the largest level count among the SOF2 frames: launch L of the scan kernel covers level L of every frame that
                           // has one; + 1 where the clip holds sequential frames that go through the scan plan (plan.sequential)
};

inline bool jpeg_clip_is_progressive(const JpegProgPlan* plan) { return plan != nullptr && !plan->baseline; }

// what both planners refuse first, and the two per-frame checks each of them makes in its own order
inline const char* jpeg_clip_check_args(const JpegDecGeom* g, const int64_t* nbytes, int frames, int entropy, int seg_bytes) {
    if (g == nullptr || nbytes == nullptr) return "NULL argument";
    if (frames < 1 || frames > JPEG_CLIP_MAX_FRAMES) return "a clip holds 1..16 frames";
    if (entropy < 0 || entropy > 2) return "entropy must be 0 (an interval per lane), 1 (segmented) or 2 (auto)";
    if (!jpeg_seg_bytes_ok(seg_bytes)) return "seg_bytes must be a power of two in 4..4096";
    return nullptr;
}
inline bool jpeg_clip_nbytes_ok(int64_t nbytes) { return nbytes >= 0 && nbytes <= JPEG_DEC_MAX_BYTES; }
inline bool jpeg_clip_geom_ok(const JpegDecGeom& g) {
    return g.intervals >= 1 && g.mcu_cols >= 1 && g.mcu_rows >= 1 && g.bpm >= 1 && g.comps >= 1 && g.comps <= 3;
}

// entropy: 0, 1 or 2 (auto), applied to every baseline stream alone; seg_bytes: a power of two in 4..4096.  nbytes[f] is read for
// baseline frames only; prog may be nullptr (no progressive frame).  nullptr, or what is wrong.
inline const char* jpeg_clip_plan_progressive(const JpegDecGeom* g, const int64_t* nbytes, const JpegProgPlan* const* prog, int frames, int entropy,
                                              int seg_bytes, JpegClipProgPlan& pp) {
    if (const char* bad = jpeg_clip_check_args(g, nbytes, frames, entropy, seg_bytes)) return bad;
    const auto is_prog = [&](int f) { return prog != nullptr && jpeg_clip_is_progressive(prog[f]); };
    for (int f = 0; f < frames; ++f) {
        if (!jpeg_clip_geom_ok(g[f])) return "bad geometry";
        if (is_prog(f)) {
            const JpegProgPlan& s = *prog[f];
            if (s.dev.empty() || s.huff.size() != size_t(s.huff_per_scan()) * s.dev.size() || (s.sequential && s.levels != 1) || s.items.empty() || s.items.size() % JPEG_PROG_LANES != 0 || s.levels < 1 ||
                s.level_off.size() != size_t(s.levels) || s.level_cnt.size() != size_t(s.levels) || s.data_bytes < 0 || s.data_bytes > JPEG_DEC_MAX_BYTES)
                return "not the plan of a progressive stream";
        } else if (!jpeg_clip_nbytes_ok(nbytes[f])) {
            return "nbytes must be 0..2^31 - 1";
        }
    }
    const auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
    pp = JpegClipProgPlan{};
    JpegClipPlan& p = pp.base;
    p.frames = frames;
    size_t at = 0;
    const auto take = [&](JpegClipRegion& r, size_t len) { r.off = at, r.len = len, at = up(at + len); };
    const auto none = [&](JpegClipRegion& r) { r = {at, 0}; };
    take(p.records, size_t(frames) * JPEG_CLIP_RECORD_BYTES);
    int prog_launches = 0, seq_launch = 0;
    for (int f = 0; f < frames; ++f) {
        JpegClipFrame& q = p.f[f];
        JpegClipProgFrame& r = pp.pf[f];
        if (is_prog(f)) {
            const JpegProgPlan& s = *prog[f];
            q.form = JPEG_CLIP_FORM_PROGRESSIVE, q.seg_bytes = 0, q.seg_cap = 0;
            r.nscans = int(s.dev.size()), r.levels = s.levels, r.list = int(s.items.size());
            ++pp.progressive;
            // (the sequential frames of a clip -- one level each -- share ONE launch of their own scan kernel, the SOF2 frames a launch per level)
            if (s.sequential) seq_launch = 1;
            else if (s.levels > prog_launches) prog_launches = s.levels;
            pp.scan_launches = prog_launches + seq_launch;
            none(q.tables);
            take(r.scans, s.dev.size() * sizeof(JpegProgScan));
            take(r.huff, s.huff.size() * sizeof(JpegDecHuff));
            take(r.qz, sizeof(s.qz));
            take(r.items, s.items.size() * sizeof(JpegProgItem));
            take(q.data, size_t(s.data_bytes));
            continue;
        }
        q.form = jpeg_dec_form(entropy, nbytes[f], g[f].intervals);
        q.seg_bytes = q.form == 1 ? seg_bytes : 0;
        q.seg_cap = q.form == 1 ? jpeg_seg_bound(nbytes[f], g[f].intervals, seg_bytes) : 0;
        if (q.seg_cap >= 0x7FFFFFFF) return "more segments than an int32 counts";
        ++p.forms[q.form];
        take(q.tables, sizeof(JpegDecTables));
        take(q.data, size_t(nbytes[f]));
        none(r.scans), none(r.huff), none(r.qz), none(r.items);
    }
    p.upload_bytes = at;
    p.zero.off = at;
    for (int f = 0; f < frames; ++f) {
        JpegClipFrame& q = p.f[f];
        if (q.form == JPEG_CLIP_FORM_PROGRESSIVE) {
            none(q.start);
            q.meta = {at, 64}, q.seg_stats = {at + 64, 0}, at = up(at + 64);
            continue;
        }
        take(q.start, size_t(g[f].intervals) * sizeof(int32_t));
        q.meta = {at, 64}, q.seg_stats = {at + 64, 8 * sizeof(int64_t)}, at = up(at + 128);
    }
    for (int f = 0; f < frames; ++f) {
        const size_t coef_bytes = size_t(g[f].mcu_cols) * size_t(g[f].mcu_rows) * size_t(g[f].bpm) * 64 * sizeof(int16_t);
        if (p.f[f].form == JPEG_CLIP_FORM_PROGRESSIVE) {
            take(pp.pf[f].raw, coef_bytes);
        } else {
            take(p.f[f].coef, coef_bytes);
            none(pp.pf[f].raw);
        }
    }
    p.zero.len = at - p.zero.off;
    for (int f = 0; f < frames; ++f)
        if (p.f[f].form == JPEG_CLIP_FORM_PROGRESSIVE)
            take(p.f[f].coef, size_t(g[f].mcu_cols) * size_t(g[f].mcu_rows) * size_t(g[f].bpm) * 64 * sizeof(int16_t));
    for (int f = 0; f < frames; ++f)
        for (int c = 0; c < 3; ++c) {
            if (c < g[f].comps) take(p.f[f].plane[c], size_t(g[f].plane_pitch[c]) * size_t(g[f].plane_rows[c]));
            else none(p.f[f].plane[c]);
        }
    for (int f = 0; f < frames; ++f) {
        JpegClipFrame& q = p.f[f];
        if (q.form == 1) {
            take(q.first_seg, (size_t(g[f].intervals) + 1) * sizeof(int32_t));
            take(q.seg_exit, size_t(q.seg_cap) * sizeof(uint64_t));
            take(q.seg_count, size_t(q.seg_cap) * sizeof(JpegSegCount));
            take(q.seg_blk, size_t(q.seg_cap) * 4 * sizeof(int32_t));
        } else {
            none(q.first_seg), none(q.seg_exit), none(q.seg_count), none(q.seg_blk);
        }
    }
    p.bytes = at;
    return nullptr;
}

// A clip of baseline streams: the planner above without plans (its own order of the per-frame checks: nbytes first)
inline const char* jpeg_clip_plan(const JpegDecGeom* g, const int64_t* nbytes, int frames, int entropy, int seg_bytes, JpegClipPlan& p) {
    if (const char* bad = jpeg_clip_check_args(g, nbytes, frames, entropy, seg_bytes)) return bad;
    for (int f = 0; f < frames; ++f) {
        if (!jpeg_clip_nbytes_ok(nbytes[f])) return "nbytes must be 0..2^31 - 1";
        if (!jpeg_clip_geom_ok(g[f])) return "bad geometry";
    }
    JpegClipProgPlan pp;
    const char* bad = jpeg_clip_plan_progressive(g, nbytes, nullptr, frames, entropy, seg_bytes, pp);
    p = pp.base;
    return bad;
}

// the plan as whenet_jpeg_clip_plan hands it out: frames * 32 + 8 words (frame_words: the stride of a frame's words)
inline void jpeg_clip_plan_words(const JpegClipPlan& p, int64_t* out, int frame_words = JPEG_CLIP_PLAN_FRAME_WORDS) {
    for (int f = 0; f < p.frames; ++f) {
        const JpegClipFrame& q = p.f[f];
        int64_t* o = out + size_t(f) * size_t(frame_words);
        o[0] = q.form, o[1] = q.seg_bytes, o[2] = q.seg_cap, o[3] = 0;
        const JpegClipRegion* r[13] = {&q.tables,   &q.data,     &q.start,     &q.meta,     &q.seg_stats, &q.coef,   &q.plane[0],
                                       &q.plane[1], &q.plane[2], &q.first_seg, &q.seg_exit, &q.seg_count, &q.seg_blk};
        for (int k = 0; k < 13; ++k) o[4 + 2 * k] = int64_t(r[k]->off), o[5 + 2 * k] = int64_t(r[k]->len);
        o[30] = o[31] = 0;
    }
    int64_t* t = out + size_t(p.frames) * size_t(frame_words);
    t[0] = int64_t(p.records.off), t[1] = int64_t(p.records.len), t[2] = int64_t(p.upload_bytes), t[3] = int64_t(p.zero.off);
    t[4] = int64_t(p.zero.len), t[5] = int64_t(p.bytes), t[6] = p.forms[0], t[7] = p.forms[1];
}

// a progressive frame's share of the upload block into `stage` (the block's first byte; data: the stream's bytes from
// plan.data_base on): the content jpeg_prog_stage writes, the padding between the regions zeroed
inline void jpeg_clip_stage_progressive(const JpegProgPlan& plan, const JpegClipFrame& q, const JpegClipProgFrame& r, const uint8_t* data,
                                        uint8_t* stage) {
    std::memset(stage + r.scans.off, 0, q.data.off - r.scans.off);
    std::memcpy(stage + r.scans.off, plan.dev.data(), r.scans.len);
    std::memcpy(stage + r.huff.off, plan.huff.data(), r.huff.len);
    std::memcpy(stage + r.qz.off, plan.qz, r.qz.len);
    std::memcpy(stage + r.items.off, plan.items.data(), r.items.len);
    if (q.data.len > 0) std::memcpy(stage + q.data.off, data, q.data.len);
}

// the plan as whenet_jpeg_clip_plan_progressive hands it out: frames * 48 + 16 words.  A frame's words 0..31 and the totals' words
// 0..7 are jpeg_clip_plan_words' (form 2: a progressive frame); a frame's words 32..41: (offset, length) of scans, huff, qz, items,
// raw; 42: its scans, 43: its levels, 44: the entries of its item list; 45..47: 0.  Totals 8: the progressive frames, 9: the
// scan-kernel launches, 10: the stride of the argument records, 11: where a frame's progressive record lies in its own; 12..15: 0.
inline void jpeg_clip_plan_progressive_words(const JpegClipProgPlan& pp, int64_t* out) {
    jpeg_clip_plan_words(pp.base, out, JPEG_CLIP_PROG_PLAN_FRAME_WORDS);
    for (int f = 0; f < pp.base.frames; ++f) {
        const JpegClipProgFrame& x = pp.pf[f];
        int64_t* o = out + size_t(f) * JPEG_CLIP_PROG_PLAN_FRAME_WORDS + JPEG_CLIP_PLAN_FRAME_WORDS;
        const JpegClipRegion* r[5] = {&x.scans, &x.huff, &x.qz, &x.items, &x.raw};
        for (int k = 0; k < 5; ++k) o[2 * k] = int64_t(r[k]->off), o[2 * k + 1] = int64_t(r[k]->len);
        o[10] = x.nscans, o[11] = x.levels, o[12] = x.list, o[13] = o[14] = o[15] = 0;
    }
    int64_t* t = out + size_t(pp.base.frames) * JPEG_CLIP_PROG_PLAN_FRAME_WORDS + JPEG_CLIP_PLAN_TOTAL_WORDS;
    t[0] = pp.progressive, t[1] = pp.scan_launches, t[2] = JPEG_CLIP_RECORD_BYTES, t[3] = JPEG_CLIP_PROG_RECORD_OFFSET;
    t[4] = t[5] = t[6] = t[7] = 0;
}

}  // namespace whenet
