// The segmented form of the JPEG decoder's entropy stage as arithmetic, shared by its host emulation (jpeg_dec_planes_seg_host,
// behind whenet_jpeg_decode_segmented_host) and the kernels of jpeg_dec_seg.hip.  It decodes every restart interval -- the single
// interval of a stream without DRI included -- with many lanes, and gives exactly what jpeg_dec_host.h's jpeg_dec_interval gives:
// coefficients, planes, frame and status, damaged streams included (include/whenet_hip.h, JPEG DECODER, "segmented form").
//
// The method is the self-synchronisation of Huffman streams: an interval's bytes are cut into segments of seg_bytes; a lane starts at
// its segment's first byte with a guessed state, the guesses are corrected until every segment's entry state is the true one, and the
// blocks are then decoded from those states.  The bit reader, the tables, the block decode and the geometry are jpeg_dec_host.h's.
// Integers only; a plain C++17 compiler builds this header (tools/jpeg_dec_seg_host_check.cpp does, under the host sanitizers).
//
// Reference: demo.py (`cv2.imread` of Sample/*.jpeg, streams without restart markers) and demo_video.py:49-53 (`cap.read()`).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "jpeg_dec_host.h"

namespace whenet {

constexpr int JPEG_SEG_MIN_BYTES = 4, JPEG_SEG_MAX_BYTES = 4096;      // seg_bytes: a power of two in this range
constexpr int JPEG_SEG_DEFAULT_BYTES = 128;
constexpr int JPEG_SEG_MAX_WINDOW = 1024;
constexpr int JPEG_SEG_OPEN_END = 0x7FFFFFFF;      // the end of an interval's last segment: it runs as far as the interval's bits
// "auto" (option jpeg_entropy = 2) takes the segmented form where the data has at least this many bytes per restart interval
constexpr int64_t JPEG_SEG_AUTO_BYTES = 4096;

inline bool jpeg_seg_bytes_ok(int64_t v) { return v >= JPEG_SEG_MIN_BYTES && v <= JPEG_SEG_MAX_BYTES && (v & (v - 1)) == 0; }
// the form a decode runs in: entropy = 0 (an interval per lane), 1 (segmented) or 2 (auto, by the bytes per interval)
inline int jpeg_dec_form(int entropy, int64_t nbytes, int intervals) {
    if (entropy != 2) return entropy;
    return nbytes / std::max(intervals, 1) >= JPEG_SEG_AUTO_BYTES ? 1 : 0;
}
// the host's bound of the segment count: every launch and every array is sized from it
inline int64_t jpeg_seg_bound(int64_t nbytes, int intervals, int seg_bytes) { return (nbytes + seg_bytes - 1) / seg_bytes + intervals; }

// ---- the sync state ----
// What a decoder needs between two code words, in one word: the position of the next unread bit (its byte in the raw data, never the
// 0x00 of a stuffed pair, and the bit's offset in that byte), the block's index in its MCU and the zigzag index (0: a DC symbol comes
// next).  Equal states have the same continuation; that equality is the only synchronisation test.  DEAD: the chain met damage, or
// the interval's bits have ended.  A walk from DEAD yields DEAD.
// A chain that dies in a segment stores DEAD as that segment's exit state and ends there: it does not carry DEAD through the later
// segments, where it would replace states that other chains have already brought to the truth.  So a stored exit state is the
// continuation of the one before it wherever that one is not DEAD, and what lies behind a DEAD exit state of the true chain is cut
// off by an OR-scan beside the block counts (JpegSegCount::dead): those segments write nothing.
constexpr uint64_t JPEG_SEG_DEAD = ~uint64_t(0);
WHENET_HD inline uint64_t jpeg_seg_pack(int pos, int off, int b, int k) {
    return (uint64_t(uint32_t(pos)) << 32) | (uint64_t(uint32_t(off)) << 16) | (uint64_t(uint32_t(b)) << 8) | uint64_t(uint32_t(k));
}
WHENET_HD inline int jpeg_seg_pos(uint64_t s) { return int(uint32_t(s >> 32)); }
WHENET_HD inline int jpeg_seg_off(uint64_t s) { return int((s >> 16) & 7u); }
WHENET_HD inline int jpeg_seg_b(uint64_t s) { return int((s >> 8) & 255u); }
WHENET_HD inline int jpeg_seg_k(uint64_t s) { return int(s & 255u); }

// where the reader's next unread bit lies.  The reader holds br.n unread bits of the ceil(n / 8) bytes it fetched last; each of them
// is one raw byte, or two where it is a stuffed 0xFF 0x00 (a 0x00 behind a 0xFF is never a byte of its own: no walk starts on one).
WHENET_HD inline void jpeg_seg_cursor(const JpegBitReader& br, int& pos, int& off) {
    int p = br.pos;
    for (int nb = (br.n + 7) >> 3; nb > 0; --nb) {
        --p;
        if (p >= 1 && br.d[p] == 0 && br.d[p - 1] == 0xFF) --p;
    }
    pos = p, off = (8 - (br.n & 7)) & 7;
}
// is the next unread bit before byte `end`?  (the cursor lies in [pos - 2 nb, pos - nb]: the exact walk back only near the end)
WHENET_HD inline bool jpeg_seg_before(const JpegBitReader& br, int end) {
    if (end == JPEG_SEG_OPEN_END) return true;
    const int nb = (br.n + 7) >> 3;
    if (br.pos - nb < end) return true;
    if (br.pos - 2 * nb >= end) return false;
    int p, off;
    jpeg_seg_cursor(br, p, off);
    return p < end;
}
// the reader of a state
WHENET_HD inline JpegBitReader jpeg_seg_reader(const uint8_t* data, int size, uint64_t s) {
    JpegBitReader br(data, jpeg_seg_pos(s), size);
    const int off = jpeg_seg_off(s);
    if (off != 0) {
        br.fill();
        br.n = br.n >= off ? br.n - off : 0;
    }
    return br;
}
WHENET_HD inline int jpeg_seg_comp(const JpegDecGeom& g, int b) { return g.comps == 1 || b < g.bpm - 2 ? 0 : b - (g.bpm - 2) + 1; }

// One code word with its extra bits: (b, k) moves on exactly as jpeg_dec_block's loop does, and it fails exactly where that does.
// dc: the DC difference where the code word was a DC symbol (k was 0).
WHENET_HD inline bool jpeg_seg_symbol(JpegBitReader& br, const JpegDecTables& t, const JpegDecGeom& g, int& b, int& k, int& dc) {
    const int c = jpeg_seg_comp(g, b);
    int v;
    if (k == 0) {
        const int s = br.decode(t.huff[g.dc[c]]);
        if (s < 0 || !br.receive(s & 15, v)) return false;
        dc = v, k = 1;
        return true;
    }
    const int sym = br.decode(t.huff[g.ac[c]]);
    if (sym < 0) return false;
    const int r = sym >> 4, s = sym & 15;
    if (s == 0) {
        if (r == 15) {      // ZRL
            k += 16;
            if (k > 64) return false;
        } else {            // EOB
            k = 64;
        }
    } else {
        k += r;
        if (k > 63 || !br.receive(s, v)) return false;
        ++k;
    }
    if (k == 64) k = 0, b = b + 1 == g.bpm ? 0 : b + 1;
    return true;
}

// From state s to the first code-word boundary at or behind byte `end`; bytes += the raw bytes the walk fetched.
WHENET_HD inline uint64_t jpeg_seg_walk(const uint8_t* data, int size, const JpegDecTables& t, const JpegDecGeom& g, uint64_t s, int end,
                                        long long& bytes) {
    if (s == JPEG_SEG_DEAD) return s;
    if (end != JPEG_SEG_OPEN_END && jpeg_seg_pos(s) >= end) return s;
    JpegBitReader br = jpeg_seg_reader(data, size, s);
    int b = jpeg_seg_b(s), k = jpeg_seg_k(s), dc;
    const int from = jpeg_seg_pos(s);
    for (;;) {      // (every code word takes a bit at least, and the bits end)
        if (!jpeg_seg_symbol(br, t, g, b, k, dc)) {
            bytes += br.pos - from;
            return JPEG_SEG_DEAD;
        }
        if (jpeg_seg_before(br, end)) continue;
        int p, off;
        jpeg_seg_cursor(br, p, off);
        bytes += br.pos - from;
        return jpeg_seg_pack(p, off, b, k);
    }
}

// ---- the segment table ----
// interval i's bytes: [start[i], the next restart marker or the end of the data)
WHENET_HD inline int jpeg_seg_interval_end(const int32_t* start, int intervals, int i, int nbytes) {
    return i + 1 < intervals && start[i + 1] > 0 ? start[i + 1] - 2 : nbytes;
}
// its segments: at least one, so that an interval without a byte is still decoded (and found damaged)
WHENET_HD inline int jpeg_seg_count(int from, int end, int seg_bytes) {
    const int n = int(((long long)(end) - from + seg_bytes - 1) / seg_bytes);
    return n < 1 ? 1 : n;
}
// the interval of flat segment s: the last i < nd with first_seg[i] <= s (first_seg is strictly increasing over the nd decoded ones)
WHENET_HD inline int jpeg_seg_interval_of(const int32_t* first_seg, int nd, int s) {
    int lo = 0, hi = nd - 1;
    while (lo < hi) {      // (at most 31 steps)
        const int mid = (lo + hi + 1) >> 1;
        if (first_seg[mid] <= s) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// A segment as its lane sees it
struct JpegSeg {
    int interval, q, nq;      // its interval, its index among the interval's nq segments
    int from, end;            // its bytes; end = JPEG_SEG_OPEN_END for the interval's last one
};
// segment s, which lies in interval i
WHENET_HD inline JpegSeg jpeg_seg_in(const int32_t* start, const int32_t* first_seg, int i, int seg_bytes, int s) {
    JpegSeg g;
    g.interval = i;
    g.q = s - first_seg[i], g.nq = first_seg[i + 1] - first_seg[i];
    g.from = start[i] + g.q * seg_bytes;
    g.end = g.q + 1 == g.nq ? JPEG_SEG_OPEN_END : g.from + seg_bytes;
    return g;
}
WHENET_HD inline JpegSeg jpeg_seg_at(const int32_t* start, const int32_t* first_seg, int nd, int seg_bytes, int s) {
    return jpeg_seg_in(start, first_seg, jpeg_seg_interval_of(first_seg, nd, s), seg_bytes, s);
}
WHENET_HD inline int jpeg_seg_end_of(const JpegSeg& g, int q, int seg_bytes) {      // the end of segment q of g's interval
    return q + 1 == g.nq ? JPEG_SEG_OPEN_END : g.from + (q - g.q + 1) * seg_bytes;
}
// the entry state of a segment before anything is known: true for an interval's first one, otherwise the guess (its first byte, or
// the byte behind it where that is the 0x00 of a stuffed pair; b = 0, k = 0)
WHENET_HD inline uint64_t jpeg_seg_entry_guess(const uint8_t* data, const JpegSeg& g) {
    if (g.q == 0) return jpeg_seg_pack(g.from, 0, 0, 0);
    const int skip = data[g.from] == 0 && data[g.from - 1] == 0xFF ? 1 : 0;
    return jpeg_seg_pack(g.from + skip, 0, 0, 0);
}

// ---- the DC predictors as maps ----
// x -> min(max(x + a, lo), hi): what a run of blocks does to its component's predictor (clamped to -32768..32767 after every block).
// Such maps compose to such a map, associatively, so a parallel prefix over them is exact where a sum of differences is not.
struct JpegSegMap {
    long long a;
    int lo, hi;
};
constexpr int JPEG_SEG_MAP_FREE = 1 << 30;      // bounds that never bind: the identity is (0, -FREE, FREE)
WHENET_HD inline JpegSegMap jpeg_seg_map_identity() { return JpegSegMap{0, -JPEG_SEG_MAP_FREE, JPEG_SEG_MAP_FREE}; }
WHENET_HD inline JpegSegMap jpeg_seg_map_block(int diff) { return JpegSegMap{diff, -32768, 32767}; }
WHENET_HD inline int jpeg_seg_map_bound(long long v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : int(v)); }
// f, then g
WHENET_HD inline JpegSegMap jpeg_seg_map_then(const JpegSegMap& f, const JpegSegMap& g) {
    return JpegSegMap{f.a + g.a, jpeg_seg_map_bound(f.lo + g.a, g.lo, g.hi), jpeg_seg_map_bound(f.hi + g.a, g.lo, g.hi)};
}
WHENET_HD inline int jpeg_seg_map_apply(const JpegSegMap& f, int x) { return jpeg_seg_map_bound(x + f.a, f.lo, f.hi); }

// ---- count ----
// A block belongs to the segment in which its DC code word begins.  From its true entry state a lane counts its blocks and composes
// their DC differences, per component.
struct JpegSegCount {
    int blocks;
    int dead;      // the segment's exit state is DEAD: the segments behind it in the interval own nothing
    JpegSegMap map[3];
};
WHENET_HD inline JpegSegCount jpeg_seg_count_blocks(const uint8_t* data, int size, const JpegDecTables& t, const JpegDecGeom& g, uint64_t s, int end) {
    JpegSegCount c;
    c.blocks = 0, c.dead = 0;
    JpegSegMap m0 = jpeg_seg_map_identity(), m1 = m0, m2 = m0;      // (three values, not an array: the component is not known at compile time)
    c.map[0] = c.map[1] = c.map[2] = m0;
    if (s == JPEG_SEG_DEAD) return c;
    JpegBitReader br = jpeg_seg_reader(data, size, s);
    int b = jpeg_seg_b(s), k = jpeg_seg_k(s), dc = 0;
    while (jpeg_seg_before(br, end)) {
        const bool first = k == 0;
        const int comp = jpeg_seg_comp(g, b);
        if (first) ++c.blocks;
        if (!jpeg_seg_symbol(br, t, g, b, k, dc)) break;
        if (first) {
            const JpegSegMap d = jpeg_seg_map_block(dc);
            if (comp == 0) m0 = jpeg_seg_map_then(m0, d);
            else if (comp == 1) m1 = jpeg_seg_map_then(m1, d);
            else m2 = jpeg_seg_map_then(m2, d);
        }
    }
    c.map[0] = m0, c.map[1] = m1, c.map[2] = m2;
    return c;
}

// ---- write ----
// The lane of a segment decodes the blocks it owns, completely (the tail behind the segment's end included), from its true entry
// state s, the index `blk` of its first block in the interval and the three predictors there.  rec0: the record of the interval's
// first block; nblocks: the interval's blocks (bytes behind the last one are padding, not damage); stage: 64 int16 of fast memory,
// 16-byte aligned.  false: damage (the block in hand keeps what was decoded of it).
WHENET_HD inline bool jpeg_seg_write(const uint8_t* data, int size, const JpegDecTables& t, const JpegDecGeom& g, uint64_t s, int end, long long blk,
                                     const int pred_in[3], long long nblocks, int16_t* rec0, int16_t* stage) {
    if (s == JPEG_SEG_DEAD || blk < 0 || blk >= nblocks) return true;
    JpegBitReader br = jpeg_seg_reader(data, size, s);
    int b = jpeg_seg_b(s), k = jpeg_seg_k(s), dc;
    while (k != 0)      // the partial block at the start is the lane's before: damage in it is that lane's to report
        if (!jpeg_seg_symbol(br, t, g, b, k, dc)) return true;
    int p0 = pred_in[0], p1 = pred_in[1], p2 = pred_in[2];
    while (blk < nblocks && jpeg_seg_before(br, end)) {
        const int c = jpeg_seg_comp(g, b);
        int16_t* const rec = rec0 + size_t(blk) * 64;
        std::memset(__builtin_assume_aligned(stage, 16), 0, 128);
        int p = c == 0 ? p0 : (c == 1 ? p1 : p2);
        const bool ok = jpeg_dec_block(br, t.huff[g.dc[c]], t.huff[g.ac[c]], t.q[g.qt[c]], t.zz, p, stage);
        std::memcpy(__builtin_assume_aligned(rec, 16), __builtin_assume_aligned(stage, 16), 128);
        if (!ok) return false;
        if (c == 0) p0 = p;
        else if (c == 1) p1 = p;
        else p2 = p;
        ++blk, b = b + 1 == g.bpm ? 0 : b + 1;
    }
    return true;
}

WHENET_HD inline long long jpeg_seg_interval_blocks(const JpegDecGeom& g, int interval) {
    const long long mcus = (long long)(g.mcu_cols) * g.mcu_rows, first = (long long)(interval) * g.ri;
    return (first + g.ri < mcus ? g.ri : mcus - first) * g.bpm;
}

// ---- the host emulation: the kernels' steps, lanes in a plain loop ----
// The saturating scan alone, for its test: pred[i] = the predictor behind difference i (from 0), by maps over chunks of `chunk`
inline void jpeg_seg_dc_scan_host(const int32_t* diff, int64_t n, int chunk, int32_t* pred) {
    const int64_t chunks = (n + chunk - 1) / chunk;
    std::vector<JpegSegMap> m(size_t(chunks), jpeg_seg_map_identity());
    for (int64_t c = 0; c < chunks; ++c)
        for (int64_t i = c * chunk; i < std::min(n, (c + 1) * chunk); ++i) m[size_t(c)] = jpeg_seg_map_then(m[size_t(c)], jpeg_seg_map_block(diff[i]));
    JpegSegMap before = jpeg_seg_map_identity();
    for (int64_t c = 0; c < chunks; ++c) {
        int p = jpeg_seg_map_apply(before, 0);
        for (int64_t i = c * chunk; i < std::min(n, (c + 1) * chunk); ++i) pred[i] = p = jpeg_seg_map_apply(jpeg_seg_map_block(diff[i]), p);
        before = jpeg_seg_map_then(before, m[size_t(c)]);
    }
}

// The coefficient records of the whole picture ([blocks][64], zeroed here) by the segmented form; returns the first bad interval or
// JPEG_DEC_NO_BAD.  stats: as whenet_jpeg_decode_segmented_host states them.
inline int jpeg_dec_coef_seg_host(const JpegDecGeom& g, const JpegDecTables& t, const uint8_t* data, int size, int seg_bytes, int window,
                                  std::vector<int16_t>& coef, int64_t stats[8]) {
    // the marker scan, as it is
    std::vector<int32_t> start;
    const int scan_bad = jpeg_dec_scan_host(data, size, g.intervals, start);
    int bad = scan_bad;
    coef.assign(size_t(g.mcu_cols) * size_t(g.mcu_rows) * size_t(g.bpm) * 64, int16_t(0));
    // 2. the segment table
    const int nd = std::min(scan_bad, g.intervals - 1) + 1;
    std::vector<int32_t> first_seg(size_t(g.intervals) + 1, 0);
    int64_t total = 0;
    for (int i = 0; i < g.intervals; ++i) {
        first_seg[size_t(i)] = int32_t(total);
        if (i < nd) total += jpeg_seg_count(start[size_t(i)], jpeg_seg_interval_end(start.data(), g.intervals, i, size), seg_bytes);
    }
    first_seg[size_t(g.intervals)] = int32_t(total);
    const int S = int(total), windows = (S + window - 1) / window;
    std::vector<uint64_t> exit_state(size_t(S), JPEG_SEG_DEAD);
    int64_t max_rounds = 0, stitched = 0, max_bytes = 0;
    // 3. sync, a window at a time: round 0 from the entry states, round r lane j on segment j + r; stores behind the round's loads
    for (int w = 0; w < windows; ++w) {
        const int base = w * window, n = std::min(window, S - base);
        std::vector<JpegSeg> seg(size_t(n), JpegSeg{});
        std::vector<uint64_t> run(size_t(n), 0), next(size_t(n), 0);
        std::vector<uint8_t> done(size_t(n), 0), wrote(size_t(n), 0);
        std::vector<long long> bytes(size_t(n), 0);
        for (int j = 0; j < n; ++j) {
            seg[size_t(j)] = jpeg_seg_at(start.data(), first_seg.data(), nd, seg_bytes, base + j);
            run[size_t(j)] = jpeg_seg_walk(data, size, t, g, jpeg_seg_entry_guess(data, seg[size_t(j)]), seg[size_t(j)].end, bytes[size_t(j)]);
            exit_state[size_t(base + j)] = run[size_t(j)];
            done[size_t(j)] = run[size_t(j)] == JPEG_SEG_DEAD;
        }
        for (int r = 1; r <= window; ++r) {
            bool any = false;
            for (int j = 0; j < n; ++j) {
                wrote[size_t(j)] = 0;
                if (done[size_t(j)]) continue;
                const JpegSeg& sg = seg[size_t(j)];
                if (j + r >= n || sg.q + r >= sg.nq) {      // the window or the interval ends: chains never cross an interval start
                    done[size_t(j)] = 1;
                    continue;
                }
                any = true;
                const uint64_t y = jpeg_seg_walk(data, size, t, g, run[size_t(j)], jpeg_seg_end_of(sg, sg.q + r, seg_bytes), bytes[size_t(j)]);
                if (y == exit_state[size_t(base + j + r)]) done[size_t(j)] = 1;
                else run[size_t(j)] = next[size_t(j)] = y, wrote[size_t(j)] = 1, done[size_t(j)] = y == JPEG_SEG_DEAD;
            }
            if (!any) break;
            for (int j = 0; j < n; ++j)
                if (wrote[size_t(j)]) exit_state[size_t(base + j + r)] = next[size_t(j)];
            max_rounds = std::max<int64_t>(max_rounds, r);
        }
        for (int j = 0; j < n; ++j) max_bytes = std::max<int64_t>(max_bytes, bytes[size_t(j)]);
    }
    // 4. stitch, a lane per interval: over each window boundary inside it with the true state, until a stored state is met
    for (int i = 0; i < nd; ++i) {
        const int s0 = first_seg[size_t(i)], s1 = first_seg[size_t(i) + 1];
        for (int wb = (s0 / window + 1) * window; wb < s1; wb += window) {
            uint64_t state = exit_state[size_t(wb) - 1];
            for (int s = wb; s < s1 && state != JPEG_SEG_DEAD; ++s) {
                const JpegSeg sg = jpeg_seg_at(start.data(), first_seg.data(), nd, seg_bytes, s);
                long long unused = 0;
                const uint64_t y = jpeg_seg_walk(data, size, t, g, state, sg.end, unused);
                ++stitched;
                if (y == exit_state[size_t(s)]) break;
                exit_state[size_t(s)] = state = y;
            }
        }
    }
    // 5. count, and the exclusive scan over each interval's segments
    std::vector<JpegSegCount> count(size_t(S), JpegSegCount{});
    std::vector<int32_t> blk(size_t(S), 0), pred(size_t(S) * 3, 0);
    const auto entry = [&](const JpegSeg& sg, int s) { return sg.q == 0 ? jpeg_seg_entry_guess(data, sg) : exit_state[size_t(s) - 1]; };
    for (int s = 0; s < S; ++s) {
        const JpegSeg sg = jpeg_seg_at(start.data(), first_seg.data(), nd, seg_bytes, s);
        count[size_t(s)] = jpeg_seg_count_blocks(data, size, t, g, entry(sg, s), sg.end);
        count[size_t(s)].dead = exit_state[size_t(s)] == JPEG_SEG_DEAD;
    }
    for (int i = 0; i < nd; ++i) {
        long long at = 0;
        bool dead = false;
        JpegSegMap m[3] = {jpeg_seg_map_identity(), jpeg_seg_map_identity(), jpeg_seg_map_identity()};
        for (int s = first_seg[size_t(i)]; s < first_seg[size_t(i) + 1]; ++s) {
            blk[size_t(s)] = dead ? 0x7FFFFFFF : int32_t(std::min<long long>(at, 0x7FFFFFFF));
            dead = dead || count[size_t(s)].dead != 0;
            for (int c = 0; c < 3; ++c) pred[size_t(s) * 3 + size_t(c)] = jpeg_seg_map_apply(m[c], 0), m[c] = jpeg_seg_map_then(m[c], count[size_t(s)].map[c]);
            at += count[size_t(s)].blocks;
        }
    }
    // 6. write
    alignas(16) int16_t stage[64];
    for (int s = 0; s < S; ++s) {
        const JpegSeg sg = jpeg_seg_at(start.data(), first_seg.data(), nd, seg_bytes, s);
        int16_t* const rec0 = coef.data() + size_t(sg.interval) * size_t(g.ri) * size_t(g.bpm) * 64;
        if (!jpeg_seg_write(data, size, t, g, entry(sg, s), sg.end, blk[size_t(s)], &pred[size_t(s) * 3], jpeg_seg_interval_blocks(g, sg.interval), rec0, stage))
            bad = std::min(bad, sg.interval);
    }
    if (stats != nullptr) {
        stats[0] = nd, stats[1] = S, stats[2] = windows, stats[3] = max_rounds, stats[4] = stitched, stats[5] = max_bytes;
        stats[6] = seg_bytes, stats[7] = 1;
    }
    return bad;
}

// one block's records -> its 8 x 8 samples on its component's plane (the two passes as jpeg_dec_planes_host runs them)
inline void jpeg_dec_block_to_plane(const JpegDecGeom& g, const int16_t* cf, long long m, int b, JpegDecPlanes& out, int rule = JPEG_RULE_OWN) {
    int comp, y0, x0;
    uint8_t smp[8][8];
    jpeg_dec_block_origin(g, m, b, comp, y0, x0);
    jpeg_dec_block_samples(cf, rule, smp);
    uint8_t* dst = out.plane[comp].data() + size_t(y0) * size_t(g.plane_pitch[comp]) + size_t(x0);
    for (int y = 0; y < 8; ++y) std::memcpy(dst + size_t(y) * size_t(g.plane_pitch[comp]), smp[y], 8);
}

// entropy data -> the padded component planes, the entropy stage in the segmented form: what jpeg_dec_planes_host gives
inline void jpeg_dec_planes_seg_host(const whenet_jpeg_info_t& in, const uint8_t* data, int size, int seg_bytes, int window, JpegDecPlanes& out,
                                     int32_t status[2], int64_t stats[8], int rule = JPEG_RULE_OWN) {
    const JpegDecGeom g = jpeg_dec_geom(in);
    std::vector<JpegDecTables> tables(1);
    jpeg_dec_build_tables(in, tables[0]);
    std::vector<int16_t> coef;
    const int bad = jpeg_dec_coef_seg_host(g, tables[0], data, size, seg_bytes, window, coef, stats);
    for (int c = 0; c < g.comps; ++c) out.plane[c].assign(size_t(g.plane_pitch[c]) * size_t(g.plane_rows[c]), 0);
    const long long mcus = (long long)(g.mcu_cols) * g.mcu_rows;
    for (long long m = 0; m < mcus; ++m)
        for (int b = 0; b < g.bpm; ++b) jpeg_dec_block_to_plane(g, coef.data() + (size_t(m) * size_t(g.bpm) + size_t(b)) * 64, m, b, out, rule);
    status[0] = bad == JPEG_DEC_NO_BAD ? WHENET_OK : WHENET_EFORMAT;
    status[1] = bad == JPEG_DEC_NO_BAD ? -1 : bad;
}

}  // namespace whenet
