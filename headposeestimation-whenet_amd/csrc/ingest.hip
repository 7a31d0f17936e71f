// Frame ingest from device memory: packed 3-byte pixels (BGR or RGB) that a decoder's post-processor or a tensor already holds
// in HBM, with a row pitch, -> the slot's tight frame [h][w][3] that the rest of the frame path reads (letterbox.hip, frame.hip).
// A byte copy: the channel order is recorded on the slot.  (The plane-reading twin for NV12 / I420 surfaces is in yuv.hip.)
//
// A thread owns 16 consecutive bytes of one row (the last thread of a row: the 1..15 bytes that are left).  Adjacent lanes own
// adjacent chunks, so a wave reads and writes 1 KiB of a row at a time.
//
// Nothing here assumes an alignment: the source starts wherever a slice starts and its pitch is any number >= 3 w; the frames of
// a clip lie back to back in the output, so a frame's first byte and its row pitch 3 w are aligned to nothing in general.  A dword
// access is taken only at a multiple of 4 and only where all four bytes belong to the chunk: a full chunk whose address is r mod 4
// moves 4 - r head bytes, three aligned dwords (funnel-shifted) and r tail bytes, on the load side and on the store side each with
// its own r.  The last chunk of a row moves its bytes one by one.  No thread reads a byte outside its row's 3 w bytes or writes a
// byte outside its chunk: behind a row's end lies the pitch gap of somebody else's surface, behind a frame's end the next frame.
#include "kernels.h"

namespace whenet {

namespace {

constexpr int THREADS = 256;
constexpr int CHUNK = 16;

__device__ __forceinline__ uint32_t funnel(uint32_t lo, uint32_t hi, int shift_bits) {      // bits [shift, shift + 32) of hi:lo, shift 8..24
    return uint32_t(((uint64_t(hi) << 32) | lo) >> shift_bits);
}

__device__ __forceinline__ void pack_item(const PackFrame& g, uint8_t* __restrict__ out, int item) {
    const int rb = g.row_bytes;
    const int cpr = (rb + CHUNK - 1) / CHUNK;       // chunks per row
    const int r = item / cpr, j = item - r * cpr;
    if (r >= g.h) return;
    const int x = j * CHUNK;
    const int n = min(CHUNK, rb - x);               // bytes of the chunk, 1..16
    const uint8_t* __restrict__ sp = g.src + size_t(r) * size_t(g.pitch) + x;
    uint8_t* __restrict__ dp = out + size_t(r) * size_t(rb) + x;
    if (n < CHUNK) {
        for (int i = 0; i < n; ++i) dp[i] = sp[i];
        return;
    }
    uint32_t w0, w1, w2, w3;                        // the 16 bytes, little-endian
    const int a = int(reinterpret_cast<uintptr_t>(sp) & 3);
    if (a == 0) {
        const uint32_t* s = reinterpret_cast<const uint32_t*>(sp);
        w0 = s[0], w1 = s[1], w2 = s[2], w3 = s[3];
    } else {
        const int head = 4 - a;                     // 1..3 bytes up to the next multiple of 4
        uint32_t hw = 0, tw = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (i < head) hw |= uint32_t(sp[i]) << (8 * i);
        const uint32_t* s = reinterpret_cast<const uint32_t*>(sp + head);
        const uint32_t d0 = s[0], d1 = s[1], d2 = s[2];
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (i < a) tw |= uint32_t(sp[head + 12 + i]) << (8 * i);
        const int up = 8 * head, down = 32 - up;
        w0 = hw | (d0 << up), w1 = funnel(d0, d1, down), w2 = funnel(d1, d2, down), w3 = funnel(d2, tw, down);
    }
    const int b = int(reinterpret_cast<uintptr_t>(dp) & 3);
    if (b == 0) {
        uint32_t* d = reinterpret_cast<uint32_t*>(dp);
        d[0] = w0, d[1] = w1, d[2] = w2, d[3] = w3;
    } else {
        const int head = 4 - b;
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (i < head) dp[i] = uint8_t(w0 >> (8 * i));
        uint32_t* d = reinterpret_cast<uint32_t*>(dp + head);
        d[0] = funnel(w0, w1, 8 * head), d[1] = funnel(w1, w2, 8 * head), d[2] = funnel(w2, w3, 8 * head);
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (i < b) dp[head + 12 + i] = uint8_t(w3 >> (8 * (head + i)));
    }
}

// workgroup b belongs to the last frame whose block0 is <= b (a scan of at most 16 values, the same in every lane)
__global__ __launch_bounds__(THREADS) void whenet_frame_pack_kernel(uint8_t* __restrict__ out, PackFrames clip) {
    const int b = int(blockIdx.x);
    int f = 0;
    for (int i = 1; i < clip.frames; ++i)
        if (clip.f[i].block0 <= b) f = i;
    const PackFrame& g = clip.f[f];
    pack_item(g, out + g.dst_off, (b - g.block0) * THREADS + int(threadIdx.x));
}

int pack_blocks(int h, int row_bytes) {
    const long long items = (long long)h * ((row_bytes + CHUNK - 1) / CHUNK);
    return int((items + THREADS - 1) / THREADS);
}

}  // namespace

// block0 / total_blocks are set here.  The callers have checked the sources (Engine::check_device_plane): the kernel reads h rows
// of row_bytes bytes at the pitch and nothing else.
void launch_frame_pack(uint8_t* d_out, PackFrames clip, hipStream_t stream) {
    WHENET_REQUIRE(d_out != nullptr && clip.frames >= 1 && clip.frames <= MIXED_MAX_FRAMES, WHENET_EINVAL, "frame_pack: 1..16 frames");
    int blocks = 0;
    for (int f = 0; f < clip.frames; ++f) {
        const PackFrame& g = clip.f[f];
        WHENET_REQUIRE(g.src != nullptr && g.h >= 1 && g.h <= LETTERBOX_MAX_FRAME_SIDE && g.row_bytes >= 3 &&
                           g.row_bytes <= 3 * LETTERBOX_MAX_FRAME_SIDE && g.row_bytes % 3 == 0 && g.pitch >= g.row_bytes,
                       WHENET_EINVAL, "frame_pack: bad frame geometry");
        clip.f[f].block0 = blocks;
        blocks += pack_blocks(g.h, g.row_bytes);
    }
    clip.total_blocks = blocks;
    hipLaunchKernelGGL(whenet_frame_pack_kernel, dim3(blocks), dim3(THREADS), 0, stream, d_out, clip);
    WHENET_HIP_CHECK(hipGetLastError());
}

}  // namespace whenet
