// The store stage of the YUV ingest kernels (yuv.hip, yuvx.hip): the 4 pixels of a group leave as dwords wherever the group lies.
// Included inside the file's own unnamed namespace in `namespace whenet`.
#pragma once

__device__ __forceinline__ uint32_t funnel(uint32_t lo, uint32_t hi, int shift_bits) {      // bits [shift, shift + 32) of hi:lo
    return uint32_t(((uint64_t(hi) << 32) | lo) >> shift_bits);
}

// the output stage of an item function: the pixels p0..p3 (B | G << 8 | R << 16) of a group of n = 1..4 pixels go to dp, which is
// aligned to nothing in general.  n == 4: 12 bytes as three dwords, or 4 - a head bytes, two aligned dwords (funnel-shifted) and a
// tail bytes where dp is a mod 4.  n < 4 (the last group of a row): 3 n bytes one by one, the next frame starts behind them.
__device__ __forceinline__ void store_group(uint8_t* __restrict__ dp, int n, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3) {
    const uint32_t w0 = p0 | (p1 << 24), w1 = (p1 >> 8) | (p2 << 16), w2 = (p2 >> 16) | (p3 << 8);
    if (n == 4) {
        const int a = int(reinterpret_cast<uintptr_t>(dp) & 3);
        if (a == 0) {
            uint32_t* d = reinterpret_cast<uint32_t*>(dp);
            d[0] = w0, d[1] = w1, d[2] = w2;
        } else {
            const int head = 4 - a;
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (j < head) dp[j] = uint8_t(w0 >> (8 * j));
            uint32_t* d = reinterpret_cast<uint32_t*>(dp + head);
            d[0] = funnel(w0, w1, 8 * head), d[1] = funnel(w1, w2, 8 * head);
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (j < a) dp[12 - a + j] = uint8_t(w2 >> (8 * (head + j)));
        }
    } else {
        const int nb = 3 * n;                   // 3, 6 or 9 bytes
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const uint32_t word = j < 4 ? w0 : (j < 8 ? w1 : w2);
            if (j < nb) dp[j] = uint8_t(word >> (8 * (j & 3)));
        }
    }
}
