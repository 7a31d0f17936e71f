// The baseline JPEG encoder on the device: a 4:2:0 JFIF surface (or packed pixels) in, one contiguous stream out.  The format and
// every formula are in include/whenet_hip.h (JPEG ENCODER); the arithmetic -- sample fetch, DCT pass, quantiser, the code words of
// a block -- is jpeg_host.h's, the same functions the host statement runs.  Integers only.
//
// Reference: demo_video.py:46-47, :60 (the annotated frame stored as Motion-JPEG by cv2.VideoWriter).
//
// One restart interval per MCU row makes the rows independent: the DC predictors start at 0 in each, so a block's DC difference
// needs its neighbour of the same component only, and every interval's bits start at a byte of their own.
//   whenet_jpeg_dct_kernel    8 lanes per block.  Lane y fetches row y and runs the row pass; the rounded rows go through LDS; lane u
//                             runs the column pass of column u and quantises its 8 coefficients into the block's zigzag record.
//   whenet_jpeg_pack_kernel   one workgroup per interval.  Pass 1: a lane per block counts the block's bits; the counts are scanned
//                             (wave shuffles + LDS totals) 256 blocks at a time with a running carry.  Pass 2: the lane walks its
//                             block again and ORs the code words, most significant bit first, into the interval's zeroed dwords.
//   whenet_jpeg_count_kernel  0xFF bytes per interval -> stuffed lengths.
//   whenet_jpeg_write_kernel  one workgroup per interval: its offset = header + the stuffed lengths and markers before it; 16 bytes
//                             per lane and step, the 0xFF counts scanned to place every byte; then RSTm or EOI.  Every store is
//                             checked against the destination's capacity; the last interval's workgroup writes the total length.
#include <algorithm>
#include <string>

#include "kernels.h"
#include "jpeg_host.h"

namespace whenet {

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int DCT_BLOCKS = THREADS / 8;                                  // blocks per workgroup of the dct kernel
constexpr int MAX_INTERVAL_BLOCKS = (JPEG_MAX_SIDE / 16) * JPEG_MCU_BLOCKS;      // 3,072
constexpr int WRITE_BYTES = 16;                                          // bytes per lane and step of the write kernel

__global__ __launch_bounds__(THREADS) void whenet_jpeg_dct_kernel(JpegArgs a) {
    __shared__ int s_r[DCT_BLOCKS][8][9];
    const int tid = int(threadIdx.x), lb = tid >> 3, l = tid & 7;
    const int g = int(blockIdx.x) * DCT_BLOCKS + lb;
    const bool live = g < a.R * a.B;
    int comp = 0;
    if (live) {
        const int interval = g / a.B;
        int y0, x0, p[8], o[8];
        jpeg_block_origin(interval, g - interval * a.B, comp, y0, x0);
#pragma unroll
        for (int x = 0; x < 8; ++x) p[x] = jpeg_sample(a.src, comp, y0 + l, x0 + x) - 128;
        jpeg_dct8(p, o);
#pragma unroll
        for (int u = 0; u < 8; ++u) s_r[lb][l][u] = jpeg_dct_round(o[u]);
    }
    __syncthreads();
    if (!live) return;
    int col[8], b[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) col[y] = s_r[lb][y][l];
    jpeg_dct8(col, b);
    const int32_t* q = a.tables->q[comp == 0 ? 0 : 1];
    int16_t* out = a.coef + size_t(g) * 64;
#pragma unroll
    for (int v = 0; v < 8; ++v) out[a.tables->zz_pos[v * 8 + l]] = int16_t(jpeg_quant(b[v], q[v * 8 + l], v + l > 0));
}

// exclusive scan of one int per lane over the workgroup (every lane calls it); total = the sum
__device__ inline int block_exclusive_scan(int v, int* s_wave, int& total) {
    const int lane = int(threadIdx.x) & 63, wave = int(threadIdx.x) >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const int t = s_wave[w];
        base += w < wave ? t : 0;
        total += t;
    }
    __syncthreads();
    return base + inc - v;
}

// Code words into an interval's dwords from bit `at` on.  The dword in hand is OR-ed in when it is full or at the end: a dword's
// other bits belong to the neighbouring blocks' lanes, which OR theirs.  Stored byte-swapped: the memory's bytes are the stream's.
struct DwordBits {
    uint32_t* buf;
    int ndw, w, fill;
    uint32_t cur;
    __device__ DwordBits(uint32_t* b, int n, int at) : buf(b), ndw(n), w(at >> 5), fill(at & 31), cur(0) {}
    __device__ void flush() {
        if (cur != 0 && w < ndw) atomicOr(buf + w, __builtin_bswap32(cur));
    }
    __device__ void put(uint32_t bits, int n) {      // 1 <= n <= 26, fill <= 31
        const uint64_t v = uint64_t(bits) << (64 - fill - n);
        cur |= uint32_t(v >> 32);
        fill += n;
        if (fill >= 32) {
            flush();
            ++w, fill -= 32, cur = uint32_t(v);
        }
    }
};

template <typename Sink>
__device__ inline void interval_block_codes(const int16_t* coef, int i, const uint16_t (*s_code)[256], const uint8_t (*s_len)[256], Sink& sink) {
    const int before = jpeg_block_before(i);
    const int pred = before < 0 ? 0 : coef[size_t(before) * 64];
    const int tb = i % JPEG_MCU_BLOCKS < 4 ? 0 : 2;
    jpeg_block_codes(coef + size_t(i) * 64, pred, s_code[tb], s_len[tb], s_code[tb + 1], s_len[tb + 1], sink);
}

__global__ __launch_bounds__(THREADS) void whenet_jpeg_pack_kernel(JpegArgs a) {
    __shared__ uint16_t s_code[4][256];
    __shared__ uint8_t s_len[4][256];
    __shared__ int s_off[MAX_INTERVAL_BLOCKS];
    __shared__ int s_wave[WAVES];
    const int tid = int(threadIdx.x), r = int(blockIdx.x);
    for (int i = tid; i < 4 * 256; i += THREADS) {
        s_code[i >> 8][i & 255] = a.tables->code[i >> 8][i & 255];
        s_len[i >> 8][i & 255] = a.tables->len[i >> 8][i & 255];
    }
    __syncthreads();
    const int16_t* coef = a.coef + size_t(r) * size_t(a.B) * 64;
    int carry = 0;
    for (int base = 0; base < a.B; base += THREADS) {
        const int i = base + tid;
        JpegBitCounter c;
        if (i < a.B) interval_block_codes(coef, i, s_code, s_len, c);
        int total;
        const int before = block_exclusive_scan(c.bits, s_wave, total);
        if (i < a.B) s_off[i] = carry + before;      // read back by this lane only
        carry += total;
    }
    uint32_t* buf = a.bits + size_t(r) * size_t(a.interval_dwords);
    for (int i = tid; i < a.B; i += THREADS) {
        DwordBits w(buf, a.interval_dwords, s_off[i]);
        interval_block_codes(coef, i, s_code, s_len, w);
        w.flush();
    }
    if (tid == 0) {
        if (carry & 7) {                              // 1-bits up to the end of the last byte
            DwordBits w(buf, a.interval_dwords, carry);
            w.put((1u << (8 - (carry & 7))) - 1u, 8 - (carry & 7));
            w.flush();
        }
        a.ulen[r] = (carry + 7) >> 3;
    }
}

__device__ inline int count_ff(uint32_t d) {
    return int((d & 0xFFu) == 0xFFu) + int((d & 0xFF00u) == 0xFF00u) + int((d & 0xFF0000u) == 0xFF0000u) + int((d >> 24) == 0xFFu);
}

__global__ __launch_bounds__(THREADS) void whenet_jpeg_count_kernel(JpegArgs a) {
    __shared__ int s_wave[WAVES];
    const int tid = int(threadIdx.x), r = int(blockIdx.x);
    const uint32_t* buf = a.bits + size_t(r) * size_t(a.interval_dwords);
    const int nbytes = a.ulen[r];
    const int ndw = min((nbytes + 3) >> 2, a.interval_dwords);      // the bytes behind nbytes are zero: none counts
    int n = 0;
    for (int i = tid; i < ndw; i += THREADS) n += count_ff(buf[i]);
    int total;
    (void)block_exclusive_scan(n, s_wave, total);
    if (tid == 0) a.slen[r] = nbytes + total;
}

__global__ __launch_bounds__(THREADS) void whenet_jpeg_write_kernel(JpegArgs a) {
    __shared__ int s_wave[WAVES];
    __shared__ unsigned long long s_before;
    const int tid = int(threadIdx.x), r = int(blockIdx.x);
    if (tid == 0) s_before = 0;
    __syncthreads();
    unsigned long long mine = 0;
    for (int j = tid; j < r; j += THREADS) mine += (unsigned long long)(a.slen[j]) + 2;
    if (mine != 0) atomicAdd(&s_before, mine);
    __syncthreads();
    const long long cap = a.cap;
    const long long at = JPEG_HEADER_BYTES + (long long)(s_before);
    if (r == 0)
        for (int i = tid; i < JPEG_HEADER_BYTES; i += THREADS)
            if (i < cap) a.dst[i] = a.tables->header[i];
    const uint32_t* buf = a.bits + size_t(r) * size_t(a.interval_dwords);
    const int nbytes = a.ulen[r];
    int carry = 0;
    for (int base = 0; base < nbytes; base += THREADS * WRITE_BYTES) {
        const int first = base + tid * WRITE_BYTES;
        uint32_t d[WRITE_BYTES / 4];
        int n = 0;
#pragma unroll
        for (int j = 0; j < WRITE_BYTES / 4; ++j) {
            const int dw = (first >> 2) + j;
            d[j] = dw * 4 < nbytes && dw < a.interval_dwords ? buf[dw] : 0u;      // (whole bytes behind nbytes are zero)
            n += count_ff(d[j]);
        }
        int total;
        const int before = block_exclusive_scan(n, s_wave, total);
        long long pos = at + first + carry + before;
#pragma unroll
        for (int j = 0; j < WRITE_BYTES; ++j) {
            if (first + j < nbytes) {
                const uint32_t b = (d[j >> 2] >> (8 * (j & 3))) & 0xFFu;
                if (pos < cap) a.dst[pos] = uint8_t(b);
                ++pos;
                if (b == 0xFFu) {
                    if (pos < cap) a.dst[pos] = 0;
                    ++pos;
                }
            }
        }
        carry += total;
    }
    if (tid == 0) {
        const long long end = at + a.slen[r];
        if (end < cap) a.dst[end] = 0xFF;
        if (end + 1 < cap) a.dst[end + 1] = uint8_t(r + 1 < a.R ? 0xD0 + (r & 7) : 0xD9);
        if (r + 1 == a.R) *a.size = end + 2;
    }
}

__global__ __launch_bounds__(THREADS) void whenet_jpeg_flush_kernel(const uint4* src, uint4* dst, const long long* size, long long cap,
                                                                    long long* dst_size) {
    const long long total = *size;
    const long long nvec = ((total < cap ? total : cap) + 15) >> 4;
    for (long long i = (long long)(blockIdx.x) * THREADS + threadIdx.x; i < nvec; i += (long long)(gridDim.x) * THREADS) dst[i] = src[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) *dst_size = total;
}

}  // namespace

JpegScratch::JpegScratch(int h, int w) {
    const auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
    R = jpeg_mcu_rows(h), B = jpeg_mcu_cols(w) * JPEG_MCU_BLOCKS;
    interval_dwords = int((jpeg_interval_bytes(w) + 3) / 4) + 2;
    coef = 0;
    bits = up(size_t(R) * size_t(B) * 64 * sizeof(int16_t));
    bits_bytes = size_t(R) * size_t(interval_dwords) * sizeof(uint32_t);
    ulen = up(bits + bits_bytes);
    slen = up(ulen + size_t(R) * sizeof(int32_t));
    bytes = up(slen + size_t(R) * sizeof(int32_t));
}

JpegArgs jpeg_args(const JpegSource& src, const JpegTables* d_tables, void* d_scratch, const JpegScratch& lay, void* d_dst, long long cap,
                   void* d_size) {
    JpegArgs a{};
    char* const s = static_cast<char*>(d_scratch);
    a.src = src, a.tables = d_tables;
    a.coef = reinterpret_cast<int16_t*>(s + lay.coef), a.bits = reinterpret_cast<uint32_t*>(s + lay.bits);
    a.ulen = reinterpret_cast<int32_t*>(s + lay.ulen), a.slen = reinterpret_cast<int32_t*>(s + lay.slen);
    a.dst = static_cast<uint8_t*>(d_dst), a.cap = cap, a.size = static_cast<long long*>(d_size);
    a.R = lay.R, a.B = lay.B, a.interval_dwords = lay.interval_dwords;
    return a;
}

void launch_jpeg_encode(const JpegArgs& a, const JpegScratch& lay, hipStream_t stream) {
    int rows[3], row_bytes[3];
    const int planes = overlay_surface_planes(a.src.format, a.src.h, a.src.w, rows, row_bytes);
    WHENET_REQUIRE(planes > 0 && a.src.h >= 1 && a.src.w >= 1 && a.src.h <= JPEG_MAX_SIDE && a.src.w <= JPEG_MAX_SIDE && a.tables != nullptr &&
                       a.coef != nullptr && a.size != nullptr && a.cap >= 0 && (a.dst != nullptr || a.cap == 0),
                   WHENET_EINVAL, "jpeg_encode: bad arguments");
    for (int p = 0; p < planes; ++p)
        WHENET_REQUIRE(a.src.plane[p] != nullptr && a.src.pitch[p] >= row_bytes[p], WHENET_EINVAL, "jpeg_encode: bad plane " + std::to_string(p));
    WHENET_REQUIRE(a.R == jpeg_mcu_rows(a.src.h) && a.B == jpeg_mcu_cols(a.src.w) * JPEG_MCU_BLOCKS && a.B <= MAX_INTERVAL_BLOCKS &&
                       a.R == lay.R && a.B == lay.B && a.interval_dwords == lay.interval_dwords &&
                       size_t(a.interval_dwords) * 4 >= size_t(jpeg_interval_bytes(a.src.w)) + 8,
                   WHENET_EINVAL, "jpeg_encode: the work buffers are not those of the frame's size");
    WHENET_HIP_CHECK(hipMemsetAsync(a.bits, 0, lay.bits_bytes, stream));
    const int nblocks = a.R * a.B;
    hipLaunchKernelGGL(whenet_jpeg_dct_kernel, dim3((nblocks + DCT_BLOCKS - 1) / DCT_BLOCKS), dim3(THREADS), 0, stream, a);
    WHENET_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(whenet_jpeg_pack_kernel, dim3(a.R), dim3(THREADS), 0, stream, a);
    WHENET_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(whenet_jpeg_count_kernel, dim3(a.R), dim3(THREADS), 0, stream, a);
    WHENET_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(whenet_jpeg_write_kernel, dim3(a.R), dim3(THREADS), 0, stream, a);
    WHENET_HIP_CHECK(hipGetLastError());
}

void launch_jpeg_flush(const void* d_stream, void* to, const long long* d_size, long long cap, long long* to_size, hipStream_t stream) {
    WHENET_REQUIRE(d_stream != nullptr && to != nullptr && d_size != nullptr && to_size != nullptr && cap >= 0 &&
                       reinterpret_cast<uintptr_t>(d_stream) % 16 == 0 && reinterpret_cast<uintptr_t>(to) % 16 == 0,
                   WHENET_EINVAL, "jpeg_flush: bad arguments");
    const long long nvec = (cap + 15) >> 4;
    const int grid = int(std::min<long long>(64, std::max<long long>(1, (nvec + THREADS - 1) / THREADS)));
    hipLaunchKernelGGL(whenet_jpeg_flush_kernel, dim3(grid), dim3(THREADS), 0, stream, static_cast<const uint4*>(d_stream),
                       static_cast<uint4*>(to), d_size, cap, to_size);
    WHENET_HIP_CHECK(hipGetLastError());
}

}  // namespace whenet
