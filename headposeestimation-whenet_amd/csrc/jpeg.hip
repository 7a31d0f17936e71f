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
constexpr int MAX_INTERVAL_BLOCKS = JPEG_MAX_INTERVAL_BLOCKS;           // 3,072 at 4:2:0 and 4:4:4, 2,048 at 4:2:2
static_assert((JPEG_MAX_SIDE / 16) * jpeg_geom(WHENET_JPEG_420).blocks <= MAX_INTERVAL_BLOCKS &&
                  (JPEG_MAX_SIDE / 16) * jpeg_geom(WHENET_JPEG_422).blocks <= MAX_INTERVAL_BLOCKS &&
                  (JPEG_MAX_SIDE / 8) * jpeg_geom(WHENET_JPEG_444).blocks <= MAX_INTERVAL_BLOCKS,
              "the pack kernel's s_off holds the blocks of the widest interval of every sampling");
constexpr int WRITE_BYTES = 16;                                          // bytes per lane and step of the write kernel

template <int S>
__global__ __launch_bounds__(THREADS) void whenet_jpeg_dct_kernel(JpegArgs a) {
    __shared__ int s_r[DCT_BLOCKS][8][9];
    const int tid = int(threadIdx.x), lb = tid >> 3, l = tid & 7;
    const int g = int(blockIdx.x) * DCT_BLOCKS + lb;
    const bool live = g < a.R * a.B;
    int comp = 0;
    if (live) {
        const int interval = g / a.B;
        int y0, x0, p[8], o[8];
        jpeg_block_origin<S>(interval, g - interval * a.B, comp, y0, x0);
#pragma unroll
        for (int x = 0; x < 8; ++x) p[x] = jpeg_sample<S>(a.src, comp, y0 + l, x0 + x) - 128;
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

template <int S, typename Sink>
__device__ inline void interval_block_codes(const int16_t* coef, int i, const uint16_t (*s_code)[256], const uint8_t (*s_len)[256], Sink& sink) {
    const int before = jpeg_block_before<S>(i);
    const int pred = before < 0 ? 0 : coef[size_t(before) * 64];
    const int tb = jpeg_block_is_luma<S>(i) ? 0 : 2;
    jpeg_block_codes(coef + size_t(i) * 64, pred, s_code[tb], s_len[tb], s_code[tb + 1], s_len[tb + 1], sink);
}

// The symbols of an interval's blocks into four LDS histograms, those added into the encode's four global ones.  Counts are
// integers: the order of the additions does not matter.
struct LdsHistogram {
    uint32_t* hist;      // [2][256]: the component's DC and AC counters
    __device__ void symbol(int cls, int sym) { atomicAdd(hist + cls * 256 + sym, 1u); }
};

template <int S>
__global__ __launch_bounds__(THREADS) void whenet_jpeg_hist_kernel(JpegArgs a) {
    __shared__ uint32_t s_hist[4 * 256];
    const int tid = int(threadIdx.x), r = int(blockIdx.x);
    for (int i = tid; i < 4 * 256; i += THREADS) s_hist[i] = 0;
    __syncthreads();
    const int16_t* coef = a.coef + size_t(r) * size_t(a.B) * 64;
    for (int i = tid; i < a.B; i += THREADS) {
        const int before = jpeg_block_before<S>(i);
        LdsHistogram sink{s_hist + (jpeg_block_is_luma<S>(i) ? 0 : 512)};
        jpeg_block_symbols(coef + size_t(i) * 64, before < 0 ? 0 : coef[size_t(before) * 64], sink);
    }
    __syncthreads();
    uint32_t* hist = &a.opt->hist[0][0];
    for (int i = tid; i < 4 * 256; i += THREADS)
        if (s_hist[i] != 0) atomicAdd(hist + i, s_hist[i]);
}

// One workgroup per encode, a wave per table (DC0, AC0, DC1, AC1).  Figure K.1's two searches run over the wave's lanes (the
// least frequency, the larger symbol on a tie: one min over a key); lane 0 merges.  Then lane 0 runs figures K.2 - K.4 and the
// canonical codes, and thread 0 writes the header: jpeg_host.h's functions, the ones the host statement runs.
__global__ __launch_bounds__(THREADS) void whenet_jpeg_table_kernel(JpegArgs a) {
    static_assert(WAVES == 4, "a wave per table");
    __shared__ JpegHuffWork s_k[4];
    __shared__ uint8_t s_bits[4][16], s_vals[4][256];
    __shared__ int s_count[4];
    const int tid = int(threadIdx.x), lane = tid & 63, tb = tid >> 6;
    JpegHuffWork& k = s_k[tb];
    for (int i = lane; i <= 256; i += 64) k.freq[i] = i < 256 ? a.opt->hist[tb][i] : 1u, k.codesize[i] = 0, k.others[i] = -1;
    __syncthreads();
    const auto least = [&](int skip) {
        unsigned long long best = ~0ull;
        for (int i = lane; i <= 256; i += 64) {
            const unsigned long long f = k.freq[i];      // below 2^40: the key fits
            const unsigned long long key = (f << 16) | (unsigned long long)(0x1FF - i);
            if (f != 0 && i != skip && key < best) best = key;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned long long o = __shfl_xor(best, d, 64);
            best = o < best ? o : best;
        }
        return best == ~0ull ? -1 : 0x1FF - int(best & 0xFFFFull);
    };
    for (int step = 0; step < 256; ++step) {      // at most 256 merges of 257 symbols
        const int c1 = least(-1), c2 = least(c1);
        if (c2 >= 0 && lane == 0) jpeg_huff_merge(k, c1, c2);
        if (__syncthreads_or(c2 >= 0) == 0) break;
    }
    if (lane == 0) {
        s_count[tb] = jpeg_huff_finish(k, s_bits[tb], s_vals[tb]);
        jpeg_huff_codes(s_bits[tb], s_vals[tb], a.opt->code[tb], a.opt->len[tb]);
    }
    __syncthreads();
    if (tid == 0) a.opt->header_bytes = jpeg_opt_header(a.tables->header, s_bits, s_vals, s_count, a.opt->header);
}

template <int S>
__global__ __launch_bounds__(THREADS) void whenet_jpeg_pack_kernel(JpegArgs a) {
    __shared__ uint16_t s_code[4][256];
    __shared__ uint8_t s_len[4][256];
    __shared__ int s_off[MAX_INTERVAL_BLOCKS];
    __shared__ int s_wave[WAVES];
    const int tid = int(threadIdx.x), r = int(blockIdx.x);
    for (int i = tid; i < 4 * 256; i += THREADS) {
        s_code[i >> 8][i & 255] = a.code[i >> 8][i & 255];
        s_len[i >> 8][i & 255] = a.len[i >> 8][i & 255];
    }
    __syncthreads();
    const int16_t* coef = a.coef + size_t(r) * size_t(a.B) * 64;
    int carry = 0;
    for (int base = 0; base < a.B; base += THREADS) {
        const int i = base + tid;
        JpegBitCounter c;
        if (i < a.B) interval_block_codes<S>(coef, i, s_code, s_len, c);
        int total;
        const int before = block_exclusive_scan(c.bits, s_wave, total);
        if (i < a.B) s_off[i] = carry + before;      // read back by this lane only
        carry += total;
    }
    uint32_t* buf = a.bits + size_t(r) * size_t(a.interval_dwords);
    for (int i = tid; i < a.B; i += THREADS) {
        DwordBits w(buf, a.interval_dwords, s_off[i]);
        interval_block_codes<S>(coef, i, s_code, s_len, w);
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
    const int header_bytes = a.header_bytes != nullptr ? *a.header_bytes : JPEG_HEADER_BYTES;      // (an optimised encode's own)
    const long long at = header_bytes + (long long)(s_before);
    if (r == 0)
        for (int i = tid; i < header_bytes; i += THREADS)
            if (i < cap) a.dst[i] = a.header[i];
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

JpegScratch::JpegScratch(int h, int w, int sampling) {
    const auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
    geom = jpeg_geom(sampling);
    R = jpeg_mcu_rows(h, sampling), B = jpeg_mcu_cols(w, sampling) * geom.blocks;
    interval_dwords = int((jpeg_interval_bytes(w, sampling) + 3) / 4) + 2;
    coef = 0;
    bits = up(size_t(R) * size_t(B) * 64 * sizeof(int16_t));
    bits_bytes = size_t(R) * size_t(interval_dwords) * sizeof(uint32_t);
    ulen = up(bits + bits_bytes);
    slen = up(ulen + size_t(R) * sizeof(int32_t));
    opt = up(slen + size_t(R) * sizeof(int32_t));
    bytes = up(opt + sizeof(JpegOptTables));
}

JpegArgs jpeg_args(const JpegSource& src, const JpegTables* d_tables, void* d_scratch, const JpegScratch& lay, void* d_dst, long long cap,
                   void* d_size, bool optimize) {
    JpegArgs a{};
    char* const s = static_cast<char*>(d_scratch);
    a.src = src, a.tables = d_tables;
    a.coef = reinterpret_cast<int16_t*>(s + lay.coef), a.bits = reinterpret_cast<uint32_t*>(s + lay.bits);
    a.ulen = reinterpret_cast<int32_t*>(s + lay.ulen), a.slen = reinterpret_cast<int32_t*>(s + lay.slen);
    a.dst = static_cast<uint8_t*>(d_dst), a.cap = cap, a.size = static_cast<long long*>(d_size);
    a.R = lay.R, a.B = lay.B, a.interval_dwords = lay.interval_dwords;
    a.geom = lay.geom;
    if (optimize) {      // the codes, the header and its length are this encode's own, built by the table kernel
        a.opt = reinterpret_cast<JpegOptTables*>(s + lay.opt);
        a.code = a.opt->code, a.len = a.opt->len, a.header = a.opt->header, a.header_bytes = &a.opt->header_bytes;
    } else if (d_tables != nullptr) {
        a.code = d_tables->code, a.len = d_tables->len, a.header = d_tables->header;
    }
    return a;
}

namespace {
template <int S>
void launch_jpeg_stages(const JpegArgs& a, hipStream_t stream) {
    const int nblocks = a.R * a.B;
    hipLaunchKernelGGL(whenet_jpeg_dct_kernel<S>, dim3((nblocks + DCT_BLOCKS - 1) / DCT_BLOCKS), dim3(THREADS), 0, stream, a);
    WHENET_HIP_CHECK(hipGetLastError());
    if (a.opt != nullptr) {
        hipLaunchKernelGGL(whenet_jpeg_hist_kernel<S>, dim3(a.R), dim3(THREADS), 0, stream, a);
        WHENET_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(whenet_jpeg_table_kernel, dim3(1), dim3(THREADS), 0, stream, a);
        WHENET_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(whenet_jpeg_pack_kernel<S>, dim3(a.R), dim3(THREADS), 0, stream, a);
    WHENET_HIP_CHECK(hipGetLastError());
}
}  // namespace

void launch_jpeg_encode(const JpegArgs& a, const JpegScratch& lay, hipStream_t stream) {
    int rows[3], row_bytes[3];
    const int planes = overlay_surface_planes(a.src.format, a.src.h, a.src.w, rows, row_bytes);
    const int S = a.geom.sampling;
    WHENET_REQUIRE(planes > 0 && a.src.h >= 1 && a.src.w >= 1 && a.src.h <= JPEG_MAX_SIDE && a.src.w <= JPEG_MAX_SIDE && a.tables != nullptr &&
                       a.coef != nullptr && a.size != nullptr && a.cap >= 0 && (a.dst != nullptr || a.cap == 0) && jpeg_sampling_ok(S) &&
                       (S == WHENET_JPEG_420 || a.src.format == WHENET_SURF_PACKED),
                   WHENET_EINVAL, "jpeg_encode: bad arguments");
    for (int p = 0; p < planes; ++p)
        WHENET_REQUIRE(a.src.plane[p] != nullptr && a.src.pitch[p] >= row_bytes[p], WHENET_EINVAL, "jpeg_encode: bad plane " + std::to_string(p));
    WHENET_REQUIRE(a.R == jpeg_mcu_rows(a.src.h, S) && a.B == jpeg_mcu_cols(a.src.w, S) * jpeg_geom(S).blocks && a.B <= MAX_INTERVAL_BLOCKS &&
                       a.R == lay.R && a.B == lay.B && a.interval_dwords == lay.interval_dwords && lay.geom.sampling == S &&
                       size_t(a.interval_dwords) * 4 >= size_t(jpeg_interval_bytes(a.src.w, S)) + 8,
                   WHENET_EINVAL, "jpeg_encode: the work buffers are not those of the frame's size and sampling");
    WHENET_HIP_CHECK(hipMemsetAsync(a.bits, 0, lay.bits_bytes, stream));
    if (a.opt != nullptr) WHENET_HIP_CHECK(hipMemsetAsync(a.opt->hist, 0, sizeof(a.opt->hist), stream));
    if (S == WHENET_JPEG_444)
        launch_jpeg_stages<WHENET_JPEG_444>(a, stream);
    else if (S == WHENET_JPEG_422)
        launch_jpeg_stages<WHENET_JPEG_422>(a, stream);
    else
        launch_jpeg_stages<WHENET_JPEG_420>(a, stream);
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
