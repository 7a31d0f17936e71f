// Launchers of the hand-written gfx950 kernels.  Every launcher enqueues exactly one kernel
// on `stream` and returns; `dtype` selects the float / _Float16 instantiation.
#pragma once

#include <string>
#include <vector>

#include "common.h"
#include "overlay_host.h"
#include "jpeg_host.h"
#include "jpeg_dec_host.h"
#include "jpeg_dec_seg_host.h"
#include "jpeg_dec_clip_host.h"
#include "jpeg_prog_host.h"
#include "yuvx_host.h"

namespace whenet {

// ---- stem.hip ---------------------------------------------------------------------------
// uint8 crops -> LUT normalise (whenet.py:23-26) -> Conv3x3/s2 'same' + BN + Swish.
struct StemArgs {
    const uint8_t* in;     // [n,224,224,3]
    void* out;             // [n,112,112,32] T
    const float* w;        // [27][32]
    const float* bias;     // [32]
    const float* lut;      // [3][256]
    int n;
    const float* in_f32 = nullptr;   // != NULL: the normalised float32 image [n,224,224,3] instead of `in`
};
void launch_stem(const StemArgs& a, int dtype, hipStream_t stream);

// ---- dw.hip -----------------------------------------------------------------------------
// Depthwise kxk conv (TF 'same') + BN + Swish, NHWC, LDS-staged halo tiles, plus the
// per-tile channel sums the squeeze-excite mean is built from.
struct DwPlan {
    int threads = 256;     // block size (128 for the stride-2 layers: 4x input footprint)
    int CV = 1;            // 16-byte channel vectors per block
    int TH = 1;            // output rows per block
    int NSX = 1;           // 7-pixel output strips per tile row  (tile width = 7*NSX)
    int tiles_x = 1, tiles_y = 1, chunks = 1;
    int IH = 0, IW = 0;    // input tile (with halo)
    size_t lds_bytes = 0;
    int ntiles() const { return tiles_x * tiles_y; }
};
DwPlan plan_dw(int dtype, int k, int s, int H, int Ho, int C);

struct DwArgs {
    const void* in;        // [n,H,H,C] T
    void* out;             // [n,Ho,Ho,C] T
    const float* w;        // [k*k][C]
    const float* bias;     // [C]
    float* partial;        // [n][ntiles][C]  sums of the tile's outputs (pre-rounding f32)
    int k, s, H, Ho, C, pad, n;
    DwPlan plan;
};
void launch_dw(const DwArgs& a, int dtype, hipStream_t stream);

// ---- se.hip -----------------------------------------------------------------------------
// SEBlock: mean over H,W -> Conv1x1+bias -> Swish -> Conv1x1+bias -> sigmoid.
struct SeArgs {
    const float* partial;  // [n][ntiles][C]
    int ntiles;
    float inv_hw;
    const float* w1t;      // [R][C]  se_reduce kernel, transposed
    const float* b1;       // [R]
    const float* w2c;      // [C][RP]  se_expand kernel, channel-major, R zero-padded to RP
    const float* b2;       // [C]
    void* gate;            // [n][C], float or (gate_f16) half: the type of the activations it multiplies
    int C, R, n;
    int gate_f16 = 0;
};
void launch_se(const SeArgs& a, hipStream_t stream);
// second half of the SEBlock when the producer (front.hip) already applied the reduce conv to its
// channel sums: r = swish(b1 + sum of the crop's np partial vectors / (H*W)) -> excite -> sigmoid
struct SeExciteArgs {
    const float* rpart;    // [n][np][RP]
    int np;
    float inv_hw;
    const float* b1;       // [R]
    const float* w2c;      // [C][RP]
    const float* b2;       // [C]
    void* gate;            // [n][C], float or (gate_f16) half
    int C, R, n;
    int gate_f16 = 0;
};
void launch_se_excite(const SeExciteArgs& a, hipStream_t stream);
int se_excite_split(int C);     // workgroups per crop
int se_padded_r(int R);

// ---- pw.hip -----------------------------------------------------------------------------
// 1x1 convolution as an MFMA GEMM over M = n*H*W rows:
//   out[m][:] = act( (a[m][:] * gate[m / HW][:]) @ W + bias ) (+ res[m][:])
enum { ACT_NONE = 0, ACT_SWISH = 1 };
struct SeFuse {            // second half of a SEBlock computed by the project GEMM itself (se_device.h)
    const float* rpart = nullptr;    // [n][np][RP] producer's squeeze-excite partial vectors, or nullptr (not fused)
    const float* b1 = nullptr;       // [R]
    const float* w2c = nullptr;      // [C][RP] excite kernel, channel-major, R zero-padded to RP
    const float* b2 = nullptr;       // [C]
    int np = 0, R = 0, RP = 0;
    float inv_hw = 0.f;
    // round 6 (GM = 3, the LDS-staged split-K kernel): every wave computes the gate of the k-groups IT owns on the matrix cores from
    // this operand image of the excite kernel ([ceil(R/16)][K/32][64 lanes][8] binary16; f32s: [hi | lo] images scaled by 2^shift)
    const void* w2p = nullptr;
    int KSr = 0;                     // ceil(R / 16)
    float w2_wsi = 1.0f;             // f32s: 2^-shift
};
struct PwArgs {
    const void* a;         // [M][K] T
    const void* wp;        // packed MFMA operand image (snapshot.h)
    const float* wdense;   // [K][N] (check kernel only)
    const float* bias;     // [N]
    const void* gate;      // [n][K] T or nullptr
    const void* res;       // [M][N] T or nullptr
    void* out;             // [M][N] T
    int M, K, N, KS, NTILES, HW, act;
    SeFuse se;             // set: the kernel computes the gate of its rows' crops itself (gate must be nullptr)
    // WHENET_F32S: float storage, products as binary16 hi/lo pairs on the f16 matrix pipe (pw.hip PwOps<float, true>)
    bool split = false;
    const void* wps = nullptr;     // [hi image | lo image], f16 fragment order (snapshot.cpp::pack_pw_split)
    int KSs = 0;                   // ceil(K / 16)
    float wsi = 1.0f;              // 2^-shift of the scaled weights
    bool staged = true;            // K >= 320: activation rows fetched coalesced and staged through LDS (whenet_pw_splitk_staged_kernel)
    // f16 split-K kernels (K >= 320): `out` / `res` in the 16-channel blocked layout [crop][N/16][HW][16]
    bool out_blocked = false, res_blocked = false;
    bool static_form = false;      // ask for the kernel with the layer's shape as compile-time constants; taken only where the launch
                                   // is a row of pw.hip's shape table (pw_static_row); same bits either way (engine option "pw_static")
};
void launch_pw(const PwArgs& a, int dtype, int impl, int num_cus, hipStream_t stream);
int pw_static_row(const PwArgs& a, int dtype, int impl, int num_cus);   // the row whose static form launch_pw(a) runs, or -1 (the generic form)
void pw_static_check(int row, const PwArgs& a, int num_cus);            // throws WHENET_EINVAL unless the row's constexpr shape equals a's, field by field
int pw_static_selftest(int row, int field, int delta);                  // (tests) the same check on a static shape with one field moved

// ---- head.hip ---------------------------------------------------------------------------
// GlobalAveragePooling2D + Dense(120|66|66) + softmax-expectation decode + argmax
// (whenet.py:10-13, 28-33; utils.py:7-11).
struct HeadsArgs {
    const void* x;         // [n][49][1280] T  (head conv output), or nullptr with feat_in
    const float* feat_in;  // [n][1280] (decode-only / tests) or nullptr
    const float* logits_in;// [n][252] decode-only or nullptr
    const float* w;        // [1280][252]
    const float* b;        // [252]
    float* feat;           // [n][1280] or nullptr
    float* logits;         // [n][252] or nullptr
    float* ypr;            // [n][3]
    int32_t* argmax;       // [n][3] or nullptr
    int n;
};
void launch_heads(const HeadsArgs& a, int dtype, hipStream_t stream);
// the same stage over heads_split() workgroups per crop; part: [n][heads_split()][252] floats of scratch,
// count: [n] counters that are zero before the first launch (the kernel leaves them zero)
void launch_heads_split(const HeadsArgs& a, float* part, unsigned* count, int dtype, hipStream_t stream);
int heads_split();

// ---- head7.hip --------------------------------------------------------------------------
// head conv 1x1 (320 -> 1280) + BN + Swish fused with GlobalAveragePooling2D (whenet.py:8-10), f16 and f32: only the pooled
// features leave the kernel.  A group of crops per workgroup, every crop on its own two MFMA strips (batch-invariant).
struct Head7Args {
    int dtype;             // WHENET_F16 / WHENET_F32
    const void* x;         // [n,7,7,K] T
    const void* wep;       // packed head-conv weights (MFMA fragment order, snapshot.h)
    const float* bias;     // [N]
    float* feat;           // [n][N] pooled features, f32
    int K, N, NTILES, n;
    // WHENET_F32S: products as binary16 hi/lo pairs (device_math.h PwOps<float, true>)
    bool split = false;
    const void* weps = nullptr;    // [hi image | lo image]
    float wsi = 1.0f;
    bool xcd_grouped = false;      // the channel chunks of a crop group on one XCD (device_math.h xcd_unit)
    bool x_blocked = false;        // f16: x is [n][K/16][49][16] (the blocked layout)
};
bool head7_supported(int dtype, int K, int N, int HW);
void launch_head7(const Head7Args& a, hipStream_t stream);
std::string kernel_name_head7(int dtype, int n, bool split = false);

// ---- stemdw.hip -------------------------------------------------------------------------
// stem conv + BN + Swish fused with block 1's depthwise 3x3 + BN + Swish (whenet.py:8, 23-26), f16 and f32: the 112 x 112 x 32 stem
// output only exists as LDS tiles.  Bitwise the two kernels' results; the tile is plan_dw()'s block-1 plan.
// what every workgroup would otherwise rebuild from the f32 tensors: built once per model on the host (build_stemdw_table),
// with the roundings stem.hip applies on the device
struct StemDwTable {
    uint32_t lut[3 * 256];          // the normalisation LUT as binary16 hi | lo << 16 (v = hi + lo)
    half8 whi[3][64], wlo[3][64];   // stem weights split the same way, as MFMA fragments per kernel row and lane
};
void build_stemdw_table(const float* w /* [27][32] */, const float* lut /* [3][256] */, StemDwTable* out);

struct StemDwArgs {
    int dtype;             // WHENET_F16 / WHENET_F32
    const uint8_t* in;     // [n,224,224,3]
    void* out;             // [n,112,112,32] T: block 1's depthwise output
    const StemDwTable* tab;// (device) f16
    const float* w;        // f32: stem [27][32]
    const float* lut;      // f32: [3][256]
    const float* bias;     // stem [32]
    const float* wd;       // depthwise [9][32]
    const float* bd;       // depthwise bias [32]
    float* partial;        // [n][56 tiles][32] channel sums for se.hip
    int n;
};
bool stemdw_supported(int dtype, const DwPlan& p, int k, int s, int H, int C);
void launch_stemdw(const StemDwArgs& a, hipStream_t stream);
const char* kernel_name_stemdw(int dtype);

// ---- front.hip --------------------------------------------------------------------------
// expand 1x1 (MFMA) + BN + Swish -> depthwise kxk + BN + Swish in one kernel (blocks 2..16).
struct FrontPlan {
    int threads = 256;     // lanes per workgroup (the tile is planned for 256 tap lanes; the extra
                           // waves only share the expand tasks)
    int CC = 32;           // expanded channels per workgroup
    int TH = 1, NSX = 1;   // output tile: TH rows x 7*NSX columns
    int tiles_x = 1, tiles_y = 1, chunks = 1;
    int EH = 0, EW = 0;    // LDS tile of the expanded input (with halo)
    int EP = 0;            // pixel pitch of that tile in bytes (channels + bank-conflict padding)
    int w_off = 0;         // byte offset of the depthwise taps in LDS
    size_t lds_bytes = 0;
    int ntiles() const { return tiles_x * tiles_y; }
};
FrontPlan plan_front(int dtype, int k, int s, int H, int Ho, int Cexp);
std::vector<FrontPlan> plan_front_candidates(int dtype, int k, int s, int H, int Ho, int Cexp,
                                             std::vector<double>* scores);
int front_threads(const FrontPlan& p, int n);    // lanes per workgroup for a launch of n crops (256 | 512)
struct FrontArgs {
    const void* x;         // [n,H,H,Cin] T  block input
    const void* wep;       // packed expand weights (MFMA fragment order)
    const float* be;       // [Cexp]
    const float* wd;       // [k*k][Cexp]
    const float* bd;       // [Cexp]
    void* out;             // [n,Ho,Ho,Cexp] T
    float* rpart;          // w1t != NULL: [n][ntiles][chunks][RP] this workgroup's share of the SE reduce conv
                           // (unscaled);  w1t == NULL: [n][ntiles][Cexp] the tile's channel sums (for launch_se)
    const float* w1t;      // [R][Cexp] se_reduce kernel, transposed, or NULL
    int R;
    int k, s, H, Ho, Cin, Cexp, pad, KSe, NTe, n;
    FrontPlan plan;
    // WHENET_F32S: the expand's products as binary16 hi/lo pairs (device_math.h PwOps<float, true>)
    bool split = false;
    const void* weps = nullptr;    // [hi image | lo image] of the expand weights
    int KSes = 0;                  // ceil(Cin / 16)
    float wsi = 1.0f;
    const float* in_gate = nullptr; // split only: [n][Cin] f32 -- the expand contracts (in_gate[crop] * x): block 2 fed by block 1's
                                    // depthwise output with block 1's project folded into weps (engine.cpp, option fold12)
    bool xcd_grouped = false;       // the channel chunks of a (crop, tile) on one XCD (device_math.h xcd_unit; engine option "xcd_map")
    bool static_form = false;       // ask for the kernel with the layer's geometry as compile-time constants; taken only where the launch
                                    // is a row of front.hip's shape table (front_static_row); same bits either way (engine option "front_static")
};
void launch_front(const FrontArgs& a, int dtype, hipStream_t stream);
// static_row >= 0: whenet_front_kernel<..., false, false, static_row>, the row's geometry as compile-time constants
std::string kernel_name_front(int dtype, int k, int s, int threads, int static_row = -1);
int front_static_row(const FrontArgs& a, int dtype);            // the row whose static form launch_front(a) runs, or -1 (the generic form)
void front_static_check(int row, const FrontArgs& a);           // throws WHENET_EINVAL unless the row's constexpr shape equals a's, field by field
int front_static_selftest(int row, int field, int delta);       // (tests) the same check on a static shape with one field moved

// ---- front2.hip -------------------------------------------------------------------------
// f16: the same stage with the depthwise taps on the matrix cores (per-channel Toeplitz products,
// v_mfma_f32_4x4x4_16B_f16) and the expanded tile channel-major in LDS.
struct Front2Plan {
    int threads = 256;     // lanes per workgroup (256 | 512)
    int CC = 32;           // expanded channels per workgroup (multiple of 32, or the whole layer)
    int TH = 7;            // output rows per tile (multiple of 7)
    int TXG = 1;           // 4-pixel output groups per tile row
    int xs = 0;            // tile origin moved this many pixels to the left (0 | 2)
    int tiles_x = 1, tiles_y = 1, chunks = 1;
    int EH = 0, EWp = 0;   // LDS tile of the expanded input: rows, pixels per row (multiple of 4)
    int RP = 0, CP = 0;    // row / channel pitch in bytes
    int off_stage = 0, off_red = 0, off_sum = 0;
    size_t lds_bytes = 0;
    int ntiles() const { return tiles_x * tiles_y; }
};
Front2Plan make_front2_plan(int k, int s, int Ho, int Cexp, int CC, int TH, int TXG, int threads, int xs);
Front2Plan plan_front2(int k, int s, int H, int Ho, int Cexp);
std::vector<Front2Plan> plan_front2_candidates(int k, int s, int Ho, int Cexp);
int front2_threads(const Front2Plan& p, int n);
std::vector<half_t> pack_dw_toeplitz(const std::vector<float>& w, int k, int s, int C, int xs);
bool front2_preferred(int k, int s, int H, int Cexp);
struct Front2Args {
    const void* x;         // [n,H,H,Cin] half  block input
    const void* wep;       // packed expand weights (MFMA fragment order, snapshot.h)
    const float* be;       // [Cexp]
    const void* wdt;       // pack_dw_toeplitz() image of the depthwise kernel (for plan.xs)
    const float* bd;       // [Cexp]
    void* out;             // [n,Ho,Ho,Cexp] half
    float* rpart;          // as FrontArgs::rpart
    const float* w1t;      // [R][Cexp] se_reduce kernel, transposed, or NULL
    const float* in_gate;  // [n][Cin] f32 or NULL: the expand contracts (in_gate[crop] * x) -- block 2 fed by block 1's
                           // depthwise output with block 1's project folded into wep (engine.cpp, option fold12);
                           // wep is then the F32 fragment image (8 floats per lane, HostModel::fold12_w32)
    int R;
    int k, s, H, Ho, Cin, Cexp, pad, KSe, NTe, n;
    Front2Plan plan;
    bool xcd_grouped = false;       // as FrontArgs::xcd_grouped
    bool static_form = false;       // run the static-plan form of the kernel where front2_tuned.inc's row has one and this launch
                                    // is that row's layer and plan (front2_static_row); same bits either way (engine option "front2_static")
};
void launch_front2(const Front2Args& a, hipStream_t stream);
// static_row >= 0: whenet_front2_static_kernel<..., static_row>, the plan of front2_tuned.inc's row as compile-time constants
std::string kernel_name_front2(int k, int s, int kse, int threads, int xs, bool gated, int static_row = -1);
int front2_static_row(const Front2Args& a);                   // the row whose static form launch_front2(a) runs, or -1 (the generic form)
void front2_static_check(int row, const Front2Args& a);       // throws WHENET_EINVAL unless the row's constexpr plan equals a's, field by field
int front2_static_selftest(int row, int field, int delta);    // (tests) the same check on a static plan with one field moved

// ---- front2s.hip ------------------------------------------------------------------------
// WHENET_F32S (float32 storage): the same stage with both convolutions on the matrix cores -- expand as binary16 hi/lo
// products (PwOps<float, true>), taps as per-channel Toeplitz products, tile in LDS at float32 precision.
struct Front2sArgs {
    const void* x;         // [n,H,H,Cin] float, or (pre) [n,H,H][hi Cin | lo Cin] binary16 pairs written by the producer
    const void* weps;      // [hi image | lo image] of the expand weights (snapshot.cpp::pack_pw_split)
    const float* be;       // [Cexp]
    const void* wdt;       // pack_dw_toeplitz_s() image of the depthwise kernel for tap mode tm
    const float* bd;       // [Cexp]
    void* out;             // [n,Ho,Ho,Cexp] float
    float* rpart;          // as FrontArgs::rpart
    const float* w1t;      // [R][Cexp] se_reduce kernel, transposed, or NULL
    int R;
    int k, s, H, Ho, Cin, Cexp, pad, KSe, NTe, n;
    float wsi = 1.0f;      // 2^-shift of the scaled expand weights
    float wsi_d = 1.0f;    // 2^-shift of the scaled depthwise taps (tm = 1)
    int tm = 2;            // taps: 1 = binary16 hi/lo pairs on v_mfma_f32_4x4x4_16B_f16, 2 = exact float32 on v_mfma_f32_4x4x1_16B_f32
    bool pre = false;      // x is in the pre-split pair form
    Front2Plan plan;       // from make_front2s_plan() (16 bytes per 4-pixel group)
};
bool front2s_supported(int k, int s, int H, int Cin);
bool front2s_preferred(int k, int s, int H, int Cexp);
Front2Plan make_front2s_plan(int k, int s, int Ho, int Cexp, int CC, int TH, int TXG, int threads);
Front2Plan plan_front2s(int k, int s, int H, int Ho, int Cexp, int* tm);
std::vector<Front2Plan> plan_front2s_candidates(int k, int s, int Ho, int Cexp);
std::vector<float> pack_dw_toeplitz_s(const std::vector<float>& w, int k, int s, int C, int tm, float* wsi);
void launch_front2s(const Front2sArgs& a, hipStream_t stream);
std::string kernel_name_front2s(int k, int s, int kse, int threads, int tm, bool pre);

// ---- front7.hip -------------------------------------------------------------------------
// the 7 x 7 blocks (13-16), both dtypes: the same stage with a GROUP of G crops per workgroup, the image-only LDS tile (no halo)
// and the chunk's expand weights staged once in LDS (round 4).
struct Front7Plan {
    int threads = 512;     // lanes per workgroup (256 | 512)
    int G = 4;             // crops per workgroup
    int CC = 64;           // expanded channels per workgroup (32 | 64 | 128)
    int chunks = 1;
    int off_w = 0, off_stage = 0, off_red = 0, off_sum = 0;
    size_t lds_bytes = 0;
};
Front7Plan make_front7_plan(int dtype, int Cin, int Cexp, int G, int CC, int threads);
Front7Plan front7_plan_for(int dtype, int Cin, int Cexp, int n);
bool front7_supported(int k, int s, int H, int Cin);
struct Front7Args {
    int dtype = WHENET_F16;
    const void* x;         // [n,7,7,Cin] T  block input
    const void* wep;       // packed expand weights (MFMA fragment order, snapshot.h)
    const float* be;       // [Cexp]
    const void* wdt;       // f16: pack_dw_toeplitz(w, k, 1, Cexp, 4 - k / 2) image of the depthwise kernel; f32: the kernel, [k*k][Cexp]
    const float* bd;       // [Cexp]
    void* out;             // [n,7,7,Cexp] T
    float* rpart;          // [n][chunks][RP] this workgroup's share of the SE reduce conv, per crop (unscaled)
    const float* w1t;      // [R][Cexp] se_reduce kernel, transposed
    int R;
    int k, Cin, Cexp, NTe, n;
    Front7Plan plan;
    // WHENET_F32S: the expand's products as binary16 hi/lo pairs (device_math.h PwOps<float, true>)
    bool split = false;
    const void* weps = nullptr;    // [hi image | lo image] of the expand weights
    float wsi = 1.0f;
    bool xcd_grouped = false;      // the channel chunks of a crop group on one XCD (device_math.h xcd_unit)
    bool x_blocked = false;        // f16: x is [n][Cin/16][49][16] (the blocked layout)
};
void launch_front7(const Front7Args& a, hipStream_t stream);
std::string kernel_name_front7(int dtype, int k, const Front7Plan& p, bool split = false);

// ---- mb7.hip ----------------------------------------------------------------------------
// f16, blocks 13-16 (7 x 7 maps, 192 -> 1152 -> 192 | 320): the whole MBConv block -- expand, depthwise, squeeze-excite, gate, project,
// skip -- as ONE launch, one workgroup per crop, every intermediate tensor in LDS (round 6).
struct Mb7Args {
    const void* x;         // [n,7,7,192] half  block input (also the skip operand)
    const void* wep;       // packed expand weights (MFMA fragment order, snapshot.h)
    const float* be;       // [1152]
    const void* wds;       // pack_mb7_taps() image of the depthwise kernel
    const float* bd;       // [1152]
    const void* w1p;       // pack_mb7_se(): se_reduce kernel, binary16 [1152][6][8]
    const float* b1;       // [48]
    const void* w2p;       // pack_mb7_se(): se_expand kernel, binary16 [6][1152][8]
    const float* b2;       // [1152]
    const void* wpp;       // packed project weights (MFMA fragment order)
    const float* bp;       // [Cout]
    void* out;             // [n,7,7,Cout] half
    void* dbg_dw = nullptr;    // single-stage calls (tests): the depthwise output [n,7,7,1152] half ...
    void* dbg_gate = nullptr;  // ... and the gate [n,1152] half; nullptr in the forward pass
    int k, Cout, n;
    bool skip;
};
bool mb7_supported(int dtype, int k, int s, int H, int Cin, int Cexp, int R, int Cout, bool skip);
std::vector<half_t> pack_mb7_taps(const std::vector<float>& w /* [k*k][C] */, int k, int C);
void pack_mb7_se(const std::vector<float>& w1t /* [R][C] */, const std::vector<float>& w2 /* [R][C] */, int C, int R,
                 std::vector<half_t>* w1p, std::vector<half_t>* w2p);
void launch_mb7(const Mb7Args& a, hipStream_t stream);
std::string kernel_name_mb7(int k, int Cout, bool skip);

// ---- frames of different sizes in one clip (letterbox.hip, yolo.hip, headplan.hip, frame.hip) --
// The stages before and after the detector body depend on the frame size; their mixed forms take one geometry record per frame,
// passed BY VALUE in the kernel's argument block (16 records: 1.8 KB): no copy is enqueued and no host buffer can be overwritten
// while a launch that reads it is still queued.  The frames lie back to back in one buffer, without padding.
constexpr int MIXED_MAX_FRAMES = 16;
struct MixedFrameCorrection {                   // yolo_correct_boxes of one image (model.py:158-162), float32 as for one image
    float image_h, image_w, off_y, off_x, scale_y, scale_x;
};
MixedFrameCorrection yolo_correction(float input_h, float input_w, float image_h, float image_w);

// ---- yolo.hip ---------------------------------------------------------------------------
// YOLOv3 post-processing (yolo_v3/model.py:125-232): decode + score threshold + per-class NMS.
struct YoloLayer {
    const float* feats;    // device [gh][gw][A*(5+C)] (a batch: [images][gh][gw][A*(5+C)])
    int gh, gw;
    int first;             // index of this layer's first box in the concatenated list
    float anchor[3][2];    // (w, h) of the layer's anchors (anchor_mask applied)
};
struct YoloArgs {
    YoloLayer layer[3];
    int num_layers, num_classes, na;       // na = anchors per layer (3)
    int N, NP;                             // boxes in total; key capacity per class (power of two >= N)
    float input_h, input_w, image_h, image_w;
    float off_y, off_x, scale_y, scale_x;  // letterbox correction (model.py:160-162), float32 as the graph computes it
    float score_thr, iou_thr;
    int max_boxes;
    int images;                            // 0 / 1: one image; F: every array below has a leading [F] axis (grid dimension y)
    float* boxes;                          // [N][4] y_min, x_min, y_max, x_max
    float* all_scores;                     // [N][C] or nullptr (tests)
    int* counts;                           // [C]
    unsigned long long* keys;              // [C][NP]
    float* out_boxes;                      // [C][max_boxes][4]
    float* out_scores;                     // [C][max_boxes]
    int* out_index;                        // [C][max_boxes]
    int* out_count;                        // [C]
};
struct YoloMixed {                              // the correction of image blockIdx.y instead of the one set in YoloArgs
    MixedFrameCorrection img[MIXED_MAX_FRAMES];
};
// mixed != nullptr: image f of the batch is corrected with mixed->img[f] (a.images <= MIXED_MAX_FRAMES)
void launch_yolo_eval(const YoloArgs& a, hipStream_t stream, const YoloMixed* mixed = nullptr);
int yolo_max_select();

// ---- frame.hip --------------------------------------------------------------------------
// Per-head pre-processing of a frame (demo_video.py:13-24): bbox margins -> crop window ->
// (BGR->RGB) -> cv2.resize-compatible fixed-point bilinear to 224x224 uint8.
constexpr int CROP_PLAN_INTS = 8 + 6 * IMG;     // header {y0,x0,h,w,area2x,xmax,-,-} + xofs|a0|a1|yofs|b0|b1
void frame_box_rect(int frame_h, int frame_w, const float bbox[4], int32_t rect[4]);
void build_crop_plan(const int32_t rect[4], int32_t* plan);
void launch_crop_resize(const uint8_t* d_frame, int fw, int swap_rb, const int32_t* d_plan, int k, uint8_t* d_out,
                        hipStream_t stream);
// The same over a CAPACITY of k rows whose head count is on the device: row i is cropped iff i < *d_count and d_valid[i] != 0
// (headplan.hip writes both); every other row is filled with zero bytes.  Valid rows: the arithmetic above, unchanged.
void launch_crop_resize_masked(const uint8_t* d_frame, int fw, int swap_rb, const int32_t* d_plan, int k, const int32_t* d_valid,
                               const int32_t* d_count, uint8_t* d_out, hipStream_t stream);
// The gathering form over the frames of a clip [F][fh][fw][3]: output row r is the crop of slot s = d_slot_of_row[r] (headplan.hip's
// compaction) with plan d_plan[s], cut from frame s / slots_per_frame; a row with s < 0 is filled with zero bytes.
void launch_crop_resize_gather(const uint8_t* d_frames, size_t frame_bytes, int fw, int swap_rb, const int32_t* d_plan, int slots_per_frame,
                               const int32_t* d_slot_of_row, int rows, uint8_t* d_out, hipStream_t stream);

// The same over the frames of a MIXED clip: the frame of slot s starts frame_off[s / slots_per_frame] bytes into d_frames and is
// fw[.] pixels wide.
struct CropFrames {
    unsigned long long frame_off[MIXED_MAX_FRAMES];
    int fw[MIXED_MAX_FRAMES];
};
void launch_crop_resize_gather_mixed(const uint8_t* d_frames, const CropFrames& frames, int swap_rb, const int32_t* d_plan,
                                     int slots_per_frame, const int32_t* d_slot_of_row, int rows, uint8_t* d_out, hipStream_t stream);

// ---- headplan.hip -----------------------------------------------------------------------
// The detector's selected boxes (yolo.hip's out_boxes / out_scores / out_count, left where launch_yolo_eval wrote them) ->
// the detections concatenated class by class, their crop windows (frame_box_rect), which of them have a window inside the
// frame (check_rects of engine_post.cpp) and the crop plan of each (build_crop_plan), bit for bit the host's.
struct HeadPlanArgs {
    const float* in_boxes;     // [C][max_boxes][4]
    const float* in_scores;    // [C][max_boxes] or nullptr (scores come out as 0)
    const int* in_count;       // [C]
    int num_classes, max_boxes;
    int frame_h, frame_w;
    int frames;                // 0 / 1: one frame; F: inputs [F][C]..., outputs [F][K]..., count [F] (grid dimension y), one frame size
    // outputs over the capacity K = C * max_boxes; rows from *count on: zeros, class -1, valid 0
    float* boxes;              // [K][4]
    float* scores;             // [K]
    int32_t* classes;          // [K]
    int32_t* count;            // [1]
    int32_t* rects;            // [K][4] (y0, x0, y1, x1)
    int32_t* valid;            // [K]
    int32_t* plans;            // [K][CROP_PLAN_INTS] or nullptr; zeros where valid is 0
};
struct HeadPlanSizes {                          // a mixed clip: the size of frame blockIdx.y instead of a.frame_h / a.frame_w
    int frame_h[MIXED_MAX_FRAMES], frame_w[MIXED_MAX_FRAMES];
};
void launch_head_plan(const HeadPlanArgs& a, hipStream_t stream, const HeadPlanSizes* mixed = nullptr);
// Compaction of a clip's heads: slot s = f * K + i (s < F * K <= 1024) is LIVE iff valid[s] != 0 and i < count[f].  The r-th
// live slot in slot order gets row[s] = r if r < max_heads; every other slot gets row -1.  slot_of_row [max_heads] is the
// inverse (-1: an empty row), *rows_used = min(live, max_heads), *overflow = live - *rows_used.  One workgroup, no atomics.
constexpr int HEAD_COMPACT_MAX_SLOTS = 1024;
void launch_head_compact(const int32_t* d_valid, const int32_t* d_count, int frames, int slots_per_frame, int max_heads, int32_t* d_row,
                         int32_t* d_slot_of_row, int32_t* d_rows_used, int32_t* d_overflow, hipStream_t stream);

// ---- letterbox.hip ----------------------------------------------------------------------
// The detector's pre-processing (yolo_v3/utils.py:23-34, yolo_postprocess.py:186-196): Pillow-exact BICUBIC resize at
// unchanged aspect ratio, pasted centred on a grey canvas; uint8 and float32 (/255) outputs.
constexpr int LETTERBOX_MAX_FRAME_SIDE = 8192;  // a frame row (3 bytes per pixel) is staged in LDS
constexpr int LETTERBOX_MAX_BOX_SIDE = 4096;
struct LetterboxPlan {                          // geometry + where each table lies in the int32 table block
    int ih, iw, oh, ow;                         // frame and canvas
    int nw, nh, x0, y0;                         // resized image and its paste offset
    int ksx, ksy;                               // coefficient row stride per axis (Pillow's ksize)
    int off_bx, off_cx, off_by, off_cy;         // bounds (xmin, n) x nw | coeffs [nw][ksx] | bounds x nh | coeffs [nh][ksy]
    int table_ints;
};
int letterbox_axis_ksize(int in_size, int out_size);
void build_letterbox_axis(int in_size, int out_size, int32_t* bounds, int32_t* coeffs);
LetterboxPlan letterbox_plan_layout(int ih, int iw, int out_h, int out_w);      // throws WHENET_EINVAL (limits, nw / nh of zero)
LetterboxPlan build_letterbox_plan(int ih, int iw, int out_h, int out_w, std::vector<int32_t>* tables);
void letterbox_float_table(float lut[256]);
// device pointers only: d_mid holds ih * nw * 3 bytes; either output may be nullptr
void launch_letterbox(const uint8_t* d_frame, const LetterboxPlan& p, int swap_rb, const int32_t* d_tables,
                      const float* d_lut, uint8_t* d_mid, uint8_t* d_canvas_u8, float* d_image_f32, int num_cus,
                      hipStream_t stream);
// the frames of a clip [F][ih][iw][3] (p: ONE frame's plan) -> canvases [F][oh][ow][3]; d_mid holds F * ih * nw * 3 bytes
void launch_letterbox_batch(const uint8_t* d_frames, int frames, const LetterboxPlan& p, int swap_rb, const int32_t* d_tables,
                            const float* d_lut, uint8_t* d_mid, uint8_t* d_canvas_u8, float* d_image_f32, int num_cus,
                            hipStream_t stream);
// A MIXED clip: F <= 16 frames of different sizes, back to back in d_frames (frame f starts frame_off bytes in; neither that
// byte nor a row pitch is 16-byte aligned in general) -> canvases [F][oh][ow][3].  Every frame has its own plan, table block
// and place in d_mid (mid_off, sum of ih * nw * 3 bytes in all); the horizontal pass walks the global rows 0 .. sum ih, frame f's
// first being row0.  total_bytes: the extent of d_frames that may be read (the 16-byte chunks around a row stay inside it).
struct LetterboxMixedFrame {
    unsigned long long frame_off, mid_off;
    const int32_t* tab;
    LetterboxPlan p;
    int row0;
};
struct LetterboxMixed {
    int frames, total_rows;
    unsigned long long total_bytes;
    LetterboxMixedFrame f[MIXED_MAX_FRAMES];
};
void launch_letterbox_mixed(const uint8_t* d_frames, const LetterboxMixed& clip, int swap_rb, const float* d_lut, uint8_t* d_mid,
                            uint8_t* d_canvas_u8, float* d_image_f32, int num_cus, hipStream_t stream);

// ---- yuv.hip ----------------------------------------------------------------------------
// 4:2:0 YUV planes (NV12 / I420) and packed 4:2:2 frames (YUYV / UYVY) -> the packed BGR frame [h][w][3]: the integer conversion of
// include/whenet_hip.h.  The planes of a frame lie TIGHT (pitch removed) in one device buffer: h rows of w luma bytes, then
// ch = (h + 1) >> 1 rows of 2 cw interleaved bytes (NV12) or ch rows of cw U bytes and ch rows of cw V bytes (I420),
// cw = (w + 1) >> 1; a packed frame is its one plane, h rows of 4 cw bytes: yuv_plane_bytes() in all.
constexpr int YUV_MAX_FRAME_SIDE = 8192;
struct YuvCoeffs {
    int yoff, cy, cvr, cug, cvg, cub;
};
const YuvCoeffs& yuv_coeffs(int matrix);        // throws WHENET_EINVAL
inline bool yuv_is_packed(int format) { return format == WHENET_YUV_YUYV || format == WHENET_YUV_UYVY; }
inline size_t yuv_plane_bytes(int h, int w, int format) {
    if (yuv_is_packed(format)) return size_t(h) * 4 * size_t((w + 1) >> 1);
    return size_t(h) * w + 2 * size_t((h + 1) >> 1) * ((w + 1) >> 1);
}
// the planes a format has (1..3), and plane p's rows and row bytes in a frame of h x w
inline int yuv_plane_count(int format) { return yuv_is_packed(format) ? 1 : (format == WHENET_YUV_NV12 ? 2 : 3); }
inline int yuv_plane_rows(int format, int p, int h) { return p == 0 ? h : (h + 1) >> 1; }
inline int yuv_plane_row_bytes(int format, int p, int w) {
    const int cw = (w + 1) >> 1;
    if (yuv_is_packed(format)) return 4 * cw;
    return p == 0 ? w : (format == WHENET_YUV_NV12 ? 2 * cw : cw);
}
// argument checks of a frame list (what: the caller's name; the failing frame's index goes into the text), and the host forms:
// the conversion itself, and the tight copy of a frame's planes that the device reads
void check_yuv_frames(const char* what, const whenet_yuv_frame_t* frames, int nframes);
void yuv_to_bgr_host(const whenet_yuv_frame_t& f, uint8_t* bgr);
void yuv_stage_planes(const whenet_yuv_frame_t& f, uint8_t* dst);
struct YuvGeom {                                // one frame of a launch
    unsigned long long src_off, dst_off;        // its planes in d_planes, its first output byte in d_bgr (any alignment)
    int h, w, format;
    YuvCoeffs k;
    int block0;                                 // (mixed) the first workgroup of the frame
};
struct YuvMixed {
    int frames, total_blocks;
    YuvGeom f[MIXED_MAX_FRAMES];
};
// one frame; `frames` frames of g's size, format and matrix, src_stride / dst_stride bytes apart (the frame is grid dimension y);
// frames of their own sizes, formats and matrices, the records by value in the argument block
void launch_yuv_to_bgr(const uint8_t* d_planes, uint8_t* d_bgr, const YuvGeom& g, hipStream_t stream);
void launch_yuv_to_bgr_batch(const uint8_t* d_planes, uint8_t* d_bgr, const YuvGeom& g, int frames, size_t src_stride, size_t dst_stride,
                             hipStream_t stream);
void launch_yuv_to_bgr_mixed(const uint8_t* d_planes, uint8_t* d_bgr, YuvMixed clip, hipStream_t stream);
// The same conversion of planes that are ALREADY in device memory, where a decoder or a tensor left them: every plane has its own
// address (any alignment) and byte pitch.  At most 16 records by value in the argument block; frame f's output starts dst_off
// bytes into d_bgr.  plane[2] / pitch[2] are unused for NV12, plane[1..2] / pitch[1..2] for YUYV / UYVY.
struct YuvPlanesFrame {
    const uint8_t* plane[3];
    int pitch[3];
    int h, w, format;
    YuvCoeffs k;
    unsigned long long dst_off;
    int block0;                                 // the first workgroup of the frame
};
struct YuvPlanes {
    int frames, total_blocks;
    YuvPlanesFrame f[MIXED_MAX_FRAMES];
};
void launch_yuv_planes_to_bgr(uint8_t* d_bgr, YuvPlanes clip, hipStream_t stream);

// ---- yuvx.hip ---------------------------------------------------------------------------
// The extended ingest of include/whenet_hip_yuv_ext.h: every layout (NV12-like, I420-like, packed 4:2:2, planar 4:4:4) with 8-bit
// or 16-bit samples -> the same packed BGR frame.  The geometry, the checks, the per-pixel function, the host statement and the
// staging are yuvx_host.h (plain C++); these wrap its checks into WHENET_EINVAL.
const YuvxCoeffs& yuvx_coeffs(int matrix);      // throws WHENET_EINVAL
void check_yuvx_frames(const char* what, const whenet_yuvx_frame_t* frames, int nframes);
// One frame of a launch, for both forms.  Upload form: the frame's planes lie TIGHT behind one another src_off bytes into
// d_planes (YuvxLayout; plane[] / pitch[] unused).  Plane form: plane[] / pitch[] are the frame's own, in device memory (src_off
// unused).  The output starts dst_off bytes into d_bgr (any alignment).
struct YuvxFrame {
    const uint8_t* plane[3];
    int pitch[3];
    int h, w, layout, container, shift;
    YuvxCoeffs k;
    unsigned long long src_off, dst_off;
    int block0;                                 // the first workgroup of the frame
};
struct YuvxClip {
    int frames, total_blocks;
    YuvxFrame f[MIXED_MAX_FRAMES];
};
YuvxFrame yuvx_frame(const whenet_yuvx_frame_t& f, size_t src_off, size_t dst_off);
// block0 / total_blocks are set by the launchers; the records travel by value in the argument block
void launch_yuvx_to_bgr(const uint8_t* d_planes, uint8_t* d_bgr, YuvxClip clip, hipStream_t stream);
void launch_yuvx_planes_to_bgr(uint8_t* d_bgr, YuvxClip clip, hipStream_t stream);

// ---- ingest.hip -------------------------------------------------------------------------
// Packed 3-byte pixels that are already in device memory -> the tight frame [h][w][3] the frame path reads: h rows of row_bytes =
// 3 w bytes, `pitch` bytes apart at src (any alignment), to d_out + dst_off (any alignment).  A byte copy: the channel order is
// the slot's business.  At most 16 records by value in the argument block.
struct PackFrame {
    const uint8_t* src;
    unsigned long long dst_off;
    int pitch, h, row_bytes;
    int block0;                                 // the first workgroup of the frame
};
struct PackFrames {
    int frames, total_blocks;
    PackFrame f[MIXED_MAX_FRAMES];
};
void launch_frame_pack(uint8_t* d_out, PackFrames clip, hipStream_t stream);

// ---- overlay.hip ------------------------------------------------------------------------
// The pose overlay (include/whenet_hip.h, POSE OVERLAY; the arithmetic is overlay_host.h's).  Plan: head i of k (<= 1024: the slots
// of a clip) takes its window from rects + i * rect_stride -- (y0, x0, y1, x1), or a crop plan's {y0, x0, h, w} with rect_is_size --
// its valid flag (nullptr: 1) and the angles of forward row row[i] (nullptr: row i; a negative row paints nothing), and writes
// segs [k][16] and flags [k]; with `labels` (nullptr: WHENET_DISPLAY_SIMPLE) also the head's label record, labels [k][3][4] words
// (overlay_host.h, OverlayLine), and OVERLAY_LABELS in its flags.  Draw: reads the tight frame [fh][fw][3] and the table of k <= 256
// heads, writes the surface's planes (device memory, any alignment, their own pitches); display WHENET_DISPLAY_FULL reads `labels`.
struct OverlayPlanArgs {
    const int32_t* rects;
    const int32_t* valid;
    const int32_t* row;
    const float* ypr;
    int k, rect_stride, rect_is_size;
    int32_t* segs;
    int32_t* flags;
    uint32_t* labels;
};
struct OverlayDrawArgs {
    const uint8_t* frame;
    int fh, fw, channel_order;
    const int32_t* segs;
    const int32_t* flags;
    int k;
    uint8_t* plane[3];
    int pitch[3];
    int format;
    Bgr2YuvCoeffs kc;
    const uint32_t* labels;
    int display;
};
void launch_overlay_plan(const OverlayPlanArgs& a, hipStream_t stream);
void launch_overlay_draw(const OverlayDrawArgs& a, hipStream_t stream);

// ---- jpeg.hip ---------------------------------------------------------------------------
// The baseline JPEG encoder (include/whenet_hip.h, JPEG ENCODER; the arithmetic is jpeg_host.h's) of ONE frame whose planes are in
// device memory (any alignment, their own pitches).  Five launches behind one memset of `bits`:
//   dct     8 lanes per 8 x 8 block, 32 blocks per workgroup: samples -> both DCT passes -> quantiser -> coef [R * B][64] (zigzag)
//   pack    one workgroup per restart interval (MCU row): the blocks' bit lengths, their exclusive scan in steps of 256 blocks with
//           a carry (an interval has up to 3,072 blocks), then every block's code words OR-ed into the interval's zeroed bit buffer
//           (atomicOr on dwords: the bytes do not depend on the order); the last byte padded with 1-bits; ulen [R]
//   count   the 0xFF bytes of every interval -> slen [R] = the interval's stuffed length
//   write   the header, every interval's stuffed bytes at 629 + sum of (slen + 2) before it, RSTm / EOI, and the total length
//           into *size -- every byte store checked against `cap`, so a stream that does not fit leaves dst's tail untouched.
// R = ceil(h / 16) intervals of B = 6 ceil(w / 16) blocks at 4:2:0; 4:2:2 and 4:4:4 have R = ceil(h / 8) intervals of 4 ceil(w / 16)
// and 3 ceil(w / 8) blocks (JpegGeom; dct, hist and pack are instantiated per sampling, so 4:2:0 keeps its code).  An optimised
// encode runs two more kernels between dct and pack, behind a memset of its four histograms:
//   hist    one workgroup per interval, a lane per block: the blocks' symbols into 4 x 256 LDS counters, those into the global ones
//   table   one workgroup: T.81 K.2 on the four histograms -> this encode's codes, header (occurring symbols only) and header length
// pack then reads the codes, write the header and its length, from the encode's own JpegOptTables in the work buffers.
// JpegScratch lays the work buffers out in one allocation.
struct JpegScratch {
    int R, B, interval_dwords;
    JpegGeom geom;
    size_t coef, bits, bits_bytes, ulen, slen, opt, bytes;      // byte offsets, the memset's extent, the allocation's size
    JpegScratch(int h, int w, int sampling = WHENET_JPEG_420);
};
struct JpegArgs {
    JpegSource src;
    const JpegTables* tables;      // device memory
    int16_t* coef;
    uint32_t* bits;
    int32_t* ulen;
    int32_t* slen;
    uint8_t* dst;                  // cap bytes
    long long cap;
    long long* size;               // one int64: the full length
    int R, B, interval_dwords;
    JpegGeom geom;
    const uint16_t (*code)[256];   // what pack reads: the tables' or the encode's own
    const uint8_t (*len)[256];
    const uint8_t* header;         // what write copies: the tables' (629 bytes) or the encode's own (*header_bytes)
    const int32_t* header_bytes;   // nullptr: JPEG_HEADER_BYTES
    JpegOptTables* opt;            // nullptr: the standard tables
};
JpegArgs jpeg_args(const JpegSource& src, const JpegTables* d_tables, void* d_scratch, const JpegScratch& lay, void* d_dst, long long cap,
                   void* d_size, bool optimize = false);
void launch_jpeg_encode(const JpegArgs& a, const JpegScratch& lay, hipStream_t stream);
// min(*d_size, cap) bytes of a stream, rounded up to whole 16-byte vectors, from d_stream to `to` (both 16-byte aligned and
// ceil(cap / 16) vectors long), and *d_size to *to_size: `to` may be pinned host memory as the device addresses it
void launch_jpeg_flush(const void* d_stream, void* to, const long long* d_size, long long cap, long long* to_size, hipStream_t stream);

// ---- jpeg_dec.hip -----------------------------------------------------------------------
// The baseline JPEG decoder (include/whenet_hip.h, JPEG DECODER; the arithmetic is jpeg_dec_host.h's) of ONE stream whose entropy
// data is in device memory (any alignment).  Four launches behind two memsets (interval starts + meta, coefficient records):
//   scan     one workgroup: the RSTm pairs of the data -> start [intervals], meta[0] = meta[1] = the first interval the markers make
//            bad (JPEG_DEC_NO_BAD: none)
//   entropy  one interval per lane, 16 per workgroup, tables in LDS: Huffman decode, dequantise, clamp -> coef [blocks][64] (natural
//            order, block = MCU * bpm + its index in the MCU); a damaged interval lowers meta[1]
//   idct     8 lanes per block: both passes -> the component planes (padded to whole MCUs, pitches multiples of 8); status[0..1]
//   frame    planes -> the destination: packed pixels in either channel order at any pitch (a tight BGR frame of a 4:2:0 stream:
//            launch_yuv_planes_to_bgr), or an I420 / NV12 surface for a 4:2:0 stream.  No thread stores outside the rows' bytes.
//            JpegDecArgs::orient = 2..8: the oriented frame kernel in its place (one launch all the same, no upright intermediate):
//            the same pixel values at the destination addresses of the EXIF orientation, 5..8 through a 32 x 32 LDS tile.
// JpegDecArgs::rule = 1 (libjpeg's bytes, packed destinations only) runs the rule-1 forms of idct and frame in their places.
// JpegDecScratch lays the work buffers out in one allocation; tables | data at its front are what a caller uploads in one copy
// (data_bytes = 0: the data lies elsewhere).
// The entropy stage has a second form (jpeg_dec_seg.hip; the arithmetic is jpeg_dec_seg_host.h's): form = 1 decodes every interval
// with many lanes, a lane per segment of seg_bytes of the data.  Behind the scan, six launches stand for `entropy`:
//   segtab   one workgroup: the segments of every decoded interval -> first_seg [intervals + 1] (an exclusive scan), the totals
//   sync     one workgroup per window of WHENET_JPEG_SEG_WINDOW segments, states in LDS: the exit state of every segment
//   stitch   one lane per interval: the true state over each window boundary inside the interval
//   count    one lane per segment: its blocks and their DC differences as saturating maps
//   segscan  one workgroup per interval: every segment's first block and entry predictors
//   write    one lane per segment: its blocks -> coef, through an LDS stage; damage lowers meta[1]
// Every grid is sized from seg_cap = ceil(nbytes / seg_bytes) + intervals, the host's bound; surplus lanes exit.
struct JpegDecScratch {
    size_t tables, data, upload_bytes, start, meta, zero_bytes, coef, coef_bytes, plane[3], bytes;      // byte offsets and extents
    size_t seg_stats, first_seg, seg_exit, seg_count, seg_blk;      // seg_stats: 8 int64 inside the zeroed bytes; the others: form 1 only
    int form, seg_bytes;
    int seg_lanes = 0;      // decoding lanes per wave of the segmented form's kernels: 16, 32 or 64 (0: the default)
    long long seg_cap;
    // nbytes: the length of the entropy data (< 0: data_bytes)
    JpegDecScratch(const JpegDecGeom& g, size_t data_bytes, long long nbytes = -1, int form = 0, int seg_bytes = 0);
    // the offsets as the region table jpeg_dec_args reads (lengths are not filled in)
    JpegClipFrame regions() const {
        JpegClipFrame q{};
        q.form = form, q.seg_bytes = seg_bytes, q.seg_cap = seg_cap;
        q.tables.off = tables, q.data.off = data, q.start.off = start, q.meta.off = meta, q.seg_stats.off = seg_stats, q.coef.off = coef;
        for (int c = 0; c < 3; ++c) q.plane[c].off = plane[c];
        q.first_seg.off = first_seg, q.seg_exit.off = seg_exit, q.seg_count.off = seg_count, q.seg_blk.off = seg_blk;
        return q;
    }
};
struct JpegDecArgs {
    JpegDecGeom g;
    const JpegDecTables* tables;   // device memory
    const uint8_t* data;           // the entropy data: nbytes bytes from the stream's data_offset on
    int nbytes;
    int32_t* start;
    int32_t* meta;
    int16_t* coef;
    uint8_t* plane[3];
    uint8_t* dst[3];
    int dst_pitch[3];
    int format, channel_order;
    int rule;                      // 0: the project's own inverse DCT and pixel rule, 1: libjpeg's (packed destinations only)
    int orient;                    // the EXIF orientation the frame kernel applies: 0 or 1 upright; 2..8 (packed destinations only): dst is
                                   // the oriented frame, jpeg_orient_h x jpeg_orient_w pixels (jpeg_dec_host.h)
    int32_t* status;               // two int32
    // the segmented form (form = 1)
    int form, seg_bytes, seg_cap;
    int seg_lanes;                 // decoding lanes per wave of the sync and write kernels: 16, 32 or 64 (0: the default)
    long long* seg_stats;          // 8, zeroed with start | meta
    int32_t* first_seg;            // [intervals + 1]
    uint64_t* seg_exit;            // [seg_cap] exit states
    JpegSegCount* seg_count;       // [seg_cap]
    int32_t* seg_blk;              // [seg_cap][4]: the first block's index in the interval, the three predictors there
};
// the segmented form's launches (jpeg_dec_seg.hip), behind the scan kernel and in front of the inverse DCT
void launch_jpeg_decode_segmented(const JpegDecArgs& a, hipStream_t stream);
// The record of one stream from a table of regions, offsets into d_base (a clip's JpegClipFrame; JpegDecScratch::regions(),
// JpegProgLayout::regions()).  Form 2, a progressive stream: a baseline record over the progressive layout -- what
// launch_jpeg_decode_tail reads of it (coef, meta, planes, destination, rule; form 0) --, the fields of the segmented form empty.
inline JpegDecArgs jpeg_dec_args(const JpegDecGeom& g, void* d_base, const JpegClipFrame& q, long long nbytes, const whenet_surface_t& dst,
                                 int channel_order, int32_t* d_status, int rule, int seg_lanes, int orient = 1) {
    JpegDecArgs a{};
    char* const s = static_cast<char*>(d_base);
    a.g = g;
    a.tables = reinterpret_cast<const JpegDecTables*>(s + q.tables.off);
    a.data = reinterpret_cast<const uint8_t*>(s + q.data.off), a.nbytes = int(nbytes);
    a.start = reinterpret_cast<int32_t*>(s + q.start.off), a.meta = reinterpret_cast<int32_t*>(s + q.meta.off);
    a.coef = reinterpret_cast<int16_t*>(s + q.coef.off);
    for (int c = 0; c < 3; ++c) {
        a.plane[c] = reinterpret_cast<uint8_t*>(s + q.plane[c].off);
        a.dst[c] = static_cast<uint8_t*>(dst.plane[c]), a.dst_pitch[c] = dst.pitch[c];
    }
    a.format = dst.format, a.channel_order = channel_order, a.rule = rule, a.orient = orient;
    a.status = d_status;
    if (q.form == JPEG_CLIP_FORM_PROGRESSIVE) return a;
    a.form = q.form, a.seg_bytes = q.seg_bytes, a.seg_cap = int(q.seg_cap), a.seg_lanes = seg_lanes;
    a.seg_stats = reinterpret_cast<long long*>(s + q.seg_stats.off);
    a.first_seg = reinterpret_cast<int32_t*>(s + q.first_seg.off), a.seg_exit = reinterpret_cast<uint64_t*>(s + q.seg_exit.off);
    a.seg_count = reinterpret_cast<JpegSegCount*>(s + q.seg_count.off), a.seg_blk = reinterpret_cast<int32_t*>(s + q.seg_blk.off);
    return a;
}
void launch_jpeg_decode(const JpegDecArgs& a, const JpegDecScratch& lay, hipStream_t stream);
// the stages behind the entropy decode on their own: the inverse DCT of a.coef (which writes the status words from a.meta[1]) and
// the colour stage of the record's rule and destination
void launch_jpeg_decode_tail(const JpegDecArgs& a, hipStream_t stream);

// ---- jpeg_prog.hip ----------------------------------------------------------------------
// The progressive decoder's entropy stage (include/whenet_hip.h, JPEG DECODER, PROGRESSIVE; the arithmetic is jpeg_prog_host.h's)
// in front of launch_jpeg_decode_tail.  JpegProgLayout lays one allocation out: scans | huff | qz | items | data are the plan's one
// upload; meta | raw (one memset); coef; the padded planes.
//   whenet_jpeg_prog_scan_kernel    one (scan, interval) item per decoding lane, 16 per 64-lane workgroup, all of ONE scan (the
//            lists are padded): the scan's record and its <= 3 JpegDecHuff lie in LDS, the scan kind is uniform.  A lane stores
//            int16s inside its scan's band only; a damaged item raises meta[0] = JPEG_DEC_NO_BAD - item (atomicMax).
//   whenet_jpeg_prog_finish_kernel  8 lanes per block: raw (zigzag) x Q, clamp -> coef (natural order), 16-byte loads and stores
//            through LDS; folds meta[1] = the first bad item (the decode's, or what the host knew: first_bad).
// levels = 1: a launch per level; 0: a launch per scan in stream order.  scan_launches (may be nullptr): += the launches.
struct JpegProgLayout {
    size_t scans, huff, qz, items, data, upload_bytes, meta, raw, zero_bytes, coef, coef_bytes, plane[3], bytes;
    JpegProgLayout(const JpegDecGeom& g, const JpegProgPlan& plan);
    // the offsets as the region table jpeg_dec_args reads: form 2, the Huffman tables for `tables` and the item list for `start`
    // (neither is read behind the entropy stage)
    JpegClipFrame regions() const {
        JpegClipFrame q{};
        q.form = JPEG_CLIP_FORM_PROGRESSIVE;
        q.tables.off = huff, q.data.off = data, q.start.off = items, q.meta.off = meta, q.coef.off = coef;
        for (int c = 0; c < 3; ++c) q.plane[c].off = plane[c];
        return q;
    }
};
struct JpegProgArgs {
    JpegDecGeom g;
    const JpegProgScan* scans;
    const JpegDecHuff* huff;       // 3 per scan
    const int16_t* qz;             // [3][64]
    const JpegProgItem* items;
    const uint8_t* data;
    int nbytes;
    int16_t* raw;
    int16_t* coef;
    int32_t* meta;
    int first_bad;
};
// the plan's upload, laid out at `stage` (host memory of lay.upload_bytes; data: the stream's bytes from plan.data_base on)
void jpeg_prog_stage(const JpegProgPlan& plan, const JpegProgLayout& lay, const uint8_t* data, uint8_t* stage);
// memset + scan launches + finish + tail.  a: a baseline record over the same scratch (coef, meta, planes, destination, rule)
void launch_jpeg_decode_progressive(const JpegDecArgs& a, const JpegProgPlan& plan, const JpegProgLayout& lay, void* d_scratch, int levels,
                                    hipStream_t stream, int64_t* scan_launches);

// A CLIP of 1..16 streams, every stage in ONE launch for all of them: the same bodies, a workgroup first finds its frame in the
// prefix sums of the per-frame workgroup counts (JpegClipGrid, by value) and reads that frame's record from d_recs -- device
// memory, records JPEG_CLIP_RECORD_BYTES apart (jpeg_dec_clip_host.h), part of the clip's one upload.  h_recs: the same records on
// the host, the launch sizes come from them.  d_zero / zero_bytes: every frame's start | meta | seg_stats and coefficient records
// (one memset).  Frames of form 0 and of form 1, and of any colour path, may stand in one clip: a stage's kernel is launched once
// if any frame needs it, so the number of enqueues depends on the forms and paths that occur, never on the frame count.
// enqueues (may be nullptr): += the launches and memsets enqueued.
struct JpegClipGrid {
    int frames, total;
    int first[MIXED_MAX_FRAMES + 1];      // frame f owns workgroups first[f] .. first[f + 1] - 1 (none: the two are equal)
};
// the grid of a stage: count(record) workgroups for every frame (0: the frame does not take part); false where no frame does
template <class Count>
inline bool jpeg_clip_grid(const JpegDecArgs* recs, int frames, Count count, JpegClipGrid& grid) {
    grid = JpegClipGrid{};
    grid.frames = frames;
    long long at = 0;
    for (int f = 0; f < frames; ++f) {
        grid.first[f] = int(at);
        at += count(recs[f]);
        WHENET_REQUIRE(at < 0x7FFFFFFF, WHENET_EINVAL, "jpeg_decode_clip: more workgroups than an int32 counts");
    }
    for (int f = frames; f <= MIXED_MAX_FRAMES; ++f) grid.first[f] = int(at);
    grid.total = int(at);
    return at > 0;
}

#if defined(__HIPCC__)
// the frame of workgroup b: the last one whose first workgroup is not behind b (a scan of at most 16 prefix sums, the same for
// every lane: b is a workgroup index), and that frame's record
__device__ __forceinline__ int jpeg_clip_frame_of(const JpegClipGrid& grid, int b) {
    int f = 0;
#pragma unroll
    for (int i = 1; i < MIXED_MAX_FRAMES; ++i) f = (i < grid.frames && b >= grid.first[i]) ? i : f;
    return f;
}
__device__ __forceinline__ const JpegDecArgs& jpeg_clip_record(const void* recs, int f) {
    return *reinterpret_cast<const JpegDecArgs*>(static_cast<const char*>(recs) + size_t(f) * JPEG_CLIP_RECORD_BYTES);
}
#endif
void launch_jpeg_decode_clip(const JpegDecArgs* h_recs, const void* d_recs, int frames, void* d_zero, size_t zero_bytes, hipStream_t stream,
                             int64_t* enqueues);
void launch_jpeg_decode_segmented_clip(const JpegDecArgs* h_recs, const void* d_recs, int frames, hipStream_t stream, int64_t* enqueues);
// launch_jpeg_decode_clip in its two halves.  entropy: the checks, the one memset, then marker scan | entropy | segmented stages for
// the frames whose `progressive` byte is 0 (nullptr: all) -- a stage no frame needs is not launched.  tail: inverse DCT and colour
// for all frames (a progressive frame's record presents coef and meta[1] as a baseline one's).
void launch_jpeg_decode_clip_entropy(const JpegDecArgs* h_recs, const void* d_recs, int frames, void* d_zero, size_t zero_bytes, hipStream_t stream,
                                     int64_t* enqueues, const uint8_t* progressive);
void launch_jpeg_decode_clip_tail(const JpegDecArgs* h_recs, const void* d_recs, int frames, hipStream_t stream, int64_t* enqueues);

// A clip that may hold PROGRESSIVE frames (jpeg_prog.hip): plans[f] is the scan plan of frame f (nullptr, or a baseline one: the frame
// runs as in launch_jpeg_decode_clip), h_prog[f] its progressive record, which also lies in the frame's uploaded record at
// JPEG_CLIP_PROG_RECORD_OFFSET (jpeg_dec_clip_host.h); h_recs[f] is then what jpeg_dec_args makes of a form-2 region table (form 0, coef, meta).
//   whenet_jpeg_prog_clip_scan_kernel    launch L covers level L of every frame that has one: a frame's share of the grid is
//            level_cnt[L] / 16 workgroups (0 for a frame with fewer levels and for a baseline frame), its first workgroup reads the
//            frame's item list from level_off[L] / 16 on (JpegProgClipLevel).  The launches: the largest level count, <= 14.
//   whenet_jpeg_prog_clip_finish_kernel  one launch for all progressive frames.
// The bodies are the single-stream kernels'.  Always by level: the per-scan launches of option "jpeg_prog_levels" = 0 are a
// measurement knob of the single-stream path.  enqueues / scan_launches (may be nullptr): += launches + memsets / scan-kernel launches.
struct JpegProgClipLevel {
    int first_group[MIXED_MAX_FRAMES];      // per frame: the level's first workgroup in the frame's own item list
};
#if defined(__HIPCC__)
__device__ __forceinline__ const JpegProgArgs& jpeg_clip_prog_record(const void* recs, int f) {
    return *reinterpret_cast<const JpegProgArgs*>(static_cast<const char*>(recs) + size_t(f) * JPEG_CLIP_RECORD_BYTES + JPEG_CLIP_PROG_RECORD_OFFSET);
}
#endif
void launch_jpeg_decode_clip_progressive(const JpegDecArgs* h_recs, const JpegProgArgs* h_prog, const JpegProgPlan* const* plans, const void* d_recs,
                                         int frames, void* d_zero, size_t zero_bytes, hipStream_t stream, int64_t* enqueues, int64_t* scan_launches);

// ---- dconv.hip --------------------------------------------------------------------------
// The detector body's layers (yolo_v3/model.py:20-122) on NHWC activations of `dtype` (WHENET_F16: binary16 storage on the f16
// matrix cores; WHENET_F32: float32 storage on v_mfma_f32_32x32x2_f32, nothing rounded to binary16): implicit-GEMM convolution
// with folded BatchNorm, LeakyReLU, residual add and the upsample + concatenate read; 2x2 max-pools; the image input stage.
// Device pointers only.
struct DconvArgs {
    const void* in0;       // [n,H,W,C0]; with in1: the HALF-resolution tensor [n,H/2,W/2,C0], read at (y >> 1, x >> 1)
    const void* in1;       // [n,H,W,C1] route tensor (channels C0.. of the concatenation) or nullptr
    const void* w;         // pack_dconv() image of the same dtype
    const float* bias;     // [ceil(Cout / 32) * 32]
    const void* skip;      // [n,Ho,Wo,Cout] residual operand or nullptr
    void* out;             // [n,Ho,Wo,Cout] in dtype, or float32 with f32_out (the output convolutions)
    float* partial;        // split-K workspace, dconv_partial_floats() floats (splits > 1)
    int n, H, W, C0, C1;
    int Ho, Wo, Cout, k, stride, leaky, f32_out, splits;
    int dtype;             // WHENET_F16 or WHENET_F32: the element type of in0, in1, w, skip and out
};
int dconv_tile_n(int cout);
int dconv_splits(int k, int cin, int cout, int Ho, int Wo);      // a function of the layer and the image size, never of the batch or the dtype
size_t dconv_partial_floats(const DconvArgs& a);
void launch_dconv(const DconvArgs& a, hipStream_t stream);
void launch_dpool(const void* in, void* out, int dtype, int n, int H, int W, int C, int stride, hipStream_t stream);
// [pixels][3] float32, or uint8 through the /255 table of letterbox.hip -> [pixels][16] binary16 or [pixels][8] float32 (channels 3.. zero)
void launch_dimage(const float* f32, const uint8_t* u8, const float* lut, void* out, int dtype, size_t pixels, hipStream_t stream);

// ---- convert.hip ------------------------------------------------------------------------
void launch_empty(hipStream_t stream);   // boundary calibration for whenet_profile()
void launch_f32_to_act(const float* src, void* dst, size_t count, int dtype, hipStream_t stream);
void launch_act_to_f32(const void* src, float* dst, size_t count, int dtype, hipStream_t stream);

const char* kernel_name_stem(int dtype);
const char* kernel_name_dw(int dtype, int k, int s);
std::string kernel_name_pw(const PwArgs& a, int dtype, int impl, int num_cus);

}  // namespace whenet
