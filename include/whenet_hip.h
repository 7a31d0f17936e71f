/*
 * libwhenet_hip.so -- C ABI of the MI355X-native WHENet inference path.
 *
 * The reference has no FFI / plugin / operator interface for this path: its boundary is
 * the Python class `WHENet` in module `whenet` (/root/reference/whenet.py:6-34), whose
 * arithmetic is delegated to Keras/TensorFlow.  Every entry point below therefore cites
 * the Python statement(s) of the reference it replaces; the ctypes binding a maintainer
 * adds on the reference side is the drop-in `whenet.py` of this repo.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types cross this boundary;
 *   - every function returns 0 (WHENET_OK) or a negative code and never throws;
 *     whenet_last_error() gives the message for the last failure on that handle
 *     (or, with a NULL handle, of the last failed whenet_create* on this thread);
 *   - all outputs are caller-allocated; inputs are never written;
 *   - a handle owns one device and 1..4 ENGINES (option "inflight", default 1), each engine with its own main
 *     stream, lane / copy streams created on demand, activation arena, hipGraphs and a copy of the device weights;
 *     a handle is NOT thread-safe: use one handle per host thread / per GPU;
 *   - crops are uint8 RGB, NHWC, [n,224,224,3] contiguous -- exactly the array the
 *     reference's callers build (demo.py:8-12, demo_video.py:21-24);
 *   - there is no CPU fallback anywhere in this library: without a gfx950 device
 *     whenet_create* fails with WHENET_ENODEV.
 */
#ifndef WHENET_HIP_H
#define WHENET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* (round 4 also: options front7, head_fuse, stem_fuse.)
 * 2 (round 3): whenet_op_trunk / whenet_op_stem_dw removed with their kernels; whenet_create_postproc and
 * whenet_op_block_range added; options front_impl, se_fuse, fold12, poison.
 * 3 (round 4): whenet_launch_stat_t carries the crops and chains of the launch it describes (what whenet_profile
 * actually ran: with option "inflight" > 1 a forward is ONE chain of the whole batch).
 * 4 (round 5): dtype WHENET_F32S; whenet_normalise_table; options pw_staged, split_pw, fanout_min / _chunk / _stage / _depth,
 * host_pinned_max, host_lanes, se_fuse_tiny.  (Additions only: a version-3 caller runs unchanged.)
 * (round 6, still 4 -- options only: mb7, f2s_mask, se_fuse = 3, fanout_engines, fanout_stage = 2 | 3; the fan-out's default form is 2.)
 * (round 7, still 4 -- option act_layout.)
 * 5 (round 8): whenet_letterbox_plan, whenet_op_letterbox and the resident-frame form whenet_frame_begin / whenet_frame_letterbox /
 * whenet_frame_heads.  (Additions only: a version-4 caller runs unchanged.)
 * (still 6 -- clips: whenet_clip_begin / whenet_clip_detect_heads / whenet_collect_clip, whenet_op_letterbox_batch,
 * whenet_yolo_eval_batch, whenet_op_head_compact.  Additions only.)
 * (still 6 -- YUV 4:2:0 ingest: whenet_yuv_frame_t, whenet_yuv_to_bgr_host, whenet_op_yuv_to_bgr, whenet_frame_begin_yuv,
 * whenet_clip_begin_yuv.  Additions only.)
 * (still 6 -- pose overlay: whenet_surface_t, whenet_overlay_segments, whenet_annotate_host, whenet_op_annotate,
 * whenet_frame_annotate.  Additions only.)
 * (still 6 -- the overlay's labels: whenet_overlay_labels, whenet_overlay_glyph, whenet_annotate_host_ex, whenet_op_annotate_ex,
 * whenet_frame_annotate_ex.  Additions only.) */
#define WHENET_ABI_VERSION 6
#define WHENET_API __attribute__((visibility("default")))

/* return codes (negative errno-style) */
#define WHENET_OK        0
#define WHENET_ENOENT   (-2)    /* snapshot file missing/unreadable  (Keras: OSError)        */
#define WHENET_EIO      (-5)
#define WHENET_ENOMEM   (-12)
#define WHENET_ENODEV   (-19)   /* no usable gfx950 device                                  */
#define WHENET_EINVAL   (-22)   /* bad argument / shape            (Keras: ValueError)      */
#define WHENET_EFORMAT  (-74)   /* not a WHNPACK1 snapshot or tensor shapes do not match    */
#define WHENET_EHIP     (-1000) /* HIP runtime call or kernel launch failed                  */

/* arithmetic type of activations and 1x1-conv weights (accumulation is always f32) */
#define WHENET_F32 0            /* parity configuration: <=1e-3 deg vs the float64 oracle   */
#define WHENET_F16 1            /* throughput configuration (north-star fp16)               */
#define WHENET_F32S 2           /* float32 storage and accumulation as WHENET_F32, the 1x1 products as binary16 hi/lo pairs on the
                                 * f16 matrix cores (w = hi + lo, x = hi + lo; lo_w*hi_x + hi_w*lo_x + hi_w*hi_x: ~22 bits per
                                 * product, 3 f16 MFMAs where WHENET_F32 issues 8 f32 MFMAs).  whenet_info_t.dtype reports
                                 * WHENET_F32 (the storage type); option "split_pw" 0 runs the exact-f32 kernels on such a handle.
                                 * Precondition: activations inside the binary16 range (|x| <= 65504; EfficientNet-B0's are O(100)
                                 * behind every BatchNorm) -- beyond it the hi half is inf and the angles come out NaN, never silently
                                 * wrong */

#define WHENET_IMG      224
#define WHENET_NLOGITS  252     /* 120 yaw | 66 pitch | 66 roll  (whenet.py:11-13)          */
#define WHENET_NFEAT    1280

typedef struct whenet_ctx whenet_t;

typedef struct whenet_info {
    int32_t abi_version;
    int32_t dtype;              /* WHENET_F32 / WHENET_F16 */
    int32_t device_id;
    int32_t compute_units;
    int64_t params_backbone;    /* 4,049,564 */
    int64_t params_heads;       /*   322,812 */
    int32_t n_tensors;          /* 315 */
    int32_t n_kernels_per_forward;
    int64_t macs_per_crop;      /* 384,857,312 */
    int64_t arena_bytes;        /* current activation arena */
    int32_t capacity;           /* crops the arena currently holds */
    int32_t graph_enabled;
    char    device_name[64];
    char    arch[32];
} whenet_info_t;

/* One kernel launch of a forward pass, as timed by whenet_profile(). */
typedef struct whenet_launch_stat {
    char    layer[32];          /* e.g. "b3/dw", "b3/project", "stem", "heads"              */
    char    kind[16];           /* stem | pw | dw | se | heads                              */
    char    kernel[64];         /* kernel symbol family, matches rocprofv3's kernel name    */
    double  avg_us;             /* mean duration over chains x iterations (HIP events)        */
    double  alg_bytes;          /* algorithmic bytes of this launch: in + out (+skip) once  */
    double  alg_flops;          /* 2 * MACs of this launch                                   */
    int32_t crops;              /* crops this launch processed (the chain's sub-batch)       */
    int32_t chains;             /* concurrent sub-batch chains the figures are averaged over */
} whenet_launch_stat_t;

/* ---- construction: replaces WHENet.__init__ (whenet.py:7-20): graph build +
 * model.load_weights(snapshot).  `snapshot_path` is a WHNPACK1 file (the 315 Keras arrays;
 * tools/convert_h5.py turns a Keras HDF5 snapshot into one). */
WHENET_API int whenet_create(const char* snapshot_path, int device_id, int dtype, whenet_t** out);
WHENET_API int whenet_create_from_memory(const void* snapshot, size_t nbytes, int device_id, int dtype,
                              whenet_t** out);
/* A handle WITHOUT a network: device, stream and scratch for the frame / detector stages only
 * (whenet_yolo_eval, whenet_op_crop_resize, whenet_frame_rects); every forward entry point returns WHENET_EINVAL. */
WHENET_API int whenet_create_postproc(int device_id, whenet_t** out);
WHENET_API void whenet_destroy(whenet_t* h);
WHENET_API const char* whenet_last_error(const whenet_t* h);
WHENET_API int whenet_get_info(const whenet_t* h, whenet_info_t* out);

/* options: "graph" (0/1, default 1: replay the forward as a hipGraph),
 *          "fuse_front" (0/1, default 1: expand 1x1 + depthwise as ONE kernel per block, the
 *                  expanded tensor stays in LDS; 0 = two launches through HBM),
 *          "se_fuse" (0..3, default 1: second half of the squeeze-excite block inside the project conv's launch -- its
 *                  workgroups compute the gate of their own rows' crops -- 0 = never (a squeeze-excite launch per block,
 *                  51 launches per forward, 50 with fold12), 2 = on every block with a fused front kernel (36 / 35 launches), 1 = on the
 *                  blocks where that is the faster schedule; the results are bitwise the same;
 *                  3 (round 6, f16 / f32s handles) = 1 plus blocks 7-16, whose project conv then computes the gate of each wave's own
 *                  channel groups on the matrix cores: ten launches fewer, another rounding path, measured slower),
 *          "front_impl" (0..2, default 1: which fused kernel a handle uses -- 0 = front.hip (depthwise taps
 *                  as f32 VALU FMAs) on every block, 2 = the kernel with the taps as Toeplitz products on the matrix
 *                  cores wherever it exists (f16: front2.hip, f16 tap weights; f32s: front2s.hip, exact-f32 or hi/lo taps;
 *                  blocks 2-12), 1 = per layer, whichever was measured faster; exact-f32 handles always run front.hip),
 *          "front7" (0/1, default 1: with front_impl = 1, blocks 13-16 (7 x 7 maps) of an f16 handle run front7.hip -- a GROUP of
 *                  2 or 4 crops per workgroup, the image-only LDS tile, the chunk's expand weights staged once in LDS; the group
 *                  size follows the launch size and changes no bit of a crop's result; 0 = round 3's per-layer choice),
 *          "head_fuse" (0/1, default 1: the head conv (whenet.py:8, last layer) pools its own output, the
 *                  GlobalAveragePooling2D of whenet.py:10, in one kernel (head7.hip; f16, and f32 since round 4b); 0 = conv, then pooling
 *                  inside the heads kernel),
 *          "stem_fuse" (0/1, default 1: handles of EITHER dtype fed uint8 crops compute the stem conv (whenet.py:8, first layer) inside block 1's
 *                  depthwise kernel (stemdw.hip): the 112 x 112 x 32 stem output never reaches HBM, one launch less; results are
 *                  BITWISE those of the two kernels (f16 and f32); 0 = stem.hip, then dw.hip.  The float32-input entry points keep the two.
 *                  f32 precision note: conv-epilogue Swish uses v_exp_f32 / v_rcp_f32 (1-ulp hardware forms, device_math.h) in both
 *                  dtypes since round 4; build with -DWHENET_PRECISE_CONV_SWISH=1 for expf + IEEE division),
 *          "fold12" (0/1, default 1: f16 handles whose block 2 runs front2.hip feed that kernel from block 1's depthwise
 *                  output, with block 1's project conv (linear) composed into block 2's expand weights when the
 *                  snapshot is loaded -- one launch and a 112x112x16 round trip through HBM less; 0 = the two convs
 *                  as two steps.  Same function, different rounding points: results agree to f16 rounding),
 *          "front2_static" (0/1, default 1: the layers of an f16 handle that run front2.hip use, where the per-layer table says so,
 *                  the form of that kernel whose tile geometry is compile-time constants (the plan of front2_tuned.inc's row; no
 *                  index divisions or LDS offsets computed in front of the workgroup's first load); 0 = the runtime-geometry
 *                  form everywhere.  Shapes and plans outside the table always run the runtime form.  Same bits either way),
 *          "front_static" (0/1, default 1: block 6 of an f16 handle -- the one block of the default forward that runs front.hip -- uses
 *                  the form of that kernel whose tile geometry is compile-time constants (the layer's plan of front_tuned_f16.inc);
 *                  0 = the runtime-geometry form.  Launches of at most 32 crops (512-lane workgroups) and plans outside the table
 *                  always run the runtime form.  Same bits either way),
 *          "pw_static" (0/1, default 1: the project 1x1 GEMMs of an f16 handle use, where the per-layer table says so, the form of
 *                  their kernel whose layer shape -- K, N, the pixels per crop, the tile and chunk counts, the squeeze-excite sizes --
 *                  is compile-time constants (a row of pw.hip's shape table: no divisions by run-time sizes and no clamps against
 *                  them in front of a workgroup's first load); 0 = the runtime-shape form everywhere.  Launches outside the table
 *                  (another blocking at small batches, se_fuse / act_layout / pw_staged other than the defaults) always run the
 *                  runtime form.  Same bits either way),
 *          "poison" (0/1, default 0, debug: the activation arena is filled with NaN bit patterns before every forward --
 *                  a kernel that reads what the forward did not write shows up in the results),
 *          "lanes" (1..8, default 2: concurrent sub-batch chains per forward, never fewer than 16 crops each),
 *          "lane_graphs" (0/1, default 0: 1 = one graph per lane launched on its own stream instead of
 *                  one forked graph; measured equal),
 *          "inflight" (1..4, default 1: n > 1 gives the handle n engines -- own streams, activation
 *                  arena, graphs, replicated weights -- and spreads whenet_forward_u8_device calls with
 *                  stream == NULL and whenet_submit_* calls over them round-robin, each forward as
 *                  one chain; independent forwards then overlap on the GPU (a forward is a chain of 46
 *                  (f16) / 49 (f32) dependent launches: whenet_info_t.n_kernels_per_forward).  The caller gives every forward in flight its own output
 *                  buffers; whenet_sync waits for all of them.  Results are bitwise those of n = 1),
 *          "fanout_min" (>= 0, default 256: a blocking whenet_forward_u8 of at least this many crops is cut into
 *                  "fanout_chunk"-crop forwards (default 128; the first two are half-size so that the GPU starts early); chunk c goes
 *                  to engine c % E through that engine's pinned submission slots, at most "fanout_depth" (1..4, default 2)
 *                  outstanding per engine, E = max("inflight", "fanout_engines").  "fanout_engines" (1..4, default 2): engines beyond
 *                  the handle's own are created on the first such call and belong to the fan-out alone -- "inflight", the round-robin
 *                  of the other entry points and their chains per forward are not touched.  Results are bitwise those of one forward.
 *                  0 = never.  "fanout_stage": 2 (default, round 6) = the caller's array is registered with the runtime for the
 *                  duration of the call (hipHostRegister / hipHostUnregister: 2 us - 0.2 ms), so the chunk copies are asynchronous:
 *                  one host thread enqueues everything, all copies travel in order on ONE stream at the link's full rate; an
 *                  array the runtime will not register -- or whose pages overlap an array another handle's call holds -- takes
 *                  form 1.  0 / 1 = round 5's forms, one host thread per engine: chunks copied into pinned staging first / the
 *                  runtime's pageable path.  -1 = calibrate 0 against 1: both forms run once untimed, then twice each timed, the
 *                  faster serves every later call.  3 (probe) = as 2 with a copy stream per engine),
 *          "host_pinned_max" (0..4096, default 8: a blocking whenet_forward_u8 of at most this many crops travels through a
 *                  pinned staging slot -- one asynchronous H2D, the forward, three asynchronous D2H, ONE wait -- instead of
 *                  four synchronous copies from / to the caller's pageable memory: the latency path of the reference's
 *                  per-head call shape (demo.py:14, demo_video.py:27)),
 *          "se_fuse_tiny" (0..64, default 0: chains of at most this many crops behave as se_fuse = 2),
 *          "host_lanes" (1..8, default 2: chains a BLOCKING host forward runs as; "lanes" sets both),
 *          "min_lane_crops" (>= 1, default 16: the smallest sub-batch a lane may get; "lanes" is cut down until every
 *                  lane has at least this many crops.  Tests set 1 to force several lanes on small batches),
 *          "repeat" (1..16, default 1, measurement only: the captured graph holds this many back-to-back copies of
 *                  the forward, so that one graph launch times `repeat` forwards without the launch boundary
 *                  between them; results are those of one forward),
 *          "pw_staged" (0/1, default 1: the K >= 1152 and the 14 x 14 K = 672 project GEMMs of f16 / f32s handles fetch their
 *                  activation rows coalesced -- 8 rows x 128 contiguous bytes per wave-instruction -- and hand them to the matrix
 *                  cores through per-wave LDS (whenet_pw_splitk_staged_kernel) instead of loading MFMA fragments (16 bytes of each
 *                  of 32 rows: 32 cache lines per KB) from global memory; 0 = the direct kernel everywhere.  Another summation
 *                  order: results agree to rounding.  Chosen by layer, never by batch),
 *          "split_pw" (0/1, default 1, WHENET_F32S handles only: 0 runs the exact-f32 kernels -- bitwise a WHENET_F32 handle),
 *          "xcd_map" (bit mask 0..7, default 7: the workgroups of a launch that read the SAME input -- the channel chunks of one crop and
 *                  tile -- are dealt to one XCD (one L2) instead of round-robin over the eight: 1 = the fused expand+depthwise kernels,
 *                  2 = the 7 x 7 form, 4 = the head conv.  A relabelling of workgroups: the same bits.  +0.8 % with the chip full, slower for
 *                  one small forward alone -- so it is applied to launches of >= 128 crops and to every launch of a handle with
 *                  "inflight" > 1),
 *          "mb7" (0/1, default 0, WHENET_F16 handles: blocks 13-16 -- the 7 x 7 stage -- run as ONE launch each, one workgroup per crop
 *                  with the expanded tensor, the depthwise output, the squeeze-excite gate in LDS (mb7.hip) instead of front + squeeze-
 *                  excite + project launches.  29 us per launch whatever the batch up to 256 crops: +3 % at batch 512, +-1 % at 64
 *                  crops x 3 in flight, -4 % one forward at a time, +60 us at batch 1 -- the schedule must not depend on the batch, so it
 *                  is not the default.  Another rounding path of the same function: binary16 squeeze-excite kernels, other orders of
 *                  summation; bitwise independent of the batch like every other schedule),
 *          "act_layout" (0..2, default 1, WHENET_F16 handles: how the tensors between the 7 x 7 blocks -- the outputs of the project
 *                  convs of blocks 12-16, C = 192 / 320 -- lie in the activation arena.  0 = NHWC everywhere; 1 = the per-layer
 *                  table: 16-channel blocks [crop][C/16][HW][16] where that is the faster form; 2 = 16-channel blocks wherever
 *                  the producer and every consumer of a tensor know the layout (today the same tensors as 1).  In the blocked
 *                  form the 32 pixels x 16 channels of one matrix-core operand are whole cache lines (1 KB in one or two runs)
 *                  instead of 16 bytes of each of 32 pixel rows.  Pure addressing, the same bytes per crop: the results are
 *                  bitwise the same for every value.  A function of the layer, never of the batch; tensors touched by "mb7",
 *                  by "front7" = 0, by the 14 x 14 front kernels or by the unfused kernels stay NHWC, as do the inputs and
 *                  outputs of the whenet_op_* entry points),
 *          "pw_impl" (0 = MFMA kernels, 1 = scalar-FMA check kernels, same results class) */
WHENET_API int whenet_set_option(whenet_t* h, const char* key, long value);

/* ---- the hot path: replaces WHENet.get_angle (whenet.py:22-34) =
 * normalise (23-26) -> Model.predict (27) -> softmax-expectation decode (28-33).
 *   crops   uint8 [n,224,224,3] RGB
 *   ypr     float [n,3]   yaw, pitch, roll in degrees           (required)
 *   argmax  int32 [n,3]   argmax bin of each head's logits      (may be NULL): the first index of the maximum, as np.argmax --
 *                         NaN counts as the maximum and the first NaN wins, so a crop with NaN logits gives 0, 0, 0; always
 *                         inside the head's 120 / 66 / 66 bins
 *   logits  float [n,252] what Model.predict returns, concatenated (may be NULL)
 * Host-pointer form: copies in, runs, copies out, returns when the results are in place. */
WHENET_API int whenet_forward_u8(whenet_t* h, const uint8_t* crops, int n,
                      float* ypr, int32_t* argmax, float* logits);

/* The same path for REAL-VALUED input: `image` is the normalised float32 image [n,224,224,3] that
 * the reference hands to Model.predict (whenet.py:27) -- i.e. (img/255 - mean)/std computed by
 * the caller as whenet.py:23-26 does (float64, then cast).  whenet.py:25 divides any numeric array
 * by 255, so crops that are not 8-bit integers (no byte LUT applies) take this entry point; the
 * drop-in get_angle routes them here.  Host pointers, blocking, eager launches.  An f16 handle computes in
 * binary16 activations: finite normalised inputs beyond +-65504 saturate there (an f32 handle takes any finite float32).
 * NON-FINITE INPUT: a crop that holds a NaN or an infinite element comes back with NaN angles and NaN logits (all 3 and all
 * 252: the squeeze-excite gates spread it over the crop), and its argmax is np.argmax of those logits: 0, 0, 0.  Every other
 * crop of the call is untouched: bitwise what the same call gives with a finite crop in that place. */
WHENET_API int whenet_forward_f32(whenet_t* h, const float* image, int n,
                       float* ypr, int32_t* argmax, float* logits);

/* Device-pointer form: all pointers are device memory on the handle's GPU; the work is
 * enqueued on `stream` (a hipStream_t; NULL = the handle's own stream, or with option "inflight"
 * > 1 the next of the handle's engines) and the call returns without waiting.  This is the form
 * bench.py times (inputs resident in HBM).
 * ORDERING: an engine has ONE activation arena, so two forwards of the same engine must not overlap.
 * Calls with stream == NULL are ordered by the engine's own stream.  A caller that passes its own
 * streams must order successive calls itself (same stream, or an event between them): the library does
 * not insert cross-stream dependencies, and two forwards enqueued on different caller streams of one
 * engine would race on the arena.  For concurrent forwards use option "inflight" (one arena per engine). */
WHENET_API int whenet_forward_u8_device(whenet_t* h, const uint8_t* d_crops, int n,
                             float* d_ypr, int32_t* d_argmax, float* d_logits, void* stream);
WHENET_API int whenet_sync(whenet_t* h);

/* Pipelined host form for per-frame callers (demo_video.py:56-58 runs one get_angle per
 * detected head, sequentially): submit copies the crops into pinned memory and enqueues
 * H2D + forward + D2H on the handle's stream; collect waits for that submission. Up to
 * WHENET_MAX_INFLIGHT submissions may be outstanding, collected in FIFO order. */
#define WHENET_MAX_INFLIGHT 4
WHENET_API int whenet_submit_u8(whenet_t* h, const uint8_t* crops, int n, int* ticket);
WHENET_API int whenet_collect(whenet_t* h, int ticket, float* ypr, int32_t* argmax, float* logits);

/* ---- per-frame pre-processing on the device: replaces the host work of
 * process_detection (demo_video.py:13-24) and crop_and_pred (demo.py:8-11) for ALL heads of a
 * frame, and the per-head get_angle calls of demo_video.py:56-58, by one submission.
 *
 * whenet_frame_rects: the bbox margin arithmetic of demo_video.py:13-19 (float32, as YOLO's boxes
 * are; y_max / x_max use the already-moved y_min / x_min) followed by the int() truncation and
 * slice clipping of demo_video.py:21.  bboxes [k,4] = (y_min, x_min, y_max, x_max) as
 * YOLO.detect returns them; rects [k,4] = (y0, x0, y1, x1), the window img[y0:y1, x0:x1].
 * Pure host arithmetic, no GPU needed.  (demo.py:9-10 uses its integer bbox as the window directly.) */
#define WHENET_RGB 0            /* frame is already RGB            (demo.py:8 converts first)       */
#define WHENET_BGR 1            /* frame is BGR as cv2 delivers it (demo_video.py:22 swaps per crop) */
WHENET_API int whenet_frame_rects(int frame_h, int frame_w, const float* bboxes, int k, int32_t* rects);
/* whenet_normalise_table: the image of /root/reference/whenet.py:23-26 (`img/255`, `(img-mean)/std` in float64) followed by
 * Keras' cast to float32 (whenet.py:27) for every byte value: lut[c*256 + v], c = R,G,B.  This is the table the stem
 * kernels apply to uint8 crops.  Pure host arithmetic, no GPU needed. */
WHENET_API int whenet_normalise_table(float lut[768]);
/* frame uint8 [frame_h, frame_w, 3] (host).  Copies the frame into pinned memory and enqueues
 * H2D(frame) -> crop + colour order + cv2.resize-compatible bilinear to [k,224,224,3] on the device
 * -> forward -> D2H of the results; whenet_collect(ticket, ...) returns the k heads' outputs in
 * rect order.  k = 0 (no head in the frame) is valid.  An empty or out-of-frame window is
 * WHENET_EINVAL (cv2.resize raises on an empty source). */
WHENET_API int whenet_submit_frame(whenet_t* h, const uint8_t* frame, int frame_h, int frame_w, int channel_order,
                        const int32_t* rects, int k, int* ticket);
/* the crop/resize kernel alone (host pointers): crops uint8 [k,224,224,3] RGB, exactly the array
 * get_angle would have been handed */
WHENET_API int whenet_op_crop_resize(whenet_t* h, const uint8_t* frame, int frame_h, int frame_w, int channel_order,
                          const int32_t* rects, int k, uint8_t* crops);

/* ---- the detector's PRE-processing on the device: replaces `letterbox_image` (yolo_v3/utils.py:23-34: Pillow BICUBIC resize at
 * unchanged aspect ratio, pasted centred on a grey (128, 128, 128) canvas) and `np.array(boxed_image, 'float32') / 255.`
 * (yolo_v3/yolo_postprocess.py:186-196), which YOLO.detect runs on the host for every frame.  Bit-exact with Pillow's 8-bit
 * resample: its coefficient tables are computed on the host in double exactly as Pillow computes them, the kernels are int32
 * arithmetic.  out_h / out_w are the reference's `model_image_size` (h, w); the reference asserts multiples of 32, this
 * interface takes any size.  LIMITS: frame sides 1..8192, output sides 1..4096; a frame so thin that the resized image would
 * have a side of zero pixels is WHENET_EINVAL (Pillow raises there).
 *
 * whenet_letterbox_plan: the geometry -- geom = {nw, nh, x0, y0}: size of the resized image and where it is pasted -- and the
 * resample tables of one axis (0 = horizontal, in_w -> nw; 1 = vertical, in_h -> nh) as the kernels use them:
 * bounds [n_out][2] = (first source pixel, number of taps), coeffs [n_out][*ksize] int32 with 22 fractional bits, zero beyond the
 * taps.  `cap` = ints `coeffs` can hold (n_out * *ksize needed; `bounds` holds 2 * n_out).  bounds and coeffs may both be NULL:
 * geom and *ksize alone.  Pure host arithmetic, no GPU needed. */
WHENET_API int whenet_letterbox_plan(int in_h, int in_w, int out_h, int out_w, int32_t geom[4], int axis, int32_t* bounds,
                          int32_t* coeffs, int cap, int* ksize);
/* the stage alone (host pointers): frame uint8 [frame_h, frame_w, 3] -> canvas_u8 uint8 [out_h, out_w, 3] and / or image_f32
 * float [out_h, out_w, 3] = canvas / 255 in float32, the `image_data` YOLO.detect feeds to sess.run (before its batch axis).
 * Either output may be NULL.  Works on a whenet_create_postproc handle. */
WHENET_API int whenet_op_letterbox(whenet_t* h, const uint8_t* frame, int frame_h, int frame_w, int channel_order, int out_h,
                        int out_w, uint8_t* canvas_u8, float* image_f32);
/* The RESIDENT-FRAME form of whenet_submit_frame for a caller that also wants the detector input: the frame crosses PCIe once,
 * when it arrives, and the detector input and the head crops are both cut from that one device copy.
 *   whenet_frame_begin      pinned staging copy + asynchronous H2D of the frame; hands out the ticket and HOLDS the submission
 *                           slot from here on (order, WHENET_MAX_INFLIGHT and option "inflight" as for whenet_submit_frame)
 *   whenet_frame_letterbox  the letterbox of the resident frame, results through pinned memory with one wait; any number of
 *                           times (any sizes) before the heads are enqueued
 *   whenet_frame_heads      crop plans -> crop / resize -> forward -> D2H enqueued exactly as whenet_submit_frame does, without
 *                           copying the frame again; k = 0 is valid
 *   whenet_collect          returns the k heads' results and frees the slot
 * A ticket that never gets heads is released by whenet_frame_heads(h, ticket, NULL, 0) + whenet_collect.  An unknown ticket,
 * heads enqueued twice and a letterbox after the heads are WHENET_EINVAL; the handle stays usable. */
WHENET_API int whenet_frame_begin(whenet_t* h, const uint8_t* frame, int frame_h, int frame_w, int channel_order, int* ticket);
WHENET_API int whenet_frame_letterbox(whenet_t* h, int ticket, int out_h, int out_w, uint8_t* canvas_u8, float* image_f32);
WHENET_API int whenet_frame_heads(whenet_t* h, int ticket, const int32_t* rects, int k);

/* ---- the detector's post-processing on the device: replaces yolo_eval (yolo_v3/model.py:193-232 =
 * yolo_head :125-150, yolo_correct_boxes :153-178, yolo_boxes_and_scores :181-190, per-class
 * tf.image.non_max_suppression), which the reference runs inside sess.run (yolo_postprocess.py:198-204).
 *   feats        num_layers host pointers to the detector's output maps, float32 [grid_h][grid_w][3*(5+num_classes)]
 *                (batch of one, as YOLO.detect feeds it), coarsest map first like the Keras model's outputs
 *   anchors      num_anchors x (w, h) as in yolo_anchors.txt; 3 maps need 9 anchors, 2 maps ("tiny") 6
 *   image_h/w    size of the original image (`input_image_shape`); the network input is 32 x the first map's grid
 *   max_boxes    per class, any value >= 1 as the reference (default 20; more than 256 selections per class spill from
 *                LDS to the output array); score: `>= score_threshold`; NMS drops IoU `> iou_threshold`
 *   boxes        float [num_classes*max_boxes][4]  y_min, x_min, y_max, x_max in image pixels (not clipped, as the reference)
 *   scores, classes, index (may be NULL: the box's position in the concatenated (map, y, x, anchor) list)
 *   count        number of detections written, class by class, descending score inside a class
 *   all_boxes [N][4], all_scores [N][num_classes] (may be NULL): every decoded box / score, for tests
 * Equal scores are taken lower index first (TensorFlow leaves ties to its heap). */
WHENET_API int whenet_yolo_eval(whenet_t* h, const float* const* feats, const int* grid_h, const int* grid_w,
                     int num_layers, const float* anchors, int num_anchors, int num_classes, float image_h,
                     float image_w, float score_threshold, float iou_threshold, int max_boxes, float* boxes,
                     float* scores, int32_t* classes, int32_t* index, int* count, float* all_boxes,
                     float* all_scores);

/* ---- the detector's network on the device (ABI 6): yolo_body / tiny_yolo_body (yolo_v3/model.py:20-122) between the letterbox
 * and whenet_yolo_eval, so that YOLO.detect (yolo_postprocess.py:180-205) needs no TensorFlow.  binary16 storage with f32
 * accumulation by default, float32 storage by option "detector_dtype".
 *   whenet_detector_load[_from_memory]  attaches a detector to ANY handle (a model handle or a whenet_create_postproc one); replaces
 *                  tiny_yolo_body / yolo_body + load_weights (yolo_postprocess.py:66-79).  A WHNPACK1 container holding
 *                  dconvNNN/kernel (Keras HWIO), dbnNNN/{gamma,beta,moving_mean,moving_variance} and, for the output convolutions,
 *                  dconvNNN/bias, numbered from 000 in the reference's layer-creation order (convolutions and BatchNorms counted
 *                  apart).  75 kernels = yolo_body, 13 = tiny_yolo_body; A * (5 + C) is the output convolutions' Cout.  A missing
 *                  or mis-shaped tensor is WHENET_EFORMAT with its name in whenet_last_error.
 *   whenet_detector_spec  pure host logic, no GPU: kind 0 = yolo_body, 1 = tiny_yolo_body; row `index` (0-based; convolutions and
 *                  pools in creation order) as {op (0 conv, 1 max-pool), k, stride, cin, cout, bn, leaky, src0, src1, skip,
 *                  is_output, cin_of_src0}.  src0 / src1 / skip are rows (-1: the image / none): with src1 >= 0 the input is
 *                  Concatenate()([UpSampling2D(2)(src0), src1]); skip is the Add() operand; a stride-2 convolution pads top and left
 *                  only.  *count = rows (75 / 19).  `out` may be NULL to ask for the count alone.
 *   whenet_op_dconv / whenet_op_dpool  one layer on caller tensors (host pointers, float32 in / out, converted on the device like
 *                  whenet_op_*): exactly the kernels the body runs.  in [n,H,W,cin] -- with in2 [n,H,W,cin2] it is the
 *                  HALF-resolution tensor [n,H/2,W/2,cin]; kernel HWIO [k,k,cin+cin2,cout]; bias [cout] (a folded BatchNorm's);
 *                  skip [n,Ho,Wo,cout] or NULL; f32_out selects the output convolutions' float32 store (else one rounding to
 *                  binary16 under detector_dtype 0).  cin = 3 runs the body's first-layer input stage.  Pool: 2x2 'same', stride 1 or 2.
 *   whenet_detector_forward  the body alone = yolo_model.predict(image_data): image float32 [n,H,W,3] (H, W multiples of 32 in
 *                  32..1024, n 1..16) -> maps[l] float32 [n][H/32 << l][W/32 << l][A*(5+C)], coarsest first (3 maps, tiny 2)
 *   whenet_op_detect  YOLO.detect on a host frame: letterbox -> body -> yolo_eval without leaving the device; outputs as
 *                  whenet_yolo_eval's (boxes [C*max_boxes][4], scores, classes; image shape = the frame's)
 *   whenet_frame_detect  the same on a resident frame, between whenet_frame_begin and whenet_frame_heads
 *   option "detector_dtype" (whenet_set_option; 0 = binary16 storage, default; 1 = float32): the storage type of the body's weights
 *                  and activations.  Read by whenet_detector_load[_from_memory], which packs the weights for it; every entry point
 *                  that runs the body (forward, op_detect, frame_detect, frame / clip_detect_heads) follows the LOADED detector;
 *                  whenet_op_dconv / whenet_op_dpool run the kernels of the handle's current value.  1 keeps float32 from the image
 *                  to the maps (v_mfma_f32_32x32x2_f32, BatchNorm folded in float64 and rounded once to float32, nothing rounded to
 *                  binary16): the parity-grade body, whose boxes give the float64 evaluation's crop windows.  Any other value is
 *                  WHENET_EINVAL; so is a change while a detector is attached (set it on a handle without one, then load again).
 * A handle without a loaded detector answers forward / detect with WHENET_EINVAL and stays usable. */
WHENET_API int whenet_detector_load(whenet_t* h, const char* snapshot_path);
WHENET_API int whenet_detector_load_from_memory(whenet_t* h, const void* snapshot, size_t nbytes);
WHENET_API int whenet_detector_spec(int kind, int anchors_per_scale, int num_classes, int index, int32_t out[12], int* count);
WHENET_API int whenet_op_dconv(whenet_t* h, const float* in, int n, int H, int W, int cin, const float* in2, int cin2,
                    const float* kernel, const float* bias, int k, int stride, int cout, int leaky, const float* skip,
                    int f32_out, float* out);
WHENET_API int whenet_op_dpool(whenet_t* h, const float* in, int n, int H, int W, int c, int stride, float* out);
WHENET_API int whenet_detector_forward(whenet_t* h, const float* image, int n, int H, int W, float* const* maps);
WHENET_API int whenet_op_detect(whenet_t* h, const uint8_t* frame, int frame_h, int frame_w, int channel_order, int out_h, int out_w,
                     const float* anchors, int num_anchors, float score_threshold, float iou_threshold, int max_boxes,
                     float* boxes, float* scores, int32_t* classes, int* count);
WHENET_API int whenet_frame_detect(whenet_t* h, int ticket, int out_h, int out_w, const float* anchors, int num_anchors,
                        float score_threshold, float iou_threshold, int max_boxes, float* boxes, float* scores,
                        int32_t* classes, int* count);

/* ---- ONE submission per video frame: detect, crop and pose without the host in between.  whenet_frame_detect takes the boxes
 * to the host (it waits for the detector), the caller turns them into windows and whenet_frame_heads uploads their crop plans;
 * here the selected boxes stay on the device, a kernel computes the windows (whenet_frame_rects) and crop plans from them, and the
 * heads are cropped and run over the CAPACITY classes x max_boxes (rows without a head are zero crops; a crop's result does not
 * depend on the batch or on its position, so head i is bitwise what the two-step path returns for detection i).
 *   whenet_frame_detect_heads  between whenet_frame_begin and the collect, in the place of whenet_frame_detect + whenet_frame_heads:
 *                  letterbox -> body -> yolo_eval -> windows + crop plans -> crop / resize -> forward -> D2H, ENQUEUE-ONLY: it returns
 *                  without waiting for the device (buffers are allocated and graphs captured on the first call for a shape).  Arguments
 *                  as whenet_frame_detect; classes x max_boxes must be 1..64 (the head detector has one class, the reference's
 *                  default max_boxes is 20).  Needs a network AND a detector on the handle.  The ticket then behaves like one whose
 *                  heads are enqueued.
 *   whenet_collect_detect  waits once and returns *count detections, class by class as whenet_yolo_eval orders them: boxes [count][4],
 *                  scores, classes, rects [count][4] = (y0, x0, y1, x1) as whenet_frame_rects, valid [count] = 1 iff the window is
 *                  non-empty and inside the frame (what whenet_frame_heads rejects with WHENET_EINVAL; the device cannot raise, so the
 *                  head is skipped and reported), and the heads' results ypr [count][3], argmax [count][3], logits [count][252]
 *                  (the last two may be NULL); rows of invalid heads are NaN / -1 / NaN.  `capacity` = rows the arrays hold, at least
 *                  classes x max_boxes of the submission.  WHENET_EINVAL for a ticket that whenet_frame_detect_heads did not submit;
 *                  whenet_collect answers such a ticket the same way.  Either error leaves the ticket collectable.
 *   whenet_op_head_plan  the window / crop plan kernel alone on caller boxes [k][4] (host pointers, k 1..2048): rects [k][4], valid [k],
 *                  plans [k][WHENET_CROP_PLAN_INTS] (may be NULL; zeros where valid is 0).  Works on a whenet_create_postproc handle.
 *   whenet_crop_plan  the crop plan of one window as the host computes it for whenet_frame_heads: {y0, x0, h, w, 2x-shrink flag (set
 *                  for a 448 x 448 window only: cv2.resize switches to INTER_AREA), xmax (first output column that reads a single
 *                  sample), 0, 0} followed by six 224-entry tables xofs | a0 | a1 | yofs | b0 | b1 (OpenCV's INTER_LINEAR offsets and
 *                  11-bit coefficients).  An empty window is WHENET_EINVAL.  Pure host arithmetic, no GPU needed. */
#define WHENET_CROP_PLAN_INTS (8 + 6 * 224)
WHENET_API int whenet_frame_detect_heads(whenet_t* h, int ticket, int out_h, int out_w, const float* anchors, int num_anchors,
                              float score_threshold, float iou_threshold, int max_boxes);
WHENET_API int whenet_collect_detect(whenet_t* h, int ticket, int capacity, int* count, float* boxes, float* scores, int32_t* classes,
                          int32_t* rects, int32_t* valid, float* ypr, int32_t* argmax, float* logits);
WHENET_API int whenet_op_head_plan(whenet_t* h, int frame_h, int frame_w, const float* boxes, int k, int32_t* rects, int32_t* valid,
                        int32_t* plans);
WHENET_API int whenet_crop_plan(const int32_t rect[4], int32_t* plan);

/* ---- CLIPS: several frames per submission (additions to ABI 6).  A caller that reads a video file or a rig of identical
 * cameras has the next frames in hand; a clip sends F of them, 1 <= F <= 16, all of one size and channel order, through
 * letterbox, detector, selection, head plans, crops and pose as ONE submission.  Every frame's results are bit for bit those of
 * whenet_frame_begin + whenet_frame_detect_heads + whenet_collect_detect on that frame alone.
 *   whenet_clip_begin  stands for F iterations of `ret, frame = cap.read()` (demo_video.py:49-53): frames uint8
 *                  [F][frame_h][frame_w][3] contiguous; one pinned staging copy, one asynchronous H2D; hands out the ticket and holds
 *                  one submission slot like whenet_frame_begin.  A clip that never gets its heads is released by
 *                  whenet_frame_heads(h, ticket, NULL, 0) + whenet_collect.
 *   whenet_clip_detect_heads  stands for F iterations of demo_video.py:54-58 (YOLO.detect, then process_detection per box):
 *                  ENQUEUE-ONLY like whenet_frame_detect_heads, arguments as there.  Per frame there are
 *                  *slots_per_frame = K = classes x max_boxes detection slots (max_boxes cut to the number of boxes the maps hold);
 *                  F x K <= 1024.  The heads that have a window inside the frame are numbered in (frame, detection) order and the
 *                  r-th of them becomes row r of ONE forward over max_heads rows, 1..256 (0 = min(F x K, 256)); rows without a head
 *                  are zero crops, heads beyond max_heads are counted in *overflow and get no result.
 *   whenet_collect_clip  waits once.  Arrays over F x K slots, slot (f, i) at f * K + i: boxes [.][4], scores, classes, rects [.][4],
 *                  valid as whenet_collect_detect returns them for frame f (slots from counts[f] on: zeros, class -1, valid 0);
 *                  row [.] = the slot's forward row or -1 (no window, beyond the count, or over max_heads); ypr [.][3], argmax [.][3],
 *                  logits [.][252] (the last two may be NULL) = the row's results, NaN / -1 / NaN where row is -1.  counts [F],
 *                  *num_frames = F, *rows_used = forward rows that hold a head, *overflow = heads that got none.  `capacity` = slots the
 *                  arrays hold, at least F x K; counts holds 16.  WHENET_EINVAL for a ticket whenet_clip_detect_heads did not submit;
 *                  whenet_collect and whenet_collect_detect answer a clip ticket the same way.  Errors leave the ticket collectable.
 * whenet_frame_letterbox / _heads (k > 0) / _detect / _detect_heads on a clip ticket and whenet_clip_detect_heads on a frame
 * ticket are WHENET_EINVAL; the handle stays usable.
 *   whenet_op_letterbox_batch  letterbox_image (yolo_v3/utils.py:23-34, yolo_postprocess.py:186-196) of F host frames
 *                  [F][frame_h][frame_w][3] -> canvas_u8 [F][out_h][out_w][3] and / or image_f32, as whenet_op_letterbox per frame
 *   whenet_yolo_eval_batch  yolo_eval (yolo_v3/model.py:193-232) of num_images images that share shape and thresholds: feats[l] =
 *                  host map [num_images][grid_h][grid_w][3*(5+C)]; with M = min(max_boxes, boxes the maps hold), image f's
 *                  detections are rows f * C * M .. + counts[f] of boxes [.][4], scores, classes, index (may be NULL), each as
 *                  whenet_yolo_eval returns them for that image alone
 *   whenet_op_head_compact  the numbering of a clip's heads alone (host pointers): valid [F x K], count [F] -> row [F x K],
 *                  slot_of_row [max_heads] (-1: an empty row), *rows_used, *overflow; F x K <= 1024, max_heads 1..256.  Works on a
 *                  whenet_create_postproc handle, like the two above. */
WHENET_API int whenet_clip_begin(whenet_t* h, const uint8_t* frames, int num_frames, int frame_h, int frame_w, int channel_order,
                      int* ticket);
WHENET_API int whenet_clip_detect_heads(whenet_t* h, int ticket, int out_h, int out_w, const float* anchors, int num_anchors,
                             float score_threshold, float iou_threshold, int max_boxes, int max_heads, int* slots_per_frame);
WHENET_API int whenet_collect_clip(whenet_t* h, int ticket, int capacity, int* num_frames, int32_t* counts, float* boxes, float* scores,
                        int32_t* classes, int32_t* rects, int32_t* valid, int32_t* row, float* ypr, int32_t* argmax, float* logits,
                        int* rows_used, int* overflow);
WHENET_API int whenet_op_letterbox_batch(whenet_t* h, const uint8_t* frames, int num_frames, int frame_h, int frame_w, int channel_order,
                              int out_h, int out_w, uint8_t* canvas_u8, float* image_f32);
WHENET_API int whenet_yolo_eval_batch(whenet_t* h, const float* const* feats, int num_images, const int* grid_h, const int* grid_w,
                           int num_layers, const float* anchors, int num_anchors, int num_classes, float image_h, float image_w,
                           float score_threshold, float iou_threshold, int max_boxes, float* boxes, float* scores,
                           int32_t* classes, int32_t* index, int32_t* counts);
WHENET_API int whenet_op_head_compact(whenet_t* h, const int32_t* valid, const int32_t* count, int num_frames, int slots_per_frame,
                           int max_heads, int32_t* row, int32_t* slot_of_row, int32_t* rows_used, int32_t* overflow);

/* ---- MIXED CLIPS: frames of different sizes in one submission, and the letterbox geometry cache (additions to ABI 6).  A rig
 * of different cameras, or several files served by one handle, sends frames whose sizes differ.  Only the stages before and
 * after the detector body depend on the frame size (the letterbox, the box correction of the decode, the head windows and the
 * crops); the body, the selection and the forward see [F][out_h][out_w] canvases and slot arrays either way.  Frame f of a
 * mixed clip returns, bit for bit, what whenet_frame_begin + whenet_frame_detect_heads + whenet_collect_detect return for it alone.
 *   whenet_clip_begin_mixed  stands for one `ret, frame = cap.read()` (demo_video.py:49-53) on each of F sources, 1 <= F <= 16:
 *                  frames[f] = uint8 [frame_h[f]][frame_w[f]][3], sides 1..8192, one channel order.  The frames are packed back
 *                  to back (no padding) with one pinned staging copy and one asynchronous H2D.  The ticket goes to
 *                  whenet_clip_detect_heads and whenet_collect_clip exactly as whenet_clip_begin's does (demo_video.py:54-58 per
 *                  frame; the letterbox of every frame is yolo_v3/utils.py:23-34 with that frame's size, the box correction
 *                  yolo_v3/model.py:153-178 with that frame's image_shape); a clip that never gets its heads is released by
 *                  whenet_frame_heads(h, ticket, NULL, 0) + whenet_collect.  WHENET_EINVAL, with the frame's index in
 *                  whenet_last_error and before anything is enqueued or a slot is taken: F outside 1..16, a NULL frame, a side
 *                  outside 1..8192, more frames than option "letterbox_cache"; from whenet_clip_detect_heads: a frame whose
 *                  resized image would be empty at that detector input (the ticket stays releasable).
 *   whenet_op_letterbox_mixed  letterbox_image (yolo_v3/utils.py:23-34, yolo_postprocess.py:186-196) of F host frames of their
 *                  own sizes -> canvas_u8 [F][out_h][out_w][3] and / or image_f32, as whenet_op_letterbox per frame.
 *   whenet_yolo_eval_mixed  whenet_yolo_eval_batch (yolo_v3/model.py:193-232) for images of different shapes: image_shapes
 *                  [num_images][2] = (h, w) of each image, as yolo_correct_boxes (model.py:153-178) takes image_shape, in place
 *                  of the two scalars; every other argument and the output layout as there.
 *   whenet_letterbox_cache_stats  out = {entries, hits, misses, host_waits} of the letterbox geometry cache, summed over the
 *                  handle's engines.  Every engine keeps the resample tables (Pillow's coefficients, utils.py:31) of up to N
 *                  geometries (frame_h, frame_w, out_h, out_w) on the device, N = option "letterbox_cache", 1..32, default 16
 *                  (setting it waits for the handle's work and empties the cache).  A frame whose geometry is cached enqueues no
 *                  table copy and waits for nothing; a new geometry replaces the least recently used one and waits at most --
 *                  host_waits counts it -- for that entry's own previous table copy, never for the stream: sources of different
 *                  sizes alternating on one handle keep the pipeline of whenet_frame_detect_heads enqueue-only. */
WHENET_API int whenet_clip_begin_mixed(whenet_t* h, const uint8_t* const* frames, int num_frames, const int* frame_h, const int* frame_w,
                            int channel_order, int* ticket);
WHENET_API int whenet_op_letterbox_mixed(whenet_t* h, const uint8_t* const* frames, int num_frames, const int* frame_h, const int* frame_w,
                              int channel_order, int out_h, int out_w, uint8_t* canvas_u8, float* image_f32);
WHENET_API int whenet_yolo_eval_mixed(whenet_t* h, const float* const* feats, int num_images, const int* grid_h, const int* grid_w,
                           int num_layers, const float* anchors, int num_anchors, int num_classes, const float* image_shapes,
                           float score_threshold, float iou_threshold, int max_boxes, float* boxes, float* scores,
                           int32_t* classes, int32_t* index, int32_t* counts);
WHENET_API int whenet_letterbox_cache_stats(whenet_t* h, int32_t out[4]);

/* ---- YUV 4:2:0 INGEST: a decoder's planes in, the resident BGR frame built on the device (additions to ABI 6).  Video decoders
 * and MJPEG cameras deliver 4:2:0 YUV; `cap.read()` (demo_video.py:51) hides a software conversion to BGR.  Here the planes are
 * uploaded as they are (1.5 bytes per pixel instead of 3) and converted by a kernel (csrc/yuv.hip) on the copy stream, behind the
 * upload and before the event every consumer of the frame waits for: the slot then holds the packed BGR frame [h][w][3], recorded
 * as whenet_frame_begin(..., WHENET_BGR) records it, and everything downstream is unchanged.
 *
 * The conversion, integers only.  Frame of h x w luma samples, 1 <= h, w <= 8192, odd sizes included; chroma planes of
 * ch = (h + 1) >> 1 rows by cw = (w + 1) >> 1 samples; pixel (y, x) takes the chroma sample (y >> 1, x >> 1) (nearest neighbour).
 * With int32 arithmetic and >> an arithmetic shift:
 *     c = max(0, Y - yoff);  d = U - 128;  e = V - 128
 *     R = clip8((CY * c           + CVR * e + (1 << 19)) >> 20)
 *     G = clip8((CY * c - CUG * d - CVG * e + (1 << 19)) >> 20)
 *     B = clip8((CY * c + CUB * d           + (1 << 19)) >> 20)
 * and {yoff, CY, CVR, CUG, CVG, CUB} = WHENET_YUV_COEFFS[matrix]:
 *     WHENET_YUV_BT601  video range, the constants of OpenCV's cvtColor (1.164, 1.596, 0.391, 0.813, 2.018 x 2^20, truncated)
 *     WHENET_YUV_BT709  video range, rint(2^20 x {255/219, 1.5748 x 255/224, 0.1873 x 255/224, 0.4681 x 255/224, 1.8556 x 255/224})
 *     WHENET_YUV_JFIF   full range (MJPEG), rint(2^20 x {1, 1.402, 0.344136, 0.714136, 1.772})
 *   WHENET_YUV_NV12  plane[0] = Y, plane[1] = U and V interleaved (U at 2 (x >> 1), V behind it), plane[2] unused
 *   WHENET_YUV_I420  plane[0] = Y, plane[1] = U, plane[2] = V
 * Every plane has its own byte pitch >= its row bytes (w; 2 cw for the interleaved plane; cw).
 * PACKED 4:2:2 (what a V4L2 / UVC camera or a capture card delivers raw), through the same struct and the same ten calls:
 *   WHENET_YUV_YUYV  (also called YUY2) bytes Y0 U Y1 V per pixel pair
 *   WHENET_YUV_UYVY  bytes U Y0 V Y1 per pixel pair
 * One plane: plane[0] has h rows of 4 cw bytes, cw = (w + 1) >> 1, pitch[0] >= 4 cw; plane[1..2] and pitch[1..2] are ignored (NULL
 * is allowed).  Sides 1..8192, odd widths included: the last pair of an odd row is whole in memory and its second luma byte is not
 * used.  Pixel (y, x) takes luma Y[x & 1] of pair x >> 1 of row y and THAT pair's U and V: nearest neighbour horizontally and NO
 * vertical sharing (every row has its own chroma), the one difference from the 4:2:0 rule above.  The arithmetic is the one above,
 * unchanged: c = max(0, Y - yoff), 20 fractional bits, the three WHENET_YUV_COEFFS rows.  BT.601 stays restated, unpinned for
 * these formats too (OpenCV's COLOR_YUV2BGR_YUY2 uses the same constants and has never been run against this); JFIF inherits the
 * Pillow pin of tests/test_yuv_cpu.py because the per-pixel function is shared.  A clip may mix NV12, I420, YUYV and UYVY frames
 * of different sizes and matrices.  Not built: YVYU / VYUY, planar 4:2:2 / 4:4:4, interpolated chroma, packed destinations.
 *   whenet_yuv_to_bgr_host  the conversion as pure host arithmetic (no GPU needed): bgr = uint8 [h][w][3]; the text of an error is
 *                  whenet_last_error(NULL)'s, the frame's index in it is 0
 *   whenet_op_yuv_to_bgr    the kernel alone, host to host, on 1..16 frames of their own sizes, formats and matrices: bgr[f] = uint8
 *                  [h_f][w_f][3].  On the device the frames lie back to back as a mixed clip packs them.  Works on a
 *                  whenet_create_postproc handle.
 *   whenet_frame_begin_yuv  as whenet_frame_begin: the ticket goes to whenet_frame_letterbox / _detect / _heads / _detect_heads and
 *                  the collect calls unchanged.
 *   whenet_clip_begin_yuv   1..16 frames, each with its own format and matrix.  All of one size: a clip as whenet_clip_begin
 *                  makes it; otherwise a mixed clip as whenet_clip_begin_mixed makes it (at most option "letterbox_cache" frames).
 * WHENET_EINVAL, with the frame's index in whenet_last_error and before a slot is taken or anything is enqueued: a NULL required
 * plane, a pitch below the plane's row bytes, an unknown format or matrix, a side outside 1..8192, a frame count outside 1..16. */
#define WHENET_YUV_NV12 0
#define WHENET_YUV_I420 1
#define WHENET_YUV_YUYV 3       /* (2 is WHENET_SURF_PACKED of whenet_surface_t; 2 is an unknown format here) */
#define WHENET_YUV_UYVY 4
#define WHENET_YUV_BT601 0
#define WHENET_YUV_BT709 1
#define WHENET_YUV_JFIF 2
#define WHENET_YUV_MATRICES 3
#define WHENET_YUV_COEFFS {{16, 1220542, 1673527, 409993, 852492, 2116026}, \
                           {16, 1220945, 1879825, 223578, 558767, 2215014}, \
                           {0, 1048576, 1470104, 360853, 748826, 1858077}}
typedef struct {
    const uint8_t* plane[3];
    int pitch[3];
    int format;
    int matrix;
    int h, w;
} whenet_yuv_frame_t;
WHENET_API int whenet_yuv_to_bgr_host(const whenet_yuv_frame_t* frame, uint8_t* bgr);
WHENET_API int whenet_op_yuv_to_bgr(whenet_t* h, const whenet_yuv_frame_t* frames, int num_frames, uint8_t* const* bgr);
WHENET_API int whenet_frame_begin_yuv(whenet_t* h, const whenet_yuv_frame_t* frame, int* ticket);
WHENET_API int whenet_clip_begin_yuv(whenet_t* h, const whenet_yuv_frame_t* frames, int num_frames, int* ticket);

/* ---- INGEST FROM DEVICE MEMORY: pitched BGR / RGB and NV12 / I420 surfaces that are already in HBM (additions to ABI 6).  The
 * card's video decoder writes its surfaces into device memory and a PyTorch-ROCm pipeline holds frames as uint8 device tensors:
 * the entry points above would have such a caller copy the frame to the host so that the library can copy it back.  These begin
 * a frame, a clip or a mixed clip from device pointers; one kernel (csrc/ingest.hip for packed pixels, csrc/yuv.hip for planes)
 * writes the slot's frame buffer, no pinned staging is touched, and everything after `begin` is unchanged: the results are bit
 * for bit those of the host-pointer call each one replaces.
 *   whenet_frame_begin_device      replaces whenet_frame_begin: d_frame = frame_h rows of 3 frame_w bytes, `pitch` bytes apart
 *   whenet_clip_begin_device       replaces whenet_clip_begin (frames all of one size) and whenet_clip_begin_mixed (otherwise; at
 *                  most option "letterbox_cache" frames): 1..16 frames, each with its own pointer, pitch and size
 *   whenet_frame_begin_yuv_device  replaces whenet_frame_begin_yuv: frame->plane[] are DEVICE pointers
 *   whenet_clip_begin_yuv_device   replaces whenet_clip_begin_yuv the same way
 *   whenet_op_pack_device          the packing kernel alone, device to host: out[f] = uint8 [h_f][w_f][3] (host), the frames packed
 *                  back to back on the device as a mixed clip packs them.  Works on a whenet_create_postproc handle; the host waits.
 *   whenet_op_yuv_to_bgr_device    the plane kernel alone, device to host, the device twin of whenet_op_yuv_to_bgr
 * ORDER.  `stream` is the caller's hipStream_t (NULL: the default stream).  The library records an event on it, lets its copy
 * stream wait for that event, runs the kernel, and makes `stream` wait for the kernel's end.  Work enqueued on `stream` BEFORE the
 * call is seen by the ingest; work enqueued on `stream` AFTER the call may overwrite or free the source; anything else that
 * writes the source (the host, another stream) must wait until the ticket's collect call has returned.  The host never waits.
 * WHENET_EINVAL, with the frame's index in whenet_last_error and before a slot is taken or anything is enqueued: a NULL pointer,
 * a pitch below the row bytes, a side outside 1..8192, a frame count outside 1..16, an unknown format or matrix; a pointer that
 * hipPointerGetAttributes does not report as hipMemoryTypeDevice memory of the handle's device (host, registered, managed and
 * other-device memory are refused); a plane whose extent (rows - 1) * pitch + row_bytes leaves the allocation that
 * hipMemGetAddressRange reports for it.  If the runtime cannot report that range, the extent check alone is skipped.
 * Not built: BGRA / 4-channel, float or CHW sources, 10-bit surfaces, memory of another GPU, IPC handles, capture of a begin
 * call into a caller's graph. */
WHENET_API int whenet_frame_begin_device(whenet_t* h, const uint8_t* d_frame, int pitch, int frame_h, int frame_w, int channel_order,
                              void* stream, int* ticket);
WHENET_API int whenet_clip_begin_device(whenet_t* h, const uint8_t* const* d_frames, const int* pitch, int num_frames, const int* frame_h,
                             const int* frame_w, int channel_order, void* stream, int* ticket);
WHENET_API int whenet_frame_begin_yuv_device(whenet_t* h, const whenet_yuv_frame_t* frame, void* stream, int* ticket);
WHENET_API int whenet_clip_begin_yuv_device(whenet_t* h, const whenet_yuv_frame_t* frames, int num_frames, void* stream, int* ticket);
WHENET_API int whenet_op_pack_device(whenet_t* h, const uint8_t* const* d_frames, const int* pitch, int num_frames, const int* frame_h,
                          const int* frame_w, void* stream, uint8_t* const* out);
WHENET_API int whenet_op_yuv_to_bgr_device(whenet_t* h, const whenet_yuv_frame_t* frames, int num_frames, void* stream, uint8_t* const* bgr);

/* ---- POSE OVERLAY: the annotated frame, produced on the device (additions to ABI 6).  demo_video.py:26-29 draws, for every head,
 * `cv2.rectangle` of its window and `draw_axis` (utils.py:13-43: three `cv2.line`s from the window's centre), then writes the frame
 * out (demo_video.py:60).  The frame, the windows and the angles are in device memory when the forward ends, so the annotated
 * frame is produced there (csrc/overlay.hip) -- into a host array, or into a pitched BGR / NV12 / I420 surface in device memory
 * for an encoder.  Built of the reference's drawing: the whole of process_detection -- the rectangle, draw_axis and, with
 * WHENET_DISPLAY_FULL, the three putText labels of `--display full` (LABELS below).  Not built: thickness / colour / font options,
 * 10-bit surfaces.
 *
 * The overlay, integers only.
 * SEGMENTS OF A HEAD.  Inputs: the window (y0, x0, y1, x1) as whenet_frame_rects / the collect calls return it, and the float32
 * angles yaw, pitch, roll in degrees.  In double precision tdx = (x0 + x1) / 2, tdy = (y0 + y1) / 2, size = (x1 - x0) // 2 (floor);
 * the angles are widened to double and go through exactly the expressions of utils.py:15-38 (every operation rounded on its own);
 * every endpoint is (int)-truncated as utils.py:40-42 does: the call INTEGRATION.md section 4 documents,
 * draw_axis(frame, y, p, r, tdx=(x0+x1)/2, tdy=(y0+y1)/2, size=(x1-x0)//2).  A head is four primitives, painted in this order:
 *     1. the rectangle outline, colour (0,0,0): the four segments (x0,y0)-(x1,y0)-(x1,y1)-(x0,y1)-(x0,y0)
 *     2. the X axis, red      (int tdx, int tdy) -> (int x1', int y1')      utils.py:28-29, :40
 *     3. the Y axis, green                       -> (int x2', int y2')      utils.py:33-34, :41
 *     4. the Z axis, blue                        -> (int x3', int y3')      utils.py:37-38, :42
 * Colours are those of utils.py:40-42 in the frame's channel order: on a WHENET_RGB frame the X axis is still red.
 * whenet_overlay_segments returns the 16 ints {x0, y0, x1, y1, then P and Q of the X, the Y and the Z axis as (x, y) pairs}.
 * A head with valid == 0, or without a forward row (clip overflow), paints nothing; a head whose angles are not all finite
 * paints its rectangle only (the ints of its axes are 0).
 * RASTER RULE.  The project's own: OpenCV has never run next to this code, so no claim is made about cv2.line's pixels.  A pixel
 * (x, y) is painted by a segment P -> Q iff its Euclidean distance to the closed segment is <= 1 -- thickness 2 with round caps --
 * decided exactly in 64-bit integers.  With d = Q - P, v = X - P, L2 = d.d:
 *     v.d <= 0:   painted iff |v|^2 <= 1
 *     v.d >= L2:  painted iff |X - Q|^2 <= 1
 *     otherwise:  painted iff (v x d)^2 <= L2
 * P = Q is a disc.  BOUNDS: frame sides are 1..8192 and the window coordinates of a painted head lie in -4096..8192 (a valid head
 * outside that range is WHENET_EINVAL at the host-pointer entry points; on the device it paints nothing), so every endpoint is below
 * 2^14 in magnitude, every difference below 2^15, |v x d| < 2^31 and its square fits a signed 64-bit integer.
 * Primitives are painted head by head in row order; where several cover a pixel the LAST one in that order wins.  Pixels outside
 * the frame are clipped.  The source frame is never modified (the head crops and the letterbox read it).
 * LABELS (display = WHENET_DISPLAY_FULL; demo_video.py:31-34).  A head paints three lines of text iff it paints its axes (flags
 * include 2: window valid and in range, all three angles finite) and every rounded angle r satisfies |r| <= 9999; otherwise it
 * paints no line and its rectangle and axes are unaffected.  Its flags then include 4.
 *     TEXT.  Line i is "yaw: ", "pitch: " or "roll: " followed by the number the executed reference prints,
 *     "{}".format(np.round(a)) for the float32 angle a: r = rintf(a) in float32 (round half to even); '-' iff signbit(r), so -0.3
 *     gives "-0.0"; the decimal digits of |r| without leading zeros; ".0".  2.5 -> "2.0", 3.5 -> "4.0", -179.6 -> "-180.0".  A line
 *     has at most 14 characters ("pitch: -9999.0").
 *     ORIGINS.  (x0, y0), (x0, y0 - 15), (x0, y0 - 30) for yaw, pitch, roll, (x0, y0) the window's corner (segments[0], [1]): as in
 *     OpenCV the baseline-left point of the line.
 *     FONT, the project's own: restated, unpinned.  OpenCV has never run next to this code and Hershey's stroke data is not part of
 *     it, so no claim is made about cv2.putText's pixels (FONT_HERSHEY_SIMPLEX, scale 0.4, thickness 1 is what the reference asks
 *     for).  WHENET_OVERLAY_GLYPHS names the 25 characters, WHENET_OVERLAY_FONT holds for each {n, then 8 rows of x0, y0, x1, y1}:
 *     its n <= 8 strokes with integer endpoints inside x in [0,5], y in [-9,3] relative to the character's origin, y growing
 *     downward, the baseline at 0 (only 'p' and 'y' go below it).  The advance is 7 pixels for every character.
 *     THIN RASTER RULE.  A pixel is painted by a stroke iff its distance to the closed segment is <= 1/2, in the integers of the
 *     raster rule above: v.d <= 0: iff X = P;  v.d >= L2: iff X = Q;  otherwise iff 4 (v x d)^2 <= L2.  A glyph therefore paints
 *     only pixels of its own 6 x 13 box, and a pixel belongs to at most one character of a line.
 *     COLOUR (100, 255, 0) as B, G, R, in the frame's channel order like the axes' colours.
 *     PAINT ORDER.  Heads in order; within a head the rectangle's sides, X, Y, Z, then the yaw, the pitch and the roll line: a later
 *     head's rectangle paints over an earlier head's text.
 * BGR -> 4:2:0, the inverse leg of the YUV ingest above.  ch = (h + 1) >> 1, cw = (w + 1) >> 1; the chroma sample (cy, cx) is
 * taken from the sums Rs, Gs, Bs over the four pixels (min(2 cy + dy, h - 1), min(2 cx + dx, w - 1)), dy, dx = 0, 1.  With int32
 * arithmetic and >> an arithmetic shift:
 *     Y = clip8(((RY * R  + GY * G  + BY * B  + (1 << 19)) >> 20) + yoff)
 *     U = clip8(((RU * Rs + GU * Gs + BU * Bs + (1 << 21)) >> 22) + 128)
 *     V = clip8(((RV * Rs + GV * Gs + BV * Bs + (1 << 21)) >> 22) + 128)
 * and {RY, GY, BY, RU, GU, BU, RV, GV, BV, yoff} = WHENET_BGR2YUV_COEFFS[matrix] = rint(2^20 x) of
 *     Kr sy, Kg sy, Kb sy | -Kr / (2 (1 - Kb)) sc, -Kg / (2 (1 - Kb)) sc, 0.5 sc | 0.5 sc, -Kg / (2 (1 - Kr)) sc, -Kb / (2 (1 - Kr)) sc
 * with (Kr, Kb) = (.299, .114) for BT.601 and JFIF, (.2126, .0722) for BT.709, Kg = 1 - Kr - Kb, and (sy, sc, yoff) =
 * (219/255, 224/255, 16) for video range, (1, 1, 0) for JFIF.  Plane layout and pitches are those of the ingest section.
 *
 * A destination is a whenet_surface_t: format WHENET_SURF_PACKED (plane[0] = rows of 3 w bytes in the frame's channel order),
 * WHENET_YUV_NV12 or WHENET_YUV_I420 (planes as whenet_yuv_frame_t, `matrix` read for these two only); every plane its own byte pitch
 * >= its row bytes; on_device = 1 for planes in the handle's device memory, 0 for host memory.  Only the rows' bytes are ever
 * written: pitch padding and whatever lies behind a plane belong to the caller.
 *   whenet_overlay_segments  pure host: window + angles -> the 16 ints above; *flags (may be NULL) = 1 rectangle | 2 axes
 *   whenet_annotate_host     the whole overlay as pure host arithmetic (no GPU): frame uint8 [frame_h][frame_w][3], rects [k][4],
 *                  valid [k] (may be NULL: all valid), ypr [k][3], k = 0..256 -> a host surface.  The statement the kernels are held to.
 *                  The text of an error is whenet_last_error(NULL)'s.
 *   whenet_op_annotate       the kernels alone, host to host, same arguments: the primitive table is built on the device from the
 *                  windows and angles (whenet_overlay_plan_kernel), one pass reads the frame and writes the surface
 *                  (whenet_overlay_draw_kernel).  Works on a whenet_create_postproc handle.  dst->on_device must be 0.
 * WHENET_EINVAL: a NULL argument or plane, a pitch below the row bytes, an unknown format / matrix / channel order, a side outside
 * 1..8192, k outside 0..256, a valid head's window outside -4096..8192.
 *   whenet_frame_annotate    the annotated frame of a ticket, from what its heads left on the device.  Call it after the ticket's
 *                  heads are enqueued (whenet_submit_frame, whenet_frame_heads, whenet_frame_detect_heads, whenet_clip_detect_heads)
 *                  and before its collect call; frame_index is 0 for a frame, 0..F-1 for a clip; at most one call per (ticket,
 *                  frame_index).  ENQUEUE-ONLY: the two kernels go on the engine's stream behind the forward; buffers are allocated
 *                  on the first call for a size.  The windows, valid flags and angles are those the ticket's collect call returns
 *                  (a clip's head without a forward row paints nothing); the channel order is the frame's (YUV ingest: BGR).
 *                  Host destination (on_device = 0): it travels through pinned staging and is complete when the ticket's collect
 *                  call returns; the pointers must stay valid until then.  Device destination (on_device = 1): the kernel writes
 *                  it in place.  ORDER, the ingest section's paragraph mirrored: with `stream` (the caller's hipStream_t) given,
 *                  the kernel waits for the work enqueued on `stream` BEFORE the call (the surface's previous reader) and `stream`
 *                  waits for the kernel's end, so work enqueued on it AFTER the call sees the annotated surface; the host never
 *                  waits.  With stream == NULL the surface is complete when the collect call returns.  The collect call's results
 *                  are bit for bit those of the same submission without an annotate.
 *                  WHENET_EINVAL, before anything is enqueued and with the handle usable and the ticket still collectable: an
 *                  unknown ticket; heads not yet enqueued; a ticket without a frame (whenet_submit_u8, a whenet_submit_frame with
 *                  k = 0 -- it uploads no frame -- or a released clip); a second call; a frame index outside the clip; more than
 *                  256 head slots per frame; a NULL plane, a pitch below the row bytes, an unknown format / matrix; a device plane
 *                  that fails the checks of the device ingest (memory type, device, extent inside its allocation); a host pointer
 *                  marked on_device, or device memory marked as host. */
#define WHENET_SURF_PACKED 2    /* beside WHENET_YUV_NV12 (0) and WHENET_YUV_I420 (1) */
#define WHENET_BGR2YUV_COEFFS {{269262, 528618, 102662, -155423, -305128, 460551, 460551, -385654, -74897, 16}, \
                               {191455, 644067, 65019, -105533, -355018, 460551, 460551, -418321, -42230, 16}, \
                               {313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262, 0}}
#define WHENET_DISPLAY_SIMPLE 0  /* demo_video.py --display simple: rectangle and axes */
#define WHENET_DISPLAY_FULL 1    /* ... full: and the three labels */
/* the font of the labels: the characters, and for each {n, then 8 rows of x0, y0, x1, y1 (the rows behind the n-th are 0)} */
#define WHENET_OVERLAY_GLYPHS "0123456789achiloprtwy: -."
#define WHENET_OVERLAY_FONT { \
    {8, 1,-8,3,-8, 3,-8,4,-7, 4,-7,4,-1, 4,-1,3,0, 3,0,1,0, 1,0,0,-1, 0,-1,0,-7, 0,-7,1,-8}, \
    {3, 1,-6,2,-8, 2,-8,2,0, 1,0,3,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0}, \
    {5, 0,-8,4,-8, 4,-8,4,-4, 4,-4,0,-4, 0,-4,0,0, 0,0,4,0, 0,0,0,0, 0,0,0,0, 0,0,0,0}, \
    {4, 0,-8,4,-8, 4,-8,4,0, 4,0,0,0, 1,-4,4,-4, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0}, \
    {3, 3,-8,0,-3, 0,-3,4,-3, 3,-8,3,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0}, \
    {5, 4,-8,0,-8, 0,-8,0,-4, 0,-4,4,-4, 4,-4,4,0, 4,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0}, \
    {5, 4,-8,0,-8, 0,-8,0,0, 0,0,4,0, 4,0,4,-4, 4,-4,0,-4, 0,0,0,0, 0,0,0,0, 0,0,0,0}, \
    {2, 0,-8,4,-8, 4,-8,1,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0}, \
    {5, 0,-8,4,-8, 4,-8,4,0, 4,0,0,0, 0,0,0,-8, 0,-4,4,-4, 0,0,0,0, 0,0,0,0, 0,0,0,0}, \
    {5, 4,-4,0,-4, 0,-4,0,-8, 0,-8,4,-8, 4,-8,4,0, 4,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0}, \
    {8, 4,-5,4,0, 1,-5,3,-5, 3,-5,4,-4, 4,-1,3,0, 3,0,1,0, 1,0,0,-1, 0,-1,0,-4, 0,-4,1,-5}, \
    {7, 1,-5,3,-5, 3,-5,4,-4, 4,-1,3,0, 3,0,1,0, 1,0,0,-1, 0,-1,0,-4, 0,-4,1,-5, 0,0,0,0}, \
    {5, 0,-8,0,0, 0,-4,1,-5, 1,-5,3,-5, 3,-5,4,-4, 4,-4,4,0, 0,0,0,0, 0,0,0,0, 0,0,0,0}, \
    {4, 1,-5,2,-5, 2,-5,2,0, 1,0,3,0, 2,-7,2,-7, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0}, \
    {2, 2,-8,2,-1, 2,-1,3,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0}, \
    {8, 1,-5,3,-5, 3,-5,4,-4, 4,-4,4,-1, 4,-1,3,0, 3,0,1,0, 1,0,0,-1, 0,-1,0,-4, 0,-4,1,-5}, \
    {8, 0,-5,0,3, 1,-5,3,-5, 3,-5,4,-4, 4,-4,4,-1, 4,-1,3,0, 3,0,1,0, 1,0,0,-1, 0,-4,1,-5}, \
    {3, 0,-5,0,0, 0,-3,2,-5, 2,-5,4,-5, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0}, \
    {4, 2,-8,2,-1, 2,-1,3,0, 3,0,4,0, 0,-5,4,-5, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0}, \
    {4, 0,-5,1,0, 1,0,2,-3, 2,-3,3,0, 3,0,4,-5, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0}, \
    {3, 0,-5,2,0, 4,-5,1,3, 1,3,0,3, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0}, \
    {2, 2,-5,2,-4, 2,-1,2,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0}, \
    {0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0}, \
    {1, 0,-4,4,-4, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0}, \
    {2, 2,-1,2,0, 3,-1,3,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0, 0,0,0,0}}
typedef struct {
    void* plane[3];
    int pitch[3];
    int format;
    int matrix;
    int on_device;
} whenet_surface_t;
WHENET_API int whenet_overlay_segments(const int32_t rect[4], float yaw, float pitch, float roll, int32_t segments[16], int32_t* flags);
WHENET_API int whenet_annotate_host(const uint8_t* frame, int frame_h, int frame_w, int channel_order, const int32_t* rects,
                         const int32_t* valid, const float* ypr, int k, const whenet_surface_t* dst);
WHENET_API int whenet_op_annotate(whenet_t* h, const uint8_t* frame, int frame_h, int frame_w, int channel_order, const int32_t* rects,
                       const int32_t* valid, const float* ypr, int k, const whenet_surface_t* dst);
WHENET_API int whenet_frame_annotate(whenet_t* h, int ticket, int frame_index, const whenet_surface_t* dst, void* stream);
/* The labels (additions to ABI 6).
 *   whenet_overlay_labels    pure host: window + float32 angles -> the three NUL-terminated texts, their origins (x, y) and *flags
 *                  (may be NULL) = what the head paints: 1 rectangle | 2 axes | 4 labels.  Without the 4 the texts are empty.
 *   whenet_overlay_glyph     pure host: the strokes of character `ch` as rows of x0, y0, x1, y1; returns their number 0..8, or
 *                  WHENET_EINVAL for a character outside WHENET_OVERLAY_GLYPHS or a NULL pointer.
 *   whenet_annotate_host_ex, whenet_op_annotate_ex, whenet_frame_annotate_ex: the three calls above with `display` =
 *                  WHENET_DISPLAY_SIMPLE (their bytes, their cost) or WHENET_DISPLAY_FULL; any other value is WHENET_EINVAL.  The
 *                  calls without _ex are these with WHENET_DISPLAY_SIMPLE. */
WHENET_API int whenet_overlay_labels(const int32_t rect[4], float yaw, float pitch, float roll, char text[3][16], int32_t origin[3][2],
                          int32_t* flags);
WHENET_API int whenet_overlay_glyph(int ch, int32_t segs[8][4]);
WHENET_API int whenet_annotate_host_ex(const uint8_t* frame, int frame_h, int frame_w, int channel_order, const int32_t* rects,
                            const int32_t* valid, const float* ypr, int k, const whenet_surface_t* dst, int display);
WHENET_API int whenet_op_annotate_ex(whenet_t* h, const uint8_t* frame, int frame_h, int frame_w, int channel_order, const int32_t* rects,
                          const int32_t* valid, const float* ypr, int k, const whenet_surface_t* dst, int display);
WHENET_API int whenet_frame_annotate_ex(whenet_t* h, int ticket, int frame_index, const whenet_surface_t* dst, void* stream, int display);

/* ---- JPEG ENCODER: a frame in, a baseline JPEG stream out (additions to ABI 6).  demo_video.py:46-47, :60 store the annotated frame
 * as Motion-JPEG; the overlay already leaves a JFIF-matrix 4:2:0 surface in device memory, which is a baseline encoder's input
 * (csrc/jpeg.hip; the arithmetic is csrc/jpeg_host.h's).  Integers only.  The Annex K tables and the zigzag order are the JPEG
 * standard's (ITU-T T.81), written out as data in csrc/jpeg_host.h.
 * FORMAT.  Baseline sequential DCT, 8 bit, three components, 4:2:0: Y id 1, 2x2 sampling, quantiser 0, Huffman tables 0; Cb id 2 and
 * Cr id 3, 1x1, quantiser 1, Huffman tables 1.  The stream, in this order: SOI; APP0 "JFIF\0" version 1.01, units 0, density 1:1,
 * no thumbnail; two DQT segments (8 bit, zigzag order, table 0 then table 1); SOF0; four DHT segments (DC0, AC0, DC1, AC1: Annex K's
 * "typical" tables); DRI with the interval ceil(w / 16), ONE RESTART INTERVAL PER MCU ROW; SOS (Ss 0, Se 63, Ah/Al 0); the
 * entropy-coded data; EOI.  The header (SOI..SOS) has WHENET_JPEG_HEADER_BYTES = 629 bytes and depends on (h, w, quality) only.
 * SOURCE.  A whenet_surface_t of h x w pixels, sides 1..8192: WHENET_YUV_I420 or WHENET_YUV_NV12 with matrix WHENET_YUV_JFIF (any
 * other matrix is WHENET_EINVAL: JFIF is full-range BT.601), or WHENET_SURF_PACKED with a channel order, whose planes are BY
 * DEFINITION those of "BGR -> 4:2:0" above with the JFIF row: encoding a packed frame equals, bit for bit, encoding the I420
 * surface whenet_annotate_host writes from it.
 * MCU.  16 x 16 luma pixels, blocks in the order Y00, Y01, Y10, Y11, Cb, Cr.  A sample beyond the right or bottom edge of its plane
 * (h x w luma, ceil(h/2) x ceil(w/2) chroma) is the last column's or row's.
 * FORWARD DCT.  T[u][x] = rint(4096 s(u) cos((2x+1) u pi / 16)), s(0) = sqrt(1/8), s(u>0) = 1/2: WHENET_JPEG_DCT below.  With
 * p = sample - 128, int32 arithmetic and >> an arithmetic shift:
 *     a[y][u] = sum_x T[u][x] p[y][x]        r[y][u] = (a[y][u] + 256) >> 9
 *     b[v][u] = sum_y T[v][y] r[y][u]        (the coefficient scaled by 2^15; |b| < 2^25)
 * QUANTISER.  Annex K's luminance and chrominance tables scaled the IJG way: scale = 5000 / quality (integer division) for quality
 * < 50, else 200 - 2 quality; Q = clamp((base scale + 50) / 100, 1, 255); quality 1..100.
 *     k = sign(b) ((|b| + (Q << 14)) / (Q << 15))     (integer division: rounds half away from zero)
 * AC coefficients are clamped to +-1023; DC needs no clamp.
 * ENTROPY CODING.  Huffman coding of the DC differences (category + extra bits) and of the (run, size) AC symbols with ZRL and EOB;
 * no EOB when coefficient 63 is non-zero.  The DC predictors are 0 at the start of every restart interval.  The last byte of an
 * interval is padded with 1-bits; behind every interval but the last stands RSTm, m = interval index mod 8.  Inside the entropy
 * data every 0xFF byte is followed by 0x00.
 *   whenet_jpeg_header  pure host: the header bytes into out (cap >= WHENET_JPEG_HEADER_BYTES) and the two quantiser tables in
 *                  NATURAL order into qtables (either may be NULL); returns the header's length, or WHENET_EINVAL
 *   whenet_jpeg_bound   pure host: a capacity no stream of an h x w frame exceeds (WHENET_EINVAL for a side outside 1..8192).  A block
 *                  is at most 11 + 11 bits of DC and 63 x (16 + 10) bits of AC = 1660 bits; an interval of B = 6 ceil(w / 16)
 *                  blocks at most U = ceil(1660 B / 8) bytes, 2 U when every byte is stuffed, and 2 more for its RSTm or EOI:
 *                  bound = 629 + ceil(h / 16) (2 U + 2).
 *   whenet_jpeg_encode_host  the whole encoder as pure host arithmetic (no GPU): the statement the kernels are held to.  *size is
 *                  always the stream's full length; when it exceeds cap, nothing beyond out[cap - 1] is written and the call
 *                  returns WHENET_EOVERFLOW.  src->on_device must be 0; channel_order is read for WHENET_SURF_PACKED only.
 *   whenet_op_jpeg_encode    the kernels alone, host to host, same arguments and results.  Works on a whenet_create_postproc handle.
 *   whenet_jpeg_encode_device  source planes, dst (cap bytes) and dsize (one int64: the full length, also on overflow) in the
 *                  handle's device memory, ENQUEUE-ONLY on the engine's stream and ordered against `stream` by events as the
 *                  ingest section's ORDER paragraph states; the device-pointer checks of the device ingest apply to every
 *                  plane, to dst and to dsize; cap <= 2^31 - 1.  A stream that does not fit leaves dst's bytes from cap on untouched.
   whenet_frame_annotate_jpeg  the annotated frame of a ticket as a JPEG stream: what whenet_frame_annotate_ex does, into an I420
 *                  JFIF surface in device memory that the engine owns (allocated on the first call for a size), and the encoder
 *                  behind it on the engine's stream.  ENQUEUE-ONLY.  The stream's length is known on the device only and the call
 *                  must not wait: the encoder lands the stream in device memory and one more kernel copies min(length, cap) bytes
 *                  and the length into pinned host memory that the device addresses -- the compressed bytes are all that crosses
 *                  the link.  out[0 .. min(*size, cap)), *size (always the full length) and *status (WHENET_OK or WHENET_EOVERFLOW)
 *                  are complete when the ticket's collect call returns; the pointers must stay valid until then.  Call order and
 *                  WHENET_EINVAL cases as whenet_frame_annotate (and a quality outside 1..100); it counts as the (ticket,
 *                  frame_index)'s one annotate call; the collect call's own results are bit for bit those of the same submission
 *                  without it.
 * WHENET_EINVAL: a NULL argument or plane, a pitch below the row bytes, an unknown format / channel order, a YUV source whose
 * matrix is not WHENET_YUV_JFIF, a side outside 1..8192, quality outside 1..100, cap < 0.
 * SAMPLING AND OPTIMISED TABLES (the _ex calls; additions to ABI 6).  Each _ex call is the call of the same name with two more
 * arguments; sampling = WHENET_JPEG_420 and optimize = 0 give that call's bytes.
 * SAMPLING.  WHENET_JPEG_420 (above), WHENET_JPEG_422 (H2V1) or WHENET_JPEG_444; any other value is WHENET_EINVAL.  The luma sampling
 * factors hs x vs are 2x2, 2x1, 1x1; the MCU is 8 hs x 8 vs luma pixels: hs vs luma blocks in row order, then Cb, then Cr (Y0 Y1 Cb
 * Cr at 4:2:2, Y Cb Cr at 4:4:4).  One restart interval per MCU row of that sampling: ceil(h / 8 vs) intervals, DRI = ceil(w / 8 hs).
 * The SOF0 sampling byte of Y (0x22, 0x21, 0x11) and the DRI value are the only header bytes that differ.  The chroma planes are
 * ceil(h / vs) x ceil(w / hs).  A chroma sample of packed pixels keeps the one rule of "BGR -> 4:2:0": overlay_cb / overlay_cr of
 * R, G, B SUMS WORTH FOUR PIXELS -- 4:4:4 passes 4 x the pixel, 4:2:2 passes 2 x the sum of the two horizontal neighbours (the
 * right edge replicated): Cb = clamp(((RU r + GU g + BU b + 2^21) >> 22) + 128) of those sums, which for 4:4:4 is
 * ((RU R + GU G + BU B + 2^19) >> 20) + 128 of the pixel.  NV12 / I420 sources carry 4:2:0 chroma: with another sampling they are
 * WHENET_EINVAL.
 * OPTIMISED TABLES.  optimize != 0: the four Huffman tables are built from the frame's own symbols.  The histograms count, per
 * table (DC0, AC0, DC1, AC1), the DC categories and the (run, size) / ZRL / EOB symbols exactly as the entropy coder emits them.
 * A table follows T.81 K.2 (figures K.1 - K.4): a 257th symbol of frequency 1 is added (so no code is all ones); the two trees of
 * least non-zero frequency are merged until one is left, ties broken towards the LARGER symbol value, as libjpeg's
 * jpeg_gen_optimal_table does; code lengths above 16 are shortened by figure K.3; the reserved symbol is removed from the longest
 * length; the symbols are listed by code size, then by value.  The DHT segments list the occurring symbols only, so the header
 * SOI..SOS is shorter than WHENET_JPEG_HEADER_BYTES (at most 12 + 162 symbols occur per table pair: never longer).  The pixels of
 * the decoded stream are those of the standard tables' stream.
 * BOUND.  With B_s = (hs vs + 2) ceil(w / 8 hs) blocks per interval: bound = 629 + ceil(h / 8 vs) (2 ceil(1660 B_s / 8) + 2); it does
 * not depend on optimize.
 *   whenet_jpeg_optimal_table  pure host: freq[256] -> bits[16] (the codes of each length 1..16), vals (the symbols in code order)
 *                  and *count (their number).  WHENET_EINVAL for a NULL pointer or when no frequency is non-zero.
 *   whenet_jpeg_header_ex, whenet_jpeg_bound_ex   the standard-table header and the bound of a sampling.
 *   whenet_jpeg_encode_host_ex, whenet_op_jpeg_encode_ex   hist (may be NULL) receives the four histograms when optimize != 0.
 *   whenet_jpeg_encode_device_ex   as whenet_jpeg_encode_device: ENQUEUE-ONLY also with optimize (the histogram and table kernels
 *                  run between the DCT and the pack kernel on the engine's stream; the tables, the header and its length are
 *                  the encode's own device memory).
 *   whenet_frame_annotate_jpeg_ex  at WHENET_JPEG_422 / 444 the overlay goes into a PACKED surface the engine owns, in the frame's
 *                  channel order, and the encoder reads that: the stream is whenet_jpeg_encode_host_ex of whenet_annotate_host_ex's
 *                  packed frame.  At WHENET_JPEG_420 the I420 surface above. */
#define WHENET_JPEG_420 0
#define WHENET_JPEG_422 1
#define WHENET_JPEG_444 2
#define WHENET_EOVERFLOW (-75)  /* the result does not fit the caller's capacity; the needed size is reported */
#define WHENET_JPEG_HEADER_BYTES 629
#define WHENET_JPEG_DEFAULT_QUALITY 95
#define WHENET_JPEG_DCT {{1448, 1448, 1448, 1448, 1448, 1448, 1448, 1448}, {2009, 1703, 1138, 400, -400, -1138, -1703, -2009}, \
                         {1892, 784, -784, -1892, -1892, -784, 784, 1892}, {1703, -400, -2009, -1138, 1138, 2009, 400, -1703}, \
                         {1448, -1448, -1448, 1448, 1448, -1448, -1448, 1448}, {1138, -2009, 400, 1703, -1703, -400, 2009, -1138}, \
                         {784, -1892, 1892, -784, -784, 1892, -1892, 784}, {400, -1138, 1703, -2009, 2009, -1703, 1138, -400}}
WHENET_API int whenet_jpeg_header(int h, int w, int quality, uint8_t* out, int cap, int32_t qtables[2][64]);
WHENET_API int64_t whenet_jpeg_bound(int h, int w);
WHENET_API int whenet_jpeg_encode_host(const whenet_surface_t* src, int h, int w, int channel_order, int quality, uint8_t* out, int64_t cap,
                            int64_t* size);
WHENET_API int whenet_op_jpeg_encode(whenet_t* h, const whenet_surface_t* src, int hh, int ww, int channel_order, int quality, uint8_t* out,
                          int64_t cap, int64_t* size);
WHENET_API int whenet_jpeg_encode_device(whenet_t* h, const whenet_surface_t* src, int hh, int ww, int channel_order, int quality, void* dst,
                              int64_t cap, int64_t* dsize, void* stream);
WHENET_API int whenet_frame_annotate_jpeg(whenet_t* h, int ticket, int frame_index, int display, int quality, uint8_t* out, int64_t cap,
                               int64_t* size, int32_t* status);
WHENET_API int whenet_jpeg_optimal_table(const uint32_t freq[256], uint8_t bits[16], uint8_t vals[256], int* count);
WHENET_API int whenet_jpeg_header_ex(int h, int w, int quality, int sampling, uint8_t* out, int cap, int32_t qtables[2][64]);
WHENET_API int64_t whenet_jpeg_bound_ex(int h, int w, int sampling);
WHENET_API int whenet_jpeg_encode_host_ex(const whenet_surface_t* src, int h, int w, int channel_order, int quality, int sampling, int optimize,
                               uint8_t* out, int64_t cap, int64_t* size, uint32_t hist[4][256]);
WHENET_API int whenet_op_jpeg_encode_ex(whenet_t* h, const whenet_surface_t* src, int hh, int ww, int channel_order, int quality, int sampling,
                             int optimize, uint8_t* out, int64_t cap, int64_t* size, uint32_t hist[4][256]);
WHENET_API int whenet_jpeg_encode_device_ex(whenet_t* h, const whenet_surface_t* src, int hh, int ww, int channel_order, int quality,
                                 int sampling, int optimize, void* dst, int64_t cap, int64_t* dsize, void* stream);
WHENET_API int whenet_frame_annotate_jpeg_ex(whenet_t* h, int ticket, int frame_index, int display, int quality, int sampling, int optimize,
                                  uint8_t* out, int64_t cap, int64_t* size, int32_t* status);

/* ---- JPEG DECODER: a JPEG still or an MJPG frame in, the resident frame out (additions to ABI 6).  demo.py starts with `cv2.imread`
 * of a JPEG, demo_video.py:49-53 with `cap.read()` -- for a camera or an MJPG file a Motion-JPEG decode.  Here the compressed bytes
 * are what crosses the link; the kernels of csrc/jpeg_dec.hip decode them (the arithmetic is csrc/jpeg_dec_host.h's).  Integers only.
 * ACCEPTED.  Baseline sequential DCT (SOF0), 8 bit, one interleaved scan, Huffman coding.  Three components are Y, Cb, Cr (JFIF) with
 * luma sampling 2x2 (4:2:0), 2x1 (4:2:2) or 1x1 (4:4:4) and chroma sampling 1x1; one component is grey.  8-bit DQT with ids 0..3 and
 * DHT with ids 0..1 per class, several tables per segment allowed; any DRI or none; APPn and COM are skipped; sides 1..8192; streams
 * below 2^31 bytes.  (SOF1, several scans and three more samplings: LAYOUTS below, opt-in.)  Everything else -- SOF1, SOF2 and later frame types, arithmetic coding, 12 bit, 4 components, a scan that does
 * not hold every component, 16-bit DQT, other sampling factors (LAYOUTS below: opt-in), a missing table, a header that ends early -- is WHENET_EFORMAT from
 * the host parser with the reason in whenet_last_error (NULL handle for the pure-host calls), before anything is enqueued.
 * PARSE.  SOI .. SOS into a whenet_jpeg_info_t: size, components, the luma sampling factors hs, vs (1 or 2), per component the
 * quantiser id qt and the Huffman ids dc, ac; restart_interval Ri in MCUs (0: none); intervals = ceil(MCUs / Ri), 1 without DRI;
 * data_offset of the entropy data; the quantisers q in NATURAL order; the Huffman tables at index 2 id + class (DC0, AC0, DC1, AC1) as
 * counts[16] and values.  The struct is self-contained: a decode needs it and the bytes from data_offset on only.
 * An MCU is 8 hs x 8 vs luma samples: hs vs luma blocks in row order, then Cb, then Cr (grey: one block, 8 x 8).
 * INTERVALS.  The restart markers are the pairs 0xFF 0xD0..0xD7 of the entropy data, in order.  Interval 0 begins at the data's
 * first byte, interval k + 1 behind marker k.  Marker k must be RST(k mod 8) and there must be intervals - 1 markers: the first k
 * whose marker has another number, or intervals - 1 if there are more, or the number of markers if there are fewer, is a bad
 * interval; it is still decoded from its start, the intervals behind it are not (their coefficients are zero).
 * ENTROPY DECODE.  T.81 F.2 Huffman decoding, the DC predictors 0 at the start of every interval and kept inside -32768..32767.
 * 0xFF 0x00 yields one 0xFF data byte; at any other byte pair that begins with 0xFF, and at the end of the data, the interval's
 * bits end.  An AC symbol (r, s): s > 0 skips r coefficients and reads one; (15, 0) skips 16; any other (r, 0) ends the block.
 * Coefficient k is clamp(value x Q[k], -2048, 2047) in natural order: every legitimate coefficient of an 8-bit image lies inside,
 * the clamp keeps every stream inside the int32 arithmetic below.
 * DAMAGE.  A code that is no code word, a run that passes coefficient 63, bits that end inside a symbol: the block in hand keeps
 * what was decoded of it, the remaining blocks of the interval are zero coefficients (DC included), and the interval is bad.
 * Nothing faults and nothing is read or written outside its buffer.  status[0] = WHENET_OK, or WHENET_EFORMAT with status[1] = the
 * first bad interval (else -1); the output is fully defined either way and the kernels' equals the host statement's byte for byte.
 * INVERSE DCT.  T = WHENET_JPEG_DCT, c = a block's coefficients [v][u], int32 arithmetic, >> an arithmetic shift:
 *     a[y][u] = sum_v T[v][y] c[v][u]        r[y][u] = (a[y][u] + 128) >> 8
 *     b[y][x] = sum_u T[u][x] r[y][u]        sample  = clamp(((b[y][x] + 32768) >> 16) + 128, 0, 255)
 * The columns of |T| sum to at most 10,822, so |a| < 2.3e7, |r| < 8.7e4, |b| < 9.5e8.  Within 1 level of the rounded float64
 * inverse DCT (about 2 % of the samples differ from it by one).
 * PLANES.  The luma plane is h x w samples, the chroma planes ceil(h / vs) x ceil(w / hs); blocks beyond those edges are decoded
 * and their samples dropped.
 * FRAME.  WHENET_SURF_PACKED: pixel (x, y) takes the chroma sample (x >> (hs - 1), y >> (vs - 1)) and the JFIF row of the YUV
 * ingest's conversion; channel_order says where R and B go; grey gives B = G = R = Y.  For a 4:2:0 stream this is bit for bit
 * whenet_yuv_to_bgr_host of the decoded I420 planes.  A 4:2:0 stream also decodes into a WHENET_YUV_I420 or WHENET_YUV_NV12 surface
 * whose matrix is WHENET_YUV_JFIF (other samplings, another matrix: WHENET_EINVAL).  This is RULE 0, the default.  It differs from
 * libjpeg's bytes (nearest-neighbour chroma against a triangle filter, another inverse DCT, another YCbCr row); rule 1 below does not.
 *   whenet_jpeg_parse        pure host: the stream's header into *info
 *   whenet_jpeg_decode_host  the whole decoder as pure host arithmetic (no GPU): the statement the kernels are held to.  dst: a
 *                  host surface (on_device = 0) of the stream's size; channel_order is read for WHENET_SURF_PACKED only
 *   whenet_jpeg_decode_planes_host  the same up to the component planes: plane[c] = rows of the component's width, pitch[c] bytes
 *                  apart (>= the width), c < components
 *   whenet_op_jpeg_decode    the kernels alone, host to host, same arguments and results.  Works on a whenet_create_postproc handle.
 *   whenet_jpeg_decode_device  info (host memory, from whenet_jpeg_parse of the header bytes), d_entropy = the nbytes bytes of the
 *                  stream from data_offset on, dst (on_device = 1) and d_status (two int32) in the handle's device memory.
 *                  ENQUEUE-ONLY on the engine's stream and ordered against `stream` as the ingest section's ORDER paragraph states
 *                  -- with two exceptions in which the host WAITS for the engine's stream first: a call whose stream needs larger
 *                  work buffers than any call before it, and a call whose quantisers or Huffman tables differ from the previous
 *                  call's (then followed by one blocking copy of the 6 KB of decode tables).  The first call always waits; the
 *                  frames of one MJPG stream, which repeat their tables and their size, do not;
 *                  the device-pointer checks of the device ingest apply to d_entropy, every plane and d_status.  The stream
 *                  whenet_jpeg_encode_device left in device memory decodes this way with whenet_jpeg_header's bytes parsed on the
 *                  host; where the stream's length is known on the device only, nbytes may be the capacity of a buffer that was
 *                  zero-filled before the encode: bytes behind EOI are scanned for restart markers like the rest, zeros hold none.
 *   whenet_frame_begin_jpeg  stands for cv2.imread / cap.read(): parses on the host (a refused stream takes no slot), copies only
 *                  the compressed bytes into pinned staging, one asynchronous H2D, and the decode kernels on the copy stream into the
 *                  slot's frame buffer, before the event every consumer waits for -- where csrc/yuv.hip runs for
 *                  whenet_frame_begin_yuv.  The ticket then behaves as whenet_frame_begin's with the same channel_order.  status[0..1]
 *                  are complete when the ticket's collect call returns; the pointer must stay valid until then.  Damaged data still
 *                  gives a ticket and a fully defined frame.
 * ENTROPY FORMS.  The entropy stage has two forms with the same output, bit for bit, damaged streams included.  Form 0 runs one
 * restart interval per lane: a stream without DRI is ONE interval, one lane walking the whole picture, correct and serial.  Form 1,
 * the SEGMENTED form (csrc/jpeg_dec_seg.hip, the arithmetic is csrc/jpeg_dec_seg_host.h's), decodes every interval with many lanes
 * by the self-synchronisation of Huffman streams.  The bytes of interval i (from its start to the next restart marker or the end of
 * the data) are cut into segments of seg_bytes, a power of two in 4..4096, numbered flat over the decoded intervals; the host bounds
 * their number by ceil(nbytes / seg_bytes) + intervals and sizes every launch from that, nothing waits for the device.  A SYNC STATE
 * is what a decoder needs between two code words: the raw byte and the bit offset of the next unread bit, the block's index in its
 * MCU and the zigzag index, or DEAD (damage met, or the interval's bits have ended); equal states continue alike.  SYNC: a window of
 * WHENET_JPEG_SEG_WINDOW consecutive segments is one workgroup's; an interval's first segment starts from its true state, every
 * other one from a guess (its first byte -- behind the 0x00 of a stuffed pair that began in the segment before -- block 0, a DC
 * symbol next); in round 0 lane j walks its segment to the first code-word boundary at or behind its end and stores the exit state,
 * in round r it walks segment j + r from its running state and either meets the stored exit state there (done) or replaces it,
 * stores behind a barrier, chains never cross an interval start, at most `window` rounds.  STITCH: one lane per interval carries the
 * true state over each window boundary inside it until it meets a stored state.  COUNT: a block belongs to the segment in which its
 * DC code word begins; from its true entry state a lane counts its blocks and composes their DC differences per component as maps
 * x -> min(max(x + a, L), H), which compose associatively where a sum of differences under the -32768..32767 clamp does not; an
 * exclusive scan over an interval's segments gives every segment its first block's index and its three predictors.  WRITE: a lane
 * decodes the blocks it owns, the tail in later segments included, by the block decode of form 0, and stops at the interval's block
 * count (bytes behind are padding); damage lowers the first bad interval exactly as DAMAGE states, and every later segment starts
 * DEAD and writes nothing.  The marker scan, the inverse DCT and the frame kernels are those of form 0.
 *   option "jpeg_entropy"    0: form 0; 1: form 1; 2: auto -- form 1 where nbytes / intervals >= 4096 bytes (default, see
 *                  docs/experiments.md section 32).  Read by whenet_op_jpeg_decode, whenet_jpeg_decode_device, whenet_frame_begin_jpeg.
 *   option "jpeg_seg_bytes"  seg_bytes of form 1, a power of two in 4..4096, default 128
 *   option "jpeg_seg_lanes"  a measurement knob: decoding lanes per 64-lane wave of form 1's sync, count and write kernels, 16, 32
 *                  or 64 (0: the default, 32); the output does not depend on it
 *   whenet_jpeg_decode_segmented_host  whenet_jpeg_decode_host with the entropy stage run as the host emulation of form 1 (lanes in
 *                  a plain loop), window in 1..1024.  stats (may be NULL): [0] intervals decoded, [1] segments, [2] windows, [3] the
 *                  largest number of sync rounds in a window, [4] segments walked by the stitch, [5] the largest number of bytes a
 *                  lane fetched during sync, [6] seg_bytes, [7] the form that ran (0 or 1)
 *   whenet_jpeg_decode_segmented_planes_host  the same up to the component planes, as whenet_jpeg_decode_planes_host
 *   whenet_op_jpeg_decode_ex  whenet_op_jpeg_decode with the form forced (entropy 0 or 1; seg_bytes is read for 1); stats as above,
 *                  read back from the device (form 0: [0] and [7] only)
 *   whenet_jpeg_decode_counters  out = {decodes launched in form 0, in form 1, 0, 0} over the engines of the handle (host-side counts)
 *   whenet_jpeg_seg_dc_scan_host  the saturating scan alone: pred[i] = the predictor behind difference i, by maps over chunks
 * Measured on one MI355X (docs/experiments.md section 32): a 1080p stream without DRI decodes in 15.7 ms in form 1 against 1.03 s in
 * form 0, one with 68 intervals in 5.2-6.6 ms against 32 ms; a host decoder on one core takes 8.6 ms, and is still faster at 480p.
 * CLIPS OF JPEG STREAMS (four entry points, 101 in all, ABI still 6).  Up to 16 streams per submission, as whenet_clip_begin and
 * its kin take up to 16 frames.  Frame f is exactly what whenet_frame_begin_jpeg(data[f]) makes: the same frame bytes, the same two
 * status words.  Every stream keeps its own size, sampling, tables and DRI, and gets its own entropy form: "jpeg_entropy" and
 * "jpeg_seg_bytes" are applied stream by stream, so under auto a clip may hold streams of both forms.  A damaged stream gives its own
 * defined frame and status and leaves every other frame untouched.  Records, decode tables and entropy bytes of all frames travel
 * as ONE H2D; every stage runs for all frames in one launch (one memset in front), so the number of enqueues depends on the forms
 * and colour paths that occur in the clip, never on the frame count.
 *   whenet_clip_begin_jpeg   ENQUEUE-ONLY.  The slot ends up as whenet_clip_begin leaves it where every frame has one size, else as
 *                  whenet_clip_begin_mixed leaves it (frames back to back, unaligned; at most option letterbox_cache frames);
 *                  whenet_clip_detect_heads, the annotate calls and whenet_collect_clip then work unchanged.  status: int32
 *                  [num_frames][2], complete when the ticket's collect call returns; the pointer must stay valid until then.
 *                  Refusals come before a slot is taken and name the frame: num_frames outside 1..16, a NULL pointer or a size
 *                  < 1 (WHENET_EINVAL), a stream the parser refuses (WHENET_EFORMAT: one refused stream refuses the whole call).
 *   whenet_op_jpeg_decode_clip  the clip kernels alone, host to host: frame f into dst[f] (host surfaces at the caller's pitches;
 *                  packed, or I420 / NV12 for a 4:2:0 stream), status [num_frames][2].  entropy -1: the handle's options; 0 / 1
 *                  and seg_bytes as in whenet_op_jpeg_decode_ex.  Works on a whenet_create_postproc handle.
 *   whenet_jpeg_clip_plan    pure host, no GPU: the layout the engine uses.  infos: the parsed headers, nbytes[f]: the length of
 *                  frame f's entropy data (size - data_offset), entropy 0, 1 or 2 (auto), seg_bytes a power of two in 4..4096.
 *                  out: num_frames * WHENET_JPEG_CLIP_PLAN_FRAME_WORDS + WHENET_JPEG_CLIP_PLAN_TOTAL_WORDS int64.  Per frame:
 *                  [0] the form, [1] seg_bytes (0 in form 0), [2] seg_cap (0 in form 0), [3] 0, then (offset, length) in bytes of
 *                  tables, data, start, meta, seg_stats, coef, plane 0, 1, 2, first_seg, seg_exit, seg_count, seg_blk ([4]..[29];
 *                  length 0: the frame has no such region), [30..31] 0.  Behind the last frame: [0..1] offset and length of the
 *                  argument records, [2] the bytes of the upload block (records | per frame tables | data, from offset 0),
 *                  [3..4] offset and length of the zeroed bytes (every frame's start | meta | seg_stats, then every frame's
 *                  coef), [5] the bytes of the whole buffer, [6] frames of form 0, [7] frames of form 1.  Every region starts at a
 *                  multiple of 256, but seg_stats, which lies 64 bytes behind meta.
 *   whenet_jpeg_clip_counters  out = {clip decodes enqueued, frames in them, kernel launches plus memsets enqueued for them, H2D
 *                  copies enqueued for them} over the engines of the handle (host-side counts).  A clip decode also counts each of
 *                  its frames into whenet_jpeg_decode_counters' form-0 or form-1 word.
 * JPEG DECODER, RULE 1 (six entry points, 107 in all, ABI still 6).  A second rule for the inverse DCT, the chroma upsampling and
 * the colour row, chosen per handle (option "jpeg_rule") and per call: a packed frame whose bytes are those of a libjpeg-turbo
 * decode with its defaults (JDCT_ISLOW, fancy upsampling, YCC to RGB) -- what cv2.imread and cap.read() hand the reference's first
 * line.  Rule 0 above stays the default and none of its bytes change.  ACCEPTED, PARSE, INTERVALS, ENTROPY DECODE (both forms), the
 * coefficient records clamp(value x Q, -2048, 2047) and DAMAGE with its status words are shared and the same under both rules.
 * Integer arithmetic, >> an arithmetic shift.
 * INVERSE DCT (jidctint.c: 13 constant bits, 2 pass-1 bits).  One 8-point pass on inputs i0..i7:
 *     z1 = (i2+i6) 4433      t2 = z1 - i6 15137     t3 = z1 + i2 6270      t0 = (i0+i4) << 13     t1 = (i0-i4) << 13
 *     t10 = t0+t3            t13 = t0-t3            t11 = t1+t2            t12 = t1-t2
 *     a0 = i7   a1 = i5   a2 = i3   a3 = i1         z1 = a0+a3   z2 = a1+a2   z3 = a0+a2   z4 = a1+a3   z5 = (z3+z4) 9633
 *     a0 *= 2446             a1 *= 16819            a2 *= 25172            a3 *= 12299
 *     z1 *= -7373            z2 *= -20995           z3 = z3 (-16069) + z5  z4 = z4 (-3196) + z5
 *     a0 += z1+z3            a1 += z2+z4            a2 += z2+z3            a3 += z1+z4
 *     outputs 0..7 = t10+a3, t11+a2, t12+a1, t13+a0, t13-a0, t12-a1, t11-a2, t10-a3, each descaled as (x + 2^(s-1)) >> s
 * Pass 1 runs down the columns with s = 11, pass 2 along the rows of its results with s = 18; sample = clamp(result + 128, 0, 255).
 * (libjpeg's shortcuts for all-zero AC columns and rows give the same values.)  A pass is exact and linear, out[k] = sum_j C[j][k]
 * i[j], and the columns of |C| sum to at most 61,214.  With |coefficient| <= 2048 pass 1 stays below 1.26e8 (every intermediate
 * below 3.5e8): int32.  Its results reach 61,214, so pass 2 reaches 61,214^2 = 3.75e9, above 2^31: pass 2 is int64, on the host
 * and in the kernel, for every clamped coefficient block, damaged ones included.
 * CHROMA (jdsample.c, fancy).  The chroma planes are ch = ceil(h / vs) rows of cw = ceil(w / hs) samples; rows >= ch and columns
 * >= cw of the padded working planes never enter a result: neighbour indices are clamped to 0..ch-1 and 0..cw-1.  4:4:4 and grey:
 * nothing to do.  4:2:2 with cw > 2: out[2i] = (3 in[i] + in[i-1] + 1) >> 2, out[2i+1] = (3 in[i] + in[i+1] + 2) >> 2.  4:2:0 with
 * cw > 2: output row 2r uses s[i] = 3 in[r][i] + in[r-1][i], row 2r+1 uses 3 in[r][i] + in[r+1][i]; then out[2i] = (3 s[i] + s[i-1]
 * + 8) >> 4, out[2i+1] = (3 s[i] + s[i+1] + 7) >> 4.  cw <= 2, either sampling: replication, in[y >> (vs-1)][x >> (hs-1)], with no
 * vertical filter either (libjpeg's own switch).  The output is cropped to h x w.
 * COLOUR (jdcolor.c).  d = Cb - 128, e = Cr - 128, F(x) = int(x 65536 + 0.5), clamp to 0..255:
 *     R = clamp(Y + ((F(1.402) e + 32768) >> 16))        B = clamp(Y + ((F(1.772) d + 32768) >> 16))
 *     G = clamp(Y + ((-F(0.34414) d + 32768 - F(0.71414) e) >> 16))
 * Grey gives R = G = B = Y; channel_order places R and B as under rule 0.
 * SCOPE.  Rule 1 equals libjpeg's bytes wherever no dequantised coefficient is touched by the +-2048 clamp -- every stream an
 * encoder makes from 8-bit samples; libjpeg's range-limit table wraps on wilder values where this clamps.  For damaged or
 * adversarial streams the output is still fully defined, kernel = host statement byte for byte, status as under rule 0.  The pin is
 * executed Pillow (bundled libjpeg-turbo), byte for byte on every stream of the tests; OpenCV has never run here.
 * Rule 1 decodes to WHENET_SURF_PACKED only: an I420 / NV12 destination under rule 1 is WHENET_EINVAL.  The kernels are rule-1 forms
 * of the inverse DCT and frame kernels (the rule is fixed at compile time in each); a clip is decoded by one rule and enqueues no more
 * than under rule 0.
 *   option "jpeg_rule"       0: rule 0 (default); 1: rule 1.  Read by whenet_frame_begin_jpeg, whenet_clip_begin_jpeg,
 *                  whenet_jpeg_decode_device, whenet_op_jpeg_decode[_ex] and whenet_op_jpeg_decode_clip.
 *   The six calls below are the calls they are named after with `rule` beside their arguments: 0 or 1, and for the calls on a handle
 *   -1 = the handle's option (as entropy -1 = the handle's entropy options, which whenet_op_jpeg_decode_rule accepts too).
 *   whenet_jpeg_decode_rule_host, whenet_jpeg_decode_segmented_rule_host   the host statement, plain and segmented
 *   whenet_op_jpeg_decode_rule, whenet_op_jpeg_decode_clip_rule            the kernels alone, one stream and a clip
 *   whenet_frame_begin_jpeg_rule, whenet_clip_begin_jpeg_rule              the resident-frame calls
 * Not built: clips of streams already in device memory, a stitch of several lanes per interval, a marker scan of several
 * workgroups, arithmetic / 12-bit streams, YUV surfaces under rule 1, OpenCV's own bytes (progressive streams: the next section).
 * WHENET_EINVAL: a NULL argument or plane, size < 1, a pitch below the row bytes, an unknown format / channel order, a seg_bytes,
 * window, entropy or rule value outside its range.
 *
 * JPEG DECODER, PROGRESSIVE (seven entry points, ABI still 6; csrc/jpeg_prog.hip, the arithmetic is csrc/jpeg_prog_host.h's).
 * Stills are where progressive streams (SOF2) are common, and cv2.imread opens them without a word.  The decoder for them is OPT-IN:
 * every call above keeps refusing SOF2 with its defaults ("progressive DCT (SOF2) ..."), every clip call above always does.  The calls
 * named ..._progressive, and whenet_frame_begin_jpeg[_rule] / whenet_op_jpeg_decode[_ex|_rule] on a handle whose option
 * "jpeg_progressive" is 1 (default 0), accept them.  A SOF0 stream through those calls is the baseline decoder's result, byte for
 * byte (its entropy options apply; for SOF2 they are ignored): one call serves a folder of mixed files.
 * ACCEPTED.  SOF2, 8 bit, 1 or 3 components, the samplings, sides and 8-bit DQT of the baseline parser.  Between scans: DHT (class
 * 0..1, ids 0..3; libjpeg writes optimised tables in front of almost every scan), DRI (a scan uses the value in force at its SOS),
 * APPn and COM; a DQT behind the first SOS is refused.  A scan holds all components (interleaved: the frame's MCUs) or ONE; a scan
 * of one component of a 3-component frame has single blocks as its MCUs and covers ceil(cw / 8) x ceil(ch / 8) blocks of that
 * component in raster order, cw = ceil(w hs_c / hs_max) -- NOT the plane padded to whole frame MCUs; blocks of the padded plane
 * outside that grid receive DC only.  Refused with the reason (WHENET_EFORMAT, on the host, before anything is enqueued): Ns = 2 (LAYOUTS below: opt-in);
 * Ss > Se or Se > 63; Ss = 0 with Se != 0; Ss > 0 with Ns > 1; Ah or Al > 13; a first scan (Ah = 0) of a coefficient that already
 * had one; a refinement of a coefficient without a first scan, or with Ah != the coefficient's current Al or Al != Ah - 1; an AC
 * scan of a component whose DC has had no scan; more than WHENET_JPEG_PROG_MAX_SCANS scans; a missing table.
 * SCAN PLAN.  The host walks the entropy data for 0xFF pairs to find each scan's end and its restart markers (INTERVALS above, per
 * scan); the starts of all (scan, interval) ITEMS travel with the plan and no device marker scan runs.  Items are numbered scan by
 * scan in stream order, an item per interval.  level(s) = 1 + the largest level of an earlier scan that shares a component and
 * overlaps its band [Ss, Se] (else 1): the scans of one level touch different values.  libjpeg's default script has 3 levels.
 * SCAN DECODE (T.81 G.1.2 / G.2 as jdphuff.c executes it).  Raw coefficients are int16 [block][64], record order as above, ZIGZAG
 * order inside a record, zero at the start, computed in int32 and clamped to -32768..32767 at every store.  DC first: the baseline
 * DC symbol and EXTEND, predictors 0 at every interval start; coefficient 0 = pred << Al.  DC refine: one bit per block; 1: |= 1 <<
 * Al.  AC first: (r, s > 0) skips r, coefficient k = EXTEND(s bits) << Al; (15, 0) skips 16; (r < 15, 0): EOBRUN = (1 << r) + r
 * extra bits, which ends this block and the next EOBRUN - 1 blocks of the interval.  AC refine, p1 = 1 << Al: a symbol with s != 0
 * must have s = 1 and reads a sign bit; on the way over r coefficients without a history every non-zero coefficient reads one
 * correction bit (1 and (coef & p1) == 0: coef moves by p1 away from zero); then the new +-p1 is placed; (15, 0) passes 16 such
 * coefficients the same way; inside an EOB run and behind an EOB the non-zero coefficients of the band still read their bits.
 * DAMAGE makes the ITEM bad: no code word; bits ending inside a symbol, a sign or a correction bit; a run that passes Se; s > 1
 * in a refinement; an EOBRUN that passes the interval's last block.  The block in hand keeps what was written, the scan does not
 * touch the rest of that interval, OTHER SCANS GO ON and see what the raw coefficients hold.  status[0] = WHENET_OK or
 * WHENET_EFORMAT, status[1] = the smallest bad item (else -1).  INCOMPLETE PROGRESSION -- EOI or the end of the bytes before every
 * coefficient of every component reached Al = 0 -- is decoded from what the scans hold: WHENET_EFORMAT with status[1] = the item
 * count.  There is NO block smoothing (libjpeg smooths the blocks of an incomplete progression; here they are not).
 * FINISH.  record[natural k] = clamp(raw[zigzag k] x Q[k], -2048, 2047): the records the inverse DCT above reads; planes, frame and
 * YUV surfaces follow unchanged under both rules (rule 1's SCOPE paragraph applies as written).
 *   whenet_jpeg_parse_scans   pure host: *info (for SOF2 its Huffman fields stay empty) and up to cap whenet_jpeg_scan_t records;
 *                  *num_scans = the stream's scans (cap below it: WHENET_EINVAL).  A SOF0 stream is one scan (0..63, Ah = Al = 0).
 *   whenet_jpeg_decode_progressive_host, ..._planes_host   the host statement, as the calls they are named after, with `rule`
 *   whenet_jpeg_progressive_coefficients_host   the finished records int16 [blocks][64] and, where not NULL, the raw ones and the
 *                  counters int64 [8]: scans, items, levels, the largest EOBRUN met, ZRLs in refinement scans, correction bits read,
 *                  correction bits that changed a coefficient, 0.  blocks = MCUs x blocks per MCU (cap_blocks below it:
 *                  WHENET_EINVAL); SOF2 only.
 *   whenet_op_jpeg_decode_progressive   the kernels alone, host to host; rule as whenet_op_jpeg_decode_rule; stats (may be NULL)
 *                  int64 [8]: for SOF2 items, levels, scans, launches of the scan kernel; for SOF0 whenet_op_jpeg_decode_ex's.
 *   whenet_frame_begin_jpeg_progressive   the twin of whenet_frame_begin_jpeg_rule: ONE H2D of the plan (scan records, per-scan
 *                  tables, item lists, the bytes from the first scan's data on), one memset, a launch per level, the finish, then
 *                  the inverse DCT and colour kernels: enqueue-only on the copy stream.
 *   whenet_jpeg_progressive_counters   out[0..2]: decodes enqueued, scan-kernel launches, scans in them.
 *   option "jpeg_progressive"  0 (default) / 1, above.   option "jpeg_prog_levels"  1 (default): a launch per level; 0: a launch per
 *                  scan in stream order (a measurement knob of the SINGLE-STREAM path: the bytes are the same; clips always launch
 *                  by level).
 * PROGRESSIVE STREAMS IN CLIPS (three more entry points, ABI still 6).  The clip calls above keep refusing SOF2 and do not read the
 * option "jpeg_progressive"; the three below accept it.  Frame f of such a clip is whenet_jpeg_decode_progressive_host(data[f],
 * rule) with its status pair, byte for byte, whether the stream is SOF2, SOF0 or the clip a mix of both; a SOF0 frame keeps the
 * entropy form it has in a baseline clip; a damaged stream damages its own frame only; a stream the scan parser refuses is
 * WHENET_EFORMAT "frame N: <the parser's reason>" before anything is enqueued.  Limits as above: 1..16 frames, one rule per clip,
 * option "letterbox_cache" for frames of different sizes.  Still ONE H2D (records | per frame tables | data, or, SOF2: scans | huff |
 * qz | items | data) and ONE memset (per frame start | meta | seg_stats | coef, or, SOF2: meta | raw coefficients).  Launch L of
 * the clip scan kernel covers level L of every SOF2 frame that has one, so their number is the LARGEST level count among the
 * frames (<= 14), not the sum; one finish launch; then the clip's inverse DCT and colour launches for all frames.  The marker
 * scan, entropy and segmented launches run for the SOF0 frames only, and not at all without one.
 *   whenet_op_jpeg_decode_clip_progressive   the arguments of whenet_op_jpeg_decode_clip_rule
 *   whenet_clip_begin_jpeg_progressive       the arguments of whenet_clip_begin_jpeg_rule
 *   whenet_jpeg_clip_plan_progressive        pure host, from the streams themselves: the layout such a clip gets.  out: num_frames *
 *                  WHENET_JPEG_CLIP_PROG_PLAN_FRAME_WORDS + WHENET_JPEG_CLIP_PROG_PLAN_TOTAL_WORDS int64.  A frame's words 0..31
 *                  and the totals' words 0..7 are whenet_jpeg_clip_plan's, form 2 marking a SOF2 frame (data, meta, coef and the
 *                  planes are its regions; tables, start, seg_stats and the segmented regions are empty).  A frame's words 32..41:
 *                  (offset, length) of scans, huff, qz, items, raw (empty for SOF0); 42..44: its scans, levels, item-list entries;
 *                  45..47: 0.  Totals 8: SOF2 frames, 9: scan-kernel launches, 10: the stride of the argument records, 11: where
 *                  a frame's progressive record lies inside its own; 12..15: 0.  Without a SOF2 frame the words 0..31 / 0..7
 *                  equal whenet_jpeg_clip_plan's.  entropy 0, 1 or 2 (auto), as there.
 * whenet_jpeg_clip_counters counts these clips as the others; whenet_jpeg_progressive_counters adds a decode per SOF2 frame, the
 * scan launches once per clip and the scans of all its frames.
 * Not built: a segmented (many lanes per interval) form for progressive scans -- a scan without DRI is ONE lane --, arithmetic, 12-bit and CMYK streams, block smoothing, a progressive
 * encoder, streams already in device memory.
 *
 * JPEG DECODER, ORIENTATION (six entry points, ABI still 6; the parser is csrc/jpeg_dec_host.h's jpeg_exif_orientation, the kernels
 * are the oriented frame kernels of csrc/jpeg_dec.hip).  Phone and camera stills are stored in sensor order with the EXIF
 * orientation tag (0x0112) set, and cv2.imread returns them upright.  The oriented decode is OPT-IN: every call above ignores the
 * tag, the six below apply it, and whenet_frame_begin_jpeg[_rule|_progressive] / whenet_op_jpeg_decode[_ex|_rule|_progressive] on a
 * handle whose option "jpeg_orient" is 1 (default 0) apply it too; the clip calls take the argument only.
 * THE TAG.  The marker segments from SOI to the first SOS; the FIRST APP1 whose payload starts with "Exif\0\0" (an XMP APP1 in front
 * of it is passed, a second Exif APP1 is never read); behind it the TIFF header ("II" or "MM", 42, the offset of IFD0); in IFD0
 * only, at any position, the entry with tag 0x0112, count 1 and type SHORT (3) or LONG (4).  A value outside 1..8, another type or
 * count, a bad header, an offset, an entry count or an entry that leaves the segment, no such segment: 1.  Broken EXIF never
 * refuses a stream and never changes its status; SOF0 and SOF2 streams are read alike.
 * THE FRAME.  With u the upright frame [h][w] of the same rule and t its transpose [w][h], the oriented frame is
 *     1: u    2: u[:, ::-1]    3: u[::-1, ::-1]    4: u[::-1]           (h x w)
 *     5: t    6: t[:, ::-1]    7: t[::-1, ::-1]    8: t[::-1]           (w x h)
 * byte for byte, under both rules and both channel orders: the pixel of source position (y, x) is what the upright kernels compute,
 * only its destination differs.  The destination (and a slot's frame, with everything behind it: letterbox, detector, crops,
 * overlay, boxes) has the ORIENTED size: for 5..8 w rows of at least 3 h bytes.  The oriented frame kernel takes the frame kernel's
 * place: 2..4 reverse and mirror a lane's 4-pixel group, 5..8 stage a 32 x 32 tile of the DESTINATION through LDS; no upright frame
 * exists in device memory, the work buffers do not grow, a single decode enqueues what the upright one enqueues and a clip with
 * turned frames at most one launch more.  A stream with value 1 runs exactly the upright launches.  Damage: the status pair is
 * the upright decode's, the frame the orientation of its defined frame.  Oriented decodes write WHENET_SURF_PACKED only: a stream
 * with a value 2..8 and an I420 / NV12 destination is WHENET_EINVAL (nothing is enqueued).
 *   whenet_jpeg_orientation             pure host: 1..8 (NULL or no stream: 1)
 *   whenet_jpeg_decode_oriented_host    the host statement: the table applied to the host decode by `rule` (0 / 1); progressive = 1
 *                  also accepts SOF2
 *   whenet_op_jpeg_decode_oriented      the kernels alone; entropy, seg_bytes, rule as whenet_op_jpeg_decode_rule; progressive and
 *                  orient -1 (the handle's option), 0 or 1; *orientation (may be NULL) = the value applied, 1 where orient is off
 *   whenet_op_jpeg_decode_clip_oriented the arguments of whenet_op_jpeg_decode_clip_rule, progressive and orient 0 or 1, orientation
 *                  (may be NULL) int32 [num_frames]; every frame has its own value; upright and turned frames share a clip
 *   whenet_frame_begin_jpeg_oriented, whenet_clip_begin_jpeg_oriented   the resident-frame calls, the same arguments: the slot is what
 *                  whenet_frame_begin / whenet_clip_begin[_mixed] of the oriented frames leaves; a clip is one-size by its ORIENTED sizes
 *   option "jpeg_orient"   0 (default) / 1, above.
 * Not built: oriented I420 / NV12 destinations, whenet_jpeg_decode_device (it sees no header), an orientation stored anywhere but IFD0
 * of the first Exif APP1, other EXIF tags.
 *
 * JPEG DECODER, DEFAULT TABLES (one entry point, 131 in all, ABI still 6; csrc/jpeg_dec_host.h's jpeg_add_default_tables).  The MJPG
 * frames of UVC cameras and of many AVI writers carry no DHT segment: their Huffman tables are T.81's Annex K ones, which every
 * player installs (libjpeg's std_huff_tables).  Every call above refuses such a stream with "a missing Huffman table (DHT)", and
 * keeps doing so; this pure host function completes the stream first:
 *   whenet_jpeg_add_default_tables   walks the header to the first SOS.  For each of the four slots DC 0, AC 0, DC 1, AC 1 that no
 *                  DHT in front of that SOS defines it adds the Annex K table of that slot (K.3 / K.5 for id 0, K.4 / K.6 for id
 *                  1): the missing tables go into ONE DHT segment, in that order, directly in front of the first SOS marker, at
 *                  most 420 bytes more.  out[0 .. *out_size) is the completed stream.  A stream that defines all four comes back
 *                  byte for byte, and so does a header that cannot be followed to an SOS (no SOI, a truncated or malformed
 *                  segment): this call never refuses a stream, the decoder then gives its own reason.  Ids 2 and 3 are never
 *                  filled.  WHENET_EINVAL only for a NULL argument or capacity < size + 420.
 * Not built: default tables for ids 2 / 3, default quantiser tables (no player installs any).
 *
 * JPEG DECODER, LAYOUTS (ten entry points, declared in the companion header include/whenet_hip_jpeg_accept.h, which includes
 * this one; this header keeps its 131; ABI still 6; the parsers of csrc/jpeg_dec_host.h and csrc/jpeg_prog_host.h
 * with their `layouts` argument, frame_group of csrc/jpeg_dec.hip, the sequential scan kernel of csrc/jpeg_prog.hip).  Three kinds of
 * ordinary 8-bit Huffman JPEG that cv2.imread opens without a word are refused by every call above: the chroma samplings 4:4:0 (luma
 * 1x2: what a lossless quarter turn makes of a 4:2:2 camera file), 4:1:1 (luma 4x1: DV-derived cameras and grabbers) and 4:1:0 (luma
 * 4x2: old webcams); sequential frames of several scans and scans of two components (jpegtran -scans, several camera firmwares);
 * SOF1, which libjpeg writes as soon as a frame uses a Huffman table id above 1.  Decoding them is OPT-IN: every call above keeps
 * refusing them with the text it has; the calls named ..._accept take one set of bits `accept` -- WHENET_JPEG_ACCEPT_PROGRESSIVE (1:
 * what `progressive` = 1 is above) and WHENET_JPEG_ACCEPT_LAYOUTS (2) --, and whenet_frame_begin_jpeg[_rule|_progressive|_oriented] /
 * whenet_op_jpeg_decode[_ex|_rule|_progressive|_oriented] with their defaults and whenet_jpeg_decode_device on a handle whose option
 * "jpeg_layouts" is 1 (default 0) accept them too; clips take the argument only.  The `progressive` arguments above keep their 0 / 1
 * range.  A stream every call accepts is the same bytes with the bit.
 * ACCEPTED with the LAYOUTS bit, besides everything accepted without it.
 *   Samplings: luma (hs, vs) in {1, 2, 4} x {1, 2} with chroma 1x1, in SOF0, SOF1 and (with the PROGRESSIVE bit) SOF2 frames: bpm =
 *   hs vs + 2 blocks per MCU, up to 10 (T.81's limit); info.hs / info.vs simply take the new values.
 *   Sequential frames (SOF0 / SOF1, 8 bit): any number of scans in which every component occurs exactly once, each with Ns 1..3 (its
 *   components in the frame's order), Ss = 0, Se = 63, Ah = Al = 0 and Huffman ids 0..3; DHT, DRI, APPn and COM between scans (a scan
 *   uses the tables and the DRI in force at its SOS).  A scan of one component of a 3-component frame covers that component's own
 *   ceil(cw / 8) x ceil(ch / 8) blocks in raster order (the PROGRESSIVE section's rule; cw = ceil(w / hs) for chroma); a scan of two
 *   or three components is interleaved over the FRAME's MCU grid, its MCU the H_c V_c blocks of each of its components in scan order
 *   (T.81 A.2.3).
 *   SOF2: a DC scan (first or refinement) of two components, interleaved the same way.
 * REFUSED with the bit, on the host, before anything is written -- with a reason that names the factors: a chroma factor other than
 * 1x1 ("chroma sampling factors other than 1x1 ..."), Cb and Cr that differ, vs = 4, any other luma pair; with the reasons they have
 * above: 16-bit DQT, 12 bit, arithmetic coding, 4 components, lossless and hierarchical frames; with new reasons: "a component in two
 * scans of a sequential frame", "a spectral selection or successive approximation in a sequential frame (...)", a DQT behind the
 * first scan.
 * ROUTING.  A sequential frame of ONE interleaved scan with Huffman ids 0..1 -- SOF0, or SOF1 that happens to qualify -- is the
 * baseline decoder's: both entropy forms, the auto rule, clips and whenet_jpeg_decode_device, on the general geometry.  Every other
 * sequential frame goes through the SCAN PLAN of the PROGRESSIVE section as a fifth scan kind, "sequential": an item is one (scan,
 * interval); per block the baseline block decode (DC symbol + EXTEND on the component's predictor, 0 at every interval start, then AC
 * symbols, no EOB runs) writes RAW values in zigzag order into records the memset zeroed; FINISH, inverse DCT and frame follow
 * unchanged and give exactly the baseline decoder's records.  The scans of one frame hold different components, so all are level 1:
 * ONE launch of the sequential scan kernel per frame, and ONE for all such frames of a clip (next to the launches per level of the
 * clip's SOF2 frames).  The plan carries six tables per sequential scan (the DC tables of its components, then their AC tables).
 * DAMAGE and the status pair follow the PROGRESSIVE section's ITEM rule (items numbered scan by scan, one per restart interval); a
 * component without a scan at EOI or at the end of the bytes is the incomplete-progression status (status[1] = the item count) and
 * its plane is decoded from zero coefficients.  Stated, not fixed: a multi-scan stream without DRI is one lane per scan.
 * GEOMETRY.  An MCU is 8 hs x 8 vs luma samples: its luma blocks in vs rows of hs, then Cb, then Cr, as above.  Both entropy forms,
 * the sync state of the segmented form (the block's index in its MCU, 0..9, in 8 bits), the component of a block in the count and
 * write kernels, the clip plans and the scan plan are written in hs, vs and bpm and take the new values as they are: the output does
 * not depend on the form, seg_bytes or "jpeg_seg_lanes".  Every work buffer, clip-plan word and segment bound is computed from the
 * stream's own counts -- records: MCUs x bpm x 128 bytes; segments: ceil(nbytes / seg_bytes) + intervals --, never from a
 * per-sampling constant: a full-width MCU row is 1024 x 4 = 4096 blocks at 4:4:0, 256 x 6 = 1536 at 4:1:1 and 256 x 10 = 2560 at
 * 4:1:0, against (8192 / 16) x 6 = 3072 at 4:2:0 and 1024 x 3 = 3072 at 4:4:4.  (JPEG_MAX_INTERVAL_BLOCKS = 3072 of csrc/jpeg_host.h
 * bounds the ENCODER's three samplings -- its per-interval bit budget -- and is not read by the decoder.)
 * FRAME, RULE 0.  Pixel (x, y) takes the chroma sample (x >> log2 hs, y >> log2 vs); for hs = 4 a lane's four pixels share one
 * sample, loaded as one byte (aligned wherever it lies, inside the padded plane: x / 4 < 8 mcu_cols).
 * FRAME, RULE 1 (libjpeg-turbo's jdsample.c as Pillow 12.2.0 / libjpeg-turbo 3.1.4.1 executes it; tests/test_jpeg_layouts_cpu.py
 * holds every stream of its table to the executed library, on noisy pictures).  4:4:0 is h1v2_fancy_upsample: with r = y >> 1 and the
 * neighbour rows clamped to 0 .. ch - 1, an even row is (3 in[r] + in[r - 1] + 1) >> 2 and an odd row (3 in[r] + in[r + 1] + 2) >> 2;
 * nothing is filtered along x and there is NO narrow-width switch (w = 2 is filtered, unlike 4:2:0 / 4:2:2).  4:1:1 and 4:1:0 are
 * plain replication, in[y >> log2 vs][x >> 2] (int_upsample: no filter in either direction).  jdcolor's row and the SCOPE paragraph
 * apply as written.  The oriented frame kernels compute their pixels through the same function and inherit both rules.  I420 / NV12
 * destinations stay 4:2:0-only (WHENET_EINVAL otherwise) and stay refused under rule 1.
 *   whenet_jpeg_parse_scans_accept      whenet_jpeg_parse_scans with the bits: a sequential frame of several scans lists them (level
 *                  1 each, progressive = 0); without the PROGRESSIVE bit a SOF2 stream is refused with the baseline parser's text
 *   whenet_jpeg_decode_accept_host      the host statement: rule 0 / 1, orient 0 / 1 (the EXIF orientation is applied),
 *                  *orientation (may be NULL) = the value applied
 *   whenet_jpeg_decode_accept_planes_host   the same up to the component planes
 *   whenet_jpeg_decode_segmented_accept_host, ..._accept_planes_host   the emulation of the segmented form (the baseline decoder's
 *                  streams only); accept 0 or 2
 *   whenet_op_jpeg_decode_accept        whenet_op_jpeg_decode_oriented with `accept` (-1: the handle's two options) for `progressive`;
 *                  stats of a frame that went through the scan plan: items, levels, scans, launches of the scan kernel
 *   whenet_op_jpeg_decode_clip_accept, whenet_frame_begin_jpeg_accept, whenet_clip_begin_jpeg_accept   the twins of the ..._oriented
 *                  calls, `accept` for `progressive` (a clip: 0..3, never -1)
 *   whenet_jpeg_clip_plan_accept        whenet_jpeg_clip_plan_progressive with the bits; a sequential frame that goes through the
 *                  scan plan is a form-2 frame of ONE level there, its `huff` region six tables per scan, and the totals' word 9
 *                  is the SOF2 frames' largest level count + 1 where the clip holds such a frame
 *   option "jpeg_layouts"   0 (default) / 1, above.
 * whenet_jpeg_progressive_counters counts a frame that goes through the scan plan, its launch and its scans like a SOF2 frame's.
 * Not built: a segmented (many lanes per interval) form for the scans of the scan plan, a component split over several sequential
 * scans, default tables for ids 2 / 3, a DQT between scans. */
#define WHENET_JPEG_SEG_WINDOW 256
#define WHENET_JPEG_PROG_MAX_SCANS 128
#define WHENET_JPEG_CLIP_PLAN_FRAME_WORDS 32
#define WHENET_JPEG_CLIP_PLAN_TOTAL_WORDS 8
#define WHENET_JPEG_CLIP_PROG_PLAN_FRAME_WORDS 48
#define WHENET_JPEG_CLIP_PROG_PLAN_TOTAL_WORDS 16
typedef struct {
    int32_t h, w, components;
    int32_t hs, vs;                  /* luma sampling factors (1 or 2; LAYOUTS: hs 1, 2 or 4); chroma is 1 x 1 */
    int32_t qt[3], dc[3], ac[3];     /* per component: quantiser id, DC and AC Huffman table ids */
    int32_t restart_interval;        /* Ri in MCUs; 0: no DRI */
    int32_t intervals;               /* ceil(MCUs / Ri); 1 without DRI */
    int64_t data_offset;             /* where the entropy data begins in the stream */
    uint8_t q[4][64];                /* natural order */
    uint8_t q_present[4];
    uint8_t huff_counts[4][16];      /* index 2 id + class: DC0, AC0, DC1, AC1 */
    uint8_t huff_values[4][256];
    uint8_t huff_present[4];
} whenet_jpeg_info_t;
typedef struct {
    int32_t ns, comp[3];             /* the scan's components: indices into the frame's */
    int32_t ss, se, ah, al;
    int32_t dc[3], ac[3];            /* per scan component: the table ids of its SOS */
    int32_t tables;                  /* the snapshot of the Huffman tables in force at its SOS: DHT segments seen so far */
    int32_t ri, intervals;           /* Ri in the scan's own MCUs, ceil(scan MCUs / Ri) */
    int32_t level;                   /* 1.. */
    int32_t first_item;              /* its first flat item index */
    int32_t progressive;             /* 1: a scan of a SOF2 frame; 0: the one scan of a SOF0 frame */
    int64_t data_offset, data_bytes; /* its entropy data in the stream */
} whenet_jpeg_scan_t;
WHENET_API int whenet_jpeg_parse(const uint8_t* data, int64_t size, whenet_jpeg_info_t* info);
WHENET_API int whenet_jpeg_decode_host(const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int32_t status[2]);
WHENET_API int whenet_jpeg_decode_planes_host(const uint8_t* data, int64_t size, uint8_t* const* planes, const int* pitch, int32_t status[2]);
WHENET_API int whenet_op_jpeg_decode(whenet_t* h, const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order,
                          int32_t status[2]);
WHENET_API int whenet_jpeg_decode_device(whenet_t* h, const whenet_jpeg_info_t* info, const uint8_t* d_entropy, int64_t nbytes,
                              const whenet_surface_t* dst, int channel_order, int32_t* d_status, void* stream);
WHENET_API int whenet_frame_begin_jpeg(whenet_t* h, const uint8_t* data, int64_t size, int channel_order, int* ticket, int32_t* status);
WHENET_API int whenet_jpeg_decode_segmented_host(const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int seg_bytes,
                                      int window, int32_t status[2], int64_t stats[8]);
WHENET_API int whenet_jpeg_decode_segmented_planes_host(const uint8_t* data, int64_t size, uint8_t* const* planes, const int* pitch, int seg_bytes,
                                             int window, int32_t status[2], int64_t stats[8]);
WHENET_API int whenet_op_jpeg_decode_ex(whenet_t* h, const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int entropy,
                             int seg_bytes, int32_t status[2], int64_t stats[8]);
WHENET_API int whenet_jpeg_decode_counters(whenet_t* h, int64_t out[4]);
WHENET_API int whenet_jpeg_seg_dc_scan_host(const int32_t* diff, int64_t n, int chunk, int32_t* pred);
WHENET_API int whenet_clip_begin_jpeg(whenet_t* h, const uint8_t* const* data, const int64_t* size, int num_frames, int channel_order, int* ticket,
                           int32_t* status);
WHENET_API int whenet_op_jpeg_decode_clip(whenet_t* h, const uint8_t* const* data, const int64_t* size, int num_frames, const whenet_surface_t* dst,
                               int channel_order, int32_t* status, int entropy, int seg_bytes);
WHENET_API int whenet_jpeg_clip_plan(const whenet_jpeg_info_t* infos, const int64_t* nbytes, int num_frames, int entropy, int seg_bytes,
                          int64_t* out);
WHENET_API int whenet_jpeg_clip_counters(whenet_t* h, int64_t out[4]);
WHENET_API int whenet_jpeg_decode_rule_host(const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int rule,
                                 int32_t status[2]);
WHENET_API int whenet_jpeg_decode_segmented_rule_host(const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order,
                                           int seg_bytes, int window, int rule, int32_t status[2], int64_t stats[8]);
WHENET_API int whenet_op_jpeg_decode_rule(whenet_t* h, const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int entropy,
                               int seg_bytes, int rule, int32_t status[2], int64_t stats[8]);
WHENET_API int whenet_op_jpeg_decode_clip_rule(whenet_t* h, const uint8_t* const* data, const int64_t* size, int num_frames,
                                    const whenet_surface_t* dst, int channel_order, int32_t* status, int entropy, int seg_bytes, int rule);
WHENET_API int whenet_frame_begin_jpeg_rule(whenet_t* h, const uint8_t* data, int64_t size, int channel_order, int rule, int* ticket,
                                 int32_t* status);
WHENET_API int whenet_clip_begin_jpeg_rule(whenet_t* h, const uint8_t* const* data, const int64_t* size, int num_frames, int channel_order, int rule,
                                int* ticket, int32_t* status);

WHENET_API int whenet_jpeg_parse_scans(const uint8_t* data, int64_t size, whenet_jpeg_info_t* info, whenet_jpeg_scan_t* scans, int cap,
                            int* num_scans);
WHENET_API int whenet_jpeg_decode_progressive_host(const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int rule,
                                        int32_t status[2]);
WHENET_API int whenet_jpeg_decode_progressive_planes_host(const uint8_t* data, int64_t size, uint8_t* const* planes, const int* pitch, int rule,
                                               int32_t status[2]);
WHENET_API int whenet_jpeg_progressive_coefficients_host(const uint8_t* data, int64_t size, int16_t* coef, int16_t* raw, int64_t cap_blocks,
                                              int64_t counters[8], int32_t status[2]);
WHENET_API int whenet_op_jpeg_decode_progressive(whenet_t* h, const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order,
                                      int rule, int32_t status[2], int64_t stats[8]);
WHENET_API int whenet_frame_begin_jpeg_progressive(whenet_t* h, const uint8_t* data, int64_t size, int channel_order, int rule, int* ticket,
                                        int32_t* status);
WHENET_API int whenet_jpeg_progressive_counters(whenet_t* h, int64_t out[4]);
WHENET_API int whenet_op_jpeg_decode_clip_progressive(whenet_t* h, const uint8_t* const* data, const int64_t* size, int num_frames,
                                           const whenet_surface_t* dst, int channel_order, int32_t* status, int entropy, int seg_bytes,
                                           int rule);
WHENET_API int whenet_clip_begin_jpeg_progressive(whenet_t* h, const uint8_t* const* data, const int64_t* size, int num_frames, int channel_order,
                                       int rule, int* ticket, int32_t* status);
WHENET_API int whenet_jpeg_clip_plan_progressive(const uint8_t* const* data, const int64_t* size, int num_frames, int entropy, int seg_bytes,
                                      int64_t* out);

WHENET_API int whenet_jpeg_add_default_tables(const uint8_t* data, int64_t size, uint8_t* out, int64_t capacity, int64_t* out_size);
WHENET_API int whenet_jpeg_orientation(const uint8_t* data, int64_t size);
WHENET_API int whenet_jpeg_decode_oriented_host(const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int rule,
                                     int progressive, int32_t status[2]);
WHENET_API int whenet_op_jpeg_decode_oriented(whenet_t* h, const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order,
                                   int entropy, int seg_bytes, int rule, int progressive, int orient, int32_t status[2], int64_t stats[8],
                                   int32_t* orientation);
WHENET_API int whenet_op_jpeg_decode_clip_oriented(whenet_t* h, const uint8_t* const* data, const int64_t* size, int num_frames,
                                        const whenet_surface_t* dst, int channel_order, int32_t* status, int entropy, int seg_bytes, int rule,
                                        int progressive, int orient, int32_t* orientation);
WHENET_API int whenet_frame_begin_jpeg_oriented(whenet_t* h, const uint8_t* data, int64_t size, int channel_order, int rule, int progressive,
                                     int orient, int* ticket, int32_t* status, int32_t* orientation);
WHENET_API int whenet_clip_begin_jpeg_oriented(whenet_t* h, const uint8_t* const* data, const int64_t* size, int num_frames, int channel_order,
                                    int rule, int progressive, int orient, int* ticket, int32_t* status, int32_t* orientation);

/* ---- measurement: run `iters` eager forwards of `n` device-resident crops exactly as the
 * timed path runs them (same concurrent sub-batch chains, same streams) with ONE HIP event
 * recorded on the chain's stream between consecutive kernel launches; a launch's time is
 * previous event -> its own event.  Fills up to `cap` entries, one per launch of a chain in
 * launch order, averaged over chains and iterations; alg_bytes / alg_flops are those of one
 * chain's launch (its sub-batch).  *count = launches per chain. */
WHENET_API int whenet_profile(whenet_t* h, const uint8_t* d_crops, int n, int iters,
                   whenet_launch_stat_t* stats, int cap, int* count);

/* ---- single-stage entry points (host pointers, float32 activations in/out, converted to
 * the handle's dtype on the device).  They run exactly the kernels the forward uses, on
 * caller-supplied inputs, so each kernel can be compared with the oracle on every layer
 * shape.  Any output pointer may be NULL. */
/* stem: normalise + Conv3x3/s2 + BN + Swish.  out [n,112,112,32] */
WHENET_API int whenet_op_stem(whenet_t* h, const uint8_t* crops, int n, float* out);
/* MBConv block `index` (1..16) on input [n,H,W,Cin]:
 *   expand_out [n,H,W,Cexp] (NULL for block 1), dw_out [n,Ho,Wo,Cexp], gate [n,Cexp],
 *   out [n,Ho,Wo,Cout] (after project + BN + skip) */
WHENET_API int whenet_op_block(whenet_t* h, int index, const float* in, int n,
                    float* expand_out, float* dw_out, float* gate, float* out);
/* MBConv blocks first..last (1 <= first <= last <= 16) chained exactly as the forward pass chains them -- including
 * option fold12 (block 1's project folded into block 2's expand) when the range holds blocks 1 and 2 -- on input
 * [n,H,W,Cin] of block `first`; out [n,Ho,Wo,Cout] of block `last`.  The input and the output are NHWC; the tensors between
 * the blocks take the layout the forward gives them (option act_layout). */
WHENET_API int whenet_op_block_range(whenet_t* h, int first, int last, const float* in, int n, float* out);
/* head: Conv1x1(1280)+BN+Swish + GAP + Dense heads + decode on input [n,7,7,320]:
 *   feat [n,1280], logits [n,252], ypr [n,3], argmax [n,3]
 * Runs the launches the forward runs under the handle's options: head conv + pooling as one kernel and the four-workgroup heads
 * kernel on its features (head_fuse = 1 and split_heads = 1, the default); else the head conv as a GEMM and the heads stage on its
 * output tensor, as four workgroups per crop (split_heads = 1) or as one (split_heads = 0).  The four-workgroup kernel on the
 * tensor has no feature output: there `feat` comes from a separate launch of the one-workgroup kernel, whose logits, angles and
 * argmax are discarded.  whenet_op_decode always runs the one-workgroup kernel (the other one has no logits input). */
WHENET_API int whenet_op_head(whenet_t* h, const float* in, int n,
                   float* feat, float* logits, float* ypr, int32_t* argmax);
/* decode only (whenet.py:28-33) on caller logits [n,252] -> ypr [n,3], argmax [n,3] */
WHENET_API int whenet_op_decode(whenet_t* h, const float* logits, int n, float* ypr, int32_t* argmax);

/* layer geometry as the engine sees it (for cross-checking against whenet_hip/spec.py):
 * fills out[0..7] = {k, stride, expand, cin, cout, h_in, h_out, se_reduced} for block
 * `index` (1..16). */
WHENET_API int whenet_block_spec(int index, int32_t out[8]);

/* the depthwise tile plan of block `index` for `dtype` (pure host logic; no GPU needed):
 * out = {threads, CV, TH, NSX, tiles_x, tiles_y, chunks, IH, IW, lds_bytes, pad_before, C} */
WHENET_API int whenet_dw_plan(int dtype, int index, int32_t out[12]);

/* the fused expand+depthwise tile plan of block `index` (2..16) for `dtype` (pure host logic):
 * out = {threads, CC, TH, NSX, tiles_x, tiles_y, chunks, EH, EW, lds_bytes, w_off, Cexp} */
WHENET_API int whenet_front_plan(int dtype, int index, int32_t out[12]);

/* front2.hip's static-plan check (pure host logic): the constexpr plan of row `row` of the kernel's plan table against the
 * plan the engine launches for that layer, field by field, with the static plan's field number `field` moved by `delta`
 * (field = -1: nothing moved).  WHENET_OK when they agree; WHENET_EINVAL when they differ (a launch would refuse to run),
 * the row has no static form or there is no such field. */
WHENET_API int whenet_front2_static_check(int row, int field, int delta);

/* The same for pw.hip's static-shape form of the project GEMMs: row 0..10 of its shape table (b2, b3, b4, b5, b6, b7/b8, b9, b10/b11,
 * b12, b13-15, b16; also the rows whose static form is not built) as the engine launches the layer at 64 crops, against the row's constexpr shape with its field-th int
 * (K, N, HW, KS, NTILES, NCH, family, B2, GM, RES, lay, np, R, RP) moved by delta (field = -1: nothing moved). */
WHENET_API int whenet_pw_static_check(int row, int field, int delta);

/* The same for front.hip's static-shape form: row 0 (block 6) with plan_front()'s plan and 256 lanes, against the row's constexpr
 * shape with its field-th int (H, Ho, Cin, Cexp, pad, KSe, NTe, CC, TH, NSX, tiles_x, tiles_y, EH, EW, EP, w_off, R, RP, ntiles,
 * chunks, k, s, threads, lds_bytes) moved by delta. */
WHENET_API int whenet_front_static_check(int row, int field, int delta);

/* raw device-memory helpers so a host without torch can use the device-pointer form */
WHENET_API int whenet_device_alloc(whenet_t* h, size_t nbytes, void** d_ptr);
WHENET_API int whenet_device_free(whenet_t* h, void* d_ptr);
WHENET_API int whenet_memcpy_h2d(whenet_t* h, void* d_dst, const void* src, size_t nbytes);
WHENET_API int whenet_memcpy_d2h(whenet_t* h, void* dst, const void* d_src, size_t nbytes);

#ifdef __cplusplus
}
#endif
#endif /* WHENET_HIP_H */
