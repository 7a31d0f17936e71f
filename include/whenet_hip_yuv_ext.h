/* YUV INGEST, EXTENDED: what a decoder makes of today's video -- 16-bit sample containers (P010 / P012 / P016, yuv420p10le / I010,
 * the 16-bit surfaces of a hardware decoder), planar 4:4:4 (I444, 8 or 16 bit) and the BT.2020 matrix -- through seven entry points,
 * the twins of the seven YUV calls of whenet_hip.h, in a header of their own.  The same library exports them; the ABI is
 * whenet_hip.h's (6); whenet_yuv_frame_t, its calls, its format codes and WHENET_YUV_MATRICES / WHENET_YUV_COEFFS are what they
 * were: a caller who does not include this header sees the interface whenet_hip.h had before it.
 *
 * A FRAME is a layout times a sample container.
 *   layout     WHENET_YUV_NV12   Y plane and an interleaved U V plane, 4:2:0              (plane[2] unused)
 *              WHENET_YUV_I420   Y, U, V planes, 4:2:0
 *              WHENET_YUV_YUYV / WHENET_YUV_UYVY   packed 4:2:2, one plane, 8-bit container only   (plane[1..2] unused)
 *              WHENET_YUVX_I444  Y, U, V planes, all h x w
 *   container  WHENET_YUVX_U8    one byte per sample
 *              WHENET_YUVX_U16   two bytes per sample, little endian, with the frame's `shift` in 0..8: the sample at 16 bits,
 *                                MSB-aligned, is s16 = (word << shift) & 0xFFFF.  shift 0: P010 / P012 / P016 and a hardware
 *                                decoder's 16-bit surfaces (one layout; the low bits are simply used).  shift 6: yuv420p10le / I010
 *                                (bits above bit 9 of a word are masked off).  shift 4: the 12-bit LSB-aligned forms.
 * So NV12 x U16 is the P010 / P016 family, I420 x U16 the I010 family, I444 x U8 is I444 / a decoder's YUV444 surface, I444 x U16 its
 * 16-bit twin; and the four formats of whenet_yuv_frame_t are the layouts 0, 1, 3, 4 with WHENET_YUVX_U8 and shift 0.
 * Sizes: h x w luma samples, sides 1..8192, odd sizes included; 4:2:0 chroma planes have ch = (h + 1) >> 1 rows of cw = (w + 1) >> 1
 * samples (2 cw for the interleaved plane) and pixel (y, x) takes the sample (y >> 1, x >> 1); 4:4:4 chroma planes have h rows of w
 * samples and pixel (y, x) takes the sample (y, x).  Chroma is nearest neighbour, as in whenet_hip.h.  pitch[] is in BYTES, >= the
 * plane's row bytes (samples x 1 or 2).  A plane of a 16-bit container lies at an even address with an even pitch.
 *
 * THE ARITHMETIC.  An 8-bit container uses the statement of whenet_hip.h unchanged.  A 16-bit container, with
 * {yoff, CY, CVR, CUG, CVG, CUB} = WHENET_YUVX_COEFFS[matrix], in EXACT integers (the terms reach 2^37.2: 64-bit arithmetic) and >>
 * an arithmetic shift:
 *     c = max(0, Y16 - (yoff << 8));  d = U16 - 32768;  e = V16 - 32768
 *     base = CY * c + (1 << 27)
 *     B = clip8((base + CUB * d) >> 28)
 *     G = clip8((base - CUG * d - CVG * e) >> 28)
 *     R = clip8((base + CVR * e) >> 28)
 * A 16-bit frame whose samples are 8-bit samples << 8 gives exactly the 8-bit statement's bytes (every term is the 8-bit term x 256).
 * MATRICES.  WHENET_YUVX_COEFFS holds the three rows of WHENET_YUV_COEFFS and a fourth:
 *     WHENET_YUV_BT2020  non-constant luminance, video range: rint(2^20 x {255/219, 2 (1 - Kr) s, 2 Kb (1 - Kb) / Kg s,
 *                        2 Kr (1 - Kr) / Kg s, 2 (1 - Kb) s}), Kr = 0.2627, Kb = 0.0593, Kg = 1 - Kr - Kb, s = 255/224
 * available here for every layout and container, the 8-bit ones included.
 *
 * THE CALLS are whenet_yuv_to_bgr_host, whenet_op_yuv_to_bgr, whenet_frame_begin_yuv, whenet_clip_begin_yuv,
 * whenet_frame_begin_yuv_device, whenet_clip_begin_yuv_device and whenet_op_yuv_to_bgr_device of whenet_hip.h with
 * whenet_yuvx_frame_t in the place of whenet_yuv_frame_t: the same tickets, slots, stream order, size rules of a clip (one size: a
 * clip; otherwise a mixed clip of at most option "letterbox_cache" frames) and device-pointer checks.  A frame that
 * whenet_yuv_frame_t can describe gives the bytes of the old call; a clip may mix old and new frames.  The kernels are
 * csrc/yuvx.hip.  WHENET_EINVAL, with the frame's index in whenet_last_error and before a slot is taken or anything is enqueued:
 * a NULL required plane, a pitch below the plane's row bytes, an unknown layout, container or matrix, a shift outside 0..8 or
 * non-zero with an 8-bit container, a packed layout with a 16-bit container, a side outside 1..8192, a frame count outside 1..16,
 * a 16-bit plane at an odd address or with an odd pitch.
 * Not built: Y210 / Y216 / v210 (packed 10-bit 4:2:2), NV16 / NV24, big-endian samples, HDR transfer functions (PQ / HLG tone
 * mapping: the bytes are the matrix's, nothing is tone-mapped), full-range variants of BT.709 / BT.2020, 10-bit DESTINATIONS of the
 * pose overlay. */
#ifndef WHENET_HIP_YUV_EXT_H
#define WHENET_HIP_YUV_EXT_H

#include "whenet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WHENET_YUVX_I444 16     /* a layout, beside WHENET_YUV_NV12 (0), _I420 (1), _YUYV (3), _UYVY (4) */
#define WHENET_YUVX_U8 8        /* containers: the bits of a stored sample */
#define WHENET_YUVX_U16 16
#define WHENET_YUVX_MAX_SHIFT 8
#define WHENET_YUV_BT2020 3
#define WHENET_YUVX_MATRICES 4
#define WHENET_YUVX_COEFFS {{16, 1220542, 1673527, 409993, 852492, 2116026}, \
                            {16, 1220945, 1879825, 223578, 558767, 2215014}, \
                            {0, 1048576, 1470104, 360853, 748826, 1858077}, \
                            {16, 1220945, 1760217, 196426, 682019, 2245811}}
typedef struct {
    const uint8_t* plane[3];
    int pitch[3];               /* bytes */
    int layout;
    int container;
    int shift;
    int matrix;
    int h, w;
} whenet_yuvx_frame_t;
WHENET_API int whenet_yuvx_to_bgr_host(const whenet_yuvx_frame_t* frame, uint8_t* bgr);
WHENET_API int whenet_op_yuvx_to_bgr(whenet_t* h, const whenet_yuvx_frame_t* frames, int num_frames, uint8_t* const* bgr);
WHENET_API int whenet_frame_begin_yuvx(whenet_t* h, const whenet_yuvx_frame_t* frame, int* ticket);
WHENET_API int whenet_clip_begin_yuvx(whenet_t* h, const whenet_yuvx_frame_t* frames, int num_frames, int* ticket);
WHENET_API int whenet_frame_begin_yuvx_device(whenet_t* h, const whenet_yuvx_frame_t* frame, void* stream, int* ticket);
WHENET_API int whenet_clip_begin_yuvx_device(whenet_t* h, const whenet_yuvx_frame_t* frames, int num_frames, void* stream, int* ticket);
WHENET_API int whenet_op_yuvx_to_bgr_device(whenet_t* h, const whenet_yuvx_frame_t* frames, int num_frames, void* stream, uint8_t* const* bgr);

#ifdef __cplusplus
}
#endif
#endif /* WHENET_HIP_YUV_EXT_H */
