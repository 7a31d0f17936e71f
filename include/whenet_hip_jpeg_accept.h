/* The JPEG decoder's accept bits: the ten entry points of the section JPEG DECODER, LAYOUTS of whenet_hip.h -- 4:4:0 / 4:1:1 / 4:1:0
 * streams, sequential frames of several scans, scans of two components, SOF1 -- in a header of their own.  The contract, the
 * arguments and the option "jpeg_layouts" are stated there; this file declares.  The same library exports them; the ABI is
 * whenet_hip.h's (6), and whenet_jpeg_info_t / whenet_jpeg_scan_t keep their layout.  A caller who does not include this header
 * sees the interface whenet_hip.h had before the section. */
#ifndef WHENET_HIP_JPEG_ACCEPT_H
#define WHENET_HIP_JPEG_ACCEPT_H

#include "whenet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the bits of `accept` (a clip: 0..3; the single-stream handle calls also -1, the handle's options "jpeg_progressive" / "jpeg_layouts") */
#define WHENET_JPEG_ACCEPT_PROGRESSIVE 1
#define WHENET_JPEG_ACCEPT_LAYOUTS 2

WHENET_API int whenet_jpeg_parse_scans_accept(const uint8_t* data, int64_t size, int accept, whenet_jpeg_info_t* info, whenet_jpeg_scan_t* scans,
                                              int cap, int* num_scans);
WHENET_API int whenet_jpeg_decode_accept_host(const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order, int rule,
                                              int accept, int orient, int32_t status[2], int32_t* orientation);
WHENET_API int whenet_jpeg_decode_accept_planes_host(const uint8_t* data, int64_t size, uint8_t* const* planes, const int* pitch, int rule,
                                                     int accept, int32_t status[2]);
WHENET_API int whenet_jpeg_decode_segmented_accept_host(const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order,
                                                        int seg_bytes, int window, int rule, int accept, int32_t status[2], int64_t stats[8]);
WHENET_API int whenet_jpeg_decode_segmented_accept_planes_host(const uint8_t* data, int64_t size, uint8_t* const* planes, const int* pitch,
                                                               int seg_bytes, int window, int rule, int accept, int32_t status[2],
                                                               int64_t stats[8]);
WHENET_API int whenet_op_jpeg_decode_accept(whenet_t* h, const uint8_t* data, int64_t size, const whenet_surface_t* dst, int channel_order,
                                            int entropy, int seg_bytes, int rule, int accept, int orient, int32_t status[2], int64_t stats[8],
                                            int32_t* orientation);
WHENET_API int whenet_op_jpeg_decode_clip_accept(whenet_t* h, const uint8_t* const* data, const int64_t* size, int num_frames,
                                                 const whenet_surface_t* dst, int channel_order, int32_t* status, int entropy, int seg_bytes,
                                                 int rule, int accept, int orient, int32_t* orientation);
WHENET_API int whenet_frame_begin_jpeg_accept(whenet_t* h, const uint8_t* data, int64_t size, int channel_order, int rule, int accept, int orient,
                                              int* ticket, int32_t* status, int32_t* orientation);
WHENET_API int whenet_clip_begin_jpeg_accept(whenet_t* h, const uint8_t* const* data, const int64_t* size, int num_frames, int channel_order,
                                             int rule, int accept, int orient, int* ticket, int32_t* status, int32_t* orientation);
WHENET_API int whenet_jpeg_clip_plan_accept(const uint8_t* const* data, const int64_t* size, int num_frames, int entropy, int seg_bytes,
                                            int accept, int64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* WHENET_HIP_JPEG_ACCEPT_H */
