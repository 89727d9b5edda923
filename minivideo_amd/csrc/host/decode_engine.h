// decode_engine.h -- the pipelined whole-path decoder behind mvhp_engine_* (include/minivideo_hotpath.h) and
// minivideo_decode(): entropy threads -> page-locked chunks -> H2D -> batched reconstruction -> D2H -> sink.
//
// Replaces, as one pipeline, the reference's serial loop: NAL loop h264.c:76-188 -> decode_slice h264_slice.c:64-109
// -> macroblock loop h264_slice.c:1046-1139 -> export_idr export.c:618-767.
//
// The engine is plain C++ over a small table of device operations (DeviceApi), so that the threading can be built and
// checked on a CPU-only box against a stub device (tools/engine_harness.cpp, tests/test_engine_harness.py: ThreadSanitizer + AddressSanitizer); the product's table is HIP
// (csrc/hip/hotpath_abi.hip) and there is no CPU implementation of it in the library.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "minivideo_hotpath.h"

struct mvhp_stream;

namespace mvengine {

struct DevCtx;   // one device context: a reconstruction context plus its upload / compute / download queues

// Every operation blocks its calling thread until the device has finished it; the engine runs one thread per queue
// and context, which is what overlaps upload(k+1), kernel(k) and download(k-1).  *ms = device-side duration.
struct DeviceApi {
    int    (*device_count)();
    void  *(*host_alloc)(size_t bytes);           // page-locked
    void   (*host_free)(void *p);
    DevCtx *(*ctx_create)(int device, std::string &err);
    void   (*ctx_destroy)(DevCtx *c);
    void  *(*dev_alloc)(DevCtx *c, size_t bytes);
    void   (*dev_free)(DevCtx *c, void *p);
    size_t (*dev_free_bytes)(DevCtx *c);
    // n pieces in one go (one piece per picture: compact pictures have individual sizes)
    int    (*h2d)(DevCtx *c, int n, void *const *d_dst, const void *const *h_src, const size_t *bytes, float *ms, std::string &err);
    // n pieces in one go (the planes and the RGB of an output chunk: one wait instead of two)
    int    (*d2h)(DevCtx *c, int n, void *const *h_dst, const void *const *d_src, const size_t *bytes, float *ms, std::string &err);
    // compact pictures (`stride` bytes apart) -> packed records in d_packed (scratch) -> planes (+ RGB)
    int    (*recon)(DevCtx *c, const mvhp_stream_params_t *p, const void *d_compact, size_t stride, void *d_packed,
                    int n_pictures, uint8_t *d_yuv, uint8_t *d_rgb, float *ms, int *layout, int *waves, std::string &err);
    // optional (may be NULL): `sets` x 4 batch buffers {compact, records, planes, RGB} inside one arena, records / planes / RGB
    // each in a group of the device's memory regions of its own (mvhp_placed_alloc_sets); ptrs[s * 4 + i]; nullptr = failed
    void  *(*placed_alloc)(DevCtx *c, int sets, const size_t bytes[4], void **ptrs);
    void   (*placed_free)(DevCtx *c, void *arena);
    // optional (may be NULL: a batch with an output geometry then fails), last so that a positional initialiser of the
    // operations above still compiles: `recon` without its fused colour epilogue into d_yuv_coded (scratch: planes of the coded
    // size), the deblocking filter when p asks for it, then mvhp_resample_dev into n pictures of geometry g -- planes into
    // d_yuv_out and / or RGB into d_rgb_out (either may be NULL)
    int    (*recon_geometry)(DevCtx *c, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g, const void *d_compact,
                             size_t stride, void *d_packed, int n_pictures, uint8_t *d_yuv_coded, uint8_t *d_yuv_out,
                             uint8_t *d_rgb_out, float *ms, int *layout, int *waves, std::string &err);
    // optional (may be NULL: a call with MVHP_OUT_JPEG then fails), last for the same reason: `recon` planes only into d_yuv_coded,
    // the deblocking filter when p asks for it, mvhp_resample_dev into d_yuv_out when `resample` (g then differs from the coded
    // size; otherwise d_yuv_out is NULL), then mvhp_jpeg_encode_dev of the n pictures of geometry g into d_blob (cap_bytes) and
    // d_table (n entries)
    int    (*recon_jpeg)(DevCtx *c, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g, int resample,
                         const mvhp_jpeg_params_t *jp, const void *d_compact, size_t stride, void *d_packed, int n_pictures,
                         uint8_t *d_yuv_coded, uint8_t *d_yuv_out, uint8_t *d_blob, size_t cap_bytes, mvhp_jpeg_entry_t *d_table,
                         float *ms, int *layout, int *waves, std::string &err);
    // optional (may be NULL: a call with MVHP_OUTPUT_SCORE then fails), last for the same reason: mvhp_luma_stats_dev over the crop
    // rectangle of g on the n coded planes that recon / recon_geometry / recon_jpeg left in d_yuv_coded (after the deblocking
    // filter, where p asks for it) -> n records in d_stats; *ms = its device-side duration
    int    (*luma_stats)(DevCtx *c, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g, const uint8_t *d_yuv_coded,
                         int n_pictures, mvhp_luma_stats_t *d_stats, float *ms, std::string &err);
};

class Engine;

Engine *engine_create(const DeviceApi &api, const mvhp_engine_opts_t *opts, std::string &err);
void    engine_destroy(Engine *e);
void    engine_release_picture(Engine *e, int seq);
int     effective_cores();   // hardware threads cut down to the container's CPU quota
// one of sink / sink_ex (or neither); req NULL or flags 0: pictures of the coded size, the path without a geometry pass
int     engine_decode(Engine *e, const mvhp_stream &s, const int *order, int n_order, int wanted, int out_mask,
                      const mvhp_output_request_t *req, mvhp_picture_sink_t sink, mvhp_picture_sink_ex_t sink_ex, void *user,
                      mvhp_decode_stats_t *stats, std::string &err);

} // namespace mvengine

// the product's device table (HIP); defined in csrc/hip/hotpath_abi.hip
const mvengine::DeviceApi &mvhp_hip_device_api();
