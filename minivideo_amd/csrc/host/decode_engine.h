// decode_engine.h -- the pipelined whole-path decoder behind mvhp_engine_* (include/minivideo_hotpath.h) and
// minivideo_decode(): entropy threads -> page-locked chunks -> H2D -> batched reconstruction -> D2H -> sink.
//
// Replaces, as one pipeline, the reference's serial loop: NAL loop h264.c:76-188 -> decode_slice h264_slice.c:64-109
// -> macroblock loop h264_slice.c:1046-1139 -> export_idr export.c:618-767.
//
// The engine is plain C++ over a small table of device operations (DeviceApi: allocation, the two copies, and one operation
// that runs a whole batch from a descriptor, BatchJob), so that the threading can be built and
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

// Everything one batch runs on the device, in order, on the context's compute queue: compact pictures (`stride` bytes apart) ->
// packed records in d_packed (scratch) -> planes -> the passes the fields below ask for.
struct BatchJob {
    const mvhp_stream_params_t *params;
    const void *d_compact; size_t stride; void *d_packed; int n;
    uint8_t *d_yuv;   // n x planes of the coded size: always written (after the deblocking filter where params ask for it).  The
                      // output of a job with nothing below, the scratch every later pass reads otherwise
    uint8_t *d_rgb;   // fused RGB of the coded size, or NULL.  Only without a resample pass and without JPEG: those reconstruct
                      // planes only, without the fused colour epilogue (with `png` and no pass in between it is the encoder's input)
    const mvhp_output_geometry_t *geom;   // of the n pictures; NULL: the coded size, nothing below but `stats` may be set
    uint8_t *out_yuv, *out_rgb;   // (turns 0) mvhp_resample_dev of d_yuv into n pictures of `geom`: planes and / or RGB (either may be NULL);
                                  // both NULL: no resample pass (only with `jpeg`: files of the coded size, geom names that size)
    int turns;          // quarter turns (1..3; 0: none, mid_yuv NULL).  `geom` is then the geometry DELIVERED (out_w / out_h exchanged for
    uint8_t *mid_yuv;   // odd turns) and out_yuv / out_rgb hold the turned pictures: mvhp_orient_dev straight from the crop rectangle
                        // of d_yuv where nothing scales (mid_yuv NULL), else mvhp_resample_dev of d_yuv into mid_yuv (planes of the
                        // geometry before the turn) and mvhp_orient_dev of those
    const mvhp_jpeg_params_t *jpeg;   // NULL: no encoder.  Else mvhp_jpeg_encode_dev of the n pictures of `geom` -- out_yuv where a
                                      // resample pass ran, else d_yuv -- into `blob` (blob_cap bytes) and `table` (n entries)
    const mvhp_png_params_t *png;     // NULL: no PNG encoder (never beside `jpeg`).  Else mvhp_png_encode_dev of the n pictures of
                                      // `geom` -- out_rgb where a pass behind the reconstruction wrote it, else the fused d_rgb --
                                      // into the same `blob` and `table`
    uint8_t *blob; size_t blob_cap; mvhp_jpeg_entry_t *table;
    const mvhp_color_params_t *color;   // NULL: RGB by the reference's formula, fused or inside the passes.  Else no pass and no
                                        // epilogue makes RGB: mvhp_color_dev of the FINAL planes -- out_yuv into out_rgb where a
                                        // pass behind the reconstruction ran (both set), else d_yuv into d_rgb with `geom` the coded
                                        // size -- and `png` reads that RGB.  Never beside `jpeg`
    mvhp_luma_stats_t *stats;   // NULL: no picture scores.  Else mvhp_luma_stats_dev over the crop rectangle of `geom` (the whole
                                // picture without one) on the n coded planes in d_yuv -> n records
    mvhp_luma_bars_t *bars;     // NULL: no black-bar probe.  Else mvhp_luma_bars_dev at `bars_level` over the same rectangle of the
    int bars_level;             // same planes -> n records (never beside `stats`, `jpeg` or `png`)
    mvhp_plane_hist_t *hist;    // NULL: no plane histograms.  Else mvhp_plane_hist_dev over the same rectangle of the same planes ->
                                // n records of 3104 bytes, 16-byte aligned (beside anything but `bars`)
    const mvhp_tensor_params_t *tensor;   // NULL: no tensors.  Else mvhp_tensor_dev of the n RGB pictures the job makes -- out_rgb where a
    void *tensor_out;                     // pass behind the reconstruction wrote it, else d_rgb; src_w x src_h is their size -- into
    const int32_t *slots_host;            // tensor_out (16-byte aligned).  slots_host NULL: picture i into slot i of tensor_out; else
    int32_t *d_slots;                     // n slot numbers in HOST memory (negative: the picture is skipped), which the job copies to
                                          // d_slots (device, n x 4 bytes) on its queue first.  Never beside `jpeg`, `png` or `bars`
};
struct BatchDone {
    float ms;            // device-side duration of the whole job, one bracketed interval
    int layout, waves;   // of the reconstruction launch
};

// what run_batch can do beyond pictures of the coded size; a job that needs a missing bit fails in the engine, with a message
enum : uint32_t { CAP_GEOMETRY = 1, CAP_JPEG = 2, CAP_SCORE = 4, CAP_ORIENT = 8, CAP_PNG = 16, CAP_COLOR = 32, CAP_BARS = 64, CAP_HIST = 128, CAP_TENSOR = 256 };

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
    int    (*run_batch)(DevCtx *c, const BatchJob &job, BatchDone &done, std::string &err);
    uint32_t caps;   // CAP_*
    // optional (may be NULL): `sets` x 4 batch buffers {compact, records, planes, RGB} inside one arena, records / planes / RGB
    // each in a group of the device's memory regions of its own (mvhp_placed_alloc_sets); ptrs[s * 4 + i]; nullptr = failed
    void  *(*placed_alloc)(DevCtx *c, int sets, const size_t bytes[4], void **ptrs);
    void   (*placed_free)(DevCtx *c, void *arena);
};

class Engine;

Engine *engine_create(const DeviceApi &api, const mvhp_engine_opts_t *opts, std::string &err);
void    engine_destroy(Engine *e);
void    engine_release_picture(Engine *e, int seq);
const mvhp_plane_hist_t *engine_picture_hist(Engine *e, int seq);   // mvhp_engine_picture_hist (include/minivideo_hotpath.h)
// mvhp_engine_set_tensor (include/minivideo_hotpath.h): t NULL clears; a malformed request is refused with a message
int     engine_set_tensor(Engine *e, const mvhp_tensor_request_t *t, std::string &err);
int     engine_contexts(Engine *e);   // mvhp_engine_contexts
int     effective_cores();   // hardware threads cut down to the container's CPU quota
// one of sink / sink_ex (or neither); req NULL or flags 0: pictures of the coded size, the path without a geometry pass
int     engine_decode(Engine *e, const mvhp_stream &s, const int *order, int n_order, int wanted, int out_mask,
                      const mvhp_output_request_t *req, mvhp_picture_sink_t sink, mvhp_picture_sink_ex_t sink_ex, void *user,
                      mvhp_decode_stats_t *stats, std::string &err);

} // namespace mvengine

// the product's device table (HIP); defined in csrc/hip/hotpath_abi.hip
const mvengine::DeviceApi &mvhp_hip_device_api();
