// engine_harness.cpp -- the decode engine's threading, built WITHOUT HIP against a stub device table, so that it can
// run under ThreadSanitizer on a CPU-only box (tests/test_engine_harness.py).  TEST INFRASTRUCTURE: the stub "device"
// does no reconstruction -- it stamps every output picture with a checksum of the packed records it was handed, which
// lets the sink check that the right picture arrives in the right place, in order, through chunks, batches, several
// contexts and a re-queue.  Nothing here is part of libminivideo.so.
//
// usage: engine_harness <stream.264> [<stream with a broken picture> <its index> [<stream whose SPS crop changes> [jpeg | png | score | bars | hist | tensor | orient | color <stream whose SPS VUI changes>]]]
// The fourth argument adds the geometry mode: mvhp_engine_decode_ex and minivideo_decode under MINIVIDEO_CROP /
// MINIVIDEO_THUMBNAIL against the stub's resample targets.  A fifth argument adds the JPEG mode (MVHP_OUT_JPEG), the PNG mode (MVHP_OUT_PNG against the stub's PNG operation) or the
// score mode (MVHP_OUTPUT_SCORE against the stub's picture scores, which sum the stub's coded planes on the CPU), or the orient
// mode (MVHP_OUTPUT_ORIENT / MVHP_OUTPUT_ROTATE and MINIVIDEO_ROTATE against the stub's turn), or the color mode (MVHP_OUTPUT_ASPECT /
// MVHP_OUTPUT_COLOR, MINIVIDEO_ASPECT and MINIVIDEO_COLOR against the stub's colour pass; a sixth argument names a stream whose
// SPSs alternate between two VUIs that differ in matrix and range only, so that the colour setting changes and no geometry does),
// or the tensor mode (MVHP_OUT_TENSOR and mvhp_engine_set_tensor against the stub's tensor operation: host delivery, and device
// delivery into a stand-in target in host memory).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "blank_policy.h"
#include "decode_engine.h"
#include "png_format.h"
#include "represent_policy.h"
#include "tensor_policy.h"
#include "minivideo.h"
#include "stream_internal.h"

// ---- the pieces of the C-ABI the engine uses that live in the HIP translation unit of the product ----
extern "C" {
size_t mvhp_packed_frame_bytes(const mvhp_stream_params_t *p) { return p ? (size_t)p->width_mbs * p->height_mbs * MVHP_MB_BYTES : 0; }
size_t mvhp_yuv_frame_bytes(const mvhp_stream_params_t *p) { return p ? (size_t)p->width_mbs * p->height_mbs * 384 : 0; }
size_t mvhp_rgb_frame_bytes(const mvhp_stream_params_t *p) { return p ? (size_t)p->width_mbs * p->height_mbs * 768 : 0; }
int mvhp_device_count(void) { return 1; }
}

namespace mvengine {
struct DevCtx {
    int device;
};
} // namespace mvengine

namespace {

using mvengine::DevCtx;

std::atomic<int> g_recon_calls{0}, g_live_ctx{0}, g_geometry_calls{0}, g_ctx_created{0};
std::atomic<long> g_dev_allocs{0};
int g_devices = 2;
std::atomic<int> g_slow_host_alloc_us{0};   // page-locking is slow on a real box: the feeder drops its lock around it

uint64_t checksum(const uint8_t *p, size_t n)
{
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}

int stub_device_count() { return g_devices; }
void *stub_host_alloc(size_t n)
{
    if (g_slow_host_alloc_us > 0) std::this_thread::sleep_for(std::chrono::microseconds(g_slow_host_alloc_us.load()));
    return malloc(n ? n : 1);
}
void stub_host_free(void *p) { free(p); }
DevCtx *stub_ctx_create(int device, std::string &) { g_live_ctx++; g_ctx_created++; return new DevCtx{device}; }
void stub_ctx_destroy(DevCtx *c) { g_live_ctx--; delete c; }
void *stub_dev_alloc(DevCtx *, size_t n) { g_dev_allocs++; return malloc(n ? n : 1); }
void stub_dev_free(DevCtx *, void *p) { g_dev_allocs--; free(p); }
size_t stub_dev_free_bytes(DevCtx *) { return (size_t)1 << 32; }
int stub_copy_n(DevCtx *, int n, void *const *dst, const void *const *src, const size_t *bytes, float *ms, std::string &)
{
    for (int i = 0; i < n; i++) memcpy(dst[i], src[i], bytes[i]);
    std::this_thread::sleep_for(std::chrono::microseconds(50));
    if (ms) *ms = 0.05f;
    return MVHP_SUCCESS;
}
// compact picture -> packed records (the CPU restatement of csrc/hip/expand_compact.hip, for this harness only)
void expand_compact(const uint8_t *pic, size_t mbs, uint8_t *packed)
{
    const uint32_t *off = reinterpret_cast<const uint32_t *>(pic);
    for (size_t mb = 0; mb < mbs; mb++) {
        const uint8_t *rec = pic + mbs * 4 + off[mb];
        uint8_t *out = packed + mb * MVHP_MB_BYTES;
        memset(out, 0, MVHP_MB_BYTES);
        memcpy(out, rec, MVHP_MB_HEADER_BYTES);
        uint32_t n;
        memcpy(&n, rec + 28, 4);
        const bool dense = (rec[5] & 1) != 0;
        out[5] = 0;
        memset(out + 28, 0, 4);
        if (dense) { memcpy(out + MVHP_MB_HEADER_BYTES, rec + MVHP_MB_HEADER_BYTES, MVHP_MB_COEFS * 2); continue; }
        int16_t *coef = reinterpret_cast<int16_t *>(out + MVHP_MB_HEADER_BYTES);
        for (uint32_t i = 0; i < n; i++) {
            uint32_t e;
            memcpy(&e, rec + MVHP_MB_HEADER_BYTES + 4 * i, 4);
            if ((e & 0xffffu) < (uint32_t)MVHP_MB_COEFS) coef[e & 0xffffu] = (int16_t)(e >> 16);
        }
    }
}
// The coded planes a job with a geometry or JPEG leaves behind: 0x11, the luma plane filled with the eight bytes of the records'
// checksum over and over, so that every rectangle of it sums to something that depends on the picture (score mode).  The planes of
// a job of the coded size are its output: 0x5a with the checksum in bytes 0-7.
uint8_t coded_luma(uint64_t h, bool pattern, size_t j) { return pattern ? (uint8_t)(h >> (8 * (j & 7))) : j < 8 ? (uint8_t)(h >> (8 * j)) : 0x5a; }
void fill_coded(uint8_t *pic, size_t yb, uint64_t h)
{
    memset(pic, 0x11, yb);
    for (size_t j = 0; j < yb / 3 * 2; j++) pic[j] = coded_luma(h, true, j);
}
mvhp_luma_stats_t expected_stats(uint64_t h, bool pattern, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g)
{
    mvhp_luma_stats_t st{};
    const size_t Wp = (size_t)p->width_mbs * 16;
    for (uint32_t y = g->crop_y; y < g->crop_y + g->crop_h; y++)
        for (uint32_t x = g->crop_x; x < g->crop_x + g->crop_w; x++) {
            const uint64_t v = coded_luma(h, pattern, (size_t)y * Wp + x);
            st.sum += v;
            st.sumsq += v * v;
        }
    st.samples = g->crop_w * g->crop_h;
    return st;
}

// The box the stub's black-bar operation reports for a picture (bars mode): inside the rectangle, a function of the records'
// checksum, so that every picture has its own; every seventh checksum gives the empty box.
mvhp_luma_bars_t expected_bars(uint64_t h, const mvhp_output_geometry_t *g)
{
    mvhp_luma_bars_t b{};
    const uint32_t cw = g->crop_w, ch = g->crop_h;
    if (h % 7 == 0 || cw < 2 || ch < 2) return b;
    const uint32_t ox = (uint32_t)(h % (cw / 2)), oy = (uint32_t)((h >> 8) % (ch / 2));
    b.x = g->crop_x + ox;
    b.y = g->crop_y + oy;
    b.w = cw - ox - (uint32_t)((h >> 16) % ((cw - ox + 1) / 2));
    b.h = ch - oy - (uint32_t)((h >> 24) % ((ch - oy + 1) / 2));
    b.rows = b.h;
    b.cols = b.w;
    return b;
}

// The histograms the stub's plane-histogram operation counts (hist mode): honest counts over the rectangle of the coded planes the
// batch buffer holds -- the luma as coded_luma() says, both chroma planes one value (0x11 under the pattern, else 0x5a).
mvhp_plane_hist_t expected_hist(uint64_t h, bool pattern, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g)
{
    mvhp_plane_hist_t r{};
    const size_t Wp = (size_t)p->width_mbs * 16;
    for (uint32_t y = g->crop_y; y < g->crop_y + g->crop_h; y++)
        for (uint32_t x = g->crop_x; x < g->crop_x + g->crop_w; x++) r.y[coded_luma(h, pattern, (size_t)y * Wp + x)]++;
    r.samples = g->crop_w * g->crop_h;
    r.chroma_samples = (g->crop_w / 2) * (g->crop_h / 2);
    r.cb[pattern ? 0x11 : 0x5a] = r.cr[pattern ? 0x11 : 0x5a] = r.chroma_samples;
    return r;
}

// The one batch operation.  Every job expands its pictures and leaves coded planes; then, as the descriptor asks:
// * nothing more (pictures of the coded size): the planes are the output, 0x5a with the checksum of the records in bytes 0-7; RGB
//   0xa5 with the checksum in bytes 8-15;
// * resample targets: the coded planes are written in full (the scratch buffer must hold them), every output picture is filled up
//   to its last byte (the output buffers must hold n pictures of the geometry) and stamped: planes 0x5a, checksum of the records in
//   bytes 0-7, 0x77 in the last byte; RGB 0xa5, the checksum in bytes 8-15, 0x78 last;
// * JPEG: the coded planes (and the output planes of a batch with a resample pass) are written in full, and every picture gets a
//   "file" whose length depends on its records -- 32 + checksum % (half the raw picture) bytes of 0x3c, the checksum in bytes 0-7,
//   0x79 last -- at the next multiple of 16 of the blob; a picture whose checksum is a multiple of 5 is reported too big;
// * turns (orient mode): the outputs are stamped as resample targets are -- `geom` is the delivered geometry, so the output buffers
//   must hold n pictures of it -- and a batch that scales before the turn must bring the buffer of the unturned planes, which is
//   written in full, and no other batch may bring one;
// * colour (color mode): no other pass may have been asked for RGB; the RGB -- out_rgb behind a pass, where the planes out_yuv must
//   be there to read, else d_rgb of the coded size -- is stamped as above, with the setting in byte 16 (0xc0 | matrix << 3 |
//   full_range << 2 | siting) and 0x7b last; planes of the coded size stay the output they are without the pass;
// * scores: honest sums over the rectangle of the coded planes the batch buffer holds.
// * black bars (bars mode): never beside scores, JPEG or PNG; the level must be 1 .. 254 and is remembered; every picture gets
//   expected_bars() of its records over the rectangle of the geometry (the coded picture without one).
// * plane histograms (hist mode): never beside black bars; honest counts over the rectangle of the three coded planes the batch
//   buffer holds, into records that must be 16-byte aligned.
// * PNG: the RGB the encoder reads is stamped as above (the fused RGB of a batch of the coded size, the resample or turn target
//   otherwise; no output planes), and every picture gets a "file" of 64 + checksum % (the longest file - 64) bytes of 0x3d that
//   starts with bytes 8-15 of that RGB (the checksum) and ends in 0x7a; the blob must be n x the longest file rounded to 16, so
//   no picture is too big.
// * tensors (tensor mode): never beside JPEG, PNG or black bars; the RGB the operation reads must be there (the fused RGB of a batch
//   of the coded size, a pass's target otherwise) and src_w x src_h must be its size; a host slot table must come with its device
//   twin, to which it is copied first; every picture whose slot is not negative gets a "tensor" of mvhp_tensor_bytes at that
//   slot of tensor_out: 0x3e, bytes 8-15 of that RGB (the checksum) in bytes 0-7, tensor_tag() in byte 8, 0x7c last.
constexpr uint8_t kLastTensor = 0x7c;
std::atomic<int> g_tensor_calls{0};
uint8_t tensor_tag(const mvhp_tensor_params_t &t) { return (uint8_t)(0x80 | t.dtype << 4 | t.layout << 1 | (t.flags & 1)); }
constexpr uint8_t kLastYuv = 0x77, kLastRgb = 0x78, kLastJpeg = 0x79, kLastPng = 0x7a, kLastColor = 0x7b;
std::atomic<int> g_jpeg_calls{0}, g_stats_calls{0}, g_orient_calls{0}, g_mid_calls{0}, g_png_calls{0}, g_color_calls{0};
std::atomic<int> g_bars_calls{0}, g_bars_level{0}, g_hist_calls{0};
std::atomic<uint32_t> g_watch_crop[4];   // bars mode: launches whose geometry has this crop rectangle are counted
std::atomic<int> g_watch_hits{0};
uint8_t color_tag(const mvhp_color_params_t &c) { return (uint8_t)(0xc0 | (c.matrix << 3) | (c.full_range << 2) | c.siting); }
size_t stub_png_room(const mvhp_output_geometry_t *g) { return (mvhp::png_max_bytes((int)g->out_w, (int)g->out_h) + 15) & ~(size_t)15; }
size_t stub_png_length(uint64_t h, const mvhp_output_geometry_t *g) { return 64 + (size_t)(h % (mvhp::png_max_bytes((int)g->out_w, (int)g->out_h) - 64)); }
size_t stub_jpeg_length(uint64_t h, size_t raw) { return 32 + (size_t)(h % (raw / 2)); }
bool stub_jpeg_too_big(uint64_t h) { return h % 5 == 0; }
int stub_run_batch(DevCtx *, const mvengine::BatchJob &j, mvengine::BatchDone &done, std::string &err)
{
    const mvhp_stream_params_t *p = j.params;
    const mvhp_output_geometry_t *g = j.geom;
    const bool resample = j.out_yuv || j.out_rgb;
    (j.jpeg ? g_jpeg_calls : j.png ? g_png_calls : resample ? g_geometry_calls : g_recon_calls)++;
    if (!j.d_yuv || (!j.jpeg && !j.png && !j.color && (g != nullptr) != resample)) { err = "stub: geometry launch without buffers"; return MVHP_FAILURE; }
    if (j.color) {
        if (!g || j.jpeg || (resample ? (!j.out_yuv || !j.out_rgb) : !j.d_rgb) || j.color->reserved || j.color->matrix < 0 || j.color->matrix > 1 ||
            j.color->full_range < 0 || j.color->full_range > 1 || j.color->siting < 1 || j.color->siting > 2) {
            err = "stub: colour pass without buffers or parameters";
            return MVHP_FAILURE;
        }
        g_color_calls++;
    }
    const bool coded_out = !g || (j.color && !resample && !j.png);   // the planes of the coded size are what is delivered
    if (j.turns < 0 || j.turns > 3 || (!j.turns && j.mid_yuv) || (j.turns && (!g || !resample))) { err = "stub: orientation without buffers"; return MVHP_FAILURE; }
    if (j.turns) {
        const uint32_t w0 = (j.turns & 1) ? g->out_h : g->out_w, h0 = (j.turns & 1) ? g->out_w : g->out_h;   // before the turn
        if ((j.mid_yuv != nullptr) != (w0 != g->crop_w || h0 != g->crop_h)) { err = "stub: the unturned planes exactly where the batch scales"; return MVHP_FAILURE; }
        if (j.mid_yuv) { memset(j.mid_yuv, 0x13, (size_t)j.n * mvhp_geometry_yuv_bytes(g)); g_mid_calls++; }
        g_orient_calls++;
    }
    // (JPEG: a resample pass exactly where the pictures are not of the coded size)
    if (j.jpeg && (!g || !j.blob || !j.table || j.out_rgb || j.jpeg->quality < 1 || j.jpeg->quality > 100 ||
                   (j.out_yuv != nullptr) != (j.turns != 0 || g->out_w != p->width_mbs * 16 || g->out_h != p->height_mbs * 16))) {
        err = "stub: JPEG launch without buffers or parameters";
        return MVHP_FAILURE;
    }
    // (PNG: RGB present -- fused where the pictures are of the coded size, a pass's target exactly where they are not -- no planes)
    if (j.png && (!g || j.jpeg || !j.blob || !j.table || (j.out_yuv && !j.color) || j.png->reserved || !(resample ? j.out_rgb : j.d_rgb) ||
                  (j.out_rgb != nullptr) != (j.turns != 0 || g->out_w != p->width_mbs * 16 || g->out_h != p->height_mbs * 16))) {
        err = "stub: PNG launch without buffers or parameters";
        return MVHP_FAILURE;
    }
    if (j.png && j.blob_cap != (size_t)j.n * stub_png_room(g)) { err = "stub: the blob is not n longest files long"; return MVHP_FAILURE; }
    const int n = j.n;
    const size_t pb = mvhp_packed_frame_bytes(p), yb = mvhp_yuv_frame_bytes(p), rb = mvhp_rgb_frame_bytes(p);
    const size_t gy = mvhp_geometry_yuv_bytes(g), gr = mvhp_geometry_rgb_bytes(g);
    if (j.jpeg && j.blob_cap != (size_t)n * gy) { err = "stub: the blob is not n raw pictures long"; return MVHP_FAILURE; }
    mvhp_output_geometry_t rect{};   // of the scores: the crop of the geometry, the coded picture without one
    rect.crop_w = p->width_mbs * 16;
    rect.crop_h = p->height_mbs * 16;
    if (g) rect = *g;
    if (j.stats && (n <= 0 || rect.crop_w == 0 || rect.crop_h == 0 || rect.crop_x + rect.crop_w > p->width_mbs * 16 ||
                    rect.crop_y + rect.crop_h > p->height_mbs * 16)) { err = "stub: picture-score launch without buffers or rectangle"; return MVHP_FAILURE; }
    if (j.bars && (j.stats || j.jpeg || j.png || j.bars_level < 1 || j.bars_level > 254 || n <= 0 || rect.crop_w == 0 || rect.crop_h == 0 ||
                   rect.crop_x + rect.crop_w > p->width_mbs * 16 || rect.crop_y + rect.crop_h > p->height_mbs * 16)) {
        err = "stub: black-bar launch without buffers, level or rectangle";
        return MVHP_FAILURE;
    }
    if (j.hist && (j.bars || ((uintptr_t)j.hist & 15) || n <= 0 || rect.crop_w < 2 || rect.crop_h < 2 || ((rect.crop_x | rect.crop_y | rect.crop_w | rect.crop_h) & 1) ||
                   rect.crop_x + rect.crop_w > p->width_mbs * 16 || rect.crop_y + rect.crop_h > p->height_mbs * 16)) {
        err = "stub: plane-histogram launch without buffers or rectangle";
        return MVHP_FAILURE;
    }
    if (j.tensor) {
        const uint32_t sw = g ? g->out_w : p->width_mbs * 16, sh = g ? g->out_h : p->height_mbs * 16;
        if (j.jpeg || j.png || j.bars || !j.tensor_out || ((uintptr_t)j.tensor_out & 15) || !(resample ? j.out_rgb : j.d_rgb) || j.tensor->src_w != sw ||
            j.tensor->src_h != sh || !mvtensor::bytes(*j.tensor) || !mvtensor::finite(*j.tensor) || (j.slots_host != nullptr) != (j.d_slots != nullptr)) {
            err = "stub: tensor launch without buffers or parameters";
            return MVHP_FAILURE;
        }
    }
    if (g && g->crop_x == g_watch_crop[0] && g->crop_y == g_watch_crop[1] && g->crop_w == g_watch_crop[2] && g->crop_h == g_watch_crop[3]) g_watch_hits++;
    for (int i = 0; i < n; i++)
        expand_compact((const uint8_t *)j.d_compact + (size_t)i * j.stride, (size_t)p->width_mbs * p->height_mbs, (uint8_t *)j.d_packed + (size_t)i * pb);
    if (j.jpeg && j.out_yuv) memset(j.out_yuv, 0x12, (size_t)n * gy);
    size_t pos = 0;
    for (int i = 0; i < n; i++) {
        const uint64_t h = checksum((const uint8_t *)j.d_packed + (size_t)i * pb, pb);
        uint8_t *coded = j.d_yuv + (size_t)i * yb;
        if (!coded_out) fill_coded(coded, yb, h);
        else {
            memset(coded, 0x5a, yb);
            memcpy(coded, &h, sizeof(h));
        }
        if (j.d_rgb && (!g || j.png || (j.color && !resample))) {
            memset(j.d_rgb + (size_t)i * rb, 0xa5, rb);
            memcpy(j.d_rgb + (size_t)i * rb + 8, &h, sizeof(h));
        }
        if (j.out_yuv && !j.jpeg) {
            memset(j.out_yuv + (size_t)i * gy, 0x5a, gy);
            memcpy(j.out_yuv + (size_t)i * gy, &h, sizeof(h));
            j.out_yuv[(size_t)i * gy + gy - 1] = kLastYuv;
        }
        if (j.out_rgb) {
            memset(j.out_rgb + (size_t)i * gr, 0xa5, gr);
            memcpy(j.out_rgb + (size_t)i * gr + 8, &h, sizeof(h));
            j.out_rgb[(size_t)i * gr + gr - 1] = kLastRgb;
        }
        if (j.color) {
            uint8_t *rgb = resample ? j.out_rgb + (size_t)i * gr : j.d_rgb + (size_t)i * rb;
            rgb[16] = color_tag(*j.color);
            rgb[(resample ? gr : rb) - 1] = kLastColor;
        }
        if (j.jpeg) {
            const size_t len = stub_jpeg_length(h, gy);
            mvhp_jpeg_entry_t e{pos, 0, MVHP_JPEG_TOO_BIG};
            if (!stub_jpeg_too_big(h) && pos + len <= j.blob_cap) {
                memset(j.blob + pos, 0x3c, len);
                memcpy(j.blob + pos, &h, sizeof(h));
                j.blob[pos + len - 1] = kLastJpeg;
                e.length = (uint32_t)len;
                e.status = MVHP_JPEG_OK;
                pos = (pos + len + 15) & ~(size_t)15;
            }
            j.table[i] = e;
        }
        if (j.png) {
            const uint8_t *src = resample ? j.out_rgb + (size_t)i * gr : j.d_rgb + (size_t)i * rb;
            const size_t len = stub_png_length(h, g);
            memset(j.blob + pos, 0x3d, len);
            memcpy(j.blob + pos, src + 8, 8);
            j.blob[pos + len - 1] = kLastPng;
            j.table[i] = mvhp_jpeg_entry_t{pos, (uint32_t)len, MVHP_PNG_OK};
            pos = (pos + len + 15) & ~(size_t)15;
        }
        if (j.stats) {
            mvhp_luma_stats_t st{};
            const size_t Wp = (size_t)p->width_mbs * 16;
            for (uint32_t y = rect.crop_y; y < rect.crop_y + rect.crop_h; y++)
                for (uint32_t x = rect.crop_x; x < rect.crop_x + rect.crop_w; x++) {
                    const uint64_t v = coded[(size_t)y * Wp + x];
                    st.sum += v;
                    st.sumsq += v * v;
                }
            st.samples = rect.crop_w * rect.crop_h;
            j.stats[i] = st;
        }
        if (j.bars) j.bars[i] = expected_bars(h, &rect);
        if (j.tensor) {
            if (i == 0 && j.slots_host) memcpy(j.d_slots, j.slots_host, (size_t)n * sizeof(int32_t));
            const int32_t slot = j.d_slots ? j.d_slots[i] : i;
            if (slot >= 0) {
                const size_t tb = mvtensor::bytes(*j.tensor);
                const uint8_t *src = resample ? j.out_rgb + (size_t)i * gr : j.d_rgb + (size_t)i * rb;
                uint8_t *t = (uint8_t *)j.tensor_out + (size_t)slot * tb;
                memset(t, 0x3e, tb);
                memcpy(t, src + 8, 8);
                t[8] = tensor_tag(*j.tensor);
                t[tb - 1] = kLastTensor;
            }
        }
        if (j.hist) {
            mvhp_plane_hist_t r{};
            const size_t Wp = (size_t)p->width_mbs * 16, Hp = (size_t)p->height_mbs * 16;
            const uint8_t *cb = coded + Wp * Hp, *cr = cb + Wp * Hp / 4;
            for (uint32_t y = rect.crop_y; y < rect.crop_y + rect.crop_h; y++)
                for (uint32_t x = rect.crop_x; x < rect.crop_x + rect.crop_w; x++) r.y[coded[(size_t)y * Wp + x]]++;
            for (uint32_t y = rect.crop_y / 2; y < (rect.crop_y + rect.crop_h) / 2; y++)
                for (uint32_t x = rect.crop_x / 2; x < (rect.crop_x + rect.crop_w) / 2; x++) {
                    r.cb[cb[(size_t)y * (Wp / 2) + x]]++;
                    r.cr[cr[(size_t)y * (Wp / 2) + x]]++;
                }
            r.samples = rect.crop_w * rect.crop_h;
            r.chroma_samples = (rect.crop_w / 2) * (rect.crop_h / 2);
            j.hist[i] = r;
        }
    }
    std::this_thread::sleep_for(std::chrono::microseconds(200));
    done.ms = j.stats ? 0.25f : 0.2f;
    done.layout = MVHP_LAYOUT_ROWS;
    done.waves = 8;
    if (j.stats) g_stats_calls++;
    if (j.bars) { g_bars_calls++; g_bars_level = j.bars_level; }
    if (j.hist) g_hist_calls++;
    if (j.tensor) g_tensor_calls++;
    return MVHP_SUCCESS;
}

mvengine::DeviceApi g_stub = {stub_device_count, stub_host_alloc, stub_host_free, stub_ctx_create, stub_ctx_destroy,
                                    stub_dev_alloc, stub_dev_free, stub_dev_free_bytes, stub_copy_n, stub_copy_n, stub_run_batch,
                                    mvengine::CAP_GEOMETRY | mvengine::CAP_JPEG | mvengine::CAP_SCORE | mvengine::CAP_ORIENT | mvengine::CAP_PNG | mvengine::CAP_COLOR | mvengine::CAP_BARS | mvengine::CAP_HIST | mvengine::CAP_TENSOR,
                                    nullptr, nullptr};   // (no placed arena on the stub device)

uint64_t picture_checksum(const mvhp_stream &s, int idr)
{
    mvhp_stream_params_t p;
    if (mvhp_stream_params(&s, idr, &p) != MVHP_SUCCESS) return 0;
    std::vector<uint8_t> packed(mvhp_packed_frame_bytes(&p));
    std::string e;
    if (s.decode_packed(idr, packed.data(), packed.size(), e) != h264::RC_SUCCESS) return 0;
    return checksum(packed.data(), packed.size());
}

// sink of the geometry mode: the right picture, in order, with the geometry mvhp_output_geometry gives for it and buffers that
// reach to the last byte of that geometry (pictures of the coded size are the stub's coded planes: no end mark)
struct CheckG {
    const mvhp_stream *s = nullptr;
    mvhp_output_request_t req{};
    bool want_yuv = true, want_rgb = false;
    int calls = 0, ok = 0, failed = 0, bad = 0, next_seq = 0, with_geometry = 0;
    std::vector<int> order;
    static int sink(void *user, int seq, int idr, int rc, const char *err, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g,
                    const uint8_t *yuv, const uint8_t *rgb)
    {
        CheckG &c = *static_cast<CheckG *>(user);
        c.calls++;
        if (seq != c.next_seq || idr != c.order[(size_t)seq] || !g) c.bad++;
        c.next_seq = seq + 1;
        mvhp_output_geometry_t want;
        const bool formed = mvhp_output_geometry(c.s, idr, &c.req, &want) == MVHP_SUCCESS;
        if (rc != MVHP_SUCCESS) {
            c.failed++;
            if (!err || !*err || yuv || rgb || formed) c.bad++;   // (the only failures of this mode: a geometry that cannot be formed)
            return 0;
        }
        if (!formed || !g || memcmp(&want, g, sizeof(want)) != 0) { c.bad++; return 0; }
        const bool coded = g->crop_x == 0 && g->crop_y == 0 && g->out_w == p->width_mbs * 16 && g->out_h == p->height_mbs * 16 &&
                           g->crop_w == g->out_w && g->crop_h == g->out_h;
        if (!coded) c.with_geometry++;
        const uint64_t h = picture_checksum(*c.s, idr);
        const size_t gy = mvhp_geometry_yuv_bytes(g), gr = mvhp_geometry_rgb_bytes(g);
        uint64_t got = 0;
        if (c.want_yuv) {
            if (!yuv) { c.bad++; return 0; }
            memcpy(&got, yuv, 8);
            if (got != h || yuv[8] != 0x5a || yuv[gy - 1] != (coded ? 0x5a : kLastYuv)) c.bad++;
        } else if (yuv) c.bad++;
        if (c.want_rgb) {
            if (!rgb) { c.bad++; return 0; }
            memcpy(&got, rgb + 8, 8);
            if (got != h || rgb[0] != 0xa5 || rgb[gr - 1] != (coded ? 0xa5 : kLastRgb)) c.bad++;
        } else if (rgb) c.bad++;
        c.ok++;
        return 1;
    }
};

// sink of the orient mode: the geometry is the one mvhp_output_geometry announces for the request (the turned one), the buffers are
// sized by it, and every picture of a call that turns went through a pass (the stub's last-byte stamps)
struct CheckO {
    const mvhp_stream *s = nullptr;
    mvhp_output_request_t req{};
    bool want_yuv = true, want_rgb = false;
    int calls = 0, ok = 0, failed = 0, bad = 0, next_seq = 0, no_op = 0;
    uint64_t bytes = 0;
    std::vector<int> order;
    static int sink(void *user, int seq, int idr, int rc, const char *err, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g,
                    const uint8_t *yuv, const uint8_t *rgb)
    {
        CheckO &c = *static_cast<CheckO *>(user);
        c.calls++;
        if (seq != c.next_seq || idr != c.order[(size_t)seq] || !g) c.bad++;
        c.next_seq = seq + 1;
        mvhp_output_geometry_t want;
        const bool formed = mvhp_output_geometry(c.s, idr, &c.req, &want) == MVHP_SUCCESS;
        if (rc != MVHP_SUCCESS) {
            c.failed++;
            if (err && strstr(err, "no orientation operation")) c.no_op++;
            else if (!err || !*err || yuv || rgb || formed) c.bad++;
            return 0;
        }
        if (!formed || !g || memcmp(&want, g, sizeof(want)) != 0) { c.bad++; return 0; }
        const int turns = mvhp_output_turns(c.s, &c.req);
        const bool coded = turns == 0 && g->crop_x == 0 && g->crop_y == 0 && g->out_w == p->width_mbs * 16 && g->out_h == p->height_mbs * 16 &&
                           g->crop_w == g->out_w && g->crop_h == g->out_h;
        const uint64_t h = picture_checksum(*c.s, idr);
        const size_t gy = mvhp_geometry_yuv_bytes(g), gr = mvhp_geometry_rgb_bytes(g);
        uint64_t got = 0;
        if (c.want_yuv) {
            if (!yuv) { c.bad++; return 0; }
            memcpy(&got, yuv, 8);
            if (got != h || yuv[8] != 0x5a || yuv[gy - 1] != (coded ? 0x5a : kLastYuv)) c.bad++;
            c.bytes += gy;
        } else if (yuv) c.bad++;
        if (c.want_rgb) {
            if (!rgb) { c.bad++; return 0; }
            memcpy(&got, rgb + 8, 8);
            if (got != h || rgb[0] != 0xa5 || rgb[gr - 1] != (coded ? 0xa5 : kLastRgb)) c.bad++;
            c.bytes += gr;
        } else if (rgb) c.bad++;
        c.ok++;
        return 1;
    }
};

// sink of the color mode: the geometry mvhp_output_geometry announces, buffers sized by it; with the colour flag in a call that
// delivers RGB the picture's RGB carries ITS OWN setting (mvhp_color_resolve of its display info under the request's mode, centred
// where the pass scaled) and the colour pass's end mark, the planes are what they are without the flag
struct CheckC {
    const mvhp_stream *s = nullptr;
    mvhp_output_request_t req{};
    bool want_yuv = true, want_rgb = false, png = false;
    int calls = 0, ok = 0, failed = 0, bad = 0, next_seq = 0, no_op = 0, settings_seen[16] = {0};
    uint64_t bytes = 0;
    std::vector<int> order;
    static uint8_t expected_tag(const mvhp_stream *s, int idr, const mvhp_output_request_t &req, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g)
    {
        mvhp_display_info_t d;
        mvhp_color_params_t c;
        const bool have = mvhp_stream_display(s, idr, &d) == MVHP_SUCCESS;
        mvhp_color_resolve(have ? &d : nullptr, p->width_mbs * 16, p->height_mbs * 16, (int)((req.flags & MVHP_OUTPUT_COLOR_MODE_MASK) >> MVHP_OUTPUT_COLOR_MODE_SHIFT), &c);
        const int turns = mvhp_output_turns(s, &req);
        const uint32_t w0 = (turns & 1) ? g->out_h : g->out_w, h0 = (turns & 1) ? g->out_w : g->out_h;
        if (w0 != g->crop_w || h0 != g->crop_h) c.siting = MVHP_CHROMA_CENTER;
        return color_tag(c);
    }
    static int sink(void *user, int seq, int idr, int rc, const char *err, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g,
                    const uint8_t *yuv, const uint8_t *rgb)
    {
        CheckC &c = *static_cast<CheckC *>(user);
        c.calls++;
        if (seq != c.next_seq || idr != c.order[(size_t)seq] || !g) c.bad++;
        c.next_seq = seq + 1;
        mvhp_output_geometry_t want;
        const bool formed = mvhp_output_geometry(c.s, idr, &c.req, &want) == MVHP_SUCCESS;
        if (rc != MVHP_SUCCESS) {
            c.failed++;
            if (err && strstr(err, "no colour operation")) c.no_op++;
            else if (!err || !*err || yuv || rgb || formed) c.bad++;
            return 0;
        }
        if (!formed || !g || want.crop_x != g->crop_x || want.crop_y != g->crop_y || want.crop_w != g->crop_w || want.crop_h != g->crop_h ||
            want.out_w != g->out_w || want.out_h != g->out_h) { c.bad++; return 0; }
        const int turns = mvhp_output_turns(c.s, &c.req);
        const bool coded = turns == 0 && g->crop_x == 0 && g->crop_y == 0 && g->out_w == p->width_mbs * 16 && g->out_h == p->height_mbs * 16 &&
                           g->crop_w == g->out_w && g->crop_h == g->out_h;
        const bool color = (c.req.flags & MVHP_OUTPUT_COLOR) != 0;
        const uint64_t h = picture_checksum(*c.s, idr);
        const size_t gy = mvhp_geometry_yuv_bytes(g), gr = mvhp_geometry_rgb_bytes(g);
        uint64_t got = 0;
        if (c.png) {   // the stub's file starts with bytes 8-15 of the RGB it was made of; its length is in reserved[0]
            if (yuv || !rgb || g->reserved[0] < 64) { c.bad++; return 0; }
            memcpy(&got, rgb, 8);
            if (got != h || rgb[g->reserved[0] - 1] != kLastPng) c.bad++;
            c.bytes += 16 + g->reserved[0];
            c.ok++;
            return 1;
        }
        if (c.want_yuv) {
            if (!yuv) { c.bad++; return 0; }
            memcpy(&got, yuv, 8);
            if (got != h || yuv[8] != 0x5a || yuv[gy - 1] != (coded ? 0x5a : kLastYuv)) c.bad++;
            c.bytes += gy;
        } else if (yuv) c.bad++;
        if (c.want_rgb) {
            if (!rgb) { c.bad++; return 0; }
            memcpy(&got, rgb + 8, 8);
            const uint8_t tag = color ? expected_tag(c.s, idr, c.req, p, g) : 0xa5;
            if (got != h || rgb[0] != 0xa5 || rgb[16] != tag || rgb[gr - 1] != (color ? kLastColor : coded ? 0xa5 : kLastRgb)) c.bad++;
            if (color) c.settings_seen[tag & 15]++;
            c.bytes += gr;
        } else if (rgb) c.bad++;
        c.ok++;
        return 1;
    }
};

// sink of the JPEG mode: no planes, the stub's file of the right picture in `rgb`, its length in g->reserved[0]; the failures
// are the geometries that cannot be formed and the pictures the stub reports too big
struct CheckJ {
    const mvhp_stream *s = nullptr;
    mvhp_output_request_t req{};
    int calls = 0, ok = 0, failed = 0, too_big = 0, bad = 0, next_seq = 0;
    uint64_t bytes = 0;   // what the downloader had to move: 16 per picture in a batch + the files
    std::vector<int> order;
    static int sink(void *user, int seq, int idr, int rc, const char *err, const mvhp_stream_params_t *, const mvhp_output_geometry_t *g,
                    const uint8_t *yuv, const uint8_t *rgb)
    {
        CheckJ &c = *static_cast<CheckJ *>(user);
        c.calls++;
        if (seq != c.next_seq || idr != c.order[(size_t)seq] || !g || yuv) c.bad++;
        c.next_seq = seq + 1;
        mvhp_output_geometry_t want;
        const bool formed = mvhp_output_geometry(c.s, idr, &c.req, &want) == MVHP_SUCCESS;
        const uint64_t h = picture_checksum(*c.s, idr);
        if (formed) c.bytes += sizeof(mvhp_jpeg_entry_t);
        if (rc != MVHP_SUCCESS) {
            c.failed++;
            if (formed) c.too_big++;
            if (!err || !*err || rgb || (formed && !stub_jpeg_too_big(h))) c.bad++;
            return 0;
        }
        const size_t len = formed ? stub_jpeg_length(h, mvhp_geometry_yuv_bytes(&want)) : 0;
        want.reserved[0] = (uint32_t)len;
        if (!formed || !rgb || stub_jpeg_too_big(h) || memcmp(&want, g, sizeof(want)) != 0) { c.bad++; return 0; }
        uint64_t got = 0;
        memcpy(&got, rgb, 8);
        if (got != h || rgb[8] != 0x3c || rgb[len - 1] != kLastJpeg) c.bad++;
        c.bytes += len;
        c.ok++;
        return 1;
    }
};

// sink of the PNG mode: no planes, the right picture's file in `rgb`, its length in reserved[0]; a picture fails only where its
// geometry cannot be formed, or -- `no_op` -- where the device table lacks the operation
struct CheckP {
    const mvhp_stream *s = nullptr;
    mvhp_output_request_t req{};
    bool scored = false;   // the request has MVHP_OUTPUT_SCORE: reserved[1] is the picture's score (the score mode checks its value)
    int calls = 0, ok = 0, failed = 0, bad = 0, next_seq = 0, no_op = 0;
    uint64_t bytes = 0;   // what the downloader had to move: 16 per picture in a batch + the files
    std::vector<int> order;
    static int sink(void *user, int seq, int idr, int rc, const char *err, const mvhp_stream_params_t *, const mvhp_output_geometry_t *g,
                    const uint8_t *yuv, const uint8_t *rgb)
    {
        CheckP &c = *static_cast<CheckP *>(user);
        c.calls++;
        if (seq != c.next_seq || idr != c.order[(size_t)seq] || !g || yuv) c.bad++;
        c.next_seq = seq + 1;
        mvhp_output_geometry_t want;
        const bool formed = mvhp_output_geometry(c.s, idr, &c.req, &want) == MVHP_SUCCESS;
        const uint64_t h = picture_checksum(*c.s, idr);
        if (rc != MVHP_SUCCESS) {
            c.failed++;
            if (err && strstr(err, "no PNG operation")) c.no_op++;
            else if (!err || !*err || rgb || formed) c.bad++;
            return 0;
        }
        if (!formed || !rgb) { c.bad++; return 0; }
        const size_t len = stub_png_length(h, &want);
        want.reserved[0] = (uint32_t)len;
        if (c.scored) want.reserved[1] = g->reserved[1];
        if (memcmp(&want, g, sizeof(want)) != 0) { c.bad++; return 0; }
        uint64_t got = 0;
        memcpy(&got, rgb, 8);
        if (got != h || rgb[8] != 0x3d || rgb[len - 1] != kLastPng) c.bad++;
        c.bytes += sizeof(mvhp_jpeg_entry_t) + len;
        c.ok++;
        return 1;
    }
};

// sink of the score mode: what CheckG and CheckJ check of the picture, and g->reserved[1] = the score of the stub's coded planes over
// the geometry's rectangle
struct CheckS {
    const mvhp_stream *s = nullptr;
    mvhp_output_request_t req{};   // without MVHP_OUTPUT_SCORE: what decides the geometry
    int mask = 0;
    int calls = 0, ok = 0, failed = 0, bad = 0, next_seq = 0, formed_n = 0, no_op = 0;
    std::vector<int> order;
    std::vector<uint32_t> scores;
    static int sink(void *user, int seq, int idr, int rc, const char *err, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g,
                    const uint8_t *yuv, const uint8_t *rgb)
    {
        CheckS &c = *static_cast<CheckS *>(user);
        c.calls++;
        if (seq != c.next_seq || idr != c.order[(size_t)seq] || !g) c.bad++;
        c.next_seq = seq + 1;
        const bool jpeg = (c.mask & MVHP_OUT_JPEG) != 0;
        mvhp_output_geometry_t want;
        const bool formed = mvhp_output_geometry(c.s, idr, &c.req, &want) == MVHP_SUCCESS;
        if (formed) c.formed_n++;
        const uint64_t h = picture_checksum(*c.s, idr);
        if (rc != MVHP_SUCCESS) {
            c.failed++;
            if (err && strstr(err, "picture-score operation")) c.no_op++;
            else if (!err || !*err || yuv || rgb || (formed && !(jpeg && stub_jpeg_too_big(h)))) c.bad++;
            return 0;
        }
        if (!formed) { c.bad++; return 0; }
        const bool coded = want.crop_x == 0 && want.crop_y == 0 && want.out_w == p->width_mbs * 16 && want.out_h == p->height_mbs * 16 &&
                           want.crop_w == want.out_w && want.crop_h == want.out_h;
        const mvhp_luma_stats_t st = expected_stats(h, jpeg || !coded, p, &want);
        want.reserved[1] = mvblank::luma_score(st.sum, st.sumsq, st.samples);
        if (jpeg) want.reserved[0] = (uint32_t)stub_jpeg_length(h, mvhp_geometry_yuv_bytes(&want));
        if (memcmp(&want, g, sizeof(want)) != 0) { c.bad++; return 0; }
        c.scores.push_back(g->reserved[1]);
        uint64_t got = 0;
        if (jpeg) {
            if (yuv || !rgb) { c.bad++; return 0; }
            memcpy(&got, rgb, 8);
            if (got != h || rgb[want.reserved[0] - 1] != kLastJpeg) c.bad++;
        } else {
            const bool want_rgb = (c.mask & 1) != 0, want_yuv = !want_rgb || (c.mask & 2) == 0;
            if ((yuv != nullptr) != want_yuv || (rgb != nullptr) != want_rgb) { c.bad++; return 0; }
            if (yuv) { memcpy(&got, yuv, 8); if (got != h || yuv[mvhp_geometry_yuv_bytes(g) - 1] != (coded ? 0x5a : kLastYuv)) c.bad++; }
            if (rgb) { memcpy(&got, rgb + 8, 8); if (got != h || rgb[mvhp_geometry_rgb_bytes(g) - 1] != (coded ? 0xa5 : kLastRgb)) c.bad++; }
        }
        c.ok++;
        return 1;
    }
};

// sink of the hist mode: everything CheckS checks (with `scored`: the score too; without it reserved[1] is 0), and
// mvhp_engine_picture_hist: inside the sink call the picture's own record, the stub's counts over the geometry's rectangle; NULL for
// a failed picture, for a picture that is not in its sink call, and without the flag.  Every fourth picture is kept (verdict 2): its
// record stays readable until the next picture's sink call gives it back, and is NULL from then on.
struct CheckH {
    CheckS base;
    mvhp_engine_t *e = nullptr;
    bool flag = true, scored = false;
    int bad = 0, records = 0, kept = -1, kept_checked = 0, n_order = 0;
    mvhp_plane_hist_t kept_want{};
    static int sink(void *user, int seq, int idr, int rc, const char *err, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g,
                    const uint8_t *yuv, const uint8_t *rgb)
    {
        CheckH &c = *static_cast<CheckH *>(user);
        if (c.kept >= 0) {   // the picture kept in the previous call: still there, then given back, then gone
            const mvhp_plane_hist_t *k = mvhp_engine_picture_hist(c.e, c.kept);
            if (!k || memcmp(k, &c.kept_want, sizeof(*k)) != 0) c.bad++;
            mvhp_engine_release_picture(c.e, c.kept);
            if (mvhp_engine_picture_hist(c.e, c.kept) != nullptr) c.bad++;
            c.kept = -1;
            c.kept_checked++;
        }
        const mvhp_plane_hist_t *got = mvhp_engine_picture_hist(c.e, seq);
        if (mvhp_engine_picture_hist(c.e, seq + 1) || mvhp_engine_picture_hist(c.e, seq - 1) || mvhp_engine_picture_hist(c.e, -1) ||
            mvhp_engine_picture_hist(c.e, c.n_order)) c.bad++;
        mvhp_output_geometry_t g2{};
        if (g) g2 = *g;
        if (!c.scored && g2.reserved[1] != 0) c.bad++;
        const int ok0 = c.base.ok;
        if (!c.scored && rc == MVHP_SUCCESS) {   // (CheckS expects the score in reserved[1]: hand it the one it would compute)
            mvhp_output_geometry_t want;
            if (mvhp_output_geometry(c.base.s, idr, &c.base.req, &want) == MVHP_SUCCESS) {
                const bool coded = want.crop_x == 0 && want.crop_y == 0 && want.out_w == p->width_mbs * 16 && want.out_h == p->height_mbs * 16 &&
                                   want.crop_w == want.out_w && want.crop_h == want.out_h;
                const mvhp_luma_stats_t st = expected_stats(picture_checksum(*c.base.s, idr), (c.base.mask & MVHP_OUT_JPEG) || !coded, p, &want);
                g2.reserved[1] = mvblank::luma_score(st.sum, st.sumsq, st.samples);
            }
        }
        const int verdict = CheckS::sink(&c.base, seq, idr, rc, err, p, g ? &g2 : nullptr, yuv, rgb);
        if (rc != MVHP_SUCCESS || c.base.ok == ok0 || !c.flag) {
            if (got) c.bad++;
            return verdict;
        }
        mvhp_output_geometry_t want;
        if (!got || ((uintptr_t)got & 15) || mvhp_output_geometry(c.base.s, idr, &c.base.req, &want) != MVHP_SUCCESS) { c.bad++; return verdict; }
        const bool coded = want.crop_x == 0 && want.crop_y == 0 && want.out_w == p->width_mbs * 16 && want.out_h == p->height_mbs * 16 &&
                           want.crop_w == want.out_w && want.crop_h == want.out_h;
        const mvhp_plane_hist_t exp = expected_hist(picture_checksum(*c.base.s, idr), (c.base.mask & MVHP_OUT_JPEG) || !coded, p, &want);
        if (memcmp(got, &exp, sizeof(exp)) != 0) c.bad++;
        mvhp_luma_stats_t from_hist;   // one probe serves both features: the score of the histogram is the picture's score
        mvrep::hist_stats(*got, from_hist);
        if (mvblank::luma_score(from_hist.sum, from_hist.sumsq, from_hist.samples) != g2.reserved[1]) c.bad++;
        c.records++;
        if (seq % 4 == 0 && seq + 1 < c.n_order) { c.kept = seq; c.kept_want = exp; return 2; }
        return verdict;
    }
};

// sink of the bars mode: what CheckG checks of the picture, and the picture's own box in the two reserved words
struct CheckB {
    const mvhp_stream *s = nullptr;
    mvhp_output_request_t req{};   // without MVHP_OUTPUT_BARS: what decides the geometry
    int mask = 0;
    int calls = 0, ok = 0, failed = 0, bad = 0, next_seq = 0, formed_n = 0, no_op = 0, empty = 0;
    std::vector<int> order;
    std::vector<uint64_t> boxes;
    static int sink(void *user, int seq, int idr, int rc, const char *err, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g,
                    const uint8_t *yuv, const uint8_t *rgb)
    {
        CheckB &c = *static_cast<CheckB *>(user);
        c.calls++;
        if (seq != c.next_seq || idr != c.order[(size_t)seq] || !g) c.bad++;
        c.next_seq = seq + 1;
        mvhp_output_geometry_t want;
        const bool formed = mvhp_output_geometry(c.s, idr, &c.req, &want) == MVHP_SUCCESS;
        if (formed) c.formed_n++;
        const uint64_t h = picture_checksum(*c.s, idr);
        if (rc != MVHP_SUCCESS) {
            c.failed++;
            if (err && strstr(err, "black-bar operation")) c.no_op++;
            else if (!err || !*err || yuv || rgb || formed) c.bad++;
            return 0;
        }
        if (!formed) { c.bad++; return 0; }
        const bool coded = want.crop_x == 0 && want.crop_y == 0 && want.out_w == p->width_mbs * 16 && want.out_h == p->height_mbs * 16 &&
                           want.crop_w == want.out_w && want.crop_h == want.out_h;
        const mvhp_luma_bars_t b = expected_bars(h, &want);
        want.reserved[0] = b.x | b.y << 16;
        want.reserved[1] = b.w | b.h << 16;
        if (memcmp(&want, g, sizeof(want)) != 0) { c.bad++; return 0; }
        if (b.w == 0) c.empty++;
        c.boxes.push_back((uint64_t)g->reserved[0] << 32 | g->reserved[1]);
        uint64_t got = 0;
        const bool want_rgb = (c.mask & 1) != 0, want_yuv = !want_rgb || (c.mask & 2) == 0;
        if ((yuv != nullptr) != want_yuv || (rgb != nullptr) != want_rgb) { c.bad++; return 0; }
        if (yuv) { memcpy(&got, yuv, 8); if (got != h || yuv[mvhp_geometry_yuv_bytes(g) - 1] != (coded ? 0x5a : kLastYuv)) c.bad++; }
        if (rgb) { memcpy(&got, rgb + 8, 8); if (got != h || rgb[mvhp_geometry_rgb_bytes(g) - 1] != (coded ? 0xa5 : kLastRgb)) c.bad++; }
        c.ok++;
        return 1;
    }
};

int plain_sink_accepts(void *, int, int, int rc, const char *, const mvhp_stream_params_t *, const uint8_t *, const uint8_t *) { return rc == MVHP_SUCCESS; }

std::vector<uint8_t> read_file(const std::string &path)
{
    std::vector<uint8_t> b;
    FILE *f = fopen(path.c_str(), "rb");
    uint8_t tmp[65536];
    for (size_t n; f && (n = fread(tmp, 1, sizeof(tmp), f)) > 0;) b.insert(b.end(), tmp, tmp + n);
    if (f) fclose(f);
    return b;
}

// BMP (24 bit, bottom-up, B G R, rows padded to 4 bytes) / TGA (type 10, bottom row first, B G R) -> top-down R G B of w x h, or empty
std::vector<uint8_t> bmp_pixels(const std::vector<uint8_t> &f, int w, int h)
{
    const size_t row = ((size_t)w * 3 + 3) & ~(size_t)3;
    uint32_t fw = 0, fh = 0, size = 0;
    if (f.size() != 54 + row * (size_t)h || f[0] != 'B' || f[1] != 'M') return {};
    memcpy(&size, &f[2], 4); memcpy(&fw, &f[18], 4); memcpy(&fh, &f[22], 4);
    if (size != f.size() || fw != (uint32_t)w || fh != (uint32_t)h || f[28] != 24) return {};
    std::vector<uint8_t> rgb((size_t)w * h * 3);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            for (int k = 0; k < 3; k++) rgb[((size_t)y * w + x) * 3 + k] = f[54 + (size_t)(h - 1 - y) * row + (size_t)x * 3 + 2 - k];
    return rgb;
}
std::vector<uint8_t> tga_pixels(const std::vector<uint8_t> &f, int w, int h)
{
    if (f.size() < 18 || f[2] != 10 || f[16] != 24 || (f[12] | (f[13] << 8)) != w || (f[14] | (f[15] << 8)) != h) return {};
    std::vector<uint8_t> bgr;
    size_t at = 18;
    while (at < f.size() && bgr.size() < (size_t)w * h * 3) {
        const int n = (f[at] & 127) + 1;
        const bool run = (f[at] & 128) != 0;
        at++;
        if (at + (run ? 3 : (size_t)n * 3) > f.size()) return {};
        for (int i = 0; i < n; i++) bgr.insert(bgr.end(), &f[at + (run ? 0 : (size_t)i * 3)], &f[at + (run ? 0 : (size_t)i * 3)] + 3);
        at += run ? 3 : (size_t)n * 3;
    }
    if (at != f.size() || bgr.size() != (size_t)w * h * 3) return {};
    std::vector<uint8_t> rgb(bgr.size());
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            for (int k = 0; k < 3; k++) rgb[((size_t)y * w + x) * 3 + k] = bgr[((size_t)(h - 1 - y) * w + x) * 3 + 2 - k];
    return rgb;
}

struct Check {
    const mvhp_stream *s = nullptr;
    bool want_rgb = false;
    int calls = 0, ok = 0, failed = 0, bad = 0, next_seq = 0;
    int abort_after = -1;
    std::vector<int> order;
    static int sink(void *user, int seq, int idr, int rc, const char *err, const mvhp_stream_params_t *p, const uint8_t *yuv,
                    const uint8_t *rgb)
    {
        Check &c = *static_cast<Check *>(user);
        c.calls++;
        if (seq != c.next_seq || idr != c.order[(size_t)seq]) c.bad++;   // in order, the right picture
        c.next_seq = seq + 1;
        if (rc != MVHP_SUCCESS) {
            c.failed++;
            if (!err || !*err || yuv || rgb) c.bad++;
            return 0;
        }
        std::vector<uint8_t> packed(mvhp_packed_frame_bytes(p));
        std::string e;
        if (c.s->decode_packed(idr, packed.data(), packed.size(), e) != h264::RC_SUCCESS) { c.bad++; return 0; }
        const uint64_t h = checksum(packed.data(), packed.size());
        uint64_t got = 0;
        memcpy(&got, yuv, 8);
        if (got != h || yuv[8] != 0x5a) c.bad++;
        if (c.want_rgb) {
            if (!rgb) c.bad++;
            else { memcpy(&got, rgb + 8, 8); if (got != h || rgb[0] != 0xa5) c.bad++; }
        } else if (rgb) c.bad++;
        c.ok++;
        if (c.abort_after >= 0 && c.calls > c.abort_after) return -1;
        return 1;
    }
};

} // namespace

const mvengine::DeviceApi &mvhp_hip_device_api() { return g_stub; }

#define EXPECT(cond)                                                                          \
    do {                                                                                      \
        if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s <stream.264>\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> buf;
    uint8_t tmp[65536];
    for (size_t n; (n = fread(tmp, 1, sizeof(tmp), f)) > 0;) buf.insert(buf.end(), tmp, tmp + n);
    fclose(f);
    mvhp_stream s;
    s.data = buf.data();
    s.size = buf.size();
    std::string err;
    if (s.build(err) != h264::RC_SUCCESS) { fprintf(stderr, "stream: %s\n", err.c_str()); return 2; }
    const int n_idr = (int)s.idrs.size();
    int failures = 0;
    std::vector<int> all(n_idr);
    for (int i = 0; i < n_idr; i++) all[i] = i;

    auto run = [&](const char *name, mvhp_engine_opts_t o, const std::vector<int> &order, int wanted, bool rgb, Check &c,
                   mvhp_decode_stats_t &st) {
        mvhp_engine_t *e = nullptr;
        int rc = mvhp_engine_create(&o, &e);
        if (rc != MVHP_SUCCESS) { fprintf(stderr, "%s: engine_create failed\n", name); failures++; return MVHP_FAILURE; }
        c.s = &s;
        c.want_rgb = rgb;
        c.order = order;
        rc = mvhp_engine_decode(e, &s, order.data(), (int)order.size(), wanted, rgb, Check::sink, &c, &st);
        mvhp_engine_destroy(e);
        printf("%-28s rc=%d issued=%u ok=%u failed=%u batches=%u requeued=%u ctx=%u threads=%u max_batch=%u\n", name, rc,
               st.pictures_issued, st.pictures_ok, st.pictures_failed, st.batches, st.batches_requeued, st.contexts, st.host_threads,
               st.max_batch_pictures);
        return rc;
    };
    mvhp_engine_opts_t base;
    memset(&base, 0, sizeof(base));
    base.fail_context = -1;
    base.host_threads = 4;

    {   // every picture, two contexts, small chunks and batches so that many of each are in flight
        mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 3; o.batch_pictures = 7;
        Check c; mvhp_decode_stats_t st;
        EXPECT(run("all/2ctx", o, all, n_idr, true, c, st) == MVHP_SUCCESS);
        EXPECT(c.bad == 0 && c.ok == n_idr && c.calls == n_idr);
        EXPECT((int)st.pictures_issued == n_idr && st.batches >= (uint32_t)(n_idr / 7));
    }
    {   // one thumbnail out of a long stream: exactly one picture is entropy-decoded (h264.c:173-179)
        mvhp_engine_opts_t o = base; o.contexts = 2;
        Check c; mvhp_decode_stats_t st;
        EXPECT(run("wanted=1", o, all, 1, false, c, st) == MVHP_SUCCESS);
        EXPECT(c.bad == 0 && c.ok == 1 && c.calls == 1 && st.pictures_issued == 1 && st.batches == 1);
    }
    {   // three pictures wanted: no more than three are decoded
        mvhp_engine_opts_t o = base; o.contexts = 3; o.chunk_pictures = 2;
        Check c; mvhp_decode_stats_t st;
        EXPECT(run("wanted=3", o, all, 3, true, c, st) == MVHP_SUCCESS);
        EXPECT(c.bad == 0 && c.ok == 3 && st.pictures_issued == 3);
    }
    {   // a batch fails on context 0: its pictures are decoded again and re-queued to another context, order is kept
        mvhp_engine_opts_t o = base; o.contexts = 3; o.chunk_pictures = 2; o.batch_pictures = 5; o.fail_context = 0;
        Check c; mvhp_decode_stats_t st;
        EXPECT(run("requeue/3ctx", o, all, n_idr, true, c, st) == MVHP_SUCCESS);
        EXPECT(c.bad == 0 && c.ok == n_idr && st.batches_requeued == 1 && (int)st.pictures_issued > n_idr);
    }
    {   // one context: a failed batch has nowhere to go, its pictures are reported as failures, the rest arrive
        mvhp_engine_opts_t o = base; o.contexts = 1; o.chunk_pictures = 2; o.batch_pictures = 5; o.fail_context = 0;
        Check c; mvhp_decode_stats_t st;
        EXPECT(run("fail/1ctx", o, all, n_idr, false, c, st) == MVHP_SUCCESS);
        EXPECT(c.bad == 0 && c.failed == 5 && c.ok == n_idr - 5 && st.batches_requeued == 0);
    }
    {   // ADVICE r2 (feeder race): a re-queued group arrives while the feeder has dropped its lock to page-lock a LARGER chunk
        // than the group holds (batches ramp 64 -> 128 -> 256, the chunk buffers regrow with them, the stub's page-locking
        // takes 30 ms, the first 64-picture batch fails on context 0 meanwhile).  The feeder must finish the chunk it was
        // sizing from the ordinary list and take the group on its next iteration; indexing the group with that chunk's
        // count read past its vector (AddressSanitizer) and delivered pictures twice / never.
        std::vector<int> order;
        for (int k = 0; k < 700; k++) order.push_back(k % n_idr);
        mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 256; o.fail_context = 0;
        Check c; mvhp_decode_stats_t st;
        g_slow_host_alloc_us = 30000;
        EXPECT(run("requeue during page-lock", o, order, (int)order.size(), false, c, st) == MVHP_SUCCESS);
        g_slow_host_alloc_us = 0;
        EXPECT(c.bad == 0 && c.ok == (int)order.size() && c.failed == 0 && st.batches_requeued == 1);
        EXPECT((int)st.pictures_issued > (int)order.size());   // the failed batch's pictures were entropy-decoded twice
    }
    {   // the sink keeps pictures (verdict 2) and two other threads give them back later (minivideo_decode's file writers):
        // the memory must still hold the same picture at release time -- an output chunk that went back to the pool early
        // would have been overwritten by a later download -- and the call must not return before the last release
        std::vector<int> order;
        for (int k = 0; k < 400; k++) order.push_back((k * 7) % n_idr);
        mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 3; o.batch_pictures = 9;
        mvhp_engine_t *e = nullptr;
        EXPECT(mvhp_engine_create(&o, &e) == MVHP_SUCCESS);
        struct Kept { int seq; const uint8_t *yuv; uint64_t h; };
        struct Keeper {
            mvhp_engine_t *e; const mvhp_stream *s;
            std::mutex mu; std::condition_variable cv; std::deque<Kept> q; bool closing = false;
            std::atomic<int> released{0}, bad{0}; int calls = 0;
        } kp;
        kp.e = e; kp.s = &s;
        auto keeper = [&kp] {
            for (;;) {
                Kept k;
                {
                    std::unique_lock<std::mutex> l(kp.mu);
                    kp.cv.wait(l, [&] { return kp.closing || !kp.q.empty(); });
                    if (kp.q.empty()) return;
                    k = kp.q.front(); kp.q.pop_front();
                }
                if (k.seq % 3) std::this_thread::sleep_for(std::chrono::microseconds(300));
                uint64_t got = 0;
                memcpy(&got, k.yuv, 8);
                if (got != k.h || k.yuv[8] != 0x5a) kp.bad++;
                kp.released++;
                mvhp_engine_release_picture(kp.e, k.seq);
            }
        };
        std::thread t1(keeper), t2(keeper);
        auto sink = [](void *u, int seq, int idr, int rc, const char *, const mvhp_stream_params_t *p, const uint8_t *yuv, const uint8_t *) {
            Keeper &x = *static_cast<Keeper *>(u);
            x.calls++;
            if (rc != MVHP_SUCCESS) { x.bad++; return 0; }
            std::vector<uint8_t> packed(mvhp_packed_frame_bytes(p));
            std::string er;
            if (x.s->decode_packed(idr, packed.data(), packed.size(), er) != h264::RC_SUCCESS) { x.bad++; return 0; }
            const uint64_t h = checksum(packed.data(), packed.size());
            if (seq % 5 == 4) return 1;   // (some pictures are not kept: both kinds share chunks)
            { std::lock_guard<std::mutex> l(x.mu); x.q.push_back(Kept{seq, yuv, h}); }
            x.cv.notify_one();
            if (seq % 6 == 0) std::this_thread::sleep_for(std::chrono::microseconds(500));   // released before this returns
            return 2;
        };
        mvhp_decode_stats_t st;
        EXPECT(mvhp_engine_decode(e, &s, order.data(), (int)order.size(), (int)order.size(), 0, sink, &kp, &st) == MVHP_SUCCESS);
        const int released_at_return = kp.released.load();
        { std::lock_guard<std::mutex> l(kp.mu); kp.closing = true; }
        kp.cv.notify_all();
        t1.join(); t2.join();
        mvhp_engine_release_picture(e, 3);   // a stale release is ignored
        mvhp_engine_destroy(e);
        printf("%-28s calls=%d kept=%d bad=%d ok=%u\n", "kept pictures", kp.calls, released_at_return, kp.bad.load(), st.pictures_ok);
        EXPECT(kp.bad == 0 && kp.calls == 400 && released_at_return == 320 && st.pictures_ok == 400);
    }
    {   // the sink stops the decode
        mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 2; o.batch_pictures = 4;
        Check c; c.abort_after = 5; mvhp_decode_stats_t st;
        EXPECT(run("abort", o, all, n_idr, false, c, st) == MVHP_FAILURE);
        EXPECT(c.bad == 0 && c.calls == 6);
    }
    {   // a list with repeats and a reversed order (ORDERED / DISTRIBUTED selections are arbitrary lists)
        std::vector<int> order;
        for (int i = n_idr - 1; i >= 0; i -= 2) order.push_back(i);
        order.push_back(0);
        order.push_back(0);
        mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 4;
        Check c; mvhp_decode_stats_t st;
        EXPECT(run("arbitrary order", o, order, (int)order.size(), true, c, st) == MVHP_SUCCESS);
        EXPECT(c.bad == 0 && c.ok == (int)order.size());
    }
    if (argc > 2) {   // a second stream whose picture argv[3] is broken: the failure arrives in its place
        const int broken = atoi(argv[3]);
        FILE *g = fopen(argv[2], "rb");
        std::vector<uint8_t> b2;
        for (size_t n; g && (n = fread(tmp, 1, sizeof(tmp), g)) > 0;) b2.insert(b2.end(), tmp, tmp + n);
        if (g) fclose(g);
        mvhp_stream s2;
        s2.data = b2.data();
        s2.size = b2.size();
        EXPECT(s2.build(err) == h264::RC_SUCCESS);
        std::vector<int> o2(s2.idrs.size());
        for (size_t i = 0; i < o2.size(); i++) o2[i] = (int)i;
        mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 3; o.batch_pictures = 6;
        mvhp_engine_t *e = nullptr;
        EXPECT(mvhp_engine_create(&o, &e) == MVHP_SUCCESS);
        struct S2 { int broken, bad = 0, ok = 0, failed = 0; } st2{broken};
        auto sink2 = [](void *u, int seq, int, int rc, const char *, const mvhp_stream_params_t *, const uint8_t *, const uint8_t *) {
            S2 &x = *static_cast<S2 *>(u);
            if ((rc == MVHP_SUCCESS) == (seq == x.broken)) x.bad++;
            if (rc == MVHP_SUCCESS) x.ok++; else x.failed++;
            return rc == MVHP_SUCCESS ? 1 : 0;
        };
        mvhp_decode_stats_t st;
        const int wanted = (int)o2.size() - 1;   // the broken picture makes the engine reach one picture further
        EXPECT(mvhp_engine_decode(e, &s2, o2.data(), (int)o2.size(), wanted, 0, sink2, &st2, &st) == MVHP_SUCCESS);
        mvhp_engine_destroy(e);
        printf("%-28s ok=%d failed=%d issued=%u\n", "broken picture", st2.ok, st2.failed, st.pictures_issued);
        EXPECT(st2.bad == 0 && st2.failed == 1 && st2.ok == wanted);
    }
    {   // the PUBLIC API on the stub device: minivideo_open / parse / decode with the file-writer pool (the sink keeps pictures,
        // writer threads write and release them) -- under the sanitizers this is the check of that hand-over.  The stub's
        // "pictures" carry the checksum of their records in the first eight bytes, which is what the files must start with.
        char tmpl[] = "/tmp/mvharness_XXXXXX";
        const char *dir = mkdtemp(tmpl);
        EXPECT(dir != nullptr);
        char cwd[4096];
        EXPECT(getcwd(cwd, sizeof(cwd)) != nullptr);
        std::string in = argv[1];
        if (in[0] != '/') in = std::string(cwd) + "/" + in;
        EXPECT(dir && chdir(dir) == 0);
        for (const char *writers : {"3", "0"}) {
            setenv("MINIVIDEO_WRITERS", writers, 1);
            MediaFile_t *m = nullptr;
            EXPECT(minivideo_open(in.c_str(), &m) == SUCCESS);
            EXPECT(m && minivideo_parse(m, false, true, false) == SUCCESS);
            EXPECT(m && minivideo_decode(m, ".", PICTURE_YUV420, 75, n_idr, PICTURE_UNFILTERED) == SUCCESS);
            int files = 0, good = 0;
            for (int k = 0; k < n_idr; k++) {
                const std::string name = std::string(m->file_name) + "_" + std::to_string(k) + ".yuv";
                FILE *g = fopen(name.c_str(), "rb");
                if (!g) continue;
                files++;
                uint64_t got = 0;
                std::vector<uint8_t> packed;
                mvhp_stream_params_t p;
                if (fread(&got, 1, 8, g) == 8 && mvhp_stream_params(&s, k, &p) == MVHP_SUCCESS) {
                    packed.resize(mvhp_packed_frame_bytes(&p));
                    std::string er;
                    if (s.decode_packed(k, packed.data(), packed.size(), er) == h264::RC_SUCCESS && got == checksum(packed.data(), packed.size())) good++;
                }
                fclose(g);
                remove(name.c_str());
            }
            printf("%-28s writers=%s files=%d of %d, right picture in %d\n", "public API", writers, files, n_idr, good);
            EXPECT(files == n_idr && good == n_idr);
            EXPECT(minivideo_close(&m) == SUCCESS);
        }
        unsetenv("MINIVIDEO_WRITERS");
        EXPECT(chdir(cwd) == 0);
        rmdir(dir);
    }
    EXPECT(g_geometry_calls == 0);   // nothing above asks for an output geometry
    if (argc > 4) {   // ---- geometry mode ----
        std::vector<uint8_t> b3 = read_file(argv[4]);
        mvhp_stream s3;
        s3.data = b3.data();
        s3.size = b3.size();
        EXPECT(s3.build(err) == h264::RC_SUCCESS);
        const int n3 = (int)s3.idrs.size();
        std::vector<int> o3((size_t)n3);
        for (int i = 0; i < n3; i++) o3[(size_t)i] = i;
        // what the engine has to form under `req`: runs of equal geometry are batches (the batch size below is larger than any
        // run), pictures whose geometry is the coded size take the plain operation, those without a geometry fail in place
        auto expect = [&](const mvhp_stream &st, const std::vector<int> &order, const mvhp_output_request_t &req, int &runs, int &geom_runs, int &unformed) {
            runs = geom_runs = unformed = 0;
            mvhp_output_geometry_t prev{};
            bool have = false;
            for (int idr : order) {
                mvhp_output_geometry_t g;
                mvhp_stream_params_t p;
                if (mvhp_output_geometry(&st, idr, &req, &g) != MVHP_SUCCESS) { unformed++; continue; }   // (occupies no slot: the run goes on)
                EXPECT(mvhp_stream_params(&st, idr, &p) == MVHP_SUCCESS);
                if (!have || memcmp(&prev, &g, sizeof(g)) != 0) {
                    runs++;
                    if (!(g.crop_x == 0 && g.crop_y == 0 && g.out_w == p.width_mbs * 16 && g.out_h == p.height_mbs * 16 && g.crop_w == g.out_w && g.crop_h == g.out_h)) geom_runs++;
                }
                prev = g;
                have = true;
            }
        };
        auto run_ex = [&](const char *name, mvhp_engine_opts_t o, const mvhp_stream &st, const std::vector<int> &order, int mask,
                          const mvhp_output_request_t &req, CheckG &c, mvhp_decode_stats_t &stats) {
            mvhp_engine_t *e = nullptr;
            if (mvhp_engine_create(&o, &e) != MVHP_SUCCESS) { failures++; return MVHP_FAILURE; }
            c.s = &st; c.req = req; c.order = order;
            c.want_rgb = (mask & 1) != 0;
            c.want_yuv = !c.want_rgb || (mask & 2) == 0;
            const int rc = mvhp_engine_decode_ex(e, &st, order.data(), (int)order.size(), (int)order.size(), mask, &req, CheckG::sink, &c, &stats);
            mvhp_engine_destroy(e);
            printf("%-28s rc=%d issued=%u ok=%u failed=%u batches=%u geometry=%u requeued=%u d2h=%llu\n", name, rc, stats.pictures_issued,
                   stats.pictures_ok, stats.pictures_failed, stats.batches, stats.geometry_launches, stats.batches_requeued,
                   (unsigned long long)stats.d2h_bytes);
            return rc;
        };
        auto d2h_expected = [&](const mvhp_stream &st, const std::vector<int> &order, const mvhp_output_request_t &req, int mask) {
            uint64_t sum = 0;
            for (int idr : order) {
                mvhp_output_geometry_t g;
                if (mvhp_output_geometry(&st, idr, &req, &g) != MVHP_SUCCESS) continue;
                if (!(mask & 1) || !(mask & 2)) sum += mvhp_geometry_yuv_bytes(&g);
                if (mask & 1) sum += mvhp_geometry_rgb_bytes(&g);
            }
            return sum;
        };
        const mvhp_output_request_t crop{MVHP_OUTPUT_CROP, 0, 0, 0}, box{MVHP_OUTPUT_CROP | MVHP_OUTPUT_BOX, 40, 40, 0};
        for (int mask : {0, MVHP_OUT_RGB, MVHP_OUT_RGB_ONLY})
            for (const mvhp_output_request_t &req : {crop, box}) {   // batches split where the geometry changes
                mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 2; o.batch_pictures = 64;
                CheckG c; mvhp_decode_stats_t st;
                int runs, geom_runs, unformed;
                expect(s3, o3, req, runs, geom_runs, unformed);
                const int before = g_geometry_calls;
                EXPECT(run_ex(req.flags & MVHP_OUTPUT_BOX ? "geometry box" : "geometry crop", o, s3, o3, mask, req, c, st) == MVHP_SUCCESS);
                EXPECT(runs >= 4 && geom_runs >= 3 && unformed >= 1);   // (the stream the test wrote mixes crops)
                EXPECT(c.bad == 0 && c.calls == n3 && c.failed == unformed && c.ok == n3 - unformed);
                EXPECT((int)st.batches == runs && (int)st.geometry_launches == geom_runs && g_geometry_calls - before == geom_runs);
                EXPECT(st.d2h_bytes == d2h_expected(s3, o3, req, mask));
            }
        {   // small batches inside the runs, three contexts, the first batch of context 0 fails: re-queued with its geometry
            std::vector<int> order;
            for (int k = 0; k < 3 * n3; k++) order.push_back(k % n3);
            mvhp_engine_opts_t o = base; o.contexts = 3; o.chunk_pictures = 2; o.batch_pictures = 3; o.fail_context = 0;
            CheckG c; mvhp_decode_stats_t st;
            int runs, geom_runs, unformed;
            expect(s3, order, box, runs, geom_runs, unformed);
            EXPECT(run_ex("geometry requeue/3ctx", o, s3, order, MVHP_OUT_RGB, box, c, st) == MVHP_SUCCESS);
            EXPECT(c.bad == 0 && c.failed == unformed && c.ok == (int)order.size() - unformed && st.batches_requeued == 1);
            EXPECT((int)st.batches >= runs && st.d2h_bytes == d2h_expected(s3, order, box, MVHP_OUT_RGB));
        }
        {   // requests that equal the coded size -- a crop of an uncropped stream, a box that already contains it -- never call the
            // geometry operation
            const int before = g_geometry_calls;
            for (const mvhp_output_request_t &req : {crop, mvhp_output_request_t{MVHP_OUTPUT_CROP | MVHP_OUTPUT_BOX, 4096, 4096, 0}}) {
                mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 3; o.batch_pictures = 7;
                CheckG c; mvhp_decode_stats_t st;
                EXPECT(run_ex("geometry = coded size", o, s, all, MVHP_OUT_RGB, req, c, st) == MVHP_SUCCESS);
                EXPECT(c.bad == 0 && c.ok == n_idr && c.with_geometry == 0 && st.geometry_launches == 0);
            }
            EXPECT(g_geometry_calls == before);
        }
        {   // a malformed request is refused
            mvhp_engine_opts_t o = base; o.contexts = 1;
            mvhp_engine_t *e = nullptr;
            EXPECT(mvhp_engine_create(&o, &e) == MVHP_SUCCESS);
            const mvhp_output_request_t bad{MVHP_OUTPUT_BOX, 1, 40, 0};
            mvhp_decode_stats_t st;
            EXPECT(mvhp_engine_decode_ex(e, &s3, o3.data(), n3, n3, 0, &bad, nullptr, nullptr, &st) == MVHP_FAILURE);
            mvhp_engine_destroy(e);
        }
        {   // minivideo_decode under MINIVIDEO_CROP / MINIVIDEO_THUMBNAIL: files of the output geometry, the stub's stamps in place
            char tmpl[] = "/tmp/mvharness_XXXXXX";
            const char *dir = mkdtemp(tmpl);
            char cwd[4096];
            EXPECT(dir != nullptr && getcwd(cwd, sizeof(cwd)) != nullptr);
            std::string in = argv[4];
            if (in[0] != '/') in = std::string(cwd) + "/" + in;
            EXPECT(dir && chdir(dir) == 0);
            struct Sw { const char *crop, *thumb; mvhp_output_request_t req; };
            const Sw sws[] = {{"1", nullptr, crop}, {nullptr, "40x40", box}, {"1", "40x40", box}, {"0", nullptr, mvhp_output_request_t{}}};
            for (const Sw &sw : sws)
                for (int fmt : {PICTURE_YUV420, PICTURE_BMP, PICTURE_TGA})
                    for (const char *writers : {"2", "0"}) {
                        setenv("MINIVIDEO_WRITERS", writers, 1);
                        if (sw.crop) setenv("MINIVIDEO_CROP", sw.crop, 1); else unsetenv("MINIVIDEO_CROP");
                        if (sw.thumb) setenv("MINIVIDEO_THUMBNAIL", sw.thumb, 1); else unsetenv("MINIVIDEO_THUMBNAIL");
                        MediaFile_t *m = nullptr;
                        EXPECT(minivideo_open(in.c_str(), &m) == SUCCESS);
                        EXPECT(m && minivideo_parse(m, false, true, false) == SUCCESS);
                        EXPECT(m && minivideo_decode(m, ".", fmt, 75, n3, PICTURE_UNFILTERED) == SUCCESS);
                        const char *ext = fmt == PICTURE_BMP ? ".bmp" : fmt == PICTURE_TGA ? ".tga" : ".yuv";
                        int files = 0, good = 0, k = 0, expected = 0;
                        for (int idr = 0; idr < n3; idr++) {   // pictures without a geometry are skipped: file k is the k-th good one
                            mvhp_output_geometry_t g;
                            mvhp_stream_params_t p;
                            if (mvhp_output_geometry(&s3, idr, &sw.req, &g) != MVHP_SUCCESS) continue;
                            expected++;
                            EXPECT(mvhp_stream_params(&s3, idr, &p) == MVHP_SUCCESS);
                            const bool coded = g.crop_x == 0 && g.crop_y == 0 && g.out_w == p.width_mbs * 16 && g.out_h == p.height_mbs * 16 &&
                                               g.crop_w == g.out_w && g.crop_h == g.out_h;
                            const std::string name = std::string(m->file_name) + "_" + std::to_string(k++) + ext;
                            const std::vector<uint8_t> f = read_file(name);
                            if (f.empty()) continue;
                            files++;
                            remove(name.c_str());
                            const uint64_t h = picture_checksum(s3, idr);
                            const int w = (int)g.out_w, ht = (int)g.out_h;
                            uint64_t got = 0;
                            if (fmt == PICTURE_YUV420) {
                                if (f.size() != mvhp_geometry_yuv_bytes(&g)) continue;
                                memcpy(&got, f.data(), 8);
                                if (got == h && f[8] == 0x5a && f.back() == (coded ? 0x5a : kLastYuv)) good++;
                            } else {
                                const std::vector<uint8_t> rgb = fmt == PICTURE_BMP ? bmp_pixels(f, w, ht) : tga_pixels(f, w, ht);
                                if (rgb.size() != mvhp_geometry_rgb_bytes(&g)) continue;
                                memcpy(&got, rgb.data() + 8, 8);
                                if (got == h && rgb[0] == 0xa5 && rgb.back() == (coded ? 0xa5 : kLastRgb)) good++;
                            }
                        }
                        printf("%-28s crop=%s thumbnail=%s format=%d writers=%s files=%d of %d, right in %d\n", "public API, geometry",
                               sw.crop ? sw.crop : "-", sw.thumb ? sw.thumb : "-", fmt, writers, files, expected, good);
                        EXPECT(expected >= 4 && files == expected && good == expected);
                        EXPECT(minivideo_close(&m) == SUCCESS);
                    }
            // malformed values: FAILURE, with a message, before the device is touched
            unsetenv("MINIVIDEO_CROP");
            for (const char *bad : {"abc", "0x10", "320", "1x40", "40x1", "40x", "x40", "40x40x", " 40x40", "40X40", "-4x40", "40x99999"}) {
                setenv("MINIVIDEO_THUMBNAIL", bad, 1);
                MediaFile_t *m = nullptr;
                EXPECT(minivideo_open(in.c_str(), &m) == SUCCESS);
                EXPECT(m && minivideo_parse(m, false, true, false) == SUCCESS);
                const int ctx_before = g_ctx_created, recon_before = g_recon_calls + g_geometry_calls;
                fflush(stdout);
                fflush(stderr);
                int pipefd[2];
                EXPECT(pipe(pipefd) == 0);
                const int saved = dup(2);
                dup2(pipefd[1], 2);
                const int rc = m ? minivideo_decode(m, ".", PICTURE_YUV420, 75, n3, PICTURE_UNFILTERED) : SUCCESS;
                fflush(stderr);
                dup2(saved, 2);
                close(saved);
                close(pipefd[1]);
                char msg[512] = "";
                const ssize_t got = read(pipefd[0], msg, sizeof(msg) - 1);
                close(pipefd[0]);
                printf("%-28s '%s' rc=%d message: %s", "malformed thumbnail", bad, rc, got > 0 ? msg : "(none)\n");
                EXPECT(rc == FAILURE && got > 0 && strstr(msg, "MINIVIDEO_THUMBNAIL") != nullptr);
                EXPECT(g_ctx_created == ctx_before && g_recon_calls + g_geometry_calls == recon_before);
                EXPECT(minivideo_close(&m) == SUCCESS);
            }
            unsetenv("MINIVIDEO_THUMBNAIL");
            unsetenv("MINIVIDEO_WRITERS");
            EXPECT(chdir(cwd) == 0);
            rmdir(dir);
        }
        printf("GEOMETRY MODE DONE\n");
        if (argc > 5 && !strcmp(argv[5], "jpeg")) {   // ---- JPEG mode: MVHP_OUT_JPEG against the stub's JPEG operation ----
            auto run_jpeg = [&](const char *name, mvhp_engine_opts_t o, const mvhp_stream &st, const std::vector<int> &order, int wanted,
                                const mvhp_output_request_t &req, CheckJ &c, mvhp_decode_stats_t &stats) {
                mvhp_engine_t *e = nullptr;
                if (mvhp_engine_create(&o, &e) != MVHP_SUCCESS) { failures++; return MVHP_FAILURE; }
                c.s = &st; c.req = req; c.order = order;
                const int rc = mvhp_engine_decode_ex(e, &st, order.data(), (int)order.size(), wanted, MVHP_OUT_JPEG, &req, CheckJ::sink, &c, &stats);
                mvhp_engine_destroy(e);
                printf("%-28s rc=%d issued=%u ok=%u failed=%u (too big %d) batches=%u geometry=%u requeued=%u d2h=%llu\n", name, rc,
                       stats.pictures_issued, stats.pictures_ok, stats.pictures_failed, c.too_big, stats.batches, stats.geometry_launches,
                       stats.batches_requeued, (unsigned long long)stats.d2h_bytes);
                return rc;
            };
            std::vector<int> order;
            for (int k = 0; k < 3 * n3; k++) order.push_back(k % n3);
            int unformed = 0, big = 0;
            for (int idr : order) {
                mvhp_output_geometry_t g;
                if (mvhp_output_geometry(&s3, idr, &box, &g) != MVHP_SUCCESS) unformed++;
                else if (stub_jpeg_too_big(picture_checksum(s3, idr))) big++;
            }
            for (int contexts = 1; contexts <= 3; contexts++)
                for (mvhp_output_request_t req : {mvhp_output_request_t{0, 0, 0, 0}, crop, box}) {
                    req.reserved = MVHP_JPEG_REQUEST(contexts == 2 ? 0 : 90, contexts == 3 ? 2 : 0);
                    mvhp_engine_opts_t o = base; o.contexts = contexts; o.chunk_pictures = 2; o.batch_pictures = contexts == 1 ? 64 : 3;
                    o.fail_context = contexts == 3 ? 0 : -1;   // three contexts: the first batch of context 0 fails and is re-queued
                    CheckJ c; mvhp_decode_stats_t st;
                    const int before = g_jpeg_calls, recon_before = g_recon_calls + g_geometry_calls;
                    EXPECT(run_jpeg(req.flags & MVHP_OUTPUT_BOX ? "jpeg box" : req.flags ? "jpeg crop" : "jpeg coded size", o, s3, order,
                                    (int)order.size(), req, c, st) == MVHP_SUCCESS);
                    EXPECT(c.bad == 0 && c.calls == (int)order.size() && c.ok + c.failed == c.calls && c.ok == (int)st.pictures_ok);
                    if (req.flags & MVHP_OUTPUT_BOX) EXPECT(c.failed == unformed + big && c.too_big == big);
                    if (!req.flags) EXPECT(st.geometry_launches == 0);
                    EXPECT(st.d2h_bytes == c.bytes && (int)st.batches == g_jpeg_calls - before);
                    EXPECT(g_recon_calls + g_geometry_calls == recon_before);   // every launch of a JPEG call is the JPEG operation
                    EXPECT((int)st.batches_requeued == (contexts == 3 ? 1 : 0));
                }
            EXPECT(big >= 1 && unformed >= 1);
            {   // `wanted` caps the call: failed pictures (too big) do not count towards it
                mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 2; o.batch_pictures = 4;
                CheckJ c; mvhp_decode_stats_t st;
                EXPECT(run_jpeg("jpeg wanted = 5", o, s3, order, 5, box, c, st) == MVHP_SUCCESS);
                EXPECT(c.bad == 0 && c.ok == 5 && st.pictures_ok == 5);
            }
            {   // the plain sink cannot take a file's length: refused
                mvhp_engine_opts_t o = base; o.contexts = 1;
                mvhp_engine_t *e = nullptr;
                EXPECT(mvhp_engine_create(&o, &e) == MVHP_SUCCESS);
                Check c; mvhp_decode_stats_t st;
                EXPECT(mvhp_engine_decode(e, &s3, o3.data(), n3, n3, MVHP_OUT_JPEG, Check::sink, &c, &st) == MVHP_FAILURE);
                mvhp_engine_destroy(e);
            }
            printf("JPEG MODE DONE\n");
        }
        if (argc > 5 && !strcmp(argv[5], "png")) {   // ---- PNG mode: MVHP_OUT_PNG against the stub's PNG operation ----
            auto run_png = [&](const char *name, mvhp_engine_opts_t o, const mvhp_stream &st, const std::vector<int> &order, int wanted,
                               const mvhp_output_request_t &req, CheckP &c, mvhp_decode_stats_t &stats) {
                mvhp_engine_t *e = nullptr;
                if (mvhp_engine_create(&o, &e) != MVHP_SUCCESS) { failures++; return MVHP_FAILURE; }
                c.s = &st; c.req = req; c.req.flags &= ~MVHP_OUTPUT_SCORE; c.scored = (req.flags & MVHP_OUTPUT_SCORE) != 0; c.order = order;
                const int rc = mvhp_engine_decode_ex(e, &st, order.data(), (int)order.size(), wanted, MVHP_OUT_PNG, &req, CheckP::sink, &c, &stats);
                mvhp_engine_destroy(e);
                printf("%-28s flags=%#x rc=%d issued=%u ok=%u failed=%u batches=%u geometry=%u requeued=%u d2h=%llu\n", name, req.flags, rc,
                       stats.pictures_issued, stats.pictures_ok, stats.pictures_failed, stats.batches, stats.geometry_launches,
                       stats.batches_requeued, (unsigned long long)stats.d2h_bytes);
                return rc;
            };
            std::vector<int> order;
            for (int k = 0; k < 3 * n3; k++) order.push_back(k % n3);
            int unformed = 0;
            for (int idr : order) {
                mvhp_output_geometry_t g;
                if (mvhp_output_geometry(&s3, idr, &box, &g) != MVHP_SUCCESS) unformed++;
            }
            mvhp_output_request_t turned = crop, turned_box = box;
            turned.flags |= MVHP_OUTPUT_ROTATE(1);
            turned_box.flags |= MVHP_OUTPUT_ROTATE(3);
            for (int contexts = 1; contexts <= 3; contexts++)
                for (const mvhp_output_request_t &req : {mvhp_output_request_t{0, 0, 0, 0}, crop, box, turned, turned_box}) {
                    mvhp_engine_opts_t o = base; o.contexts = contexts; o.chunk_pictures = 2; o.batch_pictures = contexts == 1 ? 64 : 3;
                    o.fail_context = contexts == 3 ? 0 : -1;   // three contexts: the first batch of context 0 fails and is re-queued
                    CheckP c; mvhp_decode_stats_t st;
                    const int before = g_png_calls, others_before = g_recon_calls + g_geometry_calls + g_jpeg_calls;
                    EXPECT(run_png("png", o, s3, order, (int)order.size(), req, c, st) == MVHP_SUCCESS);
                    EXPECT(c.bad == 0 && c.no_op == 0 && c.calls == (int)order.size() && c.ok + c.failed == c.calls && c.ok == (int)st.pictures_ok);
                    if (req.flags & MVHP_OUTPUT_BOX) EXPECT(c.failed == unformed);
                    if (!req.flags) EXPECT(st.geometry_launches == 0 && c.failed == 0);
                    EXPECT(st.d2h_bytes == c.bytes && (int)st.batches == g_png_calls - before);
                    EXPECT(g_recon_calls + g_geometry_calls + g_jpeg_calls == others_before);   // every launch of a PNG call is the PNG operation
                    EXPECT((int)st.batches_requeued == (contexts == 3 ? 1 : 0));
                }
            EXPECT(unformed >= 1);
            {   // `wanted` caps the call
                mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 2; o.batch_pictures = 4;
                CheckP c; mvhp_decode_stats_t st;
                EXPECT(run_png("png wanted = 5", o, s3, order, 5, crop, c, st) == MVHP_SUCCESS);
                EXPECT(c.bad == 0 && c.ok == 5 && st.pictures_ok == 5 && st.pictures_issued < order.size());
            }
            {   // scores travel beside the files: 32 more bytes per delivered picture, the same files
                mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 2; o.batch_pictures = 3;
                mvhp_output_request_t scored = crop;
                scored.flags |= MVHP_OUTPUT_SCORE;
                CheckP c; mvhp_decode_stats_t st;
                const int stats0 = g_stats_calls;
                EXPECT(run_png("png + scores", o, s3, order, (int)order.size(), scored, c, st) == MVHP_SUCCESS);
                EXPECT(c.bad == 0 && c.ok > 0 && c.ok + c.failed == c.calls && g_stats_calls - stats0 == (int)st.batches);
                EXPECT(st.d2h_bytes == c.bytes + 32ull * (uint64_t)c.ok);
            }
            {   // a device table without the operation: every picture fails with a message, nothing is launched
                mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 2; o.batch_pictures = 3;
                g_stub.caps &= ~mvengine::CAP_PNG;
                CheckP c; mvhp_decode_stats_t st;
                const int before = g_png_calls;
                EXPECT(run_png("png without the operation", o, s3, order, (int)order.size(), mvhp_output_request_t{0, 0, 0, 0}, c, st) != MVHP_SUCCESS);
                EXPECT(c.bad == 0 && c.ok == 0 && c.no_op == (int)order.size() && g_png_calls == before);
                g_stub.caps |= mvengine::CAP_PNG;
            }
            {   // the plain sink cannot take a file's length, and a call delivers one kind of file: refused
                mvhp_engine_opts_t o = base; o.contexts = 1;
                mvhp_engine_t *e = nullptr;
                EXPECT(mvhp_engine_create(&o, &e) == MVHP_SUCCESS);
                Check c; CheckP cp; mvhp_decode_stats_t st;
                EXPECT(mvhp_engine_decode(e, &s3, o3.data(), n3, n3, MVHP_OUT_PNG, Check::sink, &c, &st) == MVHP_FAILURE);
                EXPECT(mvhp_engine_decode_ex(e, &s3, o3.data(), n3, n3, MVHP_OUT_PNG | MVHP_OUT_JPEG, nullptr, CheckP::sink, &cp, &st) == MVHP_FAILURE);
                EXPECT(cp.calls == 0);
                mvhp_engine_destroy(e);
            }
            printf("PNG MODE DONE\n");
        }
        if (argc > 5 && !strcmp(argv[5], "orient")) {   // ---- orient mode: MVHP_OUTPUT_ORIENT / _ROTATE against the stub's turn ----
            auto run_o = [&](const char *name, mvhp_engine_opts_t o, const mvhp_stream &st, const std::vector<int> &order, int mask,
                             const mvhp_output_request_t &req, CheckO &c, mvhp_decode_stats_t &stats) {
                mvhp_engine_t *e = nullptr;
                if (mvhp_engine_create(&o, &e) != MVHP_SUCCESS) { failures++; return MVHP_FAILURE; }
                c.s = &st; c.req = req; c.order = order;
                c.want_rgb = (mask & 1) != 0;
                c.want_yuv = !c.want_rgb || (mask & 2) == 0;
                const int rc = mvhp_engine_decode_ex(e, &st, order.data(), (int)order.size(), (int)order.size(), mask, &req, CheckO::sink, &c, &stats);
                mvhp_engine_destroy(e);
                printf("%-28s flags=%#x rc=%d ok=%u failed=%u batches=%u geometry=%u requeued=%u d2h=%llu\n", name, req.flags, rc, stats.pictures_ok,
                       stats.pictures_failed, stats.batches, stats.geometry_launches, stats.batches_requeued, (unsigned long long)stats.d2h_bytes);
                return rc;
            };
            // runs of equal delivered geometry are batches; those that scale before the turn bring the extra buffer
            auto expect_o = [&](const std::vector<int> &order, const mvhp_output_request_t &req, int &runs, int &scaled_runs, int &unformed) {
                runs = scaled_runs = unformed = 0;
                mvhp_output_geometry_t prev{};
                bool have = false;
                const int turns = mvhp_output_turns(&s3, &req);
                for (int idr : order) {
                    mvhp_output_geometry_t g;
                    if (mvhp_output_geometry(&s3, idr, &req, &g) != MVHP_SUCCESS) { unformed++; continue; }
                    if (!have || memcmp(&prev, &g, sizeof(g)) != 0) {
                        runs++;
                        const uint32_t w0 = (turns & 1) ? g.out_h : g.out_w, h0 = (turns & 1) ? g.out_w : g.out_h;
                        if (w0 != g.crop_w || h0 != g.crop_h) scaled_runs++;
                    }
                    prev = g;
                    have = true;
                }
            };
            int scaled_seen = 0, unscaled_seen = 0;
            for (uint32_t q = 1; q <= 3; q++)
                for (uint32_t shape : {0u, (uint32_t)MVHP_OUTPUT_CROP, (uint32_t)(MVHP_OUTPUT_CROP | MVHP_OUTPUT_BOX)})
                    for (int mask : {0, MVHP_OUT_RGB, MVHP_OUT_RGB_ONLY}) {
                        const mvhp_output_request_t req{shape | MVHP_OUTPUT_ROTATE(q), 40, 24, 0};   // (an oblong box: turned, it is another box)
                        mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 2; o.batch_pictures = 64;
                        CheckO c; mvhp_decode_stats_t st;
                        int runs, scaled_runs, unformed;
                        expect_o(o3, req, runs, scaled_runs, unformed);
                        const int orient0 = g_orient_calls, mid0 = g_mid_calls;
                        EXPECT(run_o("orient", o, s3, o3, mask, req, c, st) == MVHP_SUCCESS);
                        EXPECT(c.bad == 0 && c.calls == n3 && c.failed == unformed && c.ok == n3 - unformed);
                        // every batch of a call that turns has the pass and counts as a geometry launch; the buffer of the unturned
                        // planes exists exactly in the batches that scale
                        // (the turn alone forms one geometry per picture size, and a batch also ends where the stream parameters change)
                        EXPECT(shape == 0 ? (int)st.batches >= runs : (int)st.batches == runs);
                        EXPECT(st.geometry_launches == st.batches && g_orient_calls - orient0 == (int)st.batches);
                        EXPECT(shape == 0 ? scaled_runs == 0 && g_mid_calls == mid0 : g_mid_calls - mid0 == scaled_runs);
                        EXPECT(st.d2h_bytes == c.bytes);   // the turned pictures only
                        scaled_seen += scaled_runs;
                        unscaled_seen += runs - scaled_runs;
                    }
            EXPECT(scaled_seen > 0 && unscaled_seen > 0);
            {   // odd turns exchange the sides of what is delivered, and the box is applied to the turned picture
                const mvhp_output_request_t r0{MVHP_OUTPUT_CROP | MVHP_OUTPUT_BOX, 40, 24, 0}, r1{MVHP_OUTPUT_CROP | MVHP_OUTPUT_BOX | MVHP_OUTPUT_ROTATE(1), 24, 40, 0};
                int swapped = 0;
                for (int idr = 0; idr < n3; idr++) {
                    mvhp_output_geometry_t a, b;
                    if (mvhp_output_geometry(&s3, idr, &r0, &a) != MVHP_SUCCESS) continue;
                    EXPECT(mvhp_output_geometry(&s3, idr, &r1, &b) == MVHP_SUCCESS);
                    EXPECT(a.out_w == b.out_h && a.out_h == b.out_w && a.crop_x == b.crop_x && a.crop_y == b.crop_y && a.crop_w == b.crop_w && a.crop_h == b.crop_h);
                    EXPECT(mvhp_geometry_yuv_bytes(&a) == mvhp_geometry_yuv_bytes(&b));
                    swapped++;
                }
                EXPECT(swapped >= 4);
            }
            {   // turns that come to 0 -- no angle, "auto" on a stream without a rotation -- take today's paths: no turn, no extra buffer, and
                // where the pictures are of the coded size no geometry launch either
                const int orient0 = g_orient_calls, mid0 = g_mid_calls, geom0 = g_geometry_calls;
                for (const mvhp_output_request_t &req : {mvhp_output_request_t{MVHP_OUTPUT_ROTATE(0), 0, 0, 0}, mvhp_output_request_t{MVHP_OUTPUT_ORIENT, 0, 0, 0},
                                                         mvhp_output_request_t{MVHP_OUTPUT_ORIENT | MVHP_OUTPUT_CROP | MVHP_OUTPUT_BOX, 4096, 4096, 0}}) {
                    mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 3; o.batch_pictures = 7;
                    CheckO c; mvhp_decode_stats_t st;
                    EXPECT(run_o("orient: zero turns", o, s, all, MVHP_OUT_RGB, req, c, st) == MVHP_SUCCESS);
                    EXPECT(c.bad == 0 && c.ok == n_idr && st.geometry_launches == 0);
                }
                EXPECT(g_orient_calls == orient0 && g_mid_calls == mid0 && g_geometry_calls == geom0);
                // ... and with a crop the launches of the request without the flag
                const mvhp_output_request_t with{MVHP_OUTPUT_ORIENT | MVHP_OUTPUT_CROP, 0, 0, 0};
                mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 2; o.batch_pictures = 64;
                CheckO c; CheckG cg; mvhp_decode_stats_t st, stg;
                EXPECT(run_o("orient: zero turns, crop", o, s3, o3, MVHP_OUT_RGB, with, c, st) == MVHP_SUCCESS && c.bad == 0);
                EXPECT(run_ex("the same without the flag", o, s3, o3, MVHP_OUT_RGB, crop, cg, stg) == MVHP_SUCCESS && cg.bad == 0);
                EXPECT(st.batches == stg.batches && st.geometry_launches == stg.geometry_launches && st.d2h_bytes == stg.d2h_bytes);
                EXPECT(g_orient_calls == orient0 && g_mid_calls == mid0);
            }
            {   // small batches, three contexts, the first batch of context 0 fails: re-queued with its turn
                std::vector<int> order;
                for (int k = 0; k < 3 * n3; k++) order.push_back(k % n3);
                const mvhp_output_request_t req{MVHP_OUTPUT_CROP | MVHP_OUTPUT_BOX | MVHP_OUTPUT_ROTATE(3), 40, 24, 0};
                mvhp_engine_opts_t o = base; o.contexts = 3; o.chunk_pictures = 2; o.batch_pictures = 3; o.fail_context = 0;
                CheckO c; mvhp_decode_stats_t st;
                int runs, scaled_runs, unformed;
                expect_o(order, req, runs, scaled_runs, unformed);
                EXPECT(run_o("orient requeue/3ctx", o, s3, order, MVHP_OUT_RGB, req, c, st) == MVHP_SUCCESS);
                EXPECT(c.bad == 0 && c.failed == unformed && c.ok == (int)order.size() - unformed && st.batches_requeued == 1);
                EXPECT((int)st.batches >= runs && st.d2h_bytes == c.bytes);
            }
            {   // JPEG of turned pictures: the encoder reads the turned planes, the blob is sized by the delivered geometry
                const mvhp_output_request_t req{MVHP_OUTPUT_CROP | MVHP_OUTPUT_BOX | MVHP_OUTPUT_ROTATE(1), 40, 24, MVHP_JPEG_REQUEST(80, 0)};
                mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 2; o.batch_pictures = 5;
                mvhp_engine_t *e = nullptr;
                EXPECT(mvhp_engine_create(&o, &e) == MVHP_SUCCESS);
                CheckJ c; mvhp_decode_stats_t st;
                c.s = &s3; c.req = req; c.order = o3;
                const int orient0 = g_orient_calls;
                EXPECT(mvhp_engine_decode_ex(e, &s3, o3.data(), n3, n3, MVHP_OUT_JPEG, &req, CheckJ::sink, &c, &st) == MVHP_SUCCESS);
                mvhp_engine_destroy(e);
                printf("%-28s ok=%d failed=%d batches=%u d2h=%llu\n", "orient: jpeg", c.ok, c.failed, st.batches, (unsigned long long)st.d2h_bytes);
                EXPECT(c.bad == 0 && c.ok == (int)st.pictures_ok && c.ok > 0 && st.d2h_bytes == c.bytes && g_orient_calls - orient0 == (int)st.batches);
            }
            {   // a device table without the operation: every picture of a call that turns fails with the message; zero turns is not affected
                g_stub.caps &= ~mvengine::CAP_ORIENT;
                mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 2; o.batch_pictures = 4;
                CheckO c; mvhp_decode_stats_t st;
                const int orient0 = g_orient_calls, recon0 = g_recon_calls + g_geometry_calls + g_jpeg_calls;
                EXPECT(run_o("orient: table without it", o, s, all, 0, mvhp_output_request_t{MVHP_OUTPUT_ROTATE(2), 0, 0, 0}, c, st) == MVHP_FAILURE);
                EXPECT(c.bad == 0 && c.ok == 0 && c.no_op == n_idr && g_orient_calls == orient0);
                EXPECT(g_recon_calls + g_geometry_calls + g_jpeg_calls == recon0);
                CheckO c0;
                EXPECT(run_o("orient: table without it, 0", o, s, all, 0, mvhp_output_request_t{MVHP_OUTPUT_ORIENT, 0, 0, 0}, c0, st) == MVHP_SUCCESS && c0.bad == 0 && c0.ok == n_idr);
                g_stub.caps |= mvengine::CAP_ORIENT;
            }
            {   // a malformed request: the box must still be well formed
                mvhp_engine_opts_t o = base; o.contexts = 1;
                mvhp_engine_t *e = nullptr;
                EXPECT(mvhp_engine_create(&o, &e) == MVHP_SUCCESS);
                const mvhp_output_request_t bad{MVHP_OUTPUT_BOX | MVHP_OUTPUT_ROTATE(1), 1, 40, 0}, unknown{64u, 0, 0, 0};
                mvhp_decode_stats_t st;
                EXPECT(mvhp_engine_decode_ex(e, &s3, o3.data(), n3, n3, 0, &bad, nullptr, nullptr, &st) == MVHP_FAILURE);
                EXPECT(mvhp_engine_decode_ex(e, &s3, o3.data(), n3, n3, 0, &unknown, nullptr, nullptr, &st) == MVHP_FAILURE);
                mvhp_engine_destroy(e);
            }
            {   // minivideo_decode under MINIVIDEO_ROTATE: files of the turned size; malformed values fail before the device is touched
                char tmpl[] = "/tmp/mvharness_XXXXXX";
                const char *dir = mkdtemp(tmpl);
                char cwd[4096];
                EXPECT(dir != nullptr && getcwd(cwd, sizeof(cwd)) != nullptr);
                std::string in = argv[4];
                if (in[0] != '/') in = std::string(cwd) + "/" + in;
                EXPECT(dir && chdir(dir) == 0);
                struct Sw { const char *rotate, *thumb; mvhp_output_request_t req; };
                const Sw sws[] = {{"90", nullptr, mvhp_output_request_t{MVHP_OUTPUT_ROTATE(1), 0, 0, 0}},
                                  {"270", "40x24", mvhp_output_request_t{MVHP_OUTPUT_CROP | MVHP_OUTPUT_BOX | MVHP_OUTPUT_ROTATE(3), 40, 24, 0}},
                                  {"180", nullptr, mvhp_output_request_t{MVHP_OUTPUT_ROTATE(2), 0, 0, 0}},
                                  {"auto", nullptr, mvhp_output_request_t{}}, {"0", nullptr, mvhp_output_request_t{}}, {"", nullptr, mvhp_output_request_t{}}};
                for (const Sw &sw : sws)
                    for (int fmt : {PICTURE_YUV420, PICTURE_BMP}) {
                        setenv("MINIVIDEO_ROTATE", sw.rotate, 1);
                        if (sw.thumb) setenv("MINIVIDEO_THUMBNAIL", sw.thumb, 1); else unsetenv("MINIVIDEO_THUMBNAIL");
                        MediaFile_t *m = nullptr;
                        EXPECT(minivideo_open(in.c_str(), &m) == SUCCESS);
                        EXPECT(m && minivideo_parse(m, false, true, false) == SUCCESS);
                        EXPECT(m && minivideo_decode(m, ".", fmt, 75, n3, PICTURE_UNFILTERED) == SUCCESS);
                        const int turns = mvhp_output_turns(&s3, &sw.req);
                        int good = 0, k = 0, expected = 0;
                        for (int idr = 0; idr < n3; idr++) {
                            mvhp_output_geometry_t g;
                            if (mvhp_output_geometry(&s3, idr, &sw.req, &g) != MVHP_SUCCESS) continue;
                            expected++;
                            const std::string name = std::string(m->file_name) + "_" + std::to_string(k++) + (fmt == PICTURE_BMP ? ".bmp" : ".yuv");
                            const std::vector<uint8_t> f = read_file(name);
                            if (f.empty()) continue;
                            remove(name.c_str());
                            const uint64_t h = picture_checksum(s3, idr);
                            uint64_t got = 0;
                            if (fmt == PICTURE_YUV420) {
                                if (f.size() != mvhp_geometry_yuv_bytes(&g)) continue;
                                memcpy(&got, f.data(), 8);
                                if (got == h && f.back() == (turns ? kLastYuv : 0x5a)) good++;
                            } else {
                                const std::vector<uint8_t> rgb = bmp_pixels(f, (int)g.out_w, (int)g.out_h);
                                if (rgb.size() != mvhp_geometry_rgb_bytes(&g)) continue;
                                memcpy(&got, rgb.data() + 8, 8);
                                if (got == h && rgb.back() == (turns ? kLastRgb : 0xa5)) good++;
                            }
                        }
                        printf("%-28s rotate='%s' thumbnail=%s format=%d files right in %d of %d\n", "public API, orientation", sw.rotate,
                               sw.thumb ? sw.thumb : "-", fmt, good, expected);
                        EXPECT(expected >= 4 && good == expected);
                        EXPECT(minivideo_close(&m) == SUCCESS);
                    }
                unsetenv("MINIVIDEO_THUMBNAIL");
                for (const char *bad : {"45", "90x", "Auto", " 90", "-90", "360"}) {
                    setenv("MINIVIDEO_ROTATE", bad, 1);
                    MediaFile_t *m = nullptr;
                    EXPECT(minivideo_open(in.c_str(), &m) == SUCCESS);
                    EXPECT(m && minivideo_parse(m, false, true, false) == SUCCESS);
                    const int ctx_before = g_ctx_created, recon_before = g_recon_calls + g_geometry_calls;
                    fflush(stdout);
                    fflush(stderr);
                    int pipefd[2];
                    EXPECT(pipe(pipefd) == 0);
                    const int saved = dup(2);
                    dup2(pipefd[1], 2);
                    const int rc = m ? minivideo_decode(m, ".", PICTURE_YUV420, 75, n3, PICTURE_UNFILTERED) : SUCCESS;
                    fflush(stderr);
                    dup2(saved, 2);
                    close(saved);
                    close(pipefd[1]);
                    char msg[512] = "";
                    const ssize_t got = read(pipefd[0], msg, sizeof(msg) - 1);
                    close(pipefd[0]);
                    printf("%-28s '%s' rc=%d message: %s", "malformed rotation", bad, rc, got > 0 ? msg : "(none)\n");
                    EXPECT(rc == FAILURE && got > 0 && strstr(msg, "MINIVIDEO_ROTATE") != nullptr);
                    EXPECT(g_ctx_created == ctx_before && g_recon_calls + g_geometry_calls == recon_before);
                    EXPECT(minivideo_close(&m) == SUCCESS);
                }
                unsetenv("MINIVIDEO_ROTATE");
                EXPECT(chdir(cwd) == 0);
                rmdir(dir);
            }
            printf("ORIENT MODE DONE\n");
        }
        if (argc > 6 && !strcmp(argv[5], "color")) {   // ---- color mode: MVHP_OUTPUT_ASPECT / MVHP_OUTPUT_COLOR against the stub's colour pass ----
            std::vector<uint8_t> b4 = read_file(argv[6]);
            mvhp_stream s4;   // every SPS carries SAR 4:3 and a crop; even SPSs say BT.709 full range, odd ones BT.601 limited
            s4.data = b4.data();
            s4.size = b4.size();
            EXPECT(s4.build(err) == h264::RC_SUCCESS);
            const int n4 = (int)s4.idrs.size();
            EXPECT(n4 >= 6);
            std::vector<int> o4((size_t)n4);
            for (int i = 0; i < n4; i++) o4[(size_t)i] = i;
            auto run_c = [&](const char *name, mvhp_engine_opts_t o, const mvhp_stream &st, const std::vector<int> &order, int mask,
                             const mvhp_output_request_t &req, CheckC &c, mvhp_decode_stats_t &stats) {
                mvhp_engine_t *e = nullptr;
                if (mvhp_engine_create(&o, &e) != MVHP_SUCCESS) { failures++; return MVHP_FAILURE; }
                c.s = &st; c.req = req; c.order = order;
                c.png = mask == MVHP_OUT_PNG;
                c.want_rgb = !c.png && (mask & 1) != 0;
                c.want_yuv = !c.png && (!c.want_rgb || (mask & 2) == 0);
                const int rc = mvhp_engine_decode_ex(e, &st, order.data(), (int)order.size(), (int)order.size(), mask, &req, CheckC::sink, &c, &stats);
                mvhp_engine_destroy(e);
                printf("%-28s flags=%#x kind=%d rc=%d ok=%u failed=%u batches=%u geometry=%u d2h=%llu\n", name, req.flags, mask, rc, stats.pictures_ok,
                       stats.pictures_failed, stats.batches, stats.geometry_launches, (unsigned long long)stats.d2h_bytes);
                return rc;
            };
            {   // the display information and the aspect rule behind the geometry
                mvhp_display_info_t d0, d1;
                EXPECT(mvhp_stream_display(&s4, 0, &d0) == MVHP_SUCCESS && mvhp_stream_display(&s4, 1, &d1) == MVHP_SUCCESS);
                EXPECT(d0.sar_w == 4 && d0.sar_h == 3 && d1.sar_w == 4 && d1.sar_h == 3 && d0.matrix_coefficients == 1 && d0.full_range == 1 &&
                       d1.matrix_coefficients == 6 && d1.full_range == 0);
                mvhp_output_geometry_t gc, ga, gb;
                const mvhp_output_request_t rc_{MVHP_OUTPUT_CROP, 0, 0, 0}, ra{MVHP_OUTPUT_ASPECT, 0, 0, 0}, rb{MVHP_OUTPUT_ASPECT | MVHP_OUTPUT_BOX, 40, 40, 0};
                EXPECT(mvhp_output_geometry(&s4, 0, &rc_, &gc) == MVHP_SUCCESS && mvhp_output_geometry(&s4, 0, &ra, &ga) == MVHP_SUCCESS &&
                       mvhp_output_geometry(&s4, 0, &rb, &gb) == MVHP_SUCCESS);
                EXPECT(ga.crop_w == gc.crop_w && ga.crop_h == gc.crop_h && ga.out_w == gc.crop_w &&
                       ga.out_h == std::max(2u, 2 * ((gc.crop_h * 3 + 4) / 8)) && ga.out_h < gc.crop_h);
                uint32_t fw = 0, fh = 0;
                EXPECT(mvhp_geometry_fit(ga.out_w, ga.out_h, 40, 40, &fw, &fh) == MVHP_SUCCESS && gb.out_w == fw && gb.out_h == fh);
            }
            // every output kind that has RGB x every shape x auto and a forced mode: each picture carries its own setting, batches split
            // where the setting changes (auto: at every picture of this stream; forced: nowhere, the siting being the same), the
            // buffers hold n pictures of the geometry, and only what is delivered is downloaded
            for (int mask : {MVHP_OUT_RGB, MVHP_OUT_RGB_ONLY, MVHP_OUT_PNG})
                for (uint32_t shape : {0u, (uint32_t)MVHP_OUTPUT_CROP, (uint32_t)(MVHP_OUTPUT_CROP | MVHP_OUTPUT_BOX), (uint32_t)MVHP_OUTPUT_ASPECT,
                                       (uint32_t)(MVHP_OUTPUT_ASPECT | MVHP_OUTPUT_BOX), (uint32_t)(MVHP_OUTPUT_ASPECT | MVHP_OUTPUT_ROTATE(1))})
                    for (int mode : {0, 4}) {
                        const mvhp_output_request_t req{shape | MVHP_OUTPUT_COLOR | MVHP_OUTPUT_COLOR_MODE(mode), 40, 24, 0};
                        mvhp_output_request_t plain = req;
                        plain.flags &= ~(MVHP_OUTPUT_COLOR | MVHP_OUTPUT_COLOR_MODE_MASK);
                        mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 2; o.batch_pictures = 64;
                        CheckC c, c0; mvhp_decode_stats_t st, st0;
                        const int color0 = g_color_calls;
                        EXPECT(run_c("color", o, s4, o4, mask, req, c, st) == MVHP_SUCCESS);
                        EXPECT(c.bad == 0 && c.ok == n4 && g_color_calls - color0 == (int)st.batches && st.d2h_bytes == c.bytes);
                        const int color1 = g_color_calls;
                        EXPECT(run_c("the same without the flag", o, s4, o4, mask, plain, c0, st0) == MVHP_SUCCESS);
                        EXPECT(c0.bad == 0 && c0.ok == n4 && g_color_calls == color1 && st0.d2h_bytes == c0.bytes && st.d2h_bytes == st0.d2h_bytes);
                        EXPECT(st.geometry_launches == (shape ? st.batches : 0u));
                        if (mode == 0) {
                            EXPECT((int)st.batches == n4);   // the setting changes at every picture
                            if (mask != MVHP_OUT_PNG) { int kinds = 0; for (int k : c.settings_seen) kinds += k > 0; EXPECT(kinds == 2); }
                        } else {
                            EXPECT(st.batches == st0.batches);   // one setting: the batches of the request without the flag
                            if (mask != MVHP_OUT_PNG) { int kinds = 0; for (int k : c.settings_seen) kinds += k > 0; EXPECT(kinds == 1); }
                        }
                    }
            {   // the flag where no RGB is delivered -- planes, JPEG -- changes nothing and runs no colour pass
                const int color0 = g_color_calls;
                mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 2; o.batch_pictures = 64;
                for (uint32_t shape : {0u, (uint32_t)MVHP_OUTPUT_ASPECT}) {
                    const mvhp_output_request_t req{shape | MVHP_OUTPUT_COLOR, 0, 0, 0}, plain{shape, 0, 0, 0};
                    CheckC c, c0; mvhp_decode_stats_t st, st0;
                    EXPECT(run_c("color: planes only", o, s4, o4, 0, req, c, st) == MVHP_SUCCESS && c.bad == 0 && c.ok == n4);
                    EXPECT(run_c("the same without the flag", o, s4, o4, 0, plain, c0, st0) == MVHP_SUCCESS && c0.bad == 0);
                    EXPECT(st.batches == st0.batches && st.geometry_launches == st0.geometry_launches && st.d2h_bytes == st0.d2h_bytes);
                }
                const mvhp_output_request_t jreq{MVHP_OUTPUT_CROP | MVHP_OUTPUT_COLOR, 0, 0, MVHP_JPEG_REQUEST(80, 0)};
                mvhp_engine_t *e = nullptr;
                EXPECT(mvhp_engine_create(&o, &e) == MVHP_SUCCESS);
                CheckJ cj; mvhp_decode_stats_t st;
                cj.s = &s4; cj.req = jreq; cj.order = o4;
                EXPECT(mvhp_engine_decode_ex(e, &s4, o4.data(), n4, n4, MVHP_OUT_JPEG, &jreq, CheckJ::sink, &cj, &st) == MVHP_SUCCESS);
                mvhp_engine_destroy(e);
                EXPECT(cj.bad == 0 && cj.ok == (int)st.pictures_ok && cj.ok > 0);
                EXPECT(g_color_calls == color0);
            }
            {   // colour alone at the coded size on a stream without VUI: one setting, the batches of a call without a request
                mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 3; o.batch_pictures = 7;
                CheckC c, c0; mvhp_decode_stats_t st, st0;
                const int geom0 = g_geometry_calls;
                EXPECT(run_c("color: coded size", o, s, all, MVHP_OUT_RGB, mvhp_output_request_t{MVHP_OUTPUT_COLOR, 0, 0, 0}, c, st) == MVHP_SUCCESS);
                EXPECT(run_c("the same without the flag", o, s, all, MVHP_OUT_RGB, mvhp_output_request_t{}, c0, st0) == MVHP_SUCCESS);
                EXPECT(c.bad == 0 && c0.bad == 0 && c.ok == n_idr && st.batches == st0.batches && st.geometry_launches == 0 && g_geometry_calls == geom0);
            }
            {   // small batches, three contexts, the first batch of context 0 fails: re-queued with its setting
                std::vector<int> order;
                for (int k = 0; k < 3 * n4; k++) order.push_back(k % n4);
                const mvhp_output_request_t req{MVHP_OUTPUT_ASPECT | MVHP_OUTPUT_BOX | MVHP_OUTPUT_COLOR, 40, 24, 0};
                mvhp_engine_opts_t o = base; o.contexts = 3; o.chunk_pictures = 2; o.batch_pictures = 3; o.fail_context = 0;
                CheckC c; mvhp_decode_stats_t st;
                EXPECT(run_c("color requeue/3ctx", o, s4, order, MVHP_OUT_RGB, req, c, st) == MVHP_SUCCESS);
                EXPECT(c.bad == 0 && c.ok == (int)order.size() && st.batches_requeued == 1 && st.d2h_bytes == c.bytes);
            }
            {   // a device table without the operation: every picture of a call that asks for it fails with the message
                g_stub.caps &= ~mvengine::CAP_COLOR;
                mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 2; o.batch_pictures = 4;
                CheckC c, c0; mvhp_decode_stats_t st;
                const int color0 = g_color_calls;
                EXPECT(run_c("color: table without it", o, s4, o4, MVHP_OUT_RGB, mvhp_output_request_t{MVHP_OUTPUT_COLOR, 0, 0, 0}, c, st) == MVHP_FAILURE);
                EXPECT(c.bad == 0 && c.ok == 0 && c.no_op == n4 && g_color_calls == color0);
                EXPECT(run_c("color: table without it, planes", o, s4, o4, 0, mvhp_output_request_t{MVHP_OUTPUT_COLOR, 0, 0, 0}, c0, st) == MVHP_SUCCESS && c0.bad == 0 && c0.ok == n4);
                g_stub.caps |= mvengine::CAP_COLOR;
            }
            {   // malformed requests: a colour mode above 4
                mvhp_engine_opts_t o = base; o.contexts = 1;
                mvhp_engine_t *e = nullptr;
                EXPECT(mvhp_engine_create(&o, &e) == MVHP_SUCCESS);
                const mvhp_output_request_t bad{MVHP_OUTPUT_COLOR | MVHP_OUTPUT_COLOR_MODE(5), 0, 0, 0};
                mvhp_decode_stats_t st;
                EXPECT(mvhp_engine_decode_ex(e, &s4, o4.data(), n4, n4, MVHP_OUT_RGB, &bad, nullptr, nullptr, &st) == MVHP_FAILURE);
                mvhp_engine_destroy(e);
            }
            {   // minivideo_decode under MINIVIDEO_ASPECT / MINIVIDEO_COLOR: files of the aspect's size, RGB with the picture's setting;
                // planes are not touched by the colour switch; malformed values fail before the device is touched
                char tmpl[] = "/tmp/mvharness_XXXXXX";
                const char *dir = mkdtemp(tmpl);
                char cwd[4096];
                EXPECT(dir != nullptr && getcwd(cwd, sizeof(cwd)) != nullptr);
                std::string in = argv[6];
                if (in[0] != '/') in = std::string(cwd) + "/" + in;
                EXPECT(dir && chdir(dir) == 0);
                struct Sw { const char *aspect, *color; mvhp_output_request_t req; };
                const Sw sws[] = {{"1", nullptr, mvhp_output_request_t{MVHP_OUTPUT_ASPECT, 0, 0, 0}},
                                  {"1", "auto", mvhp_output_request_t{MVHP_OUTPUT_ASPECT | MVHP_OUTPUT_COLOR, 0, 0, 0}},
                                  {nullptr, "bt709-full", mvhp_output_request_t{MVHP_OUTPUT_COLOR | MVHP_OUTPUT_COLOR_MODE(4), 0, 0, 0}},
                                  {"0", "0", mvhp_output_request_t{}}, {"", "", mvhp_output_request_t{}}};
                for (const Sw &sw : sws)
                    for (int fmt : {PICTURE_YUV420, PICTURE_BMP}) {
                        if (sw.aspect) setenv("MINIVIDEO_ASPECT", sw.aspect, 1); else unsetenv("MINIVIDEO_ASPECT");
                        if (sw.color) setenv("MINIVIDEO_COLOR", sw.color, 1); else unsetenv("MINIVIDEO_COLOR");
                        MediaFile_t *m = nullptr;
                        EXPECT(minivideo_open(in.c_str(), &m) == SUCCESS);
                        EXPECT(m && minivideo_parse(m, false, true, false) == SUCCESS);
                        const int color0 = g_color_calls;
                        EXPECT(m && minivideo_decode(m, ".", fmt, 75, n4, PICTURE_UNFILTERED) == SUCCESS);
                        const bool color = (sw.req.flags & MVHP_OUTPUT_COLOR) != 0 && fmt == PICTURE_BMP;
                        EXPECT((g_color_calls > color0) == color);
                        int good = 0;
                        for (int idr = 0; idr < n4; idr++) {
                            mvhp_output_geometry_t g;
                            mvhp_stream_params_t p;
                            EXPECT(mvhp_output_geometry(&s4, idr, &sw.req, &g) == MVHP_SUCCESS && mvhp_stream_params(&s4, idr, &p) == MVHP_SUCCESS);
                            const std::string name = std::string(m->file_name) + "_" + std::to_string(idr) + (fmt == PICTURE_BMP ? ".bmp" : ".yuv");
                            const std::vector<uint8_t> f = read_file(name);
                            if (f.empty()) continue;
                            remove(name.c_str());
                            const uint64_t h = picture_checksum(s4, idr);
                            const bool coded = g.out_w == p.width_mbs * 16 && g.out_h == p.height_mbs * 16;
                            uint64_t got = 0;
                            if (fmt == PICTURE_YUV420) {
                                if (f.size() != mvhp_geometry_yuv_bytes(&g)) continue;
                                memcpy(&got, f.data(), 8);
                                if (got == h && f.back() == (coded ? 0x5a : kLastYuv)) good++;
                            } else {
                                const std::vector<uint8_t> rgb = bmp_pixels(f, (int)g.out_w, (int)g.out_h);
                                if (rgb.size() != mvhp_geometry_rgb_bytes(&g)) continue;
                                memcpy(&got, rgb.data() + 8, 8);
                                const uint8_t tag = color ? CheckC::expected_tag(&s4, idr, sw.req, &p, &g) : 0xa5;
                                if (got == h && rgb[16] == tag && rgb.back() == (color ? kLastColor : coded ? 0xa5 : kLastRgb)) good++;
                            }
                        }
                        printf("%-28s aspect='%s' color='%s' format=%d files right in %d of %d\n", "public API, display", sw.aspect ? sw.aspect : "-",
                               sw.color ? sw.color : "-", fmt, good, n4);
                        EXPECT(good == n4);
                        EXPECT(minivideo_close(&m) == SUCCESS);
                    }
                struct Bad { const char *var, *value; };
                for (const Bad &b : {Bad{"MINIVIDEO_COLOR", "709"}, Bad{"MINIVIDEO_COLOR", "bt709x"}, Bad{"MINIVIDEO_COLOR", "Auto"}, Bad{"MINIVIDEO_COLOR", "1"},
                                     Bad{"MINIVIDEO_ASPECT", "yes"}, Bad{"MINIVIDEO_ASPECT", "2"}, Bad{"MINIVIDEO_ASPECT", "4:3"}}) {
                    unsetenv("MINIVIDEO_ASPECT"); unsetenv("MINIVIDEO_COLOR");
                    setenv(b.var, b.value, 1);
                    MediaFile_t *m = nullptr;
                    EXPECT(minivideo_open(in.c_str(), &m) == SUCCESS);
                    EXPECT(m && minivideo_parse(m, false, true, false) == SUCCESS);
                    const int ctx_before = g_ctx_created, recon_before = g_recon_calls + g_geometry_calls + g_color_calls;
                    fflush(stdout);
                    fflush(stderr);
                    int pipefd[2];
                    EXPECT(pipe(pipefd) == 0);
                    const int saved = dup(2);
                    dup2(pipefd[1], 2);
                    const int rc = m ? minivideo_decode(m, ".", PICTURE_BMP, 75, n4, PICTURE_UNFILTERED) : SUCCESS;
                    fflush(stderr);
                    dup2(saved, 2);
                    close(saved);
                    close(pipefd[1]);
                    char msg[512] = "";
                    const ssize_t got = read(pipefd[0], msg, sizeof(msg) - 1);
                    close(pipefd[0]);
                    printf("%-28s %s='%s' rc=%d message: %s", "malformed display switch", b.var, b.value, rc, got > 0 ? msg : "(none)\n");
                    EXPECT(rc == FAILURE && got > 0 && strstr(msg, b.var) != nullptr);
                    EXPECT(g_ctx_created == ctx_before && g_recon_calls + g_geometry_calls + g_color_calls == recon_before);
                    EXPECT(minivideo_close(&m) == SUCCESS);
                }
                unsetenv("MINIVIDEO_ASPECT"); unsetenv("MINIVIDEO_COLOR");
                EXPECT(chdir(cwd) == 0);
                rmdir(dir);
            }
            printf("COLOR MODE DONE\n");
        }
        if (argc > 5 && !strcmp(argv[5], "score")) {   // ---- score mode: MVHP_OUTPUT_SCORE against the stub's picture-score operation ----
            std::vector<int> order;
            for (int k = 0; k < 3 * n3; k++) order.push_back(k % n3);
            auto run_score = [&](const char *name, mvhp_engine_opts_t o, int mask, mvhp_output_request_t req, bool flag, CheckS &c,
                                 mvhp_decode_stats_t &stats) {
                mvhp_engine_t *e = nullptr;
                if (mvhp_engine_create(&o, &e) != MVHP_SUCCESS) { failures++; return MVHP_FAILURE; }
                c.s = &s3; c.req = req; c.order = order; c.mask = mask;
                if (flag) req.flags |= MVHP_OUTPUT_SCORE;
                const int rc = mvhp_engine_decode_ex(e, &s3, order.data(), (int)order.size(), (int)order.size(), mask, &req, CheckS::sink, &c, &stats);
                mvhp_engine_destroy(e);
                printf("%-28s rc=%d mask=%d flags=%u ok=%u failed=%u batches=%u geometry=%u requeued=%u d2h=%llu\n", name, rc, mask, req.flags,
                       stats.pictures_ok, stats.pictures_failed, stats.batches, stats.geometry_launches, stats.batches_requeued,
                       (unsigned long long)stats.d2h_bytes);
                return rc;
            };
            int distinct_checked = 0;
            for (int contexts = 1; contexts <= 3; contexts++)
                for (int mask : {0, MVHP_OUT_RGB, MVHP_OUT_RGB_ONLY, MVHP_OUT_JPEG})
                    for (mvhp_output_request_t req : {mvhp_output_request_t{0, 0, 0, 0}, crop, box}) {
                        if (mask == MVHP_OUT_JPEG) req.reserved = MVHP_JPEG_REQUEST(80, 0);
                        mvhp_engine_opts_t o = base; o.contexts = contexts; o.chunk_pictures = 2; o.batch_pictures = contexts == 1 ? 64 : 3;
                        // without the flag: the sink's geometry has reserved[1] = 0 (CheckG / CheckJ compare all of it) and the
                        // operation is never called
                        mvhp_decode_stats_t st0;
                        const int calls0 = g_stats_calls;
                        if (mask == MVHP_OUT_JPEG) {
                            CheckJ cj; cj.s = &s3; cj.req = req; cj.order = order;
                            mvhp_engine_t *e = nullptr;
                            EXPECT(mvhp_engine_create(&o, &e) == MVHP_SUCCESS);
                            EXPECT(mvhp_engine_decode_ex(e, &s3, order.data(), (int)order.size(), (int)order.size(), mask, &req, CheckJ::sink, &cj, &st0) == MVHP_SUCCESS);
                            mvhp_engine_destroy(e);
                            EXPECT(cj.bad == 0);
                        } else {
                            CheckG cg;
                            EXPECT(run_ex("score: flag off", o, s3, order, mask, req, cg, st0) == MVHP_SUCCESS);
                            EXPECT(cg.bad == 0);
                        }
                        EXPECT(g_stats_calls == calls0);
                        // with it (three contexts: the first batch of context 0 fails and is re-queued, and scored again)
                        o.fail_context = contexts == 3 ? 0 : -1;
                        CheckS c; mvhp_decode_stats_t st;
                        EXPECT(run_score(req.flags & MVHP_OUTPUT_BOX ? "score box" : req.flags ? "score crop" : "score coded size", o, mask, req,
                                         true, c, st) == MVHP_SUCCESS);
                        EXPECT(c.bad == 0 && c.no_op == 0 && c.calls == (int)order.size() && c.ok == (int)st.pictures_ok && c.ok + c.failed == c.calls);
                        EXPECT(c.ok == (int)st0.pictures_ok);
                        EXPECT(st.d2h_bytes == st0.d2h_bytes + 32ull * (uint64_t)c.formed_n);   // exactly one record per picture of a batch
                        EXPECT((int)st.batches_requeued == (contexts == 3 ? 1 : 0));
                        EXPECT(g_stats_calls - calls0 == (int)st.batches);   // one call behind every launch that succeeded
                        if (!req.flags) EXPECT(st.geometry_launches == 0);   // the flag alone: still the coded-size path
                        std::vector<uint32_t> d = c.scores;
                        std::sort(d.begin(), d.end());
                        if (std::unique(d.begin(), d.end()) - d.begin() >= 3) distinct_checked++;
                    }
            // The scores tell pictures apart in 27 of the 36 runs: there the stub's planes are the picture's repeated checksum.  In the
            // 9 coded-size runs without JPEG its planes are 0x5a past their first 8 bytes, and the scores of pictures nearly agree.
            EXPECT(distinct_checked >= 27);
            {   // a device table without the operation: every picture of the call fails with the message
                g_stub.caps &= ~mvengine::CAP_SCORE;
                mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 2; o.batch_pictures = 4;
                CheckS c; mvhp_decode_stats_t st;
                const int calls0 = g_stats_calls, recon0 = g_recon_calls + g_geometry_calls + g_jpeg_calls;
                EXPECT(run_score("score: table without it", o, 0, crop, true, c, st) == MVHP_FAILURE);
                EXPECT(c.bad == 0 && c.ok == 0 && c.no_op == c.formed_n && c.no_op > 0 && g_stats_calls == calls0);
                EXPECT(g_recon_calls + g_geometry_calls + g_jpeg_calls == recon0);
                CheckG cg;   // ... and a call without the flag is not affected
                EXPECT(run_ex("score: table without it, off", o, s3, order, 0, crop, cg, st) == MVHP_SUCCESS && cg.bad == 0);
                g_stub.caps |= mvengine::CAP_SCORE;
            }
            {   // minivideo_decode under MINIVIDEO_SKIP_BLANK=1 on the stub device: two engine calls on one engine, the second one's
                // files written over the first one's.  With the threshold at its maximum every stub picture is blank, so each slot
                // with alternates ends on the highest score among its candidates; the files start with the records' checksum.
                char tmpl[] = "/tmp/mvharness_XXXXXX";
                const char *dir = mkdtemp(tmpl);
                char cwd[4096];
                EXPECT(dir != nullptr && getcwd(cwd, sizeof(cwd)) != nullptr);
                std::string in = argv[4];
                if (in[0] != '/') in = std::string(cwd) + "/" + in;
                EXPECT(dir && chdir(dir) == 0);
                setenv("MINIVIDEO_SKIP_BLANK", "1", 1);
                setenv("MINIVIDEO_BLANK_VARIANCE", "16256", 1);
                setenv("MINIVIDEO_BLANK_ALTERNATES", "3", 1);
                std::vector<uint32_t> sc((size_t)n3);
                for (int idr = 0; idr < n3; idr++) {
                    mvhp_stream_params_t p;
                    mvhp_output_geometry_t g;
                    EXPECT(mvhp_stream_params(&s3, idr, &p) == MVHP_SUCCESS && mvhp_output_geometry(&s3, idr, nullptr, &g) == MVHP_SUCCESS);
                    const mvhp_luma_stats_t st = expected_stats(picture_checksum(s3, idr), false, &p, &g);
                    sc[(size_t)idr] = mvblank::luma_score(st.sum, st.sumsq, st.samples);
                }
                int moved = 0;
                for (int num : {1, 2, n3 - 2})
                    for (const char *writers : {"2", "0"}) {
                        setenv("MINIVIDEO_WRITERS", writers, 1);
                        MediaFile_t *m = nullptr;
                        EXPECT(minivideo_open(in.c_str(), &m) == SUCCESS);
                        EXPECT(m && minivideo_parse(m, false, true, false) == SUCCESS);
                        const int calls0 = g_stats_calls;
                        EXPECT(m && minivideo_decode(m, ".", PICTURE_YUV420, 75, num, PICTURE_UNFILTERED) == SUCCESS);
                        EXPECT(g_stats_calls > calls0);
                        std::vector<int> slots;
                        for (int k = 0; k < num; k++) slots.push_back(k);
                        int good = 0;
                        for (int k = 0; k < num; k++) {
                            std::vector<int> cand{slots[(size_t)k]};
                            for (int i : mvblank::alternates(slots, n3, 3, k)) cand.push_back(i);
                            std::vector<uint32_t> v;
                            for (int i : cand) v.push_back(sc[(size_t)i]);
                            const int final_idr = cand[(size_t)mvblank::choose(v.data(), (int)v.size(), 16u * 16256u)];
                            if (final_idr != slots[(size_t)k]) moved++;
                            const std::string name = std::string(m->file_name) + (num > 1 ? "_" + std::to_string(k) : "") + ".yuv";
                            const std::vector<uint8_t> f = read_file(name);
                            remove(name.c_str());
                            uint64_t got = 0;
                            if (f.size() >= 8) memcpy(&got, f.data(), 8);
                            if (got == picture_checksum(s3, final_idr)) good++;
                        }
                        printf("%-28s n=%d writers=%s right picture in %d files\n", "public API, blank pictures", num, writers, good);
                        EXPECT(good == num);
                        EXPECT(minivideo_close(&m) == SUCCESS);
                    }
                EXPECT(moved >= 1);   // (some slot did give way to an alternate)
                unsetenv("MINIVIDEO_SKIP_BLANK"); unsetenv("MINIVIDEO_BLANK_VARIANCE"); unsetenv("MINIVIDEO_BLANK_ALTERNATES"); unsetenv("MINIVIDEO_WRITERS");
                EXPECT(chdir(cwd) == 0);
                rmdir(dir);
            }
            // malformed values of the three switches of minivideo_decode: FAILURE, with a message, before the device is touched
            struct Bad { const char *var, *value; };
            for (const Bad &b : {Bad{"MINIVIDEO_BLANK_VARIANCE", "abc"}, Bad{"MINIVIDEO_BLANK_VARIANCE", "-1"}, Bad{"MINIVIDEO_BLANK_VARIANCE", "16257"},
                                 Bad{"MINIVIDEO_BLANK_ALTERNATES", "0"}, Bad{"MINIVIDEO_BLANK_ALTERNATES", "17"}, Bad{"MINIVIDEO_SKIP_BLANK", "yes"}}) {
                setenv("MINIVIDEO_SKIP_BLANK", "1", 1);
                setenv(b.var, b.value, 1);
                MediaFile_t *m = nullptr;
                EXPECT(minivideo_open(argv[4], &m) == SUCCESS);
                EXPECT(m && minivideo_parse(m, false, true, false) == SUCCESS);
                const int ctx_before = g_ctx_created, launches_before = g_recon_calls + g_geometry_calls + g_stats_calls;
                fflush(stdout);
                fflush(stderr);
                int pipefd[2];
                EXPECT(pipe(pipefd) == 0);
                const int saved = dup(2);
                dup2(pipefd[1], 2);
                const int rc = m ? minivideo_decode(m, ".", PICTURE_YUV420, 75, n3, PICTURE_UNFILTERED) : SUCCESS;
                fflush(stderr);
                dup2(saved, 2);
                close(saved);
                close(pipefd[1]);
                char msg[512] = "";
                const ssize_t got = read(pipefd[0], msg, sizeof(msg) - 1);
                close(pipefd[0]);
                printf("%-28s %s='%s' rc=%d message: %s", "malformed blank switch", b.var, b.value, rc, got > 0 ? msg : "(none)\n");
                EXPECT(rc == FAILURE && got > 0 && strstr(msg, b.var) != nullptr);
                EXPECT(g_ctx_created == ctx_before && g_recon_calls + g_geometry_calls + g_stats_calls == launches_before);
                EXPECT(minivideo_close(&m) == SUCCESS);
                unsetenv(b.var);
            }
            unsetenv("MINIVIDEO_SKIP_BLANK");
            printf("SCORE MODE DONE\n");
        }
        if (argc > 5 && !strcmp(argv[5], "hist")) {   // ---- hist mode: MVHP_OUTPUT_HIST against the stub's plane-histogram operation ----
            std::vector<int> order;
            for (int k = 0; k < 3 * n3; k++) order.push_back(k % n3);
            auto run_hist = [&](const char *name, mvhp_engine_opts_t o, int mask, mvhp_output_request_t req, uint32_t extra, CheckH &c,
                                mvhp_decode_stats_t &stats) {
                mvhp_engine_t *e = nullptr;
                if (mvhp_engine_create(&o, &e) != MVHP_SUCCESS) { failures++; return MVHP_FAILURE; }
                c.base.s = &s3; c.base.req = req; c.base.order = order; c.base.mask = mask;
                c.e = e; c.n_order = (int)order.size();
                c.flag = (extra & MVHP_OUTPUT_HIST) != 0; c.scored = (extra & MVHP_OUTPUT_SCORE) != 0;
                req.flags |= extra;
                const int rc = mvhp_engine_decode_ex(e, &s3, order.data(), (int)order.size(), (int)order.size(), mask, &req, CheckH::sink, &c, &stats);
                for (int k = -1; k <= (int)order.size(); k++) EXPECT(mvhp_engine_picture_hist(e, k) == nullptr);   // the call is over
                mvhp_engine_destroy(e);
                printf("%-28s rc=%d mask=%d flags=%#x ok=%u failed=%u batches=%u geometry=%u requeued=%u d2h=%llu records=%d kept=%d\n", name, rc, mask,
                       req.flags, stats.pictures_ok, stats.pictures_failed, stats.batches, stats.geometry_launches, stats.batches_requeued,
                       (unsigned long long)stats.d2h_bytes, c.records, c.kept_checked);
                return rc;
            };
            EXPECT(mvhp_engine_picture_hist(nullptr, 0) == nullptr);
            for (int contexts = 1; contexts <= 3; contexts++)
                for (int mask : {0, MVHP_OUT_RGB, MVHP_OUT_RGB_ONLY, MVHP_OUT_JPEG})
                    for (mvhp_output_request_t req : {mvhp_output_request_t{0, 0, 0, 0}, crop, box}) {
                        if (mask == MVHP_OUT_JPEG) req.reserved = MVHP_JPEG_REQUEST(80, 0);
                        mvhp_engine_opts_t o = base; o.contexts = contexts; o.chunk_pictures = 2; o.batch_pictures = contexts == 1 ? 64 : 3;
                        // without the flag: the same pictures, no record, the operation never called
                        const int calls0 = g_hist_calls;
                        CheckH c0; mvhp_decode_stats_t st0;
                        EXPECT(run_hist("hist: flag off", o, mask, req, 0, c0, st0) == MVHP_SUCCESS);
                        EXPECT(c0.bad == 0 && c0.base.bad == 0 && c0.records == 0 && g_hist_calls == calls0);
                        // with it (three contexts: the first batch of context 0 fails and is re-queued, and counted again), alone and
                        // beside the score
                        o.fail_context = contexts == 3 ? 0 : -1;
                        for (uint32_t extra : {(uint32_t)MVHP_OUTPUT_HIST, (uint32_t)(MVHP_OUTPUT_HIST | MVHP_OUTPUT_SCORE)}) {
                            const int calls1 = g_hist_calls, stats1 = g_stats_calls;
                            CheckH c; mvhp_decode_stats_t st;
                            EXPECT(run_hist(req.flags & MVHP_OUTPUT_BOX ? "hist box" : req.flags ? "hist crop" : "hist coded size", o, mask, req, extra, c,
                                            st) == MVHP_SUCCESS);
                            EXPECT(c.bad == 0 && c.base.bad == 0 && c.base.no_op == 0 && c.base.calls == (int)order.size());
                            EXPECT(c.base.ok == (int)st.pictures_ok && c.base.ok == (int)st0.pictures_ok && c.records == c.base.ok && c.kept_checked > 0);
                            const uint64_t per = 3104ull + ((extra & MVHP_OUTPUT_SCORE) ? 32ull : 0ull);
                            EXPECT(st.d2h_bytes == st0.d2h_bytes + per * (uint64_t)c.base.formed_n);   // exactly one record per picture of a batch
                            EXPECT((int)st.batches_requeued == (contexts == 3 ? 1 : 0));
                            EXPECT(g_hist_calls - calls1 == (int)st.batches);   // one call behind every launch that succeeded
                            EXPECT(g_stats_calls - stats1 == ((extra & MVHP_OUTPUT_SCORE) ? (int)st.batches : 0));
                            if (!req.flags) EXPECT(st.geometry_launches == 0);   // the flag alone: still the coded-size path
                        }
                    }
            {   // a device table without the operation: every picture of the call fails with the message, nothing is launched
                g_stub.caps &= ~mvengine::CAP_HIST;
                mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 2; o.batch_pictures = 4;
                mvhp_engine_t *e = nullptr;
                EXPECT(mvhp_engine_create(&o, &e) == MVHP_SUCCESS);
                struct NoOp { mvhp_engine_t *e; int calls = 0, no_op = 0, other = 0, records = 0; } n{e};
                auto sink = [](void *user, int seq, int, int rc, const char *err, const mvhp_stream_params_t *, const mvhp_output_geometry_t *,
                               const uint8_t *, const uint8_t *) {
                    NoOp &c = *static_cast<NoOp *>(user);
                    c.calls++;
                    if (rc != MVHP_SUCCESS && err && strstr(err, "plane-histogram operation")) c.no_op++;
                    else if (rc == MVHP_SUCCESS) c.other++;
                    if (mvhp_engine_picture_hist(c.e, seq)) c.records++;
                    return 0;
                };
                mvhp_output_request_t req = crop;
                req.flags |= MVHP_OUTPUT_HIST;
                mvhp_decode_stats_t st;
                const int calls0 = g_hist_calls, recon0 = g_recon_calls + g_geometry_calls + g_jpeg_calls;
                int formed = 0;
                for (int idr : order) { mvhp_output_geometry_t g; formed += mvhp_output_geometry(&s3, idr, &crop, &g) == MVHP_SUCCESS; }
                const int rc = mvhp_engine_decode_ex(e, &s3, order.data(), (int)order.size(), (int)order.size(), 0, &req, sink, &n, &st);
                printf("%-28s rc=%d calls=%d no operation=%d\n", "hist: table without it", rc, n.calls, n.no_op);
                EXPECT(rc == MVHP_FAILURE && n.other == 0 && n.records == 0 && n.no_op == formed && formed > 0 && g_hist_calls == calls0);
                EXPECT(g_recon_calls + g_geometry_calls + g_jpeg_calls == recon0);
                mvhp_engine_destroy(e);
                CheckG cg;   // ... and a call without the flag is not affected
                EXPECT(run_ex("hist: table without it, off", o, s3, order, 0, crop, cg, st) == MVHP_SUCCESS && cg.bad == 0);
                g_stub.caps |= mvengine::CAP_HIST;
            }
            {   // two probes in one call are refused, with a message and before any work
                mvhp_engine_opts_t o = base; o.contexts = 1;
                std::string why;
                mvengine::Engine *pe = mvengine::engine_create(g_stub, &o, why);
                EXPECT(pe != nullptr);
                const int launches0 = g_recon_calls + g_geometry_calls + g_bars_calls + g_hist_calls;
                mvhp_output_request_t req{MVHP_OUTPUT_HIST | MVHP_OUTPUT_BARS, 0, 0, 0};
                CheckB c; c.s = &s3; c.order = order; mvhp_decode_stats_t st;
                const int rc = pe ? mvengine::engine_decode(pe, s3, order.data(), (int)order.size(), (int)order.size(), 0, &req, nullptr, CheckB::sink, &c,
                                                            &st, why) : MVHP_SUCCESS;
                printf("%-28s rc=%d message: %s\n", "hist with bars", rc, why.c_str());
                EXPECT(rc == MVHP_FAILURE && c.calls == 0 && why.find("MVHP_OUTPUT_HIST") != std::string::npos && why.find("MVHP_OUTPUT_BARS") != std::string::npos);
                EXPECT(pe && mvengine::engine_picture_hist(pe, 0) == nullptr);
                if (pe) mvengine::engine_destroy(pe);
                EXPECT(g_recon_calls + g_geometry_calls + g_bars_calls + g_hist_calls == launches0);
            }
            {   // minivideo_decode under MINIVIDEO_REPRESENTATIVE=1 on the stub device: three engine calls on one engine.  The stub's
                // histograms are functions of the records' checksum and the rectangle, so the winners, the order lists of passes 2
                // and 3 (the second stats line) and the files -- which start with the records' checksum -- are known beforehand.
                char tmpl[] = "/tmp/mvharness_XXXXXX";
                const char *dir = mkdtemp(tmpl);
                char cwd[4096];
                EXPECT(dir != nullptr && getcwd(cwd, sizeof(cwd)) != nullptr);
                std::string in = argv[4];
                if (in[0] != '/') in = std::string(cwd) + "/" + in;
                EXPECT(dir && chdir(dir) == 0);
                setenv("MINIVIDEO_REPRESENTATIVE", "1", 1);
                setenv("MINIVIDEO_STATS", "1", 1);
                struct Case { const char *name; bool crop; const char *blank_variance; const char *alts; int num; const char *batch, *gpus, *writers; };
                int moved = 0, resized = 0, blank_ruled = 0;
                for (const Case &cs : {Case{"plain", false, nullptr, nullptr, 1, nullptr, nullptr, "0"},
                                       Case{"plain, batches of 1", false, nullptr, nullptr, 1, "1", nullptr, "0"},
                                       Case{"plain, 3 contexts", false, nullptr, nullptr, 1, nullptr, "3", "2"},
                                       Case{"3 alternates, 4 files", false, nullptr, "3", 4, nullptr, nullptr, "2"},
                                       Case{"3 alternates, 4 files, b=1", false, nullptr, "3", 4, "1", "3", "0"},
                                       Case{"all files: no alternates", false, nullptr, nullptr, n3, nullptr, nullptr, "2"},
                                       Case{"cropped", true, nullptr, "16", 2, nullptr, nullptr, "0"},
                                       Case{"cropped, batches of 1", true, nullptr, "16", 2, "1", "3", "0"},
                                       Case{"cropped, with blank skipping", true, "5000", "16", 2, nullptr, nullptr, "0"},
                                       Case{"all blank", false, "16256", "5", 2, nullptr, nullptr, "0"}}) {
                    const int a = cs.alts ? atoi(cs.alts) : 8;
                    if (cs.alts) setenv("MINIVIDEO_REPRESENTATIVE_ALTERNATES", cs.alts, 1); else unsetenv("MINIVIDEO_REPRESENTATIVE_ALTERNATES");
                    if (cs.crop) setenv("MINIVIDEO_CROP", "1", 1); else unsetenv("MINIVIDEO_CROP");
                    if (cs.batch) setenv("MINIVIDEO_BATCH", cs.batch, 1); else unsetenv("MINIVIDEO_BATCH");
                    if (cs.gpus) setenv("MINIVIDEO_FAKE_GPUS", cs.gpus, 1); else unsetenv("MINIVIDEO_FAKE_GPUS");
                    setenv("MINIVIDEO_WRITERS", cs.writers, 1);
                    if (cs.blank_variance) {
                        setenv("MINIVIDEO_SKIP_BLANK", "1", 1);
                        setenv("MINIVIDEO_BLANK_VARIANCE", cs.blank_variance, 1);
                        setenv("MINIVIDEO_BLANK_ALTERNATES", "1", 1);   // (not read: the alternates are the representative switch's)
                    } else { unsetenv("MINIVIDEO_SKIP_BLANK"); unsetenv("MINIVIDEO_BLANK_VARIANCE"); unsetenv("MINIVIDEO_BLANK_ALTERNATES"); }
                    const uint32_t min_score = 16u * (uint32_t)(cs.blank_variance ? atoi(cs.blank_variance) : 256);
                    // what must happen.  Unfiltered: the slots are the first `num` pictures that decode (under the crop IDRs
                    // whose crop leaves nothing fail and the next one takes the slot)
                    const mvhp_output_request_t r1{cs.crop ? MVHP_OUTPUT_CROP : 0u, 0, 0, 0};
                    std::vector<int> slots;
                    for (int idr = 0; idr < n3 && (int)slots.size() < cs.num; idr++) {
                        mvhp_output_geometry_t g;
                        if (mvhp_output_geometry(&s3, idr, &r1, &g) == MVHP_SUCCESS) slots.push_back(idr);
                    }
                    auto hist_of = [&](int idr, mvhp_plane_hist_t &h) {
                        mvhp_output_geometry_t g;
                        mvhp_stream_params_t p;
                        if (mvhp_output_geometry(&s3, idr, &r1, &g) != MVHP_SUCCESS || mvhp_stream_params(&s3, idr, &p) != MVHP_SUCCESS) return false;
                        const bool coded = g.crop_x == 0 && g.crop_y == 0 && g.out_w == p.width_mbs * 16 && g.out_h == p.height_mbs * 16 &&
                                           g.crop_w == g.out_w && g.crop_h == g.out_h;
                        h = expected_hist(picture_checksum(s3, idr), !coded, &p, &g);
                        return true;
                    };
                    std::vector<int> finals, want2, want3;
                    for (int k = 0; k < (int)slots.size(); k++) {
                        std::vector<mvhp_plane_hist_t> cand(1);
                        std::vector<int> cand_idr{slots[(size_t)k]};
                        EXPECT(hist_of(slots[(size_t)k], cand[0]));
                        for (int i : mvblank::alternates(slots, n3, a, k)) {
                            want2.push_back(i);
                            mvhp_plane_hist_t h;
                            if (hist_of(i, h)) { cand.push_back(h); cand_idr.push_back(i); }
                        }
                        std::vector<uint8_t> el;
                        std::vector<uint32_t> sc;
                        for (const mvhp_plane_hist_t &h : cand) {
                            mvhp_luma_stats_t ls;
                            mvrep::hist_stats(h, ls);
                            sc.push_back(mvblank::luma_score(ls.sum, ls.sumsq, ls.samples));
                            el.push_back(sc.back() >= min_score);
                            if (h.samples != cand[0].samples) resized++;
                        }
                        int w = mvrep::choose(cand.data(), (int)cand.size(), cs.blank_variance ? el.data() : nullptr);
                        if (w < 0) { w = mvblank::choose(sc.data(), (int)sc.size(), min_score); blank_ruled++; }
                        finals.push_back(cand_idr[(size_t)w]);
                        if (w > 0) { want3.push_back(cand_idr[(size_t)w]); moved++; }
                    }
                    auto list = [](const std::vector<int> &v) {
                        std::string l;
                        for (int i : v) l += " " + std::to_string(i);
                        return v.empty() ? std::string(" none") : l;
                    };
                    const std::string want_line = "pass 2 order:" + list(want2) + "; pass 3 order:" + list(want3) + "\n";
                    MediaFile_t *m = nullptr;
                    EXPECT(minivideo_open(in.c_str(), &m) == SUCCESS);
                    EXPECT(m && minivideo_parse(m, false, true, false) == SUCCESS);
                    const int calls0 = g_hist_calls, stats0 = g_stats_calls;
                    fflush(stdout);
                    fflush(stderr);
                    char errfile[] = "stderr.txt";
                    const int saved = dup(2);
                    FILE *ef = fopen(errfile, "w");
                    EXPECT(ef != nullptr);
                    if (ef) dup2(fileno(ef), 2);
                    const int rc = m ? minivideo_decode(m, ".", PICTURE_YUV420, 75, cs.num, PICTURE_UNFILTERED) : FAILURE;
                    fflush(stderr);
                    dup2(saved, 2);
                    close(saved);
                    if (ef) fclose(ef);
                    const std::vector<uint8_t> eb = read_file(errfile);
                    remove(errfile);
                    const std::string etext(eb.begin(), eb.end());
                    EXPECT(rc == SUCCESS && g_hist_calls > calls0 && g_stats_calls == stats0);   // (the score comes from the histogram)
                    EXPECT(etext.find(want_line) != std::string::npos);
                    EXPECT(etext.find(std::to_string(want2.size()) + " candidates listed") != std::string::npos);
                    EXPECT(etext.find(std::to_string(want3.size()) + " files replaced") != std::string::npos);
                    EXPECT(etext.find("blank pictures:") == std::string::npos);   // blank skipping's own pass is not run
                    int good = 0;
                    for (int k = 0; k < (int)slots.size(); k++) {
                        const std::string name = std::string(m->file_name) + (cs.num > 1 ? "_" + std::to_string(k) : "") + ".yuv";
                        const std::vector<uint8_t> f = read_file(name);
                        remove(name.c_str());
                        uint64_t got = 0;
                        if (f.size() >= 8) memcpy(&got, f.data(), 8);
                        if (got == picture_checksum(s3, finals[(size_t)k])) good++;
                        EXPECT(read_file(name + ".part").empty());
                    }
                    printf("%-28s %s: n=%d right picture in %d files; expected %s", "public API, representative", cs.name, cs.num, good, want_line.c_str());
                    EXPECT(good == (int)slots.size() && (int)slots.size() == std::min(cs.num, n3));
                    EXPECT(minivideo_close(&m) == SUCCESS);
                }
                EXPECT(moved >= 3 && resized >= 1 && blank_ruled >= 1);   // (slots did give way; sizes did differ; the blank rule did decide)
                for (const char *v : {"MINIVIDEO_REPRESENTATIVE", "MINIVIDEO_REPRESENTATIVE_ALTERNATES", "MINIVIDEO_STATS", "MINIVIDEO_CROP", "MINIVIDEO_BATCH",
                                      "MINIVIDEO_FAKE_GPUS", "MINIVIDEO_WRITERS", "MINIVIDEO_SKIP_BLANK", "MINIVIDEO_BLANK_VARIANCE", "MINIVIDEO_BLANK_ALTERNATES"})
                    unsetenv(v);
                EXPECT(chdir(cwd) == 0);
                rmdir(dir);
            }
            // malformed values of the two switches of minivideo_decode: FAILURE, with a message, before the device is touched --
            // whether or not the feature is on
            struct Bad { const char *var, *value, *on; };
            for (const Bad &b : {Bad{"MINIVIDEO_REPRESENTATIVE_ALTERNATES", "abc", "1"}, Bad{"MINIVIDEO_REPRESENTATIVE_ALTERNATES", "0", "1"},
                                 Bad{"MINIVIDEO_REPRESENTATIVE_ALTERNATES", "17", "0"}, Bad{"MINIVIDEO_REPRESENTATIVE", "yes", nullptr},
                                 Bad{"MINIVIDEO_REPRESENTATIVE", "2", nullptr}}) {
                if (b.on) setenv("MINIVIDEO_REPRESENTATIVE", b.on, 1);
                setenv(b.var, b.value, 1);
                MediaFile_t *m = nullptr;
                EXPECT(minivideo_open(argv[4], &m) == SUCCESS);
                EXPECT(m && minivideo_parse(m, false, true, false) == SUCCESS);
                const int ctx_before = g_ctx_created, launches_before = g_recon_calls + g_geometry_calls + g_hist_calls;
                fflush(stdout);
                fflush(stderr);
                int pipefd[2];
                EXPECT(pipe(pipefd) == 0);
                const int saved = dup(2);
                dup2(pipefd[1], 2);
                const int rc = m ? minivideo_decode(m, ".", PICTURE_YUV420, 75, n3, PICTURE_UNFILTERED) : SUCCESS;
                fflush(stderr);
                dup2(saved, 2);
                close(saved);
                close(pipefd[1]);
                char msg[512] = "";
                const ssize_t got = read(pipefd[0], msg, sizeof(msg) - 1);
                close(pipefd[0]);
                printf("%-28s %s='%s' rc=%d message: %s", "malformed representative switch", b.var, b.value, rc, got > 0 ? msg : "(none)\n");
                EXPECT(rc == FAILURE && got > 0 && strstr(msg, b.var) != nullptr);
                EXPECT(g_ctx_created == ctx_before && g_recon_calls + g_geometry_calls + g_hist_calls == launches_before);
                EXPECT(minivideo_close(&m) == SUCCESS);
                unsetenv(b.var);
                unsetenv("MINIVIDEO_REPRESENTATIVE");
            }
            printf("HIST MODE DONE\n");
        }
        if (argc > 5 && !strcmp(argv[5], "tensor")) {   // ---- tensor mode: MVHP_OUT_TENSOR against the stub's tensor operation ----
            std::vector<int> order;
            for (int k = 0; k < 3 * n3; k++) order.push_back(k % n3);
            // sink: the right picture, in order, its geometry that of the request, no planes; host delivery: the stub's tensor of
            // the picture's own RGB, of exactly the length g->reserved[0] names; device delivery: nothing comes, and the tensor
            // stands in its slot of the target by the time the sink runs
            struct CheckT {
                const mvhp_stream *s = nullptr;
                mvhp_output_request_t req{};
                mvhp_tensor_request_t treq{};
                std::vector<int> order;
                const uint8_t *target = nullptr;
                size_t slot_bytes = 0;
                int calls = 0, ok = 0, failed = 0, bad = 0, next_seq = 0, past_target = 0, no_canvas = 0;
                uint64_t bytes = 0;
                std::vector<int> delivered;
                static int sink(void *user, int seq, int idr, int rc, const char *err, const mvhp_stream_params_t *, const mvhp_output_geometry_t *g,
                                const uint8_t *yuv, const uint8_t *rgb)
                {
                    CheckT &c = *static_cast<CheckT *>(user);
                    c.calls++;
                    if (seq != c.next_seq || idr != c.order[(size_t)seq] || !g) c.bad++;
                    c.next_seq = seq + 1;
                    if (rc != MVHP_SUCCESS) {
                        c.failed++;
                        if (!err || !*err || yuv || rgb) c.bad++;
                        if (err && strstr(err, "slots")) c.past_target++;
                        if (err && strstr(err, "canvas")) c.no_canvas++;
                        return 0;
                    }
                    mvhp_output_geometry_t want, got = *g;
                    got.reserved[0] = got.reserved[1] = 0;   // (the tensor's length; the score, where the call asks for it)
                    if (mvhp_output_geometry(c.s, idr, &c.req, &want) != MVHP_SUCCESS || memcmp(&want, &got, sizeof(want)) != 0) { c.bad++; return 0; }
                    const mvhp_tensor_params_t t = mvtensor::of_request(c.treq, g->out_w, g->out_h);
                    const size_t tb = mvtensor::bytes(t);
                    if (!tb || g->reserved[0] != tb || yuv || (rgb != nullptr) != (c.target == nullptr)) { c.bad++; return 0; }
                    if (c.target && tb != c.slot_bytes) { c.bad++; return 0; }
                    const uint8_t *ten = c.target ? c.target + (size_t)seq * tb : rgb;
                    const uint64_t h = picture_checksum(*c.s, idr);
                    uint64_t stamp = 0;
                    memcpy(&stamp, ten, 8);
                    if (stamp != h || ten[8] != tensor_tag(t) || ten[9] != 0x3e || ten[tb - 1] != kLastTensor) c.bad++;
                    c.bytes += tb;
                    c.ok++;
                    c.delivered.push_back(seq);
                    return 1;
                }
            };
            auto tensor_request = [](uint32_t cw, uint32_t ch, uint32_t dtype, uint32_t layout, uint32_t flags) {
                mvhp_tensor_request_t t{};
                t.canvas_w = cw; t.canvas_h = ch; t.dtype = dtype; t.layout = layout; t.flags = flags; t.pad_rgb = 0x102030;
                for (int k = 0; k < 3; k++) { t.scale[k] = 1.0f / 255.0f; t.bias[k] = -0.5f * (float)k; }
                return t;
            };
            auto run_tensor = [&](const char *name, mvhp_engine_opts_t o, const mvhp_stream &st, const std::vector<int> &ord, mvhp_output_request_t req,
                                  const mvhp_tensor_request_t &treq, uint32_t extra, CheckT &c, mvhp_decode_stats_t &stats) {
                mvhp_engine_t *e = nullptr;
                if (mvhp_engine_create(&o, &e) != MVHP_SUCCESS) { failures++; return MVHP_FAILURE; }
                c.s = &st; c.req = req; c.treq = treq; c.order = ord;
                c.target = (const uint8_t *)treq.d_target;
                EXPECT(mvhp_engine_set_tensor(e, &treq) == MVHP_SUCCESS);
                req.flags |= extra;
                const int rc = mvhp_engine_decode_ex(e, &st, ord.data(), (int)ord.size(), (int)ord.size(), MVHP_OUT_TENSOR, &req, CheckT::sink, &c, &stats);
                mvhp_engine_destroy(e);
                printf("%-28s rc=%d contexts=%d flags=%#x ok=%u failed=%u batches=%u geometry=%u requeued=%u d2h=%llu\n", name, rc, o.contexts, req.flags,
                       stats.pictures_ok, stats.pictures_failed, stats.batches, stats.geometry_launches, stats.batches_requeued,
                       (unsigned long long)stats.d2h_bytes);
                return rc;
            };
            int formed_crop = 0;
            for (int idr : order) { mvhp_output_geometry_t g; formed_crop += mvhp_output_geometry(&s3, idr, &crop, &g) == MVHP_SUCCESS; }
            // ---- host delivery: one to three contexts, large and small batches, the coded size, cropped, boxed onto a fixed canvas
            int combo = 0;
            for (int contexts = 1; contexts <= 3; contexts++)
                for (int batch : {64, 3})
                    for (mvhp_output_request_t req : {mvhp_output_request_t{0, 0, 0, 0}, crop, box})
                        for (uint32_t extra : {0u, (uint32_t)MVHP_OUTPUT_SCORE}) {
                            mvhp_engine_opts_t o = base; o.contexts = contexts; o.chunk_pictures = 2; o.batch_pictures = batch;
                            o.fail_context = contexts == 3 ? 0 : -1;   // (three contexts: context 0's first batch fails and is re-queued)
                            const bool boxed = (req.flags & MVHP_OUTPUT_BOX) != 0;
                            const mvhp_tensor_request_t treq = tensor_request(boxed ? 48 : 0, boxed ? 48 : 0, (uint32_t)(combo % 3), (uint32_t)(combo / 3 % 2), (uint32_t)(combo / 6 % 2));
                            combo++;
                            const int calls0 = g_tensor_calls, stats0 = g_stats_calls;
                            CheckT c; mvhp_decode_stats_t st;
                            EXPECT(run_tensor(boxed ? "tensor box, host" : req.flags ? "tensor crop, host" : "tensor coded size, host", o, s3, order, req, treq,
                                              extra, c, st) == MVHP_SUCCESS);
                            EXPECT(c.bad == 0 && c.calls == (int)order.size() && c.ok == (int)st.pictures_ok && c.ok == (req.flags ? formed_crop : (int)order.size()));
                            EXPECT(st.d2h_bytes == c.bytes + (extra ? 32ull * (uint64_t)c.ok : 0ull));   // the tensors (and the scores), nothing else
                            EXPECT(g_tensor_calls - calls0 == (int)st.batches && g_stats_calls - stats0 == (extra ? (int)st.batches : 0));
                            EXPECT((int)st.batches_requeued == (contexts == 3 ? 1 : 0));
                            if (!req.flags) EXPECT(st.geometry_launches == 0);
                        }
            {   // a picture larger than the canvas fails in its place with a message; the others are delivered
                mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 2; o.batch_pictures = 4;
                CheckT c; mvhp_decode_stats_t st;
                EXPECT(run_tensor("tensor: canvas too small", o, s3, order, box, tensor_request(32, 48, MVHP_TENSOR_F16, MVHP_TENSOR_NCHW, 0), 0, c, st) == MVHP_FAILURE);
                EXPECT(c.bad == 0 && c.ok == 0 && c.no_canvas == formed_crop && formed_crop > 0);
            }
            // ---- device delivery into a stand-in target in host memory, one context
            auto aligned = [](std::vector<uint8_t> &v) { return v.data() + ((16 - ((uintptr_t)v.data() & 15)) & 15); };
            for (int batch : {64, 3}) {
                mvhp_engine_opts_t o = base; o.contexts = 1; o.chunk_pictures = 2; o.batch_pictures = batch;
                mvhp_tensor_request_t treq = tensor_request(48, 48, MVHP_TENSOR_BF16, MVHP_TENSOR_NHWC, MVHP_TENSOR_BGR);
                const size_t tb = 3 * 48 * 48 * 2;
                const int slots = (int)order.size() - 2;   // the last two pictures have no slot
                std::vector<uint8_t> mem((size_t)order.size() * tb + 16, 0xee);
                treq.d_target = aligned(mem);
                treq.target_pictures = (uint32_t)slots;
                CheckT c; c.slot_bytes = tb; mvhp_decode_stats_t st;
                const int calls0 = g_tensor_calls;
                EXPECT(run_tensor("tensor box, device", o, s3, order, box, treq, 0, c, st) == MVHP_SUCCESS);
                EXPECT(c.bad == 0 && c.calls == (int)order.size() && c.ok == (int)st.pictures_ok && c.ok > 0 && st.d2h_bytes == 0);
                EXPECT(c.past_target >= 1 && c.past_target <= 2 && g_tensor_calls - calls0 == (int)st.batches);
                std::vector<bool> got(order.size(), false);
                for (int seq : c.delivered) got[(size_t)seq] = true;
                for (size_t k = 0; k < order.size(); k++) {   // a failed picture's slot (and the room past the last slot) is untouched
                    if (got[k]) { EXPECT((int)k < slots); continue; }
                    const uint8_t *t = aligned(mem) + k * tb;
                    bool same = true;
                    for (size_t i = 0; i < tb; i++) same = same && t[i] == 0xee;
                    EXPECT(same);
                }
            }
            {   // a picture that fails to parse, in the middle of a batch: its slot stays as it was (canvas 0: slots of the pictures' size)
                std::vector<uint8_t> b2 = read_file(argv[2]);
                const int broken = atoi(argv[3]);
                mvhp_stream s2;
                s2.data = b2.data();
                s2.size = b2.size();
                EXPECT(s2.build(err) == h264::RC_SUCCESS);
                std::vector<int> o2(s2.idrs.size());
                for (size_t i = 0; i < o2.size(); i++) o2[i] = (int)i;
                mvhp_stream_params_t p2;
                EXPECT(mvhp_stream_params(&s2, 0, &p2) == MVHP_SUCCESS);
                mvhp_engine_opts_t o = base; o.contexts = 1; o.chunk_pictures = 3; o.batch_pictures = 6;
                mvhp_tensor_request_t treq = tensor_request(0, 0, MVHP_TENSOR_F32, MVHP_TENSOR_NCHW, 0);
                const size_t tb = (size_t)p2.width_mbs * p2.height_mbs * 768 * 4;
                std::vector<uint8_t> mem(o2.size() * tb + 16, 0xee);
                treq.d_target = aligned(mem);
                treq.target_pictures = (uint32_t)o2.size();
                CheckT c; c.slot_bytes = tb; mvhp_decode_stats_t st;
                EXPECT(run_tensor("tensor, device, broken", o, s2, o2, mvhp_output_request_t{0, 0, 0, 0}, treq, 0, c, st) == MVHP_SUCCESS);
                EXPECT(c.bad == 0 && c.failed == 1 && c.ok == (int)o2.size() - 1 && st.d2h_bytes == 0);
                const uint8_t *t = aligned(mem) + (size_t)broken * tb;
                bool same = true;
                for (size_t i = 0; i < tb; i++) same = same && t[i] == 0xee;
                EXPECT(same);
            }
            {   // ---- refusals, each with a message and before any launch
                struct Refused { const char *name; int contexts; bool set, device; int mask; uint32_t flags; bool plain_sink; const char *word; };
                std::vector<uint8_t> mem(64, 0xee);
                for (const Refused &r : {Refused{"tensor: no request", 1, false, false, MVHP_OUT_TENSOR, 0, false, "mvhp_engine_set_tensor"},
                                         Refused{"tensor with JPEG", 1, true, false, MVHP_OUT_TENSOR | MVHP_OUT_JPEG, 0, false, "MVHP_OUT_JPEG"},
                                         Refused{"tensor with PNG", 1, true, false, MVHP_OUT_TENSOR | MVHP_OUT_PNG, 0, false, "MVHP_OUT_PNG"},
                                         Refused{"tensor with bars", 1, true, false, MVHP_OUT_TENSOR, MVHP_OUTPUT_BARS, false, "MVHP_OUTPUT_BARS"},
                                         Refused{"tensor, plain sink", 1, true, false, MVHP_OUT_TENSOR, 0, true, "mvhp_engine_decode_ex"},
                                         Refused{"tensor, device, 2 contexts", 2, true, true, MVHP_OUT_TENSOR, 0, false, "one context"}}) {
                    mvhp_engine_opts_t o = base; o.contexts = r.contexts;
                    std::string why;
                    mvengine::Engine *pe = mvengine::engine_create(g_stub, &o, why);
                    EXPECT(pe != nullptr);
                    mvhp_tensor_request_t treq = tensor_request(48, 48, MVHP_TENSOR_F16, MVHP_TENSOR_NCHW, 0);
                    if (r.device) { treq.d_target = aligned(mem); treq.target_pictures = 1; }
                    if (r.set) EXPECT(pe && mvengine::engine_set_tensor(pe, &treq, why) == MVHP_SUCCESS);
                    const int launches0 = g_recon_calls + g_geometry_calls + g_jpeg_calls + g_png_calls + g_tensor_calls;
                    mvhp_output_request_t req{r.flags, 0, 0, 0};
                    CheckT c; c.s = &s3; c.order = order; mvhp_decode_stats_t st;
                    Check cp; cp.s = &s3; cp.order = order;
                    const int rc = !pe ? MVHP_SUCCESS
                                   : r.plain_sink ? mvengine::engine_decode(pe, s3, order.data(), (int)order.size(), (int)order.size(), r.mask, nullptr, Check::sink, nullptr, &cp, &st, why)
                                                  : mvengine::engine_decode(pe, s3, order.data(), (int)order.size(), (int)order.size(), r.mask, &req, nullptr, CheckT::sink, &c, &st, why);
                    printf("%-28s rc=%d message: %s\n", r.name, rc, why.c_str());
                    EXPECT(rc == MVHP_FAILURE && c.calls == 0 && cp.calls == 0 && why.find(r.word) != std::string::npos);
                    EXPECT(g_recon_calls + g_geometry_calls + g_jpeg_calls + g_png_calls + g_tensor_calls == launches0);
                    if (pe && r.set) {   // taking the request back: the call is refused again
                        EXPECT(mvengine::engine_set_tensor(pe, nullptr, why) == MVHP_SUCCESS);
                        const mvhp_output_request_t none{0, 0, 0, 0};
                        EXPECT(mvengine::engine_decode(pe, s3, order.data(), (int)order.size(), (int)order.size(), MVHP_OUT_TENSOR, &none, nullptr, CheckT::sink, &c, &st, why) == MVHP_FAILURE);
                        EXPECT(why.find("mvhp_engine_set_tensor") != std::string::npos && c.calls == 0);
                    }
                    mvengine::engine_destroy(pe);
                }
                // malformed requests
                mvhp_engine_opts_t o = base; o.contexts = 1;
                std::string why;
                mvengine::Engine *pe = mvengine::engine_create(g_stub, &o, why);
                EXPECT(pe != nullptr);
                int n_bad = 0;
                for (int k = 0; pe && k < 9; k++) {
                    mvhp_tensor_request_t t = tensor_request(48, 48, MVHP_TENSOR_F16, MVHP_TENSOR_NCHW, 0);
                    if (k == 0) t.dtype = 3;
                    if (k == 1) t.layout = 2;
                    if (k == 2) t.flags = 2;
                    if (k == 3) t.canvas_w = 0;
                    if (k == 4) t.canvas_h = 16385;
                    if (k == 5) t.scale[1] = INFINITY;
                    if (k == 6) t.reserved = 1;
                    if (k == 7) { t.d_target = aligned(mem) + 8; t.target_pictures = 1; }
                    if (k == 8) { t.d_target = aligned(mem); t.target_pictures = 0; }
                    const int rc = mvengine::engine_set_tensor(pe, &t, why);
                    printf("%-28s %d rc=%d message: %s\n", "malformed tensor request", k, rc, why.c_str());
                    EXPECT(rc == MVHP_FAILURE && why.find("mvhp_engine_set_tensor") != std::string::npos);
                    n_bad += rc == MVHP_FAILURE;
                }
                EXPECT(n_bad == 9);
                mvengine::engine_destroy(pe);
                EXPECT(mvhp_engine_set_tensor(nullptr, nullptr) == MVHP_FAILURE && mvhp_engine_contexts(nullptr) == 0);
            }
            {   // a device table without the operation: the call fails with the message before any launch; other calls are not affected
                g_stub.caps &= ~mvengine::CAP_TENSOR;
                mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 2; o.batch_pictures = 4;
                std::string why;
                mvengine::Engine *pe = mvengine::engine_create(g_stub, &o, why);
                EXPECT(pe != nullptr);
                const mvhp_tensor_request_t treq = tensor_request(0, 0, MVHP_TENSOR_F16, MVHP_TENSOR_NCHW, 0);
                EXPECT(pe && mvengine::engine_set_tensor(pe, &treq, why) == MVHP_SUCCESS);
                const int launches0 = g_recon_calls + g_geometry_calls + g_tensor_calls;
                CheckT c; c.s = &s3; c.order = order; mvhp_decode_stats_t st;
                mvhp_output_request_t req = crop;
                const int rc = pe ? mvengine::engine_decode(pe, s3, order.data(), (int)order.size(), (int)order.size(), MVHP_OUT_TENSOR, &req, nullptr, CheckT::sink, &c, &st, why) : MVHP_SUCCESS;
                printf("%-28s rc=%d message: %s\n", "tensor: table without it", rc, why.c_str());
                EXPECT(rc == MVHP_FAILURE && c.calls == 0 && why.find("tensor operation") != std::string::npos);
                EXPECT(g_recon_calls + g_geometry_calls + g_tensor_calls == launches0);
                mvengine::engine_destroy(pe);
                CheckG cg;
                EXPECT(run_ex("tensor: table without it, off", o, s3, order, MVHP_OUT_RGB_ONLY, crop, cg, st) == MVHP_SUCCESS && cg.bad == 0);
                g_stub.caps |= mvengine::CAP_TENSOR;
            }
            {   // without MVHP_OUT_TENSOR a set request changes nothing: the same pictures, the operation never called
                mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 2; o.batch_pictures = 4;
                mvhp_engine_t *e = nullptr;
                EXPECT(mvhp_engine_create(&o, &e) == MVHP_SUCCESS);
                const mvhp_tensor_request_t treq = tensor_request(48, 48, MVHP_TENSOR_F16, MVHP_TENSOR_NCHW, 0);
                EXPECT(mvhp_engine_set_tensor(e, &treq) == MVHP_SUCCESS && mvhp_engine_contexts(e) == 2);
                const int calls0 = g_tensor_calls;
                CheckG cg; cg.s = &s3; cg.req = box; cg.order = order; cg.want_rgb = true; cg.want_yuv = false;
                mvhp_decode_stats_t st;
                EXPECT(mvhp_engine_decode_ex(e, &s3, order.data(), (int)order.size(), (int)order.size(), MVHP_OUT_RGB_ONLY, &box, CheckG::sink, &cg, &st) == MVHP_SUCCESS);
                EXPECT(cg.bad == 0 && g_tensor_calls == calls0 && st.d2h_bytes == d2h_expected(s3, order, box, MVHP_OUT_RGB_ONLY));
                printf("%-28s ok=%u d2h=%llu\n", "tensor: request set, flag off", st.pictures_ok, (unsigned long long)st.d2h_bytes);
                mvhp_engine_destroy(e);
            }
            printf("TENSOR MODE DONE\n");
        }
        if (argc > 5 && !strcmp(argv[5], "bars")) {   // ---- bars mode: MVHP_OUTPUT_BARS / MVHP_OUTPUT_TRIM against the stub's black-bar operation ----
            std::vector<int> order;
            for (int k = 0; k < 3 * n3; k++) order.push_back(k % n3);
            auto run_bars = [&](const char *name, mvhp_engine_opts_t o, int mask, mvhp_output_request_t req, CheckB &c, mvhp_decode_stats_t &stats) {
                mvhp_engine_t *e = nullptr;
                if (mvhp_engine_create(&o, &e) != MVHP_SUCCESS) { failures++; return MVHP_FAILURE; }
                c.s = &s3; c.req = req; c.req.reserved = 0; c.order = order; c.mask = mask;
                req.flags |= MVHP_OUTPUT_BARS;
                const int rc = mvhp_engine_decode_ex(e, &s3, order.data(), (int)order.size(), (int)order.size(), mask, &req, CheckB::sink, &c, &stats);
                mvhp_engine_destroy(e);
                printf("%-28s rc=%d mask=%d flags=%u ok=%u failed=%u batches=%u geometry=%u requeued=%u d2h=%llu\n", name, rc, mask, req.flags,
                       stats.pictures_ok, stats.pictures_failed, stats.batches, stats.geometry_launches, stats.batches_requeued,
                       (unsigned long long)stats.d2h_bytes);
                return rc;
            };
            int distinct_checked = 0, empty_seen = 0;
            for (int contexts = 1; contexts <= 3; contexts++)
                for (int mask : {0, MVHP_OUT_RGB, MVHP_OUT_RGB_ONLY})
                    for (mvhp_output_request_t req : {mvhp_output_request_t{0, 0, 0, 0}, crop, box}) {
                        mvhp_engine_opts_t o = base; o.contexts = contexts; o.chunk_pictures = 2; o.batch_pictures = contexts == 1 ? 64 : 3;
                        // without the flag: the two words are 0 (CheckG compares all of the geometry) and the operation is never called
                        mvhp_decode_stats_t st0;
                        const int calls0 = g_bars_calls;
                        CheckG cg;
                        EXPECT(run_ex("bars: flag off", o, s3, order, mask, req, cg, st0) == MVHP_SUCCESS);
                        EXPECT(cg.bad == 0 && g_bars_calls == calls0);
                        // with it (three contexts: the first batch of context 0 fails and is re-queued, and probed again)
                        o.fail_context = contexts == 3 ? 0 : -1;
                        const int level = contexts == 2 ? 37 : 0;   // (0 means 24)
                        req.reserved = MVHP_BARS_REQUEST(level);
                        const int launches0 = g_recon_calls + g_geometry_calls;
                        CheckB c; mvhp_decode_stats_t st;
                        EXPECT(run_bars(req.flags & MVHP_OUTPUT_BOX ? "bars box" : req.flags ? "bars crop" : "bars coded size", o, mask, req, c, st) == MVHP_SUCCESS);
                        EXPECT(c.bad == 0 && c.no_op == 0 && c.calls == (int)order.size() && c.ok == (int)st.pictures_ok && c.ok + c.failed == c.calls);
                        EXPECT(c.ok == (int)st0.pictures_ok);
                        EXPECT(st.d2h_bytes == st0.d2h_bytes + 32ull * (uint64_t)c.formed_n);   // exactly one record per picture of a batch
                        EXPECT((int)st.batches_requeued == (contexts == 3 ? 1 : 0));
                        EXPECT(g_bars_calls - calls0 == (int)st.batches);                          // every launch of such a call carries `bars`
                        EXPECT(g_recon_calls + g_geometry_calls - launches0 == (int)st.batches);
                        EXPECT(g_bars_level == (level ? level : MVHP_BARS_LEVEL_DEFAULT));
                        if (!req.flags) EXPECT(st.geometry_launches == 0);   // the flag alone: still the coded-size path
                        std::vector<uint64_t> d = c.boxes;
                        std::sort(d.begin(), d.end());
                        if (std::unique(d.begin(), d.end()) - d.begin() >= 3) distinct_checked++;
                        empty_seen += c.empty;
                    }
            EXPECT(distinct_checked == 27);   // the sink got each picture's own box
            printf("%-28s %d empty boxes delivered\n", "bars", empty_seen);
            {   // a device table without the operation: every picture of the call fails with the message
                g_stub.caps &= ~mvengine::CAP_BARS;
                mvhp_engine_opts_t o = base; o.contexts = 2; o.chunk_pictures = 2; o.batch_pictures = 4;
                CheckB c; mvhp_decode_stats_t st;
                const int calls0 = g_bars_calls, recon0 = g_recon_calls + g_geometry_calls;
                EXPECT(run_bars("bars: table without it", o, 0, crop, c, st) == MVHP_FAILURE);
                EXPECT(c.bad == 0 && c.ok == 0 && c.no_op == c.formed_n && c.no_op > 0 && g_bars_calls == calls0);
                EXPECT(g_recon_calls + g_geometry_calls == recon0);
                CheckG cg;   // ... and a call without the flag is not affected
                EXPECT(run_ex("bars: table without it, off", o, s3, order, 0, crop, cg, st) == MVHP_SUCCESS && cg.bad == 0);
                g_stub.caps |= mvengine::CAP_BARS;
            }
            {   // the four refusals, each with a message and before any work
                mvhp_engine_opts_t o = base; o.contexts = 1;
                std::string why;
                mvengine::Engine *pe = mvengine::engine_create(g_stub, &o, why);
                EXPECT(pe != nullptr);
                const int launches0 = g_recon_calls + g_geometry_calls + g_jpeg_calls + g_png_calls + g_bars_calls;
                struct Refused { const char *name; int mask; uint32_t flags; const char *word; };
                for (const Refused &r : {Refused{"bars with JPEG", MVHP_OUT_JPEG, MVHP_OUTPUT_BARS, "MVHP_OUT_JPEG"},
                                         Refused{"bars with PNG", MVHP_OUT_PNG, MVHP_OUTPUT_BARS | MVHP_OUTPUT_CROP, "MVHP_OUT_PNG"},
                                         Refused{"bars with the score", 0, MVHP_OUTPUT_BARS | MVHP_OUTPUT_SCORE, "MVHP_OUTPUT_SCORE"}}) {
                    mvhp_output_request_t req{r.flags, 0, 0, 0};
                    CheckB c; c.s = &s3; c.order = order; mvhp_decode_stats_t st;
                    why.clear();
                    const int rc = pe ? mvengine::engine_decode(pe, s3, order.data(), (int)order.size(), (int)order.size(), r.mask, &req, nullptr,
                                                                CheckB::sink, &c, &st, why) : MVHP_SUCCESS;
                    printf("%-28s rc=%d message: %s\n", r.name, rc, why.c_str());
                    EXPECT(rc == MVHP_FAILURE && c.calls == 0 && why.find(r.word) != std::string::npos && why.find("MVHP_OUTPUT_BARS") != std::string::npos);
                }
                {   // a level of 255
                    mvhp_output_request_t req{MVHP_OUTPUT_BARS, 0, 0, MVHP_BARS_REQUEST(255)};
                    CheckB c; c.s = &s3; c.order = order; mvhp_decode_stats_t st;
                    why.clear();
                    EXPECT(pe && mvengine::engine_decode(pe, s3, order.data(), (int)order.size(), (int)order.size(), 0, &req, nullptr, CheckB::sink, &c, &st,
                                                         why) == MVHP_FAILURE && c.calls == 0 && why.find("255") != std::string::npos);
                }
                {   // the plain sink has no geometry to carry the box
                    mvhp_output_request_t req{MVHP_OUTPUT_BARS, 0, 0, 0};
                    mvhp_decode_stats_t st;
                    why.clear();
                    const int rc = pe ? mvengine::engine_decode(pe, s3, order.data(), (int)order.size(), (int)order.size(), 0, &req, plain_sink_accepts,
                                                                nullptr, nullptr, &st, why) : MVHP_SUCCESS;
                    printf("%-28s rc=%d message: %s\n", "bars with the plain sink", rc, why.c_str());
                    EXPECT(rc == MVHP_FAILURE && why.find("MVHP_OUTPUT_BARS") != std::string::npos && why.find("mvhp_engine_decode_ex") != std::string::npos);
                }
                if (pe) mvengine::engine_destroy(pe);
                EXPECT(g_recon_calls + g_geometry_calls + g_jpeg_calls + g_png_calls + g_bars_calls == launches0);
            }
            {   // MVHP_OUTPUT_TRIM with a box set on the stream: the geometry is launched with the trimmed rectangle; without the
                // flag, or without a box, with the SPS crop
                mvhp_luma_bars_t u{};
                u.x = 3; u.y = 9; u.w = 70; u.h = 55;
                mvhp_output_geometry_t sps{}, cut{};
                EXPECT(mvhp_stream_crop(&s3, 0, &sps) == MVHP_SUCCESS && mvhp_trim_rect(&sps, &u, &cut) == 1);
                EXPECT(memcmp(&sps, &cut, sizeof(sps)) != 0);
                g_watch_crop[0] = cut.crop_x; g_watch_crop[1] = cut.crop_y; g_watch_crop[2] = cut.crop_w; g_watch_crop[3] = cut.crop_h;
                const mvhp_output_request_t trim{MVHP_OUTPUT_TRIM, 0, 0, 0}, trim_box{MVHP_OUTPUT_TRIM | MVHP_OUTPUT_BOX, 40, 40, 0};
                for (int contexts = 1; contexts <= 3; contexts++) {
                    mvhp_engine_opts_t o = base; o.contexts = contexts; o.chunk_pictures = 2; o.batch_pictures = contexts == 1 ? 64 : 3;
                    o.fail_context = contexts == 3 ? 0 : -1;
                    mvhp_decode_stats_t st, st_crop;
                    g_watch_hits = 0;
                    CheckG c0;   // no box set: the flag is MVHP_OUTPUT_CROP (CheckG forms the geometry it expects from the same stream)
                    EXPECT(run_ex("trim: no box", o, s3, order, 0, trim, c0, st) == MVHP_SUCCESS && c0.bad == 0 && g_watch_hits == 0);
                    CheckG cc;
                    EXPECT(run_ex("trim: crop for comparison", o, s3, order, 0, crop, cc, st_crop) == MVHP_SUCCESS && cc.bad == 0);
                    EXPECT(st.d2h_bytes == st_crop.d2h_bytes && st.geometry_launches == st_crop.geometry_launches);
                    EXPECT(mvhp_stream_set_trim(&s3, &u) == MVHP_SUCCESS);
                    CheckG c1;   // a box set, no flag: nothing changes
                    EXPECT(run_ex("trim: box, flag off", o, s3, order, 0, crop, c1, st) == MVHP_SUCCESS && c1.bad == 0 && g_watch_hits == 0);
                    EXPECT(st.d2h_bytes == st_crop.d2h_bytes);
                    for (const mvhp_output_request_t &req : {trim, trim_box}) {
                        for (int mask : {0, MVHP_OUT_RGB}) {
                            g_watch_hits = 0;
                            CheckG c2;
                            EXPECT(run_ex(req.flags & MVHP_OUTPUT_BOX ? "trim box" : "trim", o, s3, order, mask, req, c2, st) == MVHP_SUCCESS);
                            EXPECT(c2.bad == 0 && c2.ok == cc.ok && c2.with_geometry == c2.ok && g_watch_hits >= 1);
                            EXPECT(st.d2h_bytes == d2h_expected(s3, order, req, mask));
                        }
                    }
                    {   // and probing a trimmed call: the boxes are those of the trimmed rectangle
                        mvhp_output_request_t req = trim;
                        CheckB cb;
                        EXPECT(run_bars("trim and bars", o, 0, req, cb, st) == MVHP_SUCCESS && cb.bad == 0 && cb.ok == cc.ok);
                    }
                    EXPECT(mvhp_stream_set_trim(&s3, nullptr) == MVHP_SUCCESS);
                }
                for (auto &w : g_watch_crop) w = 0;
            }
            {   // minivideo_decode under MINIVIDEO_TRIM=1 on the stub device: the probe call, then the decode call, on one engine; and
                // the malformed switches: FAILURE, with a message, before the device is touched
                char tmpl[] = "/tmp/mvharness_XXXXXX";
                const char *dir = mkdtemp(tmpl);
                char cwd[4096];
                EXPECT(dir != nullptr && getcwd(cwd, sizeof(cwd)) != nullptr);
                std::string in = argv[4];
                if (in[0] != '/') in = std::string(cwd) + "/" + in;
                EXPECT(dir && chdir(dir) == 0);
                setenv("MINIVIDEO_TRIM", "1", 1);
                setenv("MINIVIDEO_TRIM_LEVEL", "40", 1);
                for (const char *probes : {"1", "3", "64"}) {
                    setenv("MINIVIDEO_TRIM_PROBES", probes, 1);
                    MediaFile_t *m = nullptr;
                    EXPECT(minivideo_open(in.c_str(), &m) == SUCCESS);
                    EXPECT(m && minivideo_parse(m, false, true, false) == SUCCESS);
                    const int calls0 = g_bars_calls;
                    const int num = 5;
                    EXPECT(m && minivideo_decode(m, ".", PICTURE_YUV420, 75, num, PICTURE_UNFILTERED) == SUCCESS);
                    EXPECT(g_bars_calls > calls0 && g_bars_level == 40);
                    int good = 0;
                    for (int k = 0; k < num; k++) {
                        const std::string name = std::string(m->file_name) + "_" + std::to_string(k) + ".yuv";
                        const std::vector<uint8_t> f = read_file(name);
                        remove(name.c_str());
                        uint64_t got = 0;
                        if (f.size() >= 8) memcpy(&got, f.data(), 8);
                        if (got == picture_checksum(s3, k)) good++;
                    }
                    printf("%-28s probes=%s right picture in %d files\n", "public API, black bars", probes, good);
                    EXPECT(good == num);
                    EXPECT(minivideo_close(&m) == SUCCESS);
                }
                unsetenv("MINIVIDEO_TRIM_LEVEL"); unsetenv("MINIVIDEO_TRIM_PROBES");
                struct Bad { const char *var, *value; };
                for (const Bad &b : {Bad{"MINIVIDEO_TRIM_LEVEL", "300"}, Bad{"MINIVIDEO_TRIM_LEVEL", "0"}, Bad{"MINIVIDEO_TRIM_LEVEL", "255"},
                                     Bad{"MINIVIDEO_TRIM_PROBES", "0"}, Bad{"MINIVIDEO_TRIM_PROBES", "65"}, Bad{"MINIVIDEO_TRIM", "x"}}) {
                    setenv("MINIVIDEO_TRIM", "1", 1);
                    setenv(b.var, b.value, 1);
                    MediaFile_t *m = nullptr;
                    EXPECT(minivideo_open(in.c_str(), &m) == SUCCESS);
                    EXPECT(m && minivideo_parse(m, false, true, false) == SUCCESS);
                    const int ctx_before = g_ctx_created, launches_before = g_recon_calls + g_geometry_calls + g_bars_calls;
                    fflush(stdout);
                    fflush(stderr);
                    int pipefd[2];
                    EXPECT(pipe(pipefd) == 0);
                    const int saved = dup(2);
                    dup2(pipefd[1], 2);
                    const int rc = m ? minivideo_decode(m, ".", PICTURE_YUV420, 75, n3, PICTURE_UNFILTERED) : SUCCESS;
                    fflush(stderr);
                    dup2(saved, 2);
                    close(saved);
                    close(pipefd[1]);
                    char msg[512] = "";
                    const ssize_t got = read(pipefd[0], msg, sizeof(msg) - 1);
                    close(pipefd[0]);
                    printf("%-28s %s='%s' rc=%d message: %s", "malformed trim switch", b.var, b.value, rc, got > 0 ? msg : "(none)\n");
                    EXPECT(rc == FAILURE && got > 0 && strstr(msg, b.var) != nullptr);
                    EXPECT(g_ctx_created == ctx_before && g_recon_calls + g_geometry_calls + g_bars_calls == launches_before);
                    EXPECT(minivideo_close(&m) == SUCCESS);
                    unsetenv(b.var);
                }
                unsetenv("MINIVIDEO_TRIM");
                EXPECT(chdir(cwd) == 0);
                rmdir(dir);
            }
            printf("BARS MODE DONE\n");
        }
    }
    EXPECT(g_live_ctx == 0 && g_dev_allocs == 0);
    printf(failures ? "HARNESS FAILED (%d)\n" : "HARNESS OK\n", failures);
    return failures ? 1 : 0;
}
