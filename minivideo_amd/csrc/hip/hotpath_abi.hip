// hotpath_abi.hip -- C-ABI (include/minivideo_hotpath.h) over the HIP kernels.
// There is deliberately NO CPU fallback here: without a usable HIP device every
// reconstruction entry point fails with MVHP_FAILURE and a message.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "decode_engine.h"
#include "blank_policy.h"
#include "launch_plan.h"
#include "minivideo_hotpath.h"
#include "png_format.h"
#include "recon_kernels.h"
#include "represent_policy.h"
#include "tensor_policy.h"

namespace {

thread_local char g_err[512] = "";

void set_err(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    fprintf(stderr, "[minivideo-hip] %s\n", g_err);
}

#define HIP_TRY(expr)                                                                  \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess) {                                                        \
            set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return MVHP_FAILURE;                                                       \
        }                                                                              \
    } while (0)

bool params_ok(const mvhp_stream_params_t *p)
{
    if (!p) return false;
    if (p->width_mbs == 0 || p->height_mbs == 0) return false;
    if (p->width_mbs > 1024 || p->height_mbs > 1024) return false; // LDS line buffer: 32 B per MB column
    if (p->chroma_qp_index_offset < -12 || p->chroma_qp_index_offset > 12) return false;
    if (p->second_chroma_qp_index_offset < -12 || p->second_chroma_qp_index_offset > 12) return false;
    return true;
}

} // namespace

struct mvhp_ctx {
    int          device;
    hipStream_t  stream;
    uint32_t    *d_err;
    int          waves;       // 0 = auto
    int          layout;      // MVHP_LAYOUT_*
    int          fused_color; // 1 = RGB written by the reconstruction kernel's epilogue (default)
    int          crop_copy;   // 1 = crop-only geometries run the copy kernel (crop_copy.hip), 0 = the general resample kernel
    int          stats_band;  // luma rows per workgroup of the picture-score kernel, 0 = choose (mvhp_set_stats_band)
    int          bars_band;   // luma rows per workgroup of the black-bar counting pass, 0 = choose (mvhp_set_bars_band)
    int          hist_band;   // luma rows per workgroup of the plane-histogram kernel, 0 = choose (mvhp_set_hist_band)
    int          tensor_rows; // canvas rows per workgroup of the tensor kernel, 0 = choose (mvhp_set_tensor_rows)
    int          n_cus;
    size_t       max_lds;
    int          last_layout, last_waves;   // what the last reconstruction launch used
    // wide launches (MVHP_LAYOUT_WIDE / QUAD_WIDE): ticket counter, seam granules, the tag of the last launch.  One set per
    // context: two wide launches of one context never overlap (a launch on another stream waits for the previous one).
    uint32_t    *d_ticket;
    uint32_t     ticket_base;               // value of *d_ticket once every launch issued so far has run
    uint32_t     wide_epoch;
    void        *d_seam;
    size_t       d_seam_bytes;
    hipEvent_t   wide_done;                 // recorded behind the last wide launch
    hipStream_t  wide_stream;               // the stream it ran on
    int          ticket_skew_once;          // test hook (mvhp_debug_skew_next_ticket_base): added to the next wide launch's base
    // staging for the host convenience path
    void        *d_packed;
    size_t       d_packed_bytes;
    uint8_t     *d_yuv;
    size_t       d_yuv_bytes;
    uint8_t     *d_rgb;
    size_t       d_rgb_bytes;
    // JPEG encoder (jpeg_encode.hip): levels, non-zero maps and interval lengths of one batch.  One per context: an encode on
    // another stream waits for the previous one.
    void        *d_jpeg;
    size_t       d_jpeg_bytes;
    hipEvent_t   jpeg_done;
    hipStream_t  jpeg_stream;
    // PNG encoder (png_encode.hip): filter types, code lengths and chunk lengths of one batch, kept like the JPEG encoder's
    void        *d_png;
    size_t       d_png_bytes;
    hipEvent_t   png_done;
    hipStream_t  png_stream;
    // black bars (luma_bars.hip): row and column counters of one batch, kept like the encoders' scratch
    void        *d_bars;
    size_t       d_bars_bytes;
    hipEvent_t   bars_done;
    hipStream_t  bars_stream;
};

static hipStream_t stream_of(const mvhp_ctx *c, void *stream) { return stream ? (hipStream_t)stream : c->stream; }

static mvhp::PlanDevice plan_device(const mvhp_ctx *c) { return {c->n_cus, c->max_lds, c->layout, c->waves}; }

extern "C" {

MVHP_EXPORT const char *mvhp_last_error(void) { return g_err; }

MVHP_EXPORT size_t mvhp_packed_frame_bytes(const mvhp_stream_params_t *p)
{
    return p ? (size_t)p->width_mbs * p->height_mbs * MVHP_MB_BYTES : 0;
}
MVHP_EXPORT size_t mvhp_yuv_frame_bytes(const mvhp_stream_params_t *p)
{
    return p ? (size_t)p->width_mbs * p->height_mbs * 384 : 0;
}
MVHP_EXPORT size_t mvhp_rgb_frame_bytes(const mvhp_stream_params_t *p)
{
    return p ? (size_t)p->width_mbs * p->height_mbs * 768 : 0;
}

MVHP_EXPORT int mvhp_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

MVHP_EXPORT int mvhp_create(int device, mvhp_ctx_t **out)
{
    if (!out) return MVHP_FAILURE;
    *out = nullptr;
    int n = mvhp_device_count();
    if (n <= 0) {
        set_err("no HIP device available: the reconstruction path has no CPU fallback");
        return MVHP_FAILURE;
    }
    if (device < 0 || device >= n) {
        set_err("device %d out of range (0..%d)", device, n - 1);
        return MVHP_FAILURE;
    }
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    mvhp_ctx *c = new mvhp_ctx();
    memset(c, 0, sizeof(*c));
    c->device = device;
    c->fused_color = 1;
    c->crop_copy = 1;
    if (const char *e = getenv("MINIVIDEO_LAYOUT")) { // tuning / test override, speed only
        for (int l = MVHP_LAYOUT_ROWS; l < MVHP_LAYOUT_COUNT; l++)   // (an unknown name is ignored)
            if (!strcmp(e, mvhp::kernel_form(l).name)) c->layout = l;
    }
    c->n_cus = prop.multiProcessorCount;
    c->max_lds = prop.maxSharedMemoryPerMultiProcessor ? prop.maxSharedMemoryPerMultiProcessor : 65536;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&c->d_err, 2 * sizeof(uint32_t)) != hipSuccess ||
        hipMemset(c->d_err, 0, 2 * sizeof(uint32_t)) != hipSuccess ||
        hipEventCreateWithFlags(&c->wide_done, hipEventDisableTiming) != hipSuccess) {
        set_err("context allocation failed on device %d", device);
        delete c;
        return MVHP_FAILURE;
    }
    c->d_ticket = c->d_err + 1;   // (the error word and the ticket counter share one small allocation)
    *out = c;
    return MVHP_SUCCESS;
}

MVHP_EXPORT void mvhp_destroy(mvhp_ctx_t *c)
{
    if (!c) return;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    if (c->d_packed) hipFree(c->d_packed);
    if (c->d_yuv) hipFree(c->d_yuv);
    if (c->d_rgb) hipFree(c->d_rgb);
    if (c->d_err) hipFree(c->d_err);
    if (c->d_seam) hipFree(c->d_seam);
    if (c->d_jpeg) hipFree(c->d_jpeg);
    if (c->jpeg_done) hipEventDestroy(c->jpeg_done);
    if (c->d_png) hipFree(c->d_png);
    if (c->png_done) hipEventDestroy(c->png_done);
    if (c->d_bars) hipFree(c->d_bars);
    if (c->bars_done) hipEventDestroy(c->bars_done);
    if (c->wide_done) hipEventDestroy(c->wide_done);
    hipStreamDestroy(c->stream);
    delete c;
}

MVHP_EXPORT int mvhp_set_waves_per_picture(mvhp_ctx_t *c, int waves)
{
    if (!c || !(waves == 0 || waves == 1 || waves == 2 || waves == 4 || waves == 6 || waves == 8 || waves == 12 || waves == 16)) return MVHP_FAILURE;
    c->waves = waves;
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_set_layout(mvhp_ctx_t *c, int layout)
{
    if (!c || layout < MVHP_LAYOUT_AUTO || layout >= MVHP_LAYOUT_COUNT) return MVHP_FAILURE;
    c->layout = layout;
    return MVHP_SUCCESS;
}

MVHP_EXPORT void *mvhp_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) {   // portable: every device may DMA from / to it
        set_err("hipHostMalloc(%zu) failed", bytes);
        return nullptr;
    }
    return p;
}

MVHP_EXPORT void mvhp_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}

MVHP_EXPORT int mvhp_set_fused_color(mvhp_ctx_t *c, int on)
{
    if (!c) return MVHP_FAILURE;
    c->fused_color = on ? 1 : 0;
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_set_crop_copy(mvhp_ctx_t *c, int on)
{
    if (!c) return MVHP_FAILURE;
    c->crop_copy = on ? 1 : 0;
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_set_stats_band(mvhp_ctx_t *c, int rows)
{
    if (!c || rows < 0 || rows > 65536) return MVHP_FAILURE;
    c->stats_band = rows;
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_set_bars_band(mvhp_ctx_t *c, int rows)
{
    if (!c || rows < 0 || rows > 65536) return MVHP_FAILURE;
    c->bars_band = rows;
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_set_tensor_rows(mvhp_ctx_t *c, int rows)
{
    if (!c || rows < 0 || rows > 16384) return MVHP_FAILURE;
    c->tensor_rows = rows;
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_set_hist_band(mvhp_ctx_t *c, int rows)
{
    if (!c || rows < 0 || rows > 65536) return MVHP_FAILURE;
    c->hist_band = rows;
    return MVHP_SUCCESS;
}

// Everything a wide launch needs besides the batch: seam granules for its band boundaries (grown on demand, zeroed once: a
// granule counts when its tag equals the launch's epoch, and epochs never repeat), the ticket base, ordering behind the
// context's previous wide launch when that ran on another stream (they share the counter and the seams).
static int wide_prepare(mvhp_ctx *c, mvhp::ReconArgs &a, size_t seam_bytes, hipStream_t st)
{
    if (c->wide_stream && c->wide_stream != st) HIP_TRY(hipStreamWaitEvent(st, c->wide_done, 0));
    if (seam_bytes > c->d_seam_bytes) {
        if (c->d_seam) {
            HIP_TRY(hipEventSynchronize(c->wide_done));   // (the previous wide launch may still read the old one)
            HIP_TRY(hipFree(c->d_seam));
            c->d_seam = nullptr;
            c->d_seam_bytes = 0;
        }
        const size_t want = seam_bytes + seam_bytes / 4;
        HIP_TRY(hipMalloc(&c->d_seam, want));
        c->d_seam_bytes = want;
        HIP_TRY(hipMemsetAsync(c->d_seam, 0, want, st));
    }
    if (++c->wide_epoch == 0) {   // 2^32 launches later: tags would repeat
        if (c->d_seam) HIP_TRY(hipMemsetAsync(c->d_seam, 0, c->d_seam_bytes, st));
        c->wide_epoch = 1;
    }
    a.wide_ticket = c->d_ticket;
    a.wide_base = c->ticket_base + (uint32_t)c->ticket_skew_once;
    c->ticket_skew_once = 0;
    a.wide_epoch = c->wide_epoch;
    a.seam = (unsigned long long *)c->d_seam;
    c->wide_stream = st;
    return MVHP_SUCCESS;
}

// Waits for `st` and reads the context's error word behind it (bit 0 / 1: reconstruction kernels, bit 2: deblocking kernel).
// text: empty when the word is clear, else what it means -- with the word itself in front (with_word) or without.  The word is
// left as it is: what clears it, and how, is the caller's business.
static hipError_t read_err_word(mvhp_ctx *c, hipStream_t st, bool with_word, std::string &text)
{
    uint32_t err = 0;
    hipError_t e = hipMemcpyAsync(&err, c->d_err, sizeof(err), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    text.clear();
    if (e != hipSuccess || !err) return e;
    const char *what = (err & 2u) ? "a workgroup's ticket lay outside the launch" : (err & 1u) ? "row dependency wait timed out"
                     : (err & 4u) ? "deblocking row wait timed out" : "unknown";
    char word[16] = "";
    if (with_word) snprintf(word, sizeof(word), " 0x%x", err);
    text = std::string("reconstruction kernel reported error word") + word + " (" + what + ")";
    return hipSuccess;
}

// recon: the reconstruction kernel; deblock: the deblocking kernel over d_yuv (in place); color: RGB into d_rgb.  A deblocked
// batch converts to RGB in the separate colour kernel: the reconstruction kernel's fused epilogue would see unfiltered samples.
static int launch_all(mvhp_ctx *c, const mvhp_stream_params_t *p, const void *d_packed, int n_frames,
                      uint8_t *d_yuv, uint8_t *d_rgb, hipStream_t st, bool recon, bool color, bool deblock)
{
    const bool fuse = recon && c->fused_color && !deblock;
    if (deblock && mvhp::deblock_lds_bytes((int)p->width_mbs, mvhp::deblock_waves(n_frames)) > c->max_lds) {
        set_err("picture too wide for the deblocking line buffer (%u macroblocks)", p->width_mbs);
        return MVHP_UNSUPPORTED;
    }
    if (recon) {
        mvhp::ReconArgs a;
        a.packed = (const uint8_t *)d_packed;
        a.yuv = d_yuv;
        a.rgb = (fuse && color) ? d_rgb : nullptr;
        a.err = c->d_err;
        a.width_mbs = (int)p->width_mbs;
        a.height_mbs = (int)p->height_mbs;
        a.cqp_off_cb = p->chroma_qp_index_offset;
        a.cqp_off_cr = p->second_chroma_qp_index_offset;
        a.n_frames = n_frames;
        a.dc_shift_from = (p->flags & MVHP_PARAM_SPEC_LUMA_DC) ? 36 : 37;
        a.slices = (p->flags & MVHP_PARAM_SLICES) ? 1 : 0;
        a.scaling = (p->flags & MVHP_PARAM_SCALING) ? 1 : 0;
        if (a.scaling) {
            memcpy(a.weights, p->scaling4, 48);
            memcpy(a.weights + 48, p->scaling8, 64);
        } else {
            memset(a.weights, 16, sizeof(a.weights));
        }
        a.wide_ticket = nullptr;
        a.wide_base = a.wide_epoch = 0;
        a.seam = nullptr;
        const mvhp::LaunchPlan plan = mvhp::plan_launch(plan_device(c), *p, n_frames);
        const mvhp::KernelForm &form = mvhp::kernel_form(plan.layout);
        c->last_layout = plan.layout;
        c->last_waves = plan.waves;
        // (rows and wide only: the planner takes every other form off pictures whose line buffers do not fit)
        if (form.lds_bytes(a.width_mbs, plan.waves) > c->max_lds) {
            set_err("picture too wide for the LDS line buffer (%u macroblocks)", p->width_mbs);
            return MVHP_UNSUPPORTED;
        }
        if (form.banded) {
            const int rc = wide_prepare(c, a, plan.seam_bytes, st);
            if (rc != MVHP_SUCCESS) return rc;
        }
        HIP_TRY(form.launch(a, plan.waves, st));
        if (form.banded) {
            c->ticket_base += plan.tickets;   // every workgroup takes one ticket
            HIP_TRY(hipEventRecord(c->wide_done, st));
        }
    }
    if (deblock) {
        mvhp::DeblockArgs da;
        da.packed = (const uint8_t *)d_packed;
        da.yuv = d_yuv;
        da.err = c->d_err;
        da.width_mbs = (int)p->width_mbs;
        da.height_mbs = (int)p->height_mbs;
        da.n_frames = n_frames;
        da.cqp_off_cb = p->chroma_qp_index_offset;
        da.cqp_off_cr = p->second_chroma_qp_index_offset;
        HIP_TRY(mvhp::launch_deblock(da, mvhp::deblock_waves(n_frames), st));
    }
    if (color && d_rgb && !fuse) {
        mvhp::ColorArgs ca;
        ca.yuv = d_yuv;
        ca.rgb = d_rgb;
        ca.width_mbs = (int)p->width_mbs;
        ca.height_mbs = (int)p->height_mbs;
        ca.n_frames = n_frames;
        HIP_TRY(mvhp::launch_color(ca, st));
    }
    return MVHP_SUCCESS;
}

MVHP_EXPORT size_t mvhp_recon_align(void) { return MVHP_RECON_ALIGN; }

// The caller buffers of the three reconstruction entry points (MVHP_RECON_ALIGN in minivideo_hotpath.h: the kernels behind them
// use naturally aligned 16-byte accesses): true when `ptr` (NULL passes: an absent optional buffer) is aligned, else the error
// text names the argument.  Asked before hipSetDevice and before anything is launched.
static bool recon_aligned(const char *fn, const char *arg, const void *ptr)
{
    if (((uintptr_t)ptr & (uintptr_t)(MVHP_RECON_ALIGN - 1)) == 0) return true;
    set_err("%s: %s is not %d-byte aligned", fn, arg, MVHP_RECON_ALIGN);
    return false;
}

MVHP_EXPORT int mvhp_recon_batch_dev(mvhp_ctx_t *c, const mvhp_stream_params_t *p, const void *d_packed,
                                     int n_frames, uint8_t *d_yuv, uint8_t *d_rgb, void *stream)
{
    if (!c || !params_ok(p) || !d_packed || !d_yuv || n_frames <= 0) {
        set_err("mvhp_recon_batch_dev: invalid argument");
        return MVHP_FAILURE;
    }
    if (!recon_aligned("mvhp_recon_batch_dev", "d_packed", d_packed) || !recon_aligned("mvhp_recon_batch_dev", "d_yuv", d_yuv) ||
        !recon_aligned("mvhp_recon_batch_dev", "d_rgb", d_rgb))
        return MVHP_FAILURE;
    HIP_TRY(hipSetDevice(c->device));
    return launch_all(c, p, d_packed, n_frames, d_yuv, d_rgb, stream_of(c, stream), true, true, (p->flags & MVHP_PARAM_DEBLOCK) != 0);
}

MVHP_EXPORT int mvhp_expand_compact_dev(mvhp_ctx_t *c, const mvhp_stream_params_t *p, const void *d_compact, size_t stride,
                                        int n_pictures, void *d_packed, void *stream)
{
    if (!c || !params_ok(p) || !d_compact || !d_packed || n_pictures <= 0 || (stride & 3) ||
        stride < (size_t)p->width_mbs * p->height_mbs * 4 + MVHP_MB_HEADER_BYTES) {
        set_err("mvhp_expand_compact_dev: invalid argument");
        return MVHP_FAILURE;
    }
    if (!recon_aligned("mvhp_expand_compact_dev", "d_compact", d_compact) || !recon_aligned("mvhp_expand_compact_dev", "d_packed", d_packed))
        return MVHP_FAILURE;
    HIP_TRY(hipSetDevice(c->device));
    mvhp::ExpandArgs a;
    a.compact = (const uint8_t *)d_compact;
    a.stride = stride;
    a.packed = (uint8_t *)d_packed;
    a.mbs = (int)(p->width_mbs * p->height_mbs);
    a.n_pictures = n_pictures;
    HIP_TRY(mvhp::launch_expand(a, stream_of(c, stream)));
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_recon_stages_dev(mvhp_ctx_t *c, const mvhp_stream_params_t *p, const void *d_packed,
                                      int n_frames, uint8_t *d_yuv, uint8_t *d_rgb, void *stream, int stages)
{
    if (!c || !params_ok(p) || !d_packed || !d_yuv || n_frames <= 0 || (stages & ~7) || !stages) {
        set_err("mvhp_recon_stages_dev: invalid argument");
        return MVHP_FAILURE;
    }
    if (!recon_aligned("mvhp_recon_stages_dev", "d_packed", d_packed) || !recon_aligned("mvhp_recon_stages_dev", "d_yuv", d_yuv) ||
        !recon_aligned("mvhp_recon_stages_dev", "d_rgb", d_rgb))
        return MVHP_FAILURE;
    HIP_TRY(hipSetDevice(c->device));
    const hipStream_t st = stream_of(c, stream);
    const bool recon = (stages & MVHP_STAGE_RECON) != 0;
    return launch_all(c, p, d_packed, n_frames, d_yuv, d_rgb, st, recon, (stages & MVHP_STAGE_COLOR) != 0,
                      (stages & MVHP_STAGE_DEBLOCK) || (recon && (p->flags & MVHP_PARAM_DEBLOCK)));
}

MVHP_EXPORT int mvhp_resample_dev(mvhp_ctx_t *c, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g,
                                  const uint8_t *d_yuv_coded, int n, uint8_t *d_yuv_out, uint8_t *d_rgb_out, void *stream)
{
    if (!c || !params_ok(p) || !g || !d_yuv_coded || n <= 0 || ((uintptr_t)d_yuv_coded & 15) || ((uintptr_t)d_yuv_out & 3) ||
        ((uintptr_t)d_rgb_out & 3)) {
        set_err("mvhp_resample_dev: invalid argument");
        return MVHP_FAILURE;
    }
    const uint32_t Wp = p->width_mbs * 16, Hp = p->height_mbs * 16;
    const bool even = ((g->crop_x | g->crop_y | g->crop_w | g->crop_h | g->out_w | g->out_h) & 1u) == 0;
    if (!even || g->crop_w < 2 || g->crop_h < 2 || g->crop_x > Wp || g->crop_w > Wp - g->crop_x || g->crop_y > Hp ||
        g->crop_h > Hp - g->crop_y || g->out_w < 2 || g->out_h < 2 || g->out_w > g->crop_w || g->out_h > g->crop_h) {
        set_err("mvhp_resample_dev: geometry outside the coded picture (crop %u,%u %ux%u -> %ux%u of %ux%u)", g->crop_x,
                g->crop_y, g->crop_w, g->crop_h, g->out_w, g->out_h, Wp, Hp);
        return MVHP_FAILURE;
    }
    HIP_TRY(hipSetDevice(c->device));
    mvhp::ResampleArgs a;
    a.src = d_yuv_coded;
    a.yuv = d_yuv_out;
    a.rgb = d_rgb_out;
    a.width_mbs = (int)p->width_mbs;
    a.height_mbs = (int)p->height_mbs;
    a.n_frames = n;
    a.cx = (int)g->crop_x; a.cy = (int)g->crop_y; a.cw = (int)g->crop_w; a.ch = (int)g->crop_h;
    a.ow = (int)g->out_w; a.oh = (int)g->out_h;
    if (c->crop_copy && a.ow == a.cw && a.oh == a.ch) {   // crop only: a copy (the same bytes; no LDS row buffers, so any width)
        if (!d_yuv_out && !d_rgb_out) return MVHP_SUCCESS;
        // chroma rows per workgroup: eight (sixteen luma rows: about eight 16-byte blocks per lane at 1080p), fewer when the
        // grid would leave CUs idle
        int band = 8;
        while (band > 1 && (double)n * ((a.ch / 2 + band - 1) / band) < 4.0 * c->n_cus) band /= 2;
        a.band = band;
        HIP_TRY(mvhp::launch_crop_copy(a, stream_of(c, stream)));
        return MVHP_SUCCESS;
    }
    // chroma output rows per workgroup: four (eight luma rows), fewer when that would leave CUs idle or not fit the LDS
    int band = 4;
    while (band > 1 && (double)n * ((a.oh / 2 + band - 1) / band) < 4.0 * c->n_cus) band /= 2;
    while (band > 1 && mvhp::resample_lds_bytes(a.cw, a.ow, band) > c->max_lds) band /= 2;
    if (mvhp::resample_lds_bytes(a.cw, a.ow, band) > c->max_lds) {
        set_err("mvhp_resample_dev: picture too wide for the LDS row buffers (%u samples)", g->crop_w);
        return MVHP_UNSUPPORTED;
    }
    a.band = band;
    if (!d_yuv_out && !d_rgb_out) return MVHP_SUCCESS;
    HIP_TRY(mvhp::launch_resample(a, stream_of(c, stream)));
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_orient_dev(mvhp_ctx_t *c, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g, int quarter_turns,
                                uint32_t src_flags, const uint8_t *d_src, int n, uint8_t *d_yuv_out, uint8_t *d_rgb_out, void *stream)
{
    const bool coded = (src_flags & MVHP_ORIENT_SRC_CODED) != 0;
    if (!c || !g || !d_src || n < 0 || quarter_turns < 0 || quarter_turns > 3 || (src_flags & ~MVHP_ORIENT_SRC_CODED) ||
        (coded && !params_ok(p)) || ((uintptr_t)d_src & (coded ? 15 : 3)) || ((uintptr_t)d_yuv_out & 3) || ((uintptr_t)d_rgb_out & 3)) {
        set_err("mvhp_orient_dev: invalid argument");
        return MVHP_FAILURE;
    }
    if (((g->out_w | g->out_h) & 1u) || g->out_w < 2 || g->out_h < 2 || g->out_w > 16384 || g->out_h > 16384) {
        set_err("mvhp_orient_dev: pictures of %u x %u (even sides of 2 to 16384)", g->out_w, g->out_h);
        return MVHP_FAILURE;
    }
    mvhp::OrientArgs a;
    a.w = (int)g->out_w;
    a.h = (int)g->out_h;
    if (coded) {
        const uint32_t Wp = p->width_mbs * 16, Hp = p->height_mbs * 16;
        if (((g->crop_x | g->crop_y | g->crop_w | g->crop_h) & 1u) || g->crop_w < 2 || g->crop_h < 2 || g->crop_x > Wp ||
            g->crop_w > Wp - g->crop_x || g->crop_y > Hp || g->crop_h > Hp - g->crop_y || g->out_w != g->crop_w || g->out_h != g->crop_h) {
            set_err("mvhp_orient_dev: rectangle %u,%u %ux%u -> %ux%u of a %ux%u picture (even, inside the picture, not scaled)",
                    g->crop_x, g->crop_y, g->crop_w, g->crop_h, g->out_w, g->out_h, Wp, Hp);
            return MVHP_FAILURE;
        }
        a.pitch = (int)Wp;
        a.frame_bytes = mvhp_yuv_frame_bytes(p);
        a.y_off = (size_t)g->crop_y * Wp + g->crop_x;
        a.cb_off = (size_t)Wp * Hp + (size_t)(g->crop_y >> 1) * (Wp >> 1) + (g->crop_x >> 1);
        a.cr_off = a.cb_off + (size_t)(Wp >> 1) * (Hp >> 1);
    } else {
        a.pitch = a.w;
        a.frame_bytes = (size_t)a.w * a.h * 3 / 2;
        a.y_off = 0;
        a.cb_off = (size_t)a.w * a.h;
        a.cr_off = a.cb_off + (size_t)(a.w >> 1) * (a.h >> 1);
    }
    if (n == 0 || (!d_yuv_out && !d_rgb_out)) return MVHP_SUCCESS;
    HIP_TRY(hipSetDevice(c->device));
    a.src = d_src;
    a.src_end = d_src + (((size_t)n * a.frame_bytes) & ~(size_t)3);
    a.turns = quarter_turns;
    a.n = n;
    a.yuv = d_yuv_out;
    a.rgb = d_rgb_out;
    // 0 and 2 turns, chroma rows per workgroup: the rule of the crop copy above (1 and 3 turns run in tiles)
    int band = 8;
    while (band > 1 && (double)n * ((a.h / 2 + band - 1) / band) < 4.0 * c->n_cus) band /= 2;
    a.band = band;
    HIP_TRY(mvhp::launch_orient(a, stream_of(c, stream)));
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_color_dev(mvhp_ctx_t *c, const mvhp_output_geometry_t *g, const mvhp_color_params_t *cp, const uint8_t *d_yuv, int n,
                               uint8_t *d_rgb_out, void *stream)
{
    if (!c || !g || !cp || !d_yuv || !d_rgb_out || n < 0 || ((uintptr_t)d_yuv & 3) || ((uintptr_t)d_rgb_out & 3)) {
        set_err("mvhp_color_dev: invalid argument");
        return MVHP_FAILURE;
    }
    if (((g->out_w | g->out_h) & 1u) || g->out_w < 2 || g->out_h < 2 || g->out_w > 16384 || g->out_h > 16384) {
        set_err("mvhp_color_dev: pictures of %u x %u (even sides of 2 to 16384)", g->out_w, g->out_h);
        return MVHP_FAILURE;
    }
    int32_t k[6];
    if (cp->siting < MVHP_CHROMA_NEAREST || cp->siting > MVHP_CHROMA_CENTER || cp->reserved != 0 ||
        mvhp_color_coefficients(cp->matrix, cp->full_range, k) != MVHP_SUCCESS) {
        set_err("mvhp_color_dev: parameters {matrix %d, full_range %d, siting %d} are not ones the header names", cp->matrix, cp->full_range, cp->siting);
        return MVHP_FAILURE;
    }
    if (n == 0) return MVHP_SUCCESS;
    HIP_TRY(hipSetDevice(c->device));
    mvhp::ColorConvertArgs a;
    a.w = (int)g->out_w;
    a.h = (int)g->out_h;
    a.n = n;
    a.yuv = d_yuv;
    a.yuv_end = d_yuv + (((size_t)n * ((size_t)a.w * a.h * 3 / 2)) & ~(size_t)3);
    a.rgb = d_rgb_out;
    a.siting = cp->siting;
    a.ymul = 16 * k[0]; a.crv = k[1]; a.cbu = k[2]; a.gcb = k[3]; a.gcr = k[4]; a.yoff = k[5];
    // chroma rows per workgroup: the rule of the crop copy and the turn (fewer where the launch would leave CUs idle)
    int band = 8;
    while (band > 1 && (double)n * ((a.h / 2 + band - 1) / band) < 4.0 * c->n_cus) band /= 2;
    a.band = band;
    HIP_TRY(mvhp::launch_color_convert(a, stream_of(c, stream)));
    return MVHP_SUCCESS;
}

static int ensure(void **ptr, size_t *have, size_t need)
{
    if (*have >= need) return MVHP_SUCCESS;
    if (*ptr) hipFree(*ptr);
    *ptr = nullptr;
    *have = 0;
    HIP_TRY(hipMalloc(ptr, need));
    *have = need;
    return MVHP_SUCCESS;
}

MVHP_EXPORT uint32_t mvhp_luma_score(const mvhp_luma_stats_t *st)
{
    return st ? mvblank::luma_score(st->sum, st->sumsq, st->samples) : 0;
}

MVHP_EXPORT int mvhp_blank_choose(const uint32_t *scores, int n, uint32_t min_score) { return mvblank::choose(scores, n, min_score); }

MVHP_EXPORT int mvhp_luma_stats_dev(mvhp_ctx_t *c, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g,
                                    const uint8_t *d_yuv_coded, int n, mvhp_luma_stats_t *d_stats, void *stream)
{
    if (!c || !params_ok(p) || !g || !d_yuv_coded || n < 0 || ((uintptr_t)d_yuv_coded & 15) || !d_stats || ((uintptr_t)d_stats & 7)) {
        set_err("mvhp_luma_stats_dev: invalid argument");
        return MVHP_FAILURE;
    }
    const uint32_t Wp = p->width_mbs * 16, Hp = p->height_mbs * 16;
    if (((g->crop_x | g->crop_y | g->crop_w | g->crop_h) & 1u) || g->crop_w < 2 || g->crop_h < 2 || g->crop_x > Wp ||
        g->crop_w > Wp - g->crop_x || g->crop_y > Hp || g->crop_h > Hp - g->crop_y) {
        set_err("mvhp_luma_stats_dev: rectangle %u,%u %ux%u of a %ux%u picture (even offsets and sizes of at least 2, inside the picture)",
                g->crop_x, g->crop_y, g->crop_w, g->crop_h, Wp, Hp);
        return MVHP_FAILURE;
    }
    if ((uint64_t)g->crop_w * g->crop_h > ((uint64_t)1 << 28)) {   // `samples` and the score's arithmetic are sized for this
        set_err("mvhp_luma_stats_dev: rectangles of %u x %u are too large (at most 2^28 samples)", g->crop_w, g->crop_h);
        return MVHP_UNSUPPORTED;
    }
    if (n == 0) return MVHP_SUCCESS;
    HIP_TRY(hipSetDevice(c->device));
    mvhp::LumaStatsArgs a;
    a.src = d_yuv_coded;
    a.frame_bytes = mvhp_yuv_frame_bytes(p);
    a.n = n;
    a.pitch = (int)Wp;
    a.cx = (int)g->crop_x; a.cy = (int)g->crop_y; a.cw = (int)g->crop_w; a.ch = (int)g->crop_h;
    // luma rows per workgroup: sixteen (at 1080p 1920 blocks of 16 bytes, 7.5 per lane), fewer when the grid would leave CUs
    // idle -- the rule of the crop copy above.  Speed only: the sums are integers, any band size gives the same record.
    int band = c->stats_band > 0 ? c->stats_band : 16;
    while (c->stats_band <= 0 && band > 1 && (double)n * ((a.ch + band - 1) / band) < 4.0 * c->n_cus) band /= 2;
    a.band = band;
    a.stats = d_stats;
    HIP_TRY(mvhp::launch_luma_stats(a, stream_of(c, stream)));
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_luma_bars_dev(mvhp_ctx_t *c, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g,
                                   const uint8_t *d_yuv_coded, int n, int level, mvhp_luma_bars_t *d_bars, void *stream)
{
    if (!c || !params_ok(p) || !g || !d_yuv_coded || n < 0 || ((uintptr_t)d_yuv_coded & 15) || !d_bars || ((uintptr_t)d_bars & 7)) {
        set_err("mvhp_luma_bars_dev: invalid argument");
        return MVHP_FAILURE;
    }
    if (level < 1 || level > 254) {
        set_err("mvhp_luma_bars_dev: level %d (1 ... 254)", level);
        return MVHP_FAILURE;
    }
    const uint32_t Wp = p->width_mbs * 16, Hp = p->height_mbs * 16;
    if (((g->crop_x | g->crop_y | g->crop_w | g->crop_h) & 1u) || g->crop_w < 2 || g->crop_h < 2 || g->crop_x > Wp ||
        g->crop_w > Wp - g->crop_x || g->crop_y > Hp || g->crop_h > Hp - g->crop_y) {
        set_err("mvhp_luma_bars_dev: rectangle %u,%u %ux%u of a %ux%u picture (even offsets and sizes of at least 2, inside the picture)",
                g->crop_x, g->crop_y, g->crop_w, g->crop_h, Wp, Hp);
        return MVHP_FAILURE;
    }
    if (n == 0) return MVHP_SUCCESS;
    HIP_TRY(hipSetDevice(c->device));
    mvhp::LumaBarsArgs a{};
    a.src = d_yuv_coded;
    a.frame_bytes = mvhp_yuv_frame_bytes(p);
    a.n = n;
    a.pitch = (int)Wp;
    a.cx = (int)g->crop_x; a.cy = (int)g->crop_y; a.cw = (int)g->crop_w; a.ch = (int)g->crop_h;
    a.level = level;
    // luma rows per workgroup of the counting pass.  Every band adds its column counts to the picture's counters, cw atomic adds
    // a band, so: as few bands as the kernel's LDS tile of 1024 rows gives (1080p: two of 540 rows -- 2048 pictures issue 8 M
    // adds, not the 260 M of sixteen-row bands), doubled while the grid would leave compute units idle and a band keeps sixteen
    // rows.  Speed only: the counts are integers, any band size gives the same record.
    int band = c->bars_band;
    if (band <= 0) {
        int bands = (a.ch + 1023) / 1024;
        while ((double)n * bands < 4.0 * c->n_cus && (a.ch + 2 * bands - 1) / (2 * bands) >= 16) bands *= 2;
        band = (a.ch + bands - 1) / bands;
    }
    a.band = band;
    a.bars = d_bars;
    const hipStream_t st = stream_of(c, stream);
    const size_t need = mvhp::luma_bars_scratch_bytes(a);
    if (!c->bars_done) HIP_TRY(hipEventCreateWithFlags(&c->bars_done, hipEventDisableTiming));
    if (ensure(&c->d_bars, &c->d_bars_bytes, need) != MVHP_SUCCESS) return MVHP_FAILURE;   // (hipFree waits for the device)
    if (c->bars_stream && c->bars_stream != st) HIP_TRY(hipStreamWaitEvent(st, c->bars_done, 0));
    a.scratch = (uint32_t *)c->d_bars;
    HIP_TRY(mvhp::launch_luma_bars(a, st));
    HIP_TRY(hipEventRecord(c->bars_done, st));
    c->bars_stream = st;
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_hist_stats(const mvhp_plane_hist_t *h, mvhp_luma_stats_t *out)
{
    if (!h || !out) return MVHP_FAILURE;
    mvrep::hist_stats(*h, *out);
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_represent_choose(const mvhp_plane_hist_t *h, int n, const uint8_t *eligible) { return mvrep::choose(h, n, eligible); }

MVHP_EXPORT int mvhp_plane_hist_dev(mvhp_ctx_t *c, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g,
                                    const uint8_t *d_yuv_coded, int n, mvhp_plane_hist_t *d_hist, void *stream)
{
    if (!c || !params_ok(p) || !g || !d_yuv_coded || n < 0 || ((uintptr_t)d_yuv_coded & 15) || !d_hist || ((uintptr_t)d_hist & 15)) {
        set_err("mvhp_plane_hist_dev: invalid argument");
        return MVHP_FAILURE;
    }
    const uint32_t Wp = p->width_mbs * 16, Hp = p->height_mbs * 16;
    if (((g->crop_x | g->crop_y | g->crop_w | g->crop_h) & 1u) || g->crop_w < 2 || g->crop_h < 2 || g->crop_x > Wp ||
        g->crop_w > Wp - g->crop_x || g->crop_y > Hp || g->crop_h > Hp - g->crop_y) {
        set_err("mvhp_plane_hist_dev: rectangle %u,%u %ux%u of a %ux%u picture (even offsets and sizes of at least 2, inside the picture)",
                g->crop_x, g->crop_y, g->crop_w, g->crop_h, Wp, Hp);
        return MVHP_FAILURE;
    }
    // (a coded picture has at most 2^28 samples: `samples`, every count and the choice's arithmetic are sized for that)
    if (n == 0) return MVHP_SUCCESS;
    HIP_TRY(hipSetDevice(c->device));
    mvhp::PlaneHistArgs a;
    a.src = d_yuv_coded;
    a.frame_bytes = mvhp_yuv_frame_bytes(p);
    a.n = n;
    a.pitch = (int)Wp;
    a.rows = (int)Hp;
    a.cx = (int)g->crop_x; a.cy = (int)g->crop_y; a.cw = (int)g->crop_w; a.ch = (int)g->crop_h;
    // luma rows per workgroup: a workgroup zeroes and sums 48 KiB of LDS and issues up to 768 atomic adds whatever its band, so
    // bands are tall (256 rows: 1080p in five; measured against 16 ... 1080 rows, DESIGN.md 3 "Representative pictures"), halved
    // while the grid would leave CUs idle -- the rule of the crop copy above.  Speed only: the counts are integers, any band size
    // gives the same record.
    int band = c->hist_band > 0 ? c->hist_band : 256;
    while (c->hist_band <= 0 && band > 1 && (double)n * ((a.ch + band - 1) / band) < 4.0 * c->n_cus) band /= 2;
    a.band = band;
    a.hist = d_hist;
    HIP_TRY(mvhp::launch_plane_hist(a, stream_of(c, stream)));
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_tensor_dev(mvhp_ctx_t *c, const mvhp_tensor_params_t *t, const uint8_t *d_rgb, int n, void *d_out,
                                const int32_t *d_slots, void *stream)
{
    if (!c || !t) { set_err("mvhp_tensor_dev: no %s", c ? "parameters" : "context"); return MVHP_FAILURE; }
    if (const char *why = mvtensor::malformed(*t)) { set_err("mvhp_tensor_dev: invalid %s", why); return MVHP_FAILURE; }
    if (!mvtensor::finite(*t)) { set_err("mvhp_tensor_dev: scale / bias is not finite"); return MVHP_FAILURE; }
    if (n < 0) { set_err("mvhp_tensor_dev: n = %d", n); return MVHP_FAILURE; }
    if (!d_rgb || ((uintptr_t)d_rgb & 3)) { set_err("mvhp_tensor_dev: d_rgb is NULL or not 4-byte aligned"); return MVHP_FAILURE; }
    if (!d_out || ((uintptr_t)d_out & 15)) { set_err("mvhp_tensor_dev: d_out is NULL or not 16-byte aligned"); return MVHP_FAILURE; }
    if ((uintptr_t)d_slots & 3) { set_err("mvhp_tensor_dev: d_slots is not 4-byte aligned"); return MVHP_FAILURE; }
    if (n == 0) return MVHP_SUCCESS;
    HIP_TRY(hipSetDevice(c->device));
    mvhp::TensorArgs a{};
    a.src = d_rgb;
    a.src_end = d_rgb + (size_t)n * 3 * t->src_w * t->src_h;
    a.n = n;
    a.sw = (int)t->src_w; a.sh = (int)t->src_h;
    a.cw = (int)mvtensor::canvas_w(*t); a.ch = (int)mvtensor::canvas_h(*t);
    a.dtype = (int)t->dtype; a.layout = (int)t->layout; a.bgr = (t->flags & MVHP_TENSOR_BGR) != 0;
    a.pad_rgb = t->pad_rgb;
    for (int k = 0; k < 3; k++) { a.scale[k] = t->scale[k]; a.bias[k] = t->bias[k]; }
    // canvas rows per workgroup: about 16 KiB of source (a row of the widest picture is 48 KiB: one row then) and at most 64 KiB of
    // tensor, so that several workgroups share a CU; halved while the grid would leave CUs idle -- the rule of the crop copy above.
    // Speed only: every element is made by one lane from its own sample.
    const size_t es = mvtensor::element_bytes(t->dtype);
    int rows = std::max(1, std::min(64, 16384 / (3 * a.sw)));
    rows = std::min(rows, std::max(1, (int)(65536 / ((size_t)a.cw * 3 * es))));
    rows = std::min(rows, a.ch);
    while (rows > 1 && (double)n * ((a.ch + rows - 1) / rows) < 4.0 * c->n_cus) rows = (rows + 1) / 2;
    // (a forced value, as far as a workgroup's LDS -- 64 KiB -- holds the source rows and 32-bit counts the strip's elements)
    if (c->tensor_rows > 0) rows = std::max(1, std::min(std::min(c->tensor_rows, a.ch), std::min(4096, (65536 - 64) / (3 * a.sw))));
    a.rows = rows;
    a.out = (uint8_t *)d_out;
    a.tensor_bytes = mvtensor::bytes(*t);
    a.slots = d_slots;
    HIP_TRY(mvhp::launch_tensor(a, stream_of(c, stream)));
    return MVHP_SUCCESS;
}

MVHP_EXPORT size_t mvhp_jpeg_header_bytes(void) { return MVHP_JPEG_HEADER_BYTES; }

MVHP_EXPORT int mvhp_jpeg_quant_tables(int quality, uint8_t out[128])
{
    if (!out) return MVHP_FAILURE;
    mvhp::jpeg_quant_tables(quality, out);
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_jpeg_encode_dev(mvhp_ctx_t *c, const mvhp_output_geometry_t *g, const mvhp_jpeg_params_t *jp,
                                     const uint8_t *d_yuv, int n, uint8_t *d_blob, size_t cap_bytes, mvhp_jpeg_entry_t *d_table,
                                     void *stream)
{
    if (!c || !g || !jp || !d_yuv || n <= 0 || !d_blob || ((uintptr_t)d_blob & 15) || !d_table || ((uintptr_t)d_table & 7) ||
        (jp->reserved & ~7u)) {
        set_err("mvhp_jpeg_encode_dev: invalid argument");
        return MVHP_FAILURE;
    }
    if (((g->out_w | g->out_h) & 1u) || g->out_w < 2 || g->out_h < 2 || g->out_w > 65534 || g->out_h > 65534) {
        set_err("mvhp_jpeg_encode_dev: pictures of %u x %u cannot be coded (even sides of 2 .. 65534)", g->out_w, g->out_h);
        return MVHP_FAILURE;
    }
    if ((uint64_t)g->out_w * g->out_h > ((uint64_t)1 << 28)) {   // lengths are 32-bit: a file is at most 6.5 x its raw picture
        set_err("mvhp_jpeg_encode_dev: pictures of %u x %u are too large (at most 2^28 samples of luma)", g->out_w, g->out_h);
        return MVHP_UNSUPPORTED;
    }
    mvhp::JpegArgs a;
    a.yuv = d_yuv;
    a.n = n;
    a.w = (int)g->out_w;
    a.h = (int)g->out_h;
    a.quality = jp->quality < 1 ? 1 : jp->quality > 100 ? 100 : jp->quality;
    a.restart = jp->restart_mcus ? (int)jp->restart_mcus : (a.w + 15) / 16;
    if (jp->restart_mcus > 65535) {
        set_err("mvhp_jpeg_encode_dev: restart interval of %u MCUs (1 .. 65535)", jp->restart_mcus);
        return MVHP_FAILURE;
    }
    a.stages = jp->reserved ? (int)jp->reserved : (int)(MVHP_JPEG_STAGE_DCT | MVHP_JPEG_STAGE_COUNT | MVHP_JPEG_STAGE_WRITE);
    a.blob = d_blob;
    a.cap = cap_bytes;
    a.table = d_table;
    HIP_TRY(hipSetDevice(c->device));
    const hipStream_t st = stream_of(c, stream);
    const size_t need = mvhp::jpeg_scratch_bytes(a);
    if (jp->reserved && c->d_jpeg_bytes < need) {
        set_err("mvhp_jpeg_encode_dev: single stages need a whole call with the same arguments before them");
        return MVHP_FAILURE;
    }
    if (!c->jpeg_done) HIP_TRY(hipEventCreateWithFlags(&c->jpeg_done, hipEventDisableTiming));
    if (ensure(&c->d_jpeg, &c->d_jpeg_bytes, need) != MVHP_SUCCESS) return MVHP_FAILURE;   // (hipFree waits for the device)
    if (c->jpeg_stream && c->jpeg_stream != st) HIP_TRY(hipStreamWaitEvent(st, c->jpeg_done, 0));
    a.scratch = (uint8_t *)c->d_jpeg;
    HIP_TRY(mvhp::launch_jpeg_encode(a, st));
    HIP_TRY(hipEventRecord(c->jpeg_done, st));
    c->jpeg_stream = st;
    return MVHP_SUCCESS;
}

MVHP_EXPORT size_t mvhp_png_header_bytes(void) { return MVHP_PNG_HEADER_BYTES; }

MVHP_EXPORT int mvhp_png_segment_rows(int w) { return mvhp::png_segment_rows(w); }

MVHP_EXPORT size_t mvhp_png_max_bytes(int w, int h) { return mvhp::png_max_bytes(w, h); }

MVHP_EXPORT int mvhp_png_encode_dev(mvhp_ctx_t *c, const mvhp_output_geometry_t *g, const mvhp_png_params_t *pp,
                                    const uint8_t *d_rgb, int n, uint8_t *d_blob, size_t cap_bytes, mvhp_png_entry_t *d_table,
                                    void *stream)
{
    if (!c || !g || !pp || !d_rgb || ((uintptr_t)d_rgb & 3) || n < 0 || !d_blob || ((uintptr_t)d_blob & 15) || !d_table ||
        ((uintptr_t)d_table & 7) || (pp->reserved & ~7u)) {
        set_err("mvhp_png_encode_dev: invalid argument");
        return MVHP_FAILURE;
    }
    if (((g->out_w | g->out_h) & 1u) || g->out_w < 2 || g->out_h < 2 || g->out_w > MVHP_PNG_MAX_WIDTH) {
        set_err("mvhp_png_encode_dev: pictures of %u x %u cannot be coded (even sides of at least 2, widths up to %d: a filtered "
                "row has to fit a stored block)", g->out_w, g->out_h, MVHP_PNG_MAX_WIDTH);
        return MVHP_FAILURE;
    }
    if ((uint64_t)g->out_w * g->out_h > ((uint64_t)1 << 28)) {   // lengths are 32-bit: a file is at most 3.01 x its samples
        set_err("mvhp_png_encode_dev: pictures of %u x %u are too large (at most 2^28 samples)", g->out_w, g->out_h);
        return MVHP_UNSUPPORTED;
    }
    if (n == 0) return MVHP_SUCCESS;
    mvhp::PngArgs a;
    a.rgb = d_rgb;
    a.n = n;
    a.w = (int)g->out_w;
    a.h = (int)g->out_h;
    a.stages = pp->reserved ? (int)pp->reserved : (int)(MVHP_PNG_STAGE_ANALYSE | MVHP_PNG_STAGE_PLACE | MVHP_PNG_STAGE_WRITE);
    a.blob = d_blob;
    a.cap = cap_bytes;
    a.table = d_table;
    HIP_TRY(hipSetDevice(c->device));
    const hipStream_t st = stream_of(c, stream);
    const size_t need = mvhp::png_scratch_bytes(a);
    if (pp->reserved && c->d_png_bytes < need) {
        set_err("mvhp_png_encode_dev: single stages need a whole call with the same arguments before them");
        return MVHP_FAILURE;
    }
    if (!c->png_done) HIP_TRY(hipEventCreateWithFlags(&c->png_done, hipEventDisableTiming));
    if (ensure(&c->d_png, &c->d_png_bytes, need) != MVHP_SUCCESS) return MVHP_FAILURE;   // (hipFree waits for the device)
    if (c->png_stream && c->png_stream != st) HIP_TRY(hipStreamWaitEvent(st, c->png_done, 0));
    a.scratch = (uint8_t *)c->d_png;
    HIP_TRY(mvhp::launch_png_encode(a, st));
    HIP_TRY(hipEventRecord(c->png_done, st));
    c->png_stream = st;
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_recon_batch_host(mvhp_ctx_t *c, const mvhp_stream_params_t *p, const void *h_packed,
                                      int n_frames, uint8_t *h_yuv, uint8_t *h_rgb)
{
    if (!c || !params_ok(p) || !h_packed || !h_yuv || n_frames <= 0) {
        set_err("mvhp_recon_batch_host: invalid argument");
        return MVHP_FAILURE;
    }
    HIP_TRY(hipSetDevice(c->device));
    const size_t pb = mvhp_packed_frame_bytes(p) * n_frames;
    const size_t yb = mvhp_yuv_frame_bytes(p) * n_frames;
    const size_t rb = mvhp_rgb_frame_bytes(p) * n_frames;
    if (ensure(&c->d_packed, &c->d_packed_bytes, pb) != MVHP_SUCCESS) return MVHP_FAILURE;
    if (ensure((void **)&c->d_yuv, &c->d_yuv_bytes, yb) != MVHP_SUCCESS) return MVHP_FAILURE;
    if (h_rgb && ensure((void **)&c->d_rgb, &c->d_rgb_bytes, rb) != MVHP_SUCCESS) return MVHP_FAILURE;
    HIP_TRY(hipMemsetAsync(c->d_err, 0, sizeof(uint32_t), c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_packed, h_packed, pb, hipMemcpyHostToDevice, c->stream));
    int rc = launch_all(c, p, c->d_packed, n_frames, c->d_yuv, h_rgb ? c->d_rgb : nullptr, c->stream, true, true,
                        (p->flags & MVHP_PARAM_DEBLOCK) != 0);
    if (rc != MVHP_SUCCESS) return rc;
    HIP_TRY(hipMemcpyAsync(h_yuv, c->d_yuv, yb, hipMemcpyDeviceToHost, c->stream));
    if (h_rgb) HIP_TRY(hipMemcpyAsync(h_rgb, c->d_rgb, rb, hipMemcpyDeviceToHost, c->stream));
    std::string err;
    HIP_TRY(read_err_word(c, c->stream, true, err));
    if (!err.empty()) {
        set_err("%s", err.c_str());
        return MVHP_FAILURE;
    }
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_sync_check(mvhp_ctx_t *c, void *stream)
{
    if (!c) return MVHP_FAILURE;
    HIP_TRY(hipSetDevice(c->device));
    std::string err;
    HIP_TRY(read_err_word(c, stream_of(c, stream), true, err));
    if (!err.empty()) {
        set_err("%s", err.c_str());
        hipMemset(c->d_err, 0, sizeof(uint32_t));
        return MVHP_FAILURE;
    }
    return MVHP_SUCCESS;
}

/* Test hook (tests/test_gpu_wide.py): the next wide launch of `c` hands out its units `delta` off, i.e. one unit is never
 * reconstructed and one ticket falls outside the launch -- what a corrupted ticket counter would look like.  The launch must END
 * (bounded waits) with the error word set, and mvhp_sync_check() must say so. */
MVHP_EXPORT int mvhp_debug_skew_next_ticket_base(mvhp_ctx_t *c, int delta)
{
    if (!c) return MVHP_FAILURE;
    c->ticket_skew_once = delta;
    return MVHP_SUCCESS;
}

// Every launch issued on the context has run: the last banded one (it may be on a caller's stream) and the context's own stream.
static int wide_drain(mvhp_ctx *c)
{
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->wide_done));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MVHP_SUCCESS;
}

/* Test hook (tests/test_gpu_wide_wrap.py): puts the ticket counter and the epoch tag where 2^32 tickets / launches would have
 * taken them, so that a CORRECT launch runs across a wraparound.  The seams keep the tags of earlier launches: discarding them
 * is wide_prepare()'s business. */
MVHP_EXPORT int mvhp_debug_set_wide_state(mvhp_ctx_t *c, uint32_t ticket, uint32_t epoch)
{
    if (!c) return MVHP_FAILURE;
    if (wide_drain(c) != MVHP_SUCCESS) return MVHP_FAILURE;
    HIP_TRY(hipMemcpy(c->d_ticket, &ticket, sizeof(ticket), hipMemcpyHostToDevice));
    c->ticket_base = ticket;
    c->wide_epoch = epoch;
    return MVHP_SUCCESS;
}

/* Test hook (tests/test_gpu_wide_wrap.py): the counter on the device beside the host's bookkeeping of it. */
MVHP_EXPORT int mvhp_debug_get_wide_state(mvhp_ctx_t *c, uint32_t *device_ticket, uint32_t *ticket_base, uint32_t *epoch,
                                          size_t *seam_bytes)
{
    if (!c) return MVHP_FAILURE;
    if (wide_drain(c) != MVHP_SUCCESS) return MVHP_FAILURE;
    if (device_ticket) HIP_TRY(hipMemcpy(device_ticket, c->d_ticket, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (ticket_base) *ticket_base = c->ticket_base;
    if (epoch) *epoch = c->wide_epoch;
    if (seam_bytes) *seam_bytes = c->d_seam_bytes;
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_plan_launch(const mvhp_ctx_t *c, const mvhp_plan_device_t *d, const mvhp_stream_params_t *p, int n_frames,
                                 int *layout, int *waves)
{
    if ((c != nullptr) == (d != nullptr) || !params_ok(p) || n_frames <= 0) return MVHP_FAILURE;
    if (d && (d->n_cus <= 0 || d->layout < MVHP_LAYOUT_AUTO || d->layout >= MVHP_LAYOUT_COUNT)) return MVHP_FAILURE;
    const mvhp::PlanDevice dev = c ? plan_device(c) : mvhp::PlanDevice{d->n_cus, (size_t)d->max_lds_bytes, d->layout, d->waves};
    const mvhp::LaunchPlan plan = mvhp::plan_launch(dev, *p, n_frames);
    if (layout) *layout = plan.layout;
    if (waves) *waves = plan.waves;
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_last_launch_info(const mvhp_ctx_t *c, int *layout, int *waves)
{
    if (!c) return MVHP_FAILURE;
    if (layout) *layout = c->last_layout;
    if (waves) *waves = c->last_waves;
    return MVHP_SUCCESS;
}

} // extern "C"

// ---------------------------------------------------------------------------------------------------------------
// The decode engine's device table (csrc/host/decode_engine.h): every operation runs on its own HIP stream of the
// context and blocks the calling engine thread until the device has finished it; durations come from HIP events
// recorded on that stream.
// ---------------------------------------------------------------------------------------------------------------
namespace mvengine {
struct DevCtx {
    mvhp_ctx   *c = nullptr;
    hipStream_t up = nullptr, down = nullptr;
    hipEvent_t  ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // begin/end per queue: upload, compute, download
};
} // namespace mvengine

namespace {

using mvengine::DevCtx;

#define ENG_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) {                                                                           \
            err = std::string(#expr) + " failed: " + hipGetErrorString(e_);                               \
            return MVHP_FAILURE;                                                                          \
        }                                                                                                 \
    } while (0)

DevCtx *eng_ctx_create(int device, std::string &err)
{
    mvhp_ctx_t *c = nullptr;
    if (mvhp_create(device, &c) != MVHP_SUCCESS) { err = mvhp_last_error(); return nullptr; }
    DevCtx *d = new DevCtx();
    d->c = c;
    bool ok = hipStreamCreateWithFlags(&d->up, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&d->down, hipStreamNonBlocking) == hipSuccess;
    // blocking-sync events: the engine's copy / launch threads sleep in hipEventSynchronize instead of spinning on a core
    // the entropy threads could use
    for (int i = 0; i < 6 && ok; i++) ok = hipEventCreateWithFlags(&d->ev[i], hipEventBlockingSync) == hipSuccess;
    if (!ok) {
        err = "stream / event creation failed on device " + std::to_string(device);
        for (int i = 0; i < 6; i++) if (d->ev[i]) hipEventDestroy(d->ev[i]);
        if (d->up) hipStreamDestroy(d->up);
        if (d->down) hipStreamDestroy(d->down);
        mvhp_destroy(c);
        delete d;
        return nullptr;
    }
    return d;
}

void eng_ctx_destroy(DevCtx *d)
{
    if (!d) return;
    hipSetDevice(d->c->device);
    hipStreamSynchronize(d->up);
    hipStreamSynchronize(d->down);
    for (int i = 0; i < 6; i++) hipEventDestroy(d->ev[i]);
    hipStreamDestroy(d->up);
    hipStreamDestroy(d->down);
    mvhp_destroy(d->c);
    delete d;
}

void *eng_dev_alloc(DevCtx *d, size_t bytes)
{
    void *p = nullptr;
    if (hipSetDevice(d->c->device) != hipSuccess || hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    return p;
}

void eng_dev_free(DevCtx *d, void *p)
{
    hipSetDevice(d->c->device);
    (void)hipFree(p);
}

size_t eng_dev_free_bytes(DevCtx *d)
{
    size_t fr = 0, tot = 0;
    if (hipSetDevice(d->c->device) != hipSuccess || hipMemGetInfo(&fr, &tot) != hipSuccess) return 0;
    return fr;
}

// n copies on the queue `st`, bracketed by its two events; returns when the last one is done
int eng_copy_all(DevCtx *d, hipStream_t st, hipEvent_t e0, hipEvent_t e1, hipMemcpyKind kind, int n, void *const *dst,
                 const void *const *src, const size_t *bytes, float *ms, std::string &err)
{
    ENG_TRY(hipSetDevice(d->c->device));
    ENG_TRY(hipEventRecord(e0, st));
    for (int i = 0; i < n; i++)
        if (bytes[i]) ENG_TRY(hipMemcpyAsync(dst[i], src[i], bytes[i], kind, st));
    ENG_TRY(hipEventRecord(e1, st));
    ENG_TRY(hipEventSynchronize(e1));
    if (ms) ENG_TRY(hipEventElapsedTime(ms, e0, e1));
    return MVHP_SUCCESS;
}

int eng_h2d(DevCtx *d, int n, void *const *dst, const void *const *src, const size_t *bytes, float *ms, std::string &err)
{
    return eng_copy_all(d, d->up, d->ev[0], d->ev[1], hipMemcpyHostToDevice, n, dst, src, bytes, ms, err);
}

int eng_d2h(DevCtx *d, int n, void *const *dst, const void *const *src, const size_t *bytes, float *ms, std::string &err)
{
    return eng_copy_all(d, d->down, d->ev[4], d->ev[5], hipMemcpyDeviceToHost, n, dst, src, bytes, ms, err);
}

// One batch, on the context's stream inside one pair of events: expand, reconstruction (planes only when a resample pass or the
// encoder follows, otherwise with fused RGB into d_rgb), the resample pass, the turn, the encoder, the picture scores; then one wait and one
// read of the error word.  (When the word is set the scores of that batch have been computed already: nothing reads them.)
int eng_run_batch(DevCtx *d, const mvengine::BatchJob &j, mvengine::BatchDone &done, std::string &err)
{
    mvhp_ctx *c = d->c;
    const mvhp_stream_params_t *p = j.params;
    const bool resample = j.out_yuv || j.out_rgb;   // (a pass behind the reconstruction writes them: the resample pass, the turn, or both)
    if (j.turns < 0 || j.turns > 3 || (j.turns == 0 && j.mid_yuv) || (j.turns && !resample)) { err = "reconstruction: invalid orientation"; return MVHP_FAILURE; }
    if (!params_ok(p) || !j.d_compact || !j.d_packed || !j.d_yuv || j.n <= 0) { err = "reconstruction: invalid argument"; return MVHP_FAILURE; }
    if ((resample || j.jpeg || j.png) && !j.geom) { err = "reconstruction: no output geometry"; return MVHP_FAILURE; }
    if (j.jpeg && (!j.blob || !j.table || j.out_rgb)) { err = "reconstruction: invalid JPEG output"; return MVHP_FAILURE; }
    if (j.png && (j.jpeg || !j.blob || !j.table || !(resample ? j.out_rgb : j.d_rgb))) { err = "reconstruction: invalid PNG output"; return MVHP_FAILURE; }
    if (j.geom && !resample && !j.jpeg && !j.png && !j.color) { err = "reconstruction: an output geometry without an output buffer"; return MVHP_FAILURE; }
    // colour pass: RGB from the final planes -- out_yuv -> out_rgb behind a pass, else d_yuv -> d_rgb at the coded size
    if (j.color && (j.jpeg || !j.geom || (resample ? (!j.out_yuv || !j.out_rgb) : !j.d_rgb))) { err = "reconstruction: invalid colour pass"; return MVHP_FAILURE; }
    // tensors: from the RGB the job makes -- out_rgb behind a pass, else d_rgb of the coded size
    if (j.tensor && (j.jpeg || j.png || j.bars || !j.tensor_out || !(resample ? j.out_rgb : j.d_rgb) || (j.slots_host && !j.d_slots))) { err = "reconstruction: invalid tensor output"; return MVHP_FAILURE; }
    ENG_TRY(hipSetDevice(c->device));
    ENG_TRY(hipEventRecord(d->ev[2], c->stream));
    if (mvhp_expand_compact_dev(c, p, j.d_compact, j.stride, j.n, j.d_packed, c->stream) != MVHP_SUCCESS) { err = mvhp_last_error(); return MVHP_FAILURE; }
    const bool deblock = (p->flags & MVHP_PARAM_DEBLOCK) != 0;
    int rc = (resample || j.jpeg || j.color) ? launch_all(c, p, j.d_packed, j.n, j.d_yuv, nullptr, c->stream, true, false, deblock)
                                  : launch_all(c, p, j.d_packed, j.n, j.d_yuv, j.d_rgb, c->stream, true, true, deblock);
    uint8_t *const pass_rgb = j.color ? nullptr : j.out_rgb;   // (with a colour pass the passes below make planes only)
    if (rc == MVHP_SUCCESS && resample && !j.turns) rc = mvhp_resample_dev(c, p, j.geom, j.d_yuv, j.n, j.out_yuv, pass_rgb, c->stream);
    if (rc == MVHP_SUCCESS && j.turns) {   // the geometry before the turn; planes of it first where the box scales
        mvhp_output_geometry_t g0 = *j.geom;
        if (j.turns & 1) std::swap(g0.out_w, g0.out_h);
        if (j.mid_yuv) rc = mvhp_resample_dev(c, p, &g0, j.d_yuv, j.n, j.mid_yuv, nullptr, c->stream);
        if (rc == MVHP_SUCCESS)
            rc = mvhp_orient_dev(c, p, &g0, j.turns, j.mid_yuv ? 0u : MVHP_ORIENT_SRC_CODED, j.mid_yuv ? j.mid_yuv : j.d_yuv, j.n,
                                 j.out_yuv, pass_rgb, c->stream);
    }
    if (rc == MVHP_SUCCESS && j.color)
        rc = mvhp_color_dev(c, j.geom, j.color, resample ? j.out_yuv : j.d_yuv, j.n, resample ? j.out_rgb : j.d_rgb, c->stream);
    if (rc == MVHP_SUCCESS && j.jpeg)
        rc = mvhp_jpeg_encode_dev(c, j.geom, j.jpeg, resample ? j.out_yuv : j.d_yuv, j.n, j.blob, j.blob_cap, j.table, c->stream);
    if (rc == MVHP_SUCCESS && j.png)
        rc = mvhp_png_encode_dev(c, j.geom, j.png, resample ? j.out_rgb : j.d_rgb, j.n, j.blob, j.blob_cap, j.table, c->stream);
    if (rc == MVHP_SUCCESS && j.tensor) {   // (the slot table rides the job's own queue, in front of the kernel that reads it; the
        // host copy stays where it is until the wait below)
        if (j.slots_host) ENG_TRY(hipMemcpyAsync(j.d_slots, j.slots_host, (size_t)j.n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        rc = mvhp_tensor_dev(c, j.tensor, resample ? j.out_rgb : j.d_rgb, j.n, j.tensor_out, j.slots_host ? j.d_slots : nullptr, c->stream);
    }
    if (rc == MVHP_SUCCESS && j.stats) {
        mvhp_output_geometry_t whole{};   // (no geometry: the rectangle is the coded picture)
        whole.crop_w = whole.out_w = p->width_mbs * 16;
        whole.crop_h = whole.out_h = p->height_mbs * 16;
        rc = mvhp_luma_stats_dev(c, p, j.geom ? j.geom : &whole, j.d_yuv, j.n, j.stats, c->stream);
    }
    if (rc == MVHP_SUCCESS && j.bars) {
        mvhp_output_geometry_t whole{};
        whole.crop_w = whole.out_w = p->width_mbs * 16;
        whole.crop_h = whole.out_h = p->height_mbs * 16;
        rc = mvhp_luma_bars_dev(c, p, j.geom ? j.geom : &whole, j.d_yuv, j.n, j.bars_level, j.bars, c->stream);
    }
    if (rc == MVHP_SUCCESS && j.hist) {
        mvhp_output_geometry_t whole{};
        whole.crop_w = whole.out_w = p->width_mbs * 16;
        whole.crop_h = whole.out_h = p->height_mbs * 16;
        rc = mvhp_plane_hist_dev(c, p, j.geom ? j.geom : &whole, j.d_yuv, j.n, j.hist, c->stream);
    }
    if (rc != MVHP_SUCCESS) { err = mvhp_last_error(); return rc; }
    ENG_TRY(hipEventRecord(d->ev[3], c->stream));
    std::string ew;
    ENG_TRY(hipEventSynchronize(d->ev[3]));   // (sleeps: blocking-sync event)
    ENG_TRY(read_err_word(c, c->stream, false, ew));
    ENG_TRY(hipEventElapsedTime(&done.ms, d->ev[2], d->ev[3]));
    done.layout = c->last_layout;
    done.waves = c->last_waves;
    if (!ew.empty()) {
        (void)hipMemsetAsync(c->d_err, 0, sizeof(uint32_t), c->stream);
        err = ew;
        return MVHP_FAILURE;
    }
    return MVHP_SUCCESS;
}

// the engine's batch buffers from one placed arena (MINIVIDEO_PLACED=1): records / planes / RGB of a batch in three groups of
// the device's memory regions (placement.hip); the compact staging area goes wherever room is left
void *eng_placed_alloc(DevCtx *d, int sets, const size_t bytes[4], void **ptrs)
{
    static const uint8_t any_group[4] = {1, 0, 0, 0};   // {compact, records, planes, RGB}
    void *arena = nullptr;
    int found = 0;
    // an arena sized from the need, not "everything that is free": twice the buffers (room to choose blocks of the
    // right group) + 16 GB, inside the library's cap -- what the device keeps free stays available to ordinary allocations
    // (another picture shape, a second context on the device)
    const size_t blk = (size_t)4 << 30;   // (placement.hip hands out runs of 4-GB blocks)
    size_t need = 0;
    for (int i = 0; i < 4; i++) need += (bytes[i] + blk - 1) / blk * blk;
    need *= (size_t)sets;
    size_t want = need + need / 2 + ((size_t)16 << 30);
    size_t cap = (size_t)200 << 30;
    if (const char *e = getenv("MVHP_PLACED_ARENA_GB")) { const long gb = atol(e); if (gb >= 8 && gb <= 256) cap = (size_t)gb << 30; }
    size_t fr = 0, tot = 0;
    if (hipSetDevice(d->c->device) == hipSuccess && hipMemGetInfo(&fr, &tot) == hipSuccess) {
        const size_t reserve = (size_t)24 << 30;
        cap = std::min(cap, fr > reserve ? fr - reserve : (size_t)0);
    }
    want = std::min(want, cap);
    if (want < need) return nullptr;
    if (mvhp_placed_alloc_sets(d->c->device, sets, 4, bytes, any_group, want, ptrs, &arena, nullptr, &found) != MVHP_SUCCESS) return nullptr;
    return arena;
}

void eng_placed_free(DevCtx *d, void *arena)
{
    (void)d;
    mvhp_placed_free(arena);
}

const mvengine::DeviceApi g_hip_api = {
    mvhp_device_count, mvhp_host_alloc, mvhp_host_free, eng_ctx_create, eng_ctx_destroy, eng_dev_alloc, eng_dev_free,
    eng_dev_free_bytes, eng_h2d, eng_d2h, eng_run_batch, mvengine::CAP_GEOMETRY | mvengine::CAP_JPEG | mvengine::CAP_SCORE | mvengine::CAP_ORIENT | mvengine::CAP_COLOR | mvengine::CAP_PNG | mvengine::CAP_BARS | mvengine::CAP_HIST | mvengine::CAP_TENSOR,
    eng_placed_alloc, eng_placed_free,
};

} // namespace

const mvengine::DeviceApi &mvhp_hip_device_api() { return g_hip_api; }
