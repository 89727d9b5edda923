// decode_engine.cpp -- see decode_engine.h.
//
// Threads of one decode call (all joined before it returns):
//   feeder              hands out pictures in `order`, never more than `wanted` minus what is already accepted or in
//                       flight (the reference stops after picture_number IDRs, h264.c:173-179), grouped into chunks
//                       (one H2D transfer) and batches (one kernel launch, one set of stream parameters, one output
//                       geometry);
//   T entropy workers   mvhp_stream::decode_compact() straight into a page-locked chunk slot (the compact transfer
//                       format: only non-zero levels cross PCIe; the GPU expands it into packed records);
//   per context:        uploader (claims whole batches from the shared queue: pictures are independent, so this is
//                       the frame-level work queue of SURVEY 8e -- no collective), launcher, downloader;
//   caller thread       calls the sink once per picture, in order.
// One mutex + one condition variable guard all queues; the heavy work (entropy decode, copies, kernels, sink) runs
// outside the lock.
#include "decode_engine.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "blank_policy.h"
#include "h264_frontend.h"
#include "png_format.h"
#include "stream_internal.h"
#include "tensor_policy.h"

namespace mvengine {

namespace {

double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    return atoi(e);
}

} // namespace

// Host cores this process may actually use: the hardware thread count, cut down to the CPU-time quota of the
// container (cgroup v2 cpu.max / v1 cfs quota) -- a box of 256 hardware threads often grants 16 CPUs per GPU, and
// 256 entropy threads sharing 16 CPUs only thrash.
int effective_cores()
{
    int n = (int)std::thread::hardware_concurrency();
    if (n < 1) n = 1;
    long quota = -1, period = -1;
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32] = "";
        if (fscanf(f, "%31s %ld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atol(q);
        fclose(f);
    } else {
        if (FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(g, "%ld", &quota) != 1) quota = -1; fclose(g); }
        if (FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(g, "%ld", &period) != 1) period = -1; fclose(g); }
    }
    if (quota > 0 && period > 0) n = std::min<long>(n, std::max<long>(1, (quota + period - 1) / period));
    return n;
}

namespace {

bool same_params(const mvhp_stream_params_t &a, const mvhp_stream_params_t &b)
{
    return a.width_mbs == b.width_mbs && a.height_mbs == b.height_mbs &&
           a.chroma_qp_index_offset == b.chroma_qp_index_offset &&
           a.second_chroma_qp_index_offset == b.second_chroma_qp_index_offset && a.flags == b.flags &&
           (!(a.flags & MVHP_PARAM_SCALING) ||
            (memcmp(a.scaling4, b.scaling4, sizeof(a.scaling4)) == 0 && memcmp(a.scaling8, b.scaling8, sizeof(a.scaling8)) == 0));
}

bool same_color(const mvhp_color_params_t &a, const mvhp_color_params_t &b)
{
    return a.matrix == b.matrix && a.full_range == b.full_range && a.siting == b.siting;
}

bool same_geometry(const mvhp_output_geometry_t &a, const mvhp_output_geometry_t &b)
{
    return a.crop_x == b.crop_x && a.crop_y == b.crop_y && a.crop_w == b.crop_w && a.crop_h == b.crop_h && a.out_w == b.out_w &&
           a.out_h == b.out_h;
}

// the geometry of a picture delivered at its coded size
mvhp_output_geometry_t coded_geometry(const mvhp_stream_params_t &p)
{
    mvhp_output_geometry_t g{};
    g.crop_w = g.out_w = p.width_mbs * 16;
    g.crop_h = g.out_h = p.height_mbs * 16;
    return g;
}

struct Pinned {
    uint8_t *p = nullptr;
    size_t cap = 0;
};

struct InChunk {
    Pinned buf;              // n slots of pic_bytes: one compact picture each (include/minivideo_hotpath.h)
    int batch = -1;
    int first_slot = 0;      // picture offset inside the batch
    int n = 0;               // pictures in this chunk
    size_t pic_bytes = 0;    // slot size = the most a compact picture of these parameters can take
    std::vector<size_t> used;// bytes of each slot actually written
    int remaining = 0;       // pictures not yet entropy-decoded (guarded by the engine mutex)
};

struct OutChunk {
    Pinned yuv, rgb;         // (MVHP_OUT_JPEG, MVHP_OUT_PNG: rgb holds the files of the chunk's pictures, tab their table entries)
    Pinned tab;
    Pinned stats;            // (MVHP_OUTPUT_SCORE: the records of the chunk's pictures)
    Pinned hist;             // (MVHP_OUTPUT_HIST: the histograms of the chunk's pictures)
    int refs = 0;            // pictures handed to the sink queue and not yet consumed
};

struct PicResult {
    int idr = -1;
    int rc = MVHP_FAILURE;
    std::string err;
    mvhp_stream_params_t params{};
    mvhp_output_geometry_t geom{};   // what yuv / rgb hold (the coded size unless the call has an output request)
    OutChunk *oc = nullptr;
    const uint8_t *yuv = nullptr, *rgb = nullptr;
    const mvhp_plane_hist_t *hist = nullptr;   // MVHP_OUTPUT_HIST: the picture's record in `oc` (picture_hist())
    bool ready = false;      // final: the sink may take it
    bool parsed_ok = false;
    bool kept = false;       // the sink answered 2: its output chunk stays referenced until release_picture()
};

// The device buffers of a batch, one per kind.  The first four are what reconstruction itself needs and may be pieces of a placed
// arena; the others are ordinary allocations always, also beside an arena: they are the small side of a batch that has them.
enum BufKind {
    kCompact,    // uploaded compact pictures, slot stride as in the chunks
    kPacked,     // the records they expand to
    kYuv,        // planes of the coded size: the output, or the input of the passes behind reconstruction
    kRgb,        // fused RGB of the coded size
    kOutYuv,     // output pictures of a batch with a geometry (what is downloaded then)
    kOutRgb,
    kMidYuv,     // a batch that scales AND turns: the resampled planes before the turn (the turn reads them, nothing downloads them)
    kJpegBlob,   // MVHP_OUT_JPEG: the encoder's blob (n x the raw picture); MVHP_OUT_PNG: n x the longest file ...
    kJpegTab,    // ... and table of a batch
    kStats,      // MVHP_OUTPUT_SCORE or MVHP_OUTPUT_BARS (never both): the records of a batch (n x 32 bytes)
    kHist,       // MVHP_OUTPUT_HIST: the plane histograms of a batch (n x 3104 bytes)
    kTensor,     // MVHP_OUT_TENSOR, host delivery: the tensors of a batch (what is downloaded then)
    kSlots,      // MVHP_OUT_TENSOR, device delivery: the slot numbers of a batch (n x 4 bytes; the tensors go to the caller's memory)
    kBufKinds,
    kArenaKinds = kOutYuv,
};

struct DevBuf {
    struct { uint8_t *p = nullptr; size_t cap = 0; } m[kBufKinds];
    bool busy = false;
    bool arena_piece = false;   // the first four buffers are pieces of the context's placed arena: never freed one by one
    void leave_arena()          // the four arena pieces are forgotten (they go with the arena); the output buffers stay
    {
        for (int k = 0; k < kArenaKinds; k++) m[k] = {};
        arena_piece = false;
    }
};

// slot size of a compact picture: the format's upper bound, 16-byte aligned
size_t compact_slot_bytes(const mvhp_stream_params_t &p)
{
    const size_t mbs = (size_t)p.width_mbs * p.height_mbs;
    return (mbs * MVHP_COMPACT_MB_BYTES_MAX + MVHP_COMPACT_SLACK_BYTES + 15) & ~(size_t)15;
}

// a valid compact picture without a single level (every offset points at one empty Intra4x4 record): what a slot holds
// when its picture failed to parse, so that the batch can still be expanded
size_t write_empty_compact(uint8_t *buf, size_t mbs)
{
    memset(buf, 0, mbs * 4 + MVHP_MB_HEADER_BYTES);
    return mbs * 4 + MVHP_MB_HEADER_BYTES;
}

// which outputs a call delivers
struct Wants {
    bool yuv = true, rgb = false;   // which of them are downloaded (the planes are always reconstructed)
    bool jpeg = false;              // MVHP_OUT_JPEG: neither of them; JPEG files made on the device
    bool png = false;               // MVHP_OUT_PNG: neither of them; PNG files made on the device from the RGB
    bool score = false;             // MVHP_OUTPUT_SCORE (it changes no picture and no path)
    int turns = 0;                  // quarter turns the request applies (mvhp_output_turns): one value per call
    bool color = false;             // MVHP_OUTPUT_COLOR in a call that delivers RGB or PNG: the RGB comes from a colour pass over the
                                    // final planes (which a batch with a geometry then keeps, whether or not they are downloaded)
    bool bars = false;              // MVHP_OUTPUT_BARS (it changes no picture and no path; never beside score, jpeg or png)
    int bars_level = MVHP_BARS_LEVEL_DEFAULT;
    bool hist = false;              // MVHP_OUTPUT_HIST (it changes no picture and no path; never beside bars)
    bool tensor = false;            // MVHP_OUT_TENSOR: the RGB is made as for `rgb` alone (which is set) and packed into tensors of
    mvhp_tensor_request_t treq{};   // this request; only those are delivered.  Never beside jpeg, png or bars
};
// the tensor of a picture of the delivered geometry g under a call's request
mvhp_tensor_params_t tensor_params(const Wants &w, const mvhp_output_geometry_t &g) { return mvtensor::of_request(w.treq, g.out_w, g.out_h); }
// whether a batch of the DELIVERED geometry g, turned by `turns`, has a resample pass in front of the turn
bool scales_before_turn(const mvhp_output_geometry_t &g, int turns)
{
    const uint32_t w = (turns & 1) ? g.out_h : g.out_w, h = (turns & 1) ? g.out_w : g.out_h;
    return turns != 0 && (w != g.crop_w || h != g.crop_h);
}
// what a placed arena and the job's largest batch are planned for: pictures of the coded size, planes and RGB
constexpr Wants kPlanesAndRgb = {true, true, false, false, false, 0, false};

// MVHP_OUT_PNG: the room of one picture in the blob -- the longest file there is (every segment stored), so that no picture can be
// too big, rounded to the 16 bytes files are placed at
size_t png_blob_bytes(const mvhp_output_geometry_t &g)
{
    return (mvhp::png_max_bytes((int)g.out_w, (int)g.out_h) + 15) & ~(size_t)15;
}

// Device bytes per picture of one kind, for a batch of these parameters and this geometry (use_geom: it differs from the coded
// size) in a call with these outputs; 0 = such a batch has no buffer of the kind.  The only place where the size of a batch
// buffer is written: the allocations, the memory budget, the launch and the download all read it.
size_t picture_bytes(BufKind k, const mvhp_stream_params_t &p, const mvhp_output_geometry_t &g, bool use_geom, const Wants &w)
{
    switch (k) {
    case kCompact:  return compact_slot_bytes(p);
    case kPacked:   return mvhp_packed_frame_bytes(&p);
    case kYuv:      return mvhp_yuv_frame_bytes(&p);
    case kRgb:      return (w.rgb || w.png) && !use_geom ? mvhp_rgb_frame_bytes(&p) : 0;
    case kOutYuv:   return use_geom && (w.yuv || w.jpeg || w.color) ? mvhp_geometry_yuv_bytes(&g) : 0;   // (the colour pass reads them)
    case kOutRgb:   return use_geom && (w.rgb || w.png) ? mvhp_geometry_rgb_bytes(&g) : 0;
    case kMidYuv:   return use_geom && scales_before_turn(g, w.turns) ? mvhp_geometry_yuv_bytes(&g) : 0;
    case kJpegBlob: return w.jpeg ? mvhp_geometry_yuv_bytes(&g) : w.png ? png_blob_bytes(g) : 0;
    case kJpegTab:  return w.jpeg || w.png ? sizeof(mvhp_jpeg_entry_t) : 0;
    case kStats:    return w.score ? sizeof(mvhp_luma_stats_t) : w.bars ? sizeof(mvhp_luma_bars_t) : 0;
    case kHist:     return w.hist ? sizeof(mvhp_plane_hist_t) : 0;
    case kTensor:   return w.tensor && !w.treq.d_target ? mvtensor::bytes(tensor_params(w, g)) : 0;
    case kSlots:    return w.tensor && w.treq.d_target ? sizeof(int32_t) : 0;
    default:        return 0;
    }
}

// all of them, and the one term that is no batch buffer: the JPEG encoder's scratch, which lives in the context.  136 bytes per
// 8x8 block = 2.125 x the planes padded to whole MCUs; with the blob, 1 x the planes, that is 3.125 x, budgeted as 4.25 x for
// that padding on small pictures -- the scratch's share is what the blob and the table entry leave of it
size_t batch_picture_bytes(const mvhp_stream_params_t &p, const mvhp_output_geometry_t &g, bool use_geom, const Wants &w)
{
    size_t sum = 0;
    for (int k = 0; k < kBufKinds; k++) sum += picture_bytes((BufKind)k, p, g, use_geom, w);
    if (w.jpeg) sum += mvhp_geometry_yuv_bytes(&g) * 17 / 4 - mvhp_geometry_yuv_bytes(&g) - sizeof(mvhp_jpeg_entry_t);
    // (the PNG encoder's scratch: one byte per row, 304 per segment -- and a segment has at least one row)
    if (w.png && g.out_w) {
        const size_t R = (size_t)mvhp::png_segment_rows((int)g.out_w);
        sum += (size_t)g.out_h + 304 * (((size_t)g.out_h + R - 1) / R) + 16;
    }
    return sum;
}

// where the pictures of a batch are downloaded from: the resample targets of a batch with a geometry, else the coded size
BufKind planes_kind(bool use_geom) { return use_geom ? kOutYuv : kYuv; }
BufKind rgb_kind(bool use_geom) { return use_geom ? kOutRgb : kRgb; }

struct Batch {
    int id = 0;
    mvhp_stream_params_t params{};
    mvhp_output_geometry_t geom{};   // of every picture of the batch
    bool use_geom = false;           // geom differs from the coded size: the batch has a resample pass
    mvhp_color_params_t color{};     // MVHP_OUTPUT_COLOR: the resolved setting of every picture of the batch
    std::vector<int> seqs;           // slot -> position in `order`
    int capacity = 0;                // planned pictures (device buffers are sized for it)
    int total = -1;                  // pictures, known once the closing chunk has been issued
    int uploaded = 0;
    int ctx = -1;                    // claimed by this context
    int exclude_ctx = -1;            // a re-queued batch does not go back to the context it failed on
    bool retry = false;
    bool dead = false;
    std::string dead_why;
    DevBuf *buf = nullptr;
    std::deque<InChunk *> ready;     // entropy-decoded chunks waiting for upload
    double t_open = 0, t_claim = 0, t_closed = 0, t_uploaded = 0, t_kernel = 0;   // MINIVIDEO_ENGINE_TRACE (seconds into the call)
};

struct Item {
    InChunk *chunk;
    int slot;   // inside the chunk
    int seq;
};

struct RetryGroup {
    std::vector<int> seqs;
    int exclude_ctx = -1;
    size_t pos = 0;
};

constexpr int kMaxDevBufs = 8;

struct Ctx {
    DevCtx *dev = nullptr;
    int device = 0;
    DevBuf bufs[kMaxDevBufs];   // n_bufs of them in use.  Three batches per context is the minimum: one filling / uploading, one in
                      // the kernel, one downloading -- with two, the batch after next could not be claimed until a download finished
                      // and the entropy threads ran out of chunk slots (170 pictures took 90 ms instead of 44 to fill in the taper of
                      // a 2048-picture job).  More (MINIVIDEO_DEVBUFS = 4...8) were measured in round 3: no gain (tools/e2e_devbufs_sweep.sh)
    int n_bufs = 3;
    int open_batch = -1;
    std::deque<int> to_launch, to_download;
    bool fail_next = false;
    bool launched_once = false;   // (over the engine's life: the code objects stay loaded)
    void *arena = nullptr;        // MINIVIDEO_PLACED=1: the three batch buffers live in one placed arena ...
    int arena_pictures = 0;       // ... sized for this many pictures per batch ...
    mvhp_stream_params_t arena_params{};   // ... of this shape
    bool arena_tried = false;
    size_t mem_budget = 0;   // bytes one batch may occupy on the device
};

} // namespace

class Engine {
public:
    Engine(const DeviceApi &api) : api_(api) {}
    ~Engine();
    bool init(const mvhp_engine_opts_t *opts, std::string &err);
    int decode(const mvhp_stream &s, const int *order, int n_order, int wanted, int out_mask, const mvhp_output_request_t *req,
               mvhp_picture_sink_t sink, mvhp_picture_sink_ex_t sink_ex, void *user, mvhp_decode_stats_t *stats, std::string &err);

private:
    // ---- threads ----
    void feeder();
    void worker(int t);
    void uploader(int k);
    void launcher(int k);
    void downloader(int k);
    // ---- helpers (mutex held unless noted) ----
    int allowance() const { return wanted_ - ok_ - (issued_ - consumed_); }
    bool pick_chunk(int k, InChunk **c, Batch **b);
    void fail_batch(Batch *b, const std::string &why);
    void close_batch(Batch *b);
    void release_batch(Batch *b);
    void put_out(OutChunk *oc);
public:
    void release_picture(int seq);   // any thread
    const mvhp_plane_hist_t *picture_hist(int seq);   // any thread
    int set_tensor(const mvhp_tensor_request_t *t, std::string &err);   // between decode calls
    int contexts() const { return (int)ctx_.size(); }
private:
    bool tensor_fits(int seq, const mvhp_output_geometry_t &g, std::string &why);   // MVHP_OUT_TENSOR: may picture `seq` be issued
    bool grow(Pinned &p, size_t need);   // no lock needed
    int launch_cap(size_t per_picture) const;
    int batch_capacity(const mvhp_stream_params_t &p, const mvhp_output_geometry_t &g, bool use_geom, int remaining) const;
    size_t need(const Batch &b, BufKind k) const { return picture_bytes(k, b.params, b.geom, b.use_geom, w_); }   // per picture; 0: not needed
    bool picture_geometry(int idr, const mvhp_stream_params_t &p, mvhp_output_geometry_t &g, bool &use, std::string &why) const;
    int planned_batch(int cap, int remaining, int batch_id) const;
    int chunk_pictures(const mvhp_stream_params_t &p) const;
    bool grow_dev(Ctx &c, DevBuf &b, BufKind k, size_t bytes);                   // no lock needed
    bool ensure_devbuf(Ctx &c, DevBuf &b, const Batch &bt, std::string &err);   // no lock needed

    const DeviceApi &api_;
    mvhp_engine_opts_t opts_{};
    std::vector<Ctx> ctx_;
    int host_threads_ = 1;
    std::vector<std::unique_ptr<InChunk>> all_in_;
    std::vector<std::unique_ptr<OutChunk>> all_out_;
    size_t in_limit_ = 4, out_limit_ = 4;

    // ---- state of the running decode call ----
    std::mutex mu_;
    std::condition_variable cv_;
    const mvhp_stream *s_ = nullptr;
    const int *order_ = nullptr;
    int n_order_ = 0, wanted_ = 0;
    Wants w_;                                   // (score: taken out of req_.flags)
    mvhp_jpeg_params_t jpeg_{};
    mvhp_png_params_t png_{};
    mvhp_tensor_request_t tensor_req_{};        // mvhp_engine_set_tensor: what the next MVHP_OUT_TENSOR call copies into w_ ...
    bool have_tensor_req_ = false;              // ... if there is one
    size_t tensor_slot_bytes_ = 0;   // device delivery: the size of the target's slots, the first issued picture's tensor (0: none yet)
    int color_mode_ = 0;             // MVHP_OUTPUT_COLOR_MODE of the call
    mvhp_color_params_t picture_color(int idr, const mvhp_stream_params_t &p, const mvhp_output_geometry_t &g) const;
    mvhp_output_request_t req_{};               // flags 0: pictures of the coded size
    bool stop_ = false;
    bool sink_waiting_ = false;
    int pos_ = 0;                 // next position of `order` the feeder has not issued yet
    int issued_ = 0, consumed_ = 0, ok_ = 0, failed_ = 0;
    int kept_ = 0;                // pictures a sink kept (verdict 2) and has not released yet
    int in_sink_ = -1;            // the picture whose sink callback is running
    bool released_early_ = false; // ... and was given back by another thread meanwhile
    int next_batch_id_ = 0;
    std::vector<PicResult> results_;
    std::map<int, std::unique_ptr<Batch>> batches_;
    std::deque<Item> work_q_;
    std::deque<RetryGroup> retry_q_;
    std::deque<InChunk *> free_in_;
    std::deque<OutChunk *> free_out_;
    mvhp_decode_stats_t st_{};
    std::vector<double> worker_busy_, worker_wait_;   // per entropy thread: inside decode_compact / waiting for work
    double feeder_wait_chunk_ = 0, t_last_entropy_ = 0, t_last_download_ = 0, t_start_ = 0;   // MINIVIDEO_ENGINE_TRACE
    std::atomic<uint64_t> stream_bytes_{0};
    // allocations of the running call (cold-start accounting; their own lock: grow() and ensure_devbuf() run unlocked)
    std::mutex alloc_mu_;
    double alloc_host_s_ = 0, alloc_dev_s_ = 0, first_launch_s_ = 0, first_picture_s_ = 0;
    uint64_t alloc_host_bytes_ = 0, alloc_dev_bytes_ = 0;
    bool placed_ = false;    // MINIVIDEO_PLACED=1 / opts.reserved[0] & 1
    int job_cap_ = 1;        // the largest batch the running call can form (per context)
    mvhp_stream_params_t job_params_{};   // ... of pictures of this size (the first picture's)
};

Engine::~Engine()
{
    for (auto &c : all_in_) api_.host_free(c->buf.p);
    for (auto &c : all_out_) { api_.host_free(c->yuv.p); api_.host_free(c->rgb.p); api_.host_free(c->tab.p); api_.host_free(c->stats.p); api_.host_free(c->hist.p); }
    for (Ctx &c : ctx_) {
        if (c.arena) {   // pieces of the arena go with it; a buffer that left the arena is freed below like any other
            for (DevBuf &b : c.bufs) if (b.arena_piece) b.leave_arena();
            api_.placed_free(c.dev, c.arena);
        }
        for (DevBuf &b : c.bufs)
            for (auto &m : b.m) if (m.p) api_.dev_free(c.dev, m.p);
        if (c.dev) api_.ctx_destroy(c.dev);
    }
}

bool Engine::init(const mvhp_engine_opts_t *opts, std::string &err)
{
    if (opts) opts_ = *opts;
    else opts_.fail_context = -1;
    const int n_dev = api_.device_count();
    if (n_dev <= 0) { err = "no HIP device available: this build has no CPU reconstruction path"; return false; }
    int n_ctx = opts_.contexts;
    if (n_ctx <= 0) {
        n_ctx = n_dev;
        const int cap = env_int("MINIVIDEO_GPUS", 0);
        if (cap > 0 && cap < n_ctx) n_ctx = cap;
        const int fake = env_int("MINIVIDEO_FAKE_GPUS", 0);   // several contexts on the devices there are (tests)
        if (fake > 0) n_ctx = fake;
    }
    if (n_ctx > 64) n_ctx = 64;
    host_threads_ = opts_.host_threads > 0 ? opts_.host_threads : env_int("MINIVIDEO_HOST_THREADS", 0);
    if (host_threads_ <= 0) host_threads_ = effective_cores();
    if (host_threads_ < 1) host_threads_ = 1;
    if (host_threads_ > 256) host_threads_ = 256;
    if (opts_.batch_pictures <= 0) opts_.batch_pictures = env_int("MINIVIDEO_BATCH", 0);
    if (opts_.fail_context < 0) opts_.fail_context = env_int("MINIVIDEO_TEST_FAIL_CONTEXT", -1);
    placed_ = (opts_.reserved[0] & 1) != 0 || env_int("MINIVIDEO_PLACED", 0) != 0;
    ctx_.resize((size_t)n_ctx);
    for (int k = 0; k < n_ctx; k++) {
        ctx_[k].device = (std::max(0, opts_.first_device) + k) % n_dev;
        ctx_[k].dev = api_.ctx_create(ctx_[k].device, err);
        if (!ctx_[k].dev) return false;
    }
    // device memory one batch may take: half of what is free now, split over the batch buffers (filling / in the kernel / downloading / waiting for the download) of every context
    // that shares the device
    for (int k = 0; k < n_ctx; k++) {
        int sharers = 0;
        for (int j = 0; j < n_ctx; j++) sharers += ctx_[j].device == ctx_[k].device;
        const size_t free_b = api_.dev_free_bytes(ctx_[k].dev);
        ctx_[k].n_bufs = std::max(3, std::min(kMaxDevBufs, env_int("MINIVIDEO_DEVBUFS", 3)));
        ctx_[k].mem_budget = free_b / 2 / (size_t)ctx_[k].n_bufs / (size_t)std::max(1, sharers);   // half of what is free, over the batch buffers
    }
    return true;
}

bool Engine::grow(Pinned &p, size_t need)
{
    if (need <= p.cap) return true;
    api_.host_free(p.p);
    const double t0 = now_s();
    p.p = (uint8_t *)api_.host_alloc(need);
    {
        std::lock_guard<std::mutex> l(alloc_mu_);
        alloc_host_s_ += now_s() - t0;
        alloc_host_bytes_ += need;
    }
    p.cap = p.p ? need : 0;
    return p.p != nullptr;
}

// pictures per transfer: ~64 MiB of records, so that a transfer runs at the link rate and a short job is not held up
int Engine::chunk_pictures(const mvhp_stream_params_t &p) const
{
    if (opts_.chunk_pictures > 0) return opts_.chunk_pictures;
    const size_t pb = std::max<size_t>(1, mvhp_packed_frame_bytes(&p));
    return (int)std::min<size_t>(64, std::max<size_t>(1, ((size_t)64 << 20) / pb));
}

// pictures per launch.  Speed only.  The batch kernels want 4 x CUs (four pictures per workgroup) or 8 x CUs (eight)
// pictures, but the host entropy stage is the slow side and the download of a batch (9.4 MB per 1080p picture) is
// next: what matters is that downloads start early and that the job's last download is short.  So batches RAMP UP from 64
// pictures, doubling, to the cap (the download of batch k hides behind the entropy work of batch k+1 as long as batches
// do not shrink faster than the link is quicker than the entropy stage), and TAPER at the end (each takes at most 35 %
// of what is left per context, down to one picture per entropy thread): 16 32 64 128 256 512 364 236 154 100 65 42 27 18 16 18
// for 2048 pictures on one context and 16 threads (round 2 started and ended on 64);
// long jobs run most of their pictures in 1024-picture launches.  Modelled wall for 2048 x 1080p: 0.56 s against 0.63 s
// with 1024 512 256 128 64 64 and 0.535 s of pure entropy work.
// The geometry of picture `idr` under the call's request.  use = it differs from the coded size (otherwise the picture takes
// the path of a call without a request: fused RGB, no extra pass, no extra buffers).  false: it cannot be formed (`why`).
bool Engine::picture_geometry(int idr, const mvhp_stream_params_t &p, mvhp_output_geometry_t &g, bool &use, std::string &why) const
{
    g = coded_geometry(p);
    use = false;
    if (req_.flags == 0) return true;
    if (mvhp_output_geometry(s_, idr, &req_, &g) != MVHP_SUCCESS) {
        const char *e = mvhp_stream_last_error();
        why = (e && *e) ? e : "the output geometry cannot be formed";
        g = mvhp_output_geometry_t{};
        return false;
    }
    use = w_.turns != 0 || !same_geometry(g, coded_geometry(p));   // (a turned picture of the coded size still has a pass)
    return true;
}

// The colour setting of picture `idr` under MVHP_OUTPUT_COLOR (all zero without it): what the stream says under the call's mode;
// a picture the resample pass scales takes the centred siting (an area average of chroma is centred on its 2x2 luma cell).
mvhp_color_params_t Engine::picture_color(int idr, const mvhp_stream_params_t &p, const mvhp_output_geometry_t &g) const
{
    mvhp_color_params_t c{};
    if (!w_.color) return c;
    mvhp_display_info_t d{};
    const bool have = mvhp_stream_display(s_, idr, &d) == MVHP_SUCCESS;
    mvhp_color_resolve(have ? &d : nullptr, p.width_mbs * 16, p.height_mbs * 16, color_mode_, &c);
    const uint32_t w = (w_.turns & 1) ? g.out_h : g.out_w, h = (w_.turns & 1) ? g.out_w : g.out_h;
    if (w != g.crop_w || h != g.crop_h) c.siting = MVHP_CHROMA_CENTER;
    return c;
}

// the most pictures a launch may hold, of pictures that take per_picture bytes of device memory each
int Engine::launch_cap(size_t per_picture) const
{
    const int n_ctx = (int)ctx_.size();
    // the cap: four pictures per CU (the four-picture kernel's full round); a long job -- from 4096 pictures per context on --
    // runs its steady state in launches of 2048, eight per CU, which is what the eight-picture kernel wants (round 3: the
    // product path reaches the kernel the bench times; the ramp and the taper stay as they are)
    const int cap = opts_.batch_pictures > 0 ? opts_.batch_pictures : ((n_order_ >= 4096 * n_ctx) ? 2048 : 1024);
    size_t budget = ctx_[0].mem_budget;
    for (const Ctx &c : ctx_) budget = std::min(budget, c.mem_budget);
    return std::min(cap, (int)std::min<size_t>(1 << 20, std::max<size_t>(1, budget / std::max<size_t>(1, per_picture))));
}

int Engine::batch_capacity(const mvhp_stream_params_t &p, const mvhp_output_geometry_t &g, bool use_geom, int remaining) const
{
    int cap = launch_cap(batch_picture_bytes(p, g, use_geom, w_));
    for (const Ctx &c : ctx_)
        if (c.arena && c.arena_pictures > 0 && same_params(c.arena_params, p)) cap = std::min(cap, c.arena_pictures);
    return planned_batch(cap, remaining, next_batch_id_);
}

// batches ramp up (the first pictures should not wait for a full-size batch to fill), run at the cap, and taper off (the
// last batch's upload, kernel and download are the tail nobody overlaps with)
int Engine::planned_batch(int cap, int remaining, int batch_id) const
{
    const int n_ctx = (int)ctx_.size();
    const int share = (remaining + n_ctx - 1) / n_ctx;
    if (opts_.batch_pictures > 0) return std::max(1, std::min(cap, share));   // an explicit batch size is taken as given
    const int round = batch_id / n_ctx;                                         // batches each context has been given so far
    // the ramp starts at, and the taper ends on, one picture per entropy thread: the threads finish such a batch together, and
    // the last batch's upload + kernel + download (the tail nothing overlaps) is 6 ms for 16 full-HD pictures against 15 ms
    // for 64.  Round 3: both were 64 -- a 64-picture job was ONE launch (36 ms; 26 ms in batches of 16), tools/e2e_ab.py.
    const int unit = std::max(8, std::min(64, host_threads_ / n_ctx));
    const int ramp = round < 10 ? std::min((long)unit << round, (long)cap) : cap;
    const int taper = std::max(unit, (int)((remaining * 0.35 + n_ctx - 1) / n_ctx));
    int b = std::max(1, std::min(std::min(cap, ramp), std::min(share, taper)));
    if (share - b > 0 && share - b < unit / 2 && share <= cap) b = share;   // (no two-picture batch behind the last full one)
    return b;
}

bool Engine::ensure_devbuf(Ctx &c, DevBuf &b, const Batch &bt, std::string &err)
{
    // MINIVIDEO_PLACED=1 (opt-in; for engines that live long: the arena is one allocation of up to 200 GB, seconds to get):
    // the context's three batch buffers come from mvhp_placed_alloc_sets -- records, planes and RGB of a batch each in a group
    // of the device's memory regions of its own, which is where the bench's kernel timings are taken (DESIGN 3 "Placement").
    // Once, for the first batch shape the context sees, sized for the largest batch the job can form; a batch that does not fit
    // (another shape, a larger explicit batch) uses ordinary allocations as before.
    if (placed_ && api_.placed_alloc && !c.arena_tried) {
        c.arena_tried = true;
        const int n = std::max(bt.capacity, job_cap_);
        size_t bytes[kArenaKinds];
        for (int i = 0; i < kArenaKinds; i++) bytes[i] = (size_t)n * picture_bytes((BufKind)i, bt.params, bt.geom, false, kPlanesAndRgb);
        void *ptrs[12];
        const double t0 = now_s();
        c.arena = api_.placed_alloc(c.dev, 3, bytes, ptrs);
        {
            std::lock_guard<std::mutex> l(alloc_mu_);
            alloc_dev_s_ += now_s() - t0;
            if (c.arena) alloc_dev_bytes_ += 3 * (bytes[0] + bytes[1] + bytes[2] + bytes[3]);
        }
        if (c.arena) {
            c.arena_pictures = n;
            c.arena_params = bt.params;
            {   // what is left of the device now bounds every later ordinary allocation (a batch of another shape, another
                // context on this device): the budgets of all contexts on it are taken again
                const size_t free_b = api_.dev_free_bytes(c.dev);
                for (Ctx &o : ctx_) {
                    if (o.device != c.device) continue;
                    int sharers = 0;
                    for (const Ctx &j : ctx_) sharers += j.device == c.device;
                    o.mem_budget = std::min(o.mem_budget, free_b / 2 / (size_t)o.n_bufs / (size_t)std::max(1, sharers));
                }
            }
            for (int k = 0; k < 3; k++) {
                DevBuf &d = c.bufs[k];
                // (ordinary buffers from an earlier call of another shape are released; none is in use: the first batch)
                for (int i = 0; i < kArenaKinds; i++) {
                    if (d.m[i].p) api_.dev_free(c.dev, d.m[i].p);
                    d.m[i] = {(uint8_t *)ptrs[k * 4 + i], bytes[i]};
                }
                d.arena_piece = true;
            }
        }
    }
    if (b.arena_piece) {
        bool fits = true;
        for (int i = 0; i < kArenaKinds; i++)
            fits = fits && (size_t)bt.capacity * picture_bytes((BufKind)i, bt.params, bt.geom, false, kPlanesAndRgb) <= b.m[i].cap;
        // a batch the arena was not sized for (another picture size, a later and longer job): this batch buffer leaves the
        // arena for ordinary allocations -- its pieces stay where they are until the engine goes (batch_capacity() keeps
        // batches of the arena's own shape inside it)
        if (!fits) b.leave_arena();
    }
    // The sizing rule is a property of the kind.  The first four are sized for the largest batch this call can form on a context,
    // not for the batch at hand: the ramp and the taper hand a buffer batches of changing sizes, and every growth is a hipFree +
    // hipMalloc in the middle of the pipeline (hipFree waits for the device) -- the second and third call of an engine still paid
    // for that (0.55 s, then 0.51 s, same job).  The others -- output pictures of a geometry, JPEG blob and table, scores -- are
    // sized for the batch at hand: geometries change inside a job, and these buffers are the small side of a batch.
    static const struct { const char *of, *unit; } what[kBufKinds] = {
        {"", " pictures"}, {"", " pictures"}, {"", " pictures"}, {"", " pictures"}, {"the output pictures of ", ""}, {"the output pictures of ", ""},
        {"the unturned pictures of ", ""},
        {"the JPEG files of ", ""}, {"the JPEG files of ", ""}, {"the picture scores of ", ""}, {"the plane histograms of ", ""},
        {"the tensors of ", ""}, {"the tensor slots of ", ""}};
    const bool job_shape = bt.params.width_mbs == job_params_.width_mbs && bt.params.height_mbs == job_params_.height_mbs;
    for (int k = 0; k < kBufKinds; k++) {
        if (k < kArenaKinds && b.arena_piece) continue;   // (checked above; never grown one by one)
        const size_t n = (size_t)std::max(bt.capacity, k < kArenaKinds && job_shape ? job_cap_ : 0);
        if (!grow_dev(c, b, (BufKind)k, n * need(bt, (BufKind)k))) {
            err = std::string("out of device memory for ") + what[k].of + "a batch of " + std::to_string(bt.capacity) + what[k].unit;
            return false;
        }
    }
    return true;
}

// allocate or grow one batch buffer (bytes 0: not needed, what it holds stays)
bool Engine::grow_dev(Ctx &c, DevBuf &b, BufKind k, size_t bytes)
{
    auto &m = b.m[k];
    if (m.cap >= bytes) return true;
    const double t0 = now_s();
    if (m.p) api_.dev_free(c.dev, m.p);
    m.p = (uint8_t *)api_.dev_alloc(c.dev, bytes);
    m.cap = m.p ? bytes : 0;
    {
        std::lock_guard<std::mutex> l(alloc_mu_);
        alloc_dev_s_ += now_s() - t0;
        alloc_dev_bytes_ += bytes;
    }
    return m.p != nullptr;
}

// ---------------------------------------------------------------------------------------------------------------
// feeder
// ---------------------------------------------------------------------------------------------------------------
// The batch gets no more pictures.  Usually the uploader sees the total when it finishes the closing chunk; a batch
// closed after its last chunk went up is handed on here.
void Engine::close_batch(Batch *b)
{
    b->total = (int)b->seqs.size();
    b->t_closed = now_s() - t_start_;
    st_.max_batch_pictures = std::max(st_.max_batch_pictures, (uint32_t)b->total);
    if (b->ctx >= 0 && b->uploaded == b->total) {
        Ctx &cx = ctx_[(size_t)b->ctx];
        if (cx.open_batch == b->id) cx.open_batch = -1;
        if (b->dead) fail_batch(b, b->dead_why);
        else cx.to_launch.push_back(b->id);
    }
}

// MVHP_OUT_TENSOR: a picture of the delivered geometry g has a tensor of the request's canvas and, with device delivery, a slot of
// the target: slot `seq`, every slot of one size -- the canvas's, or with canvas 0 the first issued picture's.
bool Engine::tensor_fits(int seq, const mvhp_output_geometry_t &g, std::string &why)
{
    if (!w_.tensor) return true;
    const mvhp_tensor_params_t t = tensor_params(w_, g);
    const size_t tb = mvtensor::bytes(t);
    if (!tb) {
        why = "the picture (" + std::to_string(g.out_w) + " x " + std::to_string(g.out_h) + ") does not fit the tensor canvas (" +
              std::to_string(t.canvas_w) + " x " + std::to_string(t.canvas_h) + ")";
        return false;
    }
    if (!w_.treq.d_target) return true;
    if ((uint32_t)seq >= w_.treq.target_pictures) {
        why = "picture " + std::to_string(seq) + " is past the tensor target's " + std::to_string(w_.treq.target_pictures) + " slots";
        return false;
    }
    if (!tensor_slot_bytes_) tensor_slot_bytes_ = tb;
    if (tb != tensor_slot_bytes_) {
        why = "device delivery without a canvas: the picture's tensor (" + std::to_string(tb) + " bytes) is not of the slots' size (" +
              std::to_string(tensor_slot_bytes_) + ")";
        return false;
    }
    return true;
}

void Engine::feeder()
{
    std::unique_lock<std::mutex> l(mu_);
    Batch *cur = nullptr;   // the open batch
    for (;;) {
        RetryGroup *rg = retry_q_.empty() ? nullptr : &retry_q_.front();
        const bool have = rg || (pos_ < n_order_ && allowance() > 0);
        // an open batch is closed as soon as it cannot take the next picture: nothing may be issued right now, or the
        // next pictures are a re-queued group (they go into a batch of their own, kept off the context they failed on)
        if (cur && (stop_ || !have || cur->retry != (rg != nullptr) || (rg && rg->exclude_ctx != cur->exclude_ctx))) {
            close_batch(cur);
            cur = nullptr;
            cv_.notify_all();
        }
        if (stop_) return;
        if (!have) { cv_.wait(l); continue; }
        const int first_seq = rg ? rg->seqs[rg->pos] : pos_;
        mvhp_stream_params_t p0{};
        if (mvhp_stream_params(s_, order_[first_seq], &p0) != MVHP_SUCCESS) {
            // a picture whose parameter sets never arrived fails without occupying a slot (never a re-queued one)
            PicResult &r = results_[(size_t)first_seq];
            const mvhp_stream::Idr &idr = s_->idrs[(size_t)order_[first_seq]];
            r.rc = MVHP_FAILURE;
            r.err = idr.why.empty() ? "parameter sets missing" : idr.why;
            r.ready = true;
            if (rg) { if (++rg->pos >= rg->seqs.size()) retry_q_.pop_front(); }
            else { pos_++; issued_++; }
            cv_.notify_all();
            continue;
        }
        mvhp_output_geometry_t g0{};
        bool use0 = false;
        {
            std::string why;
            if (!picture_geometry(order_[first_seq], p0, g0, use0, why) || !tensor_fits(first_seq, g0, why)) {
                // a picture whose geometry cannot be formed (the crop leaves nothing), or whose tensor has no place (larger than
                // the canvas, past the target's last slot), fails without occupying a slot
                PicResult &r = results_[(size_t)first_seq];
                r.rc = MVHP_FAILURE;
                r.err = why;
                r.params = p0;
                r.ready = true;
                if (rg) { if (++rg->pos >= rg->seqs.size()) retry_q_.pop_front(); }
                else { pos_++; issued_++; }
                cv_.notify_all();
                continue;
            }
        }
        const mvhp_color_params_t c0 = picture_color(order_[first_seq], p0, g0);
        if (cur && (!same_params(cur->params, p0) || !same_geometry(cur->geom, g0) || !same_color(cur->color, c0))) {   // a batch holds one
            close_batch(cur);                                                // set of stream parameters, one geometry and one colour setting
            cur = nullptr;
        }
        const int avail = rg ? (int)(rg->seqs.size() - rg->pos) : std::min(allowance(), n_order_ - pos_);
        if (!cur) {
            auto nb = std::make_unique<Batch>();
            nb->id = next_batch_id_++;
            nb->params = p0;
            nb->geom = g0;
            nb->use_geom = use0;
            nb->color = c0;
            nb->capacity = batch_capacity(p0, g0, use0, avail);
            nb->retry = rg != nullptr;
            nb->exclude_ctx = rg ? rg->exclude_ctx : -1;
            nb->seqs.reserve((size_t)nb->capacity);
            nb->t_open = now_s() - t_start_;
            cur = nb.get();
            batches_[cur->id] = std::move(nb);
        }
        const int C = std::min(chunk_pictures(p0), cur->capacity);
        int n = std::min(std::min(C, avail), cur->capacity - (int)cur->seqs.size());
        auto seq_at = [&](int i) { return rg ? rg->seqs[rg->pos + (size_t)i] : pos_ + i; };
        int same = 1;
        while (same < n) {
            mvhp_stream_params_t pi{};
            if (mvhp_stream_params(s_, order_[seq_at(same)], &pi) != MVHP_SUCCESS || !same_params(pi, p0)) break;
            mvhp_output_geometry_t gi{};
            bool ui = false;
            std::string why;
            if (!picture_geometry(order_[seq_at(same)], pi, gi, ui, why) || !same_geometry(gi, g0)) break;
            if (!tensor_fits(seq_at(same), gi, why)) break;   // (it fails as the first picture of the next round)
            if (!same_color(picture_color(order_[seq_at(same)], pi, gi), c0)) break;
            same++;
        }
        n = same;
        // a free page-locked chunk (the pool grows up to its limit; page-locking happens outside the lock)
        InChunk *c = nullptr;
        const size_t pic_bytes = compact_slot_bytes(p0);
        for (;;) {
            if (stop_) break;
            if (!free_in_.empty()) { c = free_in_.front(); free_in_.pop_front(); break; }
            if (all_in_.size() < in_limit_) {
                all_in_.push_back(std::make_unique<InChunk>());
                c = all_in_.back().get();
                break;
            }
            const double w0 = now_s();
            cv_.wait(l);
            feeder_wait_chunk_ += now_s() - w0;
        }
        if (!c) continue;   // stopping: the head of the loop closes the batch
        bool have_mem = true;
        if (c->buf.cap < (size_t)C * pic_bytes) {
            l.unlock();
            have_mem = grow(c->buf, (size_t)C * pic_bytes);
            l.lock();
            // `rg` is NOT fetched again: a group another context pushed meanwhile waits for the next iteration (`avail` and
            // `n` were sized without it), and push_back keeps references to a deque's elements valid -- only this
            // thread pops
        }
        if (!have_mem) {   // no page-locked memory: these pictures fail
            free_in_.push_back(c);
            for (int i = 0; i < n; i++) {
                PicResult &r = results_[(size_t)seq_at(i)];
                r.rc = MVHP_FAILURE;
                r.err = "out of page-locked host memory";
                r.ready = true;
            }
        } else {
            c->batch = cur->id;
            c->first_slot = (int)cur->seqs.size();
            c->n = n;
            c->pic_bytes = pic_bytes;
            c->used.assign((size_t)n, 0);
            c->remaining = n;
            for (int i = 0; i < n; i++) {
                const int seq = seq_at(i);
                cur->seqs.push_back(seq);
                PicResult &r = results_[(size_t)seq];
                r.params = p0;
                r.geom = g0;
                r.parsed_ok = false;
                work_q_.push_back(Item{c, i, seq});
            }
            st_.pictures_issued += (uint32_t)n;
        }
        if (rg) {
            rg->pos += (size_t)n;
            if (rg->pos >= rg->seqs.size()) {
                retry_q_.pop_front();
                if (cur) { close_batch(cur); cur = nullptr; }   // one batch per re-queued group
            }
        } else {
            pos_ += n;
            issued_ += n;
        }
        if (cur && (int)cur->seqs.size() >= cur->capacity) {
            close_batch(cur);
            cur = nullptr;
        }
        if (cur && cur->seqs.empty()) {   // (only after an allocation failure on a batch's first chunk)
            batches_.erase(cur->id);
            cur = nullptr;
        }
        cv_.notify_all();
    }
}

// ---------------------------------------------------------------------------------------------------------------
// entropy workers
// ---------------------------------------------------------------------------------------------------------------
void Engine::worker(int t)
{
    for (;;) {
        Item it;
        {
            std::unique_lock<std::mutex> l(mu_);
            const double w0 = now_s();
            cv_.wait(l, [&] { return stop_ || !work_q_.empty(); });
            if (stop_) return;
            worker_wait_[(size_t)t] += now_s() - w0;
            it = work_q_.front();
            work_q_.pop_front();
        }
        const int idr = order_[it.seq];
        std::string err;
        const double t0 = now_s();
        uint8_t *slot = it.chunk->buf.p + (size_t)it.slot * it.chunk->pic_bytes;
        size_t used = 0;
        const int rc = s_->decode_compact(idr, slot, it.chunk->pic_bytes, &used, err);
        if (rc != h264::RC_SUCCESS) {   // the slot still has to expand to something: an empty picture
            const mvhp_stream::Idr &d = s_->idrs[(size_t)idr];
            used = write_empty_compact(slot, (size_t)d.sps.width_mbs * (size_t)d.sps.height_map_units);
        }
        it.chunk->used[(size_t)it.slot] = used;   // (each slot has one writer; read by the uploader behind the engine mutex)
        worker_busy_[(size_t)t] += now_s() - t0;
        bool wake = false;
        if (idr >= 0 && (size_t)idr < s_->idrs.size()) stream_bytes_ += s_->samples[s_->idrs[(size_t)idr].sample].nal_size;
        {
            std::lock_guard<std::mutex> l(mu_);
            PicResult &r = results_[(size_t)it.seq];
            t_last_entropy_ = now_s() - t_start_;
            if (rc == h264::RC_SUCCESS) {
                r.parsed_ok = true;
            } else {   // final: entropy decoding is deterministic, a second try would fail the same way
                r.parsed_ok = false;
                r.rc = rc;
                r.err = err;
                r.ready = true;
            }
            wake = rc != h264::RC_SUCCESS;   // a final result: the sink may be waiting for exactly this picture
            if (--it.chunk->remaining == 0) {
                auto bi = batches_.find(it.chunk->batch);
                if (bi != batches_.end()) bi->second->ready.push_back(it.chunk);
                else free_in_.push_back(it.chunk);
                wake = true;                 // a chunk for the uploader (or back in the pool for the feeder)
            }
        }
        // (every waiter shares one condition variable: waking them per picture cost the sixteen entropy threads' CPU quota --
        //  a decoded picture inside an unfinished chunk changes nothing anyone waits for)
        if (wake) cv_.notify_all();
    }
}

// ---------------------------------------------------------------------------------------------------------------
// per-context stages
// ---------------------------------------------------------------------------------------------------------------
bool Engine::pick_chunk(int k, InChunk **c, Batch **b)
{
    Ctx &cx = ctx_[(size_t)k];
    if (cx.open_batch >= 0) {
        Batch *ob = batches_[cx.open_batch].get();
        if (ob->ready.empty()) return false;
        *c = ob->ready.front();
        ob->ready.pop_front();
        *b = ob;
        return true;
    }
    DevBuf *fb = nullptr;
    for (int i = 0; i < cx.n_bufs; i++)
        if (!cx.bufs[i].busy) { fb = &cx.bufs[i]; break; }
    if (!fb) return false;
    for (auto &kv : batches_) {   // lowest id first: batches are claimed in the order they were opened
        Batch *nb = kv.second.get();
        if (nb->ctx >= 0 || nb->ready.empty()) continue;
        if (nb->exclude_ctx == k) continue;
        nb->ctx = k;
        nb->t_claim = now_s() - t_start_;
        nb->buf = fb;
        fb->busy = true;
        cx.open_batch = nb->id;
        *c = nb->ready.front();
        nb->ready.pop_front();
        *b = nb;
        return true;
    }
    return false;
}

void Engine::release_batch(Batch *b)
{
    if (b->buf) b->buf->busy = false;
    for (InChunk *c : b->ready) free_in_.push_back(c);
    batches_.erase(b->id);
}

// A batch that failed on its context: entropy-decode its pictures again and queue them for another context, once.
void Engine::fail_batch(Batch *b, const std::string &why)
{
    std::vector<int> open;
    const int n = b->total >= 0 ? b->total : (int)b->seqs.size();
    for (int i = 0; i < n; i++) {
        const PicResult &r = results_[(size_t)b->seqs[(size_t)i]];
        if (r.parsed_ok && !r.ready) open.push_back(b->seqs[(size_t)i]);
    }
    if (!b->retry && ctx_.size() > 1 && !open.empty()) {
        RetryGroup g;
        g.seqs = open;
        g.exclude_ctx = b->ctx;
        retry_q_.push_back(std::move(g));
        st_.batches_requeued++;
    } else {
        for (int seq : open) {
            PicResult &r = results_[(size_t)seq];
            r.rc = MVHP_FAILURE;
            r.err = why;
            r.ready = true;
        }
    }
    release_batch(b);
}

void Engine::uploader(int k)
{
    Ctx &cx = ctx_[(size_t)k];
    for (;;) {
        InChunk *c = nullptr;
        Batch *b = nullptr;
        {
            std::unique_lock<std::mutex> l(mu_);
            cv_.wait(l, [&] { return stop_ || pick_chunk(k, &c, &b); });
            if (stop_) return;
        }
        // b stays alive: only this context's stages release a batch it has claimed
        std::string err;
        float ms = 0.f;
        bool ok = !b->dead;
        if (ok) ok = ensure_devbuf(cx, *b->buf, *b, err);   // sized once per batch (capacity is fixed when it opens)
        if (ok) {
            std::vector<void *> dst((size_t)c->n);
            std::vector<const void *> src((size_t)c->n);
            size_t bytes = 0;
            for (int i = 0; i < c->n; i++) {   // only what the entropy stage wrote crosses the link
                dst[(size_t)i] = b->buf->m[kCompact].p + (size_t)(c->first_slot + i) * c->pic_bytes;
                src[(size_t)i] = c->buf.p + (size_t)i * c->pic_bytes;
                bytes += c->used[(size_t)i];
            }
            ok = api_.h2d(cx.dev, c->n, dst.data(), src.data(), c->used.data(), &ms, err) == MVHP_SUCCESS;
            if (ok) {
                std::lock_guard<std::mutex> l(mu_);
                st_.h2d_s += ms * 1e-3;
                st_.h2d_bytes += bytes;
            }
        }
        {
            std::lock_guard<std::mutex> l(mu_);
            if (!ok && !b->dead) { b->dead = true; b->dead_why = err; }
            b->uploaded += c->n;
            free_in_.push_back(c);
            if (b->total >= 0 && b->uploaded == b->total) {
                cx.open_batch = -1;
                b->t_uploaded = now_s() - t_start_;
                if (b->dead) fail_batch(b, b->dead_why);
                else cx.to_launch.push_back(b->id);
            }
        }
        cv_.notify_all();
    }
}

void Engine::launcher(int k)
{
    Ctx &cx = ctx_[(size_t)k];
    for (;;) {
        Batch *b = nullptr;
        bool inject = false;
        {
            std::unique_lock<std::mutex> l(mu_);
            cv_.wait(l, [&] { return stop_ || !cx.to_launch.empty(); });
            if (stop_) return;
            b = batches_[cx.to_launch.front()].get();
            cx.to_launch.pop_front();
            if (cx.fail_next) { cx.fail_next = false; inject = true; }
        }
        std::string err;
        BatchDone done{};
        int rc = MVHP_FAILURE;
        const double t_call = now_s();
        if (inject) err = "injected failure (test hook)";
        else if (w_.score && !(api_.caps & CAP_SCORE)) err = "this device table has no picture-score operation";
        else if (w_.bars && !(api_.caps & CAP_BARS)) err = "this device table has no black-bar operation";
        else if (w_.hist && !(api_.caps & CAP_HIST)) err = "this device table has no plane-histogram operation";
        else if (w_.jpeg && !(api_.caps & CAP_JPEG)) err = "this device table has no JPEG operation";
        else if (w_.png && !(api_.caps & CAP_PNG)) err = "this device table has no PNG operation";
        else if (b->use_geom && !w_.jpeg && !(api_.caps & CAP_GEOMETRY)) err = "this device table has no output-geometry operation";
        else if (w_.turns && !(api_.caps & CAP_ORIENT)) err = "this device table has no orientation operation";
        else if (w_.color && !(api_.caps & CAP_COLOR)) err = "this device table has no colour operation";
        else {
            auto buf = [&](BufKind k) { return need(*b, k) ? b->buf->m[k].p : nullptr; };   // (a buffer may hold an earlier batch's kind)
            BatchJob job{};
            job.params = &b->params;
            job.d_compact = buf(kCompact);
            job.stride = need(*b, kCompact);
            job.d_packed = buf(kPacked);
            job.n = b->total;
            job.d_yuv = buf(kYuv);
            job.d_rgb = buf(kRgb);
            job.geom = b->use_geom || w_.jpeg || w_.png || w_.color ? &b->geom : nullptr;
            job.color = w_.color ? &b->color : nullptr;
            job.out_yuv = buf(kOutYuv);
            job.out_rgb = buf(kOutRgb);
            job.turns = w_.turns;
            job.mid_yuv = buf(kMidYuv);
            job.jpeg = w_.jpeg ? &jpeg_ : nullptr;
            job.png = w_.png ? &png_ : nullptr;
            job.blob = buf(kJpegBlob);
            job.blob_cap = (size_t)b->total * need(*b, kJpegBlob);
            job.table = (mvhp_jpeg_entry_t *)buf(kJpegTab);
            job.stats = w_.score ? (mvhp_luma_stats_t *)buf(kStats) : nullptr;
            job.bars = w_.bars ? (mvhp_luma_bars_t *)buf(kStats) : nullptr;
            job.bars_level = w_.bars_level;
            job.hist = w_.hist ? (mvhp_plane_hist_t *)buf(kHist) : nullptr;
            const mvhp_tensor_params_t tensor = tensor_params(w_, b->geom);
            std::vector<int32_t> slots;
            if (w_.tensor) {
                job.tensor = &tensor;
                job.tensor_out = w_.treq.d_target ? w_.treq.d_target : (void *)buf(kTensor);
                if (w_.treq.d_target) {   // picture `seq` into slot `seq`; a picture that failed to parse (final by now) into none
                    slots.resize((size_t)b->total);
                    std::lock_guard<std::mutex> l(mu_);
                    for (int i = 0; i < b->total; i++) {
                        const PicResult &r = results_[(size_t)b->seqs[(size_t)i]];
                        slots[(size_t)i] = r.parsed_ok && !r.ready ? b->seqs[(size_t)i] : -1;
                    }
                    job.slots_host = slots.data();
                    job.d_slots = (int32_t *)buf(kSlots);
                }
            }
            rc = api_.run_batch(cx.dev, job, done, err);
        }
        const float ms = done.ms;
        const int layout = done.layout;
        if (!cx.launched_once) {   // host time of the first call beyond the device time: code-object load, first-launch setup
            cx.launched_once = true;
            std::lock_guard<std::mutex> la(alloc_mu_);
            first_launch_s_ += std::max(0.0, (now_s() - t_call) - ms * 1e-3);
        }
        {
            std::lock_guard<std::mutex> l(mu_);
            if (rc == MVHP_SUCCESS) {
                st_.batches++;
                if (b->use_geom) st_.geometry_launches++;
                st_.kernel_s += ms * 1e-3;
                if (layout >= 0 && layout < 4) st_.launches_by_layout[layout]++;
                else if (layout >= MVHP_LAYOUT_WIDE && layout <= MVHP_LAYOUT_PIPE1) st_.launches_wide[layout - MVHP_LAYOUT_WIDE]++;
                b->t_kernel = now_s() - t_start_;
                cx.to_download.push_back(b->id);
            } else {
                fail_batch(b, err);
            }
        }
        cv_.notify_all();
    }
}

void Engine::release_picture(int seq)
{
    {
        std::lock_guard<std::mutex> l(mu_);
        if (seq >= 0 && seq == in_sink_) { released_early_ = true; return; }   // its callback is still running: see the sink loop
        if (seq < 0 || (size_t)seq >= results_.size() || !results_[(size_t)seq].kept) return;
        PicResult &r = results_[(size_t)seq];
        r.kept = false;
        if (r.oc && --r.oc->refs == 0) put_out(r.oc);
        r.oc = nullptr;
        kept_--;
    }
    cv_.notify_all();
}

const mvhp_plane_hist_t *Engine::picture_hist(int seq)
{
    std::lock_guard<std::mutex> l(mu_);
    if (seq < 0 || (size_t)seq >= results_.size()) return nullptr;
    const PicResult &r = results_[(size_t)seq];
    // (inside the picture's sink call, or kept by it: its output chunk, which holds the record, is referenced)
    if ((seq != in_sink_ && !r.kept) || r.rc != MVHP_SUCCESS || !r.oc) return nullptr;
    return r.hist;
}

int Engine::set_tensor(const mvhp_tensor_request_t *t, std::string &err)
{
    std::lock_guard<std::mutex> l(mu_);
    if (s_) { err = "mvhp_engine_set_tensor: a decode call is running"; return MVHP_FAILURE; }
    if (!t) { have_tensor_req_ = false; tensor_req_ = mvhp_tensor_request_t{}; return MVHP_SUCCESS; }
    // (judged for a picture that fills the canvas -- one sample where there is none -- every picture is judged again when it is issued)
    const mvhp_tensor_params_t p = mvtensor::of_request(*t, t->canvas_w ? t->canvas_w : 1, t->canvas_h ? t->canvas_h : 1);
    const char *why = mvtensor::malformed(p);
    if (!why && !mvtensor::finite(p)) why = "scale / bias (not finite)";
    if (!why && t->reserved) why = "reserved (must be 0)";
    if (!why && ((uintptr_t)t->d_target & 15)) why = "d_target (not 16-byte aligned)";
    if (!why && t->d_target && !t->target_pictures) why = "target_pictures (0 with a device target)";
    if (why) { err = std::string("mvhp_engine_set_tensor: invalid ") + why; return MVHP_FAILURE; }
    tensor_req_ = *t;
    have_tensor_req_ = true;
    return MVHP_SUCCESS;
}

void Engine::put_out(OutChunk *oc)
{
    free_out_.push_back(oc);
}

void Engine::downloader(int k)
{
    Ctx &cx = ctx_[(size_t)k];
    for (;;) {
        Batch *b = nullptr;
        {
            std::unique_lock<std::mutex> l(mu_);
            cv_.wait(l, [&] { return stop_ || !cx.to_download.empty(); });
            if (stop_) return;
            b = batches_[cx.to_download.front()].get();
            cx.to_download.pop_front();
        }
        // what comes back, from where, how many bytes per picture (a batch with a geometry: only its output pictures)
        const BufKind ky = planes_kind(b->use_geom), kr = rgb_kind(b->use_geom);
        // (MVHP_OUT_TENSOR: the tensors take the place of the RGB -- the batch's own with host delivery, none with device delivery,
        //  where the pictures are in the caller's memory already: the batch's kernels have completed)
        const size_t yb = w_.yuv ? need(*b, ky) : 0, rb = w_.tensor ? need(*b, kTensor) : w_.rgb ? need(*b, kr) : 0, sb = need(*b, kStats);
        const size_t hb = need(*b, kHist);
        const uint32_t tensor_len = w_.tensor ? (uint32_t)std::min<size_t>(mvtensor::bytes(tensor_params(w_, b->geom)), UINT32_MAX) : 0;
        const uint8_t *d_y = b->buf->m[ky].p, *d_r = b->buf->m[w_.tensor ? kTensor : kr].p, *d_s = b->buf->m[kStats].p, *d_h = b->buf->m[kHist].p;
        const int C = std::min(chunk_pictures(b->params), b->capacity);
        std::string fail;
        for (int g = 0; g < b->total && fail.empty(); g += C) {
            const int n = std::min(C, b->total - g);
            OutChunk *oc = nullptr;
            {
                // A free output chunk.  The pool is bounded, except that a starved sink lets it grow: every parked
                // chunk is then ahead of the picture the sink waits for, and that picture may need a chunk itself
                // (re-queued batches run behind later ones).
                std::unique_lock<std::mutex> l(mu_);
                for (;;) {
                    if (stop_) return;
                    if (!free_out_.empty()) { oc = free_out_.front(); free_out_.pop_front(); break; }
                    if (all_out_.size() < out_limit_ || sink_waiting_) {
                        all_out_.push_back(std::make_unique<OutChunk>());
                        oc = all_out_.back().get();
                        break;
                    }
                    cv_.wait(l);
                }
            }
            std::string err;
            float ms = 0.f, ms2 = 0.f;
            // MVHP_OUTPUT_SCORE: the chunk's records travel with it, one more piece of the chunk's own download call
            const mvhp_luma_stats_t *recs = nullptr;
            const size_t score_bytes = (size_t)n * sb;
            // MVHP_OUTPUT_HIST: likewise, one more piece
            const size_t hist_bytes = (size_t)n * hb;
            if (!grow(oc->stats, (size_t)C * sb) || !grow(oc->hist, (size_t)C * hb)) {
                std::lock_guard<std::mutex> l(mu_);
                put_out(oc);
                fail = "out of page-locked host memory";
                continue;
            }
            const mvhp_luma_bars_t *boxes = nullptr;   // MVHP_OUTPUT_BARS: the same piece, the other record
            if (sb && w_.score) recs = (const mvhp_luma_stats_t *)oc->stats.p;
            if (sb && w_.bars) boxes = (const mvhp_luma_bars_t *)oc->stats.p;
            const mvhp_plane_hist_t *hists = hb ? (const mvhp_plane_hist_t *)oc->hist.p : nullptr;
            if (w_.jpeg || w_.png) {   // the table rows of the chunk's pictures, then exactly the bytes they name, one piece per file
                const mvhp_jpeg_entry_t *tab = nullptr;
                const size_t tb = need(*b, kJpegTab);
                size_t base = 0, span = 0, moved = (size_t)n * tb;
                bool ok = grow(oc->tab, (size_t)C * tb);
                if (!ok) err = "out of page-locked host memory";
                if (ok) {
                    void *dst[3] = {oc->tab.p};
                    const void *src[3] = {b->buf->m[kJpegTab].p + (size_t)g * tb};
                    size_t nb[3] = {moved};
                    int np = 1;
                    if (sb) { dst[np] = oc->stats.p; src[np] = d_s + (size_t)g * sb; nb[np++] = score_bytes; }
                    if (hb) { dst[np] = oc->hist.p; src[np] = d_h + (size_t)g * hb; nb[np++] = hist_bytes; }
                    ok = api_.d2h(cx.dev, np, dst, src, nb, &ms, err) == MVHP_SUCCESS;
                    tab = (const mvhp_jpeg_entry_t *)oc->tab.p;
                }
                const size_t blob_cap = (size_t)b->total * need(*b, kJpegBlob);
                if (ok) {
                    base = (size_t)tab[0].offset;
                    for (int i = 0; i < n && ok; i++) {
                        if (tab[i].status != MVHP_JPEG_OK) continue;
                        if (tab[i].offset < base || tab[i].offset > blob_cap || tab[i].length > blob_cap - tab[i].offset) {
                            ok = false;
                            err = w_.png ? "the PNG table names bytes outside the blob" : "the JPEG table names bytes outside the blob";
                        }
                        span = std::max(span, (size_t)(tab[i].offset - base) + tab[i].length);
                    }
                }
                if (ok && span && !grow(oc->rgb, span)) { ok = false; err = "out of page-locked host memory"; }
                if (ok && span) {
                    std::vector<void *> dst;
                    std::vector<const void *> src;
                    std::vector<size_t> nb;
                    for (int i = 0; i < n; i++) {
                        if (tab[i].status != MVHP_JPEG_OK) continue;
                        dst.push_back(oc->rgb.p + (tab[i].offset - base));
                        src.push_back(b->buf->m[kJpegBlob].p + tab[i].offset);
                        nb.push_back(tab[i].length);
                        moved += tab[i].length;
                    }
                    ok = api_.d2h(cx.dev, (int)dst.size(), dst.data(), src.data(), nb.data(), &ms2, err) == MVHP_SUCCESS;
                }
                {
                    std::lock_guard<std::mutex> l(mu_);
                    if (ok) {
                        st_.d2h_s += (ms + ms2) * 1e-3;
                        st_.d2h_bytes += moved + score_bytes + hist_bytes;
                        oc->refs = 0;
                        for (int i = 0; i < n; i++) {
                            PicResult &r = results_[(size_t)b->seqs[(size_t)(g + i)]];
                            if (!r.parsed_ok || r.ready) continue;
                            if (tab[i].status == MVHP_JPEG_OK) {
                                r.rc = MVHP_SUCCESS;
                                r.oc = oc;
                                r.rgb = oc->rgb.p + (tab[i].offset - base);
                                r.geom.reserved[0] = tab[i].length;
                                oc->refs++;
                            } else {   // a JPEG larger than the raw picture is of no use: the picture fails, decoding goes on
                                r.rc = MVHP_FAILURE;
                                r.err = w_.png ? "the PNG file does not fit into the blob" : "the JPEG file does not fit into the room of the raw picture";
                            }
                            if (recs) r.geom.reserved[1] = mvblank::luma_score(recs[i].sum, recs[i].sumsq, recs[i].samples);
                            if (hists && r.rc == MVHP_SUCCESS) r.hist = hists + i;
                            r.yuv = nullptr;
                            r.ready = true;
                        }
                        if (oc->refs == 0) put_out(oc);
                    } else {
                        put_out(oc);
                        fail = err;
                    }
                }
                cv_.notify_all();
                continue;
            }
            bool ok = grow(oc->yuv, (size_t)C * yb) && grow(oc->rgb, (size_t)C * rb);
            if (!ok) err = "out of page-locked host memory";
            if (ok) {
                void *dst[4];
                const void *src[4];
                size_t nb[4];
                int np = 0;
                if (yb) { dst[np] = oc->yuv.p; src[np] = d_y + (size_t)g * yb; nb[np++] = (size_t)n * yb; }
                if (rb) { dst[np] = oc->rgb.p; src[np] = d_r + (size_t)g * rb; nb[np++] = (size_t)n * rb; }
                if (sb) { dst[np] = oc->stats.p; src[np] = d_s + (size_t)g * sb; nb[np++] = score_bytes; }
                if (hb) { dst[np] = oc->hist.p; src[np] = d_h + (size_t)g * hb; nb[np++] = hist_bytes; }
                ok = np == 0 || api_.d2h(cx.dev, np, dst, src, nb, &ms, err) == MVHP_SUCCESS;   // (np 0: tensors delivered on the device)
            }
            {
                std::lock_guard<std::mutex> l(mu_);
                if (ok) {
                    st_.d2h_s += (ms + ms2) * 1e-3;
                    st_.d2h_bytes += (uint64_t)n * (yb + rb) + score_bytes + hist_bytes;
                    oc->refs = 0;
                    for (int i = 0; i < n; i++) {
                        PicResult &r = results_[(size_t)b->seqs[(size_t)(g + i)]];
                        if (!r.parsed_ok || r.ready) continue;
                        r.rc = MVHP_SUCCESS;
                        r.oc = oc;
                        r.yuv = yb ? oc->yuv.p + (size_t)i * yb : nullptr;
                        r.rgb = rb ? oc->rgb.p + (size_t)i * rb : nullptr;
                        if (recs) r.geom.reserved[1] = mvblank::luma_score(recs[i].sum, recs[i].sumsq, recs[i].samples);
                        if (boxes) {   // (sides are at most 16384: two to a word)
                            r.geom.reserved[0] = boxes[i].x | boxes[i].y << 16;
                            r.geom.reserved[1] = boxes[i].w | boxes[i].h << 16;
                        }
                        if (hists) r.hist = hists + i;
                        if (w_.tensor) r.geom.reserved[0] = tensor_len;
                        r.ready = true;
                        oc->refs++;
                    }
                    if (oc->refs == 0) put_out(oc);
                } else {
                    put_out(oc);
                    fail = err;
                }
            }
            cv_.notify_all();
        }
        {
            std::lock_guard<std::mutex> l(mu_);
            t_last_download_ = now_s() - t_start_;
            if (getenv("MINIVIDEO_ENGINE_TRACE"))
                fprintf(stderr, "engine trace: batch %d: %d pictures, opened %.4f claimed %.4f closed %.4f uploaded %.4f kernel done %.4f downloaded %.4f\n",
                        b->id, b->total, b->t_open, b->t_claim, b->t_closed, b->t_uploaded, b->t_kernel, t_last_download_);
            if (!fail.empty()) fail_batch(b, fail);   // pictures already delivered stay delivered
            else release_batch(b);
        }
        cv_.notify_all();
    }
}

// ---------------------------------------------------------------------------------------------------------------
// one decode call
// ---------------------------------------------------------------------------------------------------------------
int Engine::decode(const mvhp_stream &s, const int *order, int n_order, int wanted, int out_mask, const mvhp_output_request_t *req,
                   mvhp_picture_sink_t sink, mvhp_picture_sink_ex_t sink_ex, void *user, mvhp_decode_stats_t *stats,
                   std::string &err)
{
    if (req && ((req->flags & ~(MVHP_OUTPUT_CROP | MVHP_OUTPUT_BOX | MVHP_OUTPUT_SCORE | MVHP_OUTPUT_ORIENT | MVHP_OUTPUT_ROTATE_MASK | MVHP_OUTPUT_ASPECT | MVHP_OUTPUT_COLOR | MVHP_OUTPUT_COLOR_MODE_MASK | MVHP_OUTPUT_BARS | MVHP_OUTPUT_TRIM | MVHP_OUTPUT_HIST)) ||
                ((req->flags & MVHP_OUTPUT_COLOR_MODE_MASK) >> MVHP_OUTPUT_COLOR_MODE_SHIFT) > 4 || ((req->flags & MVHP_OUTPUT_BOX) && (req->box_w < 2 || req->box_h < 2)))) {
        err = "malformed output request (box sides must be at least 2, colour modes are 0 to 4)";
        return MVHP_FAILURE;
    }
    if ((out_mask & MVHP_OUT_JPEG) && sink) {
        err = "MVHP_OUT_JPEG needs mvhp_engine_decode_ex: its sink gets the file's length with the geometry";
        return MVHP_FAILURE;
    }
    if ((out_mask & MVHP_OUT_PNG) && (sink || (out_mask & MVHP_OUT_JPEG))) {
        err = sink ? "MVHP_OUT_PNG needs mvhp_engine_decode_ex: its sink gets the file's length with the geometry"
                   : "MVHP_OUT_PNG and MVHP_OUT_JPEG are two output kinds: a call delivers one";
        return MVHP_FAILURE;
    }
    if (out_mask & MVHP_OUT_TENSOR) {   // (the tensor's length travels in g->reserved[0], as a file's length does)
        const char *why = sink ? "MVHP_OUT_TENSOR needs mvhp_engine_decode_ex: its sink gets the tensor's length with the geometry"
                          : (out_mask & MVHP_OUT_JPEG) ? "MVHP_OUT_TENSOR and MVHP_OUT_JPEG are two output kinds: a call delivers one"
                          : (out_mask & MVHP_OUT_PNG) ? "MVHP_OUT_TENSOR and MVHP_OUT_PNG are two output kinds: a call delivers one"
                          : (req && (req->flags & MVHP_OUTPUT_BARS)) ? "MVHP_OUTPUT_BARS and MVHP_OUT_TENSOR both use g->reserved[0]: a call delivers one"
                          : !have_tensor_req_ ? "MVHP_OUT_TENSOR without a tensor request: mvhp_engine_set_tensor comes first"
                          : !(api_.caps & CAP_TENSOR) ? "this device table has no tensor operation"
                          : (tensor_req_.d_target && ctx_.size() != 1) ? "MVHP_OUT_TENSOR with a device target needs an engine of exactly one context: the pointer belongs to one device" : nullptr;
        if (why) { err = why; return MVHP_FAILURE; }
    }
    if (req && (req->flags & MVHP_OUTPUT_BARS)) {   // the box travels in the two words that are the file length and the score elsewhere
        const char *why = sink ?"MVHP_OUTPUT_BARS needs mvhp_engine_decode_ex: its sink gets the box with the geometry"
                          : (out_mask & MVHP_OUT_JPEG) ? "MVHP_OUTPUT_BARS and MVHP_OUT_JPEG both use g->reserved[0]: a call delivers one"
                          : (out_mask & MVHP_OUT_PNG) ? "MVHP_OUTPUT_BARS and MVHP_OUT_PNG both use g->reserved[0]: a call delivers one"
                          : (req->flags & MVHP_OUTPUT_SCORE) ? "MVHP_OUTPUT_BARS and MVHP_OUTPUT_SCORE both use g->reserved[1]: a call delivers one"
                          : (req->flags & MVHP_OUTPUT_HIST) ? "MVHP_OUTPUT_BARS and MVHP_OUTPUT_HIST are two probes: a call runs one" : nullptr;
        if (why) { err = why; return MVHP_FAILURE; }
        const uint32_t level = req->reserved >> 24;
        if (level == 255) { err = "MVHP_OUTPUT_BARS: level 255 (1 ... 254; 0 = 24)"; return MVHP_FAILURE; }
    }
    if (!order || n_order <= 0 || wanted <= 0) { err = "nothing to decode"; return MVHP_FAILURE; }
    for (int i = 0; i < n_order; i++)
        if (order[i] < 0 || (size_t)order[i] >= s.idrs.size()) { err = "IDR index out of range"; return MVHP_FAILURE; }
    const double t_start = now_s();
    const int n_ctx = (int)ctx_.size();
    {
        std::lock_guard<std::mutex> l(mu_);
        s_ = &s; order_ = order; n_order_ = n_order; wanted_ = std::min(wanted, n_order);
        w_.jpeg = (out_mask & MVHP_OUT_JPEG) != 0;
        w_.png = (out_mask & MVHP_OUT_PNG) != 0;
        w_.tensor = (out_mask & MVHP_OUT_TENSOR) != 0;
        w_.treq = w_.tensor ? tensor_req_ : mvhp_tensor_request_t{};
        tensor_slot_bytes_ = 0;
        w_.rgb = !w_.jpeg && !w_.png && ((out_mask & 1) != 0 || w_.tensor);   // (a tensor call makes its RGB as MVHP_OUT_RGB_ONLY does)
        w_.yuv = !w_.jpeg && !w_.png && !w_.tensor && (!w_.rgb || (out_mask & 2) == 0);
        jpeg_ = mvhp_jpeg_params_t{};
        if (w_.jpeg) {   // mvhp_output_request_t::reserved carries the encoder's parameters
            const uint32_t rsv = req ? req->reserved : 0;
            jpeg_.quality = (rsv & 0xffu) ? (int32_t)(rsv & 0xffu) : 75;
            jpeg_.restart_mcus = (rsv >> 8) & 0xffffu;
        }
        req_ = req ? *req : mvhp_output_request_t{};
        w_.score = (req_.flags & MVHP_OUTPUT_SCORE) != 0;
        w_.bars = (req_.flags & MVHP_OUTPUT_BARS) != 0;
        w_.bars_level = (req_.reserved >> 24) ? (int)(req_.reserved >> 24) : MVHP_BARS_LEVEL_DEFAULT;
        w_.hist = (req_.flags & MVHP_OUTPUT_HIST) != 0;
        req_.flags &= ~(MVHP_OUTPUT_SCORE | MVHP_OUTPUT_BARS | MVHP_OUTPUT_HIST);   // (what is left decides the geometry: none = the path of a call without a request)
        // colour: only where the call delivers RGB or PNG; otherwise, and always for the geometry, the request without the bits
        w_.color = (req_.flags & MVHP_OUTPUT_COLOR) != 0 && (w_.rgb || w_.png);
        color_mode_ = (int)((req_.flags & MVHP_OUTPUT_COLOR_MODE_MASK) >> MVHP_OUTPUT_COLOR_MODE_SHIFT);
        req_.flags &= ~(MVHP_OUTPUT_COLOR | MVHP_OUTPUT_COLOR_MODE_MASK);
        w_.turns = mvhp_output_turns(&s, &req_);
        if (w_.turns == 0) req_.flags &= ~(MVHP_OUTPUT_ORIENT | MVHP_OUTPUT_ROTATE_MASK);   // (turns that come to 0: today's paths exactly)
        stop_ = false; sink_waiting_ = false;
        pos_ = issued_ = consumed_ = ok_ = failed_ = 0;
        next_batch_id_ = 0;
        results_.assign((size_t)n_order, PicResult());
        for (int i = 0; i < n_order; i++) results_[(size_t)i].idr = order[i];
        batches_.clear(); work_q_.clear(); retry_q_.clear();
        free_in_.clear(); free_out_.clear();
        for (auto &c : all_in_) free_in_.push_back(c.get());
        for (auto &c : all_out_) { c->refs = 0; free_out_.push_back(c.get()); }
        for (Ctx &c : ctx_) { c.open_batch = -1; c.to_launch.clear(); c.to_download.clear(); for (DevBuf &d : c.bufs) d.busy = false; c.fail_next = false; }
        if (opts_.fail_context >= 0 && opts_.fail_context < n_ctx) ctx_[(size_t)opts_.fail_context].fail_next = true;
        memset(&st_, 0, sizeof(st_));
        worker_busy_.assign((size_t)host_threads_, 0.0);
        worker_wait_.assign((size_t)host_threads_, 0.0);
        feeder_wait_chunk_ = t_last_entropy_ = t_last_download_ = 0;
        t_start_ = t_start;
        stream_bytes_ = 0;
        {
            std::lock_guard<std::mutex> la(alloc_mu_);
            alloc_host_s_ = alloc_dev_s_ = first_launch_s_ = first_picture_s_ = 0;
            alloc_host_bytes_ = alloc_dev_bytes_ = 0;
        }
        // pools: enough input chunks that every entropy thread has a slot to write while the earlier chunks upload (three
        // pictures per thread were measured too: no gain, and page-locking the extra chunks costs the first call 0.1 s), and
        // a few output chunks per context
        mvhp_stream_params_t p0{};
        int C = 8;
        for (int i = 0; i < n_order; i++)
            if (mvhp_stream_params(&s, order[i], &p0) == MVHP_SUCCESS) { C = chunk_pictures(p0); break; }
        in_limit_ = (size_t)std::max(3, (host_threads_ + C - 1) / C + 1 + n_ctx);
        if (const int e = env_int("MINIVIDEO_IN_CHUNKS", 0)) in_limit_ = (size_t)std::max(2, std::min(64, e));   // developer aid
        {   // the largest batch this call can form on a context: what a placed arena is sized for
            int cap = launch_cap(batch_picture_bytes(p0, coded_geometry(p0), false, kPlanesAndRgb));
            cap = std::max(1, std::min(cap, (wanted_ + n_ctx - 1) / n_ctx));
            job_cap_ = 1;   // the largest batch the ramp / cap / taper will actually form when nothing fails
            for (int rem = wanted_, id = 0; rem > 0; id++) {
                const int b = planned_batch(cap, rem, id);
                job_cap_ = std::max(job_cap_, b);
                rem -= b;
            }
            job_params_ = p0;
        }
        out_limit_ = (size_t)(2 * n_ctx + 2);
    }
    const int threads = std::min(host_threads_, std::max(1, wanted_));
    std::vector<std::thread> th;
    th.emplace_back([this] { feeder(); });
    for (int t = 0; t < threads; t++) th.emplace_back([this, t] { worker(t); });
    for (int k = 0; k < n_ctx; k++) {
        th.emplace_back([this, k] { uploader(k); });
        th.emplace_back([this, k] { launcher(k); });
        th.emplace_back([this, k] { downloader(k); });
    }

    // ---- sink loop (this thread) ----
    bool aborted = false;
    double sink_s = 0;
    for (int next = 0; next < n_order;) {
        PicResult r;
        {
            std::unique_lock<std::mutex> l(mu_);
            if (ok_ >= wanted_) break;
            if (!results_[(size_t)next].ready) {
                sink_waiting_ = true;   // (lets the downloader grow its pool rather than deadlock behind a re-queued batch)
                cv_.notify_all();
                cv_.wait(l, [&] { return results_[(size_t)next].ready; });
                sink_waiting_ = false;
            }
            r = results_[(size_t)next];
            in_sink_ = next;
            released_early_ = false;
        }
        if (next == 0) first_picture_s_ = now_s() - t_start;
        int verdict = (r.rc == MVHP_SUCCESS) ? 1 : 0;
        if (sink || sink_ex) {
            const double t0 = now_s();
            verdict = sink_ex ? sink_ex(user, next, r.idr, r.rc, r.err.c_str(), &r.params, &r.geom, r.yuv, r.rgb)
                              : sink(user, next, r.idr, r.rc, r.err.c_str(), &r.params, r.yuv, r.rgb);
            sink_s += now_s() - t0;
        }
        bool wake = false;
        {
            std::lock_guard<std::mutex> l(mu_);
            in_sink_ = -1;
            if (verdict == 2 && r.rc == MVHP_SUCCESS && r.oc && !released_early_) {   // kept by the sink: the chunk stays out until
                results_[(size_t)next].kept = true;                                    // release_picture(next)
                kept_++;
                verdict = 1;
            } else {   // (released_early_: the other thread was done with it before the callback had returned)
                if (verdict == 2) verdict = (r.rc == MVHP_SUCCESS) ? 1 : 0;
                if (r.oc && --r.oc->refs == 0) { put_out(r.oc); wake = true; }   // an output chunk for the downloader
                results_[(size_t)next].oc = nullptr;
            }
            consumed_++;
            if (r.rc == MVHP_SUCCESS && verdict == 1) ok_++;
            else { failed_++; wake = true; }                                  // the allowance grew: the feeder may issue another picture
        }
        if (wake) cv_.notify_all();
        next++;
        if (verdict < 0) { aborted = true; break; }
    }
    {
        std::lock_guard<std::mutex> l(mu_);
        stop_ = true;
    }
    cv_.notify_all();
    for (auto &t : th) t.join();
    {   // pictures the sink kept (verdict 2) live in this engine's output chunks: the call ends when the last one is back
        std::unique_lock<std::mutex> l(mu_);
        cv_.wait(l, [&] { return kept_ == 0; });
    }
    {
        std::lock_guard<std::mutex> l(mu_);
        batches_.clear();
        work_q_.clear();
        st_.pictures_ok = (uint32_t)ok_;
        st_.pictures_failed = (uint32_t)failed_;
        st_.contexts = (uint32_t)n_ctx;
        st_.host_threads = (uint32_t)threads;
        st_.sink_s = sink_s;
        st_.stream_bytes = stream_bytes_;
        for (double b : worker_busy_) st_.entropy_busy_s += b;
        st_.wall_s = now_s() - t_start;
        {
            std::lock_guard<std::mutex> la(alloc_mu_);
            st_.host_alloc_s = alloc_host_s_; st_.dev_alloc_s = alloc_dev_s_; st_.first_launch_s = first_launch_s_;
            st_.first_picture_s = first_picture_s_;
            st_.host_alloc_bytes = alloc_host_bytes_; st_.dev_alloc_bytes = alloc_dev_bytes_;
        }
        for (const Ctx &c : ctx_) if (c.arena) st_.placed_buffers = 1;
        if (getenv("MINIVIDEO_ENGINE_TRACE")) {   // where the wall time went (developer aid)
            double wait = 0, wmax = 0, bmin = 1e30, bmax = 0;
            for (double w : worker_wait_) { wait += w; wmax = std::max(wmax, w); }
            for (double b : worker_busy_) { bmin = std::min(bmin, b); bmax = std::max(bmax, b); }
            fprintf(stderr, "engine trace: wall %.4f s, threads %d: busy min %.4f max %.4f, waiting for work sum %.4f max %.4f; feeder waited %.4f s for a free "
                            "input chunk; last entropy result at %.4f s, last download at %.4f s, sink %.4f s, batches %u\n",
                    st_.wall_s, threads, bmin, bmax, wait, wmax, feeder_wait_chunk_, t_last_entropy_, t_last_download_, sink_s, st_.batches);
        }
        if (stats) *stats = st_;
        s_ = nullptr; order_ = nullptr;
    }
    if (aborted) { err = "stopped by the sink"; return MVHP_FAILURE; }
    if (ok_ >= wanted_ || ok_ > 0) return MVHP_SUCCESS;
    err = "no picture could be decoded";
    return MVHP_FAILURE;
}

Engine *engine_create(const DeviceApi &api, const mvhp_engine_opts_t *opts, std::string &err)
{
    Engine *e = new Engine(api);
    if (!e->init(opts, err)) { delete e; return nullptr; }
    return e;
}

void engine_destroy(Engine *e) { delete e; }
void engine_release_picture(Engine *e, int seq) { e->release_picture(seq); }
int engine_contexts(Engine *e) { return e ? e->contexts() : 0; }
int engine_set_tensor(Engine *e, const mvhp_tensor_request_t *t, std::string &err)
{
    if (!e) { err = "no engine"; return MVHP_FAILURE; }
    return e->set_tensor(t, err);
}
const mvhp_plane_hist_t *engine_picture_hist(Engine *e, int seq) { return e ? e->picture_hist(seq) : nullptr; }

int engine_decode(Engine *e, const mvhp_stream &s, const int *order, int n_order, int wanted, int out_mask,
                  const mvhp_output_request_t *req, mvhp_picture_sink_t sink, mvhp_picture_sink_ex_t sink_ex, void *user,
                  mvhp_decode_stats_t *stats, std::string &err)
{
    if (!e) { err = "no engine"; return MVHP_FAILURE; }
    return e->decode(s, order, n_order, wanted, out_mask, req, sink, sink_ex, user, stats, err);
}

} // namespace mvengine

// ---- C-ABI (include/minivideo_hotpath.h) ----
struct mvhp_engine {
    mvengine::Engine *e = nullptr;
};

static thread_local std::string g_engine_err;

extern "C" {

MVHP_EXPORT int mvhp_engine_create(const mvhp_engine_opts_t *opts, mvhp_engine_t **out)
{
    if (!out) return MVHP_FAILURE;
    *out = nullptr;
    mvengine::Engine *e = mvengine::engine_create(mvhp_hip_device_api(), opts, g_engine_err);
    if (!e) {
        fprintf(stderr, "[minivideo] %s\n", g_engine_err.c_str());
        return MVHP_FAILURE;
    }
    *out = new mvhp_engine{e};
    return MVHP_SUCCESS;
}

MVHP_EXPORT void mvhp_engine_destroy(mvhp_engine_t *h)
{
    if (!h) return;
    mvengine::engine_destroy(h->e);
    delete h;
}

MVHP_EXPORT void mvhp_engine_release_picture(mvhp_engine_t *h, int seq)
{
    if (h) mvengine::engine_release_picture(h->e, seq);
}

MVHP_EXPORT const mvhp_plane_hist_t *mvhp_engine_picture_hist(mvhp_engine_t *h, int seq)
{
    return h ? mvengine::engine_picture_hist(h->e, seq) : nullptr;
}

MVHP_EXPORT int mvhp_engine_contexts(mvhp_engine_t *h) { return h ? mvengine::engine_contexts(h->e) : 0; }

MVHP_EXPORT int mvhp_engine_set_tensor(mvhp_engine_t *h, const mvhp_tensor_request_t *t)
{
    if (!h) return MVHP_FAILURE;
    const int rc = mvengine::engine_set_tensor(h->e, t, g_engine_err);
    if (rc != MVHP_SUCCESS) fprintf(stderr, "[minivideo] %s\n", g_engine_err.c_str());
    return rc;
}

MVHP_EXPORT int mvhp_engine_decode(mvhp_engine_t *h, const mvhp_stream_t *s, const int *order, int n_order, int wanted,
                                   int want_rgb, mvhp_picture_sink_t sink, void *user, mvhp_decode_stats_t *stats)
{
    if (!h || !s) return MVHP_FAILURE;
    const int rc = mvengine::engine_decode(h->e, *s, order, n_order, wanted, want_rgb, nullptr, sink, nullptr, user, stats, g_engine_err);
    if (rc != MVHP_SUCCESS) fprintf(stderr, "[minivideo] %s\n", g_engine_err.c_str());
    return rc;
}

MVHP_EXPORT int mvhp_engine_decode_ex(mvhp_engine_t *h, const mvhp_stream_t *s, const int *order, int n_order, int wanted,
                                      int want_rgb, const mvhp_output_request_t *req, mvhp_picture_sink_ex_t sink, void *user,
                                      mvhp_decode_stats_t *stats)
{
    if (!h || !s) return MVHP_FAILURE;
    const int rc = mvengine::engine_decode(h->e, *s, order, n_order, wanted, want_rgb, req, nullptr, sink, user, stats, g_engine_err);
    if (rc != MVHP_SUCCESS) fprintf(stderr, "[minivideo] %s\n", g_engine_err.c_str());
    return rc;
}

} // extern "C"
