// api.cpp -- MiniVideo's public API (include/minivideo.h) over the split decoder:
//   minivideo_open   <- import.c:510 (import_fileOpen: path split, size, container sniff)
//   minivideo_parse  <- minivideo.c:199-251 + demuxer/esparser/esparser.c:40-143
//   minivideo_decode <- minivideo.c:255-303, demuxer/filter.c:52-215, decoder/h264/h264.c:41-195,
//                       export.c:618-767 (file naming, format fallbacks)
//   minivideo_close  <- import.c:570-616
// Entropy decoding runs on host threads, reconstruction + colour conversion on every visible HIP
// device (frame-level work queue, no collectives); pictures are written in stream order.
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "decode_engine.h"
#include "bars_policy.h"
#include "blank_policy.h"
#include "represent_policy.h"
#include "export.h"
#include "h264_frontend.h"
#include "minivideo.h"
#include "minivideo_hotpath.h"
#include "mp4_demux.h"
#include "stream_internal.h"

namespace {

void log_err(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void log_err(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "[minivideo] ");
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
}

// ---- import.c:60-135: absolute path, directory, name (no extension), extension ----
void infos_from_path(MediaFile_t *m)
{
    if (m->file_path[0] != '/') {
        char cwd[4096];
        if (getcwd(cwd, sizeof(cwd)) != NULL) {
            std::string abs = std::string(cwd) + "/" + m->file_path;
            if (abs.size() < sizeof(m->file_path)) {
                FILE *t = fopen(abs.c_str(), "r");
                if (t) { fclose(t); strncpy(m->file_path, abs.c_str(), sizeof(m->file_path) - 1); }
            }
        }
    }
    const char *slash = strrchr(m->file_path, '/');
    if (!slash) return;
    size_t dlen = (size_t)(slash - m->file_path) + 1;
    if (dlen > sizeof(m->file_directory) - 1) dlen = sizeof(m->file_directory) - 1;
    memcpy(m->file_directory, m->file_path, dlen);
    const char *dot = strrchr(m->file_path, '.');
    if (dot && dot > slash) {
        size_t nlen = (size_t)(dot - slash) - 1;
        if (nlen > sizeof(m->file_name) - 1) nlen = sizeof(m->file_name) - 1;
        memcpy(m->file_name, slash + 1, nlen);
        strncpy(m->file_extension, dot + 1, sizeof(m->file_extension) - 1);
    } else {
        strncpy(m->file_name, slash + 1, sizeof(m->file_name) - 1);
    }
}

// ---- import.c:186-470: magic bytes first, then the extension ----
ContainerFormat_e sniff_container(MediaFile_t *m)
{
    uint8_t b[16] = {0};
    rewind(m->file_pointer);
    if (fread(b, 1, sizeof(b), m->file_pointer) < 8) { /* tiny file: fall through to the extension */ }
    rewind(m->file_pointer);
    ContainerFormat_e c = CONTAINER_UNKNOWN;
    if (b[0] == 0x47) c = CONTAINER_MPEG_TS;
    else if (b[0] == 0x1A && b[1] == 0x45 && b[2] == 0xDF && b[3] == 0xA3) c = CONTAINER_MKV;
    else if (b[0] == 'R' && b[1] == 'I' && b[2] == 'F' && b[3] == 'F') {
        if (b[8] == 'A' && b[9] == 'V' && b[10] == 'I' && b[11] == ' ') c = CONTAINER_AVI;
        else if (b[8] == 'W' && b[9] == 'A' && b[10] == 'V' && b[11] == 'E') c = CONTAINER_WAVE;
    } else if (b[0] == 0 && b[1] == 0) {
        if (b[2] == 1) {
            if (b[3] == 0xBA) c = CONTAINER_MPEG_PS;
            else if (b[3] == 0xB3 || b[3] == 0x67) c = CONTAINER_ES;
        } else if (b[2] == 0 && b[3] == 1) {
            if (b[4] == 0xBA) c = CONTAINER_MPEG_PS;
            else if (b[4] == 0xB3 || b[4] == 0x67) c = CONTAINER_ES;
        }
        if (b[4] == 'f' && b[5] == 't' && b[6] == 'y' && b[7] == 'p') c = CONTAINER_MP4;
    }
    if (c == CONTAINER_UNKNOWN) {
        const char *e = m->file_extension;
        if (!strcmp(e, "264") || !strcmp(e, "h264") || !strcmp(e, "265") || !strcmp(e, "h265")) c = CONTAINER_ES;
        else if (!strcmp(e, "mp4") || !strcmp(e, "mov") || !strcmp(e, "m4v") || !strcmp(e, "3gp")) c = CONTAINER_MP4;
        else if (!strcmp(e, "avi")) c = CONTAINER_AVI;
        else if (!strcmp(e, "mkv") || !strcmp(e, "webm")) c = CONTAINER_MKV;
        else if (!strcmp(e, "ts") || !strcmp(e, "m2ts")) c = CONTAINER_MPEG_TS;
        else if (!strcmp(e, "mpg") || !strcmp(e, "mpeg") || !strcmp(e, "vob")) c = CONTAINER_MPEG_PS;
        else if (!strcmp(e, "wav")) c = CONTAINER_WAVE;
        else if (!strcmp(e, "mp3")) c = CONTAINER_ES_MP3;
    }
    return c;
}

void free_map(BitstreamMap_t **pm)
{
    if (!pm || !*pm) return;
    BitstreamMap_t *m = *pm;
    free(m->stream_encoder); free(m->track_title); free(m->track_languagecode); free(m->subtitles_name);
    free(m->sample_type); free(m->sample_size); free(m->sample_offset); free(m->sample_pts); free(m->sample_dts);
    free(m);
    *pm = NULL;
}

double wall_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The whole file in memory.  (Not mapped: a file that shrinks under a mapping kills the process; a short read is an error
// return.)  minivideo_parse leaves the bytes of the file it parsed last in a one-entry cache, so that the minivideo_decode
// that follows does not read 200 MB a second time (0.06 s of a 1.2-s mini_thumbnailer run); minivideo_close drops it.
struct FileBytes {
    std::unique_ptr<uint8_t[]> p;   // (not a vector: no zero fill of what fread overwrites)
    size_t n = 0;
    const uint8_t *data() const { return p.get(); }
    size_t size() const { return n; }
};

std::mutex g_last_parsed_mu;
const MediaFile_t *g_last_parsed_owner = nullptr;
std::shared_ptr<FileBytes> g_last_parsed;

std::shared_ptr<FileBytes> read_whole_file(MediaFile_t *m)
{
    if (!m->file_pointer || m->file_size <= 0) return nullptr;
    auto buf = std::make_shared<FileBytes>();
    buf->n = (size_t)m->file_size;
    buf->p.reset(new (std::nothrow) uint8_t[buf->n]);
    if (!buf->p) return nullptr;
    rewind(m->file_pointer);
    const size_t got = fread(buf->p.get(), 1, buf->n, m->file_pointer);
    rewind(m->file_pointer);
    return got == buf->n ? buf : nullptr;
}

void remember_parsed(const MediaFile_t *m, std::shared_ptr<FileBytes> buf)
{
    std::lock_guard<std::mutex> l(g_last_parsed_mu);
    g_last_parsed_owner = m;
    g_last_parsed = std::move(buf);
}

std::shared_ptr<FileBytes> take_parsed(const MediaFile_t *m, bool keep)
{
    std::lock_guard<std::mutex> l(g_last_parsed_mu);
    if (g_last_parsed_owner != m) return nullptr;
    std::shared_ptr<FileBytes> r = g_last_parsed;
    if (!keep) { g_last_parsed_owner = nullptr; g_last_parsed.reset(); }
    return r;
}

// ---- MP4: public sample map as convertTrack builds it (demuxer/mp4/mp4.c:150-500): the avcC parameter sets first,
//      then every sample of the video track, sync samples marked ----
int parse_mp4_track(MediaFile_t *m, const FileBytes &buf)
{
    mp4::VideoTrack trk;
    std::string err;
    if (!mp4::parse(buf.data(), buf.size(), trk, err)) { log_err("%s", err.c_str()); return FAILURE; }
    free_map(&m->tracks_video[0]);
    BitstreamMap_t *map = (BitstreamMap_t *)calloc(1, sizeof(BitstreamMap_t));
    if (!map) return FAILURE;
    const size_t n = trk.sps.size() + trk.pps.size() + trk.samples.size();
    map->sample_type = (uint32_t *)calloc(n, sizeof(uint32_t));
    map->sample_size = (uint32_t *)calloc(n, sizeof(uint32_t));
    map->sample_offset = (int64_t *)calloc(n, sizeof(int64_t));
    map->sample_pts = (int64_t *)calloc(n, sizeof(int64_t));
    map->sample_dts = (int64_t *)calloc(n, sizeof(int64_t));
    if (!map->sample_type || !map->sample_size || !map->sample_offset || !map->sample_pts || !map->sample_dts) {
        free_map(&map);
        return FAILURE;
    }
    map->stream_type = stream_VIDEO;
    map->stream_codec = CODEC_H264;
    map->stream_fcc = 0x61766331u; // 'avc1'
    map->sample_alignment = true;
    map->width = trk.width;
    map->height = trk.height;
    if (trk.timescale) map->duration_ms = (unsigned int)((double)trk.duration / (double)trk.timescale * 1000.0);
    size_t k = 0;
    for (const mp4::NalRef &r : trk.sps) { map->sample_type[k] = sample_VIDEO_PARAM; map->sample_offset[k] = (int64_t)r.offset; map->sample_size[k] = (uint32_t)r.size; map->sample_pts[k] = map->sample_dts[k] = -1; k++; }
    for (const mp4::NalRef &r : trk.pps) { map->sample_type[k] = sample_VIDEO_PARAM; map->sample_offset[k] = (int64_t)r.offset; map->sample_size[k] = (uint32_t)r.size; map->sample_pts[k] = map->sample_dts[k] = -1; k++; }
    for (const mp4::Sample &sm : trk.samples) {
        map->sample_type[k] = sm.sync ? sample_VIDEO_SYNC : sample_VIDEO;
        map->sample_offset[k] = (int64_t)sm.offset;
        map->sample_size[k] = (uint32_t)sm.size;
        map->stream_size += sm.size;
        if (sm.sync) map->frame_count_idr++;
        k++;
    }
    map->sample_count = (uint32_t)n;
    map->frame_count = (uint32_t)trk.samples.size();
    m->tracks_video[0] = map;
    m->tracks_video_count = 1;
    return SUCCESS;
}

// ---- demuxer/filter.c:52-215: which IDR samples to decode, in which order ----
std::vector<int> select_idrs(const mvhp_stream &s, int picture_number, int mode)
{
    const int n_idr = (int)s.idrs.size();
    std::vector<int> sel;
    if (n_idr == 0 || picture_number <= 0) return sel;
    if (picture_number > n_idr) picture_number = n_idr;
    if (mode == PICTURE_UNFILTERED) {
        for (int i = 0; i < n_idr; i++) sel.push_back(i); // decode in order until picture_number succeed (h264.c:173)
        return sel;
    }
    // ORDERED / DISTRIBUTED: keep pictures larger than (mean IDR sample size)/1.66, drop 3 % at both ends
    // when there are more than 48 of them (filter.c:100-122)
    double payload = 0;
    for (int i = 0; i < n_idr; i++) payload += (double)s.samples[s.idrs[i].sample].sample_size;
    const int threshold = (int)((payload / n_idr) / 1.66);
    const int borders = n_idr > 48 ? (int)ceil(n_idr * 0.03) : 0;
    std::vector<int> cand;
    for (int i = borders; i < n_idr - borders; i++)
        if ((int)s.samples[s.idrs[i].sample].sample_size > threshold) cand.push_back(i);
    const int T = (int)cand.size();
    if (T == 0) return sel;
    if (picture_number > T) picture_number = T;
    // filter.c:140 divides by (picture_number - 1) and crashes for one picture; one picture = first candidate
    const int jump = picture_number > 1 ? T / (picture_number - 1) : 0;
    for (int i = 0; i < picture_number; i++) {
        int k = (mode == PICTURE_ORDERED) ? i : i * jump;
        if (k > T - 1) k = T - 1; // the reference indexes past its candidate list here (filter.c:170-175)
        sel.push_back(cand[k]);
    }
    return sel;
}

// ---- MINIVIDEO_CROP=1 / MINIVIDEO_THUMBNAIL=<w>x<h> / MINIVIDEO_ROTATE=<auto or angle> / MINIVIDEO_ASPECT=1 / MINIVIDEO_COLOR=<auto or matrix> (opt-in, include/minivideo.h): the output request of the decode call.
// A box implies the crop.  false: a malformed value (the call fails before any device work; it is not ignored).
bool output_request_from_env(mvhp_output_request_t &req, std::string &why)
{
    memset(&req, 0, sizeof(req));
    if (const char *e = getenv("MINIVIDEO_CROP"))
        if (atoi(e) != 0) req.flags |= MVHP_OUTPUT_CROP;
    // MINIVIDEO_ROTATE=auto|0|90|180|270 (opt-in): "auto" = the MP4's own display rotation, an angle = that many degrees
    // clockwise whatever the file says; empty = unset
    if (const char *r = getenv("MINIVIDEO_ROTATE")) {
        if (!strcmp(r, "auto")) req.flags |= MVHP_OUTPUT_ORIENT;
        else if (!strcmp(r, "90")) req.flags |= MVHP_OUTPUT_ROTATE(1);
        else if (!strcmp(r, "180")) req.flags |= MVHP_OUTPUT_ROTATE(2);
        else if (!strcmp(r, "270")) req.flags |= MVHP_OUTPUT_ROTATE(3);
        else if (*r && strcmp(r, "0")) {
            why = std::string("MINIVIDEO_ROTATE='") + r + "' is not auto, 0, 90, 180 or 270";
            return false;
        }
    }
    // MINIVIDEO_ASPECT=1 (opt-in): the VUI's sample aspect ratio is applied -- square samples out; implies the crop.  0 and the
    // empty string = unset; anything but 0 or 1 is malformed
    if (const char *a = getenv("MINIVIDEO_ASPECT")) {
        if (!strcmp(a, "1")) req.flags |= MVHP_OUTPUT_ASPECT;
        else if (*a && strcmp(a, "0")) {
            why = std::string("MINIVIDEO_ASPECT='") + a + "' is not 0 or 1";
            return false;
        }
    }
    // MINIVIDEO_COLOR=auto|bt601|bt709|bt601-full|bt709-full (opt-in): RGB by the stream's own matrix, range and chroma siting
    // ("auto") or by a forced matrix and range; 0 and the empty string = unset
    if (const char *c = getenv("MINIVIDEO_COLOR")) {
        static const char *const names[5] = {"auto", "bt601", "bt709", "bt601-full", "bt709-full"};
        int mode = -1;
        for (int k = 0; k < 5; k++)
            if (!strcmp(c, names[k])) mode = k;
        if (mode >= 0) req.flags |= MVHP_OUTPUT_COLOR | MVHP_OUTPUT_COLOR_MODE(mode);
        else if (*c && strcmp(c, "0")) {
            why = std::string("MINIVIDEO_COLOR='") + c + "' is not auto, bt601, bt709, bt601-full or bt709-full";
            return false;
        }
    }
    const char *t = getenv("MINIVIDEO_THUMBNAIL");
    if (!t || !*t) return true;
    // decimal digits, 'x', decimal digits, nothing else; each side 2 ... 65535
    unsigned long side[2] = {0, 0};
    const char *q = t;
    bool ok = true;
    for (int k = 0; k < 2 && ok; k++) {
        int digits = 0;
        for (; *q >= '0' && *q <= '9' && digits < 6; q++, digits++) side[k] = side[k] * 10 + (unsigned long)(*q - '0');
        ok = digits > 0 && side[k] >= 2 && side[k] <= 65535 && *q == (k == 0 ? 'x' : '\0');
        if (k == 0) q++;
    }
    if (!ok) {
        why = std::string("MINIVIDEO_THUMBNAIL='") + t + "' is not <width>x<height> with both sides between 2 and 65535";
        return false;
    }
    req.flags |= MVHP_OUTPUT_CROP | MVHP_OUTPUT_BOX;
    req.box_w = (uint32_t)side[0];
    req.box_h = (uint32_t)side[1];
    return true;
}

// ---- the sink of minivideo_decode: export.c:618-767 (file naming, format fallbacks, writers) ----
// The pipeline itself (entropy threads -> H2D -> batched kernels -> D2H, frame-level work queue over every HIP
// device) is the decode engine, csrc/host/decode_engine.cpp; it calls this once per picture, in stream order.
struct ExportSink {
    const MediaFile_t *m = nullptr;
    int fmt = PICTURE_YUV420;
    const char *ext = "yuv";
    bool want_rgb = false;
    int picture_number = 1;
    int exported = 0, errors = 0;   // exported: pictures named so far (the _k of the file name)
    bool aborted = false;

    // File writers (round 3): one picture's write to the page cache is a 3-6 MB copy, 0.5 ms -- on the calling thread that
    // capped minivideo_decode at 2000 pictures/s while the pipeline delivers 3300.  The sink keeps the picture (verdict 2),
    // a small pool writes it and gives it back.  MINIVIDEO_WRITERS=0: write on the calling thread as before.
    struct Job { int seq; std::string name; int W, H; const uint8_t *yuv, *rgb; size_t file_bytes; };
    mvhp_engine_t *eng = nullptr;
    std::vector<std::thread> pool;
    std::mutex mu;
    std::condition_variable cv_job, cv_room;
    std::deque<Job> jobs;
    size_t max_jobs = 8;            // pictures queued or being written: bounds what is kept out of the engine's chunks
    size_t in_flight = 0;
    int n_writers = 0;
    bool closing = false;
    std::atomic<int> written{0}, write_errors{0};
    bool stopped_by_write_error = false;
    // MINIVIDEO_SKIP_BLANK=1: what each slot (the _k of the file name) holds after pass 1 -- its IDR, its score, its file
    struct Slot { int idr; uint32_t score; std::string name; };
    std::vector<Slot> *slots = nullptr;
    // MINIVIDEO_REPRESENTATIVE=1: the plane histograms of the slots' pictures, one per entry of `slots` (MVHP_OUTPUT_HIST); the
    // slot's score is then the histogram's own (mvhp_hist_stats), not g->reserved[1]
    std::vector<mvhp_plane_hist_t> *hists = nullptr;
    void note_slot(int seq, int idr, uint32_t score, const std::string &name)
    {
        if (!slots) return;
        if (hists) {
            const mvhp_plane_hist_t *h = mvhp_engine_picture_hist(eng, seq);
            hists->push_back(h ? *h : mvhp_plane_hist_t{});
            mvhp_luma_stats_t st;
            mvrep::hist_stats(hists->back(), st);
            score = mvblank::luma_score(st.sum, st.sumsq, st.samples);
        }
        slots->push_back(Slot{idr, score, name});
    }

    bool png_dev = false;           // MINIVIDEO_PNG=1 and fmt == PICTURE_PNG: the files are made on the device (MVHP_OUT_PNG)
    bool device_file() const { return fmt == PICTURE_JPG || png_dev; }
    // file_bytes: PICTURE_JPG under MINIVIDEO_JPEG=1 and PICTURE_PNG under MINIVIDEO_PNG=1 only -- `rgb` then is the finished
    // file (made on the device)
    int write_one(const std::string &name, int W, int H, const uint8_t *yuv, const uint8_t *rgb, size_t file_bytes) const
    {
        if (device_file()) {
            FILE *f = fopen(name.c_str(), "wb");
            if (!f) return 0;
            const bool ok = fwrite(rgb, 1, file_bytes, f) == file_bytes;
            return (fclose(f) == 0 && ok) ? 1 : 0;
        }
        if (fmt == PICTURE_PNG) return mvexport::write_png(name, rgb, W, H);
        if (fmt == PICTURE_BMP) return mvexport::write_bmp(name, rgb, W, H);
        if (fmt == PICTURE_TGA) return mvexport::write_tga(name, rgb, W, H);
        if (fmt == PICTURE_YUV444) return mvexport::write_yuv444(name, yuv, W, H);
        return mvexport::write_yuv420(name, yuv, W, H);
    }
    void start(int n, mvhp_engine_t *e)
    {
        eng = e;
        n_writers = n;
        max_jobs = (size_t)n + 4;
        for (int i = 0; i < n; i++) pool.emplace_back([this] { writer(); });
    }
    void finish()
    {
        {
            std::lock_guard<std::mutex> l(mu);
            closing = true;
        }
        cv_job.notify_all();
        for (auto &t : pool) t.join();
        pool.clear();
    }
    void writer()
    {
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> l(mu);
                cv_job.wait(l, [&] { return closing || !jobs.empty(); });
                if (jobs.empty()) return;
                j = std::move(jobs.front());
                jobs.pop_front();
            }
            if (write_one(j.name, j.W, j.H, j.yuv, j.rgb, j.file_bytes)) written++;
            else { log_err("Unable to write '%s'", j.name.c_str()); write_errors++; }
            mvhp_engine_release_picture(eng, j.seq);
            {
                std::lock_guard<std::mutex> l(mu);
                in_flight--;
            }
            cv_room.notify_one();
        }
    }

    static int call(void *user, int seq, int idr, int rc, const char *err, const mvhp_stream_params_t *p,
                    const mvhp_output_geometry_t *g, const uint8_t *yuv, const uint8_t *rgb)
    {
        (void)p;
        ExportSink &x = *static_cast<ExportSink *>(user);
        if (rc != MVHP_SUCCESS) {
            log_err("IDR %d: %s", idr, err ? err : "failed");
            if (++x.errors > 64) { x.aborted = true; return -1; }   // h264.c:181-187
            return 0;
        }
        x.errors = 0;
        // export.c:627-642, 704-708: <file_name>[_k].<ext> in the current working directory
        std::string name = x.m->file_name;
        if (x.picture_number > 1) name += "_" + std::to_string(x.exported);
        name += ".";
        name += x.ext;
        const int W = (int)g->out_w, H = (int)g->out_h;   // the coded size unless MINIVIDEO_CROP / MINIVIDEO_THUMBNAIL ask for less
        const size_t file_bytes = x.device_file() ? g->reserved[0] : 0;   // (MVHP_OUT_JPEG / _PNG: the length of the file in `rgb`)
        if (!x.pool.empty()) {
            if (x.write_errors.load() == 0) x.note_slot(seq, idr, g->reserved[1], name);
            // Writers run behind the pipeline, so a write that fails is only known later: no further picture is decoded in
            // its place (the synchronous path below does that).  Once one has failed -- a full disk does not get better --
            // decoding stops, and minivideo_decode answers FAILURE unless every wanted file was written (contract: minivideo.h).
            if (x.write_errors.load() > 0) { x.stopped_by_write_error = true; return -1; }
            {
                std::unique_lock<std::mutex> l(x.mu);
                x.cv_room.wait(l, [&] { return x.in_flight < x.max_jobs; });
                x.in_flight++;
                x.jobs.push_back(Job{seq, std::move(name), W, H, yuv, rgb, file_bytes});
            }
            x.cv_job.notify_one();
            x.exported++;
            return 2;
        }
        if (!x.write_one(name, W, H, yuv, rgb, file_bytes)) {
            log_err("Unable to write '%s'", name.c_str());
            x.errors++;
            return 0;
        }
        x.note_slot(seq, idr, g->reserved[1], name);
        x.exported++;
        x.written++;
        return 1;
    }
};

// ---- MINIVIDEO_SKIP_BLANK=1, pass 2 (include/minivideo.h; DESIGN.md 3 "Picture scores"): the alternates of the blank slots, decoded
// in one more engine call.  A slot's file is written again -- on the calling thread: two writes to one name must land in order --
// whenever mvhp_blank_choose over the scores seen so far for the slot (the primary first) moves to the new candidate.
struct AlternateSink {
    ExportSink *x = nullptr;                        // the writer of pass 1 (format, counters)
    std::vector<ExportSink::Slot> *slots = nullptr;
    std::vector<int> slot_of;                       // per picture of pass 2's order: its slot
    std::vector<std::vector<uint32_t>> scores;      // per slot: the primary's score, then its alternates' as they arrive
    uint32_t min_score = 0;
    int replaced = 0;

    static int call(void *user, int seq, int idr, int rc, const char *err, const mvhp_stream_params_t *p,
                    const mvhp_output_geometry_t *g, const uint8_t *yuv, const uint8_t *rgb)
    {
        (void)p;
        AlternateSink &a = *static_cast<AlternateSink *>(user);
        ExportSink &x = *a.x;
        if (rc != MVHP_SUCCESS) {   // a failed alternate is skipped
            log_err("IDR %d: %s", idr, err ? err : "failed");
            if (++x.errors > 64) { x.aborted = true; return -1; }   // h264.c:181-187
            return 0;
        }
        x.errors = 0;
        const int k = a.slot_of[(size_t)seq];
        std::vector<uint32_t> &sc = a.scores[(size_t)k];
        if (sc[(size_t)mvblank::choose(sc.data(), (int)sc.size(), a.min_score)] >= a.min_score) return 1;   // the slot is settled
        sc.push_back(g->reserved[1]);
        if (mvblank::choose(sc.data(), (int)sc.size(), a.min_score) != (int)sc.size() - 1) return 1;
        ExportSink::Slot &slot = (*a.slots)[(size_t)k];
        const size_t file_bytes = x.device_file() ? g->reserved[0] : 0;
        // beside the slot's file first, then renamed over it: a write that fails leaves the file of the earlier candidate whole,
        // which is what `written` counted.  The candidate is then taken out of the slot's scores again, so that a later
        // alternate is weighed against what the file holds.
        const std::string part = slot.name + ".part";
        if (!x.write_one(part, (int)g->out_w, (int)g->out_h, yuv, rgb, file_bytes) || rename(part.c_str(), slot.name.c_str()) != 0) {
            log_err("Unable to write '%s'", slot.name.c_str());
            (void)unlink(part.c_str());
            sc.pop_back();
            x.errors++;
            return 0;
        }
        slot.idr = idr;
        slot.score = g->reserved[1];
        a.replaced++;
        return 1;
    }
};

// ---- MINIVIDEO_REPRESENTATIVE=1 (include/minivideo.h; DESIGN.md 3 "Representative pictures") ----
// pass 2: the alternates of every slot, decoded for their histograms alone; the planes that come with them are not looked at
struct HistSink {
    mvhp_engine_t *eng = nullptr;
    std::vector<mvhp_plane_hist_t> hists;   // per picture of pass 2's order
    std::vector<uint8_t> have;              // ... and whether it arrived: a failed alternate is skipped
    int decoded = 0;

    static int call(void *user, int seq, int idr, int rc, const char *err, const mvhp_stream_params_t *, const mvhp_output_geometry_t *,
                    const uint8_t *, const uint8_t *)
    {
        HistSink &a = *static_cast<HistSink *>(user);
        const mvhp_plane_hist_t *h = rc == MVHP_SUCCESS ? mvhp_engine_picture_hist(a.eng, seq) : nullptr;
        if (!h) {
            log_err("IDR %d: %s", idr, err && *err ? err : "failed");
            return 0;
        }
        a.hists[(size_t)seq] = *h;
        a.have[(size_t)seq] = 1;
        a.decoded++;
        return 1;
    }
};

// pass 3: the winners that are not their slot's primary, decoded with the request and the output kind of pass 1; each file is
// written beside the slot's file and renamed over it, on the calling thread, as AlternateSink does
struct ReplaceSink {
    ExportSink *x = nullptr;
    std::vector<ExportSink::Slot> *slots = nullptr;
    std::vector<int> slot_of;               // per picture of pass 3's order: its slot
    int replaced = 0;

    static int call(void *user, int seq, int idr, int rc, const char *err, const mvhp_stream_params_t *, const mvhp_output_geometry_t *g,
                    const uint8_t *yuv, const uint8_t *rgb)
    {
        ReplaceSink &a = *static_cast<ReplaceSink *>(user);
        ExportSink &x = *a.x;
        if (rc != MVHP_SUCCESS) {   // the slot keeps its primary
            log_err("IDR %d: %s", idr, err && *err ? err : "failed");
            return 0;
        }
        ExportSink::Slot &slot = (*a.slots)[(size_t)a.slot_of[(size_t)seq]];
        const size_t file_bytes = x.device_file() ? g->reserved[0] : 0;
        const std::string part = slot.name + ".part";   // (a write that fails leaves the earlier file whole)
        if (!x.write_one(part, (int)g->out_w, (int)g->out_h, yuv, rgb, file_bytes) || rename(part.c_str(), slot.name.c_str()) != 0) {
            log_err("Unable to write '%s'", slot.name.c_str());
            (void)unlink(part.c_str());
            return 0;
        }
        slot.idr = idr;
        a.replaced++;
        return 1;
    }
};

} // namespace

extern "C" {

minivideo_EXPORT void minivideo_print_infos(void)
{
    printf("\nminivideo_print_infos()\n");
    printf("* Library version %d.%d-%d (MI355X-native H.264 intra path, gfx950)\n", minivideo_VERSION_MAJOR,
           minivideo_VERSION_MINOR, minivideo_VERSION_PATCH);
    printf("* HIP devices visible: %d\n", mvhp_device_count());
}

minivideo_EXPORT void minivideo_get_infos(int *major, int *minor, int *patch, const char **builddate, const char **buildtime)
{
    if (major) *major = minivideo_VERSION_MAJOR;
    if (minor) *minor = minivideo_VERSION_MINOR;
    if (patch) *patch = minivideo_VERSION_PATCH;
    if (builddate) *builddate = __DATE__;
    if (buildtime) *buildtime = __TIME__;
}

minivideo_EXPORT int minivideo_endianness(void)
{
    const uint32_t i = 0x01020304u;
    const uint8_t *p = (const uint8_t *)&i;
    return (p[0] == 0x04) ? 1234 : 4321;
}

minivideo_EXPORT int minivideo_open(const char *input_filepath, MediaFile_t **input_media)
{
    if (!input_filepath || !input_media) return FAILURE;
    MediaFile_t *m = (MediaFile_t *)calloc(1, sizeof(MediaFile_t));
    if (!m) return FAILURE;
    strncpy(m->file_path, input_filepath, sizeof(m->file_path) - 1);
    m->file_pointer = fopen(input_filepath, "r");
    if (!m->file_pointer) {
        log_err("Unable to open the media file: '%s'", input_filepath);
        free(m);
        *input_media = NULL;
        return FAILURE;
    }
    infos_from_path(m);
    fseek(m->file_pointer, 0, SEEK_END);
    m->file_size = (int64_t)ftell(m->file_pointer);
    rewind(m->file_pointer);
    m->container = sniff_container(m);
    *input_media = m;
    return SUCCESS;
}

minivideo_EXPORT int minivideo_parse(MediaFile_t *m, const bool extract_audio, const bool extract_video,
                                     const bool extract_subtitles)
{
    (void)extract_audio; (void)extract_video; (void)extract_subtitles;
    if (!m) { log_err("Unable to parse NULL MediaFile_t struct!"); return FAILURE; }
    if (m->file_size == 0) { log_err("Unable to parse emtpy file!"); return FAILURE; }
    if (m->container != CONTAINER_ES && m->container != CONTAINER_MP4) {
        log_err("Unable to parse container format '%s': only H.264 elementary streams and MP4/MOV are handled by this build",
                getContainerString(m->container, false));
        return FAILURE;
    }
    const double t_call = wall_s();
    std::shared_ptr<FileBytes> file = read_whole_file(m);
    if (!file) { log_err("Unable to read the media file"); return FAILURE; }
    const FileBytes &buf = *file;
    remember_parsed(m, file);
    const double t_read = wall_s();
    if (m->container == CONTAINER_MP4) return parse_mp4_track(m, buf);
    std::vector<h264::EsSample> samples;
    const bool spec = getenv("MINIVIDEO_SPEC") && atoi(getenv("MINIVIDEO_SPEC")) != 0;   // opt-in, SURVEY 8f row f4
    if ((spec ? h264::index_annexb_spec(buf.data(), buf.size(), samples) : h264::index_annexb(buf.data(), buf.size(), samples)) != h264::RC_SUCCESS) {
        log_err("No NAL Unit have been found in this bitstream!");
        return FAILURE;
    }
    free_map(&m->tracks_video[0]);
    BitstreamMap_t *map = (BitstreamMap_t *)calloc(1, sizeof(BitstreamMap_t));
    if (!map) return FAILURE;
    const size_t n = samples.size();
    map->sample_type = (uint32_t *)calloc(n, sizeof(uint32_t));
    map->sample_size = (uint32_t *)calloc(n, sizeof(uint32_t));
    map->sample_offset = (int64_t *)calloc(n, sizeof(int64_t));
    map->sample_pts = (int64_t *)calloc(n, sizeof(int64_t));
    map->sample_dts = (int64_t *)calloc(n, sizeof(int64_t));
    if (!map->sample_type || !map->sample_size || !map->sample_offset || !map->sample_pts || !map->sample_dts) {
        free_map(&map);
        return FAILURE;
    }
    map->stream_type = stream_VIDEO;
    map->stream_codec = CODEC_H264;
    map->sample_alignment = true;
    map->stream_intracoded = false;
    for (size_t i = 0; i < n; i++) {
        map->sample_type[i] = samples[i].is_idr ? sample_VIDEO_SYNC : sample_VIDEO_PARAM;
        map->sample_size[i] = (uint32_t)samples[i].sample_size;
        map->sample_offset[i] = (int64_t)samples[i].offset;
        map->sample_pts[i] = -1;
        map->stream_size += samples[i].sample_size;
        if (samples[i].is_idr) map->frame_count_idr++;
    }
    map->sample_count = (uint32_t)n;
    map->frame_count = map->frame_count_idr;
    m->tracks_video[0] = map;
    m->tracks_video_count = 1;
    if (getenv("MINIVIDEO_STATS"))
        fprintf(stderr, "[minivideo] parse call: reading the file %.3f s, indexing + sample map %.3f s\n", t_read - t_call, wall_s() - t_read);
    return SUCCESS;
}

minivideo_EXPORT int minivideo_decode(MediaFile_t *m, const char *output_directory, const int picture_format,
                                      const int picture_quality, const int picture_number,
                                      const int picture_extractionmode)
{
    (void)output_directory; // accepted and ignored, like the reference (h264.c:65)
    if (!m) { log_err("Unable to start decoding because of an empty MediaFile_t structure! Parsing failed?"); return FAILURE; }
    BitstreamMap_t *map = m->tracks_video[0];
    if (!map || map->stream_type != stream_VIDEO) { log_err("No video track to decode"); return FAILURE; }
    if (map->stream_codec != CODEC_H264) { log_err("Unable to decode given file format: no decoder available!"); return FAILURE; }
    mvhp_output_request_t req;
    {   // before any device work: a malformed switch fails the call
        std::string why;
        if (!output_request_from_env(req, why)) { log_err("%s", why.c_str()); return FAILURE; }
    }
    mvblank::Settings blank;
    {   // the same for the blank-picture switches
        std::string why;
        if (!mvblank::settings_from(getenv("MINIVIDEO_SKIP_BLANK"), getenv("MINIVIDEO_BLANK_VARIANCE"),
                                    getenv("MINIVIDEO_BLANK_ALTERNATES"), blank, why)) { log_err("%s", why.c_str()); return FAILURE; }
    }
    mvrep::Settings represent;
    {   // and for the representative-picture switches
        std::string why;
        if (!mvrep::settings_from(getenv("MINIVIDEO_REPRESENTATIVE"), getenv("MINIVIDEO_REPRESENTATIVE_ALTERNATES"), represent, why)) {
            log_err("%s", why.c_str());
            return FAILURE;
        }
    }
    mvbars::Settings trim;
    {   // and for the black-bar switches
        std::string why;
        if (!mvbars::settings_from(getenv("MINIVIDEO_TRIM"), getenv("MINIVIDEO_TRIM_LEVEL"), getenv("MINIVIDEO_TRIM_PROBES"), trim, why)) {
            log_err("%s", why.c_str());
            return FAILURE;
        }
    }

    // The engine (HIP runtime, one context per device, its thread pools: 0.2-0.5 s in a fresh process) comes up on a thread
    // of its own while this one reads and indexes the file.
    const double t_call = wall_s();
    struct EngineStart {
        mvhp_engine_t *eng = nullptr;
        int rc = MVHP_FAILURE;
        double seconds = 0;
        std::thread th;
        bool joined = false;
        void join() { if (!joined) { th.join(); joined = true; } }
        ~EngineStart()
        {
            join();
            const double t = wall_s();
            if (eng) mvhp_engine_destroy(eng);
            if (getenv("MINIVIDEO_STATS")) fprintf(stderr, "[minivideo] engine torn down in %.3f s\n", wall_s() - t);
        }
    } es;
    es.th = std::thread([&es] { const double t = wall_s(); es.rc = mvhp_engine_create(nullptr, &es.eng); es.seconds = wall_s() - t; });

    // the bytes minivideo_parse read, once: the cache is emptied here (a second minivideo_decode of the same MediaFile_t reads
    // the file again -- a 200-MB stream does not stay resident until minivideo_close)
    std::shared_ptr<FileBytes> file = take_parsed(m, false);
    if (!file) file = read_whole_file(m);
    if (!file) { log_err("Unable to read the media file"); return FAILURE; }
    const FileBytes &buf = *file;
    const double t_read = wall_s();
    mvhp_stream s;
    s.data = buf.data();
    s.size = buf.size();
    // opt-in: index and reconstruct by the standard instead of by the reference's quirks
    if (const char *e = getenv("MINIVIDEO_SPEC")) s.spec = atoi(e) != 0;
    // opt-in, independent of the above: the in-loop deblocking filter (clause 8.7), which the reference does not apply
    if (const char *e = getenv("MINIVIDEO_DEBLOCK")) s.deblock = atoi(e) != 0;
    std::string err;
    const int brc = (m->container == CONTAINER_MP4) ? s.build_mp4(err) : s.build(err);
    if (brc != h264::RC_SUCCESS) { log_err("%s", err.c_str()); return FAILURE; }

    // idr_filtering (filter.c:52-92)
    int wanted = picture_number;
    if ((int)s.idrs.size() < wanted) wanted = (int)s.idrs.size();
    if (wanted <= 0) { log_err("No picture to decode after filtering!"); return FAILURE; }
    std::vector<int> order = select_idrs(s, wanted, picture_extractionmode);
    if (order.empty()) { log_err("No picture to decode after filtering!"); return FAILURE; }
    if (picture_extractionmode != PICTURE_UNFILTERED && (int)order.size() < wanted) wanted = (int)order.size();

    // export.c:644-690: format fallbacks of a build with stb_image_write only (ENABLE_JPEG = ENABLE_PNG = 0)
    // opt-in (MINIVIDEO_JPEG=1, outside the parity contract): PICTURE_JPG is written as JPEG, coded on the device from the planes as
    // export.c:341-430 does with libjpeg (jpeg_set_quality(picture_quality), 2x2 / 1x1 / 1x1, no colour conversion)
    const bool jpeg = picture_format == PICTURE_JPG && getenv("MINIVIDEO_JPEG") && atoi(getenv("MINIVIDEO_JPEG")) != 0;
    int fmt = picture_format;
    if (fmt == PICTURE_JPG && !jpeg) fmt = PICTURE_PNG;
    const char *ext = "yuv";
    if (fmt == PICTURE_JPG) ext = "jpg";
    else if (fmt == PICTURE_PNG) ext = "png";
    else if (fmt == PICTURE_BMP) ext = "bmp";
    else if (fmt == PICTURE_TGA) ext = "tga";
    const bool want_rgb = (fmt == PICTURE_PNG || fmt == PICTURE_BMP || fmt == PICTURE_TGA);
    // opt-in (MINIVIDEO_PNG=1, outside the parity contract): whenever the format resolves to PNG the files are compressed PNG made on
    // the device from the RGB (DESIGN.md 3 "PNG output") instead of the host writer's stored ones; only their bytes come back
    const bool png_dev = fmt == PICTURE_PNG && getenv("MINIVIDEO_PNG") && atoi(getenv("MINIVIDEO_PNG")) != 0;

    const double t_indexed = wall_s();
    es.join();
    if (es.rc != MVHP_SUCCESS) return FAILURE;   // (the reason has been printed)
    mvhp_engine_t *eng = es.eng;
    const double t_engine = wall_s();
    ExportSink sink;
    sink.m = m;
    sink.fmt = fmt;
    sink.ext = ext;
    sink.want_rgb = want_rgb;
    sink.png_dev = png_dev;
    sink.picture_number = picture_number;
    sink.eng = eng;
    {   // file writers: two per sixteen cores keep up with the pipeline on the raw formats (0.5 ms of copying per picture);
        // the entropy threads need the rest.  PNG and TGA cost more CPU per picture than entropy decoding does (two checksums
        // over 6.3 MB, 7 ms; the run-length coder, 5 ms; against 3.7 ms): half as many writers as cores -- they sleep when
        // there is nothing to write, and the scheduler shares the cores between the two kinds of work.
        const int cores = mvengine::effective_cores();
        int writers = ((fmt == PICTURE_PNG && !png_dev) || fmt == PICTURE_TGA) ? std::min(16, std::max(2, cores / 2))
                      : (fmt == PICTURE_BMP)                         ? std::min(8, std::max(2, cores / 4))   // (4 ms: the B-G-R swap)
                                                                     : std::min(4, std::max(1, cores / 8));   // (finished files too)
        if (const char *e = getenv("MINIVIDEO_WRITERS")) writers = std::max(0, std::min(16, atoi(e)));
        if (wanted < 4) writers = 0;
        if (writers > 0) sink.start(writers, eng);
    }
    mvhp_decode_stats_t st;
    // decodes in order until `wanted` pictures have been written (h264.c:173-179) or 64 errors in a row (h264.c:181-187)
    // RGB formats are written from the RGB picture alone: the planes stay on the device
    // JPEG files come back finished: only their bytes are downloaded and written
    // MINIVIDEO_COLOR is about RGB: with planes or JPEG files the request is the one without it
    if (!want_rgb) req.flags &= ~(MVHP_OUTPUT_COLOR | MVHP_OUTPUT_COLOR_MODE_MASK);
    if (jpeg) req.reserved = MVHP_JPEG_REQUEST(std::min(100, std::max(1, picture_quality)), 0);
    // opt-in (MINIVIDEO_SKIP_BLANK=1, outside the parity contract): the same call with every picture's score, pass 1 of 2
    std::vector<ExportSink::Slot> slots;
    // opt-in (MINIVIDEO_REPRESENTATIVE=1, outside the parity contract): the same call with every picture's plane histograms, pass 1
    // of 3.  With both switches the histograms serve both: their own score is the blank score, and blank skipping's pass is not run
    std::vector<mvhp_plane_hist_t> hists;
    if (represent.on) { req.flags |= MVHP_OUTPUT_HIST; sink.slots = &slots; sink.hists = &hists; }
    else if (blank.on) { req.flags |= MVHP_OUTPUT_SCORE; sink.slots = &slots; }
    const int out_kind = jpeg ? MVHP_OUT_JPEG : png_dev ? MVHP_OUT_PNG : want_rgb ? MVHP_OUT_RGB_ONLY : 0;
    if (trim.on) {
        // opt-in (MINIVIDEO_TRIM=1, outside the parity contract): black bars are a property of the stream, so a few pictures of
        // the list are probed first -- order[floor(k size / P)], k = 0 .. P - 1, the first picture among them -- in one call that
        // only collects their content boxes; the union of the boxes travels with the stream and MVHP_OUTPUT_TRIM applies it to
        // every picture of the calls below alike.  The probes are entropy-decoded twice: at most MINIVIDEO_TRIM_PROBES pictures
        // per call.  The union is commutative and the probes are a function of the list: the files do not depend on batch
        // sizes, threads or contexts.  A probe that fails to decode is simply missing.
        struct ProbeSink {
            std::vector<mvhp_luma_bars_t> boxes;
            static int call(void *user, int, int, int rc, const char *, const mvhp_stream_params_t *, const mvhp_output_geometry_t *g,
                            const uint8_t *, const uint8_t *)
            {
                if (rc != MVHP_SUCCESS || !g) return 0;
                mvhp_luma_bars_t b{};
                b.x = g->reserved[0] & 0xffffu; b.y = g->reserved[0] >> 16;
                b.w = g->reserved[1] & 0xffffu; b.h = g->reserved[1] >> 16;
                ((ProbeSink *)user)->boxes.push_back(b);
                return 1;
            }
        } probe;
        const double t_probe = wall_s();
        const size_t size = order.size(), P = std::min<size_t>((size_t)trim.probes, size);
        std::vector<int> probes;
        for (size_t k = 0; k < P; k++) probes.push_back(order[k * size / P]);
        mvhp_output_request_t preq{};
        preq.flags = MVHP_OUTPUT_CROP | MVHP_OUTPUT_BARS;
        preq.reserved = MVHP_BARS_REQUEST(trim.level);
        mvhp_decode_stats_t pst;
        memset(&pst, 0, sizeof(pst));
        (void)mvhp_engine_decode_ex(eng, &s, probes.data(), (int)P, (int)P, 0, &preq, ProbeSink::call, &probe, &pst);
        mvhp_luma_bars_t u{};
        const int with_content = mvhp_bars_union(probe.boxes.data(), (int)probe.boxes.size(), &u);
        (void)mvhp_stream_set_trim(&s, with_content ? &u : nullptr);
        req.flags |= MVHP_OUTPUT_TRIM;
        if (getenv("MINIVIDEO_STATS")) {
            mvhp_output_geometry_t crop{}, cut{};
            const int applied = mvhp_stream_crop(&s, order[0], &crop) == MVHP_SUCCESS && mvhp_trim_rect(&crop, &u, &cut);
            fprintf(stderr, "[minivideo] black bars: %d probes listed, %d decoded, %d with content above %d; union %u,%u %ux%u, %s "
                            "(first picture: %u,%u %ux%u), %.3f s\n", (int)P, (int)probe.boxes.size(), with_content, trim.level,
                    u.x, u.y, u.w, u.h, applied ? "applied" : "not applied", cut.crop_x, cut.crop_y, cut.crop_w, cut.crop_h,
                    wall_s() - t_probe);
        }
    }
    (void)mvhp_engine_decode_ex(eng, &s, order.data(), (int)order.size(), wanted, out_kind,
                                (req.flags || jpeg) ? &req : nullptr, ExportSink::call, &sink, &st);   // (MVHP_OUT_PNG has no parameters)
    sink.finish();   // (every kept picture is back: mvhp_engine_decode waits for that)
    if (represent.on && !sink.aborted && sink.write_errors.load() == 0 && hists.size() == slots.size()) {
        // pass 2: the alternates of every slot -- the IDRs strictly between its picture and the next slot's, at most
        // MINIVIDEO_REPRESENTATIVE_ALTERNATES -- in one call that asks for planes of the rectangle pass 1 counted over (the crop
        // where pass 1 crops, trims, scales or squares; no box, turn, colour or file coding) and keeps only the histograms.
        // Slots, alternates, histograms and the choice are functions of the stream and the switches alone: the files do not
        // depend on batch sizes, threads or contexts.
        std::vector<int> idrs, order2, first_of;   // first_of[k]: where slot k's alternates start in order2
        for (const ExportSink::Slot &sl : slots) idrs.push_back(sl.idr);
        for (int k = 0; k < (int)slots.size(); k++) {
            first_of.push_back((int)order2.size());
            for (int i : mvblank::alternates(idrs, (int)s.idrs.size(), represent.alternates, k)) order2.push_back(i);
        }
        first_of.push_back((int)order2.size());
        HistSink hs;
        hs.eng = eng;
        hs.hists.resize(order2.size());
        hs.have.assign(order2.size(), 0);
        mvhp_decode_stats_t st2, st3;
        memset(&st2, 0, sizeof(st2));
        memset(&st3, 0, sizeof(st3));
        if (!order2.empty()) {
            mvhp_output_request_t req2{};
            req2.flags = MVHP_OUTPUT_HIST | (req.flags & MVHP_OUTPUT_TRIM);
            if (req.flags & (MVHP_OUTPUT_CROP | MVHP_OUTPUT_BOX | MVHP_OUTPUT_ASPECT | MVHP_OUTPUT_TRIM)) req2.flags |= MVHP_OUTPUT_CROP;
            (void)mvhp_engine_decode_ex(eng, &s, order2.data(), (int)order2.size(), (int)order2.size(), 0, &req2, HistSink::call, &hs, &st2);
        }
        // the choice, per slot: the primary first, then the alternates that arrived.  With MINIVIDEO_SKIP_BLANK=1 a candidate is
        // eligible when its score reaches the threshold; a slot without an eligible candidate goes to the blank policy's rule.
        ReplaceSink rs;
        rs.x = &sink;
        rs.slots = &slots;
        std::vector<int> order3;
        for (int k = 0; k < (int)slots.size() && !order2.empty(); k++) {
            std::vector<mvhp_plane_hist_t> cand{hists[(size_t)k]};
            std::vector<int> cand_idr{slots[(size_t)k].idr};
            for (int i = first_of[(size_t)k]; i < first_of[(size_t)k + 1]; i++)
                if (hs.have[(size_t)i]) { cand.push_back(hs.hists[(size_t)i]); cand_idr.push_back(order2[(size_t)i]); }
            if (cand.size() < 2) continue;
            std::vector<uint8_t> eligible;
            std::vector<uint32_t> scores;
            for (const mvhp_plane_hist_t &h : cand) {
                mvhp_luma_stats_t ls;
                mvrep::hist_stats(h, ls);
                scores.push_back(mvblank::luma_score(ls.sum, ls.sumsq, ls.samples));
                eligible.push_back(scores.back() >= blank.min_score ? 1 : 0);
            }
            int w = mvrep::choose(cand.data(), (int)cand.size(), blank.on ? eligible.data() : nullptr);
            if (w < 0) w = mvblank::choose(scores.data(), (int)scores.size(), blank.min_score);
            if (w > 0) { order3.push_back(cand_idr[(size_t)w]); rs.slot_of.push_back(k); }
        }
        // pass 3: the winners that are not primaries, with the request and the output kind of pass 1, written over the slots' files
        if (!order3.empty()) {
            mvhp_output_request_t req3 = req;
            req3.flags &= ~MVHP_OUTPUT_HIST;
            (void)mvhp_engine_decode_ex(eng, &s, order3.data(), (int)order3.size(), (int)order3.size(), out_kind,
                                        (req3.flags || jpeg) ? &req3 : nullptr, ReplaceSink::call, &rs, &st3);
        }
        if (getenv("MINIVIDEO_STATS")) {
            std::string l2, l3;
            for (int i : order2) l2 += " " + std::to_string(i);
            for (int i : order3) l3 += " " + std::to_string(i);
            fprintf(stderr, "[minivideo] representative pictures: %d slots, %d candidates listed, %d decoded, %d files replaced, "
                            "pass 2 %.3f s (%u entropy-decoded), pass 3 %.3f s (%u entropy-decoded)\n", (int)slots.size(), (int)order2.size(),
                    hs.decoded, rs.replaced, st2.wall_s, st2.pictures_issued, st3.wall_s, st3.pictures_issued);
            fprintf(stderr, "[minivideo] representative pictures: pass 2 order:%s; pass 3 order:%s\n", l2.empty() ? " none" : l2.c_str(),
                    l3.empty() ? " none" : l3.c_str());
        }
    }
    if (blank.on && !represent.on && !sink.aborted && sink.write_errors.load() == 0) {
        // pass 2: the alternates of every slot whose picture scores below the threshold -- the IDRs between it and the next
        // slot's picture (select_idrs' size filter does not apply to them).  Slots, scores and alternates are functions of
        // the stream and the switches alone, and the sink sees pictures in the order of the list: the files do not depend on
        // batch sizes, threads or contexts.
        AlternateSink alt;
        alt.x = &sink;
        alt.slots = &slots;
        alt.min_score = blank.min_score;
        std::vector<int> idrs, order2;
        for (const ExportSink::Slot &sl : slots) { idrs.push_back(sl.idr); alt.scores.push_back({sl.score}); }
        int n_blank = 0;
        for (int k = 0; k < (int)slots.size(); k++) {
            if (slots[(size_t)k].score >= blank.min_score) continue;
            n_blank++;
            for (int i : mvblank::alternates(idrs, (int)s.idrs.size(), blank.alternates, k)) { order2.push_back(i); alt.slot_of.push_back(k); }
        }
        mvhp_decode_stats_t st2;
        memset(&st2, 0, sizeof(st2));
        if (!order2.empty())
            (void)mvhp_engine_decode_ex(eng, &s, order2.data(), (int)order2.size(), (int)order2.size(), out_kind, &req,
                                        AlternateSink::call, &alt, &st2);
        if (getenv("MINIVIDEO_STATS"))
            fprintf(stderr, "[minivideo] blank pictures: %d of %d slots score below %u; second pass: %d alternates listed, %u "
                            "entropy-decoded, %d files replaced, %.3f s\n", n_blank, (int)slots.size(), blank.min_score,
                    (int)order2.size(), st2.pictures_issued, alt.replaced, st2.wall_s);
    }
    if (getenv("MINIVIDEO_STATS")) {
        fprintf(stderr, "[minivideo] decode call: reading the file %.3f s, indexing %.3f s, engine up after %.3f s (its thread took "
                        "%.3f s), decode %.3f s, %d file writers\n", t_read - t_call, t_indexed - t_read, t_engine - t_call, es.seconds,
                wall_s() - t_engine, (int)sink.n_writers);
        fprintf(stderr, "[minivideo] decode: %u pictures entropy-decoded, %u written, %u failed, %u launches (largest %u pictures), "
                        "%u contexts, %u host threads, %.3f s (first picture after %.3f s; page-locking %.3f s for %.2f GB, device "
                        "allocations %.3f s for %.2f GB, first launches %.3f s; entropy threads busy %.3f s, H2D %.3f s, kernels %.3f s, "
                        "D2H %.3f s for %.3f GB, sink %.3f s; %u launches with the output-geometry pass)\n", st.pictures_issued, st.pictures_ok, st.pictures_failed, st.batches,
                st.max_batch_pictures, st.contexts, st.host_threads, st.wall_s, st.first_picture_s, st.host_alloc_s,
                st.host_alloc_bytes / 1e9, st.dev_alloc_s, st.dev_alloc_bytes / 1e9, st.first_launch_s, st.entropy_busy_s, st.h2d_s,
                st.kernel_s, st.d2h_s, st.d2h_bytes / 1e9, st.sink_s, st.geometry_launches);
    }
    if (sink.aborted) return FAILURE;
    if (sink.write_errors.load() > 0 && sink.written.load() < wanted) return FAILURE;   // files are missing because writes failed
    return sink.written.load() > 0 ? SUCCESS : FAILURE;   // all wanted pictures, or the stream ended after the last good IDR
}

minivideo_EXPORT int minivideo_extract(MediaFile_t *m, const char *output_directory, const bool extract_audio,
                                       const bool extract_video, const bool extract_subtitles, const int output_format)
{
    (void)m; (void)output_directory; (void)extract_audio; (void)extract_video; (void)extract_subtitles; (void)output_format;
    log_err("minivideo_extract: elementary-stream re-export is not part of this build (muxer/ is out of scope)");
    return FAILURE;
}

minivideo_EXPORT int minivideo_close(MediaFile_t **pm)
{
    int retcode = SUCCESS;
    if (pm && *pm) {
        MediaFile_t *m = *pm;
        (void)take_parsed(m, false);
        if (m->file_pointer && fclose(m->file_pointer) != 0) retcode = FAILURE;
        for (int i = 0; i < 16; i++) { free_map(&m->tracks_audio[i]); free_map(&m->tracks_video[i]); free_map(&m->tracks_subt[i]); }
        free(m);
        *pm = NULL;
    }
    return retcode;
}

minivideo_EXPORT const char *getContainerString(ContainerFormat_e c, bool long_description)
{
    switch (c) {
    case CONTAINER_AVI: return long_description ? "AVI 'Audio Video Interleave'" : "AVI";
    case CONTAINER_MKV: return long_description ? "Matroska" : "MKV";
    case CONTAINER_MP4: return long_description ? "ISO Base Media format (MOV, MP4, ...)" : "MP4";
    case CONTAINER_MPEG_PS: return long_description ? "MPEG 'Program Stream'" : "MPEG-PS";
    case CONTAINER_MPEG_TS: return long_description ? "MPEG 'Transport Stream'" : "MPEG-TS";
    case CONTAINER_WAVE: return long_description ? "WAVE 'Waveform Audio File Format'" : "WAVE";
    case CONTAINER_ES: return long_description ? "Undefined 'Elementary Stream'" : "ES";
    case CONTAINER_ES_MP3: return long_description ? "MP3 'Elementary Stream'" : "MP3 ES";
    default: return long_description ? "Unknown container format" : "UNKNOWN";
    }
}

minivideo_EXPORT const char *getCodecString(StreamType_e type, AVCodec_e codec, bool long_description)
{
    (void)type;
    if (codec == CODEC_H264) return long_description ? "H.264 (MPEG-4 Part 10 'Advanced Video Coding')" : "H.264";
    return long_description ? "Unknown codec" : "UNKNOWN";
}

minivideo_EXPORT const char *getPictureString(PictureFormat_e p, bool long_description)
{
    (void)long_description;
    switch (p) {
    case PICTURE_BMP: return "BMP";
    case PICTURE_JPG: return "JPG";
    case PICTURE_PNG: return "PNG";
    case PICTURE_WEBP: return "WebP";
    case PICTURE_TGA: return "TGA";
    case PICTURE_YUV444: return "YCbCr 4:4:4";
    case PICTURE_YUV420: return "YCbCr 4:2:0";
    default: return "UNKNOWN";
    }
}

minivideo_EXPORT AVCodec_e getCodecFromFourCC(const uint32_t fcc)
{
    // big-endian FourCC words as the reference builds them (fourcc.h): 'avc1', 'AVC1', 'h264', 'H264', 'x264', 'X264'
    switch (fcc) {
    case 0x61766331u: case 0x41564331u: case 0x68323634u: case 0x48323634u: case 0x78323634u: case 0x58323634u:
        return CODEC_H264;
    default: return CODEC_UNKNOWN;
    }
}

} // extern "C"
