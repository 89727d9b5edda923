// recon_kernels.h -- launch interface between the C-ABI layer and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "minivideo_hotpath.h"

namespace mvhp {

struct ReconArgs {
    const uint8_t *packed;   // n_frames * W*H * 800 B packed macroblock records
    uint8_t       *yuv;      // n_frames * W*H * 384 B planar Y|Cb|Cr
    uint8_t       *rgb;      // n_frames * W*H * 768 B RGB8 written by the fused colour epilogue, or NULL
    uint32_t      *err;      // device word: bit0 = dependency wait timed out
    int            width_mbs, height_mbs;
    int            cqp_off_cb, cqp_off_cr;
    int            n_frames;
    int            dc_shift_from;   // Intra16x16 luma DC takes the left-shift branch from this qP on: 37 = the reference's
                                    // `qP > 36` (h264_transform.c:797), 36 = the standard (MVHP_PARAM_SPEC_LUMA_DC)
    // SURVEY 8f row f4 (MVHP_STREAM_SPEC streams; the one-picture-per-workgroup kernel only -- the launcher routes there):
    int            slices;          // MVHP_PARAM_SLICES: mvhp_mb_header_t::unavail is honoured
    int            scaling;         // MVHP_PARAM_SCALING: weights[] below instead of Flat_4x4_16 / Flat_8x8_16
    uint8_t        weights[112];    // scaling4[3][16] | scaling8[64], raster order
    // Wide launches (launch_recon_wide / launch_recon_quad_wide): a picture's macroblock rows are spread over several
    // workgroups ("bands" of NW consecutive rows), so that a handful of pictures fills the chip.
    uint32_t      *wide_ticket;     // device counter; a workgroup's unit (picture, band) = atomicAdd(ticket, 1) - wide_base:
                                    // units are taken in the order workgroups START, so the band a workgroup waits for is
                                    // always held by a workgroup that is already running (no assumption on dispatch order)
    uint32_t       wide_base;       // value of *wide_ticket when this launch starts (the counter is never reset)
    uint32_t       wide_epoch;      // tag of this launch's seam granules (never 0, differs from every tag left in `seam`)
    unsigned long long *seam;       // [picture][seam = band boundary][macroblock column][8] granules {bottom-row dword, tag}:
                                    // the last row of a band hands its bottom samples (16 luma + 8 Cb + 8 Cr per column) to the
                                    // first row of the next band, which runs on another CU
};

// granules per macroblock column of a seam, and their size
constexpr int SEAM_GRANULES = 8;
inline size_t recon_wide_seam_bytes(int width_mbs, int height_mbs, int n_frames, int nw)
{
    const int bands = (height_mbs + nw - 1) / nw;
    return (size_t)n_frames * (size_t)(bands > 1 ? bands - 1 : 0) * width_mbs * SEAM_GRANULES * sizeof(unsigned long long);
}

struct ExpandArgs {
    const uint8_t *compact;  // n_pictures compact pictures, `stride` bytes apart
    size_t         stride;
    uint8_t       *packed;   // n_pictures * mbs * 800 B packed records (output)
    int            mbs, n_pictures;
};

struct ColorArgs {
    const uint8_t *yuv;
    uint8_t       *rgb;
    int            width_mbs, height_mbs, n_frames;
};

// Every launcher: a.n_frames pictures with nw waves per workgroup (the banded forms: nw rows per band); hipErrorInvalidValue
// for an nw the kernel is not built for (launch_plan.hip: kernel_form) or, banded forms, without ticket counter / epoch / seams.
size_t     recon_lds_bytes(int width_mbs, int nw);
hipError_t launch_recon(const ReconArgs &a, int nw, hipStream_t stream);
// the same kernel with a picture's rows in bands of `nw` (4) over several workgroups (wide_* and seam of ReconArgs set)
hipError_t launch_recon_wide(const ReconArgs &a, int nw, hipStream_t stream);
// four pictures per workgroup, 16 lanes per picture (recon_quad.hip)
size_t     recon_quad_lds_bytes(int width_mbs, int nw);
hipError_t launch_recon_quad(const ReconArgs &a, int nw, hipStream_t stream);
// ... in bands of `nw` (4 or 8) rows over several workgroups (seams sized for 4 * ceil(n_frames / 4) pictures)
hipError_t launch_recon_quad_wide(const ReconArgs &a, int nw, hipStream_t stream);
// four pictures per wavefront in bands of four rows, three wavefronts per row (recon_pipe.hip); seams as the wide form with nw = 4
size_t     recon_pipe_lds_bytes(int width_mbs, int rows);
hipError_t launch_recon_pipe(const ReconArgs &a, int rows, hipStream_t stream);   // rows per band: 1, 2 or 4
// the same pipeline with one picture per wavefront (recon_pipe1.hip); handles slices / scaling matrices
size_t     recon_pipe1_lds_bytes(int width_mbs, int rows);
hipError_t launch_recon_pipe1(const ReconArgs &a, int rows, hipStream_t stream);
// eight pictures per workgroup, 8 lanes per picture (recon_oct.hip)
size_t     recon_oct_lds_bytes(int width_mbs, int nw);
hipError_t launch_recon_oct(const ReconArgs &a, int nw, hipStream_t stream);
hipError_t launch_color(const ColorArgs &a, hipStream_t stream);
hipError_t launch_expand(const ExpandArgs &a, hipStream_t stream);

// the deblocking filter (deblock.hip): in place on the planes, one workgroup of `nw` (4 or 16) wavefronts per picture
struct DeblockArgs {
    const uint8_t *packed;   // the pictures' packed records (headers only are read)
    uint8_t       *yuv;      // n_frames reconstructed pictures, filtered in place
    uint32_t      *err;      // device word: bit 2 = row wait timed out
    int            width_mbs, height_mbs, n_frames;
    int            cqp_off_cb, cqp_off_cr;
};
size_t     deblock_lds_bytes(int width_mbs, int nw);
int        deblock_waves(int n_frames);
hipError_t launch_deblock(const DeblockArgs &a, int nw, hipStream_t stream);

// the output-geometry pass (resample.hip): coded planes -> cropped / resampled planes and / or RGB, one workgroup per
// (picture, band of `band` chroma output rows = 2 * band luma rows)
struct ResampleArgs {
    const uint8_t *src;      // n_frames coded pictures, planar Y | Cb | Cr, 16-byte aligned
    uint8_t       *yuv;      // n_frames output pictures (ow x oh planes) or NULL
    uint8_t       *rgb;      // n_frames output RGB pictures or NULL
    int            width_mbs, height_mbs, n_frames;
    int            cx, cy, cw, ch;   // luma crop rectangle (even)
    int            ow, oh;           // output size (even, <= cw / ch)
    int            band;             // chroma output rows per workgroup
};
size_t     resample_lds_bytes(int cw, int ow, int band);
hipError_t launch_resample(const ResampleArgs &a, hipStream_t stream);
// crop only (ow == cw, oh == ch) as a copy from global memory to global memory (crop_copy.hip): the same bytes, no LDS, any width
hipError_t launch_crop_copy(const ResampleArgs &a, hipStream_t stream);

// display orientation (orient.hip): a rectangle of w x h of every source picture -> the picture turned by `turns` quarter turns
// (clockwise), as planes and / or the RGB of the turned planes; the output is h x w for odd turns
struct OrientArgs {
    const uint8_t *src;          // n source pictures, frame_bytes apart, 4-byte aligned
    const uint8_t *src_end;      // end of the last one, rounded down to a dword boundary (nothing behind it is read)
    size_t         frame_bytes;
    size_t         y_off, cb_off, cr_off;   // of the rectangle's first sample of each plane inside a source picture
    int            pitch;        // of the source's luma plane (even; chroma: half of it)
    int            w, h;         // the rectangle (even, at least 2)
    int            turns;        // 0 .. 3
    int            n;
    int            band;         // 0 and 2 turns: chroma output rows per workgroup
    uint8_t       *yuv, *rgb;    // n output pictures each, dense, 4-byte aligned; either may be NULL
};
hipError_t launch_orient(const OrientArgs &a, hipStream_t stream);

// colour conversion (color_convert.hip): n dense planar pictures of w x h -> n dense RGB8 pictures, by matrix / range
// coefficients and a chroma siting (include/minivideo_hotpath.h "Colour conversion")
struct ColorConvertArgs {
    const uint8_t *yuv;          // n pictures, w * h * 3 / 2 apart, 4-byte aligned
    const uint8_t *yuv_end;      // end of the last one, rounded down to a dword boundary (nothing behind it is read)
    uint8_t       *rgb;          // n pictures, w * h * 3 apart, 4-byte aligned
    int            w, h, n;      // even sides, 2 .. 16384
    int            siting;       // MVHP_CHROMA_*
    int            band;         // chroma rows per workgroup (launch_color_convert lowers it to what the LDS holds)
    int            ymul, yoff;   // 16 * cy, and the luma offset
    int            crv, cbu, gcb, gcr;
};
hipError_t launch_color_convert(const ColorConvertArgs &a, hipStream_t stream);

// baseline JPEG from planar pictures (jpeg_encode.hip): DCT + quantisation, count, scans, write, headers
struct JpegArgs {
    const uint8_t     *yuv;      // n pictures, planar Y | Cb | Cr of w x h
    int                n, w, h;  // w, h even, 2 .. 65534
    int                quality;  // clamped to 1 .. 100
    int                restart;  // MCUs per restart interval, 1 .. 65535
    int                stages;   // MVHP_JPEG_STAGE_*
    uint8_t           *blob;     // 16-byte aligned
    size_t             cap;
    mvhp_jpeg_entry_t *table;    // n entries
    uint8_t           *scratch;  // jpeg_scratch_bytes(), 16-byte aligned
};
size_t     jpeg_scratch_bytes(const JpegArgs &a);
hipError_t launch_jpeg_encode(const JpegArgs &a, hipStream_t stream);
void       jpeg_quant_tables(int quality, uint8_t out[128]);
void       jpeg_header(int w, int h, int quality, int restart, uint8_t out[MVHP_JPEG_HEADER_BYTES]);

// PNG files from dense RGB8 pictures (png_encode.hip): filter choice + histogram + code lengths, scans, write, headers
struct PngArgs {
    const uint8_t     *rgb;      // n pictures of w x h, RGB8, dense, 4-byte aligned
    int                n, w, h;  // w, h even; 3 w + 1 <= 65535
    int                stages;   // MVHP_PNG_STAGE_*
    uint8_t           *blob;     // 16-byte aligned
    size_t             cap;
    mvhp_png_entry_t  *table;    // n entries
    uint8_t           *scratch;  // png_scratch_bytes(), 16-byte aligned
};
size_t     png_scratch_bytes(const PngArgs &a);
hipError_t launch_png_encode(const PngArgs &a, hipStream_t stream);
void       png_header(int w, int h, uint8_t out[MVHP_PNG_HEADER_BYTES]);
// (png_segment_rows() and png_max_bytes(): csrc/host/png_format.h, host arithmetic the decode engine shares)

// picture scores (luma_stats.hip): sum and sum of squares of the luma samples of one rectangle of every picture
struct LumaStatsArgs {
    const uint8_t     *src;          // n coded pictures, 16-byte aligned
    size_t             frame_bytes;  // from one picture to the next (a multiple of 16)
    int                n;
    int                pitch;        // of the luma plane, a multiple of 16
    int                cx, cy, cw, ch;   // the rectangle, inside the picture, cw and ch at least 1
    int                band;         // luma rows per workgroup
    mvhp_luma_stats_t *stats;        // n records, 8-byte aligned
};
hipError_t launch_luma_stats(const LumaStatsArgs &a, hipStream_t stream);

// black bars (luma_bars.hip): the box of the content rows and columns of one rectangle of every picture
struct LumaBarsArgs {
    const uint8_t     *src;          // n coded pictures, 16-byte aligned
    size_t             frame_bytes;  // from one picture to the next (a multiple of 16)
    int                n;
    int                pitch;        // of the luma plane, a multiple of 16
    int                cx, cy, cw, ch;   // the rectangle, inside the picture, cw and ch at least 1
    int                band;         // luma rows per workgroup of the counting pass
    int                level;        // 1 .. 254: a sample is bright when it is above
    uint32_t          *scratch;      // luma_bars_scratch_bytes(), 4-byte aligned
    uint32_t          *cols, *rows;  // (set by the launch function: the two parts of scratch)
    mvhp_luma_bars_t  *bars;         // n records, 8-byte aligned
};
size_t     luma_bars_scratch_bytes(const LumaBarsArgs &a);
hipError_t launch_luma_bars(const LumaBarsArgs &a, hipStream_t stream);

// representative pictures (plane_hist.hip): the histograms of the three planes over one rectangle of every picture
struct PlaneHistArgs {
    const uint8_t     *src;          // n coded pictures, 16-byte aligned
    size_t             frame_bytes;  // from one picture to the next (a multiple of 16)
    int                n;
    int                pitch;        // of the luma plane, a multiple of 16 (the chroma planes: half of it)
    int                rows;         // of the luma plane (the chroma planes follow it: Cb at pitch * rows, Cr a quarter further)
    int                cx, cy, cw, ch;   // the luma rectangle, inside the picture, all even, cw and ch at least 2
    int                band;         // luma rows per workgroup
    mvhp_plane_hist_t *hist;         // n records, 16-byte aligned
};
hipError_t launch_plane_hist(const PlaneHistArgs &a, hipStream_t stream);

// tensor output (tensor_pack.hip): dense RGB8 pictures -> normalised, padded tensors of one shape
struct TensorArgs {
    const uint8_t *src;          // the call's pictures, 3 * sw * sh bytes apart, 4-byte aligned
    const uint8_t *src_end;      // their end: no load reaches outside [src, src_end)
    int            n;            // pictures first .. first + n of them (launch_tensor splits a call into launches)
    int            first;
    int            sw, sh;       // picture
    int            cw, ch;       // canvas (each >= the picture's side)
    int            dtype, layout, bgr;
    uint32_t       pad_rgb;
    float          scale[3], bias[3];
    int            rows;         // canvas rows per workgroup: tensor_lds_bytes(rows, sw) must fit a workgroup's LDS (64 KiB)
    uint8_t       *out;          // 16-byte aligned; a picture's tensor is tensor_bytes long
    size_t         tensor_bytes;
    const int32_t *slots;        // NULL: picture i of the call goes to slot i
};
size_t     tensor_lds_bytes(int rows, int sw);
hipError_t launch_tensor(const TensorArgs &a, hipStream_t stream);

} // namespace mvhp
