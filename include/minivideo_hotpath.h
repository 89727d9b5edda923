/*
 * minivideo_hotpath.h -- C-ABI of the MI355X-native H.264 intra reconstruction
 * hot path (libminivideo.so).  Plain pointers and sizes only; no torch / HIP
 * types in any signature (a HIP stream is passed as an opaque void*).
 *
 * What each entry point replaces in the reference (paths relative to
 * minivideo/src/ of misterk72/MiniVideo):
 *
 *   mvhp_parse_annexb / mvhp_index_annexb
 *       demuxer/esparser/esparser.c:40-143      (es_fileParse)
 *       decoder/h264/h264.c:76-188              (NAL loop)
 *       decoder/h264/h264_nalu.c:109-249        (header, emulation prevention)
 *       decoder/h264/h264_parameterset.c:123-397, 812-942 (SPS, PPS)
 *       decoder/h264/h264_slice.c:156-334, 1013-1142      (slice header, MB loop)
 *       decoder/h264/h264_macroblock.c:75-313   (macroblock_layer, minus :278-281)
 *       decoder/h264/h264_cavlc.c:79-346, h264_cabac.c:138-325 (residual blocks)
 *       decoder/h264/h264_intra_prediction.c:196-290, 977-1083 (pred-mode derivation)
 *   mvhp_recon_batch_dev / mvhp_recon_batch_host
 *       decoder/h264/h264_macroblock.c:278-281  (intra_prediction_process call)
 *       decoder/h264/h264_intra_prediction.c:112-2564 (all sample prediction)
 *       decoder/h264/h264_transform.c:121-1610  (dequant, IDCT, DC transforms,
 *                                                picture construction)
 *       export.c:65-188, export_utils.c:117-198 (planar YCbCr gather)
 *       export_utils.c:209-324                  (mb_to_rgb colour conversion)
 *       -- plus, opt-in (MVHP_PARAM_DEBLOCK), the in-loop deblocking filter of clause 8.7, which the reference does not have.
 *
 * The packed macroblock record below is the build's replacement for the
 * reference's Macroblock_t (decoder/h264/h264_macroblock_struct.h:209-319) as
 * the interface between entropy decoding (host) and reconstruction (GPU).
 */
#ifndef MINIVIDEO_HOTPATH_H
#define MINIVIDEO_HOTPATH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVHP_EXPORT __attribute__((visibility("default")))

/* Return codes follow the reference convention (typedef.h:40-42). */
#define MVHP_SUCCESS      1
#define MVHP_FAILURE      0
#define MVHP_UNSUPPORTED (-1)

/* ---------------------------------------------------------------------------
 * Packed macroblock record: 32-byte header + 384 int16 coefficients = 800 B.
 *
 * Coefficient area (int16, little endian), already inverse-scanned
 * (zig-zag -> raster, h264_transform.c:440-480 is a pure permutation that the
 * host applies while scattering entropy-decoder output):
 *   [  0..255]  luma. mb_kind I4x4 / I16x16: 16 blocks in luma4x4BlkIdx
 *               order (h264_spatial.c:210), each 16 coefficients c[row][col]
 *               row-major.  I16x16: slot 0 of block b holds the *untransformed*
 *               Intra16x16 DC level c1[i][j] with {i,j}=raster position of b
 *               (h264_transform.c:180-186); the kernel runs the 4x4 Hadamard.
 *               mb_kind I8x8: 4 blocks in luma8x8BlkIdx order, each 64
 *               coefficients c[row][col] row-major.
 *   [256..319]  Cb: 4 blocks (chroma4x4BlkIdx order), 16 coefficients each;
 *               slot 0 of block k holds the untransformed chroma DC level k
 *               (h264_transform.c:313-316,354).
 *   [320..383]  Cr, same layout.
 * ------------------------------------------------------------------------- */
#define MVHP_MB_HEADER_BYTES  32
#define MVHP_MB_COEFS         384
#define MVHP_MB_BYTES         800

#define MVHP_KIND_I4x4   0
#define MVHP_KIND_I8x8   1
#define MVHP_KIND_I16x16 2
/* I_PCM (h264_macroblock.c:151-154 returns UNSUPPORTED, ipcm_construction_process h264_intra_prediction.c:2585-2630 is dead
 * code in the reference): only streams opened with MVHP_STREAM_SPEC produce it (outside parity).  The
 * coefficient area then holds the 384 SAMPLES, one byte each, arranged so that every owner of a 32-byte piece of the record
 * finds whole rows in it: for j = 0..7, bytes [64j, 64j+32) = luma rows 2j and 2j+1 (16 samples each), bytes [64j+32, 64j+40) =
 * Cb row j, [64j+40, 64j+48) = Cr row j, [64j+48, 64j+64) = 0; the chroma part of the area (bytes 512..767) is 0.
 * nz_mask = 0, qp_y = 0 (QP'Y of an I_PCM macroblock, 7.4.5). */
#define MVHP_KIND_IPCM   3

typedef struct mvhp_mb_header {
    uint8_t  mb_kind;          /* MVHP_KIND_*  (MbPartPredMode, h264_macroblock_struct.h:33-44) */
    uint8_t  qp_y;             /* QP'Y of this macroblock (h264_macroblock.c:263-269)           */
    uint8_t  cbp;              /* bits 0-3 CodedBlockPatternLuma, bits 4-5 ...Chroma            */
    uint8_t  chroma_pred_mode; /* IntraChromaPredMode 0=DC 1=H 2=V 3=Plane                      */
    uint8_t  i16_pred_mode;    /* Intra16x16PredMode 0=V 1=H 2=DC 3=Plane                       */
    uint8_t  flags;            /* bits 1-2: disable_deblocking_filter_idc (0, 1, 2) of the macroblock's slice -- set only by
                                  streams opened with MVHP_STREAM_DEBLOCK, read only under MVHP_PARAM_DEBLOCK / stage
                                  MVHP_STAGE_DEBLOCK; bit 0: compact transfer form only ("dense", see below); bits 3-7: 0
                                  (TransformBypassModeFlag is never set for 8-bit)                                      */
    uint8_t  unavail;          /* MVHP_UNAVAIL_*: neighbouring macroblocks that exist by geometry but lie in ANOTHER SLICE
                                  (6.4.8: not available); always 0 for the reference's one-slice pictures -- set only by
                                  streams opened with MVHP_STREAM_SPEC, announced by MVHP_PARAM_SLICES   */
    uint8_t  dbk_offsets;      /* deblocking filter offsets of the macroblock's slice (MVHP_STREAM_DEBLOCK streams, else 0):
                                  bits 0-3 slice_alpha_c0_offset_div2, bits 4-7 slice_beta_offset_div2, each a 4-bit
                                  two's-complement value in -6..6                                                      */
    uint32_t nz_mask;          /* bit b (0-15): luma 4x4 block b (or 8x8 block b>>2) has a
                                  non-zero level; bit 16+k: Cb block k; bit 20+k: Cr block k.
                                  DC levels count for the block whose slot 0 they occupy.
                                  A hint only: the kernel may skip all-zero blocks.         */
    uint8_t  pred_mode[16];    /* final Intra4x4PredMode[16] or Intra8x8PredMode[4]             */
    uint32_t reserved1;
} mvhp_mb_header_t;

#define MVHP_UNAVAIL_A 1u   /* left        (mbAddrA, h264_spatial.c:333-416) */
#define MVHP_UNAVAIL_B 2u   /* above       (mbAddrB) */
#define MVHP_UNAVAIL_C 4u   /* above right (mbAddrC) */
#define MVHP_UNAVAIL_D 8u   /* above left  (mbAddrD) */
#define MVHP_DBK_IDC_SHIFT 1   /* mvhp_mb_header_t::flags: (flags >> MVHP_DBK_IDC_SHIFT) & 3 = disable_deblocking_filter_idc */

/* ---------------------------------------------------------------------------
 * Compact pictures: the transfer format between the host front end and the GPU (PCIe carries it instead of the packed
 * records, of which most int16 slots are zero: ~140 instead of 800 bytes per macroblock on dense content).  One picture =
 *     uint32 mb_off[W*H]          byte offset of each macroblock's compact record, counted from the end of this table
 *     compact records, 4-byte aligned, in macroblock order:
 *         mvhp_mb_header_t        as in the packed record, with reserved1 = number of entries that follow
 *         uint32 entry[n]         one per non-zero level, in the order the entropy decoder delivered them:
 *                                 bits 0-15 = int16 slot of the coefficient area (0..383), bits 16-31 = the level
 *       or, for a macroblock of more than MVHP_COMPACT_MAX_ENTRIES levels, header.flags bit 0 set, reserved1 = 0 and
 *       the 768-byte coefficient area itself.
 * mvhp_expand_compact_dev() turns it into packed records on the device (a memory-bound pass of < 1 KB per macroblock);
 * the packed record stays the input format of the reconstruction kernels.
 * ------------------------------------------------------------------------- */
#define MVHP_COMPACT_MAX_ENTRIES  191
#define MVHP_COMPACT_MB_BYTES_MAX 804    /* 4 (offset) + 32 + 768: a picture needs at most W*H times this ...          */
#define MVHP_COMPACT_SLACK_BYTES  1536   /* ... plus this (entries of one macroblock before it is found to be dense)   */

/* Parameters shared by every picture of one batch (one SPS/PPS pair). */
typedef struct mvhp_stream_params {
    uint32_t width_mbs;                      /* PicWidthInMbs                          */
    uint32_t height_mbs;                     /* PicHeightInMapUnits (frame MBs only)   */
    int32_t  chroma_qp_index_offset;         /* PPS, Cb (h264_transform.c:611-618)     */
    int32_t  second_chroma_qp_index_offset;  /* PPS, Cr                                */
    uint32_t flags;                          /* MVHP_PARAM_*                            */
    /* MVHP_PARAM_SCALING only (ignored otherwise): the weight matrices in force for the batch's pictures, after the
     * fall-back rules of 7.4.2.1.1 / 7.4.2.2 (h264_parameterset.c:723-736, 904-923 parse them; the reference's own LevelScale
     * is only right for flat lists), in RASTER order [i*4+j] / [i*8+j]: LevelScale4x4[plane][m][i][j] =
     * scaling4[plane][i*4+j] * normAdjust4x4(m,i,j) (h264_transform.c:645-741). */
    uint8_t  scaling4[3][16];                /* Intra Y, Cb, Cr                          */
    uint8_t  scaling8[64];                   /* Intra Y 8x8                              */
} mvhp_stream_params_t;

/* flags: the batch may contain Intra8x8 macroblocks (PPS transform_8x8_mode_flag).  A hint for the kernel choice
 * only -- every kernel reconstructs every macroblock kind; callers that build records themselves may leave it 0. */
#define MVHP_PARAM_MAY_HAVE_8X8 1u
/* flags: Intra16x16 luma DC dequantisation by the standard's rule (qP >= 36 takes the left-shift branch, 8.5.10) instead
 * of the reference's `qP > 36` (h264_transform.c:797-808), i.e. without the reference's QP'Y = 36 defect.  Results
 * differ from the reference exactly on Intra16x16 macroblocks at QP'Y = 36.  Set by streams opened with
 * MVHP_STREAM_SPEC (outside the parity contract, opt-in). */
#define MVHP_PARAM_SPEC_LUMA_DC 2u
/* flags (set only for streams opened with MVHP_STREAM_SPEC; outside the parity contract -- the reference
 * decodes none of these correctly):
 * MVHP_PARAM_SLICES   pictures of several slices: records carry mvhp_mb_header_t::unavail.  Reconstructed by the one-picture-
 *                     per-workgroup kernel, where availability is a per-wavefront scalar (the batch kernels keep eight / four
 *                     pictures in lock step at one macroblock position and derive availability from the position alone).
 * MVHP_PARAM_SCALING  scaling4 / scaling8 hold non-flat weight matrices (SPS / PPS scaling lists).  Same kernel. */
#define MVHP_PARAM_SLICES  4u
#define MVHP_PARAM_SCALING 8u
/* flags: apply the in-loop deblocking filter (clause 8.7) to the reconstructed pictures, with the per-macroblock
 * disable_deblocking_filter_idc / offsets of the records (mvhp_mb_header_t::flags bits 1-2, dbk_offsets) and slice boundaries
 * from mvhp_mb_header_t::unavail.  Set by mvhp_stream_params() for streams opened with MVHP_STREAM_DEBLOCK; callers that build
 * records themselves may set it.  Outside the parity contract (the reference never deblocks); without it no filter is
 * applied.  Filtered pictures are converted to RGB by the separate colour kernel, after the filter. */
#define MVHP_PARAM_DEBLOCK 16u

/* Bytes of one reconstructed picture: planar Y | Cb | Cr of the *uncropped*
 * coded size (export.c:80-81), and interleaved RGB8. */
MVHP_EXPORT size_t mvhp_packed_frame_bytes(const mvhp_stream_params_t *p);
MVHP_EXPORT size_t mvhp_yuv_frame_bytes(const mvhp_stream_params_t *p);
MVHP_EXPORT size_t mvhp_rgb_frame_bytes(const mvhp_stream_params_t *p);

/* ---------------------------------------------------------------------------
 * Host front end (no GPU involved): Annex-B bytes -> packed pictures.
 * ------------------------------------------------------------------------- */
typedef struct mvhp_stream mvhp_stream_t;   /* parsed elementary stream */

/* Index + parse parameter sets of an Annex-B buffer held in memory.
 * The buffer must outlive the handle. */
MVHP_EXPORT int  mvhp_stream_open(const uint8_t *data, size_t size, mvhp_stream_t **out);
/* The same with flags.  0 = reference parity (everything above).  MVHP_STREAM_SPEC (opt-in; also
 * chosen by minivideo_decode when the environment has MINIVIDEO_SPEC=1): index the stream the way the standard
 * defines it instead of the way esparser.c:40-143 does -- three-byte start codes (Annex B), slice / SPS / PPS NAL units
 * of any nal_ref_idc, no 32-byte blind tail -- and reconstruct Intra16x16 at QP'Y = 36 by the standard's rule
 * (MVHP_PARAM_SPEC_LUMA_DC); pictures of several slices (MVHP_PARAM_SLICES), SPS / PPS scaling lists (MVHP_PARAM_SCALING) and
 * I_PCM macroblocks (MVHP_KIND_IPCM) are decoded by the standard's rules. */
#define MVHP_STREAM_SPEC 1u
/* MVHP_STREAM_DEBLOCK (opt-in, independent of MVHP_STREAM_SPEC; also chosen by minivideo_decode when the environment has
 * MINIVIDEO_DEBLOCK=1): the front end fills the records' deblocking fields from the slice headers (and refuses a slice whose
 * disable_deblocking_filter_idc is above 2 or whose offsets lie outside -6..6), and mvhp_stream_params() sets
 * MVHP_PARAM_DEBLOCK.  Without it those record bytes stay 0 and no picture is filtered. */
#define MVHP_STREAM_DEBLOCK 2u
MVHP_EXPORT int  mvhp_stream_open_ex(const uint8_t *data, size_t size, uint32_t flags, mvhp_stream_t **out);
/* Same for an ISO-BMFF (MP4/MOV) buffer: avcC parameter sets + the IDR NAL units of the sync samples of the first
 * video track (replaces demuxer/mp4/mp4.c:2587 mp4_fileParse for the thumbnail path). */
MVHP_EXPORT int  mvhp_stream_open_mp4(const uint8_t *data, size_t size, mvhp_stream_t **out);
MVHP_EXPORT void mvhp_stream_close(mvhp_stream_t *s);
MVHP_EXPORT int  mvhp_stream_idr_count(const mvhp_stream_t *s);
/* The display rotation of the stream, clockwise, in degrees: 0, 90, 180 or 270.  MP4: the video track's tkhd matrix when it is
 * one of the four pure rotations (a mirrored, scaled or sheared matrix, non-zero u / v, a w other than 1.0 or a box too short
 * for the matrix give 0; the translation is ignored; the movie header's matrix is not read).  Annex-B streams: 0.  The
 * reference reads the matrix, traces it and drops it (demuxer/mp4/mp4.c:1167-1197).  Information only: nothing turns unless an
 * output request asks for it ("Orientation" below). */
MVHP_EXPORT int  mvhp_stream_rotation(const mvhp_stream_t *s);
/* What the VUI of the SPS in force for IDR picture `idr` says about display (E.1.1, up to and excluding timing_info; the
 * reference parses these fields and only traces them, h264_parameterset.c:1318-1350).  sar_w : sar_h is the sample aspect ratio
 * after Table E-1 (aspect_ratio_idc 1..16) or the transmitted pair (idc 255), reduced by their gcd; 0 : 0 = unspecified (no VUI,
 * no aspect_ratio_info, idc 0 or 17..254, or a zero term).  matrix_coefficients is 2 ("unspecified") and chroma_loc 0 when the
 * stream does not carry them; chroma_loc is chroma_sample_loc_type_top_field (frames only).  A VUI that ends early or carries a
 * chroma_sample_loc_type above 5 never fails the SPS: every field is then "unspecified" and vui_present stays 1.  Information
 * only: nothing changes unless an output request asks for it ("Display aspect and colour" below).  MVHP_FAILURE: the picture has
 * no parameter sets. */
typedef struct mvhp_display_info {
    uint32_t sar_w, sar_h;
    uint32_t vui_present;          /* vui_parameters_present_flag                                             */
    uint32_t signal_present;       /* video_signal_type_present_flag                                          */
    uint32_t full_range;           /* video_full_range_flag (0 when absent)                                   */
    uint32_t matrix_coefficients;  /* Table E-5; 2 when absent                                                */
    uint32_t chroma_loc;           /* chroma_sample_loc_type_top_field, 0..5; 0 when absent                   */
    uint32_t reserved;
} mvhp_display_info_t;
MVHP_EXPORT int  mvhp_stream_display(const mvhp_stream_t *s, int idr, mvhp_display_info_t *out);
/* Parameters in force for IDR picture `idr` (valid after mvhp_stream_open). */
MVHP_EXPORT int  mvhp_stream_params(const mvhp_stream_t *s, int idr, mvhp_stream_params_t *out);
/* Entropy-decode IDR picture `idr` into `packed` (mvhp_packed_frame_bytes()).
 * Thread-safe for distinct `idr` on the same handle. */
MVHP_EXPORT int  mvhp_stream_decode_packed(const mvhp_stream_t *s, int idr, void *packed, size_t packed_bytes);
/* The same into the compact transfer format; `cap` >= W*H * MVHP_COMPACT_MB_BYTES_MAX + MVHP_COMPACT_SLACK_BYTES,
 * *used = bytes written. */
MVHP_EXPORT int  mvhp_stream_decode_compact(const mvhp_stream_t *s, int idr, void *buf, size_t cap, size_t *used);
MVHP_EXPORT const char *mvhp_stream_last_error(void);

/* ---------------------------------------------------------------------------
 * GPU reconstruction.
 * ------------------------------------------------------------------------- */
typedef struct mvhp_ctx mvhp_ctx_t;

MVHP_EXPORT int  mvhp_device_count(void);
MVHP_EXPORT int  mvhp_create(int device, mvhp_ctx_t **out);
MVHP_EXPORT void mvhp_destroy(mvhp_ctx_t *ctx);
MVHP_EXPORT const char *mvhp_last_error(void);

/* Alignment, in bytes, of every device buffer handed to the three entry points below: d_packed, d_yuv and d_rgb of
 * mvhp_recon_batch_dev / mvhp_recon_stages_dev, d_compact and d_packed of mvhp_expand_compact_dev.  The kernels behind them move
 * records, luma rows and RGB in naturally aligned 16-byte pieces (DESIGN.md 5 "Caller buffers of the reconstruction entry
 * points" has the widest access per buffer and kernel form).  The per-picture sizes -- 800, 384 and 768 bytes per macroblock --
 * are multiples of it, so picture k of an aligned buffer is aligned too; a caller that carves its buffers out of a larger
 * allocation rounds each piece's start up to it.  A pointer below it is refused with MVHP_FAILURE before anything is launched,
 * and mvhp_last_error() names the argument.  mvhp_recon_align() returns the same number. */
#define MVHP_RECON_ALIGN 16
MVHP_EXPORT size_t mvhp_recon_align(void);

/* Reconstruct n_frames pictures whose packed records are resident in device
 * memory.  d_yuv receives n_frames * mvhp_yuv_frame_bytes(); d_rgb (may be
 * NULL) receives n_frames * mvhp_rgb_frame_bytes(); d_packed, d_yuv and d_rgb
 * are MVHP_RECON_ALIGN-byte aligned.  `stream` is a hipStream_t
 * (NULL = the context's own stream).  Asynchronous with respect to the host. */
MVHP_EXPORT int  mvhp_recon_batch_dev(mvhp_ctx_t *ctx, const mvhp_stream_params_t *p,
                                      const void *d_packed, int n_frames,
                                      uint8_t *d_yuv, uint8_t *d_rgb, void *stream);

/* n_pictures compact pictures (see "Compact pictures" above), `stride` bytes apart in device memory, -> packed records
 * (n_pictures * mvhp_packed_frame_bytes()) in device memory.  d_compact and d_packed are MVHP_RECON_ALIGN-byte aligned, `stride` is
 * a multiple of 4 (the kernel reads the compact pictures in 4-byte words; the pointer's rule is the one rule of the three entry
 * points).  Asynchronous on `stream` (NULL = the context's own). */
MVHP_EXPORT int  mvhp_expand_compact_dev(mvhp_ctx_t *ctx, const mvhp_stream_params_t *p, const void *d_compact,
                                         size_t stride, int n_pictures, void *d_packed, void *stream);

/* Same, but only the stages selected by `stages` -- lets a caller bracket each kernel with its own events:
 * bit 0: reconstruction kernel (followed by the deblocking filter when p->flags has MVHP_PARAM_DEBLOCK),
 * bit 1: colour conversion of d_yuv into d_rgb (after the filter when both run),
 * bit 2: the deblocking filter alone, in place on d_yuv, with the record headers of d_packed and the params (whatever
 *        p->flags says).
 * Error word of the context (mvhp_sync_check): bit 0 a reconstruction row wait timed out, bit 1 a wide launch's ticket lay
 * outside the launch, bit 2 a deblocking row wait timed out.
 * d_packed, d_yuv and d_rgb (may be NULL) are MVHP_RECON_ALIGN-byte aligned, whichever stages run. */
#define MVHP_STAGE_RECON   1
#define MVHP_STAGE_COLOR   2
#define MVHP_STAGE_DEBLOCK 4
MVHP_EXPORT int  mvhp_recon_stages_dev(mvhp_ctx_t *ctx, const mvhp_stream_params_t *p,
                                       const void *d_packed, int n_frames,
                                       uint8_t *d_yuv, uint8_t *d_rgb, void *stream, int stages);

/* ---------------------------------------------------------------------------
 * Output geometry (opt-in): the visible or a downscaled picture instead of the coded size.  By default every entry point
 * delivers the coded size, as the reference does, which parses the SPS crop (h264_parameterset.c:360-378) and never applies
 * it.  An mvhp_output_request_t asks for more: mvhp_engine_decode_ex takes one, minivideo_decode builds one from
 * MINIVIDEO_CROP / MINIVIDEO_THUMBNAIL (include/minivideo.h), and the functions below are the pieces for callers that manage
 * device buffers themselves.
 *   crop: the SPS frame-cropping rectangle (7.4.2.1.1; 4:2:0 frames: CropUnitX = CropUnitY = 2), luma samples:
 *         x = 2 left, y = 2 top, w = 16 W - 2 (left + right), h = 16 H - 2 (top + bottom); chroma is the same rectangle halved.
 *   box:  the cropped picture fitted into box_w x box_h (DESIGN.md 3 "Output geometry": aspect kept, even sides, never
 *         enlarged) by an integer area-average filter that is exact for D = S (crop only is the same pass).
 * Crop and box treat samples as square: a 1440 x 1080 SAR 4:3 picture keeps its 4:3 grid.  MVHP_OUTPUT_ASPECT (below) applies the
 * VUI's sample aspect ratio (mvhp_stream_display) first.
 * ------------------------------------------------------------------------- */
typedef struct mvhp_output_geometry {
    uint32_t crop_x, crop_y, crop_w, crop_h;   /* luma rectangle of the coded picture that is kept (all even)          */
    uint32_t out_w, out_h;                     /* size of the output picture (even; equal to crop_w / crop_h, or less) */
    uint32_t reserved[2];
} mvhp_output_geometry_t;

#define MVHP_OUTPUT_CROP 1u   /* mvhp_output_request_t::flags: pictures are the SPS's cropped rectangle         */
#define MVHP_OUTPUT_BOX  2u   /* ... fitted into box_w x box_h (implies MVHP_OUTPUT_CROP); box sides >= 2     */
#define MVHP_OUTPUT_SCORE 4u  /* mvhp_engine_decode_ex: every picture's score in g->reserved[1] ("Picture scores" below); changes no
                                 picture: a request with this flag alone still means pictures of the coded size */
/* Orientation (opt-in; DESIGN.md 3 "Orientation"): pictures turned by quarter turns, clockwise.  MVHP_OUTPUT_ORIENT applies the
 * stream's own rotation (mvhp_stream_rotation), MVHP_OUTPUT_ROTATE(q) adds q further quarter turns; what is applied is the sum
 * modulo 4 (mvhp_output_turns).  "auto" is the flag alone, an explicit angle the field alone.  Both compose with every flag
 * above.  A sum of 0 is the request without these bits: the same paths, launches, buffers and bytes. */
#define MVHP_OUTPUT_ORIENT 8u
#define MVHP_OUTPUT_ROTATE_SHIFT 4
#define MVHP_OUTPUT_ROTATE_MASK  0x30u
#define MVHP_OUTPUT_ROTATE(q) (((uint32_t)(q) & 3u) << MVHP_OUTPUT_ROTATE_SHIFT)
/* Display aspect (opt-in; DESIGN.md 3 "Display aspect and colour"): MVHP_OUTPUT_ASPECT (implies MVHP_OUTPUT_CROP) makes the
 * samples of the output square.  With the crop cw x ch and the stream's sample aspect ratio a : b (1 : 1 when unspecified), in
 * 64-bit arithmetic, one axis shrinks and nothing is ever enlarged:
 *     a > b:  out_w = cw, out_h = max(2, 2 floor((ch b + a) / (2 a)))        a < b:  out_h = ch, out_w = max(2, 2 floor((cw a + b) / (2 b)))
 * (1440 x 1080 at 4:3 -> 1440 x 810; 720 x 576 at 12:11 -> 720 x 528; 720 x 480 at 10:11 -> 654 x 480).  A box is fitted to that
 * size afterwards (1440 x 1080 at 4:3 in 320 x 320 -> 320 x 180), a turn exchanges the sides last; crop_* do not change.  The
 * resample pass filters each axis with its own ratio, so it is the pass of a box with that output size.
 * Colour (opt-in): MVHP_OUTPUT_COLOR makes the RGB a call delivers (MVHP_OUT_RGB, MVHP_OUT_RGB_ONLY, MVHP_OUT_PNG) with
 * mvhp_color_dev from the FINAL planes -- behind the crop, the box and the turn -- instead of the reference's BT.601
 * limited-range formula; the parameters are mvhp_color_resolve() of the picture's mvhp_stream_display() under the mode
 * MVHP_OUTPUT_COLOR_MODE(m) (bits 8-10: 0 auto, 1 BT.601 limited, 2 BT.709 limited, 3 BT.601 full, 4 BT.709 full), except that
 * pictures a resample pass SCALED take MVHP_CHROMA_CENTER whatever the stream says (an area average of chroma is centred on its
 * 2x2 luma cell; a turned picture keeps the stream's siting as read along its own rows -- an approximation).  Planes and JPEG
 * files are not affected (JFIF defines what its planes mean); a call that delivers no RGB ignores the flag and launches nothing.
 * A batch holds pictures of one geometry and one resolved colour setting.  Without these flags every path, launch, buffer and
 * byte is what it is without them. */
#define MVHP_OUTPUT_ASPECT 0x800u   /* (0x40 stays an unknown flag: the engine harness pins it as the one a request is refused for) */
#define MVHP_OUTPUT_COLOR  0x80u
#define MVHP_OUTPUT_COLOR_MODE_SHIFT 8
#define MVHP_OUTPUT_COLOR_MODE_MASK  0x700u
#define MVHP_OUTPUT_COLOR_MODE(m) (((uint32_t)(m) & 7u) << MVHP_OUTPUT_COLOR_MODE_SHIFT)
/* Black bars (opt-in; "Black bars" below).  MVHP_OUTPUT_TRIM (implies MVHP_OUTPUT_CROP): crop_* of a picture's geometry is
 * mvhp_trim_rect(the picture's SPS crop, the box the stream carries -- mvhp_stream_set_trim); aspect, box and the turn's exchange of
 * sides follow unchanged and start from that rectangle.  A picture for which the rule says 0 (another SPS in mid-stream, a
 * different size) keeps its SPS crop: trimming never fails a picture.  With no box set the flag is MVHP_OUTPUT_CROP.
 * MVHP_OUTPUT_BARS (mvhp_engine_decode_ex only) probes: behind whatever reconstructs the batch (and the deblocking filter)
 * mvhp_luma_bars_dev runs over each picture's crop rectangle on the coded planes, the 32-byte records come back with the pictures
 * and the sink finds g->reserved[0] = x | y << 16 and g->reserved[1] = w | h << 16 (sides are at most 16384).  Those words are the
 * file length and the score elsewhere: the flag is refused together with MVHP_OUT_JPEG, MVHP_OUT_PNG, MVHP_OUTPUT_SCORE and the
 * plain sink of mvhp_engine_decode.  The level travels in bits 24-31 of mvhp_output_request_t::reserved (MVHP_BARS_REQUEST; 0 = 24).
 * The flag changes no picture: a request with this flag alone still means pictures of the coded size; d2h_bytes grows by exactly
 * 32 per delivered picture. */
#define MVHP_OUTPUT_BARS 0x1000u
#define MVHP_OUTPUT_TRIM 0x2000u
#define MVHP_BARS_REQUEST(level) (((uint32_t)(level) & 0xffu) << 24)
/* Representative pictures (opt-in; "Representative pictures" below).  MVHP_OUTPUT_HIST (mvhp_engine_decode_ex only) probes: behind
 * whatever reconstructs the batch (and the deblocking filter) mvhp_plane_hist_dev runs over each picture's crop rectangle on the
 * coded planes, the 3104-byte records come back with the pictures, and the sink reads its picture's record with
 * mvhp_engine_picture_hist (the sink's signature and g->reserved[] stay as they are).  The flag changes no picture: a request with
 * this flag alone still means pictures of the coded size; d2h_bytes grows by exactly 3104 per delivered picture of a downloaded
 * batch.  It composes with every other flag, MVHP_OUTPUT_SCORE included, and every output kind, except MVHP_OUTPUT_BARS: two
 * probes in one call are refused. */
#define MVHP_OUTPUT_HIST 0x4000u
typedef struct mvhp_output_request {
    uint32_t flags;           /* MVHP_OUTPUT_*; 0 = the coded size (what the reference writes)                  */
    uint32_t box_w, box_h;
    uint32_t reserved;
} mvhp_output_request_t;

/* The SPS cropping rectangle of IDR picture `idr` (out_w / out_h = its size; a stream without frame_cropping_flag gives
 * the coded size).  Information only: it changes nothing.  MVHP_FAILURE (mvhp_stream_last_error() says why) when the
 * picture has no parameter sets or the crop leaves nothing (w <= 0 or h <= 0). */
MVHP_EXPORT int    mvhp_stream_crop(const mvhp_stream_t *s, int idr, mvhp_output_geometry_t *out);
/* The quarter turns (0..3, clockwise) that `req` applies to pictures of `s` (NULL request: 0). */
MVHP_EXPORT int    mvhp_output_turns(const mvhp_stream_t *s, const mvhp_output_request_t *req);
/* The output geometry of picture `idr` under `req` (NULL or flags 0: the coded size, no crop).  It is what the sink gets: under a
 * request that turns by an odd number of quarter turns the geometry is formed with box_w and box_h exchanged and out_w / out_h
 * are exchanged afterwards (1920 x 1080 in a 320 x 320 box: 320 x 180 unturned, 180 x 320 turned); crop_* stay in coded
 * coordinates.  The bytes of a picture (mvhp_geometry_*_bytes) do not change with the turn. */
MVHP_EXPORT int    mvhp_output_geometry(const mvhp_stream_t *s, int idr, const mvhp_output_request_t *req,
                                        mvhp_output_geometry_t *out);
/* The size rule alone: cw x ch (even) fitted into bw x bh (each >= 2) -> *ow x *oh. */
MVHP_EXPORT int    mvhp_geometry_fit(uint32_t cw, uint32_t ch, uint32_t bw, uint32_t bh, uint32_t *ow, uint32_t *oh);
/* The aspect rule alone (MVHP_OUTPUT_ASPECT above): cw x ch (even, >= 2) with sample aspect ratio sar_w : sar_h (0 in either: 1 : 1)
 * -> *ow x *oh. */
MVHP_EXPORT int    mvhp_geometry_aspect(uint32_t cw, uint32_t ch, uint32_t sar_w, uint32_t sar_h, uint32_t *ow, uint32_t *oh);
/* Bytes of one output picture: planar Y | Cb | Cr of out_w x out_h, and interleaved RGB8. */
MVHP_EXPORT size_t mvhp_geometry_yuv_bytes(const mvhp_output_geometry_t *g);
MVHP_EXPORT size_t mvhp_geometry_rgb_bytes(const mvhp_output_geometry_t *g);
/* n coded pictures (d_yuv_coded: n * mvhp_yuv_frame_bytes(p), 16-byte aligned) -> n output pictures of geometry g: planes
 * into d_yuv_out (n * mvhp_geometry_yuv_bytes(g), may be NULL) and / or RGB (the reference's integer formula, 2x2-nearest
 * chroma) into d_rgb_out (n * mvhp_geometry_rgb_bytes(g), may be NULL); both 4-byte aligned.  Asynchronous on `stream`
 * (NULL = the context's own). */
MVHP_EXPORT int    mvhp_resample_dev(mvhp_ctx_t *ctx, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g,
                                     const uint8_t *d_yuv_coded, int n, uint8_t *d_yuv_out, uint8_t *d_rgb_out, void *stream);

/* Orientation on the device (orient.hip): n pictures turned by `quarter_turns` (0..3, clockwise) into planes (d_yuv_out, may be
 * NULL) and / or RGB (d_rgb_out, may be NULL), both dense and 4-byte aligned like the outputs of mvhp_resample_dev.  `g` is the
 * geometry BEFORE the turn.  With MVHP_ORIENT_SRC_CODED in src_flags, d_src holds n coded pictures of `p` (16-byte aligned) and
 * the crop rectangle of g is read out of them (out_w / out_h must equal crop_w / crop_h: a turned crop needs no copy pass
 * first); without it d_src holds n dense pictures of g->out_w x g->out_h (4-byte aligned), as mvhp_resample_dev leaves them (p
 * is not read and may be NULL).  Output pictures are out_h x out_w for odd turns and out_w x out_h for even ones.  For a source
 * plane S of w x h and its output O (each plane with its own size):
 *     1 turn:  O[y][x] = S[h-1-x][y]       2 turns: O[y][x] = S[h-1-y][w-1-x]       3 turns: O[y][x] = S[x][w-1-y]
 * RGB is made from the TURNED planes with the reference's integer formula and 2x2-nearest chroma.  All sides are even, so a 2x2
 * chroma cell of the source is a 2x2 cell of the output: RGB of the turned planes equals the turned RGB of the source.  Zero
 * turns is valid: a crop or copy plus colour conversion.  n = 0 does nothing; turns outside 0..3, n < 0, odd or zero sizes and
 * a rectangle outside the coded picture are refused (MVHP_FAILURE) before anything is launched.  Asynchronous on `stream` (NULL
 * = the context's own).  Nothing is shared between workgroups, no kernel waits and nothing survives a launch: safe under stream
 * capture, and two calls on two streams do not meet. */
#define MVHP_ORIENT_SRC_CODED 1u
MVHP_EXPORT int    mvhp_orient_dev(mvhp_ctx_t *ctx, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g, int quarter_turns,
                                   uint32_t src_flags, const uint8_t *d_src, int n, uint8_t *d_yuv_out, uint8_t *d_rgb_out,
                                   void *stream);

/* ---------------------------------------------------------------------------
 * Colour conversion (opt-in; DESIGN.md 3 "Display aspect and colour"; color_convert.hip): RGB from planar 4:2:0 pictures by the
 * matrix, range and chroma siting the stream names, in integers only -- the bytes are a function of the samples and the three
 * parameters (tests/color_ref.py restates them).
 *   Chroma in sixteenths.  For luma (x, y), j = y >> 1, k = x >> 1, chroma indices clamped at the plane's edges:
 *     vertical:            y even: rows (j-1, j) weights (1, 3);           y odd: rows (j, j+1) weights (3, 1)
 *     MVHP_CHROMA_LEFT:    x even: column k weight 4;                      x odd: columns (k, k+1) weights (2, 2)
 *     MVHP_CHROMA_CENTER:  x even: columns (k-1, k) weights (1, 3);        x odd: columns (k, k+1) weights (3, 1)
 *     c16 = sum of wy wx C (the weights sum to 16, nothing is rounded);    MVHP_CHROMA_NEAREST: c16 = 16 C[j][k]
 *   Colour.  y' = 16 cy (Y - yoff), cb = Cb16 - 2048, cr = Cr16 - 2048, >> arithmetic:
 *     R = clamp8((y' + crv cr + 2^17) >> 18)   G = clamp8((y' - gcb cb - gcr cr + 2^17) >> 18)   B = clamp8((y' + cbu cb + 2^17) >> 18)
 *   Coefficients {cy, crv, cbu, gcb, gcr, yoff} = round(2^14 x) of the exact rationals of (Kr, Kb) = (0.299, 0.114) for BT.601
 *   and (0.2126, 0.0722) for BT.709, times 255/219 (luma) and 255/224 (chroma) for limited range (yoff 16, else 0):
 *   mvhp_color_coefficients().
 * ------------------------------------------------------------------------- */
#define MVHP_MATRIX_BT601 0
#define MVHP_MATRIX_BT709 1
#define MVHP_CHROMA_NEAREST 0
#define MVHP_CHROMA_LEFT    1
#define MVHP_CHROMA_CENTER  2
typedef struct mvhp_color_params {
    int32_t matrix;       /* MVHP_MATRIX_*            */
    int32_t full_range;   /* 0 limited (16..235 / 16..240), 1 full (0..255) */
    int32_t siting;       /* MVHP_CHROMA_*            */
    int32_t reserved;     /* 0                        */
} mvhp_color_params_t;
/* out = {cy, crv, cbu, gcb, gcr, yoff}.  Host only.  MVHP_FAILURE: a matrix or range outside the values above. */
MVHP_EXPORT int    mvhp_color_coefficients(int matrix, int full_range, int32_t out[6]);
/* The parameters for pictures of `coded_w` x `coded_h` whose stream says `d` (NULL: nothing).  Host only.
 *   mode 0 (auto): matrix_coefficients 1 -> BT.709; 5 or 6 -> BT.601; anything else or absent -> BT.709 when coded_w >= 1280 or
 *     coded_h > 576, else BT.601 (GBR, YCgCo, BT.2020 and the other codes are not supported and take this fallback); full range
 *     from video_full_range_flag when the signal type is present, else limited;
 *   mode 1 .. 4: BT.601 limited, BT.709 limited, BT.601 full, BT.709 full, whatever the stream says;
 *   siting, every mode: chroma_loc even -> MVHP_CHROMA_LEFT, odd -> MVHP_CHROMA_CENTER (types 2..5 keep only their horizontal
 *     part: the vertical weights are those of types 0 and 1 -- an approximation).
 * MVHP_FAILURE: a mode outside 0..4 or no `out`. */
MVHP_EXPORT int    mvhp_color_resolve(const mvhp_display_info_t *d, uint32_t coded_w, uint32_t coded_h, int mode, mvhp_color_params_t *out);
/* n dense planar pictures of g->out_w x g->out_h (d_yuv, 4-byte aligned, as mvhp_resample_dev and mvhp_orient_dev leave them;
 * planes of the coded size go with a geometry of the coded size) -> n dense RGB8 pictures (d_rgb_out, 4-byte aligned).  Only
 * out_w and out_h of g are read.  n = 0 does nothing; n < 0, odd or zero sizes or sizes above 16384, enum values outside the
 * ones above, a non-zero `reserved` and misaligned or NULL pointers are refused (MVHP_FAILURE) before anything is launched.
 * Asynchronous on `stream` (NULL = the context's own).  Nothing is shared between workgroups, no kernel waits and nothing
 * survives a launch: safe under stream capture, and two calls on two streams do not meet. */
MVHP_EXPORT int    mvhp_color_dev(mvhp_ctx_t *ctx, const mvhp_output_geometry_t *g, const mvhp_color_params_t *params,
                                  const uint8_t *d_yuv, int n, uint8_t *d_rgb_out, void *stream);

/* ---------------------------------------------------------------------------
 * JPEG output (opt-in; DESIGN.md 3 "JPEG output"): baseline sequential JFIF files made on the device from planar pictures, the
 * planes taken as they are (Y 2x2, Cb and Cr 1x1, no colour conversion), as the reference's writer does with libjpeg
 * (export.c:341-430).  The stream format is fixed -- SOI, APP0 "JFIF" 1.01, one DQT (tables 0 and 1), SOF0, four DHT (the
 * Annex K.3 tables), DRI, SOS, entropy-coded data with RSTm, EOI -- and the transform is integer-only, so the bytes are a
 * function of the samples, the quality and the restart interval alone (tests/jpeg_ref.py restates them).
 * ------------------------------------------------------------------------- */
typedef struct mvhp_jpeg_params {
    int32_t  quality;        /* IJG quality, clamped to 1 .. 100: Annex K.1 / K.2 scaled by 5000 / q below 50, else 200 - 2 q   */
    uint32_t restart_mcus;   /* MCUs (16x16 luma) per restart interval, 1 .. 65535; 0 = one MCU row                            */
    uint32_t reserved;       /* 0.  Measurements only: MVHP_JPEG_STAGE_* bits run just those stages of a call made before with
                                the same arguments (its scratch buffer holds what they need).  The write stage checks every
                                table entry against cap_bytes again, so a stale table cannot send a store outside the blob  */
} mvhp_jpeg_params_t;
#define MVHP_JPEG_STAGE_DCT   1u   /* forward DCT + quantisation into the context's scratch buffer                           */
#define MVHP_JPEG_STAGE_COUNT 2u   /* count pass + the scans: writes the table                                              */
#define MVHP_JPEG_STAGE_WRITE 4u   /* write pass + headers: writes the blob                                                 */

#define MVHP_JPEG_OK      0u
#define MVHP_JPEG_TOO_BIG 1u       /* the picture did not fit into what was left of the blob: length 0, nothing written     */
typedef struct mvhp_jpeg_entry {
    uint64_t offset;         /* of the picture's file in the blob, a multiple of 16                                          */
    uint32_t length;         /* bytes of the file                                                                            */
    uint32_t status;         /* MVHP_JPEG_*                                                                                  */
} mvhp_jpeg_entry_t;

#define MVHP_JPEG_HEADER_BYTES 625
/* Bytes of a file before its entropy-coded data (every file of this encoder: the segments above have fixed sizes). */
MVHP_EXPORT size_t mvhp_jpeg_header_bytes(void);
/* The two quantisation tables of `quality`, luma then chroma, each in row-major order (the files carry them in zigzag
 * order).  A host function: needs no device. */
MVHP_EXPORT int    mvhp_jpeg_quant_tables(int quality, uint8_t out[128]);
/* n pictures of geometry g (d_yuv: n * mvhp_geometry_yuv_bytes(g), planar Y | Cb | Cr of g->out_w x g->out_h -- coded-size
 * planes with a geometry of the coded size, or what mvhp_resample_dev delivered; only out_w / out_h are read) -> n JPEG files in
 * d_blob (16-byte aligned, cap_bytes long) and d_table (n entries, 8-byte aligned).  Pictures are placed in order, each at the
 * next multiple of 16; a picture whose file would pass cap_bytes is marked MVHP_JPEG_TOO_BIG, takes no room, and those behind
 * it that fit are placed as if it were not there.  No byte at or beyond cap_bytes is written, nor any between a file's end and
 * the next file's start.  Pictures of more than 2^28 luma samples are refused (MVHP_UNSUPPORTED): lengths are 32-bit, and a
 * baseline file is at most 6.5 x its raw picture (26 bits of code and value per level, every byte stuffed).  Asynchronous on `stream` (NULL = the context's own); the intermediate data lives in a scratch buffer
 * of the context (136 bytes per 8x8 block), so two encodes of one context run one after the other, whatever their streams. */
MVHP_EXPORT int    mvhp_jpeg_encode_dev(mvhp_ctx_t *ctx, const mvhp_output_geometry_t *g, const mvhp_jpeg_params_t *params,
                                        const uint8_t *d_yuv, int n, uint8_t *d_blob, size_t cap_bytes,
                                        mvhp_jpeg_entry_t *d_table, void *stream);

/* ---------------------------------------------------------------------------
 * PNG output (opt-in; DESIGN.md 3 "PNG output"): compressed PNG files made on the device from dense RGB8 pictures.  The format
 * is fixed, so a file is a function of the samples alone (tests/png_ref.py restates it): signature, IHDR (8 bit, colour type 2,
 * no interlace), one IDAT per segment of mvhp_png_segment_rows(w) rows, IEND; every row filtered with the type (0 .. 4) whose
 * bytes have the least sum of min(f, 256 - f), ties to the lowest type; every segment one deflate block that starts on a byte,
 * Huffman-coded literals only (a dynamic block with a code built from the segment's own histogram), or a stored block where that
 * would not be shorter -- so no file is longer than mvhp_png_max_bytes(w, h).
 * ------------------------------------------------------------------------- */
typedef struct mvhp_png_params {
    uint32_t reserved;       /* 0.  Measurements only: MVHP_PNG_STAGE_* bits run just those stages of a call made before with the
                                same arguments (its scratch buffer holds what they need).  The write stage checks every table
                                entry against cap_bytes again, so a stale table cannot send a store outside the blob          */
} mvhp_png_params_t;
#define MVHP_PNG_STAGE_ANALYSE 1u  /* filter types, histograms, code lengths and chunk lengths into the context's scratch buffer */
#define MVHP_PNG_STAGE_PLACE   2u  /* the scans: writes the table                                                             */
#define MVHP_PNG_STAGE_WRITE   4u  /* write pass + signature, IHDR, IEND: writes the blob                                      */

#define MVHP_PNG_OK      MVHP_JPEG_OK
#define MVHP_PNG_TOO_BIG MVHP_JPEG_TOO_BIG   /* the picture did not fit into what was left of the blob: length 0, nothing written */
typedef mvhp_jpeg_entry_t mvhp_png_entry_t;  /* {offset, length, status}: the table of both encoders                               */

#define MVHP_PNG_HEADER_BYTES 33
#define MVHP_PNG_MAX_WIDTH 21844             /* 3 w + 1 <= 65535: a filtered row fits one stored block                           */
/* Bytes of a file before its first IDAT chunk (signature + IHDR). */
MVHP_EXPORT size_t mvhp_png_header_bytes(void);
/* Rows per segment: max(1, 32768 / (3 w + 1)); 0 for w < 1.  A host function: needs no device. */
MVHP_EXPORT int    mvhp_png_segment_rows(int w);
/* The longest file a w x h picture can give (every segment stored): 51 + 17 segments + h (3 w + 1); 0 for sizes below 1.  A
 * host function: needs no device. */
MVHP_EXPORT size_t mvhp_png_max_bytes(int w, int h);
/* n pictures of g->out_w x g->out_h (d_rgb: n * 3 * out_w * out_h bytes, dense RGB8, 4-byte aligned -- what the fused epilogue
 * leaves for a geometry of the coded size, or mvhp_resample_dev / mvhp_orient_dev; only out_w / out_h are read) -> n PNG files in
 * d_blob (16-byte aligned, cap_bytes long) and d_table (n entries, 8-byte aligned), placed by the rule of mvhp_jpeg_encode_dev:
 * in order, each at the next multiple of 16; a picture whose file would pass cap_bytes is marked MVHP_PNG_TOO_BIG, takes no room,
 * and those behind it that fit are placed as if it were not there.  No byte at or beyond cap_bytes is written, nor any between a
 * file's end and the next file's start.  n = 0 does nothing.  Refused before any launch (MVHP_FAILURE): n < 0, odd or zero sizes,
 * widths above MVHP_PNG_MAX_WIDTH, misaligned pointers; pictures of more than 2^28 samples are refused with MVHP_UNSUPPORTED
 * (lengths are 32-bit).  Asynchronous on `stream` (NULL = the context's own); filter types, code lengths and chunk lengths live in
 * a scratch buffer of the context (one byte per row, 304 bytes per segment), so two encodes of one context run one after the
 * other, whatever their streams.  Nothing is shared between workgroups but that buffer between launches, no kernel waits and
 * nothing survives the call: safe under stream capture once the scratch buffer has its size. */
MVHP_EXPORT int    mvhp_png_encode_dev(mvhp_ctx_t *ctx, const mvhp_output_geometry_t *g, const mvhp_png_params_t *params,
                                       const uint8_t *d_rgb, int n, uint8_t *d_blob, size_t cap_bytes, mvhp_png_entry_t *d_table,
                                       void *stream);

/* ---------------------------------------------------------------------------
 * Picture scores (opt-in; DESIGN.md 3 "Picture scores"): how much a picture shows, measured on the device as the variance of
 * its luma samples, so that a caller can pass over black lead-ins, fades and flat title cards (minivideo_decode does under
 * MINIVIDEO_SKIP_BLANK=1, include/minivideo.h).  The device sums; the score is integer arithmetic on the host.
 * ------------------------------------------------------------------------- */
typedef struct mvhp_luma_stats {   /* 32 bytes, 8-byte aligned */
    uint64_t sum;        /* of the luma samples of the rectangle   */
    uint64_t sumsq;      /* of their squares                       */
    uint32_t samples;    /* crop_w * crop_h (<= 2^28)              */
    uint32_t reserved[3];/* 0                                      */
} mvhp_luma_stats_t;
/* floor(16 (N Q - S^2) / N^2) with N = samples, S = sum, Q = sumsq: the luma variance in sixteenths, 0 ... 260100 (half the
 * samples 0, half 255).  128-bit integer arithmetic, no floating point; N = 0 gives 0.  This integer is the only form of the
 * score: thresholds compare it, ties are decided on it.  A host function: needs no device. */
MVHP_EXPORT uint32_t mvhp_luma_score(const mvhp_luma_stats_t *st);
/* Over a slot's candidates in order (the primary first): the index of the first whose score is at least min_score; if there
 * is none, of the largest score, the earliest on a tie.  n <= 0: -1.  A host function. */
MVHP_EXPORT int      mvhp_blank_choose(const uint32_t *scores, int n, uint32_t min_score);
/* n coded pictures (d_yuv_coded: mvhp_yuv_frame_bytes(p) apart, 16-byte aligned, luma pitch 16 W) -> n records in d_stats
 * (8-byte aligned), each over the luma rectangle crop_x, crop_y, crop_w, crop_h of g (all even, inside the coded picture, at
 * least 2 x 2; out_w / out_h are not read: the score is a property of the source picture, whatever size is delivered).  n = 0
 * does nothing; n < 0, a rectangle outside the picture, odd or zero sizes are refused (MVHP_FAILURE) before anything is
 * launched.  Asynchronous on `stream` (NULL = the context's own); the call zeroes the records on that stream itself.  Nothing
 * survives a launch and no kernel waits: safe under stream capture, and two calls on two streams do not meet. */
MVHP_EXPORT int      mvhp_luma_stats_dev(mvhp_ctx_t *ctx, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g,
                                         const uint8_t *d_yuv_coded, int n, mvhp_luma_stats_t *d_stats, void *stream);

/* ---------------------------------------------------------------------------
 * Black bars (opt-in; DESIGN.md 3 "Black bars"): where the content of a letterboxed or pillarboxed picture lies, found on the
 * device by counting, so that a caller can trim the bars (minivideo_decode does under MINIVIDEO_TRIM=1, include/minivideo.h).
 * A sample is bright when Y > level (1 ... 254; 24 = video black 16 plus noise).  Row y of a rectangle cw x ch is content when at
 * least mvhp_bars_need(cw) of its samples are bright, column x when at least mvhp_bars_need(ch) of its samples are.  Integers
 * only: a record is a function of the samples alone.  Bars are a property of the stream, not of a picture (a dark scene has no
 * edge): a caller probes a few pictures, unites their boxes (mvhp_bars_union), lets mvhp_trim_rect decide whether to trust the
 * union and hands it to the stream (mvhp_stream_set_trim), where MVHP_OUTPUT_TRIM applies it to every picture alike.
 * ------------------------------------------------------------------------- */
typedef struct mvhp_luma_bars {   /* 32 bytes, 8-byte aligned */
    uint32_t x, y, w, h;          /* box of the content rows / columns, luma samples, CODED-picture coordinates: x the first content
                                     column, x + w - 1 the last, likewise rows (the box spans first to last: bars in the middle of
                                     a picture are not bars); w = h = 0 (and x = y = 0): no content row or no content column */
    uint32_t rows, cols;          /* how many rows / columns of the rectangle are content (they need not be contiguous); reported
                                     also for an empty box */
    uint32_t reserved[2];         /* 0 */
} mvhp_luma_bars_t;
#define MVHP_BARS_LEVEL_DEFAULT 24
/* max(1, len >> 5): bright samples that make a row of `len` samples (a column of `len` rows) content.  A host function. */
MVHP_EXPORT uint32_t mvhp_bars_need(uint32_t len);
/* The smallest box that holds every non-empty box of b[0..n) into *out (rows = cols = 0; empty when there is none); returns the
 * number of non-empty boxes.  Commutative: the order of b does not matter.  A host function. */
MVHP_EXPORT int      mvhp_bars_union(const mvhp_luma_bars_t *b, int n, mvhp_luma_bars_t *out);
/* The trim rule.  `u` is intersected with the rectangle crop_* of `crop` (even, as every crop is); the left and top edge move
 * down to even, the right and bottom edge up to even (the result stays inside the crop); the trimmed rectangle is accepted only
 * when its width is at least (cw + 1) / 2 and its height at least (ch + 1) / 2 -- a detection that would throw away more than
 * half of a side is a dark scene, not a bar.  Accepted: out->crop_* is the trimmed rectangle, returns 1.  Otherwise (also for an
 * empty u or an empty intersection): out->crop_* is the crop, returns 0.  Either way out_w / out_h = crop_w / crop_h and
 * reserved = 0; out may be crop.  A host function. */
MVHP_EXPORT int      mvhp_trim_rect(const mvhp_output_geometry_t *crop, const mvhp_luma_bars_t *u, mvhp_output_geometry_t *out);
/* The stream carries one box in coded coordinates, read only by mvhp_output_geometry under MVHP_OUTPUT_TRIM: setting it changes
 * nothing by itself.  u == NULL or an empty box clears it.  mvhp_stream_trim copies it out (empty when none is set).  Not
 * thread-safe against a decode call that runs on the stream: set it between calls. */
MVHP_EXPORT int      mvhp_stream_set_trim(mvhp_stream_t *s, const mvhp_luma_bars_t *u);
MVHP_EXPORT int      mvhp_stream_trim(const mvhp_stream_t *s, mvhp_luma_bars_t *out);
/* n coded pictures (d_yuv_coded: mvhp_yuv_frame_bytes(p) apart, 16-byte aligned, luma pitch 16 W) -> n records in d_bars (8-byte
 * aligned), each over the luma rectangle crop_x, crop_y, crop_w, crop_h of g (all even, inside the coded picture, at least
 * 2 x 2; out_w / out_h are not read).  n = 0 does nothing; a level outside 1 ... 254, n < 0, a rectangle outside the picture, odd
 * or zero sizes and NULL or misaligned pointers are refused (MVHP_FAILURE) before anything is launched.  Asynchronous on `stream`
 * (NULL = the context's own).  The row and column counters live in a scratch buffer of the context (4 (cw + ch) bytes per
 * picture), which the call zeroes on that stream itself: two calls of one context run one after the other, whatever their
 * streams.  No kernel waits and nothing survives the call but the records: safe under stream capture once the scratch buffer
 * has its size. */
MVHP_EXPORT int      mvhp_luma_bars_dev(mvhp_ctx_t *ctx, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g,
                                        const uint8_t *d_yuv_coded, int n, int level, mvhp_luma_bars_t *d_bars, void *stream);

/* ---------------------------------------------------------------------------
 * Representative pictures (opt-in; DESIGN.md 3 "Representative pictures"): the histograms of the three planes of a picture's
 * rectangle, counted on the device, so that a caller can keep, among a handful of candidates, the one that looks most like all
 * of them (minivideo_decode does under MINIVIDEO_REPRESENTATIVE=1, include/minivideo.h).  The device counts; the choice is
 * integer arithmetic on the host.
 * ------------------------------------------------------------------------- */
typedef struct mvhp_plane_hist {   /* 3104 bytes, 16-byte aligned */
    uint32_t y[256], cb[256], cr[256];   /* counts of the samples of the rectangle, per value */
    uint32_t samples;                    /* crop_w * crop_h (<= 2^28)                          */
    uint32_t chroma_samples;             /* (crop_w / 2) * (crop_h / 2)                        */
    uint32_t reserved[6];                /* 0                                                  */
} mvhp_plane_hist_t;
/* The picture-score record of the same rectangle, from the luma histogram: sum = sum of v y[v], sumsq = sum of v^2 y[v],
 * samples = sum of y[v], reserved = 0 -- the 32 bytes mvhp_luma_stats_dev writes for that rectangle, so mvhp_luma_score of it is
 * the picture's blank score and one probe serves both features.  A host function. */
MVHP_EXPORT int      mvhp_hist_stats(const mvhp_plane_hist_t *h, mvhp_luma_stats_t *out);
/* The candidate that looks most like all of them.  The candidates are the entries of h[0..n) that are eligible (eligible[i] != 0;
 * NULL = all) and whose samples and chroma_samples equal those of the first eligible entry (entry 0, the primary, when it is
 * eligible).  With k candidates and M[b] the sum of their counts in bin b, over all 768 bins of the three planes,
 * D_i = sum over b of (k h_i[b] - M[b])^2 -- k^2 times the squared distance to the mean histogram, in 128-bit integers (counts up
 * to 2^28 and k up to 17 stay far inside them) -- and the function returns the index of the smallest D, the earliest on a tie: the
 * first candidate for k = 1 and k = 2.  No eligible entry, n <= 0 or h == NULL: -1.  A host function. */
MVHP_EXPORT int      mvhp_represent_choose(const mvhp_plane_hist_t *h, int n, const uint8_t *eligible);
/* n coded pictures (d_yuv_coded: mvhp_yuv_frame_bytes(p) apart, 16-byte aligned, luma pitch 16 W, chroma pitch 8 W) -> n records
 * in d_hist (16-byte aligned): y over the luma rectangle crop_x, crop_y, crop_w, crop_h of g (all even, inside the coded picture,
 * at least 2 x 2; out_w / out_h are not read), cb and cr over the same rectangle halved.  n = 0 does nothing; n < 0, a rectangle
 * outside the picture, odd or zero sizes and NULL or misaligned pointers are refused (MVHP_FAILURE) before anything is launched.
 * Asynchronous on `stream` (NULL = the context's own); the call zeroes the records on that stream itself.  Nothing survives a
 * launch and no kernel waits: safe under stream capture, and two calls on two streams do not meet. */
MVHP_EXPORT int      mvhp_plane_hist_dev(mvhp_ctx_t *ctx, const mvhp_stream_params_t *p, const mvhp_output_geometry_t *g,
                                         const uint8_t *d_yuv_coded, int n, mvhp_plane_hist_t *d_hist, void *stream);

/* ---------------------------------------------------------------------------
 * Tensor output (opt-in; DESIGN.md 3 "Tensor output"): dense RGB8 pictures -> a batch tensor of one fixed shape, in the caller's
 * element type and layout, normalised and padded on the device, so that what a model reads never leaves it.
 *
 * Arithmetic, the whole contract: a sample c (0 .. 255) of colour k becomes fmaf((float)c, scale[k], bias[k]) -- one IEEE
 * binary32 fused multiply-add, one rounding -- stored as it is (F32) or rounded to nearest-even to binary16 (F16) or bfloat16
 * (BF16).  Subnormal results are kept in all three types; F16 overflows to infinity as IEEE says.
 * Placement: the picture sits at ox = (canvas_w - src_w) / 2, oy = (canvas_h - src_h) / 2 of the canvas (floor division);
 * every other element is the value of pad_rgb's sample of its colour under the same arithmetic.  NCHW is three planes of
 * canvas_h x canvas_w, NHWC interleaved; MVHP_TENSOR_BGR puts the planes / the interleave in the order B, G, R (scale, bias and
 * pad_rgb stay indexed by colour).  Out of scope: enlarging, a "cover" crop, canvases per picture, picture files.
 * ------------------------------------------------------------------------- */
#define MVHP_TENSOR_F32 0
#define MVHP_TENSOR_F16 1
#define MVHP_TENSOR_BF16 2
#define MVHP_TENSOR_NCHW 0
#define MVHP_TENSOR_NHWC 1
#define MVHP_TENSOR_BGR  1u          /* flags: channel planes / interleave order B,G,R instead of R,G,B */
typedef struct mvhp_tensor_params {
    uint32_t src_w, src_h;           /* dense RGB8 pictures in, as every RGB path of the library leaves them (1..16384) */
    uint32_t canvas_w, canvas_h;     /* tensor H x W; 0,0 = src size; each >= src side, <= 16384, odd allowed */
    uint32_t dtype, layout, flags;
    uint32_t pad_rgb;                /* 0x00RRGGBB: colour of the canvas outside the picture */
    float    scale[3], bias[3];      /* per R, G, B (indexed by colour, not by output position) */
} mvhp_tensor_params_t;
/* Bytes of one picture's tensor (3 x canvas_h x canvas_w elements); 0 = bad parameters (an enum value outside those above, an
 * unknown flag bit, a side of 0 or above 16384, one canvas side 0 and the other not, a canvas smaller than the picture).  A host
 * function. */
MVHP_EXPORT size_t   mvhp_tensor_bytes(const mvhp_tensor_params_t *t);
/* The usual normalisation (x / 255 - mean) / std as scale and bias: in double, scale = 1 / (255 std), bias = -mean / std, each
 * then converted to float.  MVHP_FAILURE for std == 0 and for non-finite input.  A host function. */
MVHP_EXPORT int      mvhp_tensor_constants(const double mean[3], const double std[3], float scale[3], float bias[3]);
/* n pictures in d_rgb (3 src_w src_h bytes apart, 4-byte aligned) -> n tensors: picture i at d_out + slot *
 * mvhp_tensor_bytes(t), slot = d_slots ? d_slots[i] : i (d_slots: device memory; a negative slot skips the picture); d_out is
 * 16-byte aligned.  n = 0 does nothing.  Refused (MVHP_FAILURE, mvhp_last_error() names the argument) before anything is
 * launched: parameters mvhp_tensor_bytes refuses, non-finite scale / bias, n < 0, NULL or misaligned pointers.  Asynchronous on
 * `stream` (NULL = the context's own); nothing is shared between workgroups or launches: safe under stream capture.  More than
 * 65535 pictures take a second launch. */
MVHP_EXPORT int      mvhp_tensor_dev(mvhp_ctx_t *ctx, const mvhp_tensor_params_t *t, const uint8_t *d_rgb, int n, void *d_out,
                                     const int32_t *d_slots /* may be NULL */, void *stream);

/* Page-locked host memory for the host-buffer entry points (H2D / D2H at full PCIe rate). */
MVHP_EXPORT void *mvhp_host_alloc(size_t bytes);
MVHP_EXPORT void  mvhp_host_free(void *p);

/* Wait for `stream` (NULL = context stream) and report any error the kernels
 * flagged since the last check. */
MVHP_EXPORT int  mvhp_sync_check(mvhp_ctx_t *ctx, void *stream);

/* Host-buffer convenience: H2D, reconstruct, D2H, synchronise. */
MVHP_EXPORT int  mvhp_recon_batch_host(mvhp_ctx_t *ctx, const mvhp_stream_params_t *p,
                                       const void *h_packed, int n_frames,
                                       uint8_t *h_yuv, uint8_t *h_rgb);

/* Test hook: the next launch of a banded kernel form hands out its work units `delta` off (see hotpath_abi.hip).  Never in products. */
MVHP_EXPORT int  mvhp_debug_skew_next_ticket_base(mvhp_ctx_t *ctx, int delta);

/* Test hook: waits for every launch issued on the context, then sets the ticket counter of the banded kernel forms (the device
 * word and the host's mirror of it) to `ticket` and the epoch tag of the last banded launch to `epoch`: the next banded launch
 * hands out its units from `ticket` and tags its seams epoch + 1 -- or, after 0xFFFFFFFF, zeroes the seams and starts again at 1.
 * The seam buffer is left as it is, tags of earlier launches included.  Never in products. */
MVHP_EXPORT int  mvhp_debug_set_wide_state(mvhp_ctx_t *ctx, uint32_t ticket, uint32_t epoch);

/* Test hook: waits in the same way, then reports the device's ticket counter, the host's mirror of it (equal once every banded
 * launch has run: one ticket per workgroup), the epoch tag of the last banded launch and the size of the seam buffer.  Any out
 * pointer may be NULL.  Never in products. */
MVHP_EXPORT int  mvhp_debug_get_wide_state(mvhp_ctx_t *ctx, uint32_t *device_ticket, uint32_t *ticket_base, uint32_t *epoch,
                                           size_t *seam_bytes);

/* What the last reconstruction launch of this context used (speed-only choices of the launch planner, see mvhp_plan_launch):
 * *layout = the kernel form that ran, MVHP_LAYOUT_ROWS .. MVHP_LAYOUT_PIPE1 (never MVHP_LAYOUT_AUTO); *waves = wavefronts per
 * workgroup (ROWS, QUAD, OCT) or macroblock rows per band (WIDE, QUAD_WIDE; PIPE, PIPE1: three wavefronts per row).  Either
 * pointer may be NULL. */
MVHP_EXPORT int  mvhp_last_launch_info(const mvhp_ctx_t *ctx, int *layout, int *waves);

/* 1 (default): the reconstruction kernel converts to RGB in its epilogue when d_rgb is given;
 * 0: a separate colour kernel reads the planes back.  Speed only, never results. */
MVHP_EXPORT int  mvhp_set_fused_color(mvhp_ctx_t *ctx, int on);

/* 1 (default): mvhp_resample_dev runs geometries with out_w == crop_w and out_h == crop_h (crop only) on the copy kernel
 * (global memory to global memory, no LDS row buffers: their width limit does not apply); 0: on the general resample kernel,
 * for which such a geometry is one tap of 2^14 per axis, i.e. the same bytes.  Speed only, never results. */
MVHP_EXPORT int  mvhp_set_crop_copy(mvhp_ctx_t *ctx, int on);

/* Test-only knob, like the tuning knobs below (speed only, never results; not meant for products): luma rows per workgroup of
 * mvhp_luma_stats_dev, 1 ... 65536; 0 (default) = sixteen, fewer when the grid would leave compute units idle.  It exists so that
 * a test can force band sizes and compare the records: the sums are integers, every value gives the same 32 bytes. */
MVHP_EXPORT int  mvhp_set_stats_band(mvhp_ctx_t *ctx, int rows);

/* Test-only knob, like the one above (speed only, never results; not meant for products): luma rows per workgroup of the counting
 * pass of mvhp_luma_bars_dev, 1 ... 65536; 0 (default) = choose from the batch (few, tall bands where there are many pictures,
 * short ones where the grid would leave compute units idle).  It exists so that a test can force band sizes and compare the
 * records: the counts are integers, every value gives the same 32 bytes. */
MVHP_EXPORT int  mvhp_set_bars_band(mvhp_ctx_t *ctx, int rows);

/* Test-only knob, like the two above (speed only, never results; not meant for products): luma rows per workgroup of
 * mvhp_plane_hist_dev, 1 ... 65536; 0 (default) = 256, fewer when the grid would leave compute units idle.  It exists so that a
 * test can force band sizes and compare the records: the counts are integers, every value gives the same 3104 bytes. */
MVHP_EXPORT int  mvhp_set_hist_band(mvhp_ctx_t *ctx, int rows);

/* Test-only knob, like those above (speed only, never results; not meant for products): canvas rows per workgroup of
 * mvhp_tensor_dev, 1 ... 16384 (cut down to what a workgroup's LDS holds of the source); 0 (default) = about 16 KiB of source and
 * at most 64 KiB of tensor, fewer when the grid would leave compute units idle.  It exists so that a test can force strip sizes
 * and compare the bytes: every element is made by one lane from its own sample, every value gives the same tensor. */
MVHP_EXPORT int  mvhp_set_tensor_rows(mvhp_ctx_t *ctx, int rows);

/* Tuning knob (speed only, never results): waves per picture workgroup, or macroblock rows per band of the banded forms
 * (1, 2, 4, 6, 8, 12 or 16; a layout that is not built for the value takes the next smaller one it is built for, or its
 * smallest); 0 = choose from batch size. */
MVHP_EXPORT int  mvhp_set_waves_per_picture(mvhp_ctx_t *ctx, int waves);

/* Tuning knob (speed only, never results): how pictures map onto workgroups, seven kernel forms.
 * MVHP_LAYOUT_AUTO chooses among all seven from the device's size, the picture shape, the flags and the batch size
 * (mvhp_plan_launch says what it would take).  A forced form that cannot run a batch -- line buffers that do
 * not fit in LDS, pictures with slices / scaling matrices on a form other than ROWS, WIDE or PIPE1 -- is replaced by the next
 * one that can.
 * MVHP_LAYOUT_ROWS: one picture per workgroup, one wavefront per macroblock row; MVHP_LAYOUT_QUAD: four pictures per
 * workgroup, 16 lanes per picture (fewer instructions per macroblock; a full round is 4 x CUs pictures); MVHP_LAYOUT_OCT:
 * eight pictures per workgroup, 8 lanes per picture (fewest instructions; whole rounds of 8 x CUs pictures). */
#define MVHP_LAYOUT_AUTO 0
#define MVHP_LAYOUT_ROWS 1
#define MVHP_LAYOUT_QUAD 2
#define MVHP_LAYOUT_OCT  3
/* The "wide" forms spread ONE picture (one group of four) over several workgroups -- bands of macroblock rows on different
 * CUs, the rows between two bands handed over through global memory -- so that a handful of pictures fills the chip:
 * MVHP_LAYOUT_WIDE = the one-picture kernel in bands (High batches between PIPE1's and QUAD_WIDE's ranges; larger batches
 * with slices / scaling matrices), MVHP_LAYOUT_QUAD_WIDE = the four-picture kernel in bands (up to about a round of QUAD,
 * and ragged batches beyond one). */
#define MVHP_LAYOUT_WIDE      4
#define MVHP_LAYOUT_QUAD_WIDE 5
/* MVHP_LAYOUT_PIPE: four pictures over several workgroups as QUAD_WIDE, and every macroblock row worked on by THREE wavefronts
 * in a pipeline (residuals / prediction / write-out): the shortest macroblock step, i.e. the lowest latency of a small batch. */
#define MVHP_LAYOUT_PIPE      6
/* MVHP_LAYOUT_PIPE1: the same pipeline with ONE picture per wavefront (nothing runs in lock step with another picture): the
 * lowest latency of a handful of pictures on any profile; also reconstructs slices / scaling matrices. */
#define MVHP_LAYOUT_PIPE1     7
#define MVHP_LAYOUT_COUNT     8
MVHP_EXPORT int  mvhp_set_layout(mvhp_ctx_t *ctx, int layout);

typedef struct mvhp_plan_device {
    int32_t  n_cus;            /* compute units                                                      */
    uint64_t max_lds_bytes;    /* LDS a workgroup may use                                            */
    int32_t  layout;           /* forced MVHP_LAYOUT_*, MVHP_LAYOUT_AUTO = choose                    */
    int32_t  waves;            /* forced value of mvhp_set_waves_per_picture, 0 = choose             */
} mvhp_plan_device_t;
/* What a reconstruction launch of n_frames pictures would run on: exactly one of ctx / dev is non-NULL (ctx: that context's
 * device and forced settings).  Pure host arithmetic: needs no HIP device, launches nothing.  Speed only. */
MVHP_EXPORT int  mvhp_plan_launch(const mvhp_ctx_t *ctx, const mvhp_plan_device_t *dev, const mvhp_stream_params_t *p,
                                  int n_frames, int *layout, int *waves);

/* ---------------------------------------------------------------------------
 * Decode engine: the whole split path as one pipelined call --
 *   host threads entropy-decode pictures (h264.c:76-188 NAL loop, h264_slice.c:1046-1139 macroblock loop)
 *   into page-locked chunks -> H2D -> batched reconstruction kernel -> D2H into page-locked chunks ->
 *   `sink` called once per picture, in the order of `order` (export.c:618-767 is what minivideo_decode's sink does).
 * Pictures are independent, so contexts (one per HIP device; several per device when `contexts` exceeds the
 * device count, e.g. to exercise the multi-device path on one GPU) pull whole batches from one queue; no collective.
 * A batch that fails on one context is entropy-decoded again and re-queued once to another context.
 * ------------------------------------------------------------------------- */
typedef struct mvhp_engine mvhp_engine_t;

typedef struct mvhp_engine_opts {
    int32_t contexts;        /* 0 = one per visible HIP device (env MINIVIDEO_GPUS caps it, MINIVIDEO_FAKE_GPUS sets it) */
    int32_t host_threads;    /* entropy threads; 0 = hardware concurrency (env MINIVIDEO_HOST_THREADS)                */
    int32_t batch_pictures;  /* pictures per kernel launch; 0 = auto (device fill, memory budget)  (MINIVIDEO_BATCH)  */
    int32_t chunk_pictures;  /* pictures per H2D / D2H transfer; 0 = auto (~64 MiB of records)                       */
    int32_t fail_context;    /* test hook: the first batch launched on this context reports a failure; -1 = off       */
    int32_t first_device;    /* context k runs on HIP device (first_device + k) % device count (one process per GPU:  */
                             /* contexts = 1, first_device = LOCAL_RANK)                                              */
    int32_t reserved[2];     /* [0] bit 0: the contexts' batch buffers come from one placed arena each (mvhp_placed_alloc_sets;
                                also env MINIVIDEO_PLACED=1) -- for engines that live long: the arena takes seconds to get */
} mvhp_engine_opts_t;

typedef struct mvhp_decode_stats {
    uint32_t pictures_issued;      /* pictures handed to the entropy stage (a re-queued picture counts twice)       */
    uint32_t pictures_ok;          /* pictures the sink accepted                                                     */
    uint32_t pictures_failed;      /* parse / device / sink failures delivered to the sink                           */
    uint32_t batches;              /* kernel launches                                                                */
    uint32_t batches_requeued;     /* batches that failed on one context and were re-queued to another               */
    uint32_t contexts;
    uint32_t host_threads;
    uint32_t launches_by_layout[4];/* indexed by MVHP_LAYOUT_AUTO .. MVHP_LAYOUT_OCT; the wide forms: launches_wide below   */
    uint32_t max_batch_pictures;
    double   wall_s;               /* whole call                                                                     */
    double   entropy_busy_s;       /* summed over host threads                                                       */
    double   h2d_s, kernel_s, d2h_s; /* device-side durations (HIP events), summed over contexts                     */
    double   sink_s;               /* time inside the sink callback                                                  */
    uint64_t stream_bytes;         /* NAL bytes entropy-decoded                                                      */
    uint64_t h2d_bytes, d2h_bytes;
    /* where a COLD call's time goes (an engine keeps its pools: the second call of the same shape allocates nothing)  */
    double   host_alloc_s;         /* page-locking host memory (summed over the threads that did it)                 */
    double   dev_alloc_s;          /* device allocations                                                             */
    double   first_launch_s;       /* the first reconstruction call of each context: code-object load + first launch */
    double   first_picture_s;      /* from the call to the first picture at the sink                                 */
    uint64_t host_alloc_bytes, dev_alloc_bytes;
    uint32_t placed_buffers;       /* 1: the device batch buffers come from mvhp_placed_alloc (MINIVIDEO_PLACED=1)   */
    uint32_t geometry_launches;    /* launches that ran the output-geometry pass behind the reconstruction (mvhp_engine_decode_ex
                                      with a request that changes the picture); 0 on the coded-size path                      */
    uint32_t launches_wide[4];     /* launches on MVHP_LAYOUT_WIDE, _QUAD_WIDE, _PIPE, _PIPE1 (launches_by_layout: 0..3)   */
} mvhp_decode_stats_t;

/* Called on the calling thread, once per picture, in the order of `order`.  rc = MVHP_SUCCESS: yuv (and rgb when
 * asked for) point into page-locked memory valid during the call.  Otherwise yuv = rgb = NULL and err says why.
 * Return 1: picture accepted (counts towards `wanted`); 0: not accepted (counts as a failure); -1: stop decoding;
 * 2: accepted AND kept -- yuv / rgb stay valid after the call returns, until mvhp_engine_release_picture(e, seq), which any
 * thread may call (a pool of file writers: minivideo_decode).  Kept pictures occupy the engine's output chunks, so keep few
 * (the pipeline waits for a free chunk); mvhp_engine_decode does not return before the last kept picture has been released. */
typedef int (*mvhp_picture_sink_t)(void *user, int seq, int idr, int rc, const char *err,
                                   const mvhp_stream_params_t *p, const uint8_t *yuv, const uint8_t *rgb);

MVHP_EXPORT int  mvhp_engine_create(const mvhp_engine_opts_t *opts /* may be NULL */, mvhp_engine_t **out);
MVHP_EXPORT void mvhp_engine_destroy(mvhp_engine_t *e);
/* `want_rgb` of mvhp_engine_decode: 0 = planes only; MVHP_OUT_RGB = planes and RGB; MVHP_OUT_RGB_ONLY = RGB only (the planes
 * are still reconstructed on the device -- RGB is made from them -- but not downloaded: the sink gets yuv = NULL). */
#define MVHP_OUT_RGB      1
#define MVHP_OUT_RGB_ONLY 3
/* mvhp_engine_decode_ex only (opt-in; "JPEG output" above): neither planes nor RGB are downloaded; every picture is coded on the
 * device by mvhp_jpeg_encode_dev behind the reconstruction (and the deblocking filter and the geometry pass, where the stream
 * and the request ask for them), and only the files come back.  The sink gets yuv = NULL, rgb = the picture's JPEG file and
 * g->reserved[0] = its length in bytes.  The encoder's parameters travel in mvhp_output_request_t::reserved: bits 0-7 the
 * quality (0 = 75, above 100 = 100), bits 8-23 restart_mcus (0 = one MCU row); a request with flags 0 still means pictures of the
 * coded size.  A batch's blob has room for n x mvhp_geometry_yuv_bytes(g): a picture whose file does not fit into it (larger
 * than the raw picture: of no use) reaches the sink as a failed picture, and decoding goes on.  d2h_bytes counts the table
 * entries (16 bytes per picture) and the files' bytes. */
#define MVHP_OUT_JPEG     4
#define MVHP_JPEG_REQUEST(quality, restart_mcus) (((uint32_t)(quality) & 0xffu) | (((uint32_t)(restart_mcus) & 0xffffu) << 8))
/* mvhp_engine_decode_ex only (opt-in; "PNG output" above): neither planes nor RGB are downloaded; every picture's RGB -- the fused
 * epilogue's where the picture is of the coded size, else what the geometry and orientation passes deliver -- is coded on the
 * device by mvhp_png_encode_dev, and only the files come back.  The sink gets yuv = NULL, rgb = the picture's PNG file and
 * g->reserved[0] = its length in bytes.  A batch's blob has room for n x mvhp_png_max_bytes(out_w, out_h) (rounded to 16), so no
 * picture can be too big.  d2h_bytes counts the table entries (16 bytes per picture) and the files' bytes.  Not together with
 * MVHP_OUT_JPEG. */
#define MVHP_OUT_PNG      8
/* mvhp_engine_decode_ex only (opt-in; "Tensor output" above): the batch's RGB is made exactly as for MVHP_OUT_RGB_ONLY under the
 * same request (crop, box, aspect, trim, turn and MVHP_OUTPUT_COLOR all apply), mvhp_tensor_dev runs behind it with src_w x src_h
 * = the geometry's out_w x out_h, and neither planes nor RGB are downloaded.  The parameters are those of the last
 * mvhp_engine_set_tensor (read at the start of the call; without one the call fails).  canvas 0,0: every tensor has its picture's
 * size; a picture larger than a non-zero canvas reaches the sink as a failed picture, and decoding goes on.
 * Host delivery (d_target NULL): only the tensors are downloaded; the sink gets yuv = NULL, rgb = the tensor's bytes and
 * g->reserved[0] = their length; d2h_bytes grows by exactly mvhp_tensor_bytes per delivered picture.
 * Device delivery (d_target: device memory of target_pictures tensors, 16-byte aligned): the tensor of picture `seq` is written
 * straight to d_target + seq * mvhp_tensor_bytes, nothing of the picture is downloaded, and the sink is called with yuv = rgb =
 * NULL and g->reserved[0] = the length once the batch's kernels have completed.  A failed picture leaves its slot untouched;
 * seq >= target_pictures fails that picture.  It needs an engine of exactly one context -- the pointer belongs to one device --
 * and, for the slots to be of one size, a non-zero canvas or pictures of one geometry.
 * Not together with MVHP_OUT_JPEG, MVHP_OUT_PNG or MVHP_OUTPUT_BARS (g->reserved[0]); composes with MVHP_OUTPUT_SCORE and
 * MVHP_OUTPUT_HIST. */
#define MVHP_OUT_TENSOR   16
typedef struct mvhp_tensor_request {
    uint32_t canvas_w, canvas_h, dtype, layout, flags, pad_rgb;   /* as in mvhp_tensor_params_t */
    float scale[3], bias[3];
    void *d_target; uint32_t target_pictures; uint32_t reserved;  /* reserved: 0 */
} mvhp_tensor_request_t;
/* MVHP_OUTPUT_SCORE in mvhp_output_request_t::flags (mvhp_engine_decode_ex only; composes with MVHP_OUTPUT_CROP / _BOX and every
 * output kind above): behind whatever reconstructs the batch (and the deblocking filter, where the stream asks for it)
 * mvhp_luma_stats_dev sums the coded planes over each picture's crop rectangle, the 32-byte records come back with the
 * pictures, and the sink finds g->reserved[1] = mvhp_luma_score of the picture's record (g->reserved[0] stays the JPEG length).
 * Without the flag g->reserved[1] is 0 and there is no extra launch, buffer or byte; with it d2h_bytes grows by exactly 32 per
 * delivered picture.  The pictures themselves are the same bytes either way. */
/* Decode the pictures order[0..n_order) of `s` (IDR indices) until `wanted` of them have been accepted by the sink
 * (the reference stops after picture_number IDRs, h264.c:173-179: no more pictures than needed are entropy-decoded).
 * sink may be NULL (every reconstructed picture counts as accepted).  Returns MVHP_SUCCESS when `wanted` pictures
 * were accepted, or when the list ended after at least one. */
MVHP_EXPORT int  mvhp_engine_decode(mvhp_engine_t *e, const mvhp_stream_t *s, const int *order, int n_order, int wanted,
                                    int want_rgb, mvhp_picture_sink_t sink, void *user, mvhp_decode_stats_t *stats);
/* The same with an output request (see "Output geometry" above; NULL or flags 0 = the coded size) and a sink that also gets
 * the picture's geometry: yuv holds mvhp_geometry_yuv_bytes(g), rgb mvhp_geometry_rgb_bytes(g).  mvhp_engine_decode is this
 * call with req = NULL.  A batch holds pictures of one set of stream parameters and ONE geometry: a stream whose SPS crop
 * changes from picture to picture is decoded in small batches.  Where the geometry of a picture equals the coded size (no
 * SPS crop, no box or a box that already contains the picture) the engine takes the path of mvhp_engine_decode exactly;
 * otherwise the batch is reconstructed without the fused colour epilogue, deblocked when the stream asks for it, passed
 * through mvhp_resample_dev on the device, and only the output pictures are downloaded (stats: geometry_launches).  A picture
 * whose geometry cannot be formed (the SPS crop leaves nothing) reaches the sink as a failed picture (g all zero, err says
 * why); decoding goes on. */
typedef int (*mvhp_picture_sink_ex_t)(void *user, int seq, int idr, int rc, const char *err, const mvhp_stream_params_t *p,
                                      const mvhp_output_geometry_t *g, const uint8_t *yuv, const uint8_t *rgb);
MVHP_EXPORT int  mvhp_engine_decode_ex(mvhp_engine_t *e, const mvhp_stream_t *s, const int *order, int n_order, int wanted,
                                       int want_rgb, const mvhp_output_request_t *req, mvhp_picture_sink_ex_t sink, void *user,
                                       mvhp_decode_stats_t *stats);
/* Gives back a picture the sink kept (verdict 2) during the running mvhp_engine_decode call; anything else is ignored. */
MVHP_EXPORT void mvhp_engine_release_picture(mvhp_engine_t *e, int seq);
/* MVHP_OUTPUT_HIST: the record of picture `seq` of the running call.  Valid inside the sink call for `seq`, and for a picture the
 * sink kept (verdict 2) until mvhp_engine_release_picture; NULL without the flag, for a failed picture and at any other time. */
MVHP_EXPORT const mvhp_plane_hist_t *mvhp_engine_picture_hist(mvhp_engine_t *e, int seq);
/* The tensor request of the MVHP_OUT_TENSOR calls that follow (copied; NULL clears it).  Malformed requests -- what
 * mvhp_tensor_bytes refuses for a picture of the canvas's size, non-finite scale / bias, reserved != 0, a misaligned d_target or
 * one without target_pictures -- are refused (MVHP_FAILURE).  Not while a decode call is running. */
/* The number of device contexts the engine runs (what mvhp_decode_stats_t::contexts reports after a call). */
MVHP_EXPORT int  mvhp_engine_contexts(mvhp_engine_t *e);
MVHP_EXPORT int  mvhp_engine_set_tensor(mvhp_engine_t *e, const mvhp_tensor_request_t *t /* NULL clears */);

/* ---- memory placement (MI355X: device memory alternates, in regions of tens of GB, between two halves of the memory
 * system; DESIGN.md 3 "Placement") ---- */
/* Time concurrent streaming writes over two device windows of `bytes` each (both are overwritten): two windows in the
 * same half take about twice as long per pass as two windows in different halves. */
MVHP_EXPORT int  mvhp_probe_pair(int device, void *d_a, void *d_b, size_t bytes, int reps, float *ms_per_pass);
/* `count` (<= 8) device buffers of at least bytes[i] inside ONE allocation (arena_bytes = 0: what is free less 24 GB, at most
 * 200 GB or MVHP_PLACED_ARENA_GB from the environment), placed -- as far as the arena shows several groups -- so that every buffer lies in a group of its own, the largest
 * choosing first: records, planes and RGB of a batch in three different groups is the fastest placement there is
 * (tools/placement_predict.py).  For long-lived batch buffers: the large allocation takes seconds (the driver clears it).
 * groups_of[i] (may be NULL): group of buffer i, -1 = straddles; *groups_found (may be NULL): groups seen in the arena.
 * MVHP_FAILURE: not enough memory -- use ordinary allocations. */
MVHP_EXPORT int  mvhp_placed_alloc(int device, int count, const size_t *bytes, size_t arena_bytes, void **d_ptrs, void **arena,
                                   int *groups_of, int *groups_found);
/* The same for a pipeline's batch buffers: `sets` copies of `count` (<= 8) buffers, d_ptrs[s * count + i] = buffer i of set s;
 * buffer i of every set lies in the group chosen for i (a launch reads / writes the buffers of ONE set: its records, planes and
 * RGB are in three different groups); any_group[i] != 0 (may be NULL = none): buffer i goes wherever room is left.  At most
 * four buffers may ask for a group of their own.  The decode engine uses it when MINIVIDEO_PLACED=1. */
MVHP_EXPORT int  mvhp_placed_alloc_sets(int device, int sets, int count, const size_t *bytes, const uint8_t *any_group,
                                        size_t arena_bytes, void **d_ptrs, void **arena, int *groups_of, int *groups_found);
MVHP_EXPORT void mvhp_placed_free(void *arena);

#ifdef __cplusplus
}
#endif
#endif /* MINIVIDEO_HOTPATH_H */
