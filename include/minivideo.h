/*
 * minivideo.h -- public API of libminivideo.so (MI355X-native build).
 *
 * Drop-in for the reference's public header set (minivideo/src/minivideo.h:59-149
 * plus what it pulls in: typedef.h:40-42 return codes, avcodecs.h:33-66,180-199
 * container / picture enums, avutils.h:32-60,143-149 stream / sample /
 * repartition enums, bitstream_map_struct.h:46-129 and mediafile_struct.h:39-73
 * public structs).  The stock mini_thumbnailer (mini_thumbnailer/src/main.cpp)
 * compiles and links against this header and library unchanged.
 *
 * Behavioural contract kept from the reference:
 *   - return codes SUCCESS = 1, FAILURE = 0, UNSUPPORTED = -1 (typedef.h:40-42);
 *   - minivideo_decode() writes <input basename>[_k].<ext> into the CURRENT WORKING
 *     DIRECTORY and ignores output_directory (export.c:627-642,704-708, h264.c:65);
 *   - no deblocking filter is applied by default; the picture is the uncropped coded size
 *     (opt-in, outside the reference's behaviour: MINIVIDEO_DEBLOCK=1 in the environment applies the standard's in-loop
 *     deblocking filter, clause 8.7, to Annex-B and MP4 input alike; independent of MINIVIDEO_SPEC=1);
 *   - opt-in, outside the reference's behaviour and independent of the two switches above: MINIVIDEO_CROP=1 writes the SPS's
 *     cropped rectangle instead of the coded size (1920x1080 instead of 1920x1088), MINIVIDEO_THUMBNAIL=<w>x<h> writes the
 *     cropped picture fitted into a w x h box (aspect kept, even sides, never enlarged; it implies the crop; both sides 2 ...
 *     65535), made on the GPU.  Every format is written at that size, file names do not change, Annex-B and MP4 input behave
 *     alike.  A malformed MINIVIDEO_THUMBNAIL ("abc", "0x10", "320", a side below 2) is not ignored: minivideo_decode()
 *     returns FAILURE with a message before any device work.  A picture whose crop leaves nothing is skipped like a picture
 *     that does not decode;
 *   - opt-in, outside the reference's behaviour (which reads an MP4 track's display matrix, traces it and drops it,
 *     demuxer/mp4/mp4.c:1167-1197) and independent of the switches above: MINIVIDEO_ROTATE=auto|0|90|180|270 turns the
 *     pictures on the GPU before they are written.  "auto" applies the rotation of the MP4 video track's tkhd matrix when it
 *     is a pure quarter-turn rotation (a phone's portrait clip comes out upright; mirrored, scaled or sheared matrices and
 *     Annex-B input: no turn), an angle turns by that many degrees clockwise whatever the file says.  Every format is written
 *     at the turned size (1080 x 1920 for a 90-degree 1920 x 1080 clip), a MINIVIDEO_THUMBNAIL box is the box of the turned
 *     picture, file names do not change; 0, the empty string and a rotation that comes to 0 are the files without the switch.
 *     Any other value ("45", "90x") is not ignored: minivideo_decode() returns FAILURE with a message before any device work;
 *   - opt-in, outside the reference's behaviour (which parses the SPS's VUI and only traces it, h264_parameterset.c:1318-1350)
 *     and independent of the switches above: MINIVIDEO_ASPECT=1 applies the VUI's sample aspect ratio -- the pictures are
 *     written with square samples, one axis of the cropped picture shrunk on the GPU (1440 x 1080 at SAR 4:3: 1440 x 810; implies
 *     MINIVIDEO_CROP; a MINIVIDEO_THUMBNAIL box is fitted to that size); MINIVIDEO_COLOR=auto|bt601|bt709|bt601-full|bt709-full
 *     makes the RGB formats (png, bmp, tga, also compressed PNG) from the final planes by the stream's own matrix, range and
 *     chroma siting ("auto": matrix_coefficients 1 = BT.709, 5 / 6 = BT.601, otherwise by size; video_full_range_flag;
 *     chroma_sample_loc_type) or by the named matrix and range, instead of the reference's BT.601 limited-range formula; yuv and
 *     jpg files are not touched.  0 and the empty string are the files without the switch; any other value is not ignored:
 *     minivideo_decode() returns FAILURE with a message before any device work;
 *   - PICTURE_JPG is written as PNG, as a reference built without libjpeg does (export.c:644-690).  Opt-in, outside the
 *     reference's behaviour and independent of the switches above: with MINIVIDEO_JPEG=1 PICTURE_JPG writes <name>[_k].jpg,
 *     baseline JFIF files coded on the GPU from the 4:2:0 planes as export.c:341-430 does with libjpeg (2x2 / 1x1 / 1x1
 *     sampling, no colour conversion), at picture_quality (clamped to 1 ... 100; otherwise this argument is unused), of the
 *     coded size or of the size MINIVIDEO_CROP / MINIVIDEO_THUMBNAIL ask for.  The other formats are not affected;
 *   - opt-in, outside the reference's behaviour: with MINIVIDEO_PNG=1 every PNG file (PICTURE_PNG, and PICTURE_JPG without
 *     MINIVIDEO_JPEG) is a compressed PNG -- row filters and Huffman-only deflate -- coded on the GPU from the picture's RGB
 *     instead of the stored-deflate file of the host writer: the same names, the same pixels, about half the bytes on camera
 *     content, and only the files' bytes are downloaded.  It composes with every switch above and below;
 *   - opt-in, outside the reference's behaviour and independent of the switches above: MINIVIDEO_SKIP_BLANK=1 replaces blank
 *     pictures -- black lead-ins, fades, flat title cards -- by later ones.  Every decoded picture gets a score on the GPU,
 *     the variance of its luma samples (of the SPS's cropped rectangle under MINIVIDEO_CROP / MINIVIDEO_THUMBNAIL, else of the
 *     coded picture) in sixteenths, and is blank when the score is below 16 x MINIVIDEO_BLANK_VARIANCE (an integer 0 ...
 *     16256, default 256).  First every picture is written as without the switch, under the same names.  Then, for each file
 *     whose picture is blank, up to MINIVIDEO_BLANK_ALTERNATES (1 ... 16, default 4) of the IDR pictures between it and the
 *     next selected picture (to the end of the stream behind the last one) are decoded in stream order, and the file is
 *     written again with the first of them that is not blank or, if there is none, with the highest-scoring of them all, the
 *     original included (the earliest on a tie).  A replacement is written to <name>.part and renamed over the file: if that
 *     write fails, the file keeps the picture it had.  The number of files, their names, the return value and picture_number mean
 *     what they mean without the switch, and the files do not depend on batch sizes, threads or devices.  A malformed value
 *     of any of the three variables is not ignored: minivideo_decode() returns FAILURE with a message before any device work;
 *   - opt-in, outside the reference's behaviour (which writes the coded picture, bars and all) and independent of the switches
 *     above: MINIVIDEO_TRIM=1 trims the black bars of a letterboxed or pillarboxed stream off every picture (implies
 *     MINIVIDEO_CROP).  Bars are a property of the stream, not of a picture -- a dark scene has no edge, and pictures of
 *     differing sizes are of no use -- so up to MINIVIDEO_TRIM_PROBES (1 ... 64, default 8) of the selected pictures, spread evenly
 *     over the selection and the first among them, are decoded first and measured on the GPU: a luma sample is bright above
 *     MINIVIDEO_TRIM_LEVEL (1 ... 254, default 24: video black plus noise), a row or column of the SPS's cropped rectangle is
 *     content when at least 1/32 of its samples (at least one) are bright, and a picture's box spans its first to its last
 *     content row and column (a subtitle burnt into a bar keeps its rows).  The union of the probes' boxes, its edges moved
 *     outward to even, replaces the cropped rectangle of EVERY picture -- unless less than half of the width or of the height
 *     would be left (a dark scene, not a bar) or no probe shows content: then, and for a picture of another size in
 *     mid-stream, the files are exactly those of MINIVIDEO_CROP=1.  Everything else starts from the trimmed rectangle: a
 *     MINIVIDEO_THUMBNAIL box is fitted to it, MINIVIDEO_ASPECT and MINIVIDEO_ROTATE apply to it, the score of
 *     MINIVIDEO_SKIP_BLANK is taken over it.  The number of files, their names, the return value and picture_number mean what
 *     they mean without the switch, Annex-B and MP4 input behave alike, and the files do not depend on batch sizes, threads or
 *     devices.  Cost: the probes are entropy-decoded twice, at most MINIVIDEO_TRIM_PROBES pictures per call.  0 and the empty
 *     string for MINIVIDEO_TRIM are the files without the switch; a malformed value of any of the three variables is not
 *     ignored: minivideo_decode() returns FAILURE with a message before any device work;
 *   - opt-in, outside the reference's behaviour and independent of the switches above: MINIVIDEO_REPRESENTATIVE=1 lets every
 *     file hold a representative picture instead of whatever IDR picture the selection lands on (a title card, a flash
 *     frame).  First every picture is written as without the switch, under the same names, and the GPU counts the histograms
 *     of its luma and chroma samples (of the SPS's cropped rectangle where a switch above crops, else of the coded picture).
 *     Then up to MINIVIDEO_REPRESENTATIVE_ALTERNATES (1 ... 16, default 8) of the IDR pictures between each file's picture
 *     and the next selected one (to the end of the stream behind the last one) are decoded for their histograms alone, and
 *     each file's candidates -- its picture first, then its alternates in stream order, those of another size left out --
 *     are compared: the one nearest the candidates' mean histogram wins (sum over the 768 bins of the three planes of the
 *     squared difference, in integers; the earliest on a tie, so one or two candidates keep the file as it is).  Last, the
 *     winners that are not already in their files are decoded once more with all the switches of the call, written to
 *     <name>.part and renamed over the files: if that write fails, the file keeps the picture it had.  With
 *     MINIVIDEO_SKIP_BLANK=1 as well the two run as one: only candidates that are not blank (the score is taken from the
 *     histogram, the threshold is MINIVIDEO_BLANK_VARIANCE) are compared, a file whose candidates are all blank gets the
 *     highest-scoring one, and MINIVIDEO_BLANK_ALTERNATES is not read.  The number of files, their names, the return value
 *     and picture_number mean what they mean without the switch, and the files do not depend on batch sizes, threads or
 *     devices.  Cost: every alternate is entropy-decoded and reconstructed, up to MINIVIDEO_REPRESENTATIVE_ALTERNATES + 1
 *     times the work per file.  A malformed value of either variable is not ignored: minivideo_decode() returns FAILURE with
 *     a message before any device work;
 *   - H.264 IDR pictures only, from Annex-B elementary streams (.264/.h264 or a
 *     file starting with an SPS start code) or from the first H.264 video track
 *     of an MP4/MOV file (demuxer/mp4/mp4.c:1950 mp4_fileParse -> sync samples).
 *   - minivideo_decode() returns SUCCESS when at least one picture file was written and none of the wanted ones is missing
 *     because a WRITE failed (files are written by a pool of threads behind the decode pipeline; after the first failed
 *     write -- a full disk -- decoding stops and the call returns FAILURE; the synchronous path used for fewer than four
 *     pictures decodes a replacement picture instead, like the reference's loop h264.c:173-179);
 * Differences: reconstruction runs on HIP devices (there is no CPU
 * reconstruction path: without a GPU minivideo_decode() returns FAILURE);
 * invalid streams return FAILURE instead of calling exit().
 */
#ifndef MINIVIDEO_H
#define MINIVIDEO_H

#include <stdint.h>
#include <stdio.h>
#ifndef __cplusplus
#include <stdbool.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define minivideo_EXPORT __attribute__((visibility("default")))

#define minivideo_VERSION_MAJOR 0
#define minivideo_VERSION_MINOR 8
#define minivideo_VERSION_PATCH 0

/* Custom return codes (typedef.h:40-42) */
#define UNSUPPORTED (-1)
#define FAILURE       0
#define SUCCESS       1

/* minivideo.h:42-52 (names and values kept; no function of the reference returns them: callers test == SUCCESS) */
typedef enum MiniVideoErrorCodes_e {
    ERROR_UNKNOWN           = 1,

    ERROR_CONTAINER_UNKNOWN = 10,
    ERROR_CONTAINER_FAILURE = 11,

    ERROR_CODEC_UNKNOWN     = 20,
    ERROR_CODEC_FAILURE     = 21
} MiniVideoErrorCodes_e;

/* avcodecs.h:33-66 (values kept) */
typedef enum ContainerFormat_e {
    CONTAINER_UNKNOWN = 0,
    CONTAINER_AVI = 1,
    CONTAINER_ASF = 2,
    CONTAINER_MKV = 3,
    CONTAINER_MP4 = 4,
    CONTAINER_MPEG_PS = 5,
    CONTAINER_MPEG_TS = 6,
    CONTAINER_MPEG_MT = 7,
    CONTAINER_MXF = 8,
    CONTAINER_FLV = 9,
    CONTAINER_OGG = 10,
    CONTAINER_RM = 11,
    CONTAINER_FLAC = 12,
    CONTAINER_WAVE = 13,
    CONTAINER_ES = 16,
    CONTAINER_ES_AAC = 17,
    CONTAINER_ES_AC3 = 18,
    CONTAINER_ES_MP3 = 19
} ContainerFormat_e;

/* avcodecs.h:66-178: only the members this library can report */
typedef enum AVCodec_e {
    CODEC_UNKNOWN = 0,
    CODEC_H264 = 262
} AVCodec_e;

/* avcodecs.h:180-193 */
typedef enum PictureFormat_e {
    PICTURE_UNKNOWN = 0,
    PICTURE_BMP = 1,
    PICTURE_JPG = 2,
    PICTURE_PNG = 3,
    PICTURE_WEBP = 4,
    PICTURE_TGA = 5,
    PICTURE_YUV444 = 16,
    PICTURE_YUV420 = 17
} PictureFormat_e;

/* avutils.h:32-44 */
typedef enum StreamType_e {
    stream_UNKNOWN = 0,
    stream_AUDIO = 1,
    stream_VIDEO = 2,
    stream_TEXT = 3,
    stream_MENU = 4,
    stream_TMCD = 5,
    stream_META = 6,
    stream_HINT = 7
} StreamType_e;

/* avutils.h:48-64 */
typedef enum SampleType_e {
    sample_UNKNOWN = 0,
    sample_AUDIO,
    sample_AUDIO_TAG,
    sample_VIDEO,
    sample_VIDEO_SYNC,
    sample_VIDEO_PARAM,
    sample_TEXT,
    sample_TEXT_FILE,
    sample_OTHER
} SampleType_e;

/* avutils.h:143-149 */
typedef enum PictureRepartition_e {
    PICTURE_UNFILTERED = 0,
    PICTURE_ORDERED = 1,
    PICTURE_DISTRIBUTED = 2
} PictureRepartition_e;

/* bitstream_map_struct.h:46-129 -- field order and types kept (public struct) */
typedef struct BitstreamMap_t {
    StreamType_e stream_type;
    uint64_t stream_size;
    uint32_t stream_fcc;
    AVCodec_e stream_codec;
    bool stream_intracoded;
    char *stream_encoder;

    unsigned int track_id;
    char *track_title;
    char *track_languagecode;
    bool track_default;
    bool track_forced;

    unsigned int bitrate;
    unsigned int bitrate_mode;
    unsigned int bitrate_min;
    unsigned int bitrate_max;

    unsigned int duration_ms;
    unsigned int creation_time;
    unsigned int modification_time;

    unsigned int width;
    unsigned int height;
    unsigned int visible_width;
    unsigned int visible_height;
    unsigned int color_depth;
    unsigned int color_subsampling;
    unsigned int color_encoding;
    unsigned int color_matrix;
    unsigned int color_range;

    double display_aspect_ratio;
    unsigned int display_aspect_ratio_h;
    unsigned int display_aspect_ratio_v;
    double video_aspect_ratio;
    unsigned int video_aspect_ratio_h;
    unsigned int video_aspect_ratio_v;
    double pixel_aspect_ratio;
    unsigned int pixel_aspect_ratio_h;
    unsigned int pixel_aspect_ratio_v;

    double framerate;
    double framerate_num;
    double framerate_base;
    double frame_duration;
    unsigned int framerate_mode;

    unsigned int channel_count;
    unsigned int channel_mode;
    unsigned int sampling_rate;
    unsigned int bit_per_sample;
    unsigned int sample_per_frames;
    unsigned int pcm_sample_size;
    unsigned int pcm_sample_format;
    unsigned int pcm_sample_endianness;

    char *subtitles_name;
    unsigned int subtitles_encoding;

    bool sample_alignment;
    uint32_t sample_count;
    uint32_t frame_count;
    uint32_t frame_count_idr;

    uint32_t *sample_type;
    uint32_t *sample_size;
    int64_t *sample_offset;
    int64_t *sample_pts;
    int64_t *sample_dts;
} BitstreamMap_t;

/* mediafile_struct.h:39-73 -- field order and types kept (public struct) */
typedef struct MediaFile_t {
    FILE *file_pointer;

    int64_t file_size;
    char file_path[4096];
    char file_directory[4096];
    char file_name[255];
    char file_extension[255];
    unsigned int file_creation_time;
    unsigned int file_modification_time;

    char *creation_app;
    unsigned int creation_time;
    unsigned int modification_time;
    unsigned int duration;

    ContainerFormat_e container;

    unsigned int tracks_audio_count;
    BitstreamMap_t *tracks_audio[16];
    unsigned int tracks_video_count;
    BitstreamMap_t *tracks_video[16];
    unsigned int tracks_subtitles_count;
    BitstreamMap_t *tracks_subt[16];
    unsigned int tracks_others_count;
    BitstreamMap_t *tracks_others[16];
} MediaFile_t;

/* minivideo.h:59-149 */
minivideo_EXPORT void minivideo_print_infos(void);
minivideo_EXPORT void minivideo_get_infos(int *minivideo_major, int *minivideo_minor, int *minivideo_patch,
                                          const char **minivideo_builddate, const char **minivideo_buildtime);
minivideo_EXPORT int minivideo_endianness(void);
minivideo_EXPORT int minivideo_open(const char *input_filepath, MediaFile_t **input_media);
minivideo_EXPORT int minivideo_parse(MediaFile_t *input_media, const bool extract_audio, const bool extract_video,
                                     const bool extract_subtitles);
minivideo_EXPORT int minivideo_decode(MediaFile_t *input_media, const char *output_directory, const int picture_format,
                                      const int picture_quality, const int picture_number,
                                      const int picture_extractionmode);
minivideo_EXPORT int minivideo_extract(MediaFile_t *input_media, const char *output_directory, const bool extract_audio,
                                       const bool extract_video, const bool extract_subtitles, const int output_format);
minivideo_EXPORT int minivideo_close(MediaFile_t **input_media);

/* avcodecs.h:197-199, fourcc.h:240 */
minivideo_EXPORT const char *getContainerString(ContainerFormat_e container, bool long_description);
minivideo_EXPORT const char *getCodecString(StreamType_e type, AVCodec_e codec, bool long_description);
minivideo_EXPORT const char *getPictureString(PictureFormat_e picture, bool long_description);
minivideo_EXPORT AVCodec_e getCodecFromFourCC(const uint32_t fcc);

#ifdef __cplusplus
}
#endif
#endif /* MINIVIDEO_H */
