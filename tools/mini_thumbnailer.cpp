// tools/mini_thumbnailer.cpp -- a small thumbnailer CLI over libminivideo's public API with the
// same options as the reference's mini_thumbnailer (mini_thumbnailer/src/main.cpp:47-302):
//   -i <file> [-o <dir>] [-f jpg|png|bmp|tga|yuv420|yuv444] [-q 1..99] [-n 1..999] [-e unfiltered|ordered|distributed]
// plus a few of its own, which set the library's opt-in switches (include/minivideo.h) before the decode call:
//   -c            pictures are the SPS's cropped rectangle (MINIVIDEO_CROP=1)
//   -s <w>x<h>    ... fitted into a w x h box, never enlarged (MINIVIDEO_THUMBNAIL=<w>x<h>; implies -c)
//   -r <value>    pictures turned: auto = the MP4's display rotation, or 0 / 90 / 180 / 270 degrees clockwise (MINIVIDEO_ROTATE)
//   -a            square samples: the VUI's sample aspect ratio is applied (MINIVIDEO_ASPECT=1; implies -c)
//   -m <value>    RGB by the stream's own colour description (auto) or bt601 / bt709 / bt601-full / bt709-full (MINIVIDEO_COLOR)
// The stock mini_thumbnailer also builds unchanged against include/minivideo.h; this file exists so
// that the GPU box (which has no copy of the reference) has a CLI to run.
#include <minivideo.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unistd.h>

// MINIVIDEO_STATS=1: where a run's wall time goes, seen from the process (the library prints its own account of the calls)
static double g_t0;
static bool g_stats;
static double since_start()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() - g_t0;
}
static void mark(const char *what)
{
    if (g_stats) fprintf(stderr, "[mini_thumbnailer] %.3f s: %s\n", since_start(), what);
}

int main(int argc, char *argv[])
{
    g_t0 = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    g_stats = getenv("MINIVIDEO_STATS") != nullptr;
    atexit([] { mark("last exit handler (registered first: everything the runtimes tear down at exit is over)"); });
    const char *in = nullptr, *outdir = nullptr;
    int fmt = PICTURE_JPG, quality = 75, number = 1, mode = PICTURE_UNFILTERED;
    bool help = false;
    for (int i = 1; i < argc; i++) {
        const bool has = i + 1 < argc;
        if (!strcmp(argv[i], "-i") && has) in = argv[++i];
        else if (!strcmp(argv[i], "-o") && has) outdir = argv[++i];
        else if (!strcmp(argv[i], "-f") && has) {
            const char *f = argv[++i];
            if (!strcmp(f, "jpg")) fmt = PICTURE_JPG;
            else if (!strcmp(f, "png")) fmt = PICTURE_PNG;
            else if (!strcmp(f, "bmp")) fmt = PICTURE_BMP;
            else if (!strcmp(f, "tga")) fmt = PICTURE_TGA;
            else if (!strcmp(f, "yuv420")) fmt = PICTURE_YUV420;
            else if (!strcmp(f, "yuv444")) fmt = PICTURE_YUV444;
            else fprintf(stderr, "-f : No valid picture format specified\n");
        } else if (!strcmp(argv[i], "-q") && has) {
            const int q = atoi(argv[++i]);
            if (q > 0 && q < 100) quality = q;
        } else if (!strcmp(argv[i], "-n") && has) {
            const int n = atoi(argv[++i]);
            if (n > 0 && n < 1000) number = n;
        } else if (!strcmp(argv[i], "-e") && has) {
            const char *e = argv[++i];
            if (!strcmp(e, "unfiltered")) mode = PICTURE_UNFILTERED;
            else if (!strcmp(e, "ordered")) mode = PICTURE_ORDERED;
            else if (!strcmp(e, "distributed")) mode = PICTURE_DISTRIBUTED;
            else fprintf(stderr, "-e : No valid extraction mode specified\n");
        } else if (!strcmp(argv[i], "-c")) setenv("MINIVIDEO_CROP", "1", 1);
        else if (!strcmp(argv[i], "-s") && has) setenv("MINIVIDEO_THUMBNAIL", argv[++i], 1);   // (the library checks the value)
        else if (!strcmp(argv[i], "-r") && has) setenv("MINIVIDEO_ROTATE", argv[++i], 1);      // (the library checks the value)
        else if (!strcmp(argv[i], "-a")) setenv("MINIVIDEO_ASPECT", "1", 1);
        else if (!strcmp(argv[i], "-m") && has) setenv("MINIVIDEO_COLOR", argv[++i], 1);       // (the library checks the value)
        else if (!strcmp(argv[i], "-j")) setenv("MINIVIDEO_JPEG", "1", 1);   // -f jpg writes JPEG files (made on the GPU), not the PNG fallback
        else if (!strcmp(argv[i], "-z")) setenv("MINIVIDEO_PNG", "1", 1);    // PNG files are compressed, and made on the GPU
        else if (!strcmp(argv[i], "-b")) setenv("MINIVIDEO_SKIP_BLANK", "1", 1);   // blank pictures (black, faded, flat) give way to later ones
        else if (!strcmp(argv[i], "-t")) setenv("MINIVIDEO_TRIM", "1", 1);         // black bars (letterbox, pillarbox) are trimmed off every picture
        else if (!strcmp(argv[i], "-p")) setenv("MINIVIDEO_REPRESENTATIVE", "1", 1);   // each file holds the picture that looks most like its neighbours
        else if (!strcmp(argv[i], "-h") || !strcmp(argv[i], "--help")) help = true;
        else fprintf(stderr, "* Unknown argument '%s'\n", argv[i]);
    }
    if (!in || help) {
        printf("* Usage:\nmini_thumbnailer -i <filepath> [-o <directory>] [-f picture_format][-q picture_quality]"
               "[-n picture_number] [-e extraction_mode] [-c] [-s <width>x<height>] [-r auto|0|90|180|270] [-a] [-m auto|bt601|bt709|bt601-full|bt709-full] [-j] [-z] [-b] [-t] [-p]\n"
               "-z : PNG files (-f png, and -f jpg without -j) are compressed, and made on the GPU (MINIVIDEO_PNG=1)\n"
               "-b : skip blank pictures (MINIVIDEO_SKIP_BLANK=1; MINIVIDEO_BLANK_VARIANCE=<0..16256, default 256>, "
               "MINIVIDEO_BLANK_ALTERNATES=<1..16, default 4>)\n"
               "-t : trim black bars (MINIVIDEO_TRIM=1; MINIVIDEO_TRIM_LEVEL=<1..254, default 24>, "
               "MINIVIDEO_TRIM_PROBES=<1..64, default 8>)\n"
               "-p : representative pictures: each file holds, of its picture and the IDR pictures that follow it, the one nearest "
               "their mean histogram (MINIVIDEO_REPRESENTATIVE=1; MINIVIDEO_REPRESENTATIVE_ALTERNATES=<1..16, default 8>)\n");
        return EXIT_FAILURE;
    }
    mark("main, arguments read");
    minivideo_print_infos();
    mark("minivideo_print_infos returned");
    minivideo_endianness();
    MediaFile_t *media = nullptr;
    int rc = minivideo_open(in, &media);
    int decode_rc = FAILURE;
    if (rc == SUCCESS) {
        rc = minivideo_parse(media, false, true, false);
        mark("minivideo_parse returned");
        if (rc == SUCCESS) decode_rc = minivideo_decode(media, outdir, fmt, quality, number, mode);
        mark("minivideo_decode returned");
        rc = minivideo_close(&media);
    }
    mark("minivideo_close returned; leaving main");
    // like the reference, the exit status reflects minivideo_close (main.cpp:285-298); the decode status
    // is reported on stderr so that scripts can still see it
    if (decode_rc != SUCCESS) fprintf(stderr, "mini_thumbnailer: decode did not succeed (rc=%d)\n", decode_rc);
    // Every file is written and closed, the engine is gone: what is left is the HIP / HSA runtimes' own teardown at exit
    // (finalizers behind the exit handlers: 0.05-0.1 s, a third of a one-thumbnail run, tools/startup_probe.sh).  A CLI that
    // has nothing more to do leaves without it; MINIVIDEO_FULL_EXIT=1 keeps the ordinary exit (leak checkers).
    if (!getenv("MINIVIDEO_FULL_EXIT")) {
        mark("leaving with _exit");
        fflush(stdout);
        fflush(stderr);
        _exit(rc == SUCCESS ? EXIT_SUCCESS : EXIT_FAILURE);
    }
    return rc == SUCCESS ? EXIT_SUCCESS : EXIT_FAILURE;
}
