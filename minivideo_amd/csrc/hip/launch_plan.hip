// launch_plan.hip -- which kernel form a reconstruction launch runs on and with how many waves (launch_plan.h).
#include <math.h>

#include "launch_plan.h"

namespace mvhp {

// Everything the host knows about a kernel form, in one place.  (MVHP_LAYOUT_AUTO is no form: its entry is empty.)
const KernelForm &kernel_form(int layout)
{
    static const KernelForm forms[MVHP_LAYOUT_COUNT] = {
        // name       pictures banded LDS cost          built for (waves; banded: rows per band)  cap  falls back to   launcher
        {"auto",      0, false, nullptr,               {0},               0,               MVHP_LAYOUT_AUTO,      nullptr},
        {"rows",      1, false, recon_lds_bytes,       {16, 8, 4},        0,               MVHP_LAYOUT_AUTO,      launch_recon},
        {"quad",      4, false, recon_quad_lds_bytes,  {16, 12, 8, 6, 4}, 0,               MVHP_LAYOUT_ROWS,      launch_recon_quad},
        {"oct",       8, false, recon_oct_lds_bytes,   {8, 6, 4},         (size_t)1 << 19, MVHP_LAYOUT_QUAD,      launch_recon_oct},
        {"wide",      1, true,  recon_lds_bytes,       {4},               0,               MVHP_LAYOUT_AUTO,      launch_recon_wide},
        {"quad_wide", 4, true,  recon_quad_lds_bytes,  {8, 4},            (size_t)1 << 20, MVHP_LAYOUT_WIDE,      launch_recon_quad_wide},
        {"pipe",      4, true,  recon_pipe_lds_bytes,  {4, 2, 1},         (size_t)1 << 20, MVHP_LAYOUT_QUAD_WIDE, launch_recon_pipe},
        {"pipe1",     1, true,  recon_pipe1_lds_bytes, {4, 2, 1},         0,               MVHP_LAYOUT_WIDE,      launch_recon_pipe1},
    };
    return forms[layout];
}

static bool fits(const PlanDevice &dev, int layout, const mvhp_stream_params_t *p, int nw)
{
    return kernel_form(layout).lds_bytes((int)p->width_mbs, nw) <= dev.max_lds;
}

// Which kernel form a batch runs on: speed only, results identical.
//   Few pictures: ONE picture (one group of four) spread over several workgroups, bands of four macroblock rows each
//   ("wide" forms: SURVEY 7 step 5's "grid = F x PicHeightInMbs wavefronts"); many pictures: one workgroup per group of
//   four / eight.  Measured on 1080p (tools/layout_crossover.py, profiles/r04l_crossover_{base,high}.log; ms per launch):
//     Baseline      1      4     16     64    128    256    512    768   1024
//     rows        2.45   2.47   2.49   2.53   2.55   2.58   5.00     -    8.86    one workgroup per picture (rounds 1-3)
//     quad        2.73   3.69   3.69   3.71   3.71   3.75   3.96   4.27   4.72    ... per four pictures
//     wide        1.00   1.00   1.01   1.21   1.50   2.34   4.16   6.06   8.00    one picture in 17 bands
//     quad_wide   1.05   1.38   1.38   1.43   1.61   1.93   2.80   3.89   5.05    four pictures in 17 bands
//     pipe        0.59   0.78   0.79   0.95   1.23   1.88   3.28   4.72   6.27    ... three waves per row: residuals / luma / chroma + output
//     pipe1       0.64   0.64   0.65   0.92   1.44   2.61   5.01     -      -     one picture per wavefront, three waves per row
//     High        1      4     16     64    128    256    512    768   1024
//     wide        1.03   1.04   1.05   1.30   1.62   2.50   4.46   6.49   8.57
//     quad_wide   1.18   1.91   1.91   1.99   2.20   2.61   3.70   5.12   6.47    (the four pictures of a wavefront run their
//     pipe        0.67   1.18   1.19   1.41   1.85   2.72   4.69     -      -      three luma paths one after the other)
//     pipe1       0.60   0.60   0.63   0.93   1.50   2.74   5.31     -      -
//     quad        3.03   5.17   5.17   5.20   5.20   5.21   5.24   5.34   5.60
//   ONE Baseline picture: the quarters of a wavefront hold the same picture (no divergence): pipe (0.57 against pipe1's 0.65 ms;
//   at three pictures 0.73 against 0.65).  pipe1 has no lock
//   step at all and its Intra4x4 chain takes ten dependent steps instead of sixteen, but needs three resident waves per ROW.
//   720p and 2160p: profiles/r04l_crossover_{high720,base2160,high2160,high2160b}.log.  Small batches with slices / scaling
//   matrices: pipe1 (it reconstructs them as the one-picture kernel does), larger ones wide.
static int pick_layout(const PlanDevice &dev, const mvhp_stream_params_t *p, int n_frames)
{
    int layout = dev.layout;
    // pictures of several slices and scaling matrices (MVHP_STREAM_SPEC streams): the one-picture kernel,
    // where a neighbour's availability is a per-wavefront scalar and LevelScale is a table in LDS -- whatever was asked for;
    // in bands at every batch size (2.44 against 2.58 ms at 256 pictures, 8.5 against 8.9 at 1024) unless "rows" is forced
    const bool pipe1_fits = fits(dev, MVHP_LAYOUT_PIPE1, p, 1);
    if (p->flags & (MVHP_PARAM_SLICES | MVHP_PARAM_SCALING)) {
        if (layout == MVHP_LAYOUT_ROWS || layout == MVHP_LAYOUT_WIDE) return layout;
        if (layout == MVHP_LAYOUT_PIPE1) return pipe1_fits ? MVHP_LAYOUT_PIPE1 : MVHP_LAYOUT_WIDE;
        return (pipe1_fits && (double)n_frames * (double)p->height_mbs <= 40.0 * dev.n_cus) ? MVHP_LAYOUT_PIPE1 : MVHP_LAYOUT_WIDE;
    }
    if (layout == MVHP_LAYOUT_AUTO) {
        const double cus = (double)dev.n_cus;
        const double row_waves = (double)n_frames * (double)p->height_mbs;
        const bool may8 = (p->flags & MVHP_PARAM_MAY_HAVE_8X8) != 0;
        const bool pipe_fits = fits(dev, MVHP_LAYOUT_PIPE, p, 1);
        // round 4, after the wave priorities went in (profiles/r04l_crossover_*.log: 720p, 1080p and 2160p, both profiles): what
        // decides between the one-picture forms is ROW-WAVES (three waves per row have to be resident), what decides between the
        // four-picture forms is PICTURES (a round of the unbanded kernel is 4 x CUs pictures whatever their size):
        //   Baseline  pipe (1 picture) | pipe1 up to 18 x CUs row-waves | pipe up to 76 x CUs row-waves (rows of 240: 1.15 x CUs pictures) | quad_wide | round model
        //   High                       pipe1 up to 46 (rows of > 160 macroblocks: 40) x CUs row-waves | wide up to 76 x CUs row-waves (rows of 240: 1.2 x CUs pictures) | quad_wide | round model
        // quad_wide against a first round of quad: 0.84 x 4 x CUs pictures at 120 macroblocks per row (720p: 0.80), 0.65 at 240
        const double wide_rows = fmax(0.0, ((double)p->width_mbs - 120.0) / 120.0);   // 0 at 1080p, 1 at 2160p
        const double qw_share = fmin(0.84, fmax(0.60, 0.84 - (may8 ? 0.19 : 0.06) * wide_rows));
        // four pictures per wavefront in bands against the forms below them: 76 x CUs row-waves on rows of up to 160 macroblocks
        // (720p: 450 pictures, 1080p: 300), at most 2 x CUs pictures; on longer rows 1.15 / 1.2 x CUs pictures (r04r_grid*.log)
        const bool below_qw = (p->width_mbs <= 160) ? (row_waves <= 76.0 * cus && n_frames <= 2.0 * cus) : (n_frames <= (may8 ? 1.2 : 1.15) * cus);
        if (pipe_fits && !may8 && n_frames <= 1) {
            layout = MVHP_LAYOUT_PIPE;
        } else if (pipe1_fits && row_waves <= (may8 ? (p->width_mbs <= 160 ? 46.0 : 40.0) : 18.0) * cus) {
            layout = MVHP_LAYOUT_PIPE1;
        } else if (pipe_fits && !may8 && below_qw) {
            layout = MVHP_LAYOUT_PIPE;
        } else if (may8 ? below_qw : (!pipe_fits && row_waves <= 34.0 * cus)) {
            layout = MVHP_LAYOUT_WIDE;
        } else if (n_frames <= qw_share * 4.0 * cus) {
            layout = MVHP_LAYOUT_QUAD_WIDE;
        } else {
            // A launch is a number of "rounds" of one workgroup per CU (the batch kernels fill a CU with one workgroup), in
            // units of one full round of the four-picture kernel (5.4 ms for 4 * CUs pictures of 1080p): the four-picture
            // kernel 0.77 with one workgroup on the device .. 1.0 with all CUs busy; the eight-picture kernel 1.48 .. 1.85
            // (8 * CUs pictures; round 4, with the priorities: 1.45 .. 1.75).  (1100 pictures: quad 8.5 / oct 7.4 ms, 2048: 8.7 / 7.9, 2560: 13.7 / 16.1.)
            auto rounds = [&](double per_round, double lo, double hi) {
                const double full = floor(n_frames / per_round), rem = n_frames - full * per_round;
                return full * hi + (rem > 0 ? lo + (hi - lo) * rem / per_round : 0.0);
            };
            // (2160p High: one 16-wave workgroup per CU, a partial round costs a whole one: 1300 pictures 40.4 ms = 2 x 20)
            const double t_quad = rounds(4 * cus, (may8 && p->width_mbs > 160) ? 1.0 : 0.77, 1.0);
            const bool oct_fits = fits(dev, MVHP_LAYOUT_OCT, p, 8);   // with six waves it loses to quad
            const double t_oct = oct_fits ? (may8 ? rounds(8 * cus, 1.8, 2.0) : rounds(8 * cus, 1.45, 1.75)) : 1e30;   // (High: 10.3 against 5.3 ms per round)
            // ... and the banded four-picture form, whose time is linear in the pictures (8-row bands at these sizes): between one
            // and two rounds it beats both (1100 x 1080p: 5.15 ms against 8.5 / 7.4; profiles/r04q_crossover_big*.log); per round
            // 1.0 (Baseline) / 1.05 (High) at 120 macroblocks per row, 1.14 / 1.49 at 240
            const double t_qw = (n_frames / (4.0 * cus)) * (may8 ? 1.05 + 0.44 * wide_rows : 1.0 + 0.14 * wide_rows);
            layout = (n_frames > 4 * cus && t_qw < t_quad && t_qw < t_oct) ? MVHP_LAYOUT_QUAD_WIDE : (t_oct < t_quad) ? MVHP_LAYOUT_OCT : MVHP_LAYOUT_QUAD;
        }
    }
    // the batch kernels address a workgroup's pictures with 32-bit offsets and keep one line buffer per picture in LDS: a form
    // whose pictures are too large hands over to the next simpler one (rows and wide end the chains: launch_all() refuses
    // what does not fit there either)
    const size_t mbs = (size_t)p->width_mbs * p->height_mbs;
    for (;;) {
        const KernelForm &f = kernel_form(layout);
        if (f.fallback == MVHP_LAYOUT_AUTO || ((f.max_mbs == 0 || mbs <= f.max_mbs) && fits(dev, layout, p, f.smallest()))) break;
        layout = f.fallback;
    }
    return layout;
}

// waves per workgroup (banded forms: rows per band) when none is forced
static int auto_waves(const PlanDevice &dev, const mvhp_stream_params_t *p, int n_frames, int layout)
{
    switch (layout) {
    case MVHP_LAYOUT_PIPE:
    case MVHP_LAYOUT_PIPE1:
        // rows per band (three wavefronts each), built for 1, 2 and 4: 4 unless asked; the one-picture form at the upper end of its
        // range (more than 0.44 x CUs pictures) packs better with single rows (150 x 1080p High: 1.61 against 1.68 ms; 64: the same;
        // 16: 0.77 against 0.63 -- profiles/r04o_pipe1_rows.log), but not on rows of 240 macroblocks, where a seam per row costs
        // more (75 x 2160p: 3.58 against 3.29 -- profiles/r04q_crossover_pipe1_rows.log)
        return (layout == MVHP_LAYOUT_PIPE1 && n_frames > 0.44 * dev.n_cus && p->width_mbs <= 160) ? 1 : 4;
    case MVHP_LAYOUT_WIDE:
        return 4;   // rows per band (built for 4: the finest grain, 17 bands per 1080p picture)
    case MVHP_LAYOUT_QUAD_WIDE:
        // rows per band, built for 4 and 8: 8-wave workgroups fit two to a CU (LDS) = 16 waves, 4-wave ones three = 12;
        // the finer grain is the faster one on Baseline at every batch size measured (512 x 1080p: 2.83 against 2.95 ms), the
        // coarser one on High from ~1.5 x CUs pictures on (640 pictures: 4.13 against 4.28; profiles/r04o_qw48_*.log)
        return (p->width_mbs <= 160 && (((p->flags & MVHP_PARAM_MAY_HAVE_8X8) && n_frames >= 1.5 * dev.n_cus) || n_frames > 3.4 * dev.n_cus)) ? 8 : 4;   // (rows of 240: 4 everywhere)
    case MVHP_LAYOUT_OCT:
        return 8;   // speed only: built for 4, 6 and 8 waves; one workgroup per CU (LDS)
    case MVHP_LAYOUT_QUAD: {
        // speed only: built for 4, 6, 8, 12 and 16 waves; 8-wave workgroups fit two to a CU (LDS, 128 VGPRs) = 16 waves
        // per CU; when only one workgroup per CU will be resident (few workgroups, or wide pictures whose four line
        // buffers leave LDS for one), it should bring the 16 waves itself
        const int groups = (n_frames + 3) / 4;
        const bool two_fit = 2 * recon_quad_lds_bytes((int)p->width_mbs, 8) <= dev.max_lds;
        return (groups >= 2 * dev.n_cus && two_fit) ? 8 : 16;
    }
    default:
        // speed only (DESIGN.md "waves per picture"): 8-wave workgroups fit three to a CU (LDS) = 24 waves/CU,
        // 16-wave workgroups one to a CU; small batches need the wider workgroup to occupy the chip.
        return (n_frames >= 384) ? 8 : 16;
    }
}

// The largest count the form is built for that is not above what was asked for (or chosen), that fits the LDS and -- one
// workgroup per group of pictures: a wavefront works on every second row at most -- that the picture has rows for; the
// smallest one the form is built for when there is none.
static int pick_waves(const PlanDevice &dev, const mvhp_stream_params_t *p, int n_frames, int layout)
{
    const KernelForm &f = kernel_form(layout);
    const int nw = dev.waves ? dev.waves : auto_waves(dev, p, n_frames, layout);
    for (int k = 0; k < 5 && f.built[k]; k++) {
        const int o = f.built[k];
        if (o > nw) continue;
        if (o > f.smallest() && ((!f.banded && (o + 1) / 2 >= (int)p->height_mbs) || !fits(dev, layout, p, o))) continue;
        return o;
    }
    return f.smallest();
}

LaunchPlan plan_launch(const PlanDevice &dev, const mvhp_stream_params_t &p, int n_frames)
{
    LaunchPlan plan = {};
    plan.layout = pick_layout(dev, &p, n_frames);
    plan.waves = pick_waves(dev, &p, n_frames, plan.layout);
    const KernelForm &f = kernel_form(plan.layout);
    if (f.banded) {   // one workgroup, i.e. one ticket, per (group of pictures, band of `waves` rows)
        const int bands = ((int)p.height_mbs + plan.waves - 1) / plan.waves;
        plan.tickets = (uint32_t)((n_frames + f.pictures - 1) / f.pictures) * (uint32_t)bands;
        plan.seam_bytes = recon_wide_seam_bytes((int)p.width_mbs, (int)p.height_mbs, n_frames, plan.waves);
    }
    return plan;
}

} // namespace mvhp
