// launch_plan.h -- which kernel form a reconstruction launch runs on, and with how many waves: pure host arithmetic on the
// device's size, the forced settings, the stream parameters and the batch size (no HIP call, no context).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "minivideo_hotpath.h"
#include "recon_kernels.h"

namespace mvhp {

struct PlanDevice {
    int    n_cus;
    size_t max_lds;   // LDS bytes a workgroup may use
    int    layout;    // forced MVHP_LAYOUT_*, 0 = auto
    int    waves;     // forced waves per workgroup / rows per band, 0 = auto
};

struct LaunchPlan {
    int      layout, waves;
    uint32_t tickets;      // workgroups of a banded launch (each takes one ticket); 0 for the unbanded forms
    size_t   seam_bytes;   // seam granules a banded launch needs; 0 for the unbanded forms
};

// What the host knows about a kernel form: kernel_form(MVHP_LAYOUT_ROWS .. MVHP_LAYOUT_PIPE1), one table in launch_plan.hip.
struct KernelForm {
    const char *name;                               // MINIVIDEO_LAYOUT=<name>
    int         pictures;                           // per workgroup (banded: per group of workgroups): 1, 4 or 8
    bool        banded;                             // a picture's rows in bands over several workgroups (tickets, seams)
    size_t    (*lds_bytes)(int width_mbs, int nw);  // LDS of a workgroup of nw waves (pipe forms: nw rows of three waves)
    int         built[5];                           // the nw the kernel is instantiated for, largest first, 0 = end
    size_t      max_mbs;                            // macroblocks per picture its 32-bit offsets reach, 0 = no cap
    int         fallback;                           // the form that takes a picture this one cannot, MVHP_LAYOUT_AUTO = none
    hipError_t (*launch)(const ReconArgs &a, int nw, hipStream_t stream);

    int smallest() const { int k = 0; while (k < 4 && built[k + 1]) k++; return built[k]; }
};
const KernelForm &kernel_form(int layout);

LaunchPlan plan_launch(const PlanDevice &dev, const mvhp_stream_params_t &p, int n_frames);

} // namespace mvhp
